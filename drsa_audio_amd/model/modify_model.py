"""Virtual DRSA layers inserted after feature layer ``j`` of a VGG-type CNN.

API mirrors ``cxai.model.modify_model``:

* ``ProjectionModel``  — reference ``cxai/model/modify_model.py:4-60``
* ``SubspaceFilter``   — reference ``cxai/model/modify_model.py:63-72``
* ``Projection``       — reference ``cxai/model/modify_model.py:75-96``  (h = a·U, viewed [b, n, K, d_k])
* ``InvProjection``    — reference ``cxai/model/modify_model.py:99-123`` (a' = h·Uᵀ, back to [b, d, H, W])
* ``MultiProjectionModel``, ``MultiProjection``, ``MultiInvProjection`` — (no reference) the same three layers
  with a table of matrices and a table index per batch row, for batches of mixed classes

These modules carry the layer names the name maps refer to
(``features.projection``, ``features.subspacefilter``, ``features.invprojection``).
The HIP engine (``drsa_audio_amd.engine``) recognises them structurally and runs
the projection forward and the ε/mask/ε relevance backward as fused kernels; the
PyTorch ``forward`` methods below are only the model definition.
"""
from __future__ import annotations

import torch
import torch.nn as nn

__all__ = ["ProjectionModel", "SubspaceFilter", "Projection", "InvProjection",
           "MultiProjectionModel", "MultiProjection", "MultiInvProjection", "stack_projections"]


class SubspaceFilter(nn.Module):
    """Identity; the subspace relevance mask is attached to it by the composite."""

    def forward(self, act_map: torch.Tensor) -> torch.Tensor:
        return act_map


class Projection(nn.Module):
    """a [b, d, H, W] -> h [b, H*W, K, d_k] with h = a_vec · U."""

    def __init__(self, U: torch.Tensor, num_concepts: int) -> None:
        super().__init__()
        self.U = U
        self.num_concepts = int(num_concepts)
        self.d_k = U.size(0) // self.num_concepts

    def forward(self, act_map: torch.Tensor) -> torch.Tensor:
        b, d = act_map.size(0), act_map.size(1)
        vecs = act_map.reshape(b, d, -1).transpose(1, 2)
        h = vecs @ self.U.to(act_map)
        return h.reshape(b, vecs.size(1), self.num_concepts, self.d_k)


class InvProjection(nn.Module):
    """h [b, n, K, d_k] -> a' [b, d, sqrt(n), sqrt(n)] with a' = h · Uᵀ (square maps, as the reference)."""

    def __init__(self, U: torch.Tensor, num_concepts: int) -> None:
        super().__init__()
        self.U_inv = U.T
        self.num_concepts = int(num_concepts)
        self.d = self.U_inv.size(0)
        self.d_k = self.d // self.num_concepts

    def forward(self, h: torch.Tensor) -> torch.Tensor:
        b, n = h.size(0), h.size(1)
        side = int(round(n ** 0.5))
        a = h.reshape(b, n, self.d) @ self.U_inv.to(h)
        return a.transpose(1, 2).reshape(b, self.d, side, side).contiguous()


class ProjectionModel(nn.Module):
    """Copy of ``model`` with Projection -> SubspaceFilter -> InvProjection inserted
    right after ``model.features[layer_idx]``.

    ``case`` selects the flattened width between trunk and head exactly like the
    reference (2048 for 'gtzan', 64 for 'toy'); ``num_flat_features`` may be given
    explicitly for other models.
    """

    def __init__(self, model: nn.Module, layer_idx: int, U: torch.Tensor,
                 num_concepts: int, case: str = "gtzan",
                 num_flat_features: int | None = None) -> None:
        super().__init__()
        n_feat = len(model.features)
        if not (0 < layer_idx < n_feat):
            raise ValueError(f"layer_idx must be in (0, {n_feat})")
        if num_flat_features is None:
            num_flat_features = 2048 if case == "gtzan" else 64
        self.num_flat_features = int(num_flat_features)
        self.layer_idx = int(layer_idx)
        self.num_concepts = int(num_concepts)
        self.U = U
        self.features = nn.Sequential()
        for idx, layer in enumerate(model.features.children()):
            if idx == layer_idx + 1:
                self.features.add_module("projection", Projection(U, num_concepts))
                self.features.add_module("subspacefilter", SubspaceFilter())
                self.features.add_module("invprojection", InvProjection(U, num_concepts))
            self.features.add_module(str(idx), layer)
        self.classifier = nn.Sequential()
        for idx, layer in enumerate(model.classifier.children()):
            self.classifier.add_module(str(idx), layer)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.features(x)
        return self.classifier(x.reshape(-1, self.num_flat_features))


def stack_projections(Us, num_concepts: int) -> torch.Tensor:
    """``Us`` (a sequence of [d][d] matrices or an [n][d][d] tensor) as one contiguous fp32 table [n][d][d];
    ValueError unless there is at least one matrix, all are square of one width d, and ``num_concepts`` divides d."""
    if isinstance(Us, torch.Tensor):
        tab = Us
    else:
        Us = list(Us)
        if not Us:
            raise ValueError("MultiProjectionModel: the table of projection matrices is empty")
        for i, U in enumerate(Us):
            if not isinstance(U, torch.Tensor) or U.dim() != 2 or U.shape != Us[0].shape:
                raise ValueError(f"MultiProjectionModel: matrix {i} has shape "
                                 f"{tuple(getattr(U, 'shape', ()))}, matrix 0 has {tuple(Us[0].shape)}")
        tab = torch.stack([U.to(Us[0].device, torch.float32) for U in Us])
    if tab.dim() != 3 or tab.size(0) < 1 or tab.size(1) != tab.size(2):
        raise ValueError(f"MultiProjectionModel: the table must be [n][d][d] with n >= 1 (got {tuple(tab.shape)})")
    K = int(num_concepts)
    if K < 1 or tab.size(1) % K:
        raise ValueError(f"MultiProjectionModel: num_concepts={num_concepts} must be a positive divisor of "
                         f"d={tab.size(1)}")
    return tab.to(torch.float32).contiguous()


def _row_matrices(tab: torch.Tensor, rows, b: int, like: torch.Tensor) -> torch.Tensor:
    """[b][d][d]: matrix ``rows[i]`` of the table for row i."""
    if rows is None:
        raise ValueError("MultiProjectionModel: set .rows (one table index per batch row) before the forward")
    idx = torch.as_tensor(rows, dtype=torch.long, device=tab.device).reshape(-1)
    if idx.numel() != b:
        raise ValueError(f"MultiProjectionModel: rows has {idx.numel()} entries for a batch of {b}")
    if b and (int(idx.min()) < 0 or int(idx.max()) >= tab.size(0)):
        raise ValueError(f"MultiProjectionModel: rows must lie in [0, {tab.size(0) - 1}]")
    return tab[idx].to(like)


class MultiProjection(nn.Module):
    """Projection with a matrix per row: h_i = a_i · U_tab[rows[i]]  (a batched matmul)."""

    def __init__(self, U_tab: torch.Tensor, num_concepts: int) -> None:
        super().__init__()
        self.U_tab = U_tab
        self.num_concepts = int(num_concepts)
        self.d_k = U_tab.size(1) // self.num_concepts
        self.rows = None

    def forward(self, act_map: torch.Tensor) -> torch.Tensor:
        b, d = act_map.size(0), act_map.size(1)
        vecs = act_map.reshape(b, d, -1).transpose(1, 2)
        h = torch.bmm(vecs, _row_matrices(self.U_tab, self.rows, b, act_map))
        return h.reshape(b, vecs.size(1), self.num_concepts, self.d_k)


class MultiInvProjection(nn.Module):
    """InvProjection with a matrix per row: a'_i = h_i · U_tab[rows[i]]ᵀ."""

    def __init__(self, U_tab: torch.Tensor, num_concepts: int) -> None:
        super().__init__()
        self.U_tab = U_tab
        self.num_concepts = int(num_concepts)
        self.d = U_tab.size(1)
        self.d_k = self.d // self.num_concepts
        self.rows = None

    def forward(self, h: torch.Tensor) -> torch.Tensor:
        b, n = h.size(0), h.size(1)
        side = int(round(n ** 0.5))
        a = torch.bmm(h.reshape(b, n, self.d), _row_matrices(self.U_tab, self.rows, b, h).transpose(1, 2))
        return a.transpose(1, 2).reshape(b, self.d, side, side).contiguous()


class MultiProjectionModel(nn.Module):
    """ProjectionModel for mixed-class batches: a table ``Us`` of orthogonal matrices (a sequence or an
    [n][d][d] tensor, one ``num_concepts``) and, per batch row, the table index the row projects through
    (``rows``, set before the forward: a sequence or an int tensor [B]).

    The three virtual layers keep the names ``features.projection``, ``features.subspacefilter`` and
    ``features.invprojection``, so name maps and ``get_class_composite`` apply unchanged.  The HIP engine
    compiles one plan for the whole table and takes the row indices per call (``u_rows``)."""

    def __init__(self, model: nn.Module, layer_idx: int, Us, num_concepts: int, case: str = "gtzan",
                 num_flat_features: int | None = None) -> None:
        super().__init__()
        n_feat = len(model.features)
        if not (0 < layer_idx < n_feat):
            raise ValueError(f"layer_idx must be in (0, {n_feat})")
        if num_flat_features is None:
            num_flat_features = 2048 if case == "gtzan" else 64
        self.num_flat_features = int(num_flat_features)
        self.layer_idx = int(layer_idx)
        self.num_concepts = int(num_concepts)
        self.U_tab = stack_projections(Us, num_concepts)
        self.features = nn.Sequential()
        for idx, layer in enumerate(model.features.children()):
            if idx == layer_idx + 1:
                self.features.add_module("projection", MultiProjection(self.U_tab, num_concepts))
                self.features.add_module("subspacefilter", SubspaceFilter())
                self.features.add_module("invprojection", MultiInvProjection(self.U_tab, num_concepts))
            self.features.add_module(str(idx), layer)
        self.classifier = nn.Sequential()
        for idx, layer in enumerate(model.classifier.children()):
            self.classifier.add_module(str(idx), layer)

    @property
    def rows(self):
        return self.features.projection.rows

    @rows.setter
    def rows(self, rows) -> None:
        self.features.projection.rows = rows
        self.features.invprojection.rows = rows

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.features(x)
        return self.classifier(x.reshape(-1, self.num_flat_features))
