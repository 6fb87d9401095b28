"""Principal Relevant Component Analysis (PRCA): DRSA's closed-form companion, on the GPU.

Given the activation and context vectors ``A, C`` ([N, d], the tensors ``SubspaceOptimizer`` trains
on), PRCA maximises ``tr(U^T M U)`` over orthonormal ``U`` with ``M = (A^T C + C^T A) / (2N)``: the
solution is the eigenvectors of the symmetric, indefinite ``M`` by descending eigenvalue.  It needs
no optimisation run and is the standard baseline of DRSA in the same paper; the reference
repository does not ship it.  Both steps run on device through ``libdrsa_amd.so``
(``csrc/prca.hip``): the cross-covariance on fp32 MFMA with a deterministic fixed-order reduction,
and a one-workgroup Jacobi eigensolver (``drsa_amd_syevj``) with a Newton-Schulz re-orthogonalised
basis, so no ``.cpu().double()`` + ``eigh`` round trip sits in the pipeline.

A full ``d x d`` PRCA basis is a valid ``U`` for ``ProjectionModel``, ``HeatmapGenerator``,
``compute_subspace_relevances`` and ``concept_flipping``: with ``K | d`` concept block 0 is the
top-``d/K`` PRCA subspace and the later blocks are the residual in descending relevance.

* ``relevance_covariance(A, C) -> M [d, d]`` (``relevance_covariance_partial`` /
  ``relevance_covariance_finish`` expose the shard-wise form: slabs of row shards add up)
* ``eigh_descending(M) -> (w [d], V [d, d])``
* ``prca(A, C) -> (U [d, d], w [d])``: ``U[:, :k]`` is the PRCA subspace of dimension ``k`` and
  ``w[:k].sum()`` its objective
* ``main(...)`` writes ``drsa.main``'s file layout with one run, so ``load_projection_matrix``,
  ``get_best_run`` and ``concept_flipping(path_to_U=...)`` read a PRCA basis unchanged.

GPU fp32 tensors only (``DrsaAmdError`` otherwise), ``1 <= d <= 128``.
"""
from __future__ import annotations

import os
import pickle
from typing import Tuple

import numpy as np
import torch

from ... import _capi
from .drsa import _dev, drsa_objective

__all__ = ["relevance_covariance", "relevance_covariance_partial", "relevance_covariance_finish", "eigh_descending",
           "prca", "main"]

MAX_D = 128


def _check_rows(A: torch.Tensor, C: torch.Tensor) -> Tuple[int, int]:
    _capi.require_gpu(A, "activation_vecs")
    _capi.require_gpu(C, "context_vecs")
    if A.dim() != 2 or A.shape != C.shape:
        raise ValueError("activation and context vectors must both be [N, d]")
    N, d = A.shape
    if N < 1 or not 1 <= d <= MAX_D:
        raise ValueError(f"PRCA needs N >= 1 and 1 <= d <= {MAX_D} (got N={N}, d={d})")
    if C.device != A.device:
        raise ValueError("activation and context vectors must live on one device")
    return N, d


def relevance_covariance_partial(A: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """The un-normalised ``A^T C`` [d, d] of these rows (the slabs of row shards add up)."""
    N, d = _check_rows(A, C)
    nbytes = int(_capi.lib().drsa_amd_prca_workspace_bytes(N, d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    slab = torch.empty(d, d, dtype=torch.float32, device=A.device)
    _capi.call("drsa_amd_prca_partial", A.data_ptr(), C.data_ptr(), N, d, slab.data_ptr(), ws.data_ptr(), nbytes,
               _capi.stream_ptr(A.device))
    return slab


def relevance_covariance_finish(slab: torch.Tensor, n_total: int) -> torch.Tensor:
    """``M = (G + G^T) / (2 n_total)`` from the summed slab ``G``: symmetric bit for bit."""
    _capi.require_gpu(slab, "slab")
    if slab.dim() != 2 or slab.size(0) != slab.size(1) or not 1 <= slab.size(0) <= MAX_D:
        raise ValueError(f"slab must be [d, d] with 1 <= d <= {MAX_D}")
    if n_total < 1:
        raise ValueError("n_total must be positive")
    M = torch.empty_like(slab)
    _capi.call("drsa_amd_prca_finish", slab.data_ptr(), int(n_total), slab.size(0), M.data_ptr(),
               _capi.stream_ptr(slab.device))
    return M


def relevance_covariance(A: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """``M = (A^T C + C^T A) / (2N)`` [d, d] on device."""
    return relevance_covariance_finish(relevance_covariance_partial(A, C), A.size(0))


def eigh_descending(M: torch.Tensor, return_sweeps: bool = False):
    """Eigenvalues ``w`` [d] (descending) and eigenvectors ``V`` [d, d] (column k belongs to w[k];
    its entry of largest magnitude is positive) of the symmetric ``M``, whose upper triangle is
    read.  ``return_sweeps`` adds the Jacobi sweep count (an int; reading it synchronises)."""
    _capi.require_gpu(M, "M")
    if M.dim() != 2 or M.size(0) != M.size(1) or not 1 <= M.size(0) <= MAX_D:
        raise ValueError(f"M must be [d, d] with 1 <= d <= {MAX_D}")
    d = M.size(0)
    nbytes = int(_capi.lib().drsa_amd_syevj_workspace_bytes(d))
    status = torch.empty(nbytes // 4, dtype=torch.int32, device=M.device)
    w = torch.empty(d, dtype=torch.float32, device=M.device)
    V = torch.empty(d, d, dtype=torch.float32, device=M.device)
    _capi.call("drsa_amd_syevj", M.data_ptr(), d, w.data_ptr(), V.data_ptr(), None, status.data_ptr(), nbytes,
               _capi.stream_ptr(M.device))
    return (w, V, int(status[0].item())) if return_sweeps else (w, V)


def prca(A: torch.Tensor, C: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(U [d, d], w [d])``: the PRCA basis (columns by descending relevance) and its eigenvalues."""
    w, U = eigh_descending(relevance_covariance(A, C))
    return U, w


def main(activation_vecs: torch.Tensor, context_vecs: torch.Tensor, model_root: str, num_concepts: int = 4,
         device: str | torch.device = torch.device("cuda")) -> torch.Tensor:
    """Writes ``model_root/run1/projection_matrix.pkl`` (U, numpy float32) and ``train_stats.csv`` (one
    ``loss`` row: the DRSA objective of U at ``num_concepts``), the layout of ``drsa.main`` with one
    run.  Returns U."""
    import pandas as pd
    device = _dev(device)
    A = activation_vecs.detach().to(device, torch.float32).contiguous()
    C = context_vecs.detach().to(device, torch.float32).contiguous()
    U, _ = prca(A, C)
    loss = drsa_objective(A, C, U, int(num_concepts))
    path = os.path.join(model_root, "run1")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "projection_matrix.pkl"), "wb") as fh:
        pickle.dump(U.cpu().numpy(), fh)
    pd.DataFrame({"loss": [np.float32(loss.item())]}).to_csv(os.path.join(path, "train_stats.csv"))
    return U
