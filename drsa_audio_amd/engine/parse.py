"""Step 1 of a plan, on the host alone: (model, composite, bf16) -> the ConvStage / DenseStage lists.

Nothing here touches a device or the library: weights are read to the host in fp32, every structural
refusal (EngineError) is raised here, and ``LRPEngine.check`` is this function and no more.  The device
weight sets are made by the prepare step (plan.py), the per-shape launch decisions by schedule.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from ..zennit.canonizers import SequentialMergeBatchNorm


def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def _kind(rule) -> Optional[str]:
    k = None if rule is None else getattr(rule, "kind", type(rule).__name__)
    # zennit Norm(stabilizer) on a conv/dense layer is Epsilon(epsilon=stabilizer): same input/output modifiers,
    # parameters unmodified (NoMod with no keys), gradient mapper out_grad / stabilize(z) and reducer x * grad
    return "epsilon" if k == "norm" else k


def _eps_of(rule) -> float:
    return float(getattr(rule, "epsilon", getattr(rule, "stabilizer", 0.0)))


def _bf16r(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and back: the values a bf16 plan's kernels see."""
    return t.to(torch.bfloat16).to(t.dtype)


@dataclass
class ProjGroup:
    U: torch.Tensor
    K: int
    P: Optional[torch.Tensor]   # U U^T - I (drsa_amd_projection_residual), set by the prepare step
    eps_inv: float
    eps_proj: float
    mask: bool          # SubspaceHook on the filter
    pool_after: bool
    # MultiProjectionModel: a table [n][d][d] of matrices (U is None), the residuals likewise; the row -> matrix
    # index is per-call data (LRPEngine.forward(u_rows=...)), never part of the plan
    U_tab: Optional[torch.Tensor] = None
    P_tab: Optional[torch.Tensor] = None

    @property
    def multi(self) -> bool:
        return self.U_tab is not None

    @property
    def d(self) -> int:
        return int((self.U_tab if self.multi else self.U).size(-1))


@dataclass
class ConvStage:
    name: str
    cin: int
    cout: int
    rule_kind: Optional[str]
    eps: float
    pool: bool
    proj: Optional[ProjGroup]
    input_nonneg: bool
    W: torch.Tensor = None               # host, fp32 (bf16 plan: rounded to bf16 values)
    b: torch.Tensor = None
    rule: object = None
    den_kind: Optional[str] = None       # "gamma" | "eps" | "map" | "ab" | "box" | None
    ng_fwd: int = 1                      # weight groups of the forward / backward conv
    ng_bwd: int = 1
    bwd_bf16: bool = False               # the stage gets a bf16 backward weight set (schedule.mark_bwd_bf16)
    # prepared (plan.py, on the device)
    wts_fwd: torch.Tensor = None
    bias3: torch.Tensor = None
    W2: torch.Tensor = None              # WSquare / Flat: the weights and bias of the denominator map
    b2: torch.Tensor = None
    wts_w2: torch.Tensor = None          # K x K WSquare / Flat: W2 in the forward layout, bias3 row 1 = b2
    bias3_w2: torch.Tensor = None
    # AlphaBeta: second forward (W, W-) for den_n, and the two backward weight sets
    wts_fwd_n: torch.Tensor = None
    bias3_n: torch.Tensor = None
    wts_bwd_n: torch.Tensor = None
    wts_fwd_bf: torch.Tensor = None      # bf16 plan: [ng][cin_p/16][9][2][cout_p][8] bfloat16
    wts_fwd_n_bf: torch.Tensor = None
    wts_bwd_bf: torch.Tensor = None       # bf16 backward: [cout_p/16][9][2][pad32(cin)][8] bfloat16
    alpha: float = 1.0
    beta: float = 0.0
    wts_bwd: torch.Tensor = None
    xmode_bwd: int = 0                   # XM_NONE
    w2_first: Optional[torch.Tensor] = None
    # ZBox (first conv, one input channel): W+ / W- packed [2][cout][9] and b+ / b- [cout]; the bounds
    # images and the rule's maps are per input shape, in den_maps
    zb_wpn: Optional[torch.Tensor] = None
    zb_bp: Optional[torch.Tensor] = None
    zb_bn: Optional[torch.Tensor] = None
    den_maps: Dict[Tuple[int, int], torch.Tensor] = field(default_factory=dict)
    relu_name: Optional[str] = None      # features.<i> of the ReLU after the conv
    pool_name: Optional[str] = None      # features.<i> of the MaxPool2d / AvgPool2d (None: no pool)
    pool_k: Tuple[int, int] = (2, 2)     # pool kernel (= stride); a 2x2 max-pool is fused into the conv
    k: Tuple[int, int] = (3, 3)          # conv kernel (kh, kw); other than 3x3: the drsa_amd_convk_* kernels
    pool_kind: str = "max"               # "max" | "avg" (AvgPool2d: pool_k any pair, never fused, no argmax)
    pool_rule: Optional[str] = None      # avg: None (the pool's plain gradient) | "epsilon" (Epsilon / Norm on it)
    pool_eps: float = 0.0                # avg: that rule's stabiliser

    @property
    def avg(self) -> bool:
        return self.pool and self.pool_kind == "avg"

    @property
    def generic(self) -> bool:           # not 3x3: no fused pool, no den ring / map, fp32 only
        return self.k != (3, 3)


@dataclass
class DenseStage:
    name: str
    W: torch.Tensor
    b: Optional[torch.Tensor]
    rule_kind: Optional[str]
    eps: float
    relu_after: bool
    input_nonneg: bool = False           # the layer's input is known >= 0: the rule's x- terms are dropped
    # Gamma / ZPlus / WSquare / Flat: dense_rule_params(W, b, rule) (None: Epsilon / no rule)
    rp: Optional[dict] = None
    # relevance arriving through the ReLU after the layer is masked by [z > 0].  Not so when that ReLU
    # carries Pass (the gradient passes unchanged) and the next dense layer is WSquare / Flat, whose
    # R_in is not multiplied by its input and so is not already zero where z <= 0
    mask: bool = False
    relu_pass: bool = False              # the ReLU after the layer carries Pass

    @property
    def split(self) -> bool:             # Gamma / ZPlus: modified weight sets and per-sample denominators
        return self.rule_kind in ("gamma", "zplus")

    @property
    def negden(self) -> bool:            # Gamma with unmasked relevance: [z < 0] can hold, den_n is needed
        return self.rule_kind == "gamma" and not self.mask


class EngineError(NotImplementedError):
    pass


DENSE_RULES = (None, "epsilon", "gamma", "zplus", "wsquare", "flat")
# conv rule -> the form of its denominator (ConvStage.den_kind)
_DEN_KIND = {None: None, "epsilon": "eps", "gamma": "gamma", "zplus": "gamma", "wsquare": "map", "flat": "map",
             "alphabeta": "ab", "zbox": "box"}


@torch.no_grad()
def dense_rule_params(W: torch.Tensor, b: Optional[torch.Tensor], rule) -> dict:
    """The parameter sets of a rule on a dense layer (weight ``W [N][K]``, bias ``b`` or None), as
    plan constants: the oracle's own expressions (oracle/lrp_ref.py rule_backward_analytic), two
    roundings each, evaluated once in fp32 where ``W`` lives (the plan calls it on the host).

      gamma    Wp, Wn = W + g W.clamp(min=0), W + g W.clamp(max=0);  bp, bn likewise
      zplus    Wp, Wn = W.clamp(min=0), W.clamp(max=0);  bp = b.clamp(min=0), bn = None
      wsquare  W2, b2 = W W, b b;  den [N] = f(1; W2, b2): one k-ascending fp32 chain per output
               neuron, the bias added last -- it does not depend on the input
      flat     W2, b2 = 1, 0;  den likewise
    ``kind`` and ``eps`` are always present; Epsilon / Norm / no rule need nothing else."""
    kind = _kind(rule)
    if kind not in DENSE_RULES:
        raise EngineError(f"engine: rule {type(rule).__name__} on a dense layer is not supported")
    out = {"kind": kind, "eps": 0.0 if kind is None else float(_eps_of(rule))}
    mod = lambda fn: None if b is None else fn(b)       # noqa: E731
    if kind == "gamma":
        g = rule.gamma
        out.update(Wp=W + g * W.clamp(min=0), Wn=W + g * W.clamp(max=0),
                   bp=mod(lambda t: t + g * t.clamp(min=0)), bn=mod(lambda t: t + g * t.clamp(max=0)))
    elif kind == "zplus":
        out.update(Wp=W.clamp(min=0), Wn=W.clamp(max=0), bp=mod(lambda t: t.clamp(min=0)), bn=None)
    elif kind in ("wsquare", "flat"):
        W2, b2 = (W * W, mod(lambda t: t * t)) if kind == "wsquare" else (torch.ones_like(W), mod(torch.zeros_like))
        acc = torch.zeros(W.size(0), dtype=W.dtype, device=W.device)
        for col in W2.t().contiguous():          # fmaf(1, w2, acc) = fl(acc + w2), k ascending
            acc = acc + col
        out.update(W2=W2, b2=b2, den=acc if b2 is None else acc + b2)
    return out


def _host(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().to(torch.float32)


def _weights(m, nxt, bn_type, merge_bn: bool, where: str):
    """(W, b or None, whether ``nxt`` was folded in) of a conv / linear layer, on the host in fp32 (a BN merge
    there is the same IEEE arithmetic as zennit's canonizer on CPU)."""
    W, b = _host(m.weight), None if m.bias is None else _host(m.bias)
    if not isinstance(nxt, bn_type):
        return W, b, False
    if not merge_bn:
        raise EngineError(f"{bn_type.__name__} in the {where} needs the SequentialMergeBatchNorm canonizer")
    var = _host(nxt.running_var)      # detached fp32 host copies of the BN statistics
    bn = SimpleNamespace(running_var=var, running_mean=_host(nxt.running_mean), eps=nxt.eps,
                         weight=torch.ones_like(var) if nxt.weight is None else _host(nxt.weight),
                         bias=torch.zeros_like(var) if nxt.bias is None else _host(nxt.bias))
    return (*SequentialMergeBatchNorm.fold(W, b, bn), True)


KMAX = 7    # largest conv kernel side (drsa_amd_convk_supported)


def _check_conv(m: nn.Conv2d, name) -> Tuple[int, int]:
    """(kh, kw) of an odd stride-1 'same' zero-padded conv up to 7 x 7; any other conv is refused."""
    kh, kw = (int(k) for k in m.kernel_size)
    same = m.padding == "same" or (not isinstance(m.padding, str) and tuple(m.padding) == ((kh - 1) // 2, (kw - 1) // 2))
    ok = (kh % 2 == 1 and kw % 2 == 1 and max(kh, kw) <= KMAX and tuple(m.stride) == (1, 1)
          and tuple(m.dilation) == (1, 1) and m.groups == 1 and same and m.padding_mode == "zeros")
    if not ok:
        raise EngineError(f"engine: features.{name} must be a stride-1 'same' zero-padded conv with an odd kernel "
                          f"up to {KMAX}x{KMAX} (got kernel {kh}x{kw}, stride {tuple(m.stride)}, padding {m.padding!r}, "
                          f"padding_mode {m.padding_mode!r})")
    return kh, kw


def _convk_supported(kh: int, kw: int, cin: int, cout: int) -> bool:
    """drsa_amd_convk_supported where the library is built (host code, no GPU); its rule otherwise, so
    that LRPEngine.check needs no library."""
    from .. import _capi
    try:
        return bool(_capi.lib().drsa_amd_convk_supported(kh, kw, cin, cout))
    except (_capi.DrsaAmdError, OSError, AttributeError):
        return kh in (1, 3, 5, 7) and kw in (1, 3, 5, 7) and 1 <= cin <= 1 << 20 and (cout + 31) // 32 <= 65535


def _check_pool(m: nn.MaxPool2d):
    ks, st, pd, dl = (v if isinstance(v, tuple) else (v, v) for v in (m.kernel_size, m.stride, m.padding, m.dilation))
    if tuple(ks) != tuple(st) or tuple(pd) != (0, 0) or tuple(dl) != (1, 1) or m.ceil_mode or ks[0] * ks[1] > 256:
        raise EngineError(f"engine: MaxPool2d must have stride = kernel, no padding/dilation (got kernel {ks}, "
                          f"stride {st})")
    return (int(ks[0]), int(ks[1]))


def _check_avgpool(m: nn.AvgPool2d, name: str) -> Tuple[int, int]:
    """(ph, pw) of an AvgPool2d with stride = kernel, no padding, floor mode and its own divisor; any other is
    refused (that the window divides the map is the schedule's check, per input shape)."""
    ks, pd = (v if isinstance(v, tuple) else (v, v) for v in (m.kernel_size, m.padding))
    st = ks if m.stride is None else (m.stride if isinstance(m.stride, tuple) else (m.stride, m.stride))
    if (tuple(ks) != tuple(st) or tuple(pd) != (0, 0) or m.ceil_mode or m.divisor_override is not None
            or min(ks) < 1):
        raise EngineError(f"engine: AvgPool2d {name} must have stride = kernel, no padding, ceil_mode=False and no "
                          f"divisor_override (got kernel {tuple(ks)}, stride {tuple(st)}, padding {tuple(pd)}, "
                          f"ceil_mode {m.ceil_mode}, divisor_override {m.divisor_override})")
    return (int(ks[0]), int(ks[1]))


def _avgpool_rule(rule, name: str, relu_name: str, relu_rule) -> Tuple[Optional[str], float]:
    """(pool_rule, pool_eps) of the rule mapped to an average pool: unmapped (its plain gradient), or Epsilon /
    Norm; anything else, Pass included, is refused."""
    if rule is None:
        if relu_rule is not None:
            # the pool's plain gradient hands relevance to dead pixels (a = 0) of a live window; with Pass on the
            # ReLU it would pass them, and the conv rules form no [z < 0] branch (the reasoning of the dense
            # WSquare / Flat refusal below)
            raise EngineError(f"engine: an unmapped AvgPool2d {name} below a Pass on its block's activation "
                              f"({relu_name}) is not supported: map the pool to Norm / Epsilon or leave the "
                              "activation unmapped")
        return None, 0.0
    if _kind(rule) != "epsilon":
        raise EngineError(f"engine: rule {type(rule).__name__} on AvgPool2d {name} is not supported (Norm, Epsilon "
                          "or no rule)")
    return "epsilon", _eps_of(rule)


def _rule_ok_on_activation(rule):
    if rule is not None and _kind(rule) != "pass":
        raise EngineError(f"engine: rule {type(rule).__name__} on an activation/pool layer is not supported")


def _is(m, name: str) -> bool:
    return type(m).__name__ == name


@torch.no_grad()
def parse(model: nn.Module, composite, bf16: bool = False) -> Tuple[List[ConvStage], List[DenseStage]]:
    """The stages of ``model`` under ``composite``; raises the EngineError that compiling the plan would."""
    rules = composite.rules(model) if composite is not None else {}
    merge_bn = any(isinstance(c, SequentialMergeBatchNorm) for c in getattr(composite, "canonizers", []))
    stages, dense = [], []
    feats = list(model.features.named_children())
    i, n = 0, len(feats)
    prev_nonneg = False          # raw network input may be negative
    while i < n:
        name, m = feats[i]
        if isinstance(m, (nn.Dropout, nn.Identity)):
            i += 1
            continue
        if not isinstance(m, nn.Conv2d):
            raise EngineError(f"engine: unexpected feature layer features.{name} ({type(m).__name__})")
        ksz = _check_conv(m, name)
        W, b, bn = _weights(m, feats[i + 1][1] if i + 1 < n else None, nn.BatchNorm2d, merge_bn, "trunk")
        W, b = _bf16r(W) if bf16 else W, torch.zeros(m.out_channels) if b is None else b
        j = i + 1 + bn
        if j >= n or not isinstance(feats[j][1], nn.ReLU):
            raise EngineError(f"engine: conv features.{name} must be followed by ReLU")
        relu_name = f"features.{feats[j][0]}"
        _rule_ok_on_activation(rules.get(relu_name))
        j += 1
        proj = None
        if j < n and (_is(feats[j][1], "Projection") or _is(feats[j][1], "MultiProjection")):
            multi = _is(feats[j][1], "MultiProjection")
            if not (j + 2 < n and _is(feats[j + 1][1], "SubspaceFilter")
                    and _is(feats[j + 2][1], "MultiInvProjection" if multi else "InvProjection")):
                raise EngineError("engine: Projection must be followed by SubspaceFilter, InvProjection")
            pm = feats[j][1]
            r_p, r_f, r_i = (rules.get(f"features.{feats[j + d][0]}") for d in range(3))
            if _kind(r_p) != "epsilon" or _kind(r_i) != "epsilon":
                raise EngineError("engine: projection layers need Epsilon rules (get_class_composite)")
            if r_f is not None and type(r_f).__name__ != "SubspaceHook":
                raise EngineError("engine: only SubspaceHook is supported on the subspace filter")
            if multi and feats[j + 2][1].U_tab is not pm.U_tab:
                raise EngineError("engine: MultiProjection and MultiInvProjection must share one table of matrices")
            proj = ProjGroup(U=None if multi else _host(pm.U).contiguous(), K=int(pm.num_concepts), P=None,
                             eps_inv=_eps_of(r_i), eps_proj=_eps_of(r_p), mask=r_f is not None, pool_after=False,
                             U_tab=_host(pm.U_tab).contiguous() if multi else None)
            if r_f is not None and int(r_f.num_concepts) != proj.K:
                raise EngineError("engine: SubspaceHook num_concepts differs from the projection")
            j += 3
        pool, pool_name, pool_k, pool_kind, pool_rule, pool_eps = False, None, (2, 2), "max", None, 0.0
        if j < n and isinstance(feats[j][1], nn.MaxPool2d):
            pool_k = _check_pool(feats[j][1])
            pool, pool_name = True, f"features.{feats[j][0]}"
            _rule_ok_on_activation(rules.get(pool_name))
            j += 1
        elif j < n and isinstance(feats[j][1], nn.AvgPool2d):
            pool, pool_name, pool_kind = True, f"features.{feats[j][0]}", "avg"
            pool_k = _check_avgpool(feats[j][1], pool_name)
            if proj is not None:
                raise EngineError(f"engine: AvgPool2d {pool_name} after a ProjectionModel layer is not supported (the "
                                  "projection kernels pool by maximum): a MaxPool2d(2) or no pool there")
            pool_rule, pool_eps = _avgpool_rule(rules.get(pool_name), pool_name, relu_name, rules.get(relu_name))
            j += 1
        elif j < n and isinstance(feats[j][1], nn.AdaptiveAvgPool2d):
            raise EngineError(f"engine: AdaptiveAvgPool2d features.{feats[j][0]} is not supported: use an AvgPool2d "
                              "whose kernel (= stride) divides the map")
        if proj is not None:
            proj.pool_after = pool
            if pool and pool_k != (2, 2):
                raise EngineError("engine: a ProjectionModel layer must be followed by MaxPool2d(2) or no pool")
        rule = rules.get(f"features.{name}")
        kind = _kind(rule)
        if kind not in (None, "epsilon", "gamma", "wsquare", "flat", "zplus", "alphabeta", "zbox"):
            raise EngineError(f"engine: rule {type(rule).__name__} on conv features.{name} is not supported yet")
        if kind == "zbox" and (stages or m.in_channels != 1):
            raise EngineError(f"engine: ZBox on features.{name} is not supported: it is the rule of the first "
                              "conv of a one-channel input (the box bounds the network input)")
        if ksz != (3, 3):
            if kind == "zbox":
                raise EngineError(f"engine: ZBox on features.{name} needs a 3x3 conv (its kernels are 3x3; got "
                                  f"{ksz[0]}x{ksz[1]})")
            if bf16:
                raise EngineError(f"engine: a bf16 plan needs 3x3 convs (features.{name} is {ksz[0]}x{ksz[1]}; the "
                                  "K x K kernels are fp32)")
            if not _convk_supported(*ksz, m.in_channels, m.out_channels):
                raise EngineError(f"engine: no K x K kernel for features.{name} ({ksz[0]}x{ksz[1]}, "
                                  f"{m.in_channels} -> {m.out_channels} channels)")
        if pool_kind == "avg" and kind in ("alphabeta", "zbox"):
            raise EngineError(f"engine: {type(rule).__name__} on features.{name}, whose block AvgPool2d {pool_name} "
                              "pools, is not supported (its kernels take relevance through a max-pool or none)")
        if kind == "alphabeta" and (not prev_nonneg or (pool and pool_k != (2, 2))):
            raise EngineError(f"engine: AlphaBeta on features.{name} needs a non-negative input (not the first "
                              "conv) and a 2x2 or no max-pool after it")
        # Gamma / ZPlus run one weight group more per sign of the input (forward: W itself first)
        den_kind = _DEN_KIND[kind]
        signs = (1 if prev_nonneg else 2) if den_kind == "gamma" else 0
        stages.append(ConvStage(name=f"features.{name}", cin=m.in_channels, cout=m.out_channels, rule_kind=kind,
                                eps=_eps_of(rule) if kind else 0.0, pool=pool, proj=proj, input_nonneg=prev_nonneg,
                                W=W, b=b, rule=rule, den_kind=den_kind, ng_fwd=2 if den_kind == "ab" else 1 + signs,
                                ng_bwd=max(signs, 1), relu_name=relu_name, pool_name=pool_name, pool_k=pool_k, k=ksz,
                                pool_kind=pool_kind, pool_rule=pool_rule, pool_eps=pool_eps))
        prev_nonneg = proj is None      # outputs are post-ReLU (pooled) unless a' follows
        i = j
    # classifier
    cl = list(model.classifier.named_children())
    i, n = 0, len(cl)
    while i < n:
        name, m = cl[i]
        if isinstance(m, (nn.Dropout, nn.Identity)):
            i += 1
            continue
        if not isinstance(m, nn.Linear):
            raise EngineError(f"engine: unexpected classifier layer classifier.{name} ({type(m).__name__})")
        W, b, bn = _weights(m, cl[i + 1][1] if i + 1 < n else None, nn.BatchNorm1d, merge_bn, "head")
        j = i + 1 + bn
        relu = relu_pass = False
        while j < n and isinstance(cl[j][1], (nn.ReLU, nn.Dropout)):
            if isinstance(cl[j][1], nn.ReLU):
                relu = True
                _rule_ok_on_activation(rules.get(f"classifier.{cl[j][0]}"))
                relu_pass = rules.get(f"classifier.{cl[j][0]}") is not None
            j += 1
        rule = rules.get(f"classifier.{name}")
        kind = _kind(rule)
        if dense and dense[-1].relu_pass and kind in ("wsquare", "flat"):
            dense[-1].mask = False      # see DenseStage.mask
        if not dense and kind in ("wsquare", "flat"):
            # towards the trunk there is no such unmasked path: the hand-off to the last conv stage
            # masks by [a > 0] and the conv rules form no [z < 0] branch (Gamma: no den_n), while a
            # Pass on that stage's ReLU lets WSquare / Flat relevance through where a = 0.  Refused
            # whatever the conv's rule; with the ReLU unmapped autograd's own mask is the hand-off's
            lst = stages[-1]
            if lst.proj is None and rules.get(lst.relu_name) is not None:
                raise EngineError(f"engine: {type(rule).__name__} on classifier.{name} above a Pass on the last "
                                  f"conv block's activation ({lst.relu_name}) is not supported: leave that "
                                  "activation unmapped")
        if kind not in DENSE_RULES:
            raise EngineError(f"engine: rule {type(rule).__name__} on classifier.{name} is not supported yet")
        if rule is not None and "bias" in getattr(rule, "zero_params", ()):
            raise EngineError("engine: zero_params on dense layers is not supported yet")
        # the rule's weight sets / constant denominator are formed on the host, once per plan
        rp = dense_rule_params(W, b, rule) if kind in ("gamma", "zplus", "wsquare", "flat") else None
        dense.append(DenseStage(name=f"classifier.{name}", W=W, b=b, rule_kind=kind, eps=_eps_of(rule) if kind else 0.0,
                                relu_after=relu, input_nonneg=prev_nonneg, rp=rp, mask=relu, relu_pass=relu_pass))
        prev_nonneg = relu
        i = j
    if not stages or not dense:
        raise EngineError("engine: model must have a conv trunk and a dense head")
    return stages, dense
