"""Step 3 of a plan: which launches each stage gets at one shape, as plain data.

``schedule`` is a pure function of integers: the stages' sizes and rule facts (parse.py), the input shape,
the capture / stop_after / fanout of the call, the three alternative-form flags (plan.py) and the
library's ``*_has_kernel*`` queries (host code, no GPU needed).  Every choice between two kernels is made
here and nowhere else; ``LRPEngine.forward`` / ``backward`` walk the result, get buffers and launch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple, Union

from .. import _capi
from .._capi import POST_DIV, POST_DIV_MAP, POST_DIV_RING, POST_MASK, POST_NONE
from .parse import ConvStage, DenseStage, EngineError, _pad32

_FWD, _BWD, _LIN = "drsa_amd_conv_fwd", "drsa_amd_conv_bwd", "drsa_amd_linear"
_FWDK, _BWDK = "drsa_amd_convk_fwd", "drsa_amd_convk_bwd"     # a conv that is not 3x3 (ConvStage.generic)


def lib_has_kernel(query: str, *args: int) -> bool:
    """One of the library's four conv ``*_has_kernel*`` queries (csrc/lrp_conv.hip)."""
    return bool(getattr(_capi.lib(), query)(*args))


def mark_bwd_bf16(stages: List[ConvStage], bf16_backward: bool, has_kernel: Callable = lib_has_kernel) -> None:
    """Which stages get a bf16 backward weight set (``st.bwd_bf16``; the prepare step builds the tensor
    from it): one weight group, not AlphaBeta, and a bf16 backward kernel for the channel pair."""
    for st in stages:
        st.bwd_bf16 = bool(bf16_backward and st.cin > 1 and st.ng_bwd == 1 and st.den_kind != "ab"
                           and has_kernel(_BWD + "_has_kernel_bf16", st.cout, st.cin, 32, 1, 0))


def _proj_hw(h: int, w: int) -> Tuple[int, int]:
    """The map size the projection kernels tile for an h x w map (W 8, 16 or a multiple of 32, H a
    multiple of 64 / min(W, 32) rows): (h, w) itself wherever they take it as it is."""
    wk = 8 if w <= 8 else 16 if w <= 16 else _pad32(w)
    rows = 64 // min(wk, 32)
    return (h + rows - 1) // rows * rows, wk


@dataclass(frozen=True)
class ConvStep:
    hw: Tuple[int, int]         # the conv's map
    out_hw: Tuple[int, int]     # the stage output (after projection and pool)
    form: str                   # "fused" (pool in the conv epilogue) | "unfused" (conv, then maxpool_capture) | "full"
    #                             (no pool in the conv: none follows, or the projection comes first) | "avg" (conv at
    #                             full resolution with its denominator, then drsa_amd_avgpool_fwd)
    fwd: str                    # conv forward entry point
    pool: int                   # its pool code: 0, 1 (2x2), 2 (2x4)
    den: str                    # left for the division below: "none" | "copy" (per sample, at the argmax; "full" and
    #                             "avg": at every pixel) | "ring"
    #                             (compact border ring + the map's interior value) | "map" (the shared map itself)
    proj: Optional[Tuple[int, int, bool]] = None    # projection stage: its kernels' map size (padded when != hw),
    #                             and whether projection_fwd stores h and a' for projection_bwd
    g_in: str = "dense"         # backward: g arrives "dense" | "sparse" (pooled, with argmax bytes) | through "unpool"
    #                             (drsa_amd_relevance_unpool first) | from "proj" (drsa_amd_projection_bwd first) |
    #                             through "unavg" (drsa_amd_avgpool_bwd first: the raw relevance at the pool's output
    #                             in, the stage's own division included: the launch above runs without a post step)
    pool_w: int = 2             # pool width of a sparse g (4: the folded (2,4) pool)
    bwd: Optional[str] = None   # backward entry point (None: at or below stop_after, not run)
    wts_bf16: bool = False      # it runs on the stage's bf16 weight set
    post: int = POST_NONE       # its post step: the division / mask of the layer below (stop_after folded in)
    clones: int = 1             # relevance clones per sample in g and below
    tap_post: int = POST_NONE   # a tapped stage above the lowest tap: the post step taken out of the backward above it
    #                             (POST_DIV | POST_MASK), which drsa_amd_relevance_post applies once R is recorded
    rel_full: bool = False      # an average-pooled stage whose ReLU output is captured: drsa_amd_avgpool_bwd also writes
    #                             the relevance at that output (the stage at stop_after included)


@dataclass(frozen=True)
class DenseStep:
    fwd: str            # drsa_amd_linear_fwd | drsa_amd_linear_rule_fwd
    bwd: str            # drsa_amd_linear_bwd | drsa_amd_linear_rule_bwd
    signed: int         # x_signed of the rule entries (the input may be negative)
    wn: bool            # the rule entries get Wn
    relu_mask: int
    bcast: int          # rule_bwd den_bcast (WSquare / Flat: the plan's constant denominator)
    zsign: int          # rule_bwd zsign (Gamma); linear_bwd rule_eps (Epsilon)
    xmul: int           # rule_bwd xmul (Gamma / ZPlus); linear_bwd xmode (Epsilon: XM_MUL)
    post: int           # first dense stage: the post step of the last conv stage


def _post_of(st: ConvStage, den: str) -> int:
    """The post step for relevance arriving at the OUTPUT of a conv stage that leaves ``den``."""
    if st.proj is not None or st.den_kind in (None, "ab"):
        return POST_NONE if st.proj is not None else POST_MASK
    return {"map": POST_DIV_MAP, "ring": POST_DIV_RING}.get(den, POST_DIV)


def capture_stage(stages: List[ConvStage], layer_name: str) -> Tuple[int, str]:
    """(stage index, "relu" | "pool") of a trunk module name (features.<layer_idx>)."""
    for li, st in enumerate(stages):
        if st.relu_name == layer_name:
            if st.proj is not None:
                raise EngineError("engine: capture inside a ProjectionModel layer is not supported")
            return li, "relu"
        if st.pool_name == layer_name and st.proj is None:
            return li, "pool"
    raise EngineError(f"engine: {layer_name} is not a ReLU or MaxPool2d / AvgPool2d output of the conv trunk "
                      "(DRSA data is captured at ReLU/pool outputs, preprocessing.py:60)")


def capture_set(stages: List[ConvStage], layer_names: Sequence[str]
                ) -> Tuple[List[Tuple[int, str]], Tuple[int, ...], int, Tuple[int, ...]]:
    """One pass for several captured layers: ([(stage, "relu" | "pool") per name], capture, stop_after, taps)
    as ``schedule`` takes them.  The ReLU and the pool of one stage may both be named (they share the stage's
    relevance); the same name twice is an error."""
    names = list(layer_names)
    if not names:
        raise ValueError("capture: no layer given")
    if len(set(names)) != len(names):
        raise ValueError(f"capture: a layer is named twice in {names}")
    where = [capture_stage(stages, n) for n in names]
    tapped = sorted({li for li, _ in where})
    keep = tuple(li for li in tapped if stages[li].pool and (li, "relu") in where)
    return where, keep, tapped[0], tuple(tapped[1:])


def schedule(stages: List[ConvStage], dense: List[DenseStage], B: int, H: int, W: int,
             capture: Union[None, int, Tuple[int, ...]] = None, stop_after: Optional[int] = None, fanout: int = 0,
             bf16: bool = False, proj_store: bool = False, den_copy: bool = False, pool24_sparse: bool = True,
             has_kernel: Callable = lib_has_kernel, taps: Tuple[int, ...] = ()
             ) -> Tuple[Tuple[ConvStep, ...], Tuple[DenseStep, ...]]:
    """(conv steps, dense steps) of one call form at one input shape.  ``bf16``: the plan's precision; the
    three flags: plan._PROJ_STORE, _DEN_COPY, _POOL24_SPARSE as the engine read them.  ``capture``: the stage, or
    the stages, whose full-resolution ReLU output the forward keeps.  ``taps``: conv stages above ``stop_after``,
    ascending, at whose OUTPUT the backward also records the raw relevance: the backward above a tap leaves its
    post step out, as above ``stop_after``, and the tapped step carries it (``tap_post``)."""
    keep = () if capture is None else (capture,) if isinstance(capture, int) else tuple(capture)
    taps = tuple(taps)
    if list(taps) != sorted(set(taps)) or any(not 0 <= t < len(stages) for t in taps) or \
            (taps and stop_after is not None and taps[0] <= stop_after):
        raise ValueError(f"taps {taps} must be conv stages in ascending order, all above stop_after ({stop_after})")
    L, conv, below, (h, w) = len(stages), [], POST_NONE, (H, W)
    for li, st in enumerate(stages):
        ph, pw = st.pool_k if st.pool else (1, 1)
        # w % 4: the conv's rule backward and its unpooled forward move float4 rows (the C entry points refuse
        # other widths), so a map the backward could not cross is refused here
        if h % 2 or w % 4 or h % ph or w % pw:
            raise ValueError(f"{st.name}: feature map {h}x{w} must have an even height, a width divisible by 4 "
                             f"and sides divisible by the pool")
        if st.den_kind == "ab" and li in keep and st.pool:
            raise EngineError("engine: capture at the ReLU of an AlphaBeta conv is not supported")
        bf = bf16 and st.cin > 1
        entry, den = _FWD + ("_bf16" if bf else ""), "none" if st.den_kind is None else "copy"
        # a conv that is not 3x3 runs on the K x K kernels: no pool in its epilogue, a dense g, and a
        # per-sample denominator copy on both of its sides (post NONE / DIV / MASK only)
        if st.generic:
            entry = _FWDK
        # a WSquare / Flat map is read in place of a per-sample copy where the next backward can divide by it
        # (a tapped stage's division is a launch of its own, which reads the per-sample copy)
        in_place = (st.den_kind == "map" and st.proj is None and li + 1 < L and stages[li + 1].den_kind != "ab"
                    and not den_copy and li not in taps and not st.generic and not stages[li + 1].generic)
        # pools fused into the conv epilogue: 2x2 and 2x4 (code 1 / 2); others, and the capture layer (its
        # full-resolution ReLU output is kept), go through maxpool_capture
        fusable = st.pool and not st.avg and st.proj is None and not st.generic
        code = {(2, 2): 1, (2, 4): 2}.get(st.pool_k, 0) if fusable else 0
        if code == 2 and not has_kernel(_FWD + "_has_kernel", st.cin, st.cout, w, st.ng_fwd, 2, int(bf)):
            code = 0
        if st.den_kind == "box" and code == 2:
            # the ZBox denominator at a pooled map's argmax is formed for 2x2 cells (drsa_amd_first_layer_zbox_den);
            # any other pool goes through maxpool_capture, which gathers the full-resolution copy
            code = 0
        proj = None
        if st.proj is not None or not st.pool:
            # WSquare / Flat without a pool after it (VGGish conv0 -> conv3): the per-sample denominator IS the
            # input-independent map; the next backward reads the map itself (drsa_amd_conv_bwd_den_map), no
            # per-sample copy is written
            form, den = "full", "map" if in_place else den
            # a map smaller than the projection kernels tile (the toy net's last block: 4 x 4) runs zero-padded at
            # its right and bottom: every pixel and every 2 x 2 window is on its own there, and the kernel-side
            # buffers (a, h, a', pooled, argmax) keep that size
            proj = None if st.proj is None else (*_proj_hw(h, w), proj_store)
        elif st.avg:
            # an average pool is a launch of its own on the full-resolution map, and the stage's denominator stays
            # at full resolution for drsa_amd_avgpool_bwd: the shared WSquare / Flat map itself where the 3x3
            # forward can leave it (the K x K forward writes its per-sample copy)
            form, den = "avg", "map" if st.den_kind == "map" and not st.generic else den
        elif li in keep or code == 0:
            form, code = "unfused", 0
        else:
            form = "fused"
            # WSquare / Flat first layer under a 2x2 pool: its map is one value per channel off the image's border
            # ring, so the forward stores the per-sample denominator copy only on the ring, compactly
            # (drsa_amd_conv_fwd_den_ring), and the next conv's backward reads the map's interior value elsewhere
            # (drsa_amd_conv_bwd_den_ring; bit-identical)
            if in_place and code == 1 and st.cin == 1 and w % 16 == 0 and h >= 4:
                entry, den = _FWD + "_den_ring", "ring"
        step = dict(hw=(h, w), out_hw=(h // ph, w // pw), form=form, fwd=entry, pool=code, den=den, proj=proj)
        if st.avg and li in keep:
            step["rel_full"] = True
        w_in, (h, w) = w, step["out_hw"]
        # the post step of the layer below; this stage's, for the next (none above an average pool, as above a tap:
        # drsa_amd_avgpool_bwd takes the raw relevance at the pool's output)
        below_raw, below = below, POST_NONE if st.avg else _post_of(st, den)
        if stop_after is not None and li <= stop_after:
            conv.append(ConvStep(**step))
            continue
        # ---- the stage's backward: g from above, the post step of the layer below ----
        post = POST_NONE if (stop_after == li - 1 or li - 1 in taps) else below_raw
        fold = (pool24_sparse and st.pool and not st.avg and st.pool_k == (2, 4) and st.den_kind != "ab" and li > 0
                and not st.generic)
        above = next((s.proj for s in stages[li:] if s.proj is not None), None)     # clones start at the projection
        clones = {1: above.K + 1, 2: above.K}.get(int(fanout), 1) if above is not None and above.mask else 1
        g_in, pool_w, bf = "dense", 2, False
        if st.proj is not None:
            g_in = "proj"
        elif st.avg:
            g_in = "unavg"
        elif st.pool and st.pool_k == (2, 2) and not st.generic:
            g_in = "sparse"
        elif (fold and st.bwd_bf16 and below_raw != POST_DIV_RING
              and has_kernel(_BWD + "_has_kernel_bf16_pw", st.cout, st.cin, w_in, 4)):
            # the (2,4) pool backward folded into the bf16 backward's staging (no unpooled g); never above a den
            # ring, whether or not stop_after leaves its division out
            g_in, pool_w = "sparse", 4
        elif (fold and not st.bwd_bf16 and post == POST_DIV_MAP
              and has_kernel(_BWD + "_has_kernel_pw", st.cout, st.cin, w_in, st.ng_bwd, 4)):
            # the same fold in the fp32 backward (VGGish block 1 above the WSquare layer: the den-map backward takes
            # the pooled g and its argmax bytes)
            g_in, pool_w = "sparse", 4
        elif st.pool:
            g_in = "unpool"
        if st.generic:                  # every rule, AlphaBeta's two plain backwards included
            entry = _BWDK
        elif li == 0 and st.den_kind == "map" and st.cin == 1:
            entry = "drsa_amd_first_layer_bwd"
        elif st.den_kind == "box":      # parse: the first conv, one input channel; g pool-sparse or dense as above
            entry = "drsa_amd_first_layer_zbox_bwd"
        elif st.den_kind == "ab":       # ab_split, two plain backward convs, ab_combine (which applies post)
            entry = _BWD
        else:
            # the entry point follows the post step of the layer below (compact den ring, shared den map, else any
            # other) and the pool width of a pool-sparse g; it runs on the bf16 weights where the plan prepared them
            # and a kernel exists.  For g at 2x2-pool resolution, has_kernel_bf16_pw(pool_w = 2) is
            # has_kernel_bf16(ng = 1, sparse = 1)
            query = ("_has_kernel_bf16_pw", st.cout, st.cin, w_in, pool_w) if g_in == "sparse" else \
                ("_has_kernel_bf16", st.cout, st.cin, w_in, 1, 0)
            bf = st.bwd_bf16 and has_kernel(_BWD + query[0], *query[1:])
            if post in (POST_DIV_RING, POST_DIV_MAP):
                entry = _BWD + ("_den_ring" if post == POST_DIV_RING else "_den_map")
            else:   # a (2,4) pool is folded without the den map only onto the bf16 kernel (bf holds: the same query)
                entry = _BWD + ("_bf16_pw" if pool_w == 4 else "_bf16" if bf else "")
        conv.append(ConvStep(g_in=g_in, pool_w=pool_w, bwd=entry, wts_bf16=bf, post=post, clones=clones,
                             tap_post=below if li in taps else POST_NONE, **step))
    head = []
    for di, ds in enumerate(dense):
        rule, eps_r, signed = ds.rp is not None, int(ds.rule_kind == "epsilon"), int(ds.split and not ds.input_nonneg)
        head.append(DenseStep(
            fwd=_LIN + ("_rule_fwd" if ds.split else "_fwd"), bwd=_LIN + ("_rule_bwd" if rule else "_bwd"),
            signed=signed, wn=bool(signed or ds.negden), relu_mask=int(ds.mask), bcast=int(not ds.split),
            zsign=int(ds.rule_kind == "gamma") if rule else eps_r, xmul=int(ds.split) if rule else eps_r,
            post=POST_NONE if (di > 0 or stop_after == L - 1 or L - 1 in taps) else below))
    return tuple(conv), tuple(head)
