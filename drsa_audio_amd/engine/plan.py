"""LRP kernel plan: compile (model, composite) once, then run batches through HIP kernels.

The reference attaches zennit hooks and lets autograd re-run 1-5 modified forwards per layer (attribute.py:98-107).
Here the sequential VGG structure (create_model.py:8-97, optionally with the ProjectionModel virtual layers,
modify_model.py:19-60) is compiled into *stages*:

  ConvStage   Conv2d [+BN folded by SequentialMergeBatchNorm] -> ReLU
              [-> Projection/SubspaceFilter/InvProjection] [-> MaxPool2d(k) | AvgPool2d(k)]
  DenseStage  Linear [+BN folded] [-> ReLU] [-> Dropout]

in three steps: parse (parse.py, host only: the stages and every structural refusal), prepare (here, once per plan:
the device weight sets, rule-modified, flipped/transposed for the backward, padded to the kernels' channel tiles)
and schedule (schedule.py, once per input shape and call form: which entry point each stage runs).  ``forward``
and ``backward`` only walk the schedule: they get buffers (cached per batch shape, like the schedule) and launch.

Forward: one ``drsa_amd_conv_fwd`` per conv stage computes y = pool(relu(conv)), the pool argmax and the rule's
denominator at the argmax (the only place relevance arrives).  Backward: one ``drsa_amd_conv_bwd`` per conv stage,
the max-pool/ReLU backward folded into its input, the next lower layer's division folded into its output.  The
subspace path fans one forward out into K+1 relevance clones at the projection (``drsa_amd_projection_bwd``),
instead of replicating the batch K+1 times (explainer.py:92).  A MultiProjectionModel's plan holds a table of
projection matrices and runs ``drsa_amd_projection_fwd_multi`` / ``_bwd_multi`` on the per-call ``u_rows`` (the table
index of each row: mixed-class batches in one pass).  A dense stage under Epsilon (or no rule) is one
``drsa_amd_linear_fwd`` and one ``drsa_amd_linear_bwd``; under Gamma / ZPlus its forward also writes the rule's
denominators (``drsa_amd_linear_rule_fwd``) and under Gamma / ZPlus / WSquare / Flat its backward is one
``drsa_amd_linear_rule_bwd`` with a chain per term of R_in (pf.py:18-27, 257-292: the dense rule comes from the
same rule_mapper as the conv rule).  A conv whose kernel is not 3x3 (odd sides up to 7, create_model.py:17,58) runs on
``drsa_amd_convk_fwd`` / ``drsa_amd_convk_bwd`` in the same arithmetic: its pool is a launch of its own, its g dense,
and the denominators on both of its sides per-sample copies.  A stage that ends in AvgPool2d(k) runs
its conv at full resolution, then ``drsa_amd_avgpool_fwd``; on the way back one ``drsa_amd_avgpool_bwd`` takes the raw
relevance at the pool's output through the pool's rule, the ReLU mask and the conv rule's division to a dense g
(DESIGN 18).

Precision: a model whose parameters are bfloat16 (``model.bfloat16()``) compiles a bf16 plan (the
reference has no bf16 path): every conv weight set (rule-modified, forward and backward) is rounded to bf16, the
network input is rounded to bf16, and every conv with Cin > 1 runs forward on ``drsa_amd_conv_fwd_bf16`` (inputs
rounded to bf16 as they are staged, v_mfma_f32_32x32x16_bf16, fp32 accumulation).  Biases, activations,
denominators, the dense head and the whole relevance backward stay fp32 (oracle: ``lrp_ref.lrp(mode="bf16")``).
With ``bf16_backward`` (``DRSA_AMD_BF16_BACKWARD=1``) every backward conv with Cin > 1 (ng = 1) also runs on bf16
operands: ``drsa_amd_conv_bwd_bf16`` rounds the quotient g = R / stab(den) to bf16 as it is staged, accumulates in
fp32, and keeps the epilogue fp32 (oracle: ``mode="bf16bwd"``).
"""
from __future__ import annotations

import os
import weakref
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from .. import _capi
from .._capi import POST_DIV, POST_DIV_MAP, POST_DIV_RING, POST_NONE, XM_MUL, XM_NONE, XM_SPLIT
from .parse import ConvStage, DenseStage, EngineError, _bf16r, _pad32, dense_rule_params, parse   # noqa: F401
from .schedule import (ConvStep, _proj_hw, capture_set, capture_stage, mark_bwd_bf16,   # noqa: F401 (names re-exported)
                       schedule)

# Alternative plan forms, bit-identical to the defaults, that the parity tests switch on to prove it (module
# attributes, not run-time knobs; an engine reads them once, when it is constructed):
# _PROJ_STORE: the projection forward stores h and a' and projection_bwd reads them (instead of recomputing them);
# _DEN_COPY: the WSquare/Flat layer's forward stores its per-sample denominator at the argmax everywhere and the
#   next backward reads it there (POST_DIV) instead of the ring form;
# _POOL24_SPARSE = False: the (2,4) pool backward as a separate unpool before a dense-g backward instead of
#   folded into the backward conv's staging.
_PROJ_STORE = False
_DEN_COPY = False
_POOL24_SPARSE = True


class LRPEngine:
    def __init__(self, model: nn.Module, composite, device: Optional[torch.device] = None,
                 precision: Optional[str] = None, bf16_backward: Optional[bool] = None):
        _capi.load()
        # no strong references to the model / composite: the plan owns prepared copies of what it
        # needs, and get_engine's cache is keyed by weak references (engine/__init__.py)
        self._model_ref = weakref.ref(model)
        self._composite_ref = (lambda: None) if composite is None else weakref.ref(composite)
        p0 = next(model.parameters())
        self.device = device or p0.device
        if precision is None:
            precision = "bf16" if p0.dtype == torch.bfloat16 else "fp32"
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        self.precision, self.bf16 = precision, precision == "bf16"
        # bf16 plan option: the relevance backward convs on bf16 operands too (g rounded to bf16 as it
        # is staged, fp32 accumulation and epilogue); default from DRSA_AMD_BF16_BACKWARD (off)
        self.bf16_backward = self.bf16 and bool(bf16_backward_default() if bf16_backward is None else bf16_backward)
        if self.device.type != "cuda":
            raise _capi.DrsaAmdError("the LRP engine runs on the GPU only; move the model to a HIP device")
        self.stages, self.dense = parse(model, composite, self.bf16)
        mark_bwd_bf16(self.stages, self.bf16_backward)
        for st in self.stages:
            self._prepare_conv(st)
        for ds in self.dense:
            self._prepare_dense(ds)
        self._flags = dict(proj_store=_PROJ_STORE, den_copy=_DEN_COPY, pool24_sparse=_POOL24_SPARSE)
        self._schedules: Dict[tuple, tuple] = {}
        self._buffers: Dict[tuple, dict] = {}
        self.last: Optional[dict] = None
        self.trace: Optional[list] = None      # set to [] to record (tag, start_event, end_event)

    @staticmethod
    def check(model: nn.Module, composite) -> None:
        """The parse step of a plan alone, on the host: raises the EngineError that compiling the
        plan for ``model`` under ``composite`` would raise, and prepares nothing.  Needs no GPU."""
        parse(model, composite)

    model = property(lambda self: self._model_ref())
    composite = property(lambda self: self._composite_ref())

    def release(self) -> None:
        """Free the cached activation/relevance buffers and prepared per-shape state."""
        self._buffers.clear()
        self._schedules.clear()
        self._cur_bufs = {}
        for st in self.stages:
            st.den_maps.clear()
        self.last = None

    def _call(self, tag: str, name: str, *args) -> None:
        if self.trace is None:
            return _capi.call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _capi.call(name, *args)
        e1.record()
        self.trace.append((tag, e0, e1))

    # ---------------------------------------------------------------- prepare
    @torch.no_grad()
    def _prepare_conv(self, st: ConvStage):
        dev = self.device
        W, b = st.W.to(dev), st.b.to(dev)
        cin_p, cin_o, cout_p = (1 if st.cin == 1 else _pad32(st.cin)), _pad32(st.cin), _pad32(st.cout)
        bd = torch.zeros_like(b) if "bias" in getattr(st.rule, "zero_params", ()) else b
        # every weight set the kernels see holds bf16 values in a bf16 plan (forward and backward alike)
        rnd = _bf16r if self.bf16 else (lambda t: t)

        def fwd_layout(*sets):   # [cout][cin][3][3] each -> [ng][9*cin_p][cout_p], row k = ci*9 + ky*3 + kx
            if st.generic:       # not 3x3: the K x K kernels' layout (fp32 plans only: parse)
                return _convk_fwd_layout(sets)
            t = torch.zeros(len(sets), cin_p, 3, 3, cout_p, device=dev)
            for i, Wx in enumerate(sets):
                t[i, :st.cin, :, :, :st.cout] = rnd(Wx).permute(1, 2, 3, 0)
            return t.reshape(len(sets), 9 * cin_p, cout_p)

        def bwd_layout(*sets):   # transposed conv as 'same' conv: [ng][9*cout_p][pad32(cin)], flipped taps
            if st.generic:
                return _convk_bwd_layout(sets)
            t = torch.zeros(len(sets), cout_p, 3, 3, cin_o, device=dev)
            for i, Wx in enumerate(sets):
                t[i, :st.cout, :, :, :st.cin] = rnd(Wx).flip(2, 3).permute(0, 2, 3, 1)
            return t.reshape(len(sets), 9 * cout_p, cin_o)

        bias3 = torch.zeros(3, cout_p, device=dev)
        bias3[0, :st.cout] = b
        k = st.rule_kind
        sets, bsets, st.xmode_bwd = [W], [W], XM_NONE       # no rule: plain gradient
        if k in ("gamma", "zplus"):
            # zennit 0.5.1 Gamma: den+ = (conv(x+; W+) + b+) + conv(x-; W-), the x- term's
            # modifier zeroing the bias (zero_bias). Only den+ is formed: R reaches the
            # conv through its ReLU, so g- = R [z < 0] / den- is 0.  zennit ZPlus: (x+, W+, b+) and
            # (x-, W-, 0) with one shared denominator: the Gamma kernels with the clamped weight sets
            pos, neg = (lambda t: t.clamp(min=0)), (lambda t: t.clamp(max=0))
            if k == "gamma":
                g = st.rule.gamma
                pos, neg = (lambda t: t + g * t.clamp(min=0)), (lambda t: t + g * t.clamp(max=0))
            Wp, Wn = pos(W), neg(W)
            bias3[1, :st.cout], bias3[2, :st.cout] = pos(bd), 0.0
            sets = [W, Wp] + ([Wn] if not st.input_nonneg else [])
            st.xmode_bwd, bsets = (XM_MUL, [Wp]) if st.input_nonneg else (XM_SPLIT, [Wp, Wn])
        elif k == "alphabeta":
            # zennit AlphaBeta on a non-negative input (oracle lrp_ref.py alphabeta): positive set
            # (x, W+, b+) and negative set (x, W-, b-), the x- terms vanish; den_p and den_n come
            # from two Gamma-form forwards (den = (conv(x; W+-) + b+-) + 0)
            Wp, Wn = W.clamp(min=0), W.clamp(max=0)
            bias3[1, :st.cout] = bd.clamp(min=0)
            st.bias3_n = torch.zeros(3, cout_p, device=dev)
            st.bias3_n[0, :st.cout], st.bias3_n[1, :st.cout] = b, bd.clamp(max=0)
            sets, bsets, st.xmode_bwd = [W, Wp], [Wp], XM_MUL
            st.wts_fwd_n, st.wts_bwd_n = fwd_layout(W, Wn), bwd_layout(Wn)
            st.alpha, st.beta = float(st.rule.alpha), float(st.rule.beta)
        elif k == "epsilon":
            bias3[1, :st.cout], st.xmode_bwd = bd, XM_MUL
        elif k in ("wsquare", "flat"):
            W2, b2 = (W * W, bd * bd) if k == "wsquare" else (torch.ones_like(W), torch.zeros_like(b))
            st.W2, st.b2, bsets = rnd(W2.contiguous()), b2.contiguous(), [W2]
            if st.generic:
                # the map is the K x K forward over an all-ones input: den = chain(1; W2) + b2 (bias row 1)
                st.wts_w2, st.bias3_w2 = fwd_layout(W2), torch.zeros(3, cout_p, device=dev)
                st.bias3_w2[1, :st.cout] = b2
            elif st.cin == 1:
                st.w2_first = st.W2.reshape(st.cout, 9).contiguous()
        elif k == "zbox":
            # zennit ZBox: (x; W, b), (l; W+, b+), (h; W-, b-).  b = b+ + b- cancels in the denominator, so
            # zero_params=("bias",) changes only roundings there and nothing in R_in: the plan is the same
            Wr = rnd(W).reshape(st.cout, 9)
            st.zb_wpn = torch.stack([Wr.clamp(min=0), Wr.clamp(max=0)]).contiguous()
            st.zb_bp, st.zb_bn = b.clamp(min=0).contiguous(), b.clamp(max=0).contiguous()
        assert (len(sets), len(bsets)) == (st.ng_fwd, st.ng_bwd)
        st.wts_fwd, st.bias3, st.wts_bwd = fwd_layout(*sets), bias3, bwd_layout(*bsets)
        if self.bf16 and st.cin > 1:
            st.wts_fwd_bf = _bf16_layout(st.wts_fwd, cin_p, cout_p)
            if st.wts_fwd_n is not None:
                st.wts_fwd_n_bf = _bf16_layout(st.wts_fwd_n, cin_p, cout_p)
        if st.bwd_bf16:
            st.wts_bwd_bf = _bf16_layout(st.wts_bwd, cout_p, cin_o)
        if st.proj is not None:
            P = st.proj
            if P.d != st.cout:
                raise EngineError("engine: projection width differs from the conv channels")
            if P.multi:     # the table and, per matrix, its residual
                P.U_tab = P.U_tab.to(dev).contiguous()
                P.P_tab = torch.empty_like(P.U_tab)
                for U, Pm in zip(P.U_tab, P.P_tab):
                    _capi.call("drsa_amd_projection_residual", U.data_ptr(), P.d, Pm.data_ptr(), _capi.stream_ptr(dev))
            else:
                P.U = P.U.to(dev).contiguous()
                P.P = torch.empty_like(P.U)
                _capi.call("drsa_amd_projection_residual", P.U.data_ptr(), P.U.size(0), P.P.data_ptr(),
                           _capi.stream_ptr(dev))

    def _prepare_dense(self, ds: DenseStage):   # the weights and the rule's sets (formed on the host) to the device
        dev = self.device
        ds.W, ds.b = ds.W.to(dev).contiguous(), None if ds.b is None else ds.b.to(dev).contiguous()
        if ds.rp is not None:
            ds.rp = {k: v.to(dev).contiguous() if isinstance(v, torch.Tensor) else v for k, v in ds.rp.items()}

    def _den_map(self, st: ConvStage, H: int, W: int) -> torch.Tensor:
        if (H, W) not in st.den_maps:
            den = st.den_maps[(H, W)] = torch.empty(st.cout, H, W, device=self.device)
            if st.generic:
                ones, scratch = torch.ones(1, st.cin, H, W, device=self.device), torch.empty_like(den)
                _capi.call("drsa_amd_convk_fwd", ones.data_ptr(), st.wts_w2.data_ptr(), st.bias3_w2.data_ptr(), None,
                           scratch.data_ptr(), den.data_ptr(), 1, st.cin, st.cout, H, W, *st.k, 1,
                           _capi.stream_ptr(self.device))
                torch.cuda.current_stream(self.device).synchronize()     # ones / scratch are freed on return
                return den
            _capi.call("drsa_amd_first_layer_den", st.W2.data_ptr(), st.b2.data_ptr(), den.data_ptr(), st.cout,
                       st.cin, H, W, _capi.stream_ptr(self.device))
        return st.den_maps[(H, W)]

    def _den_const4(self, st: ConvStage, H: int, W: int) -> torch.Tensor:
        """[cout][4]: the map's interior value per channel (drsa_amd_first_layer_den computes every
        interior pixel with the same 9-tap chain, so map[c][1][1] is all of them), 4 copies."""
        if ("c4", H, W) not in st.den_maps:
            st.den_maps["c4", H, W] = self._den_map(st, H, W)[:, 1, 1].reshape(-1, 1).expand(-1, 4).contiguous()
        return st.den_maps["c4", H, W]

    def _zbox_maps(self, st: ConvStage, H: int, W: int) -> Tuple[torch.Tensor, ...]:
        """(low_img, high_img [H][W], zl, zh [cout][H][W]) of a ZBox first layer: the bounds spread over one
        sample and the rule's two input-independent maps, made once per input shape like the WSquare map."""
        if ("zbox", H, W) not in st.den_maps:
            lo, hi = (t.reshape(H, W).contiguous() for t in
                      st.rule.bounds(torch.empty(1, 1, H, W, device=self.device)))
            zl, zh = (torch.empty(st.cout, H, W, device=self.device) for _ in range(2))
            _capi.call("drsa_amd_first_layer_zbox_maps", st.zb_wpn[0].data_ptr(), st.zb_bp.data_ptr(),
                       st.zb_wpn[1].data_ptr(), st.zb_bn.data_ptr(), lo.data_ptr(), hi.data_ptr(), zl.data_ptr(),
                       zh.data_ptr(), st.cout, H, W, _capi.stream_ptr(self.device))
            st.den_maps["zbox", H, W] = (lo, hi, zl, zh)
        return st.den_maps["zbox", H, W]

    def _zbox_den(self, st: ConvStage, a, amax, den, B, h, w, s):
        """den = (a - zl) - zh at the argmax pixel (a pooled, with amax) or at every pixel (a at full resolution)."""
        _, _, zl, zh = self._zbox_maps(st, h, w)
        self._call(f"first_layer_zbox_den:{st.name}", "drsa_amd_first_layer_zbox_den", a.data_ptr(), _capi.ptr(amax),
                   zl.data_ptr(), zh.data_ptr(), den.data_ptr(), B, st.cout, h, w, s)

    def _schedule(self, *key, taps: Tuple[int, ...] = ()):
        """The (conv steps, dense steps) of (B, H, W, capture, stop_after, fanout) and the taps, made once per key."""
        if not taps:
            if key not in self._schedules:
                self._schedules[key] = schedule(self.stages, self.dense, *key, bf16=self.bf16, **self._flags)
            return self._schedules[key]
        if key + (taps,) not in self._schedules:
            self._schedules[key + (taps,)] = schedule(self.stages, self.dense, *key, bf16=self.bf16, taps=taps,
                                                      **self._flags)
        return self._schedules[key + (taps,)]

    # ---------------------------------------------------------------- buffers
    def _buf(self, key, shape, dtype=torch.float32, zero=False):
        t = self._cur_bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self._cur_bufs[key] = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
        return t

    def _pad_map(self, key, t: torch.Tensor, hk: int, wk: int) -> torch.Tensor:
        """``t [n][c][h][w]`` copied into the top-left corner of a cached ``[n][c][hk][wk]`` buffer whose
        remainder is zero (zeroed when the buffer is made; only the corner is ever written)."""
        p = self._buf(key, (t.size(0), t.size(1), hk, wk), t.dtype, zero=True)
        p[:, :, :t.size(2), :t.size(3)].copy_(t)
        return p

    # ------------------------------------------------------- matrix per row
    def _multi_proj(self):
        """The plan's multi-matrix projection group (MultiProjectionModel), or None (looked up once)."""
        try:
            return self._multi
        except AttributeError:
            self._multi = next((st.proj for st in self.stages if st.proj is not None and st.proj.multi), None)
            return self._multi

    def _u_rows(self, u_rows, B: int) -> Optional[torch.Tensor]:
        """``u_rows`` (a host sequence or an int tensor [B]: the table index of each row) checked on the host and
        uploaded as the int32 [B] the ``_multi`` kernels read; None for a single-matrix plan.  Per-call data: no
        part of the schedule or of the plan."""
        P = self._multi_proj()
        if P is None:
            if u_rows is not None:
                raise ValueError("u_rows given to a single-matrix plan (ProjectionModel): it has one U for every row; "
                                 "per-row matrices need a MultiProjectionModel")
            return None
        if u_rows is None:
            raise ValueError("this plan has a matrix per row (MultiProjectionModel): pass u_rows, one table index "
                             "per row")
        if isinstance(u_rows, torch.Tensor):
            if u_rows.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
                raise ValueError(f"u_rows must be an integer tensor (got {u_rows.dtype})")
            host = u_rows.detach().reshape(-1).to("cpu", torch.int64)
        else:
            try:
                host = torch.tensor([int(v) for v in u_rows], dtype=torch.int64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"u_rows must be a sequence of table indices or an int tensor [B] ({e})") from None
        if host.numel() != B:
            raise ValueError(f"u_rows has {host.numel()} entries for a batch of {B} rows")
        n_u = P.U_tab.size(0)
        bad = ((host < 0) | (host >= n_u)).nonzero()
        if bad.numel():
            r = int(bad[0])
            raise ValueError(f"u_rows[{r}] = {int(host[r])} is outside the table of {n_u} matrices (row {r})")
        return host.to(torch.int32).to(self.device)

    # ---------------------------------------------------------------- forward
    def _conv_fwd(self, tag, name, st: ConvStage, neg: bool, cur, den_map, out, amax, den, B, h, w, ng, pool, s):
        """One conv forward launch of entry point ``name`` on its weight layout (fp32 or bf16)."""
        bias3 = st.bias3_n if neg else st.bias3
        if name.endswith("_bf16"):
            wts = st.wts_fwd_n_bf if neg else st.wts_fwd_bf
        else:
            wts = st.wts_fwd_n if neg else st.wts_fwd
        if st.generic:      # the K x K forward: no pool, so no argmax
            return self._call(tag, name, cur.data_ptr(), wts.data_ptr(), bias3.data_ptr(), _capi.ptr(den_map),
                              out.data_ptr(), _capi.ptr(den), B, st.cin, st.cout, h, w, *st.k, ng, s)
        self._call(tag, name, cur.data_ptr(), wts.data_ptr(), bias3.data_ptr(), _capi.ptr(den_map), out.data_ptr(),
                   _capi.ptr(amax), _capi.ptr(den), B, st.cin, st.cout, h, w, ng, pool, s)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, capture: Union[None, int, Tuple[int, ...]] = None,
                taps: Tuple[int, ...] = (), u_rows=None) -> torch.Tensor:
        """Model forward with all LRP state (argmax, denominators) kept on device.  ``capture``:
        index of a conv stage, or a tuple of them, whose full-resolution ReLU output is kept even though a
        max-pool follows (the reference's store_hook, preprocessing.py:92-103).  ``taps``: the taps the
        backward will be given (a tapped stage leaves its denominator as a per-sample copy).  ``u_rows``: for a
        MultiProjectionModel plan, the table index of each row's projection matrix (a host sequence or an int
        tensor [B]; checked on the host); the backward of this forward uses the same."""
        _capi.require_gpu(x, "input", dtype=None)
        x = x.detach()
        if self.bf16:
            x = x.to(torch.bfloat16)
        x = x.to(torch.float32).contiguous()
        if x.dim() != 4 or x.size(1) != self.stages[0].cin:
            raise ValueError(f"input must be [B, {self.stages[0].cin}, H, W]")
        B, _, H, W = x.shape
        u_dev = self._u_rows(u_rows, B)
        capture, taps = tuple(capture) if isinstance(capture, (tuple, list)) else capture, tuple(taps)
        conv_steps, dense_steps = self._schedule(B, H, W, capture, None, 0, taps=taps)
        self._cur_bufs = self._buffers.setdefault(("fwd", B, H, W), {})
        s = _capi.stream_ptr(self.device)
        state = {"B": B, "stages": [], "key": (B, H, W, capture), "taps": taps, "tap_rel": {}, "avg_rel": {},
                 "u_rows": u_dev}
        cur = x
        for li, (st, sp) in enumerate(zip(self.stages, conv_steps)):
            (h, w), (ho, wo), C = sp.hw, sp.out_hw, st.cout
            den_map = self._den_map(st, h, w) if st.den_kind == "map" else None
            # the stage's buffers: the full-resolution map a (every form but the fused pool), the pooled
            # y with its argmax bytes, and the denominator the schedule says the stage leaves
            dh, dw = (h, w) if sp.form in ("full", "avg") else (ho, wo)
            a = self._buf((li, "a"), (B, C, h, w)) if sp.form != "fused" else None
            y = amax = den = None
            if sp.form != "full":
                y = self._buf((li, "y"), (B, C, ho, wo))
                amax = self._buf((li, "amax"), (B, C, ho, wo), torch.uint8) if sp.form != "avg" else None
            if sp.den == "ring":
                den = self._buf((li, "den_ring"), (B, C, 2 * (w // 2) + 8 * (h // 2 - 2)))
            elif sp.den == "copy":
                den = self._buf((li, "den"), (B, C, dh, dw))
            tag, out = f"conv_fwd:{st.name}", y if sp.form == "fused" else a
            rec = {"in": cur, "H": h, "W": w, "Hout": ho, "Wout": wo, "a": a, "y": a if y is None else y, "amax": amax,
                   "den": den, "den_map": den_map}
            # ZBox: the conv leaves no denominator; drsa_amd_first_layer_zbox_den forms it from the conv's output
            box = st.den_kind == "box" and den is not None
            if sp.form == "avg":
                # the conv at full resolution with its denominator there (or the shared map, which is not copied),
                # then the average pool on its own: no argmax, nothing gathered
                self._conv_fwd(tag, sp.fwd, st, False, cur, den_map, a, None, den, B, h, w, st.ng_fwd, 0, s)
                self._call(f"avgpool:{st.pool_name}", "drsa_amd_avgpool_fwd", a.data_ptr(), y.data_ptr(), B, C, h, w,
                           *st.pool_k, s)
            elif sp.form == "unfused":
                den_full = self._buf((li, "den_full"), (B, C, h, w)) if den is not None else None
                self._conv_fwd(tag, sp.fwd, st, False, cur, den_map, a, None, None if box else den_full, B, h, w,
                               st.ng_fwd, 0, s)
                if box:
                    self._zbox_den(st, a, None, den_full, B, h, w, s)
                self._call(f"maxpool:{st.pool_name}", "drsa_amd_maxpool_capture", a.data_ptr(), _capi.ptr(den_full),
                           y.data_ptr(), amax.data_ptr(), _capi.ptr(den), B, C, h, w, *st.pool_k, s)
            elif sp.den == "ring":
                rec["den_const4"] = self._den_const4(st, h, w)
                self._call(tag, sp.fwd, cur.data_ptr(), st.wts_fwd.data_ptr(), st.bias3.data_ptr(), den_map.data_ptr(),
                           y.data_ptr(), amax.data_ptr(), den.data_ptr(), B, C, h, w, st.ng_fwd, s)
            else:
                self._conv_fwd(tag, sp.fwd, st, False, cur, den_map, out, amax, None if box else den, B, h, w,
                               st.ng_fwd, sp.pool, s)
                if box:
                    self._zbox_den(st, out, amax, den, B, h, w, s)
            if st.den_kind == "ab":   # second pass: den_n (y and argmax rewritten with the same values)
                rec["den_n"] = self._buf((li, "den_n"), (B, C, dh, dw))
                if sp.form == "unfused":    # a K x K conv under a pool: den_n at full resolution, gathered at the argmax
                    den_n_full = self._buf((li, "den_n_full"), (B, C, h, w))
                    rec["den_ab_full"] = (den_full, den_n_full)     # ab_split runs on the unpooled g
                    self._conv_fwd(f"conv_fwd_n:{st.name}", sp.fwd, st, True, cur, None, a, None, den_n_full, B, h, w, 2,
                                   0, s)
                    self._call(f"maxpool:{st.pool_name}", "drsa_amd_maxpool_capture", a.data_ptr(), den_n_full.data_ptr(),
                               y.data_ptr(), amax.data_ptr(), rec["den_n"].data_ptr(), B, C, h, w, *st.pool_k, s)
                else:
                    self._conv_fwd(f"conv_fwd_n:{st.name}", sp.fwd, st, True, cur, None, out, amax, rec["den_n"], B, h, w,
                                   2, sp.pool, s)
            if st.proj is not None:
                P, (hk, wk, store) = st.proj, sp.proj
                # h and a' are recomputed by projection_bwd from a (no HBM round trip); a' is
                # stored only when it is the stage output (no pool after the projection)
                padded = (hk, wk) != (h, w)
                ak = self._pad_map((li, "a_pad"), a, hk, wk) if padded else a
                hb = self._buf((li, "h"), (B, C, hk * wk)) if store else None
                ap = self._buf((li, "ap"), (B, C, hk, wk)) if (store or not P.pool_after) else None
                pooled = amax = None
                if P.pool_after:
                    pooled = self._buf((li, "y_pad" if padded else "y"), (B, C, hk // 2, wk // 2))
                    amax = self._buf((li, "amax"), (B, C, hk // 2, wk // 2), torch.uint8)
                if P.multi:
                    self._call("projection_fwd", "drsa_amd_projection_fwd_multi", ak.data_ptr(), P.U_tab.data_ptr(),
                               P.P_tab.data_ptr(), u_dev.data_ptr(), P.U_tab.size(0), _capi.ptr(hb), _capi.ptr(ap),
                               _capi.ptr(pooled), _capi.ptr(amax), B, C, hk, wk, 1 if P.pool_after else 0, s)
                else:
                    self._call("projection_fwd", "drsa_amd_projection_fwd", ak.data_ptr(), P.U.data_ptr(),
                               P.P.data_ptr(), _capi.ptr(hb), _capi.ptr(ap), _capi.ptr(pooled), _capi.ptr(amax), B, C,
                               hk, wk, 1 if P.pool_after else 0, s)
                y = pooled if P.pool_after else ap
                if padded:
                    y = self._buf((li, "y" if P.pool_after else "ap_crop"), (B, C, ho, wo))
                    y.copy_((pooled if P.pool_after else ap)[:, :, :ho, :wo])
                rec.update(h=hb, ap=ap, amax=amax, a_k=ak, pad=(hk, wk) if padded else None, y=y)
            state["stages"].append(rec)
            cur = rec["y"]
        flat = cur.reshape(B, -1)
        if flat.size(1) != self.dense[0].W.size(1):
            raise ValueError(f"flattened trunk output {flat.size(1)} != classifier input {self.dense[0].W.size(1)}")
        dense_recs, inp = [], flat
        for di, (ds, dp) in enumerate(zip(self.dense, dense_steps)):
            N, Kd = ds.W.shape
            z = self._buf(("d", di, "z"), (B, N))
            act = self._buf(("d", di, "a"), (B, N)) if ds.relu_after else None
            den_p = den_n = None
            if ds.split:
                # Gamma / ZPlus: z and the rule's denominators in one launch over one staged x
                rp = ds.rp
                den_p = self._buf(("d", di, "den_p"), (B, N))
                den_n = self._buf(("d", di, "den_n"), (B, N)) if ds.negden else None
                self._call(f"linear_rule_fwd:{ds.name}", dp.fwd, inp.data_ptr(), ds.W.data_ptr(), rp["Wp"].data_ptr(),
                           rp["Wn"].data_ptr() if dp.wn else None, _capi.ptr(ds.b), _capi.ptr(rp["bp"]),
                           _capi.ptr(rp["bn"]) if ds.negden else None, z.data_ptr(), _capi.ptr(act), den_p.data_ptr(),
                           _capi.ptr(den_n), dp.signed, B, N, Kd, s)
            else:
                self._call(f"linear_fwd:{ds.name}", dp.fwd, inp.data_ptr(), ds.W.data_ptr(), _capi.ptr(ds.b),
                           z.data_ptr(), _capi.ptr(act), B, N, Kd, s)
            dense_recs.append({"x": inp, "z": z, "a": act, "den_p": den_p, "den_n": den_n})
            inp = act if act is not None else z
        state["dense"], self.last = dense_recs, state
        return dense_recs[-1]["z"]

    # --------------------------------------------------------------- backward
    def _post_args(self, li: int, post: int):
        """(den, eps) of post step ``post``: the denominator conv stage ``li`` left in the form the schedule
        chose for it (POST_DIV_RING: its record, den on the ring and den_const4 elsewhere)."""
        if post not in (POST_DIV, POST_DIV_MAP, POST_DIV_RING):
            return None, 0.0
        rec = self.last["stages"][li]
        return {POST_DIV: rec["den"], POST_DIV_MAP: rec["den_map"], POST_DIV_RING: rec}[post], self.stages[li].eps

    def _conv_bwd(self, st: ConvStage, sp: ConvStep, g, amax_in, den, eps, x_in, out, Bq, s):
        """One conv rule-backward launch, the mirror of _conv_fwd: the schedule's entry point on the fp32 or
        bf16 weight set, with the arguments that entry takes."""
        wts = (st.wts_bwd_bf if sp.wts_bf16 else st.wts_bwd).data_ptr()
        x = x_in.data_ptr() if (st.xmode_bwd != XM_NONE or sp.post != POST_NONE) else None
        tag, shape = f"conv_bwd:{st.name}", (Bq, sp.clones, st.cout, st.cin, *sp.hw)
        if st.generic:      # the K x K backward: dense g, a per-sample den
            return self._call(tag, sp.bwd, g.data_ptr(), wts, x, _capi.ptr(den), out.data_ptr(), *shape, *st.k,
                              st.ng_bwd, st.xmode_bwd, sp.post, float(eps), s)
        if sp.bwd.endswith("_den_ring"):
            self._call(tag, sp.bwd, g.data_ptr(), _capi.ptr(amax_in), wts, int(sp.wts_bf16), x, den["den"].data_ptr(),
                       den["den_const4"].data_ptr(), out.data_ptr(), *shape, st.ng_bwd, st.xmode_bwd, float(eps), s)
        elif sp.bwd.endswith("_den_map"):
            self._call(tag, sp.bwd, g.data_ptr(), _capi.ptr(amax_in), sp.pool_w, wts, int(sp.wts_bf16), x,
                       den.data_ptr(), out.data_ptr(), *shape, st.ng_bwd, st.xmode_bwd, float(eps), s)
        elif sp.bwd.endswith("_bf16_pw"):
            self._call(tag, sp.bwd, g.data_ptr(), amax_in.data_ptr(), sp.pool_w, wts, x, _capi.ptr(den), out.data_ptr(),
                       *shape, st.xmode_bwd, sp.post, float(eps), s)
        else:
            self._call(tag, sp.bwd, g.data_ptr(), _capi.ptr(amax_in), wts, x, _capi.ptr(den), out.data_ptr(), *shape,
                       st.ng_bwd, st.xmode_bwd, sp.post, float(eps), s)

    def _unavg(self, li: int, sp: ConvStep, R_y: torch.Tensor, s) -> torch.Tensor:
        """The way back through the average pool of stage ``li``: from the raw relevance at the pool's output to the
        dense g of the stage's conv backward (the pool's rule, the ReLU mask, the conv rule's own division), and the
        relevance at the ReLU's output when that is captured (``self.last["avg_rel"][li]``), in one launch."""
        st, rec = self.stages[li], self.last["stages"][li]
        (h, w), Bq = sp.hw, R_y.size(0)
        g = self._buf((li, "g_unavg"), (Bq, st.cout, h, w))
        rel = self._buf((li, "rel_full"), (Bq, st.cout, h, w)) if sp.rel_full else None
        den = rec["den_map"] if sp.den == "map" else rec["den"]
        self._call(f"avgpool_bwd:{st.pool_name}", "drsa_amd_avgpool_bwd", R_y.data_ptr(), rec["y"].data_ptr(),
                   rec["a"].data_ptr(), _capi.ptr(den), int(sp.den == "map"), int(st.pool_rule is not None),
                   float(st.pool_eps), float(st.eps), g.data_ptr(), _capi.ptr(rel), Bq, Bq // self.last["B"], st.cout,
                   h, w, *st.pool_k, s)
        if rel is not None:
            self.last["avg_rel"][li] = rel
        return g

    @torch.no_grad()
    def backward(self, seed: Optional[torch.Tensor] = None, cls: Optional[torch.Tensor] = None,
                 one_hot: bool = False, fanout: int = 0, stop_after: Optional[int] = None,
                 taps: Tuple[int, ...] = (), u_rows=None) -> torch.Tensor:
        """Relevance at the input.  ``seed`` [B, n_out] (output relevance) or ``cls`` [B] int32 (lrp_output_modifier
        semantics).  ``fanout``: the projection stage emits K+1 clones per sample (HeatmapGenerator path); otherwise
        rows are treated as the reference's replicated batch.  ``stop_after``: stop once the relevance at the OUTPUT
        of conv stage ``stop_after`` is known and return it (pool resolution when that stage pools).  ``taps``: conv
        stages above ``stop_after`` (ascending; the forward was given the same) whose output relevance is recorded
        on the way down, ``self.last["tap_rel"][stage]``: the buffer the launch above wrote without its post step,
        readable until the next call; drsa_amd_relevance_post then makes the g the walk goes on with.  ``u_rows``
        (MultiProjectionModel plans): default, the forward's; given, checked like the forward's and used instead
        (with ``fanout`` 0 one index per replicated row, as the forward saw them)."""
        st0 = self.last
        if st0 is None:
            raise RuntimeError("backward() before forward()")
        B, taps = st0["B"], tuple(taps)
        if taps != st0["taps"]:
            raise ValueError(f"backward(taps={taps}) after forward(taps={st0['taps']}): they must be the same")
        u_dev = st0["u_rows"] if u_rows is None else self._u_rows(u_rows, B)
        conv_steps, dense_steps = self._schedule(*st0["key"], stop_after, fanout, taps=taps)
        s = _capi.stream_ptr(self.device)
        self._cur_bufs = self._buffers.setdefault(("bwd", B, fanout), {})
        # ---- dense head, top-down ----
        L, R = len(self.stages), seed
        for di in range(len(self.dense) - 1, -1, -1):
            ds, dp, rec = self.dense[di], dense_steps[di], st0["dense"][di]
            N, Kd = ds.W.shape
            out = self._buf(("d", di), (B, Kd))
            den, eps_post = self._post_args(L - 1, dp.post)
            den_flat = None if den is None else den.reshape(B, -1)
            # the relevance entering the layer: the fused class seed at the top, else R
            if di == len(self.dense) - 1 and cls is not None:
                seed_args = (None, cls.data_ptr(), 1 if one_hot else 0)
            else:
                if R is None:
                    raise ValueError("backward needs a seed or class indices")
                R = R.to(self.device, torch.float32).contiguous()
                seed_args = (R.data_ptr(), None, 0)
            head, x = (*seed_args, rec["z"].data_ptr(), dp.relu_mask), rec["x"].data_ptr()
            tail = (_capi.ptr(den_flat), dp.post, eps_post, out.data_ptr(), B, N, Kd, s)
            if ds.rp is None:
                self._call(f"linear_bwd:{ds.name}", dp.bwd, *head, dp.zsign, ds.eps, ds.W.data_ptr(), x, dp.xmul, *tail)
            else:
                # Gamma / ZPlus / WSquare / Flat: one launch, every term of R_in its own chain over one staged g
                rp = ds.rp
                if ds.split:
                    dn_p, dn_n, Wp, Wn = rec["den_p"], rec["den_n"], rp["Wp"], rp["Wn"] if dp.wn else None
                else:
                    dn_p, dn_n, Wp, Wn = rp["den"], None, rp["W2"], None
                self._call(f"linear_rule_bwd:{ds.name}", dp.bwd, *head, dn_p.data_ptr(), _capi.ptr(dn_n), dp.bcast,
                           dp.zsign, ds.eps, Wp.data_ptr(), _capi.ptr(Wn), x, dp.xmul, dp.signed, *tail)
            R = out
        # ---- conv trunk, top-down ----
        g = R.reshape(B, self.stages[-1].cout, *conv_steps[-1].out_hw)
        for li in range(L - 1, -1, -1):
            if stop_after is not None and li == stop_after:
                if conv_steps[li].rel_full:     # the captured ReLU of an average-pooled stage: its relevance is the
                    self._unavg(li, conv_steps[li], g, s)       # pool backward's by-product
                return g
            st, sp, rec = self.stages[li], conv_steps[li], st0["stages"][li]
            (h, w), clones, Bq = sp.hw, sp.clones, B * sp.clones
            if li in taps:
                # g is the raw relevance at this stage's output; the post step the launch above left out, into a
                # buffer of its own
                st0["tap_rel"][li] = g
                if sp.tap_post != POST_NONE:
                    gt, (den, eps) = self._buf((li, "tap_g"), tuple(g.shape)), self._post_args(li, sp.tap_post)
                    self._call(f"tap_post:{st.pool_name if st.pool else st.relu_name}", "drsa_amd_relevance_post",
                               g.data_ptr(), rec["y"].data_ptr(), _capi.ptr(den), gt.data_ptr(), Bq, clones,
                               g.numel() // Bq, sp.tap_post, float(eps), s)
                    g = gt
            amax_in = rec["amax"] if sp.g_in == "sparse" else None
            if sp.g_in == "proj":
                P = st.proj
                if not P.mask:
                    raise EngineError("engine: projection without SubspaceHook is not supported yet")
                G = self._buf((li, "G"), (Bq, st.cout, h, w))
                denk = rec["den"] if st.den_kind not in (None, "ab") else None
                hk, wk, store = sp.proj
                gk, Gk = g, G
                if rec["pad"]:      # the forward's zero-padded map: g and den padded alike, G cropped
                    gk = self._pad_map((li, "g_pad"), g, *((hk // 2, wk // 2) if P.pool_after else (hk, wk)))
                    denk = None if denk is None else self._pad_map((li, "den_pad"), denk, hk, wk)
                    Gk = self._buf((li, "G_pad"), (Bq, st.cout, hk, wk))
                head = (gk.data_ptr(), _capi.ptr(rec["amax"] if P.pool_after else None),
                        _capi.ptr(rec["ap"] if store else None), _capi.ptr(rec["h"]), rec["a_k"].data_ptr(),
                        _capi.ptr(denk))
                tail = (Gk.data_ptr(), B, st.cout, hk, wk, P.K, P.eps_inv, st.eps if denk is not None else 0.0,
                        int(fanout), s)
                if P.multi:
                    self._call("projection_bwd", "drsa_amd_projection_bwd_multi", *head, P.U_tab.data_ptr(),
                               P.P_tab.data_ptr(), u_dev.data_ptr(), P.U_tab.size(0), *tail)
                else:
                    self._call("projection_bwd", "drsa_amd_projection_bwd", *head, P.U.data_ptr(), P.P.data_ptr(), *tail)
                if rec["pad"]:
                    G.copy_(Gk[:, :, :h, :w])
                g = G
            elif sp.g_in == "unavg":
                g = self._unavg(li, sp, g, s)
            elif sp.g_in == "unpool":
                gf = self._buf((li, "g_unpool"), (Bq, st.cout, h, w))
                self._call(f"maxpool_bwd:{st.pool_name}", "drsa_amd_relevance_unpool", g.data_ptr(),
                           rec["amax"].data_ptr(), Bq, clones, st.cout, h, w, *st.pool_k, gf.data_ptr(), s)
                g = gf
            # rule backward of conv li, with the post step of the layer below
            x_in = rec["in"]
            den, eps = self._post_args(li - 1, sp.post)
            out = self._buf((li, "R"), (Bq, st.cin, h, w))
            if sp.bwd == "drsa_amd_first_layer_bwd":
                self._call(f"first_layer_bwd:{st.name}", sp.bwd, g.data_ptr(), _capi.ptr(amax_in),
                           st.w2_first.data_ptr(), out.data_ptr(), Bq, clones, st.cout, h, w, s)
            elif sp.bwd == "drsa_amd_first_layer_zbox_bwd":
                lo, hi, _, _ = self._zbox_maps(st, h, w)
                self._call(f"first_layer_bwd:{st.name}", sp.bwd, g.data_ptr(), _capi.ptr(amax_in),
                           st.zb_wpn.data_ptr(), x_in.data_ptr(), lo.data_ptr(), hi.data_ptr(), out.data_ptr(), Bq,
                           clones, st.cout, h, w, s)
            elif st.den_kind == "ab":
                # R (ReLU-masked) at the conv output -> gp, gn -> two backward convs -> combine + post
                n_out = g.numel() // Bq
                gp, gn = (self._buf((li, k), tuple(g.shape)) for k in ("ab_gp", "ab_gn"))
                # g was unpooled (a K x K conv under a pool): the denominators at full resolution
                den_p, den_n = rec["den_ab_full"] if sp.g_in == "unpool" else (rec["den"], rec["den_n"])
                self._call(f"ab_split:{st.name}", "drsa_amd_ab_split", g.data_ptr(), den_p.data_ptr(),
                           den_n.data_ptr(), gp.data_ptr(), gn.data_ptr(), Bq, clones, n_out, float(st.eps), s)
                pos, neg = (self._buf((li, k), (Bq, st.cin, h, w)) for k in ("ab_pos", "ab_neg"))
                for gg, wts, dst in ((gp, st.wts_bwd, pos), (gn, st.wts_bwd_n, neg)):
                    if st.generic:
                        self._call(f"conv_bwd:{st.name}", sp.bwd, gg.data_ptr(), wts.data_ptr(), x_in.data_ptr(), None,
                                   dst.data_ptr(), Bq, clones, st.cout, st.cin, h, w, *st.k, 1, XM_MUL, POST_NONE, 0.0, s)
                        continue
                    self._call(f"conv_bwd:{st.name}", sp.bwd, gg.data_ptr(), _capi.ptr(amax_in),
                               wts.data_ptr(), x_in.data_ptr(), None, dst.data_ptr(), Bq, clones, st.cout, st.cin, h, w,
                               1, XM_MUL, POST_NONE, 0.0, s)
                self._call(f"ab_combine:{st.name}", "drsa_amd_ab_combine", pos.data_ptr(), neg.data_ptr(), st.alpha,
                           st.beta, x_in.data_ptr() if sp.post != POST_NONE else None, _capi.ptr(den), out.data_ptr(),
                           Bq, clones, st.cin * h * w, sp.post, float(eps), s)
            else:
                self._conv_bwd(st, sp, g, amax_in, den, eps, x_in, out, Bq, s)
            g = out
        return g

    # ------------------------------------------------------------ DRSA data
    def capture_stage(self, layer_name: str) -> Tuple[int, str]:
        """(stage index, "relu" | "pool") of a trunk module name (features.<layer_idx>)."""
        return capture_stage(self.stages, layer_name)

    def _captured(self, li: int, where: str, R: torch.Tensor) -> dict:
        """What capture() returns for the ReLU or the pool of stage ``li``, whose output relevance is ``R``."""
        st, rec = self.stages[li], self.last["stages"][li]
        if where == "pool":
            return {"act": rec["y"], "rel": R, "amax": None, "H": rec["Hout"], "W": rec["Wout"], "C": st.cout,
                    "ph": 1, "pw": 1}
        if st.avg:      # the relevance at the ReLU above an average pool is dense: drsa_amd_avgpool_bwd wrote it
            return {"act": rec["a"], "rel": self.last["avg_rel"][li], "amax": None, "H": rec["H"], "W": rec["W"],
                    "C": st.cout, "ph": 1, "pw": 1}
        return {"act": rec["a"], "rel": R, "amax": rec["amax"] if st.pool else None, "H": rec["H"], "W": rec["W"],
                "C": st.cout, "ph": st.pool_k[0], "pw": st.pool_k[1]}

    @torch.no_grad()
    def capture(self, x: torch.Tensor, layer_name: str, cls: Optional[torch.Tensor] = None, one_hot: bool = False,
                seed_fn=None) -> dict:
        """get_intermediate (preprocessing.py:106-176) for one batch: forward, LRP backward down to layer
        ``layer_name`` only, and that layer's activation and relevance.  The relevance of a pooled ReLU output is
        returned pooled with its argmax (``amax``); the activation is the full map."""
        li, where = self.capture_stage(layer_name)
        st = self.stages[li]
        out = self.forward(x, capture=li if (where == "relu" and st.pool) else None)
        if seed_fn is not None:
            R = self.backward(seed=seed_fn(out).contiguous(), stop_after=li)
        else:
            R = self.backward(cls=cls, one_hot=one_hot, stop_after=li)
        return self._captured(li, where, R)

    @torch.no_grad()
    def capture_many(self, x: torch.Tensor, layer_names: Sequence[str], cls: Optional[torch.Tensor] = None,
                     one_hot: bool = False, seed_fn=None) -> Dict[str, dict]:
        """capture() for several layers in one pass: one forward that keeps every named ReLU map, and one LRP
        backward down to the lowest named layer that records the relevance at each named layer on its way.
        {name: what capture(x, name) returns}, bit for bit; the tensors are the engine's buffers, valid until its
        next call."""
        names = list(layer_names)
        where, keep, stop, taps = capture_set(self.stages, names)
        out = self.forward(x, capture=keep, taps=taps)
        if seed_fn is not None:
            R = self.backward(seed=seed_fn(out).contiguous(), stop_after=stop, taps=taps)
        else:
            R = self.backward(cls=cls, one_hot=one_hot, stop_after=stop, taps=taps)
        rel = {stop: R, **self.last["tap_rel"]}
        return {n: self._captured(li, wh, rel[li]) for n, (li, wh) in zip(names, where)}

    # -------------------------------------------------------------- heatmaps
    @torch.no_grad()
    def subspace_heatmaps(self, x: torch.Tensor, class_idx=None, cls: Optional[torch.Tensor] = None,
                          one_hot: bool = False, standard: str = "sum", u_rows=None) -> dict:
        """HeatmapGenerator.generate_subspace_heatmaps on device: one shared forward, the top backward once,
        relevance clones below the projection, then split/sum/sort.  ``standard="sum"``: K clones, the standard
        heatmap is the sum of the K concept heatmaps (every rule is linear in the relevance, so this is clone 0 up to
        fp32 rounding; the bottom of the network runs K instead of K+1 times).  ``"clone"``: K+1 clones, the standard
        heatmap is clone 0 as in the reference's replicated batch (explainer.py:92).  ``u_rows``: the table index of
        each row's matrix, for a MultiProjectionModel plan (required there, refused elsewhere)."""
        if standard not in ("sum", "clone"):
            raise ValueError("standard must be 'sum' or 'clone'")
        proj = [st.proj for st in self.stages if st.proj is not None]
        if len(proj) != 1 or not proj[0].mask:
            raise EngineError("subspace heatmaps need exactly one projection group with a SubspaceHook")
        K = proj[0].K
        self.forward(x, u_rows=u_rows)
        B = x.size(0)
        if cls is None:
            cls = torch.full((B,), int(class_idx), dtype=torch.int32, device=self.device)
        ssum = standard == "sum"
        hm = self.backward(cls=cls, one_hot=one_hot, fanout=2 if ssum else 1)   # [B*(K or K+1), 1, H, W]
        H, W = hm.shape[-2:]
        out = {
            "standard_heatmaps": torch.empty(B, 1, H, W, device=self.device),
            "standard_relevance": torch.empty(B, device=self.device),
            "subspace_heatmaps": torch.empty(B, K, H, W, device=self.device),
            "subspace_relevances": torch.empty(B, K, device=self.device),
            "mask": torch.empty(B, K, dtype=torch.int64, device=self.device),
        }
        self._call("heatmap_sort", "drsa_amd_heatmap_sort", hm.data_ptr(), B, K, H * W, 1 if ssum else 0,
                   out["standard_heatmaps"].data_ptr(), out["standard_relevance"].data_ptr(),
                   out["subspace_heatmaps"].data_ptr(), out["subspace_relevances"].data_ptr(), out["mask"].data_ptr(),
                   _capi.stream_ptr(self.device))
        return out


def bf16_backward_default() -> bool:
    """DRSA_AMD_BF16_BACKWARD=1: bf16 plans also run the relevance backward convs on bf16 operands."""
    return os.environ.get("DRSA_AMD_BF16_BACKWARD", "0") not in ("", "0")


def _bf16_layout(wf: torch.Tensor, cin_p: int, cout_p: int) -> torch.Tensor:
    """[ng][9*cin_p][cout_p] fp32 (row k = ci*9 + tap) -> [ng][cin_p/16][9][2][cout_p][8] bf16,
    input channel ci = 16*chunk + 8*half + j (drsa_amd_conv_fwd_bf16, include/drsa_amd.h)."""
    t = wf.reshape(wf.size(0), cin_p // 16, 2, 8, 9, cout_p).permute(0, 1, 4, 2, 5, 3)
    return t.to(torch.bfloat16).contiguous()


def _convk_fwd_layout(sets: Sequence[torch.Tensor]) -> torch.Tensor:
    """Forward-shaped weight sets [cout][cin][kh][kw] -> [ng][cin_p * kh * kw][cout_p] fp32, row
    k = (ci * kh + ky) * kw + kx, cin_p = cin rounded up to 2, cout_p to 32, padding zero
    (drsa_amd_convk_fwd, include/drsa_amd.h)."""
    cout, cin, kh, kw = sets[0].shape
    cin_p, cout_p = (cin + 1) // 2 * 2, _pad32(cout)
    t = torch.zeros(len(sets), cin_p, kh, kw, cout_p, device=sets[0].device)
    for i, w in enumerate(sets):
        t[i, :cin, :, :, :cout] = w.permute(1, 2, 3, 0)
    return t.reshape(len(sets), cin_p * kh * kw, cout_p).contiguous()


def _convk_bwd_layout(sets: Sequence[torch.Tensor]) -> torch.Tensor:
    """The transposed conv as a 'same' conv over g: [ng][cout_p * kh * kw][cin_p] fp32 with cout_p = cout
    rounded up to 2 and cin_p = cin to 32, row (co * kh + ky) * kw + kx = w[co][:, kh-1-ky, kw-1-kx]
    (drsa_amd_convk_bwd)."""
    cout, cin, kh, kw = sets[0].shape
    cout_p, cin_p = (cout + 1) // 2 * 2, _pad32(cin)
    t = torch.zeros(len(sets), cout_p, kh, kw, cin_p, device=sets[0].device)
    for i, w in enumerate(sets):
        t[i, :cout, :, :, :cin] = w.flip(2, 3).permute(0, 2, 3, 1)
    return t.reshape(len(sets), cout_p * kh * kw, cin_p).contiguous()
