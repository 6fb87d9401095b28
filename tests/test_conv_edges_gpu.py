"""The 3x3 conv kernels (csrc/lrp_conv_kernel.h and its parts, the conv_*.hip tables, conv_small.hip,
conv_first.hip) at partial tiles and
padded channel counts, through the C ABI, against the CPU reference tests/conv_ref.py (GPU).

fp32: every output is bit-identical to the reference (oracle/lrp_exact.c's k-ordered fma chains plus
elementwise fp32 steps): torch.equal, NaN positions compared separately.  bf16: the reference, the
elementwise bound and the argmax rule of tests/test_bf16_gpu.py / test_bf16_bwd_gpu.py with their
KTOL.  tests/test_conv_ref_cpu.py checks the reference itself and that the inputs can show a halo,
tie or mask mistake in the last row, the last column and the corner.

Harness: every output is a view into a larger allocation with 4096 sentinel elements on either
side, prefilled with a marked NaN (bytes: 0xEE); after the call the sentinels are untouched and no
element of the view still holds the prefill.  An output that is not requested is passed as null.
Every case first asserts its ``*_has_kernel*`` query; none is skipped.

Shapes (H, W), the smallest that reach each path:
  (12, 40)  H = 8 + 4; W = 32 + 8 / 16 + 16 + 8 / 5 x 8 by the pair's wide tile; W/2 = 20 aligned sparse staging
  (6, 12)   one partial tile per row on 8 x 8 and 4 x 8 tiles; W/2 = 6 per-cell sparse staging
  (10, 20)  W/2 = 10 per-cell sparse staging
  (6, 36)   W >= 32 with W/2 = 18 per-cell sparse staging and W % 8 != 0
  (6, 10), (12, 34)  pooled forward only: W % 4 != 0, the scalar dense staging
  (12, 48), (12, 80) the 2x4 pool: forward pool = 2, backward pool_w = 4 (drsa_amd_conv_bwd_den_map)
Channel pairs (forward cin -> cout; the backward calls mirror them): 1->32, 1->64 (the generic
Cin = 1 kernels at pool = 0 and at pool = 1 with W % 8 != 0; conv_first.hip at (12, 40) pool = 1),
20->32, 32->48, 64->64, 64->100, 100->128, 128->128.
Batch: two distinct samples, run as 3 rows (x clones) and, where an 8 x 8 entry serves the shape,
also as ceil(512 / tiles) rows so that the 8 x 8 kernel runs instead of its 4 x 8 stand-in; the
samples are replicated, the reference is computed for the two, every replica is checked.

Dropped from the cross product (tests/conv_ref.py builds the lists): per (pair, shape, pool) the
forward runs two of the seven (ng, den) combinations {1, 2, 3} x {none, computed} + (1, map),
rotating, so every pair runs on both of its tiles (the wide one and 8 x 8) and every combination runs on every
tile shape; per (pair, shape, dense / sparse g) the backward runs two of the four modes, rotating so
that every pair sees all eight (g, mode) combinations on each of its tiles; the 2x4 pool and the
den_map / den_ring entry points run on the pairs listed there, not on all eight; bf16 runs three
pairs (+ 64->64 for the 2x4 pool) on four shapes with ng rotating.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr
from drsa_audio_amd import _capi
from test_bf16_gpu import KTOL, _r, _ref as _bf16_fwd_ref
from test_conv_small_gpu import _rep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 4096
NAN_FILL = 0x7FC0BEEF        # a quiet NaN no arithmetic produces
SENTINEL = {torch.float32: -12345.0, torch.uint8: 0x5A}


class Guard:
    """An output buffer between two runs of sentinels, prefilled with a marked NaN (bytes: 0xEE)."""

    def __init__(self, shape, dtype=torch.float32):
        n = 1
        for d in shape:
            n *= d
        self.n, self.dtype = n, dtype
        self.buf = torch.full((n + 2 * PAD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(shape)
        if dtype == torch.uint8:
            self.view.fill_(0xEE)
        else:
            self.view.view(torch.int32).fill_(NAN_FILL)
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        s = SENTINEL[self.dtype]
        assert bool((self.buf[:PAD] == s).all()) and bool((self.buf[PAD + self.n:] == s).all()), "sentinel overwritten"
        if self.dtype == torch.uint8:
            assert bool((self.view != 0xEE).all()), "amax element not written"
        else:
            assert bool((self.view.view(torch.int32) != NAN_FILL).all()), "output element not written"
        return self.view.cpu()


def _same(got, want, what):
    """Bit-for-bit up to NaN payloads: equal NaN positions, torch.equal elsewhere."""
    assert got.shape == want.shape, what
    if got.is_floating_point():
        assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN positions"
        got, want = torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.size(0)} of {got.numel()} differ, first at {i}: got {got[i]} want {want[i]}")


def _cid(case):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)


# ------------------------------------------------------------------ fp32 forward
@functools.lru_cache(maxsize=4)
def _fwd_shared(cin, cout, H, W, ng):
    return cr.fwd_inputs(cin, cout, H, W, ng), {}


def _out_hw(H, W, pool):
    return (H // 2, W // (4 if pool == 2 else 2)) if pool else (H, W)


@pytest.mark.parametrize("case", sorted(cr.fwd_cases()), ids=_cid)
def test_conv_fwd_edges(case):
    cin, cout, H, W, ng, pool, den = case
    lib = _capi.lib()
    assert lib.drsa_amd_conv_fwd_has_kernel(cin, cout, W, ng, pool, 0) == 1
    (x, sets, bias3, den_map), memo = _fwd_shared(cin, cout, H, W, ng)
    kind = den.split("_")[0]
    y_ref, am_ref, d_ref = cr.conv_fwd_ref(x, sets, bias3, pool, kind, den_map, memo=memo)
    wd, bd = cr.pack_fwd(sets).to(DEV), cr.pack_bias(bias3, cout).to(DEV)
    assert wd.numel() == lib.drsa_amd_conv_weight_floats(cin, cout, ng)
    dm = None
    if den == "map":
        dm = den_map.to(DEV).contiguous()
    elif den == "map_unaligned":          # a map pointer off the 16-byte grid (the map is gathered per pixel)
        dm = torch.cat([torch.zeros(1), den_map.flatten()]).to(DEV)[1:]
        assert pool and dm.data_ptr() % 16 != 0
    Ho, Wo = _out_hw(H, W, pool)
    for B in cr.batches(True, cin, cout, H, W):
        xb = _rep(x, B).to(DEV)
        out = Guard((B, cout, Ho, Wo))
        am = Guard((B, cout, Ho, Wo), torch.uint8) if pool else None
        dn = Guard((B, cout, Ho, Wo)) if kind != "none" else None
        _capi.call("drsa_amd_conv_fwd", xb.data_ptr(), wd.data_ptr(), bd.data_ptr(), _capi.ptr(dm), out.ptr(),
                   am.ptr() if am else None, dn.ptr() if dn else None, B, cin, cout, H, W, ng, pool,
                   _capi.stream_ptr(DEV))
        torch.cuda.synchronize()
        if pool:
            _same(am.result(), _rep(am_ref, B), f"amax B={B}")
        _same(out.result(), _rep(y_ref, B), f"out B={B}")
        if dn:
            _same(dn.result(), _rep(d_ref, B), f"den B={B}")


# ------------------------------------------------------------------ fp32 backward
def _bwd_run(entry, cin, cout, H, W, pw, ng, xmode, post, clones, gin, am, sets, x, den, ref, extra=None):
    """One backward entry point at every batch size of the shape; cin -> cout is the forward pair.
    entry: "bwd", "map" (den [cin][H][W] shared) or "ring" (extra = (den_ring, c4); also checked
    against POST_DIV on the full copy den)."""
    lib = _capi.lib()
    wd = cr.pack_bwd(sets).to(DEV)
    assert wd.numel() == lib.drsa_amd_conv_weight_floats(cout, cin, ng)
    s = _capi.stream_ptr(DEV)
    need_x = xmode != cr.XM_NONE or post != cr.POST_NONE
    for Bq in cr.batches(False, cout, cin, H, W, clones):
        S = Bq // clones
        gb = _rep(gin, Bq).to(DEV)
        ab = _rep(am, S).to(DEV) if am is not None else None
        xb = _rep(x, S).to(DEV) if need_x else None
        out = Guard((Bq, cin, H, W))
        if entry == "bwd":
            db = _rep(den, S).to(DEV) if post == cr.POST_DIV else None
            _capi.call("drsa_amd_conv_bwd", gb.data_ptr(), _capi.ptr(ab), wd.data_ptr(), _capi.ptr(xb), _capi.ptr(db),
                       out.ptr(), Bq, clones, cout, cin, H, W, ng, xmode, post, cr.EPS, s)
        elif entry == "map":
            db = den.to(DEV).contiguous()
            _capi.call("drsa_amd_conv_bwd_den_map", gb.data_ptr(), _capi.ptr(ab), pw or 2, wd.data_ptr(), 0,
                       xb.data_ptr(), db.data_ptr(), out.ptr(), Bq, clones, cout, cin, H, W, ng, xmode, cr.EPS, s)
        else:
            ring, c4 = extra
            rb, cb, db = _rep(ring, S).to(DEV), c4.to(DEV).contiguous(), _rep(den, S).to(DEV)
            _capi.call("drsa_amd_conv_bwd_den_ring", gb.data_ptr(), _capi.ptr(ab), wd.data_ptr(), 0, xb.data_ptr(),
                       rb.data_ptr(), cb.data_ptr(), out.ptr(), Bq, clones, cout, cin, H, W, ng, xmode, cr.EPS, s)
            full = Guard((Bq, cin, H, W))
            _capi.call("drsa_amd_conv_bwd", gb.data_ptr(), _capi.ptr(ab), wd.data_ptr(), xb.data_ptr(), db.data_ptr(),
                       full.ptr(), Bq, clones, cout, cin, H, W, ng, xmode, cr.POST_DIV, cr.EPS, s)
        torch.cuda.synchronize()
        got = out.result()
        _same(got, _rep(ref, Bq), f"{entry} Bq={Bq}")
        if entry == "ring":
            _same(full.result(), got, f"POST_DIV on the full copy Bq={Bq}")


@pytest.mark.parametrize("case", cr.bwd_cases(), ids=_cid)
def test_conv_bwd_edges(case):
    cin, cout, H, W, sparse, (ng, xmode, post, clones) = case
    # the query of the pool-sparse g; the ABI has none for a dense g, which the same tables serve
    assert _capi.lib().drsa_amd_conv_bwd_has_kernel_pw(cout, cin, W, ng, 2) == 1
    pw = 2 if sparse else 0
    gin, am, sets, x, den = cr.bwd_inputs(cin, cout, H, W, ng, pw, clones)
    ref = cr.conv_bwd_ref(gin, am, pw, sets, x, den, clones, xmode, post, cr.EPS)
    _bwd_run("bwd", cin, cout, H, W, pw, ng, xmode, post, clones, gin, am, sets, x, den, ref)


@pytest.mark.parametrize("case", cr.den_map_cases(), ids=_cid)
def test_conv_bwd_den_map_edges(case):
    cin, cout, H, W, pw, xmode = case
    assert _capi.lib().drsa_amd_conv_bwd_has_kernel_pw(cout, cin, W, 1, pw or 2) == 1
    clones = 2
    gin, am, sets, x, den = cr.bwd_inputs(cin, cout, H, W, 1, pw, clones, shared_den=True)
    ref = cr.conv_bwd_ref(gin, am, pw, sets, x, den, clones, xmode, cr.POST_DIV, cr.EPS, den_shared=True)
    _bwd_run("map", cin, cout, H, W, pw, 1, xmode, cr.POST_DIV, clones, gin, am, sets, x, den, ref)


@pytest.mark.parametrize("case", cr.den_ring_cases(), ids=_cid)
def test_conv_bwd_den_ring_edges(case):
    cin, cout, H, W, sparse, xmode = case
    assert _capi.lib().drsa_amd_conv_bwd_has_kernel_pw(cout, cin, W, 1, 2) == 1
    clones, pw = 2, 2 if sparse else 0
    gin, am, sets, x, den, ring, c4 = cr.ring_inputs(cin, cout, H, W, sparse, clones)
    ref = cr.conv_bwd_ref(gin, am, pw, sets, x, den, clones, xmode, cr.POST_DIV, cr.EPS)
    _bwd_run("ring", cin, cout, H, W, pw, 1, xmode, cr.POST_DIV, clones, gin, am, sets, x, den, ref, (ring, c4))


# ------------------------------------------------------------------ bf16
@pytest.mark.parametrize("case", cr.bf16_fwd_cases(), ids=_cid)
def test_conv_fwd_bf16_edges(case):
    """tests/test_bf16_gpu.py's test_conv_fwd_bf16_kernel (reference, bound, argmax rule) at the
    edge shapes, in the sentinel harness."""
    cin, cout, H, W, ng, pool = case
    lib = _capi.lib()
    assert lib.drsa_amd_conv_fwd_has_kernel(cin, cout, W, ng, pool, 1) == 1
    x, sets, bias3, _ = cr.fwd_inputs(cin, cout, H, W, ng)
    x = torch.nan_to_num(x, nan=0.5)
    if ng < 3:
        x = x.clamp(min=0)                # ng = 1 / 2: the non-negative input contract of the forward sets
    y, den, sc = _bf16_fwd_ref(x, sets, bias3, ng)
    bound = KTOL * (sc + bias3.abs().sum(0).double()[None, :, None, None]) + 1e-30
    wb = cr.pack_bf16(cr.pack_fwd([_r(s) for s in sets], bf16=True)).to(DEV)
    assert wb.numel() == lib.drsa_amd_conv_weight_bf16_elems(cin, cout, ng)
    bd, xd = cr.pack_bias(bias3, cout).to(DEV), x.to(DEV).contiguous()
    B = x.size(0)
    Ho, Wo = _out_hw(H, W, pool)
    out, dn = Guard((B, cout, Ho, Wo)), Guard((B, cout, Ho, Wo))
    am = Guard((B, cout, Ho, Wo), torch.uint8) if pool else None
    _capi.call("drsa_amd_conv_fwd_bf16", xd.data_ptr(), wb.data_ptr(), bd.data_ptr(), None, out.ptr(),
               am.ptr() if am else None, dn.ptr(), B, cin, cout, H, W, ng, pool, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    o, dg = out.result().double(), dn.result().double()
    if not pool:
        assert torch.all((o - y).abs() <= bound) and torch.all((dg - den).abs() <= bound)
        return
    pw = 4 if pool == 2 else 2
    a = am.result().long()
    win, bwin = cr.windows(y, pw), cr.windows(bound, pw)
    assert torch.all((o - win.max(-1).values).abs() <= bwin.max(-1).values)
    top2 = win.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * bwin.max(-1).values
    assert clear.any() and torch.equal(a[clear], win.argmax(-1)[clear])
    dref = torch.gather(cr.windows(den, pw), -1, a[..., None])[..., 0]
    bsel = torch.gather(bwin, -1, a[..., None])[..., 0]
    assert torch.all((dg - dref).abs() <= bsel)


@pytest.mark.parametrize("case", cr.bf16_bwd_cases(), ids=_cid)
def test_conv_bwd_bf16_edges(case):
    """tests/test_bf16_bwd_gpu.py's test_conv_bwd_bf16_kernel (reference and bounds) at the edge
    shapes, with drsa_amd_conv_bwd_bf16_pw for pool_w = 4 (and pool_w = -2: that entry point at
    pool width 2), in the sentinel harness."""
    cin, cout, H, W, pwc = case
    lib = _capi.lib()
    pw, via_pw = abs(pwc), pwc in (4, -2)
    if pw:
        assert lib.drsa_amd_conv_bwd_has_kernel_bf16_pw(cout, cin, W, pw) == 1
    else:
        assert lib.drsa_amd_conv_bwd_has_kernel_bf16(cout, cin, W, 1, 0) == 1
    clones = 2
    gin, am, sets, x, den = cr.bwd_inputs(cin, cout, H, W, 1, pw, clones)
    x = x.clamp(min=0)
    w = sets[0]
    wb = cr.pack_bf16(cr.pack_bwd([_r(w)])).to(DEV)
    assert wb.numel() == lib.drsa_amd_conv_weight_bf16_elems(cout, cin, 1)
    gd = (cr.unpool(gin, am, pw, clones) if pw else gin).double()
    acc = F.conv_transpose2d(_r(gd), _r(w.double()), padding=1)
    bound = KTOL * F.conv_transpose2d(_r(gd).abs(), _r(w.double()).abs(), padding=1) + 1e-30
    xq, dq = x.double().repeat_interleave(clones, 0), den.double().repeat_interleave(clones, 0)
    sden = dq + torch.where(dq >= 0, cr.EPS, -cr.EPS)
    Bq = 2 * clones
    gdv, amd = gin.to(DEV).contiguous(), None if am is None else am.to(DEV).contiguous()
    xd, dd = x.to(DEV).contiguous(), den.to(DEV).contiguous()
    for xm, post in ((cr.XM_NONE, cr.POST_NONE), (cr.XM_MUL, cr.POST_DIV)):
        out = Guard((Bq, cin, H, W))
        xp, dp = (xd.data_ptr() if xm else None), (dd.data_ptr() if post else None)
        if via_pw:
            _capi.call("drsa_amd_conv_bwd_bf16_pw", gdv.data_ptr(), amd.data_ptr(), pw, wb.data_ptr(), xp, dp, out.ptr(),
                       Bq, clones, cout, cin, H, W, xm, post, cr.EPS, _capi.stream_ptr(DEV))
        else:
            _capi.call("drsa_amd_conv_bwd_bf16", gdv.data_ptr(), _capi.ptr(amd), wb.data_ptr(), xp, dp, out.ptr(),
                       Bq, clones, cout, cin, H, W, 1, xm, post, cr.EPS, _capi.stream_ptr(DEV))
        torch.cuda.synchronize()
        o = out.result().double()
        if xm == cr.XM_NONE:
            assert torch.all((o - acc).abs() <= bound), float((o - acc).abs().max())
        else:
            ref = torch.where(xq > 0, xq * acc / sden, torch.zeros_like(acc))
            b2 = xq * bound / sden.abs() + 1e-6 * ref.abs() + 1e-30
            assert torch.all((o - ref).abs() <= b2)
