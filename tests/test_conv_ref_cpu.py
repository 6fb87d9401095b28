"""tests/conv_ref.py (the CPU reference behind tests/test_conv_edges_gpu.py) checked without a GPU.

* Served: every case of the GPU file has a kernel by the matching ``*_has_kernel*`` query (the
  queries do no device work).  The dense fp32 backward has no query in the ABI; its cases are the
  pool-sparse ones' shapes, and a missing kernel there fails the GPU case with DRSA_EUNSUPPORTED.
* Against float64: the forward helper vs F.conv2d / F.max_pool2d(return_indices) and the backward
  helper vs autograd of maxpool(relu(conv)), both in float64.  The bound is the standard bound of an
  n-term fp32 chain (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1),
  gamma_n * conv(|x|, |W|) with gamma_n = n u / (1 - n u), u = 2^-24 and n = 9 * cin + 2 (the products, the additions and
  the bias add); biases enter the magnitude sum with |b|.  The argmax must be equal wherever the
  window's top two values are further apart than twice that bound.  Derived, not measured.
* Inputs bite: on the inputs of the GPU file, four deliberately wrong references (replicate
  padding, last maximum wins a tie, x >= 0 in the post mask, +eps for a negative denominator) each
  differ from the right one in the last row, the last column and the corner of every case they
  apply to.  x >= 0 applies where xmode is XM_NONE under a post step (the den_map and den_ring
  cases): where the rule multiplies by x, an output at x = 0 is 0 on either side of the mistake.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr
from drsa_audio_amd import _capi

U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------ served
def test_every_gpu_case_is_served():
    L = _capi.lib()
    bad = []
    for c in cr.fwd_cases():
        cin, cout, H, W, ng, pool, den = c
        if L.drsa_amd_conv_fwd_has_kernel(cin, cout, W, ng, pool, 0) != 1:
            bad.append(("fwd", c))
    for c in cr.bwd_cases():
        cin, cout, H, W, sparse, (ng, xmode, post, clones) = c
        if L.drsa_amd_conv_bwd_has_kernel_pw(cout, cin, W, ng, 2) != 1:
            bad.append(("bwd", c))
    for c in cr.den_map_cases():
        cin, cout, H, W, pool_w, xmode = c
        if L.drsa_amd_conv_bwd_has_kernel_pw(cout, cin, W, 1, pool_w or 2) != 1:
            bad.append(("den_map", c))
    for c in cr.den_ring_cases():
        cin, cout, H, W, sparse, xmode = c
        if L.drsa_amd_conv_bwd_has_kernel_pw(cout, cin, W, 1, 2) != 1:
            bad.append(("den_ring", c))
    for c in cr.bf16_fwd_cases():
        cin, cout, H, W, ng, pool = c
        if L.drsa_amd_conv_fwd_has_kernel(cin, cout, W, ng, pool, 1) != 1:
            bad.append(("fwd_bf16", c))
    for c in cr.bf16_bwd_cases():
        cin, cout, H, W, pw = c
        ok = (L.drsa_amd_conv_bwd_has_kernel_bf16_pw(cout, cin, W, abs(pw)) if pw else
              L.drsa_amd_conv_bwd_has_kernel_bf16(cout, cin, W, 1, 0))
        if ok != 1:
            bad.append(("bwd_bf16", c))
    assert not bad, bad


def test_case_list_reaches_every_path():
    """The paths the cases are chosen for, restated on the case list itself."""
    fwd, bwd = cr.fwd_cases(), cr.bwd_cases()
    for direction, cases in (("fwd", fwd), ("bwd", bwd)):
        for pair in cr.PAIRS:
            cin, cout = pair if direction == "fwd" else pair[::-1]
            fam = {cr.tile_width(direction == "fwd", cin, cout, c[3]) for c in cases if (c[0], c[1]) == pair}
            want = {cr.tile_width(direction == "fwd", cin, cout, W) for W in (12, 40)}
            assert fam == want, (direction, pair, fam, want)
    assert {c[4] for c in fwd} == {1, 2, 3} and {c[5] for c in fwd} == {0, 1, 2}
    assert any(c[3] % 4 and c[0] > 1 for c in fwd) and any(c[3] % 4 and c[0] == 1 for c in fwd)   # scalar staging
    assert any(c[0] == 1 and c[5] == 0 for c in fwd) and any(c[0] == 1 and c[5] == 1 and c[3] % 8 for c in fwd)
    assert {(c[4], c[5]) for c in bwd} == {(s, m) for s in (0, 1) for m in cr.BWD_MODES}
    assert {(c[3] // 2) % 4 for c in bwd if c[4]} == {0, 2}       # aligned and per-cell sparse staging
    assert any(c[4] == 4 for c in cr.den_map_cases())


# ------------------------------------------------------------------ against float64
@pytest.mark.parametrize("cin,cout,H,W", [(1, 32, 6, 12), (20, 32, 12, 34), (64, 100, 6, 10), (64, 64, 12, 48)])
@pytest.mark.parametrize("ng", [1, 2, 3])
def test_forward_helper_vs_float64(cin, cout, H, W, ng):
    x, sets, bias3, den_map = cr.fwd_inputs(cin, cout, H, W, ng)
    xd, b = x.double(), bias3.double()
    col = lambda v: v.view(1, -1, 1, 1)
    ins = [xd, xd, xd] if ng < 3 else [xd, xd.clamp(min=0), xd.clamp(max=0)]
    z = [F.conv2d(ins[s], sets[s].double(), padding=1) for s in range(ng)]
    mag = [F.conv2d(ins[s].abs(), sets[s].double().abs(), padding=1) for s in range(ng)]
    g = gamma(9 * cin + 2)
    y64 = (z[0] + col(b[0])).clamp(min=0)
    y64 = torch.where(torch.isnan(z[0]), z[0], y64)
    by = g * (mag[0] + col(b[0].abs()))
    if ng == 1:
        d64, bd = z[0] + col(b[1]), g * (mag[0] + col(b[1].abs()))
    elif ng == 2:
        d64, bd = (z[1] + col(b[1])) + col(b[2]), g * (mag[1] + col(b[1].abs() + b[2].abs()))
    else:
        d64, bd = (z[1] + col(b[1])) + (z[2] + col(b[2])), g * (mag[1] + mag[2] + col(b[1].abs() + b[2].abs()))
    memo = {}
    for pool_mode in (0, 1) + ((2,) if W % 8 == 0 else ()):
        out, am, den = cr.conv_fwd_ref(x, sets, bias3, pool_mode, "computed", memo=memo)
        nan = torch.isnan(y64)
        if not pool_mode:
            assert torch.equal(torch.isnan(out), nan) and torch.equal(torch.isnan(den), nan)
            assert torch.all(((out.double() - y64).abs() <= by)[~nan])
            assert torch.all(((den.double() - d64).abs() <= bd)[~nan])
            continue
        pw = 4 if pool_mode == 2 else 2
        m64, idx = F.max_pool2d(y64, (2, pw), return_indices=True)
        am64 = ((idx // W) % 2) * pw + (idx % W) % pw
        bwin = cr.windows(by, pw)
        bmax = torch.nan_to_num(bwin, nan=0.0).max(-1).values
        nanw = torch.isnan(m64)
        assert torch.equal(torch.isnan(out), nanw)
        assert torch.all(((out.double() - m64).abs() <= bmax)[~nanw])
        top2 = cr.windows(y64, pw).topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 2 * bmax          # False in windows that hold a NaN
        assert clear.any()
        assert torch.equal(am.long()[clear], am64[clear])
        dsel = torch.gather(cr.windows(d64, pw), -1, am.long().unsqueeze(-1)).squeeze(-1)
        bsel = torch.gather(cr.windows(bd, pw), -1, am.long().unsqueeze(-1)).squeeze(-1)
        ok = ~torch.isnan(dsel)
        assert torch.equal(torch.isnan(den), ~ok)
        assert torch.all(((den.double() - dsel).abs() <= bsel)[ok])
        # the map denominator is a gather of the map at the argmax
        _, _, dm = cr.conv_fwd_ref(x, sets, bias3, pool_mode, "map", den_map, memo=memo)
        assert torch.equal(dm, cr.at_argmax(den_map.expand(2, -1, -1, -1).contiguous(), am, pw))


@pytest.mark.parametrize("cin,cout,H,W,pw", [(1, 32, 6, 12, 2), (20, 32, 10, 20, 2), (64, 100, 6, 12, 2),
                                             (64, 64, 12, 48, 4), (32, 48, 6, 36, 0)])
@pytest.mark.parametrize("mode", cr.BWD_MODES)
def test_backward_helper_vs_float64_autograd(cin, cout, H, W, pw, mode):
    """The transposed conv (with the pool and ReLU backward for a pool-sparse g) is float64
    autograd's input gradient of maxpool(relu(conv(x0))) (dense g: of conv(x0)); the rule and post
    steps on top of it are restated in float64."""
    ng, xmode, post, clones = mode
    gin, _, sets, x, den = cr.bwd_inputs(cin, cout, H, W, ng, pw, clones)
    gen = torch.Generator().manual_seed(cin + H + W)
    x0 = torch.randn(2, cin, H, W, generator=gen, dtype=torch.float64).repeat_interleave(clones, 0)
    wd = [w.double() for w in sets]

    def grad(fn, upstream):
        xi = x0.clone().requires_grad_(True)
        fn(xi).backward(upstream)
        return xi.grad

    am = None
    if pw:
        # the forward's argmax and its dead windows (ReLU backward), from float64; clone q of a
        # sample shares them (row q reads sample q // clones)
        m64, idx = F.max_pool2d(F.conv2d(x0, wd[0], padding=1).clamp(min=0), (2, pw), return_indices=True)
        am = (((idx // W) % 2) * pw + (idx % W) % pw).to(torch.uint8)[::clones].contiguous()
        gin = gin * (m64 > 0)
        gfull = cr.unpool(gin, am, pw, clones).double()
        t64 = [grad(lambda xi: F.max_pool2d(F.conv2d(xi, wd[0], padding=1).clamp(min=0), (2, pw)), gin.double())]
    else:
        gfull = gin.double()
        t64 = [grad(lambda xi: F.conv2d(xi, wd[0], padding=1), gfull)]
    if ng == 2:
        t64.append(grad(lambda xi: F.conv2d(xi, wd[1], padding=1), gfull))
    mag = [F.conv_transpose2d(gfull.abs(), w.abs(), padding=1) for w in wd]
    out = cr.conv_bwd_ref(gin, am, pw, sets, x, den, clones, xmode, post, cr.EPS)
    g = gamma(9 * cout + 2)
    xq, dq = x.double().repeat_interleave(clones, 0), den.double().repeat_interleave(clones, 0)
    if xmode == cr.XM_NONE:
        R, bR = t64[0], g * mag[0]
    elif xmode == cr.XM_MUL:
        R, bR = xq * t64[0], xq.abs() * g * mag[0]
    else:
        R = xq.clamp(min=0) * t64[0] + xq.clamp(max=0) * t64[1]
        bR = xq.clamp(min=0) * g * mag[0] + xq.clamp(max=0).abs() * g * mag[1]
    if post != cr.POST_NONE:
        if post == cr.POST_DIV:
            e = float(torch.tensor(cr.EPS, dtype=torch.float32))
            sd = dq + torch.where(dq >= 0, e, -e)
            R, bR = R / sd, bR / sd.abs()
        R = torch.where(xq > 0, R, torch.zeros_like(R))
        bR = torch.where(xq > 0, bR, torch.zeros_like(bR))
    # the elementwise steps (product, stab, quotient) round once each: gamma_4 of the result
    bound = bR * (1 + gamma(4)) + gamma(4) * R.abs()
    assert torch.all((out.double() - R).abs() <= bound), float(((out.double() - R).abs() - bound).max())
    assert out.abs().max() > 0


# ------------------------------------------------------------------ inputs bite
def _edges_differ(a, b):
    """Per output pair: differ in the last row, the last column and the corner?"""
    def ne(u, v):
        return bool(((u != v) & ~(torch.isnan(u) & torch.isnan(v))).any()) if u.is_floating_point() else bool((u != v).any())
    row = any(ne(u[..., -1, :], v[..., -1, :]) for u, v in zip(a, b))
    colm = any(ne(u[..., :, -1], v[..., :, -1]) for u, v in zip(a, b))
    corner = any(ne(u[..., -1, -1], v[..., -1, -1]) for u, v in zip(a, b))
    return row, colm, corner


def _fwd_groups():
    groups = {}
    for cin, cout, H, W, ng, pool, den in cr.fwd_cases():
        groups.setdefault((cin, cout, H, W, ng), []).append((pool, den.split("_")[0]))
    return groups


@pytest.mark.parametrize("key", sorted(_fwd_groups()), ids=lambda k: "-".join(map(str, k)))
def test_forward_inputs_bite(key):
    cin, cout, H, W, ng = key
    x, sets, bias3, den_map = cr.fwd_inputs(cin, cout, H, W, ng)
    right, padded = {}, {}
    for pool, den in sorted(set(_fwd_groups()[key])):
        ref = [t for t in cr.conv_fwd_ref(x, sets, bias3, pool, den, den_map, memo=right) if t is not None]
        wrong = [t for t in cr.conv_fwd_ref(x, sets, bias3, pool, den, den_map, pad="replicate", memo=padded)
                 if t is not None]
        assert _edges_differ(ref, wrong) == (True, True, True), ("replicate padding", pool, den)
        if pool:
            wrong = [t for t in cr.conv_fwd_ref(x, sets, bias3, pool, den, den_map, tie="last", memo=right)
                     if t is not None]
            assert _edges_differ(ref, wrong) == (True, True, True), ("last maximum", pool, den)


def _bwd_all():
    out = [("bwd", c[:4], 2 if c[4] else 0, c[5], False) for c in cr.bwd_cases()]
    out += [("map", c[:4], c[4], (1, c[5], cr.POST_DIV, 2), True) for c in cr.den_map_cases()]
    out += [("ring", c[:4], 2 if c[4] else 0, (1, c[5], cr.POST_DIV, 2), False) for c in cr.den_ring_cases()]
    return out


@pytest.mark.parametrize("case", _bwd_all(), ids=lambda c: "-".join(map(str, (c[0],) + c[1] + (c[2],) + c[3])))
def test_backward_inputs_bite(case):
    kind, (cin, cout, H, W), pw, (ng, xmode, post, clones), shared = case
    if kind == "ring":
        gin, am, sets, x, den = cr.ring_inputs(cin, cout, H, W, pw, clones)[:5]
    else:
        gin, am, sets, x, den = cr.bwd_inputs(cin, cout, H, W, ng, pw, clones, shared)
    memo = {}
    run = lambda **kw: [cr.conv_bwd_ref(gin, am, pw, sets, x, den, clones, xmode, post, cr.EPS, den_shared=shared, **kw)]
    ref = run(memo=memo)
    assert _edges_differ(ref, run(pad="replicate")) == (True, True, True), "replicate padding"
    if post == cr.POST_DIV:
        assert _edges_differ(ref, run(stab_plus=True, memo=memo)) == (True, True, True), "stab +eps"
    if post != cr.POST_NONE and xmode == cr.XM_NONE:
        assert _edges_differ(ref, run(mask_ge=True, memo=memo)) == (True, True, True), "x >= 0"
    elif post != cr.POST_NONE:
        assert torch.equal(ref[0], run(mask_ge=True, memo=memo)[0])      # invisible where the rule multiplies by x
