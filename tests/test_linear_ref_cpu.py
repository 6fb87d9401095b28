"""tests/linear_ref.py itself (no GPU): the reference of tests/test_linear_gpu.py against the oracle's
rule backward in exact mode and against float64, the properties its inputs need to show a mistake, the
coverage of its case lists, and that five plausible kernel mistakes change its result in the last
partial tile on exactly those inputs (so that bit equality on the GPU means something)."""
import pytest
import torch
import torch.nn as nn

import linear_ref as lr
import lrp_ref

EPS = lr.EPS


# ------------------------------------------------------------------ oracle equality
def _layer(n, k, bias, seed):
    torch.manual_seed(seed)
    lin = nn.Linear(k, n, bias=bias)
    with torch.no_grad():
        lin.weight[0, :3] = 0.0
    W, b = lin.weight.detach(), None if lin.bias is None else lin.bias.detach()
    return lrp_ref.Layer("classifier.0", lin, "linear"), W, b


def _xr(M, N, K, signed, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x = x if signed else x.abs()
    x[torch.rand(M, K, generator=g) < 0.2] = 0.0
    return x, torch.randn(M, N, generator=g)


_SHAPE = (17, 20, 33)      # M, N, K: partial tiles, a K tail


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("signed", [1, 0], ids=["signed", "unsigned"])
def test_epsilon_is_the_oracle(signed, bias):
    M, N, K = _SHAPE
    L, W, b = _layer(N, K, bias, 1)
    x, R = _xr(M, N, K, signed, 2)
    z, _ = lr.linear_fwd_ref(x, W, b)
    got = lr.linear_bwd_ref(R, None, 0, z, 0, 1, EPS, W, x, lr.XM_MUL, None, lr.POST_NONE, 0.0)
    assert torch.equal(got, lrp_ref.rule_backward_analytic(L, ("epsilon", EPS), x, z, R, ops=lrp_ref.ExactOps))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("negden", [1, 0], ids=["negden", "masked"])
@pytest.mark.parametrize("signed", [1, 0], ids=["signed", "unsigned"])
def test_gamma_is_the_oracle(signed, negden, bias):
    """With den_n the [z < 0] branch runs; without it the relevance arrives through the ReLU mask, where that
    branch is exactly zero."""
    M, N, K = _SHAPE
    L, W, b = _layer(N, K, bias, 3)
    x, R = _xr(M, N, K, signed, 4)
    rp = lr._rules(W, b, ("gamma",))["gamma"]
    z, _, dp, dn = lr.rule_fwd_ref(x, W, rp["Wp"], rp["Wn"], b, rp["bp"], rp["bn"] if negden else None, signed, negden)
    assert (z < 0).any() and (z > 0).any()
    got = lr.rule_bwd_ref(R, None, 0, z, 0 if negden else 1, dp, dn, 0, 1, rp["eps"], rp["Wp"], rp["Wn"], x, 1, signed,
                          None, lr.POST_NONE, 0.0)
    Rin = R if negden else torch.where(z > 0, R, torch.zeros_like(R))
    want = lrp_ref.rule_backward_analytic(L, ("gamma", lr.GAMMA, EPS), x, z, Rin, ops=lrp_ref.ExactOps)
    assert torch.equal(got, want)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("signed", [1, 0], ids=["signed", "unsigned"])
def test_zplus_is_the_oracle(signed, bias):
    M, N, K = _SHAPE
    L, W, b = _layer(N, K, bias, 5)
    x, R = _xr(M, N, K, signed, 6)
    rp = lr._rules(W, b, ("zplus",))["zplus"]
    z, _, dp, dn = lr.rule_fwd_ref(x, W, rp["Wp"], rp["Wn"] if signed else None, b, rp["bp"], None, signed, 0)
    assert dn is None
    got = lr.rule_bwd_ref(R, None, 0, z, 0, dp, None, 0, 0, rp["eps"], rp["Wp"], rp["Wn"] if signed else None, x, 1, signed,
                          None, lr.POST_NONE, 0.0)
    assert torch.equal(got, lrp_ref.rule_backward_analytic(L, ("zplus", EPS), x, z, R, ops=lrp_ref.ExactOps))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rule", ["wsquare", "flat"])
def test_wsquare_flat_are_the_oracle(rule, bias):
    M, N, K = _SHAPE
    L, W, b = _layer(N, K, bias, 7)
    x, R = _xr(M, N, K, 1, 8)
    rp = lr._rules(W, b, (rule,))[rule]
    z, _ = lr.linear_fwd_ref(x, W, b)
    got = lr.rule_bwd_ref(R, None, 0, z, 0, rp["den"], None, 1, 0, rp["eps"], rp["W2"], None, None, 0, 0, None,
                          lr.POST_NONE, 0.0)
    assert torch.equal(got, lrp_ref.rule_backward_analytic(L, (rule, EPS), x, z, R, ops=lrp_ref.ExactOps))


# ------------------------------------------------------------------ every case of the lists
def _all_cases():
    for name, ep, inst, shapes, modes, build in lr.entries():
        for i, shape in enumerate(shapes):
            for mode in modes:
                yield name, ep, inst, shape, mode, i, build


def test_every_chain_is_within_the_float64_bound(monkeypatch):
    """|chain - f64| <= (K + 2) 2^-24 (sum_k |x_k w_k| + |b|) for every chain of every case: K fma roundings
    and the bias add give a relative error (1 + u)^(K + 1) - 1 <= (K + 2) u on the sum of magnitudes, u = 2^-24
    (derived, not measured); NaN rows are NaN in both."""
    chain, matmul, seen = lr.chain, lr.matmul, [0]

    def check(out, xd, wd, bd):
        f = xd @ wd + (0 if bd is None else bd)
        mag = xd.abs() @ wd.abs() + (0 if bd is None else bd.abs())
        nan = torch.isnan(f)
        assert torch.equal(torch.isnan(out), nan)
        assert bool((((out.double() - f).abs() <= (xd.size(1) + 2) * 2.0 ** -24 * mag) | nan).all())
        seen[0] += 1
        return out

    monkeypatch.setattr(lr, "chain", lambda x, W, b: check(chain(x, W, b), x.double(), W.double().t(),
                                                           None if b is None else b.double()))
    monkeypatch.setattr(lr, "matmul", lambda g, W: check(matmul(g, W), g.double(), W.double(), None))
    for name, ep, inst, shape, mode, i, build in _all_cases():
        build(shape, mode, i)
    assert seen[0] > 3000


def _has_signs(t, both=True):
    return bool((t > 0).any()) and (not both or bool((t < 0).any()))


def _zero_kinds(t):
    z = t == 0
    return bool((z & ~torch.signbit(t)).any()), bool((z & torch.signbit(t)).any())


def test_forward_inputs_can_show_each_mistake():
    for M, N, K in lr.fwd_shapes():
        for signed in (0, 1):
            d = lr.fwd_inputs(M, N, K, signed)
            x, xn = d["x"], d["xnan"]
            assert bool((x == 0).any()) and not torch.isnan(x).any()
            assert _has_signs(x, both=bool(signed)) and (signed or bool((x >= 0).all()))
            # one NaN, in the last row; it reaches that row of every output and no other
            assert torch.isnan(xn).sum() == 1 and torch.isnan(xn[-1]).sum() == 1
            rows = torch.zeros(M, N, dtype=torch.bool)
            rows[-1] = True
            for inst in (i for i in lr.RULE_FWD_INSTS if i[1] == signed):
                _, want = lr.rule_fwd_case((M, N, K), inst, (1, 1, 1))
                for k, v in want.items():
                    assert v is None or torch.equal(torch.isnan(v), rows), (k, inst)
            assert bool((d["W"] == 0).any()) and _has_signs(d["W"])
            assert _has_signs(d["b"], both=N > 1)
            for rule in ("gamma", "zplus"):
                assert d["rp0"][rule]["bp"] is None and d["rp"][rule]["bp"] is not None


def test_backward_inputs_can_show_each_mistake():
    for M, Nout, Kin in lr.bwd_shapes():
        for signed in (0, 1):
            d = lr.bwd_inputs(M, Nout, Kin, signed)
            z, x, R, cls = d["z"], d["x"], d["R"], d["cls"].long()
            small = M == 1 and Nout < 4          # one or three elements cannot hold four classes
            if not small:
                assert _has_signs(z) and all(_zero_kinds(z)), (M, Nout)
            assert M * Nout < 2 or _has_signs(R)
            # the ReLU mask hits and misses in the last row and in the last column of z
            if Nout > 1:
                assert bool((z[-1] > 0).any()) and bool((~(z[-1] > 0)).any())
            if M > 1:
                assert bool((z[:, -1] > 0).any()) and bool((~(z[:, -1] > 0)).any())
            # the post mask hits and misses in the last row and in the last column of x, on an exact zero
            assert bool((x == 0).any()) and _has_signs(x, both=bool(signed)) and (signed or bool((x >= 0).all()))
            assert x[-1, -1] > 0 and bool((x[-1] == 0).any())
            assert M == 1 or (bool((x[:, -1] > 0).any()) and bool((x[:, -1] == 0).any()))
            # the seed: first and last class, not the same in every row
            assert bool((cls >= 0).all()) and bool((cls < Nout).all()) and cls[0] == Nout - 1
            if M > 1 and Nout > 1:
                assert cls[-1] == 0 and len(set(cls.tolist())) > 1
            # denominators: both signs, +0 and -0, magnitudes below eps; zeros and negatives in the last row
            dens = [("den", d["den"], lr.EPS_POST)] + ([] if small else [("den_p", d["den_p"], EPS), ("den_n", d["den_n"], EPS)])
            for name, t, eps in dens:
                assert bool((t == 0).any()) and bool((t < 0).any()), name
                if t.numel() >= 8:       # fewer elements cannot hold all five kinds
                    assert _has_signs(t) and all(_zero_kinds(t)), name
                    assert bool(((t != 0) & (t.abs() < eps)).any()), name
                if t.size(1) >= 3:
                    assert bool((t[-1] == 0).any()) and bool((t[-1] < 0).any()), name
            if Nout >= 5:
                # a zero of den_p under z > 0 and a zero of den_n under z < 0, in the last row, with R != 0
                assert bool(((d["den_p"][-1] == 0) & (z[-1] > 0) & (R[-1] != 0)).any())
                assert bool(((d["den_n"][-1] == 0) & (z[-1] < 0) & (R[-1] != 0)).any())
                assert bool(((d["den_p"][-1] < 0) & (z[-1] > 0)).any())
            # WSquare / Flat: the plan's constant with and without the bias
            for rule in ("wsquare", "flat"):
                assert d["rp"][rule]["den"].shape == (Nout,) and d["rp0"][rule]["b2"] is None


def test_case_lists_cover_every_kernel_at_every_size():
    """Per entry point and instantiation: every M and every N at each kernel the dispatch can choose, every K
    of the issue's sets, the largest case, and every value of every mode at every M and every K."""
    for name, ep, inst, shapes, modes, build in lr.entries():
        fwd = ep in ("linear_fwd", "linear_rule_fwd")
        ks = lr.FWD_KS if fwd else lr.BWD_KS
        kdim = (lambda s: s[2]) if fwd else (lambda s: s[1])
        ndim = (lambda s: s[1]) if fwd else (lambda s: s[2])
        assert {kdim(s) for s in shapes} == set(ks), name
        kernels = {lr.kernel_of(ep, kdim(s)) for s in shapes}
        assert kernels == ({"short", "long"} if fwd else {"bwd"}), name
        for kern in kernels:
            mine = [s for s in shapes if lr.kernel_of(ep, kdim(s)) == kern]
            assert {s[0] for s in mine} == set(lr.MS) and {ndim(s) for s in mine} == set(lr.NS), (name, kern)
        for K in ks:
            assert {s[0] for s in shapes if kdim(s) == K} == set(lr.MS), (name, K)
            assert {ndim(s) for s in shapes if kdim(s) == K} == set(lr.NS), (name, K)
        for M in lr.MS:
            assert {ndim(s) for s in shapes if s[0] == M} == set(lr.NS), (name, M)
        assert max(s[0] * s[1] * s[2] for s in shapes) == 50 * 48 * max(ks) and (50, 48, 384) in lr.fwd_shapes()
        # every shape runs every mode, so every mode value runs at every M and every K; the values themselves:
        for col in zip(*modes):
            assert len(set(col)) > 1, (name, col)
    assert {m[0] for m in lr.LIN_BWD_MODES} == {"R", "cls", "onehot"}
    assert {m[1:4] for m in lr.LIN_BWD_MODES} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (lr.XM_NONE, lr.XM_MUL)}
    assert {(m[0], m[4]) for m in lr.LIN_BWD_MODES} >= {(s, p) for s in ("R", "cls", "onehot") for p in (0, 1, 2)}
    assert {(m[0], m[2]) for m in lr.RULE_BWD_MODES} == {(s, p) for s in ("R", "cls", "onehot") for p in (0, 1, 2)}
    assert {(i[1], i[2]) for i in lr.RULE_FWD_INSTS if i[0] == "gamma"} == {(1, 1), (1, 0), (0, 1), (0, 0)}
    assert {(i[1], i[2]) for i in lr.RULE_BWD_INSTS if i[0] == "gamma"} == {(1, 1), (1, 0), (0, 1), (0, 0)}
    assert {i[0] for i in lr.RULE_BWD_INSTS} == {"gamma", "zplus", "wsquare", "flat"}


# ------------------------------------------------------------------ mutation sensitivity
def _chain_chunked(chain, size):
    """The K chain summed per ``size``-wide chunk, the partial sums then added (the bias last)."""
    def f(x, W, b):
        out = None
        for k in range(0, x.size(1), size):
            p = chain(x[:, k:k + size], W[:, k:k + size], None)
            out = p if out is None else out + p
        return out if b is None else out + b
    return f


def _matmul_chunked(matmul, size):
    def f(g, W):
        out = None
        for k in range(0, g.size(1), size):
            p = matmul(g[:, k:k + size], W[k:k + size])
            out = p if out is None else out + p
        return out
    return f


def _bias_first(chain):
    """The chain started from the bias: fma(1, b, +0) = b exactly, then k ascending."""
    def f(x, W, b):
        if b is None:
            return chain(x, W, None)
        return chain(torch.cat([torch.ones(x.size(0), 1), x], 1), torch.cat([b[:, None], W], 1), None)
    return f


def _stab_gt(t, e):
    e = torch.tensor(e, dtype=torch.float32)
    return t + torch.where(t > 0, e, -e)


# mutant -> ({primitive: wrong variant}, the cases it can show in: (entry point, instantiation, shape, mode) -> bool)
_POSTS = (lr.POST_DIV, lr.POST_MASK)
_MUTANTS = {
    "k-chunks-of-128": (lambda: {"chain": _chain_chunked(lr.chain, 128)},
                        lambda ep, inst, s, m: ep in ("linear_fwd", "linear_rule_fwd") and s[2] > 128),
    "k-chunks-of-32": (lambda: {"matmul": _matmul_chunked(lr.matmul, 32)},
                       lambda ep, inst, s, m: ep in ("linear_bwd", "linear_rule_bwd") and s[1] > 32),
    "bias-first": (lambda: {"chain": _bias_first(lr.chain)},
                   lambda ep, inst, s, m: ep in ("linear_fwd", "linear_rule_fwd") and m[0] == 1),
    "clamps-swapped": (lambda: {"pos": lr.neg, "neg": lr.pos},
                       lambda ep, inst, s, m: ep in ("linear_rule_fwd", "linear_rule_bwd") and inst[1] == 1),
    "stab-gt": (lambda: {"stab": _stab_gt},
                lambda ep, inst, s, m: (ep == "linear_bwd" and m[0] == "R" and m[1] == 0 and m[2] == 1)
                or (ep == "linear_rule_bwd" and inst[0] in ("gamma", "zplus") and m[0] == "R" and m[1] == 0)),
    "post-mask-ge": (lambda: {"keep": lambda x: x >= 0},
                     lambda ep, inst, s, m: (ep == "linear_bwd" and m[3] == lr.XM_NONE and m[4] in _POSTS)
                     or (ep == "linear_rule_bwd" and inst[0] in ("wsquare", "flat") and m[2] in _POSTS)),
}


def _last_tile(t):
    """The last partial 16 x 16 tile of an output (the 32 x 32 workgroup tile's last wave tile is the same cells)."""
    return t[(t.size(0) - 1) // 16 * 16:, (t.size(1) - 1) // 16 * 16:]


def _differs(a, b):
    a, b = _last_tile(a), _last_tile(b)
    return not (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


@pytest.mark.parametrize("mutant", sorted(_MUTANTS))
def test_a_wrong_variant_shows_in_the_last_partial_tile(mutant, monkeypatch):
    """For every entry point and instantiation the variant applies to, and for every M: at least one case where
    the wrong variant's result differs from the reference's inside the last partial tile."""
    make, applies = _MUTANTS[mutant]
    cases = [c for c in _all_cases() if applies(c[1], c[2], c[3], c[4])]
    good = [c[6](c[3], c[4], c[5])[1] for c in cases]
    for k, v in make().items():
        monkeypatch.setattr(lr, k, v)
    shown, groups = set(), set()
    for (name, ep, inst, shape, mode, i, build), ref in zip(cases, good):
        groups |= {name, shape[0]}
        bad = build(shape, mode, i)[1]
        if any(v is not None and _differs(bad[k], v) for k, v in ref.items()):
            shown |= {name, shape[0]}
    assert groups >= set(lr.MS) and shown == groups, groups - shown
