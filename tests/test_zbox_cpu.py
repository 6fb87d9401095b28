"""ZBox (zennit 0.5.1's first-layer rule for a bounded input) and EpsilonGammaBox, without a GPU: the
descriptors' signatures, the composite's rule assignment, what the plan's parse step accepts and refuses,
the slow path (engine/hooks.py rule_relevance) against the float64 three-term form of tests/zbox_ref.py
and a closed-form answer, conservation with a bias, den >= 0 inside the box, that the reference's inputs
tell zero padding of the bounds from padding with their own value, and the argument errors of the three
entry points (returned before any device work)."""
import inspect

import pytest
import torch
import torch.nn as nn

import zbox_ref
from lrp_common import gtzan128, toy
from drsa_audio_amd.engine.hooks import rule_relevance
from drsa_audio_amd.engine.parse import EngineError, parse
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY
from drsa_audio_amd.zennit.composites import EpsilonGammaBox, NameMapComposite, SpecialFirstLayerMapComposite
from drsa_audio_amd.zennit.rules import Epsilon, Gamma, Pass, ZBox


def _defaults(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def test_signatures():
    E = inspect.Parameter.empty
    assert _defaults(ZBox.__init__) == [("low", E), ("high", E), ("stabilizer", 1e-6), ("zero_params", None)]
    assert _defaults(EpsilonGammaBox.__init__) == [
        ("low", E), ("high", E), ("epsilon", 1e-6), ("gamma", 0.25), ("stabilizer", 1e-6), ("layer_map", None),
        ("first_map", None), ("zero_params", None), ("canonizers", None)]
    r = ZBox(-4.0, 2.0)
    assert r.kind == "zbox" and r.stabilizer == 1e-6 and r.zero_params == ()
    assert issubclass(EpsilonGammaBox, SpecialFirstLayerMapComposite)


def test_bounds_use_the_first_row_and_spread_over_the_input():
    x = torch.zeros(3, 1, 4, 5, dtype=torch.float64)
    low = torch.arange(8.0).reshape(2, 1, 4, 1)
    lo, hi = ZBox(low, 9.0).bounds(x)
    assert lo.shape == x.shape and hi.shape == x.shape and lo.dtype == torch.float64
    assert torch.equal(lo[2, 0, :, 3], torch.arange(4.0, dtype=torch.float64)) and bool((hi == 9).all())


@pytest.mark.parametrize("make", [toy, gtzan128])
def test_epsilon_gamma_box_rules(make):
    net = make()
    rules = EpsilonGammaBox(-4.0, 2.0, epsilon=1e-7, gamma=0.4, stabilizer=1e-7).rules(net)
    convs = [n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    assert convs[0] == "features.0"
    z = rules["features.0"]
    assert isinstance(z, ZBox) and (z.low, z.high, z.stabilizer) == (-4.0, 2.0, 1e-7)
    for n in convs[1:]:
        assert isinstance(rules[n], Gamma) and (rules[n].gamma, rules[n].stabilizer) == (0.4, 1e-7)
    for n, m in net.named_modules():
        if isinstance(m, nn.Linear):
            assert isinstance(rules[n], Epsilon) and rules[n].epsilon == 1e-7
        if isinstance(m, nn.ReLU):
            assert isinstance(rules[n], Pass)
    assert sum(isinstance(r, ZBox) for r in rules.values()) == 1


def _zbox_map(nm, layer="features.0"):
    return [([layer], ZBox(-4.0, 2.0, stabilizer=1e-7))] + [e for e in nm if e[0] != [layer]]


def test_parse_accepts_the_first_conv_and_names_what_it_refuses():
    net = gtzan128()
    stages, dense = parse(net, NameMapComposite(_zbox_map(LRP_NAME_MAP_GTZAN)))
    assert (stages[0].rule_kind, stages[0].den_kind, stages[0].ng_fwd, stages[0].ng_bwd) == ("zbox", "box", 1, 1)
    stages, _ = parse(net, EpsilonGammaBox(-4.0, 2.0))
    assert [st.den_kind for st in stages] == ["box"] + ["gamma"] * 4
    for layer in ("features.3", "classifier.0"):
        with pytest.raises(EngineError, match=layer.replace(".", r"\.")):
            parse(net, NameMapComposite(_zbox_map(LRP_NAME_MAP_GTZAN, layer)))


def test_existing_composites_parse_as_before():
    for net, nm, first in ((gtzan128(), LRP_NAME_MAP_GTZAN, "wsquare"), (toy(), LRP_NAME_MAP_TOY, "flat")):
        stages, dense = parse(net, NameMapComposite(nm))
        assert [(st.rule_kind, st.den_kind, st.ng_fwd, st.ng_bwd) for st in stages] == \
            [(first, "map", 1, 1)] + [("gamma", "gamma", 2, 1)] * 4
        assert [ds.rule_kind for ds in dense] == ["epsilon"] * 3
        assert all(st.zb_wpn is None for st in stages)


# ------------------------------------------------------------------ the slow path
def _conv_case(H, W, bounds, seed, bias=True):
    """A 1 -> 5 channel conv, x inside the box with pixels exactly at low and at high, signed R."""
    g = torch.Generator().manual_seed(seed)
    m = nn.Conv2d(1, 5, 3, padding=1, bias=bias)
    with torch.no_grad():
        m.weight.copy_(torch.randn(5, 1, 3, 3, generator=g) / 3)
        if bias:
            m.bias.copy_(torch.randn(5, generator=g) * 0.3)
    if bounds == "scalar":
        low, high = -4.0, 2.0
    else:       # one bound per row, [1, 1, H, 1]
        low = -4.0 + torch.rand(1, 1, H, 1, generator=g)
        high = 1.0 + torch.rand(1, 1, H, 1, generator=g)
    lo, hi = zbox_ref.images(low, high, H, W)
    u = torch.rand(3, 1, H, W, generator=g)
    x = lo + u * (hi - lo)
    where = torch.randint(0, 4, x.shape, generator=g)
    x = torch.where(where == 0, lo.expand_as(x), torch.where(where == 1, hi.expand_as(x), x)).contiguous()
    R = torch.randn(3, 5, H, W, generator=g)
    return m, low, high, lo, hi, x, R


@pytest.mark.parametrize("H,W", [(5, 7), (2, 4)])
@pytest.mark.parametrize("bounds", ["scalar", "rows"])
def test_slow_path_is_the_three_term_form(H, W, bounds):
    m, low, high, lo, hi, x, R = _conv_case(H, W, bounds, seed=H + W + len(bounds))
    assert bool((x == lo).any()) and bool((x == hi).any())
    rule = ZBox(low, high, stabilizer=1e-6)
    ref = zbox_ref.three_term_f64(m.weight.detach(), m.bias.detach(), x, lo, hi, R, 1e-6)
    m64 = nn.Conv2d(1, 5, 3, padding=1).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    r64 = rule_relevance(rule, m64, x.double(), R.double())
    assert r64.dtype == torch.float64
    scale = float(ref.abs().max())
    assert float((r64 - ref).abs().max()) <= 1e-12 * scale
    # fp32: the same arithmetic in oneDNN's order; three 9-term sums and a division per output, 45 terms per
    # input pixel: 1e-5 of the largest relevance leaves two orders of margin over fp32's 6e-8
    r32 = rule_relevance(rule, m, x, R)
    assert r32.dtype == torch.float32
    assert float((r32.double() - ref).abs().max()) <= 1e-5 * scale
    # a batched bound contributes its first row (zennit low[:1])
    if bounds == "rows":
        two = ZBox(torch.cat([low, low + 1]), torch.cat([high, high - 1]), stabilizer=1e-6)
        assert torch.equal(rule_relevance(two, m64, x.double(), R.double()), r64)


def test_slow_path_on_a_linear_layer():
    g = torch.Generator().manual_seed(3)
    m = nn.Linear(6, 4).double()
    x = torch.rand(2, 6, generator=g).double() * 2 - 1
    R = torch.randn(2, 4, generator=g).double()
    r = rule_relevance(ZBox(-1.0, 1.0), m, x, R)
    w, b = m.weight.detach(), m.bias.detach()
    lo, hi = -torch.ones_like(x), torch.ones_like(x)
    den = (x @ w.t() + b) - (lo @ w.clamp(min=0).t() + b.clamp(min=0)) - (hi @ w.clamp(max=0).t() + b.clamp(max=0))
    gq = R / (den + 1e-6 * ((den >= 0).double() * 2 - 1))
    want = x * (gq @ w) - lo * (gq @ w.clamp(min=0)) - hi * (gq @ w.clamp(max=0))
    assert torch.allclose(r, want, rtol=1e-12, atol=1e-14)


def test_known_answer():
    """A 1 x 1 image, x = 1, l = -1, h = 3, centre weight 2, b = 0.5: z = 2.5, zl = -2 + 0.5, zh = 0, den = 4
    and R_in = (x - l) w g = 2 * 2 * R / 4 = R (up to the stabilizer)."""
    m = nn.Conv2d(1, 1, 3, padding=1).double()
    with torch.no_grad():
        m.weight.zero_()
        m.weight[0, 0, 1, 1] = 2.0
        m.bias.fill_(0.5)
    x, R = torch.ones(1, 1, 1, 1, dtype=torch.float64), torch.full((1, 1, 1, 1), 0.75, dtype=torch.float64)
    lo, hi = zbox_ref.images(-1.0, 3.0, 1, 1)
    _, den, _ = zbox_ref.three_term_f64(m.weight.detach(), m.bias.detach(), x, lo, hi, R, 0.0, parts=True)
    assert float(den) == 4.0
    assert float(rule_relevance(ZBox(-1.0, 3.0, stabilizer=0.0), m, x, R)) == 0.75
    r = float(rule_relevance(ZBox(-1.0, 3.0, stabilizer=1e-6), m, x, R))
    assert abs(r - 0.75 * 4 / (4 + 1e-6)) <= 1e-15


@pytest.mark.parametrize("bounds", ["scalar", "rows"])
def test_conservation_with_a_bias_and_nonnegative_den(bounds):
    m, low, high, lo, hi, x, R = _conv_case(5, 7, bounds, seed=11)
    assert float(m.bias.abs().min()) > 0
    stab = 1e-6
    r, den, gq = zbox_ref.three_term_f64(m.weight.detach(), m.bias.detach(), x, lo, hi, R, stab, parts=True)
    assert float(den.min()) >= 0.0                      # x inside the box
    # sum R_in = sum g den = sum R den / stab(den): off sum R by at most stabilizer * sum |g|
    assert abs(float(r.sum() - R.double().sum())) <= stab * float(gq.abs().sum())
    m64 = nn.Conv2d(1, 5, 3, padding=1).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    rs = rule_relevance(ZBox(low, high, stabilizer=stab), m64, x.double(), R.double())
    assert abs(float(rs.sum() - R.double().sum())) <= stab * float(gq.abs().sum())
    # the bias cancels in the denominator: zero_params = "bias" changes roundings only
    rz = rule_relevance(ZBox(low, high, stabilizer=stab, zero_params="bias"), m64, x.double(), R.double())
    assert float((rz - rs).abs().max()) <= 1e-12 * float(rs.abs().max())


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("bounds", ["scalar", "rows"])
def test_wrong_padding_differs_on_the_border_ring_only(bounds):
    m, low, high, lo, hi, x, R = _conv_case(5, 7, bounds, seed=5)
    wp, wn, bp, bn = zbox_ref.split(m.weight.detach(), m.bias.detach())
    right, wrong = zbox_ref.maps_ref(wp, bp, wn, bn, lo, hi), zbox_ref.maps_ref(wp, bp, wn, bn, lo, hi, pad="low")
    ring = torch.ones(5, 7, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    for a, b in zip(right, wrong):
        assert torch.equal(a[:, ~ring], b[:, ~ring])
        assert bool((a != b)[:, ring].any(0).all())     # every ring pixel, in some channel
    # ... and in the rule's result, through the same inputs the kernel tests use
    r0 = zbox_ref.three_term_f64(m.weight.detach(), m.bias.detach(), x, lo, hi, R, 1e-6)
    r1 = zbox_ref.three_term_f64(m.weight.detach(), m.bias.detach(), x, lo, hi, R, 1e-6, pad="low")
    assert float((r0 - r1).abs().max()) > 1e-3 * float(r0.abs().max())


def test_reference_entry_points_against_the_three_term_form():
    """maps_ref / den_ref / bwd_ref (the kernels' two-chain form) compose to the three-term form."""
    m, low, high, lo, hi, x, R = _conv_case(5, 7, "rows", seed=9)
    w, b = m.weight.detach(), m.bias.detach()
    wp, wn, bp, bn = zbox_ref.split(w, b)
    zl, zh = zbox_ref.maps_ref(wp, bp, wn, bn, lo, hi)
    z = torch.nn.functional.conv2d(x, w, b, padding=1)
    den = zbox_ref.den_ref(z, None, zl, zh)
    gq = R / (den + 1e-6 * ((den >= 0).float() * 2 - 1))
    out = zbox_ref.bwd_ref(gq, None, wp, wn, x, lo, hi, 1)
    ref = zbox_ref.three_term_f64(w, b, x, lo, hi, R, 1e-6)
    assert float((out.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ------------------------------------------------------------------ argument errors (no launch)
def _err(lib):
    return lib.drsa_amd_last_error().decode()


def test_entry_point_argument_errors():
    from drsa_audio_amd import _capi
    lib = _capi.load()
    P, Q = 0x10000, 0x10004             # never dereferenced: every call below is refused before any device work
    bwd = lib.drsa_amd_first_layer_zbox_bwd
    cases = [
        ((P, None, P, P, P, P, P, 0, 1, 4, 8, 8, None), "bad batch"),
        ((P, None, P, P, P, P, P, 6, 4, 4, 8, 8, None), "bad batch"),
        ((P, None, P, P, P, P, P, 2, 0, 4, 8, 8, None), "bad batch"),
        ((P, None, P, P, P, P, P, 2, 1, 0, 8, 8, None), "bad shape"),
        ((P, None, P, P, P, P, P, 2, 1, 2048, 1024, 1024, None), "below 2^31"),
        ((None, None, P, P, P, P, P, 2, 1, 4, 8, 8, None), "null pointer"),
        ((P, None, None, P, P, P, P, 2, 1, 4, 8, 8, None), "null pointer"),
        ((P, None, P, None, P, P, P, 2, 1, 4, 8, 8, None), "null pointer"),
        ((P, None, P, P, None, P, P, 2, 1, 4, 8, 8, None), "null pointer"),
        ((P, None, P, P, P, None, P, 2, 1, 4, 8, 8, None), "null pointer"),
        ((P, None, P, P, P, P, None, 2, 1, 4, 8, 8, None), "null pointer"),
        ((P, P, P, P, P, P, P, 2, 1, 4, 7, 8, None), "even H and W % 4 == 0"),
        ((P, P, P, P, P, P, P, 2, 1, 4, 8, 6, None), "even H and W % 4 == 0"),
        ((P, P, P, P, P, P, Q, 2, 1, 4, 8, 8, None), "out must be 16-byte aligned"),
        ((P, P, P, Q, P, P, P, 2, 1, 4, 8, 8, None), "must be 16-byte aligned"),
    ]
    for args, msg in cases:
        assert bwd(*args) == _capi.DRSA_EINVAL, args
        assert "first_layer_zbox_bwd" in _err(lib) and msg in _err(lib), (args, _err(lib))
    maps = lib.drsa_amd_first_layer_zbox_maps
    assert maps(P, None, P, None, P, P, P, P, 0, 4, 4, None) == _capi.DRSA_EINVAL and "bad shape" in _err(lib)
    assert maps(None, None, P, None, P, P, P, P, 2, 4, 4, None) == _capi.DRSA_EINVAL and "null pointer" in _err(lib)
    assert maps(P, None, P, None, P, P, P, None, 2, 4, 4, None) == _capi.DRSA_EINVAL and "null pointer" in _err(lib)
    den = lib.drsa_amd_first_layer_zbox_den
    assert den(P, None, P, P, P, 0, 4, 4, 4, None) == _capi.DRSA_EINVAL and "bad shape" in _err(lib)
    assert den(P, None, None, P, P, 2, 4, 4, 4, None) == _capi.DRSA_EINVAL and "null pointer" in _err(lib)
    assert den(P, P, P, P, P, 2, 4, 5, 4, None) == _capi.DRSA_EINVAL and "even H and W" in _err(lib)
    assert den(P, P, Q, P, P, 2, 4, 4, 4, None) == _capi.DRSA_EINVAL and "8-byte aligned" in _err(lib)
    assert den(P, None, P, P, P, 2, 2048, 1024, 1024, None) == _capi.DRSA_EINVAL and "below 2^31" in _err(lib)


def test_plan_cache_key_takes_tensor_bounds_by_content():
    from drsa_audio_amd.engine import cache_key
    net = toy()
    low = torch.full((1, 1, 64, 1), -4.0)
    key = lambda lo, hi: cache_key(net, NameMapComposite([(["features.0"], ZBox(lo, hi))]))     # noqa: E731
    assert key(low, 2.0) == key(low.clone(), 2.0)
    assert key(low, 2.0) != key(low - 1, 2.0)
    assert key(low, 2.0) != key(low, 3.0)
    assert key(low, 2.0) != key(low.reshape(1, 1, 1, 64), 2.0)
