"""Average-pooled conv blocks through the engine's host side, without a GPU: the comparator against torch, the
parse step's acceptances and refusals, the schedule's forms, VGGType(pool="avg"), and the argument checks of
drsa_amd_avgpool_fwd / _bwd (rejected before any device work)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import avgpool_ref as A
import lrp_ref
from lrp_common import toy
from drsa_audio_amd import _capi
from drsa_audio_amd._capi import POST_DIV, POST_NONE
from drsa_audio_amd.engine.plan import EngineError, LRPEngine
from drsa_audio_amd.engine.parse import parse
from drsa_audio_amd.engine.schedule import capture_set, capture_stage, schedule
from drsa_audio_amd.model.create_model import VGGType
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.xai.explain.explainer import get_class_composite
from drsa_audio_amd.zennit.composites import EpsilonGammaBox, NameMapComposite
from drsa_audio_amd.zennit.rules import AlphaBeta, Epsilon, Flat, Gamma, Norm, Pass, ZBox

_TOY = NameMapComposite(LRP_NAME_MAP_TOY)
_POOLS = ["features.2", "features.5", "features.8", "features.11", "features.14"]
_RELUS = ["features.1", "features.4", "features.7", "features.10", "features.13"]


def _all_kernels(*_):      # a stub has_kernel: every tuned 3x3 kernel exists
    return True


def _sched(net, comp, B=2, **kw):
    stages, dense = parse(net, comp)
    return stages, *schedule(stages, dense, B, 64, 64, has_kernel=_all_kernels, **kw)


# --------------------------------------------------------------------------- the comparator
WINDOWS = [(2, 2), (2, 4), (4, 4), (4, 8), (8, 16), (3, 3), (1, 2), (2, 3)]


@pytest.mark.parametrize("ph,pw", WINDOWS)
def test_comparator_forward_is_torch_avg_pool2d(ph, pw):
    """The contract's order (one fp32 chain from 0, rows outer, columns inner, one division) IS torch's CPU
    avg_pool2d for contiguous NCHW, bit for bit; multiplying by 1 / K is not, at (3, 3)."""
    g = torch.Generator().manual_seed(ph * 100 + pw)
    x = torch.randn(3, 5, 4 * ph, 2 * pw, generator=g).clamp(min=0) * 3
    y = A.pool_fwd(x, ph, pw)
    assert torch.equal(y, F.avg_pool2d(x, (ph, pw)))
    if (ph, pw) == (3, 3):
        sums = F.avg_pool2d(x, (3, 3), divisor_override=1)
        assert torch.equal(sums / 9.0, y) and not torch.equal(sums * torch.tensor(1.0 / 9.0), y)


@pytest.mark.parametrize("ph,pw", [(2, 2), (2, 3), (4, 8)])
@pytest.mark.parametrize("rule", [None, "norm", "epsilon"])
def test_comparator_backward_is_float64_autograd(ph, pw, rule):
    """The three pool backwards against float64 autograd: the pool's input gradient for the unmapped pool,
    x * grad(R / stab(z)) for Norm / Epsilon.  Both sides are float64; they differ by the roundings of at most
    three operations per element (2^-53 each), hence 1e-14 relative."""
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 3, 2 * ph, 3 * pw, generator=g, dtype=torch.float64).clamp(min=0) * 2).requires_grad_(True)
    x.data[0, 0, :ph, :pw] = 0.0                 # a dead window: stab's [z == 0] branch
    z = F.avg_pool2d(x, (ph, pw))
    R = torch.randn(z.shape, generator=g, dtype=torch.float64)
    eps = {None: None, "norm": 1e-6, "epsilon": 0.25}[rule]
    if rule is None:
        want, = torch.autograd.grad(z, x, R)
        got = A.pool_plain_backward(R, ph, pw)
    else:
        grad, = torch.autograd.grad(z, x, R / lrp_ref.stabilize(z.detach(), eps))
        want = x.detach() * grad
        got = A.pool_rule_backward(x.detach(), A.pool_fwd(x.detach(), ph, pw), R, eps, ph, pw)
    assert float(want.abs().max()) > 0
    torch.testing.assert_close(got, want, rtol=1e-14, atol=0.0)


def test_comparator_walk_against_autograd():
    """The patched oracle walk on an all-avg toy net with no rules anywhere is the plain gradient: float64
    autograd of the logit, and the patch is gone afterwards."""
    net = A.toy_avg().double()
    x = torch.randn(2, 1, 64, 64, dtype=torch.float64, requires_grad=True)
    out = net(x)
    want, = torch.autograd.grad(out[:, 1].sum(), x)
    _, R = A.lrp(net, {}, x.detach(), class_idx=1, one_hot_encoded=True, mode="f64")
    torch.testing.assert_close(R, want, rtol=1e-9, atol=1e-12 * float(want.abs().max()))
    with pytest.raises(TypeError, match="unsupported module AvgPool2d"):
        lrp_ref.lrp(net, {}, x.detach(), class_idx=1, mode="f64")


# --------------------------------------------------------------------------- the model factory
def test_vggtype_pool_avg_same_parameters():
    kw = dict(n_filters=(8, 8, 16), n_dense=32, n_classes=3, pool_kernels=((2, 2), (2, 4), (4, 4)), dropout=0.1,
              input_size=(32, 64), conv_bn=True, dense_bn=True, block_depth=2)
    torch.manual_seed(3)
    mx = VGGType(**kw)
    torch.manual_seed(3)
    av = VGGType(**kw, pool="avg")
    sa, sm = av.state_dict(), mx.state_dict()
    assert list(sa) == list(sm) and all(torch.equal(sa[k], sm[k]) for k in sm)
    pools = [m for m in av.features if isinstance(m, (nn.AvgPool2d, nn.MaxPool2d))]
    assert [type(m) for m in pools] == [nn.AvgPool2d] * 3 and [A.pool_k(m) for m in pools] == [(2, 2), (2, 4), (4, 4)]
    assert not any(isinstance(m, nn.AvgPool2d) for m in mx.features)
    assert av.eval()(torch.randn(2, 1, 32, 64)).shape == (2, 3)
    with pytest.raises(ValueError, match="pool must be"):
        VGGType(**kw, pool="mean")


# --------------------------------------------------------------------------- parse / check / schedule
@pytest.mark.parametrize("kinds", [("avg",) * 5, ("max", "avg", "max", "avg", "max"), ("avg", "max", "avg", "max", "avg")])
def test_parse_and_check_accept(kinds):
    net = A.toy_avg(kinds)
    LRPEngine.check(net, _TOY)
    stages, _ = parse(net, _TOY)
    assert [st.pool_kind for st in stages] == list(kinds) and all(st.pool for st in stages)
    assert [st.pool_name for st in stages] == _POOLS
    assert all(st.pool_rule is None and st.pool_eps == 0.0 for st in stages)
    assert [st.avg for st in stages] == [k == "avg" for k in kinds]


def test_parse_records_the_pool_rule():
    net = A.toy_avg(("avg", "avg", "max", "avg", "avg"), last_k=(4, 4))
    nm = LRP_NAME_MAP_TOY + [(["features.2"], Norm(stabilizer=1e-5)), (["features.14"], Epsilon(epsilon=0.5))]
    stages, _ = parse(net, NameMapComposite(nm))
    assert [(st.pool_kind, st.pool_rule, st.pool_eps) for st in stages] == [
        ("avg", "epsilon", 1e-5), ("avg", None, 0.0), ("max", None, 0.0), ("avg", None, 0.0), ("avg", "epsilon", 0.5)]
    assert stages[-1].pool_k == (4, 4)


def test_epsilon_gamma_box_preset_maps_norm_to_the_pools():
    """The preset's (AvgPool, Norm) entry reaches the plan; its ZBox on the first conv of an averaged block is
    refused by name, and taken once that block pools by maximum."""
    comp = EpsilonGammaBox(low=-4.0, high=0.0)
    with pytest.raises(EngineError, match=r"ZBox on features\.0.*AvgPool2d features\.2"):
        LRPEngine.check(A.toy_avg(), comp)
    stages, _ = parse(A.toy_avg(("max", "avg", "avg", "avg", "avg")), comp)
    assert [(st.pool_rule, st.pool_eps) for st in stages[1:]] == [("epsilon", 1e-6)] * 4


def test_max_pool_schedule_is_unchanged_and_new_fields_default():
    stages, conv, _ = _sched(toy(), _TOY)
    assert all((st.pool_kind, st.pool_rule, st.pool_eps, st.avg) == ("max", None, 0.0, False) for st in stages)
    assert [sp.form for sp in conv] == ["fused"] * 5 and [sp.g_in for sp in conv] == ["sparse"] * 5
    assert not any(sp.rel_full for sp in conv) and conv[0].den == "ring"


def test_schedule_all_avg():
    stages, conv, head = _sched(A.toy_avg(last_k=(4, 4)), _TOY)
    assert [sp.form for sp in conv] == ["avg"] * 5 and [sp.pool for sp in conv] == [0] * 5
    assert [sp.g_in for sp in conv] == ["unavg"] * 5
    assert [sp.den for sp in conv] == ["map", "copy", "copy", "copy", "copy"]
    # the launch above an averaged stage leaves its post step out; the first dense stage counts as above
    assert [sp.post for sp in conv] == [POST_NONE] * 5 and head[0].post == POST_NONE
    assert [sp.out_hw for sp in conv] == [(32, 32), (16, 16), (8, 8), (4, 4), (1, 1)]
    assert conv[0].bwd == "drsa_amd_first_layer_bwd" and {sp.bwd for sp in conv[1:]} == {"drsa_amd_conv_bwd"}


def test_schedule_alternating():
    """max, avg, max, avg, max: only the launch above an averaged stage loses its post step."""
    stages, conv, head = _sched(A.toy_avg(("max", "avg", "max", "avg", "max")), _TOY)
    assert [sp.form for sp in conv] == ["fused", "avg", "fused", "avg", "fused"]
    assert [sp.g_in for sp in conv] == ["sparse", "unavg", "sparse", "unavg", "sparse"]
    assert [sp.post for sp in conv[1:]] == [conv[1].post, POST_NONE, POST_DIV, POST_NONE]
    assert conv[1].post != POST_NONE and head[0].post == POST_DIV


def test_schedule_5x5_and_no_rule():
    net = A.toy_avg(conv_kernel=(5, 5))
    stages, conv, _ = _sched(net, NameMapComposite([(["features.0"], Flat()), (["features.6"], Gamma(0.25))]))
    assert {sp.fwd for sp in conv} == {"drsa_amd_convk_fwd"} and {sp.bwd for sp in conv} == {"drsa_amd_convk_bwd"}
    assert [sp.den for sp in conv] == ["copy", "none", "copy", "none", "none"]
    assert [sp.form for sp in conv] == ["avg"] * 5 and [sp.post for sp in conv] == [POST_NONE] * 5


def test_schedule_refuses_a_window_that_does_not_divide_the_map():
    net = A.toy_avg()
    net.features[14] = nn.AvgPool2d(3)
    stages, dense = parse(net, _TOY)
    with pytest.raises(ValueError, match="sides divisible by the pool"):
        schedule(stages, dense, 2, 64, 64, has_kernel=_all_kernels)


def test_capture_stage_and_rel_full():
    net = A.toy_avg(("max", "avg", "avg", "max", "avg"))
    stages, dense = parse(net, _TOY)
    assert capture_stage(stages, "features.5") == (1, "pool") and capture_stage(stages, "features.4") == (1, "relu")
    where, keep, stop, taps = capture_set(stages, ["features.4", "features.8", "features.7"])
    assert (where, keep, stop, taps) == ([(1, "relu"), (2, "pool"), (2, "relu")], (1, 2), 1, (2,))
    conv, _ = schedule(stages, dense, 2, 64, 64, capture=keep, stop_after=stop, taps=taps, has_kernel=_all_kernels)
    assert [sp.rel_full for sp in conv] == [False, True, True, False, False]
    assert conv[2].tap_post == POST_NONE and conv[1].bwd is None and conv[3].post == POST_NONE
    # a pool capture alone asks for no dense relevance
    conv, _ = schedule(stages, dense, 2, 64, 64, stop_after=1, has_kernel=_all_kernels)
    assert not any(sp.rel_full for sp in conv)


def test_projection_at_a_max_pooled_stage_of_an_averaged_net():
    """ProjectionModel at features.7 (a max-pooled stage) below and above averaged ones: accepted, and the
    clones run through the averaged stages below the projection."""
    net = A.toy_avg(("avg", "avg", "max", "avg", "avg"))
    pm = ProjectionModel(net, 7, torch.eye(16), 4, case="toy").eval()
    comp = get_class_composite(LRP_NAME_MAP_TOY, 4)
    LRPEngine.check(pm, comp)
    stages, dense = parse(pm, comp)
    conv, _ = schedule(stages, dense, 2, 64, 64, fanout=1, has_kernel=_all_kernels)
    assert [sp.g_in for sp in conv] == ["unavg", "unavg", "proj", "unavg", "unavg"]
    assert [sp.clones for sp in conv] == [5, 5, 5, 1, 1]


# --------------------------------------------------------------------------- refusals, by message
def _with(net, idx, mod):
    net.features[idx] = mod
    return net


def _proj_before_avg():
    return ProjectionModel(A.toy_avg(), 7, torch.eye(16), 4, case="toy").eval()


@pytest.mark.parametrize("make,comp,needle", [
    (lambda: _with(A.toy_avg(), 5, nn.AvgPool2d(2, stride=1)), _TOY, r"AvgPool2d features\.5 must have stride = kernel"),
    (lambda: _with(A.toy_avg(), 5, nn.AvgPool2d(2, padding=1)), _TOY, r"AvgPool2d features\.5 must have stride = kernel"),
    (lambda: _with(A.toy_avg(), 5, nn.AvgPool2d(2, ceil_mode=True)), _TOY, r"AvgPool2d features\.5 must have.*ceil_mode"),
    (lambda: _with(A.toy_avg(), 5, nn.AvgPool2d(2, divisor_override=3)), _TOY,
     r"AvgPool2d features\.5 must have.*divisor_override"),
    (lambda: _with(A.toy_avg(), 14, nn.AdaptiveAvgPool2d(1)), _TOY, r"AdaptiveAvgPool2d features\.14 is not supported"),
    (lambda: A.toy_avg(), NameMapComposite(LRP_NAME_MAP_TOY + [(["features.8"], Pass())]),
     r"rule Pass on AvgPool2d features\.8 is not supported"),
    (lambda: A.toy_avg(), NameMapComposite(LRP_NAME_MAP_TOY + [(["features.8"], Gamma(0.25))]),
     r"rule Gamma on AvgPool2d features\.8 is not supported"),
    (lambda: A.toy_avg(), NameMapComposite(LRP_NAME_MAP_TOY + [(["features.7"], Pass())]),
     r"unmapped AvgPool2d features\.8 below a Pass on its block's activation \(features\.7\)"),
    (_proj_before_avg, get_class_composite(LRP_NAME_MAP_TOY, 4),
     r"AvgPool2d features\.\w+ after a ProjectionModel layer is not supported"),
    (lambda: A.toy_avg(), NameMapComposite([(["features.3"], AlphaBeta(2.0, 1.0))]),
     r"AlphaBeta on features\.3.*AvgPool2d features\.5"),
    (lambda: A.toy_avg(), NameMapComposite([(["features.0"], ZBox(-4.0, 0.0))]),
     r"ZBox on features\.0.*AvgPool2d features\.2"),
], ids=["stride", "padding", "ceil", "divisor", "adaptive", "pass-on-pool", "gamma-on-pool", "unmapped-below-pass",
        "projection", "alphabeta", "zbox"])
def test_refusals(make, comp, needle):
    with pytest.raises(EngineError, match=needle):
        LRPEngine.check(make(), comp)


def test_pass_on_the_relu_is_taken_with_a_rule_on_the_pool():
    nm = LRP_NAME_MAP_TOY + [(_RELUS, Pass()), (_POOLS, Norm(stabilizer=1e-6))]
    LRPEngine.check(A.toy_avg(), NameMapComposite(nm))


# --------------------------------------------------------------------------- the C ABI
_PTR = {k: 0x10000 * (i + 1) for i, k in enumerate(("R_y", "y", "a", "den", "g", "rel_full"))}
_ORDER = {
    "avgpool_fwd": "a y B C H W ph pw stream",
    "avgpool_bwd": "R_y y a den den_bcast rule eps_pool eps_conv g rel_full Bq clones C H W ph pw stream",
}
_VALID = dict(_PTR, B=2, Bq=4, clones=2, C=5, H=8, W=16, ph=2, pw=4, den_bcast=0, rule=1, eps_pool=1e-6, eps_conv=1e-6,
              stream=None)
_SHAPE = "the map's sides must be multiples of the pool's"
_REJECTIONS = (
    ("avgpool_fwd", dict(a=None), "null pointer"), ("avgpool_fwd", dict(y=None), "null pointer"),
    ("avgpool_fwd", dict(ph=0), "bad pool kernel 0x4"), ("avgpool_fwd", dict(pw=-1), "bad pool kernel 2x-1"),
    ("avgpool_fwd", dict(ph=3), _SHAPE), ("avgpool_fwd", dict(pw=3), _SHAPE), ("avgpool_fwd", dict(C=0), "bad shape"),
    ("avgpool_fwd", dict(B=-1), "bad shape"), ("avgpool_fwd", dict(H=0), "bad shape"),
    ("avgpool_bwd", dict(R_y=None), "null pointer"), ("avgpool_bwd", dict(a=None), "null pointer"),
    ("avgpool_bwd", dict(g=None), "null pointer"), ("avgpool_bwd", dict(y=None), "needs the pool's output y"),
    ("avgpool_bwd", dict(rule=2), "rule must be 0"), ("avgpool_bwd", dict(rule=-1), "rule must be 0"),
    ("avgpool_bwd", dict(den_bcast=2), "den_bcast must be 0 or 1"), ("avgpool_bwd", dict(clones=0), "bad clones"),
    ("avgpool_bwd", dict(Bq=3), "bad clones"), ("avgpool_bwd", dict(Bq=-2), "bad clones"),
    ("avgpool_bwd", dict(ph=0), "bad pool kernel 0x4"), ("avgpool_bwd", dict(ph=3), _SHAPE),
    ("avgpool_bwd", dict(pw=3), _SHAPE), ("avgpool_bwd", dict(C=0), "bad shape"),
    ("avgpool_bwd", dict(W=18, pw=2), "multiple of 4"), ("avgpool_bwd", dict(g=_PTR["g"] + 4), "16-byte aligned"),
    ("avgpool_bwd", dict(den=_PTR["den"] + 8), "16-byte aligned"),
    ("avgpool_bwd", dict(rel_full=_PTR["rel_full"] + 4), "16-byte aligned"),
)


@pytest.mark.parametrize("entry,changes,needle", _REJECTIONS,
                         ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c, _ in _REJECTIONS])
def test_entry_points_reject_bad_arguments(entry, changes, needle):
    """Fake device addresses: every call fails its argument check, before anything is dereferenced."""
    args = dict(_VALID, **changes)
    rc = getattr(_capi.lib(), "drsa_amd_" + entry)(*[args[k] for k in _ORDER[entry].split()])
    msg = _capi.lib().drsa_amd_last_error().decode()
    assert rc == _capi.DRSA_EINVAL, (rc, msg)
    assert needle in msg and msg.startswith(entry + ":"), msg


def test_empty_batches_are_no_ops():
    """B = 0 launches nothing (the fake addresses are never read)."""
    lib = _capi.lib()
    assert lib.drsa_amd_avgpool_fwd(*[dict(_VALID, B=0)[k] for k in _ORDER["avgpool_fwd"].split()]) == _capi.DRSA_OK
    assert lib.drsa_amd_avgpool_bwd(*[dict(_VALID, Bq=0)[k] for k in _ORDER["avgpool_bwd"].split()]) == _capi.DRSA_OK
