"""K x K convs through the engine's host side, without a GPU: the parse step's acceptances and refusals,
the schedule's forms for a stage that is not 3x3, the model factory's classifier width, and the argument
checks of the four drsa_amd_convk_* entry points (rejected before any device work)."""
import pytest
import torch
import torch.nn as nn

import convk_ref as K
from drsa_audio_amd import _capi
from drsa_audio_amd._capi import POST_DIV, POST_MASK, POST_NONE
from drsa_audio_amd.engine.plan import EngineError, LRPEngine
from drsa_audio_amd.engine.parse import parse
from drsa_audio_amd.engine.schedule import schedule
from drsa_audio_amd.model.create_model import VGGType, get_out_shape
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.rules import AlphaBeta, Epsilon, Gamma, WSquare, ZBox

_FK, _BK = "drsa_amd_convk_fwd", "drsa_amd_convk_bwd"
_TOY = NameMapComposite(LRP_NAME_MAP_TOY)


def _all_kernels(*_):      # a stub has_kernel: every tuned 3x3 kernel exists
    return True


def _sched(net, comp, **kw):
    stages, dense = parse(net, comp)
    return stages, schedule(stages, dense, 2, 64, 64, has_kernel=_all_kernels, **kw)[0]


@pytest.mark.parametrize("name", ["all5x5", "first7x7"])
def test_check_accepts(name):
    LRPEngine.check(K.toy_k(K.TOY_NETS[name]), _TOY)


def test_schedule_all_5x5():
    stages, steps = _sched(K.toy_k(K.TOY_NETS["all5x5"]), _TOY)
    assert [st.k for st in stages] == [(5, 5)] * 5
    for li, sp in enumerate(steps):
        assert (sp.fwd, sp.pool, sp.form, sp.den) == (_FK, 0, "unfused", "copy")
        assert (sp.bwd, sp.g_in, sp.wts_bf16) == (_BK, "unpool", False)
        assert sp.post == (POST_NONE if li == 0 else POST_DIV)


def test_schedule_mixed():
    """7x7 on features.0 under 3x3 convs: the tuned stage above divides by the generic stage's per-sample copy."""
    stages, steps = _sched(K.toy_k(K.TOY_NETS["first7x7"]), _TOY)
    assert (steps[0].fwd, steps[0].form, steps[0].den, steps[0].bwd, steps[0].g_in) == (_FK, "unfused", "copy", _BK, "unpool")
    assert (steps[1].fwd, steps[1].form, steps[1].bwd, steps[1].post, steps[1].g_in) == (
        "drsa_amd_conv_fwd", "fused", "drsa_amd_conv_bwd", POST_DIV, "sparse")


def test_3x3_wsquare_under_a_5x5_conv_leaves_a_copy():
    net = K.toy_k([None, (5, 5), None, None, None])
    stages, steps = _sched(net, _TOY)
    assert (steps[0].fwd, steps[0].den) == ("drsa_amd_conv_fwd", "copy")
    assert (steps[1].bwd, steps[1].post) == (_BK, POST_DIV)
    # the all-3x3 toy net keeps its ring
    assert _sched(K.toy_k([None] * 5), _TOY)[1][0].den == "ring"


def test_schedule_rules_without_pool_and_alphabeta():
    """No rule: den "none" and POST_MASK above; AlphaBeta keeps its two plain backwards on the new entry; a
    conv without a pool after it is "full" with a dense g."""
    nm = [(["features.0"], WSquare()), (["features.3"], AlphaBeta(2.0, 1.0)), (["features.9"], Gamma(0.25)),
          (["features.12"], Epsilon())]
    net = K.toy_k(K.TOY_NETS["all5x5"])
    stages, steps = _sched(net, NameMapComposite(nm))
    assert stages[1].den_kind == "ab" and steps[1].bwd == _BK and steps[1].g_in == "unpool"
    assert steps[2].den == "none" and steps[3].post == POST_MASK
    assert {sp.post for sp in steps} <= {POST_NONE, POST_DIV, POST_MASK}
    feats = [m for n, m in net.features.named_children() if n != "14"]      # drop the last pool
    net.features = nn.Sequential(*feats)
    net.classifier[0] = nn.Linear(16 * 4 * 4, 32)
    stages, steps = _sched(net, NameMapComposite([(["features.12"], Epsilon())]))
    assert (steps[-1].form, steps[-1].g_in, steps[-1].fwd, steps[-1].den) == ("full", "dense", _FK, "copy")


def _conv0(net, conv):
    net.features[0] = conv
    return net


@pytest.mark.parametrize("make,comp,needle", [
    (lambda: K.toy_k([(5, 5), None, None, None, None]),
     NameMapComposite([(["features.0"], ZBox(-4.0, 0.0))]), "ZBox on features.0 needs a 3x3 conv"),
    (lambda: _conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, 4, padding="same")), _TOY, "odd kernel"),
    (lambda: _conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, 9, padding="same")), _TOY, "up to 7x7"),
    (lambda: _conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, 5, stride=2, padding=2)), _TOY, "stride-1"),
    (lambda: _conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, 5, padding="same", padding_mode="reflect")), _TOY, "zero-padded"),
    (lambda: _conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, 5, padding=1)), _TOY, "'same'"),
    (lambda: _conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, (3, 5), padding=(2, 1))), _TOY, "'same'"),
], ids=["zbox5x5", "even", "9x9", "stride2", "reflect", "valid", "pad-transposed"])
def test_refusals(make, comp, needle):
    with pytest.raises(EngineError, match=needle):
        LRPEngine.check(make(), comp)


def test_integer_same_padding_is_accepted():
    LRPEngine.check(_conv0(K.toy_k([None] * 5), nn.Conv2d(1, 8, (3, 5), padding=(1, 2))), _TOY)


def test_factory_5x5_classifier_width():
    torch.manual_seed(0)
    net = VGGType(n_filters=(8, 8, 16, 16, 16), conv_kernel=(5, 5), n_dense=32, n_classes=2, pool_kernels=((2, 2),) * 5,
                  dropout=0.0, input_size=(64, 64), conv_bn=False, dense_bn=False, block_depth=1).eval()
    assert net(torch.randn(2, 1, 64, 64)).shape == (2, 2)
    LRPEngine.check(net, _TOY)


def test_get_out_shape_unchanged_at_3x3():
    """The three model configurations of lrp_common.py (toy, gtzan128, vggish), with 'same' and with 1."""
    for kw, want in ((dict(input_size=(64, 64), pool_kernels=((2, 2),) * 5, out_filters=16, block_depth=1), 16 * 2 * 2),
                     (dict(input_size=(128, 128), pool_kernels=((2, 2),) * 5, out_filters=128, block_depth=1), 128 * 4 * 4),
                     (dict(input_size=(128, 256), pool_kernels=((2, 4), (2, 2), (2, 2), (2, 2), (2, 2)), out_filters=128,
                           block_depth=2), 128 * 4 * 4)):
        assert get_out_shape(conv_kernel=(3, 3), padding="same", **kw) == want
        assert get_out_shape(conv_kernel=(3, 3), padding=1, **kw) == want
        assert get_out_shape(conv_kernel=(5, 3), padding="same", **kw) == want


# --------------------------------------------------------------------------- the C ABI
_PTR = {k: 0x10000 * (i + 1) for i, k in enumerate(("in", "g", "wts", "bias", "x", "den", "den_map", "out", "out_den"))}
_ORDER = {
    "convk_fwd": "in wts bias den_map out out_den B cin cout H W kh kw ng stream",
    "convk_bwd": "g wts x den out Bq clones cin cout H W kh kw ng xmode post eps stream",
}
_VALID = dict(_PTR, B=2, Bq=2, clones=1, cin=64, cout=64, H=8, W=32, kh=5, kw=5, ng=1, xmode=1, post=1, eps=1e-6, stream=None)
_E = _capi.DRSA_EINVAL
_BOTH = [(dict(kh=4), "kh and kw must be odd"), (dict(kw=2), "kh and kw must be odd"), (dict(kh=9), "kh and kw must be odd"),
         (dict(kw=0), "kh and kw must be odd"), (dict(kh=-3), "kh and kw must be odd"), (dict(wts=None), "null pointer"),
         (dict(out=None), "null pointer"), (dict(H=7), "H must be even and W % 4 == 0 (got 7x32)"),
         (dict(W=30), "H must be even and W % 4 == 0 (got 8x30)"), (dict(H=0), "bad shape"), (dict(cin=0), "bad shape"),
         (dict(cin=128, cout=128, H=4096, W=4096), "2^31")]
_REJECTIONS = (
    *[("convk_fwd", ch, msg) for ch, msg in _BOTH], *[("convk_bwd", ch, msg) for ch, msg in _BOTH],
    ("convk_fwd", {"in": None}, "null pointer"), ("convk_fwd", dict(bias=None), "null pointer"),
    ("convk_fwd", dict(ng=0), "ng must be 1..3"), ("convk_fwd", dict(ng=4), "ng must be 1..3"), ("convk_fwd", dict(B=0), "bad shape"),
    ("convk_bwd", dict(g=None), "null pointer"), ("convk_bwd", dict(ng=0), "ng must be 1..2"), ("convk_bwd", dict(ng=3), "ng must be 1..2"),
    ("convk_bwd", dict(Bq=0), "bad batch/clones"), ("convk_bwd", dict(clones=0), "bad batch/clones"),
    ("convk_bwd", dict(Bq=3, clones=2), "bad batch/clones"), ("convk_bwd", dict(xmode=3), "bad xmode"),
    ("convk_bwd", dict(post=3), "post must be 0, 1 or 2"), ("convk_bwd", dict(x=None, post=0), "xmode needs x"),
    ("convk_bwd", dict(den=None), "POST_DIV needs x and den"), ("convk_bwd", dict(x=None, xmode=0), "POST_DIV needs x and den"),
)


@pytest.mark.parametrize("entry,changes,needle", _REJECTIONS,
                         ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c, _ in _REJECTIONS])
def test_entry_points_reject_bad_arguments(entry, changes, needle):
    args = dict(_VALID, **changes)
    rc = getattr(_capi.lib(), "drsa_amd_" + entry)(*[args[k] for k in _ORDER[entry].split()])
    msg = _capi.lib().drsa_amd_last_error().decode()
    assert rc == _E, (rc, msg)
    assert needle in msg and msg.startswith(entry + ":"), msg


def test_supported_and_weight_floats():
    lib = _capi.lib()
    for kh in (1, 3, 5, 7):
        for kw in (1, 3, 5, 7):
            assert lib.drsa_amd_convk_supported(kh, kw, 1, 8) == 1 and lib.drsa_amd_convk_supported(kh, kw, 40, 33) == 1
            for cin, cout, ng in ((1, 8, 1), (40, 33, 3), (33, 40, 2)):
                n = lib.drsa_amd_convk_weight_floats(kh, kw, cin, cout, ng)
                assert n > 0 and n == K._convk_fwd_layout([torch.zeros(cout, cin, kh, kw)] * ng).numel()
    for kh, kw in ((2, 3), (3, 4), (9, 3), (3, 9), (0, 1), (-1, 3)):
        assert lib.drsa_amd_convk_supported(kh, kw, 8, 8) == 0 and lib.drsa_amd_convk_weight_floats(kh, kw, 8, 8, 1) == 0
    assert lib.drsa_amd_convk_supported(3, 3, 0, 8) == 0 and lib.drsa_amd_convk_supported(3, 3, 8, 0) == 0
