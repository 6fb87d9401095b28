"""Which backward conv entry point the engine calls for each trunk layer (engine/plan.py backward()).

The engine chooses between drsa_amd_conv_bwd, _bf16, _bf16_pw, _den_map and _den_ring per layer, by
the plan's precision, the pool under the layer, the post step of the layer below and the
``*_has_kernel*`` queries.  The tests here only observe: they wrap ``_capi.call``, pair every
``drsa_amd_conv_bwd*`` call with its tag from the engine's trace, and compare the sequence of
(tag, entry point, pool_w, wts_bf16) with the lists below, written down from a run of the engine
before its four backward branches were folded into one method (the features.2 capture: from reading
those branches, then confirmed by the same run).  pool_w is the argument where the
entry point has one (None otherwise); wts_bf16 is the argument of the den-map / den-ring entries,
1 for the _bf16 entries and 0 for drsa_amd_conv_bwd.  A second run on the same engine must give the
same bits.

Inputs: batch 2; GTZAN at its classifier's 128 x 128 (the den-ring layer at 64 x 64 pooled); VGGish
at 32 x 128, the smallest map whose fifth block is still 2 x 4 (W % 4 == 0), with block 1 at W = 128
(W >= 32, W / 4 % 4 == 0: the (2,4) pool folds).
"""
import copy

import pytest
import torch

from lrp_common import gtzan128, logmel, vggish
from drsa_audio_amd import _capi
from drsa_audio_amd.engine.plan import LRPEngine
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_VGGISH
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

_B = "drsa_amd_conv_bwd"
_POOL_W = {_B + "_bf16_pw": 2, _B + "_den_map": 2}            # entry -> index of its pool_w argument
_WTS_BF16 = {_B + "_den_map": 4, _B + "_den_ring": 3}         # entry -> index of its wts_bf16 argument


def _plain(layers, bf16):
    return [(f"conv_bwd:features.{i}", _B + ("_bf16" if bf16 else ""), None, bf16) for i in layers]


# (model, plan, capture layer) -> [(tag, entry point, pool_w, wts_bf16), ...] top-down
_G, _V = (12, 9, 6), (31, 28, 24, 21, 17, 14, 10, 7)
EXPECTED = {
    # GTZAN: features.3 sits above the WSquare first layer under its 2x2 pool (the compact den ring);
    # a capture at features.1 stops there, so features.3 has no post step and is a plain backward
    ("gtzan", "fp32", None): _plain(_G, 0) + [("conv_bwd:features.3", _B + "_den_ring", None, 0)],
    ("gtzan", "bf16", None): _plain(_G, 0) + [("conv_bwd:features.3", _B + "_den_ring", None, 0)],
    ("gtzan", "bf16bwd", None): _plain(_G, 1) + [("conv_bwd:features.3", _B + "_den_ring", None, 1)],
    ("gtzan", "fp32", "features.1"): _plain(_G + (3,), 0),
    # VGGish: features.3 sits under the (2,4) pool (folded: pool_w 4) and above the WSquare first layer
    # without a pool between (the shared den map); without the map's division (capture at features.2)
    # the bf16 backward takes the folded pool through drsa_amd_conv_bwd_bf16_pw
    ("vggish", "fp32", None): _plain(_V, 0) + [("conv_bwd:features.3", _B + "_den_map", 4, 0)],
    ("vggish", "bf16", None): _plain(_V, 0) + [("conv_bwd:features.3", _B + "_den_map", 4, 0)],
    ("vggish", "bf16bwd", None): _plain(_V, 1) + [("conv_bwd:features.3", _B + "_den_map", 4, 1)],
    ("vggish", "bf16bwd", "features.12"): _plain(_V[:6], 1),
    ("vggish", "bf16bwd", "features.2"): _plain(_V, 1) + [("conv_bwd:features.3", _B + "_bf16_pw", 4, 1)],
}


def _models():
    g = gtzan128(), NameMapComposite(LRP_NAME_MAP_GTZAN), logmel(2, 128, 128, seed=3)
    v = (vggish(input_size=(32, 128)), NameMapComposite(LRP_NAME_MAP_VGGISH, canonizers=[SequentialMergeBatchNorm()]),
         logmel(2, 32, 128, seed=4))
    return {"gtzan": g, "vggish": v}


def _record(monkeypatch, eng, run):
    calls = []
    real = _capi.call

    def spy(name, *args):
        if name.startswith(_B):
            calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(_capi, "call", spy)
    eng.trace = []
    out = run().clone()
    torch.cuda.synchronize()
    tags = [t for t, _, _ in eng.trace if t.startswith("conv_bwd:")]
    eng.trace = None
    monkeypatch.setattr(_capi, "call", real)
    assert len(tags) == len(calls)
    seq = [(t, n, a[_POOL_W[n]] if n in _POOL_W else None,
            a[_WTS_BF16[n]] if n in _WTS_BF16 else int(n in (_B + "_bf16", _B + "_bf16_pw")))
           for t, (n, a) in zip(tags, calls)]
    return seq, out


@pytest.mark.parametrize("model,plan,capture", [
    ("gtzan", "fp32", None), ("gtzan", "bf16", None), ("gtzan", "bf16bwd", None), ("gtzan", "fp32", "features.1"),
    ("vggish", "fp32", None), ("vggish", "bf16", None), ("vggish", "bf16bwd", None), ("vggish", "bf16bwd", "features.12"),
    ("vggish", "bf16bwd", "features.2"),
])
def test_backward_entry_points_per_layer(model, plan, capture, monkeypatch):
    net, comp, x = _models()[model]
    if plan != "fp32":
        net, x = net.bfloat16(), x.bfloat16()
    eng = LRPEngine(copy.deepcopy(net).to(DEV), comp, bf16_backward=plan == "bf16bwd")
    assert eng.precision == plan[:4] and eng.bf16_backward == (plan == "bf16bwd")
    x = x.to(DEV)
    cls = torch.full((x.size(0),), 1, dtype=torch.int32, device=DEV)

    def run():
        if capture is not None:
            return eng.capture(x, capture, cls=cls)["rel"]
        eng.forward(x)
        return eng.backward(cls=cls)

    seq, out = _record(monkeypatch, eng, run)
    print((model, plan, capture), seq)
    assert seq == EXPECTED[(model, plan, capture)]
    seq2, out2 = _record(monkeypatch, eng, run)
    assert seq2 == seq
    assert torch.isfinite(out).all() and torch.equal(out, out2)
