"""Which entry points the engine calls for each layer, forward and backward (engine/plan.py forward() and
backward(), which walk the schedule of engine/schedule.py).

The schedule chooses between drsa_amd_conv_fwd, _bf16 and _den_ring with a fused or a separate pool, and
between drsa_amd_conv_bwd, _bf16, _bf16_pw, _den_map and _den_ring, per layer, by the plan's precision, the
pool under the layer, the post step of the layer below and the ``*_has_kernel*`` queries.  The tests here
only observe: they wrap ``_capi.call``, pair every call with its tag from the engine's trace, and compare
the two sequences (engine_dispatch.launched) with the literal lists of engine_dispatch.py, which
test_engine_schedule_cpu.py holds the schedule to as well, and with what the engine's own schedule stands
for (engine_dispatch.said).  A second run on the same engine must give the same bits.  Inputs and shapes:
engine_dispatch.py.
"""
import copy

import pytest
import torch

from engine_dispatch import CASES, EXPECTED, FWD_EXPECTED, launched, models, said
from drsa_audio_amd import _capi
from drsa_audio_amd.engine.plan import LRPEngine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _record(monkeypatch, eng, run):
    calls = []
    real = _capi.call

    def spy(name, *args):
        if name != "drsa_amd_first_layer_den":      # made once per map size, outside the trace
            calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(_capi, "call", spy)
    eng.trace = []
    out = run().clone()
    torch.cuda.synchronize()
    tags = [t for t, _, _ in eng.trace]
    eng.trace = None
    monkeypatch.setattr(_capi, "call", real)
    return launched(tags, calls), out


@pytest.mark.parametrize("model,plan,capture", CASES)
def test_backward_entry_points_per_layer(model, plan, capture, monkeypatch):
    net, comp, x = models()[model]
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

    (fwd, bwd), out = _record(monkeypatch, eng, run)
    print((model, plan, capture), fwd, bwd)
    assert bwd == EXPECTED[(model, plan, capture)]
    assert fwd == FWD_EXPECTED[(model, plan, capture)]
    stop = None if capture is None else eng.capture_stage(capture)[0]
    assert (fwd, bwd) == said(eng.stages, eng.dense, eng._schedule(*eng.last["key"], stop, 0))
    seq2, out2 = _record(monkeypatch, eng, run)
    assert seq2 == (fwd, bwd)
    assert torch.isfinite(out).all() and torch.equal(out, out2)
