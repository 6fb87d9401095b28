"""The engine's schedule (engine/schedule.py) on the host: which entry point each layer gets is a pure
function of the parsed stages, the input shape and the library's ``*_has_kernel*`` queries, so it is held
to the literal sequences of engine_dispatch.py without a GPU (test_engine_dispatch_gpu.py holds the
executor to the same lists).  Also: the three alternative plan forms, with the values the engine launched
before the schedule existed; LRPEngine.check on a ProjectionModel net without a GPU; and the engine's
per-key cache, which must ask the library nothing the second time.
"""
from types import SimpleNamespace

import pytest

import engine_dispatch as E
from drsa_audio_amd._capi import POST_DIV, POST_DIV_MAP
from drsa_audio_amd.engine.plan import EngineError, LRPEngine
from drsa_audio_amd.engine.schedule import lib_has_kernel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.zennit.composites import NameMapComposite

_B = "drsa_amd_conv_bwd"


@pytest.fixture(scope="module")
def nets():
    return E.models()


@pytest.mark.parametrize("model,plan,capture", E.CASES)
def test_schedule_sequences(nets, model, plan, capture):
    fwd, bwd = E.said(*E.host_schedule(*nets[model], plan=plan, capture=capture))
    assert fwd == E.FWD_EXPECTED[(model, plan, capture)]
    assert bwd == E.EXPECTED[(model, plan, capture)]


@pytest.mark.parametrize("fanout,clones", [(2, 4), (1, 5), (0, 1)])
def test_toy_projection_schedule(fanout, clones):
    net, comp, x = E.toy_projection()
    LRPEngine.check(net, comp)          # parse alone: no GPU, no library call
    stages, dense, sched = E.host_schedule(net, comp, x, fanout=fanout)
    assert E.said(stages, dense, sched) == (E.TOY_FWD, E.TOY_BWD)
    # the 4 x 4 map of the last block runs padded to 8 x 8; h and a' are recomputed, not stored
    assert sched[0][-1].proj == (8, 8, False) and sched[0][-1].g_in == "proj"
    assert [sp.clones for sp in sched[0]] == [clones] * 5
    with pytest.raises(EngineError, match="projection layers need Epsilon rules"):
        LRPEngine.check(net, NameMapComposite(LRP_NAME_MAP_TOY))


def test_proj_store_flag():
    net, comp, x = E.toy_projection()
    stages, dense, sched = E.host_schedule(net, comp, x, fanout=2, proj_store=True)
    assert sched[0][-1].proj == (8, 8, True)        # projection_fwd is given the h and a' buffers
    assert E.said(stages, dense, sched) == (E.TOY_FWD, E.TOY_BWD)


def test_den_copy_flag(nets):
    """GTZAN with the per-sample denominator copy: a plain fused forward of the first layer, and features.3
    divides by the copy (drsa_amd_conv_bwd, POST_DIV) instead of the ring."""
    stages, dense, sched = E.host_schedule(*nets["gtzan"], den_copy=True)
    fwd, bwd = E.said(stages, dense, sched)
    assert sched[0][0].den == "copy" and fwd[0] == ("conv_fwd:features.0", "drsa_amd_conv_fwd", 1, 1)
    assert fwd[1:] == E.FWD_EXPECTED[("gtzan", "fp32", None)][1:]
    assert (sched[0][1].bwd, sched[0][1].post, sched[0][1].g_in) == (_B, POST_DIV, "sparse")
    assert bwd == E._plain((12, 9, 6, 3), 0)
    # VGGish bf16 backward: without the map's division, features.3 takes the folded pool on drsa_amd_conv_bwd_bf16_pw
    stages, dense, sched = E.host_schedule(*nets["vggish"], plan="bf16bwd", den_copy=True)
    assert sched[0][0].den == "copy" and sched[0][1].post == POST_DIV
    assert E.said(stages, dense, sched)[1] == E.EXPECTED[("vggish", "bf16bwd", "features.2")]


@pytest.mark.parametrize("plan", ["fp32", "bf16bwd"])
def test_pool24_unfolded_flag(nets, plan):
    """VGGish with the (2,4) pool backward as a step of its own (maxpool_bwd: drsa_amd_relevance_unpool), then
    features.3 on the den-map backward with a dense g (pool_w 2, no argmax bytes)."""
    stages, dense, sched = E.host_schedule(*nets["vggish"], plan=plan, pool24_sparse=False)
    sp = sched[0][1]
    assert stages[1].name == "features.3" and stages[1].pool_name == "features.6"
    assert (sp.g_in, sp.pool_w, sp.bwd, sp.post, sp.wts_bf16) == ("unpool", 2, _B + "_den_map", POST_DIV_MAP, plan != "fp32")
    fwd, bwd = E.said(stages, dense, sched)
    assert fwd == E.FWD_EXPECTED[("vggish", plan, None)]
    assert bwd == E.EXPECTED[("vggish", plan, None)][:-1] + [("conv_bwd:features.3", _B + "_den_map", 2, int(plan != "fp32"))]
    assert [s.g_in for s in sched[0]].count("unpool") == 1


def test_second_call_asks_the_library_nothing(nets):
    """LRPEngine._schedule, the engine's cache of schedules, on a stand-in that holds what it reads."""
    asked = []

    def has_kernel(query, *args):
        asked.append(query)
        return lib_has_kernel(query, *args)

    net, comp, x = nets["vggish"]
    stages, dense, want = E.host_schedule(net, comp, x, plan="bf16bwd", has_kernel=has_kernel)
    eng = SimpleNamespace(stages=stages, dense=dense, bf16=True, _flags={"has_kernel": has_kernel}, _schedules={})
    del asked[:]
    key = (2, 32, 128, None, None, 0)
    first = LRPEngine._schedule(eng, *key)
    assert first == want and len(asked) > 0
    n = len(asked)
    assert LRPEngine._schedule(eng, *key) is first and len(asked) == n
    LRPEngine._schedule(eng, 2, 32, 128, None, 1, 0)        # another call form: scheduled (and asked) anew
    assert len(asked) > n and len(eng._schedules) == 2
