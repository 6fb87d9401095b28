"""The schedule of a multi-layer capture (engine/schedule.py: ``capture_set``, ``schedule(taps=)``) on the host.

One forward and one LRP backward give the DRSA data of several layers: the backward records the raw relevance at
every tapped stage's output, so the launch above a tap leaves its post step out (as above ``stop_after``) and the
tapped step carries it (``tap_post``, applied by drsa_amd_relevance_post).  Held here without a GPU: which steps
change and which do not, that an int capture without taps is scheduled as before, and the refusals.
"""
from dataclasses import replace

import pytest

import engine_dispatch as E
from drsa_audio_amd._capi import POST_DIV, POST_MASK, POST_NONE
from drsa_audio_amd.engine.parse import EngineError, parse
from drsa_audio_amd.engine.schedule import capture_set, mark_bwd_bf16, schedule
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_VGGISH
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.rules import AlphaBeta, Flat


@pytest.fixture(scope="module")
def nets():
    return E.models()


def _parsed(net, comp, plan="fp32"):
    stages, dense = parse(net, comp, plan != "fp32")
    mark_bwd_bf16(stages, plan == "bf16bwd")
    return stages, dense


def _gtzan_with(rule, layer="features.6"):
    return NameMapComposite([(n, rule if n == [layer] else r) for n, r in LRP_NAME_MAP_GTZAN])


@pytest.mark.parametrize("plan", ["fp32", "bf16bwd"])
def test_vggish_three_layers(nets, plan):
    net, comp, x = nets["vggish"]
    stages, dense = _parsed(net, comp, plan)
    shape, bf16 = (x.size(0), x.size(2), x.size(3)), plan != "fp32"
    where, keep, stop, taps = capture_set(stages, ["features.19", "features.26", "features.33"])
    idx = [li for li, _ in where]
    assert [stages[li].relu_name for li in idx] == ["features.19", "features.26", "features.33"]
    assert [w for _, w in where] == ["relu"] * 3 and keep == tuple(idx) and stop == idx[0] and taps == tuple(idx[1:])
    assert idx[2] == len(stages) - 1                                    # layer 33: the last conv stage
    conv, head = schedule(stages, dense, *shape, keep, stop, 0, bf16=bf16, taps=taps)
    plain, plain_head = schedule(stages, dense, *shape, stop, stop, 0, bf16=bf16)
    assert [conv[li].form for li in idx] == ["unfused"] * 3
    assert conv[idx[0] + 1].post == POST_NONE and conv[idx[1] + 1].post == POST_NONE
    assert head[0].post == POST_NONE and plain_head[0].post == POST_DIV
    assert conv[idx[0]].tap_post == POST_NONE                           # the lowest tap: the walk ends there
    for li in idx[1:]:
        assert (conv[li].tap_post, conv[li].den) == (POST_DIV, "copy")
    for li, (sp, pl) in enumerate(zip(conv, plain)):
        if li in idx:
            continue
        # the step right above a tap differs by the post step it leaves out and by nothing else
        assert sp == (replace(pl, post=POST_NONE) if li - 1 in taps else pl), li
    assert head[1:] == plain_head[1:] and head[0] == replace(plain_head[0], post=POST_NONE)
    # the ReLU and the pool of one stage share the stage's relevance; an unpooled stage keeps nothing extra
    where, keep, stop, taps = capture_set(stages, ["features.20", "features.16", "features.19"])
    assert where == [(idx[0], "pool"), (idx[0] - 1, "relu"), (idx[0], "relu")]
    assert (keep, stop, taps) == ((idx[0],), idx[0] - 1, (idx[0],))
    assert capture_set(stages, ["features.20"]) == ([(idx[0], "pool")], (), idx[0], ())


@pytest.mark.parametrize("model,plan,capture", E.CASES)
def test_int_capture_without_taps_is_scheduled_as_before(nets, model, plan, capture):
    stages, dense, sched = E.host_schedule(*nets[model], plan=plan, capture=capture)
    assert E.said(stages, dense, sched) == (E.FWD_EXPECTED[(model, plan, capture)], E.EXPECTED[(model, plan, capture)])
    assert all(sp.tap_post == POST_NONE for sp in sched[0])
    if capture is not None:
        # the same layer through capture_set: a tuple capture, no taps, the same steps
        x = nets[model][2]
        where, keep, stop, taps = capture_set(stages, [capture])
        assert taps == ()
        assert schedule(stages, dense, x.size(0), x.size(2), x.size(3), keep, stop, 0, bf16=plan != "fp32",
                        taps=taps) == sched


def test_tapped_flat_stage_leaves_a_copy(nets):
    """A WSquare / Flat stage whose denominator the next backward would read as the shared map (no pool after it)
    leaves a per-sample copy once it is tapped above the lowest tap: drsa_amd_relevance_post reads that."""
    net, _, x = nets["gtzan"]
    stages, dense = _parsed(net, _gtzan_with(Flat(stabilizer=1e-7)))
    shape = (x.size(0), x.size(2), x.size(3))
    where, keep, stop, taps = capture_set(stages, ["features.4", "features.7"])
    conv, _ = schedule(stages, dense, *shape, keep, stop, 0, taps=taps)
    assert stages[2].name == "features.6" and stages[2].den_kind == "map" and taps == (2,)
    assert (conv[2].den, conv[2].tap_post, conv[3].post, conv[3].bwd) == ("copy", POST_DIV, POST_NONE, "drsa_amd_conv_bwd")
    # the unpooled form of the same: VGGish with Flat on features.14 reads the map in place until the stage is tapped
    net, _, x = nets["vggish"]
    rest = [([n for n in names if n != "features.14"], r) for names, r in LRP_NAME_MAP_VGGISH]
    comp = NameMapComposite([(["features.14"], Flat(stabilizer=1e-7))] + [(n, r) for n, r in rest if n],
                            canonizers=[SequentialMergeBatchNorm()])
    stages, dense = _parsed(net, comp)
    st = next(s for s in stages if s.name == "features.14")
    li = stages.index(st)
    assert st.den_kind == "map" and not st.pool
    shape = (x.size(0), x.size(2), x.size(3))
    assert schedule(stages, dense, *shape, None, 1, 0)[0][li].den == "map"
    conv, _ = schedule(stages, dense, *shape, None, 1, 0, taps=(li,))
    assert (conv[li].den, conv[li].tap_post, conv[li + 1].post, conv[li + 1].bwd) == ("copy", POST_DIV, POST_NONE,
                                                                                     "drsa_amd_conv_bwd")


def test_refusals(nets):
    net, comp, x = nets["gtzan"]
    stages, dense = _parsed(net, comp)
    with pytest.raises(ValueError, match="twice"):
        capture_set(stages, ["features.4", "features.7", "features.4"])
    with pytest.raises(EngineError, match="not a ReLU or MaxPool2d"):
        capture_set(stages, ["features.4", "features.6"])
    with pytest.raises(ValueError, match="ascending"):
        schedule(stages, dense, 2, 128, 128, None, 1, 0, taps=(3, 2))
    with pytest.raises(ValueError, match="above stop_after"):
        schedule(stages, dense, 2, 128, 128, None, 2, 0, taps=(2, 3))
    # a layer inside a ProjectionModel block
    pnet, pcomp, _ = E.toy_projection()
    pstages, _ = parse(pnet, pcomp)
    inside = next(st for st in pstages if st.proj is not None)
    with pytest.raises(EngineError, match="ProjectionModel"):
        capture_set(pstages, ["features.4", inside.relu_name])
    # the ReLU of a pooled AlphaBeta stage anywhere in the capture set
    stages, dense = _parsed(net, _gtzan_with(AlphaBeta(alpha=2.0, beta=1.0)))
    where, keep, stop, taps = capture_set(stages, ["features.4", "features.7"])
    with pytest.raises(EngineError, match="AlphaBeta"):
        schedule(stages, dense, 2, 128, 128, keep, stop, 0, taps=taps)
    # its pool output, and taps around it, are fine: the stage keeps no full-resolution map
    where, keep, stop, taps = capture_set(stages, ["features.4", "features.10"])
    conv, _ = schedule(stages, dense, 2, 128, 128, keep, stop, 0, taps=taps)
    assert (stop, taps) == (1, (3,)) and conv[3].tap_post == POST_DIV and conv[4].post == POST_NONE
    assert conv[3].post == POST_MASK and conv[2].post == POST_NONE     # into the AlphaBeta stage; above stop_after
