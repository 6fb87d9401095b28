"""Which entry point each layer of the test models gets: the expected launch sequences, shared by the CPU
test of the schedule (test_engine_schedule_cpu.py) and the GPU test of the executor
(test_engine_dispatch_gpu.py), and the two ways to obtain a sequence: from a schedule (``said``) and
from the arguments of observed library calls (``launched``).

A forward entry is (tag, entry point, pool code, ng), a backward entry (tag, entry point, pool_w,
wts_bf16); a field is None where the entry point has no such argument, and wts_bf16 is 1 for the _bf16
entries and 0 for drsa_amd_conv_bwd, which have none.

Inputs: batch 2; GTZAN at its classifier's 128 x 128 (the den-ring layer at 64 x 64 pooled); VGGish
at 32 x 128, the smallest map whose fifth block is still 2 x 4 (W % 4 == 0), with block 1 at W = 128
(W >= 32, W / 4 % 4 == 0: the (2,4) pool folds); the toy net at 64 x 64 with the ProjectionModel
layers after its last conv block (a 4 x 4 map, run padded to 8 x 8).
"""
from lrp_common import gtzan128, logmel, ortho, toy, vggish
from drsa_audio_amd.engine.parse import parse
from drsa_audio_amd.engine.schedule import lib_has_kernel, mark_bwd_bf16, schedule
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY, LRP_NAME_MAP_VGGISH
from drsa_audio_amd.xai.explain.explainer import get_class_composite
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite

_F, _B = "drsa_amd_conv_fwd", "drsa_amd_conv_bwd"
CASES = [("gtzan", "fp32", None), ("gtzan", "bf16", None), ("gtzan", "bf16bwd", None), ("gtzan", "fp32", "features.1"),
         ("vggish", "fp32", None), ("vggish", "bf16", None), ("vggish", "bf16bwd", None),
         ("vggish", "bf16bwd", "features.12"), ("vggish", "bf16bwd", "features.2")]


def _plain(layers, bf16):
    return [(f"conv_bwd:features.{i}", _B + ("_bf16" if bf16 else ""), None, bf16) for i in layers]


# (model, plan, capture layer) -> [(tag, entry point, pool_w, wts_bf16), ...] top-down.  Written down from
# a run of the engine before its four backward branches were folded into one method (the features.2
# capture: from reading those branches, then confirmed by the same run)
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


def _fwd(convs, bf16, head, unfused=None):
    """The trunk's conv forwards ((layer, pool code) each, ng 2: Gamma on a non-negative input), a
    maxpool_capture after layer ``unfused[0]`` (its pool is layer ``unfused[1]``), then the head."""
    out = []
    for i, pool in convs:
        out.append((f"conv_fwd:features.{i}", _F + ("_bf16" if bf16 else ""), pool, 2))
        if unfused and i == unfused[0]:
            out.append((f"maxpool:features.{unfused[1]}", "drsa_amd_maxpool_capture", None, None))
    return out + [(f"linear_fwd:classifier.{i}", "drsa_amd_linear_fwd", None, None) for i in head]


# (model, plan, capture layer) -> [(tag, entry point, pool code, ng), ...] bottom-up.  Recorded from the
# commit before the schedule existed (its forward() made every one of these choices inline), on an
# MI355X, by spying on _capi.call as ``launched`` below does
_GF = [(3, 1), (6, 1), (9, 1), (12, 1)]
_VF = [(3, 2), (7, 0), (10, 1), (14, 0), (17, 1), (21, 0), (24, 1), (28, 0), (31, 1)]
_G0 = [("conv_fwd:features.0", _F + "_den_ring", None, 1)]      # WSquare first layer, 2x2 pool: the den ring
_V0 = [("conv_fwd:features.0", _F, 0, 1)]                       # WSquare first layer, no pool: the shared map
FWD_EXPECTED = {
    ("gtzan", "fp32", None): _G0 + _fwd(_GF, 0, (0, 3, 6)),
    ("gtzan", "bf16", None): _G0 + _fwd(_GF, 1, (0, 3, 6)),
    ("gtzan", "bf16bwd", None): _G0 + _fwd(_GF, 1, (0, 3, 6)),
    # the captured layer keeps its full-resolution ReLU output: plain conv, per-sample den copy, maxpool_capture
    ("gtzan", "fp32", "features.1"): [("conv_fwd:features.0", _F, 0, 1), ("maxpool:features.2", "drsa_amd_maxpool_capture",
                                                                        None, None)] + _fwd(_GF, 0, (0, 3, 6)),
    ("vggish", "fp32", None): _V0 + _fwd(_VF, 0, (0, 4, 8)),
    ("vggish", "bf16", None): _V0 + _fwd(_VF, 1, (0, 4, 8)),
    ("vggish", "bf16bwd", None): _V0 + _fwd(_VF, 1, (0, 4, 8)),
    ("vggish", "bf16bwd", "features.12"): _V0 + _fwd([(i, 0 if i == 10 else p) for i, p in _VF], 1, (0, 4, 8), (10, 13)),
    ("vggish", "bf16bwd", "features.2"): _V0 + _fwd(_VF, 1, (0, 4, 8)),     # a ReLU without a pool: nothing to keep
}

# the toy net with ProjectionModel layers after features.12 (K = 4), HeatmapGenerator's standard="sum"
# (fanout 2), fp32; same source as FWD_EXPECTED
TOY_FWD = (_G0 + _fwd([(3, 1), (6, 1), (9, 1), (12, 0)], 0, ())
           + [("projection_fwd", "drsa_amd_projection_fwd", 1, None)]
           + [(f"linear_fwd:classifier.{i}", "drsa_amd_linear_fwd", None, None) for i in (0, 2, 4)])
TOY_BWD = _plain((12, 9, 6), 0) + [("conv_bwd:features.3", _B + "_den_ring", None, 0)]


def models():
    g = gtzan128(), NameMapComposite(LRP_NAME_MAP_GTZAN), logmel(2, 128, 128, seed=3)
    v = (vggish(input_size=(32, 128)), NameMapComposite(LRP_NAME_MAP_VGGISH, canonizers=[SequentialMergeBatchNorm()]),
         logmel(2, 32, 128, seed=4))
    return {"gtzan": g, "vggish": v}


def toy_projection():
    """The toy net of test_projection_small_map_gpu.py as HeatmapGenerator wraps it (layer_idx 13)."""
    return (ProjectionModel(toy(), 13, ortho(16, 1), 4, case="toy").eval(), get_class_composite(LRP_NAME_MAP_TOY, 4),
            logmel(2, 64, 64, seed=5))


def host_schedule(net, comp, x, plan="fp32", capture=None, fanout=0, has_kernel=lib_has_kernel, **flags):
    """Parse on the host and schedule at x's shape, as an engine of that plan does: (stages, dense, (conv steps, dense steps)).
    ``flags``: proj_store / den_copy / pool24_sparse.
    ``capture``: a layer name, as LRPEngine.capture takes it."""
    stages, dense = parse(net, comp, plan != "fp32")
    mark_bwd_bf16(stages, plan == "bf16bwd", has_kernel)
    li = keep = None
    if capture is not None:
        li = next(i for i, st in enumerate(stages) if capture in (st.relu_name, st.pool_name))
        keep = li if (stages[li].relu_name == capture and stages[li].pool) else None
    sched = schedule(stages, dense, *x.shape[:1], *x.shape[2:], keep, li, fanout, bf16=plan != "fp32",
                     has_kernel=has_kernel, **flags)
    return stages, dense, sched


def said(stages, dense, sched):
    """(forward sequence, backward conv sequence) a schedule stands for."""
    fwd, bwd = [], []
    for st, sp in zip(stages, sched[0]):
        ring = sp.fwd == _F + "_den_ring"
        fwd.append((f"conv_fwd:{st.name}", sp.fwd, None if ring else sp.pool, st.ng_fwd))
        if st.den_kind == "ab":
            fwd.append((f"conv_fwd_n:{st.name}", sp.fwd, sp.pool, 2))
        if sp.form == "unfused":
            fwd.append((f"maxpool:{st.pool_name}", "drsa_amd_maxpool_capture", None, None))
        if st.proj is not None:
            fwd.append(("projection_fwd", "drsa_amd_projection_fwd", int(st.proj.pool_after), None))
    for ds, dp in zip(dense, sched[1]):
        fwd.append((f"{dp.fwd[len('drsa_amd_'):]}:{ds.name}", dp.fwd, None, None))
    for st, sp in reversed(list(zip(stages, sched[0]))):
        if sp.bwd is not None and sp.bwd.startswith(_B):
            n = 2 if st.den_kind == "ab" else 1
            bwd += [(f"conv_bwd:{st.name}", sp.bwd, sp.pool_w if sp.bwd in _POOL_W else None, int(sp.wts_bf16))] * n
    return fwd, bwd


_POOL_W = {_B + "_bf16_pw": 2, _B + "_den_map": 2}            # entry -> index of its pool_w argument
_WTS_BF16 = {_B + "_den_map": 4, _B + "_den_ring": 3}         # entry -> index of its wts_bf16 argument
_BACKWARD_TAGS = ("linear_bwd", "linear_rule_bwd", "projection_bwd", "maxpool_bwd", "conv_bwd", "first_layer_bwd",
                  "ab_split", "ab_combine", "heatmap_sort")


def launched(tags, calls):
    """The same two sequences from what ran: the engine's trace tags and the (name, args) of the library
    calls it made through them, in order."""
    assert len(tags) == len(calls)
    fwd, bwd = [], []
    for t, (n, a) in zip(tags, calls):
        if t.startswith("conv_bwd:"):
            bwd.append((t, n, a[_POOL_W[n]] if n in _POOL_W else None,
                        a[_WTS_BF16[n]] if n in _WTS_BF16 else int(n in (_B + "_bf16", _B + "_bf16_pw"))))
        elif n in (_F, _F + "_bf16"):
            fwd.append((t, n, a[13], a[12]))
        elif n == _F + "_den_ring":
            fwd.append((t, n, None, a[11]))
        elif n == "drsa_amd_projection_fwd":
            fwd.append((t, n, a[11], None))
        elif t.split(":")[0] not in _BACKWARD_TAGS:
            fwd.append((t, n, None, None))
    return fwd, bwd
