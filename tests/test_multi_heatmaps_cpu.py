"""A projection matrix per row, on the host alone: the argument rejections of drsa_amd_projection_fwd_multi /
drsa_amd_projection_bwd_multi (fake device addresses, rejected before any device work), the bindings,
MultiProjectionModel's torch forward against ProjectionModel's, what LRPEngine.check accepts and refuses, the
ValueErrors of the model, the plan's row check and MultiHeatmapGenerator, and the plan cache key."""
from types import SimpleNamespace

import pytest
import torch

from drsa_audio_amd import _capi
from drsa_audio_amd.engine import cache_key
from drsa_audio_amd.engine.parse import parse
from drsa_audio_amd.engine.plan import EngineError, LRPEngine
from drsa_audio_amd.model.modify_model import MultiProjectionModel, ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.xai.explain.explainer import MultiHeatmapGenerator, get_class_composite
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.rules import Epsilon
from lrp_common import logmel, ortho, toy

US = [ortho(16, s) for s in (1, 2, 3)]


# --------------------------------------------------------------------------- the C ABI
_PTR = {k: 0x10000 * (i + 1) for i, k in enumerate(("a", "U", "P", "rows", "h", "ap", "pooled", "amax", "gp", "den", "G"))}
_ORDER = {
    "projection_fwd_multi": "a U P rows n_u h ap pooled amax B D H W pool stream",
    "projection_bwd_multi": "gp amax ap h a den U P rows n_u G B D H W K eps_proj eps_den fanout stream",
}
_VALID = dict(_PTR, n_u=3, B=2, D=64, H=8, W=32, pool=1, K=4, eps_proj=1e-6, eps_den=1e-7, fanout=1, stream=None)
_SHAPE = "W must be 8, 16 or a multiple of 32"
_BOTH = [(dict(U=None), "required"), (dict(P=None), "required"), (dict(rows=None), "required"),
         (dict(n_u=0), "at least one matrix"), (dict(n_u=-2), "at least one matrix"), (dict(D=0), "1 <= d <= 128"),
         (dict(D=129), "1 <= d <= 128"), (dict(W=24), _SHAPE), (dict(H=7), _SHAPE), (dict(H=4, W=8), _SHAPE),
         (dict(D=128, H=4096, W=4096), "2^31")]
_REJECTIONS = (
    *[("projection_fwd_multi", ch, msg) for ch, msg in _BOTH], *[("projection_bwd_multi", ch, msg) for ch, msg in _BOTH],
    ("projection_fwd_multi", dict(a=None), "required"), ("projection_fwd_multi", dict(pooled=None), "pool needs outputs"),
    ("projection_fwd_multi", dict(amax=None), "pool needs outputs"),
    ("projection_fwd_multi", dict(pool=0, ap=None), "without pool"),
    ("projection_bwd_multi", dict(gp=None), "required"), ("projection_bwd_multi", dict(a=None), "required"),
    ("projection_bwd_multi", dict(G=None), "required"), ("projection_bwd_multi", dict(K=0), "K must divide d"),
    ("projection_bwd_multi", dict(K=5), "K must divide d"), ("projection_bwd_multi", dict(fanout=3), "fanout must be"),
    ("projection_bwd_multi", dict(fanout=-1), "fanout must be"),
)


@pytest.mark.parametrize("entry,changes,needle", _REJECTIONS,
                         ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c, _ in _REJECTIONS])
def test_entry_points_reject_bad_arguments(entry, changes, needle):
    args = dict(_VALID, **changes)
    rc = getattr(_capi.lib(), "drsa_amd_" + entry)(*[args[k] for k in _ORDER[entry].split()])
    msg = _capi.lib().drsa_amd_last_error().decode()
    assert rc == _capi.DRSA_EINVAL, (rc, msg)
    assert needle in msg and msg.startswith(entry + ":"), msg


def test_bindings():
    for single in ("drsa_amd_projection_fwd", "drsa_amd_projection_bwd"):
        res, args = _capi.SIGNATURES[single + "_multi"]
        assert res == _capi.SIGNATURES[single][0] and len(args) == len(_capi.SIGNATURES[single][1]) + 2    # + u_row, n_u
        assert getattr(_capi.lib(), single + "_multi").argtypes == args


# --------------------------------------------------------------------------- the model
def test_layer_names_and_table():
    net = MultiProjectionModel(toy(), 7, US, 4, case="toy")
    names = [n for n, _ in net.features.named_children()]
    assert names[8:11] == ["projection", "subspacefilter", "invprojection"]
    assert names == [n for n, _ in ProjectionModel(toy(), 7, US[0], 4, case="toy").features.named_children()]
    assert net.U_tab.shape == (3, 16, 16) and all(torch.equal(net.U_tab[i], US[i]) for i in range(3))
    tab = torch.stack(US)
    assert MultiProjectionModel(toy(), 7, tab, 4, case="toy").U_tab is tab      # a table given as a tensor is not copied
    rules = get_class_composite(LRP_NAME_MAP_TOY, 4).rules(net)
    assert type(rules["features.subspacefilter"]).__name__ == "SubspaceHook"
    assert type(rules["features.projection"]).__name__ == type(rules["features.invprojection"]).__name__ == "Epsilon"


def _close(got, want, x):
    """Both are fp32 evaluations of the same sums, possibly in another order (a batched matmul against a flat one):
    two 16-term chains differ by at most about 2 * 16 ulps (4e-6) of their largest term, and the layers above carry
    that on at the scale of their own outputs; 1e-5 of the output's scale bounds it, four orders of magnitude below
    the effect of a wrong matrix."""
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


@torch.no_grad()
def test_forward_one_matrix_equals_projection_model():
    x = logmel(3, 64, 64, seed=5)
    for layer_idx in (7, 13):
        multi = MultiProjectionModel(toy(), layer_idx, US, 4, case="toy").eval()
        for m in range(3):
            multi.rows = [m] * 3
            _close(multi(x), ProjectionModel(toy(), layer_idx, US[m], 4, case="toy").eval()(x), x)


@torch.no_grad()
def test_forward_mixed_rows_equals_per_row_models():
    x, rows = logmel(5, 64, 64, seed=6), [2, 0, 2, 1, 0]
    multi = MultiProjectionModel(toy(), 7, US, 4, case="toy").eval()
    multi.rows = torch.tensor(rows)
    out = multi(x)
    singles = [ProjectionModel(toy(), 7, U, 4, case="toy").eval() for U in US]
    want = torch.cat([singles[m](x[i:i + 1]) for i, m in enumerate(rows)])
    _close(out, want, x)
    # the projection is orthogonal, so every matrix reproduces the plain model's logits up to rounding: that the
    # row's own matrix is used shows one level down, in the subspace coordinates h
    h = multi.features[:9](x)
    for i, m in enumerate(rows):
        other = singles[(m + 1) % 3].features[:9](x[i:i + 1])
        _close(h[i:i + 1], singles[m].features[:9](x[i:i + 1]), x)
        assert float((h[i:i + 1] - other).abs().max()) > 1e-2 * float(other.abs().max())


def test_model_value_errors():
    with pytest.raises(ValueError, match="empty"):
        MultiProjectionModel(toy(), 7, [], 4, case="toy")
    with pytest.raises(ValueError, match="matrix 1 has shape"):
        MultiProjectionModel(toy(), 7, [US[0], ortho(8, 1)], 4, case="toy")
    with pytest.raises(ValueError, match=r"\[n\]\[d\]\[d\]"):
        MultiProjectionModel(toy(), 7, torch.zeros(2, 16, 8), 4, case="toy")
    with pytest.raises(ValueError, match="divisor of d=16"):
        MultiProjectionModel(toy(), 7, US, 3, case="toy")
    with pytest.raises(ValueError, match="layer_idx"):
        MultiProjectionModel(toy(), 0, US, 4, case="toy")
    net, x = MultiProjectionModel(toy(), 7, US, 4, case="toy").eval(), logmel(2, 64, 64)
    with pytest.raises(ValueError, match="set .rows"):
        net(x)
    for rows, msg in (([0], "1 entries for a batch of 2"), ([0, 3], r"rows must lie in \[0, 2\]"), ([-1, 0], "rows must lie")):
        net.rows = rows
        with pytest.raises(ValueError, match=msg):
            net(x)


# --------------------------------------------------------------------------- the engine's host side
def test_check_accepts_and_parse_carries_the_table():
    for layer_idx in (7, 13):
        net, comp = MultiProjectionModel(toy(), layer_idx, US, 4, case="toy").eval(), get_class_composite(LRP_NAME_MAP_TOY, 4)
        LRPEngine.check(net, comp)
        proj = [st.proj for st in parse(net, comp)[0] if st.proj is not None]
        assert len(proj) == 1 and proj[0].multi and proj[0].U is None and proj[0].K == 4 and proj[0].d == 16
        assert torch.equal(proj[0].U_tab, torch.stack(US)) and proj[0].mask and proj[0].pool_after
    single = [st.proj for st in parse(ProjectionModel(toy(), 7, US[0], 4, case="toy"), comp)[0] if st.proj is not None]
    assert not single[0].multi and single[0].U_tab is None and single[0].d == 16


def _avgpool_after(net):
    net.features[11] = torch.nn.AvgPool2d(2)
    return net


_REFUSED = {
    "no Epsilon on the projection layers": (lambda net: net, lambda: NameMapComposite(LRP_NAME_MAP_TOY),
                                            "projection layers need Epsilon rules"),
    "another K on the SubspaceHook": (lambda net: net, lambda: get_class_composite(LRP_NAME_MAP_TOY, 2),
                                      "SubspaceHook num_concepts differs"),
    "a rule on the filter": (lambda net: net, lambda: NameMapComposite(
        list(LRP_NAME_MAP_TOY) + [(["features.invprojection", "features.projection", "features.subspacefilter"], Epsilon())]),
        "only SubspaceHook is supported"),
    "an AvgPool2d after the projection": (_avgpool_after, lambda: get_class_composite(LRP_NAME_MAP_TOY, 4),
                                          "after a ProjectionModel layer is not supported"),
}


@pytest.mark.parametrize("what", list(_REFUSED))
def test_check_refuses_what_projection_model_is_refused(what):
    change, comp, msg = _REFUSED[what]
    for net in (ProjectionModel(toy(), 7, US[0], 4, case="toy"), MultiProjectionModel(toy(), 7, US, 4, case="toy")):
        with pytest.raises(EngineError, match=msg):
            LRPEngine.check(change(net), comp())


def _plan(proj):
    """An LRPEngine as far as the row check needs it (no device: the check fails before the upload)."""
    eng = LRPEngine.__new__(LRPEngine)
    eng.stages, eng.device = [SimpleNamespace(proj=None), SimpleNamespace(proj=proj)], torch.device("cpu")
    return eng


def test_u_rows_value_errors():
    net, comp = MultiProjectionModel(toy(), 7, US, 4, case="toy"), get_class_composite(LRP_NAME_MAP_TOY, 4)
    multi = _plan(next(st.proj for st in parse(net, comp)[0] if st.proj is not None))
    assert multi._u_rows([2, 0, 1], 3).tolist() == [2, 0, 1] and multi._u_rows([2, 0, 1], 3).dtype == torch.int32
    assert multi._u_rows(torch.tensor([1, 1]), 2).tolist() == [1, 1]
    with pytest.raises(ValueError, match="pass u_rows"):
        multi._u_rows(None, 3)
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        multi._u_rows([0, 1], 3)
    with pytest.raises(ValueError, match=r"u_rows\[1\] = 3 is outside the table of 3 matrices \(row 1\)"):
        multi._u_rows([0, 3, 5], 3)
    with pytest.raises(ValueError, match=r"u_rows\[2\] = -1 .*\(row 2\)"):
        multi._u_rows(torch.tensor([0, 1, -1], dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="integer tensor"):
        multi._u_rows(torch.tensor([0.0, 1.0, 2.0]), 3)
    with pytest.raises(ValueError, match="sequence of table indices"):
        multi._u_rows(["rock", "jazz", "pop"], 3)
    single = _plan(next(st.proj for st in parse(ProjectionModel(toy(), 7, US[0], 4, case="toy"), comp)[0]
                        if st.proj is not None))
    assert single._u_rows(None, 3) is None
    with pytest.raises(ValueError, match="single-matrix plan"):
        single._u_rows([0, 0, 0], 3)


def test_generator_value_errors():
    Us = {"class1": US[0], "class2": US[1]}
    kw = dict(num_concepts=4, layer_idx=7, device="cpu")
    with pytest.raises(ValueError, match="unknown class name 'rock'"):
        MultiHeatmapGenerator(toy(), {"class1": US[0], "rock": US[1]}, LRP_NAME_MAP_TOY, case="toy", **kw)
    with pytest.raises(ValueError, match=r"Us\['class2'\] has shape \(8, 8\)"):
        MultiHeatmapGenerator(toy(), {"class1": US[0], "class2": ortho(8, 1)}, LRP_NAME_MAP_TOY, **kw)
    with pytest.raises(ValueError, match="num_concepts=3 must be a positive divisor of d=16"):
        MultiHeatmapGenerator(toy(), Us, LRP_NAME_MAP_TOY, num_concepts=3, layer_idx=7, device="cpu")
    with pytest.raises(ValueError, match="non-empty mapping"):
        MultiHeatmapGenerator(toy(), {}, LRP_NAME_MAP_TOY, **kw)
    with pytest.raises(ValueError, match="standard must be"):
        MultiHeatmapGenerator(toy(), Us, LRP_NAME_MAP_TOY, standard="mean", **kw)
    gen, x = MultiHeatmapGenerator(toy(), {"class1": US[0]}, LRP_NAME_MAP_TOY, **kw), logmel(2, 64, 64)
    assert gen.mapper == {"class1": 0, "class2": 1} and gen.table_index == {"class1": 0}
    with pytest.raises(ValueError, match=r"sample_classes\[1\] = 'class3' is not a known class \(row 1"):
        gen.generate_subspace_heatmaps(x, ["class1", "class3"])
    with pytest.raises(ValueError, match="sample_classes has 1 entries for a batch of 2"):
        gen.generate_subspace_heatmaps(x, ["class1"])
    # class2 is a class of the model, but no matrix of it is in the table
    with pytest.raises(ValueError, match=r"sample_classes\[0\] = 'class2' is not a known class \(row 0; known: \['class1'\]"):
        gen.generate_subspace_heatmaps(x, ["class2", "class1"])
    with pytest.raises(ValueError, match=r"subspace_classes\[1\] = 'class2'"):
        gen.generate_subspace_heatmaps(x, ["class2", "class1"], ["class1", "class2"])
    # a model on the CPU: what HeatmapGenerator raises (the engine has no CPU path)
    with pytest.raises(_capi.DrsaAmdError, match="GPU only"):
        gen.generate_subspace_heatmaps(x, ["class1", "class1"])


def test_cache_key_follows_the_table():
    tab = torch.stack(US)
    net, comp = MultiProjectionModel(toy(), 7, tab, 4, case="toy"), get_class_composite(LRP_NAME_MAP_TOY, 4)
    k0 = cache_key(net, comp)
    assert cache_key(net, comp) == k0
    net.rows = [0, 1]                   # per-call data: not part of the key
    assert cache_key(net, comp) == k0
    tab[1].neg_()                       # one entry edited in place
    assert cache_key(net, comp) != k0
