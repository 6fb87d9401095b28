"""MultiHeatmapGenerator (a mixed-class batch in one pass, a projection matrix per row) against the loop of
per-class HeatmapGenerators it replaces: every key of ``info_device``, row for row, bit for bit.  A row's arithmetic
does not depend on its batch (test_gtzan96x192_one_sample_of_a_large_batch) and the multi-matrix kernels run the
single-matrix chains (test_projection_multi_gpu.py), so equality is the gate, not a tolerance.

Toy net at layer_idx 7 (d = 16, K = 4) and 13 (the 4 x 4 map on the zero-padded route), both ``standard`` modes, and
GTZAN-128 at layer_idx 7 (d = 64, K = 4, three genres).  Also: the exact-order oracle per class, a second call with
permuted rows (the permuted results, nothing compiled, nothing scheduled), subspace class != attributed class, and
the fused modes of concept_flipping / interclass_concept_flipping against the unfused ones."""
import copy
import functools

import numpy as np
import pytest
import torch

import lrp_ref
from drsa_audio_amd.engine import plan as plan_mod
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY
from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator, MultiHeatmapGenerator
from drsa_audio_amd.xai.pixelflipping.cpf import concept_flipping, interclass_concept_flipping
from lrp_common import gtzan128, logmel, ortho, spec, toy

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KEYS = ("standard_heatmaps", "standard_relevance", "subspace_heatmaps", "subspace_relevances", "mask")
TOY_US = {"class1": ortho(16, 11), "class2": ortho(16, 12)}
TOY_ROWS = ["class2", "class1", "class2", "class2", "class1"]


@functools.lru_cache(maxsize=None)
def _toy():
    return toy().to(DEV), logmel(5, 64, 64, seed=5).to(DEV)


def _loop(net, Us, name_map, x, sample_classes, subspace_classes, **kw):
    """The per-class loop: for every (subspace class, attributed class) pair of the batch, one HeatmapGenerator over
    the pair's rows; {key: [B, ...]} assembled row for row."""
    out = {}
    for pair in sorted(set(zip(subspace_classes, sample_classes))):
        rows = [i for i, p in enumerate(zip(subspace_classes, sample_classes)) if p == pair]
        hg = HeatmapGenerator(net, Us[pair[0]], name_map, pair[1], device=DEV, **kw)
        hg.generate_subspace_heatmaps(x[rows], to_host=False)
        for k in KEYS:
            v = hg.info_device[k]
            out.setdefault(k, torch.empty((x.size(0),) + tuple(v.shape[1:]), dtype=v.dtype, device=DEV))[rows] = v
    return out


def _same(got, want, what=""):
    assert set(got) == set(want) == set(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("standard", ["clone", "sum"])
@pytest.mark.parametrize("layer_idx", [7, 13])
def test_toy_mixed_batch_equals_per_class_loop(layer_idx, standard, monkeypatch):
    net, x = _toy()
    kw = dict(num_concepts=4, layer_idx=layer_idx, standard=standard)
    want = _loop(net, TOY_US, LRP_NAME_MAP_TOY, x, TOY_ROWS, TOY_ROWS, **kw)
    gen = MultiHeatmapGenerator(net, TOY_US, LRP_NAME_MAP_TOY, device=DEV, **kw)
    gen.generate_subspace_heatmaps(x, TOY_ROWS)
    _same(gen.info_device, want)
    # the host copies: HeatmapGenerator's keys, shapes and dtypes
    assert set(gen.info) == set(KEYS) | {"input"} and np.array_equal(gen.info["input"], x.cpu().numpy())
    for k in KEYS:
        assert isinstance(gen.info[k], np.ndarray) and np.array_equal(gen.info[k], want[k].cpu().numpy()), k
    assert gen.info["mask"].dtype == np.int64 and gen.info["subspace_heatmaps"].shape == (5, 4, 64, 64)
    # the two classes' matrices tell apart: a row through the other class's matrix gives other concept heatmaps
    swapped = ["class1" if c == "class2" else "class2" for c in TOY_ROWS]
    gen.generate_subspace_heatmaps(x, TOY_ROWS, swapped, to_host=False)
    assert all(not torch.equal(gen.info_device["subspace_heatmaps"][i], want["subspace_heatmaps"][i]) for i in range(5))
    # a second call, rows and classes permuted: the permuted results, and neither a plan nor a schedule is made
    made = []
    prepare, schedule = plan_mod.LRPEngine._prepare_conv, plan_mod.schedule
    monkeypatch.setattr(plan_mod.LRPEngine, "_prepare_conv", lambda self, st: made.append("prepare") or prepare(self, st))
    monkeypatch.setattr(plan_mod, "schedule", lambda *a, **k: made.append("schedule") or schedule(*a, **k))
    perm = [3, 0, 4, 2, 1]
    gen.generate_subspace_heatmaps(x[perm], [TOY_ROWS[i] for i in perm], to_host=False)
    assert made == []
    _same(gen.info_device, {k: v[perm] for k, v in want.items()}, "permuted")


def test_toy_equals_exact_oracle_per_class():
    net, x = _toy()
    gen = MultiHeatmapGenerator(net, TOY_US, LRP_NAME_MAP_TOY, num_concepts=4, layer_idx=7, device=DEV)
    gen.generate_subspace_heatmaps(x, TOY_ROWS)
    cpu = copy.deepcopy(net).cpu()
    for idx, c in enumerate(("class1", "class2")):
        rows = [i for i, r in enumerate(TOY_ROWS) if r == c]
        ref = lrp_ref.subspace_heatmaps(ProjectionModel(cpu, 7, TOY_US[c], 4, case="toy").eval(), spec(LRP_NAME_MAP_TOY),
                                        4, x[rows].cpu(), class_idx=idx, mode="exact")
        for k in ("standard_heatmaps", "subspace_heatmaps", "subspace_relevances", "mask"):
            assert np.array_equal(gen.info[k][rows], ref[k]), (c, k)


@pytest.mark.parametrize("layer_idx", [7, 13])
def test_toy_interclass_rows(layer_idx):
    """The subspace class differs from the attributed class on some rows: every (subspace, attributed) pair."""
    net, x = _toy()
    attributed = ["class1", "class2", "class2", "class1", "class2"]
    kw = dict(num_concepts=4, layer_idx=layer_idx)
    want = _loop(net, TOY_US, LRP_NAME_MAP_TOY, x, attributed, TOY_ROWS, **kw)
    gen = MultiHeatmapGenerator(net, TOY_US, LRP_NAME_MAP_TOY, device=DEV, **kw)
    gen.generate_subspace_heatmaps(x, attributed, TOY_ROWS, to_host=False)
    _same(gen.info_device, want)


def test_gtzan128_three_genres():
    net, x = gtzan128().to(DEV), logmel(6, seed=21).to(DEV)
    Us = {"blues": ortho(64, 1), "metal": ortho(64, 2), "rock": ortho(64, 3)}
    rows = ["rock", "blues", "metal", "rock", "metal", "blues"]
    kw = dict(num_concepts=4, layer_idx=7)
    want = _loop(net, Us, LRP_NAME_MAP_GTZAN, x, rows, rows, **kw)
    gen = MultiHeatmapGenerator(net, Us, LRP_NAME_MAP_GTZAN, device=DEV, **kw)
    gen.generate_subspace_heatmaps(x, rows, to_host=False)
    _same(gen.info_device, want)
    perm = [5, 2, 0, 4, 1, 3]
    gen.generate_subspace_heatmaps(x[perm], [rows[i] for i in perm], to_host=False)
    _same(gen.info_device, {k: v[perm] for k, v in want.items()}, "permuted")


def test_concept_flipping_fused_equals_unfused():
    net, _ = _toy()
    x = logmel(4, 64, 64, seed=41)                  # 2 classes x 2 samples
    for standard_r in (False, True):
        kw = dict(Us=TOY_US, num_concepts=4, case="toy", device=DEV, standard_r=standard_r, return_heatmaps=True)
        a = concept_flipping(net, x, LRP_NAME_MAP_TOY, 7, **kw)
        b = concept_flipping(net, x, LRP_NAME_MAP_TOY, 7, fused=True, **kw)
        assert len(a) == len(b) == 4 and torch.equal(a[3], b[3])
        for u, f in zip(a[:3], b[:3]):
            assert np.array_equal(np.asarray(u), np.asarray(f))


@pytest.mark.parametrize("reference_indexing", [True, False])
def test_interclass_concept_flipping_fused_equals_unfused(reference_indexing):
    net, _ = _toy()
    x = logmel(4, 64, 64, seed=41)
    layers, dims = [4, 7, 13], {4: 8, 7: 16, 13: 16}
    Us = {l: {g: ortho(dims[l], 10 * l + i) for i, g in enumerate(("class1", "class2"))} for l in layers}
    kw = dict(toy=True, num_concepts=4, device=DEV, Us=Us, layer_idcs=layers, reference_indexing=reference_indexing)
    a = interclass_concept_flipping(net, x, LRP_NAME_MAP_TOY, **kw)
    b = interclass_concept_flipping(net, x, LRP_NAME_MAP_TOY, fused=True, **kw)
    assert len(a) == len(b) == len(layers)
    for u, f in zip(a, b):
        assert u.shape == (2, 2) and np.array_equal(u, f), (u, f)
