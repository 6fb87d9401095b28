"""Gamma / ZPlus / WSquare / Flat on the dense head (GPU): the fused rule kernels
(csrc/linear_rules.hip, drsa_amd_linear_rule_fwd / _bwd) against the oracle's mode="exact", every
element equal, as tests/test_lrp_gpu.py does for the Epsilon head.

Shapes: the toy net (head 64 -> 32 -> 32 -> 2: partial N tiles, the short-K kernel), GTZAN-128
(classifier.0 with K = 2048: the long-K kernel), heads whose widths (24 or 132, 20, 3) are no multiple
of 16 with and without ReLUs (signed dense inputs; every (signed input, ReLU after) combination of
the short-K and the long-K kernels), and the ProjectionModel at the last conv block, whose a' is a signed classifier
input.  The autograd slow path (engine/hooks.py) is a second comparator at the 1e-3 relative L2 of
tests/test_hooks_gpu.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import lrp_ref
from lrp_common import gtzan128, logmel, ortho, spec, toy
from drsa_audio_amd.engine import EngineError, HookedAutograd, LRPEngine, clear_cache, get_engine
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY
from drsa_audio_amd.xai.explain.attribute import compute_relevances
from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
from drsa_audio_amd.xai.pixelflipping import PixelFlipping
from drsa_audio_amd.zennit.attribution import Gradient
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.core import Hook
from drsa_audio_amd.zennit.rules import AlphaBeta, Epsilon, Flat, Gamma, Pass, WSquare, ZPlus

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

RULES = {"gamma": lambda: Gamma(gamma=0.25, stabilizer=1e-7), "zplus": lambda: ZPlus(stabilizer=1e-7),
         "wsquare": lambda: WSquare(stabilizer=1e-7), "flat": lambda: Flat(stabilizer=1e-7)}


def _gpu(m):
    return copy.deepcopy(m).to(DEV)


def _conv_part(nm):
    return [e for e in nm if not e[0][0].startswith("classifier")]


def _head(nm, names, rules):
    return _conv_part(nm) + [([n], r) for n, r in zip(names, rules)]


def _toy_map(kind, names=("classifier.0", "classifier.2", "classifier.4")):
    return _head(LRP_NAME_MAP_TOY, names, [RULES[kind]() for _ in names])


def _gtzan_mixed():
    return _head(LRP_NAME_MAP_GTZAN, ("classifier.0", "classifier.3", "classifier.6"),
                 [Gamma(gamma=0.25, stabilizer=1e-7), ZPlus(stabilizer=1e-7), Gamma(gamma=0.1, stabilizer=1e-7)])


def _exact(m, nm, x, **kw):
    return lrp_ref.lrp(m, spec(nm), x, mode="exact", **kw)[1]


# ---------------------------------------------------------------- 1. toy net, every rule, every seed mode
@pytest.fixture(scope="module")
def toy_net():
    return toy()


@pytest.mark.parametrize("kind", ["gamma", "zplus", "wsquare", "flat"])
def test_toy_all_dense_layers(toy_net, kind):
    nm = _toy_map(kind)
    m, comp = _gpu(toy_net), NameMapComposite(nm)
    x3, x4 = logmel(3, 64, 64, seed=2), logmel(4, 64, 64, seed=3)
    assert isinstance(get_engine(m, comp), LRPEngine)
    # class mode and one-hot mode (the fused seed), B = 3
    for cls in (0, 1):
        assert torch.equal(compute_relevances(m, x3.to(DEV), comp, class_idx=cls).cpu(), _exact(toy_net, nm, x3, class_idx=cls))
    assert torch.equal(compute_relevances(m, x3.to(DEV), comp, class_idx=0, one_hot_encoded=True).cpu(),
                       _exact(toy_net, nm, x3, class_idx=0, one_hot_encoded=True))
    # all classes: class per row, and a seed tensor through the attributor
    assert torch.equal(compute_relevances(m, x4.to(DEV), comp, num_classes=2).cpu(), _exact(toy_net, nm, x4, num_classes=2))
    seed = torch.repeat_interleave(torch.eye(2), 2, dim=0)
    with Gradient(m, comp) as attr:
        _, R = attr(x4.to(DEV), seed.to(DEV))
    assert torch.equal(R.cpu(), _exact(toy_net, nm, x4, num_classes=2, one_hot_encoded=True))


def test_pass_on_relu_below_wsquare_or_flat(toy_net):
    """A Pass on a ReLU lets relevance through where z <= 0.  Below a layer that multiplies by its
    input that relevance is zero anyway; below WSquare / Flat it is not, so the layer under such a
    ReLU takes unmasked relevance (Gamma: its [z < 0] branch and den_n run in mid-head)."""
    names = ("classifier.0", "classifier.2", "classifier.4")
    nm = (_head(LRP_NAME_MAP_TOY, names, [RULES["gamma"](), RULES["flat"](), RULES["wsquare"]()])
          + [(["classifier.1", "classifier.3"], Pass())])
    x = logmel(3, 64, 64, seed=2)
    m, comp = _gpu(toy_net), NameMapComposite(nm)
    eng = get_engine(m, comp)
    assert [ds.mask for ds in eng.dense] == [False, False, False] and eng.dense[0].negden
    for cls in (0, 1):
        assert torch.equal(compute_relevances(m, x.to(DEV), comp, class_idx=cls).cpu(), _exact(toy_net, nm, x, class_idx=cls))


def _trunk(conv_rule, relu13):
    return ([(["features.0"], Flat(stabilizer=1e-7))] + [([f"features.{i}"], conv_rule()) for i in (3, 6, 9, 12)]
            + ([(["features.13"], Pass())] if relu13 else []))


@pytest.mark.parametrize("head", ["flat", "wsquare"])
@pytest.mark.parametrize("conv", ["gamma", "zplus", "epsilon"])
def test_wsquare_or_flat_head_above_the_last_conv_relu(toy_net, conv, head):
    """Towards the trunk the hand-off masks by [a > 0] and the conv rules form no [z < 0] branch
    (Gamma: den+ only).  The oracle under a Pass on the last conv block's ReLU sends WSquare / Flat
    relevance to dead channels too, so that composite is refused whatever the conv's rule; with the
    ReLU unmapped the same head equals the oracle, and the oracle itself tells the two apart."""
    conv_rule = {"gamma": lambda: Gamma(gamma=0.25, stabilizer=1e-7), "zplus": RULES["zplus"],
                 "epsilon": lambda: Epsilon(epsilon=1e-7)}[conv]
    names = ("classifier.0", "classifier.2", "classifier.4")
    head_rules = [([n], RULES[head]()) for n in names]
    x = logmel(3, 64, 64, seed=2)
    m = _gpu(toy_net)
    with pytest.raises(EngineError):
        get_engine(m, NameMapComposite(_trunk(conv_rule, True) + head_rules))
    with pytest.raises(EngineError):
        compute_relevances(m, x.to(DEV), NameMapComposite(_trunk(conv_rule, True) + head_rules), class_idx=0)
    nm = _trunk(conv_rule, False) + head_rules
    comp = NameMapComposite(nm)
    for cls in (0, 1):
        R = _exact(toy_net, nm, x, class_idx=cls)
        assert torch.equal(compute_relevances(m, x.to(DEV), comp, class_idx=cls).cpu(), R)
        if conv == "gamma":
            assert not torch.equal(_exact(toy_net, _trunk(conv_rule, True) + head_rules, x, class_idx=cls), R)
    # a Pass there below a head that multiplies by its input changes nothing and is accepted
    nm = _trunk(conv_rule, True) + [([n], RULES["gamma"]()) for n in names]
    assert torch.equal(compute_relevances(m, x.to(DEV), NameMapComposite(nm), class_idx=1).cpu(),
                       _exact(toy_net, nm, x, class_idx=1))


# ---------------------------------------------------------------- 2. GTZAN-128: the long-K layer, mixed head
@pytest.fixture(scope="module")
def gtzan_net():
    return gtzan128()


@pytest.mark.parametrize("cls", [0, 1])
def test_gtzan_mixed_head(gtzan_net, cls):
    """On these inputs class 0 has a negative logit and class 1 a positive one for both samples, so
    both the [z < 0] and the [z > 0] branch of the seed layer's Gamma run."""
    nm = _gtzan_mixed()
    x = logmel(2, seed=17)
    lg, R = lrp_ref.lrp(gtzan_net, spec(nm), x, mode="exact", class_idx=cls)
    assert bool((lg[:, cls] < 0).all()) if cls == 0 else bool((lg[:, cls] > 0).all())
    Rg = compute_relevances(_gpu(gtzan_net), x.to(DEV), NameMapComposite(nm), class_idx=cls)
    assert torch.isfinite(R).all() and torch.equal(Rg.cpu(), R)


# ---------------------------------------------------------------- 3. signed input A: a' of the last conv block
@pytest.mark.parametrize("which", ["toy-gamma", "toy-zplus", "gtzan-mixed"])
def test_projection_at_last_block_signed_head_input(toy_net, gtzan_net, which):
    if which.startswith("toy"):
        net, nm, U, x, name = toy_net, _toy_map(which[4:]), ortho(16, 1), logmel(2, 64, 64, seed=5), "class2"
    else:
        net, nm, U, x, name = gtzan_net, _gtzan_mixed(), ortho(128, 4), logmel(2, seed=17), "metal"
    hg = HeatmapGenerator(_gpu(net), U, nm, name, num_concepts=4, layer_idx=13)
    pm = ProjectionModel(net, 13, U, 4, case="toy" if which.startswith("toy") else "gtzan").eval()
    ref = lrp_ref.subspace_heatmaps(pm, spec(nm), 4, x, class_idx=hg.class_idx, mode="exact")
    hg.generate_subspace_heatmaps(x)
    for k in ("standard_heatmaps", "subspace_heatmaps", "mask"):
        assert np.array_equal(hg.info[k], ref[k]), k
    assert np.isfinite(ref["subspace_heatmaps"]).all()


# ---------------------------------------------------------------- 4. signed input B: no ReLU between Linears
def _odd_head_net(relu: bool, wide: bool):
    m = toy()
    torch.manual_seed(11)
    n0 = 132 if wide else 24
    layers = [nn.Linear(64, n0), nn.Linear(n0, 20)] + ([nn.ReLU()] if relu else []) + [nn.Linear(20, 3)]
    m.classifier = nn.Sequential(*layers)
    return m.eval()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("kind", ["gamma", "zplus"])
def test_linear_after_linear_odd_widths(kind, relu, wide):
    """classifier.1 reads classifier.0's raw output (signed); 24, 20 and 3 are no multiple of the
    16-wide tiles.  Without the ReLU the middle layer is Gamma with a signed input and no ReLU
    after it: all four terms of R_in and both denominators.  ``wide``: a first width of 132, so the
    middle layer's K = 132 takes the long-K forward (K >= 128, K % 4 == 0) with a second K chunk of
    4 and partial M and N tiles, under a signed input."""
    net = _odd_head_net(relu, wide)
    names = ("classifier.0", "classifier.1", "classifier.3" if relu else "classifier.2")
    nm = _toy_map(kind, names)
    x = logmel(2, 64, 64, seed=7)
    m, comp = _gpu(net), NameMapComposite(nm)
    for cls in (0, 2):
        R = _exact(net, nm, x, class_idx=cls)
        assert torch.isfinite(R).all() and float(R.abs().max()) > 0
        assert torch.equal(compute_relevances(m, x.to(DEV), comp, class_idx=cls).cpu(), R)


# ---------------------------------------------------------------- 5. the autograd slow path as a second comparator
class Same(Hook):
    def backward(self, module, grad_input, grad_output):
        return grad_input


def _rel(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


@pytest.mark.parametrize("which", ["toy-gamma", "toy-zplus", "toy-wsquare", "toy-flat", "gtzan-mixed"])
def test_hooks_slow_path_agrees(toy_net, gtzan_net, which):
    if which.startswith("toy"):
        net, nm, x, relu = toy_net, _toy_map(which[4:]), logmel(4, 64, 64, seed=6), "features.4"
    else:
        net, nm, x, relu = gtzan_net, _gtzan_mixed(), logmel(4, seed=6), "features.4"
    m = _gpu(net)
    plan, slow = NameMapComposite(nm), NameMapComposite(nm + [([relu], Same())])
    assert isinstance(get_engine(m, plan), LRPEngine) and isinstance(get_engine(m, slow), HookedAutograd)
    R_plan = compute_relevances(m, x.to(DEV), plan, class_idx=1)
    R_slow = compute_relevances(m, x.to(DEV), slow, class_idx=1)
    err = _rel(R_slow, R_plan)
    print(f"\n[{which}] slow path vs plan: max per-sample relative L2 {err:.2e}")
    assert err <= 1e-3


# ---------------------------------------------------------------- 6. PixelFlipping's grid with dense zplus / gamma
GRID = [{"convolutional": ("zplus",), "dense": ("zplus",), "first_layer": ("flat",)},
        {"convolutional": ("zplus",), "dense": ("gamma", 0.25), "first_layer": ("flat",)}]


@pytest.mark.parametrize("forward", ["torch", "engine"])
def test_pixelflipping_dense_rules(toy_net, forward):
    x = logmel(4, 64, 64, seed=9)
    pf = PixelFlipping(copy.deepcopy(toy_net), x, perturbation_size=16, num_classes=2, device=DEV, forward=forward)
    aupc, preds, flips, heatmaps = pf(GRID, plot=False)
    assert len(heatmaps) == 2
    m = _gpu(toy_net)
    for conf in GRID:
        name = pf._get_configuration_name(conf)
        dense = ZPlus(stabilizer=1e-7) if conf["dense"][0] == "zplus" else Gamma(gamma=0.25, stabilizer=1e-7)
        nm = ([(["features.0"], Flat(stabilizer=1e-7))]
              + [([f"features.{i}"], ZPlus(stabilizer=1e-7)) for i in (3, 6, 9, 12)]
              + [([f"features.{i}"], Pass()) for i in (1, 4, 7, 10, 13)]
              + [([f"classifier.{i}"], copy.copy(dense)) for i in (0, 2, 4)] + [(["classifier.1", "classifier.3"], Pass())])
        comp = NameMapComposite(nm)
        R = torch.cat([compute_relevances(m, x[2 * i:2 * i + 2].to(DEV), comp, class_idx=i) for i in range(2)], 0)
        assert torch.equal(heatmaps[name], R), name
        Rref = torch.cat([_exact(toy_net, nm, x[2 * i:2 * i + 2], class_idx=i) for i in range(2)], 0)
        assert torch.equal(R.cpu(), Rref), name
        assert np.isfinite(aupc[name]).all() and aupc[name].shape == (2, 2)


@pytest.mark.parametrize("forward", ["torch", "engine"])
@pytest.mark.parametrize("conv", [("gamma", 0.25), ("zplus",)])
@pytest.mark.parametrize("dense", ["wsquare", "flat"])
def test_pixelflipping_refuses_wsquare_and_flat_dense(toy_net, dense, conv, forward):
    """PixelFlipping maps Pass to every activation, the last conv block's ReLU among them, so a
    WSquare / Flat dense entry is refused under every conv rule (never a masked, wrong heatmap)."""
    x = logmel(4, 64, 64, seed=9)
    pf = PixelFlipping(copy.deepcopy(toy_net), x, perturbation_size=16, num_classes=2, device=DEV, forward=forward)
    with pytest.raises(EngineError):
        pf([{"convolutional": conv, "dense": (dense,), "first_layer": ("flat",)}], plot=False)


# ---------------------------------------------------------------- capture (preprocess_data's get_intermediate)
@pytest.mark.parametrize("layer_idx", [13, 10])
def test_get_intermediate_under_a_gamma_head(toy_net, layer_idx):
    from drsa_audio_amd.xai.drsa.preprocessing import get_intermediate
    nm = _toy_map("gamma")
    x = logmel(3, 64, 64, seed=12)
    _, _, (act, rel) = lrp_ref.lrp(toy_net, spec(nm), x, class_idx=1, mode="exact", capture=f"features.{layer_idx}")
    a, r = get_intermediate(_gpu(toy_net), x.to(DEV), NameMapComposite(nm), layer_idx, 1, attr_batch_size=2)
    assert torch.equal(a.cpu(), act) and torch.equal(r.cpu(), rel)


# ---------------------------------------------------------------- 7. what stays refused; Epsilon untouched
def test_refusals_stay_and_epsilon_head_is_untouched(toy_net):
    clear_cache()
    m = _gpu(toy_net)
    x = logmel(3, 64, 64, seed=2).to(DEV)
    R0 = compute_relevances(m, x, NameMapComposite(LRP_NAME_MAP_TOY), class_idx=1).clone()
    for bad in (AlphaBeta(alpha=2.0, beta=1.0, stabilizer=1e-7), Gamma(gamma=0.25, stabilizer=1e-7, zero_params="bias"),
                Epsilon(epsilon=1e-7, zero_params="bias"), Pass()):
        nm = _head(LRP_NAME_MAP_TOY, ("classifier.0", "classifier.2", "classifier.4"),
                   [bad, Epsilon(epsilon=1e-7), Epsilon(epsilon=1e-7)])
        with pytest.raises(EngineError):
            compute_relevances(m, x, NameMapComposite(nm), class_idx=1)
    with pytest.raises(EngineError):        # a rule other than Pass on an activation
        compute_relevances(m, x, NameMapComposite(_toy_map("gamma") + [(["classifier.1"], Epsilon())]), class_idx=1)
    for kind in ("gamma", "flat"):
        compute_relevances(m, x, NameMapComposite(_toy_map(kind)), class_idx=1)
    eng = get_engine(m, comp := NameMapComposite(LRP_NAME_MAP_TOY))
    assert all(ds.rp is None for ds in eng.dense)
    eng.trace = []
    R1 = compute_relevances(m, x, comp, class_idx=1)
    tags = [t for t, _, _ in eng.trace]
    eng.trace = None
    assert torch.equal(R1, R0)
    assert [t for t in tags if t.startswith("linear")] == (
        [f"linear_fwd:classifier.{i}" for i in (0, 2, 4)] + [f"linear_bwd:classifier.{i}" for i in (4, 2, 0)])
