"""Whole plans over average-pooled conv blocks (GPU), against tests/avgpool_ref.py: the oracle's own walk in
mode "exact" with the AvgPool2d layer supplied from there, bit for bit (B = 3 unless a seed needs another).

The toy net (64 x 64, lrp_common.toy()'s sizes) with every pool averaged, with max / avg alternating, and with a
last pool of (4,4) that is global; the pool unmapped, under Norm and under Epsilon; the convs under Gamma, ZPlus,
Epsilon and no rule over a WSquare or Flat first layer; the three seeds.  One block-depth-2 BN net at 64 x 128
with a (2,4) average pool under the merge canonizer, one 5x5-conv net, HeatmapGenerator with the projection at a
max-pooled stage between averaged ones, DRSA data at a ReLU and at an AvgPool2d layer.  Second comparators: the
float64 anchor (lrp_common.f64_anchored_check), the autograd slow path (1e-3 relative L2, test_hooks_gpu.TOL),
one bf16 plan (test_bf16_gpu's method and 5e-3), and PixelFlipping's engine forward against the torch forward
(1e-4, test_pixelflipping_gpu)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import avgpool_ref as A
import convk_ref
import drsa_ref
import lrp_ref
from lrp_common import f64_anchored_check, logmel, ortho, rel_l2, spec
from drsa_audio_amd.engine import HookedAutograd, LRPEngine, get_engine
from drsa_audio_amd.model.create_model import VGGType
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.xai.explain.attribute import compute_relevances
from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.core import Hook
from drsa_audio_amd.zennit.rules import Epsilon, Flat, Gamma, Norm, Pass, WSquare, ZPlus

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

_CONVS = ["features.0", "features.3", "features.6", "features.9", "features.12"]
_RELUS = ["features.1", "features.4", "features.7", "features.10", "features.13"]
_HEAD = [([f"classifier.{i}"], Epsilon(epsilon=1e-7)) for i in (0, 2, 4)]
RULES = {
    "gamma_flat": LRP_NAME_MAP_TOY,
    "gamma_wsquare": [(["features.0"], WSquare(stabilizer=1e-7))] + LRP_NAME_MAP_TOY[1:],
    "zplus": [(["features.0"], Flat(stabilizer=1e-7)), (_CONVS[1:], ZPlus(stabilizer=1e-7))] + _HEAD,
    "epsilon": [(_CONVS, Epsilon(epsilon=1e-6))] + _HEAD,
    "norule": [(["features.0"], Flat(stabilizer=1e-7)), (["features.3", "features.9"], Gamma(gamma=0.8, stabilizer=1e-7))] + _HEAD,
    "nothing": _HEAD,
}
NETS = {
    "all_avg": dict(kinds=("avg",) * 5),
    "alternating": dict(kinds=("max", "avg", "max", "avg", "max")),
    "avg_first": dict(kinds=("avg", "max", "avg", "max", "avg")),
    "global_last": dict(kinds=("avg",) * 5, last_k=(4, 4)),
}
POOL_RULES = {"unmapped": None, "norm": Norm(stabilizer=1e-6), "epsilon": Epsilon(epsilon=0.01)}


@pytest.fixture(scope="module")
def nets():
    return {name: A.toy_avg(**kw) for name, kw in NETS.items()}


def _gpu(net):
    return copy.deepcopy(net).to(DEV)


def _name_map(net, rules, pool_rule):
    nm = list(RULES[rules])
    if POOL_RULES[pool_rule] is not None:
        nm = nm + [(A.pool_names(net), POOL_RULES[pool_rule])]
    return nm


@pytest.mark.parametrize("pool_rule", list(POOL_RULES))
@pytest.mark.parametrize("rules", list(RULES))
@pytest.mark.parametrize("name", list(NETS))
def test_compute_relevances_bit_exact(nets, name, rules, pool_rule):
    net, x = nets[name], logmel(3, 64, 64, seed=5)
    nm = _name_map(net, rules, pool_rule)
    _, R = A.lrp(net, spec(nm), x, class_idx=1, mode="exact")
    Rg = compute_relevances(_gpu(net), x.to(DEV), NameMapComposite(nm), class_idx=1)
    assert float(R.abs().max()) > 0 and torch.isfinite(R).all()
    assert Rg.shape == x.shape and torch.equal(Rg.cpu(), R)


@pytest.mark.parametrize("seed", ["class", "one_hot", "all_classes"])
@pytest.mark.parametrize("pool_rule", ["unmapped", "norm"])
def test_seeds_bit_exact(nets, seed, pool_rule):
    """class: logit x mask; one_hot: the mask; all_classes: the block-diagonal mask of a class-ordered batch, which
    needs a batch divisible by the toy net's 2 classes (B = 4 there)."""
    net = nets["all_avg"]
    nm = _name_map(net, "gamma_flat", pool_rule)
    kw = {"class": dict(class_idx=0), "one_hot": dict(class_idx=1, one_hot_encoded=True), "all_classes": dict(num_classes=2)}[seed]
    x = logmel(4 if seed == "all_classes" else 3, 64, 64, seed=8)
    _, R = A.lrp(net, spec(nm), x, mode="exact", **kw)
    Rg = compute_relevances(_gpu(net), x.to(DEV), NameMapComposite(nm), **kw)
    assert float(R.abs().max()) > 0 and torch.equal(Rg.cpu(), R)


def test_pass_on_the_relus_with_norm_on_the_pools(nets):
    """EpsilonGammaBox-style activations (Pass) over Norm pools: a * s is zero at a dead pixel, so the plan's ReLU
    mask changes at most the sign of a zero."""
    net, x = nets["all_avg"], logmel(3, 64, 64, seed=9)
    nm = LRP_NAME_MAP_TOY + [(_RELUS, Pass()), (A.pool_names(net), Norm(stabilizer=1e-6))]
    _, R = A.lrp(net, spec(nm), x, class_idx=1, mode="exact")
    Rg = compute_relevances(_gpu(net), x.to(DEV), NameMapComposite(nm), class_idx=1)
    assert float(R.abs().max()) > 0 and torch.equal(Rg.cpu(), R)


def _bn_net():
    """Block depth 2 with BatchNorm in trunk and head at 64 x 128: a (2,4) average pool first, then (2,2) max and
    (4,4) average; BN statistics randomised so that the merge is not a no-op."""
    torch.manual_seed(3)
    net = VGGType(n_filters=(8, 16, 16), n_dense=32, n_classes=3, pool_kernels=((2, 4), (2, 2), (4, 4)), dropout=0.0,
                  input_size=(64, 128), conv_bn=True, dense_bn=True, block_depth=2, pool="avg").eval()
    A.swap_pools(net, ("avg", "max", "avg"))
    g = torch.Generator().manual_seed(103)
    for mod in net.modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
            n = mod.num_features
            mod.running_mean.copy_(0.1 * torch.randn(n, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
            mod.weight.data.copy_(0.8 + 0.4 * torch.rand(n, generator=g))
            mod.bias.data.copy_(0.05 * torch.randn(n, generator=g))
    return net


@pytest.mark.parametrize("pool_rule", ["unmapped", "norm"])
def test_bn_depth2_net_with_a_2x4_average_pool(pool_rule):
    net, x = _bn_net(), logmel(3, 64, 128, seed=11)
    convs = [f"features.{n}" for n, m in net.features.named_children() if isinstance(m, nn.Conv2d)]
    lins = [f"classifier.{n}" for n, m in net.classifier.named_children() if isinstance(m, nn.Linear)]
    nm = [(convs[:1], Flat(stabilizer=1e-7)), (convs[1:], Gamma(gamma=0.3, stabilizer=1e-7)), (lins, Epsilon(epsilon=1e-7))]
    if pool_rule == "norm":
        nm.append((A.pool_names(net), Norm(stabilizer=1e-6)))
    _, R = A.lrp(lrp_ref.merge_batch_norm(net), spec(nm), x, class_idx=2, mode="exact")
    comp = NameMapComposite(nm, canonizers=[SequentialMergeBatchNorm()])
    Rg = compute_relevances(_gpu(net), x.to(DEV), comp, class_idx=2)
    assert float(R.abs().max()) > 0 and torch.equal(Rg.cpu(), R)


@pytest.mark.parametrize("rules,pool_rule", [("gamma_flat", "unmapped"), ("gamma_wsquare", "norm"), ("norule", "epsilon")])
def test_5x5_convs_bit_exact(monkeypatch, rules, pool_rule):
    """K x K convs over average pools.  The oracle's ExactOps.conv / conv_t are 3x3 only; as in
    test_convk_plan_gpu.py they dispatch every other module to tests/convk_ref.py."""
    monkeypatch.setattr(lrp_ref.ExactOps, "conv", classmethod(lambda cls, m, x, w, b: convk_ref.conv(x, w, b)))
    monkeypatch.setattr(lrp_ref.ExactOps, "conv_t", classmethod(lambda cls, m, x_shape, w, g: convk_ref.conv_t(g, w)))
    net, x = A.toy_avg(("avg", "max", "avg", "avg", "avg"), conv_kernel=(5, 5)), logmel(3, 64, 64, seed=12)
    nm = _name_map(net, rules, pool_rule)
    _, R = A.lrp(net, spec(nm), x, class_idx=1, mode="exact")
    Rg = compute_relevances(_gpu(net), x.to(DEV), NameMapComposite(nm), class_idx=1)
    assert float(R.abs().max()) > 0 and torch.equal(Rg.cpu(), R)


@pytest.mark.parametrize("standard", ["sum", "clone"])
@pytest.mark.parametrize("pool_rule", ["unmapped", "norm"])
def test_heatmap_generator_bit_exact(standard, pool_rule):
    """The projection at features.7, a max-pooled stage, with averaged stages below it (they run the K + 1 / K
    relevance clones) and above it."""
    net, U, x = A.toy_avg(("avg", "avg", "max", "avg", "avg")), ortho(16, 1), logmel(3, 64, 64, seed=6)
    nm = _name_map(net, "gamma_flat", pool_rule)
    hg = HeatmapGenerator(_gpu(net), U, nm, "class2", num_concepts=4, layer_idx=7, standard=standard)
    pm = ProjectionModel(net, 7, U, 4, case="toy").eval()
    ref = A.subspace_heatmaps(pm, spec(nm), 4, x, class_idx=hg.class_idx, mode="exact", standard=standard)
    hg.generate_subspace_heatmaps(x)
    for k in ("standard_heatmaps", "standard_relevance", "subspace_heatmaps", "subspace_relevances", "mask"):
        assert np.array_equal(hg.info[k], ref[k]), k
    assert np.abs(ref["subspace_heatmaps"]).max() > 0


@pytest.mark.parametrize("pool_rule", ["unmapped", "norm"])
def test_drsa_data_at_a_relu_and_at_an_avgpool_layer(nets, pool_rule):
    """features.4 (the ReLU above an average pool: its relevance is dense, the pool backward's by-product) and
    features.5 (the pool): get_intermediate of each against the oracle's capture=, then both in one
    preprocess_data_layers pass against the single-layer oracle vectors."""
    from drsa_audio_amd.xai.drsa.preprocessing import get_intermediate, get_intermediates, preprocess_data_layers
    net, x = nets["all_avg"], logmel(3, 64, 64, seed=13)
    nm = _name_map(net, "gamma_flat", pool_rule)
    comp, m, want = NameMapComposite(nm), _gpu(net), {}
    for layer in (4, 5):
        _, _, (act, rel) = A.lrp(net, spec(nm), x, class_idx=1, mode="exact", capture=f"features.{layer}")
        a, r = get_intermediate(m, x.to(DEV), comp, layer, 1)
        assert float(rel.abs().max()) > 0 and torch.equal(a.cpu(), act) and torch.equal(r.cpu(), rel), layer
        want[layer] = (act, rel)
    both = get_intermediates(m, x.to(DEV), comp, [5, 4], 1)
    for layer in (4, 5):
        assert torch.equal(both[layer][0].cpu(), want[layer][0]) and torch.equal(both[layer][1].cpu(), want[layer][1])
    np.random.seed(5)
    vec = {}
    for layer in (4, 5):
        act, rel = want[layer]
        idx = drsa_ref.sample_spatial_locations(3, act.shape[-2:], 4)
        va = drsa_ref.get_vectors_from_maps(act, idx)
        vec[layer] = (va, drsa_ref.compute_context_vectors(va, drsa_ref.get_vectors_from_maps(rel, idx)))
    np.random.seed(5)
    out = preprocess_data_layers(m, x.to(DEV), comp, [4, 5], 1, num_locations=4)
    for layer in (4, 5):
        assert torch.equal(out[layer][0].cpu(), vec[layer][0]) and torch.equal(out[layer][1].cpu(), vec[layer][1]), layer


def test_capture_below_and_above_other_averaged_stages(nets):
    """Three layers of the alternating net in one pass: a max-pooled ReLU, the AvgPool2d above it and the ReLU of
    the averaged stage above that."""
    from drsa_audio_amd.xai.drsa.preprocessing import get_intermediates
    net, x = nets["alternating"], logmel(3, 64, 64, seed=14)
    nm = _name_map(net, "gamma_flat", "norm")
    got = get_intermediates(_gpu(net), x.to(DEV), NameMapComposite(nm), [1, 5, 10], 1)
    for layer in (1, 5, 10):
        _, _, (act, rel) = A.lrp(net, spec(nm), x, class_idx=1, mode="exact", capture=f"features.{layer}")
        assert torch.equal(got[layer][0].cpu(), act) and torch.equal(got[layer][1].cpu(), rel), layer


# --------------------------------------------------------------------------- second comparators
class Same(Hook):
    def backward(self, module, grad_input, grad_output):
        return grad_input


@pytest.mark.parametrize("pool_rule", ["unmapped", "norm"])
def test_f64_anchor_and_slow_path(nets, pool_rule):
    """16 samples of the all-avg toy net: the plan next to the reference's own fp32 order against float64
    (lrp_common's ratios), and the plan against the autograd slow path, which a pass-through user Hook on a ReLU
    selects, within 1e-3 relative L2 per sample (test_hooks_gpu.TOL)."""
    net, x = nets["all_avg"], logmel(16, 64, 64, seed=7)
    nm = _name_map(net, "gamma_flat", pool_rule)
    g, comp = _gpu(net), NameMapComposite(nm)
    R = compute_relevances(g, x.to(DEV), comp, class_idx=1)
    _, R64 = A.lrp(net, spec(nm), x, class_idx=1, mode="f64")
    _, Ra = A.lrp(net, spec(nm), x, class_idx=1, mode="analytic")
    e32, eref = f64_anchored_check(R.cpu(), Ra, R64)
    print(f"{pool_rule}: plan vs f64 median {np.median(e32):.3g} p75 {np.percentile(e32, 75):.3g}; "
          f"analytic vs f64 median {np.median(eref):.3g} p75 {np.percentile(eref, 75):.3g}")
    hooked = NameMapComposite(nm + [(["features.4"], Same())])
    assert isinstance(get_engine(g, hooked), HookedAutograd) and isinstance(get_engine(g, comp), LRPEngine)
    Rs = compute_relevances(g, x.to(DEV), hooked, class_idx=1)
    per = rel_l2(R.cpu(), Rs.cpu())
    print(f"{pool_rule}: plan vs HookedAutograd per-sample relative L2 {per}")
    assert per.max() <= 1e-3, per


def _gtzan_avg():
    torch.manual_seed(0)
    return VGGType(n_filters=(32, 32, 64, 64, 128), n_dense=128, pool_kernels=((2, 2),) * 5, dropout=0.4,
                   input_size=(128, 128), conv_bn=False, dense_bn=False, block_depth=1, pool="avg").eval()


def test_bf16_plan_vs_oracle():
    """test_bf16_gpu's whole-plan check on the all-avg GTZAN-128 net: logits within 1e-4, relevances within 5e-3
    relative L2 per sample of the oracle's mode "bf16"; the pool itself is fp32 in both."""
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN
    net = _gtzan_avg().bfloat16()
    x = logmel(3, seed=21).bfloat16()
    nm = LRP_NAME_MAP_GTZAN + [(A.pool_names(net), Norm(stabilizer=1e-6))]
    logits, Rref = A.lrp(copy.deepcopy(net).float(), spec(nm), x.float(), class_idx=6, mode="bf16")
    ng, comp = copy.deepcopy(net).to(DEV), NameMapComposite(nm)
    R = compute_relevances(ng, x.to(DEV), comp, class_idx=6).cpu()
    eng = get_engine(ng, comp)
    assert eng.precision == "bf16" and all(st.wts_fwd_bf is not None for st in eng.stages if st.cin > 1)
    lg = eng.forward(x.to(DEV)).cpu().double()
    np.testing.assert_allclose(lg, logits, rtol=1e-4, atol=1e-4 * float(logits.abs().max()))
    for b in range(R.size(0)):
        d = float((R[b].double() - Rref[b]).norm() / Rref[b].norm())
        assert d <= 5e-3, (b, d)


def test_pixelflipping_engine_forward_equals_torch_forward():
    """forward="engine" logits against forward="torch" (rtol = atol = 1e-4, test_pixelflipping_gpu), and a whole
    PixelFlipping call in both modes with Norm on the pools (the module's Pass on the activations needs it)."""
    from drsa_audio_amd.xai.pixelflipping import PixelFlipping
    net, x = A.toy_avg(("avg", "max", "avg", "avg", "avg"), last_k=(4, 4)), logmel(4, 64, 64, seed=70)
    pf = PixelFlipping(net, x, perturbation_size=16, num_classes=2, device=DEV, forward="engine")
    fe = pf._forward_func(None)
    pf.forward = "torch"
    ft = pf._forward_func(None)
    with torch.no_grad():
        np.testing.assert_allclose(fe(x.to(DEV)).cpu(), ft(x.to(DEV)).cpu(), rtol=1e-4, atol=1e-4)
    conf = {"convolutional": ("gamma", 0.25), "dense": ("epsilon", 1e-7), "first_layer": ("wsquare",),
            "name_map": [(A.pool_names(net), Norm(stabilizer=1e-6))]}
    out = {}
    for fw in ("torch", "engine"):
        pf = PixelFlipping(net, x, perturbation_size=16, num_classes=2, device=DEV, forward=fw)
        aupc, preds, _, heat = pf([conf], plot=False)
        name = pf._get_configuration_name(conf)
        out[fw] = (aupc[name], preds[name], heat[name].cpu())
    assert torch.equal(out["engine"][2], out["torch"][2]) and float(out["torch"][2].abs().max()) > 0
    np.testing.assert_allclose(out["engine"][0], out["torch"][0], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out["engine"][1], out["torch"][1], rtol=1e-4, atol=1e-4)
