"""The engine at input sizes whose maps are not powers of two, against lrp_ref mode "exact", bit for
bit (GPU).

GTZAN-type net at 96 x 192: maps 96x192, 48x96, 24x48, 12x24, 6x12 -- the 96- and 48-wide maps on
32- and 16-wide tiles, 12- and 6-row partial tiles on the 8 x 8 / 4 x 8 families, the first layer's
denominator ring at 48 x 96, and the projection kernels on zero-padded 24 x 48 and 12 x 24 maps.
(96 x 96 is not served: its last map, 6 x 6, has a width the rule backward's float4 rows cannot
cross; 96 x 192 is the nearest size that keeps the 48-wide map and the 6-row tile.)  VGGish-BN at
96 x 128: maps 96x128, 48x32, 24x16, 12x8, 6x4 behind the (2,4) pool.  Batch 2, plus one sample of
a batch of 256, where every layer's grid reaches 512 workgroups and the 8 x 8 kernels replace their
4 x 8 stand-ins.  A size with a map the rule backward cannot cross (6 x 10, 6 x 6) is refused by
forward().
"""
import copy

import numpy as np
import pytest
import torch

import lrp_ref
from lrp_common import logmel, ortho, spec, u64, vggish
from drsa_audio_amd._capi import DrsaAmdError
from drsa_audio_amd.model.create_model import VGGType
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_VGGISH
from drsa_audio_amd.xai.explain.attribute import compute_relevances
from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.rules import Epsilon, Gamma

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# test_lrp_gpu.py's test_rule_variants_bit_exact: Gamma on the (negative-valued) input layer
GAMMA_FIRST = [(["features.0"], Gamma(gamma=0.3, stabilizer=1e-6)), (["features.3"], Epsilon(epsilon=1e-5)),
               (["features.9"], Gamma(gamma=0.1, stabilizer=1e-7)), (["classifier.0"], Epsilon(epsilon=1e-6)),
               (["classifier.6"], Epsilon(epsilon=1e-6))]


def _gtzan(size, seed=0):
    torch.manual_seed(seed)
    return VGGType(n_filters=(32, 32, 64, 64, 128), n_dense=128, pool_kernels=((2, 2),) * 5, dropout=0.4,
                   input_size=size, conv_bn=False, dense_bn=False, block_depth=1).eval()


@pytest.fixture(scope="module")
def net96():
    return _gtzan((96, 192))


@pytest.mark.parametrize("name_map", [LRP_NAME_MAP_GTZAN, GAMMA_FIRST], ids=["gtzan_map", "gamma_first"])
def test_gtzan96x192_standard_lrp_bit_exact(net96, name_map):
    x = logmel(2, 96, 192, seed=3)
    _, R = lrp_ref.lrp(net96, spec(name_map), x, class_idx=3, mode="exact")
    Rg = compute_relevances(copy.deepcopy(net96).to(DEV), x.to(DEV), NameMapComposite(name_map), class_idx=3)
    assert Rg.shape == x.shape and torch.equal(Rg.cpu(), R)


@pytest.mark.parametrize("layer_idx", [7, 10])
def test_gtzan96x192_heatmap_generator_bit_exact(net96, layer_idx):
    U = u64() if layer_idx == 7 else ortho(64, 3)
    x = logmel(2, 96, 192, seed=5 + layer_idx)
    pm = ProjectionModel(net96, layer_idx, U, 4).eval()
    ref = lrp_ref.subspace_heatmaps(pm, spec(LRP_NAME_MAP_GTZAN), 4, x, class_idx=4, mode="exact")
    hg = HeatmapGenerator(copy.deepcopy(net96).to(DEV), U, LRP_NAME_MAP_GTZAN, "reggae", num_concepts=4,
                          layer_idx=layer_idx, device="cuda")
    hg.generate_subspace_heatmaps(x)
    for k in ("standard_heatmaps", "standard_relevance", "subspace_heatmaps", "subspace_relevances", "mask"):
        assert np.array_equal(hg.info[k], ref[k]), k


def test_gtzan96x192_one_sample_of_a_large_batch(net96):
    """At B = 256 even the 6 x 12 map (two 8 x 8 tiles) has 512 workgroups, so no layer runs on
    4 x 8 tiles; a sample of that batch equals the oracle run on it alone."""
    x = logmel(256, 96, 192, seed=9)
    k = 201
    _, R = lrp_ref.lrp(net96, spec(LRP_NAME_MAP_GTZAN), x[k:k + 1], class_idx=6, mode="exact")
    Rg = compute_relevances(copy.deepcopy(net96).to(DEV), x.to(DEV), NameMapComposite(LRP_NAME_MAP_GTZAN), class_idx=6)
    assert torch.equal(Rg[k:k + 1].cpu(), R)


@pytest.fixture(scope="module")
def vgg96():
    return vggish(input_size=(96, 128))


def test_vggish_96x128_standard_lrp_bit_exact(vgg96):
    x = logmel(2, 96, 128, seed=3)
    _, R = lrp_ref.lrp(lrp_ref.merge_batch_norm(vgg96), spec(LRP_NAME_MAP_VGGISH), x, class_idx=4, mode="exact")
    comp = NameMapComposite(LRP_NAME_MAP_VGGISH, canonizers=[SequentialMergeBatchNorm()])
    Rg = compute_relevances(copy.deepcopy(vgg96).to(DEV), x.to(DEV), comp, class_idx=4)
    assert torch.equal(Rg.cpu(), R)


def test_vggish_96x128_drsa_capture_bit_exact(vgg96):
    from drsa_audio_amd.xai.drsa.preprocessing import get_intermediate
    x = logmel(2, 96, 128, seed=26)
    _, _, (act, rel) = lrp_ref.lrp(lrp_ref.merge_batch_norm(vgg96), spec(LRP_NAME_MAP_VGGISH), x, class_idx=1,
                                   mode="exact", capture="features.26")
    comp = NameMapComposite(LRP_NAME_MAP_VGGISH, canonizers=[SequentialMergeBatchNorm()])
    a, r = get_intermediate(copy.deepcopy(vgg96).to(DEV), x.to(DEV), comp, 26, 1)
    assert tuple(a.shape[-2:]) == (12, 8)
    assert torch.equal(a.cpu(), act) and torch.equal(r.cpu(), rel)


@pytest.mark.parametrize("size,last", [((96, 160), "6x10"), ((96, 96), "6x6")])
def test_unsupported_size_is_refused_with_layer_and_size(size, last):
    """96 x 160: maps 96x160 ... 6x10 (96 x 96: ... 6x6).  The pooled forward would take the last
    map, the rule backward (float4 rows, W % 4 == 0) cannot: one clean error that names the layer
    and the size, and no result."""
    net = _gtzan(size).to(DEV)
    x = logmel(2, *size, seed=1).to(DEV)
    with pytest.raises((ValueError, DrsaAmdError), match=rf"features\.12.*{last}"):
        compute_relevances(net, x, NameMapComposite(LRP_NAME_MAP_GTZAN), class_idx=0)
