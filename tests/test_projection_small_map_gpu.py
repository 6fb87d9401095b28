"""ProjectionModel on a map smaller than the projection kernels tile (GPU): the toy net's last conv
block has a 4 x 4 map, which the plan runs zero-padded to 8 x 8 and crops (plan._proj_hw).  Under
the toy net's own composite (an Epsilon head, so nothing but the padding is new) every element
equals the oracle's mode="exact", as at the layers the kernels take as they are (layer 10: 8 x 8)."""
import copy

import numpy as np
import pytest
import torch

import lrp_ref
from lrp_common import logmel, ortho, spec, toy
from drsa_audio_amd.engine.plan import _proj_hw
from drsa_audio_amd.model.modify_model import ProjectionModel
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("layer_idx,hw", [(13, (4, 4)), (10, (8, 8))])
def test_toy_projection_small_map(layer_idx, hw):
    assert (_proj_hw(*hw) != hw) == (layer_idx == 13)
    net = toy()
    U, x = ortho(16, 1), logmel(3, 64, 64, seed=5)
    hg = HeatmapGenerator(copy.deepcopy(net).to(DEV), U, LRP_NAME_MAP_TOY, "class2", num_concepts=4,
                          layer_idx=layer_idx)
    pm = ProjectionModel(net, layer_idx, U, 4, case="toy").eval()
    ref = lrp_ref.subspace_heatmaps(pm, spec(LRP_NAME_MAP_TOY), 4, x, class_idx=hg.class_idx, mode="exact")
    hg.generate_subspace_heatmaps(x)
    for k in ("standard_heatmaps", "subspace_heatmaps", "mask"):
        assert np.array_equal(hg.info[k], ref[k]), k
    assert np.isfinite(ref["subspace_heatmaps"]).all() and np.abs(ref["subspace_heatmaps"]).max() > 0
