"""drsa_amd_heatmap_sort with std_from_sum = 1 (the engine's default standard="sum": the standard map
is the K concept maps summed, k ascending) against numpy float32, bit for bit -- numpy is the
reference here (tests/test_pins_cpu.py::test_numpy_pairwise_restatement, and the pins of
lrp_pins_fixture.npz, which all use std_from_sum = 0).  Shapes: the cached kernel (128 x 128, K = 4);
the generic kernel with balanced sums (64 x 64; 128 x 256: four 8192-element chunks), with the
serial-walk sums (20 x 20, 36 x 52, 6 x 6) and a single leaf (8 x 8); K = 1, 3, 16 and 64 (the limit
of the kernel's sums / order arrays)."""
import numpy as np
import pytest
import torch

from drsa_audio_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(2, 4, 128, 128), (2, 4, 64, 64), (2, 3, 20, 20), (2, 1, 8, 8), (1, 64, 6, 6), (2, 16, 36, 52),
         (2, 4, 128, 256)]


def concept_maps(B, K, H, W, seed):
    """[B, K, H, W] concept heatmaps shaped like gen_fixtures.sort_inputs: signed, heavy-tailed."""
    rng = np.random.default_rng(9000 + seed)
    return (rng.standard_normal((B, K, H, W)) * np.exp(rng.standard_normal((B, K, 1, 1)))).astype(np.float32)


def sort_gpu(hm: np.ndarray, K: int, std_from_sum: int):
    """(std, std_rel, sub, rel, mask) as numpy; every output pre-filled with NaN / -1."""
    H, W = hm.shape[-2:]
    B = hm.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(hm)).to(DEV)
    std = torch.full((B, H, W), float("nan"), device=DEV)
    std_rel = torch.full((B,), float("nan"), device=DEV)
    sub = torch.full((B, K, H, W), float("nan"), device=DEV)
    rel = torch.full((B, K), float("nan"), device=DEV)
    mask = torch.full((B, K), -1, dtype=torch.int64, device=DEV)
    _capi.call("drsa_amd_heatmap_sort", t.data_ptr(), B, K, H * W, std_from_sum, std.data_ptr(), std_rel.data_ptr(),
               sub.data_ptr(), rel.data_ptr(), mask.data_ptr(), _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (std, std_rel, sub, rel, mask))


def sort_numpy(hm: np.ndarray, kind=None):
    B, K = hm.shape[:2]
    std = hm[:, 0].copy()
    for k in range(1, K):                                   # the float32 left fold, k ascending
        std = std + hm[:, k]
    assert std.dtype == np.float32
    std_rel = std.reshape(B, -1).sum(-1)
    rel = hm.sum(axis=(-2, -1))
    mask = np.argsort(rel, axis=-1, kind=kind)[..., ::-1]
    ar = np.arange(B)[:, None]
    return std, std_rel, hm[ar, mask], rel[ar, mask], mask


def check(hm, kind=None):
    B, K = hm.shape[:2]
    got = sort_gpu(hm, K, 1)
    ref = sort_numpy(hm, kind)
    for name, g, r in zip(("std", "std_rel", "sub", "rel", "mask"), got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype, name
        assert np.array_equal(g, r), name                   # bitwise: no NaN is left, none is expected
    # std_from_sum = 0 on the same maps with the summed map prepended as clone 0
    got0 = sort_gpu(np.concatenate([ref[0][:, None], hm], axis=1), K, 0)
    for name, g, g0 in zip(("std", "std_rel", "sub", "rel", "mask"), got, got0):
        assert np.array_equal(g, g0), name
    return ref


@pytest.mark.parametrize("B,K,H,W", CASES)
def test_sum_mode_equals_numpy(B, K, H, W):
    hm = concept_maps(B, K, H, W, K + H + W)
    ref = check(hm)
    assert all(len(np.unique(r)) == K for r in ref[3])      # no ties: any argsort kind gives this order
    # the fold is not the pairwise or the float64 sum: the check above tells them apart
    if K > 2:
        assert not np.array_equal(ref[0], hm.sum(axis=1, dtype=np.float64).astype(np.float32))


@pytest.mark.parametrize("H,W", [(128, 128), (64, 64)])
def test_sum_mode_ties(H, W):
    """An all-zero sample (every concept ties) and a sample with two identical maps: numpy's stable
    ascending order reversed, i.e. the larger index first."""
    hm = concept_maps(3, 4, H, W, H)
    hm[1] = 0.0
    hm[2, 3] = hm[2, 1]
    ref = check(hm, kind="stable")
    assert ref[4][1].tolist() == [3, 2, 1, 0]
    m2 = ref[4][2].tolist()
    assert m2.index(3) + 1 == m2.index(1)
