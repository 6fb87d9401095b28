"""proj_ref (the float64 oracle of the projection kernels) against what the repository already
trusts, so that a wrong oracle cannot hide a wrong kernel: ProjectionModel's own layers in float64,
lrp_ref.subspace_mask and the SubspaceHook pins of lrp_pins_fixture.npz, torch's max_pool2d on
planted ties, and the residual kernel's arithmetic restated in numpy against the residual bound."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import lrp_ref
import proj_ref as R
from drsa_audio_amd.model.modify_model import ProjectionModel


def _ortho(d, seed):
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0]
    return torch.from_numpy(q.astype(np.float32))


@pytest.fixture(scope="module")
def pins(golden_dir):
    return np.load(f"{golden_dir}/lrp_pins_fixture.npz")


def test_forward_equals_projection_model():
    d, K, B, S = 16, 4, 2, 8
    U = _ortho(d, 1)
    trunk = nn.Module()
    trunk.features = nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity())
    trunk.classifier = nn.Sequential()
    pm = ProjectionModel(trunk, 1, U, K, num_flat_features=d * S * S).double()
    a = torch.randn(B, d, S, S, generator=torch.Generator().manual_seed(2)).clamp_min(0)
    h, ap, pooled, amax = R.forward(a, U, pool=True)
    h_pm = pm.features.projection(a.double())                       # [B, n, K, d_k]
    ap_pm = pm.features(a.double())                                 # a' = (a U) U^T
    assert h_pm.shape == (B, S * S, K, d // K) and ap_pm.shape == a.shape
    h_pm = h_pm.reshape(B, S * S, d).transpose(1, 2).reshape(B, d, S, S)
    # float64 against float64 in another summation order: d terms of size <= |a| |U|
    assert (h - h_pm).abs().max() <= d * 2.0 ** -52 * (R.h_bound(a, U) / R.GATE).max()
    assert (ap - ap_pm).abs().max() <= 2 * d * 2.0 ** -52 * a.abs().max()
    p_t, i_t = torch.nn.functional.max_pool2d(ap, 2, return_indices=True)
    assert torch.equal(pooled, p_t)
    assert torch.equal(amax.long(), 2 * ((i_t // S) % 2) + (i_t % S) % 2)


@pytest.mark.parametrize("d", [1, 5, 16, 32, 100, 128])
def test_residual(d):
    U = _ortho(d, 40 + d)
    P64 = R.residual(U)
    assert torch.equal(P64, P64.T)
    plain = U.double() @ U.double().T - torch.eye(d, dtype=torch.float64)
    assert (P64 - plain).abs().max() <= d * 2.0 ** -52
    assert torch.count_nonzero(R.residual(torch.eye(d))) == 0
    # the kernel's arithmetic, restated, stays within the bound the GPU test applies to the kernel
    Pk = R.residual_chain_model(U)
    ratio = R.worst_ratio((Pk.double() - P64).abs(), R.residual_bound(U, P64))
    print(f"d={d} chain model / bound = {ratio:.3f}")
    assert ratio <= 1.0 and torch.equal(Pk, Pk.T)


def test_clone_mask_equals_reference_hook(pins):
    """U = I, a = 1, zero stabilisers, no den: G is the masked relevance, exactly."""
    for tag in ("k4", "k2", "k8", "k5"):
        g, ref = pins[f"hook_{tag}_in"], pins[f"hook_{tag}_out"]
        Bq, n, K, dk = g.shape
        D, H, W = K * dk, 8, 8
        gp = torch.from_numpy(g).reshape(Bq, n, D).transpose(1, 2).reshape(Bq, D, H, W)
        a = torch.ones(Bq, D, H, W)
        G, E = R.backward(gp, None, a, a, a, None, torch.eye(D), K, 0.0, 0.0, 0)
        got = G.reshape(Bq, D, n).transpose(1, 2).reshape(Bq, n, K, dk)
        assert np.array_equal(got.numpy(), ref), tag
        assert np.array_equal(lrp_ref.subspace_mask(torch.from_numpy(g), K).numpy(), ref), tag
        assert torch.isfinite(E).all() and (E >= 0).all()


@pytest.mark.parametrize("K,dk", [(4, 4), (1, 5), (5, 1), (3, 8)])
def test_fanout_rows_equal_subspace_mask(K, dk):
    """fanout 1 writes the K + 1 clones of each sample, fanout 2 drops clone 0, fanout 0 maps row b
    to clone b % (K + 1): all three against lrp_ref.subspace_mask on a replicated batch."""
    B, D, H, W = K + 2, K * dk, 2, 4
    n = H * W
    gp = torch.randint(-64, 65, (B, D, H, W), generator=torch.Generator().manual_seed(K + dk)).float()
    a = torch.ones(B, D, H, W)
    rows = gp.reshape(B, D, n).transpose(1, 2).reshape(B, n, K, dk)
    ref = lrp_ref.subspace_mask(rows.repeat_interleave(K + 1, 0), K)            # [B (K+1), n, K, dk]
    ref = ref.reshape(B, K + 1, n, D).transpose(2, 3).reshape(B, K + 1, D, H, W).double()
    G1, _ = R.backward(gp, None, a, a, a, None, torch.eye(D), K, 0.0, 0.0, 1)
    assert torch.equal(G1.reshape(B, K + 1, D, H, W), ref)
    G2, _ = R.backward(gp, None, a, a, a, None, torch.eye(D), K, 0.0, 0.0, 2)
    assert torch.equal(G2.reshape(B, K, D, H, W), ref[:, 1:])
    G0, _ = R.backward(gp, None, a, a, a, None, torch.eye(D), K, 0.0, 0.0, 0)
    assert torch.equal(G0, torch.stack([ref[b, b % (K + 1)] for b in range(B)]))
    assert [q for _, q in R.output_clones(B, K, 0)] == list(range(K + 1)) + [0]


def test_pool_tie_rule_equals_torch():
    a, want = R.tie_map()
    pooled, amax = R.max_pool(a.double())
    p_t, i_t = torch.nn.functional.max_pool2d(a.double(), 2, return_indices=True)
    assert torch.equal(pooled, p_t)
    assert torch.equal(amax.long(), 2 * ((i_t // 8) % 2) + (i_t % 8) % 2)
    assert torch.equal(amax.long()[want >= 0], want[want >= 0])
    # a NaN is the maximum, the first one wins
    a[0, 9, 0, 1] = float("nan")
    a[0, 9, 1, 1] = float("nan")
    pooled, amax = R.max_pool(a.double())
    assert torch.isnan(pooled[0, 9, 0, 0]) and amax[0, 9, 0, 0] == 1


def test_unpool_inverts_pool():
    a, _ = R.tie_map()
    pooled, amax = R.max_pool(a)
    up = R.unpool(pooled, amax)
    assert torch.equal(torch.nn.functional.max_pool2d(up, 2), pooled)
    assert torch.count_nonzero(up) == torch.count_nonzero(pooled)


def test_backward_bound_covers_float32_evaluation():
    """The chain evaluated in torch float32 (another order than the kernel's, the same roundings) stays
    within the propagated bound of the float64 result; dead channels and zero denominators included."""
    D, K, B, H, W = 24, 3, 2, 4, 8
    g = torch.Generator().manual_seed(9)
    U = _ortho(D, 3)
    a = torch.randn(B, D, H, W, generator=g).clamp_min(0)
    P = R.residual(U).float()
    h = torch.einsum("cj,bchw->bjhw", U, a)
    ap = a + torch.einsum("ck,bkhw->bchw", P, a)
    pooled, amax = R.max_pool(ap)
    gp = torch.randn(B, D, H // 2, W // 2, generator=g)
    den = torch.randn(B, D, H, W, generator=g) * 2
    den.view(-1)[::7] = 0.0
    e1, e2 = torch.tensor(1e-6), torch.tensor(1e-7)
    st = lambda t, e: t + torch.where(t >= 0, e, -e)
    g1 = R.unpool(gp, amax) / st(ap, e1)
    g2 = h * torch.einsum("cj,bchw->bjhw", U, g1) / st(h, e1)
    G64, E = R.backward(gp, amax, ap, h, a, den, U, K, 1e-6, 1e-7, 1)
    assert G64.shape == (B * (K + 1), D, H, W)
    worst = 0.0
    for row, (b, q) in enumerate(R.output_clones(B, K, 1)):
        j0, j1 = R.clone_columns(q, D, K)
        v = torch.einsum("cj,jhw->chw", U[:, j0:j1], g2[b, j0:j1])
        G = torch.where(a[b] > 0, a[b] * v / st(den[b], e2), torch.zeros_like(v))
        worst = max(worst, R.worst_ratio((G.double() - G64[row]).abs(), E[row]))
    print(f"float32 evaluation / bound = {worst:.3e}")
    assert worst <= 1.0
