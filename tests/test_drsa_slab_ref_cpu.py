"""tests/drsa_slab_ref.py (the float64 slab reference of the DRSA partial / finish kernels) against
the oracle's closed form and the library's own geometry (no GPU)."""
import numpy as np
import pytest

import drsa_ref
import drsa_slab_ref as sr
from gen_fixtures import drsa_inputs

# a padded, a phantom-concept (Kp = 8 > K = 5) and an odd-d problem
PROBLEMS = [(333, 100, 4), (333, 40, 5), (333, 42, 3)]


def _u0(d, seed):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0].astype(np.float32)


@pytest.mark.parametrize("N,d,K", PROBLEMS)
def test_slab_then_finish_is_the_closed_form(N, d, K):
    A, C = drsa_inputs(N, d, 50 + d)
    U0 = _u0(d, d + K)
    gs = sr.embed(*sr.slab(A, C, U0, K), d, K)
    f, G = sr.gradient(gs, N, d, K)
    f_ref, G_ref, r, _ = drsa_ref.closed_form(A, C, U0, K)
    assert abs(f - f_ref) <= 1e-12 * abs(f_ref)
    assert np.abs(G - G_ref).max() <= 1e-12 * np.abs(G_ref).max()
    f2, U_new = sr.finish(gs, N, U0, K)
    assert f2 == f
    assert np.abs(U_new - drsa_ref.polar(U0.astype(np.float64) + G_ref)).max() <= 1e-12
    np.testing.assert_allclose(sr.slab(A, C, U0, K)[1], (r * r).sum(0), rtol=1e-12)


@pytest.mark.parametrize("N,d,K", PROBLEMS)
@pytest.mark.parametrize("rounder", [drsa_ref.bf16_round, drsa_ref.f16_round])
def test_slab_then_finish_is_the_16bit_closed_form(N, d, K, rounder):
    A, C = drsa_inputs(N, d, 60 + d)
    Ab, Cb = rounder(A), rounder(C)
    U0 = _u0(d, d + K)
    gs = sr.embed(*sr.slab(Ab, Cb, U0, K, rounder=rounder), d, K)
    f, G = sr.gradient(gs, N, d, K)
    f_ref, G_ref = drsa_ref.closed_form_bf16(Ab, Cb, U0, K, rounder=rounder)
    assert abs(f - f_ref) <= 1e-12 * abs(f_ref)
    assert np.abs(G - G_ref).max() <= 1e-12 * np.abs(G_ref).max()
    # the rounding of U is in the reference: without it Gt moves by more than the kernels' 2e-5 gate
    Gt, _ = sr.slab(Ab, Cb, U0, K, rounder=rounder)
    Gt_plain, _ = sr.slab(Ab, Cb, U0, K)
    assert np.abs(Gt - Gt_plain).max() > 4 * 2e-5 * np.abs(Gt).max()


@pytest.mark.parametrize("d,K,DP,DKp", sr.GEOMETRIES)
def test_geometry_and_embedding(d, K, DP, DKp):
    from drsa_audio_amd import _capi
    dk, dkp, dp, Kp = sr.geom(d, K)
    assert (dk, dkp, dp, Kp) == (d // K, DKp, DP, DP // DKp)
    assert sr.slab_floats(d, K) == DP * DP + Kp == _capi.load().drsa_amd_drsa_slab_floats(d, K)
    # embed / unembed round trip; the padding mask is exactly what embed leaves at zero
    rng = np.random.default_rng(d * 131 + K)
    Gt, S = rng.standard_normal((d, d)) + 3.0, rng.random(K) + 1.0      # no zero among the real entries
    gs = sr.embed(Gt, S, d, K)
    Gt2, S2, pad = sr.unembed(gs, d, K)
    assert np.array_equal(Gt2, Gt) and np.array_equal(S2, S)
    assert gs.shape == pad.shape == (DP * DP + Kp,)
    assert np.array_equal(pad, gs == 0.0) and int((~pad).sum()) == d * d + K
    # spot checks of the layout as include/drsa_amd.h states it
    k, l, i = K - 1, dk - 1, d - 1
    assert gs[i * DP + k * DKp + l] == Gt[i, k * dk + l] and gs[DP * DP + k] == S[k]
    assert np.array_equal(sr.embed(Gt2, S2, d, K), gs)


@pytest.mark.parametrize("d,K,N", [(64, 4, 33003), (42, 3, 33003), (32, 4, 65603), (100, 4, 20603), (66, 2, 20603),
                                   (128, 16, 41003)])
def test_multitile_gates_see_one_missing_row_block(d, K, N):
    """The shapes of tests/test_drsa_multitile_gpu.py: the geometry is the library's, and the 2e-5
    gates are tight for them.  One 16-row block left out of N rows (a tile loop that ends one block
    early in a single leaf) moves the float64 Gt by at least ten times the gate."""
    from drsa_audio_amd import _capi
    assert sr.slab_floats(d, K) == _capi.load().drsa_amd_drsa_slab_floats(d, K)
    A, C = drsa_inputs(N, d, 9000 + 31 * d + K)
    U0 = sr.u0(d, d + K)
    Gt, _ = sr.slab(A, C, U0, K)
    rb = (N + 15) // 16 // 256 - 1                      # the last row block of leaf 0
    keep = np.ones(N, dtype=bool)
    keep[16 * rb:16 * rb + 16] = False
    Gt_short, _ = sr.slab(A[keep], C[keep], U0, K)
    assert np.abs(Gt_short - Gt).max() > 10 * 2e-5 * np.abs(Gt).max()


@pytest.mark.parametrize("d,K", [(99, 9), (130, 2), (129, 1), (100, 1), (0, 1), (64, 0), (64, 3), (-4, 2)])
def test_geom_rejects_what_the_library_rejects(d, K):
    from drsa_audio_amd import _capi
    assert _capi.load().drsa_amd_drsa_slab_floats(d, K) == 0
    with pytest.raises(ValueError):
        sr.geom(d, K)
