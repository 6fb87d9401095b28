"""Every instantiated DRSA partial kernel against the float64 slab reference (GPU).

drsa_step.hip's dispatch instantiates drsa_partial_kernel per padded size DP x padded concept width
DKp x A/C type (fp32, bf16, fp16) x staging (float4 rows when d % 4 == 0, scalar otherwise).  Each
geometry of drsa_slab_ref.GEOMETRIES reaches one (DP, DKp) pair: exact powers of two, padded problems
(zero columns inside every concept block, zero rows, phantom concepts) and d % 4 != 0.  The entry
points are called directly with gs of exactly drsa_amd_drsa_slab_floats(d, K) floats, pre-filled
with NaN, and the whole slab is compared in padded coordinates (drsa_slab_ref.check_slab):

* real Gt entries  |Gk - Gt|.max() <= 2e-5 |Gt|.max()
* real S           rtol 2e-5, atol 1e-6 S.max()
* every padding entry and every phantom S slot == 0.0 exactly

N = 333 is 21 leaves of one 16-row block each, the last holding 13 rows; N = 17 is two leaves, the
second holding one row.  16-bit A, C are rounded on the host and the reference rounds U the same way,
so the gates are those of fp32 (leaving the U rounding out moves Gt by ~2e-3).

drsa_amd_drsa_finish is then fed slabs built by the reference alone (never by the partial kernel).
"""
import functools

import numpy as np
import pytest
import torch

import drsa_slab_ref as sr
from gen_fixtures import drsa_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N_MAIN, N_TINY = 333, 17
GEOM16 = [g for g in sr.GEOMETRIES if g[2] >= 32]                     # the 16-bit kernels: DP >= 32
TINY = [(12, 3, 16, 4), (18, 2, 32, 16), (40, 5, 64, 8), (100, 4, 128, 32)]   # one geometry per DP


@functools.lru_cache(maxsize=None)
def _problem(N, d, K, dt):
    """(A, C, U0, Gt, S): inputs holding values of type dt, and their float64 slab."""
    A, C = drsa_inputs(N, d, 7000 + 31 * d + K)
    rnd = sr.ROUNDER[dt]
    if rnd is not None:
        A, C = rnd(A), rnd(C)
    U0 = sr.u0(d, d + K)
    Gt, S = sr.slab(A, C, U0, K, rounder=rnd)
    return A, C, U0, Gt, S


def _run_and_check(N, d, K, dt):
    A, C, U0, Gt, S = _problem(N, d, K, dt)
    rc, gs = sr.partial_rc(dt, A, C, U0, K)
    assert rc == 0, rc
    return sr.check_slab(gs, Gt, S, d, K, tag=f"partial {dt} N={N}")


@pytest.mark.parametrize("d,K,DP,DKp", sr.GEOMETRIES)
def test_partial_fp32_slab_matches_reference(d, K, DP, DKp):
    _run_and_check(N_MAIN, d, K, "fp32")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("d,K,DP,DKp", GEOM16)
def test_partial_16bit_slab_matches_reference(d, K, DP, DKp, dt):
    _run_and_check(N_MAIN, d, K, dt)


@pytest.mark.parametrize("d,K,DP,DKp,dt", [g + (dt,) for g in TINY for dt in ("fp32", "bf16", "f16")
                                            if dt == "fp32" or g[2] >= 32])
def test_partial_two_leaves_one_row_in_the_last(d, K, DP, DKp, dt):
    _run_and_check(N_TINY, d, K, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_16bit_at_dp16_is_unsupported(dt):
    """The 16-bit MFMA tiles are 32 deep: at DP = 16 the 16-bit entry points return
    DRSA_EUNSUPPORTED, say why, and leave gs alone."""
    from drsa_audio_amd import _capi
    d, K = 12, 3
    A, C, U0, _, _ = _problem(N_MAIN, d, K, dt)
    rc, gs = sr.partial_rc(dt, A, C, U0, K, poison=-7.0)
    assert rc == _capi.DRSA_EUNSUPPORTED
    assert b"unsupported d=12 K=3" in _capi.lib().drsa_amd_last_error()
    assert (gs == -7.0).all()


# ---------------------------------------------------------------------------------------------
# drsa_amd_drsa_finish on a slab the reference built
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(100, 4), (42, 3), (40, 5), (66, 2), (16, 16), (128, 2)])
def test_finish_on_reference_built_slab(d, K):
    """gs = float32(embed(slab)) -> drsa_amd_drsa_finish; the reference finish evaluates the same
    float32 slab.  The kernel forms f in double from the fp32 sums (only the final float cast
    differs: 1e-6 relative), U_out = polar(U + Gt diag(c)) within 2e-5, orthogonal to 2e-6."""
    from drsa_audio_amd import _capi
    N = N_MAIN
    A, C, U0, Gt, S = _problem(N, d, K, "fp32")
    gs32 = sr.embed(Gt, S, d, K).astype(np.float32)
    f_ref, U_ref = sr.finish(gs32.astype(np.float64), N, U0, K)
    gs = torch.from_numpy(gs32).to(DEV)
    U = torch.from_numpy(U0).to(DEV)
    U_out = torch.full_like(U, float("nan"))
    f = torch.full((1,), float("nan"), device=DEV)
    _capi.call("drsa_amd_drsa_finish", gs.data_ptr(), N, d, K, U.data_ptr(), U_out.data_ptr(), f.data_ptr(), 0, None,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    f, Un = float(f), U_out.cpu().numpy().astype(np.float64)
    dev_f, dev_u = abs(f - f_ref) / abs(f_ref), np.abs(Un - U_ref).max()
    dev_o = np.abs(Un.T @ Un - np.eye(d)).max()
    print(f"\nDRSA-FINISH d={d} K={K}: f dev {dev_f:.3e} (gate 1e-6), U dev {dev_u:.3e} (gate 2e-5), "
          f"orthogonality {dev_o:.3e} (gate 2e-6)")
    assert dev_f <= 1e-6
    assert dev_u < 2e-5
    assert dev_o < 2e-6
