"""DRSA partial kernels on leaves of two and three staged tiles (GPU).

The row partition is a fixed 256 leaves; a leaf is staged RT rows at a time (RT = 128 at padded size
DP <= 64, 80 at DP = 128), so it needs a second tile only above 256 RT rows: N > 32768 resp. 20480.
Below that the steady state of partial_core (prefetch tile t + 1, compute tile t, barrier, store,
barrier), the accumulation of one leaf's Gt over tiles, and the first arm of "this leaf's next tile,
else the next leaf's first" in drsa_partial_grouped_kernel never run.  The row counts here are the
smallest that reach them, none a multiple of 16, each just over a threshold: most leaves have one
tile and a few two (33003 rows = 2063 row blocks: 241 leaves of 8, 15 of 9; 20603 rows = 1288 row
blocks: 248 leaves of 5, 8 of 6), or most have two and a few three (65603 rows = 4101 row blocks:
251 leaves of 16, 5 of 17; 41003 rows = 2563 row blocks: 253 leaves of 10, 3 of 11).

* the partial entry points against the float64 slab (drsa_slab_ref.check_slab: 2e-5 on Gt and S,
  padding exactly 0).  A plain float32 numpy evaluation of the same formula sits within 4e-7 max|Gt|
  and 8e-6 relative on S of float64 on these inputs, so the gates hold for the reference alone;
* drsa_step against drsa_slab_ref.finish (gates of test_padded_step_matches_closed_form);
* drsa_run_batched == drsa_run bit for bit with problems of different N in one launch, so that
  leaves of one, two and three tiles follow each other inside a workgroup.
"""
import functools

import numpy as np
import pytest
import torch

import drsa_slab_ref as sr
from gen_fixtures import drsa_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")

#           d,   K,   N,     dtypes                       tiles per leaf
PARTIAL = [(64, 4, 33003, ("fp32", "bf16", "f16")),     # 1 and 2
           (42, 3, 33003, ("fp32", "bf16")),            # 1 and 2, scalar staging
           (32, 4, 65603, ("fp32",)),                   # 2 and 3
           (100, 4, 20603, ("fp32", "bf16", "f16")),    # 1 and 2 at DP = 128
           (66, 2, 20603, ("fp32", "f16")),             # 1 and 2 at DP = 128, scalar staging, width 64
           (128, 16, 41003, ("fp32", "bf16"))]          # 2 and 3 at DP = 128


@functools.lru_cache(maxsize=None)
def _inputs(N, d, K):
    A, C = drsa_inputs(N, d, 9000 + 31 * d + K)
    return A, C, sr.u0(d, d + K)


@functools.lru_cache(maxsize=None)
def _slab(N, d, K, dt):
    """(A, C) holding values of type dt and the float64 slab of them, computed once."""
    A, C, U0 = _inputs(N, d, K)
    rnd = sr.ROUNDER[dt]
    if rnd is not None:
        A, C = rnd(A), rnd(C)
    return (A, C) + sr.slab(A, C, U0, K, rounder=rnd)


def test_tile_counts():
    """The row counts reach what the docstring says (RT / 16 row blocks per tile)."""
    def tiles(N, d, K):
        rt = 8 if sr.geom(d, K)[2] <= 64 else 5
        R = (N + 15) // 16
        L = min(256, R)
        return sorted({-(-(((l + 1) * R) // L - (l * R) // L) // rt) for l in range(L)})
    assert all(N % 16 for _, _, N, _ in PARTIAL)
    assert [tiles(N, d, K) for d, K, N, _ in PARTIAL] == [[1, 2], [1, 2], [2, 3], [1, 2], [1, 2], [2, 3]]
    assert tiles(32803, 32, 4) == [1, 2] and tiles(300, 32, 4) == [1] and tiles(500, 66, 2) == [1]
    assert tiles(41003, 100, 4) == [2, 3]
    assert sr.geom(42, 3)[1:3] == (16, 64) and tiles(32803, 42, 3) == [1, 2] and tiles(300, 42, 3) == [1]


@pytest.mark.parametrize("d,K,N,dt", [(d, K, N, dt) for d, K, N, dts in PARTIAL for dt in dts])
def test_multitile_partial_slab_matches_reference(d, K, N, dt):
    A, C, Gt, S = _slab(N, d, K, dt)
    rc, gs = sr.partial_rc(dt, A, C, _inputs(N, d, K)[2], K)
    assert rc == 0, rc
    sr.check_slab(gs, Gt, S, d, K, tag=f"multitile {dt} N={N}")


@pytest.mark.parametrize("N,d,K", [(33003, 64, 4), (20603, 100, 4), (41003, 128, 16)])
def test_multitile_step_matches_reference_finish(N, d, K):
    from drsa_audio_amd.xai.drsa.drsa import drsa_step
    A, C, U0 = _inputs(N, d, K)
    _, _, Gt, S = _slab(N, d, K, "fp32")
    f_ref, U_ref = sr.finish(sr.embed(Gt, S, d, K), N, U0, K)
    Ag, Cg, Ug = (torch.from_numpy(v).to(DEV) for v in (A, C, U0))
    Un, f = drsa_step(Ag, Cg, Ug, K)
    torch.cuda.synchronize()
    Un = Un.cpu().numpy().astype(np.float64)
    dev_f, dev_u = abs(float(f) - f_ref) / abs(f_ref), np.abs(Un - U_ref).max()
    dev_o = np.abs(Un.T @ Un - np.eye(d)).max()
    print(f"\nDRSA-STEP N={N} d={d} K={K}: f dev {dev_f:.3e} (gate 1e-5), U dev {dev_u:.3e} (gate 2e-5), "
          f"orthogonality {dev_o:.3e} (gate 2e-6)")
    assert dev_f <= 1e-5
    assert dev_u < 2e-5
    assert dev_o < 2e-6


BATCHED = {"grouped": [(32803, 32, 4), (300, 32, 4)],          # drsa_partial_grouped_kernel: 1-2 tiles | 1
           "grouped128": [(20603, 100, 4), (41003, 100, 4)],   # the same at DP = 128: 1-2 tiles | 2-3
           # the grouped kernel with scalar staging (d % 4 != 0; DP = 64, DKp = 16): 1-2 tiles | 19 one-block
           # leaves in 3 groups, the last leaf 12 rows
           "grouped_scalar": [(32803, 42, 3), (300, 42, 3)],
           "leafwise": [(20603, 66, 2), (500, 66, 2)]}         # drsa_partial_leaf_batched_kernel, scalar staging


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("kind", sorted(BATCHED))
def test_multitile_batched_equals_run_bitwise(kind, blocks):
    from drsa_audio_amd.xai.drsa.drsa import drsa_run, drsa_run_batched
    steps = 2
    probs = []
    for N, d, K in BATCHED[kind]:
        A, C, U0 = _inputs(N, d, K)
        probs.append(tuple(torch.from_numpy(v).to(DEV) for v in (A, C, U0)) + (K,))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        batched = drsa_run_batched(probs, steps, blocks=blocks)
        alone = [drsa_run(*p, steps) for p in probs]
    torch.cuda.synchronize()
    for (Ub, tb), (Ua, ta) in zip(batched, alone):
        assert torch.isfinite(tb).all() and torch.isfinite(Ub).all()
        assert torch.equal(tb, ta), (tb, ta)
        assert torch.equal(Ub, Ua)
