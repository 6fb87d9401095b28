"""The natural DRSA geometry (drsa_amd_drsa_any_*) for the tests: slab layout, float64 references
and the shapes of tests/test_drsa_any_{cpu,gpu}.py (test infrastructure).

    DP = next power of two >= max(16, d)
    gs[i * DP + j] = Gt[i][j]   i, j < d        (concept k owns the real columns [k dk, (k + 1) dk))
    gs[DP * DP + k] = S[k]      k < K
    every other entry 0.0; DP * DP + K floats

Gt and S are drsa_slab_ref.slab's (geometry-free).
"""
import functools

import numpy as np

import drsa_ref
import drsa_slab_ref as sr
from gen_fixtures import drsa_inputs

# (d, K, N) of the partial test.  Natural-only shapes (the padded geometry refuses them) but the
# last, which both geometries take.  (99, 9) takes the scalar staging (d % 4 != 0); N = 20603 is
# 1288 row blocks over 256 leaves (5 or 6 blocks each, the last block holding 11 rows); N = 4099 is
# 257 blocks (one leaf with two), the last holding 3 rows; N = 333 is 21 one-block leaves; N = 17 is
# two leaves, the second holding one row; N = 1 a single row.
PARTIAL_SHAPES = [(100, 5, 20603), (100, 10, 4099), (100, 20, 4099), (99, 9, 20603), (128, 1, 20603),
                  (100, 1, 4099), (120, 3, 4099), (65, 1, 333), (100, 5, 17), (99, 9, 1), (24, 3, 40)]
NATURAL_ONLY = [(100, 5), (100, 10), (100, 20), (99, 9), (120, 3), (100, 1), (128, 1), (65, 1)]

GATE_G = 2e-5          # |Gk - Gt|.max() <= GATE_G |Gt|.max()
GATE_S_RTOL = 2e-5     # S within rtol GATE_S_RTOL,
GATE_S_ATOL = 1e-6     # atol GATE_S_ATOL S.max()


def dp_of(d):
    p = 16
    while p < d:
        p <<= 1
    return p


def slab_floats(d, K):
    return dp_of(d) ** 2 + K


def embed(Gt, S, d, K):
    """float64 natural slab holding Gt and S, zeros elsewhere."""
    DP = dp_of(d)
    G = np.zeros((DP, DP))
    G[:d, :d] = Gt
    return np.concatenate([G.ravel(), np.asarray(S, dtype=np.float64)])


def unembed(gs, d, K):
    """(Gt [d, d], S [K], pad): pad = the slab's entries that hold neither, flattened."""
    gs = np.asarray(gs)
    DP = dp_of(d)
    assert gs.shape == (DP * DP + K,), (gs.shape, d, K)
    G = gs[:DP * DP].reshape(DP, DP)
    real = np.zeros((DP, DP), dtype=bool)
    real[:d, :d] = True
    return G[:d, :d].astype(np.float64), gs[DP * DP:].astype(np.float64), G[~real]


def slab_errors(Gk, Sk, Gt, S):
    """Deviations in units of the gates: (Gt, S); <= 1 passes."""
    eg = np.abs(Gk - Gt).max() / (GATE_G * np.abs(Gt).max())
    es = (np.abs(Sk - S) / (GATE_S_RTOL * np.abs(S) + GATE_S_ATOL * S.max())).max()
    return float(eg), float(es)


def check_slab(gs, Gt, S, d, K, tag=""):
    """The gates of tests/drsa_slab_ref.check_slab on a natural slab: prints, then asserts."""
    Gk, Sk, pad = unembed(gs, d, K)
    eg, es = slab_errors(Gk, Sk, Gt, S)
    bad_pad = int(np.count_nonzero(pad != 0.0))            # NaN counts: an entry never written
    print(f"\nDRSA-ANY-SLAB {tag} d={d} K={K}: Gt dev {eg * GATE_G:.3e} (gate {GATE_G}), S dev {es:.3f} of its gate, "
          f"padding entries != 0: {bad_pad} of {pad.size}")
    assert np.isfinite(np.asarray(gs)).all(), "poison left in the slab"
    assert np.abs(Gk - Gt).max() <= GATE_G * np.abs(Gt).max()
    np.testing.assert_allclose(Sk, S, rtol=GATE_S_RTOL, atol=GATE_S_ATOL * S.max())
    assert bad_pad == 0
    return eg, es


def slab_by_map(A, C, U, concept_of, K, dtype=np.float64):
    """(Gt, S) for an arbitrary column -> concept map, evaluated in `dtype` (float64: the reference
    with that map; float32: a plain fp32 evaluation)."""
    A, C, U = (np.asarray(x, dtype=dtype) for x in (A, C, U))
    XA, XC = A @ U, C @ U
    p = XA * XC
    s = np.zeros((A.shape[0], K), dtype=dtype)
    np.add.at(s.T, concept_of, p.T)
    r = np.maximum(s, 0)
    R = r[:, concept_of]
    return (A.T @ (R * XC) + C.T @ (R * XA)).astype(np.float64), (r * r).sum(0).astype(np.float64)


def finish_ref(Gt, S, N, U, K):
    """(f, U_new) as the finish kernels define them, in float64: M = sqrt(S / N), f = (mean sqrt M)^2,
    c = sqrt(f) / (K N M^1.5) (0 where M = 0), U_new = polar(U + Gt diag(c per column))."""
    U = np.asarray(U, dtype=np.float64)
    d = U.shape[0]
    M = np.sqrt(np.asarray(S, dtype=np.float64) / float(N))
    f = float(np.mean(np.sqrt(M)) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(M > 0, np.sqrt(f) / (K * float(N) * M ** 1.5), 0.0)
    return f, drsa_ref.polar(U + np.asarray(Gt, dtype=np.float64) * np.repeat(c, d // K)[None, :])


@functools.lru_cache(maxsize=None)
def problem(N, d, K):
    """(A, C, U0, Gt, S): the project's synthetic inputs, a QR start and their float64 slab."""
    A, C = drsa_inputs(N, d, 7000 + 31 * d + K)
    U0 = sr.u0(d, d + K)
    Gt, S = sr.slab(A, C, U0, K)
    for x in (A, C, U0, Gt, S):
        x.setflags(write=False)
    return A, C, U0, Gt, S
