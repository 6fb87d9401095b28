"""The Newton-Schulz polar of csrc/polar_ns.h restated in float32 NumPy, the matrix families and the
case tables of tests/test_polar_cases_cpu.py and tests/test_polar_paths_gpu.py.  TEST INFRASTRUCTURE
ONLY (a helper module: pytest does not collect it).

ns_model follows polar_ns / polar_ns16 / drsa_finish_coop_kernel step by step (scaling rule, error,
the three stop clauses in the kernel's order); it shares neither their summation order nor their MFMA
chains, so it sizes tolerances and predicts branch and iteration count, and is not matched bit for
bit.  tests/prca_ref.polar_model_fp32 is the older, simpler model (no scaling, no "last" rule).
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
TOL = 4e-7          # kPolarTol (csrc/drsa_step.hip)
MAX_ITER = 40       # kPolarMaxIter
LAST = 1e-2         # DRSA_NS_LAST (csrc/polar_ns.h)
BRANCH_AT = 2.9     # a^2 ||P||_inf >= 2.9: the inf-norm scale

# a case's modelled ratio a^2 ||P||_inf must lie outside this band, so that the device's float32
# summation order cannot flip the branch
RATIO_BAND = (2.4, 3.5)

D_SIZES = (5, 32, 48, 64, 100, 128)


def polar_dim(d: int) -> int:
    """DP = pow2ceil(max(32, d)): the size polar_kernel embeds diag(V, I) in."""
    p = 32
    while p < d:
        p <<= 1
    return p


def embed(V: np.ndarray) -> np.ndarray:
    d = V.shape[0]
    X = np.eye(polar_dim(d), dtype=F32)
    X[:d, :d] = V
    return X


def ns_model(V, tol=TOL, max_iter=MAX_ITER, last=LAST):
    """(X[:d, :d], info) of the float32 model on the float32 V [d, d].  info: ratio (a^2 ||P||_inf
    with the trace scale a^2 = DP / tr), branch ('tr' | 'inf'), iters (the kernels' iters_out),
    exit ('tol' | 'max' | 'last' | 'floor') and err (the last max|P - I| the loop saw, before the
    final update of a 'last' / 'floor' exit)."""
    V = np.asarray(V, dtype=F32)
    d = V.shape[0]
    X = embed(V)
    DP = X.shape[0]
    I = np.eye(DP, dtype=F32)
    tol, last = F32(tol), F32(last)
    info = {}
    it, err_prev = 0, F32(1)
    with np.errstate(all="ignore"):
        while True:
            P = X.T @ X
            if it == 0:
                tr = np.trace(P, dtype=F32)
                rowmax = np.abs(P).sum(axis=1, dtype=F32).max()
                a2 = F32(DP) / tr
                info["ratio"] = float(a2 * rowmax)
                info["branch"] = "inf" if a2 * rowmax >= F32(BRANCH_AT) else "tr"
                if info["branch"] == "inf":
                    a2 = F32(1) / rowmax
                X = X * np.sqrt(a2)
                P = P * a2
            err = np.abs(P - I).max()
            if err < tol:
                info["exit"] = "tol"
                break
            if it >= max_iter:
                info["exit"] = "max"
                break
            near = F32(DP) * err < last
            floor = it > 0 and err_prev < F32(1e-4) and err > F32(0.25) * err_prev
            err_prev = err
            X = X @ (F32(1.5) * I - F32(0.5) * P)
            it += 1
            if near or floor:
                info["exit"] = "last" if near else "floor"
                break
    info["iters"], info["err"] = it, float(err)
    return X[:d, :d].copy(), info


def _butterfly(v, masks):
    """The xor-shuffle fold of the kernels: every lane ends with the same float32 sum."""
    idx = np.arange(v.shape[-1])
    for m in masks:
        v = (v + v[..., idx ^ m]).astype(F32)
    return v


def first_gram_device_order(V):
    """Iteration 0 of the kernels in THEIR float32 order, as far as the source states it: every entry
    of P = X^T X one fma chain over k ascending from +0 (the MFMA chains of polar_ns.h; an fma is
    emulated as a float64 product and sum rounded once to float32, exact but for a rare double
    rounding), tr(P) folded over 64 lanes (lane l: P[l][l] + P[l + 64][l + 64] + ..., then xor masks
    32 .. 1), the row sums of |P| over TPR = threads / DP partial sums (column c to part c % TPR,
    ascending, then xor masks 1 .. TPR / 2).  Returns {ratio, branch, err}: what decides the branch
    and whether the loop stops at once.  ns_model's NumPy sums differ from these by a few units of
    2^-24, which matters only where a case sits that close to a threshold: the zero-iteration class
    (err against tol = 6.7 units)."""
    X = embed(np.asarray(V, dtype=F32)).astype(np.float64)
    DP = X.shape[0]
    P = np.zeros((DP, DP), dtype=F32)
    for k in range(DP):
        P = (X[k, :, None] * X[k, None, :] + P.astype(np.float64)).astype(F32)
    lanes = np.zeros(64, dtype=F32)
    for i0 in range(0, DP, 64):
        n = min(64, DP - i0)
        lanes[:n] = (lanes[:n] + np.diagonal(P)[i0:i0 + n]).astype(F32)
    tr = _butterfly(lanes, (32, 16, 8, 4, 2, 1))[0]
    TPR = (1024 if DP >= 64 else 256) // DP
    rs = np.zeros((DP, TPR), dtype=F32)
    for c0 in range(0, DP, TPR):
        rs = (rs + np.abs(P[:, c0:c0 + TPR])).astype(F32)
    rowmax = _butterfly(rs, [1 << b for b in range(TPR.bit_length() - 1)])[:, 0].max()
    with np.errstate(all="ignore"):
        a2 = F32(DP) / tr
        ratio = a2 * rowmax
        branch = "inf" if ratio >= F32(BRANCH_AT) else "tr"
        if branch == "inf":
            a2 = F32(1) / rowmax
        err = np.abs((P * a2).astype(F32) - np.eye(DP, dtype=F32)).max()
    return {"ratio": float(ratio), "branch": branch, "err": float(err)}


def polar64(V) -> np.ndarray:
    """The exact polar factor of the float32 V in float64 (oracle/drsa_ref.polar)."""
    Uu, _, Vt = np.linalg.svd(np.asarray(V, dtype=np.float64))
    return Uu @ Vt


def ortho_dev(U) -> float:
    U = np.asarray(U, dtype=np.float64)
    return float(np.abs(U.T @ U - np.eye(U.shape[0])).max())


# ------------------------------------------------------------------------------------ matrix families
def _q(rng, d):
    Q, R = np.linalg.qr(rng.standard_normal((d, d)))
    return Q * np.sign(np.diag(R))[None, :]


def _rng(family, param, d, seed):
    tag = 10000 + int(round(1000 * np.log10(param))) if param else 0
    return np.random.default_rng([seed, d, FAMILIES.index(family), tag])


FAMILIES = ("orth", "scaled_orth", "perm_reflect", "geom", "one_big", "gauss", "quarter_small", "singular")


def make(family: str, d: int, param: float = 0.0, seed: int = 0, null: str = "row") -> np.ndarray:
    """A float32 [d, d] matrix of the family, built in float64 from its own seeded generator.
      orth            Q
      scaled_orth     param * Q
      perm_reflect    a permutation matrix with one sign flipped
      geom            Q1 diag(geomspace(1, 1 / param, d)) Q2^T
      one_big         Q1 diag(param, 1, ..., 1) Q2^T
      gauss           N(0, 1) entries
      quarter_small   Q1 diag(s) Q2^T, a quarter of the singular values at param, the rest 1
      singular        singular values geomspace(1, 0.1, d - 1) and one that is exactly 0 IN FLOAT32:
                      null = "row": a [d-1, d] matrix with those singular values and a zero row put in
                      (the left null vector is a unit vector; X^T X evolves as for any other input);
                      null = "col": its transpose (a zero column, which a DRSA step keeps: the gradient
                      of a zero column of U is zero).  A zero singular value of Q1 diag(s) Q2^T itself
                      does not survive the cast: it comes back at ~1e-9 and then grows by 1.5 per
                      iteration from rounding noise of the same size, which makes the count a coin toss.
    """
    rng = _rng(family, param, d, seed)
    if family == "orth":
        V = _q(rng, d)
    elif family == "scaled_orth":
        V = param * _q(rng, d)
    elif family == "perm_reflect":
        V = np.eye(d)[rng.permutation(d)]
        V[int(rng.integers(d))] *= -1.0
    elif family == "geom":
        V = (_q(rng, d) * np.geomspace(1.0, 1.0 / param, d)[None, :]) @ _q(rng, d).T
    elif family == "one_big":
        s = np.ones(d)
        s[0] = param
        V = (_q(rng, d) * s[None, :]) @ _q(rng, d).T
    elif family == "gauss":
        V = rng.standard_normal((d, d))
    elif family == "quarter_small":
        s = np.ones(d)
        s[:max(d // 4, 1)] = param
        V = (_q(rng, d) * s[None, :]) @ _q(rng, d).T
    elif family == "singular":
        R = (_q(rng, d - 1) * np.geomspace(1.0, 0.1, d - 1)[None, :]) @ _q(rng, d)[:, :d - 1].T   # [d-1, d]
        V = np.insert(R, int(rng.integers(d)), 0.0, axis=0)
        if null == "col":
            V = V.T
    else:
        raise ValueError(family)
    return np.ascontiguousarray(V, dtype=F32)


# ------------------------------------------------------------------------------------------ case table
# (family, param): the polar cases of tests/test_polar_paths_gpu.py, each at every d of D_SIZES.
# A family with one small singular value (1e-3, the rest 1) is not in the table: its modelled ratio sits
# inside RATIO_BAND (2.7 .. 3.3) at every d.  quarter_small(0.05) stands in for it.
POLAR_FAMILIES = [("orth", 0.0), ("scaled_orth", 3.0), ("scaled_orth", 1e-3), ("scaled_orth", 1e3),
                  ("perm_reflect", 0.0), ("geom", 1e1), ("geom", 1e2), ("geom", 1e3), ("geom", 1e4),
                  ("one_big", 30.0), ("gauss", 0.0), ("quarter_small", 0.05), ("singular", 0.0)]

# gates of the GPU test on U against polar64 and on U^T U - I (those of test_orthogonalize_api); the
# ill-conditioned geom(1e3), geom(1e4) take max(GATE_U, MODEL_FACTOR x the model's own deviation)
GATE_U = 5e-5
GATE_ORTH = 5e-6
MODEL_FACTOR = 4.0
ILL_CONDITIONED = {("geom", 1e3), ("geom", 1e4)}


def case_id(family, param, d):
    return f"{family}{'' if not param else f'({param:g})'}-d{d}"


def scaled_orth_ratio(c: float, d: int) -> float:
    """a^2 ||P||_inf of diag(c Q, I) in exact arithmetic: P = diag(c^2 I_d, I), tr = c^2 d + DP - d."""
    DP = polar_dim(d)
    return max(c * c, 1.0 if DP > d else 0.0) * DP / (c * c * d + DP - d)


def expected_branch(family, param, d):
    """The branch a case is named for.  orth / perm_reflect: P = I, ratio 1.  scaled_orth: the
    closed form above.  one_big(30): P has one eigenvalue 900 against a trace of ~DP + 899, ratio >=
    900 DP / (DP + 899) / 1 > 25.  gauss: ||P||_inf ~ d + 0.8 d sqrt(d) against a mean diagonal of
    d.  The others by their spectrum: at d = 5 the 27 identity rows of the embedding dominate trace
    and norm (ratio ~1.2); from d = 32 the row sums of |P| exceed the mean eigenvalue several times."""
    if family in ("orth", "perm_reflect"):
        return "tr"
    if family == "scaled_orth":
        return "inf" if scaled_orth_ratio(param, d) >= BRANCH_AT else "tr"
    if family in ("one_big", "gauss"):
        return "inf"
    return "tr" if d == 5 else "inf"


def iteration_class(family, param, d):
    """(lo, hi) bounds on the iteration count that the case's class fixes (None: open)."""
    exact_small = d == polar_dim(d) and d <= 64
    if family in ("orth", "scaled_orth", "perm_reflect") and exact_small:
        return 0, 0
    if family == "singular":
        return MAX_ITER, MAX_ITER
    if family in ("geom", "one_big", "gauss"):
        return 10, None
    return None, None


# seeds other than 0: the zero-iteration class needs max|a^2 P - I| < tol = 6.7 units of 2^-24 in the
# device's summation order too (first_gram_device_order); these two cases sat at 8 and 6 units on seed
# 0 and sit at 4 (with ns_model's NumPy order at 4 as well) on these
SEEDS = {("scaled_orth", 1e-3, 64): 10, ("scaled_orth", 1e3, 64): 2}
ZERO_CLASS_ERR = 4.5 * 2.0 ** -24   # both orders at most 4 units: two units (one of the grid above 1) under tol


@functools.lru_cache(maxsize=None)
def polar_case(family: str, param: float, d: int):
    """(V float32, X model, info, model's max|X - polar64(V)|, model's max|X^T X - I|), once per session."""
    V = make(family, d, param, SEEDS.get((family, param, d), 0))
    X, info = ns_model(V)
    dev = float(np.abs(X.astype(np.float64) - polar64(V)).max()) if family != "singular" else float("nan")
    for a in (V, X):
        a.setflags(write=False)
    return V, X, info, dev, ortho_dev(X)


def gate_u(family, param, model_dev):
    return max(GATE_U, MODEL_FACTOR * model_dev) if (family, param) in ILL_CONDITIONED else GATE_U


# ------------------------------------------------------------------------------------ hostile DRSA steps
# (N, d, K) of tests/test_polar_paths_gpu.py's step tests and the kernel whose polar drsa_run takes there
STEP_PROBLEMS = [(3000, 128, 16), (2048, 128, 4),      # cooperative finish, exact
                 (3000, 100, 4), (777, 66, 2),         # cooperative finish, padded (d = 66: scalar staging)
                 (1000, 100, 5),                       # natural geometry, drsa_any_run: cooperative too
                 (1000, 64, 4), (777, 42, 3),          # fused step
                 (777, 32, 2), (300, 12, 3)]           # separate kernels at PD = 32
# variant -> (steps, the problems it runs on; None: all)
STEP_VARIANTS = {"data8": (3, None), "u0_geom2": (2, None), "u0_3q": (2, None),
                 "u0_singular": (1, [(2048, 128, 4), (1000, 64, 4), (777, 32, 2)]),
                 "dead_concept": (2, [(2048, 128, 4), (3000, 100, 4), (1000, 64, 4)])}
STEP_CASES = [(N, d, K, v) for v, (_, only) in STEP_VARIANTS.items() for (N, d, K) in (only or STEP_PROBLEMS)]

# U0 seeds other than 17.  3 Q at (777, 66, 2) converges to the float32 floor in its 8th iteration and
# stops there only if that floor is under tol (else it updates once more: 9); on seed 17 the model's
# floor is 3.6e-7, on seed 1 it is 2.4e-7, four units of 2^-24.
STEP_SEEDS = {(777, 66, 2, "u0_3q"): 1}

# iteration classes of a step's polar: what the explicit loop asserts of iters_out
HOSTILE, FRIENDLY, STUCK = "hostile", "friendly", "stuck"
CLASS_BOUNDS = {HOSTILE: (10, MAX_ITER - 1), FRIENDLY: (0, 8), STUCK: (MAX_ITER, MAX_ITER)}


def step_classes(variant):
    steps = STEP_VARIANTS[variant][0]
    first = {"data8": HOSTILE, "u0_geom2": HOSTILE, "u0_3q": FRIENDLY, "u0_singular": STUCK,
             "dead_concept": FRIENDLY}[variant]
    return [first] + [HOSTILE if variant == "data8" else FRIENDLY] * (steps - 1)


@functools.lru_cache(maxsize=None)
def step_problem(N, d, K, variant):
    """(A, C, U0) float32 of a step case (read-only; shared by the tests of one session).
      data8         A and C of drsa_inputs times 8 (exact in float32), QR-orthogonal U0
      u0_geom2      U0 = geom(1e2)
      u0_3q         U0 = 3 Q
      u0_singular   U0 = singular(null="col"): a zero column, so that column of U0 + G is zero too
      dead_concept  U0 = I and C[:, :dk] = -A[:, :dk]: r_n0 = relu(-sum a^2) = 0 in every row"""
    from drsa_audio_amd.utils.synthetic import drsa_inputs
    A, C = drsa_inputs(N, d, 9000 + N + d)
    seed = STEP_SEEDS.get((N, d, K, variant), 17)
    if variant == "data8":
        A, C, U0 = A * F32(8), C * F32(8), make("orth", d, 0.0, seed)
    elif variant == "u0_geom2":
        U0 = make("geom", d, 1e2, seed)
    elif variant == "u0_3q":
        U0 = make("scaled_orth", d, 3.0, seed)
    elif variant == "u0_singular":
        U0 = make("singular", d, 0.0, seed, null="col")
    elif variant == "dead_concept":
        C = C.copy()
        C[:, :d // K] = -A[:, :d // K]
        U0 = np.eye(d, dtype=F32)
    else:
        raise ValueError(variant)
    out = tuple(np.ascontiguousarray(x, dtype=F32) for x in (A, C, U0))
    for x in out:
        x.setflags(write=False)
    return out


def model_steps(N, d, K, variant):
    """[info of ns_model on the float32 V = U + G of each step], U and G from the float64 closed form
    and U advanced by the exact polar (the pseudo-polar's stand-in for a stuck step is not needed: a
    stuck step is always the last)."""
    import drsa_ref
    A, C, U0 = step_problem(N, d, K, variant)
    U = U0.astype(np.float64)
    infos = []
    for _ in range(STEP_VARIANTS[variant][0]):
        _, G, _, _ = drsa_ref.closed_form(A, C, U, K)
        V = (U + G).astype(F32)
        infos.append(ns_model(V)[1])
        U = polar64(V)
    return infos
