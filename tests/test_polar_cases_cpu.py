"""The float32 model of the Newton-Schulz polar (tests/polar_ref.py) and the case tables of
tests/test_polar_paths_gpu.py, on the CPU: every case the GPU tests use takes the branch and has the
iteration count it is there for, with a margin the device's float32 summation order cannot cross, and
the model alone passes the GPU gates three times over.  (The GPU tests compare the kernels with the
float64 polar and use the model for iteration counts and for the gate of the ill-conditioned cases.)
"""
import numpy as np
import pytest

import polar_ref as pr

POLAR_CASES = [(f, p, d) for f, p in pr.POLAR_FAMILIES for d in pr.D_SIZES]


def _id(c):
    return pr.case_id(*c)


def test_model_on_matrices_with_known_answers():
    """ns_model itself: the identity and a permutation stop at once with their own bits; 2 I takes the
    trace scale to exactly I; diag(1, ..., 1, 1/2) converges to I; tol / max_iter / last are honoured."""
    for d in (5, 32, 100):
        X, info = pr.ns_model(np.eye(d, dtype=np.float32))
        assert np.array_equal(X, np.eye(d, dtype=np.float32)) and info["iters"] == 0 and info["exit"] == "tol"
        assert info["branch"] == "tr" and info["ratio"] == 1.0
    X, info = pr.ns_model(2 * np.eye(64, dtype=np.float32))
    assert np.array_equal(X, np.eye(64, dtype=np.float32)) and info["iters"] == 0
    V = np.eye(32, dtype=np.float32)
    V[-1, -1] = 0.5
    X, info = pr.ns_model(V)
    assert np.abs(X - np.eye(32)).max() < 1e-6 and 3 <= info["iters"] <= 6 and info["exit"] in ("tol", "last")
    _, info = pr.ns_model(V, max_iter=2)
    assert info["iters"] == 2 and info["exit"] == "max"
    _, info = pr.ns_model(V, last=0.0)            # no early "last": runs to tol (or the rounding floor)
    assert info["exit"] in ("tol", "floor")
    Z = pr.make("singular", 32, null="col")
    assert (Z == 0).all(axis=0).sum() == 1 and np.linalg.matrix_rank(Z.astype(np.float64)) == 31
    Z = pr.make("singular", 32)
    assert (Z == 0).all(axis=1).sum() == 1 and np.linalg.matrix_rank(Z.astype(np.float64)) == 31


def test_scaled_orth_ratio_closed_form():
    """The closed form expected_branch uses for scaled_orth against the model's ratio."""
    for c in (3.0, 1e-3, 1e3):
        for d in pr.D_SIZES:
            _, _, info, _, _ = pr.polar_case("scaled_orth", c, d)
            assert abs(info["ratio"] - pr.scaled_orth_ratio(c, d)) <= 1e-4 * info["ratio"]


@pytest.mark.parametrize("case", POLAR_CASES, ids=_id)
def test_polar_case_is_what_it_is_named_for(case):
    family, param, d = case
    V, X, info, dev, orth = pr.polar_case(*case)
    g0 = pr.first_gram_device_order(V)
    gate = pr.gate_u(family, param, dev)
    print(f"\nPOLAR-MODEL {_id(case)}: ratio {info['ratio']:.3f} ({g0['ratio']:.3f} in device order) branch "
          f"{info['branch']} iterations {info['iters']} exit {info['exit']} | U dev {dev:.2e} (gate {gate:.1e}) "
          f"orthogonality {orth:.2e} (gate {pr.GATE_ORTH:.0e})")
    assert V.dtype == np.float32 and V.shape == (d, d)
    # branch, with the ratio clear of the threshold in the model's and in the device's order
    assert info["branch"] == g0["branch"] == pr.expected_branch(*case)
    for r in (info["ratio"], g0["ratio"]):
        assert not pr.RATIO_BAND[0] <= r <= pr.RATIO_BAND[1], r
    # iteration class
    lo, hi = pr.iteration_class(*case)
    assert lo is None or info["iters"] >= lo
    assert hi is None or info["iters"] <= hi
    if (lo, hi) == (0, 0):
        assert info["exit"] == "tol"
        assert max(info["err"], g0["err"]) <= pr.ZERO_CLASS_ERR      # clear of tol in either order
    if family == "singular":
        # stuck for good: rank DP - 1 keeps some diagonal entry of P at least 1 / DP under 1, far above
        # every stop threshold (tol = 4e-7; "last" needs err < 1e-2 / DP, a hundred times less)
        assert info["exit"] == "max" and info["err"] >= 1.0 / pr.polar_dim(d)
        assert np.isfinite(X).all()
        return
    assert info["exit"] != "floor"
    # the reference alone passes: a third of the GPU gates at most
    assert dev <= gate / 3
    assert orth <= pr.GATE_ORTH / 3


def test_floor_exit_is_out_of_reach_below_dp_128():
    """err_prev < 1e-4 implies DP * err_prev < 1e-2 for DP <= 64: the loop ended one iteration
    earlier, by "last".  At DP = 128 the floor clause needs err_prev in [1e-2 / 128, 1e-4)."""
    for DP in (32, 64):
        assert DP * 1e-4 < pr.LAST
    assert pr.LAST / 128 < 1e-4
    assert all(pr.polar_case(*c)[2]["exit"] != "floor" for c in POLAR_CASES)


@pytest.mark.parametrize("case", pr.STEP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_step_case_is_in_its_iteration_class(case):
    """The model on V = U + G of every step of a step case (float64 closed form, exact polar between
    steps): hostile steps take the inf-norm branch far from the threshold, or at least 10 iterations on
    the trace branch; every step's count is in the class the GPU test asserts of iters_out."""
    N, d, K, variant = case
    infos = pr.model_steps(*case)
    classes = pr.step_classes(variant)
    assert len(infos) == len(classes) == pr.STEP_VARIANTS[variant][0]
    for t, (info, cls) in enumerate(zip(infos, classes)):
        lo, hi = pr.CLASS_BOUNDS[cls]
        print(f"\nSTEP-MODEL {case} step {t}: {cls}, ratio {info['ratio']:.2f} branch {info['branch']} "
              f"iterations {info['iters']} exit {info['exit']}")
        assert lo <= info["iters"] <= hi
        assert info["exit"] != "floor" and (info["exit"] == "max") == (cls == pr.STUCK)
        if cls == pr.HOSTILE and d >= 32:
            assert info["branch"] == "inf" and info["ratio"] > pr.RATIO_BAND[1]
    A, C, U0 = pr.step_problem(*case)
    if variant == "u0_singular":
        assert (U0 == 0).all(axis=0).sum() == 1
    if variant == "dead_concept":
        dk = d // K
        assert ((A[:, :dk].astype(np.float64) * C[:, :dk]).sum(1) < 0).all()     # r_n0 = 0 in every row
