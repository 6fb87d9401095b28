"""The Newton-Schulz polar off the near-orthogonal path, in every kernel that holds a copy of it (GPU).

Part 1, drsa_amd_polar (polar_kernel<32 | 64 | 128>: polar_ns16<32>, polar_ns16<64>, polar_ns<128>,
each exact and padded) on the matrix families of tests/polar_ref.py against the float64 SVD polar of
the float32 input, with iters_out against the float32 model (tests/test_polar_cases_cpu.py keeps the
case table honest): the inf-norm scaling branch, 10 to 28 iterations, the `err < tol` exit at 0
iterations, the max_iter exit, exact inputs and power-of-4 scale invariance.

Part 2, the DRSA step kernels on hostile steps (data scaled by 8, non-orthogonal starts, a singular
start, a dead concept): drsa_run (fused step at DP = 64, cooperative finish at DP = 128, separate
kernels below), drsa_run_joint and drsa_run_batched must equal the explicit loop of the partial and
the one-workgroup finish bit for bit, with every step's iters_out in the class the case is there for;
the first step is judged against the float64 finish of the device's own slab.

MEASURED on an MI355X (worst over d = 5, 32, 48, 64, 100, 128 per family; U dev = max|U - polar64(V)|,
orth = max|U^T U - I|; "model" is tests/polar_ref.ns_model on the same V).  The model's float32 NumPy
products turn out to round like the kernels' fma chains at most sizes, so many figures agree to every
printed digit; they differ at d = 48 and 64 (polar_ns16<64>).

    family               U dev      model      gate       orth       model      gate    iterations  model
    orth                 6.43e-08   6.43e-08   5e-5       4.79e-07   4.79e-07   5e-6     0 .. 1      0 .. 1
    scaled_orth(3)       1.02e-07   1.02e-07   5e-5       7.61e-07   7.61e-07   5e-6     0 .. 7      0 .. 7
    scaled_orth(1e-3)    1.38e-07   1.38e-07   5e-5       5.93e-07   4.87e-07   5e-6     0 .. 22     0 .. 22
    scaled_orth(1e3)     9.17e-08   7.65e-08   5e-5       5.57e-07   5.57e-07   5e-6     0 .. 21     0 .. 21
    perm_reflect         0          0          5e-5       0          0          5e-6     0           0
    geom(1e1)            3.49e-07   3.49e-07   5e-5       7.09e-07   7.09e-07   5e-6    10 .. 11    10 .. 11
    geom(1e2)            9.37e-07   9.37e-07   5e-5       3.91e-07   3.91e-07   5e-6    15 .. 17    15 .. 17
    geom(1e3)            3.48e-06   3.45e-06   5e-5 (*)   6.16e-07   6.16e-07   5e-6    21 .. 22    21 .. 22
    geom(1e4)            2.70e-05   2.70e-05   1.1e-4 (*) 4.86e-07   4.86e-07   5e-6    27 .. 28    27 .. 28
    one_big(30)          6.65e-07   5.63e-07   5e-5       4.54e-07   4.54e-07   5e-6    13 .. 14    13 .. 14
    gauss                6.49e-07   6.49e-07   5e-5       4.89e-07   4.89e-07   5e-6    11 .. 25    11 .. 25
    quarter_small(0.05)  5.31e-07   5.31e-07   5e-5       4.79e-07   4.79e-07   5e-6    11 .. 14    11 .. 14
    singular             -          -          none       3.73e-01   3.73e-01   none    40          40
    (*) max(5e-5, 4 x the model's deviation on that V): 5e-5 for every geom(1e3) case, 7.4e-5 .. 1.1e-4 for
        geom(1e4) at d >= 32 (measured 1.73e-5 .. 2.70e-5 there).
    The only count that differs from the model's: one_big(30) at d = 64, 13 against 14.

    step kernels, first step against the float64 finish of the device slab (gates 1e-6 / 2e-5 / 2e-6):
    variant        f dev      U dev      orth       iterations of every step (all nine problems)
    data8          3.88e-08   6.71e-07   4.90e-07   11 .. 23, all hostile
    u0_geom2       4.47e-08   8.04e-07   6.91e-07   15 .. 18, then 3 .. 6
    u0_3q          5.16e-08   2.61e-07   5.50e-07   3 .. 8, then 3 .. 6
    u0_singular    3.27e-08   -          -          40
    dead_concept   3.17e-08   5.39e-07   1.08e-06   4, 4
    drsa_run, drsa_run_joint and drsa_run_batched equalled the explicit loop bit for bit in every case.
"""
import functools

import numpy as np
import pytest
import torch

import drsa_any_ref as ar
import drsa_slab_ref as sr
import polar_ref as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
POLAR_CASES = [(f, p, d) for f, p in pr.POLAR_FAMILIES for d in pr.D_SIZES]


def _gpu(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in arrs]


def _polar(V):
    """(U float32 numpy, iters_out) of drsa_amd_polar on the float32 V."""
    from drsa_audio_amd import _capi
    Vg, = _gpu(V)
    out = torch.full_like(Vg, float("nan"))
    it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    _capi.call("drsa_amd_polar", Vg.data_ptr(), V.shape[0], out.data_ptr(), it.data_ptr(), _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(it)


# ---------------------------------------------------------------------------------------------
# 1. drsa_amd_polar
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POLAR_CASES, ids=lambda c: pr.case_id(*c))
def test_polar_family(case):
    family, param, d = case
    V, _, info, model_dev, model_orth = pr.polar_case(*case)
    U, iters = _polar(V)
    assert np.isfinite(U).all()
    lo, hi = pr.iteration_class(*case)
    if family == "singular":
        # no accuracy gate: (V^T V)^{-1/2} does not exist.  iters_out == max_iter is how a caller sees it.
        U2, iters2 = _polar(V)
        print(f"\nPOLAR-GPU {pr.case_id(*case)}: iterations {iters} (model {info['iters']}), "
              f"orthogonality {pr.ortho_dev(U):.3e} (model {model_orth:.3e}, no gate)")
        assert iters == iters2 == pr.MAX_ITER
        assert np.array_equal(U, U2)
        return
    dev = float(np.abs(U.astype(np.float64) - pr.polar64(V)).max())
    orth = pr.ortho_dev(U)
    gate = pr.gate_u(family, param, model_dev)
    print(f"\nPOLAR-GPU {pr.case_id(*case)}: U dev {dev:.3e} (model {model_dev:.3e}, gate {gate:.1e}), "
          f"orthogonality {orth:.3e} (model {model_orth:.3e}, gate {pr.GATE_ORTH:.0e}), "
          f"iterations {iters} (model {info['iters']}, {info['branch']} branch, ratio {info['ratio']:.2f})")
    assert dev < gate
    assert orth < pr.GATE_ORTH
    assert abs(iters - info["iters"]) <= 1
    if (lo, hi) == (0, 0):
        assert iters == 0


@pytest.mark.parametrize("d", [32, 64, 128])
def test_perm_reflect_comes_back_bit_for_bit(d):
    """P = I exactly, tr = DP, a = 1, err = 0: no arithmetic touches V."""
    V = pr.polar_case("perm_reflect", 0.0, d)[0]
    U, iters = _polar(V)
    assert iters == 0
    assert np.array_equal(U, V)


@pytest.mark.parametrize("d", [32, 64])
def test_orth_at_exact_size_is_only_scaled(d):
    """0 iterations return a V with a^2 = DP / tr(P) within rounding of 1: within 2e-7 of V entrywise."""
    V = pr.polar_case("orth", 0.0, d)[0]
    U, iters = _polar(V)
    assert iters == 0
    assert np.abs(U - V).max() <= 2e-7


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("family,param", [("geom", 1e2), ("gauss", 0.0)])
def test_power_of_four_scale_invariance_is_bitwise(family, param, d):
    """polar(4^k V) == polar(V) bit for bit on the inf-norm branch: tr, ||P||_inf, the IEEE division
    and square root (no fast-math, no contraction), X a and P a^2 are all exact under a power of 4."""
    V, _, info, _, _ = pr.polar_case(family, param, d)
    assert info["branch"] == "inf"
    U0, it0 = _polar(V)
    assert it0 >= 10
    for k in (1, -1, 10, -10):
        Vk = V * np.float32(4.0 ** k)
        assert np.array_equal(Vk.astype(np.float64), V.astype(np.float64) * 4.0 ** k)     # the scaling is exact
        Uk, itk = _polar(Vk)
        assert itk == it0, k
        assert np.array_equal(Uk, U0), k


# ---------------------------------------------------------------------------------------------
# 2. the step kernels on hostile steps
# ---------------------------------------------------------------------------------------------
def _case_id(c):
    return "-".join(map(str, c))


def _natural(d, K):
    from drsa_audio_amd.xai.drsa.drsa import geometry_kind
    return geometry_kind(d, K) == "natural"


def _dp(d, K):
    return ar.dp_of(d) if _natural(d, K) else sr.geom(d, K)[2]


@functools.lru_cache(maxsize=None)
def _loop(case):
    """The explicit partial + one-workgroup-finish loop of a step case, once per session:
    (f [steps + 1], U_S, {iters, gs0, U1}) as numpy."""
    N, d, K, variant = case
    Ag, Cg, Ug = _gpu(*pr.step_problem(*case))
    f, U, ex = sr.explicit_loop(Ag, Cg, Ug, K, pr.STEP_VARIANTS[variant][0], natural=_natural(d, K), want_iters=True)
    ex["U1"] = ex["U1"].cpu().numpy()
    return f.cpu().numpy(), U.cpu().numpy(), ex


def _run(case, steps=None):
    """drsa_run on a side stream (its hipGraph replay): (U_S, trajectory) as numpy; the cooperative
    finish's status word is checked where the workspace has one."""
    from drsa_audio_amd.xai.drsa.drsa import DrsaWorkspace, drsa_run
    N, d, K, variant = case
    Ag, Cg, Ug = _gpu(*pr.step_problem(*case))
    ws = DrsaWorkspace(N, d, K, DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        U, traj = drsa_run(Ag, Cg, Ug, K, steps or pr.STEP_VARIANTS[variant][0], ws=ws)
    torch.cuda.synchronize()
    if _dp(d, K) == 128 and not _natural(d, K):
        assert ws.coop_status() == 0
    return U.cpu().numpy(), traj.cpu().numpy()


@pytest.mark.parametrize("case", pr.STEP_CASES, ids=_case_id)
def test_run_equals_explicit_loop_bitwise_on_hostile_steps(case):
    N, d, K, variant = case
    f, U, ex = _loop(case)
    classes = pr.step_classes(variant)
    print(f"\nSTEP-GPU {_case_id(case)}: iterations {ex['iters']} (classes {classes})")
    # the case is on the path it is there for (else it would pass vacuously)
    for it, cls in zip(ex["iters"], classes):
        lo, hi = pr.CLASS_BOUNDS[cls]
        assert lo <= it <= hi, (ex["iters"], classes)
    assert np.isfinite(f).all() and np.isfinite(U).all()
    U_run, traj = _run(case)
    assert np.array_equal(traj, f), (traj, f)
    assert np.array_equal(U_run, U)


@pytest.mark.parametrize("case", pr.STEP_CASES, ids=_case_id)
def test_first_hostile_step_against_float64_finish_of_the_device_slab(case):
    """The polar judged on exactly the V the kernel saw: the device's reduced slab of step 0, cast to
    float64, through the reference finish (gates of test_finish_on_reference_built_slab); the slab
    itself against the float64 slab of the same inputs (check_slab's gates)."""
    N, d, K, variant = case
    A, C, U0 = pr.step_problem(*case)
    f, _, ex = _loop(case)
    gs0 = ex["gs0"].astype(np.float64)
    Gt, S = sr.slab(A, C, U0, K)
    if _natural(d, K):
        ar.check_slab(gs0, Gt, S, d, K, tag=variant)
        Gk, Sk, _ = ar.unembed(gs0, d, K)
        f_ref, U_ref = ar.finish_ref(Gk, Sk, N, U0, K)
    else:
        sr.check_slab(gs0, Gt, S, d, K, tag=variant)
        Gk, Sk, _ = sr.unembed(gs0, d, K)
        f_ref, U_ref = sr.finish(gs0, N, U0, K)
    U1 = ex["U1"].astype(np.float64)
    df = abs(float(f[0]) - f_ref) / abs(f_ref)
    assert np.isfinite(U1).all() and np.isfinite(f).all()
    if variant == "dead_concept":
        # S_0 = 0 -> c_0 = 0 (the reference's autograd has NaN there): concept 0's columns of the slab are
        # exact zeros and V keeps U0's columns there; the float64 finish applies the same contract
        dk = d // K
        assert Sk[0] == 0.0 and (Sk[1:] > 0).all()
        assert (Gk[:, :dk] == 0.0).all()
    if variant == "u0_singular":
        print(f"\nSTEP-ACC {_case_id(case)}: f dev {df:.3e} (gate 1e-6); singular V: no U gate")
        assert df <= 1e-6
        assert (ex["U1"] == 0).all(axis=0).sum() == 1          # the zero column stays a zero column
        return
    du, do = float(np.abs(U1 - U_ref).max()), pr.ortho_dev(U1)
    print(f"\nSTEP-ACC {_case_id(case)}: f dev {df:.3e} (gate 1e-6), U dev {du:.3e} (gate 2e-5), "
          f"orthogonality {do:.3e} (gate 2e-6), iterations {ex['iters'][0]}")
    assert df <= 1e-6
    assert du < 2e-5
    assert do < 2e-6


PADDED_PROBLEMS = [p for p in pr.STEP_PROBLEMS if p != (1000, 100, 5)]
# two variants of one shape side by side, at one step count
PAIRS = [(p, ("data8", "u0_geom2"), 3) for p in PADDED_PROBLEMS] + \
        [(p, ("u0_singular", "dead_concept"), 2) for p in ((2048, 128, 4), (1000, 64, 4))]


@pytest.mark.parametrize("problem,variants,steps", PAIRS, ids=lambda v: _case_id(v) if isinstance(v, tuple) else str(v))
def test_joint_and_batched_runs_equal_single_runs_bitwise(problem, variants, steps):
    """drsa_run_joint (one-workgroup or cooperative finish on forked streams) and drsa_run_batched
    (drsa_finish_batched_kernel: the one-workgroup polar at every DP) of two variants of one shape
    against drsa_run of each, bit for bit."""
    from drsa_audio_amd.xai.drsa.drsa import drsa_run_batched, drsa_run_joint
    N, d, K = problem
    cases = [(N, d, K, v) for v in variants]
    probs = [(*_gpu(*pr.step_problem(*c)), K) for c in cases]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        joint = drsa_run_joint(probs, steps)
        batched = drsa_run_batched(probs, steps)
    torch.cuda.synchronize()
    for c, (Uj, tj), (Ub, tb) in zip(cases, joint, batched):
        U, traj = _run(c, steps)
        assert np.isfinite(traj).all() and np.isfinite(U).all()
        assert np.array_equal(tj.cpu().numpy(), traj) and np.array_equal(Uj.cpu().numpy(), U), c
        assert np.array_equal(tb.cpu().numpy(), traj) and np.array_equal(Ub.cpu().numpy(), U), c
