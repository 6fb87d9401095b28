"""The natural DRSA geometry on the GPU (drsa_amd_drsa_any_*: every K | d at d <= 128, for the
shapes the padded geometry refuses): the ragged partial kernel against the float64 slab, the
finish at a non-power-of-two block stride, step / run against the oracle, both geometries where
both apply, row shards, the file-writing API and the unsupported combinations.

Gates are the project's for the same fp32 arithmetic (tests/test_drsa_partial_matrix_gpu.py,
tests/test_drsa_gpu.py); tests/test_drsa_any_cpu.py shows what they separate at these shapes.
"""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import drsa_any_ref as ar
import drsa_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N_STEP = 4099


def _gpu(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in arrs]


def _any_ws(N, d, K):
    from drsa_audio_amd import _capi
    nbytes = _capi.lib().drsa_amd_drsa_any_workspace_bytes(N, d, K)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV)


def _ortho(U, d):
    U = np.asarray(U, dtype=np.float64)
    return np.abs(U.T @ U - np.eye(d)).max()


@functools.lru_cache(maxsize=None)
def _oracle_step(N, d, K):
    """float64 oracle of one step: (f, U_new)."""
    A, C, U0, _, _ = ar.problem(N, d, K)
    f, G, _, _ = drsa_ref.closed_form(A, C, U0, K)
    return f, drsa_ref.polar(U0.astype(np.float64) + G)


def _check_step(tag, f, Un, N, d, K):
    """Test 3's gates against the float64 oracle (closed form + exact polar)."""
    f_ref, U_ref = _oracle_step(N, d, K)
    Un = np.asarray(Un, dtype=np.float64)
    df, du, do = abs(f - f_ref) / abs(f_ref), np.abs(Un - U_ref).max(), _ortho(Un, d)
    print(f"\nDRSA-ANY-STEP {tag} d={d} K={K}: f dev {df:.3e} (gate 1e-5), U dev {du:.3e} (gate 2e-5), "
          f"orthogonality {do:.3e} (gate 2e-6)")
    assert df <= 1e-5
    assert du < 2e-5
    assert do < 2e-6


# ---------------------------------------------------------------------------------------------
# 1. the partial against the float64 slab
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K,N", ar.PARTIAL_SHAPES)
def test_any_partial_slab_matches_reference(d, K, N):
    from drsa_audio_amd import _capi
    A, C, U0, Gt, S = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    E = _capi.lib().drsa_amd_drsa_any_slab_floats(d, K)
    assert E == ar.slab_floats(d, K)
    gs = torch.full((E,), float("nan"), dtype=torch.float32, device=DEV)
    ws = _any_ws(N, d, K)
    _capi.call("drsa_amd_drsa_any_partial", Ag.data_ptr(), Cg.data_ptr(), N, d, K, Ug.data_ptr(), gs.data_ptr(),
               ws.data_ptr(), ws.numel(), _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    ar.check_slab(gs.cpu().numpy().astype(np.float64), Gt, S, d, K, tag=f"N={N}")


def test_any_partial_of_no_rows_is_a_zero_slab():
    from drsa_audio_amd import _capi
    d, K = 100, 5
    gs = torch.full((ar.slab_floats(d, K),), float("nan"), dtype=torch.float32, device=DEV)
    p = torch.zeros(16, device=DEV)
    _capi.call("drsa_amd_drsa_any_partial", p.data_ptr(), p.data_ptr(), 0, d, K, p.data_ptr(), gs.data_ptr(), None, 0,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert (gs == 0).all()


# ---------------------------------------------------------------------------------------------
# 2. the finish on a slab the reference built (block stride dk, not a power of two)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(100, 5), (99, 9), (128, 1), (24, 3)])
def test_any_finish_on_reference_built_slab(d, K):
    from drsa_audio_amd import _capi
    N = 333
    A, C, U0, Gt, S = ar.problem(N, d, K)
    gs32 = ar.embed(Gt, S, d, K).astype(np.float32)
    G32, S32, _ = ar.unembed(gs32, d, K)
    f_ref, U_ref = ar.finish_ref(G32, S32, N, U0, K)
    gs = torch.from_numpy(gs32).to(DEV)
    U = torch.from_numpy(np.ascontiguousarray(U0)).to(DEV)
    U_out = torch.full_like(U, float("nan"))
    f = torch.full((2,), float("nan"), device=DEV)
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = _capi.stream_ptr(DEV)
    _capi.call("drsa_amd_drsa_any_finish", gs.data_ptr(), N, d, K, U.data_ptr(), U_out.data_ptr(), f.data_ptr(), 0,
               it.data_ptr(), st)
    _capi.call("drsa_amd_drsa_any_finish", gs.data_ptr(), N, d, K, U.data_ptr(), None, f[1:].data_ptr(), 1, None, st)
    torch.cuda.synchronize()
    Un = U_out.cpu().numpy().astype(np.float64)
    df, du, do = abs(float(f[0]) - f_ref) / abs(f_ref), np.abs(Un - U_ref).max(), _ortho(Un, d)
    print(f"\nDRSA-ANY-FINISH d={d} K={K}: f dev {df:.3e} (gate 1e-6), U dev {du:.3e} (gate 2e-5), "
          f"orthogonality {do:.3e} (gate 2e-6), iterations {int(it)}")
    assert df <= 1e-6
    assert du < 2e-5
    assert do < 2e-6
    assert float(f[1]) == float(f[0])          # objective-only mode
    assert 1 <= int(it) <= 40


# ---------------------------------------------------------------------------------------------
# 3. drsa_step against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(100, 5), (100, 20), (128, 1)])
def test_step_matches_oracle(d, K):
    from drsa_audio_amd.xai.drsa.drsa import drsa_objective, drsa_step, geometry_kind
    assert geometry_kind(d, K) == "natural"
    N = N_STEP
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    Un, f = drsa_step(Ag, Cg, Ug, K)
    f_obj = drsa_objective(Ag, Cg, Ug, K)
    torch.cuda.synchronize()
    _check_step("drsa_step", float(f), Un.cpu().numpy(), N, d, K)
    assert float(f_obj) == float(f)
    # the reference's own iteration (torch fp32 autograd + eigh): the same gates
    Ur, fr, _ = drsa_ref.step(torch.from_numpy(A), torch.from_numpy(C), torch.from_numpy(U0), K)
    df, du = abs(float(f) - fr) / abs(fr), (Un.cpu() - Ur).abs().max().item()
    print(f"vs drsa_ref.step: f dev {df:.3e} (gate 1e-5), U dev {du:.3e} (gate 2e-5)")
    assert df <= 1e-5
    assert du < 2e-5


# ---------------------------------------------------------------------------------------------
# 4. drsa_run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(100, 5), (128, 1)])
def test_run_equals_partial_finish_loop_bitwise_graph_and_eager(d, K):
    """drsa_run -> drsa_amd_drsa_any_run (graph-replayed; the cooperative finish at DP = 128)
    equals the explicit loop of drsa_amd_drsa_any_partial and the one-workgroup
    drsa_amd_drsa_any_finish bit for bit; graph and eager runs and two runs are identical."""
    from drsa_slab_ref import explicit_loop
    from drsa_audio_amd.xai.drsa.drsa import drsa_run
    N, steps = N_STEP, 6
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        U_g, t_g = drsa_run(Ag, Cg, Ug, K, steps, use_graph=True)
        U_e, t_e = drsa_run(Ag, Cg, Ug, K, steps, use_graph=False)
        U_2, t_2 = drsa_run(Ag, Cg, Ug, K, steps, use_graph=True)
    torch.cuda.synchronize()
    f, U = explicit_loop(Ag, Cg, Ug, K, steps, natural=True)
    assert torch.isfinite(t_g).all() and torch.isfinite(U_g).all()
    assert torch.equal(t_g, f), (t_g, f)
    assert torch.equal(U_g, U)
    assert torch.equal(U_g, U_e) and torch.equal(t_g, t_e)
    assert torch.equal(U_g, U_2) and torch.equal(t_g, t_2)


@pytest.mark.parametrize("d,K", [(100, 5), (128, 1)])
def test_run_trajectory_vs_reference(d, K):
    """20 steps against the reference's own loop (drsa_ref.run): the gate of
    test_drsa_gpu.test_trajectory_vs_reference_fixture."""
    from drsa_audio_amd.xai.drsa.drsa import drsa_run
    N, steps = N_STEP, 20
    A, C, U0, _, _ = ar.problem(N, d, K)
    U_ref, traj_ref = drsa_ref.run(torch.from_numpy(A), torch.from_numpy(C), torch.from_numpy(U0), K, steps)
    ref = np.asarray(traj_ref, dtype=np.float64)
    Ag, Cg, Ug = _gpu(A, C, U0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        U, traj = drsa_run(Ag, Cg, Ug, K, steps)
    torch.cuda.synchronize()
    traj = traj.cpu().numpy().astype(np.float64)
    assert traj.shape == ref.shape
    dt, du = np.max(np.abs(traj - ref) / np.abs(ref)), (U.cpu() - U_ref).abs().max().item()
    print(f"\nDRSA-ANY-RUN d={d} K={K}: trajectory dev {dt:.3e} (gate 1e-4), U dev {du:.3e} (gate 1e-4), "
          f"f {ref[0]:.6f} -> {ref[-1]:.6f}")
    assert dt < 1e-4
    assert du < 1e-4


# ---------------------------------------------------------------------------------------------
# 5. both geometries at a shape both accept
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(100, 4), (64, 4)])
def test_both_geometries_agree_with_the_oracle(d, K):
    from drsa_audio_amd import _capi
    from drsa_audio_amd.xai.drsa.drsa import DrsaWorkspace, geometry_kind
    assert geometry_kind(d, K) == "padded"
    N = N_STEP
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    st = _capi.stream_ptr(DEV)
    out = {}
    wsp, wsa = DrsaWorkspace(N, d, K, DEV), _any_ws(N, d, K)
    for name, ptr, nbytes in (("drsa_amd_drsa_step", wsp.ptr, wsp.nbytes),
                              ("drsa_amd_drsa_any_step", wsa.data_ptr(), wsa.numel())):
        Un = torch.full_like(Ug, float("nan"))
        f = torch.full((1,), float("nan"), device=DEV)
        _capi.call(name, Ag.data_ptr(), Cg.data_ptr(), N, d, K, Ug.data_ptr(), Un.data_ptr(), f.data_ptr(), ptr, nbytes, st)
        torch.cuda.synchronize()
        out[name] = (float(f), Un.cpu().numpy())
        _check_step(name, out[name][0], out[name][1], N, d, K)


# ---------------------------------------------------------------------------------------------
# 6. two row shards through HipBackend
# ---------------------------------------------------------------------------------------------
def test_two_row_shards_through_hip_backend():
    from drsa_audio_amd.xai.drsa.distributed import HipBackend
    from drsa_audio_amd.xai.drsa.drsa import drsa_step
    d, K, N = 100, 5, N_STEP
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    cut = 1777
    shards = [HipBackend(Ag[sl].contiguous(), Cg[sl].contiguous(), d, K) for sl in (slice(0, cut), slice(cut, N))]
    assert all(b.kind == "natural" and not b.fused_supported() and b.slab_size() == ar.slab_floats(d, K)
               for b in shards)
    gsum = shards[0].partial(Ug) + shards[1].partial(Ug)          # the all-reduce
    U_new, f = shards[0].finish(gsum, N, Ug)
    U_into, f_into = torch.empty_like(Ug), torch.empty(1, device=DEV)
    shards[1].finish_into(gsum, N, Ug, U_into, f_into)
    traj, cnt, U_cnt = torch.zeros(3, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV), torch.empty_like(Ug)
    shards[0].finish_counted(gsum, N, Ug, U_cnt, traj, cnt)
    f_obj = shards[1].objective(gsum, N, Ug)
    U_full, f_full = drsa_step(Ag, Cg, Ug, K)
    torch.cuda.synchronize()
    df, du = abs(float(f) - float(f_full)) / abs(float(f_full)), (U_new - U_full).abs().max().item()
    print(f"\nDRSA-ANY-SHARDS: f dev {df:.3e} (gate 1e-6), U dev {du:.3e} (gate 1e-5)")
    assert df <= 1e-6
    assert du < 1e-5
    assert torch.equal(U_into, U_new) and torch.equal(U_cnt, U_new)
    assert float(f_into) == float(f) == float(f_obj) == float(traj[1]) and int(cnt) == 2


# ---------------------------------------------------------------------------------------------
# 7. the file-writing API
# ---------------------------------------------------------------------------------------------
def test_optimizer_and_main_write_their_files(tmp_path):
    import pandas as pd
    from drsa_audio_amd.xai.drsa.drsa import SubspaceOptimizer, main, objective_fn
    d, K, N = 100, 5, N_STEP
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    p1 = tmp_path / "opt"
    p1.mkdir()
    opt = SubspaceOptimizer(Ug, Ag, Cg, str(p1), num_concepts=K, device="cuda")
    opt.run(steps=3)
    f0 = SubspaceOptimizer.obj_val(Ag, Cg, Ug, objective_fn, K, d // K)
    main(Ag, Cg, str(tmp_path / "main"), num_concepts=K, steps=3, runs=1, device="cuda")
    for path, f_first in ((p1, float(f0)), (tmp_path / "main" / "run1", None)):
        with open(os.path.join(path, "projection_matrix.pkl"), "rb") as fh:
            U = pickle.load(fh)
        assert U.shape == (d, d) and U.dtype == np.float32
        assert _ortho(U, d) < 2e-6
        loss = pd.read_csv(os.path.join(path, "train_stats.csv"))["loss"].to_numpy()
        assert loss.shape == (4,) and np.isfinite(loss).all() and loss[-1] > loss[0]
        if f_first is not None:
            assert abs(loss[0] - f_first) <= 1e-6 * f_first


def test_hip_runner_runs_natural_problems():
    from drsa_audio_amd.xai.drsa.cluster.optsubspaces import hip_runner
    from drsa_audio_amd.xai.drsa.drsa import drsa_run
    d, K, N = 100, 5, 333
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    Up = torch.from_numpy(np.ascontiguousarray(U0[:, ::-1])).to(DEV)
    out = hip_runner([(Ag, Cg, Ug, K), (Ag, Cg, Up, K)], 4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ref = [drsa_run(Ag, Cg, Ug, K, 4), drsa_run(Ag, Cg, Up, K, 4)]
    torch.cuda.synchronize()
    for (U, t), (Ur, tr) in zip(out, ref):
        assert torch.equal(U, Ur) and torch.equal(t, tr)


# ---------------------------------------------------------------------------------------------
# 8. unsupported combinations
# ---------------------------------------------------------------------------------------------
def test_unsupported_combinations_raise_naming_the_shape():
    from drsa_audio_amd import _capi
    from drsa_audio_amd.xai.drsa.distributed import HipBackend
    from drsa_audio_amd.xai.drsa.drsa import DrsaWorkspace, drsa_run, drsa_run_batched, drsa_run_joint, drsa_step
    d, K, N = 100, 5, 333
    A, C, U0, _, _ = ar.problem(N, d, K)
    Ag, Cg, Ug = _gpu(A, C, U0)
    for dt in (torch.bfloat16, torch.float16):
        for fn in (lambda a, c: drsa_run(a, c, Ug, K, 2), lambda a, c: drsa_step(a, c, Ug, K),
                   lambda a, c: HipBackend(a, c, d, K)):
            with pytest.raises(_capi.DrsaAmdError, match="d=100 K=5"):
                fn(Ag.to(dt), Cg.to(dt))
    with pytest.raises(_capi.DrsaAmdError, match="drsa_run_joint.*d=100 K=5"):
        drsa_run_joint([(Ag, Cg, Ug, K)], 2)
    with pytest.raises(_capi.DrsaAmdError, match="drsa_run_batched.*d=100 K=5"):
        drsa_run_batched([(Ag, Cg, Ug, K)], 2)
    with pytest.raises(_capi.DrsaAmdError, match="d=100 K=5"):
        DrsaWorkspace(N, d, K, DEV).coop_status()
    # the padded entry points still refuse the shape
    ws = DrsaWorkspace(N, d, K, DEV)
    with pytest.raises(_capi.DrsaAmdError, match="unsupported d=100 K=5"):
        _capi.call("drsa_amd_drsa_step", Ag.data_ptr(), Cg.data_ptr(), N, d, K, Ug.data_ptr(), Ug.data_ptr(),
                   ws.f.data_ptr(), ws.ptr, ws.nbytes, _capi.stream_ptr(DEV))
