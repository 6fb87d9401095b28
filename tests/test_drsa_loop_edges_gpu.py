"""Edges of the DRSA step loop (GPU): steps < 2 (no graph is opened), the odd tail step, steps = 0.

For steps in (0, 1, 2, 3, 5) every run entry point (drsa_run on the fused path, on the one-workgroup
finish and on the cooperative finish; drsa_run_joint; drsa_run_batched through the grouped and the
leaf-wise partial) is run with use_graph=True and use_graph=False on a non-default stream:

* U_S and the whole trajectory [steps + 1] are bit-identical between the two, every entry finite;
* traj[steps] is bit-equal to drsa_objective(A, C, U_S, K);
* in fp32 the joint and the batched results are bit-equal to drsa_run on each problem alone.

Everything is compared bit for bit (every path sums in one fixed order), so there is no tolerance."""
import functools

import numpy as np
import pytest
import torch

from gen_fixtures import drsa_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
STEPS = (0, 1, 2, 3, 5)
FUSED, ONE_WG, COOP = (777, 64, 4), (100, 32, 2), (2048, 128, 16)


@functools.lru_cache(maxsize=None)
def _side():
    return torch.cuda.Stream()


@functools.lru_cache(maxsize=None)
def _problem(N, d, K, seed, dtype=torch.float32):
    A, C = drsa_inputs(N, d, seed)
    U0 = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0].astype(np.float32)
    A, C, U0 = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV) for v in (A, C, U0))
    torch.cuda.synchronize()
    return A.to(dtype), C.to(dtype), U0, K


@functools.lru_cache(maxsize=None)
def _alone(N, d, K, seed, steps):
    """drsa_run of one fp32 problem on its own (the reference of the joint and batched runs)."""
    from drsa_audio_amd.xai.drsa.drsa import drsa_run
    with torch.cuda.stream(_side()):
        U, t = drsa_run(*_problem(N, d, K, seed), steps)
    torch.cuda.synchronize()
    return U, t


def _graph_and_eager(run):
    """run(use_graph) -> [(U, traj)] for both modes on the side stream."""
    with torch.cuda.stream(_side()):
        g, e = run(True), run(False)
    torch.cuda.synchronize()
    return g, e


def _check_pairs(graph, eager, steps):
    assert len(graph) == len(eager)
    for (Ug, tg), (Ue, te) in zip(graph, eager):
        assert tg.shape == (steps + 1,) and te.shape == (steps + 1,)
        assert torch.isfinite(tg).all() and torch.isfinite(te).all() and torch.isfinite(Ug).all()
        assert torch.equal(tg, te), (tg, te)
        assert torch.equal(Ug, Ue)


def _check_final_objective(probs, outs, steps):
    from drsa_audio_amd.xai.drsa.drsa import drsa_objective
    with torch.cuda.stream(_side()):
        fs = [drsa_objective(A, C, U, K) for (A, C, _, K), (U, _) in zip(probs, outs)]
    torch.cuda.synchronize()
    for f, (_, t) in zip(fs, outs):
        assert torch.equal(t[steps], f), (t, f)


def _check_equals_alone(specs, outs, steps):
    for spec, (U, t) in zip(specs, outs):
        Ua, ta = _alone(*spec, steps)
        assert torch.equal(t, ta), (spec, t, ta)
        assert torch.equal(U, Ua), spec


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("N,d,K", [FUSED, ONE_WG, COOP])
def test_run_loop_edges(N, d, K, steps):
    from drsa_audio_amd.xai.drsa.drsa import drsa_run
    prob = _problem(N, d, K, 11)
    g, e = _graph_and_eager(lambda ug: [drsa_run(*prob, steps, use_graph=ug)])
    _check_pairs(g, e, steps)
    _check_final_objective([prob], g, steps)
    if steps == 0:
        assert torch.equal(g[0][0], prob[2])


JOINT = [FUSED + (21,), COOP + (22,)]


@pytest.mark.parametrize("steps", STEPS)
def test_joint_loop_edges_fp32(steps):
    from drsa_audio_amd.xai.drsa.drsa import drsa_run_joint
    probs = [_problem(*spec) for spec in JOINT]
    g, e = _graph_and_eager(lambda ug: drsa_run_joint(probs, steps, use_graph=ug))
    _check_pairs(g, e, steps)
    _check_final_objective(probs, g, steps)
    _check_equals_alone(JOINT, g, steps)


def test_joint_odd_tail_captured_in_caller_graph_equals_eager():
    """test_joint_run_captured_in_caller_graph_equals_eager at steps = 3 (one pair and the odd tail),
    mixed geometry."""
    from drsa_audio_amd.xai.drsa.drsa import drsa_run_joint
    steps = 3
    probs = [_problem(*spec) for spec in JOINT]
    side = _side()
    with torch.cuda.stream(side):
        ref = drsa_run_joint(probs, steps)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        out = drsa_run_joint(probs, steps)
    for _ in range(2):
        with torch.cuda.stream(side):
            cg.replay()
        torch.cuda.synchronize()
        for (U, t), (Ur, tr) in zip(out, ref):
            assert torch.isfinite(t).all()
            assert torch.equal(t, tr) and torch.equal(U, Ur)


@pytest.mark.parametrize("steps", STEPS)
def test_joint_loop_edges_bf16(steps):
    """16-bit A, C: the graph run against the eager run only."""
    from drsa_audio_amd.xai.drsa.drsa import drsa_run_joint
    probs = [_problem(*spec, torch.bfloat16) for spec in JOINT]
    g, e = _graph_and_eager(lambda ug: drsa_run_joint(probs, steps, use_graph=ug))
    _check_pairs(g, e, steps)


BATCHED = {"grouped": [(300, 32, 4, 31 + j) for j in range(3)],      # drsa_partial_grouped_kernel
           "leafwise": [(300, 128, 2, 41 + j) for j in range(2)]}    # concept width 64: the per-leaf kernel


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("kind", sorted(BATCHED))
def test_batched_loop_edges(kind, blocks, steps):
    from drsa_audio_amd.xai.drsa.drsa import drsa_run_batched
    specs = BATCHED[kind]
    probs = [_problem(*spec) for spec in specs]
    g, e = _graph_and_eager(lambda ug: drsa_run_batched(probs, steps, blocks=blocks, use_graph=ug))
    _check_pairs(g, e, steps)
    _check_final_objective(probs, g, steps)
    _check_equals_alone(specs, g, steps)
