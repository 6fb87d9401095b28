"""The natural DRSA geometry (drsa_amd_drsa_any_*: every K | d at d <= 128) without a GPU: the
host queries, geometry_kind, argument errors (checked before any device work), what the GPU
tests' gates can and cannot see (float64 numpy), and hip_runner's routing."""
import ctypes

import numpy as np
import pytest
import torch

import drsa_any_ref as ar
import drsa_slab_ref as sr


def _lib():
    from drsa_audio_amd import _capi
    return _capi.load()


def test_host_queries_over_every_shape():
    lib = _lib()
    for d in range(1, 131):
        for K in range(1, d + 2):
            ok = d <= 128 and d % K == 0
            assert lib.drsa_amd_drsa_any_supported(d, K) == int(ok), (d, K)
            assert lib.drsa_amd_drsa_any_slab_floats(d, K) == (ar.dp_of(d) ** 2 + K if ok else 0), (d, K)
            assert (lib.drsa_amd_drsa_any_workspace_bytes(100, d, K) > 0) == ok, (d, K)
    for d, K in [(0, 1), (-4, 2), (16, 0), (16, -2)]:
        assert lib.drsa_amd_drsa_any_supported(d, K) == 0
        assert lib.drsa_amd_drsa_any_slab_floats(d, K) == 0
        assert lib.drsa_amd_drsa_any_workspace_bytes(100, d, K) == 0
    assert lib.drsa_amd_drsa_any_workspace_bytes(0, 100, 5) == 0
    # the padded queries still refuse what they refused
    assert lib.drsa_amd_drsa_slab_floats(100, 5) == 0 and lib.drsa_amd_drsa_workspace_bytes(100, 128, 1) == 0


def test_geometry_kind():
    from drsa_audio_amd import _capi
    from drsa_audio_amd.xai.drsa.drsa import geometry_kind, slab_floats
    lib = _lib()
    for d in range(1, 129):
        for K in range(1, d + 1):
            if d % K:
                continue
            padded = lib.drsa_amd_drsa_slab_floats(d, K) > 0
            assert geometry_kind(d, K) == ("padded" if padded else "natural"), (d, K)
    for d, K in ar.NATURAL_ONLY:
        assert geometry_kind(d, K) == "natural"
        assert slab_floats(d, K) == ar.slab_floats(d, K) == lib.drsa_amd_drsa_any_slab_floats(d, K)
    assert geometry_kind(100, 4) == "padded" and slab_floats(100, 4) == 128 * 128 + 4
    for d, K in [(129, 1), (100, 3), (0, 1), (256, 4)]:
        with pytest.raises(_capi.DrsaAmdError, match=f"d={d} K={K}"):
            geometry_kind(d, K)


# fake device addresses: every call below fails its argument check, before anything is dereferenced
P, Q, R_, S_ = 0x10000, 0x20000, 0x30000, 0x40000
BIG = 1 << 30


def _calls(N, d, K, A=P, C=Q, U=R_, U_out=S_, ws=0x50000, ws_size=BIG, out=0x60000, cnt=0x70000):
    """name -> argument tuple of every compute entry point, one knob per error case."""
    return {
        "drsa_amd_drsa_any_partial": (A, C, N, d, K, U, out, ws, ws_size, None),
        "drsa_amd_drsa_any_finish": (out, N, d, K, U, U_out, 0x80000, 0, None, None),
        "drsa_amd_drsa_any_finish_counted": (out, N, d, K, U, U_out, 0x80000, cnt, None),
        "drsa_amd_drsa_any_step": (A, C, N, d, K, U, U_out, 0x80000, ws, ws_size, None),
        "drsa_amd_drsa_any_objective": (A, C, N, d, K, U, 0x80000, ws, ws_size, None),
        "drsa_amd_drsa_any_run": (A, C, N, d, K, U, U_out, 4, 0x80000, cnt, ws, ws_size, 0, None),
    }


def _expect(name, args, code, *needles):
    from drsa_audio_amd import _capi
    lib = _lib()
    rc = getattr(lib, name)(*args)
    msg = lib.drsa_amd_last_error().decode()
    assert rc == code, (name, rc, msg)
    assert name.replace("drsa_amd_", "") in msg, (name, msg)
    for n in needles:
        assert n in msg, (name, n, msg)
    assert code in (_capi.DRSA_EINVAL, _capi.DRSA_EUNSUPPORTED)


ALL = ["drsa_amd_drsa_any_partial", "drsa_amd_drsa_any_finish", "drsa_amd_drsa_any_finish_counted",
       "drsa_amd_drsa_any_step", "drsa_amd_drsa_any_objective", "drsa_amd_drsa_any_run"]
WITH_ROWS = [n for n in ALL if "finish" not in n]       # take A, C and a workspace


@pytest.mark.parametrize("name", ALL)
def test_unsupported_shapes_name_entry_d_and_K(name):
    from drsa_audio_amd import _capi
    for d, K in [(129, 1), (100, 3), (100, 0), (0, 1)]:
        _expect(name, _calls(100, d, K)[name], _capi.DRSA_EUNSUPPORTED, f"d={d} K={K}")


@pytest.mark.parametrize("name", ALL)
def test_argument_errors_without_a_device(name):
    from drsa_audio_amd import _capi
    E = _capi.DRSA_EINVAL
    d, K, N = 100, 5, 100
    _expect(name, _calls(-1, d, K)[name], E, "N must be")
    if name != "drsa_amd_drsa_any_partial":                      # the partial alone takes N = 0
        _expect(name, _calls(0, d, K)[name], E, "N must be")
    if name in WITH_ROWS:
        need = _lib().drsa_amd_drsa_any_workspace_bytes(N, d, K)
        _expect(name, _calls(N, d, K, ws_size=need - 1)[name], E, "workspace too small")
        _expect(name, _calls(N, d, K, ws=None)[name], E, "workspace too small")
        _expect(name, _calls(N, d, K, A=P + 4)[name], E, "16B aligned")
        _expect(name, _calls(N, d, K, C=Q + 8)[name], E, "16B aligned")
        _expect(name, _calls(N, d, K, A=None)[name], E, "null pointer")
        _expect(name, _calls(N, d, K, C=None)[name], E, "null pointer")
    if name not in ("drsa_amd_drsa_any_partial", "drsa_amd_drsa_any_objective"):
        _expect(name, _calls(N, d, K, U_out=R_)[name], E, "must not alias")
        _expect(name, _calls(N, d, K, U_out=None)[name], E, "null pointer")
    _expect(name, _calls(N, d, K, U=None)[name], E, "null pointer")
    if name == "drsa_amd_drsa_any_run":
        a = list(_calls(N, d, K)[name])
        a[7] = -1
        _expect(name, tuple(a), E, "steps < 0")


# ---------------------------------------------------------------------------------------------
# What the GPU gates can see, in float64 numpy at the partial test's shapes: a plain fp32
# evaluation stays inside them; a 16-row block left out, or the concept boundaries moved by one
# column, lands far outside (> 10 gates).
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K,N", ar.PARTIAL_SHAPES)
def test_gates_separate_right_from_wrong(d, K, N):
    A, C, U0, Gt, S = ar.problem(N, d, K)
    dk = d // K
    true_map = np.arange(d) // dk
    G2, S2 = ar.slab_by_map(A, C, U0, true_map, K)
    assert np.abs(G2 - Gt).max() <= 1e-12 * np.abs(Gt).max() and np.allclose(S2, S, rtol=1e-12, atol=0)
    # fp32 evaluation: inside the gates
    eg, es = ar.slab_errors(*ar.slab_by_map(A, C, U0, true_map, K, dtype=np.float32), Gt, S)
    print(f"\nfp32 numpy d={d} K={K} N={N}: Gt {eg:.3f} gates, S {es:.3f} gates")
    assert eg <= 1.0 and es <= 1.0
    # one 16-row block dropped (the second of the leaf that has two, else the first block)
    lo = 16 if N > 32 else 0
    keep = np.r_[0:lo, min(lo + 16, N):N]
    Gd, Sd = sr.slab(A[keep], C[keep], U0, K) if keep.size else (np.zeros_like(Gt), np.zeros_like(S))
    eg, es = ar.slab_errors(Gd, Sd, Gt, S)
    print(f"dropped block: Gt {eg:.1f} gates, S {es:.1f} gates")
    assert eg > 10.0
    # boundaries one column early (cyclic): only where there is a boundary
    if K > 1:
        eg, es = ar.slab_errors(*ar.slab_by_map(A, C, U0, ((np.arange(d) + 1) // dk) % K, K), Gt, S)
        print(f"shifted boundaries: Gt {eg:.1f} gates, S {es:.1f} gates")
        assert eg > 10.0 and es > 10.0


def test_embed_roundtrip_and_padding():
    rng = np.random.default_rng(0)
    for d, K in [(100, 5), (65, 1), (24, 3), (128, 1), (7, 7)]:
        Gt, S = rng.standard_normal((d, d)), rng.random(K)
        gs = ar.embed(Gt, S, d, K)
        assert gs.shape == (ar.slab_floats(d, K),)
        G2, S2, pad = ar.unembed(gs, d, K)
        assert np.array_equal(G2, Gt) and np.array_equal(S2, S) and not pad.any()
        assert pad.size == ar.dp_of(d) ** 2 - d * d


# ---------------------------------------------------------------------------------------------
# hip_runner's routing, drsa_run / drsa_run_batched / drsa_run_joint stubbed
# ---------------------------------------------------------------------------------------------
def test_route_problems_sends_natural_problems_through_drsa_run(monkeypatch):
    from drsa_audio_amd.xai.drsa import drsa as D
    from drsa_audio_amd.xai.drsa.cluster.optsubspaces import route_problems
    log = []

    def prob(d, K, tag, dtype=torch.float32):
        return (torch.zeros(8, d, dtype=dtype), torch.zeros(8, d, dtype=dtype), tag, K)

    monkeypatch.setattr(D, "drsa_run", lambda A, C, U0, K, steps: (log.append(("run", U0, steps)), ("run", U0))[1])
    monkeypatch.setattr(D, "drsa_run_batched",
                        lambda ps, steps: (log.append(("batched", [p[2] for p in ps], steps)), [("batched", p[2]) for p in ps])[1])
    monkeypatch.setattr(D, "drsa_run_joint",
                        lambda ps, steps: (log.append(("joint", [p[2] for p in ps], steps)), [("joint", p[2]) for p in ps])[1])
    # all natural: one after another, in task order
    out = route_problems([prob(100, 5, "a"), prob(100, 5, "b"), prob(128, 1, "c")], 7)
    assert out == [("run", "a"), ("run", "b"), ("run", "c")]
    assert log == [("run", "a", 7), ("run", "b", 7), ("run", "c", 7)]
    # padded problems take today's calls
    log.clear()
    assert route_problems([prob(100, 4, "a"), prob(128, 4, "b")], 3) == [("batched", "a"), ("batched", "b")]
    assert route_problems([prob(100, 4, "a"), prob(64, 4, "b")], 3) == [("joint", "a"), ("joint", "b")]
    assert route_problems([prob(100, 4, "a", torch.bfloat16)], 3) == [("joint", "a")]
    assert [e[0] for e in log] == ["batched", "joint", "joint"]
    # mixed: results in the order of the problems
    log.clear()
    out = route_problems([prob(100, 4, "p0"), prob(100, 5, "n0"), prob(100, 4, "p1"), prob(100, 20, "n1")], 2)
    assert out == [("batched", "p0"), ("run", "n0"), ("batched", "p1"), ("run", "n1")]
    assert log == [("run", "n0", 2), ("run", "n1", 2), ("batched", ["p0", "p1"], 2)]
