"""PRCA without a GPU: the float32 model that sizes the GPU tolerances passes its own gates, the C ABI
checks its arguments before any device work, the two new ops have meta kernels and no CPU kernel."""
import ctypes
import os
import re

import pytest
import torch

import prca_ref as R
from conftest import ROOT
from drsa_audio_amd import _capi

NEW_SYMBOLS = ["drsa_amd_prca_workspace_bytes", "drsa_amd_prca_partial", "drsa_amd_prca_finish",
               "drsa_amd_syevj_workspace_bytes", "drsa_amd_syevj"]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("d", [3, 17, 64, 100, 128])
def test_model_passes_its_own_gates(family, d):
    M, err, sweeps = R.model_case(family, d)
    print(family, d, sweeps, err)
    assert err["orth"] < 5e-6
    assert sweeps < R.MAX_SWEEPS                  # ended on a sweep without a rotation, not at the cap
    # the allowance rule needs a model that is itself accurate: a loose model would license a loose kernel
    assert err["eig"] < 4e-6 and err["res"] < 4e-6


def test_model_known_answers():
    import numpy as np
    w, V, sweeps = R.jacobi_model_fp32(np.diag(np.arange(-3.0, 5.0)).astype(np.float32))
    assert sweeps == 1 and np.array_equal(w, np.arange(4.0, -4.0, -1.0)) and np.array_equal(np.abs(V).sum(0), np.ones(8))
    w, V, _ = R.jacobi_model_fp32(np.array([[0.0, 1.0], [1.0, 0.0]], dtype=np.float32))
    assert np.allclose(w, [1.0, -1.0], atol=R.FLOOR)
    for m in (2, 4, 8, 128):                      # the round robin meets every pair once per sweep
        seen = set()
        for s in range(m - 1):
            p, q = R.round_robin_pairs(m, s)
            assert len(set(p) | set(q)) == m and bool((p < q).all())
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2


def test_new_symbols_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "drsa_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name


def test_c_abi_argument_validation_without_gpu():
    lib = _capi.load()
    P = ctypes.c_void_p
    buf = (ctypes.c_float * 16)()
    ib = (ctypes.c_int * 4)()
    p, q = ctypes.cast(buf, P).value, ctypes.cast(ib, P).value
    E = _capi
    err = lib.drsa_amd_last_error
    # workspace queries
    assert lib.drsa_amd_prca_workspace_bytes(100, 129) == 0
    assert lib.drsa_amd_prca_workspace_bytes(0, 64) == 0 and lib.drsa_amd_prca_workspace_bytes(100, 0) == 0
    assert lib.drsa_amd_prca_workspace_bytes(100, 128) == 7 * 128 * 128 * 4        # ceil(100 / 16) leaves
    assert lib.drsa_amd_prca_workspace_bytes(160000, 100) == 256 * 128 * 128 * 4   # the fixed 256 leaves
    assert lib.drsa_amd_prca_workspace_bytes(1, 1) == 32 * 32 * 4
    assert lib.drsa_amd_syevj_workspace_bytes(129) == 0 and lib.drsa_amd_syevj_workspace_bytes(0) == 0
    assert lib.drsa_amd_syevj_workspace_bytes(128) > 0
    big = 1 << 30
    # partial
    assert lib.drsa_amd_prca_partial(None, p, 10, 4, p, p, big, None) == E.DRSA_EINVAL and b"A or C" in err()
    assert lib.drsa_amd_prca_partial(p, None, 10, 4, p, p, big, None) == E.DRSA_EINVAL
    assert lib.drsa_amd_prca_partial(p, p, 10, 4, None, p, big, None) == E.DRSA_EINVAL and b"slab" in err()
    assert lib.drsa_amd_prca_partial(p, p, 10, 4, p, None, big, None) == E.DRSA_EINVAL and b"ws" in err()
    assert lib.drsa_amd_prca_partial(p, p, 0, 4, p, p, big, None) == E.DRSA_EINVAL and b"N=0" in err()
    assert lib.drsa_amd_prca_partial(p, p, 10, 0, p, p, big, None) == E.DRSA_EINVAL and b"d=0" in err()
    assert lib.drsa_amd_prca_partial(p, p, 10, 129, p, p, big, None) == E.DRSA_EUNSUPPORTED and b"d=129" in err()
    need = lib.drsa_amd_prca_workspace_bytes(10, 4)
    assert lib.drsa_amd_prca_partial(p, p, 10, 4, p, p, need - 1, None) == E.DRSA_EWORKSPACE and b"ws_bytes" in err()
    # finish
    assert lib.drsa_amd_prca_finish(None, 10, 4, p, None) == E.DRSA_EINVAL and b"slab or M_out" in err()
    assert lib.drsa_amd_prca_finish(p, 10, 4, None, None) == E.DRSA_EINVAL
    assert lib.drsa_amd_prca_finish(p, 0, 4, p, None) == E.DRSA_EINVAL and b"N_total=0" in err()
    assert lib.drsa_amd_prca_finish(p, 10, -1, p, None) == E.DRSA_EINVAL and b"d=-1" in err()
    assert lib.drsa_amd_prca_finish(p, 10, 129, p, None) == E.DRSA_EUNSUPPORTED
    # syevj
    assert lib.drsa_amd_syevj(None, 4, p, p, q, q, 16, None) == E.DRSA_EINVAL and b"(M)" in err()
    assert lib.drsa_amd_syevj(p, 4, None, p, q, q, 16, None) == E.DRSA_EINVAL and b"w_out or V_out" in err()
    assert lib.drsa_amd_syevj(p, 4, p, None, q, q, 16, None) == E.DRSA_EINVAL
    assert lib.drsa_amd_syevj(p, 0, p, p, q, q, 16, None) == E.DRSA_EINVAL and b"d=0" in err()
    assert lib.drsa_amd_syevj(p, 129, p, p, q, q, 16, None) == E.DRSA_EUNSUPPORTED and b"d=129" in err()
    assert lib.drsa_amd_syevj(p, 4, p, p, None, None, 16, None) == E.DRSA_EINVAL and b"ws" in err()
    assert lib.drsa_amd_syevj(p, 4, p, p, None, q, lib.drsa_amd_syevj_workspace_bytes(4) - 1,
                              None) == E.DRSA_EWORKSPACE and b"ws_bytes" in err()


def test_meta_shapes_of_the_new_ops():
    import drsa_audio_amd.ops as dops
    assert "prca_covariance" in dops.__all__ and "syevj" in dops.__all__
    o = torch.ops.drsa_amd
    A = torch.empty(37, 100, device="meta")
    M = o.prca_covariance(A, A)
    assert M.shape == (100, 100) and M.dtype == torch.float32
    w, V = o.syevj(M)
    assert w.shape == (100,) and V.shape == (100, 100) and V.dtype == torch.float32


def test_cpu_tensors_refused():
    import drsa_audio_amd.ops  # noqa: F401  (registers the ops)
    from drsa_audio_amd.xai.drsa import prca
    with pytest.raises(RuntimeError):
        torch.ops.drsa_amd.syevj(torch.eye(8))
    with pytest.raises(RuntimeError):
        torch.ops.drsa_amd.prca_covariance(torch.rand(10, 8), torch.rand(10, 8))
    A = torch.rand(10, 8)
    with pytest.raises(_capi.DrsaAmdError):
        prca.prca(A, A)
    with pytest.raises(_capi.DrsaAmdError):
        prca.relevance_covariance(A, A)
    with pytest.raises(_capi.DrsaAmdError):
        prca.eigh_descending(torch.eye(8))
    with pytest.raises(_capi.DrsaAmdError):
        prca.relevance_covariance_finish(torch.eye(8), 10)
