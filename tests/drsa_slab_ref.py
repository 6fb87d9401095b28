"""float64 reference of the DRSA gradient slab (test infrastructure).

The slab is what drsa_amd_drsa_partial{,_bf16,_f16} writes and drsa_amd_drsa_finish reads, and the
all-reduce payload of a sharded run, in the PADDED coordinates of include/drsa_amd.h:

    dk  = d / K                        real concept width
    DKp = next power of two >= dk      (<= 64)
    DP  = next power of two >= max(16, K * DKp)   (<= 128)
    Kp  = DP / DKp                     concept slots: K real ones, then phantoms

    gs[i * DP + k * DKp + l] = Gt[i][k * dk + l]      i < d, k < K, l < dk
    gs[DP * DP + k]          = S[k]                   k < K
    every other entry 0.0 (padded rows and columns, phantom concepts' S slots)

with Gt = A^T (R (.) XC) + C^T (R (.) XA) the unscaled gradient and S_k = sum_n r_nk^2.
"""
import numpy as np

import drsa_ref


# The geometries of tests/test_drsa_partial_matrix_gpu.py as (d, K, DP, DKp): one exact problem per
# instantiated (DP, DKp) pair, padded problems with d % 4 == 0 (float4 staging), and d % 4 != 0
# (the scalar staging branch).  (40, 5) has phantom concepts (Kp = 8 > K), as have all with DP > K DKp.
EXACT = [(DP, DP // w, DP, w) for DP in (16, 32, 64, 128) for w in (1, 2, 4, 8, 16, 32, 64) if w <= min(DP, 64)]
PADDED = [(12, 3, 16, 4), (24, 3, 32, 8), (20, 5, 32, 4), (48, 4, 64, 16), (40, 5, 64, 8), (36, 1, 64, 64),
          (100, 4, 128, 32), (96, 6, 128, 16), (100, 25, 128, 4), (72, 9, 128, 8), (100, 2, 128, 64)]
UNVEC = [(6, 2, 16, 4), (5, 1, 16, 8), (18, 2, 32, 16), (30, 5, 64, 8), (35, 5, 64, 8), (42, 3, 64, 16),
         (50, 2, 64, 32), (33, 1, 64, 64), (66, 2, 128, 64), (90, 6, 128, 16), (70, 5, 128, 16), (126, 2, 128, 64)]
GEOMETRIES = EXACT + PADDED + UNVEC


def _pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def geom(d, K):
    """(dk, DKp, DP, Kp) of a supported problem; ValueError for what the library rejects."""
    d, K = int(d), int(K)
    if d <= 0 or d > 128 or K <= 0 or d % K:
        raise ValueError(f"unsupported DRSA problem d={d} K={K}: need 0 < d <= 128 and K | d")
    dk = d // K
    DKp = _pow2ceil(dk)
    if DKp > 64:
        raise ValueError(f"unsupported DRSA problem d={d} K={K}: padded concept width {DKp} > 64")
    DP = _pow2ceil(max(16, K * DKp))
    if DP > 128:
        raise ValueError(f"unsupported DRSA problem d={d} K={K}: K * padded width = {K * DKp} > 128")
    return dk, DKp, DP, DP // DKp


def slab_floats(d, K):
    _, _, DP, Kp = geom(d, K)
    return DP * DP + Kp


def slab(A, C, U, K, rounder=None):
    """(Gt [d, d], S [K]) in float64.  A and C enter as they are (the 16-bit callers pass them
    already rounded); U is rounded with `rounder` for the projections XA = A U', XC = C U' and
    enters nowhere else."""
    A = np.asarray(A, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    Up = np.asarray(rounder(U) if rounder is not None else U, dtype=np.float64)
    N, d = A.shape
    dk = d // K
    XA, XC = A @ Up, C @ Up
    r = np.maximum((XA * XC).reshape(N, K, dk).sum(-1), 0.0)
    S = (r * r).sum(0)
    R = np.repeat(r, dk, axis=1)
    Gt = A.T @ (R * XC) + C.T @ (R * XA)
    return Gt, S


def _real_index(d, K):
    """Slab positions of Gt (as [d, d]) and of S (as [K])."""
    dk, DKp, DP, _ = geom(d, K)
    j = np.arange(d)
    jp = (j // dk) * DKp + j % dk
    return np.arange(d)[:, None] * DP + jp[None, :], DP * DP + np.arange(K)


def embed(Gt, S, d, K):
    """float64 [DP * DP + Kp] slab holding Gt and S, zeros elsewhere."""
    gi, si = _real_index(d, K)
    gs = np.zeros(slab_floats(d, K), dtype=np.float64)
    gs[gi] = np.asarray(Gt, dtype=np.float64)
    gs[si] = np.asarray(S, dtype=np.float64)
    return gs


def unembed(gs, d, K):
    """Inverse of embed: (Gt [d, d], S [K], pad) with pad the boolean mask, over the whole slab,
    of the entries that hold neither."""
    gs = np.asarray(gs)
    assert gs.shape == (slab_floats(d, K),), (gs.shape, d, K)
    gi, si = _real_index(d, K)
    pad = np.ones(gs.shape, dtype=bool)
    pad[gi] = False
    pad[si] = False
    return gs[gi].astype(np.float64), gs[si].astype(np.float64), pad


def gradient(gs, N, d, K):
    """(f, G [d, d]) from a slab over N rows: M = sqrt(S / N), f = (mean sqrt M)^2,
    c = sqrt(f) / (K N M^1.5) (0 where M = 0), G = Gt diag(c per column)."""
    Gt, S, _ = unembed(gs, d, K)
    M = np.sqrt(S / float(N))
    f = float(np.mean(np.sqrt(M)) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(M > 0, np.sqrt(f) / (K * float(N) * M ** 1.5), 0.0)
    return f, Gt * np.repeat(c, d // K)[None, :]


def finish(gs, N, U, K):
    """(f, U_new) as drsa_amd_drsa_finish defines them: U_new = polar(U + G)."""
    U = np.asarray(U, dtype=np.float64)
    f, G = gradient(gs, N, U.shape[0], K)
    return f, drsa_ref.polar(U + G)


# ---------------------------------------------------------------------------------------------
# The kernels' side, shared by the GPU tests (torch and the library are imported on use only).
# ---------------------------------------------------------------------------------------------
ENTRY = {"fp32": "drsa_amd_drsa_partial", "bf16": "drsa_amd_drsa_partial_bf16", "f16": "drsa_amd_drsa_partial_f16"}
ROUNDER = {"fp32": None, "bf16": drsa_ref.bf16_round, "f16": drsa_ref.f16_round}


def u0(d, seed):
    """A QR-orthogonal float32 start."""
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0].astype(np.float32)


def partial_rc(dt, A, C, U0, K, poison=float("nan")):
    """One call of the `dt` partial entry point on A, C (float32 arrays holding values of that
    type) at U0, gs of exactly slab_floats(d, K) floats pre-filled with `poison`.  Returns the
    entry point's return code and the slab as float64."""
    import torch
    from drsa_audio_amd import _capi
    from drsa_audio_amd.xai.drsa.drsa import DrsaWorkspace
    dev = torch.device("cuda")
    tdt = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]
    N, d = A.shape
    At = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(dev).to(tdt)   # exact: already rounded
    Ct = torch.from_numpy(np.ascontiguousarray(C, dtype=np.float32)).to(dev).to(tdt)
    Ut = torch.from_numpy(np.ascontiguousarray(U0, dtype=np.float32)).to(dev)
    ws = DrsaWorkspace(N, d, K, dev)
    gs = torch.full((slab_floats(d, K),), poison, dtype=torch.float32, device=dev)
    rc = getattr(_capi.lib(), ENTRY[dt])(At.data_ptr(), Ct.data_ptr(), N, d, K, Ut.data_ptr(), gs.data_ptr(), ws.ptr,
                                         ws.nbytes, _capi.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, gs.cpu().numpy().astype(np.float64)


def check_slab(gs, Gt, S, d, K, tag=""):
    """The gates of a kernel slab against the float64 (Gt, S): real Gt entries within 2e-5 of
    max|Gt|, real S within rtol 2e-5 / atol 1e-6 max S, every other entry exactly 0.0.  Prints the
    deviations before it asserts and returns them (Gt relative to max|Gt|, S relative)."""
    Gk, Sk, pad = unembed(gs, d, K)
    dev_g = float(np.abs(Gk - Gt).max() / np.abs(Gt).max())
    dev_s = float((np.abs(Sk - S) / S).max()) if (S > 0).all() else float("nan")
    nonzero_pad = int(np.count_nonzero(gs[pad] != 0.0))      # NaN counts: an entry never written
    print(f"\nDRSA-SLAB {tag} d={d} K={K}: Gt dev {dev_g:.3e} (gate 2e-5), S dev {dev_s:.3e} (gate 2e-5), "
          f"padding entries != 0: {nonzero_pad} of {int(pad.sum())}")
    assert np.isfinite(Gk).all() and np.isfinite(Sk).all()
    assert np.abs(Gk - Gt).max() <= 2e-5 * np.abs(Gt).max()
    np.testing.assert_allclose(Sk, S, rtol=2e-5, atol=1e-6 * S.max())
    assert nonzero_pad == 0
    return dev_g, dev_s


def explicit_loop(Ag, Cg, Ug, K, steps, natural=False, want_iters=False):
    """The optimiser spelt out on the current stream: per step one call of the partial entry point and
    one of the ONE-WORKGROUP finish (drsa_amd_drsa_partial + drsa_amd_drsa_finish, or their
    drsa_amd_drsa_any_* namesakes with natural=True), then the objective at the last U.  This is what
    drsa_run / _run_joint / _run_batched (fused step, cooperative finish, batched finish) must equal
    bit for bit.  Returns (f [steps + 1], U_S) as device tensors, synchronised; with want_iters also a
    dict: "iters" (iters_out of every step's polar), "gs0" (the reduced slab of step 0, float32
    numpy) and "U1" (U after step 0)."""
    import torch
    from drsa_audio_amd import _capi
    from drsa_audio_amd.xai.drsa.drsa import DrsaWorkspace
    dev = Ag.device
    N, d = Ag.shape
    pre = "drsa_amd_drsa_any_" if natural else "drsa_amd_drsa_"
    if natural:
        nbytes = _capi.lib().drsa_amd_drsa_any_workspace_bytes(N, d, K)
        assert nbytes > 0
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ws_ptr, ws_bytes = buf.data_ptr(), buf.numel()
        gs = torch.empty(_capi.lib().drsa_amd_drsa_any_slab_floats(d, K), device=dev)
    else:
        ws = DrsaWorkspace(N, d, K, dev)
        ws_ptr, ws_bytes, gs = ws.ptr, ws.nbytes, ws.gs
    st = _capi.stream_ptr(dev)
    f = torch.empty(steps + 1, device=dev)
    its = torch.full((steps + 1,), -1, dtype=torch.int32, device=dev)
    extra = {}
    U = Ug.clone()
    for t in range(steps + 1):
        _capi.call(pre + "partial", Ag.data_ptr(), Cg.data_ptr(), N, d, K, U.data_ptr(), gs.data_ptr(), ws_ptr,
                   ws_bytes, st)
        if t == 0 and want_iters:
            extra["gs0"] = gs.clone()
        U_new = torch.empty_like(U)
        _capi.call(pre + "finish", gs.data_ptr(), N, d, K, U.data_ptr(), U_new.data_ptr(), f[t:].data_ptr(),
                   1 if t == steps else 0, its[t:].data_ptr() if want_iters and t < steps else None, st)
        if t < steps:
            U = U_new
            if t == 0 and want_iters:
                extra["U1"] = U_new
    torch.cuda.synchronize()
    if not want_iters:
        return f, U
    extra["iters"] = [int(v) for v in its[:steps].cpu()]
    extra["gs0"] = extra["gs0"].cpu().numpy()
    return f, U, extra
