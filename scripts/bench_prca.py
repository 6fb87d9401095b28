"""Times the two PRCA steps (xai/drsa/prca.py, csrc/prca.hip) next to their baselines, HIP events (or a
host clock around a synchronise where the baseline crosses to the host), 20 timed repeats after
warm-up, the two versions alternating in one process:

    covariance  N = 160 000, d = 128 (C4's rows): prca.relevance_covariance against the torch
                expression (A.T @ C + C.T @ A) / (2N) on the same GPU; GB/s of the algorithmic
                bytes (A and C read once, M written) against the 8 TB/s HBM figure.
    syevj       d in {64, 100, 128}: prca.eigh_descending against the host path the reference's
                style implies (D2H, numpy float64 eigh, H2D), on a PRCA-like matrix.

    python scripts/bench_prca.py             # both steps, each a child process under its own timeout
    python scripts/bench_prca.py cov|syevj   # one step

Prints one JSON line per step.  Nothing is gated on these times.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
REPEATS, WARMUP = 20, 3
STEP_TIMEOUT = {"cov": 240, "syevj": 240}
HBM_PEAK = 8.0e12


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def _alternate(fns, host_clock=False):
    """Each fn timed REPEATS times, the fns taking turns, after WARMUP rounds of all of them."""
    import torch
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            if host_clock:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
    return {k: _stats(v) for k, v in times.items()}


def _rows(N, d):
    import torch
    from drsa_audio_amd.utils.synthetic import drsa_inputs
    return tuple(torch.from_numpy(v).cuda() for v in drsa_inputs(N, d, seed=1))


def cov_step():
    import torch
    from drsa_audio_amd.xai.drsa import prca
    N, d = 160000, 128
    A, C = _rows(N, d)
    out = {"step": "cov", "N": N, "d": d}
    out.update(_alternate({"hip": lambda: prca.relevance_covariance(A, C),
                           "torch": lambda: (A.T @ C + C.T @ A) / (2 * N)}))
    Mh = prca.relevance_covariance(A, C).double()
    Mt = ((A.T @ C + C.T @ A) / (2 * N)).double()
    M64 = (A.double().T @ C.double() + C.double().T @ A.double()) / (2 * N)
    S = (A.double().abs().T @ C.double().abs() + C.double().abs().T @ A.double().abs()) / (2 * N)
    out["hip_err_over_sum_abs_terms"] = float(((Mh - M64).abs() / S).max())
    out["torch_err_over_sum_abs_terms"] = float(((Mt - M64).abs() / S).max())
    bytes_ = 2 * N * d * 4 + d * d * 4
    out["algorithmic_bytes"] = bytes_
    out["flop"] = 2 * N * d * d
    for k in ("hip", "torch"):
        s = out[k]["median_ms"] * 1e-3
        out[k]["GBps"] = bytes_ / s / 1e9
        out[k]["share_of_8TBps"] = bytes_ / s / HBM_PEAK
    out["hip"]["fp32_mfma_TFLOPs"] = out["flop"] / (out["hip"]["median_ms"] * 1e-3) / 1e12
    print(json.dumps(out))


def syevj_step():
    import numpy as np
    import torch
    from drsa_audio_amd.xai.drsa import prca
    out = {"step": "syevj"}
    for d in (64, 100, 128):
        A, C = _rows(4096, d)
        M = prca.relevance_covariance(A, C)

        def host():
            w, V = np.linalg.eigh(M.cpu().numpy().astype(np.float64))
            return (torch.from_numpy(np.ascontiguousarray(w[::-1])).float().cuda(),
                    torch.from_numpy(np.ascontiguousarray(V[:, ::-1])).float().cuda())

        r = _alternate({"hip": lambda: prca.eigh_descending(M), "host_f64_eigh": host}, host_clock=True)
        r["hip_device"] = _alternate({"hip": lambda: prca.eigh_descending(M)})["hip"]   # events: no launch gap
        w, V, sweeps = prca.eigh_descending(M, return_sweeps=True)
        w64, V64 = np.linalg.eigh(M.cpu().numpy().astype(np.float64))
        nrm = float(np.abs(w64).max())
        Vd, wd = V.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
        r.update(sweeps=sweeps, eig_err=float(np.abs(wd - w64[::-1]).max() / nrm),
                 orth=float(np.abs(Vd.T @ Vd - np.eye(d)).max()),
                 residual=float(np.abs(M.cpu().numpy().astype(np.float64) @ Vd - Vd * wd[None, :]).max() / nrm))
        out[f"d{d}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    steps = {"cov": cov_step, "syevj": syevj_step}
    if len(sys.argv) > 1:
        steps[sys.argv[1]]()
        sys.exit(0)
    for step in steps:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=STEP_TIMEOUT[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            sys.exit(rc)       # nothing more runs after a failed or hung step
