"""Times drsa_run on the natural geometry (drsa_amd_drsa_any_run, csrc/drsa_partial_nat.h) at
N = 100 000: the shapes the padded geometry refuses -- (d, K) = (100, 5), (100, 20), (128, 1) --
and, for context, (100, 4) through the padded drsa_amd_drsa_run and the same (100, 4) through
drsa_amd_drsa_any_run.  us per optimiser step = a STEPS-step graph-replayed run between HIP events
divided by STEPS (the run's final objective pass included); median of 20 timed repeats after
warm-up, the cases alternating in one process.

    python scripts/bench_drsa_any.py

Prints one JSON line.  Nothing is gated on these times.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
REPEATS, WARMUP = 20, 3
N, STEPS = 100000, 100
CASES = [("any_100_5", 100, 5, True), ("any_100_20", 100, 20, True), ("any_128_1", 128, 1, True),
         ("padded_100_4", 100, 4, False), ("any_100_4", 100, 4, True)]


def main():
    import numpy as np
    import torch
    from drsa_audio_amd import _capi
    from drsa_audio_amd.utils.synthetic import drsa_inputs
    from drsa_audio_amd.xai.drsa.drsa import geometry_kind
    dev = torch.device("cuda")
    lib = _capi.lib()
    stream = torch.cuda.Stream(dev)       # graph capture needs a non-default stream
    rows = {d: tuple(torch.from_numpy(v).to(dev) for v in drsa_inputs(N, d, seed=1)) for d in (100, 128)}
    fns, finals = {}, {}
    for name, d, K, use_any in CASES:
        assert use_any or geometry_kind(d, K) == "padded"
        A, C = rows[d]
        U0 = torch.from_numpy(np.linalg.qr(np.random.default_rng(d + K).standard_normal((d, d)))[0].astype(np.float32)).to(dev)
        fam = "drsa_amd_drsa_any_" if use_any else "drsa_amd_drsa_"
        ws = torch.empty(getattr(lib, fam + "workspace_bytes")(N, d, K), dtype=torch.uint8, device=dev)
        U, U_tmp = U0.clone(), torch.empty_like(U0)
        traj = torch.empty(STEPS + 1, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)

        def run(fam=fam, A=A, C=C, d=d, K=K, U0=U0, U=U, U_tmp=U_tmp, traj=traj, counter=counter, ws=ws):
            U.copy_(U0)
            _capi.call(fam + "run", A.data_ptr(), C.data_ptr(), N, d, K, U.data_ptr(), U_tmp.data_ptr(), STEPS,
                       traj.data_ptr(), counter.data_ptr(), ws.data_ptr(), ws.numel(), 1, stream.cuda_stream)

        fns[name], finals[name] = run, traj
    times = {k: [] for k in fns}
    with torch.cuda.stream(stream):
        for _ in range(WARMUP):
            for fn in fns.values():
                fn()
        stream.synchronize()
        for _ in range(REPEATS):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3 / STEPS)
    out = {"bench": "drsa_any", "N": N, "steps": STEPS, "repeats": REPEATS}
    for k, v in times.items():
        v = sorted(v)
        t = finals[k].cpu().numpy()
        out[k] = {"us_per_step_median": v[len(v) // 2], "min": v[0], "max": v[-1], "f0": float(t[0]), "fS": float(t[-1])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
