"""Times the concept-audio back end: Mel2Audio.make_audios_batch at B = 64 sources, K = 4 concepts,
GTZAN shape (320 audios of 45 720 samples), HIP events, 20 timed repeats after warm-up, next to
its two yardsticks (DESIGN.md "Concept audio"): the float32 CPU oracle (tests/audiogen_ref.py,
mode "torch32", 16 threads) on the same batch, and the HBM floor of the algorithmic bytes.

    python scripts/bench_audiogen.py            # both steps, each a child process under its own timeout
    python scripts/bench_audiogen.py gpu|cpu    # one step

Prints one JSON line per step.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
B, K, REPEATS, WARMUP = 64, 4, 20, 3
STEP_TIMEOUT = {"gpu": 240, "cpu": 600}


def inputs():
    import audiogen_ref as R
    return R.signals(B, 48000, seed=1), R.heatmaps(B, K + 1, 128, 128, seed=2, absolute=True)


def gpu_step():
    import numpy as np
    import torch
    from drsa_audio_amd.xai.explain.audiogen import Mel2Audio, heatmap_masks, percentile_rank
    dev = torch.device("cuda")
    wavs, h = inputs()
    wavs, std, sub = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (wavs, h[:, 0], h[:, 1:]))
    m = Mel2Audio("gtzan", device=dev)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPEATS)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}

    out = {"step": "gpu", "B": B, "K": K, "audios": B * (K + 1),
           "make_audios_batch": timed(lambda: m.make_audios_batch(std, sub, wavs, percentile=50))}
    mel, X = m._analyse(wavs, True)
    hm = torch.cat([std[:, None], sub], 1)
    r = percentile_rank(50, 128 * 128)
    masks = heatmap_masks(hm, m.smoother, r, r, group=K + 1)
    out["analysis"] = timed(lambda: m._analyse(wavs, True))
    out["mask"] = timed(lambda: heatmap_masks(hm, m.smoother, r, r, group=K + 1))
    out["synthesis"] = timed(lambda: m._synthesise(mel, X, masks))
    # algorithmic bytes: per audio its mask and its output, per source its mel and spectrum (P from L2)
    n_out = 360 * 127
    bytes_ = B * (K + 1) * (128 * 128 * 4 + n_out * 4) + B * (128 * 128 * 4 + 128 * 401 * 8)
    out["hbm_floor_bytes"] = bytes_
    out["hbm_floor_ms_at_6.3TBps"] = bytes_ / 6.3e12 * 1e3
    print(json.dumps(out))


def cpu_step():
    import torch
    import audiogen_ref as R
    torch.set_num_threads(16)
    wavs, h = inputs()
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        R.make_audios_batch(h[:, 0], h[:, 1:], wavs, R.GEOM["gtzan"], 50, mode="torch32")
        t.append(time.perf_counter() - t0)
    print(json.dumps({"step": "cpu", "threads": 16, "torch32_oracle_ms": min(t) * 1e3}))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        {"gpu": gpu_step, "cpu": cpu_step}[sys.argv[1]]()
        sys.exit(0)
    for step in ("gpu", "cpu"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=STEP_TIMEOUT[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            sys.exit(rc)       # nothing more runs after a failed or hung step
