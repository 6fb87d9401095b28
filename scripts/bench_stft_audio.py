"""Times concept audio at STFT resolution: Mel2Audio.make_audios_batch(resolution="stft") at B = 64
sources, K = 4 concepts, GTZAN shape (320 maps of 401 x 128, 320 audios of 45 720 samples), HIP
events, median (min ... max) of 20 timed repeats after warm-up, the whole call and each of its
launches.  The mel-resolution call on the same batch is the yardstick: the two alternate in the
same process, repeat by repeat (DESIGN.md "Concept audio at STFT resolution").  The HBM floor of
the algorithmic bytes is stated next to each.

    python scripts/bench_stft_audio.py          # the measurement, as a child process under a timeout
    python scripts/bench_stft_audio.py gpu      # the measurement itself

Prints one JSON line.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
B, K, REPEATS, WARMUP = 64, 4, 20, 3
STEP_TIMEOUT = 240
HBM_BPS = 6.3e12            # measured copy rate of the MI355X


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

    def timed(*fns):
        """The functions alternate inside every repeat; one dict of times per function."""
        for _ in range(WARMUP):
            for fn in fns:
                fn()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPEATS)]
              for _ in fns]
        for i in range(REPEATS):
            for fn, e in zip(fns, ev):
                e[i][0].record()
                fn()
                e[i][1].record()
        torch.cuda.synchronize()
        out = []
        for e in ev:
            ms = sorted(a.elapsed_time(b) for a, b in e)
            out.append({"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]})
        return out

    C, n_mels, n_freq, width, n_out = K + 1, 128, 401, 128, 360 * 127
    stft, mel_res = timed(lambda: m.make_audios_batch(std, sub, wavs, percentile=50, resolution="stft"),
                          lambda: m.make_audios_batch(std, sub, wavs, percentile=50))
    out = {"step": "gpu", "B": B, "K": K, "audios": B * C, "make_audios_batch_stft": stft,
           "make_audios_batch_mel": mel_res}
    hm = torch.cat([std[:, None], sub], 1)
    mel, X = m.analyse_stft(wavs)
    maps = m.lift_to_stft(hm, mel, X)
    r = percentile_rank(50, n_freq * width)
    masks = heatmap_masks(maps, m.smoother, r, r, group=C)
    audios = m.stft_masks_to_audio(X, masks)
    launches = {
        "analysis": (lambda: m.analyse_stft(wavs), B * (48000 * 4 + n_mels * width * 4 + width * n_freq * 8)),
        "lift": (lambda: m.lift_to_stft(hm, mel, X),
                 B * (C * n_mels * width * 4 + n_mels * width * 4 + width * n_freq * 8 + C * n_freq * width * 4)),
        "mask": (lambda: heatmap_masks(maps, m.smoother, r, r, group=C), B * C * 2 * n_freq * width * 4),
        "synthesis": (lambda: m.stft_masks_to_audio(X, masks),
                      B * (width * n_freq * 8 + C * (n_freq * width * 4 + n_out * 4))),
        "normalise": (lambda: m.normalise(audios, wavs), B * (C * 2 * n_out * 4 + 48000 * 4)),
    }
    total = 0
    for name, (fn, nbytes) in launches.items():
        out[name] = dict(timed(fn)[0], hbm_floor_bytes=nbytes, hbm_floor_ms=nbytes / HBM_BPS * 1e3)
        total += nbytes
    # algorithmic bytes of the whole call: every launch reads its inputs and writes its outputs once
    out["hbm_floor_bytes"] = total
    out["hbm_floor_ms_at_6.3TBps"] = total / HBM_BPS * 1e3
    # the mel path's floor, as scripts/bench_audiogen.py states it
    mel_bytes = B * C * (128 * 128 * 4 + n_out * 4) + B * (128 * 128 * 4 + 128 * 401 * 8)
    out["mel_hbm_floor_ms_at_6.3TBps"] = mel_bytes / HBM_BPS * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        {"gpu": gpu_step}[sys.argv[1]]()
        sys.exit(0)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "gpu"], timeout=STEP_TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        rc = 124
    sys.exit(rc)
