"""Times whole-track explanations (DESIGN.md "Whole-track explanations"): the stitch kernel
drsa_amd_track_stitch at the GTZAN track shape (30 s: n = 20 chunks of 128 columns every h = 64,
Wt = 1344, C = 5 maps) at H = 128 (mel resolution) and H = 401 (STFT resolution), next to a
composition of torch ops that computes the same thing (gather by order, multiply by the taper,
index_add_ into the track, divide by the folded taper, row sum) -- the yardstick --, and
TrackExplainer.explain() end to end on a 30 s synthetic track with the small GTZAN-128 net, split into
the engine's time and everything else.  HIP events, median (min ... max) of 20 timed repeats after
warm-up; the kernel and the composition alternate in the same process, repeat by repeat.  The bytes
the kernel moves (every input and output element once) are stated as a time at the MI355X's
measured copy rate.

    python scripts/bench_track.py          # the measurement, as a child process under a timeout
    python scripts/bench_track.py gpu      # the measurement itself

Prints one JSON line.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
N, K, W, HF, REPEATS, WARMUP = 20, 4, 128, 64, 20, 3
STEP_TIMEOUT = 300
HBM_BPS = 6.3e12            # measured copy rate of the MI355X


def gpu_step():
    import numpy as np
    import torch
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN
    from drsa_audio_amd.utils.synthetic import synthetic_songs
    from drsa_audio_amd.xai.explain.audiogen import Mel2Audio
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
    from drsa_audio_amd.xai.explain.track import TrackExplainer, make_taper, track_stitch
    import lrp_common as LC
    dev = torch.device("cuda")

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

    out = {"step": "gpu", "n": N, "K": K, "W": W, "h": HF, "Wt": (N - 1) * HF + W}
    Wt, C = out["Wt"], K + 1
    taper = make_taper(W).to(dev)
    g = torch.Generator().manual_seed(0)
    for H in (128, 401):
        std = torch.randn(N, 1, H, W, generator=g).to(dev)
        sub = torch.randn(N, K, H, W, generator=g).to(dev)
        order = torch.stack([torch.randperm(K, generator=g) for _ in range(N)]).to(dev)
        # the composition's constants (built once, as the kernel's taper is): the inverse permutation,
        # every chunk column's track column, the folded taper
        inv = torch.argsort(order, -1)
        cols = (torch.arange(N, device=dev)[:, None] * HF + torch.arange(W, device=dev)[None]).reshape(-1)
        den = torch.zeros(Wt, device=dev).index_add_(0, cols, taper.repeat(N))

        def composed():
            x = torch.cat([std, torch.gather(sub, 1, inv[:, :, None, None].expand(-1, -1, H, W))], 1)    # [N, C, H, W]
            x = (x * taper).permute(1, 2, 0, 3).reshape(C, H, N * W)
            o = torch.zeros(C, H, Wt, device=dev).index_add_(2, cols, x) / den
            return o, o.sum(1)

        a, b = track_stitch(std, sub, order, taper, HF), composed()
        err = float((a[0] - b[0]).abs().max())
        assert err <= 1e-5, err                    # the same thing, up to the order of the two-term sums
        kern, comp = timed(lambda: track_stitch(std, sub, order, taper, HF, check_order=False), composed)
        nbytes = (C * N * H * W + C * H * Wt + C * Wt) * 4
        out[f"stitch_H{H}"] = dict(kernel=kern, torch_composition=comp, max_abs_diff=err, bytes=nbytes,
                                   hbm_floor_ms=nbytes / HBM_BPS * 1e3,
                                   kernel_fraction_of_hbm_rate=nbytes / HBM_BPS * 1e3 / kern["median_ms"])

    # end to end: 30 s, the small GTZAN-128 net of the tests, K = 4 concepts at layer 7
    net = LC.gtzan128().to(dev)
    hg = HeatmapGenerator(net, LC.ortho(64, 0), LRP_NAME_MAP_GTZAN, "blues", num_concepts=K, layer_idx=7, device=dev)
    ex = TrackExplainer(hg, Mel2Audio("gtzan", device=dev))
    wav = torch.from_numpy(synthetic_songs(1, seconds=30.0, seed=1)[0]).to(dev)
    _, chunks, (n, _, _, Wr) = ex.chunks(wav)
    x = ex.loader._run(chunks, n, ex.L, 1, 0, ex.L, peak_norm=True, clamp=True)
    full, mel_only, engine = timed(lambda: ex.explain(wav), lambda: ex.explain(wav, audio=False),
                                   lambda: hg.generate_subspace_heatmaps(x, to_host=False))
    out["explain_30s"] = dict(n_chunks=n, Wr=Wr, explain=full, explain_no_audio=mel_only, engine=engine,
                              everything_else_median_ms=full["median_ms"] - engine["median_ms"])
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
