"""Times a mixed-class batch of concept heatmaps in one MultiHeatmapGenerator pass (a projection matrix per row)
beside the loop of per-class HeatmapGenerators it replaces.  HIP events, the variants alternating inside one
process, REPEATS timed repeats each after warm-up, median / min / max reported (the method of
scripts/bench_convk.py).

GTZAN-128, layer_idx 7 (d = 64), K = 4, the reference's clone semantics, ten genres x 16 rows and ten genres x 50
rows, results left on the device:
  fused      one MultiHeatmapGenerator pass over all 10 x rows
  loop_warm  ten HeatmapGenerators, one per genre over its rows, every plan in the engine cache (the cache is
             widened to hold all ten for this variant)
  loop_cold  the same loop with the default cache of eight plans, emptied first: ten genres go round a cache of
             eight, so every pass compiles its plan again, as perform_cf's loops do
Before each timed call the variant's cache state is set up, outside the event pair.  The loop is the path the
per-class interface has always taken; it is the baseline here, not code under test.

Gate (exit status 1 and "fused_faster": false when missed), per batch size: the fused pass's median is below the
warm loop's by more than the two spreads (max - min) together.  The per-tag device times of one fused pass and of
one warm loop (summed over its ten passes) are reported beside it.

    python scripts/bench_multi_u.py [out.json]      # one JSON line; also written to out.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
REPEATS, WARMUP = 20, 3
ROWS_PER_CLASS = (16, 50)
K, LAYER = 4, 7


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def _alternate(fns, preps, repeats=REPEATS, warmup=WARMUP):
    """Each fn timed ``repeats`` times, the fns taking turns, after ``warmup`` rounds of all of them; ``preps[k]``
    runs before every call of fn k, outside the event pair."""
    import torch
    times = {k: [] for k in fns}
    for it in range(warmup + repeats):
        for k, fn in fns.items():
            preps[k]()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: _stats(v) for k, v in times.items()}


def _tags(engines_and_calls):
    """Per-tag device time (ms) of the given (engine, call) pairs, summed."""
    import torch
    tags = {}
    for eng, call in engines_and_calls:
        eng.trace = []
        call()
        torch.cuda.synchronize()
        for tag, e0, e1 in eng.trace:
            tags[tag] = tags.get(tag, 0.0) + e0.elapsed_time(e1)
        eng.trace = None
    return dict(sorted(tags.items(), key=lambda kv: -kv[1])[:8]), sum(tags.values())


def _bench(spc):
    import numpy as np
    import torch
    from drsa_audio_amd import engine
    from drsa_audio_amd.model.create_model import VGGType
    from drsa_audio_amd.utils.constants import CLASS_IDX_MAPPER, LRP_NAME_MAP_GTZAN
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator, MultiHeatmapGenerator
    dev = torch.device("cuda")
    genres = list(CLASS_IDX_MAPPER)
    torch.manual_seed(0)
    net = VGGType(n_filters=(32, 32, 64, 64, 128), n_dense=128, pool_kernels=((2, 2),) * 5, dropout=0.4,
                  input_size=(128, 128), conv_bn=False, dense_bn=False, block_depth=1).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    e = torch.empty(len(genres) * spc, 1, 128, 128).exponential_(generator=g)
    tilt = 10 ** (-3 * torch.arange(128).float() / 127)
    x = torch.clamp(torch.log10(e * tilt[None, None, :, None] + 1e-7), min=-4).to(dev)
    Us = {c: torch.from_numpy(np.linalg.qr(np.random.default_rng(i).standard_normal((64, 64)))[0].astype(np.float32))
          for i, c in enumerate(genres)}
    rows = [c for c in genres for _ in range(spc)]
    multi = MultiHeatmapGenerator(net, Us, LRP_NAME_MAP_GTZAN, num_concepts=K, layer_idx=LAYER, device=dev)
    singles = [HeatmapGenerator(net, Us[c], LRP_NAME_MAP_GTZAN, c, num_concepts=K, layer_idx=LAYER, device=dev)
               for c in genres]
    default_cache = engine._MAX

    def fused():
        multi.generate_subspace_heatmaps(x, rows, to_host=False)

    def loop():
        for i, hg in enumerate(singles):
            hg.generate_subspace_heatmaps(x[i * spc:(i + 1) * spc], to_host=False)

    def warm(fn):
        def prep():
            engine._MAX = 2 * len(genres) + 2       # every plan of this script stays cached
            fn()
        return prep

    def cold():
        engine._MAX = default_cache
        engine.clear_cache()

    out = _alternate({"fused": fused, "loop_warm": loop, "loop_cold": loop},
                     {"fused": warm(fused), "loop_warm": warm(loop), "loop_cold": cold})
    # the same bits from both paths, on the last genre's rows
    warm(loop)()
    want = singles[-1].info_device["subspace_heatmaps"].clone()
    warm(fused)()
    out["equal"] = bool(torch.equal(multi.info_device["subspace_heatmaps"][-spc:], want))
    f, lw = out["fused"], out["loop_warm"]
    out["loop_warm_over_fused"] = lw["median_ms"] / f["median_ms"]
    out["loop_cold_over_fused"] = out["loop_cold"]["median_ms"] / f["median_ms"]
    out["fused_faster"] = bool(lw["median_ms"] - f["median_ms"] > (f["max_ms"] - f["min_ms"]) + (lw["max_ms"] - lw["min_ms"]))
    out["fused_tags_ms"], out["fused_device_ms"] = _tags(
        [(engine.get_engine(multi.projectionmodel, multi.composite), fused)])
    out["loop_warm_tags_ms"], out["loop_warm_device_ms"] = _tags(
        [(engine.get_engine(hg.projectionmodel, hg.composite),
          lambda hg=hg, i=i: hg.generate_subspace_heatmaps(x[i * spc:(i + 1) * spc], to_host=False))
         for i, hg in enumerate(singles)])
    engine._MAX = default_cache
    engine.clear_cache()
    return out


def main():
    out = {"model": "gtzan128", "layer_idx": LAYER, "K": K, "classes": 10, "repeats": REPEATS,
           "rows_per_class": {str(spc): _bench(spc) for spc in ROWS_PER_CLASS}}
    out["fused_faster"] = all(v["fused_faster"] for v in out["rows_per_class"].values())
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0 if out["fused_faster"] else 1


if __name__ == "__main__":
    sys.exit(main())
