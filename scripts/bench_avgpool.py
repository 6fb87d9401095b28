"""Times the average-pool kernels (csrc/pool_avg.hip) beside their max-pool counterparts, and whole plans over
average pools beside the same nets with max pools.  HIP events, the variants alternating inside one process,
REPEATS timed repeats each after warm-up, median / min / max reported (the method of scripts/bench_convk.py;
DESIGN.md 18).

(a) kernel level at B = 64, C = 32, 128 x 128, pool (2,2), relevance clones 1 and 4: drsa_amd_avgpool_fwd beside
    drsa_amd_maxpool_capture (no denominator gathered), and drsa_amd_avgpool_bwd (pool rule none / Epsilon, the
    conv's denominator none / per sample, rel_full off / on) beside drsa_amd_relevance_unpool, each as time and
    as effective bandwidth = algorithmic bytes / time.  Algorithmic bytes count every tensor once at its own
    size (a per-sample map that the clones share counts once), 4 bytes a float and 1 an argmax byte:
      avgpool_fwd       a N                    + y N/4
      maxpool_capture   a N                    + y N/4 + amax N/4 bytes
      avgpool_bwd       R_y Nq/4 [+ y N/4] + a N [+ den N] + g Nq [+ rel_full Nq]
      relevance_unpool  rel Nq/4 + amax N/4 bytes + out Nq
    with N = B C H W and Nq = clones N.
    Before every timed kernel call a 512 MiB scratch buffer is filled, outside the event pair: the maps here
    (128 MiB each) fit the 256 MiB Infinity Cache, and a kernel timed right after another that read the same map
    would be timed on a warm cache while its counterpart is not.  So every figure is a read from HBM.
    Gate (exit status 1 and "meets_bar": false when missed): every new kernel's effective bandwidth is at
    least 0.9 x its counterpart's from the same run (the forward against maxpool_capture, every backward
    variant against relevance_unpool at the same clone count).
(b) plan level, as information: one compute_relevances pass (forward + LRP backward, B = 64) on the toy and the
    GTZAN-128 nets with every pool averaged beside the same nets with max pools (whose plans fuse the pool
    into the conv and hand a pool-sparse g down, which an average pool cannot).

    python scripts/bench_avgpool.py [out.json]      # one JSON line; also written to out.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
REPEATS, WARMUP = 20, 3
B, C, H, W, PH, PW = 64, 32, 128, 128, 2, 2
CLONES = (1, 4)
BAR = 0.9


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def _alternate(fns, repeats=REPEATS, warmup=WARMUP, flush=None):
    """Each fn timed ``repeats`` times, the fns taking turns, after ``warmup`` rounds of all of them.  ``flush``: a
    buffer larger than the last-level cache, filled before every timed call (not timed)."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            if flush is not None:
                flush.fill_(len(times[k]))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: _stats(v) for k, v in times.items()}


def _kernel_level():
    import torch
    from drsa_audio_amd import _capi
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    s = _capi.stream_ptr(dev)
    ho, wo, N = H // PH, W // PW, B * C * H * W
    a = torch.randn(B, C, H, W, device=dev, generator=gen).clamp(min=0)
    den = torch.rand(B, C, H, W, device=dev, generator=gen) + 0.5
    y, ym = torch.empty(B, C, ho, wo, device=dev), torch.empty(B, C, ho, wo, device=dev)
    amax = torch.empty(B, C, ho, wo, device=dev, dtype=torch.uint8)
    fns, nbytes, keep = {}, {}, [a, den, y, ym, amax]
    fns["avgpool_fwd"] = lambda: _capi.call("drsa_amd_avgpool_fwd", a.data_ptr(), y.data_ptr(), B, C, H, W, PH, PW, s)
    nbytes["avgpool_fwd"] = 4 * N + N
    fns["maxpool_capture"] = lambda: _capi.call("drsa_amd_maxpool_capture", a.data_ptr(), None, ym.data_ptr(),
                                                amax.data_ptr(), None, B, C, H, W, PH, PW, s)
    nbytes["maxpool_capture"] = 4 * N + N + N // 4
    fns["maxpool_capture"]()        # amax and y hold real values before the backward kernels read them
    fns["avgpool_fwd"]()
    for clones in CLONES:
        Bq, Nq = B * clones, N * clones
        R = torch.randn(Bq, C, ho, wo, device=dev, generator=gen)
        g, rel, up = (torch.empty(Bq, C, H, W, device=dev) for _ in range(3))
        keep += [R, g, rel, up]
        fns[f"relevance_unpool_c{clones}"] = lambda R=R, up=up, Bq=Bq, clones=clones: _capi.call(
            "drsa_amd_relevance_unpool", R.data_ptr(), amax.data_ptr(), Bq, clones, C, H, W, PH, PW, up.data_ptr(), s)
        nbytes[f"relevance_unpool_c{clones}"] = Nq + N // 4 + 4 * Nq
        for rule in (0, 1):
            for use_den in (0, 1):
                for want_rel in (0, 1):
                    if want_rel and not (rule and use_den):
                        continue        # rel_full is timed on the heaviest form only
                    key = f"avgpool_bwd_{'eps' if rule else 'plain'}_{'den' if use_den else 'noden'}" \
                          f"{'_rel' if want_rel else ''}_c{clones}"
                    fns[key] = lambda R=R, g=g, rel=rel, Bq=Bq, clones=clones, rule=rule, use_den=use_den, want_rel=want_rel: \
                        _capi.call("drsa_amd_avgpool_bwd", R.data_ptr(), y.data_ptr(), a.data_ptr(),
                                   den.data_ptr() if use_den else None, 0, rule, 1e-6, 1e-7, g.data_ptr(),
                                   rel.data_ptr() if want_rel else None, Bq, clones, C, H, W, PH, PW, s)
                    nbytes[key] = Nq + (N if rule else 0) + 4 * N + (4 * N if use_den else 0) + 4 * Nq + \
                        (4 * Nq if want_rel else 0)
    out = _alternate(fns, flush=torch.empty(512 << 20, dtype=torch.uint8, device=dev))
    for k, st in out.items():
        st["bytes"] = nbytes[k]
        st["GBps"] = nbytes[k] / (st["median_ms"] * 1e-3) / 1e9
    pairs = {"avgpool_fwd": "maxpool_capture"}
    pairs.update({k: f"relevance_unpool_c{k.rsplit('_c', 1)[1]}" for k in out if k.startswith("avgpool_bwd")})
    ratios = {k: out[k]["GBps"] / out[ref]["GBps"] for k, ref in pairs.items()}
    del keep
    return out, ratios


def _nets():
    import torch
    from drsa_audio_amd.model.create_model import VGGType
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY
    cfg = {"toy": (dict(n_filters=(8, 8, 16, 16, 16), n_dense=32, n_classes=2, dropout=0.0, input_size=(64, 64)),
                   LRP_NAME_MAP_TOY),
           "gtzan128": (dict(n_filters=(32, 32, 64, 64, 128), n_dense=128, dropout=0.4, input_size=(128, 128)),
                        LRP_NAME_MAP_GTZAN)}
    for name, (kw, nm) in cfg.items():
        for pool in ("max", "avg"):
            torch.manual_seed(0)
            yield name, pool, nm, VGGType(pool_kernels=((2, 2),) * 5, conv_bn=False, dense_bn=False, block_depth=1, pool=pool,
                                          **kw).eval()


def _plan_level():
    import torch
    from drsa_audio_amd.xai.explain.attribute import compute_relevances
    from drsa_audio_amd.zennit.composites import NameMapComposite
    dev = torch.device("cuda")
    fns, keep = {}, []
    for name, pool, nm, net in _nets():
        net, comp = net.to(dev), NameMapComposite(nm)
        Hn = 64 if name == "toy" else 128
        g = torch.Generator().manual_seed(1)
        e = torch.empty(B, 1, Hn, Hn).exponential_(generator=g)
        tilt = 10 ** (-3 * torch.arange(Hn).float() / (Hn - 1))
        x = torch.clamp(torch.log10(e * tilt[None, None, :, None] + 1e-7), min=-4).to(dev)
        keep += [net, comp, x]
        fns[f"{name}_{pool}"] = lambda net=net, comp=comp, x=x: compute_relevances(net, x, comp, class_idx=1)
    out = _alternate(fns, repeats=10, warmup=2)
    for name in ("toy", "gtzan128"):
        out[f"{name}_avg_over_max"] = out[f"{name}_avg"]["median_ms"] / out[f"{name}_max"]["median_ms"]
    del keep
    return out


def main():
    kernel, ratios = _kernel_level()
    out = {"B": B, "C": C, "H": H, "W": W, "pool": [PH, PW], "repeats": REPEATS, "kernel": kernel,
           "GBps_over_counterpart": ratios, "bar": BAR, "meets_bar": all(r >= BAR for r in ratios.values()),
           "plan": _plan_level()}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0 if out["meets_bar"] else 1


if __name__ == "__main__":
    sys.exit(main())
