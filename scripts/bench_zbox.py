"""Times the ZBox first layer's kernels (csrc/first_layer_zbox.hip; the backward is csrc/first_layer_bwd.h with
two chains) next to the WSquare / Flat backward (the same kernel with one chain), at the headline shape of bench.py: B = 512 samples, 4 relevance clones, C = 32 channels,
128 x 128 input, relevance pool-sparse (64 x 64 cells with their argmax bytes).  HIP events, 20 timed
repeats after warm-up, the kernels alternating in one process (the method of scripts/bench_prca.py;
DESIGN.md 14):

    zbox_bwd         drsa_amd_first_layer_zbox_bwd   two fma chains per pixel, epilogue (x - l) S+ + (x - h) S-
    first_layer_bwd  drsa_amd_first_layer_bwd        one chain per pixel
    zbox_den         drsa_amd_first_layer_zbox_den   the per-sample denominator copy at the argmax

    python scripts/bench_zbox.py          # the comparison; one JSON line
    python scripts/bench_zbox.py once     # three untimed launches of zbox_bwd alone (for a counter run)

Nothing is gated on these times.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
REPEATS, WARMUP = 20, 3
B, CLONES, C, H, W = 512, 4, 32, 128, 128


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def _alternate(fns):
    """Each fn timed REPEATS times, the fns taking turns, after WARMUP rounds of all of them."""
    import torch
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: _stats(v) for k, v in times.items()}


def _setup():
    import torch
    from drsa_audio_amd import _capi
    _capi.load()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    Bq = B * CLONES
    gp = torch.randn(Bq, C, H // 2, W // 2, device=dev, generator=g)
    amax = torch.randint(0, 4, (B, C, H // 2, W // 2), device=dev, generator=g, dtype=torch.uint8)
    w = torch.randn(C, 9, device=dev, generator=g) / 3
    wpn = torch.stack([w.clamp(min=0), w.clamp(max=0)]).contiguous()
    w2 = (w * w).contiguous()
    x = torch.rand(B, 1, H, W, device=dev, generator=g) * 6 - 4
    lo, hi = torch.full((H, W), -4.0, device=dev), torch.full((H, W), 2.0, device=dev)
    a = torch.rand(B, C, H // 2, W // 2, device=dev, generator=g)
    zl, zh = torch.randn(C, H, W, device=dev, generator=g), torch.randn(C, H, W, device=dev, generator=g)
    out, den = torch.empty(Bq, 1, H, W, device=dev), torch.empty_like(a)
    s = _capi.stream_ptr(dev)
    keep = (gp, amax, wpn, w2, x, lo, hi, a, zl, zh, out, den)
    fns = {
        "zbox_bwd": lambda: _capi.call("drsa_amd_first_layer_zbox_bwd", gp.data_ptr(), amax.data_ptr(), wpn.data_ptr(),
                                       x.data_ptr(), lo.data_ptr(), hi.data_ptr(), out.data_ptr(), Bq, CLONES, C, H, W,
                                       s),
        "first_layer_bwd": lambda: _capi.call("drsa_amd_first_layer_bwd", gp.data_ptr(), amax.data_ptr(), w2.data_ptr(),
                                              out.data_ptr(), Bq, CLONES, C, H, W, s),
        "zbox_den": lambda: _capi.call("drsa_amd_first_layer_zbox_den", a.data_ptr(), amax.data_ptr(), zl.data_ptr(),
                                       zh.data_ptr(), den.data_ptr(), B, C, H, W, s),
    }
    return fns, keep


def main():
    import torch
    fns, keep = _setup()
    if len(sys.argv) > 1 and sys.argv[1] == "once":
        for _ in range(3):
            fns["zbox_bwd"]()
        torch.cuda.synchronize()
        return
    out = {"shape": {"B": B, "clones": CLONES, "C": C, "H": H, "W": W, "g": "pool-sparse"}}
    out.update(_alternate(fns))
    out["zbox_bwd_over_first_layer_bwd"] = out["zbox_bwd"]["median_ms"] / out["first_layer_bwd"]["median_ms"]
    # algorithmic bytes of zbox_bwd: g and the argmax bytes once, x per sample, out once
    Bq = B * CLONES
    bytes_ = Bq * C * (H // 2) * (W // 2) * 4 + B * C * (H // 2) * (W // 2) + B * H * W * 4 + Bq * H * W * 4
    out["zbox_bwd"]["GBps"] = bytes_ / (out["zbox_bwd"]["median_ms"] * 1e-3) / 1e9
    out["zbox_bwd"]["fp32_fma_TFLOPs"] = 2 * 2 * 9 * C * Bq * H * W / (out["zbox_bwd"]["median_ms"] * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == "__main__":
    main()
