"""Times the K x K conv kernels (csrc/conv_generic.hip) and a plan built on them.  HIP events, the variants
alternating inside one process, REPEATS timed repeats each after warm-up, median / min / max reported (the
method of scripts/bench_zbox.py).

(a) kernel level, B = 64, at the GTZAN features.3 shape (32 -> 32 channels, 64 x 64) and at the first layer's
    (1 -> 32, 128 x 128): drsa_amd_convk_fwd / _bwd at 3x3 beside drsa_amd_conv_fwd(pool = 0) /
    drsa_amd_conv_bwd(dense g) on the same data, and the new kernels at 1x1, 5x5 and 7x7 as time, fp32
    TFLOP/s (2 * B * cin * cout * kh * kw * H * W per call) and the fraction of the 157.3 TFLOP/s fp32 MFMA
    peak.  The forward runs ng = 1 with its denominator; the backward xmode 1, post 1.
(b) plan level: one HeatmapGenerator step (K = 4, layer_idx 7, the reference's clone semantics) on the
    GTZAN-128 net with 5x5 convs at B = 64, on the HIP plan and on engine/hooks.py's HookedAutograd built
    directly on the same projection model and composite -- the only other way to explain such a model here.
    Gate (exit status 1 and "plan_faster": false when missed): the plan's median is below the slow path's
    by more than the two spreads (max - min) together.

    python scripts/bench_convk.py [out.json]      # one JSON line; also written to out.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
REPEATS, WARMUP = 20, 3
B = 64
PEAK_TFLOPS = 157.3
SHAPES = {"features.3": (32, 32, 64, 64), "first": (1, 32, 128, 128)}      # cin, cout, H, W
KERNELS = [(1, 1), (3, 3), (5, 5), (7, 7)]


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def _alternate(fns, repeats=REPEATS, warmup=WARMUP):
    """Each fn timed ``repeats`` times, the fns taking turns, after ``warmup`` rounds of all of them."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: _stats(v) for k, v in times.items()}


def _pad32(c):
    return (c + 31) // 32 * 32


def _kernel_level(cin, cout, H, W):
    import torch
    from drsa_audio_amd import _capi
    from drsa_audio_amd.engine.plan import _convk_bwd_layout, _convk_fwd_layout
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    s = _capi.stream_ptr(dev)
    x = torch.randn(B, cin, H, W, device=dev, generator=g)
    gr = torch.randn(B, cout, H, W, device=dev, generator=g)
    den = torch.rand(B, cin, H, W, device=dev, generator=g) + 0.5
    bias = torch.randn(3, _pad32(cout), device=dev, generator=g) * 0.1
    y, yd, r = torch.empty(B, cout, H, W, device=dev), torch.empty(B, cout, H, W, device=dev), torch.empty_like(x)
    keep, fns = [x, gr, den, bias, y, yd, r], {}
    for kh, kw in KERNELS:
        w = torch.randn(cout, cin, kh, kw, device=dev, generator=g) / (cin * kh * kw) ** 0.5
        wf, wb = _convk_fwd_layout([w]), _convk_bwd_layout([w])
        keep += [wf, wb]
        fns[f"convk_fwd_{kh}x{kw}"] = lambda wf=wf, kh=kh, kw=kw: _capi.call(
            "drsa_amd_convk_fwd", x.data_ptr(), wf.data_ptr(), bias.data_ptr(), None, y.data_ptr(), yd.data_ptr(), B, cin,
            cout, H, W, kh, kw, 1, s)
        fns[f"convk_bwd_{kh}x{kw}"] = lambda wb=wb, kh=kh, kw=kw: _capi.call(
            "drsa_amd_convk_bwd", gr.data_ptr(), wb.data_ptr(), x.data_ptr(), den.data_ptr(), r.data_ptr(), B, 1, cout, cin,
            H, W, kh, kw, 1, 1, 1, 1e-6, s)
        if (kh, kw) == (3, 3):      # the tuned 3x3 entry points on the same weights, in their own layouts
            cin_p = 1 if cin == 1 else _pad32(cin)
            t = torch.zeros(1, cin_p, 3, 3, _pad32(cout), device=dev)
            t[0, :cin, :, :, :cout] = w.permute(1, 2, 3, 0)
            w3f = t.reshape(1, 9 * cin_p, _pad32(cout)).contiguous()
            t = torch.zeros(1, _pad32(cout), 3, 3, _pad32(cin), device=dev)
            t[0, :cout, :, :, :cin] = w.flip(2, 3).permute(0, 2, 3, 1)
            w3b = t.reshape(1, 9 * _pad32(cout), _pad32(cin)).contiguous()
            keep += [w3f, w3b]
            fns["conv_fwd_3x3"] = lambda: _capi.call(
                "drsa_amd_conv_fwd", x.data_ptr(), w3f.data_ptr(), bias.data_ptr(), None, y.data_ptr(), None, yd.data_ptr(),
                B, cin, cout, H, W, 1, 0, s)
            fns["conv_bwd_3x3"] = lambda: _capi.call(
                "drsa_amd_conv_bwd", gr.data_ptr(), None, w3b.data_ptr(), x.data_ptr(), den.data_ptr(), r.data_ptr(), B, 1,
                cout, cin, H, W, 1, 1, 1, 1e-6, s)
    out = _alternate(fns)
    for name, st in out.items():
        kh, kw = (int(v) for v in name.rsplit("_", 1)[1].split("x"))
        st["TFLOPs"] = 2.0 * B * cin * cout * kh * kw * H * W / (st["median_ms"] * 1e-3) / 1e12
        st["of_fp32_mfma_peak"] = st["TFLOPs"] / PEAK_TFLOPS
    out["convk_over_conv_fwd_3x3"] = out["convk_fwd_3x3"]["median_ms"] / out["conv_fwd_3x3"]["median_ms"]
    out["convk_over_conv_bwd_3x3"] = out["convk_bwd_3x3"]["median_ms"] / out["conv_bwd_3x3"]["median_ms"]
    del keep
    return out


def _plan_level():
    import numpy as np
    import torch
    from drsa_audio_amd.engine import HookedAutograd, LRPEngine, get_engine
    from drsa_audio_amd.model.create_model import VGGType
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = VGGType(n_filters=(32, 32, 64, 64, 128), conv_kernel=(5, 5), n_dense=128, pool_kernels=((2, 2),) * 5,
                  dropout=0.4, input_size=(128, 128), conv_bn=False, dense_bn=False, block_depth=1).eval().to(dev)
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((64, 64)))
    g = torch.Generator().manual_seed(1)
    e = torch.empty(B, 1, 128, 128).exponential_(generator=g)
    tilt = 10 ** (-3 * torch.arange(128).float() / 127)
    x = torch.clamp(torch.log10(e * tilt[None, None, :, None] + 1e-7), min=-4).to(dev)
    hg = HeatmapGenerator(net, torch.from_numpy(q.astype(np.float32)), LRP_NAME_MAP_GTZAN, "blues", num_concepts=4,
                          layer_idx=7, device=dev, standard="clone")
    plan = get_engine(hg.projectionmodel, hg.composite)
    assert isinstance(plan, LRPEngine)
    slow = HookedAutograd(hg.projectionmodel, hg.composite)
    cls = torch.full((B,), hg.class_idx, dtype=torch.int32, device=dev)
    res = {}

    def run(eng, key):
        res[key] = eng.subspace_heatmaps(x, cls=cls, standard="clone")["standard_heatmaps"]
    out = _alternate({"plan": lambda: run(plan, "plan"), "hooked_autograd": lambda: run(slow, "slow")}, repeats=10, warmup=2)
    a, b = res["plan"].double().flatten(1), res["slow"].double().flatten(1)
    out["rel_l2_plan_vs_hooked_median"] = float(((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).median())
    p, h = out["plan"], out["hooked_autograd"]
    out["hooked_over_plan"] = h["median_ms"] / p["median_ms"]
    out["plan_faster"] = bool(h["median_ms"] - p["median_ms"] > (p["max_ms"] - p["min_ms"]) + (h["max_ms"] - h["min_ms"]))
    # which launches the plan's step spends its time in
    plan.trace = []
    plan.subspace_heatmaps(x, cls=cls, standard="clone")
    torch.cuda.synchronize()
    tags = {}
    for tag, e0, e1 in plan.trace:
        tags[tag] = tags.get(tag, 0.0) + e0.elapsed_time(e1)
    plan.trace = None
    out["plan_tags_ms"] = dict(sorted(tags.items(), key=lambda kv: -kv[1])[:8])
    return out


def main():
    out = {"B": B, "repeats": REPEATS, "kernel": {k: _kernel_level(*v) for k, v in SHAPES.items()}, "plan": _plan_level()}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0 if out["plan"]["plan_faster"] else 1


if __name__ == "__main__":
    sys.exit(main())
