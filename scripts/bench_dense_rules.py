"""Times the fused dense rule kernels (drsa_amd_linear_rule_fwd / _bwd, csrc/linear_rules.hip) on the
GTZAN head at B = 512 under Gamma, next to the same work composed from the Epsilon head's launches
(DESIGN.md 7): one drsa_amd_linear_fwd per forward chain (z and every denominator term) and one
drsa_amd_linear_bwd per term of R_in.  The composition is a timing yardstick only: it stages x and g
once per launch and leaves out the element-wise passes that would join its pieces.

    python scripts/bench_dense_rules.py

HIP events, 50 timed repeats after 5 warm-up launches, the median.  Prints one JSON line per layer.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
B, REPEATS, WARMUP = 512, 50, 5
# (name, K, N, ReLU after, signed input): the GTZAN head, and classifier.0 below a ProjectionModel at
# the last conv block (its input a' is signed)
LAYERS = [("classifier.0", 2048, 128, True, False), ("classifier.3", 128, 128, True, False),
          ("classifier.6", 128, 10, False, False), ("classifier.0 signed", 2048, 128, True, True)]


def main():
    import torch
    from drsa_audio_amd import _capi
    from drsa_audio_amd._capi import POST_NONE, XM_MUL
    from drsa_audio_amd.engine.plan import dense_rule_params
    from drsa_audio_amd.zennit.rules import Gamma
    dev = torch.device("cuda")
    _capi.load()
    s = _capi.stream_ptr(dev)
    g = torch.Generator().manual_seed(0)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPEATS)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}

    for name, K, N, relu, signed in LAYERS:
        W = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g) * 0.1
        rp = {k: v.to(dev).contiguous() if isinstance(v, torch.Tensor) else v
              for k, v in dense_rule_params(W, b, Gamma(gamma=0.25, stabilizer=1e-7)).items()}
        W, b = W.to(dev), b.to(dev)
        x = torch.randn(B, K, generator=g)
        x = (x if signed else x.abs()).to(dev)
        R = torch.randn(B, N, generator=g).to(dev)
        z, act, dp, dn = (torch.empty(B, N, device=dev) for _ in range(4))
        out = torch.empty(B, K, device=dev)
        negden = not relu
        chains = 2 + (1 if signed else 0) + (1 if negden else 0) + (1 if signed and negden else 0)
        terms = (2 if signed else 1) * (2 if negden else 1)
        need_wn = signed or negden

        def fwd_composed():
            for _ in range(chains):
                _capi.call("drsa_amd_linear_fwd", x.data_ptr(), W.data_ptr(), b.data_ptr(), z.data_ptr(),
                           act.data_ptr() if relu else None, B, N, K, s)

        def fwd_fused():
            _capi.call("drsa_amd_linear_rule_fwd", x.data_ptr(), W.data_ptr(), rp["Wp"].data_ptr(),
                       rp["Wn"].data_ptr() if need_wn else None, b.data_ptr(), rp["bp"].data_ptr(),
                       rp["bn"].data_ptr() if negden else None, z.data_ptr(), act.data_ptr() if relu else None,
                       dp.data_ptr(), dn.data_ptr() if negden else None, 1 if signed else 0, B, N, K, s)

        def bwd_composed():
            for _ in range(terms):
                _capi.call("drsa_amd_linear_bwd", R.data_ptr(), None, 0, z.data_ptr(), 1 if relu else 0, 1, 1e-7,
                           W.data_ptr(), x.data_ptr(), XM_MUL, None, POST_NONE, 0.0, out.data_ptr(), B, N, K, s)

        def bwd_fused():
            _capi.call("drsa_amd_linear_rule_bwd", R.data_ptr(), None, 0, z.data_ptr(), 1 if relu else 0, dp.data_ptr(),
                       dn.data_ptr() if negden else None, 0, 1, 1e-7, rp["Wp"].data_ptr(),
                       rp["Wn"].data_ptr() if need_wn else None, x.data_ptr(), 1, 1 if signed else 0, None, POST_NONE,
                       0.0, out.data_ptr(), B, N, K, s)

        fwd_fused()      # z and the denominators the backward reads
        print(json.dumps({"layer": name, "B": B, "K": K, "N": N, "relu_after": relu, "signed_input": signed,
                          "fwd_chains": chains, "bwd_terms": terms, "fwd_composed": timed(fwd_composed),
                          "fwd_fused": timed(fwd_fused), "bwd_composed": timed(bwd_composed),
                          "bwd_fused": timed(bwd_fused)}))


if __name__ == "__main__":
    main()
