"""CPU reference of the K x K conv entry points (drsa_amd_convk_fwd / _bwd), for the kernel and plan
tests.  No GPU, no kernel knowledge: the chains of include/drsa_amd.h in tests/convk_exact.c (built on
first use with the host gcc and the flags of oracle/Makefile into a temporary directory), and on top
of them the elementwise fp32 torch ops of conv_ref.conv_fwd_ref (pool_mode 0) / conv_bwd_ref (dense g).

Weights are forward-shaped sets [cout][cin][kh][kw]; the device layouts come from engine/plan.py's
packers (_convk_fwd_layout / _convk_bwd_layout), which the plan itself uses.
"""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import torch

from conv_ref import POST_DIV, POST_MASK, POST_NONE, XM_MUL, XM_NONE, XM_SPLIT, _seed, pad32, stab   # noqa: F401
from drsa_audio_amd.engine.plan import _convk_bwd_layout, _convk_fwd_layout   # noqa: F401

KERNELS = [(1, 1), (3, 3), (5, 5), (7, 7), (3, 5), (5, 3), (1, 7)]
PAIRS = [(1, 8), (8, 40), (40, 33)]             # forward cin -> cout: padded, chunk-boundary, odd
MAPS = [(2, 4), (6, 12), (10, 36)]              # the smallest map; no tile multiples (tiles are 8 x 16)
BATCH = 3
EPS = 1e-6
CFLAGS = ["-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-std=c11"]   # oracle/Makefile

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="convk_exact_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libconvk_exact.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "convk_exact.c")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-o", so, src, "-lm"], check=True, capture_output=True)
        L = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int
        L.convk_exact.argtypes = [P, P, P, P, I, I, I, I, I, I, I]
        L.convk_transpose_exact.argtypes = [P, P, P, I, I, I, I, I, I, I]
        L.convk_exact.restype = L.convk_transpose_exact.restype = None
        _lib = L
    return _lib


def _c(t):
    return t.detach().to(torch.float32).contiguous()


def conv(x, w, b=None):
    """x [B][cin][H][W], w [cout][cin][kh][kw] -> [B][cout][H][W]: the forward chain, bias last."""
    x, w = _c(x), _c(w)
    b = None if b is None else _c(b)
    B, cin, H, W = x.shape
    assert w.size(1) == cin and w.size(2) % 2 == 1 and w.size(3) % 2 == 1
    out = torch.empty(B, w.size(0), H, W)
    lib().convk_exact(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), B, cin,
                      w.size(0), H, W, w.size(2), w.size(3))
    return out


def conv_t(g, w):
    """g [B][cout][H][W], w [cout][cin][kh][kw] -> [B][cin][H][W]: the backward chain."""
    g, w = _c(g), _c(w)
    B, cout, H, W = g.shape
    assert w.size(0) == cout
    out = torch.empty(B, w.size(1), H, W)
    lib().convk_transpose_exact(g.data_ptr(), w.data_ptr(), out.data_ptr(), B, cout, w.size(1), H, W, w.size(2),
                                w.size(3))
    return out


def pack_bias(bias3, cout):
    t = torch.zeros(3, pad32(cout))
    t[:, :cout] = bias3
    return t


def convk_fwd_ref(x, sets, bias3, den="none", den_map=None):
    """drsa_amd_convk_fwd: (out, out_den or None); conv_ref.conv_fwd_ref at pool_mode 0."""
    ng = len(sets)
    col = lambda b: b.view(1, -1, 1, 1)    # noqa: E731
    acc0 = conv(x, sets[0])
    z = acc0 + col(bias3[0])
    y = torch.where(torch.isnan(z), z, z.clamp(min=0))
    if den == "none":
        d = None
    elif den == "map":
        d = den_map.unsqueeze(0).expand(x.size(0), -1, -1, -1).contiguous()
    elif ng == 1:
        d = acc0 + col(bias3[1])
    elif ng == 2:
        d = (conv(x, sets[1]) + col(bias3[1])) + col(bias3[2])
    else:
        d = (conv(x.clamp(min=0), sets[1]) + col(bias3[1])) + (conv(x.clamp(max=0), sets[2]) + col(bias3[2]))
    return y, d


def convk_bwd_ref(g, sets, x, den, clones, xmode, post, eps):
    """drsa_amd_convk_bwd: out [Bq][cin][H][W]; conv_ref.conv_bwd_ref with a dense g."""
    t = [conv_t(g, w) for w in sets]
    xq = None if x is None else x.repeat_interleave(clones, 0)
    if xmode == XM_NONE:
        R = t[0]
    elif xmode == XM_MUL:
        R = xq * t[0]
    else:
        R = xq.clamp(min=0) * t[0] + xq.clamp(max=0) * t[1]
    if post == POST_NONE:
        return R
    if post == POST_DIV:
        R = R / stab(den.repeat_interleave(clones, 0), eps)
    return torch.where(xq > 0, R, torch.zeros_like(R))


# ------------------------------------------------------------------ the cases of test_convk_gpu.py
FWD_COMBOS = [(1, "computed"), (2, "computed"), (3, "computed"), (1, "map"), (1, "none"), (3, "none"), (2, "none")]
# (ng, xmode, post, clones): every xmode x post, clones 1 and 3; XM_SPLIT reads two weight groups
BWD_MODES = [(1, XM_NONE, POST_NONE, 1), (1, XM_MUL, POST_DIV, 3), (2, XM_SPLIT, POST_DIV, 1), (1, XM_MUL, POST_MASK, 3),
             (2, XM_NONE, POST_DIV, 1), (2, XM_MUL, POST_NONE, 3), (2, XM_SPLIT, POST_MASK, 3), (1, XM_NONE, POST_MASK, 1),
             (2, XM_SPLIT, POST_NONE, 1)]


def _rotate(options, per_case):
    """(kh, kw, cin, cout, H, W, option) with every kernel x pair and every kernel x map present, and
    ``per_case`` consecutive options per case, rotating: 9 geometry cells per kernel size."""
    cases, i = [], 0
    for kh, kw in KERNELS:
        for a in range(3):
            for b in range(3):
                # a Latin arrangement: the 3 x 3 grid of (pair, map) is covered in full
                for j in range(per_case):
                    cases.append((kh, kw, *PAIRS[a], *MAPS[b], options[(i + j) % len(options)]))
                i += per_case
        i += 1
    return cases


def fwd_cases():
    """(kh, kw, cin, cout, H, W, (ng, den)): every kernel size meets every pair, map and ng."""
    return _rotate(FWD_COMBOS, 1)


def bwd_cases():
    """(kh, kw, cin, cout, H, W, (ng, xmode, post, clones)) with cin -> cout the FORWARD pair."""
    return _rotate(BWD_MODES, 1)


def bwd_one_channel_cases():
    """The backward into one output channel (forward 1 -> 20) is a kernel of its own with chunks of 8 g
    channels: 20 channels are two full chunks and a partial one (the 1 -> 8 pair above is a single chunk)."""
    return [(5, 5, 1, 20, 6, 12, (2, XM_SPLIT, POST_DIV, 1)), (3, 5, 1, 20, 10, 36, (1, XM_MUL, POST_DIV, 3)),
            (7, 7, 1, 20, 2, 4, (1, XM_NONE, POST_NONE, 1)), (1, 1, 1, 20, 18, 20, (2, XM_SPLIT, POST_MASK, 3))]


def fwd_inputs(cin, cout, H, W, kh, kw, ng):
    """BATCH samples with exact zeros, negatives (ng != 2) and for ng = 1 one NaN."""
    g = torch.Generator().manual_seed(_seed(cin, cout, H, W, kh, kw, ng))
    x = torch.randn(BATCH, cin, H, W, generator=g) * 1.5
    if ng == 2:
        x = x.abs()                          # ng = 2 is the Gamma forward on x >= 0 (ABI contract)
    x[0, :, H - 2:, W - 3:] = 0.0
    x[1, :, :1, 1:3] = 0.0
    if ng == 1:
        x[1, 0, 1, 2] = float("nan")
    w = torch.randn(cout, cin, kh, kw, generator=g) / (kh * kw * cin) ** 0.5
    sets = [w, w + 0.25 * w.clamp(min=0), w + 0.25 * w.clamp(max=0)][:ng]
    bias3 = torch.randn(3, cout, generator=g) * 0.1
    den_map = torch.rand(cout, H, W, generator=g) + 0.5
    return x, sets, bias3, den_map


def bwd_inputs(cin, cout, H, W, kh, kw, ng, clones):
    """Dense g, weight sets, x (exact zeros and negatives) and den (both signs, exact zeros) for the
    forward pair cin -> cout; at the corner pixel sample 0 has x > 0 over a negative den, sample 1 x = 0."""
    g = torch.Generator().manual_seed(_seed(cin, cout, H, W, kh, kw, ng, clones))
    S = BATCH
    gin = torch.randn(S * clones, cout, H, W, generator=g)
    w = torch.randn(cout, cin, kh, kw, generator=g) / (kh * kw * cout) ** 0.5
    sets = [w + 0.25 * w.clamp(min=0), w + 0.25 * w.clamp(max=0)][:ng]
    x = torch.randn(S, cin, H, W, generator=g)
    x[torch.rand(S, cin, H, W, generator=g) < 0.25] = 0.0
    den = torch.randn(S, cin, H, W, generator=g)
    den[torch.rand(den.shape, generator=g) < 0.1] = 0.0
    x[0, :, -1, -1] = x[0, :, -1, -1].abs() + 0.25
    x[1, :, -1, -1] = 0.0
    den[..., -1, -1] = -0.01
    den[..., 0, 0] = 0.0
    return gin, sets, x, den


# ------------------------------------------------------------------ nets with K x K convs
def toy_k(kernels, seed=0):
    """lrp_common.toy() with its i-th conv (features.0, .3, .6, .9, .12) replaced by a 'same' conv of
    kernels[i] (None: the 3x3 conv stays); the channel counts and everything else are toy()'s."""
    import torch.nn as nn
    from lrp_common import toy
    net = toy(seed)
    convs = [(n, m) for n, m in net.features.named_children() if isinstance(m, nn.Conv2d)]
    assert len(convs) == len(kernels)
    torch.manual_seed(seed + 1)
    for (name, m), k in zip(convs, kernels):
        if k is not None:
            setattr(net.features, name, nn.Conv2d(m.in_channels, m.out_channels, k, padding="same"))
    return net.eval()


TOY_NETS = {"all5x5": [(5, 5)] * 5, "all3x5": [(3, 5)] * 5, "first7x7": [(7, 7), None, None, None, None]}
