"""CPU reference of the 3x3 conv entry points (drsa_amd_conv_fwd / _bwd and their den_map, den_ring
and bf16 forms), for the kernel tests.  No GPU, no kernel knowledge: it restates the ABI of
include/drsa_amd.h and csrc/lrp_conv.h on top of the pinned-order primitives of oracle/lrp_exact.c
(lrp_ref.ExactOps.conv / conv_t: every output one k-ordered fp32 fma chain, k = ci * 9 + tap),
followed by elementwise fp32 torch ops.  The fp32 kernels are specified to compute exactly this, so
the tests built on it compare with torch.equal.

Weights are given as forward-shaped sets [cout][cin][3][3] (the conv that maps cin -> cout
channels); ``pack_fwd`` / ``pack_bwd`` / ``pack_bf16`` lay them out for the device as
engine/plan.py's prepare step (_prepare_conv) does.  A backward call of the ABI names its channels the other way
round: its ``cin`` is the forward cout (the channels of g), its ``cout`` the forward cin.

The keyword arguments ``pad``, ``tie``, ``mask_ge`` and ``stab_plus`` select deliberately WRONG
variants (replicate padding, last maximum wins, x >= 0 in the post mask, +eps for negative
denominators).  tests/test_conv_ref_cpu.py uses them to show that the test inputs can tell each of
those mistakes from the right answer; nothing else may pass them.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import lrp_ref
from drsa_audio_amd.engine.plan import _bf16_layout

XM_NONE, XM_MUL, XM_SPLIT = 0, 1, 2
POST_NONE, POST_DIV, POST_MASK = 0, 1, 2

_M = nn.Conv2d(1, 1, 3, padding=1)      # ExactOps reads only its kernel size, stride and padding


def pad32(c):
    return (c + 31) // 32 * 32


def cin_pad(c):
    return 1 if c == 1 else pad32(c)


# ------------------------------------------------------------------ device weight layouts
def pack_fwd(sets, bf16=False):
    """[ng][9 * cin_p][cout_p] fp32, row k = ci * 9 + ky * 3 + kx (drsa_amd_conv_fwd)."""
    cout, cin = sets[0].shape[:2]
    cin_p, cout_p = (pad32(cin) if bf16 else cin_pad(cin)), pad32(cout)
    t = torch.zeros(len(sets), cin_p, 3, 3, cout_p)
    for s, w in enumerate(sets):
        t[s, :cin, :, :, :cout] = w.permute(1, 2, 3, 0)
    return t.reshape(len(sets), 9 * cin_p, cout_p).contiguous()


def pack_bwd(sets):
    """The transposed conv as a 'same' conv over g: [ng][9 * pad32(cout)][pad32(cin)] fp32, row
    k = co * 9 + tap with the taps flipped (drsa_amd_conv_bwd)."""
    cout, cin = sets[0].shape[:2]
    t = torch.zeros(len(sets), pad32(cout), 3, 3, pad32(cin))
    for s, w in enumerate(sets):
        t[s, :cout, :, :, :cin] = w.flip(2, 3).permute(0, 2, 3, 1)
    return t.reshape(len(sets), 9 * pad32(cout), pad32(cin)).contiguous()


def pack_bf16(wf):
    """A packed fp32 tensor [ng][9 * a][b] (a, b padded to 32) in the bf16 device layout."""
    return _bf16_layout(wf, wf.size(1) // 9, wf.size(2))


def pack_bias(bias3, cout):
    t = torch.zeros(3, pad32(cout))
    t[:, :cout] = bias3
    return t


# ------------------------------------------------------------------ primitives
def _memo(memo, key, fn):
    """fn() kept in the caller's dict: the references of one set of inputs share their convs."""
    if memo is None:
        return fn()
    if key not in memo:
        memo[key] = fn()
    return memo[key]


def _conv(x, w, pad="zero"):
    if pad == "replicate":
        return lrp_ref.ExactOps.conv(_M, F.pad(x, (1, 1, 1, 1), mode="replicate"), w, None)[..., 1:-1, 1:-1].contiguous()
    return lrp_ref.ExactOps.conv(_M, x, w, None)


def _conv_t(g, w, pad="zero"):
    if pad == "replicate":
        gp = F.pad(g, (1, 1, 1, 1), mode="replicate")
        return lrp_ref.ExactOps.conv_t(_M, None, w, gp)[..., 1:-1, 1:-1].contiguous()
    return lrp_ref.ExactOps.conv_t(_M, None, w, g)


def windows(t, pw):
    """[B, C, H, W] -> [B, C, H/2, W/pw, 2 * pw]: the 2 x pw pool windows, row-major inside."""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // pw, pw).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // pw, 2 * pw)


def pool(y, pw, tie="first"):
    """2 x pw max-pool and its argmax byte: the first maximum in row-major window order wins a
    tie, a NaN wins over a non-NaN (torch max_pool2d)."""
    win = windows(y, pw)
    m, am = win[..., 0].clone(), torch.zeros(win.shape[:-1], dtype=torch.uint8)
    for s in range(1, 2 * pw):
        v = win[..., s]
        take = ((v >= m) if tie == "last" else (v > m)) | (torch.isnan(v) & ~torch.isnan(m))
        m = torch.where(take, v, m)
        am = torch.where(take, torch.full_like(am, s), am)
    return m, am


def at_argmax(full, am, pw):
    return torch.gather(windows(full, pw), -1, am.long().unsqueeze(-1)).squeeze(-1)


def unpool(g, am, pw, clones=1):
    """g [Bq, C, H/2, W/pw] scattered to its argmax pixels: [Bq, C, H, W]; row q of g belongs to
    sample q // clones of am."""
    Bq, C, H2, Wp = g.shape
    amq = am.repeat_interleave(clones, 0).long()
    d = torch.zeros(Bq, C, H2, Wp, 2 * pw)
    d.scatter_(-1, amq.unsqueeze(-1), g.unsqueeze(-1))
    return d.reshape(Bq, C, H2, Wp, 2, pw).permute(0, 1, 2, 4, 3, 5).reshape(Bq, C, 2 * H2, pw * Wp).contiguous()


# ------------------------------------------------------------------ forward
def conv_fwd_ref(x, sets, bias3, pool_mode, den="none", den_map=None, pad="zero", tie="first", memo=None):
    """drsa_amd_conv_fwd: (out, out_amax or None, out_den or None).
    sets: ng forward-shaped weight sets; bias3 [3][cout] = (b0, b1, b2); pool_mode 0 / 1 / 2;
    den: "none", "computed" (by ng) or "map" (den_map [cout][H][W]); memo: a dict of the caller's
    that keeps the convs of these x and sets."""
    ng = len(sets)
    col = lambda b: b.view(1, -1, 1, 1)
    conv = lambda s, xin: _memo(memo, ("conv", s, pad), lambda: _conv(xin, sets[s], pad))
    acc0 = conv(0, x)
    z = acc0 + col(bias3[0])
    y = torch.where(torch.isnan(z), z, z.clamp(min=0))
    if den == "none":
        d = None
    elif den == "map":
        d = den_map.unsqueeze(0).expand(x.size(0), -1, -1, -1).contiguous()
    elif ng == 1:
        d = acc0 + col(bias3[1])
    elif ng == 2:
        d = (conv(1, x) + col(bias3[1])) + col(bias3[2])
    else:
        d = (conv(1, x.clamp(min=0)) + col(bias3[1])) + (conv(2, x.clamp(max=0)) + col(bias3[2]))
    if not pool_mode:
        return y, None, d
    pw = 4 if pool_mode == 2 else 2
    m, am = pool(y, pw, tie)
    return m, am, None if d is None else at_argmax(d, am, pw)


# ------------------------------------------------------------------ backward
def stab(t, eps, stab_plus=False):
    e = torch.tensor(eps, dtype=torch.float32)
    return t + (e if stab_plus else torch.where(t >= 0, e, -e))


def conv_bwd_ref(g, g_amax, pool_w, sets, x, den, clones, xmode, post, eps, den_shared=False, pad="zero",
                 mask_ge=False, stab_plus=False, memo=None):
    """drsa_amd_conv_bwd (den_shared: drsa_amd_conv_bwd_den_map): out [Bq][cin][H][W].
    g [Bq][cout][H][W], or at 2 x pool_w pool resolution with g_amax [S][cout][H/2][W/pool_w];
    sets: ng forward-shaped weight sets; x [S][cin][H][W]; den like x, or [cin][H][W] if shared;
    memo: a dict of the caller's that keeps the transposed convs of these g and sets."""
    gf = g if g_amax is None else unpool(g, g_amax, pool_w, clones)
    t = [_memo(memo, ("conv_t", s, pad), lambda: _conv_t(gf, w, pad)) for s, w in enumerate(sets)]
    xq = None if x is None else x.repeat_interleave(clones, 0)
    if xmode == XM_NONE:
        R = t[0]
    elif xmode == XM_MUL:
        R = xq * t[0]
    else:
        R = xq.clamp(min=0) * t[0] + xq.clamp(max=0) * t[1]
    if post == POST_NONE:
        return R
    live = (xq >= 0) if mask_ge else (xq > 0)
    if post == POST_DIV:
        dq = den.unsqueeze(0).expand_as(R) if den_shared else den.repeat_interleave(clones, 0)
        R = R / stab(dq, eps, stab_plus)
    return torch.where(live, R, torch.zeros_like(R))


def ring_of(den):
    """The compact border ring of drsa_amd_conv_fwd_den_ring for den [S][C][H][W] (pooled
    resolution): per plane [row 0 | row H-1 | rows 1..H-2 x (columns 0..3, W-4..W-1)]."""
    S, C, H, W = den.shape
    side = torch.cat([den[..., 1:-1, :4], den[..., 1:-1, -4:]], -1).reshape(S, C, -1)
    return torch.cat([den[..., 0, :], den[..., -1, :], side], -1).contiguous()


# ------------------------------------------------------------------ the cases of test_conv_edges_gpu.py
# Kept here, without a GPU import, so that tests/test_conv_ref_cpu.py can check the same list
# (queries, inputs) on a machine without a GPU.
PAIRS = [(1, 32), (1, 64), (20, 32), (32, 48), (64, 64), (64, 100), (100, 128), (128, 128)]   # forward cin -> cout
SHAPES = [(12, 40), (6, 12), (10, 20), (6, 36)]
SHAPES_SCALAR = [(6, 10), (12, 34)]          # W % 4 != 0: pooled forward only
SHAPES_P4 = [(12, 48), (12, 80)]             # W / 4 % 4 == 0: the 2x4 pool
RING_SHAPES = [(2, 8), (6, 24), (10, 40)]    # pooled sizes of drsa_amd_conv_bwd_den_ring
BF_PAIRS = [(32, 32), (64, 100), (100, 128)]
BF_SHAPES = [(12, 40), (6, 12), (10, 20), (12, 80)]
EPS = 1e-6
SMALL_WG = 512                               # lrp_conv.hip DRSA_CONV_SMALL_WG
# (ng, xmode, post, clones) of drsa_amd_conv_bwd
BWD_MODES = [(1, XM_NONE, POST_NONE, 1), (1, XM_MUL, POST_DIV, 2), (2, XM_SPLIT, POST_DIV, 1), (1, XM_MUL, POST_MASK, 5)]
FWD_COMBOS = [(1, "computed"), (2, "computed"), (3, "computed"), (1, "map"), (1, "none"), (3, "none"), (2, "none")]


def tile_width(fwd, cin, cout, W, bf16=False):
    """Tile width of the tile rule (csrc/lrp_conv_config.h wide_tile_w(): 8 x 32, 8 x 16 or 8 x 8 tiles at
    W >= 32, 8 x 8 below; the tables hold exactly those two per kernel set); cin -> cout are the
    call's own channel counts (a backward call: g channels -> output channels).  An 8-wide entry
    runs as 4 x 8 tiles while its grid has fewer than SMALL_WG workgroups (fp32 only)."""
    ci, co = pad32(cin), pad32(cout)
    if W < 32:
        return 8
    if bf16:
        return 32
    if fwd:
        return 8 if co == 128 else 16 if co == 64 else 32
    return 16 if (co == 64 and ci <= 128) or co == 128 else 32


def batches(fwd, cin, cout, H, W, clones=1, bf16=False):
    """Batch sizes (rows of the launch grid) a case runs at: 3 * clones and, where an 8 x 8 entry
    serves the shape, the smallest multiple of clones that makes the 8 x 8 kernel itself run."""
    out = [3 * clones]
    if tile_width(fwd, cin, cout, W, bf16) == 8 and not bf16:
        tiles = ((H + 7) // 8) * ((W + 7) // 8)
        rows = (SMALL_WG + tiles - 1) // tiles
        out.append((rows + clones - 1) // clones * clones)
    return out


def fwd_cases():
    """(cin, cout, H, W, ng, pool, den).  Per (pair, shape, pool) two of the seven (ng, den) combos,
    rotating; the 2x4 pool (64 -> 64 only) with every ng and the map."""
    cases, i = [], 0
    for cin, cout in PAIRS:
        for H, W in SHAPES + SHAPES_SCALAR:
            for pool_mode in ((1,) if W % 4 else (0, 1)):
                for j in (i, i + 3):
                    ng, den = FWD_COMBOS[j % 7]
                    cases.append((cin, cout, H, W, ng, pool_mode, den))
                i += 1
    for H, W in SHAPES_P4:
        cases += [(64, 64, H, W, ng, 2, den) for ng, den in ((1, "computed"), (2, "computed"), (3, "computed"), (1, "map"))]
        cases += [(64, 64, H, W, 1, 1, "computed"), (64, 64, H, W, 3, 0, "computed")]
    cases.append((32, 48, 6, 12, 1, 1, "map_unaligned"))
    cases.append((1, 32, 6, 12, 1, 1, "map_unaligned"))
    return cases


def bwd_cases():
    """(cin, cout, H, W, sparse, mode) with cin -> cout the FORWARD pair (the call mirrors it).
    Per (pair, shape, sparse) two of the four modes, rotating."""
    cases, i = [], 0
    for cin, cout in PAIRS:
        for H, W in SHAPES:
            for sparse in (0, 1):
                for j in (i, i + 2):
                    cases.append((cin, cout, H, W, sparse, BWD_MODES[j % 4]))
                i += 1
            i += 1
    return cases


def den_map_cases():
    """(cin, cout, H, W, pool_w, xmode); pool_w 0 = dense g.  The 2x4 fold is built for 64 -> 64."""
    cases = []
    for H, W in SHAPES_P4:
        cases += [(64, 64, H, W, 4, XM_NONE), (64, 64, H, W, 4, XM_MUL)]
    for k, (H, W) in enumerate(SHAPES_P4 + [(12, 40)]):
        for cin, cout in ((64, 64), (32, 48), (1, 64), (100, 128)):
            cases.append((cin, cout, H, W, 2, (XM_NONE, XM_MUL)[(k + cin) % 2]))
    cases += [(64, 64, 12, 40, 0, XM_NONE), (20, 32, 12, 40, 0, XM_MUL), (1, 32, 12, 40, 0, XM_NONE)]
    return cases


def den_ring_cases():
    """(cin, cout, H, W, sparse, xmode) at the pooled sizes H x W."""
    cases, i = [], 0
    for cin, cout in ((32, 48), (64, 64), (64, 100)):
        for H, W in RING_SHAPES:
            for sparse in (0, 1):
                cases.append((cin, cout, H, W, sparse, (XM_MUL, XM_NONE)[i % 2]))
                i += 1
            i += 1
    return cases


def bf16_fwd_cases():
    """(cin, cout, H, W, ng, pool)."""
    cases, i = [], 0
    for cin, cout in BF_PAIRS:
        for H, W in BF_SHAPES:
            for pool_mode in (0, 1):
                cases.append((cin, cout, H, W, 1 + i % 3, pool_mode))
                i += 1
    for H, W in BF_SHAPES:
        cases += [(64, 64, H, W, 1 + (H + W) % 3, 2)] if W % 4 == 0 else []
    return cases


def bf16_bwd_cases():
    """(cin, cout, H, W, pool_w) with the forward pair; pool_w 0 = dense g, 2 = drsa_amd_conv_bwd_bf16
    with g_amax, 4 and -2 = drsa_amd_conv_bwd_bf16_pw at pool width 4 and 2."""
    cases = [(cin, cout, H, W, pw) for cin, cout in BF_PAIRS for H, W in BF_SHAPES for pw in (0, 2)]
    cases += [(64, 64, H, W, 4) for H, W in BF_SHAPES]
    cases += [(64, 64, 12, 80, -2), (64, 64, 6, 12, -2)]
    return cases


def _seed(*k):
    s = 17
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def fwd_inputs(cin, cout, H, W, ng):
    """Two distinct samples with exact zeros (ReLU plateaus: ties in the pool windows, among them the
    corner window of sample 0), negatives (ng != 2), and for ng = 1 one NaN."""
    g = torch.Generator().manual_seed(_seed(cin, cout, H, W, ng))
    x = torch.randn(2, cin, H, W, generator=g) * 1.5
    if ng == 2:
        x = x.abs()                          # ng = 2 is the Gamma forward on x >= 0 (ABI contract)
    x[0, :, H - 3:, W - 5:] = 0.0
    x[1, :, 1:4, 3:8] = 0.0
    if ng == 1:
        x[1, 0, 2, 3] = float("nan")
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    sets = [w, w + 0.25 * w.clamp(min=0), w + 0.25 * w.clamp(max=0)][:ng]
    bias3 = torch.randn(3, cout, generator=g) * 0.1
    den_map = torch.rand(cout, H, W, generator=g) + 0.5
    return x, sets, bias3, den_map


def bwd_inputs(cin, cout, H, W, ng, pool_w, clones, shared_den=False):
    """g (dense for pool_w = 0, else pool-sparse with its argmax), weight sets, x and den for the
    forward pair cin -> cout.  x has exact zeros and negatives; den has both signs and exact zeros;
    at the corner pixel sample 0 has x > 0 over a negative den and sample 1 has x = 0, and every
    sparse corner cell of channel 0 points at the corner pixel."""
    g = torch.Generator().manual_seed(_seed(cin, cout, H, W, ng, pool_w, clones, shared_den))
    Bq = 2 * clones
    if pool_w:
        gin = torch.randn(Bq, cout, H // 2, W // pool_w, generator=g)
        am = torch.randint(0, 2 * pool_w, (2, cout, H // 2, W // pool_w), generator=g, dtype=torch.uint8)
        am[:, 0, -1, -1] = 2 * pool_w - 1
    else:
        gin, am = torch.randn(Bq, cout, H, W, generator=g), None
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cout) ** 0.5
    sets = [w + 0.25 * w.clamp(min=0), w + 0.25 * w.clamp(max=0)][:ng]
    x = torch.randn(2, cin, H, W, generator=g)
    x[torch.rand(2, cin, H, W, generator=g) < 0.25] = 0.0
    den = torch.randn((cin, H, W) if shared_den else (2, cin, H, W), generator=g)
    den[torch.rand(den.shape, generator=g) < 0.1] = 0.0
    x[0, :, -1, -1] = x[0, :, -1, -1].abs() + 0.25
    x[0, :, -1, 0] = x[0, :, -1, 0].abs() + 0.25
    x[0, :, 0, -1] = x[0, :, 0, -1].abs() + 0.25
    x[1, :, -1, -1] = 0.0
    x[1, :, -1, 1] = 0.0
    x[1, :, 1, -1] = 0.0
    den[..., -1, -1] = -0.01
    den[..., -1, 0] = -0.02
    den[..., 0, -1] = -0.03
    den[..., -1, -2] = 0.0
    return gin, am, sets, x, den


def ring_inputs(cin, cout, H, W, sparse, clones):
    """bwd_inputs at a pooled size whose den is a WSquare / Flat map's copy: one value per channel
    off the border ring of float4 groups, anything on it.  Returns (..., den_full, den_ring, c4)."""
    gin, am, sets, x, den = bwd_inputs(cin, cout, H, W, 1, 2 if sparse else 0, clones)
    const = 0.5 + torch.arange(cin, dtype=torch.float32) / 64
    inner = torch.zeros(H, W, dtype=torch.bool)
    inner[1:-1, 4:-4] = True
    den = torch.where(inner, const.view(1, -1, 1, 1).expand_as(den), den)
    return gin, am, sets, x, den, ring_of(den), const.view(-1, 1).expand(-1, 4).contiguous()
