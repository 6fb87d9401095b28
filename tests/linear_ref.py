"""CPU reference of the dense-head entry points (drsa_amd_linear_fwd / _bwd, drsa_amd_linear_rule_fwd /
_bwd; csrc/linear.hip, csrc/linear_rules.hip), with the inputs and the case lists of
tests/test_linear_gpu.py.  No GPU, no kernel knowledge: the oracle's exact primitives
(lrp_ref.ExactOps.linear / .matmul: one k-ascending fp32 fma chain from +0 per output, the bias added
last) and on top of them elementwise fp32 torch steps in the order include/drsa_amd.h documents, one
rounding per operation, no fma, IEEE division.  tests/test_linear_ref_cpu.py checks this file itself.

The primitives below (chain, matmul, stab, pos, neg, keep) are module attributes that every reference
reads at call time, so that test_linear_ref_cpu.py can swap one for a wrong variant and show that the
chosen inputs tell the two apart.
"""
import functools

import torch

import lrp_ref
from conv_ref import POST_DIV, POST_MASK, POST_NONE, XM_MUL, XM_NONE, _seed   # noqa: F401
from drsa_audio_amd.engine.parse import dense_rule_params
from drsa_audio_amd.zennit.rules import Flat, Gamma, WSquare, ZPlus

EPS, EPS_POST = 1e-6, 2.5e-6
GAMMA = 0.25


# ------------------------------------------------------------------ primitives
def chain(x, W, b):
    """x [M][K], W [N][K], b [N] or None -> [M][N]: fma chain over k ascending from +0, then + b."""
    return lrp_ref.ExactOps.linear(x, W, b)


def matmul(g, W):
    """g [M][K], W [K][N] -> [M][N]: fma chain over k ascending from +0."""
    return lrp_ref.ExactOps.matmul(g, W)


def stab(t, e):
    """t + (e if t >= 0 else -e): NaN passes through, -0 counts as >= 0."""
    e = torch.tensor(e, dtype=torch.float32)
    return t + torch.where(t >= 0, e, -e)


def pos(x):
    return x.clamp(min=0)       # NaN stays NaN


def neg(x):
    return x.clamp(max=0)


def keep(x):
    """The post step's mask."""
    return x > 0


def relu(z):
    zero = torch.zeros_like(z)
    return torch.where(z > 0, z, torch.where(torch.isnan(z), z, zero))


# ------------------------------------------------------------------ the four entry points
def linear_fwd_ref(x, W, b):
    """drsa_amd_linear_fwd: (z, relu(z))."""
    z = chain(x, W, b)
    return z, relu(z)


def _r0(R, cls, one_hot, z, relu_mask):
    """The relevance entering the layer: R, or the class seed; through the ReLU mask."""
    zero = torch.zeros_like(z)
    if cls is not None:
        hit = torch.arange(z.size(1))[None, :] == cls.long()[:, None]
        R = torch.where(hit, torch.ones_like(z) if one_hot else z, zero)
    if relu_mask:
        R = torch.where(z > 0, R, zero)
    return R


def _post(Rin, x, den, post, eps_post):
    if post == POST_NONE:
        return Rin
    if post == POST_DIV:
        Rin = Rin / stab(den, eps_post)
    return torch.where(keep(x), Rin, torch.zeros_like(Rin))


def linear_bwd_ref(R, cls, one_hot, z, relu_mask, rule_eps, eps, W, x, xmode, den, post, eps_post):
    """drsa_amd_linear_bwd: out [M][Kin]; W [Nout][Kin], z / R [M][Nout], x / den [M][Kin]."""
    R0 = _r0(R, cls, one_hot, z, relu_mask)
    g = R0 / stab(z, eps) if rule_eps else R0
    t = matmul(g, W)
    Rin = x * t if xmode == XM_MUL else t
    return _post(Rin, x, den, post, eps_post)


def rule_fwd_ref(x, W, Wp, Wn, b, bp, bn, signed, want_den_n):
    """drsa_amd_linear_rule_fwd: (z, relu(z), den_p, den_n or None)."""
    z, a = linear_fwd_ref(x, W, b)
    xp, xn = (pos(x) if signed else x), neg(x)
    zero = torch.tensor(0.0)
    term = lambda v, w, bias: chain(v, w, bias) if bias is not None else chain(v, w, None) + zero   # noqa: E731
    den_p = term(xp, Wp, bp) + (term(xn, Wn, None) if signed else zero)
    den_n = None
    if want_den_n:
        den_n = term(xp, Wn, bn) + (term(xn, Wp, None) if signed else zero)
    return z, a, den_p, den_n


def rule_bwd_ref(R, cls, one_hot, z, relu_mask, den_p, den_n, den_bcast, zsign, eps, Wp, Wn, x, xmul, signed, den, post,
                 eps_post):
    """drsa_amd_linear_rule_bwd: out [M][Kin]; den_p / den_n [M][Nout], or [Nout] under den_bcast."""
    R0 = _r0(R, cls, one_hot, z, relu_mask)
    zero = torch.zeros_like(z)
    row = (lambda d: d[None, :].expand_as(z)) if den_bcast else (lambda d: d)
    gp = (torch.where(z > 0, R0, zero) if zsign else R0) / stab(row(den_p), eps)
    t0 = matmul(gp, Wp)
    if not xmul:
        Rin = t0
    else:
        xp, xn = (pos(x) if signed else x), neg(x)
        Rin = xp * t0
        if signed:
            Rin = Rin + xn * matmul(gp, Wn)
        if den_n is not None:
            gn = torch.where(z < 0, R0, zero) / stab(row(den_n), eps)
            Rin = Rin + xp * matmul(gn, Wn)
            if signed:
                Rin = Rin + xn * matmul(gn, Wp)
    return _post(Rin, x, den, post, eps_post)


# ------------------------------------------------------------------ shapes
MS = (1, 17, 33, 50)                      # one row; a second 16-row tile of one row; a second 32-row workgroup of one
#                                           row; a partial second wave row
NS = (3, 20, 33, 48)                      # forward N, backward Kin
FWD_KS = (3, 31, 32, 33, 100, 128, 130, 132, 260, 384)
BWD_KS = (1, 3, 31, 33, 70)               # the backward GEMM's K = Nout


def _grid(ks):
    """(M, n, K): every M x K pair, n rotating so that every M and every K meets every n; the last is 50 x 48 x max K."""
    return [(M, NS[(mi + ki - len(ks) + 1) % 4], K) for ki, K in enumerate(ks) for mi, M in enumerate(MS)]


def fwd_shapes():
    """(M, N, K)."""
    return _grid(FWD_KS)


def bwd_shapes():
    """(M, Nout, Kin)."""
    return [(M, K, n) for M, n, K in _grid(BWD_KS)]


# ------------------------------------------------------------------ modes
LIN_FWD_MODES = [(1, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)]         # (bias, relu_out, nan)
RULE_FWD_INSTS = [("gamma", 1, 1), ("gamma", 1, 0), ("gamma", 0, 1), ("gamma", 0, 0), ("zplus", 1, 0), ("zplus", 0, 0)]
RULE_FWD_MODES = LIN_FWD_MODES                                                  # (biases, relu_out, nan)
# (source, relu_mask, rule_eps, xmode, post): every source x post, every relu_mask x rule_eps x xmode
LIN_BWD_MODES = [("R", 0, 1, XM_MUL, POST_NONE), ("R", 1, 0, XM_NONE, POST_DIV), ("R", 0, 1, XM_NONE, POST_MASK),
                 ("cls", 1, 1, XM_MUL, POST_DIV), ("cls", 0, 0, XM_MUL, POST_MASK), ("cls", 0, 1, XM_NONE, POST_NONE),
                 ("onehot", 0, 1, XM_MUL, POST_MASK), ("onehot", 1, 0, XM_NONE, POST_NONE),
                 ("onehot", 0, 0, XM_MUL, POST_DIV), ("R", 1, 1, XM_MUL, POST_DIV), ("R", 0, 0, XM_NONE, POST_NONE),
                 ("R", 1, 1, XM_NONE, POST_MASK), ("R", 1, 0, XM_MUL, POST_NONE)]
# (rule, signed, negden): the four instantiations under Gamma (zsign = 1), ZPlus (zsign = 0), and the
# constant-denominator rules (den_bcast = 1, xmul = 0, no Wn)
RULE_BWD_INSTS = [("gamma", 1, 1), ("gamma", 1, 0), ("gamma", 0, 1), ("gamma", 0, 0), ("zplus", 1, 0), ("zplus", 0, 0),
                  ("wsquare", 0, 0), ("flat", 0, 0)]
# (source, relu_mask, post): every source x post, both mask values on every source and every post
RULE_BWD_MODES = [("R", 0, POST_NONE), ("R", 1, POST_DIV), ("R", 0, POST_MASK), ("cls", 1, POST_NONE),
                  ("cls", 0, POST_DIV), ("cls", 1, POST_MASK), ("onehot", 0, POST_NONE), ("onehot", 1, POST_DIV),
                  ("onehot", 0, POST_MASK)]


def kernel_of(entry, K=None):
    """The kernel family a call is expected to reach (aligned pointers): what the shape coverage is counted over."""
    if entry in ("linear_fwd", "linear_rule_fwd"):
        return "long" if K % 4 == 0 and K >= 128 else "short"
    return "bwd"


# ------------------------------------------------------------------ inputs
def _plant(t, plan):
    """Write plan's ((row, col), value) into distinct cells of t; cells out of range or taken are skipped."""
    used, (M, N) = set(), t.shape
    for (r, c), v in plan:
        r, c = (r if r >= 0 else M + r), (c if c >= 0 else N + c)
        if 0 <= r < M and 0 <= c < N and (r, c) not in used:
            used.add((r, c))
            t[r, c] = v
    return t


_RULES = {"gamma": Gamma(gamma=GAMMA, stabilizer=EPS), "zplus": ZPlus(stabilizer=EPS),
          "wsquare": WSquare(stabilizer=EPS), "flat": Flat(stabilizer=EPS)}


def _rules(W, b, kinds=tuple(_RULES)):
    """The plan's own constants (engine.parse.dense_rule_params) per rule."""
    return {k: dense_rule_params(W, b, _RULES[k]) for k in kinds}


def _weights(g, n, k):
    W = torch.randn(n, k, generator=g) / k ** 0.5
    W[0, :min(3, k)] = 0.0
    b = torch.randn(n, generator=g) * 0.1
    b[0] = abs(b[0]) + 0.05
    if n > 1:
        b[-1] = -abs(b[-1]) - 0.05
    return W, b


@functools.lru_cache(maxsize=None)
def fwd_inputs(M, N, K, signed):
    """x [M][K] with exact zeros (both signs when signed, else >= 0), xnan = x with one NaN in the last row,
    W [N][K], b [N], and the plan's rule constants with (rp) and without (rp0) the bias."""
    g = torch.Generator().manual_seed(_seed(M, N, K, signed, 1))
    x = torch.randn(M, K, generator=g) * 1.5
    if not signed:
        x = x.abs()
    x[torch.rand(M, K, generator=g) < 0.2] = 0.0
    _plant(x, [((-1, K // 2), 0.7), ((0, 0), 0.0), ((-1, -1), -0.9 if signed else 0.4), ((0, K // 2), -0.3 if signed else 0.0)])
    xnan = x.clone()
    xnan[-1, K // 2] = float("nan")
    W, b = _weights(g, N, K)
    kinds = ("gamma", "zplus")
    return dict(x=x, xnan=xnan, W=W, b=b, rp=_rules(W, b, kinds), rp0=_rules(W, None, kinds))


def _den_like(g, M, N):
    """A denominator: both signs, exact zeros, -0.0, magnitudes below EPS, in the last row and in the last column.
    Against bwd_inputs' z, the last row has a zero under z < 0 (column 1), one under z > 0 (column 4) and a
    negative value under z > 0 (the corner)."""
    d = torch.randn(M, N, generator=g)
    d[torch.rand(M, N, generator=g) < 0.1] = 0.0
    return _plant(d, [((-1, -1), -0.4), ((-1, 1), 0.0), ((-1, 0), -0.0), ((-1, 2), 3e-7), ((-1, 4), 0.0), ((-1, 3), -3e-7),
                      ((-1, 5), 0.6),
                      ((0, -1), -3e-7), ((1, -1), 0.0), ((2, -1), -0.0), ((3, -1), 3e-7), ((4, -1), 0.5), ((5, -1), -0.8)])


@functools.lru_cache(maxsize=None)
def bwd_inputs(M, Nout, Kin, signed):
    """R, cls, z, den_p, den_n [M][Nout]; x, den [M][Kin]; W [Nout][Kin], b; rule constants with and without b."""
    g = torch.Generator().manual_seed(_seed(M, Nout, Kin, signed, 2))
    R = torch.randn(M, Nout, generator=g)
    _plant(R, [((-1, -1), -0.8), ((0, 0), 0.9), ((-1, 1), 0.5), ((0, -1), -0.6)])
    z = torch.randn(M, Nout, generator=g)
    z[torch.rand(M, Nout, generator=g) < 0.1] = 0.0
    # z > 0 at the last row's seed class (column 0), so that the seeded row is not blank under a z > 0 mask
    _plant(z, [((-1, -1), 0.8), ((-1, 0), 0.5), ((-1, 1), -0.6), ((-1, 2), 0.0), ((-1, 3), -0.0), ((-1, 4), 0.3),
               ((0, -1), -0.7), ((1, -1), 0.0), ((2, -1), -0.0), ((3, -1), 0.4)])
    cls = torch.randint(0, Nout, (M,), generator=g, dtype=torch.int32)
    cls[0] = Nout - 1
    if M > 1:
        cls[-1] = 0
    x = torch.randn(M, Kin, generator=g)
    if not signed:
        x = x.abs()
    x[torch.rand(M, Kin, generator=g) < 0.25] = 0.0
    # the corner stays positive (a zero there would blank the only cell of a one-cell last tile): the exact zeros
    # sit next to it in the last row and the last column
    _plant(x, [((-1, -1), 0.7), ((-1, -2), 0.0), ((-1, 0), -0.6 if signed else 0.3), ((-1, 1), 0.6), ((0, -1), 0.9),
               ((1, -1), 0.0), ((2, -1), -0.5 if signed else 0.0)])
    W, b = _weights(g, Nout, Kin)
    den_p, den_n = _den_like(g, M, Nout), _den_like(g, M, Nout)
    # where a denominator is (near) zero, R is scaled by 2^-20: the quotient R / stab(0) stays O(1), so a row that
    # holds such a cell (the last one does) still shows a one-ulp mistake anywhere in its chain
    tiny = (z.abs() < 1e-5) | (den_p.abs() < 1e-5) | (den_n.abs() < 1e-5)
    R = torch.where(tiny, R * 2.0 ** -20, R)
    return dict(R=R, cls=cls, z=z, den_p=den_p, den_n=den_n, x=x, den=_den_like(g, M, Kin), W=W, b=b,
                rp=_rules(W, b), rp0=_rules(W, None))


# ------------------------------------------------------------------ cases: ABI arguments and the reference
def lin_fwd_case(shape, mode):
    """(arguments of drsa_amd_linear_fwd as CPU tensors / None, {output name: reference or None})."""
    (M, N, K), (bias, want_relu, nan) = shape, mode
    d = fwd_inputs(M, N, K, 1)
    a = dict(x=d["xnan"] if nan else d["x"], W=d["W"], b=d["b"] if bias else None)
    z, r = linear_fwd_ref(a["x"], a["W"], a["b"])
    return a, dict(z=z, relu=r if want_relu else None)


def rule_fwd_case(shape, inst, mode):
    (M, N, K), (rule, signed, negden), (bias, want_relu, nan) = shape, inst, mode
    d = fwd_inputs(M, N, K, signed)
    rp = (d["rp"] if bias else d["rp0"])[rule]
    a = dict(x=d["xnan"] if nan else d["x"], W=d["W"], Wp=rp["Wp"], Wn=rp["Wn"] if (signed or negden) else None,
             b=d["b"] if bias else None, bp=rp["bp"], bn=rp["bn"] if negden else None, signed=signed)
    z, r, dp, dn = rule_fwd_ref(a["x"], a["W"], a["Wp"], a["Wn"], a["b"], a["bp"], a["bn"], signed, negden)
    return a, dict(z=z, relu=r if want_relu else None, den_p=dp, den_n=dn)


def _source(d, src):
    return dict(R=d["R"] if src == "R" else None, cls=None if src == "R" else d["cls"], one_hot=int(src == "onehot"))


def lin_bwd_case(shape, mode):
    (M, Nout, Kin), (src, relu_mask, rule_eps, xmode, post) = shape, mode
    d = bwd_inputs(M, Nout, Kin, 1)
    a = dict(_source(d, src), z=d["z"], relu_mask=relu_mask, rule_eps=rule_eps, eps=EPS, W=d["W"],
             x=d["x"] if (xmode != XM_NONE or post != POST_NONE) else None, xmode=xmode,
             den=d["den"] if post == POST_DIV else None, post=post, eps_post=EPS_POST)
    out = linear_bwd_ref(a["R"], a["cls"], a["one_hot"], a["z"], relu_mask, rule_eps, EPS, a["W"], a["x"], xmode, a["den"],
                         post, EPS_POST)
    return a, dict(out=out)


def rule_bwd_case(shape, inst, mode, index=0):
    """``index`` (the shape's position in the list) decides whether the WSquare / Flat constants carry a bias."""
    (M, Nout, Kin), (rule, signed, negden), (src, relu_mask, post) = shape, inst, mode
    d = bwd_inputs(M, Nout, Kin, signed)
    rp = (d["rp"] if index % 2 == 0 else d["rp0"])[rule]
    split = rule in ("gamma", "zplus")
    a = dict(_source(d, src), z=d["z"], relu_mask=relu_mask, eps=rp["eps"], signed=signed,
             den=d["den"] if post == POST_DIV else None, post=post, eps_post=EPS_POST)
    if split:
        a.update(den_p=d["den_p"], den_n=d["den_n"] if negden else None, den_bcast=0, zsign=int(rule == "gamma"),
                 Wp=rp["Wp"], Wn=rp["Wn"] if (signed or negden) else None, x=d["x"], xmul=1)
    else:
        a.update(den_p=rp["den"], den_n=None, den_bcast=1, zsign=0, Wp=rp["W2"], Wn=None,
                 x=d["x"] if post != POST_NONE else None, xmul=0)
    out = rule_bwd_ref(a["R"], a["cls"], a["one_hot"], a["z"], relu_mask, a["den_p"], a["den_n"], a["den_bcast"], a["zsign"],
                       a["eps"], a["Wp"], a["Wn"], a["x"], a["xmul"], signed, a["den"], post, EPS_POST)
    return a, dict(out=out)


def entries():
    """(id, entry point, instantiation or None, shapes, modes, case builder): what test_linear_gpu.py is parametrised by."""
    out = [("linear_fwd", "linear_fwd", None, fwd_shapes(), LIN_FWD_MODES, lambda s, m, i: lin_fwd_case(s, m)),
           ("linear_bwd", "linear_bwd", None, bwd_shapes(), LIN_BWD_MODES, lambda s, m, i: lin_bwd_case(s, m))]
    for inst in RULE_FWD_INSTS:
        out.append(("linear_rule_fwd-%s-signed%d-negden%d" % inst, "linear_rule_fwd", inst, fwd_shapes(), RULE_FWD_MODES,
                    functools.partial(lambda s, m, i, inst: rule_fwd_case(s, inst, m), inst=inst)))
    for inst in RULE_BWD_INSTS:
        out.append(("linear_rule_bwd-%s-signed%d-negden%d" % inst, "linear_rule_bwd", inst, bwd_shapes(), RULE_BWD_MODES,
                    functools.partial(lambda s, m, i, inst: rule_bwd_case(s, inst, m, i), inst=inst)))
    return out
