"""Float64 oracle for the projection layers (csrc/projection.hip).  TEST INFRASTRUCTURE ONLY (a helper
module: pytest does not collect it).  Written from the formulas in the header comments of
projection.hip (reference modify_model.py:75-123, attribute.py:42-60, explainer.py:198-203) in plain
torch float64 on whatever device the inputs live on: no MFMA order, no tiling, no padding.

    residual(U)          P = U U^T - I from the float32 U
    forward(a, U, pool)  h = a U, a' = a + a P, the 2 x 2 max pool of a' and its argmax
    max_pool(ap)         the pool alone (argmax code 2 * row + col, the lowest code wins a tie)
    backward(...)        every output row of G for fanout 0, 1 and 2, and its error bound
    h_bound / ap_bound   the error bounds of the two forward GEMMs
    residual_bound       the error bound of P, residual_chain_model the kernel's arithmetic restated
    tie_map              a map with planted pool ties, shared by the CPU and the GPU test

Layouts are the kernels': a, h, a', den, G are [rows, d, H, W] (h channel-major like a), U is [d, d]
with h[j] = sum_c a[c] U[c][j], the pooled map and its argmax are [B, d, H/2, W/2].

The backward, per sample and pixel (vectors over the d channels):

    R   = unpool(gp, argmax)                     (or the dense relevance when no pool follows)
    g1  = R / stab(a', eps_proj)
    t   = U^T g1
    g2  = h (.) t / stab(h, eps_proj)
    v_q = U_q g2_q          U_q = columns J_q of U: clone 0 all of them, clone q >= 1 the block
                            [(q-1) d/K, q d/K)   (SubspaceHook mask)
    G_q = [a > 0] a (.) v_q / stab(den, eps_den)                          (den = None: no division)
    stab(t, e) = t + (t >= 0 ? e : -e)

with output rows  fanout 1: b (K+1) + q, q = 0..K;  fanout 2: b K + (q-1), q = 1..K;  fanout 0: row
b is clone b % (K+1) of sample b (the replicated batch of the reference).

`backward` takes a' and h as inputs: the GPU tests feed it the kernel's own stored a' and h, so the
check does not depend on how close a' is to 0 (at a dead channel the fp32 and the float64 a' differ
by rounding noise of the size of eps_proj, and the quotients R / stab(a') legitimately part).

Error bounds.  The project's kernel gate allows a GEMM output 2e-5 of the sum of the
absolute values of its terms; an elementwise fp32 chain of three roundings (a product, a stab, a
quotient: 3 * 2^-24 to first order) is allowed 2^-22 of its result.  stab never cancels (t and its
eps have one sign), so its rounding is a relative one.  Carried through the chain with absolute
values, all in float64, E_x bounding |x_kernel - x_64|:

    g1:  three roundings of the inputs' quotient, 2^-23 |g1|: far inside the gate of the GEMM that
         consumes it (2e-5 > 2^-16), and not carried separately
    t:   E_t  = 2e-5 |U|^T |g1|                                   (gate of the first GEMM)
    g2:  the kernel's t enters as t64 + dt, |dt| <= E_t, scaled by h / stab(h); then the three
         roundings of h * t, stab(h), the quotient:
         E_g2 = |h / stab(h)| E_t + 2^-22 |g2|
    v:   the GEMM's inputs are off by E_g2 (carried through |U_q|) and the GEMM itself by its gate:
         E_v  = |U_q| E_g2 + 2e-5 |U_q| |g2_q|
    G:   v enters scaled by a / stab(den); then the roundings of a * v, stab(den), the quotient:
         E_G  = |a| E_v / |stab(den)| + 2^-22 |G|
         (without den: no stab and no quotient, the same formula with stab(den) = 1 holds a fortiori)

For the single-GEMM outputs the bound is the gate itself: |h - h64| <= 2e-5 |a| |U|, and for
a' = a + a P:  |a' - a'64| <= 2e-5 |a| |P64| + 2^-23 |a'64|  (the gate of the residual GEMM, which also
covers the rounding of P to fp32, and the rounding of the final sum).
"""
from __future__ import annotations

import numpy as np
import torch

GATE = 2e-5                 # the project's kernel gate: of the sum of |terms| per GEMM
R3 = 2.0 ** -22             # an elementwise fp32 chain of three roundings
F64 = torch.float64


def _f64(t):
    return None if t is None else t.to(F64)


def stab(t: torch.Tensor, e: float) -> torch.Tensor:
    return t + torch.where(t >= 0, e, -e)


def _eps32(e: float) -> float:
    """The stabiliser as the kernels receive it: a float32 argument."""
    return float(np.float32(e))


def residual(U: torch.Tensor) -> torch.Tensor:
    """U U^T - I in float64 from the float32 U.  The products of two float32 values are exact in
    float64; they are added to -I with Neumaier's compensated summation, so every entry is the exact
    value to a float64 rounding whatever its size (the entries are differences of O(1) sums that
    nearly cancel: a plain float64 matmul leaves them an absolute error of d * 2^-53)."""
    U64 = _f64(U)
    d = U64.shape[0]
    s = -torch.eye(d, dtype=F64, device=U64.device)
    c = torch.zeros_like(s)
    for k in range(d):
        x = torch.outer(U64[:, k], U64[:, k])
        t = s + x
        c += torch.where(s.abs() >= x.abs(), (s - t) + x, (x - t) + s)
        s = t
    return s + c


def residual_bound(U: torch.Tensor, P64: torch.Tensor) -> torch.Tensor:
    """|P_kernel - P64| <= 2^-23 |P64| + 2^-60 + d 2^-53 |U| |U|^T.

    The first two terms allow one fp32 rounding of a float64 value summed in another order.  The
    third is the kernel's own float64 chain (projection_residual_kernel: d fmas, each rounding the
    running sum, which no partial sum of |terms| exceeds: d * 2^-53 * sum_k |U_rk U_ck| to first
    order; the subtraction of the identity is exact, Sterbenz).  It is an absolute error, and the
    entries of P are the rounding noise of an orthonormal U (1e-8 and below, some of them 1e-12),
    so 2^-23 |P64| does not cover it: with the first two terms alone the kernel's arithmetic
    restated in numpy (residual_chain_model) misses at d >= 16 by a factor of up to 200."""
    Ua = _f64(U).abs()
    return 2.0 ** -23 * P64.abs() + 2.0 ** -60 + U.shape[0] * 2.0 ** -53 * (Ua @ Ua.T)


def residual_chain_model(U: torch.Tensor) -> torch.Tensor:
    """projection_residual_kernel restated: a float64 fma chain over k ascending (the product of two
    float32 values is exact in float64, so the fma is a product and an add), minus I, rounded to
    float32."""
    U64 = _f64(U)
    d = U64.shape[0]
    acc = torch.zeros(d, d, dtype=F64, device=U64.device)
    for k in range(d):
        acc = acc + torch.outer(U64[:, k], U64[:, k])
    return (acc - torch.eye(d, dtype=F64, device=U64.device)).to(torch.float32)


def max_pool(ap: torch.Tensor):
    """2 x 2 max pool of [B, d, H, W] -> (pooled, argmax uint8), argmax = 2 * row + col of the first
    maximum in code order (a NaN counts as the maximum, the first NaN wins)."""
    B, d, H, W = ap.shape
    win = torch.stack([ap[:, :, r::2, c::2] for r in (0, 1) for c in (0, 1)], dim=-1)   # code order
    nan = torch.isnan(win)
    best = torch.where(nan, torch.full_like(win, float("-inf")), win).max(dim=-1, keepdim=True).values
    hit = torch.where(nan.any(dim=-1, keepdim=True), nan, win == best)
    code = torch.argmax(hit.to(torch.uint8), dim=-1)                                    # first hit
    pooled = torch.gather(win, -1, code.unsqueeze(-1)).squeeze(-1)
    return pooled, code.to(torch.uint8)


def forward(a: torch.Tensor, U: torch.Tensor, pool: bool = True):
    """(h, a', pooled a', argmax) in float64; the last two are None without pool."""
    a64, U64 = _f64(a), _f64(U)
    h = torch.einsum("cj,bchw->bjhw", U64, a64)
    ap = a64 + torch.einsum("ck,bkhw->bchw", residual(U), a64)
    pooled, amax = max_pool(ap) if pool else (None, None)
    return h, ap, pooled, amax


def h_bound(a: torch.Tensor, U: torch.Tensor) -> torch.Tensor:
    return GATE * torch.einsum("cj,bchw->bjhw", _f64(U).abs(), _f64(a).abs())


def ap_bound(a: torch.Tensor, P64: torch.Tensor, ap64: torch.Tensor) -> torch.Tensor:
    return GATE * torch.einsum("ck,bkhw->bchw", P64.abs(), _f64(a).abs()) + 2.0 ** -23 * ap64.abs()


def unpool(gp: torch.Tensor, amax: torch.Tensor) -> torch.Tensor:
    """Pool backward: each pooled relevance at its window's argmax position, zeros elsewhere."""
    B, d, H2, W2 = gp.shape
    R = torch.zeros(B, d, 2 * H2, 2 * W2, dtype=gp.dtype, device=gp.device)
    for code in range(4):
        R[:, :, code // 2::2, code % 2::2] = torch.where(amax == code, gp, torch.zeros_like(gp))
    return R


def clone_columns(q: int, d: int, K: int):
    """[j0, j1): the columns of U that relevance clone q keeps (attribute.py:53-60)."""
    dk = d // K
    return (0, d) if q == 0 else ((q - 1) * dk, q * dk)


def output_clones(B: int, K: int, fanout: int):
    """[(sample, clone)] of every output row, in row order."""
    if fanout == 1:
        return [(b, q) for b in range(B) for q in range(K + 1)]
    if fanout == 2:
        return [(b, q) for b in range(B) for q in range(1, K + 1)]
    if fanout == 0:
        return [(b, b % (K + 1)) for b in range(B)]
    raise ValueError(f"fanout {fanout}")


def backward(gp, amax, ap, h, a, den, U, K: int, eps_proj: float, eps_den: float, fanout: int):
    """(G, E_G): every output row [rows, d, H, W] in float64 and its error bound (module docstring).
    gp is the pooled relevance with amax, the dense one with amax = None; den may be None."""
    gp, ap, h, a, den, U = (_f64(t) for t in (gp, ap, h, a, den, U))
    B, d = a.shape[:2]
    ep, ed = _eps32(eps_proj), _eps32(eps_den)
    R = gp if amax is None else unpool(gp, amax)
    Ua = U.abs()
    g1 = R / stab(ap, ep)
    t = torch.einsum("cj,bchw->bjhw", U, g1)
    E_t = GATE * torch.einsum("cj,bchw->bjhw", Ua, g1.abs())
    hs = h / stab(h, ep)
    g2 = hs * t
    E_g2 = hs.abs() * E_t + R3 * g2.abs()
    sden = stab(den, ed) if den is not None else torch.ones_like(a)
    live = a > 0
    G, E = [], []
    for b, q in output_clones(B, K, fanout):
        j0, j1 = clone_columns(q, d, K)
        Uq, Uqa = U[:, j0:j1], Ua[:, j0:j1]
        v = torch.einsum("cj,jhw->chw", Uq, g2[b, j0:j1])
        E_v = torch.einsum("cj,jhw->chw", Uqa, E_g2[b, j0:j1]) + GATE * torch.einsum("cj,jhw->chw", Uqa, g2[b, j0:j1].abs())
        Gq = torch.where(live[b], a[b] * v / sden[b], torch.zeros_like(v))
        G.append(Gq)
        E.append(torch.where(live[b], a[b].abs() * E_v / sden[b].abs(), torch.zeros_like(v)) + R3 * Gq.abs())
    return torch.stack(G), torch.stack(E)


def tie_map():
    """[1, 16, 8, 8]: windows with the maximum duplicated at every pair of positions, all-zero windows,
    and distinct windows; returns (map, expected argmax code per window or -1 where not planted)."""
    g = torch.Generator().manual_seed(5)
    a = torch.rand(1, 16, 8, 8, generator=g) + 0.25
    want = torch.full((1, 16, 4, 4), -1, dtype=torch.long)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    for c, (i, j) in enumerate(pairs):                      # channels 0-5: one pair each, in every window
        for code in (i, j):
            a[0, c, code // 2::2, code % 2::2] = 2.0
        want[0, c] = i
    a[0, 6] = 0.0                                           # all-zero windows (a dead post-ReLU channel)
    want[0, 6] = 0
    a[0, 7] = 3.0                                           # four equal values
    want[0, 7] = 0
    a[0, 8, 0:2, 0:2] = 0.0                                 # one zero window among live ones
    want[0, 8, 0, 0] = 0
    return a, want


def worst_ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err / bound, with 0 / 0 = 0 and x / 0 = inf."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0
