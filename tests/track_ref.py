"""CPU reference of the track stitch (drsa_amd_track_stitch, csrc/track_stitch.hip).  TEST
INFRASTRUCTURE ONLY (a helper module: pytest does not collect it).  No GPU, no kernel knowledge:
the definition of include/drsa_amd.h restated loop for loop.

``stitch``      the exact float32 result: for every output column the cover set is walked in
                ascending chunk order; ``num`` is the oracle's pinned fp32 fma chain from +0
                (lrp_ref.ExactOps.linear, as tests/linear_ref.py uses it: one k-ascending chain per
                output, here k = the position in the cover set), ``den`` a plain float32 running sum
                in the same order, and out = num / den one IEEE float32 division.
``stitch_f64``  the same sums in float64.
``act`` is not restated in float32: its summation order is the kernel's choice; the tests bound it
against the float64 row sum of the kernel's own ``out``.
"""
import numpy as np
import torch

import lrp_ref


def cover(u, W, h, n):
    """The chunks that cover track column u, ascending: max(0, ceil((u - W + 1) / h)) .. min(n - 1, u // h)."""
    return list(range(max(0, -(-(u - W + 1) // h)), min(n - 1, u // h) + 1))


def hann_taper(W):
    t = (np.arange(W, dtype=np.float64) + 0.5) / W
    return (np.sin(np.pi * t) ** 2).astype(np.float32)


def _sources(std, sub, order):
    """x[k][c] = the [H, W] map of output map k in chunk c (views, nothing copied)."""
    n, K = sub.shape[:2]
    maps = []
    if std is not None:
        maps.append([std[c, 0] for c in range(n)])
    for v in range(K):
        row = []
        for c in range(n):
            if order is None:
                j = v
            else:
                (hits,) = np.nonzero(np.asarray(order[c]) == v)
                assert hits.size == 1, f"order[{c}] is not a permutation"
                j = int(hits[0])
            row.append(sub[c, j])
        maps.append(row)
    return maps


def stitch(std, sub, order, taper, h):
    """std [n, 1, H, W] or None, sub [n, K, H, W], order [n, K] or None, taper [W] (float32 arrays)
    -> out [C, H, Wt] float32, bit for bit what the entry point defines."""
    sub, taper = np.asarray(sub, dtype=np.float32), np.asarray(taper, dtype=np.float32)
    std = None if std is None else np.asarray(std, dtype=np.float32)
    n, K, H, W = sub.shape
    Wt = (n - 1) * h + W
    src = _sources(std, sub, order)
    C = len(src)
    out = np.empty((C, H, Wt), dtype=np.float32)
    for u in range(Wt):
        cs = cover(u, W, h, n)
        assert cs, u
        w = np.array([taper[u - c * h] for c in cs], dtype=np.float32)
        den = np.float32(0.0)
        for wi in w:
            den = np.float32(den + wi)
        # rows of the chain's left operand: one per (map, row), its entries the cover set's values in order
        x = np.stack([np.stack([src[k][c][:, u - c * h] for c in cs], axis=-1) for k in range(C)]).reshape(C * H, len(cs))
        num = lrp_ref.ExactOps.linear(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(w[None].copy()), None)
        out[:, :, u] = (num.numpy().reshape(C, H) / den).astype(np.float32)
    return out


def stitch_f64(std, sub, order, taper, h):
    """The same in float64 (the float32 taper and maps widened) -> (out [C, H, Wt], mag [C, H, Wt]):
    ``mag`` = sum |taper x| / den, what the float32 chain's rounding error is measured against."""
    sub, taper = np.asarray(sub, dtype=np.float64), np.asarray(taper, dtype=np.float64)
    std = None if std is None else np.asarray(std, dtype=np.float64)
    n, K, H, W = sub.shape
    Wt = (n - 1) * h + W
    src = _sources(std, sub, order)
    C = len(src)
    out, mag = np.zeros((C, H, Wt)), np.zeros((C, H, Wt))
    for u in range(Wt):
        cs = cover(u, W, h, n)
        den = sum(taper[u - c * h] for c in cs)
        for k in range(C):
            for c in cs:
                t = u - c * h
                out[k, :, u] += taper[t] * src[k][c][:, t]
                mag[k, :, u] += np.abs(taper[t] * src[k][c][:, t])
        out[:, :, u] /= den
        mag[:, :, u] /= den
    return out, mag


def chain_bound(n_cover):
    """Relative bound (against ``mag``) of the float32 result: a chain of m fmas from +0 commits m - 1
    roundings after the first exact-from-zero step -- m roundings at most --, the float32 sum of the
    weights m - 1, the division one: (2 m) 2^-24 to first order, doubled for the higher-order terms."""
    return 4 * n_cover * 2.0 ** -24
