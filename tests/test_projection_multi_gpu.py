"""drsa_amd_projection_fwd_multi / drsa_amd_projection_bwd_multi (a projection matrix per row) against the
single-matrix entries, bit for bit: row b of every output must be what the single-matrix entry gives for that row
with U_tab[u_row[b]].

The reference of a row is a single-matrix call on that row alone (B = 1).  With fanout 0 the row index selects the
clone (b mod (K + 1)), which a one-row call would lose, so there the reference is one single-matrix call over the
whole batch per matrix of the table, of which the rows that name the matrix are taken.  Every output is a view
between sentinel bands, prefilled with a marked NaN (test_conv_edges_gpu.Guard).

The cases rotate the modes over every kernel instantiation (d = 16, 24 -> 32, 32, 64, 100 -> 128, 128), d_k = 4, 8,
16, 25, the tile shapes 8 x 8, 4 x 16, 2 x 32 and 16 x 32 (8 tiles: more than one workgroup per sample in every
kernel), pool / no pool, den / no den and fanout 0, 1, 2; each runs h and a' stored and recomputed.  The three
matrices of a table must give different outputs on the same row, so a kernel that ignored the index fails."""
import functools

import numpy as np
import pytest
import torch

from drsa_audio_amd import _capi
from test_conv_edges_gpu import Guard

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EPS_PROJ, EPS_DEN = 1e-6, 1e-7

MIXED = "mixed"             # B = 5, u_row = [2, 0, 2, 1, 0] over three matrices: unsorted and repeated
REPLICATED = "replicated"   # B = 2 (K + 1), the index constant within a sample's K + 1 rows (fanout 0)
SINGLE = "single"           # n_u = 1, all-zero indices: one single-matrix call over the batch

#        d    K   H   W  pool den   fanout pattern
CASES = [(16, 4, 8, 8, 1, True, 1, MIXED),
         (24, 3, 4, 16, 0, False, 2, MIXED),
         (32, 4, 2, 32, 1, True, 0, REPLICATED),
         (32, 2, 16, 32, 1, False, 1, MIXED),
         (64, 4, 16, 32, 1, True, 2, MIXED),
         (64, 4, 8, 8, 0, False, 1, SINGLE),
         (64, 4, 4, 16, 0, True, 0, MIXED),
         (100, 4, 4, 16, 1, False, 1, MIXED),
         (100, 4, 16, 32, 0, True, 0, REPLICATED),
         (128, 8, 2, 32, 0, True, 2, MIXED),
         (128, 32, 8, 8, 1, False, 1, MIXED)]


def _ortho(d, seed):
    return torch.from_numpy(np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0].astype(np.float32))


def _rows(pattern, K):
    if pattern == MIXED:
        return [2, 0, 2, 1, 0], 3
    if pattern == REPLICATED:
        return [2] * (K + 1) + [0] * (K + 1), 3
    return [0, 0, 0], 1


def _fwd(multi, c, a, sel, B, h, ap, pooled, amax):
    """One forward call: the multi entry with the table and ``sel`` = the index tensor, or the single-matrix entry
    with ``sel`` = the matrix number."""
    d, H, W, s = c["d"], c["H"], c["W"], _capi.stream_ptr(DEV)
    tail = (_capi.ptr(h), _capi.ptr(ap), _capi.ptr(pooled), _capi.ptr(amax), B, d, H, W, c["pool"], s)
    if multi:
        _capi.call("drsa_amd_projection_fwd_multi", a.data_ptr(), c["U_tab"].data_ptr(), c["P_tab"].data_ptr(),
                   sel.data_ptr(), c["n_u"], *tail)
    else:
        _capi.call("drsa_amd_projection_fwd", a.data_ptr(), c["U_tab"][sel].data_ptr(), c["P_tab"][sel].data_ptr(), *tail)


def _bwd(multi, c, gp, amax, ap, h, a, den, sel, G, B, fanout):
    d, H, W, s = c["d"], c["H"], c["W"], _capi.stream_ptr(DEV)
    head = (gp.data_ptr(), _capi.ptr(amax), _capi.ptr(ap), _capi.ptr(h), a.data_ptr(), _capi.ptr(den))
    tail = (G, B, d, H, W, c["K"], EPS_PROJ, EPS_DEN if den is not None else 0.0, fanout, s)
    if multi:
        _capi.call("drsa_amd_projection_bwd_multi", *head, c["U_tab"].data_ptr(), c["P_tab"].data_ptr(), sel.data_ptr(),
                   c["n_u"], *tail)
    else:
        _capi.call("drsa_amd_projection_bwd", *head, c["U_tab"][sel].data_ptr(), c["P_tab"][sel].data_ptr(), *tail)


@functools.lru_cache(maxsize=None)
def _case(d, K, H, W, pool, pattern):
    """Inputs of one case, built once and never written afterwards."""
    rows, n_u = _rows(pattern, K)
    B = len(rows)
    g = torch.Generator().manual_seed(1000 * d + 10 * H + W)
    a = torch.randn(B, d, H, W, generator=g).clamp_min(0)
    a[:, 1] = 0                                   # a dead ReLU channel
    if pattern == REPLICATED:                     # the reference's replicated batch: K + 1 copies of a sample
        a = a[::K + 1].repeat_interleave(K + 1, 0)
    U_tab = torch.stack([_ortho(d, 7 * d + i) for i in range(n_u)]).to(DEV)
    P_tab = torch.empty_like(U_tab)
    for U, P in zip(U_tab, P_tab):
        _capi.call("drsa_amd_projection_residual", U.data_ptr(), d, P.data_ptr(), _capi.stream_ptr(DEV))
    gshape = (B, d, H // 2, W // 2) if pool else (B, d, H, W)
    gp = torch.randn(*gshape, generator=g)
    gp.view(-1)[0::7] = 0.0
    gp.view(-1)[3::7] = -0.0
    den = torch.randn(B, d, H, W, generator=g) * 2
    torch.cuda.synchronize()
    return dict(d=d, K=K, H=H, W=W, pool=pool, B=B, n_u=n_u, rows=rows, a=a.to(DEV).contiguous(), U_tab=U_tab,
                P_tab=P_tab, u_row=torch.tensor(rows, dtype=torch.int32, device=DEV), gp=gp.to(DEV), den=den.to(DEV))


def _eq(got, want, what):
    """Bit for bit, the sign of zero included."""
    assert got.shape == want.shape, what
    assert not torch.isnan(want).any(), f"{what}: NaN in the reference"
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    assert torch.equal(got, want), what


def _forward(c, multi, sel, a, B, store):
    """(h, ap, pooled, amax) on the host (None where the call does not write it), each from its own Guard."""
    d, H, W, pool = c["d"], c["H"], c["W"], c["pool"]
    h = Guard((B, d, H * W)) if store else None
    ap = Guard((B, d, H, W)) if (store or not pool) else None
    pooled = Guard((B, d, H // 2, W // 2)) if pool else None
    amax = Guard((B, d, H // 2, W // 2), torch.uint8) if pool else None
    ptr = lambda gd: None if gd is None else gd.view      # noqa: E731
    _fwd(multi, c, a, sel, B, ptr(h), ptr(ap), ptr(pooled), ptr(amax))
    torch.cuda.synchronize()
    return tuple(None if gd is None else gd.result() for gd in (h, ap, pooled, amax))


def _backward(c, multi, sel, sl, B, fanout, has_den, state):
    """G [B * nq, d, H, W] on the host for the rows ``sl`` of the case (a slice)."""
    d, H, W, K = c["d"], c["H"], c["W"], c["K"]
    nq = K + 1 if fanout == 1 else K if fanout == 2 else 1
    G = Guard((B * nq, d, H, W))
    cut = lambda t: None if t is None else t[sl].contiguous()      # noqa: E731
    _bwd(multi, c, cut(c["gp"]), cut(state["amax"]), cut(state["ap"]), cut(state["h"]), cut(c["a"]),
         cut(c["den"]) if has_den else None, sel, G.ptr(), B, fanout)
    torch.cuda.synchronize()
    return G.result(), nq


@pytest.mark.parametrize("store", [False, True], ids=["recomputed", "stored"])
@pytest.mark.parametrize("d,K,H,W,pool,has_den,fanout,pattern", CASES,
                         ids=[f"d{c[0]}-K{c[1]}-{c[2]}x{c[3]}-pool{c[4]}-den{int(c[5])}-fan{c[6]}-{c[7]}" for c in CASES])
def test_multi_equals_single_matrix_rows(d, K, H, W, pool, has_den, fanout, pattern, store):
    c = _case(d, K, H, W, pool, pattern)
    B, rows, n_u, names = c["B"], c["rows"], c["n_u"], ("h", "ap", "pooled", "amax")
    # ---- forward: the multi entry over the batch
    got = _forward(c, True, c["u_row"], c["a"], B, store)
    # the single-matrix entry over the whole batch, once per matrix: the fanout-0 reference, the n_u = 1 reference,
    # and the proof that the matrices tell apart
    full = [_forward(c, False, m, c["a"], B, store) for m in range(n_u)]
    for b in range(B):
        want = full[0] if pattern == SINGLE else _forward(c, False, rows[b], c["a"][b:b + 1].contiguous(), 1, store)
        for name, g_t, w_t in zip(names, got, want):
            if g_t is not None:
                _eq(g_t[b:b + 1], w_t[b:b + 1] if pattern == SINGLE else w_t, f"forward {name} row {b}")
    for m in range(n_u):
        for m2 in range(m):     # the float outputs of two matrices differ on every row
            for name, x, y in zip(names[:3], full[m], full[m2]):
                if x is not None:
                    assert all(not torch.equal(x[b], y[b]) for b in range(B)), f"matrices {m2}, {m} agree on {name}"
    # ---- backward, on the multi forward's own state (checked equal above)
    state = {n: None if t is None else t.to(DEV) for n, t in zip(names, got)}
    if not store:
        state["h"] = state["ap"] = None           # a' may be the forward's output (no pool) and still be recomputed
    G, nq = _backward(c, True, c["u_row"], slice(0, B), B, fanout, has_den, state)
    full_G = [_backward(c, False, m, slice(0, B), B, fanout, has_den, state)[0] for m in range(n_u)]
    for b in range(B):
        if fanout == 0 or pattern == SINGLE:
            want = full_G[rows[b]][b * nq:(b + 1) * nq]
        else:
            want = _backward(c, False, rows[b], slice(b, b + 1), 1, fanout, has_den, state)[0]
        _eq(G[b * nq:(b + 1) * nq], want, f"backward G row {b}")
    assert (G[:, 1] == 0).all()                   # the dead channel stays dead in every clone
    for m in range(n_u):
        for m2 in range(m):
            assert all(not torch.equal(full_G[m][b * nq:(b + 1) * nq], full_G[m2][b * nq:(b + 1) * nq])
                       for b in range(B)), f"matrices {m2}, {m} agree on G"


def test_cases_cover_the_grid():
    """The rotation above reaches every value the kernels branch on."""
    col = lambda i: {c[i] for c in CASES}      # noqa: E731
    assert col(0) == {16, 24, 32, 64, 100, 128}
    assert {c[0] // c[1] for c in CASES} >= {4, 8, 16, 25}
    assert {(c[2], c[3]) for c in CASES} == {(8, 8), (4, 16), (2, 32), (16, 32)}
    assert col(4) == {0, 1} and col(5) == {True, False} and col(6) == {0, 1, 2} and col(7) == {MIXED, REPLICATED, SINGLE}
