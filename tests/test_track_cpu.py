"""Whole-track explanations: what holds without a GPU.  The chunk grid's known answers and refusals,
the cover sets, the taper, the reference restatement (tests/track_ref.py) against its own float64
version, and the argument checks of drsa_amd_track_stitch (all rejected before any device work).

Bound of the restatement (track_ref.chain_bound): the float32 result differs from the float64 one
by at most 4 m 2^-24 x sum |taper x| / den for a cover set of m chunks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import track_ref as TR
from drsa_audio_amd import _capi
from drsa_audio_amd.xai.explain import track as T


# ------------------------------------------------------------------- the grid
L, HOP, W, H = 16000, 240, 64, 32                                        # the toy geometry, hop_frames = 32
HOPS = H * HOP                                                           # 7680 samples


@pytest.mark.parametrize("Tn,want", [
    (1, (1, L, 64, 0)),                                                  # shorter than one hop: no column is real
    (10000, (1, L, 64, 41)),                                             # one chunk, Wr = 10000 // 240 = 41 < Wt
    (L - 1, (1, L, 64, 64)),                                             # T <= L: one chunk; 15999 // 240 = 66 > Wt
    (L, (1, L, 64, 64)),
    (L + 1, (2, L + HOPS, 96, 66)),                                      # one sample more: a second, padded chunk
    (L + 3 * HOPS, (4, L + 3 * HOPS, 160, 160)),                         # T = L + k hopS exactly: no padding
    (L + 2 * HOPS + 1000, (4, L + 3 * HOPS, 160, 134)),                  # padded; Wr = 32360 // 240 = 134 < Wt = 160
    (L + 2 * HOPS + 7000, (4, L + 3 * HOPS, 160, 159)),
])
def test_track_grid_known_answers(Tn, want):
    assert T.track_grid(Tn, L, HOP, W, H) == want
    n, T_pad, Wt, Wr = want
    assert T_pad >= Tn and T_pad - Tn < HOPS or n == 1
    assert Wt == (n - 1) * H + W and Wr == min(Wt, Tn // HOP)


def test_track_grid_default_hop_is_half_the_width():
    assert T.track_grid(100000, L, HOP, W) == T.track_grid(100000, L, HOP, W, W // 2)
    # GTZAN: 30 s at hop_frames 64 -> 20 chunks of 3 s, 1344 columns, 1333 of them inside the track
    assert T.track_grid(480000, 48000, 360, 128) == (20, 48000 + 19 * 64 * 360, 1344, 1333)


@pytest.mark.parametrize("kw,needle", [
    (dict(hop_frames=0), "at least 1"),
    (dict(hop_frames=W + 1), "gaps"),
    (dict(T=0), "no samples"),
    (dict(L=W * HOP - 1), "shorter"),
])
def test_track_grid_refusals(kw, needle):
    args = dict(T=50000, L=L, hop_length=HOP, W=W, hop_frames=H)
    args.update(kw)
    with pytest.raises(ValueError, match=needle):
        T.track_grid(**args)
    assert T.track_grid(50000, W * HOP, HOP, W, W)[0] >= 1                # the smallest L and the largest step pass


@pytest.mark.parametrize("Wd,n", [(64, 1), (64, 5), (5, 3), (128, 2)])
def test_every_column_is_covered(Wd, n):
    for h in sorted({1, max(1, Wd // 2), max(1, Wd - 1), Wd}):
        Wt = (n - 1) * h + Wd
        counts = []
        for u in range(Wt):
            cs = list(T.cover(u, Wd, h, n))
            assert cs == TR.cover(u, Wd, h, n) and cs, (h, u)
            assert all(0 <= c < n and 0 <= u - c * h < Wd for c in cs)
            # and nobody else covers u
            assert cs == [c for c in range(n) if 0 <= u - c * h < Wd]
            counts.append(len(cs))
        assert max(counts) == min(n, math.ceil(Wd / h)) and min(counts) == 1


# ------------------------------------------------------------------ the taper
@pytest.mark.parametrize("Wd", [5, 64, 128])
def test_taper_is_positive_and_symmetric(Wd):
    hann, flat = T.make_taper(Wd, "hann"), T.make_taper(Wd, "flat")
    assert hann.dtype == flat.dtype == torch.float32 and hann.shape == flat.shape == (Wd,)
    assert float(hann.min()) > 0 and float(hann.max()) <= 1
    assert torch.equal(hann, hann.flip(0))
    assert torch.equal(flat, torch.ones(Wd))
    t = (np.arange(Wd) + 0.5) / Wd
    assert np.abs(TR.hann_taper(Wd) - np.sin(np.pi * t) ** 2).max() <= 2.0 ** -24
    assert np.abs(hann.numpy() - np.sin(np.pi * t) ** 2).max() <= 2.0 ** -24
    with pytest.raises(ValueError, match="taper"):
        T.make_taper(Wd, "triangle")


# ------------------------------------------------------------ the restatement
def _case(n, K, Hh, Wd, seed, with_std=True, with_order=True):
    rng = np.random.default_rng(seed)
    sub = rng.standard_normal((n, K, Hh, Wd)).astype(np.float32)
    std = rng.standard_normal((n, 1, Hh, Wd)).astype(np.float32) if with_std else None
    order = np.stack([rng.permutation(K) for _ in range(n)]).astype(np.int64) if with_order else None
    return std, sub, order


@pytest.mark.parametrize("Wd,h,n,K", [(5, 1, 5, 2), (16, 7, 3, 3), (16, 8, 4, 1), (16, 16, 2, 2), (16, 15, 1, 2)])
@pytest.mark.parametrize("kind", ["hann", "flat"])
def test_reference_against_its_float64_version(Wd, h, n, K, kind):
    std, sub, order = _case(n, K, 3, Wd, seed=Wd + h + n)
    taper = T.make_taper(Wd, kind).numpy()
    out = TR.stitch(std, sub, order, taper, h)
    ref, mag = TR.stitch_f64(std, sub, order, taper, h)
    assert out.dtype == np.float32 and out.shape == ref.shape == (K + 1, 3, (n - 1) * h + Wd)
    m = min(n, math.ceil(Wd / h))
    assert (np.abs(out - ref) <= TR.chain_bound(m) * mag).all()
    assert np.abs(out - ref).max() > 0 or kind == "flat"                  # float32 does round
    # the un-sort: map k of the output is concept k - 1 wherever a chunk keeps it
    ident = TR.stitch(std, np.stack([sub[c][np.argsort(order[c])] for c in range(n)]), None, taper, h)
    assert np.array_equal(out, ident)
    # without std the K concept maps are the same, one index lower
    assert np.array_equal(TR.stitch(None, sub, order, taper, h), out[1:])


def test_reference_single_chunk_and_constant_maps():
    """One chunk: out = fl(fl(w x) / w), within 3 x 2^-24 |x| of x (exactly x under the flat taper).
    Constant maps: with the constant 1 the num chain is, step for step, the den sum, so out = 1
    exactly under any taper; scaling by a power of two is exact, so -4 and 2^-3 come back exactly too
    (another constant c is only within the chain bound: w c rounds)."""
    std, sub, order = _case(1, 3, 2, 16, seed=1, with_order=False)
    for kind in ("hann", "flat"):
        taper = T.make_taper(16, kind).numpy()
        out = TR.stitch(std, sub, order, taper, 8)
        full = np.concatenate([std[0], sub[0]])
        assert (np.abs(out - full) <= 3 * 2.0 ** -24 * np.abs(full)).all()
        if kind == "flat":
            assert np.array_equal(out, full)
        for h in (1, 5, 8, 16):
            const = np.stack([np.full((4, 2, 16), v, dtype=np.float32) for v in (1.0, -4.0, 0.125)], axis=1)
            got = TR.stitch(None, const, None, taper, h)
            for k, v in enumerate((1.0, -4.0, 0.125)):
                assert (got[k] == np.float32(v)).all(), (kind, h, v)


# ------------------------------------------------------- argument rejections
_BUF = (ctypes.c_double * 64)()                                          # 8-byte aligned host memory
_P = ctypes.cast(_BUF, ctypes.c_void_p)
_VALID = dict(std_maps=_P, sub=_P, order=None, taper=_P, n=2, K=4, H=64, W=64, h=32, out=_P, act=_P, ws=_P,
              ws_bytes=1 << 20, stream=None)
_EINVAL = _capi.DRSA_EINVAL


def _order(rows):
    a = (ctypes.c_int64 * (len(rows) * len(rows[0])))(*[v for r in rows for v in r])
    return a


_BAD_ORDERS = [[[0, 1, 2, 3], [0, 1, 1, 3]], [[0, 1, 2, 4], [0, 1, 2, 3]], [[3, 2, 1, 0], [-1, 0, 1, 2]]]
_REJECTIONS = [
    (dict(sub=None), _EINVAL, "null"),
    (dict(taper=None), _EINVAL, "null"),
    (dict(out=None), _EINVAL, "null"),
    (dict(act=None), _EINVAL, "null"),
    (dict(n=0), _EINVAL, "n >= 1"),
    (dict(K=0), _EINVAL, "K >= 1"),
    (dict(H=0), _EINVAL, "H >= 1"),
    (dict(h=0), _EINVAL, "1 <= h <= W"),
    (dict(h=65), _EINVAL, "1 <= h <= W"),
    (dict(W=0, h=0), _EINVAL, "1 <= h <= W"),
    (dict(n=1 << 30, h=64), _EINVAL, "too large"),
    (dict(K=65535), _EINVAL, "too large"),
    (dict(ws_bytes=0), _capi.DRSA_EWORKSPACE, "workspace"),
    (dict(ws=None), _capi.DRSA_EWORKSPACE, "workspace"),
] + [(dict(order=_order(o)), _EINVAL, "permutation") for o in _BAD_ORDERS] + [
    # a valid order in pageable host memory passes the permutation check and is refused as unreadable
    (dict(order=_order([[3, 1, 0, 2], [0, 1, 2, 3]])), _EINVAL, "pageable"),
]


@pytest.mark.parametrize("changes,code,needle", _REJECTIONS)
def test_track_stitch_rejects_bad_arguments(changes, code, needle):
    lib = _capi.load()
    args = dict(_VALID, **changes)
    rc = lib.drsa_amd_track_stitch(*args.values())
    msg = lib.drsa_amd_last_error().decode()
    assert rc == code, (rc, msg)
    assert "track_stitch" in msg and needle in msg, msg


def test_workspace_size():
    lib = _capi.load()
    f = lib.drsa_amd_track_stitch_workspace_bytes
    assert f(5, 32, 160) == 0 and f(5, 1, 160) == 0                       # one block of 32 rows: act is written directly
    assert f(5, 33, 160) == 5 * 2 * 160 * 4
    assert f(5, 401, 1344) == 5 * 13 * 1344 * 4
    assert f(0, 64, 160) == 0 and f(5, 0, 160) == 0 and f(5, 64, 0) == 0


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    sub = torch.zeros(2, 4, 8, 16)
    with pytest.raises(_capi.DrsaAmdError, match="GPU"):
        T.track_stitch(None, sub, None, T.make_taper(16), 8)
