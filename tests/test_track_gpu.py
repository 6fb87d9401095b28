"""Whole-track explanations on the GPU: drsa_amd_track_stitch (csrc/track_stitch.hip) against the
loop-for-loop restatement tests/track_ref.py, and TrackExplainer (xai/explain/track.py) end to end
at the toy geometry.

Tolerances.  ``out`` is compared bit for bit: include/drsa_amd.h fixes every operation and its order.
``act``'s order is the kernel's, so it is held to the bound of any summation order of H terms,
(H - 1) 2^-24 sum_r |out[k][r][u]|, against the float64 row sum of the kernel's own ``out``.  One
chunk: out = fl(fl(w x) / w) is within 3 x 2^-24 |x| of x (two roundings, with the second-order
term).  Constant maps come back exactly for the constants 1, -4 and 2^-3: with 1 the num chain is
the den sum step for step, and a power of two scales both exactly (for another constant c the
product w c rounds, and exactness does not follow from the arithmetic that the header fixes).
The all-ones identity takes the gate of tests/test_stft_audio_gpu.py
test_all_ones_mask_returns_the_chunk: test_audiogen_gpu.audio_check, each audio's relative L2
distance from the float64 target at most 2 x the float32 torch chain's + 1e-7 -- the same synthesis
kernel and the same window envelope, at the track's width.
"""
import functools

import numpy as np
import pytest
import torch

import lrp_common as LC
import stft_audio_ref as S
import test_audiogen_gpu as AG
import track_ref as TR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _stitch(std, sub, order, taper, h):
    from drsa_audio_amd.xai.explain.track import track_stitch
    out, act = track_stitch(_dev(std), _dev(sub), _dev(order), _dev(taper), h)
    return out.cpu().numpy(), act.cpu().numpy()


def _taper(W, kind):
    from drsa_audio_amd.xai.explain.track import make_taper
    return make_taper(W, kind).numpy()


@functools.lru_cache(maxsize=None)
def _inputs(n, K, H, W, with_std, with_order):
    rng = np.random.default_rng(1000 * n + 100 * K + H + W)
    sub = rng.standard_normal((n, K, H, W)).astype(np.float32)
    std = rng.standard_normal((n, 1, H, W)).astype(np.float32) if with_std else None
    order = np.stack([rng.permutation(K) for _ in range(n)]).astype(np.int64) if with_order else None
    for a in (sub, std, order):
        if a is not None:
            a.setflags(write=False)
    return std, sub, order


# ------------------------------------------------------------------ the kernel
# (W, h, n, H, K, order, std, taper): every value of every axis at least once.  The 16-byte kernel
# takes W, h multiples of 4 -- (64, 32), (64, 64), (128, 64): Wt = 192, 320, 64, 96, 384 (three column
# tiles of 128 exactly), 192, 128 --, the 4-byte kernel the others: Wt = 9 and 6 (below one tile of 32),
# 92, 71, 316 (a multiple of 4 but not of 32), 127 and 64 (two tiles exactly).  Cover counts run from 1
# to min(n, ceil(W / h)) = 5, 5, 2, 2, 1, 2; H = 401 takes 13 row blocks (the second act launch), H = 33 two.
CASES = [
    (5, 1, 5, 1, 1, False, False, "flat"),
    (5, 1, 2, 33, 4, True, True, "hann"),
    (64, 7, 5, 33, 4, True, True, "hann"),
    (64, 7, 2, 1, 20, True, False, "flat"),
    (64, 32, 5, 401, 4, True, True, "hann"),
    (64, 32, 1, 33, 1, False, True, "flat"),
    (64, 32, 2, 33, 20, True, False, "hann"),
    (64, 63, 5, 33, 4, False, True, "hann"),
    (64, 63, 2, 1, 1, True, True, "flat"),
    (64, 63, 1, 33, 4, True, True, "hann"),
    (64, 64, 5, 33, 4, True, True, "flat"),
    (64, 64, 1, 401, 1, False, False, "hann"),
    (128, 64, 5, 33, 20, True, True, "hann"),
    (128, 64, 2, 401, 4, False, True, "hann"),
    (128, 64, 1, 1, 4, True, False, "flat"),
]


def test_the_cases_hold_every_axis_value():
    for i, want in enumerate([{(5, 1), (64, 7), (64, 32), (64, 63), (64, 64), (128, 64)}, None, {1, 2, 5}, {1, 33, 401},
                              {1, 4, 20}, {True, False}, {True, False}, {"hann", "flat"}]):
        if i == 0:
            assert {c[:2] for c in CASES} == want
        elif want is not None:
            assert {c[i] for c in CASES} == want, i


@pytest.mark.parametrize("W,h,n,H,K,with_order,with_std,kind", CASES)
def test_stitch_bit_for_bit(W, h, n, H, K, with_order, with_std, kind):
    std, sub, order = _inputs(n, K, H, W, with_std, with_order)
    taper = _taper(W, kind)
    out, act = _stitch(std, sub, order, taper, h)
    ref = TR.stitch(std, sub, order, taper, h)
    C, Wt = K + with_std, (n - 1) * h + W
    assert out.shape == ref.shape == (C, H, Wt) and act.shape == (C, Wt)
    assert np.array_equal(out.view(np.int32), ref.view(np.int32)), np.abs(out - ref).max()
    o64 = out.astype(np.float64)
    err, bound = np.abs(act - o64.sum(1)), (H - 1) * 2.0 ** -24 * np.abs(o64).sum(1)
    print(f"\n  act: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}" if H > 1 else "")
    assert (err <= bound).all()
    # deterministic: a second run gives the same bits
    out2, act2 = _stitch(std, sub, order, taper, h)
    assert np.array_equal(out.view(np.int32), out2.view(np.int32)) and np.array_equal(act.view(np.int32), act2.view(np.int32))


@pytest.mark.parametrize("W,h,n,H,K", [(64, 32, 5, 33, 4), (64, 7, 5, 33, 4), (128, 64, 2, 401, 4)])
def test_sorted_maps_with_order_equal_unsorted_maps_without(W, h, n, H, K):
    std, sub, order = _inputs(n, K, H, W, True, True)
    taper = _taper(W, "hann")
    shuffled = np.stack([sub[c][order[c]] for c in range(n)])           # slot j of chunk c holds concept order[c][j]
    a = _stitch(std, shuffled, order, taper, h)
    b = _stitch(std, sub, None, taper, h)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.mark.parametrize("W,h,n,H,K", [(64, 32, 5, 33, 4), (128, 64, 2, 401, 4)])
def test_unaligned_pointers_take_the_narrow_kernel_with_the_same_bits(W, h, n, H, K):
    """sub one float off a 16-byte boundary: the 4-byte kernel runs; out and act do not change."""
    from drsa_audio_amd.xai.explain.track import track_stitch
    std, sub, order = _inputs(n, K, H, W, True, True)
    taper = _dev(_taper(W, "hann"))
    buf = torch.empty(sub.size + 1, device=DEV)
    off = buf[1:].view(sub.shape)
    off.copy_(_dev(sub))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    a = track_stitch(_dev(std), off, _dev(order), taper, h)
    b = track_stitch(_dev(std), _dev(sub), _dev(order), taper, h)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("kind", ["hann", "flat"])
@pytest.mark.parametrize("W,h,n", [(64, 7, 5), (64, 32, 5), (5, 1, 5)])
def test_constant_maps_come_back_constant(W, h, n, kind):
    vals = (1.0, -4.0, 0.125)
    sub = np.stack([np.full((n, 33, W), v, dtype=np.float32) for v in vals], axis=1)
    out, act = _stitch(None, sub, None, _taper(W, kind), h)
    for k, v in enumerate(vals):
        assert (out[k] == np.float32(v)).all(), (v, np.abs(out[k] - v).max())
        assert (act[k] == np.float32(33 * v)).all()                      # 33 v and every partial sum of it are exact


@pytest.mark.parametrize("kind", ["hann", "flat"])
def test_one_chunk_returns_its_own_maps(kind):
    std, sub, _ = _inputs(1, 4, 33, 64, True, False)
    out, _ = _stitch(std, sub, None, _taper(64, kind), 32)
    full = np.concatenate([std[0], sub[0]])
    assert (np.abs(out - full) <= 3 * 2.0 ** -24 * np.abs(full)).all()
    if kind == "flat":
        assert np.array_equal(out, full)


def test_wrapper_refuses_an_order_that_is_no_permutation():
    from drsa_audio_amd.xai.explain.track import track_stitch
    std, sub, order = _inputs(2, 4, 33, 64, True, True)
    bad = order.copy()
    bad[1, 0] = bad[1, 1]
    with pytest.raises(ValueError, match="permutation"):
        track_stitch(_dev(std), _dev(sub), _dev(bad), _dev(_taper(64, "hann")), 32)


# ------------------------------------------------------------------ end to end
L, HOP, W, H = 16000, 240, 64, 32
HOPS = H * HOP
T_TRACK = L + 2 * HOPS + 1000                                            # n = 4, the last chunk zero-padded


@functools.lru_cache(maxsize=None)
def _explainer(standard="clone", blur=5):
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
    from drsa_audio_amd.xai.explain.track import TrackExplainer
    hg = HeatmapGenerator(LC.toy().to(DEV), LC.ortho(16, 1), LRP_NAME_MAP_TOY, "class1", num_concepts=4, layer_idx=7,
                          device=DEV, standard=standard)
    return TrackExplainer(hg, AG._m2a("toy", blur_kernel=blur), hop_frames=H)


@functools.lru_cache(maxsize=None)
def _track(T=T_TRACK):
    from drsa_audio_amd.utils.synthetic import synthetic_songs
    w = synthetic_songs(1, seconds=3.0, seed=3)[0][:T].copy()
    assert w.shape == (T,)
    w.setflags(write=False)
    return w


def test_heatmaps_are_the_reference_stitch_of_the_generators_chunk_maps():
    """Chunking, per-chunk peak normalisation, un-sorting and cropping: the test cuts and transforms
    the chunks itself (the log-mel kernel's strided form over the padded track), asks the generator
    for their maps, and stitches them with track_ref."""
    ex, wav = _explainer(), _track()
    res = ex.explain(_dev(wav), audio=False)
    n, T_pad, Wt, Wr = 4, L + 3 * HOPS, 160, T_TRACK // HOP
    assert (res.n_chunks, res.silent_chunks, res.chunk_starts) == (n, [], [0, HOPS, 2 * HOPS, 3 * HOPS])
    pad = np.zeros(T_pad, dtype=np.float32)
    pad[:T_TRACK] = wav
    x = ex.loader._run(_dev(pad), 1, T_pad, n, HOPS, L, peak_norm=True, clamp=True)
    hg = ex.generator
    hg.generate_subspace_heatmaps(x)
    info = hg.info
    assert any((info["mask"][c] != np.arange(4)).any() for c in range(n))          # the chunks do sort differently
    ref = TR.stitch(info["standard_heatmaps"].reshape(n, 1, 64, 64), info["subspace_heatmaps"], info["mask"],
                    _taper(W, "hann"), H)
    got = res.heatmaps.cpu().numpy()
    assert got.shape == (5, 64, Wr) and Wr == 134 < Wt
    assert np.array_equal(got.view(np.int32), ref[:, :, :Wr].view(np.int32))
    assert res.activity.shape == (5, Wr) and res.relevances.shape == (5,)
    assert torch.equal(res.relevances, res.activity.sum(-1))
    assert sorted(res.order.tolist()) == [0, 1, 2, 3]
    rel = res.relevances[1:].cpu().numpy()
    assert (np.diff(rel[res.order.cpu().numpy()]) <= 0).all()
    assert np.array_equal(res.frame_times.cpu().numpy(), (np.arange(Wr) + 1) * HOP / 16000)
    assert res.audios is None and res.stft_heatmaps is None


def test_concept_maps_sum_to_the_standard_map():
    """standard="sum": a chunk's standard map is the float32 sum of its K concept maps, in some order:
    within (K - 1) 2^-24 sum_k |x_k| of their exact sum.  The stitch is linear with positive normalised
    weights, so that error arrives as at most (K - 1) 2^-24 sum_k mag_k (mag_k = the stitch of |x_k|),
    and every stitched map is within track_ref.chain_bound x its own mag of its float64 stitch."""
    ex, wav = _explainer("sum"), _track()
    res = ex.explain(_dev(wav), audio=False)
    _, chunks, (n, _, _, Wr) = ex.chunks(_dev(wav))
    std, sub, order = (v.cpu().numpy() for v in ex.chunk_maps(chunks, list(range(n))))
    _, mag = TR.stitch_f64(std, sub, order, _taper(W, "hann"), H)
    mag = mag[:, :, :Wr]
    K, cb = 4, TR.chain_bound(2)
    bound = cb * mag.sum(0) + (K - 1) * 2.0 ** -24 * (1 + 2.0 ** -20) * mag[1:].sum(0)
    hm = res.heatmaps.double().cpu().numpy()
    err = np.abs(hm[1:].sum(0) - hm[0])
    print(f"\n  linearity: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all() and float(np.abs(hm[0]).max()) > 0


def test_all_ones_maps_render_the_track_itself():
    """All-ones STFT maps, no cut (percentile None), no blur (a one-tap kernel: the mask is exactly 1):
    the un-normalised concept audios are track samples [hop, hop Wr).  Map 0 is always cut at
    percentile 50, which keeps nothing of a map of ties: its audio is exactly 0."""
    ex, wav = _explainer(blur=1), _track()
    pad, _, (n, T_pad, Wt, Wr) = ex.chunks(_dev(wav))
    ones = torch.ones(5, 241, Wr, device=DEV)
    out = ex.render(pad, ones, percentile=None)
    assert out.shape == (5, HOP * (Wr - 1))
    assert float(out[0].abs().max()) == 0.0
    padn = pad.cpu().numpy()
    want = np.broadcast_to(padn[HOP:HOP * Wr].astype(np.float64), (4, HOP * (Wr - 1)))
    g = S.geometry(480, HOP, 64, Wr)
    _, X32 = S.analysis(padn[None], g, "torch32")
    t32 = S.synthesis(X32[0], torch.ones(4, 241, Wr), g, "torch32").numpy()
    AG.audio_check(out[1:], want, t32, "track all-ones identity")


def test_a_silent_tail_is_reported_and_stays_exactly_zero():
    ex = _explainer()
    T = L + 4 * HOPS                                                     # n = 5, no padding
    wav = np.zeros(T, dtype=np.float32)
    wav[:20000] = _track()[:20000]                                       # chunks 3 and 4 start at 23040 and 30720
    res = ex.explain(_dev(wav))
    assert res.n_chunks == 5 and res.silent_chunks == [3, 4]
    Wr = 192
    assert res.heatmaps.shape == (5, 64, Wr) and res.stft_heatmaps.shape == (5, 241, Wr)
    assert res.audios.shape == (5, HOP * (Wr - 1))
    for t in (res.heatmaps, res.stft_heatmaps, res.activity, res.relevances, res.audios):
        assert torch.isfinite(t).all()
    # chunk 2 ends at column 127: from 128 on only silent chunks cover
    assert float(res.heatmaps[..., 128:].abs().max()) == 0.0 == float(res.stft_heatmaps[..., 128:].abs().max())
    assert float(res.activity[:, 128:].abs().max()) == 0.0
    assert float(res.heatmaps[..., :128].abs().amax((1, 2)).min()) > 0


def test_a_track_shorter_than_one_chunk():
    ex = _explainer()
    T = 12000
    res = ex.explain(_dev(_track()[:T].copy()), percentile=90)
    Wr = T // HOP
    assert res.n_chunks == 1 and Wr == 50
    assert res.heatmaps.shape == (5, 64, Wr) and res.stft_heatmaps.shape == (5, 241, Wr)
    assert res.audios.shape == (5, HOP * (Wr - 1)) and torch.isfinite(res.audios).all()
    assert float(res.audios.abs().amax(-1).min()) == 1.0                 # Mel2AudioToy: peak-normalised audios
