"""Concept-audio back end: the host-side pieces (no GPU): the pseudo-inverse table, the rank
rule of the percentile cut, the blur taps, the volume helpers, the window envelope, and the
argument checks of the C entry points (all rejected before any device work)."""
import ctypes

import numpy as np
import pytest
import torch

import audiogen_ref as R
from drsa_audio_amd import _capi
from drsa_audio_amd.utils.dataloading import Loader, mel_pinv
from drsa_audio_amd.utils.sound import adjust_vol, rms_normalizer
from drsa_audio_amd.xai.explain import audiogen as AG


# ------------------------------------------------------------------ pinv table
@pytest.mark.parametrize("case,rank,s_lo,s_hi", [("gtzan", 125, 0.518, 2.78), ("toy", 64, 0.153, 2.96)])
def test_pinv_table_moore_penrose_and_conditioning(case, rank, s_lo, s_hi):
    t = Loader(case).tables(torch.device("cpu"))
    A = t["fb"].to(torch.float64).numpy().T                    # [n_mels, n_freq]: mel = A |X|
    P = mel_pinv(t["fb"])
    assert P.shape == (A.shape[1], A.shape[0]) and P.dtype == np.float64
    for lhs, rhs in ((A @ P @ A, A), (P @ A @ P, P), ((A @ P).T, A @ P), ((P @ A).T, P @ A)):
        assert np.abs(lhs - rhs).max() <= 1e-10
    s = np.linalg.svd(A, compute_uv=False)
    keep = s > 1e-6 * s[0]
    assert keep.sum() == rank == np.linalg.matrix_rank(A, tol=1e-6 * s[0])
    # the quoted figures are rounded to three digits
    assert abs(s[keep].min() - s_lo) <= 6e-4 and abs(s[0] - s_hi) <= 6e-3, (s[keep].min(), s[0])
    assert (s[~keep] < 1e-10 * s[0]).all()                     # the gap: nothing between 1e-10 and the kept ones
    assert torch.equal(t["pinv"], torch.from_numpy(P).to(torch.float32))
    assert torch.equal(t["pinv_t"], t["pinv"].t())
    assert np.array_equal(P, R.pinv(R.filterbank(2 * (A.shape[1] - 1), A.shape[0], 16000)))


# ------------------------------------------------------------------- rank rule
def _three_case_rule(hp, p):
    """The definition as the feature states it: v = p/100 (n-1), lo = floor(v); a whole v keeps
    hp > a[lo]; else hp >= a[lo+1] when a[lo] < a[lo+1], and hp > a[lo] when they tie."""
    a = np.sort(hp.ravel())
    v = p / 100 * (a.size - 1)
    lo = int(np.floor(v))
    if v == lo or a[lo] == a[lo + 1]:
        return hp > a[lo]
    return hp >= a[lo + 1]


@pytest.mark.parametrize("p", [0, 50, 90, 100])
@pytest.mark.parametrize("kind", ["random", "half_zero", "ties"])
def test_rank_rule_equals_numpy_percentile(p, kind):
    rng = np.random.default_rng(p + len(kind))
    for shape in ((64, 64), (41, 61), (128, 128)):
        h = rng.standard_normal(shape).astype(np.float32)
        if kind == "random":
            hp = np.abs(h)
        elif kind == "half_zero":
            hp = np.maximum(h, 0)
        else:
            hp = np.round(np.abs(h) * 2).astype(np.float32) / 2        # a handful of distinct values
            assert np.unique(hp).size < 16
        ref = hp > np.percentile(hp.astype(np.float64), p)
        assert np.array_equal(AG.rank_keep(hp, p), ref)
        assert np.array_equal(_three_case_rule(hp, p), ref)
        assert np.array_equal(R.kept(hp, p) if p else AG.rank_keep(hp, p), ref)


def test_gaussian_taps_formula():
    for k, sigma in ((5, 1.0), (1, 1.0), (7, 2.5), (3, 0.4)):
        x = np.linspace(-(k - 1) / 2, (k - 1) / 2, k)
        w = np.exp(-0.5 * (x / sigma) ** 2)
        w /= w.sum()
        taps = AG.gaussian_taps(k, sigma)
        assert taps.dtype == torch.float32 and taps.shape == (k,)
        assert np.abs(taps.numpy() - w).max() <= 2e-7
        assert abs(float(taps.sum()) - 1) <= 2e-7
    with pytest.raises(ValueError):
        AG.GaussianBlur(4, 1.0)


# --------------------------------------------------------------- sound helpers
def test_adjust_vol_and_rms_normalizer_closed_forms():
    t = torch.arange(4000) / 16000
    a1 = 0.25 * torch.sin(2 * np.pi * 400 * t)                  # RMS 0.25 / sqrt(2)
    a2 = 0.9 * torch.sign(torch.sin(2 * np.pi * 100 * t + 0.1))  # square wave, RMS 0.9
    out = adjust_vol(a1, a2)
    want = a2 * (0.25 / np.sqrt(2) / 0.9)
    assert torch.allclose(out, want, rtol=1e-5, atol=0)
    assert abs(float(out.pow(2).mean().sqrt()) - 0.25 / np.sqrt(2)) <= 1e-6
    # the clamp: a spiky signal brought to a loud one's RMS would exceed 1
    spike = torch.zeros(4000)
    spike[::100] = 0.5
    loud = adjust_vol(a2, spike)
    gain = 0.9 / float(spike.pow(2).mean().sqrt())
    assert gain * 0.5 > 1 and float(loud.max()) == 1.0 and float(loud.min()) == 0.0
    assert torch.equal(loud, torch.clamp(spike * torch.abs(a2.pow(2).mean().sqrt() / spike.pow(2).mean().sqrt()), -1, 1))
    # sign of the ratio is dropped, numpy inputs are accepted
    assert torch.allclose(adjust_vol(a1.numpy(), -a2.numpy()), -want, rtol=1e-5, atol=0)
    x = torch.stack([a1, a2, 3.0 * a1])
    for db in (0, -20):
        y = rms_normalizer(x, db)
        assert torch.allclose(y.pow(2).mean(-1).sqrt(), torch.full((3,), 10 ** (db / 20)), rtol=1e-5)
        assert torch.allclose(y[0], y[2], rtol=1e-5, atol=1e-7)   # scale invariant per row


# ------------------------------------------------------------ window envelope
def test_istft_envelope_host_table_and_refusal():
    lib = _capi.load()
    for n_fft, hop, width, lowest in ((800, 360, 128, 0.669), (480, 240, 64, None)):
        win = torch.hann_window(n_fft)
        env = torch.empty(hop * (width - 1))
        assert lib.drsa_amd_istft_envelope(win.data_ptr(), n_fft, hop, width, env.data_ptr()) == 0
        w2 = win.to(torch.float64) ** 2
        full = torch.zeros((width - 1) * hop + n_fft, dtype=torch.float64)
        for t in range(width):
            full[t * hop:t * hop + n_fft] += w2
        ref = full[n_fft // 2:n_fft // 2 + hop * (width - 1)]
        assert torch.equal(env, ref.to(torch.float32))
        if lowest:
            assert abs(float(env.min()) - lowest) < 1e-3
    # a rectangular window that is zero over one hop's worth of every frame: gaps in the envelope
    win = torch.ones(480)
    win[:240] = 0
    env = torch.empty(480 * 9)
    assert lib.drsa_amd_istft_envelope(win.data_ptr(), 480, 480, 10, env.data_ptr()) == _capi.DRSA_EINVAL
    assert b"sum of squares" in lib.drsa_amd_last_error()
    assert lib.drsa_amd_istft_envelope(None, 480, 240, 10, env.data_ptr()) == _capi.DRSA_EINVAL
    assert lib.drsa_amd_istft_envelope(win.data_ptr(), 480, 481, 10, env.data_ptr()) == _capi.DRSA_EINVAL


# ------------------------------------------------------- argument rejections
_BUF = (ctypes.c_double * 4)()                                           # 8-byte aligned
_P = ctypes.cast(_BUF, ctypes.c_void_p)
_ODD = ctypes.c_void_p(_P.value + 4)
_VALID = {
    "stft_mel_phase": dict(wav=_P, n_chunks=1, chunk_stride=16000, chunk_len=16000, n_fft=480, hop=240, n_mels=64,
                           width=64, frame0=0, power=1, window=_P, band_lo=_P, band_n=_P, band_off=_P, band_w=_P,
                           band_nnz=4, peak_norm=0, mel=_P, X=_P, stream=None),
    "heatmap_mask": dict(heatmaps=_P, n_maps=1, H=64, W=64, group=1, rank_first=-1, rank_rest=-1, taps=_P, k=5,
                         mask=_P, stream=None),
    "mel_to_audio": dict(mel=_P, X=_P, mask=_P, n_src=1, C=1, n_fft=480, hop=240, n_mels=64, width=64, power=1,
                         window=_P, pinv_t=_P, envelope=_P, audio=_P, stream=None),
    "audio_normalize": dict(audio=_P, n_audio=1, len=100, wav=None, wav_stride=0, wav_len=0, C=1, stream=None),
}
_EINVAL, _EUNSUP = _capi.DRSA_EINVAL, _capi.DRSA_EUNSUPPORTED
_REJECTIONS = [
    ("stft_mel_phase", dict(wav=None), _EINVAL, "null"),
    ("stft_mel_phase", dict(X=None), _EINVAL, "null"),
    ("stft_mel_phase", dict(power=3), _EINVAL, "power"),
    ("stft_mel_phase", dict(power=0), _EINVAL, "power"),
    ("stft_mel_phase", dict(hop=481), _EINVAL, "hop"),
    ("stft_mel_phase", dict(n_fft=28, hop=7), _EINVAL, "factor"),           # n_fft/2 = 14 = 2 * 7
    ("stft_mel_phase", dict(n_fft=481), _EINVAL, "even"),
    ("stft_mel_phase", dict(width=70), _EINVAL, "frames"),
    ("stft_mel_phase", dict(chunk_len=200), _EINVAL, "reflect"),
    ("heatmap_mask", dict(heatmaps=None), _EINVAL, "null"),
    ("heatmap_mask", dict(taps=None), _EINVAL, "null"),
    ("heatmap_mask", dict(H=128, W=320), _EUNSUP, "LDS"),                   # 160 KB map + tables
    ("heatmap_mask", dict(H=200, W=256), _EUNSUP, "LDS"),
    ("heatmap_mask", dict(k=4), _EINVAL, "odd"),
    ("heatmap_mask", dict(H=2, W=64), _EINVAL, "reflect"),
    ("heatmap_mask", dict(rank_first=64 * 64), _EINVAL, "rank"),
    ("heatmap_mask", dict(group=0), _EINVAL, "group"),
    ("mel_to_audio", dict(mel=None), _EINVAL, "null"),
    ("mel_to_audio", dict(envelope=None), _EINVAL, "null"),
    ("mel_to_audio", dict(power=4), _EINVAL, "power"),
    ("mel_to_audio", dict(hop=500), _EINVAL, "hop"),
    ("mel_to_audio", dict(n_fft=44, hop=11), _EINVAL, "factor"),            # n_fft/2 = 22 = 2 * 11
    ("mel_to_audio", dict(hop=20), _EUNSUP, "overlaps"),
    ("mel_to_audio", dict(n_fft=4096, hop=1024), _EUNSUP, "LDS"),
    ("mel_to_audio", dict(width=1), _EINVAL, "width"),
    ("audio_normalize", dict(audio=None), _EINVAL, "null"),
    ("audio_normalize", dict(wav=_P, wav_len=0), _EINVAL, "wav_len"),
    # new rows go last: a row's place in the table is part of its test id
    ("stft_mel_phase", dict(X=_ODD), _EINVAL, "aligned"),                   # X is written as float2
    ("mel_to_audio", dict(X=_ODD), _EINVAL, "aligned"),                     # X is read as float2
]


@pytest.mark.parametrize("entry,changes,code,needle", _REJECTIONS)
def test_entry_points_reject_bad_arguments(entry, changes, code, needle):
    lib = _capi.load()
    args = dict(_VALID[entry], **changes)
    rc = getattr(lib, "drsa_amd_" + entry)(*args.values())
    msg = lib.drsa_amd_last_error().decode()
    assert rc == code, (rc, msg)
    assert entry in msg and needle in msg, msg


def test_largest_supported_maps_pass_the_size_check():
    """128x128 and 128x256 maps fit (the check that refuses 128x320 lets them through): with
    n_maps = 0 the call returns before any device work."""
    lib = _capi.load()
    for H, W in ((128, 128), (128, 256)):
        args = dict(_VALID["heatmap_mask"], H=H, W=W, n_maps=0)
        assert lib.drsa_amd_heatmap_mask(*args.values()) == 0, lib.drsa_amd_last_error()


def test_no_cpu_path():
    m = AG.Mel2Audio("toy", device=None)
    if m.device is None:
        with pytest.raises(_capi.DrsaAmdError):
            m.transform_audio(np.zeros(16000, dtype=np.float32))
    with pytest.raises(_capi.DrsaAmdError):
        AG.heatmap_masks(torch.zeros(64, 64), None, -1, -1)
