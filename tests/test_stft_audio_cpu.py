"""Concept audio at STFT resolution: what holds without a GPU.  The oracle's own identities
(tests/stft_audio_ref.py), the filterbank facts the lift relies on, the rank rule at the STFT map
size, and the argument checks of the three C entry points (all rejected before any device work).

Bounds: the float64 identities are sums of at most n_freq = 401 float64 terms, so 401 x 2^-53 =
4.5e-14 bounds their relative rounding error; 1e-12 is used.  The float32 round trip is bounded by
the FFT rounding bound of test_fft_plans_gpu._fft_bound, 8 eps32 log2(n_fft)."""
import ctypes

import numpy as np
import pytest
import torch

import audiogen_ref as R
import stft_audio_ref as S
from drsa_audio_amd import _capi
from drsa_audio_amd.utils.dataloading import Loader
from drsa_audio_amd.xai.explain import audiogen as AG

CASES = ["toy", "gtzan"]
LENGTH = {"toy": 16000, "gtzan": 48000}


# ------------------------------------------------------------ oracle identities
@pytest.mark.parametrize("case", CASES)
def test_reference_conserves_relevance(case):
    """sum_f R_stft[f][t] = sum_m R[m][t] mel / (mel + eps) in float64."""
    g = S.GEOM[case]
    wav = R.signals(2, LENGTH[case], seed=3).astype(np.float64)
    mel, X = S.analysis(wav, g, "f64")
    rel = R.heatmaps(2, 3, g["n_mels"], g["width"], seed=4)
    for b in range(2):
        lhs = S.lift(rel[b], mel[b], X[b], g, "f64").sum(-2)
        rhs = S.conserved(rel[b], mel[b])
        assert lhs.shape == rhs.shape == (3, g["width"])
        assert float((lhs - rhs).abs().max() / rhs.abs().max()) <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_reference_all_ones_mask_returns_the_chunk(case):
    """mask = 1: the synthesis of frames 1..width is wav[hop : hop width]."""
    g = S.GEOM[case]
    wav = R.signals(2, LENGTH[case], seed=5)
    want = wav[:, g["hop"]:g["hop"] * g["width"]]
    ones = torch.ones(1, g["n_fft"] // 2 + 1, g["width"])
    for mode, bound in (("f64", 1e-12), ("torch32", 8 * np.finfo(np.float32).eps * np.log2(g["n_fft"]))):
        _, X = S.analysis(wav if mode == "torch32" else wav.astype(np.float64), g, mode)
        out = np.stack([S.synthesis(X[b], ones, g, mode)[0].numpy() for b in range(2)])
        assert out.shape == want.shape
        assert R.rel_l2(out, want).max() <= bound, (mode, R.rel_l2(out, want))


# ------------------------------------------------------------- filterbank facts
@pytest.mark.parametrize("case", CASES)
def test_each_bin_is_covered_by_at_most_two_bands(case):
    g = S.GEOM[case]
    cover = S.bin_cover(g["n_fft"], g["n_mels"], g["sr"])
    assert cover.max() <= 2
    assert cover[0] == 0 and cover[g["n_fft"] // 2] == 0
    # the Loader's bin-by-bin tables are that bank: the same runs, the weights in ascending band order
    t = Loader(case).tables(torch.device("cpu"))
    fb = R.filterbank(g["n_fft"], g["n_mels"], g["sr"])
    assert np.array_equal(t["fb"].numpy(), fb)
    assert np.array_equal(t["bin_n"].numpy(), cover)
    for f in range(fb.shape[0]):
        lo, n, off = int(t["bin_lo"][f]), int(t["bin_n"][f]), int(t["bin_off"][f])
        assert np.array_equal(t["bin_w"][off:off + n].numpy(), fb[f, lo:lo + n]) and (fb[f, lo:lo + n] != 0).all()
        assert off + n <= t["bin_nnz"]


# ------------------------------------------------------------------- rank rule
@pytest.mark.parametrize("p", [50, 90, 97.5])
@pytest.mark.parametrize("kind", ["random", "half_zero", "ties"])
def test_rank_rule_equals_numpy_percentile_at_the_stft_map_size(p, kind):
    rng = np.random.default_rng(int(p) + len(kind))
    h = rng.standard_normal((401, 128)).astype(np.float32)
    if kind == "random":
        hp = np.abs(h)
    elif kind == "half_zero":
        hp = np.maximum(h, 0)
    else:
        hp = np.round(np.abs(h) * 2).astype(np.float32) / 2            # about a dozen distinct values
        assert np.unique(hp).size <= 12
    ref = hp > np.percentile(hp.astype(np.float64), p)
    assert np.array_equal(AG.rank_keep(hp, p), ref)
    assert np.array_equal(R.kept(hp, p), ref)


# ------------------------------------------------------- argument rejections
_BUF = (ctypes.c_double * 4)()                                           # 8-byte aligned
_P = ctypes.cast(_BUF, ctypes.c_void_p)
_ODD = ctypes.c_void_p(_P.value + 4)
_VALID = {
    "mel_relevance_to_stft": dict(relevance=_P, mel=_P, X=_P, n_src=1, C=1, n_mels=64, width=64, n_freq=241, bin_lo=_P,
                                  bin_n=_P, bin_off=_P, bin_w=_P, bin_nnz=4, eps=ctypes.c_float(1e-7), out=_P,
                                  stream=None),
    "heatmap_mask_large": dict(heatmaps=_P, n_maps=1, H=401, W=128, group=1, rank_first=-1, rank_rest=-1, taps=_P, k=5,
                               mask=_P, stream=None),
    "stft_mask_to_audio": dict(X=_P, mask=_P, n_src=1, C=1, n_fft=480, hop=240, width=64, window=_P, envelope=_P,
                               audio=_P, stream=None),
}
_EINVAL, _EUNSUP = _capi.DRSA_EINVAL, _capi.DRSA_EUNSUPPORTED
_REJECTIONS = [
    ("mel_relevance_to_stft", dict(relevance=None), _EINVAL, "null"),
    ("mel_relevance_to_stft", dict(X=None), _EINVAL, "null"),
    ("mel_relevance_to_stft", dict(bin_w=None), _EINVAL, "null"),
    ("mel_relevance_to_stft", dict(out=None), _EINVAL, "null"),
    ("mel_relevance_to_stft", dict(C=0), _EINVAL, "bad"),
    ("mel_relevance_to_stft", dict(width=0), _EINVAL, "bad"),
    ("mel_relevance_to_stft", dict(n_src=-1), _EINVAL, "bad"),
    ("mel_relevance_to_stft", dict(eps=ctypes.c_float(0.0)), _EINVAL, "eps"),
    ("mel_relevance_to_stft", dict(eps=ctypes.c_float(float("nan"))), _EINVAL, "eps"),
    ("mel_relevance_to_stft", dict(X=_ODD), _EINVAL, "aligned"),
    ("mel_relevance_to_stft", dict(n_freq=2049), _EUNSUP, "LDS"),         # 2049 x 33 floats alone are 264 KB
    ("heatmap_mask_large", dict(heatmaps=None), _EINVAL, "null"),
    ("heatmap_mask_large", dict(taps=None), _EINVAL, "null"),
    ("heatmap_mask_large", dict(mask=None), _EINVAL, "null"),
    ("heatmap_mask_large", dict(k=4), _EINVAL, "odd"),
    ("heatmap_mask_large", dict(k=65), _EINVAL, "odd"),
    ("heatmap_mask_large", dict(H=2, W=64), _EINVAL, "reflect"),
    ("heatmap_mask_large", dict(rank_first=401 * 128), _EINVAL, "rank"),
    ("heatmap_mask_large", dict(rank_rest=-2), _EINVAL, "rank"),
    ("heatmap_mask_large", dict(group=0), _EINVAL, "group"),
    ("heatmap_mask_large", dict(H=2049, W=2048), _EUNSUP, "elements"),    # one row above 2^22
    ("stft_mask_to_audio", dict(X=None), _EINVAL, "null"),
    ("stft_mask_to_audio", dict(envelope=None), _EINVAL, "null"),
    ("stft_mask_to_audio", dict(n_fft=481), _EINVAL, "even"),
    ("stft_mask_to_audio", dict(hop=500), _EINVAL, "hop"),
    ("stft_mask_to_audio", dict(n_fft=44, hop=11), _EINVAL, "factor"),     # n_fft/2 = 22 = 2 * 11
    ("stft_mask_to_audio", dict(hop=20), _EUNSUP, "overlaps"),
    ("stft_mask_to_audio", dict(n_fft=4096, hop=1024), _EUNSUP, "LDS"),
    ("stft_mask_to_audio", dict(n_fft=960, hop=360), _EUNSUP, "LDS"),      # 167 KB; 800 needs 139 KB
    ("stft_mask_to_audio", dict(width=1), _EINVAL, "width"),
    ("stft_mask_to_audio", dict(C=0), _EINVAL, "C >= 1"),
    ("stft_mask_to_audio", dict(X=_ODD), _EINVAL, "aligned"),
]


@pytest.mark.parametrize("entry,changes,code,needle", _REJECTIONS)
def test_entry_points_reject_bad_arguments(entry, changes, code, needle):
    lib = _capi.load()
    args = dict(_VALID[entry], **changes)
    rc = getattr(lib, "drsa_amd_" + entry)(*args.values())
    msg = lib.drsa_amd_last_error().decode()
    assert rc == code, (rc, msg)
    assert entry in msg and needle in msg, msg


def test_supported_sizes_pass_the_checks():
    """With no source or map to work on the calls return before any device work: the GTZAN and toy
    shapes, a 513 x 512 map, the largest map (2^22 elements) and the widest blur pass the checks."""
    lib = _capi.load()
    for H, W, k in ((401, 128, 5), (241, 64, 5), (513, 512, 5), (2048, 2048, 63), (41, 61, 9)):
        args = dict(_VALID["heatmap_mask_large"], H=H, W=W, k=k, n_maps=0)
        assert lib.drsa_amd_heatmap_mask_large(*args.values()) == 0, lib.drsa_amd_last_error()
    for n_mels, n_freq in ((64, 241), (128, 401)):
        args = dict(_VALID["mel_relevance_to_stft"], n_mels=n_mels, n_freq=n_freq, n_src=0)
        assert lib.drsa_amd_mel_relevance_to_stft(*args.values()) == 0, lib.drsa_amd_last_error()
    for n_fft, hop in ((480, 240), (800, 360)):
        args = dict(_VALID["stft_mask_to_audio"], n_fft=n_fft, hop=hop, n_src=0)
        assert lib.drsa_amd_stft_mask_to_audio(*args.values()) == 0, lib.drsa_amd_last_error()


# ------------------------------------------------------------------ interface
def test_unknown_resolution_raises():
    m = AG.Mel2Audio("toy", device=None)
    z = np.zeros((1, 64, 64), dtype=np.float32)
    with pytest.raises(ValueError, match="resolution"):
        m.make_audios_batch(z, z[None], np.zeros((1, 16000), dtype=np.float32), resolution="blur")
    with pytest.raises(ValueError, match="resolution"):
        m.make_audios({"standard_heatmap": z[0], "subspace_heatmaps": z}, np.zeros(16000, dtype=np.float32),
                      resolution="blur")
