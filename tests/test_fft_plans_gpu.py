"""The generic Stockham FFT (csrc/stockham.h) at every radix plan and overlap depth, through the
three kernels that run it: logmel_kernel (any n_fft but 800), stft_mel_phase_kernel (analysis) and
mel_to_audio_kernel (synthesis, the transform run as an inverse).  GPU.

The plans and geometries are the tables of tests/fft_plan_cases.py (tests/test_fft_plans_cpu.py
shows what they reach: radix 2, 3 and 5 as a first pass, every radix with twiddles, one to five
passes, odd M, fewer than 64 butterflies, partly masked last trips, overlap depths 1..8).

Tolerance: the project's anchored gates, imported and not restated.  Stage level (the spectrum X,
the mel, the log-mel): ``anchored`` of test_audiogen_gpu / test_logmel_gpu, the maximum and the
RMS of the error against the float64 oracle at most RATIO = 2 x the float32 oracle chain's (+ the
1e-7 floor).  Audios: ``audio_check``, each audio's relative L2 distance, median and worst.
Inputs are uniform noise (no quiet bins for a log to amplify) and positive heatmaps; the
filterbanks are well conditioned (tests/test_fft_plans_cpu.py).  The signal-level known answers
use no oracle: their bound is the standard FFT rounding bound, see ``_fft_bound``.

Measured on MI355X, error against float64, HIP vs torch32, range over the 16 plans (8 .. 1024):
  X        max 2.5e-7 .. 6.3e-6 vs 2.5e-7 .. 6.8e-6, RMS 1.1e-7 .. 1.7e-6 vs 1.0e-7 .. 1.7e-6;
           largest ratio 1.34 (max, n_fft 64), 1.15 (RMS, n_fft 10)
  mel      largest ratio 1.75 (max, n_fft 10: 1.1e-6 vs 6.5e-7, 2-3 ulp of the values), 1.33 (RMS, n_fft 12)
  log-mel  max 2.3e-7 .. 1.7e-6 vs 2.3e-7 .. 1.6e-6, RMS 7.8e-8 .. 3.3e-7 vs 7.3e-8 .. 3.3e-7;
           largest ratio 1.44 (max, n_fft 36), 1.26 (RMS, n_fft 36)
  audios, plans 8 .. 720, relative L2, median / worst over 6 audios:
           8.1e-8 .. 1.8e-7 / 8.7e-8 .. 1.9e-7 vs 6.9e-8 .. 1.7e-7 / 8.6e-8 .. 1.9e-7; largest ratio 1.17 (n_fft 8)
  audios, overlap depths 1 .. 8, median / worst over 10 audios:
           8.5e-8 .. 1.6e-7 / 9.3e-8 .. 1.6e-7 vs 8.9e-8 .. 1.5e-7 / 9.5e-8 .. 1.6e-7; largest ratio 1.05 (64/40)
No plan missed a gate.  The whole file takes 3 s.

What a wrong stockham.h does here (tried on scratch builds, never committed):
  bfly2's second output negated     test_analysis_spectrum_and_mel, test_logmel_generic_kernel,
                                    test_synthesis_same_inputs_both_sides at every plan with a radix-2
                                    pass (12, 16, 36, 64, 100, 108, 256, 720, 960, 1024), test_overlap_depth
                                    at n_fft 64, 36, 720, both known-answer tests at 12, 64, 720; no older test
  tw[r * k] for tw[r * k * tstep]   the same four at every plan of three or more passes, the known answers at
                                    64 and 720 (the older audio tests fail too: 480 and 800 have four passes)
  no twiddles when Ns == 2          the same four at 12, 36, 100, 108 and the known answers at 12; no older test
  Z[1] for Z[0] in the split's      test_analysis_spectrum_and_mel at all 16 plans, the known answers at all
  k == M branch                     four (the Nyquist bin has weight 0 in every mel filter, so no mel shows it;
                                    the older test_analysis_mel_and_spectrum fails too)
"""
import functools

import numpy as np
import pytest
import torch

import audiogen_ref as R
import fft_plan_cases as P
import logmel_ref as L
import test_audiogen_gpu as AG
import test_logmel_gpu as LM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SYNTH = [p for p in P.PLANS if p[0] <= P.SYNTH_MAX_N_FFT]
REFUSED = [p for p in P.PLANS if p[0] > P.SYNTH_MAX_N_FFT]
KNOWN = [p for p in P.PLANS if p[0] in (12, 30, 64, 720)]


def _ids(rows):
    return [f"nfft{r[0]}" for r in rows]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _loader(n_fft, hop, n_mels, width):
    from drsa_audio_amd.utils.dataloading import Loader
    return Loader(None, sample_rate=P.SR, n_fft=n_fft, hop_length=hop, n_mels=n_mels, slice_length=0, width=width,
                  device=DEV)


def _m2a(n_fft, hop, n_mels, width, power):
    from drsa_audio_amd.xai.explain.audiogen import Mel2Audio
    return Mel2Audio(loader=_loader(n_fft, hop, n_mels, width), power=power, blur_kernel=P.blur_size(n_mels, width))


def _geom(n_fft, hop, n_mels, width, power):
    return dict(sr=P.SR, n_fft=n_fft, hop=hop, n_mels=n_mels, width=width, power=power, frame0=0)


@functools.lru_cache(maxsize=None)
def _noise(n_fft, hop, width, rem, frame0=0, batch=P.BATCH):
    """Uniform noise chunks whose last STFT frame is frame0 + width - 1 (read-only, shared)."""
    Lw = P.chunk_len(hop, width, rem, frame0)
    wav = np.random.default_rng(n_fft + hop).uniform(-1, 1, (batch, Lw)).astype(np.float32)
    wav.setflags(write=False)
    return wav


# ------------------------------------------------------------- a. analysis
@pytest.mark.parametrize("row", P.PLANS, ids=P.PLAN_IDS)
def test_analysis_spectrum_and_mel(row):
    """stft_mel_phase_kernel: X and mel of every frame of the chunk (frame 0 reflects on the left,
    the last one on the right) against the oracle's float64 and float32 chains."""
    n_fft, _, hop, n_mels, width, power, rem, _ = row
    wav = _noise(n_fft, hop, width, rem)
    assert 1 + wav.shape[-1] // hop == width
    mel, X = _loader(n_fft, hop, n_mels, width).analyse(_dev(wav), frame0=0, width=width, power=power)
    assert mel.shape == (P.BATCH, n_mels, width) and X.shape == (P.BATCH, width, n_fft // 2 + 1)
    g = _geom(n_fft, hop, n_mels, width, power)
    mel64, X64 = R.analysis(wav, g, "f64")
    mel32, X32 = R.analysis(wav, g, "torch32")
    assert X64.shape[-1] == width
    AG.anchored(X.transpose(1, 2), X64, X32, f"n_fft {n_fft} X")
    AG.anchored(mel, mel64, mel32, f"n_fft {n_fft} mel")


@pytest.mark.parametrize("row", [p for p in P.PLANS if p[0] in (10, 720)], ids=["nfft10", "nfft720"])
def test_analysis_peak_norm_in_kernel(row):
    n_fft, _, hop, n_mels, width, power, rem, _ = row
    wav = _noise(n_fft, hop, width, rem)
    ld = _loader(n_fft, hop, n_mels, width)
    meln, Xn = ld.analyse(_dev(wav), frame0=0, width=width, power=power, peak_norm=True)
    wn = wav / np.abs(wav).max(-1, keepdims=True)
    mel2, X2 = ld.analyse(_dev(wn), frame0=0, width=width, power=power, peak_norm=False)
    assert torch.equal(meln, mel2) and torch.equal(Xn, X2)


# -------------------------------------------------------------- b. log-mel
def _logmel_case(n_fft, hop, n_mels, width, rem):
    """transform_wav (frames 1..width, the last one the chunk's last) vs logmel_ref, as
    test_logmel_gpu.test_n_fft_800_kernel_odd_shapes."""
    from drsa_audio_amd import _capi
    ld = _loader(n_fft, hop, n_mels, width)
    smem = _capi.lib().drsa_amd_logmel_smem_bytes(n_fft, hop, n_mels, width, ld.tables(DEV)["nnz"])
    assert 0 < smem <= 160 * 1024, smem
    wav = _noise(n_fft, hop, width, rem, frame0=1)
    assert wav.shape[-1] // hop == width
    out = ld.transform_wav(_dev(wav), clamp=False).cpu().numpy()
    assert out.shape == (P.BATCH, 1, n_mels, width)
    mel = L.mel_spectrogram(wav.astype(np.float64), n_fft, hop, n_mels, P.SR)
    assert mel.shape[-1] == width + 1
    ref = np.log10(mel + 1e-7)[..., 1:width + 1].reshape(P.BATCH, 1, n_mels, width)
    m32 = L.mel_spectrogram(np.asarray(wav), n_fft, hop, n_mels, P.SR, mode="torch32")
    t32 = np.log10(m32 + np.float32(1e-7))[..., 1:width + 1].reshape(P.BATCH, 1, n_mels, width)
    return LM.anchored(out, ref, t32)


@pytest.mark.parametrize("row", P.PLANS, ids=P.PLAN_IDS)
def test_logmel_generic_kernel(row):
    n_fft, _, hop, n_mels, width, _, rem, _ = row
    _logmel_case(n_fft, hop, n_mels, width, rem)


def test_logmel_hop_wider_than_the_frame():
    """hop > n_fft (the log-mel allows it, the audio back end refuses it): the 8-frame sample
    block holds gaps that no frame reads."""
    _logmel_case(30, 37, 6, 11, 5)


# ------------------------------------------------------------ c. synthesis
def _synthesis_case(n_fft, hop, n_mels, width, power, rem, B, C):
    """The kernel's own float32 mel and X and generate_mask's masks -> (Mel2Audio, out, oracle f64,
    oracle float32, the device inputs)."""
    m = _m2a(n_fft, hop, n_mels, width, power)
    wav = _noise(n_fft, hop, width, rem, batch=B)
    mel, X = m._analyse(_dev(wav), peak_norm=True)
    habs = R.heatmaps(B, C, n_mels, width, seed=n_fft + width, absolute=True)
    masks = torch.stack([torch.stack([m.generate_mask(_dev(h), m.smoother, 50) for h in hs]) for hs in habs])
    assert float(masks.amax((-1, -2)).min()) > 0
    out = m._synthesise(mel, X, masks)
    assert out.shape == (B, C, hop * (width - 1))
    g = _geom(n_fft, hop, n_mels, width, power)
    ref, t32 = (np.stack([R.synthesis(mel[b].cpu(), X[b].t().cpu(), masks[b].cpu(), g, mode).numpy()
                          for b in range(B)]) for mode in ("f64", "torch32"))
    return m, out, ref, t32, (mel, X, masks)


@pytest.mark.parametrize("row", SYNTH, ids=_ids(SYNTH))
def test_synthesis_same_inputs_both_sides(row):
    n_fft, _, hop, n_mels, width, power, rem, _ = row
    _, out, ref, t32, _ = _synthesis_case(n_fft, hop, n_mels, width, power, rem, P.BATCH, 2)
    AG.audio_check(out, ref, t32, f"n_fft {n_fft} hop {hop} synthesis")


@pytest.mark.parametrize("row", REFUSED, ids=_ids(REFUSED))
def test_synthesis_refuses_what_does_not_fit_the_lds(row):
    """The analysis runs at these sizes; the synthesis' 16 waves x 2 ping-pong buffers do not fit
    160 KB and the entry point says so (DRSA_EUNSUPPORTED)."""
    from drsa_audio_amd._capi import DRSA_EUNSUPPORTED, DrsaAmdError
    n_fft, _, hop, n_mels, width, power, rem, _ = row
    m = _m2a(n_fft, hop, n_mels, width, power)
    mel, X = m._analyse(_dev(_noise(n_fft, hop, width, rem)), peak_norm=True)
    masks = torch.ones(P.BATCH, 1, n_mels, width, device=DEV)
    with pytest.raises(DrsaAmdError, match=rf"rc={DRSA_EUNSUPPORTED}\).*LDS footprint \d+ B exceeds 160 KB"):
        m._synthesise(mel, X, masks)


# -------------------------------------------------------- d. overlap depth
@pytest.mark.parametrize("geo", P.OVERLAPS, ids=P.OVERLAP_IDS)
def test_overlap_depth(geo):
    """Every G = 16 - extra the entry point accepts, over several spans with a partial last one
    (and the one-hop audio of width 2): the oracle gate, and a batch of 5 sources x 2 masks equals
    each source run alone, bit for bit (the owned overlap-add's fixed order)."""
    n_fft, hop, n_mels, width, power = geo
    m, out, ref, t32, (mel, X, masks) = _synthesis_case(n_fft, hop, n_mels, width, power, hop // 3, 5, 2)
    extra = P.overlap_geometry(n_fft, hop, width)[0]
    AG.audio_check(out, ref, t32, f"n_fft {n_fft} hop {hop} width {width} extra {extra}")
    for i in range(5):
        one = m._synthesise(mel[i:i + 1].contiguous(), X[i:i + 1].contiguous(), masks[i:i + 1].contiguous())
        assert torch.equal(out[i:i + 1], one), i


# ------------------------------------------------- e. signal-level known answers
def _fft_bound(n_fft, scale):
    """8 eps32 log2(n_fft) max|X|: the standard bound on a floating-point FFT's error, a small
    constant x eps x log2 N relative to the spectrum's size (Higham, Accuracy and Stability of
    Numerical Algorithms, 24.1).  Reasoned, not measured."""
    return 8.0 * np.finfo(np.float32).eps * np.log2(n_fft) * scale


@pytest.mark.parametrize("row", KNOWN, ids=_ids(KNOWN))
def test_impulse_spectrum_is_the_window_sample(row):
    """A unit impulse at sample n0: a frame that starts at s and holds n0 (and no reflected copy of
    it) has X[k] = w[n0 - s] W_N^{k (n0 - s)}, so |X[k]| = w[n0 - s] at every k; a frame that does
    not hold it is zero."""
    n_fft, _, hop, n_mels, width, power, rem, _ = row
    Lw = P.chunk_len(hop, width, rem)
    tc = width // 2
    n0 = tc * hop - n_fft // 2 + n_fft // 3 + 1
    wav = np.zeros((1, Lw), dtype=np.float32)
    wav[0, n0] = 1.0
    _, X = _loader(n_fft, hop, n_mels, width).analyse(_dev(wav), frame0=0, width=width, power=power)
    X = X[0].cpu().numpy().astype(np.complex128)                               # [width, n_freq]
    w = torch.hann_window(n_fft).double().numpy()
    k = np.arange(n_fft // 2 + 1)
    seen = 0
    for t in range(width):
        s = t * hop - n_fft // 2
        if s < 0 or s + n_fft > Lw:
            continue                                                           # reflected frames: not judged here
        off = n0 - s
        want = w[off] * np.exp(-2j * np.pi * k * off / n_fft) if 0 <= off < n_fft else np.zeros(k.size)
        seen += 0 <= off < n_fft
        bound = _fft_bound(n_fft, np.abs(want).max())
        assert np.abs(np.abs(X[t]) - np.abs(want)).max() <= bound, (t, off)
        assert np.abs(X[t] - want).max() <= bound, (t, off)
    assert seen >= 1 and w[n0 - (tc * hop - n_fft // 2)] > 0.5


@pytest.mark.parametrize("row", KNOWN, ids=_ids(KNOWN))
def test_constant_signal_is_the_window_transform(row):
    """A constant c (reflect padding keeps it constant, so every frame counts): X = c DFT(w), the
    Hann window's transform, c N/2 at bin 0, -c N/4 at bin 1 and nothing above."""
    n_fft, _, hop, n_mels, width, power, rem, _ = row
    c = 0.75
    wav = np.full((1, P.chunk_len(hop, width, rem)), c, dtype=np.float32)
    _, X = _loader(n_fft, hop, n_mels, width).analyse(_dev(wav), frame0=0, width=width, power=power)
    X = X[0].cpu().numpy().astype(np.complex128)
    want = c * np.fft.rfft(torch.hann_window(n_fft).double().numpy())           # of the float32 window's values
    assert abs(want[0] - c * n_fft / 2) <= 1e-5 * n_fft and abs(want[1] + c * n_fft / 4) <= 1e-5 * n_fft
    bound = _fft_bound(n_fft, np.abs(want).max())
    assert np.abs(X - want[None]).max() <= bound
    assert np.abs(X[:, 2:]).max() <= bound + np.abs(want[2:]).max()
