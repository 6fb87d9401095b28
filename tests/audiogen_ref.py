"""CPU oracle for the concept-audio back end (xai/explain/audiogen.py).  TEST INFRASTRUCTURE ONLY
(a helper module: pytest does not collect it).

Restates the five steps of the feature's definition with torch.stft / torch.istft, F.conv2d and
numpy, in one dtype chosen by ``mode``: "f64" is the anchor, "torch32" the same chain in float32
(the precision an eager float32 implementation of the chain reaches).

    analysis    centred reflect-padded STFT, periodic Hann; mel = fb^T |X|^power; phase = X/|X|
                (1 where |X| = 0); frames frame0..frame0+width-1
    mask        relu; hp * (hp > np.percentile(hp, p)) when p is truthy; Gaussian blur (taps
                exp(-(x/sigma)^2/2) on linspace(-(k-1)/2, (k-1)/2, k), sum 1; separable; reflect)
    inversion   mag = relu(P (mel * mask))^(1/power), P = pinv(fb^T) (float64, rcond 1e-6)
    synthesis   torch.istft(mag * phase, center=True): length hop (width - 1)
    normalise   a / max|a|; clamp(a * |rms(wav) / rms(a)|, -1, 1)

Plan constants are shared by both modes, as they are the product's constants and not part of the
arithmetic under test: the filterbank is the Loader's own (torchaudio's float32 formula,
``logmel_ref.melscale_fbanks(mode="torch32")``; the float64 formula differs from it by ~1e-5
relative per entry, far above the chain's rounding), and P is its float64 pseudo-inverse, cast to
the mode's dtype.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import logmel_ref as L

GEOM = {
    "gtzan": dict(sr=16000, n_fft=800, hop=360, n_mels=128, width=128, power=1, frame0=0),
    "toy": dict(sr=16000, n_fft=480, hop=240, n_mels=64, width=64, power=2, frame0=1),
}


def _dt(mode):
    return torch.float64 if mode == "f64" else torch.float32


def filterbank(n_fft, n_mels, sr) -> np.ndarray:
    """[n_freq, n_mels] float32 values (the Loader's)."""
    return L.melscale_fbanks(n_fft // 2 + 1, 0.0, float(sr // 2), n_mels, sr, mode="torch32")


def pinv(fb: np.ndarray) -> np.ndarray:
    return np.linalg.pinv(fb.astype(np.float64).T, rcond=1e-6)           # [n_freq, n_mels]


def analysis(wav, g, mode="f64"):
    """wav [B, L] -> mel [B, n_mels, width], X [B, n_freq, width] (complex) as torch tensors."""
    dt = _dt(mode)
    x = torch.as_tensor(np.asarray(wav)).to(dt)
    X = torch.stft(x, g["n_fft"], hop_length=g["hop"], win_length=g["n_fft"],
                   window=torch.hann_window(g["n_fft"], dtype=dt), center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    X = X[..., g["frame0"]:g["frame0"] + g["width"]]
    fb = torch.from_numpy(filterbank(g["n_fft"], g["n_mels"], g["sr"])).to(dt)
    mel = torch.matmul(fb.t(), X.abs() ** g["power"])
    return mel, X


def unit_phase(X):
    mag = X.abs()
    return torch.where(mag > 0, X / mag, torch.ones_like(X))


def kept(h, percentile):
    """Boolean kept set of one map [H, W] (float32 input; the cut is decided in float64)."""
    hp = np.maximum(np.asarray(h, dtype=np.float64), 0.0)
    if not percentile:
        return np.ones(hp.shape, dtype=bool)
    return hp > np.percentile(hp, percentile)


def gaussian_taps(k, sigma, dt):
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=dt)
    pdf = torch.exp(-0.5 * (x / sigma) ** 2)
    return pdf / pdf.sum()


def mask(h, percentile, k=5, sigma=1.0, mode="f64"):
    """One map [H, W] -> its mask [H, W] (torch, mode's dtype)."""
    dt = _dt(mode)
    hp = torch.relu(torch.as_tensor(np.asarray(h)).to(dt))
    hp = hp * torch.from_numpy(kept(h, percentile)).to(dt)
    taps = gaussian_taps(k, sigma, dt)
    z = F.pad(hp[None, None], (k // 2,) * 4, mode="reflect") if k > 1 else hp[None, None]
    z = F.conv2d(z, taps.view(1, 1, 1, k))
    z = F.conv2d(z, taps.view(1, 1, k, 1))
    return z[0, 0]


def synthesis(mel, X, masks, g, mode="f64"):
    """mel [n_mels, width], X [n_freq, width], masks [C, n_mels, width] -> audio [C, hop (width-1)]."""
    dt = _dt(mode)
    cdt = torch.complex128 if mode == "f64" else torch.complex64
    P = torch.from_numpy(pinv(filterbank(g["n_fft"], g["n_mels"], g["sr"]))).to(dt)
    mel, X, masks = mel.to(dt), X.to(cdt), masks.to(dt)
    mag = torch.relu(torch.matmul(P, mel[None] * masks)) ** (1.0 / g["power"])
    Y = mag * unit_phase(X)[None]
    return torch.istft(Y, g["n_fft"], hop_length=g["hop"], win_length=g["n_fft"],
                       window=torch.hann_window(g["n_fft"], dtype=dt), center=True)


def peak_normalizer(a):
    return a / a.abs().max(dim=-1, keepdim=True)[0]


def adjust_vol(a1, a2):
    rms = lambda s: torch.sqrt(torch.mean(s ** 2))                        # noqa: E731
    return torch.clamp(a2 * torch.abs(rms(a1) / rms(a2)), -1, 1)


def make_audios_batch(std, sub, wavs, g, percentile=50, k=5, sigma=1.0, mode="f64", volume_match=True,
                      normalise=True):
    """std [B, H, W], sub [B, K, H, W], wavs [B, L] (float32 arrays) -> [B, K+1, hop (width-1)] numpy."""
    dt = _dt(mode)
    out = []
    for b in range(len(wavs)):
        w = torch.as_tensor(np.asarray(wavs[b])).to(dt)
        mel, X = analysis(peak_normalizer(w)[None], g, mode)
        ms = [mask(std[b], 50, k, sigma, mode)] + [mask(h, percentile, k, sigma, mode) for h in sub[b]]
        au = synthesis(mel[0], X[0], torch.stack(ms), g, mode)
        if normalise:
            au = torch.stack([adjust_vol(w, peak_normalizer(a)) if volume_match else peak_normalizer(a) for a in au])
        out.append(au)
    return torch.stack(out).numpy()


def rel_l2(a, ref):
    """Per-audio relative L2 distance over the last axis (float64)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.sqrt(((a - ref) ** 2).sum(-1)) / np.sqrt((ref ** 2).sum(-1))


def signals(B, Lw, seed=0, sr=16000):
    """Noise + a tone + a chirp, scaled well below 1; source 1 has no tone."""
    rng = np.random.default_rng(seed)
    t = np.arange(Lw) / sr
    out = []
    for b in range(B):
        x = 0.05 * rng.standard_normal(Lw)
        if b != 1:
            x += 0.3 * np.sin(2 * np.pi * (440.0 + 170.0 * b) * t)
        x += 0.2 * np.sin(2 * np.pi * (300.0 + (1500.0 + 400.0 * b) * t) * t)
        out.append(0.5 * x)
    return np.stack(out).astype(np.float32)


def heatmaps(B, C, H, W, seed=0, absolute=False):
    """randn x per-row gain [B, C, H, W]; ``absolute`` makes every entry positive so that
    percentile 50 cuts inside the positive part."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((B, C, H, W)) * np.linspace(0.2, 2.0, H)[None, None, :, None]
    return (np.abs(h) if absolute else h).astype(np.float32)
