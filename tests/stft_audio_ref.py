"""CPU oracle for concept audio at STFT resolution (csrc/stft_audio.hip, the ``resolution="stft"``
path of xai/explain/audiogen.py).  TEST INFRASTRUCTURE ONLY (a helper module: pytest does not
collect it).

Restates the four steps of the feature's definition on top of audiogen_ref.py, in one dtype chosen
by ``mode``: "f64" is the anchor, "torch32" the same chain in float32.

    analysis    audiogen_ref.analysis at the model's own front end: frames 1..width, power 1
    lift        q = R / (mel + eps);  a = fb q;  R_stft = |X| a        (the LRP z-rule through the bank)
    mask        audiogen_ref.mask on the [n_freq, width] map
    synthesis   torch.istft(mask * X, center=True): length hop (width - 1), sample s = chunk sample s + hop
    normalise   audiogen_ref.peak_normalizer / adjust_vol

Plan constants (the Loader's float32 filterbank, eps) are shared by both modes, as in audiogen_ref.
"""
from __future__ import annotations

import numpy as np
import torch

import audiogen_ref as R

EPS = 1e-7                                                   # the Loader's log offset
GEOM = {case: dict(g, power=1, frame0=1) for case, g in R.GEOM.items()}


def geometry(n_fft, hop, n_mels, width, sr=16000):
    return dict(sr=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, width=width, power=1, frame0=1)


def analysis(wav, g, mode="f64"):
    """wav [B, L] -> mel [B, n_mels, width], X [B, n_freq, width] of frames 1..width."""
    assert g["frame0"] == 1 and g["power"] == 1
    return R.analysis(wav, g, mode)


def lift(rel, mel, X, g, mode="f64", eps=EPS):
    """rel [C, n_mels, width], mel [n_mels, width], X [n_freq, width] -> [C, n_freq, width]."""
    dt = R._dt(mode)
    fb = torch.from_numpy(R.filterbank(g["n_fft"], g["n_mels"], g["sr"])).to(dt)     # [n_freq, n_mels]
    rel, mel = torch.as_tensor(np.asarray(rel)).to(dt), torch.as_tensor(np.asarray(mel)).to(dt)
    X = torch.as_tensor(np.asarray(X)).to(torch.complex128 if mode == "f64" else torch.complex64)
    q = rel / (mel + eps)
    return X.abs().to(dt) * torch.matmul(fb, q)


def conserved(rel, mel, eps=EPS):
    """The right-hand side of the conservation identity, float64: what the lifted maps of one
    frame sum to, sum_m R[m][t] mel[m][t] / (mel[m][t] + eps) -> [C, width]."""
    rel, mel = (torch.as_tensor(np.asarray(v)).to(torch.float64) for v in (rel, mel))
    return (rel * (mel / (mel + eps))).sum(-2)


def synthesis(X, masks, g, mode="f64"):
    """X [n_freq, width], masks [C, n_freq, width] -> audio [C, hop (width - 1)]."""
    dt = R._dt(mode)
    X = torch.as_tensor(np.asarray(X)).to(torch.complex128 if mode == "f64" else torch.complex64)
    Y = torch.as_tensor(np.asarray(masks)).to(dt) * X[None]
    return torch.istft(Y, g["n_fft"], hop_length=g["hop"], win_length=g["n_fft"],
                       window=torch.hann_window(g["n_fft"], dtype=dt), center=True)


def make_audios_batch(std, sub, wavs, g, percentile=50, k=5, sigma=1.0, mode="f64", volume_match=True,
                      normalise=True):
    """std [B, H, W], sub [B, K, H, W], wavs [B, L] (float32 arrays) -> [B, K+1, hop (width-1)] numpy."""
    dt = R._dt(mode)
    out = []
    for b in range(len(wavs)):
        w = torch.as_tensor(np.asarray(wavs[b])).to(dt)
        mel, X = analysis(R.peak_normalizer(w)[None], g, mode)
        maps = lift(np.concatenate([std[b][None], sub[b]]), mel[0], X[0], g, mode).numpy()
        ms = [R.mask(maps[0], 50, k, sigma, mode)] + [R.mask(h, percentile, k, sigma, mode) for h in maps[1:]]
        au = synthesis(X[0], torch.stack(ms), g, mode)
        if normalise:
            au = torch.stack([R.adjust_vol(w, R.peak_normalizer(a)) if volume_match else R.peak_normalizer(a)
                              for a in au])
        out.append(au)
    return torch.stack(out).numpy()


def bin_cover(n_fft, n_mels, sr=16000):
    """Number of bands with a nonzero weight on each bin [n_freq]."""
    return (R.filterbank(n_fft, n_mels, sr) != 0).sum(1)
