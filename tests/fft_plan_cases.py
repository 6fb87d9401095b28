"""Case tables and a plan model for the generic Stockham FFT (csrc/stockham.h) behind the log-mel
front end, the audio analysis and the audio synthesis.  TEST INFRASTRUCTURE ONLY (a helper module:
pytest does not collect it).  tests/test_fft_plans_cpu.py checks that the tables reach what they
claim; tests/test_fft_plans_gpu.py runs them on the kernels.
"""
from __future__ import annotations

import numpy as np

MAX_STAGES = 8          # LM_MAX_STAGES
TILE = 16               # AG_TF: frames per synthesis workgroup
SR = 16000


def radices(M: int):
    """``factor_radices`` of stockham.h: 4s first, then 2, then 3s, then 5s, at most 8 stages.
    Returns the list of passes, or None where the kernel refuses M."""
    r = []
    for R, test in ((4, 4), (2, 2), (3, 3), (5, 5)):
        while M % test == 0 and len(r) < MAX_STAGES:
            r.append(R)
            M //= R
    return r if M == 1 and r else None


def pass_shapes(M: int, plan):
    """[(R, Ns, MR)] of the plan's passes: radix, the sub-transform length on entry, and the
    number of butterflies M / R."""
    out, Ns = [], 1
    for R in plan:
        out.append((R, Ns, M // R))
        Ns *= R
    return out


def stockham_model(z, plan):
    """Forward M-point DFT of ``z[..., M]`` (complex128) by the kernel's passes.  One pass of
    radix R with sub-transform length Ns (``stockham_pass<R>`` in stockham.h), butterfly
    j < M/R:

        read     v[r] = in[j + r*M/R]
        twiddle  v[r] *= W_M^{r*k*M/(Ns*R)},  k = j % Ns       (skipped when Ns == 1)
        write    out[(j/Ns)*Ns*R + k + r*Ns] = DFT_R(v)[r]

    with W_M = exp(-2 pi i / M).  The passes alternate between two buffers; Ns grows by R."""
    x = np.asarray(z, dtype=np.complex128)
    M = x.shape[-1]
    for R, Ns, MR in pass_shapes(M, plan):
        j = np.arange(MR)
        k = j % Ns
        r = np.arange(R)[:, None]
        v = np.stack([x[..., j + q * MR] for q in range(R)], axis=-2)          # [..., R, MR]
        if Ns > 1:
            v = v * np.exp(-2j * np.pi * (r * k * (M // (Ns * R))) / M)
        y = np.einsum("sr,...rj->...sj", np.exp(-2j * np.pi * r * r.T / R), v)
        out = np.empty_like(x)
        out[..., ((j // Ns) * Ns * R + k) + r * Ns] = y
        x = out
    return x


def rfft_model(frame, plan):
    """rfft of a real frame [..., N] the kernels' way: pack z[n] = x[2n] + i x[2n+1], the
    M = N/2-point transform, then the real-input split

        X[k] = E[k] + W_N^k O[k],  E = (Z[k] + conj Z[M-k]) / 2,  O = (Z[k] - conj Z[M-k]) / (2i)

    for k = 0..M with Z[M] = Z[0] (the Nyquist bin comes from Z[0]; for odd M no bin pairs with
    itself)."""
    x = np.asarray(frame, dtype=np.float64)
    M = x.shape[-1] // 2
    Z = stockham_model(x[..., 0::2] + 1j * x[..., 1::2], plan)
    k = np.arange(M + 1)
    Zk, Zr = Z[..., k % M], np.conj(Z[..., (M - k) % M])
    return (Zk + Zr) / 2 + np.exp(-1j * np.pi * k / M) * (Zk - Zr) / 2j


def irfft_model(Y, plan):
    """irfft of a half spectrum Y[..., M+1] the synthesis kernel's way: the inverse packing

        Z[k] = (Y[k] + conj Y[M-k]) + i (Y[k] - conj Y[M-k]) conj(W_N^k),   k < M

    then z = conj(DFT(conj Z)) / 2 with the forward passes, x[2n] = Re z[n] / M,
    x[2n+1] = Im z[n] / M (the kernel folds the 1/2 and the 1/M into its 1/N).  The imaginary
    parts of Y[0] and Y[M] are dropped, as irfft does."""
    Y = np.array(Y, dtype=np.complex128)
    M = Y.shape[-1] - 1
    Y[..., 0] = Y[..., 0].real
    Y[..., M] = Y[..., M].real
    k = np.arange(M)
    Yk, Yc = Y[..., k], np.conj(Y[..., M - k])
    Z = (Yk + Yc) + 1j * (Yk - Yc) * np.exp(1j * np.pi * k / M)
    z = np.conj(stockham_model(np.conj(Z), plan)) / 2 / M
    x = np.empty(Y.shape[:-1] + (2 * M,))
    x[..., 0::2], x[..., 1::2] = z.real, z.imag
    return x


# n_fft, the passes of n_fft/2, hop, n_mels, width, power, L % hop, what the row reaches
PLANS = [
    (8, (4,), 3, 2, 5, 1, 2, "smallest accepted size; one pass; no twiddles; 1 butterfly"),
    (10, (5,), 5, 3, 19, 2, 0, "single radix-5 pass; odd M"),
    (12, (2, 3), 7, 3, 13, 1, 3, "radix 2 as first pass; radix 3 last with Ns = 2"),
    (16, (4, 2), 4, 4, 21, 2, 0, "radix 2 as last pass with twiddles"),
    (30, (3, 5), 11, 6, 9, 1, 5, "radix 3 as first pass; odd M"),
    (36, (2, 3, 3), 12, 8, 17, 2, 1, "radix 3 twice with Ns > 1"),
    (50, (5, 5), 30, 8, 11, 1, 7, "radix 5 first and with twiddles; odd M"),
    (64, (4, 4, 2), 20, 12, 23, 2, 0, "odd pass count: the result lands in the other ping-pong buffer"),
    (100, (2, 5, 5), 25, 12, 7, 1, 13, "radix 2 then radix 5 twice"),
    (108, (2, 3, 3, 3), 27, 16, 18, 2, 0, "even pass count with M < 64"),
    (256, (4, 4, 4, 2), 100, 24, 19, 1, 37, "radix-2 pass of exactly 64 butterflies"),
    (512, (4, 4, 4, 4), 128, 32, 10, 2, 0, "pure radix 4; even count; 4 passes"),
    (600, (4, 3, 5, 5), 361, 40, 14, 1, 100, "MR = 75 / 100 / 60: partial last trips"),
    (720, (4, 2, 3, 3, 5), 240, 40, 22, 2, 0, "all four radices in one plan; 5 passes; MR = 90 / 180 / 120 / 72"),
    (960, (4, 4, 2, 3, 5), 360, 40, 9, 1, 123, "all four radices in the other order; 5 passes"),
    (1024, (4, 4, 4, 4, 2), 256, 40, 13, 2, 5, "radix-2 pass of 4 trips per lane"),
]
BATCH = 3
SYNTH_MAX_N_FFT = 720       # above it the synthesis' LDS footprint exceeds 160 KB (DRSA_EUNSUPPORTED)
PLAN_IDS = [f"nfft{p[0]}" for p in PLANS]


def chunk_len(hop, width, rem, frame0=0):
    """The chunk length at which frame ``frame0 + width - 1`` is the last STFT frame, L // hop."""
    return (frame0 + width - 1) * hop + rem


# synthesis geometries (n_fft, hop, n_mels, width, power) by overlap depth
OVERLAPS = [
    (64, 40, 12, 37, 1),      # extra 1
    (64, 33, 12, 2, 2),       # extra 1, the minimum width
    (64, 24, 12, 50, 1),      # extra 2
    (64, 16, 12, 41, 2),      # extra 3: hop = n_fft / 4
    (50, 13, 8, 29, 1),       # extra 3, odd M
    (64, 13, 12, 30, 2),      # extra 4
    (64, 9, 12, 45, 1),       # extra 7
    (36, 5, 8, 40, 2),        # extra 7
    (36, 4, 8, 23, 1),        # extra 8
    (720, 80, 40, 20, 2),     # extra 8, five passes
]
OVERLAP_IDS = [f"nfft{o[0]}hop{o[1]}" for o in OVERLAPS]


def overlap_geometry(n_fft, hop, width):
    """(extra, G, nspan, partial) by drsa_amd_mel_to_audio's own formulas: the earlier frames that
    reach into a span, the hops a workgroup owns, the spans of one audio, and whether the last
    span is cut short."""
    extra = (n_fft + hop - 1) // hop - 1
    G = TILE - extra
    total = n_fft // 2 + hop * (width - 1)
    nspan = (total + G * hop - 1) // (G * hop)
    return extra, G, nspan, total % (G * hop) != 0


def blur_size(n_mels, width):
    """The largest odd blur kernel <= 5 whose reflect padding fits the map."""
    return min(5, 2 * min(n_mels, width) - 1)
