"""Concept audio: relevance heatmaps rendered to waveforms (reference
``cxai/xai/explain/audiogen.py``, ``Mel2Audio`` / ``Mel2AudioToy``) on the HIP kernels of
``csrc/audiogen.hip``.

For one source chunk and its heatmaps (DESIGN.md "Concept audio"):

1. analysis    centred reflect-padded STFT (periodic Hann), ``mel = fb^T |X|^power``, the phase
               ``X/|X|`` (1 where ``|X| = 0``).  Frames ``frame0..frame0+width-1`` with
               ``frame0 = 0``: the model input is frames 1..width, so heatmap column t masks mel
               frame t -- the reference's own one-hop offset (``transform_audio`` slices ``[:width]``).
2. mask        ``relu``, optional percentile cut (rank rule, below), Gaussian blur.
3. inversion   ``mag = relu(P (mel * mask))^(1/power)`` with ``P = pinv(fb^T)``.  This replaces
               librosa's NNLS ``mel_to_stft`` (whose L-BFGS-B refinement of this very point is not
               unique for an underdetermined bank) by the clipped least-squares solution it starts from.
4. synthesis   ``istft(mag * phase)``: window, overlap-add, window-envelope division, centre trim.
5. normalise   ``peak_normalizer`` per audio, then ``adjust_vol`` against the source waveform.

``resolution="stft"`` (DESIGN.md "Concept audio at STFT resolution", ``csrc/stft_audio.hip``) renders
the same heatmaps on the linear-frequency axis instead: the analysis is the model's own front end
(frames 1..width, power 1), the heatmaps are lifted through the filterbank onto the STFT bins
(``lift_to_stft``, an LRP z-rule), masked there, and the audio is ``istft(mask * X)``: no
pseudo-inverse, and an all-ones mask returns the chunk itself.

Everything returns device tensors; there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from ... import _capi
from ...utils.dataloading import Loader, read_wav
from ...utils.sound import get_slice


def gaussian_taps(kernel_size: int, sigma: float) -> torch.Tensor:
    """torchvision ``_get_gaussian_kernel1d``: exp(-(x/sigma)^2/2) on linspace(-(k-1)/2, (k-1)/2, k),
    normalised to sum 1 (float32)."""
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def percentile_rank(percentile: float, n: int) -> int:
    """Index ``lo = floor(percentile/100 * (n - 1))`` into the sorted map: the kept set of
    ``hp > np.percentile(hp, percentile)`` is ``hp > sorted(hp)[lo]``.  With v = p/100 (n-1):
    a whole v makes the percentile a[v] itself; a fractional one interpolates strictly inside
    (a[lo], a[lo+1]) when the two differ (keep hp >= a[lo+1], i.e. hp > a[lo]) and equals a[lo]
    when they tie."""
    return int(math.floor(percentile / 100 * (n - 1)))


def rank_keep(hp: np.ndarray, percentile: float) -> np.ndarray:
    """The rank rule on the host (numpy; the kernel's definition, used by the tests)."""
    a = np.sort(np.asarray(hp).ravel())
    return np.asarray(hp) > a[percentile_rank(percentile, a.size)]


class GaussianBlur:
    """The blur of ``generate_mask`` (torchvision ``GaussianBlur(kernel_size, sigma)``: separable
    taps, reflect padding) as a table for ``drsa_amd_heatmap_mask``."""

    def __init__(self, kernel_size: int = 5, sigma: float = 1.0) -> None:
        if kernel_size < 1 or kernel_size % 2 == 0:
            raise ValueError(f"kernel_size must be odd and positive, got {kernel_size}")
        self.kernel_size, self.sigma = int(kernel_size), float(sigma)
        self._taps = gaussian_taps(self.kernel_size, self.sigma)
        self._dev: Dict[str, torch.Tensor] = {}

    def taps(self, device: torch.device) -> torch.Tensor:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self._taps.to(device)
        return self._dev[key]


def _as_device(x, device: torch.device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def heatmap_masks(heatmaps: torch.Tensor, smoother: Optional[GaussianBlur], rank_first: int, rank_rest: int,
                  group: int = 1) -> torch.Tensor:
    """``drsa_amd_heatmap_mask`` over maps [..., H, W] (device, float32, contiguous); maps that
    do not fit its LDS (the entry answers DRSA_EUNSUPPORTED) go to ``drsa_amd_heatmap_mask_large``,
    whose results are bit-identical wherever both run."""
    _capi.require_gpu(heatmaps, "heatmap", dtype=torch.float32)
    smoother = smoother if smoother is not None else GaussianBlur(1, 1.0)
    H, W = heatmaps.shape[-2:]
    n_maps = heatmaps.numel() // (H * W)
    out = torch.empty_like(heatmaps)
    args = (heatmaps.data_ptr(), n_maps, H, W, group, rank_first, rank_rest, smoother.taps(heatmaps.device).data_ptr(),
            smoother.kernel_size, out.data_ptr(), _capi.stream_ptr(heatmaps.device))
    rc = _capi.lib().drsa_amd_heatmap_mask(*args)
    if rc == _capi.DRSA_EUNSUPPORTED:
        _capi.call("drsa_amd_heatmap_mask_large", *args)
    else:
        _capi.check(rc, "drsa_amd_heatmap_mask")
    return out


class Mel2Audio:
    """audiogen.py:15-206 (same constructor and method names) on the HIP back end."""

    power = 1          # mel = fb^T |X|^power
    frame0 = 0         # first STFT frame of the analysis
    volume_match = True

    def __init__(self, case: str = "gtzan", blur_kernel: int = 5, sigma: float = 1.0, device=None,
                 loader: Optional[Loader] = None, power: Optional[int] = None) -> None:
        """``loader`` (extension): a ``Loader`` of another geometry than ``AUDIO_PARAMS[case]``;
        ``power`` overrides the class's mel exponent."""
        ld = self.loader = loader if loader is not None else Loader(case=case, device=device)
        self.sample_rate, self.n_fft, self.hop_length = ld.sample_rate, ld.n_fft, ld.hop_length
        self.n_mels, self.width, self.slice_length = ld.n_mels, ld.width, ld.slice_length
        if power is not None:
            self.power = power
        self.device = self.loader.device
        self.smoother = GaussianBlur(blur_kernel, sigma)
        self._envelopes: Dict[Tuple[str, int], torch.Tensor] = {}

    # ------------------------------------------------------------------ plan
    def _dev(self) -> torch.device:
        if self.device is None:
            raise _capi.DrsaAmdError("Mel2Audio: no HIP device; drsa_audio_amd has no CPU path")
        return self.device

    def _width_for(self, L: int) -> int:
        return self.width

    def envelope(self, device: torch.device, width: int) -> torch.Tensor:
        """The window's overlap-added sum of squares over the kept span (``drsa_amd_istft_envelope``,
        host; raises when it is not invertible)."""
        key = (str(device), width)
        if key not in self._envelopes:
            win = torch.hann_window(self.n_fft).contiguous()
            env = torch.empty(self.hop_length * (width - 1))
            _capi.call("drsa_amd_istft_envelope", win.data_ptr(), self.n_fft, self.hop_length, width, env.data_ptr())
            self._envelopes[key] = env.to(device)
        return self._envelopes[key]

    # -------------------------------------------------------------- analysis
    def _analyse(self, wavs: torch.Tensor, peak_norm: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """wavs [B, L] -> mel [B, n_mels, width], X [B, width, n_freq] (complex)."""
        width = self._width_for(wavs.size(-1))
        return self.loader.analyse(wavs, frame0=self.frame0, width=width, power=self.power, peak_norm=peak_norm)

    def transform_audio(self, wav) -> Tuple[torch.Tensor, torch.Tensor]:
        """audiogen.py:148-158: one chunk -> (mel [n_mels, width], unit phase [n_freq, width])."""
        wav = _as_device(wav, self._dev()).reshape(1, -1)
        mel, X = self._analyse(wav, peak_norm=False)
        X = X[0].t()
        mag = X.abs()
        return mel[0], torch.where(mag > 0, X / mag, torch.ones_like(X))

    def transform_audio_from_file(self, path_to_sample: str, startpoint=None):
        """audiogen.py:160-170 with the stdlib WAV reader (first channel's slice)."""
        wav = read_wav(path_to_sample)
        if startpoint is not None:
            wav = get_slice(wav, slice_length=self.slice_length, start_point=startpoint, sample_rate=self.sample_rate)
        return self.transform_audio(wav[0] if wav.dim() > 1 else wav)

    # ------------------------------------------------------------------ mask
    @staticmethod
    def generate_mask(heatmap, smoother: Optional[GaussianBlur] = None, percentile=None, device=None) -> torch.Tensor:
        """audiogen.py:172-192: relu -> keep ``hp > np.percentile(hp, percentile)`` (when
        ``percentile`` is truthy, over the whole map) -> blur; squeezed, on the device."""
        dev = device if device is not None else (heatmap.device if isinstance(heatmap, torch.Tensor)
                                                 and heatmap.is_cuda else torch.device("cuda"))
        h = _as_device(heatmap, torch.device(dev))
        H, W = h.shape[-2:]
        if h.numel() != H * W:
            raise ValueError(f"generate_mask takes one map (np.percentile runs over all of it), got {tuple(h.shape)}")
        r = percentile_rank(percentile, H * W) if percentile else -1
        return heatmap_masks(h, smoother, r, r).reshape(H, W)

    # ------------------------------------------------------------- synthesis
    def _synthesise(self, mel: torch.Tensor, X: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
        """mel [B, n_mels, width], X [B, width, n_freq] complex, masks [B, C, n_mels, width]
        -> un-normalised audio [B, C, hop (width - 1)]."""
        B, C = masks.shape[:2]
        width = mel.size(-1)
        t = self.loader.tables(mel.device)
        env = self.envelope(mel.device, width)
        Xr = torch.view_as_real(X.contiguous())
        out = torch.empty(B, C, self.hop_length * (width - 1), device=mel.device)
        _capi.call("drsa_amd_mel_to_audio", mel.data_ptr(), Xr.data_ptr(), masks.data_ptr(), B, C, self.n_fft,
                   self.hop_length, self.n_mels, width, self.power, t["window"].data_ptr(), t["pinv_t"].data_ptr(),
                   env.data_ptr(), out.data_ptr(), _capi.stream_ptr(mel.device))
        return out

    def transform(self, heatmap, orig_mel, phase, percentile=None) -> torch.Tensor:
        """audiogen.py:114-146: one heatmap + the chunk's mel and phase -> un-normalised waveform."""
        dev = self._dev()
        mask = Mel2Audio.generate_mask(heatmap, self.smoother, percentile, device=dev)
        mel = _as_device(orig_mel, dev)
        ph = torch.as_tensor(phase).to(dev, torch.complex64)
        return self._synthesise(mel[None], ph.t().contiguous()[None], mask[None, None])[0, 0]

    # ------------------------------------------------------- STFT resolution
    def _require_model_shape(self, H: int, W: int) -> None:
        if (H, W) != (self.n_mels, self.width):
            raise ValueError(f"heatmaps are {H}x{W} but the model input is {self.n_mels}x{self.width}")

    def analyse_stft(self, wavs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """wavs [B, L] (not yet peak-normalised) -> mel [B, n_mels, width], X [B, width, n_freq]
        (complex) of the model's own front end, whatever the class: frames 1..width of the
        peak-normalised chunk, power 1 (``Loader.transform_wav``'s log-mel is log10 of this mel + 1e-7)."""
        return self.loader.analyse(wavs, frame0=1, width=self.width, power=1, peak_norm=True)

    def lift_to_stft(self, heatmaps: torch.Tensor, mel: torch.Tensor, X: torch.Tensor, eps: float = 1e-7
                     ) -> torch.Tensor:
        """Relevance at the log-mel input -> relevance on the STFT bins (``drsa_amd_mel_relevance_to_stft``):
        heatmaps [B, C, n_mels, width], mel and X as ``analyse_stft`` returns them -> [B, C, n_freq, width].
        An LRP z-rule through the filterbank; log10, the clamp and the normalisation are elementwise
        and pass relevance unchanged, the log offset ``eps`` absorbs:
        ``R_stft[f, t] = |X[t, f]| sum_m fb[f, m] R[m, t] / (mel[m, t] + eps)``."""
        for name, t in (("heatmaps", heatmaps), ("mel", mel)):
            _capi.require_gpu(t, name, dtype=torch.float32)
        _capi.require_gpu(X, "X", dtype=torch.complex64)
        B, n_mels, width = mel.shape
        n_freq = self.n_fft // 2 + 1
        if heatmaps.dim() != 4 or (heatmaps.size(0), *heatmaps.shape[2:]) != (B, n_mels, width) \
                or tuple(X.shape) != (B, width, n_freq) or n_mels != self.n_mels:
            raise ValueError(f"lift_to_stft: heatmaps {tuple(heatmaps.shape)}, mel {tuple(mel.shape)} and "
                             f"X {tuple(X.shape)} do not fit each other or the {self.n_mels} x {n_freq} filterbank")
        C = heatmaps.size(1)
        t = self.loader.tables(mel.device)
        out = torch.empty(B, C, n_freq, width, device=mel.device)
        _capi.call("drsa_amd_mel_relevance_to_stft", heatmaps.data_ptr(), mel.data_ptr(),
                   torch.view_as_real(X).data_ptr(), B, C, n_mels, width, n_freq, t["bin_lo"].data_ptr(),
                   t["bin_n"].data_ptr(), t["bin_off"].data_ptr(), t["bin_w"].data_ptr(), t["bin_nnz"], float(eps),
                   out.data_ptr(), _capi.stream_ptr(mel.device))
        return out

    def stft_heatmaps(self, standard_heatmaps, subspace_heatmaps=None, wavs=None) -> torch.Tensor:
        """Heatmaps on the linear-frequency axis: the arguments of ``make_audios_batch`` (a
        ``HeatmapGenerator.info`` dict is accepted too) -> [B, K+1, n_freq, width], map 0 the standard
        heatmap's.  Column t is STFT frame t + 1 of the peak-normalised chunk."""
        std, sub, wavs = self._batch_inputs(standard_heatmaps, subspace_heatmaps, wavs)
        self._require_model_shape(*sub.shape[-2:])
        mel, X = self.analyse_stft(wavs)
        return self.lift_to_stft(torch.cat([std, sub], dim=1), mel, X)

    def stft_masks_to_audio(self, X: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
        """X [B, width, n_freq] complex, masks [B, C, n_freq, width] -> un-normalised audio
        [B, C, hop (width - 1)] = istft(mask * X) (``drsa_amd_stft_mask_to_audio``)."""
        _capi.require_gpu(X, "X", dtype=torch.complex64)
        _capi.require_gpu(masks, "masks", dtype=torch.float32)
        B, width, n_freq = X.shape
        if masks.dim() != 4 or (masks.size(0), *masks.shape[2:]) != (B, n_freq, width) or n_freq != self.n_fft // 2 + 1:
            raise ValueError(f"stft_masks_to_audio: masks {tuple(masks.shape)} do not fit X {tuple(X.shape)} "
                             f"(n_fft {self.n_fft})")
        C = masks.size(1)
        t = self.loader.tables(X.device)
        env = self.envelope(X.device, width)
        out = torch.empty(B, C, self.hop_length * (width - 1), device=X.device)
        _capi.call("drsa_amd_stft_mask_to_audio", torch.view_as_real(X).data_ptr(), masks.data_ptr(), B, C, self.n_fft,
                   self.hop_length, width, t["window"].data_ptr(), env.data_ptr(), out.data_ptr(),
                   _capi.stream_ptr(X.device))
        return out

    def normalise(self, audios: torch.Tensor, wavs: torch.Tensor) -> torch.Tensor:
        """In place over audios [B, C, n] (``drsa_amd_audio_normalize``): ``peak_normalizer`` per
        audio, then (``volume_match``) ``adjust_vol`` against the source's waveform wavs [B, L]."""
        B, C, n = audios.shape
        _capi.call("drsa_amd_audio_normalize", audios.data_ptr(), B * C, n,
                   wavs.data_ptr() if self.volume_match else None, wavs.size(-1), wavs.size(-1), C,
                   _capi.stream_ptr(audios.device))
        return audios

    # ------------------------------------------------------------ end to end
    def _batch_inputs(self, standard_heatmaps, subspace_heatmaps, wavs):
        """The arguments of ``make_audios_batch`` as device tensors: std [B, 1, H, W], sub [B, K, H, W],
        wavs [B, L]."""
        if isinstance(standard_heatmaps, dict):
            info = standard_heatmaps
            standard_heatmaps, subspace_heatmaps = info["standard_heatmaps"], info["subspace_heatmaps"]
        dev = self._dev()
        std = _as_device(standard_heatmaps, dev)
        sub = _as_device(subspace_heatmaps, dev)
        wavs = _as_device(wavs, dev)
        wavs = wavs.reshape(-1, wavs.size(-1))
        B, K, H, W = sub.shape
        std = std.reshape(B, 1, H, W)
        if wavs.size(0) != B:
            raise ValueError(f"{B} sources of heatmaps but {wavs.size(0)} waveforms")
        return std, sub, wavs

    def make_audios_batch(self, standard_heatmaps, subspace_heatmaps=None, wavs=None, percentile=50,
                          resolution: str = "mel") -> torch.Tensor:
        """The batched ``make_audios``: standard_heatmaps [B, H, W] (or a ``HeatmapGenerator.info``
        dict holding both kinds), subspace_heatmaps [B, K, H, W], wavs [B, L] (as passed to
        ``make_audios``: not yet peak-normalised) -> [B, K+1, hop (width - 1)].  One analysis, one
        mask, one synthesis and one normalisation launch for the whole batch.  Audio 0 of a source
        is its standard heatmap's (always percentile 50, as the reference), audios 1..K its
        concepts' (``percentile``); each is peak-normalised and, for ``Mel2Audio``, brought to the
        RMS of the waveform that was passed in and clamped to [-1, 1].

        ``resolution="stft"``: the four STFT-resolution stages instead (``analyse_stft``,
        ``lift_to_stft``, ``heatmap_masks`` on the [n_freq, width] maps, ``stft_masks_to_audio``),
        then the same normalisation.  Output sample s is chunk sample s + hop."""
        if resolution not in ("mel", "stft"):
            raise ValueError(f'resolution must be "mel" or "stft", got {resolution!r}')
        std, sub, wavs = self._batch_inputs(standard_heatmaps, subspace_heatmaps, wavs)
        B, K, H, W = sub.shape
        if resolution == "stft":
            self._require_model_shape(H, W)
            mel, X = self.analyse_stft(wavs)
            maps = self.lift_to_stft(torch.cat([std, sub], dim=1), mel, X)
            return self.normalise(self.stft_masks_to_audio(X, self._batch_masks(maps, percentile)), wavs)
        mel, X = self._analyse(wavs, peak_norm=True)
        if (H, W) != tuple(mel.shape[1:]):
            raise ValueError(f"heatmaps are {H}x{W} but the mel is {mel.size(1)}x{mel.size(2)}")
        masks = self._batch_masks(torch.cat([std, sub], dim=1), percentile)
        return self.normalise(self._synthesise(mel, X, masks), wavs)

    def _batch_masks(self, maps: torch.Tensor, percentile) -> torch.Tensor:
        """The masks of maps [B, K+1, H, W]: a source's first map (its standard heatmap) is cut at
        percentile 50, the others at ``percentile`` (not cut when it is falsy)."""
        n = maps.size(-2) * maps.size(-1)
        return heatmap_masks(maps, self.smoother, percentile_rank(50, n),
                             percentile_rank(percentile, n) if percentile else -1, group=maps.size(1))

    def make_audios(self, sample_info: Dict[str, Union[np.ndarray, torch.Tensor]], original_audio=None,
                    startpoint=None, num_concepts: int = 4, percentile=50, path_to_sample: Optional[str] = None,
                    sample_idx: int = 0, resolution: str = "mel") -> List[torch.Tensor]:
        """audiogen.py:53-112: the list [standard, concept 0, ..., concept num_concepts-1] of
        explanation audios of one sample -- the B = 1 case of ``make_audios_batch``.
        ``sample_info`` holds ``standard_heatmap`` [H, W] (or ``standard_heatmaps`` [B, H, W], as
        ``HeatmapGenerator.info``, from which ``sample_idx`` picks) and ``subspace_heatmaps``."""
        if original_audio is None and path_to_sample is None:
            raise ValueError("make_audios needs original_audio or path_to_sample")
        if path_to_sample:
            if startpoint is None:
                raise ValueError("make_audios: path_to_sample needs the chunk's startpoint (seconds)")
            wav = get_slice(read_wav(path_to_sample), slice_length=self.slice_length, start_point=startpoint,
                            sample_rate=self.sample_rate)[0]
        else:
            wav = original_audio
        if "standard_heatmap" in sample_info:
            std, sub = sample_info["standard_heatmap"], sample_info["subspace_heatmaps"]
        else:
            std, sub = sample_info["standard_heatmaps"], sample_info["subspace_heatmaps"]
        std, sub = torch.as_tensor(np.asarray(std) if not torch.is_tensor(std) else std), \
            torch.as_tensor(np.asarray(sub) if not torch.is_tensor(sub) else sub)
        H, W = std.shape[-2:]
        if sub.dim() == 4:
            std, sub = std.reshape(-1, H, W)[sample_idx], sub[sample_idx]
        std, sub = std.reshape(1, H, W), sub.reshape(-1, H, W)[:num_concepts][None]
        wav = torch.as_tensor(np.asarray(wav) if not torch.is_tensor(wav) else wav).reshape(1, -1)
        return list(self.make_audios_batch(std, sub, wav, percentile=percentile, resolution=resolution)[0])


class Mel2AudioToy(Mel2Audio):
    """audiogen.py:210-358 on the same kernels: a power mel (``power = 2``), the frame window
    ``[1, n_frames - 2)`` of its ``transform_audio``, and audios that are peak-normalised only."""

    power = 2
    frame0 = 1
    volume_match = False

    def __init__(self, case: str = "toy", blur_kernel: int = 5, sigma: float = 1.0, device=None,
                 loader: Optional[Loader] = None, power: Optional[int] = None) -> None:
        super().__init__(case, blur_kernel, sigma, device, loader, power)

    def _width_for(self, L: int) -> int:
        return (1 + L // self.hop_length) - 3
