"""Whole-track explanations (no reference counterpart; DESIGN.md "Whole-track explanations"): one
track-length heatmap and one track-length audio per concept, from the per-chunk machinery of
``explainer.py`` and ``audiogen.py``.

The track is cut into chunks of the model's input length that overlap (``hop_frames`` STFT frames
from one to the next), every chunk is explained on its own, and the chunks' maps are stitched by a
tapered overlap-add (``drsa_amd_track_stitch``, ``csrc/track_stitch.hip``).  The stitch also
un-sorts: ``HeatmapGenerator`` orders a chunk's concepts by that chunk's relevances, the track's map
k is U's block k - 1 in every column.  The audio is rendered once, from the track's own spectrum
and the stitched STFT-resolution maps, and normalised once against the whole track.

Everything returns device tensors; there is no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from ... import _capi
from ...utils.dataloading import read_wav
from .audiogen import Mel2Audio
from .explainer import HeatmapGenerator


def track_grid(T: int, L: int, hop_length: int, W: int, hop_frames: Optional[int] = None) -> Tuple[int, int, int, int]:
    """The chunk grid of a track of T samples -> ``(n, T_pad, Wt, Wr)``.

    Chunks of L samples (W map columns) start every ``hopS = hop_frames * hop_length`` samples:
    n = 1 if T <= L else ceil((T - L) / hopS) + 1 chunks over the track zero-padded to
    ``T_pad = L + (n - 1) hopS`` samples.  Column t of chunk c is track column u = c hop_frames + t,
    frame u + 1 of the padded track's centred STFT (the log-mel's own one-frame offset);
    ``Wt = (n - 1) hop_frames + W`` columns in all, of which the first
    ``Wr = min(Wt, T // hop_length)`` have their frame centre inside the real track."""
    T, L, hop_length, W = int(T), int(L), int(hop_length), int(W)
    h = W // 2 if hop_frames is None else int(hop_frames)
    if T < 1:
        raise ValueError(f"track_grid: the track has no samples (T = {T})")
    if hop_length < 1 or W < 1:
        raise ValueError(f"track_grid: hop_length = {hop_length} and W = {W} must be positive")
    if h < 1:
        raise ValueError(f"track_grid: hop_frames = {h} must be at least 1")
    if h > W:
        raise ValueError(f"track_grid: hop_frames = {h} > W = {W} would leave gaps between the chunks")
    if L < W * hop_length:
        raise ValueError(f"track_grid: a chunk of L = {L} samples is shorter than its W = {W} columns of "
                         f"{hop_length} samples")
    hopS = h * hop_length
    n = 1 if T <= L else -(-(T - L) // hopS) + 1
    Wt = (n - 1) * h + W
    return n, L + (n - 1) * hopS, Wt, min(Wt, T // hop_length)


def cover(u: int, W: int, h: int, n: int) -> range:
    """The chunks that cover track column u, ascending."""
    return range(max(0, -(-(u - W + 1) // h)), min(n - 1, u // h) + 1)


def make_taper(W: int, kind: str = "hann") -> torch.Tensor:
    """The stitch weights [W] (float64 on the host, rounded to float32): ``"hann"`` is
    sin^2(pi (t + 0.5) / W), symmetric and never zero; ``"flat"`` is all ones."""
    if kind == "hann":
        t = (np.arange(W, dtype=np.float64) + 0.5) / W
        v = np.sin(np.pi * t) ** 2
        v[W - W // 2:] = v[:W // 2][::-1]          # symmetric to the bit: the second half mirrors the first
        return torch.from_numpy(v.astype(np.float32))
    if kind == "flat":
        return torch.ones(W, dtype=torch.float32)
    raise ValueError(f'taper must be "hann" or "flat", got {kind!r}')


def track_stitch(std: Optional[torch.Tensor], sub: torch.Tensor, order: Optional[torch.Tensor], taper: torch.Tensor,
                 hop_frames: int, check_order: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """``drsa_amd_track_stitch``: std [n, 1, H, W] (or None), sub [n, K, H, W], order [n, K] int64 (or
    None: identity), taper [W] -> (out [C, H, Wt], act [C, Wt]) with C = K + 1 (K without std).
    ``check_order`` verifies on the device that every row of ``order`` is a permutation (one sync)."""
    _capi.require_gpu(sub, "sub", dtype=torch.float32)
    _capi.require_gpu(taper, "taper", dtype=torch.float32)
    if sub.dim() != 4:
        raise ValueError(f"track_stitch: sub must be [n, K, H, W], got {tuple(sub.shape)}")
    n, K, H, W = sub.shape
    h = int(hop_frames)
    if std is not None:
        _capi.require_gpu(std, "std", dtype=torch.float32)
        if tuple(std.shape) != (n, 1, H, W):
            raise ValueError(f"track_stitch: std must be {(n, 1, H, W)}, got {tuple(std.shape)}")
    if tuple(taper.shape) != (W,):
        raise ValueError(f"track_stitch: taper must be [{W}], got {tuple(taper.shape)}")
    if order is not None:
        _capi.require_gpu(order, "order", dtype=torch.int64)
        if tuple(order.shape) != (n, K):
            raise ValueError(f"track_stitch: order must be {(n, K)}, got {tuple(order.shape)}")
        if check_order and not bool((order.sort(-1).values == torch.arange(K, device=order.device)).all()):
            raise ValueError("track_stitch: every row of order must be a permutation of 0..K-1")
    if not 1 <= h <= W:
        raise ValueError(f"track_stitch: hop_frames = {h} must be in 1..W = {W}")
    C, Wt = K + (std is not None), (n - 1) * h + W
    out = torch.empty(C, H, Wt, device=sub.device)
    act = torch.empty(C, Wt, device=sub.device)
    nbytes = int(_capi.lib().drsa_amd_track_stitch_workspace_bytes(C, H, Wt))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=sub.device) if nbytes else None
    _capi.call("drsa_amd_track_stitch", _capi.ptr(std), sub.data_ptr(), _capi.ptr(order), taper.data_ptr(), n, K, H, W,
               h, out.data_ptr(), act.data_ptr(), _capi.ptr(ws), nbytes, _capi.stream_ptr(sub.device))
    return out, act


@dataclass
class TrackExplanation:
    """What ``TrackExplainer.explain`` returns (device tensors; K concepts, Wr columns).  Map 0 is the
    standard heatmap's, map k concept k - 1 = U's block k - 1 everywhere."""
    heatmaps: torch.Tensor                  # [K+1, n_mels, Wr]
    activity: torch.Tensor                  # [K+1, Wr]   a map's column sums
    relevances: torch.Tensor                # [K+1]       the sum of activity
    order: torch.Tensor                     # [K] int64   concepts by descending relevance (reported, never applied)
    frame_times: torch.Tensor               # [Wr]        seconds: (u + 1) hop_length / sample_rate
    chunk_starts: List[int]                 # [n]         samples
    n_chunks: int
    silent_chunks: List[int]                # chunks of digital silence (not sent to the engine)
    stft_heatmaps: Optional[torch.Tensor] = None   # [K+1, n_freq, Wr]
    audios: Optional[torch.Tensor] = None          # [K+1, hop_length (Wr - 1)]: sample s is track sample s + hop_length


class TrackExplainer:
    """``generator`` explains the chunks, ``mel2audio`` (same geometry) lifts and renders them.
    ``hop_frames``: the chunk step in STFT frames, 1..mel_width (default mel_width // 2);
    ``taper``: "hann" or "flat"; ``batch_size``: chunks per engine call (default: all)."""

    def __init__(self, generator: HeatmapGenerator, mel2audio: Mel2Audio, hop_frames: Optional[int] = None,
                 taper: str = "hann", batch_size: Optional[int] = None) -> None:
        if not isinstance(generator, HeatmapGenerator):
            raise TypeError("TrackExplainer takes a HeatmapGenerator (MultiHeatmapGenerator is not supported)")
        self.generator, self.mel2audio, self.loader = generator, mel2audio, mel2audio.loader
        ld = self.loader
        self.W, self.hop_length = ld.width, ld.hop_length
        self.L = int(ld.slice_length * ld.sample_rate)
        self.hop_frames = self.W // 2 if hop_frames is None else int(hop_frames)
        track_grid(self.L, self.L, self.hop_length, self.W, self.hop_frames)    # refuses a bad geometry now
        if batch_size is not None and batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        self.batch_size = batch_size
        self._taper_host = make_taper(self.W, taper)
        self._taper = {}

    def taper(self, device: torch.device) -> torch.Tensor:
        key = str(device)
        if key not in self._taper:
            self._taper[key] = self._taper_host.to(device)
        return self._taper[key]

    # ----------------------------------------------------------------- stages
    def chunks(self, wav) -> Tuple[torch.Tensor, torch.Tensor, Tuple[int, int, int, int]]:
        """wav [T] -> (the zero-padded track [T_pad], its chunks [n, L], the grid)."""
        dev = self.mel2audio._dev()
        w = wav if isinstance(wav, torch.Tensor) else torch.as_tensor(np.asarray(wav))
        if w.dim() != 1:
            raise ValueError(f"explain takes one channel [T], got {tuple(w.shape)}")
        w = w.detach().to(device=dev, dtype=torch.float32)
        grid = track_grid(w.numel(), self.L, self.hop_length, self.W, self.hop_frames)
        n, T_pad = grid[:2]
        pad = torch.zeros(T_pad, device=dev)
        pad[:w.numel()] = w
        return pad, pad.unfold(0, self.L, self.hop_frames * self.hop_length).contiguous(), grid

    def chunk_maps(self, chunks: torch.Tensor, live: List[int]):
        """The generator's maps of the live chunks, the silent ones all-zero with identity order:
        std [n, 1, H, W], sub [n, K, H, W], order [n, K]."""
        n, dev, K = chunks.size(0), chunks.device, self.generator.num_concepts
        H, W = self.loader.n_mels, self.W
        std, sub = torch.zeros(n, 1, H, W, device=dev), torch.zeros(n, K, H, W, device=dev)
        order = torch.arange(K, device=dev).repeat(n, 1)
        if live:
            idx = torch.tensor(live, device=dev)
            lc = chunks if len(live) == n else chunks[idx]
            x = self.loader._run(lc, lc.size(0), self.L, 1, 0, self.L, peak_norm=True, clamp=True)
            bs = self.batch_size or len(live)
            for b0 in range(0, len(live), bs):
                self.generator.generate_subspace_heatmaps(x[b0:b0 + bs], to_host=False)
                info, rows = self.generator.info_device, idx[b0:b0 + bs]
                if tuple(info["subspace_heatmaps"].shape[1:]) != (K, H, W):
                    raise ValueError(f"the generator's maps are {tuple(info['subspace_heatmaps'].shape[1:])}, the "
                                     f"front end's geometry gives {(K, H, W)}")
                std[rows] = info["standard_heatmaps"].reshape(-1, 1, H, W)
                sub[rows] = info["subspace_heatmaps"]
                order[rows] = info["mask"]
        return std, sub, order

    def chunk_stft_maps(self, chunks: torch.Tensor, live: List[int], std: torch.Tensor, sub: torch.Tensor):
        """``Mel2Audio.stft_heatmaps`` of the live chunks, zeros for the silent ones:
        std [n, 1, n_freq, W], sub [n, K, n_freq, W] in the slot order of ``sub``."""
        n, K, n_freq = chunks.size(0), sub.size(1), self.loader.n_fft // 2 + 1
        maps = torch.zeros(n, K + 1, n_freq, self.W, device=chunks.device)
        if live:
            idx = torch.tensor(live, device=chunks.device)
            every = len(live) == n
            maps[idx] = self.mel2audio.stft_heatmaps(std if every else std[idx], sub if every else sub[idx],
                                                     chunks if every else chunks[idx])
        return maps[:, :1].contiguous(), maps[:, 1:].contiguous()

    def spectrum(self, track_pad: torch.Tensor, Wr: int) -> torch.Tensor:
        """X [1, Wr, n_freq]: frames 1..Wr of the padded track as it is (no peak normalisation)."""
        return self.loader.analyse(track_pad[None], frame0=1, width=Wr, power=1, peak_norm=False)[1]

    def render(self, track_pad: torch.Tensor, stft_maps: torch.Tensor, percentile=50) -> torch.Tensor:
        """stft_maps [K+1, n_freq, Wr] -> un-normalised audios [K+1, hop_length (Wr - 1)]: map 0 cut at
        percentile 50, the others at ``percentile`` (not cut when it is falsy), over the whole track
        map (the rank rule of ``Mel2Audio._batch_masks``), blurred, times the track's spectrum, inverted."""
        masks = self.mel2audio._batch_masks(stft_maps[None].contiguous(), percentile)
        return self.mel2audio.stft_masks_to_audio(self.spectrum(track_pad, stft_maps.size(-1)), masks)[0]

    # ------------------------------------------------------------- end to end
    def explain(self, wav, audio: bool = True, percentile=50) -> TrackExplanation:
        track_pad, chunks, (n, T_pad, Wt, Wr) = self.chunks(wav)
        T = int(wav.shape[-1]) if hasattr(wav, "shape") else len(wav)
        h, dev = self.hop_frames, track_pad.device
        peaks = chunks.abs().amax(1).cpu()
        live = [c for c in range(n) if float(peaks[c]) > 0]
        silent = [c for c in range(n) if float(peaks[c]) == 0]
        if len(live) + len(silent) != n:
            raise ValueError("explain: the track holds NaN samples")
        std, sub, order = self.chunk_maps(chunks, live)
        taper = self.taper(dev)
        out, act = track_stitch(std, sub, order, taper, h)
        K = sub.size(1)
        activity = act[:, :Wr].contiguous()
        relevances = activity.sum(-1)
        res = TrackExplanation(
            heatmaps=out[:, :, :Wr].contiguous(), activity=activity, relevances=relevances,
            order=torch.argsort(relevances[1:], descending=True, stable=True),
            # float64 on the host: the device's float64 division is not the correctly rounded one
            frame_times=torch.from_numpy((np.arange(Wr) + 1) * self.hop_length / self.loader.sample_rate).to(dev),
            chunk_starts=[c * h * self.hop_length for c in range(n)], n_chunks=n, silent_chunks=silent)
        if audio:
            if Wr < 2:
                raise ValueError(f"explain: a track of {T} samples has {Wr} columns; the audio needs two")
            s_std, s_sub = self.chunk_stft_maps(chunks, live, std, sub)
            stft_out, _ = track_stitch(s_std, s_sub, order, taper, h, check_order=False)
            res.stft_heatmaps = stft_out[:, :, :Wr].contiguous()
            audios = self.render(track_pad, res.stft_heatmaps, percentile)
            res.audios = self.mel2audio.normalise(audios[None], track_pad[None, :T].contiguous())[0]
        return res

    def explain_file(self, path: str, audio: bool = True, percentile=50) -> TrackExplanation:
        """``explain`` of the first channel of a WAV file."""
        return self.explain(read_wav(path)[0], audio=audio, percentile=percentile)
