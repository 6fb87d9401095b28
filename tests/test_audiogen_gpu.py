"""Concept-audio back end (csrc/audiogen.hip, xai/explain/audiogen.py) vs the CPU oracle
tests/audiogen_ref.py (GPU).

Tolerance, anchored as in test_logmel_gpu.py: the oracle's float64 chain is the reference, its
float32 chain ("torch32") the yardstick, and the HIP result's distance from float64 may be at most
RATIO = 2 x torch32's (+ a 1e-7 floor where both are exact).  Stage tests use the maximum and the
RMS of the absolute error (``test_logmel_gpu.anchored``'s measure); audios use each audio's
relative L2 distance, the median and the worst over the test's audios.
"""
import numpy as np
import pytest
import torch

import audiogen_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RATIO = 2.0
FLOOR = 1e-7
TOY, GTZAN = R.GEOM["toy"], R.GEOM["gtzan"]


def anchored(out, ref, t32, what, ratio=RATIO):
    """max and RMS of |out - ref| <= ratio x those of |t32 - ref| (+ floor, relative to max|ref|)."""
    out, ref, t32 = (np.asarray(v.cpu() if torch.is_tensor(v) else v) for v in (out, ref, t32))
    out, ref, t32 = (np.asarray(v, dtype=np.complex128 if np.iscomplexobj(v) else np.float64) for v in (out, ref, t32))
    assert out.shape == ref.shape == t32.shape, (out.shape, ref.shape, t32.shape)
    assert np.isfinite(out).all()
    e, e32 = np.abs(out - ref), np.abs(t32 - ref)
    m, m32, r, r32 = e.max(), e32.max(), np.sqrt(np.mean(e * e)), np.sqrt(np.mean(e32 * e32))
    print(f"\n  {what} vs f64: HIP max {m:.2e} rms {r:.2e}; torch32 max {m32:.2e} rms {r32:.2e}")
    fl = FLOOR * np.abs(ref).max()
    assert m <= ratio * m32 + fl, (what, m, m32)
    assert r <= ratio * r32 + fl, (what, r, r32)


def audio_check(out, ref, t32, what, ratio=RATIO):
    """Per-audio relative L2 from f64: median and worst <= ratio x torch32's + 1e-7."""
    out = out.cpu().numpy() if torch.is_tensor(out) else out
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all()
    e, e32 = R.rel_l2(out, ref).ravel(), R.rel_l2(t32, ref).ravel()
    print(f"\n  {what}: rel L2 vs f64 HIP median {np.median(e):.2e} worst {e.max():.2e}; "
          f"torch32 median {np.median(e32):.2e} worst {e32.max():.2e}")
    assert np.median(e) <= ratio * np.median(e32) + FLOOR, (what, np.median(e), np.median(e32))
    assert e.max() <= ratio * e32.max() + FLOOR, (what, e.max(), e32.max())
    return e, e32


def _m2a(case="toy", plain=False, **kw):
    """Mel2AudioToy for the toy case, Mel2Audio for GTZAN -- or (plain) Mel2Audio at the toy geometry."""
    from drsa_audio_amd.xai.explain.audiogen import Mel2Audio, Mel2AudioToy
    return (Mel2AudioToy if case == "toy" and not plain else Mel2Audio)(case, device=DEV, **kw)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def toy():
    """B = 3 sources x 3 heatmaps at the toy geometry, shared (read-only) by the tests."""
    wavs = R.signals(3, 16000, seed=5)
    return {"wavs": wavs, "h": R.heatmaps(3, 3, 64, 64, seed=6), "habs": R.heatmaps(3, 3, 64, 64, seed=7, absolute=True)}


# ------------------------------------------------------------------ stage tests
@pytest.mark.parametrize("percentile", [None, 50, 90])
@pytest.mark.parametrize("absolute", [False, True])
def test_mask_kept_set_and_blur(toy, percentile, absolute):
    from drsa_audio_amd.xai.explain.audiogen import GaussianBlur, Mel2Audio
    h = (toy["habs"] if absolute else toy["h"])[1, 2]
    raw = Mel2Audio.generate_mask(_dev(h), GaussianBlur(1, 1.0), percentile).cpu().numpy()    # k = 1: no blur
    keep = R.kept(h, percentile) & (h > 0)
    assert np.array_equal(raw != 0, keep)
    assert np.array_equal(raw, np.where(keep, h, 0).astype(np.float32))
    if absolute and percentile:
        assert keep.sum() == round(h.size * (100 - percentile) / 100)    # the cut is inside the positive part
    out = Mel2Audio.generate_mask(_dev(h), GaussianBlur(5, 1.0), percentile)
    assert out.shape == (64, 64) and out.is_cuda
    anchored(out, R.mask(h, percentile, mode="f64"), R.mask(h, percentile, mode="torch32"), "mask")


def test_mask_odd_map_wide_kernel_and_ties():
    """41 x 61 map (not a multiple of anything), a 9-tap blur, and a map of a few distinct values
    (the radix select walks through buckets with many equal keys)."""
    from drsa_audio_amd.xai.explain.audiogen import GaussianBlur, Mel2Audio
    rng = np.random.default_rng(2)
    h = (np.round(rng.standard_normal((41, 61)) * 2) / 2).astype(np.float32)
    for p in (50, 90, 97.5):
        raw = Mel2Audio.generate_mask(_dev(h), GaussianBlur(1, 1.0), p).cpu().numpy()
        assert np.array_equal(raw != 0, R.kept(h, p) & (h > 0)), p
    out = Mel2Audio.generate_mask(_dev(h), GaussianBlur(9, 2.0), 90)
    anchored(out, R.mask(h, 90, 9, 2.0, "f64"), R.mask(h, 90, 9, 2.0, "torch32"), "mask 41x61 k=9")


@pytest.mark.parametrize("case", ["toy", "gtzan"])
def test_analysis_mel_and_spectrum(toy, case):
    g = R.GEOM[case]
    wavs = toy["wavs"] if case == "toy" else R.signals(2, 48000, seed=3)
    m = _m2a(case)
    mel, X = m._analyse(_dev(wavs), peak_norm=False)
    assert mel.shape == (len(wavs), g["n_mels"], g["width"]) and X.shape == (len(wavs), g["width"], g["n_fft"] // 2 + 1)
    mel64, X64 = R.analysis(wavs, g, "f64")
    mel32, X32 = R.analysis(wavs, g, "torch32")
    anchored(X.transpose(1, 2), X64, X32, f"{case} X")
    anchored(mel, mel64, mel32, f"{case} mel")
    # in-kernel peak normalisation = the analysis of wav / max|wav|
    meln, Xn = m._analyse(_dev(wavs), peak_norm=True)
    wn = wavs / np.abs(wavs).max(-1, keepdims=True)
    meln2, Xn2 = m._analyse(_dev(wn), peak_norm=False)
    assert torch.equal(meln, meln2) and torch.equal(Xn, Xn2)


def test_synthesis_same_inputs_both_sides(toy):
    """The same (float32) mel, X and masks go to the kernel and to the oracle's synthesis."""
    m = _m2a("toy")
    mel, X = m._analyse(_dev(toy["wavs"]), peak_norm=True)
    masks = torch.stack([torch.stack([m.generate_mask(_dev(h), m.smoother, 50) for h in hs]) for hs in toy["habs"]])
    out = m._synthesise(mel, X, masks)
    assert out.shape == (3, 3, 240 * 63)
    ref, t32 = (np.stack([R.synthesis(mel[b].cpu(), X[b].t().cpu(), masks[b].cpu(), TOY, mode).numpy()
                          for b in range(3)]) for mode in ("f64", "torch32"))
    audio_check(out, ref, t32, "toy synthesis")


# ------------------------------------------------------------------- end to end
@pytest.mark.parametrize("percentile", [None, 50, 90])
@pytest.mark.parametrize("absolute", [False, True])
def test_end_to_end_toy(toy, percentile, absolute):
    """make_audios_batch at the toy geometry (Mel2AudioToy: power 2, frames 1..64, peak-normalised
    audios), 3 sources x (1 standard + 2 concept) heatmaps.  The ratio used is RATIO = 2.  Measured
    on MI355X, relative L2 from f64 over the 9 audios, median / worst, over the six cases: HIP
    3.8e-7..5.2e-7 / 4.2e-7..7.0e-7, torch32 3.6e-7..5.1e-7 / 4.1e-7..6.6e-7 (largest ratio 1.17)."""
    h = toy["habs"] if absolute else toy["h"]
    out = _m2a("toy").make_audios_batch(_dev(h[:, 0]), _dev(h[:, 1:]), _dev(toy["wavs"]), percentile=percentile)
    assert out.shape == (3, 3, 15120)
    ref, t32 = (R.make_audios_batch(h[:, 0], h[:, 1:], toy["wavs"], TOY, percentile, mode=mode, volume_match=False)
                for mode in ("f64", "torch32"))
    audio_check(out, ref, t32, f"toy e2e p={percentile} abs={absolute}")
    assert float(out.abs().amax(-1).min()) == 1.0 == float(out.abs().max())


def test_end_to_end_toy_geometry_with_volume_matching(toy):
    """Mel2Audio (power 1, frames 0..63, adjust_vol against the waveform as passed in) at the toy
    geometry; the concept audios' RMS equals the source's where the clamp does not bite."""
    h, wavs = toy["habs"], toy["wavs"]
    g = dict(TOY, power=1, frame0=0)
    out = _m2a("toy", plain=True).make_audios_batch(_dev(h[:, 0]), _dev(h[:, 1:]), _dev(wavs), percentile=90)
    ref, t32 = (R.make_audios_batch(h[:, 0], h[:, 1:], wavs, g, 90, mode=mode) for mode in ("f64", "torch32"))
    audio_check(out, ref, t32, "toy geometry, Mel2Audio")
    o = out.cpu().numpy().astype(np.float64)
    rms, want = np.sqrt((o ** 2).mean(-1)), np.sqrt((wavs.astype(np.float64) ** 2).mean(-1))[:, None]
    free = np.abs(o).max(-1) < 1.0
    assert free.any() and np.abs(rms / want - 1)[free].max() <= 1e-5
    assert (rms <= want * (1 + 1e-5)).all() and np.abs(o).max() <= 1.0


def test_gtzan_shape():
    wavs = R.signals(2, 48000, seed=9)
    h = R.heatmaps(2, 2, 128, 128, seed=10, absolute=True)
    out = _m2a("gtzan").make_audios_batch(_dev(h[:, 0]), _dev(h[:, 1:]), _dev(wavs), percentile=90)
    assert out.shape == (2, 2, 45720)
    ref, t32 = (R.make_audios_batch(h[:, 0], h[:, 1:], wavs, GTZAN, 90, mode=mode) for mode in ("f64", "torch32"))
    audio_check(out, ref, t32, "gtzan e2e")


@pytest.mark.parametrize("n_fft,n_mels,width,hop,L", [(800, 41, 61, 361, 24007), (128, 20, 33, 48, 2000)])
def test_off_shape_power2(n_fft, n_mels, width, hop, L):
    """As test_n_fft_800_kernel_odd_shapes: n_fft 800 with an odd hop, 41 mels x 61 frames (no
    multiple of the 16-frame tile, of the MFMA's 4-row blocks or of 64 lanes), power 2.  And
    n_fft 128: n_fft/2 = 4*4*4 is an odd number of Stockham passes, so the transform ends in the
    other ping-pong buffer (the synthesis keeps its windowed frame in the free one); hop 48
    is no divisor of n_fft either."""
    from drsa_audio_amd.utils.dataloading import Loader
    from drsa_audio_amd.xai.explain.audiogen import Mel2Audio
    m = Mel2Audio(loader=Loader(None, sample_rate=16000, n_fft=n_fft, hop_length=hop, n_mels=n_mels, slice_length=0,
                                width=width, device=DEV), power=2)
    g = dict(sr=16000, n_fft=n_fft, hop=hop, n_mels=n_mels, width=width, power=2, frame0=0)
    wavs = R.signals(3, L, seed=n_mels)
    h = R.heatmaps(3, 2, n_mels, width, seed=width, absolute=True)
    out = m.make_audios_batch(_dev(h[:, 0]), _dev(h[:, 1:]), _dev(wavs), percentile=50)
    assert out.shape == (3, 2, hop * (width - 1))
    ref, t32 = (R.make_audios_batch(h[:, 0], h[:, 1:], wavs, g, 50, mode=mode) for mode in ("f64", "torch32"))
    audio_check(out, ref, t32, f"n_fft {n_fft} hop {hop} {n_mels}x{width} power 2")


# ------------------------------------------------------------------ properties
def test_batch_independence_large_batch():
    wavs = R.signals(24, 16000, seed=21)
    h = R.heatmaps(24, 3, 64, 64, seed=22, absolute=True)
    m = _m2a("toy", plain=True)
    big = m.make_audios_batch(_dev(h[:, 0]), _dev(h[:, 1:]), _dev(wavs), percentile=90)
    for i in (0, 13, 23):
        one = m.make_audios_batch(_dev(h[i:i + 1, 0]), _dev(h[i:i + 1, 1:]), _dev(wavs[i:i + 1]), percentile=90)
        assert torch.equal(big[i:i + 1], one)


def test_silent_mask_gives_nan_audio_and_leaves_the_rest(toy):
    h = toy["habs"].copy()
    h[1, 2] = -np.abs(h[1, 2])                          # all non-positive (one exact zero too)
    h[1, 2, 0, 0] = 0.0
    m = _m2a("toy")
    out = m.make_audios_batch(_dev(h[:, 0]), _dev(h[:, 1:]), _dev(toy["wavs"]), percentile=90)
    base = m.make_audios_batch(_dev(toy["habs"][:, 0]), _dev(toy["habs"][:, 1:]), _dev(toy["wavs"]), percentile=90)
    assert torch.isnan(out[1, 2]).all()
    keep = torch.ones(3, 3, dtype=torch.bool)
    keep[1, 2] = False
    assert torch.equal(out[keep], base[keep])


def test_identity_mask_round_trip(toy):
    """All-ones heatmap, no percentile, no blur (k = 1): the audio is the mel round trip of the
    chunk.  Its distance from the (peak-normalised) chunk over the valid span is not zero -- the
    mel projection loses information -- and must equal the f64 oracle's own round-trip distance
    within the anchored ratio."""
    wavs = toy["wavs"]
    g = dict(TOY, power=1, frame0=0)
    m = _m2a("toy", plain=True, blur_kernel=1)
    mel, X = m._analyse(_dev(wavs), peak_norm=True)
    out = m._synthesise(mel, X, torch.ones(3, 1, 64, 64, device=DEV))[:, 0].cpu().numpy()
    full = (wavs / np.abs(wavs).max(-1, keepdims=True)).astype(np.float64)
    wn = full[:, :out.shape[-1]]                        # the valid span of the chunk
    ones = torch.ones(1, 64, 64)
    rt = {}
    for mode in ("f64", "torch32"):
        mel_r, X_r = R.analysis(full if mode == "f64" else full.astype(np.float32), g, mode)
        rt[mode] = np.stack([R.synthesis(mel_r[b], X_r[b], ones, g, mode)[0].numpy() for b in range(3)])
    d, d64, d32 = (R.rel_l2(v, wn) for v in (out, rt["f64"], rt["torch32"]))
    print(f"\n  round-trip distance from the chunk: HIP {d}, f64 {d64}")
    assert (d64 > 1e-3).all()                           # the projection does lose information
    # a result e away from the oracle's moves the distance by at most |e| / |chunk| (triangle inequality)
    moved32 = np.sqrt(((rt["torch32"] - rt["f64"]) ** 2).sum(-1)) / np.sqrt((wn ** 2).sum(-1))
    assert (np.abs(d - d64) <= RATIO * moved32 + FLOOR).all(), (d, d64, moved32)
    audio_check(out, rt["f64"], rt["torch32"], "identity round trip")


# ----------------------------------------------------------- reference interface
def test_make_audios_on_heatmap_generator_info():
    """The small GTZAN-128 net of test_logmel_gpu.test_feeds_the_explainer_end_to_end: songs ->
    log-mel -> HeatmapGenerator.info -> make_audios (K + 1 audios of one chunk)."""
    import logmel_ref as L
    from drsa_audio_amd.model.create_model import VGGType
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN
    from drsa_audio_amd.utils.dataloading import Loader
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
    torch.manual_seed(0)
    net = VGGType(n_filters=(32, 32, 64, 64, 128), n_dense=128, pool_kernels=((2, 2),) * 5, dropout=0.4,
                  input_size=(128, 128), conv_bn=False, dense_bn=False, block_depth=1).eval().to(DEV)
    U = torch.from_numpy(np.linalg.qr(np.random.default_rng(0).standard_normal((64, 64)))[0].astype(np.float32))
    songs = L.synthetic_songs(1, seed=1)
    x = Loader("gtzan", device=DEV).load_songs(torch.from_numpy(songs).to(DEV))
    hg = HeatmapGenerator(net, U, LRP_NAME_MAP_GTZAN, "blues", num_concepts=4, layer_idx=7, device=DEV)
    hg.generate_subspace_heatmaps(x)
    chunk = 0.3 * L.get_slice(songs, 3, 0, 8, 16000)[2, 0]                  # un-normalised original of chunk 2
    m = _m2a("gtzan")
    audios = m.make_audios(hg.info, chunk, num_concepts=4, percentile=50, sample_idx=2)
    assert len(audios) == 5
    rms0 = float(np.sqrt((chunk.astype(np.float64) ** 2).mean()))
    for a in audios:
        assert a.shape == (45720,) and a.is_cuda and torch.isfinite(a).all()
        if float(a.abs().max()) < 1.0:
            assert abs(float(a.double().pow(2).mean().sqrt()) / rms0 - 1) <= 1e-5
    one = {"standard_heatmap": hg.info["standard_heatmaps"][2], "subspace_heatmaps": hg.info["subspace_heatmaps"][2]}
    again = m.make_audios(one, torch.from_numpy(chunk), num_concepts=4, percentile=50)
    assert all(torch.equal(a, b) for a, b in zip(audios, again))
    batch = m.make_audios_batch({k: v[2:3] for k, v in hg.info.items() if k.endswith("heatmaps")}, wavs=chunk[None])
    assert torch.equal(batch[0], torch.stack(audios))


def test_transform_and_transform_audio_match_the_batch_path(toy):
    m = _m2a("toy", plain=True)
    wn = toy["wavs"][0] / np.abs(toy["wavs"][0]).max()
    mel, phase = m.transform_audio(wn)
    assert mel.shape == (64, 64) and phase.shape == (241, 64) and phase.is_complex() and mel.is_cuda
    assert float((phase.abs() - 1).abs().max()) <= 1e-6
    a = m.transform(toy["habs"][0, 1], mel, phase, percentile=90)
    assert a.shape == (15120,)
    ref = R.make_audios_batch(toy["habs"][:1, 0], toy["habs"][:1, 1:2], toy["wavs"][:1], dict(TOY, power=1, frame0=0),
                              90, mode="f64", normalise=False)[0, 1]
    assert R.rel_l2(a.cpu().numpy(), ref) <= 1e-5


def test_transform_wav_return_all():
    from drsa_audio_amd.utils.dataloading import Loader
    ld = Loader("toy", device=DEV)
    wavs = R.signals(2, 16000, seed=4)
    wavs[1, :] = 0.0                                    # a silent chunk: |X| = 0, phase 1 + 0i
    w = _dev(wavs).reshape(2, 1, 16000)
    wav, mag, phase, mel = ld.transform_wav(w, return_all=True)
    assert wav.shape == (2, 1, 16000) and mag.shape == (2, 1, 241, 64) == phase.shape and mel.shape == (2, 1, 64, 64)
    assert all(t.is_cuda for t in (wav, mag, phase, mel)) and phase.is_complex() and not mag.is_complex()
    g = dict(TOY, power=1, frame0=0)
    mel64, X64 = R.analysis(wavs, g, "f64")
    mel32, X32 = R.analysis(wavs, g, "torch32")
    anchored((mag * phase)[:, 0], X64, X32, "mag * phase")
    anchored(mel[:, 0], mel64, mel32, "return_all mel")
    assert torch.equal(phase[1], torch.ones_like(phase[1])) and float(mag[1].abs().max()) == 0.0
    # the log-mel path is frames 1..width of the same transform: one hop later than return_all's
    logmel = ld.transform_wav(w[:1], clamp=False)
    lin = 10.0 ** logmel[0, 0].double() - 1e-7
    assert torch.allclose(lin[:, :-1], mel[0, 0, :, 1:].double(), rtol=1e-4, atol=1e-7)


def test_file_entry_points_match_the_in_memory_ones(tmp_path, toy):
    """transform_audio_from_file / make_audios(path_to_sample=...) read a 16-bit WAV with the stdlib
    reader and slice it like get_slice: the same results as passing that slice."""
    import wave
    pcm = np.round(R.signals(1, 3 * 16000, seed=8)[0] * 32767).astype("<i2")
    path = str(tmp_path / "song.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    chunk = pcm[16000:32000].astype(np.float32) / 32768.0          # second 1..2 (toy slice_length = 1 s)
    m = _m2a("toy", plain=True)
    mel, ph = m.transform_audio_from_file(path, startpoint=1)
    mel2, ph2 = m.transform_audio(chunk)
    assert torch.equal(mel, mel2) and torch.equal(ph, ph2)
    info = {"standard_heatmap": toy["habs"][0, 0], "subspace_heatmaps": toy["habs"][0, 1:]}
    a = m.make_audios(info, None, startpoint=1, num_concepts=2, percentile=90, path_to_sample=path)
    b = m.make_audios(info, chunk, num_concepts=2, percentile=90)
    assert len(a) == len(b) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        m.make_audios(info, None)
