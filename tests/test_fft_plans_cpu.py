"""The case tables of tests/fft_plan_cases.py reach what they claim, and its numpy model of the
Stockham passes, the real-input split and the inverse packing (the formulas of csrc/stockham.h,
csrc/logmel.hip and csrc/audiogen.hip) is a DFT.  CPU only; the kernels run in
tests/test_fft_plans_gpu.py."""
import numpy as np
import pytest

import audiogen_ref as R
import fft_plan_cases as P


def test_radices_match_the_table():
    for n_fft, passes, *_ in P.PLANS:
        assert P.radices(n_fft // 2) == list(passes), n_fft
        assert int(np.prod(passes)) == n_fft // 2
    assert P.radices(7) is None and P.radices(4 ** 9) is None          # a prime factor > 5; more than 8 stages
    assert P.radices(240) == [4, 4, 3, 5] and P.radices(400) == [4, 4, 5, 5]   # the plans of the older tests


def test_table_reaches_every_pass_kind():
    shapes = {n_fft: P.pass_shapes(n_fft // 2, passes) for n_fft, passes, *_ in P.PLANS}
    first = {s[0][0] for s in shapes.values()}
    later = {R_ for s in shapes.values() for R_, Ns, _ in s if Ns > 1}
    assert {2, 3, 5} <= first
    assert later == {2, 3, 4, 5}
    counts = {len(s) for s in shapes.values()}
    assert any(c % 2 for c in counts) and any(c % 2 == 0 for c in counts)
    assert 5 in counts and 1 in counts
    Ms = {n_fft // 2 for n_fft in shapes}
    assert any(M % 2 for M in Ms) and any(M < 64 for M in Ms)
    assert any(MR % 64 and MR > 64 for s in shapes.values() for _, _, MR in s)      # a partly masked last trip
    assert any(MR == 64 for s in shapes.values() for _, _, MR in s)
    assert any(MR > 128 and R_ == 2 for s in shapes.values() for R_, _, MR in s)    # radix 2, several trips per lane
    assert any(sum(1 for R_, Ns, _ in s if R_ == 3 and Ns > 1) >= 2 for s in shapes.values())
    assert any(sum(1 for R_, Ns, _ in s if R_ == 5 and Ns > 1) >= 2 for s in shapes.values())
    assert any({R_ for R_, _, _ in s} == {2, 3, 4, 5} for s in shapes.values())


def test_table_geometry():
    rows = [(n_fft, hop, width, power, rem) for n_fft, _, hop, _, width, power, rem, _ in P.PLANS]
    assert any(n_fft % hop == 0 for n_fft, hop, *_ in rows) and any(n_fft % hop for n_fft, hop, *_ in rows)
    assert any(hop % 2 for _, hop, *_ in rows)
    assert sum(2 * hop > n_fft for n_fft, hop, *_ in rows) >= 2
    assert all(width % 8 for _, _, width, *_ in rows)
    assert any(width < 8 for _, _, width, *_ in rows) and any(width > 16 for _, _, width, *_ in rows)
    assert [power for *_, power, _ in rows] == [1, 2] * (len(rows) // 2)
    assert 2 * sum(rem != 0 for *_, rem in rows) >= len(rows)
    for n_fft, hop, width, _, rem in rows:
        assert 0 <= rem < hop
        for frame0 in (0, 1):           # the analysis starts at frame 0, the log-mel at frame 1
            L = P.chunk_len(hop, width, rem, frame0)
            assert L // hop == frame0 + width - 1 and L % hop == rem and L > n_fft // 2


@pytest.mark.parametrize("row", P.PLANS, ids=P.PLAN_IDS)
def test_model_is_rfft_and_irfft(row):
    n_fft, passes = row[0], row[1]
    rng = np.random.default_rng(n_fft)
    x = rng.uniform(-1, 1, (4, n_fft))
    X = np.fft.rfft(x, axis=-1)
    got = P.rfft_model(x, passes)
    assert np.abs(got - X).max() <= 1e-12 * np.abs(X).max()
    Y = rng.standard_normal((4, n_fft // 2 + 1)) + 1j * rng.standard_normal((4, n_fft // 2 + 1))
    y = np.fft.irfft(Y, n=n_fft, axis=-1)
    assert np.abs(P.irfft_model(Y, passes) - y).max() <= 1e-12 * np.abs(y).max()
    z = rng.standard_normal((2, n_fft // 2)) + 1j * rng.standard_normal((2, n_fft // 2))
    Z = np.fft.fft(z, axis=-1)
    assert np.abs(P.stockham_model(z, passes) - Z).max() <= 1e-12 * np.abs(Z).max()


def test_filterbanks_are_well_conditioned():
    """No empty filter and a singular-value ratio <= 1e3 for every (n_fft, n_mels) of the tables:
    P = pinv(fb^T) amplifies both float32 chains' rounding by up to that ratio."""
    pairs = {(p[0], p[3]) for p in P.PLANS} | {(o[0], o[2]) for o in P.OVERLAPS}
    for n_fft, n_mels in sorted(pairs):
        fb = R.filterbank(n_fft, n_mels, P.SR).astype(np.float64)
        assert (fb.max(0) > 0).all(), (n_fft, n_mels)
        s = np.linalg.svd(fb, compute_uv=False)
        assert s[0] / s[-1] <= 1e3, (n_fft, n_mels, s[0] / s[-1])


def test_overlaps_cover_every_depth():
    geo = [P.overlap_geometry(n_fft, hop, width) for n_fft, hop, _, width, _ in P.OVERLAPS]
    assert {e for e, *_ in geo} == {1, 2, 3, 4, 7, 8}
    assert all(e + G == P.TILE and 0 < e <= P.TILE // 2 for e, G, _, _ in geo)
    for (n_fft, hop, n_mels, width, power), (extra, G, nspan, partial) in zip(P.OVERLAPS, geo):
        assert hop <= n_fft and power in (1, 2)
        assert nspan == 1 or (nspan >= 3 and partial), (n_fft, hop, width, nspan)
    for e in (1, 2, 3, 4, 7, 8):
        assert any(g[0] == e and g[2] >= 3 and g[3] for g in geo), e              # each depth over several spans
    assert any(width == 2 for _, _, _, width, _ in P.OVERLAPS)
    assert any(hop * 4 == n_fft for n_fft, hop, *_ in P.OVERLAPS)
    assert any((n_fft // 2) % 2 for n_fft, *_ in P.OVERLAPS)
