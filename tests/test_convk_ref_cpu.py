"""tests/convk_ref.py checks itself, without a GPU: at 3x3 it is the oracle's pinned-order primitives
bit for bit, a zero-embedded 3x3 kernel keeps those bits at every larger size, and at asymmetric
sizes it agrees with float64 torch (which tells a kh / kw transposition or a missing tap flip from
the right answer)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import convk_ref as K
import lrp_ref

_M = nn.Conv2d(1, 1, 3, padding=1)


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, 6, 8, generator=g)
    x[0, :, 2:4, 3:6] = 0.0
    gr = torch.randn(2, 7, 6, 8, generator=g)
    w = torch.randn(7, 5, 3, 3, generator=g) / 45 ** 0.5
    b = torch.randn(7, generator=g) * 0.1
    return x, gr, w, b


def test_3x3_is_the_oracle(data):
    x, gr, w, b = data
    assert torch.equal(K.conv(x, w, b), lrp_ref.ExactOps.conv(_M, x, w, b))
    assert torch.equal(K.conv(x, w), lrp_ref.ExactOps.conv(_M, x, w, None))
    assert torch.equal(K.conv_t(gr, w), lrp_ref.ExactOps.conv_t(_M, None, w, gr))


@pytest.mark.parametrize("kh,kw", [(5, 5), (7, 7), (3, 5), (5, 3)])
def test_zero_embedded_3x3_keeps_its_bits(data, kh, kw):
    x, gr, w, b = data          # finite inputs: NaN * 0 would differ
    big = torch.zeros(7, 5, kh, kw)
    big[:, :, (kh - 3) // 2:(kh + 3) // 2, (kw - 3) // 2:(kw + 3) // 2] = w
    assert torch.equal(K.conv(x, big, b), K.conv(x, w, b))
    assert torch.equal(K.conv_t(gr, big), K.conv_t(gr, w))


@pytest.mark.parametrize("kh,kw", [(5, 3), (3, 5)])
def test_asymmetric_kernels_against_float64(data, kh, kw):
    x, gr, _, b = data
    w = torch.randn(7, 5, kh, kw, generator=torch.Generator().manual_seed(kh * 10 + kw)) / (5 * kh * kw) ** 0.5
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=pad)
    assert float((K.conv(x, w, b).double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    ref_t = torch.nn.grad.conv2d_input(x.double().shape, w.double(), gr.double(), padding=pad)
    assert float((K.conv_t(gr, w).double() - ref_t).abs().max()) <= 1e-5 * float(ref_t.abs().max())


def test_case_lists_cover_the_axes():
    """Every kernel size meets every map, every channel pair and every ng; the backward list every xmode x post
    and both clone counts."""
    for cases, ngs in ((K.fwd_cases(), {1, 2, 3}), (K.bwd_cases(), {1, 2})):
        for k in K.KERNELS:
            mine = [c for c in cases if c[:2] == k]
            assert {c[2:4] for c in mine} == set(K.PAIRS) and {c[4:6] for c in mine} == set(K.MAPS)
            assert {c[6][0] for c in mine} == ngs
    modes = {m[1:] for *_, m in K.bwd_cases()}
    assert {(xm, po) for xm, po, _ in modes} == {(xm, po) for xm in range(3) for po in range(3)}
    assert {cl for _, _, cl in modes} == {1, 3}


def test_packers_place_the_taps():
    """Row k = (ci * kh + ky) * kw + kx forward, the flipped tap backward, zero padding to (2, 32)."""
    w = torch.arange(3 * 5 * 3 * 5, dtype=torch.float32).reshape(3, 5, 3, 5) + 1
    f, b = K._convk_fwd_layout([w, 2 * w]), K._convk_bwd_layout([w])
    assert f.shape == (2, 6 * 15, 32) and b.shape == (1, 4 * 15, 32)
    assert f[1, (4 * 3 + 2) * 5 + 1, 2] == 2 * w[2, 4, 2, 1] and float(f[:, 5 * 15:].abs().max()) == 0 and float(f[:, :, 3:].abs().max()) == 0
    assert b[0, (2 * 3 + 0) * 5 + 1, 4] == w[2, 4, 2, 3] and float(b[:, 3 * 15:].abs().max()) == 0 and float(b[:, :, 5:].abs().max()) == 0
