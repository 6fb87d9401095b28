"""The projection kernels (csrc/projection.hip) against the float64 oracle of proj_ref.py, at kernel
level: the residual P, the forward's h, a', pooled a' and argmax, the pool's tie rule, and every
output row of the backward for fanout 0, 1 and 2 in stored and recompute mode.  Bounds: the project's
kernel gate (2e-5 of the sum of |terms| per GEMM) and explicit fp32 roundings, carried
through the chain as proj_ref's docstring derives.  d = 32 runs the unpadded <32, false> kernels (the
register-operand forward at NB = 2), d = 5 / 24 / 33 / 100 the padded embeddings; the maps cover the
three tile shapes and a last forward workgroup that holds fewer than its four tiles behind a full one.
Each test prints its worst error-to-bound ratio before it asserts."""
import numpy as np
import pytest
import torch

import proj_ref as R
from drsa_audio_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAN = float("nan")
EPS_PROJ, EPS_DEN = 1e-6, 1e-7


def _ortho(d, seed):
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0]
    return torch.from_numpy(q.astype(np.float32)).to(DEV)


def _residual(U):
    P = torch.full_like(U, NAN)
    _capi.call("drsa_amd_projection_residual", U.data_ptr(), U.shape[0], P.data_ptr(), _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return P


def _forward(a, U, P, pool, with_h=True, with_ap=True):
    """(h, a', pooled, argmax), every output pre-filled with NaN / 255."""
    B, D, H, W = a.shape
    h = torch.full((B, D, H, W), NAN, device=DEV) if with_h else None
    ap = torch.full((B, D, H, W), NAN, device=DEV) if with_ap else None
    pooled = torch.full((B, D, H // 2, W // 2), NAN, device=DEV) if pool else None
    amax = torch.full((B, D, H // 2, W // 2), 255, dtype=torch.uint8, device=DEV) if pool else None
    _capi.call("drsa_amd_projection_fwd", a.data_ptr(), U.data_ptr(), P.data_ptr(), _capi.ptr(h), _capi.ptr(ap),
               _capi.ptr(pooled), _capi.ptr(amax), B, D, H, W, pool, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return h, ap, pooled, amax


# ------------------------------------------------------------------------------------------ residual
@pytest.mark.parametrize("D", [1, 5, 16, 32, 100, 128])
def test_residual_against_float64(D):
    U = _ortho(D, 40 + D)
    P, P64 = _residual(U), R.residual(U)
    err = (P.double() - P64).abs()
    ratio = R.worst_ratio(err, R.residual_bound(U, P64))
    print(f"D={D} residual: max err / bound = {ratio:.3f}")
    assert torch.equal(P, P.T)
    assert ratio <= 1.0
    # U U^T = I exactly: the identity and a signed permutation
    assert torch.count_nonzero(_residual(torch.eye(D, device=DEV))) == 0
    g = torch.Generator().manual_seed(D)
    S = torch.zeros(D, D)
    S[torch.arange(D), torch.randperm(D, generator=g)] = torch.randint(0, 2, (D,), generator=g).float() * 2 - 1
    assert torch.count_nonzero(_residual(S.to(DEV))) == 0


# ------------------------------------------------------------------------------------------- forward
# (8, 8): one 8 x 8 tile; (40, 16): ten 4 x 16 tiles, the last forward workgroup holds two;
# (6, 64): six 2 x 32 tiles, two per row pair; (18, 32): nine, the last workgroup holds one
MAPS = [(8, 8), (40, 16), (6, 64), (18, 32)]


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("D", [32, 16, 64, 128, 5, 24, 33, 100])
def test_forward_against_float64(D, H, W):
    B = 2
    g = torch.Generator().manual_seed(1000 * D + H + W)
    a = torch.randn(B, D, H, W, generator=g).clamp_min(0).to(DEV)        # about half the channels dead
    U = _ortho(D, D + 1)
    P, P64 = _residual(U), R.residual(U)
    h64, ap64, _, _ = R.forward(a, U, pool=False)
    hb, apb = R.h_bound(a, U), R.ap_bound(a, P64, ap64)
    first = None
    for pool in (0, 1):
        for with_h in (True, False):
            h, ap, pooled, amax = _forward(a, U, P, pool, with_h)
            rh = R.worst_ratio((h.double() - h64).abs(), hb) if with_h else 0.0
            rap = R.worst_ratio((ap.double() - ap64).abs(), apb)
            print(f"D={D} {H}x{W} pool={pool} h={int(with_h)}: h err / bound = {rh:.3e}, a' err / bound = {rap:.3e}")
            assert not torch.isnan(ap).any() and (not with_h or not torch.isnan(h).any())
            assert rh <= 1.0 and rap <= 1.0
            if first is None:
                first = (h, ap)
            assert torch.equal(ap, first[1]) and (not with_h or torch.equal(h, first[0]))
            if pool:
                po, ao = R.max_pool(ap)                                   # over the kernel's own a'
                assert not torch.isnan(pooled).any() and (amax < 4).all()
                assert torch.equal(pooled, po) and torch.equal(amax, ao)
                if not with_h:   # the plan's call: neither h nor a' stored
                    _, _, p2, a2 = _forward(a, U, P, 1, False, False)
                    assert torch.equal(p2, pooled) and torch.equal(a2, amax)


def test_pool_ties_and_nan():
    a, want = R.tie_map()
    a, want = a.to(DEV), want.to(DEV)
    D = a.shape[1]
    U = torch.eye(D, device=DEV)
    P = _residual(U)
    for with_h in (True, False):
        h, ap, pooled, amax = _forward(a, U, P, 1, with_h)
        assert torch.equal(ap, a) and (not with_h or torch.equal(h, a))   # U = I: a' = a exactly
        po, ao = R.max_pool(a)
        assert torch.equal(pooled, po) and torch.equal(amax, ao)
        assert torch.equal(amax.long()[want >= 0], want[want >= 0])     # ties and zeros: the lowest code
    # one NaN: 0 * NaN = NaN in the residual GEMM, so the pixel is NaN in every channel; which NaN of a
    # window wins differs between PyTorch and this kernel and nothing downstream depends on it
    an = a.clone()
    an[0, 9, 2, 5] = NAN
    _, ap, pooled, amax = _forward(an, U, P, 1, False)
    nanpix = torch.isnan(ap)
    assert nanpix[0, :, 2, 5].all() and nanpix.sum() == D
    assert torch.isnan(pooled[0, :, 1, 2]).all()
    code = amax[0, :, 1, 2].long()
    assert torch.isnan(ap[0, torch.arange(D), 2 + code // 2, 4 + code % 2]).all()
    keep = torch.ones_like(pooled, dtype=torch.bool)
    keep[0, :, 1, 2] = False
    po, ao = R.max_pool(a)
    assert torch.equal(pooled[keep], po[keep]) and torch.equal(amax[keep], ao[keep])


# ------------------------------------------------------------------------------------------ backward
def _backward(gp, amax, ap, h, a, den, U, P, K, fanout):
    B, D, H, W = a.shape
    nq = K + 1 if fanout == 1 else K if fanout == 2 else 1
    G = torch.full((B * nq, D, H, W), NAN, device=DEV)
    _capi.call("drsa_amd_projection_bwd", gp.data_ptr(), _capi.ptr(amax), _capi.ptr(ap), _capi.ptr(h), a.data_ptr(),
               _capi.ptr(den), U.data_ptr(), P.data_ptr(), G.data_ptr(), B, D, H, W, K, EPS_PROJ, EPS_DEN, fanout,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return G


# d_k = 8, 16, 4, 16, 8, 8, 25, 1, 5: the generic clone loop, its d_k = 16 form, partial 4-column steps
@pytest.mark.parametrize("H,W", [(16, 16), (6, 64)])
@pytest.mark.parametrize("fanout", [0, 1, 2])
@pytest.mark.parametrize("D,K", [(32, 4), (32, 2), (16, 4), (64, 4), (128, 16), (24, 3), (100, 4), (5, 5), (5, 1)])
def test_backward_every_row_against_float64(D, K, fanout, H, W):
    B = K + 2 if fanout == 0 else 2          # fanout 0: every clone index and one wrap-around
    g = torch.Generator().manual_seed(100 * D + 10 * K + fanout + H)
    a = torch.randn(B, D, H, W, generator=g).clamp_min(0).to(DEV)
    U = _ortho(D, D + K)
    P = _residual(U)
    den_full = torch.randn(B, D, H, W, generator=g) * 2                  # signed, a few exact zeros
    den_full.view(-1)[torch.randint(0, den_full.numel(), (32,), generator=g)] = 0.0
    den_full = den_full.to(DEV)
    h, ap, _, amax_p = _forward(a, U, P, 1)
    dead = (a == 0).repeat_interleave(K + 1 if fanout == 1 else K if fanout == 2 else 1, 0)
    for pool in (0, 1):
        amax = amax_p if pool else None
        gp = torch.randn(*((B, D, H // 2, W // 2) if pool else (B, D, H, W)), generator=g).to(DEV)
        for den in (den_full, None):
            Gs = _backward(gp, amax, ap, h, a, den, U, P, K, fanout)
            Gr = _backward(gp, amax, None, None, a, den, U, P, K, fanout)
            G64, E = R.backward(gp, amax, ap, h, a, den, U, K, EPS_PROJ, EPS_DEN, fanout)
            assert Gs.shape == G64.shape
            ratio = R.worst_ratio((Gs.double() - G64).abs(), E)
            print(f"D={D} K={K} fanout={fanout} {H}x{W} pool={pool} den={int(den is not None)}: "
                  f"max err / bound = {ratio:.3e}")
            assert not torch.isnan(Gs).any() and not torch.isnan(Gr).any()
            assert ratio <= 1.0
            assert torch.count_nonzero(Gs[dead]) == 0
            assert torch.equal(Gs, Gr)                                   # recompute == stored, bitwise
