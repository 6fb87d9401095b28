"""drsa_amd_projection_bwd, recompute path with the batched relevance gather and compile-time
pool / den flags, against the stored-buffer kernel (untouched, one tile per workgroup), bitwise, on
what the restructuring can break:

* tile counts per workgroup: the recompute kernel walks two tiles per workgroup, so maps of one tile
  (8 x 8), two tiles (4 x 32) and three tiles (6 x 32: the last workgroup holds a single tile) catch
  state carried from one tile of a workgroup to the next;
* the argmax select after the reordered loads: argmax constant at each of 0, 1, 2, 3 and random,
  relevance with +0.0, -0.0 and negative entries;
* zeros and signs: a with exact zeros (ReLU output, one channel dead everywhere), negative a',
  den of both signs;
* every tile holds different (random) data, and every output starts NaN-poisoned.

Every case runs {den, no den} x fan-out {0, 1, 2}; d = 16 / 64 run the unpadded register path,
d = 100 the zero-padded one in the 128-wide kernel."""
import functools

import numpy as np
import pytest
import torch

from drsa_audio_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, K = 2, 4
MAPS = [(8, 8), (4, 32), (6, 32)]          # 1, 2 and 3 tiles of 64 pixels
RELEVANCE = ["dense", "amax0", "amax1", "amax2", "amax3", "amax_random"]


@functools.lru_cache(maxsize=None)
def _case(D, H, W):
    """Inputs shared by every test of one (d, map): built once and never written afterwards."""
    g = torch.Generator().manual_seed(1000 * D + 10 * H + W)
    a = torch.randn(B, D, H, W, generator=g).clamp_min(0)
    a[:, 1] = 0                                       # a dead ReLU channel
    a = a.to(DEV)
    U = torch.from_numpy(np.linalg.qr(np.random.default_rng(D).standard_normal((D, D)))[0].astype(np.float32)).to(DEV)
    s = _capi.stream_ptr(DEV)
    P = torch.empty_like(U)
    _capi.call("drsa_amd_projection_residual", U.data_ptr(), D, P.data_ptr(), s)
    h = torch.empty(B, D, H, W, device=DEV)
    ap = torch.empty(B, D, H, W, device=DEV)
    _capi.call("drsa_amd_projection_fwd", a.data_ptr(), U.data_ptr(), P.data_ptr(), h.data_ptr(), ap.data_ptr(),
               None, None, B, D, H, W, 0, s)
    den = (torch.randn(B, D, H, W, generator=g) * 2).to(DEV)

    def relevance(*shape):
        r = torch.randn(*shape, generator=g)
        flat = r.view(-1)
        flat[0::7] = 0.0
        flat[3::7] = -0.0
        return r.to(DEV)

    gp = {"dense": relevance(B, D, H, W), "pooled": relevance(B, D, H // 2, W // 2)}
    amax = {f"amax{v}": torch.full((B, D, H // 2, W // 2), v, dtype=torch.uint8, device=DEV) for v in range(4)}
    amax["amax_random"] = torch.randint(0, 4, (B, D, H // 2, W // 2), generator=g, dtype=torch.uint8).to(DEV)
    torch.cuda.synchronize()
    assert (a == 0).any() and (ap < 0).any() and (den < 0).any() and (den > 0).any()
    for r in gp.values():
        assert (r < 0).any() and ((r == 0) & torch.signbit(r)).any() and ((r == 0) & ~torch.signbit(r)).any()
    return dict(a=a, U=U, P=P, h=h, ap=ap, den=den, gp=gp, amax=amax)


@pytest.mark.parametrize("relevance", RELEVANCE)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("D", [16, 64, 100])
def test_batched_gather_equals_stored(D, H, W, relevance):
    c = _case(D, H, W)
    s = _capi.stream_ptr(DEV)
    gp = c["gp"]["dense" if relevance == "dense" else "pooled"]
    amax = None if relevance == "dense" else c["amax"][relevance]
    for has_den in (True, False):
        den = c["den"] if has_den else None
        for fanout in (0, 1, 2):
            nq = K + 1 if fanout == 1 else K if fanout == 2 else 1
            outs = []
            for stored in (True, False):
                G = torch.full((B * nq, D, H, W), float("nan"), device=DEV)
                _capi.call("drsa_amd_projection_bwd", gp.data_ptr(), _capi.ptr(amax),
                           c["ap"].data_ptr() if stored else None, c["h"].data_ptr() if stored else None,
                           c["a"].data_ptr(), _capi.ptr(den), c["U"].data_ptr(), c["P"].data_ptr(), G.data_ptr(),
                           B, D, H, W, K, 1e-6, 1e-7, fanout, s)
                outs.append(G)
            torch.cuda.synchronize()
            what = f"den={has_den} fanout={fanout}"
            assert not torch.isnan(outs[0]).any(), what
            assert not torch.isnan(outs[1]).any(), what
            # bit for bit, the sign of zero included
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), what
            # the dead channel stays dead ([a > 0] select) in every clone
            assert (outs[1][:, 1] == 0).all(), what
