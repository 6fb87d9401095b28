"""drsa_amd_avgpool_fwd / drsa_amd_avgpool_bwd on the GPU, through _capi: every element equal to the
restatement in tests/avgpool_ref.py (fp32, one rounding per operation, the header's order).

B = 3, C = 5, clones 1 and 3 (rows sample * clones + clone).  Maps and pools: 8 x 16 with (2,2), (2,4), (4,4)
and the global (8,16); 4 x 12 with (2,3), where a float4 of g straddles two windows; 16 x 32 with (16,32), 512
elements (past the max-pool's argmax byte); 8 x 8 with (1,2).  Every case runs the denominator as none, per
sample and shared map, the pool rule none and Epsilon, rel_full on and off.  The activation has whole dead
windows (y = 0: the stabiliser's [t == 0] branch) and dead pixels inside live windows, R_y both signs, den both
signs with exact zeros; 3 * 5 * 8 * 16 = 1920 elements is no multiple of 1024, so the last block is partial."""
import pytest
import torch
import torch.nn.functional as F

import avgpool_ref as A
from conv_ref import _seed
from drsa_audio_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, C = 3, 5
SHAPES = [(8, 16, 2, 2), (8, 16, 2, 4), (8, 16, 4, 4), (8, 16, 8, 16), (4, 12, 2, 3), (16, 32, 16, 32), (8, 8, 1, 2)]
EPS_POOL, EPS_CONV = 1e-6, 1e-7


def inputs(H, W, ph, pw, clones):
    g = torch.Generator().manual_seed(_seed(H, W, ph, pw, clones))
    ho, wo = H // ph, W // pw
    a = torch.randn(B, C, H, W, generator=g).clamp(min=0) * 2       # about half the pixels dead
    live = torch.rand(B, C, ho, wo, generator=g) >= 0.25            # a quarter of the windows all dead
    live[0, 0, 0, 0], live[1, 1, -1, -1], live[2, 2, 0, -1] = False, True, False
    a = a * A.spread(live.float(), ph, pw)
    a[1, 1, -1, -1] = 0.75                                          # that window stays live
    R_y = torch.randn(B * clones, C, ho, wo, generator=g)
    den = torch.randn(B, C, H, W, generator=g)
    den[torch.rand(den.shape, generator=g) < 0.1] = 0.0
    den_map = torch.rand(C, H, W, generator=g) + 0.5
    return a, R_y, den, den_map


def run_fwd(a, ph, pw):
    ad = a.to(DEV).contiguous()
    y = torch.full((a.size(0), a.size(1), a.size(2) // ph, a.size(3) // pw), float("nan"), device=DEV)
    _capi.call("drsa_amd_avgpool_fwd", ad.data_ptr(), y.data_ptr(), a.size(0), a.size(1), a.size(2), a.size(3), ph, pw,
               _capi.stream_ptr(DEV))
    return y.cpu()


def run_bwd(R_y, y, a, den, den_bcast, rule, clones, ph, pw, want_rel):
    Rd, yd, ad = (t.to(DEV).contiguous() for t in (R_y, y, a))
    dd = None if den is None else den.to(DEV).contiguous()
    Bq, H, W = R_y.size(0), a.size(2), a.size(3)
    g = torch.full((Bq, C, H, W), float("nan"), device=DEV)
    rel = torch.full((Bq, C, H, W), float("nan"), device=DEV) if want_rel else None
    _capi.call("drsa_amd_avgpool_bwd", Rd.data_ptr(), yd.data_ptr() if rule else None, ad.data_ptr(), _capi.ptr(dd),
               int(den_bcast), int(rule), EPS_POOL, EPS_CONV, g.data_ptr(), _capi.ptr(rel), Bq, clones, C, H, W, ph, pw,
               _capi.stream_ptr(DEV))
    return g.cpu(), None if rel is None else rel.cpu()


@pytest.mark.parametrize("H,W,ph,pw", SHAPES, ids=[f"{h}x{w}-{p}x{q}" for h, w, p, q in SHAPES])
def test_avgpool_fwd_bitwise(H, W, ph, pw):
    a, _, _, _ = inputs(H, W, ph, pw, 1)
    y = run_fwd(a, ph, pw)
    assert torch.equal(y, A.avgpool_fwd_ref(a, ph, pw)) and torch.equal(y, F.avg_pool2d(a, (ph, pw)))
    assert (y == 0).any() and (y > 0).any()


def test_avgpool_fwd_unaligned_and_odd_width():
    """A width that is no multiple of 4 and a view that is not 16-byte aligned take the scalar kernel."""
    a = torch.randn(2, 3, 6, 10).clamp(min=0)
    assert torch.equal(run_fwd(a, 2, 2), F.avg_pool2d(a, 2)) and torch.equal(run_fwd(a, 3, 5), F.avg_pool2d(a, (3, 5)))
    buf = torch.zeros(2 * 3 * 8 * 16 + 1, device=DEV)
    buf[1:] = torch.randn(2 * 3 * 8 * 16).clamp(min=0).to(DEV)
    view = buf[1:].view(2, 3, 8, 16)
    assert view.data_ptr() % 16 == 4
    y = torch.empty(2, 3, 4, 8, device=DEV)
    _capi.call("drsa_amd_avgpool_fwd", view.data_ptr(), y.data_ptr(), 2, 3, 8, 16, 2, 2, _capi.stream_ptr(DEV))
    assert torch.equal(y.cpu(), F.avg_pool2d(view.cpu(), 2))


@pytest.mark.parametrize("rule", [0, 1], ids=["plain", "epsilon"])
@pytest.mark.parametrize("clones", [1, 3])
@pytest.mark.parametrize("H,W,ph,pw", SHAPES, ids=[f"{h}x{w}-{p}x{q}" for h, w, p, q in SHAPES])
def test_avgpool_bwd_bitwise(H, W, ph, pw, clones, rule):
    a, R_y, den, den_map = inputs(H, W, ph, pw, clones)
    y = A.avgpool_fwd_ref(a, ph, pw)
    assert (y == 0).any() and ((a == 0) & (A.spread(y, ph, pw) > 0)).any()     # dead windows; dead pixels in live ones
    for dname, d, bcast in (("none", None, 0), ("sample", den, 0), ("map", den_map, 1)):
        g_ref, t_ref = A.avgpool_bwd_ref(R_y, y, a, d, bcast, rule, EPS_POOL, EPS_CONV, clones, ph, pw)
        assert torch.isfinite(g_ref).all() and float(g_ref.abs().max()) > 0
        for want_rel in (False, True):
            g, rel = run_bwd(R_y, y, a, d, bcast, rule, clones, ph, pw, want_rel)
            assert torch.equal(g, g_ref), (dname, want_rel)
            assert rel is None or torch.equal(rel, t_ref), dname
