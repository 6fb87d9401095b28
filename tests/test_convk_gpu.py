"""The K x K conv kernels (csrc/conv_generic.hip) through the C ABI against the CPU reference
tests/convk_ref.py (GPU): every output bit-identical (torch.equal, NaN positions compared separately).

Cases (tests/convk_ref.py builds the lists; tests/test_convk_ref_cpu.py checks their coverage): kernel
sizes (1,1) (3,3) (5,5) (7,7) (3,5) (5,3) (1,7) x channel pairs 1 -> 8 (k padded to the MFMA step),
8 -> 40 (two output slices, the second padded), 40 -> 33 (two input chunks at 1x1, odd output count) x
maps 2x4 (every halo larger than the image), 6x12 and 10x36 (partial 8 x 16 tiles, several workgroups),
batch 3, with the (ng, den) combinations forward and the (ng, xmode, post, clones) modes backward rotating
over them; and 1 -> 20 backward (the one-output-channel kernel over three chunks of g channels, 18 x 20: two
of its 16 x 16 tiles each way).  Outputs are NaN-prefilled views between sentinel bands (test_conv_edges_gpu.Guard).

Anchors: at 3x3, 64 -> 64 on 8 x 32 the new entry points return the bits of drsa_amd_conv_fwd(pool = 0) /
drsa_amd_conv_bwd(g_amax = NULL); a 5x5 kernel with zero outer taps returns the bits of the 3x3 entry points.
"""
import pytest
import torch

import conv_ref as cr
import convk_ref as K
from drsa_audio_amd import _capi
from test_conv_edges_gpu import DEV, Guard, _cid, _same

pytestmark = pytest.mark.gpu


def _fwd(x, sets, bias3, den_map, want_den, kh, kw):
    B, cin, H, W = x.shape
    cout, ng = sets[0].size(0), len(sets)
    wts, bias = K._convk_fwd_layout(sets).to(DEV), K.pack_bias(bias3, cout).to(DEV)
    assert wts.numel() == _capi.lib().drsa_amd_convk_weight_floats(kh, kw, cin, cout, ng)
    out, den = Guard((B, cout, H, W)), Guard((B, cout, H, W)) if want_den else None
    dm = None if den_map is None else den_map.to(DEV)
    _capi.call("drsa_amd_convk_fwd", x.to(DEV).data_ptr(), wts.data_ptr(), bias.data_ptr(), _capi.ptr(dm), out.ptr(),
               den.ptr() if den else None, B, cin, cout, H, W, kh, kw, ng, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.result(), den.result() if den else None


def _bwd(g, sets, x, den, clones, xmode, post, kh, kw, eps=K.EPS):
    """sets are forward-shaped (cin -> cout); the call mirrors the pair."""
    Bq, cout, H, W = g.shape
    cin, ng = sets[0].size(1), len(sets)
    wts = K._convk_bwd_layout(sets).to(DEV)
    assert wts.numel() == _capi.lib().drsa_amd_convk_weight_floats(kh, kw, cout, cin, ng)
    need_x = xmode != K.XM_NONE or post != K.POST_NONE
    xd, dd = x.to(DEV) if need_x else None, den.to(DEV) if post == K.POST_DIV else None
    out = Guard((Bq, cin, H, W))
    _capi.call("drsa_amd_convk_bwd", g.to(DEV).data_ptr(), wts.data_ptr(), _capi.ptr(xd), _capi.ptr(dd), out.ptr(), Bq,
               clones, cout, cin, H, W, kh, kw, ng, xmode, post, eps, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.result()


@pytest.mark.parametrize("case", K.fwd_cases(), ids=_cid)
def test_forward(case):
    kh, kw, cin, cout, H, W, (ng, den) = case
    assert _capi.lib().drsa_amd_convk_supported(kh, kw, cin, cout) == 1
    x, sets, bias3, den_map = K.fwd_inputs(cin, cout, H, W, kh, kw, ng)
    want_y, want_d = K.convk_fwd_ref(x, sets, bias3, den, den_map)
    got_y, got_d = _fwd(x, sets, bias3, den_map if den == "map" else None, den != "none", kh, kw)
    _same(got_y, want_y, "out")
    if den != "none":
        _same(got_d, want_d, "out_den")


@pytest.mark.parametrize("case", K.bwd_cases() + K.bwd_one_channel_cases(), ids=_cid)
def test_backward(case):
    kh, kw, cin, cout, H, W, (ng, xmode, post, clones) = case
    g, sets, x, den = K.bwd_inputs(cin, cout, H, W, kh, kw, ng, clones)
    want = K.convk_bwd_ref(g, sets, x, den, clones, xmode, post, K.EPS)
    _same(_bwd(g, sets, x, den, clones, xmode, post, kh, kw), want, "out")


# ------------------------------------------------------------------ anchors on the 3x3 entry points
def _conv3_fwd(x, sets, bias3, den_map, want_den):
    B, cin, H, W = x.shape
    cout, ng = sets[0].size(0), len(sets)
    wts, bias = cr.pack_fwd(sets).to(DEV), cr.pack_bias(bias3, cout).to(DEV)
    out, den = Guard((B, cout, H, W)), Guard((B, cout, H, W)) if want_den else None
    dm = None if den_map is None else den_map.to(DEV)
    _capi.call("drsa_amd_conv_fwd", x.to(DEV).data_ptr(), wts.data_ptr(), bias.data_ptr(), _capi.ptr(dm), out.ptr(), None,
               den.ptr() if den else None, B, cin, cout, H, W, ng, 0, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.result(), den.result() if den else None


def _conv3_bwd(g, sets, x, den, clones, xmode, post):
    Bq, cout, H, W = g.shape
    cin, ng = sets[0].size(1), len(sets)
    wts = cr.pack_bwd(sets).to(DEV)
    need_x = xmode != K.XM_NONE or post != K.POST_NONE
    xd, dd = x.to(DEV) if need_x else None, den.to(DEV) if post == K.POST_DIV else None
    out = Guard((Bq, cin, H, W))
    _capi.call("drsa_amd_conv_bwd", g.to(DEV).data_ptr(), None, wts.data_ptr(), _capi.ptr(xd), _capi.ptr(dd), out.ptr(), Bq,
               clones, cout, cin, H, W, ng, xmode, post, K.EPS, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.result()


def _embed(w, kh, kw):
    big = torch.zeros(*w.shape[:2], kh, kw)
    big[:, :, (kh - 3) // 2:(kh + 3) // 2, (kw - 3) // 2:(kw + 3) // 2] = w
    return big


def _finite(x):
    return torch.nan_to_num(x, nan=0.5)


@pytest.mark.parametrize("combo", K.FWD_COMBOS, ids=_cid)
def test_forward_3x3_is_conv_fwd(combo):
    ng, den = combo
    x, sets, bias3, den_map = K.fwd_inputs(64, 64, 8, 32, 3, 3, ng)
    x = x[:2].contiguous()
    dm = den_map if den == "map" else None
    got, want = _fwd(x, sets, bias3, dm, den != "none", 3, 3), _conv3_fwd(x, sets, bias3, dm, den != "none")
    _same(got[0], want[0], "out")
    if den != "none":
        _same(got[1], want[1], "out_den")
    # the device's zero-embedding: 5x5 with zero outer taps, on finite inputs (NaN * 0 would differ)
    xf = _finite(x)
    emb = _fwd(xf, [_embed(w, 5, 5) for w in sets], bias3, dm, den != "none", 5, 5)
    ref = _conv3_fwd(xf, sets, bias3, dm, den != "none")
    _same(emb[0], ref[0], "embedded out")
    if den != "none":
        _same(emb[1], ref[1], "embedded out_den")


@pytest.mark.parametrize("mode", K.BWD_MODES, ids=_cid)
def test_backward_3x3_is_conv_bwd(mode):
    ng, xmode, post, clones = mode
    g, sets, x, den = K.bwd_inputs(64, 64, 8, 32, 3, 3, ng, clones)
    g, x, den = g[:2 * clones].contiguous(), x[:2].contiguous(), den[:2].contiguous()
    want = _conv3_bwd(g, sets, x, den, clones, xmode, post)
    _same(_bwd(g, sets, x, den, clones, xmode, post, 3, 3), want, "out")
    _same(_bwd(g, [_embed(w, 5, 5) for w in sets], x, den, clones, xmode, post, 5, 5), want, "embedded out")
