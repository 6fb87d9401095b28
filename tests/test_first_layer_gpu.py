"""drsa_amd_first_layer_bwd (WSquare / Flat backward of the one-channel input conv): the pool-sparse
kernel (cells staged through range-checked buffer loads into a pixel image that keeps its zeros)
against the dense kernel fed the host-unpooled relevance, bitwise -- both run the (channel, dy, dx)
chain of oracle/lrp_exact.c.  Shapes cover partial 16 x 64-cell tiles in both directions (the
out-of-range rows and columns of the staging), one channel, and 1-4 clones sharing one argmax map.
The dense kernel alone against the float64 transposed conv within the kernel gate (2e-5 of the sum of
|terms|), at W % 4 != 0 (its scalar-load form), with signed weights and exact zeros, and from a
16-byte aligned and an unaligned base; drsa_amd_first_layer_den against the float64 conv of ones, with
more than one input channel.
Reference: cxai/xai/explain/attribute.py (compute_relevances through zennit's WSquare / Flat)."""
import pytest
import torch

from drsa_audio_amd import _capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _unpool(gp, amax, clones):
    Bq, C, H2, W2 = gp.shape
    am = amax.repeat_interleave(clones, 0).long()
    up = torch.zeros(Bq, C, 2 * H2, 2 * W2, device=gp.device)
    for sb in range(4):
        up[:, :, sb // 2::2, sb % 2::2] = torch.where(am == sb, gp, torch.zeros_like(gp))
    return up


@pytest.mark.parametrize("H,W", [(128, 128), (34, 128), (2, 128), (64, 64), (34, 200), (2, 4), (96, 136)])
@pytest.mark.parametrize("C", [1, 5, 32])
@pytest.mark.parametrize("clones", [1, 4])
def test_pooled_equals_dense(H, W, C, clones):
    g = torch.Generator().manual_seed(H + W + C + clones)
    Bs = 3
    Bq = Bs * clones
    gp = torch.randn(Bq, C, H // 2, W // 2, generator=g).to(DEV)
    amax = torch.randint(0, 4, (Bs, C, H // 2, W // 2), generator=g, dtype=torch.uint8).to(DEV)
    w2 = torch.rand(C, 9, generator=g).to(DEV)
    s = _capi.stream_ptr(DEV)
    outs = []
    for pooled in (True, False):
        out = torch.full((Bq, 1, H, W), float("nan"), device=DEV)
        src = gp if pooled else _unpool(gp, amax, clones)
        _capi.call("drsa_amd_first_layer_bwd", src.data_ptr(), amax.data_ptr() if pooled else None, w2.data_ptr(),
                   out.data_ptr(), Bq, clones, C, H, W, s)
        outs.append(out)
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1])
    # semantics: the transposed 3 x 3 conv of the unpooled relevance with the squared weights
    ref = torch.nn.functional.conv_transpose2d(_unpool(gp, amax, clones).double(), w2.double().view(C, 1, 3, 3), padding=1)
    assert torch.allclose(outs[0].double(), ref, rtol=1e-5, atol=1e-5)


def _dense_inputs(Bq, C, H, W, seed):
    """Signed weights, relevance with about a third of its entries exactly 0 (some of them -0)."""
    g = torch.Generator().manual_seed(seed)
    rel = torch.randn(Bq, C, H, W, generator=g)
    kind = torch.randint(0, 6, rel.shape, generator=g)
    rel = torch.where(kind == 0, torch.zeros_like(rel), rel)
    rel = torch.where(kind == 1, -torch.zeros_like(rel), rel)
    return rel.to(DEV), torch.randn(C, 9, generator=g).to(DEV)


def _dense_call(rel, w2, H, W):
    Bq, C = rel.shape[:2]
    out = torch.full((Bq, 1, H, W), float("nan"), device=DEV)
    _capi.call("drsa_amd_first_layer_bwd", rel.data_ptr(), None, w2.data_ptr(), out.data_ptr(), Bq, 1, C, H, W,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out


def _dense_check(out, rel, w2, tag):
    """Within the kernel gate (2e-5 of the sum of |terms|) of the float64 transposed conv."""
    C = rel.shape[1]
    ct = torch.nn.functional.conv_transpose2d
    ref = ct(rel.double(), w2.double().view(C, 1, 3, 3), padding=1)
    bound = 2e-5 * ct(rel.double().abs(), w2.double().abs().view(C, 1, 3, 3), padding=1)
    err = (out.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()
    print(f"{tag}: max err / bound = {ratio:.3e}")
    assert not torch.isnan(out).any()
    assert ratio <= 1.0


# W % 4 = 1, 2, 3 (first_layer_bwd_kernel<false>: scalar loads under a per-element column mask), W = 64k + 1
# and 64k + 2 (a second tile column that holds one or two pixels: the right halo column of the first
# and the masked last float4 meet), H = 16k + 1, and a map smaller than the 3 x 3 window
@pytest.mark.parametrize("H,W", [(5, 7), (16, 64), (17, 65), (3, 130), (33, 66), (1, 1), (2, 3)])
@pytest.mark.parametrize("C", [1, 5, 8])
def test_dense_against_float64(H, W, C):
    rel, w2 = _dense_inputs(2, C, H, W, 31 * H + W + C)
    _dense_check(_dense_call(rel, w2, H, W), rel, w2, f"{H}x{W} C={C}")


def test_dense_aligned_and_unaligned_base():
    """The float4 loads of the dense kernel need a 16-byte aligned relevance; a base that is not takes
    the scalar-load kernel (the dispatch tests the base, not only W % 4) and gives the same bits."""
    Bq, C, H, W = 2, 5, 17, 64
    rel, w2 = _dense_inputs(Bq, C, H, W, 5)
    buf = torch.empty(rel.numel() + 1, device=DEV)
    outs = []
    for off in (0, 1):
        view = buf[off:off + rel.numel()].view(rel.shape)
        view.copy_(rel)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
        out = _dense_call(view, w2, H, W)
        _dense_check(out, rel, w2, f"base % 16 = {4 * off}")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    # the pooled kernel stores float4: it refuses an output that is not 16-byte aligned
    gp = torch.randn(Bq, C, H // 2, W // 2, device=DEV)
    amax = torch.zeros(Bq, C, H // 2, W // 2, dtype=torch.uint8, device=DEV)
    obuf = torch.zeros(Bq * 16 * W + 1, device=DEV)
    with pytest.raises(_capi.DrsaAmdError, match="16-byte aligned"):
        _capi.call("drsa_amd_first_layer_bwd", gp.data_ptr(), amax.data_ptr(), w2.data_ptr(), obuf[1:].data_ptr(), Bq,
                   1, C, 16, W, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert torch.count_nonzero(obuf) == 0


# C output channels x CI input channels (the plan and the ring test only ever pass CI = 1); the corners
# and edges of the map see 4 and 6 of the 9 taps
@pytest.mark.parametrize("C,CI", [(1, 1), (5, 1), (4, 3)])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (9, 4)])
@pytest.mark.parametrize("bias", [True, False])
def test_den_map(C, CI, H, W, bias):
    g = torch.Generator().manual_seed(C + 10 * CI + H + W)
    w2 = torch.randn(C, CI, 3, 3, generator=g).to(DEV)
    b2 = torch.randn(C, generator=g).to(DEV) if bias else None
    den = torch.full((C, H, W), float("nan"), device=DEV)
    _capi.call("drsa_amd_first_layer_den", w2.data_ptr(), _capi.ptr(b2), den.data_ptr(), C, CI, H, W,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    ones = torch.ones(1, CI, H, W, dtype=torch.float64, device=DEV)
    conv = torch.nn.functional.conv2d
    ref = conv(ones, w2.double(), padding=1)[0]
    bound = conv(ones, w2.double().abs(), padding=1)[0]
    if bias:
        ref = ref + b2.double().view(C, 1, 1)
        bound = bound + b2.double().abs().view(C, 1, 1)
    err = (den.double() - ref).abs()
    ratio = (err / (2e-5 * bound)).max().item()
    print(f"C={C} CI={CI} {H}x{W} bias={int(bias)}: max err / bound = {ratio:.3e}")
    assert not torch.isnan(den).any()
    assert ratio <= 1.0
    # the four corners and the edges differ from the interior: each against its own taps
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 0), (0, W // 2)):
        ys, xs = [k for k in range(3) if 0 <= y + k - 1 < H], [k for k in range(3) if 0 <= x + k - 1 < W]
        want = w2.double()[:, :, ys][:, :, :, xs].sum((1, 2, 3)) + (b2.double() if bias else 0)
        assert ((den[:, y, x].double() - want).abs() <= 2e-5 * bound[:, y, x]).all(), (y, x)
