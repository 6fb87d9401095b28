"""The ZBox first layer on the GPU: drsa_amd_first_layer_zbox_maps / _den / _bwd bit for bit against their CPU
restatement (tests/zbox_ref.py: pinned fma chains, every rounding of the epilogue explicit), and the engine
with a ZBox first layer against the float64 slow path (zbox_ref.slow_lrp: engine/hooks.py rule_relevance
under autograd), next to the fp32 slow path (lrp_common.f64_anchored_check at its default ratios).
Engine inputs are log-mels clamped to the box [-4, 2].  Parity with real zennit output is not pinned
(zennit is not installed here): the reference is the restated rule."""
import copy

import numpy as np
import pytest
import torch

import zbox_ref
from conv_ref import unpool
from lrp_common import f64_anchored_check, gtzan128, logmel, rel_l2, toy, u64, vggish
from drsa_audio_amd import _capi
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY, LRP_NAME_MAP_VGGISH
from drsa_audio_amd.xai.explain.attribute import compute_relevances
from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.rules import ZBox

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LOW, HIGH = -4.0, 2.0


def _weights(C, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    w[0, 0, 0, 0] = 0.0                                       # a tap in neither set
    return (w, torch.randn(C, generator=g) * 0.3 if bias else None)


def _bounds(H, W, seed):
    """Per-row bounds inside [-4, 2] (a scalar bound would hide a row / column mix-up)."""
    g = torch.Generator().manual_seed(seed)
    return zbox_ref.images(LOW + torch.rand(1, 1, H, 1, generator=g), HIGH - torch.rand(1, 1, H, 1, generator=g), H, W)


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


# ------------------------------------------------------------------ maps
@pytest.mark.parametrize("C,H,W", [(1, 1, 1), (5, 2, 5), (4, 9, 4)])
@pytest.mark.parametrize("bias", [True, False])
def test_maps(C, H, W, bias):
    w, b = _weights(C, C + H + W, bias)
    wp, wn, bp, bn = zbox_ref.split(w, b)
    lo, hi = _bounds(H, W, 7 + H)
    zl_ref, zh_ref = zbox_ref.maps_ref(wp, bp, wn, bn, lo, hi)
    zl, zh = (torch.full((C, H, W), float("nan"), device=DEV) for _ in range(2))
    keep = [_d(t) for t in (wp, bp, wn, bn, lo, hi)]
    _capi.call("drsa_amd_first_layer_zbox_maps", *(_capi.ptr(t) for t in keep), zl.data_ptr(), zh.data_ptr(), C, H, W,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert torch.equal(zl.cpu(), zl_ref) and torch.equal(zh.cpu(), zh_ref)


# ------------------------------------------------------------------ den
@pytest.mark.parametrize("H,W,pooled", [(2, 4, True), (34, 128, True), (5, 7, False)])
def test_den(H, W, pooled):
    B, C = 3, 5
    g = torch.Generator().manual_seed(H + W)
    zl, zh = torch.randn(C, H, W, generator=g), torch.randn(C, H, W, generator=g)
    if pooled:
        a = torch.randn(B, C, H // 2, W // 2, generator=g).clamp(min=0)
        amax = torch.randint(0, 4, a.shape, generator=g, dtype=torch.uint8)
        amax.view(-1)[:4] = torch.arange(4, dtype=torch.uint8)           # all four argmax bytes, whatever the draw
    else:
        a, amax = torch.randn(B, C, H, W, generator=g).clamp(min=0), None
    ref = zbox_ref.den_ref(a, amax, zl, zh)
    den = torch.full(a.shape, float("nan"), device=DEV)
    keep = [_d(t) for t in (a, amax, zl, zh)]
    _capi.call("drsa_amd_first_layer_zbox_den", *(_capi.ptr(t) for t in keep), den.data_ptr(), B, C, H, W,
               _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert torch.equal(den.cpu(), ref)


# ------------------------------------------------------------------ backward
def _bwd_inputs(C, H, W, clones, pooled, seed):
    """g with exact zeros (+0 and -0), negatives and every argmax position; x inside the per-row box with
    pixels exactly at low and at high; three samples."""
    g = torch.Generator().manual_seed(seed)
    S = 3
    Bq = S * clones
    hg, wg = (H // 2, W // 2) if pooled else (H, W)
    rel = torch.randn(Bq, C, hg, wg, generator=g)
    kind = torch.randint(0, 6, rel.shape, generator=g)
    rel = torch.where(kind == 0, torch.zeros_like(rel), rel)
    rel = torch.where(kind == 1, -torch.zeros_like(rel), rel)
    amax = None
    if pooled:
        amax = torch.randint(0, 4, (S, C, hg, wg), generator=g, dtype=torch.uint8)
        amax[:, 0, -1, -1] = 3                                 # the image's corner pixel
        amax.view(-1)[:4] = torch.arange(4, dtype=torch.uint8)
    lo, hi = _bounds(H, W, seed + 1)
    x = lo + torch.rand(S, 1, H, W, generator=g) * (hi - lo)
    where = torch.randint(0, 4, x.shape, generator=g)
    x = torch.where(where == 0, lo.expand_as(x), torch.where(where == 1, hi.expand_as(x), x)).contiguous()
    return rel, amax, x, lo, hi


def _bwd_call(rel, amax, wpn, x, lo, hi, clones, C, H, W):
    out = torch.full((rel.size(0), 1, H, W), float("nan"), device=DEV)
    _capi.call("drsa_amd_first_layer_zbox_bwd", rel.data_ptr(), _capi.ptr(amax), wpn.data_ptr(), x.data_ptr(),
               lo.data_ptr(), hi.data_ptr(), out.data_ptr(), rel.size(0), clones, C, H, W, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.cpu()


# dense: a map smaller than the window, W % 4 != 0 (scalar loads), 16k + 1 rows and 64k + 1 / 64k + 2 columns;
# pooled: one cell row, a partial 16 x 64-cell tile in each direction, and the W == 128 specialisation
DENSE = [(1, 1), (5, 7), (17, 65), (3, 130)]
POOLED = [(2, 4), (34, 128), (6, 136)]


@pytest.mark.parametrize("H,W,pooled", [(h, w, False) for h, w in DENSE] + [(h, w, True) for h, w in POOLED])
@pytest.mark.parametrize("C", [1, 5, 32])
@pytest.mark.parametrize("clones", [1, 4])
def test_bwd(H, W, pooled, C, clones):
    rel, amax, x, lo, hi = _bwd_inputs(C, H, W, clones, pooled, 31 * H + W + C + clones)
    w, _ = _weights(C, C + 3, bias=False)
    wp, wn, _, _ = zbox_ref.split(w)
    ref = zbox_ref.bwd_ref(rel, amax, wp, wn, x, lo, hi, clones)
    dwpn, dx, dlo, dhi, drel, damax = (_d(t) for t in (zbox_ref.pack_wpn(wp, wn), x, lo, hi, rel, amax))
    out = _bwd_call(drel, damax, dwpn, dx, dlo, dhi, clones, C, H, W)
    assert torch.equal(out, ref)
    if pooled:      # the pooled kernel equals the dense one on the expanded g
        dense = _bwd_call(_d(unpool(rel, amax, 2, clones)), None, dwpn, dx, dlo, dhi, clones, C, H, W)
        assert torch.equal(out, dense)


def test_bwd_dense_misaligned_g():
    """A dense g 4 bytes off a 16-byte boundary takes the scalar loads: the same bits."""
    C, H, W, clones = 5, 17, 64, 2
    rel, _, x, lo, hi = _bwd_inputs(C, H, W, clones, False, 77)
    w, _ = _weights(C, 8, bias=False)
    wp, wn, _, _ = zbox_ref.split(w)
    ref = zbox_ref.bwd_ref(rel, None, wp, wn, x, lo, hi, clones)
    buf = torch.empty(rel.numel() + 1, device=DEV)
    view = buf[1:].view(rel.shape)
    view.copy_(rel)
    assert view.data_ptr() % 16 == 4
    out = _bwd_call(view, None, _d(zbox_ref.pack_wpn(wp, wn)), _d(x), _d(lo), _d(hi), clones, C, H, W)
    assert torch.equal(out, ref)


# dense: scalar loads with partial tiles both ways, float4 loads; pooled: generic width with a partial tile,
# the W == 128 specialisation with partial tile rows
@pytest.mark.parametrize("H,W,pooled", [(17, 65, False), (16, 64, False), (6, 136, True), (34, 128, True)])
def test_bwd_runs_the_chain_of_first_layer_bwd(H, W, pooled):
    """Non-negative weights (W+ = w2, W- = +0), x = 1, low = 0, high = 1: ZBox returns (1 - 0) S+ + (1 - 1) S-
    = S+ + 0, and S+ is the chain of drsa_amd_first_layer_bwd on the same g, amax and w2: bit for bit (a
    signed zero compares equal), both entry points being one kernel with one or two chains."""
    C, clones = 5, 2
    rel, amax, x, _, _ = _bwd_inputs(C, H, W, clones, pooled, 500 + H + W)
    w2 = torch.rand(C, 9, generator=torch.Generator().manual_seed(H * W))
    wpn = torch.stack([w2, torch.zeros_like(w2)])
    drel, damax, dw2, dwpn = (_d(t) for t in (rel, amax, w2, wpn))
    one, lo, hi = torch.ones_like(x), torch.zeros(H, W), torch.ones(H, W)
    zbox = _bwd_call(drel, damax, dwpn, _d(one), _d(lo), _d(hi), clones, C, H, W)
    out = torch.full((rel.size(0), 1, H, W), float("nan"), device=DEV)
    _capi.call("drsa_amd_first_layer_bwd", drel.data_ptr(), _capi.ptr(damax), dw2.data_ptr(), out.data_ptr(),
               rel.size(0), clones, C, H, W, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert float(out.abs().max().cpu()) > 0 and torch.equal(zbox, out.cpu())


# ------------------------------------------------------------------ engine
def _zmap(nm):
    return [(["features.0"], ZBox(LOW, HIGH, stabilizer=1e-7))] + list(nm[1:])


def _x(B, H, W, seed):
    return logmel(B, H, W, seed=seed).clamp(LOW, HIGH)


def _gpu(m):
    return copy.deepcopy(m).to(DEV)


def _anchored(net, nm, x, cls, canonizers=(), tag=""):
    merge = bool(canonizers)
    _, R64 = zbox_ref.slow_lrp(net, nm, x, cls, torch.float64, merge_bn=merge)
    _, R32 = zbox_ref.slow_lrp(net, nm, x, cls, torch.float32, merge_bn=merge)
    comp = NameMapComposite(nm, canonizers=list(canonizers))
    Rg = compute_relevances(_gpu(net), x.to(DEV), comp, class_idx=cls).cpu()
    e, eref = rel_l2(Rg, R64), rel_l2(R32, R64)
    print(f"\n[zbox {tag}] rel-L2 vs f64: HIP median {np.median(e):.2e} p75 {np.percentile(e, 75):.2e} "
          f"max {e.max():.2e}; fp32 slow path median {np.median(eref):.2e} p75 {np.percentile(eref, 75):.2e} max {eref.max():.2e}")
    f64_anchored_check(Rg, R32, R64)
    return comp, Rg


@pytest.mark.parametrize("which", ["toy", "gtzan128"])
def test_engine_f64_anchored_and_batch_split(which):
    net, nm, (H, W), cls = (toy(), LRP_NAME_MAP_TOY, (64, 64), 1) if which == "toy" else \
        (gtzan128(), LRP_NAME_MAP_GTZAN, (128, 128), 7)
    x = _x(8, H, W, seed=61)
    assert float(x.min()) == LOW and float(x.max()) <= HIGH
    comp, Rg = _anchored(net, _zmap(nm), x, cls, tag=which)
    m = _gpu(net)
    halves = [compute_relevances(m, x[i:i + 4].to(DEV), comp, class_idx=cls).cpu() for i in (0, 4)]
    assert torch.equal(torch.cat(halves), Rg)


def test_engine_vggish_dense_first_layer():
    """VGGish: no pool after the first conv, so its backward takes a dense g (through the second conv)."""
    net = vggish(input_size=(64, 128))
    x = _x(8, 64, 128, seed=62)
    _anchored(net, _zmap(LRP_NAME_MAP_VGGISH), x, 3, canonizers=[SequentialMergeBatchNorm()], tag="vggish 64x128")


def test_engine_bf16_plan():
    """model.bfloat16(): within the whole-plan bf16 bound (5e-3 relative L2 per sample) of the
    slow path on the bf16 definition (bf16-rounded weights, input and conv inputs; float64 otherwise; with
    the WSquare map it equals the oracle's mode "bf16" to the last bit).

    The inputs are those of test_bf16_gpu's whole-plan case (seed 21, class 6; the clamp leaves them as they
    are).  A bf16 plan's forward does not depend on the first layer's rule, and it is the forward where an
    accumulation order can flip the bf16 rounding of an activation: on the CPU, the same definition
    accumulated in fp32 instead of float64 moves sample 0 of seed 63 by 1.7e-2, with WSquare as with ZBox, so
    such a sample says nothing about the first layer."""
    from drsa_audio_amd.engine import get_engine
    net = gtzan128().bfloat16()
    x = _x(4, 128, 128, seed=21).bfloat16()
    nm = _zmap(LRP_NAME_MAP_GTZAN)
    _, Rref = zbox_ref.slow_lrp(copy.deepcopy(net).float(), nm, x.float(), 6, torch.float64, bf16=True)
    comp = NameMapComposite(nm)
    m = _gpu(net)
    R = compute_relevances(m, x.to(DEV), comp, class_idx=6).cpu()
    assert get_engine(m, comp).precision == "bf16"
    e = rel_l2(R, Rref)
    print(f"\n[zbox bf16] rel-L2 vs the bf16 definition: {e}")
    assert e.max() <= 5e-3


@pytest.mark.parametrize("standard", ["sum", "clone"])
def test_heatmap_generator(standard):
    """j = 7, K = 4: both standard-heatmap modes run on the ZBox first layer (K and K + 1 clones through the
    pool-sparse backward); the concept maps sum to clone 0 within the bound of test_bench_size_properties."""
    net, x = gtzan128(), _x(4, 128, 128, seed=64).to(DEV)
    nm = _zmap(LRP_NAME_MAP_GTZAN)
    hg = HeatmapGenerator(_gpu(net), u64(), nm, "jazz", num_concepts=4, layer_idx=7, standard=standard)
    hg.generate_subspace_heatmaps(x, to_host=False)
    a = hg.info_device
    assert torch.isfinite(a["subspace_heatmaps"]).all() and float(a["standard_heatmaps"].abs().max()) > 0
    hc = HeatmapGenerator(_gpu(net), u64(), nm, "jazz", num_concepts=4, layer_idx=7, standard="clone")
    hc.generate_subspace_heatmaps(x, to_host=False)
    std = hc.info_device["standard_heatmaps"][:, 0].double()
    s = a["subspace_heatmaps"].double().sum(1)
    scale = std.abs().amax(dim=(1, 2), keepdim=True)
    assert float(((s - std).abs() / scale).max()) < 1e-4


def test_wsquare_plan_unchanged_around_a_zbox_plan():
    """A WSquare plan compiled before and after a ZBox plan in one process: bit-identical heatmaps (nothing is
    shared through the per-shape map cache)."""
    net, x = gtzan128(), _x(2, 128, 128, seed=65).to(DEV)
    comp_w = lambda: NameMapComposite(LRP_NAME_MAP_GTZAN)     # noqa: E731
    before = compute_relevances(_gpu(net), x, comp_w(), class_idx=2)
    m = _gpu(net)
    rz = compute_relevances(m, x, NameMapComposite(_zmap(LRP_NAME_MAP_GTZAN)), class_idx=2)
    same_model = compute_relevances(m, x, comp_w(), class_idx=2)
    after = compute_relevances(_gpu(net), x, comp_w(), class_idx=2)
    assert torch.equal(before, after) and torch.equal(before, same_model)
    assert not torch.equal(before, rz)


def test_epsilon_gamma_box_composite():
    """zennit's preset on the toy net (ZBox, Gamma, Epsilon, Pass on every activation): the same gate."""
    from drsa_audio_amd.zennit.composites import EpsilonGammaBox
    net, x = toy(), _x(8, 64, 64, seed=66)
    comp = EpsilonGammaBox(LOW, HIGH, epsilon=1e-7, gamma=0.8, stabilizer=1e-7)
    nm = [([n], r) for n, r in comp.rules(net).items()]
    _, R64 = zbox_ref.slow_lrp(net, nm, x, 0, torch.float64)
    _, R32 = zbox_ref.slow_lrp(net, nm, x, 0, torch.float32)
    Rg = compute_relevances(_gpu(net), x.to(DEV), comp, class_idx=0).cpu()
    f64_anchored_check(Rg, R32, R64)
