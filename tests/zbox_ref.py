"""CPU reference of the ZBox first-layer entry points (drsa_amd_first_layer_zbox_maps / _den / _bwd), for
the kernel tests, in the style of conv_ref.py.  No GPU, no kernel knowledge: it restates the ABI of
include/drsa_amd.h on top of the pinned-order primitives of oracle/lrp_exact.c (lrp_ref.ExactOps.conv /
conv_t: every output one k-ordered fp32 fma chain, k = channel * 9 + tap), followed by elementwise fp32
torch ops, one rounding each.  The kernels are specified to compute exactly this, so the tests built on
it compare with torch.equal.

``three_term_f64`` is zennit's own form of the rule (three modified forwards, the reducer
x grad_x - l grad_l - h grad_h) in float64: the definition the slow path (engine/hooks.py) is checked
against.  ``slow_lrp`` runs a whole model through that slow path on the CPU, in fp32 or float64: the
anchor of the engine tests.

The keyword argument ``pad="low"`` selects a deliberately WRONG variant: l / h padded with their own value
instead of the conv's zeros.  tests/test_zbox_cpu.py uses it to show that the test inputs can tell that
mistake from the right answer; nothing else may pass it.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_ref import _conv, _conv_t, at_argmax, unpool


def split(w, b=None):
    """(wp, wn [C][1][3][3], bp, bn [C] or None) of a first conv's weight [C][1][3][3] and bias."""
    bp, bn = (None, None) if b is None else (b.clamp(min=0), b.clamp(max=0))
    return w.clamp(min=0), w.clamp(max=0), bp, bn


def pack_wpn(wp, wn):
    """[2][C][9]: W+ then W- (drsa_amd_first_layer_zbox_bwd)."""
    return torch.stack([wp.reshape(-1, 9), wn.reshape(-1, 9)]).contiguous()


def images(low, high, H, W):
    """The bounds spread over one sample, [H][W] fp32 each (ZBox.bounds: low[:1].expand_as(x))."""
    out = []
    for v in (low, high):
        t = torch.as_tensor(v, dtype=torch.float32)
        if t.dim() == 4 and t.size(0) > 1:
            t = t[:1]
        out.append(t.expand(1, 1, H, W).reshape(H, W).contiguous())
    return out


# ------------------------------------------------------------------ the three entry points
def maps_ref(wp, bp, wn, bn, low_img, high_img, pad="zero"):
    """drsa_amd_first_layer_zbox_maps: (zl, zh) [C][H][W]; one fma chain per output over the in-image
    taps (ky, kx ascending; a zero-padded tap adds fma(0, w, acc) = acc), then one add for the bias."""
    mode = "replicate" if pad == "low" else "zero"
    zl = _conv(low_img[None, None], wp, mode)[0]
    zh = _conv(high_img[None, None], wn, mode)[0]
    if bp is not None:
        zl = zl + bp.view(-1, 1, 1)
    if bn is not None:
        zh = zh + bn.view(-1, 1, 1)
    return zl, zh


def den_ref(a, amax, zl, zh):
    """drsa_amd_first_layer_zbox_den: (a - zl[at]) - zh[at]; amax: a is 2x2-pooled, at = the argmax pixel."""
    if amax is not None:
        B = a.size(0)
        zl = at_argmax(zl.unsqueeze(0).expand(B, -1, -1, -1).contiguous(), amax, 2)
        zh = at_argmax(zh.unsqueeze(0).expand(B, -1, -1, -1).contiguous(), amax, 2)
    return (a - zl) - zh


def bwd_ref(g, amax, wp, wn, x, low_img, high_img, clones):
    """drsa_amd_first_layer_zbox_bwd: out [Bq][1][H][W].  S+ and S- are one fma chain each per pixel in the
    order (channel, dy, dx) (ExactOps.conv_t); then x - l, x - h, the two products and their sum, each rounded."""
    gf = g if amax is None else unpool(g, amax, 2, clones)
    sp, sn = _conv_t(gf, wp), _conv_t(gf, wn)
    xq = x.repeat_interleave(clones, 0)
    return (xq - low_img) * sp + (xq - high_img) * sn


# ------------------------------------------------------------------ zennit's three-term form, float64
def three_term_f64(w, b, x, low_img, high_img, R, stabilizer, pad="zero", parts=False):
    """R_in of ZBox on a 3x3 'same' conv in float64: den = (f(x; W, b) - f(l; W+, b+)) - f(h; W-, b-),
    g = R / stab(den), R_in = x J^T_W g - l J^T_{W+} g - h J^T_{W-} g.  parts: (R_in, den, g)."""
    d = torch.float64
    w, x, R = w.to(d), x.to(d), R.to(d)
    b = None if b is None else b.to(d)
    lo, hi = low_img.to(d).expand_as(x), high_img.to(d).expand_as(x)
    wp, wn, bp, bn = split(w, b)

    def f(t, wt, bt, own):
        if own:     # the wrong variant: the bound's own value beyond the border
            return F.conv2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), wt, bt)
        return F.conv2d(t, wt, bt, padding=1)
    own = pad == "low"
    den = (f(x, w, b, False) - f(lo, wp, bp, own)) - f(hi, wn, bn, own)
    g = R / (den + stabilizer * ((den >= 0).to(d) * 2 - 1))
    jt = lambda wt: F.conv_transpose2d(g, wt, padding=1)    # noqa: E731
    r = x * jt(w) - lo * jt(wp) - hi * jt(wn)
    return (r, den, g) if parts else r


# ------------------------------------------------------------------ a whole model through the slow path
class _Bf16Round(torch.autograd.Function):
    """Round to bf16 values in the forward; the gradient passes as it is (a dtype cast would round it too)."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


_bf16r = _Bf16Round.apply


def slow_lrp(model, name_map, x, class_idx, dtype=torch.float32, merge_bn=False, bf16=False):
    """The relevance at the input of ``model`` under ``name_map`` by engine/hooks.py's rule_relevance (zennit's
    structure: modified forwards and autograd), on the CPU in ``dtype``; unmapped modules take the plain
    gradient.  ``bf16``: the bf16 plan's definition (oracle lrp_ref.Bf16Ops) on this path: the input and every
    conv's input and (rule-modified) weights rounded to bf16 values, everything else at full precision."""
    from drsa_audio_amd.engine import hooks
    net = copy.deepcopy(model).to(dtype).eval()
    if merge_bn:
        net = hooks._merge_bn(net)
    rules = {n: r for names, r in name_map for n in names}
    mods, store, handles = dict(net.named_modules()), {}, []
    aff0 = hooks._aff

    def aff_bf16(m, t, w, b):
        if isinstance(m, nn.Conv2d):
            return F.conv2d(_bf16r(t), _bf16r(w), b, m.stride, m.padding, m.dilation, m.groups)
        return aff0(m, t, w, b)
    if bf16:
        x = _bf16r(x.to(dtype))
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.forward = (lambda t, m=m: aff_bf16(m, t, m.weight, m.bias))
    for name, rule in rules.items():
        m = mods[name]

        def fwd(mod, inp, out, name=name):
            store[name] = inp[0].detach()

        def bwd(mod, grad_input, grad_output, name=name, rule=rule):
            R_in = hooks.rule_relevance(rule, mod, store[name], grad_output[0])
            return tuple(R_in if (gi is not None and gi.shape == R_in.shape) else gi for gi in grad_input)
        handles += [m.register_forward_hook(fwd), m.register_full_backward_hook(bwd)]
    try:
        hooks._aff = aff_bf16 if bf16 else aff0
        xin = x.detach().to(dtype).requires_grad_(True)
        out = net(xin)
        mask = torch.zeros_like(out)
        mask[:, class_idx] = 1
        R, = torch.autograd.grad(out, xin, (out * mask).detach())
    finally:
        hooks._aff = aff0
        for h in handles:
            h.remove()
    return out.detach(), R.detach()
