"""The dense-head kernels (csrc/linear.hip, csrc/linear_rules.hip: seven MFMA kernels behind
drsa_amd_linear_fwd / _bwd and drsa_amd_linear_rule_fwd / _bwd) at tile and chunk edges, through the C
ABI, against the CPU reference tests/linear_ref.py (GPU).

Every output is bit-identical to the reference (the oracle's k-ascending fma chains plus elementwise
fp32 steps): torch.equal, NaN positions compared separately (test_conv_edges_gpu._same).  Every output
sits in test_conv_edges_gpu.Guard: a view between two runs of sentinels, prefilled with a marked NaN;
after the call the sentinels are untouched and no element still holds the prefill.  An output that is
not requested is passed as null.  tests/test_linear_ref_cpu.py checks the reference itself, that the
inputs can show a guard, stabiliser, clamp or mask mistake in the last partial tile, and that the lists
below reach every kernel at every M, N and K.

Shapes (linear_ref.fwd_shapes / bwd_shapes), the smallest that reach each path:
  M        1, 17 (a second 16-row tile of one row), 33 (a second 32-row workgroup of one row), 50
  N / Kin  3, 20, 33, 48
  fwd K    3, 31, 32, 33, 100 (K % 4 == 0 below 128: the short kernel), 128 (one long chunk, no prefetch),
           130 (the short kernel over five chunks), 132 and 260 (a tail of 4 after one and two full
           chunks), 384 (three full chunks)
  bwd K    Nout = 1, 3, 31, 33, 70
Every M meets every K, N rotating so that every M and every K meets every N; the largest case is
50 x 48 x 384.  Every shape runs every instantiation and every mode of its entry point:
  linear_fwd       bias x relu_out, and one run with a NaN in the last row of x
  linear_bwd       R / class seed / one-hot seed x post NONE / DIV / MASK, relu_mask x rule_eps x xmode
  linear_rule_fwd  Gamma (signed, den_n) in all four, ZPlus signed / unsigned; biases x relu_out, one NaN run
  linear_rule_bwd  Gamma's four (zsign = 1), ZPlus' two (zsign = 0), WSquare and Flat (den_bcast = 1, xmul = 0,
                   no Wn; the plan's constant denominator); source x post, relu_mask alternating
Anchors: linear_rule_fwd's z and relu are linear_fwd's bits on the same device buffers; linear_rule_bwd
unsigned without den_n at zsign = 0, Wp = W, den_p = z is linear_bwd(rule_eps = 1, XM_MUL).  Alignment:
x or a weight set one float off the 16-byte grid at K = 132 and 260 (the long-K kernels read float4;
the dispatch sends such a call to the element-wise kernel) gives the aligned call's bits.
"""
import pytest
import torch

import linear_ref as lr
from drsa_audio_amd import _capi
from test_conv_edges_gpu import DEV, Guard, _same

pytestmark = pytest.mark.gpu


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _off(t):
    """t on the device as a contiguous view that starts one float into its buffer."""
    buf = torch.zeros(t.numel() + 8, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _guards(want, shape):
    return {k: (Guard(shape) if v is not None else None) for k, v in want.items()}


def _gp(g):
    return g.ptr() if g is not None else None


def _check(outs, want, what):
    torch.cuda.synchronize()
    got = {}
    for k, ref in want.items():
        if ref is not None:
            got[k] = outs[k].result()
            _same(got[k], ref, f"{what} {k}")
    return got


def _run_lin_fwd(d, want, M, N, K):
    outs = _guards(want, (M, N))
    _capi.call("drsa_amd_linear_fwd", d["x"].data_ptr(), d["W"].data_ptr(), _capi.ptr(d["b"]), outs["z"].ptr(),
               _gp(outs["relu"]), M, N, K, _capi.stream_ptr(DEV))
    return outs


def _run_rule_fwd(d, want, M, N, K):
    outs = _guards(want, (M, N))
    _capi.call("drsa_amd_linear_rule_fwd", d["x"].data_ptr(), d["W"].data_ptr(), d["Wp"].data_ptr(), _capi.ptr(d["Wn"]),
               _capi.ptr(d["b"]), _capi.ptr(d["bp"]), _capi.ptr(d["bn"]), outs["z"].ptr(), _gp(outs["relu"]),
               outs["den_p"].ptr(), _gp(outs["den_n"]), d["signed"], M, N, K, _capi.stream_ptr(DEV))
    return outs


def _run_lin_bwd(d, want, M, Nout, Kin):
    outs = _guards(want, (M, Kin))
    _capi.call("drsa_amd_linear_bwd", _capi.ptr(d["R"]), _capi.ptr(d["cls"]), d["one_hot"], d["z"].data_ptr(),
               d["relu_mask"], d["rule_eps"], d["eps"], d["W"].data_ptr(), _capi.ptr(d["x"]), d["xmode"], _capi.ptr(d["den"]),
               d["post"], d["eps_post"], outs["out"].ptr(), M, Nout, Kin, _capi.stream_ptr(DEV))
    return outs


def _run_rule_bwd(d, want, M, Nout, Kin):
    outs = _guards(want, (M, Kin))
    _capi.call("drsa_amd_linear_rule_bwd", _capi.ptr(d["R"]), _capi.ptr(d["cls"]), d["one_hot"], d["z"].data_ptr(),
               d["relu_mask"], d["den_p"].data_ptr(), _capi.ptr(d["den_n"]), d["den_bcast"], d["zsign"], d["eps"],
               d["Wp"].data_ptr(), _capi.ptr(d["Wn"]), _capi.ptr(d["x"]), d["xmul"], d["signed"], _capi.ptr(d["den"]),
               d["post"], d["eps_post"], outs["out"].ptr(), M, Nout, Kin, _capi.stream_ptr(DEV))
    return outs


_RUN = {"linear_fwd": _run_lin_fwd, "linear_rule_fwd": _run_rule_fwd, "linear_bwd": _run_lin_bwd,
        "linear_rule_bwd": _run_rule_bwd}


def _upload(a):
    return {k: (_dev(v) if isinstance(v, torch.Tensor) else v) for k, v in a.items()}


_ENTRIES = lr.entries()


@pytest.mark.parametrize("entry", _ENTRIES, ids=[e[0] for e in _ENTRIES])
def test_linear_edges(entry):
    """Every shape x mode of one entry point and instantiation, bit for bit."""
    name, ep, inst, shapes, modes, build = entry
    n = 0
    for i, shape in enumerate(shapes):
        for mode in modes:
            a, want = build(shape, mode, i)
            d = _upload(a)
            what = f"{name} shape={shape} mode={mode}"
            got = _check(_RUN[ep](d, want, *shape), want, what)
            if ep == "linear_rule_fwd":
                # anchor: z and relu are drsa_amd_linear_fwd's bits on the same device buffers
                w2 = dict(z=want["z"], relu=want["relu"])
                g2 = _check(_run_lin_fwd(d, w2, *shape), w2, what + " (linear_fwd)")
                for k in g2:
                    _same(got[k], g2[k], what + f" {k} against linear_fwd")
            n += 1
    assert n == len(shapes) * len(modes)
    print(f"{name}: {n} cases")


@pytest.mark.parametrize("mode", lr.RULE_BWD_MODES, ids=lambda m: "-".join(map(str, m)))
def test_rule_bwd_degenerates_to_linear_bwd(mode):
    """linear_rule_bwd unsigned, without den_n, zsign = 0, Wp = W and den_p = z is the Epsilon backward
    linear_bwd(rule_eps = 1, XM_MUL): the same bits, and the reference's."""
    src, relu_mask, post = mode
    for shape in lr.bwd_shapes():
        a, want = lr.lin_bwd_case(shape, (src, relu_mask, 1, lr.XM_MUL, post))
        d = _upload(a)
        lin = _check(_run_lin_bwd(d, want, *shape), want, f"linear_bwd {shape}")
        d2 = dict(d, den_p=d["z"], den_n=None, den_bcast=0, zsign=0, Wp=d["W"], Wn=None, xmul=1, signed=0)
        rule = _check(_run_rule_bwd(d2, want, *shape), want, f"linear_rule_bwd {shape}")
        _same(rule["out"], lin["out"], f"rule against linear {shape}")


_ALIGN_SHAPES = [s for s in lr.fwd_shapes() if s[2] in (132, 260)]


@pytest.mark.parametrize("which", ["x", "W"])
def test_linear_fwd_unaligned_operand(which):
    """x or W one float off the 16-byte grid at K = 132 / 260: the aligned call's bits."""
    assert len(_ALIGN_SHAPES) == 8
    for shape in _ALIGN_SHAPES:
        a, want = lr.lin_fwd_case(shape, (1, 1, 0))
        d = _upload(a)
        assert all(d[k].data_ptr() % 16 == 0 for k in ("x", "W"))
        ref = _check(_run_lin_fwd(d, want, *shape), want, f"aligned {shape}")
        got = _check(_run_lin_fwd(dict(d, **{which: _off(a[which])}), want, *shape), want, f"{which} off by 4 bytes {shape}")
        for k in ref:
            _same(got[k], ref[k], f"{which} off by 4 bytes against aligned {shape} {k}")


@pytest.mark.parametrize("which", ["x", "W", "Wp", "Wn"])
@pytest.mark.parametrize("inst", [("gamma", 1, 1), ("gamma", 0, 0)], ids=["signed-negden", "unsigned"])
def test_linear_rule_fwd_unaligned_operand(inst, which):
    """x or one weight set one float off the 16-byte grid at K = 132 / 260: the aligned call's bits.  The
    unsigned forward without den_n is given a Wn too (it does not read it): every set that is passed counts."""
    for shape in _ALIGN_SHAPES:
        a, want = lr.rule_fwd_case(shape, inst, (1, 1, 0))
        if a["Wn"] is None:
            a = dict(a, Wn=lr.fwd_inputs(*shape, inst[1])["rp"]["gamma"]["Wn"])
        d = _upload(a)
        assert all(d[k].data_ptr() % 16 == 0 for k in ("x", "W", "Wp", "Wn"))
        ref = _check(_run_rule_fwd(d, want, *shape), want, f"aligned {shape}")
        got = _check(_run_rule_fwd(dict(d, **{which: _off(a[which])}), want, *shape), want,
                     f"{which} off by 4 bytes {shape}")
        for k in ref:
            _same(got[k], ref[k], f"{which} off by 4 bytes against aligned {shape} {k}")
