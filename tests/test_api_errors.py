"""Error behaviour of the host layer and the C ABI (CPU: every check fires before device work).

Mirrors the reference's runtime asserts (drsa.py:61-62, modify_model.py:40-41,
sound.py:37,41, dataloading.py:174-175) and the no-CPU-fallback rule: product entry points
raise on CPU tensors instead of computing there."""
import ctypes

import numpy as np
import pytest
import torch

from drsa_audio_amd import _capi


def test_subspace_optimizer_asserts_like_reference():
    from drsa_audio_amd.xai.drsa.drsa import SubspaceOptimizer
    U = torch.eye(8)
    A = torch.rand(10, 8)
    with pytest.raises(AssertionError):
        SubspaceOptimizer(U, A, A, ".", num_concepts=0)
    with pytest.raises(AssertionError):
        SubspaceOptimizer(U, A, A, ".", num_concepts=3)
    with pytest.raises(_capi.DrsaAmdError):
        SubspaceOptimizer(U, A, A, ".", num_concepts=4, device="cpu")


def test_projection_model_layer_range():
    from drsa_audio_amd.model.create_model import VGGType
    from drsa_audio_amd.model.modify_model import ProjectionModel
    m = VGGType(n_filters=(8, 8, 16, 16, 16), n_dense=32, n_classes=2, pool_kernels=((2, 2),) * 5,
                input_size=(64, 64), conv_bn=False, dense_bn=False, block_depth=1)
    for bad in (0, len(m.features)):
        with pytest.raises(ValueError):
            ProjectionModel(m, bad, torch.eye(16), 4)


def test_product_paths_refuse_cpu_tensors():
    from drsa_audio_amd.utils.dataloading import Loader
    from drsa_audio_amd.xai.drsa.preprocessing import normalize_vectors
    from drsa_audio_amd.xai.drsa.drsa import orthogonalize
    ld = Loader("gtzan", device="cpu")
    with pytest.raises(_capi.DrsaAmdError):
        ld.transform_wav(torch.zeros(1, 48000))
    with pytest.raises(_capi.DrsaAmdError):
        normalize_vectors(torch.rand(4, 8))
    with pytest.raises(_capi.DrsaAmdError):
        orthogonalize(torch.eye(8))


def test_lrp_engine_refuses_cpu_model():
    from drsa_audio_amd.model.create_model import VGGType
    from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN
    from drsa_audio_amd.zennit.composites import NameMapComposite
    from drsa_audio_amd.xai.explain.attribute import compute_relevances
    m = VGGType(n_filters=(32, 32, 64, 64, 128), n_dense=128, pool_kernels=((2, 2),) * 5, input_size=(128, 128),
                conv_bn=False, dense_bn=False, block_depth=1).eval()
    with pytest.raises(_capi.DrsaAmdError):
        compute_relevances(m, torch.zeros(1, 1, 128, 128), NameMapComposite(LRP_NAME_MAP_GTZAN), class_idx=0)


def test_get_slice_asserts():
    from drsa_audio_amd.utils.sound import get_slice
    # sound.py:41 compares the start point (seconds) with a sample count, as the reference does
    get_slice(torch.zeros(1, 16000 * 4), 3, 0, 1, 16000)
    with pytest.raises(AssertionError):
        get_slice(torch.zeros(1, 16000 * 4), 3, 17000, 1, 16000)
    with pytest.raises(AssertionError):                      # sound.py:37 not enough audio for 8 chunks
        get_slice(torch.zeros(1, 16000 * 10), 3, 0, 8, 16000)


def test_c_abi_argument_validation_without_gpu():
    lib = _capi.load()
    P = ctypes.c_void_p
    # logmel: null pointers, odd n_fft, frames past the end
    assert lib.drsa_amd_logmel(None, 1, 48000, 1, 0, 48000, 800, 360, 128, 128, 1, None, None, None, None, None, 0,
                               1, 1, -4.0, 1e-7, None, None) == -1
    assert b"null" in lib.drsa_amd_last_error()
    buf = (ctypes.c_float * 4)()
    ib = (ctypes.c_int * 4)()
    p, q = ctypes.cast(buf, P).value, ctypes.cast(ib, P).value
    assert lib.drsa_amd_logmel(p, 1, 48000, 1, 0, 48000, 801, 360, 128, 128, 1, p, q, q, q, p, 1, 1, 1, -4.0, 1e-7,
                               p, None) == -1
    assert lib.drsa_amd_logmel(p, 1, 48000, 1, 0, 48000, 800, 360, 128, 140, 1, p, q, q, q, p, 1, 1, 1, -4.0, 1e-7,
                               p, None) == -1
    assert b"frames" in lib.drsa_amd_last_error()
    # DRSA vectors: bad layout; pooled relevance with an odd map
    assert lib.drsa_amd_drsa_vectors(p, p, None, q, 1, 4, 4, 4, 1, 1, 2, 7, p, p, None) == -1
    assert lib.drsa_amd_drsa_vectors(p, p, q, q, 1, 4, 5, 4, 2, 2, 2, 0, p, p, None) == -1
    # pool kernel must divide the map
    assert lib.drsa_amd_maxpool_capture(p, None, p, q, None, 1, 4, 6, 8, 4, 4, None) == -1
    # Cin = 1 forward: one sample's cout x H x W past 2^31 (32-bit offsets)
    assert lib.drsa_amd_conv_fwd(p, p, p, p, p, q, p, 1, 1, 1 << 16, 256, 256, 1, 1, None) == -1
    assert b"2^31" in lib.drsa_amd_last_error()
    # joint DRSA: no problems
    assert lib.drsa_amd_drsa_run_multi(0, None, 10, 1, None) == -1
    # workspace size query rejects unsupported problems
    assert lib.drsa_amd_drsa_workspace_bytes(100, 48, 5) == 0      # K must divide d
    assert lib.drsa_amd_drsa_workspace_bytes(100, 100, 5) == 0     # padded 5 x 32 > 128
    assert lib.drsa_amd_drsa_workspace_bytes(100, 100, 4) > 0      # VGGish layer 19 (padded to 128)
    assert lib.drsa_amd_drsa_slab_floats(100, 4) == 128 * 128 + 4
    assert lib.drsa_amd_drsa_slab_floats(64, 4) == 64 * 64 + 4
    assert lib.drsa_amd_drsa_workspace_bytes(100, 128, 3) == 0
    # padded size 128 carries the cooperative finish's hand-off area (two 128 x 128 X buffers, the
    # per-workgroup scalars and the ticket) beyond the slabs: at N = 16 (one leaf) the partial slabs,
    # the reduced slab and that area
    slab = 4 * (128 * 128 + 4)
    assert lib.drsa_amd_drsa_workspace_bytes(16, 128, 16) >= 2 * slab + 2 * 128 * 128 * 4
    assert lib.drsa_amd_drsa_workspace_bytes(16, 64, 4) < 2 * 4 * (64 * 64 + 4) + 4096
    # compact den ring backward: pooled W >= 8 (W % 8 == 0) and H >= 2, as the forward's layout needs
    for H, W in ((4, 4), (0, 8), (4, 12)):
        with pytest.raises(_capi.DrsaAmdError, match="pooled H >= 2"):
            _capi.call("drsa_amd_conv_bwd_den_ring", p, None, p, 0, p, p, p, p, 1, 1, 32, 32, H, W, 1, 1, 1e-7, None)


def test_alphabeta_parameter_checks_like_zennit():
    from drsa_audio_amd.zennit.rules import AlphaBeta
    AlphaBeta(2.0, 1.0)
    AlphaBeta(1.0, 0.0)
    for a, b in ((-1.0, -2.0), (1.0, -0.0 - 1.0), (2.0, 0.5), (0.5, 0.0)):
        with pytest.raises(ValueError):
            AlphaBeta(a, b)


def test_coop_status_and_spin_budget_argument_errors():
    """drsa_amd_drsa_coop_status / drsa_amd_debug_coop_spin_budget reject bad arguments before any
    device work (the status itself is read on the GPU: tests/test_drsa_gpu.py)."""
    lib = _capi.lib()
    st = ctypes.c_int(7)
    assert lib.drsa_amd_drsa_coop_status(None, 100, 128, 16, ctypes.addressof(st), None) == _capi.DRSA_EINVAL
    assert lib.drsa_amd_drsa_coop_status(ctypes.c_void_p(16), 100, 128, 3, ctypes.addressof(st), None) == _capi.DRSA_EINVAL
    assert lib.drsa_amd_drsa_coop_status(ctypes.c_void_p(16), 0, 128, 16, ctypes.addressof(st), None) == _capi.DRSA_EINVAL
    assert lib.drsa_amd_debug_coop_spin_budget(-2) == _capi.DRSA_EINVAL
    assert lib.drsa_amd_debug_coop_spin_budget(-1) == 0


# ---------------------------------------------------------------------------------------------
# conv entry points: one row per argument check of csrc/lrp_conv.hip.  Every row starts from a
# valid call of that entry point (64 -> 64 channels, 8 x 32 map, batch 2; never launched here: only
# the changed argument differs, and it is rejected before any device work) and names the argument
# it breaks, the expected code and a substring of the message.
# ---------------------------------------------------------------------------------------------
_PTR = {k: 0x10000 * (i + 1) for i, k in enumerate(
    ("in", "g", "g_amax", "wts", "bias", "x", "den", "den_map", "den_ring", "den_const4", "out", "out_amax", "out_den"))}
_CONV_ORDER = {
    "conv_fwd": "in wts bias den_map out out_amax out_den B cin cout H W ng pool stream",
    "conv_fwd_bf16": "in wts bias den_map out out_amax out_den B cin cout H W ng pool stream",
    "conv_fwd_den_ring": "in wts bias den_map out out_amax den_ring B cout H W ng stream",
    "conv_bwd": "g g_amax wts x den out Bq clones cin cout H W ng xmode post eps stream",
    "conv_bwd_bf16": "g g_amax wts x den out Bq clones cin cout H W ng xmode post eps stream",
    "conv_bwd_bf16_pw": "g g_amax pool_w wts x den out Bq clones cin cout H W xmode post eps stream",
    "conv_bwd_den_map": "g g_amax pool_w wts wts_bf16 x den_map out Bq clones cin cout H W ng xmode eps stream",
    "conv_bwd_den_ring": "g g_amax wts wts_bf16 x den_ring den_const4 out Bq clones cin cout H W ng xmode eps stream",
}
_CONV_VALID = dict(_PTR, B=2, Bq=2, clones=1, cin=64, cout=64, H=8, W=32, ng=1, pool=1, pool_w=2, wts_bf16=0,
                   xmode=1, post=1, eps=1e-6, stream=None)
_E, _U = _capi.DRSA_EINVAL, _capi.DRSA_EUNSUPPORTED
_FWDS, _BWDS = ("conv_fwd", "conv_fwd_bf16"), ("conv_bwd", "conv_bwd_bf16", "conv_bwd_bf16_pw", "conv_bwd_den_map",
                                               "conv_bwd_den_ring")
_CONV_REJECTIONS = (
    # forward, fp32 and bf16 weights
    *[(e, ch, _E, msg) for e in _FWDS for ch, msg in (
        (dict(B=0), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"),
        (dict(ng=0), "ng must be 1..3"), (dict(ng=4), "ng must be 1..3"),
        (dict(H=7), "H and W must be even (got 7x32)"), (dict(W=31), "H and W must be even (got 8x31)"),
        (dict(pool=-1), "pool must be 0"), (dict(pool=3), "pool must be 0"),
        (dict(out_amax=None), "pool needs out_amax"),
        (dict(pool=0, W=6), "unpooled output needs W % 4 == 0"),
        (dict(pool=2, W=6), "2x4 pool needs W % 4 == 0 (got W=6)"))],
    ("conv_fwd_bf16", dict(cin=1), _E, "cin = 1 runs on drsa_amd_conv_fwd"),
    ("conv_fwd_bf16", dict(wts=_PTR["wts"] + 8), _E, "16-byte aligned"),
    ("conv_fwd", dict(cin=128, cout=32), _U, "no kernel for cin=128 cout=32 W=32"),
    ("conv_fwd_bf16", dict(cin=128, cout=32), _U, "no kernel for cin=128 cout=32 W=32"),
    # the den-ring first-layer forward
    *[("conv_fwd_den_ring", {k: None}, _E, "null pointer") for k in ("in", "wts", "den_map", "out", "out_amax", "den_ring")],
    *[("conv_fwd_den_ring", ch, _E, "needs H >= 4 even and W % 16 == 0 (got") for ch in (
        dict(B=0), dict(H=2), dict(H=7), dict(W=0), dict(W=24))],
    ("conv_fwd_den_ring", dict(ng=0), _E, "ng must be 1..3"), ("conv_fwd_den_ring", dict(ng=4), _E, "ng must be 1..3"),
    # every backward
    *[(e, ch, _E, "bad batch/clones") for e in _BWDS for ch in (dict(Bq=0), dict(clones=0), dict(Bq=3, clones=2))],
    *[(e, ch, _E, "W % 4 == 0") for e in _BWDS[:4] for ch in (dict(H=7), dict(W=30))],
    *[(e, ch, _E, "H must be even and W % 4 == 0 (got") for e in ("conv_bwd", "conv_bwd_bf16", "conv_bwd_den_map")
      for ch in (dict(H=7), dict(W=30))],
    *[(e, dict(x=None, post=0), _E, "xmode needs x") for e in _BWDS[:3]],
    *[(e, ch, _E, "POST_DIV needs x and den") for e in _BWDS[:3] for ch in (
        dict(x=None, xmode=0), dict(den=None), dict(x=None, xmode=0, post=2))],
    *[(e, dict(cin=32, cout=64), _U, "no kernel for cin=32 cout=64 W=32") for e in _BWDS if e != "conv_bwd_bf16_pw"],
    # fp32 weights
    ("conv_bwd", dict(ng=0), _E, "ng must be 1..2"), ("conv_bwd", dict(ng=3), _E, "ng must be 1..2"),
    # bf16 weights
    ("conv_bwd_bf16", dict(ng=2), _E, "the Gamma x-/W- term is for the fp32 first layer"),
    ("conv_bwd_bf16", dict(cin=8), _E, "cin >= 16"), ("conv_bwd_bf16_pw", dict(cin=8), _E, "cin >= 16"),
    ("conv_bwd_bf16", dict(wts=_PTR["wts"] + 8), _E, "16-byte aligned"),
    ("conv_bwd_bf16_pw", dict(wts=_PTR["wts"] + 8), _E, "16-byte aligned"),
    *[(e, dict(wts_bf16=1, **ch), _E, msg) for e in ("conv_bwd_den_map", "conv_bwd_den_ring") for ch, msg in (
        (dict(ng=2), "bf16 weights need ng == 1"), (dict(cin=8), "cin >= 16"),
        (dict(wts=_PTR["wts"] + 8), "16-byte align"))],
    # g at 2 x pool_w resolution
    *[("conv_bwd_bf16_pw", ch, _E, "needs g_amax and pool_w 2 or 4") for ch in (
        dict(g_amax=None), dict(pool_w=0), dict(pool_w=3))],
    ("conv_bwd_bf16_pw", dict(pool_w=4, cin=32, cout=32), _U, "no kernel for cin=32 cout=32 W=32"),
    # the shared den map
    ("conv_bwd_den_map", dict(x=None), _E, "needs x and den"), ("conv_bwd_den_map", dict(den_map=None), _E, "needs x and den"),
    ("conv_bwd_den_map", dict(pool_w=3), _E, "pool_w must be 2 or 4"),
    ("conv_bwd_den_map", dict(xmode=3), _E, "bad xmode"), ("conv_bwd_den_map", dict(xmode=-1), _E, "bad xmode"),
    ("conv_bwd_den_map", dict(ng=0), _E, "1..2"), ("conv_bwd_den_map", dict(ng=3), _E, "1..2"),
    ("conv_bwd_den_map", dict(ng=2, pool_w=4), _E, "ng 1 under a 2x4 pool"),
    ("conv_bwd_den_map", dict(pool_w=4, W=8), _E, "2x4 pool-sparse g needs W / 4 % 4 == 0 (got W=8)"),
    # the compact den ring
    *[("conv_bwd_den_ring", {k: None}, _E, "needs x, den_ring and den_const4") for k in ("x", "den_ring", "den_const4")],
    *[("conv_bwd_den_ring", ch, _E, "needs pooled H >= 2 and W >= 8, W % 8 == 0 (got") for ch in (
        dict(H=1), dict(W=4), dict(W=12))],
    ("conv_bwd_den_ring", dict(xmode=3), _E, "bad xmode"),
    ("conv_bwd_den_ring", dict(den_const4=_PTR["den_const4"] + 4), _E, "den_const4 must be 16-byte aligned"),
    ("conv_bwd_den_ring", dict(ng=0), _E, "ng must be 1..2"), ("conv_bwd_den_ring", dict(ng=3), _E, "ng must be 1..2"),
    # launch: one sample's planes are addressed with 32-bit offsets
    *[(e, dict(cin=128, cout=128, H=4096, W=4096), _E, "conv: one sample's channels x H x W must stay below 2^31")
      for e in _FWDS + ("conv_bwd", "conv_bwd_bf16", "conv_bwd_den_map", "conv_bwd_den_ring")],
    ("conv_fwd_den_ring", dict(cout=128, H=4096, W=4096), _E, "2^31"),
)


def _conv_call(entry, changes):
    args = dict(_CONV_VALID, **changes)
    rc = getattr(_capi.lib(), "drsa_amd_" + entry)(*[args[k] for k in _CONV_ORDER[entry].split()])
    return rc, _capi.lib().drsa_amd_last_error().decode()


@pytest.mark.parametrize("entry,changes,code,needle", _CONV_REJECTIONS,
                         ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c, _, _ in _CONV_REJECTIONS])
def test_conv_entry_points_reject_bad_arguments(entry, changes, code, needle):
    rc, msg = _conv_call(entry, changes)
    assert rc == code, (rc, msg)
    assert needle in msg, msg
    # the message names its entry point (the 32-bit-offset limit is checked in the shared launch)
    assert msg.startswith(entry + ":") or needle.startswith("conv:") or "2^31" in needle, msg


def test_conv_rejection_table_covers_every_entry_point():
    """Each launching conv entry point has rows, and all but the den-ring forward (Cin = 1 kernel,
    no table lookup) have their "no kernel" row."""
    assert {e for e, *_ in _CONV_REJECTIONS} == set(_CONV_ORDER)
    assert {e for e, _, c, _ in _CONV_REJECTIONS if c == _U} == set(_CONV_ORDER) - {"conv_fwd_den_ring"}


# ---------------------------------------------------------------------------------------------
# dense head (csrc/linear.hip): one row per argument check, from a valid call (never launched here)
# ---------------------------------------------------------------------------------------------
_LIN_ORDER = {
    "linear_fwd": "x W bias z_out relu_out M N K stream",
    "linear_bwd": "R seed_cls one_hot z relu_mask rule_eps eps W x xmode den post eps_post out M Nout Kin stream",
}
_LIN_VALID = dict({k: 0x10000 * (i + 1) for i, k in enumerate(("x", "W", "bias", "z_out", "relu_out", "R", "z", "den", "out"))},
                  seed_cls=None, one_hot=0, relu_mask=1, rule_eps=1, eps=1e-6, xmode=_capi.XM_MUL, post=_capi.POST_DIV,
                  eps_post=1e-6, M=4, N=8, K=16, Nout=8, Kin=16, stream=None)
_LIN_REJECTIONS = (
    ("linear_fwd", dict(M=0), "bad shape"),
    *[("linear_fwd", {k: None}, "x, W and z_out are required") for k in ("x", "W", "z_out")],
    ("linear_bwd", dict(Kin=0), "bad shape"),
    ("linear_bwd", dict(R=None), "need R or a seed"),
    *[("linear_bwd", {k: None}, "z, W and out are required") for k in ("z", "W", "out")],
    *[("linear_bwd", dict(xmode=v), "xmode must be XM_NONE or XM_MUL") for v in (_capi.XM_SPLIT, -1)],
    *[("linear_bwd", dict(post=v), "post must be POST_NONE, POST_DIV or POST_MASK") for v in (_capi.POST_DIV_RING, -1)],
    ("linear_bwd", dict(x=None, post=_capi.POST_NONE), "xmode needs x"),
    ("linear_bwd", dict(den=None), "POST_DIV needs x and den"),
    ("linear_bwd", dict(x=None, xmode=_capi.XM_NONE, post=_capi.POST_MASK), "POST_DIV needs x and den"),
)


@pytest.mark.parametrize("entry,changes,needle", _LIN_REJECTIONS,
                         ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c, _ in _LIN_REJECTIONS])
def test_dense_entry_points_reject_bad_arguments(entry, changes, needle):
    args = dict(_LIN_VALID, **changes)
    rc = getattr(_capi.lib(), "drsa_amd_" + entry)(*[args[k] for k in _LIN_ORDER[entry].split()])
    msg = _capi.lib().drsa_amd_last_error().decode()
    assert rc == _capi.DRSA_EINVAL, (rc, msg)
    assert msg.startswith(entry + ":") and needle in msg, msg
