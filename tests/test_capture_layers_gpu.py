"""DRSA data of several layers from one LRP pass (GPU): drsa_amd_relevance_post, LRPEngine.capture_many and the
public functions over it (get_intermediates, preprocess_data_layers, drsa_training_data_layers, make_datasets).

The contract is equality with the single-layer path, bit for bit: the multi-layer pass keeps more stages unfused
in the forward and takes the post step of every tapped stage out of the conv epilogue into a launch of its own,
and neither may change a bit of any layer's activations, relevances or sampled vectors, nor the numpy stream.
"""
import copy
import socket

import numpy as np
import pytest
import torch

import lrp_ref
from lrp_common import gtzan128, logmel, spec, toy, vggish
from drsa_audio_amd import _capi
from drsa_audio_amd._capi import DRSA_EINVAL, POST_DIV, POST_MASK
from drsa_audio_amd.engine import get_engine
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_GTZAN, LRP_NAME_MAP_TOY, LRP_NAME_MAP_VGGISH
from drsa_audio_amd.xai.drsa.preprocessing import (drsa_training_data, drsa_training_data_layers, get_intermediates,
                                                   preprocess_data, preprocess_data_layers)
from drsa_audio_amd.zennit.canonizers import SequentialMergeBatchNorm
from drsa_audio_amd.zennit.composites import NameMapComposite
from drsa_audio_amd.zennit.rules import AlphaBeta

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------- the kernel alone
def _post_case(n, clones, seed):
    """R [2 * clones][n], x and den [2][n]: den with both zeros, both signs, tiny and subnormal values, x with
    zeros and negatives."""
    g = torch.Generator().manual_seed(seed)
    Bq = 2 * clones
    R = torch.randn(Bq, n, generator=g)
    x = torch.randn(2, n, generator=g)
    x[torch.rand(2, n, generator=g) < 0.25] = 0.0
    den = torch.randn(2, n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 5e-8, -5e-8, 1e-7, -1e-7])
    pick = torch.rand(2, n, generator=g) < 0.5
    den[pick] = special[torch.randint(0, len(special), (int(pick.sum()),), generator=g)]
    x.view(-1)[0] = 1.0                       # n = 1: one row is sure to pass the mask
    return R, x, den


def _post_ref(R, x, den, clones, post, eps):
    xr, dr = x.repeat_interleave(clones, 0), den.repeat_interleave(clones, 0)
    if post == POST_MASK:
        return torch.where(xr > 0, R, torch.zeros(()))
    return torch.where(xr > 0, R / (dr + torch.where(dr >= 0, eps, -eps)), torch.zeros(()))


def _post_run(R, x, den, out, clones, post, eps):
    _capi.call("drsa_amd_relevance_post", R.data_ptr(), x.data_ptr(), _capi.ptr(den), out.data_ptr(), R.size(0),
               clones, R.size(1), post, eps, _capi.stream_ptr(DEV))
    torch.cuda.synchronize()


@pytest.mark.parametrize("post", [POST_DIV, POST_MASK])
@pytest.mark.parametrize("clones", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 1028])
def test_relevance_post_kernel_bitwise(n, clones, post):
    """n = 4 / 1028 take the float4 path when every pointer is aligned (1028 over several blocks), the others the
    scalar path; an R offset by one float takes the scalar path at every n; out = R is allowed."""
    _capi.load()
    eps = 1e-7
    R, x, den = _post_case(n, clones, 100 * n + clones)
    ref = _post_ref(R, x, den, clones, post, torch.tensor(eps))
    Rd, xd, dd = R.to(DEV), x.to(DEV), den.to(DEV)
    out = torch.full_like(Rd, float("nan"))
    _post_run(Rd, xd, dd if post == POST_DIV else None, out, clones, post, eps)
    assert torch.equal(_bits(out.cpu()), _bits(ref))
    assert torch.equal(Rd.cpu(), R)                                   # R is left as it was
    # an unaligned R (a slice offset by one float), written in place
    buf = torch.empty(R.numel() + 1, device=DEV)
    Ru = buf[1:].view_as(Rd)
    Ru.copy_(Rd)
    assert Ru.data_ptr() % 16 == 4
    _post_run(Ru, xd, dd, Ru, clones, post, eps)
    assert torch.equal(_bits(Ru.cpu()), _bits(ref))
    # in place on the aligned tensor
    _post_run(Rd, xd, dd, Rd, clones, post, eps)
    assert torch.equal(_bits(Rd.cpu()), _bits(ref))


def test_relevance_post_bad_arguments():
    fn, s = _capi.load().drsa_amd_relevance_post, _capi.stream_ptr(DEV)
    R, x, den, out = (torch.ones(6, 8, device=DEV) for _ in range(4))
    p = [t.data_ptr() for t in (R, x, den, out)]
    assert fn(*p, 6, 3, 8, POST_DIV, 1e-7, s) == 0
    assert fn(p[0], p[1], None, p[3], 6, 3, 8, POST_MASK, 0.0, s) == 0
    for post in (0, 3, 4, -1):
        assert fn(*p, 6, 3, 8, post, 1e-7, s) == DRSA_EINVAL
        assert b"post" in _capi.lib().drsa_amd_last_error()
    for bad in ((None, p[1], p[2], p[3]), (p[0], None, p[2], p[3]), (p[0], p[1], None, p[3]), (p[0], p[1], p[2], None)):
        assert fn(*bad, 6, 3, 8, POST_DIV, 1e-7, s) == DRSA_EINVAL
        assert b"null" in _capi.lib().drsa_amd_last_error()
    for Bq, clones, n in ((6, 4, 8), (0, 1, 8), (6, 0, 8), (6, 3, 0), (-3, 3, 8)):
        assert fn(*p, Bq, clones, n, POST_DIV, 1e-7, s) == DRSA_EINVAL
        assert b"shape" in _capi.lib().drsa_amd_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ the models
def _vcomp():
    return NameMapComposite(LRP_NAME_MAP_VGGISH, canonizers=[SequentialMergeBatchNorm()])


@pytest.fixture(scope="module")
def vgg64():
    return vggish(input_size=(64, 128)).to(DEV), _vcomp()


@pytest.fixture(scope="module")
def gtzan():
    return gtzan128().to(DEV), NameMapComposite(LRP_NAME_MAP_GTZAN)


def test_oracle_anchor_vggish_three_layers():
    net = vggish(input_size=(32, 128))
    x = logmel(2, 32, 128, seed=4)
    got = get_intermediates(copy.deepcopy(net).to(DEV), x.to(DEV), _vcomp(), [19, 26, 33], 1)
    assert list(got) == [19, 26, 33]
    merged = lrp_ref.merge_batch_norm(net)
    for layer in (19, 26, 33):
        _, _, (act, rel) = lrp_ref.lrp(merged, spec(LRP_NAME_MAP_VGGISH), x, class_idx=1, mode="exact",
                                       capture=f"features.{layer}")
        assert torch.equal(got[layer][0].cpu(), act), layer
        assert torch.equal(got[layer][1].cpu(), rel), layer


def _same_as_single(model, comp, x, layers, L, layout=0, chunk=2):
    """preprocess_data_layers against one preprocess_data call per layer, in A, in C and in the numpy stream."""
    np.random.seed(5)
    one = {layer: preprocess_data(model, x, comp, layer, 1, num_locations=L, attr_batch_size=chunk, layout=layout)
           for layer in layers}
    state_one = np.random.get_state()
    np.random.seed(5)
    many = preprocess_data_layers(model, x, comp, layers, 1, num_locations=L, attr_batch_size=chunk, layout=layout)
    state_many = np.random.get_state()
    assert list(many) == list(layers)
    for layer in layers:
        for got, want in zip(many[layer], one[layer]):
            assert got.shape == want.shape and torch.isfinite(want).all()
            assert torch.equal(_bits(got), _bits(want)), layer
    assert state_one[0] == state_many[0] and np.array_equal(state_one[1], state_many[1])
    assert state_one[2:] == state_many[2:]
    return many


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("layers", [[19, 26, 33], [33, 19, 26], [16, 19, 20], [26]])
def test_vggish_equals_single_layer_calls(vgg64, layers, layout):
    x = logmel(3, 64, 128, seed=7).to(DEV)
    many = _same_as_single(*vgg64, x, layers, 4, layout)
    assert all(A.shape[0] == 3 * 4 and A.abs().sum() > 0 and C.abs().sum() > 0 for A, C in many.values())


@pytest.mark.parametrize("layout", [0, 1])
def test_gtzan_equals_single_layer_calls(gtzan, layout):
    _same_as_single(*gtzan, logmel(3, seed=8).to(DEV), [4, 7, 8, 13], 4, layout)


def test_toy_all_locations_equals_single_layer_calls():
    _same_as_single(toy().to(DEV), NameMapComposite(LRP_NAME_MAP_TOY), logmel(3, 64, 64, seed=9).to(DEV), [4, 7], None)


def test_capture_many_one_layer_equals_capture(gtzan):
    model, comp = gtzan
    eng, x = get_engine(model, comp), logmel(2, seed=10).to(DEV)
    cls = torch.full((2,), 1, dtype=torch.int32, device=DEV)
    for name in ("features.7", "features.8"):
        one = {k: v.clone() if torch.is_tensor(v) else v for k, v in eng.capture(x, name, cls=cls).items()}
        many = eng.capture_many(x, [name], cls=cls)
        assert list(many) == [name] and many[name].keys() == one.keys()
        for k, v in one.items():
            assert torch.equal(many[name][k], v) if torch.is_tensor(v) else many[name][k] == v, (name, k)
    with pytest.raises(ValueError, match="twice"):
        eng.capture_many(x, ["features.7", "features.7"], cls=cls)


def test_alphabeta_between_taps():
    comp = NameMapComposite([(n, AlphaBeta(alpha=2.0, beta=1.0) if n == ["features.6"] else r)
                             for n, r in LRP_NAME_MAP_GTZAN])
    _same_as_single(gtzan128().to(DEV), comp, logmel(3, seed=11).to(DEV), [4, 10], 4)


def test_one_pass_launches(vgg64):
    """One chunk of [19, 26, 33]: every conv forward once, every conv backward above layer 19 once, two tap_post
    launches, and nothing at or below the stage of layer 19."""
    model, comp = vgg64
    eng = get_engine(model, comp)
    x = logmel(2, 64, 128, seed=12).to(DEV)
    eng.trace = []
    try:
        preprocess_data_layers(model, x, comp, [19, 26, 33], 1, num_locations=4)
        torch.cuda.synchronize()
        tags = [t for t, _, _ in eng.trace]
    finally:
        eng.trace = None
    low = eng.capture_stage("features.19")[0]
    fwd = [t for t in tags if t.startswith("conv_fwd:")]
    assert sorted(fwd) == sorted(f"conv_fwd:{st.name}" for st in eng.stages)
    bwd = [t for t in tags if t.startswith("conv_bwd:") or t.startswith("first_layer_bwd:")]
    assert bwd == [f"conv_bwd:{st.name}" for st in reversed(eng.stages[low + 1:])]
    assert [t for t in tags if t.startswith("tap_post:")] == ["tap_post:features.34", "tap_post:features.27"]
    assert sum(t.startswith("linear_bwd:") for t in tags) == len(eng.dense)
    assert sum(t.startswith("linear_fwd:") for t in tags) == len(eng.dense)


def test_bf16_plan_equals_single_layer_calls():
    """The bf16 plan: the forward convs run on bf16 operands in the fused and in the unfused form alike, so the
    multi-layer pass must still equal the single-layer calls bit for bit."""
    model = gtzan128().to(DEV).bfloat16()
    comp = NameMapComposite(LRP_NAME_MAP_GTZAN)
    assert get_engine(model, comp).precision == "bf16"
    _same_as_single(model, comp, logmel(3, seed=13).to(DEV), [4, 7, 13], 4)


def test_training_data_layers(gtzan):
    import torch.distributed as dist
    model, comp = gtzan
    x, layers = logmel(3, seed=14).to(DEV), [7, 4, 13]

    def both(group):
        np.random.seed(5)
        one = {layer: drsa_training_data(model, x, comp, layer, 2, num_locations=4, attr_batch_size=2, group=group)
               for layer in layers}
        np.random.seed(5)
        many = drsa_training_data_layers(model, x, comp, layers, 2, num_locations=4, attr_batch_size=2, group=group)
        assert list(many) == layers
        for layer in layers:
            for got, want in zip(many[layer], one[layer]):
                assert torch.isfinite(want).all() and torch.equal(_bits(got), _bits(want)), layer
        return many

    plain = both(None)
    made = not dist.is_initialized()
    if made:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        group = dist.new_group(ranks=[dist.get_rank()], backend="gloo")
        grouped = both(group)
    finally:
        if made:
            dist.destroy_process_group()
    # a world of one normalises over the same rows (the grouped reduction is its own kernel pair: 1 ulp)
    for layer in layers:
        for got, want in zip(grouped[layer], plain[layer]):
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-6, atol=1e-7)


def test_make_datasets(gtzan, tmp_path):
    from drsa_audio_amd.xai.drsa.cluster.getdrsadata import load_and_normalize_data, make_datasets
    from drsa_audio_amd.xai.drsa.cluster.optsubspaces import optimize_grid
    model, comp = gtzan
    batches = {"blues": (logmel(2, seed=15).to(DEV), 0), "disco": (logmel(2, seed=16).to(DEV), 3)}
    np.random.seed(5)
    raw = make_datasets(model, batches, comp, [7, 13], num_locations=4)
    np.random.seed(5)
    data = make_datasets(model, batches, comp, [7, 13], num_locations=4, output_path=str(tmp_path), normalize=True)
    assert list(data) == [("blues", 7), ("blues", 13), ("disco", 7), ("disco", 13)] == list(raw)
    for (name, layer), (A, C) in data.items():
        assert A.shape == C.shape == (8, 64 if layer == 7 else 128)
        a, c = load_and_normalize_data(str(tmp_path / "gtzan" / "bn" / name / f"dataset_layer{layer}.pkl"), DEV)
        np.testing.assert_allclose(a.cpu().numpy(), A.cpu().numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(c.cpu().numpy(), C.cpu().numpy(), rtol=2e-6, atol=1e-7)
        # the unnormalised return is what one preprocess_data call per layer gives
        assert float(raw[(name, layer)][0].abs().max()) > 0
    np.random.seed(5)
    for name, (xb, cls) in batches.items():
        for layer in (7, 13):
            A, C = preprocess_data(model, xb, comp, layer, cls, num_locations=4)
            assert torch.equal(A, raw[(name, layer)][0]) and torch.equal(C, raw[(name, layer)][1])
    res = optimize_grid(data, None, steps=2, runs=1)
    assert sorted(res) == [(name, layer, 1) for name in ("blues", "disco") for layer in (7, 13)]
    assert all(np.isfinite(v["objective"]) for v in res.values())
