"""PRCA on the GPU (xai/drsa/prca.py, csrc/prca.hip) against the float64 oracle of prca_ref.py.

Tolerances: the covariance keeps the project's kernel gate (2e-5 of the sum of |terms|);
orthogonality keeps test_orthogonalize_api's 5e-6 (the finish is the same polar); every other
eigensolver figure is allowed 4 x the error of prca_ref.jacobi_model_fp32 on the same matrix,
floored at 8 * 2^-24 (prca_ref.allowance).  Each test prints its figures before it asserts."""
import copy
import os

import numpy as np
import pytest
import torch

import prca_ref as R
from lrp_common import logmel, toy
from drsa_audio_amd.utils.constants import LRP_NAME_MAP_TOY
from drsa_audio_amd.utils.synthetic import drsa_inputs
from drsa_audio_amd.xai.drsa import prca

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COV_SHAPES = [(1, 1), (15, 3), (16, 16), (17, 25), (255, 64), (4101, 100), (4133, 128)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


# ------------------------------------------------------------------------------------- 1. covariance
@pytest.mark.parametrize("N,d", COV_SHAPES)
def test_covariance_against_float64(N, d):
    A, C = drsa_inputs(N, d, seed=7 + d)
    assert A.min() >= 0                               # DRSA's inputs: A post-ReLU-like, C signed
    Ad, Cd = _dev(A), _dev(C)
    M = prca.relevance_covariance(Ad, Cd)
    M64, S = R.relevance_covariance(A, C), R.covariance_scale(A, C)
    err = np.abs(M.cpu().numpy().astype(np.float64) - M64)
    print(f"N={N} d={d} max err / scale = {float((err / S).max()):.3e}")
    assert M.shape == (d, d) and (err <= 2e-5 * S).all()
    assert torch.equal(M, M.T)
    assert torch.equal(M, prca.relevance_covariance(Ad, Cd))
    if N >= 2:   # the sharding identity: slabs of row shards add up
        n1 = max(1, N // 3)
        slab = prca.relevance_covariance_partial(Ad[:n1], Cd[:n1]) + prca.relevance_covariance_partial(Ad[n1:], Cd[n1:])
        Ms = prca.relevance_covariance_finish(slab, N)
        errs = np.abs(Ms.cpu().numpy().astype(np.float64) - M64)
        print(f"  sharded at {n1}: {float((errs / S).max()):.3e}")
        assert (errs <= 2e-5 * S).all() and torch.equal(Ms, Ms.T)


# ---------------------------------------------------------------------------- 2. syevj known answers
def _sign_rule_holds(V: np.ndarray) -> bool:
    idx = np.argmax(np.abs(V), axis=0)
    return bool((V[idx, np.arange(V.shape[1])] > 0).all())


def test_syevj_known_answers():
    w, V, sweeps = prca.eigh_descending(_dev(np.diag(np.arange(-3.0, 5.0))), return_sweeps=True)
    w, V = w.cpu().numpy(), V.cpu().numpy()
    assert sweeps == 1 and np.array_equal(w, np.arange(4.0, -4.0, -1.0))
    assert np.array_equal(np.abs(V), np.eye(8)[:, ::-1]) and _sign_rule_holds(V)     # a signed permutation
    w, V = prca.eigh_descending(torch.zeros(5, 5, device=DEV))
    assert np.array_equal(w.cpu().numpy(), np.zeros(5))
    V = V.cpu().numpy().astype(np.float64)
    assert np.abs(V.T @ V - np.eye(5)).max() < 5e-6
    w, V, sweeps = prca.eigh_descending(_dev([[0.0, 1.0], [1.0, 0.0]]), return_sweeps=True)   # zero diagonal: must rotate
    print("[[0,1],[1,0]]:", w.cpu().numpy(), sweeps)
    assert np.abs(w.cpu().numpy().astype(np.float64) - [1.0, -1.0]).max() <= R.FLOOR and sweeps == 2
    V = V.cpu().numpy().astype(np.float64)
    assert np.abs(np.abs(V) - np.sqrt(0.5)).max() <= R.FLOOR and _sign_rule_holds(V)
    w, V = prca.eigh_descending(_dev([[-2.5]]))                                      # d = 1
    assert w.cpu().numpy().tolist() == [-2.5] and V.cpu().numpy().tolist() == [[1.0]]
    # the upper triangle is what is read
    Mu = R.make_matrix("separated", 16)
    a = prca.eigh_descending(_dev(Mu))
    b = prca.eigh_descending(_dev(np.triu(Mu) + 7.0 * np.tril(np.ones_like(Mu), -1)))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_syevj_ends_on_non_finite_input():
    M = R.make_matrix("separated", 17).copy()
    M[3, 5] = M[5, 3] = np.nan
    w, V, sweeps = prca.eigh_descending(_dev(M), return_sweeps=True)
    torch.cuda.synchronize()
    assert 1 <= sweeps <= R.MAX_SWEEPS and w.shape == (17,)


# -------------------------------------------------------------------------- 3. syevj against float64
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("d", R.D_SIZES)
def test_syevj_against_float64(family, d):
    M32, model, model_sweeps = R.model_case(family, d)
    Md = _dev(M32)
    w, V, sweeps = prca.eigh_descending(Md, return_sweeps=True)
    w2, V2 = prca.eigh_descending(Md)
    k_list, top = R.check_lists(family, d)
    got = R.eig_errors(M32, w.cpu().numpy(), V.cpu().numpy(), k_list, top)
    print(f"{family} d={d} sweeps gpu/model {sweeps}/{model_sweeps}")
    for key in got:
        print(f"  {key}: gpu {got[key]:.3e} model {model[key]:.3e} allowed "
              f"{5e-6 if key == 'orth' else R.allowance(model[key]):.3e}")
    assert got["orth"] < 5e-6
    for key in got:
        if key != "orth":
            assert got[key] <= R.allowance(model[key]), key
    wn = w.cpu().numpy()
    assert (wn[:-1] >= wn[1:]).all()
    assert _sign_rule_holds(V.cpu().numpy())
    assert 1 <= sweeps <= R.MAX_SWEEPS
    assert torch.equal(w, w2) and torch.equal(V, V2)


# ------------------------------------------------------------------------------ 4. prca end to end
def _planted(N, d, seed):
    rng = np.random.default_rng(seed)
    P, _ = np.linalg.qr(rng.standard_normal((N, d)))
    Q = R._orthogonal(d, rng)
    lam = np.linspace(1.0, -1.0, d)
    A = (np.sqrt(N) * P @ Q.T).astype(np.float32)
    C = (A.astype(np.float64) @ (Q * lam[None, :]) @ Q.T).astype(np.float32)
    return A, C, lam


@pytest.mark.parametrize("d,K", [(25, 5), (64, 4)])
def test_prca_planted_spectrum(d, K):
    """M = Q diag(lambda) Q^T in exact arithmetic.  Against float64 eigh of the float64 M of the
    fp32-cast inputs the result carries two errors: the covariance's (elementwise within the project's
    gate 2e-5 * S, so ||dM||_2 <= ||dM||_F <= 2e-5 ||S||_F) moves eigenvalues by at most ||dM||_2
    (Weyl) and a spectral projector by at most ||dM||_2 / (gap - ||dM||_2) (Davis-Kahan), and the
    eigensolver's own, allowed as in test 3 from the model on the float32 cast of M."""
    from scipy.stats import ortho_group
    from drsa_audio_amd.xai.explain.explainer import compute_subspace_relevances
    N = 512
    A, C, lam = _planted(N, d, seed=d)
    Ad, Cd = _dev(A), _dev(C)
    U, w = prca.prca(Ad, Cd)
    M64 = R.relevance_covariance(A, C)
    w64, V64 = R.eigh_descending(M64)
    nrm = float(np.abs(w64).max())
    assert np.abs(w64 - lam).max() < 1e-5                                  # the planted spectrum is there
    dM = 2e-5 * float(np.linalg.norm(R.covariance_scale(A, C)))
    wm, Vm, _ = R.jacobi_model_fp32(M64.astype(np.float32))
    me = R.eig_errors(M64.astype(np.float32), wm, Vm, k_list=(1, d // 4))
    Un, wn = U.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    gap = 2.0 / (d - 1)
    e_w = float(np.abs(wn - w64).max())
    print(f"d={d}: |w - w64| = {e_w:.3e} (allowed {dM + R.allowance(me['eig']) * nrm:.3e})")
    assert e_w <= dM + R.allowance(me["eig"]) * nrm
    for k in (1, d // 4):
        e_p = float(np.abs(R.projector(Un, k) - R.projector(V64, k)).max())
        allowed = dM / (gap - dM) + R.allowance(me[f"proj{k}"])
        print(f"  projector k={k}: {e_p:.3e} (allowed {allowed:.3e})")
        assert e_p <= allowed
        np.random.seed(100 + k)
        obj = np.trace(Un[:, :k].T @ M64 @ Un[:, :k])
        for _ in range(5):
            B = ortho_group.rvs(d)[:, :k]
            assert obj >= np.trace(B.T @ M64 @ B)
    # an independently written kernel: the relevance of concept block k is N * (sum of w over the block)
    Rk = compute_subspace_relevances(Ad[None], Cd[None], U, K)[0].cpu().numpy().astype(np.float64)
    terms = np.abs((A.astype(np.float64) @ Un) * (C.astype(np.float64) @ Un)).reshape(N, K, d // K).sum((0, 2)) / N
    blocks = wn.reshape(K, d // K).sum(1)
    print("  block relevance / N - block sum of w, over 2e-5 sum|terms|:", np.abs(Rk / N - blocks) / (2e-5 * terms))
    assert (np.abs(Rk / N - blocks) <= 2e-5 * terms).all()
    assert (Rk[:-1] >= Rk[1:]).all()


# ---------------------------------------------------------------------- 5. integration on the toy net
@pytest.fixture(scope="module")
def toy_case():
    from drsa_audio_amd.xai.drsa.preprocessing import preprocess_data
    from drsa_audio_amd.zennit.composites import NameMapComposite
    net = toy(3)
    m = copy.deepcopy(net).to(DEV).eval()
    x = logmel(4, 64, 64, seed=43).to(DEV)            # 2 classes x 2 samples
    A, C = preprocess_data(m, x[2:], NameMapComposite(LRP_NAME_MAP_TOY), 7, 1, device=DEV)
    d = A.size(-1)
    return m, x, A.reshape(-1, d).contiguous(), C.reshape(-1, d).contiguous()


def test_prca_basis_drives_the_heatmap_generator(toy_case):
    from drsa_audio_amd.xai.explain.explainer import HeatmapGenerator
    m, x, A, C = toy_case
    U = prca.prca(A, C)[0]
    hg = HeatmapGenerator(m, U, LRP_NAME_MAP_TOY, "class2", num_concepts=4, layer_idx=7, device=DEV, standard="clone")
    hg.generate_subspace_heatmaps(x[2:], to_host=False)
    out = hg.info_device
    std = out["standard_heatmaps"][:, 0].double()
    s = out["subspace_heatmaps"].double().sum(1)
    scale = std.abs().amax(dim=(1, 2), keepdim=True)
    err = float(((s - std).abs() / scale).max())
    print("sum of concept heatmaps vs standard:", err)
    assert out["subspace_heatmaps"].shape == (2, 4, 64, 64) and err < 1e-4
    assert torch.isfinite(out["subspace_heatmaps"]).all()


def test_prca_main_writes_the_drsa_layout(toy_case, tmp_path):
    from drsa_audio_amd.utils.evaluation import get_best_run, load_projection_matrix
    from drsa_audio_amd.xai.drsa.drsa import drsa_objective
    m, x, A, C = toy_case
    root = os.path.join(str(tmp_path), "class2", "layer7")
    U = prca.main(A, C, root, num_concepts=4, device=DEV)
    assert torch.equal(U, prca.prca(A, C)[0])
    assert torch.equal(load_projection_matrix("class2", 7, str(tmp_path)), U.cpu())
    run, loss, _, path, losses = get_best_run(root)
    assert run == 1 and path.endswith("run1") and len(losses) == 1
    assert loss == pytest.approx(float(drsa_objective(A, C, U, 4)), rel=1e-6) and loss > 0


def test_prca_concept_flipping_baseline(toy_case, tmp_path):
    from drsa_audio_amd.xai.pixelflipping.cpf import cf_prca_subspace, perform_cf
    m, x, _, _ = toy_case
    Rn = cf_prca_subspace(m, x, LRP_NAME_MAP_TOY, 7, case="toy", device=DEV, num_concepts=4)
    assert isinstance(Rn, np.ndarray) and Rn.shape == (4, 4, 64, 64) and np.isfinite(Rn).all()
    Rt = cf_prca_subspace(m, x, LRP_NAME_MAP_TOY, 7, case="toy", device=DEV, num_concepts=4, as_tensor=True)
    assert torch.is_tensor(Rt) and np.array_equal(Rt.cpu().numpy(), Rn)
    out = tmp_path / "out"
    res = perform_cf(m, x, LRP_NAME_MAP_TOY, str(out), layer_idcs=[7], num_concepts=[4], toy=True, prefix="prca",
                     device=DEV)
    from drsa_audio_amd.utils import safe_pickle
    with open(out / "prca" / "4_concepts" / "aupcs_layer_7.pkl", "rb") as fh:
        saved = safe_pickle.load(fh)
    assert np.array_equal(saved, np.stack(res[(4, 7)], axis=0)) and np.isfinite(saved).all()


# -------------------------------------------------------------------------------------------- 6. ops
@pytest.fixture(scope="module")
def ops():
    import drsa_audio_amd.ops as o
    return o


def test_ops_schema_and_fake_kernels(ops):
    A, C = (_dev(v) for v in drsa_inputs(300, 25, seed=2))
    torch.library.opcheck(ops.prca_covariance, (A, C), test_utils=("test_schema", "test_faketensor"))
    M = ops.prca_covariance(A, C)
    torch.library.opcheck(ops.syevj, (M,), test_utils=("test_schema", "test_faketensor"))


def test_ops_equal_ctypes_path(ops):
    A, C = (_dev(v) for v in drsa_inputs(1000, 100, seed=3))
    M = ops.prca_covariance(A, C)
    assert torch.equal(M, prca.relevance_covariance(A, C))
    w, V = ops.syevj(M)
    w2, V2 = prca.eigh_descending(M)
    assert torch.equal(w, w2) and torch.equal(V, V2)


def test_ops_graph_capture_on_a_side_stream(ops):
    A, C = (_dev(v) for v in drsa_inputs(2000, 64, seed=4))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                      # warm-up: code objects, LDS attributes
        M0 = ops.prca_covariance(A, C)
        w0, V0 = ops.syevj(M0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        Mg = ops.prca_covariance(A, C)
        wg, Vg = ops.syevj(Mg)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Mg, M0) and torch.equal(wg, w0) and torch.equal(Vg, V0)
