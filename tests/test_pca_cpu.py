"""Device-side PCA, the parts that need no GPU: the float64 oracle (tests/pca_oracle.py) against scikit-learn's
PCA(K, whiten=True, svd_solver="full") on the planted cubes -- outputs, components and variances within 1e-9 (the worst
figure seen is 3e-12) --, the host-side refusals of every vc_pca_* entry point (VC_REQUIRE returns 1 before any
launch: the null pointers are never touched), the size queries, the `PCA` constructor's validation, the unchanged
defaults of `PatchBatcher`, and the `pca_components` that `get_model` records under applyPCA."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pca_oracle as O
from pca_cases import NARROW, NARROW_K, NARROW_RANK, WIDE, planted

SK_CASES = [(W, H, C, K, rank, 0.5) for W, H, C, K, rank in WIDE] + \
           [(W, H, C, min(NARROW_K, C), NARROW_RANK, 0.85) for W, H, C in NARROW[:3]]


@pytest.mark.parametrize("W,H,C,K,rank,ratio", SK_CASES)
def test_oracle_equals_scikit_learn(W, H, C, K, rank, ratio):
    dec = pytest.importorskip("sklearn.decomposition")
    X = planted(W, H, C, rank, ratio).reshape(-1, C).astype(np.float64)
    sk = dec.PCA(n_components=K, whiten=True, svd_solver="full")
    y = sk.fit_transform(X)
    ref = O.pca(X, K)
    worst = max(float(np.abs(y - ref["y"]).max()), float(np.abs(sk.components_ - ref["components"]).max()),
                float(np.abs(sk.explained_variance_ - ref["explained_variance"]).max()),
                float(np.abs(sk.mean_ - ref["mean"]).max()))
    print(f"PARITY pca_oracle vs scikit-learn {(W, H, C, K)} {worst:.3e} 1.000e-09")
    assert worst < 1e-9, worst


def test_sign_flip_matches_the_package():
    from vitcnn_amd.pca import sign_flip
    v = np.array([[0.1, -0.9, 0.3], [0.5, 0.2, -0.1], [0.0, 0.0, 0.0]])
    want = np.array([[-0.1, 0.9, -0.3], [0.5, 0.2, -0.1], [0.0, 0.0, 0.0]])
    assert np.array_equal(sign_flip(v), want) and np.array_equal(O.sign_flip(v), want)


def _raw():
    from vitcnn_amd._lib import lib
    return lib().raw


# vc_pca_mean(n, C, ld, x, workspace, mean, stream); vc_pca_cov(n, C, ld, x, mean32, workspace, cov, stream);
# vc_pca_project(n, C, ld, K, x, mean32, wt, y, ldy, stream); vc_pca_cov_workspace(n, C, bytes)
REJECTED = [
    ("mean C = 0", "vc_pca_mean", (4, 0, 0, None, None, None, None)),
    ("mean C = 513", "vc_pca_mean", (4, 513, 513, None, None, None, None)),
    ("mean n = 1", "vc_pca_mean", (1, 4, 4, None, None, None, None)),
    ("mean ld < C", "vc_pca_mean", (4, 4, 3, None, None, None, None)),
    ("cov C = 0", "vc_pca_cov", (4, 0, 0, None, None, None, None, None)),
    ("cov C = 513", "vc_pca_cov", (4, 513, 513, None, None, None, None, None)),
    ("cov n = 1", "vc_pca_cov", (1, 4, 4, None, None, None, None, None)),
    ("cov ld < C", "vc_pca_cov", (4, 4, 3, None, None, None, None, None)),
    ("project C = 0", "vc_pca_project", (4, 0, 0, 1, None, None, None, None, 1, None)),
    ("project C = 513", "vc_pca_project", (4, 513, 513, 3, None, None, None, None, 3, None)),
    ("project K = 0", "vc_pca_project", (4, 8, 8, 0, None, None, None, None, 3, None)),
    ("project K > C", "vc_pca_project", (4, 8, 8, 9, None, None, None, None, 9, None)),
    ("project K = 65", "vc_pca_project", (4, 144, 144, 65, None, None, None, None, 65, None)),
    ("project n = 1", "vc_pca_project", (1, 8, 8, 3, None, None, None, None, 3, None)),
    ("project ld < C", "vc_pca_project", (4, 8, 7, 3, None, None, None, None, 3, None)),
    ("project ldy < K", "vc_pca_project", (4, 8, 8, 3, None, None, None, None, 2, None)),
    ("workspace C = 0", "vc_pca_cov_workspace", (4, 0, None)),
    ("workspace C = 513", "vc_pca_cov_workspace", (4, 513, None)),
    ("workspace n = 1", "vc_pca_cov_workspace", (1, 4, None)),
]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_host_side_rejections(what, name, args):
    assert _raw()[name](*args) == 1, what


def test_size_queries():
    from vitcnn_amd.pca import cov_workspace_bytes, slab_rows
    R = _raw()["vc_pca_slab_rows"]()
    assert R == slab_rows() and R >= 64 and R % 32 == 0
    out = ctypes.c_long(-1)
    assert _raw()["vc_pca_cov_workspace"](2, 1, ctypes.addressof(out)) == 0 and out.value >= 64 * 64 * 4
    # one fp32 tile of 64 x 64 per slab and upper-triangle tile pair: 3 slabs x 6 pairs at C = 144
    assert cov_workspace_bytes(2 * R + 3, 144) == 3 * 6 * 64 * 64 * 4
    assert cov_workspace_bytes(R, 512) == 36 * 64 * 64 * 4
    # many rows, few bands: the mean's fp64 partial rows still fit
    assert cov_workspace_bytes(349 * 1905, 144) >= 1024 * 144 * 8


@pytest.mark.parametrize("bad", [0, -1, 65, 2.5, "3", None, True])
def test_pca_constructor_rejects(bad):
    from vitcnn_amd.pca import PCA
    with pytest.raises(ValueError):
        PCA(bad)


def test_pca_constructor_and_unfitted_state():
    from vitcnn_amd.pca import PCA
    p = PCA(30)
    assert p.n_components == 30 and p.whiten is True and not p.fitted and p.components_ is None
    assert PCA(np.int64(3), whiten=False).whiten is False
    with pytest.raises(RuntimeError):
        p.transform(np.zeros((2, 2, 40), dtype=np.float32))
    with pytest.raises(RuntimeError):
        p.state_dict()


def test_pca_state_dict_round_trip_on_the_host():
    from vitcnn_amd.pca import PCA
    ref = O.pca(planted(9, 9, 7, 7, 0.5).reshape(-1, 7), 3)
    p = PCA(3)
    p.mean_, p.components_, p.explained_variance_, p.covariance_ = (ref["mean"], ref["components"],
                                                                      ref["explained_variance"], ref["cov"])
    p.n_samples_ = 81
    q = PCA(1, whiten=False).load_state_dict(p.state_dict())
    assert q.n_components == 3 and q.whiten is True and q.n_samples_ == 81 and q.fitted
    assert all(isinstance(v, np.ndarray) for v in p.state_dict().values())
    for k in ("mean_", "components_", "explained_variance_", "covariance_"):
        assert np.array_equal(getattr(p, k), getattr(q, k)) and getattr(q, k).dtype == np.float64
    assert np.array_equal(p._projection(), q._projection()) and p._projection().dtype == np.float32
    # a K-th eigenvalue that is not positive: no whitening (scikit-learn would return inf)
    p.explained_variance_ = np.array([1.0, 0.5, 0.0])
    with pytest.raises(ValueError):
        p._projection()


def test_patchbatcher_defaults_are_unchanged():
    from vitcnn_amd.window import PatchBatcher
    prm = inspect.signature(PatchBatcher.__init__).parameters
    assert prm["applyPCA"].default is False and prm["pca"].default is None and prm["pca_components"].default == 3


def test_cube_accepts_a_float32_tensor_only():
    from vitcnn_amd.window import _cube
    t = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    assert _cube(t, torch.device("cpu")).data_ptr() == t.data_ptr()
    assert _cube(t[:, :, 0], torch.device("cpu")).shape == (2, 3, 1)
    assert torch.equal(_cube(t.numpy(), torch.device("cpu")), t)
    with pytest.raises(TypeError):
        _cube(t.double(), torch.device("cpu"))


KW = dict(n_classes=5, ignored_labels=[0], dataset="x", device=torch.device("cpu"))


@pytest.mark.parametrize("name,want", [("Multimodality_Mamba", 30), ("S2EFT", 30), ("MFT", 30), ("SpectralFormer", 30),
                                       ("HCTnet", 3)])
def test_get_model_records_pca_components(name, want):
    from vitcnn_amd.model_utils import get_model
    kw = get_model(name, n_bands=(63, 1), applyPCA=True, **KW)[3]
    assert kw["pca_components"] == want and kw["applyPCA"] is True
    kw = get_model(name, n_bands=(63, 1), applyPCA=True, pca_components=5, **KW)[3]
    assert kw["pca_components"] == 5          # setdefault: the caller's value stands
    kw = get_model(name, n_bands=(63, 1), applyPCA=False, **KW)[3]
    assert "pca_components" not in kw


@pytest.mark.parametrize("name", ["Early_fusion_CNN", "EndNet", "FusAtNet"])
def test_get_model_branches_that_ignore_apply_pca_record_nothing(name):
    from vitcnn_amd.model_utils import get_model
    assert "pca_components" not in get_model(name, n_bands=(63, 1), applyPCA=True, **KW)[3]
