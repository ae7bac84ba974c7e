"""`vitcnn_amd.pca.PCA` on the MI355X against the float64 oracle (tests/pca_oracle.py, pinned to scikit-learn by
tests/test_pca_cpu.py) on the planted cubes of tests/pca_cases.py, and through `PatchBatcher` / `get_model` / `train` /
`test()`.  u = 2^-24, g(m) = m u / (1 - m u), R = vc_pca_slab_rows(); every bound is computed in float64 by the test.

a. Wide eigenvalue gaps (ratio 0.5): each component is determined.
   covariance_, elementwise, with d = |mean64 - mean32|:  (2 g(R + 3) sum|xc_i||xc_j| + n d_i d_j) / (n - 1)
   each output column j, with E the covariance difference, gap_j the nearer eigenvalue gap, r = max_n ||xc_n||:
       2 ||E||_2 / gap_j * r / sqrt(l_j) + max|y_j| ||E||_2 / l_j  +  the projection bound 2 g(C + 1) sum_c |xc_c||wt_cj|
   and that bound must itself stay below 5e-3 (a cap, so that a loose bound cannot hide a failure).
b. Narrow gaps (ratio 0.85, K = 30): single columns are not determined, so properties are checked instead --
   whiteness of the float64 re-projection with the object's own components_ / explained_variance_ within
   ||E||_2 / l_K (at most 1e-2); the device output within the projection bound of that re-projection; for K < C the
   projector distance to the oracle's subspace within 2 ||E||_2 / (l_K - l_{K+1}) (at most 2e-2).
c. PatchBatcher(pca="device") equals, bit for bit, a batcher built on PCA(3).fit_transform(cube).
d. End to end, the path that was unreachable: ViT-CNN built for the 30 PCA components trains through
   PatchBatcher(applyPCA=True, pca="device", pca_components=30) and test() shares the batcher's fit; HCTnet likewise
   with 3 components; load_state_dict(state_dict()) reproduces transform bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

import pca_oracle as O
from helpers import within
from pca_cases import NARROW, NARROW_K, NARROW_RANK, WIDE, planted
from pca_oracle import g

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def fitted(W, H, C, K, rank, ratio):
    """(the fitted PCA, its device output [n, K] on the host, the oracle's result): computed once per case"""
    from vitcnn_amd.pca import PCA
    cube = planted(W, H, C, rank, ratio).copy()   # the shared cube is read-only; torch wants a writable array
    p = PCA(K)
    y = p.fit_transform(cube)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == (W, H, K)
    return p, y.cpu().numpy().reshape(-1, K).astype(np.float64), O.pca(cube.reshape(-1, C), K)


def ratio_of(err, bound):
    assert np.isfinite(err).all() and (bound > 0).all()
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------ a. wide gaps
@pytest.mark.parametrize("W,H,C,K,rank", WIDE)
def test_wide_attributes_and_covariance(W, H, C, K, rank):
    _need_gpu()
    from vitcnn_amd.pca import slab_rows
    p, _, ref = fitted(W, H, C, K, rank, 0.5)
    n, xc = W * H, ref["xc"]
    assert p.n_samples_ == n and p.mean_.shape == (C,) and p.components_.shape == (K, C)
    assert p.explained_variance_.shape == (K,) and p.covariance_.shape == (C, C)
    assert all(a.dtype == np.float64 for a in (p.mean_, p.components_, p.explained_variance_, p.covariance_))
    x64 = planted(W, H, C, rank, 0.5).reshape(-1, C).astype(np.float64)
    within("PCA.mean_", (W, H, C), ratio_of(np.abs(p.mean_ - ref["mean"]), 1e-12 * np.abs(x64).mean(axis=0)), 1.0,
           inclusive=True)
    d = np.abs(ref["mean"] - p.mean_.astype(np.float32).astype(np.float64))
    bound = (2 * g(slab_rows() + 3) * (np.abs(xc).T @ np.abs(xc)) + n * np.outer(d, d)) / (n - 1)
    within("PCA.covariance_", (W, H, C), ratio_of(np.abs(p.covariance_ - ref["cov"]), bound), 1.0, inclusive=True)
    assert np.array_equal(p.covariance_, p.covariance_.T)


@pytest.mark.parametrize("W,H,C,K,rank", WIDE)
def test_wide_output_columns(W, H, C, K, rank):
    _need_gpu()
    p, y, ref = fitted(W, H, C, K, rank, 0.5)
    xc, lam = ref["xc"], ref["eigenvalues"]
    nE = float(np.linalg.norm(p.covariance_ - ref["cov"], 2))
    r = float(np.linalg.norm(xc, axis=1).max())
    wt = ref["components"].T / np.sqrt(ref["explained_variance"])
    proj = 2 * g(C + 1) * (np.abs(xc) @ np.abs(wt))
    for j in range(K):
        gaps = [lam[i] - lam[i + 1] for i in (j - 1, j) if 0 <= i and i + 1 < C]
        lj = lam[j]
        col = 2 * nE / min(gaps) * r / np.sqrt(lj) + np.abs(ref["y"][:, j]).max() * nE / lj if gaps else 0.0
        bound = col + proj[:, j]
        within("PCA output bound (cap)", (W, H, C, j), float(bound.max()), 5e-3)
        within("PCA output column", (W, H, C, j), ratio_of(np.abs(y[:, j] - ref["y"][:, j]), bound), 1.0, inclusive=True)
    assert np.abs(p.explained_variance_ - ref["explained_variance"]).max() <= nE + 1e-12   # Weyl's inequality


# ---------------------------------------------------------------------------------------------- b. narrow gaps
@pytest.mark.parametrize("W,H,C", NARROW)
def test_narrow_whiteness_output_and_subspace(W, H, C):
    _need_gpu()
    K = NARROW_K
    p, y, ref = fitted(W, H, C, K, NARROW_RANK, 0.85)
    n, lam = W * H, ref["eigenvalues"]
    x64 = planted(W, H, C, NARROW_RANK, 0.85).reshape(-1, C).astype(np.float64)
    nE = float(np.linalg.norm(p.covariance_ - ref["cov"], 2))
    assert nE > 0
    # whiteness of the float64 re-projection with the object's own attributes
    re = O.project(x64, p.mean_, p.components_, p.explained_variance_)
    white = float(np.linalg.norm(re.T @ re / (n - 1) - np.eye(K), 2))
    wb = nE / lam[K - 1]
    within("PCA whiteness bound (cap)", (W, H, C), wb, 1e-2, inclusive=True)
    within("PCA whiteness", (W, H, C), white, wb, inclusive=True)
    # the device output against that re-projection
    wt = p.components_.T / np.sqrt(p.explained_variance_)
    proj = 2 * g(C + 1) * (np.abs(x64 - p.mean_) @ np.abs(wt))
    within("PCA device output", (W, H, C), ratio_of(np.abs(y - re), proj), 1.0, inclusive=True)
    # the subspace against the oracle's
    if K < C:
        sb = 2 * nE / (lam[K - 1] - lam[K])
        dist = float(np.linalg.norm(p.components_.T @ p.components_ - ref["components"].T @ ref["components"], 2))
        within("PCA subspace bound (cap)", (W, H, C), sb, 2e-2, inclusive=True)
        within("PCA subspace", (W, H, C), dist, sb, inclusive=True)


# ------------------------------------------------------------------------------------------------- errors
def test_fit_rejections():
    _need_gpu()
    from vitcnn_amd.pca import PCA
    with pytest.raises(ValueError):
        PCA(8).fit(planted(9, 9, 7, 7, 0.5).copy())                         # n_components > C
    with pytest.raises(ValueError):
        PCA(1).fit(np.ones((1, 1, 4), dtype=np.float32))                # fewer than 2 pixels
    flat = PCA(2)
    with pytest.raises(ValueError):
        flat.fit(np.full((6, 5, 4), 3.0, dtype=np.float32))             # no variance: nothing to whiten by
    assert not flat.fitted                                              # and the object stays unfitted
    p = PCA(2, whiten=False).fit(np.full((6, 5, 4), 3.0, dtype=np.float32))
    assert np.array_equal(p.explained_variance_, np.zeros(2))           # unwhitened, the same cube is accepted
    with pytest.raises(ValueError):
        fitted(9, 9, 7, 3, 7, 0.5)[0].transform(planted(5, 7, 4, 4, 0.5).copy())   # another band count


# ------------------------------------------------------------------------------------- c. batcher equivalence
SW, SH, SC1, SCLS = 24, 21, 63, 4


@functools.lru_cache(maxsize=None)
def _scene():
    """a 24 x 21 scene of 3 classes in blocks, 63 HSI bands + 1 LiDAR band, a few unlabelled pixels"""
    gen = torch.Generator().manual_seed(5)
    xs, ys = torch.meshgrid(torch.arange(SW), torch.arange(SH), indexing="ij")
    cls = 1 + ((xs // 4 + ys // 5) % 3)
    gt = cls.clone()
    gt[torch.rand(SW, SH, generator=gen) < 0.1] = 0
    proto = torch.rand(SCLS, SC1 + 1, generator=gen)
    cube = proto[cls] + 0.1 * torch.randn(SW, SH, SC1 + 1, generator=gen)
    return cube[:, :, :SC1].numpy().copy(), cube[:, :, SC1:].numpy().copy(), gt.numpy().astype(np.int64)


def test_patchbatcher_device_pca_equals_a_batcher_on_the_transformed_cube():
    _need_gpu()
    from vitcnn_amd.pca import PCA
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    kw = dict(ignored_labels=(0,), batch_size=64, device="cuda", seed=3)
    a = PatchBatcher(img1, img2, gt, 11, applyPCA=True, pca="device", **kw)
    reduced = PCA(3).fit_transform(img1)
    b = PatchBatcher(reduced, img2, gt, 11, **kw)
    shared = PatchBatcher(img1, img2, gt, 11, applyPCA=True, pca=a.pca, **kw)      # a fitted object is used as it is
    unfitted = PCA(3)
    late = PatchBatcher(img1, img2, gt, 11, applyPCA=True, pca=unfitted, **kw)     # an unfitted one is fitted first
    c = PatchBatcher(img1, img2, gt, 11, pca="device", **kw)                       # applyPCA stays the switch
    assert a.pca is not None and a.pca.fitted and a.pca.n_components == 3 and shared.pca is a.pca
    assert late.pca is unfitted and unfitted.fitted and c.pca is None and b.pca is None
    ba, bb = list(a), list(b)
    assert len(ba) == len(bb) == len(a) >= 2
    for (x1, x2, t), (y1, y2, u), (z1, _, _), (w1, _, _) in zip(ba, bb, shared, late):
        assert x1.shape[1:] == (3, 11, 11) and x2.shape[1:] == (1, 11, 11)
        assert torch.equal(x1, y1) and torch.equal(x2, y2) and torch.equal(t, u)
        assert torch.equal(x1, z1) and torch.equal(x1, w1)
    assert next(iter(c))[0].shape[1] == SC1


# --------------------------------------------------------------------------------------------- d. end to end
@pytest.mark.parametrize("name,components,extra", [("Multimodality_Mamba", 30, dict(patch_size=7)), ("HCTnet", 3, {})])
def test_apply_pca_trains_and_tests_on_the_device(name, components, extra, tmp_path, monkeypatch):
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.pca import PCA
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model(name, n_classes=SCLS, n_bands=(SC1, 1), ignored_labels=[0], dataset="synthetic",
                                    applyPCA=True, device=dev, **extra)
    assert kw["pca_components"] == components
    P = kw["patch_size"]
    loader = PatchBatcher(img1, img2, gt, P, ignored_labels=(0,), batch_size=64, device=dev, seed=0,
                          applyPCA=kw["applyPCA"], pca="device", pca_components=kw["pca_components"])
    loader.bs = -(-len(loader.centers) // 2)     # one epoch of two batches
    assert len(loader) == 2 and loader.pca.n_components == components
    mu.train("t", 0, None, m, opt, crit, loader, 1, device=dev, display_iter=0)
    losses = mu.train.last_stats["losses"]
    assert len(losses) == 2 and np.isfinite(losses).all()
    # whole-image inference with the batcher's fit
    hp = dict(kw, n_classes=SCLS, batch_size=64, test_stride=1, pca=loader.pca)
    probs = mu.test(0, m, img1, img2, hp)
    assert probs.shape == (SW, SH, SCLS) and np.isfinite(probs).all()
    reduced = loader.pca.transform(img1)
    assert reduced.shape == (SW, SH, components)
    nw, nh = SW - P + 1, SH - P + 1

    def windows(t):
        t = t.permute(2, 0, 1)
        return t.unfold(1, P, 1).unfold(2, P, 1).permute(1, 2, 0, 3, 4).reshape(nw * nh, -1, P, P).contiguous()

    b1 = windows(reduced)
    b2 = windows(torch.from_numpy(np.ascontiguousarray(img2, dtype=np.float32)).cuda())
    m.eval()
    with torch.no_grad():
        ref = torch.cat([m(b1[k:k + 50], b2[k:k + 50]).cpu() for k in range(0, nw * nh, 50)])   # another grouping
    p = P // 2
    got = torch.from_numpy(probs[p:SW - p, p:SH - p].reshape(nw * nh, SCLS)).float()
    err = float((got - ref).abs().max() / ref.abs().max())
    # both sides run the same fp32 kernels on the same windows in other batch groupings, so they differ by summation
    # order only (the GEMM plan depends on the row count): 1e-5 of the largest logit, the bound of test_hctnet.py for the same comparison
    within(f"test() with the shared PCA, {name}", (SW, SH, components), err, 1e-5)
    # the fit survives a state_dict round trip bit for bit
    q = PCA(1).load_state_dict(loader.pca.state_dict())
    assert torch.equal(q.transform(img1), reduced)
