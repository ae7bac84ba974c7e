"""Device-side PCA of the HSI cube (the reference's utils.py:85-93 applyPCA, scikit-learn's PCA(whiten=True) on the host).

`PCA(n_components, whiten=True)` mirrors the scikit-learn estimator for the one use the pipelines make of it: fit on the
[W, H, C] cube's W * H pixel spectra, transform that cube (or another one of the same band count) to [W, H, K].  Mean,
covariance and projection are HIP kernels (csrc/pca.hip: vc_pca_mean, vc_pca_cov, vc_pca_project); the cube is uploaded
once and the transformed cube stays on the device, so `PatchBatcher` and `test()` cut their patches from it directly.

What stays on the host is the C x C eigendecomposition: `fit` makes one device-to-host copy of the fp64 mean and
covariance and runs `numpy.linalg.eigh` in float64 (C <= 512, once per scene: a few milliseconds against the scene's
training run; a device eigensolver is out of scope).  Eigenvalues are sorted descending, K kept, and each component
flipped so that its largest-magnitude entry is positive -- scikit-learn's `svd_flip(u, v, u_based_decision=False)`, so
the columns agree in sign with `sklearn.decomposition.PCA(K, whiten=True, svd_solver="full")`.  The whitening
1 / sqrt(explained_variance_) is folded into the projection matrix in float64, which is then rounded once to fp32.

Divergence from scikit-learn: with `whiten=True`, a K-th eigenvalue that is not positive (fewer than K directions of
variance) raises ValueError here; scikit-learn divides by zero and returns inf / nan columns.

The device kernels centre with the fp32 rounding of the fp64 mean (`mean_.astype(float32)`), in `fit` and in
`transform` alike; `mean_` itself is the fp64 value, as scikit-learn's attribute.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import lib

MAX_BANDS = 512        # vc_pca_*: 1 <= C <= 512
MAX_COMPONENTS = 64    # vc_pca_project: 1 <= K <= min(C, 64)


def slab_rows() -> int:
    """R of vc_pca_cov: the rows of the cube one block accumulates in fp32 before the fp64 sum over the slabs"""
    return int(lib().raw["vc_pca_slab_rows"]())


def cov_workspace_bytes(n: int, C: int) -> int:
    out = ctypes.c_long(0)
    lib().vc_pca_cov_workspace(n, C, ctypes.addressof(out))
    return int(out.value)


def sign_flip(components: np.ndarray) -> np.ndarray:
    """scikit-learn's svd_flip(..., u_based_decision=False) on the rows of `components` [K, C]: every component gets the
    sign that makes its largest-magnitude entry positive"""
    idx = np.argmax(np.abs(components), axis=1)
    signs = np.sign(components[np.arange(components.shape[0]), idx])
    signs[signs == 0] = 1.0
    return components * signs[:, None]


class PCA:
    """fit / transform / fit_transform over [W, H, C] cubes (a numpy array or a float32 device tensor; a [W, H] array
    is one band).  Attributes after `fit`, in float64 as scikit-learn's: `mean_` [C], `components_` [K, C],
    `explained_variance_` [K], `n_samples_`; plus `covariance_` [C, C] (over n - 1)."""

    _STATE = ("mean_", "components_", "explained_variance_", "covariance_")

    def __init__(self, n_components: int, whiten: bool = True, device="cuda"):
        if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)):
            raise ValueError(f"n_components must be an integer, got {n_components!r}")
        if not 1 <= int(n_components) <= MAX_COMPONENTS:
            raise ValueError(f"n_components must lie in 1 .. {MAX_COMPONENTS}, got {n_components}")
        self.n_components = int(n_components)
        self.whiten = bool(whiten)
        self.device = torch.device(device)
        self.mean_ = self.components_ = self.explained_variance_ = self.covariance_ = None
        self.n_samples_ = None
        self._dev = None   # (device, mean32 [C], wt [C, K]) of the fitted transform

    @property
    def fitted(self) -> bool:
        return self.components_ is not None

    def _upload(self, cube) -> torch.Tensor:
        from .window import _cube
        dev = cube.device if isinstance(cube, torch.Tensor) and cube.is_cuda else self.device
        if dev.type != "cuda":
            raise RuntimeError("the PCA kernels run on a ROCm device; there is no CPU path")
        x = _cube(cube, dev)
        if x.dim() != 3:
            raise ValueError(f"expected a [W, H, C] cube, got shape {tuple(x.shape)}")
        return x

    def fit(self, cube) -> "PCA":
        """mean and covariance on the device, one copy of the C + C * C doubles to the host, `numpy.linalg.eigh` there
        in float64 (C <= 512, once per scene), sign flip, whitening folded into the fp32 projection matrix"""
        self._fit(self._upload(cube))
        return self

    def _fit(self, x: torch.Tensor) -> None:
        L = lib()
        n, C, K = int(x.shape[0] * x.shape[1]), int(x.shape[2]), self.n_components
        if n < 2:
            raise ValueError(f"PCA needs at least 2 pixels, the cube has {n}")
        if K > C:
            raise ValueError(f"n_components = {K} exceeds the cube's {C} bands")
        if C > MAX_BANDS:
            raise ValueError(f"at most {MAX_BANDS} bands, the cube has {C}")
        s = torch.cuda.current_stream(x.device).cuda_stream
        ws = torch.empty(cov_workspace_bytes(n, C), dtype=torch.uint8, device=x.device)
        stats = torch.empty(C + C * C, dtype=torch.float64, device=x.device)   # mean | covariance: one copy back
        mean, cov = stats[:C], stats[C:]
        L.vc_pca_mean(n, C, C, x.data_ptr(), ws.data_ptr(), mean.data_ptr(), s)
        mean32 = mean.to(torch.float32)
        L.vc_pca_cov(n, C, C, x.data_ptr(), mean32.data_ptr(), ws.data_ptr(), cov.data_ptr(), s)
        host = stats.cpu().numpy()
        self.mean_ = host[:C].copy()
        self.covariance_ = host[C:].reshape(C, C).copy()
        w, v = np.linalg.eigh(self.covariance_)
        order = np.argsort(w)[::-1][:K]
        self.explained_variance_ = w[order].copy()
        self.components_ = sign_flip(np.ascontiguousarray(v[:, order].T))
        self.n_samples_ = n
        self._dev = None
        try:
            self._projection()   # raises on a non-positive eigenvalue under whitening
        except ValueError:
            self.mean_ = self.components_ = self.explained_variance_ = self.covariance_ = self.n_samples_ = None
            raise                # the object stays unfitted

    def _projection(self) -> np.ndarray:
        """wt [C, K] fp32: the components, with the whitening folded in in float64, rounded once"""
        wt = self.components_.T.astype(np.float64)
        if self.whiten:
            if not self.explained_variance_[-1] > 0:
                raise ValueError(
                    f"whitening needs {self.n_components} positive eigenvalues; the smallest kept one is "
                    f"{self.explained_variance_[-1]:.3e} (scikit-learn would return inf / nan columns here)")
            wt = wt / np.sqrt(self.explained_variance_)[None, :]
        return np.ascontiguousarray(wt.astype(np.float32))

    def _device_state(self, dev):
        if self._dev is None or self._dev[0] != dev:
            mean32 = torch.as_tensor(self.mean_.astype(np.float32)).to(dev)
            self._dev = (dev, mean32, torch.as_tensor(self._projection()).to(dev))
        return self._dev[1], self._dev[2]

    def transform(self, cube) -> torch.Tensor:
        """[W, H, K] float32 on the device; nothing returns to the host"""
        if not self.fitted:
            raise RuntimeError("PCA.transform before fit")
        return self._transform(self._upload(cube))

    def _transform(self, x: torch.Tensor) -> torch.Tensor:
        W, H, C = (int(d) for d in x.shape)
        K = self.n_components
        if C != self.mean_.shape[0]:
            raise ValueError(f"fitted on {self.mean_.shape[0]} bands, the cube has {C}")
        mean32, wt = self._device_state(x.device)
        y = torch.empty(W, H, K, dtype=torch.float32, device=x.device)
        lib().vc_pca_project(W * H, C, C, K, x.data_ptr(), mean32.data_ptr(), wt.data_ptr(), y.data_ptr(), K,
                             torch.cuda.current_stream(x.device).cuda_stream)
        return y

    def fit_transform(self, cube) -> torch.Tensor:
        x = self._upload(cube)
        self._fit(x)
        return self._transform(x)

    def state_dict(self) -> dict:
        if not self.fitted:
            raise RuntimeError("PCA.state_dict before fit")
        sd = {k: np.array(getattr(self, k), dtype=np.float64) for k in self._STATE}
        sd["n_samples_"] = np.array(self.n_samples_, dtype=np.int64)
        sd["n_components"] = np.array(self.n_components, dtype=np.int64)
        sd["whiten"] = np.array(self.whiten)
        return sd

    def load_state_dict(self, sd: dict) -> "PCA":
        K = int(sd["n_components"])
        comps = np.array(sd["components_"], dtype=np.float64)
        if comps.ndim != 2 or comps.shape[0] != K or not 1 <= K <= MAX_COMPONENTS:
            raise ValueError("state_dict: components_ must be [n_components, C]")
        self.n_components, self.whiten = K, bool(sd["whiten"])
        for k in self._STATE:
            setattr(self, k, np.array(sd[k], dtype=np.float64))
        self.n_samples_ = int(sd["n_samples_"])
        self._dev = None
        return self


def resolve(pca, n_components: int, x: torch.Tensor):
    """The `pca=` argument of PatchBatcher / test(): "device" fits a new PCA(n_components) on the uploaded cube `x`; a
    PCA object is used as it is, fitted on `x` first if it is unfitted.  Returns (the fitted object, transform(x))."""
    if isinstance(pca, str):
        if pca != "device":
            raise ValueError(f'pca must be None, "device" or a PCA object, got {pca!r}')
        pca = PCA(n_components, device=x.device)
    elif not isinstance(pca, PCA):
        raise ValueError(f'pca must be None, "device" or a PCA object, got {type(pca).__name__}')
    if not pca.fitted:
        pca._fit(x)
    return pca, pca._transform(x)
