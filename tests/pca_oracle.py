"""Float64 numpy restatement of the whitened PCA the pipelines use (scikit-learn's PCA(K, whiten=True,
svd_solver="full") on the pixel spectra): column mean, covariance over n - 1, eigh, eigenvalues sorted descending,
svd_flip(u_based_decision=False) -- each component's largest-magnitude entry made positive --, outputs divided by
sqrt(explained_variance).  tests/test_pca_cpu.py pins it to scikit-learn where that is installed."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32


def g(m):
    """gamma_m = m u / (1 - m u): the rounding-error constant of an m-operation fp32 sum"""
    return m * U / (1.0 - m * U)


def sign_flip(components):
    idx = np.argmax(np.abs(components), axis=1)
    signs = np.sign(components[np.arange(components.shape[0]), idx])
    signs[signs == 0] = 1.0
    return components * signs[:, None]


def pca(X, K, whiten=True):
    """X [n, C] -> dict(mean [C], cov [C, C], eigenvalues [C] descending, components [K, C], explained_variance [K],
    y [n, K]), all float64"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    mean = X.mean(axis=0)
    xc = X - mean
    cov = xc.T @ xc / (n - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w)[::-1]
    w, v = w[order], v[:, order]
    comps = sign_flip(np.ascontiguousarray(v[:, :K].T))
    ev = w[:K].copy()
    y = xc @ comps.T
    if whiten:
        y = y / np.sqrt(ev)
    return dict(mean=mean, cov=cov, eigenvalues=w, components=comps, explained_variance=ev, y=y, xc=xc)


def project(X, mean, components, explained_variance, whiten=True):
    """float64 projection of X [n, C] with a fitted transform's own attributes"""
    y = (np.asarray(X, dtype=np.float64) - mean) @ np.asarray(components, dtype=np.float64).T
    return y / np.sqrt(explained_variance) if whiten else y
