"""Planted cubes for the PCA tests: `rank` orthonormal directions of the band space (min(rank, C) of them: a cube of C
bands has no more) with standard deviations ratio**j, plus white noise of standard deviation 1e-3 and a per-band offset
in [10, 11) -- so the covariance has the eigenvalues ratio**(2 j) + 1e-6 and the fp32 cube sits far from zero, where
centring matters.  ratio = 0.5 gives wide eigenvalue gaps (each component is determined), ratio = 0.85 narrow ones."""
import functools

import numpy as np

# (W, H, C, K, rank): wide gaps, ratio 0.5
WIDE = ((20, 17, 144, 3, 6), (9, 9, 7, 3, 7), (20, 17, 3, 3, 3), (5, 7, 4, 1, 4))
# (W, H, C): narrow gaps, K = 30, rank 40, ratio 0.85
NARROW = ((20, 17, 63), (33, 31, 103), (20, 17, 30), (40, 41, 512))
NARROW_K, NARROW_RANK = 30, 40


@functools.lru_cache(maxsize=None)
def planted(W, H, C, rank, ratio, seed=0):
    """the [W, H, C] float32 cube (read-only: shared between tests)"""
    rng = np.random.RandomState(1000 + seed + 7 * C + W)
    r = min(rank, C)
    q, _ = np.linalg.qr(rng.standard_normal((C, r)))
    std = ratio ** np.arange(r)
    z = rng.standard_normal((W * H, r)) * std
    x = z @ q.T + 1e-3 * rng.standard_normal((W * H, C)) + (10.0 + rng.random_sample(C))
    cube = np.ascontiguousarray(x.reshape(W, H, C).astype(np.float32))
    cube.setflags(write=False)
    return cube
