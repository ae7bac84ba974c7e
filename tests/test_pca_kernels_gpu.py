"""Per-kernel parity of csrc/pca.hip on the MI355X: vc_pca_mean, vc_pca_cov and vc_pca_project against float64 of the
same fp32 operands, at the smallest shapes that break each mechanism -- rows n in {2, 81, R - 1, R, R + 1, 2 R + 3}
(row tails, the slab boundary, the sum over slabs; R = vc_pca_slab_rows()), bands C in {1, 3, 4, 7, 63, 64, 65, 144,
512} (column tails, the 64-column tile boundary, the LDS maximum), components K in {1, 3, 30, 40, min(C, 64)}, leading
dimension C or C + 3 with NaN in the gap, base pointer aligned or one element off; for the projection also the row
counts past which a block walks more than one 64-row tile (768 and 256 tiles for its two weight images).

Inputs are helpers.Poisoned (NaN around the logical operand), outputs helpers.Guarded (gaps and guard untouched), the
covariance's workspace starts as NaN.  Bounds are derived, not measured: u = 2^-24, g(m) = m u / (1 - m u); the factor
2 is there because the MFMA's internal summation order and rounding are not specified as sequential IEEE; inputs stay
in the normal range.
  mean        |mean - mean64|  <= 1e-12 * mean|x|                       (fp64 accumulation)
  covariance  |S_ij - T_ij|    <= 2 g(R + 1) * sum_n |xc_i| |xc_j|      (S, T the sums; both divided by n - 1)
  projection  |y - y64|        <= 2 g(C + 1) * sum_c |xc_c| |wt_ck|
Each figure is reported as a fraction of its bound through helpers.within.  A second call gives identical bits."""
import numpy as np
import pytest
import torch

from helpers import Guarded, Poisoned, within
from pca_oracle import g

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def rows(spec, R):
    return {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}.get(spec, spec)


def matrix(n, C, seed):
    """[n, C] fp32 in the normal range: uniform(-1, 1) scaled per column, on a per-column offset in [0.5, 2.5)"""
    gen = torch.Generator().manual_seed(seed)
    scale = 0.25 + torch.rand(C, generator=gen)
    off = 0.5 + 2.0 * torch.rand(C, generator=gen)
    return (torch.rand(n, C, generator=gen) * 2.0 - 1.0) * scale + off


def workspace(n, C):
    from vitcnn_amd.pca import cov_workspace_bytes
    return torch.full((cov_workspace_bytes(n, C),), 0xFF, dtype=torch.uint8, device=DEV)   # NaN in every word


def ratio(err, bound):
    """max err / bound; where the bound is exactly zero the error must be too"""
    err, bound = np.asarray(err), np.asarray(bound)
    assert np.isfinite(err).all()
    zero = bound == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# (n, C, gap columns, lead elements)
STAT_CASES = [(2, 1, 0, 0), (2, 3, 3, 1), (81, 4, 0, 0), (81, 7, 3, 0), ("R-1", 63, 0, 1), ("R", 64, 0, 0),
              ("R+1", 65, 3, 0), ("2R+3", 144, 0, 0), ("2R+3", 3, 3, 1), (81, 144, 3, 1), (81, 512, 0, 0),
              ("R+1", 512, 0, 0)]


@pytest.mark.parametrize("n,C,gap,lead", STAT_CASES)
def test_mean(L, n, C, gap, lead):
    from vitcnn_amd.pca import slab_rows
    n = rows(n, slab_rows())
    x = matrix(n, C, seed=n + C)
    xd = Poisoned(x, ld=C + gap, lead=lead)
    ws = workspace(n, C)
    outs = []
    for _ in range(2):
        m = Guarded(1, C, dtype=torch.float64)
        L.vc_pca_mean(n, C, C + gap, xd.ptr, ws.data_ptr(), m.ptr, S())
        outs.append(m.check()[0].numpy())
    x64 = x.double().numpy()
    within("vc_pca_mean", (n, C, gap, lead), ratio(np.abs(outs[0] - x64.mean(axis=0)), 1e-12 * np.abs(x64).mean(axis=0)),
           1.0, inclusive=True)
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)), "vc_pca_mean: a second call differs"


@pytest.mark.parametrize("n,C,gap,lead", STAT_CASES)
def test_cov(L, n, C, gap, lead):
    from vitcnn_amd.pca import slab_rows
    R = slab_rows()
    n = rows(n, R)
    x = matrix(n, C, seed=n + C)
    mean32 = x.double().mean(dim=0).float()
    xd, md = Poisoned(x, ld=C + gap, lead=lead), Poisoned(mean32[None, :], lead=lead)
    outs = []
    for _ in range(2):
        ws = workspace(n, C)
        cov = Guarded(C, C, dtype=torch.float64)
        L.vc_pca_cov(n, C, C + gap, xd.ptr, md.ptr, ws.data_ptr(), cov.ptr, S())
        outs.append(cov.check().numpy())
    xc = (x.double() - mean32.double()).numpy()
    T = xc.T @ xc / (n - 1)
    bound = 2 * g(R + 1) * (np.abs(xc).T @ np.abs(xc)) / (n - 1)
    within("vc_pca_cov", (n, C, gap, lead), ratio(np.abs(outs[0] - T), bound), 1.0, inclusive=True)
    assert np.array_equal(outs[0], outs[0].T), "vc_pca_cov: not exactly symmetric"
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)), "vc_pca_cov: a second call differs"


# (n, C, K, gap columns of x, lead elements of x, gap columns of y)
PROJECT_CASES = [(2, 1, 1, 0, 0, 0), (81, 3, 3, 3, 1, 0), (81, 4, 3, 0, 0, 3), (81, 7, 3, 3, 0, 0), (81, 7, 1, 0, 1, 3),
                 ("R-1", 63, 30, 0, 0, 0), ("R", 64, 64, 0, 0, 3), ("R+1", 65, 40, 3, 1, 0), ("2R+3", 144, 30, 0, 0, 0),
                 (81, 144, 3, 3, 0, 0), (81, 144, 64, 0, 1, 0), (81, 512, 1, 0, 0, 0), (81, 512, 30, 3, 0, 3),
                 (64 * 256 + 3, 512, 64, 0, 0, 0),     # the 128-KB weight image; its blocks walk two row tiles
                 (64 * 768 + 5, 144, 30, 0, 0, 0),     # the 32-KB image, likewise (five pieces per tile)
                 (64 * 768 + 5, 4, 1, 0, 0, 0)]        # and with one piece per tile


@pytest.mark.parametrize("n,C,K,gap,lead,ygap", PROJECT_CASES)
def test_project(L, n, C, K, gap, lead, ygap):
    from vitcnn_amd.pca import slab_rows
    n = rows(n, slab_rows())
    x = matrix(n, C, seed=n + C + K)
    gen = torch.Generator().manual_seed(K)
    mean32 = x.double().mean(dim=0).float()
    wt = (torch.rand(C, K, generator=gen) * 2.0 - 1.0) * (0.5 + 4.0 * torch.rand(K, generator=gen))
    xd, md = Poisoned(x, ld=C + gap, lead=lead), Poisoned(mean32[None, :], lead=lead)
    wd = Poisoned(wt.reshape(1, C * K), lead=lead)
    outs = []
    for _ in range(2):
        y = Guarded(n, K, ld=K + ygap, lead=lead)
        L.vc_pca_project(n, C, C + gap, K, xd.ptr, md.ptr, wd.ptr, y.ptr, K + ygap, S())
        outs.append(y.check().numpy())
    xc = (x.double() - mean32.double()).numpy()
    w64 = wt.double().numpy()
    bound = 2 * g(C + 1) * (np.abs(xc) @ np.abs(w64))
    within("vc_pca_project", (n, C, K, gap, lead, ygap), ratio(np.abs(outs[0] - xc @ w64), bound), 1.0, inclusive=True)
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "vc_pca_project: a second call differs"
