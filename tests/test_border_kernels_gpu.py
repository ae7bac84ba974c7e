"""vc_patch_gather_border and vc_center_argmax on the GPU, alone: the gather against slices of np.pad (data movement:
array-equal), against vc_patch_gather where no window leaves the scene (bit for bit), with the cube embedded in a
NaN-filled buffer so that a read outside it would show in the result; the argmax against np.argmax on ties, NaN,
negative and infinite rows, and centres off the scene."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = 13, 11
MODES = {1: "symmetric", 2: "reflect", 3: "constant"}
CODES = [0, 1, 2, 3, 4, 8, 12]          # none, fliplr, flipud, both, rot90 k = 1, 2, 3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np_xform(p, code):
    """datasets.py flip / rotate on a [P, P, C] patch"""
    if code & 3:
        if code & 1:
            p = np.fliplr(p)
        if code & 2:
            p = np.flipud(p)
    elif code >> 2:
        p = np.rot90(p, k=code >> 2)
    return p


def _scene(C, seed):
    """(img [W, H, C], its device copy as a view inside a larger buffer whose other floats are NaN, the buffer)"""
    img = np.random.default_rng(seed).random((W, H, C), dtype=np.float32)
    guard = 4096
    buf = torch.full((guard + W * H * C + guard,), float("nan"), device=DEV)
    cube = buf[guard:guard + W * H * C].view(W, H, C)
    cube.copy_(torch.from_numpy(img))
    return img, cube, buf


def _corners(P):
    """the four extreme corners of the contract, the four edge mid-points and three interior windows"""
    h = P // 2
    x0, x1, y0, y1 = -h, W - P + h, -h, H - P + h
    xm, ym = (W - P) // 2, (H - P) // 2
    cor = [(x0, y0), (x0, y1), (x1, y0), (x1, y1), (x0, ym), (x1, ym), (xm, y0), (xm, y1),
           (0, 0), (xm, ym), (W - P, H - P)]
    return cor


@pytest.mark.parametrize("border", [1, 2, 3])
@pytest.mark.parametrize("C,P", [(5, 5), (35, 4), (1, 1), (3, 8)])
def test_gather_border_is_a_slice_of_np_pad(C, P, border):
    _need_gpu()
    from vitcnn_amd._lib import lib
    img, cube, buf = _scene(C, 100 * C + P)
    h = P // 2
    padded = np.pad(img, ((h, h), (h, h), (0, 0)), MODES[border])
    wins = [(c, code) for c in _corners(P) for code in CODES]
    cor = np.array([c for c, _ in wins], dtype=np.int32)
    codes = np.array([code for _, code in wins], dtype=np.uint8)
    want = np.stack([_np_xform(padded[x + h:x + h + P, y + h:y + h + P], code).transpose(2, 0, 1)
                     for (x, y), code in wins])
    cd, xd = torch.from_numpy(cor).to(DEV), torch.from_numpy(codes).to(DEV)
    out = torch.full((len(wins), C, P, P), float("nan"), device=DEV)
    lib().vc_patch_gather_border(W, H, C, P, cube.data_ptr(), cd.data_ptr(), len(wins), xd.data_ptr(), border,
                                 out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()                     # every element written, nothing read outside the cube
    assert np.array_equal(got, np.ascontiguousarray(want))
    # without codes (xform = NULL) the windows come out untransformed
    out2 = torch.full((len(wins), C, P, P), float("nan"), device=DEV)
    lib().vc_patch_gather_border(W, H, C, P, cube.data_ptr(), cd.data_ptr(), len(wins), None, border,
                                 out2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plain = np.stack([padded[x + h:x + h + P, y + h:y + h + P].transpose(2, 0, 1) for (x, y), _ in wins])
    assert np.array_equal(out2.cpu().numpy(), plain)
    assert torch.isnan(buf[:4096]).all() and torch.isnan(buf[-4096:]).all()


@pytest.mark.parametrize("border", [1, 2, 3])
@pytest.mark.parametrize("C,P", [(5, 5), (35, 4), (1, 1), (3, 8)])
def test_gather_border_equals_the_plain_gather_inside_the_scene(C, P, border):
    _need_gpu()
    from vitcnn_amd._lib import lib
    L = lib()
    _, cube, _ = _scene(C, 7 * C + P)
    cor = np.array([(x, y) for x in range(0, W - P + 1, 2) for y in range(0, H - P + 1, 3)], dtype=np.int32)
    n = len(cor)
    codes = np.array([CODES[i % len(CODES)] for i in range(n)], dtype=np.uint8)
    cd, xd = torch.from_numpy(cor).to(DEV), torch.from_numpy(codes).to(DEV)
    a = torch.full((n, C, P, P), float("nan"), device=DEV)
    b = torch.full((n, C, P, P), float("nan"), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    L.vc_patch_gather(W, H, C, P, cube.data_ptr(), cd.data_ptr(), 0, 0, n, xd.data_ptr(), a.data_ptr(), s)
    L.vc_patch_gather_border(W, H, C, P, cube.data_ptr(), cd.data_ptr(), n, xd.data_ptr(), border, b.data_ptr(), s)
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)


def _special_rows(ncls, n, rng):
    """logit rows [n, ncls]: random ones, then an exact tie, a NaN before a larger value, all negative, -inf entries,
    all -inf, two NaNs, +inf before a NaN"""
    lg = rng.standard_normal((n, ncls)).astype(np.float32)
    m = ncls // 2
    lg[0, :] = -1.0
    lg[0, [m, ncls - 1]] = 2.5                               # tie: the first wins
    lg[1, m] = np.nan
    lg[1, ncls - 1] = 1e30                                   # a NaN counts as the maximum
    lg[2] = -np.abs(lg[2]) - 1.0
    lg[3] = -np.inf
    lg[3, ncls - 1] = -3.0
    lg[4] = -np.inf                                          # all equal: index 0
    lg[5, [m, ncls - 1]] = np.nan                            # the first NaN
    lg[6, 0] = np.inf
    lg[6, ncls - 1] = np.nan
    return lg


@pytest.mark.parametrize("P", [5, 4, 1])
@pytest.mark.parametrize("ncls", [1, 5, 16])
def test_center_argmax_is_np_argmax(ncls, P):
    _need_gpu()
    from vitcnn_amd._lib import lib
    rng = np.random.default_rng(10 * ncls + P)
    h = P // 2
    # distinct centres all over the scene (a bordered run's corners: from -h), in a shuffled order
    cor = np.array([(x - h, y - h) for x in range(W) for y in range(H) if (x + 2 * y) % 3], dtype=np.int32)
    rng.shuffle(cor)
    off = []
    if P % 2 == 0:   # even P: the far-edge windows of the contract have their centre off the scene
        off = [(W - P + h, 0), (0, H - P + h), (W - P + h, H - P + h)]
        assert all(x + h == W or y + h == H for x, y in off)
    cor = np.concatenate([cor, np.array(off, dtype=np.int32).reshape(-1, 2)])
    n = len(cor)
    lg = _special_rows(ncls, n, rng)
    want = np.full((W, H), 7, dtype=np.int64)
    for (x, y), row in zip(cor[:n - len(off)], lg):
        want[x + h, y + h] = np.argmax(row)
    labels = torch.full((W, H), 7, dtype=torch.int64, device=DEV)
    cd, ld = torch.from_numpy(cor).to(DEV), torch.from_numpy(lg).to(DEV)
    lib().vc_center_argmax(W, H, P, ncls, cd.data_ptr(), n, ld.data_ptr(), labels.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), want)
    assert (want == 7).sum() > W * H // 4              # the pixels no window is centred on stay as they were
    if ncls > 1:
        assert len(set(want[want != 7].tolist())) > 1
