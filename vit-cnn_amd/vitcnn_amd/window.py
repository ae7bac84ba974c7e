"""Device-side patch windows: whole-image inference (test()) and training-batch assembly.

* `SlidingWindowInference` — model_utils.test (model_utils.py:1067-1132) over
  utils.sliding_window / count_sliding_window / grouper (utils.py:357-415, :567-582), centre-pixel
  mode.  The two image cubes are uploaded once in their source layout img[x][y][c]; each batch of
  windows is gathered on the device (vc_patch_gather) and its logits are added into an fp64
  probability map on the device (vc_center_accumulate).  Window order, clamping and the float64
  accumulation are the reference's; eval-mode BatchNorm uses running statistics, so the batch
  size only changes throughput, not results.
* `PatchBatcher` — MultiModalX (datasets.py:461-593): labelled centre pixels inside the border,
  shuffled once, batches gathered on the device with the reference's flip / rot90 augmentation
  decisions drawn on the host (datasets.py:511-526) and applied inside the gather.
* `border=` on both -- the reference's utils.padding_image / restore_from_padding (np.pad of P // 2 around the
  scene, utils.py:320-354) as an index map inside the gather (vc_patch_gather_border), so edge pixels are trained
  on and classified without a padded copy of the cube; `run(centers=)` / `run_labels()` evaluate chosen pixels only
  and write the class map on the device (vc_center_argmax).  DESIGN.md section 32.
* `epoch_order` / `device_decisions` -- numpy restatements of vc_epoch_shuffle and vc_aug_draw, the per-epoch
  reshuffle and the per-sample augmentation draws that `PatchBatcher(shuffle="epoch", draws="device")` runs on the
  device.  DESIGN.md section 33.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import lib


def window_count(W: int, H: int, P: int, step: int) -> int:
    out = ctypes.c_long(0)
    lib().vc_window_count(W, H, P, step, ctypes.addressof(out))
    return int(out.value)


def _cube(img, device) -> torch.Tensor:
    """the [W, H, C] fp32 cube on `device`: from a numpy array (uploaded once) or a float32 tensor (a cube that is
    already on the device, such as `PCA.transform`'s, is taken as it is)"""
    if isinstance(img, torch.Tensor):
        if img.dtype != torch.float32:
            raise TypeError(f"a cube given as a tensor must be float32, got {img.dtype}")
        t = img.detach()
    else:
        t = torch.as_tensor(np.ascontiguousarray(img, dtype=np.float32))
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    return t.to(device).contiguous()


BORDER_MODES = {"symmetric": 1, "reflect": 2, "constant": 3}   # np.pad's names -> vc_patch_gather_border's codes


def border_code(border, shape=None, patch_size=None) -> int:
    """the gather's code of a border mode name (None: 0, no border).  An unknown name, and with the scene's `shape`
    and `patch_size` a scene the border gather would refuse, raise ValueError here, on the host and before any launch."""
    if border is None:
        return 0
    if not isinstance(border, str) or border not in BORDER_MODES:
        raise ValueError(f"unknown border mode {border!r}: expected None or one of {sorted(BORDER_MODES)}")
    if shape is not None:
        W, H = int(shape[0]), int(shape[1])
        if patch_size is not None and (W < patch_size or H < patch_size):
            raise ValueError(f"a {W} x {H} scene is smaller than the {patch_size} x {patch_size} window")
        if border == "reflect" and min(W, H) < 2:
            raise ValueError(f"border='reflect' needs at least 2 pixels along each axis, the scene is {W} x {H}")
    return BORDER_MODES[border]


def border_index(i: int, n: int, mode: str) -> int:
    """The pixel of an axis of length n that index i reads under np.pad's `mode` (the index map of
    vc_patch_gather_border, restated on the host): i itself inside [0, n); outside, symmetric mirrors about the
    edge (-i - 1, 2n - 1 - i), reflect about the edge pixel (-i, 2n - 2 - i), and constant returns -1: no pixel is
    read, the value is 0.  Like the kernel it applies one reflection and clamps, which is exact for windows that
    leave the scene by at most P // 2 <= n // 2."""
    border_code(mode)
    if 0 <= i < n:
        return i
    if mode == "constant":
        return -1
    if mode == "symmetric":
        j = -i - 1 if i < 0 else 2 * n - 1 - i
    else:
        j = -i if i < 0 else 2 * n - 2 - i
    return min(max(j, 0), n - 1)


def _axis_corners(L: int, P: int, step: int) -> np.ndarray:
    """sliding_window's corners along one axis (utils.py:374-397): every step-th, the last clamped to L - P"""
    off = (L - P) % step
    return np.minimum(np.arange(0, L - P + off + 1, step), L - P)


def _axis_centres(L: int, P: int, step: int, bordered: bool) -> np.ndarray:
    """the window centres along one axis in traversal order, in scene coordinates: the in-scene windows', or with a
    border those of the axis padded by P // 2 on each side (a padded corner xp has the scene centre xp; the one
    centre past the far edge that an even P gives is dropped)"""
    if not bordered:
        return _axis_corners(L, P, step) + P // 2
    c = _axis_corners(L + 2 * (P // 2), P, step)
    return c[c < L]


def border_corners(W: int, H: int, P: int, step: int) -> np.ndarray:
    """int32 [n, 2] window corners of a bordered run in scene coordinates (components from -(P // 2)): the windows of
    the reference's sliding_window over the scene padded by P // 2 (utils.padding_image), in its order and with its
    clamping, shifted back by P // 2, those whose centre restore_from_padding would cut away dropped."""
    return _grid(_axis_centres(W, P, step, True), _axis_centres(H, P, step, True)) - np.int32(P // 2)


def _grid(xs, ys) -> np.ndarray:
    """[len(xs) * len(ys), 2] int32, x outer and y inner (sliding_window's loop order)"""
    g = np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.ascontiguousarray(g, dtype=np.int32)


class SlidingWindowInference:
    """`border` (None, "symmetric", "reflect" or "constant"): the run of the reference over the scene padded by
    P // 2 with that np.pad mode and cut back afterwards -- restore_from_padding(test(padding_image(img1, [P, P],
    mode), padding_image(img2, [P, P], mode))), utils.py:320-354 -- so that every pixel has a window; no padded
    cube is built, the border gather mirrors the addresses."""

    def __init__(self, net, img1, img2, patch_size: int, step: int = 1, n_classes: int = 16, device="cuda",
                 border=None):
        self.border = border_code(border, np.shape(img1) if not isinstance(img1, torch.Tensor) else img1.shape,
                                  int(patch_size))
        self.net = net
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("whole-image inference runs on a ROCm device; there is no CPU path")
        self.c1 = _cube(img1, self.device)
        self.c2 = _cube(img2, self.device)
        self.W, self.H = int(self.c1.shape[0]), int(self.c1.shape[1])
        if tuple(self.c2.shape[:2]) != (self.W, self.H):
            raise RuntimeError("the two modalities must cover the same image grid")
        self.P, self.step, self.ncls = int(patch_size), int(step), int(n_classes)
        self.n = window_count(self.W, self.H, self.P, self.step)
        # with a border: the whole corner list, on the device (the sliding enumeration of vc_patch_gather knows
        # in-scene windows only)
        self.corners = None
        if self.border:
            self.corners = torch.as_tensor(border_corners(self.W, self.H, self.P, self.step)).to(self.device)
            self.n = int(self.corners.shape[0])

    def _corners_at(self, centers) -> torch.Tensor:
        """int32 [m, 2] device corners of the run's windows centred at `centers` ([m, 2] scene pixels), in traversal
        order, each once; a centre that no window of the run has (off the scene, between strides, or without a border
        within P // 2 of an edge) is skipped"""
        c = np.asarray(centers)
        if c.ndim != 2 or c.shape[1] != 2 or not (c.size == 0 or np.issubdtype(c.dtype, np.integer)):
            raise ValueError("centers must be an [m, 2] integer array of scene pixels")
        c = c.astype(np.int64).reshape(-1, 2)
        okx, oky = np.zeros(self.W, dtype=bool), np.zeros(self.H, dtype=bool)
        okx[_axis_centres(self.W, self.P, self.step, bool(self.border))] = True
        oky[_axis_centres(self.H, self.P, self.step, bool(self.border))] = True
        c = c[(c[:, 0] >= 0) & (c[:, 0] < self.W) & (c[:, 1] >= 0) & (c[:, 1] < self.H)]
        c = c[okx[c[:, 0]] & oky[c[:, 1]]]
        c = np.unique(c, axis=0) if len(c) else c     # row-major, i.e. x outer and y inner: the traversal's order
        return torch.as_tensor(np.ascontiguousarray(c - self.P // 2, dtype=np.int32)).to(self.device)

    def _traverse(self, corners, batch_size, max_batch, sink):
        """gather -> eval forward -> sink(corner pointer or None, k0, n, logits pointer, stream) per batch of windows:
        `corners` None walks the in-scene sliding enumeration (no border), a device [n, 2] tensor those windows"""
        L = lib()
        self.net.eval()
        total = self.n if corners is None else int(corners.shape[0])
        bs = max(int(batch_size), min(int(max_batch), total))
        C1, C2, P = int(self.c1.shape[2]), int(self.c2.shape[2]), self.P
        buf1 = torch.empty(bs, C1, P, P, device=self.device)
        buf2 = torch.empty(bs, C2, P, P, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        for k0 in range(0, total, bs):
            n = min(bs, total - k0)
            x1, x2 = buf1[:n], buf2[:n]
            if corners is None:
                cor = None
                L.vc_patch_gather(self.W, self.H, C1, P, self.c1.data_ptr(), None, k0, self.step, n, None,
                                  x1.data_ptr(), s)
                L.vc_patch_gather(self.W, self.H, C2, P, self.c2.data_ptr(), None, k0, self.step, n, None,
                                  x2.data_ptr(), s)
            else:
                cor = corners[k0:k0 + n].data_ptr()
                for C, cube, x in ((C1, self.c1, x1), (C2, self.c2, x2)):
                    if self.border:
                        L.vc_patch_gather_border(self.W, self.H, C, P, cube.data_ptr(), cor, n, None, self.border,
                                                 x.data_ptr(), s)
                    else:   # the host kept in-scene windows only
                        L.vc_patch_gather(self.W, self.H, C, P, cube.data_ptr(), cor, 0, 0, n, None, x.data_ptr(), s)
            out = self.net(x1, x2)
            if isinstance(out, tuple):
                out = out[0]
            out = out.detach().to(torch.float32).contiguous()
            sink(cor, k0, n, out.data_ptr(), s)

    @torch.no_grad()
    def run(self, batch_size: int = 64, max_batch: int = 4096, centers=None) -> np.ndarray:
        """probs [W, H, n_classes] float64.  Windows go through the model `max(batch_size, ...)`
        at a time (eval-mode results do not depend on the grouping).  `centers` ([m, 2] integer scene pixels):
        only the run's windows centred there are evaluated, every other row stays zero."""
        L = lib()
        probs = torch.zeros(self.W, self.H, self.ncls, dtype=torch.float64, device=self.device)
        corners = self.corners if centers is None else self._corners_at(centers)

        def accumulate(cor, k0, n, logits, s):
            if cor is None:
                L.vc_center_accumulate(self.W, self.H, self.P, self.ncls, None, k0, self.step, n, logits,
                                       probs.data_ptr(), s)
            else:
                L.vc_center_accumulate(self.W, self.H, self.P, self.ncls, cor, 0, 0, n, logits, probs.data_ptr(), s)

        self._traverse(corners, batch_size, max_batch, accumulate)
        return probs.cpu().numpy()

    @torch.no_grad()
    def run_labels(self, centers=None, batch_size: int = 64, max_batch: int = 4096) -> torch.Tensor:
        """The class map int64 [W, H] on the device: argmax of each window's logits written at its centre
        (vc_center_argmax), 0 where no window was evaluated -- np.argmax(run(...), -1) without the probability map.
        Only at stride 1, where every centre has exactly one window."""
        if self.step != 1:
            raise ValueError(f"run_labels needs test_stride 1 (one window per centre), got {self.step}")
        L = lib()
        labels = torch.zeros(self.W, self.H, dtype=torch.int64, device=self.device)
        if centers is not None:
            corners = self._corners_at(centers)
        elif self.border:
            corners = self.corners
        else:
            corners = torch.as_tensor(_grid(_axis_corners(self.W, self.P, 1), _axis_corners(self.H, self.P, 1))
                                      ).to(self.device)
        self._traverse(corners, batch_size, max_batch,
                       lambda cor, k0, n, logits, s: L.vc_center_argmax(self.W, self.H, self.P, self.ncls, cor, n,
                                                                        logits, labels.data_ptr(), s))
        return labels


SHUFFLE_MAX = 1 << 17                   # VC_SHUFFLE_MAX: the longest list vc_epoch_shuffle orders
SHUFFLE_DOMAIN = 0xD1B54A32D192ED03     # VC_SHUFFLE_DOMAIN: keeps the order's keys apart from the noise hash's
AUG_FLIP, AUG_RADIATION, AUG_MIXTURE = 1, 2, 4   # VC_AUG_*: vc_aug_draw's flag bits
_M64 = (1 << 64) - 1


def _mix64(z: np.ndarray) -> np.ndarray:
    """the splitmix64 finaliser of patches.hip over a uint64 array (array arithmetic wraps modulo 2^64)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u64(v: int) -> np.ndarray:
    return np.array([int(v) & _M64], dtype=np.uint64)


def epoch_keys(N: int, seed: int, epoch: int, key_bits: int = 64) -> np.ndarray:
    """uint64 [N]: key_j = mix64(base + j) >> (64 - key_bits) with base = mix64((seed ^ SHUFFLE_DOMAIN) + epoch),
    the sort keys of vc_epoch_shuffle"""
    if not 1 <= int(key_bits) <= 64:
        raise ValueError(f"key_bits must be in 1..64, got {key_bits}")
    base = _mix64(_u64((int(seed) & _M64) ^ SHUFFLE_DOMAIN) + _u64(epoch))
    return _mix64(base + np.arange(int(N), dtype=np.uint64)) >> np.uint64(64 - int(key_bits))


def epoch_order(N: int, seed: int, epoch: int, rank: int = 0, world: int = 1, key_bits: int = 64) -> np.ndarray:
    """int32 [ceil(N / world)]: the source indices vc_epoch_shuffle writes as order_out -- the stable argsort of
    `epoch_keys` (equal keys keep the smaller index first), wrapped to a multiple of `world` and cut every world-th
    from `rank`, np.resize(perm, per * world)[rank::world].  world 1 is the whole permutation of range(N).  Numpy only:
    an epoch's order can be reproduced without the device."""
    N, rank, world = int(N), int(rank), int(world)
    if not 1 <= N <= SHUFFLE_MAX:
        raise ValueError(f"N must be in 1..{SHUFFLE_MAX}, got {N}")
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} is outside [0, world = {world})")
    perm = np.argsort(epoch_keys(N, seed, epoch, key_bits), kind="stable")
    per = -(-N // world)
    return np.ascontiguousarray(np.resize(perm, per * world)[rank::world], dtype=np.int32)


def device_decisions(seed: int, gid0: int, n: int, flip: bool, radiation: bool, mixture: bool):
    """(xform codes [n] u8, radiation alpha [n] f32, mixture (a1, a2) [n, 2] f32), bit for bit what vc_aug_draw writes
    for the samples gid0 .. gid0 + n - 1: the decision tree of MultiModalX.__getitem__ (datasets.py:559-568, :511-535)
    over ten 24-bit uniforms u_e = (mix64(dkey + e) >> 40) * 2^-24 of the sample's key dkey = mix64(seed ^
    mix64(gid << 2 | 3)), stream 3 of the noise hash.  Each value is one fused multiply-add of float32 operands on
    the device; here the product and the sum are exact in float64 and rounded to float32 once, which is the same."""
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    f32, f64 = np.float32, np.float64
    gid = _u64(gid0) + np.arange(n, dtype=np.uint64)
    dkey = _mix64(_u64(seed) ^ _mix64((gid << np.uint64(2)) | np.uint64(3)))
    u = [(_mix64(dkey + np.uint64(e)) >> np.uint64(40)).astype(f32) * f32(2.0 ** -24) for e in range(10)]

    def fma(a, x, b):
        return (f64(f32(a)) * x.astype(f64) + f64(f32(b))).astype(f32)

    codes, rad, mix = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=f32), np.zeros((n, 2), dtype=f32)
    if flip:
        flips = (u[1] > f32(0.5)).astype(np.uint8) | ((u[2] > f32(0.5)).astype(np.uint8) << 1)
        rot = (1 + np.minimum(2, (f32(3.0) * u[4]).astype(np.int32))).astype(np.uint8) << 2
        codes = np.where(u[0] > f32(0.5), flips, np.where(u[3] > f32(0.5), rot, 0)).astype(np.uint8)
    if radiation:
        rad = np.where(u[5] < f32(0.1), fma(0.2, u[6], 0.9), f32(0)).astype(f32)
    if mixture:
        on = (u[7] < f32(0.2))[:, None]
        mix = np.where(on, np.stack([fma(0.99, u[8], 0.01), fma(0.99, u[9], 0.01)], axis=1), f32(0)).astype(f32)
    return codes, rad, np.ascontiguousarray(mix)


class PatchBatcher:
    """Training batches of MultiModalX patches assembled on the device.

    Iterating yields (hsi [B,C1,P,P], lidar [B,C2,P,P], target [B] int64) on `device`, in the
    order of the shuffled `indices` (DataLoader(shuffle=False) over the dataset; the reference's train
    loader reshuffles every epoch, main.py:434-440; this one keeps its construction-time order unless
    `shuffle="epoch"`, below).
    `rank`/`world` select a disjoint shard for data parallelism: every rank builds the batcher with the
    same `seed` and takes every world-th centre of the padded shuffled list (equal batch counts on every
    rank; `parallel.is_sharded` sees the attributes, so train() does not shard it again).

    `applyPCA=True` reduces the HSI cube to `pca_components` whitened principal components before any patch is cut
    (MultiModalX, datasets.py:507-508; `get_model` records the count its model needs as `kwargs["pca_components"]`):
    `pca=None` through scikit-learn on the host as the reference does, `pca="device"` with `vitcnn_amd.pca.PCA` fitted
    on the uploaded cube, `pca=<PCA object>` with that object (fitted first if it is not).  The fitted object is
    `self.pca`; handing it to `test()` as `hyperparams["pca"]` shares the one fit.

    Augmentations of MultiModalX.__getitem__ (datasets.py:559-568), per sample in the reference's
    order and with its probabilities, the decisions drawn from one host RandomState in the reference's
    call order (or on the device, `draws="device"` below): flip / rot90 (flip_augmentation, :511-526)
    folded into the gather; radiation noise (p 0.1: alpha ~ U(0.9, 1.1), x = alpha x + N/25, :529-532)
    and mixture noise (p 0.2: a1, a2 ~
    U(0.01, 1), x = (a1 x + a2 d2) / (a1 + a2) + N/25 with d2 the spectra of random same-class training
    pixels, :534-545) on the HSI patch by `vc_patch_noise`.  The per-element normal fields and the
    per-pixel same-class choices (the reference's np.random.normal(size=patch) / np.random.choice) are
    drawn on the device from a counter-based hash, so the host stream differs from the reference's
    after the first noisy sample (same distributions).

    Mixture noise is a deliberate divergence whose parity is UNPINNED: in the reference,
    datasets.py:540 evaluates `np.nonzero(self.labels == value)` with `self.labels` a Python list, so
    the comparison is a scalar False, np.random.choice receives an empty array and raises -- the
    reference's --mixture_augmentation never completes.  This path implements the evident intent,
    pairing the UNshuffled label list with the shuffled index list as the surrounding code does
    (:505-506, :540-543: for class v the candidates are indices[j] over the positions j with
    labels[j] == v), and is checked only against its own CPU restatement
    (oracle/patch_noise_oracle.py).

    `border` (None, "symmetric", "reflect" or "constant"): with a mode, `centers` are ALL pixels whose label is not
    ignored -- the reference's edge filter `p < x < W - p` (datasets.py:498-504) is dropped -- and a window over an
    edge reads the scene as np.pad of P // 2 in that mode would continue it (`vc_patch_gather_border`; the label
    windows of the mixture noise too), the reference's padding_image without a padded copy.  Shuffling, sharding,
    augmentation draws and the noise hash are the same; `border=None` is the reference's filter and the plain gather.

    `shuffle="epoch"` (default None: the construction-time order, every pass): the reference's per-epoch reshuffle.
    The whole construction-time centre list -- corners and labels, before sharding -- stays on the device, and every
    pass starts with one `vc_epoch_shuffle` launch on the current stream that orders it for epoch `e` and gathers this
    rank's shard into `corners` / `labels`; batch slicing is unchanged.  `e` counts the passes from 0, `set_epoch(e)`
    sets the next pass's (DistributedSampler's convention).  With `world > 1` the shard is cut from each epoch's
    permutation of the whole list, so samples move between ranks; every rank counts epochs alike, so the seed check of
    `parallel.check_loader_shard` still suffices.  The order is a uniform permutation (independent 64-bit hash keys,
    sorted), as np.random.shuffle's is, but not numpy's stream; `epoch_order` gives it on the host, and `centers` is
    then the centre list of the current epoch's shard.  The mixture tables keep the construction-time list.  At most
    SHUFFLE_MAX centres.

    `draws="device"` (default "host": `decisions()`, one RandomState loop per batch and three uploads): the per-sample
    flip / rot90 code, radiation alpha and mixture weights are drawn by `vc_aug_draw` from stream 3 of the noise hash
    into device arrays that the gather and `vc_patch_noise` read -- the reference's tree and probabilities, not
    numpy's stream (`device_decisions` restates it); no RandomState call, no upload, and with radiation or mixture
    enabled `vc_patch_noise` is always launched (it returns early per sample on zero decisions).  DESIGN.md
    section 33."""

    def __init__(self, img1, img2, gt, patch_size: int, ignored_labels=(0,), batch_size: int = 64,
                 flip_augmentation: bool = False, device="cuda", seed: int = 0, rank: int = 0, world: int = 1,
                 name: str = "synthetic", radiation_augmentation: bool = False, mixture_augmentation: bool = False,
                 applyPCA: bool = False, pca=None, pca_components: int = 3, border=None, shuffle=None,
                 draws: str = "host"):
        if shuffle is not None and shuffle != "epoch":
            raise ValueError(f"unknown shuffle {shuffle!r}: expected None or 'epoch'")
        if draws not in ("host", "device"):
            raise ValueError(f"unknown draws {draws!r}: expected 'host' or 'device'")
        self.shuffle, self.draws = shuffle, draws
        self.border = border_code(border, np.shape(gt), int(patch_size))
        self.device = torch.device(device)
        self.pca = None
        if applyPCA:   # MultiModalX (datasets.py:507-508): the HSI cube reduced to its components before any patch is cut
            if pca is None:   # the reference's host path (scikit-learn)
                from .model_utils import apply_pca
                img1 = apply_pca(np.asarray(img1), pca_components)
            else:             # on the device: "device" fits here, a PCA object is shared (pca.py)
                from .pca import resolve
                self.pca, img1 = resolve(pca, pca_components, _cube(img1, self.device))
        self.c1, self.c2 = _cube(img1, self.device), _cube(img2, self.device)
        self.P, self.bs, self.flip = int(patch_size), int(batch_size), bool(flip_augmentation)
        self.radiation, self.mixture = bool(radiation_augmentation), bool(mixture_augmentation)
        self.ignored_labels = set(ignored_labels)
        self.name = name
        self.seed = int(seed) & ((1 << 63) - 1)
        gt = np.asarray(gt)
        mask = np.ones_like(gt)
        for lab in self.ignored_labels:
            mask[gt == lab] = 0
        xs, ys = np.nonzero(mask)
        p = self.P // 2
        keep = (xs > p) & (xs < gt.shape[0] - p) & (ys > p) & (ys < gt.shape[1] - p)
        if self.border:   # every labelled pixel: windows over an edge read the mirrored scene (corners may be negative)
            keep = np.ones_like(keep)
        idx = np.stack([xs[keep], ys[keep]], axis=1)
        if self.shuffle == "epoch" and not 1 <= len(idx) <= SHUFFLE_MAX:
            raise ValueError(f"shuffle='epoch' orders 1..{SHUFFLE_MAX} centres on the device, the scene has {len(idx)}")
        labels_unshuffled = gt[idx[:, 0], idx[:, 1]].astype(np.int64)
        self.rng = np.random.RandomState(seed)
        self.rng.shuffle(idx)
        self.W, self.H = int(self.c1.shape[0]), int(self.c1.shape[1])
        if self.mixture:
            self._mixture_tables(gt, idx, labels_unshuffled)
        self.rank, self.world = int(rank), int(world)
        self.epoch = self._next_epoch = 0    # the pass `corners` / `labels` hold, and the next one (shuffle="epoch")
        self._all_centers = None
        if self.shuffle == "epoch":
            # the whole list stays on the device; the shard is cut from each epoch's order of it (epoch 0's here, on
            # the host, so that `corners` / `labels` exist before the first pass; every pass launches vc_epoch_shuffle)
            if self.world < 1 or not 0 <= self.rank < self.world:
                raise ValueError(f"rank {self.rank} is outside [0, world = {self.world})")
            self._all_centers = idx
            self._all_corners = torch.as_tensor(np.ascontiguousarray((idx - p).astype(np.int32))).to(self.device)
            self._all_labels = torch.as_tensor(gt[idx[:, 0], idx[:, 1]].astype(np.int64)).to(self.device)
            idx = idx[epoch_order(len(idx), self.seed, 0, self.rank, self.world)]
        elif self.world > 1:
            # data-parallel shard: the shuffled list padded by wrapping to ceil(N / world) * world, then every
            # world-th centre from `rank` -- disjoint shards of equal length (equal batch counts: train()
            # exchanges one gradient per batch on every rank); parallel.check_loader_shard verifies that
            # every rank built its batcher from the same seed, i.e. cut its shard from the same permutation
            per = -(-len(idx) // self.world)
            idx = np.resize(idx, (per * self.world, 2))[self.rank::self.world] if len(idx) else idx
        if self.world > 1 and self.rank > 0:
            # host augmentation draws of their own on every rank (rank 0 keeps the single-process stream)
            self.rng = np.random.RandomState((int(seed) + 7919 * self.rank) % (1 << 32))
        self.noise_seed = (self.seed ^ (0x9E3779B97F4A7C15 * self.rank)) & ((1 << 63) - 1)
        self._centers = idx
        self.labels = torch.as_tensor(gt[idx[:, 0], idx[:, 1]].astype(np.int64)).to(self.device)
        corners = (idx - p).astype(np.int32)
        self.corners = torch.as_tensor(np.ascontiguousarray(corners)).to(self.device)
        self.gid = 0     # samples drawn so far (the noise hash's counter)

    def _mixture_tables(self, gt, idx_shuffled, labels_unshuffled):
        """class v -> candidate source pixels idx_shuffled[j] for j with labels_unshuffled[j] == v, as
        CSR (off [nlab + 1], pix = x * H + y); ignored classes get none (d2 stays 0, :539); the label
        map as a float cube for the label-window gather"""
        nlab = int(max(int(gt.max()), int(labels_unshuffled.max()) if len(labels_unshuffled) else 0)) + 1
        order = np.argsort(labels_unshuffled, kind="stable")
        counts = np.bincount(labels_unshuffled, minlength=nlab)
        for lab in self.ignored_labels:
            if 0 <= lab < nlab:
                counts[lab] = 0
        keep = np.isin(labels_unshuffled[order], list(self.ignored_labels), invert=True)
        src = idx_shuffled[order[keep]]
        off = np.zeros(nlab + 1, dtype=np.int32)
        off[1:] = np.cumsum(counts)
        self.nlab = nlab
        self.mix_off = torch.as_tensor(off).to(self.device)
        self.mix_pix = torch.as_tensor((src[:, 0] * self.H + src[:, 1]).astype(np.int32)).to(self.device)
        self.gt_cube = torch.as_tensor(np.ascontiguousarray(gt, dtype=np.float32)[:, :, None]).to(self.device)

    def __len__(self):
        return -(-len(self._centers) // self.bs)

    @property
    def centers(self) -> np.ndarray:
        """[n, 2] centre pixels in the order the batches take them: the construction-time list, or with
        shuffle="epoch" the shard of epoch `self.epoch` (the pass last started), from `epoch_order`"""
        if self._all_centers is None:
            return self._centers
        return self._all_centers[epoch_order(len(self._all_centers), self.seed, self.epoch, self.rank, self.world)]

    def set_epoch(self, epoch: int):
        """the epoch whose order the next pass takes (shuffle="epoch"; later passes count on from it).  Without
        shuffle="epoch" the order does not depend on the epoch and the call changes nothing, so a loop that calls it on
        every loader, as for a DistributedSampler, needs no special case."""
        self._next_epoch = int(epoch)

    def _start_pass(self, stream):
        """shuffle="epoch": order the whole list for the next epoch and gather this rank's shard, on the device.  The
        shard goes into new tensors, so label slices handed out by an earlier pass keep their values.  The batcher
        is iterated on ONE stream: the replaced tensors return to the caching allocator, which may hand their memory
        out again on that stream only because everything that read them was enqueued there before."""
        e = self._next_epoch
        corners, labels = torch.empty_like(self.corners), torch.empty_like(self.labels)
        lib().vc_epoch_shuffle(len(self._all_centers), self.seed, e & _M64, self.rank, self.world, 64,
                               self._all_corners.data_ptr(), self._all_labels.data_ptr(), corners.data_ptr(),
                               labels.data_ptr(), None, stream)
        self.corners, self.labels = corners, labels
        self.epoch, self._next_epoch = e, e + 1

    @property
    def dataset(self):
        """DataLoader-style access (train() reads data_loader.dataset.name / .ignored_labels)"""
        return self

    def xform_codes(self, n: int) -> np.ndarray:
        """MultiModalX flip/rotate decisions (datasets.py:511-526, :559-564) as gather codes."""
        return self.decisions(n)[0]

    def decisions(self, n: int):
        """(xform codes [n] u8, radiation alpha [n] f32 (0: none), mixture (a1, a2) [n, 2] f32 (0: none)):
        per sample, in __getitem__'s order (datasets.py:559-568), from the batcher's RandomState"""
        codes = np.zeros(n, dtype=np.uint8)
        rad = np.zeros(n, dtype=np.float32)
        mix = np.zeros((n, 2), dtype=np.float32)
        r = self.rng
        flip = self.flip and self.P > 1
        if not (flip or self.radiation or self.mixture):
            return codes, rad, mix
        for i in range(n):
            if flip:
                if r.random_sample() > 0.5:
                    h = r.random_sample() > 0.5
                    v = r.random_sample() > 0.5
                    codes[i] = (1 if h else 0) | (2 if v else 0)
                elif r.random_sample() > 0.5:
                    codes[i] = int(r.choice([1, 2, 3])) << 2
            if self.radiation and r.random_sample() < 0.1:
                rad[i] = r.uniform(0.9, 1.1)
            if self.mixture and r.random_sample() < 0.2:
                mix[i] = r.uniform(0.01, 1.0, size=2)
        return codes, rad, mix

    def __iter__(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        C1, C2, P = int(self.c1.shape[2]), int(self.c2.shape[2]), self.P
        if self.shuffle == "epoch":
            self._start_pass(s)
        corners, labels = self.corners, self.labels     # this pass's: a later pass replaces them
        total = len(self._centers)
        flags = ((AUG_FLIP if self.flip and P > 1 else 0) | (AUG_RADIATION if self.radiation else 0)
                 | (AUG_MIXTURE if self.mixture else 0)) if self.draws == "device" else 0
        for b0 in range(0, total, self.bs):
            n = min(self.bs, total - b0)
            x1 = torch.empty(n, C1, P, P, device=self.device)
            x2 = torch.empty(n, C2, P, P, device=self.device)
            cor = corners[b0:b0 + n]
            if self.draws == "device":
                xfp = None
                if flags:   # all three arrays on the device, drawn there: nothing is uploaded
                    xf = torch.empty(n, dtype=torch.uint8, device=self.device)
                    rad_d, mix_d = torch.empty(n, device=self.device), torch.empty(n, 2, device=self.device)
                    lib().vc_aug_draw(n, flags, self.noise_seed, self.gid, xf.data_ptr(), rad_d.data_ptr(),
                                      mix_d.data_ptr(), s)
                    xfp = xf.data_ptr() if flags & AUG_FLIP else None
                self._gather(C1, self.c1, cor, n, xfp, x1, s)
                self._gather(C2, self.c2, cor, n, xfp, x2, s)
                if flags & (AUG_RADIATION | AUG_MIXTURE):
                    self._noise(x1, cor, xfp, rad_d, mix_d, s)
            else:
                codes, rad, mix = self.decisions(n)
                xf = torch.as_tensor(codes).to(self.device) if self.flip else None
                xfp = xf.data_ptr() if xf is not None else None
                self._gather(C1, self.c1, cor, n, xfp, x1, s)
                self._gather(C2, self.c2, cor, n, xfp, x2, s)
                if rad.any() or mix.any():
                    self.apply_noise(x1, cor, xfp, rad, mix, s)
            self.gid += n
            yield x1, x2, labels[b0:b0 + n]

    def _gather(self, C, cube, cor, n, xfp, out, stream):
        """n windows of `cube` at the device corners `cor` into out [n, C, P, P]: vc_patch_gather, or with a border
        the gather that mirrors reads outside the scene"""
        L = lib()
        if self.border:
            L.vc_patch_gather_border(self.W, self.H, C, self.P, cube.data_ptr(), cor.data_ptr(), n, xfp, self.border,
                                     out.data_ptr(), stream)
        else:
            L.vc_patch_gather(self.W, self.H, C, self.P, cube.data_ptr(), cor.data_ptr(), 0, 0, n, xfp,
                              out.data_ptr(), stream)

    def apply_noise(self, x1, cor, xfp, rad, mix, stream):
        """vc_patch_noise on x1 with the host decisions `rad` [n] / `mix` [n, 2] (numpy), uploaded here"""
        rad_d = torch.as_tensor(rad).to(self.device)
        mix_d = torch.as_tensor(np.ascontiguousarray(mix)).to(self.device)
        self._noise(x1, cor, xfp, rad_d, mix_d, stream)

    def _noise(self, x1, cor, xfp, rad_d, mix_d, stream):
        L = lib()
        n, C1, P = x1.shape[0], x1.shape[1], self.P
        lab = off = pix = None
        nlab = 0
        if self.mixture:
            lab = torch.empty(n, 1, P, P, device=self.device)
            self._gather(1, self.gt_cube, cor, n, xfp, lab, stream)
            off, pix, nlab = self.mix_off.data_ptr(), self.mix_pix.data_ptr(), self.nlab
        L.vc_patch_noise(n, C1, P, self.H, x1.data_ptr(), lab.data_ptr() if lab is not None else None,
                         rad_d.data_ptr(), mix_d.data_ptr(), off, pix, nlab, self.c1.data_ptr(), self.noise_seed, self.gid,
                         stream)
        self._last_noise = (rad_d, mix_d, lab)   # keep the uploads alive until the kernel has run
