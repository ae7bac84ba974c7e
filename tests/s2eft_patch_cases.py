"""Cases of the S2EFT patch tests: the neighbour-band token rule and the float64 spectral gate in numpy, and the
seeded inputs the CPU and GPU tests share.

Token rule (the circular neighbour-band grouping of the SpectralFormer / S2EFT data preparation, band_patch = near,
on the patch with the LiDAR bands appended after the HSI bands): with r = cat(x1, x2) over channels viewed
[B, N, P*P] and nn = near // 2,

    tokens[b, j, s*P*P + p] = r[b, (j + s - nn) mod N, p]        j in 0..N-1, s in 0..near-1

Gate (S2EFT.py:134-145 on the token rows): mask[b, j] = sigmoid(conv1d_k7_pad3([mean_c, max_c])[j]) >= beta.
"""
import functools

import numpy as np
import torch

BETA = 0.4
MARGIN = 1e-4   # a gated case keeps every float64 sigmoid at least this far from BETA


def tokens(x1, x2, near=3):
    """[B, N, near * P * P] from x1 [B, C1, P, P] and x2 [B, C2, P, P] (or None): the rule above, by index arrays"""
    r = x1 if x2 is None or x2.shape[1] == 0 else np.concatenate([x1, x2], axis=1)
    B, N = r.shape[:2]
    r = r.reshape(B, N, -1)
    src = (np.arange(N)[:, None] + np.arange(near)[None, :] - near // 2) % N      # [N, near]
    return np.ascontiguousarray(r[:, src, :].reshape(B, N, near * r.shape[2]))


def gate_sigmoid(tok, w, bias):
    """float64 sigmoid(conv1d_k7_pad3([mean_c, max_c])) [B, N] of token rows tok [B, N, C]; w [1, 2, 7], bias [1]"""
    t = tok.astype(np.float64)
    stats = np.stack([t.mean(2), t.max(2)], axis=1)                                # [B, 2, N]
    pad = np.pad(stats, ((0, 0), (0, 0), (3, 3)))
    N = t.shape[1]
    w = np.asarray(w, dtype=np.float64).reshape(2, 7)
    pre = np.full(stats.shape[::2], float(np.asarray(bias).reshape(-1)[0]))
    for k in range(7):
        pre += w[0, k] * pad[:, 0, k:k + N] + w[1, k] * pad[:, 1, k:k + N]
    return 1.0 / (1.0 + np.exp(-pre))


@functools.lru_cache(maxsize=None)
def case(shape, seed, near=3):
    """shape = (B, C1, C2, P).  The gate's conv from torch.manual_seed(seed) + nn.Conv1d(2, 1, 7, 1, 3); x1, then x2,
    standard normals of np.random.default_rng(seed), fp32.  Returns a dict with x1, x2 (None when C2 = 0), w, bias,
    tokens, the float64 sigmoid, mask (fp32 0/1), `margin` = min |sigmoid - BETA| and `ones`, the share of ones."""
    B, C1, C2, P = shape
    torch.manual_seed(seed)
    conv = torch.nn.Conv1d(2, 1, 7, 1, 3)
    w, bias = conv.weight.detach().numpy().copy(), conv.bias.detach().numpy().copy()
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal((B, C1, P, P)).astype(np.float32)
    x2 = rng.standard_normal((B, C2, P, P)).astype(np.float32) if C2 else None
    tok = tokens(x1, x2, near)
    sig = gate_sigmoid(tok, w, bias)
    mask = (sig >= np.float64(np.float32(BETA))).astype(np.float32)
    return dict(x1=x1, x2=x2, w=w, bias=bias, tokens=tok, sigmoid=sig, mask=mask,
                margin=float(np.abs(sig - np.float64(np.float32(BETA))).min()), ones=float(mask.mean()))


def conditioned(c):
    """the condition every gated case meets before a kernel result is looked at"""
    assert c["margin"] >= MARGIN, f"a float64 sigmoid lies within {MARGIN} of beta ({c['margin']:.2e})"
    assert 0.0 < c["ones"] < 1.0, f"the oracle mask holds one value only (share of ones {c['ones']})"
