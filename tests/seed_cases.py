"""numpy restatement of the dropout hash (csrc/s2eft.hip mix32, shared by pixel.hip and hctnet.hip) and the index of one
HCTnet site's bytes in its kernel's mask buffer, for the device-seed tests."""
import numpy as np


def mix32_keep(seed, idx, p):
    """keep_i = float(mix32(seed, i) >> 8) / 2^24 >= p for the element indices `idx`, in uint64 / fp32 as the kernel"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (u >= np.float32(p)).astype(np.uint8)


def hct_enc_attn_index(B, T, branch=0):
    """element indices of site enc.{h,l}.attn [B, T, 64] in vc_hct_encoder_fwd's mask [2][B][T*64 | T*8 | T*64]"""
    per = T * 136
    return ((branch * B + np.arange(B))[:, None] * per + np.arange(T * 64)[None, :]).reshape(B, T, 64)


HCT_ENC_SITE = 2     # hctnet.py: the encoder launch is site 2 of the forward (0, 1: the two tokenisers; 3: cross-token)


def within_bands(masks, p):
    """(keep fractions, consecutive differing fractions, ok) for the issue's bands: 5 sigma, sigma = sqrt(p (1 - p) / N),
    around 1 - p and around 2 p (1 - p)"""
    n = masks[0].size
    sigma = (p * (1 - p) / n) ** 0.5
    keep = [float(m.mean()) for m in masks]
    diff = [float((a != b).mean()) for a, b in zip(masks, masks[1:])]
    ok = all(abs(k - (1 - p)) <= 5 * sigma for k in keep) and all(abs(d - 2 * p * (1 - p)) <= 5 * sigma for d in diff)
    return keep, diff, ok
