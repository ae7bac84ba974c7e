"""Float64 restatement of the HCTnet comparison model from torch functional ops (the yardstick of tests/test_hctnet*.py).

Written from the reference's `model/compare_method/HCTnet.py` (line numbers cited per step); it contains none of its
text.  `P` maps the reference's state_dict names to tensors; every function is differentiable through torch
autograd, so `train_step` yields the loss and every parameter gradient.

Dropout sites (`drop`: {site: (keep mask, p)}, applied as x * mask / (1 - p)); absent sites apply none:
  "emb.h", "emb.l"                  the embedding dropout of the HSI / LiDAR token rows (:345, :353)
  "enc.<b>.attn"                    Attention.do1 (:93) of branch b (h, l)
  "enc.<b>.ff1", "enc.<b>.ff2"      MLP_Block's two dropouts (:48, :50)
  "ct.<b>.prob", "ct.<b>.out"       CTAttention's probability dropout (:127) and to_out's (:111) for the direction whose
                                    query is branch b's cls row
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM, LN_EPS = 1e-5, 0.1, 1e-5
HEADS = 8
SITES = ("emb.h", "emb.l") + tuple(f"enc.{b}.{s}" for b in "hl" for s in ("attn", "ff1", "ff2")) + \
    tuple(f"ct.{b}.{s}" for b in "hl" for s in ("prob", "out"))


def _drop(drop, site, x):
    if drop is None or site not in drop:
        return x
    mask, p = drop[site]
    return x * mask.to(x.dtype).reshape(x.shape) / (1.0 - p)


def batchnorm(P, pfx, x, train, rec):
    """nn.BatchNorm2d / 3d over dim 1: batch statistics in training (the running statistics torch would hold
    afterwards go to rec["running"]), the running ones in eval; the result (the pre-ReLU value) to rec["pre"]"""
    w, b = P[pfx + ".weight"], P[pfx + ".bias"]
    if train:
        dims = [d for d in range(x.dim()) if d != 1]
        n = x.numel() // x.shape[1]
        mean, var = x.detach().mean(dims), x.detach().var(dims, unbiased=False)
        rec.setdefault("running", {})[pfx + ".running_mean"] = \
            (1 - BN_MOMENTUM) * P[pfx + ".running_mean"].to(x.dtype) + BN_MOMENTUM * mean
        rec["running"][pfx + ".running_var"] = \
            (1 - BN_MOMENTUM) * P[pfx + ".running_var"].to(x.dtype) + BN_MOMENTUM * var * n / (n - 1)
        y = F.batch_norm(x, None, None, w, b, True, 0.0, BN_EPS)
    else:
        y = F.batch_norm(x, P[pfx + ".running_mean"].to(x.dtype), P[pfx + ".running_var"].to(x.dtype), w, b, False, 0.0,
                         BN_EPS)
    rec.setdefault("pre", {})[pfx] = y.detach()
    return y


def tokens(P, X, drop, site):
    """HCTnet.py:326-353: A = softmax over the pixels of (wA X^T) [B, L, HW]; T = A (X wV); the cls row in front,
    + pos_embedding, the embedding dropout.  Both sources use the same four parameters."""
    A = torch.softmax(torch.einsum("lj,bij->bli", P["token_wA"][0], X), dim=-1)
    T = A @ (X @ P["token_wV"][0])
    x = torch.cat((P["cls_token"].expand(X.shape[0], -1, -1), T), dim=1) + P["pos_embedding"]
    return _drop(drop, site, x)


def encoder(P, pfx, x, drop, site):
    """Transformer (HCTnet.py:205-219) of depth 1: Residual(LayerNormalize(Attention)), Residual(LayerNormalize(MLP))"""
    B, N, C = x.shape
    a, m = pfx + ".layers.0.0.fn", pfx + ".layers.0.1.fn"
    n = F.layer_norm(x, (C,), P[a + ".norm.weight"], P[a + ".norm.bias"], LN_EPS)
    qkv = F.linear(n, P[a + ".fn.to_qkv.weight"], P[a + ".fn.to_qkv.bias"]).chunk(3, dim=-1)           # :75
    q, k, v = (t.reshape(B, N, HEADS, C // HEADS).transpose(1, 2) for t in qkv)                         # :76
    att = torch.softmax((q @ k.transpose(-2, -1)) * C ** -0.5, dim=-1)     # :61, :78: the scale is dim^-0.5
    o = (att @ v).transpose(1, 2).reshape(B, N, C)
    x = x + _drop(drop, site + ".attn", F.linear(o, P[a + ".fn.nn1.weight"], P[a + ".fn.nn1.bias"]))    # :92-93
    n = F.layer_norm(x, (C,), P[m + ".norm.weight"], P[m + ".norm.bias"], LN_EPS)
    h = _drop(drop, site + ".ff1", F.gelu(F.linear(n, P[m + ".fn.net.0.weight"], P[m + ".fn.net.0.bias"])))
    return x + _drop(drop, site + ".ff2", F.linear(h, P[m + ".fn.net.3.weight"], P[m + ".fn.net.3.bias"]))


def cross_token(P, pfx, cls, patches, drop, site):
    """ProjectInOut(identity) of LayerNormalize(CTAttention) with kv_include_self (HCTnet.py:96-131, :166-167): the
    LayerNorm is on the query row only; the context is cat(normed cls, the other branch's patch tokens)"""
    B, _, C = cls.shape
    f = pfx + ".fn"
    x = F.layer_norm(cls, (C,), P[f + ".norm.weight"], P[f + ".norm.bias"], LN_EPS)
    ctx = torch.cat((x, patches), dim=1)                                                               # :119
    q = F.linear(x, P[f + ".fn.to_q.weight"])
    k, v = F.linear(ctx, P[f + ".fn.to_kv.weight"]).chunk(2, dim=-1)
    dh = q.shape[-1] // HEADS
    q, k, v = (t.reshape(B, t.shape[1], HEADS, dh).transpose(1, 2) for t in (q, k, v))
    att = _drop(drop, site + ".prob", torch.softmax((q @ k.transpose(-2, -1)) * dh ** -0.5, dim=-1))    # :124-127
    o = (att @ v).transpose(1, 2).reshape(B, 1, HEADS * dh)
    o = F.linear(o, P[f + ".fn.to_out.0.weight"], P[f + ".fn.to_out.0.bias"])
    return _drop(drop, site + ".out", o) + cls                                                          # :166


def forward(P, x1, x2, train=True, drop=None, rec=None):
    """HCTnet.forward (HCTnet.py:316-367) -> logits [B, num_classes]; x1 [B, 3, p, p], x2 [B, 1, p, p]"""
    rec = {} if rec is None else rec
    B = x1.shape[0]
    a = F.conv3d(x1.unsqueeze(1), P["conv3d_features.0.weight"], P["conv3d_features.0.bias"])          # :317-318
    a = torch.relu(batchnorm(P, "conv3d_features.1", a, train, rec))
    a = a.reshape(B, a.shape[1] * a.shape[2], a.shape[3], a.shape[4])                                  # :319
    a = F.conv2d(a, P["conv2d_features.0.weight"], P["conv2d_features.0.bias"])
    a = torch.relu(batchnorm(P, "conv2d_features.1", a, train, rec))
    l = F.conv2d(x2, P["conv2d_features2.0.weight"], P["conv2d_features2.0.bias"])                     # :323
    l = torch.relu(batchnorm(P, "conv2d_features2.1", l, train, rec))
    h = tokens(P, a.flatten(2).transpose(1, 2), drop, "emb.h")
    l = tokens(P, l.flatten(2).transpose(1, 2), drop, "emb.l")
    fe = "fusion_encoder.layers.0"
    h = encoder(P, fe + ".0", h, drop, "enc.h")                                                        # :200
    l = encoder(P, fe + ".1", l, drop, "enc.l")
    ct = fe + ".2.layers.0"
    hc = cross_token(P, ct + ".0", h[:, :1], l[:, 1:], drop, "ct.h")                                   # :166
    lc = cross_token(P, ct + ".1", l[:, :1], h[:, 1:], drop, "ct.l")                                   # :167
    outs = []
    for c in (hc, lc):                                                                                 # :362-364
        n = F.layer_norm(c[:, 0], (c.shape[-1],), P["mlp_head.0.weight"], P["mlp_head.0.bias"], LN_EPS)
        outs.append(F.linear(n, P["mlp_head.1.weight"], P["mlp_head.1.bias"]))
    return outs[0] + outs[1]


def is_param(name):
    return not (name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked"))


def train_step(sd, x1, x2, target, weight, drop=None, dtype=torch.float64):
    """one train-mode forward + weighted CE + backward in `dtype`:
    (logits, loss, {name: gradient}, {name: running statistic after the step}, {bn prefix: pre-ReLU values})"""
    P = {k: (v.detach().to(dtype).requires_grad_(True) if is_param(k) else v.detach()) for k, v in sd.items()}
    rec = {}
    logits = forward(P, x1.to(dtype), x2.to(dtype), True, drop, rec)
    loss = F.cross_entropy(logits, target, weight=weight.to(dtype))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items() if is_param(k)}
    return logits.detach(), loss.detach(), grads, rec["running"], rec["pre"]


def eval_logits(sd, x1, x2, dtype=torch.float64):
    P = {k: (v.detach().to(dtype) if is_param(k) else v.detach()) for k, v in sd.items()}
    with torch.no_grad():
        return forward(P, x1.to(dtype), x2.to(dtype), False)
