"""Float64 restatement of the MFT comparison model from torch functional ops (the yardstick of tests/test_mft.py).

Written from the reference's `model/compare_method/MFT.py` (line numbers cited per step); it contains none of its
text.  `P` maps the reference's state_dict names to tensors; every function is differentiable through torch
autograd, so `train_step` yields the loss and every parameter gradient.

Dropout sites (`drop`: {site: (keep mask, p)}, applied as x * mask / (1 - p)): "emb" (:210), "<i>.attn"
(proj_drop :58), "<i>.ff1" and "<i>.ff2" (Mlp.dropout :81, :83) for block i; absent sites apply none.
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM, LN_EPS = 1e-5, 0.1, 1e-6
HEADS = 8


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


def tokenise(X, wA, wV):
    """MFT.py:187-207: A = softmax over the pixels of (wA X^T) [B, L, HW]; T = A (X wV) [B, L, 64]"""
    A = torch.softmax(torch.einsum("lj,bij->bli", wA[0], X), dim=-1)
    return A @ (X @ wV[0])


def cross_attention(P, pfx, x, drop, site):
    """MCrossAttention (MFT.py:42-59): Linear(8, 64) on each of the 8 feature slices, the query from row 0 only"""
    B, N, C = x.shape
    xs = x.reshape(B, N, HEADS, C // HEADS)
    q = (xs[:, 0:1] @ P[pfx + ".wq.weight"].t()).permute(0, 2, 1, 3)     # [B, 8, 1, 64]
    k = (xs @ P[pfx + ".wk.weight"].t()).permute(0, 2, 1, 3)             # [B, 8, N, 64]
    v = (xs @ P[pfx + ".wv.weight"].t()).permute(0, 2, 1, 3)
    attn = torch.softmax((q @ k.transpose(-2, -1)) * (C // HEADS) ** -0.5, dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(B, 1, C * HEADS)
    return _drop(drop, site, F.linear(o, P[pfx + ".proj.weight"], P[pfx + ".proj.bias"]))


def block(P, pfx, li, x, drop):
    """Block (MFT.py:97-108): the attention's [B, 1, 64] is broadcast over the 5 rows of the residual"""
    h = x
    x = F.layer_norm(x, (x.shape[-1],), P[pfx + ".attention_norm.weight"], P[pfx + ".attention_norm.bias"], LN_EPS)
    x = cross_attention(P, pfx + ".attn", x, drop, f"{li}.attn") + h
    h = x
    x = F.layer_norm(x, (x.shape[-1],), P[pfx + ".ffn_norm.weight"], P[pfx + ".ffn_norm.bias"], LN_EPS)
    x = F.gelu(F.linear(x, P[pfx + ".ffn.fc1.weight"], P[pfx + ".ffn.fc1.bias"]))
    x = _drop(drop, f"{li}.ff1", x)
    x = F.linear(x, P[pfx + ".ffn.fc2.weight"], P[pfx + ".ffn.fc2.bias"])
    return _drop(drop, f"{li}.ff2", x) + h


def forward(P, x1, x2, train=True, drop=None, rec=None):
    """MFT.forward (MFT.py:178-214) -> logits [B, Classes]; x1 [B, NC, p, p], x2 [B, NCLidar, p, p]"""
    rec = {} if rec is None else rec
    B, _, p, _ = x1.shape
    a = F.conv3d(x1.unsqueeze(1), P["conv5.0.weight"], P["conv5.0.bias"], padding=(0, 1, 1))      # :182
    a = torch.relu(batchnorm(P, "conv5.1", a, train, rec)).reshape(B, -1, p, p)                    # :183
    g = a.shape[1] // P["conv6.0.gwc.weight"].shape[1]
    a = F.conv2d(a, P["conv6.0.gwc.weight"], P["conv6.0.gwc.bias"], padding=1, groups=g) + \
        F.conv2d(a, P["conv6.0.pwc.weight"], P["conv6.0.pwc.bias"])                                # :25
    a = torch.relu(batchnorm(P, "conv6.1", a, train, rec))                                         # :185
    l = F.conv2d(x2, P["lidarConv.0.weight"], P["lidarConv.0.bias"], padding=1)                    # :186
    l = F.gelu(batchnorm(P, "lidarConv.1", l, train, rec))
    tl = tokenise(l.flatten(2).transpose(1, 2), P["token_wA_L"], P["token_wV_L"])                 # :187-196
    th = tokenise(a.flatten(2).transpose(1, 2), P["token_wA"], P["token_wV"])                     # :197-207
    x = _drop(drop, "emb", torch.cat((tl, th), dim=1) + P["position_embeddings"])                 # :208-210
    for li in range(2):
        x = block(P, f"ca.layer.{li}", li, x, drop)
    x = F.layer_norm(x, (x.shape[-1],), P["ca.encoder_norm.weight"], P["ca.encoder_norm.bias"], LN_EPS)[:, 0]
    return F.linear(x, P["out3.weight"], P["out3.bias"])                                           # :213


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
