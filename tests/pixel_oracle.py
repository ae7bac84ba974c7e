"""Float64 restatement of the per-pixel comparison models EndNet and SpectralFormer and of EndNet_Loss, from torch
functional ops (the yardstick of tests/test_pixel.py and tests/test_pixel_kernels_gpu.py).

Written from the reference's `model/compare_method/EndNet.py`, `model/compare_method/spectralformer.py` and
`losses.py` (line numbers cited per step); it contains none of their text.  `P` maps the reference's state_dict names
to tensors; every function is differentiable through torch autograd, so the train steps yield the loss and every
parameter gradient.

SpectralFormer dropout sites (`drop`: {site: (keep mask, p)}, applied as x * mask / (1 - p)): "emb" (:147),
"<i>.attn" (to_out :43-46), "<i>.ff1" and "<i>.ff2" (FeedForward :28, :30) for layer i; absent sites apply none.
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM, LN_EPS = 1e-5, 0.1, 1e-5
DIM_HEAD = 16


def is_param(name):
    return not (name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked"))


def _params(sd, dtype, grad):
    return {k: (v.detach().to(dtype).requires_grad_(grad) if is_param(k) else v.detach()) for k, v in sd.items()}


def _grads(P):
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items() if is_param(k)}


def _rows(x):
    return x.reshape(x.shape[0], -1)


# ---------------------------------------------------------------------------------------------- EndNet
def batchnorm1d(P, pfx, x, train, rec):
    """nn.BatchNorm1d over the batch: batch statistics in training (the running statistics torch would hold afterwards
    go to rec["running"]), the running ones in eval; the result (the pre-ReLU value) to rec["pre"]"""
    w, b = P[pfx + ".weight"], P[pfx + ".bias"]
    if train:
        n = x.shape[0]
        mean, var = x.detach().mean(0), x.detach().var(0, unbiased=False)
        run = rec.setdefault("running", {})
        run[pfx + ".running_mean"] = (1 - BN_MOMENTUM) * P[pfx + ".running_mean"].to(x.dtype) + BN_MOMENTUM * mean
        run[pfx + ".running_var"] = (1 - BN_MOMENTUM) * P[pfx + ".running_var"].to(x.dtype) + \
            BN_MOMENTUM * var * n / (n - 1)
        run[pfx + ".num_batches_tracked"] = P[pfx + ".num_batches_tracked"] + 1
        y = F.batch_norm(x, None, None, w, b, True, 0.0, BN_EPS)
    else:
        y = F.batch_norm(x, P[pfx + ".running_mean"].to(x.dtype), P[pfx + ".running_var"].to(x.dtype), w, b, False, 0.0,
                         BN_EPS)
    rec.setdefault("pre", {})[pfx] = y.detach()
    return y


def _lin(P, name, x):
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def endnet_forward(P, x1, x2, train=True, rec=None):
    """EndNet.forward (EndNet.py:59-90) -> (out, de_x1, de_x2); joint_encoder_bn7 is never applied (:76)"""
    rec = {} if rec is None else rec
    h = []
    for sfx, x in (("_a", _rows(x1)), ("_b", _rows(x2))):                                    # :61-71
        for i in range(1, 5):
            x = torch.relu(batchnorm1d(P, f"encoder_bn{i}{sfx}", _lin(P, f"encoder_fc{i}{sfx}", x), train, rec))
        h.append(x)
    joint = torch.cat(h, 1)                                                                  # :73
    joint = torch.relu(batchnorm1d(P, "joint_encoder_bn5", _lin(P, "joint_encoder_fc5", joint), train, rec))
    out = torch.relu(batchnorm1d(P, "joint_encoder_bn6", _lin(P, "joint_encoder_fc6", joint), train, rec))
    out = _lin(P, "joint_encoder_fc7", out)                                                  # :76
    de = []
    for sfx in ("_a", "_b"):                                                                 # :78-88
        x = joint
        for i in range(1, 5):
            x = torch.sigmoid(_lin(P, f"decoder_fc{i}{sfx}", x))
        de.append(x)
    return out, de[0], de[1]


def endnet_loss(out, de1, de2, x1, x2, target, weight):
    """EndNet_Loss (losses.py:29-35)"""
    return F.cross_entropy(out, target, weight=weight) + F.mse_loss(de1, _rows(x1)) + F.mse_loss(de2, _rows(x2))


def endnet_train_step(sd, x1, x2, target, weight, dtype=torch.float64):
    """one train-mode forward + EndNet_Loss + backward in `dtype`: ((out, de_x1, de_x2), loss, {name: gradient},
    {name: running statistic after the step}, {bn prefix: pre-ReLU values})"""
    P = _params(sd, dtype, True)
    rec = {}
    x1, x2 = x1.to(dtype), x2.to(dtype)
    outs = endnet_forward(P, x1, x2, True, rec)
    loss = endnet_loss(*outs, x1, x2, target, weight.to(dtype))
    loss.backward()
    running = {k: v for k, v in sd.items() if not is_param(k)}      # bn7: untouched
    running.update(rec["running"])
    return tuple(o.detach() for o in outs), loss.detach(), _grads(P), running, rec["pre"]


def endnet_eval(sd, x1, x2, dtype=torch.float64):
    P = _params(sd, dtype, False)
    with torch.no_grad():
        return endnet_forward(P, x1.to(dtype), x2.to(dtype), False)


# ---------------------------------------------------------------------------------------------- SpectralFormer
def _drop(drop, site, x):
    if drop is None or site not in drop:
        return x
    mask, p = drop[site]
    return x * mask.to(x.dtype).reshape(x.shape) / (1.0 - p)


def sf_forward(P, x1, x2, drop=None):
    """SpectralFormer.forward (spectralformer.py:131-156) in 'ViT' mode (Transformer.forward :94-97): every band of the
    concatenated spectrum is a token of one value"""
    x = torch.cat((_rows(x1), _rows(x2)), dim=1).unsqueeze(-1)                               # :132-139  [B, N, 1]
    x = _lin(P, "patch_to_embedding", x)                                                     # :140
    B, N, D = x.shape
    x = torch.cat((P["cls_token"].expand(B, 1, D), x), dim=1) + P["pos_embedding"][:, :N + 1]   # :144-146
    x = _drop(drop, "emb", x)                                                                # :147
    depth = 1 + max(int(k.split(".")[2]) for k in P if k.startswith("transformer.layers."))
    for i in range(depth):
        a, f = f"transformer.layers.{i}.0.fn", f"transformer.layers.{i}.1.fn"
        y = F.layer_norm(x, (D,), P[a + ".norm.weight"], P[a + ".norm.bias"], LN_EPS)        # PreNorm :19-20
        qkv = F.linear(y, P[a + ".fn.to_qkv.weight"])                                        # :52
        h = qkv.shape[-1] // (3 * DIM_HEAD)
        q, k, v = (t.reshape(B, N + 1, h, DIM_HEAD).transpose(1, 2) for t in qkv.chunk(3, dim=-1))   # :54
        att = torch.softmax(q @ k.transpose(-2, -1) * DIM_HEAD ** -0.5, dim=-1)              # :57, :69
        o = (att @ v).transpose(1, 2).reshape(B, N + 1, h * DIM_HEAD)                        # :71-73
        x = _drop(drop, f"{i}.attn", _lin(P, a + ".fn.to_out.0", o)) + x                     # :74, Residual :12
        y = F.layer_norm(x, (D,), P[f + ".norm.weight"], P[f + ".norm.bias"], LN_EPS)
        y = _drop(drop, f"{i}.ff1", F.gelu(_lin(P, f + ".fn.net.0", y)))                     # :26-28
        x = _drop(drop, f"{i}.ff2", _lin(P, f + ".fn.net.3", y)) + x                         # :29-30
    y = F.layer_norm(x[:, 0], (D,), P["mlp_head.0.weight"], P["mlp_head.0.bias"], LN_EPS)    # :153-156
    return _lin(P, "mlp_head.1", y)


def sf_train_step(sd, x1, x2, target, weight, drop=None, dtype=torch.float64):
    """one train-mode forward + weighted CE + backward in `dtype`: (logits, loss, {name: gradient})"""
    P = _params(sd, dtype, True)
    logits = sf_forward(P, x1.to(dtype), x2.to(dtype), drop)
    loss = F.cross_entropy(logits, target, weight=weight.to(dtype))
    loss.backward()
    return logits.detach(), loss.detach(), _grads(P)


def sf_eval(sd, x1, x2, dtype=torch.float64):
    P = _params(sd, dtype, False)
    with torch.no_grad():
        return sf_forward(P, x1.to(dtype), x2.to(dtype))
