"""Float64 restatement of the MHST comparison model from torch functional ops (the yardstick of tests/test_mhst*.py).

Written from the semantics of the reference's `model/compare_method/MHST/` (MHST.py, HSPT.py, Pooling.py, PyConv2D.py);
it contains none of its text.  `P` maps the reference's state_dict names to tensors; everything is differentiable
through torch autograd, so `train_step` yields the loss and every parameter gradient.

Randomness enters as data:
  noise [hs_depth, B, 16]   the gates' g1 - g2 (training only); gate i thresholds v = (logits + noise[i]) / tau at 0 and
                            passes the straight-through value hard - y.detach() + y with y = sigmoid(v)
  sel   [hs_depth, B, 16]   optional: the hard decisions to adopt instead of v > 0 (the HIP path's, for inputs whose
                            float64 decisions are not pinned); rec["gate"][i] always holds v
  dec   optional: {"relu": {BatchNorm prefix: mask shaped like its output}, "pool": {"hsi" | "lidar": winning taps
        [B, 16, 64] (dh * 2 + dw per pooled position and channel)}}: the ReLU and max-pool decisions to adopt instead of
        float64's own (x * mask; the window's tap gathered); rec["pre"] / rec["pool_in"] always hold float64's values
  drop  {site: (keep mask, p)} applied as x * mask / (1 - p); absent sites apply none.  Sites: "emb"; per encoder layer l
        "en<l>.attn", "en<l>.ff1", "en<l>.ff2"; per head-select block i "hs<i>.prob" [B,16,65,65], "hs<i>.proj",
        "hs<i>.fc1", "hs<i>.fc2".
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM, LN_EPS = 1e-5, 0.1, 1e-5
PY_KERNELS = (3, 5, 7, 9)
SPECTRAL_TAPS = (1, 3, 5, 11)
TAU = 5.0


def depths(P):
    """(en_depth, hs_depth) read off the parameter names"""
    en = len({k.split(".")[2] for k in P if k.startswith("en_transformer.layers.")})
    hs = len({k.split(".")[2] for k in P if k.startswith("HeadSelectViT.blocks.")})
    return en, hs


def sites(P):
    en, hs = depths(P)
    return ("emb",) + tuple(f"en{i}.{s}" for i in range(en) for s in ("attn", "ff1", "ff2")) + \
        tuple(f"hs{i}.{s}" for i in range(hs) for s in ("prob", "proj", "fc1", "fc2"))


def _drop(drop, site, x):
    if drop is None or site not in drop:
        return x
    mask, p = drop[site]
    return x * mask.to(x.dtype).reshape(x.shape) / (1.0 - p)


def batchnorm(P, pfx, x, train, rec):
    """BatchNorm over dim 1: batch statistics in training (the running statistics torch would hold afterwards go to
    rec["running"]), the running ones in eval; the pre-ReLU result is noted in rec["pre"]"""
    w, b = P[pfx + ".weight"], P[pfx + ".bias"]
    shape = [1, -1] + [1] * (x.dim() - 2)
    if train:
        dims = [d for d in range(x.dim()) if d != 1]
        n = x.numel() // x.shape[1]
        mean, var = x.mean(dims), x.var(dims, unbiased=False)
        run = rec.setdefault("running", {})
        run[pfx + ".running_mean"] = (1 - BN_MOMENTUM) * P[pfx + ".running_mean"].to(x.dtype) + BN_MOMENTUM * mean.detach()
        run[pfx + ".running_var"] = (1 - BN_MOMENTUM) * P[pfx + ".running_var"].to(x.dtype) + \
            BN_MOMENTUM * var.detach() * n / (n - 1)
    else:
        mean, var = P[pfx + ".running_mean"].to(x.dtype), P[pfx + ".running_var"].to(x.dtype)
    y = (x - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + BN_EPS) * w.reshape(shape) + b.reshape(shape)
    rec.setdefault("pre", {})[pfx] = y.detach()
    return y


def pyconv(P, pfx, x, kernels, groups):
    return torch.cat([F.conv2d(x, P[f"{pfx}.conv2_{i + 1}.weight"], padding=k // 2, groups=g)
                      for i, (k, g) in enumerate(zip(kernels, groups))], dim=1)


def relu_bn(P, pfx, x, train, rec, dec=None):
    """ReLU(BatchNorm(x)); with an adopted mask the ReLU is y * mask"""
    y = batchnorm(P, pfx, x, train, rec)
    if dec is None or pfx not in dec.get("relu", {}):
        return F.relu(y)
    return y * dec["relu"][pfx].to(y.dtype)


def maxpool(x, rec, site, dec=None):
    rec.setdefault("pool_in", {})[site] = x.detach()
    if dec is None or site not in dec.get("pool", {}):
        return F.max_pool2d(x, 2)
    b, c, h, w = x.shape
    win = x.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, h // 2, w // 2, 4)
    taps = dec["pool"][site].to(torch.int64).transpose(1, 2).reshape(b, c, h // 2, w // 2, 1)
    return torch.gather(win, 4, taps)[..., 0]


def ln(P, pfx, x):
    return F.layer_norm(x, (x.shape[-1],), P[pfx + ".weight"], P[pfx + ".bias"], LN_EPS)


def hsi_encoder(P, x, train, rec, dec=None):
    e = "hsi_encoder."
    x = x.unsqueeze(1)
    x = relu_bn(P, e + "bn1", F.conv3d(x, P[e + "conv1.weight"], P[e + "conv1.bias"], stride=(3, 1, 1),
                                       padding=(5, 1, 1)), train, rec, dec)
    x = torch.cat([F.conv3d(x, P[f"{e}conv2_{i + 1}.weight"], P[f"{e}conv2_{i + 1}.bias"], padding=(k // 2, 0, 0))
                   for i, k in enumerate(SPECTRAL_TAPS)], dim=1)
    x = relu_bn(P, e + "bn2", x, train, rec, dec)
    x = relu_bn(P, e + "bn3", F.conv3d(x, P[e + "conv3.weight"], P[e + "conv3.bias"], padding=1), train, rec, dec)
    x = x.reshape(x.shape[0], -1, x.shape[3], x.shape[4])     # (c d) h w
    x = relu_bn(P, e + "bn4", pyconv(P, e + "conv4", x, PY_KERNELS, (1, 2, 4, 8)), train, rec, dec)
    x = relu_bn(P, e + "bn5", F.conv2d(x, P[e + "conv5.weight"], P[e + "conv5.bias"]), train, rec, dec)
    return maxpool(x, rec, "hsi", dec)


def lidar_encoder(P, x, train, rec, dec=None):
    e = "lidar_encoder."
    x = relu_bn(P, e + "bn1", pyconv(P, e + "conv1", x, PY_KERNELS, (1, 1, 1, 1)), train, rec, dec)
    x = relu_bn(P, e + "bn2", pyconv(P, e + "conv2", x, PY_KERNELS, (1, 1, 1, 1)), train, rec, dec)
    x = relu_bn(P, e + "bn3", F.conv2d(x, P[e + "conv3.weight"], P[e + "conv3.bias"]), train, rec, dec)
    return maxpool(x, rec, "lidar", dec)


def encoder_layer(P, pre, x, drop, li):
    B, N, _ = x.shape
    qkv = F.linear(ln(P, pre + ".0.fn.norm", x), P[pre + ".0.fn.fn.to_qkv.weight"])
    q, k, v = (t.reshape(B, N, 4, 16).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    a = torch.softmax(q @ k.transpose(-1, -2) * 0.25, dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, N, 64)
    o = F.linear(o, P[pre + ".0.fn.fn.to_out.0.weight"], P[pre + ".0.fn.fn.to_out.0.bias"])
    x = x + _drop(drop, f"en{li}.attn", o)
    h = F.gelu(F.linear(ln(P, pre + ".1.fn.norm", x), P[pre + ".1.fn.fn.mlp.0.weight"], P[pre + ".1.fn.fn.mlp.0.bias"]))
    h = _drop(drop, f"en{li}.ff1", h)
    h = F.linear(h, P[pre + ".1.fn.fn.mlp.3.weight"], P[pre + ".1.fn.fn.mlp.3.bias"])
    return x + _drop(drop, f"en{li}.ff2", h)


def attn_pool(P, a, n, t):
    """t [B, 65, 64] -> [B, 16, 65, 4]: per head the depthwise 3x3 conv over rows 1.. as an 8x8 grid, then LayerNorm(4)"""
    B = t.shape[0]
    t = t.reshape(B, 65, 16, 4).transpose(1, 2)
    cls, g = t[:, :, :1], t[:, :, 1:]
    g = g.reshape(B * 16, 8, 8, 4).permute(0, 3, 1, 2)
    g = F.conv2d(g, P[f"{a}pool_{n}.weight"], padding=1, groups=4)
    g = g.reshape(B, 16, 4, 64).transpose(2, 3)
    return ln(P, f"{a}norm_{n}", torch.cat([cls, g], dim=2))


def hs_block(P, pre, x, i, train, noise, sel, drop, rec):
    B = x.shape[0]
    logits = F.linear(x[:, 0], P[pre + ".head_select.mlp_head.weight"], P[pre + ".head_select.mlp_head.bias"])
    v = (logits + noise[i].to(x.dtype)) / TAU if train else logits
    y = torch.sigmoid(v)
    hard = (v > 0).to(x.dtype) if sel is None else sel[i].to(x.dtype)
    rec.setdefault("gate", {})[i] = v.detach()
    s = hard - y.detach() + y
    w = s.repeat_interleave(4, dim=1)[:, None, :]            # each decision over its head's 4 channels
    a = pre + ".attn."
    y1 = ln(P, pre + ".norm1", x)
    q, k, vv = (attn_pool(P, a, n, F.linear(y1, P[f"{a}{name}.weight"]) * w)
                for n, name in (("q", "query"), ("k", "key"), ("v", "value")))
    at = torch.softmax(q @ k.transpose(-1, -2) * 0.5, dim=-1)
    at = _drop(drop, f"hs{i}.prob", at)
    o = at @ vv
    o = o + torch.cat([torch.zeros_like(q[:, :, :1]), q[:, :, 1:]], dim=2)
    o = o.transpose(1, 2).reshape(B, 65, 64)
    o = F.linear(o * w, P[a + "proj.weight"], P[a + "proj.bias"])
    x = x + _drop(drop, f"hs{i}.proj", o)
    h = F.gelu(F.linear(ln(P, pre + ".norm2", x) * w, P[pre + ".mlp.fc1.weight"], P[pre + ".mlp.fc1.bias"]))
    h = _drop(drop, f"hs{i}.fc1", h)
    h = F.linear(h, P[pre + ".mlp.fc2.weight"], P[pre + ".mlp.fc2.bias"])
    return x + _drop(drop, f"hs{i}.fc2", h)


def forward(P, hsi, lidar, train, noise=None, sel=None, drop=None, rec=None, dec=None):
    """the mixture of the two classifiers' probabilities [B, ncls]"""
    rec = {} if rec is None else rec
    en, hs = depths(P)
    B = hsi.shape[0]
    f = P["weight_hsi"] * hsi_encoder(P, hsi, train, rec, dec) + \
        P["weight_lidar"] * lidar_encoder(P, lidar, train, rec, dec)
    xc = F.linear(f.flatten(2), P["encoder_embedding.weight"], P["encoder_embedding.bias"])     # [B, 64 c, 64 j]
    xcnn = xc.transpose(1, 2)
    x = xcnn + P["encoder_pos_embed"][:, 1:]
    x = torch.cat([P["cls_token"].expand(B, 1, 64), x], dim=1) + P["encoder_pos_embed"][:, :1]
    x = _drop(drop, "emb", x)
    for li in range(en):
        x = encoder_layer(P, f"en_transformer.layers.{li}", x, drop, li)
    for i in range(hs):
        x = hs_block(P, f"HeadSelectViT.blocks.{i}", x, i, train, noise, sel, drop, rec)
    cls = ln(P, "HeadSelectViT.norm", x)[:, 0]
    p1 = torch.softmax(F.linear(ln(P, "mlp_head.0", cls), P["mlp_head.1.weight"], P["mlp_head.1.bias"]), dim=1)
    img = xc.reshape(B, 64, 8, 8)
    z = relu_bn(P, "pyconv_classifier.bn1", pyconv(P, "pyconv_classifier.conv1", img, (3, 5), (2, 2)), train, rec, dec)
    w2 = P["pyconv_classifier.conv2.0.weight"]
    p2 = torch.softmax(F.linear(z.mean((2, 3)), w2.reshape(w2.shape[0], 32), P["pyconv_classifier.conv2.0.bias"]), dim=1)
    return p1 * P["vit_cls_coefficient"] + p2 * P["cnn_cls_coefficient"]


def is_param(k):
    return not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))


def train_step(state, hsi, lidar, target, weight, noise, sel=None, drop=None, dec=None):
    """one training forward / backward in float64 -> (out, loss, {name: grad}, rec)"""
    P = {k: torch.as_tensor(v).double().clone() for k, v in state.items()}
    for k in P:
        if is_param(k):
            P[k].requires_grad_(True)
    rec = {}
    out = forward(P, hsi.double(), lidar.double(), True, noise=noise, sel=sel, drop=drop, rec=rec, dec=dec)
    loss = F.cross_entropy(out, target, weight=weight.double())     # the mixture goes in as the reference passes it
    loss.backward()
    grads = {k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])) for k in P if is_param(k)}
    return out.detach(), loss.detach(), grads, rec


def eval_forward(state, hsi, lidar, rec=None):
    P = {k: torch.as_tensor(v).double() for k, v in state.items()}
    with torch.no_grad():
        return forward(P, hsi.double(), lidar.double(), False, rec=rec)
