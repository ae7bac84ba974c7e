"""Float64 restatement of the GLT-Net comparison model and of every `vc_glt_*` kernel, from the formulas in
include/vitcnn.h (the yardstick of tests/test_glt*.py).  It contains none of the reference's text.  `P` maps the
reference's state_dict names to tensors; everything is differentiable through torch autograd, so `train_step` yields the
loss and every parameter gradient.

The model takes ONE 3P patch per modality; its three scales are the centre crops at offsets P, P/2 and 0.

Randomness enters as data: drop {site: (keep mask, p)} applied as x * mask / (1 - p); absent sites apply none.  Sites:
"emb"; per encoder layer l "en<l>.attn", "en<l>.ff1", "en<l>.ff2"; per decoder layer l "de<l>.attn", "de<l>.ff1",
"de<l>.ff2".
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM, LN_EPS = 1e-5, 0.1, 1e-5
HEADS, DIM_HEAD = 4, 16


# ---------------------------------------------------------------- the kernels' formulas
def crops(x, P):
    """vc_glt_crops: the P, 2P and 3P windows around the centre of a [B, C, 3P, 3P] patch"""
    h = P // 2
    return x[:, :, P:2 * P, P:2 * P], x[:, :, h:h + 2 * P, h:h + 2 * P], x


def upconv(x, w, b, s):
    """vc_glt_upconv_fwd: y[o, y, x] = b[o] + sum_{c, dy, dx} w[o, c, dy, dx] u[c, y + dy - 1, x + dx - 1], where
    u[c, i, j] = x[c, floor(i / s), floor(j / s)] inside [0, sP) and 0 outside"""
    n = x.shape[-1]
    idx = torch.arange(s * n) // s
    return F.conv2d(x[:, :, idx][:, :, :, idx], w, b, padding=1)


def sigmse(y, t):
    """vc_glt_sigmse_fwd's term: mean((sigmoid(y) - t)^2)"""
    return ((torch.sigmoid(y) - t) ** 2).mean()


def fuse(pa, pb, xs1, xs2, W, bias, w7, pos, cls):
    """vc_glt_fuse_fwd from the pooled maps pa[k], pb[k] [B, 64, kP/2, kP/2] (k = 1, 2, 3):
         f_k = xs1 pa_k + xs2 pb_k;   e_k[b, c, j] = bias_k[j] + sum_p W_k[j, p] f_k[b, c, p]
         avg = (e_1 + e_2 + e_3) / 3, mx = max(e_1, e_2, e_3)           (per (b, c, j))
         g[b, c] = sigmoid(conv7x7([avg[b, c], mx[b, c]] as P x P maps, w7, padding 3))
         xcnn[b, j, c] = g[b, c, j];  X0[b, 0] = cls + pos[0];  X0[b, 1 + j] = xcnn[b, j] + pos[1 + j] + pos[0]
       -> (xcnn [B, P^2, 64], X0 [B, P^2 + 1, 64], e [3, B, 64, P^2])"""
    e = torch.stack([F.linear((xs1 * pa[k] + xs2 * pb[k]).flatten(2), W[k], bias[k]) for k in range(3)])
    B, C, N = e.shape[1:]
    Pn = int(round(N ** 0.5))
    am = torch.stack([e.mean(0), e.max(0).values], dim=2).reshape(B * C, 2, Pn, Pn)
    g = torch.sigmoid(F.conv2d(am, w7, padding=3)).reshape(B, C, N)
    xcnn = g.transpose(1, 2)
    x = torch.cat([cls.reshape(1, 1, C).expand(B, 1, C), xcnn + pos[1:].reshape(1, N, C)], dim=1) + pos[:1].reshape(1, 1, C)
    return xcnn, x, e


def tail(lg1, z, W2, b2, c1, c2):
    """vc_glt_tail_fwd: avg[b, k] = mean_t z[b, t, k];  p2 = softmax(W2 avg + b2);  out = c1 lg1 + c2 p2"""
    p2 = torch.softmax(F.linear(z.mean(1), W2, b2), dim=1)
    return lg1 * c1 + p2 * c2


# ---------------------------------------------------------------- the model
def depths(P):
    en = len({k.split(".")[2] for k in P if k.startswith("en_transformer.layers.")})
    de = len({k.split(".")[2] for k in P if k.startswith("de_transformer.layers.")})
    return en, de


def sites(P):
    en, de = depths(P)
    return ("emb",) + tuple(f"en{i}.{s}" for i in range(en) for s in ("attn", "ff1", "ff2")) + \
        tuple(f"de{i}.{s}" for i in range(de) for s in ("attn", "ff1", "ff2"))


def _drop(drop, site, x):
    if drop is None or site not in drop:
        return x
    mask, p = drop[site]
    return x * mask.to(x.dtype).reshape(x.shape) / (1.0 - p)


def batchnorm(P, pfx, x, train, rec):
    """BatchNorm2d: batch statistics in training, each application updating the running statistics that the one before
    left (rec["running"], rec["nbt"]); the running ones in eval.  The pre-ReLU result is appended to rec["pre"]."""
    w, b = P[pfx + ".weight"], P[pfx + ".bias"]
    run = rec.setdefault("running", {})
    rm = run.get(pfx + ".running_mean", P[pfx + ".running_mean"].to(x.dtype))
    rv = run.get(pfx + ".running_var", P[pfx + ".running_var"].to(x.dtype))
    if train:
        n = x.numel() // x.shape[1]
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        run[pfx + ".running_mean"] = (1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean.detach()
        run[pfx + ".running_var"] = (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var.detach() * n / (n - 1)
        nbt = rec.setdefault("nbt", {})
        nbt[pfx + ".num_batches_tracked"] = nbt.get(pfx + ".num_batches_tracked",
                                                    int(P[pfx + ".num_batches_tracked"])) + 1
    else:
        mean, var = rm, rv
    y = (x - mean.reshape(1, -1, 1, 1)) / torch.sqrt(var.reshape(1, -1, 1, 1) + BN_EPS) * w.reshape(1, -1, 1, 1) + \
        b.reshape(1, -1, 1, 1)
    rec.setdefault("pre", []).append(y.detach())
    return y


def conv_bn_relu(P, pfx, x, train, rec, pad=1):
    y = F.conv2d(x, P[pfx + ".0.weight"], P[pfx + ".0.bias"], padding=pad)
    return F.relu(batchnorm(P, pfx + ".1", y, train, rec))


def ln(P, pfx, x):
    return F.layer_norm(x, (x.shape[-1],), P[pfx + ".weight"], P[pfx + ".bias"], LN_EPS)


def layer(P, pre, x, drop, site):
    """one pre-norm transformer layer: 4 heads of 16 whatever the width"""
    B, N, D = x.shape
    qkv = F.linear(ln(P, pre + ".0.fn.norm", x), P[pre + ".0.fn.fn.to_qkv.weight"])
    q, k, v = (t.reshape(B, N, HEADS, DIM_HEAD).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    a = torch.softmax(q @ k.transpose(-1, -2) * DIM_HEAD ** -0.5, dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, N, HEADS * DIM_HEAD)
    o = F.linear(o, P[pre + ".0.fn.fn.to_out.0.weight"], P[pre + ".0.fn.fn.to_out.0.bias"])
    x = x + _drop(drop, site + ".attn", o)
    h = F.gelu(F.linear(ln(P, pre + ".1.fn.norm", x), P[pre + ".1.fn.fn.net.0.weight"], P[pre + ".1.fn.fn.net.0.bias"]))
    h = _drop(drop, site + ".ff1", h)
    h = F.linear(h, P[pre + ".1.fn.fn.net.3.weight"], P[pre + ".1.fn.fn.net.3.bias"])
    return x + _drop(drop, site + ".ff2", h)


def forward(P, x1, x2, train, drop=None, rec=None):
    """(x_cls [B, ncls], con_loss []) from the two 3P patches"""
    rec = {} if rec is None else rec
    en, de = depths(P)
    B = x1.shape[0]
    Pn = x1.shape[-1] // 3
    c1, c2 = crops(x1, Pn), crops(x2, Pn)
    e = "cnn_encoder."
    h1 = [None] * 3
    h2 = [None] * 3
    for k in range(3):      # conv1 / conv2 on the three scales, in the order the running statistics see them
        h1[k] = conv_bn_relu(P, e + "conv1", c1[k], train, rec)
        h2[k] = conv_bn_relu(P, e + "conv2", c2[k], train, rec)
    pa, pb = [], []
    for k in range(3):
        a = conv_bn_relu(P, f"{e}conv1_{k + 1}", h1[k], train, rec)
        b = conv_bn_relu(P, f"{e}conv2_{k + 1}", h2[k], train, rec)
        rec.setdefault("pool_in", []).extend([a.detach(), b.detach()])
        pa.append(F.max_pool2d(a, 2))
        pb.append(F.max_pool2d(b, 2))
    xcnn, x, emb = fuse(pa, pb, P[e + "xishu1"], P[e + "xishu2"],
                        [P[f"encoder_embedding{k}.weight"] for k in (1, 2, 3)],
                        [P[f"encoder_embedding{k}.bias"] for k in (1, 2, 3)], P["sa_gdr.conv.weight"],
                        P["encoder_pos_embed"][0], P["cls_token"][0, 0])
    rec["emb"] = emb.detach()
    x = _drop(drop, "emb", x)
    for li in range(en):
        x = layer(P, f"en_transformer.layers.{li}", x, drop, f"en{li}")
    # decoder: reconstruction of the six crops from the 64-channel P x P map
    d = F.linear(x, P["decoder_embedding.weight"], P["decoder_embedding.bias"]) + P["decoder_pos_embed"]
    for li in range(de):
        d = layer(P, f"de_transformer.layers.{li}", d, drop, f"de{li}")
    d = F.linear(d, P["decoder_pred1.weight"], P["decoder_pred1.bias"])[:, 1:]
    xcon = d.transpose(1, 2).reshape(B, 64, Pn, Pn)
    con = 0.0
    for i in range(6):
        y = upconv(xcon, P[f"cnn_decoder.dconv{i + 1}.{0 if i < 2 else 1}.weight"],
                   P[f"cnn_decoder.dconv{i + 1}.{0 if i < 2 else 1}.bias"], i // 2 + 1)
        con = con + sigmse(y, (c1 if i % 2 == 0 else c2)[i // 2]) / 6.0
    # classifier: the cls row's logits plus the CNN classifier's probabilities
    lg1 = F.linear(ln(P, "mlp_head.0", x[:, 0]), P["mlp_head.1.weight"], P["mlp_head.1.bias"])
    img = xcnn.transpose(1, 2).reshape(B, 64, Pn, Pn)
    z = conv_bn_relu(P, "cnn_classifier.conv1", img, train, rec, pad=0)
    w2 = P["cnn_classifier.conv2.0.weight"]
    out = tail(lg1, z.flatten(2).transpose(1, 2), w2.reshape(w2.shape[0], 32), P["cnn_classifier.conv2.0.bias"],
               P["coefficient1"], P["coefficient2"])
    return out, con


def is_param(k):
    return not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))


def train_step(state, x1, x2, target, weight, drop=None):
    """one training forward / backward in float64 -> (x_cls, con_loss, loss, {name: grad}, rec)"""
    P = {k: (torch.as_tensor(v).double().clone() if is_param(k) or not k.endswith("tracked") else torch.as_tensor(v))
         for k, v in state.items()}
    for k in P:
        if is_param(k):
            P[k].requires_grad_(True)
    rec = {}
    out, con = forward(P, x1.double(), x2.double(), True, drop=drop, rec=rec)
    loss = F.cross_entropy(out, target, weight=None if weight is None else weight.double()) + con
    loss.backward()
    grads = {k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])) for k in P if is_param(k)}
    return out.detach(), con.detach(), loss.detach(), grads, rec


def eval_forward(state, x1, x2, rec=None):
    P = {k: (torch.as_tensor(v).double() if not k.endswith("tracked") else torch.as_tensor(v)) for k, v in state.items()}
    with torch.no_grad():
        return forward(P, x1.double(), x2.double(), False, rec=rec)
