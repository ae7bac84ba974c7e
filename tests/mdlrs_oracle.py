"""Float64 restatement of the four MDL-RS fusion CNNs and of the cross-fusion loss from torch functional ops (the
yardstick of tests/test_mdlrs.py; it lives here because oracle/ is frozen, as tests/mft_oracle.py does).

Written from the layer trees of the reference's `model/compare_method/DML_Hong.py` and `losses.py:7-19`; it contains
none of their text.  `P` maps the reference's state_dict names to tensors; everything is differentiable through torch
autograd, so `train_step` yields the loss and every parameter gradient.  A BatchNorm that a forward applies several
times (Cross_fusion_CNN's bn4_a / bn4_b twice, bn5 / bn6 three times) updates its running statistics once per
application, in the forward's order, and counts each in num_batches_tracked.  Logits are [B, n_classes] for every B
(the reference's torch.squeeze drops the batch axis at B = 1).
"""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
KINDS = {"Early_fusion_CNN": "early", "Middle_fusion_CNN": "middle", "Late_fusion_CNN": "late",
         "Cross_fusion_CNN": "cross"}


class _Net:
    def __init__(self, P, train, dtype):
        self.P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
        self.train = train
        self.running = {}    # the running statistics / counters torch would hold after the forward
        self.pre = []        # (name, BatchNorm output in front of a ReLU), per application

    def conv(self, name, x, pad):
        return F.conv2d(x, self.P[name + ".weight"], self.P[name + ".bias"], padding=pad)

    def bn_relu(self, name, x):
        P, R = self.P, self.running
        w, b = P[name + ".weight"], P[name + ".bias"]
        if self.train:
            n = x.numel() // x.shape[1]
            mean, var = x.detach().mean((0, 2, 3)), x.detach().var((0, 2, 3), unbiased=False)
            rm = R.get(name + ".running_mean", P[name + ".running_mean"])
            rv = R.get(name + ".running_var", P[name + ".running_var"])
            R[name + ".running_mean"] = (1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean
            R[name + ".running_var"] = (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var * n / (n - 1)
            R[name + ".num_batches_tracked"] = R.get(name + ".num_batches_tracked",
                                                     P[name + ".num_batches_tracked"]) + 1
            y = F.batch_norm(x, None, None, w, b, True, 0.0, BN_EPS)
        else:
            y = F.batch_norm(x, P[name + ".running_mean"], P[name + ".running_var"], w, b, False, 0.0, BN_EPS)
        self.pre.append((name, y.detach()))
        return F.relu(y)

    def pool(self, x):
        return F.max_pool2d(x, kernel_size=2, stride=2, padding=1)

    def front(self, sfx, x):
        """conv1 .. bn3 + ReLU of one branch"""
        x = self.bn_relu("bn1" + sfx, self.conv("conv1" + sfx, x, 1))
        x = self.pool(self.bn_relu("bn2" + sfx, self.conv("conv2" + sfx, x, 0)))
        return self.bn_relu("bn3" + sfx, self.conv("conv3" + sfx, x, 1))

    def c4(self, sfx, x):
        return self.pool(self.bn_relu("bn4" + sfx, self.conv("conv4" + sfx, x, 0)))

    def tail(self, sfx, x):
        """conv5 .. bn6 + ReLU and the global average, [B, 64, 1, 1]"""
        x = self.bn_relu("bn5" + sfx, self.conv("conv5" + sfx, x, 0))
        x = self.bn_relu("bn6" + sfx, self.conv("conv6" + sfx, x, 0))
        return x.mean((2, 3), keepdim=True)

    def head(self, x):
        return self.conv("conv7", x, 0).flatten(1)


def forward(name, P, x1, x2, train=True, dtype=torch.float64):
    """logits [B, n_classes] (a tuple of three for Cross_fusion_CNN) and the net's record"""
    net = _Net(P, train, dtype)
    x1, x2 = x1.to(dtype), x2.to(dtype)
    kind = KINDS[name]
    if kind == "early":
        out = net.head(net.tail("", net.c4("", net.front("", torch.cat([x1, x2], 1)))))
    elif kind == "middle":
        a, b = net.c4("_a", net.front("_a", x1)), net.c4("_b", net.front("_b", x2))
        out = net.head(net.tail("", torch.cat([a, b], 1)))
    elif kind == "late":
        a = net.tail("_a", net.c4("_a", net.front("_a", x1)))
        b = net.tail("_b", net.c4("_b", net.front("_b", x2)))
        out = net.head(torch.cat([a, b], 1))
    else:
        a, b = net.front("_a", x1), net.front("_b", x2)
        x11, x22, x12, x21 = net.c4("_a", a), net.c4("_b", b), net.c4("_b", a), net.c4("_a", b)
        joint = (torch.cat([x11 + x21, x22 + x12], 1), torch.cat([x11, x12], 1), torch.cat([x22, x21], 1))
        out = tuple(net.head(net.tail("", j)) for j in joint)
    return out, net


def loss_fn(name, out, target, weight):
    """weighted mean cross entropy; Cross_fusion_CNN: + the two mean squared differences to the first output"""
    if KINDS[name] != "cross":
        return F.cross_entropy(out, target, weight=weight.to(out.dtype))
    o1, o2, o3 = out
    return F.cross_entropy(o1, target, weight=weight.to(o1.dtype)) + ((o1 - o2) ** 2).mean() + ((o1 - o3) ** 2).mean()


def train_step(name, sd, x1, x2, target, weight, dtype=torch.float64):
    """one train-mode forward / backward from the state dict: (logits, loss, grads, running, pre)"""
    P = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
             else v.detach().clone()) for k, v in sd.items()}
    out, net = forward(name, P, x1, x2, True, dtype)
    loss = loss_fn(name, out, target, weight)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in net.P.items() if v.requires_grad}
    det = tuple(o.detach() for o in out) if isinstance(out, tuple) else out.detach()
    return det, loss.detach(), grads, {k: v.detach() for k, v in net.running.items()}, net.pre


def eval_logits(name, sd, x1, x2, dtype=torch.float64):
    with torch.no_grad():
        out, _ = forward(name, sd, x1, x2, False, dtype)
    return out
