"""GLT-Net comparison model (the global-local transformer, HSI + LiDAR at three scales) on the MI355X path.

Reference: `model/compare_method/GLT_Net/GLT_Net.py` (`GLT` :310-422, `CNN_Encoder` :24-100, `CNN_Decoder` :103-151,
`CNN_Classifier` :154-173, `SA_GDR` :176-206, `Transformer` :287-307).  The reference's forward takes the HSI and the
LiDAR patch at three sizes P, 2P, 3P around one pixel, and its training loop (`utils.py:train_patch`) cuts the window
`[c - p/2, c + p/2)` for each: the P and 2P windows are the centre crops, at offsets P and P/2, of the 3P window.  So here

    forward(x1 [B, l1, 3P, 3P], x2 [B, l2, 3P, 3P]) -> (x_cls [B, num_classes], con_loss [])

takes ONE 3P patch per modality (what `PatchBatcher` cuts for patch_size 3P) and the device cuts the six inputs
(`vc_glt_crops`).  Both outputs are returned in training and in eval, as the reference returns them; `GLT_Loss` adds the
reconstruction loss to the cross entropy.  x_cls is raw logits plus probabilities (`mlp_head(cls) * coefficient1 +
softmax(cnn_classifier(x_cnn)) * coefficient2`), as in the reference.

The module keeps the reference's parameter tree, creation order and initialisers, so `state_dict()` has the reference's
keys in order, `.pth` files interchange and the same `torch.manual_seed` draws the same initial values.  Both
transformers' `skipcat` convolutions are never used by the reference's forward: they stay in the state_dict, get a zero
gradient and are left bit-unchanged by the fused Adam.

Forward and backward are one hand-written program of HIP kernels over channels-last rows: the
encoder's 3x3 convs through `vc_conv3x3_tap_*` with `vc_bn_*_ex` (the shared `conv1` / `conv2` run once per scale:
three BatchNorm applications with their own batch statistics, the running statistics updated in scale order and the
weight gradients summed in scale order), `vc_maxpool2_*`, then `vc_glt_fuse_*` (fusion scalars, the three spatial
Linears, SA-GDR, tokens), both transformers on S2EFT's kernels (`vc_s2eft_attn_*`: 4 heads of 16 at width 64 and at
width 32), the six decoder convolutions with their nearest upsample folded into the implicit GEMM
(`vc_glt_upconv_*`), `vc_glt_sigmse_*` for the six reconstruction terms and `vc_glt_tail_*` for the classifier mix.

Supported: even patch_size 2..8, num_patches == patch_size ** 2, encoder_embed_dim 64, heads 4 of dim_head 16 for both
transformers; any band counts and depths.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program
from ._lib import lib
from .flat import F32, FlatParams

LN_EPS = 1e-5
DIM = 64            # encoder width = the channels of seq2img(x_cnn) = decoder_pred1's outputs
HEADS, DIM_HEAD = program.ATTN_HEADS, program.ATTN_DIM_HEAD
P_MAX = 8           # vc_glt_fuse_*: the sample's fused maps in LDS
NCLS_MAX = 256      # vc_glt_tail_*


# ---------------------------------------------------------------- parameter tree (reference names)
def _cbr(cin, cout, k, pad, pool):
    mods = [nn.Conv2d(cin, cout, k, 1, pad), nn.BatchNorm2d(cout), nn.ReLU()]
    return nn.Sequential(*(mods + ([nn.MaxPool2d(2)] if pool else [])))


class CNN_Encoder(nn.Module):
    def __init__(self, l1, l2):
        super().__init__()
        self.conv1 = _cbr(l1, 32, 3, 1, False)
        self.conv2 = _cbr(l2, 32, 3, 1, False)
        for k in (1, 2, 3):
            setattr(self, f"conv1_{k}", _cbr(32, 64, 3, 1, True))
            setattr(self, f"conv2_{k}", _cbr(32, 64, 3, 1, True))
        self.xishu1 = nn.Parameter(torch.Tensor([0.5]))
        self.xishu2 = nn.Parameter(torch.Tensor([0.5]))


class CNN_Decoder(nn.Module):
    def __init__(self, l1, l2):
        super().__init__()
        for i in range(6):
            s, cout = i // 2 + 1, (l1, l2)[i % 2]
            up = [nn.Upsample(scale_factor=s)] if s > 1 else []
            setattr(self, f"dconv{i + 1}", nn.Sequential(*up, nn.Conv2d(64, cout, 3, 1, 1), nn.Sigmoid()))


class CNN_Classifier(nn.Module):
    def __init__(self, classes):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(64, 32, 1), nn.BatchNorm2d(32), nn.ReLU(), nn.AdaptiveAvgPool2d(1))
        self.conv2 = nn.Sequential(nn.Conv2d(32, classes, 1))


class SA_GDR(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        self.conv = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()


class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class FeedForward(nn.Module):
    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden_dim, dim),
                                 nn.Dropout(dropout))


class Attention(nn.Module):
    def __init__(self, dim, heads, dim_head, dropout):
        super().__init__()
        inner = dim_head * heads
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_head, dropout, num_channel):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Residual(PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout))),
                Residual(PreNorm(dim, FeedForward(dim, mlp_head, dropout=dropout)))]))
        self.skipcat = nn.ModuleList([])   # never used by the forward (zero gradient), kept for the state_dict
        for _ in range(depth - 2):
            self.skipcat.append(nn.Conv2d(num_channel + 1, num_channel + 1, [1, 2], 1, 0))


class GLT(FlatParams, nn.Module):
    """Same constructor as the reference `GLT` (GLT_Net.py:311-312); forward(x1 [B, l1, 3P, 3P], x2 [B, l2, 3P, 3P]) ->
    (x_cls [B, num_classes], con_loss [])."""

    def __init__(self, l1, l2, patch_size, num_patches, num_classes, encoder_embed_dim, decoder_embed_dim, en_depth,
                 en_heads, de_depth, de_heads, mlp_dim, dim_head=16, dropout=0., emb_dropout=0.):
        super().__init__()
        _check_supported(l1, l2, patch_size, num_patches, num_classes, encoder_embed_dim, decoder_embed_dim, en_depth,
                         en_heads, de_depth, de_heads, mlp_dim, dim_head, dropout, emb_dropout)
        self.l1, self.l2, self.ncls = l1, l2, num_classes
        self.en_depth, self.de_depth, self.mlp_dim, self.de_dim = en_depth, de_depth, mlp_dim, decoder_embed_dim
        # creation order = the reference's, so the default initialisation draws the same numbers
        self.cnn_encoder = CNN_Encoder(l1, l2)
        self.cnn_decoder = CNN_Decoder(l1, l2)
        self.cnn_classifier = CNN_Classifier(num_classes)
        self.coefficient1 = nn.Parameter(torch.Tensor([0.5]))
        self.coefficient2 = nn.Parameter(torch.Tensor([0.5]))
        self.sa_gdr = SA_GDR()
        self.loss_fun2 = nn.MSELoss()
        self.num_patches = num_patches
        self.patch_size = patch_size
        self.encoder_embed_dim = encoder_embed_dim
        self.encoder_pos_embed = nn.Parameter(torch.randn(1, patch_size ** 2 + 1, encoder_embed_dim))
        self.decoder_pos_embed = nn.Parameter(torch.randn(1, patch_size ** 2 + 1, decoder_embed_dim))
        for k in (1, 2, 3):
            setattr(self, f"encoder_embedding{k}", nn.Linear(((patch_size // 2) * k) ** 2, patch_size ** 2))
        self.decoder_embedding = nn.Linear(encoder_embed_dim, decoder_embed_dim, bias=True)
        self.cls_token = nn.Parameter(torch.randn(1, 1, encoder_embed_dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.en_transformer = Transformer(encoder_embed_dim, en_depth, en_heads, dim_head, mlp_dim, dropout, num_patches)
        self.de_transformer = Transformer(decoder_embed_dim, de_depth, de_heads, dim_head, mlp_dim, dropout, num_patches)
        self.decoder_pred1 = nn.Linear(decoder_embed_dim, 64, bias=True)
        self.to_latent = nn.Identity()
        self.mlp_head = nn.Sequential(nn.LayerNorm(encoder_embed_dim), nn.Linear(encoder_embed_dim, num_classes))
        self._build_flat()

    def forward(self, x1: torch.Tensor, x2: torch.Tensor):
        _check_inputs(self, x1, x2)
        if x1.device.type != "cuda" or x2.device.type != "cuda":
            raise RuntimeError("GLT MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        x1 = x1.detach().to(torch.float32).contiguous()
        x2 = x2.detach().to(torch.float32).contiguous()
        return program.run(self, _Program, x1, x2)


def _check_inputs(m, x1, x2):
    """host-side shape checks of forward (no device needed)"""
    S = 3 * m.patch_size
    if x1.dim() != 4 or x1.shape[1] != m.l1 or tuple(x1.shape[2:]) != (S, S):
        raise RuntimeError(f"GLT: expected x1 [B, {m.l1}, {S}, {S}] (the 3 * patch_size window; the P and 2P inputs are "
                           f"its centre crops), got {list(x1.shape)}")
    if x2.dim() != 4 or tuple(x2.shape) != (x1.shape[0], m.l2, S, S):
        raise RuntimeError(f"GLT: expected x2 [B, {m.l2}, {S}, {S}] matching x1, got {list(x2.shape)}")
    if x1.shape[0] < 1:
        raise RuntimeError("empty batch")


def _check_supported(l1, l2, patch_size, num_patches, num_classes, dim, de_dim, en_depth, en_heads, de_depth, de_heads,
                     mlp_dim, dim_head, dropout, emb_dropout):
    """reject what the reference itself cannot run or a kernel cannot take, at construction"""
    pre = "GLT MI355X path: "
    if patch_size % 2 or not 2 <= patch_size <= P_MAX:
        raise ValueError(f"{pre}patch_size must be even (the reference's encoder_embedding2 takes ((P // 2) * 2) ** 2 "
                         f"inputs, the pooled 2P map has P ** 2) and in 2..{P_MAX}, got {patch_size}")
    if dim != DIM:
        raise ValueError(f"{pre}encoder_embed_dim must be {DIM} (CNN_Classifier takes 64 channels from seq2img), got {dim}")
    if num_patches != patch_size ** 2:
        raise ValueError(f"{pre}num_patches must be patch_size ** 2 = {patch_size ** 2}, got {num_patches}")
    if (en_heads, de_heads, dim_head) != (HEADS, HEADS, DIM_HEAD):
        raise ValueError(f"{pre}en_heads, de_heads, dim_head must be {(HEADS, HEADS, DIM_HEAD)} (vc_s2eft_attn_*), got "
                         f"{(en_heads, de_heads, dim_head)}")
    if l1 < 1 or l2 < 1 or not 1 <= num_classes <= NCLS_MAX:
        raise ValueError(f"GLT: band counts must be positive and num_classes in 1..{NCLS_MAX}")
    if en_depth < 0 or de_depth < 0 or mlp_dim < 1 or de_dim < 1:
        raise ValueError("GLT: depths >= 0, mlp_dim and decoder_embed_dim >= 1")
    if not all(0.0 <= p < 1.0 for p in (dropout, emb_dropout)):
        raise ValueError("GLT: every dropout probability must be in [0, 1)")


class _Program(program.Program):
    NAME = "GLT"
    LN_EPS = LN_EPS

    def __init__(self, m: GLT, needs_grad, x1, x2):
        super().__init__(lib(), m, needs_grad, x1, x2)
        self.x1, self.x2 = x1, x2
        self.Pn = m.patch_size
        self.NP = self.Pn ** 2
        self.T = self.NP + 1
        # ONE workspace for the GEMMs' / convs' split-K slabs, BatchNorm and colsum partials and the fp64 MSE partials:
        # every launch of the program is on one stream, in order, and each kernel has consumed its partials when it ends
        self.scratch(1 << 22, grow=True)
        self.seed_dropout(self.train)

    # ------------------------------------------------------------ helpers
    def count_batches(self):
        """the shared conv1 / conv2 BatchNorms ran three times: num_batches_tracked += 3, each tensor once per launch"""
        seen = {}
        for t in self.nbt:
            seen.setdefault(id(t), [t, 0])[1] += 1
        for n in sorted({c for _, c in seen.values()}):
            torch._foreach_add_([t for t, c in seen.values() if c == n], n)

    def transformer(self, tag, D):
        """`{tag}_transformer` (GLT_Net.py:287-307), of width D over the T tokens, as program.encoder_fwd / _bwd take it"""
        return dict(prefix=f"{tag}_transformer", T=self.T, D=D, hidden=self.m.mlp_dim, ff="net", site=tag)

    def conv(self, S, C, O, x, ldx, wt, bias):
        y = self.new(self.B * S * S, O)
        self.L.vc_conv3x3_tap_fwd(self.B, S, S, C, O, 1, x.data_ptr(), ldx, wt.data_ptr(), self.P[bias], y.data_ptr(), O,
                                  self.scr.data_ptr(), self.SCRATCH, self.s)
        return y

    # ------------------------------------------------------------ forward
    def _forward(self):
        m, L, B, P, s = self.m, self.L, self.B, self.P, self.s
        Pn, NP, T = self.Pn, self.NP, self.T
        sv = self.sv = {}
        enc = m.cnn_encoder
        # the six inputs: the centre crops of the two 3P patches, as channels-last rows padded to 4 floats
        rows = []
        for x, C in ((self.x1, m.l1), (self.x2, m.l2)):
            ld = (C + 3) // 4 * 4
            r = [self.new(B * (k * Pn) ** 2, ld) for k in (1, 2, 3)]
            L.vc_glt_crops(B, C, Pn, x.data_ptr(), r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), ld, s)
            rows.append((r, ld, C))
        sv["rows"] = rows
        # CNN encoder (GLT_Net.py:79-100): conv1 / conv2 shared by the three scales, one BatchNorm application each
        pooled, sv["enc"] = [[None] * 3, [None] * 3], [[None] * 3, [None] * 3]
        for mi, (r, ld, C) in enumerate(rows):
            name = f"cnn_encoder.conv{mi + 1}"
            wt0 = self.pack3x3(name + ".0.weight", 32, C)
            for k in range(3):
                S = (k + 1) * Pn
                M = B * S * S
                y = self.conv(S, C, 32, r[k], ld, wt0, name + ".0.bias")
                z, mean, inv = self.bn(name + ".1", getattr(enc, f"conv{mi + 1}")[1], y, M, 32)
                nk = f"{name}_{k + 1}"
                wt1 = self.pack3x3(nk + ".0.weight", 64, 32)
                y2 = self.conv(S, 32, 64, z, 32, wt1, nk + ".0.bias")
                z2, mean2, inv2 = self.bn(nk + ".1", getattr(enc, f"conv{mi + 1}_{k + 1}")[1], y2, M, 64)
                pl, arg = self.new(M // 4, 64), self.bytes(M // 4, 64)
                L.vc_maxpool2_fwd(B, S, S, 64, z2.data_ptr(), 64, pl.data_ptr(), arg.data_ptr(), s)
                pooled[mi][k] = pl
                sv["enc"][mi][k] = dict(y=y, z=z, mean=mean, inv=inv, wt1=wt1, y2=y2, mean2=mean2, inv2=inv2, arg=arg)
        # fusion, the spatial embeddings, SA-GDR and the tokens (:343-367), one launch
        xcnn, X0, e = self.new(B * NP, DIM), self.new(B * T, DIM), self.new(3, B, NP, DIM)
        pa, pb = pooled
        L.vc_glt_fuse_fwd(B, Pn, pa[0].data_ptr(), pb[0].data_ptr(), pa[1].data_ptr(), pb[1].data_ptr(),
                          pa[2].data_ptr(), pb[2].data_ptr(), P["cnn_encoder.xishu1"], P["cnn_encoder.xishu2"],
                          P["encoder_embedding1.weight"], P["encoder_embedding1.bias"], P["encoder_embedding2.weight"],
                          P["encoder_embedding2.bias"], P["encoder_embedding3.weight"], P["encoder_embedding3.bias"],
                          P["sa_gdr.conv.weight"], P["encoder_pos_embed"], P["cls_token"], xcnn.data_ptr(),
                          X0.data_ptr(), e.data_ptr(), s)
        self.pe = self.drop_p(m.dropout)
        X = self.dropped("emb", X0, None, B * T * DIM, self.pe, DIM)
        sv.update(pooled=pooled, xcnn=xcnn, e=e)
        self.lay = {}
        X, self.lay["en"] = self.encoder_fwd(X, layers=m.en_transformer.layers, **self.transformer("en", DIM))
        # decoder (:387-415): embedding + position rows, the width-32 transformer, the prediction back to 64 channels
        R, Dd = B * T, m.de_dim
        D0 = self.linear(X, R, DIM, Dd, "decoder_embedding", add=P["decoder_pos_embed"], add_ld=Dd, add_mod=T)
        Dl, self.lay["de"] = self.encoder_fwd(D0, layers=m.de_transformer.layers, **self.transformer("de", Dd))
        Yp = self.linear(Dl, R, Dd, DIM, "decoder_pred1")
        xcon = self.new(B * NP, DIM)     # the token rows without cls = the [B, 64, P, P] map, channels-last
        L.vc_add2_2d(B, NP * DIM, Yp.data_ptr() + F32 * DIM, T * DIM, None, 0, xcon.data_ptr(), NP * DIM, 0.0, s)
        con = self.new(())
        dec = []
        for i in range(6):
            sc, (r, ld, C) = i // 2 + 1, rows[i % 2]
            nm = f"cnn_decoder.dconv{i + 1}.{0 if sc == 1 else 1}"
            wt = self.pack3x3(nm + ".weight", C, DIM)
            n = B * (sc * Pn) ** 2
            y = self.new(n, ld)
            L.vc_glt_upconv_fwd(B, Pn, sc, DIM, C, xcon.data_ptr(), DIM, wt.data_ptr(), P[nm + ".bias"], y.data_ptr(), ld,
                                self.scr.data_ptr(), self.SCRATCH, s)
            # sigmoid in place, the term's mean squared error against the crop added to con_loss with weight 1/6
            L.vc_glt_sigmse_fwd(n, C, y.data_ptr(), ld, r[sc - 1].data_ptr(), ld, 1.0 / 6.0, 1 if i else 0,
                                con.data_ptr(), self.scr.data_ptr(), self.SCRATCH, self.cnt, s)
            dec.append((nm, sc, C, ld, wt, y, r[sc - 1]))
        # classifier (:373-385): mlp_head on the cls row, the CNN classifier on the position-free x_cnn
        Yc, muc, rsc = self.ln("mlp_head.0", X.data_ptr(), B, T * DIM, DIM)
        lg1 = self.linear(Yc, B, DIM, m.ncls, "mlp_head.1")
        yc = self.linear(xcnn, B * NP, DIM, 32, "cnn_classifier.conv1.0")
        zc, meanc, invc = self.bn("cnn_classifier.conv1.1", m.cnn_classifier.conv1[1], yc, B * NP, 32)
        n = m.ncls
        p2, avg, out = self.new(B, n), self.new(B, 32), self.new(B, n)
        L.vc_glt_tail_fwd(B, n, NP, lg1.data_ptr(), zc.data_ptr(), 32, P["cnn_classifier.conv2.0.weight"],
                          P["cnn_classifier.conv2.0.bias"], P["coefficient1"], P["coefficient2"], p2.data_ptr(),
                          avg.data_ptr(), out.data_ptr(), s)
        sv.update(Xlast=X, Dl=Dl, xcon=xcon, dec=dec, Yc=Yc, muc=muc, rsc=rsc, lg1=lg1, yc=yc, meanc=meanc, invc=invc,
                  p2=p2, avg=avg)
        return out, con

    # ------------------------------------------------------------ backward
    def backward(self, dout, dcon):
        """the flat gradient of every parameter, each written once"""
        m, L, B, P, s = self.m, self.L, self.B, self.P, self.s
        Pn, NP, T = self.Pn, self.NP, self.T
        sv = self.sv
        R, Dd, n = B * T, m.de_dim, m.ncls
        grad = self.new_grad()
        G = self.G
        scr, ns = self.scr.data_ptr(), self.SCRATCH
        # classifier tail
        dlg1, dzc = self.new(B, n), self.new(B * NP, 32)
        wt = n * 33 + 2
        part = self.new(B, wt)
        L.vc_glt_tail_bwd(B, n, NP, dout.data_ptr(), sv["lg1"].data_ptr(), sv["p2"].data_ptr(), sv["avg"].data_ptr(),
                          P["cnn_classifier.conv2.0.weight"], P["coefficient1"], P["coefficient2"], dlg1.data_ptr(),
                          dzc.data_ptr(), 32, part.data_ptr(), s)
        self.reduce_part(part, wt, 0, n * 32, G["cnn_classifier.conv2.0.weight"])
        self.reduce_part(part, wt, n * 32, n, G["cnn_classifier.conv2.0.bias"])
        self.reduce_part(part, wt, n * 33, 1, G["coefficient1"])
        self.reduce_part(part, wt, n * 33 + 1, 1, G["coefficient2"])
        dyc = self.bn_bwd("cnn_classifier.conv1.1", dzc, sv["yc"], sv["meanc"], sv["invc"], B * NP, 32)
        dxcnn = self.linear_bwd(dyc, sv["xcnn"], B * NP, DIM, 32, "cnn_classifier.conv1.0")
        # transformer head on the cls rows; every other row of dX starts at zero
        dYc = self.linear_bwd(dlg1, sv["Yc"], B, DIM, n, "mlp_head.1")
        dX = self.new(R, DIM)
        L.vc_fill(R * DIM, dX.data_ptr(), 0.0, s)
        self.ln_bwd("mlp_head.0", dYc, sv["Xlast"].data_ptr(), T * DIM, sv["muc"], sv["rsc"], B, DIM, dX.data_ptr(),
                    T * DIM, 0.0)
        # reconstruction: the six decoder branches accumulate into one dxcon, in branch order
        dxcon = self.new(B * NP, DIM)
        for i, (nm, sc, C, ld, wtp, y, tgt) in enumerate(sv["dec"]):
            rows = B * (sc * Pn) ** 2
            L.vc_glt_sigmse_bwd(rows, C, y.data_ptr(), ld, tgt.data_ptr(), ld, 1.0 / 6.0, dcon.data_ptr(), y.data_ptr(),
                                ld, s)
            L.vc_glt_upconv_wgrad(B, Pn, sc, DIM, C, sv["xcon"].data_ptr(), DIM, y.data_ptr(), ld, G[nm + ".weight"],
                                  G[nm + ".bias"], scr, ns, s)
            L.vc_glt_upconv_dgrad(B, Pn, sc, DIM, C, y.data_ptr(), ld, wtp.data_ptr(), 1.0 if i else 0.0,
                                  dxcon.data_ptr(), DIM, scr, ns, s)
        dYp = self.new(R, DIM)
        L.vc_fill_2d(B, DIM, dYp.data_ptr(), T * DIM, 0.0, s)
        L.vc_add2_2d(B, NP * DIM, dxcon.data_ptr(), NP * DIM, None, 0, dYp.data_ptr() + F32 * DIM, T * DIM, 0.0, s)
        dD = self.linear_bwd(dYp, sv["Dl"], R, Dd, DIM, "decoder_pred1")
        dD = self.encoder_bwd(dD, self.lay["de"], **self.transformer("de", Dd))
        L.vc_colsum(B, T * Dd, dD.data_ptr(), T * Dd, G["decoder_pos_embed"], 0.0, scr, ns, s)
        self.linear_bwd(dD, sv["Xlast"], R, DIM, Dd, "decoder_embedding", dx=dX.data_ptr(), lddx=DIM, beta=1.0)
        dX = self.encoder_bwd(dX, self.lay["en"], **self.transformer("en", DIM))
        # tokens, SA-GDR, the spatial embeddings and the fusion
        dX0 = self.drop_bwd("emb", dX, R * DIM, self.pe)
        pa, pb = sv["pooled"]
        dpa = [torch.empty_like(t) for t in pa]
        dpb = [torch.empty_like(t) for t in pb]
        fw = L.vc_glt_fuse_part_floats(Pn)
        part = self.new(B, fw)
        L.vc_glt_fuse_bwd(B, Pn, pa[0].data_ptr(), pb[0].data_ptr(), pa[1].data_ptr(), pb[1].data_ptr(),
                          pa[2].data_ptr(), pb[2].data_ptr(), P["cnn_encoder.xishu1"], P["cnn_encoder.xishu2"],
                          P["encoder_embedding1.weight"], P["encoder_embedding2.weight"], P["encoder_embedding3.weight"],
                          P["sa_gdr.conv.weight"], sv["xcnn"].data_ptr(), sv["e"].data_ptr(), dX0.data_ptr(),
                          dxcnn.data_ptr(), dpa[0].data_ptr(), dpb[0].data_ptr(), dpa[1].data_ptr(), dpb[1].data_ptr(),
                          dpa[2].data_ptr(), dpb[2].data_ptr(), part.data_ptr(), s)
        off = 0
        for k in range(3):
            nk = ((k + 1) * Pn // 2) ** 2
            self.reduce_part(part, fw, off, NP * nk, G[f"encoder_embedding{k + 1}.weight"])
            self.reduce_part(part, fw, off + NP * nk, NP, G[f"encoder_embedding{k + 1}.bias"])
            off += NP * nk + NP
        self.reduce_part(part, fw, off, 98, G["sa_gdr.conv.weight"])
        self.reduce_part(part, fw, off + 98, 1, G["cnn_encoder.xishu1"])
        self.reduce_part(part, fw, off + 99, 1, G["cnn_encoder.xishu2"])
        # position rows: row 0 was added to every token row, rows 1.. to their own; cls
        L.vc_colsum(R, DIM, dX0.data_ptr(), DIM, G["encoder_pos_embed"], 0.0, scr, ns, s)
        L.vc_colsum(B, NP * DIM, dX0.data_ptr() + F32 * DIM, T * DIM, G["encoder_pos_embed"] + F32 * DIM, 0.0, scr, ns, s)
        L.vc_colsum(B, DIM, dX0.data_ptr(), T * DIM, G["cls_token"], 0.0, scr, ns, s)
        # CNN encoder (the inputs are data: no input gradient); the shared convs' gradients summed in scale order
        for mi, (r, ld, C) in enumerate(sv["rows"]):
            name = f"cnn_encoder.conv{mi + 1}"
            nw = 32 * C * 9
            tmp = self.new(nw + 32)
            for k in range(3):
                S = (k + 1) * Pn
                M = B * S * S
                st = sv["enc"][mi][k]
                nk = f"{name}_{k + 1}"
                dz2 = self.new(M, 64)
                L.vc_maxpool2_bwd(B, S, S, 64, (dpa, dpb)[mi][k].data_ptr(), st["arg"].data_ptr(), dz2.data_ptr(), 64, s)
                dy2 = self.bn_bwd(nk + ".1", dz2, st["y2"], st["mean2"], st["inv2"], M, 64)
                L.vc_conv3x3_tap_wgrad_oihw(B, S, S, 32, 64, 1, st["z"].data_ptr(), 32, dy2.data_ptr(), 64,
                                            G[nk + ".0.weight"], G[nk + ".0.bias"], scr, ns, s)
                dz = self.new(M, 32)
                L.vc_conv3x3_tap_dgrad(B, S, S, 32, 64, 1, dy2.data_ptr(), 64, st["wt1"].data_ptr(), 0.0, dz.data_ptr(),
                                       32, scr, ns, s)
                dy = self.bn_bwd(name + ".1", dz, st["y"], st["mean"], st["inv"], M, 32, beta_w=1.0 if k else 0.0)
                if k == 0:
                    L.vc_conv3x3_tap_wgrad_oihw(B, S, S, C, 32, 1, r[k].data_ptr(), ld, dy.data_ptr(), 32,
                                                G[name + ".0.weight"], G[name + ".0.bias"], scr, ns, s)
                else:
                    L.vc_conv3x3_tap_wgrad_oihw(B, S, S, C, 32, 1, r[k].data_ptr(), ld, dy.data_ptr(), 32,
                                                tmp.data_ptr(), tmp.data_ptr() + F32 * nw, scr, ns, s)
                    L.vc_add2_2d(1, nw, tmp.data_ptr(), nw, None, 0, G[name + ".0.weight"], nw, 1.0, s)
                    L.vc_add2_2d(1, 32, tmp.data_ptr() + F32 * nw, 32, None, 0, G[name + ".0.bias"], 32, 1.0, s)
        self.sv, self.lay = {}, {}
        return grad
