"""HSI band counts that are no multiple of 4 (Trento 63, the PCA option 30, PaviaU 103, ...): what the host side
guarantees without a GPU.  Needs the built library (the constructor asks vc_tl_check), as test_host_cpu.py does.

The flat parameter layout keeps every row at its logical width (stride = width): a band count that is no multiple
of 4 changes which kernels take their 16-byte paths, never the shapes a user sees.  For the band counts that worked
before, the flat offsets are pinned to a recording of the earlier layout (tests/golden/flat_offsets_r6.json)."""
import json
import os

import pytest
import torch

from helpers import GOLDEN

BANDS = (2, 3, 5, 30, 63, 103, 145, 511)
PATCHES = (7, 9)
C2, NCLS = 1, 7


def _model(c1, P=9):
    from vitcnn_amd import Multimodality_Mamba
    return Multimodality_Mamba(P, 1, 1, c1, C2, 32, NCLS)


def _logical_shapes(c1):
    """the state_dict shapes that depend on the HSI band count (vitcnn_amd/layers.py: hsi1 reads c1 channels, hsi2
    writes c1 channels with a NonLocal of c1 // 2 inter-channels, fusion2 reads c1 + 32)"""
    ci = c1 // 2
    nl = "hsi2.FusionLayer.cross_attention."
    out = {
        "hsi1.global_view.patch_embed.projection.weight": (144, c1, 1, 1),
        "hsi1.local_feature.bn.weight": (c1,), "hsi1.local_feature.bn.bias": (c1,),
        "hsi1.local_feature.bn.running_mean": (c1,), "hsi1.local_feature.bn.running_var": (c1,),
        "hsi1.local_feature.conv.weight": (256, c1, 3, 3),
        "hsi1.channel_feature.weight": (256, c1, 1, 1),
        "hsi2.change_dim.weight": (c1, 256, 1, 1), "hsi2.change_dim.bias": (c1,),
        "hsi2.ln3.weight": (c1,), "hsi2.ln3.bias": (c1,), "hsi2.ln4.weight": (c1,), "hsi2.ln4.bias": (c1,),
        "hsi2.local_feature.conv.weight": (c1, 256, 3, 3), "hsi2.local_feature.conv.bias": (c1,),
        "hsi2.channel_feature.weight": (c1, 256, 1, 1), "hsi2.channel_feature.bias": (c1,),
        nl + "theta.weight": (ci, c1, 1, 1), nl + "theta.bias": (ci,),
        nl + "phi.0.weight": (ci, c1, 1, 1), nl + "phi.0.bias": (ci,),
        nl + "g.0.weight": (ci, c1, 1, 1), nl + "g.0.bias": (ci,),
        nl + "W.0.weight": (c1, ci, 1, 1), nl + "W.0.bias": (c1,),
        nl + "W.1.weight": (c1,), nl + "W.1.bias": (c1,), nl + "W.1.running_mean": (c1,),
        "hsi2.FusionLayer.FusionLayer.0.weight": (c1, 2 * c1, 1, 1), "hsi2.FusionLayer.FusionLayer.1.weight": (c1,),
        "hsi2.fusion.FusionLayer.0.weight": (c1, 2 * c1, 1, 1), "hsi2.fusion.FusionLayer.1.running_var": (c1,),
        "fusion2.FusionLayer.0.weight": (128, c1 + 32, 1, 1),
        "fusion1.FusionLayer.0.weight": (128, 256 + 16, 1, 1),
        "classifier.weight": (NCLS, 128),
    }
    return out


@pytest.fixture(scope="module")
def models():
    return {(c1, P): _model(c1, P) for c1 in BANDS for P in PATCHES}


@pytest.mark.parametrize("P", PATCHES)
@pytest.mark.parametrize("c1", BANDS)
def test_constructs_with_logical_shapes(models, c1, P):
    m = models[(c1, P)]
    sd = m.state_dict()
    for k, shape in _logical_shapes(c1).items():
        assert tuple(sd[k].shape) == shape, (k, tuple(sd[k].shape), shape)
    named = dict(m.named_parameters())
    assert named.keys() == dict(torch.nn.Module.named_parameters(models[(BANDS[0], P)])).keys()
    for k, p in named.items():   # the parameter views have the logical shapes too
        assert p.dtype == torch.float32 and p.is_contiguous()
        assert tuple(p.shape) == tuple(sd[k].shape)
    assert sum(p.numel() for p in named.values()) == m._n_elems


def test_one_band_is_rejected_with_a_reason():
    with pytest.raises(ValueError, match="inter-channels"):
        _model(1)
    with pytest.raises(ValueError, match="bands"):
        _model(513)


@pytest.mark.parametrize("P", PATCHES)
@pytest.mark.parametrize("c1", BANDS)
def test_large_parameters_are_16_byte_aligned_and_gaps_are_zero(models, c1, P):
    from vitcnn_amd.model import ALIGN_MIN, PARAM_ALIGN
    m = models[(c1, P)]
    assert m.flat_params.data_ptr() % 16 == 0
    covered = torch.zeros(m._n_params, dtype=torch.bool)
    for n, p in torch.nn.Module.named_parameters(m):
        off = m._poff[n]
        if p.numel() >= ALIGN_MIN:
            assert off % PARAM_ALIGN == 0, (n, off)
        assert p.data_ptr() == m.flat_params.data_ptr() + 4 * off
        assert not covered[off:off + p.numel()].any(), n   # no overlap
        covered[off:off + p.numel()] = True
    gaps = (~covered[:m._n_active]).nonzero().flatten().tolist()
    assert gaps == list(m._gaps)
    assert float(m.flat_params.detach()[~covered].abs().sum()) == 0.0
    # the stacked phi | g product is used exactly where its four tensors are adjacent
    for pfx in ("hsi1", "hsi2"):
        nl = pfx + ".FusionLayer.cross_attention."
        w, g, b, gb = (m._poff[nl + k] for k in ("phi.0.weight", "g.0.weight", "phi.0.bias", "g.0.bias"))
        cout = c1 if pfx == "hsi2" else 256
        ci = cout // 2
        assert m._pg_stacked[pfx] == (g == w + ci * cout and b == g + ci * cout and gb == b + ci)
    assert m._pg_stacked["hsi1"]


@pytest.mark.parametrize("c1", (5, 30, 63, 103))
def test_checkpoint_round_trip_holds_no_padding(models, c1, tmp_path, monkeypatch):
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.hashinit import fill_module_
    monkeypatch.chdir(tmp_path)
    m = _model(c1)
    fill_module_(m)
    assert m._n_params > m._n_elems          # this layout does have alignment gaps
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    path = mu.save_model("bands", m, "Multimodality_Mamba", "synthetic", "train", "best", run=0, epoch=1, metric=0.5)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    assert list(loaded.keys()) == list(sd.keys())
    for k, v in sd.items():
        assert loaded[k].dtype == v.dtype and tuple(loaded[k].shape) == tuple(v.shape) and torch.equal(loaded[k], v), k
    # the file's parameter storage holds the parameters' elements and nothing else
    pk = next(k for k in loaded if k in m._poff)
    assert loaded[pk].untyped_storage().nbytes() == 4 * m._n_elems
    snap = m.snapshot_state_dict()
    assert all(torch.equal(snap[k], sd[k]) and tuple(snap[k].shape) == tuple(sd[k].shape) for k in sd)
    m2 = _model(c1)
    m2.load_state_dict(loaded)
    assert torch.equal(m2.flat_params.detach(), m.flat_params.detach())   # gaps included: still zero
    for a, b in zip(m2.flat_buffers(), m.flat_buffers()):
        assert torch.equal(a, b)
    gaps = torch.tensor(m2._gaps, dtype=torch.long)
    assert float(m2.flat_params.detach()[gaps].abs().sum()) == 0.0


def test_flat_offsets_of_supported_band_counts_are_unchanged():
    """(144, 1, 9) and (64, 2, 11): every parameter's flat offset as recorded before band counts that are no
    multiple of 4 were supported"""
    from vitcnn_amd import Multimodality_Mamba
    with open(os.path.join(GOLDEN, "flat_offsets_r6.json")) as f:
        rec = json.load(f)
    for key, r in rec.items():
        c1, c2, P = (int(v) for v in key.split(","))
        m = Multimodality_Mamba(P, 1, 1, c1, c2, 32, 16)
        assert m._pnames == r["names"]
        assert [m._poff[n] for n in r["names"]] == r["offsets"]
        assert (m._n_params, m._n_active, len(m._gaps)) == (r["n_params"], r["n_active"], r["gaps"])
        assert all(m._pg_stacked.values())


@pytest.mark.parametrize("c1", BANDS)
def test_gradient_buckets_tile_the_flat_layout(models, c1):
    """data parallelism needs nothing new: the three gradient buckets are contiguous and cover [0, n_active), gaps
    (zero in every rank's gradient) included"""
    from vitcnn_amd import parallel
    m = models[(c1, 9)]
    r = parallel.bucket_ranges(m)
    spans = sorted(r.values())
    assert spans[0][0] == 0 and spans[-1][1] == m.n_active_params
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_get_model_band_options():
    from vitcnn_amd import model_utils as mu
    for kw, c1 in ((dict(n_bands=(63, 1)), 63), (dict(n_bands=(144, 1), applyPCA=True), 30),
                   (dict(n_bands=(103, 1), precision="bf16"), 103)):
        model, opt, crit, hp = mu.get_model("Multimodality_Mamba", n_classes=7, ignored_labels=[0], dataset="synthetic",
                                            device=torch.device("cpu"), **kw)
        assert model.c1 == c1 and model.hsi2.cout == c1
        assert sum(p.numel() for g in opt.param_groups for p in g["params"]) == model._n_elems
