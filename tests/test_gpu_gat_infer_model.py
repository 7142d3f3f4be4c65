"""GPU suite: ``GATv2.inference(path=...)`` -- the CSC path against the block-by-block path it replaces for
``transforms="tile"`` models (the same bits), the head mean of more than two heads against tests/gat_glue_ref.py, the library
model against an fp32 restatement, and what the path refuses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gat_glue_ref as ref

pytestmark = pytest.mark.gpu

FEAT, CLASSES = 24, 5
_cache = {}


def _graph(cuda):
    if "g" not in _cache:
        import bliss_gnn_amd as bg
        from bliss_gnn_amd.synth import chung_lu_csc
        ip, ix, ei = chung_lu_csc(4000, 200000, seed=9)
        feats = (torch.randn(4000, FEAT, generator=torch.Generator().manual_seed(1)) * 0.5).bfloat16()
        _cache["g"] = (bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda)}), ip, ix.long(), feats)
    return _cache["g"]


def _tile_model(cuda, heads, hidden):
    from bliss_gnn_amd.model import GATv2
    torch.manual_seed(3)
    return GATv2(3, FEAT, hidden, CLASSES, heads, F.elu, 0.0, 0.0, 0.2, True, transforms="tile").to(cuda).bfloat16()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("heads,hidden", [([2, 2, 1], 12), ([4, 4, 2], 8)])
def test_csc_path_has_the_bits_of_the_blocks_path(cuda, heads, hidden):
    g = _graph(cuda)[0]
    model = _tile_model(cuda, heads, hidden)
    kinds = [type(l.res_fc).__name__ for l in model.gatv2_layers]
    assert kinds == ["NoneType", "Identity", "Linear"], kinds        # both kinds of residual are in the model
    want = model.inference(g, cuda, 128, False, 0, path="blocks")
    assert model.last_inference_path == "blocks" and want.shape == (4000, CLASSES)
    assert torch.equal(_bits(g.ndata["h"]), _bits(want))
    got = model.inference(g, cuda, 128, False, 0, node_chunk=4096, path="csc")
    assert model.last_inference_path == "csc"
    assert torch.equal(_bits(g.ndata["h"]), _bits(got)) and got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(model.inference(g, cuda, 128, False, 0, node_chunk=300, path="csc")), _bits(want))
    auto = model.inference(g, cuda, 128, False, 0)
    assert model.last_inference_path == "csc" and torch.equal(_bits(auto), _bits(want))
    # ranges that really are short (the floor lowered: 300 rows, then cut by edges as well): the result does not depend on them
    model.csc_min_rows = 1
    assert len(model._csc_ranges(g, 300)) == 14
    assert torch.equal(_bits(model.inference(g, cuda, 128, False, 0, node_chunk=300, path="csc")), _bits(want))
    model.csc_max_edges = 20000
    ranges = model._csc_ranges(g, 4096)
    assert len(ranges) >= 9 and ranges[0][0] == 0 and ranges[-1][1] == 4000
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and sum(r[2] for r in ranges) == g.num_edges()
    assert max(r[2] for r in ranges) <= 20000 + 817                 # the budget plus one row's edges (the hub has 817)
    assert torch.equal(_bits(model.inference(g, cuda, 128, False, 0, path="csc")), _bits(want))
    assert model.training                                           # the mode it was called in is back


def test_four_output_heads_against_the_glue_reference(cuda):
    """More than two heads in the output layer: torch's mean(1) keeps its own order, so only the head mean
    is compared, with tests/gat_glue_ref.py, on the last layer's rows as the blocks path computes them."""
    from bliss_gnn_amd.model import _blockwise_inference
    g = _graph(cuda)[0]
    model = _tile_model(cuda, [2, 2, 4], 12)
    got = model.inference(g, cuda, 128, False, 0, path="csc")
    model.eval()
    with torch.no_grad():
        rows = _blockwise_inference(model.gatv2_layers, g, g.ndata["features"], 4096, lambda l, out: out.flatten(1))
    model.train()
    assert rows.shape == (4000, 4 * CLASSES)
    want = ref.glue_fwd(rows.float().cpu().numpy(), None, 4, CLASSES, 0, True)[0]
    assert np.array_equal(got.float().cpu().numpy(), want)


def test_default_model_keeps_the_blocks_path(cuda):
    from bliss_gnn_amd.model import GATv2
    g = _graph(cuda)[0]
    torch.manual_seed(0)
    model = GATv2(3, FEAT, 12, CLASSES, [2, 2, 1], torch.relu, 0.0, 0.0, 0.2, True).to(cuda).bfloat16()
    a = model.inference(g, cuda, 128, False, 0)
    assert model.last_inference_path == "blocks"
    assert torch.equal(_bits(a), _bits(model.inference(g, cuda, 128, False, 0, path="blocks")))
    with pytest.raises(NotImplementedError, match="ELU"):
        model.inference(g, cuda, 128, False, 0, path="csc")
    # an ELU library model is within the path's limits, but "auto" still leaves a default model where it was
    torch.manual_seed(0)
    elu = GATv2(3, FEAT, 12, CLASSES, [2, 2, 1], F.elu, 0.0, 0.0, 0.2, True).to(cuda).bfloat16()
    elu.inference(g, cuda, 128, False, 0)
    assert elu.last_inference_path == "blocks"


def test_library_model_with_elu_under_csc(cuda):
    """The bar of test_gat_inference: the fp32 restatement of the layers over all in-edges (here with ELU), within 0.05 of the
    result's scale."""
    from bliss_gnn_amd.model import GATv2
    g, ip, src, feats = _graph(cuda)
    V = feats.shape[0]
    dst = torch.repeat_interleave(torch.arange(V), ip[1:] - ip[:-1])
    torch.manual_seed(0)
    heads = [2, 1]
    model = GATv2(2, FEAT, 8, 3, heads, F.elu, 0.0, 0.0, 0.2, True).to(cuda).bfloat16()
    h = feats.float()
    for l, layer in enumerate(model.gatv2_layers):
        H, D = heads[l], layer._out_feats
        f = (h @ layer.fc_src.weight.float().cpu().t()).view(V, H, D)
        e = (F.leaky_relu(f[src] + f[dst], 0.2) * layer.attn.float().cpu()).sum(-1)                           # [E, H]
        mx = torch.full((V, H), -1e30).scatter_reduce(0, dst[:, None].expand(-1, H), e, "amax")
        ex = torch.exp(e - mx[dst])
        a = ex / torch.zeros(V, H).index_add_(0, dst, ex)[dst]
        out = torch.zeros(V, H, D).index_add_(0, dst, a[:, :, None] * f[src])
        if layer.res_fc is not None:
            res = h if isinstance(layer.res_fc, torch.nn.Identity) else h @ layer.res_fc.weight.float().cpu().t()
            out = out + res.view(V, -1, D)
        h = F.elu(out).flatten(1) if l == 0 else out.mean(1)
    ys = [model.inference(g, cuda, 128, False, 0, node_chunk=c, path="csc") for c in (4096, 300)]
    assert model.last_inference_path == "csc" and ys[0].shape == (V, 3)
    h = h.detach()
    err, scale = (ys[0].float().cpu() - h).abs().max(), h.abs().max()
    print("library model under csc: max |y - ref| = %.4g, max |ref| = %.4g" % (float(err), float(scale)))
    assert err <= 0.05 * scale
    assert torch.equal(ys[0], ys[1])


def test_what_the_csc_path_refuses(cuda):
    import bliss_gnn_amd as bg
    g, ip, ix, feats = _graph(cuda)
    model = _tile_model(cuda, [2, 2, 1], 12)
    with pytest.raises(ValueError, match="path"):
        model.inference(g, cuda, 128, False, 0, path="nope")
    with pytest.raises(NotImplementedError, match="bf16"):
        _tile_model(cuda, [2, 2, 1], 12).float().inference(g, cuda, 128, False, 0, path="csc")
    cpu_g = bg.Graph(ip, ix.to(torch.int32), ndata={"features": feats})
    with pytest.raises(NotImplementedError, match="GPU"):
        model.inference(cpu_g, cuda, 128, False, 0, path="csc")
    # fp32 FEATURES are no refusal: both paths take them as bf16, as the blocks path always did
    fp32_feats = bg.Graph(g.indptr, g.indices, ndata={"features": feats.float().to(cuda)})
    assert torch.equal(_bits(model.inference(fp32_feats, cuda, 128, False, 0, path="csc")), _bits(model.inference(g, cuda, 128, False, 0, path="csc")))


def test_fused_kernels_switched_off_is_a_refusal(cuda, monkeypatch):
    g = _graph(cuda)[0]
    model = _tile_model(cuda, [2, 2, 1], 12)
    monkeypatch.setenv("BLISS_GAT_FUSED", "0")
    with pytest.raises(NotImplementedError, match="BLISS_GAT_FUSED"):
        model.inference(g, cuda, 128, False, 0, path="csc")
