"""GPU suite (-m gpu): ``SAGE.inference(path=...)`` -- the CSC path against the batch-by-batch block path, which
runs the model's own layer chain: the same bits at the same ``batch_size``, whatever the destination ranges and launches; what
"auto" takes; what the path refuses; the default call is "chunks"; ``fit(..., inference_path=...)``.

Models: SAGE(24, 16, 5, 3) -- a Linear-first (24 > 16), an aggregate-first (16 <= 16) and a Linear-first (16 > 5) layer -- and
SAGE(12, 16, 4, 2), whose input layer is aggregate-first, both under "auto" (the MFMA path) and "tile"; a "pool" model under "tile";
a "wide" model with 1100 input features on a 300-node graph.  All in training mode before every call.  Should a model equality fail
while the kernel equality of tests/test_gpu_sage_infer.py holds, a dense product's rows would depend on the launch size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, E = 1500, 24000
_cache = {}


def _graph(feat, cuda, nodes=V, edges=E):
    key = (feat, nodes)
    if key not in _cache:
        import bliss_gnn_amd as bg
        from bliss_gnn_amd.synth import chung_lu_csc
        ip, ix, _ = chung_lu_csc(nodes, edges, seed=61)
        feats = (torch.randn(nodes, feat, generator=torch.Generator().manual_seed(1)) * 0.5).bfloat16()
        _cache[key] = (bg.Graph(ip.to(cuda), ix.to(cuda), ndata={"features": feats.to(cuda)}), ip, ix, feats)
    return _cache[key]


MODELS = {
    "auto-3": (24, (24, 16, 5, 3), {}),
    "auto-2": (12, (12, 16, 4, 2), {}),
    "tile-3": (24, (24, 16, 5, 3), dict(transforms="tile")),
    "tile-2": (12, (12, 16, 4, 2), dict(transforms="tile")),
    "pool-tile": (24, (24, 16, 5, 3), dict(transforms="tile", aggregator_type="pool")),
    "wide": (1100, (1100, 16, 4, 2), dict(transforms="wide")),
}
ORDER = {"auto-3": [True, False, True], "auto-2": [False, True], "wide": [True, True]}


def _model(name, cuda):
    from bliss_gnn_amd.model import SAGE
    feat, dims, kw = MODELS[name]
    torch.manual_seed(3)
    model = SAGE(*dims, torch.relu, 0.5, **kw).to(cuda).bfloat16()
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for layer in model.layers:                                        # biases that matter
            layer.fc_self.bias.copy_(torch.randn(layer.fc_self.bias.shape, generator=gen) * 0.1)
            if hasattr(layer, "fc_pool"):
                layer.fc_pool.bias.copy_(torch.randn(layer.fc_pool.bias.shape, generator=gen) * 0.1)
    if name in ORDER:
        assert [l._in_src_feats > l._out_feats for l in model.layers] == ORDER[name]
    g = _graph(feat, cuda, 300, 4000) if name == "wide" else _graph(feat, cuda)
    return model.train(), g[0]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("bs", [128, 37, V + 5])
@pytest.mark.parametrize("name", list(MODELS))
def test_csc_path_has_the_bits_of_the_blocks_path(cuda, name, bs):
    model, g = _model(name, cuda)
    n = g.num_nodes()
    want = model.inference(g, cuda, bs, False, 0, path="blocks")
    assert model.last_inference_path == "blocks" and want.shape == (n, model.n_classes) and model.training
    assert g.ndata["h"] is want and bool(want.float().abs().sum() > 0) and bool(torch.isfinite(want.float()).all())
    assert model.csc_refusal(g, g.ndata["features"], bs) is None
    got = model.inference(g, cuda, bs, False, 0, path="csc")
    assert model.last_inference_path == "csc" and model.training
    assert g.ndata["h"] is got and got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want))
    auto = model.inference(g, cuda, bs, False, 0, node_chunk=3, path="auto")                 # (node_chunk: accepted and ignored)
    assert model.last_inference_path == "csc" and torch.equal(_bits(auto), _bits(want))
    model.eval()
    assert torch.equal(_bits(model.inference(g, cuda, bs, False, 0, path="csc")), _bits(want)) and not model.training


@pytest.mark.parametrize("name", ["auto-3", "tile-2", "pool-tile"])
def test_the_result_does_not_depend_on_the_ranges(cuda, name):
    from bliss_gnn_amd.model import _csc_groups, _csc_ranges
    model, g = _model(name, cuda)
    bs, n_edges = 128, g.num_edges()
    ranges = lambda: _csc_ranges(g, bs, model.csc_max_edges, "SAGE.inference")
    assert len(ranges()) == 1
    want = model.inference(g, cuda, bs, False, 0, path="blocks")
    assert torch.equal(_bits(model.inference(g, cuda, bs, False, 0, path="csc")), _bits(want))
    model.csc_max_edges = 4000
    rs = ranges()
    assert len(rs) >= 4 and rs[0][0] == 0 and rs[-1][1] == V
    assert all(a[1] == b[0] and a[2] + a[3] == b[2] for a, b in zip(rs, rs[1:])) and sum(r[3] for r in rs) == n_edges
    assert all(r[0] % bs == 0 and r[1] > r[0] for r in rs)                            # whole batches, at least one
    assert _csc_groups(rs, model.csc_spmm_edges) == [(0, V, 0, n_edges)]              # the message passing still in one launch
    assert torch.equal(_bits(model.inference(g, cuda, bs, False, 0, path="csc")), _bits(want))
    model.csc_spmm_edges = 9000                                                       # ... and in several launches
    groups = _csc_groups(rs, model.csc_spmm_edges)
    assert 2 <= len(groups) <= len(rs) and groups[0][0] == 0 and groups[-1][1] == V and sum(r[3] for r in groups) == n_edges
    assert torch.equal(_bits(model.inference(g, cuda, bs, False, 0, path="csc")), _bits(want))
    model.csc_max_edges = model.csc_spmm_edges = 1                                    # every batch its own range and launch
    assert len(ranges()) == (V + bs - 1) // bs
    assert torch.equal(_bits(model.inference(g, cuda, bs, False, 0, path="csc")), _bits(want))


def test_the_default_call_is_chunks(cuda):
    model, g = _model("auto-3", cuda)
    a = model.inference(g, cuda, 128, False, 0)
    assert model.last_inference_path == "chunks" and g.ndata["h"] is a and model.training
    b = model.inference(g, cuda, 128, False, 0, path="chunks")
    assert model.last_inference_path == "chunks" and torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(model.inference(g, cuda, 128, False, 0, node_chunk=700)), _bits(a))
    pool, gp = _model("pool-tile", cuda)
    assert torch.equal(_bits(pool.inference(gp)), _bits(pool.inference(gp, path="chunks"))) and pool.last_inference_path == "chunks"


def test_what_auto_takes_and_what_csc_refuses(cuda, monkeypatch):
    from bliss_gnn_amd.model import SAGE
    import bliss_gnn_amd as bg
    g, ip, ix, feats = _graph(24, cuda)
    torch.manual_seed(0)
    pool = SAGE(24, 16, 5, 3, torch.relu, 0.5, aggregator_type="pool").to(cuda).bfloat16().train()     # "pool" under "auto" transforms
    a = pool.inference(g, cuda, 128, False, 0, path="auto")
    assert pool.last_inference_path == "chunks" and pool.training
    assert torch.equal(_bits(a), _bits(pool.inference(g, cuda, 128, False, 0)))
    with pytest.raises(NotImplementedError, match='transforms="tile"'):
        pool.inference(g, cuda, 128, False, 0, path="csc")
    assert pool.training and pool.last_inference_path == "chunks"
    model, _ = _model("auto-3", cuda)
    assert model.csc_refusal(g, g.ndata["features"], 128) is None
    with monkeypatch.context() as m:
        m.setenv("BLISS_SAGE_MFMA", "0")
        b = model.inference(g, cuda, 128, False, 0, path="auto")
        assert model.last_inference_path == "chunks" and torch.equal(_bits(b), _bits(model.inference(g, cuda, 128, False, 0)))
        with pytest.raises(NotImplementedError, match="BLISS_SAGE_MFMA=0"):
            model.inference(g, cuda, 128, False, 0, path="csc")
    with pytest.raises(ValueError, match="path"):
        model.inference(g, cuda, 128, False, 0, path="nope")
    with pytest.raises(NotImplementedError, match="batch_size"):
        model.inference(g, cuda, 0, False, 0, path="csc")
    fp32 = bg.Graph(g.indptr, g.indices, ndata={"features": feats.float().to(cuda)})
    with pytest.raises(NotImplementedError, match="bf16"):
        model.inference(fp32, cuda, 128, False, 0, path="csc")
    cpu_g = bg.Graph(ip, ix, ndata={"features": feats})
    with pytest.raises(NotImplementedError, match="GPU"):
        model.inference(cpu_g, cuda, 128, False, 0, path="csc")
    model.eval()
    with pytest.raises(NotImplementedError):
        model.inference(fp32, cuda, 128, False, 0, path="csc")
    assert not model.training                                             # the flag is what it was, also after a refusal
    model.train()

    def boom(*a, **k):
        raise RuntimeError("boom")

    monkeypatch.setattr("bliss_gnn_amd.nn.sage_infer_spmm", boom)         # an exception inside the loops: the flag comes back
    with pytest.raises(RuntimeError, match="boom"):
        model.inference(g, cuda, 128, False, 0, path="csc")
    assert model.training


def test_csc_against_the_fp32_restatement(cuda):
    """The bound of test_sage_full_neighbor_inference (0.05 of the largest magnitude: three bf16 layers deep) on that test's fp32
    restatement: plain mean over all in-neighbours, SAGEConv layer by layer, relu between layers."""
    model, g = _model("auto-3", cuda)
    _, ip, ix, feats = _graph(24, cuda)
    deg = ip[1:] - ip[:-1]
    dst = torch.repeat_interleave(torch.arange(V), deg)
    src = ix.long()
    h = feats.float()
    for l, layer in enumerate(model.layers):
        Ws, bs, Wn = (p.detach().float().cpu() for p in (layer.fc_self.weight, layer.fc_self.bias, layer.fc_neigh.weight))
        hb = h.bfloat16().float()                                    # the layer input is stored in bf16
        agg = lambda z: torch.zeros(V, z.shape[1]).index_add_(0, dst, z[src]) / deg.clamp(min=1).float()[:, None]
        neigh = agg((hb @ Wn.t()).bfloat16().float()) if Wn.shape[1] > Wn.shape[0] else agg(hb).bfloat16().float() @ Wn.t()
        h = hb @ Ws.t() + bs + neigh
        if l < 2:
            h = torch.relu(h)
    y = model.inference(g, cuda, 128, False, 0, path="csc")
    err, lim = float((y.float().cpu() - h).abs().max()), 0.05 * float(h.abs().max())
    print("SAGE-INFER-CSC against fp32: largest error %.4g, bound %.4g" % (err, lim))
    assert y.shape == (V, 5) and err <= lim


def test_fit_passes_the_path_on(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    n, classes = 600, 4
    ip, ix, ei = chung_lu_csc(n, 6000, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(n, 24, generator=gen).bfloat16()
    labels = (feats.float() @ torch.randn(24, classes, generator=gen)).argmax(1)
    perm = torch.randperm(n, generator=gen).to(torch.int32).to(cuda)
    tr, va, te = perm[:360], perm[360:480], perm[480:]
    out, pred = {}, {}
    for path in ("csc", "blocks"):
        g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
        torch.manual_seed(0)
        model = SAGE(24, 16, classes, 3, torch.relu, 0.1).to(cuda).bfloat16()
        out[path] = fit.fit(g, fit.make_sampler("neighbor", [8, 8, 8]), model, tr, va, te, batch_size=128, lr=0.01, max_epochs=1,
                            inference_path=path)
        assert model.last_inference_path == path
        pred[path] = g.ndata["h"]
    assert set(out["csc"]["final"]) == {"Train", "Validation", "Test"}
    assert out["csc"]["final"] == out["blocks"]["final"] and torch.equal(_bits(pred["csc"]), _bits(pred["blocks"]))
