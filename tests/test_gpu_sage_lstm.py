"""GPU suite (-m gpu): nn.SAGELSTMConv and model.SAGELSTM.

The layer, in both forms of ``feat``, against DGL's formula in float64 (rst = fc_self(h_dst) + fc_neigh(neigh), neigh from
lstm_agg_ref.reducer) under the acceptance inequality of tests/test_gpu_lstm_agg.py: max |layer - truth64| <= max |the same formula in
bfloat16 tensor ops - truth64| for the output and every gradient that passes through the aggregation (see the comment at the
comparison).  The model: three eager TrainSteps against three replays of one
GraphedTrainStep, bit for bit; a short fit; inference; explain.edge_gradients; the refusals."""
import math

import pytest
import torch

import bounds
import lstm_agg_ref as ref
from bliss_gnn_amd import _lib

pytestmark = pytest.mark.gpu

T = _lib.lib.bliss_lstm_tile_rows()
V, E, FEAT, CLASSES, BS = 600, 7000, 24, 4, 48


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ the layer
def _layer_ref(spec, inp, lin, gout, dtype, pair):
    """DGL's layer in ``dtype`` tensor ops with autograd: {out, dh, (dh_dst,) dW_ih, dW_hh, db_ih, db_hh, dw, dfc_neigh, dfc_self, dbias}."""
    leaf = lambda v: None if v is None else v.detach().to(dtype).requires_grad_(True)
    a = {k: leaf(v) for k, v in inp.items()}
    b = {k: leaf(v) for k, v in lin.items()}
    h_dst = leaf(inp["h"][: spec.S]) if pair else a["h"][: spec.S]
    neigh = ref.reducer(spec, a["h"], a["w"], a["W_ih"], a["W_hh"], a["b_ih"], a["b_hh"])
    out = (h_dst @ b["fc_self"].t() + b["bias"]) + neigh @ b["fc_neigh"].t()
    out.backward(gout.to(dtype))
    res = {"out": out.detach().double(), "dh": a["h"].grad.double(), "dw": a["w"].grad.double()}
    if pair:
        res["dh_dst"] = h_dst.grad.double()
    for name, key in (("dW_ih", "W_ih"), ("dW_hh", "W_hh"), ("db_ih", "b_ih"), ("db_hh", "b_hh")):
        res[name] = a[key].grad.double()
    for name, key in (("dfc_neigh", "fc_neigh"), ("dfc_self", "fc_self"), ("dbias", "bias")):
        res[name] = b[key].grad.double()
    return res


@pytest.mark.parametrize("pair", [False, True], ids=["feat", "feat_pair"])
@pytest.mark.parametrize("fin,fout", [(40, 16), (8, 24)])
def test_layer_against_truth64(cuda, fin, fout, pair):
    from bliss_gnn_amd.nn import SAGELSTMConv
    degs = ref.degree_cases(T)["no_zero"]
    assert ref.asserted(degs)
    spec = ref.make_spec(degs, 3)
    inp, _ = ref.make_inputs(spec, fin, 100 + fin, True)
    gen = torch.Generator().manual_seed(fin + fout)
    rb = lambda x: x.to(torch.bfloat16).to(torch.float32)
    bound = torch.nn.init.calculate_gain("relu") * (6.0 / (fin + fout)) ** 0.5
    lin = {"fc_neigh": rb((torch.rand(fout, fin, generator=gen) * 2 - 1) * bound), "fc_self": rb((torch.rand(fout, fin, generator=gen) * 2 - 1) * bound),
           "bias": rb(torch.randn(fout, generator=gen) * 0.1)}
    gout = rb(torch.randn(spec.S, fout, generator=gen))
    truth = _layer_ref(spec, inp, lin, gout, torch.float64, pair)
    chain = _layer_ref(spec, inp, lin, gout, torch.bfloat16, pair)

    layer = SAGELSTMConv(fin, fout).to(cuda).bfloat16()
    with torch.no_grad():
        for name, key in (("weight_ih_l0", "W_ih"), ("weight_hh_l0", "W_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(layer.lstm, name).copy_(inp[key].to(cuda))
        layer.fc_neigh.weight.copy_(lin["fc_neigh"].to(cuda))
        layer.fc_self.weight.copy_(lin["fc_self"].to(cuda))
        layer.fc_self.bias.copy_(lin["bias"].to(cuda))
    blk = bounds.to_block(spec, cuda)
    h = inp["h"].bfloat16().to(cuda).requires_grad_()
    h_dst = inp["h"][: spec.S].bfloat16().to(cuda).requires_grad_() if pair else None
    w = inp["w"].bfloat16().to(cuda).requires_grad_()
    out = layer(blk, (h, h_dst) if pair else h, edge_weight=w)
    parts = layer(blk, (h, h_dst) if pair else h, edge_weight=w, parts=True)
    assert isinstance(parts, tuple) and torch.equal(_bits(parts[0] + parts[1]), _bits(out))
    out.backward(gout.bfloat16().to(cuda))
    got = {"out": out, "dh": h.grad, "dw": w.grad, "dW_ih": layer.lstm.weight_ih_l0.grad, "dW_hh": layer.lstm.weight_hh_l0.grad,
           "db_ih": layer.lstm.bias_ih_l0.grad, "db_hh": layer.lstm.bias_hh_l0.grad, "dfc_neigh": layer.fc_neigh.weight.grad,
           "dfc_self": layer.fc_self.weight.grad, "dbias": layer.fc_self.bias.grad}
    if pair:
        got["dh_dst"] = h_dst.grad
    # what is compared: the tensors that pass through the aggregation.  d fc_self, d bias and d h_dst are the same library
    # arithmetic on both sides, and in the one-tensor form the first S rows of d h are autograd's bf16 sum of the aggregation's
    # gradient and fc_self's, whose last rounding (half a step of the sum, the same on both sides) hides the aggregation's share:
    # there d h is compared on the rows that are sources only, and on every row in the pair form, where h feeds nothing else.
    cut = (lambda k, v: v[spec.S:] if (k == "dh" and not pair) else v)
    figures = {k: (ref.max_err(cut(k, v.detach().double().cpu()), cut(k, truth[k])), ref.max_err(cut(k, chain[k]), cut(k, truth[k])))
               for k, v in got.items()}
    print(fin, fout, pair, {k: "%.3g / %.3g" % v for k, v in figures.items()})
    assert all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    for k in ("out", "dh", "dw", "dW_ih", "dW_hh", "db_ih", "db_hh", "dfc_neigh"):
        err, limit = figures[k]
        assert err <= limit, (k, err, limit)


# ------------------------------------------------------------------------------------------------ the model
def _graph(cuda):
    """The 600-node Chung-Lu graph of tests/test_gpu_sage_gcn.py."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, FEAT, generator=gen).bfloat16()
    labels = (feats.float() @ torch.randn(FEAT, CLASSES, generator=gen)).argmax(1)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    return g, torch.randperm(V, generator=gen).to(torch.int32).to(cuda)


def _model(cuda, dropout=0.0, layers=2):
    from bliss_gnn_amd.model import SAGELSTM
    torch.manual_seed(0)
    m = SAGELSTM(FEAT, 16, CLASSES, layers, torch.relu, dropout).to(cuda).bfloat16()
    m.train()
    return m


def test_eager_and_captured_training_agree(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep

    def build():
        g, perm = _graph(cuda)
        return g, fit.NeighborSampler([5, 5], draw="device"), _model(cuda), BatchLoader(perm[:400], BS, seed=5).forever()

    g, s, m, loader = build()
    before = [p.detach().clone() for p in m.parameters()]
    step = GraphedTrainStep(g, s, m, BS, lr=0.01)
    torch.manual_seed(3)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)                                              # three real steps
    losses = [float(step(next(loader))) for _ in range(3)]
    gB, sB, mB, loaderB = build()
    eager = TrainStep(gB, sB, mB, lr=0.01)
    torch.manual_seed(3)
    for _ in range(3):
        sB.sample_blocks(gB, next(loaderB))
    for _ in range(3):
        eager(next(loaderB))
    want = [float(eager(next(loaderB))) for _ in range(3)]
    print(losses, want)
    assert all(math.isfinite(x) for x in losses) and losses == want
    for (n, p), q, p0 in zip(m.named_parameters(), mB.parameters(), before):
        assert bool(torch.isfinite(p.float()).all()) and torch.equal(_bits(p), _bits(q)) and not torch.equal(p, p0), n
    if hasattr(step, "close"):
        step.close()


@pytest.mark.parametrize("kind", ["eager", "graphed"])
def test_fit_learns(cuda, kind):
    from bliss_gnn_amd import fit
    g, perm = _graph(cuda)
    model = _model(cuda, dropout=0.1)
    out = fit.fit(g, fit.NeighborSampler([5, 5], draw="device"), model, perm[:320], perm[320:420], perm[420:], batch_size=32, lr=0.01,
                  max_epochs=2, train_step=kind)                                # 2 x 10 steps
    hist = out["history"]
    print(kind, [h["train_loss"] for h in hist], out["final"])
    assert out["steps"] == 20 and len(hist) == 2 and all(math.isfinite(h["train_loss"]) for h in hist)
    assert hist[-1]["train_loss"] < hist[0]["train_loss"]
    assert model.last_inference_path == "blocks" and set(out["final"]) == {"Train", "Validation", "Test"}


def test_inference_is_the_layer_chain(cuda):
    from bliss_gnn_amd.graph import full_neighbor_block
    g, _ = _graph(cuda)
    model = _model(cuda, dropout=0.1)
    blocks = model.inference(g, batch_size=100, path="blocks").clone()
    assert model.last_inference_path == "blocks" and model.training and blocks.shape == (V, CLASSES)
    auto = model.inference(g, batch_size=100).clone()                           # the default of this model: "auto"
    assert model.last_inference_path == "blocks" and torch.equal(_bits(auto), _bits(blocks))
    for path in ("chunks", "csc"):
        with pytest.raises(NotImplementedError, match='"lstm"'):
            model.inference(g, path=path)
    model.eval()
    with torch.no_grad():                                                       # the same batches through the layers by hand
        h = g.ndata["features"]
        for l, layer in enumerate(model.layers):
            rows = []
            for b0 in range(0, V, 100):
                blk = full_neighbor_block(g, b0, min(V, b0 + 100))
                y = layer(blk, h[blk.srcdata["_ID"].long()])
                rows.append(model.activation(y) if l < len(model.layers) - 1 else y)
            h = torch.cat(rows)
    model.train()
    assert torch.equal(_bits(h), _bits(blocks)) and bool(torch.isfinite(h.float()).all())


def test_edge_gradients(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import explain, fit
    g, perm = _graph(cuda)
    model = _model(cuda)
    assert explain.refusal(model) is None
    _, _, mfgs = fit.NeighborSampler([5, 5], draw="device").sample_blocks(g, perm[:BS])
    grads = bg.edge_gradients(model, mfgs, mfgs[0].srcdata["features"], lambda y: y.float().square().sum())
    assert len(grads) == len(mfgs) == 2
    for blk, gw in zip(mfgs, grads):
        live = int(blk._counts.B) if getattr(blk, "_counts", None) is not None else blk.num_edges()
        assert gw.dtype == torch.bfloat16 and gw.shape == (blk.num_edges(),) and bool(torch.isfinite(gw.float()).all())
        assert bool(gw[:live].any()) and not _bits(gw[live:]).any()
    assert all(p.grad is None for p in model.parameters())


def test_refusals(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.nn import SAGELSTMConv, lstm_aggregate
    from bliss_gnn_amd.train import GraphedTrainStep, _live_refusal
    g, perm = _graph(cuda)
    model = _model(cuda)
    assert _live_refusal(model) is not None                                     # no batch_capacity for this model
    with pytest.raises(NotImplementedError):
        GraphedTrainStep(g, fit.NeighborSampler([5, 5], draw="device"), model, BS, batch_capacity=BS)
    assert model.forward_last_parts(None, (None, None, False)) is None          # PipelinedTrainStep: the un-split path
    _, _, mfgs = fit.NeighborSampler([5, 5], draw="device").sample_blocks(g, perm[:BS])
    blk, x = mfgs[0], mfgs[0].srcdata["features"]
    f32 = SAGELSTMConv(FEAT, 16).to(cuda)                                       # fp32 parameters: refused, no slow path
    with pytest.raises(NotImplementedError, match="bf16"):
        f32(blk, x)
    layer = SAGELSTMConv(FEAT, 16).to(cuda).bfloat16()
    with pytest.raises(NotImplementedError, match="bf16"):
        lstm_aggregate(blk, x.float(), layer.lstm)
    with pytest.raises(NotImplementedError, match="in_feats <= 256"):
        lstm_aggregate(blk, x, torch.nn.LSTM(300, 300).to(cuda).bfloat16())
