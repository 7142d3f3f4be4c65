"""GPU suite (-m gpu): SAGEGCNConv(in, out) and SAGE(..., aggregator_type="gcn") on the library path.

The layer on integers: in-degrees with deg + 1 a power of two, features, fc_neigh weights and bias in {-1, 0, 1}, edge weights in
{0.5, 1, 2}, an upstream gradient whose row i is (deg_i + 1) * {-1, 0, 1} -- every rounding point is exact (asserted on the CPU in
tests/test_spmm_self_ref.py: the restatement that rounds at every store equals the fp64 one), so the output and the gradients of h,
fc_neigh.weight and bias EQUAL fp64, for both orders of fc_neigh.

The layer on random data, per element within spmm_self_ref.layer_k (derived there from bounds.SPMM_K and bounds.dense_k: a stored
bf16 value costs 1, an aggregation 1.25, an fp32 product its n_terms * 2^-16, the last rounding is k_ulp = 1).

The model: an eager TrainStep and a GraphedTrainStep agree on loss and parameters after 3 steps (dropout 0: the library path's
dropout is torch's generator stream, whose captured replays are not this test's subject); embed_norm is the norm of every layer's
input; inference "chunks" and "blocks" agree with one full-neighbour block over all nodes pushed through the layer chain.  The three
inference paths cut a long row's fp32 sum at different chunk boundaries, so they agree normwise, not bit for bit: a stored bf16 value
may flip by one ulp (2^-8 relative), a layer stores three (Z or the product, the aggregation, the biased sum), and xavier weights
with a normalised sum amplify a relative error by no more than about 1, so two paths differ by at most L * 4 * 2^-8 = L * 2^-6 of
the largest output after L layers."""
import math

import pytest
import torch

import bounds
import spmm_self_ref as ref

pytestmark = pytest.mark.gpu

V, E, FEAT, CLASSES, BS = 600, 7000, 24, 4, 48


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


def _layer(cuda, fin, fout, w, b):
    from bliss_gnn_amd.nn import SAGEConv, SAGEGCNConv
    layer = SAGEGCNConv(fin, fout).to(cuda).bfloat16()
    with torch.no_grad():
        layer.fc_neigh.weight.copy_(w)
        layer.bias.copy_(b)
    return layer


@pytest.mark.parametrize("fin,fout", [(8, 4), (4, 8)])
def test_gcn_layer_on_integers_equals_fp64(cuda, fin, fout):
    c = ref.exact_case(fin, fout)
    blk = bounds.to_block(bounds.Spec(c["K"], c["S"], c["indptr"], c["src"], c["dst"]), cuda)
    layer = _layer(cuda, fin, fout, c["w_neigh"].to(cuda), c["bias"].to(cuda))
    h = c["h"].to(cuda).requires_grad_()
    out = torch.relu(layer(blk, h, edge_weight=c["ew"].to(cuda)))
    out.backward(c["g"].to(cuda))
    want = ref.layer_terms(c["indptr"], c["src"], c["dst"], c["h"], c["w_neigh"], bias=c["bias"], ew=c["ew"], g=c["g"], relu=True)
    for name, got in (("out", out), ("d_h", h.grad), ("d_w", layer.fc_neigh.weight.grad), ("d_b", layer.bias.grad)):
        assert torch.equal(got.detach().double().cpu(), want[name]), name
    assert (layer._in_src_feats > layer._out_feats) == (fin > fout) and not hasattr(layer, "fc_self")


@pytest.mark.parametrize("fin,fout", [(64, 32), (32, 64)])
def test_gcn_layer_on_random_data(cuda, fin, fout):
    spec = bounds.edge_shape_spec()
    assert int(spec.in_degrees().max()) <= bounds.SPMM_MAX_ROW - 3 and int(spec.out_degrees().max()) <= bounds.SPMM_MAX_ROW - 3
    blk = bounds.to_block(spec, cuda)
    gen = torch.Generator().manual_seed(fin)
    w = (torch.randn(fout, fin, generator=gen) * (2.0 / (fin + fout)) ** 0.5).bfloat16().to(cuda)
    b = (torch.randn(fout, generator=gen) * 0.1).bfloat16().to(cuda)
    h0 = torch.randn(spec.K, fin, generator=gen).bfloat16().to(cuda)
    ew = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    g = torch.randn(spec.S, fout, generator=gen).bfloat16().to(cuda)
    layer = _layer(cuda, fin, fout, w, b)
    h = h0.clone().requires_grad_()
    out = torch.relu(layer(blk, h, edge_weight=ew))
    out.backward(g)
    idx = tuple(t.to(cuda) for t in (spec.indptr, spec.src, spec.dst))
    k = ref.layer_k(fin, fout, max(spec.K, spec.S), False)
    fwd = ref.layer_terms(*idx, h0, w, bias=b, ew=ew, relu=True)
    # where the reference is positive the output is compared as it is; where it is <= 0 the output (>= 0) must lie within the bound
    # of the pre-activation value, which is what ``rst + out`` against ``rst`` states
    rst, o = fwd["rst"], out.detach().double()
    r = {"out": bounds.assert_within(torch.where(rst > 0, o, rst + o), rst, fwd["mag_rst"], *k["out"], "out")}
    # the backward's mask is the kernel's own (the forward check has held every element to its bound)
    want = ref.layer_terms(*idx, h0, w, bias=b, ew=ew, g=g, mask=out > 0, relu=True)
    for name, got in (("d_h", h.grad), ("d_w", layer.fc_neigh.weight.grad), ("d_b", layer.bias.grad)):
        r[name] = bounds.assert_within(got, want[name], want["mag_" + name], *k[name], name)
    print(fin, fout, r)


# ------------------------------------------------------------------------------------------------ the model
def _graph(cuda):
    """The 600-node Chung-Lu graph of tests/test_gpu_gcn_tile_path.py."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, FEAT, generator=gen).bfloat16()
    labels = torch.randint(0, CLASSES, (V,), generator=gen)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    return g, torch.randperm(V, generator=gen).to(torch.int32).to(cuda)


def _model(cuda, dropout=0.1, transforms="auto"):
    from bliss_gnn_amd.model import SAGE
    torch.manual_seed(0)
    m = SAGE(FEAT, 16, CLASSES, 3, torch.relu, dropout, transforms=transforms, aggregator_type="gcn").to(cuda).bfloat16()
    m.train()
    return m


def test_eager_and_captured_training_agree(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep

    def build():
        g, perm = _graph(cuda)
        return g, fit.make_sampler("poisson-bandit-keyed", [24, 16, 12]), _model(cuda, dropout=0.0), BatchLoader(perm[:400], BS, seed=5).forever()

    g, s, m, loader = build()
    assert [l._in_src_feats > l._out_feats for l in m.layers] == [True, False, True]
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
    assert torch.equal(_bits(s._w_pos), _bits(sB._w_pos)) and not torch.equal(_bits(s._w_pos[0]), _bits(torch.ones_like(s._w_pos[0])))
    if hasattr(step, "close"):
        step.close()


def test_embed_norm_is_the_norm_of_every_layers_input(cuda):
    from bliss_gnn_amd import fit, ops
    g, perm = _graph(cuda)
    model = _model(cuda)
    for training in (True, False):
        model.train(training)
        _, _, mfgs = fit.make_sampler("labor", [5, 5, 5]).sample_blocks(g, perm[:BS])
        seen = []
        hooks = [l.register_forward_pre_hook(lambda mod, args: seen.append(args[1])) for l in model.layers]
        with torch.no_grad():
            model(mfgs, mfgs[0].srcdata["features"])
        for hk in hooks:
            hk.remove()
        assert len(seen) == 3
        for blk, x in zip(mfgs, seen):
            assert torch.equal(_bits(blk.srcdata["embed_norm"]), _bits(ops.embed_norm(x.contiguous())))


def test_inference_paths_agree_with_the_full_neighbour_block(cuda):
    from bliss_gnn_amd.graph import full_neighbor_block
    g, _ = _graph(cuda)
    model = _model(cuda)
    chunks = model.inference(g, node_chunk=256).clone()
    assert model.last_inference_path == "chunks" and model.training and chunks.shape == (V, CLASSES)
    blocks = model.inference(g, batch_size=100, path="blocks").clone()
    with pytest.raises(NotImplementedError, match='"gcn"'):
        model.inference(g, path="csc")
    auto = model.inference(g, batch_size=100, path="auto").clone()
    assert model.last_inference_path == "blocks" and torch.equal(_bits(auto), _bits(blocks))
    model.eval()
    with torch.no_grad():
        blk = full_neighbor_block(g, 0, V)
        assert blk.num_src_nodes() == V
        h = g.ndata["features"]
        for l, layer in enumerate(model.layers):
            h = layer(blk, h[blk.srcdata["_ID"].long()])
            if l < 2:
                h = model.activation(h)
    model.train()
    top = float(h.float().abs().max())
    for name, got in (("chunks", chunks), ("blocks", blocks)):
        err = float((got.float() - h.float()).abs().max())
        print(name, err, top)
        assert math.isfinite(err) and err <= 3 * 2.0 ** -6 * top, name


def test_refusals(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.nn import SAGEConv, SAGEGCNConv
    from bliss_gnn_amd.train import GraphedEvalStep, GraphedTrainStep, _live_refusal
    with pytest.raises(NotImplementedError, match="gcn"):
        SAGE(FEAT, 16, CLASSES, 3, torch.relu, 0.1, transforms="wide", aggregator_type="gcn")
    g, perm = _graph(cuda)
    model = _model(cuda)
    assert "MFMA path" in _live_refusal(model)                                  # the library model takes no capacity
    with pytest.raises(NotImplementedError, match="MFMA path"):
        GraphedTrainStep(g, fit.make_sampler("labor", [5, 5, 5]), model, BS, batch_capacity=BS)
    with pytest.raises(NotImplementedError, match="MFMA path"):
        GraphedEvalStep(g, fit.make_sampler("labor", [5, 5, 5]), model, BS, batch_capacity=BS)
    assert model.forward_last_parts(None, (None, None, False)) is None           # the loss kernel's two-addend form: not for this model
    # the (feat_src, feat_dst) pair form: forward-only
    _, _, mfgs = fit.make_sampler("labor", [5, 5, 5]).sample_blocks(g, perm[:BS])
    blk, x = mfgs[0], mfgs[0].srcdata["features"]
    S = blk.num_dst_nodes()
    lin_first = SAGEGCNConv(FEAT, 16).to(cuda).bfloat16()                  # z_dst = fc_neigh(feat_dst) would need a gradient
    with pytest.raises(NotImplementedError, match="h_self"):
        lin_first(blk, (x, x[:S].clone()))
    agg_first = SAGEGCNConv(FEAT, 32).to(cuda).bfloat16()                  # z_dst = feat_dst itself: the same rows, the same bits
    with torch.no_grad():
        assert torch.equal(_bits(agg_first(blk, (x, x[:S].clone()))), _bits(agg_first(blk, x)))
        lin_first(blk, (x, x[:S].clone()))
    with pytest.raises(NotImplementedError, match="'lstm'"):
        SAGEConv(FEAT, 16, "lstm")
