"""GPU suite: ``SAGEConv(in, out, "pool")`` and ``SAGE(..., aggregator_type="pool")``.

Layer, exact: on small-integer data every value at a rounding point of the float64 restatement is an integer of magnitude at
most 256 (asserted on the CPU before anything is compared: a condition of the test, not a tolerance), so bf16 storage and fp32
accumulation are exact and the layer's output and all six gradients must EQUAL the restatement -- a missing ReLU mask, a missing
w in the backward, a transposed weight or a dropped bias gradient all change an integer.  Layer on random data: bit-equal to the
same ``nn.Linear`` calls around the CPU max.  Model: eager and captured training steps, the norms the bandit update reads,
full-neighbour inference, the refusals."""
import math

import pytest
import torch

import spmm_max_ref as ref
from bounds import Spec, edge_shape_spec, to_block

pytestmark = pytest.mark.gpu

V, E, FEAT, CLASSES, BS = 600, 7000, 24, 4, 48


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


# ------------------------------------------------------------------------------------------------ the layer, exact integers
def _int_spec():
    """41 destinations, in-degrees 1..20 and one row (7) without edges; 160 sources of out-degree <= 8, the destinations among
    them (edge e comes from source 37 e mod 160)."""
    degs = torch.tensor([max(1, (5 * i + 3) % 21) for i in range(41)])
    degs[7] = 0
    B, K = int(degs.sum()), 160
    src = (torch.arange(B) * 37) % K
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), degs.cumsum(0)])
    dst = torch.repeat_interleave(torch.arange(41), degs)
    spec = Spec(K, 41, indptr, src, dst)
    assert int(spec.in_degrees().max()) <= 20 and int(spec.out_degrees().max()) <= 8 and int(spec.in_degrees()[7]) == 0
    return spec


def _ints(gen, shape, lo, hi, keep=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=gen).double()
    return v * (torch.rand(shape, generator=gen) < keep)


def _int_case(fin, fout, seed):
    """Integer operands and the float64 restatement of the layer and its backward; asserts the exactness condition."""
    spec = _int_spec()
    S, K, B = spec.S, spec.K, spec.B
    gen = torch.Generator().manual_seed(seed)
    c = dict(h=_ints(gen, (K, fin), -1, 1), w=_ints(gen, (B,), 1, 2), gout=_ints(gen, (S, fout), -1, 1, 0.5),
             Wp=_ints(gen, (fin, fin), -1, 1, 0.6), bp=_ints(gen, (fin,), -1, 1), Wn=_ints(gen, (fout, fin), -1, 1, 0.6),
             Ws=_ints(gen, (fout, fin), -1, 1, 0.6), bs=_ints(gen, (fout,), -2, 2))
    z = c["h"] @ c["Wp"].t() + c["bp"]
    a = z.clamp(min=0)
    m, neigh, arg = ref.forward(spec.src, spec.dst, S, a.bfloat16(), c["w"].bfloat16())
    neigh = neigh.double()
    hn, hs = neigh @ c["Wn"].t(), c["h"][:S] @ c["Ws"].t() + c["bs"]
    g = c["gout"]
    d_neigh = g @ c["Wn"]
    d_a, _ = ref.backward(spec.src, K, d_neigh.bfloat16(), arg, c["w"].bfloat16())
    d_z = d_a * (z > 0)
    d_pool, d_self = d_z @ c["Wp"], g @ c["Ws"]
    d_h = d_pool.clone()
    d_h[:S] += d_self
    want = {"rst": hs + hn, "d_feat": d_h, "fc_pool.weight": d_z.t() @ c["h"], "fc_pool.bias": d_z.sum(0),
            "fc_neigh.weight": g.t() @ neigh, "fc_self.weight": g.t() @ c["h"][:S], "fc_self.bias": g.sum(0)}
    points = dict(want, z=z, m=m.double(), hn=hn, hs=hs, d_neigh=d_neigh, d_a=d_a, d_pool=d_pool, d_self=d_self)
    for k, v in points.items():
        assert bool((v == v.round()).all()) and float(v.abs().max()) <= 256, (k, float(v.abs().max()))
    assert float(m.max()) > 2 and int((arg >= 0).sum()) == (S - 1) * fin and bool((d_z != d_a).any())    # (the ReLU mask matters)
    return spec, c, want, arg


@pytest.mark.parametrize("fin,fout", [(16, 8), (8, 16)])
def test_pool_layer_on_integers_equals_the_restatement(cuda, fin, fout):
    from bliss_gnn_amd.nn import SAGEConv
    spec, c, want, _ = _int_case(fin, fout, 100 + fin)
    blk = to_block(spec, cuda)
    layer = SAGEConv(fin, fout, "pool").to(cuda).bfloat16()
    dev = lambda v: v.bfloat16().to(cuda)
    with torch.no_grad():
        layer.fc_pool.weight.copy_(dev(c["Wp"])), layer.fc_pool.bias.copy_(dev(c["bp"])), layer.fc_neigh.weight.copy_(dev(c["Wn"]))
        layer.fc_self.weight.copy_(dev(c["Ws"])), layer.fc_self.bias.copy_(dev(c["bs"]))
    h = dev(c["h"]).requires_grad_(True)
    rst = layer(blk, h, edge_weight=dev(c["w"]))
    rst.backward(dev(c["gout"]))
    got = dict({k: p.grad for k, p in layer.named_parameters()}, rst=rst, d_feat=h.grad)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] is not None and torch.equal(got[k].detach().double().cpu(), want[k]), k


@pytest.mark.parametrize("fin,fout", [(48, 16), (16, 48)])
def test_pool_layer_forward_on_random_data(cuda, fin, fout):
    """The edge-shape block: bit-equal to the same nn.Linear calls on the GPU around the max of the CPU restatement; parts=True
    returns the two addends."""
    from bliss_gnn_amd.nn import SAGEConv
    spec = edge_shape_spec()
    blk = to_block(spec, cuda)
    torch.manual_seed(fin)
    layer = SAGEConv(fin, fout, "pool").to(cuda).bfloat16()
    gen = torch.Generator().manual_seed(3)
    h = torch.randn(spec.K, fin, generator=gen).bfloat16().to(cuda)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    with torch.no_grad():
        layer.fc_pool.bias.copy_((torch.randn(fin, generator=gen) * 0.1).bfloat16())
        got = layer(blk, h, edge_weight=w)
        a, b = layer(blk, h, edge_weight=w, parts=True)
        pooled = torch.relu(layer.fc_pool(h))
        _, neigh, _ = ref.forward(spec.src, spec.dst, spec.S, pooled.cpu(), w.cpu())
        want = layer.fc_self(h[:spec.S]) + layer.fc_neigh(neigh.to(cuda))
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(a + b), _bits(want))


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


def _model(cuda):
    from bliss_gnn_amd.model import SAGE
    torch.manual_seed(0)
    m = SAGE(FEAT, 16, CLASSES, 3, torch.relu, 0.1, aggregator_type="pool").to(cuda).bfloat16()
    m.train()
    return m


def test_eager_training_moves_every_parameter(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import TrainStep
    g, perm = _graph(cuda)
    model = _model(cuda)
    assert sum(n.startswith("layers.") and ".fc_pool." in n for n, _ in model.named_parameters()) == 6
    before = [p.detach().clone() for p in model.parameters()]
    step = TrainStep(g, fit.make_sampler("labor", [5, 5, 5]), model, lr=0.01)
    losses = [float(step(perm[i * BS:(i + 1) * BS])) for i in range(2)]
    assert all(math.isfinite(l) and abs(l) < 1e4 for l in losses), losses
    for (n, p), q in zip(model.named_parameters(), before):
        assert bool(torch.isfinite(p.float()).all()) and not torch.equal(p, q), n


def _graphed_run(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    g, perm = _graph(cuda)
    sampler = fit.make_sampler("poisson-bandit-keyed", [24, 16, 12])
    model = _model(cuda)
    loader = BatchLoader(perm[:400], BS, seed=5).forever()
    step = GraphedTrainStep(g, sampler, model, BS, lr=0.01)
    torch.manual_seed(3)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)
    losses = [float(step(next(loader))) for _ in range(3)]
    torch.cuda.synchronize()
    if hasattr(sampler, "check_errors"):
        sampler.check_errors()
    out = losses, [p.detach().clone() for p in model.parameters()], sampler._w_pos.clone()
    if hasattr(step, "close"):
        step.close()
    return out


def test_captured_training_is_reproducible(cuda):
    """GraphedTrainStep on Hajek-weighted bandit blocks, 3 replayed steps; a second step built the same way (same seeds, a fresh
    model with the same init, a fresh sampler) ends with bit-identical parameters and EXP3 rows."""
    l1, p1, w1 = _graphed_run(cuda)
    l2, p2, w2 = _graphed_run(cuda)
    assert all(math.isfinite(x) for x in l1) and l1 == l2, (l1, l2)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(p1, p2))
    assert torch.equal(_bits(w1), _bits(w2)) and not torch.equal(_bits(w1[0]), _bits(torch.ones_like(w1[0])))


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


def test_inference_equals_the_chunked_restatement(cuda):
    g, _ = _graph(cuda)
    model = _model(cuda)
    chunk = 256
    got = model.inference(g, node_chunk=chunk).clone()
    assert model.training and got.shape == (V, CLASSES) and g.ndata["h"] is not None
    model.eval()
    indptr, indices = g.indptr.cpu(), g.indices.cpu().long()
    dst_all = torch.repeat_interleave(torch.arange(V), indptr[1:] - indptr[:-1])
    with torch.no_grad():
        h = g.ndata["features"]
        for l, layer in enumerate(model.layers):
            pooled = torch.relu(layer.fc_pool(h))
            y = torch.empty(V, layer._out_feats, dtype=h.dtype, device=cuda)
            for b0 in range(0, V, chunk):
                b1 = min(V, b0 + chunk)
                e0, e1 = int(indptr[b0]), int(indptr[b1])
                _, neigh, _ = ref.forward(indices[e0:e1], dst_all[e0:e1] - b0, b1 - b0, pooled.cpu())
                out = layer.fc_self(h[b0:b1]) + layer.fc_neigh(neigh.to(cuda))
                if l < len(model.layers) - 1:
                    out = model.dropout(model.activation(out))
                y[b0:b1] = out
            h = y
    model.train()
    assert bool(torch.isfinite(got.float()).all()) and torch.equal(_bits(got), _bits(h))


def test_refusals(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import GraphedTrainStep, _live_refusal
    with pytest.raises(NotImplementedError, match="pool"):
        SAGE(FEAT, 16, CLASSES, 3, torch.relu, 0.1, transforms="wide", aggregator_type="pool")
    g, _ = _graph(cuda)
    model = _model(cuda)
    assert "MFMA path" in _live_refusal(model)
    with pytest.raises(NotImplementedError, match="MFMA path"):
        GraphedTrainStep(g, fit.make_sampler("labor", [5, 5, 5]), model, BS, batch_capacity=BS)
