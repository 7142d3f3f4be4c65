"""GPU suite (-m gpu): SAGEConv 'gcn' on the bounded kernels -- ``nn.sage_gcn_tile`` per layer and
``SAGE(..., aggregator_type="gcn", transforms="tile")`` under a batch capacity.

Per layer, at in/out = 602 -> 256, 256 -> 256, 256 -> 41 (fc_neigh first where in > out) and 8 -> 41 (the aggregation first): output
and gradients per element against the fp64 restatement (spmm_self_ref.layer_terms) under spmm_self_ref.layer_k, on the edge-shape
block exact-size and capacity-padded (NaN feature rows, edge weights and gradient rows past the live counts; every buffer the layer
allocates pre-filled with NaN), with and without dropout.  The kept mask is taken from the stored output: without dropout, where the
reference is positive the output is compared as it is, and where it is <= 0 the output (>= 0) must lie within the bound of the
pre-activation value (``ref + out`` against ``ref``); with dropout p the elements the kernel kept (out != 0) are compared with
rst / (1 - p), and the kept share of the clearly positive elements (rst above 2^-6 of its magnitude: far beyond its bound) must be
1 - p within 0.06 (>= 1000 such elements: a binomial's standard deviation is below 0.016).

The model: one captured ``GraphedTrainStep(batch_capacity=64)`` driven with 64, 63, 1 and 64 live seeds against eager ``TrainStep``
calls of an identically seeded model on the same seeds, bit for bit; ``fit(vertex_limit=)`` completes two epochs; a first forward
outside the limits raises."""
import math

import pytest
import torch

import bounds
import spmm_self_ref as ref
from test_gpu_gcn_live_step import CAP, CLASSES, FEAT, SAMPLERS, _task

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LIVE = (CAP, CAP - 1, 1, CAP)


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


@pytest.fixture
def nan_empty(monkeypatch):
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)


@pytest.fixture(scope="module")
def blocks(cuda):
    spec = bounds.edge_shape_spec()
    pad = bounds.padded_block(spec, cuda)
    pad._counts_dev[3] = spec.K                         # bliss_layer_counts_t::K: the dense products are bound by the live source count
    return spec, bounds.to_block(spec, cuda), pad


def _layer(cuda, fin, fout, seed=2):
    from bliss_gnn_amd.nn import SAGEConv, SAGEGCNConv
    torch.manual_seed(seed)
    layer = SAGEGCNConv(fin, fout).to(cuda).bfloat16()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(fout, generator=torch.Generator().manual_seed(9)).bfloat16() * 0.1)
    return layer


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("fin,fout", [(602, 256), (256, 256), (256, 41), (8, 41)])
def test_layer_forward_and_gradients_per_element(cuda, blocks, nan_empty, fin, fout, p):
    from bliss_gnn_amd import ops
    from bliss_gnn_amd.nn import gat_drop_state, sage_gcn_tile
    spec, blk, pad = blocks
    S, K, B = spec.S, spec.K, spec.B
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    layer = _layer(cuda, fin, fout)
    gen = torch.Generator().manual_seed(3 + fin)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=BF)
    x = torch.cat([torch.randn(K, fin, generator=gen).bfloat16(), nan(Kc - K, fin)]).to(cuda)
    w = torch.cat([(torch.rand(B, generator=gen) + 0.05).bfloat16(), nan(Bc - B)]).to(cuda)
    g = torch.cat([torch.randn(S, fout, generator=gen).bfloat16(), nan(Sc - S, fout)]).to(cuda)
    state = gat_drop_state(1, cuda) if p > 0 else None
    idx = tuple(t.to(cuda) for t in (spec.indptr, spec.src, spec.dst))
    k = ref.layer_k(fin, fout, Kc, p > 0)
    runs, r = {}, {}
    for name, b, k_rows, s_rows, n_e in (("exact", blk, K, S, B), ("padded", pad, Kc, Sc, Bc)):
        layer.zero_grad(set_to_none=True)
        xi = x[:k_rows].clone().requires_grad_(True)
        out, norm = sage_gcn_tile(b, xi, w[:n_e].contiguous(), layer, True, p, state, True)
        out.backward(g[:s_rows].contiguous())
        out = out.detach()
        assert not bool(_bits(out[S:]).any()) and not bool(_bits(xi.grad[K:]).any()) and not bool(_bits(norm[S:]).any()), name + ": rows past the counts"
        assert torch.equal(_bits(norm[:S]), _bits(ops.embed_norm(out[:S].contiguous()))), name + ": the stored rows' norms"
        runs[name] = (out[:S], xi.grad[:K], layer.fc_neigh.weight.grad.clone(), layer.bias.grad.clone())
        T = ref.layer_terms(*idx, x[:K], layer.fc_neigh.weight, bias=layer.bias, ew=w[:B], g=g[:S], mask=out[:S] != 0, p=p, relu=True)
        rst, o = T["rst"], out[:S].double()
        if p > 0:
            kept = o != 0
            r[name + " out"] = bounds.assert_within(o[kept], (rst / (1 - p))[kept], (T["mag_rst"] / (1 - p))[kept], *k["out"], name + " out (kept)")
            clear = rst > 2.0 ** -6 * T["mag_rst"]
            share = float(kept[clear].double().mean())
            assert int(clear.sum()) >= 1000, int(clear.sum())
            assert abs(share - (1 - p)) < 0.06, share
            assert not bool((o < 0).any())
        else:
            r[name + " out"] = bounds.assert_within(torch.where(rst > 0, o, rst + o), rst, T["mag_rst"], *k["out"], name + " out")
        for key, got in (("d_h", runs[name][1]), ("d_w", runs[name][2]), ("d_b", runs[name][3])):
            r[name + " " + key] = bounds.assert_within(got, T[key], T["mag_" + key], *k[key], name + " " + key)
    if p == 0:
        for a, b2, what in zip(runs["exact"], runs["padded"], ("out", "d_h", "d_w", "d_b")):
            if what != "d_w":                                            # (dW's chunked sum is cut by the row bound, not the live count)
                assert torch.equal(_bits(a), _bits(b2)), what + ": live rows bit-equal to the exact block"
    print("SAGE-GCN-TILE %dx%d p %.2f:" % (fin, fout, p), " ".join("%s %.3f" % kv for kv in sorted(r.items())))


@pytest.mark.parametrize("fin,fout", [(8, 4), (4, 8)])
def test_tile_layer_on_integers_equals_fp64(cuda, fin, fout):
    from bliss_gnn_amd.nn import SAGEGCNConv, sage_gcn_tile
    c = ref.exact_case(fin, fout)
    blk = bounds.to_block(bounds.Spec(c["K"], c["S"], c["indptr"], c["src"], c["dst"]), cuda)
    layer = SAGEGCNConv(fin, fout).to(cuda).bfloat16()
    with torch.no_grad():
        layer.fc_neigh.weight.copy_(c["w_neigh"].to(cuda))
        layer.bias.copy_(c["bias"].to(cuda))
    h = c["h"].to(cuda).requires_grad_()
    out, _ = sage_gcn_tile(blk, h, c["ew"].to(cuda), layer, True, 0.0, None, False)
    out.backward(c["g"].to(cuda))
    want = ref.layer_terms(c["indptr"], c["src"], c["dst"], c["h"], c["w_neigh"], bias=c["bias"], ew=c["ew"], g=c["g"], relu=True)
    for name, got in (("out", out), ("d_h", h.grad), ("d_w", layer.fc_neigh.weight.grad), ("d_b", layer.bias.grad)):
        assert torch.equal(got.detach().double().cpu(), want[name]), name


# ------------------------------------------------------------------------------------------------ the model under a capacity
def _model(cuda, transforms="tile", hidden=16, act=torch.relu):
    from bliss_gnn_amd.model import SAGE
    torch.manual_seed(0)
    m = SAGE(FEAT, hidden, CLASSES, 3, act, 0.1, transforms=transforms, aggregator_type="gcn").to(cuda).bfloat16()
    m.train()
    return m


def _build(cuda, name, transforms="tile"):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader
    g, tr = _task(cuda)
    return g, fit.make_sampler(name, SAMPLERS[name]), _model(cuda, transforms), tr, BatchLoader(tr, CAP, seed=5).forever()


def _live_batches(tr):
    perm = tr[torch.randperm(tr.numel(), generator=torch.Generator().manual_seed(9)).to(tr.device)]
    out, o = [], 0
    for n in LIVE:
        out.append(perm[o:o + n].clone())
        o += n
    return out


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_one_captured_step_serves_every_batch_size(cuda, name, monkeypatch):
    from bliss_gnn_amd.train import GraphedTrainStep, TrainStep, _live_refusal
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)                              # the warm-up steps and (recorded) every replay
    g, s, m, tr, loader = _build(cuda, name)
    assert _live_refusal(m) is None and [l._in_src_feats > l._out_feats for l in m.layers] == [True, False, True]
    step = GraphedTrainStep(g, s, m, CAP, lr=0.01, batch_capacity=CAP)
    torch.manual_seed(3)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)                                              # three real steps of 64 seeds
    losses, sizes = [], []
    for seeds in _live_batches(tr):
        losses.append(float(step(seeds)))
        sizes.append(step.last_counts[0].S)
    monkeypatch.undo()
    assert sizes == list(LIVE)

    gB, sB, mB, trB, loaderB = _build(cuda, name)
    eager = TrainStep(gB, sB, mB, lr=0.01)
    torch.manual_seed(3)
    for _ in range(3):
        sB.sample_blocks(gB, next(loaderB))
    for _ in range(3):
        eager(next(loaderB))
    want = [float(eager(seeds)) for seeds in _live_batches(trB)]
    print(name, losses, want)
    assert all(math.isfinite(x) for x in losses) and losses == want
    for (k, p), q in zip(m.named_parameters(), mB.parameters()):
        assert bool(torch.isfinite(p.float()).all()) and torch.equal(_bits(p), _bits(q)), k
    if getattr(s, "_w_pos", None) is not None:                                  # the bandit sampler's EXP3 rows (its reward reads embed_norm)
        assert torch.equal(_bits(s._w_pos), _bits(sB._w_pos))
        assert not torch.equal(_bits(s._w_pos[0]), _bits(torch.ones_like(s._w_pos[0])))
    s.check_errors() if hasattr(s, "check_errors") else None
    ctrs = lambda model: [int(model._gcn_drop_state(l, cuda)["ctr"][0]) for l in range(2)]
    assert ctrs(m) == ctrs(mB) and ctrs(m)[0] > 0                               # the dropout streams advanced alike
    if hasattr(step, "close"):
        step.close()


def test_fit_under_a_vertex_limit(cuda):
    """Two epochs of the graphed loop under a vertex limit, replayed validation: finite losses, every parameter moved."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader
    g, sampler, model, tr, _ = _build(cuda, "labor")
    gen = torch.Generator().manual_seed(6)
    rest = torch.randperm(g.num_nodes(), generator=gen).to(torch.int32).to(cuda)
    va, te = rest[:100], rest[100:200]
    torch.manual_seed(11)
    loader = BatchLoader(tr, CAP, seed=0).forever()
    ks = [sampler.sample_blocks(g, next(loader))[2][0].num_src_nodes() for _ in range(4)]
    before = [p.detach().clone() for p in model.parameters()]
    torch.manual_seed(11)
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=CAP, lr=0.01, max_epochs=2, train_step="graphed", eval_step="graphed",
                  vertex_limit=int(sum(ks) / len(ks) / 2), batch_capacity=2 * CAP)
    hist = out["history"]
    print([(h["batch_size"], h["train_loss"], h["val_loss"]) for h in hist])
    assert len(hist) == 2 and all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in hist)
    for (n, p), q in zip(model.named_parameters(), before):
        assert bool(torch.isfinite(p.float()).all()) and not torch.equal(p, q), n


def test_a_first_forward_outside_the_limits_raises(cuda, monkeypatch):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import _live_refusal
    g, tr = _task(cuda)
    _, _, mfgs = fit.make_sampler("labor", SAMPLERS["labor"]).sample_blocks(g, tr[:CAP])
    x = mfgs[0].srcdata["features"]
    for model, word in ((_model(cuda, hidden=300), "out_feats <= 256"), (_model(cuda, act=torch.tanh), "ReLU"), (_model(cuda).float(), "bf16")):
        assert word in model.tile_refusal(x) and word in _live_refusal(model)
        with pytest.raises(NotImplementedError, match=word):
            model(mfgs, x)
    own = _model(cuda)
    own.layers[1].feat_drop.p = 0.1
    with pytest.raises(NotImplementedError, match="feat_drop"):
        own(mfgs, x)
    tile = _model(cuda)
    for env in ("BLISS_SAGE_MFMA", "BLISS_SAGE_MFMA_BWD"):
        monkeypatch.setenv(env, "0")
        with pytest.raises(NotImplementedError, match=env):
            tile(mfgs, x)
        monkeypatch.delenv(env)
    assert tile.tile_refusal(x) is None and tile(mfgs, x).shape == (CAP, CLASSES)
