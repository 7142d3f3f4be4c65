"""GPU suite (-m gpu): ``transforms="wide"`` from the models down -- SAGE, GATv2 and GCN at the Cora-like
input width 1433 on the K-panelled MFMA products.  A "wide" model whose layers are all narrow is the "tile" model (SAGE: the
"auto" model) bit for bit; at 1433 columns it is held against the default (library) model by the criterion
tests/test_gpu_gat_tile_path.py uses for tile against library (finite, max|a - b| <= 3 * 2^-8 * max|b|), SAGE's input layer
against fp64 per element (bounds.sage_layer_terms / sage_layer_k), and it trains, runs under a batch capacity and infers off the
CSC like a tile model does at narrow widths."""
import math

import pytest
import torch
import torch.nn.functional as F

from bounds import edge_shape_spec, padded_block
from test_gpu_sage_dense_edges import _check_layer, _report

pytestmark = pytest.mark.gpu

V, E, CLASSES, BS, WIDE = 300, 3500, 4, 32, 1433
BF, NAN = torch.bfloat16, float("nan")
MODELS = ("sage", "gat", "gcn")
DEFAULT = {"sage": "auto", "gat": "library", "gcn": "library"}           # the value each model is built with today
NARROW = {"sage": "auto", "gat": "tile", "gcn": "tile"}                  # what a narrow "wide" model must equal


def _graph(cuda, feat):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, feat, generator=gen).bfloat16()
    labels = torch.randint(0, CLASSES, (V,), generator=gen)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    return g, torch.randperm(V, generator=gen).to(torch.int32).to(cuda)


def _model(cuda, kind, transforms, in_dim, p=0.0):
    from bliss_gnn_amd.model import GATv2, GCN, SAGE
    torch.manual_seed(0)
    if kind == "sage":
        m = SAGE(in_dim, 16, CLASSES, 3, torch.relu, p, transforms=transforms)
    elif kind == "gcn":
        m = GCN(in_dim, 16, CLASSES, 3, torch.relu, p, transforms=transforms)
    else:
        m = GATv2(3, in_dim, 8, CLASSES, [2, 2, 1], F.elu, p, p, 0.2, True, transforms=transforms)
    return m.to(cuda).bfloat16()


def _sampler(kind):
    from bliss_gnn_amd import fit
    return fit.make_sampler("labor", [5, 5, 5], model="gat" if kind == "gat" else "sage")


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


def _forward(model, mfgs):
    """Evaluation-mode forward on ``mfgs`` -> logits, every block's embed_norm and (GATv2) a_ij."""
    from bliss_gnn_amd.train import _inputs
    model.eval()
    with torch.no_grad():
        out = model(mfgs, _inputs(model, mfgs))
    torch.cuda.synchronize()
    return dict(out=out.clone(), n=[b.srcdata["embed_norm"].clone() for b in mfgs],
                a=[b.edata["a_ij"].clone() for b in mfgs if "a_ij" in b.edata])


def _pair(cuda, kind, feat, other):
    """A "wide" model and its ``other`` twin with the same state dict on the same eager blocks."""
    g, perm = _graph(cuda, feat)
    _, _, mfgs = _sampler(kind).sample_blocks(g, perm[:BS])
    wide, twin = _model(cuda, kind, "wide", feat), _model(cuda, kind, other, feat)
    twin.load_state_dict(wide.state_dict())
    return _forward(wide, mfgs), _forward(twin, mfgs)


@pytest.fixture
def wide_calls(monkeypatch):
    """How often each K-panelled entry point is called (the dispatch is per product: only a reduction past 1024 goes wide)."""
    from bliss_gnn_amd import _lib
    calls = {"bliss_tile_gemm_wide": 0, "bliss_dgrad_wide": 0}
    for name in calls:
        real = getattr(_lib.lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)

        monkeypatch.setattr(_lib.lib, name, counted)
    return calls


# ------------------------------------------------------------------------------------------------ the keyword
def test_the_keyword_is_checked(cuda):
    from bliss_gnn_amd.model import GATv2, GCN, SAGE
    from bliss_gnn_amd.nn import TILE_WIDE_MAX_K, GATv2Conv, GraphConv
    for build in (lambda t: SAGE(24, 16, CLASSES, 3, torch.relu, 0.0, transforms=t), lambda t: GCN(24, 16, CLASSES, 3, torch.relu, 0.0, transforms=t),
                  lambda t: GATv2(3, 24, 8, CLASSES, [2, 2, 1], F.elu, 0.0, 0.0, 0.2, True, transforms=t),
                  lambda t: GATv2Conv(24, 8, 2, share_weights=True, transforms=t), lambda t: GraphConv(24, 8, transforms=t)):
        with pytest.raises(ValueError, match="transforms"):
            build("bogus")
        assert build("wide").transforms == "wide"
    assert SAGE(24, 16, CLASSES, 3, torch.relu, 0.0).transforms == "auto"
    assert TILE_WIDE_MAX_K == 16384
    too_wide = TILE_WIDE_MAX_K + 1
    assert GraphConv(too_wide, 8, transforms="wide").tile_refusal("GCN layer 0") is not None
    for why in (GraphConv(too_wide, 8, transforms="wide").tile_refusal("GCN layer 0"),
                GATv2Conv(too_wide, 8, 2, share_weights=True, transforms="wide").tile_refusal("GATv2 layer 0"),
                _model(cuda, "sage", "wide", too_wide).mfma_refusal(torch.zeros(1, too_wide, dtype=BF, device=cuda))):
        assert why is not None and "layer 0" in why and "16384" in why and "wide" in why, why
    assert GraphConv(TILE_WIDE_MAX_K, 8, transforms="wide").to(cuda).bfloat16().tile_refusal() is None
    assert "1024" in GraphConv(8, 1025, transforms="wide").tile_refusal()       # out_feats stays a k of the other products
    assert "1024" in GraphConv(WIDE, 8, transforms="tile").tile_refusal()


def test_a_wide_sage_never_falls_back_to_the_library_path(cuda, monkeypatch):
    """fp32 parameters, an activation other than ReLU, BLISS_SAGE_MFMA=0, a layer outside the limits: NotImplementedError at the
    forward, naming the reason -- where the same model built "auto" runs on library GEMMs without a word."""
    from bliss_gnn_amd.model import SAGE
    g, perm = _graph(cuda, WIDE)
    _, _, mfgs = _sampler("sage").sample_blocks(g, perm[:BS])
    x = mfgs[0].srcdata["features"]
    with pytest.raises(NotImplementedError, match="bf16"):
        _model(cuda, "sage", "wide", WIDE).float()(mfgs, x.float())
    with pytest.raises(NotImplementedError, match="bf16"):
        _model(cuda, "sage", "wide", WIDE).float()(mfgs, x)
    with pytest.raises(NotImplementedError, match="ReLU"):
        SAGE(WIDE, 16, CLASSES, 3, torch.tanh, 0.0, transforms="wide").to(cuda).bfloat16()(mfgs, x)
    with pytest.raises(NotImplementedError, match=r"layer 0.*out_feats <= 256"):
        SAGE(WIDE, 257, CLASSES, 3, torch.relu, 0.0, transforms="wide").to(cuda).bfloat16()(mfgs, x)
    monkeypatch.setenv("BLISS_SAGE_MFMA", "0")
    with pytest.raises(NotImplementedError, match="BLISS_SAGE_MFMA=0"):
        _model(cuda, "sage", "wide", WIDE)(mfgs, x)
    out = _model(cuda, "sage", "auto", WIDE)(mfgs, x)                           # (today's behaviour: the library path, silently)
    assert out.shape == (BS, CLASSES)


# ------------------------------------------------------------------------------------------------ narrow: the bits of before
@pytest.mark.parametrize("kind", MODELS)
def test_a_narrow_wide_model_is_the_tile_model(cuda, kind, wide_calls):
    """in_dim 48: every product is within 1024 columns, so a "wide" model makes the launches of the same model built "tile"
    (SAGE: "auto") -- no call of a K-panelled entry point; logits, every embed_norm and a_ij bit-equal."""
    wide, twin = _pair(cuda, kind, 48, NARROW[kind])
    assert wide_calls == {"bliss_tile_gemm_wide": 0, "bliss_dgrad_wide": 0}
    assert torch.equal(_bits(wide["out"]), _bits(twin["out"]))
    assert len(wide["n"]) == 3 and len(wide["a"]) == (3 if kind == "gat" else 0)
    for name in ("n", "a"):
        for l, (a, b) in enumerate(zip(wide[name], twin[name])):
            assert torch.equal(_bits(a) if a.dtype == BF else a, _bits(b) if b.dtype == BF else b), (name, l)


# ------------------------------------------------------------------------------------------------ 1433 columns
@pytest.mark.parametrize("kind", MODELS)
def test_a_wide_model_matches_the_default_model_at_1433_columns(cuda, kind, wide_calls):
    """Same state dict, same blocks, evaluation mode: logits, every block's embed_norm and GATv2's a_ij finite and within
    3 * 2^-8 of the default model's scale (the tile-against-library criterion of tests/test_gpu_gat_tile_path.py).  Only the
    input layer's product goes to a K-panelled entry point: one launch (SAGE: fc_neigh and fc_self share it; GATv2: fc_src's
    16 columns; GCN: the weight-first X W)."""
    wide, lib = _pair(cuda, kind, WIDE, DEFAULT[kind])
    assert wide_calls == ({"bliss_tile_gemm_wide": 0, "bliss_dgrad_wide": 1} if kind == "gcn" else {"bliss_tile_gemm_wide": 1, "bliss_dgrad_wide": 0})

    def close(a, b, what):
        a, b = a.float(), b.float()
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print("WIDE-vs-DEFAULT", kind, what, err, scale)
        assert bool(torch.isfinite(a).all()) and err <= 3 * 2.0 ** -8 * scale, (what, err, scale)

    close(wide["out"], lib["out"], "logits")
    for l, (a, b) in enumerate(zip(wide["n"], lib["n"])):
        close(a, b, "embed_norm %d" % l)
    assert len(wide["a"]) == len(lib["a"]) == (3 if kind == "gat" else 0)
    for l, (a, b) in enumerate(zip(wide["a"], lib["a"])):
        close(a, b, "a_ij %d" % l)


@pytest.mark.parametrize("gather,p", [(True, 0.0), (False, 0.25)])
def test_the_wide_sage_input_layer_per_element(cuda, gather, p):
    """_SageLinearPair(wide=True) at 1433 -> 64 on the capacity-padded edge-shape block of the message-passing suite, rows gathered
    from a table (repeated ids) or handed in, NaN rows beyond the device-side counts: the layer's output and dW of fc_neigh and
    fc_self (and d b, d h) against fp64 -- bounds.sage_layer_terms with bounds.sage_layer_k(1433, 64, ...), as
    test_sage_layer_nodes_per_element holds the narrow layers."""
    from bliss_gnn_amd import nn as bnn
    fin, fout = WIDE, 64
    spec = edge_shape_spec()
    blk = padded_block(spec, cuda)
    blk._counts_dev[3] = spec.K
    S, K, Sb, Kb = spec.S, spec.K, blk.num_dst_nodes(), blk.num_src_nodes()
    cd = blk._counts_dev.data_ptr()
    gen = torch.Generator().manual_seed(fin + fout)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(BF)
    leaf = lambda t: t.to(cuda).requires_grad_(True)
    wn, ws, b = leaf(rnd(fout, fin, scale=fin ** -0.5)), leaf(rnd(fout, fin, scale=fin ** -0.5)), leaf(rnd(fout))
    ew = (torch.rand(blk.num_edges(), generator=gen) + 0.05).to(BF).to(cuda)
    g = rnd(Sb, fout)
    g[S:] = NAN
    g = g.to(cuda)
    ids = None
    if gather:
        T = K + 50
        ids = torch.zeros(Kb, dtype=torch.int64)
        ids[:K] = torch.randint(0, T, (K,), generator=gen)
        ids = ids.to(torch.int32).to(cuda)
        h = leaf(rnd(T, fin))
        h_ref = h.detach()[ids.long()][:K]
    else:
        h = rnd(Kb, fin)
        h[K:] = NAN
        h = leaf(h)
        h_ref = h.detach()[:K]
    z, y, rows, norm = bnn._SageLinearPair.apply(h, ids, wn, ws, b, Kb, Sb, cd + 12, cd, True)
    assert torch.equal(_bits(norm[:K]), _bits(bnn.embed_norm(h_ref.contiguous()))) and not bool(_bits(norm[K:]).any())
    if gather:
        assert torch.equal(_bits(rows[:K]), _bits(h_ref)) and not bool(_bits(rows[K:]).any())
    ctr = torch.zeros(66, dtype=torch.int64, device=cuda) if p > 0 else None
    out = bnn.sage_epilogue(y, bnn.weighted_aggregate(blk, z, ew, mean=True), p, ctr, 5)[0]
    out.backward(g)
    torch.cuda.synchronize()
    t = dict(out=out.detach(), h=h, h_dst=None, wn=wn, ws=ws, b=b, g=g, ew=ew, h_ref=h_ref, hd_ref=None, ids=ids)
    what = "wide pair edge-padded %d->%d" % (fin, fout)
    _report(what.replace(" ", "-") + "-p%g-g%d" % (p, gather), _check_layer(cuda, spec, True, "pair", fin, fout, True, p, True, gather, t, what))


@pytest.mark.parametrize("kind", MODELS)
def test_training_steps_of_a_wide_model_move_every_parameter(cuda, kind):
    """Two eager steps on exact-size blocks at 1433 columns, dropout 0.1: finite losses, every parameter finite and changed, the
    dropout counters advanced."""
    from bliss_gnn_amd.train import TrainStep
    g, perm = _graph(cuda, WIDE)
    model = _model(cuda, kind, "wide", WIDE, p=0.1)
    model.train()
    before = [q.detach().clone() for q in model.parameters()]
    step = TrainStep(g, _sampler(kind), model, lr=0.01)
    losses = [float(step(perm[i * BS:(i + 1) * BS])) for i in range(2)]
    assert all(math.isfinite(l) and abs(l) < 1e4 for l in losses), losses
    assert all(bool(torch.isfinite(q.float()).all()) and not torch.equal(q, r) for q, r in zip(model.parameters(), before))
    if kind == "gat":
        assert [int(l._feat_state(cuda)["ctr"][0]) for l in model.gatv2_layers] == [2, 2, 2]
        for l in model.gatv2_layers:
            l.check_errors()
    elif kind == "gcn":
        assert [int(l._drop_state(cuda)["ctr"][0]) for l in model.layers] == [2, 2, 0]
    else:
        assert [int(model._dropout_state(l, cuda)[0][0]) for l in range(2)] == [2, 2]


# ------------------------------------------------------------------------------------------------ live batch size
CAP = 24
LIVE = (1, CAP - 1, CAP)


def _live_build(cuda, kind):
    from bliss_gnn_amd.train import BatchLoader
    g, perm = _graph(cuda, WIDE)
    model = _model(cuda, kind, "wide", WIDE, p=0.1 if kind == "gcn" else 0.0)
    model.train()
    tr = perm[:200]
    return g, _sampler(kind), model, tr, BatchLoader(tr, CAP, seed=5).forever()


def _live_batches(tr):
    perm = tr[torch.randperm(tr.numel(), generator=torch.Generator().manual_seed(9)).to(tr.device)]
    out, o = [], 0
    for n in LIVE:
        out.append(perm[o:o + n].clone())
        o += n
    return out


def test_wide_models_are_not_refused_a_batch_capacity(cuda):
    from bliss_gnn_amd.train import _live_refusal
    for kind in MODELS:
        assert _live_refusal(_model(cuda, kind, "wide", WIDE)) is None, kind
        assert _live_refusal(_model(cuda, kind, "wide", 48)) is None, kind
    why = _live_refusal(_model(cuda, "sage", "auto", WIDE))                     # today's refusal stays
    assert why is not None and "MFMA" in why
    assert "bf16" in _live_refusal(_model(cuda, "gcn", "wide", WIDE).float())


@pytest.mark.parametrize("kind", ["sage", "gcn"])
def test_one_captured_wide_step_serves_every_batch_size(cuda, kind, monkeypatch):
    """test_one_captured_gcn_step_serves_every_batch_size at a wide input: one captured GraphedTrainStep(batch_capacity=24) driven
    with 1, 23 and 24 live seeds -- every floating-point buffer it allocates pre-filled with NaN -- against eager TrainStep calls
    of an identically seeded model on the same seeds: the losses of all steps and all parameter bits equal."""
    from bliss_gnn_amd.train import GraphedTrainStep, TrainStep
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)                              # the warm-up steps and (recorded) every replay
    g, s, m, tr, loader = _live_build(cuda, kind)
    step = GraphedTrainStep(g, s, m, CAP, lr=0.01, batch_capacity=CAP)
    torch.manual_seed(3)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)                                              # three real steps of 24 seeds
    losses, sizes = [], []
    for seeds in _live_batches(tr):
        losses.append(float(step(seeds)))
        sizes.append(step.last_counts[0].S)
    monkeypatch.undo()
    assert sizes == list(LIVE)

    gB, sB, mB, trB, loaderB = _live_build(cuda, kind)
    eager = TrainStep(gB, sB, mB, lr=0.01)
    torch.manual_seed(3)
    for _ in range(3):
        sB.sample_blocks(gB, next(loaderB))
    for _ in range(3):
        eager(next(loaderB))
    want = [float(eager(seeds)) for seeds in _live_batches(trB)]
    print(kind, losses, want)
    assert all(math.isfinite(x) for x in losses) and losses == want
    for (k, q), r in zip(m.named_parameters(), mB.parameters()):
        assert bool(torch.isfinite(q.float()).all()) and torch.equal(_bits(q), _bits(r)), k
    if hasattr(step, "close"):
        step.close()


# ------------------------------------------------------------------------------------------------ CSC inference
def test_wide_gcn_inference_off_the_csc(cuda):
    g, _ = _graph(cuda, WIDE)
    model = _model(cuda, "gcn", "wide", WIDE, p=0.5)
    a = model.inference(g, batch_size=7, path="csc").clone()
    b = model.inference(g, batch_size=7, path="blocks").clone()
    assert a.shape == (V, CLASSES) and bool(torch.isfinite(a.float()).all()) and torch.equal(_bits(a), _bits(b))
    model.inference(g, batch_size=7)
    assert model.last_inference_path == "csc"


def test_wide_gat_inference_off_the_csc(cuda):
    g, _ = _graph(cuda, WIDE)
    model = _model(cuda, "gat", "wide", WIDE)
    model.csc_min_rows = 1                                                      # (ranges of node_chunk rows, not one range)
    a = model.inference(g, node_chunk=64, path="csc").clone()
    b = model.inference(g, node_chunk=64, path="blocks").clone()
    assert a.shape == (V, CLASSES) and bool(torch.isfinite(a.float()).all()) and torch.equal(_bits(a), _bits(b))
    model.inference(g, node_chunk=64)
    assert model.last_inference_path == "csc"
