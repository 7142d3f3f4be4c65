"""GPU suite (-m gpu): ``GCN(..., transforms="tile")`` against the default model on the same static-shape
(capacity-padded) blocks without a batch capacity: logits and ``embed_norm`` within ``3 * 2^-8`` of the tensor's scale (the bound
DESIGN.md section 22 used for its tile-against-library comparison: both round to bf16, the tile path at fewer points and with its
products accumulated in another order); ``GCN.inference`` of a tile model against the default within the same bound; one
training step of the tile model moves every parameter; the keyword is checked."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, E, FEAT, CLASSES, BS = 600, 7000, 24, 4, 48


def _graph(cuda, feat=FEAT):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, feat, generator=gen).bfloat16()
    labels = torch.randint(0, CLASSES, (V,), generator=gen)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    return g, torch.randperm(V, generator=gen).to(torch.int32).to(cuda)


def _model(cuda, transforms, in_dim=FEAT, p=0.0):
    from bliss_gnn_amd.model import GCN
    torch.manual_seed(0)
    return GCN(in_dim, 16, CLASSES, 3, torch.relu, p, transforms=transforms).to(cuda).bfloat16()


def _close(a, b, what):
    a, b = a.float(), b.float()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print("GCN TILE-vs-LIBRARY", what, err, scale)
    assert bool(torch.isfinite(a).all()) and err <= 3 * 2.0 ** -8 * scale, (what, err, scale)


@pytest.mark.parametrize("name,fan", [("labor", [5, 5, 5]), ("poisson-bandit-keyed", [24, 16, 12])])
def test_tile_model_matches_the_default_on_a_static_step(cuda, name, fan):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    g, perm = _graph(cuda)
    sampler = fit.make_sampler(name, fan)
    tile, lib = _model(cuda, "tile"), _model(cuda, "library")
    lib.load_state_dict(tile.state_dict())
    tile.eval(), lib.eval()
    step = GraphedTrainStep(g, sampler, lib, BS, lr=0.01)
    torch.manual_seed(3)
    step.calibrate(BatchLoader(perm[:400], BS, seed=5).forever(), steps=3)
    step._load_batch(perm[:BS])
    sampler._engine.stage_rng_from_torch()
    _, _, mfgs = sampler.sample_blocks_static(g, step.seeds)
    x = mfgs[0].srcdata["features"]
    got = {}
    for kind, model in (("tile", tile), ("library", lib)):
        with torch.no_grad():
            out = model(mfgs, x)
        got[kind] = dict(out=out.clone(), n=[b.srcdata["embed_norm"].clone() for b in mfgs])
    torch.cuda.synchronize()
    counts = list(reversed(sampler.finish_static()))                            # block order
    assert mfgs[-1].num_dst_nodes() == BS and counts[-1].S == BS
    assert any(c.K < b.num_src_nodes() for c, b in zip(counts, mfgs))           # the blocks are padded: the bounds matter
    _close(got["tile"]["out"][:BS], got["library"]["out"][:BS], "logits")
    for l, c in enumerate(counts):
        _close(got["tile"]["n"][l][:c.K], got["library"]["n"][l][:c.K], "embed_norm %d" % l)
        assert not bool(got["tile"]["n"][l][c.K:].view(torch.int16).any()) or l == 0      # hidden rows past the count are zero rows


def test_inference_of_a_tile_model_matches_the_default(cuda):
    g, _ = _graph(cuda)
    tile, lib = _model(cuda, "tile", p=0.5), _model(cuda, "library", p=0.5)
    lib.load_state_dict(tile.state_dict())
    for bs in (128, 500):
        a = tile.inference(g, batch_size=bs).clone()
        b = lib.inference(g, batch_size=bs).clone()
        assert a.shape == b.shape == (V, CLASSES) and tile.training and lib.training
        _close(a, b, "inference batch_size %d" % bs)


def test_training_step_of_the_tile_model_moves_every_parameter(cuda):
    """Eager exact-size blocks, dropout on: finite losses, every parameter moves, the hidden layers' dropout counters advance."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import TrainStep
    g, perm = _graph(cuda)
    sampler = fit.make_sampler("labor", [5, 5, 5])
    model = _model(cuda, "tile", p=0.1)
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    step = TrainStep(g, sampler, model, lr=0.01)
    losses = [float(step(perm[i * BS:(i + 1) * BS])) for i in range(2)]
    assert all(l == l and abs(l) < 1e4 for l in losses), losses
    assert all(bool(torch.isfinite(p.float()).all()) and not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert [int(l._drop_state(cuda)["ctr"][0]) for l in model.layers] == [2, 2, 0]


def test_the_keyword_is_checked(cuda):
    from bliss_gnn_amd.model import GCN
    from bliss_gnn_amd.nn import GraphConv
    with pytest.raises(ValueError, match="transforms"):
        GCN(FEAT, 16, CLASSES, 3, torch.relu, 0.0, transforms="bogus")
    with pytest.raises(ValueError, match="transforms"):
        GraphConv(FEAT, 8, transforms="bogus")
    assert GCN(FEAT, 16, CLASSES, 3, torch.relu, 0.0).transforms == "library"
    assert all(l.transforms == "tile" for l in GCN(FEAT, 16, CLASSES, 3, torch.relu, 0.0, transforms="tile").layers)


def test_a_width_past_the_limit_is_refused_at_the_first_forward(cuda):
    """The Cora-like width 1433: no silent fall-back to the library path; the message names the layer and the limit."""
    from bliss_gnn_amd import fit
    g, perm = _graph(cuda, feat=1433)
    model = _model(cuda, "tile", in_dim=1433)                                   # building it is fine
    _, _, mfgs = fit.make_sampler("labor", [5, 5, 5]).sample_blocks(g, perm[:16])
    with pytest.raises(NotImplementedError, match=r"layer 0.*1024"):
        model(mfgs, mfgs[0].srcdata["features"])
