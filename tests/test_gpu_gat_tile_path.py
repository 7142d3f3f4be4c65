"""GPU suite (-m gpu): ``GATv2(..., transforms="tile")`` against the default model on the same static-shape
(capacity-padded) blocks without a batch capacity: logits, ``a_ij`` and ``embed_norm`` within the fused-against-library tolerance
of section 3 (``3 * 2^-8`` of the tensor's scale: both round to bf16 where the reference's tensor ops round, the tile GEMM
accumulates its K terms in another order than the library's); the keyword's refusals."""
import pytest
import torch
import torch.nn.functional as F

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


def _model(cuda, transforms, in_dim=FEAT, **kw):
    from bliss_gnn_amd.model import GATv2
    torch.manual_seed(0)
    return GATv2(3, in_dim, 8, CLASSES, [2, 2, 1], F.elu, 0.0, 0.0, 0.2, True, transforms=transforms, **kw).to(cuda).bfloat16()


@pytest.mark.parametrize("name,fan", [("labor", [5, 5, 5]), ("poisson-bandit-keyed", [24, 16, 12])])
def test_tile_model_matches_the_default_on_a_static_step(cuda, name, fan):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    g, perm = _graph(cuda)
    sampler = fit.make_sampler(name, fan, model="gat")
    tile, lib = _model(cuda, "tile"), _model(cuda, "library")
    lib.load_state_dict(tile.state_dict())
    tile.eval(), lib.eval()
    step = GraphedTrainStep(g, sampler, tile, BS, lr=0.01)
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
        got[kind] = dict(out=out.clone(), a=[b.edata["a_ij"].clone() for b in mfgs], n=[b.srcdata["embed_norm"].clone() for b in mfgs])
    torch.cuda.synchronize()
    counts = list(reversed(sampler.finish_static()))                            # block order
    assert mfgs[-1].num_dst_nodes() == BS and counts[-1].S == BS
    assert any(c.K < b.num_src_nodes() for c, b in zip(counts, mfgs))           # the blocks are padded: the bounds matter

    def close(a, b, what):
        a, b = a.float(), b.float()
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print("TILE-vs-LIBRARY", name, what, err, scale)
        assert bool(torch.isfinite(a).all()) and err <= 3 * 2.0 ** -8 * scale, (what, err, scale)

    close(got["tile"]["out"][:BS], got["library"]["out"][:BS], "logits")
    for l, c in enumerate(counts):
        close(got["tile"]["a"][l][:c.B], got["library"]["a"][l][:c.B], "a_ij %d" % l)
        close(got["tile"]["n"][l][:c.K], got["library"]["n"][l][:c.K], "embed_norm %d" % l)
        assert not bool(got["tile"]["n"][l][c.K:].view(torch.int16).any()) or l == 0      # hidden rows past the count are zero rows


def test_training_step_of_the_tile_model_moves_every_parameter(cuda):
    """Eager exact-size blocks, dropout on: finite loss, a finite gradient for every parameter, the dropout counters advance."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import GATv2
    from bliss_gnn_amd.train import TrainStep
    g, perm = _graph(cuda)
    sampler = fit.make_sampler("labor", [5, 5, 5])
    torch.manual_seed(0)
    model = GATv2(3, FEAT, 8, CLASSES, [2, 2, 1], F.elu, 0.1, 0.1, 0.2, True, transforms="tile").to(cuda).bfloat16()
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    step = TrainStep(g, sampler, model, lr=0.01)
    losses = [float(step(perm[i * BS:(i + 1) * BS])) for i in range(2)]
    assert all(l == l and abs(l) < 1e4 for l in losses), losses
    assert all(bool(torch.isfinite(p.float()).all()) and not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert [int(l._feat_state(cuda)["ctr"][0]) for l in model.gatv2_layers] == [2, 2, 2]
    for l in model.gatv2_layers:
        l.check_errors()


def test_the_keyword_is_checked(cuda):
    from bliss_gnn_amd.model import GATv2
    from bliss_gnn_amd.nn import GATv2Conv
    with pytest.raises(ValueError, match="transforms"):
        GATv2(3, FEAT, 8, CLASSES, [2, 2, 1], F.elu, 0.0, 0.0, 0.2, True, transforms="bogus")
    with pytest.raises(ValueError, match="transforms"):
        GATv2Conv(FEAT, 8, 2, share_weights=True, transforms="bogus")
    assert GATv2(3, FEAT, 8, CLASSES, [2, 2, 1], F.elu, 0.0, 0.0, 0.2, True).transforms == "library"


def test_an_input_width_past_the_tile_kernels_limit_is_refused_at_the_first_forward(cuda):
    """The Cora-like width 1433: no silent fall-back to the library GEMM; the message names the layer and the limit."""
    from bliss_gnn_amd import fit
    g, perm = _graph(cuda, feat=1433)
    model = _model(cuda, "tile", in_dim=1433)                                   # building it is fine
    _, _, mfgs = fit.make_sampler("labor", [5, 5, 5]).sample_blocks(g, perm[:16])
    with pytest.raises(NotImplementedError, match=r"layer 0.*1024"):
        model(mfgs, mfgs[0].srcdata["features"])
    fp32 = _model(cuda, "tile").float()
    g2, _ = _graph(cuda)
    _, _, mfgs = fit.make_sampler("labor", [5, 5, 5]).sample_blocks(g2, perm[:16])
    with pytest.raises(NotImplementedError, match="bf16"):
        fp32(mfgs, mfgs[0].srcdata["features"].float())


def test_tile_conv_alone_matches_the_default_conv(cuda):
    """``GATv2Conv(transforms="tile")`` on an exact-size block: output and logits against the default layer."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.nn import GATv2Conv
    g, perm = _graph(cuda)
    _, _, (blk,) = fit.make_sampler("labor", [6]).sample_blocks(g, perm[:40])
    mk = lambda t: GATv2Conv(FEAT, 96, 3, 0.0, 0.0, 0.2, True, F.elu, bias=True, share_weights=True, allow_zero_in_degree=True, transforms=t)
    torch.manual_seed(1)
    a = mk("tile").to(cuda).bfloat16()
    b = mk("library").to(cuda).bfloat16()
    b.load_state_dict(a.state_dict())
    h = blk.srcdata["features"]
    outs = []
    for layer in (a, b):
        hd = h.clone().requires_grad_(True)
        out, e = layer(blk, hd, get_attention=True)
        out.float().square().sum().backward()
        outs.append((out.detach(), e.detach(), hd.grad, layer.fc_src.weight.grad, layer.res_fc.weight.grad))
    for name, x, y in zip(("out", "e", "d h", "d W_src", "d W_res"), outs[0], outs[1]):
        x, y = x.float(), y.float()
        assert x.shape == y.shape and float((x - y).abs().max()) <= 4 * 2.0 ** -8 * float(y.abs().max()), name
