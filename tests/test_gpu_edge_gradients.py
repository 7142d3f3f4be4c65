"""GPU suite (-m gpu): ``explain.edge_gradients`` on a 3-layer SAGE (602 -> 256 -> 256 -> 41, mean,
transforms="auto": the fused MFMA path -- _SageLinearPair + weighted_aggregate, _SageAggDual, _SageLinearPair +
weighted_aggregate) over sampled blocks of the 2000-node Chung-Lu graph of tests/test_gpu_boundary.py.

It must return exactly (torch.equal) what hand-made leaves and torch.autograd.grad give through the same forward, finite and
non-zero for every block, leave every block's edata and every parameter's .grad as they were, do the same through the plain
(library GEMM) path and for the "pool" and "gcn" aggregators, stand in bf16 ones for blocks without edge weights, and refuse the
models whose layers detach or ignore the weights."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEY = "edge_weights"


@pytest.fixture(scope="module")
def sampled(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(2000, 30000, seed=4)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda))
    g.ndata["features"] = torch.randn(2000, 602, generator=torch.Generator().manual_seed(1)).bfloat16().to(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    torch.manual_seed(1)
    _, _, blocks = bg.PoissonBanditLadiesSampler([150, 120, 90]).sample_blocks(g, torch.arange(30, dtype=torch.int32, device=cuda))
    assert len(blocks) == 3 and all(KEY in b.edata for b in blocks)
    return blocks, blocks[0].srcdata["features"]


def _model(cuda, aggregator="mean", hidden=256, classes=41, transforms="auto"):
    from bliss_gnn_amd.model import SAGE
    torch.manual_seed(3)
    m = SAGE(602, hidden, classes, 3, torch.relu, 0.0, transforms=transforms, aggregator_type=aggregator).to(cuda).bfloat16()
    return m.train()


def _objective(classes, cuda):
    c = torch.randn(classes, generator=torch.Generator().manual_seed(8)).to(cuda)
    return lambda y: (y.float() * c).sum()


def _by_hand(model, blocks, x, objective, ones=False):
    old = [b.edata[KEY] if KEY in b.edata else None for b in blocks]
    leaves = [(torch.ones(b.num_edges(), dtype=torch.bfloat16, device=x.device) if (ones or o is None) else o.detach().clone())
              .requires_grad_() for b, o in zip(blocks, old)]
    try:
        for b, leaf in zip(blocks, leaves):
            b.edata[KEY] = leaf
        grads = torch.autograd.grad(objective(model(blocks, x)), leaves)
    finally:
        for b, o in zip(blocks, old):
            if o is None:
                dict.pop(b.edata, KEY, None)
            else:
                b.edata[KEY] = o
    return grads


def _check(model, blocks, x, objective):
    from bliss_gnn_amd import explain
    before = [b.edata[KEY] if KEY in b.edata else None for b in blocks]
    assert all(p.grad is None for p in model.parameters())
    got = explain.edge_gradients(model, blocks, x, objective)
    assert all(p.grad is None for p in model.parameters())
    for b, o in zip(blocks, before):
        assert (KEY in b.edata) == (o is not None) and (o is None or b.edata[KEY] is o)
    want = _by_hand(model, blocks, x, objective)
    assert len(got) == len(blocks)
    for l, (b, gl, wl) in enumerate(zip(blocks, got, want)):
        assert gl.dtype == torch.bfloat16 and gl.shape == (b.num_edges(),) and not gl.requires_grad
        assert torch.equal(gl, wl), l
        assert bool(torch.isfinite(gl.float()).all()) and bool((gl != 0).any()), l
    return got


def test_equals_hand_made_leaves_on_the_mfma_path(sampled, cuda):
    blocks, x = sampled
    model = _model(cuda)
    assert model._mfma_ok(x)
    _check(model, blocks, x, _objective(41, cuda))


def test_equals_hand_made_leaves_on_the_plain_path(sampled, cuda, monkeypatch):
    blocks, x = sampled
    monkeypatch.setenv("BLISS_SAGE_MFMA", "0")
    model = _model(cuda)
    assert not model._mfma_ok(x)
    _check(model, blocks, x, _objective(41, cuda))


@pytest.mark.parametrize("aggregator", ("pool", "gcn"))
def test_pool_and_gcn_models(sampled, cuda, aggregator):
    blocks, x = sampled
    _check(_model(cuda, aggregator, hidden=64, classes=16), blocks, x, _objective(16, cuda))


def test_blocks_without_edge_weights_get_ones(sampled, cuda):
    from bliss_gnn_amd import explain
    blocks, x = sampled
    model, objective = _model(cuda, hidden=64, classes=16), _objective(16, cuda)
    kept = [b.edata[KEY] for b in blocks]
    try:
        for b in blocks:
            dict.pop(b.edata, KEY)
        assert not any(KEY in b.edata for b in blocks)
        got = _check(model, blocks, x, objective)
        assert not any(KEY in b.edata for b in blocks)
        for b, o in zip(blocks, kept):
            b.edata[KEY] = o
        want = _by_hand(model, blocks, x, objective, ones=True)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        for b, o in zip(blocks, kept):
            b.edata[KEY] = o


def test_refusals_on_the_gpu(sampled, cuda):
    from bliss_gnn_amd import explain
    from bliss_gnn_amd.model import GATv2, GCN
    blocks, x = sampled
    before = [b.edata[KEY] for b in blocks]
    models = [_model(cuda, "pool", 64, 16, transforms="tile"), _model(cuda, "gcn", 64, 16, transforms="tile"),
              GCN(602, 32, 16, 3, torch.relu, 0.0, transforms="tile").to(cuda).bfloat16(),
              GCN(602, 32, 16, 3, torch.relu, 0.0, transforms="wide").to(cuda).bfloat16(),
              GATv2(3, 602, 8, 16, [2, 2, 1], torch.relu, 0.0, 0.0, 0.2, False).to(cuda).bfloat16()]
    for m in models:
        with pytest.raises(NotImplementedError, match="edge_gradients"):
            explain.edge_gradients(m, blocks, x, lambda y: y.float().sum())
    assert all(b.edata[KEY] is o for b, o in zip(blocks, before))
    gcn = GCN(602, 32, 16, 3, torch.relu, 0.0).to(cuda).bfloat16().train()          # "library": differentiates
    got = explain.edge_gradients(gcn, blocks, x, _objective(16, cuda))
    assert all(bool(torch.isfinite(gl.float()).all()) and bool((gl != 0).any()) for gl in got)
