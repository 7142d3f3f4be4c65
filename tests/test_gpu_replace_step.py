"""GPU suite (-m gpu): the samplers that draw WITH replacement on the device through their classes --
``LadiesSampler`` / ``BanditLadiesSampler(draw="device-replace")`` against the oracle driven with the restatement's picks
(tests/replace_ref.py), ``NeighborSampler(draw="device", replace=True)`` with and without ``prob`` against the restatement; each of
them replayed from a HIP graph against the eager step, under a batch capacity, and through ``fit(train_step="graphed")``; a GATv2
step on blocks with repeated edges; the refusals."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import replace_ref as ref
import wneighbor_ref as wref
from conftest import bf16_bits
from test_gpu_fit import _task as fit_task
from test_gpu_mn_sampler import BS, DRAW_SEED, FAN, graph_cpu  # noqa: F401  (graph_cpu: a fixture)
from test_gpu_mn_sampler import _graph as mn_graph

pytestmark = pytest.mark.gpu

NB_FAN = [8, 4, 4]
NAMES = ["ladies", "bandit", "neighbor", "neighbor-prob"]
CAP, LIVE = 64, (64, 37, 1, 64)


def _with_prob(g):
    """``g.edata["p"]``: edge probabilities by edge id over eight octaves with a fifth zeros -- unlike ``w`` (1 / in-degree: equal
    inside a column, so the weighted draw would pick what the uniform one picks) they change the draw and the weights."""
    E = g.num_edges()
    gen = torch.Generator().manual_seed(8)
    p = torch.exp2(torch.rand(E, generator=gen) * 8 - 5).bfloat16()
    p[torch.randperm(E, generator=gen)[:E // 5]] = 0.0
    g.edata["p"] = p.to(g.device)
    return g


def _graph(graph_cpu, cuda):
    return _with_prob(mn_graph(graph_cpu, cuda))


def _sampler(name):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    if name == "bandit":
        s = bg.BanditLadiesSampler(FAN, eta=0.1, node_embedding="features", draw="device-replace")
    elif name == "ladies":
        s = bg.LadiesSampler(FAN, draw="device-replace")
    else:
        s = fit.NeighborSampler(NB_FAN, draw="device", replace=True, prob="p" if name == "neighbor-prob" else None)
    s.reset_draw(seed=DRAW_SEED)
    return s


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_layer_wise_blocks_equal_the_oracle_driven_with_the_restatements_picks(cuda, graph_cpu, kind):
    """tests/test_gpu_mn_sampler.py's arrangement: per layer the oracle's candidates and importances are the device's, the picks
    are the restatement's on the ORACLE's p, and the oracle's generate_block -- whose union drops the repeated picks -- gives the
    device's block bit for bit (for the bandit also the EXP3 rows after exp3)."""
    import bliss_gnn_amd as bg
    from oracle import bliss_oracle as bo
    ip, ix, ei = graph_cpu[:3]
    g = _graph(graph_cpu, cuda)
    og = bo.CSC(ip, ix, ei)
    edge_w = bo.normalized_edata(og)
    bandit = kind == "bandit"
    s = _sampler(kind)
    o_w = torch.ones(len(FAN), og.num_edges, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(8)
    repeats = 0
    for step in range(2):
        seeds = torch.arange(30 * step, 30 * step + BS, dtype=torch.int32)
        _, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        assert s.draw_step() == step + 1
        o_blocks, seed_nodes = [], seeds.to(torch.int64)
        for n, block_id in enumerate(reversed(range(len(FAN)))):
            blk = blocks[block_id]
            fr = bo.expand_frontier(og, seed_nodes)
            if bandit:
                W, _ = bo.exp3_edge_prob(og, fr, o_w[block_id], 0.1)
                p, _ = bo.bandit_node_importance(fr, W, True)
            else:
                W = edge_w[fr.eid]
                p, _ = bo.ladies_node_importance(fr, W, True)
            tr = blk._trace
            assert np.array_equal(tr["cand_nid"].cpu().numpy(), fr.nid.numpy().astype(np.int32))
            assert np.array_equal(bf16_bits(tr["p"]), bf16_bits(p.bfloat16()))
            picks, drawn = ref.mn_draw(bf16_bits(p.bfloat16()), FAN[block_id], DRAW_SEED, step, n)
            assert len(picks) == min(FAN[block_id], fr.nid.numel())
            repeats += len(picks) - int(drawn.sum())
            ob = bo.generate_block(og, fr, torch.from_numpy(picks.astype(np.int64)), p, W, hajek=bandit)
            assert blk.num_src_nodes() <= FAN[block_id] + seed_nodes.numel()     # the K capacity is still an exact bound
            assert np.array_equal(ob.indptr.numpy(), blk.indptr.cpu().numpy())
            assert np.array_equal(ob.src.numpy(), blk.src.cpu().numpy()) and np.array_equal(ob.dst.numpy(), blk.dst.cpu().numpy())
            assert np.array_equal(ob.eid.numpy(), blk.edata[bg.EID].cpu().numpy())
            assert np.array_equal(ob.src_nid.numpy(), blk.srcdata[bg.NID].cpu().numpy())
            assert np.array_equal(bf16_bits(ob.edge_weights), bf16_bits(blk.edata["edge_weights"]))
            if bandit:
                assert np.array_equal(bf16_bits(ob.q_ij), bf16_bits(blk.edata["q_ij"]))
                assert np.array_equal(bf16_bits(ob.node_prob), bf16_bits(blk.srcdata["node_prob"]))
            seed_nodes = ob.src_nid
            o_blocks.insert(0, ob)
        if bandit:
            en = []
            for b, ob in zip(blocks, o_blocks):
                e_ = (torch.rand(ob.n_src, generator=gen) * 20).bfloat16()
                b.srcdata["embed_norm"] = e_.to(cuda)
                en.append(e_)
            s.exp3(blocks, g)
            s.check_errors()
            o_w, _ = bo.exp3(og, o_blocks, o_w, edge_w, en)
            assert np.array_equal(bf16_bits(s.exp3_weights), bf16_bits(o_w))
    assert repeats > 0                                                            # (the draws did repeat: the union had work to do)


@pytest.mark.parametrize("name", ["neighbor", "neighbor-prob"])
def test_neighbor_blocks_equal_the_restatement(cuda, graph_cpu, name):
    """Three layers through the class and the engine's exact-size path: every block array, the sources, q_ij and the weights."""
    import bliss_gnn_amd as bg
    ip, ix, ei = (t.numpy() for t in graph_cpu[:3])
    g = _graph(graph_cpu, cuda)
    s = _sampler(name)
    pb = None
    if name == "neighbor-prob":
        pb = wref.bf16_bits(g.by_position(g.edata["p"]).float().cpu().numpy())
    for step in range(2):
        seeds = torch.arange(30 * step, 30 * step + BS, dtype=torch.int32)
        _, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        lays = ref.sample_blocks(ip, ix, ei, seeds.numpy(), list(reversed(NB_FAN)), DRAW_SEED, step, prob_bits=pb)
        for blk, want in zip(reversed(blocks), lays):
            c = blk._counts
            n = lambda t: t.cpu().numpy()
            t_indptr, t_edge = blk._transposed
            got = dict(S=c.S, E=c.E, K=c.K, B=c.B, indptr=n(blk.indptr), pos=n(blk.pos), dst=n(blk.dst), eid=n(blk.edata[bg.EID]),
                       src=n(blk.src), kept_nid=n(blk.srcdata[bg.NID]), t_indptr=n(t_indptr[:c.K + 1]), t_edge=n(t_edge[:c.B]),
                       q_ij=bf16_bits(blk._q), weights=n(blk.edata["edge_weights"].float()), picks=want["picks"])
            ref.compare(got, want)
            assert ("q_ij" in blk.edata) == (pb is not None)
            if pb is not None:
                assert not bool((blk.edata["edge_weights"] == 1).all())         # (these probabilities do weigh the edges)
    assert s.draw_step() == 2
    caps = s._engine.caps                                                         # B = S * fanout: an exact bound, |E| is none
    assert all(c["B"] == c["S"] * f for c, f in zip(caps, reversed(NB_FAN)))


def _build(cuda, graph_cpu, name):
    from bliss_gnn_amd.model import SAGE
    g = _graph(graph_cpu, cuda)
    s = _sampler(name)
    torch.manual_seed(0)
    model = SAGE(32, 16, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    model.train()
    return g, s, model


@pytest.mark.parametrize("name", NAMES)
def test_graphed_step_matches_the_eager_step(cuda, graph_cpu, name):
    """tests/test_gpu_mn_sampler.py's arrangement: A = TrainStep, B = GraphedTrainStep on the same loader with the same number of
    sampler calls (calibrate 3, warm-up 2, the captured step, 4 replays).  Sizes, loss, parameters and the EXP3 rows are
    bit-identical, the draw step is the number of sampler calls, torch's generator is untouched."""
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep
    ids = torch.arange(6000, dtype=torch.int32, device=cuda)
    g1, s1, m1 = _build(cuda, graph_cpu, name)
    eager = TrainStep(g1, s1, m1)
    l1 = BatchLoader(ids, BS, seed=5).forever()
    g2, s2, m2 = _build(cuda, graph_cpu, name)
    graphed = GraphedTrainStep(g2, s2, m2, BS)
    l2 = BatchLoader(ids, BS, seed=5).forever()
    torch.manual_seed(9)
    rng0 = torch.get_rng_state()
    graphed.calibrate(l2, steps=3)
    graphed.capture(l2, warmup=2)
    losses2 = [float(graphed(next(l2))) for _ in range(4)]
    for _ in range(3):                                                            # the calibration's sampler calls train nothing
        s1.sample_blocks(g1, next(l1))
    losses1 = [float(eager(next(l1))) for _ in range(7)]
    assert torch.equal(torch.get_rng_state(), rng0), "the device draw must not touch torch's CPU generator"
    assert s1.draw_step() == s2.draw_step() == 10
    sizes1 = [(b._counts.S, b._counts.E, b._counts.C, b._counts.K, b._counts.B) for b in reversed(eager.last["mfgs"])]
    sizes2 = [(c.S, c.E, c.C, c.K, c.B) for c in graphed.last_counts]
    print(name, "sizes", sizes1, "loss", losses1[3:], losses2)
    assert sizes1 == sizes2 and losses1[3:] == losses2 and math.isfinite(losses2[-1])
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(_bits(p1), _bits(p2))
    if name == "bandit":
        s1.check_errors(); s2.check_errors()
        assert torch.equal(_bits(s1.exp3_weights), _bits(s2.exp3_weights))
        assert not torch.equal(s2.exp3_weights, torch.ones_like(s2.exp3_weights))
    graphed.close()
    if name.startswith("neighbor"):                                               # replay hygiene of the engine's own scratch
        eng = s2._engine
        words = -(-(-(-g2.num_nodes() // 32)) // 1024) * 1024
        assert int(eng._nr_scr[:16 + words].abs().sum()) == 0 and eng._nb_scr is None and eng._wn_scr is None
        for st in eng._sets.values():
            assert bool((st["kept_map"] == -1).all())


@pytest.mark.parametrize("name", NAMES)
def test_one_captured_step_serves_every_batch_size(cuda, graph_cpu, name):
    """GraphedTrainStep(batch_capacity=64) driven with 64, 37, 1 and 64 seeds against eager TrainStep calls on the same seeds: a
    column's draws depend on its node id, not on the batch, so the live prefix of the capacity-padded call is the exact-size call."""
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep
    ids = torch.arange(6000, dtype=torch.int32, device=cuda)
    perm = ids[torch.randperm(6000, generator=torch.Generator().manual_seed(9)).to(cuda)]
    batches, o = [], 0
    for n in LIVE:
        batches.append(perm[o:o + n].clone())
        o += n
    gA, sA, mA = _build(cuda, graph_cpu, name)
    step = GraphedTrainStep(gA, sA, mA, CAP, lr=0.01, ledger=True, batch_capacity=CAP)
    lA = BatchLoader(ids, CAP, seed=5).forever()
    step.calibrate(lA, steps=3)
    step.capture(lA, warmup=2)
    got = []
    for seeds in batches:
        loss = float(step(seeds))
        got.append((loss, step.sizes()))
    gB, sB, mB = _build(cuda, graph_cpu, name)
    eager = TrainStep(gB, sB, mB, lr=0.01)
    lB = BatchLoader(ids, CAP, seed=5).forever()
    for _ in range(3):
        sB.sample_blocks(gB, next(lB))
    for _ in range(3):
        eager(next(lB))
    for seeds, (loss, sizes) in zip(batches, got):
        want = float(eager(seeds))
        want_sizes = [dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in eager.last["mfgs"]]
        print(name, int(seeds.numel()), loss, want, sizes[0]["K"])
        assert sizes == want_sizes and sizes[-1]["S"] == int(seeds.numel())
        assert loss == want and math.isfinite(want)
    for p, q in zip(mA.parameters(), mB.parameters()):
        assert torch.equal(_bits(p), _bits(q))
    if name == "bandit":
        assert torch.equal(_bits(sA._w_pos), _bits(sB._w_pos))
    assert sA.draw_step() == sB.draw_step() == 10
    rec = step.ledger()
    assert rec["steps_total"] == 7 and rec["err"] == 0 and rec["nonfinite"] == 0
    step.close()


@pytest.mark.parametrize("name", NAMES)
def test_fit_graphed_runs_two_epochs(cuda, name):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = fit_task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    _with_prob(g)
    if name.startswith("neighbor"):
        sampler = fit.NeighborSampler([5, 5, 5], draw="device", replace=True, prob="p" if name == "neighbor-prob" else None)
        assert type(fit.make_sampler("neighbor", [5, 5, 5], draw="device", replace=True)) is fit.NeighborSampler
    else:
        sampler = fit.make_sampler(name, [64, 32, 16], draw="device", replace=True)
        assert sampler.draw == "device" and sampler.replace is True
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=128, lr=0.01, max_epochs=2, train_step="graphed")
    assert len(out["history"]) == 2 and out["steps"] == 2 * (1800 // 128)
    assert all(math.isfinite(h["train_loss"]) for h in out["history"])
    assert out["history"][-1]["train_loss"] < out["history"][0]["train_loss"]     # it learns
    assert sampler.draw_step() >= out["steps"]
    sampler.check_errors()


def test_gat_step_on_blocks_with_repeated_edges(cuda, graph_cpu):
    """A GATv2 (edge softmax, attention dropout off) on with-replacement neighbor blocks: the replayed step is the eager step."""
    from bliss_gnn_amd.model import GATv2
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep
    ids = torch.arange(6000, dtype=torch.int32, device=cuda)

    def build():
        g = _graph(graph_cpu, cuda)
        s = _sampler("neighbor")
        torch.manual_seed(0)
        model = GATv2(3, 32, 8, 4, [2, 2, 1], F.elu, 0.0, 0.0, 0.2, True).to(cuda).bfloat16()
        model.train()
        return g, s, model

    g1, s1, m1 = build()
    eager = TrainStep(g1, s1, m1)
    l1 = BatchLoader(ids, BS, seed=5).forever()
    g2, s2, m2 = build()
    graphed = GraphedTrainStep(g2, s2, m2, BS)
    l2 = BatchLoader(ids, BS, seed=5).forever()
    graphed.calibrate(l2, steps=2)
    graphed.capture(l2, warmup=1)
    losses2 = [float(graphed(next(l2))) for _ in range(3)]
    for _ in range(2):
        s1.sample_blocks(g1, next(l1))
    losses1 = [float(eager(next(l1))) for _ in range(5)]
    print("gat", losses1, losses2)
    assert losses1[2:] == losses2 and math.isfinite(losses2[-1])
    blk = eager.last["mfgs"][-1]                                                  # the seeds' block: columns of few edges repeat them
    pairs = torch.stack([blk.src.long(), blk.dst.long()], 1)
    assert torch.unique(pairs, dim=0).shape[0] < pairs.shape[0]
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(_bits(p1), _bits(p2))
    graphed.close()


def test_refusals(cuda, graph_cpu):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g = _graph(graph_cpu, cuda)
    seeds = torch.arange(BS, dtype=torch.int32, device=cuda)
    model = SAGE(32, 16, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    for name in NAMES:
        s = _sampler(name)
        with pytest.raises(NotImplementedError):                                  # draw == "device": the pipelined loop's refusal
            PipelinedTrainStep(g, s, model, BS)
        s.sample_blocks(g, seeds)
        for kw in (dict(external_rng=True), dict(chain_rng=True), dict(part="main", external_rng=True)):
            with pytest.raises(NotImplementedError):
                s.sample_blocks_static(g, seeds, **kw)
    with pytest.raises(NotImplementedError, match="device-replace"):
        bg.LadiesSampler(FAN, replace=True, draw="device")
    with pytest.raises(NotImplementedError):
        fit.NeighborSampler(NB_FAN, replace=True)
    with pytest.raises(ValueError, match="1024"):
        fit.NeighborSampler([2000, 4], draw="device", replace=True)
    with pytest.raises(NotImplementedError):
        fit.BanditNeighborSampler(NB_FAN, replace=True)
    with pytest.raises(NotImplementedError):
        fit.BanditLaborSampler(NB_FAN, replace=True)
    eng = _sampler("neighbor")._bind(g)
    with pytest.raises(NotImplementedError):                                      # EXP3-mode probabilities: the bandit's, out of scope
        eng.sample_blocks_neighbor(seeds, [4], bg._engine.DrawState(1, 0, cuda), nb_prob=eng.neighbor_prob(g.by_position(g.edata["w"]).contiguous(), eta=0.4),
                                   replace=True)
