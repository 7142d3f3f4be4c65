"""GPU suite (-m gpu): the span-level decode of the frontier walks (csrc/sampler.hip: decode_span in k_bin_scatter and in
span_collect of k_block_pass1 / k_block_pass2; common.cuh: span_segments) at every shape where it takes another path, through the
public samplers over the hand-built graphs of tests/span_decode_ref.py (whose shapes tests/test_span_decode_ref.py pins on the
CPU), compared with the oracle by equality:

  * frontier lengths around an item (64), a span (256) and k_bin_scatter's batch (4096): partial items, waves whose later items
    lie past the frontier's end, a last wave that starts 64 positions before it;
  * 0, 62, 63, 64, 65 and 127 boundaries inside a span (the window of 64 covers up to 63), runs of 70 empty columns on a span's
    first position and inside a span, empty columns first / in the middle / last, a column ending on a span's end, S = 1,
    more than 1024 seeds;
  * the three term variants of k_bin_scatter (bandit, LADIES, importance_sampling=0), eager launches, the static path and three
    replays of a captured graph, a two-layer run whose second layer's seeds are a kept list;
  * k_bin_reduce with one bin of more than 8 x 1024 records beside bins of none, one and five."""
import pytest
import torch

import span_decode_ref as sd

pytestmark = pytest.mark.gpu


def _bg():
    import bliss_gnn_amd as bg
    return bg


def _bits(t):
    t = t.detach().cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _graph(case, dev):
    bg = _bg()
    og = case.og
    g = bg.Graph(og.indptr.to(dev), og.indices.to(dev), og.eid.to(dev))
    g.edata["w"] = bg.normalized_edata(g)
    return g


def _sampler(kind, fanouts):
    bg = _bg()
    if kind == "ladies":
        return bg.PoissonLadiesSampler(fanouts)
    return bg.PoissonBanditLadiesSampler(fanouts, eta=sd.ETA, importance_sampling=1 if kind == "bandit" else 0)


def _check_block(b, ob, kind, what):
    bg = _bg()
    c = b._counts
    assert c.err == 0, what
    assert (c.S, c.E, c.C, c.K, c.B) == (ob.n_dst, ob.trace["E"], ob.trace["cand_nid"].numel(), ob.n_src, ob.src.numel()), what
    assert c.c == ob.trace["c"], what
    assert torch.equal(b._trace["cand_nid"].cpu().long(), ob.trace["cand_nid"]), what
    assert ob.trace["p"].dtype == torch.bfloat16 and torch.equal(_bits(b._trace["p"]), _bits(ob.trace["p"])), what
    assert torch.equal(b.src.cpu().long(), ob.src) and torch.equal(b.dst.cpu().long(), ob.dst), what
    assert torch.equal(b.indptr.cpu().long(), ob.indptr) and torch.equal(b.edata[bg.EID].cpu().long(), ob.eid), what
    assert torch.equal(b.srcdata[bg.NID].cpu().long(), ob.src_nid), what
    assert torch.equal(_bits(b.edata["edge_weights"]), _bits(ob.edge_weights)), what
    if kind != "ladies":
        assert torch.equal(_bits(b.edata["q_ij"]), _bits(ob.q_ij)), what
        assert torch.equal(_bits(b.srcdata["node_prob"]), _bits(ob.node_prob)), what


def _sample_and_check(key, kind, dev, g=None):
    case = sd.case_of(key)
    g = g or _graph(case, dev)
    s = _sampler(kind, case.fanouts)
    torch.manual_seed(9)
    inp, _, blocks = s.sample_blocks(g, case.seeds.to(dev))
    s.check_errors()
    o_inp, o_blocks = sd.oracle_blocks(key, kind)
    assert torch.equal(inp.cpu().long(), o_inp)
    assert len(blocks) == len(o_blocks)
    for l, (b, ob) in enumerate(zip(blocks, o_blocks)):
        _check_block(b, ob, kind, "%s %s block %d" % (key, kind, l))
    return g, s, blocks


@pytest.mark.parametrize("E", sd.FRONTIER_LENGTHS)
def test_frontier_lengths(cuda, E):
    """Every span of these frontiers takes the span-level path (pinned on the CPU), the last one with lanes -- and for most
    lengths whole items -- past the frontier's end: what those lanes loaded for the last real edge must leave no trace."""
    g = None
    for kind in sd.KINDS:
        g, _, _ = _sample_and_check(E, kind, cuda, g)


@pytest.mark.parametrize("kind", sd.KINDS)
def test_boundary_structures(cuda, kind):
    """One frontier with spans on both sides of the window of 64 boundaries, spans deep inside a 33 000-edge column, runs of
    empty columns and more than 1024 seeds (tests/span_decode_ref.py: _structure_degrees)."""
    _, s, _ = _sample_and_check("structures", kind, cuda)
    assert s._engine.n_bins > 0                                          # the binned route: k_bin_scatter ran


def test_single_seed(cuda):
    g = None
    for kind in sd.KINDS:
        g, _, _ = _sample_and_check("single_seed", kind, cuda, g)


def test_two_layers(cuda):
    """[f, f]: span_collect of the second-sampled layer walks the columns of the first one's kept list."""
    _sample_and_check("two_layers", "bandit", cuda)


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_bin_reduce_bin_sizes(cuda, kind):
    """One source in the columns of more than 8 x 1024 seeds: its bin holds more records than a workgroup of k_bin_reduce reads
    in eight trips, the neighbouring bins none, one and five (pinned on the CPU for every bin count from 8 up)."""
    _, s, _ = _sample_and_check("reduce", kind, cuda)
    assert s._engine.n_bins >= 8


def _snapshot(s, blocks, cnts):
    bg = _bg()
    out = []
    for b, c in zip(reversed(blocks), cnts):                              # sampling order
        assert c.err == 0
        out.append(dict(sizes=(c.S, c.E, c.C, c.K, c.B), src=b.src[:c.B].clone(), dst=b.dst[:c.B].clone(),
                        nid=b.srcdata[bg.NID][:c.K].clone(), ew=_bits(b._edge_weights[:c.B]).clone(), q=_bits(b._q[:c.B]).clone(),
                        prob=_bits(b._node_prob[:c.K]).clone()))
    return out


def test_static_path_and_graph_replays(cuda):
    """The two-layer run through the static path and three times from one captured graph: every run leaves the eager call's
    blocks, which equal the oracle's."""
    bg = _bg()
    g, s, eager = _sample_and_check("two_layers", "bandit", cuda)
    seeds = sd.case_of("two_layers").seeds.to(cuda)
    eng = s._engine

    def static_once(launch):
        torch.manual_seed(9)
        eng.stage_rng_from_torch()
        blocks = launch()
        torch.cuda.synchronize()
        return _snapshot(s, blocks, s.finish_static())

    def same_as_eager(run, what):
        for n, (r, be) in enumerate(zip(run, reversed(eager))):
            c = be._counts
            assert r["sizes"] == (c.S, c.E, c.C, c.K, c.B), what
            assert torch.equal(r["src"], be.src) and torch.equal(r["dst"], be.dst) and torch.equal(r["nid"], be.srcdata[bg.NID]), what
            assert torch.equal(r["ew"], _bits(be.edata["edge_weights"])) and torch.equal(r["q"], _bits(be.edata["q_ij"])), what
            assert torch.equal(r["prob"], _bits(be.srcdata["node_prob"])), what

    same_as_eager(static_once(lambda: s.sample_blocks_static(g, seeds)[2]), "static")
    torch.manual_seed(9)
    eng.stage_rng_from_torch()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = s.sample_blocks_static(g, seeds)[2]

    def replay():
        graph.replay()
        return captured
    for i in range(3):
        same_as_eager(static_once(replay), "replay %d" % i)
