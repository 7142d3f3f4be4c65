"""GPU suite (-m gpu): a block that a capacity clamped is still a well-formed block (include/bliss_gnn.h "clamped blocks", DESIGN.md
section 35).  A static-shape step learns of an overflow only after its consumers have walked the block, so what a clamped layer leaves
behind must keep every consumer inside its buffers.

The harness is tests/test_gpu_engine_kinds.py's: its 300-node graph (a hub, a one-edge column, a parallel pair), its 8 seeds, fanouts
[3, 4], its samplers.  Per kind (every kind with a static call): the true sizes from one exact call, then static calls with ONE
capacity of ONE layer below the truth (written into ``eng.caps`` after set_static_caps, the only way to shrink an exact bound) and
everything else roomy.  Per call: finish_static raises, the shrunk layer's error word is exactly its BLISS_ERR_CAP_* bit, every
layer's arrays -- read at capacity length -- pass tests/block_invariants.py (I1 - I7), the engine's maps and scratch are as a replay
needs them (I8), a second clamped call gives the same bytes, and with the capacities put back the same engine's next static call is
the one recorded in tests/golden/engine_kinds.npz.  Integer and bit equalities only.

Later layers.  A clamp in the first-sampled layer changes the second layer's seeds (fewer, or -- K clamped -- a prefix): the second
layer is then an unclamped layer of other seeds, must carry no error bit under the roomy capacities, and is checked like any other.

The consumer tests at the end run a forward and a backward on two such blocks; they check the block first and come after the sampler
tests in this file on purpose."""
import copy

import numpy as np
import pytest
import torch

import block_invariants as bi
from test_gpu_engine_kinds import (FAN, HOST_RNG, KINDS, NODE_WISE, SEEDS, STEP, _after, _arrays, _assert_recorded, _sampler, _start,
                                   golden, graph, graph_np, run_exact)  # noqa: F401  (golden, graph: fixtures)

pytestmark = pytest.mark.gpu

STATIC_KINDS = tuple(k for k in KINDS if k != "multinomial_host")
LAYER_FAMILY = tuple(k for k in STATIC_KINDS if k not in NODE_WISE)
POISSON = ("stream", "poisson_keyed")
BIT = dict(C=2, K=4, B=8, S=64)                                    # BLISS_ERR_CAP_CAND / _KEPT / _EDGES / _SEEDS
# (capacity, which value below the truth); "S" is the second layer's only: its seed count is read on the device
SHRINKS = (("K", "true-1"), ("K", "S"), ("B", "true-1"), ("B", "1"), ("C", "true-1"), ("S", "K0-1"))


def _cases():
    out = []
    for kind in STATIC_KINDS:
        for layer in (0, 1):
            for cap, to in SHRINKS:
                if (cap == "C" and kind in NODE_WISE) or (cap == "S" and layer == 0):
                    continue
                out.append(pytest.param(kind, layer, cap, to, id="%s-L%d-%s=%s" % (kind, layer, cap, to)))
    return out


class _Rig:
    """One kind: its sampler and engine, the true sizes, the roomy static capacities."""

    def __init__(self, kind, g):
        self.kind, self.g = kind, g
        _, self.s, blocks = run_exact(kind, g)
        self.true = [dict(S=b._counts.S, K=b._counts.K, B=b._counts.B, C=b._counts.C, E=b._counts.E) for b in reversed(blocks)]
        self.eng = self.s._engine
        self.seeds = torch.tensor(SEEDS, dtype=torch.int32, device=g.device)
        self.eng.set_static_caps(len(SEEDS), list(reversed(FAN)), [dict(K=t["K"], B=t["B"], E=t["E"]) for t in self.true])
        self.roomy = copy.deepcopy(self.eng.caps)
        for t, c in zip(self.true, self.roomy):                    # the truth fits, and can be undercut
            assert t["S"] <= c["S"] and t["K"] <= c["K"] and t["B"] <= c["B"] and t["C"] <= c["C"]
            assert t["K"] > t["S"] > 1 and t["B"] > 1 and t["C"] > t["S"], t

    def static(self, caps):
        """One static call under ``caps`` from the fixed seed: (blocks in sampling order, counts, the RuntimeError or None)."""
        eng = self.eng
        eng.caps = copy.deepcopy(caps)
        _start(self.kind, self.s)
        if self.kind in HOST_RNG:
            eng.stage_rng_from_torch()
        _, _, published = self.s.sample_blocks_static(self.g, self.seeds)
        torch.cuda.current_stream().synchronize()
        raised = None
        try:
            self.s.finish_static()
        except RuntimeError as e:
            raised = e
        blocks = eng._static[0][0]
        return blocks, [b._counts for b in blocks], raised, published

    def persistent(self):
        """What outlives a call on the engine, as numpy: name -> array."""
        eng, out = self.eng, {}
        for i, st in eng._sets.items():
            out["set%d/kept_map" % i], out["set%d/local_id" % i] = st["kept_map"], st["local_id"]
        out["first_pos"], out["acc_p2"], out["fs_ticket"] = eng.first_pos, eng.acc_p2, eng.fs_ticket
        if self.kind in POISSON:                                    # the Poisson scale reads the histogram and leaves it zero; the
            out["hist"] = eng.hist                                  # multinomial kinds never read it (it only counts up there)
        # (the multinomial draws' scratch holds per-call prefixes beside its tickets: "ready for the next call", which the recorded
        #  call on the same engine shows, is not "equal words")
        words = -(-(-(-eng.V // 32)) // 1024) * 1024                # node bitmap: whole tiles of 1024 words
        for attr in ("_nb_scr", "_wn_scr", "_nr_scr", "_lb_scr", "_li_scr", "_wl_scr"):
            scr = getattr(eng, attr)
            if scr is not None:
                out[attr + "/tickets+bitmap"] = (scr[-1] if isinstance(scr, tuple) else scr)[:16 + words]
        return {k: v.cpu().numpy().copy() for k, v in out.items()}


_RIGS = {}


def _rig(kind, g):
    if kind not in _RIGS:
        _RIGS[kind] = _Rig(kind, g)
    return _RIGS[kind]


def _bits(t):
    return None if t is None else t.contiguous().view(torch.int16).cpu().numpy().copy()


def layer_arrays(blk, c):
    """One layer's arrays at capacity length, under block_invariants' names."""
    import bliss_gnn_amd as bg
    i = lambda t: t.cpu().numpy().copy()
    t_indptr, t_edge = blk._transposed
    return dict(S=c.S, K=c.K, B=c.B, C=c.C, err=c.err, indptr=i(blk.indptr), src=i(blk.src), dst=i(blk.dst), pos=i(blk.pos),
                eid=i(blk.edata[bg.EID]), kept_nid=i(blk.srcdata[bg.NID]), t_indptr=i(t_indptr), t_edge=i(t_edge),
                edge_weights=_bits(blk._edge_weights), q=_bits(blk._q), node_prob=_bits(blk._node_prob), p_ij=_bits(getattr(blk, "_p", None)))


def defined_part(a, cap):
    """The entries of a layer's arrays that the contract defines (what lies past B is nobody's)."""
    out = {"counts": np.array([a[k] for k in ("S", "K", "B", "C", "err")]), "indptr": a["indptr"][:cap["S"] + 1],
           "kept_nid": a["kept_nid"][:cap["K"]], "t_indptr": a["t_indptr"][:cap["K"] + 1], "node_prob": a["node_prob"][:cap["K"]]}
    for name in ("src", "dst", "pos", "eid", "t_edge", "edge_weights", "q", "p_ij"):
        if a[name] is not None:
            out[name] = a[name][:a["B"]]
    return out


def shrunk_caps(rig, layer, cap, to):
    caps, t = copy.deepcopy(rig.roomy), rig.true[layer]
    value = {"true-1": t[cap] - 1, "S": t["S"], "1": 1, "K0-1": rig.true[0]["K"] - 1}[to]
    assert value < t[cap]                                           # below the truth: the layer overflows it
    caps[layer][cap] = value
    return caps


def check_call(rig, caps, layer, cap):
    """finish_static raised, the error words, I1 - I7 on every layer, I8; returns the layers' arrays (sampling order)."""
    blocks, cnts, raised, _ = rig.static(caps)
    assert raised is not None and "the step's results are invalid" in str(raised), raised
    errs = [c.err for c in cnts]
    assert errs[layer] == BIT[cap], (errs, cap)
    assert all(e == 0 for n, e in enumerate(errs) if n != layer), errs       # (later layers: other seeds, roomy capacities)
    layers, seeds = [], np.array(SEEDS)
    for n, (blk, c) in enumerate(zip(blocks, cnts)):
        a = layer_arrays(blk, c)
        try:
            bi.check(a, caps[n], graph_np(), seeds, cap if n == layer else "")
        except bi.Violation as e:
            raise AssertionError("sampling layer %d: %s" % (n, e)) from e
        layers.append(a)
        seeds = a["kept_nid"][:a["K"]]
    # I8: what a replay relies on
    left = rig.persistent()
    for name, v in left.items():
        if name.endswith("kept_map") or name.endswith("local_id"):
            assert (v == -1).all(), name + " is not clean"
        if name.endswith("tickets+bitmap") or name == "fs_ticket" or name == "hist":
            assert not v.any(), name + " is not zero"
    for name, v in rig.clean.items():
        assert np.array_equal(v, left[name]), name + " is not as the unclamped call leaves it"
    if rig.kind not in HOST_RNG:
        assert rig.s.draw_step() == STEP + 1                        # bumped exactly once
    return layers, [c.C for c in cnts]


@pytest.mark.parametrize("kind,layer,cap,to", _cases())
def test_a_clamped_layer_leaves_a_walkable_block(graph, golden, kind, layer, cap, to):
    rig = _rig(kind, graph)
    if not hasattr(rig, "clean"):                                   # the unclamped static call, once: it is the recorded one
        blocks, cnts, raised, published = rig.static(rig.roomy)
        assert raised is None
        got = _arrays(published, cnts)
        got["after"] = _after(kind, rig.s)
        _assert_recorded(golden, kind + "/static/", got)
        rig.clean = rig.persistent()
    caps = shrunk_caps(rig, layer, cap, to)
    first, drawn = check_call(rig, caps, layer, cap)
    after = _after(kind, rig.s)
    second, _ = check_call(rig, caps, layer, cap)                   # the same seed again: the same bytes
    for n, (a, b) in enumerate(zip(first, second)):
        da, db = defined_part(a, caps[n]), defined_part(b, caps[n])
        assert sorted(da) == sorted(db)
        for name in da:
            assert np.array_equal(da[name], db[name]), "sampling layer %d: %s differs between two clamped calls" % (n, name)
    # the draw step bumped once / the generator state of the unclamped run: what the recorded static call left.  (The MT stream
    # hands out one number per candidate: where the clamp changed a layer's candidates -- its own C, or the next layer's seeds --
    # the state is the one after THAT many numbers, which the second call must reproduce.)
    assert np.array_equal(_after(kind, rig.s), after)
    if kind not in HOST_RNG or drawn == [t["C"] for t in rig.true]:
        assert np.array_equal(after, golden[kind + "/static/after"])
    # the capacities put back, the same engine: the recorded call, byte for byte
    blocks, cnts, raised, published = rig.static(rig.roomy)
    assert raised is None
    got = _arrays(published, cnts)
    got["after"] = _after(kind, rig.s)
    _assert_recorded(golden, kind + "/static/", got)


# ------------------------------------------------------------------------------------------------- consumers on a clamped block
# The padded-block contract (tests/test_gpu_grad_edges.py::test_capacity_padded_blocks and its kin) on blocks that a real overflow
# produced: the capacity-sized block of the clamped layer, feature rows >= K and gradient rows >= S NaN, against the exact-size
# block cut from the same arrays at (S, K, B).  Bit equality.  block_invariants.check runs first: a block that is not walkable
# stops the test before any consumer is launched.
CONSUMER_BLOCKS = (("labor", 0, "K", "true-1"), ("poisson_keyed", 1, "B", "true-1"))
WIDTHS = (8, 7)                                                     # vec4-aligned rows, and rows off that alignment


@pytest.fixture(scope="module", params=CONSUMER_BLOCKS, ids=["%s-L%d-%s=%s" % c for c in CONSUMER_BLOCKS])
def clamped(request, graph):
    import bounds
    kind, layer, cap, to = request.param
    rig = _rig(kind, graph)
    caps = shrunk_caps(rig, layer, cap, to)
    blocks, cnts, raised, _ = rig.static(caps)
    assert raised is not None and cnts[layer].err == BIT[cap]
    arrays = [layer_arrays(b, c) for b, c in zip(blocks, cnts)]
    seeds = np.array(SEEDS) if layer == 0 else arrays[layer - 1]["kept_nid"][:arrays[layer - 1]["K"]]
    a = arrays[layer]
    bi.check(a, caps[layer], graph_np(), seeds, cap)                # before any consumer launch
    S, K, B = a["S"], a["K"], a["B"]
    assert S >= 1 and K >= S and B >= 1
    if cap == "K":                                                  # the clamp's own edges are there: a dropped source's, at source 0
        named = a["kept_nid"][a["src"][:B]]
        assert (named != graph_np()[1][a["pos"][:B]]).any()
    t = lambda x: torch.from_numpy(np.asarray(x)).long()
    exact = bounds.to_block(bounds.Spec(K, S, t(a["indptr"][:S + 1]), t(a["src"][:B]), t(a["dst"][:B])), graph.device)
    pad = blocks[layer]
    assert pad._nnz_ptr and (pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()) == tuple(caps[layer][k] for k in "SKB")
    w = pad._edge_weights.clone()
    w[B:] = float("nan")
    return pad, exact, (S, K, B), w


def _rows(n, live, dim, seed, dev):
    x = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed)).bfloat16()
    x[live:] = float("nan")
    return x.to(dev)


def _same_bits(got, want, what):
    assert got.shape == want.shape and torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), what


def _aggregate_both(clamped, dim, op):
    """``op(block, h, w)`` forward and backward on the clamped and on the exact-size block: out and d h of the live rows."""
    pad, exact, (S, K, B), w = clamped
    dev = w.device
    rows = max(pad.num_src_nodes(), pad.num_dst_nodes())            # (a K clamp may leave fewer source slots than destination slots)
    h, g = _rows(rows, K, dim, 5, dev), _rows(pad.num_dst_nodes(), S, dim, 6, dev)
    got = {}
    for name, blk, k_rows, s_rows, n_e in (("clamped", pad, rows, pad.num_dst_nodes(), pad.num_edges()), ("exact", exact, K, S, B)):
        hi = h[:k_rows].clone().requires_grad_(True)
        out = op(blk, hi, w[:n_e].contiguous())
        out.backward(g[:s_rows].contiguous())
        got[name] = (out.detach()[:S], hi.grad[:K])
    torch.cuda.synchronize()
    _same_bits(got["clamped"][0], got["exact"][0], "out")
    _same_bits(got["clamped"][1], got["exact"][1], "d h")


@pytest.mark.parametrize("dim", WIDTHS)
def test_spmm_mean_on_a_clamped_block(clamped, dim):
    from bliss_gnn_amd.nn import weighted_aggregate
    _aggregate_both(clamped, dim, lambda blk, h, w: weighted_aggregate(blk, h, w, mean=True))


@pytest.mark.parametrize("dim", WIDTHS)
def test_spmm_max_on_a_clamped_block(clamped, dim):
    from bliss_gnn_amd.nn import max_aggregate
    _aggregate_both(clamped, dim, lambda blk, h, w: max_aggregate(blk, h, w))


@pytest.mark.parametrize("dim", WIDTHS)
def test_gcn_aggregate_on_a_clamped_block(clamped, dim):
    from bliss_gnn_amd.nn import gcn_aggregate
    _aggregate_both(clamped, dim, lambda blk, h, w: gcn_aggregate(blk, h, w))


@pytest.mark.parametrize("dim", WIDTHS)
def test_graphconv_tile_on_a_clamped_block(clamped, dim):
    """out, d feat and db of the live rows (dW's summation plan follows the row bound: the padded-block contract of
    tests/test_gpu_gcn_layer.py holds it to its error bound, not to bits, and so it is not compared here)."""
    from bliss_gnn_amd.nn import GraphConv
    pad, exact, (S, K, B), w = clamped
    dev = w.device
    torch.manual_seed(2)
    layer = GraphConv(dim, dim, activation=torch.relu, allow_zero_in_degree=True, transforms="tile").to(dev).bfloat16()
    assert layer.tile_refusal() is None
    rows = max(pad.num_src_nodes(), pad.num_dst_nodes())
    h, g = _rows(rows, K, dim, 7, dev), _rows(pad.num_dst_nodes(), S, dim, 8, dev)
    got = {}
    for name, blk, k_rows, s_rows, n_e in (("clamped", pad, pad.num_src_nodes(), pad.num_dst_nodes(), pad.num_edges()),
                                           ("exact", exact, K, S, B)):
        layer.zero_grad(set_to_none=True)
        hi = h[:k_rows].clone().requires_grad_(True)
        out = layer(blk, hi, edge_weight=w[:n_e].contiguous())
        out.backward(g[:s_rows].contiguous())
        got[name] = (out.detach()[:S], hi.grad[:K], layer.bias.grad.clone())
    torch.cuda.synchronize()
    for i, what in enumerate(("out", "d feat", "d bias")):
        _same_bits(got["clamped"][i], got["exact"][i], what)


def test_fused_gatv2_on_a_clamped_block(clamped):
    from test_gpu_grad_edges import run_fused
    pad, exact, (S, K, B), w = clamped
    dev = w.device
    H, D = 2, 8
    rows = max(pad.num_src_nodes(), pad.num_dst_nodes())
    feat, g = _rows(rows, K, H * D, 9, dev) * 0.5, _rows(pad.num_dst_nodes(), S, H * D, 10, dev)
    attn = (torch.randn(1, H, D, generator=torch.Generator().manual_seed(11)) * 0.25).bfloat16().to(dev)
    q, u = run_fused(pad, feat, attn, g, H, D), run_fused(exact, feat[:K].contiguous(), attn, g[:S].contiguous(), H, D)
    torch.cuda.synchronize()
    _same_bits(q["rst"][:S], u["rst"], "rst")
    _same_bits(q["e"][:B], u["e"], "e")
    _same_bits(q["d_feat"][:K], u["d_feat"], "d feat")
    _same_bits(q["d_attn"], u["d_attn"], "d attn")
