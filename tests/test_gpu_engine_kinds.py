"""GPU suite (-m gpu): what the sampler engine returns per kind of layer (_engine.KINDS), byte for byte against arrays recorded
from the commit before the engine got its layer-kind table (tests/golden/engine_kinds.npz), and its capacity-regrow loop per family.

The golden file is written by this module's recorder, ``python tests/test_gpu_engine_kinds.py OUT.npz``: it uses the samplers'
public methods only, so it runs unchanged on the earlier commit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, FAN, FAN_ALL = 300, [3, 4], [3, -1]          # input-most first: sampled [4, 3] / [-1, 3]
SEEDS = [0, 1, 2, 3, 50, 120, 200, 299]
DRAW_SEED, STEP, TORCH_SEED = 11, 5, 123
NODE_WISE = ("neighbor", "wneighbor", "neighbor_replace", "labor", "labor_is", "wlabor")
KINDS = ("stream", "poisson_keyed", "multinomial_host", "multinomial", "multinomial_replace") + NODE_WISE
HOST_RNG = ("stream", "multinomial_host")       # these draw from torch's CPU generator
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_kinds.npz")


def graph_np():
    """300 nodes: node 0 has no in-edge, node 1 is a hub (40 in-edges, more than any fanout), node 2 has one in-edge (fewer than
    any fanout), node 3 has a pair of parallel edges; every other node v has 2 + v % 5 in-edges.  Edge ids run against positions."""
    cols = [[], [(7 * j + 4) % V for j in range(40)], [17], [10, 10, 11]]
    cols += [[(17 * v + 31 * j + 7) % V for j in range(2 + v % 5)] for v in range(4, V)]
    indptr = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
    indices = np.array([u for c in cols for u in c], dtype=np.int32)
    return indptr, indices, np.arange(len(indices) - 1, -1, -1, dtype=np.int32)


def _graph(dev):
    import bliss_gnn_amd as bg
    ip, ix, ei = graph_np()
    g = bg.Graph(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), torch.from_numpy(ei).to(dev))
    g.edata["w"] = bg.normalized_edata(g)
    return g


def _sampler(kind, fan):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    s = {"stream": lambda: bg.PoissonLadiesSampler(fan),
         "poisson_keyed": lambda: bg.PoissonBanditLadiesSampler(fan, draw="device"),
         "multinomial_host": lambda: bg.LadiesSampler(fan),
         "multinomial": lambda: bg.BanditLadiesSampler(fan, draw="device"),
         "multinomial_replace": lambda: bg.LadiesSampler(fan, draw="device-replace"),
         "neighbor": lambda: fit.NeighborSampler(fan, draw="device"),
         "wneighbor": lambda: fit.BanditNeighborSampler(fan),
         "neighbor_replace": lambda: fit.NeighborSampler(fan, draw="device", prob="w", replace=True),
         "labor": lambda: fit.LaborSampler(fan, layer_dependency=True),
         "labor_is": lambda: fit.ImportanceLaborSampler(fan, iterations=2),
         "wlabor": lambda: fit.WeightedLaborSampler(fan, prob="w")}[kind]()
    if kind not in HOST_RNG:
        s.reset_draw(DRAW_SEED, STEP)
    return s


def _start(kind, s):
    """The fixed seed of a call."""
    torch.manual_seed(TORCH_SEED)
    if kind not in HOST_RNG:
        s.reset_draw(DRAW_SEED, STEP)


def _arrays(blocks, cnts=None):
    """Per layer (input-most first): sizes, the block's arrays cut to them, bf16 outputs as bits."""
    import bliss_gnn_amd as bg
    out = {}
    for l, blk in enumerate(blocks):
        c = blk._counts if cnts is None else cnts[len(blocks) - 1 - l]
        S, K, B = c.S, c.K, c.B
        out["L%d/SKB" % l] = np.array([S, K, B], dtype=np.int64)
        for name, t, m in (("indptr", blk.indptr, S + 1), ("src", blk.src, B), ("dst", blk.dst, B), ("pos", blk.pos, B),
                           ("eid", blk.edata[bg.EID], B), ("kept_nid", blk.srcdata[bg.NID], K)):
            out["L%d/%s" % (l, name)] = t[:m].cpu().numpy()
        for name, t, m in (("edge_weights", blk._edge_weights, B), ("q", blk._q, B), ("node_prob", blk._node_prob, K),
                           ("p_ij", getattr(blk, "_p", None), B)):
            if t is not None:
                assert t.dtype == torch.bfloat16
                out["L%d/%s" % (l, name)] = t[:m].contiguous().view(torch.int16).cpu().numpy()
    return out


def _after(kind, s):
    """What the call left behind: torch's CPU generator state, or the draw step."""
    if kind in HOST_RNG:
        return torch.get_rng_state().numpy().copy()
    return np.array([s.draw_step()], dtype=np.int64)


def run_exact(kind, g, fan=FAN):
    s = _sampler(kind, fan)
    seeds = torch.tensor(SEEDS, dtype=torch.int32, device=g.device)
    _start(kind, s)
    _, _, blocks = s.sample_blocks(g, seeds)
    out = _arrays(blocks)
    out["after"] = _after(kind, s)
    return out, s, blocks


def run_static(kind, g):
    """sample_blocks_static + finish_static from the same seed, with capacities fixed from the exact call's sizes."""
    _, s, blocks = run_exact(kind, g)
    seeds = torch.tensor(SEEDS, dtype=torch.int32, device=g.device)
    mx = [dict(K=b.num_src_nodes(), B=b.num_edges(), E=b._counts.E) for b in reversed(blocks)]      # sampling order
    eng = s._engine
    eng.set_static_caps(len(SEEDS), list(reversed(FAN)), mx)
    _start(kind, s)
    if kind in HOST_RNG:
        eng.stage_rng_from_torch()
    _, _, blocks = s.sample_blocks_static(g, seeds)
    torch.cuda.current_stream().synchronize()
    cnts = s.finish_static()
    out = _arrays(blocks, cnts)
    out["after"] = _after(kind, s)
    return out


def record(dev):
    g, out = _graph(dev), {}
    for kind in KINDS:
        runs = {"exact": run_exact(kind, g)[0]}
        if kind != "multinomial_host":
            runs["static"] = run_static(kind, g)
        if kind in NODE_WISE:
            runs["all"] = run_exact(kind, g, FAN_ALL)[0]
        for call, arrays in runs.items():
            for name, a in arrays.items():
                out["%s/%s/%s" % (kind, call, name)] = a
    return out


# ------------------------------------------------------------------------------------------------- against the recorded arrays
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def graph(cuda):
    return _graph(cuda)


def _assert_recorded(golden, prefix, got):
    want = {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}
    assert want and sorted(want) == sorted(got), (prefix, sorted(want), sorted(got))
    for name in sorted(want):
        assert want[name].dtype == got[name].dtype and np.array_equal(want[name], got[name]), prefix + name


@pytest.mark.parametrize("kind", KINDS)
def test_exact_call_is_the_recorded_one(graph, golden, kind):
    _assert_recorded(golden, kind + "/exact/", run_exact(kind, graph)[0])


@pytest.mark.parametrize("kind", KINDS)
def test_static_call_is_the_recorded_one(graph, golden, kind):
    if kind == "multinomial_host":                  # torch.multinomial on the host syncs per layer: it has no static call
        s = _sampler(kind, FAN)
        with pytest.raises(NotImplementedError):
            s.sample_blocks_static(graph, torch.tensor(SEEDS, dtype=torch.int32, device=graph.device))
        return
    _assert_recorded(golden, kind + "/static/", run_static(kind, graph))


@pytest.mark.parametrize("kind", NODE_WISE)
def test_whole_columns_are_the_recorded_ones(graph, golden, kind):
    _assert_recorded(golden, kind + "/all/", run_exact(kind, graph, FAN_ALL)[0])


# ------------------------------------------------------------------------------------------------- the regrow loop
def _same(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("kind", ["stream", "poisson_keyed", "labor"])
def test_regrow_repeats_the_same_draw(graph, kind):
    """Capacities below the true sizes: the call is repeated with larger buffers, from the same generator snapshot, on the same
    draw step."""
    want, s, blocks = run_exact(kind, graph)
    eng = s._engine
    assert eng.retries == 0
    for n, blk in enumerate(reversed(blocks)):                                  # sampling order
        assert blk.num_src_nodes() > 1 and blk.num_edges() > 1
        eng.caps[n]["K"], eng.caps[n]["B"] = blk.num_src_nodes() - 1, blk.num_edges() - 1
    eng.ws = None
    _start(kind, s)
    _, _, again = s.sample_blocks(graph, torch.tensor(SEEDS, dtype=torch.int32, device=graph.device))
    assert eng.retries >= 1
    got = _arrays(again)
    got["after"] = _after(kind, s)                  # the draw step went up by exactly one / the generator state of the unshrunk run
    _same(want, got)
    if kind not in HOST_RNG:
        assert s.draw_step() == STEP + 1


@pytest.mark.parametrize("kind", ["neighbor", "multinomial"])
def test_exact_bounds_never_regrow(graph, kind):
    want, s, _ = run_exact(kind, graph)
    eng = s._engine
    assert (eng.exact_b if kind == "neighbor" else eng.exact_k) and eng.retries == 0
    _start(kind, s)
    _, _, again = s.sample_blocks(graph, torch.tensor(SEEDS, dtype=torch.int32, device=graph.device))
    got = _arrays(again)
    got["after"] = _after(kind, s)
    _same(want, got)
    assert eng.retries == 0 and s.draw_step() == STEP + 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    arrays = record(torch.device("cuda:0"))
    np.savez_compressed(sys.argv[1], **arrays)
    print("recorded", len(arrays), "arrays into", sys.argv[1])
