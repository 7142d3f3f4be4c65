"""CPU suite: tests/block_invariants.py pinned before it judges a kernel (tests/test_gpu_clamped_blocks.py) -- it accepts the blocks
of the oracle's samplers and of the CPU restatements of the node-wise samplers on the 300-node graph of the engine-kind tests,
exact-size and capacity-padded, and rejects every planted single-entry fault under the invariant that fault breaks."""
import numpy as np
import pytest
import torch

import block_invariants as bi
import labor_ref
import neighbor_ref
import replace_ref
from block_build_ref import expected_index
from oracle import bliss_oracle as bo
from test_gpu_engine_kinds import DRAW_SEED, FAN, SEEDS, STEP, graph_np

SAMPLING_FAN = list(reversed(FAN))
PAD = dict(S=3, K=5, B=7)


def _from_ref(lay):
    """A layer dict of neighbor_ref / labor_ref / replace_ref.sample_layer: already the checker's names."""
    a = {k: lay[k] for k in ("S", "K", "B", "indptr", "src", "dst", "pos", "eid", "kept_nid", "t_indptr", "t_edge")}
    a["edge_weights"] = np.asarray(lay.get("weights", np.ones(lay["B"], dtype=np.float32)))
    a["q"] = np.asarray(lay.get("q_ij", np.full(lay["B"], 0x3F80, dtype=np.uint16)))
    a["node_prob"] = np.full(lay["K"], 0x3F80, dtype=np.uint16)
    return a, np.asarray(lay["kept_nid"][:lay["S"]])


def _from_oracle(ob, g_eid):
    """An OBlock; the CSC position of an edge is where its (unique) edge id sits in the graph."""
    where = np.empty(len(g_eid), dtype=np.int64)
    where[g_eid] = np.arange(len(g_eid))
    t_indptr, t_edge = expected_index(ob.src, ob.n_src)
    bits = lambda t: t.contiguous().view(torch.int16).numpy()
    a = dict(S=ob.n_dst, K=ob.n_src, B=int(ob.src.numel()), indptr=ob.indptr.numpy(), src=ob.src.numpy(), dst=ob.dst.numpy(),
             pos=where[ob.eid.numpy()], eid=ob.eid.numpy(), kept_nid=ob.src_nid.numpy(), t_indptr=t_indptr.numpy(),
             t_edge=t_edge.numpy(), edge_weights=bits(ob.edge_weights))
    if ob.q_ij is not None:
        a["q"], a["node_prob"] = bits(ob.q_ij), bits(ob.node_prob)
    return a, ob.dst_nid.numpy()


def _blocks():
    """name -> [(arrays, seeds)] in sampling order."""
    ip, ix, ei = graph_np()
    seeds = np.array(SEEDS)
    out = {"neighbor": neighbor_ref.sample_blocks(ip, ix, ei, seeds, SAMPLING_FAN, DRAW_SEED, STEP),
           "labor": labor_ref.sample_blocks(ip, ix, ei, seeds, SAMPLING_FAN, DRAW_SEED, STEP),
           "neighbor_replace": replace_ref.sample_blocks(ip, ix, ei, seeds, SAMPLING_FAN, DRAW_SEED, STEP)}
    out = {k: [_from_ref(lay) for lay in v] for k, v in out.items()}
    og = bo.CSC(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(ei))
    ones = torch.ones(len(FAN), og.num_edges, dtype=torch.bfloat16)
    t_seeds = torch.tensor(SEEDS, dtype=torch.int32)
    for name, poisson in (("poisson", True), ("multinomial", False)):
        torch.manual_seed(123)
        _, _, blocks = bo.sample_blocks_bandit(og, t_seeds, FAN, ones, 0.1, poisson=poisson)
        out["bandit_" + name] = [_from_oracle(ob, ei) for ob in reversed(blocks)]
        torch.manual_seed(123)
        _, _, blocks = bo.sample_blocks_ladies(og, t_seeds, FAN, bo.normalized_edata(og), poisson=poisson)
        out["ladies_" + name] = [_from_oracle(ob, ei) for ob in reversed(blocks)]
    return out


BLOCKS = _blocks()


def _exact_caps(a):
    return dict(S=a["S"], K=a["K"], B=a["B"])


def padded(a, pad=PAD):
    """The same block in capacity-sized arrays, padded as the kernels pad: empty rows, kept_nid 0, every list past K empty; what
    lies past B is nobody's (here -7, NaN for the floats)."""
    caps = dict(S=a["S"] + pad["S"], K=a["K"] + pad["K"], B=a["B"] + pad["B"])
    out = dict(a)
    fill = lambda x, n, v: np.concatenate([np.asarray(x), np.full(n, v, dtype=np.asarray(x).dtype)])
    out["indptr"] = fill(a["indptr"], pad["S"], a["B"])
    out["t_indptr"] = fill(a["t_indptr"], pad["K"], a["B"])
    out["kept_nid"] = fill(a["kept_nid"], pad["K"], 0)
    for name in ("src", "dst", "pos", "eid", "t_edge"):
        out[name] = fill(a[name], pad["B"], -7)
    for name, n in (("edge_weights", "B"), ("q", "B"), ("node_prob", "K")):
        if name in a:
            x = np.asarray(a[name])
            out[name] = fill(x, pad[n], 0x3F80 if x.dtype.kind in "iu" else 1.0)
    return out, caps


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_the_checker_accepts_the_reference_blocks(name):
    graph = graph_np()
    for n, (a, seeds) in enumerate(BLOCKS[name]):
        assert a["B"] > 0 and a["K"] > a["S"], (name, n)
        bi.check(a, _exact_caps(a), graph, seeds)
        p, caps = padded(a)
        bi.check(p, caps, graph, seeds)
        bi.check(dict(p, err=0), caps, graph, seeds)
        bi.check(p, caps, graph, None)


def test_bf16_bits_and_floats_are_both_read():
    assert bi.nonfinite(np.array([0x3F80, 0x7F80, 0xFF80, 0x7FC0, 0x0000, 0x7F7F], dtype=np.uint16)).tolist() == \
        [False, True, True, True, False, False]
    assert bi.nonfinite(np.array([0x7FC0], dtype=np.uint16).view(np.int16)).tolist() == [True]
    assert bi.nonfinite(np.array([1.0, np.inf, np.nan, -np.inf], dtype=np.float32)).tolist() == [False, True, True, True]


# ------------------------------------------------------------------------------------------------- planted faults
def _victim():
    """The second-sampled neighbor layer, capacity-padded: rows, sources and lists enough for every fault below."""
    a, seeds = BLOCKS["neighbor"][1]
    p, caps = padded(a)
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()}, caps, seeds


def _long_list(a):
    """A source with at least two edges: (list start, list end)."""
    d = np.diff(a["t_indptr"][:a["K"] + 1])
    j = int(np.flatnonzero(d >= 2)[0])
    return int(a["t_indptr"][j]), int(a["t_indptr"][j + 1])


def _src_minus_one(a, caps):
    a["src"][5] = -1
    return 5


def _src_equal_k(a, caps):
    a["src"][a["B"] - 1] = a["K"]
    return a["B"] - 1


def _dst_off_by_a_row(a, caps):
    a["dst"][7] += 1
    return 7


def _indptr_dips(a, caps):
    r = int(np.flatnonzero(np.diff(a["indptr"][:a["S"]]) > 0)[2]) + 1      # a row start above the one before it ...
    a["indptr"][r] = a["indptr"][r - 1] - 1                                  # ... now one below it
    return r - 1


def _indptr_s_is_not_b(a, caps):
    assert a["indptr"][a["S"] - 1] < a["B"]                                  # the last row holds an edge: still non-decreasing
    a["indptr"][a["S"]] = a["B"] - 1
    return a["S"]


def _padding_row_left_at_zero(a, caps):
    a["indptr"][caps["S"]] = 0
    return caps["S"] - 1


def _repeated_kept_nid(a, caps):
    a["kept_nid"][a["K"] - 1] = a["kept_nid"][2]
    return a["K"] - 1


def _t_edge_one_index_twice(a, caps):
    a["t_edge"][4] = a["t_edge"][9]
    return None


def _list_out_of_order(a, caps):
    beg, _ = _long_list(a)
    a["t_edge"][beg], a["t_edge"][beg + 1] = a["t_edge"][beg + 1], a["t_edge"][beg]
    return beg


def _t_indptr_end_is_not_b(a, caps):
    a["t_indptr"][caps["K"]] = a["B"] + 1
    return caps["K"] - a["K"]


def _one_nan_weight(a, caps):
    a["edge_weights"] = np.array(a["edge_weights"], dtype=np.float32)
    a["edge_weights"][3] = np.nan
    return 3


FAULTS = [(_src_minus_one, "I3"), (_src_equal_k, "I3"), (_dst_off_by_a_row, "I3"), (_indptr_dips, "I2"), (_indptr_s_is_not_b, "I2"),
          (_padding_row_left_at_zero, "I2"), (_repeated_kept_nid, "I4"), (_t_edge_one_index_twice, "I6"), (_list_out_of_order, "I6"),
          (_t_indptr_end_is_not_b, "I6"), (_one_nan_weight, "I7")]


@pytest.mark.parametrize("plant,invariant", FAULTS, ids=[f.__name__[1:] for f, _ in FAULTS])
def test_a_planted_fault_is_rejected_under_its_invariant(plant, invariant):
    a, caps, seeds = _victim()
    bi.check(a, caps, graph_np(), seeds)                      # sound before the fault
    at = plant(a, caps)
    with pytest.raises(bi.Violation) as e:
        bi.check(a, caps, graph_np(), seeds)
    assert e.value.invariant == invariant and str(e.value).startswith(invariant + ": "), str(e.value)
    if at is not None:
        assert "index %d" % at in str(e.value) or "[S = %d]" % at in str(e.value), (at, str(e.value))


def test_what_a_clamp_changes():
    """I1's error word and clamped counts, I4's seed prefix, I5's licence for edges whose source a K clamp dropped."""
    graph = graph_np()
    a, caps, seeds = _victim()
    for err, clamped, ok in ((0, "", True), (4, "", False), (0, "K", False), (16, "", True)):
        if ok:
            bi.check(dict(a, err=err), caps, graph, seeds, clamped)
            continue
        with pytest.raises(bi.Violation) as e:
            bi.check(dict(a, err=err), caps, graph, seeds, clamped)
        assert e.value.invariant == "I1"
    wrong = np.array(seeds)
    wrong[1] = seeds[0]
    with pytest.raises(bi.Violation) as e:
        bi.check(a, caps, graph, wrong)
    assert e.value.invariant == "I4" and "index 1" in str(e.value)
    # an edge pointed at source 0 in place of its own: inconsistent, allowed only where K was clamped and its source is not kept
    e0 = int(np.flatnonzero(a["src"][:a["B"]] == a["K"] - 1)[0])
    assert int(np.sum(a["src"][:a["B"]] == a["K"] - 1)) == 1
    b = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    b["src"][e0] = 0
    b["t_edge"] = np.concatenate([np.argsort(b["src"][:b["B"]], kind="stable"), a["t_edge"][a["B"]:]])
    b["t_indptr"] = np.concatenate([np.searchsorted(b["src"][:b["B"]][b["t_edge"][:b["B"]]], np.arange(b["K"] + 1)),
                                    a["t_indptr"][a["K"] + 1:]])
    with pytest.raises(bi.Violation) as e:
        bi.check(b, caps, graph, seeds)
    assert e.value.invariant == "I5" and "index %d" % e0 in str(e.value)
    b["K"] -= 1                                               # what a clamp at K - 1 leaves: the last source gone, its edge at source 0
    b["kept_nid"][b["K"]] = 0
    kcaps = dict(caps, K=b["K"])
    b["t_indptr"] = b["t_indptr"][:kcaps["K"] + 1]
    bi.check(dict(b, err=4), kcaps, graph, seeds, "K")
    with pytest.raises(bi.Violation) as e:
        bi.check(b, kcaps, graph, seeds, "")
    assert e.value.invariant == "I5"
