"""CPU suite for tests/shard_dense_ref.py, the host restatement that tests/test_gpu_shard_dense_edges.py holds the static-shape
sharded sampler's kernels against.

1. the restatement, run layer by layer over 1, 2 and 3 simulated ranks whose dense buffers are added as integers, gives exactly the
   candidate list, p, c / iters / all_one, P and kept list of the keyed oracle (bo.sample_blocks_bandit);
2. a structural model of the kernels (1024-element blocks, the look-back walk of sd_lookback in 64-wide rounds, the seed mark, the
   step bump, the padding rows, the bf16 rounding) equals the restatement -- and with one fault planted it does not: the
   comparison the GPU module uses (shard_dense_ref.compare on the buffers of want_candidates / want_select, sentinels included)
   fails on the GPU module's own inputs for every fault."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shard_dense_ref as R                                   # noqa: E402
from oracle import bliss_oracle as bo                          # noqa: E402

V, E, FAN, BATCH, ETA, SEED = 3000, 40000, [96, 48, 24], 24, 0.1, 11


@pytest.mark.parametrize("world", [1, 2, 3])
def test_restatement_equals_the_keyed_oracle(world):
    from bliss_gnn_amd import shard as sh
    from bliss_gnn_amd.synth import chung_lu_csc
    from shard_cpu_ops import OracleShardOps
    ip, ix, ei = chung_lu_csc(V, E, seed=5)
    seeds0 = torch.randperm(V, generator=torch.Generator().manual_seed(3))[:BATCH].to(torch.int32)
    og = bo.CSC(ip, ix, ei)
    w = torch.ones(len(FAN), og.num_edges, dtype=torch.bfloat16)
    step = 2
    _, _, oblocks = bo.sample_blocks_bandit(og, seeds0, FAN, w, ETA, uniform_fn=lambda n, nid: bo.keyed_uniform(SEED, step, n, nid))
    bounds = sh.partition_by_in_edges(ip, world)
    shards = [sh.GraphShard.from_global(ip, ix, ei, bounds, r) for r in range(world)]
    ops = [OracleShardOps(g, len(FAN), ETA) for g in shards]
    L = len(FAN)
    seeds_g = seeds0
    for n, layer in enumerate(reversed(range(L))):
        S = int(seeds_g.numel())
        dense = torch.zeros(V, 2, dtype=torch.int64)
        for g, op in zip(shards, ops):
            ls = R.local_seeds(seeds_g, S, g.lo, g.hi, S + 5)
            nl = ls["n_local"]
            assert ls["err"] == 0 and torch.equal(seeds_g[ls["seed_pos"][:nl].long()], ls["seeds_l"][:nl])
            ids, sums = op.frontier_partials(n, layer, ls["seeds_l"][:nl])
            assert torch.equal(ids[:nl], ls["seeds_l"][:nl])             # the rank's seeds first, then the other touched sources
            sc = R.scatter(ids[:nl], sums[:nl], nl, ids[nl:].long(), sums[nl:], int(ids.numel()) - nl, V)
            assert sc["err"] == 0
            dense += sc["dense"]                                        # THE exchange: integer addition
        cd = R.candidates(dense, 0, V)
        ob = oblocks[L - 1 - n]
        tr = ob.trace
        order = torch.argsort(tr["cand_nid"])
        C = cd["C"]
        assert cd["err"] == 0 and torch.equal(cd["cand_nid"].long(), tr["cand_nid"][order].long())
        assert torch.equal(cd["p"], R.bits(tr["p"])[order])
        assert torch.equal(cd["is_seed"].bool(), (order < S))          # the oracle numbers its seeds first
        sc = R.scale(cd["hist"], C, FAN[layer])
        assert (sc["all_one"] == 1) == (C <= FAN[layer])
        assert sc["all_one"] or (sc["c"] == tr["c"] and sc["iters"] == tr["iters"])
        sel = R.select_kept(cd["cand_nid"], cd["p"], cd["is_seed"], C, sc["c"], sc["all_one"], SEED, step, n, seeds_g, S, V,
                            torch.full((V,), -1, dtype=torch.int32), 0, 0)
        assert sel["err"] == 0 and torch.equal(sel["P"], R.bits(tr["P"])[order])
        kept = sel["kept_nid"]
        # shard.py's order: the seeds in (this list's) seed order, then the drawn non-seeds by ascending node id; the oracle keeps
        # first-appearance order, so its list is the same SET, seeds in front, with the same probability per node
        assert torch.equal(kept[:S], seeds_g) and torch.equal(torch.sort(kept[:S].long()).values, torch.sort(ob.src_nid[:S].long()).values)
        assert torch.equal(kept[S:].long(), torch.sort(ob.src_nid[S:]).values.long())
        oracle_prob = dict(zip(ob.src_nid.tolist(), R.bits(ob.node_prob).tolist()))
        assert sel["node_prob"].tolist() == [oracle_prob[v] for v in kept.tolist()]
        assert torch.equal(sel["kept_map"][kept.long()], torch.arange(sel["K"], dtype=torch.int32))
        seeds_g = kept


# ------------------------------------------------------------------------------------------- a structural model of the kernels
def lookback_prefix(counts, fault=None):
    """sd_lookback for every block under the schedule with the LONGEST walks (only block 0 holds an inclusive prefix, every other
    predecessor its own count): rounds of 64 predecessors, ``hi -= 64`` between them, the nearest inclusive word ends the walk."""
    c = np.asarray(counts, dtype=np.int64)
    out = np.zeros(c.size, dtype=np.int64)
    for b in range(1, c.size):
        hi, ex = b - 1, 0
        while True:
            incl = hi - 63 <= 0
            last = 0 if incl else hi - 63                         # the block under lane k
            if fault == "exclusive":                             # lane < k
                last += 1
            ex += int(c[last: hi + 1].sum())
            if fault == "drop" and last <= 1 <= hi:
                ex -= int(c[1])
            if incl:
                break
            hi -= 63 if fault == "twice" else 64
        out[b] = ex
    return out


def _ordered_slots(sel, fault):
    n = sel.numel()
    nb = R.blocks(n)
    pad = torch.zeros(nb * R.BLOCK, dtype=torch.int64)
    pad[:n] = sel.long()
    per = pad.view(nb, R.BLOCK)
    counts = per.sum(1)
    base = torch.from_numpy(lookback_prefix(counts.numpy(), fault))
    at = (base[:, None] + per.cumsum(1) - per).flatten()[:n]
    return at, int(base[-1] + counts[-1])


def model_candidates(dense, uniform_nodes, cap_c, fault=None):
    V = dense.shape[0]
    mark, s = dense[:, 1], dense[:, 0]
    at, total = _ordered_slots(mark != 0, fault if fault in ("drop", "twice", "exclusive") else None)
    out = dict(cand_nid=torch.full((cap_c + R.TAIL,), R.SENT["cand_nid"], dtype=torch.int32),
               p=torch.full((cap_c + R.TAIL,), R.SENT["p"], dtype=torch.int32),
               is_seed=torch.full((cap_c + R.TAIL,), R.SENT["is_seed"], dtype=torch.int32))
    w = torch.nonzero((mark != 0) & (at < cap_c)).flatten()
    p = R.importance(s[w], uniform_nodes)
    out["cand_nid"][at[w]] = w.to(torch.int32)
    out["p"][at[w]] = p
    out["is_seed"][at[w]] = ((mark[w] > R.SEED_MARK) if fault == "seed_gt" else (mark[w] >= R.SEED_MARK)).to(torch.int32)
    out["hist"] = torch.bincount((p & (0xFFFF if fault == "hist_sign" else 0x7FFF)).long(), minlength=R.HIST_BINS)[:R.HIST_BINS].to(torch.int32)
    out.update(C=min(total, cap_c), counts_err=0, iters=0, all_one=0, err=R.ERR_CAP_CAND if bool((at[mark != 0] >= cap_c).any()) else 0,
               dense=torch.zeros_like(dense))
    return out


def model_select(cand, p, is_seed, C, c, all_one, seed, step, layer, seeds_g, S, cap_k, cap_c, V, n_local, bump, fault=None):
    key_step = step + 1 if (fault == "step_early" and bump) else step
    P, keep = R.inclusion(cand[:C], p[:C], is_seed[:C], c, all_one, seed, key_step, layer)
    new = torch.zeros(cap_c, dtype=torch.bool)
    new[:C] = keep & ~is_seed[:C].bool()
    at, total = _ordered_slots(new, fault if fault in ("drop", "twice", "exclusive") else None)
    at = at + S
    out = dict(P=R.padded(P, cap_c + R.TAIL, R.SENT["P"]), kept_nid=torch.full((cap_k + R.TAIL,), R.SENT["kept_nid"], dtype=torch.int32),
               node_prob=torch.full((cap_k + R.TAIL,), R.SENT["node_prob"], dtype=torch.int32),
               kept_map=torch.full((V + R.TAIL,), -1, dtype=torch.int32))
    w = torch.nonzero(new & (at < cap_k)).flatten()
    out["kept_nid"][at[w]] = cand[w]
    out["node_prob"][at[w]] = P[w]
    out["kept_map"][cand[w].long()] = at[w].to(torch.int32)
    j = torch.arange(min(S, cap_k))
    out["kept_nid"][j] = seeds_g[j]
    out["node_prob"][j] = R.ONE
    out["kept_map"][seeds_g[j].long()] = j.to(torch.int32)
    over = S + total > cap_k
    out.update(K=min(S + total, cap_k), layer_C=n_local, err=R.ERR_CAP_KEPT if over else 0, step=step + (1 if bump else 0))
    return out


BIGV = 129 * 1024 + 5
CAND_INPUTS = [(1025, "all", 1, 0), (BIGV, "gap64", 2, 0), (BIGV, "gap65", 8, 1), (232965, "gap130", 2, 0), (BIGV, "random", 8, 0),
               (BIGV, "seed_boundary", 1, 0), (64 * 1024 + 1, "one_per_block", 2, 1)]


@pytest.fixture(scope="module")
def cand_inputs():
    return [(R.make_dense(v, pat, ranks, 100 + i), u) for i, (v, pat, ranks, u) in enumerate(CAND_INPUTS)]


def _select_input():
    C, Vs, S = 65 * 1024 + 1, 2 * (65 * 1024 + 1) + 7, 64
    cand, p, is_seed, seeds = R.hand_list(C, Vs, S, seed=41)
    return dict(cand=cand, p=p, is_seed=is_seed, C=C, c=0.37, all_one=0, seed=SEED, step=(1 << 40) + 3, layer=2, seeds_g=seeds, S=S,
                cap_c=C + 3000, V=Vs, n_local=S, bump=1)


def _sel_want(a, cap_k):
    return R.want_select(a["cand"], a["p"], a["is_seed"], a["C"], a["c"], a["all_one"], a["seed"], a["step"], a["layer"], a["seeds_g"], a["S"],
                         cap_k, a["cap_c"], a["V"], a["n_local"], a["bump"])


def _sel_model(a, cap_k, fault=None):
    return model_select(a["cand"], a["p"], a["is_seed"], a["C"], a["c"], a["all_one"], a["seed"], a["step"], a["layer"], a["seeds_g"], a["S"],
                        cap_k, a["cap_c"], a["V"], a["n_local"], a["bump"], fault)


def test_model_without_a_fault_equals_the_restatement(cand_inputs):
    for dense, u in cand_inputs:
        C = int((dense[:, 1] != 0).sum())
        for cap_c in R.cap_choices(C, dense.shape[0]):
            assert R.compare(model_candidates(dense, u, cap_c), R.want_candidates(dense, u, cap_c)) == []
    a = _select_input()
    K = _sel_want(a, a["V"])["K"]
    for cap_k in (K, K - 1, a["S"]):
        assert R.compare(_sel_model(a, cap_k), _sel_want(a, cap_k)) == []


@pytest.mark.parametrize("fault", ["drop", "twice", "exclusive", "seed_gt"])
def test_planted_candidate_fault_fails_the_comparison(cand_inputs, fault):
    failed = []
    for (dense, u), name in zip(cand_inputs, CAND_INPUTS):
        if R.compare(model_candidates(dense, u, dense.shape[0], fault), R.want_candidates(dense, u, dense.shape[0])):
            failed.append(name)
    assert failed, fault
    if fault == "twice":                                      # needs a walk of two rounds: every input with more than 65 blocks
        assert all(n in failed for n in CAND_INPUTS if n[0] >= 66 * 1024 and n[1] in ("random", "seed_boundary"))
    if fault == "seed_gt":
        assert [n[1] for n in failed] == ["seed_boundary"]     # the one input that holds the mark 2^32 itself


@pytest.mark.parametrize("fault", ["drop", "twice", "exclusive", "step_early"])
def test_planted_select_fault_fails_the_comparison(fault):
    a = _select_input()
    diff = R.compare(_sel_model(a, a["V"], fault), _sel_want(a, a["V"]))
    assert diff, fault
    if fault == "step_early":
        assert R.compare(_sel_model(dict(a, bump=0), a["V"], fault), _sel_want(dict(a, bump=0), a["V"])) == []


def test_histogram_with_the_sign_bit_fails_the_comparison(cand_inputs):
    """k_sd_cand cannot produce a p with the sign bit set (a square root is +0, positive or NaN, and f2bf gives every NaN the pattern
    0x7fc0), so on bliss_shard_candidates' own outputs the two histograms are the same function: the fault shows on the GPU module's
    hand-made p list, which holds 0xffc0, through the same comparison."""
    for dense, u in cand_inputs:
        assert R.compare(model_candidates(dense, u, dense.shape[0], "hist_sign"), R.want_candidates(dense, u, dense.shape[0])) == []
    _, p, _, _ = R.hand_list(5000, 9000, 10, seed=41)
    assert bool((p & 0x8000).any())
    wrong = torch.bincount((p & 0xFFFF).long(), minlength=R.HIST_BINS)[:R.HIST_BINS].to(torch.int32)
    assert R.compare(dict(hist=wrong), dict(hist=R.histogram(p))) != []


@pytest.mark.parametrize("D", [2, 130, 256, 602, 1030])
def test_padding_row_that_keeps_its_table_contents_fails(D):
    rc = R.row_case(D, seed=D)
    n_rows = rc["cap"] - 6
    want = R.pack_rows(rc["nid"], n_rows, rc["lo"], rc["hi"], rc["table"], D)
    assert not want[n_rows:].any() and bool((want[0] == R.bits(rc["table"])[0]).all()) and int(want[0, 0]) == 0x8000
    assert not want[2].any() and not want[3].any()             # ids hi and lo - 1
    faulty = R.pack_rows(rc["nid"], rc["cap"], rc["lo"], rc["hi"], rc["table"], D)     # the row count ignored
    assert R.compare(dict(out=faulty), dict(out=want)) != []


def test_bf16_by_truncation_fails_and_rne_matches_bit_arithmetic():
    v = R.take_rows_f32_values()
    src = v.repeat(2)[: 2 * (v.numel() // 2) * 2].view(2, -1).contiguous()
    D = src.shape[1]
    pos = torch.tensor([1, 0, 5, 0], dtype=torch.int32)
    want = R.take_rows(src, pos, 3, 4, D)
    assert not want[2].any() and not want[3].any()             # pos past the source, and the row behind n
    u = torch.from_numpy(src.numpy().view(np.uint32).astype(np.int64))
    trunc = (u >> 16).to(torch.int32)
    assert R.compare(dict(out=torch.stack([trunc[1], trunc[0], torch.zeros_like(trunc[0]), torch.zeros_like(trunc[0])])), dict(out=want)) != []
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF                       # common.cuh:f2bf
    rne = torch.where((u & 0x7FFFFFFF) > 0x7F800000, torch.full_like(rne, 0x7FC0), rne).to(torch.int32)
    assert R.compare(dict(out=torch.stack([rne[1], rne[0], torch.zeros_like(rne[0]), torch.zeros_like(rne[0])])), dict(out=want)) == []


def test_local_seeds_and_scatter_restatement_edges():
    seeds = torch.tensor([50, 10, 19, 20, 9, 10], dtype=torch.int32)
    r = R.local_seeds(seeds, 6, 10, 20, 8)
    assert r["seeds_l"].tolist() == [10, 19, 10, 50, 50, 50, 50, 50] and r["seed_pos"].tolist() == [1, 2, 5, 0, 0, 0, 0, 0] and r["n_local"] == 3
    r = R.local_seeds(seeds, 6, 10, 20, 4)
    assert r["err"] == R.ERR_CAP_SEEDS and r["n_local"] == 2 and r["seeds_l"].tolist() == [10, 19, 50, 50]
    assert R.local_seeds(seeds, 0, 10, 20, 3)["seeds_l"].tolist() == [10, 10, 10]
    s = R.scatter(torch.tensor([3], dtype=torch.int32), torch.tensor([7]), 1, torch.tensor([-1 & 0xFFFFFFFF, 5, 1, (9 << 32) | 2]),
                  torch.tensor([11, 12, 13, 14]), 4, 5)
    assert s["err"] == R.ERR_CAP_CAND
    assert s["dense"].tolist() == [[0, 0], [13, 1], [14, 1], [7, R.SEED_MARK + 1], [0, 0]]
