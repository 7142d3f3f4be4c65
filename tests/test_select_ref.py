"""CPU: pins tests/select_ref.py, the host restatement that tests/test_gpu_select_edges.py compares the candidate -> kept kernels of
csrc/sampler.hip against.

1. on small random graphs the restatement gives exactly the c, iters, P, kept list and node_prob of bo.sample_blocks_bandit and
   bo.sample_blocks_ladies, fed their own p and candidate lists, with the uniforms of a torch stream and of keyed_uniform; mn_select
   matches their multinomial mode;
2. every (p list, fanout) the GPU module sends through the Poisson scale meets the exact-sum condition at every iteration, so the
   sum of bandit_sampler.py:397 is the same double in any order, and the restatement's scale equals bo.poisson_scale's;
3. a structural model of select_fused_body (chunks, ballots, status words, 64-wide look-back rounds under the schedule with the
   longest walks) equals the restatement -- and with one fault planted fails ``compare`` on the GPU module's own lists."""
import functools
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import select_ref as R                                        # noqa: E402
from oracle import bliss_oracle as bo                          # noqa: E402

ETA, KEY = 0.1, (77, 5)


@functools.lru_cache(maxsize=None)
def _graph(seed, V, E, n_seeds):
    gen = torch.Generator().manual_seed(seed)
    og = bo.prepare_graph(torch.randint(0, V, (E,), generator=gen), torch.randint(0, V, (E,), generator=gen), V)
    seeds = torch.randperm(V, generator=gen)[:n_seeds]
    w = (0.25 + 0.75 * torch.rand(2, og.num_edges, generator=gen)).bfloat16()
    return og, seeds, w


GRAPHS = [(1, 1500, 20000, 24, (120, 60)), (2, 3000, 30000, 40, (400, 50)), (3, 800, 9000, 16, (2000, 90))]


def _oracle(kind, g, poisson, draw):
    og, seeds, w = _graph(*g[:4])
    fan = list(g[4])
    kw = {}
    gen = torch.Generator().manual_seed(5)
    us = [torch.rand(og.num_nodes, generator=gen) for _ in fan]
    if kind == "bandit":
        if poisson and draw == "keyed":
            kw = dict(uniform_fn=lambda n, nid: bo.keyed_uniform(KEY[0], KEY[1], n, nid))
        elif poisson:
            kw = dict(uniforms=us)
        torch.manual_seed(3)
        _, _, blocks = bo.sample_blocks_bandit(og, seeds, fan, w, ETA, poisson=poisson, **kw)
    else:
        torch.manual_seed(3)
        _, _, blocks = bo.sample_blocks_ladies(og, seeds, fan, bo.normalized_edata(og), poisson=poisson, uniforms=us if poisson else None)
    return list(zip(range(len(fan)), reversed(blocks), reversed(fan))), us


@pytest.mark.parametrize("g", GRAPHS, ids=lambda g: "g%d" % g[0])
@pytest.mark.parametrize("kind,draw", [("bandit", "stream"), ("bandit", "keyed"), ("ladies", "stream")])
def test_restatement_equals_the_poisson_oracles(g, kind, draw):
    layers, us = _oracle(kind, g, True, draw)
    for n, ob, fan in layers:
        p, cand = R.bits(ob.trace["p"].bfloat16()), ob.trace["cand_nid"].to(torch.int32)
        assert torch.equal(R.from_bits(p).float(), ob.trace["p"].float())
        C, S = int(p.numel()), ob.n_dst
        c, iters, all_one = R.scale(p, C, fan)
        assert (c, iters, all_one) == (ob.trace["c"], ob.trace["iters"], int(C <= fan))
        u = (KEY[0], KEY[1], n) if draw == "keyed" else us[n]
        r = R.select(p, cand, S, C, c, all_one, u, C, C + 5)
        assert torch.equal(r["P"], R.canon_nan(R.bits(ob.trace["P"].bfloat16())))
        chosen = ob.trace["chosen"]
        assert r["K"] == chosen.numel() == ob.n_src and r["err"] == 0
        assert torch.equal(r["kept_nid"][:r["K"]].long(), ob.src_nid)
        assert torch.equal(r["node_prob"][:r["K"]], R.bits(ob.trace["P"].bfloat16()[chosen]))
        assert torch.equal(torch.nonzero(r["new_id"] >= 0).flatten(), chosen)
        assert bool((r["kept_nid"][r["K"]:] == 0).all()) and bool((r["node_prob"][r["K"]:] == R.ONE).all())
        # the structural model on the same layer
        m, _ = R.model_select(p, cand, S, C, c, all_one, u, C, C + 5)
        assert R.compare(m, r) == []


@pytest.mark.parametrize("g", GRAPHS[:2], ids=lambda g: "g%d" % g[0])
@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_mn_select_equals_the_multinomial_oracles(g, kind):
    layers, _ = _oracle(kind, g, False, None)
    for n, ob, fan in layers:
        p, cand = R.bits(ob.trace["p"].bfloat16()), ob.trace["cand_nid"].to(torch.int32)
        C, S = int(p.numel()), ob.n_dst
        chosen = ob.trace["chosen"]
        r = R.mn_select(p, cand, S, C, None, C, C + 5, num_nodes=_graph(*g[:4])[0].num_nodes, chosen=chosen.to(torch.int32))
        u_nodes = ob.trace["u_nodes"]
        K = int(u_nodes.numel())
        assert (r["K"], r["err"]) == (K, 0)
        assert torch.equal(r["kept_nid"][:K].long(), ob.src_nid) and torch.equal(r["P"], p)
        assert torch.equal(r["node_prob"][:K], p[u_nodes])
        member = torch.zeros(C, dtype=torch.bool)
        member[u_nodes] = True
        drawn = torch.zeros(C, dtype=torch.bool)
        drawn[chosen] = True
        rank = torch.cumsum(member.long(), 0) - 1
        want = torch.where(member & drawn, rank, torch.where(member, -2 - rank, torch.full_like(rank, -1)))
        assert torch.equal(r["new_id"].long(), want)
        assert torch.equal(torch.nonzero(r["kept_map"] >= 0).flatten(), torch.sort(cand[drawn].long()).values)
        marks = drawn.to(torch.int32)
        r2 = R.mn_select(p, cand, S, C, marks, C, C + 5, num_nodes=_graph(*g[:4])[0].num_nodes)
        assert R.compare(r2, r) == []
    # chosen out of range: bit 2, the rest still marked
    bad = torch.cat([chosen.to(torch.int32), torch.tensor([-1, C], dtype=torch.int32)])
    rb = R.mn_select(p, cand, S, C, None, C, C + 5, chosen=bad)
    assert rb["err"] == R.ERR_CAP_CAND and torch.equal(rb["new_id"], r["new_id"])


@functools.lru_cache(maxsize=None)
def _list(C, kind, seed):
    return R.make_list(C, kind, seed)


def test_every_scaled_input_meets_the_exact_sum_condition():
    """q + log2(sum) < 53 at every iteration of every (list, fanout) the GPU module scales; and then the restatement's exact sum
    gives bo.poisson_scale's c and iters (torch.sum in its own order)."""
    worst, worst_q, worst_sum = -1.0, 0, 0.0
    for C, kind, seed, fan, eps in R.scale_inputs():
        p, _, _ = _list(C, kind, seed)
        conds = R.exact_sum_condition(p, C, fan, eps)
        for q, s in conds:
            if q is None:
                assert kind == "nan"
                continue
            used = q + (math.log2(s) if s > 0 else 0.0)
            assert used < 53, (C, kind, fan, q, s)
            if used > worst:
                worst, worst_q, worst_sum = used, q, s
        c, iters, all_one = R.scale(p, C, fan, eps)
        _, oc, oi = bo.poisson_scale(R.from_bits(p), 0, fan, eps)
        assert iters == oi and (c == oc or (c != c and oc != oc)), (C, kind, fan, c, oc, iters, oi)
        if kind == "nan" and C > fan:
            assert c != c and iters == 50
    print("exact-sum condition: worst q + log2(sum) = %.2f (q = %d, sum = %.6g)" % (worst, worst_q, worst_sum))
    assert 0 < worst < 53


def test_the_unsettled_list_runs_all_fifty_iterations_and_the_ladder_has_every_iteration_class():
    p, _, _ = _list(1000, "unsettled", 1007)
    assert R.scale(p, 1000, 333)[1] == 50
    seen = set()
    for C in (1025, 150000):
        p, _, _ = _list(C, "window", C)
        for f in R.fanouts(C):
            c, iters, all_one = R.scale(p, C, f)
            seen.add("all_one" if all_one else ("one" if iters == 1 else "several"))
    assert {"all_one", "several"} <= seen


MODEL_CASES = [(1, "window"), (1023, "window"), (1024, "window"), (1025, "window"), (3000, "zeros"), (3000, "high"), (1025, "tiny"),
               (3000, "nan"), (3000, "payload"), (65537, "window"), (66561, "window"), (132101, "window"), (150000, "payload")]


def _scaled(C, kind, fan):
    p, cand, V = _list(C, kind, C + 7 if kind != "window" else C)
    if kind == "payload":
        return p, cand, V, 0.37, 0
    c, _, all_one = R.scale(p, C, max(fan, 1))                # (a fanout of 0 is not a defined input: select_ref.fanouts)
    return p, cand, V, c, all_one


@pytest.mark.parametrize("C,kind", MODEL_CASES)
def test_structural_model_equals_the_restatement(C, kind):
    for i, fan in enumerate((C // 3, C // 50, C + 3)):
        p, cand, V, c, all_one = _scaled(C, kind, fan)
        S = R.seeds_for(C, i + 1)
        for cap_c, cap_k in ((C + 3000, C + 3000), (C, max(S, C // 7)), (max(C - 1, 1), C)):
            for u in (R.make_uniforms(p, C), (1234, 2 ** 40 + 3, 2)):
                r = R.select(p, cand, S, C, c, all_one, u, cap_c, cap_k, num_nodes=V)
                m, info = R.model_select(p, cand, S, C, c, all_one, u, cap_c, cap_k, num_nodes=V, bump_step=1)
                assert R.compare(m, r) == [] and R.compare(r, m) == []
                if isinstance(u, tuple):
                    assert info["step"] == 2 ** 40 + 4


def test_ladder_sizes_past_65536_walk_two_and_three_rounds():
    rounds = {}
    for C in (65 * 1024, 64 * 1024 + 1, 65 * 1024 + 1, 129 * 1024 + 5, 150000):
        p, cand, V, c, all_one = _scaled(C, "window", C // 3)
        _, info = R.model_select(p, cand, 64, C, c, all_one, R.make_uniforms(p, C), C, C)
        rounds[C] = int(info["rounds"].max())
        assert int(info["rounds"][0]) == 0 and int(info["rounds"][-1]) == rounds[C]
    assert rounds[65 * 1024] == 1 and rounds[64 * 1024 + 1] == 1            # 65 chunks: the last one has 64 predecessors
    assert rounds[65 * 1024 + 1] >= 2 and rounds[129 * 1024 + 5] >= 3 and rounds[150000] >= 3


# fault -> the lists of the GPU module on which it must show, and a list on which it cannot
FAULT_LISTS = {
    "top_65": ([(66561, "window"), (132101, "window"), (150000, "payload")], [(65537, "window")]),
    "lane_lt_stop": ([(1025, "window"), (66561, "window"), (3000, "zeros")], [(1024, "window")]),
    "agg_dropped": ([(3000, "zeros"), (66561, "window")], [(1025, "window")]),
    "pfx_exclusive": ([(1025, "window"), (132101, "window")], [(1024, "window")]),
    "seed_le": ([(1025, "window"), (3000, "high")], []),
    "bernoulli_le": ([(3000, "zeros"), (3000, "payload")], []),
    "pad_from_K1": ([(1025, "window"), (1, "window")], []),
    "truncate": ([(1025, "window"), (66561, "window")], []),
    "bump_before_key": ([(1025, "window"), (3000, "payload")], []),
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_a_planted_fault_fails_compare_on_the_gpu_modules_lists(fault):
    shows, hidden = FAULT_LISTS[fault]
    for must, cases in ((True, shows), (False, hidden)):
        for C, kind in cases:
            p, cand, V, c, all_one = _scaled(C, kind, C // 3)
            S = min(64, C // 2)
            u = (1234, 7, 2) if fault == "bump_before_key" else R.make_uniforms(p, C + 7 if kind != "window" else C)
            r = R.select(p, cand, S, C, c, all_one, u, C + 3000, C + 40, num_nodes=V)
            want = R.want_buffers(r, C + 3000, C + 40)
            good, _ = R.model_select(p, cand, S, C, c, all_one, u, C + 3000, C + 40, num_nodes=V, bump_step=1)
            assert R.compare(R.want_buffers(good, C + 3000, C + 40), want) == []
            bad, _ = R.model_select(p, cand, S, C, c, all_one, u, C + 3000, C + 40, num_nodes=V, bump_step=1, fault=fault)
            diff = R.compare(R.want_buffers(bad, C + 3000, C + 40), want)
            assert bool(diff) == must, (fault, C, kind, diff)
