"""CPU: the fixtures of tests/block_build_ref.py really contain what their GPU cases (tests/test_gpu_block_build_shapes.py) are
about -- checked with the oracle alone, so that no GPU case can pass vacuously: the exact list lengths, the parallel pairs at
the stated destinations, c == 1.0 and everything kept where a case relies on it, seeds on both sides of the bitmap's
2048-destination group, the exact frontier lengths, the empty columns, the sparse draw's empty spans."""
import collections

import pytest
import torch

import block_build_ref as bb


def _planted(key, kind="bandit", block=-1):
    """Per special of CASES[key]: (planted destinations, the oracle block's edge indices and destinations of that source)."""
    case = bb.CASES[key]()
    ob = bb.oracle_blocks(key, kind)[2][block]
    return case, ob, {nm: (dests,) + bb.source_list(ob, nid) for nm, (nid, dests) in case.specials.items()}


def _all_kept(ob):
    assert ob.trace["c"] == 1.0 and ob.trace["iters"] == 0
    assert bool(ob.trace["keep"].all()) and ob.src.numel() == ob.trace["E"]
    assert ob.n_src == ob.trace["cand_nid"].numel()


def _check_planted(case, ob, lists):
    """Every special's list in the block: exactly the planted multiset of destinations, in ascending edge index, which in a
    block (edges in frontier order) is ascending destination."""
    seeds = set(case.seeds.tolist())
    for nm, (dests, e, d) in lists.items():
        assert case.specials[nm][0] not in seeds
        assert e.numel() == len(dests), nm
        assert sorted(d.tolist()) == sorted(dests), nm
        assert bool((d[1:] >= d[:-1]).all()) and bool((e[1:] > e[:-1]).all())


def _pairs(dests):
    return {d: n for d, n in collections.Counter(dests).items() if n > 1}


def test_expected_index_is_the_stable_argsort():
    src = torch.tensor([2, 0, 2, 1, 0, 2])
    ti, te = bb.expected_index(src, 4)
    assert ti.tolist() == [0, 2, 3, 6, 6] and te.tolist() == [1, 4, 3, 0, 2, 5]


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_lists_fixture(kind):
    case, ob, lists = _planted("lists", kind)
    _all_kept(ob)
    _check_planted(case, ob, lists)
    S = bb.LIST_S
    assert ob.n_dst == S
    for n in bb.SIMPLE_LENGTHS:                                          # both sides of the 64-edge switch; 128 = two full waves
        dests = lists["simple_%d" % n][0]
        assert len(dests) == n and not _pairs(dests)
    assert len(lists["par65"][0]) == 65 and list(_pairs(lists["par65"][0]).values()) == [2]
    assert len(lists["par130"][0]) == 130 and _pairs(lists["par130"][0]) == {0: 2, 31: 2, 32: 2, S - 1: 2}
    assert len(lists["par134"][0]) == 134 and _pairs(lists["par134"][0]) == {0: 2, 31: 2, 32: 2, S - 1: 2}
    assert set(lists["par134"][0]) == set(range(S))
    assert len(lists["triple70"][0]) == 70 and _pairs(lists["triple70"][0]) == {77: 3}
    assert len(lists["doubled80"][0]) == 80 and set(_pairs(lists["doubled80"][0]).values()) == {2} and len(_pairs(lists["doubled80"][0])) == 40
    assert lists["pair2"][0] == [5, 5]
    assert len(lists["pairs64"][0]) == 64 and len(_pairs(lists["pairs64"][0])) == 32
    # the old ranking rule is wrong exactly on the long lists with a repeat, and leaves slots unwritten there
    ti, want = bb.expected_index(ob.src, ob.n_src)
    old = bb.old_rule_index(ob.src, ob.dst, ob.n_src)
    for nm, (dests, e, _) in lists.items():
        loc = int(ob.src[e[0]])
        seg = slice(int(ti[loc]), int(ti[loc + 1]))
        assert torch.equal(want[seg], e)
        wrong = int((old[seg] != want[seg]).sum())
        assert (wrong > 0) == (nm in bb.LONG_PARALLEL), (nm, wrong)
        if nm in bb.LONG_PARALLEL:
            assert int((old[seg] < 0).sum()) == len(dests) - len(set(dests))


def test_lists_alt_is_another_expectation():
    """The replay test alternates the two seed lists: same sizes, different index (a stale slot would show)."""
    a, b = bb.oracle_blocks("lists")[2][0], bb.oracle_blocks("lists_alt")[2][0]
    case, ob, lists = _planted("lists_alt")
    _all_kept(ob)
    _check_planted(case, ob, lists)
    assert (a.n_src, a.n_dst, a.src.numel()) == (b.n_src, b.n_dst, b.src.numel())
    ea, eb = bb.expected_index(a.src, a.n_src), bb.expected_index(b.src, b.n_src)
    assert not torch.equal(ea[1], eb[1]) and not torch.equal(ea[0], eb[0])


@pytest.mark.parametrize("S", bb.SMALL_S + bb.LARGE_S)
def test_seed_count_fixtures(S):
    key = "S%d" % S
    case, ob, lists = _planted(key)
    _all_kept(ob)
    _check_planted(case, ob, lists)
    assert ob.n_dst == S and lists["all"][0] == list(range(S))
    if S < bb.GROUP:
        assert _pairs(lists["doubled"][0]) == {d: 2 for d in range(S)}
        assert _pairs(lists["tripled"][0]) == {d: 3 for d in range(S)}
        assert (2 * S > 64) == (S >= 33) and 3 * S > 64          # 31, 32 doubled stay on the short path; tripled never does
    else:
        dests = lists["edge"][0]
        rep = min(bb.GROUP, S - 1)
        assert len(dests) == 71 and _pairs(dests) == {rep: 2}
        assert {0, 31, 32, bb.GROUP - 1, rep, S - 1} <= set(dests)
        assert min(dests) < bb.GROUP and (S == bb.GROUP or max(dests) >= bb.GROUP)     # both sides of the 2048 group
        old = bb.old_rule_index(ob.src, ob.dst, ob.n_src)
        assert int((old < 0).sum()) == 1                         # the old rule leaves one slot unwritten: the case can fail


@pytest.mark.parametrize("E", bb.FRONTIERS)
def test_frontier_fixtures(E):
    case, ob, lists = _planted("E%d" % E)
    _all_kept(ob)
    _check_planted(case, ob, lists)
    assert ob.trace["E"] == E == ob.src.numel()                  # chunk (1024) and span (256) edges of the block passes
    assert len(lists["all"][0]) == 70 and len(lists["par"][0]) == 71 and list(_pairs(lists["par"][0]).values()) == [2]


def test_empty_columns_fixture():
    case, ob, lists = _planted("empty")
    _all_kept(ob)
    _check_planted(case, ob, lists)
    deg = ob.indptr[1:] - ob.indptr[:-1]
    assert bb.EMPTY_AT == (0, 35, ob.n_dst - 1)                  # first, middle and last seed
    assert [int(deg[i]) for i in bb.EMPTY_AT] == [0, 0, 0] and int((deg == 0).sum()) == 3
    assert len(lists["par"][0]) == 68 and not set(bb.EMPTY_AT) & set(lists["par"][0])


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_sparse_fixture(kind):
    case, ob, lists = _planted("sparse", kind)
    _check_planted(case, ob, lists)                              # uniform 0.0: the specials are kept whatever P is
    assert ob.trace["c"] != 1.0 and ob.trace["iters"] > 0
    keep, E = ob.trace["keep"], ob.trace["E"]
    frac = float(keep.sum()) / E
    assert 0.03 < frac < 0.08, frac                              # "about 5 %" of the frontier
    per_span = [int(keep[i:i + 256].sum()) for i in range(0, E, 256)]
    assert max(per_span) <= 64                                   # one trip of the pass-1 loop
    assert sum(1 for n, i in zip(per_span, range(0, E, 256)) if n == 0 and i + 256 <= E) >= 1     # a whole span kept nothing
    lo, hi = case.info["cold"]
    assert not bool(((ob.src_nid >= lo) & (ob.src_nid < hi)).any())          # uniform 1.0: never kept
    assert len(lists["par134"][0]) == 134 and len(lists["par65"][0]) == 65


def test_two_layer_fixture():
    case = bb.CASES["two_layer"]()
    blocks = bb.oracle_blocks("two_layer")[2]
    outer, inner = blocks[0], blocks[1]                          # model order: blocks[1] is sampled first (from the seeds)
    _all_kept(outer); _all_kept(inner)
    deep, mid = case.info["deep"], case.info["mid"]
    assert outer.n_dst == inner.n_src and outer.n_dst != case.V  # the second layer's S is not its seed capacity
    assert not bool((inner.src_nid == deep).any())               # no candidate of the first-sampled layer ...
    e, d = bb.source_list(outer, deep)
    assert e.numel() == 71                                       # ... a new source with 71 edges into the second one's seeds
    assert deep not in set(inner.src_nid.tolist()) and int((outer.src_nid == deep).nonzero()) >= outer.n_dst
    dst_nid = outer.src_nid[d]                                   # (a block's destinations are its first sources)
    assert sorted(dst_nid.tolist()) == sorted(mid.tolist() + [case.info["repeat"]])
    old = bb.old_rule_index(outer.src, outer.dst, outer.n_src)
    assert int((old < 0).sum()) >= 1
