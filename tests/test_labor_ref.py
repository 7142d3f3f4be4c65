"""CPU suite: the restatement of the device-side LABOR-0 sampler's rule (tests/labor_ref.py) against a brute-force loop, at the
threshold, at d = fanout and fanout + 1, on multi-edges, its monotonicity over columns (what makes it LABOR and not the neighbor
sampler), ``layer_dependency``, six planted faults, and the inclusion statistics of one column."""
import math

import numpy as np
import pytest

import labor_ref as ref
import neighbor_ref

SEED = 1234
STAT_SOURCES = [3, 17, 42, 99, 100, 256, 1000, 4095]


def toy_graph(seed=5, n=60, e=900):
    rng = np.random.default_rng(seed)
    deg = rng.multinomial(e, np.ones(n) / n)
    deg[3] = 0
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.integers(0, n, int(indptr[-1]))
    return indptr, indices


def hash32(seed, step, layer, x):
    """The key of ONE id, in Python integers (no NumPy): SplitMix64 finaliser of mix ^ x, top 32 bits."""
    m = (1 << 64) - 1
    z = neighbor_ref.mix(seed, step, layer) ^ int(x)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z >> 32


def brute_layer(indptr, indices, seeds, fanout, seed, step, layer, ov=None, fault=None):
    """The rule as plain loops over edges.  ``fault``: one deliberate deviation from it (the planted-fault tests)."""
    seeds = [int(s) for s in seeds]
    b_indptr, pos, dst = [0], [], []
    for s, nid in enumerate(seeds):
        a, b = int(indptr[nid]), int(indptr[nid + 1])
        d = b - a
        for p in range(a, b):
            keep = True
            if fanout >= 0 and d > fanout:
                u = int(indices[p])
                if fault == "key_on_position":
                    key = hash32(seed, step, layer, p)
                elif ov is not None:
                    key = int(ov[u])
                else:
                    key = hash32(seed, step, 0 if fault == "layer_ignored" else layer, u)
                thr = (fanout << 32) // d
                if fault == "float_thr":
                    thr = int(np.float32(fanout) / np.float32(d) * np.float32(2.0 ** 32))
                keep = key <= thr if fault == "le" else key < thr
            if keep:
                pos.append(p)
                dst.append(s)
        b_indptr.append(len(pos))
    srcs = [int(indices[p]) for p in pos]
    if fault == "seeds_not_first":
        kept = sorted(set(seeds) | set(srcs))
    else:
        new = [u for u in dict.fromkeys(srcs) if u not in set(seeds)]                 # first appearance, each once
        kept = seeds + (new if fault == "first_appearance" else sorted(new))
    local = {v: i for i, v in enumerate(kept)}
    return dict(indptr=b_indptr, pos=pos, dst=dst, src=[local[u] for u in srcs], kept_nid=kept)


def same(lay, brute):
    return all(np.array_equal(np.asarray(lay[k], dtype=np.int64), np.asarray(brute[k], dtype=np.int64))
               for k in ("indptr", "pos", "dst", "src", "kept_nid"))


# ------------------------------------------------------------------------------------------------- the rule
def test_keys_are_the_neighbor_hash_of_the_source_node_id():
    nid = np.array([0, 1, 31, 32, 4095, 2 ** 31 - 1], dtype=np.int64)
    for seed, step, layer in ((SEED, 0, 0), (SEED, 7, 2), (2 ** 63 + 11, 123456789, 255)):
        k = ref.keys(seed, step, layer, nid)
        assert k.dtype == np.uint32
        assert k.tolist() == [hash32(seed, step, layer, v) for v in nid.tolist()]
    assert ref.mix is neighbor_ref.mix


def test_restatement_is_the_brute_force_loop():
    indptr, indices = toy_graph()
    seeds = np.random.default_rng(1).permutation(60)[:25]
    kept_some, dropped_some = False, False
    for fanout in (1, 4, 15, 16, 40, -1):
        for step, layer in ((3, 1), (0, 0)):
            lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, step, layer)
            assert same(lay, brute_layer(indptr, indices, seeds, fanout, SEED, step, layer))
            deg = indptr[seeds + 1] - indptr[seeds]
            assert lay["S"] == 25 and lay["E"] == deg.sum() and lay["B"] == len(lay["pos"]) and lay["K"] == len(lay["kept_nid"])
            assert np.array_equal(lay["eid"], lay["pos"])
            c = np.diff(lay["indptr"])
            full = (deg <= fanout) | (fanout < 0)
            assert np.array_equal(c[full], deg[full])
            kept_some |= bool((c[~full] > 0).any())
            dropped_some |= bool((c[~full] < deg[~full]).any())
            # sources: the seeds first, then the others in ascending node id; the by-source index
            assert np.array_equal(lay["kept_nid"][:25], seeds)
            rest = lay["kept_nid"][25:]
            assert (np.diff(rest) > 0).all() and not np.isin(rest, seeds).any()
            assert np.array_equal(lay["kept_nid"][lay["src"]], indices[lay["pos"]])
            for j in range(lay["K"]):
                e = lay["t_edge"][lay["t_indptr"][j]:lay["t_indptr"][j + 1]]
                assert (lay["src"][e] == j).all() and (np.diff(e) > 0).all()
            assert lay["t_indptr"][-1] == lay["B"]
    assert kept_some and dropped_some
    eid = np.random.default_rng(2).permutation(int(indptr[-1]))
    lay = ref.sample_layer(indptr, indices, eid, seeds, 4, SEED, 3, 1)
    assert np.array_equal(lay["eid"], eid[lay["pos"]])


def column_graph(*cols, n=None):
    """One seed column per entry of ``cols`` (its list of sources), the columns being nodes 0, 1, ...; every other node has none."""
    n = n or max(max(c) for c in cols if c) + 1
    n = max(n, len(cols))
    deg = np.zeros(n, dtype=np.int64)
    deg[:len(cols)] = [len(c) for c in cols]
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    return indptr, np.array([u for c in cols for u in c], dtype=np.int64)


def test_the_threshold_is_strict():
    srcs = [10, 11, 12, 13, 14, 15, 16]                                           # d = 7, fanout 3: thr = (3 << 32) // 7
    indptr, indices = column_graph(srcs)
    thr = ref.threshold(3, 7)
    assert thr == 1840700269 and thr == (3 * 2 ** 32) // 7
    ov = np.full(17, 0xFFFFFFFF, dtype=np.uint32)
    ov[11], ov[14], ov[16] = thr - 1, thr, 0
    lay = ref.sample_layer(indptr, indices, None, [0], 3, SEED, 0, 0, keys_override=ov)
    assert lay["pos"].tolist() == [1, 6] and lay["kept_nid"].tolist() == [0, 11, 16]
    assert same(lay, brute_layer(indptr, indices, [0], 3, SEED, 0, 0, ov=ov))


def test_degree_at_and_above_the_fanout_and_no_fanout():
    at, above = list(range(20, 25)), list(range(30, 36))                          # d = 5 = fanout, d = 6 = fanout + 1
    indptr, indices = column_graph(at, above)
    ov = np.full(36, 0xFFFFFFFF, dtype=np.uint32)                                 # no key is below any threshold ...
    lay = ref.sample_layer(indptr, indices, None, [0, 1], 5, SEED, 0, 0, keys_override=ov)
    assert lay["indptr"].tolist() == [0, 5, 5]                                    # ... d = fanout is kept whole (no key), d = fanout + 1 keeps nothing
    assert lay["pos"].tolist() == [0, 1, 2, 3, 4]
    lay = ref.sample_layer(indptr, indices, None, [0, 1], -1, SEED, 0, 0, keys_override=ov)
    assert lay["indptr"].tolist() == [0, 5, 11] and lay["B"] == 11 and lay["K"] == 2 + 11
    # with the hash: E[c] = fanout for the d = fanout + 1 column, and always c <= d
    cs = [int(np.diff(ref.sample_layer(indptr, indices, None, [1], 5, SEED, t, 0)["indptr"])[0]) for t in range(512)]
    assert max(cs) <= 6 and abs(sum(cs) / 512 - 5.0) < 5 * math.sqrt(6 * (5 / 6) * (1 / 6) / 512)


def test_a_multi_edge_is_kept_or_dropped_as_one():
    srcs = [7, 9, 7, 11, 12, 7, 13, 14]                                           # source 7 three times
    indptr, indices = column_graph(srcs)
    seen = set()
    for t in range(64):
        p = ref.sample_layer(indptr, indices, None, [0], 3, SEED, t, 0)["pos"].tolist()
        hit = [q in p for q in (0, 2, 5)]
        assert all(hit) or not any(hit)
        seen.add(all(hit))
    assert seen == {True, False}


def test_monotone_over_columns():
    """Two columns of one layer with thr_1 <= thr_2 that share a source: kept in column 1 implies kept in column 2."""
    wide, narrow = list(range(40, 52)), list(range(40, 46))                       # d = 12 and d = 6, sources 40..45 shared
    indptr, indices = column_graph(wide, narrow)
    assert ref.threshold(3, 12) <= ref.threshold(3, 6)
    both, only_narrow = 0, 0
    for t in range(256):
        lay = ref.sample_layer(indptr, indices, None, [0, 1], 3, SEED, t, 1)
        src = lay["kept_nid"][lay["src"]]
        in1, in2 = set(src[lay["dst"] == 0].tolist()), set(src[lay["dst"] == 1].tolist())
        for u in range(40, 46):
            assert u not in in1 or u in in2, (t, u)
            both += u in in1
            only_narrow += u in in2 and u not in in1
    assert both > 0 and only_narrow > 0                                           # (the implication was exercised both ways)


def test_layer_dependency():
    nid = np.arange(200)
    assert not np.array_equal(ref.keys(SEED, 4, 0, nid), ref.keys(SEED, 4, 2, nid))
    indptr, indices = toy_graph()
    seeds = np.array([7, 1, 30])
    dep = ref.sample_blocks(indptr, indices, None, seeds, [3, 3, 3], SEED, 9, layer_dependency=True)
    ind = ref.sample_blocks(indptr, indices, None, seeds, [3, 3, 3], SEED, 9, layer_dependency=False)
    assert len(dep) == len(ind) == 3
    # layer 2 of the dependent draw uses layer 0's keys; of the independent draw, its own
    want = ref.sample_layer(indptr, indices, None, dep[1]["kept_nid"], 3, SEED, 9, 0)
    assert np.array_equal(dep[2]["pos"], want["pos"]) and np.array_equal(dep[2]["kept_nid"], want["kept_nid"])
    want = ref.sample_layer(indptr, indices, None, ind[1]["kept_nid"], 3, SEED, 9, 2)
    assert np.array_equal(ind[2]["pos"], want["pos"])
    assert np.array_equal(dep[0]["pos"], ind[0]["pos"]) and not np.array_equal(dep[1]["pos"], ind[1]["pos"])
    # layers chain through the kept nodes
    assert np.array_equal(ind[1]["kept_nid"][:ind[0]["K"]], ind[0]["kept_nid"])
    # the same variate per vertex: two columns with the same sources and degree, one seeded in layer 0, one in layer 2, keep the
    # same sources under the dependent draw and (somewhere in 64 steps) different ones under the independent draw
    srcs = list(range(100, 112))
    indptr, indices = column_graph(srcs, [1], [2], srcs, n=112)                   # 0 <- srcs; 1 <- 1; 2 <- 2; 3 <- srcs
    differ = 0
    for t in range(64):
        for flag in (True, False):
            l0 = ref.sample_layer(indptr, indices, None, [0], 3, SEED, t, 0)
            l2 = ref.sample_layer(indptr, indices, None, [3], 3, SEED, t, 0 if flag else 2)
            a, b = set(l0["kept_nid"][1:].tolist()), set(l2["kept_nid"][1:].tolist())
            if flag:
                assert a == b
            else:
                differ += a != b
    assert differ > 32


# ------------------------------------------------------------------------------------------------- planted faults
def _fault_case(fault):
    """A small input on which ``fault`` must show; returns (graph, seeds, fanout, step, layer, ov)."""
    if fault in ("le", "float_thr"):
        indptr, indices = column_graph([10, 11, 12, 13, 14, 15, 16])
        ov = np.full(17, 0xFFFFFFFF, dtype=np.uint32)
        ov[11], ov[14] = ref.threshold(3, 7) - 1, ref.threshold(3, 7)             # fp32: 3/7 * 2^32 rounds ABOVE the integer quotient
        return indptr, indices, [0], 3, 0, 0, ov
    indptr, indices = toy_graph()
    seeds = np.random.default_rng(1).permutation(60)[:25]
    return indptr, indices, seeds, 4, 3, 2, None


@pytest.mark.parametrize("fault", ["key_on_position", "le", "float_thr", "layer_ignored", "first_appearance", "seeds_not_first"])
def test_planted_fault_changes_the_output(fault):
    indptr, indices, seeds, fanout, step, layer, ov = _fault_case(fault)
    lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, step, layer, keys_override=ov)
    assert same(lay, brute_layer(indptr, indices, seeds, fanout, SEED, step, layer, ov=ov))
    assert not same(lay, brute_layer(indptr, indices, seeds, fanout, SEED, step, layer, ov=ov, fault=fault)), fault


# ------------------------------------------------------------------------------------------------- statistics
def stat_graph():
    """One column (node 0) whose sources are STAT_SOURCES; 4096 nodes."""
    return column_graph(STAT_SOURCES, n=4096)


def inclusion_counts(n_steps=2048, fanout=3, seed=SEED, layer=1):
    """How often every source of the column is kept over draw steps 0..n_steps-1, and how many steps keep nothing."""
    indptr, indices = stat_graph()
    hits, empty = np.zeros(8, dtype=np.int64), 0
    for t in range(n_steps):
        p = ref.kept_positions(indices, 0, 8, fanout, seed, t, layer)
        hits[p] += 1
        empty += len(p) == 0
    return hits, empty


def check_inclusion(hits, empty, n_steps=2048, fanout=3):
    """5 sigma of the binomial around n * fanout / 8 (every source is kept with probability thr / 2^32 = 3/8 exactly here)."""
    assert ref.threshold(fanout, 8) == fanout << 29
    mean = n_steps * fanout / 8.0
    sigma = math.sqrt(n_steps * (fanout / 8.0) * (1.0 - fanout / 8.0))
    for j in range(8):
        print("source %d: kept %d times, mean %.1f, deviation %.2f sigma" % (STAT_SOURCES[j], hits[j], mean, (hits[j] - mean) / sigma))
        assert abs(hits[j] - mean) <= 5.0 * sigma, (j, hits[j], mean, sigma)
    want_empty = n_steps * (1.0 - fanout / 8.0) ** 8
    print("steps that keep nothing: %d, expected %.1f" % (empty, want_empty))
    assert abs(empty - want_empty) <= 5.0 * math.sqrt(want_empty)


def test_inclusion_frequencies():
    hits, empty = inclusion_counts()
    check_inclusion(hits, empty)
    assert hits.tolist() == [796, 747, 821, 806, 732, 772, 756, 745] and empty == 47      # (the rule is deterministic)
