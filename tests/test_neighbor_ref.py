"""CPU suite: the restatement of the device-side neighbor sampler's rule (tests/neighbor_ref.py) shares its mixing with the keyed
uniforms of the oracle, keeps min(fanout, d) edges per column -- the smallest (key, position) pairs -- and draws uniformly."""
import math

import numpy as np
import torch

import neighbor_ref as ref
from oracle import bliss_oracle as bo

SEED = 1234


def small_graph(seed=5, n=60, e=900):
    rng = np.random.default_rng(seed)
    deg = rng.multinomial(e, np.ones(n) / n)
    deg[3] = 0
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.integers(0, n, int(indptr[-1]))
    return indptr, indices


def inclusion_counts(n_steps=2048, fanout=3, seed=SEED, layer=1):
    """The issue's case: one column of degree 8 at positions 0..7; how often every edge is kept over draw steps 0..n_steps-1."""
    hits = np.zeros(8, dtype=np.int64)
    for t in range(n_steps):
        hits[ref.kept_positions(0, 8, fanout, seed, t, layer)] += 1
    return hits


def check_inclusion(hits, n_steps=2048, fanout=3):
    """5 sigma of the binomial around n * fanout / 8 (every edge of a column is kept with the same probability)."""
    mean = n_steps * fanout / 8.0
    sigma = math.sqrt(n_steps * (fanout / 8.0) * (1.0 - fanout / 8.0))
    assert int(hits.sum()) == n_steps * fanout
    for j in range(8):
        print("edge %d: kept %d times, mean %.1f, deviation %.2f sigma" % (j, hits[j], mean, (hits[j] - mean) / sigma))
        assert abs(hits[j] - mean) <= 5.0 * sigma, (j, hits[j], mean, sigma)


def test_keys_share_the_mixing_of_the_oracles_keyed_uniform():
    pos = np.concatenate([np.arange(5000), np.array([2 ** 31 - 1, 2 ** 30 + 12345])]).astype(np.int64)
    for seed, step, layer in ((SEED, 0, 0), (SEED, 7, 2), (2 ** 63 + 11, 123456789, 255)):
        k = ref.keys(seed, step, layer, pos)
        assert k.dtype == np.uint32
        u = bo.keyed_uniform(seed, step, layer, torch.from_numpy(pos)).numpy()
        assert np.array_equal((k >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), u)     # the top 24 bits


def test_per_column_counts_and_kept_positions_are_the_brute_force_selection():
    indptr, indices = small_graph()
    seeds = np.random.default_rng(1).permutation(60)[:25]
    for fanout in (1, 4, 15, 16, 40, -1):
        lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 3, 1)
        deg = indptr[seeds + 1] - indptr[seeds]
        want = deg if fanout < 0 else np.minimum(deg, fanout)
        assert np.array_equal(np.diff(lay["indptr"]), want)
        assert lay["B"] == want.sum() and lay["E"] == deg.sum() and lay["S"] == 25
        for s, nid in enumerate(seeds):
            a, b = int(indptr[nid]), int(indptr[nid + 1])
            p = lay["pos"][lay["indptr"][s]:lay["indptr"][s + 1]].astype(np.int64)
            assert ((p >= a) & (p < b)).all() and (np.diff(p) > 0).all()
            allp = np.arange(a, b)
            k = ref.keys(SEED, 3, 1, allp)
            brute = sorted(zip(k.tolist(), allp.tolist()))[:len(p)]
            assert sorted(q for _, q in brute) == p.tolist()
            assert (lay["dst"][lay["indptr"][s]:lay["indptr"][s + 1]] == s).all()
        # sources: the seeds first, then the others in ascending node id; src maps back to the graph's sources
        assert np.array_equal(lay["kept_nid"][:25], seeds)
        rest = lay["kept_nid"][25:]
        assert (np.diff(rest) > 0).all() and not np.isin(rest, seeds).any()
        assert np.array_equal(lay["kept_nid"][lay["src"]], indices[lay["pos"]])
        assert lay["K"] == len(np.union1d(seeds, indices[lay["pos"]]))
        # the by-source index: every source's edges, ascending
        for j in range(lay["K"]):
            e = lay["t_edge"][lay["t_indptr"][j]:lay["t_indptr"][j + 1]]
            assert (lay["src"][e] == j).all() and (np.diff(e) > 0).all()
        assert lay["t_indptr"][-1] == lay["B"]


def test_layers_chain_through_the_kept_nodes():
    indptr, indices = small_graph()
    seeds = np.array([7, 1, 30])
    lays = ref.sample_blocks(indptr, indices, None, seeds, [2, 3], SEED, 9)
    assert np.array_equal(lays[1]["kept_nid"][:lays[0]["K"]], lays[0]["kept_nid"])
    assert np.array_equal(lays[1]["pos"], ref.sample_layer(indptr, indices, None, lays[0]["kept_nid"], 3, SEED, 9, 1)["pos"])
    assert not np.array_equal(lays[1]["pos"], ref.sample_layer(indptr, indices, None, lays[0]["kept_nid"], 3, SEED, 9, 0)["pos"])


def test_inclusion_frequencies_are_uniform():
    check_inclusion(inclusion_counts())


def test_equal_keys_keep_the_lowest_positions():
    indptr, indices = small_graph()
    ov = np.full(int(indptr[-1]), 77, dtype=np.uint32)
    seeds = np.array([0, 10, 20, 3])
    lay = ref.sample_layer(indptr, indices, None, seeds, 5, SEED, 0, 0, keys_override=ov)
    for s, nid in enumerate(seeds):
        a, b = int(indptr[nid]), int(indptr[nid + 1])
        assert lay["pos"][lay["indptr"][s]:lay["indptr"][s + 1]].tolist() == list(range(a, min(b, a + 5)))
