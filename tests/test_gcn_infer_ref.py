"""CPU suite: tests/gcn_infer_ref.py, the NumPy restatement of GCN.inference(path="csc"), is the block
path's arithmetic -- gcn_ref.norms / gcn_ref.spmm_terms applied batch by batch to a NumPy full-neighbour block -- its float32
emulation sits inside gcn_ref.GCN_SPMM_K of the float64 value, and every planted fault lands outside.

GCN_SPMM_K = (1, 0.25): one rounding at the store; the fp32 sum of at most 16 384 terms (the longest row here has 1569)."""
import numpy as np
import pytest
import torch

import gcn_infer_ref as ref
import gcn_ref
from bounds import assert_within

_cache = {}


def _synthetic():
    if "s" not in _cache:
        from bliss_gnn_amd.synth import chung_lu_csc
        ip, ix, _ = chung_lu_csc(2500, 600000, seed=9)
        _cache["s"] = (ip.numpy().astype(np.int64), ix.numpy().astype(np.int32))
    return _cache["s"]


def _feats(V, dim, seed=1, positive=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(V, dim, generator=g) + 0.5 if positive else torch.randn(V, dim, generator=g)
    return x.bfloat16().float().numpy()


def test_the_synthetic_graph_has_the_chunk_classes_the_suites_rely_on():
    ip, ix = _synthetic()
    assert ix.size == 492138 and int(np.diff(ip).max()) == 1569 and int(np.diff(ip).min()) >= 1
    assert np.unique(ref.edge_dst(ip) * 2500 + ix).size == ix.size                       # no parallel edges
    assert ref.batch_chunks(ip, 128) == [16] * 20
    c300 = ref.batch_chunks(ip, 300)
    assert sorted(c300) == [16] + [32] * 8
    assert ref.batch_chunks(ip, 1000) == [32] * 3
    assert ref.batch_chunks(ip, 1250) == [64] * 2
    assert ref.batch_chunks(ip, 37) == [16] * 68


def test_the_small_graph_is_what_it_says():
    ip, ix = ref.small_multigraph()
    deg = np.diff(ip)
    assert ip.size == 61 and list(deg[:10]) == [0, 1, 15, 16, 17, 31, 32, 33, 64, 65] and deg[59] == 0
    row = lambda i: list(ix[ip[i]:ip[i + 1]])
    assert row(12).count(40) == 5 and 20 in row(20)
    assert [i for i in range(60) if 50 in row(i)] == [15, 16, 21] and [i for i in range(60) if 40 in row(i)] == [12]
    cnt = ref.counts(ip, ix, 7)
    e = lambda i, j: int(ip[i]) + row(i).index(j)
    assert cnt[e(15, 50)] == 2 and cnt[e(16, 50)] == 2 and cnt[e(21, 50)] == 1 and cnt[e(12, 40)] == 5
    assert ref.counts(ip, ix, 60)[e(21, 50)] == 3


@pytest.mark.parametrize("graph,bs", [("small", 1), ("small", 7), ("small", 60), ("small", 100), ("synthetic", 300), ("synthetic", 1250)])
def test_restatement_equals_the_block_arithmetic_batch_by_batch(graph, bs):
    ip, ix = ref.small_multigraph() if graph == "small" else _synthetic()
    V = ip.size - 1
    h = _feats(V, 5)
    ns, nd = ref.norms(ip, ix, bs)
    want, mag = ref.spmm_f64(ip, ix, bs, h)
    for b0 in range(0, V, bs):
        b1 = min(V, b0 + bs)
        src, dst, K, S, nid = ref.full_neighbor_block(ip, ix, b0, b1)
        ts, td = torch.from_numpy(src), torch.from_numpy(dst)
        bns, bnd = gcn_ref.norms(ts, td, K, S, sim=True)
        assert np.array_equal(bns.numpy()[src], ns[ip[b0]:ip[b1]].astype(np.float64))
        assert np.array_equal(bnd.numpy(), nd[b0:b1].astype(np.float64))
        r, m = gcn_ref.spmm_terms(ts, td, S, K, torch.from_numpy(h[nid]))
        assert np.allclose(r.numpy(), want[b0:b1], rtol=1e-12, atol=1e-300) and np.allclose(m.numpy(), mag[b0:b1], rtol=1e-12, atol=1e-300)


def _check(got, want, mag, what):
    return assert_within(torch.from_numpy(got), torch.from_numpy(want), torch.from_numpy(mag), *gcn_ref.GCN_SPMM_K, what)


@pytest.mark.parametrize("bs", [1, 7, 60, 100])
def test_float32_emulation_is_inside_the_bound_on_the_small_graph(bs):
    ip, ix = ref.small_multigraph()
    h = _feats(60, 7)
    want, mag = ref.spmm_f64(ip, ix, bs, h)
    assert _check(ref.spmm_f32(ip, ix, bs, h), want, mag, "emulation bs %d" % bs) <= 1.0


def test_float32_emulation_is_inside_the_bound_on_the_synthetic_graph():
    ip, ix = _synthetic()
    h = _feats(2500, 3)
    want, mag = ref.spmm_f64(ip, ix, 300, h)
    got = ref.spmm_f32(ip, ix, 300, h, rows=(250, 650))                         # the end of batch 0, batch 1, the start of batch 2
    assert _check(got[250:650], want[250:650], mag[250:650], "emulation bs 300") <= 1.0


@pytest.mark.parametrize("fault", [{"whole_graph": True}, {"range": (14, 28)}, {"parallel_once": True}, {"spill": True},
                                   {"nd_unclamped": True}], ids=lambda f: next(iter(f)))
def test_planted_faults_land_outside(fault):
    ip, ix = ref.small_multigraph()
    h = _feats(60, 7, positive=True)
    want, mag = ref.spmm_f64(ip, ix, 7, h)
    assert _check(ref.spmm_f32(ip, ix, 7, h), want, mag, "no fault") <= 1.0
    with pytest.raises(AssertionError, match="over the bound"):
        _check(ref.spmm_f32(ip, ix, 7, h, fault=fault), want, mag, "fault %r" % (fault,))


def test_chunk_origin_at_the_range_start_changes_bits():
    """Chunks counted from the range's first edge instead of the batch's: a row cut by the chunk grid gets other partials."""
    ip, ix = _synthetic()
    _, off = ref.batch_table(ip, 300)
    ec = ref.chunk_edges(int(off[2] - off[1]))
    assert ec == 32 and int(off[1]) % ec != 0                                   # batch 1 does not start on the range's grid
    h = _feats(2500, 3)
    rule = ref.spmm_f32(ip, ix, 300, h, rows=(300, 600))
    moved = ref.spmm_f32(ip, ix, 300, h, rows=(300, 600), origin="range", range_row0=0)
    rows = np.flatnonzero((rule[300:600] != moved[300:600]).any(1))
    print("rows of batch 1 whose bits move with the chunk origin: %d of 300" % rows.size)
    assert rows.size >= 1
