"""CPU suite for the max-reduce message passing: the vectorised restatement of tests/spmm_max_ref.py
against the definition written as a plain loop, the argument refusals of the two C entry points (no launch is made), and the
Python surface of SAGEConv('pool') that needs no GPU."""
import ctypes as C

import pytest
import torch

import spmm_max_ref as ref


def _hand_block():
    """6 destinations over 9 sources, 3 columns.  Row 0: the rounded-tie pair in column 0 (w = 1.0, 1.0078125 on h = 1.0,
    0.99609375: fp32 products 1.0 and 1.00388..., both messages bf16 1.0) -- column 1 has the larger message second, column 2 a
    second rounded tie (1.0078125 * 1.984375 rounds to 2.0).  Row 1: no edges.  Row 2: parallel edges (source 4 three times,
    unequal weights).  Row 3: one edge.  Row 4: all messages negative, with a -0.0 / 0.0 pair in column 2.  Row 5: the same source
    through equal weights (a tie between parallel edges)."""
    bf = lambda v: torch.tensor(v, dtype=torch.float32).bfloat16()
    h = bf([[1.0, 1.0, 2.0], [0.99609375, 3.0, 1.984375], [-1.0, -2.0, -0.0], [-0.5, -4.0, 0.0], [2.0, -3.0, 0.5],
            [7.0, 0.25, -8.0], [-1.5, -0.75, 0.0], [0.125, 9.0, 1.0], [5.0, 5.0, 5.0]])
    degs = [2, 0, 4, 1, 3, 2]
    src = torch.tensor([0, 1, 4, 5, 4, 4, 7, 2, 3, 6, 8, 8])
    w = bf([1.0, 1.0078125, 0.5, 1.0, 2.0, 2.0, 3.0, 1.0, 1.0, 2.0, 0.5, 0.5])
    indptr = torch.tensor([0] + degs).cumsum(0)
    dst = torch.repeat_interleave(torch.arange(len(degs)), torch.tensor(degs))
    return h, src, dst, indptr, w


@pytest.mark.parametrize("weighted", [True, False])
def test_restatement_equals_the_plain_loop(weighted):
    h, src, dst, indptr, w = _hand_block()
    w = w if weighted else None
    S, K = 6, h.shape[0]
    m, out, arg = ref.forward(src, dst, S, h, w)
    lo, la = ref.loop(indptr, src, S, h, w)
    assert arg.tolist() == la
    assert torch.equal(out.view(torch.int16), torch.tensor(lo).bfloat16().view(torch.int16))           # (-0.0 keeps its sign)
    assert arg[1].tolist() == [-1, -1, -1] and out[1].tolist() == [0.0, 0.0, 0.0]
    if weighted:
        assert 1.0 * 1.0 < float(w[1].float() * h[1, 0].float()) and m[0, 0] == m[1, 0] == 1.0      # the products differ, the messages tie
        assert arg[0].tolist() == [0, 1, 0] and arg[5].tolist() == [10, 10, 10]
        assert arg[2].tolist() == [3, 3, 4]                     # 7 > 2*2; 0.25 > -1.5 = 0.5 * -3; 2 * 0.5 == 2 * 0.5: edge 4 before 5
    assert arg[4, 2] == 7                                       # -0.0 first, 0.0 is not greater
    # backward: every (row, column) with an edge sends exactly one term
    gout = (torch.arange(S * 3, dtype=torch.float32).reshape(S, 3) - 4.0).bfloat16()
    gh, mag = ref.backward(src, K, gout, arg, w)
    want = torch.zeros(K, 3, dtype=torch.float64)
    for i in range(S):
        for c in range(3):
            e = la[i][c]
            if e >= 0:
                want[int(src[e]), c] += (float(w[e]) if weighted else 1.0) * float(gout[i, c])
    assert torch.equal(gh, want) and bool((mag >= gh.abs()).all())


def test_empty_block():
    h = torch.ones(3, 2).bfloat16()
    z = torch.zeros(0, dtype=torch.int64)
    m, out, arg = ref.forward(z, z, 2, h)
    assert m.shape == (0, 2) and not bool(out.any()) and bool((arg == -1).all())
    gh, _ = ref.backward(z, 3, torch.ones(2, 2).bfloat16(), arg)
    assert not bool(gh.any())


def test_max_entry_points_refuse_bad_arguments_before_any_launch():
    """bliss_spmm_max_fwd / _bwd validate on the host: null required pointers, negative counts, dim <= 0, strides below dim,
    missing partials when there is more than one chunk (nnz 17 > the 16-edge chunk)."""
    from bliss_gnn_amd import _lib
    lib, E = _lib.lib, _lib.EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    fwd = lambda indptr=p, src=p, dst=p, w=p, h=p, hs=8, n=4, nd=0, nnz=8, dim=8, out=p, os=8, arg=p, as_=8, part=p: \
        lib.bliss_spmm_max_fwd(indptr, src, dst, w, h, hs, n, nd, nnz, dim, out, os, arg, as_, part, 0)
    assert fwd(indptr=0) == E and fwd(h=0) == E and fwd(out=0) == E and fwd(src=0) == E and fwd(dst=0) == E
    assert fwd(n=-1) == E and fwd(nnz=-1) == E and fwd(dim=0) == E and fwd(dim=-4) == E
    assert fwd(hs=7) == E and fwd(os=7) == E and fwd(as_=7) == E
    assert lib.bliss_spmm_chunk_edges(17) == 16 and fwd(nnz=17, part=0) == E
    bwd = lambda ti=p, te=p, src=p, dst=p, w=p, g=p, gs=8, arg=p, as_=8, n=4, nd=0, nnz=8, dim=8, gh=p, hs=8, part=p: \
        lib.bliss_spmm_max_bwd(ti, te, src, dst, w, g, gs, arg, as_, n, nd, nnz, dim, gh, hs, part, 0)
    assert bwd(ti=0) == E and bwd(te=0) == E and bwd(src=0) == E and bwd(dst=0) == E and bwd(g=0) == E and bwd(arg=0) == E and bwd(gh=0) == E
    assert bwd(n=-1) == E and bwd(nnz=-1) == E and bwd(dim=0) == E
    assert bwd(gs=7) == E and bwd(as_=7) == E and bwd(hs=7) == E
    assert bwd(nnz=17, part=0) == E
    # the partials: per chunk a head and a tail slot of dim fp32 values + dim int32 args
    assert lib.bliss_spmm_max_partial_bytes(0, 8) == 0 and lib.bliss_spmm_max_partial_bytes(17, 8) == 2 * 2 * 2 * 8 * 4
    assert lib.bliss_spmm_max_partial_bytes(210000, 64) == ((210000 + 63) // 64) * 2 * 2 * 64 * 4
    assert lib.bliss_spmm_max_partial_bytes(-1, 8) == E and lib.bliss_spmm_max_partial_bytes(8, 0) == E


def test_sageconv_pool_surface():
    from bliss_gnn_amd import function as fn
    from bliss_gnn_amd.nn import SAGEConv
    layer = SAGEConv(8, 4, "pool")
    assert [(n, tuple(q.shape)) for n, q in layer.named_parameters()] == [
        ("fc_pool.weight", (8, 8)), ("fc_pool.bias", (8,)), ("fc_neigh.weight", (4, 8)), ("fc_self.weight", (4, 8)), ("fc_self.bias", (4,))]
    for other in ("lstm", "gcn"):
        with pytest.raises(NotImplementedError, match="pool"):
            SAGEConv(8, 4, other)
    assert [n for n, _ in SAGEConv(8, 4, "mean").named_parameters()] == ["fc_neigh.weight", "fc_self.weight", "fc_self.bias"]
    r = fn.max("m", "neigh")
    assert (r.kind, r.msg, r.out) == ("max", "m", "neigh")


def test_sage_model_aggregator_argument():
    from bliss_gnn_amd.model import SAGE
    m = SAGE(24, 16, 4, 3, torch.relu, 0.1, aggregator_type="pool")
    assert all(hasattr(l, "fc_pool") for l in m.layers) and len(list(m.parameters())) == 15
    assert not m._mfma_ok(torch.zeros(1))
    with pytest.raises(NotImplementedError, match="pool"):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="wide", aggregator_type="pool")
    with pytest.raises(NotImplementedError):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, aggregator_type="lstm")
    assert not any(hasattr(l, "fc_pool") for l in SAGE(24, 16, 4, 3, torch.relu, 0.1).layers)
