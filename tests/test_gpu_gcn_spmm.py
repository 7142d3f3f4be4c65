"""GPU suite (-m gpu): csrc/gcn.hip's message passing -- bliss_gcn_norms, bliss_gcn_spmm_fwd and
bliss_gcn_spmm_bwd per element against fp64 on the same bf16 operands (tests/gcn_ref.py, tests/bounds.py's assert_within).

Block: bounds.edge_shape_spec() (in-degrees 0, 1, 2, 15..17, 63..65, 255..257, 512, 513, 1500, a 12 000-edge hub, a source with
more than 3000 out-edges, sources that never send), exact-size and as bounds.padded_block (rows and edges past the live counts;
their w, h and gout entries NaN).  dim 1, 7, 16, 256; w given and NULL.

Constants gcn_ref.GCN_SPMM_K = (1, 0.25): k_ulp = 1 for the one rounding at the store; k_mag = 0.25 (SPMM_K["bf16"]'s) covers the
fp32 sum of up to 16 384 terms (2^14 * 2^-24 = 2^-10 of the magnitude); the fp32 norms, the coefficient product and the store
scale add four roundings of 2^-24, far inside it.  The norms must equal the NumPy float32 restatement bit for bit.  Padded and
exact results must be bit-equal on the live rows, rows past the counts exact zeros, and two runs bit-equal."""
import pytest
import torch

import gcn_ref as ref
from bounds import assert_within, edge_shape_spec, padded_block, to_block

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _norms(blk):
    from bliss_gnn_amd import _lib
    t_indptr, _ = blk.transposed()
    K, S = blk.num_src_nodes(), blk.num_dst_nodes()
    ns = torch.full((K,), float("nan"), dtype=torch.float32, device=blk.device)
    nd = torch.full((S,), float("nan"), dtype=torch.float32, device=blk.device)
    _lib.check(_lib.lib.bliss_gcn_norms(blk.indptr.data_ptr(), S, t_indptr.data_ptr(), K, nd.data_ptr(), ns.data_ptr(), _st()), "norms")
    return ns, nd


def _spmm(blk, ns, nd, w, h, backward):
    from bliss_gnn_amd.nn import _gcn_spmm
    t_indptr, t_edge = blk.transposed()
    n_rows = blk.num_src_nodes() if backward else blk.num_dst_nodes()
    return _gcn_spmm(backward, (blk.indptr, blk.src, blk.dst, t_indptr, t_edge), w, ns, nd, h, n_rows, blk._nnz_ptr)


@pytest.fixture(scope="module")
def blocks(cuda):
    spec = edge_shape_spec()
    return spec, to_block(spec, cuda), padded_block(spec, cuda)


def test_norms_are_the_fp32_restatement(cuda, blocks):
    spec, blk, pad = blocks
    want_ns, want_nd = ref.norms(spec.src, spec.dst, spec.K, spec.S, sim=True)
    for b in (blk, pad):
        ns, nd = _norms(b)
        assert torch.equal(ns[:spec.K].cpu(), want_ns.float()) and torch.equal(nd[:spec.S].cpu(), want_nd.float())
        assert bool((ns[spec.K:] == 1).all()) and bool((nd[spec.S:] == 1).all())      # rows past the live counts: empty, norm 1


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("dim", [1, 7, 16, 256])
def test_forward_and_backward_per_element_exact_and_padded(cuda, blocks, monkeypatch, dim, weighted):
    spec, blk, pad = blocks
    S, K, B = spec.S, spec.K, spec.B
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    gen = torch.Generator().manual_seed(100 + dim)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=BF)
    h = torch.cat([torch.randn(K, dim, generator=gen).bfloat16(), nan(Kc - K, dim)]).to(cuda)
    g = torch.cat([torch.randn(S, dim, generator=gen).bfloat16(), nan(Sc - S, dim)]).to(cuda)
    w = torch.cat([(torch.rand(B, generator=gen) + 0.05).bfloat16(), nan(Bc - B)]).to(cuda) if weighted else None
    src, dst = spec.src.to(cuda), spec.dst.to(cuda)
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)                              # outputs and fp32 partials start as NaN
    res = {}
    for name, b, hh, gg, ww in (("exact", blk, h[:K].contiguous(), g[:S].contiguous(), None if w is None else w[:B].contiguous()),
                                ("padded", pad, h, g, w), ("again", pad, h, g, w)):
        ns, nd = _norms(b)
        res[name] = (_spmm(b, ns, nd, ww, hh, False), _spmm(b, ns, nd, ww, gg, True))
    monkeypatch.undo()
    torch.cuda.synchronize()
    want_o, mag_o = ref.spmm_terms(src, dst, S, K, h[:K], None if w is None else w[:B])
    want_g, mag_g = ref.spmm_terms(src, dst, S, K, g[:S], None if w is None else w[:B], by_src=True)
    out, gh = res["exact"]
    r = (assert_within(out, want_o, mag_o, *ref.GCN_SPMM_K, "gcn spmm out dim %d" % dim),
         assert_within(gh, want_g, mag_g, *ref.GCN_SPMM_K, "gcn spmm d h dim %d" % dim))
    print("GCN-SPMM dim %d weighted %d: worst ratios out %.3f d h %.3f" % (dim, weighted, r[0], r[1]))
    bits = lambda t: t.contiguous().view(torch.int16)
    for name in ("padded", "again"):
        po, pg = res[name]
        assert po.shape == (Sc, dim) and pg.shape == (Kc, dim)
        assert torch.equal(bits(po[:S]), bits(out)) and torch.equal(bits(pg[:K]), bits(gh)), name + ": live rows bit-equal to the exact block"
        assert not bool(po[S:].any()) and not bool(pg[K:].any()), name + ": rows past the counts must be zero"

