"""GPU suite (-m gpu): the self-inclusive normalised sum of SAGEConv 'gcn' (csrc/spmm_self.hip) through
``nn.gcn_aggregate`` / ``torch.ops.bliss.spmm_self`` and ``spmm_self_t`` on bounds.edge_shape_spec() -- its first S sources are its
destinations; in-degrees 0, 1, 2, 15..17, 63..65, 255..257, 512, 513, 1500 and a 12 000-edge hub, which reaches the multi-chunk
fix-up.

Forward: bit-equal to the restatement's fp32-ordered value (tests/spmm_self_ref.py reproduces the walk's sum order for every row)
AND each element within bounds.SPMM_K["bf16"] = (1, 0.25) of fp64.  That constant is derived for an fp32 sum of at most 16 384
terms; a row here has deg + 1 terms and two more fp32 roundings (the reciprocal, the product), so it holds for rows of up to
16 381 edges -- asserted for every block used (and on the CPU in tests/test_spmm_self_ref.py).  Backward: d h per element under the
same constant, the destination rows that carry the self term and the sources past S that do not."""
import pytest
import torch

import bounds
import spmm_self_ref as ref

pytestmark = pytest.mark.gpu

K_ULP, K_MAG = bounds.SPMM_K["bf16"]
DIMS = [1, 3, 4, 41, 64, 260]
ROW_LIMIT = bounds.SPMM_MAX_ROW - 3


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


def _check_rows(spec):
    assert int(spec.in_degrees().max()) <= ROW_LIMIT and int(spec.out_degrees().max()) <= ROW_LIMIT


@pytest.fixture(scope="module")
def edge(cuda):
    spec = bounds.edge_shape_spec()
    _check_rows(spec)
    return spec, bounds.to_block(spec, cuda), tuple(t.to(cuda) for t in (spec.indptr, spec.src, spec.dst))


def _rows(n, dim, seed, dev, sliced=False, live=None):
    """Standard-normal bf16 [n, dim]; ``sliced``: columns 2 .. 2 + dim of a wider buffer (4 bytes off 8-byte alignment: the scalar
    path); rows at or past ``live`` are NaN."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, dim + (8 if sliced else 0), generator=gen).bfloat16()
    if live is not None:
        x[live:] = float("nan")
    x = x.to(dev)
    if sliced:
        x = x[:, 2:2 + dim]
        assert x.data_ptr() % 8 == 4 and x.stride(0) == dim + 8
    return x


def _weights(n, seed, dev, live=None):
    w = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) + 0.05).bfloat16()
    if live is not None:
        w[live:] = float("nan")
    return w.to(dev)


def _bwd(blk, w, g, fold, n_src=None):
    from bliss_gnn_amd import ops
    t_indptr, t_edge = blk.transposed()
    counts = getattr(blk, "_counts_dev", None) if blk._nnz_ptr else None
    return ops.spmm_self_t(t_indptr, t_edge, blk.src, blk.dst, blk.indptr, w, g, blk.num_src_nodes() if n_src is None else n_src,
                           blk.num_dst_nodes(), counts, fold)


@pytest.mark.parametrize("dim", DIMS)
def test_forward_bits_and_backward_bound_at_edge_shapes(cuda, edge, dim):
    from bliss_gnn_amd.nn import gcn_aggregate
    spec, blk, (indptr, src, dst) = edge
    S, K, B = spec.S, spec.K, spec.B
    for weighted in (True, False):
        for sliced in (False, True):
            for pair in (False, True):
                what = "dim %d weighted %d sliced %d pair %d" % (dim, weighted, sliced, pair)
                h = _rows(K, dim, 10 + dim, cuda, sliced)
                hs = _rows(S, dim, 20 + dim, cuda, sliced) if pair else None
                w = _weights(B, 30 + dim, cuda) if weighted else None
                out = gcn_aggregate(blk, h, w, hs)
                want = ref.forward_f32(indptr, src, dst, h, w, hs)
                diff = int((_bits(out) != _bits(want)).any(1).sum())
                assert diff == 0, "%s: %d rows differ from the fp32-ordered restatement" % (what, diff)
                r = bounds.assert_within(out, *ref.terms(indptr, src, dst, h, w, hs), K_ULP, K_MAG, "out " + what)
                assert torch.equal(_bits(out[0]), _bits((h if hs is None else hs)[0]))          # degree 0: the self row bit for bit
                assert torch.equal(_bits(out), _bits(gcn_aggregate(blk, h, w, hs)))             # two runs, equal bits
                g = _rows(S, dim, 40 + dim, cuda, sliced)
                gh = _bwd(blk, w, g, not pair)
                rb = bounds.assert_within(gh, *ref.terms_bwd(indptr, src, dst, g, K, w, fold_self=not pair), K_ULP, K_MAG, "d h " + what)
                assert not bool(gh[K - 16:].any())                                              # sources past S that send nothing
                assert pair or bool(gh[0].any())                                                # row 0: no in-edge, its self term
                assert torch.equal(_bits(gh), _bits(_bwd(blk, w, g, not pair)))
                same = int((_bits(gh) == _bits(ref.backward_f32(indptr, src, dst, g, K, w))).all(1).sum()) if not pair else -1
                print(what, "out ratio %.3f" % r, "d h ratio %.3f" % rb, "d h rows equal to the fp32-ordered restatement: %d of %d" % (same, K))


def test_autograd_reaches_the_backward_kernel(cuda, edge):
    from bliss_gnn_amd.nn import gcn_aggregate
    spec, blk, (indptr, src, dst) = edge
    h = _rows(spec.K, 64, 1, cuda).requires_grad_()
    w, g = _weights(spec.B, 2, cuda), _rows(spec.S, 64, 3, cuda)
    gcn_aggregate(blk, h, w).backward(g)
    assert torch.equal(_bits(h.grad), _bits(_bwd(blk, w, g, True)))
    hs = _rows(spec.S, 64, 4, cuda)
    h2 = h.detach().clone().requires_grad_()
    gcn_aggregate(blk, h2, w, hs).backward(g)                                  # a distinct h_self without a gradient: no self term
    assert torch.equal(_bits(h2.grad), _bits(_bwd(blk, w, g, False)))
    with pytest.raises(NotImplementedError, match="h_self"):
        gcn_aggregate(blk, h2, w, hs.clone().requires_grad_())
    with torch.no_grad():                                                      # (forward-only: the pair form is allowed)
        gcn_aggregate(blk, h2, w, hs.clone().requires_grad_())


@pytest.mark.parametrize("B,seed,ec", [(60000, 21, 32), (210000, 22, 64)])
def test_chunk_bands(cuda, B, seed, ec):
    from bliss_gnn_amd.nn import gcn_aggregate
    spec = bounds.spmm_band_spec(B, seed)
    _check_rows(spec)
    assert ref.chunk_edges(spec.B) == ec
    blk = bounds.to_block(spec, cuda)
    indptr, src, dst = (t.to(cuda) for t in (spec.indptr, spec.src, spec.dst))
    h, w, g = _rows(spec.K, 4, seed, cuda), _weights(spec.B, seed + 1, cuda), _rows(spec.S, 4, seed + 2, cuda)
    out = gcn_aggregate(blk, h, w)
    assert torch.equal(_bits(out), _bits(ref.forward_f32(indptr, src, dst, h, w)))
    bounds.assert_within(out, *ref.terms(indptr, src, dst, h, w), K_ULP, K_MAG, "out band %d" % B)
    bounds.assert_within(_bwd(blk, w, g, True), *ref.terms_bwd(indptr, src, dst, g, spec.K, w), K_ULP, K_MAG, "d h band %d" % B)


@pytest.mark.parametrize("dim", [4, 41])
def test_a_block_without_edges_returns_the_self_rows(cuda, dim):
    from bliss_gnn_amd.nn import gcn_aggregate
    spec = bounds.Spec(9, 5, torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    blk = bounds.to_block(spec, cuda)
    blk._transposed = (torch.zeros(10, dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda))   # no edge to group
    h, hs, g = _rows(9, dim, 1, cuda), _rows(5, dim, 2, cuda), _rows(5, dim, 3, cuda)
    assert torch.equal(_bits(gcn_aggregate(blk, h)), _bits(h[:5]))
    assert torch.equal(_bits(gcn_aggregate(blk, h, None, hs)), _bits(hs))
    gh = _bwd(blk, None, g, True)
    assert torch.equal(_bits(gh[:5]), _bits(g)) and not bool(gh[5:].any())


@pytest.mark.parametrize("dim", [4, 41])
def test_capacity_padded_block(cuda, edge, dim):
    """Rows past the live S are +0 with NaN planted in their self rows and in h past the live K; d h past the live K is zero;
    padded edges (their weights NaN) are ignored: the live rows have the bits of the exact-size block."""
    from bliss_gnn_amd.nn import gcn_aggregate
    spec, blk, _ = edge
    pad = bounds.padded_block(spec, cuda)
    S, K, B = spec.S, spec.K, spec.B
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    assert Sc > S and Kc > K and Bc > B and ref.chunk_edges(Bc) == ref.chunk_edges(B)
    h, hs, w, g = _rows(Kc, dim, 1, cuda, live=K), _rows(Sc, dim, 2, cuda, live=S), _weights(Bc, 3, cuda, live=B), _rows(Sc, dim, 4, cuda, live=S)
    for h_self in (None, hs):
        out = gcn_aggregate(pad, h, w, h_self)
        want = gcn_aggregate(blk, h[:K], w[:B], None if h_self is None else hs[:S])
        assert torch.equal(_bits(out[:S]), _bits(want)) and not bool(_bits(out[S:]).any())
    hg = h.clone().requires_grad_()
    gcn_aggregate(pad, hg, w).backward(g)
    assert torch.equal(_bits(hg.grad[:K]), _bits(_bwd(blk, w[:B], g[:S], True))) and not bool(_bits(hg.grad[K:]).any())
