"""GPU suite: bliss_spmm_max_bwd_relu (csrc/spmm_max.hip), the routed max backward under the ReLU mask of
the maximised rows, alone.

The contract: bit-equal to ``where(act > 0, bliss_spmm_max_bwd's result, +0)`` -- the same sums in the same order with the same
single rounding where the mask passes, +0 where ``act`` is +0, -0 or negative.  Beside that, per element against the float64
restatement of tests/pool_tile_ref.py under bounds.SPMM_K["bf16"] = (1, 0.25), the constant of the unmasked backward (the mask
removes whole elements, never terms of a sum).  ``arg`` is the GPU forward's own (tests/test_gpu_spmm_max.py checks it), ``act``
is independent of the forward's input so that the mask hits winners: a quarter negative, a quarter +0 / -0."""
import pytest
import torch

import pool_tile_ref as ptr
from bounds import SPMM_K, SPMM_MAX_ROW, Spec, assert_within, edge_shape_spec, padded_block, spmm_band_spec, to_block

pytestmark = pytest.mark.gpu
_SPECS = {}


def _spec(name):
    if name not in _SPECS:
        _SPECS[name] = {"edge": edge_shape_spec, "band100k": lambda: spmm_band_spec(100000, 21),
                        "band210k": lambda: spmm_band_spec(210000, 22)}[name]()
    return _SPECS[name]


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _act(rows, dim, gen):
    """bf16 [rows, dim]: half positive, a quarter negative, an eighth +0 and an eighth -0."""
    a = torch.randn(rows, dim, generator=gen).abs() + 0.01
    u = torch.rand(rows, dim, generator=gen)
    a = torch.where(u < 0.25, -a, a)
    a = torch.where((u >= 0.25) & (u < 0.375), torch.zeros(()), a)
    a = torch.where((u >= 0.375) & (u < 0.5), -torch.zeros(()), a)
    return a.bfloat16()


def _arg(blk, h, w):
    from bliss_gnn_amd import ops
    counts = blk._counts_dev if blk._nnz_ptr else None
    return ops.spmm_max(blk.indptr, blk.src, blk.dst, w, h, blk.num_dst_nodes(), counts, True, None, None)[1]


def _both(blk, w, gout, arg, act):
    """(the unmasked backward, the masked one) on the GPU; gout, arg and act may be strided views."""
    from bliss_gnn_amd import ops
    t_indptr, t_edge = blk.transposed()
    counts = blk._counts_dev if blk._nnz_ptr else None
    K = blk.num_src_nodes()
    plain = ops.spmm_max_t(t_indptr, t_edge, blk.src, blk.dst, w, gout, arg, K, counts)
    masked = ops.spmm_max_t_relu(t_indptr, t_edge, blk.src, blk.dst, w, gout, arg, act, K, counts)
    return plain, masked


def _check(spec, blk, w, gout, arg, act, what):
    """One case: the bit contract on every row of ``blk`` (the capacity-padded copy included: its rows past K are cleared by both
    entry points), the restatement on the true rows.  Returns the largest error / bound and (plain, masked)."""
    plain, masked = _both(blk, w, gout, arg, act)
    K = spec.K
    want = torch.where(act[:K].float() > 0, plain[:K], torch.zeros((), dtype=torch.bfloat16, device=plain.device))
    assert torch.equal(_bits(masked[:K]), _bits(want)), what + ": not where(act > 0, bliss_spmm_max_bwd, +0)"
    assert not bool(_bits(masked[K:]).any()), what + ": rows past the live sources"
    wc = None if w is None else w.cpu()[:spec.B]
    r, mag = ptr.masked_backward(spec.src, K, gout.cpu()[:spec.S], arg.cpu()[:spec.S], act.cpu()[:K], wc)
    ratio = assert_within(masked[:K].cpu(), r, mag, *SPMM_K["bf16"], what + " d z")
    hit = (act[:K].float() <= 0) & (plain[:K].float() != 0)
    assert bool(hit.any()), what + ": the mask never removed a non-zero sum"
    return ratio, (plain, masked)


@pytest.mark.parametrize("weighted", [True, False], ids=["w", "1"])
@pytest.mark.parametrize("dim", [1, 3, 4, 41, 64, 260])
def test_edge_shapes(cuda, dim, weighted):
    """The edge-shape block (a source with > 3000 out-edges: ~190 chunks of 16 combined by the fix-up; 16 sources that send
    nothing; chunk band 16).  Contiguous operands; for dim % 4 == 0 also act alone as a column slice 4 bytes off alignment (act
    joins the alignment test of the vector path) and all three operands as column slices (the scalar path)."""
    from bliss_gnn_amd import _lib
    spec = _spec("edge")
    assert int(_lib.lib.bliss_spmm_chunk_edges(spec.B)) == 16
    assert 3000 < int(spec.out_degrees().max()) <= SPMM_MAX_ROW and int((spec.out_degrees() == 0).sum()) >= 16
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(60 + dim)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda) if weighted else None
    h = torch.randn(spec.K, dim, generator=gen).bfloat16().to(cuda)
    gfull = torch.randn(spec.S, dim + 6, generator=gen).bfloat16().to(cuda)
    afull = _act(spec.K, dim + 6, gen).to(cuda)
    arg = _arg(blk, h, w)
    argfull = torch.full((spec.S, dim + 6), -7, dtype=torch.int32, device=cuda)
    argfull[:, 2:2 + dim] = arg
    gout, act = gfull[:, 2:2 + dim].contiguous(), afull[:, 2:2 + dim].contiguous()
    layouts = [("contig", gout, arg, act)]
    if dim % 4 == 0:
        sl = afull[:, 2:2 + dim]
        assert sl.data_ptr() % 8 == 4 and sl.stride(0) != dim
        layouts += [("act-slice", gout, arg, sl), ("slices", gfull[:, 2:2 + dim], argfull[:, 2:2 + dim], sl)]
    seen = []
    for lay, g, a, ac in layouts:
        r, (_, masked) = _check(spec, blk, w, g, a, ac, "edge d%d %s %s" % (dim, "w" if weighted else "1", lay))
        print("RATIO spmm-max-relu-edge d%d-%s-%s-dz %.3f" % (dim, "w" if weighted else "1", lay, r))
        seen.append(_bits(masked))
    assert all(torch.equal(seen[0], s) for s in seen[1:]), "the lane layouts disagree"


@pytest.mark.parametrize("name,ec", [("band100k", 32), ("band210k", 64)])
def test_chunk_bands(cuda, name, ec):
    """Chunk lengths 32 and 64, dim 64, weighted."""
    from bliss_gnn_amd import _lib
    spec = _spec(name)
    assert int(_lib.lib.bliss_spmm_chunk_edges(spec.B)) == ec
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(70 + ec)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    h = torch.randn(spec.K, 64, generator=gen).bfloat16().to(cuda)
    gout = torch.randn(spec.S, 64, generator=gen).bfloat16().to(cuda)
    act = _act(spec.K, 64, gen).to(cuda)
    r, _ = _check(spec, blk, w, gout, _arg(blk, h, w), act, name)
    print("RATIO spmm-max-relu-%s dz %.3f" % (name, r))


def _straddle_spec():
    """40 destinations of two in-edges each: one from source 3, one from source 4 + i mod 5.  By source, source 3's 40 entries
    are positions 0..39 of the list -- chunks 0, 1 and half of 2 at 16 edges a chunk: its row is finished by the fix-up --
    and sources 4..8 hold 8 entries each (the last ones finished inside their chunk)."""
    S = 40
    indptr = torch.arange(S + 1) * 2
    src = torch.stack([torch.full((S,), 3), 4 + torch.arange(S) % 5], 1).reshape(-1)
    dst = torch.repeat_interleave(torch.arange(S), 2)
    return Spec(10, S, indptr, src, dst)


@pytest.mark.parametrize("dim", [8, 5])
def test_mask_in_the_fixup_of_a_row_cut_by_chunks(cuda, dim):
    """Source 3 wins the first half of the columns of all 40 destinations, sources 4..8 the second half.  act alternates in sign
    along the columns (+0 and -0 among the masked ones): source 3's row -- combined from three chunk partials -- is +0 exactly
    where act <= 0 and keeps the unmasked sum elsewhere."""
    from bliss_gnn_amd import _lib
    spec = _straddle_spec()
    assert int(_lib.lib.bliss_spmm_chunk_edges(spec.B)) == 16 and int(spec.out_degrees()[3]) == 40
    blk = to_block(spec, cuda)
    half = dim // 2
    h = torch.ones(spec.K, dim)
    h[3, :half], h[4:9, half:] = 10.0, 20.0
    act = torch.ones(spec.K, dim)
    act[:, 0::2] = torch.tensor([-1.0, 0.0, -0.0, -3.0])[torch.arange(spec.K) % 4].reshape(-1, 1)
    gen = torch.Generator().manual_seed(5)
    gout = (torch.randn(spec.S, dim, generator=gen).abs() + 0.5).bfloat16().to(cuda)
    h, act = h.bfloat16().to(cuda), act.bfloat16().to(cuda)
    for w in (None, torch.full((spec.B,), 1.5).bfloat16().to(cuda)):
        arg = _arg(blk, h, w)
        assert bool((arg[:, :half] % 2 == 0).all()) and bool((arg[:, half:] % 2 == 1).all())
        _, (plain, masked) = _check(spec, blk, w, gout, arg, act, "straddle d%d" % dim)
        assert bool((plain[3, :half] != 0).all()) and not bool(plain[3, half:].any())
        assert not bool(_bits(masked[3, 0::2]).any()), "masked columns of the fix-up's row must be +0"
        assert torch.equal(_bits(masked[3, 1::2]), _bits(plain[3, 1::2]))


def test_block_without_edges(cuda):
    z = torch.zeros(0, dtype=torch.int64)
    spec = Spec(4, 3, torch.zeros(4, dtype=torch.int64), z, z)
    blk = to_block(spec, cuda)
    arg = torch.full((3, 8), -1, dtype=torch.int32, device=cuda)
    act = torch.full((4, 8), float("nan")).bfloat16().to(cuda)
    plain, masked = _both(blk, None, torch.ones(3, 8).bfloat16().to(cuda), arg, act)
    assert not bool(_bits(plain).any()) and not bool(_bits(masked).any())


def test_capacity_padded_block(cuda):
    """bounds.padded_block of the edge-shape block, the pad rows of act and gout NaN, of arg and of the edge weights garbage:
    the live rows have the unpadded block's bits and meet the contract, the pad rows are exactly +0."""
    spec = _spec("edge")
    S, K, B = spec.S, spec.K, spec.B
    blk, pad = to_block(spec, cuda), padded_block(spec, cuda)
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    gen = torch.Generator().manual_seed(18)
    for dim in (64, 41):
        h = torch.randn(Kc, dim, generator=gen).bfloat16().to(cuda)
        gout = torch.randn(Sc, dim, generator=gen).bfloat16()
        gout[S:] = float("nan")
        act = _act(Kc, dim, gen)
        act[K:] = float("nan")
        w = (torch.rand(Bc, generator=gen) + 0.05).bfloat16()
        w[B:] = 1e6
        gout, act, w = gout.to(cuda), act.to(cuda), w.to(cuda)
        arg = _arg(pad, h, w)
        arg[S:] = torch.randint(0, B, (Sc - S, dim), generator=gen).to(torch.int32).to(cuda)
        _, (u_plain, u_masked) = _check(spec, blk, w[:B].contiguous(), gout[:S].contiguous(), arg[:S].contiguous(), act[:K].contiguous(),
                                        "exact d%d" % dim)
        _, (p_plain, p_masked) = _check(spec, pad, w, gout, arg, act, "padded d%d" % dim)
        assert torch.equal(_bits(p_masked[:K]), _bits(u_masked)) and torch.equal(_bits(p_plain[:K]), _bits(u_plain))
        assert p_masked.shape[0] == Kc and not bool(_bits(p_masked[K:]).any())


def test_two_runs_give_identical_bits(cuda):
    spec = _spec("band100k")
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(19)
    h = torch.randn(spec.K, 64, generator=gen).bfloat16().to(cuda)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    gout = torch.randn(spec.S, 64, generator=gen).bfloat16().to(cuda)
    act = _act(spec.K, 64, gen).to(cuda)
    arg = _arg(blk, h, w)
    a, b = _both(blk, w, gout, arg, act)[1], _both(blk, w, gout, arg, act)[1]
    assert torch.equal(_bits(a), _bits(b))
