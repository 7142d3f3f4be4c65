"""GPU suite: how k_tile_gemm / k_tile_gemm_wide (csrc/sage.hip) bring their operands in -- the batched row staging of
stage_rows, the two-set W slab pipeline of mma_product and its written-out last slabs, the dword loads of the partial last
slab -- at the shapes where that code takes another path, checked for EQUALITY on exact data.

Operands are small integers (A in -3 .. 3, W in -2 .. 2, bias in -8 .. 8): every product and every fp32 partial sum is an
integer below 2^24, so the accumulator is exact whatever the order, and the stored value is the one bf16 rounding (nearest
even) of the exact sum.  The reference is that sum in float64, rounded once by torch.  A dword taken from the wrong column,
row or slab, a mask applied to the wrong register or a slab multiplied twice or not at all changes an integer.

Every operand is the window buf[:, 2 : 2 + K] of a NaN-filled buffer of width K + 4: 4-byte aligned with an even row stride
(the fast paths), and a load that strays past either end of a row and is used turns the result into NaN.  Rows beyond the
device-side count are NaN as well; the gathered table is followed by NaN rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF = torch.bfloat16


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float().to(BF)


def _window(t, dev, rows_after=0):
    """t as buf[:rows, 2 : 2 + cols] of a NaN buffer [rows + rows_after, cols + 4] on the device."""
    rows, cols = t.shape
    buf = torch.full((rows + rows_after, cols + 4), NAN, dtype=BF, device=dev)
    v = buf[:rows, 2:2 + cols]
    v.copy_(t.to(dev))
    assert v.data_ptr() % 4 == 0 and v.stride(0) % 2 == 0
    return v


def _bits(t):
    return t.contiguous().view(torch.int16)


def _exact(a1, w1, a2=None, w2=None, bias=None, relu=False):
    ref = a1.double() @ w1.double().t()
    if a2 is not None:
        ref += a2.double() @ w2.double().t()
    if bias is not None:
        ref += bias.double()
    assert float(ref.abs().max()) < 2 ** 24
    if relu:
        ref = torch.relu(ref)
    return ref.float().to(BF)


def _run(dev, K1, N, M, K2=0, gather=False, relu=False, wide=False, extra=40, seed=0):
    """One launch on m_bound = M + extra rows of which M exist; returns what it wrote and the exact reference."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(100003 * K1 + 1009 * K2 + 17 * N + M + seed)
    mb, T = M + extra, 97
    ids = None
    if gather:
        table = _ints(gen, (T, K1), -3, 3)
        ids = torch.randint(0, T, (mb,), generator=gen)
        ids[0] = T - 1                                       # the table's last row and its first one among the live rows
        ids[M - 1] = 0 if M > 1 else T - 1
        a1 = table[ids]
        src = _window(table, dev, rows_after=2)
    else:
        a1 = _ints(gen, (mb, K1), -3, 3)
        a1[M:] = NAN
        src = _window(a1, dev)
    w1 = _ints(gen, (N, K1), -2, 2)
    a2 = w2 = a2d = w2d = None
    if K2:
        a2, w2 = _ints(gen, (mb, K2), -3, 3), _ints(gen, (N, K2), -2, 2)
        a2[M:] = NAN
        a2d, w2d = _window(a2, dev), _window(w2, dev)
    bias = _ints(gen, (N,), -8, 8).to(dev)
    out = torch.full((mb, N), NAN, dtype=BF, device=dev)
    copy = torch.full((mb, K1), NAN, dtype=BF, device=dev) if gather else None
    in_norm = torch.full((mb,), NAN, dtype=BF, device=dev)
    out_norm = torch.full((mb,), NAN, dtype=BF, device=dev)
    m_dev = torch.tensor([M], dtype=torch.int32, device=dev)
    # (the argument record holds addresses only: every operand stays referenced here until the launch has been waited for)
    w1d, idsd = _window(w1, dev), None if ids is None else ids.to(torch.int32).to(dev)
    args = bnn._tg_args(src, w1d, out, mb, ids=idsd, a2=a2d, w2=w2d, bias=bias, m_dev=m_dev.data_ptr(), a_copy=copy, in_norm=in_norm,
                        out_norm=out_norm, relu=relu)
    if wide:
        import ctypes as C
        from bliss_gnn_amd import _lib
        _lib.check(_lib.lib.bliss_tile_gemm_wide(C.byref(args), None, bnn._stream()), "bliss_tile_gemm_wide")
    else:
        bnn._tile_gemm(args)
    torch.cuda.synchronize()
    ref = _exact(a1[:M].to(dev), w1.to(dev), None if a2 is None else a2[:M].to(dev), None if w2 is None else w2.to(dev), bias, relu)
    return dict(out=out, copy=copy, in_norm=in_norm, out_norm=out_norm, ref=ref, a1=a1[:M].to(dev), M=M)


def _check(r, what):
    from bliss_gnn_amd import nn as bnn
    M, out = r["M"], r["out"]
    bad = (_bits(out[:M]) != _bits(r["ref"])).nonzero()
    assert bad.numel() == 0, "%s: %d elements differ from the exact sum, first at %s" % (what, bad.shape[0], bad[0].tolist())
    assert not bool(_bits(out[M:]).any()), what + ": padding rows of out must be exact zeros"
    assert torch.equal(_bits(r["in_norm"][:M]), _bits(bnn.embed_norm(r["a1"].contiguous()))), what + ": in_norm is not embed_norm's"
    assert torch.equal(_bits(r["out_norm"][:M]), _bits(bnn.embed_norm(out[:M].contiguous()))), what + ": out_norm is not embed_norm's"
    assert not bool(_bits(r["in_norm"][M:]).any()) and not bool(_bits(r["out_norm"][M:]).any()), what + ": norms of padding rows"
    if r["copy"] is not None:
        assert torch.equal(_bits(r["copy"][:M]), _bits(r["a1"])), what + ": a_copy is not the gathered rows"
        assert not bool(_bits(r["copy"][M:]).any()), what + ": padding rows of a_copy"


# K / 2 on either side of a multiple of 64 (a lane's 1st .. 8th dword of a row; the last dword repeated beyond the row), one
# to five full W slabs (the steady loop runs 0, 0, 0, 1, 1 times, then 1, 2, 3, 2, 3 written-out slabs), and a partial last
# slab 2, 8, 26 and 62 wide behind 0 .. 15 full ones.  N and M rotate through {1, 33, 41, 255, 256} and {1, 31, 32, 33, 65}.
KS = [2, 126, 128, 130, 510, 512, 514, 1024, 64, 192, 256, 320, 66, 136, 218, 602, 258, 328, 1022, 8, 26, 62, 384, 448]
NS = [1, 33, 41, 255, 256]
MS = [1, 31, 32, 33, 65]
SINGLE = [(K, NS[i % 5], MS[(i + i // 5) % 5]) for i, K in enumerate(KS)] + [(602, 256, 65), (602, 41, 33), (256, 256, 65), (1024, 256, 1)]


@pytest.mark.parametrize("K,N,M", SINGLE, ids=lambda v: str(v))
def test_single_product_is_exact(cuda, K, N, M):
    """Rows as they lie and rows gathered through ids (with the row copy), bias, with and without ReLU."""
    _check(_run(cuda, K, N, M), "plain %dx%dx%d" % (M, K, N))
    _check(_run(cuda, K, N, M, gather=True, relu=True), "gathered %dx%dx%d" % (M, K, N))


@pytest.mark.parametrize("K1,K2,N,M", [(256, 256, 256, 65), (602, 130, 255, 33), (66, 1024, 41, 31), (1024, 602, 256, 32), (2, 64, 1, 1),
                                       (128, 320, 33, 65), (218, 26, 256, 33)], ids=lambda v: str(v))
def test_dual_product_is_exact(cuda, K1, K2, N, M):
    """Both products in one accumulator: the second one's first slabs are requested behind the first one's last."""
    _check(_run(cuda, K1, N, M, K2=K2), "dual %dx(%d+%d)x%d" % (M, K1, K2, N))
    _check(_run(cuda, K1, N, M, K2=K2, gather=True, relu=True), "dual gathered %dx(%d+%d)x%d" % (M, K1, K2, N))


@pytest.mark.parametrize("F,N,n_src,n_dst,src_cnt,dst_cnt", [(602, 256, 130, 70, 101, 65), (256, 41, 97, 33, 65, 31), (66, 255, 40, 33, 33, 1)])
def test_pair_launch_is_exact(cuda, F, N, n_src, n_dst, src_cnt, dst_cnt):
    """Two argument sets in one launch: gathered rows (ids 0 and the table's last row among them, copied out) through W_neigh,
    the first of the same rows as they lie through W_self + bias; each set with its own device-side count below its bound."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(F + n_src)
    T = 97
    table = _ints(gen, (T, F), -3, 3)
    ids = torch.randint(0, T, (n_src,), generator=gen)
    ids[0], ids[src_cnt - 1] = T - 1, 0
    x = table[ids].to(cuda)
    wn, ws, b = _ints(gen, (N, F), -2, 2), _ints(gen, (N, F), -2, 2), _ints(gen, (N,), -8, 8).to(cuda)
    z = torch.full((n_src, N), NAN, dtype=BF, device=cuda)
    y = torch.full((n_dst, N), NAN, dtype=BF, device=cuda)
    copy = torch.full((n_src, F), NAN, dtype=BF, device=cuda)
    norm = torch.full((n_src,), NAN, dtype=BF, device=cuda)
    cnt = torch.tensor([src_cnt, dst_cnt], dtype=torch.int32, device=cuda)
    xs = x.clone()
    xs[dst_cnt:] = NAN
    # (the argument records hold addresses only: every operand stays referenced here until the launch has been waited for)
    td, wnd, wsd, xsd, idsd = _window(table, cuda, rows_after=2), _window(wn, cuda), _window(ws, cuda), _window(xs[:n_dst], cuda), ids.to(torch.int32).to(cuda)
    bnn._tile_gemm(bnn._tg_args(td, wnd, z, n_src, ids=idsd, m_dev=cnt.data_ptr(), a_copy=copy, in_norm=norm),
                   bnn._tg_args(xsd, wsd, y, n_dst, bias=b, m_dev=cnt.data_ptr() + 4))
    torch.cuda.synchronize()
    assert torch.equal(_bits(z[:src_cnt]), _bits(_exact(x[:src_cnt], wn.to(cuda)))), "pair: W_neigh product"
    assert torch.equal(_bits(y[:dst_cnt]), _bits(_exact(x[:dst_cnt], ws.to(cuda), bias=b))), "pair: W_self product"
    assert torch.equal(_bits(copy[:src_cnt]), _bits(x[:src_cnt])) and not bool(_bits(copy[src_cnt:]).any()), "pair: row copy"
    assert torch.equal(_bits(norm[:src_cnt]), _bits(bnn.embed_norm(x[:src_cnt].contiguous()))), "pair: in_norm"
    assert not bool(_bits(z[src_cnt:]).any()) and not bool(_bits(y[dst_cnt:]).any()) and not bool(_bits(norm[src_cnt:]).any())


@pytest.mark.parametrize("K1,K2,N,M", [(602, 0, 256, 33), (1626, 0, 41, 65), (2048, 130, 255, 31), (1090, 1024, 256, 32)], ids=lambda v: str(v))
def test_wide_kernel_is_exact(cuda, K1, K2, N, M):
    """k_tile_gemm_wide shares the helpers: a single panel (the narrow walk), a last panel of 602 and of 66 columns (9 and 1
    full slabs and a partial one), whole panels, and a second operand."""
    _check(_run(cuda, K1, N, M, K2=K2, wide=True), "wide %dx(%d+%d)x%d" % (M, K1, K2, N))
    _check(_run(cuda, K1, N, M, K2=K2, gather=True, relu=True, wide=True), "wide gathered %dx(%d+%d)x%d" % (M, K1, K2, N))
