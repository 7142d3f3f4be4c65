"""GPU suite (-m gpu): the row kernels of csrc/spmm.hip -- k_embed_norm, k_gather_rows_norm<4|2|1>, k_sage_epilogue and
k_sage_epilogue_bwd -- through the C ABI, bit for bit against tests/row_ops_ref.py, at the shapes,
strides and addresses where a row kernel goes wrong.

Every operand is a window of a longer buffer: ``off`` elements past an aligned base, rows ``stride`` elements apart.  Around an
input window everything holds 2^60 (a value that would swamp any norm it entered); an output buffer starts as the sentinel 0xFFFF
(a NaN no kernel here writes) and is compared as a WHOLE image afterwards, so padding columns, rows past n_rows and the elements
before the window are checked with the rows themselves.

The norms are held to the restatement's bits on the path row_ops_ref.norm_path gives for the stored tensor, and the restatement to
its fp64 interval (row_ops_ref.assert_norms, the assertion tests/test_row_ops_ref.py shows the planted faults to fail).  The rows
of 2^63, 2^64 and 2^-70 (designed rows 15-17) are outside the interval's domain -- their squares or their sum leave fp32's normal
range -- and are held to the bits only.  No shape here is one the entry points refuse (those are tests/test_row_ops_abi.py's)."""
import numpy as np
import pytest
import torch

import row_ops_ref as R

pytestmark = pytest.mark.gpu
PAD_BITS = R.bf_bits(R.PAD)


@pytest.fixture
def nan_empty(monkeypatch):
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)


def _L():
    from bliss_gnn_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


class Win:
    """A [n, dim] window of uint16 bit patterns inside a device buffer of ``fill``: first element ``off`` elements past the base,
    rows ``stride`` apart, ``extra`` more rows of room behind it.  ``image`` is the buffer as it must look (numpy)."""

    def __init__(self, dev, n, dim, stride, off, fill, bits=None, extra=3):
        assert stride >= dim and off >= 0
        self.n, self.dim, self.stride, self.off = n, dim, stride, off
        self.image = np.full(off + (n + extra) * stride + 8, fill, dtype=np.uint16)
        if bits is not None:
            self.rows(self.image)[:] = bits
        self.base = torch.from_numpy(self.image.view(np.int16).copy()).to(dev)
        assert self.base.data_ptr() % 16 == 0
        self.ptr = self.base.data_ptr() + 2 * off

    def rows(self, image, first=0, n=None):
        n = self.n - first if n is None else n
        o = self.off + first * self.stride
        return image[o:o + n * self.stride].reshape(n, self.stride)[:, : self.dim]

    def row_ptr(self, first):
        return self.ptr + 2 * first * self.stride

    def path(self, first=0):
        return R.norm_path(self.dim, self.stride, self.row_ptr(first))

    def read(self):
        return self.base.cpu().numpy().view(np.uint16)

    def expect(self, bits, what, first=0):
        """The buffer is its image with ``bits`` in rows first .. first + len(bits): nothing else was written."""
        want = self.image.copy()
        self.rows(want, first, len(bits))[:] = bits
        got = self.read()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, "%d elements differ, first at %d (row %d, column %d): got %#06x want %#06x" % (
            bad.size, bad[0], (bad[0] - self.off) // self.stride, (bad[0] - self.off) % self.stride, got[bad[0]], want[bad[0]]))


def _norm_buf(dev, n):
    return torch.full((n + 8,), -1, dtype=torch.int16, device=dev)


def _norm_check(buf, n, want, what):
    got = buf.cpu().numpy().view(np.uint16)
    assert (got[n:] == R.SENTINEL).all(), (what, "norms written past n_rows")
    bad = np.nonzero(got[:n] != want)[0]
    assert bad.size == 0, (what, "norm bits differ in %d of %d rows, first %d: got %#06x want %#06x" % (bad.size, n, bad[0], got[bad[0]], want[bad[0]]))
    return got[:n]


# ---------------------------------------------------------------------------------------------------------------- embed_norm
NORM_DIMS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 252, 255, 256, 257, 260, 512, 516, 602, 1024, 1433, 4100]
NORM_ROWS = [1, 3, 4, 5, 777]
LAYOUTS = [(0, 0), (4, 0), (1, 0), (0, 1), (0, 2), (0, 4), (4, 4), (1, 1)]           # (stride - dim, off)


def _embed_norm(dev, win, first, n):
    out = _norm_buf(dev, n)
    L = _L()
    L.check(L.lib.bliss_embed_norm(win.row_ptr(first), n, win.dim, win.stride, out.data_ptr(), _st()), "bliss_embed_norm")
    return out


@pytest.mark.parametrize("dim", NORM_DIMS)
def test_embed_norm_shapes_strides_and_addresses(cuda, dim):
    bits, dom = R.designed_rows(dim)
    want = {p: R.embed_norm_bits(bits, p) for p in ("vec4", "scalar")}
    assert want["scalar"][13] == 0x7F80 and want["scalar"][14] == 0x7FC0 and want["scalar"][9] == 0      # inf, NaN, the zero row
    seen = set()
    for pad, off in LAYOUTS:
        win = Win(cuda, 777, dim, dim + pad, off, PAD_BITS, bits)
        for n in NORM_ROWS:
            first = R.START.get(n, 0)
            path = win.path(first)
            seen.add(path)
            what = ("embed_norm", dim, "stride", dim + pad, "off", off, "rows", n, path)
            got = _norm_check(_embed_norm(cuda, win, first, n), n, want[path][first:first + n], what)
            if n == 777:                                                                         # the shared assertion, on the device's answer
                R.assert_norms(got, bits, path, what, dom)
        win.expect(bits, ("embed_norm wrote to its input", dim))
    assert seen == ({"vec4", "scalar"} if dim % 4 == 0 else {"scalar"})


@pytest.mark.parametrize("dim", [64, 256, 600, 1432, 2048, 4100])
def test_embed_norm_takes_the_order_of_the_stored_rows(cuda, dim):
    """Rows whose two orders give different bits: aligned storage must give the vec4 bits, storage one element off (or an odd
    stride) the scalar bits.  A kernel on the wrong path fails."""
    rows = R.order_sensitive_rows(dim, 8, 0)
    want = {p: R.embed_norm_bits(rows, p) for p in ("vec4", "scalar")}
    assert (want["vec4"] != want["scalar"]).all()
    for pad, off, path in ((0, 0, "vec4"), (4, 0, "vec4"), (4, 4, "vec4"), (0, 1, "scalar"), (0, 2, "scalar"), (1, 0, "scalar"), (2, 0, "scalar")):
        win = Win(cuda, 8, dim, dim + pad, off, PAD_BITS, rows)
        assert win.path() == path
        what = ("order-sensitive", dim, pad, off, path)
        got = _norm_check(_embed_norm(cuda, win, 0, 8), 8, want[path], what)
        R.assert_norms(got, rows, path, what)


# ---------------------------------------------------------------------------------------------------------------- gather_rows
GATHER_DIMS = NORM_DIMS + [6144]
FEAT_LAYOUTS = [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (4, 0)]                       # (stride - dim, off): 8-, 2-, 4-, 2-, 4-, 8-byte copies
OUT_LAYOUTS = [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (4, 0)]
V = 40


def _copy_width(dim, f, o):
    al = f.ptr | o.ptr
    if dim % 4 == 0 and f.stride % 4 == 0 and o.stride % 4 == 0 and al % 8 == 0:
        return 8
    if dim % 2 == 0 and f.stride % 2 == 0 and o.stride % 2 == 0 and al % 4 == 0:
        return 4
    return 2


def _ids(n, gen):
    ids = torch.randint(0, V, (n,), generator=gen)
    ids[: min(n, 3)] = ids[0]                                                          # repeats
    ids = torch.sort(ids, descending=True).values
    if n >= 2:
        ids[0], ids[-1] = V - 1, 0                                                     # both ends of the table, still descending
    return ids.to(torch.int32)


@pytest.mark.parametrize("dim", GATHER_DIMS)
def test_gather_rows_every_copy_width_with_every_norm_path(cuda, dim):
    """8-, 4- and 2-byte copies (the offset of feat, feat_stride, and the same of out) crossed with both norm orders (out alone):
    rows equal index_select bit for bit, norms are embed_norm_bits(norm_path(out)) -- order-sensitive rows are in the table --,
    and with norm_out = NULL the copy alone.  dim 6144 needs exactly 48 KiB of LDS, the most a launch may ask for."""
    table, dom = R.designed_rows(dim, V)
    table = table.copy()
    sensitive = dim % 4 == 0 and dim >= 8
    if sensitive:
        table[V - 8:] = R.order_sensitive_rows(dim, 8, 1)
        dom[V - 8:] = True
    want = {p: R.embed_norm_bits(table, p) for p in ("vec4", "scalar")}
    for p in want:
        R.assert_norms(want[p], table, p, ("table", dim), dom)
    if sensitive:
        assert (want["vec4"][V - 8:] != want["scalar"][V - 8:]).all()
    L = _L()
    gen = torch.Generator().manual_seed(dim)
    feats = [Win(cuda, V, dim, dim + pad, off, PAD_BITS, table) for pad, off in FEAT_LAYOUTS]
    seen = set()
    launches = [(5, fi, oi, norm) for fi in range(6) for oi in range(6) for norm in (True, False)]
    launches += [(n, (k + i) % 6, (2 * k + i // 2) % 6, True) for k, n in enumerate((1, 3, 4)) for i in range(12)]
    launches += [(1000, 0, 0, True), (1000, 1, 0, True), (1000, 2, 0, True), (1000, 0, 1, True), (1000, 4, 4, False), (1000, 5, 5, True)]
    for n, fi, oi, with_norm in launches:
        f = feats[fi]
        ids = _ids(n, gen)
        ids_d = ids.to(cuda)
        o = Win(cuda, n, dim, dim + OUT_LAYOUTS[oi][0], OUT_LAYOUTS[oi][1], R.SENTINEL)
        nrm = _norm_buf(cuda, n)
        L.check(L.lib.bliss_gather_rows(f.ptr, f.stride, ids_d.data_ptr(), n, dim, o.ptr, o.stride, nrm.data_ptr() if with_norm else 0, _st()),
                "bliss_gather_rows")
        what = ("gather", dim, "rows", n, "feat", FEAT_LAYOUTS[fi], "out", OUT_LAYOUTS[oi], "copy", _copy_width(dim, f, o), o.path(), with_norm)
        o.expect(table[ids.numpy()], what)
        _norm_check(nrm, n if with_norm else 0, want[o.path()][ids.numpy()] if with_norm else np.zeros(0, np.uint16), what)
        seen.add((_copy_width(dim, f, o), o.path()))
    for f in feats:
        f.expect(table, ("gather wrote to the table", dim))
    if dim % 4 == 0:                       # every width with every order, the 2- and 4-byte copies under the vec4 norm among them
        assert seen >= {(8, "vec4"), (4, "vec4"), (2, "vec4"), (4, "scalar"), (2, "scalar")}, seen
    elif dim % 2 == 0:
        assert seen == {(4, "scalar"), (2, "scalar")}, seen
    else:
        assert seen == {(2, "scalar")}, seen


def test_gather_through_the_frame_at_the_lds_limit(cuda, nan_empty):
    """A 6144-column table goes through bliss_gather_rows (its norms are kept: row_norm_of), a 6145-column one through
    index_select (no norms); the rows are the same."""
    from bliss_gnn_amd.graph import _LazyFrame
    bits, _ = R.designed_rows(6145, V)
    wide = R.to_torch(bits).to(cuda)
    narrow = wide[:, :6144].contiguous()
    idx = _ids(33, torch.Generator().manual_seed(1)).to(cuda)
    got = {}
    for name, t in (("narrow", narrow), ("wide", wide)):
        frame = _LazyFrame({"features": t}, lambda: idx)
        x = frame["features"]
        assert torch.equal(x.view(torch.int16), t[idx.long()].view(torch.int16)), name
        got[name] = (x, frame.row_norm_of(x))
    assert torch.equal(got["wide"][0][:, :6144].view(torch.int16), got["narrow"][0].view(torch.int16))
    assert got["wide"][1] is None and got["narrow"][1] is not None
    want = R.embed_norm_bits(bits[:, :6144], "vec4")[idx.cpu().numpy()]
    assert np.array_equal(R.bits_of(got["narrow"][1]), want)


# ---------------------------------------------------------------------------------------------------------------- sage epilogue
EPI_DIMS = [1, 3, 4, 41, 64, 255, 256, 257, 260, 602]
EPI_ROWS = [1, 3, 4, 5, 252, 256, 257, 512, 516]                                      # grids of 1, 1, 1, 2, 63, 64, 65, 128, 129 workgroups
# (stride - dim, off) of a, b, out: contiguous; a and b column slices; only a one element off; b off and out on an odd stride; out off
EPI_LAYOUTS = [((0, 0), (0, 0), (0, 0)), ((4, 0), (8, 0), (0, 0)), ((0, 1), (0, 0), (0, 0)), ((0, 0), (0, 1), (1, 0)), ((4, 0), (4, 0), (4, 1)),
               ((4, 4), (0, 0), (4, 0))]
BF_MAX = 0x7F7F
PLANTS = [(1.5, -1.5), (-0.0, -0.0), (0.0, -0.0), (1.0, -1.0 + 2.0 ** -8), (-1.0, 1.0 - 2.0 ** -8),       # +0, -0 -> +0, tiny, -tiny
          (1.0, 2.0 ** -8), (1.0078125, 2.0 ** -8), (2.0 ** -8, 1.0078125),                                 # fp32 sums on bf16 ties
          (float("inf"), -float("inf")), (float("nan"), 1.0), (2.0, float("inf"))]                          # NaN sums store +0; inf stays


def _epi_operands(n, dim, seed):
    gen = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, dim, generator=gen).bfloat16(), torch.randn(n, dim, generator=gen).bfloat16()
    a, b = R.bits_of(a).copy(), R.bits_of(b).copy()
    fa, fb = a.reshape(-1), b.reshape(-1)
    for k, (x, y) in enumerate(PLANTS):
        i = (k * 37 + 5) % fa.size
        fa[i], fb[i] = R.bf_bits(x), R.bf_bits(y)
    i = (len(PLANTS) * 37 + 5) % fa.size
    fa[i] = fb[i] = BF_MAX                                                             # bf16 max + bf16 max: inf, and an inf norm
    return a, b


# what the plants must store at p = 0, in PLANTS' order, then max + max
PLANT_OUT = [0, 0, 0, R.bf_bits(2.0 ** -8), 0, R.bf_bits(1.0), R.bf_bits(1.015625), R.bf_bits(1.015625), 0, 0, 0x7F80, 0x7F80]


def _plants_stored_as_stated(out, norm):
    """The reference itself, at p = 0: +0 for a zero, a negative or a NaN sum, ties to even, inf for an overflow and in its row's norm."""
    flat, dim = out.reshape(-1), out.shape[1]
    if flat.size <= len(PLANT_OUT) * 37 + 5:                                           # (the plants overwrite each other in a tiny matrix)
        return
    for k, want in enumerate(PLANT_OUT):
        i = k * 37 + 5
        assert flat[i] == want, (k, hex(flat[i]), hex(want))
        if want == 0x7F80:
            assert norm[i // dim] == 0x7F80


def _epi_launch(dev, a, b, layout, p, seed, ctr, with_norm=True):
    n, dim = a.shape
    (pa, oa), (pb, ob), (po, oo) = layout
    A, B = Win(dev, n, dim, dim + pa, oa, PAD_BITS, a), Win(dev, n, dim, dim + pb, ob, PAD_BITS, b)
    O = Win(dev, n, dim, dim + po, oo, R.SENTINEL)
    nrm = _norm_buf(dev, n)
    L = _L()
    L.check(L.lib.bliss_sage_epilogue_fwd(A.ptr, A.stride, B.ptr, B.stride, n, dim, float(p), seed, 0 if ctr is None else ctr.data_ptr(), O.ptr,
                                          O.stride, nrm.data_ptr() if with_norm else 0, _st()), "bliss_sage_epilogue_fwd")
    return A, B, O, nrm


def _epi_cases():
    cases = [(dim, EPI_ROWS[(3 * di + 2 * li) % 9], lay) for di, dim in enumerate(EPI_DIMS) for li, lay in enumerate(EPI_LAYOUTS)]
    return cases + [(8, 4800, EPI_LAYOUTS[0]), (256, 516, EPI_LAYOUTS[0]), (602, 512, EPI_LAYOUTS[2])]     # 1200 workgroups at dim 8


@pytest.mark.parametrize("p,ctr0", [(0.0, 0), (0.1, 0), (0.25, 41), (0.5, 0xFFFFFFFE), (0.9, 1 << 33)])
def test_sage_epilogue_forward_bit_for_bit(cuda, p, ctr0):
    """out, the dropout mask and the norm against sage_epilogue_ref with the counter read BEFORE the launch; three launches in a
    row on a third of the cases.  After every launch with p > 0 ctr[0] has advanced by exactly 1 and ctr[1..65] are 0 again (the
    two-level ticket at grids of 1 .. 1200 workgroups); the hash sees the counter's low 32 bits (ctr0 = 2^32 - 2 wraps on the way).
    At p = 0 the counter is not touched, and a NULL one is accepted."""
    ctr = torch.zeros(66, dtype=torch.int64, device=cuda)
    ctr[0] = ctr0
    count, seed = ctr0, 0xC0FFEE
    rows_seen = set()
    for ci, (dim, n, layout) in enumerate(_epi_cases()):
        a, b = _epi_operands(n, dim, 1000 * dim + n)
        masks = []
        for rep in range(3 if ci % 3 == 0 else 1):
            use_ctr = None if (p == 0 and ci % 2) else ctr
            assert int(ctr[0]) == count                                                # read before the launch
            A, B, O, nrm = _epi_launch(cuda, a, b, layout, p, seed, use_ctr, with_norm=ci % 5 != 4)
            out, keep, norm = R.sage_epilogue_ref(a, b, p, seed, count, O.path())
            what = ("epilogue", "p", p, "dim", dim, "rows", n, layout, "launch", rep, "ctr", count)
            if p == 0:
                _plants_stored_as_stated(out, norm)
            O.expect(out, what)
            if ci % 5 != 4:
                _norm_check(nrm, n, norm, what)
            else:
                _norm_check(nrm, 0, norm[:0], what)                                    # norm_out = NULL: nothing written
            count += 1 if p > 0 else 0
            c = ctr.cpu().numpy()
            assert int(c[0]) == count and not c[1:].any(), (what, c[:3], int(np.abs(c[1:]).sum()))
            masks.append(keep)
            A.expect(a, what)
            B.expect(b, what)
        if p > 0 and len(masks) == 3 and n * dim >= 64:
            assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
        rows_seen.add(n)
    assert rows_seen == set(EPI_ROWS) | {4800}


@pytest.mark.parametrize("dim", [64, 256, 600])
def test_sage_epilogue_norm_takes_the_order_of_out(cuda, dim):
    """a = order-sensitive rows, b = 0, p = 0: out = a, and norm_out must have embed_norm(out)'s bits -- the vec4 order whenever
    out allows it, whether or not a and b allow 8-byte loads (k_sage_epilogue<VEC4, NORM4>), the scalar order when out does not."""
    rows = R.order_sensitive_rows(dim, 8, 0)
    zero = np.zeros_like(rows)
    want = {p: R.embed_norm_bits(rows, p) for p in ("vec4", "scalar")}
    assert (want["vec4"] != want["scalar"]).all()
    cases = [("every operand aligned", ((0, 0), (0, 0), (0, 0)), "vec4"), ("only a misaligned", ((0, 1), (0, 0), (0, 0)), "vec4"),
             ("only b misaligned", ((0, 0), (0, 2), (0, 0)), "vec4"), ("a on an odd stride", ((1, 0), (0, 0), (4, 0)), "vec4"),
             ("out misaligned", ((0, 0), (0, 0), (0, 1)), "scalar"), ("out on an odd stride", ((0, 0), (0, 0), (1, 0)), "scalar")]
    for name, layout, path in cases:
        A, B, O, nrm = _epi_launch(cuda, rows, zero, layout, 0.0, 0, None)
        assert O.path() == path
        O.expect(rows, (name, dim))
        _norm_check(nrm, 8, want[path], (name, dim, path))


@pytest.mark.parametrize("p", [0.0, 0.1, 0.25, 0.5, 0.9])
def test_sage_epilogue_backward_bit_for_bit(cuda, p):
    """din = bf16(dout * fp32(1 / (1 - p))) where out > 0, else +0, with dout, out and din on strides and offsets of their own; NaN
    and -0 in out give a zero gradient; nothing is written beside din's rows."""
    L = _L()
    layouts = EPI_LAYOUTS + [((0, 0), (0, 0), (8, 0)), ((0, 0), (0, 0), (3, 0))]      # din_stride != dim, every other operand plain
    cases = [(dim, EPI_ROWS[(3 * di + 2 * li) % 9], lay) for di, dim in enumerate(EPI_DIMS) for li, lay in enumerate(layouts)]
    for dim, n, layout in cases + [(8, 4800, layouts[0])]:
        a, b = _epi_operands(n, dim, 77 * dim + n)
        out = R.sage_epilogue_ref(a, b, p, 3, 9)[0].copy()
        g = R.bits_of(torch.randn(n, dim, generator=torch.Generator().manual_seed(dim + n)).bfloat16()).copy()
        fo, fg = out.reshape(-1), g.reshape(-1)
        for k, (o, d) in enumerate(((0x7FC0, 0x3F80), (0x8000, 0x3F80), (0x0000, 0x7F80), (0x3F80, 0x7F80), (0x3F80, 0x7FC0), (0x0001, 0xC000))):
            i = (k * 29 + 1) % fo.size                         # NaN, -0, +0 in out; inf and NaN gradients; the smallest positive out
            fo[i], fg[i] = o, d
        (pg, og), (po, oo), (pd, od) = layout
        G, O = Win(cuda, n, dim, dim + pg, og, PAD_BITS, g), Win(cuda, n, dim, dim + po, oo, PAD_BITS, out)
        D = Win(cuda, n, dim, dim + pd, od, R.SENTINEL)
        L.check(L.lib.bliss_sage_epilogue_bwd(G.ptr, G.stride, O.ptr, O.stride, n, dim, float(p), D.ptr, D.stride, _st()), "bliss_sage_epilogue_bwd")
        what = ("epilogue bwd", "p", p, "dim", dim, "rows", n, layout)
        D.expect(R.sage_epilogue_bwd_ref(g, out, p), what)
        G.expect(g, what)
        O.expect(out, what)


# ---------------------------------------------------------------------------------------------------------------- tile GEMM norms
def _tile(entry, args):
    import ctypes as C
    from bliss_gnn_amd._engine import _stream
    L = _L()
    fn = {"wide": L.lib.bliss_tile_gemm_wide, "tile": L.lib.bliss_tile_gemm}[entry]
    L.check(fn(C.byref(args), None, _stream()), "bliss_tile_gemm(%s)" % entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry,K", [("tile", 256), ("tile", 600), ("wide", 1432), ("wide", 2048), ("wide", 4100)])
def test_tile_gemm_in_norm_on_order_sensitive_rows(cuda, entry, K):
    """in_norm of A rows whose norm depends on the order: the vec4 bits (A is contiguous, K % 4 == 0) -- at K > 1024 with the
    partial sums carried across the 1024-column panels."""
    from bliss_gnn_amd import nn as bnn
    rows = R.order_sensitive_rows(K, 8, 0)
    a = R.to_torch(rows).to(cuda)
    w = (torch.randn(8, K, generator=torch.Generator().manual_seed(K)) * K ** -0.5).bfloat16().to(cuda)
    out = torch.full((8, 8), float("nan"), dtype=torch.bfloat16, device=cuda)
    nrm = _norm_buf(cuda, 8)
    _tile(entry, bnn._tg_args(a, w, out, 8, in_norm=nrm.view(torch.bfloat16)))
    got = _norm_check(nrm, 8, R.embed_norm_bits(rows, "vec4"), ("in_norm", entry, K))
    assert (got != R.embed_norm_bits(rows, "scalar")).all()
    R.assert_norms(got, rows, "vec4", ("in_norm", entry, K))


def test_tile_gemm_out_norm_on_order_sensitive_rows(cuda):
    """W = the 256 x 256 identity, no bias: out == A exactly, so out_norm is a norm of designed rows, in the vec4 order."""
    from bliss_gnn_amd import nn as bnn
    rows = R.order_sensitive_rows(256, 8, 0)
    a = R.to_torch(rows).to(cuda)
    w = torch.eye(256, dtype=torch.bfloat16, device=cuda)
    out = torch.full((8, 256), float("nan"), dtype=torch.bfloat16, device=cuda)
    nrm = _norm_buf(cuda, 8)
    _tile("tile", bnn._tg_args(a, w, out, 8, out_norm=nrm.view(torch.bfloat16)))
    assert np.array_equal(R.bits_of(out), rows)
    _norm_check(nrm, 8, R.embed_norm_bits(rows, "vec4"), "out_norm")


# ---------------------------------------------------------------------------------------------------------------- dropout needs ReLU
def test_dropout_without_relu_is_refused_before_any_launch(cuda, nan_empty):
    """bliss_sage_epilogue_bwd reads its mask from out > 0: _SageDualLinear and _SageAggDual refuse relu=False with p > 0."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(8, 16, generator=gen).bfloat16().to(cuda).requires_grad_()
    w = torch.randn(16, 16, generator=gen).bfloat16().to(cuda)
    ctr = torch.zeros(66, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="without ReLU"):
        bnn._SageDualLinear.apply(x, x, w, w, None, False, 0.25, ctr, 5, 8, 0)
    with pytest.raises(ValueError, match="without ReLU"):
        bnn._SageAggDual.apply(x, None, None, None, None, None, None, None, 8, w, w, None, False, 0.25, ctr, 5, 0)
    assert not ctr.cpu().numpy().any()                                                 # nothing ran
    out, _ = bnn._SageDualLinear.apply(x, x, w, w, None, True, 0.25, ctr, 5, 8, 0)     # with the ReLU it runs
    assert int(ctr[0]) == 1 and bool(torch.isfinite(out.float()).all())
