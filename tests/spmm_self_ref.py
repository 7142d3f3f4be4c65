"""A vectorised torch restatement of SAGEConv 'gcn' message passing (csrc/spmm_self.hip), imported by
tests/test_spmm_self_ref.py (CPU) and the GPU tests.  A plain helper module like tests/bounds.py; it works on any device.

    out[i] = bf16( (sum_{e -> i} w_e h[src_e] + h_self[i]) * (1.0f / (float)(deg_i + 1)) )
    gz[j]  = bf16( sum_{e : src_e = j} (w_e / (float)(deg_{dst_e} + 1)) g[dst_e] + (j < S ? (1.0f / (float)(deg_j + 1)) g[j] : 0) )

``forward_f32`` / ``backward_f32`` reproduce the kernels' fp32 sum order: a wave owns ``chunk_edges(nnz)`` consecutive entries of
the edge list (by destination in the forward, by source in the backward), sums the entries of one row in list order (a product,
then an add: never fused), a row cut by chunk boundaries adds its chunk partials in chunk order, the self term is added last, the
forward multiplies by the reciprocal, one rounding to bf16.  ``terms`` / ``terms_bwd`` give the fp64 value and the magnitude (the
same formula on the absolute values of the terms, self term included, as bounds.spmm_terms).  ``layer_terms`` is the layer in fp64."""
import torch


def chunk_edges(nnz):
    """spmm_walk.cuh: spmm_chunk_edges."""
    return 64 if nnz >= 200000 else (32 if nnz >= 50000 else 16)


def by_source(src, K):
    """(t_indptr [K + 1], t_edge [B]): the edges grouped by source in ascending edge order (Block.transposed())."""
    src = src.long()
    t_edge = torch.argsort(src, stable=True)
    t_indptr = torch.zeros(K + 1, dtype=torch.int64, device=src.device)
    t_indptr[1:] = torch.cumsum(torch.bincount(src, minlength=K), 0)
    return t_indptr, t_edge


def _ordered_sum(row_of, nbr, coef, h, n_rows, EC):
    """fp32 [n_rows, dim]: per row the sum of coef[k] * h[nbr[k]] over the list positions k of the row (row_of non-decreasing), in the
    walk's order: sequentially inside a (row, chunk) segment, then the segments of a row in chunk order.  Rows without an entry: 0."""
    B, D, dev = int(nbr.numel()), h.shape[1], h.device
    total = torch.zeros(n_rows, D, dtype=torch.float32, device=dev)
    if B == 0:
        return total
    pos = torch.arange(B, device=dev)
    chunk = pos // EC
    new = torch.ones(B, dtype=torch.bool, device=dev)
    new[1:] = (row_of[1:] != row_of[:-1]) | (chunk[1:] != chunk[:-1])
    seg = torch.cumsum(new, 0) - 1
    seg_start = pos[new]
    t = pos - seg_start[seg]
    acc = torch.zeros(int(seg_start.numel()), D, dtype=torch.float32, device=dev)
    hf, cf = h.float(), coef.float()
    for step in range(int(t.max()) + 1):                                    # (at most EC steps; a segment appears once per step)
        k = torch.nonzero(t == step).flatten()
        acc[seg[k]] = acc[seg[k]] + cf[k, None] * hf[nbr[k]]
    seg_row = row_of[seg_start]
    first = torch.ones_like(seg_row, dtype=torch.bool)
    first[1:] = seg_row[1:] != seg_row[:-1]
    sid = torch.arange(seg_row.numel(), device=dev)
    start_of_row = torch.cummax(torch.where(first, sid, torch.zeros_like(sid)), 0)[0]
    q = sid - start_of_row
    for step in range(int(q.max()) + 1):                                    # (a row appears once per step)
        k = torch.nonzero(q == step).flatten()
        total[seg_row[k]] = total[seg_row[k]] + acc[k]
    return total


def _w32(w, B, dev):
    return torch.ones(B, dtype=torch.float32, device=dev) if w is None else w.reshape(-1).float()


def forward_f32(indptr, src, dst, h, w=None, h_self=None):
    """The kernel's value: bf16 [S, dim].  indptr [S + 1], src / dst [B] in CSR order; h bf16 [K, dim]; h_self bf16 [S, dim] or
    None (= h[:S])."""
    S, B, dev = int(indptr.numel()) - 1, int(src.numel()), h.device
    hs = h[:S] if h_self is None else h_self[:S]
    deg = (indptr[1:] - indptr[:-1]).long()
    total = _ordered_sum(dst.long(), src.long(), _w32(w, B, dev), h, S, chunk_edges(B))
    inv = 1.0 / (deg + 1).float()                                           # IEEE fp32 division
    out = ((total + hs.float()) * inv[:, None]).bfloat16()
    return torch.where((deg == 0)[:, None], hs, out)                        # a row without edges: the self row's own bits


def backward_f32(indptr, src, dst, g, K, w=None):
    """The kernel's gradient w.r.t. h (self term on rows < S): bf16 [K, dim].  g bf16 [S, dim]."""
    S, B, dev = int(indptr.numel()) - 1, int(src.numel()), g.device
    deg = (indptr[1:] - indptr[:-1]).long()
    src, dst = src.long(), dst.long()
    t_indptr, t_edge = by_source(src, K)
    coef = _w32(w, B, dev) / (deg[dst] + 1).float()                         # one fp32 division per edge
    total = _ordered_sum(src[t_edge], dst[t_edge], coef[t_edge], g, K, chunk_edges(B))
    inv = 1.0 / (deg + 1).float()
    selfv = torch.zeros(K, g.shape[1], dtype=torch.float32, device=dev)
    selfv[:S] = inv[:, None] * g[:S].float()
    sends = (t_indptr[1:] - t_indptr[:-1]) > 0
    return torch.where(sends[:, None], total + selfv, selfv).bfloat16()


def _coef64(w, B, dev):
    return torch.ones(B, dtype=torch.float64, device=dev) if w is None else w.reshape(-1).double()


def terms(indptr, src, dst, h, w=None, h_self=None):
    """fp64 (value, magnitude) of the forward, both [S, dim]."""
    S, B = int(indptr.numel()) - 1, int(src.numel())
    H = h.double()
    HS = H[:S] if h_self is None else h_self[:S].double()
    src, dst = src.long(), dst.long()
    c = _coef64(w, B, h.device)
    inv = 1.0 / ((indptr[1:] - indptr[:-1]).double() + 1.0)
    ref = torch.zeros(S, H.shape[1], dtype=torch.float64, device=h.device).index_add_(0, dst, c[:, None] * H[src])
    mag = torch.zeros(S, H.shape[1], dtype=torch.float64, device=h.device).index_add_(0, dst, c.abs()[:, None] * H[src].abs())
    return (ref + HS) * inv[:, None], (mag + HS.abs()) * inv[:, None]


def terms_bwd(indptr, src, dst, g, K, w=None, fold_self=True):
    """fp64 (value, magnitude) of the gradient w.r.t. h, both [K, dim]; ``fold_self``: the self term on rows < S."""
    S, B = int(indptr.numel()) - 1, int(src.numel())
    G = g.double()
    src, dst = src.long(), dst.long()
    inv = 1.0 / ((indptr[1:] - indptr[:-1]).double() + 1.0)
    c = _coef64(w, B, g.device) * inv[dst]
    ref = torch.zeros(K, G.shape[1], dtype=torch.float64, device=g.device).index_add_(0, src, c[:, None] * G[dst])
    mag = torch.zeros(K, G.shape[1], dtype=torch.float64, device=g.device).index_add_(0, src, c.abs()[:, None] * G[dst].abs())
    if fold_self:
        ref[:S] += inv[:, None] * G[:S]
        mag[:S] += inv[:, None] * G[:S].abs()
    return ref, mag


def rbf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def layer_terms(indptr, src, dst, h, w_neigh, bias=None, ew=None, g=None, mask=None, p=0.0, relu=True, sim=False):
    """A SAGEConv('gcn') layer with the model's tail in float64, with magnitudes:

        lin_first (in > out):  rst = A(h Wn^T) + b        else:  rst = A(h) Wn^T + b,        out = mask / (1 - p) * rst
        A(t)[i] = (sum_e w_e t[src_e] + t[i]) / (deg_i + 1)

    ``mask`` [S, out]: the product of the ReLU's and the dropout's keep mask (None: rst > 0 when ``relu``, else ones).  With ``g``
    = d out: d = mask / (1 - p) g, db = sum d, and   lin_first: dZ = A^T d, dW = dZ^T h, dh = dZ Wn;   else: dW = d^T A(h),
    dh = A^T (d Wn).  ``sim=True`` rounds to bf16 everything the kernels store in bf16 (Z, the aggregation, the product, rst, out, d,
    dZ / d Wn and every result).  Returns a dict: rst, out, mag_out and with g: d_w, d_b, d_h and mag_<name>."""
    R = rbf if sim else (lambda t: t)
    S, K = int(indptr.numel()) - 1, h.shape[0]
    lin_first = w_neigh.shape[1] > w_neigh.shape[0]
    H, Wn = h.double(), w_neigh.double()
    A = lambda t: terms(indptr, src, dst, t, ew)
    At = lambda t: terms_bwd(indptr, src, dst, t, K, ew)
    if lin_first:
        agg = R(A(R(H @ Wn.t()))[0])
        pre, mag = agg, A(H.abs() @ Wn.abs().t())[1]
    else:
        agg, mag_agg = A(H)
        agg = R(agg)
        pre, mag = R(agg @ Wn.t()), mag_agg @ Wn.abs().t()
    rst = pre
    if bias is not None:
        rst, mag = R(pre + bias.double()), mag + bias.double().abs()
    if mask is None:
        mask = (rst > 0) if relu else torch.ones_like(rst, dtype=torch.bool)
    ms = mask.double() / (1.0 - p)
    res = dict(rst=rst, mag_rst=mag, out=R(rst * ms), mag_out=mag * ms, agg=agg)
    if g is None:
        return res
    G = g.double()
    d, mag_d = R(G * ms), G.abs() * ms
    res.update(d_b=R(d.sum(0)), mag_d_b=mag_d.sum(0))
    if lin_first:
        dz, mag_dz = At(d)[0], At(mag_d)[1]
        dz = R(dz)
        res.update(d_w=R(dz.t() @ H), mag_d_w=mag_dz.t() @ H.abs(), d_h=R(dz @ Wn), mag_d_h=mag_dz @ Wn.abs())
    else:
        dagg, mag_dagg = R(d @ Wn), mag_d @ Wn.abs()
        res.update(d_w=R(d.t() @ agg), mag_d_w=mag_d.t() @ mag_agg, d_h=R(At(dagg)[0]), mag_d_h=At(mag_dagg)[1])
    return res


EXACT_DEGREES = [0, 1, 3, 7, 15, 31] * 2            # deg + 1 a power of two: the reciprocal and every quotient are exact


def exact_case(fin, fout, seed=0, n_extra_src=48):
    """A layer on integers where every rounding point is exact (tests/test_spmm_self_ref.py asserts it: layer_terms(sim=True) equals
    layer_terms(sim=False)): in-degrees EXACT_DEGREES, features and fc_neigh weights in {-1, 0, 1}, bias in {-1, 0, 1}, edge weights
    in {0.5, 1, 2}, and an upstream gradient whose row i is (deg_i + 1) * {-1, 0, 1}, so that the 1 / (deg + 1) of the backward
    cancels.  CPU tensors: indptr, src, dst int64; h [K, fin], w_neigh [fout, fin], bias [fout], ew [B], g [S, fout] bf16."""
    gen = torch.Generator().manual_seed(seed)
    deg = torch.tensor(EXACT_DEGREES, dtype=torch.int64)
    S, B = deg.numel(), int(deg.sum())
    K = S + n_extra_src
    indptr = torch.zeros(S + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    dst = torch.repeat_interleave(torch.arange(S), deg)
    src = torch.randint(0, K, (B,), generator=gen)
    tri = lambda *shape: (torch.randint(0, 3, shape, generator=gen) - 1).to(torch.bfloat16)
    ew = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B,), generator=gen)].to(torch.bfloat16)
    g = tri(S, fout) * (deg + 1).to(torch.bfloat16)[:, None]
    return dict(indptr=indptr, src=src, dst=dst, S=S, K=K, h=tri(K, fin), w_neigh=tri(fout, fin), bias=tri(fout), ew=ew, g=g)


def layer_k(fin, fout, rows, dropout):
    """(k_ulp, k_mag) per tensor of a SAGEConv('gcn') layer with its tail on ``rows`` = max(K, S) block rows, in the units of
    tests/bounds.py, from where the kernels round (both orders of fc_neigh, the library and the tile path alike).  A value stored in
    bf16 between launches costs 1, an aggregation result 1.25 (bounds.SPMM_K's fp32 sum included), the dropout multiply of the
    forward and of the backward 1 each (``dr``), an fp32-accumulated product n_terms * 2^-16 (bounds.dense_k); the last rounding of
    each tensor is k_ulp = 1.
      out:  fc_neigh first: Z (1), the aggregation (1.25), then the bias add rounds last;  aggregation first: the aggregation (1.25), the
            product (1), then the bias add rounds last -- 2.25 + dr + (fin + 1) * 2^-16 either way (fin terms and the bias).
      d_b:  d = dropout's multiply (dr), fp32 sums over chunks of 32 rows and then over the chunk sums, nothing stored in front:
            dr + (rows + rows / 32 + 1) * 2^-16.
      d_w:  fc_neigh first: dZ = A^T d stored (1.25) in front of dZ^T h;  aggregation first: the stored aggregation (1.25) in d^T agg:
            1.25 + dr + (rows + bounds.WGRAD_TARGET) * 2^-16 (the weight-gradient kernel's chunked sum, as bounds.sage_layer_k).
      d_h:  fc_neigh first: dZ stored (1.25), then dZ Wn;  aggregation first: d Wn stored (1), the transposed aggregation rounds last
            (0.25): 1.25 + dr + fout * 2^-16."""
    import bounds
    dr = 1.0 if dropout else 0.0
    return {"out": (1, 2.25 + dr + (fin + 1) * 2.0 ** -16), "d_b": (1, dr + (rows + rows / 32 + 1) * 2.0 ** -16),
            "d_w": (1, 1.25 + dr + (rows + bounds.WGRAD_TARGET) * 2.0 ** -16), "d_h": (1, 1.25 + dr + fout * 2.0 ** -16)}
