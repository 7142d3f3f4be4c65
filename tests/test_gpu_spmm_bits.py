"""GPU suite (-m gpu): the balanced SpMM traversal (csrc/spmm_walk.cuh) as SAGEConv (bliss_spmm_fwd / _bwd) and as GraphConv
(bliss_gcn_spmm_fwd / _bwd) runs it, bit for bit against outputs recorded from the commit before the two kernels shared one
walk (tests/golden/spmm_bits.npz).

The golden file is written by this module's recorder, ``python tests/test_gpu_spmm_bits.py OUT.npz``: it calls the C ABI only,
so it runs unchanged on the earlier commit.  Inputs are regenerated from NumPy seeds (RandomState: a frozen stream) on the CPU;
only outputs are stored, as uint16 / uint32 views of their bits.  An output of more than RAW_BYTES bytes is stored as one
64-bit digest per row (SHA-256 of the row's bits, cut to 8 bytes): the dim-256 outputs of all variants alone are close to
1 MB of incompressible bits, and the fixture has to stay below tests/golden/engine_kinds.npz.

Cases
  hub/d{1,4,41,256}   40 destinations, 96 sources, EC = 16: row 1 ends exactly on a chunk boundary, row 2 has no edge, row 3
                      (37 edges) is cut twice, the last row is a hub (70 in-edges, cut by more than three boundaries, its last
                      chunk partial); source 5 sends more than 64 edges (the backward's hub).  SAGE forward and backward over
                      mean / sum x weighted / unweighted x bf16 / fp32 out; GCN forward and backward, weighted and unweighted.
  pad/d{4,41}         the same block padded to a capacity (rows, sources and edges past the live counts, their w and h NaN), the
                      live edge count on the device below the bound: the same variants; padded rows must be exact zeros.
  band/{50000,200000} 64 destinations, 512 sources, dim 4: EC = 32 and EC = 64, every row cut many times.
  layout/d4           the hub block with h and gout as column slices 4 bytes off 8-byte alignment: the scalar path."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spmm_bits.npz")
RAW_BYTES = 4096
S_HUB, K_HUB, HUB_SRC = 40, 96, 5
CAP = dict(S=48, K=112, extra_edges=43)
CASES = ["hub/d1", "hub/d4", "hub/d41", "hub/d256", "pad/d4", "pad/d41", "band/50000", "band/200000", "layout/d4"]


# ------------------------------------------------------------------------------------------------- blocks (NumPy, CPU)
def hub_block_np():
    deg = [5, 11, 0, 37] + [1 + (7 * i) % 13 for i in range(4, S_HUB - 1)] + [70]
    indptr = np.cumsum([0] + deg).astype(np.int32)
    B = int(indptr[-1])
    rs = np.random.RandomState(7)
    src = rs.randint(0, K_HUB, size=B).astype(np.int32)
    src[::4] = HUB_SRC
    dst = np.repeat(np.arange(S_HUB, dtype=np.int32), deg)
    # what the cases above promise
    assert 300 <= B <= 400 and B % 16 != 0 and indptr[2] == 16 and indptr[3] == indptr[2]
    hub0, hub1 = int(indptr[S_HUB - 1]), B
    assert hub1 - hub0 > 64 and (hub1 - 1) // 16 - hub0 // 16 >= 3
    assert int((src == HUB_SRC).sum()) > 64
    return indptr, src, dst, S_HUB, K_HUB


def band_block_np(B):
    rs = np.random.RandomState(B)
    dst = np.sort(rs.randint(0, 64, size=B)).astype(np.int32)
    src = rs.randint(0, 512, size=B).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=64))]).astype(np.int32)
    return indptr, src, dst, 64, 512


def by_source(src, K, B):
    """The by-source index of the first B edges: t_edge = edge positions grouped by source (stable), t_indptr their offsets."""
    t_edge = np.argsort(src[:B], kind="stable").astype(np.int32)
    t_indptr = np.concatenate([[0], np.cumsum(np.bincount(src[:B], minlength=K))]).astype(np.int32)
    return t_indptr, t_edge


def pad_block_np(indptr, src, dst, S, K):
    """Capacity padding: rows and sources past the live counts are empty in both indexes, edges past the count point at row 0."""
    B, Sc, Kc = len(src), CAP["S"], CAP["K"]
    Bc = B + CAP["extra_edges"]
    t_indptr, t_edge = by_source(src, K, B)
    grow = lambda a, n: np.concatenate([a, np.full(n - len(a), a[-1] if len(a) else 0, dtype=np.int32)])
    zeros = np.zeros(Bc - B, dtype=np.int32)
    return dict(indptr=grow(indptr, Sc + 1), src=np.concatenate([src, zeros]), dst=np.concatenate([dst, zeros]),
                t_indptr=grow(t_indptr, Kc + 1), t_edge=np.concatenate([t_edge, zeros]), S=Sc, K=Kc, B=Bc, live=(S, K, B))


def exact_block_np(indptr, src, dst, S, K):
    t_indptr, t_edge = by_source(src, K, len(src))
    return dict(indptr=indptr, src=src, dst=dst, t_indptr=t_indptr, t_edge=t_edge, S=S, K=K, B=len(src), live=None)


def bf16_rows(seed, rows, dim, live_rows=None):
    """Standard-normal bf16 [rows, dim] from a frozen stream; rows at or past live_rows are NaN."""
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((rows, dim)).astype(np.float32)).bfloat16()
    if live_rows is not None:
        x[live_rows:] = float("nan")
    return x


# ------------------------------------------------------------------------------------------------- launches (C ABI only)
def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


class Block:
    def __init__(self, spec, dev):
        from bliss_gnn_amd import _lib
        self.S, self.K, self.B = spec["S"], spec["K"], spec["B"]
        for name in ("indptr", "src", "dst", "t_indptr", "t_edge"):
            setattr(self, name, torch.from_numpy(spec[name]).to(dev))
        self.live = spec["live"]
        self.nnz_dev = torch.tensor([spec["live"][2]], dtype=torch.int32, device=dev) if spec["live"] else None
        self.ns = torch.full((self.K,), float("nan"), dtype=torch.float32, device=dev)
        self.nd = torch.full((self.S,), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.bliss_gcn_norms(self.indptr.data_ptr(), self.S, self.t_indptr.data_ptr(), self.K, self.nd.data_ptr(),
                                            self.ns.data_ptr(), _st()), "bliss_gcn_norms")


def launch(blk, conv, backward, w, h, mean=False, out_fp32=False):
    """One SpMM over blk: conv = 'sage' | 'gcn'; h = [K, dim] (forward) or gout = [S, dim] (backward), any row stride.  The output
    and the fp32 partials start as NaN."""
    from bliss_gnn_amd import _lib
    L = _lib.lib
    dim, dev = h.shape[1], h.device
    n_rows = blk.K if backward else blk.S
    out = torch.full((n_rows, dim), float("nan"), dtype=torch.float32 if out_fp32 else torch.bfloat16, device=dev)
    ec = L.bliss_spmm_chunk_edges(blk.B)
    part = torch.full((max(2 * ((blk.B + ec - 1) // ec) * dim, 4),), float("nan"), dtype=torch.float32, device=dev)
    a = (h.data_ptr(), h.stride(0), n_rows, _p(blk.nnz_dev), blk.B, dim)
    o = (out.data_ptr(), out.stride(0))
    if conv == "sage" and not backward:
        rc = L.bliss_spmm_fwd(blk.indptr.data_ptr(), blk.src.data_ptr(), blk.dst.data_ptr(), _p(w), *a, int(mean), *o, int(out_fp32),
                              part.data_ptr(), _st())
    elif conv == "sage":
        rc = L.bliss_spmm_bwd(blk.t_indptr.data_ptr(), blk.t_edge.data_ptr(), blk.src.data_ptr(), blk.dst.data_ptr(), blk.indptr.data_ptr(),
                              _p(w), *a, int(mean), *o, int(out_fp32), part.data_ptr(), _st())
    elif not backward:
        rc = L.bliss_gcn_spmm_fwd(blk.indptr.data_ptr(), blk.src.data_ptr(), blk.dst.data_ptr(), _p(w), blk.ns.data_ptr(), blk.nd.data_ptr(),
                                  *a, *o, part.data_ptr(), _st())
    else:
        rc = L.bliss_gcn_spmm_bwd(blk.t_indptr.data_ptr(), blk.t_edge.data_ptr(), blk.src.data_ptr(), blk.dst.data_ptr(), _p(w),
                                  blk.ns.data_ptr(), blk.nd.data_ptr(), *a, *o, part.data_ptr(), _st())
    _lib.check(rc, "%s spmm backward=%d" % (conv, backward))
    return out


ALL_VARIANTS = [("sage", mean, weighted, f32) for mean in (True, False) for weighted in (True, False) for f32 in (False, True)] + \
               [("gcn", False, weighted, False) for weighted in (True, False)]
ONE_EACH = [("sage", True, True, False), ("gcn", False, True, False)]


def bits(t):
    """The raw bits of a bf16 / fp32 tensor, as a uint16 / uint32 array of the same shape."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def pack(a):
    if a.nbytes <= RAW_BYTES:
        return a
    return np.frombuffer(b"".join(hashlib.sha256(np.ascontiguousarray(row).tobytes()).digest()[:8] for row in a), dtype=np.uint64)


def run_block(blk, dim, variants, seed, dev, sliced=False):
    """Forward and backward of every variant; returns {name: packed bits}.  On a padded block the rows past the live counts
    are checked to be exact zeros here (the recorder checks the earlier commit the same way)."""
    S, K, B = blk.live if blk.live else (blk.S, blk.K, blk.B)
    if sliced:                                                   # columns 2..5 of an 8-wide buffer: 4 bytes off 8-byte alignment
        h, g = bf16_rows(seed, blk.K, 8, K).to(dev)[:, 2:6], bf16_rows(seed + 1, blk.S, 8, S).to(dev)[:, 2:6]
        assert h.data_ptr() % 8 == 4 and g.data_ptr() % 8 == 4 and dim == 4
    else:
        h, g = bf16_rows(seed, blk.K, dim, K).to(dev), bf16_rows(seed + 1, blk.S, dim, S).to(dev)
    w = torch.from_numpy((np.random.RandomState(seed + 2).random_sample(blk.B) + 0.05).astype(np.float32)).bfloat16()
    w[B:] = float("nan")
    w = w.to(dev)
    out = {}
    for conv, mean, weighted, f32 in variants:
        for backward in (False, True):
            o = launch(blk, conv, backward, w if weighted else None, g if backward else h, mean, f32)
            live = K if backward else S
            assert not bool(o[live:].any()), "rows past the live count must be zero"
            name = "%s/%s/%s/%s/%s" % (conv, "bwd" if backward else "fwd", "mean" if mean else "sum", "w" if weighted else "1",
                                       "f32" if f32 else "bf16")
            out[name] = pack(bits(o))
    return out


def run_case(case, dev):
    kind, arg = case.split("/")
    if kind == "band":
        return run_block(Block(exact_block_np(*band_block_np(int(arg))), dev), 4, ONE_EACH, 300, dev)
    dim = int(arg[1:])
    if kind == "pad":
        return run_block(Block(pad_block_np(*hub_block_np()), dev), dim, ALL_VARIANTS, 100 + dim, dev)       # the hub case's inputs, padded
    blk = Block(exact_block_np(*hub_block_np()), dev)
    if kind == "layout":
        return run_block(blk, dim, ONE_EACH, 400, dev, sliced=True)
    return run_block(blk, dim, ALL_VARIANTS, 100 + dim, dev)


def record(dev):
    out = {}
    for case in CASES:
        for name, a in run_case(case, dev).items():
            out[case + "/" + name] = a
    return out


# ------------------------------------------------------------------------------------------------- against the recorded arrays
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_chunk_lengths_of_the_cases():
    from bliss_gnn_amd import _lib
    ec = _lib.lib.bliss_spmm_chunk_edges
    B = len(hub_block_np()[1])
    assert ec(B) == 16 and ec(B + CAP["extra_edges"]) == 16 and ec(50000) == 32 and ec(200000) == 64


@pytest.mark.parametrize("case", CASES)
def test_bits_are_the_recorded_ones(cuda, golden, case):
    got = run_case(case, cuda)
    want = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "/")}
    assert want and sorted(want) == sorted(got), (case, sorted(want), sorted(got))
    for name in sorted(want):
        assert want[name].dtype == got[name].dtype and want[name].shape == got[name].shape, (case, name)
        rows = np.nonzero((want[name] != got[name]).reshape(len(want[name]), -1).any(axis=1))[0]
        assert rows.size == 0, "%s/%s: rows %s differ from the recorded bits" % (case, name, rows[:16].tolist())


def test_padded_live_rows_equal_the_exact_block(golden):
    """The recorded outputs themselves: padding changes nothing on the live rows (where both are stored raw)."""
    n = 0
    for key, pad in golden.items():
        if key.startswith("pad/"):
            exact = golden["hub/" + key[len("pad/"):]]
            if pad.dtype != np.uint64 and exact.dtype != np.uint64:
                assert np.array_equal(pad[:len(exact)], exact), key
                n += 1
    assert n > 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    arrays = record(torch.device("cuda:0"))
    np.savez_compressed(sys.argv[1], **arrays)
    print("recorded", len(arrays), "arrays into", sys.argv[1])
