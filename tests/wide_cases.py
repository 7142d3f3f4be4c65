"""Inputs of the K-panelled product tests (bliss_tile_gemm_wide, bliss_dgrad_wide), built on the CPU so that
tests/test_wide_ref.py can show on the same numbers what the GPU checks of tests/test_gpu_wide_gemm.py catch.

A plain helper module like bounds.py.  The operand conventions are those of tests/test_gpu_sage_dense_edges.py: ``m_bound`` = M +
extra rows of which M exist, every operand row at or past M is ``pad`` (NaN or Inf), gathered ids past M name a table row that is
``pad`` too, repeated and out-of-order ids."""
import torch

BF = torch.bfloat16
NAN, INF = float("nan"), float("inf")
PANEL = 1024                              # columns of one K panel (csrc/sage.hip TG_PANEL, csrc/sage_bwd.hip DG_PANEL)
TABLE_ROWS = 300


def rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def fwd_inputs(K1, N, M, K2=0, gather=False, bias=True, pad=NAN, extra=40, seed=0):
    """CPU operands of one forward launch out = epilogue(A1 W1^T (+ A2 W2^T) + bias), W = [N, K]: a dict with a1 (the rows the launch
    sees, gathered or not, [M + extra, K1]), table / ids when gathered, w1, a2, w2, b, M, mb and n_terms."""
    gen = torch.Generator().manual_seed(1000 * K1 + 10 * N + M + seed)
    mb = M + extra
    table = ids = None
    if gather:
        table = rand(gen, TABLE_ROWS, K1)
        table[TABLE_ROWS - 1] = pad                           # the row the ids beyond the count point at: never loaded
        ids = torch.randint(0, TABLE_ROWS - 1, (mb,), generator=gen)
        ids[: min(M, 8)] = ids[0]                             # repeated ids; random ids are out of order anyway
        ids[M:] = TABLE_ROWS - 1
        a1 = table[ids]
    else:
        a1 = rand(gen, mb, K1)
    a1[M:] = pad
    w1 = rand(gen, N, K1, scale=K1 ** -0.5)
    a2 = w2 = None
    if K2:
        a2, w2 = rand(gen, mb, K2), rand(gen, N, K2, scale=K2 ** -0.5)
        a2[M:] = pad
    b = rand(gen, N) if bias else None
    return dict(a1=a1, table=table, ids=ids, w1=w1, a2=a2, w2=w2, b=b, M=M, mb=mb, K1=K1, K2=K2, N=N, n_terms=K1 + K2 + (1 if bias else 0))


def seam_cols(K):
    """The columns a one-hot probe visits: both ends, both sides of every panel seam the row has."""
    cols = [0, PANEL - 1, PANEL, PANEL + 1, K - 1]
    if K > 2 * PANEL:
        cols += [2 * PANEL - 1, 2 * PANEL]
    return sorted(set(c for c in cols if 0 <= c < K))


def one_hot_rows(K, rows):
    """(A [rows, K] with A[r, cols[r % len(cols)]] = 1 and zeros elsewhere, the column of every row)."""
    cols = seam_cols(K)
    col = torch.tensor([cols[r % len(cols)] for r in range(rows)])
    a = torch.zeros(rows, K, dtype=BF)
    a[torch.arange(rows), col] = 1.0
    return a, col


def seam_fault(a, w, fault):
    """What a broken panel walk computes for out = A W^T on the CPU, W = [N, K], in fp32 like the kernel and rounded once:
    ``drop``: column PANEL never multiplied; ``dup``: column PANEL multiplied twice (both panels stage it); ``panel0``: the second
    panel's rows staged from panel 0 again (columns PANEL + j read column j).  None: the sound walk."""
    A, W = a.float(), w.float()
    K = A.shape[1]
    if fault == "drop":
        A = A.clone()
        A[:, PANEL] = 0
    elif fault == "dup":
        A = A.clone()
        A[:, PANEL] *= 2
    elif fault == "panel0":
        A = A.clone()
        hi = min(K, 2 * PANEL)
        A[:, PANEL:hi] = A[:, : hi - PANEL]
    else:
        assert fault is None
    return (A @ W.t()).to(BF)
