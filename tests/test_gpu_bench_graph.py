"""GPU suite: the benchmark's synthetic graph (bench.chung_lu_graph) is the same in every run with the same seed -- what makes
``bench.py --dump-outputs`` of two builds comparable -- and has bliss_gnn_amd.synth.chung_lu_csc's layout."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.gpu
def test_bench_graph_is_reproducible_with_chung_lu_csc_layout(cuda):
    V, E = 3000, 60000
    ip, ix, ei = bench.chung_lu_graph(V, E, seed=4, device=cuda)
    ip2, ix2, ei2 = bench.chung_lu_graph(V, E, seed=4, device=cuda)
    assert torch.equal(ip, ip2) and torch.equal(ix, ix2) and torch.equal(ei, ei2)
    assert not torch.equal(ix, bench.chung_lu_graph(V, E, seed=5, device=cuda)[1])
    ip, ix, ei = ip.cpu(), ix.cpu().long(), ei.cpu().long()
    assert ip.dtype == torch.int64 and ip[0] == 0 and ip[-1] == ix.numel() == ei.numel()
    deg = ip[1:] - ip[:-1]
    assert bool((deg >= 1).all())
    dst = torch.repeat_interleave(torch.arange(V), deg)
    last = ip[1:] - 1
    loop = torch.zeros(ix.numel(), dtype=torch.bool)
    loop[last] = True
    assert torch.equal(ix[last], torch.arange(V))                                  # one self loop per node, last in its column
    assert not bool((ix[~loop] == dst[~loop]).any())
    key = dst[~loop] * V + ix[~loop]
    assert bool((key[1:] > key[:-1]).all())                                        # dst-major, sources ascending, no duplicates
    Ep = key.numel()
    assert torch.equal(ei[~loop], torch.arange(Ep))                                # edge ids: dst-major, then the self loops
    assert torch.equal(ei[last], Ep + torch.arange(V))
    assert 0.9 * E < ix.numel() - V <= E
