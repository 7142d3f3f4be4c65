"""CPU: the fixtures of tests/span_decode_ref.py hold the shapes they are meant to hold -- read off the host-side seg_ptr with
the model of the kernels' rule (span_stats) -- and the oracle accepts every one of them.  A fixture that silently misses its
shape fails here, not on the GPU."""
import pytest
import torch

import span_decode_ref as sd


def _deg(case):
    sp = case.seg_ptr
    return sp[1:] - sp[:-1]


@pytest.mark.parametrize("E", sd.FRONTIER_LENGTHS)
def test_frontier_lengths(E):
    c = sd.frontier_case(E)
    sp = c.seg_ptr
    assert int(sp[-1]) == E and (_deg(c) > 0).all()
    hint, nb, covered = sd.span_stats(sp)
    assert covered.all() and hint.numel() == (E + sd.SPAN - 1) // sd.SPAN      # the last, partial span takes the span-level path
    if E >= sd.SPAN:
        assert int(nb.max()) >= 30
    for kind in sd.KINDS:
        inp, (ob,) = sd.oracle_blocks(E, kind)
        assert ob.trace["E"] == E and ob.n_dst == c.seeds.numel()


def test_structures_hold_every_shape():
    c = sd.structures_case()
    sp, deg, m = c.seg_ptr, _deg(c), c.info["marks"]
    S = c.seeds.numel()
    hint, nb, covered = sd.span_stats(sp)
    got = set(nb.tolist())
    assert {0, 63, 64, 65} <= got and max(got) > 65                       # none, both sides of the window, far past it
    assert covered[nb == 63].all() and not covered[nb >= 64].any()
    assert int((covered & (nb >= 1)).sum()) >= 10 and int((~covered).sum()) >= 4
    # exactly the planted spans: columns of 4 from a span's first position; 3 + 63 x 4 + 1; 1, 1, 2 + 63 x 4; 8 + 62 x 4; mixed 1 and 3
    # (the column on the span's first position is the hint, not a boundary: 128 column starts are 127 boundaries)
    assert nb[:5].tolist() == [63, 64, 65, 62, 127]
    # spans deep inside the hub: one hint for more than a hundred spans, no boundary
    hub = m["hub"]
    assert int(deg[hub]) == sd.HUB and int((hint == hub).sum()) > 100 and int(((hint == hub) & (nb == 0)).sum()) > 100
    # runs of 64 or more empty columns followed by a non-empty one: on a span's first position and in the middle of a span
    for name in ("run_aligned", "run_inside"):
        k = m[name]
        assert (deg[k:k + 70] == 0).all() and deg[k + 70] > 0
    assert int(sp[m["run_aligned"]]) % sd.SPAN == 0 and int(sp[m["run_inside"]]) % sd.SPAN != 0
    inside = int(sp[m["run_inside"]]) // sd.SPAN
    assert int(nb[inside]) >= 64 and not covered[inside]
    # empty columns first, in the middle and last; a column ending exactly at a span's end; more than one round of k_seg_scan
    assert deg[0] == 0 and deg[-1] == 0 and int(sp[-1]) == int(sp[S - 5])
    assert ((sp[1:] % sd.SPAN == 0) & (deg > 0)).any()
    assert S > 1024 and int(sp[-1]) % sd.SPAN != 0


def test_single_seed_and_reduce_shapes():
    c = sd.single_seed_case()
    assert c.seeds.numel() == 1 and int(c.seg_ptr[-1]) == 300
    _, nb, covered = sd.span_stats(c.seg_ptr)
    assert nb.tolist() == [0, 1] and covered.all()
    r = sd.reduce_case()
    fr = sd.bo.expand_frontier(r.og, r.seeds.long())
    for n_bins in (8, 64, 256, 1024):
        h = torch.bincount(fr.src_g & (n_bins - 1), minlength=n_bins)
        assert int(h[0]) > 8 * 1024 and int(h[1]) == 1 and int(h[2]) == 5 and int(h[3]) == 0


@pytest.mark.parametrize("key", ["structures", "two_layers", "single_seed", "reduce"])
def test_oracle_accepts(key):
    c = sd.case_of(key)
    for kind in (sd.KINDS if key in ("structures", "single_seed") else ("bandit", "ladies") if key == "reduce" else ("bandit",)):
        inp, blocks = sd.oracle_blocks(key, kind)
        assert len(blocks) == len(c.fanouts)
        last = blocks[-1]                                                 # sampled first: the given seeds
        assert last.n_dst == c.seeds.numel() and last.trace["E"] == int(c.seg_ptr[-1])
        for ob in blocks:
            assert 0 < ob.src.numel() and ob.n_src >= ob.n_dst
            assert torch.isfinite(ob.edge_weights.float()).all()
    if key == "two_layers":
        # the second-sampled layer: its seeds are the first one's kept list; partly kept spans on both paths
        inp, blocks = sd.oracle_blocks(key, "bandit")
        sp2 = sd.seg_ptr_of(c.og, blocks[1].src_nid)
        _, nb, covered = sd.span_stats(sp2)
        assert blocks[1].n_src < blocks[1].trace["cand_nid"].numel()      # a real draw, not everything kept
        assert covered.any() and (~covered).any()
