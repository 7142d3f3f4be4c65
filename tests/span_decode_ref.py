"""Host-side fixtures of tests/test_gpu_span_decode_shapes.py: hand-built CSC graphs (no self loops are added, so columns can be
empty) whose frontiers put the span-level decode of csrc/sampler.hip (decode_span / span_segments: k_bin_scatter, span_collect
of k_block_pass1 / k_block_pass2) on each of its paths, the host model of which path a span takes, and the oracle's answers.
tests/test_span_decode_ref.py pins on the CPU that every intended shape really occurs and that the oracle accepts the inputs."""
import functools

import torch

from oracle import bliss_oracle as bo

ETA = 0.1
SPAN, WINDOW = 256, 64
KINDS = ("bandit", "ladies", "uniform")        # k_bin_scatter<true>, k_bin_scatter<false>, uniform_nodes (importance_sampling=0)
FRONTIER_LENGTHS = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
DEG_CYCLE = [5, 1, 9, 2, 17, 3, 11, 7]         # ~37 column starts per span: the window always covers
HUB = 33000


class Case:
    def __init__(self, og, seeds, fanouts, info=None):
        self.og, self.seeds, self.fanouts, self.info = og, seeds, fanouts, info or {}

    @property
    def seg_ptr(self):
        return seg_ptr_of(self.og, self.seeds)


def seg_ptr_of(og, seeds):
    s = seeds.long()
    out = torch.zeros(s.numel() + 1, dtype=torch.int64)
    out[1:] = torch.cumsum(og.indptr[s + 1] - og.indptr[s], 0)
    return out


def csc_from_degrees(degs, V, gen, planted=None):
    """CSC with in-degree degs[v] for node v (0 beyond the list), sources drawn with the generator (parallel edges may occur),
    planted[v] = the sources of node v's column given outright; edge ids are a permutation of the CSC positions."""
    deg = torch.zeros(V, dtype=torch.int64)
    deg[:len(degs)] = torch.as_tensor(degs, dtype=torch.int64)
    indptr = torch.zeros(V + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    E = int(indptr[-1])
    indices = torch.randint(0, V, (E,), generator=gen).to(torch.int32)
    for v, srcs in (planted or {}).items():
        assert len(srcs) == int(deg[v])
        indices[int(indptr[v]):int(indptr[v + 1])] = torch.as_tensor(srcs, dtype=torch.int32)
    return bo.CSC(indptr, indices, torch.randperm(E, generator=gen).to(torch.int32))


def span_stats(seg_ptr):
    """Per 256-position span of a frontier: (hint, boundaries, covered).  hint = the last column starting at or before the span's
    first position (what k_seg_scan leaves in span_seg); boundaries = the entries seg_ptr[k], hint < k <= S, that lie inside
    the span; covered = the window of 64 boundaries behind the hint reaches past the span, i.e. fewer than 64 lie inside."""
    S, E = seg_ptr.numel() - 1, int(seg_ptr[-1])
    wbase = torch.arange(0, E, SPAN, dtype=torch.int64)
    hint = torch.searchsorted(seg_ptr[:S].contiguous(), wbase, right=True) - 1
    nb = torch.searchsorted(seg_ptr, wbase + SPAN - 1, right=True) - 1 - hint
    return hint, nb, nb < WINDOW


@functools.lru_cache(maxsize=None)
def frontier_case(E):
    """Seeds 0 .. S-1 whose columns (lengths cycling through DEG_CYCLE, the last one cut) hold exactly E frontier edges."""
    gen = torch.Generator().manual_seed(1000 + E)
    degs, tot = [], 0
    while tot < E:
        d = min(DEG_CYCLE[len(degs) % len(DEG_CYCLE)], E - tot)
        degs.append(d); tot += d
    og = csc_from_degrees(degs, 3000, gen)
    return Case(og, torch.arange(len(degs), dtype=torch.int32), [max(1, E // 6)])


def _structure_degrees():
    """Seed columns in frontier order; every group but the hub's fills whole spans, so the groups do not disturb each other."""
    d, marks = [], {}
    d += [0, 0, 0]                                          # empty columns first
    marks["b63"] = len(d); d += [4] * 64                    # starts at 0, 4 .. 252: 63 boundaries behind the hint -> covered
    marks["b64"] = len(d); d += [3] + [4] * 63 + [1]        # 3, 7 .. 255: exactly 64 -> not covered
    marks["b65"] = len(d); d += [1, 1, 2] + [4] * 63        # 1, 2, 4, 8 .. 252: 65
    marks["b62"] = len(d); d += [8] + [4] * 62              # 8, 12 .. 252: 62 (63 column starts with the one on the first position)
    marks["mixed"] = len(d); d += [1, 3] * 64               # 128 column starts in one span
    marks["run_aligned"] = len(d); d += [0] * 70            # 70 empty columns on a span's first position ...
    marks["hub"] = len(d); d += [HUB]                       # ... then 129 spans of one column
    d += [10]
    marks["run_inside"] = len(d); d += [0] * 70 + [300]     # 70 empty columns in the middle of a span, then a non-empty one
    pos = sum(d)
    d += [SPAN - pos % SPAN]                                # a column ending exactly at a span's end
    marks["ordinary"] = len(d)
    for i in range(900):                                    # past 1024 seeds (k_seg_scan's second round), ordinary spans
        d.append(DEG_CYCLE[i % len(DEG_CYCLE)])
    d += [0] * 5                                            # empty columns last
    return d, marks


@functools.lru_cache(maxsize=None)
def structures_graph():
    gen = torch.Generator().manual_seed(77)
    V = 6000
    degs, marks = _structure_degrees()
    rest = [[0, 2, 6, 1, 0, 12, 3, 4][i % 8] for i in range(V - len(degs))]     # the other nodes' columns: a second layer's seeds
    return csc_from_degrees(degs + rest, V, gen), len(degs), marks


@functools.lru_cache(maxsize=None)
def structures_case(layers=1):
    og, S, marks = structures_graph()
    return Case(og, torch.arange(S, dtype=torch.int32), [1500] if layers == 1 else [1200, 1500], dict(marks=marks))


@functools.lru_cache(maxsize=None)
def single_seed_case():
    """S = 1: the 300-edge column alone (two spans, no boundary but seg_ptr[S])."""
    og, S, marks = structures_graph()
    k = marks["run_inside"] + 70
    assert int(og.indptr[k + 1] - og.indptr[k]) == 300
    return Case(og, torch.tensor([k], dtype=torch.int32), [40])


BIG = 8 * 1024 + 108             # seeds whose column holds the hot source: more records in one bin than 8 x 1024
HOT = 9216                       # a multiple of MAX_BINS: bin 0 whatever n_bins is


@functools.lru_cache(maxsize=None)
def reduce_case():
    """k_bin_reduce: source HOT in the columns of BIG seeds; HOT + 1 once, HOT + 2 five times, HOT + 3 never, and no other
    source congruent to 0 .. 3 modulo 8 -- so for any n_bins >= 8 bin 0 holds more than 8 x 1024 records, bin 1 one, bin 2 five
    and bin 3 none."""
    gen = torch.Generator().manual_seed(78)
    V = HOT + 8
    degs = [2] * BIG
    degs[0] = 3
    for i in range(1, 6):
        degs[i] = 3
    other = (torch.randint(0, HOT // 8, (BIG,), generator=gen) * 8 + 4 + torch.randint(0, 4, (BIG,), generator=gen)).tolist()
    planted = {i: [HOT, other[i]] for i in range(BIG)}
    planted[0] = [HOT, HOT + 1, other[0]]
    for i in range(1, 6):
        planted[i] = [HOT, other[i], HOT + 2]
    # (the other nodes' columns are no part of the frontier: their edges only size the engine's bins -- a bin's capacity is
    # 8192 records plus a share of |E|, and a bin that overflows sends the engine to its atomic passes, without k_bin_reduce)
    og = csc_from_degrees(degs + [40] * (V - BIG), V, gen, planted)
    return Case(og, torch.arange(BIG, dtype=torch.int32), [3000])


CASES = dict(structures=structures_case, single_seed=single_seed_case, reduce=reduce_case)


def case_of(key):
    if isinstance(key, int):
        return frontier_case(key)
    if key == "two_layers":
        return structures_case(2)
    return CASES[key]()


@functools.lru_cache(maxsize=None)
def oracle_blocks(key, kind):
    """(input nodes, blocks) of the oracle for a case and a sampler kind; the generator is seeded as the GPU tests seed it."""
    c = case_of(key)
    og = c.og
    torch.manual_seed(9)
    if kind == "ladies":
        inp, _, blocks = bo.sample_blocks_ladies(og, c.seeds, c.fanouts, bo.normalized_edata(og))
    else:
        ones = torch.ones(len(c.fanouts), og.num_edges, dtype=torch.bfloat16)
        inp, _, blocks = bo.sample_blocks_bandit(og, c.seeds, c.fanouts, ones, ETA, importance_sampling=kind == "bandit")
    return inp, blocks
