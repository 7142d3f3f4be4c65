"""Host-side fixtures for the block build (csrc/sampler.hip: k_block_pass1 -> k_block_scans -> k_block_pass2 -> k_tr_sort_lists):
small graphs built from explicit edge lists through oracle.bliss_oracle.prepare_graph, with planted "special" source nodes
whose out-edges into the seed set are exact -- their ids lie above the range the background sources are drawn from, and they
are no seeds.  A special is (name, [seed index, ...]); a repeated seed index is a parallel edge.  The expected by-source index
of a block is the stable argsort of its ``src`` (``expected_index``).  tests/test_block_build_ref.py checks on the CPU that
every fixture contains what its case is about; tests/test_gpu_block_build_shapes.py drives the samplers over them."""
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

ETA = 0.1
SMALL_S = (31, 32, 33, 64, 65)
LARGE_S = (2048, 2049, 4100)
FRONTIERS = (255, 256, 257, 1023, 1024, 1025)
GROUP = 2048                     # destinations per popcount-prefix round of the bitmap path (64 words)


@dataclass
class Case:
    name: str
    og: object                                  # oracle CSC
    seeds: torch.Tensor                         # int32 [S]
    fanouts: List[int]
    specials: Dict[str, tuple]                  # name -> (node id, planted seed indices in list order)
    uniforms: Optional[List[torch.Tensor]] = None       # drawn cases: one fp32 vector per layer (sampling order)
    info: dict = field(default_factory=dict)

    @property
    def V(self):
        return self.og.num_nodes


def expected_index(src, K):
    """(t_indptr [K + 1], t_edge [B]) a block's by-source index is DEFINED to be: t_edge = stable argsort of src (every source's
    edges in ascending edge index), t_indptr = exclusive prefix of the out-degrees."""
    src = torch.as_tensor(src).long()
    t_edge = torch.sort(src, stable=True).indices
    t_indptr = torch.zeros(K + 1, dtype=torch.int64)
    t_indptr[1:] = torch.cumsum(torch.bincount(src, minlength=K), 0)
    return t_indptr, t_edge


def old_rule_index(src, dst, K):
    """What ranking a list longer than 64 by 'number of members with a smaller destination' over a destination BITMAP leaves
    (the rule k_tr_sort_lists had before parallel edges were supported); -1 = a slot nobody wrote.  For the host test only:
    it shows which fixtures tell the two rules apart."""
    src, dst = np.asarray(src), np.asarray(dst)
    t_indptr, want = expected_index(torch.from_numpy(src), K)
    out = np.full(src.size, -1, dtype=np.int64)
    for j in range(K):
        beg, end = int(t_indptr[j]), int(t_indptr[j + 1])
        members = want[beg:end].numpy()
        if end - beg <= 64:
            out[beg:end] = members
            continue
        uniq = np.unique(dst[members])
        for e in members:
            out[beg + np.searchsorted(uniq, dst[e])] = e
    return torch.from_numpy(out)


def source_list(ob, nid):
    """(edge indices, destinations) of the block edges whose source is global node ``nid``, in edge order."""
    loc = (ob.src_nid == nid).nonzero().flatten()
    if loc.numel() == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    e = (ob.src == int(loc[0])).nonzero().flatten()
    return e, ob.dst[e]


def _csc(src, dst, V, no_loop=()):
    """prepare_graph; with ``no_loop`` the same construction without the self loop of those nodes (prepare_graph gives EVERY
    node one, so it cannot make an empty column)."""
    from oracle import bliss_oracle as bo
    if not len(no_loop):
        return bo.prepare_graph(src, dst, V)
    src, dst = torch.as_tensor(src).long(), torch.as_tensor(dst).long()
    keep = src != dst
    loops = torch.tensor([v for v in range(V) if v not in set(no_loop)])
    src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
    order = torch.sort(dst, stable=True).indices
    indptr = torch.zeros(V + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(dst, minlength=V), 0)
    return bo.CSC(indptr, src[order].to(torch.int32), order.to(torch.int32))


def _build(name, V, seeds, specials, fanouts, gen, n_bg, bg_dst_lo=0, extra=None, no_loop=(), info=None, reserve=0):
    """``specials``: [(name, [seed index, ...])] -> nodes V - len(specials) .. V - 1.  Background: ``n_bg`` random edges with
    sources below every special (and below the ``reserve`` nodes in front of them) and destinations in [bg_dst_lo, that bound).
    ``extra``: (src, dst) edges by node id."""
    first = V - len(specials)
    bg_hi = first - reserve
    assert int(seeds.max()) < bg_hi
    src, dst, ids = [], [], {}
    for i, (nm, dests) in enumerate(specials):
        ids[nm] = (first + i, list(dests))
        src.append(torch.full((len(dests),), first + i))
        dst.append(seeds[torch.tensor(dests)].long())
    if extra is not None:
        src.append(extra[0].long()); dst.append(extra[1].long())
    if n_bg:
        src.append(torch.randint(0, bg_hi, (n_bg,), generator=gen))
        dst.append(torch.randint(bg_dst_lo, bg_hi, (n_bg,), generator=gen))
    og = _csc(torch.cat(src), torch.cat(dst), V, no_loop)
    return Case(name, og, seeds.to(torch.int32), fanouts, ids, info=info or {})


def _subset(gen, S, n, must=()):
    """n distinct seed indices containing ``must``, in a shuffled order."""
    rest = [i for i in torch.randperm(S, generator=gen).tolist() if i not in must][:n - len(must)]
    out = list(must) + rest
    return [out[i] for i in torch.randperm(len(out), generator=gen).tolist()]


# ------------------------------------------------------------------------------------------------ the fixtures
LIST_S = 130
SIMPLE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, LIST_S)


def _list_specials(gen, S=LIST_S):
    sp = [("simple_%d" % n, _subset(gen, S, n)) for n in SIMPLE_LENGTHS]
    d = _subset(gen, S, 64)
    sp.append(("par65", d + [d[10]]))                                   # 64 distinct destinations plus one repeat
    d = _subset(gen, S, 126, must=(0, 31, 32, S - 1))
    sp.append(("par130", d + [0, 31, 32, S - 1]))                       # repeats at 0, at the bitmap's word edge, at S - 1
    sp.append(("par134", list(range(S)) + [0, 31, 32, S - 1]))          # every seed, and the same four repeats
    d = _subset(gen, S, 68, must=(77,))
    sp.append(("triple70", d + [77, 77]))                               # one destination three times
    d = _subset(gen, S, 40)
    sp.append(("doubled80", d + d))                                     # every destination twice
    sp.append(("pair2", [5, 5]))                                        # short path
    d = _subset(gen, S, 32)
    sp.append(("pairs64", d + d))                                       # short path, full: 32 pairs
    return sp


LONG_PARALLEL = ("par65", "par130", "par134", "triple70", "doubled80")


@functools.lru_cache(maxsize=None)
def lists_case(alt=False):
    """S = 130, everything kept.  ``alt``: the same graph with the seed list reversed (another expectation over the same
    buffers: what the replay test alternates with)."""
    gen = torch.Generator().manual_seed(11)
    seeds = torch.randperm(1000, generator=gen)[:LIST_S]
    c = _build("lists", 3000, seeds, _list_specials(gen), [3000], gen, n_bg=4000)
    if alt:
        c = Case("lists_alt", c.og, torch.flip(c.seeds, [0]), c.fanouts,
                 {k: (nid, [LIST_S - 1 - d for d in dests]) for k, (nid, dests) in c.specials.items()})
    return c


@functools.lru_cache(maxsize=None)
def seeds_case(S):
    """S seeds around the bitmap's word (32) and group (2048) edges, everything kept."""
    gen = torch.Generator().manual_seed(100 + S)
    large = S >= GROUP
    V = 6000 if large else 1000
    seeds = torch.randperm(V - 100, generator=gen)[:S]
    sp = [("all", list(range(S)))]
    if large:
        hot = sorted({0, 31, 32, GROUP - 1, min(GROUP, S - 1), S - 1})
        d = _subset(gen, S, 70, must=tuple(hot))
        sp.append(("edge", d + [min(GROUP, S - 1)]))                    # one repeat, at 2048 (at S - 1 where there is no 2048)
    else:
        sp.append(("doubled", list(range(S)) * 2))
        sp.append(("tripled", list(range(S)) * 3))
    return _build("S%d" % S, V, seeds, sp, [V], gen, n_bg=4000, info=dict(S=S))


@functools.lru_cache(maxsize=None)
def frontier_case(E, empty=()):
    """70 seeds whose in-degrees add up to exactly E frontier edges (no background edge ends in a seed), everything kept;
    ``empty``: seed indices whose columns are empty (no self loop, no in-edge)."""
    gen = torch.Generator().manual_seed(300 + E + len(empty))
    S, V = 70, 1500
    seeds = torch.randperm(S, generator=gen)
    live = [i for i in range(S) if i not in empty]
    sp = [("all", list(live)), ("par", list(live) + [live[len(live) // 2]])]
    base = len(live) + sum(len(d) for _, d in sp)
    n_extra = E - base
    assert 0 <= n_extra <= 1300
    xs = torch.arange(n_extra) + 100                                    # one source per extra edge: simple columns
    xd = seeds[torch.tensor([live[i % len(live)] for i in range(n_extra)], dtype=torch.long)]
    return _build("E%d%s" % (E, "_empty" if empty else ""), V, seeds, sp, [V], gen, n_bg=3000, bg_dst_lo=S, extra=(xs, xd),
                  no_loop=tuple(int(seeds[i]) for i in empty), info=dict(E=E, empty=tuple(empty)))


EMPTY_AT = (0, 35, 69)


def empty_case():
    return frontier_case(700, EMPTY_AT)


@functools.lru_cache(maxsize=None)
def sparse_case():
    """A drawn layer that keeps about 5 % of the frontier: 130 seeds with 55 random in-edges each, one seed with 700 more from
    'cold' sources whose planted uniform is 1.0 (never kept: whole spans of its column stay empty); the specials' uniform is
    0.0 (always kept), everybody else's is a seeded random number."""
    from oracle import bliss_oracle as bo
    gen = torch.Generator().manual_seed(21)
    S, V, fan = LIST_S, 4000, 40
    seeds = torch.randperm(1000, generator=gen)[:S]
    d = _subset(gen, S, 64)
    sp = [("par65", d + [d[3]]), ("par134", list(range(S)) + [0, 31, 32, S - 1])]
    cold = torch.arange(3200, 3900)
    xs = torch.cat([torch.randint(1000, 3200, (S * 55,), generator=gen), cold])
    xd = torch.cat([seeds.repeat_interleave(55), seeds[64].repeat(cold.numel())])
    c = _build("sparse", V, seeds, sp, [fan], gen, n_bg=2000, bg_dst_lo=1000, extra=(xs, xd))
    fr = bo.expand_frontier(c.og, c.seeds.long())
    u = torch.rand(fr.nid.numel(), generator=gen)
    u[fr.nid >= V - len(sp)] = 0.0
    u[(fr.nid >= 3200) & (fr.nid < 3900)] = 1.0
    c.uniforms = [u]
    c.info = dict(hub=64, cold=(3200, 3900))
    return c


@functools.lru_cache(maxsize=None)
def two_layer_case():
    """[f, f], everything kept: the second-sampled layer's seeds are the first one's kept nodes (its seed CAPACITY is the first
    layer's kept capacity, not its S).  'deep' is no candidate of the first layer; it points at 70 'mid' nodes, each of which
    has an edge into a seed and so is a seed of the second layer, and twice at one of them."""
    gen = torch.Generator().manual_seed(31)
    S, V = 40, 2000
    seeds = torch.randperm(500, generator=gen)[:S]
    mid = torch.arange(70) + 1000
    deep = V - 2                                                        # reserved: above every background source
    xs = torch.cat([mid, torch.full((71,), deep)])
    xd = torch.cat([seeds[torch.arange(70) % S], mid, mid[17:18]])
    c = _build("two_layer", V, seeds, [("all", list(range(S)))], [V, V], gen, n_bg=2500, extra=(xs, xd), reserve=1)
    c.info = dict(deep=deep, mid=mid, repeat=1017)
    return c


# ------------------------------------------------------------------------------------------------ the oracle's blocks
@functools.lru_cache(maxsize=None)
def _oracle_cached(key, kind):
    from oracle import bliss_oracle as bo
    case = CASES[key]()
    seeds = case.seeds.long()
    torch.manual_seed(0)
    if kind == "bandit":
        w = torch.ones(len(case.fanouts), case.og.num_edges, dtype=torch.bfloat16)
        return bo.sample_blocks_bandit(case.og, seeds, case.fanouts, w, ETA, uniforms=case.uniforms)
    return bo.sample_blocks_ladies(case.og, seeds, case.fanouts, bo.normalized_edata(case.og), uniforms=case.uniforms)


CASES = {"lists": lists_case, "lists_alt": lambda: lists_case(True), "sparse": sparse_case, "two_layer": two_layer_case,
         "empty": empty_case}
CASES.update({"S%d" % S: functools.partial(seeds_case, S) for S in SMALL_S + LARGE_S})
CASES.update({"E%d" % E: functools.partial(frontier_case, E) for E in FRONTIERS})
ALL_KEPT = ["lists"] + ["S%d" % S for S in SMALL_S + LARGE_S] + ["E%d" % E for E in FRONTIERS] + ["empty"]


def oracle_blocks(key, kind="bandit"):
    """(input nodes, seeds, blocks) of the oracle for CASES[key]; shared, never modified."""
    return _oracle_cached(key, kind)


def expected_of(key, kind="bandit"):
    """Per block (model order, like the sampler returns them): (t_indptr, t_edge)."""
    return [expected_index(ob.src, ob.n_src) for ob in oracle_blocks(key, kind)[2]]
