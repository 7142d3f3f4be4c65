"""CPU suite: the restatement of the device-side multinomial draw (tests/mn_draw_ref.py) is a correct draw without replacement,
its edge cases are the rule's, and the new entry points refuse bad arguments before any launch."""
import math

import numpy as np
import torch

import mn_draw_ref as ref

SEED = 20240611


def inclusion_counts(draw, n_steps, k=3):
    """``draw(step) -> fp32 keys`` of the 8-candidate case; how often every candidate is among the k drawn."""
    hits = np.zeros(8)
    for t in range(n_steps):
        hits[ref.select(draw(t), k)] += 1
    return hits


def check_inclusion(freq, n_steps, k=3):
    """5 sigma of the binomial variance pi (1 - pi) / n around the exact inclusion probabilities (no measurement involved)."""
    pi = ref.inclusion_probabilities(np.arange(1, 9), k)
    assert abs(pi.sum() - k) < 1e-12
    for j in range(8):
        bound = 5.0 * math.sqrt(pi[j] * (1.0 - pi[j]) / n_steps)
        print("candidate %d: frequency %.4f, exact %.4f, bound %.4f" % (j, freq[j], pi[j], bound))
        assert abs(freq[j] - pi[j]) <= bound, (j, freq[j], pi[j], bound)


P8 = torch.arange(1, 9, dtype=torch.float32).bfloat16()
NID8 = np.arange(8)


def test_inclusion_frequencies_match_successive_sampling():
    for n_steps in (4096, 2048):            # (2048: the run the GPU test repeats on the device with the same seed)
        hits = inclusion_counts(lambda t: ref.keys(P8, NID8, SEED, t, 0), n_steps)
        check_inclusion(hits / n_steps, n_steps)


def test_keyed_uniforms_are_in_the_half_open_unit_interval():
    u = ref.keyed_uniforms(np.arange(100000), SEED, 3, 1)
    assert u.dtype == np.float32 and u.min() > 0.0 and u.max() <= 1.0
    assert np.array_equal(u * np.float32(2.0 ** 24), np.round(u * np.float32(2.0 ** 24)))      # multiples of 2^-24: exact


def test_zero_importance_is_chosen_only_after_every_positive_one():
    p = torch.tensor([0.0, 2.0, 0.0, 1.0, 0.5, 0.0]).bfloat16()
    k = ref.keys(p, np.arange(6), SEED, 0, 0)
    assert np.isposinf(k[[0, 2, 5]]).all() and np.isfinite(k[[1, 3, 4]]).all()
    assert set(ref.select(k, 3).tolist()) == {1, 3, 4}
    assert ref.select(k, 5).tolist()[3:] == [0, 2]                      # then the zero ones, by position
    assert set(ref.select(k, 2).tolist()) < {1, 3, 4}


def test_k_at_least_c_selects_everyone_and_k_zero_nobody():
    k = ref.keys(P8, NID8, SEED, 1, 2)
    assert sorted(ref.select(k, 8).tolist()) == list(range(8))
    assert sorted(ref.select(k, 13).tolist()) == list(range(8))
    assert ref.select(k, 0).size == 0
    assert ref.drawn_mask(k, 0).sum() == 0 and ref.drawn_mask(k, 99).sum() == 8


def test_equal_keys_resolve_by_position():
    p = torch.full((10,), 0.5).bfloat16()
    k = ref.keys(p, np.arange(10), SEED, 0, 0, uniforms=np.full(10, 0.25, dtype=np.float32))
    assert np.unique(k).size == 1
    assert ref.select(k, 4).tolist() == [0, 1, 2, 3]
    k[7] = np.nextafter(k[7], np.float32(0))                             # one key a single ulp smaller: it goes first
    assert ref.select(k, 3).tolist() == [7, 0, 1]
    # u = 1: the key is +0 whatever the sign the quotient carries, and it sorts before every positive key
    z = ref.keys(p, np.arange(10), SEED, 0, 0, uniforms=np.ones(10, dtype=np.float32))
    assert np.array_equal(z.view(np.uint32), np.zeros(10, dtype=np.uint32))


def test_draw_entry_points_refuse_bad_arguments_before_any_launch():
    """bliss_multinomial_draw / bliss_multinomial_select_marked validate on the host (no kernel is launched for a refused call,
    so this runs without a GPU): null pointers, a negative fanout, cap_c <= 0, misaligned scratch, no step where one is read."""
    import ctypes as C
    from bliss_gnn_amd import _lib
    lib, E = _lib.lib, _lib.EINVAL
    buf = (C.c_int64 * 64)()
    p = (C.addressof(buf) + 15) & ~15

    def draw(cand=p, imp=p, counts=p, cap_c=8, fanout=3, uniforms=p, step=p, bump=0, scratch=p, keys=p, drawn=p):
        return lib.bliss_multinomial_draw(cand, imp, counts, cap_c, fanout, uniforms, 1, step, 0, bump, scratch, keys, drawn, 0)
    for name in ("cand", "imp", "counts", "scratch", "keys", "drawn"):
        assert draw(**{name: 0}) == E, name
    assert draw(fanout=-1) == E
    assert draw(cap_c=0) == E and draw(cap_c=-4) == E
    assert draw(scratch=p + 8) == E                                      # scratch not 16-byte aligned
    assert draw(uniforms=0, step=0) == E                                 # keyed mode reads the step
    assert draw(step=0, bump=1) == E                                     # nothing to bump
    assert lib.bliss_multinomial_draw_scratch_bytes(0) == E
    n = lib.bliss_multinomial_draw_scratch_bytes(5000)
    assert n % 16 == 0 and n >= 4 * (2048 + 5)
    assert lib.bliss_multinomial_select_marked(None, 0) == E
    ws = _lib.LayerWs()
    assert lib.bliss_multinomial_select_marked(C.byref(ws), 0) == E      # a workspace without buffers
