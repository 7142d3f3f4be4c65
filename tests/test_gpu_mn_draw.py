"""GPU suite (-m gpu): bliss_multinomial_draw through the flat C ABI on tiny arrays, against the CPU restatement of the rule
(tests/mn_draw_ref.py).  Every case checks
  (a) keys: device keys within 1 fp32 ulp of the restatement's -- both sides round ONE fp64 quotient whose log is accurate to
      about an fp64 ulp, so the fp32 results are equal or adjacent; +inf matches exactly;
  (b) selection: ``drawn`` == select(device keys, k) exactly (judged against the device's own keys: no tolerance);
and calls the entry point a second time on the same scratch: same result, i.e. no state is left behind."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mn_draw_ref as ref
from test_mn_draw_ref import NID8, P8, SEED, check_inclusion

pytestmark = pytest.mark.gpu

CHUNK = 1024


class Draw:
    """Device buffers of one flat call, sized by cap_c."""

    def __init__(self, dev, cap_c):
        from bliss_gnn_amd import _lib
        self.lib, self.dev, self.cap_c = _lib, dev, cap_c
        self.counts = torch.zeros(10, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(_lib.lib.bliss_multinomial_draw_scratch_bytes(cap_c)) // 4, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.keys = torch.full((cap_c,), -7.0, dtype=torch.float32, device=dev)
        self.drawn = torch.full((cap_c,), -7, dtype=torch.int32, device=dev)

    def __call__(self, nid, p_bf16, k, uniforms=None, seed=SEED, step=0, layer=0, bump=0, drawn=None):
        n = len(nid)
        assert n <= self.cap_c
        self.counts[2] = n                                                  # LayerCounts::C
        self.step.fill_(step)
        nid_d = torch.zeros(self.cap_c, dtype=torch.int32, device=self.dev)
        nid_d[:n] = torch.as_tensor(np.asarray(nid, dtype=np.int32))
        p_d = torch.zeros(self.cap_c, dtype=torch.bfloat16, device=self.dev)
        p_d[:n] = p_bf16
        u_d = None
        if uniforms is not None:
            u_d = torch.ones(self.cap_c, dtype=torch.float32, device=self.dev)
            u_d[:n] = torch.as_tensor(np.asarray(uniforms, dtype=np.float32))
        drawn = self.drawn if drawn is None else drawn
        st = torch.cuda.current_stream().cuda_stream
        rc = self.lib.lib.bliss_multinomial_draw(nid_d.data_ptr(), p_d.data_ptr(), self.counts.data_ptr(), self.cap_c, int(k),
                                                 0 if u_d is None else u_d.data_ptr(), seed, self.step.data_ptr(), layer, bump,
                                                 self.scratch.data_ptr(), self.keys.data_ptr(), drawn.data_ptr(), st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return self.keys[:n].cpu().numpy(), drawn[:n].cpu().numpy(), int(self.step.item())


def check(d, nid, p_bf16, k, uniforms=None, step=0, layer=0):
    keys, drawn, _ = d(nid, p_bf16, k, uniforms, step=step, layer=layer)
    want = ref.keys(p_bf16, nid, SEED, step, layer, uniforms)
    kb, wb = keys.view(np.uint32).astype(np.int64), want.view(np.uint32).astype(np.int64)
    assert (kb < 0x80000000).all()                                           # non-negative, no -0
    assert np.array_equal(np.isposinf(keys), np.isposinf(want))              # (a) +inf exactly ...
    assert np.abs(kb - wb).max(initial=0) <= 1, np.abs(kb - wb).max()        # ... everything else within one ulp
    assert np.array_equal(drawn, ref.drawn_mask(keys, k)), (len(nid), k)     # (b)
    assert drawn.sum() == min(k, len(nid))
    keys2, drawn2, _ = d(nid, p_bf16, k, uniforms, step=step, layer=layer)   # replay on the same scratch
    assert np.array_equal(keys.view(np.uint32), keys2.view(np.uint32)) and np.array_equal(drawn, drawn2)
    assert int(d.scratch[0]) == 0 and int(d.scratch[8:8 + 2048].abs().sum()) == 0      # ticket and bins are left zero
    return keys, drawn


def rand_p(n, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 3 + 0.01).bfloat16()


@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17])
def test_sizes_and_fanouts(cuda, n):
    d = Draw(cuda, n + 37)                                                   # cap_c > C
    nid = np.random.default_rng(n).permutation(10 * n + 5)[:n]
    p = rand_p(n, n)
    u = np.random.default_rng(n + 1).integers(1, 2 ** 24 + 1, n).astype(np.float32) * np.float32(2.0 ** -24)
    for k in sorted({0, 1, max(n - 1, 0), n, n + 5}):
        check(d, nid, p, k, uniforms=u)
        check(d, nid, p, k)                                                  # and with the keyed uniforms
    assert (d.keys[n:] == -7.0).all() and (d.drawn[n:] == -7).all()           # nothing past C is written


def test_all_keys_equal_resolve_by_position_across_chunks(cuda):
    n, k = 2 * CHUNK + 100, CHUNK + 3
    d = Draw(cuda, n + 8)
    keys, drawn = check(d, np.arange(n), torch.full((n,), 0.75).bfloat16(), k, uniforms=np.full(n, 0.375, dtype=np.float32))
    assert np.unique(keys).size == 1
    assert np.array_equal(np.nonzero(drawn)[0], np.arange(k))


def test_keys_with_common_leading_bits_exercise_every_radix_pass(cuda):
    # p = 1, u = consecutive fp32 values just below 1/e: keys just above 1.0, 0.68 ulp apart on average -- equal or adjacent
    # neighbours, all inside one block of 1024 ulps, so the first two passes see ONE digit and the last one decides
    n = 1200
    u = np.empty(n, dtype=np.float32)
    v = np.float32(math.exp(-1.0))
    for _ in range(4):
        v = np.nextafter(v, np.float32(0))
    for i in range(n):
        u[i] = v
        v = np.nextafter(v, np.float32(0))
    u = u[np.random.default_rng(3).permutation(n)]
    d = Draw(cuda, n + 1)
    p = torch.ones(n).bfloat16()
    for k in (1, 5, 600, n - 1):
        keys, _ = check(d, np.arange(n), p, k, uniforms=u)
    bits = keys.view(np.uint32)
    assert np.unique(bits >> 10).size == 1 and np.unique(bits).size > 256    # the top 22 bits are shared
    # two key values one ulp apart (only the lowest mantissa bit differs), alternating; the threshold falls inside a value
    ua = ub = np.float32(0.25)
    one = torch.ones(1).bfloat16()
    while ref.keys(one, [0], 0, 0, 0, [ub]).view(np.uint32)[0] != ref.keys(one, [0], 0, 0, 0, [ua]).view(np.uint32)[0] + 1:
        ub = np.nextafter(ub, np.float32(0))
    n2 = CHUNK + 1
    u2 = np.where(np.arange(n2) % 2 == 0, ua, ub).astype(np.float32)
    keys2, drawn2 = check(d, np.arange(n2), torch.ones(n2).bfloat16(), n2 // 2 + 3, uniforms=u2)
    b2 = np.unique(keys2.view(np.uint32))
    assert b2.size == 2 and b2[1] - b2[0] == 1
    assert drawn2[0::2].all() and drawn2[1::2].sum() == 2 and drawn2[1] and drawn2[3]     # -log(0.25) is the smaller key


def test_boundary_uniforms_and_zero_importance(cuda):
    n = CHUNK + 77
    d = Draw(cuda, n + 3)
    nid = np.arange(n)
    rng = np.random.default_rng(5)
    u = rng.integers(1, 2 ** 24 + 1, n).astype(np.float32) * np.float32(2.0 ** -24)
    p = rand_p(n, 6)
    # u = 2^-24: the largest finite key of a candidate (24 ln 2 / p)
    small = u.copy(); small[::3] = np.float32(2.0 ** -24)
    for k in (n // 3, n - 5):
        check(d, nid, p, k, uniforms=small)
    # u = 1: key 0, taken first, by position among themselves
    one = u.copy(); one[5::4] = np.float32(1.0)
    keys, drawn = check(d, nid, p, 10, uniforms=one)
    assert (keys.view(np.uint32)[5::4] == 0).all() and np.array_equal(np.nonzero(drawn)[0], np.arange(5, 45, 4))
    # p = 0 for half the candidates, k above the number of positive ones: the zero ones fill up by position
    pz = p.clone(); pz[1::2] = 0
    n_pos = int((pz.float() > 0).sum())
    keys, drawn = check(d, nid, pz, n_pos + 9, uniforms=u)
    assert np.isposinf(keys[1::2]).all() and drawn[0::2].all() and np.array_equal(np.nonzero(drawn[1::2])[0], np.arange(9))
    check(d, nid, pz, n_pos - 4, uniforms=one)


def test_keyed_mode_depends_on_layer_and_step_and_bumps_once(cuda):
    n = 2 * CHUNK + 9
    d = Draw(cuda, n + 64)
    nid = np.random.default_rng(9).permutation(1 << 20)[:n]
    p = rand_p(n, 10)
    seen = []
    for layer in (0, 2):
        for step in (0, 7):
            keys, _ = check(d, nid, p, 300, step=step, layer=layer)
            seen.append(keys.tobytes())
    assert len(set(seen)) == 4
    # bump_step: exactly one increment per call, whatever the number of workgroups; the keys are those of the step read
    for step in (0, 1, 2 ** 40):
        keys, drawn, after = d(nid, p, 300, step=step, layer=1, bump=1)
        assert after == step + 1
        assert np.abs(keys.view(np.uint32).astype(np.int64) - ref.keys(p, nid, SEED, step, 1).view(np.uint32).astype(np.int64)).max() <= 1
    _, _, after = d(nid, p, 300, step=5, bump=0)
    assert after == 5


def test_inclusion_frequencies_on_the_device(cuda):
    """The 8-candidate case of tests/test_mn_draw_ref.py for 2048 consecutive steps drawn on the device (the step bumped by the
    kernel): same 5 sigma bound; the restatement passes it for this seed on the CPU (test_inclusion_frequencies_...)."""
    n_steps = 2048
    d = Draw(cuda, 8)
    d.counts[2] = 8
    nid_d = torch.arange(8, dtype=torch.int32, device=cuda)
    p_d = P8.to(cuda)
    out = torch.zeros(n_steps, 8, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    for t in range(n_steps):
        rc = d.lib.lib.bliss_multinomial_draw(nid_d.data_ptr(), p_d.data_ptr(), d.counts.data_ptr(), 8, 3, 0, SEED, d.step.data_ptr(), 0, 1,
                                              d.scratch.data_ptr(), d.keys.data_ptr(), out[t].data_ptr(), st)
        assert rc == 0
    torch.cuda.synchronize()
    assert int(d.step.item()) == n_steps
    out = out.cpu().numpy()
    assert (out.sum(1) == 3).all()
    # the same draws as the restatement's (keys equal or adjacent: a flipped selection would need a near-tie; count them)
    want = np.stack([ref.drawn_mask(ref.keys(P8, NID8, SEED, t, 0), 3) for t in range(n_steps)])
    print("steps whose selection differs from the restatement's:", int((out != want).any(1).sum()))
    check_inclusion(out.sum(0) / n_steps, n_steps)
