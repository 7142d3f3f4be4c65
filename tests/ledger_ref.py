"""The step ledger's rule (include/bliss_gnn.h, csrc/ledger.hip) restated in NumPy: one record, one ``step`` per finished train
step, the epoch reset, the re-arm, and the record's bytes in the documented layout.  ``fault=`` plants one deviation from the
rule (tests/test_ledger_ref.py shows that each of them changes the record)."""
import struct
from fractions import Fraction

import numpy as np

STEP, RESET_EPOCH, REARM = 0, 1, 2
BF16, F32 = 0, 1
FAULTS = ("fma", "w_after", "ge", "err_overwrite")


def ledger_bytes(L):
    return 80 + 16 * L + 8 * ((12 * L + 7) // 8)


def widen(loss_bits, dtype):
    """The loss scalar (raw bits: 16 for bf16, 32 for fp32) widened exactly to fp64."""
    bits = (int(loss_bits) & 0xFFFF) << 16 if dtype == BF16 else int(loss_bits) & 0xFFFFFFFF
    return np.float64(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def _decay_add(c, w, x, fault):
    if fault == "fma":                                        # one rounding of the exact c * w + x
        return np.float64(float(Fraction(float(c)) * Fraction(float(w)) + Fraction(int(x))))
    if fault == "w_after":
        return np.float64((np.float64(c) + np.float64(x)) * np.float64(w))
    return np.float64(np.float64(c) * np.float64(w)) + np.float64(x)


class Ledger:
    def __init__(self, L):
        assert 1 <= L <= 8
        self.L = L
        self.steps_epoch = self.steps_total = self.nonfinite = 0
        self.loss_last = self.loss_sum = self.cum_out = np.float64(0.0)
        self.first_bad_step = self.first_near_step = -1
        self.err = self.near = 0
        self.cum_nodes, self.cum_edges = [np.float64(0.0)] * L, [np.float64(0.0)] * L
        self.hw_K, self.hw_B, self.hw_E = [0] * L, [0] * L, [0] * L

    def step(self, loss_bits, dtype, counts, caps, w, regrow_at, fault=None):
        """``counts``: int32 [L, 10] (LayerCounts: S E C K B err ...), sampling order; ``caps``: [L, 3] = cap_K, cap_B, cap_E."""
        counts = np.asarray(counts, dtype=np.int32).reshape(self.L, 10)
        caps = np.asarray(caps, dtype=np.int32).reshape(self.L, 3)
        w, regrow_at = np.float64(w), np.float64(regrow_at)
        with np.errstate(all="ignore"):
            x = widen(loss_bits, dtype)
            self.loss_last = x
            self.loss_sum = np.float64(self.loss_sum + x)
            if not np.isfinite(x):
                self.nonfinite += 1
            e, near = 0, False
            for n in range(self.L):
                S, E, _, K, B, err = (int(v) for v in counts[n, :6])
                self.cum_nodes[n] = _decay_add(self.cum_nodes[n], w, K, fault)
                self.cum_edges[n] = _decay_add(self.cum_edges[n], w, B, fault)
                self.hw_K[n], self.hw_B[n], self.hw_E[n] = max(self.hw_K[n], K), max(self.hw_B[n], B), max(self.hw_E[n], E)
                e |= err
                lim_k, lim_b = regrow_at * np.float64(caps[n, 0]), regrow_at * np.float64(caps[n, 1])
                if fault == "ge":
                    near |= bool(np.float64(K) >= lim_k or np.float64(B) >= lim_b)
                else:
                    near |= bool(np.float64(K) > lim_k or np.float64(B) > lim_b)
            self.cum_out = _decay_add(self.cum_out, w, int(counts[0, 0]), fault)
        if e:
            if self.first_bad_step < 0:
                self.first_bad_step = self.steps_total
            self.err = e if fault == "err_overwrite" else self.err | e
        if near:
            if self.first_near_step < 0:
                self.first_near_step = self.steps_total
            self.near = 1
        self.steps_epoch += 1
        self.steps_total += 1

    def reset_epoch(self):
        self.steps_epoch, self.loss_sum, self.nonfinite = 0, np.float64(0.0), 0

    def rearm(self):
        self.near, self.first_near_step = 0, -1

    def to_bytes(self):
        L = self.L
        b = struct.pack("<QQddQdqqiiii", self.steps_epoch, self.steps_total, float(self.loss_last), float(self.loss_sum), self.nonfinite,
                        float(self.cum_out), self.first_bad_step, self.first_near_step, self.err, self.near, L, 0)
        b += struct.pack("<%dd" % (2 * L), *[float(v) for v in self.cum_nodes + self.cum_edges])
        b += struct.pack("<%di" % (3 * L), *(self.hw_K + self.hw_B + self.hw_E))
        return b + b"\0" * (ledger_bytes(L) - len(b))

    def words(self):
        """The record as 8-byte words (NaN-safe comparison: ``loss_last`` may be a NaN)."""
        return np.frombuffer(self.to_bytes(), dtype=np.uint64).copy()

    def as_dict(self):
        return dict(steps_epoch=self.steps_epoch, steps_total=self.steps_total, loss_last=float(self.loss_last),
                    loss_sum=float(self.loss_sum), nonfinite=self.nonfinite, cum_out=float(self.cum_out),
                    first_bad_step=self.first_bad_step, first_near_step=self.first_near_step, err=self.err, near=self.near, n_layers=self.L,
                    cum_nodes=[float(v) for v in self.cum_nodes], cum_edges=[float(v) for v in self.cum_edges],
                    hw_K=list(self.hw_K), hw_B=list(self.hw_B), hw_E=list(self.hw_E))


def planted_steps(L, n_steps=40, regrow_at=0.85, seed=0):
    """``n_steps`` counts records with the edge cases of the rule: sizes exactly at, one below and one above regrow_at * cap (the
    K and B capacities are chosen so that the fp64 product regrow_at * cap is an integer), an err bit on step 17 (and another on 23),
    a NaN and an inf loss.  Returns (caps [L, 3], list of (loss_bits, dtype, counts [L, 10]))."""
    rng = np.random.default_rng(seed)

    def exact(lo, hi):                                                        # a capacity whose fp64 product with regrow_at is an integer
        while True:
            c = 20 * int(rng.integers(lo, hi))
            if float(np.float64(regrow_at) * np.float64(c)).is_integer():
                return c
    caps = np.array([[exact(50, 400), exact(200, 4000), 20 * int(rng.integers(500, 9000))] for _ in range(L)], dtype=np.int32)
    lim = (np.float64(regrow_at) * caps[:, :2].astype(np.float64)).astype(np.int64)
    steps = []
    for t in range(n_steps):
        c = np.zeros((L, 10), dtype=np.int32)
        c[:, 0] = rng.integers(1, 300, L)
        c[:, 1] = rng.integers(0, caps[:, 2] + 1)
        c[:, 3] = rng.integers(0, np.maximum(lim[:, 0] - 1, 1))               # below the warning ...
        c[:, 4] = rng.integers(0, np.maximum(lim[:, 1] - 1, 1))
        c[:, 2] = c[:, 3]
        c[:, 6:] = rng.integers(-5, 5, (L, 4))                                # (words the rule does not read)
        n = t % L
        if t == 9:
            c[n, 3] = lim[n, 0] - 1
        if t == 11:
            c[n, 3] = lim[n, 0]                                               # exactly at: no warning
        if t == 29:
            c[n, 4] = lim[n, 1] + 1                                           # one above: the warning
        if t == 33:
            c[n, 3] = lim[n, 0] + 1
        if t == 17:
            c[n, 5] = 8
        if t == 23:
            c[(n + 1) % L, 5] = 4
        if t % 2:
            dtype, bits = F32, int(np.array([rng.uniform(0.1, 3.0)], dtype=np.float32).view(np.uint32)[0])
        else:
            dtype, bits = BF16, int(np.array([rng.uniform(0.1, 3.0)], dtype=np.float32).view(np.uint32)[0]) >> 16
        if t == 21:
            dtype, bits = BF16, 0x7FC0                                        # NaN
        if t == 26:
            dtype, bits = F32, 0x7F800000                                     # +inf
        steps.append((bits, dtype, c))
    return caps, steps
