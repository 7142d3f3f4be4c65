"""The batch statistics' rule (include/bliss_gnn.h: bliss_batch_stats, csrc/ledger.hip) restated in plain Python: the running mean
and sum of squared deviations of the input layer's size, one ``push`` per finished train step.  Python floats are IEEE doubles
and every statement below is one rounded operation, so the record agrees with the device's bit for bit."""
import struct

PUSH, CLEAR = 0, 1
BYTES = 32


class BatchStats:
    def __init__(self):
        self.clear()

    def clear(self):
        self.n, self.m, self.s = 0, 0.0, 0.0

    def push(self, x):
        x = float(int(x))                       # (an int32 count: exact in a double)
        self.n += 1
        m_old = self.m
        d_old = x - m_old
        q = d_old / float(self.n)
        self.m = m_old + q
        d_new = x - self.m
        self.s = self.s + d_old * d_new

    def var(self):
        return self.s / (self.n - 1)

    def to_bytes(self):
        """The record in the documented layout: uint64 n, double m, double s, uint64 reserved (zero)."""
        return struct.pack("<QddQ", self.n, self.m, self.s, 0)

    @classmethod
    def from_bytes(cls, raw):
        out = cls()
        out.n, out.m, out.s, _ = struct.unpack("<QddQ", bytes(raw)[:BYTES])
        return out
