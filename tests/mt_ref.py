"""MT19937 as at::mt19937 steps it (ATen/core/MT19937RNGEngine.h), in plain numpy: the CPU reference of csrc/rng.hip.
Pinned against torch's own generator by test_mt_ref.py; no GPU and no library is involved.

A block is the generator's 624 state words.  torch regenerates the block (next_state) when a draw finds none left
unread, then hands out the tempered words in index order; torch.rand keeps the low 24 bits of each."""
import numpy as np

N, M = 624, 397
H = N - M                                    # 227: stages A and B of next_state have this many words, stage C has 170
_UPPER, _LOWER, _MATRIX_A = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)


def _twist(u, v):
    y = (u & _UPPER) | (v & _LOWER)
    return (y >> np.uint32(1)) ^ np.where(v & np.uint32(1), _MATRIX_A, np.uint32(0))


def _next_block(od):
    """at::mt19937::next_state, out of place.  The words of a stage depend only on the old block and on earlier stages:
    A: k in [0, 227) reads od[k + 397];  B: k in [227, 454) reads nw[k - 227] (stage A);  C: k in [454, 624) reads
    nw[k - 227] (stage B), and its last word pairs od[623] with nw[0]."""
    od = np.asarray(od, dtype=np.uint32)
    nw = np.zeros(N, dtype=np.uint32)
    nw[:H] = od[M:] ^ _twist(od[:H], od[1:H + 1])
    nw[H:2 * H] = nw[:H] ^ _twist(od[H:2 * H], od[H + 1:2 * H + 1])
    nw[2 * H:N - 1] = nw[H:N - 1 - H] ^ _twist(od[2 * H:N - 1], od[2 * H + 1:N])
    nw[N - 1] = nw[N - 1 - H] ^ _twist(od[N - 1:N], nw[0:1])[0]
    return nw


def temper(words):
    y = np.asarray(words, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def uniform(words):
    """at::uniform_real_distribution<float>: the low 24 bits of the tempered word, times 2^-24 (exact in float32)."""
    return (temper(words) & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)


def fields(state_bytes):
    """torch.get_rng_state() of the CPU generator -> (words uint32[624], left, next).  The legacy layout: int32 `left` at
    byte 8, int64 `next` at byte 16, the 624 state words as uint64 from byte 24."""
    raw = np.asarray(state_bytes, dtype=np.uint8).tobytes()
    left = int(np.frombuffer(raw, dtype="<i4", count=1, offset=8)[0])
    nxt = int(np.frombuffer(raw, dtype="<i8", count=1, offset=16)[0])
    wide = np.frombuffer(raw, dtype="<u8", count=N, offset=24)
    assert int(wide.max()) < 2 ** 32
    return wide.astype(np.uint32), left, nxt


def pack626(words, left, nxt):
    """The device's generator state (int32[626]): 624 state words, left, next."""
    s = np.empty(N + 2, dtype=np.int32)
    s[:N] = np.asarray(words, dtype=np.uint32).view(np.int32)
    s[N], s[N + 1] = left, nxt
    return s


def raw_blocks(words, k):
    """uint32[k + 1, 624]: block 0 = the state at entry, block i >= 1 = the i-th regenerated state."""
    out = np.empty((k + 1, N), dtype=np.uint32)
    out[0] = words
    for i in range(k):
        out[i + 1] = _next_block(out[i])
    return out


def avail_of(left):
    """Numbers still unread in the current block."""
    return min(max(left - 1, 0), N)


def blocks_for(avail, n):
    """Regenerated blocks that n draws reach when `avail` numbers of the entry block are unread."""
    return 0 if n <= avail else -(-(n - avail) // N)


def draws(blocks, left, nxt, n):
    """The n numbers torch.rand(n) returns from the state (blocks[0], left, next)."""
    avail = avail_of(left)
    stream = np.concatenate([blocks[0][nxt:nxt + avail], blocks[1:].reshape(-1)])
    assert n <= stream.size
    return uniform(stream[:n])


def state_after(blocks, left, nxt, n):
    """(words, left, next) after n draws from the state (blocks[0], left, next)."""
    avail = avail_of(left)
    if n <= avail:
        return blocks[0], left - n, nxt + n
    b, t = 1 + (n - avail - 1) // N, (n - avail - 1) % N + 1
    return blocks[b], N + 1 - t, t
