"""CPU suite: what the generator entry points of csrc/rng.hip refuse before any launch or stream creation, and the serial
plans of bliss_rng_prepare (which allocate nothing).  Needs the built library; no device is touched."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from bliss_gnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
# non-null arguments: host words that a refused call never reads
_words = (C.c_int32 * 16)()
P = C.addressof(_words)


def test_one_shot_refuses_null_pointers_and_a_negative_capacity():
    assert L.bliss_mt19937_uniform(None, P, 0, P, 8, None) == _lib.EINVAL
    assert L.bliss_mt19937_uniform(P, None, 0, P, 8, None) == _lib.EINVAL
    assert L.bliss_mt19937_uniform(P, P, 0, None, 8, None) == _lib.EINVAL
    assert L.bliss_mt19937_uniform(P, P, 0, P, -1, None) == _lib.EINVAL


@pytest.mark.parametrize("null_at", range(4))
def test_begin_refuses_a_null_pointer(null_at):
    args = [P, P, P, P]
    args[null_at] = None
    assert L.bliss_rng_stream_begin(*args, 1000, None) == _lib.EINVAL


@pytest.mark.parametrize("cap", [0, -1, -2 ** 31])
def test_begin_refuses_an_empty_stream(cap):
    assert L.bliss_rng_stream_begin(P, P, P, P, cap, None) == _lib.EINVAL


@pytest.mark.parametrize("null_at", range(3))
def test_wait_refuses_a_null_pointer(null_at):
    args = [P, P, P]
    args[null_at] = None
    assert L.bliss_rng_stream_wait(args[0], args[1], args[2], 1, 1000, None) == _lib.EINVAL


def test_chain_refuses_a_short_counts_record():
    for n in (5, 0, -1):
        assert L.bliss_rng_stream_chain(P, P, P, P, 1000, P, n, P, None) == _lib.EINVAL


_NO_GENERATOR = """
import ctypes as C
from bliss_gnn_amd import _lib
L = _lib.lib
w = (C.c_int32 * 16)()
p = C.addressof(w)
assert L.bliss_rng_stream_end(p, p, p, 1000, p, None) == _lib.EINVAL
assert L.bliss_rng_stream_chain(p, p, p, p, 1000, p, 10, p, None) == _lib.EINVAL
assert L.bliss_rng_stream_end(p, p, p, 1000, None, None) == _lib.EINVAL
print("refused")
"""


def test_end_and_chain_refuse_when_no_generator_was_started():
    """`end` and `chain` join the generator this PROCESS started last, so the refusal is that of a process that started none: a
    fresh interpreter that only loads the library (an earlier test of this session may have run generators)."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _NO_GENERATOR], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr


def test_prepare_refuses_an_empty_stream_and_a_null_plan():
    plan = (C.c_int32 * 4)()
    assert L.bliss_rng_prepare(0, plan) == _lib.EINVAL
    assert L.bliss_rng_prepare(-5, plan) == _lib.EINVAL
    assert L.bliss_rng_prepare(1000, None) == _lib.EINVAL


@pytest.mark.parametrize("cap", [1, 624, 29952])
def test_serial_plans(cap, monkeypatch):
    """Serial up to need = ceil(cap / 624) + 1 = 33 + 16 blocks: 29952 = 48 * 624 is the largest such capacity."""
    monkeypatch.delenv("BLISS_RNG_SERIAL", raising=False)
    plan = (C.c_int32 * 4)(-1, -1, -1, -1)
    assert L.bliss_rng_prepare(cap, plan) == 0
    assert tuple(plan) == (33, 0, 0, -(-cap // 624) + 1)
    if cap == 29952:
        assert plan[3] == 49 == 33 + 16
