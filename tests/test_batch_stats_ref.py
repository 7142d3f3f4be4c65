"""CPU suite: the plain-Python restatement of bliss_batch_stats' rule (tests/batch_stats_ref.py) against hand-computed records."""
import struct
from fractions import Fraction

import batch_stats_ref as ref


def test_constant_sequence_has_zero_spread():
    st = ref.BatchStats()
    for _ in range(3):
        st.push(5)
    assert (st.n, st.m, st.s) == (3, 5.0, 0.0)


def test_two_values_have_the_known_variance():
    st = ref.BatchStats()
    st.push(2)
    st.push(4)
    # mean 3, squared deviations 1 + 1: s = 2, unbiased variance 2
    assert (st.n, st.m, st.s) == (2, 3.0, 2.0) and st.var() == 2.0
    st.push(9)                                  # by hand: m = 3 + 6 / 3 = 5, s = 2 + 6 * 4 = 26
    assert (st.n, st.m, st.s) == (3, 5.0, 26.0) and st.var() == 13.0


def test_first_push_is_the_value_itself_also_zero():
    st = ref.BatchStats()
    st.push(0)
    assert (st.n, st.m, st.s) == (1, 0.0, 0.0)
    st.push(7)
    assert (st.n, st.m, st.s) == (2, 3.5, 24.5)


def test_integers_near_2_31_stay_exact():
    big = 2 ** 31 - 1
    st = ref.BatchStats()
    st.push(big)
    assert st.m == float(big) and int(st.m) == big and st.s == 0.0
    st.push(big - 2)                            # mean big - 1, s = 2: every intermediate is an integer below 2^53
    assert int(st.m) == big - 1 and st.m == float(big - 1) and st.s == 2.0
    st.push(big - 1)
    assert st.m == float(big - 1) and st.s == 2.0


def test_each_statement_is_one_correctly_rounded_operation():
    """The fold against exact rational arithmetic rounded once per statement (float(Fraction) rounds to nearest even)."""
    xs = [117000, 21000, 0, 2 ** 24 + 1, 3, 2 ** 30 + 12345, 99999, 1]
    st, n, m, s = ref.BatchStats(), 0, 0.0, 0.0
    for x in xs:
        st.push(x)
        n += 1
        d_old = float(Fraction(x) - Fraction(m))
        q = float(Fraction(d_old) / n)
        m_new = float(Fraction(m) + Fraction(q))
        d_new = float(Fraction(x) - Fraction(m_new))
        s = float(Fraction(s) + Fraction(float(Fraction(d_old) * Fraction(d_new))))
        m = m_new
        assert (st.n, st.m, st.s) == (n, m, s)


def test_record_bytes_and_clear():
    st = ref.BatchStats()
    for x in (10, 20, 40):
        st.push(x)
    raw = st.to_bytes()
    assert len(raw) == ref.BYTES == 32
    assert struct.unpack("<QddQ", raw) == (3, st.m, st.s, 0)
    back = ref.BatchStats.from_bytes(raw)
    assert (back.n, back.m, back.s) == (st.n, st.m, st.s)
    st.clear()
    assert st.to_bytes() == bytes(32)
