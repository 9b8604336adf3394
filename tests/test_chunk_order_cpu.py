"""The CPU mirror of the pivot's dispatch order (tests/chunk_order_ref.py) against its definition, without a GPU: a bijection of
[0, n) whose residues mod 8 are balanced, the identity for n < 8 and for one column."""
import numpy as np

import chunk_order_ref as CO


def _ns():
    rs = np.random.RandomState(20240817)
    return list(range(71)) + [int(x) for x in rs.randint(71, 300000, size=3000)]


def test_dispatch_index_is_a_balanced_bijection():
    for n in _ns():
        idx = CO.dispatch_index(np.arange(n), n)
        assert np.array_equal(idx, CO.dispatch_index_by_definition(n)), f"n = {n}: the closed form differs from the segments' definition"
        assert np.array_equal(np.sort(idx), np.arange(n)), f"n = {n}: not a bijection of [0, n)"
        if n:
            cnt = np.bincount(idx % CO.COLS, minlength=CO.COLS)
            assert cnt.max() - cnt.min() <= 1, f"n = {n}: residues {cnt.tolist()}"
        if n < CO.COLS:
            assert np.array_equal(idx, np.arange(n)), f"n = {n} < 8 chunks: not the identity"


def test_one_column_is_the_slot_order():
    for n in _ns()[:200]:
        assert np.array_equal(CO.dispatch_index(np.arange(n), n, cols=1), np.arange(n))


def test_a_slice_stays_in_one_column_unless_it_straddles_a_segment_boundary():
    rs = np.random.RandomState(7)
    for _ in range(200):
        S, mc = int(rs.randint(1, 257)), 16
        lens = rs.randint(0, 80, size=S) * (rs.rand(S) > 0.2)
        sl = CO.slot_slices(lens, mc)
        idx = CO.dispatch_index(np.arange(sl.size), sl.size)
        nonempty = int((lens > 0).sum())
        assert len(CO.pairs(idx, sl)) <= nonempty + CO.COLS - 1
        for r in range(CO.COLS):   # within a column a slice's chunks are adjacent rows
            m = idx % CO.COLS == r
            rows, s = idx[m] // CO.COLS, sl[m]
            o = np.argsort(rows)
            assert np.array_equal(rows[o], np.arange(o.size)) and np.all(np.diff(s[o]) >= 0)
