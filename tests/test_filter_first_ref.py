"""Pins tests/filter_first_ref.py (the inputs and the fp64 side check of the
filter-first engine tests) on the CPU: the range filters select what they
claim, topk_f64 agrees with a pure-Python brute force, its `clear` mark
switches exactly at twice the fp32 bound, and on the inputs the GPU tests
use the mark is set often enough to mean something and agrees with the
oracle's canonical fp32 scan wherever it is set."""
import math

import numpy as np
import pytest

import filter_first_ref as ffr
import oracle as orc


def test_span_selects_exactly_count():
    nums = np.arange(ffr.N)
    starts = set()
    for c in ffr.COUNTS:
        lo, hi = ffr.span(c)
        assert ((nums >= lo) & (nums <= hi)).sum() == c
        assert lo <= hi
        starts.add(lo)
        assert np.array_equal(ffr.docs_in(lo, hi, nums), nums[lo:hi + 1])
    assert len(starts) == len(ffr.COUNTS)
    assert ffr.docs_in(3, 9, [1, 3, 4, 9, 12]).tolist() == [3, 4, 9]


@pytest.mark.parametrize("metric", ["L2", "InnerProduct"])
def test_topk_f64_against_pure_python(metric):
    base, q = ffr.data(40, 4, 3, seed=5)
    base[7] = base[2]  # an exact tie: the lower id first
    ids, _ = ffr.topk_f64(base, q, 40, metric)
    for t in range(3):
        rows = []
        for i in range(40):
            x, y = q[t].astype(float).tolist(), base[i].astype(float).tolist()
            if metric == "L2":
                s = math.fsum((a - b) ** 2 for a, b in zip(x, y))
            else:
                s = -math.fsum(a * b for a, b in zip(x, y))
            rows.append((s, i))
        want = [i for _, i in sorted(rows)]
        # numpy's pairwise fp64 sum against fsum: equal order except where
        # two scores are within an fp64 rounding, which only the tie is
        assert ids[t].tolist() == want
        assert want.index(2) + 1 == want.index(7)
    ids3, _ = ffr.topk_f64(base, q, 3, metric)
    assert np.array_equal(ids3, ids[:, :3])


def test_clear_switches_at_twice_the_bound():
    """rows (x, 0, 0, 0) against q = 0: the L2 score is x^2. The bound is
    (4 + 2) u max(x^2) = 24 u, twice that 2.861e-6."""
    q = np.zeros((1, 4))
    two_b = 2 * 6 * ffr.U * 4.0

    def base(g, third=2.0):
        b = np.zeros((3, 4))
        b[:, 0] = [1.0, math.sqrt(1.0 + g), third]
        return b
    for g, want in ((two_b * 1.01, True), (two_b * 0.99, False)):
        ids, clear = ffr.topk_f64(base(g), q, 2, "L2")
        assert ids.tolist() == [[0, 1]] and clear.tolist() == [want]
    # the row just outside the result counts: k = 1 looks at two rows only
    tie = base(0.5, math.sqrt(1.5))
    assert ffr.topk_f64(tie, q, 1, "L2")[1].tolist() == [True]
    assert ffr.topk_f64(tie, q, 2, "L2")[1].tolist() == [False]
    # fewer rows than k, and none
    ids, clear = ffr.topk_f64(base(0.5)[:2], q, 10, "L2")
    assert ids.tolist() == [[0, 1]] and clear.all()
    ids, clear = ffr.topk_f64(np.zeros((0, 4)), q, 10, "L2")
    assert ids.shape == (1, 0) and clear.all()


@pytest.mark.parametrize("d", [ffr.D, 32])
@pytest.mark.parametrize("metric", ["L2", "InnerProduct"])
def test_inputs_of_the_gpu_tests(metric, d):
    """At topn 10 most queries of every candidate count are clear, and on
    those the oracle's canonical fp32 scan returns the fp64 ids. d = 32 is
    the IVFRABITQ table's dimension."""
    base, q = ffr.data(d=d)
    assert base.shape == (ffr.N, d) and q.shape == (ffr.NQ, d)
    assert base.dtype == q.dtype == np.float32
    for c in ffr.COUNTS:
        lo, hi = ffr.span(c)
        docs = ffr.docs_in(lo, hi, np.arange(ffr.N))
        ids, clear = ffr.topk_f64(base[docs], q, 10, metric)
        assert ids.shape == (ffr.NQ, min(10, c))
        if c == 0:
            continue
        assert clear.sum() >= 6 and clear[:5].sum() >= 3, (c, clear)
        _, oi = orc.flat_search(base[docs], q, 10, metric)
        for t in np.flatnonzero(clear):
            assert oi[t, :ids.shape[1]].tolist() == ids[t].tolist()
            assert (oi[t, ids.shape[1]:] == -1).all()
