"""Inputs and the fp64 side check of the filter-first engine tests (helper,
not a test; pinned by tests/test_filter_first_ref.py).

The table holds N Gaussian documents of D floats with an int field
num = vid, so the range filter span(count) selects exactly `count`
documents. The truth of a search is the oracle's canonical fp32 FLAT scan
over the matching documents; topk_f64 adds an fp64 order that is only
meaningful, and only used, for the queries it marks as clear.
"""
import numpy as np

U = 2.0 ** -24   # fp32 unit roundoff
N, D, NQ = 6000, 8, 9
COUNTS = (0, 1, 255, 256, 257, 1025, 3000)


def gaussian(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(
        np.float32)


def data(n=N, d=D, nq=NQ, seed=11):
    """(base (n, d), queries (nq, d)), float32"""
    return gaussian(n, d, seed), gaussian(nq, d, seed + 1)


def span(count, n=N):
    """inclusive [lo, hi] of `num` that holds `count` of the values
    0 .. n - 1; a different start for every count. count = 0: a range above
    every value."""
    assert 0 <= count <= n
    if count == 0:
        return n + 10, n + 20
    lo = 7 * count % (n - count + 1)
    return lo, lo + count - 1


def docs_in(lo, hi, live):
    """the ids of `live` (ascending int64 array) with lo <= id <= hi"""
    live = np.asarray(live, dtype=np.int64)
    return live[(live >= lo) & (live <= hi)]


def topk_f64(base, q, k, metric):
    """fp64 brute force over the rows of base -> (ids (nq, kk) int64, best
    first, ties by id; clear (nq,) bool), kk = min(k, rows).

    clear[t]: among query t's best kk + 1 rows every gap between neighbours
    exceeds twice the bound (d + 2) u sum|terms| of a sequential fp32 sum,
    taken at its largest over all rows, so no fp32 evaluation inside that
    bound can change the ids or their order. With no rows it is True."""
    b64 = np.asarray(base, dtype=np.float64)
    q64 = np.asarray(q, dtype=np.float64)
    nq, n, d = q64.shape[0], b64.shape[0], q64.shape[1]
    kk = min(k, n)
    if n == 0:
        return np.empty((nq, 0), np.int64), np.ones(nq, bool)
    ip = metric in ("InnerProduct", "IP")
    ids = np.empty((nq, kk), np.int64)
    clear = np.empty(nq, bool)
    for t in range(nq):
        terms = q64[t] * b64 if ip else (q64[t] - b64) ** 2
        s = -terms.sum(axis=1) if ip else terms.sum(axis=1)
        order = np.lexsort((np.arange(n), s))
        ids[t] = order[:kk]
        bound = (d + 2) * U * np.abs(terms).sum(axis=1).max()
        gaps = np.diff(s[order[:kk + 1]])
        clear[t] = bool((gaps > 2 * bound).all())
    return ids, clear
