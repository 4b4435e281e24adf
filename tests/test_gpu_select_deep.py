"""Deep top-k at kernel level: gk::select_deep and GammaDeepSelector through
their test hooks, against numpy.sort of the u64 keys (an exact total order:
every comparison is array_equal). select_deep runs at the deep sizes it was
written for (1024 < k2 <= 8192) and at the sizes the filter-first plan feeds
it: S = 1, k2 = stride = anything from 1 to 2^20, kout from 1 to 1024."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _distinct(rng, n, same_dist, id_bits=20):
    """n distinct keys with distinct ids; same_dist: one distance for all,
    so the radix select has to go down into the id digits"""
    assert n <= 1 << id_bits
    ids = rng.permutation(1 << id_bits)[:n].astype(np.uint64)
    hi = np.full(n, 0x3F800000, np.uint64) if same_dist else \
        rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    return (hi << np.uint64(32)) | ids


DEEP = [(1, 1025, 1025), (3, 2048, 10), (2, 8192, 8192)]
# what filter-first launches: k2 = ncand_pad = max(topn, candidates rounded
# up to 256), kout = topn. 1 and 7: no candidate at topn 1 and 7; 1280 and
# 262144 + 256: a k2 that is no power of two; 2^20: the engine's cap
SMALL = [(1, 1, 1), (1, 7, 7), (1, 7, 1), (1, 256, 10), (1, 256, 256),
         (1, 512, 1), (1, 1024, 1024), (1, 1024, 1), (1, 1280, 10),
         (3, 256, 10)]
LARGE = [(1, 65536, 10), (1, 262144 + 256, 1024), (1, 1 << 20, 1)]


def _keys(rng, nq, n, same_dist=False):
    bits = 20 if nq * n <= 1 << 20 else 22
    return _distinct(rng, nq * n, same_dist, bits).reshape(nq, n)


def _check(keys, S, k2, kout, ctx):
    from vearch_amd import ktest
    nq = keys.shape[0]
    want = np.sort(keys, axis=1)[:, :kout]
    for stride in (k2, k2 + 3):
        got = ktest.select_deep(keys.reshape(nq, S, k2), kout, stride)
        assert np.array_equal(got, want), (stride, ctx)


@pytest.mark.parametrize("kind", ["random", "same_dist", "short"])
@pytest.mark.parametrize("S,k2,kout", DEEP + SMALL + LARGE)
def test_select_deep(S, k2, kout, kind):
    """short: fewer real keys than kout (5 in all where kout = 10, none
    where kout = 1), the rest EMPTY. Two queries, the regions of the second
    3 keys apart from k2 so that a wrong stride shows."""
    rng = np.random.default_rng(S * k2 + kout)
    nq, n = 2, S * k2
    keys = _keys(rng, nq, n, kind == "same_dist")
    if kind == "short":
        keys[:, min(kout, n) // 2:] = EMPTY
        keys = rng.permuted(keys, axis=1)
    _check(keys, S, k2, kout, kind)


@pytest.mark.parametrize("S,k2,kout", SMALL + LARGE)
def test_select_deep_tail_empty(S, k2, kout):
    """gk::cand_scan's layout: every region holds real keys in [0, m) and
    EMPTY in [m, k2). m = 0 (a row of EMPTY comes back all EMPTY), kout - 1,
    kout, kout + 1 (the select's stop rules on either side of "as many real
    keys as asked for") and k2 - 1."""
    rng = np.random.default_rng(S * k2 + kout + 1)
    nq = 2
    full = _keys(rng, nq, S * k2).reshape(nq, S, k2)
    for m in sorted({0, kout - 1, kout, kout + 1, k2 - 1}):
        if not 0 <= m <= k2:
            continue
        keys = full.copy()
        keys[:, :, m:] = EMPTY
        _check(keys.reshape(nq, S * k2), S, k2, kout, ("m", m))


@pytest.mark.parametrize("S,k2,kout", [c for c in SMALL if c[0] * c[1] <= 256])
def test_select_deep_deep_prefix(S, k2, kout):
    """All keys of a query share their top seven bytes and differ in the
    last one. Where kout is below the number of keys, (7, 1) and (256, 10),
    the radix select walks all eight passes; where it equals it, (1, 1),
    (7, 7) and (256, 256), the select returns in its first pass and the
    shared prefix only reaches the sort."""
    rng = np.random.default_rng(S * k2 + kout + 2)
    nq, n = 2, S * k2
    low = np.stack([rng.permutation(256)[:n] for _ in range(nq)])
    top = rng.integers(0, 1 << 56, size=(nq, 1), dtype=np.uint64)
    keys = (top << np.uint64(8)) | low.astype(np.uint64)
    assert (keys != EMPTY).all()
    _check(keys, S, k2, kout, "deep_prefix")


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("k2", [1025, 4096])
@pytest.mark.parametrize("mult", ["k2-1", "4k2+1", "20k2"])
def test_deep_selector(mult, k2, order):
    """n = k2 - 1: no compaction and a padded result; 4 k2 + 1: one;
    20 k2: several. Ascending keys all pass the threshold until the first
    compaction and none after it; descending keys pass every time."""
    from vearch_amd import ktest
    n = {"k2-1": k2 - 1, "4k2+1": 4 * k2 + 1, "20k2": 20 * k2}[mult]
    keys = np.sort(_distinct(np.random.default_rng(n), n, False))
    want = np.full(k2, EMPTY)
    want[:min(n, k2)] = keys[:k2]
    got = ktest.deep_selector(keys if order == "ascending" else keys[::-1],
                              k2)
    assert np.array_equal(got, want)
