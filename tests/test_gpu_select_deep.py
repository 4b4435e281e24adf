"""Deep top-k at kernel level: gk::select_deep and GammaDeepSelector through
their test hooks, against numpy.sort of the u64 keys (an exact total order:
every comparison is array_equal)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _distinct(rng, n, same_dist):
    """n distinct keys with distinct ids; same_dist: one distance for all,
    so the radix select has to go down into the id digits"""
    ids = rng.permutation(1 << 20)[:n].astype(np.uint64)
    hi = np.full(n, 0x3F800000, np.uint64) if same_dist else \
        rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    return (hi << np.uint64(32)) | ids


@pytest.mark.parametrize("kind", ["random", "same_dist", "short"])
@pytest.mark.parametrize("S,k2,kout", [(1, 1025, 1025), (3, 2048, 10),
                                       (2, 8192, 8192)])
def test_select_deep(S, k2, kout, kind):
    """short: fewer real keys than kout (5 in all where kout = 10), the rest
    EMPTY. Two queries, the regions of the second 3 keys apart from k2 so
    that a wrong stride shows."""
    from vearch_amd import ktest
    rng = np.random.default_rng(S * k2 + kout)
    nq, n = 2, S * k2
    keys = _distinct(rng, nq * n, kind == "same_dist").reshape(nq, n)
    if kind == "short":
        keys[:, min(kout, n) // 2:] = EMPTY
        keys = rng.permuted(keys, axis=1)
    want = np.sort(keys, axis=1)[:, :kout]
    for stride in (k2, k2 + 3):
        got = ktest.select_deep(keys.reshape(nq, S, k2), kout, stride)
        assert np.array_equal(got, want), (stride, kind)


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
