"""Pins tests/binary_ref.py (the numpy reference the BINARYIVF GPU tests
compare against) to a brute-force pure-Python implementation that counts
bits with bin(x).count("1"). CPU only."""
import numpy as np
import pytest

import binary_ref as br


def _py_hamming(a, b):
    ia = int.from_bytes(bytes(a), "little")
    ib = int.from_bytes(bytes(b), "little")
    return bin(ia ^ ib).count("1")


def _py_matrix(a, b):
    return np.array([[_py_hamming(x, y) for y in b] for x in a],
                    dtype=np.int64).reshape(len(a), len(b))


def _py_topk(q, cands, k):
    """cands: list of (id, code). -> (dists, ids) padded with -1.0 / -1"""
    rows = sorted((_py_hamming(q, c), i) for i, c in cands)[:k]
    d = [float(h) for h, _ in rows] + [-1.0] * (k - len(rows))
    i = [i for _, i in rows] + [-1] * (k - len(rows))
    return np.array(d, dtype=np.float32), np.array(i, dtype=np.int64)


def _special(nbytes, rng):
    """all-zero, all-one, a duplicated pair and random rows"""
    r = rng.integers(0, 256, size=(5, nbytes), dtype=np.uint8)
    return np.concatenate([np.zeros((1, nbytes), np.uint8),
                           np.full((1, nbytes), 255, np.uint8),
                           r, r[2:3], r[2:3]])


@pytest.mark.parametrize("nbytes", [4, 12, 32])
def test_hamming_random_and_special(nbytes):
    rng = np.random.default_rng(nbytes)
    a = np.concatenate([_special(nbytes, rng),
                        rng.integers(0, 256, (6, nbytes), dtype=np.uint8)])
    b = np.concatenate([_special(nbytes, rng),
                        rng.integers(0, 256, (9, nbytes), dtype=np.uint8)])
    got = br.hamming(a, b)
    assert got.dtype == np.int64
    assert np.array_equal(got, _py_matrix(a, b))
    # all-zero vs all-one is the full dimension, a row against itself 0
    assert got[0, 1] == nbytes * 8 and got[1, 0] == nbytes * 8
    assert np.array_equal(np.diag(br.hamming(a, a)), np.zeros(len(a)))


def test_assign_and_coarse_ties_to_lowest_list():
    rng = np.random.default_rng(5)
    cent = rng.integers(0, 256, (12, 8), dtype=np.uint8)
    cent[7] = cent[3]              # duplicated centroids: ties
    cent[9] = cent[3]
    x = np.concatenate([rng.integers(0, 256, (20, 8), dtype=np.uint8),
                        cent[3:4], cent[9:10]])
    h = _py_matrix(x, cent)
    want = np.array([min(range(12), key=lambda j: (h[i, j], j))
                     for i in range(len(x))])
    assert np.array_equal(br.assign(x, cent), want)
    assert br.assign(cent[9:10], cent)[0] == 3
    for nprobe in (1, 5, 12):
        d, l = br.coarse(x, cent, nprobe)
        assert d.dtype == np.float32 and l.dtype == np.int64
        for i in range(len(x)):
            order = sorted(range(12), key=lambda j: (h[i, j], j))[:nprobe]
            assert l[i].tolist() == order
            assert d[i].tolist() == [float(h[i, j]) for j in order]


def _lists(rng, sizes, nbytes, id_space=4096):
    perm = rng.permutation(id_space)
    ids, codes, pos = [], [], 0
    for n in sizes:
        ids.append(perm[pos:pos + n].astype(np.int64))
        codes.append(rng.integers(0, 256, (n, nbytes), dtype=np.uint8))
        pos += n
    return ids, codes


def _py_search(q, ids, codes, probes, k, deleted=None):
    od, oi = [], []
    for r in range(len(q)):
        cands = []
        for ln in probes[r]:
            if ln < 0 or ln >= len(ids):
                continue
            for i, c in zip(ids[ln].tolist(), codes[ln]):
                if i < 0 or (deleted is not None and deleted[i]):
                    continue
                cands.append((i, c))
        d, i = _py_topk(q[r], cands, k)
        od.append(d)
        oi.append(i)
    return np.stack(od), np.stack(oi)


@pytest.mark.parametrize("k", [1, 7, 200])
def test_search_random(k):
    """random lists, an empty list, invalid probes, delete marks and a
    bitmap; k = 200 exceeds the candidates of some queries"""
    rng = np.random.default_rng(11 + k)
    ids, codes = _lists(rng, [0, 1, 30, 64, 90], 8)
    ids[3][::3] |= np.int64(-2 ** 63)       # bit-63 delete marks
    deleted = rng.random(4096) < 0.2
    q = rng.integers(0, 256, (6, 8), dtype=np.uint8)
    probes = np.array([[0, 1, 2], [4, -1, 3], [9, 2, 4], [0, 0, -1],
                       [3, 4, 2], [1, 5, 3]], dtype=np.int64)
    for dl in (None, deleted):
        gd, gi = br.search(q, ids, codes, probes, k, dl)
        wd, wi = _py_search(q, ids, codes, probes, k, dl)
        assert gd.dtype == np.float32 and gi.dtype == np.int64
        assert np.array_equal(gd, wd) and np.array_equal(gi, wi)
    # query 3 probes only the empty list and an invalid one
    assert np.all(gi[3] == -1) and np.all(gd[3] == -1.0)


def test_search_all_tied_orders_by_id():
    rng = np.random.default_rng(3)
    one = rng.integers(0, 256, (1, 16), dtype=np.uint8)
    ids = [rng.permutation(500)[:100].astype(np.int64)]
    codes = [np.repeat(one, 100, axis=0)]
    q = rng.integers(0, 256, (2, 16), dtype=np.uint8)
    probes = np.zeros((2, 1), dtype=np.int64)
    gd, gi = br.search(q, ids, codes, probes, 10)
    for r in range(2):
        assert gi[r].tolist() == sorted(ids[0].tolist())[:10]
        assert np.all(gd[r] == _py_hamming(q[r], one[0]))
    wd, wi = _py_search(q, ids, codes, probes, 10)
    assert np.array_equal(gd, wd) and np.array_equal(gi, wi)


def test_brute_matches_python():
    rng = np.random.default_rng(8)
    base = np.concatenate([_special(8, rng),
                           rng.integers(0, 256, (40, 8), dtype=np.uint8)])
    q = np.concatenate([base[:3], rng.integers(0, 256, (3, 8),
                                               dtype=np.uint8)])
    deleted = np.zeros(len(base), dtype=bool)
    deleted[::4] = True
    for dl in (None, deleted):
        for k in (1, 10, len(base) + 5):
            gd, gi = br.brute(q, base, k, dl)
            wd, wi = _py_search(
                q, [np.arange(len(base), dtype=np.int64)], [base],
                np.zeros((len(q), 1), dtype=np.int64), k, dl)
            assert np.array_equal(gd, wd) and np.array_equal(gi, wi)
