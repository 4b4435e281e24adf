"""CPU checks of the numpy references behind tests/test_gpu_kernels.py
(oracle/kernel_refs.py) and of the kernel test hooks' export list. If the
references were wrong the GPU kernel tests would pin the kernels to the
wrong answer, so they are pinned here against plain Python first."""
import random
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from oracle import kernel_refs as kr

KTEST_EXPORTS = [
    "GammaKTestDotsMfma", "GammaKTestSelectFromDots",
    "GammaKTestSelectRowsFull", "GammaKTestArgminRows", "GammaKTestRerank",
    "GammaKTestSortRows", "GammaKTestUnpackKeys", "GammaKTestPqEncode",
    "GammaKTestPqEncodePack4", "GammaKTestFlatStreamScan",
    "GammaKTestIvfpqScan", "GammaKTestIvfflatScan", "GammaKTestPqTablesA",
    "GammaKTestPqTablesB", "GammaKTestPqCwn", "GammaKTestPqSterm",
    "GammaKTestPqStermBuckets", "GammaKTestBucketScatter",
    "GammaKTestResiduals", "GammaKTestRowNorms", "GammaKTestExtractProbe0",
    "GammaKTestRabitqSvalBuckets",
]

F32 = np.finfo(np.float32)


def _special_floats(rng, n, zero):
    """random finite floats over the whole exponent range + the edge
    values; `zero` picks the one signed zero allowed in the row."""
    bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(
        np.uint32)
    v = bits.view(np.float32).copy()
    v = v[np.isfinite(v) & (v != 0)]
    edge = np.array(
        [np.inf, -np.inf, F32.max, -F32.max, F32.tiny, -F32.tiny,
         F32.smallest_subnormal, -F32.smallest_subnormal, 2.0 ** -140,
         -2.0 ** -140, zero, 1.0, 1.0, -3.0], dtype=np.float32)
    v = np.concatenate([v, edge, rng.choice(v, 20)])  # some duplicates
    rng.shuffle(v)
    return v


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_key_order_is_lexsort_dist_then_id(zero):
    rng = np.random.default_rng(7)
    for trial in range(20):
        v = _special_floats(rng, 300, zero)
        ids = rng.integers(0, 2 ** 32, size=v.size, dtype=np.uint64)
        ids[:40] = ids[40:80]  # duplicate ids too
        ids[0], ids[1] = 0, 2 ** 32 - 1
        k_l2 = kr.key_encode(v, ids, ip=False)
        assert np.array_equal(np.argsort(k_l2, kind="stable"),
                              np.lexsort((ids, v)))
        # inner product: descending similarity, ascending id
        k_ip = kr.key_encode(v, ids, ip=True)
        assert np.array_equal(np.argsort(k_ip, kind="stable"),
                              np.lexsort((ids, -v)))
        assert not (k_l2 == kr.EMPTY).any() and not (k_ip == kr.EMPTY).any()


def test_key_orders_negative_zero_first():
    """documented design point: the key image orders -0.0 before +0.0"""
    k = kr.key_encode(np.array([0.0, -0.0], np.float32), [5, 5], ip=False)
    assert k[1] < k[0]


@pytest.mark.parametrize("ip", [False, True])
def test_key_decode_roundtrips_bits(ip):
    rng = np.random.default_rng(11)
    v = np.concatenate([_special_floats(rng, 500, 0.0),
                        np.array([-0.0], np.float32)])
    ids = rng.integers(0, 2 ** 32, size=v.size, dtype=np.uint64)
    d, i = kr.key_decode(kr.key_encode(v, ids, ip), ip)
    assert d.dtype == np.float32 and i.dtype == np.int64
    assert np.array_equal(d.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(i, ids.astype(np.int64))
    d, i = kr.key_decode(np.array([kr.EMPTY], np.uint64), ip)
    assert d[0] == -1.0 and i[0] == -1


def _brute_topk(dist, ids, k2, ip, deleted, seeds):
    """plain Python: sort (dist, id) tuples, no key image involved"""
    rows = [(float(x), int(i)) for x, i in zip(dist, ids)
            if deleted is None or not deleted[int(i)]]
    if seeds is not None:
        sd, si = kr.key_decode(seeds, ip)
        rows += [(float(x), int(i)) for x, i in zip(sd, si) if i >= 0]
    rows.sort(key=lambda t: ((-t[0] if ip else t[0]), t[1]))
    return rows[:k2]


def test_topk_keys_matches_bruteforce_with_ties():
    rnd = random.Random(3)
    rng = np.random.default_rng(3)
    vals = np.array([-2.5, -1.0, 0.0, 0.125, 1.0, 3.0, np.inf, -np.inf],
                    np.float32)
    for trial in range(200):
        n = rnd.randint(1, 40)
        k2 = rnd.randint(1, 50)
        ip = bool(trial & 1)
        dist = rng.choice(vals, n)  # 8 values over up to 40 slots: ties
        base = rnd.randint(0, 100)
        ids = base + rng.permutation(n)
        deleted = None
        if trial % 3 == 0:
            deleted = rng.random(base + n) < 0.3
        seeds = None
        if trial % 4 == 0:
            ns = rnd.randint(1, 10)
            seeds = kr.key_encode(rng.choice(vals, ns),
                                  1000 + rng.permutation(ns), ip)
            seeds = np.concatenate(
                [seeds, np.full(2, kr.EMPTY, np.uint64)])
        got = kr.topk_keys(dist, ids, k2, ip, deleted, seeds)
        assert got.shape == (k2,) and got.dtype == np.uint64
        want = _brute_topk(dist, ids, k2, ip, deleted, seeds)
        gd, gi = kr.key_decode(got, ip)
        assert [(float(a), int(b)) for a, b in
                zip(gd[:len(want)], gi[:len(want)])] == want
        assert (got[len(want):] == kr.EMPTY).all()


def test_bitmap_words():
    dele = np.zeros(70, bool)
    dele[[0, 31, 32, 69]] = True
    w = kr.bitmap_words(dele)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1 << 5]


def test_grid_values_and_exactness_bound():
    g = kr.grid((64, 768), seed=1)
    assert g.dtype == np.float32
    assert np.array_equal(np.unique(g * 8), np.arange(-8, 9))
    # worst case at d = 768: every product / squared difference maximal.
    # In units of 2^-6 all partial sums must stay below 2^24.
    d = 768
    assert d * 1.0 * 64 < 2 ** 24          # dot:  |p| <= 1
    assert d * 4.0 * 64 < 2 ** 24          # L2:   (a-b)^2 <= 4
    assert (2 * d + 2 * d) * 64 < 2 ** 24  # qn + bn + 2|dot| of the GEMM form
    # and the measured sums are integers in those units
    q, b = kr.grid((5, d), 2), kr.grid((7, d), 3)
    dots = kr.dots_f64(q, b)
    assert np.array_equal(dots * 64, np.round(dots * 64))
    assert np.abs(dots).max() * 64 < 2 ** 24
    # the two L2 forms agree exactly on the grid
    l2 = kr.l2_from_dots(kr.dots_exact(q, b), kr.norms_exact(q),
                         kr.norms_exact(b))
    assert np.array_equal(l2, kr.l2_exact(q, b))


def test_l2_from_dots_rejects_off_grid_inputs():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((3, 32)).astype(np.float32)
    b = rng.standard_normal((4, 32)).astype(np.float32)
    with pytest.raises(AssertionError):
        kr.l2_from_dots(kr.dots_f64(q, b), (q.astype(np.float64) ** 2).sum(1),
                        (b.astype(np.float64) ** 2).sum(1))


def test_pq_encode_ref_ties_to_lowest_and_pack4():
    x = kr.grid((50, 8), 5)
    cb = kr.grid((2, 16, 4), 6)
    cb[:, 9] = cb[:, 2]  # duplicated centroid: 9 can never win
    codes = kr.pq_encode_ref(x, cb, 2, 16)
    assert codes.shape == (50, 2) and not (codes == 9).any()
    assert (codes == 2).any()
    p = kr.pack4(codes)
    assert p.shape == (50, 1)
    assert np.array_equal(p[:, 0] & 15, codes[:, 0])
    assert np.array_equal(p[:, 0] >> 4, codes[:, 1])


def _f32(x):
    """round a Python float to fp32 (struct does IEEE round-to-nearest)"""
    import struct
    return struct.unpack("f", struct.pack("f", x))[0]


def test_unpack4_inverts_pack4():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 16, size=(37, 12), dtype=np.uint8)
    p = kr.pack4(codes)
    assert p.shape == (37, 6)
    assert np.array_equal(kr.unpack4(p), codes)
    assert kr.unpack4(np.array([[0xA3]], np.uint8)).tolist() == [[3, 10]]


def test_adc_chain_and_sterm_ref_round_after_every_add():
    """Against a Python loop that rounds to fp32 after each add, on
    Gaussian tables where the order of the adds shows in the bits."""
    rng = np.random.default_rng(11)
    M, ksub, nlist, n = 12, 16, 3, 40
    btab = rng.standard_normal((nlist, M, ksub)).astype(np.float32)
    codes = rng.integers(0, ksub, size=(n, M), dtype=np.uint8)
    start = rng.standard_normal(n).astype(np.float32)
    got = kr.adc_chain(start, btab[1], codes)
    assert got.dtype == np.float32
    for i in range(n):
        acc = float(start[i])
        for m in range(M):
            acc = _f32(acc + float(btab[1, m, codes[i, m]]))
        assert got[i] == acc
    # the chain is order-sensitive here: descending m gives other bits
    rev = kr.adc_chain(start, btab[1][::-1], codes[:, ::-1])
    assert not np.array_equal(got, rev)
    # a scalar start broadcasts
    s0 = kr.adc_chain(np.float32(0.5), btab[0], codes)
    assert np.array_equal(
        s0, kr.adc_chain(np.full(n, 0.5, np.float32), btab[0], codes))
    asg = rng.integers(0, nlist, size=n).astype(np.int32)
    asg[[0, 7]] = -1
    asg[[3, 9]] = nlist
    sv = kr.sterm_ref(btab, codes, asg)
    for i in range(n):
        if not 0 <= asg[i] < nlist:
            assert sv[i] == 0.0
            continue
        acc = 0.0
        for m in range(M):
            acc = _f32(acc + float(btab[asg[i], m, codes[i, m]]))
        assert sv[i] == acc


def test_oracle_chain_wrappers():
    """The array wrappers over the oracle library's serial-fmaf chains:
    shapes, the zero-query identity the pq_cwn reference rests on, and a
    float64 cross-check on grid inputs, where every chain is exact."""
    from oracle import gamma_oracle as go
    d, M, ksub = 24, 4, 16
    q, cent = kr.grid((3, d), 1), kr.grid((5, d), 2)
    cb = kr.grid((M, ksub, d // M), 3)
    a = go.pct1_a_table(q, cb, M, ksub)
    b = go.pct1_b_table(cent, cb, M, ksub)
    t = go.adc_table_ip(q, cb, M, ksub)
    assert a.shape == t.shape == (3, M, ksub) and b.shape == (5, M, ksub)
    cb64 = cb.astype(np.float64)
    dots = np.einsum("qmt,mjt->qmj", q.reshape(3, M, -1).astype(np.float64),
                     cb64)
    cwn = (cb64 * cb64).sum(axis=2)
    assert np.array_equal(t, dots)
    assert np.array_equal(a, cwn[None] - 2.0 * dots)
    assert np.array_equal(b, 2.0 * np.einsum(
        "lmt,mjt->lmj", cent.reshape(5, M, -1).astype(np.float64), cb64))
    # zero query: fmaf(-2, 0, cwn) == cwn exactly, also off the grid
    g = np.random.default_rng(4).standard_normal(
        (M, ksub, d // M)).astype(np.float32)
    z = go.pct1_a_table(np.zeros((1, d), np.float32), g, M, ksub)[0]
    n2 = go.ip_serial(g.reshape(-1, d // M)[:5], g.reshape(-1, d // M)[:5])
    assert np.array_equal(z.ravel()[:5], np.diag(n2))
    assert np.array_equal(go.ip_serial(q, cent), kr.dots_exact(q, cent))


def test_libgamma_exports_kernel_test_hooks():
    """libgamma.so cross-compiles with ktest.cpp and exports every hook
    (the GPU suite cannot run here; a missing symbol must not wait for
    it)."""
    entry.build()
    out = subprocess.check_output(["nm", "-D", entry.SO]).decode()
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in KTEST_EXPORTS if s not in syms]
    assert not missing, f"missing kernel test hooks: {missing}"
    import ctypes
    L = ctypes.CDLL(entry.SO)
    for s in KTEST_EXPORTS:
        getattr(L, s)
