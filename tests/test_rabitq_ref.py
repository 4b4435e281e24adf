"""CPU tests of tests/rabitq_ref.py, the numpy reference the IVFRABITQ GPU
tests compare against: hand-computed tiny cases, the direct against the
decomposed estimator, the degenerate vector, and the metric relation.
(The parameter rejections need CreateTable, which needs Init, which needs
a GPU: they are in test_gpu_rabitq.py.)"""
import numpy as np
import pytest

import rabitq_ref as rr

SQ32 = np.sqrt(32.0)


def _hand_case():
    """d = 32, two lists.
    list 0: c = 0, x = (+1 x16, -1 x16): n2 = l1 = xx = 32, ndp = 1,
            Mul = sqrt(32), A_L2 = 32, A_IP = 0, sval = 0.
    list 1: c = 0.5, x = c + (+2, -1, +2, -1, ...): n2 = 80, l1 = 48,
            ndp = 48 / sqrt(80) / sqrt(32), Mul = sqrt(80) / ndp
            = 80 sqrt(32) / 48, xx = 16 * 6.25 + 16 * 0.25 = 104,
            A_L2 = 80, A_IP = -24, sval = 16 * 0.5 = 8."""
    c = np.zeros((2, 32), dtype=np.float32)
    c[1] = 0.5
    x0 = np.concatenate([np.ones(16), -np.ones(16)]).astype(np.float32)
    x1 = (c[1] + np.tile([2.0, -1.0], 16)).astype(np.float32)
    return c, x0, x1


@pytest.mark.parametrize("ip", [False, True])
def test_hand_computed_encode(ip):
    c, x0, x1 = _hand_case()
    codes, sval = rr.encode(np.stack([x0, x1]), c, ip)
    assert codes.shape == (2, 12) and codes.dtype == np.uint8
    bits, A, Mul = rr.unpack(codes, 32)
    assert np.array_equal(codes[0, :4], [0xFF, 0xFF, 0x00, 0x00])
    assert np.array_equal(codes[1, :4], [0x55] * 4)   # even dims set, LSB
    assert np.array_equal(bits[0], x0 > 0)
    assert np.array_equal(bits[1], np.tile([True, False], 16))
    assert A[0] == (0.0 if ip else 32.0)
    assert A[1] == (-24.0 if ip else 80.0)
    assert Mul[0] == np.float32(SQ32)
    assert Mul[1] == np.float32(80.0 * SQ32 / 48.0)
    assert sval[0] == 0.0 and sval[1] == 8.0
    # the factors are little-endian fp32 behind the bit bytes
    assert np.array_equal(codes[1, 4:8],
                          np.frombuffer(np.float32(A[1]).tobytes(), np.uint8))


@pytest.mark.parametrize("ip", [False, True])
def test_hand_computed_estimate(ip):
    c, x0, x1 = _hand_case()
    fac = [rr.factors(x[None], cc, ip) for x, cc in ((x0, c[0]), (x1, c[1]))]
    bits = [rr.residual_bits(x[None], cc)[1]
            for x, cc in ((x0, c[0]), (x1, c[1]))]
    # q = x0 against x0: qr = x0, dot = 16, sum qr = 0, fd = sqrt(32),
    # pre_L2 = 32 + 32 - 2 sqrt(32) sqrt(32) = 0; IP: pre = 0 + 32 - 64,
    # score = -0.5 (-32 - 32) = 32 = <q, x0>
    s = rr.estimate(x0, c[0], bits[0], fac[0][0], fac[0][1], ip)[0]
    assert abs(s - (32.0 if ip else 0.0)) < 1e-12
    # q = 0 against x1 (list 1): qr = -0.5, dot = -8, sum qr = -16,
    # fd = 0, pre = A + 8: L2 88 (true 104), IP -0.5 (-24 + 8 - 0) = 8
    s = rr.estimate(np.zeros(32, np.float32), c[1], bits[1], fac[1][0],
                    fac[1][1], ip)[0]
    assert abs(s - (8.0 if ip else 88.0)) < 1e-12
    # q = x1 against x1: the estimator is exact on the encoded vector:
    # qr = r, dot = 32, sum = 16, fd = 48 / sqrt(32),
    # pre_L2 = 80 + 80 - 2 (80 sqrt(32) / 48) (48 / sqrt(32)) = 0
    s = rr.estimate(x1, c[1], bits[1], fac[1][0], fac[1][1], ip)[0]
    assert abs(s - (104.0 if ip else 0.0)) < 1e-9


def test_hand_computed_search():
    c, x0, x1 = _hand_case()
    codes, _ = rr.encode(np.stack([x0, x1]), c, False)
    ids = [np.array([7, 3 | -2 ** 63], dtype=np.int64),
           np.array([5], dtype=np.int64)]
    lists = [np.stack([codes[0], codes[0]]), codes[1:2]]
    q = np.stack([x0, x1])
    probes = np.array([[0, 1], [1, -1]], dtype=np.int64)
    od, oi = rr.search(q, c, ids, lists, probes, 3, False)
    assert np.array_equal(oi, [[7, 5, -1], [5, -1, -1]])  # 3 is marked
    # Mul is stored as fp32: 64 * 2^-24 of rounding on a true 0
    assert abs(od[0, 0]) < 1e-5 and abs(od[1, 0]) < 1e-5
    assert od[0, 2] == -1.0
    dead = np.zeros(8, dtype=bool)
    dead[7] = True
    _, oi = rr.search(q, c, ids, lists, probes, 2, False, dead)
    assert np.array_equal(oi, [[5, -1], [5, -1]])
    # ties by id: the same entry under two ids, both metrics
    ids2 = [np.array([9, 2], dtype=np.int64), np.empty(0, np.int64)]
    for ip in (False, True):
        cd, _ = rr.encode(np.stack([x0, x0]), c[0], ip)
        _, oi = rr.search(q[:1], c, ids2, [cd, cd[:0]], probes[:1], 2, ip)
        assert np.array_equal(oi, [[2, 9]])


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("ip", [False, True])
def test_direct_equals_decomposed(D, ip):
    rng = np.random.default_rng(D + ip)
    c = rng.standard_normal(D).astype(np.float32)
    x = (c + 0.5 * rng.standard_normal((200, D))).astype(np.float32)
    q = rng.standard_normal(D).astype(np.float32)
    codes, sval = rr.encode(x, c, ip)
    bits, A, Mul = rr.unpack(codes, D)
    a = rr.estimate(q, c, bits, A, Mul, ip)
    b = rr.estimate_decomposed(q, c, bits, A, Mul, sval, ip)
    assert np.max(np.abs(a - b)) < 1e-9          # fp64 rounding only
    assert np.all(rr.tol(q, c, A, Mul, ip) > 1e-9)


@pytest.mark.parametrize("ip", [False, True])
def test_vector_equal_to_centroid(ip):
    rng = np.random.default_rng(5)
    c = rng.standard_normal(64).astype(np.float32)
    codes, sval = rr.encode(c[None], c, ip)
    bits, A, Mul = rr.unpack(codes, 64)
    assert not bits.any() and sval[0] == 0.0
    assert Mul[0] == 0.0
    q = rng.standard_normal(64).astype(np.float32)
    s = rr.estimate(q, c, bits, A, Mul, ip)
    assert np.isfinite(s).all()
    # with Mul = 0 the estimate is exact: |q - c|^2, or <q, c>
    want = float(q.astype(np.float64) @ c.astype(np.float64)) if ip else \
        float(((q.astype(np.float64) - c) ** 2).sum())
    assert abs(s[0] - want) < 1e-4


def test_coordinate_equal_to_centroid_has_bit_zero():
    c = np.linspace(-1, 1, 32).astype(np.float32)
    x = (c + 1.0).astype(np.float32)
    x[5] = c[5]
    _, bits = rr.residual_bits(x[None], c)
    assert not bits[0, 5] and bits[0].sum() == 31


def test_ip_l2_consistency():
    """A_IP = A_L2 - |x|^2, Mul and the bits do not depend on the metric,
    so pre_IP = pre_L2 - |x|^2 and the IP score estimates <q, x>."""
    rng = np.random.default_rng(11)
    D = 96
    c = rng.standard_normal(D).astype(np.float32)
    x = (c + 0.3 * rng.standard_normal((50, D))).astype(np.float32)
    q = rng.standard_normal(D).astype(np.float32)
    a2, m2, s2 = rr.factors(x, c, False)
    ai, mi, si = rr.factors(x, c, True)
    xx = (x.astype(np.float64) ** 2).sum(axis=1)
    assert np.allclose(ai, a2 - xx, rtol=0, atol=1e-12)
    assert np.array_equal(m2, mi) and np.array_equal(s2, si)
    _, bits = rr.residual_bits(x, c)
    l2 = rr.estimate(q, c, bits, a2, m2, False)
    ip = rr.estimate(q, c, bits, ai, mi, True)
    qq = float((q.astype(np.float64) ** 2).sum())
    assert np.allclose(ip, -0.5 * (l2 - xx - qq), rtol=0, atol=1e-9)
    # on the encoded vector itself the estimate is exact: with q = x,
    # 2 dot - sum r = l1 and Mul fd = n2, so pre_L2 = 0 and IP = |x|^2
    # (up to the one fp32 rounding of r = x - c, which tol() covers)
    for i in range(5):
        j = slice(i, i + 1)
        assert abs(rr.estimate(x[i], c, bits[j], a2[j], m2[j], False)[0]) \
            < rr.tol(x[i], c, a2[j], m2[j], False)[0]
        assert abs(rr.estimate(x[i], c, bits[j], ai[j], mi[j], True)[0]
                   - xx[i]) < rr.tol(x[i], c, ai[j], mi[j], True)[0]


def test_check_row_accepts_and_rejects():
    ids = np.array([4, 9, 2, 7], dtype=np.int64)
    sc = np.array([1.0, 2.0, 3.0, 4.0])
    tl = np.full(4, 0.01)
    rr.check_row([1.0, 2.004], [4, 9], ids, sc, tl, False)
    rr.check_row([4.0, 3.0, 2.0, 1.0, -1.0], [7, 2, 9, 4, -1], ids, sc, tl,
                 True)
    with pytest.raises(AssertionError):      # misses a clearly better one
        rr.check_row([1.0, 3.0], [4, 2], ids, sc, tl, False)
    with pytest.raises(AssertionError):      # score off by more than tol
        rr.check_row([1.0, 2.1], [4, 9], ids, sc, tl, False)
    with pytest.raises(AssertionError):      # too few results
        rr.check_row([1.0, -1.0], [4, -1], ids, sc, tl, False)
    with pytest.raises(AssertionError):      # not a candidate
        rr.check_row([1.0, 2.0], [4, 11], ids, sc, tl, False)
    with pytest.raises(AssertionError):      # unsorted
        rr.check_row([2.0, 1.0], [9, 4], ids, sc, tl, False)
