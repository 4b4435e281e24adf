"""Kernel-level parity tests: each HIP kernel entry of csrc/kernels.h is
driven directly through the kernel test hooks (vearch_amd/ktest.py) on
tiny device arrays and compared with a plain numpy reference
(oracle/kernel_refs.py, itself pinned on the CPU by test_kernel_refs.py).

Comparisons are exact (u64 keys, fp32 bit patterns, ints). The kernels
whose accumulation order is NOT the contract (MFMA GEMM, shuffle-tree
scans) run on grid inputs (values i/8, |i| <= 8), where every order is
exact in fp32, so they too must match a float64 reference bit for bit;
ties are everywhere on such inputs. Kernels whose order IS the contract
(rerank) run on Gaussian data against the oracle's sequential-fmaf
distances. No NaN inputs, no shape outside a kernel's documented
contract (d % 4 == 0, k2 <= 1024, select_rows_full ncols <= 8192,
sort_rows ncand <= 2048, ksub in {16, 256})."""
import itertools

import numpy as np
import pytest

import oracle as orc
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(kr.EMPTY)


@pytest.fixture(scope="module")
def kt():
    from vearch_amd import ktest
    return ktest


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def padded(mat, pad, fill=99.0):
    """(nq, ncols) -> device (nq, ncols + pad): the row stride becomes
    ncols + pad; the pad columns hold a value that must never be read."""
    buf = np.full((mat.shape[0], mat.shape[1] + pad), fill, np.float32)
    buf[:, :mat.shape[1]] = mat
    return dev(buf)


# ================================================================ dots_mfma
DOT_NQ = [1, 15, 17, 63, 64, 65, 129, 200]
DOT_N = [1, 15, 17, 63, 64, 127, 129, 300]


@pytest.mark.parametrize("d", [4, 28, 32, 36, 100])
def test_dots_mfma_grid_exact(kt, d):
    """Full nq x n cross product per d: the simple kernel (nq < 64 or
    n < 64) and the LDS-tiled kernel (both >= 64) at sizes below, at and
    off the 16/64/128 tile edges and with d off the BK=32 K tile. Grid
    inputs -> equal to the float64 product bit for bit."""
    Q = kr.grid((200, d), seed=100 + d)
    B = kr.grid((300, d), seed=200 + d)
    want = kr.dots_exact(Q, B)
    Qd, Bd = dev(Q), dev(B)
    for nq, n in itertools.product(DOT_NQ, DOT_N):
        got = kt.dots_mfma(Qd[:nq], Bd[:n]).cpu().numpy()
        assert np.array_equal(bits(got), bits(want[:nq, :n])), (nq, n, d)


def test_dots_mfma_gaussian_bound_and_kernel_identity(kt):
    """Gaussian inputs: (a) the derived error bound
    |out - f64| <= 2 d u sum|a_i||b_i| (gamma_d, doubled for unfused
    multiplies; u = 2^-24); (b) the identity kernels.hip claims — the
    tiled kernel's values are bit-identical to the simple kernel's, so a
    query gets the same coarse dots in a batch of 63 and in a batch of
    200."""
    nq, n, d = 200, 300, 100
    rng = np.random.default_rng(12)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    B = rng.standard_normal((n, d)).astype(np.float32)
    Qd, Bd = dev(Q), dev(B)
    tiled = kt.dots_mfma(Qd, Bd).cpu().numpy()
    ref = kr.dots_f64(Q, B)
    bound = 2 * d * 2.0 ** -24 * (np.abs(Q).astype(np.float64) @
                                  np.abs(B).astype(np.float64).T)
    err = np.abs(tiled.astype(np.float64) - ref)
    print("dots_mfma tiled: max err/bound = %.3g" % (err / bound).max())
    assert (err <= bound).all()
    simple_rows = kt.dots_mfma(Qd[:63], Bd).cpu().numpy()  # nq < 64
    err = np.abs(simple_rows.astype(np.float64) - ref[:63])
    assert (err <= bound[:63]).all()
    assert np.array_equal(bits(tiled[:63]), bits(simple_rows))
    simple_cols = kt.dots_mfma(Qd, Bd[:63]).cpu().numpy()  # n < 64
    assert np.array_equal(bits(tiled[:, :63]), bits(simple_cols))


# ========================================================= select_from_dots
SEL_NCOLS = [1, 3, 64, 255, 257, 4096, 5003]
SEL_NQ = [1, 9, 17]
SEL_D = 32


@pytest.fixture(scope="module")
def seldata():
    """17 grid queries x 5016 grid base vectors: exact dots, norms and
    L2 distances, computed once. Rows/columns are sliced per case."""
    n = 5003 + 8 + 5
    Q = kr.grid((17, SEL_D), seed=31)
    B = kr.grid((n, SEL_D), seed=32)
    B[1::7] = B[0:-1:7]  # exact duplicate vectors: equal dists, id ties
    dots = kr.dots_exact(Q, B)
    qn, bn = kr.norms_exact(Q), kr.norms_exact(B)
    l2 = kr.l2_from_dots(dots, qn, bn)
    rng = np.random.default_rng(33)
    deleted = rng.random(n) < 1.0 / 3.0
    return dict(dots=dots, qn=qn, bn=bn, l2=l2, deleted=deleted,
                qn_d=dev(qn), bn_d=dev(bn), n=n)


def _select_case(kt, sd, nq, ncols, col_base, pad, k2, l2, ip, use_bm,
                 all_deleted=False):
    cols = slice(col_base, col_base + ncols)
    dots = sd["dots"][:nq, cols]
    dist = sd["l2"][:nq, cols] if l2 else dots
    ids = col_base + np.arange(ncols)
    deleted = None
    bm = None
    if all_deleted:
        deleted = np.ones(sd["n"], bool)
    elif use_bm:
        deleted = sd["deleted"]
    if deleted is not None:
        bm = kt.bitmap_to_dev(kr.bitmap_words(deleted))
    got = kt.select_from_dots(
        padded(dots, pad), ncols, k2, l2, ip,
        qnorms=sd["qn_d"] if l2 else None,
        bnorms=sd["bn_d"] if l2 else None,
        col_base=col_base, bitmap=bm)
    want = kr.topk_keys_rows(dist, ids, k2, ip, deleted)
    assert np.array_equal(kt.keys_to_np(got), want), dict(
        nq=nq, ncols=ncols, col_base=col_base, pad=pad, k2=k2, l2=l2, ip=ip,
        bm=use_bm)


@pytest.mark.parametrize("k2", [1, 10, 64, 192, 193, 500, 640, 1024])
def test_select_from_dots_shapes(kt, seldata, k2):
    """k2 <= 192 is the wave-per-query kernel, above it the block kernel.
    Every ncols (incl. ncols < k2 -> EMPTY padding) x row stride
    (ncols: rows aligned iff ncols % 4 == 0; +4: aligned rows with a gap;
    +1: rows 1.. misaligned -> scalar branch) x col_base (0, 8 vector;
    5 scalar) x l2/ip_order, with nq and the bitmap cycling so that each
    appears with each k2. Grid L2 distances and grid dots are tie-heavy;
    the base holds exact duplicate vectors."""
    case = 0
    for ncols, pad, col_base in itertools.product(
            SEL_NCOLS, [0, 4, 1], [0, 8, 5]):
        for l2, ip in itertools.product([1, 0], [0, 1]):
            nq = SEL_NQ[case % 3]
            use_bm = (case // 3) % 2 == 1
            case += 1
            _select_case(kt, seldata, nq, ncols, col_base, pad, k2, l2, ip,
                         use_bm)


@pytest.mark.parametrize("k2", [10, 192, 193, 1024])
def test_select_from_dots_everything_deleted(kt, seldata, k2):
    for ncols, col_base, ip in [(257, 5, 0), (4096, 8, 1), (64, 0, 0)]:
        _select_case(kt, seldata, 9, ncols, col_base, 0, k2, 1, ip, False,
                     all_deleted=True)
    got = kt.select_from_dots(
        padded(seldata["dots"][:9, :64], 0), 64, k2, 0, 1,
        bitmap=kt.bitmap_to_dev(np.full(2, 0xFFFFFFFF, np.uint32)))
    assert (kt.keys_to_np(got) == EMPTY).all()


@pytest.mark.parametrize("k2", [64, 192, 500])
def test_select_from_dots_seeded_accumulation(kt, seldata, k2):
    """5003 columns in three calls (col_base 0 / 2048 / 4099, seeded
    0/1/1): the final state equals ONE reference top-k over all columns.
    k2 = 64, 192: wave kernel (192 = the largest seed it folds in);
    k2 = 500: block kernel. The last chunk starts at a col_base that is
    not a multiple of 4 (scalar branch) and the middle one has
    ncols % 4 != 0."""
    sd = seldata
    nq = 9
    bounds = [0, 2048, 4099, 5003]
    for l2, ip, use_bm in [(1, 0, False), (1, 0, True), (0, 1, False),
                           (0, 1, True), (0, 0, False), (1, 1, True)]:
        deleted = sd["deleted"] if use_bm else None
        bm = (kt.bitmap_to_dev(kr.bitmap_words(deleted))
              if use_bm else None)
        state = None
        for a, b in zip(bounds[:-1], bounds[1:]):
            state = kt.select_from_dots(
                padded(sd["dots"][:nq, a:b], 0), b - a, k2, l2, ip,
                qnorms=sd["qn_d"] if l2 else None,
                bnorms=sd["bn_d"] if l2 else None,
                col_base=a, bitmap=bm, state=state, seeded=a > 0)
        dist = (sd["l2"] if l2 else sd["dots"])[:nq, :5003]
        want = kr.topk_keys_rows(dist, np.arange(5003), k2, ip, deleted)
        assert np.array_equal(kt.keys_to_np(state), want), (l2, ip, use_bm)


@pytest.mark.parametrize("k2", [1, 10, 192, 193, 1024])
def test_select_from_dots_special_values(kt, k2):
    """l2 = 0 rows drawn from {-inf, -FLT_MAX, -3, -2^-140, 0, 2^-140,
    1, 1, FLT_MAX, +inf} repeated (negative values, infinities,
    subnormals, key images on both sides of 2^31), plus a row where all
    values are equal; both key orders."""
    rng = np.random.default_rng(41)
    for ncols, pad, col_base in [(257, 0, 0), (4096, 0, 8), (4096, 1, 0),
                                 (5003, 0, 5), (64, 4, 0), (3, 0, 0)]:
        rows = np.stack([
            rng.permutation(np.resize(kr.SPECIALS, ncols)),
            np.full(ncols, 1.0, np.float32),
            np.resize(kr.SPECIALS, ncols),
            np.full(ncols, -np.inf, np.float32),
            rng.choice(kr.SPECIALS, ncols)]).astype(np.float32)
        ids = col_base + np.arange(ncols)
        for ip in (0, 1):
            got = kt.select_from_dots(padded(rows, pad, fill=0.5), ncols,
                                      k2, 0, ip, col_base=col_base)
            want = kr.topk_keys_rows(rows, ids, k2, ip)
            assert np.array_equal(kt.keys_to_np(got), want), (
                ncols, pad, col_base, ip)


# ========================================================= select_rows_full
@pytest.fixture(scope="module")
def fulldata():
    Q = kr.grid((5, SEL_D), seed=51)
    B = kr.grid((8192, SEL_D), seed=52)
    B[1::5] = B[0:-1:5]
    dots = kr.dots_exact(Q, B)
    qn, bn = kr.norms_exact(Q), kr.norms_exact(B)
    return dict(dots=dots, l2=kr.l2_from_dots(dots, qn, bn),
                qn_d=dev(qn), bn_d=dev(bn))


def _full_k2s(ncols):
    ks = {1, min(ncols, 32), ncols}
    if ncols <= 100:
        ks.add(ncols + 3)
    return sorted(ks)


@pytest.mark.parametrize("ncols", [1, 5, 64, 100, 512, 513, 8192])
def test_select_rows_full(kt, fulldata, ncols):
    """pad-to-pow2 (ncols not a power of two), k2 > ncols with the
    (-1.0, -1) padding, both orders, l2 on/off, aligned and misaligned
    rows; and the promise that it has the same key order as
    select_from_dots (compared through unpack_keys where k2 <= 1024)."""
    fd = fulldata
    ids = np.arange(ncols)
    case = 0
    for k2, l2, ip in itertools.product(_full_k2s(ncols), [1, 0], [0, 1]):
        pad = case % 2
        case += 1
        dots = fd["dots"][:, :ncols]
        dist = fd["l2"][:, :ncols] if l2 else dots
        buf = padded(dots, pad)
        qn = fd["qn_d"] if l2 else None
        bn = fd["bn_d"] if l2 else None
        gd, gi = kt.select_rows_full(buf, ncols, k2, l2, ip, qn, bn)
        wd, wi = kr.key_decode(kr.topk_keys_rows(dist, ids, k2, ip), ip)
        ctx = (ncols, k2, l2, ip, pad)
        assert np.array_equal(gi.cpu().numpy(), wi), ctx
        assert np.array_equal(bits(gd.cpu().numpy()), bits(wd)), ctx
        if k2 > ncols:
            assert (wi[:, ncols:] == -1).all() and (wd[:, ncols:] == -1).all()
        if k2 <= 1024:
            keys = kt.select_from_dots(buf, ncols, k2, l2, ip, qn, bn)
            sd_, si_ = kt.unpack_keys(keys, ip)
            assert np.array_equal(si_.cpu().numpy(), gi.cpu().numpy()), ctx
            assert np.array_equal(bits(sd_.cpu().numpy()),
                                  bits(gd.cpu().numpy())), ctx


@pytest.mark.parametrize("ncols", [5, 100, 513])
def test_select_rows_full_special_values(kt, ncols):
    rng = np.random.default_rng(53)
    rows = np.stack([
        rng.permutation(np.resize(kr.SPECIALS, ncols)),
        np.full(ncols, -3.0, np.float32),
        rng.choice(kr.SPECIALS, ncols)]).astype(np.float32)
    for k2, ip in itertools.product(_full_k2s(ncols), [0, 1]):
        gd, gi = kt.select_rows_full(padded(rows, 1), ncols, k2, 0, ip)
        wd, wi = kr.key_decode(
            kr.topk_keys_rows(rows, np.arange(ncols), k2, ip), ip)
        assert np.array_equal(gi.cpu().numpy(), wi), (ncols, k2, ip)
        assert np.array_equal(bits(gd.cpu().numpy()), bits(wd))


def test_select_rows_full_rejects_rows_over_8192(kt):
    """ncols = 8193 pads to 16384 keys = 128 KB of LDS: the host entry
    must return an error code instead of launching."""
    buf = dev(np.zeros((1, 8193), np.float32))
    with pytest.raises(kt.KTestError) as ei:
        kt.select_rows_full(buf, 8193, 10, 0, 0)
    assert ei.value.code == 1  # hipErrorInvalidValue
    # the device is still healthy: the largest legal row works
    gd, gi = kt.select_rows_full(buf, 8192, 2, 0, 0)
    assert gi.cpu().numpy().tolist() == [[0, 1]]


# ================================================== sort_rows / unpack_keys
SORT_VALUES = np.concatenate([kr.SPECIALS, np.array([-0.0], np.float32)])


def _random_keys(rng, shape, ip, p_empty=0.2, nid=40):
    """keys over the special-value set with ids from a small range (so
    exact duplicate keys occur) and EMPTY interspersed"""
    dist = rng.choice(SORT_VALUES, shape)
    ids = rng.integers(0, nid, size=shape)
    keys = kr.key_encode(dist, ids, ip)
    keys[rng.random(shape) < p_empty] = EMPTY
    return keys


@pytest.mark.parametrize("ncand", [1, 3, 100, 1000, 2048])
def test_sort_rows(kt, ncand):
    rng = np.random.default_rng(60 + ncand)
    nq = 5
    for ip, k in itertools.product([0, 1], [1, 10, ncand, ncand + 5]):
        keys = _random_keys(rng, (nq, ncand), ip)
        keys[1] = EMPTY                      # a fully empty row
        keys[2] = keys[2, 0]                 # a row of one repeated key
        keys[3] = np.sort(keys[3])[::-1]     # descending input
        gd, gi = kt.sort_rows(kt.keys_to_dev(keys), k, ip)
        want = np.full((nq, k), EMPTY, np.uint64)
        m = min(k, ncand)
        want[:, :m] = np.sort(keys, axis=1)[:, :m]
        wd, wi = kr.key_decode(want, ip)
        assert np.array_equal(gi.cpu().numpy(), wi), (ncand, k, ip)
        assert np.array_equal(bits(gd.cpu().numpy()), bits(wd)), (
            ncand, k, ip)


@pytest.mark.parametrize("n", [1, 3, 255, 257, 1001])
def test_unpack_keys(kt, n):
    rng = np.random.default_rng(70 + n)
    for ip in (0, 1):
        keys = _random_keys(rng, (n,), ip, nid=2 ** 32)
        keys[0] = kr.key_encode(np.float32(-0.0), 2 ** 32 - 1, ip)
        gd, gi = kt.unpack_keys(kt.keys_to_dev(keys), ip)
        wd, wi = kr.key_decode(keys, ip)
        assert np.array_equal(gi.cpu().numpy(), wi)
        assert np.array_equal(bits(gd.cpu().numpy()), bits(wd))
    keys = np.full(n, EMPTY, np.uint64)
    gd, gi = kt.unpack_keys(kt.keys_to_dev(keys), 0)
    assert (gi.cpu().numpy() == -1).all() and (gd.cpu().numpy() == -1).all()


# ============================================================== argmin_rows
@pytest.mark.parametrize("nrows", [1, 257])
@pytest.mark.parametrize("ncols", [1, 2, 255, 4096])
def test_argmin_rows(kt, ncols, nrows):
    """Values from a small exact set so the minimum repeats in most rows
    (-> lowest column); with more than one row the first and last are
    all-infinite (-> 0), and a lone all-infinite row is run on its own."""
    rng = np.random.default_rng(80 + ncols + nrows)
    dots = (rng.integers(-4, 5, size=(nrows, ncols)) / 8.0).astype(
        np.float32)
    qn = (rng.integers(0, 17, size=nrows) / 8.0).astype(np.float32)
    bn = (rng.integers(0, 3, size=ncols) / 8.0).astype(np.float32)
    inf_rows = [0, nrows - 1] if nrows > 1 else []
    # L2: dist = fmaf(-2, dot, qn + bn); dots = -inf makes the row +inf
    dist = kr.l2_from_dots(dots, qn, bn)
    d_l2 = dots.copy()
    d_l2[inf_rows] = -np.inf
    dist[inf_rows] = np.inf
    want = np.argmin(dist, axis=1)  # first occurrence = lowest column
    assert (want[inf_rows] == 0).all()
    if ncols >= 255:
        assert ((dist == dist.min(axis=1, keepdims=True)).sum(axis=1)
                > 1).any(), "test data must contain repeated minima"
    qn_d, bn_d = dev(qn), dev(bn)
    got = kt.argmin_rows(dev(d_l2), 1, qn_d, bn_d).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # IP: best = largest dot, lowest column among equals
    d_ip = dots.copy()
    if nrows > 1:
        d_ip[0] = np.inf
        d_ip[-1] = -np.inf
    want = np.argmax(d_ip, axis=1)
    got = kt.argmin_rows(dev(d_ip), 0).cpu().numpy()
    assert np.array_equal(got, want)
    # one row, every distance +inf -> column 0
    for fill, l2 in [(-np.inf, 1), (-np.inf, 0), (np.inf, 0)]:
        row = dev(np.full((1, ncols), fill, np.float32))
        got = kt.argmin_rows(row, l2, qn_d if l2 else None,
                             bn_d if l2 else None).cpu().numpy()
        assert got.tolist() == [0], (fill, l2)


# =================================================================== rerank
RR_N, RR_NQ = 300, 3


@pytest.fixture(scope="module")
def rrdata():
    """per (d, ip): Gaussian base/queries and the oracle's canonical
    sequential-fmaf distance table T[q][id] (flat_search with k = n,
    scattered by id), computed once"""
    cache = {}

    def get(d, ip):
        if (d, ip) not in cache:
            rng = np.random.default_rng(90 + d)
            base = rng.standard_normal((RR_N, d)).astype(np.float32)
            q = rng.standard_normal((RR_NQ, d)).astype(np.float32)
            od, oi = orc.flat_search(base, q, RR_N, "IP" if ip else "L2")
            table = np.empty((RR_NQ, RR_N), np.float32)
            np.put_along_axis(table, oi, od, axis=1)
            cache[(d, ip)] = (base, q, table)
        return cache[(d, ip)]
    return get


@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("d", [32, 36, 128, 768])
def test_rerank(kt, rrdata, d, ip):
    """d = 32, 36: generic thread-per-candidate kernel; d = 128, 768: LDS
    kernel (256-candidate chunks: ncand 255 / 257 / 300 sit on both sides
    of the chunk edge). seg_shift 2 = 75 segments (> 64: the segment
    table is not cached in LDS), 4 = 19 segments with a short last one,
    9 = one segment. Ids are a random permutation, EMPTY keys sit at
    random positions and must come out EMPTY; one run per shape is done
    in place (keys_out = keys_in). Output keys are compared exactly."""
    base, q, table = rrdata(d, ip)
    qd = dev(q)
    rng = np.random.default_rng(7 * d + ip)
    for seg_shift in (2, 4, 9):
        segs = kt.split_segments(base, seg_shift)
        assert len(segs) == {2: 75, 4: 19, 9: 1}[seg_shift]
        for ncand in (1, 255, 257, 300):
            ids = np.stack([rng.permutation(RR_N)[:ncand]
                            for _ in range(RR_NQ)])
            # incoming distances are stale approximations: any value
            kin = kr.key_encode(
                rng.standard_normal(ids.shape).astype(np.float32), ids, ip)
            empty = rng.random(ids.shape) < 0.15
            if ncand > 1:
                empty[0, 0] = True
                empty[1, -1] = True
            kin[empty] = EMPTY
            want = kr.key_encode(np.take_along_axis(table, ids, axis=1),
                                 ids, ip)
            want[empty] = EMPTY
            kin_d = kt.keys_to_dev(kin)
            out = kt.rerank(qd, segs, seg_shift, ip, kin_d)
            ctx = (d, ip, seg_shift, ncand)
            assert np.array_equal(kt.keys_to_np(out), want), ctx
            assert np.array_equal(kt.keys_to_np(kin_d), kin), ctx
            same = kt.rerank(qd, segs, seg_shift, ip, kin_d, keys_out=kin_d)
            assert same is kin_d
            assert np.array_equal(kt.keys_to_np(kin_d), want), ctx


# ========================================================= flat_stream_scan
@pytest.mark.parametrize("d", [4, 36, 128, 200])
def test_flat_stream_scan(kt, d):
    """Grid data -> the shuffle-tree distances are exact, so the result
    equals float64 brute force + topk_keys. d/2 below, at and off the
    64-lane stride; n off the 4-wave pass; k2 > n pads with EMPTY;
    segment tables with many short segments and with one; exact duplicate
    base vectors tie on distance and resolve by id."""
    nq = 3
    q = kr.grid((nq, d), seed=300 + d)
    base_all = kr.grid((1001, d), seed=400 + d)
    base_all[1::3] = base_all[0:-1:3]
    rng = np.random.default_rng(d)
    deleted_all = rng.random(1001) < 1.0 / 3.0
    qd = dev(q)
    for n in (1, 3, 257, 1001):
        base = base_all[:n]
        dist = {0: kr.l2_exact(q, base), 1: kr.dots_exact(q, base)}
        ids = np.arange(n)
        for seg_shift in (4, 10):
            segs = kt.split_segments(base, seg_shift)
            for k2, use_bm, ip in itertools.product(
                    [1, 10, 300], [False, True], [0, 1]):
                deleted = deleted_all[:n] if use_bm else None
                bm = (kt.bitmap_to_dev(kr.bitmap_words(deleted))
                      if use_bm else None)
                got = kt.flat_stream_scan(qd, segs, n, seg_shift, k2, ip,
                                          bitmap=bm)
                want = kr.topk_keys_rows(dist[ip], ids, k2, ip, deleted)
                assert np.array_equal(kt.keys_to_np(got), want), (
                    d, n, seg_shift, k2, use_bm, ip)


# ========================================================= pq_encode(_pack4)
@pytest.mark.parametrize("ksub", [256, 16])
@pytest.mark.parametrize("M", [4, 8, 16])
def test_pq_encode(kt, M, ksub):
    """Grid data, d = 32; codebooks with duplicated centroids so the
    argmin ties — expected: the lowest j, from float64 brute force. At
    ksub = 16 the packed form equals the 8-bit-form codes packed
    low-nibble-even."""
    d = 32
    dsub = d // M
    x_all = kr.grid((1000, d), seed=500 + M)
    cb = kr.grid((M, ksub, dsub), seed=600 + M + ksub)
    dups = list(range(ksub // 2, ksub // 2 + 4)) + [ksub - 1]
    cb[:, dups[:4]] = cb[:, 1:5]  # duplicates of lower-j centroids
    cb[:, ksub - 1] = cb[:, 0]
    x_all[:8] = cb[:, 0].reshape(-1)  # exact hits on j = 0 (and ksub-1)
    cbd = dev(cb)
    for n in (1, 255, 1000):
        x = x_all[:n]
        want = kr.pq_encode_ref(x, cb, M, ksub)
        assert not np.isin(want, dups).any()  # a duplicate never wins
        got = kt.pq_encode(dev(x), cbd, M, ksub).cpu().numpy()
        assert np.array_equal(got, want), (M, ksub, n)
        if ksub == 16:
            gp = kt.pq_encode_pack4(dev(x), cbd, M).cpu().numpy()
            assert np.array_equal(gp, kr.pack4(want)), (M, n)
            assert np.array_equal(gp, kr.pack4(got))
