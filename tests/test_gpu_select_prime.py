"""The wave-per-query select (gk::select_from_dots, k2 <= 192) primes its
selector with a bound from a first walk over the row: the k2-th smallest of
the row's group minima. Every case here compares three results for byte
equality of the (nq, k2) keys: primed (the default), GAMMA_SELECT_PRIME=0
(the unprimed single walk) and oracle.kernel_refs.topk_keys_rows.

nq = 9: two workgroups of 8 waves, the second with one live wave.

The partition the kernel uses (gamma_walk_row / gamma_select_wave in
csrc/kernels.hip), as `group_of` models it: a row whose start is 16-byte
aligned, with ncols and col_base multiples of 4, is read as float4 and lane
(c >> 2) & 63 holds column c in slot c & 3; any other row is read by scalars
and lane c & 63 holds column c in slot (c >> 6) & 3. R = 1 for k2 <= 32, 2
for k2 <= 64, else 4, and the group of a column is (lane, slot & (R - 1)).

L2 inputs are integer-valued (dots, norms and the distances qn + bn - 2 dot
stay below 2^24), so the reference distance is exact in fp32 whatever the
order of the kernel's fmaf."""
import numpy as np
import pytest

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

NQ = 9
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
METRICS = [(1, 0), (0, 1)]  # (l2, ip_order): L2, inner product


@pytest.fixture(scope="module")
def kt():
    from vearch_amd import ktest
    return ktest


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def group_of(c, k2, vector):
    """group number in [0, 64 * R) of column c (see the module text)"""
    c = np.asarray(c)
    R = 1 if k2 <= 32 else 2 if k2 <= 64 else 4
    if vector:
        lane, slot = (c >> 2) & 63, c & 3
    else:
        lane, slot = c & 63, (c >> 6) & 3
    return lane + 64 * (slot & (R - 1))


@pytest.fixture(scope="module")
def data():
    """integer-valued dots (NQ, 8192 + 8) and norms, drawn once"""
    rng = np.random.default_rng(2024)
    n = 8192 + 8
    return dict(
        dots=rng.integers(-1000000, 1000001, size=(NQ, n)).astype(np.float32),
        qn=rng.integers(0, 1001, size=NQ).astype(np.float32),
        bn=rng.integers(0, 1001, size=n).astype(np.float32))


def check(kt, monkeypatch, data, dots, k2, l2, ip, pad=0, col_base=0,
          deleted=None, vector=None):
    """dots (NQ, ncols) host values of columns col_base .. col_base + ncols
    -> the primed keys, after asserting primed == unprimed == reference.
    pad: extra floats per row in the device matrix (1: every row whose
    number is no multiple of 4 starts off a 16-byte boundary -> scalar
    path). vector: which path the case means to take, asserted from the
    layout."""
    ncols = dots.shape[1]
    if vector is not None:
        assert vector == (ncols % 4 == 0 and col_base % 4 == 0
                          and pad % 4 == 0)
    ids = col_base + np.arange(ncols)
    qn, bn = data["qn"], data["bn"]
    if l2:
        dist = (qn[:, None] + bn[None, ids] - 2.0 * dots.astype(np.float64))
        assert np.abs(dist).max() < 2 ** 24
        dist = dist.astype(np.float32)
    else:
        dist = dots
    want = kr.topk_keys_rows(dist, ids, k2, ip, deleted)
    buf = np.full((NQ, ncols + pad), np.nan, np.float32)
    buf[:, :ncols] = dots
    dd = dev(buf)
    bm = None if deleted is None else kt.bitmap_to_dev(
        kr.bitmap_words(deleted))
    kw = dict(qnorms=dev(qn) if l2 else None, bnorms=dev(bn) if l2 else None,
              col_base=col_base, bitmap=bm)
    monkeypatch.delenv("GAMMA_SELECT_PRIME", raising=False)
    on = kt.keys_to_np(kt.select_from_dots(dd, ncols, k2, l2, ip, **kw))
    monkeypatch.setenv("GAMMA_SELECT_PRIME", "0")
    off = kt.keys_to_np(kt.select_from_dots(dd, ncols, k2, l2, ip, **kw))
    monkeypatch.delenv("GAMMA_SELECT_PRIME")
    assert np.array_equal(off, want), "unprimed != reference"
    assert np.array_equal(on, want), "primed != reference"
    assert on.tobytes() == off.tobytes()
    return on


@pytest.mark.parametrize("l2,ip", METRICS, ids=["l2", "ip"])
@pytest.mark.parametrize("k2", [1, 32, 64, 65, 192])
def test_paths_and_k2(kt, monkeypatch, data, k2, l2, ip):
    """1024 columns read as float4, 1002 columns by scalars, and 1024
    columns behind a row stride of 1025 floats (rows 1, 2, 3, 5, .. start
    off a 16-byte boundary -> scalars); every R (1, 2, 4) and both ends of
    each k2 range"""
    d = data["dots"]
    check(kt, monkeypatch, data, d[:, :1024], k2, l2, ip, vector=True)
    check(kt, monkeypatch, data, d[:, :1002], k2, l2, ip, vector=False)
    check(kt, monkeypatch, data, d[:, :1024], k2, l2, ip, pad=1,
          vector=False)


@pytest.mark.parametrize("l2,ip", METRICS, ids=["l2", "ip"])
def test_short_rows(kt, monkeypatch, data, l2, ip):
    """ncols = 40, k2 = 32: the vector path gives 10 lanes a column group
    (the scalar path 40), fewer than k2 real minima either way, so tau is
    EMPTY and the walk runs unprimed. ncols = 20 < k2: EMPTY tail."""
    d = data["dots"]
    check(kt, monkeypatch, data, d[:, :40], 32, l2, ip, vector=True)
    check(kt, monkeypatch, data, d[:, :40], 32, l2, ip, pad=1, vector=False)
    got = check(kt, monkeypatch, data, d[:, :20], 32, l2, ip)
    assert (got[:, 20:] == EMPTY).all() and (got[:, :20] != EMPTY).all()


@pytest.mark.parametrize("l2,ip", METRICS, ids=["l2", "ip"])
@pytest.mark.parametrize("k2", [32, 65])
def test_all_distances_equal(kt, monkeypatch, data, k2, l2, ip):
    """every key ties on distance: ids 0 .. k2-1 win. (L2: zero norms.)"""
    z = dict(data, qn=np.zeros_like(data["qn"]),
             bn=np.zeros_like(data["bn"]))
    for ncols, pad in [(1024, 0), (1002, 0)]:
        got = check(kt, monkeypatch, z, np.full((NQ, ncols), 3.0, np.float32),
                    k2, l2, ip, pad=pad)
        ids = (got & np.uint64(0xffffffff)).astype(np.int64)
        assert np.array_equal(ids, np.tile(np.arange(k2), (NQ, 1)))


@pytest.mark.parametrize("l2,ip", METRICS, ids=["l2", "ip"])
@pytest.mark.parametrize("k2", [32, 64, 192])
def test_sorted_rows(kt, monkeypatch, data, k2, l2, ip):
    """distances ascending by column (the winners are the first k2 columns:
    every one of them is its group's minimum) and descending (the winners
    come last; the unprimed walk admits nearly every key). Zero norms, so
    the L2 distance is -2 dot: the order flips with the metric, and both
    directions are given to both."""
    z = dict(data, qn=np.zeros_like(data["qn"]),
             bn=np.zeros_like(data["bn"]))
    for ncols in (1024, 1002):
        up = np.tile(np.arange(ncols, dtype=np.float32), (NQ, 1))
        up += 7.0 * np.arange(NQ, dtype=np.float32)[:, None]
        check(kt, monkeypatch, z, up, k2, l2, ip)
        check(kt, monkeypatch, z, up[:, ::-1].copy(), k2, l2, ip)


def _clustered_rows(ncols, k2, vector, sign):
    """Rows built group by group from group_of (the module text says how
    that follows the kernel's layout). `best` is a group of >= k2 columns.
    Its columns get the values 0 .. (in column order), so the k2 smallest
    keys of the row all lie in that one group and the other groups' minima
    decide tau. k2 - 1 further groups hold one constant each, 1000 + j for
    the j-th of them; every other column holds 100000 + c. tau is then the
    minimum of the last of those k2 - 1 groups, and all columns of the
    groups before it, (k2 - 2) * (columns per group) keys, are <= tau:
    several times the append region, so the walk flushes on the way.
    sign = -1 mirrors the values for a metric where larger is better."""
    c = np.arange(ncols)
    g = group_of(c, k2, vector)
    order = np.unique(g)
    best = order[5]
    assert (g == best).sum() >= k2
    row = (100000 + c).astype(np.float32)
    row[g == best] = np.arange((g == best).sum(), dtype=np.float32)
    others = [x for x in order if x != best][:k2 - 1]
    for j, x in enumerate(others):
        row[g == x] = 1000.0 + j
    rows = np.tile(row, (NQ, 1))
    admitted = (k2 - 2) * int((g == others[0]).sum())
    return sign * rows, c[g == best][:k2], admitted


@pytest.mark.parametrize("ncols,k2", [(4096, 32), (4090, 32), (8192, 64),
                                      (8190, 64)])
def test_winners_in_one_group(kt, monkeypatch, data, ncols, k2):
    """loose tau: see _clustered_rows. Plain dots (l2 = 0) in both key
    orders; the winners are the first k2 columns of the chosen group, and
    the counting hook confirms that the primed walk flushed on the way."""
    vector = ncols % 4 == 0
    for ip in (0, 1):
        rows, winners, admitted = _clustered_rows(
            ncols, k2, vector, -1.0 if ip else 1.0)
        got = check(kt, monkeypatch, data, rows, k2, 0, ip, vector=vector)
        ids = (got & np.uint64(0xffffffff)).astype(np.int64)
        assert np.array_equal(ids, np.tile(winners, (NQ, 1)))
        assert admitted > 2 * 512
        st, pushed, flushes = kt.select_wave_stats(dev(rows), ncols, k2, 0,
                                                   ip)
        assert np.array_equal(kt.keys_to_np(st), got)
        print("ncols=%d k2=%d ip=%d: pushed %s flushes %s" %
              (ncols, k2, ip, pushed, flushes))
        assert (flushes >= 1).all()


@pytest.mark.parametrize("l2,ip", METRICS, ids=["l2", "ip"])
@pytest.mark.parametrize("k2", [32, 65])
def test_bitmaps(kt, monkeypatch, data, k2, l2, ip):
    rng = np.random.default_rng(5)
    d = data["dots"]
    n = d.shape[1]
    for ncols, col_base, vector in [(1024, 8, True), (1002, 5, False)]:
        cols = d[:, col_base:col_base + ncols]
        # a random half deleted
        half = rng.random(n) < 0.5
        check(kt, monkeypatch, data, cols, k2, l2, ip, col_base=col_base,
              deleted=half, vector=vector)
        # every column of all but k2 - 1 groups deleted: fewer than k2 real
        # minima, tau = EMPTY, and the live columns still come out exactly
        g = group_of(np.arange(ncols), k2, vector)
        live = rng.permutation(np.unique(g))[:k2 - 1]
        dele = np.ones(n, bool)
        dele[col_base + np.flatnonzero(np.isin(g, live))] = False
        got = check(kt, monkeypatch, data, cols, k2, l2, ip,
                    col_base=col_base, deleted=dele, vector=vector)
        assert (got != EMPTY).sum(axis=1).min() == min(
            k2, int((~dele[col_base:col_base + ncols]).sum()))
        # everything deleted
        got = check(kt, monkeypatch, data, cols, k2, l2, ip,
                    col_base=col_base, deleted=np.ones(n, bool),
                    vector=vector)
        assert (got == EMPTY).all()


@pytest.mark.parametrize("l2,ip", METRICS, ids=["l2", "ip"])
@pytest.mark.parametrize("k2", [32, 64, 192])
def test_seeded_two_segments(kt, monkeypatch, data, k2, l2, ip):
    """columns [0, 1024) unseeded, then [1024, 2026) seeded with the first
    call's state (col_base != 0; the k2 seeds give the selector a real
    threshold, so the second call takes no first walk) == one shot over all
    2026 columns == reference. Seeds fewer than k2: test_few_seeds_prime."""
    d, qn, bn = data["dots"], data["qn"], data["bn"]
    ids = np.arange(2026)
    if l2:
        dist = (qn[:, None] + bn[None, ids]
                - 2.0 * d[:, :2026].astype(np.float64)).astype(np.float32)
    else:
        dist = d[:, :2026]
    want = kr.topk_keys_rows(dist, ids, k2, ip)
    kw = dict(qnorms=dev(qn) if l2 else None, bnorms=dev(bn) if l2 else None)
    a, b = dev(d[:, :1024]), dev(d[:, 1024:2026])
    one = dev(d[:, :2026])
    res = {}
    for mode in ("on", "off"):
        if mode == "off":
            monkeypatch.setenv("GAMMA_SELECT_PRIME", "0")
        else:
            monkeypatch.delenv("GAMMA_SELECT_PRIME", raising=False)
        st = kt.select_from_dots(a, 1024, k2, l2, ip, **kw)
        st = kt.select_from_dots(b, 1002, k2, l2, ip, col_base=1024,
                                 state=st, seeded=True, **kw)
        res[mode] = kt.keys_to_np(st)
        shot = kt.keys_to_np(kt.select_from_dots(one, 2026, k2, l2, ip, **kw))
        assert np.array_equal(shot, want), mode
    monkeypatch.delenv("GAMMA_SELECT_PRIME")
    assert np.array_equal(res["on"], want)
    assert np.array_equal(res["off"], want)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_coarse_select_on_equals_off(kt, monkeypatch, ip):
    """gk::coarse_select at NQ = 130, NLIST = 1000, D = 20, n1 = 256,
    nprobe = 32: the seed state the filter is handed is the same exact
    sorted top-nprobe, so keys and candidate counters do not move"""
    nq, nlist, d, n1, nprobe = 130, 1000, 20, 256, 32
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    B = rng.standard_normal((nlist, d)).astype(np.float32)
    nrm = lambda x: (x ** 2).sum(axis=1, dtype=np.float32)  # noqa: E731
    assert kt.coarse_can_filter(nq, nlist, d, nprobe, n1)
    out = {}
    for mode in ("on", "off"):
        if mode == "off":
            monkeypatch.setenv("GAMMA_SELECT_PRIME", "0")
        else:
            monkeypatch.delenv("GAMMA_SELECT_PRIME", raising=False)
        keys, cnt, flag = kt.coarse_select(
            dev(Q), dev(B), nprobe, not ip, ip, n1, nlist,
            qnorms=dev(nrm(Q)), bnorms=dev(nrm(B)))
        out[mode] = (kt.keys_to_np(keys), cnt.copy(), flag)
    monkeypatch.delenv("GAMMA_SELECT_PRIME")
    assert out["on"][2] == 0 and out["off"][2] == 0
    assert out["on"][0].tobytes() == out["off"][0].tobytes()
    assert np.array_equal(out["on"][1], out["off"][1])


def test_priming_is_live(kt, monkeypatch):
    """i.i.d. Gaussian rows, ncols = 4096, k2 = 32, read as float4: G = 64
    groups (R = 1) of g = 64 columns. A key at the quantile p of the row is
    at or above its group's minimum with probability 1 - (1 - p)^g, so
    about G (1 - (1 - p)^g) group minima lie below it; tau, the k2-th
    smallest minimum, therefore sits near the p that solves
    G (1 - (1 - p)^g) = k2, i.e. p = 1 - (1 - k2 / G)^(1 / g) = 0.01077,
    and the second walk admits about p * ncols = 44.1 keys per row (flushes
    can only lower that). The bound is twice that expectation. Unprimed,
    the selector's threshold is EMPTY until its first flush, which comes
    after the first float4 pass at the earliest: at least 256 keys."""
    ncols, k2, G = 4096, 32, 64
    g = ncols // G
    expected = ncols * (1.0 - (1.0 - k2 / G) ** (1.0 / g))
    assert 40 < expected < 48
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((64, ncols)).astype(np.float32)
    want = kr.topk_keys_rows(rows, np.arange(ncols), k2, 0)
    dd = dev(rows)
    monkeypatch.delenv("GAMMA_SELECT_PRIME", raising=False)
    st, pushed, flushes = kt.select_wave_stats(dd, ncols, k2, 0, 0)
    assert np.array_equal(kt.keys_to_np(st), want)
    print("primed: pushed mean %.1f max %d, rows flushing mid-walk %d "
          "(expected %.1f)" % (pushed.mean(), pushed.max(),
                               (flushes > 0).sum(), expected))
    monkeypatch.setenv("GAMMA_SELECT_PRIME", "0")
    st0, pushed0, _ = kt.select_wave_stats(dd, ncols, k2, 0, 0)
    monkeypatch.delenv("GAMMA_SELECT_PRIME")
    assert np.array_equal(kt.keys_to_np(st0), want)
    print("unprimed: pushed mean %.1f min %d" % (pushed0.mean(),
                                                 pushed0.min()))
    assert (pushed0 >= 256).all()
    assert pushed.mean() < 2.0 * expected


def _expected_admitted(ncols, k2, G):
    """p * ncols with p from G (1 - (1 - p)^g) = k2, g = ncols / G: the
    derivation in test_priming_is_live"""
    return ncols * (1.0 - (1.0 - k2 / G) ** (G / ncols))


def test_few_seeds_prime(kt, monkeypatch):
    """A seeded call whose seeds are fewer than k2 still primes: 20 columns
    first (20 seeds, k2 = 32: the selector's threshold stays EMPTY), then
    4096 Gaussian columns at col_base 20, read as float4. The second call
    admits what an unseeded primed walk admits (bound: twice the 44.1 of
    test_priming_is_live; the 20 seeds do not enter tau), unprimed at least
    the first pass of 256, and the state equals the reference top-k2 of all
    4116 columns."""
    k2 = 32
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((64, 20 + 4096)).astype(np.float32)
    want = kr.topk_keys_rows(rows, np.arange(rows.shape[1]), k2, 0)
    a, b = dev(rows[:, :20]), dev(rows[:, 20:])
    expected = _expected_admitted(4096, k2, 64)
    pushed = {}
    for mode in ("on", "off"):
        if mode == "off":
            monkeypatch.setenv("GAMMA_SELECT_PRIME", "0")
        else:
            monkeypatch.delenv("GAMMA_SELECT_PRIME", raising=False)
        st = kt.select_from_dots(a, 20, k2, 0, 0)
        assert (kt.keys_to_np(st)[:, 20:] == EMPTY).all()
        st, pushed[mode], _ = kt.select_wave_stats(
            b, 4096, k2, 0, 0, col_base=20, state=st, seeded=True)
        assert np.array_equal(kt.keys_to_np(st), want), mode
    monkeypatch.delenv("GAMMA_SELECT_PRIME")
    print("few seeds: pushed mean on %.1f off %.1f (expected %.1f)" %
          (pushed["on"].mean(), pushed["off"].mean(), expected))
    assert (pushed["off"] >= 256).all()
    assert pushed["on"].mean() < 2.0 * expected


def test_wide_rows_are_not_primed(kt, monkeypatch):
    """The first walk runs up to 16384 columns (GAMMA_SELECT_PRIME_MAX_COLS
    in kernels.hip: a 64 KB row) and not beyond, where its second read
    would come from HBM. Both sides of that width, k2 = 32, Gaussian rows:
    at 16384 the primed walk admits about 44.3 keys (G = 64, g = 256 in the
    derivation of test_priming_is_live; bound: twice that), at 16388 the
    default walk is the unprimed one and admits its first pass of 256."""
    k2 = 32
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((NQ, 16388)).astype(np.float32)
    monkeypatch.delenv("GAMMA_SELECT_PRIME", raising=False)
    for ncols in (16384, 16388):
        sub = np.ascontiguousarray(rows[:, :ncols])
        want = kr.topk_keys_rows(sub, np.arange(ncols), k2, 0)
        st, pushed, _ = kt.select_wave_stats(dev(sub), ncols, k2, 0, 0)
        assert np.array_equal(kt.keys_to_np(st), want), ncols
        print("ncols=%d: pushed %s" % (ncols, pushed))
        if ncols <= 16384:
            assert pushed.mean() < 2.0 * _expected_admitted(ncols, k2, 64)
        else:
            assert (pushed >= 256).all()
