"""The IVFPQ scan variants test_gpu_scan_pipeline.py does not reach, each
on its own through the kernel test hook: the 4-bit kernel k_ivfpq_scan4
(its four fast shapes with two lists in flight per workgroup, at both
block sizes and GAMMA_ADC_C 1 and 2, and its generic byte-load path) and
the resident 8-bit kernel k_ivfpq_scan at its generic path (any M, table
read from atab) and at the fast shapes M = 64 and 96.

Written like test_gpu_scan_pipeline.py and sharing its probe tables:
inputs on the exact grid of oracle.kernel_refs, a numpy reference that
adds dis0, then the S term, then one fp32 add per sub-quantizer in
ascending m, keys compared with np.array_equal. On the grid every order of
the adds gives the same bits, so `test_add_order_on_gaussian_inputs` runs
each kernel family once on Gaussian inputs against the oracle library's
serial chains.

Shapes: 32 lists with sizes from {0, 1, 127, 128, 129, 255, 256, 257, 511,
512, 513, 1100}: the neighbours of HB*C entries per pass of k_ivfpq_scan4
(HB = half a block, 128 or 256; C = 1 or 2), at most 8 queries. The probe
table "pairs" (nprobe = 3) puts next to a long list, in the same pair of
the two-list walk, a probe of -1, one >= nlist, an empty list and a list
of one entry; its odd probe count leaves the last pair half empty, and
S = 4 exceeds it."""
import numpy as np
import pytest

import test_gpu_scan_pipeline as sp
from oracle import gamma_oracle as go
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

NLIST = sp.NLIST
NDOC = sp.NDOC
SIZES = [0, 1, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1100,
         0, 1, 1, 1, 127, 128, 129, 1, 1, 1, 255, 256, 1, 0, 1, 1, 1, 1, 1, 1]
L = {s: SIZES.index(s) for s in set(SIZES)}  # first list of each size
E = [i for i, s in enumerate(SIZES) if s == 0]

FAST4 = [(32, 16), (128, 32), (128, 64), (192, 96)]  # MW 2, 4, 8, 12
GEN4 = [(16, 4), (24, 12), (96, 24)]  # 2-, 6- and 12-byte entries
FAST8 = [(128, 64), (384, 96)]  # MW 16, 24
GEN8 = [(16, 4), (48, 12), (192, 48)]
KNOBS = [(512, 1), (512, 2), (256, 1), (256, 2)]  # GAMMA_SCAN_BS, ADC_C

PERM = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)


def _tables():
    t = sp._probe_tables(SIZES, small=(127, 128, 129))
    t["pairs"] = np.array([
        [L[1100], -1, L[257]],
        [L[1100], NLIST, L[513]],
        [L[1100], E[0], L[1]],
        [L[1], L[1100], L[129]],
        [L[1100], L[1], -1],
        [-1, L[1100], L[1100]],  # a list probed twice
        [E[0], E[1], L[1100]],
        [L[513], L[512], L[511]],
    ], dtype=np.int64)
    return t


class Case:
    """One (d, M, ksub, metric): model, lists and, per probe table, every
    candidate key of every query (computed once, never modified).
    gauss: codebooks, centroids, queries, S terms and probe distances are
    standard normal instead of grid values; the tables then come from the
    serial chains the kernels promise (L2: the device's pq_tables_a, pinned
    against the oracle in test_gpu_ingest_kernels.py; inner product:
    oracle_adc_table_ip and oracle_ip)."""

    def __init__(self, d, M, ksub, ip, gauss=False):
        self.d, self.M, self.ksub, self.ip = d, M, ksub, ip
        dsub = d // M
        rng = np.random.default_rng(1000 * d + M + int(ip) + 7 * ksub)

        def values(shape, seed):
            if gauss:
                return np.random.default_rng(seed).standard_normal(
                    shape).astype(np.float32)
            return kr.grid(shape, seed=seed)

        self.centroids = values((NLIST, d), d + 1)
        self.codebooks = values((M, ksub, dsub), d + 2)
        self.queries = values((8, d), d + 3)
        self.lists = []
        ids_pool = rng.permutation(NDOC)
        at = 0
        for n in SIZES:
            ids = ids_pool[at:at + n].astype(np.uint32)
            at += n
            dead = rng.random(n) < 0.06  # delete marks: bit 31
            ids = np.where(dead, ids | np.uint32(0x80000000), ids)
            codes = rng.integers(0, ksub, size=(n, M), dtype=np.uint8)
            svals = values((n,), int(rng.integers(1 << 30)))
            self.lists.append((ids.astype(np.uint32), codes, svals))
        self.deleted = rng.random(NDOC) < 0.10  # the bitmap
        if gauss:
            if ip:
                self.tab = go.adc_table_ip(self.queries, self.codebooks, M,
                                           ksub)
                self.cdots = go.ip_serial(self.queries, self.centroids)
            else:
                import torch
                from vearch_amd import ktest
                self.tab = ktest.pq_tables_a(
                    torch.from_numpy(self.queries).cuda(),
                    torch.from_numpy(self.codebooks).cuda(), M,
                    ksub).cpu().numpy()
                self.cdots = None
            assert not np.isnan(self.tab).any()
        else:
            # exact tables: L2 A = ||cw||^2 - 2 q_m.cw, IP T = q_m.cw
            q3 = self.queries.reshape(8, M, dsub).astype(np.float64)
            cb = self.codebooks.astype(np.float64)
            dots = np.einsum("qmt,mjt->qmj", q3, cb)
            tab = dots if ip else (cb * cb).sum(axis=2)[None] - 2.0 * dots
            self.tab = kr._exact_f32(tab)
            self.cdots = kr.dots_exact(self.queries, self.centroids)
        self.tables = _tables()
        self.probe_dists = {
            name: values(t.shape, len(name) + t.shape[1])
            for name, t in self.tables.items()}
        self._cands = {}

    def cands(self, name, bitmap):
        """per query: all candidate keys of probe table `name` (uint64)."""
        key = (name, bitmap)
        if key not in self._cands:
            self._cands[key] = [
                self._row_keys(name, qi, bitmap)
                for qi in range(self.tables[name].shape[0])]
        return self._cands[key]

    def _row_keys(self, name, qi, bitmap):
        out = [np.empty(0, np.uint64)]
        for p, ln in enumerate(self.tables[name][qi]):
            if ln < 0 or ln >= NLIST or SIZES[ln] == 0:
                continue
            ids, codes, svals = self.lists[ln]
            if self.ip:
                start = np.float32(self.cdots[qi, ln])
            else:
                dis0 = np.float32(self.probe_dists[name][qi, p])
                start = (dis0 + svals).astype(np.float32)
            dis = kr.adc_chain(start, self.tab[qi], codes)
            keep = (ids >> 31) == 0
            if bitmap:
                keep &= ~self.deleted[ids & 0x7FFFFFFF]
            out.append(kr.key_encode(dis[keep], ids[keep], self.ip))
        return np.concatenate(out)

    def expect(self, name, k2, bitmap=False):
        rows = []
        for keys in self.cands(name, bitmap):
            row = np.full(k2, kr._EMPTY, dtype=np.uint64)
            top = np.sort(keys)[:k2]
            row[:top.size] = top
            rows.append(row)
        return np.stack(rows)

    def run(self, name, S, k2, bitmap=False, qmap=None, kill_flag=None,
            code_offsets=None):
        from vearch_amd import ktest
        t = self.tables[name]
        nq = t.shape[0]
        return ktest.ivfpq_scan(
            self.lists, t, self.probe_dists[name], self.queries[:nq],
            self.centroids, self.codebooks, S, k2, self.ip,
            bitmap=kr.bitmap_words(self.deleted) if bitmap else None,
            qmap=qmap, kill_flag=kill_flag, code_offsets=code_offsets,
            ksub=self.ksub)


_cases = {}


def _case(d, M, ksub, ip, gauss=False):
    key = (d, M, ksub, ip, gauss)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def _check(c, name, S, k2, **kw):
    """The kernel's own rows at S = 1 and the merge of the S partial rows
    (gk::sort_rows; where S * k2 exceeds what it takes, a plain sort of
    the kernel's keys) against the reference. Returns the kernel's keys."""
    keys, dists, ids = c.run(name, S, k2, **kw)
    want = c.expect(name, k2, bitmap=kw.get("bitmap", False))
    tag = (f"{name} d={c.d} M={c.M} ksub={c.ksub} ip={c.ip} S={S} "
           f"k2={k2} {kw}")
    assert keys.shape == (want.shape[0], S, k2), tag
    if S == 1:  # the kernel's own rows, EMPTY padding included
        assert np.array_equal(keys[:, 0, :], want), tag
    if dists is None:
        merged = np.sort(keys.reshape(keys.shape[0], S * k2), axis=1)
        assert np.array_equal(merged[:, :k2], want), tag
        return keys
    # the engine's merge of the S partial rows, re-encoded as keys
    wd, wi = kr.key_decode(want, c.ip)
    got = np.where(ids < 0, kr._EMPTY, kr.key_encode(dists, ids, c.ip))
    assert np.array_equal(got, want), tag
    assert np.array_equal(ids, wi), tag
    assert np.array_equal(dists.view(np.uint32), wd.view(np.uint32)), tag
    return keys


def _knobs(monkeypatch, bs, c):
    monkeypatch.setenv("GAMMA_SCAN_BS", str(bs))
    monkeypatch.setenv("GAMMA_ADC_C", str(c))


# every probe table at the small k2, then the two tables with rows of
# ~1900 candidates at the k2 around the selector's limits
_ALL = [(1, 200), (2, 10), (4, 1), (1, 1024)]
_DEEP = [(1, 1), (1, 10), (4, 200), (2, 1024), (1, 1030), (1, 1088),
         (2, 1088)]


def _sweep(c):
    for name in c.tables:
        for S, k2 in _ALL:
            _check(c, name, S, k2)
    for name in ("rows8", "pairs"):
        for S, k2 in _DEEP:
            _check(c, name, S, k2)


# ----------------------------------------------------------- 4-bit kernel
@pytest.mark.parametrize("bs,cc", KNOBS)
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", FAST4)
def test_scan4_fast_rows(d, M, ip, bs, cc, monkeypatch):
    """k2 = 1030 and 1088 with C = 2 leave the fast path (k2 + BS*C above
    the selector cap at BS 512): the generic kernel on fast-M entries."""
    _knobs(monkeypatch, bs, cc)
    _sweep(_case(d, M, 16, ip))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", GEN4)
def test_scan4_generic_rows(d, M, ip):
    _sweep(_case(d, M, 16, ip))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", FAST4)
def test_scan4_k2_1024_flush_margin_zero(d, M, ip, monkeypatch):
    """BS 512, C 2, k2 = 1024: k2 + BS*C is the selector cap exactly, so
    the flush margin is 0 and every pass that pushed anything flushes.
    Row 1 of rows8 offers about 1900 candidates for the 1024 slots."""
    _knobs(monkeypatch, 512, 2)
    c = _case(d, M, 16, ip)
    assert 1800 < c.cands("rows8", False)[1].size < 2000
    _check(c, "rows8", 1, 1024)
    _check(c, "pairs", 1, 1024)
    _check(c, "rows8", 2, 1024)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", FAST4)
def test_scan4_k2_1030_generic_equals_fast(d, M, ip, monkeypatch):
    """k2 = 1030: at BS 512 / C 2 the dispatcher takes the generic kernel
    (1030 + 1024 exceeds the cap), at C 1 the fast one. Same keys, and the
    reference's."""
    c = _case(d, M, 16, ip)
    _knobs(monkeypatch, 512, 2)
    generic = [_check(c, name, 1, 1030) for name in ("rows8", "pairs")]
    _knobs(monkeypatch, 512, 1)
    fast = [_check(c, name, 1, 1030) for name in ("rows8", "pairs")]
    for g, f in zip(generic, fast):
        assert np.array_equal(g, f)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", FAST4 + GEN4)
def test_scan4_bitmap_and_qmap(d, M, ip):
    c = _case(d, M, 16, ip)
    _check(c, "rows8", 1, 200, bitmap=True, qmap=PERM)
    _check(c, "rows8", 4, 200, bitmap=True, qmap=PERM)
    _check(c, "pairs", 1, 1024, bitmap=True)
    _check(c, "pairs", 2, 10, qmap=PERM)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", [(128, 32), (24, 12)])
def test_scan4_kill_flag(d, M, ip):
    """A flag raised before the launch: every row EMPTY, ids -1. A flag
    left at 0 changes nothing."""
    c = _case(d, M, 16, ip)
    for name, S, k2 in (("rows8", 1, 10), ("pairs", 2, 1024)):
        keys, _, ids = c.run(name, S, k2, kill_flag=1)
        assert keys.shape == (8, S, k2)
        assert (keys == kr._EMPTY).all(), (name, S, k2)
        assert (ids == -1).all()
        _check(c, name, S, k2, kill_flag=0)


def test_scan4_refuses_code_offsets():
    c = _case(24, 12, 16, False)
    with pytest.raises(AssertionError):
        c.run("nprobe1", 1, 1, code_offsets={L[1100]: 4})


# ------------------------------------------- 8-bit resident-table kernel
_ALL8 = [(1, 200), (2, 10), (4, 1), (1, 1030)]
_DEEP8 = [(1, 1), (1, 10), (4, 200), (2, 1030)]


def _sweep8(c, **kw):
    from vearch_amd import ktest
    for k2 in (1, 10, 200, 1030):
        assert not ktest.ivfpq_wide_info(c.d, c.M, k2)[2]
    for name in c.tables:
        for S, k2 in _ALL8:
            _check(c, name, S, k2, **kw)
    for name in ("rows8", "pairs"):
        for S, k2 in _DEEP8:
            _check(c, name, S, k2, **kw)


@pytest.mark.parametrize("bs", [512, 256])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", FAST8)
def test_scan8_fast_m64_m96_rows(d, M, ip, bs, monkeypatch):
    from vearch_amd import ktest
    monkeypatch.setenv("GAMMA_SCAN_BS", str(bs))
    assert ktest.ivfpq_scan_reads_table(d, M, 1030, ip) is False
    _sweep8(_case(d, M, 256, ip))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", GEN8)
def test_scan8_generic_rows(d, M, ip):
    from vearch_amd import ktest
    assert ktest.ivfpq_scan_reads_table(d, M, 10, ip) is (not ip)
    c = _case(d, M, 256, ip)
    _sweep8(c)
    _check(c, "rows8", 1, 200, bitmap=True, qmap=PERM)
    _check(c, "pairs", 4, 200, bitmap=True, qmap=PERM)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", GEN8)
def test_scan8_generic_dword_aligned_lists(d, M, ip):
    """The generic path loads code dwords: lists whose codes start 4 and
    12 bytes into their allocation are within its contract."""
    c = _case(d, M, 256, ip)
    offs = {L[1100]: 4, L[513]: 12, L[257]: 4}
    for name, S, k2 in (("rows8", 1, 200), ("pairs", 2, 10),
                        ("2chunk+3", 1, 1030)):
        _check(c, name, S, k2, code_offsets=offs)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", [(48, 12)])
def test_scan8_generic_kill_flag(d, M, ip):
    """The list-by-list walk the 4-bit generic path shares, from its 8-bit
    side: a flag raised before the launch leaves every row EMPTY, ids -1;
    a flag left at 0 changes nothing."""
    c = _case(d, M, 256, ip)
    for name, S, k2 in (("rows8", 1, 10), ("pairs", 2, 1024)):
        keys, _, ids = c.run(name, S, k2, kill_flag=1)
        assert keys.shape == (8, S, k2)
        assert (keys == kr._EMPTY).all(), (name, S, k2)
        assert (ids == -1).all()
        _check(c, name, S, k2, kill_flag=0)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", FAST8)
def test_scan8_fast_m64_m96_bitmap_and_qmap(d, M, ip):
    c = _case(d, M, 256, ip)
    _check(c, "rows8", 1, 200, bitmap=True, qmap=PERM)
    _check(c, "pairs", 4, 200, bitmap=True, qmap=PERM)


# ------------------------------------------------------------- add order
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M,ksub", [
    (128, 32, 16), (24, 12, 16), (48, 12, 256), (384, 96, 256)],
    ids=["4bit-fast", "4bit-generic", "8bit-generic", "8bit-fast-m96"])
def test_add_order_on_gaussian_inputs(d, M, ksub, ip):
    """Off the grid the sums round, so only dis0, then the S term, then
    the table entries in ascending m reproduce the reference's keys."""
    c = _case(d, M, ksub, ip, gauss=True)
    _check(c, "rows8", 1, 200)
    _check(c, "pairs", 2, 1024, bitmap=True)
    _check(c, "2chunk+3", 1, 10)
