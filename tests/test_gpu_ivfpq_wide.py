"""The sliced-table 8-bit IVFPQ scan (k_ivfpq_scan_wide) on its own,
through the kernel test hook: tables too wide for the resident-table kernel
(M >= 144), and narrow ones forced onto it with GAMMA_SCAN_WIDE=1, against
a numpy reference written here in the manner of test_gpu_scan_pipeline.

Inputs sit on the exact grid of oracle.kernel_refs (values i/8), so every
table entry and every partial sum of a distance is exactly representable
in fp32; the reference still adds in the kernel's order (dis0, + S term,
then one fp32 add per sub-quantizer in ascending m). Keys are compared
with np.array_equal.

The kernel walks tiles of T = 4 x block size entries (2048 at the default
512 threads, 1024 under GAMMA_SCAN_BS=256) and table slices of 32
sub-quantizers. List sizes are 0, 1 and BS-1, BS, BS+1, T-1, T, T+1 for
both block sizes; shapes give 4.5 slices (M=144), an odd last slice on
4-byte-aligned entries (M=148) and 5 whole slices (M=160). At most 8
queries.

On the grid any order of the adds gives the same bits, so one more case
per shape runs on Gaussian codebooks, S terms and probe distances
(`gauss=True`): its table is the device's own (gk::pq_tables_a /
gk::pq_tables_ip, each pinned on its own), and the reference's serial fp32
chain in ascending m is then the only order that reproduces the keys."""
import numpy as np
import pytest

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

PCH = 32  # GAMMA_SCAN_PCH of kernels.hip: probes per descriptor chunk
SIZES = [0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
         2049, 0, 0, 1, 1, 1, 1]
NLIST = len(SIZES)
L = {s: SIZES.index(s) for s in set(SIZES)}  # first list of each size
NDOC = 16384  # ids are < NDOC (the bitmap's extent)
WIDE_DMS = [(144, 144), (148, 148), (288, 144), (640, 160)]
K2S = (1, 10, 200, 1024)


def test_constants_match_the_library():
    from vearch_amd import ktest
    ms, tile, wide = ktest.ivfpq_wide_info(144, 144, 10)
    assert (ms, tile, wide) == (ktest.WIDE_MS, 512 * ktest.WIDE_E, True)
    assert (ms, tile) == (32, 2048)
    assert 2048 in SIZES and 1024 in SIZES  # T at both block sizes
    for d, M in WIDE_DMS:
        for k2 in K2S:
            assert ktest.ivfpq_wide_info(d, M, k2)[2], (d, M, k2)
    assert not ktest.ivfpq_wide_info(128, 32, 1024)[2]


def test_reads_table_decision():
    """gk::ivfpq_scan_reads_table is what IVFIndex::search builds its
    query table by. Every wide launch reads one, for both metrics — also
    at M = 96, a size whose resident kernel builds its own L2 table, once
    4*d pushes the launch over the LDS limit (d = 12000 at any k2,
    d = 10080 at k2 = 1024 but not at k2 = 1)."""
    from vearch_amd.ktest import ivfpq_scan_reads_table as reads
    from vearch_amd.ktest import ivfpq_wide_info as info
    for ip in (False, True):
        assert info(12000, 96, 1)[2] and reads(12000, 96, 1, ip)
        assert info(12000, 96, 1024)[2] and reads(12000, 96, 1024, ip)
        assert info(10080, 96, 1024)[2] and reads(10080, 96, 1024, ip)
        assert reads(144, 144, 10, ip) and reads(136, 136, 1024, ip)
        assert not info(10080, 96, 1)[2] and not reads(10080, 96, 1, ip)
        assert not reads(128, 32, 10, ip)  # fast path: builds its own
    # generic resident kernel: L2 reads atab, inner product builds its own
    assert reads(192, 48, 10, False) and not reads(192, 48, 10, True)
    assert reads(136, 136, 10, False) and not reads(136, 136, 10, True)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_fast_m_made_wide_by_d(ip):
    """d = 12000, M = 96 (dsub 125) without forcing: the sliced kernel
    with three whole slices and, for inner product, a 48 000-byte query in
    LDS. Grid sums stay exact at this d (below 2^24 units of 2^-6)."""
    from vearch_amd import ktest
    assert ktest.ivfpq_wide_info(12000, 96, 1)[2]
    c = _case(12000, 96, ip)
    _check(c, "tiles", 1, 10)
    _check(c, "blocks", 2, 1024, bitmap=True)
    _check(c, "2chunk+3", 4, 200)


def _probe_tables():
    """name -> int64 (nq, nprobe) probe table."""
    E = [i for i, s in enumerate(SIZES) if s == 0]  # the empty lists
    tiny = [i for i, s in enumerate(SIZES) if s <= 1]  # sizes 0 and 1
    rng = np.random.default_rng(7)
    pad = [E[0], -1, E[1], NLIST, E[2], E[0]]
    # tile sizes and neighbours, alone in their chunk; row 1 mixes -1,
    # ids >= nlist and four lists whose flat total (2820) spans two tiles
    # of 2048 (three of 1024) with every boundary inside the first list
    tiles = np.array([
        [E[0], E[1], E[2], E[0], E[1], E[2], E[0], E[1]],  # all empty
        [-1, L[2049], NLIST, L[513], -1, NLIST + 7, L[257], L[1]],
        [L[2047], E[0]] + pad,
        [E[1], L[2048]] + pad,
        pad + [E[2], L[2049]],
        [L[1023], E[0]] + pad,
        [E[1], L[1024]] + pad,
        pad + [L[1025], E[2]],
    ], dtype=np.int64)
    # block sizes and neighbours; the last row's total (3585) puts the
    # 2048 boundary inside its second list and 1024 inside its first
    blocks = np.array([
        [L[255], E[0]] + pad,
        [E[1], L[256]] + pad,
        pad + [L[257], E[2]],
        [L[511], E[0]] + pad,
        [E[1], L[512]] + pad,
        pad + [L[513], E[2]],
        [L[1], E[0]] + pad,
        [L[1025], -1, L[2047], E[0], NLIST, L[513], E[1], -1],
    ], dtype=np.int64)
    one = np.array([[L[2049]], [E[0]], [-1], [L[1]], [NLIST]],
                   dtype=np.int64)  # nprobe = 1; three rows with total 0
    # more probes than a chunk holds, over tiny lists (ids repeat), with
    # multi-tile lists on both sides of the chunk boundary
    c2 = rng.choice(tiny, size=(2, 2 * PCH + 3)).astype(np.int64)
    c2[1, ::5] = -1
    c2[1, PCH - 1] = L[2049]
    c2[1, PCH] = L[1025]
    return {"tiles": tiles, "blocks": blocks, "nprobe1": one,
            "2chunk+3": c2}


class Case:
    """One (d, M, metric): model, lists and, per probe table, every
    candidate key of every query (computed once, never modified)."""

    def __init__(self, d, M, ip, gauss=False):
        self.d, self.M, self.ip = d, M, ip
        dsub = d // M
        rng = np.random.default_rng(1000 * d + M + int(ip) + 7 * gauss)
        f32n = lambda shape: rng.standard_normal(shape).astype(  # noqa: E731
            np.float32)
        self.centroids = kr.grid((NLIST, d), seed=d + 1)
        self.codebooks = (f32n((M, 256, dsub)) if gauss
                          else kr.grid((M, 256, dsub), seed=d + 2))
        self.queries = kr.grid((8, d), seed=d + 3)
        self.lists = []
        ids_pool = rng.permutation(NDOC)
        at = 0
        for n in SIZES:
            ids = ids_pool[at:at + n].astype(np.uint32)
            at += n
            dead = rng.random(n) < 0.06  # delete marks: bit 31
            ids = np.where(dead, ids | np.uint32(0x80000000), ids)
            codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
            svals = kr.grid((n,), seed=int(rng.integers(1 << 30)))
            if gauss:
                svals = f32n((n,))
            self.lists.append((ids.astype(np.uint32), codes, svals))
        self.deleted = rng.random(NDOC) < 0.10  # the bitmap
        # exact tables: L2 A[q][m][j] = ||cw||^2 - 2 q_m.cw, IP T = q_m.cw
        if gauss:  # the device's own table, bit for bit
            self.tab = _device_table(self.queries, self.codebooks, M, ip)
        else:
            q3 = self.queries.reshape(8, M, dsub).astype(np.float64)
            cb = self.codebooks.astype(np.float64)
            dots = np.einsum("qmt,mjt->qmj", q3, cb)
            tab = dots if ip else (cb * cb).sum(axis=2)[None] - 2.0 * dots
            self.tab = kr._exact_f32(tab)
        self.cdots = kr.dots_exact(self.queries, self.centroids)
        self.tables = _probe_tables()
        self.probe_dists = {
            name: (f32n(t.shape) if gauss
                   else kr.grid(t.shape, seed=len(name) + t.shape[1]))
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
        marange = np.arange(self.M)
        for p, ln in enumerate(self.tables[name][qi]):
            if ln < 0 or ln >= NLIST or SIZES[ln] == 0:
                continue
            ids, codes, svals = self.lists[ln]
            if self.ip:
                dis = np.full(ids.shape, self.cdots[qi, ln], np.float32)
            else:
                dis0 = np.float32(self.probe_dists[name][qi, p])
                dis = (dis0 + svals).astype(np.float32)
            terms = self.tab[qi][marange[None, :], codes]  # (n, M) f32
            for m in range(self.M):  # fp32 add per sub-quantizer
                dis = (dis + terms[:, m]).astype(np.float32)
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
            qmap=qmap, kill_flag=kill_flag, code_offsets=code_offsets)


def _device_table(queries, codebooks, M, ip):
    import torch
    from vearch_amd import ktest
    q = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    cb = torch.from_numpy(np.ascontiguousarray(codebooks)).cuda()
    t = ktest.pq_tables_ip(q, cb, M) if ip else ktest.pq_tables_a(
        q, cb, M, 256)
    t = t.cpu().numpy()
    assert not np.isnan(t).any()
    return t


_cases = {}


def _case(d, M, ip, gauss=False):
    if (d, M, ip, gauss) not in _cases:
        _cases[(d, M, ip, gauss)] = Case(d, M, ip, gauss)
    return _cases[(d, M, ip, gauss)]


def _check_keys(keys, dists, ids, want, ip, S, k2, tag):
    nq = want.shape[0]
    assert keys.shape == (nq, S, k2), tag
    if S == 1:  # the kernel's own rows, EMPTY padding included
        assert np.array_equal(keys[:, 0, :], want), tag
    # the S partial rows together hold exactly the top-k2 (EMPTY sorts last)
    merged = np.sort(keys.reshape(nq, S * k2), axis=1)[:, :k2]
    assert np.array_equal(merged, want), tag
    if dists is None:  # S * k2 beyond the engine's single-row merge
        return
    wd, wi = kr.key_decode(want, ip)
    got = np.where(ids < 0, kr._EMPTY, kr.key_encode(dists, ids, ip))
    assert np.array_equal(got, want), tag
    assert np.array_equal(ids, wi), tag
    assert np.array_equal(dists.view(np.uint32), wd.view(np.uint32)), tag


def _check(c, name, S, k2, **kw):
    keys, dists, ids = c.run(name, S, k2, **kw)
    want = c.expect(name, k2, bitmap=kw.get("bitmap", False))
    tag = f"{name} d={c.d} M={c.M} ip={c.ip} S={S} k2={k2} {kw}"
    _check_keys(keys, dists, ids, want, c.ip, S, k2, tag)


@pytest.mark.parametrize("d,M", WIDE_DMS + [(128, 32)])
def test_ip_table_is_the_serial_fmaf_chain(d, M):
    """gk::pq_tables_ip on Gaussian codebooks and grid queries: acc =
    fmaf(q_t, cw_t, acc) in ascending t. A grid value times an fp32 value
    is exact in float64 and so is its sum with an fp32 accumulator of
    comparable size, so float64 arithmetic rounded to fp32 after every
    step is that chain."""
    rng = np.random.default_rng(d + M)
    dsub = d // M
    q = kr.grid((3, d), seed=d + 11)
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    got = _device_table(q, cb, M, True)
    q3 = q.reshape(3, M, dsub).astype(np.float64)
    acc = np.zeros((3, M, 256), dtype=np.float32)
    for t in range(dsub):
        acc = (q3[:, :, None, t] * cb[None, :, :, t].astype(np.float64) +
               acc.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), acc.view(np.uint32))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", WIDE_DMS)
def test_wide_add_order_on_gaussian_inputs(d, M, ip):
    """Off the grid the sums round, so only the kernel's order (ascending
    m across slices and inside them) reproduces the reference's keys."""
    c = _case(d, M, ip, gauss=True)
    _check(c, "tiles", 1, 200)
    _check(c, "blocks", 2, 1024, bitmap=True)
    _check(c, "2chunk+3", 1, 10)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", [(144, 144), (640, 160)])
def test_wide_misaligned_lists(d, M, ip):
    """M % 16 == 0 takes 16-byte code loads only where every list of the
    chunk is 16-byte aligned. Lists whose codes start 4, 8 or 12 bytes
    into their allocation, in chunks shared with aligned lists, fall back
    to single words for that chunk; a later chunk is aligned again."""
    c = _case(d, M, ip)
    offs = {L[2049]: 4, L[513]: 8, L[1025]: 12, L[1]: 4}
    for name in c.tables:
        for S, k2 in ((1, 200), (2, 1024)):
            _check(c, name, S, k2, code_offsets=offs)
    _check(c, "tiles", 1, 10, code_offsets={L[257]: 4}, bitmap=True)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", WIDE_DMS)
def test_wide_rows(d, M, ip, S):
    c = _case(d, M, ip)
    for name in c.tables:
        for k2 in K2S:
            _check(c, name, S, k2)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", WIDE_DMS)
def test_wide_bitmap_and_qmap(d, M, ip):
    c = _case(d, M, ip)
    _check(c, "tiles", 1, 200, bitmap=True)
    _check(c, "blocks", 1, 1024, bitmap=True)
    _check(c, "2chunk+3", 2, 10, bitmap=True)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)
    _check(c, "tiles", 1, 10, qmap=perm)
    _check(c, "blocks", 4, 200, qmap=perm, bitmap=True)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", WIDE_DMS)
def test_wide_block_256(d, M, ip, monkeypatch):
    """GAMMA_SCAN_BS=256: tiles of 1024 entries."""
    from vearch_amd import ktest
    monkeypatch.setenv("GAMMA_SCAN_BS", "256")
    assert ktest.ivfpq_wide_info(d, M, 10)[1] == 1024
    c = _case(d, M, ip)
    for name in c.tables:
        for S, k2 in ((1, 200), (2, 1024), (4, 1), (1, 10)):
            _check(c, name, S, k2)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", [(32, 16), (128, 32)])
def test_forced_wide_equals_unforced(d, M, ip, monkeypatch):
    """Tables narrower than one slice, forced onto the sliced kernel: the
    keys of the unforced (resident-table) launch, and the reference's."""
    import test_gpu_scan_pipeline as sp
    from vearch_amd import ktest
    c = sp._case(d, M, ip)
    launches = [(name, S, k2) for name in c.tables
                for S, k2 in ((1, 200), (2, 10), (4, 1), (1, 1024))]
    assert not ktest.ivfpq_wide_info(d, M, 1024)[2]
    plain = [c.run(name, S, k2)[0] for name, S, k2 in launches]
    monkeypatch.setenv("GAMMA_SCAN_WIDE", "1")
    assert ktest.ivfpq_wide_info(d, M, 1)[2]
    for (name, S, k2), pk in zip(launches, plain):
        keys, dists, ids = c.run(name, S, k2)
        tag = f"forced {name} d={d} M={M} ip={ip} S={S} k2={k2}"
        assert np.array_equal(keys, pk), tag
        _check_keys(keys, dists, ids, c.expect(name, k2), ip, S, k2, tag)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)
    keys, dists, ids = c.run("rows8", 2, 200, bitmap=True, qmap=perm)
    _check_keys(keys, dists, ids, c.expect("rows8", 200, bitmap=True), ip,
                2, 200, "forced bitmap+qmap")


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", [(144, 144), (640, 160)])
def test_wide_kill_flag(d, M, ip):
    """A flag raised before the launch: the launch returns and every row
    is EMPTY. A flag left at 0 changes nothing."""
    c = _case(d, M, ip)
    for S, k2 in ((1, 10), (2, 1024)):
        keys, _, ids = c.run("tiles", S, k2, kill_flag=1)
        assert keys.shape == (8, S, k2)
        assert (keys == kr._EMPTY).all(), (S, k2)
        if ids is not None:
            assert (ids == -1).all()
        _check(c, "tiles", S, k2, kill_flag=0)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_kernel_switch_at_m136(ip):
    """M = 136: k2 = 10 fits the resident table, k2 = 1024 does not, so one
    table is served by both kernels. Same first 10 keys per row."""
    from vearch_amd import ktest
    d = M = 136
    assert not ktest.ivfpq_wide_info(d, M, 10)[2]
    assert ktest.ivfpq_wide_info(d, M, 1024)[2]
    c = _case(d, M, ip)
    for name in c.tables:
        small = c.run(name, 1, 10)[0]
        large = c.run(name, 1, 1024)[0]
        assert np.array_equal(small[:, 0, :], large[:, 0, :10]), name
        assert np.array_equal(small[:, 0, :], c.expect(name, 10)), name
        assert np.array_equal(large[:, 0, :], c.expect(name, 1024)), name
