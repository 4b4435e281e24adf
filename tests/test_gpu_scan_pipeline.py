"""The 8-bit IVFPQ fast scan (k_ivfpq_scan, MW > 0) on its own, through
the kernel test hook: flattened probe chunks, the one-pass-ahead prefetch
and the table built in the kernel, against a numpy reference written
here.

Inputs sit on the exact grid of oracle.kernel_refs (values i/8), so every
table entry and every partial sum of a distance is exactly representable
in fp32; the reference still adds in the kernel's order (dis0, + S term,
then one fp32 add per sub-quantizer in ascending m). Keys are compared
with np.array_equal.

Shapes: 32 lists with sizes from {0, 1, 63, 64, 65, 255, 256, 257, 511,
512, 513, 1100} (block sizes 256 and 512 and their neighbours, one list of
several passes), at most 8 queries. The probe tables of `_LAUNCHES` hold
every row the kernel treats differently; see there."""
import os

import numpy as np
import pytest

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

PCH = 32  # GAMMA_SCAN_PCH of kernels.hip: probes per descriptor chunk
NLIST = 32
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1100,
         0, 1, 1, 1, 63, 64, 65, 1, 1, 1, 255, 256, 1, 0, 1, 1, 1, 1, 1, 1]
L = {s: SIZES.index(s) for s in set(SIZES)}  # first list of each size
NDOC = 8192  # ids are < NDOC (the bitmap's extent)
DMS = [(32, 16), (64, 16), (128, 32)]  # dsub 2 (scalar chain), 4, 4


def _probe_tables(SIZES=SIZES, small=(63, 64, 65)):
    """name -> int64 (nq, nprobe) probe table. SIZES: the list sizes
    (NLIST of them; 255..257, 511..513, 1100, 1, three empty lists and the
    three `small` sizes must occur)."""
    assert len(SIZES) == NLIST
    L = {s: SIZES.index(s) for s in set(SIZES)}
    s0, s1, s2 = small
    E = [i for i, s in enumerate(SIZES) if s == 0]  # the empty lists
    tiny = [i for i, s in enumerate(SIZES) if s <= 1]  # sizes 0 and 1
    rng = np.random.default_rng(5)
    a = np.array([
        [E[0], E[1], E[2], E[0], E[1], E[2], E[0], E[1]],  # all empty
        [-1, L[1100], NLIST, L[513], -1, NLIST + 7, L[257], L[s2]],
        [E[0], L[511], E[1], -1, E[2], NLIST, E[0], E[1]],  # total 511
        [L[512], E[0], E[1], -1, E[2], NLIST, E[0], E[1]],  # total 512
        [E[0], E[1], -1, E[2], NLIST, E[0], E[1], L[513]],  # total 513
        [L[255], E[0], E[1], -1, E[2], NLIST, E[0], E[1]],  # total 255
        [E[0], L[256], E[1], -1, E[2], NLIST, E[0], E[1]],  # total 256
        [L[s0], L[s1], L[s2], L[1], L[s1], E[0], -1, E[1]],  # total 257
    ], dtype=np.int64)
    assert [sum(SIZES[x] for x in r if 0 <= x < NLIST) for r in a[2:]] == [
        511, 512, 513, 255, 256, s0 + 2 * s1 + s2 + 1]
    one = np.array([[L[1100]], [E[0]], [-1], [L[1]], [NLIST]],
                   dtype=np.int64)  # nprobe = 1; three rows with total 0
    # more probes than a chunk holds, over tiny lists (ids repeat)
    c1 = rng.choice(tiny, size=(2, PCH + 1)).astype(np.int64)
    c2 = rng.choice(tiny, size=(2, 2 * PCH + 3)).astype(np.int64)
    c2[1, ::5] = -1
    c2[1, PCH] = L[513]  # a multi-pass list straddling the chunk boundary
    c2[1, PCH - 1] = L[257]
    return {"rows8": a, "nprobe1": one, "chunk+1": c1, "2chunk+3": c2}


class Case:
    """One (d, M, metric): model, lists and, per probe table, every
    candidate key of every query (computed once, never modified)."""

    def __init__(self, d, M, ip):
        self.d, self.M, self.ip = d, M, ip
        dsub = d // M
        rng = np.random.default_rng(1000 * d + M + int(ip))
        self.centroids = kr.grid((NLIST, d), seed=d + 1)
        self.codebooks = kr.grid((M, 256, dsub), seed=d + 2)
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
            self.lists.append((ids.astype(np.uint32), codes, svals))
        self.deleted = rng.random(NDOC) < 0.10  # the bitmap
        # exact tables: L2 A[q][m][j] = ||cw||^2 - 2 q_m.cw, IP T = q_m.cw
        q3 = self.queries.reshape(8, M, dsub).astype(np.float64)
        cb = self.codebooks.astype(np.float64)
        dots = np.einsum("qmt,mjt->qmj", q3, cb)
        tab = dots if ip else (cb * cb).sum(axis=2)[None] - 2.0 * dots
        self.tab = kr._exact_f32(tab)
        self.cdots = kr.dots_exact(self.queries, self.centroids)
        self.tables = _probe_tables()
        self.probe_dists = {
            name: kr.grid(t.shape, seed=len(name) + t.shape[1])
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
                dis = np.full(ids.shape, self.cdots[qi, ln], np.float32)
            else:
                dis0 = np.float32(self.probe_dists[name][qi, p])
                dis = (dis0 + svals).astype(np.float32)
            for m in range(self.M):  # fp32 add per sub-quantizer
                dis = (dis + self.tab[qi, m, codes[:, m]]).astype(np.float32)
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

    def run(self, name, S, k2, bitmap=False, qmap=None, kill_flag=None):
        from vearch_amd import ktest
        t = self.tables[name]
        nq = t.shape[0]
        return ktest.ivfpq_scan(
            self.lists, t, self.probe_dists[name], self.queries[:nq],
            self.centroids, self.codebooks, S, k2, self.ip,
            bitmap=kr.bitmap_words(self.deleted) if bitmap else None,
            qmap=qmap, kill_flag=kill_flag)


_cases = {}


def _case(d, M, ip):
    if (d, M, ip) not in _cases:
        _cases[(d, M, ip)] = Case(d, M, ip)
    return _cases[(d, M, ip)]


def _check(c, name, S, k2, **kw):
    keys, dists, ids = c.run(name, S, k2, **kw)
    want = c.expect(name, k2, bitmap=kw.get("bitmap", False))
    tag = f"{name} d={c.d} M={c.M} ip={c.ip} S={S} k2={k2} {kw}"
    if S == 1:  # the kernel's own rows, EMPTY padding included
        assert np.array_equal(keys[:, 0, :], want), tag
    # the engine's merge of the S partial rows, re-encoded as keys
    wd, wi = kr.key_decode(want, c.ip)
    got = np.where(ids < 0, kr._EMPTY, kr.key_encode(dists, ids, c.ip))
    assert np.array_equal(got, want), tag
    assert np.array_equal(ids, wi), tag
    assert np.array_equal(dists.view(np.uint32), wd.view(np.uint32)), tag


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", DMS)
def test_scan_rows(d, M, ip, S):
    c = _case(d, M, ip)
    for name in c.tables:
        for k2 in (1, 10, 200):
            _check(c, name, S, k2)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", DMS)
def test_scan_bitmap_and_qmap(d, M, ip):
    c = _case(d, M, ip)
    _check(c, "rows8", 1, 200, bitmap=True)
    _check(c, "2chunk+3", 2, 10, bitmap=True)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)
    _check(c, "rows8", 1, 10, qmap=perm)
    _check(c, "rows8", 4, 200, qmap=perm, bitmap=True)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", DMS)
def test_scan_block_256(d, M, ip, monkeypatch):
    monkeypatch.setenv("GAMMA_SCAN_BS", "256")
    assert os.environ["GAMMA_SCAN_BS"] == "256"
    c = _case(d, M, ip)
    for name in c.tables:
        for S, k2 in ((1, 200), (2, 10), (4, 1)):
            _check(c, name, S, k2)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_scan_large_k2_checks_every_pass(ip):
    """k2 + 2*512 > 2048: the flush check runs every pass, not every
    second one; 1900 candidates against 1018 free slots force flushes."""
    c = _case(128, 32, ip)
    _check(c, "rows8", 1, 1030)
    _check(c, "2chunk+3", 1, 1030)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_scan_kill_flag(ip):
    """A flag raised before the launch is read at the first chunk close:
    the launch returns and every row is EMPTY. A flag left at 0 changes
    nothing."""
    c = _case(32, 16, ip)
    for S, k2 in ((1, 10), (2, 1024)):
        keys, _, ids = c.run("2chunk+3", S, k2, kill_flag=1)
        assert keys.shape == (2, S, k2)
        assert (keys == kr._EMPTY).all(), (S, k2)
        assert (ids == -1).all()
        _check(c, "2chunk+3", S, k2, kill_flag=0)


def test_scan_adc_c_knob_is_inert(monkeypatch):
    """GAMMA_ADC_C stays accepted on the 8-bit path and changes nothing."""
    monkeypatch.setenv("GAMMA_ADC_C", "2")
    c = _case(128, 32, False)
    _check(c, "rows8", 1, 200)
    _check(c, "2chunk+3", 2, 10)


@pytest.mark.parametrize("d,M", DMS + [(96, 16), (768, 96)])
def test_lut_builder_matches_pq_tables_a(d, M):
    """The table the scan builds in LDS, bit for bit against
    gk::pq_tables_a, on Gaussian inputs (nq = 3)."""
    import torch
    from vearch_amd import ktest
    rng = np.random.default_rng(d * 7 + M)
    q = torch.from_numpy(
        rng.standard_normal((3, d)).astype(np.float32)).cuda()
    cb = torch.from_numpy(
        rng.standard_normal((M, 256, d // M)).astype(np.float32)).cuda()
    want = ktest.pq_tables_a(q, cb, M, 256).cpu().numpy()
    got = ktest.pq_lut_l2(q, cb, M, 256).cpu().numpy()
    assert not np.isnan(want).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
