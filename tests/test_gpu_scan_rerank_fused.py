"""The re-rank + top-k epilogue of k_ivfpq_scan (rerank_epilogue.hpp),
through the kernel test hook: a launch WITH the re-rank block against the
chain of the existing hooks ktest.ivfpq_scan -> ktest.rerank ->
ktest.sort_rows on the same inputs. The candidate set, the fmaf chain and
the final (dist, id) order are the same, so (dists, ids) are compared with
np.array_equal, no tolerance.

Lists, list sizes and probe tables are those of test_gpu_scan_pipeline.py
(32 lists, at most 8 queries); the raw store is NDOC on-grid vectors (values
i/8), so exact distances tie and the id tie-break decides. On the grid an
exact L2 distance or dot product is representable in fp32 whatever the
order of the adds, which gives one check that does not go through the
chain: the fused distances equal the float64 ones of base[ids].

Rounds of the epilogue (candidates per round = what the query table's LDS
stages: 62 at M = 8, 124 at M = 16, 248 at M = 32, at most 256 / 128 for
512 / 256 threads): k2 = 200 is 4 / 2 / 1 rounds, k2 = 1024 is 9 / 5; d = 96
and d = 128 are 3 and 4 slices per round, d = 32 one, d = 40 a partial
second one."""
import numpy as np
import pytest

import test_gpu_scan_pipeline as sp
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

DMS = [(32, 16), (96, 16), (128, 32)]
# k2 in {1, 65, 200, 1024} x k in {1, 10, k2}: every pair
K2K = [(1, 1), (1, 10), (65, 1), (65, 10), (65, 65), (200, 1), (200, 10),
       (200, 200), (1024, 1), (1024, 10), (1024, 1024)]
SHIFT8 = 10  # ids < 8192 span 8 segments


class RCase(sp.Case):
    """A scan case plus the raw store, the raw-space queries and a probe
    table of rows with fewer than k2 candidates."""

    def __init__(self, d, M, ip):
        super().__init__(d, M, ip)
        self.base = kr.grid((sp.NDOC, d), seed=7 * d + M)
        self.rrq = kr.grid((8, d), seed=7 * d + M + 1)  # != self.queries
        live1 = [i for i, s in enumerate(sp.SIZES)
                 if s == 1 and not (self.lists[i][0][0] >> 31)]
        assert len(live1) >= 4
        self.nfew = min(10, len(live1))  # the row with exactly k candidates
        E = [i for i, s in enumerate(sp.SIZES) if s == 0]
        few = np.full((3, 16), -1, dtype=np.int64)
        few[0, :3] = E[:3]               # no candidate at all
        few[1, :3] = [E[0], live1[1], E[1]]  # exactly one
        few[2, :self.nfew] = live1[:self.nfew]
        self.tables = dict(self.tables, few=few)
        self.probe_dists = dict(self.probe_dists,
                                few=kr.grid(few.shape, seed=11))


_rcases = {}


def _rcase(d, M, ip):
    if (d, M, ip) not in _rcases:
        _rcases[(d, M, ip)] = RCase(d, M, ip)
    return _rcases[(d, M, ip)]


def _scan_args(c, name, k2, bitmap, qmap):
    t = c.tables[name]
    nq = t.shape[0]
    return (c.lists, t, c.probe_dists[name], c.queries[:nq], c.centroids,
            c.codebooks, 1, k2, c.ip), dict(bitmap=bitmap, qmap=qmap)


def _chain(c, name, k2, k, seg_shift, rrq, bitmap=None, qmap=None):
    """scan -> rerank -> sort_rows, each through its own existing hook"""
    import torch
    from vearch_amd import ktest
    a, kw = _scan_args(c, name, k2, bitmap, qmap)
    keys, _, _ = ktest.ivfpq_scan(*a, **kw)
    nq = keys.shape[0]
    segs = ktest.split_segments(c.base, seg_shift)
    q_d = torch.from_numpy(np.ascontiguousarray(rrq[:nq])).cuda()
    rk = ktest.rerank(q_d, segs, seg_shift, c.ip,
                      ktest.keys_to_dev(keys[:, 0, :]))
    od, oi = ktest.sort_rows(rk, k, c.ip)
    return od.cpu().numpy(), oi.cpu().numpy()


def _fused(c, name, k2, k, seg_shift, rrq, bitmap=None, qmap=None):
    from vearch_amd import ktest
    a, kw = _scan_args(c, name, k2, bitmap, qmap)
    nq = a[1].shape[0]
    return ktest.ivfpq_scan_rerank(*a, c.base, seg_shift, k,
                                   rr_queries=rrq[:nq], **kw)


def _exact(c, rrq, ids):
    """float64 distances of base[ids] to the raw queries (-1 where id -1)"""
    v = c.base[np.maximum(ids, 0)].astype(np.float64)
    q = rrq[:ids.shape[0], None, :].astype(np.float64)
    e = (q * v).sum(axis=2) if c.ip else ((q - v) ** 2).sum(axis=2)
    return np.where(ids < 0, -1.0, e)


def _check(c, name, k2, k, seg_shift=SHIFT8, rrq=None, **kw):
    rrq = c.rrq if rrq is None else rrq
    gd, gi = _fused(c, name, k2, k, seg_shift, rrq, **kw)
    wd, wi = _chain(c, name, k2, k, seg_shift, rrq, **kw)
    tag = f"{name} d={c.d} M={c.M} ip={c.ip} k2={k2} k={k} {seg_shift}"
    assert np.array_equal(gi, wi), tag
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), tag
    assert np.array_equal(gd.astype(np.float64), _exact(c, rrq, gi)), tag
    return gd, gi


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", DMS)
def test_fused_matches_chain(d, M, ip):
    """every (k2, k) pair on the eight-row table; candidates of one row
    come from several of the 8 segments"""
    c = _rcase(d, M, ip)
    for k2, k in K2K:
        gd, gi = _check(c, "rows8", k2, k)
        assert (gi[0] == -1).all() and (gd[0] == -1.0).all()  # all empty
        assert (gi[1:, 0] >= 0).all()
    _, gi = _check(c, "rows8", 200, 200)
    for r in range(1, 8):
        assert len(set((gi[r][gi[r] >= 0] >> SHIFT8).tolist())) > 1, r


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", DMS)
def test_fused_other_probe_tables(d, M, ip):
    """nprobe = 1, more probes than a chunk over tiny lists (the same id
    arrives from several probes), and the rows with fewer than k2
    candidates: none, exactly one, exactly k"""
    c = _rcase(d, M, ip)
    for name in ("nprobe1", "chunk+1", "2chunk+3"):
        _check(c, name, 200, 10)
        _check(c, name, 65, 65)
    cand = c.cands("2chunk+3", False)[0]
    assert np.unique(cand & 0xFFFFFFFF).size < cand.size  # ids do repeat
    for k2, k in ((200, c.nfew), (c.nfew, c.nfew), (65, 1)):
        gd, gi = _check(c, "few", k2, k)
        assert (gi[0] == -1).all() and (gd[0] == -1.0).all()
        assert gi[1, 0] >= 0 and (gi[1, 1:] == -1).all()
        assert (gd[1, 1:] == -1.0).all()
    assert [len(x) for x in c.cands("few", False)] == [0, 1, c.nfew]
    _, gi = _check(c, "few", 200, c.nfew)
    assert (gi[2] >= 0).all()
    _, gi = _check(c, "few", 200, c.nfew + 1)
    assert (gi[2, :c.nfew] >= 0).all() and gi[2, c.nfew] == -1


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", [(32, 8), (40, 20)])
def test_fused_generic_kernel(d, M, ip):
    """M outside {16, 32, 64, 96}: the generic kernel (256 threads, the
    table read from atab). M = 8 stages 62 rows a round; d = 40 ends in a
    partial slice."""
    c = _rcase(d, M, ip)
    for k2, k in ((200, 10), (1024, 1024), (1, 1), (65, 65)):
        _check(c, "rows8", k2, k)
    _check(c, "2chunk+3", 200, 200)
    _check(c, "few", 65, 10)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_fused_block_256(ip, monkeypatch):
    monkeypatch.setenv("GAMMA_SCAN_BS", "256")
    for d, M in DMS:
        c = _rcase(d, M, ip)
        _check(c, "rows8", 200, 10)
        _check(c, "rows8", 1024, 1024)
        _check(c, "few", 65, 1)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_fused_other_fast_tables(ip):
    """the M = 64 and M = 96 instantiations: a 64 KB or 96 KB table, one
    workgroup on a CU; a round stages 256 rows"""
    from vearch_amd import ktest
    for d, M in ((128, 64), (192, 96)):
        c = _rcase(d, M, ip)
        assert ktest.ivfpq_scan_can_fuse_rerank(d, M, 200, 1)
        _check(c, "rows8", 200, 10)
        _check(c, "rows8", 1024, 1024)
        _check(c, "few", 65, 1)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_fused_many_segments(ip):
    """seg_shift = 6: 128 segments, more than k_rerank_lds caches"""
    for d, M in ((128, 32), (96, 16)):
        c = _rcase(d, M, ip)
        _check(c, "rows8", 200, 200, seg_shift=6)
        _check(c, "2chunk+3", 65, 10, seg_shift=6)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", DMS)
def test_fused_bitmap_qmap_and_raw_queries(d, M, ip):
    c = _rcase(d, M, ip)
    # a bitmap that deletes the three best re-ranked candidates of a row
    _, gi0 = _check(c, "rows8", 200, 10)
    deleted = c.deleted.copy()
    top = gi0[1:, :3].ravel()
    deleted[top[top >= 0]] = True
    bm = kr.bitmap_words(deleted)
    _, gi1 = _check(c, "rows8", 200, 10, bitmap=bm)
    assert not deleted[gi1[gi1 >= 0]].any()
    assert not np.array_equal(gi0[1:], gi1[1:])
    # a query schedule: outputs land on the original rows
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)
    _, gi2 = _check(c, "rows8", 200, 10, qmap=perm)
    assert np.array_equal(gi2, gi0)
    _check(c, "rows8", 65, 65, qmap=perm, bitmap=bm)
    # the re-rank measures against rr_queries, not the scan's queries:
    # same candidates, other distances
    gd3, _ = _check(c, "rows8", 200, 10, rrq=c.queries)
    gd0, _ = _check(c, "rows8", 200, 10)
    assert not np.array_equal(gd3[1:], gd0[1:])


def test_refusals(monkeypatch):
    """A launch that cannot fuse, with the block set, is an error from the
    launcher (hipErrorInvalidValue = 1) and launches nothing."""
    from vearch_amd import ktest
    can = ktest.ivfpq_scan_can_fuse_rerank
    assert can(128, 32, 200, 1) and can(32, 16, 1024, 1) and can(32, 8, 1, 1)
    assert can(768, 96, 200, 1)                 # one workgroup per CU
    assert not can(128, 32, 200, 2)             # probe split
    assert not can(128, 32, 200, 1, ksub=16)    # 4-bit codes
    assert not can(640, 160, 200, 1)            # sliced-table kernel
    c = _rcase(128, 32, False)
    a, kw = _scan_args(c, "rows8", 200, None, None)
    a2 = a[:6] + (2,) + a[7:]
    with pytest.raises(ktest.KTestError) as ei:
        ktest.ivfpq_scan_rerank(*a2, c.base, SHIFT8, 10)
    assert ei.value.code == 1
    with pytest.raises(ktest.KTestError):  # k beyond the sort scratch
        ktest.ivfpq_scan_rerank(*a, c.base, SHIFT8, 4096)
    monkeypatch.setenv("GAMMA_SCAN_WIDE", "1")
    assert not can(128, 32, 200, 1)
    with pytest.raises(ktest.KTestError):
        ktest.ivfpq_scan_rerank(*a, c.base, SHIFT8, 10)
    monkeypatch.delenv("GAMMA_SCAN_WIDE")
    monkeypatch.setenv("GAMMA_FUSE_RERANK", "0")
    assert not can(128, 32, 200, 1)
    with pytest.raises(ktest.KTestError):
        ktest.ivfpq_scan_rerank(*a, c.base, SHIFT8, 10)
    monkeypatch.delenv("GAMMA_FUSE_RERANK")
    assert can(128, 32, 200, 1)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_null_block_is_the_plain_launch(ip):
    """No re-rank block: exactly the out_keys of ktest.ivfpq_scan, for the
    fast and the generic kernel and for S > 1."""
    from vearch_amd import ktest
    for d, M in ((128, 32), (32, 8)):
        c = _rcase(d, M, ip)
        for S, k2 in ((1, 200), (2, 10)):
            a, kw = _scan_args(c, "rows8", k2, None, None)
            a = a[:6] + (S,) + a[7:]
            want, _, _ = ktest.ivfpq_scan(*a, **kw)
            got = ktest.ivfpq_scan_null_rerank(*a, **kw)
            assert np.array_equal(got, want), (d, M, S, k2)
            assert np.array_equal(want, c.expect("rows8", k2)[:, None, :]) \
                or S > 1
