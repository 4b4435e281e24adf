"""The list bound of the 8-bit L2 fast scan (gk::ivfpq_scan with a pruning
block, DESIGN.md "Kernels" item 3) through the kernel test hooks.

Every launch is compared byte for byte with the same launch under
GAMMA_SCAN_PRUNE=0, and at S = 1 with a numpy reference: the table the
kernel builds (gk::pq_lut_l2_dump), oracle.kernel_refs.adc_chain from
dis0 + S_v, top-k2 by key. The counting kernel says what was skipped, so no
case passes by never skipping (or by skipping where it must not).

Shapes: d = 32, M = 16 (the smallest M of the pruning kernel), 64 lists of 0..700 entries (empty and all-deleted
ones among them), 64 queries, 16 probes. Models are geometric: an entry is
its list centroid plus its decoded residual, S_v = 2 c.r, dis0 = ||q - c||^2,
which is what the bound assumes of its inputs."""
import os

import numpy as np
import pytest

from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

D, M, NLIST, NQ, NPROBE, NDOC = 32, 16, 64, 64, 16, 1 << 16
DSUB = D // M


@pytest.fixture(autouse=True)
def _bound_on(monkeypatch):
    """every launch here carries the bound unless it says otherwise"""
    monkeypatch.setenv("GAMMA_SCAN_PRUNE", "1")
    monkeypatch.delenv("GAMMA_SCAN_PRUNE_HEAD", raising=False)


def _env(**kv):
    class _E:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kv}
            for k, v in kv.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = str(v)

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


class Model:
    """centroids (nlist, D), sizes per list, queries: lists, probes, dis0."""

    def __init__(self, centroids, sizes, queries, seed, cw_sigma=0.05,
                 dead_lists=()):
        rng = np.random.default_rng(seed)
        self.centroids = centroids.astype(np.float32)
        self.queries = queries.astype(np.float32)
        nlist = len(sizes)
        self.codebooks = (rng.standard_normal((M, 256, DSUB)) *
                          cw_sigma).astype(np.float32)
        pool = rng.permutation(NDOC)
        at = 0
        self.lists = []
        cb64 = self.codebooks.astype(np.float64)
        for ln, n in enumerate(sizes):
            ids = pool[at:at + n].astype(np.uint32)
            at += n
            dead = rng.random(n) < 0.05
            if ln in dead_lists:
                dead[:] = True
            ids = np.where(dead, ids | np.uint32(0x80000000), ids)
            codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
            dec = cb64[np.arange(M)[None, :], codes].reshape(n, D)
            sv = (2.0 * dec @ self.centroids[ln].astype(np.float64))
            self.lists.append((ids.astype(np.uint32), codes,
                               sv.astype(np.float32)))
        self.base = np.zeros((NDOC, D), np.float32)  # raw store for re-rank
        for ln, (ids, codes, _) in enumerate(self.lists):
            dec = cb64[np.arange(M)[None, :], codes].reshape(len(ids), D)
            self.base[ids & 0x7FFFFFFF] = (self.centroids[ln] + dec)
        self.deleted = rng.random(NDOC) < 0.9  # the heavy filter
        d2 = ((self.queries[:, None, :].astype(np.float64) -
               self.centroids[None].astype(np.float64)) ** 2).sum(axis=2)
        nprobe = min(NPROBE, nlist)
        self.probes = np.argsort(d2, axis=1, kind="stable")[:, :nprobe]
        self.probes = self.probes.astype(np.int64)
        self.dis0 = np.take_along_axis(d2, self.probes, 1).astype(np.float32)
        self._tab = None

    def table(self):
        if self._tab is None:
            import torch
            from vearch_amd import ktest as kt
            self._tab = kt.pq_lut_l2(
                torch.from_numpy(self.queries).cuda(),
                torch.from_numpy(self.codebooks).cuda(), M, 256).cpu().numpy()
        return self._tab

    def expect(self, k2, bitmap, probes=None, dis0=None):
        probes = self.probes if probes is None else probes
        dis0 = self.dis0 if dis0 is None else dis0
        tab = self.table()
        rows = []
        for qi in range(probes.shape[0]):
            dist, ids = [np.empty(0, np.float32)], [np.empty(0, np.uint32)]
            for p, ln in enumerate(probes[qi]):
                li, lc, ls = self.lists[ln]
                start = (np.float32(dis0[qi, p]) + ls).astype(np.float32)
                keep = (li >> 31) == 0
                if bitmap:
                    keep &= ~self.deleted[li & 0x7FFFFFFF]
                dist.append(kr.adc_chain(start, tab[qi], lc)[keep])
                ids.append(li[keep])
            rows.append(kr.topk_keys(np.concatenate(dist),
                                     np.concatenate(ids), k2, False))
        return np.stack(rows)

    def run(self, S, k2, bitmap=False, count=False, rerank=None, probes=None,
            dis0=None, queries=None, qmap=None, kill_flag=None):
        from vearch_amd import ktest as kt
        return kt.ivfpq_scan_prune(
            self.lists, self.probes if probes is None else probes,
            self.dis0 if dis0 is None else dis0,
            self.queries if queries is None else queries, self.centroids,
            self.codebooks, S, k2,
            bitmap=kr.bitmap_words(self.deleted) if bitmap else None,
            qmap=qmap, kill_flag=kill_flag, count=count, rerank=rerank)


def _sizes(rng, lo_big=400):
    sizes = rng.integers(1, 701, size=NLIST)
    sizes[rng.choice(NLIST, 6, replace=False)] = 0
    big = np.flatnonzero(sizes >= lo_big)
    return sizes, big


_CACHE = {}


def clustered():
    """lists far apart (centroid distance^2 ~ 85, radius ~ 0.3); each query
    sits next to a list of >= 400 entries."""
    if "cl" not in _CACHE:
        rng = np.random.default_rng(11)
        sizes, big = _sizes(rng)
        cent = rng.random((NLIST, D)) * 4.0
        dead = [int(np.flatnonzero(sizes > 0)[0])]  # one all-deleted list
        tgt = rng.choice(np.setdiff1d(big, dead), NQ)
        q = cent[tgt] + rng.standard_normal((NQ, D)) * 0.05
        _CACHE["cl"] = Model(cent, sizes, q, 12, dead_lists=dead)
    return _CACHE["cl"]


def iid():
    """centroids closer to each other than the residual radius: no bound
    is ever positive"""
    if "iid" not in _CACHE:
        rng = np.random.default_rng(21)
        sizes, _ = _sizes(rng)
        cent = rng.standard_normal((NLIST, D)) * 0.02
        q = rng.standard_normal((NQ, D)) * 0.02
        _CACHE["iid"] = Model(cent, sizes, q, 22)
    return _CACHE["iid"]


def small_lists():
    """clustered, but four lists together hold fewer than 200 entries"""
    if "small" not in _CACHE:
        rng = np.random.default_rng(31)
        sizes = rng.integers(0, 45, size=NLIST)
        cent = rng.random((NLIST, D)) * 4.0
        q = cent[rng.integers(0, NLIST, NQ)] + \
            rng.standard_normal((NQ, D)) * 0.05
        _CACHE["small"] = Model(cent, sizes, q, 32)
    return _CACHE["small"]


def _off(m, *a, **kw):
    with _env(GAMMA_SCAN_PRUNE=0):
        return m.run(*a, **kw)[0]


@pytest.mark.parametrize("bs", [256, 512])
@pytest.mark.parametrize("head", [1, 2, 4])
@pytest.mark.parametrize("k2", [10, 200])
def test_clustered_lists_are_skipped_and_keys_stay(bs, head, k2):
    m = clustered()
    with _env(GAMMA_SCAN_BS=bs, GAMMA_SCAN_PRUNE_HEAD=head,
              GAMMA_SCAN_PRUNE=1):
        for bitmap in (False, True):
            exp = m.expect(k2, bitmap)
            keys, st = m.run(1, k2, bitmap=bitmap, count=True)
            assert np.array_equal(keys[:, 0], exp)
            assert np.array_equal(m.run(1, k2, bitmap=bitmap)[0], keys)
            assert np.array_equal(_off(m, 1, k2, bitmap=bitmap), keys)
            if not bitmap:
                # every query's own list holds >= 400 entries: with the
                # threshold set, the far lists behind the head must go
                assert (st[:, 0] > 0).all(), st[:, 0]
                assert (st[:, 1] <= st[:, 2]).all()
                assert st[:, 1].sum() > st[:, 2].sum() // 2
        k3, st3 = m.run(3, k2, count=True)
        assert np.array_equal(_off(m, 3, k2), k3)
        assert np.array_equal(m.run(3, k2)[0], k3)


@pytest.mark.parametrize("bs", [256, 512])
@pytest.mark.parametrize("head", [1, 2, 4])
@pytest.mark.parametrize("k2", [10, 200])
def test_fused_rerank_outputs_stay(bs, head, k2):
    m = clustered()
    k = min(k2, 7)
    with _env(GAMMA_SCAN_BS=bs, GAMMA_SCAN_PRUNE_HEAD=head,
              GAMMA_SCAN_PRUNE=1):
        for bitmap in (False, True):
            (od, oi), _ = m.run(1, k2, bitmap=bitmap, rerank=(m.base, 12, k))
            with _env(GAMMA_SCAN_PRUNE=0):
                (od0, oi0), _ = m.run(1, k2, bitmap=bitmap,
                                      rerank=(m.base, 12, k))
            assert np.array_equal(oi, oi0) and np.array_equal(od, od0)
            assert (oi[:, 0] >= 0).all()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("k2", [10, 200])
def test_shuffled_qmap_keeps_rows_norms_and_counters(S, k2):
    """Workgroup b serves query qmap[b]: keys land in the ORIGINAL row, and
    the query norm of the slack and the counters are taken by that row too
    (the queries' norms differ by more than 1 across the batch)."""
    m = clustered()
    qn = np.linalg.norm(m.queries, axis=1)
    assert qn.max() - qn.min() > 1.0
    qmap = np.random.default_rng(41).permutation(NQ).astype(np.int32)
    keys, st = m.run(S, k2, count=True, qmap=qmap)
    plain, st_plain = m.run(S, k2, count=True)
    assert np.array_equal(keys, plain)
    assert np.array_equal(st, st_plain)
    assert (st[:, 0] > 0).all()
    assert np.array_equal(_off(m, S, k2, qmap=qmap), keys)
    assert np.array_equal(m.run(S, k2, qmap=qmap)[0], keys)
    if S == 1:
        assert np.array_equal(keys[:, 0], m.expect(k2, False))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("head", [1, 2])
def test_kill_flag(S, head):
    """A flag raised before the launch ends every workgroup in its
    (shortened) head chunk: the launch returns, with what
    GAMMA_SCAN_PRUNE=0 writes. A flag that stays down changes nothing."""
    m = clustered()
    with _env(GAMMA_SCAN_PRUNE_HEAD=head, GAMMA_SCAN_PRUNE=1):
        for k2 in (10, 200):
            up, st = m.run(S, k2, count=True, kill_flag=1)
            assert np.array_equal(_off(m, S, k2, kill_flag=1), up)
            assert np.array_equal(m.run(S, k2, kill_flag=1)[0], up)
            assert st[:, 0].sum() == 0  # nothing behind the head was reached
            down = m.run(S, k2, kill_flag=0)[0]
            assert np.array_equal(down, m.run(S, k2)[0])
            assert np.array_equal(_off(m, S, k2, kill_flag=0), down)
    (od, oi), _ = m.run(1, 200, rerank=(m.base, 12, 7), kill_flag=1)
    with _env(GAMMA_SCAN_PRUNE=0):
        (od0, oi0), _ = m.run(1, 200, rerank=(m.base, 12, 7), kill_flag=1)
    assert np.array_equal(oi, oi0) and np.array_equal(od, od0)


@pytest.mark.parametrize("head", [1, 2, 4])
def test_iid_data_skips_nothing(head):
    m = iid()
    with _env(GAMMA_SCAN_PRUNE_HEAD=head, GAMMA_SCAN_PRUNE=1):
        for k2 in (10, 200):
            keys, st = m.run(1, k2, count=True)
            assert np.array_equal(keys[:, 0], m.expect(k2, False))
            assert np.array_equal(_off(m, 1, k2), keys)
            assert st[:, 0].sum() == 0 and st[:, 1].sum() == 0
            assert st[:, 2].sum() > 0


@pytest.mark.parametrize("head", [1, 2, 4])
def test_short_head_leaves_the_threshold_empty(head):
    m = small_lists()
    with _env(GAMMA_SCAN_PRUNE_HEAD=head, GAMMA_SCAN_PRUNE=1):
        keys, st = m.run(1, 200, count=True)
        assert np.array_equal(keys[:, 0], m.expect(200, False))
        assert np.array_equal(_off(m, 1, 200), keys)
        assert st[:, 0].sum() == 0
        k3, _ = m.run(3, 200, count=True)
        assert np.array_equal(_off(m, 3, 200), k3)


@pytest.mark.parametrize("head", [1, 2, 4])
def test_heavy_filter_loosens_the_threshold(head):
    """the bitmap removes 90 % of the ids: the head's k2-th live distance
    is looser than the unfiltered one, or absent"""
    m = clustered()
    with _env(GAMMA_SCAN_PRUNE_HEAD=head, GAMMA_SCAN_PRUNE=1):
        for k2 in (10, 200):
            keys, st = m.run(1, k2, bitmap=True, count=True)
            _, st_all = m.run(1, k2, bitmap=False, count=True)
            assert np.array_equal(keys[:, 0], m.expect(k2, True))
            assert np.array_equal(_off(m, 1, k2, bitmap=True), keys)
            assert (st[:, 1] <= st_all[:, 1]).all()


def _eps():
    terms = (M + 1) + (DSUB + 1) + (M + DSUB) + 2 * (D + 2) + (M + DSUB + 2)
    return 8.0 * terms * 2.0 ** -24


FACTORS = [-1.5, -0.9, 0.0, 0.5, 0.9, 1.1, 1.5, 4.0]


@pytest.mark.parametrize("seed", range(6))
def test_bound_at_the_threshold(seed):
    """Query j probes two near lists and one far list whose bound sits at
    the head's k2-th distance + f * slack, f = FACTORS[j]. Below 0.9 slack
    the list must be walked, above 1.1 it must be skipped, and the keys
    are the reference's either way."""
    from vearch_amd import ktest as kt
    rng = np.random.default_rng(100 + seed)
    k2, nf = 10, len(FACTORS)
    q = rng.random(D) * 2.0
    near = q[None] + rng.standard_normal((2, D)) * 0.05
    sizes = [300, 50] + [100] * nf
    # first pass with the far lists anywhere: codes do not depend on the
    # centroids, so the radii and the head's k2-th distance are final
    far0 = q[None] + 10.0
    m0 = Model(np.vstack([near, np.repeat(far0, nf, 0)]), sizes,
               np.repeat(q[None], nf, 0), 200 + seed)
    cwn = (m0.codebooks.astype(np.float32) ** 2).sum(axis=2)
    rmax = kt.pq_list_rmax(None, cwn, M, 256, len(sizes),
                           buckets=[c for _, c, _ in m0.lists])
    head = m0.expect(k2, False, probes=m0.probes[:1, :2],
                     dis0=m0.dis0[:1, :2])
    kth = kr.key_decode(head[0, k2 - 1:k2], False)[0][0].astype(np.float64)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    cent = [near[0], near[1]]
    for j, f in enumerate(FACTORS):
        rm = float(rmax[2 + j])
        t = rm + np.sqrt(kth)
        for _ in range(3):  # the slack depends on ||c||: fixed point
            c = q + t * u
            nrm = (np.linalg.norm(q.astype(np.float32)) +
                   np.linalg.norm(c.astype(np.float32)) + rm)
            t = rm + np.sqrt(max(kth + f * _eps() * nrm * nrm, 0.0))
        cent.append(q + t * u)
    m = Model(np.array(cent), sizes, np.repeat(q[None], nf, 0), 200 + seed)
    probes = np.array([[0, 1, 2 + j] for j in range(nf)], dtype=np.int64)
    qd = m.queries.astype(np.float64)
    dis0 = np.array([[((qd[j] - m.centroids[ln].astype(np.float64)) ** 2)
                      .sum() for ln in probes[j]] for j in range(nf)],
                    dtype=np.float32)
    exp = m.expect(k2, False, probes=probes, dis0=dis0)
    keys, st = m.run(1, k2, count=True, probes=probes, dis0=dis0)
    assert np.array_equal(keys[:, 0], exp)
    assert np.array_equal(_off(m, 1, k2, probes=probes, dis0=dis0), keys)
    for j, f in enumerate(FACTORS):
        if f <= 0.9:
            assert st[j, 0] == 0, (f, st[j])
        if f >= 1.1:
            assert st[j, 0] == 1 and st[j, 1] == 100, (f, st[j])


def test_pq_list_rmax_against_numpy():
    from vearch_amd import ktest as kt
    rng = np.random.default_rng(5)
    for ksub in (256, 16):
        nlist = 9
        cwn = rng.random((M, ksub)).astype(np.float32)
        sizes = [0, 1, 63, 64, 65, 300, 0, 700, 257]
        codes = [rng.integers(0, ksub, size=(n, M), dtype=np.uint8)
                 for n in sizes]
        ref = np.zeros(nlist, np.float32)
        for ln, c in enumerate(codes):
            if len(c):
                s = kr.adc_chain(np.float32(0.0), cwn, c)
                ref[ln] = np.sqrt(s.max(), dtype=np.float32)
        ent = [kr.pack4(c) if ksub == 16 else c for c in codes]
        got = kt.pq_list_rmax(None, cwn, M, ksub, nlist, buckets=ent)
        up = np.nextafter(ref, np.float32(np.inf))
        assert ((got >= ref) & (got <= up)).all(), (got, ref)
        # staged form: appends only raise; unknown list numbers are skipped
        asg = np.repeat(np.arange(nlist), sizes).astype(np.int32)
        flat = np.concatenate(ent)
        asg2 = asg.copy()
        asg2[::7] = -1
        asg2[3::11] = nlist
        r0 = rng.random(nlist).astype(np.float32) * 2.0
        got2 = kt.pq_list_rmax(flat, cwn, M, ksub, nlist, asg=asg2, rmax0=r0)
        ref2 = r0.copy()
        for ln in range(nlist):
            c = codes[ln][asg2[asg == ln] == ln]
            if len(c):
                s = kr.adc_chain(np.float32(0.0), cwn, c)
                ref2[ln] = max(ref2[ln], np.sqrt(s.max(), dtype=np.float32))
        up2 = np.nextafter(ref2, np.float32(np.inf))
        assert ((got2 >= ref2) & (got2 <= up2)).all(), (got2, ref2)
        one = kt.pq_list_rmax(flat[:5], cwn, M, ksub, nlist, asg_const=4)
        assert (one[np.arange(nlist) != 4] == 0).all() and one[4] > 0
