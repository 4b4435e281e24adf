"""The filter-first plan at the sizes the engine feeds it: gk::cand_scan at
its tile edges, gk::bitmap_candidates over many blocks and past `cap`, then
Engine::search with `filter_first` over candidate counts from 0 to 3000,
batches on both tile shapes, topn 1 and 1024, l2_sqrt, an untrained table,
the life of a table, BINARYIVF and a batch split into query groups.

References: numpy (flatnonzero, fp64 distances), gk::rerank for the canonical
fmaf chain, and the oracle's canonical FLAT scan over exactly the live
matching documents; tests/filter_first_ref.py holds the inputs."""
import os
import struct

import numpy as np
import pytest

import filter_first_ref as ffr
import oracle as orc
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(kr.EMPTY)
U = ffr.U
FILL = 0xA5A5A5A5  # ktest.bitmap_candidates' fill of the id array


@pytest.fixture(scope="module")
def kt():
    from vearch_amd import ktest
    return ktest


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ================================================================ cand_scan
CS_N, CS_SHIFT = 2048, 7  # 16 segments of 128 rows


def _check_cand_scan(kt, q, base, segs, ip, cand, pad):
    """The key matrix of one launch: EMPTY from ncand to pad; bit-equal to
    gk::rerank on the same pairs; every distance within the sequential fp32
    bound 1.01 (d + 2) u sum|terms| of the fp64 value. Returns the keys."""
    nq, d = q.shape
    ncand = cand.shape[0]
    ctx = (d, nq, ip, ncand, pad)
    got = kt.keys_to_np(kt.cand_scan(dev(q), segs, CS_SHIFT, ip, cand, pad))
    assert got.shape == (nq, pad), ctx
    assert np.all(got[:, ncand:] == EMPTY), ctx
    if ncand == 0:
        return got
    kin = kr.key_encode(np.zeros((nq, ncand), np.float32),
                        np.tile(cand, (nq, 1)), ip)
    want = kt.keys_to_np(
        kt.rerank(dev(q), segs, CS_SHIFT, ip, kt.keys_to_dev(kin)))
    assert np.array_equal(got[:, :ncand], want), ctx
    dist, ids = kr.key_decode(got[:, :ncand], ip)
    assert np.array_equal(ids, np.tile(cand.astype(np.int64), (nq, 1))), ctx
    q64, b64 = q.astype(np.float64), base[cand].astype(np.float64)
    terms = (q64[:, None, :] * b64[None] if ip
             else (q64[:, None, :] - b64[None]) ** 2)
    err = np.abs(dist.astype(np.float64) - terms.sum(axis=2))
    assert (err <= 1.01 * (d + 2) * U * np.abs(terms).sum(axis=2)).all(), ctx
    return got


@pytest.mark.parametrize("ip", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("nq", [8, 9, 64, 70])
@pytest.mark.parametrize("d", [36, 64])
def test_cand_scan_tile_edges(kt, d, nq, ip):
    """nq 8: the last batch on the 8 x 256 tile; 9: the first on 64 x 64;
    70: two query tiles, the second short. ncand around one 256-wide tile,
    then several tiles of either shape with the last one partial; 0: what
    the engine launches when the filter matches nothing (ncand_pad = 10 at
    topn 10). d = 36 has a partial last slice."""
    rng = np.random.default_rng(100 * d + nq)
    base = rng.standard_normal((CS_N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    segs = kt.split_segments(base, CS_SHIFT)
    for ncand in (0, 255, 256, 257, 600, 1500):
        cand = np.sort(rng.permutation(CS_N)[:ncand]).astype(np.uint32)
        pads = [max(1, (ncand + 255) // 256 * 256)] + [10] * (ncand == 0)
        for pad in pads:
            _check_cand_scan(kt, q, base, segs, ip, cand, pad)


@pytest.mark.parametrize("ip", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("nq", [3, 9])
def test_cand_scan_id_past_the_table(kt, nq, ip):
    """The store holds 1998 rows: 15 whole segments and one of 78. Ids whose
    segment number is 16 or more, in the first, a middle and the last
    position of the list, give EMPTY columns and change no other column;
    the list also holds the first and the last row of the short segment."""
    d, n = 36, CS_N - 50
    rng = np.random.default_rng(7 + nq)
    base = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    segs = kt.split_segments(base, CS_SHIFT)
    assert len(segs) == 16 and segs[-1].shape[0] == 78
    good = np.sort(rng.permutation(n - 2)[:298]).astype(np.uint32)
    good = np.concatenate([good[good < 1920], [1920],
                           good[good > 1920], [n - 1]]).astype(np.uint32)
    ref = _check_cand_scan(kt, q, base, segs, ip, good, 512)
    mid = good.shape[0] // 2
    bad_at = [0, mid + 1, good.shape[0] + 2]
    cand = np.concatenate([[16 << CS_SHIFT], good[:mid], [5000], good[mid:],
                           [0xFFFFFFFF]]).astype(np.uint32)
    ncand = cand.shape[0]
    got = kt.keys_to_np(kt.cand_scan(dev(q), segs, CS_SHIFT, ip, cand, 512))
    keep = np.ones(ncand, bool)
    keep[bad_at] = False
    assert np.array_equal(cand[keep], good)
    assert np.all(got[:, bad_at] == EMPTY)
    assert np.array_equal(got[:, :ncand][:, keep], ref[:, :good.shape[0]])
    assert np.all(got[:, ncand:] == EMPTY)


# ======================================================= bitmap_candidates
BLK = 8192  # ids per compaction block


MANY = 1024 * BLK + 2 * BLK + 5  # 1027 blocks: the scan takes its carry


@pytest.mark.parametrize("fill", ["sparse", "four"])
def test_bitmap_candidates_many_blocks(kt, fill):
    """sparse: 0.1 % of the ids pass. four: one id passes in each of block
    0, block 1023 (its last id), block 1024 (its first id: the first count
    behind the carry) and the last block (id n - 1); the 27 bits past n in
    the last word are clear there and must not show."""
    assert kt.BITMAP_CAND_BLOCK == BLK
    n = MANY
    nbits = (n + 31) // 32 * 32
    if fill == "sparse":
        dropped = np.random.default_rng(5).random(nbits) >= 0.001
        dropped[n:] = True
    else:
        dropped = np.ones(nbits, bool)
        dropped[[5, 1023 * BLK + BLK - 1, 1024 * BLK, n - 1]] = False
        dropped[n:] = False
    want = np.flatnonzero(~dropped[:n]).astype(np.uint32)
    assert want.size == 4 or 7000 < want.size < 10000
    # kr.bitmap_words is vectorised (fast enough at 8.4 M bits) and pinned
    # by tests/test_kernel_refs.py
    ids, count = kt.bitmap_candidates(kr.bitmap_words(dropped), n)
    assert count == want.size
    assert np.array_equal(ids[:count], want)
    assert np.all(ids[count:] == FILL)


def test_bitmap_candidates_past_cap(kt):
    """The count is the full count whatever cap is; ids[:min(cap, count)]
    is the head of the list; no slot from cap on is written (cap = 0: not
    even the one slot the wrapper allocates)."""
    n = 3 * BLK - 1
    rng = np.random.default_rng(n)
    nbits = (n + 31) // 32 * 32
    dropped = rng.random(nbits) < 0.5
    want = np.flatnonzero(~dropped[:n]).astype(np.uint32)
    words = kr.bitmap_words(dropped)
    assert want.size > 1000
    for cap in (0, 1, 1000, want.size):
        ids, count = kt.bitmap_candidates(words, n, cap=cap)
        assert ids.shape[0] == n and count == want.size, cap
        assert np.array_equal(ids[:cap], want[:cap]), cap
        assert np.all(ids[cap:] == FILL), cap


# =================================================================== engine
N, NLIST, FF = ffr.N, 16, 100000
# kind -> (metric, dimension, index parameters). IVFRABITQ takes no
# dimension below 32.
KINDS = {
    "IVFPQ": ("L2", 8, '"ncentroids": 16, "nsubvector": 4, '),
    "IVFFLAT": ("InnerProduct", 8, '"ncentroids": 16, '),
    "IVFRABITQ": ("L2", 32, '"ncentroids": 16, "nb_bits": 1, '),
    "FLAT": ("L2", 8, ""),
}


def _i32(v):
    return struct.pack("<i", v)


def _create(path, kind, d, metric, extra, threshold):
    from vearch_amd import GammaEngine, fbsenc
    os.makedirs(path, exist_ok=True)
    eng = GammaEngine(path=path)
    eng.create_table(
        d, kind, '{%s"metric_type": "%s", "training_threshold": %d}'
        % (extra, metric, threshold),
        scalar_fields=[("num", fbsenc.DATA_INT)])
    return eng


def _add(eng, base, start=0):
    """documents start .. start + len(base) - 1, `_id` and num = the id"""
    from vearch_amd import fbsenc
    for i, v in enumerate(base):
        eng.add_doc(str(start + i), v,
                    fields=[("num", _i32(start + i), fbsenc.DATA_INT)])


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """kind -> (engine, base, queries, metric): one table per kind, built
    when first asked for and kept for the module"""
    root = tmp_path_factory.mktemp("filter_first_sizes")
    made = {}

    def get(kind):
        if kind not in made:
            metric, d, extra = KINDS[kind]
            base, q = ffr.data(d=d)
            eng = _create(str(root / kind), kind, d, metric, extra, N)
            made[kind] = (eng, base, q, metric)
            _add(eng, base)
            eng.build_index()
        return made[kind]
    yield get
    for eng, _, _, _ in made.values():
        eng.close()


def _search(eng, q, lo, hi, topn=10, ff=FF, l2_sqrt=False, nprobe=1):
    """[(ids, fp32 score bits)] per query of a lo <= num <= hi request;
    ff = 0: the parameter is absent"""
    ip = '{"nprobe": %d%s}' % (nprobe,
                               ', "filter_first": %d' % ff if ff else "")
    res = eng.search_pb(q, topn=topn, index_params=ip, l2_sqrt=l2_sqrt,
                        range_filters=[("num", _i32(lo), _i32(hi), True,
                                        True)])
    assert len(res) == len(q)
    return [([int(it["fields"]["_id"]) for it in r["items"]],
             [int(np.float32(it["score"]).view(np.uint32))
              for it in r["items"]])
            for r in res]


def _truth(base, q, docs, metric, topn, sqrt=False):
    """what _search must return: the oracle's canonical-chain FLAT scan over
    the documents `docs` alone, as many results as there are documents"""
    if len(docs) == 0:
        return [([], [])] * len(q)
    od, oi = orc.flat_search(base[docs], q, topn, metric)
    if sqrt:
        od = np.sqrt(np.maximum(od, 0))  # fp32, correctly rounded
    m = min(topn, len(docs))
    assert (oi[:, :m] >= 0).all() and (oi[:, m:] == -1).all()
    return [(docs[oi[t, :m]].tolist(), od[t, :m].view(np.uint32).tolist())
            for t in range(len(q))]


def _equals_truth(got, base, q, docs, metric, topn):
    """ids and score bits equal the truth; where the fp64 reference alone
    shows clear gaps, its ids too"""
    docs = np.asarray(docs, dtype=np.int64)
    assert got == _truth(base, q, docs, metric, topn)
    ids64, clear = ffr.topk_f64(base[docs], q, topn, metric)
    for t in np.flatnonzero(clear):
        assert got[t][0] == docs[ids64[t]].tolist()
    return clear


ALL = np.arange(N)


@pytest.mark.parametrize("nq", [5, 9])
@pytest.mark.parametrize("count", ffr.COUNTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_engine_candidate_counts(tables, kind, count, nq):
    """0: empty results, no error; 1: one document (fewer than topn: all of
    them, in order, nothing else); 255 .. 257: around one candidate tile;
    1025 and 3000: ncand_pad beyond the deep select's own range. 5 queries
    run the narrow tile, 9 the wide one."""
    eng, base, q, metric = tables(kind)
    lo, hi = ffr.span(count)
    docs = ffr.docs_in(lo, hi, ALL)
    assert docs.size == count
    got = _search(eng, q[:nq], lo, hi)
    clear = _equals_truth(got, base, q[:nq], docs, metric, 10)
    assert all(len(g[0]) == min(10, count) for g in got)
    assert count == 0 or clear.any()


@pytest.mark.parametrize("count", [257, 3000])
@pytest.mark.parametrize("topn", [1, 1024])
@pytest.mark.parametrize("kind", list(KINDS))
def test_engine_topn_extremes(tables, kind, topn, count):
    eng, base, q, metric = tables(kind)
    lo, hi = ffr.span(count)
    got = _search(eng, q, lo, hi, topn=topn)
    _equals_truth(got, base, q, ffr.docs_in(lo, hi, ALL), metric, topn)
    assert all(len(g[0]) == min(topn, count) for g in got)


@pytest.mark.parametrize("kind", list(KINDS))
def test_engine_threshold_edge(tables, kind):
    """filter_first equal to the candidate count takes the plan; one below
    it leaves the request on the path it takes with the parameter absent."""
    eng, base, q, metric = tables(kind)
    lo, hi = ffr.span(257)
    docs = ffr.docs_in(lo, hi, ALL)
    plain = _search(eng, q, lo, hi, ff=0)
    if kind != "FLAT":  # one probed list holds few of the 257
        assert plain != _truth(base, q, docs, metric, 10)
    _equals_truth(_search(eng, q, lo, hi, ff=257), base, q, docs, metric, 10)
    assert _search(eng, q, lo, hi, ff=256) == plain


@pytest.mark.parametrize("count", [257, 1025])
def test_engine_l2_sqrt(tables, count):
    """scores are the fp32 square roots of the canonical distances, on the
    IVFPQ table bit for bit what the FLAT table returns"""
    eng, base, q, metric = tables("IVFPQ")
    flat = tables("FLAT")[0]
    lo, hi = ffr.span(count)
    want = _truth(base, q, ffr.docs_in(lo, hi, ALL), metric, 10, sqrt=True)
    got = _search(eng, q, lo, hi, l2_sqrt=True)
    assert got == want
    assert got == _search(flat, q, lo, hi, l2_sqrt=True)
    assert got == _search(flat, q, lo, hi, l2_sqrt=True, ff=0)


def test_engine_untrained_ivfpq(tmp_path):
    """documents added, build_index never called: the plan reads the raw
    store alone"""
    metric, d, extra = KINDS["IVFPQ"]
    base, q = ffr.data(d=d)
    eng = _create(str(tmp_path / "t"), "IVFPQ", d, metric, extra, 10 * N)
    try:
        _add(eng, base)
        lo, hi = 1000, 1299
        _equals_truth(_search(eng, q, lo, hi), base, q,
                      ffr.docs_in(lo, hi, ALL), metric, 10)
    finally:
        eng.close()


def test_engine_life_of_a_table(tmp_path):
    """After every step a 257-candidate, a 1025-candidate and a wider range
    (by their count before the delete; the wider one keeps more than 1024
    live documents after it) equal the truth over the documents then
    live."""
    metric, d, extra = KINDS["IVFPQ"]
    path = str(tmp_path / "t")
    base = ffr.gaussian(N + 500, d, 21)
    q = ffr.gaussian(ffr.NQ, d, 22)
    spans = [(5900, 6156), (5400, 6424), (4000, 6499)]
    live = np.arange(N + 500)

    def check(eng):
        for lo, hi in spans:
            docs = ffr.docs_in(lo, hi, live)
            _equals_truth(_search(eng, q, lo, hi), base, q, docs, metric, 10)

    eng = _create(path, "IVFPQ", d, metric, extra, N)
    try:
        _add(eng, base[:N])
        eng.build_index()
        _add(eng, base[N:], start=N)
        check(eng)
        gone = np.arange(5400, 6425, 3)
        for v in gone.tolist():
            assert eng.delete_doc(str(v)) == 0
        live = np.setdiff1d(live, gone)
        assert ffr.docs_in(*spans[2], live).size > 1024
        check(eng)
        eng.compact(0.0)
        check(eng)
        eng.dump()
    finally:
        eng.close()
    eng = _create(path, "IVFPQ", d, metric, extra, N)
    try:
        eng.load()
        check(eng)
    finally:
        eng.close()


def test_engine_binaryivf_ignores_the_parameter(tmp_path):
    from vearch_amd import GammaEngine, fbsenc
    n, d = 2000, 64
    rng = np.random.default_rng(31)
    base = rng.integers(0, 256, size=(n, d // 8), dtype=np.uint8)
    q = base[:5] ^ np.uint8(1)
    os.makedirs(str(tmp_path / "t"))
    eng = GammaEngine(path=str(tmp_path / "t"))
    try:
        eng.create_table(d, "BINARYIVF", '{"ncentroids": 16}',
                         scalar_fields=[("num", fbsenc.DATA_INT)])
        _add(eng, base)
        eng.build_index()
        plain = _search(eng, q, 100, 399, ff=0, nprobe=16)
        assert all(len(p[0]) == 10 for p in plain)
        assert all(100 <= i <= 399 for p in plain for i in p[0])
        assert _search(eng, q, 100, 399, nprobe=16) == plain
    finally:
        eng.close()


def test_engine_query_groups(tmp_path):
    """A group holds 256 MiB / (ncand_pad * 8) queries: with all 8192
    documents passing, 4096. 4097 queries split into a group of 4096 and a
    group of one."""
    n, d, nq = 8192, 4, 4097
    base, q = ffr.data(n, d, nq, seed=41)
    eng = _create(str(tmp_path / "t"), "FLAT", d, "L2", "", n)
    try:
        _add(eng, base)
        eng.build_index()
        got = _search(eng, q, 0, n - 1, topn=2)
        assert all(len(g[0]) == 2 and g[0][0] != g[0][1] for g in got)
        rows = sorted({0, 4095, 4096} | set(range(0, nq, 97)))
        want = _truth(base, q[rows], np.arange(n), "L2", 2)
        assert [got[r] for r in rows] == want
    finally:
        eng.close()
