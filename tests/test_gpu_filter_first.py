"""Filter-first plan: gk::bitmap_candidates and gk::cand_scan through their
kernel test hooks, then Engine::search with the `filter_first` parameter.
References are numpy (flatnonzero, fp64 distances), gk::rerank for the
canonical fmaf chain, and the oracle's canonical FLAT scan."""
import struct

import numpy as np
import pytest

import oracle as orc
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(kr.EMPTY)
U = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def kt():
    from vearch_amd import ktest
    return ktest


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ======================================================= bitmap_candidates
BLK = 8192  # ids per compaction block


@pytest.mark.parametrize("fill", ["clear", "set", 0.5, 0.001])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, BLK + 5, 3 * BLK - 1])
def test_bitmap_candidates(kt, n, fill):
    """Ids and count equal np.flatnonzero of the clear bits below n. The
    bits past n in the last word are set (random at 50 %) and must not
    show; slots past the count keep the wrapper's fill."""
    assert kt.BITMAP_CAND_BLOCK == BLK
    rng = np.random.default_rng(n + 1)
    nbits = (n + 31) // 32 * 32
    dropped = {"clear": np.zeros(nbits, bool),
               "set": np.ones(nbits, bool)}.get(fill)
    if dropped is None:
        dropped = rng.random(nbits) >= fill  # `fill` = share that passes
    dropped[n:] = rng.random(nbits - n) < 0.5 if fill == 0.5 else True
    want = np.flatnonzero(~dropped[:n]).astype(np.uint32)
    ids, count = kt.bitmap_candidates(kr.bitmap_words(dropped), n)
    assert count == want.size
    assert np.array_equal(ids[:count], want)
    assert np.all(ids[count:] == 0xA5A5A5A5)


# ================================================================ cand_scan
CS_N = 300  # raw-store rows, in segments of 32 (10, the last one short)


@pytest.mark.parametrize("ip", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("nq", [1, 3, 65])
@pytest.mark.parametrize("d", [4, 36, 128, 260])
def test_cand_scan(kt, d, nq, ip):
    """nq 1 and 3: the 8 x 256 tile; 65: the 64 x 64 tile, two query tiles.
    Every column of the key matrix: (a) fp64 distance within the fp32
    sequential-sum bound (d + 2) u sum|terms|; (b) bit-equal to gk::rerank
    on the same pairs; EMPTY from ncand to ncand_pad (69 columns: past the
    tile edge). Two candidates are the same vector: equal distance bits.
    d = 36 runs on 75 segments of 4 rows, past the LDS segment cache."""
    CS_SHIFT = 2 if d == 36 else 5
    rng = np.random.default_rng(1000 * d + nq)
    base = rng.standard_normal((CS_N, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    qd, q64 = dev(q), q.astype(np.float64)
    for ncand in (1, 63, 64, 65, 200):
        cand = np.sort(rng.permutation(CS_N)[:ncand]).astype(np.uint32)
        if ncand > 1:
            base[cand[-1]] = base[cand[0]]
        segs = kt.split_segments(base, CS_SHIFT)
        pad = ncand + 69
        got = kt.keys_to_np(kt.cand_scan(qd, segs, CS_SHIFT, ip, cand, pad))
        ctx = (d, nq, ip, ncand)
        assert got.shape == (nq, pad) and np.all(got[:, ncand:] == EMPTY), ctx
        kin = kr.key_encode(np.zeros((nq, ncand), np.float32),
                            np.tile(cand, (nq, 1)), ip)
        want = kt.keys_to_np(
            kt.rerank(qd, segs, CS_SHIFT, ip, kt.keys_to_dev(kin)))
        assert np.array_equal(got[:, :ncand], want), ctx
        dist, ids = kr.key_decode(got[:, :ncand], ip)
        assert np.array_equal(ids, np.tile(cand.astype(np.int64), (nq, 1)))
        b64 = base[cand].astype(np.float64)
        terms = (q64[:, None, :] * b64[None] if ip
                 else (q64[:, None, :] - b64[None]) ** 2)
        err = np.abs(dist.astype(np.float64) - terms.sum(axis=2))
        assert (err <= 1.01 * (d + 2) * U * np.abs(terms).sum(axis=2)).all()
        if ncand > 1:
            assert np.array_equal(dist[:, 0], dist[:, -1]), ctx


def test_cand_scan_refuses_d_not_multiple_of_4(kt):
    base = np.zeros((8, 6), np.float32)
    with pytest.raises(kt.KTestError) as e:
        kt.cand_scan(dev(base[:1]), kt.split_segments(base, 3), 3, 0,
                     np.arange(4, dtype=np.uint32))
    assert e.value.code == 1  # hipErrorInvalidValue


# =================================================================== engine
D, N, NLIST, K, NQ = 32, 4000, 16, 10, 5
MATCH = np.arange(7, N, 100)        # num == 7: 40 docs in all lists
GONE = 1207                         # one of them, deleted
FEW = np.array([50, 1550, 3050])    # num == 500
KINDS = {
    "IVFPQ": ("L2", '"ncentroids": 16, "nsubvector": 8, '),
    "IVFFLAT": ("InnerProduct", '"ncentroids": 16, '),
    "IVFRABITQ": ("L2", '"ncentroids": 16, "nb_bits": 1, '),
    "FLAT": ("L2", ""),
}


@pytest.fixture(scope="module")
def data():
    """Gaussian base and queries (seed 11), checked here on the fp64
    reference alone: no two of a query's best 11 live matching docs are
    closer than twice the fp32 bound of cand_scan's test, either metric."""
    rng = np.random.default_rng(11)
    base = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((NQ, D)).astype(np.float32)
    live = MATCH[MATCH != GONE]
    b64, q64 = base[live].astype(np.float64), q.astype(np.float64)
    for best, terms in ((-1, q64[:, None, :] * b64[None]),
                        (1, (q64[:, None, :] - b64[None]) ** 2)):
        gap = np.diff(np.sort(best * terms.sum(axis=2), axis=1), axis=1)
        assert gap[:, :10].min() > \
            2 * (D + 2) * U * np.abs(terms).sum(axis=2).max()
    return base, q


@pytest.fixture(scope="module", params=list(KINDS))
def table(request, data):
    from vearch_amd import GammaEngine, fbsenc
    kind = request.param
    metric, extra = KINDS[kind]
    eng = GammaEngine(path="/tmp/gamma_filter_first_" + kind)
    eng.create_table(
        D, kind, '{%s"metric_type": "%s", "training_threshold": %d}'
        % (extra, metric, N), scalar_fields=[("num", fbsenc.DATA_INT)])
    for vid in range(N):
        num = 500 if vid in FEW else vid % 100
        eng.add_doc(str(vid), data[0][vid], fields=[
            ("num", struct.pack("<i", num), fbsenc.DATA_INT)])
    eng.build_index()
    assert eng.delete_doc(str(GONE)) == 0
    yield eng, kind, metric
    eng.close()


def _search(eng, q, num, ff=0):
    """[(ids, fp32 score bits)] per query of a num == `num` request"""
    ip = '{"nprobe": 1%s}' % (', "filter_first": %d' % ff if ff else "")
    v = struct.pack("<i", num)
    res = eng.search_pb(q, topn=K, index_params=ip,
                        range_filters=[("num", v, v, True, True)])
    return [([int(it["fields"]["_id"]) for it in r["items"]],
             [np.float32(it["score"]).view(np.uint32) for it in r["items"]])
            for r in res]


def _truth(base, q, docs, metric):
    """(fp64 brute-force ids, the oracle's canonical-chain ids and dists)
    over `docs` alone"""
    _, gi = orc.flat_topk_f64(base[docs], q, min(K, len(docs)), metric)
    od, oi = orc.flat_search(base[docs], q, K, metric)
    return docs[gi], np.where(oi >= 0, docs[np.maximum(oi, 0)], -1), od


def test_engine_filter_first(table, data):
    eng, kind, metric = table
    base, q = data
    live = MATCH[MATCH != GONE]
    gi, oi, od = _truth(base, q, live, metric)
    plain = _search(eng, q, 7)
    got = _search(eng, q, 7, ff=100)
    for t in range(NQ):
        assert got[t][0] == gi[t].tolist() == oi[t].tolist()
        assert got[t][1] == od[t].view(np.uint32).tolist()
    if kind == "FLAT":
        assert got == plain  # the same exact result, bit for bit
    else:
        assert got != plain  # one probed list holds few of the 39
    # a threshold below the candidate count keeps the parent's path
    assert _search(eng, q, 7, ff=10) == plain
    # fewer matching docs than topn: all of them, nothing else
    gi3, _, od3 = _truth(base, q, FEW, metric)
    few = _search(eng, q, 500, ff=100)
    for t in range(NQ):
        assert few[t][0] == gi3[t].tolist()
        assert few[t][1] == od3[t, :3].view(np.uint32).tolist()
