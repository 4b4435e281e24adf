"""GPU tests of the IVFRABITQ index: the encode and scan kernels through
their test hooks, then the engine through GammaEngine and the C ABI.

The reference is tests/rabitq_ref.py (fp64 numpy, pinned by
tests/test_rabitq_ref.py). Sign bits are compared bit for bit; scores and
factors within tolerances derived from the fp32 format (rabitq_ref.tol and
the docstrings below), never from what the kernels return.
"""
import ctypes
import os

import numpy as np
import pytest

import rabitq_ref as rr
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

MARK = np.int64(-2 ** 63)            # host-side bit-63 delete mark
MARK32 = np.uint32(0x80000000)       # device-side bit-31 delete mark
U = 2.0 ** -23


def _sum_tol(D):
    """relative bound of a fixed-order fp32 sum of D terms (D 2^-24 of its
    absolute mass) with room for the handful of scalar operations behind it"""
    return (D + 16) * U


# ------------------------------------------------------------ encode kernel
@pytest.mark.parametrize("D", [32, 96, 128, 1024])
def test_kernel_encode(D):
    from vearch_amd import ktest
    rng = np.random.default_rng(D)
    n, nlist = 300, 5
    cent = rng.standard_normal((nlist, D)).astype(np.float32)
    asg = rng.integers(0, nlist, size=n).astype(np.int32)
    x = (cent[asg] + 0.4 * rng.standard_normal((n, D))).astype(np.float32)
    x[0] = cent[asg[0]]              # n2 = 0
    x[1, 3] = cent[asg[1], 3]        # r_3 = 0: the bit must be 0
    x[2, D - 1] = cent[asg[2], D - 1]
    c = cent[asg]
    r32, bits = rr.residual_bits(x, c)
    r = r32.astype(np.float64)
    for ip in (False, True):
        ent, sv = ktest.rabitq_encode(x, asg, cent, ip)
        ent2, sv2 = ktest.rabitq_encode(x, asg, cent, ip)
        assert np.array_equal(ent, ent2) and np.array_equal(sv, sv2)
        gb, gA, gM = rr.unpack(ent, D)
        assert np.array_equal(gb, bits)
        assert not gb[1, 3] and not gb[2, D - 1] and not gb[0].any()
        A, Mul, sval = rr.factors(x, c, ip)
        n2 = (r * r).sum(axis=1)
        xx = (x.astype(np.float64) ** 2).sum(axis=1)
        t = _sum_tol(D)
        assert np.all(np.abs(gA - A) <= t * (n2 + (xx if ip else 0.0)))
        # Mul = n2 sqrt(D) / l1: two such sums and a few rounded operations
        assert np.all(np.abs(gM - Mul) <= t * np.abs(Mul))
        assert np.all(np.abs(sv - sval)
                      <= t * (bits * np.abs(c.astype(np.float64))).sum(axis=1))
        assert gM[0] == 0.0 and sv[0] == 0.0
        assert np.isfinite(gA).all() and np.isfinite(gM).all()


# -------------------------------------------------------------- scan kernel
BS_SIZES = [0, 1, 255, 256, 257, 3 * 256 + 7, 511, 512, 513, 3 * 512 + 7]
NQ_SCAN = 3


def _scan_case(D, seed, dyadic, sizes, id_space):
    """lists with the given sizes, their centroids, queries and one probe
    row per query that names every list once, plus one -1 and one
    >= nlist. dyadic: every coordinate is a multiple of 1/16 in [-4, 4]."""
    rng = np.random.default_rng(seed)
    nlist = len(sizes)

    def draw(shape, spread=1.0):
        if dyadic:
            return (rng.integers(-64, 65, size=shape) / 16.0).astype(
                np.float32)
        return (spread * rng.standard_normal(shape)).astype(np.float32)

    cent = draw((nlist, D))
    perm = rng.permutation(id_space)
    ids, vecs, pos = [], [], 0
    for ln, n in enumerate(sizes):
        ids.append(perm[pos:pos + n].astype(np.uint32))
        v = draw((n, D)) if dyadic else \
            (cent[ln] + draw((n, D), 0.5)).astype(np.float32)
        vecs.append(v)
        pos += n
    queries = draw((NQ_SCAN, D))
    probes = np.stack([np.append(rng.permutation(nlist), [0, 0])
                       for _ in range(NQ_SCAN)]).astype(np.int64)
    for r in range(NQ_SCAN):
        probes[r, -2:] = (-1, nlist + r)
        probes[r] = probes[r][rng.permutation(nlist + 2)]
    return cent, ids, vecs, queries, probes


def _encode_lists(cent, vecs, ip):
    out = []
    for ln, v in enumerate(vecs):
        codes, sval = rr.encode(v, cent[ln], ip) if len(v) else (
            np.empty((0, rr.code_size(cent.shape[1])), np.uint8),
            np.empty(0))
        out.append((codes, sval.astype(np.float32)))
    return out


def _ref_table(cent, enc, queries, ip, eps):
    """per list: reference scores and tolerances, (nq, n) each"""
    D = cent.shape[1]
    tab = []
    for ln, (codes, _) in enumerate(enc):
        bits, A, Mul = rr.unpack(codes, D)
        sc = np.stack([rr.estimate(q, cent[ln], bits, A, Mul, ip)
                       for q in queries]) if len(codes) else \
            np.empty((len(queries), 0))
        tl = np.stack([eps * rr.scale(q, cent[ln], A, Mul, ip)
                       for q in queries]) if len(codes) else \
            np.empty((len(queries), 0))
        tab.append((sc, tl))
    return tab


def _cands(tab, ids, marks, deleted, probe_list, r):
    ci, cs, ct = [np.empty(0, np.int64)], [np.empty(0)], [np.empty(0)]
    for ln in probe_list:
        if ln < 0 or ln >= len(ids) or len(ids[ln]) == 0:
            continue
        live = ~marks[ln]
        if deleted is not None:
            live &= ~deleted[ids[ln]]
        ci.append(ids[ln][live].astype(np.int64))
        cs.append(tab[ln][0][r][live])
        ct.append(tab[ln][1][r][live])
    return np.concatenate(ci), np.concatenate(cs), np.concatenate(ct)


def _run_scan(D, dyadic, sizes, eps, combos, seed):
    """combos: (S, k2, kill, mode) tuples; mode 'none' or 'both' (delete
    marks and a bitmap, ~30 % each). Checks the raw partial rows (only live
    candidates of the sub-block's own probes, sorted, complete) and the
    merged rows, for both metrics."""
    from vearch_amd import ktest
    id_space = int(sum(sizes)) + 64
    cent, ids, vecs, queries, probes = _scan_case(D, seed, dyadic, sizes,
                                                  id_space)
    rng = np.random.default_rng(seed + 1)
    marks_both = [rng.random(len(i)) < 0.3 for i in ids]
    marks_none = [np.zeros(len(i), dtype=bool) for i in ids]
    bm = rng.random(id_space) < 0.3
    for ip in (False, True):
        enc = _encode_lists(cent, vecs, ip)
        tab = _ref_table(cent, enc, queries, ip, eps)
        for S, k2, kill, mode in combos:
            marks = marks_both if mode == "both" else marks_none
            deleted = bm if mode == "both" else None
            dev = [(np.where(m, i | MARK32, i).astype(np.uint32), c, s)
                   for i, m, (c, s) in zip(ids, marks, enc)]
            keys, od, oi = ktest.rabitq_scan(
                dev, probes, queries, cent, S, k2, ip,
                bitmap=None if deleted is None else kr.bitmap_words(deleted),
                kill_flag=kill)
            assert keys.shape == (NQ_SCAN, S, k2)
            for r in range(NQ_SCAN):
                for s in range(S):
                    pd, pi = kr.key_decode(keys[r, s], ip)
                    rr.check_row(pd, pi, *_cands(tab, ids, marks, deleted,
                                                 probes[r, s::S].tolist(),
                                                 r), ip)
                rr.check_row(od[r], oi[r],
                             *_cands(tab, ids, marks, deleted,
                                     probes[r].tolist(), r), ip)


DYADIC_COMBOS = [(S, k2, kill, "both")
                 for S in (1, 3) for k2 in (1, 10, 200)
                 for kill in (False, True)] + [(1, 10, False, "none"),
                                               (3, 200, True, "none")]


@pytest.mark.parametrize("D", [32, 64, 96, 256, 1024])
def test_kernel_scan_dyadic(D):
    """Every coordinate is a multiple of 1/16 in [-4, 4], so every sum the
    kernel forms is exact in fp32 in any order. About ten rounded scalar
    operations remain, each at most 2^-24 of the running magnitude; the
    bound 2^-20 scale allows more than that. 34 further small lists bring
    the probe row to 46 entries: two chunks of GAMMA_SCAN_PCH = 32 at
    S = 1."""
    sizes = BS_SIZES + [3 + (i % 5) for i in range(34)]
    _run_scan(D, True, sizes, 2.0 ** -20, DYADIC_COMBOS, 500 + D)


@pytest.mark.parametrize("D", [32, 96, 256])
def test_kernel_scan_dyadic_bs256(D, monkeypatch):
    monkeypatch.setenv("GAMMA_SCAN_BS", "256")
    sizes = BS_SIZES + [3 + (i % 5) for i in range(34)]
    _run_scan(D, True, sizes, 2.0 ** -20,
              [(1, 10, False, "both"), (3, 200, True, "both"),
               (1, 1, True, "none")], 700 + D)


def test_kernel_scan_kill_flag():
    """A flag raised before the launch is read at the first chunk close:
    the launch returns and every row is EMPTY. A flag left at 0 changes
    nothing. The D = 32 dyadic case: 46 probes, two chunks at S = 1.
    k2 = 1024 is the largest the launcher takes, and k2 + 2 * 512 = 2048
    still fits the selector, so this kernel only ever checks every second
    pass; a k2 above that bound cannot be launched."""
    from vearch_amd import ktest
    sizes = BS_SIZES + [3 + (i % 5) for i in range(34)]
    combos = ((1, 10), (2, 1024))
    cent, ids, vecs, queries, probes = _scan_case(32, 532, True, sizes,
                                                  int(sum(sizes)) + 64)
    assert probes.shape[1] > 32
    for ip in (False, True):
        dev = [(i, c, s) for i, (c, s) in zip(ids, _encode_lists(cent, vecs,
                                                                 ip))]
        for S, k2 in combos:
            keys, _, oi = ktest.rabitq_scan(dev, probes, queries, cent, S, k2,
                                            ip, kill_flag=1)
            assert keys.shape == (NQ_SCAN, S, k2)
            assert np.all(keys == np.uint64(kr.EMPTY)), (ip, S, k2)
            assert np.all(oi == -1)
    _run_scan(32, True, sizes, 2.0 ** -20,
              [(S, k2, 0, "none") for S, k2 in combos], 532)


@pytest.mark.parametrize("D", [64, 128])
def test_kernel_scan_gaussian(D):
    """Gaussian inputs: sums round, so the bound is rabitq_ref.tol,
    (D + 16) 2^-23 scale."""
    sizes = [0, 130, 700, 64, 1, 257, 90, 513]
    _run_scan(D, False, sizes, _sum_tol(D),
              [(1, 10, False, "both"), (3, 10, True, "both"),
               (1, 200, False, "none")], 900 + D)


# ------------------------------------------------------------------- engine
def make_engine(path, **kw):
    from vearch_amd import GammaEngine
    os.makedirs(str(path), exist_ok=True)
    return GammaEngine(path=str(path), **kw)


def gen_clustered(n, d, seed, ncl=64, sigma=0.3):
    """clustered Gaussians around zero-mean centres: centres N(0, 1), points
    = centre + sigma N(0, 1). (Zero mean, because the inner-product tables
    train spherical centroids, which sit on the unit sphere.)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((ncl, d)).astype(np.float32)
    x = centres[rng.integers(0, ncl, size=n)] + sigma * rng.standard_normal(
        (n, d))
    return x.astype(np.float32)


def gen_queries(base, nq, seed, sigma=0.15):
    rng = np.random.default_rng(seed)
    q = base[rng.integers(0, len(base), size=nq)] + sigma * \
        rng.standard_normal((nq, base.shape[1]))
    return q.astype(np.float32)


def _params(nlist, metric, extra=""):
    return ('{"ncentroids": %d, "nb_bits": 1, "metric_type": "%s"%s}'
            % (nlist, metric, extra))


def _lists(eng, nlist, D):
    out = [eng.debug_list(ln, rr.code_size(D)) for ln in range(nlist)]
    return [i for i, _ in out], [c for _, c in out]


def _check_lists(eng, nlist, D, ip, vec_of, live_docids):
    """Every list entry (dead ones included) equals rabitq_ref.encode of
    its vector on the engine's own centroids: bits exact, factors within
    the fp32 sum bound. Every live doc sits in exactly one list, the one of
    its nearest centroid (smallest L2 / largest inner product; a centroid
    within the fp32 bound of the best counts as nearest)."""
    cent = eng.debug_model(nlist, D)[0]
    ids, codes = _lists(eng, nlist, D)
    t = _sum_tol(D)
    seen = np.concatenate(ids)
    live_seen = seen[seen >= 0]
    assert np.array_equal(np.sort(live_seen),
                          np.asarray(sorted(live_docids), dtype=np.int64))
    c64 = cent.astype(np.float64)
    for ln in range(nlist):
        if len(ids[ln]) == 0:
            continue
        vids = ids[ln] & ~MARK
        x = np.stack([vec_of(int(v)) for v in vids])
        r32, bits = rr.residual_bits(x, cent[ln])
        gb, gA, gM = rr.unpack(codes[ln], D)
        assert np.array_equal(gb, bits), ln
        A, Mul, _ = rr.factors(x, cent[ln], ip)
        n2 = (r32.astype(np.float64) ** 2).sum(axis=1)
        xx = (x.astype(np.float64) ** 2).sum(axis=1)
        assert np.all(np.abs(gA - A) <= t * (n2 + (xx if ip else 0.0))), ln
        assert np.all(np.abs(gM - Mul) <= t * np.abs(Mul)), ln
        x64 = x.astype(np.float64)
        dots = x64 @ c64.T
        mass = xx[:, None] + (c64 * c64).sum(axis=1)[None, :]
        if ip:
            score = -dots
            slack = t * np.abs(x64) @ np.abs(c64).T
        else:
            score = mass - 2.0 * dots
            slack = t * 2.0 * mass
        best = score.min(axis=1)
        assert np.all(score[:, ln] <= best + slack[:, ln] +
                      slack[np.arange(len(x)), score.argmin(axis=1)]), ln
    return cent, ids, codes


N, D0, NLIST, NQ, K = 8192, 64, 32, 64, 10


@pytest.fixture(scope="module", params=["L2", "InnerProduct"])
def built(request):
    metric = request.param
    base = gen_clustered(N, D0, seed=42)
    q = gen_queries(base, NQ, seed=1)
    eng = make_engine("/tmp/gamma_rbq_" + metric)
    # the first engine call of the module: on a build without the index
    # type CreateTable refuses it here
    eng.create_table(D0, "IVFRABITQ",
                     _params(NLIST, metric, ', "training_threshold": %d' % N))
    eng.add(base)
    eng.build_index()
    yield eng, base, q, metric == "InnerProduct"
    eng.close()


def test_engine_parity(built):
    eng, base, q, ip = built
    assert eng.num_docs() == N
    cent, ids, codes = _check_lists(eng, NLIST, D0, ip, lambda v: base[v],
                                    range(N))
    assert sum(len(i) for i in ids) == N
    nprobe = 8
    _, pl = eng.debug_coarse_assign(q, nprobe)
    assert pl.shape == (NQ, nprobe) and pl.min() >= 0 and pl.max() < NLIST
    gd, gi = eng.raw_search(q, K, nprobe=nprobe)
    for r in range(NQ):
        rr.check_row(gd[r], gi[r],
                     *rr.candidates(q[r], cent, ids, codes, pl[r], ip), ip)
    # multi-query batches of other sizes take other probe splits
    for nq in (1, 7):
        gd1, gi1 = eng.raw_search(q[:nq], K, nprobe=nprobe)
        assert np.array_equal(gi1, gi[:nq]) and np.array_equal(gd1, gd[:nq])


def _exact_scores(q, base, ids, ip):
    b = base[np.where(ids >= 0, ids, 0)].astype(np.float64)
    q64 = q.astype(np.float64)[:, None, :]
    return (b * q64).sum(axis=2) if ip else ((b - q64) ** 2).sum(axis=2)


def test_rerank_and_recall(built):
    """nprobe = every list, recall_num = 200: the exact re-rank over the
    RaBitQ candidates. recall@10 >= 0.95 against exact brute force (the
    numpy pipeline alone reaches 1.0 on such data), and the returned
    scores are the exact scores of the returned ids: within the fp32 sum
    bound of the fp64 value."""
    eng, base, q, ip = built
    wd, wi = rr.brute(q, base, K, ip)
    gd, gi = eng.raw_search(q, K, nprobe=NLIST, rerank=200)
    hits = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(wi, gi))
    recall = hits / (NQ * K)
    print("recall@10 =", recall)
    assert recall >= 0.95
    assert np.all(gi >= 0)
    ex = _exact_scores(q, base, gi, ip)
    mass = (q.astype(np.float64) ** 2).sum(axis=1)[:, None] + \
        (base[gi].astype(np.float64) ** 2).sum(axis=2)
    assert np.all(np.abs(gd - ex) <= _sum_tol(D0) * 2.0 * mass)
    # the C ABI Search with recall_num in the request's index params
    res = eng.search_pb(q[:4], topn=K,
                        index_params='{"nprobe": %d, "recall_num": 200}'
                        % NLIST)
    for t in range(4):
        assert [int(it["fields"]["_id"]) for it in res[t]["items"]] == \
            gi[t].tolist()


def test_untrained_and_brute_equal_flat(built):
    eng, base, q, ip = built
    metric = "InnerProduct" if ip else "L2"
    flat = make_engine("/tmp/gamma_rbq_flat_" + metric)
    flat.create_table(D0, "FLAT", '{"metric_type": "%s"}' % metric)
    flat.add(base)
    fd, fi = flat.raw_search(q[:16], K)
    fres = flat.search_pb(q[:4], topn=K)
    flat.close()
    raw = make_engine("/tmp/gamma_rbq_untrained_" + metric)
    raw.create_table(D0, "IVFRABITQ", _params(NLIST, metric))
    raw.add(base)
    ud, ui = raw.raw_search(q[:16], K)
    raw.close()
    assert np.array_equal(ui, fi) and np.array_equal(ud, fd)
    bres = eng.search_pb(q[:4], topn=K, brute=1)
    for t in range(4):
        assert [(it["fields"]["_id"], it["score"]) for it in bres[t]["items"]] \
            == [(it["fields"]["_id"], it["score"]) for it in fres[t]["items"]]


def test_kill(built):
    from vearch_amd import engine as eng_mod
    eng, base, q, ip = built
    eng_mod.set_kill("rbq_kill", 1)
    try:
        with pytest.raises(InterruptedError):
            eng.search_pb(q[:2], topn=K, request_id="rbq_kill",
                          partition_id=1)
    finally:
        eng_mod.clear_kill("rbq_kill", 1)
    res = eng.search_pb(q[:2], topn=K, request_id="rbq_kill", partition_id=1)
    assert len(res) == 2 and len(res[0]["items"]) == K


# --------------------------------------------------------------- mutation
D1, NLIST1, N1, NPRE = 64, 16, 3000, 2800


def _tag(key):
    return b"grp%d" % (key % 4)


@pytest.fixture(scope="module")
def doc_engine():
    """2800 docs in bulk, the build, then 200 single documents through
    FlatBuffers (the trained single-add path)"""
    from vearch_amd import fbsenc
    base = gen_clustered(N1, D1, seed=77, ncl=32)
    eng = make_engine("/tmp/gamma_rbq_docs")
    eng.create_table(D1, "IVFRABITQ",
                     _params(NLIST1, "L2", ', "training_threshold": 2000'),
                     scalar_fields=[("tag", fbsenc.DATA_STRING)])
    for vid in range(N1):
        if vid == NPRE:
            eng.build_index()
        eng.add_doc(str(vid), base[vid],
                    fields=[("tag", _tag(vid), fbsenc.DATA_STRING)])
    yield eng, base
    eng.close()


def _pb_ids(res):
    return [[int(it["fields"]["_id"]) for it in r["items"]] for r in res]


def test_mutation(doc_engine):
    from vearch_amd import fbsenc
    eng, base = doc_engine
    vec_of = {v: base[v] for v in range(N1)}     # docid -> vector
    key_of = {v: v for v in range(N1)}           # docid -> key
    gone = np.zeros(N1 + 2000, dtype=bool)
    q = gen_queries(base, 16, seed=3)
    k, nprobe = 10, 6

    def live():
        return [v for v in range(eng.num_docs()) if not gone[v]]

    def check(filtered=True):
        cent, ids, codes = _check_lists(eng, NLIST1, D1, False,
                                        lambda v: vec_of[v], live())
        _, pl = eng.debug_coarse_assign(q, nprobe)
        n_now = eng.num_docs()
        gd, gi = eng.raw_search(q, k, nprobe=nprobe)
        for r in range(len(q)):
            rr.check_row(gd[r], gi[r],
                         *rr.candidates(q[r], cent, ids, codes, pl[r], False,
                                        gone[:n_now]), False)
        assert not gone[gi[gi >= 0]].any()
        if filtered:      # term filter tag == grp1 joins the bitmap
            tags = np.array([key_of[v] % 4 for v in range(n_now)])
            res = eng.search_pb(q, topn=k,
                                index_params='{"nprobe": %d}' % nprobe,
                                term_filters=[("tag", b"grp1")])
            # keys -> docids: the live docid that carries the key
            doc = {key_of[v]: v for v in live()}
            for r in range(len(q)):
                row = res[r]["items"]
                fi = np.full(k, -1, dtype=np.int64)
                fd = np.full(k, -1.0)
                got = [int(it["fields"]["_id"]) for it in row]
                fi[:len(row)] = [doc[g] for g in got]
                fd[:len(row)] = [it["score"] for it in row]
                rr.check_row(fd, fi,
                             *rr.candidates(q[r], cent, ids, codes, pl[r],
                                            False,
                                            gone[:n_now] | (tags != 1)),
                             False)
        return gd, gi

    check()
    # the single-add docs are found by their own vector, exactly
    for vid in (NPRE, NPRE + 57, N1 - 1):
        gd, gi = eng.raw_search(base[vid:vid + 1], 1, nprobe=NLIST1,
                                rerank=50)
        assert gi[0, 0] == vid and gd[0, 0] == 0.0

    # deletes: every 7th doc
    for vid in range(0, N1, 7):
        assert eng.delete_doc(str(vid)) == 0
        gone[vid] = True
    check()
    assert eng.compact_stats()["dead"] == len(range(0, N1, 7))

    # updates of existing keys: the old entry goes, the new one is found;
    # CompactIfNeed runs after each update, and one list takes enough of
    # them to cross 30 % dead
    _, ids, _ = _check_lists(eng, NLIST1, D1, False, lambda v: vec_of[v],
                             live())
    big = int(np.argmax([len(i) for i in ids]))
    victims = [int(v) for v in ids[big] if v >= 0]
    victims = victims[:len(victims) * 2 // 5]
    before = eng.compact_stats()["buckets"]
    rng = np.random.default_rng(8)
    for vid in victims:
        new_id = eng.num_docs()
        new_vec = (vec_of[vid] + 0.01 * rng.standard_normal(D1)).astype(
            np.float32)
        eng.add_doc(str(key_of[vid]), new_vec,
                    fields=[("tag", _tag(key_of[vid]), fbsenc.DATA_STRING)])
        assert eng.num_docs() == new_id + 1
        gone[vid] = True
        vec_of[new_id] = new_vec
        key_of[new_id] = key_of[vid]
    assert eng.compact_stats()["buckets"] > before, \
        "no update crossed the compaction threshold"
    check()
    last = eng.num_docs() - 1
    gd, gi = eng.raw_search(vec_of[last][None, :], 2, nprobe=NLIST1,
                            rerank=50)
    assert gi[0, 0] == last and gd[0, 0] == 0.0 and gi[0, 1] != victims[-1]

    # on-demand compaction: every remaining dead entry goes, and the
    # search output does not change by a bit
    want = eng.raw_search(q, k, nprobe=nprobe)
    want_rr = eng.raw_search(q, k, nprobe=nprobe, rerank=100)
    dead = eng.compact_stats()["dead"]
    assert dead > 0
    st = eng.compact(0)
    assert st["removed"] == dead and st["buckets"] >= 1
    assert eng.compact_stats()["dead"] == 0
    got = eng.raw_search(q, k, nprobe=nprobe)
    got_rr = eng.raw_search(q, k, nprobe=nprobe, rerank=100)
    for a, b in zip(want + want_rr, got + got_rr):
        assert np.array_equal(a, b)
    check()
    ids, _ = _lists(eng, NLIST1, D1)
    assert all((i >= 0).all() for i in ids)


# ------------------------------------------------------------- persistence
def test_persistence_and_rebuild(capfd):
    d, nlist, n = 96, 16, 3000
    base = gen_clustered(n, d, seed=5, ncl=32)
    q = gen_queries(base, 16, seed=6)
    path = "/tmp/gamma_rbq_dump"
    tt = ', "training_threshold": 2000'
    eng = make_engine(path)
    eng.create_table(d, "IVFRABITQ", _params(nlist, "InnerProduct", tt))
    eng.add(base)
    eng.build_index()
    for vid in range(0, n, 5):
        assert eng.delete_doc(str(vid)) == 0
    cent = eng.debug_model(nlist, d)[0]
    lists = _lists(eng, nlist, d)
    want = [eng.raw_search(q, 10, nprobe=p, rerank=r)
            for p, r in ((4, 0), (nlist, 0), (nlist, 100))]
    eng.dump()
    eng.close()

    eng2 = make_engine(path)
    eng2.create_table(d, "IVFRABITQ", _params(nlist, "InnerProduct", tt))
    eng2.load()
    assert eng2.num_docs() == n
    assert np.array_equal(eng2.debug_model(nlist, d)[0], cent)
    for a, b in zip(lists, _lists(eng2, nlist, d)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    # key for key: the svals were rebuilt to the bit
    for (wd, wi), (p, r) in zip(want, ((4, 0), (nlist, 0), (nlist, 100))):
        gd, gi = eng2.raw_search(q, 10, nprobe=p, rerank=r)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    assert eng2.compact_stats()["dead"] == len(range(0, n, 5))

    # RebuildIndex retrains from the raw store: the lists follow the new
    # centroids and the search follows the lists
    from vearch_amd.engine import lib
    lib().RebuildIndex.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int]
    assert lib().RebuildIndex(eng2.h, 1, 0, 0) == 0
    deleted = np.zeros(n, dtype=bool)
    deleted[::5] = True
    cent2, ids2, codes2 = _check_lists(eng2, nlist, d, True,
                                       lambda v: base[v], range(n))
    _, pl = eng2.debug_coarse_assign(q, 4)
    gd, gi = eng2.raw_search(q, 10, nprobe=4)
    for r in range(len(q)):
        rr.check_row(gd[r], gi[r],
                     *rr.candidates(q[r], cent2, ids2, codes2, pl[r], True,
                                    deleted), True)
    eng2.close()

    # the same dump into tables it does not fit: refused with a message
    capfd.readouterr()
    for itype, params, msg in (
            ("IVFPQ", '{"ncentroids": %d, "nsubvector": 16}' % nlist,
             "dump index type IVFRABITQ != table IVFPQ"),
            ("IVFRABITQ", _params(nlist, "L2", tt), "metric"),):
        eng3 = make_engine(path)
        eng3.create_table(d, itype, params)
        with pytest.raises(RuntimeError):
            eng3.load()
        eng3.close()
        assert msg in capfd.readouterr().err
    eng4 = make_engine(path)
    eng4.create_table(64, "IVFRABITQ", _params(nlist, "InnerProduct", tt))
    with pytest.raises(RuntimeError):
        eng4.load()
    eng4.close()
    assert "dimension" in capfd.readouterr().err


# -------------------------------------------------------------- rejections
def test_rejections():
    eng = make_engine("/tmp/gamma_rbq_reject")
    base = '"ncentroids": 16, "metric_type": "L2"'
    with pytest.raises(RuntimeError, match="nb_bits: 1"):
        eng.create_table(64, "IVFRABITQ", "{%s}" % base)       # absent
    for nb in (2, 9):
        with pytest.raises(RuntimeError, match="nb_bits: 1"):
            eng.create_table(64, "IVFRABITQ",
                             '{%s, "nb_bits": %d}' % (base, nb))
    ok = base + ', "nb_bits": 1'
    with pytest.raises(RuntimeError, match=r"qb"):
        eng.create_table(64, "IVFRABITQ", '{%s, "qb": 9}' % ok)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        eng.create_table(40, "IVFRABITQ", "{%s}" % ok)
    with pytest.raises(RuntimeError, match="4096"):
        eng.create_table(4096 + 32, "IVFRABITQ", "{%s}" % ok)
    with pytest.raises(RuntimeError, match="hnsw"):
        eng.create_table(64, "IVFRABITQ",
                         '{%s, "hnsw": {"nlinks": 32}}' % ok)
    with pytest.raises(RuntimeError, match="nprobe"):
        eng.create_table(64, "IVFRABITQ", '{%s, "nprobe": 17}' % ok)
    # accepted: qb and centered in range are parsed and ignored, and the
    # default nprobe of 80 on 16 lists probes every list
    eng.create_table(64, "IVFRABITQ",
                     '{%s, "qb": 4, "centered": true}' % ok)
    eng.add(np.zeros((4, 64), dtype=np.float32))
    assert eng.num_docs() == 4
    eng.close()
