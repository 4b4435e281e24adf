"""GPU tests of IVFRABITQ with nb_bits 4 and 8: the encode, sval and scan
kernels through their test hooks, then the engine. The reference is
tests/rabitq_ex_ref.py; tolerances come from the fp32 format, never from
what the kernels return. Case builders are those of test_gpu_rabitq.py."""
import numpy as np
import pytest

import rabitq_ex_ref as rx
import rabitq_ref as rr
from oracle import kernel_refs as kr
from test_gpu_rabitq import (BS_SIZES, MARK32, NQ_SCAN, _cands,
                             _exact_scores, _scan_case, _sum_tol,
                             gen_clustered, gen_queries, make_engine)

pytestmark = pytest.mark.gpu

BITS = [4, 8]
METRICS = [False, True]


# ------------------------------------------------------------ encode kernel
@pytest.mark.parametrize("ip", METRICS)
@pytest.mark.parametrize("D", [32, 96, 128, 288, 1024])
@pytest.mark.parametrize("B", BITS)
def test_kernel_encode(B, D, ip):
    """The code is one of the 32 float32 candidates exactly, and that
    candidate's fp64 objective is within D 2^-22 of the best: num is a fp32
    sum of D positive terms (relative error D 2^-24), squared, on either
    side of the comparison. D = 288 and 1024 take the encoder's other two
    register schemes."""
    from vearch_amd import ktest
    rng = np.random.default_rng(100 * B + D)
    n, nlist = 300, 3
    cent = rng.standard_normal((nlist, D)).astype(np.float32)
    asg = rng.integers(0, nlist, size=n).astype(np.int32)
    x = (cent[asg] + 0.4 * rng.standard_normal((n, D))).astype(np.float32)
    x[0] = cent[asg[0]]                      # rmax = 0
    x[1] = cent[asg[1]]
    x[1, 5] += 1.0                           # one non-zero component
    x[2, 3::4] = cent[asg[2], 3::4]          # r_j = 0 in places
    c = cent[asg]
    r32 = (x - c).astype(np.float32)
    ent, sv = ktest.rabitq_encode(x, asg, cent, ip, nb_bits=B)
    ent2, sv2 = ktest.rabitq_encode(x, asg, cent, ip, nb_bits=B)
    assert np.array_equal(ent, ent2) and np.array_equal(sv, sv2)
    u, gA, gM = rx.unpack(ent, D, B)
    assert np.array_equal(u >> (B - 1), (r32 > 0).astype(np.int64))
    m = rx.candidates32(r32, B)
    hit = (rx.codes_of(m, r32[None], B) == u[None]).all(axis=2)   # (32, n)
    assert hit.any(axis=0).all()
    obj = rx.objective(m, r32)
    chosen = np.where(hit, obj, -np.inf).max(axis=0)
    assert np.all(chosen >= obj.max(axis=0) * (1.0 - D * 2.0 ** -22))
    assert np.all(u[0] == (1 << (B - 1)) - 1) and gM[0] == 1.0
    A, Mul, sval = rx.factors(u, x, c, B, ip)
    t = _sum_tol(D)
    mass = (r32.astype(np.float64) ** 2).sum(axis=1)
    if ip:
        mass = mass + (x.astype(np.float64) ** 2).sum(axis=1)
    assert np.all(np.abs(gA - A) <= t * mass)
    assert np.all(np.abs(gM - Mul) <= t * np.abs(Mul))
    assert np.all(np.abs(sv - sval)
                  <= t * (u * np.abs(c.astype(np.float64))).sum(axis=1))
    # the Load-time rebuild gives the encoder's svals bit for bit
    buckets = [ent[asg == ln] for ln in range(nlist)]
    got = ktest.rabitq_sval_buckets(buckets, cent, nb_bits=B)
    for ln in range(nlist):
        k = len(buckets[ln])
        assert np.array_equal(got[ln][:k], sv[asg == ln])
        assert np.all(got[ln][k:] == ktest.SVAL_CANARY)


# -------------------------------------------------------------- scan kernel
SIZES = [0, 1, 63, 64, 65] + BS_SIZES[2:] + [3 + (i % 5) for i in range(34)]


def _encoded_lists(B, D, cent, ids, vecs, queries, marks, dyadic, ip):
    """the encode kernel's entries of the lists in the scan hook's form
    (ids carrying the delete marks), and per list the reference estimates
    with their bounds: 2^-20 scale for dyadic inputs, else _sum_tol(D)"""
    from vearch_amd import ktest
    sizes = [len(i) for i in ids]
    asg = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    cut = np.cumsum(sizes)[:-1]
    ent, sv = ktest.rabitq_encode(np.concatenate(vecs), asg, cent, ip,
                                  nb_bits=B)
    dev, tab = [], []
    for ln, (e, s) in enumerate(zip(np.split(ent, cut), np.split(sv, cut))):
        dev.append((np.where(marks[ln], ids[ln] | MARK32, ids[ln]), e, s))
        u, A, Mul = rx.unpack(e, D, B)
        sc = [rx.scale(q, cent[ln], A, Mul, B, ip) for q in queries]
        tab.append((np.stack([rx.estimate(q, cent[ln], u, A, Mul, B, ip)
                              for q in queries]),
                    np.stack(sc) * (2.0 ** -20 if dyadic else _sum_tol(D))))
    return dev, tab


def _check_rows(keys, od, oi, tab, ids, marks, bm, probes, S, ip):
    """raw partial rows against their sub-block's probes, merged rows
    against all probes"""
    for r in range(NQ_SCAN):
        for s in range(S):
            rr.check_row(*kr.key_decode(keys[r, s], ip),
                         *_cands(tab, ids, marks, bm,
                                 probes[r, s::S].tolist(), r), ip)
        rr.check_row(od[r], oi[r],
                     *_cands(tab, ids, marks, bm, probes[r].tolist(), r), ip)


@pytest.mark.parametrize("D,dyadic",
                         [(D, dy) for D in (32, 96, 128, 288)
                          for dy in (True, False)] + [(64, True), (256, True)])
@pytest.mark.parametrize("B", BITS)
def test_kernel_scan(B, D, dyadic, monkeypatch):
    """Dyadic inputs (multiples of 1/16 in [-4, 4]): every sum the kernel
    forms is exact in fp32 in any order, and the few rounded scalar
    operations behind them are bounded by 2^-20 scale. Gaussian inputs:
    rabitq_ex_ref.tol. List sizes around the wave and both block sizes, 49
    probes (two chunks; one -1, one out of range), delete marks and a
    bitmap at ~30 % each; raw partial rows and rows merged by sort_rows.
    The entries are the encode kernel's. Over both widths the D cover every
    register-resident scan (4 bits: 64, 128, 256; 8 bits: 32, 64, 128) and
    the streamed one."""
    from vearch_amd import ktest
    id_space = sum(SIZES) + 64
    cent, ids, vecs, queries, probes = _scan_case(D, 1000 * B + D, dyadic,
                                                  SIZES, id_space)
    rng = np.random.default_rng(D)
    marks = [rng.random(n) < 0.3 for n in SIZES]
    bm = rng.random(id_space) < 0.3
    for ip in METRICS:
        dev, tab = _encoded_lists(B, D, cent, ids, vecs, queries, marks,
                                  dyadic, ip)
        for bs in (512, 256):
            monkeypatch.setenv("GAMMA_SCAN_BS", str(bs))
            for S, k2 in [(S, k2) for S in (1, 3) for k2 in (1, 10, 200)]:
                keys, od, oi = ktest.rabitq_scan(
                    dev, probes, queries, cent, S, k2, ip,
                    bitmap=kr.bitmap_words(bm), kill_flag=True, nb_bits=B)
                assert keys.shape == (NQ_SCAN, S, k2)
                _check_rows(keys, od, oi, tab, ids, marks, bm, probes, S, ip)


@pytest.mark.parametrize("B", BITS)
def test_kernel_scan_kill_flag(B):
    """test_gpu_rabitq.py's kill-flag test for the multi-bit widths: a flag
    raised before the launch is read at the first chunk close, so every key
    is EMPTY and every id -1; a flag left at 0 changes nothing. The 1-bit
    test's lists (46 probes, two chunks at S = 1), dyadic, D = 32: streamed
    at 4 bits, register-resident at 8."""
    from vearch_amd import ktest
    sizes = BS_SIZES + [3 + (i % 5) for i in range(34)]
    cent, ids, vecs, queries, probes = _scan_case(32, 532 + B, True, sizes,
                                                  int(sum(sizes)) + 64)
    assert probes.shape[1] > 32
    marks = [np.zeros(n, dtype=bool) for n in sizes]
    for ip in METRICS:
        dev, tab = _encoded_lists(B, 32, cent, ids, vecs, queries, marks,
                                  True, ip)
        for S, k2 in ((1, 10), (2, 1024)):
            keys, _, oi = ktest.rabitq_scan(dev, probes, queries, cent, S,
                                            k2, ip, kill_flag=1, nb_bits=B)
            assert keys.shape == (NQ_SCAN, S, k2)
            assert np.all(keys == np.uint64(kr.EMPTY)), (ip, S, k2)
            assert np.all(oi == -1)
            keys, od, oi = ktest.rabitq_scan(dev, probes, queries, cent, S,
                                             k2, ip, kill_flag=0, nb_bits=B)
            assert keys.shape == (NQ_SCAN, S, k2)
            _check_rows(keys, od, oi, tab, ids, marks, None, probes, S, ip)


# ------------------------------------------------------------------- engine
N, D0, NLIST, NQ, K = 8192, 64, 16, 64, 10


def _params(nlist, nb, ip, tt):
    return ('{"ncentroids": %d, "nb_bits": %d, "metric_type": "%s", '
            '"training_threshold": %d}'
            % (nlist, nb, "InnerProduct" if ip else "L2", tt))


def _lists(eng, nlist, D, B):
    out = [eng.debug_list(ln, rx.code_size(D, B)) for ln in range(nlist)]
    return [i for i, _ in out], [c for _, c in out]


def _check_search(eng, q, nlist, D, B, ip, nprobe, gone=None):
    """raw_search against the reference over the engine's own lists"""
    cent = eng.debug_model(nlist, D)[0]
    ids, codes = _lists(eng, nlist, D, B)
    _, pl = eng.debug_coarse_assign(q, nprobe)
    gd, gi = eng.raw_search(q, K, nprobe=nprobe)
    for r in range(len(q)):
        rr.check_row(gd[r], gi[r],
                     *rx.candidates(q[r], cent, ids, codes, pl[r], B, ip,
                                    gone), ip)
    return ids, gi


def _recall(want, got):
    return sum(len(set(a.tolist()) & set(b.tolist()))
               for a, b in zip(want, got)) / want.size


@pytest.fixture(scope="module",
                params=[(B, ip) for B in BITS for ip in METRICS],
                ids=lambda p: "B%d-%s" % (p[0], "ip" if p[1] else "l2"))
def built(request):
    B, ip = request.param
    base = gen_clustered(N, D0, seed=42)
    q = gen_queries(base, NQ, seed=1)
    eng = make_engine("/tmp/gamma_rbqx_%d_%d" % (B, ip))
    eng.create_table(D0, "IVFRABITQ", _params(NLIST, B, ip, N))
    eng.add(base)
    eng.build_index()
    yield eng, base, q, B, ip
    eng.close()


def test_engine_parity(built):
    eng, base, q, B, ip = built
    ids, gi = _check_search(eng, q, NLIST, D0, B, ip, 6)
    assert sum(len(i) for i in ids) == N
    for nq in (1, 7):       # other batch sizes take other probe splits
        assert np.array_equal(eng.raw_search(q[:nq], K, nprobe=6)[1], gi[:nq])


def test_rerank_and_recall(built):
    """The 1-bit engine test's gate at recall_num = 200; at recall_num = 0
    the 4-bit table is no worse than a 1-bit table over the same data. The
    two numpy references alone, this seed, 16 Lloyd centroids: 0.325 (1
    bit) / 0.786 (4 bits) for L2, 0.572 / 0.900 for inner product."""
    eng, base, q, B, ip = built
    _, wi = rr.brute(q, base, K, ip)
    gd, gi = eng.raw_search(q, K, nprobe=NLIST, rerank=200)
    assert _recall(wi, gi) >= 0.95 and np.all(gi >= 0)
    mass = (q.astype(np.float64) ** 2).sum(axis=1)[:, None] + \
        (base[gi].astype(np.float64) ** 2).sum(axis=2)
    assert np.all(np.abs(gd - _exact_scores(q, base, gi, ip))
                  <= _sum_tol(D0) * 2.0 * mass)
    if B == 4:
        one = make_engine("/tmp/gamma_rbqx_one_%d" % ip)
        one.create_table(D0, "IVFRABITQ", _params(NLIST, 1, ip, N))
        one.add(base)
        one.build_index()
        r1 = _recall(wi, one.raw_search(q, K, nprobe=NLIST)[1])
        one.close()
        r4 = _recall(wi, eng.raw_search(q, K, nprobe=NLIST)[1])
        assert r4 >= r1


@pytest.mark.parametrize("B", BITS)
def test_mutation(B):
    """Single adds, a delete, updates that push one list over the
    compaction threshold, compact(): the search still equals the reference."""
    n, nlist, nprobe = 3000, 16, 6
    base = gen_clustered(n, D0, seed=77, ncl=32)
    q = gen_queries(base, 16, seed=3)
    eng = make_engine("/tmp/gamma_rbqx_mut_%d" % B)
    eng.create_table(D0, "IVFRABITQ", _params(nlist, B, False, 2000))
    for vid in range(n):         # keyed documents; the last 200 are single
        if vid == 2800:          # adds into the trained index
            eng.build_index()
        eng.add_doc(str(vid), base[vid])
    gone = np.zeros(2 * n, dtype=bool)
    vec_of = {v: base[v] for v in range(n)}

    def check():
        return _check_search(eng, q, nlist, D0, B, False, nprobe,
                             gone[:eng.num_docs()])[0]

    check()
    new = (base[5] + 0.05).astype(np.float32)
    eng.add_doc(str(n), new)                               # single add
    vec_of[n] = new
    gd, gi = eng.raw_search(new[None, :], 1, nprobe=nlist, rerank=50)
    assert gi[0, 0] == n and gd[0, 0] == 0.0
    assert eng.delete_doc("7") == 0
    gone[7] = True
    ids = check()
    big = int(np.argmax([len(i) for i in ids]))
    victims = [int(v) for v in ids[big] if v >= 0]
    # x updates of a list of L leave x dead among L + x entries: the 30 %
    # threshold is crossed at x = 0.43 L
    victims = victims[:len(victims) * 3 // 5]
    before = eng.compact_stats()["buckets"]
    for vid in victims:                                    # updates
        docid = eng.num_docs()
        vec_of[docid] = (vec_of[vid] + 0.01).astype(np.float32)
        eng.add_doc(str(vid), vec_of[docid])
        gone[vid] = True
    assert eng.compact_stats()["buckets"] > before, \
        "no update crossed the compaction threshold"
    check()
    want = eng.raw_search(q, K, nprobe=nprobe)
    dead = eng.compact_stats()["dead"]
    assert dead > 0 and eng.compact(0)["removed"] == dead
    for a, b in zip(want, eng.raw_search(q, K, nprobe=nprobe)):
        assert np.array_equal(a, b)
    ids = check()
    assert all((i >= 0).all() for i in ids)
    eng.close()


def test_persistence(capfd):
    d, nlist, n = 96, 16, 3000
    base = gen_clustered(n, d, seed=5, ncl=32)
    q = gen_queries(base, 16, seed=6)
    path = "/tmp/gamma_rbqx_dump"
    eng = make_engine(path)
    eng.create_table(d, "IVFRABITQ", _params(nlist, 4, True, 2000))
    eng.add(base)
    eng.build_index()
    for vid in range(0, n, 5):
        assert eng.delete_doc(str(vid)) == 0
    lists = _lists(eng, nlist, d, 4)
    runs = ((4, 0), (nlist, 0), (nlist, 100))
    want = [eng.raw_search(q, K, nprobe=p, rerank=r) for p, r in runs]
    eng.dump()
    eng.close()
    eng2 = make_engine(path)
    eng2.create_table(d, "IVFRABITQ", _params(nlist, 4, True, 2000))
    eng2.load()
    for a, b in zip(lists, _lists(eng2, nlist, d, 4)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    for (wd, wi), (p, r) in zip(want, runs):   # the svals came back exactly
        gd, gi = eng2.raw_search(q, K, nprobe=p, rerank=r)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    eng2.close()
    capfd.readouterr()
    for nb in (1, 8):
        eng3 = make_engine(path)
        eng3.create_table(d, "IVFRABITQ", _params(nlist, nb, True, 2000))
        with pytest.raises(RuntimeError):
            eng3.load()
        eng3.close()
        assert "nb_bits 4" in capfd.readouterr().err


def test_rejections():
    eng = make_engine("/tmp/gamma_rbqx_reject")
    base = '"ncentroids": 16, "metric_type": "L2"'
    with pytest.raises(RuntimeError, match="nb_bits: 1"):
        eng.create_table(64, "IVFRABITQ", "{%s}" % base)
    for nb in (2, 3, 5, 6, 7, 9):
        with pytest.raises(RuntimeError, match="nb_bits: 1, nb_bits: 4"):
            eng.create_table(64, "IVFRABITQ",
                             '{%s, "nb_bits": %d}' % (base, nb))
    eng.create_table(64, "IVFRABITQ", '{%s, "nb_bits": 8}' % base)
    eng.add(np.zeros((4, 64), dtype=np.float32))
    assert eng.num_docs() == 4
    eng.close()
