"""GPU tests of the BINARYIVF index: the three Hamming kernels through
their test hooks, then the engine through GammaEngine and the C ABI.

Everything is integer arithmetic, so every comparison is np.array_equal
against tests/binary_ref.py (pinned by tests/test_binary_ref.py); ties are
resolved by the engine's (dist, id) ascending order on both sides.
"""
import ctypes
import os

import numpy as np
import pytest

import binary_ref as br
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu

MARK = np.int64(-2 ** 63)            # host-side bit-63 delete mark
MARK32 = np.uint32(0x80000000)       # device-side bit-31 delete mark
WORDS = [1, 2, 3, 4, 8, 32]          # every load width + an odd count


def _rand_bytes(rng, n, W):
    return rng.integers(0, 256, size=(n, 4 * W), dtype=np.uint8)


# ------------------------------------------------------------ hamming_matrix
@pytest.mark.parametrize("W", WORDS)
def test_kernel_hamming_matrix(W):
    from vearch_amd import ktest
    rng = np.random.default_rng(100 + W)
    for nq in (1, 3, 65):
        for n in (1, 63, 64, 65, 257):
            Q = _rand_bytes(rng, nq, W)
            B = _rand_bytes(rng, n, W)
            B[0] = Q[0]                  # identical rows: distance 0
            B[n - 1] = ~Q[nq - 1]        # complementary rows: distance d
            got = ktest.hamming_matrix(Q, B)
            want = br.hamming(Q, B).astype(np.float32)
            assert np.array_equal(got, want), (nq, n)
            assert got[nq - 1, n - 1] == 32 * W
            if n > 1:
                assert got[0, 0] == 0


# --------------------------------------------------------------- binivf_scan
SIZES = [0, 1, 63, 64, 65, 511, 513, 1500]
REPEATED = 5                         # this list is one vector repeated
ID_SPACE = 4096
NQ_SCAN = 4


def _scan_case(W, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(ID_SPACE)
    ids, codes, pos = [], [], 0
    for ln, n in enumerate(SIZES):
        ids.append(perm[pos:pos + n].astype(np.uint32))
        c = _rand_bytes(rng, n, W)
        if ln == REPEATED:
            c[:] = c[0]
        codes.append(c)
        pos += n
    queries = _rand_bytes(rng, NQ_SCAN, W)
    queries[1] = codes[REPEATED][0]  # distance 0 to a whole list
    nlist = len(SIZES)
    probes = np.stack([rng.permutation(nlist) for _ in range(NQ_SCAN)])
    probes = probes.astype(np.int64)
    for r in range(NQ_SCAN):         # one -1 and one >= nlist per query
        probes[r, (2 * r) % nlist] = -1
        probes[r, (2 * r + 3) % nlist] = nlist + r
    return ids, codes, queries, probes


def _expected_partials(ids, codes, queries, probes, S, k2, marks, deleted):
    """the (nq, S, k2) keys the kernel must write: sub-block s of a query
    holds the top-k2 of its probes s, s+S, ..."""
    nq, nprobe = probes.shape
    out = np.full((nq, S, k2), kr.EMPTY, dtype=np.uint64)
    for r in range(nq):
        for s in range(S):
            ci, cd = [], []
            for ln in probes[r, s::S].tolist():
                if ln < 0 or ln >= len(ids) or len(ids[ln]) == 0:
                    continue
                live = ~marks[ln]
                ci.append(ids[ln][live])
                cd.append(br.hamming(queries[r:r + 1], codes[ln][live])[0])
            if ci:
                out[r, s] = kr.topk_keys(np.concatenate(cd),
                                         np.concatenate(ci), k2, False,
                                         deleted)
    return out


def _run_scan_modes(W, k2s, Ss):
    from vearch_amd import ktest
    ids, codes, queries, probes = _scan_case(W, 200 + W)
    rng = np.random.default_rng(300 + W)
    no_marks = [np.zeros(n, dtype=bool) for n in SIZES]
    some_marks = [rng.random(n) < 0.3 for n in SIZES]
    all_marks = [np.ones(n, dtype=bool) for n in SIZES]
    bm = rng.random(ID_SPACE) < 0.3
    modes = [("none", no_marks, None), ("marks", some_marks, None),
             ("bitmap", no_marks, bm), ("both", some_marks, bm),
             ("all", all_marks, None)]
    for name, marks, deleted in modes:
        dev_ids = [np.where(m, i | MARK32, i).astype(np.uint32)
                   for i, m in zip(ids, marks)]
        host_ids = [np.where(m, i.astype(np.int64) | MARK,
                             i.astype(np.int64)) for i, m in zip(ids, marks)]
        words = None if deleted is None else kr.bitmap_words(deleted)
        for S in Ss:
            for k2 in k2s:
                keys, od, oi = ktest.binivf_scan(
                    list(zip(dev_ids, codes)), probes, queries, S, k2,
                    bitmap=words, kill_flag=(S == 4))
                want = _expected_partials(ids, codes, queries, probes, S,
                                          k2, marks, deleted)
                assert np.array_equal(keys, want), (name, S, k2)
                if od is None:       # S * k2 > 2048: merge on the host
                    od, oi = kr.key_decode(
                        np.sort(keys.reshape(NQ_SCAN, -1))[:, :k2], False)
                wd, wi = br.search(queries, host_ids, codes, probes, k2,
                                   deleted)
                assert np.array_equal(oi, wi), (name, S, k2)
                assert np.array_equal(od, wd), (name, S, k2)
                if name == "all":
                    assert np.all(keys == np.uint64(kr.EMPTY))
    # the repeated-vector list alone: every distance equal, order by id
    only = np.full((NQ_SCAN, 8), -1, dtype=np.int64)
    only[:, 3] = REPEATED
    _, od, oi = ktest.binivf_scan(list(zip(ids, codes)), only, queries, 1,
                                  100)
    want_ids = np.sort(ids[REPEATED].astype(np.int64))[:100]
    for r in range(NQ_SCAN):
        assert np.array_equal(oi[r], want_ids)
        assert np.all(od[r] == od[r, 0])
    assert np.all(od[1] == 0.0)


@pytest.mark.parametrize("W", WORDS)
def test_kernel_binivf_scan(W):
    """k2 = 1024 exceeds the live candidates of the probed lists in the
    deleting modes (EMPTY padding); S = 4 runs with a non-null kill flag
    left at 0."""
    _run_scan_modes(W, k2s=(1, 10, 100, 1024), Ss=(1, 4))


@pytest.mark.parametrize("W", [3, 8, 32])
def test_kernel_binivf_scan_bs256(W, monkeypatch):
    monkeypatch.setenv("GAMMA_SCAN_BS", "256")
    _run_scan_modes(W, k2s=(10, 1024), Ss=(1, 4))


def test_kernel_binivf_scan_kill_flag():
    """A flag raised before the launch is read at the first chunk close:
    the launch returns and every row is EMPTY. A flag left at 0 changes
    nothing. The W = 1 case with its probe rows repeated five times: 40
    probes, two chunks at S = 1. k2 = 1024 is the largest the launcher
    takes, and k2 + 2 * 512 = 2048 still fits the selector, so this kernel
    only ever checks every second pass; a k2 above that bound cannot be
    launched."""
    from vearch_amd import ktest
    ids, codes, queries, probes = _scan_case(1, 201)
    probes = np.tile(probes, 5)
    assert probes.shape[1] > 32
    lists = list(zip(ids, codes))
    no_marks = [np.zeros(n, dtype=bool) for n in SIZES]
    for S, k2 in ((1, 10), (2, 1024)):
        keys, _, oi = ktest.binivf_scan(lists, probes, queries, S, k2,
                                        kill_flag=1)
        assert keys.shape == (NQ_SCAN, S, k2)
        assert np.all(keys == np.uint64(kr.EMPTY)), (S, k2)
        assert np.all(oi == -1)
        keys, _, _ = ktest.binivf_scan(lists, probes, queries, S, k2,
                                       kill_flag=0)
        want = _expected_partials(ids, codes, queries, probes, S, k2,
                                  no_marks, None)
        assert np.array_equal(keys, want), (S, k2)


# --------------------------------------------------------- hamming_flat_scan
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_kernel_hamming_flat_scan(W):
    from vearch_amd import ktest
    rng = np.random.default_rng(400 + W)
    seg_shift = 10                   # 5000 vectors span 5 segments
    for n in (1, 255, 256, 257, 5000):
        base = _rand_bytes(rng, n, W)
        q = _rand_bytes(rng, 3, W)
        q[0] = base[n // 2]
        h = br.hamming(q, base)
        deleted = rng.random(n) < 0.3
        for dl in (None, deleted):
            words = None if dl is None else kr.bitmap_words(dl)
            for k2 in (10, 300):     # 300 > n for the small sizes
                got = ktest.hamming_flat_scan(q, base, seg_shift, k2,
                                              bitmap=words)
                want = kr.topk_keys_rows(h, np.arange(n), k2, False, dl)
                assert np.array_equal(got, want), (n, k2, dl is not None)


# ------------------------------------------------------------- engine level
def make_engine(path, **kw):
    from vearch_amd import GammaEngine
    os.makedirs(str(path), exist_ok=True)
    return GammaEngine(path=str(path), **kw)


def gen_binary(n, d, seed, ncl=40, flip=0.10):
    """random cluster centres with ~10 % of the bits flipped per point"""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 2, size=(ncl, d), dtype=np.uint8)
    bits = centres[rng.integers(0, ncl, size=n)]
    bits ^= (rng.random((n, d)) < flip).astype(np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


def _params(nlist, extra=""):
    return '{"ncentroids": %d%s}' % (nlist, extra)


def _lists(eng, nlist, nbytes):
    out = [eng.debug_list(ln, nbytes) for ln in range(nlist)]
    return [i for i, _ in out], [c for _, c in out]


def _check_lists(eng, nlist, base_of, live_docids):
    """Every live doc sits in the list binary_ref.assign gives for it, in
    docid order, with its own bytes as the code."""
    nbytes = eng.d // 8
    cent = eng.debug_binary_centroids(nlist)
    ids, codes = _lists(eng, nlist, nbytes)
    live_docids = np.asarray(sorted(live_docids), dtype=np.int64)
    vecs = np.stack([base_of(int(v)) for v in live_docids])
    asg = br.assign(vecs, cent)
    for ln in range(nlist):
        live = ids[ln] >= 0
        assert np.array_equal(ids[ln][live], live_docids[asg == ln]), ln
        assert np.array_equal(codes[ln][live], vecs[asg == ln]), ln
    return cent, ids, codes


CONFIGS = {"d128": (128, 16, 8000, ""),
           "d256": (256, 64, 20000, ', "training_threshold": 20000')}


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def built(request):
    d, nlist, n, extra = CONFIGS[request.param]
    base = gen_binary(n, d, seed=d)
    rng = np.random.default_rng(d + 1)
    q = base[rng.integers(0, n, size=2048)].copy()
    q ^= np.packbits(rng.random((2048, d)) < 0.05, axis=1,
                     bitorder="little")
    eng = make_engine("/tmp/gamma_bin_" + request.param)
    eng.create_table(d, "BINARYIVF", _params(nlist, extra))
    eng.add(base)
    eng.build_index()
    yield eng, base, q, nlist
    eng.close()


# 1 ---------------------------------------------------------------------
def test_build_and_parity(built):
    eng, base, q, nlist = built
    n = len(base)
    assert eng.num_docs() == n
    cent, ids, codes = _check_lists(eng, nlist, lambda v: base[v], range(n))
    assert sum(len(i) for i in ids) == n
    nprobe = 4
    for nq in (64, 2048):            # probe split S > 1, then S = 1
        pd, pl = eng.debug_coarse_assign(q[:nq], nprobe)
        wd, wl = br.coarse(q[:nq], cent, nprobe)
        assert np.array_equal(pl, wl) and np.array_equal(pd, wd)
        rd, ri = br.search(q[:nq], ids, codes, pl, 100)
        for k in (1, 10, 100):
            gd, gi = eng.raw_search(q[:nq], k, nprobe=nprobe)
            assert np.array_equal(gi, ri[:, :k]), (nq, k)
            assert np.array_equal(gd, rd[:, :k]), (nq, k)
    # a search-time nprobe above nlist falls back to the index default
    # (20, clamped to nlist by the search)
    dflt = min(20, nlist)
    pd, pl = eng.debug_coarse_assign(q[:8], dflt)
    rd, ri = br.search(q[:8], ids, codes, pl, 10)
    for bad in (nlist + 1, 0):
        gd, gi = eng.raw_search(q[:8], 10, nprobe=bad)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


# 2 ---------------------------------------------------------------------
def test_all_lists_probed_is_exact(built):
    eng, base, q, nlist = built
    nq, k = 32, 10
    wd, wi = br.brute(q[:nq], base, k)
    gd, gi = eng.raw_search(q[:nq], k, nprobe=nlist)
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    bd, bi = eng.raw_search(q[:nq], k, brute=1)
    assert np.array_equal(bi, wi) and np.array_equal(bd, wd)
    # a table that was never built searches its raw store
    raw = make_engine("/tmp/gamma_bin_untrained_%d" % eng.d)
    raw.create_table(eng.d, "BINARYIVF", _params(nlist))
    raw.add(base)
    ud, ui = raw.raw_search(q[:nq], k)
    raw.close()
    assert np.array_equal(ui, wi) and np.array_equal(ud, wd)


# 3, 4 ------------------------------------------------------------------
D1, NLIST1, N1 = 128, 16, 2000


def _tag(vid):
    return b"grp%d" % (vid % 4)


@pytest.fixture(scope="module")
def doc_engine():
    """table filled one document at a time through FlatBuffers: 1800 docs
    before the build, 200 after it (the trained single-add path)"""
    from vearch_amd import fbsenc
    base = gen_binary(N1, D1, seed=77)
    eng = make_engine("/tmp/gamma_bin_docs")
    eng.create_table(D1, "BINARYIVF", _params(NLIST1),
                     scalar_fields=[("tag", fbsenc.DATA_STRING)])
    for vid in range(N1):
        if vid == 1800:
            eng.build_index()
        eng.add_doc(str(vid), base[vid],
                    fields=[("tag", _tag(vid), fbsenc.DATA_STRING)])
    yield eng, base
    eng.close()


def _pb_rows(res):
    return ([[int(it["fields"]["_id"]) for it in r["items"]] for r in res],
            [[it["score"] for it in r["items"]] for r in res])


def test_single_doc_path(doc_engine):
    eng, base = doc_engine
    rng = np.random.default_rng(9)
    q = base[rng.integers(0, N1, size=8)].copy()
    q[:, 0] ^= 0x5A
    # same data through the bulk path: same model, same lists
    bulk = make_engine("/tmp/gamma_bin_docs_bulk")
    bulk.create_table(D1, "BINARYIVF", _params(NLIST1))
    bulk.add(base[:1800])
    bulk.build_index()
    bulk.add(base[1800:])
    nbytes = D1 // 8
    assert np.array_equal(eng.debug_binary_centroids(NLIST1),
                          bulk.debug_binary_centroids(NLIST1))
    for a, b in zip(_lists(eng, NLIST1, nbytes), _lists(bulk, NLIST1, nbytes)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    k, nprobe = 10, 4
    wd, wi = bulk.raw_search(q, k, nprobe=nprobe)
    bulk.close()
    gd, gi = eng.raw_search(q, k, nprobe=nprobe)
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    assert np.all(wi >= 0)
    # protobuf Search with nq * d/8 query bytes
    res = eng.search_pb(q, topn=k, index_params='{"nprobe": %d}' % nprobe,
                        fields=("_id", "tag"), is_vector_value=True)
    assert len(res) == len(q)
    pid, psc = _pb_rows(res)
    for t in range(len(q)):
        assert pid[t] == wi[t].tolist()
        assert psc[t] == [float(x) for x in wd[t]]
        for it in res[t]["items"]:
            vid = int(it["fields"]["_id"])
            assert it["fields"]["tag"] == _tag(vid)
            assert it["fields"][eng.vec_name] == base[vid].tobytes()
    # offset paging: ranks [3, 8) of the same order
    paged = eng.search_pb(q[:2], topn=5, offset=3,
                          index_params='{"nprobe": %d}' % nprobe)
    for t in range(2):
        assert _pb_rows(paged)[0][t] == wi[t, 3:8].tolist()
    # max_score cut (scores are Hamming distances)
    for t in range(2):
        cut = float(wd[t, 4])
        r = eng.search_pb(q[t:t + 1], topn=k, min_score=0.0, max_score=cut,
                          index_params='{"nprobe": %d}' % nprobe)
        keep = wd[t] <= cut
        assert _pb_rows(r)[0][0] == wi[t][keep].tolist()
    # brute flag of the request, and the doc fetch returns the stored bytes
    wbd, wbi = br.brute(q[:2], base, k)
    rb = eng.search_pb(q[:2], topn=k, brute=1)
    assert _pb_rows(rb)[0] == wbi.tolist()
    docs = eng.query_pb(document_ids=["7", "1999"], is_vector_value=True)
    got = {it["fields"]["_id"]: it["fields"][eng.vec_name]
           for it in docs[0]["items"]}
    assert got == {b"7": base[7].tobytes(), b"1999": base[1999].tobytes()}
    # topn + offset above 1024 keeps the existing limit and message
    with pytest.raises(RuntimeError, match="1024"):
        eng.search_pb(q[:1], topn=1000, offset=100)


class _Model:
    """host model of the lists under delete / update / compaction"""

    def __init__(self, cent, ids, codes):
        self.cent = cent
        self.ids = [i.copy() for i in ids]
        self.codes = [c.copy() for c in codes]
        self.buckets = self.removed = 0

    def dead(self):
        return int(sum((i < 0).sum() for i in self.ids))

    def delete(self, vid):
        for i in self.ids:
            i[i == vid] |= MARK

    def append(self, vid, vec):
        ln = int(br.assign(vec[None, :], self.cent)[0])
        self.ids[ln] = np.append(self.ids[ln], np.int64(vid))
        self.codes[ln] = np.concatenate([self.codes[ln], vec[None, :]])

    def compact(self, ratio):
        done = removed = 0
        for ln, i in enumerate(self.ids):
            dead = int((i < 0).sum())
            if dead > 0 and (ratio <= 0 or np.float32(dead) / np.float32(
                    len(i)) >= np.float32(ratio)):
                self.ids[ln] = i[i >= 0]
                self.codes[ln] = self.codes[ln][i >= 0]
                done += 1
                removed += dead
        self.buckets += done
        self.removed += removed
        return {"buckets": done, "removed": removed}

    def stats(self):
        return {"buckets": self.buckets, "removed": self.removed,
                "dead": self.dead()}

    def check(self, eng):
        ids, codes = _lists(eng, len(self.ids), self.cent.shape[1])
        for ln in range(len(ids)):
            assert np.array_equal(ids[ln], self.ids[ln]), ln
            assert np.array_equal(codes[ln], self.codes[ln]), ln
        assert eng.compact_stats() == self.stats()


def test_mutation(doc_engine):
    """runs after test_single_doc_path on the same table"""
    eng, base = doc_engine
    nbytes = D1 // 8
    cent = eng.debug_binary_centroids(NLIST1)
    model = _Model(cent, *_lists(eng, NLIST1, nbytes))
    vec_of = {v: base[v] for v in range(N1)}   # docid -> stored bytes
    gone = np.zeros(N1 + 1000, dtype=bool)
    rng = np.random.default_rng(21)
    q = base[rng.integers(0, N1, size=16)].copy()
    q[:, 1] ^= 0x3C
    k, nprobe = 10, 6

    def check_search():
        _, pl = eng.debug_coarse_assign(q, nprobe)
        n_now = eng.num_docs()
        wd, wi = br.search(q, model.ids, model.codes, pl, k, gone[:n_now])
        gd, gi = eng.raw_search(q, k, nprobe=nprobe)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
        # term filter tag == grp1: the others join the bitmap. The tag of
        # a doc follows its key, and updates below keep key % 4.
        tags = np.array([int(eng_key[v]) % 4 for v in range(n_now)])
        fd, fi = br.search(q, model.ids, model.codes, pl, k,
                           gone[:n_now] | (tags != 1))
        res = eng.search_pb(q, topn=k, index_params='{"nprobe": %d}' % nprobe,
                            term_filters=[("tag", b"grp1")])
        pid, psc = _pb_rows(res)
        for t in range(len(q)):
            assert pid[t] == [eng_key[i] for i in fi[t] if i >= 0]
            assert psc[t] == [float(x) for x in fd[t] if x >= 0]

    eng_key = {v: v for v in range(N1)}        # docid -> key (as int)
    model.check(eng)
    check_search()

    # deletes: every 7th doc
    for vid in range(0, N1, 7):
        assert eng.delete_doc(str(vid)) == 0
        model.delete(vid)
        gone[vid] = True
    model.check(eng)
    check_search()
    assert model.dead() == len(range(0, N1, 7))

    # updates of existing keys: the old entry is marked, the new docid is
    # appended, and compact(0.3) runs after each update. One list takes
    # enough updates to cross 30 % dead.
    from vearch_amd import fbsenc
    big = int(np.argmax([len(i) for i in model.ids]))
    victims = [int(v) for v in model.ids[big] if v >= 0]
    victims = victims[:len(victims) * 2 // 5]
    compacted = 0
    for vid in victims:
        new_id = eng.num_docs()
        new_vec = vec_of[vid].copy()
        new_vec[-1] ^= 1                        # one bit away
        eng.add_doc(str(eng_key[vid]), new_vec,
                    fields=[("tag", _tag(eng_key[vid]),
                             fbsenc.DATA_STRING)])
        assert eng.num_docs() == new_id + 1
        model.delete(vid)
        gone[vid] = True
        model.append(new_id, new_vec)
        vec_of[new_id] = new_vec
        eng_key[new_id] = eng_key[vid]
        compacted += model.compact(0.3)["buckets"]
    assert compacted >= 1, "no update crossed the compaction threshold"
    model.check(eng)
    check_search()

    # explicit compact(0): every remaining dead entry goes
    want = model.compact(0.0)
    assert want["removed"] > 0
    assert eng.compact(0) == want
    assert model.dead() == 0
    model.check(eng)
    check_search()
    live = [v for v in range(eng.num_docs()) if not gone[v]]
    _check_lists(eng, NLIST1, lambda v: vec_of[v], live)


# 5 ---------------------------------------------------------------------
def test_persistence_and_rebuild():
    d, nlist, n = 256, 16, 3000
    base = gen_binary(n, d, seed=5)
    q = base[:16].copy()
    q[:, 3] ^= 0x81
    path = "/tmp/gamma_bin_dump"
    eng = make_engine(path)
    eng.create_table(d, "BINARYIVF", _params(nlist))
    eng.add(base)
    eng.build_index()
    for vid in range(0, n, 5):
        assert eng.delete_doc(str(vid)) == 0
    cent = eng.debug_binary_centroids(nlist)
    lists = _lists(eng, nlist, d // 8)
    want = [eng.raw_search(q, 10, nprobe=p) for p in (4, nlist)]
    want_b = eng.raw_search(q, 10, brute=1)
    eng.dump()
    eng.close()

    eng2 = make_engine(path)
    eng2.create_table(d, "BINARYIVF", _params(nlist))
    eng2.load()
    assert eng2.num_docs() == n
    assert np.array_equal(eng2.debug_binary_centroids(nlist), cent)
    for a, b in zip(lists, _lists(eng2, nlist, d // 8)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    for (wd, wi), p in zip(want, (4, nlist)):
        gd, gi = eng2.raw_search(q, 10, nprobe=p)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    bd, bi = eng2.raw_search(q, 10, brute=1)
    assert np.array_equal(bi, want_b[1]) and np.array_equal(bd, want_b[0])
    docs = eng2.query_pb(document_ids=["11"], is_vector_value=True)
    assert docs[0]["items"][0]["fields"][eng2.vec_name] == base[11].tobytes()
    assert eng2.compact_stats()["dead"] == len(range(0, n, 5))

    # RebuildIndex retrains from the raw store: the lists follow the new
    # centroids and the search follows the lists
    from vearch_amd.engine import lib
    lib().RebuildIndex.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int]
    assert lib().RebuildIndex(eng2.h, 1, 0, 0) == 0
    live = [v for v in range(n) if v % 5]
    deleted = np.zeros(n, dtype=bool)
    deleted[::5] = True
    # the rebuilt lists hold every raw vector; deleted docs stay out of
    # results through the bitmap
    cent2, ids2, codes2 = _check_lists(eng2, nlist, lambda v: base[v],
                                       range(n))
    _, pl = eng2.debug_coarse_assign(q, 4)
    assert np.array_equal(pl, br.coarse(q, cent2, 4)[1])
    wd, wi = br.search(q, ids2, codes2, pl, 10, deleted)
    gd, gi = eng2.raw_search(q, 10, nprobe=4)
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    assert set(gi.ravel().tolist()) <= set(live)
    eng2.close()


# 6 ---------------------------------------------------------------------
def test_rejections():
    eng = make_engine("/tmp/gamma_bin_reject")
    with pytest.raises(RuntimeError, match="multiple of 32"):
        eng.create_table(100, "BINARYIVF", _params(16))
    with pytest.raises(RuntimeError, match="4096"):
        eng.create_table(8192, "BINARYIVF", _params(16))
    with pytest.raises(RuntimeError, match="single"):
        eng.create_table(128, "BINARYIVF", _params(16),
                         extra_vecs=[("emb2", 128)])
    eng.create_table(128, "BINARYIVF", _params(16))
    eng.add_doc("0", np.zeros(16, dtype=np.uint8))
    # a float-sized vector (d * 4 bytes) on a binary table
    from vearch_amd import fbsenc
    buf = fbsenc.build_doc([
        ("_id", b"1", fbsenc.DATA_STRING),
        (eng.vec_name, np.zeros(128, dtype=np.float32).tobytes(),
         fbsenc.DATA_VECTOR)])
    from vearch_amd.engine import lib
    assert lib().AddOrUpdateDoc(eng.h, buf, len(buf)) != 0
    with pytest.raises(ValueError):
        eng.add(np.zeros((4, 128), dtype=np.float32))
    assert eng.num_docs() == 1
    eng.close()
