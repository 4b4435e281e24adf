"""GPU tests for IVF list compaction: the gk::bucket_compact kernel
through its test hook, and GammaEngine.compact / the automatic trigger
after an update.

Every expected list is a numpy boolean-mask compaction written here;
every comparison is np.array_equal (a compaction moves bytes, it does no
arithmetic, so there is nothing to tolerate).
"""
import os

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

MARK = np.int64(-2 ** 63)            # host-side bit-63 delete mark
MARK32 = np.uint32(0x80000000)       # device-side bit-31 delete mark

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
ENTRY_BYTES = [6, 16, 32, 48, 256]
PATTERNS = ["none", "all", "alternating", "first_half", "last_only",
            "random30", "bitmap_only", "mixed"]
ID_SPACE = 4096                      # ids are drawn below this


# ------------------------------------------------------------ kernel level
def _pattern(name, n, rng):
    """-> (marked bool[n], in_bitmap bool[n])"""
    mark = np.zeros(n, dtype=bool)
    bm = np.zeros(n, dtype=bool)
    if name == "all":
        mark[:] = True
    elif name == "alternating":
        mark[0::2] = True
    elif name == "first_half":
        mark[:n // 2] = True
    elif name == "last_only":
        mark[n - 1:] = True
    elif name == "random30":
        mark = rng.random(n) < 0.3
    elif name == "bitmap_only":
        bm = rng.random(n) < 0.3
    elif name == "mixed":
        mark = rng.random(n) < 0.25
        bm = rng.random(n) < 0.25   # overlaps some marks on purpose
    else:
        assert name == "none"
    return mark, bm


def _segment(n, entry_bytes, with_svals, pattern, rng):
    """-> (segment for ktest.bucket_compact, keep mask, bitmap ids)"""
    vids = rng.permutation(ID_SPACE)[:n].astype(np.uint32)
    mark, bm = _pattern(pattern, n, rng)
    ids = np.where(mark, vids | MARK32, vids).astype(np.uint32)
    data = rng.integers(0, 256, size=(n, entry_bytes), dtype=np.uint8)
    svals = (rng.standard_normal(n).astype(np.float32)
             if with_svals else None)
    return (ids, data, svals), ~mark & ~bm, vids[bm]


def _bitmap_words(bm_ids):
    words = np.zeros(ID_SPACE // 32, dtype=np.uint32)
    for v in bm_ids:
        words[int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    return words


def _check_segment(seg, keep, out):
    from vearch_amd import ktest
    ids, data, svals = seg
    o_ids, o_data, o_svals, kept = out
    want = int(keep.sum())
    assert kept == want
    assert np.array_equal(o_ids[:kept], ids[keep])
    assert np.array_equal(o_data[:kept], data[keep])
    # nothing at or beyond `kept` is written
    assert np.all(o_ids[kept:] == ktest.COMPACT_CANARY_ID)
    assert np.all(o_data[kept:] == ktest.COMPACT_CANARY_BYTE)
    if svals is not None:
        assert np.array_equal(o_svals[:kept], svals[keep])
        assert np.all(o_svals[kept:] == ktest.COMPACT_CANARY_SVAL)
    else:
        assert o_svals is None


@pytest.mark.parametrize("with_svals", [True, False])
@pytest.mark.parametrize("entry_bytes", ENTRY_BYTES)
def test_kernel_single_segment(entry_bytes, with_svals):
    """Every size x delete pattern, one segment per launch."""
    from vearch_amd import ktest
    rng = np.random.default_rng(1000 + entry_bytes + int(with_svals))
    for pattern in PATTERNS:
        for n in SIZES:
            seg, keep, bm_ids = _segment(n, entry_bytes, with_svals,
                                         pattern, rng)
            uses_bm = pattern in ("bitmap_only", "mixed")
            bitmap = (ktest.bitmap_to_dev(_bitmap_words(bm_ids))
                      if uses_bm else None)
            (out,) = ktest.bucket_compact([seg], entry_bytes, bitmap)
            _check_segment(seg, keep, out)


@pytest.mark.parametrize("with_svals", [True, False])
@pytest.mark.parametrize("entry_bytes", ENTRY_BYTES)
def test_kernel_multi_segment(entry_bytes, with_svals):
    """One launch over all sizes, patterns rotating, plus an empty and a
    fully dead segment; one shared bitmap, so every segment also sees the
    bits of the others' ids (ids are unique per segment only)."""
    from vearch_amd import ktest
    rng = np.random.default_rng(2000 + entry_bytes + int(with_svals))
    plan = [(n, PATTERNS[i % len(PATTERNS)]) for i, n in enumerate(SIZES)]
    plan += [(0, "mixed"), (300, "all"), (257, "mixed"), (1000, "mixed")]
    segs, bm_all = [], []
    for n, pattern in plan:
        seg, _, bm_ids = _segment(n, entry_bytes, with_svals, pattern, rng)
        segs.append(seg)
        bm_all.append(bm_ids)
    words = _bitmap_words(np.concatenate(bm_all))
    outs = ktest.bucket_compact(segs, entry_bytes,
                                ktest.bitmap_to_dev(words))
    assert len(outs) == len(segs)
    for seg, out in zip(segs, outs):
        ids = seg[0]
        vid = ids & ~MARK32
        in_bm = ((words[vid >> 5] >> (vid & 31)) & 1).astype(bool)
        keep = ((ids & MARK32) == 0) & ~in_bm
        _check_segment(seg, keep, out)


def test_kernel_rejects_bad_entry_size():
    from vearch_amd import ktest
    rng = np.random.default_rng(3)
    seg, _, _ = _segment(4, 0, False, "none", rng)
    with pytest.raises(ktest.KTestError):
        ktest.bucket_compact([seg], 0)


# ------------------------------------------------------------ engine level
D, N, NLIST, M = 64, 6000, 32, 16
K = 10


def make_engine(path, **kw):
    from vearch_amd import GammaEngine
    os.makedirs(str(path), exist_ok=True)
    return GammaEngine(path=str(path), **kw)


def _pq_params(nlist=NLIST, m=M, metric="L2", nbits=8, n=N):
    return ('{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": %d, '
            '"metric_type": "%s", "training_threshold": %d}'
            % (nlist, m, nbits, metric, n))


def _flat_params(nlist=NLIST, metric="L2", n=N):
    return ('{"ncentroids": %d, "metric_type": "%s", '
            '"training_threshold": %d}' % (nlist, metric, n))


@pytest.fixture(scope="module")
def data():
    base = orc.gen_clustered(N, D, seed=42, ncl=64)
    q = orc.gen_queries(base, 16, seed=1)
    return base, q


def _build(path, base, index_type, params):
    eng = make_engine(path)
    eng.create_table(base.shape[1], index_type, params)
    eng.add(base)
    eng.build_index()
    return eng


def _lists(eng, nlist, code_size):
    return [eng.debug_list(ln, code_size) for ln in range(nlist)]


def _marked(ids):
    return (ids & MARK) != 0


def _total_marks(lists):
    return int(sum(_marked(li).sum() for li, _ in lists))


def _searches(eng, q, nlist):
    return [eng.raw_search(q, K, nprobe=nlist, rerank=r) for r in (0, 50)]


def _assert_searches_equal(a, b):
    for (d0, i0), (d1, i1) in zip(a, b):
        assert np.array_equal(i0, i1)
        assert np.array_equal(d0, d1)


def _delete_scenario(eng, nlist, code_size):
    """Delete >= 40 % of three lists (three different shapes) and three
    entries (< 30 %) from three more. -> (chosen, lightly touched)"""
    lists = _lists(eng, nlist, code_size)
    big = [ln for ln in range(nlist) if len(lists[ln][0]) >= 40]
    assert len(big) >= 6, "table too small for the scenario"
    chosen, light = big[:3], big[3:6]
    for t, ln in enumerate(chosen):
        ids = lists[ln][0]
        n = len(ids)
        if t == 0:      # scattered: positions 0,2 of every 5
            victims = [ids[i] for i in range(n) if i % 5 in (0, 2)]
        elif t == 1:    # first half and the last entry
            victims = list(ids[:n // 2]) + [ids[n - 1]]
        else:           # the tail 45 %
            victims = list(ids[n - (45 * n + 99) // 100:])
        assert len(victims) >= 0.4 * n
        for v in victims:
            assert eng.delete_doc(str(int(v))) == 0
    for ln in light:
        ids = lists[ln][0]
        for v in (ids[0], ids[len(ids) // 2], ids[-1]):
            assert eng.delete_doc(str(int(v))) == 0
    return chosen, light


def _ratio_selected(lists, ratio=0.3):
    """Lists that compact(ratio) must pick, by the counter rule in fp32."""
    out = []
    for ln, (ids, _) in enumerate(lists):
        dead = int(_marked(ids).sum())
        if dead > 0 and (ratio <= 0 or np.float32(dead) / np.float32(
                len(ids)) >= np.float32(ratio)):
            out.append(ln)
    return out


def _compact_and_check(eng, q, nlist, code_size):
    """Scenario + compact(0.3) + every check of the explicit-compact test.
    -> (lists before, lists after, chosen lists)"""
    chosen, light = _delete_scenario(eng, nlist, code_size)
    before = _lists(eng, nlist, code_size)
    snap = _searches(eng, q, nlist)
    assert _ratio_selected(before) == chosen
    assert eng.compact_stats() == {
        "buckets": 0, "removed": 0, "dead": _total_marks(before)}

    st = eng.compact(0.3)

    after = _lists(eng, nlist, code_size)
    removed = 0
    for ln in range(nlist):
        b_ids, b_codes = before[ln]
        a_ids, a_codes = after[ln]
        if ln in chosen:
            keep = ~_marked(b_ids)
            removed += int((~keep).sum())
            assert np.array_equal(a_ids, b_ids[keep]), ln
            assert np.array_equal(a_codes, b_codes[keep]), ln
            assert not _marked(a_ids).any()
        else:
            assert np.array_equal(a_ids, b_ids), ln
            assert np.array_equal(a_codes, b_codes), ln
    for ln in light:
        assert int(_marked(after[ln][0]).sum()) == 3
    assert st == {"buckets": len(chosen), "removed": removed}
    assert eng.compact_stats() == {
        "buckets": len(chosen), "removed": removed,
        "dead": _total_marks(after)}
    _assert_searches_equal(snap, _searches(eng, q, nlist))
    return before, after, chosen


# 1 ---------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "InnerProduct"])
def test_explicit_compact_ivfpq8(data, metric):
    base, q = data
    eng = _build("/tmp/gamma_compact_pq8_" + metric, base, "IVFPQ",
                 _pq_params(metric=metric))
    _compact_and_check(eng, q, NLIST, M)
    # a second call finds nothing above the threshold
    assert eng.compact(0.3) == {"buckets": 0, "removed": 0}
    eng.close()


# 2 ---------------------------------------------------------------------
def test_mutation_after_compaction(data):
    """vid -> (bucket, pos) must follow the survivors: a delete after
    compaction has to mark exactly the moved entry."""
    base, q = data
    eng = _build("/tmp/gamma_compact_mut", base, "IVFPQ", _pq_params())
    before, after, chosen = _compact_and_check(eng, q, NLIST, M)
    ln = chosen[0]
    b_ids, a_ids = before[ln][0], after[ln][0]
    moved = [j for j in range(len(a_ids))
             if int(np.nonzero(b_ids == a_ids[j])[0][0]) != j]
    assert len(moved) >= 2
    j1, j2 = moved[len(moved) // 2], moved[-1]
    v1, v2 = int(a_ids[j1]), int(a_ids[j2])

    # delete a moved survivor
    _, gi = eng.raw_search(base[v1:v1 + 1], K, nprobe=NLIST, rerank=200)
    assert v1 in gi[0].tolist()
    assert eng.delete_doc(str(v1)) == 0
    _, gi = eng.raw_search(base[v1:v1 + 1], K, nprobe=NLIST, rerank=200)
    assert v1 not in gi[0].tolist()
    want = a_ids.copy()
    want[j1] |= MARK
    now_ids, now_codes = eng.debug_list(ln, M)
    assert np.array_equal(now_ids, want)
    assert np.array_equal(now_codes, after[ln][1])

    # update another moved survivor: old entry marked, new docid appended
    # to the same list (same vector -> same centroid) and found
    new_id = eng.num_docs()
    eng.add_doc(str(v2), base[v2])
    assert eng.num_docs() == new_id + 1
    want[j2] |= MARK
    now_ids, now_codes = eng.debug_list(ln, M)
    assert np.array_equal(now_ids, np.append(want, np.int64(new_id)))
    assert np.array_equal(now_codes[:-1], after[ln][1])
    assert np.array_equal(now_codes[-1], after[ln][1][j2])
    _, gi = eng.raw_search(base[v2:v2 + 1], K, nprobe=NLIST, rerank=200)
    assert new_id in gi[0].tolist() and v2 not in gi[0].tolist()

    # deleting an id that compaction already removed: as before (the key
    # is gone, -1) and nothing changes
    gone = int(b_ids[_marked(b_ids)][0] & ~MARK)
    lists0 = _lists(eng, NLIST, M)
    stats0 = eng.compact_stats()
    assert eng.delete_doc(str(gone)) == -1
    lists1 = _lists(eng, NLIST, M)
    for (i0, c0), (i1, c1) in zip(lists0, lists1):
        assert np.array_equal(i0, i1) and np.array_equal(c0, c1)
    assert eng.compact_stats() == stats0
    eng.close()


# 3 ---------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(16, 64), (12, 48)])
def test_explicit_compact_ivfpq4(m, d):
    """Packed 4-bit entries: 8 bytes at M=16, 6 bytes (not a multiple of
    4) at M=12. Bit-equal L2 distances after compaction prove the S terms
    moved with their entries."""
    base = orc.gen_clustered(N, d, seed=7, ncl=64)
    q = orc.gen_queries(base, 16, seed=2)
    eng = _build("/tmp/gamma_compact_pq4_%d" % m, base, "IVFPQ",
                 _pq_params(m=m, nbits=4))
    _compact_and_check(eng, q, NLIST, m // 2)
    eng.close()


# 4 ---------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "InnerProduct"])
def test_explicit_compact_ivfflat(data, metric):
    base, q = data
    eng = _build("/tmp/gamma_compact_flat_" + metric, base, "IVFFLAT",
                 _flat_params(metric=metric))
    _compact_and_check(eng, q, NLIST, D * 4)
    eng.close()


# 5 ---------------------------------------------------------------------
def test_automatic_trigger(data):
    base, q = data
    eng = _build("/tmp/gamma_compact_auto", base, "IVFPQ", _pq_params())
    lists = _lists(eng, NLIST, M)
    big = [ln for ln in range(NLIST) if len(lists[ln][0]) >= 40]
    la, lb = big[0], big[1]

    # list B only sees delete_doc calls, past 30 %: marks stay
    b_ids = lists[lb][0]
    nb_dead = (len(b_ids) * 2 + 4) // 5
    for v in b_ids[:nb_dead]:
        assert eng.delete_doc(str(int(v))) == 0
    assert np.float32(nb_dead) / np.float32(len(b_ids)) >= np.float32(0.3)
    now_b, _ = eng.debug_list(lb, M)
    assert len(now_b) == len(b_ids)
    assert int(_marked(now_b).sum()) == nb_dead
    assert eng.compact_stats() == {"buckets": 0, "removed": 0,
                                   "dead": nb_dead}

    # list A: update its own vectors in place (same vector -> same list)
    a_ids = lists[la][0]
    n = len(a_ids)
    u_star = next(u for u in range(1, n + 1)
                  if np.float32(u) / np.float32(n + u) >= np.float32(0.3))
    assert u_star < n
    for u in range(1, u_star + 1):
        eng.add_doc(str(int(a_ids[u - 1])), base[int(a_ids[u - 1])])
        now_a, _ = eng.debug_list(la, M)
        if u == 1:
            # the first update is "the next update" for list B
            now_b, _ = eng.debug_list(lb, M)
            assert np.array_equal(now_b, b_ids[nb_dead:])
            assert eng.compact_stats() == {"buckets": 1,
                                           "removed": nb_dead, "dead": 1}
        if u < u_star:
            assert len(now_a) == n + u
            assert int(_marked(now_a).sum()) == u
    # the update that crossed 30 % compacted list A
    assert len(now_a) == n
    assert not _marked(now_a).any()
    new_ids = np.arange(N, N + u_star, dtype=np.int64)
    assert np.array_equal(now_a, np.concatenate([a_ids[u_star:], new_ids]))
    assert eng.compact_stats() == {"buckets": 2,
                                   "removed": nb_dead + u_star, "dead": 0}
    _, gi = eng.raw_search(base[int(a_ids[0]):int(a_ids[0]) + 1], K,
                           nprobe=NLIST, rerank=200)
    assert N in gi[0].tolist() and int(a_ids[0]) not in gi[0].tolist()
    eng.close()


# 6 ---------------------------------------------------------------------
def test_dead_counter(data):
    base, q = data
    eng = _build("/tmp/gamma_compact_counter", base, "IVFPQ", _pq_params())
    rng = np.random.default_rng(5)
    victims = rng.permutation(N)[:300]
    for v in victims[:200]:
        assert eng.delete_doc(str(int(v))) == 0
    for v in victims[200:220]:          # updates: one new mark each
        eng.add_doc(str(int(v)), base[int(v)])
    lists = _lists(eng, NLIST, M)
    marks = _total_marks(lists)
    st = eng.compact_stats()
    assert marks > 0
    assert st["dead"] == marks
    # whatever the updates already compacted plus what is left is all of it
    assert st["removed"] + marks == 220
    touched = len(_ratio_selected(lists, 0))
    got = eng.compact(0)
    assert got == {"buckets": touched, "removed": marks}
    assert eng.compact_stats()["dead"] == 0
    assert _total_marks(_lists(eng, NLIST, M)) == 0
    assert eng.compact_stats()["removed"] == 220
    eng.close()


# 7 ---------------------------------------------------------------------
def _reload(path):
    eng = make_engine(path)
    eng.create_table(D, "IVFPQ", _pq_params())
    eng.load()
    return eng


def test_dump_load_after_compaction(data):
    base, q = data
    path = "/tmp/gamma_compact_dump"
    eng = _build(path, base, "IVFPQ", _pq_params())
    _, after, chosen = _compact_and_check(eng, q, NLIST, M)
    snap = _searches(eng, q, NLIST)
    eng.dump()
    eng.close()

    eng2 = _reload(path)
    loaded = _lists(eng2, NLIST, M)
    for (i0, c0), (i1, c1) in zip(after, loaded):
        assert np.array_equal(i0, i1) and np.array_equal(c0, c1)
    _assert_searches_equal(snap, _searches(eng2, q, NLIST))
    # the marks the dump still holds are counted again on load
    assert eng2.compact_stats()["dead"] == _total_marks(loaded)
    # delete in the loaded engine: the mark lands on the right entry
    ln = chosen[0]
    victim = int(loaded[ln][0][len(loaded[ln][0]) // 2])
    assert eng2.delete_doc(str(victim)) == 0
    want = loaded[ln][0].copy()
    want[len(want) // 2] |= MARK
    assert np.array_equal(eng2.debug_list(ln, M)[0], want)
    eng2.close()


def test_load_rebuilds_dead_counter(data):
    base, q = data
    path = "/tmp/gamma_compact_dump_marks"
    eng = _build(path, base, "IVFPQ", _pq_params())
    _delete_scenario(eng, NLIST, M)
    before = _lists(eng, NLIST, M)
    snap = _searches(eng, q, NLIST)
    marks = _total_marks(before)
    assert marks > 0
    eng.dump()
    eng.close()

    eng2 = _reload(path)
    assert eng2.compact_stats() == {"buckets": 0, "removed": 0,
                                    "dead": marks}
    st = eng2.compact(0)
    assert st == {"buckets": len(_ratio_selected(before, 0)),
                  "removed": marks}
    for ln, (ids, codes) in enumerate(_lists(eng2, NLIST, M)):
        keep = ~_marked(before[ln][0])
        assert np.array_equal(ids, before[ln][0][keep])
        assert np.array_equal(codes, before[ln][1][keep])
    _assert_searches_equal(snap, _searches(eng2, q, NLIST))
    eng2.close()


# 8 ---------------------------------------------------------------------
def test_append_after_compaction(data):
    base, q = data
    eng = _build("/tmp/gamma_compact_append", base, "IVFPQ", _pq_params())
    _, after, chosen = _compact_and_check(eng, q, NLIST, M)
    for t, ln in enumerate(chosen):
        ids, codes = after[ln]
        src = int(ids[len(ids) // 3])   # a survivor: same vector, same list
        new_id = eng.num_docs()
        eng.add_doc("fresh%d" % t, base[src])
        now_ids, now_codes = eng.debug_list(ln, M)
        assert np.array_equal(now_ids, np.append(ids, np.int64(new_id)))
        assert np.array_equal(now_codes[:-1], codes)
        assert np.array_equal(now_codes[-1], codes[len(ids) // 3])
        gd, gi = eng.raw_search(base[src:src + 1], K, nprobe=NLIST, rerank=200)
        row = gi[0].tolist()
        assert src in row and new_id in row
        assert gd[0][row.index(src)] == gd[0][row.index(new_id)]
    eng.close()


# 9 ---------------------------------------------------------------------
def test_multi_vector_table(data):
    """Both fields carry the same vectors, so the extra field's lists
    mirror the primary's: every count doubles when it is compacted too."""
    base, q = data
    n, nlist, nq, topn = 4000, 16, 4, 10
    eng = make_engine("/tmp/gamma_compact_multivec")
    eng.create_table(D, "IVFPQ", _pq_params(nlist=nlist, n=n),
                     extra_vecs=[("emb2", D)])
    for vid in range(n):
        eng.add_doc(str(vid), base[vid], extra_vecs=[("emb2", base[vid])])
    eng.build_index()
    chosen, _ = _delete_scenario(eng, nlist, M)
    before = _lists(eng, nlist, M)
    marks = _total_marks(before)
    removed = sum(int(_marked(before[ln][0]).sum()) for ln in chosen)
    assert eng.compact_stats()["dead"] == 2 * marks

    def merged():
        return eng.search_pb(q[:nq], topn=topn,
                             index_params='{"recall_num": 50}',
                             extra_vec_queries=[("emb2", q[:nq])],
                             multi_vector_rank=1)

    def flat(res):
        return [[(it["fields"]["_id"], it["score"]) for it in r["items"]]
                for r in res]

    snap = flat(merged())
    assert all(snap), "merged search returned nothing (vacuous)"
    st = eng.compact(0.3)
    assert st == {"buckets": 2 * len(chosen), "removed": 2 * removed}
    assert eng.compact_stats()["dead"] == 2 * (marks - removed)
    for ln in chosen:
        keep = ~_marked(before[ln][0])
        ids, codes = eng.debug_list(ln, M)
        assert np.array_equal(ids, before[ln][0][keep])
        assert np.array_equal(codes, before[ln][1][keep])
    assert flat(merged()) == snap
    eng.close()


# 10 --------------------------------------------------------------------
def _oracle_from_engine(eng, d, nlist, m, metric="L2"):
    ox = orc.OracleIVFPQ(d, nlist, m, metric=metric)
    cent, books = eng.debug_model(nlist, d, m)
    ox.centroids, ox.codebooks = cent, books
    ids_all, codes_all, offsets = [], [], [0]
    for ln in range(nlist):
        li, lc = eng.debug_list(ln, m)
        ids_all.append(li)
        codes_all.append(lc)
        offsets.append(offsets[-1] + len(li))
    ox.ids = np.concatenate(ids_all)
    ox.codes = np.concatenate(codes_all)
    ox.offsets = np.array(offsets, dtype=np.int64)
    return ox


def test_oracle_parity_after_compaction(data):
    """The CPU oracle rebuilt from the engine's model and its compacted
    lists gives the same ids and the same fp32 distances, after the
    threshold pass (some marks left) and after compact(0) (none left)."""
    base, q = data
    eng = _build("/tmp/gamma_compact_oracle", base, "IVFPQ", _pq_params())
    _compact_and_check(eng, q, NLIST, M)
    nprobe = 8
    pdists, probes = eng.debug_coarse_assign(q, nprobe)
    for ratio in (None, 0):
        if ratio is not None:
            eng.compact(ratio)
            assert _total_marks(_lists(eng, NLIST, M)) == 0
        ox = _oracle_from_engine(eng, D, NLIST, M)
        gd, gi = eng.raw_search(q, K, nprobe=nprobe)
        od, oi = ox.search_pct1(q, K, nprobe, probes=probes,
                                probe_dists=pdists)
        assert np.array_equal(gi, oi)
        assert np.array_equal(gd, od)
    eng.close()
