"""Engine-level tests for 8-bit IVFPQ tables too wide for the
resident-table scan (nsubvector >= 144), in the pattern of
test_gpu_ivfpq4.py.

Every raw-search comparison is np.array_equal on ids AND fp32 distances
against the CPU oracle run on the engine's own model, lists and probes:
the arithmetic order is pinned (dis0 + S_v, then += T[m][code_m] in
ascending m), so no tolerance is needed.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

D, M, NLIST, N = 288, 144, 16, 6000


def make_engine(tmp, **kw):
    from vearch_amd import GammaEngine
    return GammaEngine(path=str(tmp), **kw)


def _params(nlist=NLIST, M=M, metric="L2", tt=N, extra=""):
    m = '"nsubvector": %d, ' % M if M else ""
    return ('{"ncentroids": %d, %s"metric_type": "%s", '
            '"training_threshold": %d%s}' % (nlist, m, metric, tt, extra))


def _build(path, base, d=D, **kw):
    os.makedirs(str(path), exist_ok=True)
    eng = make_engine(path)
    eng.create_table(d, "IVFPQ", _params(**kw))
    eng.add(base)
    eng.build_index()
    return eng


def _oracle_from_engine(eng, d=D, nlist=NLIST, M=M, metric="L2"):
    ox = orc.OracleIVFPQ(d, nlist, M, metric=metric)
    cent, books = eng.debug_model(nlist, d, M)
    assert books.shape == (M, 256, d // M)
    ox.centroids, ox.codebooks = cent, books
    ids_all, codes_all, offsets = [], [], [0]
    for ln in range(nlist):
        li, lc = eng.debug_list(ln, M)
        assert lc.shape == (len(li), M)
        ids_all.append(li)
        codes_all.append(lc)
        offsets.append(offsets[-1] + len(li))
    ox.ids = np.concatenate(ids_all)
    ox.codes = np.concatenate(codes_all)
    ox.offsets = np.array(offsets, dtype=np.int64)
    return ox


def _check_l2(eng, ox, q, k, nprobe, del_bitmap=None, q_oracle=None):
    gd, gi = eng.raw_search(q, k, nprobe=nprobe)
    qo = q if q_oracle is None else q_oracle
    pdists, probes = eng.debug_coarse_assign(qo, nprobe)
    od, oi = ox.search_pct1(qo, k, nprobe, probes=probes,
                            probe_dists=pdists, del_bitmap=del_bitmap)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)
    return gd, gi


@pytest.fixture(scope="module")
def data():
    base = orc.gen_clustered(N, D, seed=42, ncl=60)
    q = orc.gen_queries(base, 64, seed=1)
    return base, q


@pytest.fixture(scope="module")
def engw(data):
    base, _ = data
    eng = _build("/tmp/gamma_wide_mod", base)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oxw(engw):
    """Oracle on the shared engine's model + lists; read-only."""
    return _oracle_from_engine(engw)


# 1 ---------------------------------------------------------------------
def test_l2_adc_bitexact(data, engw, oxw):
    """64 queries take the probe-split path (S > 1), 2048 queries S = 1."""
    _, q = data
    _check_l2(engw, oxw, q, 10, 8)
    _check_l2(engw, oxw, np.repeat(q, 32, axis=0), 10, 8)


# 2 ---------------------------------------------------------------------
def test_ip_bitexact(data):
    """OracleIVFPQ.search is the oracle's inner-product entry point
    (search_pct1 is the L2 decomposition and refuses the metric), as in
    test_gpu_ivfpq4.py."""
    base, q = data
    eng = _build("/tmp/gamma_wide_ip", base, metric="InnerProduct")
    ox = _oracle_from_engine(eng, metric="InnerProduct")
    for qq in (q, np.repeat(q, 32, axis=0)):
        gd, gi = eng.raw_search(qq, 10, nprobe=8)
        _, probes = eng.debug_coarse_assign(qq, 8)
        od, oi = ox.search(qq, 10, 8, probes=probes)
        assert np.array_equal(gi, oi)
        assert np.array_equal(gd, od)
    for t in range(q.shape[0]):  # IP similarity is descending
        row = [gd[t, j] for j in range(10) if gi[t, j] >= 0]
        assert row == sorted(row, reverse=True)
    eng.close()


# 3 ---------------------------------------------------------------------
def test_rerank_recall(data, engw):
    """recall_num = 200 re-ranked exactly: recall@10 against fp64 brute
    force meets the project's 0.95 gate."""
    base, q = data
    _, gi = engw.raw_search(q, 10, nprobe=NLIST, rerank=200)
    _, gti = orc.flat_topk_f64(base, q, 10)
    r10 = orc.recall_at(gti, gi, 10)
    print(f"M={M} rerank=200: recall@10={r10}")
    assert r10 >= 0.95, f"recall@10={r10}"


# 4 ---------------------------------------------------------------------
def test_search_pb_end_to_end(data, engw):
    _, q = data
    res = engw.search_pb(q[:8], topn=10,
                         index_params='{"nprobe": 8, "recall_num": 50}')
    _, gi = engw.raw_search(q[:8], 10, nprobe=8, rerank=50)
    assert len(res) == 8
    for t in range(8):
        ids = [int(it["fields"]["_id"]) for it in res[t]["items"]]
        assert ids == [i for i in gi[t].tolist() if i >= 0]


# 5 ---------------------------------------------------------------------
def test_mutation_and_persistence(data):
    """Deleted-docs bitmap, single-document add, an update that triggers
    compaction, Dump -> Load, Rebuild: bit-exact against the oracle
    rebuilt from the engine's lists at every step."""
    from vearch_amd.engine import lib
    base, q = data
    path = "/tmp/gamma_wide_mut"
    eng = _build(path, base)
    # deletes: the bitmap filters, marks stay in the lists
    for vid in range(0, N, 7):
        assert eng.delete_doc(str(vid)) == 0
    bm = np.zeros((N + 64) // 8, dtype=np.uint8)
    for vid in range(0, N, 7):
        bm[vid >> 3] |= 1 << (vid & 7)
    ox = _oracle_from_engine(eng)
    _, gi = _check_l2(eng, ox, q, 10, 8, del_bitmap=bm)
    assert not any(v % 7 == 0 for v in gi.ravel().tolist() if v >= 0)

    # a single-document add after training (144-byte entry, S term) is
    # found by the next search under its new docid
    victim = 7 * 100
    eng.add_doc(str(victim), base[victim])
    new_id = eng.num_docs() - 1
    assert new_id == N
    ox = _oracle_from_engine(eng)
    assert len(ox.ids) == N + 1
    _, gi2 = _check_l2(eng, ox, base[victim:victim + 1], 100, NLIST,
                       del_bitmap=bm)
    assert new_id in gi2[0].tolist() and victim not in gi2[0].tolist()

    # updates of one list's own vectors (same vector -> same list) until
    # its dead share crosses 30 %: that update compacts
    st0 = eng.compact_stats()
    lists = [eng.debug_list(ln, M)[0] for ln in range(NLIST)]
    sizes = [len(x) for x in lists]
    la = min((ln for ln in range(NLIST) if sizes[ln] >= 20),
             key=lambda ln: sizes[ln])
    live = [int(v) for v in lists[la] if v >= 0]
    for u, v in enumerate(live):
        eng.add_doc(str(v), base[v] if v < N else base[victim])
        if eng.compact_stats()["buckets"] > st0["buckets"]:
            break
    st = eng.compact_stats()
    assert st["buckets"] > st0["buckets"] and st["removed"] > st0["removed"]
    now, _ = eng.debug_list(la, M)
    assert (now >= 0).all()  # no marks left in the compacted list
    nd = eng.num_docs()
    bm3 = np.zeros((nd + 64) // 8, dtype=np.uint8)
    bm3[:len(bm)] = bm
    for v in live[:u + 1]:
        bm3[v >> 3] |= 1 << (v & 7)
    ox = _oracle_from_engine(eng)
    gd0, gi0 = _check_l2(eng, ox, q, 10, 8, del_bitmap=bm3)

    # Dump -> Load: S terms are rebuilt from the codes; same keys
    eng.dump()
    eng.close()
    eng2 = make_engine(path)
    eng2.create_table(D, "IVFPQ", _params())
    eng2.load()
    assert eng2.num_docs() == nd
    gd1, gi1 = eng2.raw_search(q, 10, nprobe=8)
    assert np.array_equal(gi0, gi1)
    assert np.array_equal(gd0, gd1)

    # Rebuild (drop and retrain)
    lib().RebuildIndex.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int]
    assert lib().RebuildIndex(eng2.h, 1, 0, 0) == 0
    ox = _oracle_from_engine(eng2)
    _check_l2(eng2, ox, q, 10, 8, del_bitmap=bm3)
    eng2.close()


# 6 ---------------------------------------------------------------------
def test_default_nsubvector_d512():
    """No nsubvector: M = d/2 = 256, the default that could not be
    searched."""
    d, n, nlist = 512, 3000, 8
    base = orc.gen_clustered(n, d, seed=3, ncl=40)
    q = orc.gen_queries(base, 16, seed=2)
    eng = _build("/tmp/gamma_wide_d512", base, d=d, nlist=nlist, M=0, tt=n)
    ox = _oracle_from_engine(eng, d=d, nlist=nlist, M=256)
    gd, gi = _check_l2(eng, ox, q, 10, 4)
    assert (gi[:, 0] >= 0).all()
    # 2304 queries x 256 KB of query table exceed the engine's 512 MiB
    # table scratch: table build and scan run in two query groups, and
    # every row is what it was
    gd2, gi2 = _check_l2(eng, ox, np.repeat(q, 144, axis=0), 10, 4)
    assert np.array_equal(gi2[::144], gi) and np.array_equal(gd2[::144], gd)
    assert np.array_equal(gi2[143::144], gi)
    eng.close()


# 6b --------------------------------------------------------------------
def test_single_add_entry_above_256_bytes():
    """d = 576, M = 288: a 288-byte entry does not fit the single-document
    append's small staging buffer. The document added after training is
    found by the next search, with its code and S term as the oracle
    rebuilt from the lists computes them."""
    d, n, nlist, m = 576, 3000, 8, 288
    base = orc.gen_clustered(n, d, seed=6, ncl=40)
    eng = _build("/tmp/gamma_wide_add288", base, d=d, nlist=nlist, M=m, tt=n)
    extra = orc.gen_queries(base, 1, seed=9)[0]
    eng.add_doc("fresh", extra)
    assert eng.num_docs() == n + 1
    ox = _oracle_from_engine(eng, d=d, nlist=nlist, M=m)
    assert len(ox.ids) == n + 1
    _, gi = _check_l2(eng, ox, extra[None, :], 100, nlist)
    assert n in gi[0].tolist()
    eng.close()


# 7 ---------------------------------------------------------------------
def test_opq_wide():
    """OPQ with M = 144: coarse assign and ADC run in rotated space, so
    the oracle gets the engine's own rotated queries."""
    d, n, nlist = 144, 3000, 8
    base = orc.gen_clustered(n, d, seed=5, ncl=40)
    q = orc.gen_queries(base, 16, seed=4)
    eng = _build("/tmp/gamma_wide_opq", base, d=d, nlist=nlist, tt=n,
                 extra=', "opq": {"nsubvector": 144}')
    R = eng.debug_opq(d)
    assert np.allclose(R @ R.T, np.eye(d), atol=2e-3)
    ox = _oracle_from_engine(eng, d=d, nlist=nlist)
    _check_l2(eng, ox, q, 10, 4, q_oracle=eng.debug_apply_opq(q))
    eng.close()


# 8 ---------------------------------------------------------------------
def test_create_table_names_the_bound(tmp_path):
    """What the scan cannot serve is refused at CreateTable, by name."""
    eng = make_engine(tmp_path)
    with pytest.raises(RuntimeError) as ei:
        eng.create_table(32768, "IVFPQ", _params(M=64))
    assert "16384" in str(ei.value)
    eng.close()
