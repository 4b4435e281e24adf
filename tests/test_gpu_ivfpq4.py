"""GPU parity tests for 4-bit IVFPQ (nbits_per_idx=4, ksub=16).

Codes are packed two per byte: byte b of an entry holds sub-quantizer 2b
in bits 0-3 and 2b+1 in bits 4-7. The CPU oracle already takes ksub, so
every search comparison here is np.array_equal on ids AND fp32 distances
against the oracle run on the engine's own model, lists and probes: the
arithmetic order is pinned (dis0 + S_v, then += T[m][code_m] in ascending
m), so no tolerance is needed.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle as orc
from oracle.gamma_oracle import RefLib, _c, _fp, _up8

pytestmark = pytest.mark.gpu


def make_engine(tmp, **kw):
    from vearch_amd import GammaEngine
    return GammaEngine(path=str(tmp), **kw)


def _params(nlist=64, M=16, metric="L2", tt=8000, extra=""):
    return ('{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": 4, '
            '"metric_type": "%s", "training_threshold": %d%s}'
            % (nlist, M, metric, tt, extra))


def _build(path, base, d=64, **kw):
    eng = make_engine(path)
    eng.create_table(d, "IVFPQ", _params(**kw))
    eng.add(base)
    eng.build_index()
    return eng


def _unpack(packed):
    """(n, M/2) packed bytes -> (n, M) one code per byte; the low nibble
    is the even sub-quantizer."""
    out = np.empty((packed.shape[0], packed.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


def _oracle4_from_engine(eng, d, nlist, M, metric="L2"):
    ox = orc.OracleIVFPQ(d, nlist, M, metric=metric)
    ox.ksub = 16
    cent, books = eng.debug_model(nlist, d, M, ksub=16)
    ox.centroids, ox.codebooks = cent, books
    ids_all, codes_all, offsets = [], [], [0]
    for ln in range(nlist):
        li, lc = eng.debug_list(ln, M // 2)
        assert lc.shape == (len(li), M // 2)
        ids_all.append(li)
        codes_all.append(_unpack(lc))
        offsets.append(offsets[-1] + len(li))
    ox.ids = np.concatenate(ids_all)
    ox.codes = np.concatenate(codes_all)
    ox.offsets = np.array(offsets, dtype=np.int64)
    return ox


@pytest.fixture(scope="module")
def data():
    base = orc.gen_clustered(20000, 64, seed=42, ncl=200)
    q = orc.gen_queries(base, 64, seed=1)
    return base, q


@pytest.fixture(scope="module")
def eng4(data):
    base, _ = data
    eng = _build("/tmp/gamma_ivfpq4_mod", base)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ox4(eng4):
    """Oracle on the shared engine's model + lists; read-only."""
    return _oracle4_from_engine(eng4, 64, 64, 16)


def _check_l2(eng, ox, q, k, nprobe, del_bitmap=None):
    gd, gi = eng.raw_search(q, k, nprobe=nprobe)
    pdists, probes = eng.debug_coarse_assign(q, nprobe)
    od, oi = ox.search_pct1(q, k, nprobe, probes=probes, probe_dists=pdists,
                            del_bitmap=del_bitmap)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)
    return gd, gi


# 1 ---------------------------------------------------------------------
def test_l2_adc_bitexact(data, eng4, ox4):
    """64 queries take the probe-split path (S=8), 2048 queries S=1."""
    _, q = data
    _check_l2(eng4, ox4, q, 10, 16)
    _check_l2(eng4, ox4, np.repeat(q, 32, axis=0), 10, 16)


# 2 ---------------------------------------------------------------------
def test_layout_and_encode(data, eng4):
    """Pins the nibble order independently of the scan: re-encode every
    list on the CPU (same fmaf loop, ties -> lowest index) and compare
    with the unpacked engine codes."""
    base, _ = data
    d, nlist, M = 64, 64, 16
    cent, books = eng4.debug_model(nlist, d, M, ksub=16)
    assert books.shape == (M, 16, d // M)
    lib = RefLib.lib()
    total = 0
    for ln in range(nlist):
        li, lc = eng4.debug_list(ln, M // 2)
        assert lc.shape == (len(li), M // 2)
        total += len(li)
        if len(li) == 0:
            continue
        got = _unpack(lc)
        assert got.max() < 16
        resid = _c(base[li] - cent[ln], np.float32)
        want = np.empty((len(li), M), dtype=np.uint8)
        lib.oracle_pq_encode(len(li), d, M, 16, _fp(resid),
                             _fp(_c(books, np.float32)), _up8(want))
        assert np.array_equal(got, want), ln
    assert total == 20000


# 3 ---------------------------------------------------------------------
def test_ip_bitexact(data):
    base, q = data
    eng = _build("/tmp/gamma_ivfpq4_ip", base, metric="InnerProduct")
    gd, gi = eng.raw_search(q, 10, nprobe=16)
    ox = _oracle4_from_engine(eng, 64, 64, 16, metric="InnerProduct")
    _, probes = eng.debug_coarse_assign(q, 16)
    od, oi = ox.search(q, 10, 16, probes=probes)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)
    for t in range(q.shape[0]):  # IP similarity is descending
        row = [gd[t, j] for j in range(10) if gi[t, j] >= 0]
        assert row == sorted(row, reverse=True)
    eng.close()


# 4 ---------------------------------------------------------------------
def test_generic_path_unaligned_entries():
    """M=12: 6-byte entries, not word-aligned -> generic (byte-load)
    scan path."""
    base = orc.gen_clustered(6000, 48, seed=42, ncl=200)
    q = orc.gen_queries(base, 64, seed=1)
    eng = _build("/tmp/gamma_ivfpq4_m12", base, d=48, nlist=16, M=12,
                 tt=3000)
    ox = _oracle4_from_engine(eng, 48, 16, 12)
    _check_l2(eng, ox, q, 10, 8)
    eng.close()


# 5 ---------------------------------------------------------------------
def test_fast_path_m32(data):
    """M=32: four code words per entry."""
    base, q = data
    eng = _build("/tmp/gamma_ivfpq4_m32", base, M=32)
    ox = _oracle4_from_engine(eng, 64, 64, 32)
    _check_l2(eng, ox, q, 10, 16)
    eng.close()


# 6 ---------------------------------------------------------------------
def test_deletes_and_bitmap(data):
    base, q = data
    n = base.shape[0]
    eng = _build("/tmp/gamma_ivfpq4_del", base)
    for vid in range(0, n, 7):
        eng.delete_doc(str(vid))
    bm = np.zeros((n + 7) // 8, dtype=np.uint8)
    for vid in range(0, n, 7):
        bm[vid >> 3] |= 1 << (vid & 7)
    ox = _oracle4_from_engine(eng, 64, 64, 16)
    _, gi = _check_l2(eng, ox, q, 10, 16, del_bitmap=bm)
    assert not any(v % 7 == 0 for v in gi.ravel().tolist() if v >= 0)
    # re-add one deleted vector through the single-doc path (encode, pack,
    # S term): a brute-nprobe search finds it under its new docid. Its own
    # code minimises the ADC distance within its list, but vectors with
    # the same code tie and the new (largest) docid sorts last among
    # them, hence k=100. The oracle rebuilt from the lists then pins the
    # new entry's code and S term bit-exactly.
    victim = 7 * 100
    eng.add_doc(str(victim), base[victim])
    new_id = eng.num_docs() - 1
    assert new_id == n
    ox2 = _oracle4_from_engine(eng, 64, 64, 16)
    assert len(ox2.ids) == n + 1
    bm2 = np.zeros((n + 8) // 8, dtype=np.uint8)
    bm2[:len(bm)] = bm
    _, gi2 = _check_l2(eng, ox2, base[victim:victim + 1], 100, 64,
                       del_bitmap=bm2)
    assert new_id in gi2[0].tolist()
    assert victim not in gi2[0].tolist()
    eng.close()


# 7 ---------------------------------------------------------------------
def test_rerank_and_recall_floors(data, eng4):
    """Exact rerank distances, and the reference's own recall gates
    (test_vector_index_ivfpq.py:106-111): R@1 >= 0.6, R@10 >= 0.9."""
    base, q = data
    gd, gi = eng4.raw_search(q, 10, nprobe=16, rerank=100)
    lib = RefLib.lib()
    lib.oracle_l2sqr.restype = ctypes.c_float
    for t in range(q.shape[0]):
        for j in range(10):
            if gi[t, j] < 0:
                continue
            want = lib.oracle_l2sqr(_fp(_c(q[t], np.float32)),
                                    _fp(_c(base[gi[t, j]], np.float32)), 64)
            assert gd[t, j] == want, (t, j)
        row = [(gd[t, j], gi[t, j]) for j in range(10) if gi[t, j] >= 0]
        assert row == sorted(row)
    _, gti = orc.flat_topk_f64(base, q, 100)
    r1 = orc.recall_at(gti, gi[:, :1], 1)
    r10 = orc.recall_at(gti, gi, 10)
    print(f"4-bit M=16 rerank=100: recall@1={r1} recall@10={r10}")
    assert r1 >= 0.6, f"recall@1={r1}"
    assert r10 >= 0.9, f"recall@10={r10}"


# 8 ---------------------------------------------------------------------
def test_dump_load_roundtrip(data):
    """S terms are not dumped: load rebuilds them from the packed codes."""
    base, q = data
    path = "/tmp/gamma_ivfpq4_dumpload"
    os.makedirs(path, exist_ok=True)
    eng = _build(path, base[:8000], nlist=32, tt=4000)
    gd0, gi0 = eng.raw_search(q, 10, nprobe=32)
    eng.dump()
    eng.close()
    eng2 = make_engine(path)
    eng2.create_table(64, "IVFPQ", _params(nlist=32, tt=4000))
    eng2.load()
    assert eng2.num_docs() == 8000
    gd1, gi1 = eng2.raw_search(q, 10, nprobe=32)
    assert np.array_equal(gi0, gi1)
    assert np.array_equal(gd0, gd1)
    eng2.close()


# 9 ---------------------------------------------------------------------
def test_launch_knobs_bitexact(data, eng4):
    """The 4-bit launch reads GAMMA_ADC_C, GAMMA_SCAN_BS and (through the
    probe split) GAMMA_SCAN_S; none may change results."""
    _, q = data
    qq = np.repeat(q, 32, axis=0)
    ref_d, ref_i = eng4.raw_search(qq, 10, nprobe=16, rerank=64)
    knobs = [
        {"GAMMA_ADC_C": "2"},
        {"GAMMA_SCAN_BS": "256"},
        {"GAMMA_SCAN_S": "2"},
        {"GAMMA_ADC_C": "2", "GAMMA_SCAN_BS": "256", "GAMMA_SCAN_S": "2"},
    ]
    for kv in knobs:
        for k, v in kv.items():
            os.environ[k] = v
        try:
            gd, gi = eng4.raw_search(qq, 10, nprobe=16, rerank=64)
        finally:
            for k in kv:
                del os.environ[k]
        assert np.array_equal(gi, ref_i), kv
        assert np.array_equal(gd, ref_d), kv


# 10 --------------------------------------------------------------------
@pytest.mark.parametrize("params", [
    '{"ncentroids": 64, "nsubvector": 16, "nbits_per_idx": 5}',
    '{"ncentroids": 64, "nsubvector": 16, "nbits_per_idx": 16}',
    '{"ncentroids": 64, "nsubvector": 16, "nbits_per_idx": 4, '
    '"opq": {"nsubvector": 16}}',
])
def test_rejections(tmp_path, params):
    eng = make_engine(tmp_path)
    with pytest.raises(RuntimeError) as ei:
        eng.create_table(64, "IVFPQ", params)
    # "CreateTable failed (code N): <engine message>"
    assert str(ei.value).split("): ", 1)[1].strip()
    eng.close()


def test_bulk_add_after_train_and_rebuild(data):
    """Bulk add into a trained 4-bit index (packed encode + S terms on
    the ingest path), then RebuildIndex(drop=1): both states stay
    bit-exact against the oracle rebuilt from the engine's lists."""
    from vearch_amd.engine import lib
    base, q = data
    eng = _build("/tmp/gamma_ivfpq4_rebuild", base[:9000], nlist=32,
                 tt=4000)
    eng.add(base[9000:12000])
    ox = _oracle4_from_engine(eng, 64, 32, 16)
    assert len(ox.ids) == 12000
    _check_l2(eng, ox, q, 10, 32)
    lib().RebuildIndex.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int]
    assert lib().RebuildIndex(eng.h, 1, 0, 0) == 0
    ox = _oracle4_from_engine(eng, 64, 32, 16)
    assert len(ox.ids) == 12000
    _check_l2(eng, ox, q, 10, 32)
    eng.close()


# 11 --------------------------------------------------------------------
def test_search_pb_end_to_end(data, eng4):
    _, q = data
    res = eng4.search_pb(q[:8], topn=10,
                         index_params='{"nprobe": 16, "recall_num": 50}')
    _, gi = eng4.raw_search(q[:8], 10, nprobe=16, rerank=50)
    assert len(res) == 8
    for t in range(8):
        ids = [int(it["fields"]["_id"]) for it in res[t]["items"]]
        assert ids == [i for i in gi[t].tolist() if i >= 0]
