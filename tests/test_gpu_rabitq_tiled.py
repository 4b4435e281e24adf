"""The tiled entry movement of k_rabitq_scan (nb_bits 4 and 8, entries
moved through a per-wave LDS tile in slabs of 8 eight-byte units): dispatch,
the scan against the fp64 numpy reference, bit-identity with the streamed
and the register-resident movements, and the engine. Cases, references and
bounds are those of test_gpu_rabitq_ex.py."""
import numpy as np
import pytest

import rabitq_ref as rr
from oracle import kernel_refs as kr
from test_gpu_rabitq import (NQ_SCAN, _cands, _scan_case, gen_clustered,
                             gen_queries, make_engine)
from test_gpu_rabitq_ex import SIZES, _check_rows, _encoded_lists, _params

pytestmark = pytest.mark.gpu

KNOB = "GAMMA_RBQ_TILED"


@pytest.mark.parametrize("knob,B,D,want", [
    (None, 4, 96, True), (None, 4, 768, True), (None, 8, 256, True),
    (None, 8, 1024, True), (None, 4, 128, False), (None, 8, 64, False),
    (None, 1, 96, False), ("1", 4, 128, True), ("1", 1, 96, False),
    ("0", 4, 96, False)])
def test_dispatch(knob, B, D, want, monkeypatch):
    from vearch_amd import ktest
    monkeypatch.delenv(KNOB, raising=False)
    if knob is not None:
        monkeypatch.setenv(KNOB, knob)
    assert ktest.rabitq_scan_is_tiled(B, D) is want


def _case(B, D):
    """test_kernel_scan's Gaussian case: lists, marks and a bitmap at ~30 %"""
    id_space = sum(SIZES) + 64
    case = _scan_case(D, 1000 * B + D, False, SIZES, id_space)
    rng = np.random.default_rng(D)
    marks = [rng.random(n) < 0.3 for n in SIZES]
    return case, marks, rng.random(id_space) < 0.3


@pytest.mark.parametrize("B,D", [(4, 32), (4, 96), (8, 96), (4, 288),
                                 (8, 288), (8, 544)])
def test_scan_against_reference(B, D, monkeypatch):
    """Entries of 3, 7 and 13 units (less than a slab, one partial slab, one
    slab and a partial one), 37 units (4 slabs + 5), 73 and 137 units (9 and
    17 slabs, then the factor unit alone). No legal d gives an entry of
    exactly one slab: an entry is an odd number of units."""
    from vearch_amd import ktest
    monkeypatch.setenv(KNOB, "1")
    assert ktest.rabitq_scan_is_tiled(B, D)
    (cent, ids, vecs, queries, probes), marks, bm = _case(B, D)
    for ip in (False, True):
        dev, tab = _encoded_lists(B, D, cent, ids, vecs, queries, marks,
                                  False, ip)
        for bs in (512, 256):
            monkeypatch.setenv("GAMMA_SCAN_BS", str(bs))
            for S, k2 in ((1, 1), (3, 10), (1, 200)):
                keys, od, oi = ktest.rabitq_scan(
                    dev, probes, queries, cent, S, k2, ip,
                    bitmap=kr.bitmap_words(bm), kill_flag=True, nb_bits=B)
                assert keys.shape == (NQ_SCAN, S, k2)
                _check_rows(keys, od, oi, tab, ids, marks, bm, probes, S, ip)


def test_scan_deep_selector():
    """d = 96 at 4 bits, k2 = 1500 of ~2400 live candidates: the tiled
    movement under GammaDeepSelector, the regions merged by select_deep."""
    from vearch_amd import ktest
    B, D, S, k2 = 4, 96, 2, 1500
    assert ktest.rabitq_scan_is_tiled(B, D)
    (cent, ids, vecs, queries, probes), marks, bm = _case(B, D)
    for ip in (False, True):
        dev, tab = _encoded_lists(B, D, cent, ids, vecs, queries, marks,
                                  False, ip)
        keys, _, _ = ktest.rabitq_scan(dev, probes, queries, cent, S, k2, ip,
                                       bitmap=kr.bitmap_words(bm),
                                       nb_bits=B)
        merged = ktest.select_deep(keys, k2)
        for r in range(NQ_SCAN):
            rr.check_row(*kr.key_decode(merged[r], ip),
                         *_cands(tab, ids, marks, bm, probes[r].tolist(), r),
                         ip)


@pytest.mark.parametrize("B,D", [(4, 128), (4, 256), (8, 128), (4, 96),
                                 (8, 96), (4, 288), (8, 288)])
def test_movement_does_not_enter_the_score(B, D, monkeypatch):
    """raw keys, tiled against the register-resident movement (the first
    three shapes) and against the streamed one: equal bit for bit"""
    from vearch_amd import ktest
    (cent, ids, vecs, queries, probes), marks, bm = _case(B, D)
    for ip in (False, True):
        dev, _ = _encoded_lists(B, D, cent, ids, vecs, queries, marks, False,
                                ip)
        got = {}
        for knob in ("1", "0"):
            monkeypatch.setenv(KNOB, knob)
            assert ktest.rabitq_scan_is_tiled(B, D) is (knob == "1")
            got[knob] = ktest.rabitq_scan(
                dev, probes, queries, cent, 3, 10, ip,
                bitmap=kr.bitmap_words(bm), nb_bits=B)[0]
        assert (got["1"] != np.uint64(kr.EMPTY)).any()
        assert np.array_equal(got["1"], got["0"])


def test_engine(monkeypatch):
    """an IVFRABITQ table of d = 96, nb_bits = 4 searches the same ids and
    scores, bit for bit, tiled (the default) and streamed"""
    from vearch_amd import ktest
    n, d, nlist = 4000, 96, 16
    base = gen_clustered(n, d, seed=21)
    q = gen_queries(base, 32, seed=22)
    eng = make_engine("/tmp/gamma_rbq_tiled")
    eng.create_table(d, "IVFRABITQ", _params(nlist, 4, False, n))
    eng.add(base)
    eng.build_index()
    for rerank in (0, 100):
        monkeypatch.delenv(KNOB, raising=False)
        assert ktest.rabitq_scan_is_tiled(4, d)
        td, ti = eng.raw_search(q, 10, nprobe=nlist, rerank=rerank)
        monkeypatch.setenv(KNOB, "0")
        assert not ktest.rabitq_scan_is_tiled(4, d)
        sd, si = eng.raw_search(q, 10, nprobe=nlist, rerank=rerank)
        assert (ti >= 0).all()
        assert np.array_equal(ti, si) and np.array_equal(td, sd)
    eng.close()
