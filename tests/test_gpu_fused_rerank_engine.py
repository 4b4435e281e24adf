"""Engine-level: a raw search whose exact re-rank and final top-k run
inside the IVFPQ scan kernel returns, bit for bit, what the same search
returns with GAMMA_FUSE_RERANK=0 (gk::rerank and gk::sort_rows as kernels
of their own), and the debug accessor names the path that ran. The knob is
read per search, so both paths run in this process.

GAMMA_SCAN_S=1 keeps a 64-query batch on one workgroup per query (the only
launch shape that fuses); without it such a batch is probe-split and must
report the unfused path."""
import os

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

D, M, NLIST, N, NPROBE, K, RECALL = 128, 32, 64, 20000, 8, 10, 200


def _build(path, base, nlist, extra=""):
    from vearch_amd import GammaEngine
    os.makedirs(path, exist_ok=True)
    eng = GammaEngine(path=path)
    eng.create_table(
        base.shape[1], "IVFPQ",
        '{"ncentroids": %d, "nsubvector": %d, "metric_type": "L2", '
        '"training_threshold": %d%s}' % (nlist, M, base.shape[0], extra))
    eng.add(base)
    eng.build_index()
    return eng


@pytest.fixture(scope="module")
def data():
    base = orc.gen_clustered(N, D, seed=42, ncl=200)
    return base, orc.gen_queries(base, 64, seed=1)


@pytest.fixture(scope="module")
def eng(data):
    e = _build("/tmp/gamma_fused_rr", data[0], NLIST)
    yield e
    e.close()


def _both(eng, q, monkeypatch, fused_expected=True, **kw):
    """the same search with the knob unset and = 0"""
    monkeypatch.delenv("GAMMA_FUSE_RERANK", raising=False)
    fd, fi = eng.raw_search(q, K, nprobe=NPROBE, **kw)
    assert eng.debug_last_search_fused() == fused_expected
    t = eng.last_timing()
    monkeypatch.setenv("GAMMA_FUSE_RERANK", "0")
    ud, ui = eng.raw_search(q, K, nprobe=NPROBE, **kw)
    assert not eng.debug_last_search_fused()
    monkeypatch.delenv("GAMMA_FUSE_RERANK")
    assert np.array_equal(fi, ui)
    assert np.array_equal(fd.view(np.uint32), ud.view(np.uint32))
    return fd, fi, t


@pytest.mark.parametrize("metric", [1, 2], ids=["l2", "ip"])
def test_fused_equals_unfused(data, eng, metric, monkeypatch):
    _, q = data
    monkeypatch.setenv("GAMMA_SCAN_S", "1")
    fd, fi, t = _both(eng, q, monkeypatch, rerank=RECALL, metric=metric)
    assert (fi >= 0).all()
    # best first: L2 ascending, inner product descending
    s = fd if metric == 1 else -fd
    assert (np.diff(s, axis=1) >= 0).all()
    # the fused kernel is the scan stage; nothing runs after it
    assert t["post_us"] < t["scan_us"]


def test_large_batch_fuses_by_itself(data, eng, monkeypatch):
    """2048 queries: one workgroup per query without any knob"""
    _, q = data
    monkeypatch.delenv("GAMMA_SCAN_S", raising=False)
    big = np.repeat(q, 32, axis=0)
    fd, fi, _ = _both(eng, big, monkeypatch, rerank=RECALL)
    assert np.array_equal(fi[::32], fi[31::32])
    monkeypatch.setenv("GAMMA_SCAN_S", "1")
    sd, si, _ = _both(eng, q, monkeypatch, rerank=RECALL)
    assert np.array_equal(fi[::32], si) and np.array_equal(fd[::32], sd)


def test_small_batch_is_probe_split_and_unfused(data, eng, monkeypatch):
    _, q = data
    monkeypatch.setenv("GAMMA_SCAN_S", "1")
    fd, fi, _ = _both(eng, q, monkeypatch, rerank=RECALL)
    monkeypatch.delenv("GAMMA_SCAN_S")
    sd, si, _ = _both(eng, q, monkeypatch, fused_expected=False,
                      rerank=RECALL)
    assert np.array_equal(si, fi)
    assert np.array_equal(sd.view(np.uint32), fd.view(np.uint32))


def test_no_rerank_leg_is_unfused(data, eng, monkeypatch):
    _, q = data
    monkeypatch.setenv("GAMMA_SCAN_S", "1")
    _both(eng, q, monkeypatch, fused_expected=False, rerank=0)


def test_opq_reranks_in_raw_space(monkeypatch):
    """Under OPQ the scan runs on rotated queries and the epilogue on the
    raw ones."""
    n, nlist = 6000, 16
    base = orc.gen_clustered(n, D, seed=5, ncl=60)
    q = orc.gen_queries(base, 64, seed=4)
    e = _build("/tmp/gamma_fused_rr_opq", base, nlist,
               extra=', "opq": {"nsubvector": %d}' % M)
    try:
        e.debug_opq(D)  # raises if the table has no rotation
        monkeypatch.setenv("GAMMA_SCAN_S", "1")
        fd, fi, _ = _both(e, q, monkeypatch, rerank=RECALL)
        # exact distances in RAW space, within the fp32 rounding of a
        # 128-term chain of non-negative terms: (128 + 2) * 2^-24 < 1e-5
        want = ((q[:, None, :].astype(np.float64) -
                 base[fi].astype(np.float64)) ** 2).sum(axis=2)
        assert np.allclose(fd, want, rtol=1e-5, atol=0)
    finally:
        e.close()
