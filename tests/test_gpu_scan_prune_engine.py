"""Engine level: every search of an IVFPQ table returns, bit for bit, what
the same search returns with GAMMA_SCAN_PRUNE=0, through the life of the
table: build, appends of vectors with unusually large residuals to a far
list, delete and compact, dump and load. The knob is read per launch, so
both sides run in one process. N = 20 000, d = 32, M = 16 (the smallest
sub-quantizer count the pruning kernel serves)."""
import os

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

D, M, NLIST, N, NPROBE, K, RECALL = 32, 16, 64, 20000, 16, 10, 200


def _make(path):
    from vearch_amd import GammaEngine
    os.makedirs(path, exist_ok=True)
    eng = GammaEngine(path=path)
    eng.create_table(
        D, "IVFPQ",
        '{"ncentroids": %d, "nsubvector": %d, "metric_type": "L2", '
        '"training_threshold": %d}' % (NLIST, M, N))
    return eng


def _same(eng, q, monkeypatch):
    """the search with the knob = 1 and = 0, at both launch shapes (one
    workgroup per query with the fused re-rank; probe-split parts)"""
    out = None
    for s in ("1", None):
        if s is None:
            monkeypatch.delenv("GAMMA_SCAN_S", raising=False)
        else:
            monkeypatch.setenv("GAMMA_SCAN_S", s)
        monkeypatch.setenv("GAMMA_SCAN_PRUNE", "1")
        d1, i1 = eng.raw_search(q, K, nprobe=NPROBE, rerank=RECALL)
        monkeypatch.setenv("GAMMA_SCAN_PRUNE", "0")
        d0, i0 = eng.raw_search(q, K, nprobe=NPROBE, rerank=RECALL)
        monkeypatch.delenv("GAMMA_SCAN_PRUNE")
        assert np.array_equal(i1, i0)
        assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32))
        out = (d1, i1)
    monkeypatch.delenv("GAMMA_SCAN_S", raising=False)
    return out


def test_search_is_unchanged_through_the_life_of_a_table(monkeypatch,
                                                         tmp_path):
    PATH = str(tmp_path / "table")
    base = orc.gen_clustered(N, D, seed=7, ncl=40)
    q = orc.gen_queries(base, 64, seed=3)
    eng = _make(PATH)
    try:
        eng.add(base)
        eng.build_index()
        _, ids = _same(eng, q, monkeypatch)
        assert (ids >= 0).all()

        # vectors far from every centroid: they land in some list with a
        # residual many times its radius
        rng = np.random.default_rng(9)
        far = (base.max() + 3.0 + rng.random((8, D))).astype(np.float32)
        eng.add(far)
        _same(eng, np.vstack([far, q[:8]]), monkeypatch)
        one = (far[0] + 0.01).astype(np.float32)
        eng.add_doc("late", one)  # the single-vector append
        _same(eng, np.vstack([one[None], q[:8]]), monkeypatch)

        for v in list(range(0, N, 3)) + [N, N + 1]:
            assert eng.delete_doc(str(v)) == 0
        _same(eng, np.vstack([far, q]), monkeypatch)
        eng.compact(0.0)
        _same(eng, np.vstack([far, q]), monkeypatch)
        eng.dump()
    finally:
        eng.close()

    eng = _make(PATH)
    try:
        eng.load()
        _, ids = _same(eng, np.vstack([far, q]), monkeypatch)
        assert (ids[8:, 0] >= 0).all()
    finally:
        eng.close()
