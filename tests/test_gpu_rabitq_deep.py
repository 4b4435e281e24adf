"""IVFRABITQ with recall_num / topN beyond 1024 (the deep top-k path),
through GammaEngine. d = 64, N = 6000, nlist = nprobe = 8: every entry is
scanned. References: fp64 brute force (rabitq_ref.brute) and the numpy
estimates of rabitq_ref / rabitq_ex_ref under rabitq_ref.check_row, the
comparison of the existing no-re-rank tests."""
import numpy as np
import pytest

import rabitq_ex_ref as rx
import rabitq_ref as rr
from test_gpu_rabitq import (_exact_scores, _sum_tol, gen_clustered,
                             gen_queries, make_engine)
from test_gpu_rabitq_ex import _params

pytestmark = pytest.mark.gpu

N, D, NLIST, NQ, K = 6000, 64, 8, 12, 10


GONE = np.zeros(N, dtype=bool)
GONE[::5] = True                     # the ids test (c) deletes


def _well_separated(q, base, ip, gone):
    """queries whose fp64 top-(K + 1), over the live rows, has every
    consecutive gap above twice the fp32 bound of one re-ranked distance
    (the tolerance of _check_exact), so fp32 cannot reorder them"""
    _, wi = rr.brute(q, base, K + 1, ip, del_bitmap=gone)
    ex = _exact_scores(q, base, wi, ip)
    mass = (q.astype(np.float64) ** 2).sum(axis=1)[:, None] + \
        (base[wi].astype(np.float64) ** 2).sum(axis=2)
    bound = _sum_tol(D) * 2.0 * mass.max(axis=1)
    return np.abs(np.diff(ex, axis=1)).min(axis=1) > 2.0 * bound


@pytest.fixture(scope="module",
                params=[(B, ip) for B in (1, 4, 8) for ip in (False, True)],
                ids=lambda p: "B%d-%s" % (p[0], "ip" if p[1] else "l2"))
def built(request):
    B, ip = request.param
    base = gen_clustered(N, D, seed=11)
    q = gen_queries(base, 4 * NQ, seed=12)
    ok = _well_separated(q, base, ip, None) & _well_separated(q, base, ip,
                                                              GONE)
    assert ok.sum() >= NQ
    q = q[ok][:NQ]
    eng = make_engine("/tmp/gamma_rbq_deep_%d_%d" % (B, ip))
    eng.create_table(D, "IVFRABITQ", _params(NLIST, B, ip, N))
    eng.add(base)
    eng.build_index()
    yield eng, base, q, B, ip
    eng.close()


def _check_exact(gd, gi, q, base, ip):
    """returned distances are the exact ones of the returned ids, at the
    tolerance of test_gpu_rabitq.test_rerank_and_recall"""
    mass = (q.astype(np.float64) ** 2).sum(axis=1)[:, None] + \
        (base[gi].astype(np.float64) ** 2).sum(axis=2)
    assert np.all(np.abs(gd - _exact_scores(q, base, gi, ip))
                  <= _sum_tol(D) * 2.0 * mass)


def test_rerank_sees_everything(built):
    """(a) recall_num = 8192 >= N: the ids are the fp64 brute-force top-10."""
    eng, base, q, B, ip = built
    gd, gi = eng.raw_search(q, K, nprobe=NLIST, rerank=8192)
    assert np.array_equal(gi, rr.brute(q, base, K, ip)[1])
    _check_exact(gd, gi, q, base, ip)


def test_top2048_estimates(built):
    """(b) topN = 2048 without re-rank: (id, estimate) rows against the
    numpy estimates over the engine's own lists; check_row also asserts the
    (estimate, id) order."""
    eng, base, q, B, ip = built
    cent = eng.debug_model(NLIST, D)[0]
    lists = [eng.debug_list(ln, rx.code_size(D, B)) for ln in range(NLIST)]
    ids, codes = [i for i, _ in lists], [c for _, c in lists]
    gd, gi = eng.raw_search(q, 2048, nprobe=NLIST)
    probes = np.arange(NLIST)
    for r in range(NQ):
        cand = rr.candidates(q[r], cent, ids, codes, probes, ip) if B == 1 \
            else rx.candidates(q[r], cent, ids, codes, probes, B, ip)
        rr.check_row(gd[r], gi[r], *cand, ip)


def test_deleted_ids_stay_out(built):
    """(c) a fifth of the ids deleted, recall_num = 1025. Runs last on the
    module's engine: it mutates the table."""
    eng, base, q, B, ip = built
    for vid in np.flatnonzero(GONE):
        assert eng.delete_doc(str(vid)) == 0
    gd, gi = eng.raw_search(q, K, nprobe=NLIST, rerank=1025)
    assert not GONE[gi].any()
    assert np.array_equal(gi, rr.brute(q, base, K, ip, del_bitmap=GONE)[1])
    _check_exact(gd, gi, q, base, ip)


def test_other_kinds_keep_1024():
    """(d) IVFPQ refuses recall_num = 1025 with the message as it was."""
    eng = make_engine("/tmp/gamma_rbq_deep_pq")
    base = gen_clustered(2000, D, seed=13)
    eng.create_table(D, "IVFPQ", '{"ncentroids": 8, "nsubvector": 16, '
                     '"metric_type": "L2", "training_threshold": 2000}')
    eng.add(base)
    eng.build_index()
    with pytest.raises(RuntimeError, match="recall_num\\) = 1025 exceeds this "
                       "engine's supported maximum of 1024"):
        eng.search_pb(base[:2], topn=K,
                      index_params='{"nprobe": 8, "recall_num": 1025}')
    eng.close()
