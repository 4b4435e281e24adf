"""gk::coarse_select, the seed-filtered coarse assign (select the seed
columns, filter the other columns' GEMM by each query's seed threshold,
merge): its keys must equal, bit for bit and in order, what the plain pair
gk::dots_mfma + gk::select_from_dots returns on the full width. Both sides
run through the kernel test hooks; n1 (seed columns) and cap (candidate
slots per query) are arguments of the hook."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, NLIST, D, N1 = 130, 1000, 20, 256


@pytest.fixture(scope="module")
def kt():
    from vearch_amd import ktest
    return ktest


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def norms(x):
    return (x.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)


def reference(kt, Q, B, nprobe, ip):
    """the existing pair on all columns -> (nq, nprobe) uint64 keys"""
    Qd, Bd = dev(Q), dev(B)
    dots = kt.dots_mfma(Qd, Bd)
    keys = kt.select_from_dots(dots, B.shape[0], nprobe, not ip, ip,
                               qnorms=dev(norms(Q)), bnorms=dev(norms(B)))
    return kt.keys_to_np(keys)


def filtered(kt, Q, B, nprobe, ip, n1=N1, cap=None):
    cap = B.shape[0] if cap is None else cap
    keys, cnt, flag = kt.coarse_select(
        dev(Q), dev(B), nprobe, not ip, ip, n1, cap,
        qnorms=dev(norms(Q)), bnorms=dev(norms(B)))
    return kt.keys_to_np(keys), cnt, flag


@pytest.fixture(scope="module")
def gauss():
    rng = np.random.default_rng(7)
    return (rng.standard_normal((NQ, D)).astype(np.float32),
            rng.standard_normal((NLIST, D)).astype(np.float32))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("nprobe", [1, 32, 192])
def test_tails(kt, gauss, nprobe, ip):
    """a second, nearly empty row tile (nq = 130), a column tail (1000 is
    no multiple of 128, neither is 1000 - 256), d = 20 below one K tile"""
    Q, B = gauss
    assert kt.coarse_can_filter(NQ, NLIST, D, nprobe, N1)
    want = reference(kt, Q, B, nprobe, ip)
    got, cnt, flag = filtered(kt, Q, B, nprobe, ip)
    print("nprobe=%d ip=%d: candidates mean %.1f max %d" %
          (nprobe, ip, cnt.mean(), cnt.max()))
    assert flag == 0 and (cnt >= 0).all() and (cnt <= NLIST - N1).all()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_forced_overflow(kt, gauss, ip):
    """cap = 8: lists overflow, the flag rises and the switched full-width
    pass still returns the exact result; cap = nlist cannot overflow"""
    Q, B = gauss
    want = reference(kt, Q, B, 32, ip)
    got, cnt, flag = filtered(kt, Q, B, 32, ip, cap=8)
    assert (cnt > 8).any() and flag == 1
    assert np.array_equal(got, want)
    got, cnt, flag = filtered(kt, Q, B, 32, ip, cap=NLIST)
    assert flag == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_ties_across_the_seed_boundary(kt, gauss, ip):
    """every centroid twice, columns c and c + 500: each seed column's twin
    lies past the seed columns, with the same distance and a larger id"""
    Q, B = gauss
    B2 = np.concatenate([B[:500], B[:500]])
    want = reference(kt, Q, B2, 32, ip)
    got, cnt, flag = filtered(kt, Q, B2, 32, ip)
    assert flag == 0
    assert np.array_equal(got, want)
    ids = (got & np.uint64(0xffffffff)).astype(np.int64)
    assert (ids >= 500).any() and (ids < 500).any()


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_all_equal_distances(kt, gauss, ip):
    """all-zero centroids: every key of a row ties on distance, the seeds
    are ids 0..nprobe-1 and no later column is below the threshold"""
    Q, _ = gauss
    Z = np.zeros((NLIST, D), np.float32)
    want = reference(kt, Q, Z, 32, ip)
    got, cnt, flag = filtered(kt, Q, Z, 32, ip)
    assert flag == 0 and (cnt == 0).all()
    assert np.array_equal(got, want)
    ids = (got & np.uint64(0xffffffff)).astype(np.int64)
    assert np.array_equal(ids, np.tile(np.arange(32), (NQ, 1)))


def test_all_winners_past_the_seed_columns(kt, gauss):
    """the seed columns are far away from every query: all seeds are
    displaced"""
    Q, B = gauss
    far = B.copy()
    far[:N1] += 50.0
    want = reference(kt, Q, far, 32, False)
    got, cnt, flag = filtered(kt, Q, far, 32, False)
    assert flag == 0
    assert np.array_equal(got, want)
    ids = (got & np.uint64(0xffffffff)).astype(np.int64)
    assert (ids >= N1).all()
    # every column past the seeds is below every seed here
    assert (cnt == NLIST - N1).all()


def test_predicate_and_old_path(kt, gauss):
    Q, B = gauss
    assert kt.coarse_can_filter(NQ, NLIST, D, 32, N1)
    assert kt.coarse_can_filter(64, 2 * N1, D, 192, N1)
    cases = [  # (nq, nlist, nprobe) the predicate refuses
        (NQ, 2 * N1 - 1, 32),  # nlist < 2 n1
        (NQ, NLIST, 193),      # past the wave selector
        (63, NLIST, 32),       # nq < 64
    ]
    for nq, nlist, nprobe in cases:
        assert not kt.coarse_can_filter(nq, nlist, D, nprobe, N1)
        want = reference(kt, Q[:nq], B[:nlist], nprobe, False)
        got, cnt, flag = filtered(kt, Q[:nq], B[:nlist], nprobe, False)
        assert np.array_equal(got, want), (nq, nlist, nprobe)
        # the plain pair ran: counters and flag keep the hook's pre-fill
        assert (cnt == -7).all() and flag == -7
    assert not kt.coarse_can_filter(NQ, NLIST, 18, 32, N1)   # d % 4
    assert not kt.coarse_can_filter(NQ, NLIST, D, 32, 200)   # n1 % 128


def test_switch_and_knobs(kt, monkeypatch):
    monkeypatch.delenv("GAMMA_FUSE_COARSE", raising=False)
    monkeypatch.delenv("GAMMA_COARSE_SEED_COLS", raising=False)
    monkeypatch.delenv("GAMMA_COARSE_CAND_CAP", raising=False)
    assert kt.coarse_knobs() == (4096, 1024)
    assert kt.coarse_can_filter(10000, 16384, 128, 32)
    assert kt.coarse_can_filter(10000, 8192, 128, 32)
    assert not kt.coarse_can_filter(10000, 8191, 128, 32)
    monkeypatch.setenv("GAMMA_FUSE_COARSE", "0")
    assert not kt.coarse_can_filter(10000, 16384, 128, 32)
    monkeypatch.delenv("GAMMA_FUSE_COARSE")
    monkeypatch.setenv("GAMMA_COARSE_SEED_COLS", "1024")
    monkeypatch.setenv("GAMMA_COARSE_CAND_CAP", "2048")
    assert kt.coarse_knobs() == (1024, 2048)
    assert kt.coarse_can_filter(10000, 2048, 128, 32)
    monkeypatch.setenv("GAMMA_COARSE_SEED_COLS", "1000")  # not of 128
    assert kt.coarse_knobs()[0] == 4096
