"""The ingest and table kernels on their own, through the kernel test
hooks: pq_tables_a / pq_tables_b / pq_cwn against the oracle library's
serial-fmaf chains (the promise of kernels.h the L2 ADC bit-exactness of
every IVFPQ index rests on), pq_sterm / pq_sterm_buckets against fp32 adds
in ascending m, bucket_scatter, residuals, row_norms, extract_probe0 and
rabitq_sval_buckets. Nothing here has a tolerance: fp32 bit patterns, bytes
and ints are compared with np.array_equal.

Table and S-term inputs are Gaussian: on grid values every order of the
fmafs and adds gives the same bits, so only rounding sums tell the orders
apart."""
import numpy as np
import pytest

from oracle import gamma_oracle as go
from oracle import kernel_refs as kr

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gauss(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(
        np.float32)


# ------------------------------------------------------------- PQ tables
# dsub 2, 3, 4, 6, 8, 12: the scalar branch (dsub & 3) and the float4 one
DSUB_DMS = [(8, 4), (12, 4), (16, 4), (24, 4), (32, 4), (48, 4)]
# the shapes the scan tests of test_gpu_scan_variants.py take their L2
# tables at
SCAN_DMS = {16: [(32, 16), (128, 32), (128, 64), (192, 96), (24, 12),
                 (96, 24)],
            256: [(48, 12), (192, 48), (128, 64), (384, 96)]}
NQ, NLIST = 3, 5


@pytest.mark.parametrize("ksub", [256, 16])
def test_pq_tables_match_the_oracle_chains(ksub):
    import torch
    from vearch_amd import ktest
    for d, M in DSUB_DMS + SCAN_DMS[ksub]:
        q = _gauss((NQ, d), 3 * d + M)
        cent = _gauss((NLIST, d), 5 * d + M)
        cb = _gauss((M, ksub, d // M), 7 * d + M + ksub)
        q_d, cb_d = torch.from_numpy(q).cuda(), torch.from_numpy(cb).cuda()
        tag = (d, M, ksub)
        a = ktest.pq_tables_a(q_d, cb_d, M, ksub).cpu().numpy()
        assert np.array_equal(_bits(a), _bits(go.pct1_a_table(q, cb, M, ksub))
                              ), tag
        b = ktest.pq_tables_b(cent, cb, M, ksub)
        assert np.array_equal(_bits(b),
                              _bits(go.pct1_b_table(cent, cb, M, ksub))), tag
        # fmaf(-2, 0, cwn) is cwn exactly: the A chain of a zero query
        cwn = ktest.pq_cwn(cb_d, M, ksub).cpu().numpy()
        zero = go.pct1_a_table(np.zeros((1, d), np.float32), cb, M, ksub)[0]
        assert np.array_equal(_bits(cwn), _bits(zero)), tag


# ----------------------------------------------------------------- S term
def _sterm_inputs(M, ksub, n, seed):
    rng = np.random.default_rng(seed)
    btab = _gauss((NLIST, M, ksub), seed + 1)
    codes = rng.integers(0, ksub, size=(n, M), dtype=np.uint8)
    entries = codes if ksub == 256 else kr.pack4(codes)
    return rng, btab, codes, entries


@pytest.mark.parametrize("ksub", [256, 16])
@pytest.mark.parametrize("M", [4, 12, 32])
def test_pq_sterm(M, ksub):
    from vearch_amd import ktest
    for n in (1, 255, 257, 1000):
        rng, btab, codes, entries = _sterm_inputs(M, ksub, n, 13 * M + n)
        asg = rng.integers(0, NLIST, size=n).astype(np.int32)
        asg[0] = NLIST - 1
        if n > 2:
            asg[1], asg[n - 1], asg[n // 2] = -1, NLIST, NLIST + 9
        tag = (M, ksub, n)
        got = ktest.pq_sterm(entries, btab, M, ksub, asg=asg)
        assert np.array_equal(_bits(got),
                              _bits(kr.sterm_ref(btab, codes, asg))), tag
        if n > 2:
            assert _bits(got)[[1, n - 1, n // 2]].tolist() == [0, 0, 0], tag
        # asg = NULL: every vector in list asg_const
        for ln in (0, NLIST - 1):
            got = ktest.pq_sterm(entries, btab, M, ksub, asg=None,
                                 asg_const=ln)
            want = kr.sterm_ref(btab, codes, np.full(n, ln))
            assert np.array_equal(_bits(got), _bits(want)), tag + (ln,)
        # a list number outside [0, nlist) alone: all zeros
        got = ktest.pq_sterm(entries, btab, M, ksub,
                             asg=np.full(n, -1, np.int32))
        assert not _bits(got).any(), tag


@pytest.mark.parametrize("ksub", [256, 16])
@pytest.mark.parametrize("M", [4, 12, 32])
def test_pq_sterm_buckets(M, ksub):
    from vearch_amd import ktest
    sizes = [0, 1, 257, 300, 64]
    assert len(sizes) == NLIST
    rng, btab, codes, entries = _sterm_inputs(M, ksub, sum(sizes), 17 * M)
    cuts = np.cumsum([0] + sizes)
    buckets = [entries[cuts[i]:cuts[i + 1]] for i in range(NLIST)]
    for skip in ((), (3,), (2,)):
        out = ktest.pq_sterm_buckets(buckets, btab, M, ksub, skip=skip)
        for li, n in enumerate(sizes):
            tag = (M, ksub, skip, li)
            if li in skip:
                assert out[li] is None
                continue
            own = codes[cuts[li]:cuts[li + 1]]
            want = kr.sterm_ref(btab, own, np.full(n, li))
            assert np.array_equal(_bits(out[li][:n]), _bits(want)), tag
            assert (out[li][n:] == ktest.SVAL_CANARY).all(), tag
            if n:  # and the bits of the per-vector kernel
                one = ktest.pq_sterm(buckets[li], btab, M, ksub, asg=None,
                                     asg_const=li)
                assert np.array_equal(_bits(out[li][:n]), _bits(one)), tag


# --------------------------------------------------------- bucket scatter
@pytest.mark.parametrize("entry_bytes", [6, 8, 16, 48, 512])
def test_bucket_scatter(entry_bytes):
    """Byte path (6) and word paths; segments of 0, 1 and 300 entries
    taken from non-contiguous stretches of the staged arrays, one without
    an S-term destination; a run without staged S terms. Nothing is
    written behind a segment's count."""
    from vearch_amd import ktest
    rng = np.random.default_rng(entry_bytes)
    n = 720
    ids = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    data = rng.integers(0, 256, size=(n, entry_bytes), dtype=np.uint8)
    svals = _gauss((n,), entry_bytes + 1)
    segs = [(5, 300, True), (400, 1, True), (350, 0, True),
            (419, 300, False), (0, 1, True), (719, 1, True)]
    for sv_src in (svals, None):
        out = ktest.bucket_scatter(ids, data, sv_src, segs, entry_bytes)
        for (start, count, with_sv), (oi, od, os_) in zip(segs, out):
            tag = (entry_bytes, start, count, sv_src is None)
            assert np.array_equal(oi[:count], ids[start:start + count]), tag
            assert (oi[count:] == ktest.COMPACT_CANARY_ID).all(), tag
            assert np.array_equal(od[:count], data[start:start + count]), tag
            assert (od[count:] == ktest.COMPACT_CANARY_BYTE).all(), tag
            assert (os_ is None) == (not with_sv)
            if os_ is None:
                continue
            if sv_src is None:  # nothing to copy: untouched
                assert (os_ == ktest.COMPACT_CANARY_SVAL).all(), tag
            else:
                assert np.array_equal(_bits(os_[:count]),
                                      _bits(svals[start:start + count])), tag
                assert (os_[count:] == ktest.COMPACT_CANARY_SVAL).all(), tag


# --------------------------------------------------------------- the rest
@pytest.mark.parametrize("n,d", [(63, 4), (64, 4), (65, 4), (7, 36), (1, 4),
                                 (257, 128)])
def test_residuals(n, d):
    """n * d on either side of one 256-thread block; repeated lists."""
    from vearch_amd import ktest
    rng = np.random.default_rng(n * d)
    x, cent = _gauss((n, d), n + d), _gauss((6, d), n + d + 1)
    asg = rng.integers(0, 6, size=n).astype(np.int32)
    asg[n // 2:] = asg[0]
    got = ktest.residuals(x, cent, asg)
    assert np.array_equal(_bits(got), _bits(x - cent[asg]))


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("d", [4, 36, 128])
def test_row_norms(d, n):
    from vearch_amd import ktest
    x = _gauss((n, d), 31 * d + n)
    want = np.array([go.ip_serial(x[i:i + 1], x[i:i + 1])[0, 0]
                     for i in range(n)], dtype=np.float32)
    assert np.array_equal(_bits(ktest.row_norms(x)), _bits(want))


@pytest.mark.parametrize("nq", [1, 257])
def test_extract_probe0(nq):
    from vearch_amd import ktest
    rng = np.random.default_rng(nq)
    for nprobe in (1, 7):
        probes = rng.integers(-1, 70000, size=(nq, nprobe)).astype(np.int64)
        probes[0, 0] = -1
        probes[-1, 0] = 2 ** 31 - 1
        got = ktest.extract_probe0(probes)
        assert got.dtype == np.int32
        assert np.array_equal(got, probes[:, 0].astype(np.int32))


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("d", [32, 96])
def test_rabitq_sval_buckets(d, ip):
    """Encode, drop the S terms, rebuild them from the entries: the bits
    of rabitq_encode. Centroids on the grid, so the sum of the centroid's
    coordinates under an entry's set bits is exact in any order and a
    float64 sum is a reference of its own."""
    from vearch_amd import ktest
    nlist = 5
    sizes = [70, 0, 1, 257, 9]
    cent = kr.grid((nlist, d), seed=d)
    x = _gauss((sum(sizes), d), d + 1)
    asg = np.repeat(np.arange(nlist), sizes).astype(np.int32)
    ent, sv = ktest.rabitq_encode(x, asg, cent, ip)
    bits = np.unpackbits(ent[:, :d // 8], axis=1, bitorder="little")
    want = kr._exact_f32(
        (bits.astype(np.float64) * cent[asg].astype(np.float64)).sum(axis=1))
    assert np.array_equal(_bits(sv), _bits(want))
    cuts = np.cumsum([0] + sizes)
    buckets = [ent[cuts[i]:cuts[i + 1]] for i in range(nlist)]
    for skip in ((), (3,)):
        out = ktest.rabitq_sval_buckets(buckets, cent, skip=skip)
        for li, n in enumerate(sizes):
            if li in skip:
                assert out[li] is None
                continue
            assert np.array_equal(_bits(out[li][:n]),
                                  _bits(want[cuts[li]:cuts[li + 1]])), (li,)
            assert np.array_equal(_bits(out[li][:n]),
                                  _bits(sv[cuts[li]:cuts[li + 1]])), (li,)
            assert (out[li][n:] == ktest.SVAL_CANARY).all(), (li,)
