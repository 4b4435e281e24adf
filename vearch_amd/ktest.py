"""ctypes wrapper over the kernel test hooks of libgamma.so
(include/gamma_bench.h "kernel test hooks", csrc/ktest.cpp): each function
drives ONE gk:: kernel entry on torch device tensors. TEST ONLY — the
product path never imports this module.

u64 keys travel as torch.int64 tensors (same bits); `keys_to_dev` /
`keys_to_np` convert from/to numpy uint64."""
import ctypes

import numpy as np
import torch

from . import engine

_ready = False


class KTestError(RuntimeError):
    """A hook returned a non-zero hipError_t (`.code`)."""

    def __init__(self, name, code):
        super().__init__(f"{name} failed: hipError_t {code}")
        self.code = code


def _lib():
    global _ready
    L = engine.lib()
    if not _ready:
        c = ctypes
        vp, i32, i64 = c.c_void_p, c.c_int, c.c_int64
        L.GammaKTestDotsMfma.argtypes = [vp, i32, vp, i64, i32, vp]
        L.GammaKTestSelectFromDots.argtypes = [
            i32, i64, i64, i64, vp, vp, vp, i32, i32, vp, i32, vp, i32]
        L.GammaKTestSelectRowsFull.argtypes = [
            i32, i32, i64, vp, vp, vp, i32, i32, i32, vp, vp]
        L.GammaKTestArgminRows.argtypes = [i64, i32, vp, vp, vp, i32, vp]
        L.GammaKTestRerank.argtypes = [
            i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]
        L.GammaKTestSortRows.argtypes = [i32, i32, i32, vp, i32, vp, vp]
        L.GammaKTestUnpackKeys.argtypes = [i64, vp, i32, vp, vp]
        L.GammaKTestPqEncode.argtypes = [i64, i32, i32, i32, vp, vp, vp]
        L.GammaKTestPqEncodePack4.argtypes = [i64, i32, i32, vp, vp, vp]
        L.GammaKTestFlatStreamScan.argtypes = [
            i32, i64, i32, i32, vp, vp, i32, vp, i32, vp]
        L.GammaKTestBucketCompact.argtypes = [i32, vp, vp, i32]
        L.GammaKTestPqTablesA.argtypes = [i32, i32, i32, i32, vp, vp, vp]
        L.GammaKTestPqCwn.argtypes = [i32, i32, i32, vp, vp]
        L.GammaKTestPqLutL2.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp]
        L.GammaKTestIvfpqScan.argtypes = [
            i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp,
            i32, vp, vp, i32, vp, vp, vp]
        L.GammaKTestIvfpqScanRerank.argtypes = [
            i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp,
            i32, vp, vp, i32, vp, vp, vp,
            i32, vp, vp, i32, i32, i32, vp, vp]
        L.GammaKTestIvfpqScanCanFuseRerank.argtypes = [
            i32, i32, i32, i32, i32]
        L.GammaKTestPqTablesIp.argtypes = [i32, i32, i32, vp, vp, vp]
        L.GammaKTestIvfpqWideInfo.argtypes = [
            i32, i32, i32, i32, c.POINTER(c.c_int)]
        L.GammaKTestHammingMatrix.argtypes = [vp, i32, vp, i64, i32, vp]
        L.GammaKTestBinivfScan.argtypes = [
            i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]
        L.GammaKTestHammingFlatScan.argtypes = [
            i32, i64, i32, i32, vp, vp, i32, vp, vp]
        L.GammaKTestRabitqEncode.argtypes = [
            i64, i32, vp, vp, i32, i32, vp, i32, vp, vp]
        L.GammaKTestRabitqScan.argtypes = [
            i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
        L.GammaKTestIvfflatScan.argtypes = [
            i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp]
        L.GammaKTestPqTablesB.argtypes = [i32, i32, i32, i32, vp, vp, vp]
        L.GammaKTestPqSterm.argtypes = [
            i64, i32, i32, i32, vp, vp, i32, vp, vp]
        L.GammaKTestPqStermBuckets.argtypes = [i32, i32, i32, vp, vp]
        L.GammaKTestBucketScatter.argtypes = [i32, vp, vp, vp, vp, i32]
        L.GammaKTestResiduals.argtypes = [i64, i32, vp, vp, vp, vp]
        L.GammaKTestRowNorms.argtypes = [vp, i64, i32, vp]
        L.GammaKTestExtractProbe0.argtypes = [i32, i32, vp, vp]
        L.GammaKTestRabitqSvalBuckets.argtypes = [i32, i32, vp, vp]
        L.GammaKTestCoarseSelect.argtypes = [
            vp, i32, vp, i64, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp,
            vp, vp]
        L.GammaKTestCoarseCanFilter.argtypes = [
            i32, i64, i32, i32, i32, c.POINTER(c.c_int)]
        _ready = True
    return L


def _p(t, dtype=None):
    """device pointer of a tensor (None -> NULL)"""
    if t is None:
        return None
    assert t.is_cuda, "kernel hooks take device tensors only"
    if dtype is not None:
        assert t.dtype == dtype, f"expected {dtype}, got {t.dtype}"
    return ctypes.c_void_p(t.data_ptr())


def _call(name, *args):
    torch.cuda.synchronize()  # inputs were produced on torch's stream
    rc = getattr(_lib(), name)(*args)
    if rc != 0:
        raise KTestError(name, rc)


def keys_to_dev(keys_u64):
    """numpy uint64 keys -> device int64 tensor with the same bits"""
    a = np.ascontiguousarray(keys_u64, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def keys_to_np(keys_dev):
    """device int64 key tensor -> numpy uint64"""
    return keys_dev.cpu().numpy().view(np.uint64)


def bitmap_to_dev(words_u32):
    a = np.ascontiguousarray(words_u32, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def seg_table(segs):
    """device array of device pointers, one per segment tensor. The
    caller keeps `segs` alive while the table is in use."""
    for t in segs:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    return torch.tensor([t.data_ptr() for t in segs],
                        dtype=torch.int64).cuda()


def split_segments(base_np, seg_shift):
    """(n, d) host array -> list of separately allocated device segments
    of 1 << seg_shift rows (the last one may be short)."""
    step = 1 << seg_shift
    base_np = np.ascontiguousarray(base_np, dtype=np.float32)
    return [torch.from_numpy(base_np[i:i + step].copy()).cuda()
            for i in range(0, base_np.shape[0], step)]


# ------------------------------------------------------------------ hooks
def dots_mfma(Q, B):
    """out[i][j] = dot(Q_i, B_j); Q (nq, d), B (n, d) f32 contiguous."""
    assert Q.is_contiguous() and B.is_contiguous()
    nq, d = Q.shape
    n = B.shape[0]
    assert B.shape[1] == d and d % 4 == 0
    out = torch.full((nq, n), float("nan"), dtype=torch.float32,
                     device=Q.device)
    _call("GammaKTestDotsMfma", _p(Q, torch.float32), nq,
          _p(B, torch.float32), n, d, _p(out))
    return out


def select_from_dots(dots, ncols, k2, l2, ip_order, qnorms=None,
                     bnorms=None, col_base=0, bitmap=None, state=None,
                     seeded=False):
    """dots: (nq, ld) device tensor whose first `ncols` columns are
    selected on (ld = row stride). bnorms and bitmap are indexed by the
    global id col_base + c. Returns the (nq, k2) key state (int64 bits);
    pass it back as `state` with seeded=True to accumulate."""
    assert dots.dim() == 2 and dots.stride(1) == 1
    nq, ld = dots.shape[0], dots.stride(0)
    assert 0 < ncols <= dots.shape[1] and 1 <= k2 <= 1024
    if l2:
        assert qnorms is not None and bnorms is not None
        assert qnorms.numel() >= nq and bnorms.numel() >= col_base + ncols
    if state is None:
        assert not seeded
        state = torch.full((nq, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                           device=dots.device)
    assert state.shape == (nq, k2) and state.is_contiguous()
    _call("GammaKTestSelectFromDots", nq, ncols, col_base, ld,
          _p(dots, torch.float32), _p(qnorms, torch.float32),
          _p(bnorms, torch.float32), int(bool(l2)), int(bool(ip_order)),
          _p(bitmap, torch.int32), k2, _p(state, torch.int64),
          int(bool(seeded)))
    return state


def select_rows_full(dots, ncols, k2, l2, ip_order, qnorms=None,
                     bnorms=None):
    """Full-sort row select; returns (dists f32, ids int64), (nq, k2).
    Outputs are pre-filled with a sentinel (-7) so a refused launch is
    visible."""
    assert dots.dim() == 2 and dots.stride(1) == 1
    nq, ld = dots.shape[0], dots.stride(0)
    assert 0 < ncols <= dots.shape[1]
    od = torch.full((nq, k2), -7.0, dtype=torch.float32, device=dots.device)
    oi = torch.full((nq, k2), -7, dtype=torch.int64, device=dots.device)
    _call("GammaKTestSelectRowsFull", nq, ncols, ld,
          _p(dots, torch.float32), _p(qnorms, torch.float32),
          _p(bnorms, torch.float32), int(bool(l2)), int(bool(ip_order)),
          k2, _p(od), _p(oi))
    return od, oi


def argmin_rows(dots, l2, qnorms=None, bnorms=None):
    """argmin per row of a contiguous (nrows, ncols) matrix -> int32."""
    assert dots.dim() == 2 and dots.is_contiguous()
    nrows, ncols = dots.shape
    out = torch.full((nrows,), -7, dtype=torch.int32, device=dots.device)
    _call("GammaKTestArgminRows", nrows, ncols, _p(dots, torch.float32),
          _p(qnorms, torch.float32), _p(bnorms, torch.float32),
          int(bool(l2)), _p(out))
    return out


def rerank(queries, segs, seg_shift, ip, keys_in, keys_out=None):
    """Canonical re-rank of keys_in (nq, ncand) through the segment list
    `segs` (device tensors of 1 << seg_shift rows). keys_out may be
    keys_in itself (in-place)."""
    assert queries.is_contiguous() and keys_in.is_contiguous()
    nq, d = queries.shape
    ncand = keys_in.shape[1]
    assert keys_in.shape[0] == nq and d % 4 == 0
    table = seg_table(segs)
    if keys_out is None:
        keys_out = torch.full_like(keys_in, 0x5A5A5A5A5A5A5A5A)
    _call("GammaKTestRerank", nq, ncand, d, _p(queries, torch.float32),
          _p(table), len(segs), seg_shift, int(bool(ip)),
          _p(keys_in, torch.int64), _p(keys_out, torch.int64))
    return keys_out


def sort_rows(keys, k, ip):
    """Per-row sort of (nq, ncand) keys -> top-k (dists, ids)."""
    assert keys.dim() == 2 and keys.is_contiguous()
    nq, ncand = keys.shape
    assert ncand <= 2048
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device=keys.device)
    oi = torch.full((nq, k), -7, dtype=torch.int64, device=keys.device)
    _call("GammaKTestSortRows", nq, ncand, k, _p(keys, torch.int64),
          int(bool(ip)), _p(od), _p(oi))
    return od, oi


def coarse_can_filter(nq, nlist, d, nprobe, n1=0):
    """gk::coarse_can_filter under the current GAMMA_FUSE_COARSE (n1 = 0:
    the GAMMA_COARSE_SEED_COLS knob)."""
    return _lib().GammaKTestCoarseCanFilter(nq, nlist, d, nprobe, n1,
                                            None) == 1


def coarse_knobs():
    """(seed columns, candidate cap) as the library reads its knobs"""
    out = (ctypes.c_int * 2)()
    _lib().GammaKTestCoarseCanFilter(64, 1 << 20, 4, 1, 0, out)
    return out[0], out[1]


def coarse_select(Q, B, nprobe, l2, ip_order, n1, cap, qnorms=None,
                  bnorms=None):
    """gk::coarse_select: the seed-filtered coarse assign of Q (nq, d) over
    the centroids B (nlist, d). Returns (keys (nq, nprobe) int64 bits,
    cand_cnt (nq,) int32, overflow flag). The counters are pre-filled with
    -7: they keep that value where the predicate sent the call down the
    plain full-width path."""
    assert Q.is_contiguous() and B.is_contiguous()
    nq, d = Q.shape
    nlist = B.shape[0]
    assert B.shape[1] == d and d % 4 == 0 and cap >= 1
    if l2:
        assert qnorms is not None and bnorms is not None
        assert qnorms.numel() >= nq and bnorms.numel() >= nlist
    dev = Q.device
    dots = torch.full((nq, nlist), float("nan"), dtype=torch.float32,
                      device=dev)
    cand = torch.full((nq, cap), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                      device=dev)
    cnt = torch.full((nq + 1,), -7, dtype=torch.int32, device=dev)
    keys = torch.full((nq, nprobe), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                      device=dev)
    _call("GammaKTestCoarseSelect", _p(Q, torch.float32), nq,
          _p(B, torch.float32), nlist, d, _p(qnorms, torch.float32),
          _p(bnorms, torch.float32), int(bool(l2)), int(bool(ip_order)),
          nprobe, n1, cap, _p(dots), _p(cand), _p(cnt), _p(keys))
    cnt = cnt.cpu().numpy()
    return keys, cnt[:nq], int(cnt[nq])


def unpack_keys(keys, ip):
    """keys (any shape, contiguous) -> (dists, ids) of the same shape."""
    assert keys.is_contiguous()
    od = torch.full(keys.shape, -7.0, dtype=torch.float32,
                    device=keys.device)
    oi = torch.full(keys.shape, -7, dtype=torch.int64, device=keys.device)
    _call("GammaKTestUnpackKeys", keys.numel(), _p(keys, torch.int64),
          int(bool(ip)), _p(od), _p(oi))
    return od, oi


def pq_encode(x, codebooks, M, ksub):
    """x (n, d), codebooks (M, ksub, d/M) -> codes uint8 (n, M)."""
    assert x.is_contiguous() and codebooks.is_contiguous()
    n, d = x.shape
    assert ksub in (16, 256) and d % M == 0
    assert codebooks.numel() == ksub * d
    codes = torch.full((n, M), 0xEE, dtype=torch.uint8, device=x.device)
    _call("GammaKTestPqEncode", n, d, M, ksub, _p(x, torch.float32),
          _p(codebooks, torch.float32), _p(codes))
    return codes


def pq_encode_pack4(x, codebooks, M):
    """ksub = 16 encode in packed bucket form -> uint8 (n, M/2)."""
    assert x.is_contiguous() and codebooks.is_contiguous()
    n, d = x.shape
    assert M % 2 == 0 and d % M == 0 and codebooks.numel() == 16 * d
    codes = torch.full((n, M // 2), 0xEE, dtype=torch.uint8,
                       device=x.device)
    _call("GammaKTestPqEncodePack4", n, d, M, _p(x, torch.float32),
          _p(codebooks, torch.float32), _p(codes))
    return codes


def flat_stream_scan(queries, segs, n, seg_shift, k2, ip, bitmap=None):
    """FLAT stream scan over n vectors held in `segs` -> (nq, k2) keys."""
    assert queries.is_contiguous()
    nq, d = queries.shape
    assert d % 4 == 0 and 1 <= k2 <= 1024
    assert len(segs) == (n + (1 << seg_shift) - 1) >> seg_shift
    table = seg_table(segs)
    out = torch.full((nq, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                     device=queries.device)
    _call("GammaKTestFlatStreamScan", nq, n, d, k2,
          _p(queries, torch.float32), _p(table), seg_shift,
          _p(bitmap, torch.int32), int(bool(ip)), _p(out))
    return out


COMPACT_CANARY_ID = 0x5A5A5A5A
COMPACT_CANARY_BYTE = 0xA5
COMPACT_CANARY_SVAL = -7.0


def bucket_compact(segments, entry_bytes, bitmap=None):
    """One gk::bucket_compact launch over `segments`, a list of host
    (ids uint32 (n,), data uint8 (n, entry_bytes), svals float32 (n,) or
    None). Every array gets its own device allocation; destinations have
    the source's length and are pre-filled with the COMPACT_CANARY_*
    values. bitmap: optional device int32 words (bitmap_to_dev).
    Returns one (ids uint32, data uint8, svals float32 or None, kept) per
    segment: the FULL destination arrays, canary tail included."""
    keep_alive, rows, outs = [], [], []
    kept = torch.full((max(len(segments), 1),), -7, dtype=torch.int64,
                      device="cuda")
    for i, (ids, data, svals) in enumerate(segments):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = ids.shape[0]
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(
            n, entry_bytes)
        ids_s = torch.from_numpy(ids.view(np.int32).copy()).cuda()
        data_s = torch.from_numpy(data.copy()).cuda()
        ids_d = torch.full((n,), COMPACT_CANARY_ID, dtype=torch.int32,
                           device="cuda")
        data_d = torch.full((n, entry_bytes), COMPACT_CANARY_BYTE,
                            dtype=torch.uint8, device="cuda")
        sv_s = sv_d = None
        if svals is not None:
            sv = np.ascontiguousarray(svals, dtype=np.float32)
            assert sv.shape == (n,)
            sv_s = torch.from_numpy(sv.copy()).cuda()
            sv_d = torch.full((n,), COMPACT_CANARY_SVAL,
                              dtype=torch.float32, device="cuda")
        keep_alive += [ids_s, data_s, ids_d, data_d, sv_s, sv_d]
        ptr = lambda t: t.data_ptr() if t is not None and n else 0
        rows.append([ptr(ids_s), ptr(data_s), ptr(sv_s), n, ptr(ids_d),
                     ptr(data_d), ptr(sv_d), kept.data_ptr() + 8 * i])
        outs.append((ids_d, data_d, sv_d))
    segs = torch.tensor(rows, dtype=torch.int64).reshape(-1, 8).cuda()
    _call("GammaKTestBucketCompact", len(segments), _p(segs, torch.int64),
          _p(bitmap, torch.int32), entry_bytes)
    kept_h = kept.cpu().numpy()
    return [(i_d.cpu().numpy().view(np.uint32), d_d.cpu().numpy(),
             None if s_d is None else s_d.cpu().numpy(), int(kept_h[i]))
            for i, (i_d, d_d, s_d) in enumerate(outs)]


def pq_tables_a(queries, codebooks, M, ksub):
    """gk::pq_tables_a: queries (nq, d), codebooks (M, ksub, d/M) ->
    atab (nq, M, ksub) f32."""
    assert queries.is_contiguous() and codebooks.is_contiguous()
    nq, d = queries.shape
    assert ksub in (16, 256) and d % M == 0
    assert codebooks.numel() == ksub * d
    atab = torch.full((nq, M, ksub), float("nan"), dtype=torch.float32,
                      device=queries.device)
    _call("GammaKTestPqTablesA", nq, d, M, ksub, _p(queries, torch.float32),
          _p(codebooks, torch.float32), _p(atab))
    return atab


def pq_cwn(codebooks, M, ksub):
    """gk::pq_cwn: codebooks (M, ksub, dsub) -> codeword norms (M, ksub)."""
    assert codebooks.is_contiguous()
    dsub = codebooks.numel() // (M * ksub)
    assert codebooks.numel() == M * ksub * dsub
    cwn = torch.full((M, ksub), float("nan"), dtype=torch.float32,
                     device=codebooks.device)
    _call("GammaKTestPqCwn", M, ksub, dsub, _p(codebooks, torch.float32),
          _p(cwn))
    return cwn


def pq_lut_l2(queries, codebooks, M, ksub):
    """The L2 query table the 8-bit fast scan builds in LDS (codeword
    norms from gk::pq_cwn, then the scan's own table builder), copied out
    per query: (nq, M, ksub) f32."""
    assert queries.is_contiguous() and codebooks.is_contiguous()
    nq, d = queries.shape
    assert ksub in (16, 256) and d % M == 0
    assert codebooks.numel() == ksub * d
    cwn = pq_cwn(codebooks, M, ksub)
    out = torch.full((nq, M, ksub), float("nan"), dtype=torch.float32,
                     device=queries.device)
    _call("GammaKTestPqLutL2", nq, d, M, ksub, _p(queries, torch.float32),
          _p(codebooks, torch.float32), _p(cwn), _p(out))
    return out


def pq_tables_ip(queries, codebooks, M):
    """gk::pq_tables_ip: the inner-product query table the sliced-table
    scan reads, (nq, M, 256) f32."""
    assert queries.is_contiguous() and codebooks.is_contiguous()
    nq, d = queries.shape
    assert d % M == 0 and codebooks.numel() == 256 * d
    out = torch.full((nq, M, 256), float("nan"), dtype=torch.float32,
                     device=queries.device)
    _call("GammaKTestPqTablesIp", nq, d, M, _p(queries, torch.float32),
          _p(codebooks, torch.float32), _p(out))
    return out


WIDE_MS = 32  # IVFPQ_WIDE_MS of kernels.h: sub-quantizers per table slice
WIDE_E = 4    # IVFPQ_WIDE_E: entries per thread per tile


def ivfpq_wide_info(d, M, k2, ksub=256):
    """(slice, tile, is_wide) of the sliced-table scan as the library
    reports them under the current launch knobs: sub-quantizers per table
    slice, entries per tile (WIDE_E x the GAMMA_SCAN_BS block size), and
    whether a launch of this shape takes k_ivfpq_scan_wide."""
    return _wide_info(d, M, k2, ksub)[:3]


def _wide_info(d, M, k2, ksub):
    out = (ctypes.c_int * 5)()
    rc = _lib().GammaKTestIvfpqWideInfo(d, M, ksub, k2, out)
    if rc != 0:
        raise KTestError("GammaKTestIvfpqWideInfo", rc)
    return (int(out[0]), int(out[1]), bool(out[2]), bool(out[3]),
            bool(out[4]))


def ivfpq_scan_reads_table(d, M, k2, ip, ksub=256):
    """gk::ivfpq_scan_reads_table: whether a launch of this shape reads
    `atab` -- the decision IVFIndex::search builds its query table by."""
    return _wide_info(d, M, k2, ksub)[4 if ip else 3]


def ivfpq_scan(lists, probes, probe_dists, queries, centroids, codebooks,
               S, k2, ip, bitmap=None, qmap=None, kill_flag=None,
               code_offsets=None, ksub=256):
    """One gk::ivfpq_scan launch on host arrays (8-bit codes; ksub=16: the
    4-bit kernel, see the end of this text).
    lists: one (ids uint32 (n,), codes uint8 (n, M), svals float32 (n,))
    per inverted list, n = that list's size (0 is legal); every array gets
    its own device allocation. probes int64 (nq, nprobe) may hold -1 and
    ids >= nlist; probe_dists float32 (nq, nprobe). queries (nq, d),
    centroids (nlist, d), codebooks (M, 256, d/M). bitmap: optional uint32
    words; qmap: optional int32 (nq,) query schedule. kill_flag: None
    passes NULL; an int passes a device int holding that value (1 = a
    flag raised before the launch). code_offsets: optional {list index:
    byte offset (a multiple of 4)}: that list's codes start this far into
    their allocation, so they are 4-byte but not 16-byte aligned.
    ksub=16: codebooks are (M, 16, d/M); a list's codes arrive as (n, M)
    values below 16 and are packed into (n, M/2) bucket bytes (low nibble =
    even sub-quantizer); the L2 table is pq_tables_a at ksub 16, inner
    product passes no table (the kernel builds its own) and cwn is NULL;
    code_offsets is refused: the fast shapes load 8- and 16-byte vectors and
    rely on the buckets' alignment.
    Returns (keys, dists, ids): keys uint64 (nq, S, k2) as the kernel
    wrote them, and the merge the engine applies to the S partial rows of
    a query (gk::sort_rows over S*k2 keys), top-k2: dists float32 and ids
    int64 (nq, k2), -1 / -1 where fewer than k2 candidates exist (None,
    None where S * k2 exceeds what sort_rows takes)."""
    keys = _ivfpq_scan_launch(lists, probes, probe_dists, queries,
                              centroids, codebooks, S, k2, ip, bitmap, qmap,
                              kill_flag, code_offsets, ksub, None)
    nq = keys.shape[0]
    if S * k2 > 2048:  # beyond gk::sort_rows (the engine keeps S*k2 <= 2048)
        return keys_to_np(keys), None, None
    od, oi = sort_rows(keys.reshape(nq, S * k2), k2, ip)
    return keys_to_np(keys), od.cpu().numpy(), oi.cpu().numpy()


def ivfpq_scan_can_fuse_rerank(d, M, k2, S, ksub=256):
    """gk::ivfpq_scan_can_fuse_rerank under the current GAMMA_FUSE_RERANK:
    the rule the launcher and IVFIndex::search both decide by."""
    return _lib().GammaKTestIvfpqScanCanFuseRerank(d, M, ksub, k2, S) == 1


def ivfpq_scan_rerank(lists, probes, probe_dists, queries, centroids,
                      codebooks, S, k2, ip, base, seg_shift, k,
                      rr_queries=None, bitmap=None, qmap=None,
                      kill_flag=None, ksub=256):
    """One gk::ivfpq_scan launch WITH its re-rank block: the inputs of
    ivfpq_scan, plus the raw store `base` (n, d) host array, cut into
    separately allocated segments of 1 << seg_shift rows, and k. rr_queries
    (nq, d): the raw-space queries the re-rank measures against (default:
    `queries`; under OPQ the scan's own are rotated ones). Returns (dists
    float32, ids int64), (nq, k), pre-filled with -7 so that a launch that
    wrote nothing shows. A launch the launcher refuses raises KTestError."""
    rq = queries if rr_queries is None else rr_queries
    rr = (np.ascontiguousarray(rq, dtype=np.float32),
          split_segments(base, seg_shift), seg_shift, k)
    od, oi = _ivfpq_scan_launch(lists, probes, probe_dists, queries,
                                centroids, codebooks, S, k2, ip, bitmap,
                                qmap, kill_flag, None, ksub, rr)
    return od.cpu().numpy(), oi.cpu().numpy()


def ivfpq_scan_null_rerank(lists, probes, probe_dists, queries, centroids,
                           codebooks, S, k2, ip, bitmap=None, qmap=None,
                           kill_flag=None, ksub=256):
    """The re-rank hook with NO block: today's launch. Returns the keys
    uint64 (nq, S, k2) as ivfpq_scan returns them."""
    return keys_to_np(_ivfpq_scan_launch(
        lists, probes, probe_dists, queries, centroids, codebooks, S, k2,
        ip, bitmap, qmap, kill_flag, None, ksub, "null"))


def _ivfpq_scan_launch(lists, probes, probe_dists, queries, centroids,
                       codebooks, S, k2, ip, bitmap, qmap, kill_flag,
                       code_offsets, ksub, rr):
    """The launch behind ivfpq_scan (rr None: returns the (nq, S, k2) key
    tensor) and ivfpq_scan_rerank (rr = (raw queries, segments, seg_shift,
    k): returns the (dists, ids) tensors; the key tensor is checked to be
    untouched)."""
    f32 = lambda a: torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a, dtype=np.float32).copy()).cuda()
    q_d, cent_d, cb_d = f32(queries), f32(centroids), f32(codebooks)
    nq, d = q_d.shape
    nlist = len(lists)
    M = cb_d.shape[0]
    assert ksub in (16, 256)
    assert cb_d.shape[1] == ksub and cb_d.numel() == ksub * d
    assert cent_d.shape == (nlist, d)
    if ksub == 16:
        from oracle.kernel_refs import pack4
        assert not code_offsets, "4-bit entries rely on bucket alignment"
        assert M % 2 == 0
    eb = M if ksub == 256 else M // 2  # bytes per bucket entry
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    nprobe = probes.shape[1]
    assert probes.shape == (nq, nprobe)
    pr_d = torch.from_numpy(probes.copy()).cuda()
    pd_d = f32(probe_dists)
    assert pd_d.shape == (nq, nprobe)
    keep, rows = [], []
    for li, (ids, codes, svals) in enumerate(lists):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = ids.shape[0]
        codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(n, M)
        if ksub == 16:
            assert n == 0 or codes.max() < 16
            codes = pack4(codes)
        svals = np.ascontiguousarray(svals, dtype=np.float32)
        assert svals.shape == (n,)
        off = (code_offsets or {}).get(li, 0)
        assert off % 4 == 0 and off >= 0
        buf = np.full(off + n * eb, 0xEE, dtype=np.uint8)
        buf[off:] = codes.ravel()
        cbuf = torch.from_numpy(buf).cuda()
        t = [torch.from_numpy(ids.view(np.int32).copy()).cuda(),
             cbuf[off:], torch.from_numpy(svals.copy()).cuda()]
        keep += t + [cbuf]
        rows.append([x.data_ptr() if n else 0 for x in t] + [n])
    bk_d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).cuda()
    bm_d = None if bitmap is None else bitmap_to_dev(bitmap)
    qm_d = None
    if qmap is not None:
        qm_d = torch.from_numpy(
            np.ascontiguousarray(qmap, dtype=np.int32).copy()).cuda()
    # the resident-table kernels build their own IP table and ignore atab;
    # the sliced-table kernel reads it for both metrics
    if ksub == 256:
        atab = pq_tables_ip(q_d, cb_d, M) if ip \
            else pq_tables_a(q_d, cb_d, M, 256)
        cwn = pq_cwn(cb_d, M, 256)
    else:
        atab = None if ip else pq_tables_a(q_d, cb_d, M, 16)
        cwn = None
    kf_d = None if kill_flag is None else torch.full(
        (1,), int(kill_flag), dtype=torch.int32, device="cuda")
    keys = torch.full((nq, S, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                      device="cuda")
    args = (nq, S, d, M, ksub, nprobe, k2, _p(q_d),
            _p(cent_d), _p(cb_d), _p(atab), _p(cwn), _p(pd_d),
            _p(bk_d, torch.int64), nlist, _p(pr_d, torch.int64),
            _p(bm_d, torch.int32), int(bool(ip)), _p(keys, torch.int64),
            _p(kf_d, torch.int32), _p(qm_d, torch.int32))
    if rr is None:
        _call("GammaKTestIvfpqScan", *args)
        return keys
    if rr == "null":  # the re-rank hook, no block: the plain launch
        _call("GammaKTestIvfpqScanRerank", *args, 0, None, None, 0, 0, 0,
              None, None)
        return keys
    rq, segs, seg_shift, k = rr
    rq_d = f32(rq)
    assert rq_d.shape == (nq, d)
    table = seg_table(segs)
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    _call("GammaKTestIvfpqScanRerank", *args, 1, _p(rq_d), _p(table),
          len(segs), seg_shift, k, _p(od), _p(oi))
    assert bool((keys == 0x5A5A5A5A5A5A5A5A).all()), \
        "a fused launch wrote out_keys"
    return od, oi


def ivfflat_scan(lists, probes, queries, k2, ip, bitmap=None):
    """One gk::ivfflat_scan launch on host arrays. lists: one (ids uint32
    (n,), vecs float32 (n, d)) per inverted list (n = 0 is legal), each
    array in its own device allocation; probes int64 (nq, nprobe) may hold
    -1 and ids >= nlist; queries float32 (nq, d); bitmap: optional uint32
    words. Returns the keys uint64 (nq, k2) as the kernel wrote them."""
    q_d = _f32_dev(queries)
    nq, d = q_d.shape
    assert d % 4 == 0
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    nprobe = probes.shape[1]
    assert probes.shape == (nq, nprobe)
    pr_d = torch.from_numpy(probes.copy()).cuda()
    keep, rows = [], []
    for ids, vecs in lists:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = ids.shape[0]
        vecs = np.ascontiguousarray(vecs, dtype=np.float32).reshape(n, d)
        t = [torch.from_numpy(ids.view(np.int32).copy()).cuda(),
             torch.from_numpy(vecs.copy()).cuda()]
        keep += t
        rows.append([x.data_ptr() if n else 0 for x in t] + [0, n])
    bk_d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).cuda()
    bm_d = None if bitmap is None else bitmap_to_dev(bitmap)
    keys = torch.full((nq, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                      device="cuda")
    _call("GammaKTestIvfflatScan", nq, d, nprobe, k2, _p(q_d),
          _p(bk_d, torch.int64), len(lists), _p(pr_d, torch.int64),
          _p(bm_d, torch.int32), int(bool(ip)), _p(keys, torch.int64))
    return keys_to_np(keys)


# ------------------------------------------------- ingest and table kernels
def _f32_dev(a):
    return torch.from_numpy(
        np.ascontiguousarray(a, dtype=np.float32).copy()).cuda()


def _u8_dev(a):
    return torch.from_numpy(
        np.ascontiguousarray(a, dtype=np.uint8).copy()).cuda()


def _i32_dev(a):
    return torch.from_numpy(
        np.ascontiguousarray(a, dtype=np.int32).copy()).cuda()


def pq_tables_b(centroids, codebooks, M, ksub):
    """gk::pq_tables_b on host arrays: centroids (nlist, d), codebooks
    (M, ksub, d/M) -> btab float32 (nlist, M, ksub) numpy."""
    c_d, cb_d = _f32_dev(centroids), _f32_dev(codebooks)
    nlist, d = c_d.shape
    assert ksub in (16, 256) and d % M == 0 and cb_d.numel() == ksub * d
    btab = torch.full((nlist, M, ksub), float("nan"), dtype=torch.float32,
                      device="cuda")
    _call("GammaKTestPqTablesB", d, M, ksub, nlist, _p(c_d), _p(cb_d),
          _p(btab))
    return btab.cpu().numpy()


def pq_sterm(codes, btab, M, ksub, asg=None, asg_const=0):
    """gk::pq_sterm on host arrays: codes uint8 bucket entries (n, M) or, at
    ksub = 16, packed (n, M/2); btab float32 (nlist, M, ksub); asg int32
    (n,) list numbers (any value; outside [0, nlist) gives 0.0f) or None
    (every vector in list asg_const). -> float32 (n,) numpy, nan where the
    kernel wrote nothing."""
    b_d = _f32_dev(btab)
    nlist = b_d.shape[0]
    assert b_d.shape == (nlist, M, ksub) and ksub in (16, 256)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = codes.shape[0]
    assert codes.shape == (n, M if ksub == 256 else M // 2)
    c_d = _u8_dev(codes)
    a_d = None if asg is None else _i32_dev(asg)
    assert a_d is None or a_d.shape == (n,)
    assert a_d is not None or 0 <= asg_const < nlist
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    _call("GammaKTestPqSterm", n, M, ksub, nlist, _p(c_d),
          _p(a_d, torch.int32), asg_const, _p(b_d), _p(out))
    return out.cpu().numpy()


SVAL_CANARY = -7.0


def _sval_buckets(hook, buckets, entry_bytes, skip, *args):
    """shared by pq_sterm_buckets / rabitq_sval_buckets: one (n,
    entry_bytes) uint8 host array per bucket, each in its own allocation;
    every svals array is n + 8 floats pre-filled with SVAL_CANARY (the
    kernel owns the first n); buckets listed in `skip` pass svals = NULL.
    Returns the full svals arrays (None for a skipped bucket)."""
    keep, rows, outs = [], [], []
    for li, ent in enumerate(buckets):
        ent = np.ascontiguousarray(ent, dtype=np.uint8)
        n = ent.shape[0]
        assert ent.shape == (n, entry_bytes)
        e_d = _u8_dev(ent)
        sv = None if li in skip else torch.full(
            (n + 8,), SVAL_CANARY, dtype=torch.float32, device="cuda")
        keep += [e_d, sv]
        rows.append([0, e_d.data_ptr() if n else 0,
                     0 if sv is None else sv.data_ptr(), n])
        outs.append(sv)
    bk_d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).cuda()
    hook(bk_d, len(buckets), *args)
    return [None if sv is None else sv.cpu().numpy() for sv in outs]


def pq_sterm_buckets(buckets, btab, M, ksub, skip=()):
    """gk::pq_sterm_buckets: bucket li's entries are scored against
    btab[li]. See _sval_buckets for the arguments and the result."""
    b_d = _f32_dev(btab)
    assert b_d.shape == (len(buckets), M, ksub) and ksub in (16, 256)

    def hook(bk_d, nlist):
        _call("GammaKTestPqStermBuckets", nlist, M, ksub,
              _p(bk_d, torch.int64), _p(b_d))
    return _sval_buckets(hook, buckets, M if ksub == 256 else M // 2, skip)


def rabitq_sval_buckets(buckets, centroids, skip=()):
    """gk::rabitq_sval_buckets: bucket li holds entries of d/8 + 8 bytes of
    list li, centroids float32 (nlist, d). See _sval_buckets."""
    c_d = _f32_dev(centroids)
    nlist, d = c_d.shape
    assert nlist == len(buckets) and d % 32 == 0

    def hook(bk_d, nl):
        _call("GammaKTestRabitqSvalBuckets", nl, d, _p(bk_d, torch.int64),
              _p(c_d))
    return _sval_buckets(hook, buckets, d // 8 + 8, skip)


def bucket_scatter(ids_src, data_src, svals_src, segments, entry_bytes,
                   tail=4):
    """One gk::bucket_scatter launch. Staged host arrays: ids_src uint32
    (n,), data_src uint8 (n, entry_bytes), svals_src float32 (n,) or None
    (passes NULL). segments: (src_start, count, with_svals) per bucket;
    each bucket gets its own destination arrays of count + tail entries,
    pre-filled with the COMPACT_CANARY_* values, and with_svals False
    passes sval_dst = NULL. Returns one (ids uint32, data uint8, svals
    float32 or None) per segment: the FULL arrays, canary tail included."""
    ids_src = np.ascontiguousarray(ids_src, dtype=np.uint32)
    n = ids_src.shape[0]
    data_src = np.ascontiguousarray(data_src, dtype=np.uint8)
    assert data_src.shape == (n, entry_bytes)
    i_d = torch.from_numpy(ids_src.view(np.int32).copy()).cuda()
    d_d = _u8_dev(data_src)
    s_d = None if svals_src is None else _f32_dev(svals_src)
    assert s_d is None or s_d.shape == (n,)
    rows, outs = [], []
    for start, count, with_sv in segments:
        assert 0 <= start and start + count <= n
        ids_o = torch.full((count + tail,), COMPACT_CANARY_ID,
                           dtype=torch.int32, device="cuda")
        data_o = torch.full((count + tail, entry_bytes), COMPACT_CANARY_BYTE,
                            dtype=torch.uint8, device="cuda")
        sv_o = torch.full((count + tail,), COMPACT_CANARY_SVAL,
                          dtype=torch.float32, device="cuda") \
            if with_sv else None
        rows.append([ids_o.data_ptr(), data_o.data_ptr(),
                     0 if sv_o is None else sv_o.data_ptr(), start, count])
        outs.append((ids_o, data_o, sv_o))
    segs = torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).cuda()
    _call("GammaKTestBucketScatter", len(segments), _p(segs, torch.int64),
          _p(i_d, torch.int32), _p(d_d, torch.uint8),
          _p(s_d, torch.float32), entry_bytes)
    return [(i_o.cpu().numpy().view(np.uint32), d_o.cpu().numpy(),
             None if s_o is None else s_o.cpu().numpy())
            for i_o, d_o, s_o in outs]


def residuals(x, centroids, assign):
    """gk::residuals on host arrays -> float32 (n, d) numpy."""
    x_d, c_d, a_d = _f32_dev(x), _f32_dev(centroids), _i32_dev(assign)
    n, d = x_d.shape
    assert c_d.shape[1] == d and a_d.shape == (n,)
    assert int(a_d.min()) >= 0 and int(a_d.max()) < c_d.shape[0]
    out = torch.full((n, d), float("nan"), dtype=torch.float32,
                     device="cuda")
    _call("GammaKTestResiduals", n, d, _p(x_d), _p(c_d),
          _p(a_d, torch.int32), _p(out))
    return out.cpu().numpy()


def row_norms(v):
    """gk::row_norms on a host array (n, d) -> float32 (n,) numpy."""
    v_d = _f32_dev(v)
    n, d = v_d.shape
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    _call("GammaKTestRowNorms", _p(v_d), n, d, _p(out))
    return out.cpu().numpy()


def extract_probe0(probes):
    """gk::extract_probe0 on a host int64 (nq, nprobe) -> int32 (nq,)."""
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    nq, nprobe = probes.shape
    p_d = torch.from_numpy(probes.copy()).cuda()
    out = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    _call("GammaKTestExtractProbe0", nq, nprobe, _p(p_d, torch.int64),
          _p(out))
    return out.cpu().numpy()


# ------------------------------------------------------------ BINARYIVF
def _words_dev(bytes_u8):
    """host uint8 (n, 4*W) -> device int32 (n, W) with the same bytes"""
    a = np.ascontiguousarray(bytes_u8, dtype=np.uint8)
    assert a.ndim == 2 and a.shape[1] % 4 == 0
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def hamming_matrix(Q, B):
    """gk::hamming_matrix on host uint8 arrays Q (nq, d/8), B (n, d/8),
    d % 32 == 0 -> float32 (nq, n) numpy."""
    q_d, b_d = _words_dev(Q), _words_dev(B)
    nq, W = q_d.shape
    n = b_d.shape[0]
    assert b_d.shape[1] == W
    out = torch.full((nq, n), float("nan"), dtype=torch.float32,
                     device="cuda")
    _call("GammaKTestHammingMatrix", _p(q_d, torch.int32), nq,
          _p(b_d, torch.int32), n, W, _p(out))
    return out.cpu().numpy()


def _kill_dev(kill_flag):
    """the kill_flag argument of binivf_scan / rabitq_scan: False or None
    passes NULL, True a device int left at 0, an int (0 or 1) a device int
    holding that value (1 = a flag raised before the launch)."""
    if kill_flag is None or kill_flag is False:
        return None
    return torch.full((1,), 0 if kill_flag is True else int(kill_flag),
                      dtype=torch.int32, device="cuda")


def binivf_scan(lists, probes, queries, S, k2, bitmap=None, kill_flag=False):
    """One gk::binivf_scan launch on host arrays. lists: one (ids uint32
    (n,), codes uint8 (n, d/8)) per inverted list (n = 0 is legal), each
    array in its own device allocation; probes int64 (nq, nprobe) may hold
    -1 and ids >= nlist; queries uint8 (nq, d/8); bitmap: optional uint32
    words; kill_flag: see _kill_dev.
    Returns (keys uint64 (nq, S, k2), dists, ids): the raw partial rows
    and their gk::sort_rows merge to the top-k2 (-1 / -1 padded; None,
    None where S * k2 exceeds what sort_rows takes)."""
    q_d = _words_dev(queries)
    nq, W = q_d.shape
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    nprobe = probes.shape[1]
    assert probes.shape == (nq, nprobe)
    pr_d = torch.from_numpy(probes.copy()).cuda()
    keep, rows = [], []
    for ids, codes in lists:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = ids.shape[0]
        codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(n, 4 * W)
        t = [torch.from_numpy(ids.view(np.int32).copy()).cuda(),
             _words_dev(codes)]
        keep += t
        rows.append([x.data_ptr() if n else 0 for x in t] + [0, n])
    bk_d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).cuda()
    bm_d = None if bitmap is None else bitmap_to_dev(bitmap)
    kf_d = _kill_dev(kill_flag)
    keys = torch.full((nq, S, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                      device="cuda")
    _call("GammaKTestBinivfScan", nq, S, W, nprobe, k2,
          _p(q_d, torch.int32), _p(bk_d, torch.int64), len(lists),
          _p(pr_d, torch.int64), _p(bm_d, torch.int32),
          _p(keys, torch.int64), _p(kf_d, torch.int32))
    if S * k2 > 2048:  # beyond gk::sort_rows (the engine keeps S*k2 <= 2048)
        return keys_to_np(keys), None, None
    od, oi = sort_rows(keys.reshape(nq, S * k2), k2, False)
    return keys_to_np(keys), od.cpu().numpy(), oi.cpu().numpy()


def hamming_flat_scan(queries, base, seg_shift, k2, bitmap=None):
    """gk::hamming_flat_scan over host uint8 base (n, d/8) split into
    separately allocated segments of 1 << seg_shift rows; queries uint8
    (nq, d/8) -> keys uint64 (nq, k2)."""
    q_d = _words_dev(queries)
    nq, W = q_d.shape
    base = np.ascontiguousarray(base, dtype=np.uint8)
    n = base.shape[0]
    step = 1 << seg_shift
    segs = [_words_dev(base[i:i + step]) for i in range(0, n, step)]
    table = torch.tensor([t.data_ptr() for t in segs],
                         dtype=torch.int64).cuda()
    bm_d = None if bitmap is None else bitmap_to_dev(bitmap)
    out = torch.full((nq, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                     device="cuda")
    _call("GammaKTestHammingFlatScan", nq, n, W, k2, _p(q_d, torch.int32),
          _p(table), seg_shift, _p(bm_d, torch.int32), _p(out))
    return keys_to_np(out)


# ------------------------------------------------------------ IVFRABITQ
def rabitq_encode(x, asg, centroids, ip):
    """One gk::rabitq_encode launch on host arrays: x float32 (n, d), asg
    int32 (n,) list numbers, centroids float32 (nlist, d), d % 32 == 0 ->
    (entries uint8 (n, d/8 + 8), svals float32 (n,)) numpy. Outputs are
    pre-filled (0xEE / nan) so an unwritten byte is visible."""
    f32 = lambda a: torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a, dtype=np.float32).copy()).cuda()
    x_d, c_d = f32(x), f32(centroids)
    n, d = x_d.shape
    nlist = c_d.shape[0]
    assert c_d.shape == (nlist, d) and d % 32 == 0
    a_d = torch.from_numpy(
        np.ascontiguousarray(asg, dtype=np.int32).copy()).cuda()
    assert a_d.shape == (n,)
    ent = torch.full((n, d // 8 + 8), 0xEE, dtype=torch.uint8, device="cuda")
    sv = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    _call("GammaKTestRabitqEncode", n, d, _p(x_d), _p(a_d, torch.int32), 0,
          nlist, _p(c_d), int(bool(ip)), _p(ent), _p(sv))
    return ent.cpu().numpy(), sv.cpu().numpy()


def rabitq_scan(lists, probes, queries, centroids, S, k2, ip, bitmap=None,
                kill_flag=False):
    """One gk::rabitq_scan launch on host arrays. lists: one (ids uint32
    (n,), entries uint8 (n, d/8 + 8), svals float32 (n,)) per inverted list
    (n = 0 is legal), each array in its own device allocation; probes int64
    (nq, nprobe) may hold -1 and ids >= nlist; queries float32 (nq, d);
    centroids float32 (nlist, d); bitmap: optional uint32 words; kill_flag:
    see _kill_dev.
    Returns (keys uint64 (nq, S, k2), scores, ids): the raw partial rows
    and their gk::sort_rows merge to the top-k2 (-1 / -1 padded)."""
    f32 = lambda a: torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a, dtype=np.float32).copy()).cuda()
    q_d, c_d = f32(queries), f32(centroids)
    nq, d = q_d.shape
    nlist = len(lists)
    assert c_d.shape == (nlist, d) and d % 32 == 0
    assert S * k2 <= 2048
    cs = d // 8 + 8
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    nprobe = probes.shape[1]
    assert probes.shape == (nq, nprobe)
    pr_d = torch.from_numpy(probes.copy()).cuda()
    keep, rows = [], []
    for ids, ent, svals in lists:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n = ids.shape[0]
        ent = np.ascontiguousarray(ent, dtype=np.uint8).reshape(n, cs)
        svals = np.ascontiguousarray(svals, dtype=np.float32)
        assert svals.shape == (n,)
        t = [torch.from_numpy(ids.view(np.int32).copy()).cuda(),
             _words_dev(ent), torch.from_numpy(svals.copy()).cuda()]
        keep += t
        rows.append([x.data_ptr() if n else 0 for x in t] + [n])
    bk_d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).cuda()
    bm_d = None if bitmap is None else bitmap_to_dev(bitmap)
    kf_d = _kill_dev(kill_flag)
    keys = torch.full((nq, S, k2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                      device="cuda")
    _call("GammaKTestRabitqScan", nq, S, d, nprobe, k2, _p(q_d), _p(c_d),
          _p(bk_d, torch.int64), nlist, _p(pr_d, torch.int64),
          _p(bm_d, torch.int32), int(bool(ip)), _p(keys, torch.int64),
          _p(kf_d, torch.int32))
    od, oi = sort_rows(keys.reshape(nq, S * k2), k2, ip)
    return keys_to_np(keys), od.cpu().numpy(), oi.cpu().numpy()
