/*
 * ktest.cpp — kernel test hooks (include/gamma_bench.h): one plain C
 * entry per gk:: host function so the test suite can drive a single
 * kernel on tiny device arrays. Every pointer is a DEVICE pointer. Each
 * hook launches on the null stream, synchronises the device and returns
 * the first non-zero hipError_t (0 = ok). No logic beyond that lives
 * here; the product path never calls these.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gamma_bench.h"
#include "kernels.h"

static int kt_done(hipError_t launch) {
  hipError_t sync = hipDeviceSynchronize();
  return (int)(launch != hipSuccess ? launch : sync);
}

extern "C" {

int GammaKTestDotsMfma(const float *Q, int nq, const float *B, int64_t n,
                       int d, float *out) {
  return kt_done(gk::dots_mfma(nullptr, Q, nq, B, n, d, out));
}

int GammaKTestSelectFromDots(int nq, int64_t ncols, int64_t col_base,
                             int64_t ld, const float *dots,
                             const float *qnorms, const float *bnorms,
                             int l2, int ip_order, const uint32_t *bitmap,
                             int k2, uint64_t *state_keys, int seeded) {
  return kt_done(gk::select_from_dots(nullptr, nq, ncols, col_base, ld, dots,
                                      qnorms, bnorms, l2 != 0, ip_order != 0,
                                      bitmap, k2, state_keys, seeded != 0));
}

int GammaKTestSelectRowsFull(int nq, int ncols, int64_t ld,
                             const float *dots, const float *qnorms,
                             const float *bnorms, int l2, int ip_order,
                             int k2, float *out_dists, int64_t *out_ids) {
  return kt_done(gk::select_rows_full(nullptr, nq, ncols, ld, dots, qnorms,
                                      bnorms, l2 != 0, ip_order != 0, k2,
                                      out_dists, out_ids));
}

int GammaKTestArgminRows(int64_t nrows, int ncols, const float *dots,
                         const float *qnorms, const float *bnorms, int l2,
                         int32_t *out) {
  return kt_done(gk::argmin_rows(nullptr, nrows, ncols, dots, qnorms, bnorms,
                                 l2 != 0, out));
}

int GammaKTestRerank(int nq, int ncand, int d, const float *queries,
                     const float *const *segs, int n_segs, int seg_shift,
                     int ip, const uint64_t *keys_in, uint64_t *keys_out) {
  return kt_done(gk::rerank(nullptr, nq, ncand, d, queries, segs, n_segs,
                            seg_shift, ip != 0, keys_in, keys_out));
}

int GammaKTestSortRows(int nq, int ncand, int k, const uint64_t *keys, int ip,
                       float *out_dists, int64_t *out_ids) {
  return kt_done(gk::sort_rows(nullptr, nq, ncand, k, keys, ip != 0,
                               out_dists, out_ids));
}

int GammaKTestUnpackKeys(int64_t n, const uint64_t *keys, int ip,
                         float *out_dists, int64_t *out_ids) {
  return kt_done(gk::unpack_keys(nullptr, n, keys, ip != 0, out_dists,
                                 out_ids));
}

int GammaKTestPqEncode(int64_t n, int d, int M, int ksub, const float *x,
                       const float *codebooks, uint8_t *codes) {
  return kt_done(gk::pq_encode(nullptr, n, d, M, ksub, x, codebooks, codes));
}

int GammaKTestPqEncodePack4(int64_t n, int d, int M, const float *x,
                            const float *codebooks, uint8_t *codes) {
  return kt_done(gk::pq_encode_pack4(nullptr, n, d, M, x, codebooks, codes));
}

int GammaKTestFlatStreamScan(int nq, int64_t n, int d, int k2,
                             const float *queries, const float *const *segs,
                             int seg_shift, const uint32_t *bitmap, int ip,
                             uint64_t *out_keys) {
  return kt_done(gk::flat_stream_scan(nullptr, nq, n, d, k2, queries, segs,
                                      seg_shift, bitmap, ip != 0, out_keys));
}

int GammaKTestBucketCompact(int nseg, const void *segs_dev,
                            const uint32_t *bitmap, int entry_bytes) {
  return kt_done(gk::bucket_compact(nullptr, nseg,
                                    (const GammaCompactSeg *)segs_dev, bitmap,
                                    entry_bytes));
}

int GammaKTestPqTablesA(int nq, int d, int M, int ksub, const float *queries,
                        const float *codebooks, float *atab) {
  return kt_done(gk::pq_tables_a(nullptr, nq, d, M, ksub, queries, codebooks,
                                 atab));
}

int GammaKTestPqCwn(int M, int ksub, int dsub, const float *codebooks,
                    float *cwn) {
  return kt_done(gk::pq_cwn(nullptr, M, ksub, dsub, codebooks, cwn));
}

int GammaKTestPqLutL2(int nq, int d, int M, int ksub, const float *queries,
                      const float *codebooks, const float *cwn, float *out) {
  return kt_done(gk::pq_lut_l2_dump(nullptr, nq, d, M, ksub, queries,
                                    codebooks, cwn, out));
}

int GammaKTestIvfpqScan(int nq, int S, int d, int M, int ksub, int nprobe,
                        int k2, const float *queries, const float *centroids,
                        const float *codebooks, const float *atab,
                        const float *cwn, const float *probe_dists,
                        const void *buckets_dev, int nlist,
                        const int64_t *probes, const uint32_t *bitmap, int ip,
                        uint64_t *out_keys, const int *kill_flag,
                        const int32_t *qmap) {
  static_assert(sizeof(GammaBucketDev) == 32, "4 x 8-byte fields");
  return kt_done(gk::ivfpq_scan(nullptr, nq, S, d, M, ksub, nprobe, k2,
                                queries, centroids, codebooks, atab, cwn,
                                probe_dists,
                                (const GammaBucketDev *)buckets_dev, nlist,
                                probes, bitmap, ip != 0, out_keys, kill_flag,
                                qmap));
}

int GammaKTestIvfpqScanRerank(int nq, int S, int d, int M, int ksub,
                              int nprobe, int k2, const float *queries,
                              const float *centroids, const float *codebooks,
                              const float *atab, const float *cwn,
                              const float *probe_dists,
                              const void *buckets_dev, int nlist,
                              const int64_t *probes, const uint32_t *bitmap,
                              int ip, uint64_t *out_keys,
                              const int *kill_flag, const int32_t *qmap,
                              int with_rr, const float *rr_queries,
                              const float *const *segs, int n_segs,
                              int seg_shift, int k, float *out_dists,
                              int64_t *out_ids) {
  const GammaScanRerank rr = {rr_queries, segs,      n_segs, seg_shift,
                              k,          out_dists, out_ids};
  return kt_done(gk::ivfpq_scan(nullptr, nq, S, d, M, ksub, nprobe, k2,
                                queries, centroids, codebooks, atab, cwn,
                                probe_dists,
                                (const GammaBucketDev *)buckets_dev, nlist,
                                probes, bitmap, ip != 0, out_keys, kill_flag,
                                qmap, with_rr ? &rr : nullptr));
}

int GammaKTestIvfpqScanCanFuseRerank(int d, int M, int ksub, int k2, int S) {
  return gk::ivfpq_scan_can_fuse_rerank(d, M, ksub, k2, S) ? 1 : 0;
}

int GammaKTestPqTablesIp(int nq, int d, int M, const float *queries,
                         const float *codebooks, float *out) {
  return kt_done(gk::pq_tables_ip(nullptr, nq, d, M, queries, codebooks, out));
}

int GammaKTestIvfpqWideInfo(int d, int M, int ksub, int k2, int *out5) {
  out5[0] = gk::IVFPQ_WIDE_MS;
  out5[1] = gk::ivfpq_wide_tile();
  out5[2] = gk::ivfpq_scan_is_wide(d, M, ksub, k2) ? 1 : 0;
  out5[3] = gk::ivfpq_scan_reads_table(d, M, ksub, k2, false) ? 1 : 0;
  out5[4] = gk::ivfpq_scan_reads_table(d, M, ksub, k2, true) ? 1 : 0;
  return 0;
}

int GammaKTestIvfflatScan(int nq, int d, int nprobe, int k2,
                          const float *queries, const void *buckets_dev,
                          int nlist, const int64_t *probes,
                          const uint32_t *bitmap, int ip,
                          uint64_t *out_keys) {
  return kt_done(gk::ivfflat_scan(nullptr, nq, d, nprobe, k2, queries,
                                  (const GammaBucketDev *)buckets_dev, nlist,
                                  probes, bitmap, ip != 0, out_keys));
}

int GammaKTestPqTablesB(int d, int M, int ksub, int nlist,
                        const float *centroids, const float *codebooks,
                        float *btab) {
  return kt_done(gk::pq_tables_b(nullptr, d, M, ksub, nlist, centroids,
                                 codebooks, btab));
}

int GammaKTestPqSterm(int64_t n, int M, int ksub, int nlist,
                      const uint8_t *codes, const int32_t *asg, int asg_const,
                      const float *btab, float *out) {
  return kt_done(gk::pq_sterm(nullptr, n, M, ksub, nlist, codes, asg,
                              asg_const, btab, out));
}

int GammaKTestPqStermBuckets(int nlist, int M, int ksub, const void *bks_dev,
                             const float *btab) {
  return kt_done(gk::pq_sterm_buckets(nullptr, nlist, M, ksub,
                                      (const GammaBucketDev *)bks_dev, btab));
}

int GammaKTestBucketScatter(int nseg, const void *segs_dev,
                            const uint32_t *ids_src, const uint8_t *data_src,
                            const float *svals_src, int entry_bytes) {
  static_assert(sizeof(GammaScatterSeg) == 40, "5 x 8-byte fields");
  return kt_done(gk::bucket_scatter(nullptr, nseg,
                                    (const GammaScatterSeg *)segs_dev, ids_src,
                                    data_src, svals_src, entry_bytes));
}

int GammaKTestResiduals(int64_t n, int d, const float *x,
                        const float *centroids, const int32_t *assign,
                        float *out) {
  return kt_done(gk::residuals(nullptr, n, d, x, centroids, assign, out));
}

int GammaKTestRowNorms(const float *v, int64_t n, int d, float *norms) {
  return kt_done(gk::row_norms(nullptr, v, n, d, norms));
}

int GammaKTestExtractProbe0(int nq, int nprobe, const int64_t *probes,
                            int32_t *out) {
  return kt_done(gk::extract_probe0(nullptr, nq, nprobe, probes, out));
}

int GammaKTestHammingMatrix(const uint32_t *Q, int nq, const uint32_t *B,
                            int64_t n, int W, float *out) {
  return kt_done(gk::hamming_matrix(nullptr, Q, nq, B, n, W, out));
}

int GammaKTestBinivfScan(int nq, int S, int W, int nprobe, int k2,
                         const uint32_t *queries, const void *buckets_dev,
                         int nlist, const int64_t *probes,
                         const uint32_t *bitmap, uint64_t *out_keys,
                         const int *kill_flag) {
  return kt_done(gk::binivf_scan(nullptr, nq, S, W, nprobe, k2, queries,
                                 (const GammaBucketDev *)buckets_dev, nlist,
                                 probes, bitmap, out_keys, kill_flag));
}

int GammaKTestHammingFlatScan(int nq, int64_t n, int W, int k2,
                              const uint32_t *queries,
                              const uint32_t *const *segs, int seg_shift,
                              const uint32_t *bitmap, uint64_t *out_keys) {
  return kt_done(gk::hamming_flat_scan(nullptr, nq, n, W, k2, queries, segs,
                                       seg_shift, bitmap, out_keys));
}

int GammaKTestRabitqEncode(int64_t n, int d, const float *x,
                           const int32_t *asg, int asg_const, int nlist,
                           const float *centroids, int ip, uint8_t *entries,
                           float *svals) {
  return kt_done(gk::rabitq_encode(nullptr, n, d, x, asg, asg_const, nlist,
                                   centroids, ip != 0, entries, svals));
}

int GammaKTestRabitqScan(int nq, int S, int d, int nprobe, int k2,
                         const float *queries, const float *centroids,
                         const void *buckets_dev, int nlist,
                         const int64_t *probes, const uint32_t *bitmap,
                         int ip, uint64_t *out_keys, const int *kill_flag) {
  return kt_done(gk::rabitq_scan(nullptr, nq, S, d, nprobe, k2, queries,
                                 centroids,
                                 (const GammaBucketDev *)buckets_dev, nlist,
                                 probes, bitmap, ip != 0, out_keys,
                                 kill_flag));
}

int GammaKTestRabitqSvalBuckets(int nlist, int d, const void *bks_dev,
                                const float *centroids) {
  return kt_done(gk::rabitq_sval_buckets(nullptr, nlist, d,
                                         (const GammaBucketDev *)bks_dev,
                                         centroids));
}

int GammaKTestCoarseSelect(const float *Q, int nq, const float *B,
                           int64_t nlist, int d, const float *qnorms,
                           const float *bnorms, int l2, int ip_order,
                           int nprobe, int n1, int cap, float *dots,
                           uint64_t *cand, int *cand_cnt,
                           uint64_t *sel_keys) {
  return kt_done(gk::coarse_select(nullptr, Q, nq, B, nlist, d, qnorms,
                                   bnorms, l2 != 0, ip_order != 0, nprobe, n1,
                                   cap, dots, cand, cand_cnt, sel_keys));
}

int GammaKTestCoarseCanFilter(int nq, int64_t nlist, int d, int nprobe,
                              int n1, int *knobs2) {
  if (knobs2) {
    knobs2[0] = gk::coarse_seed_cols();
    knobs2[1] = gk::coarse_cand_cap();
  }
  return gk::coarse_can_filter(nq, nlist, d, nprobe, n1) ? 1 : 0;
}

} /* extern "C" */
