/*
 * gamma_bench.h — auxiliary (non-reference) entry points of libgamma.so.
 *
 * These symbols are NOT part of the reference C ABI (include/gamma_api.h);
 * they exist for the test/bench harness only:
 *  - bulk ingest that is semantically equivalent to a loop of
 *    AddOrUpdateDoc (reference: gamma_api.h:52) without per-doc FlatBuffers
 *    marshalling, so a 10M-vector index can be built in seconds;
 *  - a raw batched search equal to the compute path behind Search
 *    (reference: gamma_api.cc:175 -> engine.cc:248 -> vector_manager.cc:851)
 *    without protobuf marshalling, so the bench can time the hot path with
 *    queries already resident in HBM (the protobuf-inclusive rate is
 *    reported separately in DESIGN.md);
 *  - layered debug hooks used by the GPU parity tests to pin each stage of
 *    the IVFPQ pipeline against the CPU oracle.
 */

#ifndef GAMMA_BENCH_H_
#define GAMMA_BENCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bulk-add n vectors (row-major float32 n*d) for vector field `field`.
 * Docids are assigned sequentially from the current max docid; the i-th
 * vector's primary key is its docid rendered as a decimal string.
 * Returns 0 on success. */
int GammaBulkAdd(void *engine, const char *field, int field_len, int n,
                 const float *vecs);

/* Batched search on the single vector index of `engine`.
 * xq: nq*d float32 (host). k results per query.
 * nprobe<=0 -> index default. rerank>0 -> exact re-rank of `rerank`
 * candidates (reference recall_num, ivfpq.cc:675-726).
 * metric: 0 = engine default, 1 = L2, 2 = InnerProduct.
 * out_dists: nq*k float32; out_ids: nq*k int64 (-1 padded).
 * Returns 0 ok, -2 killed. */
int GammaRawSearch(void *engine, int nq, const float *xq, int k, int nprobe,
                   int rerank, int metric, float *out_dists,
                   int64_t *out_ids);

/* Upload nq*d queries once into HBM; GammaRawSearchCached then times the
 * hot path with inputs already device-resident (bench contract). */
int GammaCacheQueries(void *engine, int nq, const float *xq);
int GammaRawSearchCached(void *engine, int nq, int k, int nprobe,
                         int rerank, int metric, float *out_dists,
                         int64_t *out_ids);

/* Debug: run only the coarse-assign stage (quantizer->search equivalent,
 * reference ivfpq.cc:595): top-nprobe centroids per query. */
int GammaDebugCoarseAssign(void *engine, int nq, const float *xq, int nprobe,
                           int64_t *out_lists, float *out_dists);

/* Debug: copy the trained model to host: centroids (nlist*d), pq codebooks
 * (M*ksub*dsub, ksub = 2^nbits_per_idx: 256 at 8 bits, 16 at 4 bits).
 * Buffers may be NULL to skip. */
int GammaDebugGetModel(void *engine, float *centroids, float *codebooks);
/* OPQ debug hooks (oracle parity chains on the engine's own R and its
 * GPU rotation so downstream ADC stays bit-exact):
 * GetOPQ copies the d*d row-major rotation; ApplyOPQ returns the
 * engine-rotated queries (nq*d in, nq*d out). -1 if no OPQ. */
int GammaDebugGetOPQ(void *engine, float *R);
int GammaDebugApplyOPQ(void *engine, const float *xq, int nq, float *out);

/* Debug: fetch the contents of inverted list `list_no`: returns size, and
 * copies ids (int64, with bit-63 delete marks preserved, reference
 * realtime_mem_data.h:26) and codes (size*code_size u8) if non-NULL.
 * code_size = M*nbits_per_idx/8. At 8 bits byte m is sub-quantizer m; at
 * 4 bits entries are packed, byte b = sub-quantizer 2b in bits 0-3 and
 * 2b+1 in bits 4-7 (the same layout as the device buckets and the dump). */
int64_t GammaDebugGetList(void *engine, int64_t list_no, int64_t *ids,
                          uint8_t *codes);

/* Number of indexed vectors / engine docs. */
int64_t GammaDebugNumDocs(void *engine);

/* Timing of the last GammaRawSearch, in microseconds, split by stage:
 * [0]=H2D, [1]=coarse assign+select, [2]=list scan (the dominant kernel),
 * [3]=rerank+merge, [4]=D2H, [5]=total wall. Returns 0.
 * Where the scan kernel re-ranked and selected the final top-k itself
 * (below), [2] covers that fused kernel and [3] is ~0. */
int GammaLastSearchTiming(void *engine, double *us6);

/* Debug: 1 if the last GammaRawSearch[Cached] ran the exact re-rank and
 * the final top-k inside the IVFPQ scan kernel (8-bit resident table,
 * one workgroup per query, rerank > 0, GAMMA_FUSE_RERANK not 0), 0 if
 * gk::rerank / gk::sort_rows ran as kernels of their own. */
int GammaDebugLastSearchFused(void *engine);

/* Compact deleted entries out of the inverted lists (the reference does
 * this inside Update only — realtime_mem_data.cc:347-370 CompactIfNeed —
 * and has no C ABI call for it). Every bucket of every vector field's
 * index whose counted dead entries reach min_ratio of its size is
 * rewritten without them, order preserved, capacity unchanged;
 * min_ratio <= 0 means every bucket with at least one dead entry. Takes
 * the engine's write lock. stats2 (may be NULL), for this call:
 * [0] = buckets compacted, [1] = entries removed. Returns 0 on success.
 * AddOrUpdateDoc of an existing key runs the same with min_ratio 0.3. */
int GammaCompact(void *engine, float min_ratio, int64_t *stats2);
/* Lifetime totals since the index was created or loaded: [0] = buckets
 * compacted, [1] = entries removed, and [2] = dead (delete-marked)
 * entries currently counted in the lists. Summed over vector fields. */
int GammaCompactStats(void *engine, int64_t *stats3);

/* ---- BINARYIVF tables (index_type "BINARYIVF", dimension d in bits,
 * d % 32 == 0). Vectors and queries are d/8 bytes each, bit i of a vector
 * = (byte[i>>3] >> (i&7)) & 1; scores are Hamming distances. ----
 * GammaBulkAddBinary / GammaRawSearchBinary: GammaBulkAdd / GammaRawSearch
 * on n*d/8 (nq*d/8) bytes; rerank and metric do not apply.
 * GammaDebugCoarseAssignBinary: top-nprobe centroids by (Hamming, list).
 * GammaDebugGetBinaryCentroids: nlist*d/8 bytes of binarised centroids.
 * GammaDebugGetList serves the lists with code_size = d/8. */
int GammaBulkAddBinary(void *engine, const char *field, int field_len, int n,
                       const uint8_t *vecs);
int GammaRawSearchBinary(void *engine, int nq, const uint8_t *xq, int k,
                         int nprobe, int brute, float *out_dists,
                         int64_t *out_ids);
int GammaDebugCoarseAssignBinary(void *engine, int nq, const uint8_t *xq,
                                 int nprobe, int64_t *out_lists,
                                 float *out_dists);
int GammaDebugGetBinaryCentroids(void *engine, uint8_t *centroids);

/* ---- kernel test hooks (vearch_amd/csrc/ktest.cpp) ----
 * One entry per gk:: host function of csrc/kernels.h, same arguments
 * minus the stream, bool -> int. EVERY pointer is a DEVICE pointer. Each
 * hook launches on the null stream, synchronises the device and returns
 * the first non-zero hipError_t (0 = ok). Test-only: nothing on the
 * product path calls them. See kernels.h for each kernel's contract
 * (d % 4 == 0, k2 <= 1024, select_rows_full ncols <= 8192, sort_rows
 * ncand <= 2048, ksub in {16, 256}). */
int GammaKTestDotsMfma(const float *Q, int nq, const float *B, int64_t n,
                       int d, float *out);
int GammaKTestSelectFromDots(int nq, int64_t ncols, int64_t col_base,
                             int64_t ld, const float *dots,
                             const float *qnorms, const float *bnorms,
                             int l2, int ip_order, const uint32_t *bitmap,
                             int k2, uint64_t *state_keys, int seeded);
int GammaKTestSelectRowsFull(int nq, int ncols, int64_t ld,
                             const float *dots, const float *qnorms,
                             const float *bnorms, int l2, int ip_order,
                             int k2, float *out_dists, int64_t *out_ids);
int GammaKTestArgminRows(int64_t nrows, int ncols, const float *dots,
                         const float *qnorms, const float *bnorms, int l2,
                         int32_t *out);
/* segs: device array of n_segs device pointers (segment s holds vectors
 * [s << seg_shift, (s + 1) << seg_shift)) */
int GammaKTestRerank(int nq, int ncand, int d, const float *queries,
                     const float *const *segs, int n_segs, int seg_shift,
                     int ip, const uint64_t *keys_in, uint64_t *keys_out);
int GammaKTestSortRows(int nq, int ncand, int k, const uint64_t *keys, int ip,
                       float *out_dists, int64_t *out_ids);
int GammaKTestUnpackKeys(int64_t n, const uint64_t *keys, int ip,
                         float *out_dists, int64_t *out_ids);
int GammaKTestPqEncode(int64_t n, int d, int M, int ksub, const float *x,
                       const float *codebooks, uint8_t *codes);
int GammaKTestPqEncodePack4(int64_t n, int d, int M, const float *x,
                            const float *codebooks, uint8_t *codes);
int GammaKTestFlatStreamScan(int nq, int64_t n, int d, int k2,
                             const float *queries, const float *const *segs,
                             int seg_shift, const uint32_t *bitmap, int ip,
                             uint64_t *out_keys);
/* segs_dev: device array of nseg GammaCompactSeg (csrc/kernels.h), i.e.
 * 8 x 8-byte fields per segment: ids_src, data_src, svals_src (or 0),
 * size, ids_dst, data_dst, svals_dst (or 0), kept_out. */
int GammaKTestBucketCompact(int nseg, const void *segs_dev,
                            const uint32_t *bitmap, int entry_bytes);
/* L2 query tables: atab (nq x M x ksub) from gk::pq_tables_a; cwn
 * (M x ksub codeword norms) from gk::pq_cwn; PqLutL2 writes the table the
 * 8-bit fast scan's in-kernel builder leaves in LDS (same shape as atab,
 * bit-identical to it). */
int GammaKTestPqTablesA(int nq, int d, int M, int ksub, const float *queries,
                        const float *codebooks, float *atab);
int GammaKTestPqCwn(int M, int ksub, int dsub, const float *codebooks,
                    float *cwn);
int GammaKTestPqLutL2(int nq, int d, int M, int ksub, const float *queries,
                      const float *codebooks, const float *cwn, float *out);
/* gk::ivfpq_scan. buckets_dev: device array of nlist GammaBucketDev
 * (csrc/kernels.h), i.e. 4 x 8-byte fields per list: ids (u32, bit 31 =
 * deleted), codes, svals, size. out_keys: nq x S x k2. atab / cwn: see
 * kernels.h (either may be 0 when the launch does not read it); bitmap,
 * kill_flag, qmap may be 0. */
int GammaKTestIvfpqScan(int nq, int S, int d, int M, int ksub, int nprobe,
                        int k2, const float *queries, const float *centroids,
                        const float *codebooks, const float *atab,
                        const float *cwn, const float *probe_dists,
                        const void *buckets_dev, int nlist,
                        const int64_t *probes, const uint32_t *bitmap, int ip,
                        uint64_t *out_keys, const int *kill_flag,
                        const int32_t *qmap);
/* gk::ivfpq_scan with its re-rank block (kernels.h GammaScanRerank):
 * with_rr != 0 passes {rr_queries (raw-space, nq x d), segs (device array
 * of n_segs device pointers, 1 << seg_shift rows each), k, out_dists /
 * out_ids (nq x k)} and the scan workgroups re-rank their top-k2 and write
 * the final top-k themselves; out_keys is then not written. with_rr == 0
 * passes no block: GammaKTestIvfpqScan. A launch that cannot fuse (S > 1,
 * 4-bit, wide, ...) with the block set returns hipErrorInvalidValue and
 * launches nothing. IvfpqScanCanFuseRerank is the launcher's predicate
 * (1 / 0) under the current GAMMA_FUSE_RERANK. */
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
                              int64_t *out_ids);
int GammaKTestIvfpqScanCanFuseRerank(int d, int M, int ksub, int k2, int S);
/* The sliced-table scan (k_ivfpq_scan_wide, kernels.h "Wide tables") reads
 * atab for both metrics: PqTablesIp is gk::pq_tables_ip, the inner-product
 * table (nq x M x 256). IvfpqWideInfo: out5 = {sub-quantizers per table
 * slice, entries per tile at the current GAMMA_SCAN_BS, 1 if a launch of
 * this (d, M, ksub, k2) takes the sliced kernel else 0, 1 if an L2 launch
 * reads atab (what the engine builds a table for), the same for inner
 * product}. */
int GammaKTestPqTablesIp(int nq, int d, int M, const float *queries,
                         const float *codebooks, float *out);
int GammaKTestIvfpqWideInfo(int d, int M, int ksub, int k2, int *out5);
/* gk::ivfflat_scan: buckets_dev as for GammaKTestIvfpqScan with `data` =
 * d fp32 per entry and svals 0; out_keys nq x k2; bitmap may be 0. */
int GammaKTestIvfflatScan(int nq, int d, int nprobe, int k2,
                          const float *queries, const void *buckets_dev,
                          int nlist, const int64_t *probes,
                          const uint32_t *bitmap, int ip, uint64_t *out_keys);
/* Ingest and table kernels. PqTablesB: btab nlist x M x ksub. PqSterm:
 * codes are bucket-format entries (M bytes, or M/2 packed bytes at ksub =
 * 16), asg may be 0 (every vector in list asg_const). PqStermBuckets /
 * RabitqSvalBuckets: bks_dev is nlist GammaBucketDev whose svals are
 * written (a bucket with svals 0 or size 0 is skipped). BucketScatter:
 * segs_dev is nseg GammaScatterSeg (csrc/kernels.h), i.e. 5 x 8-byte fields
 * per segment: ids_dst, data_dst, sval_dst (or 0), src_start, count;
 * svals_src may be 0. */
int GammaKTestPqTablesB(int d, int M, int ksub, int nlist,
                        const float *centroids, const float *codebooks,
                        float *btab);
int GammaKTestPqSterm(int64_t n, int M, int ksub, int nlist,
                      const uint8_t *codes, const int32_t *asg, int asg_const,
                      const float *btab, float *out);
int GammaKTestPqStermBuckets(int nlist, int M, int ksub, const void *bks_dev,
                             const float *btab);
int GammaKTestBucketScatter(int nseg, const void *segs_dev,
                            const uint32_t *ids_src, const uint8_t *data_src,
                            const float *svals_src, int entry_bytes);
int GammaKTestResiduals(int64_t n, int d, const float *x,
                        const float *centroids, const int32_t *assign,
                        float *out);
int GammaKTestRowNorms(const float *v, int64_t n, int d, float *norms);
int GammaKTestExtractProbe0(int nq, int nprobe, const int64_t *probes,
                            int32_t *out);

/* BINARYIVF kernels (W = d/32 u32 words per vector, LSB-first bits):
 * HammingMatrix out[i*n+j] = popcount(Q_i xor B_j) as f32; BinivfScan has
 * GammaKTestIvfpqScan's bucket / probe / key layout with W words per entry
 * and svals unused; HammingFlatScan walks a segment table of u32 words. */
int GammaKTestHammingMatrix(const uint32_t *Q, int nq, const uint32_t *B,
                            int64_t n, int W, float *out);
int GammaKTestBinivfScan(int nq, int S, int W, int nprobe, int k2,
                         const uint32_t *queries, const void *buckets_dev,
                         int nlist, const int64_t *probes,
                         const uint32_t *bitmap, uint64_t *out_keys,
                         const int *kill_flag);
int GammaKTestHammingFlatScan(int nq, int64_t n, int W, int k2,
                              const uint32_t *queries,
                              const uint32_t *const *segs, int seg_shift,
                              const uint32_t *bitmap, uint64_t *out_keys);

/* IVFRABITQ kernels (index_type "IVFRABITQ", nb_bits = 1; d % 32 == 0,
 * 32 <= d <= 4096). An entry is d/8 + 8 bytes: the sign bits (bit j of a
 * vector = (byte[j>>3] >> (j&7)) & 1), then the factors A and Mul as
 * little-endian fp32 — GammaDebugGetList serves the lists in this form,
 * code_size = d/8 + 8. RabitqEncode: x (n x d), asg (n list numbers; 0 =
 * every vector in list asg_const), centroids (nlist x d) -> entries
 * (n x (d/8 + 8) bytes) and svals (n floats, sum of the centroid's
 * coordinates under the set bits). RabitqScan has GammaKTestIvfpqScan's
 * bucket / probe / key layout with such entries and svals. */
int GammaKTestRabitqEncode(int64_t n, int d, const float *x,
                           const int32_t *asg, int asg_const, int nlist,
                           const float *centroids, int ip, uint8_t *entries,
                           float *svals);
int GammaKTestRabitqScan(int nq, int S, int d, int nprobe, int k2,
                         const float *queries, const float *centroids,
                         const void *buckets_dev, int nlist,
                         const int64_t *probes, const uint32_t *bitmap,
                         int ip, uint64_t *out_keys, const int *kill_flag);
int GammaKTestRabitqSvalBuckets(int nlist, int d, const void *bks_dev,
                                const float *centroids);
/* gk::coarse_select, the seed-filtered coarse assign (kernels.h): dots is
 * nq x nlist floats of scratch, cand nq x cap keys, cand_cnt nq + 1 ints
 * (per-query candidate counters, then the overflow flag), sel_keys the
 * nq x nprobe result. n1 / cap <= 0 take the knobs' values. Where
 * CoarseCanFilter is 0 the plain full-width pair runs and cand / cand_cnt
 * stay as they were. CoarseCanFilter returns gk::coarse_can_filter (1 / 0)
 * under the current GAMMA_FUSE_COARSE; knobs2 (optional, host) receives
 * {GAMMA_COARSE_SEED_COLS, GAMMA_COARSE_CAND_CAP} as read. */
int GammaKTestCoarseSelect(const float *Q, int nq, const float *B,
                           int64_t nlist, int d, const float *qnorms,
                           const float *bnorms, int l2, int ip_order,
                           int nprobe, int n1, int cap, float *dots,
                           uint64_t *cand, int *cand_cnt,
                           uint64_t *sel_keys);
int GammaKTestCoarseCanFilter(int nq, int64_t nlist, int d, int nprobe,
                              int n1, int *knobs2);

#ifdef __cplusplus
}
#endif

#endif /* GAMMA_BENCH_H_ */
