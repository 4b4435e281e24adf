/* kernels.h — host API of the gfx950 HIP kernels (kernels.hip). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

/* One IVF bucket as the device sees it (RT list storage, SURVEY §8 a7;
 * semantics of realtime_mem_data.cc:57-68: append-only SoA with a
 * per-entry delete mark). Device ids are compressed to u32 with bit 31
 * as the delete mark (docids < 2^31 per partition); every host-visible
 * surface (debug API, Dump format, oracle) keeps the reference's int64 +
 * bit-63 form — SURVEY §8d notes the 4-byte id option and the roofline
 * stays on the algorithmic 8-byte ids. For IVFPQ `data` is uint8 codes
 * (code_size per entry); for IVFFLAT fp32 vectors (d floats). */
struct GammaBucketDev {
  const uint32_t *ids;
  const void *data;
  /* IVFPQ only: per-entry S term, S_v = sum_m btab[ln][m][code_m]
   * (the list-dependent half of the decomposed ADC tables, folded into
   * one float per vector at encode time so the scan never touches the
   * B table — see kernels.h pq_sterm). Null for IVFFLAT. */
  const float *svals;
  long long size;
};

/* one bucket's slice of a bulk-ingest batch (gk::bucket_scatter):
 * copy `count` entries starting at src_start of the staged arrays into
 * this bucket's device arrays at the recorded append position */
struct GammaScatterSeg {
  uint32_t *ids_dst;
  uint8_t *data_dst;
  float *sval_dst; /* null for IVFFLAT */
  long long src_start;
  long long count;
};

/* one bucket of a compaction batch (gk::bucket_compact): the first
 * `size` entries of the *_src arrays are filtered into the *_dst arrays.
 * Source and destination are different allocations. data_src/data_dst
 * are aligned to the largest of 16/8/4/1 bytes that divides the entry
 * size (every hipMalloc'd bucket is). All fields are 8 bytes wide, so a
 * descriptor is 8 x int64 for callers that build it without this header. */
struct GammaCompactSeg {
  const uint32_t *ids_src;
  const uint8_t *data_src;
  const float *svals_src; /* null for IVFFLAT */
  long long size;
  uint32_t *ids_dst;
  uint8_t *data_dst;
  float *svals_dst; /* null for IVFFLAT */
  long long *kept_out; /* one count per segment */
};

/* re-rank block of gk::ivfpq_scan: with it the scan's workgroup re-ranks
 * its own top-k2 against the raw store and writes the final top-k itself
 * (what gk::rerank + gk::sort_rows do to out_keys). Rows are indexed by
 * the ORIGINAL query row, as out_keys is. */
struct GammaScanRerank {
  const float *queries;     /* raw-space queries, nq x d (under OPQ the
                             * scan's own `queries` are rotated ones) */
  const float *const *segs; /* raw-store segment table */
  int n_segs, seg_shift;
  int k;                    /* results per query, <= 2048 */
  float *out_dists;         /* nq x k; -1.0 where fewer than k exist */
  int64_t *out_ids;         /* nq x k; -1 there */
};

namespace gk {

/* Stable compaction of a batch of buckets in one launch, the mirror of
 * bucket_scatter (CompactBucket, realtime_mem_data.cc:94-146). Entry i of
 * a segment survives iff its id has bit 31 (the delete mark) clear and
 * `bitmap` (optional docid bitmap, u32 words) does not have bit id set.
 * Survivors keep their relative order and land at 0..kept-1 of ids_dst /
 * data_dst / svals_dst; *kept_out = kept; nothing at or beyond kept is
 * written. size == 0 is legal. entry_bytes may be any positive size. */
hipError_t bucket_compact(hipStream_t s, int nseg,
                          const GammaCompactSeg *segs_dev,
                          const uint32_t *bitmap, int entry_bytes);

/* Bulk bucket append: instead of 3 small hipMemcpys per bucket per
 * chunk (~100k calls per 64k-vector chunk at nlist=32k — the N=50M
 * build-time killer), the host stages the grouped chunk once and one
 * kernel scatters it into every bucket. */
hipError_t bucket_scatter(hipStream_t s, int nseg,
                          const GammaScatterSeg *segs_dev,
                          const uint32_t *ids_src,
                          const uint8_t *data_src,
                          const float *svals_src, int entry_bytes);

/* out[i*n+j] = dot(Q_i, B_j); f32 MFMA 16x16x4.
 * run_if (optional, device): the kernel returns at entry when *run_if is
 * 0. Only the tiled launch (nq >= 64, n >= 64) has this switch; with any
 * other shape a non-null run_if is hipErrorInvalidValue. */
hipError_t dots_mfma(hipStream_t s, const float *Q, int nq, const float *B,
                     int64_t n, int d, float *out,
                     const int *run_if = nullptr);

/* norms[i] = sum_j v[i][j]^2, canonical sequential fmaf. */
hipError_t row_norms(hipStream_t s, const float *v, int64_t n, int d,
                     float *norms);

/* Exact top-k2 select per row of a dots matrix.
 * dist = l2 ? (qn[q] + bn[col_base+c] - 2*dot) : dot; id = col_base + c.
 * bitmap: optional delete bitmap over global ids (u32 words).
 * state_keys (nq x k2 u64) is seeded from itself when `seeded`. */
hipError_t select_from_dots(hipStream_t s, int nq, int64_t ncols,
                            int64_t col_base, int64_t ld, const float *dots,
                            const float *qnorms, const float *bnorms,
                            bool l2, bool ip_order, const uint32_t *bitmap,
                            int k2, uint64_t *state_keys, bool seeded,
                            const int *run_if = nullptr);

/* Coarse assign without the nq x nlist round trip (DESIGN.md "Kernels"
 * (a2)): sel_keys (nq x nprobe u64, sorted) = exact top-nprobe of
 * select_from_dots over all nlist columns of Q x B^T, bit for bit.
 *   1. dots_mfma + select_from_dots on columns [0, n1): the seeds; the
 *      last seed key tau_q bounds row q's nprobe-th key from above.
 *   2. the tiled GEMM over [n1, nlist) with a filtering epilogue: a key
 *      below tau_q is appended to cand[q] (cap slots; cand_cnt[q] keeps
 *      counting past cap). Nothing else is written.
 *   3. a wave per query merges seeds and candidates.
 *   4. dots_mfma + select_from_dots on all columns, switched by the
 *      overflow flag cand_cnt[nq] that step 3 raises when a counter ran
 *      past cap: empty workgroups otherwise.
 * All on stream s, no host sync. dots: nq x nlist floats; cand: nq x cap
 * u64; cand_cnt: nq + 1 ints (counters, then the flag; zeroed here).
 * n1 <= 0 / cap <= 0 take GAMMA_COARSE_SEED_COLS (4096) /
 * GAMMA_COARSE_CAND_CAP (1024). Where coarse_can_filter is false this is
 * the plain full-width pair and cand / cand_cnt are not touched. */
hipError_t coarse_select(hipStream_t s, const float *Q, int nq,
                         const float *B, int64_t nlist, int d,
                         const float *qnorms, const float *bnorms, bool l2,
                         bool ip_order, int nprobe, int n1, int cap,
                         float *dots, uint64_t *cand, int *cand_cnt,
                         uint64_t *sel_keys);
/* nq >= 64, d % 4 == 0, nprobe <= 192 (the wave selector's range), n1 a
 * multiple of 128 with nprobe <= n1 and 2 * n1 <= nlist (n1 <= 0: the
 * knob). GAMMA_FUSE_COARSE=0, read per call, turns it off. The caller
 * keeps binary centroids and the full-sort branch away. */
bool coarse_can_filter(int nq, int64_t nlist, int d, int nprobe, int n1 = 0);
int coarse_seed_cols(); /* GAMMA_COARSE_SEED_COLS, default 4096 */
int coarse_cand_cap();  /* GAMMA_COARSE_CAND_CAP, default 1024 */

/* Full-sort row select for short rows (ncols <= 8192, no bitmap):
 * one workgroup bitonic-sorts the whole row of (dist,id) keys and emits
 * the top-k2 as (dists, ids) — used for the coarse top-nprobe
 * (quantizer->search, ivfpq.cc:595). Same key order as
 * select_from_dots. */
hipError_t select_rows_full(hipStream_t s, int nq, int ncols, int64_t ld,
                            const float *dots, const float *qnorms,
                            const float *bnorms, bool l2, bool ip_order,
                            int k2, float *out_dists, int64_t *out_ids);

/* argmin over each row (ties -> lowest col). out int32[nrows]. */
hipError_t argmin_rows(hipStream_t s, int64_t nrows, int ncols,
                       const float *dots, const float *qnorms,
                       const float *bnorms, bool l2, int32_t *out);

/* Decomposed ADC tables (use_precomputed_table=1 semantics,
 * gamma_index_ivfpq.h:254-262):
 *   btab[ln][m][j] = 2 * (c_ln,m . cw_mj)        (train-time)
 *   atab[q][m][j]  = fmaf(-2, q_m . cw, ||cw||^2) (per search batch)
 * Sequential-fmaf arithmetic matching oracle_pct1_*_table.
 * ksub = 256 (nbits_per_idx=8) or 16 (nbits_per_idx=4) here and in every
 * PQ entry point below; anything else is hipErrorInvalidValue. */
hipError_t pq_tables_b(hipStream_t s, int d, int M, int ksub, int nlist,
                       const float *centroids, const float *codebooks,
                       float *btab);
hipError_t pq_tables_a(hipStream_t s, int nq, int d, int M, int ksub,
                       const float *queries, const float *codebooks,
                       float *atab);
/* cwn[m][j] = ||cw_mj||^2 (M*ksub floats; dsub = d/M), the
 * query-independent term of atab with pq_tables_a's own fmaf chain.
 * Derived from the codebooks once per model; the 8-bit fast scan builds
 * its query table in LDS from it (see ivfpq_scan). */
hipError_t pq_cwn(hipStream_t s, int M, int ksub, int dsub,
                  const float *codebooks, float *cwn);
/* TEST HOOK: out[q][m][j] = the L2 table the fast scan's in-kernel
 * builder leaves in LDS for query q — bit-identical to pq_tables_a. */
hipError_t pq_lut_l2_dump(hipStream_t s, int nq, int d, int M, int ksub,
                          const float *queries, const float *codebooks,
                          const float *cwn, float *out);

/* Per-vector S term (encode/add/load time):
 *   out[i] = sum_m btab[asg_i][m][code_i[m]]   (plain adds, m order)
 * where asg_i = asg ? asg[i] : asg_const. Folding the list half of the
 * pct1 decomposition into one float per vector removes the per-(query,
 * list) B-table staging (nprobe x M x ksub floats per query) from the
 * scan: dis = coarse_dis + S_v + sum_m atab[q][m][code_m], which is
 * the same T = A + B sum grouped per vector — fp32-rounding-only
 * difference, same class as the documented pct1 deviation
 * (DESIGN.md "The L2 ADC table mode").
 * codes are bucket-format entries: M bytes at ksub=256; at ksub=16 M/2
 * bytes, byte b = sub-quantizer 2b in bits 0-3 and 2b+1 in bits 4-7. */
hipError_t pq_sterm(hipStream_t s, int64_t n, int M, int ksub, int nlist,
                    const uint8_t *codes, const int32_t *asg,
                    int asg_const, const float *btab, float *out);
/* Load-path batch: one launch rebuilds every bucket's S terms */
hipError_t pq_sterm_buckets(hipStream_t s, int nlist, int M, int ksub,
                            const GammaBucketDev *bks, const float *btab);

/* IVFPQ fused search (the kernels are in ivfpq_scan_kernels.hpp).
 *
 * 1. What the launch computes. One workgroup per (query, probe-split
 *    part) stages the query-level table ONCE (L2: A_q, dis = coarse_dis +
 *    S_v + sum A[c_m]; IP: the h:164-167 query table, dis = dis0 + sum
 *    T[c_m]), then scans the probed lists (h:923-953 semantics) and keeps
 *    the k2 best keys.
 *    - S = probe-split factor: S sub-workgroups per query, out_keys is
 *      nq x S x k2; merge with sort_rows. S = 1 gives nq x k2. S > 1 serves
 *      small batches.
 *    - qmap: optional query schedule — workgroup b serves query qmap[b/S].
 *      The engine sorts large batches by their first probed list so
 *      neighbouring workgroups scan the same lists while they are
 *      L2/LLC-resident (the 10M-doc code store is ~400 MB against the
 *      256 MiB Infinity Cache — unordered queries re-fetch every list
 *      ~nq*nprobe/nlist times from DRAM). Results are identical: the
 *      selector's top-k2 is order-independent and outputs are written at
 *      the ORIGINAL query row.
 *    - Keys do not depend on which kernel ran, nor on any knob below.
 *
 * 2. Which inputs a launch needs, by (ksub, metric, shape). The three
 *    predicates below are the authority; ivfpq_scan_reads_table says what
 *    the caller has to build.
 *    - ksub = 16 runs k_ivfpq_scan4 on packed 4-bit entries (M/2 bytes, low
 *      nibble = even sub-quantizer) with an M x 16 table; same contract.
 *      L2 needs atab (pq_tables_a); inner product needs neither atab nor
 *      cwn. ivfpq_scan_fits bounds M and d.
 *    - ksub = 256, wide — ivfpq_scan_is_wide(d, M, ksub, k2): where
 *      k_ivfpq_scan's resident table (M KB of LDS) cannot launch (M >= 144
 *      always, M of 136 to 140 depending on k2 and d; a fast-path M is wide
 *      too once 4*d fills the LDS), 8-bit codes run k_ivfpq_scan_wide, which
 *      keeps IVFPQ_WIDE_MS sub-quantizers of the table in LDS at a time and
 *      walks tiles of ivfpq_wide_tile() entries. It reads the query table
 *      from `atab` for BOTH metrics: pq_tables_a for L2, pq_tables_ip for
 *      inner product (nq x M x 256 floats; the caller bounds nq per
 *      launch). M % 4 == 0.
 *    - ksub = 256, not wide, ivfpq_scan_builds_table(M, ksub, k2) (M in
 *      {16,32,64,96}, k2 + block size within the selector cap): the kernel
 *      builds the query table itself from codebooks + cwn (pq_cwn); atab
 *      may be null. Inner product needs neither.
 *    - ksub = 256, every other launch: L2 requires atab (pq_tables_a) and
 *      cwn may be null. Inner product needs neither.
 *    ivfpq_scan_fits(d, M, ksub): whether a table of this shape can be
 *    scanned at every legal k2, for both metrics (the LDS bound on d, and
 *    on M for 4-bit codes).
 *
 * 3. Knobs, read from the environment per launch by the launcher and the
 *    predicates alike:
 *    - GAMMA_SCAN_BS (256|512 threads; default 512).
 *    - GAMMA_ADC_C (1|2 codes staged per thread, 4-bit kernel only — the
 *      8-bit fast path accepts and ignores it).
 *    - GAMMA_SCAN_WIDE=1 forces the wide kernel at any M.
 *    - GAMMA_FUSE_RERANK=0 turns ivfpq_scan_can_fuse_rerank off.
 *
 * 4. Fused re-rank: with `rr` set the resident-table 8-bit kernel ends in
 *    the epilogue of rerank_epilogue.hpp — exact distances of the query's
 *    top-k2 in gk::rerank's own fmaf chain, one sort, top-k written to
 *    rr->out_* — and out_keys is not touched (it may be null). Results are
 *    bit-identical to ivfpq_scan + rerank + sort_rows. Legal where
 *    ivfpq_scan_can_fuse_rerank: S == 1, 8-bit codes, not a wide launch,
 *    d % 4 == 0. Any other launch with rr set, or rr->k outside [1, 2048],
 *    is hipErrorInvalidValue and launches nothing. */
enum { IVFPQ_WIDE_MS = 32, IVFPQ_WIDE_E = 4 };
int ivfpq_wide_tile(); /* entries per tile at the current GAMMA_SCAN_BS */
bool ivfpq_scan_is_wide(int d, int M, int ksub, int k2);
enum { IVFPQ_MAX_DIM = 16384, IVFPQ4_MAX_LDS_TERM = 131072 };
bool ivfpq_scan_fits(int d, int M, int ksub);
/* the wide kernel's inner-product table: out[q][m][j] = q_m . cw_mj */
hipError_t pq_tables_ip(hipStream_t s, int nq, int d, int M,
                        const float *queries, const float *codebooks,
                        float *out);
bool ivfpq_scan_builds_table(int M, int ksub, int k2);
/* whether this launch reads `atab`: every wide launch (both metrics, any
 * M), and L2 launches whose kernel builds no table */
bool ivfpq_scan_reads_table(int d, int M, int ksub, int k2, bool ip);
bool ivfpq_scan_can_fuse_rerank(int d, int M, int ksub, int k2, int S);
hipError_t ivfpq_scan(hipStream_t s, int nq, int S, int d, int M, int ksub,
                      int nprobe,
                      int k2, const float *queries, const float *centroids,
                      const float *codebooks, const float *atab,
                      const float *cwn, const float *probe_dists,
                      const GammaBucketDev *buckets,
                      int nlist, const int64_t *probes,
                      const uint32_t *bitmap, bool ip, uint64_t *out_keys,
                      const int *kill_flag, const int32_t *qmap,
                      const GammaScanRerank *rr = nullptr);

/* out[q] = (int32) probes[q*nprobe] (the schedule sort key) */
hipError_t extract_probe0(hipStream_t s, int nq, int nprobe,
                          const int64_t *probes, int32_t *out);

/* IVFFLAT fused search (gamma_index_ivfflat.h:36-91). */
hipError_t ivfflat_scan(hipStream_t s, int nq, int d, int nprobe, int k2,
                        const float *queries, const GammaBucketDev *buckets,
                        int nlist, const int64_t *probes,
                        const uint32_t *bitmap, bool ip, uint64_t *out_keys);

/* Canonical-order exact re-rank (ivfpq.cc:675-726 + parity canonicalizer):
 * for each key in keys_in (nq x ncand), gather the raw vector through the
 * segment table and recompute the distance with the sequential fmaf loop.
 * keys_out may alias keys_in. */
hipError_t rerank(hipStream_t s, int nq, int ncand, int d,
                  const float *queries, const float *const *segs,
                  int n_segs, int seg_shift, bool ip,
                  const uint64_t *keys_in, uint64_t *keys_out);

/* Per-row sort of ncand keys (<= 2048), emit top-k (dists, ids). */
hipError_t sort_rows(hipStream_t s, int nq, int ncand, int k,
                     const uint64_t *keys, bool ip, float *out_dists,
                     int64_t *out_ids);

/* unpack keys -> (dists, ids) without sorting (keys already sorted). */
hipError_t unpack_keys(hipStream_t s, int64_t n, const uint64_t *keys,
                       bool ip, float *out_dists, int64_t *out_ids);

/* residuals[i] = x[i] - centroids[assign[i]] (elementwise exact). */
hipError_t residuals(hipStream_t s, int64_t n, int d, const float *x,
                     const float *centroids, const int32_t *assign,
                     float *out);

/* PQ encode: codes[i][m] = argmin_j ||x_sub - codebook[m][j]||^2
 * (pq.compute_codes, ivfpq.cc:494; ties -> lowest j). */
hipError_t pq_encode(hipStream_t s, int64_t n, int d, int M, int ksub,
                     const float *x, const float *codebooks, uint8_t *codes);
/* Same argmin at ksub=16, written as packed bucket entries: M/2 bytes
 * per vector, byte b = code 2b in bits 0-3, code 2b+1 in bits 4-7. The
 * training paths keep pq_encode's one-byte-per-code form. */
hipError_t pq_encode_pack4(hipStream_t s, int64_t n, int d, int M,
                           const float *x, const float *codebooks,
                           uint8_t *codes);

/* FLAT brute-force over the raw-vector segment table (no materialized
 * dist matrix): per query workgroup streams all n vectors. Used for small
 * nq; large nq goes through dots_mfma chunks + select_from_dots. */
hipError_t flat_stream_scan(hipStream_t s, int nq, int64_t n, int d, int k2,
                            const float *queries, const float *const *segs,
                            int seg_shift, const uint32_t *bitmap, bool ip,
                            uint64_t *out_keys);

/* ---- BINARYIVF (binary_kernels.hpp). A binary vector of d bits is
 * W = d/32 u32 words, LSB-first; distances are Hamming distances carried
 * as exact fp32 in the ordinary ascending (dist, id) key. */

/* out[i*n + j] = (float)popcount(Q_i xor B_j), Q nq x W, B n x W words.
 * Feeds select_from_dots / argmin_rows with l2 = false, ip_order = false. */
hipError_t hamming_matrix(hipStream_t s, const uint32_t *Q, int nq,
                          const uint32_t *B, int64_t n, int W, float *out);

/* Binary IVF fused scan, the contract of ivfpq_scan: one workgroup per
 * (query, probe-split sub-block), out_keys nq x S x k2 (merge with
 * sort_rows, ip = false); probes < 0 or >= nlist and empty lists are
 * skipped; bit 31 of an id and the bitmap drop an entry; kill_flag
 * (optional) stops the scan. Bucket `data` holds W words per entry,
 * `svals` is unused. W <= 128, k2 <= 1024. Reads GAMMA_SCAN_BS. */
hipError_t binivf_scan(hipStream_t s, int nq, int S, int W, int nprobe,
                       int k2, const uint32_t *queries,
                       const GammaBucketDev *buckets, int nlist,
                       const int64_t *probes, const uint32_t *bitmap,
                       uint64_t *out_keys, const int *kill_flag);

/* Exact Hamming top-k2 over the raw segment table (segments of
 * 1 << seg_shift vectors of W words), ids = row numbers < n. */
hipError_t hamming_flat_scan(hipStream_t s, int nq, int64_t n, int W, int k2,
                             const uint32_t *queries,
                             const uint32_t *const *segs, int seg_shift,
                             const uint32_t *bitmap, uint64_t *out_keys);

/* ---- IVFRABITQ (rabitq_kernels.hpp; the maths is at the top of that
 * file). d % 32 == 0, 32 <= d <= 4096. A bucket entry is d/32 sign words,
 * then the factors A and Mul as fp32 (d/8 + 8 bytes); bucket `svals` holds
 * sum_j bit_j * c_j of the entry's list centroid c. */

/* entries[i], svals[i] of vector x_i in list asg[i] (asg null: every
 * vector in list asg_const; numbers outside [0, nlist) are clamped).
 * ip selects A = n2 - ||x||^2 instead of n2. Deterministic: fixed
 * summation order, so equal inputs give equal bytes. */
hipError_t rabitq_encode(hipStream_t s, int64_t n, int d, const float *x,
                         const int32_t *asg, int asg_const, int nlist,
                         const float *centroids, bool ip, uint8_t *entries,
                         float *svals);
/* Load path: rebuild every bucket's svals from its entries and centroid
 * in one launch, bit-identical to rabitq_encode's. */
hipError_t rabitq_sval_buckets(hipStream_t s, int nlist, int d,
                               const GammaBucketDev *bks,
                               const float *centroids);
/* RaBitQ IVF fused scan, the contract of ivfpq_scan / binivf_scan: one
 * workgroup per (query, probe-split sub-block), out_keys nq x S x k2
 * (merge with sort_rows); probes < 0 or >= nlist and empty lists are
 * skipped; bit 31 of an id and the bitmap drop an entry; kill_flag
 * (optional) stops the scan. Keys are gamma_make_key<ip> of the estimate
 * (L2 ascending / inner product descending, ties by id). The kernel builds
 * its query table and the per-probe scalars itself from queries and
 * centroids. k2 <= 1024. Reads GAMMA_SCAN_BS; scores do not depend on it
 * or on S. */
hipError_t rabitq_scan(hipStream_t s, int nq, int S, int d, int nprobe,
                       int k2, const float *queries, const float *centroids,
                       const GammaBucketDev *buckets, int nlist,
                       const int64_t *probes, const uint32_t *bitmap, bool ip,
                       uint64_t *out_keys, const int *kill_flag);

}  // namespace gk
