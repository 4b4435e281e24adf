/*
 * ivfpq_scan_kernels.hpp — the IVFPQ fused scan family: codeword norms, query
 * tables, the three scan kernels, their LDS layouts, knobs, predicates and
 * launcher. Included at the end of kernels.hip (uses its WG) behind
 * select.hpp, scan_walk.hpp and rerank_epilogue.hpp, in front of
 * binary_kernels.hpp and rabitq_kernels.hpp, which read gamma_scan_bs.
 * What a launch computes is gk::ivfpq_scan's contract in kernels.h: per
 * entry dis = dis0 (+ S_v) + sum_m T[m][code_m], ascending m, plain adds,
 * bit for bit the oracle's (oracle_ivfpq_search_pct1; ivfpq.h:254-262 for
 * the decomposed L2 tables, h:164-167 for the IP table, h:923-953 the scan).
 *
 * Who serves which (ksub, M, k2, d), as gk::ivfpq_scan dispatches:
 * - ksub 256 and gk::ivfpq_scan_is_wide — gamma_scan8_smem(M, k2, d) above
 *   160 KB (M >= 144 always, 136-140 by k2 and d) or GAMMA_SCAN_WIDE=1:
 *   k_ivfpq_scan_wide<IP, BS>. Table slices of GAMMA_WIDE_MS sub-quantizers
 *   copied from `atab` (pq_tables_a / pq_tables_ip). Chunked flat walk in
 *   tiles; BS = GAMMA_SCAN_BS, or 256 where k2 + BS exceeds the selector cap.
 * - ksub 256, M in GAMMA_FAST_M, k2 + BS <= GAMMA_SORT_CAP
 *   (gamma_scan8_fast = gk::ivfpq_scan_builds_table): k_ivfpq_scan<IP, M/4,
 *   BS, RR>. Resident M*256 table built in-kernel (gamma_build_lut_l2 from
 *   codebooks + cwn, gamma_build_lut_ip). Chunked flat walk, prefetching
 *   pass loop (it stays in the kernel: scan_walk.hpp records why).
 * - ksub 256 otherwise: k_ivfpq_scan<IP, 0, WG, RR>. Resident table, L2
 *   copied from `atab` (pq_tables_a); gamma_pq_walk_lists, dword loads.
 * - ksub 16, M in GAMMA_FAST_M, k2 + BS*C <= GAMMA_SORT_CAP: k_ivfpq_scan4<IP,
 *   M/8, BS, C>. M*16 table (L2 from `atab`); two lists in flight per
 *   workgroup, C = GAMMA_ADC_C codes staged per thread per flush interval.
 * - ksub 16 otherwise: k_ivfpq_scan4<IP, 0, WG, 1>; gamma_pq_walk_lists,
 *   byte loads.
 * RR (gk::ivfpq_scan_can_fuse_rerank): the launch ends in the epilogue of
 * rerank_epilogue.hpp. The parts the kernels share come first below;
 * DESIGN.md "Kernels" item 3 names them.
 */
#pragma once
#include <type_traits>

/* cwn[e] = ||cw_e||^2 for the M*ksub codewords of dsub floats each: the
 * query-independent half of every L2 table entry, computed once per
 * model. The fmaf chain (and its float4 / scalar split on dsub & 3) is
 * the one k_pq_atable runs per query, so fmaf(-2, dot, cwn[e]) below
 * reproduces pq_tables_a bit for bit. */
__device__ __forceinline__ float gamma_cw_norm(const float *cw, int dsub) {
  float cwn = 0.0f;
  if ((dsub & 3) == 0) {
    for (int t = 0; t < dsub; t += 4) {
      float4 c4 = *(const float4 *)(cw + t);
      cwn = fmaf(c4.x, c4.x, cwn);
      cwn = fmaf(c4.y, c4.y, cwn);
      cwn = fmaf(c4.z, c4.z, cwn);
      cwn = fmaf(c4.w, c4.w, cwn);
    }
  } else {
    for (int t = 0; t < dsub; t++) cwn = fmaf(cw[t], cw[t], cwn);
  }
  return cwn;
}

__global__ void k_pq_cwn(int nent, int dsub,
                         const float *__restrict__ codebooks,
                         float *__restrict__ cwn) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nent) return;
  cwn[e] = gamma_cw_norm(codebooks + (size_t)e * dsub, dsub);
}

hipError_t gk::pq_cwn(hipStream_t s, int M, int ksub, int dsub,
                      const float *codebooks, float *cwn) {
  int nent = M * ksub;
  if (nent <= 0) return hipSuccess;
  k_pq_cwn<<<dim3((uint32_t)((nent + WG - 1) / WG)), dim3(WG), 0, s>>>(
      nent, dsub, codebooks, cwn);
  return hipGetLastError();
}

/* The L2 query table of one query, built by the whole block into `lut`
 * (M*ksub floats, usually LDS): lut[e] = fmaf(-2, q_m . cw_e, cwn[e]) with
 * k_pq_atable's dot chain, so every entry equals pq_tables_a's. `qs` is
 * the query (d floats; all lanes of a wave read the same sub-vector, an
 * LDS broadcast), lane e streams codeword e (coalesced, L2-resident).
 * The caller barriers before reading lut. */
__device__ __forceinline__ void gamma_build_lut_l2(
    float *lut, const float *qs, const float *__restrict__ codebooks,
    const float *__restrict__ cwn, int M, int kb, int dsub) {
  const int nent = M << kb;
  for (int e = threadIdx.x; e < nent; e += blockDim.x) {
    const float *cw = codebooks + (size_t)e * dsub;
    const float *qm = qs + (e >> kb) * dsub;
    float dot = 0.0f;
    if ((dsub & 3) == 0) {
      for (int t = 0; t < dsub; t += 4) {
        float4 c4 = *(const float4 *)(cw + t);
        float4 q4 = *(const float4 *)(qm + t);
        dot = fmaf(q4.x, c4.x, dot);
        dot = fmaf(q4.y, c4.y, dot);
        dot = fmaf(q4.z, c4.z, dot);
        dot = fmaf(q4.w, c4.w, dot);
      }
    } else {
      for (int t = 0; t < dsub; t++) dot = fmaf(qm[t], cw[t], dot);
    }
    lut[e] = fmaf(-2.0f, dot, cwn[e]);
  }
}
/* The inner-product query table, built the same way: lut[e] = q_m . cw_e
 * in the canonical serial chain. The caller barriers before reading lut. */
__device__ __forceinline__ void gamma_build_lut_ip(
    float *lut, const float *qs, const float *codebooks, int M, int kb,
    int dsub) {
  const int ksub = 1 << kb;
  for (int e = threadIdx.x; e < M * ksub; e += blockDim.x) {
    const int m = e >> kb, j = e & (ksub - 1);
    const float *cw = codebooks + ((size_t)m * ksub + j) * dsub;
    lut[e] = gamma_dot_serial(qs + m * dsub, cw, dsub);
  }
}
/* a precomputed table row (nfloat % 4 == 0 floats of `atab`) copied into lut
 * as float4; the caller barriers before reading */
__device__ __forceinline__ void gamma_copy_lut(float *lut, const float *row,
                                               int nfloat) {
  for (int e = threadIdx.x; e < nfloat >> 2; e += blockDim.x)
    ((float4 *)lut)[e] = ((const float4 *)row)[e];
}

/* test hook: the table gamma_build_lut_l2 leaves in LDS, per query */
__global__ void __launch_bounds__(WG)
k_pq_lut_l2_dump(int d, int M, int kb, const float *__restrict__ queries,
                 const float *__restrict__ codebooks,
                 const float *__restrict__ cwn, float *__restrict__ out) {
  extern __shared__ char smem[];
  float *lut = (float *)smem;
  float *qs = lut + ((size_t)M << kb);
  const int q = blockIdx.x;
  for (int i = threadIdx.x; i < d; i += blockDim.x)
    qs[i] = queries[(int64_t)q * d + i];
  __syncthreads();
  gamma_build_lut_l2(lut, qs, codebooks, cwn, M, kb, d / M);
  __syncthreads();
  for (int e = threadIdx.x; e < (M << kb); e += blockDim.x)
    out[((int64_t)q * M << kb) + e] = lut[e];
}

hipError_t gk::pq_lut_l2_dump(hipStream_t s, int nq, int d, int M, int ksub,
                              const float *queries, const float *codebooks,
                              const float *cwn, float *out) {
  if (ksub != 256 && ksub != 16) return hipErrorInvalidValue;
  size_t smem = ((size_t)M * ksub + d) * 4;
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  if (nq <= 0) return hipSuccess;
  k_pq_lut_l2_dump<<<dim3((uint32_t)nq), dim3(WG), smem, s>>>(
      d, M, ksub == 256 ? 8 : 4, queries, codebooks, cwn, out);
  return hipGetLastError();
}

/* ------------------------------------------------------------ LDS layouts
 * The two 8-bit kernels: table (ntab floats) | selector scratch + result |
 * the query (nqs floats, 16-B aligned for the table builder's float4 reads)
 * | chunk. k_ivfpq_scan: ntab = M*256, nqs = d. k_ivfpq_scan_wide: ntab =
 * one slice, nqs = d for IP and 0 for L2, which stages no query. */
#define GAMMA_WIDE_MS 32 /* sub-quantizers per table slice: 32 KB of LDS */
#define GAMMA_WIDE_E 4   /* entries per thread per tile */

__host__ __device__ static size_t gamma_pq_sort_off(size_t ntab) {
  return ntab * 4;
}
__host__ __device__ static size_t gamma_pq_qs_off(size_t ntab, int k2) {
  size_t o = gamma_pq_sort_off(ntab) + ((size_t)GAMMA_SORT_CAP + k2) * 8;
  return (o + 15) / 16 * 16;
}
__host__ __device__ static size_t gamma_pq_chunk_off(size_t ntab, int k2,
                                                     size_t nqs) {
  return (gamma_pq_qs_off(ntab, k2) + nqs * 4 + 7) / 8 * 8;
}
/* this total decides which M moves to the sliced kernel (ivfpq_scan_is_wide) */
static size_t gamma_scan8_smem(int M, int k2, int d) {
  return gamma_pq_chunk_off((size_t)M * 256, k2, (size_t)d) +
         sizeof(GammaScanChunk);
}
static size_t gamma_wide_smem(int k2, int d, bool ip) {
  return gamma_pq_chunk_off((size_t)GAMMA_WIDE_MS * 256, k2,
                            ip ? (size_t)d : 0) + sizeof(GammaScanChunk);
}

/* k_ivfpq_scan4: table (M*16 floats, M % 4 == 0) | selector scratch + result
 * | the query (d floats) | GammaScan4Tail. The tail's long longs stay 8-byte
 * aligned: d is even for every 4-bit table (d = M * dsub with M even). */
struct GammaScan4Tail {
  float dis0[2];    /* one per half of the two-list walk */
  long long sz[2];  /* list sizes, one per half */
  int pad;
  int state[1];     /* selector append counter */
  int kill[2];      /* the kill flag as thread 0 last read it */
};
static_assert(sizeof(GammaScan4Tail) == 40, "k_ivfpq_scan4's LDS total");
__host__ __device__ static size_t gamma_scan4_table_bytes(int M) {
  return (size_t)M * 16 * 4;
}
__host__ __device__ static size_t gamma_scan4_qs_off(int M, int k2) {
  return gamma_scan4_table_bytes(M) + ((size_t)GAMMA_SORT_CAP + k2) * 8;
}
__host__ __device__ static size_t gamma_scan4_tail_off(int M, int k2, int d) {
  return gamma_scan4_qs_off(M, k2) + (size_t)d * 4;
}
static size_t gamma_scan4_smem(int M, int k2, int d) {
  return gamma_scan4_tail_off(M, k2, d) + sizeof(GammaScan4Tail);
}

/* ------------------------------------------------------------ shared parts
 * Block b serves part `sub` of the S-way probe split of scheduled slot bq:
 * probes p = sub (mod S); sort_rows merges the parts (S > 1 lets a lone
 * query fill S CUs). The kernel returns where bq >= nq; as a flag returned
 * from here that test survived inlining as a second branch. */
struct GammaScanBlock {
  int bq, sub;
  __device__ __forceinline__ explicit GammaScanBlock(int S) {
    bq = blockIdx.x / S;
    sub = blockIdx.x - bq * S;
  }
  /* the query through the optional schedule `qmap` (outputs go to row q,
   * the ORIGINAL row). STAGE copies it into qs; sel.init has the barrier. */
  template <bool STAGE>
  __device__ __forceinline__ int query(int d, const int32_t *qmap,
                                       const float *queries, float *qs) const {
    const int q = qmap ? qmap[bq] : bq;
    if (STAGE) {
      const float *qg = queries + (int64_t)q * d;
      for (int i = threadIdx.x; i < d; i += blockDim.x) qs[i] = qg[i];
    }
    return q;
  }
};

/* dis += T[m][code_m] for the four sub-quantizers of one 8-bit code word,
 * ascending m; tab = the row of the word's first sub-quantizer and moves on
 * to the next word's (gamma_wide_add4: the same over a constant stride) */
__device__ __forceinline__ float gamma_adc8_add4(float dis, const float *&tab,
                                                 uint32_t wv) {
  dis += tab[wv & 255u];         tab += 256;
  dis += tab[(wv >> 8) & 255u];  tab += 256;
  dis += tab[(wv >> 16) & 255u]; tab += 256;
  dis += tab[wv >> 24];          tab += 256;
  return dis;
}
/* the same for the eight sub-quantizers of one 4-bit code word: nibbles
 * from bit 0 up, rows of 16 floats */
__device__ __forceinline__ float gamma_adc4_add8(float dis, const float *&tab,
                                                 uint32_t wv) {
#pragma unroll
  for (int nb = 0; nb < 8; nb++) {
    dis += tab[(wv >> (4 * nb)) & 15u];
    tab += 16;
  }
  return dis;
}

/* Chunk fill of the flat walk: store a probe's descriptor and dis0. The
 * lookup and dis0 by metric stay in the two kernels: written in here, six
 * inner-product instantiations of k_ivfpq_scan got other VGPR counts. */
__device__ __forceinline__ void gamma_pq_chunk_put(
    GammaScanChunk *ch, unsigned slot, const GammaBucketDev &bk, float dis0) {
  gamma_chunk_put(ch, slot, bk);
  ch->per.dis0[slot] = dis0;
}
/* the cursor's current list; load is the reload of GammaListCursor::seek */
struct GammaPqListRefs {
  gamma_gu32p ids;
  gamma_gu8p codes;
  gamma_gf32p svals;
  float dis0;
  __device__ __forceinline__ void load(const GammaScanChunk *ch, int li) {
    ids = ch->ids[li];
    codes = ch->codes[li];
    svals = ch->svals[li];
    dis0 = ch->per.dis0[li];
  }
};

/* The list-by-list walk of the generic (runtime-M) paths: one list at a
 * time, thread t takes entries t, t + blockDim.x, ... decode(entry, dis)
 * returns dis + sum_m T[m][code_m] over the entry's `entry_bytes` code
 * bytes, ascending m. killsh: int[2], dis0sh: float[1], both LDS. */
template <bool IP, class Decode>
__device__ __forceinline__ void gamma_pq_walk_lists(
    GammaSelector &sel, int q, int sub, int S, int d, int nprobe,
    int entry_bytes, const float *qs, const float *centroids,
    const float *probe_dists, const GammaBucketDev *buckets, int nlist,
    const int64_t *probes, const uint32_t *bitmap, const int *kill_flag,
    int *killsh, float *dis0sh, Decode &&decode) {
  int kslot = 0;
  for (int p = sub; p < nprobe; p += S, kslot ^= 1) {
    if (kill_flag) {
      /* one thread polls the kill flag and the block reads its answer from
       * LDS behind a barrier, so every thread leaves at the same probe even
       * when the flag flips between two threads' reads. The slots
       * alternate: one is rewritten two barriers after it was read. */
      if (threadIdx.x == 0)
        killsh[kslot] = __hip_atomic_load(kill_flag, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      if (killsh[kslot]) break;
    }
    int64_t ln = probes[(int64_t)q * nprobe + p];
    if (ln < 0 || ln >= nlist) continue;
    GammaBucketDev bk = buckets[ln];
    if (bk.size <= 0) continue;
    const float *cent = centroids + (size_t)ln * d;

    float dis0;
    if (IP) {
      if (threadIdx.x == 0) /* dis0 = dot(q, c), canonical order */
        dis0sh[0] = gamma_dot_serial(qs, cent, d);
      __syncthreads();
      dis0 = dis0sh[0];
    } else {
      dis0 = probe_dists[(int64_t)q * nprobe + p];
    }

    const uint32_t *ids = bk.ids;
    const uint8_t *codes = (const uint8_t *)bk.data;
    const float *svals = (const float *)bk.svals;
    for (long long j0 = 0; j0 < bk.size; j0 += blockDim.x) {
      long long j = j0 + threadIdx.x;
      if (j < bk.size) {
        int64_t id = (int64_t)(int32_t)ids[j];
        if (!((uint64_t)id >> 63) &&
            !gamma_bitmap_test(bitmap, (uint64_t)id)) {
          const float dis = decode(codes + (size_t)j * entry_bytes,
                                   IP ? dis0 : dis0 + svals[j]);
          sel.push(gamma_make_key<IP>(dis, (uint32_t)id));
        }
      }
      sel.maybe_flush(blockDim.x);
    }
    if (IP) __syncthreads(); /* dis0 slot rewritten next list */
  }
}

/* one list entry in flight: MW code words, the raw id (bit 31 = skip:
 * delete mark, or no entry at this flat index), its S term and its
 * list's dis0 */
template <int MW>
struct GammaScanElem {
  uint32_t w[MW ? MW : 1];
  uint32_t id;
  float sv, dis0;
  bool live; /* false: the lane has no entry in this pass */
};

/* RR: the launch carries a re-rank block and ends in the epilogue of
 * rerank_epilogue.hpp instead of the out_keys store (S == 1 only). A
 * template flag, not a run-time test: the RR = false instantiations keep
 * the code they had before the epilogue existed. */
template <bool IP, int MW, int BS, bool RR>
__global__ void __launch_bounds__(BS)
k_ivfpq_scan(
    int nq, int S, int d, int M, int nprobe, int k2,
    const float *__restrict__ queries, const float *__restrict__ centroids,
    const float *__restrict__ codebooks, const float *__restrict__ atab,
    const float *__restrict__ cwn, const float *__restrict__ probe_dists,
    const GammaBucketDev *__restrict__ buckets, int nlist,
    const int64_t *__restrict__ probes, const uint32_t *__restrict__ bitmap,
    uint64_t *__restrict__ out_keys, const int *__restrict__ kill_flag,
    const int32_t *__restrict__ qmap, GammaScanRerank rr) {
  extern __shared__ char smem[];
  const int ksub = 256;
  const int dsub = d / M;
  const size_t ntab = (size_t)M * 256;
  float *lut = (float *)smem;                       /* M*ksub */
  uint64_t *sortbuf = (uint64_t *)(smem + gamma_pq_sort_off(ntab));
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(smem + gamma_pq_qs_off(ntab, k2)); /* d */
  GammaScanChunk *ch =
      (GammaScanChunk *)(smem + gamma_pq_chunk_off(ntab, k2, (size_t)d));

  const GammaScanBlock blk(S);
  if (blk.bq >= nq) return;
  const int sub = blk.sub;
  const int q = blk.query<true>(d, qmap, queries, qs);

  GammaSelector sel;
  sel.init(sortbuf, res, ch->state, k2);  /* has the barrier qs needs */

  if (IP) {
    /* query-level table T[m][j] = dot(q_m, cw_mj), canonical per entry */
    gamma_build_lut_ip(lut, qs, codebooks, M, 8, dsub);
    __syncthreads();
  } else if (MW > 0) {
    /* L2 fast path: the A table is built here, straight into LDS, from the
     * codebooks and codeword norms — no pq_tables_a launch, no 32 KB/query
     * round trip through HBM; entries are bit-identical to pq_tables_a's.
     * The list half (B) arrives as one float per vector (gk::pq_sterm). */
    gamma_build_lut_l2(lut, qs, codebooks, cwn, M, 8, dsub);
    __syncthreads();
  } else {
    /* generic path: the A table comes precomputed (gk::pq_tables_a) */
    gamma_copy_lut(lut, atab + (size_t)q * M * ksub, M * ksub);
    __syncthreads();
  }

  if (MW > 0) {
    /* Flattened, software-pipelined scan over the chunked probe walk of
     * scan_walk.hpp. Thread tid handles flat entries g = it*BS + tid of
     * the current chunk, so the trip count is uniform across the block
     * (the selector's barriers stay aligned) and only a chunk's last pass
     * has idle lanes. The loads of pass it+1 (code words, id, S term) are
     * issued into a second register set BEFORE the LDS gather of pass it:
     * a workgroup's HBM latency runs under its own gather instead of in
     * front of it. The loop is unrolled by two so the register sets
     * alternate without copies and the wait in front of each gather is a
     * counted vmcnt that leaves the prefetch outstanding. Push order
     * differs from a list-by-list walk; the selector's top-k2 is exact
     * under the (dist,id) total order, so results are unchanged. */
    const unsigned tid = threadIdx.x;
    const int np_sub = sub < nprobe ? (nprobe - sub + S - 1) / S : 0;
    const int *kf = kill_flag ? kill_flag : (const int *)probes;
    bool killed = false;
    for (int c0 = 0; c0 < np_sub && !killed;) {
      const int cn = min(GAMMA_SCAN_PCH, np_sub - c0);
      if ((int)tid < cn) { /* one thread per probe of the chunk */
        const int p = sub + (c0 + (int)tid) * S;
        const int64_t ln = probes[(int64_t)q * nprobe + p];
        GammaBucketDev bk = gamma_null_bucket();
        float dis0 = 0.0f;
        if (ln >= 0 && ln < nlist) {
          bk = buckets[ln];
          if (IP) /* dis0 = dot(q, c), canonical serial order */
            dis0 = gamma_dot_serial(qs, centroids + (size_t)ln * d, d);
          else /* the coarse probe distance (ivfpq.h:255 dis0=coarse_dis); the
                  list half of the table arrives as the per-vector S term */
            dis0 = probe_dists[(int64_t)q * nprobe + p];
        }
        gamma_pq_chunk_put(ch, tid, bk, dis0);
      }
      const GammaChunkSpan sp = gamma_chunk_close(ch, cn, kill_flag);
      c0 += sp.ncons;

      GammaListCursor cur;
      cur.reset(ch, sp.total);
      GammaPqListRefs ls;
      ls.load(ch, 0);

      /* The loads sit in straight-line code (the cursor aliases a dead
       * lane to the chunk's last entry instead of skipping its loads):
       * behind a branch the compiler's wait in front of the gather has to
       * assume the prefetch may not have been issued and degrades to
       * vmcnt(0). */
      auto fetch = [&](GammaScanElem<MW> &e, unsigned it) {
        const unsigned j = cur.seek(ch, it * BS + tid, e.live,
                                    [&](int li) { ls.load(ch, li); });
        e.id = ls.ids[j];
        if (!IP) e.sv = ls.svals[j];
        e.dis0 = ls.dis0;
        gamma_gu32p cw = (gamma_gu32p)(ls.codes + (size_t)j * (MW * 4));
#pragma unroll
        for (int mw = 0; mw < MW; mw++) e.w[mw] = cw[mw];
      };
      /* wait for all of an entry's loads (one counted vmcnt; the empty
       * asm only names the registers). Loads left pending — by a skipped
       * entry, or by the prefetch past the last pass — would make the
       * compiler drain the NEXT prefetch as soon as one of their
       * registers is reused. */
      auto retire = [&](const GammaScanElem<MW> &e) {
#pragma unroll
        for (int mw = 0; mw < MW; mw++) asm volatile("" ::"v"(e.w[mw]));
        asm volatile("" ::"v"(e.id));
        if (!IP) asm volatile("" ::"v"(e.sv));
      };
      auto consume = [&](const GammaScanElem<MW> &e) {
        retire(e);
        if (e.live && !(e.id >> 31) &&
            !gamma_bitmap_test(bitmap, (uint64_t)e.id)) {
          float dis = IP ? e.dis0 : e.dis0 + e.sv;
          const float *tab = lut;
#pragma unroll
          for (int mw = 0; mw < MW; mw++)
            dis = gamma_adc8_add4(dis, tab, e.w[mw]);
          sel.push(gamma_make_key<IP>(dis, e.id));
        }
      };
      /* Flush check (one barrier). A pass pushes at most BS keys, so
       * where k2 + 2*BS fits the selector cap the check runs every
       * second pass with margin 2*BS — half the barriers, at the
       * headline shape among others — and otherwise every pass with
       * margin BS. Either way at most `fmargin` pushes separate two
       * checks (the chunk's closing check below covers an odd last pass),
       * which is maybe_flush's invariant.
       * The kill flag is polled every pass, by the rule of the prefetch:
       * the load is issued in front of it, in straight-line code (a
       * null flag polls a harmless readable word instead), and its
       * answer is used only after the gather. On a checking pass thread
       * 0 posts it in a kill[] slot before the barrier and everyone
       * reads it right behind the barrier; slots alternate so that one
       * is next written two barriers later. */
      const bool flush_each = k2 + 2 * BS > GAMMA_SORT_CAP;
      const int fmargin = flush_each ? BS : 2 * BS;
      auto pass = [&](GammaScanElem<MW> &nxt, const GammaScanElem<MW> &cur,
                      unsigned it_nxt, int slot, bool check) {
        const int kv = __hip_atomic_load(kf, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        fetch(nxt, it_nxt);
        consume(cur);
        asm volatile("" ::"v"(kv)); /* retired in every wave, as above */
        if (!check) return false;
        if (tid == 0) ch->kill[slot] = kill_flag ? kv : 0;
        sel.maybe_flush(fmargin);
        return ch->kill[slot] != 0;
      };
      killed = sp.killed;
      const unsigned niter = (sp.total + BS - 1) / BS;
      if (niter > 0) {
        GammaScanElem<MW> ea, eb;
        fetch(ea, 0);
        for (unsigned it = 0; it < niter; it += 2) {
          if ((killed = pass(eb, ea, it + 1, 0, flush_each))) break;
          if (it + 1 >= niter) break;
          if ((killed = pass(ea, eb, it + 2,
                             flush_each ? 1 : (int)((it >> 1) & 1u), true)))
            break;
        }
        retire(ea);
        retire(eb);
      }
      /* barrier: the chunk is rewritten next round. It doubles as the
       * flush check an odd last pass skipped, so every chunk starts with
       * a full margin. */
      sel.maybe_flush(fmargin);
    }
  } else {
    /* generic path: dword loads of the M/4 code words of an entry */
    const int mwords = M >> 2;
    gamma_pq_walk_lists<IP>(
        sel, q, sub, S, d, nprobe, M, qs, centroids, probe_dists, buckets,
        nlist, probes, bitmap, kill_flag, ch->kill, ch->per.dis0,
        [&](const uint8_t *entry, float dis) {
          const uint32_t *cw = (const uint32_t *)entry;
          const float *tab = lut;
          for (int mw = 0; mw < mwords; mw++)
            dis = gamma_adc8_add4(dis, tab, cw[mw]);
          return dis;
        });
  }
  sel.finish();
  if (RR) {
    /* the table and the scan's query copy are dead: the epilogue stages
     * candidate rows in the one and keeps the raw query in the other */
    gamma_rerank_topk_epilogue<IP, BS>(
        res, k2, sortbuf, lut, M * ksub, qs, rr.queries + (int64_t)q * d, d,
        rr.segs, rr.seg_shift, rr.k, rr.out_dists + (int64_t)q * rr.k,
        rr.out_ids + (int64_t)q * rr.k);
    return;
  }
  for (int i = threadIdx.x; i < k2; i += blockDim.x)
    out_keys[((int64_t)q * S + sub) * k2 + i] = res[i];
}

/* --------------------------------- IVFPQ fused scan, 8-bit, sliced table
 * k_ivfpq_scan's contract and flat, chunked probe walk for any M, with LDS
 * that does not grow with M: GAMMA_WIDE_MS sub-quantizers of the table at a
 * time (DESIGN.md "Wide PQ" has the tile and slice loops in full). Thread
 * tid owns entries tile*T + e*BS + tid, e < E = GAMMA_WIDE_E, T = BS*E, and
 * keeps their distances in registers. Per tile and slice: load the slice's
 * code words, barrier, copy the slice's rows of `tab` (nq x M x 256 floats:
 * gk::pq_tables_a for L2, gk::pq_tables_ip for IP) into LDS, barrier, add.
 * Slices and m ascend, so every distance is k_ivfpq_scan's add chain, bit
 * for bit. Code loads are 16 bytes wide where M and every list of the
 * chunk allow it, single dwords otherwise. */
typedef uint32_t gamma_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) gamma_u32x4 *gamma_gu128p;

/* one entry's code words of one slice: 16-byte loads for a whole slice of
 * 16-byte-aligned entries, single words otherwise. A partial slice has
 * msw < MSW words; the words past it repeat its last word (never read
 * past the entry) and are not used. */
template <int MSW, bool A16>
__device__ __forceinline__ void gamma_wide_load(uint32_t (&w)[MSW],
                                                gamma_gu32p p, int msw) {
  if (A16) {
    gamma_gu128p p4 = (gamma_gu128p)p;
#pragma unroll
    for (int u = 0; u < MSW / 4; u++) {
      const gamma_u32x4 v = p4[u];
      w[4 * u] = v.x; w[4 * u + 1] = v.y;
      w[4 * u + 2] = v.z; w[4 * u + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int u = 0; u < MSW; u++) w[u] = p[min(u, msw - 1)];
  }
}

/* acc += row[m][code_m] for the four sub-quantizers of one code word,
 * ascending m; row = the table row of the word's first sub-quantizer */
__device__ __forceinline__ float gamma_wide_add4(float acc, const float *row,
                                                 uint32_t wv) {
  acc += row[wv & 255u];
  acc += row[256 + ((wv >> 8) & 255u)];
  acc += row[512 + ((wv >> 16) & 255u)];
  acc += row[768 + (wv >> 24)];
  return acc;
}

/* two 512-thread workgroups per CU are 4 waves per SIMD (<= 128 VGPRs);
 * three 256-thread ones are 3 */
template <bool IP, int BS>
__global__ void __launch_bounds__(BS, BS == 512 ? 4 : 3)
k_ivfpq_scan_wide(
    int nq, int S, int d, int M, int nprobe, int k2,
    const float *__restrict__ queries, const float *__restrict__ centroids,
    const float *__restrict__ tab, const float *__restrict__ probe_dists,
    const GammaBucketDev *__restrict__ buckets, int nlist,
    const int64_t *__restrict__ probes, const uint32_t *__restrict__ bitmap,
    uint64_t *__restrict__ out_keys, const int *__restrict__ kill_flag,
    const int32_t *__restrict__ qmap) {
  extern __shared__ char smem[];
  constexpr int MS = GAMMA_WIDE_MS, E = GAMMA_WIDE_E, MSW = MS / 4;
  constexpr unsigned T = (unsigned)BS * E;
  constexpr int NT = MS * 256 / 4 / BS; /* table float4s per thread */
  const size_t ntab = (size_t)GAMMA_WIDE_MS * 256;
  float *lut = (float *)smem;                       /* MS*256 */
  uint64_t *sortbuf = (uint64_t *)(smem + gamma_pq_sort_off(ntab));
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(smem + gamma_pq_qs_off(ntab, k2)); /* d, IP only */
  GammaScanChunk *ch = (GammaScanChunk *)(smem +
      gamma_pq_chunk_off(ntab, k2, IP ? (size_t)d : 0));

  const GammaScanBlock blk(S);
  if (blk.bq >= nq) return;
  const int sub = blk.sub;
  const int q = blk.query<IP>(d, qmap, queries, qs); /* staged for IP only */
  const float *qtab = tab + (size_t)q * M * 256;

  GammaSelector sel;
  sel.init(sortbuf, res, ch->state, k2);  /* has the barrier qs needs */

  const unsigned tid = threadIdx.x;
  const int nslice = (M + MS - 1) / MS;
  const int np_sub = sub < nprobe ? (nprobe - sub + S - 1) / S : 0;
  bool killed = false;
  for (int c0 = 0; c0 < np_sub && !killed;) {
    const int cn = min(GAMMA_SCAN_PCH, np_sub - c0);
    int misaligned = 0;
    if ((int)tid < cn) { /* one thread per probe of the chunk */
      const int p = sub + (c0 + (int)tid) * S;
      const int64_t ln = probes[(int64_t)q * nprobe + p];
      GammaBucketDev bk = gamma_null_bucket();
      float dis0 = 0.0f;
      if (ln >= 0 && ln < nlist) {
        bk = buckets[ln];
        if (IP) /* as in k_ivfpq_scan */
          dis0 = gamma_dot_serial(qs, centroids + (size_t)ln * d, d);
        else
          dis0 = probe_dists[(int64_t)q * nprobe + p];
      }
      gamma_pq_chunk_put(ch, tid, bk, dis0);
      misaligned = bk.size > 0 && ((uintptr_t)bk.data & 15) != 0;
    }
    /* the close's first barrier carries the vote: 16-byte code loads need
     * every list of the chunk 16-byte aligned (and M % 16 == 0) */
    const GammaChunkSpan sp =
        gamma_chunk_close<true>(ch, cn, kill_flag, &misaligned);
    const bool a16 = !misaligned && (M & 15) == 0;
    killed = sp.killed;
    const unsigned total = sp.total;
    const unsigned ntile = (total + T - 1) / T;
    c0 += sp.ncons;

    GammaListCursor cur;
    cur.reset(ch, total);
    GammaPqListRefs ls;
    ls.load(ch, 0);

    for (unsigned tile = 0; tile < ntile; tile++) {
      /* a slot with no entry (only in a chunk's last tile) carries the
       * skip bit */
      gamma_gu32p cw[E];
      uint32_t id[E];
      float dis[E];
#pragma unroll
      for (int e = 0; e < E; e++) {
        bool live;
        const unsigned j =
            cur.seek(ch, tile * T + (unsigned)e * BS + tid, live,
                     [&](int li) { ls.load(ch, li); });
        uint32_t idv = ls.ids[j];
        if (!live ||
            (!(idv >> 31) && gamma_bitmap_test(bitmap, (uint64_t)idv)))
          idv |= 0x80000000u;
        id[e] = idv;
        dis[e] = IP ? ls.dis0 : ls.dis0 + ls.svals[j];
        cw[e] = (gamma_gu32p)(ls.codes + (size_t)j * M);
      }
      if (tid == 0) /* this tile's poll; read behind the slice barrier */
        ch->kill[1] = kill_flag
                          ? __hip_atomic_load(kill_flag, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT)
                          : 0;
      for (int sl = 0; sl < nslice; sl++) {
        const int msw = min(MSW, (M - sl * MS) >> 2); /* words this slice */
        /* the slice's code words are requested in front of the barrier */
        uint32_t w[E][MSW];
        if (a16 && msw == MSW) {
#pragma unroll
          for (int e = 0; e < E; e++)
            gamma_wide_load<MSW, true>(w[e], cw[e] + sl * MSW, msw);
        } else {
#pragma unroll
          for (int e = 0; e < E; e++)
            gamma_wide_load<MSW, false>(w[e], cw[e] + sl * MSW, msw);
        }
        __syncthreads(); /* the previous slice's gather is done */
        if (sl == 0 && (killed = ch->kill[1] != 0)) break;
        {
          const float4 *src =
              (const float4 *)(qtab + (size_t)sl * MS * 256);
          const int n4 = msw * 256; /* float4s of the slice */
#pragma unroll
          for (int k = 0; k < NT; k++) {
            const int i = (int)tid + k * BS;
            if (i < n4) ((float4 *)lut)[i] = src[i];
          }
        }
        __syncthreads();
        /* word by word across the E entries: E independent add chains
         * with 4*E lookups in flight. The scheduling fence keeps the
         * compiler from hoisting a whole slice's lookups into registers
         * (which spills at 128 VGPRs). */
#pragma unroll
        for (int u = 0; u < MSW; u++) {
          if (u < msw) { /* uniform */
#pragma unroll
            for (int e = 0; e < E; e++)
              dis[e] = gamma_wide_add4(dis[e], lut + u * 1024, w[e][u]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (killed) break; /* uniform: every thread read the same slot */
      /* Push rounds: two entries per thread and margin 2*BS where that
       * fits the selector cap, else one and margin BS. A push may follow
       * a flush check only behind another barrier: a wave still reading
       * the append counter for its check must not see a later push, or
       * the block would disagree on flushing. The last check of a tile is
       * followed by the next tile's slice barriers (or the chunk's). */
      auto push = [&](int e) {
        if (!(id[e] >> 31)) sel.push(gamma_make_key<IP>(dis[e], id[e]));
      };
      if (k2 + 2 * BS <= GAMMA_SORT_CAP) {
        static_assert(GAMMA_WIDE_E == 4, "two rounds of two entries");
        push(0); push(1);
        sel.maybe_flush(2 * BS);
        __syncthreads();
        push(2); push(3);
        sel.maybe_flush(2 * BS);
      } else {
#pragma unroll
        for (int e = 0; e < E; e++) {
          push(e);
          sel.maybe_flush(BS);
          if (e + 1 < E) __syncthreads();
        }
      }
    }
    /* barrier: the chunk is rewritten next round */
    __syncthreads();
  }
  sel.finish();
  for (int i = threadIdx.x; i < k2; i += blockDim.x)
    out_keys[((int64_t)q * S + sub) * k2 + i] = res[i];
}

/* the IP query table of the sliced scan: out[q][m][j] = q_m . cw_mj in the
 * serial fmaf chain k_ivfpq_scan runs for its own IP table */
__global__ void k_pq_iptable(int64_t total, int d, int M,
                             const float *__restrict__ queries,
                             const float *__restrict__ codebooks,
                             float *__restrict__ out) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int dsub = d / M;
  const int64_t q = e / ((int64_t)M * 256);
  const int mj = (int)(e - q * M * 256); /* m*256 + j */
  const float *cw = codebooks + (size_t)mj * dsub;
  const float *qm = queries + q * d + (mj >> 8) * dsub;
  out[e] = gamma_dot_serial(qm, cw, dsub);
}

hipError_t gk::pq_tables_ip(hipStream_t s, int nq, int d, int M,
                            const float *queries, const float *codebooks,
                            float *out) {
  const int64_t total = (int64_t)nq * M * 256;
  if (total <= 0) return hipSuccess;
  k_pq_iptable<<<dim3((uint32_t)((total + WG - 1) / WG)), dim3(WG), 0, s>>>(
      total, d, M, queries, codebooks, out);
  return hipGetLastError();
}

/* ------------------------------------------- IVFPQ fused scan, 4-bit codes
 * k_ivfpq_scan's contract for nbits_per_idx=4 (ksub=16; DESIGN.md "4-bit
 * codes"). Entries are M/2 bytes, sub-quantizer 2b in bits 0-3 of byte b and
 * 2b+1 in bits 4-7: a little-endian word decodes in ascending m by nibbles
 * from bit 0 up. A table row is 16 floats, 16 consecutive LDS banks, so the
 * per-m gather is conflict-free. MW = M/8 code words per entry (0 = generic
 * path). Fast-path entries are 8, 16, 32 or 48 bytes in 256-B-aligned
 * buckets and load as the widest vector that divides them. */
template <int MW>
__device__ __forceinline__ void gamma_load_code4(const uint8_t *p,
                                                 uint32_t (&w)[MW]) {
  if constexpr (MW % 4 == 0) {
#pragma unroll
    for (int i = 0; i < MW / 4; i++) {
      uint4 v = ((const uint4 *)p)[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z;
      w[4 * i + 3] = v.w;
    }
  } else if constexpr (MW % 2 == 0) {
#pragma unroll
    for (int i = 0; i < MW / 2; i++) {
      uint2 v = ((const uint2 *)p)[i];
      w[2 * i] = v.x; w[2 * i + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < MW; i++) w[i] = ((const uint32_t *)p)[i];
  }
}

template <bool IP, int MW, int BS, int CP>
__global__ void __launch_bounds__(BS)
k_ivfpq_scan4(
    int nq, int S, int d, int M, int nprobe, int k2,
    const float *__restrict__ queries, const float *__restrict__ centroids,
    const float *__restrict__ codebooks, const float *__restrict__ atab,
    const float *__restrict__ probe_dists,
    const GammaBucketDev *__restrict__ buckets, int nlist,
    const int64_t *__restrict__ probes, const uint32_t *__restrict__ bitmap,
    uint64_t *__restrict__ out_keys, const int *__restrict__ kill_flag,
    const int32_t *__restrict__ qmap) {
  extern __shared__ char smem[];
  const int ksub = 16;
  const int dsub = d / M;
  float *lut = (float *)smem;                       /* M*16 (M%4==0) */
  uint64_t *sortbuf = (uint64_t *)(smem + gamma_scan4_table_bytes(M));
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(smem + gamma_scan4_qs_off(M, k2)); /* d */
  GammaScan4Tail *tl =
      (GammaScan4Tail *)(smem + gamma_scan4_tail_off(M, k2, d));

  const GammaScanBlock blk(S);
  if (blk.bq >= nq) return;
  const int sub = blk.sub;
  const int q = blk.query<true>(d, qmap, queries, qs);

  GammaSelector sel;
  sel.init(sortbuf, res, tl->state, k2);  /* has the barrier qs needs */

  if (IP)
    gamma_build_lut_ip(lut, qs, codebooks, M, 4, dsub);
  else
    gamma_copy_lut(lut, atab + (size_t)q * M * ksub, M * ksub);
  __syncthreads();

  if (MW > 0) {
    /* Two probed lists in flight per workgroup: each half of the block
     * walks one list of the pair, entry by entry, with C codes staged in
     * registers per thread between two flush checks. */
    const int C = CP;
    const int HB = BS / 2;
    const int half = threadIdx.x >= HB ? 1 : 0;
    const int tid = threadIdx.x - half * HB;
    for (int t = 0;; t += 2) {
      int p0 = sub + t * S;
      if (p0 >= nprobe) break;
      /* one thread polls the kill flag; the block reads its answer from
       * LDS behind the barrier below, so every thread leaves at the same
       * pair even when the flag flips between two threads' reads */
      if (kill_flag && threadIdx.x == 0)
        tl->kill[0] = __hip_atomic_load(kill_flag, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
      int p = sub + (t + half) * S;
      int64_t ln = -1;
      if (p < nprobe) ln = probes[(int64_t)q * nprobe + p];
      if (ln >= nlist) ln = -1;
      GammaBucketDev bk;
      bk.size = 0;
      if (ln >= 0) bk = buckets[ln];
      float dis0 = 0.0f;
      if (IP) {
        if (tid == 0) { /* dis0 = dot(q, c), canonical order, per half */
          tl->dis0[half] =
              ln >= 0 ? gamma_dot_serial(qs, centroids + (size_t)ln * d, d)
                      : 0.0f;
          tl->sz[half] = bk.size;
        }
      } else {
        if (ln >= 0 && p < nprobe)
          dis0 = probe_dists[(int64_t)q * nprobe + p];
        if (tid == 0) tl->sz[half] = bk.size;
      }
      __syncthreads();
      if (kill_flag && tl->kill[0]) break;
      if (IP) dis0 = tl->dis0[half];
      long long maxsz = tl->sz[0] > tl->sz[1] ? tl->sz[0] : tl->sz[1];
      const uint32_t *ids = bk.ids;
      const uint8_t *codes = (const uint8_t *)bk.data;
      const float *svals = (const float *)bk.svals;
      for (long long j0 = 0; j0 < maxsz; j0 += (long long)HB * C) {
        long long jb = j0 + (long long)tid * C;
        uint32_t w[C][MW ? MW : 1]; /* compile-time bounds -> registers */
        int64_t idv[C];
        float sv[C];
#pragma unroll
        for (int c = 0; c < C; c++) {
          long long j = jb + c;
          if (ln >= 0 && j < bk.size) {
            idv[c] = (int64_t)(int32_t)ids[j]; /* bit31 -> negative */
            if (!IP) sv[c] = svals[j];
            gamma_load_code4<MW ? MW : 1>(codes + (size_t)j * (MW * 4),
                                          w[c]);
          } else {
            idv[c] = -1; /* bit 63 set -> skipped below */
            sv[c] = 0.0f;
          }
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
          int64_t id = idv[c];
          if (!((uint64_t)id >> 63) &&
              !gamma_bitmap_test(bitmap, (uint64_t)id)) {
            float dis = IP ? dis0 : dis0 + sv[c];
            const float *tab = lut;
#pragma unroll
            for (int mw = 0; mw < MW; mw++)
              dis = gamma_adc4_add8(dis, tab, w[c][mw]);
            sel.push(gamma_make_key<IP>(dis, (uint32_t)id));
          }
        }
        sel.maybe_flush(blockDim.x * C);
      }
      __syncthreads(); /* the tail's dis0/sz/kill rewritten next pair */
    }
  } else {
    /* generic path, byte loads: the M/2 bytes of an entry need not be a
     * multiple of 4; byte b holds sub-quantizers 2b and 2b + 1 */
    const int csz = M >> 1;
    gamma_pq_walk_lists<IP>(
        sel, q, sub, S, d, nprobe, csz, qs, centroids, probe_dists, buckets,
        nlist, probes, bitmap, kill_flag, tl->kill, tl->dis0,
        [&](const uint8_t *entry, float dis) {
          const float *tab = lut;
          for (int b = 0; b < csz; b++) {
            uint32_t v = entry[b];
            dis += tab[v & 15u]; tab += ksub;
            dis += tab[v >> 4];  tab += ksub;
          }
          return dis;
        });
  }
  sel.finish();
  for (int i = threadIdx.x; i < k2; i += blockDim.x)
    out_keys[((int64_t)q * S + sub) * k2 + i] = res[i];
}

__global__ void k_extract_probe0(int nq, int nprobe,
                                 const int64_t *__restrict__ probes,
                                 int32_t *__restrict__ out) {
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) out[q] = (int32_t)probes[(int64_t)q * nprobe];
}

hipError_t gk::extract_probe0(hipStream_t s, int nq, int nprobe,
                              const int64_t *probes, int32_t *out) {
  k_extract_probe0<<<dim3((uint32_t)((nq + WG - 1) / WG)), dim3(WG), 0,
                     s>>>(nq, nprobe, probes, out);
  return hipGetLastError();
}

/* Launch knobs, shared by the launcher and ivfpq_scan_builds_table. 512
 * threads put 24 waves on a CU at the headline LDS/WG (the ADC gather wants
 * ~4 waves/SIMD — microarch §LDS); GAMMA_SCAN_BS=256 is for experiments. */
static int gamma_scan_bs() {
  const char *e = getenv("GAMMA_SCAN_BS");
  if (e && (atoi(e) == 256 || atoi(e) == 512)) return atoi(e);
  return 512;
}
/* GAMMA_ADC_C = codes register-staged per thread per flush interval in
 * the 4-bit fast path (1 or 2). C=1 measured fastest at BS=512 (9.06 ms vs
 * 9.84 ms for C=2 on the uniform 10M/nprobe=32 microbench, see
 * tools/adc_bench.hip). The 8-bit fast path prefetches one pass ahead over
 * the chunked flat walk instead: it accepts the knob and ignores it. */
#define GAMMA_ADC_C_DEFAULT 1
static int gamma_scan_c() {
  const char *e = getenv("GAMMA_ADC_C");
  if (e && (atoi(e) == 1 || atoi(e) == 2)) return atoi(e);
  return GAMMA_ADC_C_DEFAULT;
}
/* Run-time launch values to template arguments: gamma_pick<A, B, ...>(v, f)
 * calls f(gamma_c<X>()) for the listed X equal to v (none: returns false) */
template <int V>
using gamma_c = std::integral_constant<int, V>;
template <int... Vs, class F>
static bool gamma_pick(int v, F &&f) {
  return ((v == Vs ? (f(gamma_c<Vs>()), true) : false) || ...);
}
/* The M with a compile-time entry width MW (M/4 words at 8 bits, M/8 at 4).
 * Every other M runs MW = 0, the generic path (at BS = WG, and C = 1). */
#define GAMMA_FAST_M 16, 32, 64, 96
static bool gamma_scan_fast_m(int M) {
  for (int m : {GAMMA_FAST_M})
    if (M == m) return true;
  return false;
}
/* 8-bit fast path: one selector push per thread per flush check */
static bool gamma_scan8_fast(int M, int k2, int BS) {
  return k2 + BS <= GAMMA_SORT_CAP && gamma_scan_fast_m(M);
}

/* GAMMA_SCAN_WIDE=1 sends every 8-bit launch to k_ivfpq_scan_wide (tests,
 * tools/wide_probe.py); unset, only tables that do not fit LDS go there */
static bool gamma_scan_force_wide() {
  const char *e = getenv("GAMMA_SCAN_WIDE");
  return e && atoi(e) == 1;
}
static_assert(GAMMA_WIDE_MS == gk::IVFPQ_WIDE_MS &&
                  GAMMA_WIDE_E == gk::IVFPQ_WIDE_E,
              "kernels.h exports the wide scan's slice and tile factors");

int gk::ivfpq_wide_tile() { return gamma_scan_bs() * GAMMA_WIDE_E; }
bool gk::ivfpq_scan_is_wide(int d, int M, int ksub, int k2) {
  return ksub == 256 && (gamma_scan_force_wide() ||
                         gamma_scan8_smem(M, k2, d) > 160 * 1024);
}

bool gk::ivfpq_scan_fits(int d, int M, int ksub) {
  if (ksub == 256) /* wide kernel, inner product, largest k2 */
    return d <= IVFPQ_MAX_DIM &&
           gamma_wide_smem(GAMMA_SEL_MAX_K, d, true) <= 160 * 1024;
  /* k_ivfpq_scan4's table + query; selector scratch and tail come on top */
  return gamma_scan4_table_bytes(M) + (size_t)d * 4 <= IVFPQ4_MAX_LDS_TERM;
}

bool gk::ivfpq_scan_builds_table(int M, int ksub, int k2) {
  return ksub == 256 && !gamma_scan_force_wide() &&
         gamma_scan8_fast(M, k2, gamma_scan_bs());
}
bool gk::ivfpq_scan_reads_table(int d, int M, int ksub, int k2, bool ip) {
  return gk::ivfpq_scan_is_wide(d, M, ksub, k2) ||
         (!ip && !gk::ivfpq_scan_builds_table(M, ksub, k2));
}

/* GAMMA_FUSE_RERANK=0 keeps re-rank and sort in kernels of their own
 * (A/B runs of one build, and tests that compare the two paths) */
static bool gamma_scan_fuse_rerank() {
  const char *e = getenv("GAMMA_FUSE_RERANK");
  return !(e && e[0] == '0' && e[1] == 0);
}

/* No rule on workgroups per CU: where a 64 KB or 96 KB table leaves a
 * workgroup alone on its CU nothing hides its epilogue, and the fused
 * kernel still measured faster than scan + re-rank + sort (d = 768, M = 96:
 * profiles/README.md "Fused re-rank"). */
bool gk::ivfpq_scan_can_fuse_rerank(int d, int M, int ksub, int k2, int S) {
  if (!gamma_scan_fuse_rerank()) return false;
  if (S != 1 || ksub != 256 || M <= 0 || d <= 0 || (d & 3)) return false;
  if (k2 <= 0 || k2 > GAMMA_SEL_MAX_K) return false;
  return !gk::ivfpq_scan_is_wide(d, M, ksub, k2);
}

hipError_t gk::ivfpq_scan(
    hipStream_t s, int nq, int S, int d, int M, int ksub, int nprobe, int k2,
    const float *queries, const float *centroids, const float *codebooks,
    const float *atab, const float *cwn, const float *probe_dists,
    const GammaBucketDev *buckets, int nlist, const int64_t *probes,
    const uint32_t *bitmap, bool ip, uint64_t *out_keys, const int *kill_flag,
    const int32_t *qmap, const GammaScanRerank *rr) {
  if (ksub != 256 && ksub != 16) return hipErrorInvalidValue;
  if (rr && (!gk::ivfpq_scan_can_fuse_rerank(d, M, ksub, k2, S) ||
             rr->k <= 0 || rr->k > GAMMA_SORT_CAP || !rr->queries ||
             !rr->segs || !rr->out_dists || !rr->out_ids))
    return hipErrorInvalidValue;
  const int BS = gamma_scan_bs();
  dim3 g((uint32_t)nq * (uint32_t)S);
  if (ksub == 256 && gk::ivfpq_scan_is_wide(d, M, ksub, k2)) {
    /* sliced table: LDS does not grow with M. The push rounds need
     * k2 + block size within the selector cap. */
    if (!atab || M <= 0 || (M & 3)) return hipErrorInvalidValue;
    const int WBS = k2 + BS <= GAMMA_SORT_CAP ? BS : 256;
    if (k2 + WBS > GAMMA_SORT_CAP) return hipErrorInvalidValue;
    const size_t smem = gamma_wide_smem(k2, d, ip);
    if (smem > 160 * 1024) return hipErrorInvalidValue;
    gamma_pick<0, 1>(ip, [&](auto ipc) {
      gamma_pick<256, 512>(WBS, [&](auto bs) {
        constexpr bool IPV = decltype(ipc)::value;
        constexpr int BSV = decltype(bs)::value;
        k_ivfpq_scan_wide<IPV, BSV><<<g, dim3(BSV), smem, s>>>(
            nq, S, d, M, nprobe, k2, queries, centroids, atab, probe_dists,
            buckets, nlist, probes, bitmap, out_keys, kill_flag, qmap);
      });
    });
    return hipGetLastError();
  }
  if (ksub == 256) {
    const bool fast = gamma_scan8_fast(M, k2, BS);
    if (!ip && (fast ? !cwn : !atab)) return hipErrorInvalidValue;
    const size_t smem = gamma_scan8_smem(M, k2, d);
    if (smem > 160 * 1024) return hipErrorInvalidValue;
    const GammaScanRerank rrv = rr ? *rr : GammaScanRerank{};
    gamma_pick<0, 1>(ip, [&](auto ipc) {
      gamma_pick<0, 1>(rr != nullptr, [&](auto rrc) {
        auto launch = [&](auto mw, auto bs) {
          constexpr bool IPV = decltype(ipc)::value;
          constexpr bool RRV = decltype(rrc)::value;
          constexpr int MWV = decltype(mw)::value, BSV = decltype(bs)::value;
          k_ivfpq_scan<IPV, MWV, BSV, RRV><<<g, dim3(BSV), smem, s>>>(
              nq, S, d, M, nprobe, k2, queries, centroids, codebooks, atab,
              cwn, probe_dists, buckets, nlist, probes, bitmap, out_keys,
              kill_flag, qmap, rrv);
        };
        if (!fast) return launch(gamma_c<0>(), gamma_c<WG>());
        gamma_pick<GAMMA_FAST_M>(M, [&](auto m) {
          gamma_pick<256, 512>(BS, [&](auto bs) {
            launch(gamma_c<decltype(m)::value / 4>(), bs);
          });
        });
      });
    });
    return hipGetLastError();
  }
  /* 4-bit codes: table M*16 floats (2 KB at M=32, small next to the
   * 16 KB selector scratch); MW = M/8 words per entry */
  if (!ip && !atab) return hipErrorInvalidValue;
  const size_t smem = gamma_scan4_smem(M, k2, d);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  /* batched path needs flush margin blockDim*C inside the selector cap */
  int CSEL = gamma_scan_c();
  bool fast = (k2 + BS * CSEL) <= GAMMA_SORT_CAP && gamma_scan_fast_m(M);
  if (!((k2 + BS * CSEL) <= GAMMA_SORT_CAP)) CSEL = 1;
  gamma_pick<0, 1>(ip, [&](auto ipc) {
    auto launch = [&](auto mw, auto bs, auto c) {
      constexpr bool IPV = decltype(ipc)::value;
      constexpr int MWV = decltype(mw)::value, BSV = decltype(bs)::value;
      k_ivfpq_scan4<IPV, MWV, BSV, decltype(c)::value>
          <<<g, dim3(BSV), smem, s>>>(
              nq, S, d, M, nprobe, k2, queries, centroids, codebooks, atab,
              probe_dists, buckets, nlist, probes, bitmap, out_keys,
              kill_flag, qmap);
    };
    if (!fast) return launch(gamma_c<0>(), gamma_c<WG>(), gamma_c<1>());
    gamma_pick<GAMMA_FAST_M>(M, [&](auto m) {
      gamma_pick<256, 512>(BS, [&](auto bs) {
        gamma_pick<1, 2>(CSEL, [&](auto c) {
          launch(gamma_c<decltype(m)::value / 8>(), bs, c);
        });
      });
    });
  });
  return hipGetLastError();
}
