/*
 * filter_first_kernels.hpp — the filter-first plan's two kernels (included
 * from kernels.hip; DESIGN.md "Filter-first").
 *
 * gk::bitmap_candidates turns an exclusion bitmap into the ascending list of
 * the ids it keeps; gk::cand_scan computes the exact distance of every
 * (query, candidate) pair of nq queries x ONE shared candidate list, in
 * gk::rerank's own fmaf chain, and writes the keys as an nq x ncand_pad
 * matrix for gk::select_deep.
 */
#pragma once

/* ------------------------------------------------------ bitmap_candidates
 * Ordered stream compaction in three launches. A block of 256 threads owns
 * BITMAP_CAND_BLOCK = 8192 ids = 256 bitmap words, one word per thread.
 *   1. k_bmc_count: keep[w] = ~bitmap[w] with the bits at or beyond n
 *      cleared; block_cnt[b] = popcount of the block's 256 keep words.
 *   2. k_bmc_scan: one workgroup turns block_cnt into exclusive offsets in
 *      place (1024 counts per step, carry between steps), *count = total.
 *   3. k_bmc_scatter: wave w of a block owns 64 consecutive words; a wave
 *      scan of their popcounts gives every word's offset. The wave then
 *      walks its 2048 ids 64 at a time: lane l owns id base + l, the two
 *      keep words of the step ARE the wave's ballot, and the lane's slot is
 *      the popcount of the ballot below it. A step's stores are one
 *      contiguous ascending run. Slots at or beyond cap are not written. */
#define GAMMA_BMC_BS 256

__device__ __forceinline__ uint32_t gamma_bmc_keep(
    const uint32_t *__restrict__ bitmap, int64_t w, int64_t words,
    int64_t n) {
  if (w >= words) return 0u;
  uint32_t keep = ~bitmap[w];
  const int64_t left = n - w * 32; /* ids of this word that are < n */
  if (left < 32) keep &= (1u << (int)left) - 1u;
  return keep;
}

/* inclusive scan of v over the 64 lanes of a wave */
__device__ __forceinline__ uint32_t gamma_wave_incl_scan(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

__global__ void __launch_bounds__(GAMMA_BMC_BS)
k_bmc_count(const uint32_t *__restrict__ bitmap, int64_t words, int64_t n,
            uint32_t *__restrict__ block_cnt) {
  __shared__ uint32_t wsum[GAMMA_BMC_BS / 64];
  const int64_t w = (int64_t)blockIdx.x * GAMMA_BMC_BS + threadIdx.x;
  const uint32_t c = gamma_wave_incl_scan(
      (uint32_t)__popc(gamma_bmc_keep(bitmap, w, words, n)));
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    block_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(1024)
k_bmc_scan(int nblocks, uint32_t *__restrict__ block_cnt,
           int *__restrict__ count) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += 1024) {
    const int i = base + threadIdx.x;
    const uint32_t v = i < nblocks ? block_cnt[i] : 0u;
    const uint32_t inc = gamma_wave_incl_scan(v);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t before = carry;
    for (int j = 0; j < (int)(threadIdx.x >> 6); j++) before += wsum[j];
    if (i < nblocks) block_cnt[i] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = (int)carry;
}

__global__ void __launch_bounds__(GAMMA_BMC_BS)
k_bmc_scatter(const uint32_t *__restrict__ bitmap, int64_t words, int64_t n,
              const uint32_t *__restrict__ block_off,
              uint32_t *__restrict__ out_ids, int64_t cap) {
  __shared__ uint32_t wsum[GAMMA_BMC_BS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * GAMMA_BMC_BS + wave * 64;
  const uint32_t keep = gamma_bmc_keep(bitmap, w0 + lane, words, n);
  const uint32_t pc = (uint32_t)__popc(keep);
  const uint32_t inc = gamma_wave_incl_scan(pc);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t off = block_off[blockIdx.x];
  for (int j = 0; j < wave; j++) off += wsum[j];
  const uint32_t excl = inc - pc; /* offset of this lane's word in the wave */
  const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll 4
  for (int i = 0; i < 32; i++) { /* words 2i, 2i+1 of the wave = 64 ids */
    const uint32_t lo = __shfl(keep, 2 * i, 64);
    const uint32_t hi = __shfl(keep, 2 * i + 1, 64);
    const uint32_t at = __shfl(excl, 2 * i, 64);
    const uint64_t ballot = ((uint64_t)hi << 32) | lo;
    if ((ballot >> lane) & 1) {
      const int64_t slot = (int64_t)off + at + __popcll(ballot & below);
      if (slot < cap)
        out_ids[slot] = (uint32_t)((w0 + 2 * i) * 32 + lane);
    }
  }
}

hipError_t gk::bitmap_candidates(hipStream_t s, const uint32_t *bitmap,
                                 int64_t n, uint32_t *out_ids, int64_t cap,
                                 uint32_t *block_tmp, int *count) {
  if (n < 0 || n > 0x7fffffffll || cap < 0 || !count)
    return hipErrorInvalidValue;
  const int64_t words = (n + 31) / 32;
  const int nblocks = (int)((words + GAMMA_BMC_BS - 1) / GAMMA_BMC_BS);
  static_assert(GAMMA_BMC_BS * 32 == BITMAP_CAND_BLOCK, "ids per block");
  if (nblocks > 0) {
    if (!bitmap || !block_tmp || (cap > 0 && !out_ids))
      return hipErrorInvalidValue;
    k_bmc_count<<<dim3(nblocks), dim3(GAMMA_BMC_BS), 0, s>>>(bitmap, words, n,
                                                              block_tmp);
  }
  k_bmc_scan<<<dim3(1), dim3(1024), 0, s>>>(nblocks, block_tmp, count);
  if (nblocks > 0 && cap > 0)
    k_bmc_scatter<<<dim3(nblocks), dim3(GAMMA_BMC_BS), 0, s>>>(
        bitmap, words, n, block_tmp, out_ids, cap);
  return hipGetLastError();
}

/* --------------------------------------------------------------- cand_scan
 * One workgroup of 256 threads owns a tile of TQ queries x TC candidates and
 * walks d in slices of CS_DS = 32 elements (128 B of every row).
 *
 * Movement. Eight threads cooperate on a row: thread (row, f4) loads the
 * row's float4 f4 of the slice, so a row's slice is one coalesced 128 B
 * read; candidate rows are gathered through the segment table (served from
 * LDS when it fits). The loads of slice sl + 1 are issued into registers
 * before the FMAs of slice sl, and go to LDS after them. A candidate row is
 * therefore read once per query TILE.
 *
 * LDS. Both operands are stored transposed, [t][row], with a row pitch of
 * T + 4 floats: thread (tq, tc) reads its RQ = 4 query values and its RC
 * candidate values of element t as one 16-byte (RC = 4) or 8-byte (RC = 2)
 * read each. Across a wave the candidate reads are consecutive addresses and
 * the query reads are broadcasts, so no read conflicts.
 *
 * Arithmetic. Pair (q, c) has one accumulator, updated once per element t
 * in increasing t from 0.0f by the very expression of k_rerank:
 *   IP: acc = fmaf(q[t], v[t], acc)     L2: dx = q[t] - v[t];
 *                                           acc = fmaf(dx, dx, acc)
 * which makes the keys bit-identical to gk::rerank's whatever the tile shape.
 *
 * Two shapes: RQ x RC = 4 x 4 pairs per thread on a 16 x 16 thread grid
 * (64 x 64 tile) and, for batches of at most CS_NARROW_NQ queries, 4 x 2
 * pairs on a 2 x 128 grid (8 x 256 tile): the same LDS, four times the
 * workgroups per query row. */
#define GAMMA_CS_BS 256
#define GAMMA_CS_DS 32
#define GAMMA_CS_SEG_LDS 64

template <bool IP, int RC, int TXQ>
__global__ void __launch_bounds__(GAMMA_CS_BS)
k_cand_scan(int nq, int ncand, int64_t ncand_pad, int d,
            const float *__restrict__ queries,
            const uint32_t *__restrict__ cand,
            const float *const *__restrict__ segs, int n_segs, int seg_shift,
            uint64_t *__restrict__ out_keys) {
  constexpr int RQ = 4, DS = GAMMA_CS_DS, BS = GAMMA_CS_BS;
  constexpr int TXC = BS / TXQ;          /* threads along the candidates */
  constexpr int TQ = RQ * TXQ, TC = RC * TXC;
  constexpr int LDQ = TQ + 4, LDC = TC + 4;
  constexpr int RPP = BS / 8;            /* rows staged per pass: 32 */
  constexpr int NPQ = (TQ + RPP - 1) / RPP, NPC = TC / RPP;
  static_assert(TC % RPP == 0, "candidate tile in whole staging passes");
  __shared__ __attribute__((aligned(16))) float qs[DS * LDQ];
  __shared__ __attribute__((aligned(16))) float cs[DS * LDC];
  __shared__ const float *seg_lds[GAMMA_CS_SEG_LDS];

  const int tid = threadIdx.x;
  const int q0 = blockIdx.y * TQ;
  const int64_t c0 = (int64_t)blockIdx.x * TC;
  const int f4 = tid & 7, rg = tid >> 3;
  const bool seg_cached = n_segs <= GAMMA_CS_SEG_LDS;
  if (seg_cached)
    for (int i = tid; i < n_segs; i += BS) seg_lds[i] = segs[i];
  __syncthreads();

  /* the rows this thread stages: their base pointers, null = no row */
  const float *qrow[NPQ];
  const float *crow[NPC];
  const int64_t seg_mask = ((int64_t)1 << seg_shift) - 1;
#pragma unroll
  for (int p = 0; p < NPQ; p++) {
    const int r = rg + p * RPP;
    qrow[p] = (r < TQ && q0 + r < nq) ? queries + (size_t)(q0 + r) * d
                                      : nullptr;
  }
#pragma unroll
  for (int p = 0; p < NPC; p++) {
    const int64_t c = c0 + rg + p * RPP;
    crow[p] = nullptr;
    if (c < ncand) {
      const uint32_t id = cand[c];
      const uint32_t sg = id >> seg_shift;
      if (sg < (uint32_t)n_segs)
        crow[p] = (seg_cached ? seg_lds[sg] : segs[sg]) +
                  (size_t)(id & seg_mask) * d;
    }
  }

  float4 qreg[NPQ], creg[NPC];
  auto fetch = [&](int sl) {
    const int t = sl * DS + f4 * 4;
#pragma unroll
    for (int p = 0; p < NPQ; p++) {
      qreg[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qrow[p] && t < d) qreg[p] = *(const float4 *)(qrow[p] + t);
    }
#pragma unroll
    for (int p = 0; p < NPC; p++) {
      creg[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (crow[p] && t < d) creg[p] = *(const float4 *)(crow[p] + t);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int p = 0; p < NPQ; p++) {
      const int r = rg + p * RPP;
      if (r < TQ) {
        qs[(f4 * 4 + 0) * LDQ + r] = qreg[p].x;
        qs[(f4 * 4 + 1) * LDQ + r] = qreg[p].y;
        qs[(f4 * 4 + 2) * LDQ + r] = qreg[p].z;
        qs[(f4 * 4 + 3) * LDQ + r] = qreg[p].w;
      }
    }
#pragma unroll
    for (int p = 0; p < NPC; p++) {
      const int r = rg + p * RPP;
      cs[(f4 * 4 + 0) * LDC + r] = creg[p].x;
      cs[(f4 * 4 + 1) * LDC + r] = creg[p].y;
      cs[(f4 * 4 + 2) * LDC + r] = creg[p].z;
      cs[(f4 * 4 + 3) * LDC + r] = creg[p].w;
    }
  };

  const int tc = tid % TXC, tq = tid / TXC;
  float acc[RQ][RC];
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RC; j++) acc[i][j] = 0.0f;
  auto step = [&](int t) {
    float qv[RQ], cv[RC];
    const float4 a = *(const float4 *)(qs + t * LDQ + tq * RQ);
    qv[0] = a.x; qv[1] = a.y; qv[2] = a.z; qv[3] = a.w;
    if constexpr (RC == 4) {
      const float4 b = *(const float4 *)(cs + t * LDC + tc * RC);
      cv[0] = b.x; cv[1] = b.y; cv[2] = b.z; cv[3] = b.w;
    } else {
      const float2 b = *(const float2 *)(cs + t * LDC + tc * RC);
      cv[0] = b.x; cv[1] = b.y;
    }
#pragma unroll
    for (int i = 0; i < RQ; i++)
#pragma unroll
      for (int j = 0; j < RC; j++) {
        if (IP) {
          acc[i][j] = fmaf(qv[i], cv[j], acc[i][j]);
        } else {
          const float dx = qv[i] - cv[j];
          acc[i][j] = fmaf(dx, dx, acc[i][j]);
        }
      }
  };

  const int nsl = (d + DS - 1) / DS;
  fetch(0);
  for (int sl = 0; sl < nsl; sl++) {
    __syncthreads(); /* the previous slice's reads are done */
    stage();
    __syncthreads();
    if (sl + 1 < nsl) fetch(sl + 1);
    const int nt = min(DS, d - sl * DS);
    if (nt == DS) {
#pragma unroll
      for (int t = 0; t < DS; t++) step(t);
    } else {
      for (int t = 0; t < nt; t++) step(t);
    }
  }

  /* the thread's RC keys of a query are consecutive: a wave's stores of one
   * query row are one contiguous run */
  uint32_t ids[RC];
#pragma unroll
  for (int j = 0; j < RC; j++) {
    const int64_t c = c0 + tc * RC + j;
    ids[j] = c < ncand ? cand[c] : 0u;
  }
#pragma unroll
  for (int i = 0; i < RQ; i++) {
    const int q = q0 + tq * RQ + i;
    if (q >= nq) continue;
    uint64_t *row = out_keys + (size_t)q * ncand_pad;
#pragma unroll
    for (int j = 0; j < RC; j++) {
      const int64_t c = c0 + tc * RC + j;
      if (c >= ncand_pad) continue;
      const bool real =
          c < ncand && (ids[j] >> seg_shift) < (uint32_t)n_segs;
      row[c] = real ? gamma_make_key<IP>(acc[i][j], ids[j]) : GAMMA_KEY_EMPTY;
    }
  }
}

hipError_t gk::cand_scan(hipStream_t s, int nq, int ncand, int64_t ncand_pad,
                         int d, const float *queries, const uint32_t *cand,
                         const float *const *segs, int n_segs, int seg_shift,
                         bool ip, uint64_t *out_keys) {
  if (nq < 0 || ncand < 0 || ncand_pad < ncand || d <= 0 || d % 4 != 0 ||
      n_segs < 0 || seg_shift < 0 || seg_shift > 31)
    return hipErrorInvalidValue;
  if (nq == 0 || ncand_pad == 0) return hipSuccess;
  const bool narrow = nq <= CAND_SCAN_NARROW_NQ;
  const int TC = narrow ? CAND_SCAN_PAD : 64, TQ = narrow ? 8 : 64;
  const int64_t gx = (ncand_pad + TC - 1) / TC, gy = (nq + TQ - 1) / TQ;
  if (gx > 0x7fffffffll || gy > 65535) return hipErrorInvalidValue;
  const dim3 g((uint32_t)gx, (uint32_t)gy), b(GAMMA_CS_BS);
#define GAMMA_LAUNCH_CAND_SCAN(IPV, RCV, TXQV)                               \
  k_cand_scan<IPV, RCV, TXQV><<<g, b, 0, s>>>(nq, ncand, ncand_pad, d,       \
                                              queries, cand, segs, n_segs,   \
                                              seg_shift, out_keys)
  if (narrow) {
    if (ip) GAMMA_LAUNCH_CAND_SCAN(true, 2, 2);
    else GAMMA_LAUNCH_CAND_SCAN(false, 2, 2);
  } else {
    if (ip) GAMMA_LAUNCH_CAND_SCAN(true, 4, 16);
    else GAMMA_LAUNCH_CAND_SCAN(false, 4, 16);
  }
#undef GAMMA_LAUNCH_CAND_SCAN
  return hipGetLastError();
}
