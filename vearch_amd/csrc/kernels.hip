/*
 * kernels.hip — hand-written gfx950 (CDNA4) kernels for the Gamma hot
 * path. No CUDA shims, no hipify output: wave64, MFMA, LDS-staged tables.
 *
 * Parity contract (DESIGN.md "Parity model"): every accumulation whose
 * value is returned to the caller uses the same sequential fmaf/add order
 * as oracle/ref_scan.c. Approximate orders (MFMA GEMM, shuffle-tree
 * reductions) are only used for candidate *selection* and are always
 * followed by the canonical re-rank.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.h"
#include "select.hpp"
#include "scan_walk.hpp"
#include "rerank_epilogue.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define WG 256  /* 4 waves of 64 */

/* ------------------------------------------------------------------ norms */
__global__ void k_row_norms(const float *__restrict__ v, int64_t n, int d,
                            float *__restrict__ norms) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *row = v + i * d;
  float acc = 0.0f;
  for (int j = 0; j < d; j++) acc = fmaf(row[j], row[j], acc);
  norms[i] = acc;
}

hipError_t gk::row_norms(hipStream_t s, const float *v, int64_t n, int d,
                         float *norms) {
  if (n == 0) return hipSuccess;
  int64_t blocks = (n + WG - 1) / WG;
  k_row_norms<<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(v, n, d, norms);
  return hipGetLastError();
}

/* ------------------------------------------------------- MFMA dot GEMM
 * D[i][j] = dot(Q_i, B_j) on v_mfma_f32_16x16x4_f32 (exact f32 chain,
 * 155 TF ceiling — guide §3). One workgroup = 4 waves stacked over 64
 * query rows x 16 base columns; k-loop over d in steps of 4.
 * Lane maps (guide §3): A[i=l&15][k=l>>4], B[k=l>>4][j=l&15];
 * D: col=l&15, row=(l>>4)*4+reg. */
__global__ void __launch_bounds__(WG)
k_dots_mfma(const float *__restrict__ Q, int nq,
            const float *__restrict__ B, int64_t n, int d,
            float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t col0 = (int64_t)blockIdx.x * 16;
  const int row0 = blockIdx.y * 64 + wave * 16;

  const int a_row = row0 + (lane & 15);     /* query row this lane loads */
  const int64_t b_row = col0 + (lane & 15); /* base row this lane loads */
  const int kk0 = lane >> 4;                /* k sub-index 0..3 */
  const bool a_ok = a_row < nq;
  const bool b_ok = b_row < n;
  const float *qa = Q + (int64_t)(a_ok ? a_row : 0) * d;
  const float *bb = B + (b_ok ? b_row : 0) * d;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kk = kk0; kk < d; kk += 4) {
    float a = a_ok ? qa[kk] : 0.0f;
    float b = b_ok ? bb[kk] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const int64_t col = col0 + (lane & 15);
  if (col >= n) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    int qi = row0 + (lane >> 4) * 4 + r;
    if (qi < nq) out[(int64_t)qi * n + col] = acc[r];
  }
}

/* LDS-tiled variant: 128x128 output tile per 4-wave workgroup, BK=32,
 * +1-float row pad for conflict-free column-slice ds_reads (guide §2
 * standard fix). Each wave owns a 64x64 sub-tile = 4x4 fragments of
 * 16x16. The MFMA accumulation stays a k-ordered f32 fmaf chain (k tiles
 * processed in order; zero-padded tails add exact 0s), so the dot values
 * are bit-identical to the simple kernel and the oracle's sequential
 * chain. */
#define GT_BM 128
#define GT_BK 32

/* Epilogue arguments of the filtered instantiation (coarse assign, see
 * gk::coarse_select): instead of storing the tile, every accumulator
 * becomes the select kernel's key and is appended to its query's
 * candidate list where it is below that query's seed threshold. */
struct GammaDotsFilter {
  const float *qnorms;    /* [nq], read when l2 */
  const float *bnorms;    /* indexed by the global column id, when l2 */
  const uint64_t *thresh; /* tau of row q at thresh[q * thresh_ld] */
  int64_t thresh_ld;
  int64_t col_base;       /* global id of B's row 0 */
  int l2;
  uint64_t *cand;         /* [nq][cap] */
  int *cand_cnt;          /* [nq], keeps counting past cap */
  int cap;
};

/* FILTER = false: the tile is stored to `out` (fp unused). FILTER = true:
 * fp's epilogue, nothing is stored to `out`. Tiles, k order and tail
 * guards are the same, so a dot is the same bits in both. */
template <bool FILTER, bool IP>
__device__ __forceinline__ void
gamma_dots_tile(const float *__restrict__ Q, int nq,
                const float *__restrict__ B, int64_t n, int d,
                float *__restrict__ out, const GammaDotsFilter &fp) {
  __shared__ float As[GT_BM][GT_BK + 1];
  __shared__ float Bs[GT_BM][GT_BK + 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 64; /* wave row offset in tile: 0/64 */
  const int wc = (wave & 1) * 64;  /* wave col offset in tile: 0/64 */
  const int row0 = blockIdx.y * GT_BM;
  const int64_t col0 = (int64_t)blockIdx.x * GT_BM;

  f32x4 acc[4][4] = {};
  /* each thread stages 16 floats of A and B per K tile: 4 rows x float4 */
  const int ld_row = threadIdx.x >> 3;        /* 0..31 */
  const int ld_col = (threadIdx.x & 7) * 4;   /* 0,4,..,28 */

  for (int k0 = 0; k0 < d; k0 += GT_BK) {
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      int r = ld_row + rr * 32;
      int a_row = row0 + r;
      int64_t b_row = col0 + r;
      int kk = k0 + ld_col;
      /* d % 4 == 0, so a 4-group never straddles the d boundary */
      float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
      if (kk < d) {
        if (a_row < nq)
          av = *(const float4 *)(Q + (int64_t)a_row * d + kk);
        if (b_row < n) bv = *(const float4 *)(B + b_row * d + kk);
      }
      As[r][ld_col + 0] = av.x;
      As[r][ld_col + 1] = av.y;
      As[r][ld_col + 2] = av.z;
      As[r][ld_col + 3] = av.w;
      Bs[r][ld_col + 0] = bv.x;
      Bs[r][ld_col + 1] = bv.y;
      Bs[r][ld_col + 2] = bv.z;
      Bs[r][ld_col + 3] = bv.w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GT_BK; kk += 4) {
      float a[4], b[4];
#pragma unroll
      for (int f = 0; f < 4; f++) {
        a[f] = As[wr + f * 16 + (lane & 15)][kk + (lane >> 4)];
        b[f] = Bs[wc + f * 16 + (lane & 15)][kk + (lane >> 4)];
      }
#pragma unroll
      for (int fi = 0; fi < 4; fi++)
#pragma unroll
        for (int fj = 0; fj < 4; fj++)
          acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a[fi], b[fj], acc[fi][fj], 0, 0, 0);
    }
    __syncthreads();
  }
  /* D mapping: col=lane&15, row=(lane>>4)*4+r (guide §3) */
  if constexpr (!FILTER) {
#pragma unroll
    for (int fi = 0; fi < 4; fi++) {
#pragma unroll
      for (int fj = 0; fj < 4; fj++) {
        int64_t col = col0 + wc + fj * 16 + (lane & 15);
        if (col >= n) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          int qi = row0 + wr + fi * 16 + (lane >> 4) * 4 + r;
          if (qi < nq) out[(int64_t)qi * n + col] = acc[fi][fj][r];
        }
      }
    }
  } else {
    /* A lane holds 4 columns x 16 rows. dist is k_select_from_dots_wave's
     * expression; key < tau is strict because ids are distinct.
     * One global atomic per passing key made this epilogue as long as the
     * k loop (a wave waited for ~40 returns one after the other), so
     * slots are handed out in two levels: every row of the tile counts
     * its passing keys in an LDS counter (a lane adds the 0..4 it holds
     * and keeps the offset it got), one thread per row reserves that many
     * slots of its query's list with a single global atomic, and the
     * lanes write their keys behind that base. Three barriers, all
     * unconditional. As is dead after the k loop's last barrier. */
    int *lcnt = (int *)&As[0][0]; /* [GT_BM]: row count, then row base */
    if (threadIdx.x < GT_BM) lcnt[threadIdx.x] = 0;
    __syncthreads();
    float bn[4];
    bool c_ok[4];
#pragma unroll
    for (int fj = 0; fj < 4; fj++) {
      int64_t col = col0 + wc + fj * 16 + (lane & 15);
      c_ok[fj] = col < n;
      bn[fj] = (fp.l2 && c_ok[fj]) ? fp.bnorms[fp.col_base + col] : 0.0f;
    }
    const uint32_t id0 = (uint32_t)(fp.col_base + col0 + wc + (lane & 15));
    auto key_of = [&](float dot, float qn, int fj) {
      float dist = fp.l2 ? fmaf(-2.0f, dot, qn + bn[fj]) : dot;
      return gamma_make_key<IP>(dist, id0 + fj * 16);
    };
    /* per row: bits 0..3 = which of the lane's columns pass, bits 8.. =
     * the lane's offset among the row's passing keys in this tile */
    uint32_t pk[4][4];
#pragma unroll
    for (int fi = 0; fi < 4; fi++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = wr + fi * 16 + (lane >> 4) * 4 + r;
        const int qi = row0 + row;
        uint32_t m = 0;
        if (qi < nq) {
          const uint64_t tau = fp.thresh[(int64_t)qi * fp.thresh_ld];
          const float qn = fp.l2 ? fp.qnorms[qi] : 0.0f;
#pragma unroll
          for (int fj = 0; fj < 4; fj++)
            if (c_ok[fj] && key_of(acc[fi][fj][r], qn, fj) < tau)
              m |= 1u << fj;
        }
        if (m) m |= (uint32_t)atomicAdd(&lcnt[row], __popc(m)) << 8;
        pk[fi][r] = m;
      }
    }
    __syncthreads();
    if (threadIdx.x < GT_BM) { /* a count > 0 is a row below nq */
      const int c = lcnt[threadIdx.x];
      if (c > 0)
        lcnt[threadIdx.x] = atomicAdd(&fp.cand_cnt[row0 + threadIdx.x], c);
    }
    __syncthreads();
#pragma unroll
    for (int fi = 0; fi < 4; fi++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t m = pk[fi][r];
        if (!m) continue;
        const int row = wr + fi * 16 + (lane >> 4) * 4 + r;
        const int qi = row0 + row;
        const float qn = fp.l2 ? fp.qnorms[qi] : 0.0f;
        uint64_t *dst = fp.cand + (int64_t)qi * fp.cap;
        int idx = lcnt[row] + (int)(m >> 8);
#pragma unroll
        for (int fj = 0; fj < 4; fj++) {
          if (!((m >> fj) & 1u)) continue;
          if (idx < fp.cap) dst[idx] = key_of(acc[fi][fj][r], qn, fj);
          idx++;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(WG)
k_dots_mfma_tiled(const float *__restrict__ Q, int nq,
                  const float *__restrict__ B, int64_t n, int d,
                  float *__restrict__ out) {
  gamma_dots_tile<false, false>(Q, nq, B, n, d, out, GammaDotsFilter{});
}

/* the same GEMM behind a device-side switch: returns at entry when
 * *run_if == 0 (coarse assign's overflow fallback; normally all of its
 * workgroups are empty) */
__global__ void __launch_bounds__(WG)
k_dots_mfma_tiled_if(const float *__restrict__ Q, int nq,
                     const float *__restrict__ B, int64_t n, int d,
                     float *__restrict__ out,
                     const int *__restrict__ run_if) {
  if (*run_if == 0) return; /* uniform: before any barrier */
  gamma_dots_tile<false, false>(Q, nq, B, n, d, out, GammaDotsFilter{});
}

/* 4 waves/SIMD like the plain kernel (its LDS allows 4 workgroups per CU):
 * without the bound the epilogue's hoisted threshold loads cost a wave */
template <bool IP>
__global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(4)))
k_dots_mfma_tiled_filter(const float *__restrict__ Q, int nq,
                         const float *__restrict__ B, int64_t n, int d,
                         GammaDotsFilter fp) {
  gamma_dots_tile<true, IP>(Q, nq, B, n, d, nullptr, fp);
}

hipError_t gk::dots_mfma(hipStream_t s, const float *Q, int nq,
                         const float *B, int64_t n, int d, float *out,
                         const int *run_if) {
  if (nq == 0 || n == 0) return hipSuccess;
  if (nq >= 64 && n >= 64) {
    dim3 grid((uint32_t)((n + GT_BM - 1) / GT_BM),
              (uint32_t)((nq + GT_BM - 1) / GT_BM));
    if (run_if)
      k_dots_mfma_tiled_if<<<grid, dim3(WG), 0, s>>>(Q, nq, B, n, d, out,
                                                     run_if);
    else
      k_dots_mfma_tiled<<<grid, dim3(WG), 0, s>>>(Q, nq, B, n, d, out);
  } else if (run_if) {
    return hipErrorInvalidValue; /* only the tiled kernel has the switch */
  } else {
    dim3 grid((uint32_t)((n + 15) / 16), (uint32_t)((nq + 63) / 64));
    k_dots_mfma<<<grid, dim3(WG), 0, s>>>(Q, nq, B, n, d, out);
  }
  return hipGetLastError();
}

/* -------------------------------------------------- select from dist rows */
template <bool IP>
__global__ void __launch_bounds__(WG)
k_select_from_dots(int nq, int64_t ncols, int64_t col_base, int64_t ld,
                   const float *__restrict__ dots,
                   const float *__restrict__ qnorms,
                   const float *__restrict__ bnorms, int l2,
                   const uint32_t *__restrict__ bitmap, int k2,
                   uint64_t *__restrict__ state_keys, int seeded) {
  extern __shared__ char smem[];
  uint64_t *sortbuf = (uint64_t *)smem;
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  int *state = (int *)(res + k2);

  const int q = blockIdx.x;
  if (q >= nq) return;
  const float *row = dots + (int64_t)q * ld;
  const float qn = l2 ? qnorms[q] : 0.0f;

  GammaSelector sel;
  sel.init(sortbuf, res, state, k2);
  if (seeded) sel.seed(state_keys + (int64_t)q * k2, k2);

  const int64_t chunk = (int64_t)blockDim.x * 2;
  for (int64_t c0 = 0; c0 < ncols; c0 += chunk) {
    int64_t cend = min(c0 + chunk, ncols);
    for (int64_t c = c0 + threadIdx.x; c < cend; c += blockDim.x) {
      int64_t id = col_base + c;
      if (gamma_bitmap_test(bitmap, (uint64_t)id)) continue;
      float dot = row[c];
      float dist = l2 ? fmaf(-2.0f, dot, qn + bnorms[id]) : dot;
      sel.push(gamma_make_key<IP>(dist, (uint32_t)id));
    }
    sel.maybe_flush(2 * blockDim.x);
  }
  sel.finish();
  for (int i = threadIdx.x; i < k2; i += blockDim.x)
    state_keys[(int64_t)q * k2 + i] = res[i];
}

/* Wave-per-query variant for small k2 (coarse assign: k2 = nprobe).
 * One block-wide selector per 4096-float row is barrier-dominated (it
 * measured 490 us/step, reading 164 MB at 334 GB/s); here each of the
 * 8 waves in a WG owns one query with a private GammaWaveSelector, so
 * the scan has no block barriers at all and flushes are rare (expected
 * pushes per wave ~ k2 * ln(ncols/k2)). Exact: same key order as the
 * block path (both validated against each other in tests). */
template <bool IP>
__device__ __forceinline__ void
gamma_select_wave(char *smem, int nq, int64_t ncols, int64_t col_base,
                  int64_t ld, const float *__restrict__ dots,
                  const float *__restrict__ qnorms,
                  const float *__restrict__ bnorms, int l2,
                  const uint32_t *__restrict__ bitmap, int k2,
                  uint64_t *__restrict__ state_keys, int seeded) {
  const int nw = 512 / 64;
  uint64_t *wb = (uint64_t *)smem;
  int *cnts = (int *)(wb + (size_t)nw * GAMMA_WSEL_CAP);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * nw + wave;
  if (q >= nq) return; /* q is wave-uniform: the whole wave exits */
  const float *row = dots + (int64_t)q * ld;
  const float qn = l2 ? qnorms[q] : 0.0f;

  GammaWaveSelector sel;
  sel.init(wb + (size_t)wave * GAMMA_WSEL_CAP, cnts + wave, k2);
  if (seeded) { /* fold previous segments' keys in (k2 <= cap here) */
    for (int i = lane; i < k2; i += 64) {
      uint64_t kk = state_keys[(int64_t)q * k2 + i];
      if (kk != GAMMA_KEY_EMPTY) {
        int idx = atomicAdd(sel.cnt, 1);
        sel.buf[sel.k + idx] = kk;
      }
    }
    sel.finish();
  }
  if ((ncols & 3) == 0 && (col_base & 3) == 0 && ((uintptr_t)row & 15) == 0) {
    /* vectorized: 4 dists (and 4 bnorms) per lane per pass — quarters
     * the serial trip count over a 16k-wide row (nlist=16384 coarse
     * assign reads 64 KB/query; the scalar loop was latency-bound) */
    const float4 *row4 = (const float4 *)row;
    for (int64_t c0 = 0; c0 < (ncols >> 2); c0 += 64) {
      int64_t c4 = c0 + lane;
      if (c4 < (ncols >> 2)) {
        int64_t id0 = col_base + c4 * 4;
        float4 d4 = row4[c4];
        float4 b4 = l2 ? *(const float4 *)(bnorms + id0)
                       : make_float4(0, 0, 0, 0);
        float dv[4] = {d4.x, d4.y, d4.z, d4.w};
        float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int t = 0; t < 4; t++) {
          int64_t id = id0 + t;
          if (!gamma_bitmap_test(bitmap, (uint64_t)id)) {
            float dist = l2 ? fmaf(-2.0f, dv[t], qn + bv[t]) : dv[t];
            sel.push(gamma_make_key<IP>(dist, (uint32_t)id));
          }
        }
      }
      sel.maybe_flush(64 * 4);
    }
  } else {
    for (int64_t c0 = 0; c0 < ncols; c0 += 64) {
      int64_t c = c0 + lane;
      if (c < ncols) {
        int64_t id = col_base + c;
        if (!gamma_bitmap_test(bitmap, (uint64_t)id)) {
          float dot = row[c];
          float dist = l2 ? fmaf(-2.0f, dot, qn + bnorms[id]) : dot;
          sel.push(gamma_make_key<IP>(dist, (uint32_t)id));
        }
      }
      sel.maybe_flush(64);
    }
  }
  sel.finish();
  for (int i = lane; i < k2; i += 64)
    state_keys[(int64_t)q * k2 + i] = sel.buf[i];
}

template <bool IP>
__global__ void __launch_bounds__(512)
k_select_from_dots_wave(int nq, int64_t ncols, int64_t col_base,
                        int64_t ld, const float *__restrict__ dots,
                        const float *__restrict__ qnorms,
                        const float *__restrict__ bnorms, int l2,
                        const uint32_t *__restrict__ bitmap, int k2,
                        uint64_t *__restrict__ state_keys, int seeded) {
  extern __shared__ char smem[];
  gamma_select_wave<IP>(smem, nq, ncols, col_base, ld, dots, qnorms, bnorms,
                        l2, bitmap, k2, state_keys, seeded);
}

/* the same select behind a device-side switch (see k_dots_mfma_tiled_if) */
template <bool IP>
__global__ void __launch_bounds__(512)
k_select_from_dots_wave_if(int nq, int64_t ncols, int64_t col_base,
                           int64_t ld, const float *__restrict__ dots,
                           const float *__restrict__ qnorms,
                           const float *__restrict__ bnorms, int l2,
                           const uint32_t *__restrict__ bitmap, int k2,
                           uint64_t *__restrict__ state_keys, int seeded,
                           const int *__restrict__ run_if) {
  extern __shared__ char smem[];
  if (*run_if == 0) return;
  gamma_select_wave<IP>(smem, nq, ncols, col_base, ld, dots, qnorms, bnorms,
                        l2, bitmap, k2, state_keys, seeded);
}

/* Coarse assign, final select (gk::coarse_select phase 3): wave per query
 * like k_select_from_dots_wave. state_keys[q] holds the sorted top-k2 of
 * the seed columns; the candidates of the filtered GEMM (all below the
 * k2-th seed) are merged in and the sorted top-k2 written back. Keys are
 * compared as they are, so the metric does not matter here. A query whose
 * counter ran past cap lost candidates: it raises *overflow, and the
 * caller's switched full-width pass then rewrites the whole group. */
__global__ void __launch_bounds__(512)
k_coarse_final_select(int nq, int k2, int cap,
                      const uint64_t *__restrict__ cand,
                      const int *__restrict__ cand_cnt,
                      uint64_t *__restrict__ state_keys,
                      int *__restrict__ overflow) {
  extern __shared__ char smem[];
  const int nw = 512 / 64;
  uint64_t *wb = (uint64_t *)smem;
  int *cnts = (int *)(wb + (size_t)nw * GAMMA_WSEL_CAP);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * nw + wave;
  if (q >= nq) return; /* q is wave-uniform: the whole wave exits */
  int m = cand_cnt[q];
  if (m > cap) {
    if (lane == 0) *overflow = 1;
    m = cap;
  }
  if (m == 0) return; /* the seeds stand as they are */

  GammaWaveSelector sel;
  sel.init(wb + (size_t)wave * GAMMA_WSEL_CAP, cnts + wave, k2);
  for (int i = lane; i < k2; i += 64) {
    uint64_t kk = state_keys[(int64_t)q * k2 + i];
    if (kk != GAMMA_KEY_EMPTY) {
      int idx = atomicAdd(sel.cnt, 1);
      sel.buf[sel.k + idx] = kk;
    }
  }
  sel.finish();
  const uint64_t *row = cand + (int64_t)q * cap;
  for (int c0 = 0; c0 < m; c0 += 64) {
    int c = c0 + lane;
    if (c < m) sel.push(row[c]);
    sel.maybe_flush(64);
  }
  sel.finish();
  for (int i = lane; i < k2; i += 64)
    state_keys[(int64_t)q * k2 + i] = sel.buf[i];
}

hipError_t gk::select_from_dots(hipStream_t s, int nq, int64_t ncols,
                                int64_t col_base, int64_t ld,
                                const float *dots, const float *qnorms,
                                const float *bnorms, bool l2, bool ip_order,
                                const uint32_t *bitmap, int k2,
                                uint64_t *state_keys, bool seeded,
                                const int *run_if) {
  /* k2 <= 192: seeds (k2 keys) plus one 64-push interval must fit the
   * wave cap (GAMMA_WSEL_CAP - k2), with slack; covers every coarse
   * assign (nprobe). Larger k2 (FLAT top-k accumulation) -> block path. */
  if (k2 <= 192) {
    const int nw = 512 / 64;
    size_t smem = (size_t)nw * GAMMA_WSEL_CAP * 8 + nw * sizeof(int);
    dim3 g((uint32_t)((nq + nw - 1) / nw));
    if (run_if) {
      if (ip_order)
        k_select_from_dots_wave_if<true><<<g, dim3(512), smem, s>>>(
            nq, ncols, col_base, ld, dots, qnorms, bnorms, l2 ? 1 : 0,
            bitmap, k2, state_keys, seeded ? 1 : 0, run_if);
      else
        k_select_from_dots_wave_if<false><<<g, dim3(512), smem, s>>>(
            nq, ncols, col_base, ld, dots, qnorms, bnorms, l2 ? 1 : 0,
            bitmap, k2, state_keys, seeded ? 1 : 0, run_if);
      return hipGetLastError();
    }
    if (ip_order)
      k_select_from_dots_wave<true><<<g, dim3(512), smem, s>>>(
          nq, ncols, col_base, ld, dots, qnorms, bnorms, l2 ? 1 : 0,
          bitmap, k2, state_keys, seeded ? 1 : 0);
    else
      k_select_from_dots_wave<false><<<g, dim3(512), smem, s>>>(
          nq, ncols, col_base, ld, dots, qnorms, bnorms, l2 ? 1 : 0,
          bitmap, k2, state_keys, seeded ? 1 : 0);
    return hipGetLastError();
  }
  if (run_if) return hipErrorInvalidValue; /* wave kernel only */
  size_t smem = (GAMMA_SORT_CAP + k2) * 8 + 4 * sizeof(int);
  if (ip_order)
    k_select_from_dots<true><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, ncols, col_base, ld, dots, qnorms, bnorms, l2 ? 1 : 0, bitmap,
        k2, state_keys, seeded ? 1 : 0);
  else
    k_select_from_dots<false><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, ncols, col_base, ld, dots, qnorms, bnorms, l2 ? 1 : 0, bitmap,
        k2, state_keys, seeded ? 1 : 0);
  return hipGetLastError();
}

/* ------------------------------------- coarse assign, seed-filtered GEMM */
/* GAMMA_FUSE_COARSE=0 keeps coarse assign on the full dots matrix (A/B
 * runs of one build, and tests that compare the two paths) */
static bool gamma_fuse_coarse() {
  const char *e = getenv("GAMMA_FUSE_COARSE");
  return !(e && e[0] == '0' && e[1] == 0);
}

/* experiment knobs: seed columns (a multiple of 128) and candidate slots
 * per query */
int gk::coarse_seed_cols() {
  const char *e = getenv("GAMMA_COARSE_SEED_COLS");
  if (e && atoi(e) > 0 && atoi(e) % GT_BM == 0) return atoi(e);
  return 4096; /* headline sweep: profiles/README.md "Coarse filter" */
}
int gk::coarse_cand_cap() {
  const char *e = getenv("GAMMA_COARSE_CAND_CAP");
  if (e && atoi(e) > 0) return atoi(e);
  return 1024;
}

bool gk::coarse_can_filter(int nq, int64_t nlist, int d, int nprobe,
                           int n1) {
  if (!gamma_fuse_coarse()) return false;
  if (n1 <= 0) n1 = gk::coarse_seed_cols();
  if (n1 % GT_BM != 0 || nprobe < 1 || nprobe > 192) return false;
  /* exactness needs no relation of n1 to nprobe; n1 >= nprobe makes the
   * threshold a real key. The default 4096 is > 4 * 192; the expected
   * candidates per query are about nprobe * (nlist / n1 - 1). */
  if (n1 < nprobe || nq < 64 || d <= 0 || (d & 3)) return false;
  return nlist >= 2 * (int64_t)n1;
}

hipError_t gk::coarse_select(hipStream_t s, const float *Q, int nq,
                             const float *B, int64_t nlist, int d,
                             const float *qnorms, const float *bnorms,
                             bool l2, bool ip_order, int nprobe, int n1,
                             int cap, float *dots, uint64_t *cand,
                             int *cand_cnt, uint64_t *sel_keys) {
  if (nq == 0 || nlist == 0) return hipSuccess;
  if (n1 <= 0) n1 = gk::coarse_seed_cols();
  if (cap <= 0) cap = gk::coarse_cand_cap();
  hipError_t e;
  if (!gk::coarse_can_filter(nq, nlist, d, nprobe, n1)) {
    e = gk::dots_mfma(s, Q, nq, B, nlist, d, dots);
    if (e != hipSuccess) return e;
    return gk::select_from_dots(s, nq, nlist, 0, nlist, dots, qnorms, bnorms,
                                l2, ip_order, nullptr, nprobe, sel_keys,
                                false);
  }
  int *overflow = cand_cnt + nq;
  e = hipMemsetAsync(cand_cnt, 0, ((size_t)nq + 1) * sizeof(int), s);
  if (e != hipSuccess) return e;
  /* 1. seeds: the exact sorted top-nprobe of the first n1 columns; its
   * last key bounds the full row's nprobe-th key from above */
  e = gk::dots_mfma(s, Q, nq, B, n1, d, dots);
  if (e != hipSuccess) return e;
  e = gk::select_from_dots(s, nq, n1, 0, n1, dots, qnorms, bnorms, l2,
                           ip_order, nullptr, nprobe, sel_keys, false);
  if (e != hipSuccess) return e;
  /* 2. the other columns: keep the keys below that bound */
  {
    const int64_t n = nlist - n1;
    GammaDotsFilter fp;
    fp.qnorms = qnorms;
    fp.bnorms = bnorms;
    fp.thresh = sel_keys + (nprobe - 1);
    fp.thresh_ld = nprobe;
    fp.col_base = n1;
    fp.l2 = l2 ? 1 : 0;
    fp.cand = cand;
    fp.cand_cnt = cand_cnt;
    fp.cap = cap;
    dim3 grid((uint32_t)((n + GT_BM - 1) / GT_BM),
              (uint32_t)((nq + GT_BM - 1) / GT_BM));
    const float *Bt = B + (size_t)n1 * d;
    if (ip_order)
      k_dots_mfma_tiled_filter<true><<<grid, dim3(WG), 0, s>>>(Q, nq, Bt, n,
                                                               d, fp);
    else
      k_dots_mfma_tiled_filter<false><<<grid, dim3(WG), 0, s>>>(Q, nq, Bt, n,
                                                                d, fp);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  /* 3. seeds + candidates -> sorted top-nprobe */
  {
    const int nw = 512 / 64;
    size_t smem = (size_t)nw * GAMMA_WSEL_CAP * 8 + nw * sizeof(int);
    k_coarse_final_select<<<dim3((uint32_t)((nq + nw - 1) / nw)), dim3(512),
                            smem, s>>>(nq, nprobe, cap, cand, cand_cnt,
                                       sel_keys, overflow);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  /* a candidate list that overflowed: the full-width pair rewrites the
   * group's keys; with the flag clear both launches are empty workgroups */
  e = gk::dots_mfma(s, Q, nq, B, nlist, d, dots, overflow);
  if (e != hipSuccess) return e;
  return gk::select_from_dots(s, nq, nlist, 0, nlist, dots, qnorms, bnorms,
                              l2, ip_order, nullptr, nprobe, sel_keys, false,
                              overflow);
}

/* ----------------------------------------------- full-sort row select */
template <bool IP>
__global__ void __launch_bounds__(512)
k_select_rows_full(int nq, int ncols, int64_t ld,
                   const float *__restrict__ dots,
                   const float *__restrict__ qnorms,
                   const float *__restrict__ bnorms, int l2, int k2,
                   float *__restrict__ out_dists,
                   int64_t *__restrict__ out_ids) {
  extern __shared__ char smem[];
  uint64_t *buf = (uint64_t *)smem;
  const int q = blockIdx.x;
  if (q >= nq) return;
  int n = 1;
  while (n < ncols || n < k2) n <<= 1;
  const float *row = dots + (int64_t)q * ld;
  const float qn = l2 ? qnorms[q] : 0.0f;
  for (int c = threadIdx.x; c < n; c += blockDim.x) {
    uint64_t key = GAMMA_KEY_EMPTY;
    if (c < ncols) {
      float dot = row[c];
      float dist = l2 ? fmaf(-2.0f, dot, qn + bnorms[c]) : dot;
      key = gamma_make_key<IP>(dist, (uint32_t)c);
    }
    buf[c] = key;
  }
  gamma_bitonic_sort(buf, n);
  for (int i = threadIdx.x; i < k2; i += blockDim.x) {
    uint64_t key = buf[i];
    out_dists[(int64_t)q * k2 + i] =
        (key == GAMMA_KEY_EMPTY) ? -1.0f : gamma_key_dist<IP>(key);
    out_ids[(int64_t)q * k2 + i] = gamma_key_id(key);
  }
}

hipError_t gk::select_rows_full(hipStream_t s, int nq, int ncols,
                                int64_t ld, const float *dots,
                                const float *qnorms, const float *bnorms,
                                bool l2, bool ip_order, int k2,
                                float *out_dists, int64_t *out_ids) {
  int n = 1;
  while (n < ncols || n < k2) n <<= 1;
  size_t smem = (size_t)n * 8;
  if (smem > 64 * 1024) return hipErrorInvalidValue;
  if (ip_order)
    k_select_rows_full<true><<<dim3(nq), dim3(512), smem, s>>>(
        nq, ncols, ld, dots, qnorms, bnorms, l2 ? 1 : 0, k2, out_dists,
        out_ids);
  else
    k_select_rows_full<false><<<dim3(nq), dim3(512), smem, s>>>(
        nq, ncols, ld, dots, qnorms, bnorms, l2 ? 1 : 0, k2, out_dists,
        out_ids);
  return hipGetLastError();
}

/* --------------------------------------------------------------- argmin */
__global__ void k_argmin_rows(int64_t nrows, int ncols,
                              const float *__restrict__ dots,
                              const float *__restrict__ qnorms,
                              const float *__restrict__ bnorms, int l2,
                              int32_t *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  const float *row = dots + i * ncols;
  float qn = l2 ? qnorms[i] : 0.0f;
  float best = INFINITY;
  int bestj = 0;
  for (int j = 0; j < ncols; j++) {
    float v = l2 ? fmaf(-2.0f, row[j], qn + bnorms[j]) : -row[j];
    if (v < best) { best = v; bestj = j; }
  }
  out[i] = bestj;
}

hipError_t gk::argmin_rows(hipStream_t s, int64_t nrows, int ncols,
                           const float *dots, const float *qnorms,
                           const float *bnorms, bool l2, int32_t *out) {
  if (nrows == 0) return hipSuccess;
  int64_t blocks = (nrows + WG - 1) / WG;
  k_argmin_rows<<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(
      nrows, ncols, dots, qnorms, bnorms, l2 ? 1 : 0, out);
  return hipGetLastError();
}

/* ------------------------------------------------------ IVFFLAT fused scan
 * Lists store raw fp32 vectors (gamma_index_ivfflat.h:63-91). One wave
 * handles one list vector per pass: 64 lanes x ceil(d/64) elements each,
 * coalesced 512 B reads at d=128, shuffle-tree reduction (selection only;
 * final distances are canonicalized by the re-rank kernel). */
template <bool IP>
__global__ void __launch_bounds__(WG)
k_ivfflat_scan(int nq, int d, int nprobe, int k2,
               const float *__restrict__ queries,
               const GammaBucketDev *__restrict__ buckets, int nlist,
               const int64_t *__restrict__ probes,
               const uint32_t *__restrict__ bitmap,
               uint64_t *__restrict__ out_keys) {
  extern __shared__ char smem[];
  uint64_t *sortbuf = (uint64_t *)smem;
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(res + k2);
  int *state = (int *)(qs + d);

  const int q = blockIdx.x;
  if (q >= nq) return;
  const float *qg = queries + (int64_t)q * d;
  for (int i = threadIdx.x; i < d; i += blockDim.x) qs[i] = qg[i];

  GammaSelector sel;
  sel.init(sortbuf, res, state, k2);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int half = lane >> 5;   /* two vectors per wave: one per half */
  const int hlane = lane & 31;

  for (int p = 0; p < nprobe; p++) {
    int64_t ln = probes[(int64_t)q * nprobe + p];
    if (ln < 0 || ln >= nlist) continue;
    GammaBucketDev bk = buckets[ln];
    const uint32_t *ids = bk.ids;
    const float *vecs = (const float *)bk.data;

    const int vpp = nwave * 2; /* vectors per WG pass */
    long long iters = (bk.size + vpp - 1) / vpp;
    for (long long it = 0; it < iters; it++) {
      long long j = it * vpp + wave * 2 + half;
      bool live = false;
      uint64_t id = 0;
      float dist = 0.0f;
      if (j < bk.size) {
        id = (uint64_t)(int64_t)(int32_t)ids[j];
        live = !(id >> 63) && !gamma_bitmap_test(bitmap, id);
        if (live) {
          /* float4 per half-wave lane: 32 x 16 B = one 512-B coalesced
           * read per vector at d=128 (selection only; the canonical
           * re-rank recomputes final distances) */
          const float4 *v4 = (const float4 *)(vecs + (size_t)j * d);
          const float4 *q4 = (const float4 *)qs;
          float acc = 0.0f;
          for (int e = hlane; e < (d >> 2); e += 32) {
            float4 a = q4[e], b = v4[e];
            if (IP) {
              acc = fmaf(a.x, b.x, acc);
              acc = fmaf(a.y, b.y, acc);
              acc = fmaf(a.z, b.z, acc);
              acc = fmaf(a.w, b.w, acc);
            } else {
              float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z,
                    dw = a.w - b.w;
              acc = fmaf(dx, dx, acc);
              acc = fmaf(dy, dy, acc);
              acc = fmaf(dz, dz, acc);
              acc = fmaf(dw, dw, acc);
            }
          }
          for (int off = 16; off > 0; off >>= 1)
            acc += __shfl_xor(acc, off, 64); /* within each 32-half */
          dist = acc;
        }
      }
      /* rotate the pushing hlane so buffers fill evenly */
      if (live && hlane == (int)(it & 31))
        sel.push(gamma_make_key<IP>(dist, (uint32_t)id));
      if ((it & 15) == 15) sel.maybe_flush(blockDim.x);
    }
    sel.maybe_flush(blockDim.x);
  }
  sel.finish();
  for (int i = threadIdx.x; i < k2; i += blockDim.x)
    out_keys[(int64_t)q * k2 + i] = res[i];
}

hipError_t gk::ivfflat_scan(hipStream_t s, int nq, int d, int nprobe, int k2,
                            const float *queries,
                            const GammaBucketDev *buckets, int nlist,
                            const int64_t *probes, const uint32_t *bitmap,
                            bool ip, uint64_t *out_keys) {
  size_t smem = (GAMMA_SORT_CAP + k2) * 8 + d * 4 + 4 * sizeof(int);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  if (ip)
    k_ivfflat_scan<true><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, d, nprobe, k2, queries, buckets, nlist, probes, bitmap,
        out_keys);
  else
    k_ivfflat_scan<false><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, d, nprobe, k2, queries, buckets, nlist, probes, bitmap,
        out_keys);
  return hipGetLastError();
}

/* ------------------------------------------------------ FLAT stream scan
 * Per-query workgroup streaming every segment (small-nq path; HBM-bound).
 * Distances here are selection-only (canonical re-rank follows). */
template <bool IP>
__global__ void __launch_bounds__(WG)
k_flat_stream(int nq, int64_t n, int d, int k2,
              const float *__restrict__ queries,
              const float *const *__restrict__ segs, int seg_shift,
              const uint32_t *__restrict__ bitmap,
              uint64_t *__restrict__ out_keys) {
  extern __shared__ char smem[];
  uint64_t *sortbuf = (uint64_t *)smem;
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(res + k2);
  int *state = (int *)(qs + d);

  const int q = blockIdx.x;
  if (q >= nq) return;
  const float *qg = queries + (int64_t)q * d;
  for (int i = threadIdx.x; i < d; i += blockDim.x) qs[i] = qg[i];

  GammaSelector sel;
  sel.init(sortbuf, res, state, k2);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t seg_mask = ((int64_t)1 << seg_shift) - 1;

  long long iters = (n + nwave - 1) / nwave;
  for (long long it = 0; it < iters; it++) {
    int64_t j = it * nwave + wave;
    bool live = false;
    float dist = 0.0f;
    if (j < n) {
      live = !gamma_bitmap_test(bitmap, (uint64_t)j);
      if (live) {
        const float2 *v2 = (const float2 *)(
            segs[j >> seg_shift] + (size_t)(j & seg_mask) * d);
        const float2 *q2 = (const float2 *)qs;
        float acc = 0.0f;
        for (int e = lane; e < (d >> 1); e += 64) {
          float2 a = q2[e], b = v2[e];
          if (IP) {
            acc = fmaf(a.x, b.x, acc);
            acc = fmaf(a.y, b.y, acc);
          } else {
            float dx = a.x - b.x, dy = a.y - b.y;
            acc = fmaf(dx, dx, acc);
            acc = fmaf(dy, dy, acc);
          }
        }
        for (int off = 32; off > 0; off >>= 1)
          acc += __shfl_xor(acc, off, 64);
        dist = acc;
      }
    }
    if (live && lane == (int)(j & 63))
      sel.push(gamma_make_key<IP>(dist, (uint32_t)j));
    if ((it & 15) == 15) sel.maybe_flush(blockDim.x);
  }
  sel.finish();
  for (int i = threadIdx.x; i < k2; i += blockDim.x)
    out_keys[(int64_t)q * k2 + i] = res[i];
}

hipError_t gk::flat_stream_scan(hipStream_t s, int nq, int64_t n, int d,
                                int k2, const float *queries,
                                const float *const *segs, int seg_shift,
                                const uint32_t *bitmap, bool ip,
                                uint64_t *out_keys) {
  size_t smem = (GAMMA_SORT_CAP + k2) * 8 + d * 4 + 4 * sizeof(int);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  if (ip)
    k_flat_stream<true><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, n, d, k2, queries, segs, seg_shift, bitmap, out_keys);
  else
    k_flat_stream<false><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, n, d, k2, queries, segs, seg_shift, bitmap, out_keys);
  return hipGetLastError();
}

/* ------------------------------------------------------------- re-rank
 * Canonical-order exact distances (matches oracle_l2sqr/oracle_ip).
 * Thread per (query, candidate); consecutive threads share the query so
 * its elements broadcast from L1. */
template <bool IP, int DV>
__global__ void k_rerank(int nq, int ncand, int d,
                         const float *__restrict__ queries,
                         const float *const *__restrict__ segs,
                         int seg_shift, const uint64_t *__restrict__ keys_in,
                         uint64_t *__restrict__ keys_out) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)nq * ncand) return;
  int q = (int)(idx / ncand);
  uint64_t key = keys_in[idx];
  if (key == GAMMA_KEY_EMPTY) { keys_out[idx] = GAMMA_KEY_EMPTY; return; }
  uint32_t id = (uint32_t)(key & 0xffffffffu);
  const int64_t seg_mask = ((int64_t)1 << seg_shift) - 1;
  const float *v = segs[id >> seg_shift] + (size_t)(id & seg_mask) * d;
  const float *qv = queries + (int64_t)q * d;
  /* float4 loads (d % 4 == 0), scalar fmaf chain in canonical order.
   * DV != 0 makes the trip count compile-time so the loads pipeline
   * ahead of the dependent fmaf chain. */
  const float4 *v4 = (const float4 *)v;
  const float4 *q4 = (const float4 *)qv;
  float acc = 0.0f;
  const int nt4 = DV ? (DV >> 2) : (d >> 2);
#pragma unroll 8
  for (int t = 0; t < nt4; t++) {
    float4 a = q4[t], b = v4[t];
    if (IP) {
      acc = fmaf(a.x, b.x, acc);
      acc = fmaf(a.y, b.y, acc);
      acc = fmaf(a.z, b.z, acc);
      acc = fmaf(a.w, b.w, acc);
    } else {
      float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z,
            dw = a.w - b.w;
      acc = fmaf(dx, dx, acc);
      acc = fmaf(dy, dy, acc);
      acc = fmaf(dz, dz, acc);
      acc = fmaf(dw, dw, acc);
    }
  }
  keys_out[idx] = gamma_make_key<IP>(acc, id);
}

/* LDS-staged re-rank (tools/rerank_bench.hip "v2": 0.354 ms vs 0.698 ms
 * for the thread-per-candidate version at nq=10k ncand=200 d=128 —
 * 2.95 TB/s algorithmic). One block per (query, candidate chunk); the
 * block stages BS candidate rows through LDS in 128 B slices with
 * 8 threads cooperating per row (coalesced float4s), then each thread
 * accumulates ITS candidate's distance from the staged slice in the
 * same canonical element order as the scalar chain — bit-identical
 * output, ~4x less time stalled on scattered row gathers. */
template <bool IP, int DV, int BS>
__global__ void __launch_bounds__(BS)
k_rerank_lds(int nq, int ncand, const float *__restrict__ queries,
             const float *const *__restrict__ segs, int n_segs,
             int seg_shift, const uint64_t *__restrict__ keys_in,
             uint64_t *__restrict__ keys_out) {
  const int CH = 32; /* floats per slice = 128 B */
  const int SEG_LDS = 64; /* seg-table cache (64 segs = 33M vectors) */
  __shared__ float rows[BS][CH + 1]; /* +1: bank-shift */
  __shared__ float qs[DV];
  __shared__ const float *seg_lds[SEG_LDS];
  const int nchunk = (ncand + BS - 1) / BS;
  const int q = blockIdx.x / nchunk;
  const int c0 = (blockIdx.x - q * nchunk) * BS;
  if (q >= nq) return;
  for (int i = threadIdx.x; i < DV; i += BS)
    qs[i] = queries[(size_t)q * DV + i];
  /* the row gathers chase segs[id>>shift] before every load; serve the
   * tiny pointer table from LDS instead of L2 */
  const bool seg_cached = n_segs <= SEG_LDS;
  if (seg_cached)
    for (int i = threadIdx.x; i < n_segs; i += BS) seg_lds[i] = segs[i];
  const int64_t seg_mask = ((int64_t)1 << seg_shift) - 1;
  const int my = c0 + threadIdx.x;
  uint64_t mykey = GAMMA_KEY_EMPTY;
  if (my < ncand) mykey = keys_in[(size_t)q * ncand + my];
  const bool live = my < ncand && mykey != GAMMA_KEY_EMPTY;
  const uint32_t myid = (uint32_t)(mykey & 0xffffffffu);
  float acc = 0.0f;
  const int f4 = threadIdx.x & 7, rg = threadIdx.x >> 3;
  for (int sl = 0; sl < DV / CH; sl++) {
    __syncthreads();
    for (int r = rg; r < BS; r += BS / 8) {
      int cand = c0 + r;
      if (cand < ncand) {
        uint64_t key = keys_in[(size_t)q * ncand + cand];
        if (key != GAMMA_KEY_EMPTY) {
          uint32_t id = (uint32_t)(key & 0xffffffffu);
          const float *v = (seg_cached ? seg_lds[id >> seg_shift]
                                       : segs[id >> seg_shift]) +
                           (size_t)(id & seg_mask) * DV;
          float4 x = *(const float4 *)(v + sl * CH + f4 * 4);
          rows[r][f4 * 4 + 0] = x.x;
          rows[r][f4 * 4 + 1] = x.y;
          rows[r][f4 * 4 + 2] = x.z;
          rows[r][f4 * 4 + 3] = x.w;
        }
      }
    }
    __syncthreads();
    if (live) {
      const float *qm = qs + sl * CH;
      const float *vm = rows[threadIdx.x];
#pragma unroll
      for (int t = 0; t < CH; t++) {
        if (IP) {
          acc = fmaf(qm[t], vm[t], acc);
        } else {
          float dx = qm[t] - vm[t];
          acc = fmaf(dx, dx, acc);
        }
      }
    }
  }
  if (my < ncand)
    keys_out[(size_t)q * ncand + my] =
        live ? gamma_make_key<IP>(acc, myid) : GAMMA_KEY_EMPTY;
}

hipError_t gk::rerank(hipStream_t s, int nq, int ncand, int d,
                      const float *queries, const float *const *segs,
                      int n_segs, int seg_shift, bool ip,
                      const uint64_t *keys_in, uint64_t *keys_out) {
  int64_t total = (int64_t)nq * ncand;
  if (total == 0) return hipSuccess;
  if (d == 128 || d == 768) {
    const int BS = 256;
    int nchunk = (ncand + BS - 1) / BS;
    dim3 g((uint32_t)((int64_t)nq * nchunk));
#define GAMMA_LAUNCH_RERANK_LDS(IPV, DVV)                                 \
  k_rerank_lds<IPV, DVV, BS><<<g, dim3(BS), 0, s>>>(                      \
      nq, ncand, queries, segs, n_segs, seg_shift, keys_in, keys_out)
    if (ip) {
      if (d == 128) GAMMA_LAUNCH_RERANK_LDS(true, 128);
      else GAMMA_LAUNCH_RERANK_LDS(true, 768);
    } else {
      if (d == 128) GAMMA_LAUNCH_RERANK_LDS(false, 128);
      else GAMMA_LAUNCH_RERANK_LDS(false, 768);
    }
#undef GAMMA_LAUNCH_RERANK_LDS
    return hipGetLastError();
  }
  int64_t blocks = (total + WG - 1) / WG;
#define GAMMA_LAUNCH_RERANK(IPV, DVV)                                     \
  k_rerank<IPV, DVV><<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(         \
      nq, ncand, d, queries, segs, seg_shift, keys_in, keys_out)
  if (ip) {
    GAMMA_LAUNCH_RERANK(true, 0);
  } else {
    GAMMA_LAUNCH_RERANK(false, 0);
  }
#undef GAMMA_LAUNCH_RERANK
  return hipGetLastError();
}

/* ------------------------------------------------------------ row sort */
template <bool IP>
__global__ void k_sort_rows(int nq, int ncand, int k,
                            const uint64_t *__restrict__ keys,
                            float *__restrict__ out_dists,
                            int64_t *__restrict__ out_ids) {
  extern __shared__ char smem[];
  uint64_t *buf = (uint64_t *)smem;
  const int q = blockIdx.x;
  if (q >= nq) return;
  int n = 1;
  while (n < ncand || n < k) n <<= 1; /* k <= n so the output reads are
                                       * always inside the padded region */
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    buf[i] = (i < ncand) ? keys[(int64_t)q * ncand + i] : GAMMA_KEY_EMPTY;
  gamma_bitonic_sort(buf, n);
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    uint64_t key = buf[i];
    out_dists[(int64_t)q * k + i] =
        (key == GAMMA_KEY_EMPTY) ? -1.0f : gamma_key_dist<IP>(key);
    out_ids[(int64_t)q * k + i] = gamma_key_id(key);
  }
}

hipError_t gk::sort_rows(hipStream_t s, int nq, int ncand, int k,
                         const uint64_t *keys, bool ip, float *out_dists,
                         int64_t *out_ids) {
  int n = 1;
  while (n < ncand || n < k) n <<= 1;
  size_t smem = (size_t)n * 8;
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  if (ip)
    k_sort_rows<true><<<dim3(nq), dim3(WG), smem, s>>>(nq, ncand, k, keys,
                                                       out_dists, out_ids);
  else
    k_sort_rows<false><<<dim3(nq), dim3(WG), smem, s>>>(nq, ncand, k, keys,
                                                        out_dists, out_ids);
  return hipGetLastError();
}

/* ----------------------------------------------------------- unpack keys */
template <bool IP>
__global__ void k_unpack(int64_t n, const uint64_t *__restrict__ keys,
                         float *__restrict__ out_dists,
                         int64_t *__restrict__ out_ids) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t key = keys[i];
  out_dists[i] = (key == GAMMA_KEY_EMPTY) ? -1.0f : gamma_key_dist<IP>(key);
  out_ids[i] = gamma_key_id(key);
}

hipError_t gk::unpack_keys(hipStream_t s, int64_t n, const uint64_t *keys,
                           bool ip, float *out_dists, int64_t *out_ids) {
  if (n == 0) return hipSuccess;
  int64_t blocks = (n + WG - 1) / WG;
  if (ip)
    k_unpack<true><<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(
        n, keys, out_dists, out_ids);
  else
    k_unpack<false><<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(
        n, keys, out_dists, out_ids);
  return hipGetLastError();
}

/* ---------------------------------------------------- pct1 ADC tables
 * KB = log2(ksub): 8 (nbits_per_idx=8) or 4 (nbits_per_idx=4). The
 * arithmetic does not depend on KB, only the table indexing does. */
template <int KB>
__global__ void k_pq_btable(int d, int M, int nlist,
                            const float *__restrict__ centroids,
                            const float *__restrict__ codebooks,
                            float *__restrict__ btab) {
  const int KSUB = 1 << KB;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)nlist * M * KSUB;
  if (e >= total) return;
  int dsub = d / M;
  int j = (int)(e & (KSUB - 1));
  int m = (int)((e >> KB) % M);
  int64_t ln = e / ((int64_t)M * KSUB);
  const float *cm = centroids + ln * d + m * dsub;
  const float *cw = codebooks + ((size_t)m * KSUB + j) * dsub;
  float dot = 0.0f;
  if ((dsub & 3) == 0) {
#pragma unroll 2
    for (int t = 0; t < dsub; t += 4) {
      float4 c4 = *(const float4 *)(cw + t);
      float4 m4 = *(const float4 *)(cm + t);
      dot = fmaf(m4.x, c4.x, dot);
      dot = fmaf(m4.y, c4.y, dot);
      dot = fmaf(m4.z, c4.z, dot);
      dot = fmaf(m4.w, c4.w, dot);
    }
  } else {
    for (int t = 0; t < dsub; t++) dot = fmaf(cm[t], cw[t], dot);
  }
  btab[e] = 2.0f * dot;
}

hipError_t gk::pq_tables_b(hipStream_t s, int d, int M, int ksub, int nlist,
                           const float *centroids, const float *codebooks,
                           float *btab) {
  if (ksub != 256 && ksub != 16) return hipErrorInvalidValue;
  int64_t total = (int64_t)nlist * M * ksub;
  dim3 g((uint32_t)((total + WG - 1) / WG));
  if (ksub == 256)
    k_pq_btable<8><<<g, dim3(WG), 0, s>>>(d, M, nlist, centroids, codebooks,
                                          btab);
  else
    k_pq_btable<4><<<g, dim3(WG), 0, s>>>(d, M, nlist, centroids, codebooks,
                                          btab);
  return hipGetLastError();
}

template <int KB>
__global__ void k_pq_atable(int nq, int d, int M,
                            const float *__restrict__ queries,
                            const float *__restrict__ codebooks,
                            float *__restrict__ atab) {
  const int KSUB = 1 << KB;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)nq * M * KSUB;
  if (e >= total) return;
  int dsub = d / M;
  int j = (int)(e & (KSUB - 1));
  int m = (int)((e >> KB) % M);
  int64_t q = e / ((int64_t)M * KSUB);
  const float *qm = queries + q * d + m * dsub;
  const float *cw = codebooks + ((size_t)m * KSUB + j) * dsub;
  float cwn = 0.0f, dot = 0.0f;
  if ((dsub & 3) == 0) { /* float4 loads, same fmaf order */
#pragma unroll 2
    for (int t = 0; t < dsub; t += 4) {
      float4 c4 = *(const float4 *)(cw + t);
      float4 q4 = *(const float4 *)(qm + t);
      cwn = fmaf(c4.x, c4.x, cwn);
      cwn = fmaf(c4.y, c4.y, cwn);
      cwn = fmaf(c4.z, c4.z, cwn);
      cwn = fmaf(c4.w, c4.w, cwn);
      dot = fmaf(q4.x, c4.x, dot);
      dot = fmaf(q4.y, c4.y, dot);
      dot = fmaf(q4.z, c4.z, dot);
      dot = fmaf(q4.w, c4.w, dot);
    }
  } else {
    for (int t = 0; t < dsub; t++) cwn = fmaf(cw[t], cw[t], cwn);
    for (int t = 0; t < dsub; t++) dot = fmaf(qm[t], cw[t], dot);
  }
  atab[e] = fmaf(-2.0f, dot, cwn);
}

hipError_t gk::pq_tables_a(hipStream_t s, int nq, int d, int M, int ksub,
                           const float *queries, const float *codebooks,
                           float *atab) {
  if (ksub != 256 && ksub != 16) return hipErrorInvalidValue;
  int64_t total = (int64_t)nq * M * ksub;
  dim3 g((uint32_t)((total + WG - 1) / WG));
  if (ksub == 256)
    k_pq_atable<8><<<g, dim3(WG), 0, s>>>(nq, d, M, queries, codebooks,
                                          atab);
  else
    k_pq_atable<4><<<g, dim3(WG), 0, s>>>(nq, d, M, queries, codebooks,
                                          atab);
  return hipGetLastError();
}

/* S = sum_m B[m][code_m], plain adds in ascending m. KB=8: one byte per
 * sub-quantizer. KB=4: packed entries of M/2 bytes, byte b = sub-quantizer
 * 2b in bits 0-3 and 2b+1 in bits 4-7 (low nibble first). */
template <int KB>
__device__ __forceinline__ float gamma_sterm_sum(const float *B,
                                                 const uint8_t *c, int M) {
  float acc = 0.0f;
  if (KB == 8) {
    for (int m = 0; m < M; m++) acc += B[(size_t)m * 256 + c[m]];
  } else {
    for (int b = 0; b < (M >> 1); b++) {
      uint32_t v = c[b];
      acc += B[(size_t)(2 * b) * 16 + (v & 15u)];
      acc += B[(size_t)(2 * b + 1) * 16 + (v >> 4)];
    }
  }
  return acc;
}

/* per-vector S term: out[i] = sum_m btab[asg_i][m][code_i[m]], plain
 * adds in m order (the oracle mirrors this exactly —
 * oracle_ivfpq_search_pct1's per-code B sum) */
template <int KB>
__global__ void k_pq_sterm(int64_t n, int M, int nlist,
                           const uint8_t *__restrict__ codes,
                           const int32_t *__restrict__ asg, int asg_const,
                           const float *__restrict__ btab,
                           float *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int ln = asg ? asg[i] : asg_const;
  if (ln < 0 || ln >= nlist) { /* defensive: matches the host-side
                                  bucket fixup for degenerate
                                  assignments (core.cpp add) */
    out[i] = 0.0f;
    return;
  }
  const float *B = btab + ((size_t)ln * M << KB);
  const uint8_t *c = codes + (size_t)i * (M * KB / 8);
  out[i] = gamma_sterm_sum<KB>(B, c, M);
}

/* Load-path batch: rebuild every bucket's S terms in one launch
 * (block per bucket) instead of one k_pq_sterm launch per bucket —
 * 16384 launches / 0.27 s of Load time at the headline nlist. */
template <int KB>
__global__ void k_pq_sterm_buckets(int nlist, int M,
                                   const GammaBucketDev *__restrict__ bks,
                                   const float *__restrict__ btab) {
  const GammaBucketDev bk = bks[blockIdx.x];
  if (!bk.svals || bk.size <= 0) return;
  const float *B = btab + ((size_t)blockIdx.x * M << KB);
  const uint8_t *codes = (const uint8_t *)bk.data;
  float *sv = (float *)bk.svals; /* writable: Load owns the buckets */
  for (long long j = threadIdx.x; j < bk.size; j += blockDim.x)
    sv[j] = gamma_sterm_sum<KB>(B, codes + (size_t)j * (M * KB / 8), M);
}

hipError_t gk::pq_sterm_buckets(hipStream_t s, int nlist, int M, int ksub,
                                const GammaBucketDev *bks,
                                const float *btab) {
  if (ksub != 256 && ksub != 16) return hipErrorInvalidValue;
  if (nlist <= 0) return hipSuccess;
  if (ksub == 256)
    k_pq_sterm_buckets<8><<<dim3((uint32_t)nlist), dim3(256), 0, s>>>(
        nlist, M, bks, btab);
  else
    k_pq_sterm_buckets<4><<<dim3((uint32_t)nlist), dim3(256), 0, s>>>(
        nlist, M, bks, btab);
  return hipGetLastError();
}

hipError_t gk::pq_sterm(hipStream_t s, int64_t n, int M, int ksub, int nlist,
                        const uint8_t *codes, const int32_t *asg,
                        int asg_const, const float *btab, float *out) {
  if (ksub != 256 && ksub != 16) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  dim3 g((uint32_t)((n + WG - 1) / WG));
  if (ksub == 256)
    k_pq_sterm<8><<<g, dim3(WG), 0, s>>>(n, M, nlist, codes, asg, asg_const,
                                         btab, out);
  else
    k_pq_sterm<4><<<g, dim3(WG), 0, s>>>(n, M, nlist, codes, asg, asg_const,
                                         btab, out);
  return hipGetLastError();
}

/* ------------------------------------------------------ bucket scatter */
__global__ void k_bucket_scatter(int nseg,
                                 const GammaScatterSeg *__restrict__ segs,
                                 const uint32_t *__restrict__ ids_src,
                                 const uint8_t *__restrict__ data_src,
                                 const float *__restrict__ svals_src,
                                 int entry_bytes) {
  const GammaScatterSeg sg = segs[blockIdx.x];
  for (long long i = threadIdx.x; i < sg.count; i += blockDim.x) {
    sg.ids_dst[i] = ids_src[sg.src_start + i];
    if (sg.sval_dst && svals_src)
      sg.sval_dst[i] = svals_src[sg.src_start + i];
  }
  /* entry payloads as u32 words when aligned, bytes otherwise */
  long long total = sg.count * entry_bytes;
  const uint8_t *src = data_src + sg.src_start * entry_bytes;
  if ((entry_bytes & 3) == 0) {
    const uint32_t *s4 = (const uint32_t *)src;
    uint32_t *d4 = (uint32_t *)sg.data_dst;
    for (long long i = threadIdx.x; i < (total >> 2); i += blockDim.x)
      d4[i] = s4[i];
  } else {
    for (long long i = threadIdx.x; i < total; i += blockDim.x)
      sg.data_dst[i] = src[i];
  }
}

hipError_t gk::bucket_scatter(hipStream_t s, int nseg,
                              const GammaScatterSeg *segs_dev,
                              const uint32_t *ids_src,
                              const uint8_t *data_src,
                              const float *svals_src, int entry_bytes) {
  if (nseg <= 0) return hipSuccess;
  k_bucket_scatter<<<dim3((uint32_t)nseg), dim3(256), 0, s>>>(
      nseg, segs_dev, ids_src, data_src, svals_src, entry_bytes);
  return hipGetLastError();
}

/* ------------------------------------------------------ bucket compact
 * Stable out-of-place compaction of IVF lists (CompactBucket/CompactOne,
 * realtime_mem_data.cc:94-146). One workgroup per segment walks the list
 * in tiles of WG entries. Per tile: each lane decides keep for its own
 * entry (mark bit 31 clear and docid bitmap clear), the wave ballot gives
 * the in-wave rank (popcount of the lower lanes), wave totals meet in LDS
 * and a running base is carried across tiles, so survivor j of the list
 * lands at slot j. Ids and S terms are written by the owning lane.
 * Payloads move as units of T (the widest word dividing entry_bytes);
 * G = 1 << gshift lanes (the power of two covering one entry's units,
 * capped at the wave) copy one entry together and 64/G entries go per
 * pass, survivors taken in rank order through a per-wave rank -> lane
 * table in LDS — small PQ entries are one unit per lane, an IVFFLAT row
 * is streamed by the whole wave. Both LDS arrays are double-buffered on
 * tile parity so one barrier per tile is enough. */
template <class T>
__global__ void __launch_bounds__(WG)
k_bucket_compact(int nseg, const GammaCompactSeg *__restrict__ segs,
                 const uint32_t *__restrict__ bitmap, int entry_bytes,
                 int gshift) {
  __shared__ int wtot[2][WG / 64];
  __shared__ uint8_t src_lane[2][WG / 64][64];
  const GammaCompactSeg sg = segs[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int units = entry_bytes / (int)sizeof(T);
  const int slot = lane >> gshift;            /* entry slot in a pass */
  const int sub = lane & ((1 << gshift) - 1); /* unit lane in the entry */
  const int per_pass = 64 >> gshift;
  long long base = 0;
  int par = 0;
  for (long long t0 = 0; t0 < sg.size; t0 += WG, par ^= 1) {
    const long long i = t0 + threadIdx.x;
    uint32_t id = 0x80000000u;
    if (i < sg.size) id = sg.ids_src[i];
    const bool keep =
        !(id & 0x80000000u) && !gamma_bitmap_test(bitmap, (uint64_t)id);
    const unsigned long long m = __ballot(keep);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    const int wkept = __popcll(m);
    if (keep) src_lane[par][wave][rank] = (uint8_t)lane;
    if (lane == 0) wtot[par][wave] = wkept;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < WG / 64; w++) {
      int c = wtot[par][w];
      if (w < wave) before += c;
      total += c;
    }
    const long long wbase = base + before;
    if (keep) {
      sg.ids_dst[wbase + rank] = id;
      if (sg.svals_dst && sg.svals_src)
        sg.svals_dst[wbase + rank] = sg.svals_src[i];
    }
    for (int r = slot; r < wkept; r += per_pass) {
      const long long si = t0 + wave * 64 + src_lane[par][wave][r];
      const T *s = (const T *)(sg.data_src + si * entry_bytes);
      T *d = (T *)(sg.data_dst + (wbase + r) * entry_bytes);
      for (int j = sub; j < units; j += 1 << gshift) d[j] = s[j];
    }
    base += total;
  }
  if (threadIdx.x == 0) *sg.kept_out = base;
}

hipError_t gk::bucket_compact(hipStream_t s, int nseg,
                              const GammaCompactSeg *segs_dev,
                              const uint32_t *bitmap, int entry_bytes) {
  if (entry_bytes <= 0) return hipErrorInvalidValue;
  if (nseg <= 0) return hipSuccess;
  const int wbytes = (entry_bytes % 16 == 0)  ? 16
                     : (entry_bytes % 8 == 0) ? 8
                     : (entry_bytes % 4 == 0) ? 4
                                              : 1;
  int gshift = 0;
  while (gshift < 6 && (1 << gshift) < entry_bytes / wbytes) gshift++;
  dim3 g((uint32_t)nseg), b(WG);
  if (wbytes == 16)
    k_bucket_compact<uint4><<<g, b, 0, s>>>(nseg, segs_dev, bitmap,
                                            entry_bytes, gshift);
  else if (wbytes == 8)
    k_bucket_compact<uint2><<<g, b, 0, s>>>(nseg, segs_dev, bitmap,
                                            entry_bytes, gshift);
  else if (wbytes == 4)
    k_bucket_compact<uint32_t><<<g, b, 0, s>>>(nseg, segs_dev, bitmap,
                                               entry_bytes, gshift);
  else
    k_bucket_compact<uint8_t><<<g, b, 0, s>>>(nseg, segs_dev, bitmap,
                                              entry_bytes, gshift);
  return hipGetLastError();
}

/* ----------------------------------------------------------- residuals */
__global__ void k_residuals(int64_t n, int d, const float *__restrict__ x,
                            const float *__restrict__ centroids,
                            const int32_t *__restrict__ assign,
                            float *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  int64_t row = i / d;
  int col = (int)(i - row * d);
  out[i] = x[i] - centroids[(size_t)assign[row] * d + col];
}

hipError_t gk::residuals(hipStream_t s, int64_t n, int d, const float *x,
                         const float *centroids, const int32_t *assign,
                         float *out) {
  if (n == 0) return hipSuccess;
  int64_t blocks = (n * d + WG - 1) / WG;
  k_residuals<<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(n, d, x, centroids,
                                                          assign, out);
  return hipGetLastError();
}

/* ----------------------------------------------------------- PQ encode */
/* argmin_j ||xm - cb[j]||^2, sequential fmaf, ties -> lowest j */
__device__ __forceinline__ int gamma_pq_argmin(const float *xm,
                                               const float *cb, int ksub,
                                               int dsub) {
  float best = INFINITY;
  int bestj = 0;
  for (int j = 0; j < ksub; j++) {
    const float *cw = cb + (size_t)j * dsub;
    float acc = 0.0f;
    for (int t = 0; t < dsub; t++) {
      float diff = xm[t] - cw[t];
      acc = fmaf(diff, diff, acc);
    }
    if (acc < best) { best = acc; bestj = j; }
  }
  return bestj;
}

__global__ void k_pq_encode(int64_t n, int d, int M, int ksub,
                            const float *__restrict__ x,
                            const float *__restrict__ codebooks,
                            uint8_t *__restrict__ codes) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * M) return;
  int64_t i = idx / M;
  int m = (int)(idx - i * M);
  int dsub = d / M;
  codes[idx] = (uint8_t)gamma_pq_argmin(
      x + i * d + m * dsub, codebooks + (size_t)m * ksub * dsub, ksub, dsub);
}

hipError_t gk::pq_encode(hipStream_t s, int64_t n, int d, int M, int ksub,
                         const float *x, const float *codebooks,
                         uint8_t *codes) {
  if (n == 0) return hipSuccess;
  int64_t blocks = (n * M + WG - 1) / WG;
  k_pq_encode<<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(n, d, M, ksub, x,
                                                          codebooks, codes);
  return hipGetLastError();
}

/* 4-bit ingest encode: one thread per output byte = two sub-quantizers
 * (2b in bits 0-3, 2b+1 in bits 4-7), same argmin as k_pq_encode */
__global__ void k_pq_encode_pack4(int64_t n, int d, int M,
                                  const float *__restrict__ x,
                                  const float *__restrict__ codebooks,
                                  uint8_t *__restrict__ codes) {
  const int nb = M >> 1;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * nb) return;
  int64_t i = idx / nb;
  int m = (int)(idx - i * nb) * 2;
  int dsub = d / M;
  const float *xm = x + i * d + m * dsub;
  const float *cb = codebooks + (size_t)m * 16 * dsub;
  int lo = gamma_pq_argmin(xm, cb, 16, dsub);
  int hi = gamma_pq_argmin(xm + dsub, cb + (size_t)16 * dsub, 16, dsub);
  codes[idx] = (uint8_t)(lo | (hi << 4));
}

hipError_t gk::pq_encode_pack4(hipStream_t s, int64_t n, int d, int M,
                               const float *x, const float *codebooks,
                               uint8_t *codes) {
  if (M & 1) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  int64_t blocks = (n * (M >> 1) + WG - 1) / WG;
  k_pq_encode_pack4<<<dim3((uint32_t)blocks), dim3(WG), 0, s>>>(
      n, d, M, x, codebooks, codes);
  return hipGetLastError();
}

/* IVFPQ: tables, the three fused scans, their launcher and knobs */
#include "ivfpq_scan_kernels.hpp"

/* BINARYIVF: Hamming matrix, list scan, flat scan */
#include "binary_kernels.hpp"

/* IVFRABITQ: encode, sval rebuild, list scan */
#include "rabitq_kernels.hpp"
