/*
 * rerank_epilogue.hpp — exact re-rank + final top-k of ONE query, run by the
 * scan workgroup that selected the query's candidates (device function; no
 * launch of its own). It does to the block's sorted top-k2 what gk::rerank
 * followed by gk::sort_rows do to a row of out_keys, bit for bit:
 *   - every non-empty key's vector is gathered from the raw store through
 *     the segment table and its distance to the RAW query recomputed in
 *     k_rerank's element order: one serial chain per candidate over
 *     t = 0..d-1, L2 `dx = q[t]-v[t]; acc = fmaf(dx,dx,acc)`, inner product
 *     `acc = fmaf(q[t],v[t],acc)`; the key becomes gamma_make_key<IP>(acc,id);
 *   - empty keys stay GAMMA_KEY_EMPTY;
 *   - the k2 keys, padded to a power of two >= max(k2, k), are sorted under
 *     the (dist, id) total order and the first k written as k_sort_rows
 *     writes them (-1.0 / -1 for an empty key).
 *
 * It uses no LDS of its own. The caller hands it regions that are dead once
 * the scan loop and the selector's finish() are behind the block:
 *   stage   the query table's floats — row staging, (CH+1)-float rows
 *   qs      the scan's query copy    — overwritten with the raw query
 *   sortbuf the selector's scratch   — the final sort (GAMMA_SORT_CAP keys)
 * `res` (the sorted top-k2) is only read.
 *
 * Shape of the work (k_rerank_lds's, which measured 2x faster than a thread
 * per candidate on scattered 512-B rows): 8 threads fetch one 128-B slice of
 * a candidate's row as float4s, so a wave's load covers 8 rows x 128 B of
 * whole cache lines; the slice goes through LDS to the ONE thread that owns
 * the candidate's chain. A round serves R candidates, R = what fits the
 * staging (and at most NL*BS/8, the rows the block's NL loads per thread
 * cover); a step is one slice of one round.
 * Pipelining: the loads of step s+1 (all NL of a thread) are issued into a
 * second register set before step s is staged and computed, in
 * straight-line code — an item that has no row (past k2, an empty key, the
 * step past the last) reads the query row instead of branching around its
 * load, so the wait in front of the staging stores is a counted vmcnt that
 * leaves the prefetch in flight. The loop is unrolled by two so the sets
 * alternate without copies. Row pointers are looked up once per round.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "select.hpp"

#define GAMMA_RR_CH 32 /* floats of a row per slice = one 128-B line */
#define GAMMA_RR_NL 4  /* float4 loads per thread per slice */

/* candidates per round at `stage_floats` floats of staging */
__host__ __device__ static inline int gamma_rr_round_rows(int stage_floats,
                                                          int BS) {
  const int cap = stage_floats / (GAMMA_RR_CH + 1);
  const int cover = GAMMA_RR_NL * (BS / 8);
  return cap < cover ? cap : cover;
}

/* All threads of the block call it together (barriers inside), after
 * sel.finish(). BS = blockDim.x, a multiple of 64; d % 4 == 0;
 * gamma_rr_round_rows(stage_floats, BS) >= 1; k2, k <= GAMMA_SORT_CAP. */
template <bool IP, int BS>
__device__ __forceinline__ void gamma_rerank_topk_epilogue(
    const uint64_t *res, int k2, uint64_t *sortbuf, float *stage,
    int stage_floats, float *qs, const float *__restrict__ qraw, int d,
    const float *const *__restrict__ segs, int seg_shift, int k,
    float *__restrict__ out_dists, int64_t *__restrict__ out_ids) {
  constexpr int CH = GAMMA_RR_CH, LD = CH + 1, NL = GAMMA_RR_NL;
  constexpr int RPP = BS / 8; /* rows one load per thread covers */
  const int tid = threadIdx.x;
  const int f4 = tid & 7, rg = tid >> 3;
  const int R = gamma_rr_round_rows(stage_floats, BS);
  const int nsl = (d + CH - 1) / CH;
  const int nsteps = ((k2 + R - 1) / R) * nsl;
  const int64_t seg_mask = ((int64_t)1 << seg_shift) - 1;

  for (int i = tid; i < d; i += BS) qs[i] = qraw[i];

  struct Slice { float4 v[NL]; };
  const float *rowp[NL];
  auto fetch = [&](Slice &x, int step) {
    const int rd = step / nsl, sl = step - rd * nsl;
    if (sl == 0) { /* a new round (uniform): its rows' addresses */
#pragma unroll
      for (int j = 0; j < NL; j++) {
        const int row = j * RPP + rg, cand = rd * R + row;
        uint64_t key = GAMMA_KEY_EMPTY;
        if (step < nsteps && row < R && cand < k2) key = res[cand];
        rowp[j] = qraw;
        if (key != GAMMA_KEY_EMPTY) {
          const uint32_t id = (uint32_t)(key & 0xffffffffu);
          rowp[j] = segs[id >> seg_shift] + (size_t)(id & seg_mask) * d;
        }
      }
    }
    int off = sl * CH + f4 * 4;
    if (off >= d) off = 0; /* the last slice of a d % 32 != 0 row */
#pragma unroll
    for (int j = 0; j < NL; j++) x.v[j] = *(const float4 *)(rowp[j] + off);
  };
  auto put = [&](const Slice &x) {
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const int row = j * RPP + rg;
      if (row < R) { /* the staging holds R rows */
        float *p = stage + row * LD + f4 * 4;
        p[0] = x.v[j].x;
        p[1] = x.v[j].y;
        p[2] = x.v[j].z;
        p[3] = x.v[j].w;
      }
    }
  };
  /* thread t < R owns candidate rd*R + t of round rd */
  float acc = 0.0f;
  auto compute = [&](int step) {
    const int rd = step / nsl, sl = step - rd * nsl;
    const int cand = rd * R + tid;
    const bool mine = tid < R && cand < k2;
    const uint64_t key = mine ? res[cand] : GAMMA_KEY_EMPTY;
    if (sl == 0) acc = 0.0f;
    if (key != GAMMA_KEY_EMPTY) {
      const float *qm = qs + sl * CH;
      const float *vm = stage + tid * LD;
      const int cnt = min(CH, d - sl * CH);
      if (cnt == CH) {
#pragma unroll 8
        for (int t = 0; t < CH; t++) {
          if (IP) {
            acc = fmaf(qm[t], vm[t], acc);
          } else {
            float dx = qm[t] - vm[t];
            acc = fmaf(dx, dx, acc);
          }
        }
      } else {
        for (int t = 0; t < cnt; t++) {
          if (IP) {
            acc = fmaf(qm[t], vm[t], acc);
          } else {
            float dx = qm[t] - vm[t];
            acc = fmaf(dx, dx, acc);
          }
        }
      }
    }
    if (sl == nsl - 1 && mine)
      sortbuf[cand] = key == GAMMA_KEY_EMPTY
                          ? GAMMA_KEY_EMPTY
                          : gamma_make_key<IP>(
                                acc, (uint32_t)(key & 0xffffffffu));
  };
  /* per step: stage, barrier (also the one qs needs), compute, barrier
   * (the staging is rewritten by the next step) */
  Slice a, b;
  fetch(a, 0);
  for (int s = 0; s < nsteps; s += 2) {
    fetch(b, s + 1);
    put(a);
    __syncthreads();
    compute(s);
    __syncthreads();
    if (s + 1 >= nsteps) break;
    fetch(a, s + 2);
    put(b);
    __syncthreads();
    compute(s + 1);
    __syncthreads();
  }

  int n = 1;
  while (n < k2 || n < k) n <<= 1;
  for (int i = k2 + tid; i < n; i += BS) sortbuf[i] = GAMMA_KEY_EMPTY;
  gamma_bitonic_sort(sortbuf, n);
  for (int i = tid; i < k; i += BS) {
    const uint64_t key = sortbuf[i];
    out_dists[i] =
        (key == GAMMA_KEY_EMPTY) ? -1.0f : gamma_key_dist<IP>(key);
    out_ids[i] = gamma_key_id(key);
  }
}
