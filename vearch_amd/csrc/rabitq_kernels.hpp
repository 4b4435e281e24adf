/*
 * rabitq_kernels.hpp — kernels of the IVFRABITQ index (RaBitQ codes of
 * nb_bits B = 1, 4 or 8, gamma_index_ivfrabitq.cc). Included at the end of
 * kernels.hip after binary_kernels.hpp: it uses that file's gamma_bin_load,
 * kernels.hip's WG, the GAMMA_SCAN_BS launch knob and gamma_pick
 * (ivfpq_scan_kernels.hpp) and scan_walk.hpp.
 *
 * B = 1. An entry of a d-dimensional table is EW = d/32 + 2 little-endian
 * words: W = d/32 sign words (bit j of the vector is bit j&31 of word j>>5,
 * the BINARYIVF layout), then the factors A and Mul as fp32. With c the
 * centroid of the entry's list and r = fl32(x - c):
 *   bit_j = r_j > 0,  n2 = sum r_j^2,  l1 = sum |r_j|,  xx = sum x_j^2
 *   A   = n2 (L2)  |  n2 - xx (inner product)
 *   Mul = inv_dp * sqrt(n2),  inv_dp = 1 / (l1 / sqrt(n2) / sqrt(d))
 * and one device-only float per entry, sval = sum_j bit_j * c_j (bucket
 * svals). The estimate for a query q against an entry of list l:
 *   dot = sum_j bit_j q_j - sval           (= sum_j bit_j (q - c_l)_j)
 *   fd  = (2 dot - sum_j (q - c_l)_j) / sqrt(d)
 *   pre = A + ||q - c_l||^2 - 2 Mul fd
 *   score = pre (L2)  |  -0.5 (pre - ||q||^2) (inner product)
 * sum_j bit_j q_j depends on the query alone and comes from a per-query
 * nibble table in LDS; ||q - c_l||^2 and sum (q - c_l) are one scalar each
 * per (query, probe).
 *
 * B = 4 or 8. The code (L = 2^(B-1), c the centroid of the vector's list,
 * d % 32 == 0):
 *   r = fl32(x - c), a_j = |r_j|, rmax = max_j a_j
 *   32 candidate scales s_i = fl32(g_i / rmax), g_i = L (i + 1) / 8
 *   m_j = min(L - 1, (int)floor(fl32(a_j s_i))),  v_j = m_j + 0.5
 *   the chosen i maximises num_i^2 / den_i, num_i = sum_j v_j a_j (fp32),
 *   den_i = sum_j (2 m_j + 1)^2 (exact integer); ties to the lowest i;
 *   rmax == 0: every m_j = 0
 *   u_j = L + m_j if r_j > 0, else L - 1 - m_j   (top bit = the 1-bit code)
 * B = 4: u_j is nibble j & 7 of little-endian word j >> 3; B = 8: byte j & 3
 * of word j >> 2. An entry is W = d B / 32 code words, then the factors as
 * fp32: A = n2 (L2) | n2 - xx (inner product), Mul = n2 / sum_j w_j r_j
 * with w_j = u_j - (2^B - 1)/2 (1 where |sum| < FLT_EPSILON). W is even, so
 * an entry is whole 8-byte units. One device-only float per entry,
 * sval = sum_j u_j c_j. The estimate, with cB = (2^B - 1)/2:
 *   dot = sum_j u_j q_j - sval
 *   pre = A + ||q - c||^2 - 2 Mul (dot - cB sum_j (q - c)_j)
 *   score = pre (L2)  |  -0.5 (pre - ||q||^2) (inner product)
 *
 * Who serves which (nb_bits, d), as gk::rabitq_scan dispatches, always at
 * BS = GAMMA_SCAN_BS: k_rabitq_scan<IP, B, U, NU, BS> with the entry moved
 * in units of U words. NU > 0 holds the whole entry in registers, NU = 0
 * streams it, NU = -1 tiles it through LDS (B = 4, 8 only).
 * - B = 1: d = 32, 64, 128, 256 (W = 1, 2, 4, 8) -> (U, NU) = (1, 3),
 *   (4, 1), (2, 3), (2, 5); every other d streamed, U = 2 where d/32 is
 *   even, else U = 1.
 * - B = 4: d = 64, 128, 256 -> (2, 5), (2, 9), (2, 17); else (2, -1).
 * - B = 8: d = 32, 64, 128 -> (2, 5), (2, 9), (2, 17); else (2, -1).
 * - GAMMA_RBQ_TILED, read at every launch, moves the multi-bit shapes:
 *   1 sends all of them to (2, -1), 0 sends the tiled ones back to the
 *   streamed (2, 0). B = 1 ignores it. gk::rabitq_scan_is_tiled tells.
 * gk::rabitq_encode: k_rabitq_encode at B = 1, else k_rabitq_encode_ex<B,
 * TR> with TR = 2 (d <= 128), 8 (d <= 512) or 0. gk::rabitq_sval_buckets:
 * k_rabitq_sval_buckets<B>.
 */
#pragma once

#define GAMMA_RBQ_DMAX 4096

template <int B>
struct GammaRbq {
  static_assert(B == 1 || B == 4 || B == 8, "code widths of IVFRABITQ");
  static constexpr int L = 1 << (B - 1);
  static constexpr int DPW = 32 / B;            /* dimensions per word */
  static constexpr int SH = B == 1 ? 5 : B == 4 ? 3 : 2; /* log2(DPW) */
  static constexpr uint32_t MASK = (1u << B) - 1u;
  static constexpr float CB = (float)((1 << B) - 1) * 0.5f;
};

/* what every launcher of the family accepts */
static bool gamma_rbq_ok(int d, int nb_bits) {
  return (nb_bits == 1 || nb_bits == 4 || nb_bits == 8) && d >= 32 &&
         d <= GAMMA_RBQ_DMAX && d % 32 == 0;
}

/* fixed-order sum over the 64 lanes of a wave; every lane gets the total */
__device__ __forceinline__ float gamma_rbq_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* ------------------------------------------------------- encode, B = 1
 * One wave per vector. Lane l owns dimensions l, l + 64, ...: it keeps its
 * partial sums in that order, the sign bits of a step are one ballot, and
 * the partials meet in a fixed xor tree — the same vector always yields
 * the same bytes. The residual is a single rounded subtraction (never
 * contracted into the squares), so the bits are those of fl32(x - c). */
__global__ void __launch_bounds__(WG)
k_rabitq_encode(int64_t n, int d, const float *__restrict__ x,
                const int32_t *__restrict__ asg, int asg_const, int nlist,
                const float *__restrict__ centroids, int ip,
                uint32_t *__restrict__ entries, float *__restrict__ svals) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  if (i >= n) return; /* wave-uniform */
  int a = asg ? asg[i] : asg_const;
  a = a < 0 ? 0 : (a >= nlist ? nlist - 1 : a);
  const float *xv = x + (size_t)i * d;
  const float *cv = centroids + (size_t)a * d;
  const int W = d >> 5;
  uint32_t *ent = entries + (size_t)i * (W + 2);
  float n2 = 0.0f, l1 = 0.0f, xx = 0.0f, sv = 0.0f;
  for (int t = 0; t * 64 < d; t++) {
    const int j = t * 64 + lane;
    const bool act = j < d;
    const float xj = act ? xv[j] : 0.0f;
    const float cj = act ? cv[j] : 0.0f;
    const float r = __fsub_rn(xj, cj);
    const bool bit = act && r > 0.0f;
    const unsigned long long m = __ballot(bit);
    n2 = fmaf(r, r, n2);
    l1 += fabsf(r);
    xx = fmaf(xj, xj, xx);
    sv += bit ? cj : 0.0f;
    if (lane == 0) {
      ent[2 * t] = (uint32_t)m;
      if (2 * t + 1 < W) ent[2 * t + 1] = (uint32_t)(m >> 32);
    }
  }
  n2 = gamma_rbq_wave_sum(n2);
  l1 = gamma_rbq_wave_sum(l1);
  xx = gamma_rbq_wave_sum(xx);
  sv = gamma_rbq_wave_sum(sv);
  if (lane == 0) {
    const float eps = 1.1920928955078125e-7f; /* FLT_EPSILON */
    const float inv_norm = n2 < eps ? 1.0f : 1.0f / sqrtf(n2);
    const float ndp = l1 * inv_norm / sqrtf((float)d);
    const float inv_dp = fabsf(ndp) < eps ? 1.0f : 1.0f / ndp;
    ent[W] = __float_as_uint(ip ? n2 - xx : n2);
    ent[W + 1] = __float_as_uint(inv_dp * sqrtf(n2));
    svals[i] = sv;
  }
}

/* The multi-bit encode and the sval kernels are built without packed fp32
 * instructions, so every sum stays a chain of single fused operations;
 * their lambdas are always_inline because the inliner refuses a callee
 * whose target features differ. The scan calls the shared selector, which
 * is not always_inline, so it keeps the default features and issues its
 * FMAs itself (gamma_rbq_ex_fma). */
#if defined(__HIP_DEVICE_COMPILE__)
#define GAMMA_RBQ_EX_KERNEL \
  __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define GAMMA_RBQ_EX_KERNEL __global__
#endif
#define GAMMA_RBQ_EX_INLINE __attribute__((always_inline))

/* -------------------------------------------------- encode, B = 4 or 8
 * One wave per vector, lane l owns dimensions l, l + 64, ... (step t holds
 * dimension 64 t + l). TR > 0: the residuals of the TR steps stay in
 * registers (d <= 64 TR). TR == 0: any d; a pass over the vector reloads x
 * and c (cache-resident after the first pass) and redoes the one rounded
 * subtraction, so nothing spills. Per candidate the lane partials — num in
 * fp32, den as an integer — meet in the fixed xor tree of
 * gamma_rbq_wave_sum; every lane sees the same totals and picks the same
 * winner. The winner's codes are rebuilt, the 8 (B = 4) or 4 (B = 8) lanes
 * of a word OR their fields together by xor shuffles, and the first lane of
 * the group stores the word. Every operation of the candidate construction
 * is a single correctly rounded fp32 operation. */
template <int B, int TR>
GAMMA_RBQ_EX_KERNEL void __launch_bounds__(WG)
k_rabitq_encode_ex(int64_t n, int d, const float *__restrict__ x,
                   const int32_t *__restrict__ asg, int asg_const, int nlist,
                   const float *__restrict__ centroids, int ip,
                   uint32_t *__restrict__ entries,
                   float *__restrict__ svals) {
  typedef GammaRbq<B> P;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  if (i >= n) return; /* wave-uniform */
  int a = asg ? asg[i] : asg_const;
  a = a < 0 ? 0 : (a >= nlist ? nlist - 1 : a);
  const float *xv = x + (size_t)i * d;
  const float *cv = centroids + (size_t)a * d;
  const int W = d / P::DPW;
  uint32_t *ent = entries + (size_t)i * (W + 2);
  const int T = (d + 63) >> 6;

  float rr[TR ? TR : 1];
  /* r of step t; 0 past d */
  auto resid = [&](int t) GAMMA_RBQ_EX_INLINE -> float {
    if constexpr (TR > 0) {
      return rr[t];
    } else {
      const int j = t * 64 + lane;
      return j < d ? __fsub_rn(xv[j], cv[j]) : 0.0f;
    }
  };

  float n2 = 0.0f, xx = 0.0f, rmax = 0.0f;
#pragma unroll TR ? TR : 1
  for (int t = 0; t < (TR ? TR : T); t++) {
    const int j = t * 64 + lane;
    const bool act = j < d;
    const float xj = act ? xv[j] : 0.0f;
    const float r = act ? __fsub_rn(xj, cv[j]) : 0.0f;
    if constexpr (TR > 0) rr[t] = r;
    n2 = fmaf(r, r, n2);
    xx = fmaf(xj, xj, xx);
    rmax = fmaxf(rmax, fabsf(r));
  }
  n2 = gamma_rbq_wave_sum(n2);
  xx = gamma_rbq_wave_sum(xx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));

  auto magnitude = [&](float av, float s) GAMMA_RBQ_EX_INLINE -> int {
    const int m = (int)floorf(__fmul_rn(av, s));
    return m < P::L - 1 ? m : P::L - 1;
  };
  auto scale_of = [&](int c) GAMMA_RBQ_EX_INLINE -> float {
    const float g = (float)(P::L * (c + 1)) * 0.125f; /* exact */
    return rmax > 0.0f ? __fdiv_rn(g, rmax) : 0.0f;   /* 0: every m = 0 */
  };

  int best = 0;
  float bnum = 0.0f;
  unsigned long long bden = 1;
  for (int c = 0; c < 32; c++) {
    const float s = scale_of(c);
    float num = 0.0f;
    unsigned int den = 0; /* lane: <= 64 x 255^2; wave: <= 4096 x 255^2 */
#pragma unroll TR ? TR : 1
    for (int t = 0; t < (TR ? TR : T); t++) {
      if (t * 64 + lane < d) {
        const float av = fabsf(resid(t));
        const int m = magnitude(av, s);
        num = fmaf((float)m + 0.5f, av, num);
        den += (unsigned)((2 * m + 1) * (2 * m + 1));
      }
    }
    num = gamma_rbq_wave_sum(num);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) den += __shfl_xor(den, o, 64);
    /* num^2 / den > bnum^2 / bden, cross-multiplied in fp64: the squares
     * are exact and the products round at 2^-53 */
    const double lhs = (double)num * (double)num * (double)bden;
    const double rhs = (double)bnum * (double)bnum * (double)den;
    if (c == 0 || lhs > rhs) {
      best = c;
      bnum = num;
      bden = den;
    }
  }

  const float s = scale_of(best);
  float wr = 0.0f, sv = 0.0f;
#pragma unroll TR ? TR : 1
  for (int t = 0; t < (TR ? TR : T); t++) {
    const int j = t * 64 + lane;
    const bool act = j < d;
    uint32_t u = 0;
    if (act) {
      const float r = resid(t);
      const int m = magnitude(fabsf(r), s);
      u = (uint32_t)(r > 0.0f ? P::L + m : P::L - 1 - m);
      wr = fmaf((float)u - P::CB, r, wr);
      sv = fmaf((float)u, cv[j], sv);
    }
    uint32_t w = u << (B * (lane & (P::DPW - 1)));
#pragma unroll
    for (int o = 1; o < P::DPW; o <<= 1) w |= __shfl_xor(w, o, 64);
    if (act && (lane & (P::DPW - 1)) == 0) ent[j >> P::SH] = w;
  }
  wr = gamma_rbq_wave_sum(wr);
  sv = gamma_rbq_wave_sum(sv);
  if (lane == 0) {
    const float eps = 1.1920928955078125e-7f; /* FLT_EPSILON */
    ent[W] = __float_as_uint(ip ? n2 - xx : n2);
    ent[W + 1] = __float_as_uint(fabsf(wr) < eps ? 1.0f : n2 / wr);
    svals[i] = sv;
  }
}

hipError_t gk::rabitq_encode(hipStream_t s, int nb_bits, int64_t n, int d,
                             const float *x, const int32_t *asg,
                             int asg_const, int nlist,
                             const float *centroids, bool ip,
                             uint8_t *entries, float *svals) {
  if (n <= 0) return hipSuccess;
  if (!gamma_rbq_ok(d, nb_bits) || nlist <= 0) return hipErrorInvalidValue;
  const int64_t g = (n + WG / 64 - 1) / (WG / 64);
  if (g > 0x7fffffffll) return hipErrorInvalidValue;
  auto launch = [&](auto kernel) {
    kernel<<<dim3((uint32_t)g), dim3(WG), 0, s>>>(
        n, d, x, asg, asg_const, nlist, centroids, ip ? 1 : 0,
        (uint32_t *)entries, svals);
  };
  if (nb_bits == 1) {
    launch(k_rabitq_encode);
  } else {
    gamma_pick<4, 8>(nb_bits, [&](auto b) {
      gamma_pick<2, 8, 0>(d <= 128 ? 2 : d <= 512 ? 8 : 0, [&](auto tr) {
        launch(k_rabitq_encode_ex<decltype(b)::value, decltype(tr)::value>);
      });
    });
  }
  return hipGetLastError();
}

/* Load path: sval of every stored entry from its code words and its list's
 * centroid, block per bucket, wave per entry. Lane l of step t takes
 * dimension t*64 + l: at B = 1 it adds c[dim] where the bit is set, else
 * fmaf((float)u, c[dim], sv) — the operands, the order and the tree of the
 * width's encode kernel, so the rebuilt svals equal the encoded ones bit
 * for bit. */
template <int B>
GAMMA_RBQ_EX_KERNEL void __launch_bounds__(WG)
k_rabitq_sval_buckets(int d, const GammaBucketDev *__restrict__ bks,
                      const float *__restrict__ centroids) {
  typedef GammaRbq<B> P;
  const GammaBucketDev bk = bks[blockIdx.x];
  if (!bk.svals || bk.size <= 0) return;
  const int lane = threadIdx.x & 63;
  const int W = d / P::DPW;
  const float *cv = centroids + (size_t)blockIdx.x * d;
  const uint32_t *data = (const uint32_t *)bk.data;
  float *out = (float *)bk.svals; /* writable: Load owns the buckets */
  for (long long j = threadIdx.x >> 6; j < bk.size; j += WG / 64) {
    const uint32_t *ent = data + (size_t)j * (W + 2);
    float sv = 0.0f;
    for (int t = 0; t * 64 < d; t++) {
      const int dim = t * 64 + lane;
      if constexpr (B == 1) {
        const bool act = dim < d;
        const uint32_t w = act ? ent[dim >> 5] : 0u;
        const bool bit = (w >> (lane & 31)) & 1u;
        const float cj = act ? cv[dim] : 0.0f;
        sv += bit ? cj : 0.0f;
      } else if (dim < d) {
        const uint32_t u =
            (ent[dim >> P::SH] >> (B * (dim & (P::DPW - 1)))) & P::MASK;
        sv = fmaf((float)u, cv[dim], sv);
      }
    }
    sv = gamma_rbq_wave_sum(sv);
    if (lane == 0) out[j] = sv;
  }
}

hipError_t gk::rabitq_sval_buckets(hipStream_t s, int nb_bits, int nlist,
                                   int d, const GammaBucketDev *bks,
                                   const float *centroids) {
  if (nlist <= 0) return hipSuccess;
  if (!gamma_rbq_ok(d, nb_bits)) return hipErrorInvalidValue;
  gamma_pick<1, 4, 8>(nb_bits, [&](auto b) {
    k_rabitq_sval_buckets<decltype(b)::value>
        <<<dim3((uint32_t)nlist), dim3(WG), 0, s>>>(d, bks, centroids);
  });
  return hipGetLastError();
}

/* ---------------------------------------------------- RaBitQ IVF fused scan
 * The contract of k_binivf_scan and of k_ivfpq_scan's fast path, and their
 * chunked probe walk (scan_walk.hpp): a workgroup serves (query,
 * probe-split sub-block). The widths differ in how sum_j u_j q_j is formed
 * and in the closing formula; everything else is one text.
 *
 * B = 1, query table: lut[i][n], i < d/4, n < 16 = sum of q[4i + b] over
 * the bits b set in n, ascending b. A row is 16 consecutive LDS banks, so
 * the 64 lanes of a gather hit at most 16 addresses in 16 different banks:
 * conflict-free for any code pattern, like the 4-bit ADC table and unlike
 * a 256-entry byte row. d/4 lookups per entry = 32 at d = 128, the count
 * of the 8-bit ADC scan at M = 32. Every word adds to s0 and s1
 * alternately.
 *
 * B = 4 or 8: there is no lookup table: a lane owns one entry, holds its
 * code words in VGPRs and accumulates fmaf((float)u_j, q_j, acc) over the
 * unpacked fields. B = 4: two masks per word (w & 0x0f0f0f0f, (w >> 4) &
 * 0x0f0f0f0f) put the even and the odd nibbles into byte lanes, then eight
 * byte-to-float conversions; B = 8: four conversions and no mask. q_j is
 * the same for all 64 lanes: the query row is read through the constant
 * address space with a uniform index, i.e. by scalar loads into SGPRs, and
 * enters the FMA as its scalar operand — LDS serves only the selector, the
 * chunk and the qs copy that gamma_rbq_qc reads. Summation order, fixed per
 * entry: j ascending inside a word; even words into s0, odd words into s1,
 * s0 + s1 at the end. BS, S and the entry movement do not enter.
 *
 * Per-(query, probe) scalars qc2 = ||q - c||^2 and sqc = sum (q - c) are
 * recomputed per chunk from the centroid itself, 8 lanes per probe: lane l
 * sums dimensions l, l + 8, ... in order and the 8 partials meet in a
 * fixed xor tree. Block size and probe split do not enter, so a score
 * does not depend on the launch shape.
 *
 * U = words per load unit (2 at B = 4 and 8, whose entries are whole 8-byte
 * units), NU > 0: the whole entry (code words, A, Mul) is NU units held in
 * registers and double-buffered. NU == 0: the entry is streamed in units of
 * U at consume time and only id and sval are prefetched.
 *
 * NU == -1 (B = 4, 8), the tiled movement, for entries too long for
 * registers. Streamed, a lane walks its own entry: every load of the wave
 * touches 64 cache lines and returns to each line once per unit. Tiled, the
 * WAVE moves its 64 entries together, in slabs of GAMMA_RBQ_TK 8-byte units
 * per entry, through a tile of its own in LDS (no workgroup barrier):
 * - pointers: each lane stores its entry pointer into the (still free)
 *   tile, and lane l reads back those of the entries l / TK + (64 / TK) i,
 *   i < TK, the ones it loads for;
 * - gather: load i of a slab takes unit l % TK of entry l / TK + (64 / TK) i
 *   — TK adjacent lanes cover TK adjacent units, 64 contiguous bytes, so a
 *   load touches 64 / TK spans instead of 64 lines. The TK loads of slab
 *   s + 1 are issued into registers before slab s is consumed: registers
 *   are the second buffer, the tile holds one slab;
 * - transpose: the units go to row = entry, column = unit of the tile, row
 *   pitch GAMMA_RBQ_TP = TK + 1 units. The pitch is odd, so the 32 lanes of
 *   a half-wave read the same column of 32 rows from 32 different bank
 *   pairs (ds_read_b64, conflict-free), and the writes of a load land on
 *   l + l / TK, 64 distinct consecutive pairs;
 * - consume: lane l reads row l and feeds gamma_rbq_ex_word as the other
 *   movements do, unit u = words 2u (s0) and 2u + 1 (s1). The last slab is
 *   partial: its lanes past the entry's end load nothing, and its last unit
 *   is (A, Mul).
 * Every lane of a wave with one entry to score runs the walk (the loads are
 * the wave's); only the push is per lane. LDS accesses of one wave execute
 * in order, so the wave needs no wait between its writes and its reads;
 * wave_barrier pins the compiler's order. */
#define GAMMA_RBQ_TK 8
#define GAMMA_RBQ_TP (GAMMA_RBQ_TK + 1)
static_assert(64 % GAMMA_RBQ_TK == 0 && GAMMA_RBQ_TP % 2 == 1,
              "whole slabs per load, odd row pitch");

struct GammaRbqPer {
  float qc2[GAMMA_SCAN_PCH];
  float sqc[GAMMA_SCAN_PCH];
};
struct GammaRbqChunk : GammaChunkT<GammaRbqPer> {
  float qq; /* ||q||^2 */
};

template <int U, int NU>
struct GammaRbqElem {
  uint32_t w[NU > 0 ? U * NU : 1];
  gamma_gu32p cw; /* NU <= 0: the entry's words */
  uint32_t id;
  float sv, qc2, sqc;
  bool live;
};

/* dynamic LDS of k_rabitq_scan: `tab` bytes of query table (16 d at B = 1,
 * none otherwise), selector scratch + result, query, chunk, and for the
 * tiled movement one 64-row tile per wave of the block */
__host__ __device__ static size_t gamma_rbq_tab_bytes(int nb_bits, int d) {
  return nb_bits == 1 ? (size_t)d * 16 : 0;
}
/* deep (GammaDeepSelector): the append buffer and the radix scratch take
 * the place of the scratch + k2 result keys */
__host__ __device__ static size_t gamma_rbq_qs_off(size_t tab, int k2,
                                                   bool deep = false) {
  return tab + (deep ? (size_t)GAMMA_SORT_CAP * 8 + sizeof(GammaRadixLds)
                     : ((size_t)GAMMA_SORT_CAP + k2) * 8);
}
__host__ __device__ static size_t gamma_rbq_chunk_off(size_t tab, int d,
                                                      int k2,
                                                      bool deep = false) {
  return (gamma_rbq_qs_off(tab, k2, deep) + (size_t)d * 4 + 7) / 8 * 8;
}
static_assert(sizeof(GammaRbqChunk) % 8 == 0, "the tile holds 8-byte units");
__host__ __device__ static size_t gamma_rbq_tile_off(size_t tab, int d,
                                                     int k2,
                                                     bool deep = false) {
  return gamma_rbq_chunk_off(tab, d, k2, deep) + sizeof(GammaRbqChunk);
}
/* tile_bs: the block size of a tiled launch, 0 for the other movements */
static size_t gamma_rbq_smem(int nb_bits, int d, int k2, bool deep = false,
                             int tile_bs = 0) {
  return gamma_rbq_tile_off(gamma_rbq_tab_bytes(nb_bits, d), d, k2, deep) +
         (size_t)tile_bs * GAMMA_RBQ_TP * 8;
}

/* B = 1: 8 nibble lookups of one sign word; tab advances by 8 rows */
__device__ __forceinline__ void gamma_rbq_word(uint32_t w, const float *&tab,
                                               float &s0, float &s1) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    s0 += tab[(i * 16) + ((w >> (4 * i)) & 15u)];
    s1 += tab[(i * 16 + 16) + ((w >> (4 * i + 4)) & 15u)];
  }
  tab += 128;
}

typedef const __attribute__((address_space(4))) float *gamma_cf32p;

/* B = 4, 8: acc += u * q as ONE v_fmac_f32 with q, wave-uniform, as its
 * scalar operand. Written out so that the two accumulator chains stay
 * chains of single fused operations in ascending j: left to the vectorizer
 * they are paired into packed FMAs. */
__device__ __forceinline__ void gamma_rbq_ex_fma(float u, float q,
                                                 float &acc) {
  asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "s"(q), "v"(u));
}

/* one code word against its 32 / B query coordinates at q, j ascending */
template <int B>
__device__ __forceinline__ void gamma_rbq_ex_word(uint32_t w, gamma_cf32p q,
                                                  float &acc) {
  if constexpr (B == 4) {
    uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
    /* opaque, so that the fields are taken by the four byte-to-float
     * conversions and not each by a bit-field extract of w first */
    asm("" : "+v"(lo), "+v"(hi));
    gamma_rbq_ex_fma((float)(lo & 0xffu), q[0], acc);
    gamma_rbq_ex_fma((float)(hi & 0xffu), q[1], acc);
    gamma_rbq_ex_fma((float)((lo >> 8) & 0xffu), q[2], acc);
    gamma_rbq_ex_fma((float)((hi >> 8) & 0xffu), q[3], acc);
    gamma_rbq_ex_fma((float)((lo >> 16) & 0xffu), q[4], acc);
    gamma_rbq_ex_fma((float)((hi >> 16) & 0xffu), q[5], acc);
    gamma_rbq_ex_fma((float)(lo >> 24), q[6], acc);
    gamma_rbq_ex_fma((float)(hi >> 24), q[7], acc);
  } else {
    gamma_rbq_ex_fma((float)(w & 0xffu), q[0], acc);
    gamma_rbq_ex_fma((float)((w >> 8) & 0xffu), q[1], acc);
    gamma_rbq_ex_fma((float)((w >> 16) & 0xffu), q[2], acc);
    gamma_rbq_ex_fma((float)(w >> 24), q[3], acc);
  }
}

/* 8 lanes per value: lane l of the group sums dims l, l+8, ...; returns
 * (sum (q-c)^2, sum (q-c)) on every lane of the group. c == nullptr: c = 0;
 * l < 0: the lane adds nothing. All 64 lanes of the wave must call it. */
__device__ __forceinline__ void gamma_rbq_qc(const float *qs,
                                             const float *__restrict__ c,
                                             int d, int l, float &s2,
                                             float &s1) {
  float a = 0.0f, b = 0.0f;
  if (l >= 0) {
    for (int j = l; j < d; j += 8) {
      const float df = __fsub_rn(qs[j], c ? c[j] : 0.0f);
      a = fmaf(df, df, a);
      b += df;
    }
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  s2 = a;
  s1 = b;
}

/* SEL = GammaSelector: out_keys is nq x S x k2. SEL = GammaDeepSelector:
 * out_keys is the selectors' regions, GAMMA_DEEP_REGION(k2) keys per (query,
 * sub-block); the workgroup's k2 keys end up in the first k2 slots of its
 * own. Everything between init and finish is one text. */
template <bool IP, int B, int U, int NU, int BS, class SEL = GammaSelector>
__global__ void __launch_bounds__(BS)
k_rabitq_scan(int nq, int S, int d, int nprobe, int k2,
              const float *__restrict__ queries,
              const float *__restrict__ centroids,
              const GammaBucketDev *__restrict__ buckets, int nlist,
              const int64_t *__restrict__ probes,
              const uint32_t *__restrict__ bitmap,
              uint64_t *__restrict__ out_keys,
              const int *__restrict__ kill_flag) {
  typedef GammaRbq<B> P;
  static_assert(B == 1 || U == 2, "multi-bit entries move in 8-byte units");
  static_assert(NU >= -1 && (NU >= 0 || B > 1), "tiled: multi-bit only");
  constexpr bool TILED = NU < 0;
  extern __shared__ char smem[];
  const size_t tab = gamma_rbq_tab_bytes(B, d);
  [[maybe_unused]] float *lut = (float *)smem; /* B == 1: d/4 x 16 */
  uint64_t *sortbuf = (uint64_t *)(smem + tab);
  constexpr bool DEEP = std::is_same<SEL, GammaDeepSelector>::value;
  float *qs = (float *)(smem + gamma_rbq_qs_off(tab, k2, DEEP)); /* d */
  GammaRbqChunk *ch =
      (GammaRbqChunk *)(smem + gamma_rbq_chunk_off(tab, d, k2, DEEP));

  const int q = blockIdx.x / S;
  const int sub = blockIdx.x - q * S;
  if (q >= nq) return;
  const float *qg = queries + (int64_t)q * d;
  /* B > 1: the query for the FMAs; read-only for the launch */
  [[maybe_unused]] const gamma_cf32p qc = (gamma_cf32p)qg;
  for (int i = threadIdx.x; i < d; i += BS) qs[i] = qg[i];

  SEL sel; /* init has the barrier qs needs */
  if constexpr (DEEP)
    sel.init(sortbuf, (GammaRadixLds *)(sortbuf + GAMMA_SORT_CAP), ch->state,
             out_keys + (size_t)blockIdx.x * GAMMA_DEEP_REGION(k2), k2);
  else
    sel.init(sortbuf, sortbuf + GAMMA_SORT_CAP, ch->state, k2);

  if constexpr (B == 1) {
    for (int e = threadIdx.x; e < d * 4; e += BS) {
      const float *q4 = qs + (e >> 4) * 4;
      float t = 0.0f;
      if (e & 1) t += q4[0];
      if (e & 2) t += q4[1];
      if (e & 4) t += q4[2];
      if (e & 8) t += q4[3];
      lut[e] = t;
    }
  }
  const unsigned tid = threadIdx.x;
  if (tid < 64) { /* wave 0: ||q||^2 by the scheme of the probe scalars */
    float s2, s1;
    gamma_rbq_qc(qs, nullptr, d, tid < 8 ? (int)tid : -1, s2, s1);
    if (tid == 0) ch->qq = s2;
  }
  __syncthreads();
  const float qq = ch->qq;
  [[maybe_unused]] const float inv_sqrt_d = 1.0f / sqrtf((float)d);

  constexpr int NW = NU > 0 ? U * NU : 1; /* NU > 0: words per entry */
  const int W = NU > 0 ? NW - 2 : d / P::DPW;
  const int EW = W + 2;
  /* tiled: this wave's tile, 64 rows of GAMMA_RBQ_TP units */
  [[maybe_unused]] uint64_t *tile =
      (uint64_t *)(smem + gamma_rbq_tile_off(tab, d, k2, DEEP)) +
      (threadIdx.x >> 6) * (64 * GAMMA_RBQ_TP);

  const int np_sub = sub < nprobe ? (nprobe - sub + S - 1) / S : 0;
  const int *kf = kill_flag ? kill_flag : (const int *)probes;
  bool killed = false;
  for (int c0 = 0; c0 < np_sub && !killed;) {
    const int cn = min(GAMMA_SCAN_PCH, np_sub - c0);
    if (tid < GAMMA_SCAN_PCH * 8) { /* whole waves: 8 lanes per probe */
      const int pi = (int)(tid >> 3);
      const int l = (int)(tid & 7u);
      int64_t ln = -1;
      if (pi < cn) ln = probes[(int64_t)q * nprobe + sub + (c0 + pi) * S];
      const bool ok = ln >= 0 && ln < nlist;
      float s2, s1;
      gamma_rbq_qc(qs, ok ? centroids + (size_t)ln * d : nullptr, d,
                   ok ? l : -1, s2, s1);
      if (pi < cn && l == 0) {
        GammaBucketDev bk = gamma_null_bucket();
        if (ok) bk = buckets[ln];
        gamma_chunk_put(ch, pi, bk);
        ch->per.qc2[pi] = s2;
        ch->per.sqc[pi] = s1;
      }
    }
    const GammaChunkSpan sp = gamma_chunk_close(ch, cn, kill_flag);
    c0 += sp.ncons;

    GammaListCursor cur;
    cur.reset(ch, sp.total);
    gamma_gu32p pid = ch->ids[0];
    gamma_gu32p pcodes = (gamma_gu32p)ch->codes[0];
    gamma_gf32p psv = ch->svals[0];
    float lqc2 = ch->per.qc2[0], lsqc = ch->per.sqc[0];

    auto fetch = [&](GammaRbqElem<U, NU> &e, unsigned it) {
      const unsigned j = cur.seek(ch, it * BS + tid, e.live, [&](int li) {
        pid = ch->ids[li];
        pcodes = (gamma_gu32p)ch->codes[li];
        psv = ch->svals[li];
        lqc2 = ch->per.qc2[li];
        lsqc = ch->per.sqc[li];
      });
      e.id = pid[j];
      e.sv = psv[j];
      e.qc2 = lqc2;
      e.sqc = lsqc;
      e.cw = pcodes + (size_t)j * EW;
      if constexpr (NU > 0) {
#pragma unroll
        for (int u = 0; u < NU; u++) {
          uint32_t t[U];
          gamma_bin_load<U>(e.cw + u * U, t);
#pragma unroll
          for (int i = 0; i < U; i++) e.w[u * U + i] = t[i];
        }
      }
    };
    auto retire = [&](const GammaRbqElem<U, NU> &e) {
      if constexpr (NU > 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) asm volatile("" ::"v"(e.w[i]));
      }
      asm volatile("" ::"v"(e.id));
      asm volatile("" ::"v"(e.sv));
    };
    auto consume = [&](const GammaRbqElem<U, NU> &e) {
      retire(e);
      if (e.live && !(e.id >> 31) &&
          !gamma_bitmap_test(bitmap, (uint64_t)e.id)) {
        float s0 = 0.0f, s1 = 0.0f, fa, fm;
        /* sum_j u_j q_j in the width's own order */
        if constexpr (B == 1) {
          const float *tab = lut;
          if constexpr (NU > 0) {
#pragma unroll
            for (int i = 0; i < NW - 2; i++)
              gamma_rbq_word(e.w[i], tab, s0, s1);
          } else {
            for (int u = 0; u < W / U; u++) {
              uint32_t t[U];
              gamma_bin_load<U>(e.cw + u * U, t);
#pragma unroll
              for (int i = 0; i < U; i++) gamma_rbq_word(t[i], tab, s0, s1);
            }
          }
        } else if constexpr (NU > 0) {
#pragma unroll
          for (int u = 0; u < NU - 1; u++) {
            gamma_rbq_ex_word<B>(e.w[2 * u], qc + 2 * u * P::DPW, s0);
            gamma_rbq_ex_word<B>(e.w[2 * u + 1], qc + (2 * u + 1) * P::DPW,
                                 s1);
          }
        } else {
          gamma_cf32p qp = qc;
          for (int u = 0; u < W; u += 2, qp += 2 * P::DPW) {
            uint32_t t[2];
            gamma_bin_load<2>(e.cw + u, t);
            gamma_rbq_ex_word<B>(t[0], qp, s0);
            gamma_rbq_ex_word<B>(t[1], qp + P::DPW, s1);
          }
        }
        /* the factors A and Mul behind the code words */
        if constexpr (NU > 0) {
          fa = __uint_as_float(e.w[NW - 2]);
          fm = __uint_as_float(e.w[NW - 1]);
        } else {
          uint32_t f[2];
          if constexpr (U == 2) {
            gamma_bin_load<2>(e.cw + W, f);
          } else {
            f[0] = e.cw[W];
            f[1] = e.cw[W + 1];
          }
          fa = __uint_as_float(f[0]);
          fm = __uint_as_float(f[1]);
        }
        const float dot = (s0 + s1) - e.sv;
        float pre;
        if constexpr (B == 1) {
          const float fd = (2.0f * dot - e.sqc) * inv_sqrt_d;
          pre = fa + e.qc2 - 2.0f * fm * fd;
        } else {
          const float t = fmaf(-P::CB, e.sqc, dot);
          pre = fmaf(-2.0f * fm, t, fa + e.qc2);
        }
        const float score = IP ? -0.5f * (pre - qq) : pre;
        sel.push(gamma_make_key<IP>(score, e.id));
      }
    };
    /* the tiled movement (head comment): the wave's 64 entries, slab by
     * slab, global -> registers -> tile -> the owning lane */
    auto consume_tiled = [&](const GammaRbqElem<U, NU> &e) {
      constexpr int K = GAMMA_RBQ_TK, TP = GAMMA_RBQ_TP, EPL = 64 / K;
      typedef const __attribute__((address_space(1))) gamma_u32x2 *unit_p;
      retire(e);
      const bool ok = e.live && !(e.id >> 31) &&
                      !gamma_bitmap_test(bitmap, (uint64_t)e.id);
      if (!__ballot(ok)) return; /* wave-uniform: nothing to score */
      const int lane = (int)(tid & 63u), k = lane % K, g = lane / K;
      const int nun = W / 2 + 1; /* units of an entry, (A, Mul) last */
      const int ns = (nun + K - 1) / K, rem = nun - (ns - 1) * K;
      tile[lane] = (uint64_t)e.cw;
      __builtin_amdgcn_wave_barrier();
      unit_p p[K]; /* unit k of the entries this lane loads for */
#pragma unroll
      for (int i = 0; i < K; i++)
        p[i] = (unit_p)(gamma_gu32p)tile[i * EPL + g] + k;
      __builtin_amdgcn_wave_barrier();
      uint64_t *wr = tile + g * TP + k;
      const uint64_t *rd = tile + lane * TP;
      gamma_u32x2 r[K];
#pragma unroll
      for (int i = 0; i < K; i++) r[i] = gamma_u32x2{0u, 0u};
      /* nothing is read past an entry: the last slab has rem units */
      auto load = [&](int s) {
        if (s < ns - 1 || k < rem) {
#pragma unroll
          for (int i = 0; i < K; i++) r[i] = p[i][s * K];
        }
      };
      auto store = [&]() {
#pragma unroll
        for (int i = 0; i < K; i++)
          wr[i * EPL * TP] = (uint64_t)r[i].x | ((uint64_t)r[i].y << 32);
        __builtin_amdgcn_wave_barrier();
      };
      auto unit = [&](int u, gamma_cf32p qp, float &s0, float &s1) {
        const uint64_t v = rd[u];
        gamma_rbq_ex_word<B>((uint32_t)v, qp, s0);
        gamma_rbq_ex_word<B>((uint32_t)(v >> 32), qp + P::DPW, s1);
      };
      float s0 = 0.0f, s1 = 0.0f;
      gamma_cf32p qp = qc;
      load(0);
      for (int s = 0; s < ns - 1; s++, qp += 2 * K * P::DPW) {
        store();
        load(s + 1);
#pragma unroll
        for (int u = 0; u < K; u++) unit(u, qp + 2 * u * P::DPW, s0, s1);
        __builtin_amdgcn_wave_barrier();
      }
      store();
      for (int u = 0; u < rem - 1; u++, qp += 2 * P::DPW) unit(u, qp, s0, s1);
      const uint64_t f = rd[rem - 1];
      __builtin_amdgcn_wave_barrier();
      if (ok) { /* consume's closing at B > 1, operation for operation */
        const float fa = __uint_as_float((uint32_t)f);
        const float fm = __uint_as_float((uint32_t)(f >> 32));
        const float t = fmaf(-P::CB, e.sqc, (s0 + s1) - e.sv);
        const float pre = fmaf(-2.0f * fm, t, fa + e.qc2);
        const float score = IP ? -0.5f * (pre - qq) : pre;
        sel.push(gamma_make_key<IP>(score, e.id));
      }
    };

    /* flush check, kill poll and the two-set pass loop: the scheme of
     * k_ivfpq_scan's fast path (reasons there) */
    killed = sp.killed;
    const unsigned niter = (sp.total + BS - 1) / BS;
    /* deep: the whole scratch is append room */
    const bool flush_each = !DEEP && k2 + 2 * BS > GAMMA_SORT_CAP;
    const int fmargin = flush_each ? BS : 2 * BS;
    auto pass = [&](GammaRbqElem<U, NU> &nxt, const GammaRbqElem<U, NU> &cur_e,
                    unsigned it_nxt, int slot, bool check) {
      const int kv = __hip_atomic_load(kf, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
      fetch(nxt, it_nxt);
      if constexpr (TILED) consume_tiled(cur_e);
      else consume(cur_e);
      asm volatile("" ::"v"(kv));
      if (!check) return false;
      if (tid == 0) ch->kill[slot] = kill_flag ? kv : 0;
      sel.maybe_flush(fmargin);
      return ch->kill[slot] != 0;
    };
    if (niter > 0) {
      GammaRbqElem<U, NU> ea, eb;
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
    sel.maybe_flush(fmargin);
  }
  sel.finish();
  if constexpr (!DEEP) {
    for (int i = threadIdx.x; i < k2; i += BS)
      out_keys[((int64_t)q * S + sub) * k2 + i] = sel.res[i];
  }
}

/* GAMMA_RBQ_TILED: 1 tiles every multi-bit launch, 0 none (the streamed
 * movement, for A/B runs and tests); unset or anything else: -1, tiled
 * where the entry does not fit registers */
static int gamma_rbq_tiled_knob() {
  const char *e = getenv("GAMMA_RBQ_TILED");
  if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] - '0';
  return -1;
}
/* the multi-bit shapes with a register-resident instantiation */
static bool gamma_rbq_resident(int nb_bits, int d) {
  const int W = d * nb_bits / 32;
  return W == 8 || W == 16 || W == 32;
}
bool gk::rabitq_scan_is_tiled(int nb_bits, int d) {
  if (!gamma_rbq_ok(d, nb_bits) || nb_bits == 1) return false;
  const int knob = gamma_rbq_tiled_knob();
  return knob < 0 ? !gamma_rbq_resident(nb_bits, d) : knob == 1;
}

hipError_t gk::rabitq_scan(hipStream_t s, int nb_bits, int nq, int S, int d,
                           int nprobe, int k2, const float *queries,
                           const float *centroids,
                           const GammaBucketDev *buckets, int nlist,
                           const int64_t *probes, const uint32_t *bitmap,
                           bool ip, uint64_t *out_keys,
                           const int *kill_flag) {
  if (nq <= 0) return hipSuccess;
  if (!gamma_rbq_ok(d, nb_bits) || S <= 0 || nprobe <= 0 || k2 <= 0 ||
      k2 > GAMMA_DEEP_MAX_K)
    return hipErrorInvalidValue;
  const bool deep = k2 > 1024;
  const bool tiled = gk::rabitq_scan_is_tiled(nb_bits, d);
  const size_t smem =
      gamma_rbq_smem(nb_bits, d, k2, deep, tiled ? gamma_scan_bs() : 0);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  dim3 g((uint32_t)nq * (uint32_t)S);
  const int W = d * nb_bits / 32; /* code words; the entry is W + 2 */
  gamma_pick<1, 4, 8>(nb_bits, [&](auto b) {
    gamma_pick<0, 1>(ip, [&](auto ipc) {
      gamma_pick<256, 512>(gamma_scan_bs(), [&](auto bs) {
        auto launch = [&](auto u, auto nu) {
          constexpr int BSV = decltype(bs)::value;
          auto go = [&](auto kernel) {
            kernel<<<g, dim3(BSV), smem, s>>>(
                nq, S, d, nprobe, k2, queries, centroids, buckets, nlist,
                probes, bitmap, out_keys, kill_flag);
          };
          if (deep)
            go(k_rabitq_scan<decltype(ipc)::value, decltype(b)::value,
                             decltype(u)::value, decltype(nu)::value, BSV,
                             GammaDeepSelector>);
          else
            go(k_rabitq_scan<decltype(ipc)::value, decltype(b)::value,
                             decltype(u)::value, decltype(nu)::value, BSV>);
        };
        /* the table of the head comment: (U, NU) by entry size */
        if constexpr (decltype(b)::value == 1) {
          if (W == 1) launch(gamma_c<1>(), gamma_c<3>());      /* 12 bytes */
          else if (W == 2) launch(gamma_c<4>(), gamma_c<1>()); /* 16 */
          else if (W == 4) launch(gamma_c<2>(), gamma_c<3>()); /* 24 */
          else if (W == 8) launch(gamma_c<2>(), gamma_c<5>()); /* 40 */
          else if (W % 2 == 0) launch(gamma_c<2>(), gamma_c<0>());
          else launch(gamma_c<1>(), gamma_c<0>());
        } else if (tiled) {
          launch(gamma_c<2>(), gamma_c<-1>());
        } else { /* 40, 72 and 136 bytes in registers */
          if (!gamma_pick<8, 16, 32>(W, [&](auto w) {
                launch(gamma_c<2>(), gamma_c<decltype(w)::value / 2 + 1>());
              }))
            launch(gamma_c<2>(), gamma_c<0>());
        }
      });
    });
  });
  return hipGetLastError();
}
