/*
 * rabitq_ex_kernels.hpp — the multi-bit IVFRABITQ kernels (nb_bits B = 4 or
 * 8). Included by kernels.hip behind rabitq_kernels.hpp: it uses that file's
 * gamma_rbq_wave_sum, gamma_rbq_qc, GammaRbqChunk and GAMMA_RBQ_DMAX,
 * binary_kernels.hpp's gamma_bin_load, the GAMMA_SCAN_BS knob and
 * scan_walk.hpp. The 1-bit kernels are not touched.
 *
 * The code (L = 2^(B-1), c the centroid of the vector's list, d % 32 == 0):
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
 */
#pragma once

/* The encode and sval kernels are built without packed fp32 instructions,
 * so every sum stays a chain of single fused operations; their lambdas are
 * always_inline because the inliner refuses a callee whose target features
 * differ. The scan calls the shared selector, which is not always_inline,
 * so it keeps the default features and issues its FMAs itself
 * (gamma_rbq_ex_fma). */
#if defined(__HIP_DEVICE_COMPILE__)
#define GAMMA_RBQ_EX_KERNEL \
  __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define GAMMA_RBQ_EX_KERNEL __global__
#endif
#define GAMMA_RBQ_EX_INLINE __attribute__((always_inline))

template <int B>
struct GammaRbqEx {
  static_assert(B == 4 || B == 8, "code widths of the multi-bit layout");
  static constexpr int L = 1 << (B - 1);
  static constexpr int DPW = 32 / B;            /* dimensions per word */
  static constexpr int SH = B == 4 ? 3 : 2;     /* log2(DPW) */
  static constexpr uint32_t MASK = (1u << B) - 1u;
  static constexpr float CB = (float)((1 << B) - 1) * 0.5f;
};

/* ------------------------------------------------------------- encode
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
  typedef GammaRbqEx<B> P;
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

static bool gamma_rbq_ex_ok(int d, int nb_bits) {
  return (nb_bits == 4 || nb_bits == 8) && d >= 32 && d <= GAMMA_RBQ_DMAX &&
         d % 32 == 0;
}

hipError_t gk::rabitq_encode_ex(hipStream_t s, int nb_bits, int64_t n, int d,
                                const float *x, const int32_t *asg,
                                int asg_const, int nlist,
                                const float *centroids, bool ip,
                                uint8_t *entries, float *svals) {
  if (n <= 0) return hipSuccess;
  if (!gamma_rbq_ex_ok(d, nb_bits) || nlist <= 0) return hipErrorInvalidValue;
  const int64_t g = (n + WG / 64 - 1) / (WG / 64);
  if (g > 0x7fffffffll) return hipErrorInvalidValue;
#define GAMMA_LAUNCH_RBQ_ENC(BV, TRV)                                       \
  k_rabitq_encode_ex<BV, TRV><<<dim3((uint32_t)g), dim3(WG), 0, s>>>(       \
      n, d, x, asg, asg_const, nlist, centroids, ip ? 1 : 0,                \
      (uint32_t *)entries, svals)
#define GAMMA_LAUNCH_RBQ_ENC_B(BV)                                          \
  do {                                                                      \
    if (d <= 128) GAMMA_LAUNCH_RBQ_ENC(BV, 2);                              \
    else if (d <= 512) GAMMA_LAUNCH_RBQ_ENC(BV, 8);                         \
    else GAMMA_LAUNCH_RBQ_ENC(BV, 0);                                       \
  } while (0)
  if (nb_bits == 4) GAMMA_LAUNCH_RBQ_ENC_B(4);
  else GAMMA_LAUNCH_RBQ_ENC_B(8);
#undef GAMMA_LAUNCH_RBQ_ENC_B
#undef GAMMA_LAUNCH_RBQ_ENC
  return hipGetLastError();
}

/* Load path: sval = sum_j u_j c_j of every stored entry, block per bucket,
 * wave per entry: the lane order, the fmaf chain and the tree of
 * k_rabitq_encode_ex, so the rebuilt svals equal the encoded ones bit for
 * bit. */
template <int B>
GAMMA_RBQ_EX_KERNEL void __launch_bounds__(WG)
k_rabitq_sval_buckets_ex(int d, const GammaBucketDev *__restrict__ bks,
                         const float *__restrict__ centroids) {
  typedef GammaRbqEx<B> P;
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
      if (dim < d) {
        const uint32_t u =
            (ent[dim >> P::SH] >> (B * (dim & (P::DPW - 1)))) & P::MASK;
        sv = fmaf((float)u, cv[dim], sv);
      }
    }
    sv = gamma_rbq_wave_sum(sv);
    if (lane == 0) out[j] = sv;
  }
}

hipError_t gk::rabitq_sval_buckets_ex(hipStream_t s, int nb_bits, int nlist,
                                      int d, const GammaBucketDev *bks,
                                      const float *centroids) {
  if (nlist <= 0) return hipSuccess;
  if (!gamma_rbq_ex_ok(d, nb_bits)) return hipErrorInvalidValue;
  if (nb_bits == 4)
    k_rabitq_sval_buckets_ex<4><<<dim3((uint32_t)nlist), dim3(WG), 0, s>>>(
        d, bks, centroids);
  else
    k_rabitq_sval_buckets_ex<8><<<dim3((uint32_t)nlist), dim3(WG), 0, s>>>(
        d, bks, centroids);
  return hipGetLastError();
}

/* ------------------------------------------------- multi-bit fused scan
 * The contract and the chunked probe walk of k_rabitq_scan; the inner
 * product sum_j u_j q_j is formed differently. There is no lookup table: a
 * lane owns one entry, holds its code words in VGPRs and accumulates
 * fmaf((float)u_j, q_j, acc) over the unpacked fields. B = 4: two masks
 * per word (w & 0x0f0f0f0f, (w >> 4) & 0x0f0f0f0f) put the even and the odd
 * nibbles into byte lanes, then eight byte-to-float conversions; B = 8:
 * four conversions and no mask. q_j is the same for all 64 lanes: the
 * query row is read through the constant address space with a uniform
 * index, i.e. by scalar loads into SGPRs, and enters the FMA as its scalar
 * operand — LDS serves only the selector, the chunk and the qs copy that
 * gamma_rbq_qc reads.
 *
 * Summation order, fixed per entry: j ascending inside a word; even words
 * into s0, odd words into s1, s0 + s1 at the end. BS, S and the entry
 * movement do not enter.
 *
 * NU > 0: the whole entry (code words, A, Mul) is NU 8-byte units held in
 * registers and double-buffered. NU == 0: the entry is streamed in 8-byte
 * units at consume time; only id and sval are prefetched. */
typedef const __attribute__((address_space(4))) float *gamma_cf32p;

template <int NU>
struct GammaRbqExElem {
  uint32_t w[NU ? 2 * NU : 1];
  gamma_gu32p cw; /* NU == 0: the entry's words */
  uint32_t id;
  float sv, qc2, sqc;
  bool live;
};

/* dynamic LDS of k_rabitq_scan_ex: selector scratch + result, query,
 * chunk */
__host__ __device__ static size_t gamma_rbq_ex_qs_off(int k2) {
  return ((size_t)GAMMA_SORT_CAP + k2) * 8;
}
__host__ __device__ static size_t gamma_rbq_ex_chunk_off(int d, int k2) {
  return (gamma_rbq_ex_qs_off(k2) + (size_t)d * 4 + 7) / 8 * 8;
}
static size_t gamma_rbq_ex_smem(int d, int k2) {
  return gamma_rbq_ex_chunk_off(d, k2) + sizeof(GammaRbqChunk);
}

/* acc += u * q as ONE v_fmac_f32 with q, wave-uniform, as its scalar
 * operand. Written out so that the two accumulator chains stay chains of
 * single fused operations in ascending j: left to the vectorizer they are
 * paired into packed FMAs. */
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

template <bool IP, int B, int NU, int BS>
__global__ void __launch_bounds__(BS)
k_rabitq_scan_ex(int nq, int S, int d, int nprobe, int k2,
                 const float *__restrict__ queries,
                 const float *__restrict__ centroids,
                 const GammaBucketDev *__restrict__ buckets, int nlist,
                 const int64_t *__restrict__ probes,
                 const uint32_t *__restrict__ bitmap,
                 uint64_t *__restrict__ out_keys,
                 const int *__restrict__ kill_flag) {
  typedef GammaRbqEx<B> P;
  extern __shared__ char smem[];
  uint64_t *sortbuf = (uint64_t *)smem;
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(smem + gamma_rbq_ex_qs_off(k2)); /* d */
  GammaRbqChunk *ch =
      (GammaRbqChunk *)(smem + gamma_rbq_ex_chunk_off(d, k2));

  const int q = blockIdx.x / S;
  const int sub = blockIdx.x - q * S;
  if (q >= nq) return;
  const float *qg = queries + (int64_t)q * d;
  const gamma_cf32p qc = (gamma_cf32p)qg; /* read-only for the launch */
  for (int i = threadIdx.x; i < d; i += BS) qs[i] = qg[i];

  GammaSelector sel;
  sel.init(sortbuf, res, ch->state, k2); /* has the barrier qs needs */

  const unsigned tid = threadIdx.x;
  if (tid < 64) { /* wave 0: ||q||^2 by the scheme of the probe scalars */
    float s2, s1;
    gamma_rbq_qc(qs, nullptr, d, tid < 8 ? (int)tid : -1, s2, s1);
    if (tid == 0) ch->qq = s2;
  }
  __syncthreads();
  const float qq = ch->qq;

  constexpr int NW = NU ? 2 * NU : 2; /* NU > 0: words per entry */
  const int W = NU ? NW - 2 : d / P::DPW;
  const int EW = W + 2;

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

    auto fetch = [&](GammaRbqExElem<NU> &e,
                     unsigned it) {
      const unsigned j = cur.seek(ch, it * BS + tid, e.live,
                                  [&](int li) {
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
          uint32_t t[2];
          gamma_bin_load<2>(e.cw + u * 2, t);
          e.w[u * 2] = t[0];
          e.w[u * 2 + 1] = t[1];
        }
      }
    };
    auto retire =
        [&](const GammaRbqExElem<NU> &e) {
      if constexpr (NU > 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) asm volatile("" ::"v"(e.w[i]));
      }
      asm volatile("" ::"v"(e.id));
      asm volatile("" ::"v"(e.sv));
    };
    auto consume =
        [&](const GammaRbqExElem<NU> &e) {
      retire(e);
      if (e.live && !(e.id >> 31) &&
          !gamma_bitmap_test(bitmap, (uint64_t)e.id)) {
        float s0 = 0.0f, s1 = 0.0f, fa, fm;
        if constexpr (NU > 0) {
#pragma unroll
          for (int u = 0; u < NU - 1; u++) {
            gamma_rbq_ex_word<B>(e.w[2 * u], qc + 2 * u * P::DPW, s0);
            gamma_rbq_ex_word<B>(e.w[2 * u + 1], qc + (2 * u + 1) * P::DPW,
                                 s1);
          }
          fa = __uint_as_float(e.w[NW - 2]);
          fm = __uint_as_float(e.w[NW - 1]);
        } else {
          gamma_cf32p qp = qc;
          for (int u = 0; u < W; u += 2, qp += 2 * P::DPW) {
            uint32_t t[2];
            gamma_bin_load<2>(e.cw + u, t);
            gamma_rbq_ex_word<B>(t[0], qp, s0);
            gamma_rbq_ex_word<B>(t[1], qp + P::DPW, s1);
          }
          uint32_t f[2];
          gamma_bin_load<2>(e.cw + W, f);
          fa = __uint_as_float(f[0]);
          fm = __uint_as_float(f[1]);
        }
        const float dot = (s0 + s1) - e.sv;
        const float t = fmaf(-P::CB, e.sqc, dot);
        const float pre = fmaf(-2.0f * fm, t, fa + e.qc2);
        const float score = IP ? -0.5f * (pre - qq) : pre;
        sel.push(gamma_make_key<IP>(score, e.id));
      }
    };

    /* flush check, kill poll and the two-set pass loop: the scheme of
     * k_ivfpq_scan's fast path (reasons there) */
    killed = sp.killed;
    const unsigned niter = (sp.total + BS - 1) / BS;
    const bool flush_each = k2 + 2 * BS > GAMMA_SORT_CAP;
    const int fmargin = flush_each ? BS : 2 * BS;
    auto pass = [&](GammaRbqExElem<NU> &nxt, const GammaRbqExElem<NU> &cur_e,
                    unsigned it_nxt, int slot,
                    bool check) {
      const int kv = __hip_atomic_load(kf, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
      fetch(nxt, it_nxt);
      consume(cur_e);
      asm volatile("" ::"v"(kv));
      if (!check) return false;
      if (tid == 0) ch->kill[slot] = kill_flag ? kv : 0;
      sel.maybe_flush(fmargin);
      return ch->kill[slot] != 0;
    };
    if (niter > 0) {
      GammaRbqExElem<NU> ea, eb;
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
  for (int i = threadIdx.x; i < k2; i += BS)
    out_keys[((int64_t)q * S + sub) * k2 + i] = res[i];
}

hipError_t gk::rabitq_scan_ex(hipStream_t s, int nb_bits, int nq, int S,
                              int d, int nprobe, int k2, const float *queries,
                              const float *centroids,
                              const GammaBucketDev *buckets, int nlist,
                              const int64_t *probes, const uint32_t *bitmap,
                              bool ip, uint64_t *out_keys,
                              const int *kill_flag) {
  if (nq <= 0) return hipSuccess;
  if (!gamma_rbq_ex_ok(d, nb_bits) || S <= 0 || nprobe <= 0 || k2 <= 0 ||
      k2 > 1024)
    return hipErrorInvalidValue;
  const int BS = gamma_scan_bs();
  const size_t smem = gamma_rbq_ex_smem(d, k2);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  dim3 g((uint32_t)nq * (uint32_t)S);
#define GAMMA_LAUNCH_RBQX3(IPV, BV, NUV, BSV)                               \
  k_rabitq_scan_ex<IPV, BV, NUV, BSV><<<g, dim3(BSV), smem, s>>>(           \
      nq, S, d, nprobe, k2, queries, centroids, buckets, nlist, probes,     \
      bitmap, out_keys, kill_flag)
#define GAMMA_LAUNCH_RBQX(BV, NUV)                                          \
  do {                                                                      \
    if (ip) {                                                               \
      if (BS == 256) GAMMA_LAUNCH_RBQX3(true, BV, NUV, 256);                \
      else GAMMA_LAUNCH_RBQX3(true, BV, NUV, 512);                          \
    } else {                                                                \
      if (BS == 256) GAMMA_LAUNCH_RBQX3(false, BV, NUV, 256);               \
      else GAMMA_LAUNCH_RBQX3(false, BV, NUV, 512);                         \
    }                                                                       \
  } while (0)
  const int W = d * nb_bits / 32; /* code words; the entry is W + 2 */
  if (nb_bits == 4) {
    if (W == 8) GAMMA_LAUNCH_RBQX(4, 5);        /* d = 64: 40-byte entries */
    else if (W == 16) GAMMA_LAUNCH_RBQX(4, 9);  /* d = 128: 72 */
    else if (W == 32) GAMMA_LAUNCH_RBQX(4, 17); /* d = 256: 136 */
    else GAMMA_LAUNCH_RBQX(4, 0);
  } else {
    if (W == 8) GAMMA_LAUNCH_RBQX(8, 5);        /* d = 32: 40 */
    else if (W == 16) GAMMA_LAUNCH_RBQX(8, 9);  /* d = 64: 72 */
    else if (W == 32) GAMMA_LAUNCH_RBQX(8, 17); /* d = 128: 136 */
    else GAMMA_LAUNCH_RBQX(8, 0);
  }
#undef GAMMA_LAUNCH_RBQX
#undef GAMMA_LAUNCH_RBQX3
  return hipGetLastError();
}
