/*
 * rabitq_kernels.hpp — kernels of the IVFRABITQ index (1-bit RaBitQ codes,
 * gamma_index_ivfrabitq.cc with nb_bits = 1). Included at the end of
 * kernels.hip after binary_kernels.hpp: it uses that file's gamma_bin_load,
 * kernels.hip's WG, the GAMMA_SCAN_BS launch knob (gamma_scan_bs in
 * ivfpq_scan_kernels.hpp) and scan_walk.hpp.
 *
 * An entry of a d-dimensional table is EW = d/32 + 2 little-endian words:
 * W = d/32 sign words (bit j of the vector is bit j&31 of word j>>5, the
 * BINARYIVF layout), then the factors A and Mul as fp32. With c the
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
 */
#pragma once

#define GAMMA_RBQ_DMAX 4096

/* fixed-order sum over the 64 lanes of a wave; every lane gets the total */
__device__ __forceinline__ float gamma_rbq_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* ------------------------------------------------------------- encode
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

hipError_t gk::rabitq_encode(hipStream_t s, int64_t n, int d, const float *x,
                             const int32_t *asg, int asg_const, int nlist,
                             const float *centroids, bool ip,
                             uint8_t *entries, float *svals) {
  if (n <= 0) return hipSuccess;
  if (d < 32 || d > GAMMA_RBQ_DMAX || d % 32 != 0 || nlist <= 0)
    return hipErrorInvalidValue;
  const int64_t g = (n + WG / 64 - 1) / (WG / 64);
  if (g > 0x7fffffffll) return hipErrorInvalidValue;
  k_rabitq_encode<<<dim3((uint32_t)g), dim3(WG), 0, s>>>(
      n, d, x, asg, asg_const, nlist, centroids, ip ? 1 : 0,
      (uint32_t *)entries, svals);
  return hipGetLastError();
}

/* Load path: sval of every stored entry from its sign words and its list's
 * centroid, block per bucket, wave per entry. Lane l of step t adds
 * c[t*64 + l] where the bit is set — the operands, the order and the tree
 * of k_rabitq_encode, so the rebuilt svals equal the encoded ones bit for
 * bit. */
__global__ void __launch_bounds__(WG)
k_rabitq_sval_buckets(int d, const GammaBucketDev *__restrict__ bks,
                      const float *__restrict__ centroids) {
  const GammaBucketDev bk = bks[blockIdx.x];
  if (!bk.svals || bk.size <= 0) return;
  const int lane = threadIdx.x & 63;
  const int W = d >> 5;
  const float *cv = centroids + (size_t)blockIdx.x * d;
  const uint32_t *data = (const uint32_t *)bk.data;
  float *out = (float *)bk.svals; /* writable: Load owns the buckets */
  for (long long j = threadIdx.x >> 6; j < bk.size; j += WG / 64) {
    const uint32_t *ent = data + (size_t)j * (W + 2);
    float sv = 0.0f;
    for (int t = 0; t * 64 < d; t++) {
      const int dim = t * 64 + lane;
      const bool act = dim < d;
      const uint32_t w = act ? ent[dim >> 5] : 0u;
      const bool bit = (w >> (lane & 31)) & 1u;
      const float cj = act ? cv[dim] : 0.0f;
      sv += bit ? cj : 0.0f;
    }
    sv = gamma_rbq_wave_sum(sv);
    if (lane == 0) out[j] = sv;
  }
}

hipError_t gk::rabitq_sval_buckets(hipStream_t s, int nlist, int d,
                                   const GammaBucketDev *bks,
                                   const float *centroids) {
  if (nlist <= 0) return hipSuccess;
  if (d < 32 || d > GAMMA_RBQ_DMAX || d % 32 != 0)
    return hipErrorInvalidValue;
  k_rabitq_sval_buckets<<<dim3((uint32_t)nlist), dim3(WG), 0, s>>>(
      d, bks, centroids);
  return hipGetLastError();
}

/* ---------------------------------------------------- RaBitQ IVF fused scan
 * The contract of k_binivf_scan and of k_ivfpq_scan's fast path, and their
 * chunked probe walk (scan_walk.hpp): a workgroup serves (query,
 * probe-split sub-block).
 *
 * Query table: lut[i][n], i < d/4, n < 16 = sum of q[4i + b] over the bits
 * b set in n, ascending b. A row is 16 consecutive LDS banks, so the 64
 * lanes of a gather hit at most 16 addresses in 16 different banks:
 * conflict-free for any code pattern, like the 4-bit ADC table and unlike
 * a 256-entry byte row. d/4 lookups per entry = 32 at d = 128, the count
 * of the 8-bit ADC scan at M = 32.
 *
 * Per-(query, probe) scalars qc2 = ||q - c||^2 and sqc = sum (q - c) are
 * recomputed per chunk from the centroid itself, 8 lanes per probe: lane l
 * sums dimensions l, l + 8, ... in order and the 8 partials meet in a
 * fixed xor tree. Block size and probe split do not enter, so a score
 * does not depend on the launch shape.
 *
 * U = words per load unit, NU > 0: the whole entry (sign words, A, Mul) is
 * NU units held in registers and double-buffered. NU == 0: the entry is
 * streamed in units of U (2 when d/32 is even, else 1) at consume time and
 * only id and sval are prefetched. */
struct GammaRbqPer {
  float qc2[GAMMA_SCAN_PCH];
  float sqc[GAMMA_SCAN_PCH];
};
struct GammaRbqChunk : GammaChunkT<GammaRbqPer> {
  float qq; /* ||q||^2 */
};

template <int U, int NU>
struct GammaRbqElem {
  uint32_t w[NU ? U * NU : 1];
  gamma_gu32p cw; /* NU == 0: the entry's words */
  uint32_t id;
  float sv, qc2, sqc;
  bool live;
};

/* dynamic LDS of k_rabitq_scan: table, selector scratch + result, query,
 * chunk */
__host__ __device__ static size_t gamma_rbq_sort_off(int d) {
  return (size_t)d * 16;
}
__host__ __device__ static size_t gamma_rbq_qs_off(int d, int k2) {
  return gamma_rbq_sort_off(d) + ((size_t)GAMMA_SORT_CAP + k2) * 8;
}
__host__ __device__ static size_t gamma_rbq_chunk_off(int d, int k2) {
  return (gamma_rbq_qs_off(d, k2) + (size_t)d * 4 + 7) / 8 * 8;
}
static size_t gamma_rbq_smem(int d, int k2) {
  return gamma_rbq_chunk_off(d, k2) + sizeof(GammaRbqChunk);
}

/* 8 nibble lookups of one sign word; tab advances by 8 rows */
__device__ __forceinline__ void gamma_rbq_word(uint32_t w, const float *&tab,
                                               float &s0, float &s1) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    s0 += tab[(i * 16) + ((w >> (4 * i)) & 15u)];
    s1 += tab[(i * 16 + 16) + ((w >> (4 * i + 4)) & 15u)];
  }
  tab += 128;
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

template <bool IP, int U, int NU, int BS>
__global__ void __launch_bounds__(BS)
k_rabitq_scan(int nq, int S, int d, int nprobe, int k2,
              const float *__restrict__ queries,
              const float *__restrict__ centroids,
              const GammaBucketDev *__restrict__ buckets, int nlist,
              const int64_t *__restrict__ probes,
              const uint32_t *__restrict__ bitmap,
              uint64_t *__restrict__ out_keys,
              const int *__restrict__ kill_flag) {
  extern __shared__ char smem[];
  float *lut = (float *)smem; /* d/4 x 16 */
  uint64_t *sortbuf = (uint64_t *)(smem + gamma_rbq_sort_off(d));
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  float *qs = (float *)(smem + gamma_rbq_qs_off(d, k2)); /* d */
  GammaRbqChunk *ch = (GammaRbqChunk *)(smem + gamma_rbq_chunk_off(d, k2));

  const int q = blockIdx.x / S;
  const int sub = blockIdx.x - q * S;
  if (q >= nq) return;
  const float *qg = queries + (int64_t)q * d;
  for (int i = threadIdx.x; i < d; i += BS) qs[i] = qg[i];

  GammaSelector sel;
  sel.init(sortbuf, res, ch->state, k2); /* has the barrier qs needs */

  for (int e = threadIdx.x; e < d * 4; e += BS) {
    const float *q4 = qs + (e >> 4) * 4;
    float t = 0.0f;
    if (e & 1) t += q4[0];
    if (e & 2) t += q4[1];
    if (e & 4) t += q4[2];
    if (e & 8) t += q4[3];
    lut[e] = t;
  }
  const unsigned tid = threadIdx.x;
  if (tid < 64) { /* wave 0: ||q||^2 by the scheme of the probe scalars */
    float s2, s1;
    gamma_rbq_qc(qs, nullptr, d, tid < 8 ? (int)tid : -1, s2, s1);
    if (tid == 0) ch->qq = s2;
  }
  __syncthreads();
  const float qq = ch->qq;
  const float inv_sqrt_d = 1.0f / sqrtf((float)d);

  constexpr int NW = NU ? U * NU : 1; /* NU > 0: words per entry */
  const int W = NU ? NW - 2 : (d >> 5);
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
        const float *tab = lut;
        if constexpr (NU > 0) {
#pragma unroll
          for (int i = 0; i < NW - 2; i++) gamma_rbq_word(e.w[i], tab, s0, s1);
          fa = __uint_as_float(e.w[NW - 2]);
          fm = __uint_as_float(e.w[NW - 1]);
        } else {
          for (int u = 0; u < W / U; u++) {
            uint32_t t[U];
            gamma_bin_load<U>(e.cw + u * U, t);
#pragma unroll
            for (int i = 0; i < U; i++) gamma_rbq_word(t[i], tab, s0, s1);
          }
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
        const float fd = (2.0f * dot - e.sqc) * inv_sqrt_d;
        const float pre = fa + e.qc2 - 2.0f * fm * fd;
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
    auto pass = [&](GammaRbqElem<U, NU> &nxt, const GammaRbqElem<U, NU> &cur_e,
                    unsigned it_nxt, int slot, bool check) {
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
  for (int i = threadIdx.x; i < k2; i += BS)
    out_keys[((int64_t)q * S + sub) * k2 + i] = res[i];
}

hipError_t gk::rabitq_scan(hipStream_t s, int nq, int S, int d, int nprobe,
                           int k2, const float *queries,
                           const float *centroids,
                           const GammaBucketDev *buckets, int nlist,
                           const int64_t *probes, const uint32_t *bitmap,
                           bool ip, uint64_t *out_keys,
                           const int *kill_flag) {
  if (nq <= 0) return hipSuccess;
  if (d < 32 || d > GAMMA_RBQ_DMAX || d % 32 != 0 || S <= 0 || nprobe <= 0 ||
      k2 <= 0 || k2 > 1024)
    return hipErrorInvalidValue;
  const int BS = gamma_scan_bs();
  const size_t smem = gamma_rbq_smem(d, k2);
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  dim3 g((uint32_t)nq * (uint32_t)S);
#define GAMMA_LAUNCH_RBQ3(IPV, UV, NUV, BSV)                                \
  k_rabitq_scan<IPV, UV, NUV, BSV><<<g, dim3(BSV), smem, s>>>(              \
      nq, S, d, nprobe, k2, queries, centroids, buckets, nlist, probes,     \
      bitmap, out_keys, kill_flag)
#define GAMMA_LAUNCH_RBQ(UV, NUV)                                           \
  do {                                                                      \
    if (ip) {                                                               \
      if (BS == 256) GAMMA_LAUNCH_RBQ3(true, UV, NUV, 256);                 \
      else GAMMA_LAUNCH_RBQ3(true, UV, NUV, 512);                           \
    } else {                                                                \
      if (BS == 256) GAMMA_LAUNCH_RBQ3(false, UV, NUV, 256);                \
      else GAMMA_LAUNCH_RBQ3(false, UV, NUV, 512);                          \
    }                                                                       \
  } while (0)
  const int W = d / 32;
  if (W == 1) GAMMA_LAUNCH_RBQ(1, 3);        /* 12-byte entries */
  else if (W == 2) GAMMA_LAUNCH_RBQ(4, 1);   /* 16 */
  else if (W == 4) GAMMA_LAUNCH_RBQ(2, 3);   /* 24 */
  else if (W == 8) GAMMA_LAUNCH_RBQ(2, 5);   /* 40 */
  else if (W % 2 == 0) GAMMA_LAUNCH_RBQ(2, 0);
  else GAMMA_LAUNCH_RBQ(1, 0);
#undef GAMMA_LAUNCH_RBQ
#undef GAMMA_LAUNCH_RBQ3
  return hipGetLastError();
}
