/*
 * binary_kernels.hpp — Hamming-distance kernels of the BINARYIVF index
 * (gamma_index_binary_ivf.cc). Included at the end of kernels.hip: it
 * uses that file's WG, the GAMMA_SCAN_BS launch knob (gamma_scan_bs in
 * ivfpq_scan_kernels.hpp) and scan_walk.hpp.
 *
 * A binary vector of d bits is W = d/32 little-endian u32 words (bit i of
 * the vector is bit i&31 of word i>>5, i.e. LSB-first inside each byte).
 * dist = sum_w popcount(q_w xor x_w): an integer <= d <= 4096, exact as
 * fp32, so it rides the ordinary (dist, id) u64 key with IP = false and
 * every comparison against a CPU reference is bit-exact.
 */
#pragma once

typedef uint32_t gamma_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t gamma_u32x4 __attribute__((ext_vector_type(4)));

/* U words of one entry, loaded as ONE global_load of the widest unit that
 * divides the entry (dwordx4 / dwordx2 / dword), xor'ed with the query
 * words and counted */
template <int U>
__device__ __forceinline__ void gamma_bin_load(gamma_gu32p p,
                                               uint32_t (&w)[U]) {
  if constexpr (U == 4) {
    gamma_u32x4 v =
        *(const __attribute__((address_space(1))) gamma_u32x4 *)p;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else if constexpr (U == 2) {
    gamma_u32x2 v =
        *(const __attribute__((address_space(1))) gamma_u32x2 *)p;
    w[0] = v.x; w[1] = v.y;
  } else {
    w[0] = *p;
  }
}

/* runtime-length entry: nu units of U words at p against the LDS query */
template <int U>
__device__ __forceinline__ int gamma_bin_dist_rt(gamma_gu32p p,
                                                 const uint32_t *qs,
                                                 int nu) {
  int h = 0;
  for (int u = 0; u < nu; u++) {
    uint32_t w[U];
    gamma_bin_load<U>(p + u * U, w);
#pragma unroll
    for (int i = 0; i < U; i++) h += __popc(w[i] ^ qs[u * U + i]);
  }
  return h;
}

/* ---------------------------------------------------- Hamming matrix
 * out[i*n + j] = popcount(Q_i xor B_j). A workgroup stages HM_TJ rows of
 * B in LDS (row stride W+1 words: odd, so the 64 lanes of a wave, one B
 * row each, hit 64 different banks for every W) and walks HM_QT queries;
 * wave v handles queries v, v+4, ... of the tile, lane = B row. The query
 * words are wave-uniform and come through the scalar cache. */
#define GAMMA_HM_TJ 64
#define GAMMA_HM_QT 64
__global__ void __launch_bounds__(WG)
k_hamming_matrix(const uint32_t *__restrict__ Q, int nq,
                 const uint32_t *__restrict__ B, int64_t n, int W,
                 float *__restrict__ out) {
  extern __shared__ char smem[];
  uint32_t *bs = (uint32_t *)smem; /* GAMMA_HM_TJ x (W+1) */
  const int64_t j0 = (int64_t)blockIdx.x * GAMMA_HM_TJ;
  const int rows = (int)min((int64_t)GAMMA_HM_TJ, n - j0);
  const uint32_t *bt = B + j0 * W;
  for (int e = threadIdx.x; e < rows * W; e += WG) {
    const int r = e / W, w = e - r * W;
    bs[r * (W + 1) + w] = bt[e];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i0 = blockIdx.y * GAMMA_HM_QT;
  const int i1 = min(nq, i0 + GAMMA_HM_QT);
  if (lane >= rows) return; /* no barrier below */
  const uint32_t *br = bs + lane * (W + 1);
  for (int i = i0 + wave; i < i1; i += WG / 64) {
    const uint32_t *qi = Q + (int64_t)i * W;
    int h = 0;
    for (int w = 0; w < W; w++) h += __popc(qi[w] ^ br[w]);
    out[(int64_t)i * n + j0 + lane] = (float)h;
  }
}

hipError_t gk::hamming_matrix(hipStream_t s, const uint32_t *Q, int nq,
                              const uint32_t *B, int64_t n, int W,
                              float *out) {
  if (nq <= 0 || n <= 0) return hipSuccess;
  if (W <= 0 || W > 128) return hipErrorInvalidValue;
  const int64_t gx = (n + GAMMA_HM_TJ - 1) / GAMMA_HM_TJ;
  const int gy = (nq + GAMMA_HM_QT - 1) / GAMMA_HM_QT;
  if (gx > 0x7fffffffll || gy > 65535) return hipErrorInvalidValue;
  const size_t smem = (size_t)GAMMA_HM_TJ * (W + 1) * 4;
  k_hamming_matrix<<<dim3((uint32_t)gx, (uint32_t)gy), dim3(WG), smem, s>>>(
      Q, nq, B, n, W, out);
  return hipGetLastError();
}

/* ------------------------------------------------- binary IVF fused scan
 * Same contract as k_ivfpq_scan's fast path and the same chunked probe
 * walk (scan_walk.hpp): a workgroup serves (query, probe-split sub-block).
 *
 * U = words per load unit (4/2/1, the widest that divides W). NU > 0:
 * the entry is NU units held in registers, the query words live in
 * registers too, and a pass prefetches id + entry. NU == 0: entry length
 * is a runtime count of units; only the id is prefetched and the entry is
 * streamed unit by unit against the query words in LDS (same-address
 * reads, broadcast). */
template <int U, int NU>
struct GammaBinElem {
  uint32_t w[NU ? U * NU : 1];
  gamma_gu32p cw; /* NU == 0: the entry's words */
  uint32_t id;
  bool live;
};

/* dynamic LDS of k_binivf_scan: selector scratch + result, query, chunk */
__host__ __device__ static size_t gamma_binscan_qs_off(int k2) {
  return ((size_t)GAMMA_SORT_CAP + k2) * 8;
}
__host__ __device__ static size_t gamma_binscan_chunk_off(int k2, int W) {
  return (gamma_binscan_qs_off(k2) + (size_t)W * 4 + 7) / 8 * 8;
}

template <int U, int NU, int BS>
__global__ void __launch_bounds__(BS)
k_binivf_scan(int nq, int S, int W, int nprobe, int k2,
              const uint32_t *__restrict__ queries,
              const GammaBucketDev *__restrict__ buckets, int nlist,
              const int64_t *__restrict__ probes,
              const uint32_t *__restrict__ bitmap,
              uint64_t *__restrict__ out_keys,
              const int *__restrict__ kill_flag) {
  extern __shared__ char smem[];
  uint64_t *sortbuf = (uint64_t *)smem;
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  uint32_t *qs = (uint32_t *)(smem + gamma_binscan_qs_off(k2)); /* W */
  GammaScanChunk *ch =
      (GammaScanChunk *)(smem + gamma_binscan_chunk_off(k2, W));

  const int q = blockIdx.x / S;
  const int sub = blockIdx.x - q * S;
  if (q >= nq) return;
  const uint32_t *qg = queries + (int64_t)q * W;
  for (int i = threadIdx.x; i < W; i += BS) qs[i] = qg[i];

  GammaSelector sel;
  sel.init(sortbuf, res, ch->state, k2); /* has the barrier qs needs */

  constexpr int NW = NU ? U * NU : 1;
  uint32_t qr[NW];
  if (NU > 0) {
#pragma unroll
    for (int i = 0; i < NW; i++) qr[i] = qs[i];
  }
  const int nu_rt = W / U; /* units per entry (NU == 0 path) */

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
      if (ln >= 0 && ln < nlist) bk = buckets[ln];
      gamma_chunk_put<false>(ch, tid, bk);
    }
    const GammaChunkSpan sp = gamma_chunk_close(ch, cn, kill_flag);
    c0 += sp.ncons;

    GammaListCursor cur;
    cur.reset(ch, sp.total);
    gamma_gu32p pid = ch->ids[0];
    gamma_gu32p pcodes = (gamma_gu32p)ch->codes[0];

    auto fetch = [&](GammaBinElem<U, NU> &e, unsigned it) {
      const unsigned j = cur.seek(ch, it * BS + tid, e.live, [&](int li) {
        pid = ch->ids[li];
        pcodes = (gamma_gu32p)ch->codes[li];
      });
      e.id = pid[j];
      e.cw = pcodes + (size_t)j * W;
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
    auto retire = [&](const GammaBinElem<U, NU> &e) {
      if constexpr (NU > 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) asm volatile("" ::"v"(e.w[i]));
      }
      asm volatile("" ::"v"(e.id));
    };
    auto consume = [&](const GammaBinElem<U, NU> &e) {
      int h = 0;
      if constexpr (NU > 0) {
        retire(e);
#pragma unroll
        for (int i = 0; i < NW; i++) h += __popc(e.w[i] ^ qr[i]);
      } else {
        h = gamma_bin_dist_rt<U>(e.cw, qs, nu_rt);
      }
      if (e.live && !(e.id >> 31) &&
          !gamma_bitmap_test(bitmap, (uint64_t)e.id))
        sel.push(gamma_make_key<false>((float)h, e.id));
    };
    /* flush check, kill poll and the two-set pass loop: the scheme of
     * k_ivfpq_scan's fast path (reasons there) */
    killed = sp.killed;
    const unsigned niter = (sp.total + BS - 1) / BS;
    const bool flush_each = k2 + 2 * BS > GAMMA_SORT_CAP;
    const int fmargin = flush_each ? BS : 2 * BS;
    auto pass = [&](GammaBinElem<U, NU> &nxt, const GammaBinElem<U, NU> &cur_e,
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
      GammaBinElem<U, NU> ea, eb;
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

hipError_t gk::binivf_scan(hipStream_t s, int nq, int S, int W, int nprobe,
                           int k2, const uint32_t *queries,
                           const GammaBucketDev *buckets, int nlist,
                           const int64_t *probes, const uint32_t *bitmap,
                           uint64_t *out_keys, const int *kill_flag) {
  if (nq <= 0) return hipSuccess;
  if (W <= 0 || W > 128 || S <= 0 || nprobe <= 0 || k2 <= 0 || k2 > 1024)
    return hipErrorInvalidValue;
  const int BS = gamma_scan_bs();
  const size_t smem = gamma_binscan_chunk_off(k2, W) + sizeof(GammaScanChunk);
  dim3 g((uint32_t)nq * (uint32_t)S);
#define GAMMA_LAUNCH_BIN(UV, NUV)                                          \
  do {                                                                     \
    if (BS == 256)                                                         \
      k_binivf_scan<UV, NUV, 256><<<g, dim3(256), smem, s>>>(              \
          nq, S, W, nprobe, k2, queries, buckets, nlist, probes, bitmap,   \
          out_keys, kill_flag);                                            \
    else                                                                   \
      k_binivf_scan<UV, NUV, 512><<<g, dim3(512), smem, s>>>(              \
          nq, S, W, nprobe, k2, queries, buckets, nlist, probes, bitmap,   \
          out_keys, kill_flag);                                            \
  } while (0)
  if (W == 1) GAMMA_LAUNCH_BIN(1, 1);
  else if (W == 2) GAMMA_LAUNCH_BIN(2, 1);
  else if (W == 3) GAMMA_LAUNCH_BIN(1, 3);
  else if (W == 4) GAMMA_LAUNCH_BIN(4, 1);
  else if (W == 8) GAMMA_LAUNCH_BIN(4, 2);
  else if (W % 4 == 0) GAMMA_LAUNCH_BIN(4, 0);
  else if (W % 2 == 0) GAMMA_LAUNCH_BIN(2, 0);
  else GAMMA_LAUNCH_BIN(1, 0);
#undef GAMMA_LAUNCH_BIN
  return hipGetLastError();
}

/* ------------------------------------------------- Hamming flat scan
 * Brute force over the raw segment table, the binary sibling of
 * k_flat_stream: one workgroup per query, thread tid takes vector
 * it*WG + tid (an entry is W contiguous words, loaded in units of U), one
 * push per thread per pass, flush check every pass. A lane past n
 * re-reads vector n-1 and is marked dead, so the loads are unconditional. */
template <int U>
__global__ void __launch_bounds__(WG)
k_hamming_flat(int nq, int64_t n, int W, int k2,
               const uint32_t *__restrict__ queries,
               const uint32_t *const *__restrict__ segs, int seg_shift,
               const uint32_t *__restrict__ bitmap,
               uint64_t *__restrict__ out_keys) {
  extern __shared__ char smem[];
  uint64_t *sortbuf = (uint64_t *)smem;
  uint64_t *res = sortbuf + GAMMA_SORT_CAP;
  uint32_t *qs = (uint32_t *)(res + k2);
  int *state = (int *)(qs + W);

  const int q = blockIdx.x;
  if (q >= nq) return;
  const uint32_t *qg = queries + (int64_t)q * W;
  for (int i = threadIdx.x; i < W; i += WG) qs[i] = qg[i];

  GammaSelector sel;
  sel.init(sortbuf, res, state, k2);

  const int64_t seg_mask = ((int64_t)1 << seg_shift) - 1;
  const int nu = W / U;
  const int64_t iters = (n + WG - 1) / WG;
  for (int64_t it = 0; it < iters; it++) {
    const int64_t j0 = it * WG + threadIdx.x;
    const bool live = j0 < n;
    const int64_t j = live ? j0 : n - 1;
    gamma_gu32p v = (gamma_gu32p)(segs[j >> seg_shift] +
                                  (size_t)(j & seg_mask) * W);
    const int h = gamma_bin_dist_rt<U>(v, qs, nu);
    if (live && !gamma_bitmap_test(bitmap, (uint64_t)j))
      sel.push(gamma_make_key<false>((float)h, (uint32_t)j));
    sel.maybe_flush(WG);
  }
  sel.finish();
  for (int i = threadIdx.x; i < k2; i += WG)
    out_keys[(int64_t)q * k2 + i] = res[i];
}

hipError_t gk::hamming_flat_scan(hipStream_t s, int nq, int64_t n, int W,
                                 int k2, const uint32_t *queries,
                                 const uint32_t *const *segs, int seg_shift,
                                 const uint32_t *bitmap,
                                 uint64_t *out_keys) {
  if (nq <= 0) return hipSuccess;
  if (W <= 0 || W > 128 || k2 <= 0 || k2 > 1024 || n < 0 ||
      n > 0x7fffffffll)
    return hipErrorInvalidValue;
  const size_t smem = ((size_t)GAMMA_SORT_CAP + k2) * 8 + (size_t)W * 4 +
                      4 * sizeof(int);
  if (W % 4 == 0)
    k_hamming_flat<4><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, n, W, k2, queries, segs, seg_shift, bitmap, out_keys);
  else if (W % 2 == 0)
    k_hamming_flat<2><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, n, W, k2, queries, segs, seg_shift, bitmap, out_keys);
  else
    k_hamming_flat<1><<<dim3(nq), dim3(WG), smem, s>>>(
        nq, n, W, k2, queries, segs, seg_shift, bitmap, out_keys);
  return hipGetLastError();
}
