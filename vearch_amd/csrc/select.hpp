/*
 * select.hpp — device-side exact top-k selection on u64 (dist,id) keys.
 *
 * Key layout: upper 32 bits = monotone u32 image of the fp32 distance
 * (sign-flip trick; inverted for inner-product so ascending key ==
 * descending similarity), lower 32 bits = docid. One integer compare gives
 * the exact (dist, id) total order — ties break by id deterministically
 * (SURVEY §8c pin (i)); replaces the reference's faiss CMin/CMax heaps
 * (gamma_index_ivfpq.cc:606-631, gamma_index_flat.cc:80-83).
 *
 * GammaSelector: each thread keeps a register buffer of candidates better
 * than the current block-wide threshold; the buffers are periodically
 * dumped to LDS and bitonic-merged with the running top-k, which
 * re-tightens the threshold. Exact: a candidate is dropped only when it is
 * >= the k-th best key seen so far.
 *
 * Protocol: between two maybe_flush() calls, each thread may push() at
 * most GAMMA_SEL_CHUNK candidates. All threads of the block must reach
 * maybe_flush()/finish() together (they contain barriers).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GAMMA_KEY_EMPTY 0xffffffffffffffffull

__device__ __forceinline__ uint32_t gamma_f32_key(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float gamma_key_f32(uint32_t dk) {
  uint32_t u = (dk & 0x80000000u) ? (dk & 0x7fffffffu) : ~dk;
  return __uint_as_float(u);
}

template <bool IP>
__device__ __forceinline__ uint64_t gamma_make_key(float dist, uint32_t id) {
  uint32_t dk = gamma_f32_key(dist);
  if (IP) dk = ~dk;
  return ((uint64_t)dk << 32) | (uint64_t)id;
}

template <bool IP>
__device__ __forceinline__ float gamma_key_dist(uint64_t key) {
  uint32_t dk = (uint32_t)(key >> 32);
  if (IP) dk = ~dk;
  return gamma_key_f32(dk);
}

__device__ __forceinline__ int64_t gamma_key_id(uint64_t key) {
  return (key == GAMMA_KEY_EMPTY) ? (int64_t)-1
                                  : (int64_t)(key & 0xffffffffull);
}

/* In-LDS bitonic sort (ascending) of buf[0..n), n a power of two.
 * Call with all threads of the block; barriers inside. */
__device__ inline void gamma_bitonic_sort(uint64_t *buf, int n) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int len = 2; len <= n; len <<= 1) {
    for (int inc = len >> 1; inc > 0; inc >>= 1) {
      __syncthreads();
      for (int i = tid; i < n; i += nt) {
        int j = i ^ inc;
        if (j > i) {
          bool up = (i & len) == 0;
          uint64_t a = buf[i], b = buf[j];
          if ((a > b) == up) { buf[i] = b; buf[j] = a; }
        }
      }
    }
  }
  __syncthreads();
}

#define GAMMA_SORT_CAP 2048   /* LDS sort scratch, u64 x 2048 = 16 KB */
#define GAMMA_SEL_MAX_K 1088  /* cap - margin must stay >= 0 */

/* Candidates append into the shared LDS buffer through one LDS atomic;
 * all selector state is scalar registers or LDS (no per-thread arrays —
 * runtime-indexed register arrays land in scratch memory, §5.4 rule 20,
 * which made v1 of this selector 60x slower).
 *
 * Invariant: the caller calls maybe_flush(margin) (all threads together)
 * often enough that at most `margin` pushes can happen block-wide between
 * two checks; the buffer then never overflows its cap = SORT_CAP - k. */
struct GammaSelector {
  uint64_t *sortbuf;  /* uint64_t[GAMMA_SORT_CAP] in LDS */
  uint64_t *res;      /* uint64_t[k] in LDS, sorted ascending after flush */
  int *state;         /* int[1] in LDS: append counter */
  int k, cap;
  uint64_t thresh;

  __device__ void init(uint64_t *sortbuf_, uint64_t *res_, int *state_,
                       int k_) {
    sortbuf = sortbuf_; res = res_; state = state_; k = k_;
    cap = GAMMA_SORT_CAP - k;
    thresh = GAMMA_KEY_EMPTY;
    for (int i = threadIdx.x; i < k; i += blockDim.x) res[i] = GAMMA_KEY_EMPTY;
    if (threadIdx.x == 0) state[0] = 0;
    __syncthreads();
  }

  /* seed the running result with previously selected keys (unsorted ok) */
  __device__ void seed(const uint64_t *keys, int n) {
    for (int i = threadIdx.x; i < k; i += blockDim.x)
      res[i] = (i < n) ? keys[i] : GAMMA_KEY_EMPTY;
    __syncthreads();
    flush_();
  }

  __device__ __forceinline__ void push(uint64_t key) {
    if (key < thresh) {
      int idx = atomicAdd(&state[0], 1);
      sortbuf[idx] = key; /* in range by the maybe_flush invariant */
    }
  }

  /* all threads must arrive together */
  __device__ __forceinline__ void maybe_flush(int margin) {
    __syncthreads();
    if (state[0] > cap - margin) flush_();
  }

  __device__ void finish() {
    __syncthreads();
    flush_();
  }

  /* An unconditional flush in the place of a maybe_flush (all threads
   * together; the append counter restarts at 0, so the margin invariant
   * holds behind it). Afterwards thresh is the true k-th key of everything
   * pushed so far, or still GAMMA_KEY_EMPTY where fewer than k keys came. */
  __device__ void flush_now() {
    __syncthreads();
    flush_();
  }

 private:
  __device__ void flush_() {
    const int nt = blockDim.x, tid = threadIdx.x;
    int total = state[0];
    if (total > cap) total = cap; /* belt & braces */
    /* append res at [total, total+k), pad to pow2, sort, keep k */
    int n = 1;
    while (n < total + k) n <<= 1;
    __syncthreads();
    for (int i = total + k + tid; i < n; i += nt)
      sortbuf[i] = GAMMA_KEY_EMPTY;
    for (int i = tid; i < k; i += nt) sortbuf[total + i] = res[i];
    gamma_bitonic_sort(sortbuf, n);
    for (int i = tid; i < k; i += nt) res[i] = sortbuf[i];
    if (tid == 0) state[0] = 0;
    __syncthreads();
    thresh = res[k - 1];
  }
};

/* ------------------------------------------------------------------------
 * Deep top-k (1024 < k <= GAMMA_DEEP_MAX_K). k keys plus an append region
 * of the same order do not fit LDS next to a scan's own staging, and a
 * bitonic flush over 16 K keys is the wrong algorithm, so the running
 * state lives in global memory and is compacted by radix select
 * (DESIGN.md "Deep top-k").
 *
 * gamma_radix_kth: MSD radix select over the n keys load(0..n): 8-bit
 * digits from the top, a 256-bin LDS histogram per pass, wave 0 scans the
 * bins for the one that holds rank kth (1-based, among the keys that are
 * not EMPTY). It stops as soon as that bin holds ONE key: real keys are
 * distinct (ids are), so after at most 8 passes it does. Result: (shift,
 * prefix) with exactly min(kth, real keys) real keys satisfying
 *   (key >> shift) <= (prefix >> shift);
 * the key with equality there is the kth smallest. Fewer than kth + 1 real
 * keys: shift = 0, prefix = EMPTY - 1 (every real key). All threads call
 * it together; barriers inside. */
#define GAMMA_DEEP_MAX_K 8192
#define GAMMA_DEEP_REGION(k) (4 * (size_t)(k)) /* keys per region */

struct GammaRadixLds {
  uint32_t hist[256];
  uint32_t bin, before, count, total;
  uint32_t wcnt[2][16]; /* per-wave keep counts of a compaction tile */
  uint32_t nkeep, pad;
  uint64_t pivot;
};

template <class Load>
__device__ inline void gamma_radix_kth(Load load, int n, int kth,
                                       GammaRadixLds *lds, int &shift,
                                       uint64_t &prefix) {
  const int tid = threadIdx.x, nt = blockDim.x;
  uint32_t r = (uint32_t)kth;
  prefix = 0;
  for (int p = 0; p < 8; p++) {
    const int sh = 56 - 8 * p;
    const uint64_t himask = p ? ~0ull << (sh + 8) : 0ull;
    for (int i = tid; i < 256; i += nt) lds->hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
      const uint64_t key = load(i);
      if (key != GAMMA_KEY_EMPTY && (key & himask) == prefix)
        atomicAdd(&lds->hist[(uint32_t)(key >> sh) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) { /* wave 0: lane l owns bins 4l .. 4l+3 */
      uint32_t c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) { c[j] = lds->hist[4 * tid + j]; s += c[j]; }
      uint32_t incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (tid >= o) incl += t;
      }
      uint32_t excl = incl - s;
      if (excl < r && r <= incl) { /* one lane: the bins partition the keys */
        int b = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
          if (r > excl + c[j] && b == j) { excl += c[j]; b = j + 1; }
        lds->bin = 4 * tid + b;
        lds->before = excl;
        lds->count = b == 0 ? c[0] : b == 1 ? c[1] : b == 2 ? c[2] : c[3];
      }
      if (tid == 63) lds->total = incl;
    }
    __syncthreads();
    if (lds->total < r || (p == 0 && lds->total == r)) { /* p == 0 only */
      shift = 0;
      prefix = GAMMA_KEY_EMPTY - 1;
      return;
    }
    prefix |= (uint64_t)lds->bin << sh;
    r -= lds->before;
    shift = sh;
    if (lds->count == 1) return;
  }
}

/* GammaDeepSelector: GammaSelector's protocol (init / push / maybe_flush /
 * finish, all threads together, exact u64 keys, a key is dropped only when
 * it is >= the current k-th key) with its state in global memory.
 *   buf    LDS append buffer, GAMMA_SORT_CAP keys, filled through one LDS
 *          atomic like GammaSelector's
 *   region GAMMA_DEEP_REGION(k) keys of global memory that only this
 *          workgroup touches, so workgroup barriers order every access
 *   rn     keys in the region (uniform scalar), thresh in a register
 * flush: buf is appended to the region with coalesced stores, no sort.
 * When the region cannot take another full buf it is compacted in place:
 * gamma_radix_kth finds the k-th key, a ballot / prefix stream compaction
 * keeps the k keys <= it, in tiles of one key per thread, and thresh
 * becomes that key. The region stays unsorted. finish leaves exactly k keys
 * in region[0, k), EMPTY behind the real ones.
 * A tile reads its keys before the barrier and writes them behind it, at
 * positions below the tile's own end, so the in-place move never overwrites
 * a key that is still to be read.
 * Invariant on entry of flush_: rn + GAMMA_SORT_CAP <= R. It holds after
 * init (R = 4 k > 2048) and after a compaction (3 k > 2048). */
struct GammaDeepSelector {
  uint64_t *buf;
  GammaRadixLds *lds;
  int *state;
  uint64_t *region;
  int k, rn;
  uint64_t thresh;

  __device__ void init(uint64_t *buf_, GammaRadixLds *lds_, int *state_,
                       uint64_t *region_, int k_) {
    buf = buf_; lds = lds_; state = state_; region = region_; k = k_;
    rn = 0;
    thresh = GAMMA_KEY_EMPTY;
    if (threadIdx.x == 0) state[0] = 0;
    __syncthreads();
  }

  __device__ __forceinline__ void push(uint64_t key) {
    if (key < thresh) {
      int idx = atomicAdd(&state[0], 1);
      buf[idx] = key; /* in range by the maybe_flush invariant */
    }
  }

  __device__ __forceinline__ void maybe_flush(int margin) {
    __syncthreads();
    if (state[0] > GAMMA_SORT_CAP - margin) flush_();
  }

  __device__ void finish() {
    __syncthreads();
    flush_();
    if (rn > k) compact_();
    for (int i = rn + threadIdx.x; i < k; i += blockDim.x)
      region[i] = GAMMA_KEY_EMPTY;
    __syncthreads();
  }

 private:
  __device__ void flush_() {
    int total = state[0];
    if (total > GAMMA_SORT_CAP) total = GAMMA_SORT_CAP; /* belt & braces */
    total = __builtin_amdgcn_readfirstlane(total);
    for (int i = threadIdx.x; i < total; i += blockDim.x)
      region[rn + i] = buf[i];
    rn += total;
    __syncthreads();
    if (threadIdx.x == 0) state[0] = 0;
    if (rn + GAMMA_SORT_CAP > (int)GAMMA_DEEP_REGION(k)) compact_();
    __syncthreads();
  }

  /* rn > k on entry; k keys and thresh = the k-th on exit */
  __device__ void compact_() {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = (nt + 63) >> 6;
    int shift;
    uint64_t prefix;
    const uint64_t *rd = region;
    gamma_radix_kth([&](int i) { return rd[i]; }, rn, k, lds, shift, prefix);
    const uint64_t top = prefix >> shift;
    int cnt = 0, slot = 0;
    for (int base = 0; base < rn; base += nt, slot ^= 1) {
      const int i = base + tid;
      const uint64_t key = i < rn ? region[i] : GAMMA_KEY_EMPTY;
      const bool keep = i < rn && (key >> shift) <= top;
      if (keep && (key >> shift) == top) lds->pivot = key;
      const uint64_t m = __ballot(keep);
      if (lane == 0) lds->wcnt[slot][wave] = (uint32_t)__popcll(m);
      __syncthreads();
      int before = 0, all = 0;
      for (int w = 0; w < nw; w++) {
        const int c = (int)lds->wcnt[slot][w];
        before += w < wave ? c : 0;
        all += c;
      }
      if (keep)
        region[cnt + before + __popcll(m & ((1ull << lane) - 1ull))] = key;
      cnt += all;
    }
    __syncthreads();
    rn = __builtin_amdgcn_readfirstlane(cnt);
    thresh = lds->pivot;
  }
};

/* delete-bitmap test (1 = deleted), u32 words; null bitmap = none */
__device__ __forceinline__ bool gamma_bitmap_test(const uint32_t *bm,
                                                  uint64_t id) {
  return bm && ((bm[id >> 5] >> (id & 31)) & 1u);
}

/* ------------------------------------------------------------------------
 * Scale note: on the BIG ADC scan (10M codes, 275k candidates/query)
 * this wave selector validates bit-exact but runs 38-50% SLOWER than the
 * block selector (13.6-17.1 ms vs 9.1-9.8 ms, tools/adc_bench.hip): the
 * 64-lane bitonic flush does 8 elems/lane over 45 substages and fires
 * ~4x as often (cap 312 vs 1848). It wins where per-query data is SMALL
 * (k_select_from_dots_wave: top-nprobe of nlist=4096 coarse distances,
 * ~k2*ln(n/k2) pushes => ~1 flush total) because it drops every block
 * barrier and packs 8 queries per workgroup.
 *
 * Wave-local exact top-k selector: one 64-lane wave owns a private LDS
 * region, so the scan needs NO cross-wave barriers (a wave is lockstep;
 * __builtin_amdgcn_wave_barrier() pins the compiler's DS ordering at
 * phase boundaries). The block merges the per-wave results once at the
 * end.
 * Region layout per wave (buf = uint64_t[GAMMA_WSEL_CAP], pow2):
 *   [0, k)            running top-k, sorted ascending after a flush
 *   [k, GAMMA_WSEL_CAP) append region (cap = GAMMA_WSEL_CAP - k slots)
 * flush sorts [0, k+total) in place (res already in front — no copies,
 * no overlap) and re-tightens the threshold.
 * Invariant: maybe_flush(margin) runs at least every `margin`
 * wave-pushes and k + margin <= GAMMA_WSEL_CAP. */
#define GAMMA_WSEL_CAP 512

struct GammaWaveSelector {
  uint64_t *buf; /* uint64_t[GAMMA_WSEL_CAP] in LDS, per wave */
  int *cnt;      /* int[1] in LDS, per wave */
  int k, cap;
  uint64_t thresh;

  __device__ void init(uint64_t *buf_, int *cnt_, int k_) {
    buf = buf_; cnt = cnt_; k = k_;
    cap = GAMMA_WSEL_CAP - k;
    thresh = GAMMA_KEY_EMPTY;
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < k; i += 64) buf[i] = GAMMA_KEY_EMPTY;
    if (lane == 0) *cnt = 0;
    __builtin_amdgcn_wave_barrier();
  }

  /* Admit only keys <= tau from here on. The caller guarantees that at
   * least k of the keys it is about to push are <= tau, so the k-th
   * smallest is among the admitted. Only ever tightens (a seeded
   * selector keeps its own threshold where that is lower), so push /
   * maybe_flush / finish keep their invariants. tau = EMPTY: no bound
   * (and tau + 1 would wrap). */
  __device__ __forceinline__ void prime(uint64_t tau) {
    if (tau != GAMMA_KEY_EMPTY && tau + 1 < thresh) thresh = tau + 1;
  }

  __device__ __forceinline__ void push(uint64_t key) {
    if (key < thresh) {
      int idx = atomicAdd(cnt, 1);
      buf[k + idx] = key; /* in range by the maybe_flush invariant */
    }
  }

  __device__ __forceinline__ void maybe_flush(int margin) {
    __builtin_amdgcn_wave_barrier();
    if (*cnt > cap - margin) flush_();
  }

  __device__ void finish() {
    __builtin_amdgcn_wave_barrier();
    flush_();
  }

  /* wave-level bitonic sort of [0, k+total): lockstep lanes,
   * wave_barrier pins DS ordering between stages */
  __device__ void flush_() {
    const int lane = threadIdx.x & 63;
    int total = *cnt;
    if (total > cap) total = cap;
    int n = 1;
    while (n < k + total) n <<= 1; /* n <= GAMMA_WSEL_CAP (pow2) */
    __builtin_amdgcn_wave_barrier();
    for (int i = k + total + lane; i < n; i += 64)
      buf[i] = GAMMA_KEY_EMPTY;
    __builtin_amdgcn_wave_barrier();
    for (int len = 2; len <= n; len <<= 1) {
      for (int inc = len >> 1; inc > 0; inc >>= 1) {
        for (int i = lane; i < n; i += 64) {
          int j = i ^ inc;
          if (j > i) {
            bool up = (i & len) == 0;
            uint64_t a = buf[i], b = buf[j];
            if ((a > b) == up) { buf[i] = b; buf[j] = a; }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (lane == 0) *cnt = 0;
    __builtin_amdgcn_wave_barrier();
    /* min: a flush with fewer than k keys so far (buf[k-1] still EMPTY)
     * must not lift a primed threshold; unprimed, buf[k-1] never rises */
    thresh = min(thresh, buf[k - 1]);
  }
};

__device__ __forceinline__ uint64_t gamma_readlane_u64(uint64_t v, int j) {
  uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
  uint32_t hi =
      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

/* The kth smallest (kth >= 1) of the 64 * R keys the lanes of a wave hold
 * in m[0..R): each lane ranks its own keys against every lane's (a
 * readlane loop, 64 * R * R compares per lane: no LDS, no sort) and the
 * holder of rank kth - 1 broadcasts. Real keys are distinct (ids are), so
 * that holder is unique; EMPTY entries tie with each other above every
 * real key, and when fewer than kth keys are real the answer is EMPTY.
 * All 64 lanes must call this together. */
template <int R>
__device__ __forceinline__ uint64_t gamma_wave_kth_key(const uint64_t (&m)[4],
                                                       int kth) {
  int rank[R];
#pragma unroll
  for (int s = 0; s < R; s++) rank[s] = 0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    for (int j = 0; j < 64; j++) {
      const uint64_t o = gamma_readlane_u64(m[r], j);
#pragma unroll
      for (int s = 0; s < R; s++) rank[s] += (o < m[s]) ? 1 : 0;
    }
  }
  uint64_t mine = GAMMA_KEY_EMPTY;
#pragma unroll
  for (int s = 0; s < R; s++)
    if (rank[s] == kth - 1) mine = m[s];
  const uint64_t has = __ballot(mine != GAMMA_KEY_EMPTY);
  if (has == 0) return GAMMA_KEY_EMPTY;
  return gamma_readlane_u64(mine, __builtin_ctzll(has));
}
