/*
 * scan_walk.hpp — the chunked probe walk shared by the fused IVF scan
 * kernels (k_ivfpq_scan's fast path, k_ivfpq_scan_wide, k_binivf_scan,
 * k_rabitq_scan). Included by kernels.hip behind select.hpp and kernels.h,
 * in front of ivfpq_scan_kernels.hpp, binary_kernels.hpp and
 * rabitq_kernels.hpp.
 *
 * A workgroup walks its probe subsequence in chunks of at most
 * GAMMA_SCAN_PCH lists. Per chunk: one thread per probe stores the list's
 * descriptor (gamma_chunk_put), gamma_chunk_close turns the sizes into one
 * flat index space, and a GammaListCursor maps flat indices back to (list,
 * entry). The prefetching pass loop over that space stays in each kernel
 * (k_ivfpq_scan has the reasoning): written as a shared function template
 * it came out 1-2 % slower in k_binivf_scan and k_rabitq_scan.
 * DESIGN.md "The chunked probe walk" has the overview.
 */
#pragma once

/* The lists of a chunk form ONE flat index space [0, total): off[i] is the
 * exclusive prefix sum of the list sizes, so entry g belongs to the list i
 * with off[i] <= g < off[i+1]. Invalid probes and empty lists have size 0
 * and drop out. The stream pointers carry the global address space, which
 * makes every list load a global_load (vmcnt only) — a generic pointer
 * would load with flat_load, which also ticks lgkmcnt and would make each
 * wait of the LDS gather drain the prefetch. */
#define GAMMA_SCAN_PCH 32
typedef const __attribute__((address_space(1))) uint32_t *gamma_gu32p;
typedef const __attribute__((address_space(1))) uint8_t *gamma_gu8p;
typedef const __attribute__((address_space(1))) float *gamma_gf32p;
template <class Per> /* Per: the kernel's own per-list scalars */
struct GammaChunkT {
  gamma_gu32p ids[GAMMA_SCAN_PCH];
  gamma_gu8p codes[GAMMA_SCAN_PCH];
  gamma_gf32p svals[GAMMA_SCAN_PCH];
  Per per;
  int sz[GAMMA_SCAN_PCH];
  int off[GAMMA_SCAN_PCH + 1];
  int ncons;    /* probes of the chunk whose flat space fits 31 bits */
  int kill[2];  /* the kill flag as thread 0 last read it, per parity */
  int state[2]; /* selector append counter */
};
struct GammaPqPer {
  float dis0[GAMMA_SCAN_PCH];
};
typedef GammaChunkT<GammaPqPer> GammaScanChunk;
/* part of k_ivfpq_scan's LDS total, which decides the M at which a table
 * moves to the sliced kernel (gk::ivfpq_scan_is_wide) */
static_assert(sizeof(GammaScanChunk) == 1176, "changes the kernel switch");

/* acc = fmaf(a[t], b[t], acc) for ascending t from 0: the canonical dot
 * chain of the oracle. Bit-exactness of every IP table entry and of
 * dis0 = dot(q, c) rests on this order. */
__device__ __forceinline__ float gamma_dot_serial(const float *a,
                                                  const float *b, int n) {
  float acc = 0.0f;
  for (int t = 0; t < n; t++) acc = fmaf(a[t], b[t], acc);
  return acc;
}

/* what an invalid probe stores: no entries */
__device__ __forceinline__ GammaBucketDev gamma_null_bucket() {
  GammaBucketDev bk;
  bk.ids = nullptr; bk.data = nullptr; bk.svals = nullptr;
  bk.size = 0;
  return bk;
}

/* store one probe's descriptor into slot `slot`; returns the list size as
 * the walk sees it. The kernel's own per-list fields (dis0, qc2, ...) are
 * the caller's to store. SV = false leaves svals out (no S term stream). */
template <bool SV = true, class Chunk>
__device__ __forceinline__ int gamma_chunk_put(Chunk *ch, int slot,
                                               const GammaBucketDev &bk) {
  long long sz = bk.size < 0 ? 0 : bk.size;
  if (sz > 0x7fffffffll) sz = 0x7fffffffll; /* ids are 31-bit */
  ch->ids[slot] = (gamma_gu32p)bk.ids;
  ch->codes[slot] = (gamma_gu8p)bk.data;
  if (SV) ch->svals[slot] = (gamma_gf32p)bk.svals;
  ch->sz[slot] = (int)sz;
  return (int)sz;
}

struct GammaChunkSpan {
  bool killed;    /* the kill flag was up: total is 0, leave the walk */
  int ncons;      /* probes the chunk consumed (>= 1) */
  unsigned total; /* entries in its flat space */
};

/* Close a chunk of `cn` stored descriptors: prefix sums into off[], cut to
 * a 31-bit flat space. All threads call it; two barriers inside. VOTE: the
 * first barrier also ORs *vote over the block and leaves the result there.
 *
 * In-flight kill (is_killed_every<1024> analog, ivfpq.h:927): agent-scope
 * load (L2-served, so a host write during the kernel is visible — plain
 * loads can stay L1-stale). ONE thread polls and the block reads its answer
 * from LDS behind a barrier, so every thread takes the same exit. */
template <bool VOTE = false, class Chunk>
__device__ __forceinline__ GammaChunkSpan
gamma_chunk_close(Chunk *ch, int cn, const int *kill_flag,
                  int *vote = nullptr) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    ch->kill[0] = kill_flag
                      ? __hip_atomic_load(kill_flag, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT)
                      : 0;
    ch->ncons = cn;
    ch->off[0] = 0;
  }
  if (VOTE) *vote = __syncthreads_or(*vote);
  else __syncthreads();
  if (tid < cn) {
    long long cum = 0;
    for (int u = 0; u <= tid; u++) cum += ch->sz[u];
    if (cum > 0x7fffffffll) { /* flat space is 31-bit: end the chunk
                                 before this probe (never the first) */
      atomicMin(&ch->ncons, tid);
      cum = 0x7fffffffll;
    }
    ch->off[tid + 1] = (int)cum;
  }
  __syncthreads();
  GammaChunkSpan sp;
  sp.killed = ch->kill[0] != 0;
  sp.ncons = ch->ncons;
  sp.total = sp.killed ? 0u : (unsigned)ch->off[sp.ncons];
  return sp;
}

/* A thread's position in the chunk's flat space: its current list li holds
 * entries [lstart, lend). A thread's flat indices ascend, so the cursor
 * only moves forward. */
struct GammaListCursor {
  int li;
  unsigned lstart, lend, total;

  template <class Chunk>
  __device__ __forceinline__ void reset(const Chunk *ch, unsigned total_) {
    li = 0;
    lstart = 0;
    lend = (unsigned)ch->off[1];
    total = total_;
  }

  /* Map flat index g0 to entry j of list li and return j. When li
   * changes (LDS reads only), reload(li) runs inside the same branch for
   * the caller to refresh its per-list fields.
   * Nothing is read past a list's size: a lane with no entry left
   * (g0 >= total, only at a chunk's end) aliases the chunk's last entry
   * and reports live = false, instead of skipping its loads. */
  template <class Chunk, class Reload>
  __device__ __forceinline__ unsigned seek(const Chunk *ch, unsigned g0,
                                           bool &live, Reload &&reload) {
    live = g0 < total;
    const unsigned g = live ? g0 : total - 1;
    if (g >= lend) {
      do {
        li++;
        lend = (unsigned)ch->off[li + 1];
      } while (g >= lend);
      lstart = (unsigned)ch->off[li];
      reload(li);
    }
    return g - lstart;
  }
};
