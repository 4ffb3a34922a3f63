// The postprocessor of `--prepr p...` blocks on the GPU: the grammar's expansion of a precompressed block.
// Replaces Postprocessor::uncompress (preprocessors/Postprocessor.cpp:62-133); the grammar and its expansion table
// stay host code (prepr_host.cpp: buildExpansionTable).  The mirror of k_pr_emit: a token's length is a table
// look-up, its place a prefix sum, its bytes a copy.
//
//   k_pp_heads / k_pr_head_scan   (only when the grammar has special symbols)  where the run of special bytes that
//                  reaches into a tile starts: byte i starts a token unless it is the second byte of a pair, and that
//                  depends only on the parity of the run of special bytes that ends at i - 1.
//   k_pp_count     the tokens' lengths summed per tile (and, 64 bits wide, over the block: the ONE word the host reads)
//   exclusive_scan_u32   the tiles' offsets (the total fits the output, so it fits 32 bits, or the call has returned)
//   k_pp_write     a workgroup owns a tile of input: its tokens' offsets and pool addresses go to LDS (a workgroup
//                  scan), then it produces its output range in pieces of 256 lanes x 16 bytes.  A lane owns one
//                  16-byte aligned group of the OUTPUT, finds the token that covers the group's first byte by a
//                  search of the tile's offsets and gathers from the pool from there on: a token that covers many
//                  groups is copied group by group, and no thread ever loops over an expansion.  Groups leave as one
//                  aligned 16-byte store; the two ragged ends of a tile's range leave as byte stores.
// The table (0.5 MB) and the pool are read-only and small: they stay in the L2.
#include "bwt_engine.hpp"
#include "postprocess.hpp"

#include <cstring>
#include <vector>

namespace bwtc_hip {

constexpr int kPpTPB = 256;
constexpr u32 kPpPer = 16;                       // positions per thread
constexpr u32 kPpTile = kPpTPB * kPpPer;         // 4096 positions per tile
constexpr u32 kPpKeys = bwtc::prepr::kExpansionKeys;
constexpr u32 kPpTabWords = 2 * kPpKeys + 8;     // (offset, length) per key, then the 256 special flags

// the thread's bytes d[j0 .. j0 + 16] (zero behind the data) -> c[0 .. 16]
__device__ __forceinline__ void pp_load(const u8* __restrict__ d, u64 n, u64 j0, u32 (&c)[kPpPer + 1]) {
  if (j0 + kPpPer + 1 <= n && ((reinterpret_cast<uintptr_t>(d) + j0) & 15u) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(d + j0);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (u32 k = 0; k < kPpPer; ++k) c[k] = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    c[kPpPer] = d[j0 + kPpPer];
  } else {
#pragma unroll
    for (u32 k = 0; k <= kPpPer; ++k) c[k] = j0 + k < n ? d[j0 + k] : 0u;
  }
}

__device__ __forceinline__ bool pp_special(const u32* s_sp, u32 c) { return (s_sp[c >> 5] >> (c & 31u)) & 1u; }

// (last position of a byte that is not special) + 1 among the thread's positions, 0 when it has none
__device__ __forceinline__ u32 pp_mark(const u32 (&c)[kPpPer + 1], u64 j0, u64 n, const u32* s_sp) {
  u32 last = 0;
#pragma unroll
  for (u32 k = 0; k < kPpPer; ++k) if (j0 + k < n && !pp_special(s_sp, c[k])) last = (u32)(j0 + k) + 1u;
  return last;
}

__global__ __launch_bounds__(kPpTPB) void k_pp_heads(const u8* __restrict__ d, u64 n, const u32* __restrict__ tab,
                                                     u32* __restrict__ tile_head) {
  __shared__ u32 scr[kPpTPB / kWave + 1];
  __shared__ u32 s_sp[8];
  if (threadIdx.x < 8) s_sp[threadIdx.x] = tab[2 * kPpKeys + threadIdx.x];
  __syncthreads();
  const u64 j0 = (u64)blockIdx.x * kPpTile + (u64)threadIdx.x * kPpPer;
  u32 last = 0;
  if (j0 < n) {
    u32 c[kPpPer + 1];
    pp_load(d, n, j0, c);
    last = pp_mark(c, j0, n, s_sp);
  }
  u32 total;
  (void)block_scan_incl_max<kPpTPB>(last, scr, &total);
  if (threadIdx.x == 0) tile_head[blockIdx.x] = total;
}

// What the thread's sixteen positions stand for: len[k] = bytes of the token that starts at position j0 + k (0: no
// token starts there, or it stands for nothing), src[k] = where they are in the pool.  SPECIAL: the grammar has
// special symbols; the run of special bytes that reaches position j0 - 1 starts at the last mark before j0 -- in
// earlier tiles (tile_head, exclusive maximum) or among the earlier threads of this tile.  Every thread of the
// workgroup must call it (a workgroup scan).
template <bool SPECIAL>
__device__ __forceinline__ void pp_tokens(const u8* __restrict__ d, u64 n, const u32* __restrict__ tab,
                                          const u32* __restrict__ tile_head, const u32* s_sp, u32* scr, u32* s_incl,
                                          u32 (&len)[kPpPer], u32 (&src)[kPpPer], u32* tokens, u32* pairs) {
  const u64 j0 = (u64)blockIdx.x * kPpTile + (u64)threadIdx.x * kPpPer;
  u32 c[kPpPer + 1];
  pp_load(d, n, j0 < n ? j0 : 0, c);
  u32 run = 0;
  if (SPECIAL) {
    const u32 mine = j0 < n ? pp_mark(c, j0, n, s_sp) : 0u;
    u32 total;
    s_incl[threadIdx.x] = block_scan_incl_max<kPpTPB>(mine, scr, &total);
    __syncthreads();
    run = max(tile_head[blockIdx.x], threadIdx.x ? s_incl[threadIdx.x - 1] : 0u);
    __syncthreads();
  }
  u32 nt = 0, np = 0;
#pragma unroll
  for (u32 k = 0; k < kPpPer; ++k) {
    const u64 i = j0 + k;
    len[k] = 0; src[k] = 0;
    if (i >= n) continue;
    const bool special = SPECIAL && pp_special(s_sp, c[k]);
    const bool starts = !SPECIAL || (((u32)i - run) & 1u) == 0;
    if (starts) {
      const bool pair = special && i + 1 < n;                   // a special symbol that is the last byte stands alone
      const u32 key = pair ? 256u + (c[k] << 8 | c[k + 1]) : c[k];
      const uint2 e = *reinterpret_cast<const uint2*>(tab + 2 * key);
      src[k] = e.x; len[k] = e.y;
      ++nt; np += pair;
    }
    if (SPECIAL && !special) run = (u32)i + 1u;
  }
  *tokens = nt; *pairs = np;
}

__device__ __forceinline__ unsigned long long pp_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// tile_count[t] = the bytes tile t stands for (clamped to 32 bits: a block that overflows them does not fit any
// output this route takes); totals[0..2] += bytes, tokens, pair tokens
template <bool SPECIAL>
__global__ __launch_bounds__(kPpTPB) void k_pp_count(const u8* __restrict__ d, u64 n, const u32* __restrict__ tab,
                                                     const u32* __restrict__ tile_head, u32* __restrict__ tile_count,
                                                     unsigned long long* __restrict__ totals) {
  __shared__ u32 scr[kPpTPB / kWave + 1];
  __shared__ u32 s_incl[kPpTPB];
  __shared__ u32 s_sp[8];
  __shared__ unsigned long long s_sum[kPpTPB / kWave][3];
  if (threadIdx.x < 8) s_sp[threadIdx.x] = tab[2 * kPpKeys + threadIdx.x];
  __syncthreads();
  u32 len[kPpPer], src[kPpPer], nt, np;
  pp_tokens<SPECIAL>(d, n, tab, tile_head, s_sp, scr, s_incl, len, src, &nt, &np);
  unsigned long long bytes = 0;
#pragma unroll
  for (u32 k = 0; k < kPpPer; ++k) bytes += len[k];
  bytes = pp_wave_sum(bytes);
  const unsigned long long toks = pp_wave_sum(nt), prs = pp_wave_sum(np);
  if (lane_id() == 0) { s_sum[threadIdx.x / kWave][0] = bytes; s_sum[threadIdx.x / kWave][1] = toks; s_sum[threadIdx.x / kWave][2] = prs; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t[3] = {0, 0, 0};
    for (int w = 0; w < kPpTPB / kWave; ++w) for (int q = 0; q < 3; ++q) t[q] += s_sum[w][q];
    tile_count[blockIdx.x] = t[0] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)t[0];
    for (int q = 0; q < 3; ++q) if (t[q]) atomicAdd(&totals[q], t[q]);
  }
}

template <bool SPECIAL>
__global__ __launch_bounds__(kPpTPB) void k_pp_write(const u8* __restrict__ d, u64 n, const u32* __restrict__ tab,
                                                     const u8* __restrict__ pool, const u32* __restrict__ tile_head,
                                                     const u32* __restrict__ tile_offset, u8* __restrict__ dst) {
  __shared__ u32 scr[kPpTPB / kWave + 1];
  __shared__ u32 s_incl[kPpTPB];
  __shared__ u32 s_sp[8];
  __shared__ u32 s_at[kPpTile + 1];              // tokens that stand for something, in order: offset in the tile's range
  __shared__ u32 s_src[kPpTile];                 // ... and where their bytes are in the pool
  if (threadIdx.x < 8) s_sp[threadIdx.x] = tab[2 * kPpKeys + threadIdx.x];
  __syncthreads();
  u32 len[kPpPer], src[kPpPer], nt, np;
  pp_tokens<SPECIAL>(d, n, tab, tile_head, s_sp, scr, s_incl, len, src, &nt, &np);
  u32 bytes = 0, filled = 0;
#pragma unroll
  for (u32 k = 0; k < kPpPer; ++k) { bytes += len[k]; filled += len[k] != 0; }
  u32 total, ntok;
  u32 at = block_scan_excl_add<kPpTPB>(bytes, scr, &total);
  u32 rank = block_scan_excl_add<kPpTPB>(filled, scr, &ntok);
#pragma unroll
  for (u32 k = 0; k < kPpPer; ++k)
    if (len[k]) { s_at[rank] = at; s_src[rank] = src[k]; ++rank; at += len[k]; }
  if (threadIdx.x == 0) s_at[ntok] = total;
  __syncthreads();
  if (total == 0) return;
  u8* out = dst + tile_offset[blockIdx.x];
  const u32 lead = (u32)(reinterpret_cast<uintptr_t>(out) & 15u);   // bytes of the first group that belong to the tile before
  const u64 groups = ((u64)lead + total + 15u) >> 4;
  for (u64 g = threadIdx.x; g < groups; g += kPpTPB) {
    const long long x0 = (long long)(g << 4) - (long long)lead;     // the group is the range's bytes [x0, x0 + 16)
    const u32 lo = x0 < 0 ? 0u : (u32)x0;
    const u32 hi = (u64)(x0 + 16) > (u64)total ? total : (u32)(x0 + 16);
    u32 a = 0, b = ntok;                          // the last token with s_at <= lo: it covers lo
    while (b - a > 1) { const u32 mid = (a + b) >> 1; if (s_at[mid] <= lo) a = mid; else b = mid; }
    u32 tok_at = s_at[a], tok_end = s_at[a + 1], tok_src = s_src[a];
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (u32 q = 0; q < 16; ++q) {
      const long long x = x0 + q;
      if (x < (long long)lo || x >= (long long)hi) continue;
      if ((u32)x >= tok_end) { ++a; tok_at = tok_end; tok_end = s_at[a + 1]; tok_src = s_src[a]; }
      w[q >> 2] |= (u32)pool[tok_src + ((u32)x - tok_at)] << (8 * (q & 3));
    }
    if (hi - lo == 16) {
      *reinterpret_cast<uint4*>(out + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (u32 q = 0; q < 16; ++q) {
        const long long x = x0 + q;
        if (x >= (long long)lo && x < (long long)hi) out[x] = (u8)(w[q >> 2] >> (8 * (q & 3)));
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------
#define PP_TRY(expr)                                              \
  do {                                                            \
    hipError_t e_ = (expr);                                       \
    if (e_ != hipSuccess) { (void)hipGetLastError(); return e_ == hipErrorOutOfMemory ? -2 : -3; } \
  } while (0)

struct PostProcessor {
  u32* d_tab = nullptr;                          // kPpTabWords
  u8* d_pool = nullptr;          u64 pool_cap = 0;
  u32* d_head = nullptr;         u64 tile_cap = 0;       // per-tile words: run starts, counts / offsets, scan partials
  u32* d_count = nullptr;
  u32* d_partial = nullptr;
  unsigned long long* d_totals = nullptr;        // bytes, tokens, pair tokens
  unsigned long long* h_totals = nullptr;        // pinned
  u8* d_in = nullptr;            u64 in_cap = 0;         // staging of postprocess_block
  u8* d_outb = nullptr;          u64 out_cap = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bwtc_hip_postprocess_stats stats;
};

PostProcessor* postprocessor_create() {
  PostProcessor* p = new (std::nothrow) PostProcessor();
  if (p) std::memset(&p->stats, 0, sizeof p->stats);
  return p;
}
void postprocessor_destroy(PostProcessor* p) {
  if (!p) return;
  (void)hipFree(p->d_tab); (void)hipFree(p->d_pool); (void)hipFree(p->d_head); (void)hipFree(p->d_count);
  (void)hipFree(p->d_partial); (void)hipFree(p->d_totals); (void)hipFree(p->d_in); (void)hipFree(p->d_outb);
  if (p->h_totals) (void)hipHostFree(p->h_totals);
  for (int i = 0; i < 4; ++i) if (p->ev[i]) (void)hipEventDestroy(p->ev[i]);
  delete p;
}
int postprocessor_stats(PostProcessor* p, bwtc_hip_postprocess_stats* out) {
  if (!p) { std::memset(out, 0, sizeof *out); return 0; }
  *out = p->stats;
  return 0;
}

template <typename T>
static int pp_grow(T** ptr, u64* cap, u64 need) {
  if (need <= *cap && *ptr) return 0;
  if (*ptr) { (void)hipFree(*ptr); *ptr = nullptr; *cap = 0; }
  const u64 want = need + need / 4 + 64;
  PP_TRY(hipMalloc(reinterpret_cast<void**>(ptr), want * sizeof(T)));
  *cap = want;
  return 0;
}
static void pp_workspace(PostProcessor& p) {
  p.stats.workspace_bytes = (p.d_tab ? (u64)kPpTabWords * 4 : 0) + p.pool_cap + (p.d_head ? p.tile_cap * 4 * 2 + (p.tile_cap / kScanTile + 1) * 4 : 0) +
                            (p.d_totals ? 24 : 0) + p.in_cap + p.out_cap;
}
static int pp_init(PostProcessor& p) {
  if (p.d_tab) return 0;
  for (int i = 0; i < 4; ++i) if (!p.ev[i]) PP_TRY(hipEventCreate(&p.ev[i]));
  if (!p.d_totals) PP_TRY(hipMalloc(reinterpret_cast<void**>(&p.d_totals), 3 * sizeof(unsigned long long)));
  if (!p.h_totals) PP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p.h_totals), 3 * sizeof(unsigned long long)));
  PP_TRY(hipMalloc(reinterpret_cast<void**>(&p.d_tab), (u64)kPpTabWords * 4));
  return 0;
}

// blocks the device passes do not take (their 32-bit positions and offsets): the host function, same bytes
static int pp_host_route(BwtEngine& e, PostProcessor& p, const bwtc::prepr::Grammar& g, const u8* d_data, u64 n, u8* d_out, u64 cap,
                         u64* n_out) {
  std::vector<u8> in(n), out;
  if (n) PP_TRY(hipMemcpy(in.data(), d_data, n, hipMemcpyDeviceToHost));
  if (!bwtc::prepr::postprocess(g, in.data(), n, &out, cap)) return -1;
  if (!out.empty()) PP_TRY(hipMemcpy(d_out, out.data(), out.size(), hipMemcpyHostToDevice));
  p.stats.route = 2;
  p.stats.out_bytes = out.size();
  *n_out = out.size();
  return 0;
}

// The passes up to the one host read: *total = the bytes the block stands for.  The write pass follows with the
// same table, run starts and offsets (pp_write).
static int pp_count(BwtEngine& e, PostProcessor& p, const bwtc::prepr::ExpansionTable& t, const u8* d_data, u64 n, u64* total) {
  hipStream_t st = e.stream;
  const u32 ntiles = (u32)((n + kPpTile - 1) / kPpTile);
  int rc = pp_grow(&p.d_pool, &p.pool_cap, t.pool.size());
  if (rc) return rc;
  if ((u64)ntiles > p.tile_cap || !p.d_head) {
    (void)hipFree(p.d_head); (void)hipFree(p.d_count); (void)hipFree(p.d_partial);
    p.d_head = p.d_count = p.d_partial = nullptr;
    p.tile_cap = 0;
    const u64 want = (u64)ntiles + ntiles / 4 + 64;
    PP_TRY(hipMalloc(reinterpret_cast<void**>(&p.d_head), want * 4));
    PP_TRY(hipMalloc(reinterpret_cast<void**>(&p.d_count), want * 4));
    PP_TRY(hipMalloc(reinterpret_cast<void**>(&p.d_partial), (want / kScanTile + 1) * 4));
    p.tile_cap = want;
  }
  pp_workspace(p);
  PP_TRY(hipMemcpyAsync(p.d_tab, t.entry.data(), (u64)2 * kPpKeys * 4, hipMemcpyHostToDevice, st));
  PP_TRY(hipMemcpyAsync(p.d_tab + 2 * kPpKeys, t.special, 32, hipMemcpyHostToDevice, st));
  PP_TRY(hipMemcpyAsync(p.d_pool, t.pool.data(), t.pool.size(), hipMemcpyHostToDevice, st));
  PP_TRY(hipMemsetAsync(p.d_totals, 0, 24, st));
  PP_TRY(hipEventRecord(p.ev[0], st));
  if (t.any_special) {
    hipLaunchKernelGGL(k_pp_heads, dim3(ntiles), dim3(kPpTPB), 0, st, d_data, n, (const u32*)p.d_tab, p.d_head);
    hipLaunchKernelGGL(k_pr_head_scan, dim3(1), dim3(1024), 0, st, p.d_head, ntiles);
    hipLaunchKernelGGL((k_pp_count<true>), dim3(ntiles), dim3(kPpTPB), 0, st, d_data, n, (const u32*)p.d_tab, (const u32*)p.d_head, p.d_count,
                       p.d_totals);
    p.stats.launches += 3;
  } else {
    hipLaunchKernelGGL((k_pp_count<false>), dim3(ntiles), dim3(kPpTPB), 0, st, d_data, n, (const u32*)p.d_tab, (const u32*)nullptr, p.d_count,
                       p.d_totals);
    p.stats.launches += 1;
  }
  // three-launch form or one workgroup: this stream's scans take no tickets of the transform's chain
  ScanChain* const chain = current_scan_chain();
  current_scan_chain() = nullptr;
  exclusive_scan_u32(p.d_count, ntiles, p.d_partial, st);
  current_scan_chain() = chain;
  p.stats.launches += ntiles <= (u32)kScanTile ? 1 : (ceil_div(ntiles, kScanTile) <= kScanRawTiles ? 2 : 3);
  PP_TRY(hipEventRecord(p.ev[1], st));
  PP_TRY(hipMemcpyAsync(p.h_totals, p.d_totals, 24, hipMemcpyDeviceToHost, st));
  PP_TRY(e.wait());
  PP_TRY(hipGetLastError());
  *total = p.h_totals[0];
  p.stats.tokens = p.h_totals[1];
  p.stats.pair_tokens = p.h_totals[2];
  return 0;
}

static int pp_write(BwtEngine& e, PostProcessor& p, const bwtc::prepr::ExpansionTable& t, const u8* d_data, u64 n, u8* d_out) {
  hipStream_t st = e.stream;
  const u32 ntiles = (u32)((n + kPpTile - 1) / kPpTile);
  PP_TRY(hipEventRecord(p.ev[2], st));
  if (t.any_special)
    hipLaunchKernelGGL((k_pp_write<true>), dim3(ntiles), dim3(kPpTPB), 0, st, d_data, n, (const u32*)p.d_tab, (const u8*)p.d_pool,
                       (const u32*)p.d_head, (const u32*)p.d_count, d_out);
  else
    hipLaunchKernelGGL((k_pp_write<false>), dim3(ntiles), dim3(kPpTPB), 0, st, d_data, n, (const u32*)p.d_tab, (const u8*)p.d_pool,
                       (const u32*)nullptr, (const u32*)p.d_count, d_out);
  p.stats.launches += 1;
  PP_TRY(hipEventRecord(p.ev[3], st));
  PP_TRY(e.wait());
  PP_TRY(hipGetLastError());
  float a = 0.f, b = 0.f;
  (void)hipEventElapsedTime(&a, p.ev[0], p.ev[1]);
  (void)hipEventElapsedTime(&b, p.ev[2], p.ev[3]);
  p.stats.ms_device = a + b;
  return 0;
}

static bool pp_device_takes(u64 n, u64 cap) { return n < (1ull << 31) && cap < (1ull << 32); }

static void pp_begin(PostProcessor& p, u64 n) {
  const u64 ws = p.stats.workspace_bytes;
  std::memset(&p.stats, 0, sizeof p.stats);
  p.stats.workspace_bytes = ws;
  p.stats.in_bytes = n;
}

int postprocess_device(BwtEngine& e, PostProcessor& p, const bwtc::prepr::Grammar& g, const u8* d_data, u64 n, u8* d_out, u64 cap,
                       u64* n_out) {
  PP_TRY(hipSetDevice(e.device));
  pp_begin(p, n);
  if (g.numberOfRules() == 0) {                                    // Postprocessor.cpp:114-117: the block as it is
    if (n > cap) return -1;
    if (n) PP_TRY(hipMemcpyAsync(d_out, d_data, n, hipMemcpyDeviceToDevice, e.stream));
    PP_TRY(e.wait());
    p.stats.route = 1; p.stats.tokens = n; p.stats.out_bytes = n;
    *n_out = n;
    return 0;
  }
  if (!pp_device_takes(n, cap)) return pp_host_route(e, p, g, d_data, n, d_out, cap, n_out);
  bwtc::prepr::ExpansionTable t;
  if (!bwtc::prepr::buildExpansionTable(g, cap, &t)) return -1;
  p.stats.pool_bytes = t.pool.size();
  u64 total = 0;
  if (n) {
    int rc = pp_init(p);
    if (rc == 0) rc = pp_count(e, p, t, d_data, n, &total);
    if (rc) return rc;
    if (total > cap) return -1;                                    // nothing has been written to d_out
    if (total) { rc = pp_write(e, p, t, d_data, n, d_out); if (rc) return rc; }
  }
  p.stats.route = 1;
  p.stats.out_bytes = total;
  *n_out = total;
  return 0;
}

int postprocess_block(BwtEngine& e, PostProcessor& p, const bwtc::prepr::Grammar& g, const u8* data, u64 n, u8* out, u64 cap, u64* n_out) {
  PP_TRY(hipSetDevice(e.device));
  pp_begin(p, n);
  if (g.numberOfRules() == 0) {                                    // Postprocessor.cpp:114-117: the block as it is, by way of the device
    if (n > cap) return -1;
    if (n) {
      const int rc = pp_grow(&p.d_in, &p.in_cap, n);
      if (rc) return rc;
      pp_workspace(p);
      PP_TRY(hipMemcpy(p.d_in, data, n, hipMemcpyHostToDevice));
      PP_TRY(hipMemcpy(out, p.d_in, n, hipMemcpyDeviceToHost));
    }
    p.stats.route = 1; p.stats.tokens = n; p.stats.out_bytes = n;
    *n_out = n;
    return 0;
  }
  if (!pp_device_takes(n, cap)) {                                  // a block beyond the device route: the host function
    std::vector<u8> v;
    if (!bwtc::prepr::postprocess(g, data, n, &v, cap)) return -1;
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    p.stats.route = 2; p.stats.out_bytes = v.size();
    *n_out = v.size();
    return 0;
  }
  bwtc::prepr::ExpansionTable t;
  if (!bwtc::prepr::buildExpansionTable(g, cap, &t)) return -1;
  p.stats.pool_bytes = t.pool.size();
  u64 total = 0;
  if (n) {
    int rc = pp_init(p);
    if (rc == 0) rc = pp_grow(&p.d_in, &p.in_cap, n);
    if (rc) return rc;
    PP_TRY(hipMemcpyAsync(p.d_in, data, n, hipMemcpyHostToDevice, e.stream));
    rc = pp_count(e, p, t, p.d_in, n, &total);
    if (rc) return rc;
    if (total > cap) return -1;                                    // nothing has been written to out
    if (total) {
      rc = pp_grow(&p.d_outb, &p.out_cap, total);
      if (rc) return rc;
      pp_workspace(p);
      rc = pp_write(e, p, t, p.d_in, n, p.d_outb);
      if (rc) return rc;
      PP_TRY(hipMemcpy(out, p.d_outb, total, hipMemcpyDeviceToHost));
    }
  }
  p.stats.route = 1;
  p.stats.out_bytes = total;
  *n_out = total;
  return 0;
}

}  // namespace bwtc_hip
