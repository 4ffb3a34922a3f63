// Batched block transform: K blocks, one segmented prefix doubling (gfx950, wave64).
//
// The rule (tests/batchmodel.py states it and proves it against sorted()): block b's T_b = reverse(block) + '\0' lies at
// position b * S of one array, S = 2^k the smallest power of two >= max n_b, so the block of position s is s >> k.  The
// initial key is {block id, six characters, min(length, 6)}; after one radix sort every block is a contiguous range of
// slots and rank[s] is the slot of s's group head.  A round at depth h = 6, 12, 24, ... sorts the entries of the tied
// groups by (rank[s], rank[s + h] + 1 -- or 0 where s + h is at or past the end of s's OWN block, decided before the
// read), flags the sub-group heads, scans, writes the new ranks and compacts the singletons out.  The host reads one
// word per round: the entries left.  No long keys, no finisher, no closed-form steps: this sorter is for blocks whose
// cost is launches and host round trips, not bytes.
//
// Bounds: every index that is built from data (a suffix from a list, a slot from a scan, a rank from rank[]) is
// compared with the size of the array it goes into before it is used; a miss raises the error word (-3 on return)
// and stores nothing.
#include "batch_bwt.hpp"
#include <algorithm>
#include <numeric>
#include <vector>

namespace bwtc_hip {

namespace {

struct BatchBlock { u64 offset; u32 n, base, n_lf, pad; };   // n = size + 1 suffixes; base = sum of the earlier blocks' n

constexpr int kBatchTPB = 256;
constexpr u32 kBatchLoadPer = 16;                            // positions per thread of the load pass: one 16-byte store
constexpr u32 kBatchLoadTile = kBatchTPB * kBatchLoadPer;    // 4096 positions per workgroup
constexpr u32 kBatchLdsBlocks = 16;                          // blocks of a workgroup that get an LDS histogram (S >= 256)
constexpr u32 kBatchMaxRounds = 40;

// ---- load: reverse, terminate, count -------------------------------------------------------------------------------
// A workgroup takes 4096 positions of the strided array: a piece of one block (S >= 4096) or 4096 / S whole blocks.
// Blocks of 256 positions and more count their bytes in an LDS histogram of their own, flushed once per block and
// workgroup; smaller ones (fewer bytes than a histogram has bins) add straight to their row in memory.  A thread's 16
// positions are one aligned 16-byte store, and one 16-byte load where the 16 source bytes lie inside the block at an
// aligned address; the bytes behind a block's terminator up to the 16-byte boundary are written as zeros (they are
// padding of the block's own stride and nobody reads them).
__global__ __launch_bounds__(kBatchTPB) void k_batch_load(const u8* __restrict__ src, u8* __restrict__ T,
                                                          const BatchBlock* __restrict__ blocks, u32 K, u32 kk,
                                                          u32* __restrict__ counts) {
  __shared__ u32 hist[kBatchLdsBlocks * 256];
  const u64 S = 1ull << kk;
  const u64 tile0 = (u64)blockIdx.x * kBatchLoadTile;
  const u32 b_first = (u32)(tile0 >> kk);
  const u32 nblk = S >= kBatchLoadTile ? 1u : (u32)(kBatchLoadTile >> kk);
  const bool lds = S >= 256;                                 // then nblk <= kBatchLdsBlocks
  if (lds) {
    for (u32 i = threadIdx.x; i < nblk * 256u; i += kBatchTPB) hist[i] = 0;
    __syncthreads();
  }
  const u64 s0 = tile0 + (u64)threadIdx.x * kBatchLoadPer;
  if (S >= kBatchLoadPer) {                                  // the 16 positions lie in one block
    const u32 b = (u32)(s0 >> kk);
    if (b < K) {
      const u32 i0 = (u32)(s0 & (S - 1));
      const u32 n = blocks[b].n, size = n - 1u;
      if (i0 < n) {
        const u8* blk = src + blocks[b].offset;
        u32 w[4] = {0, 0, 0, 0};
        const bool whole = i0 + kBatchLoadPer <= size;
        const u8* from = blk + (size - i0 - (whole ? kBatchLoadPer : 0u));   // (whole: the 16 source bytes start here)
        if (whole && (reinterpret_cast<uintptr_t>(from) & 15u) == 0) {
          const uint4 q = *reinterpret_cast<const uint4*>(from);
          w[0] = __builtin_bswap32(q.w); w[1] = __builtin_bswap32(q.z);
          w[2] = __builtin_bswap32(q.y); w[3] = __builtin_bswap32(q.x);
        } else {
#pragma unroll
          for (u32 j = 0; j < kBatchLoadPer; ++j) {
            const u32 i = i0 + j;
            const u32 c = i < size ? (u32)blk[size - 1u - i] : 0u;
            w[j >> 2] |= c << (8u * (j & 3u));
          }
        }
        *reinterpret_cast<uint4*>(T + s0) = make_uint4(w[0], w[1], w[2], w[3]);
        if (lds) {
          u32* row = &hist[(b - b_first) * 256u];
#pragma unroll
          for (u32 j = 0; j < kBatchLoadPer; ++j)
            if (i0 + j < size) atomicAdd(&row[(w[j >> 2] >> (8u * (j & 3u))) & 255u], 1u);
        } else {
          u32* row = counts + (u64)b * 256u;
          for (u32 j = 0; j < kBatchLoadPer; ++j)
            if (i0 + j < size) atomicAdd(&row[(w[j >> 2] >> (8u * (j & 3u))) & 255u], 1u);
        }
      }
    }
  } else {                                                   // strides of 2, 4 and 8 positions: byte by byte
    for (u32 j = 0; j < kBatchLoadPer; ++j) {
      const u64 s = s0 + j;
      const u32 b = (u32)(s >> kk);
      if (b >= K) break;
      const u32 i = (u32)(s & (S - 1));
      const u32 n = blocks[b].n, size = n - 1u;
      if (i >= n) continue;
      const u32 c = i < size ? (u32)src[blocks[b].offset + (size - 1u - i)] : 0u;
      T[s] = (u8)c;
      if (i < size) atomicAdd(&counts[(u64)b * 256u + c], 1u);
    }
  }
  if (lds) {
    __syncthreads();
    for (u32 i = threadIdx.x; i < nblk * 256u; i += kBatchTPB) {
      const u32 v = hist[i], b = b_first + (i >> 8);
      if (v && b < K) atomicAdd(&counts[(u64)b * 256u + (i & 255u)], v);
    }
  }
}

// ---- initial keys: block id (12) | six characters, zeros at and past n_b (48) | min(n_b - i, 6) (3) -----------------
__global__ __launch_bounds__(kBatchTPB) void k_batch_keys(const u8* __restrict__ T, const BatchBlock* __restrict__ blocks,
                                                          u32 K, u32 kk, u32 m, u64* __restrict__ keys,
                                                          u32* __restrict__ vals, u32* __restrict__ err) {
  const u64 s = (u64)blockIdx.x * kBatchTPB + threadIdx.x;
  const u32 b = (u32)(s >> kk);
  if (b >= K) return;
  const u32 i = (u32)(s & ((1ull << kk) - 1));
  const u32 n = blocks[b].n;
  if (i >= n) return;                                        // padding: no suffix
  const u32 left = n - i;
  u64 chars = 0;
#pragma unroll
  for (u32 j = 0; j < (u32)kBatchKeyChars; ++j) chars = (chars << 8) | (j < left ? (u64)T[s + j] : 0ull);
  const u64 q = (u64)blocks[b].base + i;
  if (q >= m) { atomicOr(err, 1u); return; }
  keys[q] = ((u64)b << 51) | (chars << 3) | (u64)min(left, (u32)kBatchKeyChars);
  vals[q] = (u32)s;
}

// ---- a round's keys: (rank[s], second key) ------------------------------------------------------------------------
__global__ __launch_bounds__(kBatchTPB) void k_batch_gather(const u32* __restrict__ sfx, u32 mlist, const u32* __restrict__ rank,
                                                            const BatchBlock* __restrict__ blocks, u32 K, u32 kk, u64 h,
                                                            int second_bits, u64* __restrict__ keys, u32* __restrict__ err) {
  const u32 p = blockIdx.x * kBatchTPB + threadIdx.x;
  if (p >= mlist) return;
  const u32 s = sfx[p];
  const u32 b = s >> kk;
  if (b >= K) { atomicOr(err, 2u); keys[p] = 0; return; }
  const u64 i = s & ((1ull << kk) - 1);
  const u32 n = blocks[b].n;
  if (i >= n) { atomicOr(err, 2u); keys[p] = 0; return; }
  // the comparison with the block's end comes first: the look-up never leaves the block
  const u64 second = i + h < (u64)n ? (u64)rank[s + (u32)h] + 1ull : 0ull;
  keys[p] = ((u64)rank[s] << second_bits) | second;
}

// ---- heads of the (sub-)groups of a sorted list, and which entries stay (those of groups of two and more) ----------
__global__ __launch_bounds__(kBatchTPB) void k_batch_heads(const u64* __restrict__ keys, u32 mlist, u32* __restrict__ heads,
                                                           u32* __restrict__ keep) {
  const u32 p = blockIdx.x * kBatchTPB + threadIdx.x;
  if (p >= mlist) return;
  const u64 k = keys[p];
  const bool head = p == 0 || keys[p - 1] != k;
  const bool next_head = p + 1 == mlist || keys[p + 1] != k;
  heads[p] = head ? 1u : 0u;
  keep[p] = head && next_head ? 0u : 1u;
}

// the slot of every sub-group's head, by sub-group number (heads[] scanned: a head's word is its number)
__global__ __launch_bounds__(kBatchTPB) void k_batch_head_slots(const u64* __restrict__ keys, const u32* __restrict__ slot, u32 mlist,
                                                                const u32* __restrict__ heads, u32* __restrict__ head_slot,
                                                                u32* __restrict__ err) {
  const u32 p = blockIdx.x * kBatchTPB + threadIdx.x;
  if (p >= mlist) return;
  if (p != 0 && keys[p - 1] == keys[p]) return;
  const u32 g = heads[p];
  if (g >= mlist) { atomicOr(err, 4u); return; }
  head_slot[g] = slot ? slot[p] : p;
}

// ---- new ranks, and the next list: the entries that are still tied, in order ------------------------------------------
// rank[] is written and not read (the second keys were gathered by an earlier launch).
__global__ __launch_bounds__(kBatchTPB) void k_batch_rank(const u64* __restrict__ keys, const u32* __restrict__ sfx,
                                                          const u32* __restrict__ slot, u32 mlist, const u32* __restrict__ heads,
                                                          const u32* __restrict__ keep, const u32* __restrict__ head_slot,
                                                          u32* __restrict__ rank, u64 positions, u32 m,
                                                          u32* __restrict__ sfx_next, u32* __restrict__ slot_next,
                                                          u32* __restrict__ left, u32* __restrict__ err) {
  const u32 p = blockIdx.x * kBatchTPB + threadIdx.x;
  if (p >= mlist) return;
  const u64 k = keys[p];
  const bool head = p == 0 || keys[p - 1] != k;
  const bool next_head = p + 1 == mlist || keys[p + 1] != k;
  const u32 g = heads[p] + (head ? 1u : 0u) - 1u;            // (a member's word counts its own head: never 0 - 1)
  const u32 s = sfx[p];
  const bool stays = !(head && next_head);
  const u32 d = keep[p];
  if (p + 1 == mlist) *left = d + (stays ? 1u : 0u);
  if (g >= mlist || (u64)s >= positions) { atomicOr(err, 8u); return; }
  const u32 r = head_slot[g];
  if (r >= m) { atomicOr(err, 8u); return; }
  rank[s] = r;
  if (stays) {
    if (d >= mlist) { atomicOr(err, 8u); return; }
    sfx_next[d] = s;
    slot_next[d] = slot ? slot[p] : p;
  }
}

// ---- emit: out[rank] = T[s - 1], the end-of-block hole, the LF powers -------------------------------------------------
// Workgroups below emit_groups take 256 positions each: suffix i > 0 of block b stands in row j = rank[s] - base_b
// and brings T[s - 1]; row n_b - 1 has no byte of its own in the output, its character goes to the row of suffix 0
// (BWTransform.cpp:60).  The workgroups behind them take one block each and note its LF powers: lf[0] = row of suffix
// 0, lf[k] = row of suffix n_b - k * (n_b / n_lf) (a power whose suffix would be n_b itself -- n_lf above n_b -- is 0).
__global__ __launch_bounds__(kBatchTPB) void k_batch_emit(const u8* __restrict__ T, const u32* __restrict__ rank,
                                                          const BatchBlock* __restrict__ blocks, u32 K, u32 kk,
                                                          u32 emit_groups, u8* __restrict__ out, u32* __restrict__ lf,
                                                          u32* __restrict__ err) {
  if (blockIdx.x >= emit_groups) {
    const u32 b = blockIdx.x - emit_groups;
    if (b >= K) return;
    const u32 n = blocks[b].n, base = blocks[b].base, n_lf = blocks[b].n_lf, t = threadIdx.x;
    const u64 s0 = (u64)b << kk;
    u32 v = 0;
    if (t < n_lf) {
      const u32 pos = t == 0 ? 0u : n - t * (n / n_lf);
      if (pos < n) {
        v = rank[s0 + pos] - base;
        if (v >= n) { atomicOr(err, 16u); v = 0; }
      }
    }
    lf[(u64)b * 256u + t] = v;
    return;
  }
  const u64 s = (u64)blockIdx.x * kBatchTPB + threadIdx.x;
  const u32 b = (u32)(s >> kk);
  if (b >= K) return;
  const u32 i = (u32)(s & ((1ull << kk) - 1));
  const u32 n = blocks[b].n, base = blocks[b].base, size = n - 1u;
  if (i >= n || i == 0) return;                              // padding; suffix 0's row is the hole
  const u32 j = rank[s] - base;
  if (j >= n) { atomicOr(err, 16u); return; }
  u8* dst = out + blocks[b].offset;
  const u8 c = T[s - 1];
  if (j < size) { dst[j] = c; return; }
  const u32 hole = rank[(u64)b << kk] - base;                // j == n - 1: the last row's character fills the hole
  if (hole >= size) { atomicOr(err, 16u); return; }          // (suffix 0 cannot stand in the last row too)
  dst[hole] = c;
}

static u64 align_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

// The batch's workspace, carved out of the context's arena behind its three byte buffers (d_T, d_out, d_in keep their
// meaning: d_in stages the host form's bytes).  Per position of the strided array: T 1 byte, rank[] 4; per suffix:
// two key arrays 16, two suffix arrays 8, two slot arrays 8, head, keep and head-slot words 12 -- 49 bytes where
// every position is a suffix, against the arena's 100 and more per position; plus the radix tables and 2 KiB per block.
struct BatchPlan {
  u8* T; u32* rank; u64* K0; u64* K1; u32* V0; u32* V1; u32* SL0; u32* SL1; u32* heads; u32* keep; u32* head_slot;
  u32* table; u32* partial; BatchBlock* blocks; u32* counts; u32* lf; u32* small;
  bool fits;
};
static BatchPlan batch_plan(const BwtEngine& e, u64 positions, u64 m, u32 k) {
  u8* base = reinterpret_cast<u8*>(e.d_SA);
  const u64 room = static_cast<u8*>(e.arena) + e.arena_bytes - base;
  u64 o = 0;
  auto take = [&](u64 bytes) { u8* r = base + o; o = align_up(o + bytes, 256); return r; };
  BatchPlan p;
  p.T = take(positions + 64);
  p.rank = reinterpret_cast<u32*>(take(positions * 4));
  p.K0 = reinterpret_cast<u64*>(take(m * 8));
  p.K1 = reinterpret_cast<u64*>(take(m * 8));
  p.V0 = reinterpret_cast<u32*>(take(m * 4));
  p.V1 = reinterpret_cast<u32*>(take(m * 4));
  p.SL0 = reinterpret_cast<u32*>(take(m * 4));
  p.SL1 = reinterpret_cast<u32*>(take(m * 4));
  p.heads = reinterpret_cast<u32*>(take(m * 4));
  p.keep = reinterpret_cast<u32*>(take(m * 4));
  p.head_slot = reinterpret_cast<u32*>(take(m * 4));
  p.table = reinterpret_cast<u32*>(take(radix_table_words(m) * 4));
  p.partial = reinterpret_cast<u32*>(take((std::max<u64>(radix_partial_words(m), m / kScanTile + 2)) * 4));
  p.blocks = reinterpret_cast<BatchBlock*>(take((u64)k * sizeof(BatchBlock)));
  p.counts = reinterpret_cast<u32*>(take((u64)k * 2 * 256 * 4));   // counts, then the LF rows: one download
  p.lf = p.counts + (u64)k * 256;
  p.small = reinterpret_cast<u32*>(take(64 * 4));                  // [0] entries left, [1] error word
  p.fits = o <= room;
  return p;
}

struct BatchShape { u32 kk; u64 positions, m; std::vector<BatchBlock> table; };

static void batch_shape(const bwtc_hip_batch_item* items, u32 k, u32 kk, BatchShape* sh) {
  sh->kk = kk;
  sh->positions = (u64)k << kk;
  sh->table.resize(k);
  u64 base = 0;
  for (u32 b = 0; b < k; ++b) {
    sh->table[b] = BatchBlock{items[b].offset, items[b].size + 1u, (u32)base, items[b].n_lf, 0u};
    base += (u64)items[b].size + 1u;
  }
  sh->m = base;
}

// the block table up, the counts cleared, T loaded: what the transform and the key hook share
static int batch_load(BwtEngine& e, const BatchPlan& p, const BatchShape& sh, const u8* d_src, u32 k) {
  hipStream_t st = e.stream;
  BWTC_HIP_TRY(hipMemcpyAsync(p.blocks, sh.table.data(), (u64)k * sizeof(BatchBlock), hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemsetAsync(p.counts, 0, (u64)k * 2 * 256 * 4, st));
  BWTC_HIP_TRY(hipMemsetAsync(p.small, 0, 64 * 4, st));
  hipLaunchKernelGGL(k_batch_load, dim3(ceil_div(sh.positions, kBatchLoadTile)), dim3(kBatchTPB), 0, st, d_src, p.T,
                     (const BatchBlock*)p.blocks, k, sh.kk, p.counts);
  hipLaunchKernelGGL(k_batch_keys, dim3(ceil_div(sh.positions, kBatchTPB)), dim3(kBatchTPB), 0, st, (const u8*)p.T,
                     (const BatchBlock*)p.blocks, k, sh.kk, (u32)sh.m, p.K0, p.V0, p.small + 1);
  return 0;
}

}  // namespace

int batch_validate(const BwtEngine& e, const bwtc_hip_batch_item* items, u32 k, u32* stride_log2) {
  if (!items || k == 0 || k > kBatchMaxBlocks) return -1;
  u32 max_n = 0;
  for (u32 b = 0; b < k; ++b) {
    if (items[b].size == 0 || items[b].size > e.max_block) return -1;
    if (items[b].n_lf == 0 || items[b].n_lf > 256) return -1;
    if (items[b].offset + items[b].size < items[b].offset) return -1;
    max_n = std::max(max_n, items[b].size + 1u);
  }
  u32 kk = 0;
  while ((1ull << kk) < max_n) ++kk;
  if (((u64)k << kk) > (u64)e.max_block + 1) return -1;
  std::vector<u32> order(k);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return items[a].offset < items[b].offset; });
  for (u32 i = 0; i + 1 < k; ++i)
    if (items[order[i]].offset + items[order[i]].size > items[order[i + 1]].offset) return -1;
  *stride_log2 = kk;
  return 0;
}

int batch_transform_device(BwtEngine& e, const u8* d_in, u8* d_out, const bwtc_hip_batch_item* items, u32 k,
                           u32* lf, u32* freqs, bwtc_hip_batch_stats* bs) {
  u32 kk = 0;
  if (!d_in || !d_out || !lf || batch_validate(e, items, k, &kk) != 0) return -1;
  BatchShape sh;
  batch_shape(items, k, kk, &sh);
  const BatchPlan p = batch_plan(e, sh.positions, sh.m, k);
  if (!p.fits) return -2;
  const u32 m = (u32)sh.m;
  hipStream_t st = e.stream;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  bwtc_hip_batch_stats s = {};
  s.blocks = k; s.stride_log2 = kk; s.suffixes = sh.m;
  e.wait_seq = 0;
  auto wait = [&]() { ++s.host_waits; return e.wait(); };
  auto grid = [](u64 items_) { return dim3(ceil_div(items_, kBatchTPB)); };
  BWTC_HIP_TRY(hipEventRecord(e.ev_begin, st));
  int rc = batch_load(e, p, sh, d_in, k);
  if (rc) return rc;

  // one ranking: a sorted list (keys, suffixes; slot == null: entry p stands in slot p) -> rank[], the next list in
  // (sfx_next, slot_next), the entries left in small[0] -> h_small[0] after the wait
  auto ranking = [&](const u64* keys, const u32* sfx, const u32* slot, u32 mlist, u32* sfx_next, u32* slot_next) -> int {
    hipLaunchKernelGGL(k_batch_heads, grid(mlist), dim3(kBatchTPB), 0, st, keys, mlist, p.heads, p.keep);
    exclusive_scan_u32(p.heads, mlist, p.partial, st);
    exclusive_scan_u32(p.keep, mlist, p.partial, st);
    hipLaunchKernelGGL(k_batch_head_slots, grid(mlist), dim3(kBatchTPB), 0, st, keys, slot, mlist, (const u32*)p.heads,
                       p.head_slot, p.small + 1);
    hipLaunchKernelGGL(k_batch_rank, grid(mlist), dim3(kBatchTPB), 0, st, keys, sfx, slot, mlist, (const u32*)p.heads,
                       (const u32*)p.keep, (const u32*)p.head_slot, p.rank, sh.positions, m, sfx_next, slot_next,
                       p.small, p.small + 1);
    BWTC_HIP_TRY(hipMemcpyAsync(e.h_small, p.small, 8, hipMemcpyDeviceToHost, st));
    BWTC_HIP_TRY(wait());
    return e.h_small[1] ? -3 : 0;
  };

  // the initial sort: only the bits in use (the block ids of a batch of k need bit_width(k - 1) of the twelve)
  u64* ks = nullptr; u32* vs = nullptr;
  radix_sort_pairs<u64, u32>(p.K0, p.K1, p.V0, p.V1, m, 51 + bit_width_u64(k - 1), p.table, p.partial, st, &ks, &vs);
  u32* sfx = vs == p.V0 ? p.V1 : p.V0;                       // the list: suffixes and slots
  u32* slots = p.SL0;
  rc = ranking(ks, vs, nullptr, m, sfx, slots);
  if (rc) return rc;
  u32 left = e.h_small[0];
  s.active[0] = left;
  const int second_bits = bit_width_u64(m), rank_bits = bit_width_u64(m - 1);
  for (u64 h = kBatchKeyChars; left > 0; h *= 2) {
    if (left > m || s.rounds >= kBatchMaxRounds) return -3;
    u32* sfx_other = sfx == p.V0 ? p.V1 : p.V0;
    u32* slots_next = slots == p.SL0 ? p.SL1 : p.SL0;
    hipLaunchKernelGGL(k_batch_gather, grid(left), dim3(kBatchTPB), 0, st, (const u32*)sfx, left, (const u32*)p.rank,
                       (const BatchBlock*)p.blocks, k, kk, h, second_bits, p.K0, p.small + 1);
    radix_sort_pairs<u64, u32>(p.K0, p.K1, sfx, sfx_other, left, second_bits + rank_bits, p.table, p.partial, st, &ks, &vs);
    u32* sfx_next = vs == p.V0 ? p.V1 : p.V0;
    rc = ranking(ks, vs, slots, left, sfx_next, slots_next);
    if (rc) return rc;
    sfx = sfx_next; slots = slots_next;
    left = e.h_small[0];
    ++s.rounds;
    if (s.rounds < 32) s.active[s.rounds] = left;
  }

  const u32 emit_groups = ceil_div(sh.positions, kBatchTPB);
  hipLaunchKernelGGL(k_batch_emit, dim3(emit_groups + k), dim3(kBatchTPB), 0, st, (const u8*)p.T, (const u32*)p.rank,
                     (const BatchBlock*)p.blocks, k, kk, emit_groups, d_out, p.lf, p.small + 1);
  std::vector<u32> back((u64)k * 2 * 256);
  BWTC_HIP_TRY(hipMemcpyAsync(back.data(), p.counts, back.size() * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_small, p.small, 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipEventRecord(e.ev_end, st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  BWTC_HIP_TRY(take_sticky_error());
  if (radix_fault_take() || e.h_small[1]) return -3;
  for (u64 i = 0; i < (u64)k * 256; ++i) lf[i] = back[(u64)k * 256 + i];
  if (freqs) for (u64 i = 0; i < (u64)k * 256; ++i) freqs[i] += back[i];
  BWTC_HIP_TRY(hipEventElapsedTime(&s.ms_total, e.ev_begin, e.ev_end));
  if (bs) *bs = s;
  return 0;
}

int batch_transform_host(BwtEngine& e, u8* data, const bwtc_hip_batch_item* items, u32 k, u32* lf, u32* freqs,
                         bwtc_hip_batch_stats* bs) {
  u32 kk = 0;
  if (!data || !lf || batch_validate(e, items, k, &kk) != 0) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  // packed: the sizes add up to less than k * S <= max_block + 1, which the staging buffers hold
  std::vector<bwtc_hip_batch_item> packed(items, items + k);
  u64 total = 0;
  for (u32 b = 0; b < k; ++b) {
    packed[b].offset = total;
    std::memcpy(e.h_stage + total, data + items[b].offset, items[b].size);
    total += items[b].size;
  }
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, e.h_stage, total, hipMemcpyHostToDevice, e.stream));
  const int rc = batch_transform_device(e, e.d_in, e.d_in, packed.data(), k, lf, freqs, bs);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_stage, e.d_in, total, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  if (bs) ++bs->host_waits;
  for (u32 b = 0; b < k; ++b) std::memcpy(data + items[b].offset, e.h_stage + packed[b].offset, items[b].size);
  return 0;
}

int batch_test_keys(BwtEngine& e, const u8* data, const bwtc_hip_batch_item* items, u32 k, u8* T_out, u64* keys_out,
                    u32* freqs_out) {
  u32 kk = 0;
  if (!data || !T_out || !keys_out || !freqs_out || batch_validate(e, items, k, &kk) != 0) return -1;
  u64 end = 0;
  for (u32 b = 0; b < k; ++b) end = std::max<u64>(end, items[b].offset + items[b].size);
  if (end > e.cap) return -1;                                // d_in holds cap + 64 bytes
  BatchShape sh;
  batch_shape(items, k, kk, &sh);
  const BatchPlan p = batch_plan(e, sh.positions, sh.m, k);
  if (!p.fits) return -2;
  hipStream_t st = e.stream;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, data, end, hipMemcpyHostToDevice, st));
  // what the kernels do not write is told apart from what they do: the keys and T start as 0xA5
  BWTC_HIP_TRY(hipMemsetAsync(p.T, 0xA5, sh.positions + 64, st));
  BWTC_HIP_TRY(hipMemsetAsync(p.K0, 0xA5, sh.m * 8, st));
  const int rc = batch_load(e, p, sh, e.d_in, k);
  if (rc) return rc;
  std::vector<u8> T(sh.positions);
  BWTC_HIP_TRY(hipMemcpyAsync(T.data(), p.T, sh.positions, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(keys_out, p.K0, sh.m * 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(freqs_out, p.counts, (u64)k * 256 * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_small, p.small, 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  if (e.h_small[1]) return -3;
  for (u32 b = 0; b < k; ++b)
    std::memcpy(T_out + sh.table[b].base, T.data() + ((u64)b << kk), sh.table[b].n);
  return 0;
}

}  // namespace bwtc_hip
