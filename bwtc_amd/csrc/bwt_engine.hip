// BwtEngine implementation: kernels + host orchestration.  See bwt_engine.hpp.
#include "bwt_engine.hpp"
#include "radix_sort.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <climits>
#include <ctime>
#include <sys/prctl.h>

namespace bwtc_hip {

// ---------------------------------------------------------------------------------------
// K1  load (+reverse) + 256-bin histogram.  T[j] = src[ncopy-1-j] (reverse) or src[j] for
//     j < ncopy; T[ncopy..padded) = 0.  The histogram is over the ncopy source bytes
//     (BWTransform.cpp:53-55 + divsufsort.c:506-512: the sentinel is never counted).
//     One workgroup = 4096 destination bytes: the source window is staged in LDS with
//     16-byte loads, every thread assembles one aligned 16-byte store.  Histogram in LDS,
//     16 interleaved copies per bin (copy = lane & 15) so that skewed inputs (text, DNA,
//     all-equal blocks) do not serialise on one address; one global atomic per non-empty
//     bin per workgroup.
// ---------------------------------------------------------------------------------------
constexpr int kLoadTPB = 256;
constexpr int kLoadTile = kLoadTPB * 16;
constexpr u32 kTextPad = 128;  // zero bytes guaranteed after T[n-1] (a code key looks at up to 74 characters of a suffix)

__global__ __launch_bounds__(kLoadTPB) void k_load_hist(const u8* __restrict__ src,
                                                        u8* __restrict__ T, u32 ncopy,
                                                        u32 padded, int reverse, int aligned,
                                                        u32* __restrict__ freqs) {
  __shared__ __attribute__((aligned(16))) u8 s_src[kLoadTile + 48];   // + slack: the fast path reads one word past its 16 bytes
  __shared__ u32 s_hist[256 * 16];
  const u32 tid = threadIdx.x;
  for (u32 i = tid; i < 256 * 16; i += kLoadTPB) s_hist[i] = 0;
  // A workgroup walks many tiles and flushes its histogram once: one flush per 4 KiB tile was
  // 65 000 global atomics on each of the 256 counters for a 256 MiB block, and that serialisation
  // -- not the bytes -- was this kernel's time.
  const u32 ntiles = (padded + (u32)kLoadTile - 1u) / (u32)kLoadTile;
  for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
  __syncthreads();                                       // the previous tile's readers of s_src are done
  const u32 d0 = tile * kLoadTile;                       // first destination byte
  const u32 dend = min(d0 + (u32)kLoadTile, padded);     // one past the last one
  // source bytes this tile needs: [a_lo, a_hi)
  u32 a_lo = 0, a_hi = 0;
  if (d0 < ncopy) {
    const u32 last = min(dend, ncopy);                   // destinations [d0, last) have a source
    if (reverse) { a_lo = ncopy - last; a_hi = ncopy - d0; }
    else { a_lo = d0; a_hi = last; }
  }
  const u32 w_lo = a_lo & ~15u;
  if (a_hi > a_lo) {
    const u32 nchunks = (a_hi - w_lo + 15u) / 16u;
    for (u32 c = tid; c < nchunks; c += kLoadTPB) {
      const u32 a = w_lo + 16u * c;
      if (aligned && a + 16u <= ncopy) {
        *reinterpret_cast<uint4*>(&s_src[16u * c]) = *reinterpret_cast<const uint4*>(src + a);
      } else {
        for (u32 b = 0; b < 16u; ++b) s_src[16u * c + b] = (a + b < ncopy) ? src[a + b] : (u8)0;
      }
    }
  }
  __syncthreads();
  const u32 j0 = d0 + tid * 16u;
  if (j0 < dend) {
    u32 wds[4] = {0, 0, 0, 0};
    const u32 copy = tid & 15u;
    if (j0 + 16u <= ncopy) {
      // all sixteen bytes have a source: five aligned LDS words, shifted into place (byte reads of
      // LDS made this kernel latency bound); reversed = the same bytes, words and bytes swapped
      const u32 off = (reverse ? (ncopy - 16u - j0) : j0) - w_lo;
      const u32* s32 = reinterpret_cast<const u32*>(s_src) + (off >> 2);
      const u32 sh = (off & 3u) * 8u;
      u32 d[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) d[q] = s32[q];
      u32 w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = sh ? ((d[q] >> sh) | (d[q + 1] << (32u - sh))) : d[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) wds[q] = reverse ? __builtin_bswap32(w[3 - q]) : w[q];
#pragma unroll
      for (int e = 0; e < 16; ++e) atomicAdd(&s_hist[((wds[e >> 2] >> (8 * (e & 3))) & 255u) * 16u + copy], 1u);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const u32 j = j0 + e;
        if (j < ncopy) {
          const u32 a = reverse ? (ncopy - 1u - j) : j;
          const u32 c = s_src[a - w_lo];
          wds[e >> 2] |= c << (8 * (e & 3));
          atomicAdd(&s_hist[c * 16u + copy], 1u);
        }
      }
    }
    *reinterpret_cast<uint4*>(T + j0) = make_uint4(wds[0], wds[1], wds[2], wds[3]);
  }
  }                                                      // tiles
  __syncthreads();
  u32 c = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) c += s_hist[tid * 16u + r];
  if (c) atomicAdd(&freqs[tid], c);
}

// ---------------------------------------------------------------------------------------
// K2  initial keys.  The alphabet is remapped to dense codes 0..sigma-1 (order preserving,
//     byte 0 -> code 0) and the key of suffix i is its first k characters as a base-sigma
//     number, most significant first (sigma^k <= 2^bits of K; mixed-radix packing wastes no
//     fractional bits: 10 characters of a 45-symbol text fit 55 bits = 7 radix passes);
//     characters past the end read the zero padding.  Slot j holds suffix
//     i = n-1-j (descending!).  Feeding the stable sort in descending suffix order puts,
//     inside every group of equal keys, the suffixes shorter than k first and
//     shortest-first -- exactly "proper prefix sorts first" -- without spending key bits.
// ---------------------------------------------------------------------------------------
// Dense codes of T[i_base .. i_base + count) into s_code, for a workgroup of 256 threads and
// count <= 2040: aligned words of T, at most two per thread and both in flight, instead of a loop
// of byte loads (each a memory latency of its own).  T is zero padded (and its region longer still).
__device__ __forceinline__ void stage_codes(const u8* __restrict__ T, const u8* s_lut, u8* s_code,
                                            u32 i_base, u32 count) {
  const u32 a0 = i_base & ~3u, sh = i_base - a0;
  const u32 nw = (sh + count + 3u) / 4u;
  u32 w[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const u32 x = threadIdx.x + 256u * e;
    w[e] = x < nw ? *reinterpret_cast<const u32*>(T + a0 + 4u * x) : 0u;
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const u32 x = threadIdx.x + 256u * e;
    if (x < nw) {
#pragma unroll
      for (u32 b = 0; b < 4u; ++b) {
        const u32 t = 4u * x + b - sh;                    // wraps for the bytes before i_base
        if (t < count) s_code[t] = s_lut[(w[e] >> (8u * b)) & 255u];
      }
    }
  }
}

template <typename K>
__global__ __launch_bounds__(256) void k_make_keys(const u8* __restrict__ T,
                                                   const u8* __restrict__ lut,
                                                   K* __restrict__ keys, u32* __restrict__ idx,
                                                   u32 n, int k, u32 sigma, K top, u8* __restrict__ plane,
                                                   int idx_hi) {
  // A workgroup makes 1024 consecutive slots.  The dense codes of its stretch of T are staged in
  // LDS once; a thread builds four consecutive suffixes' keys -- the first from k characters, the
  // next three by rolling one character out and one in (top = sigma^(k-1)), k+3 LDS bytes instead
  // of 4k -- and parks them in LDS, from where consecutive lanes write consecutive slots (a thread
  // storing its own four keys would touch a cache line per lane).
  constexpr u32 kTile = 1024;
  __shared__ u8 s_lut[256];
  __shared__ u8 s_code[kTile + 64];
  __shared__ K s_key[kTile];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const u32 J0 = blockIdx.x * kTile;                // first slot of the tile
  if (J0 >= n) return;
  const u32 cntw = min(kTile, n - J0);              // its slots
  const u32 i_base = n - J0 - cntw;                 // smallest suffix of the tile (its last slot)
  stage_codes(T, s_lut, s_code, i_base, cntw + (u32)k);
  __syncthreads();
  const u32 o = 4u * threadIdx.x;                   // this thread's suffixes: i_base + o .. + 3
  if (o < cntw) {
    const u32 cnt = min(4u, cntw - o);
    K key = 0;
    for (int t = 0; t < k; ++t) key = (K)(key * (K)sigma) + (K)s_code[o + t];
    for (u32 s = 0; s < cnt; ++s) {
      s_key[cntw - 1u - (o + s)] = key;             // slot order is descending suffix order
      key = (K)((key - (K)s_code[o + s] * top) * (K)sigma) + (K)s_code[o + s + k];
    }
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < cntw; j += 256u) {
    K key = s_key[j];
    // idx_hi: the upper bits of the suffix number ride in bits 48.. of the (at most 48-bit) key
    if (sizeof(K) == 8 && idx_hi) key |= (K)((u64)((n - 1u - (J0 + j)) >> 16) << 48);
    keys[J0 + j] = key;
    if (idx) idx[J0 + j] = n - 1u - (J0 + j);        // nullptr: the sort's first pass makes the values up
    if (plane) plane[J0 + j] = (u8)s_key[j];         // the first radix pass's digits (radix_sort.hpp, planes)
  }
}

// ---------------------------------------------------------------------------------------
// K2g initial keys from dense g-gram codes.  A text uses few of the sigma^g possible g-grams
//     (the 256 MiB synthetic text: 40 symbols, 2.56 M possible 4-grams, some ten thousand
//     present), so numbering the PRESENT grams in order packs g characters into
//     b = log2(present) bits instead of g log2(sigma): 12 characters of that text take 48 key bits
//     = 6 radix passes instead of 64 bits = 8 passes, and the order of the keys is the same
//     (the numbering is monotone in the gram's value, which is its characters as a base-sigma
//     number).  Small passes before the keys: mark the grams that occur in a byte map, pack it
//     into a bitmap, and one workgroup turns that into a rank table (word, grams before it) --
//     640 KB for the text alphabet's 4-grams, resident in L2, where a table of codes indexed by
//     the gram's value spread the few ten thousand present grams over 3.5 MB of cache lines; the
//     key maker numbers a gram with one 16-byte lookup and a popcount.  Grams that start in the
//     padding are the all-zero gram, which position n-1 (the terminator and padding) marks.
// ---------------------------------------------------------------------------------------
constexpr u32 kGramMaxU = 1u << 22;         // largest gram universe: 64 Ki bitmap words, a table of 1 MiB
constexpr u32 kGramTile = 4096;
constexpr u32 kGramMinN = 1u << 22;         // smaller blocks keep the plain base-sigma key

// Marks the grams that occur in a byte map: a look at the byte, a plain store of 1 where it is
// still 0 (every writer stores the same value; a bitmap would need an atomic OR per new bit, and
// with the lookups served by each CU's own L1 the same hot words were OR-ed from everywhere:
// three times slower).
__global__ __launch_bounds__(256) void k_gram_mark(const u8* __restrict__ T, const u8* __restrict__ lut,
                                                   u32 n, int g, u32 sigma, u32 top,
                                                   u8* __restrict__ present) {
  __shared__ u8 s_lut[256];
  __shared__ __attribute__((aligned(16))) u8 s_code[kGramTile + 64];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  const u32 ntiles = (n + kGramTile - 1u) / kGramTile;
  for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    const u32 base = tile * kGramTile;
    {
      const uint4 v = *reinterpret_cast<const uint4*>(T + base + 16u * threadIdx.x);   // T's region is padded by a tile
      const u32 w[4] = {v.x, v.y, v.z, v.w};
      u32 c[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        c[q] = (u32)s_lut[w[q] & 255u] | (u32)s_lut[(w[q] >> 8) & 255u] << 8 |
               (u32)s_lut[(w[q] >> 16) & 255u] << 16 | (u32)s_lut[w[q] >> 24] << 24;
      *reinterpret_cast<uint4*>(&s_code[16u * threadIdx.x]) = make_uint4(c[0], c[1], c[2], c[3]);
      if (threadIdx.x < 64u) s_code[kGramTile + threadIdx.x] = s_lut[T[base + kGramTile + threadIdx.x]];
    }
    __syncthreads();
    const u32 o = 16u * threadIdx.x;
    if (base + o < n) {
      u32 v = 0;
      for (int t = 0; t < g; ++t) v = v * sigma + s_code[o + t];
      const u32 cnt = min(16u, n - (base + o));
      u32 vs[16];
      u8 seen[16];
#pragma unroll
      for (u32 e = 0; e < 16u; ++e) {
        vs[e] = e < cnt ? v : 0u;
        v = (v - (u32)s_code[o + e] * top) * sigma + s_code[o + e + g];
      }
#pragma unroll
      for (u32 e = 0; e < 16u; ++e) seen[e] = present[vs[e]];     // sixteen independent lookups, then the few stores
#pragma unroll
      for (u32 e = 0; e < 16u; ++e) if (e < cnt && !seen[e]) present[vs[e]] = 1;
    }
  }
}

// 64 bytes of the map (each 0 or 1) -> one bitmap word
__global__ __launch_bounds__(256) void k_gram_pack(const u8* __restrict__ present, u32 nwords,
                                                   unsigned long long* __restrict__ bits) {
  const u32 w = blockIdx.x * 256u + threadIdx.x;
  if (w >= nwords) return;                              // the map is allocated and cleared in whole words
  const uint4* p = reinterpret_cast<const uint4*>(present + 64ull * w);
  unsigned long long out = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 v = p[q];
    const u32 x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)     // four bytes b0..b3 -> b0 | b1 << 1 | b2 << 2 | b3 << 3 in the product's top byte
      out |= (unsigned long long)((x[k] * 0x01020408u) >> 24 & 15u) << (16 * q + 4 * k);
  }
  bits[w] = out;
}

// One workgroup: the bitmap's words with the number of present grams before each ->
// table[w] = {bits low, bits high, grams before, 0}; the code of gram v is
// table[v >> 6].z + popcount(bits below bit v & 63).  At most 65 536 words.
__global__ __launch_bounds__(1024) void k_gram_table(const unsigned long long* __restrict__ present, u32 nwords,
                                                     uint4* __restrict__ table, u32* __restrict__ distinct) {
  __shared__ u32 scratch[1024 / kWave + 1];
  const u32 per = ((nwords + 1023u) / 1024u + 7u) & ~7u;   // consecutive words per thread (<= 64), in batches of eight loads
  const u32 w0 = threadIdx.x * per;
  u32 mine = 0;
  for (u32 i = 0; i < per; i += 8u) {
    unsigned long long b[8];
#pragma unroll
    for (u32 k = 0; k < 8u; ++k) b[k] = w0 + i + k < nwords ? present[w0 + i + k] : 0ull;
#pragma unroll
    for (u32 k = 0; k < 8u; ++k) mine += (u32)__popcll(b[k]);
  }
  u32 total;
  u32 run = block_scan_excl_add<1024>(mine, scratch, &total);
  for (u32 i = 0; i < per; i += 8u) {
    unsigned long long b[8];
#pragma unroll
    for (u32 k = 0; k < 8u; ++k) b[k] = w0 + i + k < nwords ? present[w0 + i + k] : 0ull;
#pragma unroll
    for (u32 k = 0; k < 8u; ++k) {
      if (w0 + i + k < nwords) table[w0 + i + k] = make_uint4((u32)b[k], (u32)(b[k] >> 32), run, 0u);
      run += (u32)__popcll(b[k]);
    }
  }
  if (threadIdx.x == 0) *distinct = total;
}

__device__ __forceinline__ u32 gram_code(const uint4* __restrict__ table, u32 v) {
  const uint4 e = table[v >> 6];
  const unsigned long long bits = (unsigned long long)e.x | ((unsigned long long)e.y << 32);
  return e.z + (u32)__popcll(bits & ((1ull << (v & 63u)) - 1ull));
}

// keys of G grams of g characters, b bits per gram code; slots in descending suffix order as in k_make_keys
//
// Long keys (lk.w != nullptr, see LongKey): the item also gets a second key word w = the NEXT lk.G2
// grams (characters G g .. (G + G2) g of the suffix), and the dense code of its predecessor character
// T[i-1] rides in spare bits of the key, so that the one long sort orders the suffixes by (G + G2) g
// characters and the ranking behind it can emit the transform's bytes without going back to T.
struct LongKey {
  u32* w; int G2;                // make: where the second words go, grams per word
  int first_r; u32 first_mask;   // a second word of fewer than eight bits: the sort's first digit is the bridge digit
                                 // (radix_sort_long), w under the key's lowest bits; first_r = w's bits, -1: the digit is w's
  int hi_shift;                  // key bits [hi_shift, hi_shift + 13): the upper bits of the suffix number
  int chr_shift; u32 chr_mask;   // key bits of the predecessor character's dense code
};
__global__ __launch_bounds__(256) void k_make_keys_gram(const u8* __restrict__ T, const u8* __restrict__ lut,
                                                        const uint4* __restrict__ gtable,
                                                        u64* __restrict__ keys, u32* __restrict__ idx, u32 n,
                                                        int g, int G, int b, u32 sigma, u32 top,
                                                        u8* __restrict__ plane, int idx_hi, LongKey lk) {
  constexpr u32 kTile = 1024;
  __shared__ u8 s_lut[256];
  __shared__ u8 s_code[kTile + 136];
  __shared__ u32 s_g[kTile + 128];
  __shared__ u64 s_key[kTile];
  __shared__ u32 s_w[kTile];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const u32 J0 = blockIdx.x * kTile;
  if (J0 >= n) return;
  const u32 cntw = min(kTile, n - J0);
  const u32 i_base = n - J0 - cntw;
  const int Gall = G + (lk.w ? lk.G2 : 0);
  const u32 span = cntw + (u32)((Gall - 1) * g);     // gram starts this tile looks at (Gall g <= 96)
  const u32 pre = (lk.w && i_base > 0) ? 1u : 0u;    // long keys: one character before the tile's first suffix
  stage_codes(T, s_lut, s_code, i_base - pre, span + (u32)g + pre);
  __syncthreads();
  const u8* s_c = s_code + pre;                       // s_c[t] = code of T[i_base + t]
  {
    // span <= 1024 + 60: at most five gram starts per thread, strided, so that the five table
    // lookups (the kernel's only latency) are in flight together
    u32 v[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const u32 t = threadIdx.x + 256u * e;
      v[e] = 0;
      if (t < span) for (int c = 0; c < g; ++c) v[e] = v[e] * sigma + s_c[t + c];
    }
    u32 cd[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) cd[e] = threadIdx.x + 256u * e < span ? gram_code(gtable, v[e]) : 0u;
#pragma unroll
    for (int e = 0; e < 5; ++e) if (threadIdx.x + 256u * e < span) s_g[threadIdx.x + 256u * e] = cd[e];
  }
  __syncthreads();
  const u32 o = 4u * threadIdx.x;
  if (o < cntw) {
    const u32 cnt = min(4u, cntw - o);
    for (u32 s = 0; s < cnt; ++s) {
      u64 key = 0;
      for (int j = 0; j < G; ++j) key = (key << b) | (u64)s_g[o + s + (u32)(j * g)];
      if (lk.w) {
        u32 w = 0;
        for (int j = G; j < Gall; ++j) w = (w << b) | s_g[o + s + (u32)(j * g)];
        s_w[cntw - 1u - (o + s)] = w;
        const u32 i = i_base + o + s;                  // its predecessor's code (suffix 0 has none)
        key |= (u64)(i ? (u32)s_c[(int)(o + s) - 1] : 0u) << lk.chr_shift;
      }
      s_key[cntw - 1u - (o + s)] = key;
    }
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < cntw; j += 256u) {
    u64 key = s_key[j];
    if (idx_hi) key |= (u64)((n - 1u - (J0 + j)) >> 16) << (lk.w ? lk.hi_shift : 48);
    keys[J0 + j] = key;
    if (idx) idx[J0 + j] = n - 1u - (J0 + j);
    if (lk.w) {
      const u32 w = s_w[j];
      lk.w[J0 + j] = w;
      if (plane) plane[J0 + j] = lk.first_r < 0 ? (u8)w : (u8)((w | ((u32)key << lk.first_r)) & lk.first_mask);   // the long sort's first digit
    } else if (plane) plane[J0 + j] = (u8)s_key[j];
  }
}

// ---------------------------------------------------------------------------------------
// K2c initial keys from an order-preserving prefix code ("code keys", round 5).
//
//     Dense gram codes pack a fixed number of characters into the key: 20 of the 64-token generator's 40
//     symbols, but 12 of a real text's 170-210 -- and, worse, the same 12 of a string that occurs a
//     million times as of one that occurs twice, so that the frequent strings' groups stay huge.  Here
//     every character is written with a prefix code that depends on the character before it (an order-1
//     model of the block, taken from a sample of its character pairs), and a suffix's key is the first
//     kbits bits of its code string: frequent continuations cost few bits, so a frequent string gets MORE
//     of its characters into the key and the groups the sort leaves are levelled out (256 MiB of the
//     generator's text: 2.6 % of the suffixes tied after 72 key bits, against 21.5 % after 20 characters).
//
//     Order.  For every context the code is alphabetic (codewords in symbol order, prefix free: a
//     weight-balanced binary tree over the symbols, k_code_build), so two suffixes that first differ at
//     character j -- whose context, character j-1, they share -- have equal code strings up to that
//     character's codeword and differ there in symbol order: the code strings compare as the suffixes do,
//     and so do their first kbits bits (with ties).  A suffix's first character has no context inside the
//     suffix: it takes the order-0 code (row 256 of the table).  The terminator and the padding behind it
//     are symbol 0 (or share the smallest symbol's code, as in k_make_keys): the smallest continuation.
//
//     Depth.  Suffixes with equal keys share the key's COMPLETE codewords (the same bits decode the same
//     way), k characters, a number that differs from key to key.  The item carries it as a 3-bit level
//     (a lower bound: kCodeLevelDepth) in spare key bits; the ranking hands it on to the finisher, which
//     compares the text from there.
//
//     All codewords of the block's text are one bit string (a character's codeword does not depend on
//     which suffix it is read for), so a tile looks its characters' codewords up ONCE, scans their
//     lengths, writes the bits into LDS, and every suffix key is 72 bits cut out of that string at the
//     suffix's second character, behind its first character's order-0 codeword.
// ---------------------------------------------------------------------------------------
constexpr u32 kCodeRows = 257;                // contexts 0..255, and the order-0 row
constexpr u32 kCodeOrder0 = 256;
constexpr u32 kCodeMaxLen = 26;               // longest codeword k_code_build may make (27 code bits + 5 length bits per entry)
constexpr u32 kCodeLA = 72;                   // characters a tile looks ahead: a key has at most 72 bits, a codeword at least one
constexpr u32 kPairReplicas = 8;              // copies of the pair counters (hot pairs: one address per XCD-worth of workgroups)
constexpr u32 kPairTile = 4096;
// the level's depth: suffixes with equal keys of that level share at least so many characters
__host__ __device__ __forceinline__ u32 code_level_depth(u32 level) { return (u32)((0x30201814100C0801ull >> (8u * level)) & 255ull); }
__device__ __forceinline__ u32 code_level_of(u32 k) {
  return k >= 48u ? 7u : k >= 32u ? 6u : k >= 24u ? 5u : k >= 20u ? 4u : k >= 16u ? 3u : k >= 12u ? 2u : k >= 8u ? 1u : 0u;
}

// Character pairs of a sample of the text: workgroup b counts the pairs of tile floor(b * ntiles / gridDim).
// cnt[replica][a * 256 + b] over dense codes; pair (T[j-1], T[j]).
__global__ __launch_bounds__(256) void k_pair_counts(const u8* __restrict__ T, const u8* __restrict__ lut, u32 n,
                                                     u32* __restrict__ cnt) {
  __shared__ u8 s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const u32 ntiles = (n + kPairTile - 1u) / kPairTile;
  const u32 tile = (u32)(((u64)blockIdx.x * ntiles) / gridDim.x);
  const u32 j0 = tile * kPairTile + 16u * threadIdx.x;
  if (j0 >= n) return;
  const uint4 v = *reinterpret_cast<const uint4*>(T + j0);          // T is padded by more than a tile
  const u32 w[4] = {v.x, v.y, v.z, v.w};
  u32 prev = j0 ? s_lut[T[j0 - 1u]] : 0u;
  u32* mine = cnt + (size_t)(blockIdx.x % kPairReplicas) * 65536u;
#pragma unroll
  for (u32 e = 0; e < 16u; ++e) {
    const u32 c = s_lut[(w[e >> 2] >> (8u * (e & 3u))) & 255u];
    if (j0 + e < n && j0 + e > 0u) atomicAdd(&mine[prev * 256u + c], 1u);
    prev = c;
  }
}

// One workgroup per context (row 256: all contexts together, the order-0 code): the alphabetic code of the
// sigma symbols for the weights count + 1 (every symbol can follow every context: unseen pairs get long
// codewords, not none).  Weight-balanced tree: an interval of symbols is cut where the two sides' weights
// differ least; every symbol walks down from the root on its own (the cuts it computes are the ones its
// neighbours compute).  codes[row * 256 + symbol] = length << 27 | bits.  Weights are scaled to sum below
// 2^16 + sigma: no codeword is longer than kCodeMaxLen (checked: *err is raised otherwise).
__global__ __launch_bounds__(256) void k_code_build(const u32* __restrict__ cnt, u32 sigma, u32* __restrict__ codes,
                                                    u32* __restrict__ err) {
  __shared__ u32 s_pre[257];
  __shared__ u32 scr[256 / kWave + 1];
  const u32 row = blockIdx.x, b = threadIdx.x;
  u32 c = 0;
  if (b < sigma) {
    if (row < 256u) {
      for (u32 r = 0; r < kPairReplicas; ++r) c += cnt[(size_t)r * 65536u + row * 256u + b];
    } else {
      for (u32 a = 0; a < sigma; ++a)
        for (u32 r = 0; r < kPairReplicas; ++r) c += cnt[(size_t)r * 65536u + a * 256u + b];
    }
  }
  u32 total;
  (void)block_scan_excl_add<256>(c, scr, &total);
  u32 sh = 0;
  while ((total >> sh) >= 65536u) ++sh;
  const u32 wt = b < sigma ? (c >> sh) + 1u : 0u;
  u32 wtot;
  const u32 ex = block_scan_excl_add<256>(wt, scr, &wtot);
  s_pre[b] = ex;
  if (b == 255u) s_pre[256] = wtot;
  __syncthreads();
  if (b >= sigma) { codes[row * 256u + b] = 0u; return; }
  u32 lo = 0, hi = sigma, bits = 0, len = 0;
  while (hi - lo > 1u && len <= 31u) {
    const u64 mid2 = (u64)s_pre[lo] + (u64)s_pre[hi];
    u32 a = lo + 1u, z = hi - 1u;                       // smallest cut in [lo+1, hi-1] with 2 pre[cut] >= mid2, else hi-1
    while (a < z) { const u32 mdl = (a + z) >> 1; if (2ull * s_pre[mdl] >= mid2) z = mdl; else a = mdl + 1u; }
    u32 cut = a;
    if (cut > lo + 1u) {
      const u64 da = 2ull * s_pre[cut] >= mid2 ? 2ull * s_pre[cut] - mid2 : mid2 - 2ull * s_pre[cut];
      const u64 db = mid2 - 2ull * s_pre[cut - 1u];       // 2 pre[cut-1] < mid2
      if (db <= da) cut = cut - 1u;
    }
    if (b < cut) { hi = cut; bits <<= 1; } else { lo = cut; bits = (bits << 1) | 1u; }
    ++len;
  }
  if (len == 0u) len = 1u;                              // (an alphabet of one symbol)
  if (len > kCodeMaxLen) atomicOr(err, 2u);
  codes[row * 256u + b] = (len << 27) | bits;
}

// keys of a tile of 1024 suffixes (slots in descending suffix order as in k_make_keys); kbits = key bits in all
// (8 .. 72: the low 32 go to the second word w, the rest to the key word)
struct CodeKey {
  const u32* codes;              // k_code_build's table
  int kbits;                     // key bits in all (33 .. 72)
  int hi_shift, chr_shift, lvl_shift;   // key word: the upper bits of the suffix number (split items), the predecessor's code, the level
};
__global__ __launch_bounds__(256) void k_make_keys_code(const u8* __restrict__ T, const u8* __restrict__ lut,
                                                        u64* __restrict__ keys, u32* __restrict__ wout, u32 n,
                                                        u8* __restrict__ plane, int idx_hi, CodeKey ck) {
  constexpr u32 kTile = 1024;
  constexpr u32 kPos = 1280;                            // codeword positions a tile can hold (five per thread)
  __shared__ u8 s_lut[256];
  __shared__ u8 s_code[kTile + kCodeLA + 24];
  __shared__ u32 s_c0[256];                             // the order-0 row
  __shared__ u32 s_bp[kPos + 8];                        // bit offset of every position's codeword
  __shared__ u32 s_bits[(kPos * kCodeMaxLen) / 32 + 8];
  __shared__ u32 s_ends[(kPos * kCodeMaxLen) / 32 + 8];   // a one at every codeword's last bit
  __shared__ u64 s_key[kTile];
  __shared__ u32 s_w[kTile];
  __shared__ u32 scr[256 / kWave + 1];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  s_c0[threadIdx.x] = ck.codes[kCodeOrder0 * 256u + threadIdx.x];
  for (u32 i = threadIdx.x; i < (kPos * kCodeMaxLen) / 32 + 8; i += 256u) { s_bits[i] = 0u; s_ends[i] = 0u; }
  __syncthreads();
  const u32 J0 = blockIdx.x * kTile;
  if (J0 >= n) return;
  const u32 cntw = min(kTile, n - J0);
  const u32 i_base = n - J0 - cntw;
  const u32 pre = i_base > 0 ? 1u : 0u;
  const u32 span = cntw + kCodeLA + 2u;                 // positions 0 .. span-1 of the tile's stretch of T
  stage_codes(T, s_lut, s_code, i_base - pre, span + pre);
  __syncthreads();
  const u8* s_c = s_code + pre;                          // s_c[t] = code of T[i_base + t]
  // codewords of positions 1 .. span-1 (position t in the context of t-1), five consecutive ones per thread
  u32 cw[5];
  const u32 t0 = 1u + 5u * threadIdx.x;
#pragma unroll
  for (u32 e = 0; e < 5u; ++e) {
    const u32 t = t0 + e;
    cw[e] = t < span ? ck.codes[(u32)s_c[t - 1u] * 256u + (u32)s_c[t]] : 0u;
  }
  u32 lsum = 0;
#pragma unroll
  for (u32 e = 0; e < 5u; ++e) lsum += cw[e] >> 27;
  u32 total;
  u32 bp = block_scan_excl_add<256>(lsum, scr, &total);
#pragma unroll
  for (u32 e = 0; e < 5u; ++e) {
    const u32 t = t0 + e;
    const u32 len = cw[e] >> 27, code = cw[e] & 0x7FFFFFFu;
    if (t <= kPos) s_bp[t] = bp;
    if (len) {
      const u32 word = bp >> 5, off = bp & 31u;
      if (off + len <= 32u) atomicOr(&s_bits[word], code << (32u - off - len));
      else {
        const u32 r = off + len - 32u;                  // bits that spill into the next word
        atomicOr(&s_bits[word], code >> r);
        atomicOr(&s_bits[word + 1u], code << (32u - r));
      }
      const u32 last = bp + len - 1u;
      atomicOr(&s_ends[last >> 5], 0x80000000u >> (last & 31u));
    }
    bp += len;
  }
  if (threadIdx.x == 0) s_bp[0] = 0u;
  __syncthreads();
  const u32 o = 4u * threadIdx.x;
  if (o < cntw) {
    const u32 cnt = min(4u, cntw - o);
    for (u32 s = 0; s < cnt; ++s) {
      const u32 t = o + s;
      const u32 first = s_c0[s_c[t]];
      const u32 l0 = first >> 27;
      const u32 need = (u32)ck.kbits - l0;              // bits taken from the string, from position t+1 on
      const u32 start = s_bp[t + 1u];
      const u32 wi = start >> 5, off = start & 31u;
      const u64 a = ((u64)s_bits[wi] << 32) | (u64)s_bits[wi + 1u];
      const u64 bq = ((u64)s_bits[wi + 2u] << 32) | (u64)s_bits[wi + 3u];
      const u64 top = off ? (a << off) | (bq >> (64u - off)) : a;             // bits start .. start+63
      const u64 nxt = off ? (bq << off) : bq;                                // bits start+64 .. (at least 32 valid ones)
      // the first `need` bits (need <= 71) as a number
      u64 x_hi, x_lo;                                     // x = x_hi * 2^32 + (x_lo & 0xFFFFFFFF), x_lo = its low 32 bits
      if (need <= 64u) {
        const u64 x = need ? top >> (64u - need) : 0ull;
        x_hi = x >> 32; x_lo = x & 0xFFFFFFFFull;
      } else {
        const u32 extra = need - 64u;                     // 1 .. 7 bits of nxt
        const u64 lowpart = nxt >> (64u - extra);
        x_lo = ((top << extra) | lowpart) & 0xFFFFFFFFull;
        x_hi = (top >> (32u - extra));                    // top's upper bits: x >> 32
      }
      // key = first codeword * 2^need + x
      const u64 fc = (u64)(first & 0x7FFFFFFu);
      u64 k_hi, k_lo;                                     // key >> 32, key & 0xFFFFFFFF
      if (need >= 32u) { k_lo = x_lo; k_hi = x_hi | (fc << (need - 32u)); }
      else { const u64 full = (fc << need) | ((x_hi << 32) | x_lo); k_lo = full & 0xFFFFFFFFull; k_hi = full >> 32; }
      // complete codewords in the key: the first character, and the codewords that end inside bits [start, start + need)
      const u64 ea = ((u64)s_ends[wi] << 32) | (u64)s_ends[wi + 1u];
      const u64 eb = ((u64)s_ends[wi + 2u] << 32) | (u64)s_ends[wi + 3u];
      const u64 etop = off ? (ea << off) | (eb >> (64u - off)) : ea;
      u32 k = 1u;
      if (need <= 64u) k += need ? (u32)__popcll(etop >> (64u - need)) : 0u;
      else k += (u32)__popcll(etop) + (u32)__popcll((off ? (eb << off) : eb) >> (128u - need));
      const u32 i = i_base + t;
      u64 key = k_hi;
      key |= (u64)(i ? (u32)s_c[(int)t - 1] : 0u) << ck.chr_shift;
      key |= (u64)code_level_of(k) << ck.lvl_shift;
      s_key[cntw - 1u - t] = key;
      s_w[cntw - 1u - t] = (u32)k_lo;
    }
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < cntw; j += 256u) {
    u64 key = s_key[j];
    if (idx_hi) key |= (u64)((n - 1u - (J0 + j)) >> 16) << ck.hi_shift;
    keys[J0 + j] = key;
    const u32 w = s_w[j];
    wout[J0 + j] = w;
    if (plane) plane[J0 + j] = (u8)w;
  }
}

// ---------------------------------------------------------------------------------------
// K4  re-ranking of a sorted list (INIT: the whole SA after the initial sort; rounds: the
//     active list after sorting by (group, rank[s+h]), keys u64).
//
//     head[p]   = p starts a new group (key differs from p-1; INIT: or p-1 is no longer
//                 than the key, which makes it a finished singleton)
//     active[p] = p's group has >= 2 members
//     new rank of p = global SA slot of its group head
//     finished suffixes go to SA; active ones are compacted (order kept) into the next
//     active list with their global slot and a dense group number.
//     Three launches: tile reduce, one-workgroup scan of the tile aggregates, tile apply.
//
//     Every wave owns 512 consecutive list slots and walks them 64 at a time (coalesced).
//     Flags become 64-bit ballots, so every prefix inside the wave is a popcount of a
//     masked ballot and the running sums live in scalar registers; only the four wave
//     totals of a tile cross LDS.
// ---------------------------------------------------------------------------------------
constexpr int kRrTPB = 256;
constexpr int kRrWaves = kRrTPB / kWave;
constexpr int kRrE = 8;
constexpr int kRrChunk = kWave * kRrE;        // slots per wave
constexpr int kRrTile = kRrTPB * kRrE;        // slots per workgroup

__device__ __forceinline__ u64 shfl_up1(u64 v) {
  return (u64)__shfl_up((unsigned long long)v, 1, kWave);
}
__device__ __forceinline__ u32 shfl_up1(u32 v) { return __shfl_up(v, 1, kWave); }
__device__ __forceinline__ u64 shfl_down1(u64 v) {
  return (u64)__shfl_down((unsigned long long)v, 1, kWave);
}
__device__ __forceinline__ u32 shfl_down1(u32 v) { return __shfl_down(v, 1, kWave); }

template <typename K, bool INIT>
struct RrMasks {
  u64 head[kRrE], act[kRrE], valid[kRrE];
  u32 sfx[kRrE];       // idx[p] of this lane's slot in iteration e
  u32 chr[kRrE];       // bits 56..63 of its key (the carried character, when there is one)
};

__device__ __forceinline__ u64 lane_value(u64 v, int l) { return (u64)__shfl((unsigned long long)v, l, kWave); }
__device__ __forceinline__ u32 lane_value(u32 v, int l) { return __shfl(v, l, kWave); }

// Masks of one wave chunk starting at list slot wbase.  All of the chunk's keys and suffixes are
// loaded before anything is compared (one iteration at a time, each with its own neighbour
// loads, was eight memory latencies in a row per wave); the neighbours across an iteration's ends
// are the adjacent iterations' end lanes, and only the two slots next to the whole chunk are
// loaded on their own.
// LONG (initial ranking after the long-key sort, radix_sort_long): a suffix's order key is (key & kmask,
// w & wmask); the upper bits of its number sit at hi_shift, its predecessor character's code at chr_shift.
// wmask: the bits of w the sort ordered by.  How many characters the members of a group are known to share: code keys
// carry a 3-bit level at lvl_shift (code_level_depth); gram keys (lvl_shift < 0) all share `depth`.  It rides to the
// finisher in the upper byte of the list entry's 16-bit character field.
struct RrLong { const u32* w; u32 wmask; int hi_shift; int chr_shift; u32 chr_mask; int lvl_shift; u32 depth; };


template <typename K, bool INIT, bool SPLIT, bool LONG = false>
__device__ __forceinline__ void rr_masks(const K* __restrict__ key, const u32* __restrict__ idx,
                                         u32 m, u32 n, u32 short_len, K kmask, u32 wbase, u32 lane,
                                         RrMasks<K, INIT>& f, RrLong lg = RrLong()) {
  // SPLIT (initial ranking of 64-bit keys only): a suffix number's upper bits sit in bits 48.. of
  // its key and idx[] holds 16-bit lower halves (the sort moved 10 bytes per item instead of 12)
  auto suffix_of = [&](K kraw, u32 word, u32 p) -> u32 {     // the 16-bit half out of its aligned word (two lanes per word)
    if (sizeof(K) == 8 && SPLIT) {
      const u32 hi = LONG ? ((u32)((u64)kraw >> lg.hi_shift) & 0x1FFFu) : (u32)((u64)kraw >> 48);
      return (hi << 16) | ((p & 1u) ? word >> 16 : word & 0xFFFFu);
    }
    return word;
  };
  K kc[kRrE];
  u32 wc[LONG ? kRrE : 1] = {};
  {
    K kraw[kRrE];
    u32 word[kRrE];
#pragma unroll
    for (int e = 0; e < kRrE; ++e) {               // nothing but loads: sixteen in flight
      const u32 p = wbase + e * kWave + lane;
      const bool ok = p < m;
      kraw[e] = ok ? key[p] : (K)0;
      word[e] = ok ? idx[(sizeof(K) == 8 && SPLIT) ? p >> 1 : p] : 0u;
      if (LONG) wc[LONG ? e : 0] = ok ? lg.w[p] : 0u;
    }
#pragma unroll
    for (int e = 0; e < kRrE; ++e) {
      const u32 p = wbase + e * kWave + lane;
      f.sfx[e] = p < m ? suffix_of(kraw[e], word[e], p) : 0u;
      f.chr[e] = LONG ? ((u32)((u64)kraw[e] >> lg.chr_shift) & lg.chr_mask) : sizeof(K) == 8 ? (u32)((u64)kraw[e] >> 56) : 0u;
      if (LONG) {                                   // the depth its group is known to share, above the character's code
        f.chr[e] |= (lg.lvl_shift >= 0 ? code_level_depth((u32)((u64)kraw[e] >> lg.lvl_shift) & 7u) : lg.depth) << 8;
        wc[LONG ? e : 0] &= lg.wmask;
      }
      kc[e] = kraw[e] & kmask;
    }
  }
  K before = (K)0, after = (K)0;          // slots wbase - 1 and wbase + chunk (where they exist)
  u32 ibefore = 0u, wbefore = 0u, wafter = 0u;
  if (lane == 0 && wbase > 0 && wbase < m) {
    const K braw = key[wbase - 1];
    before = braw & kmask;
    if (LONG) wbefore = lg.w[wbase - 1] & lg.wmask;
    if (INIT) ibefore = suffix_of(braw, idx[(sizeof(K) == 8 && SPLIT) ? (wbase - 1) >> 1 : wbase - 1], wbase - 1);
  }
  if (lane == kWave - 1 && wbase + (u32)kRrChunk < m) {
    after = key[wbase + kRrChunk] & kmask;
    if (LONG) wafter = lg.w[wbase + kRrChunk] & lg.wmask;
  }
#pragma unroll
  for (int e = 0; e < kRrE; ++e) {
    const u32 p = wbase + e * kWave + lane;
    const bool ok = p < m;
    const u32 ic = f.sfx[e];
    K kp = shfl_up1(kc[e]);
    K kn = shfl_down1(kc[e]);
    u32 ip = shfl_up1(ic);
    const K kprev_end = e > 0 ? lane_value(kc[e > 0 ? e - 1 : 0], kWave - 1) : before;
    const u32 iprev_end = e > 0 ? lane_value(f.sfx[e > 0 ? e - 1 : 0], kWave - 1) : ibefore;
    const K knext_first = e + 1 < kRrE ? lane_value(kc[e + 1 < kRrE ? e + 1 : e], 0) : after;
    if (lane == 0) { kp = (ok && p > 0) ? kprev_end : (K)0; if (INIT) ip = (ok && p > 0) ? iprev_end : 0u; }
    if (lane == kWave - 1) kn = (p + 1 < m) ? knext_first : (K)0;
    bool wdiff_p = false, wdiff_n = false;           // LONG: the second key word differs from the neighbour's
    if (LONG) {
      const u32 wme = wc[LONG ? e : 0];
      u32 wp = shfl_up1(wme), wn = shfl_down1(wme);
      const u32 wprev_end = e > 0 ? lane_value(wc[LONG && e > 0 ? e - 1 : 0], kWave - 1) : wbefore;
      const u32 wnext_first = e + 1 < kRrE ? lane_value(wc[LONG && e + 1 < kRrE ? e + 1 : 0], 0) : wafter;
      if (lane == 0) wp = (ok && p > 0) ? wprev_end : 0u;
      if (lane == kWave - 1) wn = (p + 1 < m) ? wnext_first : 0u;
      wdiff_p = wme != wp;
      wdiff_n = wme != wn;
    }
    bool h = ok && (p == 0 || kc[e] != kp || wdiff_p);
    // (long items: a suffix is known to lie inside its key when it is no longer than the key's depth; equal keys
    // have equal depths, so the slot before counts with this one's)
    const u32 sl = LONG ? f.chr[e] >> 8 : short_len;
    if (INIT) h = h || (ok && p > 0 && (u64)ip + sl >= (u64)n);
    bool hn = (p + 1 >= m) || kn != kc[e] || wdiff_n;         // is p+1 a head (or past the end)?
    if (INIT) hn = hn || ((u64)ic + sl >= (u64)n);
    f.head[e] = __ballot(h);
    f.valid[e] = __ballot(ok);
    f.act[e] = __ballot(ok && (!h || !hn));
  }
}

__device__ __forceinline__ u32 top_bit(u64 v) { return 63u - (u32)__clzll((unsigned long long)v); }

template <typename K, bool INIT, bool SPLIT = false, bool LONG = false>
__global__ __launch_bounds__(kRrTPB) void k_rerank_reduce(const K* __restrict__ key,
                                                          const u32* __restrict__ idx, u32 m,
                                                          u32 n, u32 short_len, K kmask,
                                                          u32* __restrict__ aggA,
                                                          u32* __restrict__ aggB,
                                                          u32* __restrict__ aggC, RrLong lg = RrLong()) {
  __shared__ u32 s_tot[3][kRrWaves];
  const u32 lane = lane_id();
  const u32 wave = threadIdx.x / kWave;
  const u32 wbase = blockIdx.x * kRrTile + wave * kRrChunk;
  RrMasks<K, INIT> f;
  rr_masks<K, INIT, SPLIT, LONG>(key, idx, m, n, short_len, kmask, wbase, lane, f, lg);
  u32 nact = 0, nha = 0, last = 0;
#pragma unroll
  for (int e = 0; e < kRrE; ++e) {
    nact += (u32)__popcll(f.act[e]);
    nha += (u32)__popcll(f.act[e] & f.head[e]);
    if (f.head[e]) last = wbase + e * kWave + top_bit(f.head[e]) + 1u;
  }
  if (lane == 0) { s_tot[0][wave] = nact; s_tot[1][wave] = nha; s_tot[2][wave] = last; }
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 a = 0, b = 0, c = 0;
    for (int w = 0; w < kRrWaves; ++w) { a += s_tot[0][w]; b += s_tot[1][w]; c = max(c, s_tot[2][w]); }
    aggA[blockIdx.x] = a; aggB[blockIdx.x] = b; aggC[blockIdx.x] = c;
  }
}

// Exclusive sum of aggA, aggB; exclusive max of aggC; totals -> counts[0..1].  A workgroup of 16
// waves owns 4096 consecutive entries, a wave 256 of them (four coalesced rows of 64, their twelve
// loads in flight together).  PHASE 0 leaves every workgroup's totals in part[]; PHASE 1 adds up the
// parts before it and scans its entries with that carried in.  (One workgroup walking all 131 072
// tile aggregates of a 256 MiB block took 107-168 us, three times per block, with the GPU idle beside it.)
constexpr u32 kRrScanChunk = 4096;
template <int PHASE>
__global__ __launch_bounds__(1024) void k_rerank_scan_tiles(u32* __restrict__ aggA,
                                                            u32* __restrict__ aggB,
                                                            u32* __restrict__ aggC, u32 ntiles,
                                                            u32* __restrict__ part,
                                                            u32* __restrict__ counts) {
  __shared__ u32 s_tot[3][16];
  __shared__ u32 s_base[3];
  const u32 lane = lane_id();
  const u32 wave = threadIdx.x / kWave;
  const u32 b = blockIdx.x * kRrScanChunk + wave * 256u;
  const u32 e = min(b + 256u, ntiles);
  u32 va[4], vb[4], vc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const u32 i = b + (u32)r * kWave + lane;
    const bool ok = i < e;
    va[r] = ok ? aggA[i] : 0u; vb[r] = ok ? aggB[i] : 0u; vc[r] = ok ? aggC[i] : 0u;
  }
  u32 sa = 0, sb = 0, sc = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) { sa += va[r]; sb += vb[r]; sc = max(sc, vc[r]); }
  sa = wave_scan_add(sa, lane); sb = wave_scan_add(sb, lane); sc = wave_scan_max(sc, lane);
  if (lane == kWave - 1) { s_tot[0][wave] = sa; s_tot[1][wave] = sb; s_tot[2][wave] = sc; }
  if (PHASE == 1 && wave == 0) {
    // what the workgroups before this one hold (at most a few hundred parts), and the totals
    u32 pa = 0, pb = 0, pc = 0, ta = 0, tb = 0;
    for (u32 g = lane; g < gridDim.x; g += kWave) {
      const u32 x = part[3u * g], y = part[3u * g + 1u], z = part[3u * g + 2u];
      ta += x; tb += y;
      if (g < blockIdx.x) { pa += x; pb += y; pc = max(pc, z); }
    }
    pa = wave_scan_add(pa, lane); pb = wave_scan_add(pb, lane); pc = wave_scan_max(pc, lane);
    ta = wave_scan_add(ta, lane); tb = wave_scan_add(tb, lane);
    if (lane == kWave - 1) {
      s_base[0] = pa; s_base[1] = pb; s_base[2] = pc;
      if (blockIdx.x == 0) { counts[0] = ta; counts[1] = tb; }
    }
  }
  __syncthreads();
  if (PHASE == 0) {
    if (threadIdx.x == 0) {
      u32 ta = 0, tb = 0, tc = 0;
      for (u32 w = 0; w < 16; ++w) { ta += s_tot[0][w]; tb += s_tot[1][w]; tc = max(tc, s_tot[2][w]); }
      part[3u * blockIdx.x] = ta; part[3u * blockIdx.x + 1u] = tb; part[3u * blockIdx.x + 2u] = tc;
    }
    return;
  }
  u32 ca = s_base[0], cb = s_base[1], cc = s_base[2];
  for (u32 w = 0; w < wave; ++w) { ca += s_tot[0][w]; cb += s_tot[1][w]; cc = max(cc, s_tot[2][w]); }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const u32 i = b + (u32)r * kWave + lane;
    const u32 ia = wave_scan_add(va[r], lane), ib = wave_scan_add(vb[r], lane), ic = wave_scan_max(vc[r], lane);
    const u32 pc = __shfl_up(ic, 1, kWave);
    if (i < e) {
      aggA[i] = ca + ia - va[r];
      aggB[i] = cb + ib - vb[r];
      aggC[i] = max(cc, lane ? pc : 0u);
    }
    ca += __shfl(ia, kWave - 1, kWave);
    cb += __shfl(ib, kWave - 1, kWave);
    cc = max(cc, __shfl(ic, kWave - 1, kWave));
  }
}

// PAIRS: instead of scattering rank[s] = nr from here (one random 4-byte write per element,
// each costing a whole HBM sector), emit (s, nr) in list order; the caller partitions the
// pairs by the high bits of s and k_scatter_pairs then writes into one small window of
// rank[] at a time.
//
// MODE: how the new ranks reach rank[] and how the next round gets its list.
//   0  rank[s] = nr written from here (short lists); active list compacted (aidx/aglob/agrp)
//   1  (s, nr) pairs in list order for scatter_rank_pairs; active list compacted
//   2  "dense" (most of the list stays active): one record per slot for the window-ordered
//      route -- tri_key[p] = s << 32 | nr, tri_val[p] = new dense group number, or all ones for
//      a finished suffix -- and only aglob of the active list is compacted.  The records are
//      partitioned by the high bits of s; k_scatter_dense then updates rank[] one window at a
//      time and k_gather_dense builds the next round's sort keys from the same records, reading
//      rank[s+h] (and T[s-1]) inside one window instead of at random (bwt_engine.hip, host side).
//
// EMIT: the transform's bytes leave from here instead of from a gather over the finished
// suffix array.  1: the character rides in bits 56..63 of the round's key (k_gather_key2 /
// k_gather_dense put it there: a round's key has at most 56 bits, can_carry()); 2 (initial
// ranking: its keys have no room): it is read from T[s-1] here.  A suffix that becomes final
// writes out[slot] (slot out_n, which only exists in block mode, goes to *last_char; the slot
// of suffix 0 is the end-of-block row, *pidx); one that stays active hands its character on in
// achr_out (not in MODE 2: k_gather_dense reads it again, inside a window).  SA is only
// written when somebody wants it (SA != nullptr).
struct RrEmit {
  u8* out; u32 out_n; u32* last_char; u32* pidx; const u8* T; u8* achr_out;
  u8* rec_plane; int rec_shift;      // MODE 2: digit (s >> rec_shift) & 255 of every record, for the window partition's first pass
  const u8* inv_lut;                 // EMIT 3: dense code -> byte (the character rides in the long key as its code)
  // LF powers noted as suffixes become final (the routes that never complete rank[]):
  // LF[k] = slot of suffix n - k x, k = 1 .. lf_n - 1 (divsufsort.c:337-338,350,381,390); lf_inv = floor(2^32 / x)
  u32* lf; u32 lf_n, lf_x, lf_inv;
};

// Suffix s became final at `slot`: is it one of the sampled ones?
__device__ __forceinline__ void lf_note(const RrEmit& em, u32 n, u32 s, u32 slot) {
  if (em.lf_n <= 1u) return;
  const u32 t = n - s;                                  // 1 .. n
  u32 q = em.lf_x > 1u ? __umulhi(t, em.lf_inv) : t;    // floor(t / x) or one less (x = 1: a block of a few hundred bytes with 256 powers)
  u32 r = t - q * em.lf_x;
  if (r == em.lf_x) { r = 0u; ++q; }
  if (r == 0u && q >= 1u && q < em.lf_n) em.lf[q] = slot;
}

//   3  (finisher route, after the long-key sort) nothing goes to rank[]: finished suffixes leave
//      (out, SA, LF powers), the others are compacted into the list the finisher works on --
//      suffix, slot, slot of the group's head, character.
// EMIT 3: the character's dense code rides in the long key (RrLong::chr_shift); em.inv_lut turns it back.
template <typename K, bool INIT, int MODE, int EMIT, bool SPLIT = false, bool LONG = false>
__global__ __launch_bounds__(kRrTPB) void k_rerank_apply(
    const K* __restrict__ key, const u32* __restrict__ idx, const u32* __restrict__ aglob, u32 m,
    u32 n, u32 short_len, K kmask, const u32* __restrict__ aggA, const u32* __restrict__ aggB,
    const u32* __restrict__ aggC, u32* __restrict__ rank, u32* __restrict__ SA,
    u32* __restrict__ aidx_out, u32* __restrict__ aglob_out, u32* __restrict__ agrp_out,
    u32* __restrict__ pair_s, u32* __restrict__ pair_r, RrEmit em, RrLong lg = RrLong()) {
  __shared__ u32 s_tot[3][kRrWaves];
  __shared__ u8 s_inv[EMIT == 3 ? 256 : 4];
  if (EMIT == 3) s_inv[threadIdx.x] = em.inv_lut[threadIdx.x];     // kRrTPB == 256
  const u32 lane = lane_id();
  const u32 wave = threadIdx.x / kWave;
  const u32 wbase = blockIdx.x * kRrTile + wave * kRrChunk;
  RrMasks<K, INIT> f;
  rr_masks<K, INIT, SPLIT, LONG>(key, idx, m, n, short_len, kmask, wbase, lane, f, lg);
  {
    u32 nact = 0, nha = 0, last = 0;
#pragma unroll
    for (int e = 0; e < kRrE; ++e) {
      nact += (u32)__popcll(f.act[e]);
      nha += (u32)__popcll(f.act[e] & f.head[e]);
      if (f.head[e]) last = wbase + e * kWave + top_bit(f.head[e]) + 1u;
    }
    if (lane == 0) { s_tot[0][wave] = nact; s_tot[1][wave] = nha; s_tot[2][wave] = last; }
  }
  __syncthreads();
  u32 q_run = aggA[blockIdx.x], g_run = aggB[blockIdx.x], hp_run = aggC[blockIdx.x];
  for (u32 w = 0; w < wave; ++w) {
    q_run += s_tot[0][w]; g_run += s_tot[1][w]; hp_run = max(hp_run, s_tot[2][w]);
  }
  const u64 lt = (1ull << lane) - 1ull;
  const u64 le = lt | (1ull << lane);
  // first every load of the chunk (global slots, new ranks, characters), then the stores
  u32 gs[kRrE], nrs[kRrE], grps[kRrE], qs[kRrE], cs[kRrE];
#pragma unroll
  for (int e = 0; e < kRrE; ++e) {
    const u32 base = wbase + e * kWave;
    const u32 p = base + lane;
    const u64 hd = f.head[e], ac = f.act[e];
    gs[e] = 0; nrs[e] = 0; grps[e] = 0; qs[e] = 0; cs[e] = 0;
    if ((f.valid[e] >> lane) & 1ull) {
      const bool a = (ac >> lane) & 1ull;
      const u64 hm = hd & le;
      const u32 hp1 = hm ? base + top_bit(hm) + 1u : hp_run;   // head slot + 1
      const u32 s = f.sfx[e];
      gs[e] = INIT ? p : aglob[p];
      nrs[e] = INIT ? hp1 - 1u : aglob[hp1 - 1u];
      grps[e] = g_run + (u32)__popcll(ac & hd & le) - 1u;      // dense number of p's group (if active)
      qs[e] = q_run + (u32)__popcll(ac & lt);
      if (EMIT == 1) cs[e] = f.chr[e];
      if (EMIT == 2 && (!a || MODE != 2)) cs[e] = s ? em.T[s - 1u] : 0u;
      if (EMIT == 3) cs[e] = s_inv[f.chr[e] & 0xFFu];
    }
    q_run += (u32)__popcll(ac);
    g_run += (u32)__popcll(ac & hd);
    if (hd) hp_run = base + top_bit(hd) + 1u;
  }
#pragma unroll
  for (int e = 0; e < kRrE; ++e) {
    const u32 p = wbase + e * kWave + lane;
    if ((f.valid[e] >> lane) & 1ull) {
      const bool a = (f.act[e] >> lane) & 1ull;
      const u32 s = f.sfx[e], g = gs[e], nr = nrs[e], grp = grps[e], c = cs[e];
      if (MODE == 2) {
        reinterpret_cast<u64*>(pair_s)[p] = ((u64)s << 32) | (u64)nr;
        pair_r[p] = a ? grp : 0xFFFFFFFFu;
        if (em.rec_plane) em.rec_plane[p] = (u8)(s >> em.rec_shift);
      } else if (MODE == 1) { pair_s[p] = s; pair_r[p] = nr; }
      else if (MODE == 0) { if (rank) rank[s] = nr; }
      if (a) {
        const u32 q = qs[e];
        aglob_out[q] = g;
        if (MODE != 2) {
          aidx_out[q] = s;
          agrp_out[q] = MODE == 3 ? nr : grp;
          if (MODE == 3) reinterpret_cast<unsigned short*>(em.achr_out)[q] = (unsigned short)(c | (f.chr[e] & 0xFF00u));   // character, known depth
          else if (EMIT) em.achr_out[q] = (u8)c;
        }
      } else {
        if (SA) SA[g] = s;
        if (EMIT) {
          if (s == 0u) *em.pidx = g;
          if (g < em.out_n) em.out[g] = (u8)c;
          else *em.last_char = c;
          lf_note(em, n, s, g);                    // nothing unless the caller asked for notes (lf_n)
        }
      }
    }
  }
}


// ---------------------------------------------------------------------------------------
// Finisher (after the long-key sort): the suffixes that are still tied form groups -- contiguous in
// slot order -- whose members are known to share `depth` characters (a number every list entry
// carries: code keys cover more characters of a frequent string than of a rare one).  Prefix doubling
// would first have to complete rank[] for ALL suffixes (an ISA scatter of the whole block) before it
// could look at rank[s+h]; here a group is settled by comparing its members' next kFinChars characters
// directly.  The list entry of a suffix is (suffix, slot, slot of its group's head, predecessor
// character | depth << 8).
//
// A workgroup looks at a window of kFinWin consecutive entries and owns the groups that START in its
// first kFinWin - kFinMaxGroup entries and have at most kFinMaxGroup members (so they lie inside the
// window).  It stages the owned members' characters in LDS (the route's one random access: three
// aligned words of T per member) and every member counts the members of its group below it and equal
// to it.  (Round 5 also measured a bitonic network over the window instead of that loop -- 55 steps
// whatever the groups look like: 87 ps per entry on a real text whose groups average 34 members,
// against about 25 for the loop, whose cost is the group's size; the network was dropped.)
// A member without equals is final: out[slot], SA[slot], the LF powers.  The others form the next list
// in their new order (sub-group head = old head + members below), sixteen characters deeper, appended
// with one atomic per workgroup.
//
// Larger groups are nobody's: their entries go to the "hard" list, appended by the workgroup whose
// stride range they lie in, and take the text rounds / doubling rounds (bridge, below).
// "Proper prefix sorts first": characters past the end of T compare as zero bytes, and of two members
// that are equal under that rule and of which one reaches past the end, the shorter (larger suffix
// number) is the smaller -- they are never equal (the network's comparison knows).
// ---------------------------------------------------------------------------------------
#ifndef BWTC_FIN_TPB
#define BWTC_FIN_TPB 256
#endif
constexpr int kFinTPB = BWTC_FIN_TPB;             // threads of a finisher workgroup; a window is 1024 or 2048 entries
constexpr int kFinE1 = 1024 / kFinTPB, kFinE2 = 2048 / kFinTPB;   // entries per thread
constexpr u32 kFinNone = 0xFFFFFFFFu;

struct FinList { u32* S; u32* P; u32* H; unsigned short* C; };
// A list lives in up to kFinRegions regions of its arrays (a pass appends what it leaves with one atomic per workgroup:
// 300 000 workgroups on ONE counter were 3.4 ms of serialised atomics per pass over a real text, so workgroup b appends to
// one of 16 regions, each with a counter of its own: chunks of 64 consecutive workgroups take the regions in turn -- the
// workgroups on the chip at any moment spread over all of them, and a chunk leaves at most its 64 strides of entries plus
// one group, so the regions' sizes add up to the list's plus half a per cent).  Windows never straddle regions (groups
// do not: a workgroup's output goes to one region).
constexpr u32 kFinChunk = 64;             // (kFinRegions, FinRegions: bwt_engine.hpp)
struct FinOut { u32 base[kFinRegions]; };                 // where each region of the list a pass leaves starts

// sixteen characters T[pos .. pos+16) as two big-endian words; bytes at or past n read as zero
__device__ __forceinline__ void fin_chars(const u8* __restrict__ T, u32 pos, u32 n, u64* c0, u64* c1) {
  *c0 = 0; *c1 = 0;
  if (pos >= n) return;
  const u64* a = reinterpret_cast<const u64*>(T + (pos & ~7u));      // T is 256-byte aligned and padded
  const u32 sh = (pos & 7u) * 8u;
  const u64 w0 = a[0], w1 = a[1], w2 = a[2];
  u64 lo = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0;               // bytes pos .. pos+7, first byte lowest
  u64 hi = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
  const u32 left = n - pos;                                          // real bytes from pos on
  if (left < 16u) {
    if (left <= 8u) { hi = 0; if (left < 8u) lo &= (1ull << (8u * left)) - 1ull; }
    else hi &= (1ull << (8u * (left - 8u))) - 1ull;
  }
  *c0 = __builtin_bswap64(lo);
  *c1 = __builtin_bswap64(hi);
}

// 8 NW characters T[pos .. pos + 8 NW) as NW big-endian words; bytes at or past n read as zero
template <int NW>
__device__ __forceinline__ void fin_chars_n(const u8* __restrict__ T, u32 pos, u32 n, u64 (&c)[NW]) {
#pragma unroll
  for (int q = 0; q < NW; ++q) c[q] = 0;
  if (pos >= n) return;
  const u64* a = reinterpret_cast<const u64*>(T + (pos & ~7u));      // T is 256-byte aligned and padded
  const u32 sh = (pos & 7u) * 8u;
  u64 w[NW + 1];
#pragma unroll
  for (int q = 0; q <= NW; ++q) w[q] = a[q];
  const u32 left = n - pos;                                          // real bytes from pos on
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    u64 v = sh ? (w[q] >> sh) | (w[q + 1] << (64u - sh)) : w[q];     // bytes pos + 8 q .. + 7, first byte lowest
    if (left < 8u * (u32)(q + 1)) v = left <= 8u * (u32)q ? 0ull : v & ((1ull << (8u * (left - 8u * (u32)q))) - 1ull);
    c[q] = __builtin_bswap64(v);
  }
}

// The finisher's comparison loop: how many members of the group at window positions [a, jend) are below the member at
// position lp, whose key is k (NW big-endian words)?  Four members per step, their LDS reads issued together (one member
// per step was a chain of LDS latencies); positions past the group's end are read (inside the arrays: they are padded)
// and not counted.  any_touch (the same for the whole workgroup): some member reaches past the end of T -- "proper
// prefix sorts first": characters past the end compare as zero bytes, and of two members equal under that rule of which
// one reaches past the end the shorter -- the larger suffix number -- is the smaller; they are never equal.
template <int NW>
__device__ __forceinline__ u32 fin_count_below(const u64* s_ch, const u32* s_S, u32 a, u32 jend, u32 lp, u32 sfx,
                                               const u64 (&k)[NW], bool any_touch) {
  u32 below = 0;
  if (!any_touch) {
    for (u32 j0 = a; j0 < jend; j0 += 4u) {
      u64 dd[4][NW];
#pragma unroll
      for (u32 u = 0; u < 4u; ++u) {
#pragma unroll
        for (int q = 0; q < NW; ++q) dd[u][q] = s_ch[(u32)NW * (j0 + u) + (u32)q];
      }
      // (no short cuts: with `||` and `&&` the compiler made the second word's read and comparison a branch per
      // member -- four dependent LDS round trips a step)
#pragma unroll
      for (u32 u = 0; u < 4u; ++u) {
        u32 lt = (u32)(dd[u][NW - 1] < k[NW - 1]);
#pragma unroll
        for (int q = NW - 2; q >= 0; --q) lt = (u32)(dd[u][q] < k[q]) | ((u32)(dd[u][q] == k[q]) & lt);
        below += lt & (u32)(j0 + u < jend);
      }
    }
  } else {
    const u32 me = s_S[lp];
    for (u32 j = a; j < jend; ++j) {
      const u32 sj = s_S[j];
      bool lt = false, eq = true;
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const u64 d = s_ch[(u32)NW * j + (u32)q];
        lt = lt || (eq && d < k[q]);
        eq = eq && d == k[q];
      }
      if (eq && ((sj | me) >> 31) && j != lp) lt = (sj & 0x7FFFFFFFu) > sfx;
      below += lt ? 1u : 0u;
    }
  }
  return below;
}

// hard_count[0]: entries of the hard list, [1]: the smallest depth among them.  Hard entries whose group shares fewer
// than shal.floor characters go to a list of their own (shal.count[0], [1]: entries, smallest depth): the rounds work
// at ONE depth for all their groups, the smallest, and a few groups of some exotic but repetitive string (bytes the
// code's sample never saw: a depth of one or two characters) would drag a whole text's hard groups down to theirs.
struct FinShallow { u32* S; u64* HP; u32* count; u32 floor; };
// RANK (FinRank rk; NW == 2): the members' keys are not characters but ranks -- rank[s + at] (and rank[s + at2]), the
// doubling step of Larsson and Sadakane done group by group in LDS instead of by a global sort of (group, rank): for the
// many small groups of deep repeats (copies of whole files).  rank[] must not change while a pass reads it, so the
// pass only NOTES every member's new rank (its slot when final, else its sub-group's head), by list position, and
// k_rank_updates writes them afterwards.
struct FinRank { const u32* rank; u32 at, at2; u32* us; u32* ur; };   // at2 == 0: one look-up
// NR (characters only; RANK: 1): the rounds of 8 NW characters a pass makes -- the members that a round leaves tied are
// compared again, sub-group by sub-group, without leaving the workgroup.  (A template parameter: with the rounds
// unrolled the kernel needs 30 registers less than with a loop over them, a workgroup more per CU.)
#ifdef BWTC_FIN_WAVES
#define BWTC_FIN_BOUNDS __launch_bounds__(kFinTPB, BWTC_FIN_WAVES)
#else
#define BWTC_FIN_BOUNDS __launch_bounds__(kFinTPB)
#endif
template <int kFinMaxGroup, int E_ = 4, int NW = 2, bool RANK = false, int NR = 1>
__global__ BWTC_FIN_BOUNDS void k_finish(FinList in, FinRegions rg, const u8* __restrict__ T, u32 n,
                                                    FinList next, FinOut ob, u32* __restrict__ next_count,
                                                    u32* __restrict__ hardS, u64* __restrict__ hardHP, unsigned short* __restrict__ hardC,
                                                    u32* __restrict__ hard_count, FinShallow shal, u32* __restrict__ SA, RrEmit em,
                                                    FinRank rk = FinRank()) {
  static_assert(!RANK || (NW == 2 && NR == 1), "rank keys are two words, one round");
  constexpr u32 nr = NR;
  constexpr int kFinE = E_;                                           // entries per thread: a window of 1024 or 2048
  constexpr int kFinWin = kFinTPB * kFinE;
  static_assert(kFinMaxGroup < kFinWin, "a group must fit the window");
  constexpr int kFinStride = kFinWin - kFinMaxGroup;                  // entries whose groups a workgroup owns
  constexpr u32 kChars = 8u * NW * NR;                                // characters compared by this pass
  __shared__ __attribute__((aligned(16))) u64 s_ch[(kFinWin + 4) * NW];   // the characters (+ padding for the comparison loop's reads); later the reorder staging
  __shared__ u32 s_S[kFinWin + 4];                                    // suffix | reaches past the end << 31
  __shared__ u32 s_H[kFinWin];
  __shared__ unsigned short s_g[kFinWin + 2];                         // group size by start position; [kFinWin]: the group cut by the window's start
  __shared__ u32 s_cnt2[NR > 1 ? kFinWin : 1];                        // the sub-group counters of the odd rounds (the even ones': s_H's bytes)
  __shared__ u32 scr[kFinTPB / kWave + 1];
  __shared__ u32 s_base;
  u32* st_S = reinterpret_cast<u32*>(s_ch);                           // staging, by new position
  u32* st_P = st_S + kFinWin;
  u32* st_H = st_P + kFinWin;                                         // | final << 31
  unsigned short* st_C = reinterpret_cast<unsigned short*>(st_H + kFinWin);
  const u32 tid = threadIdx.x;
  u32 reg = 0;
  while (reg + 1u < rg.nreg && blockIdx.x >= rg.wfirst[reg + 1u]) ++reg;
  const u32 w0 = rg.ebase[reg] + (blockIdx.x - rg.wfirst[reg]) * (u32)kFinStride;
  const u32 m = rg.ebase[reg] + rg.ecount[reg];                       // one past the region's last entry
  const u32 lane = lane_id();

  u32 S[kFinE], P[kFinE], H[kFinE], C[kFinE];
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    const u32 lp = tid + (u32)e * kFinTPB, q = w0 + lp;
    const bool ok = q < m;
    S[e] = ok ? in.S[q] : 0u; P[e] = ok ? in.P[q] : 0u; H[e] = ok ? in.H[q] : kFinNone; C[e] = ok ? in.C[q] : 0u;
    s_H[lp] = H[e];
    s_g[lp] = 0xFFFFu;
  }
  if (tid < 2) s_g[kFinWin + tid] = 0xFFFFu;
  __syncthreads();
  // group sizes, from each group's last member
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    const u32 lp = tid + (u32)e * kFinTPB, q = w0 + lp;
    if (q < m) {
      const bool last = (q + 1u == m) || (lp + 1u < (u32)kFinWin && s_H[lp + 1u] != H[e]);
      const u32 off = P[e] - H[e];
      if (last && off < (u32)kFinMaxGroup) {
        const int a = (int)lp - (int)off;
        s_g[a >= 0 ? a : kFinWin] = (unsigned short)(off + 1u);
      }
    }
  }
  __syncthreads();
  int A[kFinE];                   // group start (window position), or -1: not this workgroup's to settle
  u32 G[kFinE];
  u32 hard_mask = 0;
  u32* s_cnt = s_H;               // (the heads are in registers by now) members per new sub-group, by its first position
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    const u32 lp = tid + (u32)e * kFinTPB, q = w0 + lp;
    A[e] = -1; G[e] = 0;
    s_cnt[lp] = 0u;
    if (q < m) {
      const int a = (int)lp - (int)(P[e] - H[e]);
      const u32 g = (P[e] - H[e] < (u32)kFinMaxGroup) ? s_g[a >= 0 ? a : kFinWin] : 0xFFFFu;
      if (g == 0xFFFFu) { if (lp < (u32)kFinStride) hard_mask |= 1u << e; }
      else if (a >= 0 && a < kFinStride) { A[e] = a; G[e] = g; }
    }
  }
  // Rounds.  A round compares 8 NW characters (RANK: the ranks, one round): every member counts the members of its
  // (sub-)group BELOW it (fin_count_below; broadcast LDS reads: the lanes of a wave walk a few neighbouring groups).
  // That number names its new sub-group -- equal members count the same -- and its place among its equals is the order
  // in which they arrive at the sub-group's counter (any order will do: they are a set until something tells them
  // apart).  The loop carries nothing else: a real text's first pass ran 1560 instructions per entry when it also
  // counted the equal members before and after.  The next round compares the sub-groups that are left, at their new
  // places, by the next characters -- read with the first round's: they come out of the cache line the first round paid
  // for, and a pass is bound by its random reads of the text, 149 bytes of HBM traffic per entry for the first sixteen
  // characters.
  const u32 kRound = 8u * NW;
  u64 all[kFinE][NW * NR];        // every round's characters, read in one go (RANK: the keys)
  u32 a_cur[kFinE], g_cur[kFinE], pos[kFinE];
  u32 slot0[kFinE];               // the slot of window position 0, were the group to start there (head slot - group start)
  int touches = 0;
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    const u32 lp = tid + (u32)e * kFinTPB;
    a_cur[e] = A[e] >= 0 ? (u32)A[e] : 0u; g_cur[e] = A[e] >= 0 ? G[e] : 0u; pos[e] = lp;
    slot0[e] = H[e] - a_cur[e];
#pragma unroll
    for (int q = 0; q < NW * NR; ++q) all[e][q] = 0;
    if (A[e] >= 0) {
      if (RANK) {
        const u64 t1 = (u64)S[e] + rk.at, t2 = (u64)S[e] + rk.at2;
        all[e][0] = t1 < (u64)n ? (u64)rk.rank[t1] + 1ull : 0ull;            // (a suffix that ends before the look-up: the smallest key)
        all[e][NW - 1] = (rk.at2 && t2 < (u64)n) ? (u64)rk.rank[t2] + 1ull : 0ull;
      } else {
        // every round's characters in one go: the later rounds' come out of the line(s) the first round's are in.  (Loaded
        // a round later, while the round before counts, the line has left L2 again: 300 bytes of traffic per entry instead
        // of 150, and 1.2 ms more per pass over 233 M entries.)
        fin_chars_n<NW * NR>(T, S[e] + (C[e] >> 8), n, all[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    if (A[e] >= 0) {
      const u32 lp = tid + (u32)e * kFinTPB;
      const u32 touch = (!RANK && (u64)S[e] + (C[e] >> 8) + kRound > (u64)n) ? 0x80000000u : 0u;        // (in the first round)
#pragma unroll
      for (int q = 0; q < NW; ++q) s_ch[(u32)NW * lp + (u32)q] = all[e][q];
      s_S[lp] = S[e] | touch;
      touches |= (!RANK && (u64)S[e] + (C[e] >> 8) + kChars > (u64)n) ? 1 : 0;                           // (in any round)
    }
  }
  // (a member that reaches past the end of T: one workgroup in a pass, if any -- everybody else runs the lean loop)
  const bool any_touch = __syncthreads_or(touches) != 0;
#pragma unroll
  for (u32 r = 0; r < nr; ++r) {
    u32* cnt = (r & 1u) ? s_cnt2 : s_cnt;              // (the first round's was cleared above)
    if (r > 0) {
#pragma unroll
      for (int e = 0; e < kFinE; ++e) {
        cnt[tid + (u32)e * kFinTPB] = 0u;
        if (g_cur[e] > 1u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) s_ch[(u32)NW * pos[e] + (u32)q] = all[e][r * NW + q];
          s_S[pos[e]] = S[e] | (((u64)S[e] + (C[e] >> 8) + (r + 1u) * kRound > (u64)n) ? 0x80000000u : 0u);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < kFinE; ++e) {
      if (g_cur[e] > 1u) {
        u64 key[NW];
#pragma unroll
        for (int q = 0; q < NW; ++q) key[q] = all[e][r * NW + q];
        const u32 below = fin_count_below<NW>(s_ch, s_S, a_cur[e], a_cur[e] + g_cur[e], pos[e], S[e], key, any_touch);
        a_cur[e] += below;
        if (RANK) {               // the member's new rank, noted by list position (kFinNone: it keeps the one it has)
          const u32 q = w0 + pos[e];                                 // (a final member's slot is its sub-group's head)
          rk.us[q] = below ? S[e] : kFinNone;
          rk.ur[q] = slot0[e] + a_cur[e];
        }
        pos[e] = a_cur[e] + atomicAdd(&cnt[a_cur[e]], 1u);           // its place among its equals: as they arrive
      }
    }
    __syncthreads();               // every read of the round's characters is done, every arrival counted
#pragma unroll
    for (int e = 0; e < kFinE; ++e) {
      if (g_cur[e] > 1u) g_cur[e] = cnt[a_cur[e]];
    }
  }
  // (the characters' bytes become the staging)
#pragma unroll
  for (int e = 0; e < kFinE; ++e) st_P[tid + (u32)e * kFinTPB] = kFinNone;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    if (g_cur[e]) {                                                            // (a member this workgroup settles)
      const u32 np = pos[e];
      const u32 fin = g_cur[e] == 1u ? 0x80000000u : 0u;                       // nobody equals it
      st_S[np] = S[e];
      st_P[np] = slot0[e] + np;
      st_H[np] = (slot0[e] + a_cur[e]) | fin;
      st_C[np] = RANK ? (unsigned short)C[e] : (unsigned short)((C[e] & 0xFFu) | (min(255u, (C[e] >> 8) + kChars) << 8));
    }
  }
  // the hard entries of this workgroup's stride range, in any order; one atomic per workgroup and list (a wave's own
  // atomic per iteration was 600 000 on one address for a real text's 40 M hard entries)
  u32 hard_depth = 0xFFFFFFFFu, shal_depth = 0xFFFFFFFFu;
  {
    u32 hm = 0, sm = 0;                                   // this thread's hard entries: of the hard list, of the shallow one
#pragma unroll
    for (int e = 0; e < kFinE; ++e) {
      if ((hard_mask >> e) & 1u) { if ((C[e] >> 8) < shal.floor) sm |= 1u << e; else hm |= 1u << e; }
    }
    __shared__ u32 s_hbase[2];
    u32 htot, stot;
    u32 hat = block_scan_excl_add<kFinTPB>((u32)__popc(hm), scr, &htot);
    u32 sat = block_scan_excl_add<kFinTPB>((u32)__popc(sm), scr, &stot);
    if (tid == 0) { s_hbase[0] = htot ? atomicAdd(hard_count, htot) : 0u; s_hbase[1] = stot ? atomicAdd(shal.count, stot) : 0u; }
    __syncthreads();
    hat += s_hbase[0]; sat += s_hbase[1];
#pragma unroll
    for (int e = 0; e < kFinE; ++e) {
      if ((hm >> e) & 1u) {
        hardS[hat] = S[e]; hardHP[hat] = ((u64)H[e] << 32) | (u64)P[e]; hardC[hat] = (unsigned short)C[e]; ++hat;
        hard_depth = min(hard_depth, C[e] >> 8);
      } else if ((sm >> e) & 1u) {
        shal.S[sat] = S[e]; shal.HP[sat] = ((u64)H[e] << 32) | (u64)P[e]; ++sat;
        shal_depth = min(shal_depth, C[e] >> 8);
      }
    }
  }
  // (one atomic per wave that has something to say, and only when it lowers what is there)
  for (int o = kWave / 2; o > 0; o >>= 1) {
    hard_depth = min(hard_depth, (u32)__shfl_xor(hard_depth, o, kWave));
    shal_depth = min(shal_depth, (u32)__shfl_xor(shal_depth, o, kWave));
  }
  if (lane == 0 && hard_depth != 0xFFFFFFFFu && hard_depth < __hip_atomic_load(hard_count + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(hard_count + 1, hard_depth);
  if (lane == 0 && shal_depth != 0xFFFFFFFFu && shal_depth < __hip_atomic_load(shal.count + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(shal.count + 1, shal_depth);
  __syncthreads();
  // in position order: finals leave, the rest is compacted into the next list
  u32 oS[kFinE], oP[kFinE], oH[kFinE], oC[kFinE];
  u32 left = 0, heads = 0;
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    const u32 lp = tid * (u32)kFinE + (u32)e;
    oP[e] = st_P[lp]; oS[e] = st_S[lp]; oH[e] = st_H[lp]; oC[e] = st_C[lp];
    if (oP[e] != kFinNone && !(oH[e] >> 31)) { ++left; if (oP[e] == oH[e]) ++heads; }
  }
  u32 total, total_heads;
  (void)block_scan_excl_add<kFinTPB>(heads, scr, &total_heads);
  u32 at = block_scan_excl_add<kFinTPB>(left, scr, &total);
  if (tid == 0) {
    const u32 oreg = (blockIdx.x / kFinChunk) % kFinRegions;
    s_base = ob.base[oreg] + (total ? atomicAdd(&next_count[oreg], total) : 0u);
    if (total_heads) atomicAdd(&next_count[kFinRegions], total_heads);      // groups of the list this pass leaves
  }
  __syncthreads();
  at += s_base;
#pragma unroll
  for (int e = 0; e < kFinE; ++e) {
    if (oP[e] == kFinNone) continue;
    if (oH[e] >> 31) {
      const u32 slot = oP[e], sfx = oS[e];
      SA[slot] = sfx;
      if (sfx == 0u) *em.pidx = slot;
      if (slot < em.out_n) em.out[slot] = (u8)oC[e];
      else *em.last_char = oC[e] & 0xFFu;
      lf_note(em, n, sfx, slot);
    } else {
      next.S[at] = oS[e]; next.P[at] = oP[e]; next.H[at] = oH[e]; next.C[at] = (unsigned short)oC[e];
      ++at;
    }
  }
}

// ---- bridge from the finisher to the doubling rounds: what is still tied (the hard list, with the
// last pass's leftovers appended) is sorted by slot and dressed up as a list the rounds understand
// (key = head slot | character << 56, value = suffix, positional slot array), and rank[] is completed
// for everybody: rank[SA[slot]] = slot for the finished, the group's head slot for the others.
// (entries of little depth -- a list no pass has looked at -- go to the shallow list instead: one atomic per entry, they are few;
// their places in the waiting list stay empty: suffix kFinNone, dropped when the list is dressed)
__global__ __launch_bounds__(256) void k_fin_to_hard(FinList in, u32 m, u32* __restrict__ hardS,
                                                     u64* __restrict__ hardHP, u32 at, u32* __restrict__ min_depth, FinShallow shal) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  u32 d = 0xFFFFFFFFu;
  if (i < m) {
    const u32 dep = in.C[i] >> 8;
    const u64 hp = ((u64)in.H[i] << 32) | (u64)in.P[i];
    if (dep < shal.floor) {
      const u32 j = atomicAdd(shal.count, 1u);
      shal.S[j] = in.S[i]; shal.HP[j] = hp;
      atomicMin(shal.count + 1, dep);
      hardS[at + i] = kFinNone; hardHP[at + i] = ~0ull;
    } else {
      hardS[at + i] = in.S[i];
      hardHP[at + i] = hp;
      d = dep;
    }
  }
  for (int o = kWave / 2; o > 0; o >>= 1) d = min(d, (u32)__shfl_xor(d, o, kWave));
  // the depth the rounds may start from (an atomic only where it lowers what is there: one per wave was 15 ms for 85 M entries)
  if (lane_id() == 0 && d != 0xFFFFFFFFu && d < __hip_atomic_load(min_depth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(min_depth, d);
}
// rank[us[q]] = ur[q] for the list positions q of one region (k_finish<RANK>'s notes)
__global__ __launch_bounds__(256) void k_rank_updates(const u32* __restrict__ us, const u32* __restrict__ ur, u32 base, u32 count,
                                                      u32* __restrict__ rank) {
  const u32 i0 = blockIdx.x * 1024u + threadIdx.x;
  u32 s[4], r[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { const u32 i = i0 + (u32)e * 256u; s[e] = i < count ? us[base + i] : kFinNone; r[e] = i < count ? ur[base + i] : 0u; }
#pragma unroll
  for (int e = 0; e < 4; ++e) if (s[e] != kFinNone) rank[s[e]] = r[e];
}
// one region of a list, copied to the end of another list's arrays
__global__ __launch_bounds__(256) void k_list_copy(FinList in, u32 m, FinList out, u32 at, u32* __restrict__ min_depth) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  u32 d = 0xFFFFFFFFu;
  if (i < m) {
    const unsigned short c = in.C[i];
    out.S[at + i] = in.S[i]; out.P[at + i] = in.P[i]; out.H[at + i] = in.H[i]; out.C[at + i] = c;
    d = c >> 8;
  }
  for (int o = kWave / 2; o > 0; o >>= 1) d = min(d, (u32)__shfl_xor(d, o, kWave));
  if (lane_id() == 0 && d != 0xFFFFFFFFu && d < __hip_atomic_load(min_depth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(min_depth, d);
}
// complete_ranks for a list that waits in finisher form: its suffixes rank as their groups' heads
__global__ __launch_bounds__(256) void k_bridge_pairs_fix_list(FinList in, u32 m, u32* __restrict__ pair_s, u32* __restrict__ pair_r) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const u32 p = in.P[i];
  pair_s[p] = in.S[i];
  pair_r[p] = in.H[i];
}
__global__ __launch_bounds__(256) void k_raw_to_park(const u32* __restrict__ S, const u32* __restrict__ P, const u32* __restrict__ H, u32 m,
                                                     u32* __restrict__ parkS, u64* __restrict__ parkHP, u32 at) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  parkS[at + i] = S[i];
  parkHP[at + i] = ((u64)H[i] << 32) | (u64)P[i];
}
__global__ __launch_bounds__(256) void k_bridge_dress(const u64* __restrict__ hp, const u32* __restrict__ sfx, u32 m,
                                                      const u8* __restrict__ T, u64* __restrict__ key,
                                                      u32* __restrict__ aglob) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const u64 x = hp[i];
  const u32 s = sfx[i];
  key[i] = (x >> 32) | ((u64)(s ? T[s - 1u] : 0u) << 56);
  aglob[i] = (u32)x;
}
__global__ __launch_bounds__(256) void k_bridge_pairs_all(const u32* __restrict__ SA, u32 n,
                                                          u32* __restrict__ pair_s, u32* __restrict__ pair_r) {
  const u32 p0 = blockIdx.x * 1024u + threadIdx.x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const u32 p = p0 + (u32)e * 256u;
    if (p < n) { pair_s[p] = SA[p]; pair_r[p] = p; }      // unfinished slots hold anything: k_bridge_pairs_fix rewrites them
  }
}
__global__ __launch_bounds__(256) void k_bridge_pairs_fix(const u32* __restrict__ sfx, const u32* __restrict__ aglob, u32 m,
                                                          u32* __restrict__ pair_s, u32* __restrict__ pair_r) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const u32 p = aglob[i];
  pair_s[p] = sfx[i];
  pair_r[p] = p;
}

// the same for a list that waits for its turn (its groups' head slots are its suffixes' ranks until then)
__global__ __launch_bounds__(256) void k_bridge_pairs_fix_parked(const u32* __restrict__ sfx, const u64* __restrict__ hp, u32 m,
                                                                 u32* __restrict__ pair_s, u32* __restrict__ pair_r) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const u64 x = hp[i];
  pair_s[(u32)x] = sfx[i];
  pair_r[(u32)x] = (u32)(x >> 32);
}

constexpr int kSimpleE = 4;   // independent items per thread in the latency-bound kernels

// ---------------------------------------------------------------------------------------
// Window kernels.  The lists they sweep are partitioned by suffix window (the top bits of s),
// so a chunk of consecutive items touches one or two windows of rank[] / T -- but inside a
// window the order is arbitrary, and a wave's 64 accesses still hit 64 different cache lines:
// rocprofv3 showed these kernels stalled on instruction issue (SQ_WAIT_INST_ANY 0.4-0.5 of the
// wave cycles, the address pipe working through one line per lane), not on HBM.  Each workgroup
// therefore reorders its chunk in LDS by eight more bits of s first -- an unstable counting sort,
// one returning ds_add per item gives both the bin count and the item's place in its bin -- and
// performs the accesses in that order: neighbouring lanes then share cache lines.  The order in
// which a chunk's items are processed (and, for the gather, written back) does not matter.
// ---------------------------------------------------------------------------------------
constexpr int kWinTPB = 256;
constexpr int kWinE = 8;
constexpr int kWinTile = kWinTPB * kWinE;     // items per workgroup

// XCD-contiguous chunking (speed only): the lists are partitioned by destination window, so
// giving each XCD one contiguous eighth of the list keeps every window in ONE L2.
__device__ __forceinline__ bool win_chunk(u32 m, u32* blk_out) {
  const u32 nblk = (m + (u32)kWinTile - 1u) / (u32)kWinTile;
  const u32 per_xcd = (nblk + 7u) / 8u;
  const u32 blk = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  *blk_out = blk;
  return blk < nblk;
}

// Places of the chunk's items in bin order.  bin[e] (< 256) of this thread's item e (ok bit e of
// okm) -> slot[e] in [0, count); s_cnt is 256 words of LDS, scr the block scan's scratch.
// Contains barriers; every thread of the workgroup must call it.
__device__ __forceinline__ void win_places(const u32 (&bin)[kWinE], u32 okm, u32 (&slot)[kWinE],
                                           u32* s_cnt, u32* scr) {
  s_cnt[threadIdx.x] = 0;                                 // kWinTPB == 256 bins
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kWinE; ++e) slot[e] = ((okm >> e) & 1u) ? atomicAdd(&s_cnt[bin[e]], 1u) : 0u;
  __syncthreads();
  u32 total;
  const u32 base = block_scan_excl_add<kWinTPB>(s_cnt[threadIdx.x], scr, &total);
  s_cnt[threadIdx.x] = base;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kWinE; ++e) slot[e] += s_cnt[bin[e]];
}

// rank[where[i]] = what[i] for pairs partitioned by the high bits of `where`.
__global__ __launch_bounds__(kWinTPB) void k_scatter_pairs(u32* __restrict__ dst,
                                                           const u32* __restrict__ where,
                                                           const u32* __restrict__ what, u32 m,
                                                           int bin_shift) {
  __shared__ u32 s_cnt[256], scr[kWinTPB / kWave + 1];
  __shared__ u32 s_w[kWinTile], s_v[kWinTile];
  u32 blk;
  if (!win_chunk(m, &blk)) return;
  const u32 p0 = blk * (u32)kWinTile + threadIdx.x;
  u32 w[kWinE], v[kWinE], bin[kWinE], slot[kWinE], okm = 0;
#pragma unroll
  for (int e = 0; e < kWinE; ++e) {
    const u32 p = p0 + e * kWinTPB;
    const bool ok = p < m;
    w[e] = ok ? where[p] : 0u;
    v[e] = ok ? what[p] : 0u;
    bin[e] = (w[e] >> bin_shift) & 255u;
    okm |= (ok ? 1u : 0u) << e;
  }
  win_places(bin, okm, slot, s_cnt, scr);
#pragma unroll
  for (int e = 0; e < kWinE; ++e) if ((okm >> e) & 1u) { s_w[slot[e]] = w[e]; s_v[slot[e]] = v[e]; }
  __syncthreads();
  const u32 count = min((u32)kWinTile, m - blk * (u32)kWinTile);
  for (u32 i = threadIdx.x; i < count; i += kWinTPB) dst[s_w[i]] = s_v[i];
}

// Dense route, step 2: rank[s] = nr for records (s << 32 | nr) partitioned by the high bits of s.
__global__ __launch_bounds__(kWinTPB) void k_scatter_dense(u32* __restrict__ rank,
                                                           const u64* __restrict__ rec, u32 m,
                                                           int bin_shift) {
  __shared__ u32 s_cnt[256], scr[kWinTPB / kWave + 1];
  __shared__ u64 s_r[kWinTile];
  u32 blk;
  if (!win_chunk(m, &blk)) return;
  const u32 p0 = blk * (u32)kWinTile + threadIdx.x;
  u64 r[kWinE];
  u32 bin[kWinE], slot[kWinE], okm = 0;
#pragma unroll
  for (int e = 0; e < kWinE; ++e) {
    const u32 p = p0 + e * kWinTPB;
    const bool ok = p < m;
    r[e] = ok ? rec[p] : 0ull;
    bin[e] = ((u32)(r[e] >> 32) >> bin_shift) & 255u;
    okm |= (ok ? 1u : 0u) << e;
  }
  win_places(bin, okm, slot, s_cnt, scr);
#pragma unroll
  for (int e = 0; e < kWinE; ++e) if ((okm >> e) & 1u) s_r[slot[e]] = r[e];
  __syncthreads();
  const u32 count = min((u32)kWinTile, m - blk * (u32)kWinTile);
  for (u32 i = threadIdx.x; i < count; i += kWinTPB) { const u64 x = s_r[i]; rank[(u32)(x >> 32)] = (u32)x; }
}

// ---------------------------------------------------------------------------------------
// Runs.  k[s] = number of positions from s on that hold T[s] (the run ends at n at the latest).  A group whose
// members share c^h holds exactly the suffixes with k >= h, and their order is known in closed form: the members whose
// run is followed by something smaller (or by the end of T) first, by ascending k, then the others by descending k;
// members equal in that come from different runs, share exactly k characters and are ordered by the rank of the
// run's tail, rank[s + k].  So ONE round (the run step, mode 1) gives such members the second key (type, k | n - k)
// instead of rank[s + h] + 1 -- a bit more than a rank needs -- and does not double the list's depth; every later
// round (mode 2) looks a member with k >= h_split up at rank[s + max(h, k)] instead of rank[s + h].  k[] is made by the
// stretch-length pass below, as the lengths of period 1.
// ---------------------------------------------------------------------------------------
// merged (BWTC_HIP_MULTI, tests/multimodel.py): k[] holds the block's merged look-up words, which several steps have written
// -- a length in bits 0 ... 30 (0: no step has taken s), and bit 31 = "member of the current step", which only that step's
// own round (mode 1) reads.  The member takes the closed-form key; every other suffix with a length looks up at
// max(h, length), in the step's own round too; h_split is not read.
constexpr u32 kStepMember = 0x80000000u, kStepLength = 0x7FFFFFFFu;
struct RunKeys { const u32* k; u32 h_split; int mode; u32 p; bool merged; };   // mode 0: no runs in play (k is not read); 1: the run step; 2: a round after it; 3: a copy round (k[] is K[], "Copies" below); p: the period k[] was made for (1: runs)
__device__ __forceinline__ u32 run_offset(const RunKeys& rk, u32 s, u32 h) {
  if (rk.mode == 3) {                                   // K[s] + h; a sum past 32 bits lies past the end of every block
    const u32 kk = rk.k[s];
    return kk > ~h ? 0xFFFFFFFFu : kk + h;
  }
  if (rk.merged) {
    if (rk.mode == 0) return h;
    const u32 kk = rk.k[s] & kStepLength;
    return kk ? max(h, kk) : h;
  }
  if (rk.mode != 2) return h;
  const u32 kk = rk.k[s];
  return kk >= rk.h_split ? max(h, kk) : h;
}
// the second key of suffix s in a round at depth h (b2: the key's bits, one more than a rank's in the run step);
// rank == nullptr (a run step before rank[] is complete): the members without a long run keep their group
__device__ __forceinline__ u64 run_key2(const RunKeys& rk, const u32* __restrict__ rank, const u8* __restrict__ T,
                                        u32 s, u32 n, u32 h, int b2) {
  if (rk.mode == 1) {
    const u32 w = rk.k[s];
    const u32 kk = rk.merged ? w & kStepLength : w;
    if (rk.merged ? (w & kStepMember) != 0u : kk >= h) {
      const u64 e = (u64)s + kk;
      const bool falling = e >= (u64)n || T[e] < T[e - rk.p];   // (p = 1: T[e - 1] is the run's byte, T[s]; kk >= h >= p)
      return falling ? (u64)kk : (1ull << (b2 - 1)) | (u64)(n - kk);
    }
  }
  if (!rank) return 0ull;
  const u64 t = (u64)s + run_offset(rk, s, h);
  return t < (u64)n ? (u64)rank[t] + 1ull : 0ull;
}

// ---------------------------------------------------------------------------------------
// Periods.  The run rule holds for every period p >= 1 (tests/periodmodel.py): position q is a break when q >= p and
// T[q] != T[q - p] (p = 1: a run start); k_p[s] = (the first break at or behind s + p, or n) - s is the number of leading
// characters of suffix s that are p-periodic, and k_1 is the runs' k.  Once a list is sorted to a depth h >= p, a group
// holds members with k_p >= h only or none, and those are ordered as a run's: the falling ones (the end of T, or
// T[s + k] < T[s + k - p]) by ascending k, then the rising ones by descending k, ties by rank[s + k].  So the period step
// is the run step over k_p[] (d_runK holds the lengths of one period at a time) with RunKeys::p = p.
//
// The stretch-length pass makes k_p[] for any p, runs included: three launches over tiles of kRunTile positions (256
// threads x 64 consecutive bytes, 16-byte loads), a right-to-left carry in one workgroup, coalesced 4-byte stores.  A
// thread works out the first break at or behind x for the positions x of its tile and stores it as k_p[x - p]: nobody
// looks ahead into the next chunks, and the tiles cover x in [p, n + p).  The 64-bit break mask of a thread's positions
// is made in two ways, and the kernels are templated on which: run_starts (p = 1) carries the previous byte in
// registers and reads the text once; period_breaks (any p) compares with the text p bytes back, a second stream read
// by aligned 16-byte loads and shifted into place.  The run instantiation also keeps its own store form, one
// `if constexpr` in the store loop: the thread at q looks at the break bits behind q and stores k[q].
// A third maker, flag_breaks, reads a flag byte per position in the text's place with p = 0 (copy rounds, "Copies" below).
// ---------------------------------------------------------------------------------------
constexpr u32 kRunTile = 16384, kRunTPB = 256, kRunNone = 0xFFFFFFFFu;
// the 64 positions from `at` on (a multiple of 64): bit j set = position at + j starts a run
__device__ __forceinline__ u64 run_starts(const u8* __restrict__ T, u32 at, u32 n) {
  if (at >= n) return 0ull;
  u32 prev = at ? T[at - 1u] : 0u;
  u64 mask = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32 a = at + 16u * q;
    if (a >= n) break;                                  // (T is padded: a 16-byte load that begins below n is the arena's)
    const uint4 v = *reinterpret_cast<const uint4*>(T + a);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const u32 c = (w[j >> 2] >> (8 * (j & 3))) & 255u;
      if (c != prev) mask |= 1ull << (16 * q + j);
      prev = c;
    }
  }
  if (at == 0) mask &= ~1ull;                           // position 0 starts no run: nothing lies before it
  const u32 left = n - at;                              // positions at or past n are not the text's
  if (left < 64u) mask &= (1ull << left) - 1ull;
  return mask;
}
__device__ __forceinline__ u32 differing_bytes(u32 x) {   // bit j set = byte j of x is not zero
  return ((x & 0x000000FFu) ? 1u : 0u) | ((x & 0x0000FF00u) ? 2u : 0u) | ((x & 0x00FF0000u) ? 4u : 0u) | ((x & 0xFF000000u) ? 8u : 0u);
}
// the sixteen words of T that begin bs bytes into w[], beside the words a[]
__device__ __forceinline__ u64 period_compare(const u32 (&a)[16], const u32 (&w)[20], u32 bs) {
  u64 mask = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const u64 two = ((u64)w[i + 1] << 32) | (u64)w[i];
    const u32 b = (u32)(two >> (8u * bs));
    mask |= (u64)differing_bytes(a[i] ^ b) << (4 * i);
  }
  return mask;
}
// the 64 positions from `at` on (a multiple of 64): bit j set = position at + j is a break of period p
__device__ __forceinline__ u64 period_breaks(const u8* __restrict__ T, u32 at, u32 n, u32 p) {
  if (at >= n || at + 64u <= p) return 0ull;
  u64 mask = 0;
  if (at < p) {
    // the one chunk of the block that holds position p: nothing lies p bytes before its first positions
    for (u32 j = p - at; j < 64u && at + j < n; ++j)
      if (T[at + j] != T[at + j - p]) mask |= 1ull << j;
    return mask;
  }
  const u32 from = at - p;                              // the second stream: T[from ...] beside T[at ...]
  const u32 a0 = from & ~15u, sh = from & 15u;          // (sh is the same for every thread: at is a multiple of 64)
  u32 a[16], w[20];
#pragma unroll
  for (int q = 0; q < 4; ++q) {                         // (T is padded: a 16-byte load that begins below n is the arena's)
    const u32 x = at + 16u * q;
    const uint4 v = x < n ? *reinterpret_cast<const uint4*>(T + x) : make_uint4(0u, 0u, 0u, 0u);
    a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const u32 x = a0 + 16u * q;
    const uint4 v = x < n ? *reinterpret_cast<const uint4*>(T + x) : make_uint4(0u, 0u, 0u, 0u);
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  // the second stream begins sh bytes into w[]: whole words first, by moves between registers (a switch over the word
  // count becomes an indexed w[], which leaves the registers), then bytes
  if (sh & 8u) {
#pragma unroll
    for (int i = 0; i < 18; ++i) w[i] = w[i + 2];
  }
  if (sh & 4u) {
#pragma unroll
    for (int i = 0; i < 17; ++i) w[i] = w[i + 1];
  }
  mask = period_compare(a, w, sh & 3u);
  const u32 left = n - at;                              // positions at or past n are not the text's
  if (left < 64u) mask &= (1ull << left) - 1ull;
  return mask;
}
// The proper positions among the suffixes q = at + j - p that the 64 positions from `at` on stand for (k_stretch_lengths
// stores k_p[x - p] at x): bit j set = q + 1 < n and T[q] != T[q + 1].  No position inside a run of one byte is proper,
// and a unit that is not one byte over and over has a proper position among any p consecutive ones.  The bytes are the
// second stream of period_breaks and one more: the same aligned loads (the caches hold them), shifted the same way.
__device__ __forceinline__ u64 proper_starts(const u8* __restrict__ T, u32 at, u32 n, u32 p) {
  if (at + 64u <= p || n < 2u) return 0ull;
  u64 mask = 0;
  if (at < p) {
    for (u32 j = p - at; j < 64u && at + j - p + 1u < n; ++j)
      if (T[at + j - p] != T[at + j - p + 1u]) mask |= 1ull << j;
    return mask;
  }
  const u32 from = at - p;
  if (from >= n - 1u) return 0ull;
  const u32 a0 = from & ~15u, sh = from & 15u;
  u32 w[20];
#pragma unroll
  for (int q = 0; q < 5; ++q) {                         // (T is padded: a 16-byte load that begins below n is the arena's)
    const u32 x = a0 + 16u * q;
    const uint4 v = x < n ? *reinterpret_cast<const uint4*>(T + x) : make_uint4(0u, 0u, 0u, 0u);
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  if (sh & 8u) {
#pragma unroll
    for (int i = 0; i < 18; ++i) w[i] = w[i + 2];
  }
  if (sh & 4u) {
#pragma unroll
    for (int i = 0; i < 17; ++i) w[i] = w[i + 1];
  }
  const u32 bs = sh & 3u;
#pragma unroll
  for (int i = 0; i < 16; ++i) {                        // (w[16] is the text's still: 3 words and 3 bytes of shift, 68 bytes wanted, 80 loaded)
    const u64 two = ((u64)w[i + 1] << 32) | (u64)w[i];
    const u32 b = (u32)(two >> (8u * bs)), c = (u32)(two >> (8u * bs + 8u));
    mask |= (u64)differing_bytes(b ^ c) << (4 * i);
  }
  const u32 left = n - 1u - from;                       // suffixes from n - 1 on have no byte behind them
  if (left < 64u) mask &= (1ull << left) - 1ull;
  return mask;
}
// The third maker (copy rounds, "Copies" below): T is not the text but one flag byte per position, P[]; bit j set =
// P[at + j] is 0.  p is 0 then: the general store form stores K[q] = (the first break at or behind q) - q at q itself.
__device__ __forceinline__ u64 flag_breaks(const u8* __restrict__ P, u32 at, u32 n) {
  if (at >= n) return 0ull;
  u64 mask = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {                         // (P[] has the room of four bytes per position: the loads are its own)
    const u32 a = at + 16u * q;
    if (a >= n) break;
    const uint4 v = *reinterpret_cast<const uint4*>(P + a);
    const u64 set = (u64)differing_bytes(v.x) | ((u64)differing_bytes(v.y) << 4) | ((u64)differing_bytes(v.z) << 8) | ((u64)differing_bytes(v.w) << 12);
    mask |= (~set & 0xFFFFull) << (16 * q);
  }
  const u32 left = n - at;                              // positions at or past n are not the block's
  if (left < 64u) mask &= (1ull << left) - 1ull;
  return mask;
}
// RUN: the pass of period 1, its mask from run_starts (p is 1 then); FLAGS: flag_breaks' (p is 0); else period_breaks'
template <bool RUN, bool FLAGS = false>
__device__ __forceinline__ u64 stretch_breaks(const u8* __restrict__ T, u32 at, u32 n, u32 p) {
  static_assert(!(RUN && FLAGS), "one maker of the break mask");
  if constexpr (RUN) return run_starts(T, at, n);
  else if constexpr (FLAGS) return flag_breaks(T, at, n);
  else return period_breaks(T, at, n, p);
}
// launch 1: first[t] = the first break in tile t, or none (tiles past n included: the lengths' tiles reach n + p)
template <bool RUN, bool FLAGS = false>
__global__ __launch_bounds__(kRunTPB) void k_stretch_tiles(const u8* __restrict__ T, u32 n, u32 p, u32* __restrict__ first) {
  __shared__ u32 s_min[kRunTPB / kWave];
  const u32 at = blockIdx.x * kRunTile + threadIdx.x * 64u;
  const u64 mask = stretch_breaks<RUN, FLAGS>(T, at, n, p);
  u32 f = mask ? at + (u32)__builtin_ctzll(mask) : kRunNone;
  for (int o = kWave / 2; o > 0; o >>= 1) f = min(f, (u32)__shfl_xor(f, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) s_min[threadIdx.x / kWave] = f;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 w = 1; w < kRunTPB / kWave; ++w) f = min(f, s_min[w]);
    first[blockIdx.x] = f;
  }
}
// launch 2 (one workgroup): behind[t] = the first break in a tile after t, or n -- a right-to-left carry
__global__ __launch_bounds__(1024) void k_run_carry(const u32* __restrict__ first, u32 tiles, u32 n, u32* __restrict__ behind) {
  __shared__ u32 s_part[1024];
  const u32 per = (tiles + 1023u) / 1024u;
  const u32 lo = min(tiles, threadIdx.x * per), hi = min(tiles, lo + per);
  u32 f = kRunNone;
  for (u32 t = lo; t < hi; ++t) f = min(f, first[t]);
  s_part[threadIdx.x] = f;
  __syncthreads();
  if (threadIdx.x == 0) {                               // exclusive suffix minimum of the 1024 parts
    u32 run = kRunNone;
    for (int i = 1023; i >= 0; --i) { const u32 v = s_part[i]; s_part[i] = run; run = min(run, v); }
  }
  __syncthreads();
  u32 run = s_part[threadIdx.x];
  for (u32 t = hi; t > lo; --t) {
    behind[t - 1u] = run == kRunNone ? n : run;
    run = min(run, first[t - 1u]);
  }
}
// launch 3: k_p[x - p] for the positions x of the tile (coalesced 4-byte stores), and the block's longest k_p.
// PROPER (never with RUN): the longest k_p over the proper positions too (proper_starts), into longest[1] -- a second
// mask per thread, a second maximum per wave; the instantiations without it are what they were.
// MERGE (with PROPER, never with RUN; BWTC_HIP_MULTI): k[] holds the block's merged look-up words (tests/multimodel.py) --
// a length in bits 0 ... 30, bit 31 = "member of the current step".  The step of period p at depth h takes s when
// k_p[s] >= h and k_p[s] >= the old length (0 for everybody when fresh: the block's first step); it stores k_p | bit 31
// there and the old length, its flag cleared, everywhere else.  One more coalesced 4-byte load per store; both maxima
// are over k_p, not over the merged word.  h and fresh are read by this instantiation alone.
// FLAGS (never with the others; copy rounds): the mask comes from flag_breaks over P[] in T's place, p_any is 0, and the
// general store form writes K[q] at q itself -- the aligned stores the run instantiation keeps its own form for.
template <bool RUN, bool PROPER = false, bool MERGE = false, bool FLAGS = false>
__global__ __launch_bounds__(kRunTPB) void k_stretch_lengths(const u8* __restrict__ T, u32 n, u32 p_any, const u32* __restrict__ behind,
                                                              u32* __restrict__ k, u32* __restrict__ longest, u32 h, u32 fresh) {
  static_assert(!MERGE || (PROPER && !RUN), "the merging pass is the general form with both maxima");
  static_assert(!FLAGS || (!RUN && !PROPER && !MERGE), "the flags' pass is the general form with p = 0");
  __shared__ u64 s_mask[kRunTPB];
  __shared__ u32 s_next[kRunTPB];                      // the first break behind the thread's 64 positions
  __shared__ u32 s_wave[kRunTPB / kWave];
  const u32 p = RUN ? 1u : p_any;
  const u32 base = blockIdx.x * kRunTile;
  const u32 at = base + threadIdx.x * 64u;
  const u64 mask = stretch_breaks<RUN, FLAGS>(T, at, n, p);
  s_mask[threadIdx.x] = mask;
  __shared__ u64 s_proper[PROPER ? kRunTPB : 1];
  if constexpr (PROPER) s_proper[threadIdx.x] = proper_starts(T, at, n, p);
  // suffix minimum of the threads' first breaks: inside the wave by shuffles, across the four waves through LDS
  const u32 lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  u32 incl = mask ? at + (u32)__builtin_ctzll(mask) : kRunNone;
  for (int o = 1; o < kWave; o <<= 1) {
    const u32 t = __shfl_down(incl, o, kWave);
    if (lane + o < (u32)kWave) incl = min(incl, t);
  }
  if (lane == 0) s_wave[wave] = incl;
  u32 excl = __shfl_down(incl, 1, kWave);
  if (lane == kWave - 1) excl = kRunNone;
  __syncthreads();
  for (u32 w = wave + 1; w < kRunTPB / kWave; ++w) excl = min(excl, s_wave[w]);
  if (excl == kRunNone) excl = behind[blockIdx.x];
  s_next[threadIdx.x] = excl;
  __syncthreads();
  u32 best = 0;
  [[maybe_unused]] u32 best_proper = 0;
  for (u32 j = 0; j < kRunTile / kRunTPB; ++j) {
    const u32 x = base + j * kRunTPB + threadIdx.x;     // chunk j * 4 + wave of the tile, bit `lane`
    const u32 c = j * (kRunTPB / 64u) + wave;
    u32 q, nd;
    if constexpr (RUN) {
      // (runs: the thread looks one position ahead and stores at its own -- the same k[], by stores that begin at a
      // multiple of 1 KiB: measurably faster than the stores 4 bytes before it; the last tile of n + 1 may find nothing)
      q = x;
      if (q >= n) break;
      const u64 later = lane < 63u ? s_mask[c] >> (lane + 1u) : 0ull;
      nd = later ? q + 1u + (u32)__builtin_ctzll(later) : s_next[c];
    } else {
      if (x < p) continue;
      q = x - p;                                        // the suffix whose periodic stretch ends at the first break from x on
      if (q >= n) break;
      const u64 here = s_mask[c] >> lane;
      nd = here ? x + (u32)__builtin_ctzll(here) : s_next[c];
    }
    const u32 kk = min(nd, n) - q;
    if constexpr (MERGE) {
      if (k) {
        const u32 was = fresh ? 0u : (k[q] & kStepLength);
        k[q] = (kk >= h && kk >= was) ? (kk | kStepMember) : was;
      }
    } else {
      if (k) k[q] = kk;                                 // (k == nullptr: a trial, for the longest stretch alone)
    }
    best = max(best, kk);
    if constexpr (PROPER) { if ((s_proper[c] >> lane) & 1ull) best_proper = max(best_proper, kk); }
  }
  for (int o = kWave / 2; o > 0; o >>= 1) best = max(best, (u32)__shfl_xor(best, o, kWave));
  if (lane == 0 && best) atomicMax(longest, best);
  if constexpr (PROPER) {
    for (int o = kWave / 2; o > 0; o >>= 1) best_proper = max(best_proper, (u32)__shfl_xor(best_proper, o, kWave));
    if (lane == 0 && best_proper) atomicMax(longest + 1, best_proper);
  }
}

// ---------------------------------------------------------------------------------------
// Copies (BWTC_HIP_COPIES, tests/copymodel.py).  Whole copies of a piece at places that are no period of the text between
// them stay tied for the rest of the copy.  In a list at depth h with rank[] current:
//   F(G)   every member s of the tied group G has s + 1 < n, and rank[s + 1] is one value for all of them
//   P(s)   s is tied in this list and F holds for its group;  K(s) = the positions q = s, s + 1, ... with P(q)
// All members of a group have one K and share K + h characters, so the round looks up rank[s + K(s) + h] (RunKeys mode 3)
// and doubles its depth as ever.  K[] is made by three passes over the list the ranking's apply kernel has just left
// (suffix and dense group number per entry, in list order), after rank[] is updated and before the key kernel:
//   marks     bad[g] = 1 where two neighbours of group g differ in rank[s + 1] (none: all ones).  A lane takes its
//             neighbour's value by a cross-lane move; lane 0 of a wave -- the wave and tile seams -- fetches it itself
//   flags     P[s] = 1 for every entry whose group is not bad, over zeros
//   lengths   the stretch-length pass with flag_breaks as the maker of the break mask, into d_runK
// bad[] is cleared per pass (a byte per group); P[] is a byte per position: plain stores, no atomics.
// ---------------------------------------------------------------------------------------
constexpr u32 kCopyTPB = 256, kCopyE = 4, kCopyTile = kCopyTPB * kCopyE, kCopyNone = 0xFFFFFFFFu;
__device__ __forceinline__ u32 copy_successor(const u32* __restrict__ rank, u32 s, u32 n) { return s + 1u < n ? rank[s + 1u] : kCopyNone; }
__global__ __launch_bounds__(kCopyTPB) void k_copy_marks(const u32* __restrict__ aidx, const u32* __restrict__ agrp, u32 m,
                                                         const u32* __restrict__ rank, u32 n, u8* __restrict__ bad) {
  const u32 lane = threadIdx.x & (kWave - 1);
  u32 g[kCopyE], v[kCopyE];
#pragma unroll
  for (u32 e = 0; e < kCopyE; ++e) {                    // (all of a wave's lanes make every cross-lane move: no early way out)
    const u32 i = blockIdx.x * kCopyTile + e * kCopyTPB + threadIdx.x;
    g[e] = i < m ? agrp[i] : kCopyNone;
    v[e] = i < m ? copy_successor(rank, aidx[i], n) : kCopyNone;
  }
#pragma unroll
  for (u32 e = 0; e < kCopyE; ++e) {
    const u32 i = blockIdx.x * kCopyTile + e * kCopyTPB + threadIdx.x;
    u32 pg = __shfl_up(g[e], 1, kWave), pv = __shfl_up(v[e], 1, kWave);
    if (lane == 0) {
      pg = kCopyNone;
      if (i > 0 && i < m) { pg = agrp[i - 1u]; pv = copy_successor(rank, aidx[i - 1u], n); }
    }
    if (i < m && pg == g[e] && pv != v[e]) bad[g[e]] = 1;
  }
}
__global__ __launch_bounds__(kCopyTPB) void k_copy_flags(const u32* __restrict__ aidx, const u32* __restrict__ agrp, u32 m,
                                                         const u8* __restrict__ bad, u32 n, u8* __restrict__ P) {
#pragma unroll
  for (u32 e = 0; e < kCopyE; ++e) {
    const u32 i = blockIdx.x * kCopyTile + e * kCopyTPB + threadIdx.x;
    if (i >= m) continue;
    const u32 s = aidx[i];
    if (s + 1u < n && !bad[agrp[i]]) P[s] = 1;          // (a group of one whose member is n - 1 has no neighbour to differ from)
  }
}

// The period finder: one pass over a sorted list.  Neighbouring entries of one group (equal keys under kmask) that lie
// d positions apart, 2 <= d <= kPeriodMax, vote for d: inside a stretch of period p the members of a group lie p apart
// and are neighbours.  A histogram in LDS per workgroup, then one global add per non-empty bin, the workgroups
// beginning at different bins.
constexpr u32 kVoteTPB = 256, kVoteTile = 16384, kVoteBins = kPeriodMax + 1;
constexpr int kSmallPeriod = 802;      // d_small: the block's longest k_p; [803] the probe's flag; [804..805] the finder's winner and its votes (k_period_winners: [804..819], 8 such pairs)
constexpr u32 kPeriodMinVotes = 256;   // the winner's votes buy the period-length pass from max(this, n / 64) on (find_period)
constexpr u64 kPeriodWorth = 8;        // a voted period's longest stretch must reach this many times max(the first round's depth, p)
// RUNS_OUT (BWTC_HIP_MIXED, with k_1[] in k1): two members of one run of one byte do not vote -- a long run's group
// comes in the order of the sort's windows, and its members would outvote the stretches with the windows' distance.
template <bool RUNS_OUT>
__global__ __launch_bounds__(kVoteTPB) void k_period_votes(const u64* __restrict__ ks, const u32* __restrict__ vs, u32 m, u64 kmask,
                                                           u32* __restrict__ table, const u32* __restrict__ k1) {
  __shared__ u32 s_bin[kVoteBins];
  for (u32 b = threadIdx.x; b < kVoteBins; b += kVoteTPB) s_bin[b] = 0;
  __syncthreads();
  const u32 base = blockIdx.x * kVoteTile;
  for (u32 j = 0; j < kVoteTile / kVoteTPB; ++j) {
    const u32 i = base + j * kVoteTPB + threadIdx.x;
    if (i + 1u >= m) break;
    if (((ks[i] ^ ks[i + 1u]) & kmask) != 0ull) continue;
    const u32 a = vs[i], b = vs[i + 1u];
    const u32 d = a > b ? a - b : b - a;
    if (d < 2u || d > kPeriodMax) continue;
    if constexpr (RUNS_OUT) { if (k1[min(a, b)] > d) continue; }
    atomicAdd(&s_bin[d], 1u);
  }
  __syncthreads();
  const u32 turn = (blockIdx.x * 67u) % kVoteBins;
  for (u32 b = threadIdx.x; b < kVoteBins; b += kVoteTPB) {
    u32 bb = b + turn;
    if (bb >= kVoteBins) bb -= kVoteBins;
    const u32 c = s_bin[bb];
    if (c) atomicAdd(&table[bb], c);
  }
}
// The probe before the pass: thread i walks the window of `span` positions from p + i * span on and stops at its first
// break; a window without one sets the flag, and threads that find it set do not begin.
__global__ __launch_bounds__(256) void k_period_probe(const u8* __restrict__ T, u32 n, u32 p, u32 span, u32 windows, u32* flag) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= windows) return;
  if (*reinterpret_cast<volatile u32*>(flag)) return;
  const u64 x0 = (u64)p + (u64)i * span;
  if (x0 + span > (u64)n) return;
  const u8* a = T + x0;
  const u8* b = a - p;
  for (u32 j = 0; j < span; ++j)
    if (a[j] != b[j]) return;
  atomicOr(flag, 1u);
}
// (one workgroup) out[0] = the distance with the most votes (the smallest of equals), out[1] = its votes
__global__ __launch_bounds__(1024) void k_period_winner(const u32* __restrict__ table, u32* __restrict__ out) {
  __shared__ u64 s_best[1024];
  u64 best = 0;
  for (u32 b = threadIdx.x; b < kVoteBins; b += 1024u) {
    const u64 v = ((u64)table[b] << 32) | (u64)(kVoteBins - b);
    best = v > best ? v : best;
  }
  s_best[threadIdx.x] = best;
  __syncthreads();
  for (u32 o = 512; o > 0; o >>= 1) {
    if (threadIdx.x < o) { const u64 v = s_best[threadIdx.x + o]; if (v > s_best[threadIdx.x]) s_best[threadIdx.x] = v; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const u64 v = s_best[0];
    out[0] = (v >> 32) ? kVoteBins - (u32)v : 0u;
    out[1] = (u32)(v >> 32);
  }
}

// (one workgroup; BWTC_HIP_MULTI) The finder's candidates, tests/multimodel.py's candidates(): out[2 i], out[2 i + 1] = the
// distance in 2 ... kPeriodMax with the i-th most votes among those with `need` votes or more (the smaller distance first
// among equals) and its votes, i < kPeriodCandidates; zeros from where there are no more.  A bin's key is
// votes << 32 | kVoteBins - distance, so no two are equal: selection i is the largest key below selection i - 1.
__global__ __launch_bounds__(1024) void k_period_winners(const u32* __restrict__ table, u32 need, u32* __restrict__ out) {
  __shared__ u64 s_best[1024];
  u64 key[(kVoteBins + 1023u) / 1024u];
#pragma unroll
  for (u32 j = 0; j < (kVoteBins + 1023u) / 1024u; ++j) {
    const u32 b = j * 1024u + threadIdx.x;
    const u32 v = (b >= 2u && b < kVoteBins) ? table[b] : 0u;
    key[j] = (v >= need && v) ? ((u64)v << 32) | (u64)(kVoteBins - b) : 0ull;
  }
  u64 below = ~0ull;
  for (u32 i = 0; i < kPeriodCandidates; ++i) {
    u64 best = 0;
#pragma unroll
    for (u32 j = 0; j < (kVoteBins + 1023u) / 1024u; ++j)
      if (key[j] < below && key[j] > best) best = key[j];
    s_best[threadIdx.x] = best;
    __syncthreads();
    for (u32 o = 512; o > 0; o >>= 1) {
      if (threadIdx.x < o) { const u64 v = s_best[threadIdx.x + o]; if (v > s_best[threadIdx.x]) s_best[threadIdx.x] = v; }
      __syncthreads();
    }
    below = s_best[0];
    __syncthreads();
    if (threadIdx.x == 0) {
      out[2u * i] = below ? kVoteBins - (u32)below : 0u;
      out[2u * i + 1u] = (u32)(below >> 32);
    }
    // (below == 0: nothing is left, and nothing is below 0 -- the entries from here on come out as zeros)
  }
}

// ---------------------------------------------------------------------------------------
// Long periods (BWTC_HIP_LONG_PERIODS, tests/longperiodmodel.py).  The rule, the stretch-length pass and the deferred step
// know no limit on p; the finder above and its probe do.  Under the switch neighbours that lie kPeriodMax < d <= dmax apart
// vote too, exactly, in two sweeps: sweep 1 is the vote kernel with a second LDS table of coarse bins d >> 12 beside the
// short one (one pass over the list for both); a distance with `need` votes lies in a coarse bin with `need` votes, of
// which a list holds at most kLongSel, so sweep 2 -- only behind such a bin -- makes the exact histograms of d & 4095 for
// the bins k_long_coarse_pick selected, kFineGroup of them per workgroup.  k_long_period_winners merges them with the short
// table by k_period_winners' order.  The long finder's words (d_lvotes): the coarse table, then the selected bins, then
// kLongSel fine tables of kFineBins words.
// ---------------------------------------------------------------------------------------
constexpr u32 kCoarseShift = 12, kFineBins = 1u << kCoarseShift, kCoarseBins = (kLongPeriodMax >> kCoarseShift) + 1;
constexpr u32 kLongSel = 64;           // (m - 1) / need: below 65 for need = max(256, n / 64) and m <= n
constexpr u32 kLongSelAt = 4352, kLongFineAt = 8192;   // d_lvotes: the words of the selected bins, of the fine tables
constexpr u32 kFineGroup = 3;          // fine tables per workgroup of sweep 2: 48 KiB of LDS
constexpr u32 kLongVoteTile = kVoteTile;   // entries per workgroup of both sweeps (tiles of four times as many measured no faster on 268 M entries, 1.23 against 1.29 ms, and slower on shorter lists: DESIGN.md section 6)
constexpr int kSmallLong = kSmallPeriod + 2 + 2 * (int)kPeriodCandidates;   // d_small: the coarse bins with `need` votes
static_assert(kCoarseBins <= kLongSelAt && kLongSelAt + kLongSel <= kLongFineAt, "the long finder's words do not overlap");
template <bool RUNS_OUT>
__global__ __launch_bounds__(kVoteTPB) void k_period_votes_long(const u64* __restrict__ ks, const u32* __restrict__ vs, u32 m, u64 kmask,
                                                                u32* __restrict__ table, const u32* __restrict__ k1,
                                                                u32* __restrict__ coarse, u32 dmax) {
  // one table for both: short bin b counts in the lower half of word b, coarse bin b in the upper half -- a tile's
  // kLongVoteTile entries cannot carry out of 16 bits, and the kernel keeps k_period_votes' LDS and occupancy
  __shared__ u32 s_bin[kVoteBins];
  for (u32 b = threadIdx.x; b < kVoteBins; b += kVoteTPB) s_bin[b] = 0;
  __syncthreads();
  const u32 base = blockIdx.x * kLongVoteTile;
  for (u32 j = 0; j < kLongVoteTile / kVoteTPB; ++j) {
    const u32 i = base + j * kVoteTPB + threadIdx.x;
    if (i + 1u >= m) break;
    if (((ks[i] ^ ks[i + 1u]) & kmask) != 0ull) continue;
    const u32 a = vs[i], b = vs[i + 1u];
    const u32 d = a > b ? a - b : b - a;
    if (d < 2u || (d > kPeriodMax && d > dmax)) continue;
    if constexpr (RUNS_OUT) { if (k1[min(a, b)] > d) continue; }
    if (d <= kPeriodMax) atomicAdd(&s_bin[d], 1u);
    else atomicAdd(&s_bin[d >> kCoarseShift], 1u << 16);   // (dmax <= kLongPeriodMax: the bin is the table's)
  }
  __syncthreads();
  const u32 turn = (blockIdx.x * 67u) % kVoteBins;
  for (u32 b = threadIdx.x; b < kVoteBins; b += kVoteTPB) {
    u32 bb = b + turn;
    if (bb >= kVoteBins) bb -= kVoteBins;
    const u32 c = s_bin[bb];
    if (c & 0xFFFFu) atomicAdd(&table[bb], c & 0xFFFFu);
    if (c >> 16) atomicAdd(&coarse[bb], c >> 16);
  }
}
static_assert(kCoarseBins == kVoteBins && kLongVoteTile < (1u << 16), "k_period_votes_long: one LDS word per bin of both tables, 16 bits each");
// (one workgroup) the coarse bins with `need` votes or more into sel[] (the first kLongSel of them), their number into *count
__global__ __launch_bounds__(1024) void k_long_coarse_pick(const u32* __restrict__ coarse, u32 need, u32* __restrict__ sel, u32* __restrict__ count) {
  __shared__ u32 s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  for (u32 b = threadIdx.x; b < kCoarseBins; b += 1024u) {
    const u32 v = coarse[b];
    if (v && v >= need) {
      const u32 at = atomicAdd(&s_count, 1u);
      if (at < kLongSel) sel[at] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *count = s_count;
}
// Sweep 2: workgroup (x, y) votes over tile x of the list for the coarse bins sel[y * kFineGroup ...] alone, by d & 4095
template <bool RUNS_OUT>
__global__ __launch_bounds__(kVoteTPB) void k_period_votes_fine(const u64* __restrict__ ks, const u32* __restrict__ vs, u32 m, u64 kmask,
                                                                const u32* __restrict__ k1, const u32* __restrict__ sel, u32 n_sel,
                                                                u32* __restrict__ fine, u32 dmax) {
  __shared__ u32 s_fine[kFineGroup * kFineBins];
  const u32 g0 = blockIdx.y * kFineGroup;
  if (g0 >= n_sel) return;
  const u32 cnt = min(kFineGroup, n_sel - g0), bins = cnt * kFineBins;
  u32 c[kFineGroup];
#pragma unroll
  for (u32 g = 0; g < kFineGroup; ++g) c[g] = g < cnt ? sel[g0 + g] : 0xFFFFFFFFu;
  for (u32 b = threadIdx.x; b < bins; b += kVoteTPB) s_fine[b] = 0;
  __syncthreads();
  const u32 base = blockIdx.x * kLongVoteTile;
  for (u32 j = 0; j < kLongVoteTile / kVoteTPB; ++j) {
    const u32 i = base + j * kVoteTPB + threadIdx.x;
    if (i + 1u >= m) break;
    if (((ks[i] ^ ks[i + 1u]) & kmask) != 0ull) continue;
    const u32 a = vs[i], b = vs[i + 1u];
    const u32 d = a > b ? a - b : b - a;
    if (d <= kPeriodMax || d > dmax) continue;
    const u32 cb = d >> kCoarseShift;
    u32 slot = kFineGroup;
#pragma unroll
    for (u32 g = 0; g < kFineGroup; ++g) if (cb == c[g]) slot = g;
    if (slot == kFineGroup) continue;
    if constexpr (RUNS_OUT) { if (k1[min(a, b)] > d) continue; }
    atomicAdd(&s_fine[slot * kFineBins + (d & (kFineBins - 1u))], 1u);
  }
  __syncthreads();
  const u32 turn = (blockIdx.x * 67u) % bins;
  u32* const out = fine + (size_t)g0 * kFineBins;
  for (u32 b = threadIdx.x; b < bins; b += kVoteTPB) {
    u32 bb = b + turn;
    if (bb >= bins) bb -= bins;
    const u32 v = s_fine[bb];
    if (v) atomicAdd(&out[bb], v);
  }
}
// (one workgroup) k_period_winners over the short table and the n_sel fine tables together: the distance of word e of fine
// table q is sel[q] << 12 | e.  A key is votes << 32 | kLongKeyBase - distance.
constexpr u32 kLongKeyBase = 1u << 25;
__global__ __launch_bounds__(1024) void k_long_period_winners(const u32* __restrict__ table, const u32* __restrict__ sel, u32 n_sel,
                                                              const u32* __restrict__ fine, u32 need, u32* __restrict__ out) {
  __shared__ u64 s_best[1024];
  const u32 words = n_sel * kFineBins;
  u64 below = ~0ull;
  for (u32 i = 0; i < kPeriodCandidates; ++i) {
    u64 best = 0;
    for (u32 b = threadIdx.x; b < kVoteBins; b += 1024u) {
      const u32 v = b >= 2u ? table[b] : 0u;
      const u64 key = (v >= need && v) ? ((u64)v << 32) | (u64)(kLongKeyBase - b) : 0ull;
      if (key < below && key > best) best = key;
    }
    for (u32 e = threadIdx.x; e < words; e += 1024u) {
      const u32 v = fine[e], d = (sel[e >> kCoarseShift] << kCoarseShift) | (e & (kFineBins - 1u));
      const u64 key = (v >= need && v && d > kPeriodMax) ? ((u64)v << 32) | (u64)(kLongKeyBase - d) : 0ull;
      if (key < below && key > best) best = key;
    }
    s_best[threadIdx.x] = best;
    __syncthreads();
    for (u32 o = 512; o > 0; o >>= 1) {
      if (threadIdx.x < o) { const u64 v = s_best[threadIdx.x + o]; if (v > s_best[threadIdx.x]) s_best[threadIdx.x] = v; }
      __syncthreads();
    }
    below = s_best[0];
    __syncthreads();
    if (threadIdx.x == 0) {
      out[2u * i] = below ? kLongKeyBase - (u32)below : 0u;
      out[2u * i + 1u] = (u32)(below >> 32);
    }
  }
}
// The probe for p > kPeriodMax, k_period_probe's answer: one workgroup per window of `span` positions from p + i * span
// on, 256 threads x 64 positions a turn by period_breaks' 16-byte loads of T beside T - p.  The workgroup leaves at the
// first turn that holds a break; a window without one sets the flag, and workgroups that find it set do not begin.
__global__ __launch_bounds__(256) void k_period_probe_wide(const u8* __restrict__ T, u32 n, u32 p, u32 span, u32* flag) {
  __shared__ u32 s_set;
  if (threadIdx.x == 0) s_set = *reinterpret_cast<volatile u32*>(flag);
  __syncthreads();
  if (s_set) return;
  const u64 x0 = (u64)p + (u64)blockIdx.x * span;
  if (x0 + span > (u64)n) return;
  const u32 lo = (u32)x0, hi = lo + span;
  for (u32 base = lo & ~63u; base < hi; base += 256u * 64u) {   // (the host keeps n two tiles below 2^32: no wrap)
    const u32 at = base + threadIdx.x * 64u;
    u64 mask = at < hi ? period_breaks(T, at, n, p) : 0ull;
    if (at < lo) mask &= ~0ull << (lo - at);                    // (thread 0 of the first turn alone: lo - at < 64)
    if (at < hi && hi - at < 64u) mask &= (1ull << (hi - at)) - 1ull;
    if (__syncthreads_or(mask != 0ull)) return;
  }
  if (threadIdx.x == 0) atomicOr(flag, 1u);
}

// Dense route, step 3 (after ALL of rank[] is updated): the next round's sort input, written
// over the records.  Record p of suffix s with dense group number grp (all ones: finished)
// becomes key = grp << b2 | rank[s+h]+1 (0 when s+h is past the end; with runs in play run_key2: the run step's
// closed-form key, or the look-up at the member's own offset) | T[s-1] << 56 (emit),
// value = s; finished suffixes become the all-ones key, which the sort's first pass drops.
// The records are in window order of s and h is small against a window at the dense stage, so
// rank[s+h] and T[s-1] are read from the window being swept, not at random.  The chunk's items
// are written back in their LDS order (any order will do: the sort that follows does not care).
__global__ __launch_bounds__(kWinTPB) void k_gather_dense(u64* __restrict__ rec, u32* __restrict__ val,
                                                          const u32* __restrict__ rank,
                                                          const u8* __restrict__ T, u32 m, u32 n, u32 h,
                                                          int b2, int emit, int bin_shift, RunKeys rk) {
  __shared__ u32 s_cnt[256], scr[kWinTPB / kWave + 1];
  __shared__ u32 s_s[kWinTile], s_g[kWinTile];
  u32 blk;
  if (!win_chunk(m, &blk)) return;
  const u32 base = blk * (u32)kWinTile;
  const u32 p0 = base + threadIdx.x;
  u32 s[kWinE], g[kWinE], bin[kWinE], slot[kWinE], okm = 0;
#pragma unroll
  for (int e = 0; e < kWinE; ++e) {
    const u32 p = p0 + e * kWinTPB;
    const bool ok = p < m;
    s[e] = ok ? (u32)(rec[p] >> 32) : 0u;
    g[e] = ok ? val[p] : 0xFFFFFFFFu;
    bin[e] = (s[e] >> bin_shift) & 255u;
    okm |= (ok ? 1u : 0u) << e;
  }
  win_places(bin, okm, slot, s_cnt, scr);
#pragma unroll
  for (int e = 0; e < kWinE; ++e) if ((okm >> e) & 1u) { s_s[slot[e]] = s[e]; s_g[slot[e]] = g[e]; }
  __syncthreads();
  const u32 count = min((u32)kWinTile, m - base);
  for (u32 i = threadIdx.x; i < count; i += kWinTPB) {
    const u32 ss = s_s[i], gg = s_g[i];
    u64 key = ~0ull;
    if (gg != 0xFFFFFFFFu) {
      const u64 r = run_key2(rk, rank, T, ss, n, h, b2);
      const u32 c = (emit && ss) ? T[ss - 1u] : 0u;
      key = ((u64)gg << b2) | r | ((u64)c << 56);
    }
    rec[base + i] = key;
    val[base + i] = ss;
  }
}

// ---------------------------------------------------------------------------------------
// K5  second sort key of a doubling round:  (group << b2) | key2,  key2 = rank[s+h] + 1,
//     or 0 for the one suffix whose h-successor is the empty suffix.
// ---------------------------------------------------------------------------------------
//     achr (may be null): the suffix's carried character, put into bits 56..63 of the key.
__global__ __launch_bounds__(256) void k_gather_key2(const u32* __restrict__ aidx,
                                                     const u32* __restrict__ agrp,
                                                     const u32* __restrict__ rank,
                                                     const u8* __restrict__ achr,
                                                     u64* __restrict__ key, u32 m, u32 n, u32 h,
                                                     int b2, RunKeys rk, const u8* __restrict__ T) {
  const u32 p0 = blockIdx.x * (256u * kSimpleE) + threadIdx.x;
  if (rk.mode != 0) {
    // a block with long runs (see RunKeys): the run step's keys, or the later rounds' look-ups at each member's own offset
#pragma unroll
    for (int e = 0; e < kSimpleE; ++e) {
      const u32 p = p0 + e * 256u;
      if (p < m) key[p] = ((u64)agrp[p] << b2) | run_key2(rk, rank, T, aidx[p], n, h, b2) | (achr ? (u64)achr[p] << 56 : 0ull);
    }
    return;
  }
  u64 t[kSimpleE];
  u32 r[kSimpleE], g[kSimpleE];
#pragma unroll
  for (int e = 0; e < kSimpleE; ++e) {
    const u32 p = p0 + e * 256u;
    t[e] = p < m ? (u64)aidx[p] + (u64)h : ~0ull;
    g[e] = p < m ? agrp[p] : 0u;
  }
#pragma unroll
  for (int e = 0; e < kSimpleE; ++e) r[e] = (t[e] < (u64)n) ? rank[t[e]] + 1u : 0u;
#pragma unroll
  for (int e = 0; e < kSimpleE; ++e) {
    const u32 p = p0 + e * 256u;
    if (p < m) key[p] = ((u64)g[e] << b2) | (u64)r[e] | (achr ? (u64)achr[p] << 56 : 0ull);
  }
}

// Text round (after the finisher, for the groups it could not take): the second sort key is the
// suffix's next c characters themselves, no rank[] needed:
//   key = group << (8c + 4) | characters << 4 | t,   t = c - (characters past the end of T), so that of
// suffixes equal on those characters the one that ends there comes first, shortest first.
__global__ __launch_bounds__(256) void k_gather_text(const u32* __restrict__ aidx, const u32* __restrict__ agrp,
                                                     const u8* __restrict__ T, const u8* __restrict__ achr,
                                                     u64* __restrict__ key, u32 m, u32 n, u32 h, u32 c, RunKeys rk) {
  const u32 p = blockIdx.x * 256u + threadIdx.x;
  if (p >= m) return;
  const u32 s = aidx[p];
  u64 c0, c1;
  // s + h < 2^31: h stays small in text rounds; a run's member reads behind its run (RunKeys), which may be anywhere up to n:
  // its sub-group shares its k characters and what the text rounds since the run step (at depth h_split) have compared
  u64 at = (u64)s + h;
  if (rk.mode == 2) {                                    // (rank[] is refined between rounds, the text is not: max(h, k) would read the same characters again)
    const u32 kk = rk.merged ? rk.k[s] & kStepLength : rk.k[s];
    // (merged: text rounds follow first-round steps only, which all ran at h_split, and a taken suffix has kk >= h_split)
    if (rk.merged ? kk != 0u : kk >= rk.h_split) at = (u64)s + max((u64)h, (u64)kk + (h - rk.h_split));
  }
  fin_chars(T, (u32)min(at, (u64)n), n, &c0, &c1);
  const u64 chars = c0 >> (64u - 8u * c);
  const u64 end = at + c;
  const u32 over = end > (u64)n ? (u32)min((u64)c, end - (u64)n) : 0u;
  key[p] = ((u64)agrp[p] << (8u * c + 4u)) | (chars << 4) | (u64)(c - over) | (achr ? (u64)achr[p] << 56 : 0ull);
}

// ---------------------------------------------------------------------------------------
// K9  BWT gather: out[j] = T[SA[j]-1]; the row of suffix 0 is the end-of-block row.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bwt_gather(const u32* __restrict__ SA,
                                                    const u8* __restrict__ T,
                                                    u8* __restrict__ out, u32 n,
                                                    u32* __restrict__ pidx) {
  const u32 w = blockIdx.x * 256u + threadIdx.x;
  const u32 j0 = w * 4u;
  if (j0 >= n) return;
  u32 word = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const u32 j = j0 + b;
    if (j < n) {
      const u32 s = SA[j];
      u32 c = 0;
      if (s) c = T[s - 1];
      else *pidx = j;
      word |= c << (8 * b);
    }
  }
  reinterpret_cast<u32*>(out)[w] = word;
}

// End-of-block patch + LF powers.  block mode: out[pidx] = out[n-1] (BWTransform.cpp:60);
// raw mode: out[pidx] = the input byte at pidx (divsufsort.c:507-511 leaves it untouched).
// LF[0] = pidx, LF[k] = ISA[n - k*(n/nLF)] (divsufsort.c:337-338,350,381,390).
// last_char (emitting rankers): the character of row n-1, which has no slot in a block's output.
// lf_noted: LF[1..] were noted as the suffixes became final (lf_note); rank[] is not complete then.
__global__ void k_finalize(u8* __restrict__ out, const u8* __restrict__ T,
                           const u32* __restrict__ rank, u32* __restrict__ lf, u32 n_lf, u32 n,
                           const u32* __restrict__ pidx, int raw, const u32* __restrict__ last_char, int lf_noted = 0) {
  const u32 p = *pidx;
  const u32 k = threadIdx.x;
  if (k == 0) {
    if (raw) out[p] = T[p];
    else if (p + 1u < n) out[p] = last_char ? (u8)*last_char : out[n - 1];
    lf[0] = p;
  } else if (k < n_lf && !lf_noted) {
    const u32 x = n / n_lf;
    lf[k] = rank[n - k * x];
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// The switches: off is a value that begins with '0'; a number is clamped to [lo, hi], stored only when the switch is set (-> true).
static bool env_off(const char* name) { const char* v = std::getenv(name); return v && v[0] == '0'; }
static bool env_is(const char* name, const char* value) { const char* v = std::getenv(name); return v && std::strcmp(v, value) == 0; }
static bool env_int(const char* name, int* dst, int lo = INT_MIN, int hi = INT_MAX) {
  const char* v = std::getenv(name);
  if (v) *dst = std::min(hi, std::max(lo, std::atoi(v)));
  return v != nullptr;
}
static inline bool debug_on() { return std::getenv("BWTC_HIP_DEBUG") != nullptr; }

static u64 align_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

struct ArenaPlan {
  u64 off_T, off_out, off_in, off_SA, off_rank, off_R1, off_R2, off_V0, off_V1, off_G0, off_G1,
      off_GRP, off_C0, off_C1, off_P0, off_P1, off_W0, off_W1, off_table, off_partial, off_aggA, off_aggB, off_aggC, off_agg_part, off_small, off_ent, off_comp, off_sweep, off_parkS, off_parkHP, off_hardS, off_hardHP, off_hardC, off_LP0, off_LH0, off_LH1, off_LC1, off_US, off_UR, off_pairs, off_codes, off_runK, off_runF, off_runB, off_votes, off_lvotes, total;
};

// The entries an array of a finisher list holds (fin_room: what a pass needs of them), in a context of capacity cap.
// (Whether that is room enough for the wide shape is ADVICE.md's item; the formula is as it was.)
static constexpr u64 fin_list_cap(u64 cap) { return cap + cap / 128 + 65536; }

static ArenaPlan plan_arena(u64 cap) {
  ArenaPlan a;
  u64 o = 0;
  auto take = [&](u64 bytes) { u64 r = o; o = align_up(o + bytes, 256); return r; };
  a.off_T = take(cap + kTextPad + kLoadTile);
  a.off_out = take(cap + 64);
  a.off_in = take(cap + 64);
  a.off_SA = take(cap * 4);
  a.off_rank = take(cap * 4);
  a.off_R1 = take(cap * 8);
  a.off_R2 = take(cap * 8);
  // (the finisher's lists live in regions sized for the most their workgroups can leave: up to 17 strides beyond the entries)
  const u64 lcap = fin_list_cap(cap);
  a.off_V0 = take(lcap * 4);
  a.off_V1 = take(lcap * 4);
  a.off_G0 = take(lcap * 4);
  a.off_G1 = take(lcap * 4);
  a.off_GRP = take(lcap * 4);
  a.off_C0 = take(2 * lcap + 64);      // carried characters; the finisher's lists keep 16 bits per entry (character, depth)
  a.off_C1 = take(2 * lcap + 64);
  a.off_P0 = take(cap + 64);
  a.off_P1 = take(cap + 64);
  a.off_W0 = take(lcap * 4);           // (W0 and W1 are neighbours: together also one region of 8 * cap bytes)
  a.off_W1 = take(lcap * 4);
  a.off_table = take(radix_table_words(cap) * 4);
  a.off_partial = take(radix_partial_words(cap) * 4);
  const u64 rr_tiles = (cap + kRrTile - 1) / kRrTile + 1;
  a.off_aggA = take((rr_tiles + 64) * 4);   // (64 spare words each: the test hooks' canaries behind the last tile's entry)
  a.off_aggB = take((rr_tiles + 64) * 4);
  a.off_aggC = take((rr_tiles + 64) * 4);
  a.off_agg_part = take((rr_tiles / 4096 + 2) * 12);
  a.off_small = take(1024 * 4);
  a.off_ent = take(2u << 20);
  a.off_comp = take(huffman_compress_bound(cap));
  a.off_sweep = take(SweepWs::small_words() * 4);
  a.off_parkS = take(cap * 4);          // finisher route: what waits for the rounds (the passes' leftovers, groups the code rounds gave up on)
  a.off_parkHP = take(cap * 8);
  a.off_hardS = take(lcap * 4);         // finisher route: the groups too large for a window, until they join the waiting list;
  a.off_hardHP = take(lcap * 8);        //   then, with the arrays below, the two homes of the local list and its rank notes (k_finish<RANK>)
  a.off_hardC = take(lcap * 2 + 64);
  a.off_LP0 = take(lcap * 4);
  a.off_LH0 = take(lcap * 4);
  a.off_LH1 = take(lcap * 4);
  a.off_LC1 = take(lcap * 2 + 64);
  a.off_US = take(lcap * 4);
  a.off_UR = take(lcap * 4);
  a.off_pairs = take((u64)kPairReplicas * 65536 * 4);
  a.off_codes = take((u64)kCodeRows * 256 * 4);
  a.off_runK = take(cap * 4);            // runs: k[] of every suffix, and the run-length pass's two words per tile
  const u64 run_tiles = 2 * ((cap + kRunTile - 1) / kRunTile) + 2;   // (the tiles reach n + p, and a long period is below n: stretch_lengths)
  a.off_runF = take(run_tiles * 4);
  a.off_runB = take(run_tiles * 4);
  a.off_votes = take((u64)kVoteBins * 4);   // periods: the finder's vote table
  a.off_lvotes = take(((u64)kLongFineAt + (u64)kLongSel * kFineBins) * 4);   // long periods: the coarse table, the selected bins, the fine tables
  a.total = o;
  return a;
}

// Contexts for tiny blocks still get room for the entropy front-ends' per-section tables
// (256 sections x 4096 run lengths).
static u64 arena_items(u32 max_block) { return std::max<u64>((u64)max_block + 1, 1u << 20); }

u64 BwtEngine::workspace_bytes(u32 max_block) { return plan_arena(arena_items(max_block)).total; }

int BwtEngine::init(int dev, u32 max_block_size) {
  device = dev;
  max_block = max_block_size;
  cap = arena_items(max_block_size);
  std::memset(&stats, 0, sizeof stats);
  BWTC_HIP_TRY(hipSetDevice(dev));
  BWTC_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  const ArenaPlan a = plan_arena(cap);
  arena_bytes = a.total;
  BWTC_HIP_TRY(hipMalloc(&arena, arena_bytes));
  u8* base = static_cast<u8*>(arena);
  d_T = base + a.off_T;
  d_out = base + a.off_out;
  d_in = base + a.off_in;
  d_SA = reinterpret_cast<u32*>(base + a.off_SA);
  d_rank = reinterpret_cast<u32*>(base + a.off_rank);
  d_R1 = base + a.off_R1;
  d_R2 = base + a.off_R2;
  d_V0 = reinterpret_cast<u32*>(base + a.off_V0);
  d_V1 = reinterpret_cast<u32*>(base + a.off_V1);
  d_G0 = reinterpret_cast<u32*>(base + a.off_G0);
  d_G1 = reinterpret_cast<u32*>(base + a.off_G1);
  d_GRP = reinterpret_cast<u32*>(base + a.off_GRP);
  d_C0 = base + a.off_C0;
  d_C1 = base + a.off_C1;
  d_P0 = base + a.off_P0;
  d_P1 = base + a.off_P1;
  d_W0 = reinterpret_cast<u32*>(base + a.off_W0);
  d_W1 = reinterpret_cast<u32*>(base + a.off_W1);
  d_table = reinterpret_cast<u32*>(base + a.off_table);
  d_partial = reinterpret_cast<u32*>(base + a.off_partial);
  d_aggA = reinterpret_cast<u32*>(base + a.off_aggA);
  d_aggB = reinterpret_cast<u32*>(base + a.off_aggB);
  d_aggC = reinterpret_cast<u32*>(base + a.off_aggC);
  d_agg_part = reinterpret_cast<u32*>(base + a.off_agg_part);
  d_small = reinterpret_cast<u32*>(base + a.off_small);
  d_ent = base + a.off_ent;
  d_comp = base + a.off_comp;
  d_sweep = reinterpret_cast<u32*>(base + a.off_sweep);
  d_parkS = reinterpret_cast<u32*>(base + a.off_parkS);
  d_parkHP = reinterpret_cast<u64*>(base + a.off_parkHP);
  d_hardS = reinterpret_cast<u32*>(base + a.off_hardS);
  d_hardHP = reinterpret_cast<u64*>(base + a.off_hardHP);
  d_hardC = reinterpret_cast<unsigned short*>(base + a.off_hardC);
  d_LP0 = reinterpret_cast<u32*>(base + a.off_LP0);
  d_LH0 = reinterpret_cast<u32*>(base + a.off_LH0);
  d_LH1 = reinterpret_cast<u32*>(base + a.off_LH1);
  d_LC1 = reinterpret_cast<unsigned short*>(base + a.off_LC1);
  d_US = reinterpret_cast<u32*>(base + a.off_US);
  d_UR = reinterpret_cast<u32*>(base + a.off_UR);
  d_pairs = reinterpret_cast<u32*>(base + a.off_pairs);
  d_codes = reinterpret_cast<u32*>(base + a.off_codes);
  d_runK = reinterpret_cast<u32*>(base + a.off_runK);
  d_runF = reinterpret_cast<u32*>(base + a.off_runF);
  d_runB = reinterpret_cast<u32*>(base + a.off_runB);
  d_votes = reinterpret_cast<u32*>(base + a.off_votes);
  d_lvotes = reinterpret_cast<u32*>(base + a.off_lvotes);
  use_sweep = env_is("BWTC_HIP_SORT", "sweep");
  wavelet_on_host = env_is("BWTC_HIP_WAVELET", "host");
  device_models = !env_is("BWTC_HIP_MODELS", "host"); letter_models = env_is("BWTC_HIP_LETTER_MODELS", "1"); models_side_stream = !env_off("BWTC_HIP_MODELS_STREAM");
  int v = 0;
  if (env_int("BWTC_HIP_WAVELET_DEPTH", &v) && v > 0) max_inflight = (unsigned)v;
  dense_route = !env_off("BWTC_HIP_DENSE");
  no_emit = std::getenv("BWTC_HIP_NO_EMIT") != nullptr;
  if (env_int("BWTC_HIP_WINDOW_BITS", &v) && v > 0) window_bits = std::min(24, v);
  digit_planes = !env_off("BWTC_HIP_PLANES"); split_index = !env_off("BWTC_HIP_SPLIT_INDEX");
  if (env_int("BWTC_HIP_GRAMS", &gram_count_override)) gram_keys = !env_off("BWTC_HIP_GRAMS");   // 0: base-sigma keys only; N > 0: N grams per key
  long_keys = !env_off("BWTC_HIP_LONG");
  env_int("BWTC_HIP_LONG_G2", &long_grams_override);
  const bool group_given = env_int("BWTC_HIP_FIN_GROUP", &fin_max_group), window_given = env_int("BWTC_HIP_FIN_WINDOW", &fin_window);
  fin_shape_fixed = group_given || window_given;
  fin_wide_short = !env_off("BWTC_HIP_FIN_WIDE");
  fin_window = fin_window >= 2048 ? 2048 : 1024;
  fin_max_group = fin_max_group >= 1024 ? 1024 : fin_max_group >= 512 ? 512 : 256;
  if (fin_max_group >= fin_window) fin_max_group = fin_window / 2;
  code_keys = !env_is("BWTC_HIP_KEYS", "grams");
  env_int("BWTC_HIP_CODE_BITS", &code_bits, 40, 72);
  finisher = !env_off("BWTC_HIP_FINISHER");
  gm_partition_lines = env_is("BWTC_HIP_GM_PARTITION", "lines");
  wt_segmented = !env_off("BWTC_HIP_SEG_STEPS");
  gram_min_n = kGramMinN;
  if (env_int("BWTC_HIP_GRAM_MIN_N", &v, 64)) gram_min_n = (u32)v;   // tests: small blocks through the gram / long-key routes
  if (env_int("BWTC_HIP_LONG_E", &v)) long_items_per_thread = v == 6 ? 6 : 8;
  env_int("BWTC_HIP_FIN_PASSES", &fin_max_passes, 0); env_int("BWTC_HIP_FIN_WORDS", &fin_words, 2, 4);
  long_direct = !env_off("BWTC_HIP_LONG_DIRECT");
  env_int("BWTC_HIP_FIN_ROUNDS", &fin_rounds, 1, 4);
  run_ranks = !env_off("BWTC_HIP_RUNS"); period_ranks = !env_off("BWTC_HIP_PERIODS");
  if (env_int("BWTC_HIP_PERIOD", &v, 0, (int)kPeriodMax)) period_forced = (u32)v;
  copy_rounds = env_is("BWTC_HIP_COPIES", "1");
  long_periods = env_is("BWTC_HIP_LONG_PERIODS", "1");
  // (BWTC_HIP_LONG_PERIOD=p, under the switch alone: what BWTC_HIP_PERIOD is below kPeriodMax, for tests)
  if (long_periods && env_int("BWTC_HIP_LONG_PERIOD", &v, (int)kPeriodMax + 1, (int)kLongPeriodMax)) period_forced = (u32)v;
  multi_steps = env_is("BWTC_HIP_MULTI", "1");
  mixed_steps = env_is("BWTC_HIP_MIXED", "1") || multi_steps;   // (BWTC_HIP_MULTI switches MIXED's rules on)
  local_rounds = !env_off("BWTC_HIP_LOCAL_ROUNDS");
  if (env_int("BWTC_HIP_FIN_FLOOR", &v, 0)) fin_floor = (u32)v;
  text_rounds_fixed = env_int("BWTC_HIP_TEXT_ROUNDS", &text_rounds, 0);
  if (env_int("BWTC_HIP_HUGE_MI", &v) && v > 0) huge_group_elements = (u64)v << 20;
  // Opt-in (BWTC_HIP_SCAN=chained): measured on MI355X the single-launch scan is SLOWER for the
  // sorter's tables (63 us against 25 + 11 + 6 us for 8.4 M words: 2048 tiles are too few to hide
  // the look-back hops), so the three-launch form stays the default.
  if (env_is("BWTC_HIP_SCAN", "chained")) {
    scan_chain.cap_tiles = (u32)(cap / kScanTile + 4096);
    BWTC_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&scan_chain.status), ((u64)scan_chain.cap_tiles + 1) * 8));
    BWTC_HIP_TRY(hipMemset(scan_chain.status, 0, ((u64)scan_chain.cap_tiles + 1) * 8));
    scan_chain.ticket = scan_chain.status + scan_chain.cap_tiles;     // the last word
    scan_chain.err = d_small + 522;                                  // kSmallError: read back with every ranking step's counts
    scan_chain.stream = stream;                                      // the transform's, the stream kernels' (and the farm's model passes)
    scan_chain.issued = 0;
    scan_chain.epoch = 0;
  }
  BWTC_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_small), 1024 * 4, hipHostMallocDefault));
  BWTC_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_stage), cap + 32, hipHostMallocDefault));
  BWTC_HIP_TRY(hipEventCreateWithFlags(&ev_wait, hipEventBlockingSync | hipEventDisableTiming));
  wait_mode = env_is("BWTC_HIP_SYNC", "spin") ? 1 : env_is("BWTC_HIP_SYNC", "block") ? 2 : 0;
  BWTC_HIP_TRY(hipEventCreate(&ev_begin));
  BWTC_HIP_TRY(hipEventCreate(&ev_end));
  for (int i = 0; i < kMaxSortEvents; ++i) BWTC_HIP_TRY(hipEventCreate(&ev_sort[i]));
  return 0;
}

hipError_t BwtEngine::ensure_d2h_stream() {
  if (d2h_stream) return hipSuccess;
  hipError_t rc = hipStreamCreateWithFlags(&d2h_stream, hipStreamNonBlocking);
  if (rc != hipSuccess) return rc;
  rc = hipEventCreateWithFlags(&ev_packed, hipEventDisableTiming);
  if (rc != hipSuccess) return rc;
  rc = hipEventCreateWithFlags(&ev_models, hipEventDisableTiming);
  if (rc != hipSuccess) return rc;
  return hipEventCreateWithFlags(&ev_codes, hipEventBlockingSync | hipEventDisableTiming);
}

hipError_t BwtEngine::codes_wait() {
  if (!codes_in_flight) return hipSuccess;
  codes_in_flight = false;
  return sleepy_wait(ev_codes, kWaitSlots - 1);
}

// A wait that gives the CPU away.  On this runtime hipEventSynchronize spins even on an event made with
// hipEventBlockingSync (scripts/r4/wait_probe.py: the waiting thread's CPU time equals the wall time), and
// with the 'B' coder the thread that feeds the GPU then takes a whole CPU of a quota that the range coders
// need (measured: 0.04 CPU-seconds per 256 MiB block, a twentieth of sixteen CPUs).  So: poll the event
// and sleep in between, in slices that are a quarter of what the wait is still expected to take (every
// wait of a block has a slot, and remembers how long it took for the previous blocks), at most 200 us and
// at least 20 us -- a wake-up comes at most a slice late.
hipError_t BwtEngine::sleepy_wait(hipEvent_t ev, int slot) {
  using clk = std::chrono::steady_clock;
  static thread_local bool slack_set = false;
  if (!slack_set) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL); slack_set = true; }   // default: 50 us of slack on every sleep
  const auto t0 = clk::now();
  float& ema = wait_us[slot < 0 ? 0 : slot >= kWaitSlots ? kWaitSlots - 1 : slot];
  double slice = 20.0;
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    const double el = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
    if (q != hipErrorNotReady) {
      ema = ema > 0.f ? 0.5f * ema + 0.5f * (float)el : (float)el;
      return q;
    }
    const double left = (double)ema - el;
    if (left > 80.0) slice = std::min(200.0, left * 0.25);
    else slice = std::min(200.0, std::max(20.0, slice * 1.25));
    timespec ts;
    ts.tv_sec = 0;
    ts.tv_nsec = (long)(slice * 1e3);
    nanosleep(&ts, nullptr);
  }
}

int BwtEngine::reserve_run_arrays() {
  if (d_run_start[0] && d_run_start[1] && d_run_sym[0] && d_run_sym[1]) return 0;
  // all four or none: a half-allocated set left behind by a failed call would let the next
  // block's scanner write through a null pointer
  bool ok = true;
  for (int b = 0; b < 2; ++b) {
    if (!d_run_start[b]) ok = ok && hipMalloc(reinterpret_cast<void**>(&d_run_start[b]), (cap + 2) * 4) == hipSuccess;
    if (!d_run_sym[b]) ok = ok && hipMalloc(reinterpret_cast<void**>(&d_run_sym[b]), cap + 64) == hipSuccess;
  }
  if (ok) return 0;
  (void)hipGetLastError();
  for (int b = 0; b < 2; ++b) {
    if (d_run_start[b]) (void)hipFree(d_run_start[b]);
    if (d_run_sym[b]) (void)hipFree(d_run_sym[b]);
    d_run_start[b] = nullptr; d_run_sym[b] = nullptr;
  }
  return -2;
}

hipError_t BwtEngine::wait() {
  const bool block = wait_mode == 2 || (wait_mode == 0 && pipeline != nullptr);
  if (!block || !ev_wait) return hipStreamSynchronize(stream);
  hipError_t rc = hipEventRecord(ev_wait, stream);
  if (rc != hipSuccess) return rc;
  if (wait_seq < kWaitSlots - 2) ++wait_seq;
  return sleepy_wait(ev_wait, wait_seq);
}

void BwtEngine::release() {
  wavelet_pipeline_release(*this);
  if (stream) (void)hipStreamSynchronize(stream);
  if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); copy_stream = nullptr; }
  if (ev_copy) { (void)hipEventDestroy(ev_copy); ev_copy = nullptr; }
  if (d2h_stream) { (void)hipStreamSynchronize(d2h_stream); (void)hipStreamDestroy(d2h_stream); d2h_stream = nullptr; }
  if (ev_packed) { (void)hipEventDestroy(ev_packed); ev_packed = nullptr; }
  if (ev_models) { (void)hipEventDestroy(ev_models); ev_models = nullptr; }
  if (scan_chain.status) { (void)hipFree(scan_chain.status); scan_chain = ScanChain(); }
  if (d_gm) { (void)hipFree(d_gm); d_gm = nullptr; gm_bytes = 0; }
  if (d_gm_w) { (void)hipFree(d_gm_w); d_gm_w = nullptr; gm_w_bytes = 0; }
  if (h_gm) { (void)hipHostFree(h_gm); h_gm = nullptr; h_gm_bytes = 0; }
  if (ev_gm_upload) { (void)hipEventDestroy(ev_gm_upload); ev_gm_upload = nullptr; gm_upload_pending = false; }
  if (gm_stream) { (void)hipStreamSynchronize(gm_stream); (void)hipStreamDestroy(gm_stream); gm_stream = nullptr; }
  if (ev_packed_ready) { (void)hipEventDestroy(ev_packed_ready); ev_packed_ready = nullptr; }
  if (ev_gm_done) { (void)hipEventDestroy(ev_gm_done); ev_gm_done = nullptr; gm_done_pending = false; }
  if (ev_codes) { (void)hipEventDestroy(ev_codes); ev_codes = nullptr; }
  if (arena) (void)hipFree(arena);
  if (h_small) (void)hipHostFree(h_small);
  if (h_stage) (void)hipHostFree(h_stage);
  for (int b = 0; b < 2; ++b) {
    if (d_run_start[b]) (void)hipFree(d_run_start[b]);
    if (d_run_sym[b]) (void)hipFree(d_run_sym[b]);
    d_run_start[b] = nullptr; d_run_sym[b] = nullptr;
  }
  if (d_wt) (void)hipFree(d_wt);
  if (h_wt) (void)hipHostFree(h_wt);
  if (h_stats) (void)hipHostFree(h_stats);
  h_stats = nullptr; h_stats_bytes = 0;
  d_wt = nullptr; h_wt = nullptr; wt_bytes = 0; h_wt_bytes = 0;
  if (ev_wait) (void)hipEventDestroy(ev_wait);
  ev_wait = nullptr;
  if (ev_begin) (void)hipEventDestroy(ev_begin);
  if (ev_end) (void)hipEventDestroy(ev_end);
  for (int i = 0; i < kMaxSortEvents; ++i) if (ev_sort[i]) (void)hipEventDestroy(ev_sort[i]);
  probe.destroy();
  if (stream) (void)hipStreamDestroy(stream);
  arena = nullptr; h_small = nullptr; h_stage = nullptr; stream = nullptr;
}

static constexpr int kSmallFreqs = 0, kSmallLf = 256, kSmallPidx = 512, kSmallCounts = 520,
                     kSmallLut = 600,   // 64 words = 256-byte alphabet remap table
                     kSmallInv = 664;   // 64 words: dense code -> byte

// Width of the initial sort key.  The alphabet of T is remapped to dense w-bit codes and as
// many characters as fit are packed into a 32- or 64-bit key: 16 characters of DNA or 4 raw
// bytes in 32 bits, 9 characters of text in 64 bits.  32 bits are used when the order-0
// entropy says the 32-bit key already separates almost all suffixes; the choice only
// changes speed, never the result.
struct KeyPlan { int k, bits; u32 sigma; bool wide; u8 lut[256]; };

static int radix_passes(int bits) { return (bits + kRadixBits - 1) / kRadixBits; }
static u32 depth32(u64 h) { return (u32)std::min<u64>(h, 0xFFFFFFFFull); }   // a depth as the kernels take it
// rank[] in windows: a block's suffix numbers have `bits` bits; those from `lo` up pick the window (window_bits of
// them), the eight below them (from bin_shift) the bin inside it
struct WindowShifts { int bits, lo, bin_shift; };
static WindowShifts window_shifts(u32 n, int window_bits) {
  const int bits = bit_width_u64(n ? n - 1 : 0), lo = bits > window_bits ? bits - window_bits : 0;
  return WindowShifts{bits, lo, lo > 8 ? lo - 8 : 0};
}

// most characters per 8-bit radix pass for keys of at most `maxbits` bits; ties -> longer key
static void best_packing(u32 sigma, int maxbits, int* k_out, int* bits_out) {
  double best = -1.0;
  unsigned __int128 pow = 1;
  *k_out = 1; *bits_out = 8;
  for (int k = 1; k <= 32; ++k) {
    pow *= sigma;
    if (pow > ((unsigned __int128)1 << maxbits)) break;
    int bits = 0;
    for (unsigned __int128 v = pow - 1; v; v >>= 1) ++bits;
    if (bits == 0) bits = 1;
    const int passes = radix_passes(bits);
    const double ratio = (double)k / passes;
    if (ratio >= best) { best = ratio; *k_out = k; *bits_out = bits; }
  }
}

// lone_sentinel: the only zero byte of T is the terminator planted at T[n-1].  It then
// shares code 0 with the smallest real symbol instead of costing a code of its own (DNA
// stays at 4 symbols): a suffix whose key window reaches the terminator has length <= k,
// and all of those are split off as singletons in true order by the "shorter first" rule
// of the initial ranking, so the merged code is never compared.
static KeyPlan plan_keys(const u32 hist[256], u32 n, bool lone_sentinel, bool force_wide = false) {
  KeyPlan p;
  int sigma = 0;
  double total = 0.0, h0 = 0.0;
  for (int c = 0; c < 256; ++c) {
    p.lut[c] = (u8)(sigma > 255 ? 255 : sigma);
    const bool present = hist[c] != 0 && !(c == 0 && lone_sentinel);
    if (present) { ++sigma; total += hist[c]; }
  }
  for (int c = lone_sentinel ? 1 : 0; c < 256; ++c)
    if (hist[c]) { const double q = hist[c] / total; h0 -= q * std::log2(q); }
  p.sigma = (u32)(sigma < 2 ? 2 : sigma);
  int k32, b32, k64, b64;
  best_packing(p.sigma, 32, &k32, &b32);
  best_packing(p.sigma, 64, &k64, &b64);
  const double need = std::log2((double)n + 1.0) + 2.0;
  p.wide = (k64 > k32) && (force_wide || k32 * h0 < need);
  p.k = p.wide ? k64 : k32;
  p.bits = p.wide ? b64 : b32;
  return p;
}

static constexpr int kSmallError = 522;   // sticky error word of the chained sort
static constexpr int kSmallLastChar = 524; // character of row n-1 (emitting rankers, block mode)

// Blocks for which a round's sort key (group bits + rank bits) leaves bits 56..63 free for the
// carried character in every round: groups <= n/2, ranks <= n.
static int rank_bits(u32 n) { return bit_width_u64((u64)n + 1); }   // rank + 1 <= n, and never all ones
static bool can_carry(u32 n) { return rank_bits(n) + bit_width_u64(n / 2 ? n / 2 - 1 : 0) <= 56; }

// Algorithmic bytes of P radix passes over `items` items of `item` bytes (key `key` bytes): each pass reads a
// digit plane (or, without planes, the keys) for its histograms, reads and writes the items, and all but the
// last leave the next pass's plane.
static u64 sort_bytes(u64 items, int passes, int item, int key, bool planes) {
  if (passes <= 0) return 0;
  return items * (u64)passes * (u64)(2 * item + (planes ? 1 : key)) + (planes ? items * (u64)(passes - 1) : 0);
}

template <typename K>
void BwtEngine::sort_pairs(K* k0, K* k1, u32* v0, u32* v1, u64 n, int nbits, K** ks, u32** vs,
                           bool probe_it, int bit_lo, u64 n_holes, bool plane_ready, bool values_descend) {
  if (use_sweep && n_holes == 0) {
    SweepWs ws;
    ws.hist_all = d_sweep;
    ws.bases = d_sweep + kSweepMaxPasses * kChains * kRadixBins;
    ws.tickets = d_sweep + 2 * kSweepMaxPasses * kChains * kRadixBins;
    ws.status = d_table;
    ws.error = d_small + kSmallError;
    radix_sort_pairs_sweep<K>(k0, k1, v0, v1, n, nbits, ws, stream, ks, vs, probe_it ? &probe : nullptr,
                              bit_lo);
  } else {
    radix_sort_pairs<K>(k0, k1, v0, v1, n, nbits, d_table, d_partial, stream, ks, vs,
                        probe_it ? &probe : nullptr, bit_lo, false, false, n_holes,
                        digit_planes ? d_P0 : nullptr, digit_planes ? d_P1 : nullptr, plane_ready && digit_planes,
                        values_descend);
  }
}

// The window kernels' and the rounds' key kernels' launches: rank_step's and scatter_rank_pairs', and the test hooks'
// (BwtEngine::test_rank_scatter, test_round_keys).
static u32 win_grid(u32 m) { return (ceil_div(m, kWinTile) + 7u) / 8u * 8u; }   // whole eighths: win_chunk deals the chunks to the XCDs
static void launch_scatter_pairs(BwtEngine& e, const u32* where, const u32* what, u32 m, int bin_shift) {
  hipLaunchKernelGGL(k_scatter_pairs, dim3(win_grid(m)), dim3(kWinTPB), 0, e.stream, e.d_rank, where, what, m, bin_shift);
}
static void launch_scatter_dense(BwtEngine& e, const u64* rec, u32 m, int bin_shift) {
  hipLaunchKernelGGL(k_scatter_dense, dim3(win_grid(m)), dim3(kWinTPB), 0, e.stream, e.d_rank, rec, m, bin_shift);
}
static void launch_gather_dense(BwtEngine& e, u64* rec, u32* val, u32 m, u32 n, u32 h, int b2, int emit, int bin_shift, const RunKeys& rk) {
  hipLaunchKernelGGL(k_gather_dense, dim3(win_grid(m)), dim3(kWinTPB), 0, e.stream, rec, val, (const u32*)e.d_rank, (const u8*)e.d_T, m, n, h,
                     b2, emit, bin_shift, rk);
}
static void launch_gather_key2(BwtEngine& e, const u32* aidx, const u32* agrp, const u32* rank, const u8* achr, u64* key, u32 m, u32 n, u32 h,
                               int b2, const RunKeys& rk) {
  hipLaunchKernelGGL(k_gather_key2, dim3(ceil_div(m, 256 * kSimpleE)), dim3(256), 0, e.stream, aidx, agrp, rank, achr, key, m, n, h, b2, rk,
                     (const u8*)e.d_T);
}
static void launch_gather_text(BwtEngine& e, const u32* aidx, const u32* agrp, const u8* achr, u64* key, u32 m, u32 n, u32 h, u32 c,
                               const RunKeys& rk) {
  hipLaunchKernelGGL(k_gather_text, dim3(ceil_div(m, 256)), dim3(256), 0, e.stream, aidx, agrp, (const u8*)e.d_T, achr, key, m, n, h, c, rk);
}

// rank[pairs_s[i]] = pairs_r[i] for i < m, made cache-friendly: the pairs (two arrays of
// `cap` words inside one 8*cap-byte region) are first partitioned by the top 16 bits of the
// destination with two stable radix passes (tmp = another 8*cap-byte region), after which
// consecutive pairs write into the same 4096-word window of rank[].
void BwtEngine::scatter_rank_pairs(u32* pairs, u32* tmp, u32 m, u32 n) {
  const WindowShifts w = window_shifts(n, window_bits);
  u32 *ws = pairs, *wr = pairs + cap;
  if (m >= pairs_min && w.bits > 12) {
    sort_pairs<u32>(pairs, tmp, pairs + cap, tmp + cap, m, w.bits, &ws, &wr, false, w.lo);
    stats.alg_bytes += sort_bytes(m, radix_passes(w.bits - w.lo), 8, 4, digit_planes);
  }
  stats.alg_bytes += (u64)m * (8 + 4);                   // k_scatter_pairs
  launch_scatter_pairs(*this, ws, wr, m, w.bin_shift);
}

// The ranking kernels' one launch path: rank_step's, and the test hooks' (BwtEngine::test_rank_pass).  A form is what
// rank_step decides per list: 16-bit suffix halves (split) and long items (lng) -- both only for the initial ranking of
// 64-bit keys -- the MODE of k_rerank_apply and where a finished suffix's character comes from (RrEmit: 0 nothing is
// emitted, 1 bits 56..63 of a round's key, 2 T[s-1], 3 the long key's code).  Long items emit with form 3 or not at all,
// split ones with form 2 or not at all, an initial ranking never with form 1 (rr_emit_legal).  RrForm::emit is that
// form, as rank_step (rr_emit_form) or the hook's caller decided it: the launch code takes it as it stands and picks the
// instantiation by the items' shape and the form.  A form the shape does not have never gets there: rank_step makes none,
// and the hook refuses it before anything is launched.
// parts: kRrReduceScan -- the tile reduce and both scan phases, which leave the aggregates in d_aggA/B/C as apply reads
// them and the two counts in d_small -- and kRrApply; rank_step reads the counts between the two to choose the MODE.
struct RrForm { bool split, lng; int mode, emit; };
struct RrOut { u32* rank; u32* SA; u32* aidx; u32* aglob; u32* agrp; u32* pair_s; u32* pair_r; };
constexpr u32 kRrReduceScan = 1u, kRrApply = 2u;
static bool rr_emit_legal(bool split, bool lng, bool init, int emit) {
  return emit == 0 || emit == (lng ? 3 : 2) || (emit == 1 && !lng && !split && !init);
}
// long items carry the character's code in the key (3); the initial ranking of other items, and rounds whose keys had
// no room for it, read T[s-1] (2); rounds find it in bits 56..63 of their key (1)
static int rr_emit_form(bool emit, bool split, bool lng, bool init, bool carried) {
  return !emit ? 0 : lng ? 3 : (split || init || !carried) ? 2 : 1;
}

// both phases of the aggregates' scan over d_aggA/B/C, the parts in d_agg_part, the totals in d_small[kSmallCounts ..]
static void launch_rerank_scan(BwtEngine& e, u32 tiles) {
  u32* counts = e.d_small + kSmallCounts;
  const u32 parts = ceil_div(tiles, kRrScanChunk);
  hipLaunchKernelGGL(k_rerank_scan_tiles<0>, dim3(parts), dim3(1024), 0, e.stream, e.d_aggA, e.d_aggB, e.d_aggC, tiles, e.d_agg_part, counts);
  hipLaunchKernelGGL(k_rerank_scan_tiles<1>, dim3(parts), dim3(1024), 0, e.stream, e.d_aggA, e.d_aggB, e.d_aggC, tiles, e.d_agg_part, counts);
}
template <typename K, bool INIT, bool SP, bool LG>
static void launch_rerank_reduce(BwtEngine& e, u32 tiles, const K* ks, const u32* vs, u32 m, u32 n, u32 short_len, K kmask, const RrLong& lg) {
  hipLaunchKernelGGL((k_rerank_reduce<K, INIT, SP, LG>), dim3(tiles), dim3(kRrTPB), 0, e.stream, ks, vs, m, n, short_len, kmask,
                     e.d_aggA, e.d_aggB, e.d_aggC, lg);
}
template <typename K, bool INIT, int MODE, int EMIT, bool SP, bool LG>
static void launch_rerank_apply(BwtEngine& e, u32 tiles, const K* ks, const u32* vs, const u32* aglob, u32 m, u32 n, u32 short_len, K kmask,
                                const RrLong& lg, const RrOut& o, const RrEmit& re) {
  hipLaunchKernelGGL((k_rerank_apply<K, INIT, MODE, EMIT, SP, LG>), dim3(tiles), dim3(kRrTPB), 0, e.stream, ks, vs, aglob, m, n, short_len,
                     kmask, e.d_aggA, e.d_aggB, e.d_aggC, o.rank, o.SA, o.aidx, o.aglob, o.agrp, o.pair_s, o.pair_r, re, lg);
}
template <typename K, bool INIT, int MODE>
static void launch_rerank_mode(BwtEngine& e, u32 tiles, const RrForm& f, const K* ks, const u32* vs, const u32* aglob, u32 m, u32 n,
                               u32 short_len, K kmask, const RrLong& lg, const RrOut& o, const RrEmit& re) {
  constexpr bool kCanSplit = INIT && sizeof(K) == 8;
  if (f.lng && f.split) {                               // (the form is legal, rr_emit_legal: long and split items have one that emits)
    if (f.emit) launch_rerank_apply<K, INIT, MODE, 3, kCanSplit, kCanSplit>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
    else launch_rerank_apply<K, INIT, MODE, 0, kCanSplit, kCanSplit>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
  } else if (f.lng) {
    if (f.emit) launch_rerank_apply<K, INIT, MODE, 3, false, kCanSplit>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
    else launch_rerank_apply<K, INIT, MODE, 0, false, kCanSplit>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
  } else if (f.split) {
    if (f.emit) launch_rerank_apply<K, INIT, MODE, 2, kCanSplit, false>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
    else launch_rerank_apply<K, INIT, MODE, 0, kCanSplit, false>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
  } else if (f.emit == 0) launch_rerank_apply<K, INIT, MODE, 0, false, false>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
  else if (f.emit == 1) launch_rerank_apply<K, INIT, MODE, 1, false, false>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
  else launch_rerank_apply<K, INIT, MODE, 2, false, false>(e, tiles, ks, vs, aglob, m, n, short_len, kmask, lg, o, re);
}
template <typename K, bool INIT>
static void launch_rerank(BwtEngine& e, u32 parts, const RrForm& f, const K* ks, const u32* vs, const u32* aglob, u32 m, u32 n, u32 short_len,
                          K kmask, const RrLong& lg, const RrOut& o, const RrEmit& re) {
  constexpr bool kCanSplit = INIT && sizeof(K) == 8;
  const u32 tiles = ceil_div(m, kRrTile);
  if (parts & kRrReduceScan) {
    if (f.lng && f.split) launch_rerank_reduce<K, INIT, kCanSplit, kCanSplit>(e, tiles, ks, vs, m, n, short_len, kmask, lg);
    else if (f.lng) launch_rerank_reduce<K, INIT, false, kCanSplit>(e, tiles, ks, vs, m, n, short_len, kmask, lg);
    else if (f.split) launch_rerank_reduce<K, INIT, kCanSplit, false>(e, tiles, ks, vs, m, n, short_len, kmask, lg);
    else launch_rerank_reduce<K, INIT, false, false>(e, tiles, ks, vs, m, n, short_len, kmask, lg);
    launch_rerank_scan(e, tiles);
  }
  if (parts & kRrApply) {
    switch (f.mode) {
      case 0: launch_rerank_mode<K, INIT, 0>(e, tiles, f, ks, vs, aglob, m, n, short_len, kmask, lg, o, re); break;
      case 1: launch_rerank_mode<K, INIT, 1>(e, tiles, f, ks, vs, aglob, m, n, short_len, kmask, lg, o, re); break;
      case 2: launch_rerank_mode<K, INIT, 2>(e, tiles, f, ks, vs, aglob, m, n, short_len, kmask, lg, o, re); break;
      default: launch_rerank_mode<K, INIT, 3>(e, tiles, f, ks, vs, aglob, m, n, short_len, kmask, lg, o, re); break;
    }
  }
}

// A block's list between suffix_sort's stages: where it lives (home), what the last ranking step reported (res), the
// emitter with the spare plane of carried characters, and whether rank[] is complete.
struct SortList { u32 n; bool emit; BwtEngine::ListHome home; RrEmit re; BwtEngine::RankResult res; u8* achr_other; bool ranks_complete; };

// What differs between the calls of rank_step.  short_len, kmask, split and lg are an initial ranking's (a round's mask
// follows from whether its keys carry the character: carried_mask); kind and run_mode are a round's.
enum class RoundKind { kOrdinary, kText, kRaw };   // kText: rank[] is neither read nor (before it is complete) written; kRaw: the list goes back to its owner ungrouped
struct RankRequest {
  u32 m = 0;                     // entries of the list
  u64 h_next = 0;                // the depth the next list's second keys look up at
  u32 short_len = 0;             // suffixes of at most this length are finished by the initial ranking
  u64 kmask = ~0ull;             // the key's own bits
  u32 split = 0;                 // 16-bit suffix halves, the upper bits in the key
  const RrLong* lg = nullptr;    // long items: the second key word and the fields of the first
  RoundKind kind = RoundKind::kOrdinary;
  int run_mode = 0;              // RunKeys::mode of the next list's second keys
  bool copies = false;           // the round may be a copy round (run_rounds; run_mode is 0 then): the step decides by the next list's length
};
static u64 carried_mask(bool carried) { return carried ? (1ull << 56) - 1ull : ~0ull; }   // a round's keys: the character rides in bits 56..63

// The next list, shared by the routes that make one: the key kernel has left its keys in (ka, va) -- among them `holes`
// finished entries where drop_holes says that the sort's first pass drops them -- and they are sorted between (ka, va) and
// (kb, vb); the passes are counted, with key_bytes for what the route moved before the sort, and L.home moves to where
// the sort ended.  timed: between two of the block's sort events (while there are any left), with the probe.
int BwtEngine::next_list(SortList& L, u64* ka, u64* kb, u32* va, u32* vb, u32 m_next, int bits, u32 holes, bool drop_holes, u64 key_bytes, bool timed) {
  const bool events = timed && n_sort_events + 2 <= kMaxSortEvents;
  u64* ks = nullptr; u32* vs = nullptr;
  if (events) BWTC_HIP_TRY(hipEventRecord(ev_sort[n_sort_events++], stream));
  sort_pairs<u64>(ka, kb, va, vb, m_next, bits, &ks, &vs, timed, 0, (u64)holes);
  if (events) BWTC_HIP_TRY(hipEventRecord(ev_sort[n_sort_events++], stream));
  // the hole-dropping first pass reads every entry and writes the active ones; the others are plain passes
  const int plain = drop_holes ? std::max(0, radix_passes(bits) - 1) : radix_passes(bits);
  const u64 all = (u64)m_next + holes;
  stats.sort_pass_items += (drop_holes ? all : 0) + (u64)m_next * (u64)plain;
  stats.alg_bytes += key_bytes + (drop_holes ? all * (8 + 12) + (u64)m_next * 12 : 0) + sort_bytes(m_next, plain, 12, 8, digit_planes);
  L.home.advance(ks, vs);
  return 0;
}

// One ranking step over the sorted list in L.home (INIT: all suffixes by their initial key; rounds: the active list by
// (group, rank[s+h])): new ranks into rank[], finished suffixes out, and -- when anything stays active -- the next
// round's list, sorted, with L.home moved to it.  In three parts: decide (reduce and scan, the one read-back of the
// counts, the bit widths and the route), apply (one launch_rerank, its MODE and outputs by the route), and the next list
// (a key kernel by the route, then next_list).  L.res is what the step reports; L.home stays where it was when nothing
// stays active and in the routes that hand the list on raw -- in (home.v_free, home.slots_next, d_GRP) --, kFinish and
// kRaw.  L.re is copied: what the dense route sets in it is this call's.
//   kFinish   long items with an emitter: the finisher takes what is tied, rank[] is not written (MODE 3)
//   kDense    most of a long list stays active: window-ordered records (MODE 2)
//   kRaw      a round that may neither read the text nor double: the list back to its owner (MODE 3)
//   kTextRun  the run step before rank[] is complete: closed-form second keys, the others keep their groups (MODE 0)
//   kText     the next list's keys are characters of the text (MODE 0)
//   kPairs    list order, the new ranks as pairs through scatter_rank_pairs (MODE 1)
//   kShort    list order, rank[] written by apply (MODE 0)
enum class Route { kFinish, kDense, kRaw, kTextRun, kText, kPairs, kShort };
template <typename K, bool INIT>
int BwtEngine::rank_step(SortList& L, const RankRequest& rq) {
  constexpr bool kCanSplit = INIT && sizeof(K) == 8;
  ListHome& home = L.home;
  RankResult& res = L.res;
  RrEmit re = L.re;
  const u32 m = rq.m, n = L.n;
  const bool emit = L.emit, split = rq.split != 0;
  const bool carried = !INIT && res.carry;                // this list's keys hold the characters in bits 56..63 (only an emitting list's do)
  const K* ks = static_cast<const K*>(home.keys);
  const K kmask = INIT ? (K)rq.kmask : (K)carried_mask(carried);
  const bool lng = kCanSplit && rq.lg && rq.lg->w;        // items of the long-key sort (split: 16-bit values + upper bits in the key)
  const RrLong lgv = lng ? *rq.lg : RrLong();

  // ---- decide: how much stays active decides the route, so the counts are read before the apply kernel
  launch_rerank<K, INIT>(*this, kRrReduceScan, RrForm{split, lng, 0, 0}, ks, home.vals, (const u32*)nullptr, m, n, rq.short_len, kmask, lgv, RrOut{}, re);
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallCounts, d_small + kSmallCounts, 12, hipMemcpyDeviceToHost, stream));
  BWTC_HIP_TRY(wait());
  if (h_small[kSmallError] & 1u) { std::fprintf(stderr, "bwtc_hip: chained radix sort timed out\n"); return -3; }
  if (h_small[kSmallError]) return -3;                  // (2: k_code_build -- suffix_sort retries the block with gram keys)
  const u32 m_next = h_small[kSmallCounts], groups = h_small[kSmallCounts + 1];
  {
    // reduce and apply read the list (key, suffix, slot; the second key word of long items); apply writes a
    // byte (and in the finisher route the suffix) per finished suffix and a list entry / record per active one
    const u64 in_bytes = sizeof(K) + (lng ? 2 + 4 : split ? 2 : 4) + (INIT ? 0 : 4);
    stats.alg_bytes += (u64)m * in_bytes * 2 + (u64)(m - m_next) * 5 + (u64)m_next * 13;
  }
  const int b2 = rank_bits(n), b1 = bit_width_u64(groups ? groups - 1 : 0);
  // the run step's second key takes one bit more than a rank (RunKeys); a key that would not fit 64 bits: an ordinary round
  const bool run_now = !INIT && rq.run_mode == 1 && b1 + b2 + 1 <= 64;
  const int b2k = run_now ? b2 + 1 : b2;
  const int kbits = b1 + b2k;
  const StretchStep& step = blk.current_step();
  RunKeys rkeys{d_runK, run_now ? 0u : step.depth, run_now ? 1 : (rq.run_mode == 2 ? 2 : 0), step.p, blk.merged};
  // a copy round ("Copies"): the list is worth a pass over the block from n / 32 entries on (3.4 ps per byte for a
  // stretch pass against 116 ps per entry for a round); the marks want the list in list order, so not the dense route
  const bool copy_now = !INIT && rq.copies && rq.run_mode == 0 && rq.kind == RoundKind::kOrdinary && m_next > 0 && (u64)m_next * 32 >= n &&
                        (u64)n + 2ull * kRunTile <= 0xFFFFFFFFull;
  // a key of more than 56 bits has no room for the carried character (blocks above 256 MiB with many groups): the
  // next list then goes without, and its ranking reads T[s-1] for what it finishes
  const bool carry_next = emit && kbits <= 56;
  const bool text = rq.kind != RoundKind::kOrdinary;      // no look-ups in rank[]
  // Long items of which at most half is still tied (a 256 MiB text block: 21 %, a 1 GiB one: 37 %): the finisher
  // settles the rest by direct comparison (suffix_sort); rank[] is not written at all.  Above that the list is
  // dominated by long repeats and the doubling rounds are the better tool.
  // (with the last gram's low bits left out of the sort -- long_drop -- the list also holds what those bits would have
  // told apart: the bound is three fifths then)
  const Route route = lng && emit && finisher ? Route::kFinish
                      : !text && dense_route && m_next > 0 && (u64)m_next * 2 >= m && m >= pairs_min && !use_sweep && !copy_now ? Route::kDense
                      : rq.kind == RoundKind::kRaw ? Route::kRaw
                      : text ? (run_now && m_next > 0 ? Route::kTextRun : Route::kText)
                      : (m >= pairs_min || INIT) ? Route::kPairs : Route::kShort;
  const bool raw_list = route == Route::kFinish || route == Route::kRaw;
  res.m = m_next; res.groups = groups;
  res.ran_run = run_now; res.finish = route == Route::kFinish;
  // (the keys of the lists that the finisher's bridge and the text kernel make carry the character whenever there is an emitter)
  res.carry = route == Route::kFinish ? true : (route == Route::kRaw || route == Route::kText) ? emit : carry_next;
  if (route == Route::kText || route == Route::kTextRun) res.text_chars = route == Route::kText ? (u32)std::min(6, (56 - b1 - 4) / 8) : 0u;

  // ---- apply: new ranks, finished suffixes out, what stays active raw into (v_free, slots_next, d_GRP)
  u64* recA = static_cast<u64*>(home.rec_free);
  u64* recB = static_cast<u64*>(home.rec_keys);
  u32* pairs = reinterpret_cast<u32*>(recA);
  const WindowShifts w = window_shifts(n, window_bits);
  const int mode = route == Route::kDense ? 2 : route == Route::kPairs ? 1 : raw_list ? 3 : 0;
  if (route == Route::kFinish) blk.fin_active = true;
  // dense: records partitioned by the top 16 bits of s (bits 32.. of the record), two stable passes: apply leaves the first one's digits
  if (route == Route::kDense) { re.rec_plane = digit_planes ? d_P0 : nullptr; re.rec_shift = w.lo; }
  u32* sa_out = (emit && !blk.fin_active) ? nullptr : d_SA;   // finisher route: the bridge will want the finished suffixes' slots
  u32* rank_arg = (text && !blk.ranks_live) ? nullptr : d_rank;   // text rounds before rank[] is completed: neither complete nor needed; after: kept exact
  launch_rerank<K, INIT>(*this, kRrApply, RrForm{split, lng, mode, rr_emit_form(emit, split, lng, INIT, carried)}, ks, home.vals, (const u32*)home.slots,
                         m, n, rq.short_len, kmask, lgv,
                         RrOut{rank_arg, sa_out, mode == 2 ? nullptr : home.v_free, home.slots_next, d_GRP, (mode == 1 || mode == 2) ? pairs : nullptr,
                               mode == 1 ? pairs + cap : mode == 2 ? home.v_free : nullptr}, re);
  if (route == Route::kPairs) scatter_rank_pairs(pairs, reinterpret_cast<u32*>(recB), m, n);
  if (raw_list || m_next == 0) return 0;

  // ---- the next list: its keys by the route, then the sort
  const u8* achr = carry_next ? (const u8*)re.achr_out : (const u8*)nullptr;
  if (copy_now) {
    // rank[] is current and the list lies raw in (v_free, d_GRP): K[] for it, and the gate for the rounds to come
    BlockSort::Copies& cp = blk.copies;
    u32 longest = 0;
    const int rcc = copy_lengths(home.v_free, d_GRP, m_next, groups, n, &longest);
    if (rcc) return rcc;
    ++cp.passes;
    cp.longest = std::max(cp.longest, longest);
    if ((u64)longest < rq.h_next) cp.open = false;
    if (longest) {
      rkeys = RunKeys{d_runK, 0u, 3, 0u, false};
      if (!cp.rounds++) cp.first_depth = depth32(rq.h_next);
      stats.route |= 1024u;
    }
  }
  const u32 run_bytes = rkeys.mode ? 4u + (run_now ? 1u : 0u) : 0u;      // k[], and the byte behind the run
  switch (route) {
    case Route::kDense: {
      u64* ws = nullptr; u32* wv = nullptr;
      sort_pairs<u64>(recA, recB, home.v_free, home.vals, m, 32 + w.bits, &ws, &wv, false, 32 + w.lo, 0, true);
      home.sorted_into(ws, wv);                           // the records in window order: what is sorted next, their partners free
      launch_scatter_dense(*this, (const u64*)ws, m, w.bin_shift);
      launch_gather_dense(*this, ws, wv, m, n, depth32(rq.h_next), b2k, carry_next ? 1 : 0, w.bin_shift, rkeys);
      const u64 bytes = sort_bytes(m, 2, 12, 8, digit_planes)                     // window partition of the records
                        + (u64)m * (12 + 4) + (u64)m * (12 + 4 + 1 + 12)          // k_scatter_dense, k_gather_dense
                        + (u64)m_next * run_bytes;
      return next_list(L, ws, static_cast<u64*>(home.rec_free), wv, home.v_free, m_next, kbits, m - m_next, true, bytes, true);
    }
    case Route::kTextRun:
      // the members without a long run keep their groups (key 0)
      launch_gather_key2(*this, (const u32*)home.v_free, (const u32*)d_GRP, (const u32*)nullptr, achr, recA, m_next, n, depth32(rq.h_next), b2k, rkeys);
      return next_list(L, recA, recB, home.v_free, home.vals, m_next, kbits, 0u, false, (u64)m_next * (4 + 4 + 4 + 1 + 1 + 8), false);
    case Route::kText:
      launch_gather_text(*this, (const u32*)home.v_free, (const u32*)d_GRP, emit ? (const u8*)re.achr_out : (const u8*)nullptr, recA, m_next, n,
                         (u32)rq.h_next, res.text_chars, rkeys);
      stats.route |= 4u;
      return next_list(L, recA, recB, home.v_free, home.vals, m_next, b1 + 8 * (int)res.text_chars + 4, 0u, false,
                       (u64)m_next * (4 + 4 + 1 + 16 + 8 + (rkeys.mode ? 4 : 0)), false);
    default:
      launch_gather_key2(*this, (const u32*)home.v_free, (const u32*)d_GRP, (const u32*)d_rank, achr, recA, m_next, n, depth32(rq.h_next), b2k, rkeys);
      return next_list(L, recA, recB, home.v_free, home.vals, m_next, kbits, 0u, false, (u64)m_next * (4 + 4 + 4 + 1 + 8 + run_bytes), true);
  }
}

// Decides whether the initial key is made of dense gram codes (K2g) and, if so, leaves the code
// table in d_rank (free until the first ranking step; the byte map lives in d_SA).  G = 0: keep
// the base-sigma key.  The gram length is the longest whose universe fits kGramMaxU; the key takes
// as few grams as cover the base-sigma key's characters, and is used when that saves a radix pass.
static constexpr int kSmallGram = 526;
static constexpr int kSmallFin = 528;     // finisher: counts and smallest depths of the hard and shallow lists (FinWord)
static constexpr int kSmallFinNext = 540; // finisher: entries of the next list's kFinRegions regions, then the groups it holds
int BwtEngine::plan_grams(const KeyPlan& plan, u32 n, const u8* d_lut, GramPlan* gp) {
  hipStream_t st = stream;
  gp->G = 0;
  if (!gram_keys || n < gram_min_n) return 0;
  int g = 1;
  u64 U = plan.sigma;
  while (U * plan.sigma <= kGramMaxU && U * plan.sigma <= (u64)cap / 2 && g < 32) { U *= plan.sigma; ++g; }
  if (g < 2) return 0;
  const u32 nwords = ceil_div((u32)U, 64u);                // <= 65536
  u8* present = reinterpret_cast<u8*>(d_SA);               // byte map, then (behind it) the bitmap
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(present + 64ull * nwords);
  uint4* table = reinterpret_cast<uint4*>(d_rank);
  u32 top = 1;
  for (int t = 1; t < g; ++t) top *= plan.sigma;
  stats.alg_bytes += (u64)n + 64ull * nwords * 2;        // k_gram_mark reads T; the byte map is cleared and packed
  BWTC_HIP_TRY(hipMemsetAsync(present, 0, 64ull * nwords, st));
  hipLaunchKernelGGL(k_gram_mark, dim3(std::min<u32>(ceil_div(n, kGramTile), 4096u)), dim3(256), 0, st,
                     (const u8*)d_T, d_lut, n, g, plan.sigma, top, present);
  hipLaunchKernelGGL(k_gram_pack, dim3(ceil_div(nwords, 256u)), dim3(256), 0, st, (const u8*)present, nwords, bits);
  hipLaunchKernelGGL(k_gram_table, dim3(1), dim3(1024), 0, st, (const unsigned long long*)bits, nwords, table,
                     d_small + kSmallGram);
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallGram, d_small + kSmallGram, 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(wait());
  const u32 distinct = h_small[kSmallGram];
  if (distinct == 0) return -3;
  const int b = std::max(1, bit_width_u64(distinct - 1));
  const int g_max = std::min(64 / b, 64 / g);                 // key bits, and the text's zero padding
  if (g_max < 1) return 0;
  int G = std::min(g_max, (plan.k + g - 1) / g);
  if (gram_count_override > 0) G = std::min(g_max, gram_count_override);
  const int passes = radix_passes(b * G);
  const int base_passes = radix_passes(plan.bits);
  // fewer passes for at least as many characters, or the same passes for more
  const bool better = (g * G >= plan.k && passes < base_passes) || (g * G > plan.k && passes <= base_passes);
  if (debug_on())
    std::fprintf(stderr, "grams: sigma=%u g=%d universe=%llu present=%u bits=%d G=%d (%d chars, %d passes) vs base %d chars, %d passes -> %s\n",
                 plan.sigma, g, (unsigned long long)U, distinct, b, G, g * G, passes, plan.k, base_passes,
                 better || gram_count_override > 0 ? "grams" : "base");
  if (!better && gram_count_override <= 0) return 0;
  gp->g = g; gp->G = G; gp->b = b; gp->top = top;
  return 0;
}

// (the debug line of a block that looked for a period and takes no period step: decide_step and the rounds)
static void say_no_period_step(const BwtEngine& e, u64 h_first) {
  if (debug_on())
    std::fprintf(stderr, "periods: period %u with %u votes, longest stretch %u, the rounds begin at depth %llu: no period step\n",
                 e.blk.weighed.p, e.blk.weighed.votes, e.blk.weighed.longest, (unsigned long long)h_first);
}

// The code-key stage as suffix_sort launches it (and, kernel by kernel, BwtEngine::test_code_stage).  The key word's
// layout: the key's upper code_bits - 32 bits, 13 upper bits of the suffix number (split items), the predecessor's
// code, the level.  parts: 1 the sampled pair counts, 2 the code table, 4 the keys.
static CodeKey code_key_layout(const u32* codes, int code_bits, int split_now) {
  const int key_bits = code_bits - 32, hi_bits = split_now ? 13 : 0;
  CodeKey ck;
  ck.codes = codes; ck.kbits = code_bits; ck.hi_shift = key_bits; ck.chr_shift = key_bits + hi_bits; ck.lvl_shift = ck.chr_shift + 8;
  return ck;
}
static u32 code_sample_tiles(u32 n) { return std::min<u32>(ceil_div(n, kPairTile), 512u); }
static int launch_code_stage(BwtEngine& e, u32 parts, u32 n, const u8* d_lut, u32 sigma, u64* ka, u8* key_plane, int split_now,
                             const CodeKey& ck) {
  hipStream_t st = e.stream;
  if (parts & 1u) {
    BWTC_HIP_TRY(hipMemsetAsync(e.d_pairs, 0, (size_t)kPairReplicas * 65536 * 4, st));
    hipLaunchKernelGGL(k_pair_counts, dim3(code_sample_tiles(n)), dim3(256), 0, st, (const u8*)e.d_T, d_lut, n, e.d_pairs);
  }
  if (parts & 2u)
    hipLaunchKernelGGL(k_code_build, dim3(kCodeRows), dim3(256), 0, st, (const u32*)e.d_pairs, sigma, e.d_codes, e.d_small + kSmallError);
  if (parts & 4u)
    hipLaunchKernelGGL(k_make_keys_code, dim3(ceil_div(n, 1024)), dim3(256), 0, st, (const u8*)e.d_T, d_lut, ka, e.d_W0, n, key_plane, split_now, ck);
  return 0;
}

int BwtEngine::test_code_stage(u32 parts, u32 n, const u32* hist, bool lone_sentinel, int kbits, bool split, u8* lut, u32* sigma) {
  if (parts & 1u) {
    const KeyPlan plan = plan_keys(hist, n, lone_sentinel, true);
    std::memcpy(lut, plan.lut, 256);
    *sigma = plan.sigma;
  }
  std::memcpy(h_small + kSmallLut, lut, 256);
  BWTC_HIP_TRY(hipMemcpyAsync(d_small + kSmallLut, h_small + kSmallLut, 256, hipMemcpyHostToDevice, stream));
  const int split_now = split ? 1 : 0;
  const CodeKey ck = code_key_layout(d_codes, kbits, split_now);
  return launch_code_stage(*this, parts, n, reinterpret_cast<const u8*>(d_small + kSmallLut), *sigma, static_cast<u64*>(d_R1), d_P0,
                           split_now, ck);
}

// What the stages of the initial sort share: the block, its key plan and where the key makers write.
struct InitialSort {
  u32 n; const u32* hist; bool lone_sentinel; const KeyPlan& plan; const u8* d_lut;
  u8* key_plane;       // the key makers leave the first pass's digits
  bool implied_idx;    // slot j holds suffix n-1-j: the sort's first pass can make that up instead of reading it
  u32* idx_out;
};
static const LongKey kNoLongKey{nullptr, 0, -1, 0, 48, 0, 0};   // one key word: no second one, the suffix number's upper bits from bit 48
static constexpr int kCodeTableFull = -1000;   // initial_long -> suffix_sort, and no further: the block is sorted again, with gram keys

// the sorted keys and values reach the ranking step: the arrays the sort ended in (between the regions ka / kb and
// d_V0 / d_V1), their partners as free space; the list has no slots of its own, the next one's go to d_G0
static void hand_over(const BwtEngine& e, SortList& L, void* ka, void* kb, const void* ks, u32* vs) {
  L.home = BwtEngine::ListHome::sorted(ka, kb, e.d_V0, e.d_V1, e.d_G1, e.d_G0, ks, vs);
}

// the passes of an initial sort over keys of key_bits bits, and what they and the key maker move
static void count_initial_sort(BwtEngine& e, u32 n, int key_bits, bool wide) {
  const int passes = radix_passes(key_bits);
  e.stats.sort_pass_items += (u64)n * (u64)passes;
  // items of (u64, u32 or u16 + upper bits in the key) / (u32, u32)
  if (key_bits) e.stats.alg_bytes += (u64)n * (1 + (u64)(wide ? 8 : 4) + 1) + sort_bytes(n, passes, wide ? 12 : 8, wide ? 8 : 4, e.digit_planes);
}

// k characters as a base-sigma number
template <typename K>
static void launch_make_keys(BwtEngine& e, const InitialSort& in, K* ka, int split) {
  K top = 1;
  for (int t = 1; t < in.plan.k; ++t) top *= in.plan.sigma;
  hipLaunchKernelGGL(k_make_keys<K>, dim3(ceil_div(in.n, 1024)), dim3(256), 0, e.stream, e.d_T, in.d_lut, ka,
                     in.idx_out, in.n, in.plan.k, in.plan.sigma, top, in.key_plane, split);
}

// dense gram codes; lk.w: with a second word (the long keys, whose values the sort's first pass makes up: no idx_out)
static void launch_gram_keys(BwtEngine& e, const InitialSort& in, const BwtEngine::GramPlan& gp, u64* ka, int split, const LongKey& lk) {
  hipLaunchKernelGGL(k_make_keys_gram, dim3(ceil_div(in.n, 1024)), dim3(256), 0, e.stream, e.d_T, in.d_lut, (const uint4*)e.d_rank, ka,
                     lk.w ? (u32*)nullptr : in.idx_out, in.n, gp.g, gp.G, gp.b, in.plan.sigma, gp.top, in.key_plane, split, lk);
}

// the long-key sort in one of its shapes: whole suffix numbers, or their 16-bit lower halves in tiles of E items per thread
template <typename V, int E>
static u32* sort_long_as(BwtEngine& e, u64* ka, u64* kb, u32 n, int key_bits, int w_bits, u64** ks, u32** ws) {
  V* vs = nullptr;
  radix_sort_long<V, E>(ka, kb, reinterpret_cast<V*>(e.d_V0), reinterpret_cast<V*>(e.d_V1), e.d_W0, e.d_W1, n, key_bits, w_bits, e.d_table,
                        e.d_partial, e.stream, ks, &vs, ws, &e.probe, e.d_P0, e.d_P1, 0, false, e.long_direct);
  return reinterpret_cast<u32*>(vs);
}

// dense code -> byte, for the rankers that emit from the long keys' character codes (RrEmit::inv_lut)
static hipError_t upload_inverse_lut(BwtEngine& e, const InitialSort& in) {
  u8* inv = reinterpret_cast<u8*>(e.h_small + kSmallInv);
  std::memset(inv, 0, 256);
  for (int c = 255; c >= 0; --c) if (in.hist[c] && !(c == 0 && in.lone_sentinel)) inv[in.plan.lut[c]] = (u8)c;
  return hipMemcpyAsync(e.d_small + kSmallInv, inv, 256, hipMemcpyHostToDevice, e.stream);
}

// The 32-bit keys.  Suffixes of length <= k are finished by the initial ranking (a suffix of length exactly
// k is a proper prefix of every other suffix with the same key): short_len, here and in the 64-bit plans.
int BwtEngine::initial_keys32(const InitialSort& in, SortList& L, u64 h) {
  u32* ka = static_cast<u32*>(d_R1); u32* kb = ka + cap;
  launch_make_keys<u32>(*this, in, ka, 0);
  u32* ks = nullptr; u32* vs = nullptr;
  sort_pairs<u32>(ka, kb, d_V0, d_V1, in.n, in.plan.bits, &ks, &vs, true, 0, 0, in.key_plane != nullptr, in.implied_idx);
  BWTC_HIP_TRY(hipEventRecord(ev_sort[n_sort_events++], stream));
  hand_over(*this, L, d_R1, d_R2, ks, vs);              // both 32-bit key arrays live in R1
  RankRequest rq;
  rq.m = in.n; rq.h_next = h; rq.short_len = (u32)in.plan.k;
  const int rc = rank_step<u32, true>(L, rq);
  if (rc) return rc;
  count_initial_sort(*this, in.n, in.plan.bits, false);
  return 0;
}

// The 64-bit plans: long keys where the block can take them (initial_long), else one key word (initial_keys64).
int BwtEngine::initial_wide(const InitialSort& in, bool allow_code_keys, SortList& L, u64* h) {
  const u32 n = in.n;
  const bool long_ok = long_keys && in.implied_idx && L.emit && in.key_plane && n >= gram_min_n;
  const bool coded = long_ok && code_keys && finisher && allow_code_keys;   // (the code keys take no gram plan)
  GramPlan gp;
  if (!coded) { const int rc = plan_grams(in.plan, n, in.d_lut, &gp); if (rc) return rc; }
  int key_bits = in.plan.bits;
  u32 short_len = (u32)in.plan.k;
  if (gp.G > 0) { key_bits = gp.b * gp.G; short_len = (u32)(gp.g * gp.G); *h = (u64)short_len; }
  // Keys of at most 48 bits leave room for the upper bits of the suffix number: the passes of
  // the initial sort then carry (u64 key, u16 low half) = 10 bytes per item instead of 12.
  const int split = (split_index && in.implied_idx && key_bits <= 48 && n <= (1u << 29)) ? 1 : 0;
  if (coded || (long_ok && gp.G > 0)) {
    bool ranked = false;
    const int rc = initial_long(in, gp, key_bits, split, coded, L, h, &ranked);
    if (rc || ranked) return rc;
  }
  return initial_keys64(in, gp, key_bits, short_len, split, L, *h);
}

// One key word: dense gram codes (gp.G > 0) or k characters as a base-sigma number.
int BwtEngine::initial_keys64(const InitialSort& in, const GramPlan& gp, int key_bits, u32 short_len, int split, SortList& L, u64 h) {
  const u32 n = in.n;
  u64* ka = static_cast<u64*>(d_R1); u64* kb = static_cast<u64*>(d_R2);
  if (gp.G > 0) launch_gram_keys(*this, in, gp, ka, split, kNoLongKey);
  else launch_make_keys<u64>(*this, in, ka, split);
  u64* ks = nullptr; u32* vs = nullptr;
  if (split) {
    unsigned short* vs16 = nullptr;
    radix_sort_pairs<u64, unsigned short>(ka, kb, reinterpret_cast<unsigned short*>(d_V0), reinterpret_cast<unsigned short*>(d_V1),
                                          n, key_bits, d_table, d_partial, stream, &ks, &vs16, &probe, 0, false, false, 0,
                                          digit_planes ? d_P0 : nullptr, digit_planes ? d_P1 : nullptr, in.key_plane != nullptr, true);
    vs = reinterpret_cast<u32*>(vs16);
  } else {
    sort_pairs<u64>(ka, kb, d_V0, d_V1, n, key_bits, &ks, &vs, true, 0, 0, in.key_plane != nullptr, in.implied_idx);
  }
  BWTC_HIP_TRY(hipEventRecord(ev_sort[n_sort_events++], stream));
  hand_over(*this, L, ka, kb, ks, vs);
  RankRequest rq;
  rq.m = n; rq.h_next = h; rq.short_len = short_len; rq.split = (u32)split;
  rq.kmask = split ? (1ull << 48) - 1ull : ~0ull;       // (split: the suffix numbers' upper bits lie above)
  const int rc = rank_step<u64, true>(L, rq);
  if (rc) return rc;
  count_initial_sort(*this, n, key_bits, true);
  return 0;
}

// Long keys: the sort also orders by a second key word and the items carry their predecessor character's code, so
// that the ranking behind the ONE long sort can emit the transform's bytes and the finisher takes what is tied.
// Two makers: the order-1 prefix code (k_make_keys_code, the default) and dense gram codes (round 4, BWTC_HIP_KEYS=grams).
// *ranked stays false where the gram codes leave no room for a second word: nothing was launched, the block takes one
// key word.  kCodeTableFull: see below.
int BwtEngine::initial_long(const InitialSort& in, const GramPlan& gp, int key_bits, int split, bool coded, SortList& L, u64* h, bool* ranked) {
  hipStream_t st = stream;
  const u32 n = in.n;
  u64* ka = static_cast<u64*>(d_R1); u64* kb = static_cast<u64*>(d_R2);
  // (without the split -- blocks above 512 MiB, gram keys above 48 bits -- the items carry whole 32-bit suffix numbers:
  // 16 bytes instead of 14, and the key only needs room for the character)
  int w_bits = 0, split_now = split;
  u32 short_len = 0;
  RrLong lg{nullptr, ~0u, 0, 0, 0, -1, 0};
  if (coded) {
    // the block's order-1 statistics from a sample of its character pairs, the alphabetic codes, the keys
    split_now = (split_index && n <= (1u << 29)) ? 1 : 0;
    key_bits = code_bits - 32;                        // the key word's share; the second word takes 32
    w_bits = 32;
    const CodeKey ck = code_key_layout(d_codes, code_bits, split_now);
    BWTC_HIP_TRY(upload_inverse_lut(*this, in));
    const u32 sample_tiles = code_sample_tiles(n);
    const int rc = launch_code_stage(*this, 7u, n, in.d_lut, in.plan.sigma, ka, in.key_plane, split_now, ck);
    if (rc) return rc;
    lg.hi_shift = ck.hi_shift; lg.chr_shift = ck.chr_shift; lg.chr_mask = 0xFFu; lg.lvl_shift = ck.lvl_shift;
    short_len = 0;                                    // every item has its own (rr_masks)
    *h = 1;
    stats.alg_bytes += (u64)sample_tiles * kPairTile + (u64)kPairReplicas * 65536 * 8;
    if (debug_on())
      std::fprintf(stderr, "code keys: %d + %d bits, sigma %u, %u sampled tiles, character code at bit %d, level at bit %d\n",
                   key_bits, w_bits, in.plan.sigma, sample_tiles, ck.chr_shift, ck.lvl_shift);
  } else {
    const int cb = std::max(1, bit_width_u64(in.plan.sigma - 1));
    int G2 = std::min(32 / gp.b, (64 - gp.g * gp.G) / gp.g);
    G2 = std::min(G2, long_grams_override > 0 ? long_grams_override : 2);
    const int hi_bits = split ? 13 : 0;
    if (G2 < 1 || key_bits + hi_bits + cb > 64) return 0;
    LongKey lk = kNoLongKey;
    lk.w = d_W0; lk.G2 = G2; lk.hi_shift = key_bits; lk.chr_shift = key_bits + hi_bits; lk.chr_mask = (1u << cb) - 1u;
    BWTC_HIP_TRY(upload_inverse_lut(*this, in));
    w_bits = gp.b * lk.G2;
    if (w_bits < kRadixBits) { lk.first_r = w_bits; lk.first_mask = (1u << std::min(kRadixBits, w_bits + key_bits)) - 1u; }
    short_len = (u32)(gp.g * (gp.G + lk.G2));
    *h = (u64)short_len;
    launch_gram_keys(*this, in, gp, ka, split, lk);
    lg.hi_shift = lk.hi_shift; lg.chr_shift = lk.chr_shift; lg.chr_mask = lk.chr_mask; lg.lvl_shift = -1; lg.depth = short_len;
    if (debug_on())
      std::fprintf(stderr, "long keys: %d + %d bits, %d + %d grams of %d characters, character code at bit %d\n",
                   key_bits, w_bits, gp.G, lk.G2, gp.g, lk.chr_shift);
  }
  u64* ks = nullptr; u32* ws = nullptr;
  u32* vs = !split_now ? sort_long_as<u32, 6>(*this, ka, kb, n, key_bits, w_bits, &ks, &ws)
            : long_items_per_thread == 6 ? sort_long_as<unsigned short, 6>(*this, ka, kb, n, key_bits, w_bits, &ks, &ws)
                                         : sort_long_as<unsigned short, 8>(*this, ka, kb, n, key_bits, w_bits, &ks, &ws);
  BWTC_HIP_TRY(hipEventRecord(ev_sort[n_sort_events++], st));
  hand_over(*this, L, ka, kb, ks, vs);
  lg.w = ws; lg.wmask = w_bits >= 32 ? ~0u : (1u << w_bits) - 1u;
  RankRequest rq;
  rq.m = n; rq.h_next = *h; rq.short_len = short_len; rq.kmask = (1ull << key_bits) - 1ull; rq.split = (u32)split_now; rq.lg = &lg;
  const int rc = rank_step<u64, true>(L, rq);
  if (rc == -3 && coded && (h_small[kSmallError] & 2u)) {
    // a codeword came out longer than the table's fields hold (k_code_build): nothing has been emitted yet --
    // this block again, with gram keys (suffix_sort, allow_code_keys == false)
    if (debug_on()) std::fprintf(stderr, "code keys: a codeword above %u bits, the block takes gram keys\n", kCodeMaxLen);
    BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallError, 0, 4, st));
    return kCodeTableFull;
  }
  if (rc) return rc;
  const int long_passes = radix_passes(key_bits + w_bits);
  stats.sort_pass_items += (u64)n * (u64)long_passes;
  stats.alg_bytes += (u64)n * (1 + 12 + 1)               // the key maker: T read, key + second word + first plane written (the values are made up by the first pass)
                     + sort_bytes(n, long_passes, split_now ? 14 : 16, 8, true);
  stats.route |= coded ? 17u : 1u;
  *ranked = true;
  return 0;
}

// Is a step of the block's this round's?  The first entry still to come is, where decide_step made it the first round's
// (BWTC_HIP_MULTI: several such entries take consecutive rounds at one depth, each storing its merged words when it is due).
// Behind them the first entry that waits is due in the round whose depth h_round has reached its p, with rank[] complete,
// no live local list and no text round pending -- as long as the stretches are longer than that: the step's gate, by
// the longest stretch, or, behind a run step (BWTC_HIP_MIXED), by the longest proper stretch.  There d_runK still holds
// k_1[]: the storing pass puts k_p[] in its place first (store_step).  An entry whose gate is shut is dropped and the
// next one that waits is looked at.  The entry that is due becomes the current one.
int BwtEngine::step_due(const SortList& L, u32 m, u64 h_round, u64 h_first, bool text_round, bool* due) {
  *due = false;
  int i = 0;
  while (i < blk.n_steps && blk.steps[i].when == StretchStep::kNone) ++i;   // the first entry that is still to come
  if (i == blk.n_steps) return 0;
  if (blk.steps[i].when == StretchStep::kThisRound) {
    // (BWTC_HIP_MULTI: several of the first round's take consecutive rounds at its depth; each stores when it is due)
    blk.steps[i].when = StretchStep::kNone;
    if (m == 0) return 0;
    if (blk.merged) { const int rc = store_step(L.n, blk.steps[i], h_round, false); if (rc) return rc; }
    blk.current = i;
    *due = true;
    return 0;
  }
  if (m == 0) return 0;
  for (; i < blk.n_steps; ++i) {
    StretchStep& step = blk.steps[i];
    if (step.when != StretchStep::kWaiting) continue;
    const bool behind_run = i > 0;
    if ((u64)blk.due_gate(i) <= std::max<u64>(h_round, step.p)) {
      step.when = StretchStep::kNone;
      step.dropped = true;
      say_no_period_step(*this, h_first);
      continue;                                          // (the next entry that waits may be this round's)
    }
    if (h_round >= (u64)step.p && L.ranks_complete && blk.fin.local_m == 0 && !text_round) {
      step.when = StretchStep::kNone;
      const int rc = store_step(L.n, step, h_round, behind_run);
      if (rc) return rc;
      blk.current = i;
      *due = true;
    }
    return 0;
  }
  return 0;
}

// The storing pass of the step that is due at depth h_round.  One period's lengths: k_p[] over whatever d_runK held (a
// run's member with k_1 >= p has k_p = k_1, one with k_1 < p <= h_round would look up at h_round anyway: nothing is lost
// with k_1[]).  Merged words (BWTC_HIP_MULTI): the merging pass, which needs the step's depth
// and the earlier steps' words -- the block's first one writes them fresh.
int BwtEngine::store_step(u32 n, StretchStep& step, u64 h_round, bool behind_run) {
  if (blk.merged) {
    const StepMerge merge{depth32(h_round), !blk.merged_stored};
    u32 longest = 0, proper = 0;
    const int rc = stretch_lengths(n, step.p, true, &longest, &proper, &merge);
    if (rc) return rc;
    blk.merged_stored = true;
    return 0;
  }
  if (blk.lengths_period == step.p) return 0;            // (a waiting step at the front: its lengths were stored when it was decided)
  return stretch_lengths(n, step.p, true, &step.longest, behind_run ? &step.proper : nullptr);
}

// The rounds over the sorted list in L.home, from depth ask.h0 until nothing is tied.  ask.text_rounds: rounds that compare
// the text itself first (finisher route: rank[] is not complete, and completing it costs an ISA scatter of the whole block).
// ask.doubling == false: text rounds only; what they leave tied comes back raw in (home.v_free, home.slots_next, d_GRP) --
// suffix, slot, head slot -- out->left entries at depth out->h_left.
int BwtEngine::run_rounds(SortList& L, const RoundsRequest& ask, RoundsLeft* out) {
  const u32 n = L.n;
  ListHome& home = L.home;
  RankResult& res = L.res;
  RrEmit& re = L.re;
  u32 m = ask.m;
  u64 h = ask.h0;
  bool keep_h = ask.keep_first;             // the list is sorted to depth h as it stands (no doubling before the next step)
  int text_left = ask.text_rounds;
  // the block's closed-form steps (runs, periods), decided where a list is about to double: an entry's `when` says whether
  // it is the first round's or waits for a deeper one
  const u64 h_first = ask.keep_first ? ask.h0 : ask.h0 * 2;
  if (ask.doubling && m > 0) {
    const int rcs = decide_step(n, m, h_first, static_cast<const u64*>(home.keys), home.vals, carried_mask(res.carry));
    if (rcs) return rcs;
  }
  int text_extra = text_rounds_fixed ? 0 : 12;        // further ones, one at a time, while the list is short (not when BWTC_HIP_TEXT_ROUNDS says how many)
  while (m > 0 || (ask.doubling && blk.fin.local_m > 0)) {
    if (h >= (u64)n * 2 + 64) return -3;   // cannot happen: every group splits by then
    ++stats.rounds;
    stats.active_sum += m;
    const bool text_round = text_left > 0 && m > 0;
    bool run_req = false;
    const int rcd = step_due(L, m, keep_h ? h : h * 2, h_first, text_round, &run_req);
    if (rcd) return rcd;
    StretchStep& step = blk.current_step();
    const bool period_req = run_req && step.p >= 2;
    const bool text = text_round || (run_req && !L.ranks_complete);   // the run step reads no rank[]: it does not need the completion either
    const bool raw = !text && !ask.doubling;           // out of text rounds and not allowed to double: hand the list back
    if (debug_on()) std::fprintf(stderr, "round %u%s: h=%llu m=%u groups=%u\n", stats.rounds, text ? " (text)" : "", (unsigned long long)h, m, res.groups);
    if (!keep_h) h *= 2;
    keep_h = false;
    if (!text && !raw && !L.ranks_complete) {
      // the doubling rounds start here: rank[] for everybody first (the finished from SA; the list's own
      // ranks come from the ranking step below, before anything reads them; a parked list's are its groups' heads)
      complete_ranks(n, home.vals, home.slots, m, home.spare_region(d_R2, d_R1, d_W0), home.rec_free);
      L.ranks_complete = true;
      blk.ranks_live = true;
      stats.route |= 8u;
      stats.alg_bytes += (u64)n * (4 + 8);                // k_bridge_pairs_all (the partition and scatter count themselves)
    }
    // what the local list's last pass noted reaches rank[] now: before this round's look-ups, after the last round's
    if (!text && !raw) { const int rcu = local_updates(); if (rcu) return rcu; }
    if (m == 0) { const int rcl = local_pass(n, 0, re); if (rcl) return rcl; continue; }   // only the local list is left
    // the list just sorted lies in L.home (positions are the active list's, home.slots gives their global slots); the
    // characters of what stays active go to the plane the list's own do not lie in
    std::swap(re.achr_out, L.achr_other);
    RankRequest rq;
    rq.m = m; rq.h_next = h; rq.kind = raw ? RoundKind::kRaw : text ? RoundKind::kText : RoundKind::kOrdinary;
    rq.run_mode = run_req ? 1 : (blk.merged ? blk.merged_ran : step.depth != 0) ? 2 : 0;   // the second keys (RunKeys::mode): the run step, a round behind one, or no runs in play
    // a copy round ("Copies"): an ordinary doubling round over a complete rank[], no local list beside it, nothing parked,
    // no step that ran or waits (d_runK is nobody's), the gate open
    rq.copies = copy_rounds && ask.doubling && !text && !raw && L.ranks_complete && blk.fin.local_m == 0 && blk.fin.parked == 0 &&
                rq.run_mode == 0 && !blk.step_in_play() && blk.copies.open;
    const int rc2 = rank_step<u64, false>(L, rq);
    if (rc2) return rc2;
    m = res.m;
    const bool ran = run_req && res.ran_run;
    if (period_req && !ran) say_no_period_step(*this, h_first);   // (the key had no room for the step's bit: an ordinary round)
    if (run_req && !ran && blk.merged) {
      // ... and the merged words name members that no closed-form key has ranked: nobody reads them again, no step follows
      blk.merged_ran = false;
      for (int i = 0; i < blk.n_steps; ++i)
        if (blk.steps[i].when != StretchStep::kNone) { blk.steps[i].when = StretchStep::kNone; blk.steps[i].dropped = true; }
    }
    if (ran) {
      // the list is sorted to depth h still: a run's members by their closed-form keys, the others as they were (or by rank[s + h])
      step.depth = depth32(h);
      stats.route |= period_req ? 256u : 32u;
      if (step.ranks_runs) stats.route |= 32u;           // (BWTC_HIP_MIXED: one step over k_p[] ranked the runs too)
      if (blk.merged) blk.merged_ran = true;
      if (blk.period_steps_ran() > 1) stats.route |= 512u;   // (BWTC_HIP_MULTI: more than one period step in the block)
      if (period_req && step.p > kPeriodMax) stats.route |= 2048u;   // (BWTC_HIP_LONG_PERIODS: a period step with p > kPeriodMax)
      keep_h = true;
      if (period_req && debug_on())
        std::fprintf(stderr, "periods: period %u with %u votes, longest stretch %u, the rounds begin at depth %llu: period step at depth %u\n",
                     step.p, step.votes, blk.said_longest(step), (unsigned long long)h_first, step.depth);
      // rank[] still incomplete: one text round behind the runs first -- a block that is one giant run ends there,
      // without the completion of rank[] that the first doubling round costs.  Not beside a live local list: its
      // members' ranks are local_depth deep, and the first doubling look-up must not lie deeper than that (text rounds
      // raise h; that is why a list with a local list beside it takes none)
      if (!L.ranks_complete && text_left == 0 && !text_rounds_fixed && blk.fin.local_m == 0) text_left = 1;
    }
    if (raw) { if (out) *out = RoundsLeft{m, h}; return 0; }
    // the local list's doubling step beside the global list's (both read the rank[] this round's ranking step left)
    if (!text && ask.doubling && blk.fin.local_m > 0) { const int rcl = local_pass(n, h, re); if (rcl) return rcl; }
    if (text && !ran) {
      h += res.text_chars; keep_h = true;
      if (text_round) --text_left;
      // Out of text rounds with a short list left: a few more cost tens of microseconds each, the doubling rounds
      // cost the completion of rank[] for the whole block first (5 ms per 256 MiB, 16 ms for the 1 GiB text -- the
      // block whose text rounds ended with 10 entries still tied paid it).  Long lists (deep repeats) go on to the
      // doubling rounds as before: their depth doubles there and only creeps here.
      if (text_left == 0 && m > 0 && (u64)m * 4096 < (u64)n && text_extra > 0) { text_left = 1; --text_extra; }
    }
  }
  bool waited = false;                                   // (the rounds ended before their depth reached p)
  for (int i = 0; i < blk.n_steps; ++i)
    if (blk.steps[i].when == StretchStep::kWaiting) { blk.steps[i].when = StretchStep::kNone; blk.steps[i].dropped = true; waited = true; }
  if (waited) say_no_period_step(*this, h_first);
  if (blk.merged && ask.doubling && debug_on()) {
    std::fprintf(stderr, "steps: %d entries", blk.n_steps);
    for (int i = 0; i < blk.n_steps; ++i)
      std::fprintf(stderr, "%s (p %u, depth %u, gate %u, votes %u)", i ? "," : ":", blk.steps[i].p, blk.steps[i].depth, blk.steps[i].shown_gate(true), blk.steps[i].votes);
    std::fprintf(stderr, "\n");
  } else if (mixed_steps && ask.doubling && debug_on()) {
    const StretchStep period = blk.period_ran();
    std::fprintf(stderr, "steps: run step at depth %u, period step of period %u at depth %u, longest run %u, longest proper stretch %u\n",
                 blk.run_depth(), period.p, period.depth, blk.run_longest, blk.weighed.proper);
  }
  if (long_periods && ask.doubling && debug_on())
    std::fprintf(stderr, "steps: long periods on, route bit 11 %s (period step of period %u at depth %u)\n", (stats.route & 2048u) ? "set" : "clear",
                 blk.period_ran().p, blk.period_ran().depth);
  if (copy_rounds && ask.doubling && debug_on())
    std::fprintf(stderr, "copies: %u passes, %u copy rounds, longest K %u, first depth %u, the rounds begin at depth %llu\n", blk.copies.passes,
                 blk.copies.rounds, blk.copies.longest, blk.copies.first_depth, (unsigned long long)h_first);
  if (out) *out = RoundsLeft{0, h};
  return 0;
}

// The finisher's counter words in d_small, by their place from kSmallFin on.  The kernels take a pair of them, (entries,
// smallest depth), and index [0] and [1] from there: the hard pair and the shallow pair.
enum FinWord : int {
  kFinSpare,                       // (reset and read back with the hard pair; nothing counts in it)
  kFinHard, kFinHardDepth,         // the hard list (groups too large for a window): its entries, the smallest depth among them
  kFinWaitDepth,                   // the smallest depth of what waits for the rounds (k_fin_to_hard)
  kFinShallow, kFinShallowDepth,   // the shallow list (hard groups that share fewer than fin_floor characters): the same pair
  kFinLocalDepth,                  // the smallest depth of the local list (k_list_copy)
  kFinWords,
  kFinNext = kSmallFinNext - kSmallFin,                       // the list a launch leaves: the entries of its kFinRegions regions,
  kFinNextLast = kFinNext + kFinRegions - 1, kFinGroupsLeft   //   then the groups it holds
};
static_assert(kFinWords <= kFinNext, "the finisher's counter words end before the next list's");
static_assert(kSmallFin + kFinGroupsLeft < kSmallLut, "the next list's words end before the next words of d_small in use");
// The words on the device (word), their mirror in h_small ([]), and the transfers of words first .. last between the two
// on the engine's stream (to: a test hook's array in place of the mirror).
struct FinCounters {
  u32* d; u32* h; hipStream_t st;
  explicit FinCounters(const BwtEngine& e) : d(e.d_small + kSmallFin), h(e.h_small + kSmallFin), st(e.stream) {}
  u32& operator[](int w) const { return h[w]; }
  u32* word(int w) const { return d + w; }
  FinShallow shallow_sink(u32* S, u64* HP, u32 floor) const { return FinShallow{S, HP, d + kFinShallow, floor}; }
  hipError_t upload(int first, int last) const { return hipMemcpyAsync(d + first, h + first, (last - first + 1) * 4, hipMemcpyHostToDevice, st); }
  hipError_t fetch(int first, int last, u32* to = nullptr) const { return hipMemcpyAsync(to ? to : h + first, d + first, (last - first + 1) * 4, hipMemcpyDeviceToHost, st); }
  hipError_t clear(int first, int last) const { return hipMemsetAsync(d + first, 0, (last - first + 1) * 4, st); }
};
// The finisher's list between its passes: where it lies (a) and where a pass puts what it leaves (b), its entries and
// regions (finisher_passes begins with the m entries as one region).  And what the passes are asked: the block's size and
// emitter, the shallow sink, whether what they leave tied may become the local list, and how many they may be.
struct FinWork { FinList a, b; u32 m; FinRegions rg; };
struct FinRequest { u32 n; RrEmit& re; FinShallow shal; bool keep_local; int max_passes; };

// The finisher's start: its counter words, and the two homes its lists alternate between.  The first list's suffixes lie
// in S (the ranking's free value array; d_V0 in the test hooks), its slots in d_G0, its characters in d_C0, where the
// initial ranking leaves them.
hipError_t BwtEngine::finisher_begin(u32* S, u32 m, FinWork* w) {
  *w = FinWork{FinList{S, d_G0, d_GRP, reinterpret_cast<unsigned short*>(d_C0)}, FinList{d_W0, d_W1, d_G1, reinterpret_cast<unsigned short*>(d_C1)}, m, FinRegions{}};
  const FinCounters fc(*this);
  fc[kFinWaitDepth] = 0xFFFFFFFFu; fc[kFinShallow] = 0; fc[kFinShallowDepth] = 0xFFFFFFFFu; fc[kFinLocalDepth] = 0xFFFFFFFFu;
  return fc.upload(kFinWaitDepth, kFinLocalDepth);
}

// The finisher route: the long-key ranking's list through the finisher's passes; the shallow list's rounds, what they
// and the passes leave waiting (parked), the local list, and the rounds that end the block.
int BwtEngine::finisher_route(SortList& L, u32 n_lf) {
  const ListHome& home = L.home;
  if (L.re.lf_n == 0 && n_lf > 1) return -3;
  blk.lf_noted = true;                     // every suffix that becomes final notes its LF power (lf_note), in every route
  L.ranks_complete = false;
  FinWork w;
  BWTC_HIP_TRY(finisher_begin(home.v_free, L.res.m, &w));
  const FinRequest rq{L.n, L.re, FinCounters(*this).shallow_sink(home.vals, static_cast<u64*>(home.rec_free), fin_floor),
                      local_rounds && !copy_rounds,   // (copy rounds: no local list -- copies of up to 256 members would never meet the rule)
                      finisher_shape(L.n, L.res)};
  FinOutcome fo;
  int rc = finisher_passes(w, rq, &fo);
  if (rc) return rc;
  u32 shallow_depth = 0xFFFFFFFFu;
  if (fo.shallow) { rc = shallow_rounds(L, fo, &shallow_depth); if (rc) return rc; }
  if (!blk.fin.parked && !blk.fin.local_m) return 0;
  return waiting_to_rounds(L, fo, shallow_depth);
}

// The passes' shape for the list the long-key ranking left (-> blk.fin.window / group), and the passes it may take.
int BwtEngine::finisher_shape(u32 n, const RankResult& res) {
  // Groups of hundreds of members on average (a period, one text many times over) are not the finisher's: its loop
  // costs a group's size per member.  The list then goes to the rounds as it is (shallow groups apart).
  const bool giant = res.groups > 0 && (u64)res.m > (u64)res.groups * 64;
  if (giant && debug_on())
    std::fprintf(stderr, "finisher: skipped, %u entries in %u groups (more than 64 members on average)\n", res.m, res.groups);
  // The shape of the passes.  The comparison loop costs a group's size per member, which is why groups above 256 members
  // are not the finisher's on a real text (most of the block is on its list).  A SHORT list -- the long keys told
  // nearly everything apart: 2.6 % of the generator's text is left -- takes windows of 2048 entries and groups of up to
  // 1024 members instead: the few large groups (tokens repeated: 19 K entries of 7 M) are settled with the others and
  // no hard list is left for the text rounds, whose five rounds of tiny launches cost more than the whole pass
  // (256 MiB: 21.9 -> 21.3 ms).  Bounded: the wide shape costs at most 0.45 ns per entry more (measured on a real
  // text, where every group is large), n / 24 entries at most.
  blk.fin.window = fin_window; blk.fin.group = fin_max_group;
  // One pass only in that shape: what three rounds of sixteen characters leave tied in a short list is deep repeats
  // (copies of a long piece), the rounds' business -- further passes over groups of hundreds of members cost their size
  // per member and settle nothing (300 copies of a 10 KB piece in the generator's text: 32.6 ms with three passes, 30.0
  // in the narrow shape, where such groups are hard at once).
  const bool wide = !fin_shape_fixed && fin_wide_short && !giant && (u64)res.m * 24 <= (u64)n;
  if (wide) { blk.fin.window = 2048; blk.fin.group = 1024; }
  return giant ? 0 : wide ? std::min(1, fin_max_passes) : fin_max_passes;
}

// The few hard groups of little depth first, on their own: text rounds only (rank[] must not go live while
// finisher passes are still to come); what they leave tied joins the waiting list, at the depth they reached.
int BwtEngine::shallow_rounds(SortList& L, const FinOutcome& fo, u32* shallow_depth) {
  const ListHome& home = L.home;
  int rc = dress_list(L, fo.shallow, home.vals, static_cast<u64*>(home.rec_free));
  if (rc) return rc;
  RoundsLeft tied;
  rc = run_rounds(L, RoundsRequest{fo.shallow, std::max<u64>(1, fo.shallow_depth), std::max(text_rounds, 3), true, false}, &tied);
  if (rc || !tied.left) return rc;
  if ((u64)blk.fin.parked + tied.left > cap) return -3;
  hipLaunchKernelGGL(k_raw_to_park, dim3(ceil_div(tied.left, 256)), dim3(256), 0, stream, (const u32*)home.v_free, (const u32*)home.slots_next,
                     (const u32*)d_GRP, tied.left, d_parkS, d_parkHP, blk.fin.parked);
  blk.fin.parked += tied.left;
  *shallow_depth = depth32(tied.h_left);
  if (debug_on()) std::fprintf(stderr, "shallow groups: %u entries still tied at depth %llu join the waiting list\n", tied.left, (unsigned long long)tied.h_left);
  return 0;
}

// The waiting list (what the passes and the shallow groups' rounds parked) goes to the rounds that end the block, at the
// smallest depth any of it has, with the local list beside it.
int BwtEngine::waiting_to_rounds(SortList& L, const FinOutcome& fo, u32 shallow_depth) {
  const FinCounters fc(*this);
  BWTC_HIP_TRY(fc.fetch(kFinWaitDepth, kFinWaitDepth));
  BWTC_HIP_TRY(wait());
  u64 h_pk = std::min<u64>(std::min<u64>(fc[kFinWaitDepth], fo.hard ? fo.hard_depth : 0xFFFFFFFFu), shallow_depth);
  if (blk.fin.local_m) h_pk = std::min<u64>(h_pk, blk.fin.local_depth);   // every rank is at least as deep as the rounds' first look-up
  const u32 total = blk.fin.parked;
  if (debug_on())
    std::fprintf(stderr, "finisher: %u entries (%u of groups too large) go on to the rounds at depth %llu; %u entries of small groups double beside them from depth %u\n",
                 total, fo.hard, (unsigned long long)h_pk, blk.fin.local_m, blk.fin.local_m ? blk.fin.local_depth : 0u);
  if (total) {
    BWTC_HIP_TRY(hipMemcpyAsync(d_V0, d_parkS, (size_t)total * 4, hipMemcpyDeviceToDevice, stream));
    BWTC_HIP_TRY(hipMemcpyAsync(d_R1, d_parkHP, (size_t)total * 8, hipMemcpyDeviceToDevice, stream));
    blk.fin.parked = 0;                    // (the list is in the rounds' hands now: complete_ranks takes it from them)
    const int rc = dress_list(L, total, d_V0, static_cast<u64*>(d_R1), blk.fin.park_holes);
    if (rc) return rc;
  } else {
    // no global list: the rounds still want free regions to complete rank[] in
    L.res.m = 0; L.res.groups = 0;
    L.home = ListHome::at(d_W0, d_R1, d_V0, d_V1, d_G0, d_G1);
  }
  const u32 listed = total ? L.res.m : 0u;               // (the waiting list without its holes)
  // text rounds -- a global sort per six characters -- are for what is left of a text; a long list is deep repeats,
  // which only doubling gets through
  const int text_now = (!blk.fin.local_m && ((u64)listed * 16 < (u64)L.n || text_rounds_fixed)) ? text_rounds : 0;
  return run_rounds(L, RoundsRequest{listed, std::max<u64>(1, h_pk), text_now, true, true});
}

// The driver: the block's state and key plan, the initial sort and ranking, then the finisher route or the rounds.
int BwtEngine::suffix_sort(u32 n, const u32* hist, bool lone_sentinel, const EmitTarget* em, bool allow_code_keys) {
  n_sort_events = 0;
  stats.rounds = 0; stats.active_sum = 0; stats.sort_pass_items = 0; stats.route = 0; stats.finisher_entries = 0;
  blk = BlockSort{};                       // (nothing of the last block's; what bwtc_hip_period_get reports lived until here)
  if (n == 0) return 0;

  const KeyPlan plan = plan_keys(hist, n, lone_sentinel, gram_min_n < kGramMinN);   // (the tests' small blocks: 64-bit keys whatever the entropy says)
  std::memcpy(h_small + kSmallLut, plan.lut, 256);
  BWTC_HIP_TRY(hipMemcpyAsync(d_small + kSmallLut, h_small + kSmallLut, 256, hipMemcpyHostToDevice, stream));
  const bool implied_idx = !use_sweep && n > 1;
  const InitialSort in{n, hist, lone_sentinel, plan, reinterpret_cast<const u8*>(d_small + kSmallLut),
                       digit_planes && !use_sweep ? d_P0 : nullptr, implied_idx, implied_idx ? nullptr : d_V0};
  RrEmit re{em ? em->out : nullptr, em ? em->out_n : 0u, d_small + kSmallLastChar, d_small + kSmallPidx, d_T, d_C0, nullptr, 0,
            reinterpret_cast<const u8*>(d_small + kSmallInv), d_small + kSmallLf, 0, 0, 0};
  if (em && em->n_lf > 1 && n / em->n_lf >= 1) {
    re.lf_n = em->n_lf; re.lf_x = n / em->n_lf; re.lf_inv = re.lf_x > 1 ? (u32)((1ull << 32) / re.lf_x) : 0u;
  }
  SortList L{n, em != nullptr, ListHome{}, re, RankResult{}, d_C1, true};   // (hand_over gives the list its home)
  u64 h = (u64)plan.k;                     // the next round compares rank[s + h]

  BWTC_HIP_TRY(hipEventRecord(ev_sort[n_sort_events++], stream));
  int rc = plan.wide ? initial_wide(in, allow_code_keys, L, &h) : initial_keys32(in, L, h);
  if (rc == kCodeTableFull) return suffix_sort(n, hist, lone_sentinel, em, false);
  if (rc) return rc;
  rc = L.res.finish ? finisher_route(L, em->n_lf) : run_rounds(L, RoundsRequest{L.res.m, h, 0, false, true});
  if (rc) return rc;
  BWTC_HIP_TRY(hipGetLastError());
  BWTC_HIP_TRY(take_sticky_error());
  return 0;
}

// BWTC_HIP_DEBUG (read at the call: tests and scripts switch it on a live context): a pass times itself between two
// events, for scripts/runs_bench.py and scripts/periods_bench.py.  The events are destroyed on every way out.
namespace {
struct PassTimer {
  const bool on = debug_on();
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  explicit PassTimer(hipStream_t s) : st(s) {}
  ~PassTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  hipError_t start() {
    if (!on) return hipSuccess;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    return e == hipSuccess ? hipEventRecord(a, st) : e;
  }
  hipError_t stop() { return on ? hipEventRecord(b, st) : hipSuccess; }
  hipError_t ms(float* out) { return hipEventElapsedTime(out, a, b); }   // (behind a wait for the stream)
};
}  // namespace

// The stretch-length pass (three launches behind whatever the stream holds, one host wait): k_p[] for every suffix of
// the block into d_runK, unless this is a trial, and the block's longest stretch of period p.  p = 1 is the run-length
// pass: the text read once per launch, and the block's longest run is known from then on.
static constexpr int kSmallStretch = 800;   // d_small: the two words a pass reads back (the longest stretch; the longest proper one)
// merge (BWTC_HIP_MULTI and its test hook; with store and proper): d_runK holds the block's merged look-up words, and the
// pass is the step's of depth merge->h -- the first of the block (fresh) or one behind others, whose words it reads.
int BwtEngine::stretch_lengths(u32 n, u32 p, bool store, u32* longest, u32* proper, const StepMerge* merge) {
  if (merge && (!store || !proper || n > kStepLength)) return -1;
  if (proper) *proper = 0;
  // (the tiles reach n + p and their positions are 32-bit: a block within two tiles of 2^32 takes no step)
  if ((u64)n + p + 2ull * kRunTile > 0xFFFFFFFFull) { *longest = 0; return 0; }
  // (... and the tiles' words have room for n + p <= 2 cap positions: a named long period at or above n is nobody's period)
  if (p > kPeriodMax && p >= n) { *longest = 0; return 0; }
  hipStream_t st = stream;
  const u32 tiles = (u32)(((u64)n + p + kRunTile - 1) / kRunTile);   // the tiles cover the positions x = s + p, s < n
  u32* k = store ? d_runK : nullptr;
  PassTimer timer(st);
  BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallStretch, 0, proper ? 8 : 4, st));
  BWTC_HIP_TRY(timer.start());
  if (p == 1 && !proper) {
    hipLaunchKernelGGL(k_stretch_tiles<true>, dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)d_T, n, p, d_runF);
    hipLaunchKernelGGL(k_run_carry, dim3(1), dim3(1024), 0, st, (const u32*)d_runF, tiles, n, d_runB);
    hipLaunchKernelGGL(k_stretch_lengths<true>, dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)d_T, n, p, (const u32*)d_runB, k, d_small + kSmallStretch, 0u, 0u);
  } else {
    hipLaunchKernelGGL(k_stretch_tiles<false>, dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)d_T, n, p, d_runF);
    hipLaunchKernelGGL(k_run_carry, dim3(1), dim3(1024), 0, st, (const u32*)d_runF, tiles, n, d_runB);
    if (merge)
      hipLaunchKernelGGL((k_stretch_lengths<false, true, true>), dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)d_T, n, p, (const u32*)d_runB, k, d_small + kSmallStretch,
                         merge->h, merge->fresh ? 1u : 0u);
    else if (proper)   // (the second maximum: BWTC_HIP_MIXED and its test hook only; p = 1 takes the general form for it)
      hipLaunchKernelGGL((k_stretch_lengths<false, true>), dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)d_T, n, p, (const u32*)d_runB, k, d_small + kSmallStretch, 0u, 0u);
    else
      hipLaunchKernelGGL(k_stretch_lengths<false>, dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)d_T, n, p, (const u32*)d_runB, k, d_small + kSmallStretch, 0u, 0u);
  }
  BWTC_HIP_TRY(timer.stop());
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallStretch, d_small + kSmallStretch, proper ? 8 : 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(wait());
  if (timer.on) {
    float ms = 0.f;
    BWTC_HIP_TRY(timer.ms(&ms));
    if (p == 1 && store) std::fprintf(stderr, "runs: the run-length pass took %.4f ms for %u suffixes\n", ms, n);
    else std::fprintf(stderr, store ? "periods: the period-length pass took %.4f ms for %u suffixes, period %u\n"
                                    : "periods: a trial pass (no lengths stored) took %.4f ms for %u suffixes, period %u\n", ms, n, p);
  }
  *longest = h_small[kSmallStretch];
  if (proper) *proper = h_small[kSmallStretch + 1];
  if (store) blk.lengths_period = p;
  if (p == 1) blk.run_longest = *longest;
  // T read twice (p > 1: both streams of it), the lengths written; the tiles' words written and read
  stats.alg_bytes += (u64)n * ((p == 1 && !proper ? 1 + 1 : 2 + 2) + (store ? 4 : 0) + (merge && !merge->fresh ? 4 : 0)) + (u64)tiles * 16;
  return 0;
}

// The copy round's three passes ("Copies") behind whatever the stream holds, and one host wait for the one word a stretch
// pass reads back: K[] for every position of the block into d_runK, and the longest K.  bad[] (a byte per group) lives in
// d_LP0 and P[] (a byte per position, read by 16-byte loads that begin below n) in d_parkS: a local list's home and the
// waiting list, both dead in a round with no local list live and nothing parked.  d_runK's lengths are no period's now.
int BwtEngine::copy_lengths(const u32* aidx, const u32* agrp, u32 m, u32 groups, u32 n, u32* longest) {
  *longest = 0;
  if (m == 0 || groups == 0 || (u64)n + 2ull * kRunTile > 0xFFFFFFFFull) return -1;
  hipStream_t st = stream;
  u8* bad = reinterpret_cast<u8*>(d_LP0);
  u8* P = reinterpret_cast<u8*>(d_parkS);
  const u32 tiles = (u32)(((u64)n + kRunTile - 1) / kRunTile), grid = ceil_div(m, kCopyTile);
  PassTimer t_marks(st), t_flags(st), t_lengths(st);
  BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallStretch, 0, 4, st));
  BWTC_HIP_TRY(t_marks.start());
  BWTC_HIP_TRY(hipMemsetAsync(bad, 0, groups, st));
  hipLaunchKernelGGL(k_copy_marks, dim3(grid), dim3(kCopyTPB), 0, st, aidx, agrp, m, (const u32*)d_rank, n, bad);
  BWTC_HIP_TRY(t_marks.stop());
  BWTC_HIP_TRY(t_flags.start());
  BWTC_HIP_TRY(hipMemsetAsync(P, 0, n, st));
  hipLaunchKernelGGL(k_copy_flags, dim3(grid), dim3(kCopyTPB), 0, st, aidx, agrp, m, (const u8*)bad, n, P);
  BWTC_HIP_TRY(t_flags.stop());
  BWTC_HIP_TRY(t_lengths.start());
  hipLaunchKernelGGL((k_stretch_tiles<false, true>), dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)P, n, 0u, d_runF);
  hipLaunchKernelGGL(k_run_carry, dim3(1), dim3(1024), 0, st, (const u32*)d_runF, tiles, n, d_runB);
  hipLaunchKernelGGL((k_stretch_lengths<false, false, false, true>), dim3(tiles), dim3(kRunTPB), 0, st, (const u8*)P, n, 0u, (const u32*)d_runB, d_runK,
                     d_small + kSmallStretch, 0u, 0u);
  BWTC_HIP_TRY(t_lengths.stop());
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallStretch, d_small + kSmallStretch, 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(wait());
  if (t_marks.on) {
    float a = 0.f, b = 0.f, c = 0.f;
    BWTC_HIP_TRY(t_marks.ms(&a)); BWTC_HIP_TRY(t_flags.ms(&b)); BWTC_HIP_TRY(t_lengths.ms(&c));
    std::fprintf(stderr, "copies: marks %.4f ms, flags %.4f ms, lengths %.4f ms for %u entries in %u groups, %u suffixes: longest K %u\n", a, b, c, m, groups, n,
                 h_small[kSmallStretch]);
  }
  *longest = h_small[kSmallStretch];
  blk.lengths_period = 0;
  // the marks read the list and gather a rank per entry; the flags read the list and store a byte; P[] cleared, read twice; K[] written
  stats.alg_bytes += (u64)m * (8 + 4) + (u64)m * (8 + 1 + 1) + (u64)groups + (u64)n * (1 + 2 + 4) + (u64)tiles * 16;
  return 0;
}

// The finder's candidates over the vote table in d_votes (k_period_winners): up to kPeriodCandidates (distance, votes)
// pairs with `need` votes or more into out[], most votes first -> their number (one host wait).
int BwtEngine::period_winners(u32 need, u32* out, u32* n_out) {
  hipStream_t st = stream;
  hipLaunchKernelGGL(k_period_winners, dim3(1), dim3(1024), 0, st, (const u32*)d_votes, need, d_small + kSmallPeriod + 2);
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallPeriod + 2, d_small + kSmallPeriod + 2, kPeriodCandidates * 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(wait());
  u32 found = 0;
  while (found < kPeriodCandidates && h_small[kSmallPeriod + 2 + 2 * found]) ++found;
  std::memcpy(out, h_small + kSmallPeriod + 2, kPeriodCandidates * 8);
  *n_out = found;
  stats.alg_bytes += (u64)kVoteBins * 4;
  return 0;
}

// The long finder ("Long periods") over the sorted list (ks, vs, m entries): sweep 1 with the short votes, the coarse bins
// with `need` votes, and -- behind one -- sweep 2 and the merged candidates.  A list has fewer than m votes to give:
// (m - 1) / need above kLongSel is refused before anything is launched (-1; the product's need never is).
int BwtEngine::long_period_votes(const u64* ks, const u32* vs, u32 m, u64 kmask, const u32* k1, u32 need, u32 dmax, bool winner_only, u32* out,
                                 u32* n_out, bool* swept) {
  *n_out = 0; *swept = false;
  std::memset(out, 0, kPeriodCandidates * 8);
  if (need == 0 || m < 2 || (u64)(m - 1) / need > kLongSel || dmax > kLongPeriodMax) return -1;
  hipStream_t st = stream;
  u32* const coarse = d_lvotes;
  u32* const sel = d_lvotes + kLongSelAt;
  u32* const fine = d_lvotes + kLongFineAt;
  u32* const d_cand = d_small + kSmallPeriod + 2;
  u32* const h_cand = h_small + kSmallPeriod + 2;
  const u32 tiles = ceil_div(m, kLongVoteTile);
  PassTimer t_one(st), t_two(st);
  BWTC_HIP_TRY(hipMemsetAsync(d_votes, 0, (size_t)kVoteBins * 4, st));
  BWTC_HIP_TRY(hipMemsetAsync(coarse, 0, (size_t)kCoarseBins * 4, st));
  BWTC_HIP_TRY(t_one.start());
  if (k1) hipLaunchKernelGGL(k_period_votes_long<true>, dim3(tiles), dim3(kVoteTPB), 0, st, ks, vs, m, kmask, d_votes, k1, coarse, dmax);
  else hipLaunchKernelGGL(k_period_votes_long<false>, dim3(tiles), dim3(kVoteTPB), 0, st, ks, vs, m, kmask, d_votes, (const u32*)nullptr, coarse, dmax);
  BWTC_HIP_TRY(t_one.stop());
  hipLaunchKernelGGL(k_long_coarse_pick, dim3(1), dim3(1024), 0, st, (const u32*)coarse, need, sel, d_small + kSmallLong);
  if (winner_only) {
    BWTC_HIP_TRY(hipMemsetAsync(d_cand + 2, 0, (kPeriodCandidates - 1) * 8, st));
    hipLaunchKernelGGL(k_period_winner, dim3(1), dim3(1024), 0, st, (const u32*)d_votes, d_cand);
  } else {
    hipLaunchKernelGGL(k_period_winners, dim3(1), dim3(1024), 0, st, (const u32*)d_votes, need, d_cand);
  }
  BWTC_HIP_TRY(hipMemcpyAsync(h_cand, d_cand, (kPeriodCandidates * 2 + 1) * 4, hipMemcpyDeviceToHost, st));   // (the candidates and kSmallLong behind them)
  BWTC_HIP_TRY(wait());
  const u32 n_sel = h_small[kSmallLong];
  if (t_one.on) {
    float ms = 0.f;
    BWTC_HIP_TRY(t_one.ms(&ms));
    std::fprintf(stderr, "periods: the vote kernel took %.4f ms for %u entries\n", ms, m);
    std::fprintf(stderr, "periods: sweep 1 of the long finder (the vote kernel with the coarse table) took %.4f ms, %u coarse bins with %u votes\n", ms, n_sel, need);
  }
  if (n_sel > kLongSel) return -1;                      // (cannot happen: the votes are fewer than m)
  if (n_sel) {
    const u32 groups = ceil_div(n_sel, kFineGroup);
    BWTC_HIP_TRY(hipMemsetAsync(fine, 0, (size_t)n_sel * kFineBins * 4, st));
    BWTC_HIP_TRY(t_two.start());
    if (k1) hipLaunchKernelGGL(k_period_votes_fine<true>, dim3(tiles, groups), dim3(kVoteTPB), 0, st, ks, vs, m, kmask, k1, (const u32*)sel, n_sel, fine, dmax);
    else hipLaunchKernelGGL(k_period_votes_fine<false>, dim3(tiles, groups), dim3(kVoteTPB), 0, st, ks, vs, m, kmask, (const u32*)nullptr, (const u32*)sel, n_sel, fine, dmax);
    BWTC_HIP_TRY(t_two.stop());
    // (winner_only: a short winner below `need` stays what it is where the merged candidates are none)
    u32* const d_merged = winner_only ? d_lvotes + kLongSelAt + kLongSel : d_cand;
    static_assert(kLongSelAt + kLongSel + 2 * kPeriodCandidates <= kLongFineAt, "the merged candidates' words");
    hipLaunchKernelGGL(k_long_period_winners, dim3(1), dim3(1024), 0, st, (const u32*)d_votes, (const u32*)sel, n_sel, (const u32*)fine, need, d_merged);
    u32* const merged = h_small + kSmallLong + 1;         // (2 * kPeriodCandidates spare words of the pinned mirror)
    BWTC_HIP_TRY(hipMemcpyAsync(merged, d_merged, 2 * kPeriodCandidates * 4, hipMemcpyDeviceToHost, st));
    BWTC_HIP_TRY(wait());
    if (!winner_only || merged[0]) std::memcpy(h_cand, merged, 2 * kPeriodCandidates * 4);
    if (t_two.on) {
      float ms = 0.f;
      BWTC_HIP_TRY(t_two.ms(&ms));
      std::fprintf(stderr, "periods: sweep 2 of the long finder took %.4f ms for %u coarse bins\n", ms, n_sel);
    }
    *swept = true;
  }
  u32 found = 0;
  while (found < kPeriodCandidates && h_cand[2 * found] && h_cand[2 * found + 1] >= need) ++found;
  std::memcpy(out, h_cand, kPeriodCandidates * 8);
  *n_out = found;
  return 0;
}

// The wide probe ("Long periods") over d_T: is any aligned window of `span` positions from p on free of breaks of period p?
int BwtEngine::long_period_probe(u32 n, u32 p, u32 span, bool* found) {
  *found = false;
  if (span == 0 || (u64)n + p + 2ull * kRunTile > 0xFFFFFFFFull) return 0;   // (the block that takes no step: stretch_lengths)
  const u64 windows = (u64)n > (u64)p + span ? ((u64)n - p) / span : 0;
  if (!windows) return 0;
  hipStream_t st = stream;
  BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallPeriod + 1, 0, 4, st));
  hipLaunchKernelGGL(k_period_probe_wide, dim3(depth32(windows)), dim3(256), 0, st, (const u8*)d_T, n, p, span, d_small + kSmallPeriod + 1);
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallPeriod + 1, d_small + kSmallPeriod + 1, 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(wait());
  *found = h_small[kSmallPeriod + 1] != 0;
  stats.alg_bytes += windows * 2;                       // (at the least, as the short probe counts)
  return 0;
}

// Candidate p, the finder's with its votes (or BWTC_HIP_PERIOD's), through what decides whether it is worth a step: the
// probe, the period-length pass (a trial unless store), the worth test and the division of a period above the first
// round's depth.  -> *out: the period that is left (0: refused) with the lengths of the last pass over it; a candidate
// that no pass was made for leaves lengths of 0.
int BwtEngine::weigh_period(u32 n, u64 h_first, bool mixed, bool store, u32 p, u32 votes, WeighedPeriod* out) {
  hipStream_t st = stream;
  const bool voted = period_forced == 0;                // (a forced period skips the probe, the worth tests and the division)
  WeighedPeriod w;
  w.p = p >= 2 ? p : 0u; w.votes = votes;
  u32* const proper = mixed ? &w.proper : nullptr;      // (the passes' second maximum exists under the rule only)
  if (w.p && voted) {
    // votes say how many members lie p apart, not for how long they tie: fixed-width records with a few free bytes
    // each vote for their width and tie for less than two records.  Before the pass, a probe: is any aligned window
    // of (W - p) / 2 positions free of breaks, W = kPeriodWorth x max(the first round's depth, p) being the stretch
    // the step is worth?  A stretch of W characters holds such a window; the probe's threads stop at their first break.
    const u64 worth = kPeriodWorth * std::max<u64>(h_first, w.p);
    const u32 span = (u32)std::min<u64>((worth - w.p) / 2, 0x40000000ull);
    const u64 windows = (u64)n > w.p + span ? ((u64)n - w.p) / span : 0;
    bool found = false;
    if (w.p > kPeriodMax) {
      // (BWTC_HIP_LONG_PERIODS: a window of a long period is a workgroup's, not a thread's -- the wide probe)
      const int rcl = long_period_probe(n, w.p, span, &found);
      if (rcl) return rcl;
    } else if (windows) {
      BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallPeriod + 1, 0, 4, st));
      hipLaunchKernelGGL(k_period_probe, dim3((u32)((windows + 255) / 256)), dim3(256), 0, st, (const u8*)d_T, n, w.p, span, depth32(windows), d_small + kSmallPeriod + 1);
      BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallPeriod + 1, d_small + kSmallPeriod + 1, 4, hipMemcpyDeviceToHost, st));
      BWTC_HIP_TRY(wait());
      found = h_small[kSmallPeriod + 1] != 0;
      stats.alg_bytes += windows * 2;                   // (at the least: a byte of each stream per window)
    }
    if (!found) {
      if (debug_on()) std::fprintf(stderr, "periods: no window of %u positions of period %u without a break: no period-length pass\n", span, w.p);
      w.p = 0;
    }
  }
  if (w.p) {
    // (a run of one byte is a stretch of every period, and the run step's business: the block's longest run first --
    // known already unless BWTC_HIP_RUNS=0, where a trial pass of period 1 finds it -- and no period step where the
    // longest stretch is no longer than that.  Under the rule runs do not count in the gate length, and the test goes.)
    const bool runs_count = !mixed && voted;
    int rcb = (runs_count && !run_ranks) ? stretch_lengths(n, 1, false, &blk.run_longest) : 0;
    if (rcb) return rcb;
    rcb = stretch_lengths(n, w.p, store, &w.longest, proper);
    if (rcb) return rcb;
    // ... and none where the gate length is short of kPeriodWorth times the depth it has to pass: doubling gets through
    // it in three rounds, and the step's own round and the passes cost as much
    if ((runs_count && blk.run_longest >= w.longest) || (voted && (u64)w.gate(mixed) < kPeriodWorth * std::max<u64>(h_first, w.p)))
      w.p = 0;
  }
  if (w.p && voted && (u64)w.p > h_first && (u64)w.gate(mixed) > w.p) {
    // The winner may be a multiple of the stretches' period: a list that a sort by windows of the suffix number
    // has been through holds a group's members in another order than by position.  A period above the first
    // round's depth defers the step, so it is worth dividing: p / q for the winner's prime factors q, kept while
    // the gate length stays as long (trial passes: the longest stretches alone, no lengths stored).
    // (No block of the tests or of scripts/sorter_trace.py has a winner that this loop reduces, so its handling of the
    // lengths is the one it always had, over the record instead of the block's words: the trial passes write into the
    // record, g reads whichever length the gate goes by, and the voted lengths are put back behind the loop.)
    const u32& g = mixed ? w.proper : w.longest;
    const u32 winner = w.p, longest_voted = w.longest, proper_voted = w.proper, g_voted = g;
    u32 rest = winner;
    for (u32 q = 2; q <= rest && w.p / q >= 2; ) {
      if (rest % q) { q = (u64)q * q > rest ? rest : q + 1; continue; }   // (no factor up to its root: what is left is prime)
      rest /= q;
      const int rcb = stretch_lengths(n, w.p / q, false, &w.longest, proper);
      if (rcb) return rcb;
      if (g >= g_voted) w.p /= q;
      else while (rest % q == 0) rest /= q;            // (the same candidate again)
    }
    w.longest = longest_voted; w.proper = proper_voted;
    if (w.p != winner) {
      const int rcb = stretch_lengths(n, w.p, store, &w.longest, proper);
      if (rcb) return rcb;
    }
  }
  *out = w;
  return 0;
}

// The block's closed-form steps, into blk.steps, for a list of m > 0 entries that is about to double and whose first round
// establishes depth h_first.  Once per block: run_rounds calls it before the one doubling list a block has.
int BwtEngine::decide_step(u32 n, u32 m, u64 h_first, const u64* ks, const u32* vs, u64 kmask) {
  // Runs: the list may hold long runs of one byte, which doubling takes log2(length) rounds over.  k[] and the block's
  // longest run are made here (one host wait); a run longer than the depth the first round establishes gets the run
  // step as that round, before any text round and before rank[] is completed.
  // (BWTC_HIP_PERIOD=1: the run step is the period step of period 1, whatever BWTC_HIP_RUNS says)
  if (run_ranks || period_forced == 1) {
    const int rcr = stretch_lengths(n, 1, true, &blk.run_longest);
    if (rcr) return rcr;
    if ((u64)blk.run_longest > h_first) blk.schedule(WeighedPeriod{1, blk.run_longest}, StretchStep::kThisRound);
    if (debug_on())
      std::fprintf(stderr, "runs: longest run %u, the rounds begin at depth %llu: %s\n", blk.run_longest, (unsigned long long)h_first,
                   blk.n_steps ? "run step" : "no run step");
  }
  // Periods: a list that takes doubling rounds and no run step may hold stretches of a period p > 1, which tie their
  // suffixes for the stretch's length just as a run does.  The finder votes for p over the list as it stands (or
  // BWTC_HIP_PERIOD names it); votes above the threshold buy the period-length pass, which puts k_p[] where k[] was.
  // p <= the first round's depth: that round is the period step, exactly as the run step.  A deeper p: the step waits
  // for the first doubling round whose depth reaches p (kWaiting), with rank[] complete and no local list beside it.
  // BWTC_HIP_MIXED=1 (with the run ranking on): the block that takes the run step looks for a period too, and the gates
  // are the longest PROPER stretch's -- the largest k_p over the positions s with T[s] != T[s + 1], which no run of one
  // byte holds and every p positions of a stretch of another unit do -- so a run neither counts as a stretch nor keeps
  // one from its step.
  const bool mixed = mixed_rule();
  const bool run_due = blk.n_steps != 0;
  if (!looks_for_period(run_due)) return 0;
  PeriodCandidates cands;
  const int rcp = find_period(n, ks, vs, m, kmask, &cands);
  if (rcp) return rcp;
  // BWTC_HIP_MULTI: every candidate of the finder's, most votes first, through the same probe, pass, worth test and
  // division (tests/multimodel.py, accept()), up to kMaxPeriodSteps accepted; a multiple or a divisor of an accepted
  // period is skipped -- a p'-stretch longer than p is a p-stretch when p' divides p -- before its passes and again
  // behind the division.  (A forced period is one candidate; a block of 2^31 bytes or more has no bit for the merged
  // words' flag.)  Else the leader alone.
  const bool several = multi_steps && mixed && period_forced == 0 && (u64)n <= kStepLength;
  const u32 n_cands = several ? cands.n : std::min(cands.n, 1u);
  // While a run step is due d_runK holds k_1[] for it, so the passes are trials.  Else the first candidate weighed stores
  // its lengths: where one period is all there is, the block is MIXED's from here on.
  const bool store = !run_due;
  WeighedPeriod acc[BlockSort::kMaxPeriodSteps];
  int na = 0;
  const auto related = [&](u32 q) { for (int i = 0; i < na; ++i) if (q % acc[i].p == 0 || acc[i].p % q == 0) return true; return false; };
  blk.weighed.votes = cands.at[0].votes;
  for (u32 c = 0; c < n_cands && na < BlockSort::kMaxPeriodSteps; ++c) {
    if (related(cands.at[c].p)) continue;
    WeighedPeriod w;
    const int rcw = weigh_period(n, h_first, mixed, store && c == 0, cands.at[c].p, cands.at[c].votes, &w);
    if (rcw) return rcw;
    if (w.longest) { blk.weighed.longest = w.longest; blk.weighed.proper = w.proper; }   // (a refused candidate's too: the last pass made)
    if (w.p && !related(w.p)) acc[na++] = w;
  }
  std::sort(acc, acc + na, [](const WeighedPeriod& a, const WeighedPeriod& b) { return a.p < b.p; });
  // The first round's steps are those with p <= h_first whose stretches are longer than that, by ascending p; the others
  // wait, by ascending p, as long as their stretches are longer than p.
  const auto first_round = [&](const WeighedPeriod& w) { return (u64)w.p <= h_first && (u64)w.gate(mixed) > h_first; };
  const auto waits = [&](const WeighedPeriod& w) { return (u64)w.p > h_first && w.gate(mixed) > w.p; };
  // Several periods: the steps merge their look-up lengths in d_runK, each storing when it is due (step_due, store_step).
  // One period: d_runK holds its k_p[] alone, stored here -- by the first candidate's pass above, or now where another
  // candidate stored or where the step is the first round's over a run step that was due: ONE period step over k_p[]
  // instead, which ranks the runs too (k_p = k_1 for k_1 >= p), so the storing pass overwrites k_1[].  (A step that
  // waits behind the run step stores when it is due.)
  blk.merged = na >= 2;
  if (na == 1 && (store ? blk.lengths_period != acc[0].p : first_round(acc[0]))) {
    const int rcb = stretch_lengths(n, acc[0].p, true, &acc[0].longest, mixed ? &acc[0].proper : nullptr);
    if (rcb) return rcb;
  }
  if (na) blk.weighed = acc[0];
  bool any_first = false;
  for (int i = 0; i < na; ++i) any_first = any_first || first_round(acc[i]);
  if (any_first) blk.n_steps = 0;                        // (the first of them ranks the runs too, in place of the run step that was due)
  int period_steps = 0;
  for (int i = 0; i < na; ++i)
    if (first_round(acc[i])) {
      blk.schedule(acc[i], StretchStep::kThisRound);
      if (run_due && blk.n_steps == 1) blk.steps[0].ranks_runs = true;
      ++period_steps;
    }
  for (int i = 0; i < na; ++i)
    if (waits(acc[i])) { blk.schedule(acc[i], StretchStep::kWaiting); ++period_steps; }   // behind the run step, if one is due (step_due)
  // (a voted period that was accepted is the first round's or waits, by the worth test; a forced one may be neither)
  if (!period_steps) say_no_period_step(*this, h_first);
  return 0;
}

// The block's candidate periods, most votes first: BWTC_HIP_PERIOD's, or those of the vote over the list whose votes reach
// the threshold -- a 64th of the block, and kPeriodMinVotes at the least; the leader alone unless BWTC_HIP_MULTI.
int BwtEngine::find_period(u32 n, const u64* ks, const u32* vs, u32 m, u64 kmask, PeriodCandidates* out) {
  *out = PeriodCandidates{};
  if (period_forced) { out->n = 1; out->at[0].p = period_forced; return 0; }
  if (m < 2) return 0;
  hipStream_t st = stream;
  const u64 need = std::max<u64>(kPeriodMinVotes, (u64)n / 64);
  // (d_runK holds k_1[] where the run step is due: decide_step made it just now)
  const bool runs_out = mixed_steps && blk.lengths_period == 1 && blk.steps[0].p == 1;
  u32 found[2 * kPeriodCandidates] = {}, n_found = 0;   // (distance, votes) pairs, as the finder's kernels leave them (PeriodCandidates::at)
  bool say_leader = false;
  if (long_periods) {
    // BWTC_HIP_LONG_PERIODS: the same pass over the list votes for the distances up to min(kLongPeriodMax, n / 8) too (a
    // longer period's stretch of kPeriodWorth periods has no room in the block), and the candidates are the merged ones
    const u32 dmax = (u32)std::min<u64>(kLongPeriodMax, (u64)n / kPeriodWorth);
    bool swept = false;
    const int rcl = long_period_votes(ks, vs, m, kmask, runs_out ? (const u32*)d_runK : nullptr, (u32)need, dmax, !multi_steps, found, &n_found, &swept);
    if (rcl) return rcl;
    // (what the short finder counts, so that a block without a long candidate counts what it did; sweep 2: the list again, its tables)
    stats.alg_bytes += (u64)m * (8 + 4) + (u64)kVoteBins * 8 + (multi_steps ? (u64)kVoteBins * 4 : 0) + (swept ? (u64)m * (8 + 4) + (u64)kLongSel * kFineBins * 4 : 0);
  } else {
    PassTimer timer(st);
    BWTC_HIP_TRY(hipMemsetAsync(d_votes, 0, (size_t)kVoteBins * 4, st));
    BWTC_HIP_TRY(timer.start());
    if (runs_out)
      hipLaunchKernelGGL(k_period_votes<true>, dim3(ceil_div(m, kVoteTile)), dim3(kVoteTPB), 0, st, ks, vs, m, kmask, d_votes, (const u32*)d_runK);
    else
      hipLaunchKernelGGL(k_period_votes<false>, dim3(ceil_div(m, kVoteTile)), dim3(kVoteTPB), 0, st, ks, vs, m, kmask, d_votes, (const u32*)nullptr);
    BWTC_HIP_TRY(timer.stop());
    if (multi_steps) {
      // BWTC_HIP_MULTI: the up to kPeriodCandidates distances whose votes reach the threshold, not the winner alone
      const int rcw = period_winners((u32)need, found, &n_found);
      if (rcw) return rcw;
    } else {
      hipLaunchKernelGGL(k_period_winner, dim3(1), dim3(1024), 0, st, (const u32*)d_votes, d_small + kSmallPeriod + 2);
      BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallPeriod + 2, d_small + kSmallPeriod + 2, 8, hipMemcpyDeviceToHost, st));
      BWTC_HIP_TRY(wait());
      found[0] = h_small[kSmallPeriod + 2]; found[1] = h_small[kSmallPeriod + 3];
    }
    if (timer.on) {
      float ms = 0.f;
      BWTC_HIP_TRY(timer.ms(&ms));
      std::fprintf(stderr, "periods: the vote kernel took %.4f ms for %u entries\n", ms, m);
    }
    say_leader = timer.on;                              // (the long finder says what its sweeps found instead)
    stats.alg_bytes += (u64)m * (8 + 4) + (u64)kVoteBins * 8;   // the list's keys and suffixes read; the table zeroed and read
  }
  // the winner alone: one candidate, if its votes reach the threshold
  if (!multi_steps) n_found = (found[0] >= 2 && (u64)found[1] >= need) ? 1u : 0u;
  out->n = n_found;
  for (u32 c = 0; c < kPeriodCandidates; ++c) { out->at[c].p = found[2 * c]; out->at[c].votes = found[2 * c + 1]; }
  if (!out->n && say_leader) std::fprintf(stderr, "periods: distance %u leads with %u votes of the %llu a pass takes\n", found[0], found[1], (unsigned long long)need);
  return 0;
}

// The finisher passes over the list the long-key ranking left (k_finish).  Every entry knows the depth
// its group shares (the upper byte of its character field); a pass adds kFinChars to it.  Passes go on
// while the list shrinks: one that keeps more than three fifths of a list that is still longer than
// n / 64 has met deep repeats (copies of whole files, not of lines), which only doubling gets through.
// What is left for the rounds, as raw lists (suffix; head slot << 32 | slot), unsorted:
//   *shallow entries in (home.vals, home.rec_free): groups too large for a window that share fewer than
//    fin_floor characters; they share at least *h_shallow
//   `parked` entries in (d_parkS, d_parkHP): the other groups too large for a window, and what the last
//    pass left tied; at least *h_parked characters
//
// The lists a pass writes hold fin_list_cap(cap) entries, and a pass needs room for its regions' worst case:
// chunk c of 64 workgroups appends to region c mod 16 and leaves at most its workgroups' strides of entries and one
// group more -- m + m / 64 in the wide shape (stride and group 1024).  A pass (or the local list's steps) whose room
// would not fit is not made: the list goes to the global rounds as it stands (stats.route bit 7).
static bool fin_room(const FinRegions& rg, u32 stride, u32 group, u64 lcap, FinOut* ob) {
  u64 room[kFinRegions] = {};
  const u32 grid = rg.wfirst[rg.nreg];
  const u32 nchunks = ceil_div(grid, kFinChunk);
  for (u32 c = 0; c < nchunks; ++c) {
    const u32 wgs = std::min(kFinChunk, grid - c * kFinChunk);
    room[c % kFinRegions] += (u64)wgs * stride + group;
  }
  u64 at = 0;
  for (u32 r = 0; r < kFinRegions; ++r) { ob->base[r] = (u32)std::min<u64>(at, 0xFFFFFFFFu); at += room[r]; }
  return at <= lcap;
}
// A list of m entries as one region, from entry 0.
static FinRegions fin_one_region(u32 m, u32 stride) {
  FinRegions rg{};
  rg.nreg = 1; rg.wfirst[1] = ceil_div(m, stride); rg.ecount[0] = m;
  return rg;
}
// The regions a pass left, from its region counts and its FinOut (the empty ones left out); *total: their entries.
static FinRegions fin_regions_left(const u32* counts, const FinOut& ob, u32 stride, u32* total) {
  FinRegions nx{};
  *total = 0;
  for (u32 r = 0; r < kFinRegions; ++r) {
    const u32 c = counts[r];
    if (!c) continue;
    nx.ebase[nx.nreg] = ob.base[r]; nx.ecount[nx.nreg] = c;
    nx.wfirst[nx.nreg + 1] = nx.wfirst[nx.nreg] + ceil_div(c, stride);
    ++nx.nreg;
    *total += c;
  }
  if (nx.nreg == 0) nx.nreg = 1;
  return nx;
}

// One k_finish launch: the list it reads and its regions, the list it leaves and where each region of that starts (fin_room),
// the hard sink, the shallow sink, and the ranks of a local step.
struct FinLaunch {
  u32 n; FinList in; FinRegions rg; FinList out; FinOut ob;
  u32* hardS; u64* hardHP; unsigned short* hardC; FinShallow shal; bool ranks; FinRank rk;
  // a pass of the finisher: hard groups go to (hardS, hardHP) with their characters in d_hardC, shallow ones to shal
  static FinLaunch pass(const BwtEngine& e, u32 n, FinList in, const FinRegions& rg, FinList out, const FinOut& ob, u32* hardS, u64* hardHP, FinShallow shal) {
    return FinLaunch{n, in, rg, out, ob, hardS, hardHP, e.d_hardC, shal, false, FinRank()};
  }
  // a step of the local list, from its home `home` to the other, by rank[s + at] and rank[s + at2]: no group is too large
  // and none is shallow, so the hard characters' array is never written and the shallow sink is a dummy with floor 0
  static FinLaunch local_step(const BwtEngine& e, u32 n, int home, const FinRegions& rg, const FinOut& ob, u32 at, u32 at2) {
    return FinLaunch{n, e.local_list(home), rg, e.local_list(1 - home), ob, e.d_parkS, e.d_parkHP, e.d_LC1,
                     FinCounters(e).shallow_sink(e.d_parkS, e.d_parkHP, 0u), true, FinRank{e.d_rank, at, at2, e.d_US, e.d_UR}};
  }
};

// One k_finish launch in this block's shape (blk.fin.window / group): the passes' (fin_words words of characters, or
// fin_rounds rounds of two), the local list's steps (q.ranks), and, launch by launch, the test hooks'
// (BwtEngine::test_finish_pass).  The counters are the finisher's own (FinCounters).
static void launch_finish(BwtEngine& e, const FinLaunch& q, const RrEmit& re) {
  hipStream_t st = e.stream;
  const int window = e.blk.fin.window, group = e.blk.fin.group, fin_words = e.fin_words, fin_rounds = e.fin_rounds;
  const auto& [n, a, rg, b, ob, hardS, hardHP, hardC, shal, ranks, ranks_by] = q;   // (the names the launches below are written in)
  u32 *ncnt = FinCounters(e).word(kFinNext), *hard_count = FinCounters(e).word(kFinHard);
  const FinRank* rk = ranks ? &ranks_by : nullptr;
  const u32 grid = rg.wfirst[rg.nreg];
#define BWTC_FINISH_W(G, E, NW) hipLaunchKernelGGL((k_finish<G, E, NW>), dim3(grid), dim3(kFinTPB), 0, st, a, rg, (const u8*)e.d_T, n, \
                                             b, ob, ncnt, hardS, hardHP, hardC, hard_count, shal, e.d_SA, re)
#define BWTC_FINISH_R(G, E, NR) hipLaunchKernelGGL((k_finish<G, E, 2, false, NR>), dim3(grid), dim3(kFinTPB), 0, st, a, rg, (const u8*)e.d_T, n, \
                                             b, ob, ncnt, hardS, hardHP, hardC, hard_count, shal, e.d_SA, re)
#define BWTC_LOCAL(G, E) hipLaunchKernelGGL((k_finish<G, E, 2, true>), dim3(grid), dim3(kFinTPB), 0, st, a, rg, (const u8*)e.d_T, n, \
                                            b, ob, ncnt, hardS, hardHP, hardC, hard_count, shal, e.d_SA, re, *rk)
#define BWTC_FINISH(G, E) do { if (rk) BWTC_LOCAL(G, E); \
                               else if (fin_words >= 4) BWTC_FINISH_W(G, E, 4); else if (fin_words == 3) BWTC_FINISH_W(G, E, 3); \
                               else if (fin_rounds >= 4) BWTC_FINISH_R(G, E, 4); else if (fin_rounds == 3) BWTC_FINISH_R(G, E, 3); \
                               else if (fin_rounds == 2) BWTC_FINISH_R(G, E, 2); else BWTC_FINISH_W(G, E, 2); } while (0)
  if (window <= 1024) { if (group <= 256) BWTC_FINISH(256, kFinE1); else BWTC_FINISH(512, kFinE1); }
  else if (group <= 256) BWTC_FINISH(256, kFinE2);
  else if (group <= 512) BWTC_FINISH(512, kFinE2);
  else BWTC_FINISH(1024, kFinE2);
#undef BWTC_FINISH
#undef BWTC_LOCAL
#undef BWTC_FINISH_W
#undef BWTC_FINISH_R
}

int BwtEngine::finisher_passes(FinWork& w, const FinRequest& rq, FinOutcome* fo) {
  u32& m = w.m;
  const FinCounters fc(*this);
  fc[kFinSpare] = 0; fc[kFinHard] = 0; fc[kFinHardDepth] = 0xFFFFFFFFu;
  BWTC_HIP_TRY(fc.upload(kFinSpare, kFinHardDepth));
  blk.fin.passes_done = 0;
  const u32 park0 = blk.fin.parked;        // the groups too large for a window join the waiting list from here
  const u32 stride = blk.fin.stride();
  w.rg = fin_one_region(m, stride);        // the list as given is one region
  const u32 pass_chars = 8u * (u32)fin_words * (fin_words == 2 ? (u32)fin_rounds : 1u);
  const int depth_passes = (int)((255u - 48u) / pass_chars);      // the depth byte holds 255 (a level's depth is 48 at most)
  for (int it = 0; it < std::min(std::min(fin_max_passes, std::max(1, depth_passes)), rq.max_passes) && m > 0; ++it) {
    // the regions of the list this pass leaves
    FinOut ob;
    if (!fin_room(w.rg, stride, (u32)blk.fin.group, fin_list_cap(cap), &ob)) {
      stats.route |= 128u;
      if (debug_on())
        std::fprintf(stderr, "finisher pass %d: %u entries would not fit the lists in this shape (%d / %d); on to the rounds\n", it, m, blk.fin.window, blk.fin.group);
      break;
    }
    ++stats.rounds;
    stats.active_sum += m;
    stats.finisher_entries += m;
    stats.route |= 2u;
    // a window of entries is read by the workgroups whose windows overlap there (4/3 on average), sixteen characters
    // (three aligned words) per owned entry, a byte and a suffix per finished one, an entry per member that stays
    stats.alg_bytes += (u64)m * (14 * 4 / 3 + (pass_chars + 8) + 5);
    BWTC_HIP_TRY(fc.clear(kFinNext, kFinGroupsLeft));
    launch_finish(*this, FinLaunch::pass(*this, rq.n, w.a, w.rg, w.b, ob, d_parkS + park0, d_parkHP + park0, rq.shal), rq.re);
    BWTC_HIP_TRY(fc.fetch(kFinSpare, kFinShallowDepth));
    BWTC_HIP_TRY(fc.fetch(kFinNext, kFinGroupsLeft));
    BWTC_HIP_TRY(wait());
    const u32 m_was = m;
    w.rg = fin_regions_left(&fc[kFinNext], ob, stride, &m);   // what the pass left, region by region
    if (debug_on())
      std::fprintf(stderr, "finisher pass %d: %u entries -> %u still tied; %u hard (depth from %u), %u shallow (from %u)\n", it, m_was, m,
                   fc[kFinHard], fc[kFinHardDepth], fc[kFinShallow], fc[kFinShallowDepth]);
    std::swap(w.a, w.b);
    blk.fin.passes_done = it + 1;
    if (m < 4096u) break;                                                          // a handful: they join the waiting list (a pass of their own is a launch and a host wait for nothing)
    if (it >= 1 && (u64)m * 5 > (u64)m_was * 3 && (u64)m * 64 > (u64)rq.n) break;     // deep repeats: on to the rounds
    if (it >= 2 && (u64)m * 4 > (u64)m_was * 3) break;                             // a list that hardly shrinks any more: the rounds double, this creeps
  }
  // (the mirror holds what the last pass read back: the hard list's words, or their reset values where no pass ran)
  blk.fin.parked += fc[kFinHard];
  if ((u64)blk.fin.parked > cap) return -3;
  fo->hard = fc[kFinHard]; fo->hard_depth = fc[kFinHardDepth];
  // (a pass has run: no group above the bound is left in the list; and its groups are small -- the comparison loop costs a
  // group's size per member: a block that is one text 256 times over has groups of 256 throughout and is the global rounds')
  // (the local list's steps leave up to kFinRegions regions of it: room for that many more windows)
  FinOut unused;
  const bool local_fits = fin_room(fin_one_region(m + kFinRegions * stride, stride), stride, (u32)blk.fin.group, fin_list_cap(cap), &unused);
  const bool want_local = m && rq.keep_local && blk.fin.passes_done >= 1 && (u64)m * 64 >= (u64)rq.n && (u64)fc[kFinGroupsLeft] * 24 >= (u64)m;
  if (want_local && !local_fits) stats.route |= 128u;
  const int rc = (want_local && local_fits) ? local_handover(w, fo) : m ? park_rest(w, rq, fo) : 0;
  fo->shallow = fc[kFinShallow]; fo->shallow_depth = fc[kFinShallowDepth];
  return rc;
}

// One region of a list's arrays as a list of its own.
static FinList fin_part(const FinList& a, u32 base) { return FinList{a.S + base, a.P + base, a.H + base, a.C + base}; }

// Deep repeats in small groups: the doubling rounds take them group by group (local_pass), not through the global sort.
// What the last pass left becomes the local list, one region in its home 0.
int BwtEngine::local_handover(const FinWork& w, FinOutcome* fo) {
  const FinCounters fc(*this);
  u32 at = 0;
  for (u32 r = 0; r < w.rg.nreg; ++r) {
    if (!w.rg.ecount[r]) continue;
    hipLaunchKernelGGL(k_list_copy, dim3(ceil_div(w.rg.ecount[r], 256)), dim3(256), 0, stream, fin_part(w.a, w.rg.ebase[r]), w.rg.ecount[r], local_list(0), at,
                       fc.word(kFinLocalDepth));
    at += w.rg.ecount[r];
  }
  BWTC_HIP_TRY(fc.fetch(kFinLocalDepth, kFinLocalDepth));
  BWTC_HIP_TRY(wait());
  blk.fin.local_depth = fc[kFinLocalDepth];
  // its smallest depth: every member has taken the same passes, from a level's depth
  blk.fin.local_m = fo->local = w.m;
  blk.fin.local_rg = fin_one_region(w.m, blk.fin.stride()); blk.fin.local_home = 0;
  return 0;
}

// What the last pass left tied waits for the rounds: appended to d_parkS / d_parkHP.
int BwtEngine::park_rest(const FinWork& w, const FinRequest& rq, FinOutcome* fo) {
  const FinCounters fc(*this);
  if ((u64)blk.fin.parked + w.m > cap) return -3;
  for (u32 r = 0; r < w.rg.nreg; ++r) {
    if (!w.rg.ecount[r]) continue;
    hipLaunchKernelGGL(k_fin_to_hard, dim3(ceil_div(w.rg.ecount[r], 256)), dim3(256), 0, stream, fin_part(w.a, w.rg.ebase[r]), w.rg.ecount[r], d_parkS, d_parkHP,
                       blk.fin.parked, fc.word(kFinWaitDepth), blk.fin.passes_done ? FinShallow{rq.shal.S, rq.shal.HP, rq.shal.count, 0u} : rq.shal);
    blk.fin.parked += w.rg.ecount[r];
  }
  if (!blk.fin.passes_done) {
    // a list no pass has looked at: its shallow entries went to the shallow list and left holes behind
    const u32 before = fc[kFinShallow];
    BWTC_HIP_TRY(fc.fetch(kFinShallow, kFinShallowDepth));
    BWTC_HIP_TRY(wait());
    blk.fin.park_holes += fc[kFinShallow] - before;
  }
  fo->left = w.m;
  return 0;
}

// The local list: what the finisher's passes left of a block with deep repeats -- small groups (none above the
// finisher's bound), many of them.  In the doubling rounds it is refined group by group in LDS (k_finish<RANK>)
// beside the global list, which keeps the groups too large for that.
FinList BwtEngine::local_list(int home) const {
  if (home == 0) return FinList{d_hardS, d_LP0, d_LH0, d_hardC};
  return FinList{reinterpret_cast<u32*>(d_hardHP), reinterpret_cast<u32*>(d_hardHP) + fin_list_cap(cap), d_LH1, d_LC1};
}
int BwtEngine::local_updates() {
  if (!blk.fin.local_pending) return 0;
  hipStream_t st = stream;
  for (u32 r = 0; r < blk.fin.local_upd.nreg; ++r)
    if (blk.fin.local_upd.ecount[r])
      hipLaunchKernelGGL(k_rank_updates, dim3(ceil_div(blk.fin.local_upd.ecount[r], 1024)), dim3(256), 0, st, (const u32*)d_US, (const u32*)d_UR,
                         blk.fin.local_upd.ebase[r], blk.fin.local_upd.ecount[r], d_rank);
  blk.fin.local_pending = false;
  return 0;
}
// One doubling step of the local list.  h_global: the depth the global list's groups are sorted to (0: there is no
// global list); every rank[] entry is at least min(h_global, local_depth) deep, so a member looks up rank[s + local_depth]
// and, that far behind it, a second rank: the step adds twice that depth.  A local list far ahead of the global one
// (two of its steps and more) sits the round out.
int BwtEngine::local_pass(u32 n, u64 h_global, RrEmit& re) {
  if (blk.fin.local_m == 0) return 0;
  if (h_global && (u64)blk.fin.local_depth >= 2 * h_global) return 0;
  const u64 delta = h_global ? std::min<u64>(h_global, blk.fin.local_depth) : blk.fin.local_depth;
  const u64 at = blk.fin.local_depth, at2 = (u64)blk.fin.local_depth + delta;
  if (at2 + delta > 0xFFFFFFF0ull) return -3;
  const FinCounters fc(*this);
  BWTC_HIP_TRY(fc.clear(kFinNext, kFinNextLast));
  BWTC_HIP_TRY(fc.clear(kFinHard, kFinHard));
  FinOut ob;
  // (the shape is the passes': the local list's groups are as large as they left them; finisher_passes keeps lists without room off this route)
  if (!fin_room(blk.fin.local_rg, blk.fin.stride(), (u32)blk.fin.group, fin_list_cap(cap), &ob)) return -3;
  launch_finish(*this, FinLaunch::local_step(*this, n, blk.fin.local_home, blk.fin.local_rg, ob, (u32)at, (u32)at2), re);
  BWTC_HIP_TRY(fc.fetch(kFinHard, kFinHard));
  BWTC_HIP_TRY(fc.fetch(kFinNext, kFinNextLast));
  BWTC_HIP_TRY(wait());
  if (fc[kFinHard]) return -3;                            // a group above the finisher's bound in a list that has none
  stats.finisher_entries += blk.fin.local_m;
  stats.active_sum += blk.fin.local_m;
  stats.route |= 64u;
  stats.alg_bytes += (u64)blk.fin.local_m * (14 * 4 / 3 + 8 + 8 + 5 + 8 + 4);
  blk.fin.local_upd = blk.fin.local_rg;
  blk.fin.local_pending = true;
  const u32 m_was = blk.fin.local_m;
  blk.fin.local_rg = fin_regions_left(&fc[kFinNext], ob, blk.fin.stride(), &blk.fin.local_m);
  if (debug_on())
    std::fprintf(stderr, "local pass: %u entries at depth %u (+ 2 x %llu) -> %u still tied\n", m_was, blk.fin.local_depth, (unsigned long long)delta, blk.fin.local_m);
  blk.fin.local_home = 1 - blk.fin.local_home;
  blk.fin.local_depth = (u32)std::min<u64>(at2 + delta, 0xFFFFFFF0ull);
  return 0;
}

// ---- test hook: one k_finish launch ("The finisher hooks") -------------------------------------------
// What k_finish assumes of its list, checked on the host: a list that breaks it makes the kernel store past its arrays.
static bool fin_test_list_ok(const FinPassTest& t, u64 cap, FinRegions* rg, FinOut* ob, u32* m_out, u32* span_out, u64* room_out) {
  const u32 n = t.n;
  const u64 lcap = fin_list_cap(cap);
  if (n < 1u || (u64)n + TestCanaries::kBytes > cap) return false;
  if (!((t.window == 1024 && (t.group == 256 || t.group == 512)) || (t.window == 2048 && (t.group == 256 || t.group == 512 || t.group == 1024)))) return false;
  if (t.words < 2 || t.words > 4 || t.rounds < 1 || t.rounds > 4 || (t.words != 2 && t.rounds != 1)) return false;
  if (t.ranks && (t.words != 2 || t.rounds != 1)) return false;
  if (t.nreg < 1u || t.nreg > kFinRegions) return false;
  if (t.lf_n > 256u || (t.lf_n > 1u && (t.lf_x != n / t.lf_n || t.lf_x < 1u))) return false;
  if (t.out_n != n && t.out_n + 1u != n) return false;
  const u32 stride = (u32)(t.window - t.group);
  std::memset(rg, 0, sizeof *rg);
  rg->nreg = t.nreg;
  u64 m = 0, end = 0;
  for (u32 r = 0; r < t.nreg; ++r) {
    if ((u64)t.ebase[r] < end) return false;                           // ascending, disjoint
    end = (u64)t.ebase[r] + t.ecount[r];
    if (end + 128u > lcap) return false;                               // (and room for the canary behind the 16-bit array)
    rg->ebase[r] = t.ebase[r]; rg->ecount[r] = t.ecount[r];
    rg->wfirst[r + 1] = rg->wfirst[r] + ceil_div(t.ecount[r], stride);
    m += t.ecount[r];
  }
  if (m < 1u || m > n) return false;
  if (!fin_room(*rg, stride, (u32)t.group, lcap, ob)) return false;
  const u32 grid = rg->wfirst[rg->nreg];
  const u64 room = (u64)grid * stride + (u64)ceil_div(grid, kFinChunk) * (u32)t.group;     // where fin_room's last region ends
  if (room + 128u > lcap || room > t.next_cap) return false;
  std::vector<u8> seen_s(n, 0), seen_p(n, 0);
  for (u32 r = 0; r < t.nreg; ++r) {
    u32 run = 0;                                                       // members of the current group so far
    for (u32 i = t.ebase[r]; i < t.ebase[r] + t.ecount[r]; ++i) {
      const u32 s = t.S[i], p = t.P[i], h = t.H[i];
      if (s >= n || p >= n || seen_s[s] || seen_p[p]) return false;
      seen_s[s] = 1; seen_p[p] = 1;                                    // (distinct P: no head in two runs or two regions)
      const bool cont = run > 0 && t.H[i - 1] == h;
      if (cont) {
        if (p != h + run || (t.C[i] >> 8) != (t.C[i - 1] >> 8)) return false;
        ++run;
      } else {
        if (t.ranks && run > 0 && run < 2u) return false;
        if (p != h) return false;
        run = 1;
      }
      if (t.ranks && run > (u32)t.group) return false;
    }
    if (t.ranks && t.ecount[r] && run < 2u) return false;
  }
  if (t.ranks) {
    if (!t.rank || t.at < 1u || (t.at2 != 0u && t.at2 <= t.at)) return false;
    if (t.at2 && (u64)t.at2 + (t.at2 - t.at) >= 0xFFFFFFF0ull) return false;
    for (u32 i = 0; i < n; ++i) if (t.rank[i] >= n) return false;
  }
  *m_out = (u32)m; *span_out = (u32)end; *room_out = room;
  return true;
}

// A test hook's arrays, each with its bytes: poisoned (fill), then a canary behind each (can); copied, array by array.  A
// list's four arrays over `entries` entries, and a raw list's two (suffix; head slot << 32 | slot).
struct TestSpan { const void* p; u64 bytes; };
static hipError_t fin_test_guard(const std::vector<TestSpan>& arrays, bool fill, TestCanaries* can, hipStream_t st) {
  hipError_t rc = hipSuccess;
  for (const TestSpan& a : arrays) if (fill && rc == hipSuccess) rc = hipMemsetAsync(const_cast<void*>(a.p), 0xA5, a.bytes, st);
  for (const TestSpan& a : arrays) if (can && rc == hipSuccess) rc = can->put(const_cast<void*>(a.p), a.bytes, st);
  return rc;
}
static hipError_t fin_test_copy(const std::vector<TestSpan>& to, const std::vector<TestSpan>& from, hipMemcpyKind kind, hipStream_t st) {
  hipError_t rc = hipSuccess;
  for (size_t i = 0; i < to.size(); ++i) if (rc == hipSuccess) rc = hipMemcpyAsync(const_cast<void*>(to[i].p), from[i].p, to[i].bytes, kind, st);
  return rc;
}
static std::vector<TestSpan> fin_spans(const void* S, const void* P, const void* H, const void* C, u64 entries) { return {{S, entries * 4}, {P, entries * 4}, {H, entries * 4}, {C, entries * 2}}; }
static std::vector<TestSpan> fin_spans(const FinList& x, u64 entries) { return fin_spans(x.S, x.P, x.H, x.C, entries); }
static std::vector<TestSpan> fin_spans(const void* S, const void* HP, u64 entries) { return {{S, entries * 4}, {HP, entries * 8}}; }

// the emissions of a hooked launch: SA, out, pidx, last_char and lf[] poisoned, and the RrEmit that points at them
static hipError_t fin_test_emit_begin(BwtEngine& e, u32 n, u32 out_n, u32 lf_n, u32 lf_x, RrEmit* re) {
  hipStream_t st = e.stream;
  hipError_t rc = hipMemsetAsync(e.d_SA, 0xA5, (u64)n * 4, st);
  if (rc == hipSuccess) rc = hipMemsetAsync(e.d_out, 0xA5, n, st);
  if (rc == hipSuccess) rc = hipMemsetAsync(e.d_small + kSmallLf, 0xA5, 256 * 4, st);
  if (rc == hipSuccess) rc = hipMemsetAsync(e.d_small + kSmallPidx, 0xA5, 4, st);
  if (rc == hipSuccess) rc = hipMemsetAsync(e.d_small + kSmallLastChar, 0xA5, 4, st);
  std::memset(re, 0, sizeof *re);
  re->out = e.d_out; re->out_n = out_n; re->last_char = e.d_small + kSmallLastChar; re->pidx = e.d_small + kSmallPidx; re->T = e.d_T;
  re->lf = e.d_small + kSmallLf; re->lf_n = lf_n; re->lf_x = lf_x; re->lf_inv = lf_x > 1u ? (u32)((1ull << 32) / lf_x) : 0u;
  return rc;
}
static hipError_t fin_test_emit_fetch(BwtEngine& e, u32 n, u32* SA, u8* out, u32* small, u32* lf) {
  hipStream_t st = e.stream;
  hipError_t rc = hipMemcpyAsync(SA, e.d_SA, (u64)n * 4, hipMemcpyDeviceToHost, st);
  if (rc == hipSuccess) rc = hipMemcpyAsync(out, e.d_out, n, hipMemcpyDeviceToHost, st);
  if (rc == hipSuccess) rc = hipMemcpyAsync(small, e.d_small + kSmallPidx, 4, hipMemcpyDeviceToHost, st);
  if (rc == hipSuccess) rc = hipMemcpyAsync(small + 1, e.d_small + kSmallLastChar, 4, hipMemcpyDeviceToHost, st);
  if (rc == hipSuccess) rc = hipMemcpyAsync(lf, e.d_small + kSmallLf, 256 * 4, hipMemcpyDeviceToHost, st);
  return rc;
}

// The finisher's knobs while a hook runs: the passes' shape from the hook's arguments (block state, like everything else
// a hook leaves changed in blk: the next transform begins with a new BlockSort), and the context's switches -- words,
// rounds, floor, and fin_max_passes at its default of eight whatever BWTC_HIP_FIN_PASSES said when the context was
// made -- which are put back when the hook returns.
struct FinKnobScope {
  BwtEngine& e;
  const int words, rounds, max_passes; const u32 floor;
  FinKnobScope(BwtEngine& eng, int w, int g, int nw, int nr, u32 fl)
      : e(eng), words(eng.fin_words), rounds(eng.fin_rounds), max_passes(eng.fin_max_passes), floor(eng.fin_floor) {
    e.blk.fin.window = w; e.blk.fin.group = g; e.fin_words = nw; e.fin_rounds = nr; e.fin_floor = fl; e.fin_max_passes = 8;
  }
  ~FinKnobScope() { e.fin_words = words; e.fin_rounds = rounds; e.fin_floor = floor; e.fin_max_passes = max_passes; }
};

int BwtEngine::test_finish_pass(FinPassTest& t) {
  FinRegions rg; FinOut ob;
  u32 m = 0, span = 0; u64 room = 0;
  if (!fin_test_list_ok(t, cap, &rg, &ob, &m, &span, &room)) return -1;
  hipStream_t st = stream;
  const u32 n = t.n;
  FinKnobScope knobs(*this, t.window, t.group, t.words, t.rounds, t.floor);
  // the lists' homes: the passes' own arrays, the local list's two homes in RANK mode
  FinWork w;
  BWTC_HIP_TRY(finisher_begin(d_V0, m, &w));            // (and the shallow list's counter words)
  const FinCounters fc(*this);
  const FinLaunch q = t.ranks ? FinLaunch::local_step(*this, n, 0, rg, ob, t.at, t.at2)
                              : FinLaunch::pass(*this, n, w.a, rg, w.b, ob, d_parkS, d_parkHP, fc.shallow_sink(d_V1, static_cast<u64*>(d_R2), fin_floor));
  TestCanaries can;
  BWTC_HIP_TRY(fin_test_copy(fin_spans(q.in, span), fin_spans(t.S, t.P, t.H, t.C, span), hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(q.in, span), false, &can, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(q.out, room), true, &can, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(d_parkS, d_parkHP, m), true, &can, st));
  if (t.ranks) {
    BWTC_HIP_TRY(hipMemcpyAsync(d_rank, t.rank, (u64)n * 4, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(hipMemsetAsync(d_US, 0xFF, (u64)span * 4, st));       // kFinNone: a place no member notes is no update
    BWTC_HIP_TRY(hipMemsetAsync(d_UR, 0xA5, (u64)span * 4, st));
    BWTC_HIP_TRY(fin_test_guard({{d_US, (u64)span * 4}, {d_UR, (u64)span * 4}}, false, &can, st));
  } else {
    BWTC_HIP_TRY(fin_test_guard({{d_hardC, (u64)m * 2}}, true, &can, st));
    BWTC_HIP_TRY(fin_test_guard(fin_spans(q.shal.S, q.shal.HP, m), true, &can, st));
  }
  fc[kFinHard] = 0; fc[kFinHardDepth] = 0xFFFFFFFFu;
  BWTC_HIP_TRY(fc.upload(kFinHard, kFinHardDepth));
  BWTC_HIP_TRY(fc.clear(kFinNext, kFinGroupsLeft));
  RrEmit re;
  BWTC_HIP_TRY(fin_test_emit_begin(*this, n, t.out_n, t.lf_n, t.lf_x, &re));
  launch_finish(*this, q, re);
  if (t.ranks) {
    blk.fin.local_upd = rg; blk.fin.local_pending = true;
    const int rcu = local_updates();
    if (rcu) return rcu;
    BWTC_HIP_TRY(fin_test_copy({{t.rank, (u64)n * 4}, {t.us, (u64)span * 4}, {t.ur, (u64)span * 4}},
                               {{d_rank, (u64)n * 4}, {d_US, (u64)span * 4}, {d_UR, (u64)span * 4}}, hipMemcpyDeviceToHost, st));
  } else {
    BWTC_HIP_TRY(hipMemcpyAsync(t.hC, d_hardC, (u64)m * 2, hipMemcpyDeviceToHost, st));
    BWTC_HIP_TRY(fin_test_copy(fin_spans(t.sS, t.sHP, m), fin_spans(q.shal.S, q.shal.HP, m), hipMemcpyDeviceToHost, st));
  }
  BWTC_HIP_TRY(fin_test_copy(fin_spans(t.hS, t.hHP, m), fin_spans(d_parkS, d_parkHP, m), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fin_test_copy(fin_spans(t.nS, t.nP, t.nH, t.nC, room), fin_spans(q.out, room), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fc.fetch(kFinNext, kFinGroupsLeft, t.next_count));
  BWTC_HIP_TRY(fc.fetch(kFinHard, kFinHardDepth, t.hard_count));
  BWTC_HIP_TRY(fc.fetch(kFinShallow, kFinShallowDepth, t.shal_count));
  BWTC_HIP_TRY(fin_test_emit_fetch(*this, n, t.SA, t.out, t.small, t.lf));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  for (u32 r = 0; r < kFinRegions; ++r) t.next_base[r] = ob.base[r];
  return can.verdict();
}

int BwtEngine::test_finisher(bwtc_hip_fin_run& t) {
  // the list's contracts are one pass's, over one region from entry 0
  const u32 ebase = 0, ecount = t.m;
  FinPassTest one;
  std::memset(&one, 0, sizeof one);
  one.n = t.n; one.nreg = 1; one.ebase = &ebase; one.ecount = &ecount; one.S = t.S; one.P = t.P; one.H = t.H; one.C = t.C;
  one.window = t.window; one.group = t.group; one.words = t.words; one.rounds = t.rounds;
  one.floor = t.floor; one.out_n = t.out_n; one.lf_n = t.lf_n; one.lf_x = t.lf_x; one.next_cap = 0xFFFFFFFFu;
  FinRegions rg; FinOut ob;
  u32 m = 0, span = 0; u64 room = 0;
  if (t.max_passes < 0 || !fin_test_list_ok(one, cap, &rg, &ob, &m, &span, &room)) return -1;
  // a later pass reads up to 16 regions, each with a last window that is not full: 16 strides (and a chunk's group) more
  room += 16ull * (u32)(t.window - t.group) + 2ull * (u32)t.group;
  if (room + 128u > fin_list_cap(cap)) return -1;
  hipStream_t st = stream;
  const u32 n = t.n;
  blk = BlockSort{};                               // a block of its own
  stats.route = 0;
  FinKnobScope knobs(*this, t.window, t.group, t.words, t.rounds, t.floor);
  FinWork w;
  BWTC_HIP_TRY(finisher_begin(d_V0, m, &w));
  const FinCounters fc(*this);
  const FinShallow shal = fc.shallow_sink(d_V1, static_cast<u64*>(d_R2), fin_floor);
  TestCanaries can;
  // both lists take a pass's output in turn: never more than the first pass's room, the longest list's
  BWTC_HIP_TRY(fin_test_guard(fin_spans(w.a, room), true, &can, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(w.b, room), true, &can, st));
  BWTC_HIP_TRY(fin_test_copy(fin_spans(w.a, m), fin_spans(t.S, t.P, t.H, t.C, m), hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(d_parkS, d_parkHP, m), true, &can, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(shal.S, shal.HP, m), true, &can, st));
  BWTC_HIP_TRY(fin_test_guard(fin_spans(local_list(0), m), true, &can, st));   // (d_hardC: the passes' dead output, then the local list's characters)
  RrEmit re;
  BWTC_HIP_TRY(fin_test_emit_begin(*this, n, t.out_n, t.lf_n, t.lf_x, &re));
  FinOutcome fo;
  const int rc = finisher_passes(w, FinRequest{n, re, shal, t.keep_local != 0, t.max_passes}, &fo);
  if (rc) return rc;
  BWTC_HIP_TRY(fc.fetch(kFinWaitDepth, kFinShallowDepth));
  BWTC_HIP_TRY(wait());
  if (blk.fin.parked > m || fc[kFinShallow] > m || fo.local > m) return -3;
  t.outcome[0] = fo.hard; t.outcome[1] = fo.hard_depth; t.outcome[2] = fo.left; t.outcome[3] = fo.local;
  t.info[0] = (u32)blk.fin.passes_done; t.info[1] = stats.route; t.info[2] = blk.fin.parked; t.info[3] = blk.fin.park_holes;
  t.info[4] = fc[kFinShallow]; t.info[5] = fc[kFinShallowDepth]; t.info[6] = fc[kFinWaitDepth]; t.info[7] = fo.local ? blk.fin.local_depth : 0u;
  BWTC_HIP_TRY(fin_test_copy(fin_spans(t.pS, t.pHP, blk.fin.parked), fin_spans(d_parkS, d_parkHP, blk.fin.parked), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fin_test_copy(fin_spans(t.sS, t.sHP, t.info[4]), fin_spans(shal.S, shal.HP, t.info[4]), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fin_test_copy(fin_spans(t.lS, t.lP, t.lH, t.lC, fo.local), fin_spans(local_list(0), fo.local), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fin_test_emit_fetch(*this, n, t.SA, t.out, t.small, t.lf));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

// A raw list becomes a list the rounds understand: sorted by slot (groups contiguous, a positional slot
// array), key = head slot | character << 56, value = suffix.  S / HP must be one of (d_V0 | d_V1) and one
// of (d_R1 | d_R2), between which the sort by slot runs; d_W0 / d_W1 and d_G0 receive the list, and L.home says so:
// keys in W0 with R1 free, the values where the sort left them, slots in G0.  Of L.res only m and groups are the new
// list's; carry stays (the keys made here hold the character, and so did the keys of every list the finisher route had).
int BwtEngine::dress_list(SortList& L, u32 total, u32* S, u64* HP, u32 holes) {
  hipStream_t st = stream;
  const u32 n = L.n;
  u64* hp_other = HP == static_cast<u64*>(d_R1) ? static_cast<u64*>(d_R2) : static_cast<u64*>(d_R1);
  u32* s_other = S == d_V0 ? d_V1 : d_V0;
  u64* hp_sorted = nullptr; u32* s_sorted = nullptr;
  sort_pairs<u64>(HP, hp_other, S, s_other, total, bit_width_u64(n ? n - 1 : 0), &hp_sorted, &s_sorted, false);
  u64* fkey = reinterpret_cast<u64*>(d_W0);              // d_W0 and d_W1 are neighbours in the arena: 8 * cap bytes
  total -= holes;                                        // (entries that left for the shallow list: all ones, sorted to the end)
  hipLaunchKernelGGL(k_bridge_dress, dim3(ceil_div(total, 256)), dim3(256), 0, st, (const u64*)hp_sorted, (const u32*)s_sorted,
                     total, (const u8*)d_T, fkey, d_G0);
  L.res.m = total; L.res.groups = 0;
  L.home = ListHome::sorted(fkey, d_R1, d_V0, d_V1, d_G0, d_G1, fkey, s_sorted);
  return 0;
}

// rank[] for everybody, late: rank[SA[slot]] = slot for the finished suffixes, any rank for the list's
// (the ranking step that follows writes theirs).  pairs / tmp: two free 8 * cap-byte regions.
void BwtEngine::complete_ranks(u32 n, const u32* list_sfx, const u32* list_slot, u32 m, void* pairs_region, void* tmp_region) {
  hipStream_t st = stream;
  u32* pairs = static_cast<u32*>(pairs_region);
  hipLaunchKernelGGL(k_bridge_pairs_all, dim3(ceil_div(n, 1024)), dim3(256), 0, st, (const u32*)d_SA, n, pairs, pairs + cap);
  if (m) hipLaunchKernelGGL(k_bridge_pairs_fix, dim3(ceil_div(m, 256)), dim3(256), 0, st, list_sfx, list_slot, m, pairs, pairs + cap);
  for (u32 r = 0; blk.fin.local_m && r < blk.fin.local_rg.nreg; ++r) {
    if (!blk.fin.local_rg.ecount[r]) continue;
    hipLaunchKernelGGL(k_bridge_pairs_fix_list, dim3(ceil_div(blk.fin.local_rg.ecount[r], 256)), dim3(256), 0, st,
                       fin_part(local_list(blk.fin.local_home), blk.fin.local_rg.ebase[r]), blk.fin.local_rg.ecount[r], pairs, pairs + cap);
  }
  if (blk.fin.parked) hipLaunchKernelGGL(k_bridge_pairs_fix_parked, dim3(ceil_div(blk.fin.parked, 256)), dim3(256), 0, st, (const u32*)d_parkS, (const u64*)d_parkHP, blk.fin.parked, pairs, pairs + cap);
  scatter_rank_pairs(pairs, static_cast<u32*>(tmp_region), n, n);
}

// Loads `ncopy` bytes of d_src into d_T (reversed or not), zero-fills up to n + padding and
// returns the histogram of T[0..n-1] (the implicit zeros included) in hist_T.
int BwtEngine::load_text(const u8* d_src, u32 ncopy, u32 n, bool reverse, u32* hist_T) {
  hipStream_t st = stream;
  BWTC_HIP_TRY(hipMemsetAsync(d_small, 0, 1024 * 4, st));
  stats.alg_bytes = 2ull * n;                            // k_load_hist: the block read, T written
  const u32 padded = (u32)((((u64)n + kTextPad + 15) / 16) * 16);
  const int aligned = (reinterpret_cast<uintptr_t>(d_src) & 15u) == 0;
  hipLaunchKernelGGL(k_load_hist, dim3(std::min<u32>(ceil_div(padded, kLoadTile), 2048u)), dim3(kLoadTPB), 0, st, d_src,
                     d_T, ncopy, padded, reverse ? 1 : 0, aligned, d_small + kSmallFreqs);
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallFreqs, d_small + kSmallFreqs, 256 * 4,
                              hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(wait());
  for (int c = 0; c < 256; ++c) hist_T[c] = h_small[kSmallFreqs + c];
  hist_T[0] += n - ncopy;
  return 0;
}

int BwtEngine::transform(const u8* d_src, u8* d_dst, u32 size, bool raw, u32* lf, u32 n_lf,
                         u32* freqs) {
  BwtEngine::ScanScope scan_scope(*this);
  hipStream_t st = stream;
  // block mode: size source bytes, n = size + 1 suffixes.  raw mode: `size` is the length
  // of T including the caller's sentinel, so the source bytes that count are size - 1.
  const u32 n = raw ? size : size + 1u;
  const u32 nsrc = n - 1u;
  if (n_lf == 0 || n_lf > 256 || !lf) return -1;
  if ((u64)n > cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(device));
  BWTC_HIP_TRY(hipEventRecord(ev_begin, st));
  wait_seq = 0;                                          // the block's waits come in the same order for every block of a stream
  u32 hist_T[256];
  int rc = load_text(d_src, nsrc, n, !raw, hist_T);
  if (rc) return rc;
  if (freqs) for (int c = 0; c < 256; ++c) freqs[c] += h_small[kSmallFreqs + c];
  // Blocks up to 256 MiB: the transform's bytes are written by the ranking kernels, straight
  // into the caller's buffer (d_src was consumed by load_text, so d_dst may alias it).
  // Larger blocks (a round's key then needs the character's bits): suffix array + gather.
  // The transform's bytes leave from the ranking kernels (a list whose keys have no room for the carried
  // character -- more than 56 bits, only possible above 256 MiB -- reads T[s-1] for what it finishes).
  const EmitTarget em{d_dst, raw ? n : size, n_lf};
  rc = suffix_sort(n, hist_T, h_small[kSmallFreqs] == 0, no_emit ? nullptr : &em);
  if (rc) return rc;
  if (!no_emit) {
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, st, d_dst, d_T, d_rank,
                       d_small + kSmallLf, n_lf, n, d_small + kSmallPidx, raw ? 1 : 0,
                       d_small + kSmallLastChar, blk.lf_noted ? 1 : 0);
  } else {
    hipLaunchKernelGGL(k_bwt_gather, dim3(ceil_div(ceil_div(n, 4), 256)), dim3(256), 0, st, d_SA,
                       d_T, d_out, n, d_small + kSmallPidx);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, st, d_out, d_T, d_rank,
                       d_small + kSmallLf, n_lf, n, d_small + kSmallPidx, raw ? 1 : 0,
                       (const u32*)nullptr);
    if (raw ? n : size)
      BWTC_HIP_TRY(hipMemcpyAsync(d_dst, d_out, raw ? n : size, hipMemcpyDeviceToDevice, st));
  }
  BWTC_HIP_TRY(hipMemcpyAsync(h_small + kSmallLf, d_small + kSmallLf, 264 * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipEventRecord(ev_end, st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  BWTC_HIP_TRY(take_sticky_error());
  if (radix_fault_take()) { std::fprintf(stderr, "bwtc_hip: a radix pass's digit table and its items disagreed (checked build)\n"); return -3; }
  for (u32 k = 0; k < n_lf; ++k) lf[k] = h_small[kSmallLf + k];
  probe.harvest();
  stats.n = n;
  BWTC_HIP_TRY(hipEventElapsedTime(&stats.ms_total, ev_begin, ev_end));
  stats.ms_sort = 0.f;
  for (int i = 0; i + 1 < n_sort_events; i += 2) {
    float ms = 0.f;
    BWTC_HIP_TRY(hipEventElapsedTime(&ms, ev_sort[i], ev_sort[i + 1]));
    stats.ms_sort += ms;
  }
  return 0;
}

// ---- test hooks: the ranking step and the rounds' kernels ("The ranking hooks") -----------------------
// What the ranking kernels assume of their list, checked on the host.  Of these only m <= n, the suffixes and slots below n
// and m == n with INIT keep the stores inside their arrays; the others (distinct suffixes, ascending slots, the forms
// rank_step pairs, the long items' fields) are what an honest list satisfies and what the model is defined for.
static bool rank_test_pass_ok(const bwtc_hip_rank_pass& t, u64 cap) {
  const u32 m = t.m, n = t.n;
  if (m < 1u || m > n || (u64)n + TestCanaries::kBytes > cap) return false;
  if (!t.keys || !t.idx) return false;
  if (t.key_bytes != 4 && t.key_bytes != 8) return false;
  if (t.init ? m != n : t.key_bytes != 8) return false;
  if ((t.split || t.lng) && !(t.init && t.key_bytes == 8)) return false;
  if (t.mode < 0 || t.mode > 3 || t.emit < 0 || t.emit > 3) return false;
  if (!rr_emit_legal(t.split != 0, t.lng != 0, t.init != 0, t.emit)) return false;   // (t.emit is the form, as RrForm::emit takes it)
  if (t.split && n > (1u << 29)) return false;
  if (t.lng) {
    if (!t.w || t.wmask == 0u || t.hi_shift < 0 || t.chr_shift < 0 || t.chr_shift > 63 || t.chr_mask > 255u) return false;
    if (t.hi_shift > (t.split ? 51 : 63) || t.lvl_shift < -1 || t.lvl_shift > 61 || t.depth >= (1u << 24)) return false;
  }
  if (t.emit == 3 && !t.inv_lut) return false;
  if (t.out_n != n && t.out_n + 1u != n) return false;
  if (t.lf_n > 256u || (t.lf_n > 1u && (t.lf_x != n / t.lf_n || t.lf_x < 1u))) return false;
  if (t.rec_shift < 0 || t.rec_shift > 31) return false;
  std::vector<u8> seen(n, 0);
  for (u32 p = 0; p < m; ++p) {
    u32 s;
    if (t.split) {
      const u64 k = static_cast<const u64*>(t.keys)[p];
      const u32 hi = t.lng ? ((u32)(k >> t.hi_shift) & 0x1FFFu) : (u32)(k >> 48);
      if (hi >= (1u << 13)) return false;
      s = (hi << 16) | static_cast<const unsigned short*>(t.idx)[p];
    } else s = static_cast<const u32*>(t.idx)[p];
    if (s >= n || seen[s]) return false;
    seen[s] = 1;
  }
  if (!t.init) {
    if (!t.aglob) return false;
    for (u32 p = 0; p < m; ++p) if (t.aglob[p] >= n || (p > 0 && t.aglob[p] <= t.aglob[p - 1])) return false;
  }
  return true;
}

int BwtEngine::test_rank_pass(bwtc_hip_rank_pass& t) {
  if (!rank_test_pass_ok(t, cap)) return -1;
  hipStream_t st = stream;
  const u32 m = t.m, n = t.n, tiles = ceil_div(m, kRrTile);
  const bool wide = t.key_bytes == 8, mode3 = t.mode == 3;
  // the list where suffix_sort's stages leave it (keys in R1, values in V0, second words in W0, slots in G0); what apply
  // writes where rank_step points it: the next list in V1 / G1 / GRP / C0, pairs or records in R2, the records' values in
  // the free value array, their plane in P0
  u32* pairs = static_cast<u32*>(d_R2);
  u32* pair_s = t.mode == 1 || t.mode == 2 ? pairs : nullptr;
  u32* pair_r = t.mode == 1 ? pairs + cap : t.mode == 2 ? d_V1 : nullptr;
  const u64 idx_bytes = t.split ? ((u64)m * 2 + 3) / 4 * 4 : (u64)m * 4;
  const u64 achr_bytes = mode3 ? (u64)m * 2 : (u64)m;
  TestCanaries can;
  BWTC_HIP_TRY(hipMemcpyAsync(d_R1, t.keys, (u64)m * (wide ? 8 : 4), hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemsetAsync(d_V0, 0, idx_bytes, st));
  BWTC_HIP_TRY(hipMemcpyAsync(d_V0, t.idx, (u64)m * (t.split ? 2 : 4), hipMemcpyHostToDevice, st));
  if (t.lng) BWTC_HIP_TRY(hipMemcpyAsync(d_W0, t.w, (u64)m * 4, hipMemcpyHostToDevice, st));
  if (!t.init) BWTC_HIP_TRY(hipMemcpyAsync(d_G0, t.aglob, (u64)m * 4, hipMemcpyHostToDevice, st));
  if (t.emit == 3) BWTC_HIP_TRY(hipMemcpyAsync(d_small + kSmallInv, t.inv_lut, 256, hipMemcpyHostToDevice, st));
  u32* const out4[] = {d_V1, d_G1, d_GRP};
  for (u32* a : out4) { BWTC_HIP_TRY(hipMemsetAsync(a, 0xA5, (u64)m * 4, st)); BWTC_HIP_TRY(can.put(a, (u64)m * 4, st)); }
  BWTC_HIP_TRY(hipMemsetAsync(d_C0, 0xA5, (u64)m * 2, st)); BWTC_HIP_TRY(can.put(d_C0, achr_bytes, st));
  BWTC_HIP_TRY(hipMemsetAsync(pairs, 0xA5, (u64)m * 8, st)); BWTC_HIP_TRY(can.put(pairs, (u64)m * (t.mode == 2 ? 8 : 4), st));
  BWTC_HIP_TRY(hipMemsetAsync(pairs + cap, 0xA5, (u64)m * 4, st)); BWTC_HIP_TRY(can.put(pairs + cap, (u64)m * 4, st));
  BWTC_HIP_TRY(hipMemsetAsync(d_P0, 0xA5, m, st)); BWTC_HIP_TRY(can.put(d_P0, m, st));
  BWTC_HIP_TRY(hipMemsetAsync(d_rank, 0xA5, (u64)n * 4, st)); BWTC_HIP_TRY(can.put(d_rank, (u64)n * 4, st));
  u32* const agg[] = {d_aggA, d_aggB, d_aggC};
  for (u32* a : agg) { BWTC_HIP_TRY(hipMemsetAsync(a, 0xA5, (u64)tiles * 4, st)); BWTC_HIP_TRY(can.put(a, (u64)tiles * 4, st)); }
  BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallCounts, 0xA5, 8, st));
  RrEmit re;
  BWTC_HIP_TRY(fin_test_emit_begin(*this, n, t.out_n, t.lf_n, t.lf_x, &re));
  BWTC_HIP_TRY(can.put(d_SA, (u64)n * 4, st)); BWTC_HIP_TRY(can.put(d_out, n, st));
  re.achr_out = d_C0;
  re.inv_lut = reinterpret_cast<const u8*>(d_small + kSmallInv);
  re.rec_plane = t.mode == 2 && t.plane ? d_P0 : nullptr;
  re.rec_shift = t.rec_shift;
  const RrLong lg = t.lng ? RrLong{d_W0, t.wmask, t.hi_shift, t.chr_shift, t.chr_mask, t.lvl_shift, t.depth} : RrLong();
  const RrForm form{t.split != 0, t.lng != 0, t.mode, t.emit};
  const RrOut o{d_rank, d_SA, t.mode == 2 ? nullptr : d_V1, d_G1, d_GRP, pair_s, pair_r};
  const u32* aglob = t.init ? nullptr : d_G0;
  if (!wide) launch_rerank<u32, true>(*this, kRrReduceScan | kRrApply, form, static_cast<const u32*>(d_R1), d_V0, aglob, m, n, t.short_len, (u32)t.kmask, lg, o, re);
  else if (t.init) launch_rerank<u64, true>(*this, kRrReduceScan | kRrApply, form, static_cast<const u64*>(d_R1), d_V0, aglob, m, n, t.short_len, (u64)t.kmask, lg, o, re);
  else launch_rerank<u64, false>(*this, kRrReduceScan | kRrApply, form, static_cast<const u64*>(d_R1), d_V0, aglob, m, n, t.short_len, (u64)t.kmask, lg, o, re);
  BWTC_HIP_TRY(hipMemcpyAsync(t.aggA, d_aggA, (u64)tiles * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.aggB, d_aggB, (u64)tiles * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.aggC, d_aggC, (u64)tiles * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.counts, d_small + kSmallCounts, 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.rank, d_rank, (u64)n * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.pair_s, pairs, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.pair_r, pairs + cap, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.rec, pairs, (u64)m * 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.val, d_V1, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.rplane, d_P0, m, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.aidx, d_V1, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.aglob_out, d_G1, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.agrp, d_GRP, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.achr, d_C0, (u64)m * 2, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fin_test_emit_fetch(*this, n, t.SA, t.out, t.small, t.lf));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

int BwtEngine::test_rank_scan(u32* a, u32* b, u32* c, u32 ntiles, u32* parts_out, u32 parts_cap, u32* counts_out) {
  const u64 rr_tiles = (cap + kRrTile - 1) / kRrTile + 1;                 // what init reserved (plan_arena)
  const u64 part_words = (rr_tiles / 4096 + 2) * 3;
  if (ntiles < 1u || (u64)ntiles > rr_tiles || parts_cap > part_words) return -1;   // (the canaries lie in the arrays' 64 spare words)
  if ((u64)ceil_div(ntiles, kRrScanChunk) * 3 > part_words) return -1;
  hipStream_t st = stream;
  TestCanaries can;
  u32* const dev[] = {d_aggA, d_aggB, d_aggC};
  u32* const host[] = {a, b, c};
  for (int i = 0; i < 3; ++i) {
    BWTC_HIP_TRY(hipMemcpyAsync(dev[i], host[i], (u64)ntiles * 4, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(can.put(dev[i], (u64)ntiles * 4, st));
  }
  BWTC_HIP_TRY(hipMemsetAsync(d_agg_part, 0xA5, part_words * 4, st));     // (d_small lies behind it: no room for a canary, the poison is returned)
  BWTC_HIP_TRY(hipMemsetAsync(d_small + kSmallCounts, 0xA5, 8, st));
  launch_rerank_scan(*this, ntiles);
  for (int i = 0; i < 3; ++i) BWTC_HIP_TRY(hipMemcpyAsync(host[i], dev[i], (u64)ntiles * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(parts_out, d_agg_part, (u64)parts_cap * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(counts_out, d_small + kSmallCounts, 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

int BwtEngine::test_rank_scatter(bool dense, const u32* where, const u32* what, const u64* rec, u32 m, u32 n, int bin_shift, u32* rank) {
  if (m < 1u || m > n || (u64)n + TestCanaries::kBytes > cap || bin_shift < 0 || bin_shift > 24 || !rank) return -1;
  if (dense ? !rec : (!where || !what)) return -1;
  {
    std::vector<u8> seen(n, 0);
    for (u32 i = 0; i < m; ++i) {
      const u32 s = dense ? (u32)(rec[i] >> 32) : where[i];
      if (s >= n || seen[s]) return -1;
      seen[s] = 1;
    }
  }
  hipStream_t st = stream;
  u32* pairs = static_cast<u32*>(d_R2);                  // where rank_step keeps its pairs and records
  TestCanaries can;
  if (dense) BWTC_HIP_TRY(hipMemcpyAsync(pairs, rec, (u64)m * 8, hipMemcpyHostToDevice, st));
  else {
    BWTC_HIP_TRY(hipMemcpyAsync(pairs, where, (u64)m * 4, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(hipMemcpyAsync(pairs + cap, what, (u64)m * 4, hipMemcpyHostToDevice, st));
  }
  BWTC_HIP_TRY(hipMemcpyAsync(d_rank, rank, (u64)n * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(can.put(d_rank, (u64)n * 4, st));
  if (dense) launch_scatter_dense(*this, static_cast<const u64*>(d_R2), m, bin_shift);
  else launch_scatter_pairs(*this, pairs, pairs + cap, m, bin_shift);
  BWTC_HIP_TRY(hipMemcpyAsync(rank, d_rank, (u64)n * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

int BwtEngine::test_round_keys(bwtc_hip_round_keys& t) {
  const u32 m = t.m, n = t.n;
  if (m < 1u || m > n || (u64)n + TestCanaries::kBytes > cap || t.kind < 0 || t.kind > 2 || !t.keys) return -1;
  if (t.run_mode < 0 || t.run_mode > 2) return -1;
  const bool dense = t.kind == 2, text = t.kind == 1;
  if (dense ? (!t.rec || !t.val || !t.rank || t.bin_shift < 0 || t.bin_shift > 24) : (!t.aidx || !t.agrp)) return -1;
  if (text && t.rank) return -1;
  if (t.kind == 0 && !t.rank && t.run_mode != 1) return -1;             // (rank_step makes keys without rank[] in the run step alone)
  const bool chr = dense ? t.emit != 0 : t.achr != nullptr;
  const int room = chr ? 56 : 64;
  int gshift;
  if (text) {
    if (t.bc < 1 || t.bc > 6 || t.run_mode == 1 || (t.run_mode == 2 && t.h_split > t.h)) return -1;
    gshift = 8 * t.bc + 4;
  } else {
    if (t.bc < 1 || t.bc > 33 || ((u64)n >> (t.run_mode == 1 ? t.bc - 1 : t.bc)) != 0) return -1;
    gshift = t.bc;
  }
  if (t.run_mode != 0) {
    if (!t.k || t.p < 1u || (t.run_mode == 1 && t.p > t.h)) return -1;
    for (u32 s = 0; s < n; ++s) if (t.k[s] > n - s) return -1;
  }
  if (t.rank) for (u32 s = 0; s < n; ++s) if (t.rank[s] >= n) return -1;
  for (u32 i = 0; i < m; ++i) {
    const u32 s = dense ? (u32)(t.rec[i] >> 32) : t.aidx[i];
    const u32 g = dense ? t.val[i] : t.agrp[i];
    if (s >= n) return -1;
    if (dense && g == 0xFFFFFFFFu) continue;
    if (gshift < 64 && ((u64)g >> (room - gshift)) != 0) return -1;
  }
  hipStream_t st = stream;
  TestCanaries can;
  u64* keys = static_cast<u64*>(d_R2);                   // rank_step's recA
  const RunKeys rk{d_runK, t.h_split, t.run_mode, t.p};
  if (t.run_mode) BWTC_HIP_TRY(hipMemcpyAsync(d_runK, t.k, (u64)n * 4, hipMemcpyHostToDevice, st));
  if (t.rank) BWTC_HIP_TRY(hipMemcpyAsync(d_rank, t.rank, (u64)n * 4, hipMemcpyHostToDevice, st));
  if (dense) {
    BWTC_HIP_TRY(hipMemcpyAsync(keys, t.rec, (u64)m * 8, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(hipMemcpyAsync(d_V1, t.val, (u64)m * 4, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(can.put(keys, (u64)m * 8, st)); BWTC_HIP_TRY(can.put(d_V1, (u64)m * 4, st));
    launch_gather_dense(*this, keys, d_V1, m, n, t.h, t.bc, t.emit ? 1 : 0, t.bin_shift, rk);
    BWTC_HIP_TRY(hipMemcpyAsync(t.val, d_V1, (u64)m * 4, hipMemcpyDeviceToHost, st));
  } else {
    BWTC_HIP_TRY(hipMemcpyAsync(d_V1, t.aidx, (u64)m * 4, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(hipMemcpyAsync(d_GRP, t.agrp, (u64)m * 4, hipMemcpyHostToDevice, st));
    if (t.achr) BWTC_HIP_TRY(hipMemcpyAsync(d_C0, t.achr, m, hipMemcpyHostToDevice, st));
    BWTC_HIP_TRY(hipMemsetAsync(keys, 0xA5, (u64)m * 8, st));
    BWTC_HIP_TRY(can.put(keys, (u64)m * 8, st));
    if (text) launch_gather_text(*this, d_V1, d_GRP, t.achr ? d_C0 : nullptr, keys, m, n, t.h, (u32)t.bc, rk);
    else launch_gather_key2(*this, d_V1, d_GRP, t.rank ? d_rank : nullptr, t.achr ? d_C0 : nullptr, keys, m, n, t.h, t.bc, rk);
  }
  BWTC_HIP_TRY(hipMemcpyAsync(t.keys, keys, (u64)m * 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

// The driver: rank_step<u64, false> once.  pairs_min and window_bits are the call's and are put back; the block state is
// a new one in the finisher route with rank[] live (finished suffixes also go to SA, text rounds keep rank[] exact).
struct RoundKnobScope {
  BwtEngine& e;
  const u32 pairs_min; const int window_bits;
  RoundKnobScope(BwtEngine& eng, u32 pm, int wb) : e(eng), pairs_min(eng.pairs_min), window_bits(eng.window_bits) { e.pairs_min = pm; e.window_bits = wb; }
  ~RoundKnobScope() { e.pairs_min = pairs_min; e.window_bits = window_bits; }
};

int BwtEngine::test_round(bwtc_hip_round& t) {
  const u32 m = t.m, n = t.n;
  if (m < 1u || m > n || (u64)n + TestCanaries::kBytes > cap || !t.ks || !t.vs || !t.aglob || !t.rank) return -1;
  if (t.h_next < 1u || t.pairs_min < 1u || t.window_bits < 1 || t.window_bits > 32 || (t.raw_out && !t.text)) return -1;
  if (t.run_mode < 0 || t.run_mode > 2 || (t.text && t.h_next >= (1ull << 31))) return -1;
  if (t.out_n != n && t.out_n + 1u != n) return -1;
  if (t.lf_n > 256u || (t.lf_n > 1u && (t.lf_x != n / t.lf_n || t.lf_x < 1u))) return -1;
  if (t.run_mode != 0) {
    if (!t.k || t.step_p < 1u || (t.run_mode == 1 && (u64)t.step_p > t.h_next) || (t.run_mode == 2 && t.text && (u64)t.step_depth > t.h_next)) return -1;
    for (u32 s = 0; s < n; ++s) if (t.k[s] > n - s) return -1;
  }
  {
    std::vector<u8> seen(n, 0);
    for (u32 p = 0; p < m; ++p) {
      const u32 s = t.vs[p];
      if (s >= n || seen[s] || t.aglob[p] >= n || (p > 0 && t.aglob[p] <= t.aglob[p - 1])) return -1;
      seen[s] = 1;
    }
    for (u32 s = 0; s < n; ++s) if (t.rank[s] >= n) return -1;
  }
  hipStream_t st = stream;
  RoundKnobScope knobs(*this, t.pairs_min, t.window_bits);
  blk = BlockSort{};
  blk.fin_active = true; blk.ranks_live = true;
  blk.set_step(StretchStep{t.run_mode ? t.step_p : 0u, StretchStep::kNone, t.run_mode == 2 ? t.step_depth : 0u});
  n_sort_events = 0;
  TestCanaries can;
  BWTC_HIP_TRY(hipMemcpyAsync(d_R1, t.ks, (u64)m * 8, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(d_V0, t.vs, (u64)m * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(d_G0, t.aglob, (u64)m * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(d_rank, t.rank, (u64)n * 4, hipMemcpyHostToDevice, st));
  if (t.run_mode) BWTC_HIP_TRY(hipMemcpyAsync(d_runK, t.k, (u64)n * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(can.put(d_rank, (u64)n * 4, st));
  u32* const out4[] = {d_G1, d_GRP};
  for (u32* a : out4) { BWTC_HIP_TRY(hipMemsetAsync(a, 0xA5, (u64)m * 4, st)); BWTC_HIP_TRY(can.put(a, (u64)m * 4, st)); }
  BWTC_HIP_TRY(hipMemsetAsync(d_C0, 0xA5, (u64)m * 2, st)); BWTC_HIP_TRY(can.put(d_C0, t.raw_out ? (u64)m * 2 : (u64)m, st));
  BWTC_HIP_TRY(hipMemsetAsync(d_V1, 0xA5, (u64)m * 4, st));
  RrEmit re;
  BWTC_HIP_TRY(fin_test_emit_begin(*this, n, t.out_n, t.lf_n, t.lf_x, &re));
  BWTC_HIP_TRY(can.put(d_SA, (u64)n * 4, st)); BWTC_HIP_TRY(can.put(d_out, n, st));
  re.achr_out = d_C0;
  SortList L{n, t.emit != 0, ListHome::at(d_R1, d_R2, d_V0, d_V1, d_G0, d_G1), re, RankResult{}, d_C1, true};
  L.res.carry = t.carry_in != 0;                         // what the step before reported of this list's keys
  RankRequest rq;
  rq.m = m; rq.h_next = t.h_next; rq.run_mode = t.run_mode;
  rq.kind = t.raw_out ? RoundKind::kRaw : t.text ? RoundKind::kText : RoundKind::kOrdinary;
  const int rc = rank_step<u64, false>(L, rq);
  if (rc) return rc;
  const RankResult& res = L.res;
  t.result[0] = res.m; t.result[1] = res.groups; t.result[2] = res.carry ? 1u : 0u; t.result[3] = res.text_chars;
  t.result[4] = res.ran_run ? 1u : 0u; t.result[5] = res.finish ? 1u : 0u;
  if (t.raw_out) BWTC_HIP_TRY(hipMemcpyAsync(t.nvs, d_V1, (u64)m * 4, hipMemcpyDeviceToHost, st));
  else if (res.m > 0) {
    BWTC_HIP_TRY(hipMemcpyAsync(t.nks, L.home.keys, (u64)res.m * 8, hipMemcpyDeviceToHost, st));
    BWTC_HIP_TRY(hipMemcpyAsync(t.nvs, L.home.vals, (u64)res.m * 4, hipMemcpyDeviceToHost, st));
  }
  BWTC_HIP_TRY(hipMemcpyAsync(t.naglob, d_G1, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.ngrp, d_GRP, (u64)m * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.nchr, d_C0, (u64)m * 2, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(t.rank, d_rank, (u64)n * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(fin_test_emit_fetch(*this, n, t.SA, t.out, t.small, t.lf));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

// Test hook (bwtc_hip_test_copy_lengths): copy_lengths over a given list and rank[]; no text is read.
int BwtEngine::test_copy_lengths(const u32* suf, const u32* grp, u32 m, const u32* rank, u32 n, u32* k_out, u32* longest_out) {
  if (m < 1u || n < 1u || m > n || n > max_block || (u64)n + TestCanaries::kBytes > cap || !suf || !grp || !rank || !k_out || !longest_out) return -1;
  u32 groups = 0;
  std::vector<u8> seen(n, 0);
  for (u32 i = 0; i < m; ++i) {                          // dense group numbers in list order, as the ranking's apply kernel leaves them
    if (suf[i] >= n || seen[suf[i]]) return -1;
    seen[suf[i]] = 1;
    if (i == 0 ? grp[i] != 0u : (grp[i] != grp[i - 1] && grp[i] != grp[i - 1] + 1u)) return -1;
    groups = grp[i] + 1u;
  }
  hipStream_t st = stream;
  blk = BlockSort{};
  TestCanaries can;
  BWTC_HIP_TRY(hipMemcpyAsync(d_V0, suf, (u64)m * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(d_GRP, grp, (u64)m * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(d_rank, rank, (u64)n * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemsetAsync(d_runK, 0xA5, (u64)n * 4, st));
  BWTC_HIP_TRY(can.put(d_runK, (u64)n * 4, st));
  BWTC_HIP_TRY(can.put(d_parkS, n, st));
  BWTC_HIP_TRY(can.put(d_LP0, groups, st));
  const int rc = copy_lengths(d_V0, d_GRP, m, groups, n, longest_out);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(k_out, d_runK, (u64)n * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

}  // namespace bwtc_hip
