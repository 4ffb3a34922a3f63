// Decoder of the 'H' coder's BWT-block records (HuffmanDecoder::decodeBlock,
// HuffmanCoders.cpp:324-616) on the GPU.
//
// A section's Huffman stream and gamma stream carry no length fields and nothing marks where a
// code starts, but the run count of the section and the longest code M of each stream are known
// before the stream is read.  So a stream is cut into tiles of kTileBits bits and every tile gets
// a transition map, exact for every code (no self-synchronisation is assumed): a code that crosses
// into a tile enters it at one of its first M bits, and for each entry e < M one lane decodes to
// the tile's end and records (exit offset into the next tile, codes decoded, error).  Maps compose
// (h[e] = g[f[e]], counts added), 64 at a time in LDS, up to one map; the walk back down gives every
// tile its true entry and its code base, and a last pass decodes each tile once from that entry and
// writes the run symbols / run lengths at their bases.  A section's two streams are one chain on
// the device (the gamma stream starts where the Huffman stream ended, read from a device word);
// the host reads the gamma stream's end back and parses the next section's code shape there.
//
// After all sections: an exclusive scan of the run lengths (scan.hpp) gives every run its offset
// in the block, and one pass expands the runs into the BWT bytes with vector stores.
//
// Every loop is bounded by the tile, the window (a stream cannot be longer than its run count
// times its longest code) and the record; a bit pattern that is no code, a stream that leaves the
// record and run lengths that do not add up come back as error codes, never as a fault.
#include "bwt_engine.hpp"
#include "huffman_decoder.hpp"
#include "scan.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace bwtc_hip {

namespace {

constexpr u32 kTileBits = 512;          // bits per tile (>= 64 >= any M)
constexpr u32 kFastBits = 12;           // first-level Huffman table
constexpr u32 kMapTPB = 256;
constexpr u32 kDecTPB = 256;
constexpr u32 kExpandBytes = 32;        // output bytes per thread of the expansion
constexpr u64 kNoEnd = 1ull << 62;      // end word before a stream's end is found

// map word: exit offset (7 bits) | error (2 bits) << 7 | codes decoded << 9 (64 bits: a map high up the
// tree covers 2^30 tiles and more codes than 32 bits hold)
constexpr u32 kErrCode = 1, kErrPast = 2;
__host__ __device__ inline u64 map_pack(u32 exit, u32 err, u64 cnt) { return exit | (err << 7) | (cnt << 9); }

// device tables of one section's Huffman code (canonical codes of computeHuffmanCodes,
// Utils.cpp:180-202: the longest codes start at 0, a length's codes ascend with the symbol)
struct alignas(16) HTable {
  uint16_t fast[1u << kFastBits];       // sym << 4 | len for codes <= 12 bits, 0 = longer code, 0xFFFF = no code
  u64 first[65];
  u32 count[65];
  u32 offset[65];
  u8 syms[256];
  u32 max_len;
};

// per-section words the host reads back
struct SecResult {
  u64 hend;                             // bit after the last Huffman code (kNoEnd: not found)
  u64 gend;                             // bit after the last gamma code
  u64 sum;                              // run lengths added up
  u32 err;                              // first HDecodeError seen (0 = none)
  u32 pad;
};

__device__ __forceinline__ u64 bswap64(u64 v) { return __builtin_bswap64(v); }

// MSB-first bits of the record; the device copy is padded with zero words, so a read at any bit
// before the record's end may look 64 bits further
struct BitPeek {
  const u64* w;
  __device__ __forceinline__ u64 at(u64 pos) const {
    const u64 i = pos >> 6;
    const u32 s = (u32)(pos & 63);
    const u64 hi = bswap64(w[i]);
    if (!s) return hi;
    return (hi << s) | (bswap64(w[i + 1]) >> (64 - s));
  }
};

struct alignas(16) SmemTable {                  // load_table copies the fast table 16 bytes at a time
  uint16_t fast[1u << kFastBits];
  u64 first[65];
  u32 count[65];
  u32 offset[65];
  u8 syms[256];
};

__device__ void load_table(SmemTable& s, const HTable* t) {
  const uint4* src = reinterpret_cast<const uint4*>(t->fast);
  uint4* dst = reinterpret_cast<uint4*>(s.fast);
  for (u32 i = threadIdx.x; i < sizeof(s.fast) / 16; i += blockDim.x) dst[i] = src[i];
  for (u32 i = threadIdx.x; i < 65; i += blockDim.x) { s.first[i] = t->first[i]; s.count[i] = t->count[i]; s.offset[i] = t->offset[i]; }
  for (u32 i = threadIdx.x; i < 256; i += blockDim.x) s.syms[i] = t->syms[i];
  __syncthreads();
}

// one code at pos: its length (0 = no code) and value (symbol / run length)
template <bool GAMMA>
__device__ __forceinline__ u32 decode_one(const BitPeek& bits, u64 pos, const SmemTable* tab, u32 max_len, u64* value) {
  const u64 w = bits.at(pos);
  if (GAMMA) {
    if (w == 0) return 0;
    const u32 z = (u32)__builtin_clzll(w);
    const u32 len = 2 * z + 1;
    if (len > max_len) return 0;                   // a run longer than the section
    *value = w >> (64 - len);
    return len;
  } else {
    const u32 f = tab->fast[w >> (64 - kFastBits)];
    if (f == 0xFFFFu) return 0;
    if (f) { *value = f >> 4; return f & 15u; }
    for (u32 L = kFastBits + 1; L <= max_len; ++L) {
      const u64 v = w >> (64 - L);
      const u64 k = v - tab->first[L];
      if (v >= tab->first[L] && k < tab->count[L]) { *value = tab->syms[tab->offset[L] + (u32)k]; return L; }
    }
    return 0;
  }
}

// no gamma code could be read at pos: true when its leading one lies past the window's end (the
// device copy reads zeros there) and a code with that many zeros would still fit max_len, i.e. the
// code was cut by the end rather than being too long for the section
__device__ __forceinline__ bool gamma_cut_by_end(const BitPeek& bits, u64 pos, u64 wend, u32 max_len) {
  const u64 a = wend - pos, w = bits.at(pos);
  return (w ? (u64)__builtin_clzll(w) : 64ull) >= a && 2 * a + 1 <= max_len;
}

__device__ __forceinline__ u64 stream_start(const u64* d_start, u64 start) {
  if (!d_start) return start;
  const u64 h = *d_start;                         // the Huffman stream's end: the gamma stream starts at the next byte
  return h >= kNoEnd ? kNoEnd : (h + 7) & ~7ull;
}

// ---- maps: one lane per (tile, entry); 64 / M tiles per wave --------------------------------
// Every entry decodes its tile to the end: no merging of entries whose paths meet.
template <bool GAMMA>
__global__ __launch_bounds__(kMapTPB) void k_hd_map(const u64* __restrict__ rec, u64 rec_bits, const u64* d_start, u64 start_h,
                                                     u64 win_bits, u32 M, const HTable* __restrict__ tab, u32 ntiles,
                                                     u64* __restrict__ maps) {
  __shared__ SmemTable s;
  if (!GAMMA) load_table(s, tab);
  const u32 max_len = GAMMA ? M : tab->max_len;
  const u64 start = stream_start(d_start, start_h);
  const u64 wend = start >= rec_bits ? 0 : min(start + win_bits, rec_bits);
  const u32 tpw = kWave / M;
  const u32 lane = threadIdx.x % kWave;
  const u32 sub = lane / M, e = lane % M;
  const u64 wave = ((u64)blockIdx.x * kMapTPB + threadIdx.x) / kWave;
  const u64 tile = wave * tpw + sub;
  if (sub >= tpw || tile >= ntiles) return;
  const BitPeek bits{rec};
  const u64 t0 = start + tile * kTileBits, tend = t0 + kTileBits;
  u64 pos = t0 + e;
  u32 cnt = 0, err = 0;
  while (pos < tend) {
    if (pos >= wend) { err = kErrPast; break; }
    u64 v;
    const u32 len = decode_one<GAMMA>(bits, pos, &s, max_len, &v);
    if (!len) { err = kErrCode; break; }
    if (pos + len > wend) { err = kErrPast; break; }
    pos += len;
    ++cnt;
  }
  maps[tile * M + e] = map_pack(err ? 0u : (u32)(pos - tend), err, cnt);
}

// ---- up: out map j = in maps 64j .. 64j+63 composed, one wave per workgroup (walk in LDS) --------
__global__ __launch_bounds__(kWave) void k_hd_compose(const u64* __restrict__ in, u32 n_in, u32 M, u64* __restrict__ out, u32 n_out) {
  __shared__ u64 sm[kWave * kWave];
  const u32 lane = threadIdx.x;
  const u32 j = blockIdx.x;
  const u32 first = j * kWave, n = j < n_out ? min((u32)kWave, n_in - first) : 0u;
  u64* m = sm;
  for (u32 i = lane; i < n * M; i += kWave) m[i] = in[(u64)first * M + i];
  __syncthreads();
  if (j >= n_out || lane >= M) return;
  u32 at = lane, err = 0;
  u64 cnt = 0;
  for (u32 k = 0; k < n && !err; ++k) {
    const u64 w = m[k * M + at];
    cnt += w >> 9;
    err = (u32)(w >> 7) & 3u;
    at = (u32)w & 127u;
  }
  out[(u64)j * M + lane] = map_pack(err ? 0u : at, err, cnt);
}

// entry word of a map: code base << 16 | error << 8 | entry offset
__host__ __device__ inline u64 entry_pack(u64 base, u32 err, u32 e) { return (base << 16) | ((u64)err << 8) | e; }

// ---- down: children 64j .. 64j+63 of parent j get their entries (the parent's, walked) --------
__global__ __launch_bounds__(kWave) void k_hd_down(const u64* __restrict__ maps, u32 n_maps, u32 M, const u64* __restrict__ parent,
                                                      u64* __restrict__ entries, u32 n_groups) {
  __shared__ u64 sm[kWave * kWave];
  const u32 lane = threadIdx.x;
  const u32 j = blockIdx.x;
  const u32 first = j * kWave, n = j < n_groups ? min((u32)kWave, n_maps - first) : 0u;
  u64* m = sm;
  for (u32 i = lane; i < n * M; i += kWave) m[i] = maps[(u64)first * M + i];
  __syncthreads();
  if (j >= n_groups || lane) return;
  const u64 p = parent ? parent[j] : 0;
  u64 base = p >> 16;
  u32 err = (u32)(p >> 8) & 3u, at = (u32)p & 255u;
  for (u32 k = 0; k < n; ++k) {
    entries[first + k] = entry_pack(base, err, at);
    if (!err) {
      const u64 w = m[k * M + at];
      base += w >> 9;
      err = (u32)(w >> 7) & 3u;
      at = (u32)w & 127u;
    }
  }
}

__device__ __forceinline__ void set_error(u32* err, u32 code) { atomicCAS(err, 0u, code); }

// ---- decode: one thread per tile, from its true entry --------------------------------------------
template <bool GAMMA>
__global__ __launch_bounds__(kDecTPB) void k_hd_decode(const u64* __restrict__ rec, u64 rec_bits, const u64* d_start, u64 start_h,
                                                        u64 win_bits, u32 M, const HTable* __restrict__ tab, u32 ntiles,
                                                        const u64* __restrict__ entries, u64 n_runs, u8* __restrict__ run_sym,
                                                        u32* __restrict__ run_len, SecResult* res, u32 soft) {
  __shared__ SmemTable s;
  if (!GAMMA) load_table(s, tab);
  const u32 max_len = GAMMA ? M : tab->max_len;
  const u64 start = stream_start(d_start, start_h);
  const u32 tile = blockIdx.x * kDecTPB + threadIdx.x;
  if (tile >= ntiles || start >= rec_bits) return;
  const u64 wend = min(start + win_bits, rec_bits);
  const u64 en = entries[tile];
  u64 idx = en >> 16;
  if (((en >> 8) & 3u) || idx >= n_runs) return;   // before an earlier tile's error, or past the stream
  const BitPeek bits{rec};
  const u64 t0 = start + (u64)tile * kTileBits, tend = t0 + kTileBits;
  u64 pos = t0 + (en & 255u), sum = 0;
  while (pos < tend && idx < n_runs) {
    u64 v;
    const u32 len = pos < wend ? decode_one<GAMMA>(bits, pos, &s, max_len, &v) : 0;
    if (!len || pos + len > wend) {
      const bool past = pos >= wend || (len ? pos + len > wend : GAMMA && gamma_cut_by_end(bits, pos, wend, max_len));
      if (past && soft) return;                   // an estimated window: the host maps the stream again in full
      // a gamma stream that outruns its window inside the record holds lengths that cannot add up to S
      const bool record_end = !GAMMA || wend == rec_bits;
      set_error(&res->err, (u32)-(past ? (record_end ? kHdPastRecord : kHdRuns) : GAMMA ? kHdRuns : kHdNoCode));
      return;
    }
    if (GAMMA) { run_len[idx] = (u32)v; sum += v; }
    else run_sym[idx] = (u8)v;
    pos += len;
    ++idx;
  }
  if (GAMMA && sum) atomicAdd((unsigned long long*)&res->sum, (unsigned long long)sum);
  if (idx == n_runs) { if (GAMMA) res->gend = pos; else res->hend = pos; }
}

// ---- expansion: runs -> BWT bytes, 32 bytes per thread --------------------------------------------
__global__ __launch_bounds__(256) void k_hd_expand(const u8* __restrict__ run_sym, const u32* __restrict__ run_off, u64 n_runs,
                                                   u32 size, u8* __restrict__ out) {
  const u64 c0 = ((u64)blockIdx.x * 256 + threadIdx.x) * kExpandBytes;
  if (c0 >= size) return;
  u64 lo = 0, hi = n_runs - 1;                    // last run with off <= c0
  while (lo < hi) {
    const u64 mid = (lo + hi + 1) >> 1;
    if (run_off[mid] <= c0) lo = mid; else hi = mid - 1;
  }
  u64 r = lo;
  u32 next = r + 1 < n_runs ? run_off[r + 1] : size;
  u8 sym = run_sym[r];
  u32 w[kExpandBytes / 4];
#pragma unroll
  for (u32 i = 0; i < kExpandBytes; ++i) {
    const u64 p = c0 + i;
    while (p >= next && r + 1 < n_runs) { ++r; sym = run_sym[r]; next = r + 1 < n_runs ? run_off[r + 1] : size; }
    if ((i & 3) == 0) w[i >> 2] = 0;
    w[i >> 2] |= (u32)sym << (8 * (i & 3));
  }
  if (c0 + kExpandBytes <= size) {
    uint4* o = reinterpret_cast<uint4*>(out + c0);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  } else {
    for (u32 i = 0; c0 + i < size; ++i) out[c0 + i] = (u8)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// ---- host side ----------------------------------------------------------------------------------

// bounds-checked MSB-first reader over the host copy of the record
struct HostBits {
  const u8* p; u64 n; u64 bit = 0; bool over = false;
  u32 bitv() { if ((bit >> 3) >= n) { over = true; return 0; } const u32 b = (p[bit >> 3] >> (7 - (bit & 7))) & 1u; ++bit; return b; }
  u64 bits(u32 k) { u64 v = 0; while (k--) v = (v << 1) | bitv(); return v; }
  void flush() { bit = (bit + 7) & ~7ull; }
  u64 packed() {                                  // utils::readPackedInteger, Utils.hpp:164-178
    u64 r = 0; u32 shift = 0;
    for (;;) { const u64 b = bits(8); if (shift < 64) r |= (b & 0x7f) << shift; shift += 7; if (!(b & 0x80) || over || shift > 70) break; }
    if (shift > 70) over = true;
    return r;
  }
};

static u32 ceil_log2(u64 n) { u32 l = 0; while ((1ull << l) < n) ++l; return l; }
// utils::binaryDecode / binaryInterpolativeDecode, Utils.hpp:299-360, with the ranges checked
static bool binary_decode(HostBits& in, u64 lo, u64 hi, u64* out) {
  if (hi < lo) return false;
  const u64 range = hi - lo + 1;
  if (range == 1) { *out = lo; return true; }
  const u32 k = ceil_log2(range);
  const u64 n_short = (1ull << k) - range, n_long_left = (range - n_short) / 2;
  u64 v = in.bits(k - 1);
  if (v >= n_long_left) { *out = v + lo; }
  else { v = (v << 1) | in.bitv(); *out = v < n_long_left ? v + lo : v + lo + n_short; }
  return *out >= lo && *out <= hi && !in.over;
}
static bool interpolative_decode(HostBits& in, std::vector<u32>& list, u64 lo, u64 hi, u64 elements, u32 depth) {
  if (elements == 0) return true;
  if (hi < lo || elements > hi - lo + 1 || depth > 64) return false;
  if (elements == hi - lo + 1) { for (u64 v = lo; v <= hi; ++v) list.push_back((u32)v); return true; }
  const u64 h = (elements - 1) / 2, r = elements / 2 - h;
  if (lo + h > hi - h - r) return false;
  u64 mid;
  if (!binary_decode(in, lo + h, hi - h - r, &mid)) return false;
  if (!interpolative_decode(in, list, lo, mid - 1, h, depth + 1)) return false;
  list.push_back((u32)mid);
  return interpolative_decode(in, list, mid + 1, hi, elements - h - 1, depth + 1);
}

// HuffmanDecoder::deserializeShape (HuffmanCoders.cpp:88-117) into device tables; 0 or an error code
static int read_shape(HostBits& in, HTable& t) {
  const u64 max_sym = in.bits(8);
  u64 nsym = in.bits(8);
  if (nsym == 0) nsym = 256;
  const u64 max_len = in.packed();
  if (in.over) return kHdPastRecord;
  if (max_len == 0 || max_len > 64 || nsym > max_sym + 1) return kHdShape;
  std::vector<u32> alphabet;
  alphabet.reserve(nsym);
  if (!interpolative_decode(in, alphabet, 0, max_sym, nsym, 0))
    return in.over ? kHdPastRecord : kHdShape;
  u8 clen[256] = {0};
  for (u64 i = 0; i < nsym; ++i) {
    u64 n = 1;
    while (!in.bitv()) { if (in.over) return kHdPastRecord; if (++n > max_len) return kHdShape; }
    clen[alphabet[i]] = (u8)(max_len - n + 1);
  }
  in.flush();
  if (in.over) return kHdPastRecord;
  // Kraft sum: an over-full code is no prefix code
  unsigned __int128 kraft = 0;
  u32 count[65] = {0};
  for (int c = 0; c < 256; ++c) if (clen[c]) { kraft += (unsigned __int128)1 << (64 - clen[c]); ++count[clen[c]]; }
  if (kraft > ((unsigned __int128)1 << 64)) return kHdNoCode;
  u64 first[65] = {0}, next_first = 0;            // computeHuffmanCodes, entropy_host.cpp
  for (int len = (int)max_len; len >= 0; --len) { first[len] = next_first; next_first = (next_first + count[len]) >> 1; }
  std::memset(&t, 0, sizeof(t));
  for (u32 i = 0; i < (1u << kFastBits); ++i) t.fast[i] = 0xFFFFu;
  u32 off = 0;
  for (u32 L = 1; L <= 64; ++L) { t.first[L] = first[L]; t.count[L] = count[L]; t.offset[L] = off; off += count[L]; }
  u32 fill[65] = {0};
  for (int c = 0; c < 256; ++c) {
    const u32 L = clen[c];
    if (!L) continue;
    const u64 code = first[L] + fill[L];
    t.syms[t.offset[L] + fill[L]++] = (u8)c;
    if (L <= kFastBits) {
      const u32 pad = kFastBits - L;
      const u64 b = code << pad;
      for (u64 f = 0; f < (1ull << pad) && b + f < (1u << kFastBits); ++f) t.fast[b + f] = (uint16_t)((c << 4) | L);
    } else {
      const u64 p = code >> (L - kFastBits);
      if (p < (1u << kFastBits) && t.fast[p] == 0xFFFFu) t.fast[p] = 0;
    }
  }
  t.max_len = (u32)max_len;
  return 0;
}

}  // namespace

struct HDecoder {
  int device = -1;
  u64 rec_cap = 0, run_cap = 0, len_cap = 0, off_cap = 0, part_cap = 0, map_cap = 0, ent_cap = 0, bwt_cap = 0;
  u64* d_rec = nullptr;
  u8* d_sym = nullptr;
  u32* d_len = nullptr;
  u32* d_off = nullptr;
  u32* d_partial = nullptr;
  u64* d_maps = nullptr;
  u64* d_ent = nullptr;
  u8* d_bwt = nullptr;
  HTable* d_tab = nullptr;
  SecResult* d_res = nullptr;
  HTable* h_tab = nullptr;                        // pinned
  SecResult* h_res = nullptr;                     // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evA = nullptr, evB = nullptr;   // whole decode / one section's kernels
  bwtc_hip_huffman_decode_stats stats{};

  void release() {
    void* dev[] = {d_rec, d_sym, d_len, d_off, d_partial, d_maps, d_ent, d_bwt, d_tab, d_res};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (h_tab) (void)hipHostFree(h_tab);
    if (h_res) (void)hipHostFree(h_res);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (evA) (void)hipEventDestroy(evA);
    if (evB) (void)hipEventDestroy(evB);
  }
};

HDecoder* hdecoder_create() { return new (std::nothrow) HDecoder(); }
void hdecoder_destroy(HDecoder* d) { if (d) { d->release(); delete d; } }
int hdecoder_stats(HDecoder* d, bwtc_hip_huffman_decode_stats* out) { if (!d) std::memset(out, 0, sizeof(*out)); else *out = d->stats; return 0; }
u8* hdecoder_bwt_buffer(HDecoder* d) { return d ? d->d_bwt : nullptr; }

template <typename T>
static hipError_t grow(T** p, u64* cap, u64 need) {
  if (need <= *cap) return hipSuccess;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const u64 n = need + need / 4;
  hipError_t rc = hipMalloc((void**)p, n * sizeof(T));
  if (rc == hipSuccess) *cap = n;
  return rc;
}

// maps of one stream at every level: level 0 = tiles, level l+1 = ceil(level l / 64) maps
struct Levels { u32 n[8]; u64 map_off[8]; u64 ent_off[8]; u32 count; u64 map_words; u64 ent_words; };
static Levels plan_levels(u32 ntiles, u32 M) {
  Levels L{};
  u64 mw = 0, ew = 0;
  u32 n = ntiles;
  for (;;) {
    L.n[L.count] = n; L.map_off[L.count] = mw; L.ent_off[L.count] = ew;
    mw += (u64)n * M; ew += n; ++L.count;
    if (n <= (u32)kWave) break;
    n = ceil_div(n, kWave);
  }
  L.map_words = mw; L.ent_words = ew;
  return L;
}

// one stream: maps, up, down, decode
template <bool GAMMA>
static void run_stream(HDecoder& d, hipStream_t st, u64 rec_bits, const u64* d_start, u64 start_h, u64 win, u32 M, u32 ntiles,
                       u64 n_runs, u64 run_base, const Levels& L, u32 soft) {
  u64* maps = d.d_maps;
  u64* ent = d.d_ent;
  const u32 waves = ceil_div(ntiles, kWave / M);
  hipLaunchKernelGGL(k_hd_map<GAMMA>, dim3(ceil_div((u64)waves * kWave, kMapTPB)), dim3(kMapTPB), 0, st, d.d_rec, rec_bits, d_start,
                     start_h, win, M, d.d_tab, ntiles, maps);
  for (u32 l = 0; l + 1 < L.count; ++l)
    hipLaunchKernelGGL(k_hd_compose, dim3(L.n[l + 1]), dim3(kWave), 0, st, maps + L.map_off[l], L.n[l], M,
                       maps + L.map_off[l + 1], L.n[l + 1]);
  const u32 top = L.count - 1;
  hipLaunchKernelGGL(k_hd_down, dim3(1), dim3(kWave), 0, st, maps + L.map_off[top], L.n[top], M, (const u64*)nullptr,
                     ent + L.ent_off[top], 1u);
  for (u32 l = top; l-- > 0;)
    hipLaunchKernelGGL(k_hd_down, dim3(L.n[l + 1]), dim3(kWave), 0, st, maps + L.map_off[l], L.n[l], M,
                       (const u64*)(ent + L.ent_off[l + 1]), ent + L.ent_off[l], L.n[l + 1]);
  hipLaunchKernelGGL(k_hd_decode<GAMMA>, dim3(ceil_div(ntiles, kDecTPB)), dim3(kDecTPB), 0, st, d.d_rec, rec_bits, d_start, start_h,
                     win, M, d.d_tab, ntiles, (const u64*)ent, n_runs, d.d_sym + run_base, d.d_len + run_base, d.d_res, soft);
  d.stats.tiles += ntiles;
  d.stats.map_entries += (u64)ntiles * M;
  d.stats.launches += 2 + 2 * (L.count - 1) + 1;
}

#define HD_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_ == hipErrorOutOfMemory ? -2 : -3; } while (0)

int huffman_decode(BwtEngine& e, HDecoder& d, const u8* rec, const u8* d_rec_src, u64 rec_bytes, u8* d_out, u64 cap,
                   u32* lf_out, u32* n_lf_out, u32* size_out, u64* consumed_out) {
  hipStream_t st = e.stream;
  HD_TRY(hipSetDevice(e.device));
  if (!d.h_tab) {
    HD_TRY(hipHostMalloc((void**)&d.h_tab, sizeof(HTable), 0));
    HD_TRY(hipHostMalloc((void**)&d.h_res, sizeof(SecResult), 0));
    HD_TRY(hipMalloc((void**)&d.d_tab, sizeof(HTable)));
    HD_TRY(hipMalloc((void**)&d.d_res, sizeof(SecResult)));
    HD_TRY(hipEventCreate(&d.ev0));
    HD_TRY(hipEventCreate(&d.ev1));
    HD_TRY(hipEventCreate(&d.evA));
    HD_TRY(hipEventCreate(&d.evB));
  }
  d.stats.sections = d.stats.streams = 0;
  d.stats.runs = d.stats.tiles = d.stats.map_entries = d.stats.launches = 0;
  d.stats.host_syncs = d.stats.retries = d.stats.max_code_len = 0;
  d.stats.ms_entropy = d.stats.ms_entropy_wall = d.stats.ms_chain_host = d.stats.ms_inverse = 0.f;
  float ms_kernels = 0.f;
  d.stats.route = 0;

  // ---- header (read48bits, BWTBlock::readHeader BWTBlock.cpp:88-102, section lengths) ----
  // The buffer may go on past the record (a caller hands over the rest of a file): only the
  // record the 48-bit length announces is read, uploaded and mapped.  A stream that runs past that
  // end while the buffer goes on disagrees with the length field (E_LENGTH); one that runs past
  // the buffer is cut short (E_PAST_RECORD).
  if (rec_bytes < 6) return kHdPastRecord;
  u64 compressed = 0;
  for (int i = 0; i < 6; ++i) compressed = (compressed << 8) | rec[i];
  const u64 rec_end = std::min<u64>(rec_bytes, 6 + compressed);
  const int past = rec_end < rec_bytes ? kHdLength : kHdPastRecord;
  HostBits in{rec, rec_end};
  in.bit = 48;
  const u32 n_lf = (u32)in.bits(8) + 1;
  u32 lf[256];
  for (u32 i = 0; i < n_lf; ++i) lf[i] = (u32)in.bits(31);
  in.flush();
  u64 sections = in.bits(8);
  if (sections == 0) sections = 256;
  u64 sec_len[256], total = 0;
  for (u64 i = 0; i < sections; ++i) { sec_len[i] = in.packed(); if (sec_len[i] > cap) sec_len[i] = cap + 1; total += sec_len[i]; }
  if (in.over) return past;
  if (total > cap || total > 0xFFFFFFF0ull) return kHdCapacity;      // run offsets are 32-bit

  // ---- workspace (first call, grown on demand) ----
  const u64 rec_words = (rec_end + 7) / 8 + 2;
  HD_TRY(grow(&d.d_rec, &d.rec_cap, rec_words));
  HD_TRY(grow(&d.d_sym, &d.run_cap, total + 1));
  HD_TRY(grow(&d.d_len, &d.len_cap, total + 1));
  HD_TRY(grow(&d.d_off, &d.off_cap, total + 1));
  HD_TRY(grow(&d.d_partial, &d.part_cap, (u64)ceil_div(total + 1, kScanTile) + 1));
  HD_TRY(grow(&d.d_bwt, &d.bwt_cap, total + 64));
  HD_TRY(hipMemsetAsync((u8*)d.d_rec + (rec_words - 2) * 8, 0, 16, st));
  HD_TRY(hipMemsetAsync((u8*)d.d_rec + (rec_end & ~7ull), 0, 8, st));
  HD_TRY(hipEventRecord(d.ev0, st));
  if (d_rec_src) HD_TRY(hipMemcpyAsync(d.d_rec, d_rec_src, rec_end, hipMemcpyDeviceToDevice, st));
  else HD_TRY(hipMemcpyAsync(d.d_rec, rec, rec_end, hipMemcpyHostToDevice, st));
  const u64 rec_bits = rec_end * 8;

  u64 run_base = 0;
  for (u64 s = 0; s < sections; ++s) {
    const u64 S = sec_len[s];
    if (!S) continue;
    const u64 n_runs = in.packed();
    if (in.over) return past;
    if (n_runs == 0 || n_runs > S) return kHdRuns;
    const int rs = read_shape(in, *d.h_tab);
    if (rs) return rs == kHdPastRecord ? past : rs;
    const u64 h0 = in.bit;
    // windows: a stream is at most n_runs codes of its longest length; the gamma stream of lengths
    // that add up to S is at most n (2 log2(S/n) + 1) bits (Jensen)
    const u32 Mh = d.h_tab->max_len;
    const u32 Mg = 2 * (63 - __builtin_clzll(S)) + 1;
    if (h0 >= rec_bits) return past;
    d.stats.max_code_len = std::max(d.stats.max_code_len, Mh);
    const u64 full_h = std::min<u64>(n_runs * Mh, rec_bits - h0);
    // first try: twice the length a code fitted to its lengths gives n_runs symbols (sum of
    // len * 2^-len per run); a stream that does not end there is mapped again over full_h
    double kraft_len = 0;
    for (u32 L = 1; L <= Mh; ++L) kraft_len += (double)d.h_tab->count[L] * L * std::ldexp(1.0, -(int)L);
    const u64 est_h = (u64)(2.0 * kraft_len * (double)n_runs) + 4096;
    u64 win_h = std::min(full_h, est_h);
  retry:
    const double gb = (double)n_runs * (2.0 * std::log2((double)S / (double)n_runs) + 1.0);
    const u64 win_g = std::min<u64>((u64)gb + 64 + n_runs / 1024, rec_bits - h0);
    const u32 soft = win_h < full_h;
    const u32 nt_h = ceil_div(win_h, kTileBits), nt_g = ceil_div(win_g, kTileBits);
    const Levels Lh = plan_levels(nt_h, Mh), Lg = plan_levels(nt_g, Mg);
    HD_TRY(grow(&d.d_maps, &d.map_cap, std::max(Lh.map_words, Lg.map_words)));
    HD_TRY(grow(&d.d_ent, &d.ent_cap, std::max(Lh.ent_words, Lg.ent_words)));
    d.h_res->hend = kNoEnd; d.h_res->gend = kNoEnd; d.h_res->sum = 0; d.h_res->err = 0; d.h_res->pad = 0;
    HD_TRY(hipMemcpyAsync(d.d_tab, d.h_tab, sizeof(HTable), hipMemcpyHostToDevice, st));
    HD_TRY(hipMemcpyAsync(d.d_res, d.h_res, sizeof(SecResult), hipMemcpyHostToDevice, st));
    HD_TRY(hipEventRecord(d.evA, st));
    run_stream<false>(d, st, rec_bits, nullptr, h0, win_h, Mh, nt_h, n_runs, run_base, Lh, soft);
    run_stream<true>(d, st, rec_bits, &d.d_res->hend, 0, win_g, Mg, nt_g, n_runs, run_base, Lg, 0u);
    HD_TRY(hipEventRecord(d.evB, st));
    HD_TRY(hipMemcpyAsync(d.h_res, d.d_res, sizeof(SecResult), hipMemcpyDeviceToHost, st));
    HD_TRY(hipStreamSynchronize(st));
    HD_TRY(hipGetLastError());
    ++d.stats.host_syncs;
    { float ms = 0.f; (void)hipEventElapsedTime(&ms, d.evA, d.evB); ms_kernels += ms; }
    const SecResult r = *d.h_res;
    if (r.err) return r.err == (u32)-kHdPastRecord ? past : -(int)r.err;
    if (r.hend >= kNoEnd && soft) { win_h = full_h; ++d.stats.retries; goto retry; }
    if (r.hend >= kNoEnd || r.gend >= kNoEnd) {
      // the path left the window: past the record, or (gamma) lengths that cannot add up to S
      if (r.hend >= kNoEnd) return full_h == rec_bits - h0 ? past : kHdNoCode;
      return win_g == rec_bits - h0 ? past : kHdRuns;
    }
    if (r.sum != S) return kHdRuns;
    in.bit = (r.gend + 7) & ~7ull;
    run_base += n_runs;
    d.stats.sections++;
    d.stats.streams += 2;
  }
  const u64 consumed = in.bit >> 3;
  if (consumed > rec_end) return past;
  if (consumed - 6 != compressed) return kHdLength;

  // ---- offsets and expansion ----
  HD_TRY(hipEventRecord(d.evA, st));
  const bool direct = d_out && ((uintptr_t)d_out & 15) == 0;   // the expansion stores 16 bytes at a time
  u8* out = direct ? d_out : d.d_bwt;
  if (run_base) {
    HD_TRY(hipMemcpyAsync(d.d_off, d.d_len, run_base * 4, hipMemcpyDeviceToDevice, st));
    exclusive_scan_u32(d.d_off, run_base, d.d_partial, st);
    hipLaunchKernelGGL(k_hd_expand, dim3(ceil_div(ceil_div(total, kExpandBytes), 256)), dim3(256), 0, st, (const u8*)d.d_sym,
                       (const u32*)d.d_off, run_base, (u32)total, out);
    d.stats.launches += 2;
    if (d_out && !direct) HD_TRY(hipMemcpyAsync(d_out, d.d_bwt, total, hipMemcpyDeviceToDevice, st));
  }
  HD_TRY(hipEventRecord(d.ev1, st));
  HD_TRY(hipStreamSynchronize(st));
  HD_TRY(hipGetLastError());
  { float ms = 0.f; (void)hipEventElapsedTime(&ms, d.evA, d.ev1); ms_kernels += ms; }
  (void)hipEventElapsedTime(&d.stats.ms_entropy_wall, d.ev0, d.ev1);
  d.stats.ms_entropy = ms_kernels;
  d.stats.ms_chain_host = std::max(0.f, d.stats.ms_entropy_wall - ms_kernels);
  d.stats.runs = run_base;
  d.stats.route = 1;
  d.stats.workspace_bytes = d.rec_cap * 8 + d.run_cap + (d.len_cap + d.off_cap + d.part_cap) * 4 + (d.map_cap + d.ent_cap) * 8 + d.bwt_cap +
                            sizeof(HTable) + sizeof(SecResult);
  for (u32 i = 0; i < n_lf; ++i) lf_out[i] = lf[i];
  *n_lf_out = n_lf;
  *size_out = (u32)total;
  *consumed_out = consumed;
  return 0;
}

int huffman_decode_block_device(BwtEngine& e, HDecoder& d, const u8* rec, u64 rec_bytes, u8* d_out, u64 cap, u32* size_out,
                                u64* consumed_out) {
  u32 lf[256], n_lf = 0, size = 0;
  int rc = huffman_decode(e, d, rec, nullptr, rec_bytes, nullptr, std::min<u64>(cap, e.max_block), lf, &n_lf, &size, consumed_out);
  if (rc) return rc;
  if (size) {
    rc = inverse_bwt_device(e, d.d_bwt, d_out, size, lf, n_lf);
    d.stats.ms_inverse = e.stats.ms_total;
    if (rc) return rc;
  }
  *size_out = size;
  return 0;
}

int huffman_decode_block(BwtEngine& e, HDecoder& d, const u8* rec, u64 rec_bytes, u8* out, u64 cap, u32* size_out, u64* consumed_out) {
  u32 size = 0;
  const int rc = huffman_decode_block_device(e, d, rec, rec_bytes, e.d_in, cap, &size, consumed_out);
  if (rc) return rc;
  if (size) {
    HD_TRY(hipMemcpyAsync(e.h_stage, e.d_in, size, hipMemcpyDeviceToHost, e.stream));
    HD_TRY(e.wait());
    std::memcpy(out, e.h_stage, size);
  }
  *size_out = size;
  return 0;
}

}  // namespace bwtc_hip
