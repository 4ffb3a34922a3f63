// The wavelet rebuild on the device (gfx950, wave64): flattened forest -> BWT bytes.  Passes, all on the context's
// stream with one read-back per block:
//   k_wr_line_count   ones of every 7-word line of the word array
//   3-launch scan     exclusive prefix of the line counts (scan.hpp's reduce / apply; never the chained form)
//   k_wr_lines        the rank directory: 64-byte lines of 7 words of bits + the ones before the line, so ONE
//                     64-byte read serves a rank query (a prefix per word beside the words would take two requests,
//                     the gather's cost on this memory system being requests, not bytes)
//   k_wr_node_rank    every node's rank origin (ones before its first word)
//   k_wr_walk         one run per thread, grid stride: symbol tree, length code, escape (wr_walk, wavelet_rebuild.hpp)
//   k_wr_verdict      the sections' totals against their announced bytes
//   3-launch scan     exclusive prefix of the run lengths
//   k_wr_expand       runs -> bytes, 32 per thread with 16-byte stores; does nothing once the error word is set
// Every loop is bounded by a node's bit count, a step cap or the output's size, so a forest decoded from a corrupt
// record ends in an error code, not in a fault.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>

#include "bwt_engine.hpp"
#include "scan.hpp"
#include "wavelet_rebuild.hpp"

namespace bwtc_hip {

namespace {

constexpr u32 kWalkTPB = 256;
constexpr u32 kExpandBytes = 32;
constexpr u64 kNoError = ~0ull;

// what the walks leave for the host: read back once per block
struct WrResult {
  unsigned long long err;                  // (run or section index << 8) | -code of the first thing wrong; kNoError
  unsigned long long bit_reads;
  unsigned long long sec_total[kWrMaxSections];
};

// ---- rank directory ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wr_line_count(const u64* __restrict__ words, u64 n_words, u32* __restrict__ cnt, u32 n_lines) {
  const u32 line = blockIdx.x * 256u + threadIdx.x;
  if (line >= n_lines) return;
  const u64 w0 = (u64)line * kWrLineWords;
  u32 c = 0;
#pragma unroll
  for (u32 k = 0; k < kWrLineWords; ++k) if (w0 + k < n_words) c += (u32)__popcll(words[w0 + k]);
  cnt[line] = c;
}

// eight threads per line: one 64-byte store per line, coalesced over the wave
__global__ __launch_bounds__(256) void k_wr_lines(const u64* __restrict__ words, u64 n_words, const u32* __restrict__ prefix,
                                                  u64* __restrict__ lines, u32 n_lines) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 line = i >> 3;
  const u32 k = (u32)i & 7u;
  if (line >= n_lines) return;
  u64 v;
  if (k == kWrLineWords) v = prefix[line];
  else { const u64 w = line * kWrLineWords + k; v = w < n_words ? words[w] : 0ull; }
  lines[i] = v;
}

// One lane reads the whole line (four 16-byte loads into 8 registers) and counts up to 6 words before its own.
// NOT MEASURED: the choice of 7-word lines over a prefix per word rests on the request count alone (one 64-byte
// request per bit read against two); no counter run has compared the two layouts, and the popcounts and the
// division by 7 are the price that such a run would have to weigh against the saved request.
struct LineRank {
  const u64* __restrict__ lines;
  // ones of the word array before bit `bit` of word `gw` (mod 2^32), and that word
  __device__ __forceinline__ u32 operator()(u32 gw, u32 bit, u64& word) const {
    const u32 line = gw / kWrLineWords, slot = gw - line * kWrLineWords;
    const ulonglong2* L = reinterpret_cast<const ulonglong2*>(lines + (u64)line * 8u);
    const ulonglong2 a = L[0], b = L[1], c = L[2], d = L[3];
    const u64 w[8] = {a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
    u32 r = (u32)w[7];
    u64 cur = 0;
#pragma unroll
    for (u32 k = 0; k < kWrLineWords; ++k) {
      if (k < slot) r += (u32)__popcll(w[k]);
      if (k == slot) cur = w[k];
    }
    word = cur;
    return r + (u32)__popcll(cur & ((1ull << bit) - 1ull));
  }
};

__global__ __launch_bounds__(256) void k_wr_node_rank(WrNode* __restrict__ nodes, u32 n_nodes, const u64* __restrict__ lines) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_nodes) return;
  u32 r = 0;
  if (nodes[i].bits) { u64 w; r = LineRank{lines}(nodes[i].first_word, 0u, w); }
  nodes[i].rank0 = r;
}

// ---- the walk ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWalkTPB) void k_wr_walk(const WrSection* __restrict__ secs, u32 n_secs, const WrNode* __restrict__ nodes,
                                                      const WrCode* __restrict__ codes, const u64* __restrict__ lines, u64 n_runs,
                                                      u8* __restrict__ run_sym, u32* __restrict__ run_len, WrResult* __restrict__ res) {
  __shared__ u32 s_start[kWrMaxSections + 1];
  for (u32 i = threadIdx.x; i < n_secs; i += kWalkTPB) s_start[i] = secs[i].run_start;
  __syncthreads();
  const LineRank rank{lines};
  const u32 lane = lane_id();
  unsigned long long reads_sum = 0;
  const u64 stride = (u64)gridDim.x * kWalkTPB;
  // whole waves stay in the loop together (the totals are reduced over the wave)
  for (u64 base = (u64)blockIdx.x * kWalkTPB + (threadIdx.x & ~63u); base < n_runs; base += stride) {
    const u64 j = base + lane;
    const bool live = j < n_runs;
    u32 s = 0;
    unsigned long long len = 0;
    if (live) {
      u32 lo = 0, hi = n_secs - 1;                 // last section with run_start <= j
      while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if (s_start[mid] <= j) lo = mid; else hi = mid - 1; }
      s = lo;
      const WrSection S = secs[s];
      u32 sym = 0, reads = 0;
      u64 l = 0;
      const int rc = wr_walk(S, nodes, codes, rank, (u32)(j - S.run_start), &sym, &l, &reads);
      if (rc) { atomicMin(&res->err, (unsigned long long)((j << 8) | (u64)(u32)(-rc))); l = 0; }
      run_sym[j] = (u8)sym;
      run_len[j] = (u32)l;
      len = l;
      reads_sum += reads;
    }
    // a wave's runs lie in one section almost always: one atomic then, else one per lane
    const u32 s0 = __shfl(s, 0, kWave);
    if (__all(!live || s == s0)) {
      unsigned long long t = len;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, kWave);
      if (lane == 0 && t) atomicAdd(&res->sec_total[s0], t);
    } else if (live && len) {
      atomicAdd(&res->sec_total[s], len);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) reads_sum += __shfl_xor(reads_sum, o, kWave);
  if (lane == 0 && reads_sum) atomicAdd(&res->bit_reads, reads_sum);
}

__global__ __launch_bounds__(256) void k_wr_verdict(const WrSection* __restrict__ secs, u32 n_secs, WrResult* __restrict__ res) {
  if (res->err != kNoError) return;
  const u32 s = threadIdx.x;
  if (s < n_secs && res->sec_total[s] != secs[s].bytes)
    atomicMin(&res->err, (unsigned long long)(((u64)s << 8) | (u64)(u32)(-BWTC_HIP_E_W_TOTAL)));
}

// runs -> bytes: same job as the 'H' decoder's expansion, plus the error word (offsets of a refused forest are
// not monotone, and a search over them has no bound worth the name)
__global__ __launch_bounds__(256) void k_wr_expand(const u8* __restrict__ run_sym, const u32* __restrict__ run_off, u64 n_runs,
                                                   u32 size, u8* __restrict__ out, const WrResult* __restrict__ res) {
  if (res->err != kNoError) return;
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

// scan.hpp's three launches, whatever chain the calling thread's context has set up; returns the launches made
u32 scan3(u32* data, u64 n, u32* partial, hipStream_t st) {
  if (n == 0) return 0;
  const u32 tiles = ceil_div(n, kScanTile);
  if (tiles == 1) { hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, data, (u32)n, (u32*)nullptr); return 1; }
  hipLaunchKernelGGL(k_scan_reduce, dim3(tiles), dim3(kScanTPB), 0, st, data, partial, n);
  hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, partial, tiles, (u32*)nullptr);
  hipLaunchKernelGGL(k_scan_apply<false>, dim3(tiles), dim3(kScanTPB), 0, st, data, partial, n);
  return 3;
}

}  // namespace

// ---- tables ----------------------------------------------------------------------------------------------------
int wr_flatten(const bwtc_hip_wforest& f, u64 cap, std::vector<WrSection>& secs, std::vector<WrNode>& nodes, std::vector<WrCode>& codes,
               u64* total_out, u64* runs_out) {
  if (f.n_sections > kWrMaxSections) return BWTC_HIP_E_W_FOREST;
  if ((f.n_sections && !f.sections) || (f.n_nodes && !f.nodes) || (f.n_codes && !f.codes) || (f.n_words && !f.words)) return -1;
  if (f.n_words >= (u64(1) << 32)) return BWTC_HIP_E_W_LIMIT;
  secs.resize(f.n_sections);
  nodes.resize(f.n_nodes);
  codes.resize(f.n_codes);
  std::memset(nodes.data(), 0, nodes.size() * sizeof(WrNode));
  u64 total = 0, runs = 0;
  for (u32 s = 0; s < f.n_sections; ++s) {
    const bwtc_hip_wforest_section& S = f.sections[s];
    if (S.n_nodes == 0 || S.n_codes == 0 || (u64)S.first_node + S.n_nodes > f.n_nodes || (u64)S.first_code + S.n_codes > f.n_codes ||
        S.symbol_nodes == 0 || S.symbol_nodes > S.n_nodes || S.W > 15)
      return BWTC_HIP_E_W_FOREST;
    if (S.runs == 0 || S.runs > S.bytes) return BWTC_HIP_E_W_TOTAL;   // a run is at least one byte
    total += S.bytes;
    if (total > cap) return BWTC_HIP_E_W_CAP;
    if (total >= (u64(1) << 31)) return BWTC_HIP_E_W_LIMIT;
    WrSection& D = secs[s];
    D.run_start = (u32)runs; D.runs = S.runs; D.bytes = S.bytes; D.first_node = S.first_node; D.symbol_nodes = S.symbol_nodes;
    D.n_nodes = S.n_nodes; D.first_code = S.first_code; D.n_codes = S.n_codes; D.W = S.W; D.plain_fixed = S.plain_fixed ? 1u : 0u;
    runs += S.runs;
    for (u32 i = 0; i < S.n_nodes; ++i) {
      const bwtc_hip_wforest_node& n = f.nodes[S.first_node + i];
      if (n.left < -1 || n.right < -1 || n.left >= (int)S.n_nodes || n.right >= (int)S.n_nodes) return BWTC_HIP_E_W_FOREST;
      if (n.bits && (u64)n.first_word + ((u64)n.bits + 63) / 64 > f.n_words) return BWTC_HIP_E_W_FOREST;
      WrNode& d = nodes[S.first_node + i];
      d.left = n.left < 0 ? -1 : (int)(S.first_node + n.left);
      d.right = n.right < 0 ? -1 : (int)(S.first_node + n.right);
      d.sym = (n.has_symbol && i < S.symbol_nodes ? 0x80000000u : 0u) | (n.symbol & 0xFFu);
      d.bits = n.bits;
      d.first_word = n.bits ? n.first_word : 0u;
    }
    for (u32 i = 0; i < S.n_codes; ++i) {
      const bwtc_hip_wforest_code& c = f.codes[S.first_code + i];
      if (c.left < -1 || c.right < -1 || c.left >= (int)S.n_codes || c.right >= (int)S.n_codes) return BWTC_HIP_E_W_FOREST;
      WrCode& d = codes[S.first_code + i];
      d.left = c.left < 0 ? -1 : (int)(S.first_code + c.left);
      d.right = c.right < 0 ? -1 : (int)(S.first_code + c.right);
      d.has_symbol = c.has_symbol ? 1u : 0u;
      d.symbol = c.symbol;
    }
  }
  *total_out = total;
  *runs_out = runs;
  return 0;
}

// ---- host twin ---------------------------------------------------------------------------------------------------
namespace {
struct HostRank {
  const u64* words; const u64* dir; u32 G;
  u32 operator()(u32 gw, u32 bit, u64& word) const {
    const u64 line = gw / G;
    u64 r = dir[line];
    for (u64 k = line * G; k < gw; ++k) r += (u64)__builtin_popcountll(words[k]);
    word = words[gw];
    return (u32)(r + (u64)__builtin_popcountll(word & ((1ull << bit) - 1ull)));
  }
};
}  // namespace

int host_wavelet_rebuild(const bwtc_hip_wforest& f, u8* out, u64 cap, u64* size, u32 G, u64* bit_reads) {
  if (G == 0) return -1;
  std::vector<WrSection> secs; std::vector<WrNode> nodes; std::vector<WrCode> codes;
  u64 total = 0, runs = 0;
  const int rc = wr_flatten(f, cap, secs, nodes, codes, &total, &runs);
  if (rc) return rc;
  const u64 n_lines = (f.n_words + G - 1) / G;
  std::vector<u64> dir(n_lines + 1, 0);
  { u64 acc = 0;
    for (u64 l = 0; l < n_lines; ++l) {
      dir[l] = acc;
      for (u64 k = l * G; k < std::min<u64>(f.n_words, (l + 1) * G); ++k) acc += (u64)__builtin_popcountll(f.words[k]);
    } }
  const HostRank rank{f.words, dir.data(), G};
  for (WrNode& n : nodes) if (n.bits) { u64 w; n.rank0 = rank(n.first_word, 0, w); }
  // the device's order of verdicts: the first run that goes wrong, then the first section whose total is off
  std::vector<u8> sym(runs);
  std::vector<u32> len(runs);
  u64 reads_sum = 0;
  std::vector<u64> sec_total(secs.size(), 0);
  for (size_t s = 0; s < secs.size(); ++s)
    for (u32 i = 0; i < secs[s].runs; ++i) {
      u32 sy = 0, reads = 0; u64 l = 0;
      const int wrc = wr_walk(secs[s], nodes.data(), codes.data(), rank, i, &sy, &l, &reads);
      if (wrc) return wrc;
      sym[secs[s].run_start + i] = (u8)sy; len[secs[s].run_start + i] = (u32)l;
      sec_total[s] += l; reads_sum += reads;
    }
  for (size_t s = 0; s < secs.size(); ++s) if (sec_total[s] != secs[s].bytes) return BWTC_HIP_E_W_TOTAL;
  u64 at = 0;
  for (u64 j = 0; j < runs; ++j) { std::memset(out + at, sym[j], len[j]); at += len[j]; }   // at + len <= total <= cap
  *size = total;
  if (bit_reads) *bit_reads = reads_sum;
  return 0;
}

// ---- device workspace -----------------------------------------------------------------------------------------
#define WR_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_ == hipErrorOutOfMemory ? -2 : -3; } while (0)

struct WRebuild {
  u64 word_cap = 0, line_cap = 0, cnt_cap = 0, part_cap = 0, node_cap = 0, code_cap = 0, run_cap = 0, len_cap = 0, off_cap = 0, bwt_cap = 0;
  u64* d_words = nullptr;
  u64* d_lines = nullptr;
  u32* d_cnt = nullptr;
  u32* d_partial = nullptr;
  WrNode* d_nodes = nullptr;
  WrCode* d_codes = nullptr;
  u8* d_sym = nullptr;
  u32* d_len = nullptr;
  u32* d_off = nullptr;
  u8* d_bwt = nullptr;
  WrSection* d_secs = nullptr;
  WrResult* d_res = nullptr;
  // page-locked staging of the tables (the words of the decode route are page-locked in the forest itself)
  u64 h_node_cap = 0, h_code_cap = 0;
  WrNode* h_nodes = nullptr;
  WrCode* h_codes = nullptr;
  WrSection* h_secs = nullptr;
  WrResult* h_res = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // two forests in page-locked memory: the range decoder fills one while the device half of the block before it
  // reads the other (wavelet_decode_begin / wavelet_decode_end)
  WrForest forest[kWrSlots];
  float ms_range[kWrSlots] = {0.f, 0.f};
  std::vector<WrSection> secs; std::vector<WrNode> nodes; std::vector<WrCode> codes;
  bwtc_hip_wavelet_decode_stats stats{};

  void release() {
    void* dev[] = {d_words, d_lines, d_cnt, d_partial, d_nodes, d_codes, d_sym, d_len, d_off, d_bwt, d_secs, d_res};
    for (void* p : dev) if (p) (void)hipFree(p);
    void* host[] = {h_nodes, h_codes, h_secs, h_res};
    for (void* p : host) if (p) (void)hipHostFree(p);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (WrForest& f : forest) f.words.drop();
  }
};

static void* pinned_alloc(u64 bytes) { void* p = nullptr; return hipHostMalloc(&p, bytes, 0) == hipSuccess ? p : nullptr; }
static void pinned_free(void* p) { (void)hipHostFree(p); }

WRebuild* wrebuild_create() {
  WRebuild* w = new (std::nothrow) WRebuild();
  if (w) for (WrForest& f : w->forest) { f.words.alloc = pinned_alloc; f.words.release = pinned_free; }
  return w;
}
void wrebuild_destroy(WRebuild* w) { if (w) { w->release(); delete w; } }
int wrebuild_stats(WRebuild* w, bwtc_hip_wavelet_decode_stats* out) { if (!w) std::memset(out, 0, sizeof(*out)); else *out = w->stats; return 0; }

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
template <typename T>
static hipError_t grow_pinned(T** p, u64* cap, u64 need) {
  if (need <= *cap) return hipSuccess;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const u64 n = need + need / 4;
  hipError_t rc = hipHostMalloc((void**)p, n * sizeof(T), 0);
  if (rc == hipSuccess) *cap = n;
  return rc;
}

int wavelet_rebuild_device(BwtEngine& e, WRebuild& w, const bwtc_hip_wforest& f, u8* d_out, u64 cap, u64* size, u8** d_bwt) {
  hipStream_t st = e.stream;
  WR_TRY(hipSetDevice(e.device));
  w.stats.route = 0;
  w.stats.sections = 0;
  w.stats.runs = w.stats.nodes = w.stats.words = w.stats.bit_reads = w.stats.launches = 0;
  w.stats.ms_rebuild = w.stats.ms_inverse = 0.f;
  u64 total = 0, runs = 0;
  const int frc = wr_flatten(f, cap, w.secs, w.nodes, w.codes, &total, &runs);
  if (frc) return frc;
  // each on its own: a call that failed half way through leaves the rest for the next one
  if (!w.h_secs) WR_TRY(hipHostMalloc((void**)&w.h_secs, sizeof(WrSection) * kWrMaxSections, 0));
  if (!w.h_res) WR_TRY(hipHostMalloc((void**)&w.h_res, sizeof(WrResult), 0));
  if (!w.d_secs) WR_TRY(hipMalloc((void**)&w.d_secs, sizeof(WrSection) * kWrMaxSections));
  if (!w.d_res) WR_TRY(hipMalloc((void**)&w.d_res, sizeof(WrResult)));
  if (!w.ev0) WR_TRY(hipEventCreate(&w.ev0));
  if (!w.ev1) WR_TRY(hipEventCreate(&w.ev1));
  *size = total;
  if (d_bwt) *d_bwt = nullptr;
  if (total == 0) { w.stats.route = 1; ++w.stats.routed_device; return 0; }
  const u32 n_secs = (u32)w.secs.size(), n_nodes = (u32)w.nodes.size(), n_codes = (u32)w.codes.size();
  const u64 n_words = f.n_words;
  const u32 n_lines = (u32)((n_words + kWrLineWords - 1) / kWrLineWords);

  WR_TRY(grow(&w.d_words, &w.word_cap, n_words + 1));
  WR_TRY(grow(&w.d_lines, &w.line_cap, (u64)n_lines * 8 + 8));
  WR_TRY(grow(&w.d_cnt, &w.cnt_cap, (u64)n_lines + 1));
  WR_TRY(grow(&w.d_nodes, &w.node_cap, n_nodes));
  WR_TRY(grow(&w.d_codes, &w.code_cap, n_codes));
  WR_TRY(grow(&w.d_sym, &w.run_cap, runs + 1));
  WR_TRY(grow(&w.d_len, &w.len_cap, runs + 1));
  WR_TRY(grow(&w.d_off, &w.off_cap, runs + 1));
  WR_TRY(grow(&w.d_partial, &w.part_cap, (u64)ceil_div(std::max<u64>(runs, n_lines) + 1, kScanTile) + 1));
  WR_TRY(grow(&w.d_bwt, &w.bwt_cap, total + 64));
  WR_TRY(grow_pinned(&w.h_nodes, &w.h_node_cap, n_nodes));
  WR_TRY(grow_pinned(&w.h_codes, &w.h_code_cap, n_codes));
  std::memcpy(w.h_secs, w.secs.data(), n_secs * sizeof(WrSection));
  std::memcpy(w.h_nodes, w.nodes.data(), (u64)n_nodes * sizeof(WrNode));
  std::memcpy(w.h_codes, w.codes.data(), (u64)n_codes * sizeof(WrCode));
  std::memset(w.h_res, 0, sizeof(WrResult));
  w.h_res->err = kNoError;

  WR_TRY(hipEventRecord(w.ev0, st));
  WR_TRY(hipMemcpyAsync(w.d_secs, w.h_secs, n_secs * sizeof(WrSection), hipMemcpyHostToDevice, st));
  WR_TRY(hipMemcpyAsync(w.d_nodes, w.h_nodes, (u64)n_nodes * sizeof(WrNode), hipMemcpyHostToDevice, st));
  WR_TRY(hipMemcpyAsync(w.d_codes, w.h_codes, (u64)n_codes * sizeof(WrCode), hipMemcpyHostToDevice, st));
  WR_TRY(hipMemcpyAsync(w.d_res, w.h_res, sizeof(WrResult), hipMemcpyHostToDevice, st));
  if (n_words) WR_TRY(hipMemcpyAsync(w.d_words, f.words, n_words * 8, hipMemcpyHostToDevice, st));
  u64 launches = 0;
  if (n_lines) {
    hipLaunchKernelGGL(k_wr_line_count, dim3(ceil_div(n_lines, 256)), dim3(256), 0, st, (const u64*)w.d_words, n_words, w.d_cnt, n_lines);
    launches += 1 + scan3(w.d_cnt, n_lines, w.d_partial, st);
    hipLaunchKernelGGL(k_wr_lines, dim3(ceil_div((u64)n_lines * 8, 256)), dim3(256), 0, st, (const u64*)w.d_words, n_words,
                       (const u32*)w.d_cnt, w.d_lines, n_lines);
    ++launches;
  }
  hipLaunchKernelGGL(k_wr_node_rank, dim3(ceil_div(n_nodes, 256)), dim3(256), 0, st, w.d_nodes, n_nodes, (const u64*)w.d_lines);
  const u32 walk_blocks = (u32)std::min<u64>(ceil_div(runs, kWalkTPB), 256u * 16u);
  hipLaunchKernelGGL(k_wr_walk, dim3(walk_blocks), dim3(kWalkTPB), 0, st, (const WrSection*)w.d_secs, n_secs, (const WrNode*)w.d_nodes,
                     (const WrCode*)w.d_codes, (const u64*)w.d_lines, runs, w.d_sym, w.d_len, w.d_res);
  hipLaunchKernelGGL(k_wr_verdict, dim3(1), dim3(256), 0, st, (const WrSection*)w.d_secs, n_secs, w.d_res);
  const bool direct = d_out && ((uintptr_t)d_out & 15) == 0;        // the expansion stores 16 bytes at a time
  u8* out = direct ? d_out : w.d_bwt;
  WR_TRY(hipMemcpyAsync(w.d_off, w.d_len, runs * 4, hipMemcpyDeviceToDevice, st));
  launches += 3 + scan3(w.d_off, runs, w.d_partial, st);
  hipLaunchKernelGGL(k_wr_expand, dim3(ceil_div(ceil_div(total, kExpandBytes), 256)), dim3(256), 0, st, (const u8*)w.d_sym,
                     (const u32*)w.d_off, runs, (u32)total, out, (const WrResult*)w.d_res);
  ++launches;
  if (d_out && !direct) WR_TRY(hipMemcpyAsync(d_out, w.d_bwt, total, hipMemcpyDeviceToDevice, st));
  WR_TRY(hipEventRecord(w.ev1, st));
  WR_TRY(hipMemcpyAsync(w.h_res, w.d_res, sizeof(WrResult), hipMemcpyDeviceToHost, st));
  WR_TRY(hipStreamSynchronize(st));
  WR_TRY(hipGetLastError());
  (void)hipEventElapsedTime(&w.stats.ms_rebuild, w.ev0, w.ev1);
  w.stats.sections = n_secs;
  w.stats.runs = runs; w.stats.nodes = n_nodes; w.stats.words = n_words;
  w.stats.bit_reads = w.h_res->bit_reads;
  w.stats.launches = launches;
  w.stats.workspace_bytes = (w.word_cap + w.line_cap) * 8 + (w.cnt_cap + w.part_cap + w.len_cap + w.off_cap) * 4 + w.node_cap * sizeof(WrNode) +
                            w.code_cap * sizeof(WrCode) + w.run_cap + w.bwt_cap + sizeof(WrSection) * kWrMaxSections + sizeof(WrResult);
  if (w.h_res->err != kNoError) return -(int)(w.h_res->err & 0xFFu);
  w.stats.route = 1;
  ++w.stats.routed_device;
  if (d_bwt) *d_bwt = out;
  return 0;
}

// The host half of a block: the record's forest into slot `slot`.  No device work and no statistics are touched, so it
// may run on one thread while another is inside wavelet_decode_end of the other slot.
int wavelet_decode_begin(BwtEngine& e, WRebuild& w, WDecoderState& dec, const u8* rec, u64 rec_bytes, u64 cap, u32 slot, u32* size,
                         u64* consumed) {
  if (slot >= kWrSlots) return -1;
  WR_TRY(hipSetDevice(e.device));                                    // the forest's words are page-locked
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = wavelet_range_decode(dec, rec, rec_bytes, std::min<u64>(cap, e.max_block), w.forest[slot], consumed);
  w.ms_range[slot] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc) return rc;
  *size = (u32)w.forest[slot].bytes;
  return 0;
}

// The device half: upload of slot `slot`, rebuild, inverse; the original block at d_out.
int wavelet_decode_end_device(BwtEngine& e, WRebuild& w, u32 slot, u8* d_out, u64 cap, u32* size) {
  if (slot >= kWrSlots) return -1;
  WR_TRY(hipSetDevice(e.device));
  w.stats.route = 0;
  const WrForest& F = w.forest[slot];
  u64 total = 0;
  u8* d_bwt = nullptr;
  int rc = wavelet_rebuild_device(e, w, F.view(), nullptr, std::min<u64>(cap, e.max_block), &total, &d_bwt);
  w.stats.ms_range_decode = w.ms_range[slot];
  if (rc) return rc;
  if (total) {
    rc = inverse_bwt_device(e, d_bwt, d_out, (u32)total, F.lf, F.n_lf);
    w.stats.ms_inverse = e.stats.ms_total;
    if (rc) return rc;
  }
  *size = (u32)total;
  return 0;
}

// The same with the block downloaded through the context's page-locked stage into out (host).
int wavelet_decode_end(BwtEngine& e, WRebuild& w, u32 slot, u8* out, u64 cap, u32* size) {
  u32 n = 0;
  const int rc = wavelet_decode_end_device(e, w, slot, e.d_in, cap, &n);
  if (rc) return rc;
  if (n) {
    WR_TRY(hipMemcpyAsync(e.h_stage, e.d_in, n, hipMemcpyDeviceToHost, e.stream));
    WR_TRY(e.wait());
    std::memcpy(out, e.h_stage, n);
  }
  *size = n;
  return 0;
}

// begin + end in one call; whatever refuses the record, the decoder is left as it was before the call
int wavelet_decode_block_device(BwtEngine& e, WRebuild& w, WDecoderState& dec, const u8* rec, u64 rec_bytes, u8* d_out, u64 cap, u32* size,
                                u64* consumed) {
  u32 n = 0;
  int rc = wavelet_decode_begin(e, w, dec, rec, rec_bytes, cap, 0, &n, consumed);
  if (rc) { w.stats.route = 0; return rc; }
  rc = wavelet_decode_end_device(e, w, 0, d_out, cap, size);
  if (rc) wdecoder_undo(&dec);
  return rc;
}

int wavelet_decode_block(BwtEngine& e, WRebuild& w, WDecoderState& dec, const u8* rec, u64 rec_bytes, u8* out, u64 cap, u32* size,
                         u64* consumed) {
  u32 n = 0;
  int rc = wavelet_decode_begin(e, w, dec, rec, rec_bytes, cap, 0, &n, consumed);
  if (rc) { w.stats.route = 0; return rc; }
  rc = wavelet_decode_end(e, w, 0, out, cap, size);
  if (rc) wdecoder_undo(&dec);
  return rc;
}

}  // namespace bwtc_hip
