// extern "C" surface of libbwtc_hip.so (include/bwtc_hip.h).
#include "bwt_engine.hpp"
#include "gpu_lanes.hpp"
#include "huffman_decoder.hpp"
#include "postprocess.hpp"
#include "wavelet_rebuild.hpp"
#include "batch_bwt.hpp"
#include "prepr_host.hpp"
#include <new>
#include "radix_sort.hpp"
#include "bwtc_hip.h"
#include "entropy_host.hpp"
#include "wavelet_host.hpp"
#include "wavelet_gpu_models.hpp"
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

using namespace bwtc_hip;

struct bwtc_hip_ctx {
  BwtEngine eng;
  bwtc_hip::HDecoder* hdec = nullptr;   // 'H' decoder, made by the first decode call
  bwtc_hip::PostProcessor* post = nullptr;   // `--prepr` postprocessor, made by the first postprocess call
  bwtc_hip::WRebuild* wreb = nullptr;        // wavelet rebuild, made by the first 'B' / 'b' / 'u' decode call
  bwtc_hip_batch_stats batch_stats = {};     // what the last batched transform did (batch_bwt.hip)
};
struct bwtc_hip_wavelet_decoder {
  bwtc_hip::WDecoderState* state;
  bwtc_hip::WrForest forest;                 // of the pure host route
};
struct bwtc_hip_grammar {
  bwtc::prepr::Grammar g;
};
namespace bwtc_hip {
int pair_replace_device(BwtEngine& e, bwtc::prepr::Grammar& grammar, const u8* d_src, u64 n, u8* d_dst, u64* n_out, u32* replaced);
int pair_stats_device(BwtEngine& e, const u8* d_src, u64 n, u32* host_counts);
}

template <typename K>
static int test_sort(bwtc_hip_ctx* ctx, K* keys, uint32_t* vals, uint64_t n, int nbits) {
  if (!ctx || !keys || !vals) return -1;
  BwtEngine& e = ctx->eng;
  if (n > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  K* k0 = static_cast<K*>(e.d_R1);
  K* k1 = static_cast<K*>(e.d_R2);
  BWTC_HIP_TRY(hipMemcpyAsync(k0, keys, n * sizeof(K), hipMemcpyHostToDevice, e.stream));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_V0, vals, n * 4, hipMemcpyHostToDevice, e.stream));
  K* ks; u32* vs;
  BWTC_HIP_TRY(hipMemsetAsync(e.d_small, 0, 1024 * 4, e.stream));
  e.sort_pairs<K>(k0, k1, e.d_V0, e.d_V1, n, nbits, &ks, &vs, false);
  BWTC_HIP_TRY(hipMemcpyAsync(keys, ks, n * sizeof(K), hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(hipMemcpyAsync(vals, vs, n * 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_small + 522, e.d_small + 522, 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  if (e.h_small[522]) return -3;
  BWTC_HIP_TRY(hipGetLastError());
  return 0;
}

// ---- test hooks of the radix sorts themselves (bwtc_hip_test_radix_*; DESIGN.md, "The sort hooks") ----------------
// radix_sort_pairs / _long / _keys_segmented called directly on the engine's buffers, three-launch scans (no ScanScope),
// no BwtEngine::sort_pairs in between.  A hook checks the sort's contract on the host before it launches anything (-1),
// makes the "producer's" first digit plane itself, and puts 256 bytes of canary behind the last item of both buffers of
// every ping-pong pair it hands over: a changed canary is -20 - (index in the order they were put).
namespace {
constexpr size_t kSortCanaryBytes = TestCanaries::kBytes;
typedef TestCanaries SortCanaries;                    // (bwt_engine.hpp; shared with the finisher's hook)

// keys: n + n_holes items in, n out; vals likewise (given values), n out (made-up values), untouched (keys only).
// values_mode as k_radix_scatter's: 0 given, 1 positions, 2 keys only, 3 descending.  planes: 0 none, 1 both, 2 both and
// the first pass's digits ready in the first.
template <typename K, typename V>
int test_radix_pairs(BwtEngine& e, K* keys, V* vals, u64 n, u64 n_holes, int bit_lo, int nbits, int values_mode, int planes) {
  const u64 n_in = n + n_holes;
  if (n == 0 || n_in < n || n_in + kSortCanaryBytes > e.cap) return -1;                  // (the planes are cap + 64 bytes)
  if (bit_lo < 0 || bit_lo > nbits || nbits > 8 * (int)sizeof(K)) return -1;
  if (values_mode < 0 || values_mode > 3 || planes < 0 || planes > 2) return -1;
  if (values_mode != 2 && !vals) return -1;
  // holes come with given values only; values are made up by the first pass, so there has to be one
  if (values_mode != 0 && n_holes) return -1;
  if (n_holes && bit_lo >= 8 * (int)sizeof(K)) return -1;                      // the compacting pass takes a digit at bit_lo
  if ((values_mode == 1 || values_mode == 3) && (n < 2 || nbits == bit_lo)) return -1;
  if (n_holes) {
    u64 ones = 0;
    for (u64 i = 0; i < n_in; ++i) ones += keys[i] == ~(K)0;
    if (ones != n_holes) return -1;
  }
  BWTC_HIP_TRY(hipSetDevice(e.device));
  hipStream_t st = e.stream;
  K* k0 = static_cast<K*>(e.d_R1);
  K* k1 = static_cast<K*>(e.d_R2);
  V* v0 = reinterpret_cast<V*>(e.d_V0);
  V* v1 = reinterpret_cast<V*>(e.d_V1);
  const bool keys_only = values_mode == 2;
  std::vector<u8> plane;
  SortCanaries can;
  // the input's buffers hold n + n_holes items, the other side never more than the n that exist
  BWTC_HIP_TRY(hipMemcpyAsync(k0, keys, n_in * sizeof(K), hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(can.put(k0, n_in * sizeof(K), st));
  BWTC_HIP_TRY(can.put(k1, n * sizeof(K), st));
  if (!keys_only) {
    if (values_mode == 0) BWTC_HIP_TRY(hipMemcpyAsync(v0, vals, n_in * sizeof(V), hipMemcpyHostToDevice, st));
    else BWTC_HIP_TRY(hipMemsetAsync(v0, 0xA5, n_in * sizeof(V), st));          // "v0 need not be filled"
    BWTC_HIP_TRY(can.put(v0, n_in * sizeof(V), st));
    BWTC_HIP_TRY(can.put(v1, n * sizeof(V), st));
  }
  if (planes) {
    if (planes == 2) {
      // the first pass's digit rule: radix_digit(key, bit_lo), one byte per slot of the input
      plane.resize(n_in);
      for (u64 i = 0; i < n_in; ++i) plane[i] = (u8)((keys[i] >> (bit_lo < 8 * (int)sizeof(K) ? bit_lo : 0)) & 255u);
      BWTC_HIP_TRY(hipMemcpyAsync(e.d_P0, plane.data(), n_in, hipMemcpyHostToDevice, st));
    } else {
      BWTC_HIP_TRY(hipMemsetAsync(e.d_P0, 0x5A, n_in, st));                     // a plane nobody may read
    }
    BWTC_HIP_TRY(can.put(e.d_P0, n_in, st));
    BWTC_HIP_TRY(can.put(e.d_P1, n, st));
  }
  K* ks = nullptr; V* vs = nullptr;
  radix_sort_pairs<K, V>(k0, k1, keys_only ? (V*)nullptr : v0, keys_only ? (V*)nullptr : v1, n, nbits, e.d_table, e.d_partial, st, &ks, &vs,
                         nullptr, bit_lo, values_mode == 1, keys_only, n_holes, planes ? e.d_P0 : nullptr, planes ? e.d_P1 : nullptr,
                         planes == 2, values_mode == 3);
  BWTC_HIP_TRY(hipMemcpyAsync(keys, ks, n * sizeof(K), hipMemcpyDeviceToHost, st));
  if (!keys_only) BWTC_HIP_TRY(hipMemcpyAsync(vals, vs, n * sizeof(V), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

// keys, w: n items in and out; vals: n out (the first pass makes them up: item i's value is n - 1 - i).
template <typename V, int EL>
int test_radix_long(BwtEngine& e, u64* keys, V* vals, u32* w, u64 n, int kbits, int wbits, bool direct_w) {
  if (n < 2 || n + kSortCanaryBytes > e.cap) return -1;                        // made-up values: there has to be a pass
  if (kbits < 1 || kbits > 64 || wbits < 1 || wbits > 32) return -1;
  if (wbits < 32) for (u64 i = 0; i < n; ++i) if (w[i] >> wbits) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  hipStream_t st = e.stream;
  u64* k0 = static_cast<u64*>(e.d_R1);
  u64* k1 = static_cast<u64*>(e.d_R2);
  V* v0 = reinterpret_cast<V*>(e.d_V0);
  V* v1 = reinterpret_cast<V*>(e.d_V1);
  // the first pass's digit rule (radix_sort_long's pass plan): w's lowest digit, or -- w shorter than a digit -- the
  // bridge digit: w's wbits bits under the key's lowest, cut to min(8, wbits + kbits) bits
  std::vector<u8> plane(n);
  if (wbits >= kRadixBits) {
    for (u64 i = 0; i < n; ++i) plane[i] = (u8)(w[i] & 255u);
  } else {
    const u32 dmask = (1u << std::min(kRadixBits, wbits + kbits)) - 1u;
    for (u64 i = 0; i < n; ++i) plane[i] = (u8)((w[i] | ((u32)keys[i] << wbits)) & dmask);
  }
  SortCanaries can;
  BWTC_HIP_TRY(hipMemcpyAsync(k0, keys, n * 8, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_W0, w, n * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_P0, plane.data(), n, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemsetAsync(v0, 0xA5, n * sizeof(V), st));
  BWTC_HIP_TRY(can.put(k0, n * 8, st));
  BWTC_HIP_TRY(can.put(k1, n * 8, st));
  BWTC_HIP_TRY(can.put(v0, n * sizeof(V), st));
  BWTC_HIP_TRY(can.put(v1, n * sizeof(V), st));
  BWTC_HIP_TRY(can.put(e.d_W0, n * 4, st));
  BWTC_HIP_TRY(can.put(e.d_W1, n * 4, st));
  BWTC_HIP_TRY(can.put(e.d_P0, n, st));
  BWTC_HIP_TRY(can.put(e.d_P1, n, st));
  u64* ks = nullptr; V* vs = nullptr; u32* ws = nullptr;
  radix_sort_long<V, EL>(k0, k1, v0, v1, e.d_W0, e.d_W1, n, kbits, wbits, e.d_table, e.d_partial, st, &ks, &vs, &ws, nullptr,
                         e.d_P0, e.d_P1, 0, false, direct_w);
  BWTC_HIP_TRY(hipMemcpyAsync(keys, ks, n * 8, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(vals, vs, n * sizeof(V), hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(w, ws, n * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}
}  // namespace

// how every buffer handed out by bwtc_hip_host_alloc was locked (see lockedHostAlloc)
static std::mutex& host_allocs_mu() { static std::mutex m; return m; }
static std::map<void*, std::pair<int, uint64_t> >& host_allocs() { static std::map<void*, std::pair<int, uint64_t> > m; return m; }

// bwtc_hip_copy_probe: a streaming copy, one 16-byte item per thread.  (Of the forms tried on MI355X -- grid-stride
// loops with 4 or 8 loads in flight, contiguous chunks per workgroup, non-temporal accesses, hipMemcpy device to
// device: 4.1-5.5 TB/s -- this plain one is the fastest, 6.2 TB/s: scripts/dev/copy_probe.cpp.)
static __global__ __launch_bounds__(256) void k_copy_probe(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t n16) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

extern "C" {

int bwtc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* bwtc_hip_version(void) { return "bwtc_hip 0.1 (gfx950)"; }

uint64_t bwtc_hip_workspace_bytes(uint32_t max_block_size) {
  return BwtEngine::workspace_bytes(max_block_size);
}

int bwtc_hip_create(int device, uint32_t max_block_size, bwtc_hip_ctx** ctx_out) {
  if (!ctx_out) return -1;
  *ctx_out = nullptr;
  if (max_block_size >= 0x7FFFFFFEu) return -1;   // PrecompressorBlock.cpp:126
  bwtc_hip_ctx* c = new (std::nothrow) bwtc_hip_ctx();
  if (!c) return -2;
  for (int i = 0; i < BwtEngine::kMaxSortEvents; ++i) c->eng.ev_sort[i] = nullptr;
  int rc = c->eng.init(device, max_block_size);
  if (rc != 0) { c->eng.release(); delete c; return rc; }
  *ctx_out = c;
  return 0;
}

void bwtc_hip_destroy(bwtc_hip_ctx* ctx) {
  if (!ctx) return;
  bwtc_hip::hdecoder_destroy(ctx->hdec);
  bwtc_hip::postprocessor_destroy(ctx->post);
  bwtc_hip::wrebuild_destroy(ctx->wreb);
  ctx->eng.release();
  delete ctx;
}

void* bwtc_hip_stream(bwtc_hip_ctx* ctx) { return ctx ? (void*)ctx->eng.stream : nullptr; }

int bwtc_hip_get_stats(bwtc_hip_ctx* ctx, bwtc_hip_stats* out) {
  if (!ctx || !out) return -1;
  *out = ctx->eng.stats;
  return 0;
}

int bwtc_hip_set_profiling(bwtc_hip_ctx* ctx, int on) {
  if (!ctx) return -1;
  ctx->eng.probe.enabled = on != 0;
  return 0;
}

int bwtc_hip_get_kernel_timers(bwtc_hip_ctx* ctx, bwtc_hip_kernel_timers* out, int reset) {
  if (!ctx) return -1;
  ScatterProbe& p = ctx->eng.probe;
  if (out) { out->scatter_launches = p.total_launches; out->scatter_bytes = p.total_bytes; out->scatter_ms = p.total_ms; }
  if (reset) { p.total_launches = 0; p.total_bytes = 0; p.total_ms = 0.0; }
  return 0;
}

int bwtc_hip_copy_probe(bwtc_hip_ctx* ctx, uint64_t bytes, int reps, double* gbps) {
  if (!ctx || !gbps || bytes < 16 || reps < 1) return -1;
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  void *a = nullptr, *b = nullptr;
  if (hipMalloc(&a, bytes) != hipSuccess) return -2;
  if (hipMalloc(&b, bytes) != hipSuccess) { (void)hipFree(a); return -2; }
  hipStream_t st = ctx->eng.stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = 0;
  float ms = 0.f;
  const uint64_t n16 = bytes / 16;
  if (hipMemsetAsync(a, 1, bytes, st) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = -3;
  if (!rc) {
    const dim3 grid((unsigned)((n16 + 255) / 256));
    hipLaunchKernelGGL(k_copy_probe, grid, dim3(256), 0, st, (const uint4*)a, (uint4*)b, n16);      // warm
    (void)hipEventRecord(e0, st);
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_copy_probe, grid, dim3(256), 0, st, (const uint4*)a, (uint4*)b, n16);
    (void)hipEventRecord(e1, st);
    if (hipStreamSynchronize(st) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.f) rc = -3;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(a); (void)hipFree(b);
  if (rc) { (void)hipGetLastError(); return rc; }
  *gbps = (double)reps * 2.0 * (double)(n16 * 16) / ((double)ms * 1e-3) / 1e9;
  return 0;
}

void* bwtc_hip_malloc(bwtc_hip_ctx* ctx, uint64_t bytes) {
  if (!ctx || hipSetDevice(ctx->eng.device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
  return p;
}
void bwtc_hip_free(bwtc_hip_ctx* ctx, void* d_ptr) {
  if (ctx && d_ptr && hipSetDevice(ctx->eng.device) == hipSuccess) (void)hipFree(d_ptr);
}
int bwtc_hip_memcpy_to_device(bwtc_hip_ctx* ctx, void* d_dst, const void* src, uint64_t bytes) {
  if (!ctx || (!d_dst && bytes) || (!src && bytes)) return -1;
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  if (bytes) BWTC_HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
int bwtc_hip_memcpy_to_host(bwtc_hip_ctx* ctx, void* dst, const void* d_src, uint64_t bytes) {
  if (!ctx || (!dst && bytes) || (!d_src && bytes)) return -1;
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  if (bytes) BWTC_HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
  return 0;
}

void* bwtc_hip_host_alloc(bwtc_hip_ctx* ctx, uint64_t bytes) {
  if (!ctx || hipSetDevice(ctx->eng.device) != hipSuccess) return nullptr;
  int kind = 0;
  void* p = bwtc_hip::lockedHostAlloc(bytes ? bytes : 1, &kind);
  if (!p) return nullptr;
  std::lock_guard<std::mutex> g(host_allocs_mu());
  host_allocs()[p] = std::make_pair(kind, bytes ? bytes : 1);
  return p;
}
void bwtc_hip_host_free(bwtc_hip_ctx* ctx, void* p) {
  if (!ctx || !p || hipSetDevice(ctx->eng.device) != hipSuccess) return;
  std::pair<int, uint64_t> how;
  {
    std::lock_guard<std::mutex> g(host_allocs_mu());
    std::map<void*, std::pair<int, uint64_t> >::iterator it = host_allocs().find(p);
    if (it == host_allocs().end()) return;          // not one of ours
    how = it->second;
    host_allocs().erase(it);
  }
  bwtc_hip::lockedHostFree(p, how.first, static_cast<size_t>(how.second));
}
int bwtc_hip_memcpy_to_device_async(bwtc_hip_ctx* ctx, void* d_dst, const void* src, uint64_t bytes) {
  if (!ctx || (!d_dst && bytes) || (!src && bytes)) return -1;
  BwtEngine& e = ctx->eng;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  if (!e.copy_stream) {
    BWTC_HIP_TRY(hipStreamCreateWithFlags(&e.copy_stream, hipStreamNonBlocking));
    BWTC_HIP_TRY(hipEventCreateWithFlags(&e.ev_copy, hipEventBlockingSync | hipEventDisableTiming));
  }
  if (bytes) BWTC_HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, e.copy_stream));
  return 0;
}
int bwtc_hip_copy_wait(bwtc_hip_ctx* ctx) {
  if (!ctx) return -1;
  BwtEngine& e = ctx->eng;
  if (!e.copy_stream) return 0;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipEventRecord(e.ev_copy, e.copy_stream));
  if (e.pipeline) BWTC_HIP_TRY(e.sleepy_wait(e.ev_copy, BwtEngine::kWaitSlots - 2));     // the 'B' workers need the CPU
  else BWTC_HIP_TRY(hipEventSynchronize(e.ev_copy));
  return 0;
}

uint32_t bwtc_hip_n_lf(uint32_t size, uint32_t starting_points) {
  if (starting_points < 1) starting_points = 1;          // BWTManager.cpp:60-64
  else if (starting_points > 256) starting_points = 256;
  if (size <= 256) return 1;                             // BWTBlock.cpp:104-108
  return starting_points;
}

static int stage_in(BwtEngine& e, const uint8_t* host, uint32_t bytes) {
  if (!bytes) return 0;
  std::memcpy(e.h_stage, host, bytes);
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, e.h_stage, bytes, hipMemcpyHostToDevice, e.stream));
  return 0;
}
static int stage_out(BwtEngine& e, uint8_t* host, uint32_t bytes) {
  if (!bytes) return 0;
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_stage, e.d_in, bytes, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  std::memcpy(host, e.h_stage, bytes);
  return 0;
}

int bwtc_hip_bwt(bwtc_hip_ctx* ctx, uint8_t* T, uint32_t length, uint32_t* lf, uint32_t n_lf,
                 uint32_t* freqs) {
  if (!ctx || !T || !lf || n_lf == 0) return -1;
  if (length <= 1) return 0;                             // divsufsort.c:489
  BwtEngine& e = ctx->eng;
  if ((u64)length > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  int rc = stage_in(e, T, length);
  if (rc) return rc;
  rc = e.transform(e.d_in, e.d_in, length, true, lf, n_lf, freqs);
  if (rc) return rc;
  return stage_out(e, T, length);
}

int bwtc_hip_bwt_block(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size, uint32_t* lf,
                       uint32_t n_lf, uint32_t* freqs) {
  if (!ctx || (!block && size) || !lf || n_lf == 0) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  int rc = stage_in(e, block, size);
  if (rc) return rc;
  rc = e.transform(e.d_in, e.d_in, size, false, lf, n_lf, freqs);
  if (rc) return rc;
  return stage_out(e, block, size);
}

int bwtc_hip_bwt_block_device(bwtc_hip_ctx* ctx, const uint8_t* d_in, uint8_t* d_out,
                              uint32_t size, uint32_t* lf, uint32_t n_lf, uint32_t* freqs) {
  if (!ctx || ((!d_in || !d_out) && size) || !lf || n_lf == 0) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  return e.transform(d_in, d_out, size, false, lf, n_lf, freqs);
}

// ---- batched block transform (batch_bwt.hip) ----
int bwtc_hip_bwt_blocks(bwtc_hip_ctx* ctx, uint8_t* data, const bwtc_hip_batch_item* items, uint32_t k,
                        uint32_t* lf, uint32_t* freqs) {
  if (!ctx) return -1;
  return batch_transform_host(ctx->eng, data, items, k, lf, freqs, &ctx->batch_stats);
}
int bwtc_hip_bwt_blocks_device(bwtc_hip_ctx* ctx, const uint8_t* d_in, uint8_t* d_out,
                               const bwtc_hip_batch_item* items, uint32_t k, uint32_t* lf, uint32_t* freqs) {
  if (!ctx) return -1;
  return batch_transform_device(ctx->eng, d_in, d_out, items, k, lf, freqs, &ctx->batch_stats);
}
int bwtc_hip_batch_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_batch_stats* out) {
  if (!ctx || !out) return -1;
  *out = ctx->batch_stats;
  return 0;
}
int bwtc_hip_test_batch_keys(bwtc_hip_ctx* ctx, const uint8_t* data, const bwtc_hip_batch_item* items, uint32_t k,
                             uint8_t* T_out, uint64_t* keys_out, uint32_t* freqs_out) {
  if (!ctx) return -1;
  return batch_test_keys(ctx->eng, data, items, k, T_out, keys_out, freqs_out);
}

int bwtc_hip_inverse_bwt_block(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size,
                               const uint32_t* lf, uint32_t n_lf) {
  if (!ctx || (!block && size) || !lf || n_lf == 0) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  if (size == 0) return 0;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  int rc = stage_in(e, block, size);
  if (rc) return rc;
  rc = inverse_bwt_device(e, e.d_in, e.d_in, size, lf, n_lf);
  if (rc) return rc;
  return stage_out(e, block, size);
}

int bwtc_hip_inverse_bwt_block_device(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint8_t* d_out,
                                      uint32_t size, const uint32_t* lf, uint32_t n_lf) {
  if (!ctx || ((!d_bwt || !d_out) && size) || !lf || n_lf == 0) return -1;
  if (size > ctx->eng.max_block) return -1;
  return inverse_bwt_device(ctx->eng, d_bwt, d_out, size, lf, n_lf);
}

uint64_t bwtc_hip_compress_bound(uint32_t size) { return huffman_compress_bound(size); }

// ---- 'H' decoding (HuffmanCoders.cpp:324-616, InverseBWT.cpp:47-51) ----
static HDecoder* hdecoder(bwtc_hip_ctx* ctx) {
  if (!ctx->hdec) ctx->hdec = hdecoder_create();
  return ctx->hdec;
}

int bwtc_hip_huffman_decode(bwtc_hip_ctx* ctx, const uint8_t* rec, uint64_t rec_bytes, uint8_t* bwt_out,
                            uint64_t cap, uint32_t* lf_out, uint32_t* n_lf, uint32_t* size, uint64_t* consumed) {
  if (!ctx || !rec || (!bwt_out && cap) || !lf_out || !n_lf || !size || !consumed) return -1;
  HDecoder* d = hdecoder(ctx);
  if (!d) return -2;
  BwtEngine& e = ctx->eng;
  int rc = huffman_decode(e, *d, rec, nullptr, rec_bytes, nullptr, cap, lf_out, n_lf, size, consumed);
  if (rc) return rc;
  if (*size) {
    BWTC_HIP_TRY(hipMemcpyAsync(bwt_out, hdecoder_bwt_buffer(d), *size, hipMemcpyDeviceToHost, e.stream));
    BWTC_HIP_TRY(e.wait());
  }
  return 0;
}

int bwtc_hip_huffman_decode_device(bwtc_hip_ctx* ctx, const uint8_t* d_rec, uint64_t rec_bytes, uint8_t* d_bwt_out,
                                   uint64_t cap, uint32_t* lf_out, uint32_t* n_lf, uint32_t* size, uint64_t* consumed) {
  if (!ctx || !d_rec || (!d_bwt_out && cap) || !lf_out || !n_lf || !size || !consumed) return -1;
  HDecoder* d = hdecoder(ctx);
  if (!d) return -2;
  BwtEngine& e = ctx->eng;
  // header and code shapes are parsed on the host: bring the record down (the 48-bit length says
  // how much of the buffer it is)
  BWTC_HIP_TRY(hipSetDevice(e.device));
  uint8_t head[6] = {0};
  const uint64_t nh = rec_bytes < 6 ? rec_bytes : 6;
  if (nh) BWTC_HIP_TRY(hipMemcpy(head, d_rec, nh, hipMemcpyDeviceToHost));
  uint64_t len = 0;
  for (int i = 0; i < 6; ++i) len = (len << 8) | head[i];
  const uint64_t rec_end = nh < 6 ? nh : std::min<uint64_t>(rec_bytes, 6 + len);
  std::vector<uint8_t> host(rec_end);
  if (rec_end) BWTC_HIP_TRY(hipMemcpyAsync(host.data(), d_rec, rec_end, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  return huffman_decode(e, *d, host.data(), d_rec, rec_bytes, d_bwt_out, cap, lf_out, n_lf, size, consumed);
}

int bwtc_hip_decode_block_H(bwtc_hip_ctx* ctx, const uint8_t* rec, uint64_t rec_bytes, uint8_t* out, uint64_t cap,
                            uint32_t* size, uint64_t* consumed) {
  if (!ctx || !rec || (!out && cap) || !size || !consumed) return -1;
  HDecoder* d = hdecoder(ctx);
  if (!d) return -2;
  return huffman_decode_block(ctx->eng, *d, rec, rec_bytes, out, cap, size, consumed);
}

int bwtc_hip_decode_block_H_device(bwtc_hip_ctx* ctx, const uint8_t* rec, uint64_t rec_bytes, uint8_t* d_out, uint64_t cap,
                                   uint32_t* size, uint64_t* consumed) {
  if (!ctx || !rec || (!d_out && cap) || !size || !consumed) return -1;
  HDecoder* d = hdecoder(ctx);
  if (!d) return -2;
  return huffman_decode_block_device(ctx->eng, *d, rec, rec_bytes, d_out, cap, size, consumed);
}

int bwtc_hip_huffman_decode_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_huffman_decode_stats* out) {
  if (!ctx || !out) return -1;
  return hdecoder_stats(ctx->hdec, out);
}

// ---- 'B' / 'b' / 'u' decoding: host range decoder + wavelet rebuild (wavelet_rebuild.hip) ----
static WRebuild* wrebuild(bwtc_hip_ctx* ctx) {
  if (!ctx->wreb) ctx->wreb = wrebuild_create();
  return ctx->wreb;
}

bwtc_hip_wavelet_decoder* bwtc_hip_wavelet_decoder_create(char coder) {
  WDecoderState* s = wdecoder_create(coder);
  if (!s) return nullptr;
  bwtc_hip_wavelet_decoder* d = new (std::nothrow) bwtc_hip_wavelet_decoder();
  if (!d) { wdecoder_destroy(s); return nullptr; }
  d->state = s;
  return d;
}
void bwtc_hip_wavelet_decoder_destroy(bwtc_hip_wavelet_decoder* d) {
  if (!d) return;
  wdecoder_destroy(d->state);
  d->forest.words.drop();
  delete d;
}
void bwtc_hip_wavelet_decoder_reset(bwtc_hip_wavelet_decoder* d) { if (d) wdecoder_reset(d->state); }

int bwtc_hip_decode_block_W(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes, uint8_t* out,
                            uint64_t cap, uint32_t* size, uint64_t* consumed) {
  if (!ctx || !dec || !rec || (!out && cap) || !size || !consumed) return -1;
  WRebuild* w = wrebuild(ctx);
  if (!w) return -2;
  return wavelet_decode_block(ctx->eng, *w, *dec->state, rec, rec_bytes, out, cap, size, consumed);
}

int bwtc_hip_decode_block_W_device(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes,
                                   uint8_t* d_out, uint64_t cap, uint32_t* size, uint64_t* consumed) {
  if (!ctx || !dec || !rec || (!d_out && cap) || !size || !consumed) return -1;
  WRebuild* w = wrebuild(ctx);
  if (!w) return -2;
  return wavelet_decode_block_device(ctx->eng, *w, *dec->state, rec, rec_bytes, d_out, cap, size, consumed);
}

int bwtc_hip_decode_block_W_begin(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes, uint64_t cap,
                                  uint32_t slot, uint32_t* size, uint64_t* consumed) {
  if (!ctx || !dec || !rec || slot >= kWrSlots || !size || !consumed) return -1;
  WRebuild* w = wrebuild(ctx);
  if (!w) return -2;
  return wavelet_decode_begin(ctx->eng, *w, *dec->state, rec, rec_bytes, cap, slot, size, consumed);
}

int bwtc_hip_decode_block_W_end(bwtc_hip_ctx* ctx, uint32_t slot, uint8_t* out, uint64_t cap, uint32_t* size) {
  if (!ctx || !ctx->wreb || slot >= kWrSlots || (!out && cap) || !size) return -1;
  return wavelet_decode_end(ctx->eng, *ctx->wreb, slot, out, cap, size);
}

int bwtc_hip_decode_block_W_end_device(bwtc_hip_ctx* ctx, uint32_t slot, uint8_t* d_out, uint64_t cap, uint32_t* size) {
  if (!ctx || !ctx->wreb || slot >= kWrSlots || (!d_out && cap) || !size) return -1;
  return wavelet_decode_end_device(ctx->eng, *ctx->wreb, slot, d_out, cap, size);
}

int bwtc_hip_wavelet_decode_bwt_host(bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes, uint8_t* bwt_out,
                                     uint64_t cap, uint32_t* lf_out, uint32_t* n_lf, uint32_t* size, uint64_t* consumed) {
  if (!dec || !rec || (!bwt_out && cap) || !lf_out || !n_lf || !size || !consumed) return -1;
  int rc = wavelet_range_decode(*dec->state, rec, rec_bytes, cap, dec->forest, consumed);
  if (rc) return rc;
  uint64_t total = 0;
  try { rc = host_wavelet_rebuild(dec->forest.view(), bwt_out, cap, &total, 8, nullptr); }
  catch (const std::bad_alloc&) { rc = -2; }
  if (rc) { wdecoder_undo(dec->state); return rc; }
  for (uint32_t i = 0; i < dec->forest.n_lf; ++i) lf_out[i] = dec->forest.lf[i];
  *n_lf = dec->forest.n_lf;
  *size = (uint32_t)total;
  return 0;
}

int bwtc_hip_wavelet_decode_counts(bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes, uint64_t cap,
                                   uint64_t* counts, uint64_t* consumed) {
  if (!dec || !rec || !counts || !consumed) return -1;
  const int rc = wavelet_range_decode(*dec->state, rec, rec_bytes, cap, dec->forest, consumed);
  if (rc) return rc;
  counts[0] = dec->forest.sections.size(); counts[1] = dec->forest.runs; counts[2] = dec->forest.nodes.size();
  counts[3] = dec->forest.n_words; counts[4] = dec->forest.bytes;
  // bits the run walks take: the host twin counts them (it writes the block into a scratch buffer)
  try {
    std::vector<uint8_t> scratch(dec->forest.bytes + 1);
    uint64_t total = 0;
    return host_wavelet_rebuild(dec->forest.view(), scratch.data(), dec->forest.bytes, &total, 8, &counts[5]);
  } catch (const std::bad_alloc&) { return -2; }
}

int bwtc_hip_wavelet_decoder_forest(bwtc_hip_wavelet_decoder* dec, bwtc_hip_wforest* out, uint32_t* lf_out, uint32_t* n_lf) {
  if (!dec || !out) return -1;
  *out = dec->forest.view();
  if (lf_out && n_lf) {
    for (uint32_t i = 0; i < dec->forest.n_lf; ++i) lf_out[i] = dec->forest.lf[i];
    *n_lf = dec->forest.n_lf;
  }
  return 0;
}

int bwtc_hip_wavelet_rebuild_device(bwtc_hip_ctx* ctx, const bwtc_hip_wforest* forest, uint8_t* d_out, uint64_t cap, uint64_t* size) {
  if (!ctx || !forest || (!d_out && cap) || !size) return -1;
  WRebuild* w = wrebuild(ctx);
  if (!w) return -2;
  return wavelet_rebuild_device(ctx->eng, *w, *forest, d_out, cap, size, nullptr);
}

int bwtc_hip_wavelet_rebuild(bwtc_hip_ctx* ctx, const bwtc_hip_wforest* forest, uint8_t* out, uint64_t cap, uint64_t* size) {
  if (!ctx || !forest || (!out && cap) || !size) return -1;
  WRebuild* w = wrebuild(ctx);
  if (!w) return -2;
  uint8_t* d_bwt = nullptr;
  const int rc = wavelet_rebuild_device(ctx->eng, *w, *forest, nullptr, cap, size, &d_bwt);
  if (rc) return rc;
  if (*size) BWTC_HIP_TRY(hipMemcpy(out, d_bwt, *size, hipMemcpyDeviceToHost));
  return 0;
}

int bwtc_hip_host_wavelet_rebuild(const bwtc_hip_wforest* forest, uint8_t* out, uint64_t cap, uint64_t* size, uint32_t line_words,
                                  uint64_t* bit_reads) {
  if (!forest || (!out && cap) || !size || line_words == 0) return -1;
  return host_wavelet_rebuild(*forest, out, cap, size, line_words, bit_reads);
}

int bwtc_hip_wavelet_decode_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decode_stats* out) {
  if (!ctx || !out) return -1;
  return wrebuild_stats(ctx->wreb, out);
}

int bwtc_hip_huffman_encode_device(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                   const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                   uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (!d_bwt && size) || !d_out || !lf || !freqs || !out_bytes) return -1;
  if (size > ctx->eng.max_block) return -1;
  return huffman_encode_device(ctx->eng, d_bwt, size, lf, n_lf, freqs, d_out, out_cap, out_bytes);
}

int bwtc_hip_huffman_encode(bwtc_hip_ctx* ctx, const uint8_t* bwt, uint32_t size,
                            const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (!bwt && size) || !out || !lf || !freqs || !out_bytes) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  int rc = stage_in(e, bwt, size);
  if (rc) return rc;
  u64 n = 0;
  rc = huffman_encode_device(e, e.d_in, size, lf, n_lf, freqs, e.d_comp,
                             huffman_compress_bound(e.cap), &n);
  if (rc) return rc;
  if (n > out_cap) return -1;
  BWTC_HIP_TRY(hipMemcpyAsync(out, e.d_comp, n, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  *out_bytes = n;
  return 0;
}

int bwtc_hip_transform_and_encode(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size,
                                  uint32_t starting_points, uint8_t* out, uint64_t out_cap,
                                  uint64_t* out_bytes) {
  if (!ctx || (!block && size) || !out || !out_bytes) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  uint32_t lf[256];
  uint32_t freqs[256];
  std::memset(freqs, 0, sizeof freqs);                    // HuffmanCoders.cpp:53
  const uint32_t n_lf = bwtc_hip_n_lf(size, starting_points);
  int rc = stage_in(e, block, size);
  if (rc) return rc;
  rc = e.transform(e.d_in, e.d_in, size, false, lf, n_lf, freqs);
  if (rc) return rc;
  u64 n = 0;
  rc = huffman_encode_device(e, e.d_in, size, lf, n_lf, freqs, e.d_comp,
                             huffman_compress_bound(e.cap), &n);
  if (rc) return rc;
  if (n > out_cap) return -1;
  BWTC_HIP_TRY(hipMemcpyAsync(out, e.d_comp, n, hipMemcpyDeviceToHost, e.stream));
  rc = stage_out(e, block, size);
  if (rc) return rc;
  *out_bytes = n;
  return 0;
}

int bwtc_hip_wavelet_section_stats(bwtc_hip_ctx* ctx, const uint8_t* bwt, uint32_t size,
                                   const uint32_t* freqs, uint32_t* n_sections,
                                   uint32_t* section_len, uint32_t* run_freqs,
                                   uint64_t* total_runs, uint32_t* dist_offset,
                                   uint32_t* dist_len, uint32_t* dist_cnt, uint32_t dist_cap) {
  if (!ctx || (!bwt && size) || !freqs || !n_sections || !section_len || !run_freqs ||
      !total_runs || !dist_offset || !dist_len || !dist_cnt) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  int rc = stage_in(e, bwt, size);
  if (rc) return rc;
  WaveletSectionStats st;
  rc = wavelet_section_stats_device(e, e.d_in, size, freqs, &st);
  if (rc) return rc;
  const uint32_t nsec = (uint32_t)st.sections.size();
  *n_sections = nsec;
  uint32_t at = 0;
  for (uint32_t s = 0; s < nsec; ++s) {
    section_len[s] = st.sections[s];
    total_runs[s] = st.total_runs[s];
    std::memcpy(run_freqs + (size_t)s * 256, &st.run_freqs[(size_t)s * 256], 1024);
    dist_offset[s] = at;
    if ((uint64_t)at + st.dist[s].size() > dist_cap) return -1;
    for (size_t i = 0; i < st.dist[s].size(); ++i) { dist_len[at] = st.dist[s][i].first; dist_cnt[at] = st.dist[s][i].second; ++at; }
  }
  dist_offset[nsec] = at;
  return 0;
}

// CPUs this process may keep busy: the hardware threads, cut down to the cgroup's CPU quota
// (a container with a quota is throttled as a whole, the GPU-feeding thread included, when
// more threads than that run).
static unsigned usable_cpus() {
  unsigned n = std::thread::hardware_concurrency();
  if (n == 0) n = 1;
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char quota[32] = {0};
    unsigned long period = 0;
    if (std::fscanf(f, "%31s %lu", quota, &period) == 2 && period > 0 && std::strcmp(quota, "max") != 0) {
      const unsigned long q = std::strtoul(quota, nullptr, 10);
      if (q > 0) n = std::min<unsigned long>(n, std::max<unsigned long>(1, q / period));
    }
    std::fclose(f);
  }
  return n;
}

uint32_t bwtc_hip_host_usable_cpus(void) { return usable_cpus(); }

static unsigned pick_threads(uint32_t threads) {
  if (threads) return threads;
  // all of them: the thread that feeds the GPU sleeps while it waits (BwtEngine::wait), and what
  // it computes between waits is a tenth of a CPU
  return std::min(usable_cpus(), 64u);
}

int bwtc_hip_wavelet_start(bwtc_hip_ctx* ctx, char coder) {
  if (!ctx || !bwtc::wavelet::isWaveletModel(coder)) return -1;
  // blocks begun with _begin that have not joined their stream yet belong to the OLD stream:
  // they join it now, with its state and its model, before either changes
  const int rc = wavelet_join_begun(ctx->eng);
  // whatever became of the old stream's blocks (a failed join is reported, and their _end reports it again), the
  // NEW stream starts from the fresh state: never the old stream's carried state under a new header
  ctx->eng.wavelet_state = 4;
  ctx->eng.wavelet_model = coder;
  ctx->eng.stream_start_error = 0;                    // the caller has the code: the new stream starts clean
  return rc;
}
void bwtc_hip_wavelet_reset(bwtc_hip_ctx* ctx) {      // no result of its own: a failure is kept, the next _begin / _prepare returns it
  const int rc = bwtc_hip_wavelet_start(ctx, 'B');
  if (ctx) ctx->eng.stream_start_error = rc;
}
uint32_t bwtc_hip_wavelet_depth(bwtc_hip_ctx* ctx) { return ctx ? ctx->eng.max_inflight : 0u; }
int bwtc_hip_wavelet_set_depth(bwtc_hip_ctx* ctx, uint32_t depth) {
  if (!ctx || depth == 0) return -1;
  BwtEngine& e = ctx->eng;
  if (e.jobs.size() > depth) return -6;                     // more blocks under way than the new depth allows: collect first
  e.max_inflight = depth;
  // page-locked staging follows the need: what the pools hold beyond the blocks that can still be begun goes back
  const size_t spare = depth + 2 > e.jobs.size() ? depth + 2 - e.jobs.size() : 0;
  e.codes_pool.trim(spare);
  e.w_pool.trim(spare);
  return 0;
}
uint32_t bwtc_hip_wavelet_depth_needed(bwtc_hip_ctx* ctx) { return ctx && ctx->eng.pipeline ? ctx->eng.pipeline->depthNeeded() : 0u; }
int bwtc_hip_wavelet_host_clock(bwtc_hip_ctx* ctx, double* model_seconds, double* coder_seconds, uint64_t* blocks) {
  if (!ctx) return -1;
  const HostPipeline* p = ctx->eng.pipeline;
  if (model_seconds) *model_seconds = p ? p->clock.model_ns.load() * 1e-9 : 0.0;
  if (coder_seconds) *coder_seconds = p ? p->clock.coder_ns.load() * 1e-9 : 0.0;
  if (blocks) *blocks = p ? p->clock.blocks.load() : 0;
  return 0;
}

int bwtc_hip_numa_node(bwtc_hip_ctx* ctx) {
  if (!ctx) return -1;
  char id[64] = {0};
  if (hipDeviceGetPCIBusId(id, sizeof id, ctx->eng.device) != hipSuccess) { (void)hipGetLastError(); return -1; }
  for (char* p = id; *p; ++p) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');     // sysfs spells the id in lower case
  const std::string path = std::string("/sys/bus/pci/devices/") + id + "/numa_node";
  int node = -1;
  if (FILE* f = std::fopen(path.c_str(), "r")) { if (std::fscanf(f, "%d", &node) != 1) node = -1; std::fclose(f); }
  return node;
}

int bwtc_hip_host_cpu_slice(int numa_node, uint32_t rank, uint32_t ranks, uint32_t* cpus, uint32_t cap) {
  if (!cpus || ranks == 0 || rank >= ranks) return -1;
  cpu_set_t mine;
  CPU_ZERO(&mine);
  if (sched_getaffinity(0, sizeof mine, &mine) != 0) return -1;
  std::vector<uint32_t> usable;
  for (int c = 0; c < CPU_SETSIZE; ++c) if (CPU_ISSET(c, &mine)) usable.push_back((uint32_t)c);
  if (numa_node >= 0) {
    // "0-15,128-143" -> the node's CPUs; kept only if some of them are ours
    char path[96];
    std::snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", numa_node);
    // BWTC_HIP_NODE<k>_CPULIST=<file>: a made-up topology (tests of the farm's slicing on boxes with one node)
    char var[48];
    std::snprintf(var, sizeof var, "BWTC_HIP_NODE%d_CPULIST", numa_node);
    const char* fake = std::getenv(var);
    std::vector<uint32_t> on_node;
    if (FILE* f = std::fopen(fake ? fake : path, "r")) {
      unsigned a = 0, b = 0;
      for (;;) {
        if (std::fscanf(f, "%u", &a) != 1) break;
        b = a;
        int ch = std::fgetc(f);
        if (ch == '-') { if (std::fscanf(f, "%u", &b) != 1) break; ch = std::fgetc(f); }
        for (unsigned c = a; c <= b && c < (unsigned)CPU_SETSIZE; ++c) if (CPU_ISSET(c, &mine)) on_node.push_back(c);
        if (ch != ',') break;
      }
      std::fclose(f);
    }
    if (!on_node.empty()) usable.swap(on_node);
  }
  const size_t n = usable.size(), b = n * rank / ranks, e = n * (rank + 1) / ranks;
  uint32_t k = 0;
  for (size_t i = b; i < e && k < cap; ++i) cpus[k++] = usable[i];
  return (int)k;
}

int bwtc_hip_set_worker_cpus(bwtc_hip_ctx* ctx, const uint32_t* cpus, uint32_t n) {
  if (!ctx || (n && !cpus)) return -1;
  ctx->eng.worker_cpus.assign(cpus, cpus + n);
  if (ctx->eng.pipeline) ctx->eng.pipeline->setWorkerCpus(ctx->eng.worker_cpus);
  return 0;
}

int bwtc_hip_wavelet_host_progress(bwtc_hip_ctx* ctx, uint64_t* queued, uint64_t* finished) {
  if (!ctx) return -1;
  const HostPipeline* p = ctx->eng.pipeline;
  if (queued) *queued = p ? p->clock.blocks.load() : 0;
  if (finished) *finished = p ? p->clock.finished.load() : 0;
  return 0;
}

int bwtc_hip_wavelet_latency(bwtc_hip_ctx* ctx, double* mean_seconds) {
  if (!ctx || !mean_seconds) return -1;
  const HostPipeline* p = ctx->eng.pipeline;
  const uint64_t n = p ? p->clock.finished.load() : 0;
  *mean_seconds = n ? p->clock.latency_ns.load() * 1e-9 / (double)n : 0.0;
  return 0;
}

int bwtc_hip_wavelet_routes(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_route_counts* out, int reset) {
  if (!ctx || !out) return -1;
  WaveletRoutes& r = ctx->eng.routes;
  auto take = [reset](std::atomic<uint64_t>& c) { return reset ? c.exchange(0) : c.load(); };
  out->trees_device = take(r.trees_device);
  out->trees_host = take(r.trees_host);
  out->models_device = take(r.models_device);
  out->models_rejected = take(r.models_rejected);
  out->reject_reasons = reset ? r.reject_reasons.exchange(0) : r.reject_reasons.load();
  out->lost_turn = take(r.lost_turn);
  out->models_host_two_stage = take(r.host_two_stage);
  out->models_host_fused = take(r.host_fused);
  out->models_host_lanes = take(r.host_lanes);
  return 0;
}

int bwtc_hip_host_staging_bytes(uint64_t* now, uint64_t* peak) {
  if (now) *now = bwtc_hip::PinnedGauge::get().now.load();
  if (peak) *peak = bwtc_hip::PinnedGauge::get().peak.load();
  return 0;
}

int bwtc_hip_wavelet_encode_device_begin(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                         const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                         uint32_t threads, uint8_t* out, uint64_t out_cap,
                                         uint64_t* ticket) {
  if (!ctx || (!d_bwt && size) || !lf || !freqs || !out || !ticket) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  return wavelet_encode_begin(e, d_bwt, size, lf, n_lf, freqs, pick_threads(threads), out, out_cap, ticket);
}

int bwtc_hip_wavelet_encode_device_prepare(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                           const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                           uint32_t threads, uint8_t* out, uint64_t out_cap,
                                           uint64_t* ticket) {
  if (!ctx || (!d_bwt && size) || !lf || !freqs || !out || !ticket) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  return wavelet_encode_prepare(e, d_bwt, size, lf, n_lf, freqs, pick_threads(threads), out, out_cap, ticket);
}

int bwtc_hip_wavelet_encode_queue(bwtc_hip_ctx* ctx, uint64_t ticket, uint32_t state_in, uint32_t* state_out) {
  if (!ctx || !state_out || state_in > 7) return -1;
  return wavelet_encode_queue(ctx->eng, ticket, state_in, state_out);
}

int bwtc_hip_wavelet_encode_end(bwtc_hip_ctx* ctx, uint64_t ticket, uint64_t* out_bytes) {
  if (!ctx || !out_bytes) return -1;
  return wavelet_encode_end(ctx->eng, ticket, out_bytes);
}

int bwtc_hip_wavelet_encode_device(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                   const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                   uint32_t threads, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_bytes) {
  uint64_t ticket = 0;
  int rc = bwtc_hip_wavelet_encode_device_begin(ctx, d_bwt, size, lf, n_lf, freqs, threads, out, out_cap, &ticket);
  if (rc) return rc;
  return bwtc_hip_wavelet_encode_end(ctx, ticket, out_bytes);
}

int bwtc_hip_wavelet_encode(bwtc_hip_ctx* ctx, const uint8_t* bwt, uint32_t size,
                            const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                            uint32_t threads, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (!bwt && size)) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  int rc = stage_in(e, bwt, size);
  if (rc) return rc;
  return bwtc_hip_wavelet_encode_device(ctx, e.d_in, size, lf, n_lf, freqs, threads, out, out_cap, out_bytes);
}

int bwtc_hip_transform_and_encode_wavelet(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size,
                                          uint32_t starting_points, uint32_t threads,
                                          uint8_t* out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (!block && size) || !out || !out_bytes) return -1;
  BwtEngine& e = ctx->eng;
  if (size > e.max_block) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  uint32_t lf[256];
  uint32_t freqs[256];
  std::memset(freqs, 0, sizeof freqs);                    // WaveletCoders.cpp:78-79
  const uint32_t n_lf = bwtc_hip_n_lf(size, starting_points);
  int rc = stage_in(e, block, size);
  if (rc) return rc;
  rc = e.transform(e.d_in, e.d_in, size, false, lf, n_lf, freqs);
  if (rc) return rc;
  rc = stage_out(e, block, size);                         // the run scanner reuses the workspace
  if (rc) return rc;
  return bwtc_hip_wavelet_encode_device(ctx, e.d_in, size, lf, n_lf, freqs, threads, out, out_cap, out_bytes);
}

int bwtc_hip_host_wavelet_sections(uint32_t n_sections, const uint32_t* first_run,
                                   const uint8_t* run_sym, const uint32_t* run_start,
                                   const uint32_t* run_freqs, const uint32_t* dist_offset,
                                   const uint32_t* dist_len, const uint32_t* dist_cnt,
                                   uint32_t threads, char coder, uint32_t* state, uint8_t* out,
                                   uint64_t out_cap, uint64_t* out_bytes) {
  if (!first_run || !run_sym || !run_start || !run_freqs || !dist_offset || !dist_len || !dist_cnt ||
      !state || !out || !out_bytes || n_sections > 256 || !bwtc::wavelet::isWaveletModel(coder)) return -1;
  std::vector<std::vector<std::pair<uint32_t, uint32_t> > > dist(n_sections);
  std::vector<bwtc::wavelet::SectionRuns> secs(n_sections);
  for (uint32_t s = 0; s < n_sections; ++s) {
    for (uint32_t i = dist_offset[s]; i < dist_offset[s + 1]; ++i) dist[s].push_back(std::make_pair(dist_len[i], dist_cnt[i]));
    secs[s].symbols = run_sym + first_run[s];
    secs[s].starts = run_start + first_run[s];
    secs[s].n_runs = first_run[s + 1] - first_run[s];
    secs[s].run_freqs = run_freqs + (size_t)s * 256;
    secs[s].dist = dist[s].data();
    secs[s].n_dist = dist[s].size();
  }
  std::vector<bwtc::wavelet::SectionOutput> outs;
  bwtc::wavelet::encodeSections(secs, pick_threads(threads), state, &outs, coder);
  uint64_t n = 0;
  for (uint32_t s = 0; s < n_sections; ++s) {
    if (n + outs[s].bytes.size() > out_cap) return -1;
    std::memcpy(out + n, outs[s].bytes.data(), outs[s].bytes.size());
    n += outs[s].bytes.size();
  }
  *out_bytes = n;
  return 0;
}

int bwtc_hip_host_wavelet_streams(uint32_t n_sections, const uint32_t* first_run,
                                  const uint8_t* run_sym, const uint32_t* run_start,
                                  const uint32_t* run_freqs, const uint32_t* dist_offset,
                                  const uint32_t* dist_len, const uint32_t* dist_cnt,
                                  uint32_t threads, char coder, uint32_t* state, uint8_t* out,
                                  uint64_t out_cap, uint64_t* out_bytes) {
  if (!first_run || !run_sym || !run_start || !run_freqs || !dist_offset || !dist_len || !dist_cnt ||
      !state || !out || !out_bytes || n_sections > 256 || !bwtc::wavelet::isWaveletModel(coder)) return -1;
  std::vector<std::vector<std::pair<uint32_t, uint32_t> > > dist(n_sections);
  std::vector<bwtc::wavelet::SectionRuns> secs(n_sections);
  for (uint32_t s = 0; s < n_sections; ++s) {
    for (uint32_t i = dist_offset[s]; i < dist_offset[s + 1]; ++i) dist[s].push_back(std::make_pair(dist_len[i], dist_cnt[i]));
    secs[s].symbols = run_sym + first_run[s];
    secs[s].starts = run_start + first_run[s];
    secs[s].n_runs = first_run[s + 1] - first_run[s];
    secs[s].run_freqs = run_freqs + (size_t)s * 256;
    secs[s].dist = dist[s].data();
    secs[s].n_dist = dist[s].size();
  }
  bwtc::wavelet::StreamPlan plan;
  if (!bwtc::wavelet::planStreams(secs, &plan)) return -5;
  std::vector<uint32_t> coded_pos;
  std::vector<uint8_t> codes;
  if (!bwtc::wavelet::expandStreamsOnHost(plan, secs, &coded_pos, &codes)) return -3;
  codes.push_back(0);
  std::vector<bwtc::wavelet::SectionOutput> outs;
  bwtc::wavelet::codeStreams(plan, coded_pos.data(), codes.data(), pick_threads(threads), state, &outs, nullptr, coder);
  uint64_t n = 0;
  for (uint32_t s = 0; s < n_sections; ++s) {
    if (n + outs[s].bytes.size() > out_cap) return -1;
    std::memcpy(out + n, outs[s].bytes.data(), outs[s].bytes.size());
    n += outs[s].bytes.size();
  }
  *out_bytes = n;
  return 0;
}

int bwtc_hip_host_wavelet_streams_lanes(uint32_t n_sections, const uint32_t* first_run,
                                        const uint8_t* run_sym, const uint32_t* run_start,
                                        const uint32_t* run_freqs, const uint32_t* dist_offset,
                                        const uint32_t* dist_len, const uint32_t* dist_cnt,
                                        uint32_t threads, char coder, uint32_t* state, uint8_t* out,
                                        uint64_t out_cap, uint64_t* out_bytes) {
  if (!first_run || !run_sym || !run_start || !run_freqs || !dist_offset || !dist_len || !dist_cnt ||
      !state || !out || !out_bytes || n_sections > 256 || coder != 'B') return -1;
  std::vector<std::vector<std::pair<uint32_t, uint32_t> > > dist(n_sections);
  std::vector<bwtc::wavelet::SectionRuns> secs(n_sections);
  for (uint32_t s = 0; s < n_sections; ++s) {
    for (uint32_t i = dist_offset[s]; i < dist_offset[s + 1]; ++i) dist[s].push_back(std::make_pair(dist_len[i], dist_cnt[i]));
    secs[s].symbols = run_sym + first_run[s];
    secs[s].starts = run_start + first_run[s];
    secs[s].n_runs = first_run[s + 1] - first_run[s];
    secs[s].run_freqs = run_freqs + (size_t)s * 256;
    secs[s].dist = dist[s].data();
    secs[s].n_dist = dist[s].size();
  }
  bwtc::wavelet::StreamPlan plan;
  if (!bwtc::wavelet::planStreams(secs, &plan)) return -5;
  std::vector<uint32_t> coded_pos;
  std::vector<uint8_t> codes;
  if (!bwtc::wavelet::expandStreamsOnHost(plan, secs, &coded_pos, &codes)) return -3;
  const uint32_t total = coded_pos.back();
  std::vector<uint32_t> packed(total / 16 + 8, 0);
  std::memcpy(packed.data(), codes.data(), codes.size());
  std::vector<bwtc::wavelet::gm::Task> tasks;
  std::vector<bwtc::wavelet::gm::Chunk> chunks;
  bwtc::wavelet::gm::buildTasks(plan, coded_pos.data(), &tasks, &chunks);
  std::vector<uint16_t> w((size_t)total + 8);
  if (!bwtc::wavelet::gm::modelsOnHostLanes(packed.data(), total, tasks, chunks, state, w.data())) return -7;
  std::vector<bwtc::wavelet::SectionOutput> outs(plan.sections.size());
  bwtc::wavelet::StreamCoder sc(plan, coded_pos.data(), *state, bwtc::wavelet::StreamCoder::Modelled());
  std::atomic<size_t> cursor(0);
  (void)threads;
  sc.codeSectionsW(&cursor, w.data(), &outs);
  uint64_t n = 0;
  for (uint32_t s = 0; s < n_sections; ++s) {
    if (n + outs[s].bytes.size() > out_cap) return -1;
    std::memcpy(out + n, outs[s].bytes.data(), outs[s].bytes.size());
    n += outs[s].bytes.size();
  }
  *out_bytes = n;
  return 0;
}

void bwtc_hip_host_huffman_lengths(const uint64_t* freqs, uint8_t* clen) {
  bwtc::utils::calculateHuffmanLengths(freqs, clen);
}
void bwtc_hip_host_huffman_codes(const uint8_t* clen, uint32_t* code) {
  bwtc::utils::computeHuffmanCodes(clen, code);
}
uint32_t bwtc_hip_host_serialize_shape(const uint8_t* clen, uint8_t* out, uint32_t cap) {
  bool any = false;
  for (int c = 0; c < 256; ++c) any = any || clen[c];
  if (!any) return 0;
  std::vector<uint8_t> v;
  bwtc::serializeShape(clen, v);
  if (v.size() > cap) return 0;
  std::memcpy(out, v.data(), v.size());
  return (uint32_t)v.size();
}
uint32_t bwtc_hip_host_sections(const uint32_t* freqs, uint32_t* section_len) {
  const std::vector<uint32_t> s = bwtc::deduceSections(freqs);
  for (size_t i = 0; i < s.size(); ++i) section_len[i] = s[i];
  return (uint32_t)s.size();
}
uint32_t bwtc_hip_host_bwtblock_header(const uint32_t* lf, uint32_t n_lf, uint8_t* out, uint32_t cap) {
  std::vector<uint8_t> v;
  bwtc::writeBWTBlockHeader(lf, n_lf, v);
  if (v.size() > cap) return 0;
  std::memcpy(out, v.data(), v.size());
  return (uint32_t)v.size();
}

int bwtc_hip_suffix_array(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t length, uint32_t* sa) {
  if (!ctx || !T || !sa) return -1;
  if (length == 0) return 0;
  BwtEngine& e = ctx->eng;
  if ((u64)length > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, length, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  int rc = e.load_text(e.d_in, length, length, false, hist);
  if (rc) return rc;
  rc = e.suffix_sort(length, hist, false);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(sa, e.d_SA, (u64)length * 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  return 0;
}

int bwtc_hip_test_sort_u32(bwtc_hip_ctx* ctx, uint32_t* keys, uint32_t* vals, uint64_t n, int nbits) {
  return test_sort<u32>(ctx, keys, vals, n, nbits);
}
int bwtc_hip_test_sort_u64(bwtc_hip_ctx* ctx, uint64_t* keys, uint32_t* vals, uint64_t n, int nbits) {
  return test_sort<u64>(ctx, keys, vals, n, nbits);
}

int bwtc_hip_test_radix_pairs(bwtc_hip_ctx* ctx, void* keys, void* vals, uint64_t n, uint64_t n_holes, int key_bytes, int val_bytes,
                              int bit_lo, int nbits, int values_mode, int planes) {
  if (!ctx || !keys) return -1;
  BwtEngine& e = ctx->eng;
  typedef unsigned short u16v;
  if (key_bytes == 4 && val_bytes == 4) return test_radix_pairs<u32, u32>(e, static_cast<u32*>(keys), static_cast<u32*>(vals), n, n_holes, bit_lo, nbits, values_mode, planes);
  if (key_bytes == 8 && val_bytes == 4) return test_radix_pairs<u64, u32>(e, static_cast<u64*>(keys), static_cast<u32*>(vals), n, n_holes, bit_lo, nbits, values_mode, planes);
  if (key_bytes == 4 && val_bytes == 2) return test_radix_pairs<u32, u16v>(e, static_cast<u32*>(keys), static_cast<u16v*>(vals), n, n_holes, bit_lo, nbits, values_mode, planes);
  if (key_bytes == 8 && val_bytes == 2) return test_radix_pairs<u64, u16v>(e, static_cast<u64*>(keys), static_cast<u16v*>(vals), n, n_holes, bit_lo, nbits, values_mode, planes);
  return -1;
}

int bwtc_hip_test_radix_long(bwtc_hip_ctx* ctx, uint64_t* keys, void* vals, uint32_t* w, uint64_t n, int val_bytes, int items_per_thread,
                             int kbits, int wbits, int direct_w) {
  if (!ctx || !keys || !vals || !w) return -1;
  BwtEngine& e = ctx->eng;
  typedef unsigned short u16v;
  // the three instantiations the suffix sorter makes
  if (val_bytes == 4 && items_per_thread == 6) return test_radix_long<u32, 6>(e, keys, static_cast<u32*>(vals), w, n, kbits, wbits, direct_w != 0);
  if (val_bytes == 2 && items_per_thread == 6) return test_radix_long<u16v, 6>(e, keys, static_cast<u16v*>(vals), w, n, kbits, wbits, direct_w != 0);
  if (val_bytes == 2 && items_per_thread == 8) return test_radix_long<u16v, 8>(e, keys, static_cast<u16v*>(vals), w, n, kbits, wbits, direct_w != 0);
  return -1;
}

// The period step's last block: its period, its longest periodic stretch, the winner's votes and the depth of the step
// (zeros where nothing was looked for, nothing was found or no step ran).
int bwtc_hip_period_get(bwtc_hip_ctx* ctx, uint32_t* p, uint32_t* longest, uint32_t* votes, uint32_t* step_depth) {
  if (!ctx) return -1;
  const BwtEngine& e = ctx->eng;
  if (p) *p = e.blk.weighed.p;
  if (longest) *longest = e.blk.weighed.longest;
  if (votes) *votes = e.blk.weighed.votes;
  if (step_depth) *step_depth = e.blk.period_ran().depth;
  return 0;
}

// The closed-form steps of the last block: the depths the run step and the period step ran at (0: it did not; one
// period step that ranked the runs too reports its depth as both), the period step's period, the block's longest run
// and its longest proper stretch (0 where no pass made it).
int bwtc_hip_steps_get(bwtc_hip_ctx* ctx, uint32_t* run_depth, uint32_t* period_p, uint32_t* period_depth, uint32_t* longest_run,
                       uint32_t* longest_proper) {
  if (!ctx) return -1;
  const BwtEngine::BlockSort& b = ctx->eng.blk;
  const BwtEngine::StretchStep period = b.period_ran();
  if (run_depth) *run_depth = b.run_depth();
  if (period_p) *period_p = period.p;
  if (period_depth) *period_depth = period.depth;
  if (longest_run) *longest_run = b.run_longest;
  if (longest_proper) *longest_proper = b.weighed.proper;
  return 0;
}

// The copy rounds of the last block (BWTC_HIP_COPIES=1): the rounds that looked up at K[s] + h, the passes that made K[],
// the longest K any pass found, the depth of the first copy round (zeros without the switch or where no round took a pass).
int bwtc_hip_copies_get(bwtc_hip_ctx* ctx, uint32_t* rounds, uint32_t* passes, uint32_t* longest, uint32_t* first_depth) {
  if (!ctx) return -1;
  const BwtEngine::BlockSort::Copies& c = ctx->eng.blk.copies;
  if (rounds) *rounds = c.rounds;
  if (passes) *passes = c.passes;
  if (longest) *longest = c.longest;
  if (first_depth) *first_depth = c.first_depth;
  return 0;
}

// The copy round's three passes (BwtEngine::copy_lengths) over a given list and rank[]; no text is needed.
int bwtc_hip_test_copy_lengths(bwtc_hip_ctx* ctx, const uint32_t* suf, const uint32_t* grp, uint32_t m, const uint32_t* rank, uint32_t n,
                               uint32_t* k_out, uint32_t* longest_out) {
  if (!ctx) return -1;
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  return ctx->eng.test_copy_lengths(suf, grp, m, rank, n, k_out, longest_out);
}

// The last block's schedule of closed-form steps, in the order it took them: 5 words per entry -- the period (1: the run
// step), the depth it ran at or 0, its gate length, its votes, flags (1: it ranked the runs too; 2: it was dropped).
// Gate lengths and votes are reported under BWTC_HIP_MULTI only, by the blocks that look for a period; else 0.
// *n_out: the block's entries, of which min(cap, *n_out) are written.
int bwtc_hip_schedule_get(bwtc_hip_ctx* ctx, uint32_t* entries, uint32_t cap, uint32_t* n_out) {
  if (!ctx || !n_out || (cap && !entries)) return -1;
  const BwtEngine& e = ctx->eng;
  const BwtEngine::BlockSort& b = e.blk;
  // (under the switch a run step is due only where the rule holds or BWTC_HIP_PERIOD=1, so run_due decides nothing here)
  const bool reported = e.multi_steps && e.looks_for_period(false);
  *n_out = (uint32_t)b.n_steps;
  for (u32 i = 0; i < cap && i < (u32)b.n_steps; ++i) {
    const BwtEngine::StretchStep& s = b.steps[i];
    uint32_t* w = entries + 5 * i;
    w[0] = s.p; w[1] = s.depth; w[2] = reported ? s.shown_gate(e.mixed_rule()) : 0u; w[3] = reported ? s.votes : 0u; w[4] = (s.ranks_runs ? 1u : 0u) | (s.dropped ? 2u : 0u);
  }
  return 0;
}

// The sorter's own stretch-length pass (BwtEngine::stretch_lengths: three launches; p = 1: the run-length pass) over T as
// the sorter holds it -- loaded by load_text, padded with zero bytes -- on the context's buffers.  proper_out: the pass
// with the second maximum (bwtc_hip_test_period_proper).
static int test_period_pass(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest_out, uint32_t* proper_out);
int bwtc_hip_test_period_lengths(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest_out) {
  return test_period_pass(ctx, T, n, p, k_out, longest_out, nullptr);
}
int bwtc_hip_test_period_proper(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest_out,
                                uint32_t* proper_out) {
  if (!proper_out) return -1;
  return test_period_pass(ctx, T, n, p, k_out, longest_out, proper_out);
}
static int test_period_pass(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest_out, uint32_t* proper_out) {
  if (!ctx || !T || !k_out || !longest_out) return -1;
  BwtEngine& e = ctx->eng;
  if (p == 0 || p > kPeriodMax || n == 0 || (u64)n > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  int rc = e.load_text(e.d_in, n, n, false, hist);
  if (rc) return rc;
  rc = e.stretch_lengths(n, p, true, longest_out, proper_out);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(k_out, e.d_runK, (u64)n * 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return 0;
}

// The merging storing pass of BWTC_HIP_MULTI (stretch_lengths with a StepMerge: k_stretch_lengths<false, true, true>) over
// T as the sorter holds it.  k_inout: the block's merged words before the step (not read when fresh) and after it; h: the
// step's depth.  The refusals are bwtc_hip_test_period_lengths', and h == 0 or a word count above 2^31 - 1.
int bwtc_hip_test_period_merge(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t h, int fresh, uint32_t* k_inout,
                               uint32_t* longest_out, uint32_t* proper_out) {
  if (!ctx || !T || !k_inout || !longest_out || !proper_out) return -1;
  BwtEngine& e = ctx->eng;
  if (p == 0 || p > kPeriodMax || n == 0 || (u64)n > e.cap || h == 0 || n > 0x7FFFFFFFu) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  int rc = e.load_text(e.d_in, n, n, false, hist);
  if (rc) return rc;
  if (!fresh) BWTC_HIP_TRY(hipMemcpyAsync(e.d_runK, k_inout, (u64)n * 4, hipMemcpyHostToDevice, e.stream));
  else BWTC_HIP_TRY(hipMemsetAsync(e.d_runK, 0xA5, (u64)n * 4, e.stream));   // (a fresh pass must not read what lies there)
  const BwtEngine::StepMerge merge{h, fresh != 0};
  rc = e.stretch_lengths(n, p, true, longest_out, proper_out, &merge);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(k_inout, e.d_runK, (u64)n * 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return 0;
}

// The finder's candidates (BwtEngine::period_winners: k_period_winners, one workgroup) over a vote table of kPeriodMax + 1
// words, copied into the context's own d_votes: up to 8 (distance, votes) pairs into out[16], their number into *n_out.
int bwtc_hip_test_period_winners(bwtc_hip_ctx* ctx, const uint32_t* table, uint32_t need, uint32_t* out, uint32_t* n_out) {
  if (!ctx || !table || !out || !n_out) return -1;
  BwtEngine& e = ctx->eng;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_votes, table, (size_t)(kPeriodMax + 1) * 4, hipMemcpyHostToDevice, e.stream));
  const int rc = e.period_winners(need, out, n_out);
  if (rc) return rc;
  BWTC_HIP_TRY(hipGetLastError());
  return 0;
}

// ---- test hooks of the long periods (BWTC_HIP_LONG_PERIODS; they need no switch) -----------------------------------
// The long finder (BwtEngine::long_period_votes: sweep 1, the coarse bins' pick, sweep 2, the merged candidates) over a
// given sorted list of m entries: ks into d_R1, vs into d_V0, and -- the RUNS_OUT rule -- k1[0 ... max(vs)] into d_runK.
// Up to 8 (distance, votes) pairs with `need` votes or more, distances 2 ... 2^24, into out16, zeros behind them; their
// number into *found.  -1: m < 2, m or a suffix number above the context's block size, need == 0 or (m - 1) / need > 64.
int bwtc_hip_test_long_period_votes(bwtc_hip_ctx* ctx, const uint64_t* ks, const uint32_t* vs, uint32_t m, uint64_t kmask, const uint32_t* k1,
                                    uint32_t need, uint32_t* out16, uint32_t* found) {
  if (!ctx || !ks || !vs || !out16 || !found) return -1;
  BwtEngine& e = ctx->eng;
  if (m < 2 || (u64)m > e.cap) return -1;
  u32 top = 0;
  for (u32 i = 0; i < m; ++i) top = std::max(top, vs[i]);
  if ((u64)top >= e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  hipStream_t st = e.stream;
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_R1, ks, (u64)m * 8, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_V0, vs, (u64)m * 4, hipMemcpyHostToDevice, st));
  if (k1) BWTC_HIP_TRY(hipMemcpyAsync(e.d_runK, k1, ((u64)top + 1) * 4, hipMemcpyHostToDevice, st));
  u32 cand[2 * kPeriodCandidates], n_found = 0;
  bool swept = false;
  const int rc = e.long_period_votes(reinterpret_cast<const u64*>(e.d_R1), e.d_V0, m, kmask, k1 ? (const u32*)e.d_runK : nullptr, need, kLongPeriodMax,
                                     false, cand, &n_found, &swept);
  if (rc) return rc;
  BWTC_HIP_TRY(hipGetLastError());
  std::memcpy(out16, cand, sizeof cand);
  *found = n_found;
  return 0;
}

// The wide probe (BwtEngine::long_period_probe: k_period_probe_wide) over T as the sorter holds it: *flag_out = 1 when an
// aligned window of `span` positions from p on, p + i * span, holds no break of period p.  -1: p outside 4097 ... 2^24,
// span == 0, n == 0 or above the context's block size.
int bwtc_hip_test_long_period_probe(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t span, uint32_t* flag_out) {
  if (!ctx || !T || !flag_out) return -1;
  BwtEngine& e = ctx->eng;
  if (p <= kPeriodMax || p > kLongPeriodMax || span == 0 || n == 0 || (u64)n > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  int rc = e.load_text(e.d_in, n, n, false, hist);
  if (rc) return rc;
  bool found = false;
  rc = e.long_period_probe(n, p, span, &found);
  if (rc) return rc;
  BWTC_HIP_TRY(hipGetLastError());
  *flag_out = found ? 1u : 0u;
  return 0;
}

// The sorter's own stretch-length pass with both maxima (bwtc_hip_test_period_proper's) for 4097 <= p <= 2^24 and p < n:
// k_p[] into k_out, longest2[0] = the longest stretch, longest2[1] = the longest proper one.  -1 outside that range (and
// for n above the context's block size); k_out is not written then.
int bwtc_hip_test_long_period_lengths(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest2) {
  if (!ctx || !T || !k_out || !longest2) return -1;
  BwtEngine& e = ctx->eng;
  if (p <= kPeriodMax || p > kLongPeriodMax || p >= n || (u64)n > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  int rc = e.load_text(e.d_in, n, n, false, hist);
  if (rc) return rc;
  rc = e.stretch_lengths(n, p, true, longest2, longest2 + 1);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(k_out, e.d_runK, (u64)n * 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return 0;
}

// ---- test hooks of the code-key stage (bwtc_hip_test_code_*; DESIGN.md, "The code-key hooks") --------------------
// k_pair_counts, k_code_build and k_make_keys_code through BwtEngine::test_code_stage: suffix_sort's launch shapes and
// key layout, T loaded by load_text, the context's own d_pairs / d_codes / d_R1 / d_W0 / d_P0.  Contracts are checked on
// the host before anything is launched (-1); canaries sit behind the keys, the second words, the plane and the table.
namespace {
constexpr u32 kCodeTableWords = 257u * 256u;
constexpr u32 kCodeErrorWord = 522;                    // kSmallError

bool code_shape_ok(const BwtEngine& e, const uint8_t* T, uint32_t n, int code_bits, int split) {
  if (!T || n == 0 || (u64)n + kSortCanaryBytes > e.cap) return false;
  if (code_bits < 40 || code_bits > 72) return false;
  return !(split && n > (1u << 29));
}

// every row prefix free over `sigma` symbols, lengths 1 .. 26, no bits above a codeword's length
bool code_table_ok(const uint32_t* table, uint32_t sigma) {
  for (u32 row = 0; row < 257u; ++row) {
    const uint32_t* r = table + (size_t)row * 256u;
    for (u32 s = 0; s < sigma; ++s) {
      const u32 ls = r[s] >> 27, bs = r[s] & 0x7FFFFFFu;
      if (ls < 1u || ls > 26u || (bs >> ls)) return false;
      for (u32 t = 0; t < s; ++t) {
        const u32 lt = r[t] >> 27, bt = r[t] & 0x7FFFFFFu;
        if (ls <= lt ? (bt >> (lt - ls)) == bs : (bs >> (ls - lt)) == bt) return false;
      }
    }
  }
  return true;
}

// loads T, guards and poisons the key maker's outputs
int code_prepare(BwtEngine& e, const uint8_t* T, uint32_t n, u32* hist, SortCanaries& can) {
  BWTC_HIP_TRY(hipSetDevice(e.device));
  hipStream_t st = e.stream;
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, n, hipMemcpyHostToDevice, st));
  const int rc = e.load_text(e.d_in, n, n, false, hist);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemsetAsync(e.d_R1, 0xA5, (u64)n * 8, st));
  BWTC_HIP_TRY(hipMemsetAsync(e.d_W0, 0xA5, (u64)n * 4, st));
  BWTC_HIP_TRY(hipMemsetAsync(e.d_P0, 0xA5, n, st));
  BWTC_HIP_TRY(can.put(e.d_R1, (u64)n * 8, st));
  BWTC_HIP_TRY(can.put(e.d_W0, (u64)n * 4, st));
  BWTC_HIP_TRY(can.put(e.d_P0, n, st));
  return 0;
}

int code_fetch_keys(BwtEngine& e, uint32_t n, uint64_t* keys, uint32_t* w, uint8_t* plane) {
  hipStream_t st = e.stream;
  if (keys) BWTC_HIP_TRY(hipMemcpyAsync(keys, e.d_R1, (u64)n * 8, hipMemcpyDeviceToHost, st));
  if (w) BWTC_HIP_TRY(hipMemcpyAsync(w, e.d_W0, (u64)n * 4, hipMemcpyDeviceToHost, st));
  if (plane) BWTC_HIP_TRY(hipMemcpyAsync(plane, e.d_P0, n, hipMemcpyDeviceToHost, st));
  return 0;
}
}  // namespace

int bwtc_hip_test_code_stage(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, int lone_sentinel, int code_bits, int split, uint8_t* lut_out,
                             uint32_t* sigma_out, uint32_t* counts_out, uint32_t* table_out, uint32_t* err_out, uint64_t* keys, uint32_t* w,
                             uint8_t* plane) {
  if (!ctx || !lut_out || !sigma_out || !counts_out || !table_out || !err_out) return -1;
  BwtEngine& e = ctx->eng;
  if (!code_shape_ok(e, T, n, code_bits, split)) return -1;
  if (lone_sentinel && (T[n - 1] != 0 || std::memchr(T, 0, n - 1))) return -1;   // the only zero byte is the terminator
  hipStream_t st = e.stream;
  SortCanaries can;
  u32 hist[256];
  int rc = code_prepare(e, T, n, hist, can);
  if (rc) return rc;
  BWTC_HIP_TRY(can.put(e.d_codes, (u64)kCodeTableWords * 4, st));
  rc = e.test_code_stage(7u, n, hist, lone_sentinel != 0, code_bits, split != 0, lut_out, sigma_out);
  if (rc) return rc;
  std::vector<u32> replicas((size_t)8 * 65536);
  BWTC_HIP_TRY(hipMemcpyAsync(replicas.data(), e.d_pairs, replicas.size() * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(table_out, e.d_codes, (u64)kCodeTableWords * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_small + kCodeErrorWord, e.d_small + kCodeErrorWord, 4, hipMemcpyDeviceToHost, st));
  rc = code_fetch_keys(e, n, keys, w, plane);
  if (rc) return rc;
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  for (u32 i = 0; i < 65536u; ++i) {
    u32 sum = 0;
    for (u32 r = 0; r < 8u; ++r) sum += replicas[(size_t)r * 65536u + i];
    counts_out[i] = sum;
  }
  *err_out = e.h_small[kCodeErrorWord];
  return can.verdict();
}

int bwtc_hip_test_code_table(bwtc_hip_ctx* ctx, const uint32_t* counts, uint32_t sigma, uint32_t* table_out, uint32_t* err_out) {
  if (!ctx || !counts || !table_out || !err_out || sigma < 1 || sigma > 256) return -1;
  BwtEngine& e = ctx->eng;
  u64 total = 0;
  for (u32 i = 0; i < 65536u; ++i) total += counts[i];
  if (total > (1ull << 21)) return -1;                  // the product's sample: at most 512 tiles of 4096 pairs
  BWTC_HIP_TRY(hipSetDevice(e.device));
  hipStream_t st = e.stream;
  SortCanaries can;
  BWTC_HIP_TRY(hipMemsetAsync(e.d_pairs, 0, (size_t)8 * 65536 * 4, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_pairs, counts, 65536 * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemsetAsync(e.d_small + kCodeErrorWord, 0, 4, st));
  BWTC_HIP_TRY(hipMemsetAsync(e.d_codes, 0xA5, (u64)kCodeTableWords * 4, st));
  BWTC_HIP_TRY(can.put(e.d_codes, (u64)kCodeTableWords * 4, st));
  u8 lut[256] = {0};
  const int rc = e.test_code_stage(2u, 0, nullptr, false, 72, false, lut, &sigma);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(table_out, e.d_codes, (u64)kCodeTableWords * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.h_small + kCodeErrorWord, e.d_small + kCodeErrorWord, 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  *err_out = e.h_small[kCodeErrorWord];
  return can.verdict();
}

int bwtc_hip_test_code_keys(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, int code_bits, int split, const uint8_t* lut, uint32_t sigma,
                            const uint32_t* table, uint64_t* keys, uint32_t* w, uint8_t* plane) {
  if (!ctx || !lut || !table || !keys || !w || !plane || sigma < 1 || sigma > 256) return -1;
  BwtEngine& e = ctx->eng;
  if (!code_shape_ok(e, T, n, code_bits, split)) return -1;
  if (lut[0] >= sigma) return -1;                       // the padding behind T
  for (u32 i = 0; i < n; ++i) if (lut[T[i]] >= sigma) return -1;
  if (!code_table_ok(table, sigma)) return -1;
  hipStream_t st = e.stream;
  SortCanaries can;
  u32 hist[256];
  int rc = code_prepare(e, T, n, hist, can);
  if (rc) return rc;
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_codes, table, (u64)kCodeTableWords * 4, hipMemcpyHostToDevice, st));
  u8 lut_in[256];
  std::memcpy(lut_in, lut, 256);
  rc = e.test_code_stage(4u, n, nullptr, false, code_bits, split != 0, lut_in, &sigma);
  if (rc) return rc;
  rc = code_fetch_keys(e, n, keys, w, plane);
  if (rc) return rc;
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

// ---- test hooks of the finisher (bwtc_hip_test_finish_pass / _local_pass; DESIGN.md, "The finisher hooks") -------
// One k_finish launch through BwtEngine::test_finish_pass, which checks the list's contracts on the host, guards every
// array the kernel may write with canaries and shares its launch code with finisher_passes / local_pass.
static int test_fin_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_pass* p, int ranks) {
  if (!ctx || !T || !p) return -1;
  if (!p->ebase || !p->ecount || !p->S || !p->P || !p->H || !p->C || !p->nS || !p->nP || !p->nH || !p->nC || !p->next_base || !p->next_count ||
      !p->hS || !p->hHP || !p->hard_count || !p->shal_count || !p->SA || !p->out || !p->small || !p->lf) return -1;
  if (ranks ? (!p->rank || !p->us || !p->ur) : (!p->hC || !p->sS || !p->sHP)) return -1;
  BwtEngine& e = ctx->eng;
  if (p->n == 0 || (u64)p->n + kSortCanaryBytes > e.cap) return -1;
  p->ranks = ranks;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, p->n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  const int rc = e.load_text(e.d_in, p->n, p->n, false, hist);
  if (rc) return rc;
  return e.test_finish_pass(*p);
}
int bwtc_hip_test_finish_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_pass* pass) { return test_fin_pass(ctx, T, pass, 0); }
int bwtc_hip_test_local_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_pass* pass) { return test_fin_pass(ctx, T, pass, 1); }
int bwtc_hip_test_finisher(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_run* p) {
  if (!ctx || !T || !p) return -1;
  if (!p->S || !p->P || !p->H || !p->C || !p->outcome || !p->info || !p->pS || !p->pHP || !p->sS || !p->sHP || !p->lS || !p->lP || !p->lH || !p->lC ||
      !p->SA || !p->out || !p->small || !p->lf) return -1;
  BwtEngine& e = ctx->eng;
  if (p->n == 0 || (u64)p->n + kSortCanaryBytes > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, p->n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  const int rc = e.load_text(e.d_in, p->n, p->n, false, hist);
  if (rc) return rc;
  return e.test_finisher(*p);
}

// ---- test hooks of the ranking step and the rounds' kernels (bwtc_hip_test_rank_* / _round_keys; DESIGN.md, "The ranking hooks")
// Through BwtEngine::test_rank_pass / _scan / _scatter / test_round_keys, which check the kernels' contracts on the host,
// guard the arrays the kernels may write and share their launch code with rank_step (launch_rerank and its neighbours).
static int test_load_text(BwtEngine& e, const uint8_t* T, u32 n) {
  if (!T || n == 0 || (u64)n + kSortCanaryBytes > e.cap) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_in, T, n, hipMemcpyHostToDevice, e.stream));
  u32 hist[256];
  return e.load_text(e.d_in, n, n, false, hist);
}
int bwtc_hip_test_rank_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_rank_pass* p) {
  if (!ctx || !T || !p) return -1;
  if (!p->aggA || !p->aggB || !p->aggC || !p->counts || !p->rank || !p->pair_s || !p->pair_r || !p->rec || !p->val || !p->rplane || !p->aidx ||
      !p->aglob_out || !p->agrp || !p->achr || !p->SA || !p->out || !p->small || !p->lf) return -1;
  const int rc = test_load_text(ctx->eng, T, p->n);
  if (rc) return rc;
  return ctx->eng.test_rank_pass(*p);
}
int bwtc_hip_test_rank_scan(bwtc_hip_ctx* ctx, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t ntiles, uint32_t* parts_out, uint32_t parts_cap,
                            uint32_t* counts_out) {
  if (!ctx || !a || !b || !c || !parts_out || !counts_out) return -1;
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  return ctx->eng.test_rank_scan(a, b, c, ntiles, parts_out, parts_cap, counts_out);
}
int bwtc_hip_test_rank_scatter(bwtc_hip_ctx* ctx, int dense, const uint32_t* where, const uint32_t* what, const uint64_t* rec, uint32_t m,
                               uint32_t n, int bin_shift, uint32_t* rank) {
  if (!ctx) return -1;
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  return ctx->eng.test_rank_scatter(dense != 0, where, what, rec, m, n, bin_shift, rank);
}
int bwtc_hip_test_round_keys(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_round_keys* rk) {
  if (!ctx || !T || !rk) return -1;
  const int rc = test_load_text(ctx->eng, T, rk->n);
  if (rc) return rc;
  return ctx->eng.test_round_keys(*rk);
}

int bwtc_hip_test_round(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_round* p) {
  if (!ctx || !T || !p) return -1;
  if (!p->result || !p->nks || !p->nvs || !p->naglob || !p->ngrp || !p->nchr || !p->SA || !p->out || !p->small || !p->lf) return -1;
  const int rc = test_load_text(ctx->eng, T, p->n);
  if (rc) return rc;
  return ctx->eng.test_round(*p);
}

int bwtc_hip_test_radix_segmented(bwtc_hip_ctx* ctx, uint32_t* keys, uint64_t n, int bit_lo, const uint32_t* tile_first, uint32_t nseg) {
  if (!ctx || !keys || !tile_first) return -1;
  BwtEngine& e = ctx->eng;
  const u64 tile = (u64)radix_tile<u32>();
  if (n == 0 || n % tile != 0 || n + kSortCanaryBytes > e.cap) return -1;
  if (bit_lo < 0 || bit_lo + 2 * kRadixBits > 32) return -1;
  if (nseg == 0 || (u64)nseg + 1 > e.cap || tile_first[0] != 0 || (u64)tile_first[nseg] != n / tile) return -1;
  for (u32 s = 0; s < nseg; ++s) if (tile_first[s] > tile_first[s + 1]) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  hipStream_t st = e.stream;
  u32* k0 = static_cast<u32*>(e.d_R1);
  u32* k1 = static_cast<u32*>(e.d_R2);
  std::vector<u8> plane(n);                             // the first pass's digit rule: radix_digit(key, bit_lo)
  for (u64 i = 0; i < n; ++i) plane[i] = (u8)((keys[i] >> bit_lo) & 255u);
  SortCanaries can;
  BWTC_HIP_TRY(hipMemcpyAsync(k0, keys, n * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_P0, plane.data(), n, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(hipMemcpyAsync(e.d_V0, tile_first, ((u64)nseg + 1) * 4, hipMemcpyHostToDevice, st));
  BWTC_HIP_TRY(can.put(k0, n * 4, st));
  BWTC_HIP_TRY(can.put(k1, n * 4, st));
  BWTC_HIP_TRY(can.put(e.d_P0, n, st));
  BWTC_HIP_TRY(can.put(e.d_P1, n, st));
  u32* ks = nullptr;
  radix_sort_keys_segmented(k0, k1, n, bit_lo, e.d_V0, nseg, e.d_table, e.d_partial, st, &ks, e.d_P0, e.d_P1);
  BWTC_HIP_TRY(hipMemcpyAsync(keys, ks, n * 4, hipMemcpyDeviceToHost, st));
  BWTC_HIP_TRY(can.fetch(st));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return can.verdict();
}

// Test hook of the GPU lane engine (gpu_lanes.hpp): k chains of w-elements, chain j = elements [bounds[j], bounds[j+1]),
// each coded from a fresh BitEncoder -- on GPU lanes (mode 0) or by the host's runChainW (mode 1).  The chains' bytes
// (flush included) come back one after the other in `out`, offsets[j] .. offsets[j+1].
int bwtc_hip_test_gpu_lanes(bwtc_hip_ctx* ctx, const uint16_t* w, uint64_t n, const uint64_t* bounds, uint32_t k, int mode,
                            uint8_t* out, uint64_t out_cap, uint64_t* offsets) {
  if (!ctx || !w || !bounds || !out || !offsets || k == 0 || bounds[k] > n) return -1;
  for (uint32_t j = 0; j < k; ++j) if (bounds[j] > bounds[j + 1]) return -1;       // chains are [bounds[j], bounds[j + 1])
  BWTC_HIP_TRY(hipSetDevice(ctx->eng.device));
  std::vector<std::vector<uint8_t> > outs(k);
  struct Src : bwtc::wavelet::ChainSource {
    const uint16_t* w; const uint64_t* bounds; uint32_t k; std::vector<std::vector<uint8_t> >* outs; std::atomic<uint32_t> at{0}, finished{0};
    bool next(bwtc::wavelet::ChainDesc* d) {
      const uint32_t j = at.fetch_add(1);
      if (j >= k) return false;
      d->codes = nullptr; d->prob = nullptr; d->w = w; d->begin = bounds[j]; d->end = bounds[j + 1]; d->out = &(*outs)[j];
      d->cookie = this;
      return true;
    }
    void done(void*) { ++finished; }
  } src;
  src.w = w; src.bounds = bounds; src.k = k; src.outs = &outs;
  int rc = 0;
  if (mode == 0) {
    uint16_t* d_w = nullptr;
    BWTC_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_w), n * 2 + 256));
    if (hipMemcpy(d_w, w, n * 2, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_w); return -3; }
    const uint16_t* dw = d_w;
    bwtc_hip::GpuLaneStats st;
    rc = bwtc_hip::runCoderLanesGpu(src, ctx->eng.device, [dw](void*) { return dw; }, &st);
    (void)hipFree(d_w);
    if (std::getenv("BWTC_HIP_DEBUG"))
      std::fprintf(stderr, "gpu lanes: %llu chains on lanes, %llu on the host, %llu elements, %llu slices, %llu bytes; %.1f ns per lane step\n", (unsigned long long)st.chains.load(),
                   (unsigned long long)st.host_chains.load(), (unsigned long long)st.elements.load(), (unsigned long long)st.slices.load(), (unsigned long long)st.bytes.load(),
                   st.slice_steps.load() ? (double)st.slice_ns.load() / (double)st.slice_steps.load() : 0.0);
  } else {
    bwtc::wavelet::ChainDesc d;
    while (src.next(&d)) {
      bwtc::wavelet::CoderChain c;
      c.start(d.begin, d.end, d.out);
      bwtc::wavelet::runChainW(c, d.w, c.e);
      c.finish();
      src.done(d.cookie);
    }
  }
  if (rc) return rc;
  if (src.finished.load() != k) return -3;
  uint64_t at = 0;
  for (uint32_t j = 0; j < k; ++j) {
    offsets[j] = at;
    if (at + outs[j].size() > out_cap) return -1;
    std::memcpy(out + at, outs[j].data(), outs[j].size());
    at += outs[j].size();
  }
  offsets[k] = at;
  return 0;
}
// ---- test hooks of the model passes (wavelet_gpu_models.hip / .hpp) ------------------------
namespace {
// the hooks' contract for a task list: types 0..3, tasks non-empty and tiling [0, n_coded) in order
bool model_tasks_from(const uint32_t* tasks, uint32_t nt, uint32_t n_coded, std::vector<bwtc::wavelet::gm::Task>* out) {
  if (!tasks || nt == 0 || n_coded == 0 || n_coded > 0xFFFFF800u) return false;
  uint32_t at = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t b = tasks[3 * (size_t)t], e = tasks[3 * (size_t)t + 1], type = tasks[3 * (size_t)t + 2];
    if (type > 3u || b != at || e <= b || e > n_coded) return false;
    at = e;
  }
  if (at != n_coded) return false;
  out->resize(nt);
  for (uint32_t t = 0; t < nt; ++t) (*out)[t] = bwtc::wavelet::gm::Task{tasks[3 * (size_t)t], tasks[3 * (size_t)t + 1], tasks[3 * (size_t)t + 2], 0};
  return true;
}
}  // namespace

int bwtc_hip_test_models(bwtc_hip_ctx* ctx, const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks, uint32_t nt,
                         uint32_t state_in, uint32_t flags, bwtc_hip_models_out* out) {
  return bwtc_hip_test_models_letter(ctx, 'B', packed, n_coded, tasks, nt, state_in, flags, out);
}

int bwtc_hip_test_models_letter(bwtc_hip_ctx* ctx, char letter, const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks,
                                uint32_t nt, uint32_t state_in, uint32_t flags, bwtc_hip_models_out* out) {
  namespace gm = bwtc::wavelet::gm;
  if (!ctx || !packed || !tasks || !out || !out->w || state_in > 7u || flags > 3u || !bwtc::wavelet::isWaveletModel(letter)) return -1;
  const u32 kind = gm::kindOfLetter(letter);
  const bool lean = (flags & 2u) != 0;
  if (!lean && (!out->chunks || !out->cmap || !out->cstate || !out->base || !out->sb || !out->sbits || !out->smap || !out->snaps ||
                !out->sstart)) return -1;
  BwtEngine& e = ctx->eng;
  const u64 piece_bytes = ((u64)n_coded + 63) / 64 * 16;              // the packed streams go to R1 (8 * cap bytes)
  if (piece_bytes > e.cap * 8) return -1;
  std::vector<gm::Task> tk;
  if (!model_tasks_from(tasks, nt, n_coded, &tk)) return -1;
  std::vector<gm::Chunk> chunks;
  gm::cutChunks(&tk, &chunks);
  const u32 nc = (u32)chunks.size();
  BWTC_HIP_TRY(hipSetDevice(e.device));
  BWTC_HIP_TRY(e.codes_wait());
  BWTC_HIP_TRY(e.wait());
  u32* d_packed = static_cast<u32*>(e.d_R1);
  BWTC_HIP_TRY(hipMemsetAsync(d_packed, 0, piece_bytes, e.stream));
  BWTC_HIP_TRY(hipMemcpyAsync(d_packed, packed, ((u64)n_coded + 15) / 16 * 4, hipMemcpyHostToDevice, e.stream));
  struct Lines {                                                      // the form of the partition pass, for this call only
    BwtEngine& e; bool was;
    Lines(BwtEngine& en, bool on) : e(en), was(en.gm_partition_lines) { e.gm_partition_lines = on; }
    ~Lines() { e.gm_partition_lines = was; }
  } lines(e, (flags & 1u) != 0);
  GmPass g;
  int rc = wavelet_models_prepare_tasks(e, d_packed, n_coded, tk, chunks, &g, true, nullptr, kind);
  if (rc) return rc;
  if (!g.ends_ready) return -3;
  for (int i = 0; i < 8; ++i) out->ends[i] = g.ends[i];
  out->tail[0] = out->tail[1] = out->tail[2] = out->tail[3] = 0xFFFFFFFFu;
  u32 early = 0xFFFFFFFFu;
  rc = wavelet_models_run(e, g, state_in, out->w, out->tail, &early);
  const hipError_t hw = e.codes_wait();                               // (also after an error: whatever was queued is through)
  const hipError_t hs = e.wait();
  if (rc) return rc;
  BWTC_HIP_TRY(hw);
  BWTC_HIP_TRY(hs);
  BWTC_HIP_TRY(hipGetLastError());
  if (early != (kind == gm::kKindB ? g.ends[state_in] : gm::mainStart(kind))) return -3;
  out->nc = nc;
  out->nsc = g.nsc;
  if (lean) return 0;
  // the chunk table as the device holds it
  {
    std::vector<gm::Chunk> back(nc);
    BWTC_HIP_TRY(hipMemcpy(back.data(), g.d_chunks, (size_t)nc * sizeof(gm::Chunk), hipMemcpyDeviceToHost));
    for (u32 c = 0; c < nc; ++c) {
      out->chunks[3 * (size_t)c] = back[c].begin; out->chunks[3 * (size_t)c + 1] = back[c].end; out->chunks[3 * (size_t)c + 2] = back[c].task_first;
    }
  }
  BWTC_HIP_TRY(hipMemcpy(out->cmap, g.d_cmap, (size_t)nc * 8, hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->cstate, g.d_cstate, (size_t)nc * 4, hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->base, g.d_base, (size_t)g.n_base * 4, hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->sb, g.d_sb, ((size_t)g.ns + 1) * 4, hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->sbits, g.d_sbits, ((size_t)n_coded / 32 + 16) * 4, hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->smap, g.d_smap, (size_t)g.nsc * sizeof(gm::SlotMap), hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->snaps, g.d_snaps, (((size_t)n_coded + gm::kSample - 1) / gm::kSample) * sizeof(gm::SlotMap), hipMemcpyDeviceToHost));
  BWTC_HIP_TRY(hipMemcpy(out->sstart, g.d_sstart, (size_t)g.nsc * 2, hipMemcpyDeviceToHost));
  return 0;
}

int bwtc_hip_host_test_models(const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks, uint32_t nt,
                              uint32_t state_in, uint16_t* w_out, uint32_t* state_out) {
  return bwtc_hip_host_test_models_letter('B', packed, n_coded, tasks, nt, state_in, w_out, state_out);
}

int bwtc_hip_host_test_models_letter(char letter, const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks, uint32_t nt,
                                     uint32_t state_in, uint16_t* w_out, uint32_t* state_out) {
  namespace gm = bwtc::wavelet::gm;
  if (!packed || !tasks || !w_out || !state_out || state_in > 7u || !bwtc::wavelet::isWaveletModel(letter)) return -1;
  std::vector<gm::Task> tk;
  if (!model_tasks_from(tasks, nt, n_coded, &tk)) return -1;
  std::vector<gm::Chunk> chunks;
  gm::cutChunks(&tk, &chunks);
  // buffers of exactly the sizes wavelet_models_prepare and reserve_models allot: whole 16-byte pieces, n_coded + 8 elements
  std::vector<uint32_t> pk(((size_t)n_coded + 63) / 64 * 4, 0);
  std::memcpy(pk.data(), packed, ((size_t)n_coded + 15) / 16 * 4);
  std::vector<uint16_t> w((size_t)n_coded + 8);
  uint32_t st = state_in;
  if (!gm::modelsOnHostLanes(pk.data(), n_coded, tk, chunks, &st, w.data(), letter)) return -7;
  std::memcpy(w_out, w.data(), (size_t)n_coded * 2);
  *state_out = st;
  return 0;
}

int bwtc_hip_host_wavelet_elements(uint32_t n_sections, const uint32_t* first_run,
                                   const uint8_t* run_sym, const uint32_t* run_start,
                                   const uint32_t* run_freqs, const uint32_t* dist_offset,
                                   const uint32_t* dist_len, const uint32_t* dist_cnt, uint32_t* state,
                                   uint32_t* n_coded, uint32_t* nt, uint32_t* packed, uint64_t packed_words,
                                   uint32_t* tasks, uint32_t tasks_cap, uint16_t* w, uint64_t w_cap) {
  return bwtc_hip_host_wavelet_elements_letter('B', n_sections, first_run, run_sym, run_start, run_freqs, dist_offset, dist_len, dist_cnt,
                                               state, n_coded, nt, packed, packed_words, tasks, tasks_cap, w, w_cap);
}

int bwtc_hip_host_wavelet_elements_letter(char letter, uint32_t n_sections, const uint32_t* first_run,
                                          const uint8_t* run_sym, const uint32_t* run_start,
                                          const uint32_t* run_freqs, const uint32_t* dist_offset,
                                          const uint32_t* dist_len, const uint32_t* dist_cnt, uint32_t* state,
                                          uint32_t* n_coded, uint32_t* nt, uint32_t* packed, uint64_t packed_words,
                                          uint32_t* tasks, uint32_t tasks_cap, uint16_t* w, uint64_t w_cap) {
  if (!bwtc::wavelet::isWaveletModel(letter)) return -1;
  if (!first_run || !run_sym || !run_start || !run_freqs || !dist_offset || !dist_len || !dist_cnt ||
      !state || !n_coded || !nt || n_sections > 256) return -1;
  std::vector<std::vector<std::pair<uint32_t, uint32_t> > > dist(n_sections);
  std::vector<bwtc::wavelet::SectionRuns> secs(n_sections);
  for (uint32_t s = 0; s < n_sections; ++s) {
    for (uint32_t i = dist_offset[s]; i < dist_offset[s + 1]; ++i) dist[s].push_back(std::make_pair(dist_len[i], dist_cnt[i]));
    secs[s].symbols = run_sym + first_run[s];
    secs[s].starts = run_start + first_run[s];
    secs[s].n_runs = first_run[s + 1] - first_run[s];
    secs[s].run_freqs = run_freqs + (size_t)s * 256;
    secs[s].dist = dist[s].data();
    secs[s].n_dist = dist[s].size();
  }
  bwtc::wavelet::StreamPlan plan;
  if (!bwtc::wavelet::planStreams(secs, &plan)) return -5;
  std::vector<uint32_t> coded_pos;
  std::vector<uint8_t> codes;
  if (!bwtc::wavelet::expandStreamsOnHost(plan, secs, &coded_pos, &codes)) return -3;
  const uint32_t total = coded_pos.back();
  std::vector<bwtc::wavelet::gm::Task> tk;
  std::vector<bwtc::wavelet::gm::Chunk> chunks;
  bwtc::wavelet::gm::buildTasks(plan, coded_pos.data(), &tk, &chunks);
  *n_coded = total;
  *nt = (uint32_t)tk.size();
  if (!packed && !tasks && !w) return 0;                              // the sizes alone
  if (!packed || !tasks || !w || packed_words < ((uint64_t)total + 15) / 16 || tasks_cap < tk.size() || w_cap < total) return -1;
  for (uint64_t i = 0; i < ((uint64_t)total + 15) / 16; ++i) packed[i] = 0;
  std::memcpy(packed, codes.data(), std::min<size_t>(codes.size(), ((size_t)total + 3) / 4));
  for (size_t t = 0; t < tk.size(); ++t) { tasks[3 * t] = tk[t].begin; tasks[3 * t + 1] = tk[t].end; tasks[3 * t + 2] = tk[t].type; }
  // the sequential coder's models: group by group, the probability of a ONE per element -> w form
  codes.push_back(0);
  bwtc::wavelet::StreamCoder sc(plan, coded_pos.data(), codes.data(), *state, letter);
  std::vector<uint16_t> prob((size_t)total + 8, 0);
  for (size_t k = 0; k < sc.modelTasks(); ++k) sc.model(k, prob.data());
  for (uint32_t i = 0; i < total; ++i) {
    const uint32_t bit = (codes[i >> 2] >> ((i & 3u) * 2u)) & 1u;
    w[i] = (uint16_t)((bit << 15) | (bit ? prob[i] : 4096u - prob[i]));
  }
  *state = sc.endState();
  return 0;
}

int bwtc_hip_test_scan_u32(bwtc_hip_ctx* ctx, uint32_t* data, uint64_t n) {
  if (!ctx || !data) return -1;
  BwtEngine& e = ctx->eng;
  // the scan borrows R1 for the data and R2 for the tile partials
  if (n * 4 > e.cap * 8) return -1;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  u32* d = static_cast<u32*>(e.d_R1);
  BwtEngine::ScanScope scan_scope(e);                // the context's single-launch scan, where it is set up
  BWTC_HIP_TRY(hipMemcpyAsync(d, data, n * 4, hipMemcpyHostToDevice, e.stream));
  exclusive_scan_u32(d, n, static_cast<u32*>(e.d_R2), e.stream);
  BWTC_HIP_TRY(hipMemcpyAsync(data, d, n * 4, hipMemcpyDeviceToHost, e.stream));
  e.h_small[1] = 0;
  if (e.scan_chain.err) BWTC_HIP_TRY(hipMemcpyAsync(e.h_small + 1, e.scan_chain.err, 4, hipMemcpyDeviceToHost, e.stream));
  BWTC_HIP_TRY(e.wait());
  BWTC_HIP_TRY(hipGetLastError());
  return e.h_small[1] ? -3 : 0;
}

// ---- pair-replacing pre-stage (prepr.hip, prepr_host.cpp) ---------------------------------------------
bwtc_hip_grammar* bwtc_hip_grammar_create(void) { return new (std::nothrow) bwtc_hip_grammar(); }
void bwtc_hip_grammar_destroy(bwtc_hip_grammar* g) { delete g; }
uint32_t bwtc_hip_grammar_rules(const bwtc_hip_grammar* g) { return g ? g->g.numberOfRules() : 0; }
uint32_t bwtc_hip_grammar_special_symbols(const bwtc_hip_grammar* g) { return g ? g->g.numberOfSpecialSymbols() : 0; }
int bwtc_hip_grammar_is_special(const bwtc_hip_grammar* g, unsigned symbol) { return g && g->g.isSpecial(static_cast<uint8_t>(symbol)) ? 1 : 0; }
int bwtc_hip_grammar_write(const bwtc_hip_grammar* g, uint8_t* out, uint64_t cap, uint64_t* bytes) {
  if (!g || !out || !bytes) return -1;
  std::vector<uint8_t> v;
  g->g.write(&v);
  if (v.size() > cap) return -1;
  std::memcpy(out, v.data(), v.size());
  *bytes = v.size();
  return 0;
}
int bwtc_hip_grammar_read(bwtc_hip_grammar* g, const uint8_t* in, uint64_t n, uint64_t* consumed) {
  if (!g || !in || !consumed || g->g.numberOfRules() || g->g.numberOfSpecialSymbols()) return -1;
  const size_t used = g->g.read(in, static_cast<size_t>(n));
  if (used == static_cast<size_t>(-1)) return -1;
  *consumed = used;
  return 0;
}
int bwtc_hip_pair_replace_device(bwtc_hip_ctx* ctx, bwtc_hip_grammar* g, const uint8_t* d_src, uint64_t n,
                                 uint8_t* d_dst, uint64_t* n_out, uint32_t* replaced) {
  if (!ctx || !g || !d_src || !d_dst || !n_out || !replaced) return -1;
  return bwtc_hip::pair_replace_device(ctx->eng, g->g, d_src, n, d_dst, n_out, replaced);
}
int bwtc_hip_test_pair_stats(bwtc_hip_ctx* ctx, const uint8_t* d_src, uint64_t n, uint32_t* pair_cnt, uint32_t* byte_cnt) {
  if (!ctx || !d_src || !pair_cnt || !byte_cnt) return -1;
  std::vector<uint32_t> counts(65536 + 256);
  if (const int rc = bwtc_hip::pair_stats_device(ctx->eng, d_src, n, counts.data())) return rc;
  std::memcpy(pair_cnt, counts.data(), 65536 * 4);
  std::memcpy(byte_cnt, counts.data() + 65536, 256 * 4);
  return 0;
}
int bwtc_hip_host_precompress(bwtc_hip_grammar* g, const char* options, uint8_t* block, uint64_t n, uint64_t* n_out);
int bwtc_hip_precompress(bwtc_hip_ctx* ctx, bwtc_hip_grammar* g, const char* options, uint8_t* block, uint64_t n, uint64_t* n_out) {
  if (!ctx || !g || !block || !n_out) return -1;
  *n_out = n;
  if (!options || !options[0] || n < 3) return 0;
  BwtEngine& e = ctx->eng;
  BWTC_HIP_TRY(hipSetDevice(e.device));
  // The device passes index their tiles and output offsets with 32 bits: a precompressor block of 2 GiB and more (the
  // reference's PairReplacer takes them up to 4 GiB: `compress --prepr p -m 2903` and above) takes the host's twin of
  // the same two passes -- same bytes, same grammar.
  if (n >= (1ull << 31) || n / 4096 + 2 > e.cap) return bwtc_hip_host_precompress(g, options, block, n, n_out);
  uint8_t *d_a = nullptr, *d_b = nullptr;
  BWTC_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_a), 2 * n + 64));
  if (hipMalloc(reinterpret_cast<void**>(&d_b), 2 * n + 64) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d_a); return -2; }
  int rc = hipMemcpy(d_a, block, n, hipMemcpyHostToDevice) == hipSuccess ? 0 : -3;
  uint64_t length = n;
  for (const char* c = options; rc == 0 && *c; ++c) {            // Precompressor.cpp:76-105
    const uint64_t before = length;
    if (*c == 'p') {
      uint64_t now = 0;
      uint32_t replaced = 0;
      rc = bwtc_hip::pair_replace_device(e, g->g, d_a, length, d_b, &now, &replaced);
      if (rc) break;
      std::swap(d_a, d_b);
      length = now;
    }
    if (length == before || length < 3) break;
  }
  if (rc == 0 && hipMemcpy(block, d_a, length, hipMemcpyDeviceToHost) != hipSuccess) rc = -3;
  (void)hipFree(d_a);
  (void)hipFree(d_b);
  if (rc == 0) *n_out = length;
  return rc;
}
int bwtc_hip_host_precompress(bwtc_hip_grammar* g, const char* options, uint8_t* block, uint64_t n, uint64_t* n_out) {
  if (!g || !block || !n_out) return -1;
  *n_out = n;
  if (!options || !options[0] || n < 3) return 0;
  std::vector<uint8_t> other(2 * n + 64);
  std::vector<uint64_t> bf(256), pf(65536);
  uint64_t length = n;
  for (const char* c = options; *c; ++c) {
    const uint64_t before = length;
    if (*c == 'p') {
      bwtc::prepr::pairStatisticsOnHost(block, length, bf.data(), pf.data());
      bwtc::prepr::Replacements r;
      bwtc::prepr::decideReplacements(&g->g, bf.data(), pf.data(), &r);
      if (r.count) {
        length = bwtc::prepr::writeReplacedOnHost(r, block, length, other.data());
        std::memcpy(block, other.data(), length);
      }
    }
    if (length == before || length < 3) break;
  }
  *n_out = length;
  return 0;
}
int bwtc_hip_postprocess(const bwtc_hip_grammar* g, const uint8_t* data, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* n_out) {
  if (!g || (!data && n) || !out || !n_out) return -1;
  std::vector<uint8_t> v;
  if (!bwtc::prepr::postprocess(g->g, data, static_cast<size_t>(n), &v, static_cast<size_t>(cap))) return -1;
  if (!v.empty()) std::memcpy(out, v.data(), v.size());
  *n_out = v.size();
  return 0;
}

static PostProcessor* postprocessor(bwtc_hip_ctx* ctx) {
  if (!ctx->post) ctx->post = postprocessor_create();
  return ctx->post;
}
int bwtc_hip_postprocess_device(bwtc_hip_ctx* ctx, const bwtc_hip_grammar* g, const uint8_t* d_data, uint64_t n, uint8_t* d_out,
                                uint64_t cap, uint64_t* n_out) {
  if (!ctx || !g || (!d_data && n) || !d_out || !n_out) return -1;
  PostProcessor* p = postprocessor(ctx);
  if (!p) return -2;
  return postprocess_device(ctx->eng, *p, g->g, d_data, n, d_out, cap, n_out);
}
int bwtc_hip_postprocess_block(bwtc_hip_ctx* ctx, const bwtc_hip_grammar* g, const uint8_t* data, uint64_t n, uint8_t* out,
                               uint64_t cap, uint64_t* n_out) {
  if (!ctx || !g || (!data && n) || !out || !n_out) return -1;
  PostProcessor* p = postprocessor(ctx);
  if (!p) return -2;
  return postprocess_block(ctx->eng, *p, g->g, data, n, out, cap, n_out);
}
int bwtc_hip_postprocess_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_postprocess_stats* out) {
  if (!ctx || !out) return -1;
  return postprocessor_stats(ctx->post, out);
}
int bwtc_hip_host_postprocess_tiles(const bwtc_hip_grammar* g, const uint8_t* data, uint64_t n, uint8_t* out, uint64_t cap,
                                    uint64_t* n_out, uint32_t tile) {
  if (!g || (!data && n) || !out || !n_out || tile == 0) return -1;
  if (g->g.numberOfRules() == 0) {
    if (n > cap) return -1;
    if (n) std::memcpy(out, data, n);
    *n_out = n;
    return 0;
  }
  bwtc::prepr::ExpansionTable t;
  if (!bwtc::prepr::buildExpansionTable(g->g, static_cast<size_t>(cap), &t)) return -1;
  const int64_t total = bwtc::prepr::postprocessTilesOnHost(t, data, static_cast<size_t>(n), out, static_cast<size_t>(cap), tile);
  if (total < 0) return -1;
  *n_out = static_cast<uint64_t>(total);
  return 0;
}

}  // extern "C"
