// BwtEngine: device-resident Burrows-Wheeler transform of one block on one MI355X.
//
// Replaces the work of Divsufsorter / SAISBWTransform behind
// BWTransform::doTransform (bwtransforms/BWTransform.hpp:53-58, BWTransform.cpp:52-64):
// suffix sort of T = reverse(block) + '\0' under "proper prefix sorts first", BWT
// emission with the reference's end-of-block and LFpowers conventions
// (bwtransforms/divsufsort.c:328-404,480-522) and the 256-bin histogram.
//
// Algorithm (integer / index work, HBM-bound, no MFMA):
//   1. load+reverse+histogram, 4-byte big-endian keys            (streaming)
//   2. LSD radix sort of (key32, suffix) pairs                   (radix_sort.hpp)
//   3. ranking: group heads -> rank[], singleton suffixes are final, the rest is
//      compacted into the active list (suffix, global slot, dense group id)
//   4. prefix doubling with discarding: per round gather rank[s+h], radix sort the active
//      list by (group, rank[s+h]), re-rank, compact; stop when nothing is active
//   5. BWT gather T[SA-1], end-of-block patch, LF powers from the final rank[] (= ISA)
#pragma once
#include "common.hpp"
#include "bwtc_hip.h"
#include "radix_sort.hpp"
#include "scan.hpp"
#include "wavelet_host.hpp"
#include "wavelet_pipeline.hpp"
#include <sys/mman.h>
#include <condition_variable>
#include <future>
#include <map>
#include <mutex>
#include <thread>
#include <memory>
#include <utility>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace bwtc { namespace wavelet { namespace gm { struct Task; struct Chunk; } } }   // wavelet_gpu_models.hpp

namespace bwtc_hip {

struct RrEmit;
struct RrLong;
struct FinList;
struct FinShallow;
struct InitialSort;
struct SortList;
struct RankRequest;
struct FinWork;
struct FinRequest;
// what finisher_passes left: entries of groups too large for a window (and their smallest depth), entries its last pass left
// tied and parked, entries handed to the local list, entries of the shallow list (and their smallest depth)
struct FinOutcome { u32 hard = 0, hard_depth = 0xFFFFFFFFu, left = 0, local = 0, shallow = 0, shallow_depth = 0xFFFFFFFFu; };
// A finisher list lives in up to kFinRegions regions of its arrays (bwt_engine.hip, k_finish)
constexpr u32 kFinRegions = 16;
constexpr u32 kPeriodMax = 4096;   // the longest period the period step looks for (bwt_engine.hip, "Periods")
constexpr u32 kLongPeriodMax = 1u << 24;   // ... and the longest under BWTC_HIP_LONG_PERIODS (bwt_engine.hip, "Long periods")
constexpr u32 kPeriodCandidates = 8;  // the distances the finder returns under BWTC_HIP_MULTI (k_period_winners)
struct FinRegions { u32 nreg; u32 wfirst[kFinRegions + 1]; u32 ebase[kFinRegions]; u32 ecount[kFinRegions]; };

// 256 bytes of canary behind the last item a test hook's kernels may write (c_abi.hip, BwtEngine::test_finish_pass): a
// changed canary is kBase - (index in the order they were put).
struct TestCanaries {
  static constexpr size_t kBytes = 256;
  static constexpr int kBase = -20, kMax = 16;
  u8 pat[kBytes];
  u8 back[kMax][kBytes];
  const u8* at[kMax];
  int count = 0;
  TestCanaries() { for (size_t i = 0; i < kBytes; ++i) pat[i] = (u8)(0xC3u ^ (i * 29u)); }
  hipError_t put(void* buf, u64 bytes, hipStream_t st) {
    if (count >= kMax) return hipErrorInvalidValue;     // (no room to remember another one: the hook fails, nothing is guarded less)
    u8* p = static_cast<u8*>(buf) + bytes;
    at[count++] = p;
    return hipMemcpyAsync(p, pat, kBytes, hipMemcpyHostToDevice, st);
  }
  hipError_t fetch(hipStream_t st) {
    for (int i = 0; i < count; ++i) {
      const hipError_t rc = hipMemcpyAsync(back[i], at[i], kBytes, hipMemcpyDeviceToHost, st);
      if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
  }
  int verdict() const {                                 // after the stream has been waited for
    for (int i = 0; i < count; ++i) if (std::memcmp(back[i], pat, kBytes) != 0) return kBase - i;
    return 0;
  }
};

typedef bwtc_hip_fin_pass FinPassTest;   // one k_finish launch for the test hooks (bwtc_hip.h; BwtEngine::test_finish_pass)

// ---- device side of the 'B' block pipeline (host side: wavelet_pipeline.hpp) ----------------
// Page-locked host bytes: the packed streams are copied from the device straight into the
// block's own buffer.  Recycled between blocks (locking pages is slow), contents lost on growth.
// Where the system will not lock that many pages (96 blocks under way hold 12 GB per context) the
// bytes are ordinary memory: the copy is then staged by the runtime, slower but the same bytes.
struct PinnedGauge {                                // bytes of host staging held by this process, now and at most
  std::atomic<uint64_t> now{0}, peak{0};
  void add(uint64_t n) {
    const uint64_t v = now.fetch_add(n) + n;
    uint64_t p = peak.load();
    while (p < v && !peak.compare_exchange_weak(p, v)) {}
  }
  void sub(uint64_t n) { now.fetch_sub(n); }
  static PinnedGauge& get() { static PinnedGauge g; return g; }
};

// Page-locked host memory, the fast way: an anonymous mapping of transparent huge pages, touched by the
// calling thread (on its own NUMA node, outside the driver), then registered -- 50 ms per 1.2 GB where
// hipHostMalloc takes 200 ms, most of it under the driver's lock, and 130 ms more to free
// (scripts/dev/pin_bench.cpp; the copies run at the same 57 GB/s).  Only for buffers of 32 MiB and more
// (the w-elements and staging buffers of full-size blocks): a mapping of its own, never memory carved
// from the allocator's heap, so nothing else ever lives in, next to or after a registered range.
// *kind: 2 registered mapping, 1 hipHostMalloc, 0 nothing could be locked.
constexpr size_t kLockedHugePage = (size_t)2 << 20;
constexpr size_t kLockedMapFrom = (size_t)32 << 20;
inline size_t lockedMapBytes(size_t n) { return (n + kLockedHugePage - 1) / kLockedHugePage * kLockedHugePage; }
inline void* lockedHostAlloc(size_t n, int* kind) {
  void* q = nullptr;
  if (n >= kLockedMapFrom && !std::getenv("BWTC_HIP_NO_HUGE_PAGES")) {
    const size_t bytes = lockedMapBytes(n);
    // over-map by one huge page and trim to a 2 MiB boundary
    void* raw = mmap(nullptr, bytes + kLockedHugePage, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (raw != MAP_FAILED) {
      const uintptr_t r = reinterpret_cast<uintptr_t>(raw);
      const uintptr_t al = (r + kLockedHugePage - 1) / kLockedHugePage * kLockedHugePage;
      if (al > r) (void)munmap(raw, al - r);
      const size_t tail = (r + bytes + kLockedHugePage) - (al + bytes);
      if (tail) (void)munmap(reinterpret_cast<void*>(al + bytes), tail);
      q = reinterpret_cast<void*>(al);
      (void)madvise(q, bytes, MADV_HUGEPAGE);
      for (size_t i = 0; i < bytes; i += 4096) static_cast<volatile char*>(q)[i] = 0;
      // Huge pages only where the first touch got them: from here on the range is left alone (no later
      // collapse by khugepaged under a registered range -- the device's mapping of a page that the kernel
      // is replacing is what round 3's write fault looked like).
      (void)madvise(q, bytes, MADV_NOHUGEPAGE);
      if (hipHostRegister(q, bytes, hipHostRegisterDefault) == hipSuccess) {
        if (std::getenv("BWTC_HIP_DEBUG")) std::fprintf(stderr, "pinned: registered [%p, %p) (%zu MiB, mapping of its own)\n", q, static_cast<char*>(q) + bytes, bytes >> 20);
        *kind = 2;
        return q;
      }
      (void)hipGetLastError();
      (void)munmap(q, bytes);
      q = nullptr;
    }
  }
  if (hipHostMalloc(&q, n ? n : 1, hipHostMallocDefault) == hipSuccess) { *kind = 1; return q; }
  (void)hipGetLastError();                         // not an error of the caller's stream
  *kind = 0;
  return nullptr;
}
// `n`: the size the buffer was asked for (kind 2 needs it to unmap)
inline void lockedHostFree(void* p, int kind, size_t n) {
  if (!p) return;
  if (kind == 2) {
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return; }   // still known to the device: the mapping stays
    if (std::getenv("BWTC_HIP_DEBUG")) std::fprintf(stderr, "pinned: unregistered and unmapped [%p, %p)\n", p, static_cast<char*>(p) + lockedMapBytes(n));
    (void)munmap(p, lockedMapBytes(n));
  } else if (kind == 1) (void)hipHostFree(p);
  else std::free(p);
}

class PinnedBytes {
 public:
  PinnedBytes() : p_(nullptr), n_(0), locked_(0) {}
  ~PinnedBytes() { release(); }
  PinnedBytes(const PinnedBytes&) = delete;
  PinnedBytes& operator=(const PinnedBytes&) = delete;
  void swap(PinnedBytes& o) { std::swap(p_, o.p_); std::swap(n_, o.n_); std::swap(locked_, o.locked_); }
  bool reserve(size_t n) {
    if (n <= n_) return true;
    release();
    void* q = lockedHostAlloc(n + n / 8, &locked_);
    if (!q) {
      if (std::getenv("BWTC_HIP_DEBUG")) std::fprintf(stderr, "PinnedBytes: %zu bytes could not be page-locked, using ordinary memory\n", n + n / 8);
      q = std::malloc(n + n / 8);
      if (!q) return false;
    }
    p_ = static_cast<uint8_t*>(q);
    n_ = n + n / 8;
    PinnedGauge::get().add(n_);
    return true;
  }
  uint8_t* data() { return p_; }
  size_t size() const { return n_; }
 private:
  void release() {
    if (p_) { lockedHostFree(p_, locked_, n_); PinnedGauge::get().sub(n_); }
    p_ = nullptr; n_ = 0;
  }
  uint8_t* p_;
  size_t n_;
  int locked_;                                   // see lockedHostAlloc
};

// Page-locked buffers of one size class, recycled between blocks.  Locking a gigabyte of pages
// takes 60 ms: once blocks overlap, a helper thread allocates a few buffers AHEAD of the thread that
// feeds the GPU (never more than `limit` in all), so that a stream's first blocks do not each stop
// for it.
class PinnedPool {
 public:
  ~PinnedPool() { stop(); }
  // a recycled (or pre-allocated) buffer, if there is one
  bool take(PinnedBytes* into) {
    std::lock_guard<std::mutex> g(mu_);
    if (free_.empty()) return false;
    into->swap(*free_.back());
    free_.pop_back();
    cv_.notify_all();
    return true;
  }
  void give(PinnedBytes* from, size_t keep_at_most) {
    std::lock_guard<std::mutex> g(mu_);
    if (from->size() && free_.size() < keep_at_most) {
      free_.push_back(std::unique_ptr<PinnedBytes>(new PinnedBytes()));
      free_.back()->swap(*from);
    }
  }
  // the caller allocated one itself (counts against the limit of the helper)
  void noteAllocated() { std::lock_guard<std::mutex> g(mu_); ++made_; }
  // from now on keep up to four spare buffers of `bytes` ready, `limit` buffers in all
  void allocateAhead(int device, size_t bytes, unsigned limit) {
    std::lock_guard<std::mutex> g(mu_);
    if (running_ || bytes == 0) return;
    running_ = true; quit_ = false;
    helper_ = std::thread([this, device, bytes, limit] {
      (void)hipSetDevice(device);
      std::unique_lock<std::mutex> l(mu_);
      while (!quit_ && made_ < limit) {
        if (free_.size() >= 4) { cv_.wait(l); continue; }
        l.unlock();
        std::unique_ptr<PinnedBytes> b(new PinnedBytes());
        const bool ok = b->reserve(bytes);
        l.lock();
        if (!ok) break;
        ++made_;
        free_.push_back(std::move(b));
      }
    });
  }
  void stop() {
    { std::lock_guard<std::mutex> g(mu_); quit_ = true; cv_.notify_all(); }
    if (helper_.joinable()) helper_.join();
    std::lock_guard<std::mutex> g(mu_);
    running_ = false;
  }
  void clear() { stop(); std::lock_guard<std::mutex> g(mu_); free_.clear(); made_ = 0; }
  // the stream needs fewer buffers than were made: the spare ones above `keep` go back to the system
  void trim(size_t keep) {
    std::lock_guard<std::mutex> g(mu_);
    while (free_.size() > keep) { free_.pop_back(); if (made_) --made_; }
  }
 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<PinnedBytes> > free_;
  std::thread helper_;
  unsigned made_ = 0;
  bool running_ = false, quit_ = false;
};

// The model passes of one block between their two parts (wavelet_gpu_models.hip): where its tables
// and intermediates live in the context's workspace.
struct GmPass {
  bool ready = false;
  const u32* d_packed = nullptr;
  u32 n_coded = 0, nt = 0, nc = 0, ns = 0, nsc = 0, ntiles = 0, gsize = 0, ng = 0;
  u64 n_base = 0;
  void *d_tasks = nullptr, *d_chunks = nullptr, *d_order = nullptr, *d_excl = nullptr, *d_tagg = nullptr, *d_tstate = nullptr,
       *d_cmap = nullptr, *d_cstate = nullptr, *d_base = nullptr, *d_partial = nullptr, *d_sb = nullptr, *d_sbits = nullptr,
       *d_smap = nullptr, *d_sstart = nullptr, *d_gmap = nullptr, *d_gL = nullptr, *d_tg = nullptr, *d_snaps = nullptr,
       *d_tail = nullptr;
  u32 ends[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // the carried state after the block, by the state it starts in
  bool ends_ready = false;
  void* side = nullptr;                        // the stream the passes run on when it is not the context's (wavelet_models_device)
  u32 kind = 0;                                // the main model the passes were prepared for (gm::kKindB / kKindb / kKindu)
};

// A block of the pipeline whose streams came from this device: owns the page-locked bytes.
struct WaveletSectionStats;
struct DeviceWaveletJob : WaveletJob {
  ~DeviceWaveletJob() { if (plan_future.valid()) plan_future.wait(); }   // the planner reads this object
  PinnedBytes codes_owner;
  PinnedBytes w_owner;                 // device-modelled blocks: the w-elements (2 bytes per coded element)
  u32* h_tail = nullptr;               //   {state after the block, error flags, elements counted} (in w_owner, behind the elements)
  u32 gm_state_in = 0;                 //   the carried state the device passes were given
  char gm_letter = 'B';                //   the main model the device passes were made for: the block's, whatever the context's becomes
  GmPass gm;                           // farmed streams: the passes' first part is done, the rest waits for the state (_queue)
  // between wavelet_encode_prepare and wavelet_encode_queue
  bool streams_ready = false;          // plan + coded_pos + codes are in place for HostPipeline::queue
  bool host_route = false;             // coded by encodeSections at queue time instead
  bool queued = false;
  bool joins_from_callback = false;    // farmed stream: the block joins the host pipeline from a callback on the d2h stream
  std::atomic<bool> callback_seen{false};
  bool half = false;                   // scanned and (being) planned; streams not made yet
  bool copying = false;                // streams made, their copy to the host may still be in flight
  int run_buf = 0;                     // which of the engine's run-array buffers holds its runs
  u32 block_size = 0;
  std::future<bool> plan_future;       // planStreams on a helper thread
  std::vector<bwtc::wavelet::SectionRuns> host_secs;
  std::vector<u8> host_run_sym;
  std::vector<u32> host_run_start;
  std::shared_ptr<WaveletSectionStats> host_stats;
  unsigned host_threads = 0;
};

struct KeyPlan;
struct BwtEngine {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;   // uploads that overlap the kernels (bwtc_hip_memcpy_to_device_async)
  hipEvent_t ev_copy = nullptr;
  hipStream_t d2h_stream = nullptr;    // packed wavelet streams to the host, under the next block's transform
  hipEvent_t ev_packed = nullptr, ev_codes = nullptr, ev_models = nullptr;
  bool codes_in_flight = false;
  hipError_t ensure_d2h_stream();
  hipError_t codes_wait();             // the copy issued by wavelet_streams_device(async_copy) has landed
  u32 max_block = 0;     // largest block size in bytes
  u64 cap = 0;           // suffix capacity = max_block + 1

  // device workspace
  void* arena = nullptr;
  u64 arena_bytes = 0;
  u8* d_T = nullptr;       // cap + 32
  u8* d_out = nullptr;     // cap + 32
  u8* d_in = nullptr;      // staging for host blocks: cap + 32
  u32* d_SA = nullptr;     // cap
  u32* d_rank = nullptr;   // cap
  void* d_R1 = nullptr;    // 8*cap : K32a|K32b, later K64a
  void* d_R2 = nullptr;    // 8*cap : K64b
  u32* d_V0 = nullptr;     // cap
  u32* d_V1 = nullptr;     // cap
  u32* d_G0 = nullptr;     // cap
  u32* d_G1 = nullptr;     // cap
  u32* d_GRP = nullptr;    // cap
  u8* d_C0 = nullptr;      // cap : carried characters of the active list (ping-pong)
  u8* d_C1 = nullptr;
  u8* d_P0 = nullptr;      // cap : digit planes of the radix passes (radix_sort.hpp)
  u8* d_P1 = nullptr;
  u32* d_W0 = nullptr;     // cap : second key words of the long-key initial sort (ping-pong)
  u32* d_W1 = nullptr;
  u32* d_table = nullptr;  // radix tables
  u32* d_partial = nullptr;
  u32* d_aggA = nullptr;   // rerank tile aggregates
  u32* d_aggB = nullptr;
  u32* d_aggC = nullptr;
  u32* d_agg_part = nullptr;   // totals per 4096 tile aggregates (k_rerank_scan_tiles)
  u32* d_sweep = nullptr;  // chained radix sort: histograms, bases, tickets (SweepWs::small_words)
  bool use_sweep = false;  // BWTC_HIP_SORT=sweep selects the chained single-read passes (measured
                           // slower on MI355X than the XCD-contiguous three-kernel passes)
  u8* d_comp = nullptr;    // compressed-block staging, huffman_compress_bound(max_block)
  u8* d_ent = nullptr;     // 2 MiB of small tables for the entropy front-end
  u32* d_small = nullptr;  // [0..255] freqs, [256..511] lf, [512] pidx, [520..521] counts
  u32* h_small = nullptr;  // pinned mirror of d_small
  u8* h_stage = nullptr;   // pinned staging, cap + 32
  void* d_wt = nullptr;    // wavelet stream workspace, sized by the block's step count (wavelet_tree.hip)
  u64 wt_bytes = 0;
  u8* h_wt = nullptr;      // pinned: tables up, packed streams down
  u64 h_wt_bytes = 0;
  u8* h_stats = nullptr;   // pinned: the run scanner's statistics come down in two copies and one wait
  u64 h_stats_bytes = 0;
  int reserve_stats(u64 bytes);
  // the adaptive models on the device (wavelet_gpu_models.hip): tables and slot space, the
  // w-elements of the block whose copy to the host is under way, pinned staging for the tables
  void* d_gm = nullptr;  u64 gm_bytes = 0;
  void* d_gm_w = nullptr; u64 gm_w_bytes = 0;
  u8* h_gm = nullptr;    u64 h_gm_bytes = 0;
  hipStream_t gm_stream = nullptr;     // the model passes of the _begin flow: beside the next block's transform
  hipEvent_t ev_packed_ready = nullptr, ev_gm_done = nullptr;
  bool gm_done_pending = false;        // the main stream must wait for ev_gm_done before the packed streams' workspace is written again
  bool models_side_stream = true;      // BWTC_HIP_MODELS_STREAM=0: the passes stay on the context's stream (round 4)
  hipEvent_t ev_gm_upload = nullptr;   // the tables' upload from h_gm has finished (the next block may fill h_gm)
  bool gm_upload_pending = false;
  int reserve_models(u64 device_bytes, u64 host_bytes, u64 w_bytes);
  ScanChain scan_chain;                // single-launch scans (scan.hpp): BWTC_HIP_SCAN=chained switches them on (slower here)
  // while alive, the calling thread's scans go through this context's chain
  struct ScanScope {
    ScanChain* prev;
    explicit ScanScope(BwtEngine& e) : prev(current_scan_chain()) { current_scan_chain() = e.scan_chain.status ? &e.scan_chain : nullptr; }
    ~ScanScope() { current_scan_chain() = prev; }
  };
  bool device_models = true;           // BWTC_HIP_MODELS=host: the models stay on the worker threads (all routes of round 2)
  bool letter_models = false;          // BWTC_HIP_LETTER_MODELS=1: the models of 'b' and 'u' blocks on the device too
  // this letter's models run on the device
  bool models_on_device(char letter) const {
    return device_models && (letter == 'B' || (letter_models && (letter == 'b' || letter == 'u')));
  }
  std::vector<u32> long_count;   // host scratch of the run statistics: counts of long run lengths, all zero between calls
  // blocks of the 'B' coder between _begin and _end (wavelet_pipeline.hpp)
  // run arrays of the 'B' coder's scanner, two buffers: block i is scanned while block i-1's runs still
  // wait for their stream kernels (wavelet_encoder.hip)
  u32* d_run_start[2] = {nullptr, nullptr};
  u8* d_run_sym[2] = {nullptr, nullptr};
  int next_run_buf = 0;
  int reserve_run_arrays();
  std::shared_ptr<DeviceWaveletJob> half_job;   // scanned + planned, its streams still to be made
  std::shared_ptr<DeviceWaveletJob> copy_job;   // streams made, copy to the host in flight, not queued yet (_begin flow)
  std::weak_ptr<DeviceWaveletJob> gm_pending;   // _prepare / _queue flow: the job whose model passes wait in the workspace for their state
  bool deferred_queue = false;        // _begin is in use: a begun block joins the stream one or two calls later
  bool async_streams_copy = false;    // set by _begin around its _prepare
  WaveletRoutes routes;               // which route each wavelet block took (bwtc_hip_wavelet_routes)
  HostPipeline* pipeline = nullptr;   // worker threads, lane engines, coder tasks ('B'; made by the first block)
  std::vector<int> worker_cpus;       // bwtc_hip_set_worker_cpus: where those threads may run (empty: anywhere)
  std::map<u64, std::shared_ptr<DeviceWaveletJob> > jobs;
  u64 next_ticket = 1;
  unsigned max_inflight = 16;          // BWTC_HIP_WAVELET_DEPTH
  u64 huge_group_elements = 32u << 20; // BWTC_HIP_HUGE_MI: groups this large are modelled by scalar tasks, not lanes
  PinnedPool codes_pool, w_pool;                                       // recycled: no fresh pages per block
  std::vector<std::unique_ptr<RawBuffer<uint16_t> > > prob_free;
  u64 wt_elements = 0, wt_coded = 0;   // steps / coded elements of the last block
  bool gm_partition_lines = false;     // BWTC_HIP_GM_PARTITION=lines: the model passes' partition assembled in LDS and stored as whole lines
  bool wt_segmented = true;            // BWTC_HIP_SEG_STEPS=0: the 'B' coder's step sort over block-wide group numbers (three passes)
  bool wavelet_on_host = false;        // BWTC_HIP_WAVELET=host: build the trees on the host instead

  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  hipEvent_t ev_wait = nullptr;        // blocking-sync event (hipEventBlockingSync)
  int wait_mode = 0;                   // 0 auto: block while the 'B' worker pool exists, spin otherwise; 1 spin; 2 block (BWTC_HIP_SYNC)
  // Waits for the context's stream.  hipStreamSynchronize spins, which costs the calling thread
  // (and a runtime helper thread) a CPU or two for the whole device time of a block; harmless
  // when nothing else runs, but the 'B' coder's worker threads need those CPUs, so the wait then
  // sleeps on an interrupt instead.
  hipError_t wait();
  static constexpr int kWaitSlots = 64;
  float wait_us[kWaitSlots] = {};      // how long each of a block's waits took for the previous blocks (sleepy_wait)
  int wait_seq = 0;
  hipError_t sleepy_wait(hipEvent_t ev, int slot);
  static constexpr int kMaxSortEvents = 160;
  hipEvent_t ev_sort[kMaxSortEvents];
  int n_sort_events = 0;

  bwtc_hip_stats stats;
  int stream_start_error = 0;   // bwtc_hip_wavelet_start / _reset could not let the old stream's blocks join: the next _begin / _prepare says so
  u32 wavelet_state = 4;   // FSM8 state carried from block to block by one WaveletEncoder
  char wavelet_model = 'B'; // coder letter = main probability model ('B', 'b' or 'u')
  ScatterProbe probe;

  static u64 workspace_bytes(u32 max_block);
  int init(int dev, u32 max_block_size);
  void release();
  int reserve_wavelet(u64 device_bytes, u64 host_bytes);

  // Sorts the suffixes of d_T[0..n-1]; on return d_SA holds the suffix array and d_rank
  // its inverse.  d_T must be followed by >= 8 zero bytes.
  // hist = byte histogram of d_T[0..n-1] (drives the width of the initial sort key).
  // em != nullptr: instead of storing the suffix array the ranking kernels write the
  // transform's bytes, out[slot] = T[SA[slot]-1] for slot < out_n, as suffixes become final
  // (blocks for which can_carry() holds only; see k_rerank_apply).  allow_code_keys == false: the block's second go, with gram keys.
  struct EmitTarget { u8* out; u32 out_n; u32 n_lf; };
  int suffix_sort(u32 n, const u32* hist, bool lone_sentinel, const EmitTarget* em = nullptr, bool allow_code_keys = true);
  // A period as weigh_period leaves it: the period behind the division (0: refused), its longest stretch, its longest
  // proper stretch (0: no pass made it) and the candidate's votes.  The worth tests go by the proper stretch under
  // BWTC_HIP_MIXED's rule (BwtEngine::mixed_rule), else by the longest.
  struct WeighedPeriod { u32 p = 0, longest = 0, proper = 0, votes = 0; u32 gate(bool mixed) const { return mixed ? proper : longest; } };
  // A closed-form step (runs and periods, below): its period (1: the run step), when it is due (kWaiting: the first doubling
  // round whose depth reaches p; kNone: not any more), the depth it ran at (0: it has not), and whether it ranked the runs
  // too (BWTC_HIP_MIXED: the first round is one period step over k_p[] in place of the run step that was due).  Its facts,
  // from the moment it is scheduled and under every switch: the longest stretch of its period (the run step: the longest
  // run), the longest proper stretch and the finder's votes for it; dropped says that its gate was shut when its depth came.
  struct StretchStep { u32 p = 0; enum When { kNone, kThisRound, kWaiting } when = kNone; u32 depth = 0; bool ranks_runs = false;
                       u32 longest = 0, proper = 0, votes = 0; bool dropped = false;
                       // the length bwtc_hip_schedule_get and the merged block's debug line show as the entry's gate
                       u32 shown_gate(bool mixed) const { return p == 1 || !mixed ? longest : proper; } };
  // The finder's candidates (find_period), most votes first: n of them reach the threshold.  at[0] also holds what the
  // finder says of a leader below it: the winner's pair as k_period_winner and the long finder leave it, zeros under
  // BWTC_HIP_MULTI's short finder (k_period_winners names nothing below the threshold); a forced period has no votes.
  struct PeriodCandidates { u32 n = 0; struct { u32 p, votes; } at[kPeriodCandidates] = {}; };
  // This block's state: suffix_sort begins a block by assigning BlockSort{} (so does test_finisher), and nothing else resets it.
  struct BlockSort {
    bool ranks_live = false;   // rank[] has been completed (every ranking step keeps it exact from then on)
    bool fin_active = false;   // the block takes the finisher route: finished suffixes also go to d_SA
    bool lf_noted = false;     // the LF powers were noted as suffixes became final (rank[] is not complete)
    // the finisher's state (bwt_engine.hip, finisher_route): the waiting list, the passes' shape, the local list
    struct Finisher {
      u32 parked = 0;            // entries waiting in d_parkS / d_parkHP
      u32 park_holes = 0;        //   of which empty (all ones: they sort to the list's end)
      // the passes' shape (finisher_passes and local_pass must agree: the local list's groups are as large as the passes left them):
      int window = 1024, group = 256;   // set by finisher_shape before the passes, by FinKnobScope for a test hook
      u32 stride() const { return (u32)(window - group); }   // entries whose groups a workgroup owns
      // the local list (deep repeats in small groups, doubled group by group beside the global list: bwt_engine.hip, local_pass)
      u32 local_m = 0, local_depth = 0; int local_home = 0, passes_done = 0; bool local_pending = false;
      FinRegions local_rg = {}, local_upd = {};   // where the local list lives now; where the last pass's notes lie
    } fin;
    u32 lengths_period = 0;    // the period d_runK's lengths were made for (0: none yet)
    u32 run_longest = 0;       // the longest run, once a pass of period 1 has found it (made at most once per block)
    // What bwtc_hip_period_get and bwtc_hip_steps_get report beside the steps, and say_no_period_step's line: the period the
    // block's first period step is for, or, where none was accepted, p = 0 with the lengths of the last pass over a
    // candidate and the leader's votes (decide_step)
    WeighedPeriod weighed;
    // The block's closed-form steps in the order it takes them (decide_step): the run step, then one period step, or
    // either alone; with BWTC_HIP_MULTI the run step and up to three period steps, the first round's before those that
    // wait, by ascending period.  `current` is the entry whose lengths went into d_runK last and whose period and depth the
    // second keys take (RunKeys): the front, until a step behind it comes due (step_due).
    static constexpr int kMaxSteps = 4, kMaxPeriodSteps = 3;
    StretchStep steps[kMaxSteps]; int n_steps = 0, current = 0;
    void schedule(const WeighedPeriod& w, StretchStep::When when) {
      if (n_steps < kMaxSteps) steps[n_steps++] = StretchStep{w.p, when, 0, false, w.longest, w.proper, w.votes};
    }
    // The length the gate of waiting entry i goes by when its depth comes (step_due).  Merged steps and a step behind the
    // run step: the longest proper stretch -- a run is no stretch there.  One waiting step at the front: the longest
    // stretch, even where BWTC_HIP_MIXED's rule decided it by the proper one (no run step is due, so none is in its way).
    u32 due_gate(int i) const { return merged || i > 0 ? steps[i].proper : steps[i].longest; }
    // ... and the length its debug line shows as the longest stretch: an unmerged block's is the longest, behind a run step too
    u32 said_longest(const StretchStep& s) const { return merged ? s.proper : s.longest; }
    // BWTC_HIP_MULTI: d_runK holds merged look-up words (tests/multimodel.py), not one period's lengths.  merged: this
    // block's steps merge; merged_stored: a storing pass has written the words (the next one is not the first);
    // merged_ran: a step has run over them, so every round's second keys read them.
    bool merged = false, merged_stored = false, merged_ran = false;
    int period_steps_ran() const { int c = 0; for (int i = 0; i < n_steps; ++i) c += steps[i].p >= 2 && steps[i].depth; return c; }
    void set_step(const StretchStep& s) { steps[0] = s; n_steps = 1; current = 0; }   // the one step, in place of whatever was scheduled
    StretchStep& current_step() { return steps[current]; }                           // (no step scheduled: one of period 0 and depth 0)
    // what the block's steps did, for bwtc_hip_period_get, bwtc_hip_steps_get and the debug line: the depth the runs were
    // ranked at (0: they were not), and the period step that ran (period and depth 0: none did)
    u32 run_depth() const { for (int i = 0; i < n_steps; ++i) if (steps[i].p == 1 || steps[i].ranks_runs) return steps[i].depth; return 0; }
    StretchStep period_ran() const { for (int i = 0; i < n_steps; ++i) if (steps[i].p >= 2 && steps[i].depth) return steps[i]; return StretchStep{}; }
    // BWTC_HIP_COPIES (bwt_engine.hip, "Copies"): a pass is taken every round that may until one finds a longest K below its
    // round's depth (the gate shuts); rounds: those whose look-ups went by K[]; first_depth: the depth of the first of them
    struct Copies { bool open = true; u32 passes = 0, rounds = 0, longest = 0, first_depth = 0; } copies;
    bool step_in_play() const { for (int i = 0; i < n_steps; ++i) if (steps[i].depth || steps[i].when != StretchStep::kNone) return true; return false; }
  } blk;
  // radix sort front door: picks the chained single-read passes or the classic ones
  template <typename K>
  void sort_pairs(K* k0, K* k1, u32* v0, u32* v1, u64 n, int nbits, K** ks, u32** vs, bool probe_it, int bit_lo = 0, u64 n_holes = 0, bool plane_ready = false, bool values_descend = false);
  // one ranking step of the suffix sorter (bwt_engine.hip)
  // Where a list lives between the steps: its sorted keys (u32 or u64, inside the 8 * cap-byte region rec_keys, which is
  // free once a step's apply kernel has run) and values, the region and the value array nobody uses, the list's slots by
  // position and the array the next list's slots go to.  A step writes what stays active raw into (v_free, slots_next,
  // d_GRP) -- suffix, slot, head slot -- and sorts the next list between the two regions and the two value arrays.
  struct ListHome {
    const void* keys; void* rec_keys; void* rec_free; u32* vals; u32* v_free; u32* slots; u32* slots_next;
    // a list that lies in the first of each pair
    static ListHome at(void* rec, void* rec_free, u32* vals, u32* v_free, u32* slots, u32* slots_next) { return ListHome{rec, rec, rec_free, vals, v_free, slots, slots_next}; }
    // a sort between the two regions and the two value arrays ended in (ks, vs): their partners are the free ones now
    ListHome& sorted_into(const void* ks, u32* vs) {
      if (ks == rec_free) std::swap(rec_keys, rec_free);
      if (vs == v_free) std::swap(vals, v_free);
      keys = ks;
      return *this;
    }
    static ListHome sorted(void* rec_a, void* rec_b, u32* v_a, u32* v_b, u32* slots, u32* slots_next, const void* ks, u32* vs) {
      return at(rec_a, rec_b, v_a, v_b, slots, slots_next).sorted_into(ks, vs);
    }
    // what a step left becomes what the next one reads: the list it sorted into (ks, vs), with the slots it wrote for it
    void advance(const void* ks, u32* vs) { sorted_into(ks, vs); std::swap(slots, slots_next); }
    // an 8 * cap-byte region of the three that is neither the keys' nor rec_free: with rec_free, two free ones
    void* spare_region(void* a, void* b, void* c) const { return (a != rec_keys && a != rec_free) ? a : (b != rec_keys && b != rec_free) ? b : c; }
  };
  // what a step reports.  text_chars is rewritten by a text round alone; carry: the next list's keys hold the characters in
  // bits 56..63; ran_run: the step made the run step's keys (run_mode 1 and the key had room)
  struct RankResult { u32 m, groups; bool finish; u32 text_chars; bool carry; bool ran_run; };
  template <typename K, bool INIT>
  int rank_step(struct SortList& L, const struct RankRequest& rq);
  int next_list(struct SortList& L, u64* ka, u64* kb, u32* va, u32* vb, u32 m_next, int bits, u32 holes, bool drop_holes, u64 key_bytes, bool timed);
  bool dense_route = true;   // BWTC_HIP_DENSE=0: always the list-order route (random rank[s+h] gather)
  bool digit_planes = true;  // BWTC_HIP_PLANES=0: every histogram pass reads the keys
  u32 pairs_min = 1u << 21;  // lists of at least this many entries take the window-ordered routes to rank[] (pairs partitioned before the
                             // scatter, dense records); a field so that the round hook can lower it for one call (RoundKnobScope): no environment variable
  int window_bits = 16;      // BWTC_HIP_WINDOW_BITS: rank[] is updated / read in windows of n >> window_bits suffixes
  bool split_index = true;   // BWTC_HIP_SPLIT_INDEX=0: the initial sort always carries 32-bit suffix numbers
  bool gram_keys = true;     // BWTC_HIP_GRAMS=0: initial keys are always base-sigma numbers (no dense gram codes)
  int gram_count_override = 0;
  struct GramPlan { int g = 0, G = 0, b = 0; u32 top = 0; };
  int plan_grams(const KeyPlan& plan, u32 n, const u8* d_lut, GramPlan* gp);
  // suffix_sort's stages (bwt_engine.hip): the initial sort and ranking by key plan, the rounds, the finisher route
  int initial_keys32(const InitialSort& in, SortList& L, u64 h);
  int initial_wide(const InitialSort& in, bool allow_code_keys, SortList& L, u64* h);
  int initial_keys64(const InitialSort& in, const GramPlan& gp, int key_bits, u32 short_len, int split, SortList& L, u64 h);
  int initial_long(const InitialSort& in, const GramPlan& gp, int key_bits, int split, bool coded, SortList& L, u64* h, bool* ranked);
  // the rounds over a sorted list of m entries from depth h0: text_rounds rounds that compare the text first; keep_first: the
  // list is sorted to h0 as it stands; doubling == false: text rounds only, and what they leave tied comes back in RoundsLeft
  struct RoundsRequest { u32 m; u64 h0; int text_rounds; bool keep_first, doubling; };
  struct RoundsLeft { u32 left = 0; u64 h_left = 0; };
  int run_rounds(SortList& L, const RoundsRequest& ask, RoundsLeft* out = nullptr);
  int step_due(const SortList& L, u32 m, u64 h_round, u64 h_first, bool text_round, bool* due);
  int finisher_route(SortList& L, u32 n_lf);
  int finisher_shape(u32 n, const RankResult& res);                                        // -> blk.fin.window / group; the passes at most
  int shallow_rounds(SortList& L, const FinOutcome& fo, u32* shallow_depth);
  int waiting_to_rounds(SortList& L, const FinOutcome& fo, u32 shallow_depth);
  hipError_t finisher_begin(u32* S, u32 m, FinWork* w);
  bool no_emit = false;      // BWTC_HIP_NO_EMIT: suffix array + gather even for blocks that could carry
  bool long_keys = true;     // BWTC_HIP_LONG=0: never the long-key initial sort
  int long_items_per_thread = 8;   // BWTC_HIP_LONG_E=6: tiles of 3072 items (three workgroups per CU instead of two)
  u32 gram_min_n = 1u << 22; // blocks below this keep the plain base-sigma key (BWTC_HIP_GRAM_MIN_N: tests)
  bool code_keys = true;     // BWTC_HIP_KEYS=grams: the long key is made of dense gram codes (round 4) instead of the order-1 prefix code
  int code_bits = 72;        // BWTC_HIP_CODE_BITS=N (40..72): bits of a code key (the low 32 in the second word)
  u32* d_pairs = nullptr;    // code keys: sampled character-pair counts (kPairReplicas x 65536 words), and the code table (257 x 256 words)
  u32* d_codes = nullptr;
  u32* d_parkS = nullptr;    // finisher route: the hard list (suffix; head slot << 32 | slot) while the shallow list takes its rounds
  u64* d_parkHP = nullptr;
  u32* d_hardS = nullptr;    // finisher route: the groups too large for a window (suffix; head slot << 32 | slot; character | depth << 8), until their code round
  u64* d_hardHP = nullptr;
  unsigned short* d_hardC = nullptr;
  u32 fin_floor = 12;        // BWTC_HIP_FIN_FLOOR: hard groups that share fewer characters take their rounds first, on their own
  bool finisher = true;      // BWTC_HIP_FINISHER=0: after the long-key sort straight into the doubling rounds
  int fin_window = 1024;     // BWTC_HIP_FIN_WINDOW=2048: entries a finisher workgroup sorts
  int fin_max_group = 256;   // BWTC_HIP_FIN_GROUP=256|512|1024: the largest group the finisher settles (larger ones take the text rounds)
  int fin_words = 2;         // BWTC_HIP_FIN_WORDS=2|3|4: 8-character words a finisher pass compares
  bool fin_shape_fixed = false;  // either of the two was given: every block takes that shape
  bool fin_wide_short = true;    // BWTC_HIP_FIN_WIDE=0: a short list (the long keys left at most n / 24 suffixes tied) keeps the default shape;
                                 // else it takes windows of 2048 entries and groups of up to 1024 members, and no hard list is left for the rounds
  bool long_direct = true;   // BWTC_HIP_LONG_DIRECT=0: every pass of the long-key sort takes its histogram from a digit plane (else: the second word's passes read the words)
  int fin_rounds = 3;        // BWTC_HIP_FIN_ROUNDS=1..4 (with two words): rounds of fin_words words a finisher pass makes (the members a round leaves tied are compared again inside the workgroup)
  int fin_max_passes = 8;    // BWTC_HIP_FIN_PASSES: finisher passes at most before what is still tied takes the doubling rounds
  int text_rounds = 6;       // BWTC_HIP_TEXT_ROUNDS: rounds that compare the text itself before rank[] is completed for doubling
  bool text_rounds_fixed = false;
  void complete_ranks(u32 n, const u32* list_sfx, const u32* list_slot, u32 m, void* pairs_region, void* tmp_region);
  // finisher passes over the list w (m entries, one region; b: spare list arrays): groups too large for a window go to
  // d_parkS / d_parkHP / d_hardC, shallow ones to rq.shal; what the last pass leaves tied becomes the local list
  // (local_handover) or is appended to d_parkS / d_parkHP (park_rest; `parked`)
  int finisher_passes(FinWork& w, const FinRequest& rq, FinOutcome* fo);
  int local_handover(const FinWork& w, FinOutcome* fo);
  int park_rest(const FinWork& w, const FinRequest& rq, FinOutcome* fo);
  // the local list (deep repeats in small groups, doubled group by group beside the global list: bwt_engine.hip, local_pass)
  bool local_rounds = true;  // BWTC_HIP_LOCAL_ROUNDS=0: what the finisher's passes leave joins the waiting list, as in round 4
  u32* d_LP0 = nullptr; u32* d_LH0 = nullptr; u32* d_LH1 = nullptr; unsigned short* d_LC1 = nullptr;
  u32* d_US = nullptr; u32* d_UR = nullptr;          // k_finish<RANK>'s notes: suffix (or none), its new rank, by list position
  struct FinList local_list(int home) const;
  int local_updates();
  int local_pass(u32 n, u64 h_global, struct RrEmit& re);
  // Test hook: one k_finish launch (chars or RANK) through the launch code of finisher_passes / local_pass, on d_T as
  // load_text left it.  -1: the list breaks a contract of k_finish (nothing is launched); -20 - i: a canary changed.
  int test_finish_pass(FinPassTest& t);
  int test_finisher(bwtc_hip_fin_run& t);   // the same for the driver, finisher_passes, over a one-region list
  // Test hooks (bwtc_hip_test_rank_* / _round_keys): one ranking through launch_rerank, the aggregates' scan
  // alone, a window scatter, a round's key kernel -- rank_step's launch code and shapes, on d_T as load_text left it.
  // -1: a contract of the kernels fails (nothing is launched); -20 - i: a canary changed.
  int test_rank_pass(bwtc_hip_rank_pass& t);
  int test_rank_scan(u32* a, u32* b, u32* c, u32 ntiles, u32* parts_out, u32 parts_cap, u32* counts_out);
  int test_rank_scatter(bool dense, const u32* where, const u32* what, const u64* rec, u32 m, u32 n, int bin_shift, u32* rank);
  int test_round_keys(bwtc_hip_round_keys& t);
  int test_round(bwtc_hip_round& t);        // the driver: rank_step<u64, false> once, pairs_min and window_bits set and restored
  // a raw list (suffix; head slot << 32 | slot) in (S, HP) -> a sorted list the rounds understand, in L.home / L.res
  int dress_list(SortList& L, u32 total, u32* S, u64* HP, u32 holes = 0);
  // runs and periods (bwt_engine.hip, "Runs" / "Periods"): long runs of one byte (period 1) and stretches of a period p > 1
  // are ranked in closed form by one round, the step.  A block's steps stand in BlockSort::steps in the order it takes them,
  // over the one length array d_runK: one step per block -- or, with BWTC_HIP_MIXED=1, the run step and then one period
  // step, whose lengths replace the runs' in d_runK; with BWTC_HIP_MULTI=1 up to three period steps, which merge their
  // look-up lengths there (tests/multimodel.py).  decide_step fills the schedule, step_due says which entry is a round's.
  bool run_ranks = true;     // BWTC_HIP_RUNS=0: no run step; the longest run is found only to tell a run from a voted period (decide_step)
  bool period_ranks = true;  // BWTC_HIP_PERIODS=0: no votes, no period-length pass, no period step
  u32 period_forced = 0;     // BWTC_HIP_PERIOD=p: that period, no votes (1: the run path)
  bool mixed_steps = false;  // BWTC_HIP_MIXED=1: a block may take the run step and a period step (decide_step)
  bool multi_steps = false;  // BWTC_HIP_MULTI=1: MIXED's rules, and up to three period steps per block over merged look-up words (decide_step)
  u32* d_runK = nullptr;     // k_p[s]: the leading characters of suffix s that are p-periodic (p = 1: the positions from s on that hold T[s])
  u32* d_runF = nullptr; u32* d_runB = nullptr;   // the stretch-length pass's words per tile
  u32* d_votes = nullptr;    // the finder's table: votes per distance 0 ... kPeriodMax
  // copies (bwt_engine.hip, "Copies"): whole copies at places that are no period look up past the copy in a doubling round
  bool copy_rounds = false;  // BWTC_HIP_COPIES=1
  // K[] into d_runK for the list (aidx, agrp: suffix and dense group number, m entries in list order, `groups` groups) over
  // the current rank[]: the marks, the flags, the lengths, one read-back -> the longest K.  bad[] lives in d_LP0, P[] in d_parkS
  int copy_lengths(const u32* aidx, const u32* agrp, u32 m, u32 groups, u32 n, u32* longest);
  int test_copy_lengths(const u32* suf, const u32* grp, u32 m, const u32* rank, u32 n, u32* k_out, u32* longest_out);
  // store == false: the longest stretch alone (a trial); proper: the longest proper stretch too (the general form for p = 1)
  struct StepMerge { u32 h; bool fresh; };   // a storing pass over the merged look-up words: the step's depth; the block's first step
  int stretch_lengths(u32 n, u32 p, bool store, u32* longest, u32* proper = nullptr, const StepMerge* merge = nullptr);
  int period_winners(u32 need, u32* out, u32* n_out);   // the finder's up to 8 candidates over d_votes (distance, votes)
  bool mixed_rule() const { return mixed_steps && run_ranks && period_forced != 1; }   // BWTC_HIP_MIXED's rule holds: a run is no stretch
  // decide_step goes on to look for a period (behind a run step that is due, under the rule only); bwtc_hip_schedule_get
  // reports gate lengths and votes for these blocks alone
  bool looks_for_period(bool run_due) const { return period_ranks && period_forced != 1 && (!run_due || mixed_rule()); }
  int find_period(u32 n, const u64* ks, const u32* vs, u32 m, u64 kmask, PeriodCandidates* out);
  int decide_step(u32 n, u32 m, u64 h_first, const u64* ks, const u32* vs, u64 kmask);   // -> blk.steps, blk.weighed
  // candidate p through the probe, the pass, the worth test and the division -> *out (p == 0: refused)
  int weigh_period(u32 n, u64 h_first, bool mixed, bool store, u32 p, u32 votes, WeighedPeriod* out);
  int store_step(u32 n, StretchStep& step, u64 h_round, bool behind_run);   // the storing pass of the step that is due
  // long periods (bwt_engine.hip, "Long periods"): the finder votes for distances up to kLongPeriodMax too, and a period
  // above kPeriodMax takes the wide probe; everything behind them is the code a short period goes through
  bool long_periods = false;   // BWTC_HIP_LONG_PERIODS=1 (BWTC_HIP_LONG_PERIOD=p names a period above kPeriodMax, as BWTC_HIP_PERIOD does below)
  u32* d_lvotes = nullptr;     // the long finder's words: the coarse table, the selected bins, the fine tables
  // Both sweeps and the merged candidates over a sorted list: up to kPeriodCandidates (distance, votes) pairs with `need`
  // votes or more, distances 2 ... kPeriodMax and kPeriodMax + 1 ... dmax, into out[16] and their number into *n_out
  // (one host wait, a second one behind sweep 2).  k1: the RUNS_OUT rule.  winner_only (the product without
  // BWTC_HIP_MULTI): the short table's winner whatever its votes, as k_period_winner leaves it, where no long distance
  // has `need` votes.  *swept: sweep 2 ran.
  int long_period_votes(const u64* ks, const u32* vs, u32 m, u64 kmask, const u32* k1, u32 need, u32 dmax, bool winner_only, u32* out,
                        u32* n_out, bool* swept);
  int long_period_probe(u32 n, u32 p, u32 span, bool* found);   // the wide probe over d_T (one host wait)
  int long_grams_override = 0;   // BWTC_HIP_LONG_G2=N: N grams in the second key word
  void scatter_rank_pairs(u32* pairs, u32* tmp, u32 m, u32 n);
  int load_text(const u8* d_src, u32 ncopy, u32 n, bool reverse, u32* hist_T);
  // Test hook (bwtc_hip_test_code_*): the code-key stage's kernels with suffix_sort's launch shapes and key layout, on
  // d_T as load_text left it and d_pairs / d_codes / d_R1 / d_W0 / d_P0.  parts: 1 the pair counts, 2 the table, 4 the
  // keys.  With part 1 the dense codes come from plan_keys(hist) and go out in lut / *sigma; without it they come in.
  int test_code_stage(u32 parts, u32 n, const u32* hist, bool lone_sentinel, int kbits, bool split, u8* lut, u32* sigma);
  // Device-resident block transform: d_src (size bytes) -> d_dst (size bytes).
  // raw=false: block semantics (reverse, sentinel, EOB patch).  raw=true: d_src already is
  // T (size = length), position pidx keeps its input byte.
  int transform(const u8* d_src, u8* d_dst, u32 size, bool raw, u32* lf, u32 n_lf, u32* freqs);
};

u64 huffman_compress_bound(u64 size);
// 'H' coder over an already transformed block that is resident on the device: writes the
// complete BWT-block record (48-bit length, BWTBlock header, sections, payloads) to d_out.
int huffman_encode_device(BwtEngine& e, const u8* d_bwt, u32 size, const u32* lf, u32 n_lf,
                          const u32* freqs, u8* d_out, u64 out_cap, u64* out_bytes);

// What the WaveletTree constructor first computes for every section of a transformed block
// (utils::calculateRunsAndCharacters, Utils.cpp:128-147; WaveletTree.hpp:294-308).
struct WaveletSectionStats {
  std::vector<u32> sections;                                  // section lengths
  std::vector<u32> run_freqs;                                 // [section][256] runs per symbol
  std::vector<u64> total_runs;                                // runs per section
  std::vector<std::vector<std::pair<u32, u32> > > dist;       // per section: (run length, count), ascending
  std::vector<u32> first_run;                                 // first run of every section, + total
};
// d_run_start / d_run_sym: where the runs go (null: the transform's workspace, e.d_R1 / e.d_R2)
// while_waiting: host work to do after the scanner's kernels and copies are queued, before the wait for them
int wavelet_section_stats_device(BwtEngine& e, const u8* d_bwt, u32 size, const u32* freqs,
                                 WaveletSectionStats* out, u32* d_run_start = nullptr, u8* d_run_sym = nullptr,
                                 const std::function<void()>* while_waiting = nullptr);

// Steps of all runs of the block sorted into coding order, skipped bits dropped, the packed
// streams copied into `codes` (wavelet_tree.hip); plan comes from bwtc::wavelet::planStreams.
int wavelet_streams_device(BwtEngine& e, const u32* d_run_start, const u8* d_run_sym, u32 n_runs, const std::vector<u32>& first_run,
                           const bwtc::wavelet::StreamPlan& plan, std::vector<u32>* coded_pos,
                           PinnedBytes* codes, bool async_copy = false, const u32** d_packed = nullptr);
// The adaptive models of a block whose packed streams are in HBM (wavelet_gpu_models.hip): queues
// the passes and the copy of the w-elements to h_w, of {state after, error flags, count} to h_tail.
int wavelet_models_device(BwtEngine& e, const u32* d_packed, u32 n_coded, const bwtc::wavelet::StreamPlan& plan,
                          const std::vector<u32>& coded_pos, u32 state_in, uint16_t* h_w, u32* h_tail, u32 kind = 0);
// the same in two parts: what does not depend on the carried state (read_ends: and, after a wait for the
// device, the state after the block for each of the eight states it can start in), and the rest
// (early_state != null: the state after the block is returned before the long passes are queued -- from
// that table, else read back with a short wait).  kind: the main model (gm::kKindB / kKindb / kKindu), kept in *g; a
// letter's passes do not look at state_in, their table is ends[i] = i with or without read_ends, and nothing waits
int wavelet_models_prepare(BwtEngine& e, const u32* d_packed, u32 n_coded, const bwtc::wavelet::StreamPlan& plan,
                           const std::vector<u32>& coded_pos, GmPass* g, bool read_ends = false, hipStream_t side = nullptr,
                           u32 kind = 0);
// the same from "tasks and chunks are known" on (gm::buildTasks / gm::cutChunks, wavelet_gpu_models.hpp)
int wavelet_models_prepare_tasks(BwtEngine& e, const u32* d_packed, u32 n_coded, const std::vector<bwtc::wavelet::gm::Task>& tasks,
                                 const std::vector<bwtc::wavelet::gm::Chunk>& chunks, GmPass* g, bool read_ends = false,
                                 hipStream_t side = nullptr, u32 kind = 0);
int wavelet_models_run(BwtEngine& e, const GmPass& g, u32 state_in, uint16_t* h_w, u32* h_tail, u32* early_state);

// WaveletEncoder: writeBlockHeader + encodeData + finishBlock (WaveletCoders.cpp:173-219,
// 112-157, 159-163) for a device-resident transformed block, in two halves so that blocks
// overlap (wavelet_pipeline.hpp): _begin does the device work (run scanner, stream kernels),
// advances the encoder's carried model state and queues the block's models and range coders
// on the engine's worker threads (created with `threads` threads by the first call); _end waits
// for that block and reports the record's size (the bytes are in `out` given to _begin).
int wavelet_encode_begin(BwtEngine& e, const u8* d_bwt, u32 size, const u32* lf, u32 n_lf,
                         const u32* freqs, unsigned threads, u8* out, u64 out_cap, u64* ticket);
int wavelet_encode_end(BwtEngine& e, u64 ticket, u64* out_bytes);
// _begin in two halves, for a stream whose blocks are spread over several contexts: _prepare is
// everything that does not depend on earlier blocks, _queue hands the block to the workers with
// the carried model state after the previous block and reports the state after this one.
int wavelet_encode_prepare(BwtEngine& e, const u8* d_bwt, u32 size, const u32* lf, u32 n_lf,
                           const u32* freqs, unsigned threads, u8* out, u64 out_cap, u64* ticket,
                           const std::function<void()>* while_scanning = nullptr);
int wavelet_encode_queue(BwtEngine& e, u64 ticket, u32 state_in, u32* state_out);
// Blocks begun with _begin join their stream one or two calls later; this makes every such block
// join NOW, in ticket order, with the stream's current state and model -- what must happen before
// the context starts another stream (bwtc_hip_wavelet_start / _reset).
int wavelet_join_begun(BwtEngine& e);
void wavelet_pipeline_release(BwtEngine& e);

// Inverse transform of a device-resident transformed block (d_bwt and d_out may alias).
// Returns -4 when an LF power does not lie on the LF walk (corrupt header or data).
int inverse_bwt_device(BwtEngine& e, const u8* d_bwt, u8* d_out, u32 size, const u32* lf, u32 n_lf);

}  // namespace bwtc_hip
