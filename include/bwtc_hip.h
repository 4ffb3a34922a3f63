/*
 * bwtc_hip.h -- C ABI of libbwtc_hip.so, the MI355X (gfx950) back-end for the
 * BWTManager -> BWTransform hot path of pjmikkol/bwtc and for the data-parallel half of
 * its 'H' entropy coder.  Plain pointers and sizes only; no exceptions cross this
 * boundary.  Citations are file:line relative to the reference tree.
 *
 * Return convention (mirrors divbwtf, bwtransforms/divsufsort.c:448,513-515):
 *   0 success, -1 bad arguments, -2 out of (device) memory, -3 HIP runtime error,
 *   -10 .. -15 a corrupt 'H' record (BWTC_HIP_E_*, below).
 *
 * A context owns one device, one stream and a persistent HBM workspace sized for
 * max_block_size, the way the reference back-ends own their per-call workspace
 * (bwtransforms/divsufsort.c:491-493) -- but allocated once, not per block.
 * A context is not thread-safe; use one per worker (= one per GPU in the block farm).
 */
#ifndef BWTC_HIP_H
#define BWTC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bwtc_hip_ctx bwtc_hip_ctx;

/* Statistics of the last transform on a context (all device work, HIP events on the
 * context's stream). */
typedef struct bwtc_hip_stats {
  uint32_t n;                 /* suffixes sorted = block size + 1                          */
  uint32_t rounds;            /* prefix-doubling rounds after the initial 4-byte sort      */
  uint64_t active_sum;        /* sum over rounds of suffixes still in non-singleton groups */
  uint64_t sort_pass_items;   /* sum over all radix passes of items moved                  */
  float    ms_total;          /* whole transform, device time                              */
  float    ms_sort;           /* radix sort passes only                                    */
  /* round 4: which way the block went, and the algorithmic bytes of the kernels that ran      */
  uint32_t route;             /* bit 0: long-key initial sort; bit 1: finisher settled the ties;
                                 bit 2: text rounds ran; bit 3: rank[] completed late for doubling rounds;
                                 bit 4: the long key is the order-1 prefix code (not dense gram codes);
                                 bit 5: a run step ran -- long runs of one byte were ranked in closed form
                                        (BWTC_HIP_RUNS=0: never);
                                 bit 6: the finisher's small groups doubled beside the rounds' list (local list);
                                 bit 7: a finisher list too long for its pass's shape went to the rounds;
                                 bit 8: a period step ran -- stretches of a period p > 1 were ranked in closed form
                                        (BWTC_HIP_PERIODS=0: never; together with bit 5 only under BWTC_HIP_MIXED=1: the block
                                        took the run step and a period step, or one period step that ranked its runs too) */
  uint32_t finisher_entries;  /* list entries over all finisher passes                      */
  uint64_t alg_bytes;         /* compulsory bytes of the transform's kernels: every array a kernel
                                 reads counted once, every array it writes counted once (SURVEY.md
                                 8(d)'s counting rule applied to the kernel list that actually ran) */
} bwtc_hip_stats;

/* Per-kernel device timing of the dominant kernel (the radix scatter pass), gathered with
 * HIP events on the context's stream while profiling is on.  bytes = ALGORITHMIC bytes:
 * items * (key + value) read once and written once. */
typedef struct bwtc_hip_kernel_timers {
  uint64_t scatter_launches;
  uint64_t scatter_bytes;
  double   scatter_ms;
} bwtc_hip_kernel_timers;

int  bwtc_hip_device_count(void);
const char* bwtc_hip_version(void);

/* Workspace bytes a context for blocks up to max_block_size bytes will allocate. */
uint64_t bwtc_hip_workspace_bytes(uint32_t max_block_size);

/* Create / destroy.  *ctx_out is NULL on failure. */
int  bwtc_hip_create(int device, uint32_t max_block_size, bwtc_hip_ctx** ctx_out);
void bwtc_hip_destroy(bwtc_hip_ctx* ctx);
void* bwtc_hip_stream(bwtc_hip_ctx* ctx);          /* hipStream_t of the context */
int  bwtc_hip_get_stats(bwtc_hip_ctx* ctx, bwtc_hip_stats* out);
int  bwtc_hip_set_profiling(bwtc_hip_ctx* ctx, int on);
int  bwtc_hip_get_kernel_timers(bwtc_hip_ctx* ctx, bwtc_hip_kernel_timers* out, int reset);
/* What this GPU streams: a copy of `bytes` bytes (16 bytes per lane, the library's own kernel) repeated `reps`
 * times on the context's stream, timed with HIP events; *gbps = bytes read + bytes written per second / 1e9.  The
 * denominator bench.py quotes beside the spec peak (not part of the reference's interface: measurement only). */
int  bwtc_hip_copy_probe(bwtc_hip_ctx* ctx, uint64_t bytes, int reps, double* gbps);

/* Device buffers for callers of the *_device entry points that do not link the HIP runtime
 * themselves (allocation on the context's GPU; copies are synchronous). */
void* bwtc_hip_malloc(bwtc_hip_ctx* ctx, uint64_t bytes);
void  bwtc_hip_free(bwtc_hip_ctx* ctx, void* d_ptr);
int   bwtc_hip_memcpy_to_device(bwtc_hip_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);
int   bwtc_hip_memcpy_to_host(bwtc_hip_ctx* ctx, void* dst, const void* d_src, uint64_t bytes);

/* Page-locked host memory and uploads that overlap the context's kernels: a farm worker keeps
 * two device buffers and copies block i+1 in (on the context's own copy stream) while block i
 * is transformed on the compute stream.  _async returns at once (src should come from
 * bwtc_hip_host_alloc; pageable memory still works but is staged by the runtime);
 * bwtc_hip_copy_wait blocks until every copy issued so far on this context has landed.
 * These replace nothing in the reference (its blocks never leave host memory); they are what
 * SURVEY.md 8(e) calls the pinned staging ring of a GPU worker. */
void* bwtc_hip_host_alloc(bwtc_hip_ctx* ctx, uint64_t bytes);
void  bwtc_hip_host_free(bwtc_hip_ctx* ctx, void* p);
int   bwtc_hip_memcpy_to_device_async(bwtc_hip_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);
int   bwtc_hip_copy_wait(bwtc_hip_ctx* ctx);

/* LF powers a block of `size` bytes gets for `starting_points`
 * (BWTManager::setStartingPoints clamp, bwtransforms/BWTManager.cpp:60-64, then
 * BWTBlock::prepareLFpowers, BWTBlock.cpp:104-108). */
uint32_t bwtc_hip_n_lf(uint32_t size, uint32_t starting_points);

/* Raw transform.  Replaces BWTransform::doTransform(byte* begin, uint32 length,
 * std::vector<uint32>& LF, uint32 freqs[256]) (bwtransforms/BWTransform.hpp:53-58) as
 * implemented by Divsufsorter (bwtransforms/Divsufsorter.hpp:60-65) and SAISBWTransform
 * (bwtransforms/SA-IS-bwt.cpp:48-54): T[0..length-1] (host memory, caller already planted
 * the 0 sentinel at T[length-1]) is transformed in place; every position except LF[0] is
 * written; lf[0..n_lf-1] receives the LF powers; freqs (may be NULL) is INCREMENTED. */
int bwtc_hip_bwt(bwtc_hip_ctx* ctx, uint8_t* T, uint32_t length, uint32_t* lf, uint32_t n_lf,
                 uint32_t* freqs);

/* Block-level transform.  Replaces BWTransform::doTransform(BWTBlock&, uint32 freqs[256])
 * (bwtransforms/BWTransform.cpp:52-64): block[0..size-1] (host) is reversed, terminated,
 * transformed and the end-of-block hole filled, all on the device; block[size] is never
 * touched (the reference borrows and restores it).  n_lf as from bwtc_hip_n_lf(). */
int bwtc_hip_bwt_block(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size, uint32_t* lf,
                       uint32_t n_lf, uint32_t* freqs);

/* Same, device-resident: d_in/d_out are device pointers to `size` bytes (may alias);
 * lf (n_lf words) and freqs (256 words, incremented; may be NULL) are HOST pointers.
 * Work is issued on the context's stream and has completed on return. */
int bwtc_hip_bwt_block_device(bwtc_hip_ctx* ctx, const uint8_t* d_in, uint8_t* d_out,
                              uint32_t size, uint32_t* lf, uint32_t n_lf, uint32_t* freqs);

/* ---- batched block transform (batch_bwt.hip; DESIGN.md section 3, "The batched sorter") -------
 * k blocks in one set of launches: the same bytes, LF powers and counts as k calls of
 * bwtc_hip_bwt_block, with one host wait per sorting round for the whole batch.
 * Block i is data[offset .. offset + size), transformed in place (the device form: from
 * d_in + offset to d_out + offset; d_in and d_out may be the same pointer).  Blocks may touch each
 * other; no byte outside a block's `size` bytes is written.  lf: k rows of 256 words, row i
 * holds block i's n_lf powers (the rest of the row is zeroed); freqs: k rows of 256, incremented;
 * may be NULL.  Returns -1 with nothing written when k == 0 or k > 4096, a size is 0, an n_lf is 0
 * or above 256, two blocks overlap, or k * S exceeds max_block_size + 1, where S is the smallest
 * power of two that is >= the largest size + 1; -2 / -3 as the other entry points do.
 * A context is driven by one thread, and no single-block transform is under way during the call. */
typedef struct { uint64_t offset; uint32_t size; uint32_t n_lf; } bwtc_hip_batch_item;
int bwtc_hip_bwt_blocks(bwtc_hip_ctx* ctx, uint8_t* data, const bwtc_hip_batch_item* items, uint32_t k,
                        uint32_t* lf, uint32_t* freqs);
int bwtc_hip_bwt_blocks_device(bwtc_hip_ctx* ctx, const uint8_t* d_in, uint8_t* d_out,
                               const bwtc_hip_batch_item* items, uint32_t k, uint32_t* lf, uint32_t* freqs);
/* What the last batched call on the context did.  active[0]: entries of tied groups after the initial sort,
 * active[r]: after round r (the first 32); host_waits: every point of the call at which the host waited for
 * the device; ms_total: device time between the call's first and last command (HIP events). */
typedef struct {
  uint32_t blocks, stride_log2, rounds, host_waits;
  uint64_t suffixes;
  uint64_t active[32];
  float ms_total;
} bwtc_hip_batch_stats;
int bwtc_hip_batch_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_batch_stats* out);
/* Test hook: the load pass and the initial keys alone.  data: host bytes, uploaded at their own offsets (the
 * largest offset + size must fit the context); T_out: the reversed, terminated blocks one after the other
 * (sum of size + 1 bytes); keys_out: one 63-bit key per suffix in the same order; freqs_out: k rows of 256. */
int bwtc_hip_test_batch_keys(bwtc_hip_ctx* ctx, const uint8_t* data, const bwtc_hip_batch_item* items, uint32_t k,
                             uint8_t* T_out, uint64_t* keys_out, uint32_t* freqs_out);

/* ---- inverse transform ---------------------------------------------------------------- */

/* Replaces InverseBWTransform::doTransform(BWTBlock&) (bwtransforms/InverseBWT.cpp:47-51) and
 * the MTL-SA walk behind it (bwtransforms/MtlSaInverseBWT.cpp:246-362): block[0..size-1]
 * (host) holds a transformed block as the forward path leaves it, lf[0..n_lf-1] its LF powers
 * (lf[0] = end-of-block row); on return block holds the original bytes.  The reference needs
 * block[size] as scratch (InverseBWT.cpp:49); this entry point does not touch it.
 * Returns -4 if an LF power is inconsistent with the data. */
int bwtc_hip_inverse_bwt_block(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size,
                               const uint32_t* lf, uint32_t n_lf);

/* Same with device pointers (may alias); lf is a HOST array. */
int bwtc_hip_inverse_bwt_block_device(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint8_t* d_out,
                                      uint32_t size, const uint32_t* lf, uint32_t n_lf);

/* ---- 'H' entropy coder (HuffmanCoders.cpp) ------------------------------------------- */

/* Upper bound of the bytes one encoded BWT block of `size` input bytes can take. */
uint64_t bwtc_hip_compress_bound(uint32_t size);

/* Encodes an already transformed block.  Replaces the part of
 * HuffmanEncoder::transformAndEncode (HuffmanCoders.cpp:51-61) after the transform:
 * writeBlockHeader (:271-313), encodeData (:119-257) and finishBlock (:259-261).  Output =
 * the complete BWT-block record: 48-bit big-endian length of the rest, BWTBlock header
 * (BWTBlock.cpp:61-86), section count and packed section lengths, then per section packed
 * run count, serialised code shape, Huffman-coded run symbols and gamma-coded run lengths.
 * d_bwt/d_out are device pointers (d_out 4-byte aligned, out_cap bytes); lf/freqs are the
 * HOST arrays the transform returned (freqs is not modified).  *out_bytes = record size. */
int bwtc_hip_huffman_encode_device(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                   const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                   uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes);

/* Same with host buffers (staged through the context's workspace). */
int bwtc_hip_huffman_encode(bwtc_hip_ctx* ctx, const uint8_t* bwt, uint32_t size,
                            const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_bytes);

/* HuffmanEncoder::transformAndEncode(block, bwtm, out) (HuffmanCoders.cpp:51-61) in one
 * call: block (host, `size` bytes, left transformed like the reference leaves it) ->
 * encoded BWT-block record in `out` (host).  starting_points as given to
 * BWTManager::setStartingPoints. */
int bwtc_hip_transform_and_encode(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size,
                                  uint32_t starting_points, uint8_t* out, uint64_t out_cap,
                                  uint64_t* out_bytes);

/* ---- 'H' decoding on the device ------------------------------------------------------ */

/* Return codes of a corrupt 'H' record (the decoders below never write past their output and
 * never loop without bound on any input): */
#define BWTC_HIP_E_NO_CODE     (-10)  /* a bit pattern that is no code, or an over-full code shape */
#define BWTC_HIP_E_SHAPE       (-11)  /* code lengths above maxLen, maxLen above 64, a bad alphabet   */
#define BWTC_HIP_E_PAST_RECORD (-12)  /* a header, shape or stream runs past the record              */
#define BWTC_HIP_E_RUNS        (-13)  /* run lengths that do not add up to their section's length    */
#define BWTC_HIP_E_CAPACITY    (-14)  /* a block larger than the output's capacity                  */
#define BWTC_HIP_E_LENGTH      (-15)  /* the 48-bit length field disagrees with what was consumed   */

/* Entropy decode of one BWT-block record.  Replaces HuffmanDecoder::decodeBlock
 * (HuffmanCoders.cpp:324-616): rec (host, rec_bytes bytes; it may go on past the record: only
 * the 6 + <48-bit length> bytes the record announces are read and uploaded) -> the transformed
 * block in bwt_out (host, cap bytes), its LF powers in lf_out[256] and their number in *n_lf,
 * *size = block size, *consumed = the record's bytes.  The block may be larger than the
 * context's max_block_size (up to cap, below 2^32).  The Huffman and gamma streams are decoded by
 * transition maps over tiles on the GPU; the device workspace is the decoder's own, allocated by
 * the first call and grown on demand (bwtc_hip_huffman_decode_stats: workspace_bytes). */
int bwtc_hip_huffman_decode(bwtc_hip_ctx* ctx, const uint8_t* rec, uint64_t rec_bytes, uint8_t* bwt_out,
                            uint64_t cap, uint32_t* lf_out, uint32_t* n_lf, uint32_t* size, uint64_t* consumed);
/* Same with the record (d_rec) and the transformed block (d_bwt_out) in device memory; lf_out
 * and the counts are host pointers.  The record is also read on the host (shapes, header). */
int bwtc_hip_huffman_decode_device(bwtc_hip_ctx* ctx, const uint8_t* d_rec, uint64_t rec_bytes, uint8_t* d_bwt_out,
                                   uint64_t cap, uint32_t* lf_out, uint32_t* n_lf, uint32_t* size, uint64_t* consumed);
/* Entropy decode plus InverseBWTransform::doTransform (InverseBWT.cpp:47-51): record (host) ->
 * the original block in out (host, cap bytes).  The record goes up once and the block comes
 * down once.  The inverse runs in the context's workspace, so cap is clipped to the context's
 * max_block_size: a larger block returns BWTC_HIP_E_CAPACITY. */
int bwtc_hip_decode_block_H(bwtc_hip_ctx* ctx, const uint8_t* rec, uint64_t rec_bytes, uint8_t* out, uint64_t cap,
                            uint32_t* size, uint64_t* consumed);
/* What the last decode on this context did: route 1 = the device decoder made the bytes. */
typedef struct bwtc_hip_huffman_decode_stats {
  uint32_t route;             /* 1: decoded on the device                                        */
  uint32_t sections;          /* non-empty sections                                              */
  uint32_t streams;           /* Huffman + gamma streams                                         */
  uint32_t host_syncs;        /* host round trips of the section chain (one per section + retries) */
  uint32_t retries;           /* Huffman streams that outran their estimated window (mapped again) */
  uint32_t max_code_len;      /* longest Huffman code length (maxLen) over the sections          */
  uint64_t runs;              /* runs decoded                                                    */
  uint64_t tiles;             /* tiles mapped (512 bits each)                                    */
  uint64_t map_entries;       /* entries mapped, tiles x M: each entry decodes its tile to the end
                                 (no boundary merging), so map_entries / tiles = M full-tile decodes */
  uint64_t launches;          /* kernels launched                                                */
  uint64_t workspace_bytes;   /* device workspace the decoder holds                              */
  float    ms_entropy;        /* device time of the decode's kernels: every section's kernel span
                                 plus the scan and expansion (event pairs on the stream)          */
  float    ms_entropy_wall;   /* record upload to BWT bytes, the section chain's host round trips
                                 and shape parsing included                                       */
  float    ms_chain_host;     /* ms_entropy_wall - ms_entropy: what the host-driven chain adds    */
  float    ms_inverse;        /* device time of the inverse transform (decode_block_H)           */
} bwtc_hip_huffman_decode_stats;
int bwtc_hip_huffman_decode_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_huffman_decode_stats* out);

/* ---- wavelet coders: run scanner (front-end statistics only) ---------------------------- */

/* utils::calculateRunsAndCharacters (Utils.cpp:128-147) for every section of a transformed
 * block, as the WaveletTree constructor needs it (WaveletTree.hpp:294-308): bwt = host buffer
 * of `size` bytes, freqs = the histogram the transform returned.  Outputs (host):
 *   *n_sections, section_len[256], run_freqs[256*256] ([section][symbol]), total_runs[256],
 *   dist_offset[257] and the (dist_len[i], dist_cnt[i]) pairs of section s in
 *   [dist_offset[s], dist_offset[s+1]), ascending by length (the reference's std::map order).
 * Returns -1 if dist_cap pairs do not suffice. */
int bwtc_hip_wavelet_section_stats(bwtc_hip_ctx* ctx, const uint8_t* bwt, uint32_t size,
                                   const uint32_t* freqs, uint32_t* n_sections,
                                   uint32_t* section_len, uint32_t* run_freqs,
                                   uint64_t* total_runs, uint32_t* dist_offset,
                                   uint32_t* dist_len, uint32_t* dist_cnt, uint32_t dist_cap);

/* WaveletEncoder::transformAndEncode (WaveletCoders.cpp:77-87) for coder 'B' (FSM8 model):
 * block (host, left transformed) -> encoded BWT-block record in `out` (host).  The transform
 * and the run scanner run on the GPU; tree building and the range coder are bit-serial and
 * run on `threads` host threads, one section at a time per thread (0 = all cores).  The
 * coder's model state is carried from call to call like the reference's encoder object
 * carries it from block to block; bwtc_hip_wavelet_reset starts a new stream. */
int bwtc_hip_transform_and_encode_wavelet(bwtc_hip_ctx* ctx, uint8_t* block, uint32_t size,
                                          uint32_t starting_points, uint32_t threads,
                                          uint8_t* out, uint64_t out_cap, uint64_t* out_bytes);
/* Same for an already transformed block (host). */
int bwtc_hip_wavelet_encode(bwtc_hip_ctx* ctx, const uint8_t* bwt, uint32_t size,
                            const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                            uint32_t threads, uint8_t* out, uint64_t out_cap, uint64_t* out_bytes);
/* Same for a transformed block that is resident on the device (the record still goes to host
 * memory: the coder runs there). */
int bwtc_hip_wavelet_encode_device(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                   const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                   uint32_t threads, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_bytes);
/* The same in two halves, so that a caller with several blocks overlaps them (the
 * reference's Compressor::compress loop, Compressor.cpp:103-137, made a pipeline): _begin does
 * the device work of the block (run scanner, tree bit vectors, traversal order, gap flags),
 * advances the encoder's carried model state and queues the block's adaptive models and range
 * coders on the context's worker threads (created by the first call, `threads` of them, 0 =
 * the CPUs the process may use -- affinity and cgroup quota -- up to 64); it returns as soon as the GPU is free for the next block.  _end waits
 * for that block; the record is then in the `out` given to _begin, *out_bytes long.  Records
 * are those of a strictly sequential encoder whatever the overlap.  At most
 * bwtc_hip_wavelet_depth(ctx) blocks (BWTC_HIP_WAVELET_DEPTH, default 16) are under way; a
 * further _begin returns -6 at once: collect the oldest with _end first.  `out` must stay valid
 * until _end (or until bwtc_hip_destroy returns: it lets blocks under way finish);
 * _begin/_end of one context are called from one thread. */
int bwtc_hip_wavelet_encode_device_begin(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                         const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                         uint32_t threads, uint8_t* out, uint64_t out_cap,
                                         uint64_t* ticket);
int bwtc_hip_wavelet_encode_end(bwtc_hip_ctx* ctx, uint64_t ticket, uint64_t* out_bytes);
/* _begin in two halves, for ONE stream whose blocks are farmed over several contexts (one per
 * GPU): _prepare does everything that does not depend on earlier blocks -- the
 * whole device half -- and may run on all contexts at once; _queue gives the block its place in
 * the stream: state_in is the main model's carried state after the previous block (4 for the
 * first block of a stream; the reference's WaveletEncoder carries it inside its m_probModel,
 * probmodels/FSM.hpp:196-205), *state_out the state after this block, to be passed to the _queue
 * of the next block on whichever context holds it.  _queue calls of a stream are made in block
 * order; each returns at once.  _begin = _prepare + _queue with the context's own state.
 * With the adaptive models on the device (the default for 'B') _prepare returns when its device
 * half is done -- it leaves the state after the block for each of the eight states the block can
 * start in, so that _queue has nothing to wait for -- and _queue launches the passes that depend
 * on the state; the block joins the context's worker threads when its elements have reached the
 * host.  A block prepared while another prepared block of the same context has not been queued
 * yet takes that one's place in the device workspace: the earlier block's models then run on the
 * worker threads (same bytes). */
int bwtc_hip_wavelet_encode_device_prepare(bwtc_hip_ctx* ctx, const uint8_t* d_bwt, uint32_t size,
                                           const uint32_t* lf, uint32_t n_lf, const uint32_t* freqs,
                                           uint32_t threads, uint8_t* out, uint64_t out_cap,
                                           uint64_t* ticket);
int bwtc_hip_wavelet_encode_queue(bwtc_hip_ctx* ctx, uint64_t ticket, uint32_t state_in,
                                  uint32_t* state_out);
/* Blocks that may be between _begin and _end at once on this context. */
uint32_t bwtc_hip_wavelet_depth(bwtc_hip_ctx* ctx);
/* Lowers (or raises) the number of blocks that may be under way, and gives the page-locked staging buffers the
 * stream no longer needs back to the system: a stream's first blocks run at the default depth, the depth it has
 * shown to need (bwtc_hip_wavelet_depth_needed) is usually half of it, and eight ranks of a node each hold what
 * they keep.  -6: more blocks are under way than `depth` allows (collect some first). */
int bwtc_hip_wavelet_set_depth(bwtc_hip_ctx* ctx, uint32_t depth);
/* Blocks the caller has to keep between _begin and _end for the rate the stream has shown so far: the mean time
 * from a block's _begin to its finished record over the mean time between two _begins, a quarter more, plus two.
 * 0 until four blocks have finished.  A caller that keeps fewer in flight waits in _end; more only hold memory
 * (1.3 GB of page-locked staging per 256 MiB text block under way). */
uint32_t bwtc_hip_wavelet_depth_needed(bwtc_hip_ctx* ctx);
/* Host CPUs for the worker threads of the contexts of one node (one context per GPU):
 * the 'B' coder's host half is memory- and cache-hungry, so a context's workers -- and the
 * page-locked buffers they read, placed by first touch / the caller's policy -- belong on the NUMA
 * node of its GPU, and contexts must not share cores.
 *   _numa_node        NUMA node of the context's GPU (PCI bus id -> /sys/bus/pci/devices/<id>/numa_node),
 *                     -1 when the system does not say;
 *   _host_cpu_slice   host-only: the CPUs this process may use (its affinity mask), cut down to those
 *                     of `numa_node` when that is >= 0 and the node has any, split into `ranks`
 *                     contiguous slices; slice `rank` goes to cpus[0..], the return value is its size
 *                     (0: nothing to hand out, negative: bad arguments).  Callers give rank / ranks
 *                     among the contexts that share the node;
 *   _set_worker_cpus  the context's worker threads (existing ones and those made later) may run on
 *                     exactly these CPUs; n = 0 lifts the restriction.  The calling thread is left alone. */
int bwtc_hip_numa_node(bwtc_hip_ctx* ctx);
int bwtc_hip_host_cpu_slice(int numa_node, uint32_t rank, uint32_t ranks, uint32_t* cpus, uint32_t cap);
int bwtc_hip_set_worker_cpus(bwtc_hip_ctx* ctx, const uint32_t* cpus, uint32_t n);
/* Host time the context's worker threads have spent so far in the two host stages of the wavelet
 * coder (adaptive models, range coders; seconds summed over threads) and the blocks queued. */
int bwtc_hip_wavelet_host_clock(bwtc_hip_ctx* ctx, double* model_seconds, double* coder_seconds,
                                uint64_t* blocks);
/* Blocks that have joined the host half so far (*queued) and blocks whose record the worker
 * threads have finished (*finished): what a caller needs to tell the rate the host half sustains
 * from the rate at which blocks are begun. */
int bwtc_hip_wavelet_host_progress(bwtc_hip_ctx* ctx, uint64_t* queued, uint64_t* finished);
/* Mean time a block has been under way so far: from the start of its device half (_begin / _prepare)
 * to its finished record.  Blocks under way needed = that time / the time per block of the caller's
 * loop; a context keeps the limit it was created with (BWTC_HIP_WAVELET_DEPTH). */
int bwtc_hip_wavelet_latency(bwtc_hip_ctx* ctx, double* mean_seconds);
/* The routes the context's wavelet blocks took (every route writes the same bytes; these say which
 * one did), one count per block:
 *   trees_device / trees_host   trees built by the stream kernels / by the host's own tree builder
 *                               (blocks planStreams declines, BWTC_HIP_WAVELET=host);
 *   models_device               models computed by the device passes and used;
 *   models_rejected             device passes whose result was not used, reject_reasons the OR of
 *                               the BWTC_HIP_REJECT_* bits seen;
 *   lost_turn                   prepared blocks (_prepare / _queue) whose device passes lost their
 *                               turn in the workspace to a later block;
 *   models_host_*               blocks of a device-built tree modelled on the worker threads: two-stage
 *                               (models, then range coders), fused engines, 16-lane model engines.
 * reset != 0: the counters start again from zero after they are read. */
#define BWTC_HIP_REJECT_FLAGS 1u     /* the passes flagged the block */
#define BWTC_HIP_REJECT_COUNT 2u     /* elements counted != elements coded */
#define BWTC_HIP_REJECT_SCAN  4u     /* a chained scan timed out */
#define BWTC_HIP_REJECT_STATE 8u     /* the state in or after the block is not the stream's */
#define BWTC_HIP_REJECT_TEST  16u    /* BWTC_HIP_TEST_MODELS_FALLBACK */
typedef struct bwtc_hip_wavelet_route_counts {
  uint64_t trees_device, trees_host;
  uint64_t models_device, models_rejected, reject_reasons, lost_turn;
  uint64_t models_host_two_stage, models_host_fused, models_host_lanes;
} bwtc_hip_wavelet_route_counts;
int bwtc_hip_wavelet_routes(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_route_counts* out, int reset);
/* Host staging memory (page-locked where the system allows) held by this process for blocks under
 * way -- packed streams and w-elements of every context -- now and at its highest so far: what a
 * deployment has to provide per rank for the depth it runs (no reference counterpart; the reference
 * holds one block, Compressor.cpp:100-108). */
int bwtc_hip_host_staging_bytes(uint64_t* now, uint64_t* peak);
/* CPUs this process may keep busy: the hardware threads, cut down to the cgroup's CPU quota -- what
 * `threads` = 0 means in the calls above.  A caller that runs several contexts splits this number
 * between them (the reference is single-threaded, Compressor.cpp:67-70). */
uint32_t bwtc_hip_host_usable_cpus(void);
void bwtc_hip_wavelet_reset(bwtc_hip_ctx* ctx);
/* A new wavelet stream with the main probability model of coder letter `coder`
 * (WaveletEncoder(char), WaveletCoders.hpp:52; giveProbabilityModel,
 * probmodels/ProbabilityModel.cpp:47-76): 'B' FSM8 (what bwtc_hip_wavelet_reset selects),
 * 'b' FSM<6, EvenIntervalPredictor<4>>, 'u' EvenIntervalPredictor<4>.  -1 for other letters:
 * 'm' / 'M' (SimpleMarkov) index one entry past their history table in the reference
 * (:91-93 vs :110-118), their output is undefined and they are not offered. */
int bwtc_hip_wavelet_start(bwtc_hip_ctx* ctx, char coder);

/* Host half of the 'B' coder alone (no device work): the sections' runs as the GPU scanner
 * delivers them -> the concatenated section payloads (packed bitsInRoot, tree shape, range-coded
 * bytes per section).  first_run[n_sections+1] delimits every section's runs inside
 * run_sym[] / run_start[] (run_start has one extra entry: the end of the last run);
 * run_freqs[n_sections*256]; the run-length distribution of section s is the pairs
 * [dist_offset[s], dist_offset[s+1]).  *state is the model state carried in and out. */
int bwtc_hip_host_wavelet_sections(uint32_t n_sections, const uint32_t* first_run,
                                   const uint8_t* run_sym, const uint32_t* run_start,
                                   const uint32_t* run_freqs, const uint32_t* dist_offset,
                                   const uint32_t* dist_len, const uint32_t* dist_cnt,
                                   uint32_t threads, char coder, uint32_t* state, uint8_t* out,
                                   uint64_t out_cap, uint64_t* out_bytes);

/* Same arguments and same bytes as bwtc_hip_host_wavelet_sections, computed the way the device
 * path does it: the tree shapes are planned from the statistics alone, every run is expanded
 * into (tree node, bit) steps that are sorted into coding order, and the coder only sees the
 * finished streams.  The expansion is done with plain host loops here (no device work), so
 * the planning and stream-coding halves can be checked without a GPU.  -5: a shape the
 * stream path does not take (the library then uses the tree builder of ..._sections). */
int bwtc_hip_host_wavelet_streams(uint32_t n_sections, const uint32_t* first_run,
                                  const uint8_t* run_sym, const uint32_t* run_start,
                                  const uint32_t* run_freqs, const uint32_t* dist_offset,
                                  const uint32_t* dist_len, const uint32_t* dist_cnt,
                                  uint32_t threads, char coder, uint32_t* state, uint8_t* out,
                                  uint64_t out_cap, uint64_t* out_bytes);
/* The same, with the adaptive models run the way the GPU runs them (wavelet_gpu_models.hpp: state
 * scan, slot space, bracketed chains, w-elements) -- lane by lane on the host, for tests without a
 * GPU.  Coder 'B' only.  -7: the passes raised their error flag. */
int bwtc_hip_host_wavelet_streams_lanes(uint32_t n_sections, const uint32_t* first_run,
                                  const uint8_t* run_sym, const uint32_t* run_start,
                                  const uint32_t* run_freqs, const uint32_t* dist_offset,
                                  const uint32_t* dist_len, const uint32_t* dist_cnt,
                                  uint32_t threads, char coder, uint32_t* state, uint8_t* out,
                                  uint64_t out_cap, uint64_t* out_bytes);

/* Host-only pieces of the 'H' coder (no device work; usable without a GPU).  They are the
 * small-table steps the encoder runs between its device passes, exported so the host logic
 * can be checked on its own:
 *   lengths : utils::calculateHuffmanLengths (Utils.cpp:408-473), freqs[256] -> clen[256]
 *   codes   : utils::computeHuffmanCodes (Utils.cpp:180-202)
 *   shape   : HuffmanEncoder::serializeShape, byte padded (HuffmanCoders.cpp:63-86,181-192);
 *             returns bytes written (<= cap) or 0
 *   sections: section heuristic of writeBlockHeader (HuffmanCoders.cpp:282-296); returns count
 *   header  : BWTBlock::writeHeader (BWTBlock.cpp:61-86); returns bytes written */
void     bwtc_hip_host_huffman_lengths(const uint64_t* freqs, uint8_t* clen);
void     bwtc_hip_host_huffman_codes(const uint8_t* clen, uint32_t* code);
uint32_t bwtc_hip_host_serialize_shape(const uint8_t* clen, uint8_t* out, uint32_t cap);
uint32_t bwtc_hip_host_sections(const uint32_t* freqs, uint32_t* section_len);
uint32_t bwtc_hip_host_bwtblock_header(const uint32_t* lf, uint32_t n_lf, uint8_t* out, uint32_t cap);

/* Synthetic inputs of the BASELINE.json configurations (no device
 * work): kind 'r' random bytes (C1), 'd' uniform ACGT (C2), 't' token text (C3/C4/C5), generated
 * from splitmix64(seed) -- the same bytes as bwtc_amd/synth.py.  -1 for another kind. */
int bwtc_hip_synth(char kind, uint64_t seed, uint64_t size, uint8_t* out);

/* Suffix array of T[0..length-1] under "proper prefix sorts first"
 * (test/SaisTest.cpp:45-53); sa is a host buffer of `length` words.  Test hook for the
 * property the reference checks in test/SaisTest.cpp:55-70. */
int bwtc_hip_suffix_array(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t length, uint32_t* sa);

/* Unit-test hooks for the sort/scan primitives (host buffers, in place). */
int bwtc_hip_test_sort_u32(bwtc_hip_ctx* ctx, uint32_t* keys, uint32_t* vals, uint64_t n, int nbits);
int bwtc_hip_test_sort_u64(bwtc_hip_ctx* ctx, uint64_t* keys, uint32_t* vals, uint64_t n, int nbits);
int bwtc_hip_test_scan_u32(bwtc_hip_ctx* ctx, uint32_t* data, uint64_t n);
/* Unit-test hooks for the radix sorts themselves (radix_sort.hpp: radix_sort_pairs, radix_sort_long,
 * radix_sort_keys_segmented), called directly on the context's buffers with three-launch scans; host buffers, in place.
 * Each checks the sort's contract on the host before it launches anything (-1 otherwise), makes the producer's first
 * digit plane itself from the keys, and guards both buffers of every ping-pong pair with 256 canary bytes behind the
 * last item: -20 - i when canary i changed (in the order keys, values, second words, planes; two each).
 *   _pairs: keys = n + n_holes items of key_bytes (4 | 8) in, n out; n_holes > 0: exactly that many keys are all ones
 *     and do not exist (given values only).  Sorted bits [bit_lo, nbits), 0 <= bit_lo <= nbits <= 8 * key_bytes.
 *     vals of val_bytes (4 | 2).  values_mode 0: given (n + n_holes in, n out), 1: item i's value is i, 3: n - 1 - i
 *     (n out; n >= 2 and nbits > bit_lo, the first pass makes them), 2: keys only (vals unused).
 *     planes 0: none, 1: digit planes, 2: digit planes and the first pass's digits ready in the first.
 *   _long: items (keys[i], w[i]) ordered by (keys bits [0, kbits), w bits [0, wbits)), 1 <= kbits <= 64,
 *     1 <= wbits <= 32, w without bits at or above wbits, n >= 2; vals (n out) are n - 1 - i of the item's first place.
 *     (val_bytes, items_per_thread) is (4, 6), (2, 6) or (2, 8); direct_w as radix_sort_long's.
 *   _segmented: n = whole tiles of 8192 keys; segment s is tiles [tile_first[s], tile_first[s + 1]), tile_first[0] = 0,
 *     non-decreasing, tile_first[nseg] = n / 8192; every segment sorted on its own by bits [bit_lo, bit_lo + 16). */
int bwtc_hip_test_radix_pairs(bwtc_hip_ctx* ctx, void* keys, void* vals, uint64_t n, uint64_t n_holes, int key_bytes, int val_bytes,
                              int bit_lo, int nbits, int values_mode, int planes);
int bwtc_hip_test_radix_long(bwtc_hip_ctx* ctx, uint64_t* keys, void* vals, uint32_t* w, uint64_t n, int val_bytes, int items_per_thread,
                             int kbits, int wbits, int direct_w);
int bwtc_hip_test_radix_segmented(bwtc_hip_ctx* ctx, uint32_t* keys, uint64_t n, int bit_lo, const uint32_t* tile_first, uint32_t nseg);
/* The period step of the context's last block: *p its period (the finder's winner above the
 * threshold, or BWTC_HIP_PERIOD's), *longest the block's longest p-periodic stretch, *votes the winner's votes,
 * *step_depth the depth of the period step that ran.  Zeros where nothing was looked for or found. */
int bwtc_hip_period_get(bwtc_hip_ctx* ctx, uint32_t* p, uint32_t* longest, uint32_t* votes, uint32_t* step_depth);
/* The closed-form steps of the context's last block (BWTC_HIP_MIXED=1 lets a block take the run step and a period step):
 * *run_depth and *period_depth the depths at which the run step and the period step ran, 0 for a step that did not run (one
 * period step over k_p[] that ranked the block's long runs too reports its depth as both); *period_p that step's period;
 * *longest_run the block's longest run of one byte; *longest_proper its longest proper stretch -- the largest k_p[s] over
 * the s with s + 1 < n and T[s] != T[s + 1] -- and 0 where no pass made it (only passes under the switch do). */
int bwtc_hip_steps_get(bwtc_hip_ctx* ctx, uint32_t* run_depth, uint32_t* period_p, uint32_t* period_depth, uint32_t* longest_run,
                       uint32_t* longest_proper);
/* The schedule of closed-form steps of the context's last block, in the order it took them (BWTC_HIP_MULTI=1 lets a
 * block take the run step and up to three period steps): 5 words per entry -- the period (1: the run step), the depth
 * the step ran at (0: it did not), its gate length (the longest run; a period's longest proper stretch), the finder's
 * votes for it, flags (1: a period step that ranked the block's long runs too; 2: the entry was dropped, its gate shut
 * when its depth came or the rounds over before).  Gate lengths and votes are 0 without the switch.  *n_out the entries
 * the block has, of which the first min(cap, *n_out) are written.  bwtc_hip_period_get and bwtc_hip_steps_get report the
 * first period step that ran. */
int bwtc_hip_schedule_get(bwtc_hip_ctx* ctx, uint32_t* entries, uint32_t cap, uint32_t* n_out);
/* The copy rounds of the context's last block.  With BWTC_HIP_COPIES=1 a doubling round over a
 * list of at least n / 32 entries, in a block without a closed-form step, makes K[s] -- the positions from s on whose
 * tied groups' successors all lie in one group -- and looks up rank[s + K[s] + h] in place of rank[s + h]: whole copies
 * of a piece at places that are no period are passed in one round.  *rounds the rounds that looked up that way, *passes
 * the passes that made K[] (one more: the pass whose longest K lay below its round's depth and shut the gate), *longest
 * the longest K of any pass, *first_depth the depth h of the first copy round.  Zeros without the switch or where no
 * round took a pass; route bit 10 (1024) of bwtc_hip_stats says that at least one copy round ran. */
int bwtc_hip_copies_get(bwtc_hip_ctx* ctx, uint32_t* rounds, uint32_t* passes, uint32_t* longest, uint32_t* first_depth);
/* Test hook: the copy round's three passes (marks, flags, lengths) with the sorter's launch code over a given list -- suf[i]
 * the suffix and grp[i] the dense group number (0, then equal to or one above the entry before) of entry i < m, in list
 * order -- and rank[0..n): k_out[s] = K[s] for every s < n, *longest_out their maximum.  No text is read.  -1, before
 * anything is launched, for m = 0, n = 0, m > n, n above the context's block size, an entry at or above n or group
 * numbers that are not dense; -20 - i: canary i behind an output changed. */
int bwtc_hip_test_copy_lengths(bwtc_hip_ctx* ctx, const uint32_t* suf, const uint32_t* grp, uint32_t m, const uint32_t* rank, uint32_t n,
                               uint32_t* k_out, uint32_t* longest_out);
/* Test hook: the sorter's own period-length pass (three launches; p = 1: the run-length pass) over T[0..n), on the
 * context's buffers: k_out[s] = the number of leading characters of suffix s that are p-periodic, *longest_out their
 * maximum.  -1, before anything is launched, for p = 0, p > 4096, n = 0 or n above the context's block size. */
int bwtc_hip_test_period_lengths(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest_out);
/* Test hook: the same pass with its second maximum, as the sorter launches it under BWTC_HIP_MIXED=1 (p = 1 in the general
 * form): *proper_out = the longest proper stretch, 0 where no s has T[s] != T[s + 1].  The same refusals. */
int bwtc_hip_test_period_proper(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest_out,
                                uint32_t* proper_out);
/* Test hook: the merging storing pass that a block's second and later closed-form steps take under BWTC_HIP_MULTI, and,
 * with fresh != 0, its first one (tests/multimodel.py, merge_words).  A word of k_inout[0..n) is a look-up length in bits
 * 0 ... 30 (0: no step has taken the suffix) and, in bit 31, "member of the current step".  The step of period p at depth
 * h takes suffix s when k_p[s] >= h and k_p[s] >= the old length (0 everywhere when fresh: k_inout is not read then); it
 * stores k_p[s] | 1 << 31 there, and the old length with bit 31 clear elsewhere.  *longest_out and *proper_out are the
 * two maxima over k_p[], as bwtc_hip_test_period_proper gives them.  The same refusals, and -1 for h = 0. */
int bwtc_hip_test_period_merge(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t h, int fresh, uint32_t* k_inout,
                               uint32_t* longest_out, uint32_t* proper_out);
/* Test hook: the finder's candidates under BWTC_HIP_MULTI (k_period_winners, one workgroup) over table[0..4096], the
 * votes per distance: out[2 i], out[2 i + 1] = the distance in 2 ... 4096 with the i-th most votes among those with `need`
 * votes or more (and at least one), the smaller distance first among equals, and its votes; i < 8, zeros from *n_out on. */
int bwtc_hip_test_period_winners(bwtc_hip_ctx* ctx, const uint32_t* table, uint32_t need, uint32_t* out, uint32_t* n_out);
/* Test hooks of the long periods (BWTC_HIP_LONG_PERIODS=1: periods 4097 ... 2^24; tests/longperiodmodel.py).  They run
 * whatever the switch says; a period step with such a period sets route bit 11 (2048) of bwtc_hip_stats.
 * _votes: the finder's two sweeps and its merged candidates over a given sorted list of m entries, ks[i] the key and vs[i]
 *   the suffix of entry i.  Neighbours with (ks[i] ^ ks[i + 1]) & kmask == 0 that lie d apart, 2 <= d <= 2^24, vote for d;
 *   with k1 != NULL (k1[0 ... max(vs)], the runs' lengths) a pair with k1[min(suffixes)] > d does not.  out16[2 i],
 *   out16[2 i + 1] = the distance with the i-th most votes among those with `need` votes or more, the smaller distance
 *   first among equals, and its votes, exactly; i < 8, zeros from *found on.  -1, before anything is launched, for m < 2,
 *   m or a suffix above the context's block size, need = 0 or (m - 1) / need > 64.
 * _probe: the probe of a period above 4096 over T[0..n): *flag_out = 1 when one of the windows of `span` positions that
 *   begin at p + i * span and end at or below n holds no position q with T[q] != T[q - p], else 0.  -1 for p outside
 *   4097 ... 2^24, span = 0, n = 0 or n above the context's block size.
 * _lengths: the sorter's period-length pass with both maxima for 4097 <= p <= 2^24 and p < n: k_out[s] as
 *   bwtc_hip_test_period_lengths gives it, longest2[0] their maximum, longest2[1] the longest proper stretch.  -1 outside
 *   that range or for n above the context's block size; k_out is not written then. */
int bwtc_hip_test_long_period_votes(bwtc_hip_ctx* ctx, const uint64_t* ks, const uint32_t* vs, uint32_t m, uint64_t kmask, const uint32_t* k1,
                                    uint32_t need, uint32_t* out16, uint32_t* found);
int bwtc_hip_test_long_period_probe(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t span, uint32_t* flag_out);
int bwtc_hip_test_long_period_lengths(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, uint32_t p, uint32_t* k_out, uint32_t* longest2);
/* Test hooks of the suffix sorter's code-key stage: k_pair_counts, k_code_build and
 * k_make_keys_code with suffix_sort's launch shapes and key layout (hi_shift = code_bits - 32, 13 upper bits of the suffix
 * number when split, then the predecessor's code, then the level), over T[0..n) as the sorter holds it (loaded by
 * load_text, zero padded), on the context's own buffers.  -1, before anything is launched, for n = 0, n + 256 above the
 * context's block size, code_bits outside 40..72, split with n > 2^29, and each hook's own contract; -20 - i when canary
 * i changed (keys, second words, plane, table).  A table is 257 rows of 256 entries, length << 27 | bits.
 *   _stage: the whole stage.  lone_sentinel: T[n-1] is T's only zero byte (-1 otherwise).  Out: the dense codes lut[256]
 *     and *sigma of plan_keys, the 65536 pair counts summed over the replicas, the table, the sort's error word, and
 *     (each may be null) keys, w and plane, n each, slot j for suffix n - 1 - j. */
int bwtc_hip_test_code_stage(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, int lone_sentinel, int code_bits, int split, uint8_t* lut_out,
                             uint32_t* sigma_out, uint32_t* counts_out, uint32_t* table_out, uint32_t* err_out, uint64_t* keys, uint32_t* w,
                             uint8_t* plane);
/*   _table: k_code_build alone over one replica's 65536 counts (the others zero): sigma in 1..256, the counts sum to at
 *     most 2^21 (the product's sample; -1 otherwise).  Out: the table and the error word. */
int bwtc_hip_test_code_table(bwtc_hip_ctx* ctx, const uint32_t* counts, uint32_t sigma, uint32_t* table_out, uint32_t* err_out);
/*   _keys: k_make_keys_code alone with the caller's lut[256], sigma and table: every byte of T and the padding's zero map
 *     below sigma, every row is prefix free over sigma symbols with lengths 1..26 (-1 otherwise).  Out: keys, w, plane. */
int bwtc_hip_test_code_keys(bwtc_hip_ctx* ctx, const uint8_t* T, uint32_t n, int code_bits, int split, const uint8_t* lut, uint32_t sigma,
                            const uint32_t* table, uint64_t* keys, uint32_t* w, uint8_t* plane);
/* Test hooks of the suffix sorter's finisher: ONE k_finish launch through the launch code of
 * finisher_passes / local_pass, over T[0..n) as the sorter holds it (loaded by load_text, zero padded), on the context's
 * own buffers.  All pointers are the caller's arrays.  The shape is set from the arguments (and restored): no
 * environment variable takes part.
 *   in:  the list (S suffix, P slot, H slot of the group's head, C predecessor byte | depth << 8) in nreg <= 16 regions
 *        [ebase[r], ebase[r] + ecount[r]) of arrays of `span` entries (where the last region ends); window / group 1024 /
 *        256 | 512 or 2048 / 256 | 512 | 1024; words 2, 3, 4; rounds 1..4 (1 unless words is 2); floor; out_n (n or
 *        n - 1); lf_n <= 256 and lf_x (n / lf_n where lf_n > 1).
 *   out: the next list in arrays of next_cap entries (at least the room the pass needs: workgroups x (window - group) +
 *        ceil(workgroups / 64) x group), region r at next_base[r] with next_count[r] entries, next_count[16] its groups;
 *        the hard list (hS, hHP = head << 32 | slot, hC) and the shallow list (sS, sHP), arrays of as many entries as
 *        the list has, with {entries, smallest depth} in hard_count[2] / shal_count[2]; SA[n], out[n], small = {pidx,
 *        last_char}, lf[256], all poisoned with 0xA5 bytes first.
 *   _local_pass (ranks != 0): k_finish<RANK> with rank[n], at, at2, then k_rank_updates over the regions read.  Out: the
 *        next list, the notes us / ur (span entries; us filled with all ones first), rank[] after the updates, the
 *        emissions; hC, sS, sHP are not used.
 * -1, before anything is launched, unless 1 <= n, n + 256 <= the context's capacity, 1 <= entries <= n, the regions
 * ascend, do not overlap and end (as does the room) 128 entries below capacity + capacity / 128 + 65536, every S < n and P
 * < n is distinct, a group is a maximal run of equal H inside a region whose j-th entry has P = H + j and whose members
 * carry one depth; with ranks also: every group has 2..group members, rank[] < n, 1 <= at, at2 = 0 or at2 > at, at2 +
 * (at2 - at) < 0xFFFFFFF0.  -20 - i when canary i changed (behind S, P, H, C of the list and of the next list, hS, hHP,
 * then hC, sS, sHP or us, ur). */
typedef struct bwtc_hip_fin_pass {
  uint32_t n, nreg;
  const uint32_t* ebase; const uint32_t* ecount;
  const uint32_t *S, *P, *H; const uint16_t* C;
  int window, group, words, rounds;
  uint32_t floor, out_n, lf_n, lf_x;
  int ranks;
  uint32_t* rank; uint32_t at, at2;
  uint32_t *us, *ur;
  uint32_t next_cap;
  uint32_t *nS, *nP, *nH; uint16_t* nC;
  uint32_t* next_base; uint32_t* next_count;
  uint32_t* hS; uint64_t* hHP; uint16_t* hC; uint32_t* hard_count;
  uint32_t* sS; uint64_t* sHP; uint32_t* shal_count;
  uint32_t* SA; uint8_t* out; uint32_t* small; uint32_t* lf;
} bwtc_hip_fin_pass;
int bwtc_hip_test_finish_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_pass* pass);
int bwtc_hip_test_local_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_pass* pass);
/*   _finisher: the driver finisher_passes(n, m, a, b, re, shal, &fo, keep_local, max_passes) over a list of m entries in
 *        one region, under the same contracts.  Out: outcome = {hard, hard_depth, left, local} (FinOutcome), info =
 *        {passes_done, stats.route, parked, park_holes, shallow entries, their smallest depth, the smallest depth of what
 *        waits for the rounds, local_depth}; the parked raw list (pS, pHP: `parked` entries, holes -- all ones --
 *        included), the shallow raw list (sS, sHP), the local list after k_list_copy (lS, lP, lH, lC: `local` entries),
 *        arrays of m entries each; SA[n], out[n], small = {pidx, last_char}, lf[256], poisoned first. */
typedef struct bwtc_hip_fin_run {
  uint32_t n, m;
  const uint32_t *S, *P, *H; const uint16_t* C;
  int window, group, words, rounds;
  uint32_t floor, out_n, lf_n, lf_x;
  int keep_local, max_passes;
  uint32_t* outcome; uint32_t* info;
  uint32_t* pS; uint64_t* pHP; uint32_t* sS; uint64_t* sHP;
  uint32_t *lS, *lP, *lH; uint16_t* lC;
  uint32_t* SA; uint8_t* out; uint32_t* small; uint32_t* lf;
} bwtc_hip_fin_run;
int bwtc_hip_test_finisher(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_fin_run* run);
/* Test hooks of the suffix sorter's ranking step and round kernels, over T[0..n) as the sorter
 * holds it (loaded by load_text, zero padded), on the context's own buffers.  All pointers are the caller's arrays; every
 * output is poisoned with 0xA5 bytes first and has 256 canary bytes behind the last item a kernel may write.  No
 * environment variable takes part.  -1, before anything is launched, where a contract below fails; -20 - i when canary i
 * changed.
 *   _rank_pass: ONE ranking through launch_rerank (k_rerank_reduce, k_rerank_scan_tiles<0>, <1>, k_rerank_apply), the
 *     launch code of rank_step, over a list of m items.
 *     in:  keys (m words of key_bytes = 4 or 8), idx (m 32-bit suffix numbers; split: m 16-bit lower halves, the upper
 *          bits in the key at bit 48, long items at hi_shift, 13 bits), w (long items' second words), aglob (rounds: the
 *          items' slots); short_len, kmask; the RrLong fields wmask, hi_shift, chr_shift, chr_mask, lvl_shift (-1: every
 *          item shares `depth`), depth; inv_lut[256] (emit 3); the form: init, split, lng, mode 0..3, emit 0..3; out_n,
 *          lf_n, lf_x, rec_shift and plane (mode 2).
 *     out: aggA/B/C (ceil(m / 2048) entries each) as apply read them, counts[2], rank[n] (mode 0), pair_s / pair_r (m
 *          each, mode 1), rec / val / rplane (m each, mode 2), the next list aidx / aglob_out / agrp (m each) and achr (2 m
 *          bytes: m characters, or in mode 3 m 16-bit entries), SA[n], out[n], small = {pidx, last_char}, lf[256].
 *     contracts: 1 <= m <= n, n + 256 <= the context's capacity; init: m == n; 4-byte keys, split and lng only with init
 *          (split, lng: 8-byte keys); every suffix number (the split undone) below n and distinct; rounds: aglob below n
 *          and strictly ascending, emit 0, 1 or 2; init: emit 0 or 2, long items 0 or 3, split items 0 or 2; split: n <=
 *          2^29; long: w given, wmask != 0, shifts below 64 (hi_shift + 13 <= 64 when split), chr_mask <= 255, lvl_shift
 *          -1 or <= 61, depth < 2^24; emit 3: inv_lut given; out_n = n or n - 1; lf_n <= 256, lf_x = n / lf_n >= 1 where
 *          lf_n > 1; rec_shift < 32.
 *   _rank_scan: k_rerank_scan_tiles<0> then <1> over a, b, c (ntiles entries each, scanned in place) on the engine's
 *     aggregate arrays; parts_out: the whole part array (3 words per 4096 entries, then poison; parts_cap words are
 *     written back, at most what the context holds), counts_out[2].  1 <= ntiles <= what the context reserved
 *     (block size / 2048 + 2).
 *   _rank_scatter: k_scatter_pairs (dense == 0: where[m], what[m]) or k_scatter_dense (rec[m] = s << 32 | value) with the
 *     engine's grid and bin_shift, into rank[n] as the caller preset it.  1 <= m <= n, n + 256 <= capacity, every
 *     destination below n and distinct, 0 <= bin_shift <= 24.
 *   _round_keys: kind 0 k_gather_key2, 1 k_gather_text, 2 k_gather_dense with the engine's launch shape.
 *     in:  the list aidx / agrp (kinds 0, 1), or the records rec (s << 32 | any) and values val (group, or all ones:
 *          finished) (kind 2, both rewritten in place); rank[n] or null (kind 0 only); achr[m] or null (kinds 0, 1); h; b2
 *          (kinds 0, 2) or c (kind 1) in bc; emit and bin_shift (kind 2); RunKeys: run_mode 0, 1, 2 with k[n], h_split, p.
 *     out: keys[m] (kind 2: rec), and for kind 2 val.
 *     contracts: 1 <= m <= n, n + 256 <= capacity; every suffix below n; rank[] below n; kinds 0, 2: 1 <= b2 <= 33, n <
 *          2^b2 (run_mode 1: n < 2^(b2 - 1)), every group << b2 below 2^56 (2^64 without achr / emit); kind 1: 1 <= c <= 6,
 *          every group << (8 c + 4) below 2^56; kind 2: rank given, 0 <= bin_shift <= 24; run_mode != 0: k given, k[s] <=
 *          n - s, 1 <= p; run_mode 1: p <= h (kind 1 has no run_mode 1); kind 1 with run_mode 2: h_split <= h. */
typedef struct bwtc_hip_rank_pass {
  uint32_t m, n;
  int key_bytes, init, split, lng, mode, emit;
  const void* keys; const void* idx; const uint32_t* w; const uint32_t* aglob;
  uint32_t short_len; uint64_t kmask;
  uint32_t wmask; int hi_shift, chr_shift; uint32_t chr_mask; int lvl_shift; uint32_t depth;
  const uint8_t* inv_lut;
  uint32_t out_n, lf_n, lf_x; int rec_shift, plane;
  uint32_t *aggA, *aggB, *aggC, *counts;
  uint32_t* rank; uint32_t *pair_s, *pair_r; uint64_t* rec; uint32_t* val; uint8_t* rplane;
  uint32_t *aidx, *aglob_out, *agrp; uint8_t* achr;
  uint32_t* SA; uint8_t* out; uint32_t* small; uint32_t* lf;
} bwtc_hip_rank_pass;
int bwtc_hip_test_rank_pass(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_rank_pass* pass);
int bwtc_hip_test_rank_scan(bwtc_hip_ctx* ctx, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t ntiles, uint32_t* parts_out, uint32_t parts_cap,
                            uint32_t* counts_out);
int bwtc_hip_test_rank_scatter(bwtc_hip_ctx* ctx, int dense, const uint32_t* where, const uint32_t* what, const uint64_t* rec, uint32_t m,
                               uint32_t n, int bin_shift, uint32_t* rank);
typedef struct bwtc_hip_round_keys {
  int kind; uint32_t m, n;
  const uint32_t *aidx, *agrp; uint64_t* rec; uint32_t* val;
  const uint32_t* rank; const uint8_t* achr;
  uint32_t h; int bc, emit, bin_shift;
  int run_mode; const uint32_t* k; uint32_t h_split, p;
  uint64_t* keys;
} bwtc_hip_round_keys;
int bwtc_hip_test_round_keys(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_round_keys* rk);
/*   _round: the driver, rank_step<u64, false>, ONCE, from the state run_rounds gives it in the finisher route (finished
 *     suffixes also go to SA; rank[] live), with pairs_min and window_bits set for this call and restored.
 *     in:  a sorted list ks / vs / aglob (m each), rank[n] (in and out), h_next, the flags emit, text, carry_in, raw_out
 *          (with text), run_mode 0, 1, 2 with k[n], step_p and step_depth (RunKeys::p and h_split), out_n, lf_n, lf_x.
 *     out: result = {m_next, groups, carry, text_chars, ran_run, finish}; the next list as sorted (nks, nvs: m_next
 *          entries) or, raw_out, the raw list's suffixes in nvs; naglob (slots), ngrp (the groups before the sort; raw_out:
 *          head slots), nchr (2 m bytes: characters, raw_out: 16-bit entries), m entries each; rank[]; SA, out, small, lf.
 *     contracts: the list's as for a round of _rank_pass; rank[] below n; 1 <= h_next; 1 <= pairs_min; 1 <= window_bits
 *          <= 32; raw_out only with text; run_mode != 0: k given, k[s] <= n - s, 1 <= step_p; run_mode 1: step_p <=
 *          h_next; text with run_mode 2: step_depth <= h_next; text: h_next < 2^31.  Canaries behind naglob, ngrp, nchr,
 *          rank, SA, out (the keys and values ping-pong between the sort's own arrays). */
typedef struct bwtc_hip_round {
  uint32_t m, n;
  const uint64_t* ks; const uint32_t* vs; const uint32_t* aglob;
  uint32_t* rank; const uint32_t* k;
  uint64_t h_next;
  int emit, text, carry_in, raw_out, run_mode;
  uint32_t step_p, step_depth, pairs_min; int window_bits;
  uint32_t out_n, lf_n, lf_x;
  uint32_t* result; uint64_t* nks; uint32_t* nvs; uint32_t* naglob; uint32_t* ngrp; uint8_t* nchr;
  uint32_t* SA; uint8_t* out; uint32_t* small; uint32_t* lf;
} bwtc_hip_round;
int bwtc_hip_test_round(bwtc_hip_ctx* ctx, const uint8_t* T, bwtc_hip_round* round);
/* Test hook: k range-coder chains over w-elements (w = bit << 15 | probability of the coded bit), chain j = elements
 * [bounds[j], bounds[j+1]), on the GPU lane engine (mode 0; BitEncoder, BitCoders.cpp:59-113, one lane per chain) or by the
 * host's scalar loop (mode 1); bytes of chain j = out[offsets[j] .. offsets[j+1]). */
int bwtc_hip_test_gpu_lanes(bwtc_hip_ctx* ctx, const uint16_t* w, uint64_t n, const uint64_t* bounds, uint32_t k, int mode,
                            uint8_t* out, uint64_t out_cap, uint64_t* offsets);

/* Test hooks of the 'B' coder's model passes (wavelet_gpu_models.hip / .hpp).
 * _test_models runs the product's wavelet_models_prepare (from "tasks and chunks are known" on, read_ends on) and
 * wavelet_models_run over caller-given packed streams (16 elements per word: bit 0 the bit, bit 1 the gap flag;
 * (n_coded + 15) / 16 words, padded on the device to whole 16-byte pieces by the hook) and tasks (three words each:
 * begin, end, type 0 root | 1 gaps | 2 inner | 3 integers), and copies back w, the tail words and what every pass left.
 * flags: bit 0 = the lines form of the partition pass for this call, bit 1 = no intermediate copies (only w, tail,
 * ends, nc, nsc).  Checked before anything is launched, -1 otherwise: no null argument, n_coded > 0, nt > 0, every
 * type <= 3, tasks non-empty and tiling [0, n_coded) in order, the packed streams within the context's workspace
 * (n_coded <= 32 * (max_block + 1)).  Room the caller gives: chunks 3 words for each of nt + n_coded / 2048 chunks
 * (begin, end, task | first chunk of its task << 31), cmap and cstate one per chunk, base 15 per chunk + 1,
 * sb 15 nt + 1, sbits n_coded / 32 + 16, smap 2 words per slot-chunk of 2048 ({base L | end value << 16, mask}),
 * snaps 2 words per 32 positions ({value of the lowest candidate, mask}), sstart one per slot-chunk. */
typedef struct bwtc_hip_models_out {
  uint16_t* w;                 /* n_coded */
  uint32_t tail[4];            /* state after the block, error flags, elements counted, scan error */
  uint32_t ends[8];            /* the state after the block by the state it starts in */
  uint32_t nc, nsc;            /* chunks, slot-chunks */
  uint32_t* chunks; uint64_t* cmap; uint32_t* cstate; uint32_t* base; uint32_t* sb; uint32_t* sbits;
  uint32_t* smap; uint32_t* snaps; uint16_t* sstart;
} bwtc_hip_models_out;
int bwtc_hip_test_models(bwtc_hip_ctx* ctx, const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks, uint32_t nt,
                         uint32_t state_in, uint32_t flags, bwtc_hip_models_out* out);
/* The same passes for a main model given by its letter ('B' as above, 'b', 'u'; -1 for any other).  For 'b' and 'u'
 * nothing is carried: state_in changes nothing, tail[0] is what every task starts from (3, 0), ends[i] = i, and in
 * slot space (smap, snaps, sstart) a main slot's value is its counter's index 0, 1, 2. */
int bwtc_hip_test_models_letter(bwtc_hip_ctx* ctx, char letter, const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks,
                                uint32_t nt, uint32_t state_in, uint32_t flags, bwtc_hip_models_out* out);
/* The same input through the passes run lane by lane on the host (gm::modelsOnHostLanes; no context, no device), in
 * buffers of exactly the sizes the device path allots: w_out[n_coded], *state_out the state after the block.
 * -1 as above, -7: the passes raised their error flag. */
int bwtc_hip_host_test_models(const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks, uint32_t nt,
                              uint32_t state_in, uint16_t* w_out, uint32_t* state_out);
int bwtc_hip_host_test_models_letter(char letter, const uint32_t* packed, uint32_t n_coded, const uint32_t* tasks, uint32_t nt,
                                     uint32_t state_in, uint16_t* w_out, uint32_t* state_out);
/* The coded elements of a real block (arguments as bwtc_hip_host_wavelet_streams): *n_coded and *nt always; where
 * packed, tasks and w are given (room: packed_words, tasks_cap tasks of three words, w_cap elements; -1 when too
 * small) also the packed codes, the model tasks in coding order and the w of the SEQUENTIAL host coder
 * (StreamCoder::model over planStreams / expandStreamsOnHost).  state: the carried state, updated.  -5 / -3 as there. */
int bwtc_hip_host_wavelet_elements(uint32_t n_sections, const uint32_t* first_run,
                                   const uint8_t* run_sym, const uint32_t* run_start,
                                   const uint32_t* run_freqs, const uint32_t* dist_offset,
                                   const uint32_t* dist_len, const uint32_t* dist_cnt, uint32_t* state,
                                   uint32_t* n_coded, uint32_t* nt, uint32_t* packed, uint64_t packed_words,
                                   uint32_t* tasks, uint32_t tasks_cap, uint16_t* w, uint64_t w_cap);
/* ... and of the sequential host coder under another main model ('B', 'b', 'u'; -1 for any other letter) */
int bwtc_hip_host_wavelet_elements_letter(char letter, uint32_t n_sections, const uint32_t* first_run,
                                          const uint8_t* run_sym, const uint32_t* run_start,
                                          const uint32_t* run_freqs, const uint32_t* dist_offset,
                                          const uint32_t* dist_len, const uint32_t* dist_cnt, uint32_t* state,
                                          uint32_t* n_coded, uint32_t* nt, uint32_t* packed, uint64_t packed_words,
                                          uint32_t* tasks, uint32_t tasks_cap, uint16_t* w, uint64_t w_cap);

/* ---- pair-replacing pre-stage, `--prepr p...` ------------------------------------------
 * Replaces preprocessors/PairReplacer.cpp (analyseData :53-63, decideReplacements :402-484,
 * writeReplacedVersion :330-400), Grammar.cpp (writeGrammar :309-320, readGrammar :198-307),
 * Precompressor::precompress (Precompressor.cpp:62-121) and Postprocessor::uncompress (Postprocessor.cpp:112-133).
 * A grammar object is what a PrecompressorBlock carries (PrecompressorBlock.hpp:70): it is updated by every
 * round over the block and written into the block's header (PrecompressorBlock.cpp:64-90). */
typedef struct bwtc_hip_grammar bwtc_hip_grammar;
bwtc_hip_grammar* bwtc_hip_grammar_create(void);                       /* Grammar::Grammar: no rules */
void     bwtc_hip_grammar_destroy(bwtc_hip_grammar* g);
uint32_t bwtc_hip_grammar_rules(const bwtc_hip_grammar* g);            /* Grammar::numberOfRules          */
uint32_t bwtc_hip_grammar_special_symbols(const bwtc_hip_grammar* g);  /* Grammar::numberOfSpecialSymbols */
int      bwtc_hip_grammar_is_special(const bwtc_hip_grammar* g, unsigned symbol);
/* Grammar::writeGrammar into out (cap bytes): 0, *bytes = size; -1 when it does not fit */
int      bwtc_hip_grammar_write(const bwtc_hip_grammar* g, uint8_t* out, uint64_t cap, uint64_t* bytes);
/* Grammar::readGrammar into an EMPTY grammar: 0, *consumed = bytes read; -1 when the input is cut short */
int      bwtc_hip_grammar_read(bwtc_hip_grammar* g, const uint8_t* in, uint64_t n, uint64_t* consumed);
/* One PairReplacer (analyseData + decideReplacements + writeReplacedVersion) over a device-resident text of
 * 3 <= n < 2^31 bytes: d_src -> d_dst (room for 2 n bytes; must not overlap), *n_out = the new length,
 * *replaced = pairs replaced (0: the text is copied unchanged). */
int      bwtc_hip_pair_replace_device(bwtc_hip_ctx* ctx, bwtc_hip_grammar* g, const uint8_t* d_src, uint64_t n,
                                      uint8_t* d_dst, uint64_t* n_out, uint32_t* replaced);
/* Test hook: the statistics step of bwtc_hip_pair_replace_device alone (the same function: counters cleared, counted,
 * read back) over a device-resident text: pair_cnt[first << 8 | second] (65536 words) and byte_cnt (256 words), host
 * buffers.  -1 for n < 3 or n >= 2^31, as there. */
int      bwtc_hip_test_pair_stats(bwtc_hip_ctx* ctx, const uint8_t* d_src, uint64_t n, uint32_t* pair_cnt, uint32_t* byte_cnt);
/* Precompressor::precompress over a host block, in place: one round per letter of `options` ('p'), stopped by the
 * first round that does not shorten the block; *n_out = the new length.  Blocks shorter than three bytes are left
 * alone (the reference asserts length > 2). */
int      bwtc_hip_precompress(bwtc_hip_ctx* ctx, bwtc_hip_grammar* g, const char* options, uint8_t* block, uint64_t n,
                              uint64_t* n_out);
/* the same with both sweeps on the calling thread (no device; the CPU test suite, and the mirror's blocks below 64 KiB) */
int      bwtc_hip_host_precompress(bwtc_hip_grammar* g, const char* options, uint8_t* block, uint64_t n, uint64_t* n_out);
/* Postprocessor::uncompress: data (n bytes) expanded into out (cap bytes); -1 when it does not fit */
int      bwtc_hip_postprocess(const bwtc_hip_grammar* g, const uint8_t* data, uint64_t n, uint8_t* out, uint64_t cap,
                              uint64_t* n_out);
/* ---- Postprocessor on the device (postprocess.hip) --------------------------------------------------
 * The grammar's expansion table is built on the host; lengths are summed per tile, the tiles' offsets come from a
 * device scan, the bytes are written by a gather from the table's pool.  The device workspace (per-tile words,
 * table, pool, the staging of _block) is the postprocessor's own, made by the first call and grown on demand
 * (bwtc_hip_postprocess_stats: workspace_bytes).  Blocks of n >= 2^31 or cap >= 2^32 bytes take the host function
 * (same bytes), as bwtc_hip_precompress does. */
/* Postprocessor::uncompress(const byte* data, size_t length, OutStream* to, size_t originalSize)
 * (preprocessors/Postprocessor.cpp:112-133) with the block and its expansion in device memory: d_data (n bytes) ->
 * d_out (cap bytes; must not overlap d_data), *n_out = the expansion's size.  -1: bad arguments, or the expansion
 * does not fit cap (nothing has been written to d_out then); -2 / -3 as everywhere. */
int      bwtc_hip_postprocess_device(bwtc_hip_ctx* ctx, const bwtc_hip_grammar* g, const uint8_t* d_data, uint64_t n,
                                     uint8_t* d_out, uint64_t cap, uint64_t* n_out);
/* The same interface with host buffers, as bwtc_hip_postprocess has them: data goes up, is expanded on the device
 * and comes down once. */
int      bwtc_hip_postprocess_block(bwtc_hip_ctx* ctx, const bwtc_hip_grammar* g, const uint8_t* data, uint64_t n,
                                    uint8_t* out, uint64_t cap, uint64_t* n_out);
/* HuffmanDecoder::decodeBlock (HuffmanCoders.cpp:324-616) plus InverseBWTransform::doTransform
 * (InverseBWT.cpp:47-51) like bwtc_hip_decode_block_H, with the original block left in DEVICE memory at d_out (cap
 * bytes; the record still comes from the host): the slices of one precompressor block are decoded side by side into
 * one device buffer (Decompressor.cpp:71-80) and expanded there.  Same error codes. */
int      bwtc_hip_decode_block_H_device(bwtc_hip_ctx* ctx, const uint8_t* rec, uint64_t rec_bytes, uint8_t* d_out,
                                        uint64_t cap, uint32_t* size, uint64_t* consumed);
/* What the last postprocess on this context did. */
typedef struct bwtc_hip_postprocess_stats {
  uint32_t route;             /* 1: the device made the bytes, 2: the host function (the limits above)          */
  uint32_t launches;          /* kernels launched                                                                */
  uint64_t tokens;            /* tokens of the block (single bytes and pairs)                                    */
  uint64_t pair_tokens;       /* ... of which pairs that start with a special symbol                             */
  uint64_t in_bytes;          /* n                                                                               */
  uint64_t out_bytes;         /* the expansion's size                                                            */
  uint64_t pool_bytes;        /* bytes of the expansion table's pool                                             */
  uint64_t workspace_bytes;   /* device memory the postprocessor holds                                           */
  float    ms_device;         /* device time of the passes (event pairs on the context's stream)                 */
} bwtc_hip_postprocess_stats;
int      bwtc_hip_postprocess_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_postprocess_stats* out);
/* Host twin of the device passes (no device work): the same run starts, per-tile counts, offsets and the write
 * pass's search from the output's side, over tiles of `tile` bytes on the calling thread.  Same results as
 * bwtc_hip_postprocess. */
int      bwtc_hip_host_postprocess_tiles(const bwtc_hip_grammar* g, const uint8_t* data, uint64_t n, uint8_t* out,
                                         uint64_t cap, uint64_t* n_out, uint32_t tile);

/* ---- 'B' / 'b' / 'u' decoding: host range decoder + wavelet rebuild on the device ------------------------------- */

/* Return codes of the wavelet rebuild (beside the record-level BWTC_HIP_E_* above).  Every device loop is bounded
 * by a node's bit count, a step cap and the output's capacity: no input makes a kernel write past out + cap. */
#define BWTC_HIP_E_W_CHILD   (-20)  /* a run's path asks for a child the tree does not have                      */
#define BWTC_HIP_E_W_BITS    (-21)  /* a node has fewer bits than the runs that reach it                          */
#define BWTC_HIP_E_W_ESCAPE  (-22)  /* an escape code with more than 32 leading ones                              */
#define BWTC_HIP_E_W_TOTAL   (-23)  /* a section's run lengths do not add up to its announced bytes               */
#define BWTC_HIP_E_W_CAP     (-24)  /* the sections' bytes go past the output's capacity                          */
#define BWTC_HIP_E_W_DEPTH   (-25)  /* a path longer than its tree has nodes (child links that form a cycle)      */
#define BWTC_HIP_E_W_LIMIT   (-26)  /* beyond the device route's limits (block below 2^31 bytes, words below 2^32
                                       and below 4 x bytes + nodes): the caller takes the host route; the decoder
                                       handle is as it was before the call                                        */
#define BWTC_HIP_E_W_FOREST  (-27)  /* a table entry that points outside its table                                */

/* A block's decoded wavelet trees, flattened: what WaveletTree::decodeTreeBF leaves, and all WaveletTree::message
 * needs.  Child links are relative to their section's first node (-1: none). */
typedef struct bwtc_hip_wforest_section {
  uint32_t runs;          /* rootSize: bits of the root = runs of the section                                    */
  uint32_t bytes;         /* the section's announced length                                                      */
  uint32_t first_node;    /* root of the symbol tree in nodes[]                                                  */
  uint32_t symbol_nodes;  /* nodes of the symbol tree; run-length data nodes follow                              */
  uint32_t n_nodes;       /* all nodes of the section                                                            */
  uint32_t first_code;    /* root of the run-length code tree in codes[]                                         */
  uint32_t n_codes;
  uint32_t W;             /* width parameter of the escape code, 0..15                                           */
  uint32_t plain_fixed;   /* no length has a code of its own: every run is escape coded                          */
} bwtc_hip_wforest_section;
typedef struct bwtc_hip_wforest_node {
  int32_t  left, right;
  uint32_t has_symbol;    /* a leaf of the symbol tree                                                           */
  uint32_t symbol;
  uint32_t bits;          /* bits of this node                                                                   */
  uint32_t first_word;    /* where they start in words[] (bit i of the node = bit i % 64 of word i / 64)         */
} bwtc_hip_wforest_node;
typedef struct bwtc_hip_wforest_code {
  int32_t  left, right;
  uint32_t has_symbol;
  uint32_t symbol;        /* run length; 0 = escape                                                              */
} bwtc_hip_wforest_code;
typedef struct bwtc_hip_wforest {
  const bwtc_hip_wforest_section* sections; uint32_t n_sections;
  const bwtc_hip_wforest_node*    nodes;    uint32_t n_nodes;
  const bwtc_hip_wforest_code*    codes;    uint32_t n_codes;
  const uint64_t*                 words;    uint64_t n_words;
} bwtc_hip_wforest;

/* What the last wavelet decode / rebuild on this context did. */
typedef struct bwtc_hip_wavelet_decode_stats {
  uint32_t route;             /* 1: the device kernels made the BWT bytes                                        */
  uint32_t sections;          /* non-empty sections                                                              */
  uint64_t routed_device;     /* calls so far on this context whose bytes the device kernels made                */
  uint64_t runs;
  uint64_t nodes;
  uint64_t words;
  uint64_t bit_reads;         /* bits taken out of nodes by the run walks (counted on the device)                */
  uint64_t launches;          /* kernels launched                                                                */
  uint64_t workspace_bytes;   /* device memory the rebuild holds                                                 */
  float    ms_range_decode;   /* host: header, shapes and the range decoder (decode_block_W only)                */
  float    ms_rebuild;        /* device span: upload of the forest to BWT bytes                                  */
  float    ms_inverse;        /* device time of the inverse transform (decode_block_W only)                      */
} bwtc_hip_wavelet_decode_stats;
int bwtc_hip_wavelet_decode_stats_get(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decode_stats* out);

/* The range decoder's state (three adaptive model sets and the coder) of one stream: the main model's state carries
 * on from block to block, so one handle decodes a stream's blocks in order.  coder: 'B', 'b' or 'u'. */
typedef struct bwtc_hip_wavelet_decoder bwtc_hip_wavelet_decoder;
bwtc_hip_wavelet_decoder* bwtc_hip_wavelet_decoder_create(char coder);
void bwtc_hip_wavelet_decoder_destroy(bwtc_hip_wavelet_decoder* d);
void bwtc_hip_wavelet_decoder_reset(bwtc_hip_wavelet_decoder* d);

/* Twin of bwtc_hip_decode_block_H for the wavelet coders: record (host) -> the original block in out (host, cap
 * bytes).  The host range-decodes the record into a flattened forest in page-locked staging, which goes up once;
 * the device rebuilds the BWT bytes (rank directory, run walk, expansion) and inverts them with the header's LF
 * powers.  The rebuild's workspace is its own, made by the first call and grown on demand.  cap is clipped to
 * the context's max_block_size (BWTC_HIP_E_CAPACITY beyond).  An error of the range decoder (the record-level codes,
 * BWTC_HIP_E_W_LIMIT) or a forest the kernels refuse (BWTC_HIP_E_W_*): any non-zero return leaves the decoder handle
 * as it was before the call, so the caller can take another route with the same handle. */
int bwtc_hip_decode_block_W(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes,
                            uint8_t* out, uint64_t cap, uint32_t* size, uint64_t* consumed);
/* Same with the original block left in device memory at d_out. */
int bwtc_hip_decode_block_W_device(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decoder* dec, const uint8_t* rec,
                                   uint64_t rec_bytes, uint8_t* d_out, uint64_t cap, uint32_t* size, uint64_t* consumed);
/* The same block in two halves, so that a caller's worker thread can run block k's device half while the calling
 * thread range-decodes block k+1 (the range decoder is serial by the format; nothing else has to wait for it).
 * _begin is the host half: header, shapes and the range decoder, into forest slot `slot` (0 or 1) of the context,
 * page-locked; *size = the block's bytes.  It does no device work and touches no statistics, and it may run while
 * another thread is inside _end of the OTHER slot; every other pair of calls on one context is the caller's to
 * order.  An error leaves the decoder handle as it was.  _end / _end_device is the device half of the slot: upload,
 * rebuild, inverse (and download through page-locked memory); by then the models have moved on, and a forest the
 * kernels refuse ends the stream. */
int bwtc_hip_decode_block_W_begin(bwtc_hip_ctx* ctx, bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes,
                                  uint64_t cap, uint32_t slot, uint32_t* size, uint64_t* consumed);
int bwtc_hip_decode_block_W_end(bwtc_hip_ctx* ctx, uint32_t slot, uint8_t* out, uint64_t cap, uint32_t* size);
int bwtc_hip_decode_block_W_end_device(bwtc_hip_ctx* ctx, uint32_t slot, uint8_t* d_out, uint64_t cap, uint32_t* size);
/* Pure host route with the same handle (no device work): record -> BWT bytes in bwt_out and the LF powers in
 * lf_out[256].  For blocks below the device route's floor or beyond its limits. */
int bwtc_hip_wavelet_decode_bwt_host(bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes,
                                     uint8_t* bwt_out, uint64_t cap, uint32_t* lf_out, uint32_t* n_lf, uint32_t* size,
                                     uint64_t* consumed);
/* The record's forest alone (host; what the device route uploads): counts for tests and tools.  counts[0..5] =
 * sections, runs, nodes, words, bytes, bits taken out of nodes (counted by the host twin of the kernels, which
 * writes the block into a scratch buffer of its size: -2 when that cannot be had). */
int bwtc_hip_wavelet_decode_counts(bwtc_hip_wavelet_decoder* dec, const uint8_t* rec, uint64_t rec_bytes, uint64_t cap,
                                   uint64_t* counts, uint64_t* consumed);

/* A view of the forest the handle's last bwtc_hip_wavelet_decode_bwt_host / _decode_counts call decoded (and its LF
 * powers, lf_out[256]; both may be null): valid until the next call on the handle.  What the rebuild entry points
 * below take, for a real record. */
int bwtc_hip_wavelet_decoder_forest(bwtc_hip_wavelet_decoder* dec, bwtc_hip_wforest* out, uint32_t* lf_out, uint32_t* n_lf);

/* Flattened forest -> BWT bytes on the device: out is host memory (rebuild) or device memory at any alignment
 * (rebuild_device).  *size = the sections' bytes. */
int bwtc_hip_wavelet_rebuild(bwtc_hip_ctx* ctx, const bwtc_hip_wforest* forest, uint8_t* out, uint64_t cap, uint64_t* size);
int bwtc_hip_wavelet_rebuild_device(bwtc_hip_ctx* ctx, const bwtc_hip_wforest* forest, uint8_t* d_out, uint64_t cap,
                                    uint64_t* size);
/* Host twin of the kernels (no device work): the same rank-directory walk on the calling thread, with one
 * directory entry per `line_words` words (the device uses 7).  Same bytes, same error codes; *bit_reads (may be
 * null) = bits taken out of nodes. */
int bwtc_hip_host_wavelet_rebuild(const bwtc_hip_wforest* forest, uint8_t* out, uint64_t cap, uint64_t* size,
                                  uint32_t line_words, uint64_t* bit_reads);

#ifdef __cplusplus
}
#endif
#endif
