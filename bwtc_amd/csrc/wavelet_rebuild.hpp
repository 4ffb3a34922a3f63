// The wavelet rebuild: a block's decoded wavelet trees (what the range decoder leaves) -> BWT bytes.
// WaveletTree::message (WaveletTree.hpp:1277-1378) takes every node's bits in order, so the position of a run in a
// child is the rank of its bit in the parent: a run's walk is the textbook wavelet-tree access and needs no
// cursor.  wr_walk below is that walk, written once for the kernels (wavelet_rebuild.hip) and their host twin.
#pragma once
#include <cstdlib>
#include <vector>

#include "bwtc_hip.h"
#include "common.hpp"

#if defined(__HIPCC__)
#define WR_HD __host__ __device__ __forceinline__
#else
#define WR_HD inline
#endif

namespace bwtc_hip {

struct BwtEngine;

// tables as the walks read them: links absolute, the node's rank origin beside its bits
struct alignas(32) WrNode {
  int left, right;
  u32 sym;          // bit 31: leaf of the symbol tree; low byte: its symbol
  u32 bits;
  u32 first_word;
  u32 rank0;        // ones of the whole word array before first_word (mod 2^32)
  u32 pad0, pad1;
};
struct alignas(16) WrCode { int left, right; u32 has_symbol, symbol; };
struct WrSection {
  u32 run_start, runs, bytes, first_node, symbol_nodes, n_nodes, first_code, n_codes, W, plain_fixed;
};

constexpr u32 kWrLineWords = 7;        // device directory: 7 words of bits + their prefix = one 64-byte line
constexpr u32 kWrMaxLeadingOnes = 32;
constexpr u32 kWrMaxSections = 256;
constexpr u32 kWrSlots = 2;            // forests a context holds: one being decoded, one being rebuilt

// walk results: 0 or the BWTC_HIP_E_W_* code of the first thing wrong on the path
template <class Rank>
WR_HD int wr_take(const WrNode& n, const Rank& rank, u32& pos, bool& bit) {
  if (pos >= n.bits) return BWTC_HIP_E_W_BITS;
  u64 w;
  const u32 ones = rank(n.first_word + (pos >> 6), pos & 63u, w) - n.rank0;
  bit = (w >> (pos & 63u)) & 1u;
  pos = bit ? ones : pos - ones;              // where this run sits in the child it goes to
  return 0;
}

// run i of section S: its symbol, its length (clipped to 2^32-1) and the bits it took
template <class Rank>
WR_HD int wr_walk(const WrSection& S, const WrNode* __restrict__ nodes, const WrCode* __restrict__ codes, const Rank& rank,
                  u32 i, u32* sym_out, u64* len_out, u32* reads_out) {
  u32 pos = i, reads = 0, steps = 0;
  int nd = (int)S.first_node;
  WrNode cur = nodes[nd];
  bool bit = false;
  int rc;
  *reads_out = 0;
  do {                                                               // the symbol tree
    if ((rc = wr_take(cur, rank, pos, bit)) != 0) return rc;
    ++reads;
    nd = bit ? cur.right : cur.left;
    if (nd < 0) return BWTC_HIP_E_W_CHILD;
    if ((u32)nd - S.first_node >= S.symbol_nodes || ++steps > S.symbol_nodes) return BWTC_HIP_E_W_DEPTH;
    cur = nodes[nd];
  } while (!(cur.sym >> 31));
  *sym_out = cur.sym & 0xFFu;
  u64 len = 0;
  if (!S.plain_fixed) {                                              // the length code: data nodes and code nodes in step
    int code = (int)S.first_code;
    WrCode c = codes[code];
    steps = 0;
    do {
      if ((rc = wr_take(cur, rank, pos, bit)) != 0) return rc;
      ++reads;
      nd = bit ? cur.right : cur.left;
      code = bit ? c.right : c.left;
      if (nd < 0 || code < 0) return BWTC_HIP_E_W_CHILD;
      if (++steps > S.n_codes) return BWTC_HIP_E_W_DEPTH;
      cur = nodes[nd];
      c = codes[code];
    } while (!c.has_symbol);
    len = c.symbol;
  }
  if (len == 0) {                                                    // escape: leading ones, then leadingOnes + W bits
    u32 ones = 0;
    if ((rc = wr_take(cur, rank, pos, bit)) != 0) return rc;
    ++reads;
    while (bit) {
      if (++ones > kWrMaxLeadingOnes) return BWTC_HIP_E_W_ESCAPE;
      nd = cur.right;
      if (nd < 0) return BWTC_HIP_E_W_CHILD;
      cur = nodes[nd];
      if ((rc = wr_take(cur, rank, pos, bit)) != 0) return rc;
      ++reads;
    }
    for (u32 k = 0; k < ones + S.W; ++k) {
      nd = bit ? cur.right : cur.left;
      if (nd < 0) return BWTC_HIP_E_W_CHILD;
      cur = nodes[nd];
      if ((rc = wr_take(cur, rank, pos, bit)) != 0) return rc;
      ++reads;
      len = (len << 1) | (bit ? 1u : 0u);
    }
    len += 1 + (((u64(1) << ones) - 1) << S.W);
  }
  *len_out = len > 0xFFFFFFFFull ? 0xFFFFFFFFull : len;
  *reads_out = reads;
  return 0;
}

// ---- host half (wavelet_decode_host.cpp) -----------------------------------------------------------------------

// the flattened word array grows as the range decoder goes; the device route keeps it in page-locked memory
struct WrWordBuf {
  u64* p = nullptr;
  u64 cap = 0;                                                       // words
  void* (*alloc)(u64 bytes) = nullptr;                               // null: malloc / free
  void (*release)(void*) = nullptr;
  bool reserve(u64 words);
  void drop();
};

struct WrForest {
  std::vector<bwtc_hip_wforest_section> sections;
  std::vector<bwtc_hip_wforest_node> nodes;
  std::vector<bwtc_hip_wforest_code> codes;
  WrWordBuf words;
  u64 n_words = 0, runs = 0, bytes = 0;
  u32 lf[256];
  u32 n_lf = 0;
  bwtc_hip_wforest view() const {
    bwtc_hip_wforest f;
    f.sections = sections.data(); f.n_sections = (u32)sections.size();
    f.nodes = nodes.data(); f.n_nodes = (u32)nodes.size();
    f.codes = codes.data(); f.n_codes = (u32)codes.size();
    f.words = words.p; f.n_words = n_words;
    return f;
  }
};

struct WDecoderState;                                                // models + coder letter
WDecoderState* wdecoder_create(char coder);
void wdecoder_destroy(WDecoderState* d);
void wdecoder_reset(WDecoderState* d);
// record -> forest; 0 or an error code, and then the decoder is as it was before the call
int wavelet_range_decode(WDecoderState& d, const u8* rec, u64 rec_bytes, u64 cap, WrForest& out, u64* consumed);
// takes the last successful wavelet_range_decode back (once): the models as they were before it
void wdecoder_undo(WDecoderState* d);

// ---- tables and the host twin (wavelet_rebuild.hip) --------------------------------------------------------------

// checks every link and extent of a forest and restates it with absolute links; *total = the sections' bytes
int wr_flatten(const bwtc_hip_wforest& f, u64 cap, std::vector<WrSection>& secs, std::vector<WrNode>& nodes,
               std::vector<WrCode>& codes, u64* total, u64* runs);
int host_wavelet_rebuild(const bwtc_hip_wforest& f, u8* out, u64 cap, u64* size, u32 line_words, u64* bit_reads);

struct WRebuild;                                                     // device workspace of one context
WRebuild* wrebuild_create();
void wrebuild_destroy(WRebuild* w);
int wrebuild_stats(WRebuild* w, bwtc_hip_wavelet_decode_stats* out);
// forest -> BWT bytes at d_out (device, any alignment; null: the workspace's own buffer, returned in *d_bwt)
int wavelet_rebuild_device(BwtEngine& e, WRebuild& w, const bwtc_hip_wforest& f, u8* d_out, u64 cap, u64* size, u8** d_bwt);
// a block in two halves: begin = the range decoder into forest slot `slot` (host only; may run beside the end of the
// other slot on another thread), end = upload, rebuild, inverse (and download)
int wavelet_decode_begin(BwtEngine& e, WRebuild& w, WDecoderState& dec, const u8* rec, u64 rec_bytes, u64 cap, u32 slot, u32* size,
                         u64* consumed);
int wavelet_decode_end_device(BwtEngine& e, WRebuild& w, u32 slot, u8* d_out, u64 cap, u32* size);
int wavelet_decode_end(BwtEngine& e, WRebuild& w, u32 slot, u8* out, u64 cap, u32* size);
int wavelet_decode_block_device(BwtEngine& e, WRebuild& w, WDecoderState& dec, const u8* rec, u64 rec_bytes, u8* d_out, u64 cap,
                                u32* size, u64* consumed);
int wavelet_decode_block(BwtEngine& e, WRebuild& w, WDecoderState& dec, const u8* rec, u64 rec_bytes, u8* out, u64 cap, u32* size,
                         u64* consumed);

}  // namespace bwtc_hip
