// GPU decoder of 'H' records (huffman_decoder.hip).  The workspace is the decoder's own, made by
// the first decode call and grown when a later record needs more; bwtc_hip_create's arena is left
// as it is.
#pragma once
#include "common.hpp"
#include "bwtc_hip.h"

namespace bwtc_hip {

struct BwtEngine;
struct HDecoder;

// return codes of a corrupt record (bwtc_hip.h)
constexpr int kHdNoCode = BWTC_HIP_E_NO_CODE;
constexpr int kHdShape = BWTC_HIP_E_SHAPE;
constexpr int kHdPastRecord = BWTC_HIP_E_PAST_RECORD;
constexpr int kHdRuns = BWTC_HIP_E_RUNS;
constexpr int kHdCapacity = BWTC_HIP_E_CAPACITY;
constexpr int kHdLength = BWTC_HIP_E_LENGTH;

HDecoder* hdecoder_create();
void hdecoder_destroy(HDecoder* d);
int hdecoder_stats(HDecoder* d, bwtc_hip_huffman_decode_stats* out);
u8* hdecoder_bwt_buffer(HDecoder* d);

// record (host `rec`, or device `d_rec_src` with its host copy in `rec`) -> BWT bytes in d_out
// (device; null: the decoder's own buffer) and the LF powers
int huffman_decode(BwtEngine& e, HDecoder& d, const u8* rec, const u8* d_rec_src, u64 rec_bytes, u8* d_out, u64 cap,
                   u32* lf_out, u32* n_lf_out, u32* size_out, u64* consumed_out);
// the same plus the inverse transform; out = host
int huffman_decode_block(BwtEngine& e, HDecoder& d, const u8* rec, u64 rec_bytes, u8* out, u64 cap, u32* size_out,
                         u64* consumed_out);
// the same with the original block left in device memory at d_out
int huffman_decode_block_device(BwtEngine& e, HDecoder& d, const u8* rec, u64 rec_bytes, u8* d_out, u64 cap, u32* size_out,
                                u64* consumed_out);

}  // namespace bwtc_hip
