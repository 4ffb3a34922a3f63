// The batched block transform (batch_bwt.hip): K small blocks through one plain, segmented prefix doubling, so that
// the launches and host waits of a transform are paid once per batch and not once per block.  The rule is stated in
// tests/batchmodel.py; DESIGN.md section 3, "The batched sorter".
#pragma once
#include "bwt_engine.hpp"

namespace bwtc_hip {

constexpr u32 kBatchMaxBlocks = 4096;    // 12 bits of block id in the initial key
constexpr int kBatchKeyChars = 6;        // characters in the initial key: the first round's depth

// Checks the items (bwtc_hip.h lists the refusals) and gives the stride's log2.  -1: refused.
int batch_validate(const BwtEngine& e, const bwtc_hip_batch_item* items, u32 k, u32* stride_log2);
// d_in + offset -> d_out + offset for every block (d_in == d_out is fine: the load pass has consumed a block's bytes
// before the emit pass writes any).  lf: k rows of 256; freqs: k rows of 256, incremented, or null.
int batch_transform_device(BwtEngine& e, const u8* d_in, u8* d_out, const bwtc_hip_batch_item* items, u32 k,
                           u32* lf, u32* freqs, bwtc_hip_batch_stats* bs);
// the same for host bytes: the blocks are packed into the context's staging buffer, uploaded once and brought back once
int batch_transform_host(BwtEngine& e, u8* data, const bwtc_hip_batch_item* items, u32 k, u32* lf, u32* freqs,
                         bwtc_hip_batch_stats* bs);
// test hook: k_batch_load and k_batch_keys alone
int batch_test_keys(BwtEngine& e, const u8* data, const bwtc_hip_batch_item* items, u32 k, u8* T_out, u64* keys_out,
                    u32* freqs_out);

}  // namespace bwtc_hip
