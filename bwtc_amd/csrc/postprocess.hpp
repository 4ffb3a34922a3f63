// GPU postprocessor of `--prepr` blocks (postprocess.hip).  The workspace is the postprocessor's own, made by the
// first call and grown when a later block needs more; bwtc_hip_create's arena is left as it is.
#pragma once
#include "common.hpp"
#include "bwtc_hip.h"
#include "prepr_host.hpp"

namespace bwtc_hip {

struct BwtEngine;
struct PostProcessor;

PostProcessor* postprocessor_create();
void postprocessor_destroy(PostProcessor* p);
int postprocessor_stats(PostProcessor* p, bwtc_hip_postprocess_stats* out);

// d_data (n bytes, device) expanded into d_out (cap bytes, device; must not overlap): 0 and *n_out, -1 when the
// output does not fit (nothing has been written to d_out then), -2 / -3
int postprocess_device(BwtEngine& e, PostProcessor& p, const bwtc::prepr::Grammar& g, const u8* d_data, u64 n, u8* d_out, u64 cap,
                       u64* n_out);
// the same with host buffers: data goes up, the expansion comes down once
int postprocess_block(BwtEngine& e, PostProcessor& p, const bwtc::prepr::Grammar& g, const u8* data, u64 n, u8* out, u64 cap,
                      u64* n_out);

}  // namespace bwtc_hip
