// attn_decode_paged_combine (paged_attn.hip) for the other sources that write
// its split-K partials: the kernel lives in that file's unnamed namespace, this
// launcher is the way in.  Internal to the library (hidden visibility).
#pragma once

#include "pli_common.h"

namespace pli {

// Enqueue the merge of `splits` fp32 partials per (batch, kv head, row):
// part_o [bh, splits, M, D] and part_ml (m, l) [bh, splits, M] as
// attn_decode_paged writes them, o with element strides {o_b, o_h, o_n}.
// dtype PLI_BF16 / PLI_F16, head_dim 64 / 128.  Nothing is checked here.
void launch_paged_combine(int dtype, int head_dim, const float* part_o, const void* part_ml, void* o, int batch,
                          int kv_heads, int group, int rows, int64_t o_b, int64_t o_h, int64_t o_n, int splits,
                          hipStream_t stream);

}  // namespace pli
