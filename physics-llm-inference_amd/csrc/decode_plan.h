// The split-K plan of decode attention as pure host code: how a (batch, kv
// head) grid over n_kv keys is cut into chunks.  Standard headers only, so
// decode_attn.hip (contiguous cache), paged_attn.hip (paged pool) and the CPU
// checks (tests/host/paged_plan_check.cpp) share one copy of the rule.
#pragma once

#include <cstdint>

namespace pli {

constexpr int DEC_WAVES = 4;
constexpr int DEC_STEP = 32;                        // keys per wave step
constexpr int DEC_QUANT = DEC_WAVES * DEC_STEP;     // chunk granularity
constexpr int DEC_MAXM = 16;                        // query rows per kv head

// Chunking: enough workgroups to keep every CU's loads in flight (~4 per CU),
// at least one 32-key step per wave; chunk is a multiple of 4 waves x 32 keys.
struct DecPlan {
    int chunk, splits;
};
constexpr int64_t kDefaultTargetWgs = 1024;
// Short caches (<= kNoSplitKeys keys) with >= kNoSplitWgs (batch, kv head)
// pairs take one chunk per pair: the combine launch (~4.7 us) costs more than
// the serial key loop it saves (graph decode step, batch 32, 560-key cache:
// 1.279 -> 1.246 ms/token); with few pairs the split stays (batch 1: 8
// one-chunk workgroups ran 0.715 vs 0.681 ms/token).
constexpr int kNoSplitKeys = 1024, kNoSplitWgs = 128;
inline DecPlan plan_decode(int64_t bh, int n_kv, int64_t kTargetWgs = kDefaultTargetWgs) {
    // (int arithmetic, as the rule always ran: the quotients fit)
    auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
    const int64_t max_splits = cdiv(n_kv, DEC_QUANT);
    int64_t splits = bh >= kTargetWgs || (n_kv <= kNoSplitKeys && bh >= kNoSplitWgs)
                         ? 1
                         : cdiv((int)kTargetWgs, (int)bh);
    splits = splits < 1 ? 1 : (splits > max_splits ? max_splits : splits);
    const int chunk = (int)(cdiv(cdiv(n_kv, (int)splits), DEC_QUANT) * DEC_QUANT);
    return {chunk, (int)cdiv(n_kv, chunk)};
}

}  // namespace pli
