// The flash forward launchers behind the dispatch of flash_attn.hip; which one
// a call takes, and with what parameters, is plan_flash's answer
// (flash_plan.h).  D in {64, 128}, 16-bit operands, 16-byte aligned rows.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flash_plan.h"

namespace pli {

// Lean-softmax forward (flash_v7.hip); plan.sub selects a build of the body
// (A/B levers, see flash_v7.hip)
int launch_attn_v7(const FlashCall& call, const FlashPlan& plan, const void* q, const void* k, const void* v,
                   void* o, hipStream_t stream);
// attn_fwd_v12 (flash_v12.hip): one wave per SIMD, 64 rows per wave, O/Q/K in
// the accumulator file (attn_v12_ok).  plan.thr: the defer-max threshold (log2
// units); 64 and 0 are the built forms
int launch_attn_v12(const FlashCall& call, const FlashPlan& plan, const void* q, const void* k, const void* v,
                    void* o, hipStream_t stream);
// attn_fwd_v13 / attn_fwd_pp64 (flash_v13.hip, flash_v13_d64.hip,
// flash_pp64.hip): packs the plan's argument block (pack_v13) and launches the
// body it names; stamps: the diagnostic build's clock buffer
int launch_attn_v13(const FlashCall& call, const FlashPlan& plan, const void* q, const void* k, const void* v,
                    void* o, hipStream_t stream, uint32_t* stamps = nullptr);

}  // namespace pli
