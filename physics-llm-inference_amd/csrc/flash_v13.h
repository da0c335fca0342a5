// The generated v13 / pp64 bodies as launch_attn_v13 (flash_v13.hip) sees
// them: each file maps (fp16, causal, ragged -- Nk % 64 != 0) to one kernel
// over the shared argument block V13Args (flash_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include "flash_plan.h"

namespace pli {

struct V13Entry {
    void (*kernel)(V13Args);
    const char* route;  // the kernel's name, as pli_last_route reports it
};
#define PLI_V13_ENTRY(kernel) V13Entry{kernel, #kernel}

V13Entry v13_d128_entry(bool fp16, bool causal, bool ragged);  // flash_v13.hip: workgroups of 256 threads
V13Entry v13_d64_entry(bool fp16, bool causal, bool ragged);   // flash_v13_d64.hip: 256 threads
// flash_pp64.hip: head dim 64, Nk % 64 == 0 (never ragged; causal: Nq and
// Nk - Nq too), the arguments with 512-row blocks, workgroups of 512 threads
V13Entry pp64_entry(bool fp16, bool causal, bool ragged);

// launch `entry` on `grid` workgroups of `block` threads; returns the launch status
int launch_v13_body(const V13Entry& entry, unsigned grid, unsigned block, const V13Args& args, hipStream_t stream);

}  // namespace pli
