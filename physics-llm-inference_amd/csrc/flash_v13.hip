// attn_fwd_v13: flash-attention forward on v_mfma_f32_16x16x32_bf16
// (reference ch06/flash_attention.py:14-74; gfx950, bf16 / fp16, D = 128 /
// 64, Nk a multiple of 64 and >= 128 or -- attn_fwd_v13r -- any Nk > 64;
// causal -- bottom-right, any Nq <= Nk -- as attn_fwd_v13c / v13rc; other
// cases take v12 / v10).
//
// One wave per SIMD, 64 query rows per wave (4 q-blocks of 16), persistent
// workgroups of 4 waves walking 256-row blocks.  The body is ONE generated
// instruction stream (flash_v13_asm.h from tools/gen_flash_v13.py; the
// layout, schedule and the reasons for them are in tools/v13/kernel.py): the
// 16x16x32 MFMA shape holds a higher clock under load than 32x32x16 (DESIGN
// 3.1), but its 16-cycle gaps leave 8 issue cycles each, so the softmax
// stream, the fragment reads and the LDS-DMA are placed gap by gap, with the
// hazard padding and wait counts computed by the generator (hipcc pads
// nothing inside an asm statement).  tests/test_v13_emu.py runs the same
// program in a CPU emulator; tests/test_gpu_flash_v13.py on the device.
//
// Differences from v12 a caller can see: none in the contract; numerically
// P = bf16(exp2(s c - mu)) with mu = (row max) c + muoff (62 from the
// planner: P <= 2^-62 when the max is taken, checked < 2 per tile, so a row
// max may grow by 63 log2 units before the rescale path -- v12's THR 64
// rule), l from the same rounded P on the matrix core, 1/l by v_rcp.
#include "flash_v7.h"
#ifdef PLI_V13_AB_HEADER  // timing-only A/B builds (tools/build_v13_ab.sh)
#include PLI_V13_AB_HEADER
#else
#include "flash_v13_asm.h"
#endif
#include "pli_common.h"
#include "flash_v13.h"

namespace pli {
namespace {

#define PLI_V13_KERNEL(name, body)                                                                       \
    __global__ __launch_bounds__(256, 1) void name(V13Args args) {                                      \
        __shared__ __attribute__((aligned(1024))) char smem[163840];                                    \
        (void)args;                                                                                     \
        const void* kp = (const void*)__builtin_amdgcn_kernarg_segment_ptr();                           \
        const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                         \
        const unsigned wg = blockIdx.x;                                                                 \
        asm volatile(body::"s"(kp), "s"(wg), "s"(wave), "s"((unsigned)(uintptr_t)smem) : PLI_V13_CLOBBERS); \
    }

PLI_V13_KERNEL(attn_fwd_v13, PLI_V13_BODY)
// causal (bottom-right mask): the same program with the masked step bodies
// and the causal walks (tools/v13/kernel.py Gen(causal=True))
PLI_V13_KERNEL(attn_fwd_v13c, PLI_V13C_BODY)
// fp16 Q / K / V / O: the same programs on v_mfma_f32_16x16x32_f16, P packed
// to fp16 (RNE) and checked with the bit-14 test (tools/v13/kernel.py
// Gen(dtype="f16"); the planner passes mu offset v13_muoff_f16)
PLI_V13_KERNEL(attn_fwd_v13h, PLI_V13H_BODY)
PLI_V13_KERNEL(attn_fwd_v13hc, PLI_V13HC_BODY)
// Nk % 64 != 0 (non-causal): the last key tile is streamed from key Nk - 64,
// inside the head, and the keys it shares with the tile before get P = 0
// (tools/v13/kernel.py RAGGED; P0 = 64 - Nk % 64 in the cw argument)
PLI_V13_KERNEL(attn_fwd_v13r, PLI_V13R_BODY)
PLI_V13_KERNEL(attn_fwd_v13hr, PLI_V13HR_BODY)
// causal with Nk % 64 != 0: the shifted last key tile, masked by VALU on its
// shifted keys (tools/v13/kernel.py rag step; P0 in the top byte of hx)
PLI_V13_KERNEL(attn_fwd_v13rc, PLI_V13RC_BODY)
PLI_V13_KERNEL(attn_fwd_v13hrc, PLI_V13HRC_BODY)

#ifdef PLI_FLASH_STAMPS
// diagnostic build only (tools/build_diag.sh): the same program with
// s_memtime / s_memrealtime at each wave's entry and exit (8 dwords per wave
// at args.stamp + 128 * (workgroup * 4 + wave); lanes 15-21: the seam sums of
// tools/v13/kernel.py Gen.seam_stamp)
#include "flash_v13_stamp_asm.h"
int g_diag_grid = 0;  // pli_diag_v13_set_grid: persistent grid override (0: the CU count)
PLI_V13_KERNEL(attn_fwd_v13_stamp, PLI_V13_STAMP_BODY)
#endif

}  // namespace

V13Entry v13_d128_entry(bool fp16, bool causal, bool ragged) {
    static const V13Entry table[2][2][2] = {  // [ragged][causal][fp16]
        {{PLI_V13_ENTRY(attn_fwd_v13), PLI_V13_ENTRY(attn_fwd_v13h)},
         {PLI_V13_ENTRY(attn_fwd_v13c), PLI_V13_ENTRY(attn_fwd_v13hc)}},
        {{PLI_V13_ENTRY(attn_fwd_v13r), PLI_V13_ENTRY(attn_fwd_v13hr)},
         {PLI_V13_ENTRY(attn_fwd_v13rc), PLI_V13_ENTRY(attn_fwd_v13hrc)}}};
    return table[ragged][causal][fp16];
}

int launch_v13_body(const V13Entry& entry, unsigned grid, unsigned block, const V13Args& args, hipStream_t stream) {
    hipLaunchKernelGGL(entry.kernel, dim3(grid), dim3(block), 0, stream, args);
    return launch_status(entry.route);
}

int launch_attn_v13(const FlashCall& call, const FlashPlan& plan, const void* q, const void* k, const void* v,
                    void* o, hipStream_t stream, uint32_t* stamps) {
#ifndef PLI_FLASH_STAMPS
    stamps = nullptr;
#endif
    V13Launch L = pack_v13(call, plan, q, k, v, o, stamps);
    PLI_REQUIRE(!L.error[0], "%s", L.error);
#ifdef PLI_FLASH_STAMPS
    if (stamps) {
        // diagnostic: a smaller persistent grid (a multiple of 8) when asked
        if (g_diag_grid >= 8 && g_diag_grid % 8 == 0 && g_diag_grid < L.grid) L.args.w[A_G] = L.grid = g_diag_grid;
        return launch_v13_body(PLI_V13_ENTRY(attn_fwd_v13_stamp), L.grid, 256, L.args, stream);
    }
#endif
    const auto entry = L.pp64 ? pp64_entry : L.D == 64 ? v13_d64_entry : v13_d128_entry;
    const V13Entry e = entry(L.fp16, L.causal, L.ragged);
    PLI_REQUIRE(e.route && !strcmp(flash_route(call, plan).name, e.route),
                "attn_fwd_v13: no body for this plan");
    return launch_v13_body(e, L.grid, L.pp64 ? 512 : 256, L.args, stream);
}

}  // namespace pli

#ifdef PLI_FLASH_STAMPS
// Diagnostic entry (tools/libpli_diag.so only): one clock-stamped launch of
// attn_fwd_v13 (persistent) on contiguous [B,H,N,128] bf16; stamps: 8 dwords
// per wave (entry s_memtime lo/hi, s_memrealtime lo/hi, then the exit ones)
extern "C" int pli_diag_v13_clock(const void* q, const void* k, const void* v, void* o, int B, int H, int N,
                                  uint32_t* stamps) {
    using namespace pli;
    const int64_t sn = 128, sh = (int64_t)N * 128, sb = (int64_t)H * N * 128;
    const V7Strides st{sb, sh, sn, sb, sh, sn, sb, sh, sn, sb, sh, sn};
    FlashCall call{B, H, 1, N, N, 128, false, false, st, 1.f / sqrtf(128.f), cu_count(0)};
    const FlashPlan plan{FlashFamily::v13, kV13, 0, true, 64.f, 62.f};
    const int rc = launch_attn_v13(call, plan, q, k, v, o, 0, stamps);
    if (rc != 0 || hipDeviceSynchronize() != hipSuccess) return -1;
    return 0;
}
// the stamped launches' persistent grid (a multiple of 8 below the CU count;
// 0 = the product's): the seam's cost against how many CUs seam together
extern "C" void pli_diag_v13_set_grid(int grid) { pli::g_diag_grid = grid; }
#endif
