// The flash-attention dispatch as pure host code: which kernel family a call
// runs (plan_flash) and the 64-dword argument block of the generated v13 /
// pp64 programs (pack_v13).  Standard headers only, so the plan and the block
// are checked on the CPU (tests/test_flash_plan.py, tests/host/
// flash_plan_check.cpp: the route table, every variant, and the block word
// for word against tools/v13/run.py args_for, the mirror the emulator runs).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace pli {

// element strides of Q / K / V / O: batch, head, row
struct V7Strides {
    int64_t qb, qh, qn, kb, kh, kn, vb, vh, vn, ob, oh, on;
};

// attn_fwd_v13's kernel argument block, shared by the D = 128 bodies
// (flash_v13.hip), the D = 64 ones (flash_v13_d64.hip) and attn_fwd_pp64: 64
// dwords in the layout of tools/v13/kernel.py ARG_LAYOUT (the generated body
// reads it through the kernarg pointer).
struct V13Args {
    uint32_t w[64];
};
static_assert(sizeof(V13Args) == 256, "V13Args layout");
// (A_SHIFTS packs the three magic-division shifts and the head count:
// shq | shh << 5 | shg << 10 | H << 16 -- the block-parameter dwords 0..36
// then fit s56..s92 and the program keeps off s32 / s100 / s101)
enum : int {
    A_Q = 0, A_K = 2, A_V = 4, A_O = 6, A_QB = 8, A_QH = 10, A_KB = 12, A_KH = 14, A_VB = 16, A_VH = 18,
    A_OB = 20, A_OH = 22, A_QN = 24, A_ON, A_NQ, A_NT, A_QBLOCKS, A_NBLOCKS, A_MAGQ, A_MAGH, A_MAGG, A_SHIFTS,
    A_CW, A_HX, A_G, A_KN, A_VN, A_C, A_MUOFF, A_TBK, A_TBV, A_STAMP, A_STAMP_HI, A_OFFT
};
static_assert(A_G == 36 && A_OFFT == 45, "argument layout (tools/v13/kernel.py ARG_LAYOUT)");

// Kernel variants behind the same ABI (pli_flash_attn_fwd_variant, tuning /
// A-B runs; every one is parity-tested, the default at the full bench size):
//  21: attn_fwd_v2, 8 waves, permlane row max + defer-max (THR 8, log2) +
//      rounded-P row sum by v_dot2c (the round-1 default, kept as baseline)
//  50: attn_fwd_v7 (flash_v7.hip): Q prescaled by scale*log2(e) (bf16-rounded)
//      with -m as the first QK^T MFMA's C operand, speculative exp2, row sum
//      on the matrix core; register-staged K/V, one tile ahead
//  51: attn_fwd_v7 with exact scaling (p = exp2(fma(s, c, -m)))
//  54: attn_fwd_v10: v7's body, K/V by LDS-DMA two tiles ahead into a 3-deep
//      ring of XOR-swizzled images (D = 128; other head dims take v7), prescaled
//  55: attn_fwd_v10 with exact scaling (D = 128; D = 64 -> 51)
//  60: attn_fwd_v10 exact with 4-wave workgroups (128 rows), two per CU, a
//      2-slot ring one tile ahead (D = 128; D = 64 -> 51)
// The round-1 experiments (XOR-swizzled v1, staggered v3, pipelined v4/v5,
// 16x16x32 v6, ping-pong, segmented, one-wave-per-SIMD w4/w4p) and the
// round-2 ones that lost (in-wave pipelined v8, one-wave-per-SIMD v9, a
// two-barrier stagger with s_setprio, a half-tile lag on a 4-deep ring, the
// 4-wave one-wave-per-SIMD software-pipelined v11: 719-760 TF, static
// s_setprio 1 on waves 4-7: 1088 vs 1088 TF, the DMA pieces issued between
// the PV MFMAs: 1035 vs 1061 TF, two 64-key tiles per barrier on a 4-slot
// ring: 1054 vs 1054 TF, causal 850 vs 844) are
// not in the library; their measurements are in DESIGN.md 3.1.
//  70: attn_fwd_v12 (flash_v12.hip): 4 waves x 64 rows, one wave per SIMD,
//      O / Q / K fragments in literally named accumulator registers, a
//      hand-placed stream (one exp per MFMA gap), 5-slot LDS ring; bitwise
//      equal to 55 (bf16, D = 128, non-causal, Nk % 64 == 0; else 55)
//  71: attn_fwd_v12 persistent (one workgroup per CU walking its XCD's
//      blocks, the K/V stream and the next block's Q across block seams;
//      1181 vs 1082 TF/s for 55)
//  73 / 74: attn_fwd_v12 causal (bottom-right, Nq <= Nk), one block per
//      workgroup heaviest first / persistent with the pair walk
//  72: variant 71 with the defer-max threshold at 0 (a rescale whenever a
//      tile raises a row's max): tests only, the threshold sweep of
//      cdna_hip_programming.md rule 26 (72 and 71 agree to rounding)
//  80: attn_fwd_v13 (flash_v13.hip): 4 waves x 64 rows, one wave per SIMD,
//      v_mfma_f32_16x16x32_bf16 (the shape the chip clocks higher under load),
//      one generated instruction stream (tools/gen_flash_v13.py), persistent;
//      defer-max on P itself (D = 128 / 64, non-causal, Nk % 64 == 0 and Nk
//      >= 128, or any Nk > 64 on the ragged bodies attn_fwd_v13r / v13hr --
//      round 5; else 71); fp16 inputs run the same program on the f16 MFMA
//      (attn_fwd_v13h / v13hc, since round 5; before: 71 -> 55 / 60)
//  81: variant 80 with one block per workgroup
//  82: variant 80 with mu = max * c (P = 1 at the max, so every row's l >= 1
//      and the rare path runs at every tile): tests only
//  83 / 84: attn_fwd_v13c causal (bottom-right, Nq <= Nk; any diagonal
//      offset -- virtual rows -- and ragged Nk -- attn_fwd_v13rc -- since
//      round 5): 83 persistent (the pair walk where it tiles the grid), 84 one
//      block per workgroup heaviest first; 85 = 83 with mu = max * c
//  86: attn_fwd_pp64 / pp64h (causal: pp64c / pp64hc) where it applies
//      (head dim 64, bf16 / fp16, Nk % 64 == 0; causal with Nq and Nk - Nq
//      multiples of 64; tools/v14/pp64.py), else the default v13 form; 87: the
//      same with the rescale path at every tile (muoff 0 / -1, tests)
//  88: the default (kAuto, below)
enum FlashVariant : int {
    kV2 = 21,
    kV7Prescaled = 50, kV7 = 51, kV10Prescaled = 54, kV10 = 55, kV10FourWave = 60,
    kV12 = 70, kV12Persistent = 71, kV12Thr0 = 72, kV12Causal = 73, kV12CausalPersistent = 74,
    kV13 = 80, kV13OneBlock = 81, kV13Sweep = 82, kV13Causal = 83, kV13CausalOneBlock = 84, kV13CausalSweep = 85,
    kPP64 = 86, kPP64Sweep = 87, kAuto = 88
};
// default since round 4: attn_fwd_v13 (80), 1388 vs 1242 TF/s for v12 (71)
// at B8 S4096 H32 D128 in the same process (profiles/r04/flash/ab.log); where
// v13 does not apply (D not 64 / 128, Nk <= 64) it routes to 71 / 74.
// Since round 6 the default is 88: attn_fwd_pp64 / pp64h (86) for head dim 64
// non-causal where its blocks fill the chip (two waves per SIMD in ping-pong;
// bitwise v13's D = 64 result, 1259 vs 1104 TF/s at B8 H32 S4096 D64 in the
// same process, profiles/r06/pp64/), v13 (80) for everything else
constexpr int kDefaultVariant = kAuto;
// causal: attn_fwd_v12 causal (74; one block per workgroup where the
// persistent pair walk does not tile the shape), 60 where v12 does not apply
// (fp16, D != 128, Nq > Nk, Nk % 64): B8 S4096 H32 D128 bf16 1002 (74, the
// first rotation walk) vs 945 (60) TF/s, B2 S8192 1098 vs 1013, B32 S2048 867
// vs 830 (profiles/r03/flash/ab_causal.log); the pair walk: 1049 at B8 S4096,
// 1154 at B2 S8192, 1223 at B1 H64 S16384 (ab_causal_pair.log)
// causal default since round 4: attn_fwd_v13c (83), 1210 vs 1058 TF/s for
// 74 (profiles/r04/flash/ab_causal.log); since round 5 83 takes any diagonal
// offset, ragged Nk, fp16 and D 64 too; Nk <= 64 -> 74 where v12 applies (bf16,
// D 128, Nk = 64), else 60 (so also other D and Nq > Nk)
constexpr int kDefaultCausalVariant = kV13Causal;

// v13's mu = row max * c + PLI_V13_MUOFF (log2 units): P <= 2^-MUOFF right
// after a max is taken and a tile takes the rescale path once some row's sum l
// reaches 1 (since round 5; a row max grown by about MUOFF - log2 Nk -- the P
// >= 2 bit test of round 4 fired at MUOFF + 1).  62 (since round 4; was 7, the THR 8 of v10 /
// v12): P stays a normal bf16 / fp32 down to 2^-126, so only scores 64+ log2
// units under the row max flush to 0 (weight < 2^-64), and the rescale path
// all but vanishes where the scaled scores spread wide -- B8 H32 S4096, N(0,1)
// inputs, TF/s 7 -> 62: scale 1.0 590 -> 1368 (causal 452 -> 1172), 0.25
// 1150 -> 1386 (891 -> 1167), 1/sqrt(128) 1377 -> 1390 (1166 -> 1167)
// (profiles/r04/scale/ab_muoff.jsonl)
#ifndef PLI_V13_MUOFF
#define PLI_V13_MUOFF 62.f
#endif
// Range of V this offset supports (bf16 v13; the v12 / v7 / v10 bf16 bodies'
// threshold 64 mirrors it): P is about 2^-62 at a row's max, so P * V stays a
// normal fp32 down to |V| ~ 2^-64 and products below flush gradually
// (subnormal fp32 keeps 2^-149 absolute); on the other side P <= 1 (v13's
// clamp) and O <= l max|V|, so any finite bf16 V is safe.  Exercised at |V|
// scaled by 2^-60 and 2^50 against f64 (tests/test_gpu_flash_v13.py
// test_v13_v_range, variants 80 / 83 / 71 / 55).
// fp16 (attn_fwd_v13h / v13hc, since round 5): fp16 P is normal down to 2^-14
// and zero below 2^-24, so the offset stays small -- P <= 2^-4 when a max is
// taken, the rescale path once a row max grows by 5 (some P >= 2, the bit-14
// test), scores 20+ log2 units under the running estimate flush to 0 (weight
// < 2^-20 of the row's largest: at most Nk * 2^-20 of the sum in total)
//
// Round 6: that flush is what limits fp16 at long context.  On an
// attention-sink row (one dominant key, the rest d log2 units under it) the
// weights just above 2^-(24 - offset) are quantised to a few subnormal steps
// and those below it dropped, so the worst-case error grows with Nk * 2^offset:
// a numpy model of the packing gives, offset 4 / 3 / 2 / 1 (torch's fp16 SDPA
// in brackets), Nk 4096 2.9e-3 / 1.5e-3 / 7.5e-4 / 1.9e-4 (9.3e-4), 8192
// 9.6e-3 / 2.5e-3 / 1.5e-3 / 3.4e-4 (1.3e-3), 16384 1.1e-2 / 5.9e-3 / 3.2e-3 /
// 6.9e-4 (1.5e-3), 32768 2.6e-2 / 1.1e-2 / 5.6e-3 / 1.5e-3 (1.5e-3), 65536
// 4.6e-2 / 2.7e-2 / 1.1e-2 / 3.1e-3 (2.7e-3).  So the offset
// falls by one per doubling of Nk past 4096 (floor 1): the worst case stays
// at ~3e-3, within ~2x of torch's, and the bench's Nk 4096 keeps offset 4.
// A smaller offset takes the rescale path more often (B8 S4096: 4 / 2 / 0 at
// 1308 / 1138 / 662 TF/s; B1 S32768: 1393 / 1324 / 1035).
#ifndef PLI_V13_MUOFF_F16
#define PLI_V13_MUOFF_F16 4.f
#endif
inline float v13_muoff_f16(int Nk) {
    float m = PLI_V13_MUOFF_F16;
    for (int64_t n = 4096; n < Nk && m > 1.f; n *= 2) m -= 1.f;
    return m;
}

// attn_fwd_v12 (flash_v12.hip): bf16, D = 128, non-causal, Nk a multiple of 64
inline bool attn_v12_ok(int D, bool bf16, bool causal, int Nk) {
    return D == 128 && bf16 && !causal && Nk >= 64 && Nk % 64 == 0;
}

// attn_fwd_v13 (flash_v13.hip, flash_v13_d64.hip): bf16 and fp16 programs
inline bool attn_v13_ok(int D, bool causal, int Nq, int Nk, const V7Strides& st) {
    // head dim 128, or 64 (the D = 64 bodies in flash_v13_d64.hip); Nk a
    // multiple of 64 from 128, or (non-causal) any Nk > 64: the ragged bodies
    if ((D != 128 && D != 64) || Nq < 1) return false;
    if (Nk % 64 == 0 ? Nk < 128 : Nk <= 64) return false;
    // causal: Nq <= Nk, any diagonal offset -- rows are processed as Nq + s
    // virtual rows, s = (Nk - Nq) & 63, which puts the bottom-right diagonal
    // on 64-key tile boundaries (tools/v13/kernel.py qshift; rows below s are
    // neither loaded nor stored); Nk % 64 != 0 on the ragged causal bodies
    if (causal && Nq > Nk) return false;
    // causal: the stream's tile count and index carry the block's order in
    // bit 16 (tools/v13/kernel.py block_params), so counts stay below 2^16
    if (causal && (Nk + 63) / 64 > 0xFFFF) return false;
    // 32-bit per-lane offsets: a Q / O head's rows, a K / V tile
    const int64_t q_ext = ((int64_t)Nq - 1) * st.qn * 2 + 2 * D, o_ext = ((int64_t)Nq - 1) * st.on * 2 + 2 * D;
    const int64_t kv_tile = 64 * std::max(st.kn, st.vn) * 2;
    if (q_ext >= (1ll << 32) || o_ext >= (1ll << 32) || kv_tile >= (1ll << 31)) return false;
    for (int64_t s : {st.qb, st.qh, st.kb, st.kh, st.vb, st.vh, st.ob, st.oh, st.qn, st.kn, st.vn, st.on})
        if (s < 0) return false;
    return true;
}

// attn_fwd_pp64 (flash_pp64.hip; bf16 and fp16 bodies): D = 64, Nk % 64 == 0;
// causal: Nq % 64 == 0 and Nk - Nq a non-negative multiple of 64
inline bool attn_pp64_ok(int D, bool causal, int Nq, int Nk) {
    if (D != 64 || Nk % 64 != 0) return false;
    return !causal || (Nq % 64 == 0 && Nk >= Nq && (Nk - Nq) % 64 == 0);
}

// One call of pli_flash_attn_fwd, as the planner sees it.
struct FlashCall {
    int B, H, group, Nq, Nk, D;
    bool fp16, causal;  // fp16: else bf16
    V7Strides st;
    float scale;
    int cus;  // compute units of the stream's device
    // 16-bit operands at 16-byte-aligned addresses (the caller's check);
    // false (fp32, odd pointers): only the generic kernel reads them
    bool mfma_operands = true;
};

enum class FlashFamily { generic, v2, v7, v12, v13, pp64, unknown };

struct FlashPlan {
    FlashFamily family;
    int variant;      // the variant that ran, or fell out of the chain unknown
    int sub;          // v7: the body (launch_attn_v7: variant - 50)
    bool persistent;  // v12 / v13 / pp64: workgroups walk blocks (else one block each)
    float thr;        // v12: the defer-max threshold, 64 or 0
    float muoff;      // v13 / pp64: mu = row max * c + muoff
};

// The whole dispatch: each family applies where its *_ok rule holds, else the
// call falls to the next one: pp64 -> v13 -> v12 -> v7 / v10 -> v2; generic
// for what no MFMA kernel reads.  variant < 0: the default.
inline FlashPlan plan_flash(const FlashCall& f, int variant) {
    FlashPlan p{FlashFamily::generic, variant, 0, false, 64.f, 0.f};
    // n_kv == 0 (softmax over no keys) goes to the generic kernel, which
    // defines the output as zeros; the MFMA kernels' running max assumes a
    // positive scale (below)
    bool vec = f.mfma_operands && (f.D == 64 || f.D == 128) && f.Nk > 0 && f.scale > 0.f;
    const int64_t s[12] = {f.st.qb, f.st.qh, f.st.qn, f.st.kb, f.st.kh, f.st.kn,
                           f.st.vb, f.st.vh, f.st.vn, f.st.ob, f.st.oh, f.st.on};
    for (int i = 0; i < 12; ++i) vec = vec && s[i] % 8 == 0 && (i % 3 != 2 || s[i] >= f.D);
    if (!vec) return p;
    if (variant < 0) variant = f.causal ? kDefaultCausalVariant : kDefaultVariant;
    const bool bf = !f.fp16;
    // the MFMA bodies' defer-max sets m from the raw score max times c =
    // scale*log2(e): only for c > 0 is that the row's largest scaled score
    // (c <= 0 would make exp2(s*c - m) >= 1 and overflow); zero or negative
    // scales never get here (the generic kernel's max is of the scaled scores).
    // The prescaled variants 50 / 54 multiply Q by c in the 16-bit input type
    // (so c > 1 could overflow fp16 Q): they need c <= 1.  The exact bodies
    // (v12 70-74, v7 / v10 51 / 55 / 60) and the bf16 v13 / pp64 ones apply c
    // by fma to the fp32 scores: any c > 0.  The fp16 v13 bodies (v13h*, D 128
    // and 64) have prescaled Q by c in fp16 since round 6, yet take any c > 0
    // like the rest: their routing for c > 1 is the open ADVICE item.
    const float c_log2 = f.scale * 1.4426950408889634f;
    const bool c_ok = c_log2 > 0.f && c_log2 <= 1.f, c_pos = c_log2 > 0.f;
    const bool v13_ok = attn_v13_ok(f.D, f.causal, f.Nq, f.Nk, f.st) && c_pos && f.H < (1 << 16);
    // the rare-path sweep (82 / 85 / 87): bf16's l check trips at every tile with
    // mu = max * c (P = 1 at the max), fp16's P-bit check with mu = max * c - 1
    const float muoff = bf ? PLI_V13_MUOFF : v13_muoff_f16(f.Nk), sweep = bf ? 0.f : -1.f;
    // 88 (the default since round 6): 86 where its 512-row blocks fill the
    // chip (B H ceil(Nq / 512) >= the CU count), else 80 -- below that v13's
    // 256-row blocks spread the same work over twice as many CUs (B2 H8 S512:
    // 61 vs 85 TF/s on pp64, profiles/r06/pp64/)
    // (causal stays on v13c: pp64c -- the causal pp64 forms, one block per
    // workgroup heaviest first -- measured 725 vs 946 TF/s bf16, 802 vs 941
    // fp16 at B8 H32 S4096 D64, profiles/r06/pp64/ab9_causal_*.jsonl)
    if (variant == kAuto) {
        const bool fill = (int64_t)f.B * f.H * (((int64_t)f.Nq + 511) / 512) >= f.cus;
        variant = f.causal ? kV13Causal : fill ? kPP64 : kV13;
    }
    if (variant == kPP64 || variant == kPP64Sweep) {
        const bool sw = variant == kPP64Sweep;
        if (attn_pp64_ok(f.D, f.causal, f.Nq, f.Nk) && v13_ok)
            return {FlashFamily::pp64, variant, 0, true, 64.f, sw ? sweep : muoff};
        variant = f.causal ? (sw ? kV13CausalSweep : kV13Causal) : sw ? kV13Sweep : kV13;
    }
    if (variant >= kV13 && variant <= kV13CausalSweep) {
        const bool sw = variant == kV13Sweep || variant == kV13CausalSweep;
        if ((variant >= kV13Causal) == f.causal && v13_ok)
            return {FlashFamily::v13, variant, 0, variant != kV13OneBlock && variant != kV13CausalOneBlock, 64.f,
                    sw ? sweep : muoff};
        variant = f.causal ? kV12CausalPersistent : kV12Persistent;
    }
    if (variant == kV12 || variant == kV12Persistent || variant == kV12Thr0) {
        if (attn_v12_ok(f.D, bf, f.causal, f.Nk) && c_pos)
            return {FlashFamily::v12, variant, 0, variant != kV12, variant == kV12Thr0 ? 0.f : 64.f, 0.f};
        variant = f.causal ? kV10FourWave : kV10;
    }
    if (variant == kV12Causal || variant == kV12CausalPersistent) {
        if (f.causal && attn_v12_ok(f.D, bf, false, f.Nk) && f.Nq <= f.Nk && c_pos)
            return {FlashFamily::v12, variant, 0, variant == kV12CausalPersistent, 64.f, 0.f};
        variant = f.causal ? kV10FourWave : kV10;
    }
    if (variant == kV7Prescaled || variant == kV7 || variant == kV10Prescaled || variant == kV10 ||
        variant == kV10FourWave) {
        if (variant == kV7Prescaled || variant == kV10Prescaled ? c_ok : c_pos)
            return {FlashFamily::v7, variant, variant - kV7Prescaled, false, 64.f, 0.f};
        variant = kV2;
    }
    return {variant == kV2 ? FlashFamily::v2 : FlashFamily::unknown, variant, 0, false, 64.f, 0.f};
}

// The kernel a plan ends in, as pli_last_route names it ("" for an unknown
// variant); launch_attn_v13 checks its table entry against this.
struct FlashRoute {
    char name[32];
};
inline FlashRoute flash_route(const FlashCall& f, const FlashPlan& p) {
    static const char* const fixed[] = {"attn_fwd_generic", "attn_fwd_v2", "attn_fwd_v7", "attn_fwd_v12"};
    const char *h = f.fp16 ? "h" : "", *c = f.causal ? "c" : "", *r = f.Nk % 64 != 0 ? "r" : "";
    FlashRoute out{};
    if (p.family == FlashFamily::v13)
        std::snprintf(out.name, sizeof(out.name), "attn_fwd_v13%s%s%s%s", h, r, c, f.D == 64 ? "_d64" : "");
    else if (p.family == FlashFamily::pp64)
        std::snprintf(out.name, sizeof(out.name), "attn_fwd_pp64%s%s", h, c);
    else if (p.family != FlashFamily::unknown)
        std::snprintf(out.name, sizeof(out.name), "%s", fixed[(int)p.family]);
    return out;
}

// floor(x / d) == ((x * m) >> 31) >> l for 0 <= x < 2^31 (Granlund-Montgomery,
// N = 31: m = ceil(2^(31+l) / d) < 2^32 with l = ceil(log2 d))
inline void magic31(uint32_t d, uint32_t& m, uint32_t& l) {
    l = 0;
    while ((1ull << l) < d) ++l;
    const unsigned __int128 num = (unsigned __int128)1 << (31 + l);
    m = (uint32_t)((num + d - 1) / d);
}

// What launch_attn_v13 launches: the filled block, the grid, and the body
// (pp64 or v13, D, fp16, causal, ragged pick the kernel); error[0] != 0: the
// call is out of range, nothing to launch.
struct V13Launch {
    V13Args args;
    int grid;
    int D;
    bool pp64, fp16, causal, ragged;
    char error[96];
};

// The argument block of a v13 / pp64 plan (tools/v13/run.py args_for and
// tools/v14/pp64_run.py are its Python twins, the ones the emulator runs).
// stamps: the diagnostic build's clock buffer, else null.
inline V13Launch pack_v13(const FlashCall& f, const FlashPlan& p, const void* q, const void* k, const void* v,
                          void* o, uint32_t* stamps = nullptr) {
    const int Nq = f.Nq, Nk = f.Nk;
    const bool causal = f.causal, pp = p.family == FlashFamily::pp64;
    V13Launch L;
    std::memset(&L, 0, sizeof(L));
    L.D = f.D, L.pp64 = pp, L.fp16 = f.fp16, L.causal = causal, L.ragged = Nk % 64 != 0;
#define PLI_PLAN_REQUIRE(cond, ...)                             \
    if (!(cond)) {                                              \
        std::snprintf(L.error, sizeof(L.error), __VA_ARGS__);   \
        return L;                                               \
    }
    PLI_PLAN_REQUIRE(attn_v13_ok(f.D, causal, Nq, Nk, f.st) && (!pp || attn_pp64_ok(f.D, causal, Nq, Nk)),
                     "attn_fwd_v13: shape not supported");
    PLI_PLAN_REQUIRE(f.H > 0 && f.H < (1 << 16), "attn_fwd_v13: H = %d past the packed 16-bit head count", f.H);
    PLI_PLAN_REQUIRE(!((f.fp16 || f.D != 128 || L.ragged || causal || pp) && stamps),
                     "attn_fwd_v13: the stamp build is bf16, D = 128, non-causal, Nk %% 64 == 0");
    const int nqv = causal ? Nq + ((Nk - Nq) & 63) : Nq;  // causal: virtual rows, (Nk - nqv) % 64 == 0
    // attn_fwd_pp64: 512-row blocks (8 waves of 64 rows), one per workgroup
    const int rows = pp ? 512 : 256, qblocks = (nqv + rows - 1) / rows;
    const int64_t nb = (int64_t)f.B * f.H * qblocks;
    PLI_PLAN_REQUIRE(nb < (1ll << 31) && nb > 0, "attn_fwd_v13: grid too large");
    int grid = (int)nb;
    // (pp64's persistent walk streams the next block's first four key tiles
    // during the current block: it needs Nk >= 256)
    if (p.persistent && (!pp || (Nk / 64 >= 4 && !causal))) {
        const int g = f.cus / 8 * 8;
        if (g >= 8 && nb > g) grid = g;
    }
    // causal walk: the pair walk where it tiles the grid exactly (query
    // heights QB-1-a then a of one head per workgroup step, the QB/2
    // workgroups of a head in step on one XCD; G/8 and QB/2 powers of two),
    // else one block per workgroup, heaviest first
    uint32_t cw = 0, hx = 0;
    if (causal && pp) {
        cw = 2u;  // pp64c: block_params' remap walk, heaviest block first, one per workgroup
    } else if (causal) {
        const int64_t bh = nb / qblocks, w = grid / 8, hq = qblocks / 2;
        auto pw2 = [](int64_t x) { return x > 0 && (x & (x - 1)) == 0; };
        const bool pair = grid < nb && qblocks % 2 == 0 && hq > 0 && w % hq == 0 && bh % 8 == 0 &&
                          (bh / 8) % (w / hq) == 0 && nb % grid == 0 && (nb / grid) % 2 == 0 && pw2(w) && pw2(hq);
        if (pair) {
            uint32_t lg8 = 0, lghq = 0;
            while ((1ll << lg8) < w) ++lg8;
            while ((1ll << lghq) < hq) ++lghq;
            cw = 1u | (lg8 << 8) | (lghq << 16) | ((uint32_t)(w / hq) << 24);
            hx = (uint32_t)(bh / 8);
        } else {
            cw = 2u;
            grid = (int)nb;
        }
    }
    // ragged Nk: P0 = 64 - Nk % 64 in cw (non-causal: the walk word is free)
    // or in the top byte of hx (causal: the pair walk uses cw, hx < 2^24)
    const uint32_t p0 = L.ragged ? (uint32_t)(64 - Nk % 64) : 0u;
    PLI_PLAN_REQUIRE(hx < (1u << 24), "attn_fwd_v13: %u heads per XCD past the 24-bit walk field", hx);
#undef PLI_PLAN_REQUIRE
    uint32_t* w = L.args.w;
    auto put64 = [w](int at, uint64_t x) { w[at] = (uint32_t)x, w[at + 1] = (uint32_t)(x >> 32); };
    const V7Strides& st = f.st;
    put64(A_Q, (uint64_t)(uintptr_t)q);
    put64(A_K, (uint64_t)(uintptr_t)k);
    put64(A_V, (uint64_t)(uintptr_t)v);
    put64(A_O, (uint64_t)(uintptr_t)o);
    put64(A_QB, (uint64_t)st.qb * 2);
    put64(A_QH, (uint64_t)st.qh * 2);
    put64(A_KB, (uint64_t)st.kb * 2);
    put64(A_KH, (uint64_t)st.kh * 2);
    put64(A_VB, (uint64_t)st.vb * 2);
    put64(A_VH, (uint64_t)st.vh * 2);
    put64(A_OB, (uint64_t)st.ob * 2);
    put64(A_OH, (uint64_t)st.oh * 2);
    w[A_QN] = (uint32_t)(st.qn * 2);
    w[A_KN] = (uint32_t)(st.kn * 2);
    w[A_VN] = (uint32_t)(st.vn * 2);
    w[A_ON] = (uint32_t)(st.on * 2);
    w[A_NQ] = (uint32_t)Nq;
    w[A_NT] = (uint32_t)((Nk + 63) / 64);
    w[A_QBLOCKS] = (uint32_t)qblocks;
    w[A_NBLOCKS] = (uint32_t)nb;
    uint32_t shq, shh, shg;
    magic31((uint32_t)qblocks, w[A_MAGQ], shq);
    magic31((uint32_t)f.H, w[A_MAGH], shh);
    magic31((uint32_t)f.group, w[A_MAGG], shg);
    w[A_SHIFTS] = shq | (shh << 5) | (shg << 10) | ((uint32_t)f.H << 16);
    w[A_CW] = L.ragged && !causal ? p0 : cw;
    w[A_HX] = causal ? hx | (p0 << 24) : hx;
    w[A_OFFT] = causal ? (uint32_t)((Nk - nqv) / 64) : 0u;
    const float c = f.scale * 1.4426950408889634f;
    std::memcpy(&w[A_C], &c, 4);
    std::memcpy(&w[A_MUOFF], &p.muoff, 4);
    w[A_G] = (uint32_t)grid;
    w[A_TBK] = (uint32_t)(64 * st.kn * 2);
    w[A_TBV] = (uint32_t)(64 * st.vn * 2);
    put64(A_STAMP, (uint64_t)(uintptr_t)stamps);
    L.grid = grid;
    return L;
}

}  // namespace pli
