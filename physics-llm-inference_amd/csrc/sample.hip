// Next-token sampling on the device (pli_sample): temperature, top-k, top-p and
// the draw of ch02/generation.py:23-31, ch02/cached_generation.py:245,265 and
// ch10/engine.py:96-115 as one graph-capturable launch, one workgroup per row.
//
// The rule is DESIGN.md's "Sampling" section; csrc/sample_plan.h holds every
// piece of it a host can replay (Philox, keys, digits, fixed-point weights, the
// wave -> segment map).  Shape of the kernel (sample_select):
//
//   A  max key of the row (integer max: exact).  No logit above -inf: token -1.
//   B  top-k: radix select of the k-th key, 8 bits a pass from the top (2
//      passes for the 16-bit types, 4 for fp32), counts in an LDS histogram.
//      Gives the cut key T1 and how many of the tokens tied at T1 are kept
//      (the lowest indices).  Skipped when top-k keeps the row.
//   C  S1 = sum of the kept weights (only when top_p < 1).
//   D  top-p: the same radix select over weights: the smallest key whose
//      tokens still start at a prefix weight <= top_p * S1, and from the
//      prefix weight left how many of its tied tokens are kept.
//   E  per-wave sums of the kept weights; S2; the wave that holds the draw;
//      that wave re-cuts its segment into one contiguous run per lane, two
//      wave scans (tie counts, weights) find the lane, the lane walks its run.
//
// A weight is floor(exp((x - m) / temperature) * 2^45) as a 64-bit integer, so
// every sum above is an integer sum: exact, independent of the order of the
// (integer) LDS atomics and of the reduction shape.  No floating-point atomic
// and no floating-point sum feeds a decision.  Greedy (temperature == 0) is a
// one-pass kernel of its own (sample_greedy): max of (key, ~index).
//
// The row is walked from global memory / L2 in every pass (no LDS copy), so
// there is no LDS-resident limit; wave w owns the contiguous segment
// [w * seg, (w + 1) * seg) and takes 64 consecutive elements a step, eight
// steps' loads in flight at a time; "lower index first" is "lower wave first".
#include "pli_common.h"
#include "sample_plan.h"

namespace pli {
namespace {

template <typename T> struct sample_elem;
template <> struct sample_elem<float> {
    static constexpr int dtype = PLI_F32;
    __device__ __forceinline__ static uint32_t bits(const void* row, int i) {
        return reinterpret_cast<const uint32_t*>(row)[i];
    }
    __device__ __forceinline__ static float value(uint32_t key) { return __uint_as_float(sample_unkey_f32(key)); }
};
template <> struct sample_elem<f16_t> {
    static constexpr int dtype = PLI_F16;
    __device__ __forceinline__ static uint32_t bits(const void* row, int i) {
        return reinterpret_cast<const uint16_t*>(row)[i];
    }
    __device__ __forceinline__ static float value(uint32_t key) {
        return (float)__builtin_bit_cast(_Float16, (uint16_t)sample_unkey_16(key));
    }
};
template <> struct sample_elem<bf16_t> {
    static constexpr int dtype = PLI_BF16;
    __device__ __forceinline__ static uint32_t bits(const void* row, int i) {
        return reinterpret_cast<const uint16_t*>(row)[i];
    }
    __device__ __forceinline__ static float value(uint32_t key) { return __uint_as_float(sample_unkey_16(key) << 16); }
};

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ u64 wave_max_u64(u64 x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

struct SampleShared {
    u64 hist[256];
    u64 wave_w[kSampleWaves];
    uint32_t wave_eq[kSampleWaves];
    uint32_t wave_key[kSampleWaves];
    u64 sel_excl;
    uint32_t sel_digit;
    float u;
};

// what every pass needs of the row
template <typename T> struct SampleRow {
    const void* p;
    int vocab, seg, steps, wave, lane;
    uint32_t maxkey;
    float m, temperature;
    bool pos_inf;  // the row holds +inf: weight 1 for +inf, 0 for the rest

    __device__ __forceinline__ int index(int step) const { return sample_index(wave, step, lane, seg); }
    __device__ __forceinline__ uint32_t key(int i) const {
        return sample_key(sample_elem<T>::bits(p, i), sample_elem<T>::dtype);
    }
    // the keys of steps step0 .. step0 + kBatch - 1, loaded together so that kBatch loads per lane are in flight (one
    // workgroup walks the row: its passes are bound by load latency); 0, below every key, where there is no element
    static constexpr int kBatch = 8;
    __device__ __forceinline__ void keys(int step0, uint32_t (&k)[kBatch]) const {
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int i = index(step0 + j);
            k[j] = (step0 + j < steps && i < vocab) ? key(i) : 0u;
        }
    }
    __device__ __forceinline__ u64 weight(uint32_t key) const {
        if (pos_inf) return key == maxkey ? kSampleOne : 0;
        return sample_weight_fx(sample_elem<T>::value(key), m, temperature);
    }
};

// Radix select from the most significant digit.  Token i carries the value
// v_i (WEIGHTS: its weight if key_i > t1, else nothing; counts: 1); tie_add is
// added to the bucket of t1 itself.  Finds the largest key t with
// sum{v_i : key_i >= t} > q (walking each digit's buckets from the top, the
// first bucket whose inclusive sum exceeds what is left of q) and returns what
// is left of q below it: q - sum{v_i : key_i > t}.
template <typename T, bool WEIGHTS>
__device__ void radix_select(SampleShared& sh, const SampleRow<T>& r, u64 q, uint32_t t1, u64 tie_add, uint32_t& t_out,
                             u64& q_out) {
    constexpr int dt = sample_elem<T>::dtype;
    const int tid = r.wave * 64 + r.lane;
    uint32_t prefix = 0;
    for (int pass = 0; pass < sample_digit_passes(dt); ++pass) {
        if (tid < 256) sh.hist[tid] = 0;
        __syncthreads();
        for (int step0 = 0; step0 < r.steps; step0 += SampleRow<T>::kBatch) {
            uint32_t keys[SampleRow<T>::kBatch];
            r.keys(step0, keys);
#pragma unroll
            for (int j = 0; j < SampleRow<T>::kBatch; ++j) {
                if (step0 + j >= r.steps) break;
                const uint32_t key = keys[j];
                bool match = key != 0u && sample_prefix(key, pass, dt) == prefix;
                if (WEIGHTS) match = match && key > t1;
                const u64 v = !match ? 0 : WEIGHTS ? r.weight(key) : 1;
                const uint32_t digit = sample_digit(key, pass, dt);
                const u64 mm = __ballot(match);
                if (mm) {  // (wave-uniform) the lanes on the first matching lane's digit go in as one add
                    const int leader = __ffsll((long long)mm) - 1;
                    const uint32_t lead_digit = __shfl(digit, leader, 64);
                    const bool same = match && digit == lead_digit;
                    const u64 s = WEIGHTS ? wave_sum_u64(same ? v : 0) : (u64)__popcll(__ballot(same));
                    if (r.lane == leader)
                        atomicAdd(&sh.hist[lead_digit], s);
                    else if (match && !same)
                        atomicAdd(&sh.hist[digit], v);
                }
            }
        }
        __syncthreads();
        if (tid == 0 && tie_add && sample_prefix(t1, pass, dt) == prefix) sh.hist[sample_digit(t1, pass, dt)] += tie_add;
        __syncthreads();
        if (r.wave == 0) {  // lane l holds buckets 255 - 4l .. 252 - 4l, the top ones first
            u64 h[4], loc = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h[j] = sh.hist[255 - 4 * r.lane - j];
                loc += h[j];
            }
            const u64 incl = wave_incl_scan_u64(loc, r.lane);
            u64 run = incl - loc, ex = 0;
            int hit = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (hit < 0) {
                    if (run + h[j] > q) {
                        hit = j;
                        ex = run;
                    } else {
                        run += h[j];
                    }
                }
            }
            const u64 hm = __ballot(hit >= 0);
            if (hm) {
                if (r.lane == __ffsll((long long)hm) - 1) {
                    sh.sel_digit = 255 - 4 * r.lane - hit;
                    sh.sel_excl = ex;
                }
            } else if (r.lane == 63) {  // nothing exceeds q: everything is kept, the cut is the lowest bucket
                sh.sel_digit = 0;
                sh.sel_excl = incl - h[3];
            }
        }
        __syncthreads();
        prefix = (prefix << kSampleDigitBits) | sh.sel_digit;
        q -= sh.sel_excl;
    }
    t_out = prefix;
    q_out = q;
}

// per wave: sum of the weights of its tokens with key > t, and how many of its tokens have key == t
template <typename T> __device__ void wave_sums(SampleShared& sh, const SampleRow<T>& r, uint32_t t) {
    __syncthreads();  // (the previous readers of wave_w / wave_eq are done)
    u64 acc = 0;
    uint32_t eq = 0;
#pragma unroll 8
    for (int step = 0; step < r.steps; ++step) {
        const int i = r.index(step);
        if (i < r.vocab) {
            const uint32_t key = r.key(i);
            if (key > t) acc += r.weight(key);
            eq += key == t;
        }
    }
    acc = wave_sum_u64(acc);
    eq = (uint32_t)wave_sum_u64(eq);
    if (r.lane == 0) {
        sh.wave_w[r.wave] = acc;
        sh.wave_eq[r.wave] = eq;
    }
    __syncthreads();
}

constexpr long long kSampleAll = 1ll << 40;  // "every tied token": above any count

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void sample_select_kernel(
    const void* __restrict__ logits, int64_t ld, int vocab, float temperature, int top_k, float top_p,
    const float* __restrict__ uniforms, uint64_t seed, const int32_t* __restrict__ offset_dev, int64_t offset_add,
    int64_t* __restrict__ tokens, int64_t ld_tokens) {
    constexpr int dt = sample_elem<T>::dtype;
    __shared__ SampleShared sh;
    const int row = blockIdx.x;
    SampleRow<T> r;
    r.p = reinterpret_cast<const char*>(logits) + (int64_t)row * ld * elem<T>::bytes;
    r.vocab = vocab;
    r.seg = sample_seg_len(vocab);
    r.steps = r.seg / 64;
    r.wave = threadIdx.x >> 6;
    r.lane = threadIdx.x & 63;
    r.temperature = temperature;

    // A: the row maximum
    uint32_t mk = 0;
#pragma unroll 8
    for (int step = 0; step < r.steps; ++step) {
        const int i = r.index(step);
        if (i < vocab) mk = max(mk, r.key(i));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mk = max(mk, (uint32_t)__shfl_xor(mk, o, 64));
    if (r.lane == 0) sh.wave_key[r.wave] = mk;
    if (threadIdx.x == 0)
        sh.u = uniforms ? uniforms[row]
                        : sample_philox_u(seed, (offset_dev ? (int64_t)*offset_dev : 0) + offset_add, (uint32_t)row);
    __syncthreads();
    mk = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) mk = max(mk, sh.wave_key[w]);
    if (mk == sample_key_neg_inf(dt)) {  // (the whole workgroup) no logit above -inf
        if (threadIdx.x == 0) tokens[(int64_t)row * ld_tokens] = -1;
        return;
    }
    r.maxkey = mk;
    r.pos_inf = mk == sample_key_pos_inf(dt);
    r.m = sample_elem<T>::value(mk);
    const float u = sh.u;

    // B: top-k.  K1 = {key > t1} and the first need1 (by index) of {key == t1}
    const bool keep_all = top_k <= 0 || top_k >= vocab;
    uint32_t t1 = 0;  // (below every key)
    long long need1 = kSampleAll;
    if (!keep_all) {
        u64 left;
        radix_select<T, false>(sh, r, (u64)(top_k - 1), 0u, 0, t1, left);
        need1 = (long long)left + 1;
    }

    // C, D: top-p.  K2 = {key > tc} and the first n_eq of {key == tc}
    uint32_t tc = t1;
    long long n_eq = need1;
    if (top_p < 1.0f) {
        wave_sums(sh, r, t1);
        const u64 tie_add = keep_all ? 0 : (u64)need1 * r.weight(t1);
        u64 s1 = tie_add;
#pragma unroll
        for (int w = 0; w < kSampleWaves; ++w) s1 += sh.wave_w[w];
        u64 left;
        radix_select<T, true>(sh, r, sample_scale_fx(top_p, s1), t1, tie_add, tc, left);
        // token number j (from 0) of the ties at tc starts at prefix weight G + j * wc: kept iff j * wc <= P - G = left
        const u64 wc = r.weight(tc);
        const long long n_p = wc == 0 ? kSampleAll : (long long)(left / wc) + 1;
        const long long lim = (!keep_all && tc == t1) ? need1 : kSampleAll;
        n_eq = n_p < lim ? n_p : lim;
    }

    // E: S2, the wave of the draw, the draw
    wave_sums(sh, r, tc);
    const u64 wc = r.weight(tc);
    u64 s2 = 0;
    long long eq_before = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) {
        const long long eqw = sh.wave_eq[w], room = n_eq - eq_before;
        s2 += sh.wave_w[w] + (u64)(room <= 0 ? 0 : room < eqw ? room : eqw) * wc;
        eq_before += eqw;
    }
    const u64 target = sample_scale_fx(u, s2);  // < s2: some running sum exceeds it
    u64 carry = 0;
    long long eq_run = 0;
    int wstar = kSampleWaves - 1;
    for (int w = 0; w < kSampleWaves; ++w) {
        const long long eqw = sh.wave_eq[w], room = n_eq - eq_run;
        const u64 tot = sh.wave_w[w] + (u64)(room <= 0 ? 0 : room < eqw ? room : eqw) * wc;
        if (carry + tot > target) {
            wstar = w;
            break;
        }
        carry += tot;
        eq_run += eqw;
    }
    if (r.wave != wstar) return;
    // the wave of the draw re-cuts its segment so that lane l holds the r.steps consecutive elements from
    // wstar * seg + l * r.steps (index order = lane order, then the lane's own order): two wave scans find the
    // lane, and that lane walks its elements
    const int first = sample_index(wstar, 0, 0, r.seg) + r.lane * r.steps;
    u64 gt = 0;
    uint32_t eqc = 0;
#pragma unroll 8
    for (int e = 0; e < r.steps; ++e) {
        if (first + e < vocab) {
            const uint32_t key = r.key(first + e);
            if (key > tc) gt += r.weight(key);
            eqc += key == tc;
        }
    }
    const long long eq_lane = eq_run + (long long)(wave_incl_scan_u64(eqc, r.lane) - eqc);  // ties before this lane
    const long long room = n_eq - eq_lane;
    const u64 tot = gt + (u64)(room <= 0 ? 0 : room < (long long)eqc ? room : (long long)eqc) * wc;
    const u64 incl = wave_incl_scan_u64(tot, r.lane);
    const u64 hm = __ballot(carry + incl > target);
    if (hm == 0 || r.lane != __ffsll((long long)hm) - 1) return;
    u64 run = carry + incl - tot;
    long long rank = eq_lane;
    for (int e = 0; e < r.steps; ++e) {
        if (first + e >= vocab) break;
        const uint32_t key = r.key(first + e);
        if (key > tc) {
            run += r.weight(key);
        } else if (key == tc) {
            if (rank < n_eq) run += wc;
            ++rank;
        }
        if (run > target) {
            tokens[(int64_t)row * ld_tokens] = first + e;
            return;
        }
    }
}

// temperature == 0: the first token in the order = max of (key, ~index)
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void sample_greedy_kernel(const void* __restrict__ logits, int64_t ld,
                                                                       int vocab, int64_t* __restrict__ tokens,
                                                                       int64_t ld_tokens) {
    constexpr int dt = sample_elem<T>::dtype;
    __shared__ u64 red[kSampleWaves];
    const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const void* p = reinterpret_cast<const char*>(logits) + (int64_t)row * ld * elem<T>::bytes;
    const int seg = sample_seg_len(vocab), steps = seg / 64;
    u64 best = 0;
#pragma unroll 8
    for (int step = 0; step < steps; ++step) {
        const int i = sample_index(wave, step, lane, seg);
        if (i < vocab) {
            const u64 cand = ((u64)sample_key(sample_elem<T>::bits(p, i), dt) << 32) | (uint32_t)~(uint32_t)i;
            best = cand > best ? cand : best;
        }
    }
    best = wave_max_u64(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kSampleWaves; ++w) best = red[w] > best ? red[w] : best;
        tokens[(int64_t)row * ld_tokens] =
            (uint32_t)(best >> 32) == sample_key_neg_inf(dt) ? (int64_t)-1 : (int64_t)(~(uint32_t)best);
    }
}

template <typename T>
int launch_sample(const void* logits, int64_t ld, int rows, int vocab, float temperature, int top_k, float top_p,
                  const float* uniforms, uint64_t seed, const int32_t* offset_dev, int64_t offset_add, int64_t* tokens,
                  int64_t ld_tokens, hipStream_t s) {
    const dim3 grid((unsigned)rows), block(kSampleThreads);
    if (temperature == 0.0f) {
        hipLaunchKernelGGL(sample_greedy_kernel<T>, grid, block, 0, s, logits, ld, vocab, tokens, ld_tokens);
        return launch_status("sample_greedy");
    }
    hipLaunchKernelGGL(sample_select_kernel<T>, grid, block, 0, s, logits, ld, vocab, temperature, top_k, top_p,
                       uniforms, seed, offset_dev, offset_add, tokens, ld_tokens);
    return launch_status("sample_select");
}

}  // namespace
}  // namespace pli

extern "C" size_t pli_sample_workspace_size(int rows, int vocab, int dtype) {
    (void)rows, (void)vocab, (void)dtype;
    return 0;  // the kernels keep their state in LDS
}

extern "C" int pli_sample(const void* logits, int64_t ld_logits, int rows, int vocab, int dtype, float temperature,
                          int top_k, float top_p, const float* uniforms, uint64_t seed, const int32_t* offset_dev,
                          int64_t offset_add, int64_t* tokens, int64_t ld_tokens, void* workspace,
                          size_t workspace_bytes, void* stream) {
    using namespace pli;
    clear_error();
    PLI_REQUIRE(rows >= 0 && vocab >= 1 && ld_logits >= vocab && ld_tokens >= 1,
                "pli_sample: bad shape rows=%d vocab=%d ld_logits=%lld ld_tokens=%lld", rows, vocab,
                (long long)ld_logits, (long long)ld_tokens);
    PLI_REQUIRE(dtype == PLI_F32 || dtype == PLI_F16 || dtype == PLI_BF16, "pli_sample: bad dtype %d", dtype);
    PLI_REQUIRE(temperature >= 0.0f && top_p >= 0.0f,
                "pli_sample: temperature and top_p must be >= 0 and not NaN (temperature=%g top_p=%g)",
                (double)temperature, (double)top_p);
    PLI_REQUIRE(workspace_bytes >= pli_sample_workspace_size(rows, vocab, dtype) &&
                    (workspace == nullptr || aligned16(workspace)),
                "pli_sample: workspace too small or not 16-byte aligned");
    if (vocab > kSampleMaxVocab) {
        set_error("pli_sample: vocab=%d above the supported %d", vocab, kSampleMaxVocab);
        return PLI_EUNSUPPORTED;
    }
    if (rows == 0) return PLI_OK;
    PLI_REQUIRE(logits && tokens, "pli_sample: null pointer");
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case PLI_F32:
            return launch_sample<float>(logits, ld_logits, rows, vocab, temperature, top_k, top_p, uniforms, seed,
                                        offset_dev, offset_add, tokens, ld_tokens, s);
        case PLI_F16:
            return launch_sample<f16_t>(logits, ld_logits, rows, vocab, temperature, top_k, top_p, uniforms, seed,
                                        offset_dev, offset_add, tokens, ld_tokens, s);
        default:
            return launch_sample<bf16_t>(logits, ld_logits, rows, vocab, temperature, top_k, top_p, uniforms, seed,
                                         offset_dev, offset_add, tokens, ld_tokens, s);
    }
}
