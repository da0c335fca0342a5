/*
 * pli.h -- C ABI of libpli_hip.so, the MI355X (gfx950) hot path of
 * Infatoshi/physics-llm-inference re-built as hand-written HIP kernels.
 *
 * Conventions (every entry point):
 *   - plain pointers and sizes only; no torch / HIP types in signatures.
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - the CALLER owns every buffer, outputs included; the library never
 *     allocates, frees or synchronises (calls are graph-capturable).
 *   - device pointers must be 16-byte aligned for the vectorised kernels;
 *     misaligned / oddly strided operands are routed to the generic kernels.
 *   - strides are in ELEMENTS; the innermost (head_dim / K) stride is 1.
 *   - empty operands: a pointer to an operand with zero elements may be NULL
 *     (torch hands out a NULL data_ptr for empty tensors).  A call whose
 *     output is empty does nothing and returns PLI_OK; an empty reduction
 *     (no keys, K == 0) writes what torch gives for it (O = 0, C = bias or
 *     0, y = 0).
 *   - return value: PLI_OK (0), a hipError_t code (1..999) from the launch,
 *     or one of the PLI_E* codes below.  pli_last_error() returns a
 *     thread-local message for the last failing call on this thread.
 *
 * The reference has no FFI layer: its boundary is a set of
 * Python call signatures.  Each entry point below names the reference
 * function whose device arithmetic it replaces; the Python mirror packages
 * (physics-llm-inference_amd/ch0X) keep those signatures and call in here.
 */
#ifndef PLI_H
#define PLI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points
 * declared here are exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* element types */
enum {
    PLI_F32 = 0,
    PLI_F16 = 1,
    PLI_BF16 = 2
};

/* status codes beyond hipError_t */
enum {
    PLI_OK = 0,
    PLI_EINVAL = 1000,      /* bad argument (shape, stride, dtype, null)     */
    PLI_EUNSUPPORTED = 1001 /* valid but not implemented on this path        */
};

/* Library version string, e.g. "pli_hip 0.1.0 gfx950". */
const char* pli_version(void);

/* Message for the last non-zero return on the calling thread ("" if none). */
const char* pli_last_error(void);

/* The kernels the calling thread's last entry-point call launched, in launch
 * order, '+'-separated (e.g. "attn_fwd_v13c", "gemm_splitk_lds_nt+
 * gemm_splitk_reduce"); "" when it launched none (an empty output).  For
 * tests and tuning: which route the dispatch took. */
const char* pli_last_route(void);

/* Synchronous debug mode: when on, every kernel launch is
 * followed by hipDeviceSynchronize + hipGetLastError, and a failure is
 * returned by the entry point that launched the kernel, its name in
 * pli_last_error() ("<kernel>: kernel failed (PLI_SYNC): ...").  Starts as
 * the environment says (PLI_SYNC=1 or HIP_LAUNCH_BLOCKING=1: on; else off).
 * mode 0 / 1 sets
 * it, mode < 0 only queries; returns the previous state.  Debugging only:
 * it serialises every call and must not be on while a stream is captured. */
int pli_debug_sync(int mode);

/*
 * Fused attention forward:  O = softmax(Q K^T * scale [+ causal mask]) V.
 *
 * Replaces the device work of
 *   ch06/flash_attention.py:14-74   flash_attention_forward (tile loop)
 *   ch06/attention_memory.py:19-33  naive_attention
 *   ch01/attention.py:65-69         MultiHeadAttention.forward core
 *   ch01/gqa.py:30-34               GQA (kv head = h / (H / Hkv), no repeat)
 *
 * Layout: logical [batch, heads, n, head_dim]; q/o have `heads` heads and
 * n_q rows, k/v have `kv_heads` heads and n_kv rows.  strides[12] holds, in
 * elements, {q_b, q_h, q_n, k_b, k_h, k_n, v_b, v_h, v_n, o_b, o_h, o_n}.
 * causal != 0 masks key j for query i when j > i + (n_kv - n_q)
 * (bottom-right aligned, = torch.triu(ones, diagonal=1) when n_q == n_kv).
 * dtype: PLI_BF16 / PLI_F16 with head_dim 64 or 128 run the MFMA kernels --
 * attn_fwd_v13 (one generated program per dtype x head_dim x causal x
 * whole / ragged key tiles) where n_kv > 64 (causal: n_q <= n_kv, any
 * diagonal offset), else attn_fwd_v12 / v10; PLI_F32 (and any other
 * head_dim <= 256) the generic fp32-accumulate kernel.  Softmax statistics
 * are fp32 regardless of dtype.  n_kv == 0 gives O = 0.
 */
int pli_flash_attn_fwd(const void* q, const void* k, const void* v, void* o,
                       int batch, int heads, int kv_heads, int n_q, int n_kv,
                       int head_dim, const int64_t* strides, float scale,
                       int causal, int dtype, void* stream);

/*
 * GEMV  y[m] = sum_k W[m, k] * x[k]   (fp32 accumulate, output in dtype).
 * Replaces torch.mv in ch03/gemv_benchmark.py:38 (decode weight GEMV).
 * W row-major with leading dimension ldw (elements, >= k).
 */
int pli_gemv(const void* w, const void* x, void* y, int m, int k, int64_t ldw,
             int dtype, void* stream);

/*
 * GEMM  C[m, n] = A[m, k] * op(B) (+ bias[n])   (fp32 accumulate).
 * trans_b = 0: B is [k, n] row-major (torch.mm, ch03/gemm_benchmark.py:35,
 *              ch05/tiled_matmul.cu:22-61);
 * trans_b = 1: B is [n, k] row-major, i.e. C = A B^T (F.linear,
 *              ch09/tensor_parallel.py:39,67; ch01/attention.py:59-61,71;
 *              x @ weight.T of ch03/batching_benchmark.py:30).
 * bias may be NULL.  A, C row-major with leading dimensions lda, ldc.
 */
int pli_gemm(const void* a, const void* b, void* c, const void* bias, int m,
             int n, int k, int64_t lda, int64_t ldb, int64_t ldc, int trans_b,
             int dtype, void* stream);

/*
 * NT GEMM with an fp32 output: C[m, n] = A[m, k] * B[n, k]^T, A / B bf16 or
 * fp16 (dtype), C fp32 contiguous (ldc = n), fp32 accumulate -- the
 * row-parallel partial of ch09/tensor_parallel.py:66-68 kept in fp32 so the
 * all-reduce sums unrounded partials (RowParallelLinear(reduce_dtype=
 * torch.float32)).  Routes, in the order gemm.hip pli_gemm_f32out checks
 * them: (1) K % 64 == 0, N % 32 == 0, lda % 8 == 0, ldb % 8 == 0, A / B / C
 * 16-byte aligned, M >= 512, N >= 512, at least 128 tiles of 256 x 256 and
 * 256 rows of A and B addressable by a 32-bit offset: gemm_w5 with an fp32
 * epilogue (its persistent walk when M, N are multiples of 256 and K >=
 * 128); (2) the rest of (1)'s alignment class (K % 64 == 0, N % 32 == 0,
 * lda / ldb % 8 == 0, 16-byte aligned A / B / C): the LDS split-K kernel
 * with one slice; (3) everything else: a one-thread-per-output kernel.
 */
int pli_gemm_f32out(const void* a, const void* b, float* c, int m, int n, int k, int64_t lda,
                    int64_t ldb, int dtype, void* stream);

/*
 * pli_gemm with a caller-owned device workspace (16-byte aligned) of at least
 * pli_gemm_workspace_size(m, n, k, trans_b, dtype) bytes (0: none needed, the
 * call is pli_gemm).  Decode-batch / TP-shard NT shapes (16 < m <= 256) then
 * split K over workgroups and sum the fp32 slices in a fixed order (the
 * ch09/tensor_parallel.py:67 row shard at M = 128, ch03/batching_benchmark.py
 * batches).  The workspace is scratch: nothing persists between calls.
 */
size_t pli_gemm_workspace_size(int m, int n, int k, int trans_b, int dtype);
int pli_gemm_ws(const void* a, const void* b, void* c, const void* bias, int m,
                int n, int k, int64_t lda, int64_t ldb, int64_t ldc, int trans_b,
                int dtype, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Fused SwiGLU projection  h[m, n] = silu(x Wg^T)[m, n] * (x Wu^T)[m, n]
 * (fp32 accumulate, silu(g) = g / (1 + e^-g)).
 * Replaces gate_proj -> silu, up_proj, multiply of
 *   ch09/tensor_parallel.py:95-99   TensorParallelMLP.forward (per rank)
 *   ch01/ffn.py:34-39               SwiGLUFFN; ch01/ffn.py:51-57 FusedSwiGLUFFN
 *                                   (gate_up_proj halves: wg = W, wu = W + n*ldw)
 *   ch02/cached_generation.py:119   SwiGLUFFN of the cached model
 * x [m, k] (ldx), wg / wu [n, k] row-major (ldwg, ldwu), h [m, n] (ldh).
 * Neither gate nor up is written to memory.
 */
int pli_gemm_swiglu(const void* x, const void* wg, const void* wu, void* h,
                    int m, int n, int k, int64_t ldx, int64_t ldwg,
                    int64_t ldwu, int64_t ldh, int dtype, void* stream);
/* pli_gemm_swiglu with a caller workspace of pli_gemm_swiglu_workspace_size
 * bytes (0: none needed): decode batches (16 < m <= 256) split K over
 * workgroups for gate and up and apply silu(g) * u in a fixed-order reduce. */
size_t pli_gemm_swiglu_workspace_size(int m, int n, int k, int dtype);
int pli_gemm_swiglu_ws(const void* x, const void* wg, const void* wu, void* h,
                       int m, int n, int k, int64_t ldx, int64_t ldwg,
                       int64_t ldwu, int64_t ldh, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);

/*
 * HBM calibration kernels of ch05/coalescing.cu:7-20 (fp32):
 *   out[i] = 2 * in[i * stride],  i in [0, n_out).
 * stride == 1 is the coalesced stream (16-byte vector loads), the roofline
 * denominator measured on the device; stride > 1 is the strided contrast.
 */
int pli_scale_copy(const float* in, float* out, int64_t n_out, int stride,
                   void* stream);

/*
 * Roofline calibration (ch03/roofline.py measure_mfma_peak): `blocks`
 * workgroups of 256 threads, one per CU (96 KiB of LDS each) so ONE wave per
 * SIMD, each wave issuing `iters` rounds of back-to-back bf16 MFMAs from
 * registers into independent accumulators, pseudo-random operands; both
 * shapes the same 64x64 output tile per wave and 262,144 FLOP per round
 * (shape 0: 8 x v_mfma_f32_32x32x16_bf16, 1: 16 x v_mfma_f32_16x16x32_bf16).
 * One float per thread goes to out[blocks * 256] so the work is not dead;
 * when `clocks` is non-null, wave w writes clocks[2w] = s_memtime ticks
 * (shader clock) and clocks[2w+1] = s_memrealtime ticks (100 MHz) around its
 * loop.  FLOPs = blocks * 4 * iters * 262144.
 */
int pli_mfma_probe(float* out, uint64_t* clocks, int blocks, int iters, int shape, void* stream);

/*
 * ch05/tiled_matmul.cu:9-20 naive_matmul (the contrast kernel of the ch05
 * demo): C[m][n] = sum_k A[m][k] B[k][n], fp32 row-major, one thread per
 * output element straight from global memory.  Not a production path --
 * pli_gemm with PLI_F32 runs the MFMA tile kernel.
 */
int pli_gemm_naive(const float* a, const float* b, float* c, int m, int n, int k, int64_t lda,
                   int64_t ldb, int64_t ldc, void* stream);

/*
 * Read-only HBM calibration (ch03/roofline.py measure_hbm_read_bandwidth):
 * `blocks` x 256 threads stream `bytes` (16-byte aligned, multiple of 16)
 * with 16-byte non-temporal loads; one XOR word per thread goes to
 * out[blocks * 256].  mode 0: grid-stride (4 loads per lane in flight);
 * mode 1: one contiguous slice per block, 8 loads per lane in flight.
 */
int pli_hbm_read_probe(const void* buf, int64_t bytes, uint32_t* out, int blocks, int mode,
                       void* stream);

/*
 * Row softmax with the single-pass online (max, sum) recurrence of
 * ch06/online_softmax.py:13-25 (== standard_softmax, :5-10), over the last
 * dimension of a contiguous [rows, n] tensor; statistics in fp32.
 */
int pli_softmax_rows(const void* x, void* y, int64_t rows, int n, int dtype,
                     void* stream);

/*
 * ch06/online_softmax.py:28-53 online_softmax_with_output over contiguous
 * x [rows, n] and v [rows, n, dv]:  o[r] = sum_i softmax(x[r])_i v[r, i],
 * d[r] = sum_i exp(x[r, i] - max_r).  o is [rows, dv], d is [rows].
 */
int pli_online_softmax_with_output(const void* x, const void* v, void* o,
                                   void* d, int64_t rows, int n, int dv,
                                   int dtype, void* stream);

/* Decode attention over a KV cache (split-K flash-decoding).
 * Replaces the decode branch of ch02/kv_cache.py:74-101 (GQAWithCache.forward)
 * and ch02/cached_generation.py:58-98 (CachedGQA.forward): repeat_interleave
 * of the cache to Hq heads, matmul, softmax, matmul.
 * Same operand conventions as pli_flash_attn_fwd (strides[12] in elements,
 * q/o [B, Hq, n_q, D]-indexed, k/v [B, Hkv, n_kv, D]-indexed; the cache
 * layout [B, S_max, Hkv, D] is k_b = S_max*Hkv*D, k_h = D, k_n = Hkv*D).
 * causal masks bottom-right (query i sees keys j <= n_kv - n_q + i), the mask
 * of ch02/kv_cache.py:91-95.  The fast path takes bf16/fp16, D in {64, 128}
 * and n_q * Hq/Hkv <= 16 rows per kv head; other shapes run the prefill
 * kernel.  `workspace` (16-byte aligned, fp32 partials) must hold
 * pli_attn_decode_workspace_size(...) bytes; NULL when that is 0. */
size_t pli_attn_decode_workspace_size(int batch, int heads, int kv_heads,
                                      int n_q, int n_kv, int head_dim);
int pli_attn_decode(const void* q, const void* k, const void* v, void* o,
                    int batch, int heads, int kv_heads, int n_q, int n_kv,
                    int head_dim, const int64_t* strides, float scale,
                    int causal, void* workspace, size_t workspace_bytes,
                    int dtype, void* stream);

/*
 * RMSNorm with an optional fused residual add (rows of n elements):
 *   h = x + residual (stored in dtype, as the torch add would; h = x when
 *   residual is NULL), y = h / sqrt(mean(h^2) + eps) * weight, fp32 statistics.
 * Replaces ch02/cached_generation.py:101-109 (RMSNorm.forward) and the
 * residual adds of CachedTransformerBlock.forward (:143-145).  residual and
 * h_out may be NULL; h_out must not alias x or residual.
 */
int pli_rmsnorm(const void* x, const void* residual, const void* weight, void* y,
                void* h_out, int64_t rows, int n, int64_t ldx, int64_t ldr,
                int64_t ldy, int64_t ldh, float eps, int dtype, void* stream);

/*
 * Mixture of experts (ch09/moe_layer.py:18-83: Router softmax/topk/renorm and
 * the per-expert masked loop).
 *
 * pli_moe_route: logits [tokens, experts] (ld_logits) -> per (token, k):
 *   weights (fp32; renormalised over the k when normalize), expert_idx,
 *   pos (row of the expert-sorted activation matrix); gather[row] = token;
 *   offsets[experts + 1] = each expert's row range.  experts <= 64, top_k <= 8.
 *   workspace: int32 [experts + tokens * top_k].
 * pli_gemm_grouped: for every expert e, rows r in [offsets[e], offsets[e+1]):
 *   c[r] = x[gather[r]] W_e^T  (gather NULL = identity), or with wu_ptrs
 *   silu(x W1_e^T) * (x W3_e^T); w_ptrs / wu_ptrs are DEVICE arrays of the
 *   experts' [n, k] weight pointers; rows_bound >= offsets[experts], the
 *   number of sorted rows (a host value: it also bounds every expert's rows,
 *   picks the kernel and sizes its grid; a smaller value leaves rows
 *   unwritten); c holds rows_bound rows.  bf16/fp16, k % 128 == 0, n % 16 == 0.
 *   Any number of experts the grid of the chosen kernel holds: the LDS-staged
 *   kernel (16 < rows_bound <= 1024) indexes experts in blockIdx.z and is
 *   chosen only for experts <= 65535; beyond that the weight-streaming and
 *   256-row-tile kernels run ("grid too large" past 2^31 workgroups).
 * pli_moe_combine: out[t] = sum_k weights[t, k] * y[pos[t, k]] (fp32 sum in k
 *   order).
 */
int pli_moe_route(const void* logits, int64_t ld_logits, int tokens, int experts,
                  int top_k, int normalize, int dtype, float* weights,
                  int32_t* expert_idx, int32_t* pos, int32_t* gather,
                  int32_t* offsets, int32_t* workspace, void* stream);
int pli_gemm_grouped(const void* x, const int32_t* gather,
                     const void* const* w_ptrs, const void* const* wu_ptrs,
                     void* c, const int32_t* offsets, int experts, int rows_bound,
                     int n, int k, int64_t ldx, int64_t ldw, int64_t ldc,
                     int dtype, void* stream);
int pli_moe_combine(const void* y, int64_t ldy, const int32_t* pos,
                    const float* weights, void* out, int64_t ldo, int tokens,
                    int top_k, int hidden, int dtype, void* stream);

/* Graph-replayable decode (ch08/cuda_graph.py:18-82 captures the decode step;
 * a captured launch cannot take the growing cache length as a host value).
 *
 * pli_kv_append: write n_new tokens of K and V ([B, n_new, Hkv, D]) into the
 * caches at rows *pos_dev .. *pos_dev + n_new - 1 (rows >= capacity are
 * dropped) -- the device-side form of KVCache.update, ch02/kv_cache.py:37-48.
 * strides[12] in elements: {kn_b, kn_h, kn_n, kc_b, kc_h, kc_n, vc_b, vc_h,
 * vc_n, vn_b, vn_h, vn_n}.  bf16/fp16, head_dim % 8 == 0.
 *
 * pli_attn_decode_dev: pli_attn_decode over n_kv = min(*n_kv_dev + n_kv_add,
 * n_kv_max) valid cache rows; the split-K grid and the workspace are sized
 * for n_kv_max (pli_attn_decode_workspace_size(..., n_kv_max, ...)).
 * Fast-path shapes only (else PLI_EUNSUPPORTED). */
int pli_kv_append(const void* k_new, const void* v_new, void* k_cache,
                  void* v_cache, int batch, int n_new, int kv_heads,
                  int head_dim, int capacity, const int64_t* strides,
                  const int32_t* pos_dev, int dtype, void* stream);
/* pli_gemm_multi_nt: the q, k and v projections of a decode step in one
 * launch, k / v written straight into the caches (fuses pli_kv_append).
 * Up to 3 groups share x [m, k] (m <= 128 rows = batch x tokens_per_batch);
 * group g computes x W_g^T ([n_g, k] weights, ldw_g) and stores row
 * r = b * tokens_per_batch + s at
 *   c_g + b * stride_batch_g + (s + *row_offset_g) * stride_token_g (+ col),
 * row_offset_g a device int32 or NULL (= 0); rows >= capacity_g are dropped.
 * bf16/fp16, k % 8 == 0; m > 16 (small-M MFMA kernel) also needs k % 128 == 0,
 * n_g % 16 == 0, strides % 4 == 0 and 8-byte aligned c_g. */
int pli_gemm_multi_nt(const void* x, int64_t ldx, int m, int k,
                      int tokens_per_batch, const void* const* w,
                      void* const* c, const int* n, const int64_t* ldw,
                      const int64_t* stride_batch, const int64_t* stride_token,
                      const int32_t* const* row_offset, const int* capacity,
                      int ngroups, int dtype, void* stream);
/* pli_rms_gemm_nt: a decode-step RMSNorm fused into the projection that
 * consumes it (ch02/cached_generation.py:112-120 RMSNorm -> :58-69 q/k/v,
 * :136-140 gate/up, :180-185 final norm -> lm_head).  Rows: h = a (+ residual)
 * (written to h_out if not NULL), y = h * rsqrt(mean(h^2) + eps) * norm_weight
 * -- bitwise the row pli_rmsnorm writes -- kept on chip; then the groups of
 * pli_gemm_multi_nt on y (w_up non-NULL: every group is SwiGLU,
 * silu(y.w) * (y.w_up), w_up rows with the same ldw).  1 <= m <= 4 rows,
 * k % 8 == 0, k <= 8192, bf16/fp16.  A workgroup holds the m normalised rows
 * in m * k * 2 + 16 bytes of LDS: 65552 at the largest shape (m = 4,
 * k = 8192), inside the 163840 bytes a gfx950 workgroup may use, so every
 * shape these rules accept is launched. */
int pli_rms_gemm_nt(const void* a, int64_t lda, const void* residual, int64_t ldr,
                    const void* norm_weight, float eps, void* h_out, int64_t ldh, int m, int k,
                    int tokens_per_batch, const void* const* w, const void* const* w_up,
                    void* const* c, const int* n, const int64_t* ldw,
                    const int64_t* stride_batch, const int64_t* stride_token,
                    const int32_t* const* row_offset, const int* capacity, int ngroups,
                    int dtype, void* stream);
int pli_attn_decode_dev(const void* q, const void* k, const void* v, void* o,
                        int batch, int heads, int kv_heads, int n_q,
                        int n_kv_max, int head_dim, const int64_t* strides,
                        float scale, int causal, const int32_t* n_kv_dev,
                        int n_kv_add, void* workspace, size_t workspace_bytes,
                        int dtype, void* stream);

/* Paged KV cache: decode attention straight over the block pool, and the
 * append that feeds it.  Serves ch07/paged_memory.py:16-51,171-175: the
 * reference's PagedKVCache allocates the pools k_cache / v_cache
 * [num_blocks, num_layers, block_size, num_heads, head_dim] and describes, but
 * never writes, the attention kernel that "reads from scattered blocks / uses
 * block table for indirection".
 *
 * block_table: device int32 [batch, max_blocks_per_seq], entry (b, i) the
 *   page that holds tokens i*block_size .. (i+1)*block_size - 1 of sequence b.
 *   Entries are clamped into [0, num_blocks - 1] before use, so a stale entry
 *   reads the wrong page, never memory outside the pool; unused entries should
 *   still hold a valid page index.
 * seq_lens: device int32 [batch].  Both are read on the device, nothing is
 *   allocated or synchronised: the calls can be captured in a graph and
 *   replayed while the table and the lengths change in place.
 * Pools: k_pool / v_pool point at page 0; a layer view k_cache[:, layer] of
 *   the reference layout is passed without a copy through its strides.
 *
 * pli_attn_decode_paged: sequence b attends over its first
 *   n_kv(b) = clamp(seq_lens[b] + n_kv_add, 0, max_kv) tokens.  q / o are
 *   [B, Hq, n_q, D]-indexed.  strides[12] in elements: {q_b, q_h, q_n,
 *   k_page, k_token, k_head, v_page, v_token, v_head, o_b, o_h, o_n}.
 *   max_kv is a host upper bound on every length (<= max_blocks_per_seq *
 *   block_size): the split-K grid and the workspace are sized for it, as
 *   pli_attn_decode_dev's are for n_kv_max.  causal masks bottom-right per
 *   sequence (query i sees keys j <= n_kv(b) - n_q + i); a row that sees no
 *   key (an empty sequence among them) is written as 0.
 *   The MFMA kernel attn_decode_paged takes bf16/fp16, D in {64, 128},
 *   n_q * Hq/Hkv <= 16 rows per kv head, a power-of-two block_size >= 16,
 *   scale > 0, strides % 8 == 0 and 16-byte aligned operands; everything else
 *   (fp32, head_dim <= 256, any block_size) runs attn_decode_paged_generic,
 *   a correctness path.  `workspace` (16-byte aligned, fp32 partials) must
 *   hold pli_attn_decode_paged_workspace_size bytes; NULL when that is 0.
 *   pli_last_route: "attn_decode_paged", "attn_decode_paged+
 *   attn_decode_paged_combine" or "attn_decode_paged_generic".
 * pli_kv_append_paged: token t of k_new / v_new ([B, n_new, Hkv, D]) of
 *   sequence b goes to logical position seq_lens[b] + t; positions >=
 *   max_blocks_per_seq * block_size are dropped.  seq_lens is not advanced
 *   (the caller adds n_new on the device).  strides[12] in elements: {kn_b,
 *   kn_h, kn_n, k_page, k_token, k_head, v_page, v_token, v_head, vn_b, vn_h,
 *   vn_n}.  Rows of whole 16-byte chunks: head_dim and every stride a multiple
 *   of 8 (bf16/fp16) or 4 (fp32) elements, 16-byte aligned operands.
 * PLI_EINVAL before any HIP call for bad shapes, heads % kv_heads != 0, null
 * pointers, a non-finite scale, block_size <= 0, max_kv > max_blocks_per_seq *
 * block_size, a short workspace; an empty output (batch == 0, n_q == 0,
 * n_new == 0) returns PLI_OK and its operands may be NULL. */
size_t pli_attn_decode_paged_workspace_size(int batch, int heads, int kv_heads,
                                            int n_q, int max_kv, int head_dim);
int pli_attn_decode_paged(const void* q, const void* k_pool, const void* v_pool,
                          void* o, const int32_t* block_table,
                          const int32_t* seq_lens, int batch, int heads,
                          int kv_heads, int n_q, int head_dim, int block_size,
                          int num_blocks, int max_blocks_per_seq, int max_kv,
                          const int64_t* strides, float scale, int causal,
                          int n_kv_add, void* workspace, size_t workspace_bytes,
                          int dtype, void* stream);
int pli_kv_append_paged(const void* k_new, const void* v_new, void* k_pool,
                        void* v_pool, const int32_t* block_table,
                        const int32_t* seq_lens, int batch, int n_new,
                        int kv_heads, int head_dim, int block_size,
                        int num_blocks, int max_blocks_per_seq,
                        const int64_t* strides, int dtype, void* stream);

/* Packed variable-length attention over the same paged pool: one call for a
 * step in which every sequence brings its own number of new tokens (prompt
 * chunks, decode rows, sequences that sit the step out).  The kernel the
 * reference's ch08 text assumes ("process all in single forward pass ...
 * FlashAttention handles both cases") and never writes.
 *
 * q / o: packed [max_tokens, heads, head_dim].  cu_seqlens_q: device int32
 *   [batch + 1]; sequence b owns packed tokens cu[b] .. cu[b+1] - 1,
 *   q_len(b) = max(0, cu[b+1] - cu[b]); a q_len of 0 sits the step out.
 * seq_lens[b]: the kv length AFTER this step's tokens are in the pool;
 *   n_kv(b) = clamp(seq_lens[b], 0, max_kv).  block_table and the pools are
 *   those of pli_attn_decode_paged.
 * pli_attn_varlen_paged: strides[10] in elements: {q_t, q_h, k_page, k_token,
 *   k_head, v_page, v_token, v_head, o_t, o_h}.  causal masks bottom-right:
 *   token i of sequence b sees keys j <= n_kv(b) - q_len(b) + i; causal == 0:
 *   every key below n_kv(b).  A row that sees no key (n_kv < q_len among them)
 *   is written as 0; packed rows >= min(cu[batch], max_tokens) are not written.
 *   cu_seqlens_q, block_table and seq_lens are read on the device; the grid
 *   depends on (batch, max_tokens, heads, kv_heads) only; nothing is allocated
 *   or synchronised and there is no workspace, so the call replays in a
 *   captured graph while the three tensors change in place.  Every address is
 *   clamped into its operand whatever the three tensors hold.
 *   The MFMA kernel attn_varlen_paged takes bf16/fp16, D in {64, 128},
 *   heads/kv_heads in {1, 2, 4, 8, 16}, a power-of-two block_size >= 16,
 *   scale > 0, strides % 8 == 0 and 16-byte aligned operands; everything else
 *   (fp32, head_dim <= 256, any block_size, any group size) runs
 *   attn_varlen_paged_generic, a correctness path.  pli_last_route names one
 *   of the two.
 * pli_kv_append_varlen_paged: token i of sequence b (packed row cu[b] + i of
 *   k_new / v_new [max_tokens, Hkv, D]) goes to logical position
 *   seq_lens[b] - q_len(b) + i; negative positions and positions >=
 *   max_blocks_per_seq * block_size are dropped.  It takes the same three
 *   device tensors as the attention call.  strides[10] in elements: {kn_t,
 *   kn_h, k_page, k_token, k_head, v_page, v_token, v_head, vn_t, vn_h}; rows of
 *   whole 16-byte chunks as for pli_kv_append_paged.  pli_last_route:
 *   "kv_append_varlen_paged".
 * PLI_EINVAL before any HIP call as for the paged entry points above; an
 * empty call (batch == 0 or max_tokens == 0) returns PLI_OK and its operands
 * may be NULL. */
int pli_attn_varlen_paged(const void* q, const void* k_pool, const void* v_pool,
                          void* o, const int32_t* cu_seqlens_q,
                          const int32_t* block_table, const int32_t* seq_lens,
                          int batch, int max_tokens, int heads, int kv_heads,
                          int head_dim, int block_size, int num_blocks,
                          int max_blocks_per_seq, int max_kv,
                          const int64_t* strides, float scale, int causal,
                          int dtype, void* stream);
int pli_kv_append_varlen_paged(const void* k_new, const void* v_new,
                               void* k_pool, void* v_pool,
                               const int32_t* cu_seqlens_q,
                               const int32_t* block_table,
                               const int32_t* seq_lens, int batch,
                               int max_tokens, int kv_heads, int head_dim,
                               int block_size, int num_blocks,
                               int max_blocks_per_seq, const int64_t* strides,
                               int dtype, void* stream);

/* The same four calls over a 1-byte KV pool: OCP fp8 e4m3fn codes (not fnuz;
 * 0x7E = 448 the largest finite value, 0x7F / 0xFF NaN, no infinity) in the
 * layout above, one byte per element, so the same memory holds twice the
 * tokens and decode attention reads half the bytes.
 *
 * Pools: k_pool / v_pool point at page 0 of byte pools; their strides are in
 *   elements, which are bytes.
 * Scales: k_scale / v_scale are device fp32 [kv_heads]; an element's value is
 *   code * scale[kv head].  They are read on the device, so a captured call
 *   replays while the scales change in place.  NULL means all ones.  A scale
 *   must be finite and > 0; any other value gives unspecified values in that
 *   head's rows and never an access outside an operand.
 * Attention: scores = scale * k_scale[hk] * (q . K8), O = v_scale[hk] *
 *   softmax(scores) . V8, K8 / V8 the codes' values.  Each code is widened
 *   exactly to q's type on its way into the kernel (every e4m3 value is a bf16
 *   and an fp16 value); k_scale is folded into the softmax constant and v_scale
 *   into the final 1/l, so the result is attention over the dequantised pool
 *   with the arithmetic of the 16-bit kernels.  `dtype` is q / o's.
 * Append: code = e4m3fn_rne(clamp(x * inv, -448, 448)), inv = 1.0f / scale[h]
 *   and the product in fp32, round to nearest even.  NaN stays NaN (0x7F /
 *   0xFF by its sign), +-inf and everything past +-448 saturate to +-448.
 *   `dtype` is the source's (fp32 / fp16 / bf16).
 *
 * pli_attn_decode_paged_fp8: pli_attn_decode_paged otherwise, workspace from
 *   pli_attn_decode_paged_workspace_size.  The MFMA kernel
 *   attn_decode_paged_fp8 takes what attn_decode_paged takes with the pool
 *   strides multiples of 16 (bytes) and q / o strides multiples of 8; it loads
 *   16 codes per lane and instruction.  pli_last_route:
 *   "attn_decode_paged_fp8", "attn_decode_paged_fp8+attn_decode_paged_combine"
 *   or "attn_decode_paged_generic_fp8" (fp32 q, any head_dim <= 256, any
 *   block_size; it decodes with csrc/fp8_codec.h).
 * pli_attn_varlen_paged_fp8: pli_attn_varlen_paged otherwise; the same rule
 *   picks "attn_varlen_paged_fp8" or "attn_varlen_paged_generic_fp8".
 * pli_kv_append_paged_fp8 / pli_kv_append_varlen_paged_fp8: positions, drops
 *   and clamps of the 16-bit appends.  strides as there: the source's in its
 *   elements, the pools' in bytes.  Rows of whole 8-element chunks: head_dim
 *   and every stride a multiple of 8, 16-byte aligned operands.
 *   pli_last_route: "kv_append_paged_fp8" / "kv_append_varlen_paged_fp8".
 * Argument checks, PLI_EINVAL and empty calls as for the 16-bit calls. */
int pli_attn_decode_paged_fp8(const void* q, const void* k_pool,
                              const void* v_pool, void* o,
                              const int32_t* block_table,
                              const int32_t* seq_lens, const float* k_scale,
                              const float* v_scale, int batch, int heads,
                              int kv_heads, int n_q, int head_dim,
                              int block_size, int num_blocks,
                              int max_blocks_per_seq, int max_kv,
                              const int64_t* strides, float scale, int causal,
                              int n_kv_add, void* workspace,
                              size_t workspace_bytes, int dtype, void* stream);
int pli_kv_append_paged_fp8(const void* k_new, const void* v_new, void* k_pool,
                            void* v_pool, const int32_t* block_table,
                            const int32_t* seq_lens, const float* k_scale,
                            const float* v_scale, int batch, int n_new,
                            int kv_heads, int head_dim, int block_size,
                            int num_blocks, int max_blocks_per_seq,
                            const int64_t* strides, int dtype, void* stream);
int pli_attn_varlen_paged_fp8(const void* q, const void* k_pool,
                              const void* v_pool, void* o,
                              const int32_t* cu_seqlens_q,
                              const int32_t* block_table,
                              const int32_t* seq_lens, const float* k_scale,
                              const float* v_scale, int batch, int max_tokens,
                              int heads, int kv_heads, int head_dim,
                              int block_size, int num_blocks,
                              int max_blocks_per_seq, int max_kv,
                              const int64_t* strides, float scale, int causal,
                              int dtype, void* stream);
int pli_kv_append_varlen_paged_fp8(const void* k_new, const void* v_new,
                                   void* k_pool, void* v_pool,
                                   const int32_t* cu_seqlens_q,
                                   const int32_t* block_table,
                                   const int32_t* seq_lens,
                                   const float* k_scale, const float* v_scale,
                                   int batch, int max_tokens, int kv_heads,
                                   int head_dim, int block_size,
                                   int num_blocks, int max_blocks_per_seq,
                                   const int64_t* strides, int dtype,
                                   void* stream);

/* Split-K for the packed calls: pli_attn_varlen_paged / _fp8 with a caller
 * workspace.  The plain calls give a 64-row tile one workgroup that walks all
 * of the tile's keys; these cut the tile's key range [0, key_end) into chunks
 * of `span` keys, give every chunk a workgroup, and merge the chunks' fp32
 * partials in a second kernel.  The plain calls are untouched.
 *
 * split_keys: > 0 the span, a multiple of 64; 0 the plan's choice, span =
 *   max(2048, round-up-to-64(ceil(max_kv / 16))): at most 16 chunks per tile
 *   whatever max_kv is, and no split at all up to 2048 keys.  splits_max = max(1, ceil(max_kv / span)) is the
 *   number of chunks the grid provides per tile.  span and splits_max depend
 *   on the host arguments only (pli_attn_varlen_paged_split_plan reports
 *   them), so the grid and the workspace replay in a captured graph while
 *   cu_seqlens_q, block_table and seq_lens change in place; a tile uses
 *   max(1, ceil(key_end / span)) of its chunks, counted on the device, and
 *   the other workgroups leave before any K / V load.
 * workspace: pli_attn_varlen_paged_workspace_size bytes = splits_max *
 *   max_tokens * heads * (head_dim + 2) * 4 (fp32 partial O, then (m, l) per
 *   (chunk, packed token, head)), 16-byte aligned; it need not be initialised
 *   and holds nothing between calls.  The size is 0 when splits_max == 1 or
 *   when the shape (head_dim, heads / kv_heads) can only take the generic
 *   kernel; the workspace may then be NULL.
 * Routes (pli_last_route): "attn_varlen_paged_split+attn_varlen_paged_combine"
 *   or "attn_varlen_paged_split_fp8+attn_varlen_paged_combine"; when
 *   splits_max == 1 the call IS the plain call ("attn_varlen_paged" /
 *   "attn_varlen_paged_fp8", same kernel, same cost); when the MFMA kernel's
 *   rule fails the generic kernel runs as in the plain call and the workspace
 *   is not used.  Rows of a tile with one chunk are bitwise those of the plain
 *   call; rows merged from several chunks differ from it by fp32 rounding.
 * Which call: the _ws call wins where tiles are few and long -- decode rows
 *   or one prompt chunk at long context, alone or inside a mixed step
 *   (measured 1.7x - 4.3x over the plain call at 32k keys, 2.6x - 6.3x over
 *   an fp8 pool).  A step whose tiles already fill the device (about a
 *   thousand workgroups of 4k keys each) is 1.17x SLOWER when it is cut in
 *   two and 1.9x slower when max_kv is 32k while every sequence holds 4k:
 *   such a step should take the plain call, and every caller should pass the
 *   max_kv it needs rather than the pool's.  Decode-only batches stay on
 *   pli_attn_decode_paged (1.25x faster than this call).  DESIGN.md section
 *   3.2e has the numbers.
 * PLI_EINVAL before any HIP call: everything the plain calls reject, a
 *   negative split_keys or one that is not a multiple of 64, a NULL,
 *   misaligned or short workspace when the size is > 0, a grid past 2^31.
 *   Empty calls (batch == 0 or max_tokens == 0) return PLI_OK and their
 *   operands may be NULL.  Nothing is allocated or synchronised. */
size_t pli_attn_varlen_paged_workspace_size(int batch, int max_tokens, int heads,
                                            int kv_heads, int max_kv,
                                            int head_dim, int split_keys);
int pli_attn_varlen_paged_split_plan(int batch, int max_tokens, int heads,
                                     int kv_heads, int max_kv, int head_dim,
                                     int split_keys, int* span,
                                     int* splits_max);
int pli_attn_varlen_paged_ws(const void* q, const void* k_pool,
                             const void* v_pool, void* o,
                             const int32_t* cu_seqlens_q,
                             const int32_t* block_table,
                             const int32_t* seq_lens, int batch, int max_tokens,
                             int heads, int kv_heads, int head_dim,
                             int block_size, int num_blocks,
                             int max_blocks_per_seq, int max_kv,
                             const int64_t* strides, float scale, int causal,
                             int dtype, int split_keys, void* workspace,
                             size_t workspace_bytes, void* stream);
int pli_attn_varlen_paged_fp8_ws(const void* q, const void* k_pool,
                                 const void* v_pool, void* o,
                                 const int32_t* cu_seqlens_q,
                                 const int32_t* block_table,
                                 const int32_t* seq_lens, const float* k_scale,
                                 const float* v_scale, int batch,
                                 int max_tokens, int heads, int kv_heads,
                                 int head_dim, int block_size, int num_blocks,
                                 int max_blocks_per_seq, int max_kv,
                                 const int64_t* strides, float scale,
                                 int causal, int dtype, int split_keys,
                                 void* workspace, size_t workspace_bytes,
                                 void* stream);

/* Weight-only fp8 linear (W8A16) for decode batches: the weight stream of
 * pli_gemv / pli_gemm NT / pli_gemm_swiglu at one byte per element.
 *
 * Weights: w8 [n, k] OCP fp8 e4m3fn codes (as the 1-byte KV pool above: 0x7E =
 *   448, 0x7F / 0xFF NaN), row-major, leading dimension ldw in bytes
 *   (= elements, >= k).  w_scale is device fp32 [n], one scale per output
 *   row, read on the device (a captured call replays while codes and scales
 *   change in place); NULL means all ones.  Element (j, i) has the value
 *   decode(code) * w_scale[j].
 * Result: C[r, j] = round_T( w_scale[j] * sum_i decode(w8[j, i]) * X[r, i]
 *   (+ bias[j]) ), the sum in fp32 and one rounding to T.  T (dtype) is bf16
 *   or fp16 and is the type of X, C and bias; PLI_F32 is refused.  Each code
 *   is widened exactly to T on its way into the kernel and a code x 16-bit
 *   product is exact in fp32, so the result is the 16-bit linear over the
 *   dequantised weights with the scale folded in after the sum.  A NaN code
 *   makes exactly the outputs of its row NaN.
 * SwiGLU: h = silu(wg_scale[j] * sum g) * (wu_scale[j] * sum u), silu(g) =
 *   g / (1 + e^-g) as pli_gemm_swiglu; neither gate nor up is written.
 * Routes, in this order, from host arguments only (csrc/fp8w_plan.h;
 *   pli_last_route names the kernels):
 *   1. k == 0: C = bias or 0 ("linear_fp8w_generic"); m == 0 or n == 0:
 *      nothing.
 *   2. "linear_fp8w_smallm" (MFMA 16x16x32): 1 < m <= 128, k % 256 == 0,
 *      n % 16 == 0, w8 / x / c 16-byte aligned, ldw % 16 == 0, ldx and ldc
 *      % 8 == 0.
 *   3. "linear_fp8w_vec" (VALU, one wave per 2 / 4 weight rows): m <= 16,
 *      k % 16 == 0, ldw % 16 == 0, ldx % 8 == 0, w8 / x 16-byte aligned.
 *      Its MACs are v_dot2 on the packed pairs (fp32 accumulate), so it
 *      agrees with the other routes to fp32 rounding, not bitwise.
 *   4. "fp8w_widen+<pli_gemm's route>": m > 16, no fast route, a workspace
 *      given, and pli_gemm's vector class (k, n, ldx, ldc % 8 == 0, x / c
 *      16-byte aligned, bias 8-byte aligned).  The codes are widened to
 *      T(decode * scale) (one fp32 multiply, one rounding) into the
 *      workspace, contiguous [n][k], and the existing pli_gemm (trans_b = 1)
 *      or pli_gemm_swiglu (gate, then up at the next 16-byte boundary) runs
 *      over them: the prefill path.
 *   5. "linear_fp8w_generic": one thread per output, any shape, leading
 *      dimension and alignment.
 *   The SwiGLU kernels report "<name><swiglu>".
 * Workspace: pli_linear_fp8w_workspace_size is 0 for m <= 16 and for
 *   m <= 128 with k % 256 == 0 and n % 16 == 0 (a fast route takes aligned
 *   operands), else n * k * 2 rounded up to 16 bytes; twice that for SwiGLU.
 *   Caller-owned, 16-byte aligned scratch; nothing persists between calls.
 *   Without one (NULL) such a shape takes the generic kernel.
 * pli_gemv_fp8w: y[m] = w8[m, k] x, pli_linear_fp8w with one X row and no
 *   bias on the same kernel, bitwise equal to it.
 * PLI_EINVAL before any HIP call: a dtype other than fp16 / bf16, a negative
 *   shape, a leading dimension below its width, a NULL operand of a
 *   non-empty call, a misaligned or short workspace when route 4 would be
 *   taken.  m == 0 or n == 0 returns PLI_OK and the operands may be NULL;
 *   k == 0 writes bias or 0 and reads neither x nor the weights.  Nothing
 *   is allocated or synchronised. */
int pli_gemv_fp8w(const void* w8, const float* w_scale, const void* x, void* y,
                  int m, int k, int64_t ldw, int dtype, void* stream);
size_t pli_linear_fp8w_workspace_size(int m, int n, int k, int dtype);
int pli_linear_fp8w(const void* x, const void* w8, const float* w_scale,
                    const void* bias, void* c, int m, int n, int k,
                    int64_t ldx, int64_t ldw, int64_t ldc, int dtype,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t pli_linear_swiglu_fp8w_workspace_size(int m, int n, int k, int dtype);
int pli_linear_swiglu_fp8w(const void* x, const void* wg8,
                           const float* wg_scale, const void* wu8,
                           const float* wu_scale, void* h, int m, int n, int k,
                           int64_t ldx, int64_t ldwg, int64_t ldwu,
                           int64_t ldh, int dtype, void* workspace,
                           size_t workspace_bytes, void* stream);
/* pli_rms_gemm_nt_fp8w: pli_rms_gemm_nt over fp8 weights -- a decode-step
 * RMSNorm fused into the W8A16 projection that consumes it, one launch
 * (kernel "rms_gemm_fp8w": the norm phase of pli_rms_gemm_nt in front of the
 * dot phase of "linear_fp8w_vec").
 * Norm, groups, row offsets, capacity and h_out are pli_rms_gemm_nt's: rows
 *   h = a (+ residual) (written to h_out if not NULL, once), y = h *
 *   rsqrt(mean(h^2) + eps) * norm_weight -- bitwise the row pli_rmsnorm writes
 *   -- kept on chip; 1..3 groups share y, group g stores row r = b *
 *   tokens_per_batch + s of its n_g columns at
 *     c_g + b * stride_batch_g + (s + *row_offset_g) * stride_token_g (+ col),
 *   row_offset_g a device int32 or NULL (= 0); rows >= capacity_g are dropped.
 *   Group widths are arbitrary (a wave's rows may straddle two groups).
 *   h_out must not overlap a or residual: every workgroup reads both while
 *   workgroup 0 writes h_out (the same holds for pli_rms_gemm_nt), and no
 *   output may overlap an input.
 * Codes and scales are pli_linear_fp8w's: w8[g] [n_g, k] e4m3fn codes, leading
 *   dimension ldw_g bytes; w_scale[g] device fp32 [n_g], read on the device.
 *   w_scale (the array) or any one entry may be NULL: all ones.  Column j of
 *   group g is round_T( w_scale_g[j] * sum_i decode(w8_g[j, i]) * y[r, i] ),
 *   the sum in fp32 with the v_dot2 MACs, chunk order and accumulate order of
 *   "linear_fp8w_vec", so for m <= 4 the result is bitwise pli_rmsnorm followed
 *   by pli_linear_fp8w (pli_linear_swiglu_fp8w) on its vec route.  A NaN code
 *   makes exactly its output column NaN (in all m rows).
 * wu8 non-NULL: every group is SwiGLU, silu(w_scale_g[j] sum g) *
 *   (wu_scale_g[j] sum u), wu8[g] with the same ldw_g; wu_scale as w_scale.
 * PLI_EINVAL with a message, before any HIP call, unless: 1 <= m <= 4 rows in
 *   whole batches of tokens_per_batch; k > 0, k % 16 == 0, k <= 8192;
 *   lda / ldr / ldh >= k and % 8 == 0; ldw_g >= k and % 16 == 0; a, residual,
 *   h_out, norm_weight, w8_g and wu8_g 16-byte aligned; 1..3 groups, n_g > 0;
 *   dtype bf16 or fp16; eps finite and >= 0; a, norm_weight, the arrays
 *   w8 / c / n / ldw / stride_batch / stride_token / row_offset / capacity
 *   and every w8_g, c_g (wu8_g with wu8) non-NULL.
 * A workgroup holds the m normalised rows in m * k * 2 + 16 bytes of LDS: 65552
 *   at the largest shape (m = 4, k = 8192), inside the 163840 bytes a gfx950
 *   workgroup may use, so every shape these rules accept is launched.  No
 *   workspace; nothing is allocated or synchronised; the call replays in a
 *   captured graph while codes, scales and *row_offset_g change in place.
 *   pli_last_route: "rms_gemm_fp8w" or "rms_gemm_fp8w<swiglu>". */
int pli_rms_gemm_nt_fp8w(const void* a, int64_t lda, const void* residual, int64_t ldr,
                         const void* norm_weight, float eps, void* h_out, int64_t ldh,
                         int m, int k, int tokens_per_batch,
                         const void* const* w8, const float* const* w_scale,
                         const void* const* wu8, const float* const* wu_scale,
                         void* const* c, const int* n, const int64_t* ldw,
                         const int64_t* stride_batch, const int64_t* stride_token,
                         const int32_t* const* row_offset, const int* capacity,
                         int ngroups, int dtype, void* stream);

/* fp8 activations (W8A8): a row quantiser and an NT GEMM over two operands of
 * e4m3fn codes on the block-scaled matrix instruction of gfx950
 * (v_mfma_scale_f32_32x32x64_f8f6f4, e4m3 x e4m3 at twice the bf16 MFMA rate
 * per clock), for prefill and batches above the decode kernels' 16 rows.
 *
 * pli_quantize_rows_fp8: x [m, k] bf16 / fp16 (ldx in elements; PLI_F32 is
 *   refused) -> x8 [m, k] e4m3fn codes (ldx8 in bytes) and x_scale, device
 *   fp32 [m], both written by the call.  Per row, the rule of the Python
 *   quantize_weight_fp8: scale = absmax / 448 in fp32 (1.0 for a row with no
 *   non-zero finite element), inv = 1.0f / scale, code = e4m3fn(clamp(fp32(x)
 *   * inv, +-448)), round to nearest even; for finite rows codes and scales
 *   are bitwise that function's.  A device call cannot raise, so: a NaN
 *   element is skipped by the absmax and gets code 0x7F; +-inf is skipped by
 *   the absmax and gets the code of +-448 (0x7E / 0xFE).
 *   Kernel "quant_rows_fp8", one workgroup per row.  With k and ldx multiples
 *   of 8, ldx8 a multiple of 8, x 16-byte and x8 8-byte aligned a row of up to
 *   8192 elements is read once (held in registers between the absmax and the
 *   encode) and the rest of a longer one twice; any other call reads x twice.
 *   k == 0 writes scale 1.0 and no codes; m == 0 does nothing.
 * pli_gemm_fp8: C[r, j] = round_T( x_scale[r] * w_scale[j] *
 *   sum_i decode(x8[r, i]) * decode(w8[j, i])  (+ bias[j]) ).  x8 [m, k] and
 *   w8 [n, k] codes, leading dimensions ldx8 / ldw in bytes; T (dtype) is
 *   bf16 or fp16 and is the type of C (ldc in elements) and bias.  Either
 *   scale pointer may be NULL: all ones.  Both scales are device fp32, read
 *   on the device: a captured call replays while codes and scales change in
 *   place.  A code x code product has at most 8 significant bits and is exact
 *   in fp32; the sum is fp32; sum * (x_scale[r] * w_scale[j]) and the bias
 *   come after the sum and the result is rounded once.  A NaN code in x8
 *   makes exactly its row of C NaN, one in w8 exactly its column.  No
 *   workspace; nothing is allocated or synchronised.
 * Routes, in this order, from host arguments only (csrc/fp8a_plan.h;
 *   pli_last_route names the kernel):
 *   1. k == 0: C = bias or 0 ("gemm_fp8_generic"); m == 0 or n == 0: nothing.
 *   2. "gemm_fp8_mx": m >= 17, k % 128 == 0, x8 / w8 16-byte aligned, ldx8
 *      and ldw % 16 == 0, n and ldc % 4 == 0, c 8-byte aligned.  128 x 128
 *      tile, codes staged by 16-byte LDS-DMA into a swizzled two-stage LDS
 *      image, K-step 128, both E8M0 block scales at 2^0; ragged m / n edges
 *      by clamped loads and masked stores.  The order in which the
 *      instruction sums its 64 products is its own, so this route agrees with
 *      route 3 to fp32 rounding, and bitwise only where every partial sum is
 *      exact.
 *   3. "gemm_fp8_generic": one thread per output, fp32 fma in k order, any
 *      shape, leading dimension and alignment.
 * PLI_EINVAL before any HIP call, in this order: a dtype other than fp16 /
 *   bf16, a negative shape, a leading dimension below its width, a NULL
 *   operand of a non-empty call (x_scale of the quantiser included; the
 *   GEMM's scales and bias may be NULL), a grid too large. */
int pli_quantize_rows_fp8(const void* x, int64_t ldx, void* x8, int64_t ldx8,
                          float* x_scale, int m, int k, int dtype, void* stream);
int pli_gemm_fp8(const void* x8, const float* x_scale, const void* w8,
                 const float* w_scale, const void* bias, void* c, int m, int n,
                 int k, int64_t ldx8, int64_t ldw, int64_t ldc, int dtype,
                 void* stream);

/* Next-token sampling on the device: temperature, top-k, top-p and the draw of
 * ch02/generation.py:23-31 (temperature, top-k, multinomial),
 * ch02/cached_generation.py:245,265 (temperature) and ch10/engine.py:96-115
 * (greedy at temperature 0, top-p, multinomial) in one launch, one workgroup
 * per row of `vocab` logits.  The rule, per row (DESIGN.md "Sampling" has it in
 * full; csrc/sample_plan.h is its host-replayable part):
 *   NaN counts as -inf and -0 as +0.  No logit above -inf: token -1.  With a
 *   +inf in the row the +inf logits weigh 1 and all others 0.  "Before" means
 *   larger value first, lower index first among equal values (comparisons on
 *   integer keys, never arithmetic).  temperature == 0: the first token
 *   (argmax, lowest index on ties); top_k, top_p and the uniform are ignored.
 *   Otherwise K1 = the first top_k tokens (top_k <= 0 or >= vocab: all),
 *   w_i = exp((x_i - max) / temperature), S1 = sum over K1; token i of K1 is
 *   kept iff the weight of the K1 tokens before it is <= top_p * S1 (the first
 *   always; top_p >= 1: all of K1); the draw walks the kept tokens in
 *   ascending index and takes the first whose running sum exceeds u * S2.
 *   Weights are held as integers, floor(w * 2^45): every sum is exact and
 *   order-free, so the same inputs give the same token on every call and
 *   every replay.
 * u: uniforms[row] (device fp32 [rows], each in [0, 1)) when uniforms is not
 *   NULL; else (r0 >> 8) * 2^-24, r0 the first word of Philox4x32-10 with key
 *   {seed & 0xffffffff, seed >> 32} and counter {(uint32)offset, row, 0, 0},
 *   offset = (offset_dev ? *offset_dev : 0) + offset_add.  offset_dev is read
 *   by the kernel: a captured call replays while it changes in place.
 * logits [rows, vocab] of dtype (fp32 / fp16 / bf16), leading dimension
 *   ld_logits >= vocab elements, any alignment.  tokens: int64, row r at
 *   tokens[r * ld_tokens], ld_tokens >= 1.  vocab <= 262144 (2^18 weights of
 *   at most 2^45 sum below 2^64); above it PLI_EUNSUPPORTED.
 * Workspace: pli_sample_workspace_size is 0 (the state is in LDS); workspace
 *   may be NULL, a non-NULL one must be 16-byte aligned.
 * PLI_EINVAL before any HIP call: rows < 0, vocab < 1, ld_logits < vocab,
 *   ld_tokens < 1, a bad dtype, a negative or NaN temperature or top_p, a
 *   misaligned workspace, NULL logits or tokens when rows > 0.  rows == 0 does
 *   nothing and returns PLI_OK.  Nothing is allocated or synchronised.
 * pli_last_route: "sample_greedy" (temperature == 0) or "sample_select". */
size_t pli_sample_workspace_size(int rows, int vocab, int dtype);
int pli_sample(const void* logits, int64_t ld_logits, int rows, int vocab, int dtype,
               float temperature, int top_k, float top_p, const float* uniforms,
               uint64_t seed, const int32_t* offset_dev, int64_t offset_add,
               int64_t* tokens, int64_t ld_tokens, void* workspace,
               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Tuning section: the same operations with an explicit kernel choice, for
 * A/B runs (tools/tune.py) and the per-variant parity tests.  Not part of
 * the drop-in surface above -- a caller that binds the reference's
 * interface never needs them.  variant / mode < 0 (or 0 where noted) is the
 * default route; every listed value is parity-tested at the bench sizes
 * (tests/test_gpu_fullsize.py) and on the small edge cases
 * (tests/test_gpu_parity.py, test_gpu_decode.py, test_gpu_moe.py,
 * test_gpu_swiglu.py).
 *
 * pli_flash_attn_fwd_variant: 21 attn_fwd_v2 (round-1 kernel), 50 / 51
 *   attn_fwd_v7 prescaled / exact, 54 / 55 attn_fwd_v10 prescaled / exact,
 *   60 attn_fwd_v10 exact in 4-wave workgroups, 70 / 71 attn_fwd_v12 (one
 *   wave per SIMD, 64 rows per wave; 71 persistent, bitwise equal to 55;
 *   other inputs take 55); 72 = 71 with the defer-max threshold at 0
 *   (tests); 73 / 74 attn_fwd_v12 causal, one block per workgroup /
 *   persistent pair walk; 80 / 81 / 82 attn_fwd_v13 (16x16x32 MFMA, one
 *   generated instruction stream) persistent / one block per workgroup /
 *   80 with the rescale path at every tile (tests) -- 80 is the default
 *   for bf16 and fp16 (attn_fwd_v13h, the f16 MFMA) D = 128 / 64 with Nk a
 *   multiple of 64 from 128, or any Nk > 64 (attn_fwd_v13r / v13hr: the last
 *   key tile fetched from key Nk - 64, its overlap masked in P); 83 / 84 /
 *   85 the causal forms (83 = causal default for any Nq <= Nk and Nk > 64,
 *   ragged Nk on attn_fwd_v13rc / v13hrc; other shapes take 74 / 60);
 *   86 / 87 attn_fwd_pp64 / pp64h (head dim 64, two waves per SIMD,
 *   512-row blocks; causal: pp64c / pp64hc with Nq and Nk - Nq multiples
 *   of 64) / the same with the rescale path at every tile, other shapes
 *   take 80 / 83 (82 / 85); 88 (the default since round 6) = 86 for
 *   non-causal D = 64 where B H ceil(Nq / 512) fills the CUs, else 80 /
 *   83.  Prescaled variants round Q * scale * log2(e) to
 *   the 16-bit input type (2^-9 relative score error in bf16).  The v13
 *   forms, v12 and the exact v7 / v10 bodies (51 / 55 / 60) take any
 *   scale > 0; the prescaled 50 / 54 take scale * log2(e) <= 1 (larger
 *   scales fall back to 21).
 * pli_gemm_w5 schedule (all gemm_w5 routes): W5_SPLIT, DMA spread over both
 *   halves of each 64-deep K step (gemm_w5.hip).
 * pli_gemm_variant / pli_gemm_ws_variant: 0 default; 1 128^2 tile; 2 256^2
 *   one-phase; 3 phased SCHED 0; 4 one-phase + setprio; 5-8 phased SCHED
 *   1/3/5/7; 9-11 grouped one-phase (group_m 4/8/16); 12-15 grouped phased
 *   (8/4/2/16); 20 mid-M; 21 small-M; 22/24 direct-load split-K; 25-29 LDS
 *   split-K (256/512/128 targets, 3-deep ring); 40 gemm_w4v (one wave per
 *   SIMD, K 32 deep); 41 gemm_w5 (K 64 deep), 43 gemm_w5 persistent walk
 *   (M, N multiples of 256) -- 43 is the large-shape default (K >= 128).
 * pli_gemv_variant: 0-16 (rows per wave x 16-B chunks per lane x waves per
 *   block, gemv.hip), -1 default.
 * pli_attn_decode_variant: mode -1 default, 2/9/11/13 load-layout modes
 *   (decode_attn.hip); target_wgs 0 = automatic split.
 * pli_gemm_swiglu_ws_variant: 0 default, 1 split K wherever the split-K
 *   route applies, 2 never split, 3 gemm_w5's SwiGLU tile (the prefill
 *   default), 4 the phased 256 x 128 tile (3 and 4 never split).
 * pli_gemm_grouped_variant: 0 default, 1/2 alternate routes (gemm.hip
 *   grouped_dispatch); 2, the LDS-staged kernel wherever it applies, is an
 *   argument error with more than 65535 experts.
 */
int pli_flash_attn_fwd_variant(const void* q, const void* k, const void* v, void* o, int batch,
                               int heads, int kv_heads, int n_q, int n_kv, int head_dim,
                               const int64_t* strides, float scale, int causal, int dtype,
                               void* stream, int variant);
int pli_gemm_variant(const void* a, const void* b, void* c, const void* bias, int m, int n, int k,
                     int64_t lda, int64_t ldb, int64_t ldc, int trans_b, int dtype, void* stream,
                     int variant);
int pli_gemm_ws_variant(const void* a, const void* b, void* c, const void* bias, int m, int n,
                        int k, int64_t lda, int64_t ldb, int64_t ldc, int trans_b, int dtype,
                        void* workspace, size_t workspace_bytes, void* stream, int variant);
int pli_gemv_variant(const void* w, const void* x, void* y, int m, int k, int64_t ldw, int dtype,
                     void* stream, int variant);
int pli_attn_decode_variant(const void* q, const void* k, const void* v, void* o, int batch,
                            int heads, int kv_heads, int n_q, int n_kv, int head_dim,
                            const int64_t* strides, float scale, int causal, void* workspace,
                            size_t workspace_bytes, int dtype, void* stream, int mode,
                            int target_wgs);
int pli_gemm_swiglu_ws_variant(const void* x, const void* wg, const void* wu, void* h, int m, int n,
                               int k, int64_t ldx, int64_t ldwg, int64_t ldwu, int64_t ldh,
                               int dtype, void* workspace, size_t workspace_bytes, void* stream,
                               int variant);
int pli_gemm_grouped_variant(const void* x, const int32_t* gather, const void* const* w_ptrs,
                             const void* const* wu_ptrs, void* c, const int32_t* offsets,
                             int experts, int rows_bound, int n, int k, int64_t ldx, int64_t ldw,
                             int64_t ldc, int dtype, void* stream, int variant);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* PLI_H */
