/* ppf_hip.h -- C ABI of the MI355X (gfx950) ProtoPFormer hot-path library (protopformer_amd/lib/libppf_hip.so).
 *
 * The reference (zju-vipa/ProtoPFormer) has no native/FFI layer: its hot path is Python calling ATen.  This header is
 * the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md): one entry point per fused operation, each
 * citing the reference lines it replaces (paths relative to the reference repo; deit = tools/deit_models_attn.py,
 * cait = tools/cait_models_attn.py).
 *
 * Conventions
 *   - plain C: raw device pointers + explicit sizes/strides; no torch types.  "bf16" buffers are uint16_t storage.
 *   - every function enqueues work on `stream` and returns immediately (asynchronous w.r.t. the host).
 *   - the caller owns all memory; the library keeps no pointers after return and allocates nothing persistent.
 *   - return 0 on success, <0 for invalid shape/alignment/argument (PPF_ERR_*), >0 = hipError_t of a failed launch;
 *     ppf_last_error() returns a thread-local message.  No exceptions cross the boundary.
 *   - one host thread per process drives one GPU (data parallel = one process per GPU); re-entrant across streams.
 */
#ifndef PPF_HIP_H
#define PPF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ppf_stream_t; /* == hipStream_t */

#define PPF_ERR_SHAPE (-1)
#define PPF_ERR_ALIGN (-2)
#define PPF_ERR_ARG (-3)

/* Bumped whenever an entry point changes its parameter list or meaning.  ppf_abi_version() returns the value the library was built
 * with; the binding (protopformer_amd/_lib.py EXPECTED_ABI) refuses a library of another version instead of shifting arguments. */
#define PPF_ABI_VERSION 10

/* ---- runtime ------------------------------------------------------------------------------------------------- */
const char* ppf_last_error(void);
int ppf_abi_version(void);
int ppf_device_info(int* cu_count, int* clock_mhz, char* name, int name_len);
/* stream ordering for the two-lane schedule of the host mirror (weight gradients / head-mean maps / prototype gradients on a side
 * stream): pooled, timing-disabled events inside the library; one call per dependency.
 * wait_stream: everything on src so far happens-before later work on dst.  mark / wait_mark: a ticket for "src so far".
 * arm (round 6): while a stream is armed (on = 1) every kernel the library launches on it carries its own completion event
 * (hipExtLaunchKernel stop event), and the next wait_stream(dst, stream) waits for the last of them instead of recording an event --
 * no packet enters the producer's queue.  Armed by the replay loop around the one library call that precedes a wait. */
int ppf_stream_arm(ppf_stream_t stream, int on);
int ppf_stream_wait_stream(ppf_stream_t dst, ppf_stream_t src);
int64_t ppf_stream_mark(ppf_stream_t stream);
int ppf_stream_wait_mark(ppf_stream_t stream, int64_t ticket);

/* ---- dense bf16 MFMA GEMM family: every nn.Linear / 1x1 conv / PatchEmbed conv of the path ----------------------
 * C[m][n] (+)= epi( sum_kc A(m,kc) * B(n,kc) ), fp32 accumulate.
 *   trans_a = 0: A[m*lda + kc]      trans_a = 1: A[kc*lda + m]        (same for B with ldb / n)
 *   forward  y = x W^T + b                (0,0)  deit:47,58 (qkv, proj), timm Mlp fc1/fc2 (deit:80), PatchEmbed (deit:174),
 *                                                add_on_layers 1x1 conv (protopformer.py:111-114,171-172)
 *   dgrad    dx = dy W                    (0,1)  autograd of the above
 *   wgrad    dW += dy^T x (+ db)          (1,1)  split over kc, fp32 atomics into C, colsum[m] += sum_kc A(m,kc)
 * epi: 0 bf16 out | 1 f32 out | 2 bias+GELU(erf): C=gelu(pre) bf16, aux_out=gelu'(pre) as ONE BYTE per element (saved for backward:
 *        code q = rint(196 d + 26), d' = (q - 26) / 196: 0 and 1 are code points, |error| <= 2.55e-3) | 3 sigmoid f32 out |
 *      4 residual: C f32 = res + rowscale[m/rows_per_group]*colscale[n]*(acc+bias)  (DropPath deit:79-80, LayerScale
 *        cait:156-157), optional aux_out = raw branch output bf16 | 5 dGELU: C bf16 = acc * aux_in (aux_in = the gelu' codes of epi 2) | 6 atomic f32.
 * ldaux counts ELEMENTS of the aux tensor (bytes for epi 2 / 5, bf16 for epi 4). */
int ppf_gemm_bf16(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int trans_a,
                  int trans_b, int epi, const float* bias, const float* res, int ldres, const float* rowscale,
                  int rows_per_group, const float* colscale, const void* aux_in, void* aux_out, int ldaux, float* colsum,
                  float alpha, void* workspace, size_t workspace_bytes, ppf_stream_t stream);
/* split-K scratch an accumulating (epi 6) GEMM of this shape wants (deterministic ordered reduction instead of atomics).  Contract: the
 * workspace is handed to ppf_gemm_bf16 calls of ONE stream only (every weight gradient recycles it: the 28 MB of partial tiles live and die
 * in the L2 / memory-side cache); its first 16 KiB are a reserved prefix (the arrival counters of round 3's in-kernel reduce, deleted). */
size_t ppf_gemm_workspace_bytes(int M, int N, int K);

/* Test hook (tests/test_gpu_gemm.py): force = 1 sends every shape the 224 x 128 NT kernel can legally take to it, 0 = the cost model. */
int ppf_gemm_test_force_g224(int force);
/* Test hook (tests/test_gpu_wgrad_dma.py): data path of the eight-wave weight-gradient kernel behind epi 6 with a workspace.  path = 0 the
 * dispatch as shipped, 1 register-staged for every shape, 2 LDS-DMA for every shape it can take (K % 64 == 0; others stay register-staged).
 * Both paths produce the same bits. */
int ppf_gemm_test_wgrad_path(int path);
/* Test hook (tests/test_gpu_gemm_paths.py): the kernel the last ppf_gemm_bf16 call launched, recorded on the host in front of the launch:
 * 0 none yet | 1 gemm_kernel NT | 2 gemm_kernel NN | 3 gemm_kernel TT f32 | 4 gemm_kernel TT atomic | 5 gemm_kernel TT partial + reduce |
 * 6 gemm128g | 7 gemm224g | 8 wgrad8<4,2> register-staged | 9 wgrad8<4,2> DMA | 10 wgrad8<2,4> register-staged | 11 wgrad8<2,4> DMA.
 * Not thread-safe; tests only. */
int ppf_gemm_test_last_kernel(void);

/* Roofline probe of the split-K weight-gradient kernel (epi 6 with a workspace): HIP events (from a reused pool) on the launch
 * stream around the kernel itself.  ppf_gemm_probe(1) clears and starts, (0) stops, (2) stops and destroys the pool;
 * ppf_gemm_probe_read synchronises the events and returns the summed kernel time, the launch count and the algorithmic
 * flops / bytes of those launches (bench.py's `roofline`).  Enabled while a step is being captured into a HIP graph, the records
 * become event-record nodes: a read after replays returns the last replay's durations. */
int ppf_gemm_probe(int enable);
int ppf_gemm_probe_read(double* ms_total, int64_t* launches, double* flops, double* bytes);

/* Path probe (round 5): the same mechanism around the kernels BASELINE.json's north_star names -- tag 0 attention forward
 * (ppf_attn_fwd / ppf_attn_fwd_hm), 1 attention backward (ppf_attn_bwd), 2 prototype forward (ppf_proto_fwd) -- for bench.py's
 * roofline.named_path.  ppf_path_probe(1) clears and starts, (0) stops, (2) stops and destroys the pools; ppf_path_probe_read
 * returns the summed in-step kernel time, the launch count and the algorithmic flops / bytes of the recorded launches.
 * Single-threaded and eager-only: launches into a capturing stream are not recorded, and at most 4096 launches per tag are kept. */
int ppf_path_probe(int enable);
int ppf_path_probe_read(int tag, double* ms_total, int64_t* launches, double* flops, double* bytes);

/* ---- fp32 verification mode, backward (csrc/precise.hip, round 5; DeiT): never on the measured path -----------------------------
 * LayerNorm backward with the statistics recomputed from x (rows of dy <-> rows row_map[r] of x, dx_out written at the x rows -- dx_out may
 * alias dres_in; dw / db by fp32 atomics, either may be NULL for a frozen LayerNorm); elementwise pieces (kind 0 x gelu'(pre), 1 sigmoid', 2 DropPath row scale, 3 product, 4 row scale x LayerScale column, 5 ReLU' from its output); column sums; Attention backward with the
 * policy softmax of deit:29-43 (scratch: B*H*2*N*N floats). */
int ppf_layernorm_bwd_f32(const float* dy, const float* x, const int* row_map, const float* w, const float* dres_in, float* dx_out, float* dw, float* db,
                          int rows, int D, float eps, ppf_stream_t stream);
int ppf_ew_bwd_f32(int kind, const float* a, const float* b, float* out, const float* rowscale, int rows_per_group, int M, int N, ppf_stream_t stream);
int ppf_colsum_f32(const float* in, float* out, int M, int N, ppf_stream_t stream);
int ppf_attn_bwd_f32(const float* qkv, const float* dout, const float* policy, float* dqkv, float* scratch, int B, int H, int N, int D, int self_keep,
                     int eps_n, ppf_stream_t stream);
/* CaiT: TalkingHeadAttn backward (cait:115-132; dqkv zero-filled by the caller, mixer gradients accumulate) and ClassAttn backward (cait:50-90) */
int ppf_th_attn_bwd_f32(const float* qkv, const float* dout, const float* wl, const float* bl, const float* ww, const float* bw, float* dqkv,
                        float* dwl, float* dbl, float* dww, float* dbw, int B, int H, int N, int D, ppf_stream_t stream);
int ppf_class_attn_bwd_f32(const float* q, const float* k, const float* v, const float* policy, const float* dout, float* dq, float* dk, float* dv,
                           int B, int H, int N1, int D, ppf_stream_t stream);

/* ---- full-row GEMM with row-wise fused epilogues (csrc/rowgemm.hip) ------------------------------------------------------------
 * acc = A[M][K] . B[D][K]^T with D = the model width (192 or 384): a workgroup owns complete output rows (tiles of rows_per_tile <=
 * 208 rows, the host passes the tokens of one sample), so what the reference does next to those rows runs in the epilogue and the
 * GEMM output / the separate LayerNorm pass never touch HBM.  Both operands contraction-contiguous, bf16; K % 32 == 0.
 *   ppf_rowgemm_bf16      out bf16 = acc + bias                                   input gradient of attn.proj (autograd of deit:58)
 *   ppf_rowgemm_resid_ln  xout = res + rowscale[m / rows_per_group] * colscale[n] * (acc + bias) (fp32, may alias res):
 *                         `x = x + drop_path(attn(...))` / `x = x + drop_path(mlp(...))` (deit:79-80, timm DropPath); colscale = CaiT's
 *                         LayerScale gamma_1 / gamma_2 (cait:153-155) or NULL, aux_out (optional) = bf16(acc + bias), the unscaled
 *                         branch its gradient needs; ln_out = bf16(LN(xout)), mean, rstd = the
 *                         LayerNorm that follows (deit:79 norm2 / the next block's norm1, eps 1e-6); ln_out == NULL: residual only
 *   ppf_rowgemm_lnbwd     dn = acc: gradient w.r.t. a LayerNorm output (input of qkv / fc1, deit:47 / timm Mlp fc1);
 *                         dx_out = dres_in + LN'(dn; x, mean, rstd, w) (fp32, may alias dres_in; NULL = 0);
 *                         cast_out = bf16(rowscale[m / rows_per_group] * dx_out) = the gradient entering the residual branch below
 *                         (optional); partial[tiles][2][D] = per-tile column sums (d ln weight, d ln bias), summed in a fixed order
 *                         by ppf_rowgemm_colsum (may run on another stream).  colscale != NULL = CaiT's LayerScale on the branch
 *                         below (cait:153-155): cast_out = bf16(rowscale * colscale[n] * dx_out), branch = the bf16 unscaled branch
 *                         output saved by ppf_rowgemm_resid_ln's aux_out, partial[tiles][3][D] with d gamma's sums third. */
int ppf_rowgemm_supported(int D, int K, int rows_per_tile);
int ppf_rowgemm_bf16(const void* A, const void* B, int M, int D, int K, int lda, int ldb, int rows_per_tile, const float* bias, void* out,
                     ppf_stream_t stream);
int ppf_rowgemm_resid_ln(const void* A, const void* B, int M, int D, int K, int lda, int ldb, int rows_per_tile, const float* bias,
                         const float* res, float* xout, const float* rowscale, int rows_per_group, const float* colscale, void* aux_out,
                         const float* ln_w, const float* ln_b, void* ln_out, float* ln_mean, float* ln_rstd, float eps, ppf_stream_t stream);
int ppf_rowgemm_lnbwd(const void* A, const void* B, int M, int D, int K, int lda, int ldb, int rows_per_tile, const float* x, const float* mean,
                      const float* rstd, const float* w, const float* dres_in, float* dx_out, void* cast_out, const float* rowscale,
                      int rows_per_group, const float* colscale, const void* branch, float* partial, size_t partial_bytes, ppf_stream_t stream);
int ppf_rowgemm_colsum(const float* partial, int tiles, int D, int nparts, float* dw, float* db, float* dg, ppf_stream_t stream);
/* Transposed bf16 copies of n weight matrices in one launch (the input-gradient products read W^T contraction-contiguous):
 * desc (device, int64 [n][4]) = (source element offset, destination element offset, rows, cols) into src / dst; dst[c][r] = src[r][c].
 * total_tiles = sum over the matrices of ceil(rows / 64) * ceil(cols / 64). */
int ppf_transpose_bf16_batched(const void* src, void* dst, const void* desc_i64, int n, int total_tiles, ppf_stream_t stream);

/* ---- LayerNorm (deit:67,72,238 norm1/norm2/norm, eps 1e-6) ----------------------------------------------------
 * fwd: y bf16 [rows][D] = LN(x fp32 [row_map ? row_map[r] : r][D]); saves mean / rstd per output row.
 * bwd: dx_out[src] = dres_in[src] + LN'(dy); dw/db accumulate.  Optional fused pass for the residual branch below:
 *      cast_out = bf16(rowscale*colscale*dx_out), dbias_next += its column sums, dcolscale += sum(rowscale*dx_out*branch).
 *      dy == NULL: only the fused pass over dres_in. */
int ppf_layernorm_fwd(const float* x, const int* row_map, const float* w, const float* b, void* y, float* mean, float* rstd,
                      int rows, int D, float eps, ppf_stream_t stream);
int ppf_layernorm_bwd(const void* dy, const float* x, const int* row_map, const float* w, const float* mean, const float* rstd,
                      const float* dres_in, float* dx_out, float* dw, float* db, void* cast_out, const float* rowscale,
                      int rows_per_group, const float* colscale, float* dbias_next, const void* branch, float* dcolscale,
                      int rows, int D, float* partial, size_t partial_bytes, ppf_stream_t stream);
/* partial != NULL: the column sums (dw, db, dbias_next, dcolscale) are NOT accumulated by ppf_layernorm_bwd; each workgroup
 * writes its partial sums into partial[ppf_layernorm_bwd_blocks(rows)][4][D] (the last rows are second-level scratch) and ppf_layernorm_bwd_reduce adds them up in a
 * fixed order (deterministic, no float atomics; may run on another stream).  partial == NULL: fp32 atomics. */
int ppf_layernorm_bwd_blocks(int rows);
int ppf_layernorm_bwd_reduce(const float* partial, int rows, int D, float* dw, float* db, float* dbias_next, float* dcolscale,
                             ppf_stream_t stream);
/* Test hook (tests/test_gpu_ln_bwd_lean.py): form of the half-wave-per-row backward kernel behind ppf_layernorm_bwd.  path = 0 the dispatch
 * as shipped, 1 the parent form (111 VGPRs at D = 384) for every width, 2 the register-lean form (at most 96 VGPRs: two waves per SIMD beside
 * a resident weight-gradient workgroup) wherever it is instantiated: D = 384 without LayerScale operands; every other case keeps the parent
 * form.  Both forms produce the same bits. */
int ppf_layernorm_test_bwd_path(int path);

/* ---- attention with the policy softmax (deit:29-60; class attention cait:50-90 with self_keep = 0) -------------
 * qkv bf16 [B*N][3D] packed q|k|v, head h at columns h*hd.  policy [B][N] in {0,1} or NULL.
 * fwd saves rowmax and 1/(sum+eps) [B][H][N]; headmean = mean over heads of the probabilities, [B][N][NP] fp32
 * (the rollout input, deit:104 `attn.mean(axis=1)`), recomputed from those statistics.
 * eps_n: the N of the softmax's +eps/N term (deit:42); 0 = N.  Blocks that run on the reserved tokens only (compacted after the
 * rollout) pass the original token count so that the kept entries equal the masked full-length computation. */
int ppf_attn_fwd(const void* qkv, void* out, const float* policy, float* rowmax, float* zinv, int B, int H, int N, int D,
                 int self_keep, int eps_n, ppf_stream_t stream);
/* forward pass + head-mean map in ONE launch (16-row tiles: Q.K^T is computed once, N = 197 runs as 13 x 16 = 208 rows): headmean may be
 * NULL (no map).  ppf_attn_fwd_hm_supported: 1 for head_dim 64 and N <= 208, else use ppf_attn_fwd + ppf_attn_headmean. */
int ppf_attn_fwd_hm_supported(int H, int N, int D);
int ppf_attn_fwd_hm(const void* qkv, void* out, const float* policy, float* rowmax, float* zinv, float* headmean, int NP, int B, int H, int N,
                    int D, int self_keep, int eps_n, ppf_stream_t stream);
int ppf_attn_headmean(const void* qkv, const float* policy, const float* rowmax, const float* zinv, float* headmean, int NP,
                      int B, int H, int N, int D, int self_keep, int eps_n, ppf_stream_t stream);
int ppf_attn_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, const float* policy, const float* rowmax,
                 const float* zinv, float* delta, int B, int H, int N, int D, int self_keep, int eps_n, ppf_stream_t stream);

/* ---- CaiT: talking-heads self-attention (cait:93-132) and class attention (cait:34-90) --------------------------------
 * Talking heads (cait:119-128) is one fused path: no (B,H,N,N) fp32 tensor is materialised and no float atomics are used.  A shape
 * outside its cover is an error (PPF_ERR_SHAPE); there is no other route.  ppf_th_fused_supported: 1 when (heads, tokens, width) is
 * covered (head_dim in {32,48,64}, heads in {2,4}, N <= 224, K and V images of all heads within the 160 KiB LDS), else 0.
 * ppf_th_fwd: a16 = bf16 proj_w(softmax(proj_l(scale q k^T))) [B][H][N][NPK], hm = its head mean [B][N][NP] (rollout input, cait:228),
 * rowmax / zinv [B][H][N] = softmax statistics of the mixed logits (saved for backward); out (optional) = the attention output A V,
 * bf16 [B*N][D] (cait:128).  Paddings: N <= NP <= NPK <= 32 ceil(N / 32), NP % 4 == 0, NPK % 8 == 0 -- the kernel zeroes pad columns only up to
 * the last 32-key trip it visits, so a wider a16 / hm is refused (PPF_ERR_SHAPE), not left partly unwritten.  Every pointer but out must
 * be non-null (PPF_ERR_ARG).
 * ppf_th_bwd: ds16 = bf16 dS [B][H][N][NPK] from dout = dO [B*N][D]; partial (>= ppf_th_bwd_partial_floats floats) receives one row of
 * parameter-gradient sums per workgroup; N <= NPK <= 16 ceil(N / 16), NPK % 8 == 0 (pad columns are zeroed up to the last 16-key tile; a
 * wider ds16 is refused); no pointer may be null (PPF_ERR_ARG).  ppf_th_param_reduce adds their fixed-order (bit-reproducible) totals to
 * dww, dbw, dbl, dwl (none may be null). */
int ppf_th_fused_supported(int H, int N, int D);
int ppf_th_fwd(const void* qkv, const float* wl, const float* bl, const float* ww, const float* bw, void* a16, float* hm, float* rowmax,
               float* zinv, void* out, int B, int H, int N, int D, int NP, int NPK, ppf_stream_t stream);
size_t ppf_th_bwd_partial_floats(int B, int H, int N);
int ppf_th_bwd(const void* qkv, const void* dout, const float* wl, const float* bl, const float* ww, const float* rowmax, const float* zinv,
               void* ds16, float* partial, int B, int H, int N, int D, int NPK, ppf_stream_t stream);
int ppf_th_param_reduce(const float* partial, int B, int H, int N, float* dww, float* dbw, float* dbl, float* dwl, ppf_stream_t stream);
/* the three per-head products behind ppf_th_bwd in one launch: dqkv [B*N][3D] bf16 <- dQ_h = scale dS_h K_h | dK_h = scale dS_h^T Q_h |
 * dV_h = A_h^T dO_h from ds16 / a16 [B][H][N][NPK], packed qkv and dout [B*N][D] (ppf_th_grads_supported: N <= 208, head_dim 32/48/64;
 * any head count H >= 1 with D % H == 0 is accepted: one workgroup per (sample, head); NPK must be N rounded up to 8;
 * a shape it does not cover cannot be trained) */
int ppf_th_grads_supported(int H, int N, int D);
int ppf_th_grads(const void* qkv, const void* dout, const void* ds16, const void* a16, void* dqkv, int B, int H, int N, int D, int NPK,
                 ppf_stream_t stream);
/* class attention: q [B][D] (cls rows, unscaled), k/v [B*N1][D] bf16; policy softmax WITHOUT the identity term (cait:58-59);
 * 1 <= H <= 4, 1 <= N1 <= 256, head_dim even and <= 64 (else PPF_ERR_SHAPE); every pointer but policy must be non-null (PPF_ERR_ARG) */
int ppf_class_attn_fwd(const void* q, const void* k, const void* v, const float* policy, float* attn, float* zinv, float* rowmean,
                       void* out, int B, int H, int N1, int D, ppf_stream_t stream);
int ppf_class_attn_bwd(const void* q, const void* k, const void* v, const float* attn, const float* zinv, const void* dout, void* dq,
                       void* dk, void* dv, int B, int H, int N1, int D, ppf_stream_t stream);
/* out bf16 [rows][D] = a + b (+ cq[row / N1] where row % N1 == 0): input gradient of the class-attention q/k/v projections */
int ppf_merge3_cast(const float* a, const float* b, const float* cq, void* out, int rows, int D, int N1, ppf_stream_t stream);

/* ---- attention rollout + token reservation (deit:99-124, 223-234; cait:223-261, 328-339) ------------------------
 * hm [L][B][N][NP] head-mean attention of the rollout layers; kdrop = int(N*N*0.9), kdrop_init = int((N+1)*0.9).
 * lead = 1 (DeiT): row 0 of a_{L-1}..a_0, outputs skip the cls column; lead = 0 (CaiT): init_rows [n_init][B][N+1] are the
 * class-attention rows.  Outputs: cls_attn [B][N-lead], idx [B][k] int32 ascending (topk + sort), policy [B][N-lead+1].
 * thr_u32 (optional) [L][B]: the per (layer, sample) discard thresholds from ppf_rollout_threshold -- the exact order statistic
 * "int(N*N*0.9)-th smallest entry" (deit:108-112) does not depend on the chain, so it can be taken per layer as soon as that layer's
 * head-mean map exists (off the critical path); NULL: selected inside ppf_rollout. */
int ppf_rollout_threshold(const float* hm_layer, int B, int N, int NP, int kdrop, void* thr_out_u32, ppf_stream_t stream);
int ppf_rollout(const float* hm, int64_t layer_stride, int L, int B, int N, int NP, const float* init_rows, int n_init, int lead,
                int kdrop, int kdrop_init, float identity, int k, const void* thr_u32, float* cls_attn, int* idx, float* policy,
                ppf_stream_t stream);
/* topk(k) + ascending sort of indices on given scores [B][n] (protopformer.py:157-158, 273-274) */
int ppf_topk_sorted(const float* scores, int B, int n, int k, int* idx, ppf_stream_t stream);

/* ---- prototype layer (protopformer.py:201-247): squared L2 distances, log similarity, max-pool -------------------
 * sample b's token i is at tok + b*stride_b + (t0+i)*Dp (fp32); T tokens per sample (T == 1: global / cls branch).
 * act_kind 0: log((d+1)/(d+eps)), 1: -d.  Outputs act_max [B][P], argmax [B][P], optional dist_full/act_full [B][P][T]. */
int ppf_proto_fwd(const float* tok, int64_t stride_b, int t0, int T, const float* protos, int B, int P, int Dp, int act_kind,
                  float eps, float* act_max, int* argmax, float* dist_full, float* act_full, void* workspace, size_t workspace_bytes,
                  ppf_stream_t stream);
/* workspace: optional scratch of ppf_proto_fwd_workspace(P, Dp) bytes (any content, 16-byte aligned) -- the prototypes split ONCE per launch
 * into the bf16 piece planes the pooled kernel reads (NULL: every workgroup splits its own rows; same results to fp32 summation order). */
size_t ppf_proto_fwd_workspace(int P, int Dp);
int ppf_proto_bwd(const float* tok, int64_t stride_b, int t0, int T, const float* protos, int B, int P, int Dp, int act_kind,
                  float eps, const float* dist_full, int map_is_act, const float* g_full, const float* g_max, const int* argmax, float* dtok,
                  int64_t dstride_b, float* dprotos, void* zeroed_workspace, size_t workspace_bytes, ppf_stream_t stream);
/* map_is_act != 0: the [B][P][T] map passed as dist_full holds the ACTIVATIONS ppf_proto_fwd wrote (act_full), not the distances; the
 * derivative is then taken from them (a = log((d+1)/(d+eps)) => da/dd = -(e^a - 1)^2 / ((1 - eps) e^a), 0 at the clipped d == 0), so a
 * training forward writes one (B,P,T) map instead of two. */
/* workspace: ppf_proto_bwd_workspace() bytes = [bitmap of the non-zero dL/dd entries, B*T*ceil(P/32)*4 bytes rounded up to 256, present
 * and ZERO-FILLED by the caller when dtok != NULL][scratch of the prototype gradients when dprotos != NULL, any content].  A workspace
 * that only holds the bitmap is accepted: the prototype gradients then take the per-prototype gather kernel (same results to rounding). */
size_t ppf_proto_bwd_workspace(int B, int T, int P, int Dp, int want_dtok, int want_dprotos);
/* The same backward with the activation-map gradient in the block form get_PPC_loss produces (protopformer.py:259-288: only the ppc
 * prototypes of the sample's own class get a gradient): g_rows [B][ppc][T] = dL/d act_full[b][label[b]*ppc + k][t]; every other entry
 * of the (B,P,T) gradient is zero and is never materialised.  label_i64: int64 labels [B] (0 <= label*ppc <= P - ppc). */
int ppf_proto_bwd_rows(const float* tok, int64_t stride_b, int t0, int T, const float* protos, int B, int P, int Dp, int act_kind,
                       float eps, const float* dist_full, int map_is_act, const float* g_rows, const void* label_i64, int ppc, const float* g_max,
                       const int* argmax, float* dtok, int64_t dstride_b, float* dprotos, void* workspace, size_t workspace_bytes,
                       ppf_stream_t stream);
/* T == 1 (global branch, protopformer.py:295,311 and its autograd): dense form of the same backward -- two fp32 products instead of the
 * gather.  g [B][P] = upstream gradient of the activations, dist [B][P]; dtok rows are overwritten (when non-null), dprotos accumulated. */
size_t ppf_proto_bwd_single_workspace(int B, int P, int Dp);
int ppf_proto_bwd_single(const float* tok, int64_t stride_b, int t0, const float* protos, int B, int P, int Dp, int act_kind, float eps,
                         const float* dist, const float* g, float* dtok, int64_t dstride_b, float* dprotos, void* workspace,
                         size_t workspace_bytes, ppf_stream_t stream);

/* ---- losses and the frozen class-connection head ------------------------------------------------------------------
 * PPC loss (protopformer.py:249-288): loss[0] = cov term, loss[1] = mean term; gcov/gmean [B][ppc][T] analytic grads. */
int ppf_ppc_loss(const float* act, const int* idx, const void* label_i64, int B, int P, int T, int ppc, int side,
                 float cov_thresh, float mean_thresh, float* partial, float* gcov, float* gmean, float* loss, ppf_stream_t stream);
int ppf_ppc_loss_bwd(const float* gcov, const float* gmean, const float* up_cov, const float* up_mean, const void* label_i64,
                     float* g_full, int B, int P, int T, int ppc, ppf_stream_t stream);
/* nn.CrossEntropyLoss (main.py:390): mean loss + d/dlogits */
int ppf_cross_entropy(const float* logits, const void* label_i64, float* per_sample, float* dlogits, float* loss, int B, int C,
                      ppf_stream_t stream);
/* soft-target / label-smoothing cross-entropy (main.py:384-390; timm SoftTargetCrossEntropy / LabelSmoothingCrossEntropy, and
 * nn.CrossEntropyLoss given probability targets): loss = mean over the batch, dlogits [B][C] = d(loss)/d(logits); per_sample [B]
 * scratch.  Exactly one of the two target forms (device pointers), the other NULL:
 *   target [B][C] fp32 (dense):  loss_b = sum_c t_c (lse - x_c) = lse*sum(t) - sum(t*x),  dlogits = (softmax*sum(t) - t) / B
 *                                (sum(t) == 1 is not assumed, as in torch);
 *   label_i64 [B] + smoothing s: loss_b = (1-s)(lse - x_label) + s(lse - mean_c x),      dlogits = (softmax - (1-s) onehot - s/C) / B.
 * Row statistics in fp64, one wave per row, fixed-order batch mean: deterministic.  A label outside [0, C) reads nothing. */
int ppf_soft_cross_entropy(const float* logits, const float* target, const void* label_i64, float smoothing, float* per_sample,
                           float* dlogits, float* loss, int B, int C, ppf_stream_t stream);
/* Evaluation metrics (tools/engine_proto.py:143-184) of one batch ADDED into acc, a device double[8] that persists across batches (the
 * caller zeroes it once per epoch and reads it once at the end); logits* [B][C] fp32, logits_global / logits_local may be NULL (their
 * slots then stay untouched):
 *   acc[0] samples seen, acc[1] sum of per-sample cross-entropy of logits, acc[2] top-1 hits, acc[3] top-5 hits of logits,
 *   acc[4] top-1 hits of logits_global, acc[5] top-1 hits of logits_local, acc[6] rows whose label is outside [0, C), acc[7] reserved (0).
 * Top-1 hit: label == FIRST index of the row maximum (torch argmax).  Top-5 hit: #{j : x_j > x_t or (x_j == x_t and j < t)} < 5 (equal to
 * "label in topk(5)" without ties; always a hit when C < 5).  A label outside [0, C) reads nothing and counts in acc[0] and acc[6] only.
 * Row statistics in fp64 ((mx - x_t) + log(sum exp(x - mx))); one wave per row, then LDS, then a fixed-order sum over the workgroups and
 * one adder: no floating-point atomics, two runs over the same batches give bit-identical acc.  The workgroup partials are kept in a
 * device buffer owned by the library: calls of one process must be ordered on ONE stream. */
int ppf_eval_metrics(const float* logits, const float* logits_global, const float* logits_local, const void* label_i64, double* acc,
                     int B, int C, ppf_stream_t stream);
/* Prototype bank: dataset-wide nearest patches per prototype (the ranking ProtoPNet-family tools show and project onto; the reference
 * has no such pass).  One launch merges a batch's candidates into persistent per-prototype lists of K entries, sorted best-first, all in
 * device memory and updated in place: val [P][K] fp32 activations, img [P][K] int32 image ids, pos [P][K] int32 index in the side x side
 * patch grid (idx[b][argmax[b][p]]; -1 on the global branch), best_feat [P][Dp] fp32 = the latent token of the rank-0 entry, rewritten
 * only when the launch changes rank 0.  ppf_proto_topk_init fills val with -inf and img / pos with -1 (an unfilled slot; sorts last).
 *   act_max [B][P], argmax [B][P]: as ppf_proto_fwd writes them; argmax == NULL (global / cls branch): the token is tok row t0 itself.
 *   idx [B][k] int32: the reserved-token indices (NULL exactly when argmax is NULL).  tok / stride_b / t0 / Dp: the addressing of
 *   ppf_proto_fwd (sample b's token i at tok + b*stride_b + (t0+i)*Dp; tok and best_feat 16-byte aligned, stride_b % 4 == 0).
 *   label_i64 [B], image_id [B] int32 (>= 0).  ppc > 0: class-specific, sample b is offered to prototype p only if label[b] == p / ppc;
 *   ppc == 0: every sample is offered to every prototype (label_i64 may be NULL).
 * Order (total): larger activation first, equal activations by smaller image id; NaN and -inf candidates are never admitted.  The final
 * state is therefore independent of the batch size and of the order the batches arrive in.  Image ids must be unique across all the
 * launches that feed one list: the caller's contract, not checked.  1 <= K <= 64, 1 <= B <= 1024, P >= 1, Dp % 4 == 0. */
int ppf_proto_topk_init(float* val, int* img, int* pos, int P, int K, ppf_stream_t stream);
int ppf_proto_topk_merge(const float* act_max, const int* argmax, const int* idx, int k, const float* tok, int64_t stride_b, int t0, int Dp,
                         const void* label_i64, const int* image_id, int ppc, int B, int P, int K, float* val, int* img, int* pos,
                         float* best_feat, ppf_stream_t stream);
/* Local analysis (csrc/explain.hip): why did sample b get class c?  The counterpart of the bank's global analysis, from what an eval
 * forward leaves on the device (ProtoPNet's "local analysis"; the reference's main_visualize.py draws every prototype of a chosen class
 * and never ranks evidence).  One launch per branch explains M classes of each of B samples: for list (b, m) of class c = cls_out[b][m]
 * the contribution of prototype p is fl(act_max[b][p] * fl(scale * weight[c][p])) -- two separate fp32 roundings, nothing fused or
 * reassociated -- and proto / contrib / act / cell [B][M][K] hold the K best under a TOTAL order: sign * contrib descending, equal keys
 * by smaller prototype id.  sign = +1: evidence for the class, sign = -1: the strongest evidence against it.  NaN and +-inf
 * contributions are never admitted.  Unfilled slots (K > P, or too few admissible candidates): proto = -1, cell = -1, contrib = act = -inf.
 *   act_max [B][P], argmax [B][P]: as ppf_proto_fwd writes them.  argmax == NULL: the global / cls branch; idx, act_full and maps are
 *   NULL too and cell is filled with -1.  idx [B][T] int32: the grid positions of the reserved tokens (distinct within a sample);
 *   cell = idx[b][argmax[b][p]], -1 when that argmax lies outside [0, T).  weight [C][P]: the branch's last layer; scale: the branch's
 *   share of the logit (1 - global_coe local, global_coe global), rounded once to fp32 by the caller; ppc: prototypes per class.
 *   logits [B][C]; cls_in [B][M] int32: the classes to explain, or NULL: the kernel picks the top-M classes of logits itself (larger
 *   logit first, equal logits by smaller class id, NaN never picked).  cls_out [B][M] and cls_logit [B][M] (= logits[b][c]) are always
 *   written.  A class outside [0, C), or a slot with no pickable class, gives cls_out = -1, cls_logit = -inf, an all-unfilled list, zero
 *   evidence and zero maps, and reads nothing out of range.
 *   evidence [B][M][2]: [0] = the sum of the contributions of the class's own prototypes (p / ppc == c), [1] = the sum over all others;
 *   their sum is this branch's share of logits[b][c].  Non-finite terms are included: the sums agree with the logits, they do not hide a
 *   NaN.  Summed in fp64, rounded once to fp32.
 *   maps [B][M][K][G] (optional; G = cells of the full patch grid, G <= 8192): map (b, m, k) is zero everywhere except
 *   act_full[b][p][t] at cell idx[b][t] for the selected p (act_full [B][P][T] as ppf_proto_fwd writes it; an idx entry outside [0, G)
 *   is skipped) -- interpret.expand_to_grid for the K selected prototypes only; all zero for an unfilled slot.
 * 1 <= K <= 64, 1 <= M <= 8, M <= C, P % ppc == 0, sign = +-1.  One wave per list, no atomics: deterministic. */
int ppf_explain_topk(const float* act_max, const int* argmax, const int* idx, int T, const float* act_full, const float* weight, float scale,
                     int ppc, const float* logits, const int* cls_in, int sign, int B, int P, int C, int M, int K, int G, int* cls_out,
                     float* cls_logit, int* proto, float* contrib, float* act, int* cell, float* evidence, float* maps, ppf_stream_t stream);
/* Prototype statistics over a data set (csrc/proto_stats.hip): which prototypes does the model use?  ProtoPNet's pruning pass and the
 * activation percentiles of its local analysis both need, per prototype, the distribution of the pooled activation over the own-class
 * and the other-class images; the reference has no such pass.  One call adds a batch into persistent int32 accumulators in device
 * memory, zeroed once by the caller.  Addition of ABI 10: no existing entry point changed.
 *   act_max [B][P], argmax [B][P]: as ppf_proto_fwd writes them; idx [B][T] int32: the grid positions of the reserved tokens.
 *   argmax == NULL: the global / cls branch; idx must be NULL too, coloc may be NULL and is not touched.  label_i64 [B]; C = P / ppc.
 *   hist [P][2][NB]: hist[p][slot][bin(act_max[b][p])] += 1 with slot 0 when label[b] == p / ppc (own class), else slot 1.
 *     bin(a): t = fl(fl(a - lo) * inv_width) in fp32, two separate roundings, nothing fused; bin 0 when t < 0 (-inf included),
 *     bin NB-1 when t >= NB (+inf included), else (int)t.  The caller passes inv_width = fl(NB / fl(hi - lo)), rounded on the host.
 *   nan_count [P][2]: a NaN activation is not binned; nan_count[p][slot] += 1 instead.
 *   coloc [P][ppc] (local branch): fed by own-class samples only.  For sample b of class c and prototypes p, q of class c:
 *     cell(p) = idx[b][argmax[b][p]], invalid when that argmax lies outside [0, T); coloc[p][q % ppc] += 1 when both cells are valid
 *     and equal.  The diagonal counts the own-class images in which p has a valid cell.
 *   images [C]: images[label[b]] += 1.  A label outside [0, C) adds one to bad[0], reads nothing else and adds nothing else (the
 *     ppf_part_meter_update convention).
 * 1 <= B <= 1024, P >= 1, P % ppc == 0, 1 <= ppc <= 64, 8 <= NB <= 128, T >= 1 on the local branch, lo finite, inv_width finite
 * and > 0 (else PPF_ERR_SHAPE).  Integer atomics only: any split of the same images into batches, in any order, gives the same tables. */
int ppf_proto_stats_update(const float* act_max, const int* argmax, const int* idx, int T, const void* label_i64, int ppc, int B, int P, int NB,
                           float lo, float inv_width, int* hist, int* nan_count, int* coloc, int* images, int* bad, ppf_stream_t stream);
/* Faithfulness of an explanation (csrc/faithful.hip): deletion / insertion curves (Petsiuk et al., RISE, 2018).  Rank the G cells of the
 * patch grid by their evidence for a class, remove (or show only) the first counts[s] of them, and read the class probability off the
 * model's logits for the perturbed images; the forwards in between are the caller's.  The reference has no such pass.  Additions of
 * ABI 10: no existing entry point changed.
 *   ppf_cell_order     order, rank int32 [B][M][G] and score fp32 [B][M][G]: a TOTAL order of the cells per (sample, class) row, tier
 *                      ascending, then score descending, then smaller cell; NaN sorts below -inf within its tier, -0 == +0;
 *                      rank[b][m][order[b][m][r]] == r.  The ranking uses the returned fp32 score, so it can be verified from the scores.
 *                      mode 0 (evidence): a reserved cell g = idx[b][t] is tier 0 with score = fp32( sum over p in fp64 of
 *                        double(fl(scale * weight[c][p])) * double(act_full[b][p][t]) ) -- the fp32 product of ppf_explain_topk, every fp64
 *                        term exact, one rounding at the end, summation order unspecified; an unreserved cell is tier 1 with score
 *                        token_attn[b][g].  idx entries outside [0, G) are ignored, a cell listed twice takes its smallest t.
 *                      mode 1 (attention): every cell tier 0, score token_attn[b][g] (what the token reservation looks at).
 *                      mode 2 (random): every cell tier 0, score (word >> 8) * 2^-24 with word = the first word of Philox4x32-10, key =
 *                        seed, counter = (cell, 0, image id low, image id high): a function of (seed, image id, cell) alone, not of the
 *                        batch size or order (as ppf_add_gauss_noise).
 *                      act_full [B][P][T], idx [B][T] int32, token_attn [B][G], weight [C][P], classes [B][M] int32, image_id_i64 [B]
 *                      int64; pointers a mode does not read may be NULL.  A class outside [0, C): order = rank = -1, score = 0 for that
 *                      row.  1 <= G <= 1024, 1 <= T <= G (mode 0), 1 <= M <= 8.  One workgroup per row, no float atomics: deterministic.
 *   ppf_patch_perturb  out fp32 [S][B][M][Cc][H][W] from x [B][Cc][H][W], rank [B][M][G] as above and counts int32 [S] on the DEVICE:
 *                      insertion = 0 (deletion): a pixel of cell g is the baseline when rank[b][m][g] < counts[s], else x;
 *                      insertion = 1: a pixel is x when rank[b][m][g] < counts[s], else the baseline.  A row of ranks -1 copies x.
 *                      baseline fp32 [B][Cc][H][W], or NULL: the constant baseline_const.  The grid is side x side, side = sqrt(G),
 *                      row-major; H == W, side divides H, and the patch width H / side is a multiple of 4 (a 16-byte vector never
 *                      straddles a cell); x, baseline, out 16-byte aligned.  x and the baseline are read once, all S * M copies written
 *                      from registers.
 *   ppf_class_prob     prob [R] = softmax(logits[r])[cls[r]] = expf(l[c] - max) / sum expf(l - max) of logits fp32 [R][C], cls int32 [R]:
 *                      accurate expf, the sum in fp64, one wave per row; the softmax rows are never written.  A class outside [0, C) or
 *                      a NaN in the row gives NaN. */
int ppf_cell_order(const float* act_full, const int* idx, const float* token_attn, const float* weight, float scale, const int* classes,
                   const void* image_id_i64, uint64_t seed, int mode, int B, int P, int C, int T, int G, int M, int* order, int* rank, float* score,
                   ppf_stream_t stream);
int ppf_patch_perturb(const float* x, const int* rank, const int* counts, int S, int insertion, const float* baseline, float baseline_const, int B,
                      int M, int Cc, int H, int W, int G, float* out, ppf_stream_t stream);
int ppf_class_prob(const float* logits, const int* cls, int R, int C, float* prob, ppf_stream_t stream);
/* The same curves per PIXEL, from a blurred canvas (csrc/pixel_faithful.hip): the metric as published removes pixels in saliency order and
 * starts the insertion curve from a blurred image.  n = H * W pixels per row, pixel i = y * W + x.  Additions of ABI 10: no existing entry
 * point changed.
 *   ppf_pixel_order    rank int32 [R][n] from score fp32 [R][n] and classes int32 [R]: rank[r][i] = the number of pixels j of row r that
 *                      come before i -- a larger score_key(score) (order_keys.h: NaN lowest, -0 == +0), or the same key and j < i.  Every
 *                      row is a permutation of 0 .. n-1; a row with classes[r] < 0 is all -1.  1 <= n <= 65536, R >= 1.  The composite key
 *                      pixel_order_key(score, i) = (~score_key << 32) | i (order_keys.h) is unique per row and ascending in this order, so
 *                      any correct sort gives these bits.  Built: a workgroup per row runs a stable LSD radix sort, 8 bits per pass, over
 *                      the 32-bit word ~score_key, with (key, pixel) pairs ping-ponging through `scratch` (stable passes from pixel order
 *                      keep equal keys in pixel order); the four digit histograms come from one read of the row and a pass whose digit is
 *                      constant over the row is skipped (up-sampled maps have few distinct values).  Not the bitonic network on 64-bit
 *                      keys: a row does not fit LDS (50 176 x 8 B against 160 KiB) and the network is 136 stages over 65 536 padded keys
 *                      against at most four passes.  scratch: ppf_pixel_order_scratch_bytes(R, n) = min(R, 256) * 16 * n bytes, 4-byte
 *                      aligned, used by this launch only (0 for sizes outside the limits).  Integer LDS atomics only: deterministic.
 *   ppf_pixel_random   score fp32 [B][n] = (word >> 8) * 2^-24, word = the first word of Philox4x32-10, key = seed, counter = (pixel,
 *                      0x80000000, image id low, image id high): a function of (seed, image id, pixel) alone.  Counter word 1 across the
 *                      library: 0 the random cell order, 1 + n < 2^31 the RISE masks, e/4 high (0 below 2^34 elements) the input noise of
 *                      ppf_add_gauss_noise, 0x80000000 ppf_warp_nodes, 0x80000001 + (n >> 1) in [0x80000001, 0xC0000000] the KernelSHAP
 *                      coalitions (ppf_shap_coalitions), 0xC0000001 the PartsWorld scene and 0xC0000002 its pixel noise (ppf_synth_scene,
 *                      ppf_synth_render; the rest of (0xC0000000, 0xFFFFFFFF] is free) -- so this draw is disjoint from the cell order,
 *                      the RISE masks, the coalitions and PartsWorld but NOT from ppf_warp_nodes: pixel q and warp node q < (s + 1)^2 <= 289 of the same image under the same seed share
 *                      a Philox block (this draw reads word .x, the node's dy).  The two never meet in one computation (a pixel order and
 *                      a shape perturbation of 'because'); a caller who needs them independent gives them different seeds.
 *   ppf_pixel_perturb  ppf_patch_perturb's contract with rank int32 [B][M][n], n = H * W, in place of the cell's rank: out fp32
 *                      [S][B][M][Cc][H][W]; deletion: the pixel is the baseline when rank < counts[s]; insertion: the pixel is x when
 *                      rank < counts[s]; a negative rank keeps x (a row of -1 copies x).  H >= 1, W a multiple of 4, 1 <= M <= 8; x,
 *                      baseline, rank and out 16-byte aligned.  x, the baseline and the rank are read once per launch, all S * M copies
 *                      written from registers.
 *   ppf_gauss_blur     out fp32 [R][H][W] = a separable blur of every plane of x with a zero border and taps fp32 [2r + 1] on the DEVICE.
 *                      Horizontal: t[y][x] = the fp32 sum, started from +0, over d = -r .. r in that order of fl(taps[d + r] * x[y][x + d]),
 *                      one rounding per multiply and per add, nothing contracted; a tap with x + d outside [0, W) is skipped, not added
 *                      as zero.  Vertical: the same over t (rounded to fp32) along y.  1 <= r <= 16, H, W >= 1, R <= 65535 planes,
 *                      H <= 65535 * 16, out != x.  One launch, the intermediate in LDS. */
size_t ppf_pixel_order_scratch_bytes(int R, int n);
int ppf_pixel_order(const float* score, const int* classes, int R, int n, int* rank, void* scratch, size_t scratch_bytes, ppf_stream_t stream);
int ppf_pixel_random(const void* image_id_i64, uint64_t seed, int B, int n, float* score, ppf_stream_t stream);
int ppf_pixel_perturb(const float* x, const int* rank, const int* counts, int S, int insertion, const float* baseline, float baseline_const, int B,
                      int M, int Cc, int H, int W, float* out, ppf_stream_t stream);
int ppf_gauss_blur(const float* x, const float* taps, int r, int R, int H, int W, float* out, ppf_stream_t stream);
/* RISE saliency (csrc/rise.hip): the model-agnostic baseline the deletion / insertion metric was published with (Petsiuk et al., 2018):
 * N random masks per image, the class probability of each masked image (the forwards and ppf_class_prob are the caller's), saliency =
 * the probability-weighted mean mask.  The reference has no such pass.  Additions of ABI 10: no existing entry point changed.
 * The masks are integer-exact; this is the contract the numpy referees (interpret.rise_*) keep bit for bit.
 *   sizes     image H x W with H == W and W % 4 == 0; s low-resolution cells per side, 1 <= s <= 14; node spacing c = ceil(H / s) <= 4096;
 *             L = s + 2 nodes per side; N masks per image, 1 <= N <= 2^31 - 2; keep threshold thr in [1, 2^24], computed once by the
 *             host as round(p * 2^24): the effective keep probability is thr / 2^24.
 *   draws     Philox4x32-10 with key = seed (64 bits, as ppf_cell_order) and counter = (k, 1 + n, image id low, image id high) for mask n
 *             of image id (the random cell order uses counter word 1 = 0: the streams are disjoint).  Node q = i * L + j is on when
 *             (word[q % 4] of call k = q / 4) >> 8 < thr.  The shift comes from call k = 0xFFFFFFFF: dy = ((w.x >> 8) * c) >> 24,
 *             dx = ((w.y >> 8) * c) >> 24, both in [0, c).  A mask depends on (seed, image id, n) alone, not on the batch.
 *   value     pixel (y, x): uy = y + dy, i = uy / c, ry = uy % c, likewise j and rx from x + dx (i + 1 <= s + 1 always); numerator
 *             K = (c-ry) * ((c-rx) * g[i][j] + rx * g[i][j+1]) + ry * ((c-rx) * g[i+1][j] + rx * g[i+1][j+1]) in [0, c^2];
 *             mask value m = fdiv_rn((float)K, (float)(c*c)), one rounding.
 *   ppf_rise_nodes       nodes uint8 [B][N][L*L] (0 / 1) and shift int32 [B][N][2] = (dy, dx) of image_id_i64 [B]; H enters through c only.
 *   ppf_rise_apply       out fp32 [Nc][B][Cc][H][W] for masks n0 .. n0 + Nc - 1 (0 <= n0, n0 + Nc <= N) of the tables above:
 *                        out = fadd_rn(fmul_rn(m, x), fmul_rn(fsub_rn(1, m), base)), base = baseline fp32 [B][Cc][H][W] or, NULL, the
 *                        constant baseline_const (as ppf_patch_perturb).  The mask does not depend on the class: one image per
 *                        (mask, sample).  x and the baseline are read once, the copies written from registers; the node table is read,
 *                        Philox is not run.  Shifts in the table are clamped into [0, c).  x, baseline, out 16-byte aligned.
 *   ppf_rise_accumulate  from the tables and prob fp32 [N][B][M], 1 <= M <= 8, with norm = N * (thr / 2^24) * c^2 in fp64 (evaluated
 *                        left to right):  sal fp32 [B][M][H][W] = (float)(acc / norm), acc = the fp64 sum over n ascending of
 *                        (double)prob * (double)K (every product exact);  cell fp32 [B][M][G] = (float)(accW / (norm * patch^2)), accW =
 *                        the fp64 sum over n ascending of (double)prob * (double)W[n][g], W = the int32 sum of K over the pixels of cell
 *                        g of the side x side grid, side = sqrt(G), patch = H / side (side divides H, G <= 1024, patch^2 * c^2 <= 2^29
 *                        so these products are exact too).  The masks are regenerated from the node table, never stored at pixel
 *                        resolution; no floating-point atomics; a NaN probability makes its (sample, class) row NaN by propagation.
 *                        sal 16-byte aligned.  Two launches (pixels, cells). */
int ppf_rise_nodes(const void* image_id_i64, uint64_t seed, int thr, int B, int N, int s, int H, void* nodes_u8, int* shift, ppf_stream_t stream);
int ppf_rise_apply(const float* x, const void* nodes_u8, const int* shift, int N, int n0, int Nc, int s, const float* baseline, float baseline_const,
                   int B, int Cc, int H, int W, float* out, ppf_stream_t stream);
int ppf_rise_accumulate(const void* nodes_u8, const int* shift, const float* prob, int B, int N, int M, int s, int thr, int H, int W, int G, float* sal,
                        float* cell, ppf_stream_t stream);
/* KernelSHAP cell attributions (csrc/shap.hip; Lundberg & Lee, 2017): Shapley values of d = s x s square players of an image for the
 * value of a class, by the least-squares fit to N sampled coalitions under the constraint that the attributions add up to
 * f(x) - f(baseline), with the paired sampling of Covert & Lee (2021).  Forwards only, as RISE; the forwards and ppf_class_prob are the
 * caller's.  The reference has no such pass, and nobody has run this one on a trained checkpoint.  Additions of ABI 10: no existing
 * entry point changed.  Coalitions, masked images and the Gram matrix are integer-exact; this is the contract the numpy referees
 * (interpret.shap_*) keep bit for bit, and csrc/shap_plan.h states its index rules for a host program (tests/shap_plan_check.cpp).
 *   sizes     image H x W with H == W; s players per side, 2 <= s <= 14, d = s^2 players in [4, 196]; s divides H and the player width
 *             H / s is a multiple of 4 (a 16-byte vector never straddles a player); s divides side = sqrt(G), a player is r x r grid
 *             cells, r = side / s.  N samples per image, N even, 2 <= N <= 2^30; 1 <= M <= 8 classes per image.
 *             Player of pixel (y, x): (y / (H / s)) * s + x / (W / s); of grid cell (gy, gx): (gy / r) * s + gx / r.
 *   draws     Philox4x32-10 with key = seed (64 bits) and counter = (k, 0x80000001 + j, image id low, image id high) for pair j = n >> 1
 *             of image id: counter word 1 lies in [0x80000001, 0xC0000000], disjoint from every other draw of the library (the list is
 *             under ppf_pixel_random).  Key of player q: word q % 4 of call k = q / 4, all 32 bits.  Size of coalition 2j: from call
 *             k = 0xFFFFFFFF, u = w.x >> 8, size = 1 + #{t in [0, d - 3] : table[t] <= u}, so 1 <= size <= d - 1 whatever the table holds.
 *   table     int32 [d - 1] on the DEVICE, computed once by the host: table[t] = round(2^24 * sum_{k <= t + 1} w_k / sum_k w_k) with
 *             w_k = 1 / (k (d - k)), k = 1 .. d - 1, the Shapley kernel's distribution of sizes; table[d - 2] = 2^24.  The host side of
 *             the binding refuses a table that is not non-decreasing or does not end at 2^24 (ops.shap_coalitions).
 *   members   q is in coalition 2j iff #{r : (key_r, r) < (key_q, q) lexicographically} < size: a uniform subset of that size, by a
 *             counting rank, no atomics.  Coalition 2j + 1 is the complement of coalition 2j.  A coalition depends on (seed, image id,
 *             n, d) alone, not on the batch.
 *   ppf_shap_coalitions  coal uint32 [B][N][Wd], Wd = ceil(d / 32): bit q % 32 of word q / 32 is the membership of player q; unused bits 0.
 *   ppf_shap_apply       out fp32 [Nc][B][Cc][H][W] for samples n0 .. n0 + Nc - 1 (0 <= n0, n0 + Nc <= N): a pixel is x when its player's
 *                        bit is set, else base = baseline fp32 [B][Cc][H][W] or, NULL, the constant baseline_const (as
 *                        ppf_patch_perturb).  A select only: bit-exact.  x and the baseline are read once, all Nc copies written from
 *                        registers with 16-byte accesses; the coalition words of the chunk are staged in LDS.  x, baseline, out 16-byte
 *                        aligned.
 *   ppf_shap_gram        from coal, val fp32 [N][B][M] and v0 fp32 [B][M]:  A int32 [B][d][d] = #{n : z_i and z_j}, the full symmetric
 *                        matrix (popcounts of ANDed bit-columns, integer adds only);  bvec fp64 [B][M][d] = the sum over n ascending,
 *                        over the samples with z_{n,i} = 1 only, of fsub((double)val, (double)v0): one rounded subtract and one rounded
 *                        add per term, nothing contracted, started from +0.  Both bit-exact to a numpy loop.
 *   ppf_shap_solve       per image in fp64: A = L L^T by Cholesky, x_m = A^-1 b_m and y = A^-1 1, delta_m = (double)v1 - (double)v0 (v1
 *                        fp32 [B][M], the value of the whole image), phi_m = x_m - y * ((sum x_m - delta_m) / sum y): the least-squares
 *                        fit under sum phi = delta.  One factorisation per image serves the M + 1 right-hand sides; fixed summation
 *                        order, no atomics: repeats are bit-identical.  The factor lives in `scratch`
 *                        (ppf_shap_solve_scratch_bytes(B, d) = B * d^2 * 8 bytes, 8-byte aligned, used by this launch only; 0 for sizes
 *                        outside the limits).  Writes phi fp64 [B][M][d], cell fp32 [B][M][G] = (float)(phi[player of g] / r^2) and bad
 *                        int32 [B].  A pivot that is <= 0 or NaN sets bad[b] = 1 and makes all M rows of that image NaN (else bad[b] =
 *                        0); a row whose bvec or delta is not finite is all NaN and leaves the other rows alone.  G <= 1024. */
int ppf_shap_coalitions(const void* image_id_i64, uint64_t seed, const int* table, int B, int N, int s, void* coal_u32, ppf_stream_t stream);
int ppf_shap_apply(const float* x, const void* coal_u32, int N, int n0, int Nc, int s, const float* baseline, float baseline_const, int B, int Cc,
                   int H, int W, float* out, ppf_stream_t stream);
int ppf_shap_gram(const void* coal_u32, const float* val, const float* v0, int B, int N, int M, int s, int* A, double* bvec, ppf_stream_t stream);
size_t ppf_shap_solve_scratch_bytes(int B, int d);
int ppf_shap_solve(const int* A, const double* bvec, const float* v0, const float* v1, int B, int M, int s, int G, void* scratch, size_t scratch_bytes,
                   double* phi, float* cell, int* bad, ppf_stream_t stream);
/* Integrated gradients (csrc/ig.hip; Sundararajan et al., 2017): attribution = (x - baseline) * the gradient averaged along the straight
 * path from the baseline to x; the attributions of an image sum to f(x) - f(baseline).  The forwards and backwards along the path are the
 * caller's (interpret.input_gradient); these three streaming kernels are everything in between.  The reference has no such pass.
 * Additions of ABI 10: no existing entry point changed.
 * The arithmetic is the contract the numpy referees (interpret.ig_point, ig_accumulate, ig_finish with device=False) keep bit for bit:
 * plain fp32, every operation rounded once to nearest (fsub_rn / fmul_rn / fadd_rn), nothing fused or reassociated, no transcendental
 * function, no floating-point atomics.  16-byte accesses when the sizes named below are multiples of 4 and every pointer is 16-byte
 * aligned, scalar ones otherwise: the values do not depend on it.  base[e] is baseline[e], or the constant baseline_const when baseline
 * is NULL (as ppf_patch_perturb / ppf_rise_apply).
 *   ppf_ig_point       out[e] = fadd_rn(base[e], fmul_rn(alpha, fsub_rn(x[e], base[e]))) over n >= 1 fp32 elements (vectors: n % 4 == 0).
 *                      alpha = 0 gives the baseline exactly for finite inputs; a constant baseline of 0 and alpha = 1 give x.
 *   ppf_ig_accumulate  g fp32 [R][n]; row r of the accumulator starts at acc + r * acc_stride, acc_stride >= n (so one class column of a
 *                      [B][M][...] accumulator can be the target).  first = 1: acc = fmul_rn(w, g), the accumulator is not read (no
 *                      zero fill before the first step); first = 0: acc = fadd_rn(acc, fmul_rn(w, g)).  Elements between the rows
 *                      are not touched.  NaN propagates.  Vectors: n % 4 == 0 and acc_stride % 4 == 0.  first other than 0 / 1 is
 *                      PPF_ERR_ARG.
 *   ppf_ig_finish      acc, attr fp32 [B][M][C][H][W]; x, baseline fp32 [B][C][H][W] (shared by the M class columns):
 *                      attr = fmul_rn(fsub_rn(x, base), acc).  cell64 fp64 [B][M][G], G = (H / patch) * (W / patch), cells row-major:
 *                      the sum over the cell's C * patch^2 elements of (double)attr (every term exact).  The order of that sum is
 *                      fixed but unspecified (within C * patch^2 * 2^-53 * sum |attr| of any other order); repeated runs are
 *                      bit-identical; a NaN makes its own cell NaN and no other.  One pass: the attribution is written from the
 *                      registers that feed the cell sums.  patch divides H and W, 1 <= M <= 8, G <= 1024 (ppf_cell_order's limits),
 *                      else PPF_ERR_SHAPE before any device call.  Vectors: patch % 4 == 0. */
int ppf_ig_point(const float* x, const float* baseline, float baseline_const, float alpha, int64_t n, float* out, ppf_stream_t stream);
int ppf_ig_accumulate(const float* g, float w, int first, int R, int64_t n, float* acc, int64_t acc_stride, ppf_stream_t stream);
int ppf_ig_finish(const float* acc, const float* x, const float* baseline, float baseline_const, int B, int M, int C, int H, int W, int patch,
                  float* attr, double* cell64, ppf_stream_t stream);
/* "This looks like that, because ..." (csrc/because.hip; Nauta et al., 2021): suppress one visual characteristic of an image -- hue,
 * saturation, contrast, texture or shape --, run the model again and read the prototype's similarity at the same grid cell; the forwards
 * in between are the caller's.  The reference has no such pass.  Additions of ABI 10: no existing entry point changed.
 * The arithmetic is the contract the numpy referees (interpret.color_affine, gray_sum, contrast_offset, bilateral, warp_nodes_from_ids,
 * warp_apply, because_score) keep bit for bit: plain fp32, fl() = one rounding to nearest, nothing fused or reassociated, every
 * division correctly rounded, no transcendental function on the device.
 *   images    x, out fp32 [B][3][H][W], normalised; mean3 / std3 / matrix9 / ws / wr256 are HOST pointers (as ppf_image_finish_u8's).
 *             B <= 65535, H * W <= 2^22.  16-byte accesses when W % 4 == 0 and the pointers are 16-byte aligned, scalar ones otherwise:
 *             the values do not depend on it (ppf_warp_apply is a gather: one pixel per lane either way; the bilateral filter reads
 *             through LDS).
 *   pixel     v_c = clamp(fl(fl(x_c * std_c) + mean_c)); clamp(v) = v > 0 ? (v < 1 ? v : 1) : 0, so NaN becomes 0.  A result u_c is
 *             written as fl(fl(clamp(u_c) - mean_c) / std_c).
 *   luma      y = fl(fl(fl(0.299 r) + fl(0.587 g)) + fl(0.114 b)) of the clamped (r, g, b) = v; q8 = min(max((int)floor(fl(fl(255 y) +
 *             0.5)), 0), 255).
 *   ppf_color_affine     u_k = fl(fl(fl(fl(M[k][0] r) + fl(M[k][1] g)) + fl(M[k][2] b)) + offset[b][k]), matrix9 = M row-major; offset
 *                        fp32 [B][3] on the device, or NULL: that addition is left out.  Saturation f: M = f I + (1 - f) [w; w; w] with
 *                        w = (0.299, 0.587, 0.114); hue: M = T^-1 R(theta) T with T = RGB -> YIQ; contrast f: M = f I and
 *                        offset[b][k] = (1 - f) * the image's mean luma (below); each formed in fp64 by the host, rounded once.
 *   ppf_gray_sum         sum int32 [B] = the integer sum of q8 over the image's pixels (zeroed by the call; integer atomics: exact and
 *                        the same at any launch shape; 255 * H * W < 2^31).
 *   ppf_contrast_offset  offset[b][k] = fl(one_minus_f * fl(fl((float)sum[b] / (float)(H * W)) / 255)) for k = 0 .. 2, on the device: no
 *                        host read between the sum and the colour transform.
 *   ppf_bilateral        joint bilateral filter of window radius r, 1 <= r <= 8, guided by q8: for pixel p, over the taps q = p + (dy,
 *                        dx) in row-major window order (dy outer, both ascending from -r), taps outside the image skipped:
 *                          w = fl(ws[dy + r][dx + r] * wr256[|q8(p) - q8(q)|]);  sw = fl(sw + w);  s_k = fl(s_k + fl(w * v_k(q)))
 *                        from sw = s_k = 0, the same w for the three channels; u_k = fl(s_k / sw).  ws: (2r + 1)^2 spatial weights,
 *                        wr256: 256 range weights, all finite and >= 0 (Gaussians, computed by the caller in fp64 and rounded).  sw = 0
 *                        gives 0 / 0 = NaN, which the clamp writes as 0.  out != x.  One workgroup stages a 32 x 16 tile and its halo in
 *                        LDS once (dynamic LDS <= 30 KiB).
 *   ppf_warp_nodes       nodes int32 [B][(s + 1)^2][2] = (dy, dx) of node q = i * (s + 1) + j in units of 1 / 256 pixel, uniform in
 *                        [-amp256, amp256]: d = (((word >> 8) * (2 amp256 + 1)) >> 24) - amp256 with word = .x (dy) / .y (dx) of
 *                        Philox4x32-10, key = seed, counter = (q, 0x80000000, image id low, image id high) -- disjoint from the random
 *                        cell order (word 1 = 0) and the RISE masks (word 1 = 1 + n < 2^31).  A function of (seed, image id, node) alone.
 *                        1 <= s <= 16, 0 <= amp256 <= 2^15.
 *   ppf_warp_apply       out fp32 [B][Cc][H][W] from x of the same shape (any normalisation: the blend is linear) and the node table;
 *                        H == W, node spacing c = ceil(H / s) <= 2048, c^2 * amp256 <= 2^31 - 1.  Pixel (y, x): i = y / c, ry = y % c,
 *                        j = x / c, rx = x % c; K = ((c-ry)(c-rx), (c-ry) rx, ry (c-rx), ry rx) on nodes (i, j), (i, j+1), (i+1, j),
 *                        (i+1, j+1) (sum c^2); displacement d = floor(sum K_n d_n / c^2) per axis, in int32 (node values are clamped
 *                        into [-amp256, amp256] first).  Y = min(max(256 y + dy, 0), 256 (H - 1)), likewise X; (sy, sx) = (Y >> 8,
 *                        X >> 8), (fy, fx) = (Y & 255, X & 255), sy1 = min(sy + 1, H - 1), sx1 likewise; a = fx / 256, e = fy / 256 (exact):
 *                          top = fx ? fl(fl((1 - a) * x[sy][sx]) + fl(a * x[sy][sx1])) : x[sy][sx]
 *                          bot = fx ? fl(fl((1 - a) * x[sy1][sx]) + fl(a * x[sy1][sx1])) : x[sy1][sx]
 *                          out = fy ? fl(fl((1 - e) * top) + fl(e * bot)) : top
 *                        so amplitude 0 copies x bit for bit.  out != x.
 *   ppf_because_score    row (b, k), one wave each, of protos int32 [B][K] and cells int32 [B][K] (the clean forward's cell of the
 *                        prototype) against a PERTURBED forward's act_full [B][P][T], idx int32 [B][T] and act_max [B][P]:
 *                          best[b][k] = act_max[b][p];  same[b][k] = act_full[b][p][t] for the smallest t with idx[b][t] == cell and
 *                          lost[b][k] = 0;  no such t (the perturbed image no longer reserves the cell; cell outside [0, G), so an idx
 *                          entry outside the grid never matches): same = 0 -- the zero interpret.expand_to_grid puts there -- and lost = 1.
 *                        A NaN activation is written as it is.  p outside [0, P): best = NaN, same = 0, lost = 1, nothing read.
 *                        idx == NULL: the global / cls branch, which has no cells: only best is written (act_full, cells, same, lost
 *                        may be NULL).  same, best fp32 and lost int32 [B][K]. */
int ppf_color_affine(const float* x, const float* matrix9, const float* offset, const float* mean3, const float* std3, int B, int H, int W, float* out,
                     ppf_stream_t stream);
int ppf_gray_sum(const float* x, const float* mean3, const float* std3, int B, int H, int W, int* sum, ppf_stream_t stream);
int ppf_contrast_offset(const int* gray_sum, int B, int H, int W, float one_minus_f, float* offset, ppf_stream_t stream);
int ppf_bilateral(const float* x, const float* ws, const float* wr256, int r, const float* mean3, const float* std3, int B, int H, int W, float* out,
                  ppf_stream_t stream);
int ppf_warp_nodes(const void* image_id_i64, uint64_t seed, int B, int s, int amp256, int* nodes, ppf_stream_t stream);
int ppf_warp_apply(const float* x, const int* nodes, int s, int amp256, int B, int Cc, int H, int W, float* out, ppf_stream_t stream);
int ppf_because_score(const float* act_full, const int* idx, const float* act_max, const int* protos, const int* cells, int B, int P, int T, int G, int K,
                      float* same, float* best, int* lost, ppf_stream_t stream);
/* Spatial alignment of prototypes (csrc/alignment.hip): the image gradient's last step and the two kernels of the misalignment test
 * (Sacha et al., AAAI 2024): perturb only the pixels outside a prototype's box, follow its activation and its peak, and report the share
 * of the pixel gradient inside the box; the forwards and backwards in between are the caller's.  The reference has no such pass.
 * Additions of ABI 10: no existing entry point changed.
 *   ppf_col2im_patch_f32  img fp32 [B][C][H][W] from cols fp32 [B*gh*gw][C*patch*patch]: the exact inverse of the column order
 *                         ppf_im2col_patch / ppf_im2col_patch_f32 write (patch (gy, gx) row-major, columns (c, py, px)).  The patch
 *                         stride equals the patch size, so every image element is written exactly once: no atomics, no zero fill.
 *                         The image gradient is col2im(dtok . W_patch_embed) (autograd of deit:174).  patch divides H and W.
 *   ppf_grad_box_mass     g fp32 [R][C][H][W], box int32 [R][4] = (y0, y1, x0, x1), half-open (the layout of ppf_act_box; the part
 *                         outside the image is ignored; 16-byte aligned): per row total[r] = sum |g| and inside[r] = sum |g| over the box,
 *                         both fp64.  A non-finite element counts as 0 in both sums; nonfinite[r] (int32, may be NULL) = how many there
 *                         were.  One workgroup per row, fixed reduction order: repeated runs are bit-identical.  C*H*W <= 2^31 - 1.
 *   ppf_pgd_step_box      one projected signed-gradient step on x fp32 [R][C][H][W] in place, x0 / g of the same shape, with per-channel
 *                         alpha3 / eps3 / lo3 / hi3 fp32 [C] on the device and dir = +1 (ascend) or -1 (descend).  Outside the box of row r:
 *                           x <- min(max(x + dir * alpha_c * sign(g), max(x0 - eps_c, lo_c)), min(x0 + eps_c, hi_c)),
 *                         sign(+-0) = sign(NaN) = 0; inside the box: x <- x0.  Plain fp32, every operation rounded once (dir * alpha_c *
 *                         sign is exact, so a fused multiply-add and the unfused form agree): bit-exact to interpret.pgd_step_box
 *                         (device=False) for finite x and x0.  16-byte accesses when W % 4 == 0 and x, x0, g are 16-byte aligned. */
int ppf_col2im_patch_f32(const float* cols, float* img, int B, int C, int H, int W, int patch, ppf_stream_t stream);
int ppf_grad_box_mass(const float* g, const int* box, int R, int C, int H, int W, double* inside, double* total, int* nonfinite,
                      ppf_stream_t stream);
int ppf_pgd_step_box(float* x, const float* x0, const float* g, const int* box, const float* alpha3, const float* eps3, const float* lo3,
                     const float* hi3, float dir, int R, int C, int H, int W, ppf_stream_t stream);
/* last_layer / last_layer_global (protopformer.py:126-131, 314-316): C = alpha * A B^T + beta * C, arbitrary strides */
int ppf_sgemm(const float* A, const float* Bm, float* C, int M, int N, int K, int64_t sam, int64_t sak, int64_t sbn, int64_t sbk,
              int ldc, float alpha, float beta, float* workspace, int64_t workspace_floats, ppf_stream_t stream);
/* Two such products with the same M in one launch + one ordered reduction: out_i = alpha_i A_i B_i^T (may be NULL) and
 * sum = c0 A0 B0^T + c1 A1 B1^T (may be NULL; N0 == N1): logits = g * logits_global + (1 - g) * logits_local (protopformer.py:314-316)
 * and the two input gradients of that layer. */
int64_t ppf_sgemm_pair_workspace(int M, int N0, int K0, int N1, int K1);
int ppf_sgemm_pair(const float* A0, const float* B0, float* out0, int N0, int K0, int64_t sam0, int64_t sak0, int64_t sbn0, int64_t sbk0,
                   int ldo0, float alpha0, const float* A1, const float* B1, float* out1, int N1, int K1, int64_t sam1, int64_t sak1,
                   int64_t sbn1, int64_t sbk1, int ldo1, float alpha1, float* sum, int ldsum, float c0, float c1, int M, float* workspace,
                   int64_t workspace_floats, ppf_stream_t stream);
int ppf_axpby(const float* x, const float* y, float* out, float a, float b, int64_t n, ppf_stream_t stream);
/* out = a x + b y + c z: loss = CE + ppc_cov_coe * cov + ppc_mean_coe * mean in one launch (tools/engine_proto.py:61-64) */
int ppf_axpbypcz(const float* x, const float* y, const float* z, float* out, float a, float b, float c, int64_t n, ppf_stream_t stream);

/* ---- interpretability post-processing (csrc/interp.hip; protopformer_amd/interpret.py resize_cubic, prototype_part_table,
 * find_high_activation_crop; reference eval_interpretability.py:206-226, main_visualize.py:44-66,381-398) ------------------------------
 * grids [M][g][g] fp32 (contiguous): the activation maps of M (image, prototype) pairs on the patch grid.  Every entry point below
 * up-samples them to S x S exactly as interpret.resize_cubic does (cv2.INTER_CUBIC: Keys kernel a = -0.75, half-pixel centres,
 * replicated border; fp64 without contraction, axis 0 then axis 1, taps added in index order, one cast to fp32): the values are
 * bit-identical to the host function's, so ties resolve as they do there.  1 <= g <= 64, 1 <= S <= 1024, and the LDS image
 * (g*g + 4*S + 32*g)*8 + 4*S bytes must fit 48 KiB; M >= 1.  Additions of ABI 10: no existing entry point changed.
 *   ppf_act_upsample     out [M][S][S] fp32 = the maps themselves (16-byte stores when S % 4 == 0 and out is 16-byte aligned).
 *   ppf_act_peak         the same arithmetic without writing the map: peak_val [M] = the map's maximum, peak_yx [M][2] int32 = (y, x) of
 *                        its FIRST occurrence in row-major order (np.where(up == up.max())[..][0]).  The part table is FUSED into this
 *                        launch: with parts != NULL it also writes table_u8 as ppf_act_part_table would (parts == NULL: table_u8 NULL
 *                        and maps_per_img / n_parts / half_size ignored).
 *   ppf_act_part_table   table_u8 [M][n_parts] uint8 (0/1) from given peaks = interpret.prototype_part_table: map m belongs to image
 *                        m / maps_per_img, parts [M / maps_per_img][n_parts][3] int32 = (valid, x, y) per part id, entry 1 iff valid and
 *                        y0 <= y <= y1 and x0 <= x <= x1 (inclusive on both ends, as in_bbox) for the box y0 = max(0, peak_y - half_size),
 *                        y1 = min(S, peak_y + half_size), likewise in x.
 *   ppf_act_order_stats  stats [M][2] fp32 = the values of ascending 0-based ranks k_lo and k_hi (k_lo <= k_hi <= k_lo + 1, k_hi < S*S)
 *                        among the S*S fp32 values of each map: an exact radix selection on the bit patterns, not a sort (-0 orders
 *                        below +0).  The caller interpolates the percentile threshold between the two on the host (numpy's own lerp).
 *   ppf_act_box          box [M][4] int32 = (y0, y1, x0, x1), end-exclusive, of the entries with (double)up >= thr[m] (thr: fp64 [M]);
 *                        (0, 1, 0, 1) when nothing passes (interpret.find_high_activation_crop).
 * NaN never wins a comparison (a map of NaNs: peak (0, 0), value -inf).  Deterministic: integer atomics only. */
int ppf_act_upsample(const float* grids, float* out, int M, int g, int S, ppf_stream_t stream);
int ppf_act_peak(const float* grids, int M, int g, int S, float* peak_val, int* peak_yx, const int* parts, int maps_per_img, int n_parts,
                 int half_size, void* table_u8, ppf_stream_t stream);
int ppf_act_part_table(const int* peak_yx, int M, int S, const int* parts, int maps_per_img, int n_parts, int half_size, void* table_u8,
                       ppf_stream_t stream);
int ppf_act_order_stats(const float* grids, int M, int g, int S, int k_lo, int k_hi, float* stats, ppf_stream_t stream);
int ppf_act_box(const float* grids, const double* thr, int M, int g, int S, int* box, ppf_stream_t stream);
/* Foreground focus (csrc/interp.hip, csrc/explain.hip; interpret.foreground_focus): does the model look at the object?  The reserved
 * tokens, the peaks and the positive mass of the prototype maps, and the class evidence, each against an annotated object box per image
 * (the energy-based pointing game of Wang et al., Score-CAM, 2020, on the positive part of the up-sampled map).  The reference has no
 * such pass.  Additions of ABI 10: no existing entry point changed.
 * An object box is int32 (y0, y1, x0, x1), half-open, in pixels of the S x S model input (the layout ppf_act_box writes and
 * ppf_grad_box_mass reads).  Every entry point clips it to [0, S] per coordinate; a box whose upper end is not above its lower end is
 * empty, and an empty box is accepted.
 *   ppf_act_focus        grids [M][g][g] as above (the same limits on g, S and LDS as ppf_act_peak), obj [M / maps_per_img][4]: map m
 *                        belongs to image m / maps_per_img (M a multiple of maps_per_img >= 1).  One workgroup per map, the map never
 *                        written.  peak_val [M], peak_yx [M][2]: bit-identical to ppf_act_peak on the same maps (first occurrence in
 *                        row-major order, NaN never wins, a map of NaNs gives (0, 0) with value -inf).  hit [M] int32 = 1 iff
 *                        y0 <= peak_y < y1 and x0 <= peak_x < x1.  inside [M], total [M] fp64 = the sum of max(v, 0) over the finite fp32
 *                        values v of the up-sampled map inside the box and over the whole map, every term exact; the summation order is
 *                        fixed by the thread mapping and otherwise unspecified.  nonfinite [M] int32 (may be NULL) = how many values were
 *                        NaN or +-inf; they add 0 to both sums.  No floating-point atomics: repeated runs are bit-identical.
 *   ppf_focus_box_terms  box [M][4] (as ppf_act_box writes it), obj [M / maps_per_img][4] -> terms [M][4] int32 = (intersection area, box
 *                        area, object area, union area) of the two boxes, both clipped to [0, S]^2.  Integers only.  1 <= S <= 32768.
 *   ppf_reserve_focus    idx [B][T] int32 = the grid cells of the reserved tokens on the g x g grid of patch x patch pixel cells
 *                        (S = g * patch <= 32768), obj [B][4] -> out [B][4] int32 = (pixels of the reserved cells inside the box: the sum
 *                        of the exact rectangle overlaps; reserved cells whose centre pixel (cy * patch + patch / 2, cx * patch + patch / 2)
 *                        is inside; all g*g cells whose centre is inside; idx entries inside [0, g*g)).  An idx entry outside [0, g*g) is
 *                        skipped everywhere; a cell listed twice counts twice.  token_attn [B][g*g] fp32 not NULL: also attn [B][2] fp64
 *                        = the rollout score summed over the cells with centre inside and over all cells, non-finite scores counting
 *                        0 (fixed order).  token_attn and attn are both given or both NULL.  T * patch^2 <= 2^31 - 1.
 *   ppf_evidence_focus   the local branch's evidence for classes [B][M] int32 (1 <= M <= 8), one wave per (sample, class) row: the
 *                        contribution of prototype p is fl(act_max[b][p] * fl(scale * weight[c][p])), ppf_explain_topk's two roundings;
 *                        its cell is idx[b][argmax[b][p]] and it is "located" when that argmax lies in [0, T) and the cell in [0, g*g)
 *                        (argmax == NULL, the k = 1 model: the cell is idx[b][0]).  ev [B][M][4] fp64 = the sums over (own class and
 *                        centre inside obj[b], own class and not inside, other classes and inside, other classes and not inside), own
 *                        class meaning p / ppc == c; a prototype that is not located counts as not inside.  The four sums together are
 *                        the branch's share of logits[b][c], so non-finite terms are included, as in ppf_explain_topk's evidence.
 *                        cnt [B][M][4] int32 = the number of terms of each sum.  A class outside [0, C): zeros, nothing read out of
 *                        range.  act_max [B][P], argmax [B][P], idx [B][T], weight [C][P], obj [B][4]; P % ppc == 0, T >= 1. */
int ppf_act_focus(const float* grids, const int* obj, int M, int g, int S, int maps_per_img, float* peak_val, int* peak_yx, int* hit,
                  double* inside, double* total, int* nonfinite, ppf_stream_t stream);
int ppf_focus_box_terms(const int* box, const int* obj, int M, int maps_per_img, int S, int* terms, ppf_stream_t stream);
int ppf_reserve_focus(const int* idx, const int* obj, const float* token_attn, int B, int T, int g, int patch, int* out, double* attn,
                      ppf_stream_t stream);
int ppf_evidence_focus(const float* act_max, const int* argmax, const int* idx, int T, const float* weight, float scale, int ppc,
                       const int* classes, const int* obj, int g, int patch, int B, int P, int C, int M, double* ev, int* cnt,
                       ppf_stream_t stream);
/* Stability score (Huang et al., ICCV 2023: does a prototype point at the same parts when the input is perturbed?) next to the
 * consistency score, both accumulated on the device.  Additions of ABI 10: no existing entry point changed.
 *   ppf_add_gauss_noise    out[b][e] = fmaf(sigma, n(seed, image_id[b], e), x[b][e]) on fp32 [B][n_per_img]; out may be x.  n is a standard
 *                          normal from Philox4x32-10 with key = seed and counter = (e/4 low, e/4 high, image id low, image id high): one
 *                          call yields the normals of elements 4q .. 4q+3 by two Box-Muller pairs, u0 = ((r.x >> 8) + 0.5) / 2^24,
 *                          u1 = (r.y >> 8) / 2^24, n0 = sqrt(-2 ln u0) cos(2 pi u1), n1 = sqrt(-2 ln u0) sin(2 pi u1), n2 / n3 likewise from
 *                          (r.z, r.w); accurate logf / sincospif.  The noise of an image depends on (seed, image id, element) only, not
 *                          on the batch size, the position in the batch or the number of calls.  image_id_i64 [B] int64.  16-byte loads and
 *                          stores when n_per_img % 4 == 0 and both pointers are 16-byte aligned, scalar otherwise.  B >= 1,
 *                          1 <= n_per_img <= 2^31, sigma finite and >= 0 (else PPF_ERR_SHAPE).
 *   ppf_part_meter_update  adds a batch into int32 accumulators hits [C][ppc][n_parts], visible [C][n_parts], stable [C][ppc], images [C],
 *                          bad [1]: for image b of class c = label[b]: images[c] += 1, visible[c][q] += (parts[b][q].valid != 0),
 *                          hits[c][p][q] += table[b][p][q], and with table_noisy_u8 != NULL stable[c][p] += 1 when rows p of the two tables
 *                          agree in all n_parts entries.  table_u8 / table_noisy_u8 [B][ppc][n_parts] uint8 as ppf_act_peak writes them,
 *                          parts [B][n_parts][3] int32 (valid, x, y).  A label outside [0, C) adds one to bad[0] and nothing else.
 *                          Integer atomics only: any split of the same images into batches, in any order, gives the same accumulators. */
int ppf_add_gauss_noise(const float* x, float* out, int B, int64_t n_per_img, const void* image_id_i64, float sigma, uint64_t seed,
                        ppf_stream_t stream);
int ppf_part_meter_update(const void* table_u8, const void* table_noisy_u8, const int* parts, const void* label_i64, int B, int ppc, int n_parts,
                          int C, int* hits, int* visible, int* stable, int* images, int* bad, ppf_stream_t stream);

/* ---- streaming kernels -------------------------------------------------------------------------------------------- */
int ppf_cast_f32_bf16(const float* in, void* out, int64_t n, ppf_stream_t stream);
/* bf16 -> fp32 (exact; n % 8 == 0): the optional bf16 wire format of the gradient all-reduce (engine.GradSync payload='bf16';
 * replaces nothing in the reference -- main.py:369-371 exchanges fp32 through DistributedDataParallel) */
int ppf_cast_bf16_f32(const void* in, float* out, int64_t n, ppf_stream_t stream);
/* PatchEmbed unfold (timm PatchEmbed conv k=s=patch, deit:174): img [B][C][H][W] -> cols bf16 [B*gh*gw][C*p*p] */
int ppf_im2col_patch(const float* img, void* cols, int B, int C, int H, int W, int patch, ppf_stream_t stream);
/* cls token + position embedding (deit:176-178 lead=1; cait:307-309 lead=0) and its backward */
int ppf_assemble_tokens(const float* tok, const float* cls, const float* pos, float* x, int B, int Np, int D, int lead,
                        ppf_stream_t stream);
int ppf_assemble_tokens_bwd(const float* dx, void* dtok, float* dpos, float* dcls, int B, int Np, int D, int lead,
                            ppf_stream_t stream);
/* backward of the add-on Sigmoid (protopformer.py:113): dz = bf16(df*f*(1-f)), dbias += column sums.  partial (>=
 * ppf_sigmoid_bwd_blocks(rows)*cols floats) makes the column sums a fixed-order two-pass reduction; NULL = fp32 atomics. */
int ppf_sigmoid_bwd_blocks(int rows);
int ppf_sigmoid_bwd(const float* df, const float* f, void* dz, float* dbias, int rows, int cols, float* partial, size_t partial_bytes,
                    ppf_stream_t stream);
/* fused AdamW (+EMA, +bf16 re-cast) over flat buffers (tools/create_optimizer.py:92, engine_proto.py:80-81) */
int ppf_adamw_step(float* p, const float* g, float* m, float* v, float* ema, void* p16, int64_t n, int nseg,
                   const int64_t* seg_bounds, const float* seg_lr, const float* seg_wd, float beta1, float beta2, float eps,
                   int step, float ema_decay, float grad_scale, ppf_stream_t stream);
/* The same step with every step-dependent scalar in DEVICE memory: hyper[0..7] lr per segment, [8..15] weight decay per segment,
 * [16] 1-beta1^t, [17] sqrt(1-beta2^t), [18] gradient scale (1/world), [19] clip coefficient (ppf_clip_grad_scale; 1 = off).
 * Nothing step-dependent is baked into the launch, so a captured HIP graph of the train step can be replayed
 * (lr schedule tools/create_scheduler.py:20-32 keeps working: the host refreshes `hyper` before each replay). */
int ppf_adamw_step_dev(float* p, const float* g, float* m, float* v, float* ema, void* p16, int64_t n, int nseg,
                       const int64_t* seg_bounds, const float* hyper, float beta1, float beta2, float eps, float ema_decay,
                       ppf_stream_t stream);
/* ppf_adamw_step_dev with the reference's per-step non-finite-loss check (tools/engine_proto.py:66-70: print + sys.exit(1) in front of
 * optimizer.step()) evaluated on the device: `loss` = the step's loss scalar (device); if it is NaN / inf nothing is updated and
 * *nonfinite_flag = 1 (read by the host at its logging cadence: engine.train_one_epoch).  loss == NULL && flag == NULL: no check. */
int ppf_adamw_step_guarded(float* p, const float* g, float* m, float* v, float* ema, void* p16, int64_t n, int nseg,
                           const int64_t* seg_bounds, const float* hyper, float beta1, float beta2, float eps, float ema_decay,
                           const float* loss, int* nonfinite_flag, ppf_stream_t stream);
/* hyper[0..n) <- host_vals[0..n) (n <= 20), passed by value at enqueue time (safe when the host runs ahead of the device) */
int ppf_hyper_set(float* hyper, const float* host_vals, int n, ppf_stream_t stream);
/* clip_grad_norm_ (timm dispatch_clip_grad 'norm' via NativeScaler, engine_proto.py:74-76, main.py --clip-grad): hyper[19] =
 * min(1, max_norm / (pre_scale*||g||_2 + 1e-6)); partial = ppf_clip_grad_blocks() floats of scratch; norm_out optional. */
int ppf_clip_grad_blocks(void);
int ppf_clip_grad_scale(const float* g, int64_t n, float max_norm, float pre_scale, float* partial, float* hyper, float* norm_out,
                        ppf_stream_t stream);
/* timm DropPath factors floor(keep+U)/keep for all (slot, sample) pairs of one step (deit:71,79-80): out [nslot][B], keep [nslot]
 * (device).  Philox4x32-10 keyed by seed, counter = (state_u64[0], element); the launch advances state_u64[0] (device) by one. */
int ppf_droppath_scales(float* out, const float* keep, int nslot, int B, uint64_t seed, void* state_u64, ppf_stream_t stream);
/* token reservation plumbing (protopformer.py:156-162 gather of [cls, 1+idx...]): flat source rows of the reserved tokens,
 * row gather, and zero-filled row scatter (its backward). row_bytes % 16 == 0. */
int ppf_reserved_rows_map(const int* idx, int* rows, int B, int k, int N, ppf_stream_t stream);
int ppf_gather_rows(const void* src, const int* rows, void* dst, int nrows, int row_bytes, ppf_stream_t stream);
int ppf_scatter_rows(const void* src, const int* rows, void* dst, int nrows_src, int nrows_dst, int row_bytes, ppf_stream_t stream);
int ppf_memset_zero(void* ptr, size_t bytes, ppf_stream_t stream);
/* strided sub-matrix copy (bytes): dst[r][0..width) = src[r][0..width), rows rows, independent row pitches (torch.cat / slicing of the
 * class-attention stage, cait:314-316, kept on the library's launch path) */
int ppf_copy_2d(void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width, int64_t rows, ppf_stream_t stream);
/* input pipeline finisher (tools/datasets.py:280-336: ToTensor + Normalize; timm RandomErasing 'pixel'): uint8 [B][H][W][3] frames
 * -> fp32 [B][3][H][W] = (x/255 - mean)/std; rects [B][4] = (y, x, h, w) erase rectangles filled with N(0,1) noise (h == 0: none;
 * rects == NULL: no erasing); mean3 / std3 are HOST pointers; state_u64 (device, optional) = step counter mixed into the noise key. */
int ppf_image_finish_u8(const void* in_u8_hwc, float* out_nchw, int B, int H, int W, const float* mean3, const float* std3,
                        const int* rects, uint64_t seed, const void* state_u64, ppf_stream_t stream);
/* Device-resident data sets (protopformer_amd/csrc/device_data.hip): the decoded originals stay on the device as one flat uint8 buffer of HWC frames and
 * every batch is cropped, flipped and augmented there, bit-equal to Pillow (the CPU path of data.build_transform: tools/datasets.py:280-336
 * with timm's RandomResizedCropAndInterpolation, RandomHorizontalFlip and rand-m9-mstd0.5-inc1).  The host draws, the device applies.
 * Additions of ABI 10: no existing entry point changed.  This file is compiled without floating-point contraction.
 *
 * ppf_resize_crop_u8: out uint8 [B][H][W][3] = PIL Image.resize((ow, oh), filter, box) of sample b's frame, cropped to the window
 * rows [y0, y0 + H) x columns [x0, x0 + W) of that (oh, ow) result, then mirrored left-right when the flag is set.  Only the window is
 * computed.  The plan is fp64 [B][PPF_RC_WORDS] = (frame offset in bytes into flat, frame h, w, box x0, y0, x1, y1, oh, ow, window y0,
 * x0, mirror).  plan_host is a HOST copy read during the call only: every sample is validated on it (the frame inside flat_bytes, the box
 * inside the frame and not empty, the window inside (oh, ow)) before anything is launched; plan_dev is the same table on the device.
 * Arithmetic, per axis (x: in0 = box x0, in1 = box x1, size = w, out = ow; y likewise), all of it Pillow's 8-bit resample:
 *   scale = (in1 - in0) / out, filterscale = max(1, scale), support = S * filterscale, ss = 1 / filterscale            (fp64)
 *   filter 3 (BICUBIC): S = 2, the weight below; filter 2 (BILINEAR, the square view of interp_eval): S = 1, weight max(0, 1 - |x|)
 *   for output coordinate xx: center = in0 + (xx + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)),
 *     xmax = min(size, (int)(center + support + 0.5))  -- the taps clamp at the FRAME, not at the box
 *   w_t = bicubic(((t + xmin) - center + 0.5) * ss) for t = 0 .. xmax - xmin - 1 with a = -0.5:
 *     |x| < 1: ((a + 2) |x| - (a + 3)) |x| |x| + 1;  |x| < 2: (((|x| - 5) |x| + 8) |x| - 4) a;  else 0
 *   ww = sum of w_t in tap order; w_t /= ww when ww != 0; k_t = (int)(w_t < 0 ? -0.5 + w_t * 2^22 : 0.5 + w_t * 2^22)
 *   The fp64 part runs on the device, one thread per output coordinate, IEEE + - * / only, no contraction.
 *   value = clip8((2^21 + sum_t p_t * k_t) >> 22) in int32, clip8 clamping to [0, 255].
 * The horizontal pass comes first over the source rows the window's vertical taps need; its result is rounded to uint8 (in the
 * workspace); the vertical pass runs over those rows.  workspace: ppf_resize_crop_workspace_bytes(plan_host, B, H, W, filter, flat_bytes) bytes,
 * 16-byte aligned (0 and ppf_last_error() for an invalid plan).  Limits: B, H, W >= 1, H, W, oh, ow <= 16384, at most 1024 taps per axis.
 *
 * RandAugment on uint8 [B][H][W][3] frames.  The plan is fp64 [B][PPF_AUG_SLOTS][PPF_AUG_WORDS] = (op, resample, p0 .. p5) on the device;
 * every entry point works on one slot, reads `in` and writes `out` (never in place) for the samples whose op is its own and leaves
 * the other samples of `out` alone.  op = index into data.RandAugment.OPS (PPF_AUG_*), PPF_AUG_SKIP = copy.  An op out of range copies.
 *   ppf_aug_hist       hist int32 [B][3][256] (zeroed by the call, integer atomics, exact at any launch shape): per-channel counts for
 *                      AutoContrast and Equalize; for ContrastIncreasing the counts of L = (19595 R + 38470 G + 7471 B + 2^15) >> 16 in
 *                      channel 0.  Other samples' counters stay zero.
 *   ppf_aug_lut_build  lut uint8 [B][3][256] of the table ops (other samples' tables are not written):
 *                      AutoContrast: lo / hi = first / last non-empty bin; hi <= lo: identity; else scale = 255.0 / (hi - lo),
 *                        offset = -lo * scale, lut[i] = clamp((int)(i * scale + offset), 0, 255)                       (fp64)
 *                      Equalize: with fewer than two non-empty bins or step = (H*W - hist[last non-empty]) / 255 == 0: identity; else
 *                        lut[i] = min(255, (step / 2 + sum_{j < i} hist[j]) / step)                                     (integer)
 *                      Invert 255 - i; Posterize i & ~(2^(8 - p0) - 1); Solarize i < p0 ? i : 255 - i; SolarizeAdd i < 128 ?
 *                        min(255, i + p0) : i; Brightness blend(0, i, p0); Contrast blend(m, i, p0) with
 *                        m = (int)(sum of L / (double)(H*W) + 0.5).
 *   blend(a, b, f)     Image.blend: alpha = (float)f; t = (float)a + alpha * (float)(b - a) in fp32, two roundings; 0 <= alpha <= 1:
 *                      (uint8)t (truncation); else t <= 0 -> 0, t >= 255 -> 255, else truncation.
 *   ppf_aug_apply      table ops: out = lut[channel][in]; ColorIncreasing: out = blend(L, in, p0) with the pixel's own L; skip: copy.
 *   ppf_aug_sharpness  SharpnessIncreasing: out = blend(s, in, p0), s = ImageFilter.SMOOTH: the one-pixel border (and every pixel when
 *                      H < 3 or W < 3) is the input; inside t = 0.5f, then for rows y + 1, y, y - 1 in this order
 *                      t += (in[x-1] * k0 + in[x] * k1 + in[x+1] * k2) in fp32 with k = 1.0f/13.0f, the centre 5.0f/13.0f;
 *                      t <= 0 -> 0, t >= 255 -> 255, else truncation.
 *   ppf_aug_affine     Rotate, ShearX, ShearY, TranslateXRel, TranslateYRel: Image.transform(AFFINE, (p0 .. p5), resample, fill).  The
 *                      matrix comes from the host (the rotation's sine and cosine as Image.rotate rounds them); the device uses no
 *                      transcendental.  Per output pixel, in fp64: xin = p0 * (x + 0.5) + p1 * (y + 0.5) + p2, yin = p3 * (x + 0.5) +
 *                      p4 * (y + 0.5) + p5; outside [0, W) x [0, H): the fill colour; else xin -= 0.5, yin -= 0.5, xf = floor(xin),
 *                      dx = xin - xf (y likewise); column and row indices clamp to the frame.
 *                      resample 2 (BILINEAR): row value a + (b - a) * dx over columns xf, xf + 1; rows yf and yf + 1 (a row outside
 *                        the frame repeats the previous row's value); v = v1 + (v2 - v1) * dy.
 *                      resample 3 (BICUBIC): c(v1, v2, v3, v4, d) = v2 + d * ((-v1 + v3) + d * ((2 * (v1 - v2) + v3 - v4) + d *
 *                        (-v1 + v2 - v3 + v4))) over columns xf - 1 .. xf + 2, then over rows yf - 1 .. yf + 2 (row yf - 1 clamps
 *                        into the frame, each later row outside the frame repeats the previous row's value).
 *                      Both filters: v <= 0 -> 0, v >= 255 -> 255, else truncation (no rounding). */
#define PPF_RC_WORDS 12
#define PPF_AUG_WORDS 8
#define PPF_AUG_SLOTS 2
#define PPF_AUG_SKIP (-1)
#define PPF_AUG_AUTOCONTRAST 0
#define PPF_AUG_EQUALIZE 1
#define PPF_AUG_INVERT 2
#define PPF_AUG_ROTATE 3
#define PPF_AUG_POSTERIZE 4
#define PPF_AUG_SOLARIZE 5
#define PPF_AUG_SOLARIZE_ADD 6
#define PPF_AUG_COLOR 7
#define PPF_AUG_CONTRAST 8
#define PPF_AUG_BRIGHTNESS 9
#define PPF_AUG_SHARPNESS 10
#define PPF_AUG_SHEAR_X 11
#define PPF_AUG_SHEAR_Y 12
#define PPF_AUG_TRANSLATE_X 13
#define PPF_AUG_TRANSLATE_Y 14
size_t ppf_resize_crop_workspace_bytes(const double* plan_host, int B, int H, int W, int filter, int64_t flat_bytes);
int ppf_resize_crop_u8(const void* flat_u8, int64_t flat_bytes, const double* plan_host, const double* plan_dev, int B, int H, int W,
                       int filter, void* workspace, size_t workspace_bytes, void* out_u8, ppf_stream_t stream);
int ppf_aug_hist(const void* in_u8, const double* plan_dev, int slot, int B, int H, int W, int* hist, ppf_stream_t stream);
int ppf_aug_lut_build(const int* hist, const double* plan_dev, int slot, int B, int H, int W, void* lut_u8, ppf_stream_t stream);
int ppf_aug_apply(const void* in_u8, const double* plan_dev, int slot, const void* lut_u8, int B, int H, int W, void* out_u8,
                  ppf_stream_t stream);
int ppf_aug_sharpness(const void* in_u8, const double* plan_dev, int slot, int B, int H, int W, void* out_u8, ppf_stream_t stream);
int ppf_aug_affine(const void* in_u8, const double* plan_dev, int slot, int B, int H, int W, int fill_r, int fill_g, int fill_b,
                   void* out_u8, ppf_stream_t stream);
/* PartsWorld (csrc/synth.hip; the shared arithmetic is csrc/synth_plan.h, checked on the host by tests/synth_plan_check.cpp): a data set
 * the library renders itself, with classes defined by parts and, per image, the object's box, every part's place and the class table that
 * says which parts tell two classes apart -- annotations true by construction (the idea of FunnyBirds, Hesse et al., ICCV 2023).  The
 * reference has no such pass.  Additions of ABI 10: no existing entry point changed.  Integers only, so the numpy referees
 * (data.partsworld_*) and the kernels agree bit for bit.
 *   spec      C classes in [2, 1024], K parts per object in [1, 8], D distractors in [0, 8], frame H in [32, 1024], W in [32, 1024] and a
 *             multiple of 16, g background cells per side in [1, 8], noise amplitude in [0, 32], seed (64 bits).  Both entry points take
 *             all of them and refuse, before any device call and by name, K, D, C, C > A^K, H, W, W % 16, g, noise, B < 1 and an out or
 *             partmap that is not 16-byte aligned: PPF_ERR_SHAPE every one of them; a null pointer is PPF_ERR_ARG.
 *   ids       image ids int64 [B], >= 0.  label = id % C.  (data.PartsWorld: train ids 0 .. n_train - 1, test ids test_id_base + i.)
 *   classes   A = 24 attributes = shape * 6 + colour; shapes disk, square, diamond, ring; colours red (220, 40, 40), green (40, 180, 60),
 *             blue (50, 80, 220), yellow (235, 210, 40), magenta (200, 60, 200), cyan (40, 200, 210).  class_parts[c][k] = digit k of c in
 *             base A: a function of the spec alone, and two classes below A^K differ in a digit; hence C <= A^K.
 *   draws     Philox4x32-10, key = seed, counter = (item, 0xC0000001, id low, id high); u = word >> 8 is a 24-bit draw and
 *             range(u, n) = (u * n) >> 24 in [0, n).  Items: 0 the object (x: half-size, y: centre x, z: centre y, w: the part forced
 *             visible); 1 + k part k (x: visible, y: jitter x, z: jitter y); 9 + 2d distractor d (x: on, y: attribute, z: radius) and
 *             10 + 2d (x: centre x, y: centre y); 32 + e / 4, word e % 4: channel e % 3 of background node e / 3.
 *   object    m = min(H, W); hs = 5m/16 + range(u, 13m/32 - 5m/16 + 1); ox = hs + range(u, W - 2 hs), oy likewise with H: the body is the
 *             square |x - ox| <= hs, |y - oy| <= hs, colour (112, 112, 112); box = (ox - hs, oy - hs, ox + hs + 1, oy + hs + 1), upper
 *             edges exclusive, inside the frame because 2 hs + 1 <= m.
 *   parts     pitch p = (2 hs + 1) / 3, jitter j = (p - 1) / 8, radius r = (p - 1) / 2 - j >= 3.  Part k sits on cell (0, 2, 6, 8, 1, 3, 5,
 *             7)[k] of the 3 x 3 grid of pitch p around (ox, oy) (row-major, the centre cell is left to the body): cx = ox + (cell % 3 - 1)
 *             * p + range(u, 2j + 1) - j, cy likewise with cell / 3.  Since 2 (r + j) <= p - 1 a part stays in its cell: the parts of one
 *             object are disjoint and inside the box by construction.  visible = (u < 3 * 2^22) or k == range(u of item 0 w, K): at
 *             least one part is visible.  attribute = class_parts[label][k].
 *   others    distractor d: on = u < 2^23, attribute = range(u, 24), r = m/16 + range(u, m/8 - m/16 + 1), cx = r + range(u, W - 2r),
 *             cy = r + range(u, H - 2r): inside the frame, possibly under the object.  Node channel = 64 + range(u, 128).
 *   shapes    with dx, dy the offsets from the centre and d2 = dx^2 + dy^2: disk d2 <= r^2; square max(|dx|, |dy|) <= r; diamond
 *             |dx| + |dy| <= r; ring d2 <= r^2 and not (r^2 / 16 < d2 < r^2 / 4), taken as 16 d2 > r^2 and 4 d2 < r^2: an annulus with
 *             a centre dot, so every shape contains its centre and lies inside max(|dx|, |dy|) <= r.
 *   scene     int32 [B][PPF_SYNTH_WORDS]: word 0 the label, 1 .. 4 the box, 5 + 5k .. part k as (visible, cx, cy, r, attribute), 45 + 5d
 *             .. distractor d as (on, cx, cy, r, attribute), 85 + q node q = i * (g + 1) + j as r | g << 8 | b << 16; the rest zero.
 *             The table is the annotation.
 *   pixels    painter's order.  1. background: ch = ceil(H / g), cw = ceil(W / g), i = y / ch, ry = y % ch, j and rx likewise; per
 *             channel floor(((ch-ry) * ((cw-rx) * n[i][j] + rx * n[i][j+1]) + ry * ((cw-rx) * n[i+1][j] + rx * n[i+1][j+1])) / (ch * cw)).
 *             2. the distractors that are on, in index order.  3. the body.  4. the visible parts in index order.  Then, when noise > 0,
 *             per pixel q = y * W + x one Philox call with counter (q, 0xC0000002, id low, id high): channel c gets
 *             + range(word c >> 8, 2 noise + 1) - noise and is clamped to [0, 255].  A frame depends on (spec, id) alone.
 *   ppf_synth_scene   scene of ids; one lane per image.
 *   ppf_synth_render  out uint8 [B][H][W][3] from the scene table (the ids are read for the noise only); partmap uint8 [B][H][W] or NULL:
 *                     the code of the topmost primitive, 0 background, 1 distractor, 2 body, 3 + k part k.  The caller's buffers hold
 *                     B * H * W * 3 and B * H * W bytes from the pointers on; nothing else is written.  A lane owns 16 pixels of a row
 *                     and writes them as three 16-byte stores (the partmap as one); the image's scene row is staged in LDS. */
#define PPF_SYNTH_WORDS 168
int ppf_synth_scene(int* scene, const void* ids_i64, int B, int C, int K, int D, int H, int W, int g, int noise, uint64_t seed, ppf_stream_t stream);
int ppf_synth_render(void* out_u8, void* partmap_u8, const int* scene, const void* ids_i64, int B, int H, int W, int C, int K, int D, int g,
                     int noise, uint64_t seed, ppf_stream_t stream);
/* Part interventions on PartsWorld (csrc/synth.hip, csrc/partcheck.hip; interpret.part_interventions / part_attribution / part_agreement):
 * the scene table is the render's input, so a row edited and rendered again under the same id is the same image without part k, without
 * the distractors, or with another class's part -- the noise is keyed by (id, pixel), so only the edited pixels differ (the protocol of
 * FunnyBirds, Hesse et al., ICCV 2023).  The reference has no such pass.  Additions of ABI 10: no existing entry point changed.
 *   ppf_synth_edit  scene int32 [B][PPF_SYNTH_WORDS] as ppf_synth_scene writes it; edits int32 [B][E][2] = (op, arg) per image and edit;
 *                   out int32 [B][E][PPF_SYNTH_WORDS] the edited rows, changed int32 [B][E].  One launch, integers only; the rule is
 *                   csrc/synth_plan.h's synth_edit_valid / synth_edit_word (checked on the host by tests/synth_edit_check.cpp), and the
 *                   numpy referee data.partsworld_edit(device=False) agrees bit for bit.  Ops:
 *                     0 COPY             the row as it is;
 *                     1 PARTS_OFF        arg a bit mask over the parts: visible := 0 for every part k with bit k set;
 *                     2 DISTRACTORS_OFF  arg a bit mask over the distractors: on := 0 for the masked ones;
 *                     3 BACKGROUND       arg = r | g << 8 | b << 16: every one of the (g + 1)^2 nodes takes this colour (a flat background);
 *                     4 PART_ATTR        arg = k | attr << 8: part k's attribute becomes attr in [0, 24).
 *                   changed = 1 when the edit alters a word of a primitive that is on before or after the edit, or alters a node; else 0
 *                   (hiding an invisible part, recolouring an invisible part, an attribute set to its own value).  An edit is invalid
 *                   when its op is unknown, a mask bit is at or above K (or D), k >= K, attr >= 24, or a colour is above 0xFFFFFF (a
 *                   negative arg is invalid for every op but COPY): the row is copied unchanged and changed = -1 -- the table lives on
 *                   the device, so it cannot be refused on the host; ops.synth_edit raises on any -1 after its one read.  An edit list
 *                   is applied to the SAME row, edit by edit; a chain (the counterfactual: PART_ATTR for every part that differs from
 *                   another class's row) is a sequence of calls with the previous out as scene, made by the Python wrapper
 *                   (interpret.part_interventions).  Refused by name: B < 1, E < 1, B * E beyond the grid, K, D, g (PPF_ERR_SHAPE), a null
 *                   pointer (PPF_ERR_ARG).  C is taken for the spec's sake and checked like ppf_synth_scene's.
 *   view rule       the square view of S x S pixels of an H x W frame (data.partsworld_view: the bilinear (S, S) resize the eval loaders
 *                   make) takes the primitive code of view pixel (y, x) from frame pixel (PPF_VIEW_SRC(y, H, S), PPF_VIEW_SRC(x, W, S)):
 *                   ((2 i + 1) * n) / (2 S) in integers, nearest by pixel centre, always inside the frame.
 *   ppf_part_mass   score fp32 [R][S][S] (the [B, M, S, S] maps of interpret.pixel_scores; row r belongs to image r / rows_per_img),
 *                   partmap uint8 [R / rows_per_img][H][W] with codes 0 .. 2 + K.  Per row r and code c in [0, 3 + K):
 *                   pos[r][c] = sum max(s, 0) and neg[r][c] = sum max(-s, 0) in fp64 over the view pixels whose code (view rule) is c,
 *                   count[r][c] int32 the number of those pixels.  A non-finite score adds 0 to both sums (its pixel is still counted
 *                   under its code); a code above 2 + K is added and counted nowhere; nonfinite[r] int32 (or NULL) counts the pixels
 *                   that are either.  One workgroup per row; lane partials, wave reduction by shuffles, the waves combined in wave
 *                   order: no floating-point atomics, bit-identical from run to run.  Every term is exact in fp64, so any order is
 *                   within n * 2^-53 * sum |s| of the exact sum of a bin of n terms.  16-byte score loads when S % 4 == 0 and score is
 *                   16-byte aligned, single elements otherwise.  Refused by name (PPF_ERR_SHAPE): K outside [1, 8], S < 1, H < 1, W < 1,
 *                   rows_per_img < 1, R < 1, R % rows_per_img != 0, S * S > 2^31 - 1, H * W > 2^31 - 1; a null pointer other than
 *                   nonfinite is PPF_ERR_ARG.  The numpy referee is interpret.part_mass(device=False). */
#define PPF_VIEW_SRC(i, n, S) ((int)(((2 * (int64_t)(i) + 1) * (int64_t)(n)) / (2 * (int64_t)(S))))
int ppf_synth_edit(int* out, int* changed, const int* scene, const int* edits, int B, int E, int C, int K, int D, int g, ppf_stream_t stream);
int ppf_part_mass(const float* score, const void* partmap_u8, int R, int rows_per_img, int S, int H, int W, int K, double* pos, double* neg,
                  int* count, int* nonfinite, ppf_stream_t stream);
/* Mixup / CutMix of the device batch (timm 0.5.4 Mixup, tools/engine_proto.py:47-48, main.py:325-335).  The per-sample parameter
 * table is int32 [B][PPF_MIX_WORDS]: kind (0 untouched, 1 blend, 2 box paste), the box rows [yl, yh) and columns [xl, xh), and two
 * fp32 weights stored as their bits.  Sample i is mixed with sample j = B-1-i as it was before the call:
 *   blend: x_i = fl(fl(x_i * w_self) + fl(x_j * w_other))   (no FMA: bit-exact to timm's torch arithmetic for the same weights)
 *   box:   x_i[:, yl:yh, xl:xh] = x_j[:, yl:yh, xl:xh]       (w_self / w_other then only serve ppf_mixup_target)
 * ppf_mixup_apply: x fp32 [B][Cc][H][W] (device, in place).  table_host is a HOST pointer (pinned, unchanged until the copy has run
 * on `stream`), validated (kind in range, box inside the image) and copied to table_dev (device, B*PPF_MIX_WORDS int32) on `stream`
 * before the launch; no launch when every kind is 0. */
#define PPF_MIX_KIND 0
#define PPF_MIX_YL 1
#define PPF_MIX_YH 2
#define PPF_MIX_XL 3
#define PPF_MIX_XH 4
#define PPF_MIX_WSELF 5
#define PPF_MIX_WOTHER 6
#define PPF_MIX_WORDS 8
int ppf_mixup_apply(float* x, const int* table_host, int* table_dev, int B, int Cc, int H, int W, ppf_stream_t stream);
/* timm mixup_target: target [B][C] fp32 = w_self_b * onehot_s(label_b) + w_other_b * onehot_s(label_{B-1-b}) with onehot_s = off_value
 * everywhere and on_value at the label (off = smoothing / C, on = 1 - smoothing + off, rounded to fp32 by the caller); label_i64 [B]
 * and lam (device): w_self_b = lam[b*lam_stride], w_other_b = lam[b*lam_stride + 1] (lam_stride 0: one pair for the whole batch;
 * the mixing table: lam = table_dev + PPF_MIX_WSELF, lam_stride = PPF_MIX_WORDS). */
int ppf_mixup_target(const void* label_i64, const float* lam, int lam_stride, float off_value, float on_value, float* target, int B,
                     int C, ppf_stream_t stream);
/* out = x * (*scalar_dev): chain rule with a device-resident upstream scalar (autograd of nn.CrossEntropyLoss, main.py:390) */
int ppf_scale_by_scalar(const float* x, const float* scalar_dev, float* out, int64_t n, ppf_stream_t stream);

/* ---- fp32 verification path (forward only; PPNet.precise / PPF_PRECISE=1) ------------------------------------------------
 * Every operand and intermediate fp32, contractions through ppf_sgemm, exact-erf GELU: used by the parity tests to hold the whole
 * forward / loss to 1e-3 rel against the reference fixtures.  Same reference lines as the bf16 kernels above. */
int ppf_im2col_patch_f32(const float* img, float* cols, int B, int C, int H, int W, int patch, ppf_stream_t stream);
int ppf_layernorm_fwd_f32(const float* x, const int* row_map, const float* w, const float* b, float* y, int rows, int D, float eps,
                          ppf_stream_t stream);
/* in place on C[M][N]: kind 0 +bias | 1 gelu_erf(+bias) | 2 sigmoid(+bias) | 3 res + rowscale[m/rows_per_group]*colscale[n]*(C+bias) |
 * 4 relu(+bias) (the bottleneck add-on head, protopformer.py:90-107) */
int ppf_epilogue_f32(float* C, const float* bias, int kind, const float* res, const float* rowscale, int rows_per_group,
                     const float* colscale, int M, int N, ppf_stream_t stream);
/* deit:29-60 on fp32 qkv [B*N][3D]; headmean (optional) [B][N][NP] = mean over heads of the probabilities (deit:104) */
int ppf_attn_fwd_f32(const float* qkv, float* out, const float* policy, float* headmean, int NP, int B, int H, int N, int D,
                     int self_keep, int eps_n, ppf_stream_t stream);
/* cait:115-132 on fp32 qkv; headmean = mean over heads of the returned (post proj_w) attention (cait:328) */
int ppf_th_attn_fwd_f32(const float* qkv, const float* wl, const float* bl, const float* ww, const float* bw, float* out,
                        float* headmean, int NP, int B, int H, int N, int D, ppf_stream_t stream);
/* cait:50-90: q [B][D] cls rows, k / v [B*N1][D]; attn_mean [B][N1] = mean over heads of the probabilities */
int ppf_class_attn_fwd_f32(const float* q, const float* k, const float* v, const float* policy, float* attn_mean, float* out, int B,
                           int H, int N1, int D, ppf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PPF_HIP_H */
