/*
 * bem_hip.h -- C ABI of libbem_hip.so: the MI355X (gfx950) hot path of the Bayesian Enhancement
 * Model (two-stage N-sample Bayesian low-light enhancement).
 *
 * Conventions (all entry points)
 *   - plain device pointers + sizes, float32, NCHW / (B, C, L) contiguous unless a stride is given;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream),
 *     no internal synchronisation, no global state, re-entrant across streams -- the same contract
 *     as the reference's extension (selective_scan_oflex.cpp:232-233);
 *   - return value 0 = launched, non-zero = rejected (bad shape / null pointer / HIP launch error);
 *     bem_last_error() gives the message for the calling thread.  Nothing is launched on rejection.
 *   - "reference" paths below are relative to vfrantc/Bayesian-Enhancement-Model.
 *
 * The library has NO CPU path: without a gfx950 device the calls fail (hipErrorNoDevice).
 */
#ifndef BEM_HIP_H
#define BEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEM_OK 0
#define BEM_ERR_INVALID 1
#define BEM_ERR_LAUNCH 2

const char* bem_last_error(void);
int bem_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Operator seam: what basicsr/vmamba/models/csms6s.py and csm_triton.py call.
 * ------------------------------------------------------------------------------------------- */

/* Replaces selective_scan_cuda_oflex.fwd (kernels/selective_scan/csrc/selective_scan/cusoflex/
 * selective_scan_oflex.cpp:157-243; kernel selective_scan_fwd_kernel_oflex.cuh:67-180), f32 in/out.
 * u, delta, out: (batch, dim, L); A: (dim, dstate); Bm, Cm: (batch, ngroups, dstate, L);
 * D, delta_bias: (dim) or NULL.  dim % ngroups == 0, 1 <= dstate <= 256. */
int bem_selective_scan_fwd_f32(const float* u, const float* delta, const float* A, const float* Bm,
                               const float* Cm, const float* D, const float* delta_bias, float* out,
                               int batch, int dim, int L, int dstate, int ngroups, int delta_softplus,
                               void* stream);

/* The same call with u, delta, Bm, Cm in float16 (in_dtype 1) or bfloat16 (in_dtype 2), read as they are (8-byte aligned when
 * L % 4 == 0); A, D, delta_bias and out float32 -- the extension's input_t = at::Half / at::BFloat16 instantiations with
 * out_float = true (selective_scan_oflex.cpp:166-216; csms6s.py:85 passes oflex). */
int bem_selective_scan_fwd_in16(const void* u, const void* delta, const float* A, const void* Bm, const void* Cm, const float* D,
                                const float* delta_bias, float* out, int in_dtype, int batch, int dim, int L, int dstate,
                                int ngroups, int delta_softplus, void* stream);

/* Element casts for the 16-bit forms of the seam's backward (the extension converts inside its kernels, selective_scan_bwd_kernel_oflex.cuh:
 * 108-140; here the f32 kernel runs between two casts): dtype 1 = float16, 2 = bfloat16, round to nearest even, n elements. */
int bem_cast16_to_f32(const void* src, float* dst, int64_t n, int dtype, void* stream);
int bem_cast_f32_to16(const float* src, void* dst, int64_t n, int dtype, void* stream);

/* Replaces selective_scan_cuda_oflex.bwd (selective_scan_oflex.cpp:245-358, kernel selective_scan_bwd_kernel_oflex.cuh:73-289),
 * f32.  dout, du, ddelta: (batch, dim, L); dA (dim, dstate); dB, dC (batch, ngroups, dstate, L) f32; dD, ddelta_bias (dim)
 * or NULL exactly when D / delta_bias are NULL.  ws: scratch of bem_selective_scan_bwd_ws_elems(...) floats (the role of
 * the reference's opaque `x` blob; recomputed here, so the forward need not be re-run by the caller).  dA/dB/dC/dD/
 * ddelta_bias are zeroed by the call and accumulated with float atomics across batch / group members (run-to-run
 * last-bit differences, like the reference). */
int64_t bem_selective_scan_bwd_ws_elems(int batch, int dim, int L, int dstate);
int bem_selective_scan_bwd_f32(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                               const float* D, const float* delta_bias, const float* dout, float* ws, float* du,
                               float* ddelta, float* dA, float* dB, float* dC, float* dD, float* ddelta_bias,
                               int batch, int dim, int L, int dstate, int ngroups, int delta_softplus, void* stream);

/* Replaces cross_scan_fn / triton_cross_scan_flex (csm_triton.py:278-423): x (B,C,H,W) -> xs (B,4,C,H*W). */
int bem_cross_scan_f32(const float* x, float* xs, int B, int C, int H, int W, void* stream);
/* Replaces cross_merge_fn (csm_triton.py:446-471): ys (B,4,C,H,W) -> y (B,C,H*W). */
int bem_cross_merge_f32(const float* ys, float* y, int B, int C, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused SS2D core (replaces the cross_scan -> x_proj -> dt_proj -> selective_scan chain of
 * SS2D.forward_corev2, basicsr/vmamba/models/vmamba.py:657-684) for d_state = 1, K = 4.
 *
 *   x0  (B,C,L)        activations in row-major pixel order (directions 0 fwd / 2 rev)
 *   x1  (B,C,L)        the same planes transposed (W,H) (directions 1 fwd / 3 rev)
 *   xd0 (B,2,R+2,L)    x_proj output rows [dt_0..dt_{R-1}, B, C] of directions {0,2}, row-major order
 *   xd1 (B,2,R+2,L)    the same for directions {1,3}, transposed order
 *   dtw (4,C,R), dtb (4,C), A (4C) = -exp(A_logs), Ds (4C)
 *   y0  (B,C,L)        out: y(dir0) + y(dir2) in row-major order
 *   y1  (B,C,L)        out: y(dir1) + y(dir3) in transposed order
 *
 * The x_dbl tensors may be channel slices of wider buffers: xd*_bstride = elements between batch rows
 * (0 = contiguous 2*(R+2)*L; multiples of 4).  Lets one x_proj GEMM over the row-major planes produce all four
 * directions' rows, the {1,3} half being transposed afterwards (10 planes instead of a second pass over C planes).
 * ------------------------------------------------------------------------------------------- */
int bem_ss2d_scan_strided_f32(const float* x0, const float* x1, const float* xd0, const float* xd1,
                              const float* dtw, const float* dtb, const float* A, const float* Ds,
                              float* y0, float* y1, int B, int C, int L, int R, int64_t xd0_bstride, int64_t xd1_bstride,
                              void* stream);

/* Row-major in, row-major out: x (B,C,H,W) feeds both orientations and y1 (directions 1 + 3) comes back already in
 * (B,C,H,W) order -- a workgroup of the column-major orientation stages its planes in LDS, so neither the transposed copy
 * of x nor the transposed y exist in HBM.  xd1 stays in transposed pixel order (2 (R+2) small planes).  Plane sizes / ranks
 * of a 256x256 image only: bem_ss2d_scan_rm_supported(H, W, R) != 0. */
int bem_ss2d_scan_rm_supported(int H, int W, int R);
int bem_ss2d_scan_rm_f32(const float* x, const float* xd0, const float* xd1, const float* dtw, const float* dtb,
                         const float* A, const float* Ds, float* y0, float* y1, int B, int C, int H, int W, int R,
                         int64_t xd0_bstride, int64_t xd1_bstride, void* stream);

/* Fused SS2D core for d_state = N > 1 (SS2D with ssm_d_state from the option file, vmamba.py:251-253,345-346,442,518-519: x_proj emits
 * R + 2N rows per direction, A_logs is (4C, N), forward_corev2 splits [R, N, N] at :660-671).  The operands of bem_ss2d_scan_strided_f32
 * except:
 *   xd0, xd1 (B,2,R+2N,L)  rows [dt_0..dt_{R-1}, B_0..B_{N-1}, C_0..C_{N-1}] per direction; batch strides as above (0 = contiguous)
 *   A (4C, N) = -exp(A_logs)
 * Per direction y = sum_n C_n h_n + D x with h_n = exp(dl A_n) h_n + dl B_n x, dl = softplus(dt + dtb) (threshold 20).
 * 1 <= N <= 16 (bem_ss2d_scan_n_supported), 1 <= R <= 16.  The d_state = 1 path keeps the kernels above. */
int bem_ss2d_scan_n_supported(int N);
int bem_ss2d_scan_n_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dtw, const float* dtb,
                        const float* A, const float* Ds, float* y0, float* y1, int B, int C, int L, int R, int N,
                        int64_t xd0_bstride, int64_t xd1_bstride, void* stream);

/* The deterministic middle of SS2D (d_state = 1) on small planes as one kernel, one workgroup per sample with the sample's planes in LDS:
 *   y = (y_dir0 + y_dir2) + (y_dir1 + y_dir3), row-major, of xc = SiLU(dw3x3(t) + bias), x_dbl = x_proj(xc) and the four-direction scan.
 *   t   (B,C,H,W)          the in_proj output
 *   dww (C,9) | (B,C,9)    depthwise weights, dww_bstride = 0 (shared) or the elements between samples
 *   dwb (C) | (B,C) | NULL depthwise bias, dwb_bstride likewise
 *   xw  (4(R+2),C)         raw f32 x_proj rows, directions in the order [0 | 2 | 1 | 3], per direction [dt_0..dt_{R-1}, B, C]
 *   dtw (4,C,R), dtb (4,C), A (4C) = -exp(A_logs), Ds (4C)
 *   y   (B,C,H,W)          out
 * Neither xc nor x_dbl nor a transposed plane reaches memory; no atomics (the same bits from launch to launch).
 * bem_ss2d_core_small_supported: C % 4 == 0, W % 4 == 0, R >= 1, H W = 64, 128 or 256 or below 64, and
 * 4 ((H W < 64 ? 5 C H W + 64 : C H W) + 4 (R + 2) (H W + C) + 4 C (R + 3)) bytes within 160 KiB of LDS.  t, y and xw on 16 bytes. */
int bem_ss2d_core_small_supported(int C, int H, int W, int R);
int bem_ss2d_core_small_f32(const float* t, const float* dww, int64_t dww_bstride, const float* dwb, int64_t dwb_bstride,
                            const float* xw, const float* dtw, const float* dtb, const float* A, const float* Ds, float* y,
                            int B, int C, int H, int W, int R, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pointwise (1x1) channel-mix GEMM with fused prologue / epilogue (argument block of bem_pw_gemm_x6_f32).  Replaces
 * Linear2d / nn.Conv2d(k=1) / LayerNorm2d+Linear2d chains (vmamba.py:42-63,123-133,702,715,1326-1334).
 *
 *   out[b][m][p] = act( sum_k W[b?][m][k] * pro(x)[b][k][p] + bias[b?][m] ) + res[b][m][p]
 *   pro: in_mode 0: x = x1 (K = C1) | 1: x = x1 + x2 (K = C1 = C2) | 2: x = cat(x1, x2) (K = C1 + C2);
 *        then LayerNorm over the K channels of each pixel when ln_w != NULL (eps = ln_eps).
 *   Wp : weights pre-packed by bem_pack_pw_weight_x6; w_bstride / bias_bstride = element stride
 *        between per-batch-element weight sets (0 = shared by the whole batch).
 *   act: 0 none, 1 PReLU with the single slope *prelu.
 *   out_mode 0: out (B,M,L).  out_mode 1: ConvTranspose2d(k=2,s=2) scatter -- M = 4*Co, row
 *        (dy*2+dx)*Co + co goes to out (B,Co,2H,2W)[co][2y+dy][2x+dx], L = H*Win.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x1; const float* x2; int C1; int C2; int in_mode;
    const float* ln_w; const float* ln_b; float ln_eps;
    const float* Wp; int64_t w_bstride;
    const float* bias; int64_t bias_bstride;
    const float* res;
    const float* prelu; int act;
    float* out; int out_mode; int Win;
    int B; int M; int K; int L;
} bem_pw_args;
/* natural (nsets, M, K) row-major -> packed f32-MFMA operand order (nsets, MT, KS, 64), MT = ceil(M/32), KS = ceil(K/2):
 * the weight format of the implicit-GEMM convolutions (BEM_CONV_MFMA of bem_conv2d_f32). */
int bem_pack_pw_weight_f32(const float* W, float* Wp, int nsets, int M, int K, void* stream);
int64_t bem_pw_packed_elems(int M, int K);

/* The same GEMM contract (bem_pw_args, identical semantics and error behaviour) with the products evaluated on the
 * bf16 matrix cores as an exact 3-limb expansion of both f32 operands (six limb products per term, f32 accumulate;
 * the dropped terms are <= 2^-23 of a product, i.e. f32-level error) -- 6/16 of the f32-MFMA cost.
 * Wp must come from bem_pack_pw_weight_x6: natural (nsets, M, K) f32 -> (nsets, MT, KB, 3 limbs, 64 lanes) 16-byte vectors
 * of 8 bf16, MT = ceil(M/32), KB = ceil(K/16); bem_pw_x6_packed_elems(M, K) = floats per set (w_bstride unit), 16-byte
 * aligned.  LayerNorm prologue for K <= 160. */
int bem_pw_gemm_x6_f32(const bem_pw_args* a, void* stream);
int bem_pack_pw_weight_x6(const float* W, float* Wp, int nsets, int M, int K, void* stream);
/* The same from a strided view (element strides over set, row, k): the transposed weight of an input-gradient GEMM (W^T = strides (., 1, K))
 * or a column block of a concatenated weight is packed where it lies, without a contiguous copy. */
int bem_pack_pw_weight_x6_strided(const float* W, float* Wp, int nsets, int M, int K, int64_t set_stride, int64_t row_stride,
                                  int64_t col_stride, void* stream);
/* Many matrices packed by one launch.  jobs: njobs x 8 64-bit words {source pointer; first float of the packed output in `arena` (multiple
 * of 4); int32 M, int32 K; row stride; column stride (elements); work items = ceil(M/32) * ceil(K/16) * 64; 0; 0}; blks: nblk x {int32 job,
 * int32 first block of 256 work items}.  Each output is what bem_pack_pw_weight_x6_strided writes for that view (one set). */
int bem_pack_pw_weight_x6_jobs(const void* jobs, const void* blks, int nblk, float* arena, void* stream);
int64_t bem_pw_x6_packed_elems(int M, int K);
/* bem_bnn_sample_f32 (below) and bem_pack_pw_weight_x6 in one pass for the weights of a Bayesian 1x1 layer: nsets weight
 * sets w = mu + log1p(exp(rho)) * eps written straight in x6 operand order; eps (nsets, M, K) injected or NULL = the
 * sampler's Philox draws for (seed, stream_id) -- identical values to sampling first and packing afterwards. */
int bem_bnn_sample_pack_x6(const float* mu, const float* rho, const float* eps, float* Wp, int nsets, int M, int K,
                           uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, int sigma_given,
                           void* stream);   /* sigma_given: rho already holds log1p(exp(rho)); stream_add: see bem_bnn_sample_f32 */
/* A Stage-II decoder level's fuse(cat(up(f), skip)) -- ConvTranspose2d(Cin, Cin/2, 2, stride 2) followed by a bias-free 1x1 conv over the
 * concatenation with the skip -- as ONE x6 GEMM; the up-sampled tensor is never formed:
 *   out[b][co][2i+a][2j+b'] = sum_k Wc[a,b'][co][k] f[b][k][i][j] + sum_c Wf2[co][c] skip[b][c][2i+a][2j+b'] + bias[co]
 * f (B, Cin, h, w), skip and out (B, Cin/2, 2h, 2w), 8-byte aligned; Cin even, >= 2.  Wc_packed = bem_pack_pw_weight_x6 of the four composed
 * phase matrices (4, Cin/2, Cin), set = 2a + b'; Wf2_packed = the same of (Cin/2, Cin/2); bias (Cin/2) the composed bias.  One weight set
 * for the whole batch. */
int bem_upfuse_x6_f32(const float* f, const float* skip, const float* Wc_packed, const float* Wf2_packed, const float* bias, float* out,
                      int B, int Cin, int h, int w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Convolutions.
 * ------------------------------------------------------------------------------------------- */
/* Depthwise 3x3, padding 1 (vmamba.py:507-515 conv2d, :124 gdMlp.dwconv, QD/model4.py:157-165).
 *   mode 0: out[c] = dw(x[c]) (+bias)            mode 1: SiLU(...)
 *   mode 2: gdMlp gate, x has 2*Cout channels: out[c] = GELU(dw(x[c])) * dw(x[c+Cout])
 *   mode 3: PostSmooth: out[c] = x[c] + ReLU(dw(x[c]) + bias)
 * w: (Cw,1,3,3), bias (Cw) or NULL, Cw = 2*Cout in mode 2 else Cout; *_bstride as above. */
int bem_dwconv3x3_f32(const float* x, const float* w, int64_t w_bstride, const float* bias,
                      int64_t bias_bstride, float* out, int B, int Cout, int H, int W, int mode, void* stream);

/* Dense convolution KHxKW, given stride / zero padding / dilation (nn.Conv2d semantics), optional bias, ReLU and up to two residual
 * tensors added after the activation:
 *   out = relu?(conv(x) + bias) + res1 + res2.      x (B,Cin,H,W) -> out (B,Cout,Ho,Wo)
 * x may be a channel slice of a wider tensor: x_bstride = elements between batch items.
 * res1_rep >= 1: output row b adds res1 row b / res1_rep, so res1 has B / res1_rep rows -- a term that is the same for the res1_rep
 * Monte-Carlo samples of an image is computed once per image.  1: one residual row per output row.
 * bem_conv2d_f32 runs the kernel form it is given, with w in that form's operand format, and rejects a form whose conditions the arguments miss. */
#define BEM_CONV_ROWS 1     /* coalesced rows on the bf16-limb (x6) matrix cores (conv_x6.hip), f32-level error (bem_pw_gemm_x6_f32); w as for TAPS */
#define BEM_CONV_TAPS 2     /* KH*KW shifted 1x1 taps on the same machinery; w = bem_pack_pw_weight_x6 of the (KH*KW, Cout, Cin) tap matrices, tap = ky*KW + kx */
#define BEM_CONV_MFMA 3     /* implicit GEMM on the f32 matrix cores; w = bem_pack_pw_weight_f32 of the (Cout, Cin*KH*KW) view of the weight */
#define BEM_CONV_DIRECT 4   /* VALU kernel staged through LDS; w = the plain (Cout,Cin,KH,KW) weight */
int bem_conv2d_f32(int form, const float* x, int64_t x_bstride, const float* w, const float* bias, const float* res1, const float* res2,
                   float* out, int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad, int dilation, int relu,
                   int res1_rep, void* stream);

/* Which form takes a convolution: BEM_CONV_*, or 0 with bem_last_error() saying why no kernel does.  Host arithmetic on the arguments alone:
 * no pointer is read (only whether it is NULL and its low four bits count), nothing is launched.  x is the pointer after the channel slice;
 * out NULL = an allocation of the caller's own (aligned).
 * allow: the forms that may be chosen where a rule says "x6 allowed" / "MFMA allowed" (tests and measurements reach the other kernels by
 * clearing a bit).  K = KH, Wo = output width; the first row that matches decides:
 *   0  KH != KW, (K, stride) none of (3,1) (3,2) (4,2) (5,1), or dilation not 1 / 2                                    -> refused
 *   1  dilation != 1, or K = 3 stride 2 (QD/model2.py:171-181, QD/model3.py:176): K = 3, pad = dilation, (stride, dilation) one of
 *      (1,1) (1,2) (2,1), Wo even, Cin % 8 == 0, x 8-byte aligned -> TAPS, else refused; the allow bits do not apply
 *   2  K = 3, s1, p1, x6 allowed, W even, Cin % 8 == 0, x 8-byte aligned: W a power of two in 4 .. 128, x / out / res1 / res2 16-byte
 *      aligned and x_bstride % 4 == 0 -> ROWS, else TAPS
 *   3  K = 5, s1, p2 (LPIPS conv2), x6 allowed, W even, Cin % 8 == 0, x 8-byte aligned                                 -> TAPS
 *   4  K = 4, s2, p1, no res1 / res2, Cin % 8 == 0, H and W even, Wo a power of two in 2 .. 64, x 16-byte aligned, x_bstride % 4 == 0 -> ROWS; no allow bit applies
 *   5  MFMA allowed, Cout <= 160, (K, stride) one of (3,1) (4,2), any pad                                              -> MFMA
 *   6  (K, stride) one of (3,1) (4,2), or (5,1) with Cin % 8 == 0                                                     -> DIRECT
 *   7  anything else                                                                                                   -> refused */
#define BEM_CONV_ALLOW_X6 1
#define BEM_CONV_ALLOW_MFMA 2
int bem_conv2d_route(const float* x, int64_t x_bstride, const float* res1, const float* res2, const float* out, int Cin, int H, int W,
                     int Cout, int KH, int KW, int stride, int pad, int dilation, int allow);

/* ---------------------------------------------------------------------------------------------
 * Quaternion / Haar primitives (basicsr/QD/model4.py:7-37,216-232; QD/quaternion.py:3-17).
 * ------------------------------------------------------------------------------------------- */
/* RGB (B,3,H,W; x_bstride elements between batch items) -> quaternion stack (8 ch) -> Haar DWT
 * -> out (B,32,H/2,W/2), channel = band*8 + q, bands LL,HL,LH,HH. */
int bem_quat_dwt_f32(const float* rgb, int64_t x_bstride, float* out, int B, int H, int W, void* stream);
/* bem_quat_dwt_f32 of bem_bilinear_up_f32(cond, s) in one pass, bit for bit, without the enlarged image in memory: the Stage-I conditions
 * cond (R,3,H,W) -> out (R,32,H*s/2,W*s/2); H*s and W*s even. */
int bem_cond_dwt_f32(const float* cond, float* out, int R, int H, int W, int s, void* stream);
int bem_dwt_f32(const float* x, float* out, int B, int C, int H, int W, void* stream);
int bem_iwt_f32(const float* x, float* out, int B, int C4, int H, int W, void* stream);
/* IWT of q1w, q2w (B,16,h,w) + Hamilton product, real part dropped -> out (B,3,2h,2w).
 * (DecompDualBranchDDWavelet_arch.py:361-367) */
int bem_iwt_hamilton_f32(const float* q1w, const float* q2w, float* out, int B, int h, int w, void* stream);
/* Hamilton product of q[:, 0:4] and q[:, 4:8] (B,8,H,W), real part dropped -> (B,3,H,W). */
int bem_hamilton_f32(const float* q, float* out, int B, int H, int W, void* stream);

/* hamilton_product(q1, q2) of QD/quaternion.py:3-17: q1, q2 (B,4,H,W) -> out (B,4,H,W) = [real, i, j, k]. */
int bem_hamilton_full_f32(const float* q1, const float* q2, float* out, int B, int H, int W, void* stream);

/* Channel cross-attention of the decomposition net (QD/model4.py:81-139) folded with the 1x1 `fuse`
 * conv that follows it.  Step 1: accumulate per image S = F1 F2^T (32x32), s1 = F1 1, s2 = F2 1 in f64
 * (stats: (B, 32*32 + 64) doubles, zeroed by the call).  Step 2: softmax + fold all 1x1 weights into
 * one per-image (32 x 64) matrix + bias: W_out (B, 32, 64) row-major, columns 0..31 for f1, 32..63 for f2 (bem_pw_gemm_x6_f32 in_mode 2
 * after bem_pack_pw_weight_x6). */
int bem_attn_stats_f64(const float* f1, const float* f2, double* stats, int B, int L, void* stream);
int bem_attn_fold_f32(const double* stats, const float* attn_w /* 8 x (32x32 + 32): q1,k2,v2,q2,k1,v1,out1,out2 */,
                      const float* fuse_w /* (32,64) */, const float* fuse_b /* (32) */,
                      float* W_out /* (B, 32, 64) */, float* bias_out /* (B,32) */, int B, int L,
                      void* stream);
/* Step 2 with the attention dropout of QD/model3.py:98,124-131 (nn.Dropout(0.1) on attn_1 and attn_2 after the softmax, live in train()
 * mode): every softmaxed entry is multiplied by keep / (1 - p) in f64 before the fold, which is linear in the maps.  keep comes from
 * `mask` (B, 2, 32, 32) of 0 / 1 values, map 0 = attn_1 and map 1 = attn_2, or, with mask NULL, from Philox4x32-10 under
 * (seed, stream_id): element e = ((b * 2 + map) * 1024 + i * 32 + j) is word e & 3 of counter block e >> 2 (the layout of the weight
 * sampler), u = (word >> 8) * 2^-24, kept iff u >= p in f32.  0 <= p < 1; p = 0 without a mask gives bem_attn_fold_f32's result bit
 * for bit. */
int bem_attn_fold_drop_f32(const double* stats, const float* attn_w, const float* fuse_w, const float* fuse_b,
                           const float* mask_or_null, float p, uint64_t seed, uint64_t stream_id,
                           float* W_out, float* bias_out, int B, int L, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Layout / resampling helpers.
 * ------------------------------------------------------------------------------------------- */
/* (P planes of H x W) -> (P planes of W x H); src/dst plane p at base + (p / ppb) * bstride + (p % ppb) * H*W. */
int bem_transpose_planes_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride,
                             int nbatch, int ppb, int H, int W, void* stream);
/* dst[b][dst_c0 + c][l] = src[b][c][l]  (c < C), strides in elements. */
int bem_copy_channels_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride,
                          int B, int C, int L, void* stream);
/* The same with dst row b reading src row b / rep (B = dst rows): decomp(image), evaluated once per image, handed to its rep
 * Monte-Carlo samples (the loop of eval.py:199-213 feeds the same image to every sample). */
int bem_copy_channels_rep_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride, int B, int C, int L, int rep,
                              void* stream);
/* dst[b][c][l] += src[b][c][l]  (c < C); DecompDualBranch2's "Q + [cond, 0]" (DecompDualBranch_arch.py:241-246). */
int bem_add_channels_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride,
                         int B, int C, int L, void* stream);
/* F.interpolate(scale_factor=s, mode='bilinear', align_corners=False) (eval.py:220, UNet_arch.py:130). */
int bem_bilinear_up_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride,
                        int B, int C, int H, int W, int s, void* stream);
/* PatchMerging gather (UNet_arch.py:74-78): (B,C,H,W) -> (B,4C,H/2,W/2), blocks [ee, oe, eo, oo]. */
int bem_space_to_depth_f32(const float* x, float* out, int B, int C, int H, int W, void* stream);
/* nn.PixelShuffle(2): (B,4C,H,W) -> (B,C,2H,2W). */
int bem_pixel_shuffle2_f32(const float* x, float* out, int B, int C, int H, int W, void* stream);

/* Every Bayesian tensor of a net drawn for a stochastic forward in one launch (the N weight sets per leaf of eval.py:199-211, all leaves).
 * segs: nseg x 8 64-bit words {mu, sig pointers (sig = precomputed sigma for packed tensors, rho for natural ones); first float of the
 * tensor's output in `arena` (multiple of 4); n = elements per set; int32 M, int32 K (K > 0: the nsets sets in x6 operand order exactly as
 * bem_bnn_sample_pack_x6 with sigma_given writes them; K = 0: natural order as bem_bnn_sample_f32); stream counter; work items (packed:
 * nsets * ceil(M/32) * ceil(K/16) * 64, natural: ceil(nsets * n / 4)); nsets * n}; blks: nblk x {int32 segment, int32 first block of 256
 * work items}.  Draws: (seed, stream_base + counter), element numbering of the per-tensor entry points. */
int bem_bnn_ebank_sample_f32(const void* segs, const void* blks, int nblk, float* arena, uint64_t seed, uint64_t stream_base, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DecompDualBranch's bottleneck blocks (basicsr/archs/DecompModel_arch.py:57-99).
 * ------------------------------------------------------------------------------------------- */
/* out[m][k] = w[m][k] * scale[m]: folds CrossFusionBlock's per-channel gate (:57-66, x_tgt + gate * (W x_src + b)) into W (M,K) and,
 * with K = 1, into b; the block then runs as bem_pw_gemm_x6_f32 with x_tgt as the residual. */
int bem_row_scale_f32(const float* w, const float* scale, float* out, int M, int K, void* stream);
/* SEBlock's gate (:68-83): y (B,C) = sigmoid(w2 relu(w1 mean)), mean (B,C) from bem_plane_mean_f32, w1 (Cr,C), w2 (C,Cr), no biases. */
int bem_se_gate_f32(const float* mean, const float* w1, const float* w2, float* y, int B, int C, int Cr, void* stream);
/* SpatialAttention (:85-99) of x * chan_scale (chan_scale (B,C) = the SE gate that precedes it, :318-324, or NULL):
 * out = x * chan_scale * sigmoid(conv_kxk([mean_c, max_c](x * chan_scale))), w (1,2,k,k), k = 3 or 7, zero padding k/2, no bias;
 * map_ws: (B,2,H,W) floats of workspace; x, out (B,C,H,W). */
int bem_spatial_attention_f32(const float* x, const float* chan_scale, const float* w, float* map_ws, float* out, int B, int C, int H, int W,
                              int k, void* stream);

/* Training side of the same blocks (autograd nodes of bem/autograd.py: CrossFusion = PwFn + GateAddFn, SEBlockFn, SpatialAttnFn).
 * chan_scale: out = scale[b * scale_bstride + c] * x (+ add) (+ add_bc[b][c] * add_bc_scale); scale_bstride = C (per-image factors) or 0
 * (a parameter).  chan_dot: per_batch ? out (B,C) = sum_p a b : out (C) += sum_{b,p} a b.  se_gate_bwd: backward of bem_se_gate_f32 through
 * sigmoid / W2 / relu / W1 (dw1, dw2 accumulated, dmean (B,C) written).  spatial_attention_bwd: backward of bem_spatial_attention_f32 with
 * chan_scale = NULL; map = the (B,2,H,W) workspace its forward filled, dpre_ws (B,H,W) floats, dw (1,2,k,k) accumulated. */
int bem_chan_scale_f32(const float* x, const float* scale, int64_t scale_bstride, const float* add, const float* add_bc, float add_bc_scale,
                       float* out, int B, int C, int64_t HW, void* stream);
int bem_chan_dot_f32(const float* a, const float* b, float* out, int B, int C, int64_t HW, int per_batch, void* stream);
int bem_se_gate_bwd_f32(const float* mean, const float* w1, const float* w2, const float* y, const float* dy, float* dmean, float* dw1,
                        float* dw2, int B, int C, int Cr, void* stream);
int bem_spatial_attention_bwd_f32(const float* x, const float* dout, const float* map, const float* w, float* dpre_ws, float* dx, float* dw,
                                  int B, int C, int H, int W, int k, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bayesian sampling + Monte-Carlo loop pieces (basicsr/bayesian/conv.py:106-114, eval.py:199-264).
 * ------------------------------------------------------------------------------------------- */
/* out[s][i] = mu[i] + log1p(exp(rho[i])) * eps, eps = eps_in[s][i] when eps_in != NULL else a
 * Philox4x32-10 N(0,1) draw keyed by (seed, stream_id, s*n + i).  stream_add (NULL or one uint64 in device memory) is added to
 * stream_id by the kernel: the per-iteration part of the id stays in HBM, so a captured HIP graph of a training step (the
 * replacement of torch's generator advancing between iterations, condition_generator_model.py:176-218) draws new numbers on
 * each replay. */
int bem_bnn_sample_f32(const float* mu, const float* rho, const float* eps_in, float* out,
                       int nsets, int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, void* stream);
/* Image preparation of eval.py:146-176: reflect-pad bottom/right of P planes (H,W) -> (Hp,Wp) (numpy 'reflect'), and the
 * x1/s INTER_LINEAR condition image of the padded planes (even s dividing Hp, Wp): mean of the 2x2 centre taps. */
int bem_pad_reflect_f32(const float* x, float* out, int P, int H, int W, int Hp, int Wp, void* stream);
int bem_resize_down_f32(const float* x, float* out, int P, int Hp, int Wp, int s, void* stream);
/* N(0,1) draws from the same Philox4x32-10 stream family as bem_bnn_sample_f32 (torch.randn_like of eval.py:209). */
int bem_randn_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, void* stream);
/* Stage-I post-processing (eval.py:200-209): c = clamp(pred,0,1); if target_mean: c = clamp(c *
 * target_mean[b_img][ch] / mean_hw(c), 0, 1); c += noise * noise_level.  pred/out (Bn,3,h,w);
 * target_mean (n_img,3) with image index = b / samples_per_image; noise may be NULL. */
int bem_cond_postproc_f32(const float* pred, const float* target_mean, const float* noise, float* out,
                          int Bn, int h, int w, int samples_per_image, float noise_level, void* stream);
/* Per-plane mean over the top-left (h,w) window of (P, Hs, Ws) planes -> means (P) (f32 out, f64 accumulate). */
int bem_plane_mean_f32(const float* x, float* means, int P, int Hs, int Ws, int h, int w, void* stream);
/* Candidate finalisation (eval.py:222-226,246-252, Enhancement/utils.py:5-9): crop to (h,w), clamp to
 * [0,1], optional per-channel GT-mean rescale + clip, write final (Bn,3,h,w) and PSNR (Bn) vs target
 * (n_img,3,h,w).  pred is (Bn,3,Hp,Wp). */
int bem_candidate_finalize_f32(const float* pred, const float* target, float* final_out, float* psnr, double* ws,
                               int Bn, int samples_per_image, int Hp, int Wp, int h, int w, int gt_mean,
                               void* stream);   /* ws: scratch of 7*Bn doubles (zeroed by the call) */

/* calculate_ssim(img_as_ubyte(target), img_as_ubyte(pred)) of Enhancement/utils.py:12-57 per candidate: uint8 values rint(255 x), f64,
 * 11x11 Gaussian (sigma 1.5) over the valid region, mean over region and channels.  pred (Bn,3,h,w), target (Bn/spi,3,h,w), h, w > 10;
 * ssim (Bn) f32 out; ws: scratch of Bn doubles (zeroed by the call). */
int bem_ssim_f32(const float* pred, const float* target, float* ssim, double* ws, int Bn, int samples_per_image, int h, int w, void* stream);

/* Selection rules of eval.py:268-297 on the device, FIRST index on ties (python list.index), f64 comparisons:
 *   rule 0: max of weight * s1 / max(s1) + (1 - weight) * s2 / max(s2)  (PSNR / SSIM, UIQM / UCIQE; s2 NULL = weight 1); passes NaN over
 *   rule 1: max of s1 (no-reference, CLIP-IQA)      rule 2: min of s1 (NIQE)
 *   rule 3: max of s1 / max(s1), s2 NULL (eval.py:284-285 with psnr_weight = 1, the eval step's default); keeps a leading NaN like python
 * NaN, zero and negative maxima: the comment above first_better in csrc/selection.hip.
 * best (B) int32; best_s1 / best_s2 (B) or NULL; best_img[b] = cand[b*N + best[b]] (chw floats each) when cand / best_img are given.
 * Everything stays on the device: no host round trip per step. */
int bem_select_scores_f32(const float* cand, const float* s1, const float* s2, float weight, int rule, int* best, float* best_s1,
                          float* best_s2, float* best_img, int B, int N, int64_t chw, void* stream);

/* NIQE of Enhancement/eval.py:248-254 (calculate_niqe(pred * 255, crop_border=0), basicsr/metrics/niqe.py) per candidate, the
 * no-reference score that eval.py:272-274 minimises.  final (Bn,3,h,w) f32 in [0,1], RGB as BEMPipeline.candidates returns it; h, w >= 96
 * (the reference silently yields NaN below one 96 x 96 block).  Steps, with the reference's dtypes:
 *   Y of metric_util.py:32-45 / color_util.py:38-70 on the stored order (its BGR weights: 24.966 multiplies R), rounded half to even,
 *   cropped to floor(h/96)*96 x floor(w/96)*96 (top-left); MSCN with the 7x7 `window` (scipy.ndimage.convolve, 'nearest', f64 sums,
 *   f32 result); per 96 x 96 block the AGGD fits of compute_feature (niqe.py:13-62); imresize(img/255, 0.5, antialiasing=True) * 255
 *   (matlab_functions.py:16-175, two passes); MSCN and 48 x 48 block fits again; mu_d = nanmean, cov_d = np.cov over NaN-free rows;
 *   score = sqrt(d^T ((cov_pris + cov_d)/2)^-1 d), d = mu_pris - mu_d (niqe.py:65-143), by a Cholesky solve in f64.
 * mu_pris (36), cov_pris (36x36), window (7x7): niqe_pris_params.npz, f64 on the device.  gam_tab (4 x ntab f64): gam = arange(0.2,
 * 10.001, 0.001), r_gam = G(2/a)^2 / (G(1/a) G(3/a)), sqrt(G(1/a) / G(3/a)), G(2/a) / G(1/a).  rs_wh / rs_ih (h'/2 x kh): resize weights
 * and symmetric-padded source rows of the H pass, rs_ww / rs_iw (w'/2 x kw) of the W pass (h', w' = cropped size).  scores (Bn) f64 out;
 * a candidate with fewer than 2 NaN-free block rows scores NaN (the reference raises there).  ws: bem_niqe_ws_bytes(Bn, h, w) bytes. */
int bem_niqe_f32(const float* final, const double* mu_pris, const double* cov_pris, const double* window, const double* gam_tab, int ntab,
                 const float* rs_wh, const int* rs_ih, int kh, const float* rs_ww, const int* rs_iw, int kw, double* scores, void* ws,
                 int64_t ws_bytes, int Bn, int h, int w, void* stream);
int64_t bem_niqe_ws_bytes(int Bn, int h, int w);   /* 0 for h or w < 96 */

/* UIQM and UCIQE of Enhancement/eval.py:255-260 (getUIQM / getUCIQE of basicsr/metrics/uciqe_uiqm.py) per candidate, the no-reference scores
 * that eval.py:276-280 weighs.  final (Bn,3,h,w) f32 in [0,1], RGB as BEMPipeline.candidates returns it.  u8 = img_as_ubyte(final) (rint(255 x),
 * half to even).  UIQM on Image.fromarray(u8).resize((256, Hr)), Hr = int(256 / w * h) >= 10: Pillow's 8-bit BICUBIC, horizontal pass first,
 * uint8 between the passes; rs_bh (256 x 2: first source column, tap count) and rs_kh (256 x kh) are the fixed-point (22-bit) coefficients
 * of the w -> 256 pass, rs_bv / rs_kv (Hr x 2, Hr x kv) of the h -> Hr pass.  UICM (alpha-trimmed means from 511- and 1021-bin histograms,
 * the trimmed sum in f32 in sorted order), UISM (Sobel, mode reflect; EME over 10 x 10 blocks whose last row / column absorbs the remainder,
 * f32 terms summed in f32; weights 0.299, 0.587, 0.144), UIConM (10 x 10 x 3 blocks of the cropped image, f64); the UIQM total is rounded
 * as NumPy 2 does (f32 from the c2 * uism term on).  UCIQE on u8 after OpenCV's 8-bit RGB2Lab_b: lab_tab = sRGB gamma x 2040 (256 ints),
 * 2^15 f(i / 2040) (3072), the 3 x 3 matrix cvRound(4096 sRGB2XYZ_D65 / D65white) (9).  A plane without Sobel edges makes UISM and UIQM
 * NaN.  uiqm, uciqe (Bn) f64 out.  ws: bem_uiqm_ws_bytes(Bn, h, w, Hr) bytes; it starts with parts (Bn x 8 f64: uicm, uism, uiconm, uiqm,
 * var_chr, con_lum, aver_sat, uciqe), then the resized image (Bn,3,Hr,256) u8 and the Lab image (Bn,3,h,w) u8, each region aligned to
 * 256 bytes. */
int bem_uiqm_uciqe_f32(const float* final, const int* lab_tab, const int* rs_bh, const int* rs_kh, int kh, const int* rs_bv, const int* rs_kv,
                       int kv, double* uiqm, double* uciqe, void* ws, int64_t ws_bytes, int Bn, int h, int w, int Hr, void* stream);
int64_t bem_uiqm_ws_bytes(int Bn, int h, int w, int Hr);   /* 0 for Hr < 10 */

/* Monte-Carlo mean of eval.py:224-225,308-314: out (B,3,h,w) = clamp(mean_n clamp(pred[b*N+n][:, :h, :w], 0, 1), 0, 1), with gt_mean scaled
 * by mean(gray(target)) / mean(gray(out)) (cv2 BGR2GRAY weights on the stored channel order) and clipped.  pred (B*N,3,Hp,Wp);
 * ws: 2 B doubles (zeroed by the call) when gt_mean. */
int bem_mc_mean_f32(const float* pred, const float* target, float* out, double* ws, int B, int N, int Hp, int Wp, int h, int w,
                    int gt_mean, void* stream);

/* The same mean, and the per-pixel spread of the N predictions, streamed over chunks of the N samples (a chunk = Nc samples of every
 * image; the chunks of a run are handed over in sample order).  State planes (B,3,h,w) f32, zero before the first chunk:
 *   sum       += clamp(raw[b*Nc+n][:, :h, :w], 0, 1), n = 0 .. Nc-1 one at a time: the additions bem_mc_mean_f32 performs, in its order
 *   mean, m2  Welford's update with fin[b*Nc+n] as sample number n_done + n + 1 (d = x - mean; mean += d / k; m2 += d * (x - mean)),
 *             every operation rounded to f32 on its own (no contraction)
 * raw (B*Nc,3,Hp,Wp) with sum, and / or fin (B*Nc,3,h,w) with mean and m2; either pair may be NULL.  An element's state depends on the
 * sequence of its samples alone, so any split of N into chunks leaves the same bits. */
int bem_mc_accum_f32(const float* raw, const float* fin, float* sum, float* mean, float* m2, int B, int Nc, int n_done, int Hp, int Wp,
                     int h, int w, void* stream);

/* What the state planes hold after N samples.  sum with mc: mc (B,3,h,w) = clamp(sum / N, 0, 1) and the GT-mean rescale, bit for bit
 * bem_mc_mean_f32 of the same N raw outputs (target when gt_mean).  m2 with std: std (B,3,h,w) = sqrt(m2 / (N - 1)), zeros for N = 1, and
 * std_mean (B) f64 = its mean over the 3 h w elements of an image (per-workgroup f64 partials summed in a fixed order by a second launch:
 * the same bits on every run).  Either pair may be NULL.  ws: 258 B doubles. */
int bem_mc_finish_f32(const float* sum, const float* m2, const float* target, float* mc, float* std, double* std_mean, double* ws, int B,
                      int N, int h, int w, int gt_mean, void* stream);

/* bem_select_scores_f32's rules 1 (max) and 2 (min) over chunks of an image's samples handed over in sample order: best (B) int32,
 * best_score (B) and best_img (B, chw) are the running choice over the n_done samples seen so far (not read when n_done = 0).  They
 * change only where the chunk (scores (B*Nc), cand (B*Nc, chw)) holds a strictly better score, compared in f64 -- the first index wins
 * ties, as in one bem_select_scores_f32 call over all the samples: it is that call's kernel and loop, started from the running score.
 * cand / best_img may both be NULL; pick: B int32 of scratch. */
int bem_select_merge_f32(const float* cand, const float* scores, int rule, int* best, float* best_score, float* best_img, int* pick, int B,
                         int Nc, int n_done, int64_t chw, void* stream);

/* The whole gdMlp branch of a VSSBlock in one kernel (vmamba.py:116-133 gdMlp.forward + the block's norm2 / residual :1330-1333):
 *   out (B,C,H,W) = x + W_o (GELU(h[0:Hd]) * h[Hd:2Hd]) + b_o,   h = dw3x3(W_i LayerNorm2d(x) + b_i) + b_dw.
 * Neither the 2Hd-channel project_in output nor the Hd-channel gate tensor reaches HBM (4 x 32 pixel tiles, both live as 16-gate-channel
 * slices in LDS).  x (B,C,H,W) with C <= 80, out != x; ln_w / ln_b (C).
 * Wp_gate = bem_pack_pw_weight_x6 of the (2Hd, C) project_in matrix in gate-interleaved row order: packed row 32 j + 2 c + s =
 * W_i[s Hd + 16 j + c] (c < 16, s < 2; Hd % 16 == 0); bias_gate (Hd/16, 16, 2) = b_i in the same order (zeros for a layer without bias);
 * dw_gate10 (Hd,10,2): [c][tap < 9] = (dww[c][tap], dww[Hd + c][tap]), [c][9] = (dwb[c], dwb[Hd + c]) (zeros for a layer without bias);
 * Wp_out = bem_pack_pw_weight_x6 of the (C, Hd) project_out matrix; bias_out (C) | NULL.  Packed weights, bias_gate and dw_gate10 16-byte
 * aligned: the kernel moves them chunk by chunk into LDS with LDS-DMA (global_load_lds_dwordx4). */
int bem_gdmlp_x6_f32(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const float* Wp_gate,
                     const float* bias_gate, const float* dw_gate10, const float* Wp_out,
                     const float* bias_out, float* out, int B, int C, int Hd, int H, int W, void* stream);

/* The back half of a VSSBlock in one kernel: the SS2D tail (vmamba.py:700-716 after the scan) and the gdMlp branch above,
 *   x1 = x + W_op LayerNorm2d(y0 + y1) + b_op,   out = x1 + W_o (GELU(h[0:Hd]) * h[Hd:2Hd]) + b_o,   h = dw3x3(W_i LayerNorm2d(x1) + b_i) + b_dw.
 * x1 is never a tensor: every tile forms it on its halo as well, and parks its own pixels in out for the residual.  The first sixteen
 * arguments are those of bem_gdmlp_x6_f32, x now the SS2D branch's input; y0 / y1 (B,C,H,W) the two scan outputs (d_inner == C), on_w / on_b (C)
 * and on_eps the out_norm parameters, bias_outproj (C) | NULL.  C <= 48, C % 8 == 0, C H W < 2^30; out differs from x, y0 and y1.
 * Wp_outproj = bem_pack_pw_weight_x6 of a (32 MT, C) matrix, MT = ceil(ceil(C / 16) / 2), whose row 32 mt + (r & 3) + 8 (r >> 2) + 4 kh
 * (r < 16, kh < 2) is W_op[16 (s >> 3) + 8 kh + (s & 7)] with s = 16 mt + r, and zero where s >= 8 ceil(C / 16) or that channel is >= C
 * (bem.ops.vss_back_rows): the accumulator register of a lane then holds the channel the lane needs as the next GEMM's operand.  16-byte aligned. */
int bem_vss_back_x6_f32(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const float* Wp_gate,
                        const float* bias_gate, const float* dw_gate10, const float* Wp_out,
                        const float* bias_out, float* out, int B, int C, int Hd, int H, int W,
                        const float* y0, const float* y1, const float* on_w, const float* on_b, float on_eps,
                        const float* Wp_outproj, const float* bias_outproj, void* stream);

/* SS2D front half in one kernel (vmamba.py:700-716 up to the scan, with the block's norm :1326):
 *   xc (B,C,H,W) = SiLU(dw3x3(W_in LayerNorm2d(x) + b_in) + b_dw),   xd (B,Mx,H*W) = W_x xc  (Mx = 4 (R + 2): the x_dbl rows of all four directions).
 * The in_proj output exists only as a 4 x 32 pixel tile (+ halo) in LDS.  x (B,C,H,W) with C <= 48, C % 8 == 0, xc != x; ln_w / ln_b (C);
 * Wp_in = bem_pack_pw_weight_x6 of the (C, C) in_proj matrix, bias_in (C) | NULL; dww (C,9), dwb (C) | NULL: depthwise 3x3;
 * Wp_x = bem_pack_pw_weight_x6 of the (Mx, C) x_proj rows, Mx <= 32. */
int bem_ss2d_front_x6_f32(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const float* Wp_in, const float* bias_in,
                          const float* dww, const float* dwb, const float* Wp_x, float* xc, float* xd, int B, int C, int Mx, int H, int W,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training step: backward of the Stage-II forward + optimizer, i.e. what
 * `l_total.backward()`, clip_grad_norm_ and AdamW.step do in basicsr/models/image_enhancer_model.py:165-216.
 * Gradient buffers of parameters (dw, dbias, dgamma, ...) are ACCUMULATED INTO (+=, float atomics) unless noted:
 * the caller zeroes them once per step (optimizer.zero_grad()).
 * ------------------------------------------------------------------------------------------- */

/* L1Loss(loss_weight, reduction='mean') (basicsr/losses/losses.py:28): loss[0] (or NULL) = weight * mean |pred - gt|;
 * dpred (or NULL) = gmul[0] * weight * sign(pred - gt) / n, gmul = device scalar dL/dloss (NULL = 1).
 * ws: one double of scratch (zeroed by the call). */
int bem_l1_loss_f32(const float* pred, const float* gt, float* dpred, float* loss, double* ws, int64_t n, float weight,
                    const float* gmul, void* stream);

/* SSIM loss (basicsr/losses/my_loss.py:37-38: 1 - pytorch_msssim.ssim(y_true, y_pred, data_range=1.0, size_average=True)) on f32
 * tensors in [0,1], no quantisation (csrc/ssim_loss.hip states the formulas).  pred, gt (planes,H,W), planes = B*C handled independently,
 * H, W >= 11, H*W < 2^31, planes <= 32768 * 65535: loss[0] = weight * (1 - mean of the SSIM map over all planes * (H-10) * (W-10) valid
 * positions), bit-reproducible from call to call (per-workgroup f64 partials in ws, added in a fixed order by a second launch; no atomics).
 * coef (or NULL): the three coefficient maps a | b | c of the backward, 3 x (planes,H-10,W-10), written by the same launch.
 * ws: bem_ssim_loss_ws_elems(planes, H, W) doubles of scratch (every one written by the call).  bem_ssim_loss_tile: the edge of the
 * square tile of valid positions (forward) / pixels (backward) one workgroup takes. */
int bem_ssim_loss_tile(void);
int64_t bem_ssim_loss_ws_elems(int64_t planes, int H, int W);
int bem_ssim_loss_f32(const float* pred, const float* gt, float* loss, float* coef, double* ws, int64_t planes, int H, int W,
                      float weight, void* stream);
/* Backward of bem_ssim_loss_f32 (basicsr/losses/my_loss.py:37-38 under autograd; pred alone takes a gradient):
 * dpred (planes,H,W) = gmul[0] * -(weight / Npos) * (G^T a + 2 pred G^T b + gt G^T c), G^T the full 11x11 correlation of a valid-region
 * map back to H x W, coef = a | b | c as the forward wrote them, gmul = device scalar dL/dloss (NULL = 1). */
int bem_ssim_loss_bwd_f32(const float* pred, const float* gt, const float* coef, float* dpred, int64_t planes, int H, int W,
                          float weight, const float* gmul, void* stream);

/* MSELoss(reduction='mean') under a weight (F.mse_loss: basicsr/losses/my_loss.py:19, the criterion 'l2' of basic_loss.py:191-192), the
 * contract of bem_l1_loss_f32: loss[0] (or NULL) = weight * mean (pred - gt)^2; dpred (or NULL) = gmul[0] * weight * 2 (pred - gt) / n.
 * ws: one double of scratch (zeroed by the call). */
int bem_mse_loss_f32(const float* pred, const float* gt, float* dpred, float* loss, double* ws, int64_t n, float weight,
                     const float* gmul, void* stream);

/* CharbonnierLoss(reduction='mean') under a weight (basicsr/losses/basic_loss.py:23-25, 96-115), the contract of bem_l1_loss_f32 with
 * c = sqrt((pred - gt)^2 + eps) evaluated in f32 one operation at a time (eps >= 0 is not folded away: 1e-12 decides c below
 * |pred - gt| ~ 1e-6): loss[0] (or NULL) = weight * mean c; dpred (or NULL) = gmul[0] * weight * (pred - gt) / c / n, exactly 0 where
 * pred == gt (eps > 0).  Bit-reproducible from call to call: one f64 partial per workgroup in ws, added in a fixed order by a second
 * launch; no atomics.  16-byte vector accesses when pred, gt and dpred are all 16-byte aligned (the last n % 4 elements one by one),
 * single floats otherwise.  ws: bem_charbonnier_loss_ws_elems(n) doubles of scratch (every one written by the call). */
int64_t bem_charbonnier_loss_ws_elems(int64_t n);
int bem_charbonnier_loss_f32(const float* pred, const float* gt, float* dpred, float* loss, double* ws, int64_t n, float weight,
                             float eps, const float* gmul, void* stream);

/* The per-pixel statistics of CombinedLoss (basicsr/losses/my_loss.py:51-74) in one pass over pred and gt, contiguous (B, n1) f32 with
 * n1 = C*H*W elements per sample, d = pred - gt, n = B * n1 < 2^32 (the histogram counters are 32 bits wide; refused above):
 *   out[1] smooth_l1 = mean(|d| < 1 ? d^2 / 2 : |d| - 1/2)                         (my_loss.py:30-31)
 *   out[2] mse = mean d^2,   out[3] psnr = 40 - 20 log10(1 / sqrt(mse))            (my_loss.py:25-28; -inf for mse == 0)
 *   out[4] color = mean_b |mean gt_b - mean pred_b|                                (my_loss.py:22-23)
 *   out[5] hist = mean_k |h_gt[k] / sum h_gt - h_pred[k] / sum h_pred|, h = torch.histc(x, 256, 0, 1): bin floor(256 x), 1.0 in bin 255,
 *          x < 0, x > 1 and NaN not counted; NaN when pred or gt has no value in [0,1]   (my_loss.py:40-49)
 *   out[0] loss = a1 smooth_l1 + a3 hist + a5 psnr + a6 color, alphas >= 0, a term with a zero alpha left out   (my_loss.py:70-72)
 * Bit-reproducible from call to call: f64 partials per workgroup (no workgroup crosses a sample) added in a fixed order by a second
 * launch, integer histogram counts.  rec (or NULL): the backward's record, 2 + B doubles c1 | c2 | cc_b.  ws: bem_pixstat_loss_ws_bytes
 * bytes of scratch, 16-byte aligned; its first 512 uint32 hold the counts of pred | gt after the call.  bem_pixstat_loss_chunk: the
 * elements one workgroup takes of a sample larger than a quarter of it (smaller samples go to workgroups whole, a wave each). */
int bem_pixstat_loss_chunk(void);
int64_t bem_pixstat_loss_ws_bytes(int64_t B, int64_t n1);
int bem_pixstat_loss_f32(const float* pred, const float* gt, float* out, double* rec, void* ws, int64_t B, int64_t n1, double a1,
                         double a3, double a5, double a6, void* stream);
/* Backward of bem_pixstat_loss_f32 (my_loss.py:62-74 under autograd; pred alone takes a gradient, the histogram term has none):
 * dpred = gmul[0] * (c1 clamp(d, -1, 1) + c2 d + cc_b),  c1 = a1 / n,  c2 = a5 * 20 / (ln 10 * n * mse) (0 where mse == 0: torch gives
 * NaN there),  cc_b = -a6 sign(mean gt_b - mean pred_b) / n with sign(0) = 0; rec as the forward wrote it, gmul = device scalar
 * dL/dloss (NULL = 1). */
int bem_pixstat_loss_bwd_f32(const float* pred, const float* gt, const double* rec, float* dpred, int64_t B, int64_t n1,
                             const float* gmul, void* stream);

/* Backward of bem_iwt_hamilton_f32: dout (B,3,2h,2w) -> dq1w, dq2w (B,16,h,w) (written). */
int bem_iwt_hamilton_bwd_f32(const float* q1w, const float* q2w, const float* dout, float* dq1w, float* dq2w, int B, int h, int w,
                             void* stream);
/* Backward of bem_hamilton_f32 (the full-resolution archs: hamilton_product(out_1, out_2)[:, 1:], DecompModel_arch.py:351-352):
 * q8 (B,8,H,W) = [p | q], dout (B,3,H,W) -> dq8 (B,8,H,W) = [dp | dq]. */
int bem_hamilton_bwd_f32(const float* q8, const float* dout, float* dq8, int B, int H, int W, void* stream);

/* nn.PixelUnshuffle(2): x (B,C,2H,2W) -> out (B,4C,H,W), out[c*4 + i*2 + j][y][x] = x[c][2y+i][2x+j] (H, W = OUTPUT plane size).
 * Rearranges dL/dout of ConvTranspose2d(k=2,s=2) so that its input / weight gradients are 1x1 GEMMs, and is the inverse of
 * bem_pixel_shuffle2_f32 (used for the input gradient of the 4x4 stride-2 convolution). */
int bem_pixel_unshuffle2_f32(const float* x, float* out, int B, int C, int H, int W, void* stream);

/* out[c] += sum over batch and pixels of x (B,C,L)  (bias gradients). */
int bem_channel_sum_f32(const float* x, float* out, int B, int C, int64_t L, void* stream);
/* out = a + alpha * b (n elements): gradient accumulation where a tensor feeds two consumers (encoder skips, shared
 * bottleneck), and conds = gt_down + noise_level * randn of the training step (image_enhancer_model.py:143-148). */
int bem_add_f32(const float* a, const float* b, float* out, int64_t n, float alpha, void* stream);

/* LayerNorm2d backward (vmamba.py:58-63): x = x1 (+ x2 when non-NULL), all (B,C,L); dn = dL/dLN(x).
 *   dx = (dres or 0) + LN'(dn)   written;   n_out (or NULL) = LN(x) written (the operand of the consumer's weight gradient);
 *   dgamma, dbeta (C) accumulated. */
int bem_ln_bwd_f32(const float* x1, const float* x2, const float* dn, const float* gamma, const float* beta, float eps,
                   const float* dres, float* dx, float* n_out, float* dgamma, float* dbeta, int B, int C, int64_t L, void* stream);
int bem_ln_fwd_f32(const float* x1, const float* x2, const float* gamma, const float* beta, float eps, float* n_out, int B, int C,
                   int64_t L, void* stream);

/* Backward of bem_dwconv3x3_f32 through the activation (modes 0 plain, 1 SiLU, 2 gdMlp gate), shared weights:
 *   t (B,Cw,H,W) the conv input, dout (B,Cout,H,W); dpre (B,Cw,H,W) = dL/d(conv output + bias) written;
 *   dw (Cw,9), dbias (Cw)|NULL accumulated.  The input gradient is bem_dwconv3x3_f32(dpre, flipped w, mode 0). */
int bem_dwact_bwd_f32(const float* t, const float* w, const float* bias, const float* dout, float* dpre, float* dw, float* dbias,
                      int B, int Cout, int H, int W, int mode, void* stream);

/* Weight gradient of a 1x1 layer: dw[m][k] += sum_{b,p} dy[b][m][p] * x[b][k][p], x = x1 rows [0,C1) then x2 rows [C1,C1+C2)
 * (the concat input mode of bem_pw_args; C2 = 0 / x2 = NULL otherwise); dbias[m] += sum dy[b][m][p] when non-NULL.
 * *_bstride: elements between batch items (0 = contiguous).  dw row m is stored at row perm[m / blk_rows] * blk_rows + m % blk_rows
 * with row stride ldw (blk_rows = 0: identity) -- lets the stacked x_proj GEMM of the fused SS2D write its per-direction blocks. */
typedef struct {
    const float* dy; int64_t dy_bstride; int M;
    const float* x1; int64_t x1_bstride; int C1;
    const float* x2; int64_t x2_bstride; int C2;
    float* dw; int64_t ldw; int blk_rows; int perm[4];
    float* dbias;
    int B; int L;
} bem_wgrad_args;
int bem_pw_wgrad_f32(const bem_wgrad_args* a, void* stream);
/* The same contract for L % 32 == 0 on the bf16 matrix cores: both operands are loaded in MFMA operand order straight from their
 * channel planes (consecutive pixels per lane), split into three bf16 limbs and multiplied as six exact limb products with f32
 * accumulation (the arithmetic of bem_pw_gemm_x6_f32) -- no LDS transposes.  ws: scratch of at least
 * bem_pw_wgrad_x6_ws_elems(M, C1 + C2, B, L) floats (per-workgroup partial tiles, summed by a second kernel: no float atomics). */
int64_t bem_pw_wgrad_x6_ws_elems(int M, int K, int B, int L);
int bem_pw_wgrad_x6_f32(const bem_wgrad_args* a, float* ws, int64_t ws_elems, void* stream);
/* Weight (+ bias) gradient of the dense convolution of bem_conv2d_f32: dw (Cout,Cin,KH,KW) += dy (*) x, rows gathered on the
 * fly (no im2col tensor); dy (B,Cout,Ho,Wo) contiguous, x (B,Cin,H,W) with batch stride x_bstride (0 = contiguous). */
int bem_conv_wgrad_f32(const float* dy, const float* x, int64_t x_bstride, float* dw, float* dbias, int B, int Cin, int H, int W,
                       int Cout, int KH, int KW, int stride, int pad, void* stream);

/* Backward of bem_ss2d_scan_strided_f32 (same operand layout).  dy0 / dy1 = dL/dy0, dL/dy1; dx0 / dx1 written;
 * dxd0 / dxd1 (B,2,R+2,L) contiguous: zeroed by the call, then accumulated over channels; dAlog (4C) = gradient of A_logs,
 * dDs (4C), ddtw (4,C,R), ddtb (4,C) accumulated. */
int bem_ss2d_scan_bwd_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dy0, const float* dy1,
                          const float* dtw, const float* dtb, const float* A, const float* Ds, float* dx0, float* dx1, float* dxd0,
                          float* dxd1, float* dAlog, float* dDs, float* ddtw, float* ddtb, int B, int C, int L, int R,
                          int64_t xd0_bstride, int64_t xd1_bstride, void* stream);
/* Backward of bem_ss2d_scan_n_f32 (what autograd runs through forward_corev2 with d_state N, vmamba.py:657-684; SelectiveScanCuda.backward
 * csms6s.py:95-113).  Outputs as bem_ss2d_scan_bwd_f32 with dxd0 / dxd1 (B,2,R+2N,L) contiguous, zeroed by the call, and dAlog (4C, N).
 * ws: scratch of at least bem_ss2d_scan_n_bwd_ws_elems(B, C, L, N) floats (the forward states entering every 256-position tile). */
int64_t bem_ss2d_scan_n_bwd_ws_elems(int B, int C, int L, int N);
int bem_ss2d_scan_n_bwd_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dy0, const float* dy1,
                            const float* dtw, const float* dtb, const float* A, const float* Ds, float* dx0, float* dx1, float* dxd0,
                            float* dxd1, float* dAlog, float* dDs, float* ddtw, float* ddtb, float* ws, int64_t ws_elems, int B, int C,
                            int L, int R, int N, int64_t xd0_bstride, int64_t xd1_bstride, void* stream);

/* Output head of the two-branch Stage-II archs (replaces TunedModel_arch.py:315-319,406 and FusedModel_arch.py:234-238,330:
 * fusion = Sequential(Conv2d(6,3,3,p=1), ReLU, Conv2d(3,3,3,p=1)) applied to cat(out_1, out_2); and TwoBranchNaive_arch.py:268).
 *   mode 0: out = conv2(relu(conv1(cat(o1, o2)) + b1)) + b2, h zero-padded at the image border like nn.Conv2d.
 *           w1 (3,6,3,3), b1 (3), w2 (3,3,3,3), b2 (3), read on the device.
 *   mode 1: out = (o1 + o2) / 2 (weights unused, may be NULL).
 * o1 / o2 (B,3,H,W) planes contiguous, batch strides o*_bstride elements (0 = 3*H*W); out (B,3,H,W) contiguous.  Only C_out = 3 and
 * C_in = 6 (two 3-channel branch outputs) are supported; other values are refused. */
int bem_fusion_head_f32(const float* o1, int64_t o1_bstride, const float* o2, int64_t o2_bstride, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* out, int B, int Cin, int Cout, int H, int W, int mode, void* stream);
/* Backward of bem_fusion_head_f32.  The pre-activation is recomputed from o1 / o2 (nothing is saved by the forward); the ReLU passes
 * the gradient where pre > 0 only (threshold_backward).  do1 / do2 (B,3,H,W) contiguous are written.  mode 0: dw1, db1, dw2, db2
 * += the weight gradients, summed from per-workgroup partials in ws (at least bem_fusion_head_bwd_ws_elems(B, H, W) floats) in f64
 * in a fixed order by a second launch -- bitwise reproducible, no float atomics.  mode 1: do1 = do2 = dout / 2 (o1, o2, weights,
 * ws unused). */
int64_t bem_fusion_head_bwd_ws_elems(int B, int H, int W);
int bem_fusion_head_bwd_f32(const float* o1, int64_t o1_bstride, const float* o2, int64_t o2_bstride, const float* dout, const float* w1,
                            const float* b1, const float* w2, float* do1, float* do2, float* dw1, float* db1, float* dw2, float* db2,
                            float* ws, int64_t ws_elems, int B, int Cin, int Cout, int H, int W, int mode, void* stream);

/* clip_grad_norm_ + torch.optim.AdamW on one flat parameter buffer.  bem_grad_sumsq_f32: acc[0] = sum g^2 (f64, zeroed by the
 * call).  bem_adamw_step_f32: g *= min(1, max_norm / (sqrt(sumsq) + 1e-6)) when max_norm > 0 (read on the device), then the AdamW
 * update with bias corrections of `step` (>= 1); norm_out (or NULL) receives the unclipped total norm.  hyper (NULL or three floats
 * in device memory: lr, 1 - beta1^t, sqrt(1 - beta2^t)) overrides lr / step with values read by the kernel -- the per-iteration
 * inputs of a captured step. */
int bem_grad_sumsq_f32(const float* g, int64_t n, double* acc, void* stream);
int bem_adamw_step_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int step, float max_norm, const double* sumsq, float* norm_out, const float* hyper,
                       void* stream);
/* torch.optim.Adam (amsgrad=False, maximize=False) in place of AdamW, everything else as bem_adamw_step_f32 (the clip, norm_out,
 * hyper): the weight decay enters the gradient the moments see, g' = g + weight_decay * p, and the parameter is not scaled:
 *   m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 * g receives the clipped gradient, not g'.  One kernel body with AdamW, chosen by a compile-time flag. */
int bem_adam_step_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float max_norm, const double* sumsq, float* norm_out, const float* hyper,
                      void* stream);

/* base_model.py:77-84: ema = decay * ema + (1 - decay) * p over n floats.
 * The averaged copy of the weights (train.ema_decay), one launch per flat parameter buffer, after the optimizer step.  The host passes
 * decay = (float)decay and one_minus_decay = (float)(1.0 - (double)decay), the two constants of torch's mul_(decay).add_(p, alpha=1 - decay);
 * per element the kernel computes fmaf(one_minus_decay, p, decay * ema): the product decay * ema rounded once, then one fused
 * multiply-add.  decay == 0 gives ema = p bit for bit (model_ema(0), the initial copy).  ema and p must not overlap.  16-byte vector
 * accesses when both pointers are 16-byte aligned, scalar ones otherwise and for the last n % 4 elements.  n == 0 returns 0 without a
 * launch; n < 0 or a null pointer is BEM_ERR_INVALID. */
int bem_ema_update_f32(float* ema, const float* p, int64_t n, float decay, float one_minus_decay, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage-I training: ConditionGenerator.optimize_parameters,
 * basicsr/models/condition_generator_model.py:176-218.  Everything else of that step runs on the Stage-II training entry points.
 * --------------------------------------------------------------------------------------------- */

/* Writes n (<= 512) 32-bit words from HOST memory into device memory at dst, carried as the arguments of one kernel launch on
 * `stream` (ordered with the launches around it; the host buffer may be reused at once).  The per-iteration inputs of a captured
 * Stage-I step (stream_add of the samplers, hyper of bem_adamw_step_f32, decay_dev below) are refreshed with it before each replay. */
int bem_store_words(void* dst, const void* host_words, int n, void* stream);

/* Threshold-EMA prior of a Bayesian leaf (basicsr/bayesian/conv.py:86-98, linear.py:63-74):
 * prior = decay * prior + (1 - decay) * current, for mu and rho; the caller passes decay = min(layer.decay, (1 + step) / (10 + step)),
 * by value or (decay_dev != NULL) as one float in device memory that the kernel reads -- the form a captured step uses. */
int bem_bnn_prior_ema_f32(float* prior_mu, float* prior_rho, const float* mu, const float* rho, float decay, const float* decay_dev,
                          int64_t n, void* stream);

/* The four Bayesian training steps (prior EMA + eps draw + sample, KL, KL backward, reparameterisation backward) for ALL Bayesian
 * tensors of a net in one launch each.  segs: nseg x 8 64-bit words {mu, rho, dmu, drho pointers; first element in the arenas
 * (multiple of 4); elements n; stream counter; float 1/n in the low half of the last word}; blks: nblk x {int32 segment, int32 first
 * element}: one workgroup = 1024 consecutive elements of one segment.  prior_mu / prior_rho / w / eps / gw are flat arenas indexed by
 * segment offset + element.  sample: prior = decay prior + (1 - decay) param; eps = the Philox draw bem_randn_f32 makes for
 * (seed, stream_base + counter [+ *stream_add]); w = mu + log1p(exp(rho)) eps; gw = 0.  kl / kl_bwd / reparam_bwd: as the per-tensor
 * entry points below, gradients accumulated through the dmu / drho pointers.  Replaces conv.py:84-112 + tools.py:76-84 over a net. */
int bem_bnn_bank_sample_f32(const void* segs, const void* blks, int nblk, float* prior_mu, float* prior_rho, float* w, float* eps, float* gw,
                            float decay, const float* decay_dev, uint64_t seed, uint64_t stream_base, const uint64_t* stream_add, void* stream);
int bem_bnn_bank_kl_f32(const void* segs, const void* blks, int nblk, const float* prior_mu, const float* prior_rho, float* out, void* stream);
int bem_bnn_bank_kl_bwd_f32(const void* segs, const void* blks, int nblk, const float* prior_mu, const float* prior_rho, const float* g,
                            void* stream);
int bem_bnn_bank_reparam_bwd_f32(const void* segs, const void* blks, int nblk, const float* gw, const float* eps, void* stream);

/* out[0] += mean( log sp - log sq + (sq^2 + (mu - prior_mu)^2) / (2 sp^2) - 0.5 ), s = log1p(exp(rho))  (base_layer.py:26-40 kl_div). */
int bem_bnn_kl_f32(const float* mu, const float* rho, const float* prior_mu, const float* prior_rho, int64_t n, float* out, void* stream);

/* gradient of g[0] * (that mean) accumulated into dmu / drho (g: one float on the device, the upstream gradient of the KL term). */
int bem_bnn_kl_bwd_f32(const float* mu, const float* rho, const float* prior_mu, const float* prior_rho, int64_t n, const float* g,
                       float* dmu, float* drho, void* stream);

/* Reparameterisation w = mu + log1p(exp(rho)) * eps (conv.py:100-104): dmu += gw, drho += gw * eps * sigmoid(rho). */
int bem_bnn_reparam_bwd_f32(const float* gw, const float* eps, const float* rho, float* dmu, float* drho, int64_t n, void* stream);

/* Masked-image-modelling mix (basicsr/archs/UNet_arch.py:463-466): out = fea * (1 - w) + token[c] * w, w = mask (B,H,W);
 * backward: dfea = dout * (1 - w), dtoken[c] += sum dout * w. */
int bem_mask_token_f32(const float* fea, const float* mask, const float* token, float* out, int B, int C, int H, int W, void* stream);
int bem_mask_token_bwd_f32(const float* dout, const float* mask, float* dfea, float* dtoken, int B, int C, int H, int W, void* stream);

/* Inverse of bem_space_to_depth_f32 (= backward of PatchMerging's gather, UNet_arch.py:74-78): d4 (B,4C,H/2,W/2) -> dx (B,C,H,W). */
int bem_depth_to_space_f32(const float* d4, float* dx, int B, int C, int H, int W, void* stream);

/* nn.PReLU() with one shared slope (DualUpSample, UNet_arch.py:106,120): forward, and backward dx = dout * (x >= 0 ? 1 : a),
 * dslope[0] += sum dout * x over x < 0. */
int bem_prelu_f32(const float* x, const float* slope, float* out, int64_t n, void* stream);
int bem_prelu_bwd_f32(const float* x, const float* slope, const float* dout, float* dx, float* dslope, int64_t n, void* stream);

/* Adjoint of bem_bilinear_up_f32 (nn.Upsample(scale_factor = s, bilinear, align_corners = False), UNet_arch.py:121-123):
 * dout (B,C,H*s,W*s) -> dx (B,C,H,W), zeroed by the call. */
int bem_bilinear_up_bwd_f32(const float* dout, float* dx, int B, int C, int H, int W, int s, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VGG19 perceptual loss (basicsr/losses/basic_loss.py:146-238): the kernels between its convolutions (csrc/percep.hip).
 * All tensors f32, channel-planar, contiguous; every kernel is one pass and writes each output element itself (no memset).
 * ------------------------------------------------------------------------------------------- */

/* Input normalisation of VGGFeatureExtractor.forward (basicsr/archs/vgg_arch.py:150-153) for both images at once:
 * pred, gt (B,3,H,W) -> xn (2B,8,H,W), rows [0,B) from pred and [B,2B) from gt; channels 0..2 = (x - mean) / std (input_norm; a true
 * division) after x = (x + 1) / 2 (range_norm), channels 3..7 zero (conv1_1 with its weight zero-padded to 8 input channels). */
int bem_vgg_prep_f32(const float* pred, const float* gt, float* xn, int B, int H, int W, int input_norm, int range_norm, void* stream);
/* Its adjoint for the pred rows: dpred (B,3,H,W) = dxn[:, :3] / std (/ 2 under range_norm); dxn_bstride = elements between rows of dxn. */
int bem_vgg_prep_bwd_f32(const float* dxn, int64_t dxn_bstride, float* dpred, int B, int H, int W, int input_norm, int range_norm,
                         void* stream);

/* nn.MaxPool2d(kernel_size=2, stride=2) (vgg_arch.py:120): x (planes,H,W) -> out (planes,H/2,W/2), floor: an odd last row / column is
 * dropped.  H, W >= 2. */
int bem_maxpool2_f32(const float* x, float* out, int64_t planes, int H, int W, void* stream);
/* Backward of pool(y) with y = relu(.) and of that ReLU (autograd of vgg_arch.py:156-157 over a 'relu*', 'pool*' pair): dy (planes,H,W) =
 * dpool (planes,H/2,W/2) of the window at its first maximum in row-major order (torch's rule) where y > 0 there, zero elsewhere -- a
 * dropped odd row / column included. */
int bem_relu_pool_bwd_f32(const float* y, const float* dpool, float* dy, int64_t planes, int H, int W, void* stream);
/* Backward of nn.ReLU (vgg_arch.py:156-157 over a 'relu*' entry) on its output y: out = dy * (y > 0); out may be dy. */
int bem_relu_bwd_f32(const float* y, const float* dy, float* out, int64_t n, void* stream);
/* nn.ReLU (the same lines): needed where a requested 'conv*' feature is kept before its ReLU and the walk goes on; out may be x. */
int bem_relu_f32(const float* x, float* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LPIPS v0.1 with the AlexNet trunk (csrc/lpips.hip; the metric of Enhancement/eval.py:143-145,301-306 and
 * Enhancement/cal_metrics_with_imgs.py:39-41,51-55).  The five convolutions are bem_conv2d_f32.
 * ------------------------------------------------------------------------------------------- */

/* Input stage for both images at once, written as the operand of the first convolution.  ref, pred (B,3,H,W), H, W >= 31 (below that the
 * second pool has no output).  mode 1: images in [0,1] -> u = rint(clip(x,0,1) * 255) (img_as_ubyte, the quantisation of
 * bem_ssim_f32), u / 127.5 - 1 (lpips.im2tensor); mode 0: x is already in [-1,1]; mode 2: 2 x - 1 (forward(normalize=True)).  Then the scaling layer (x - shift_c) / scale_c, true f32
 * divisions.  xs (2B,48,Hb,Wb), rows [0,B) from ref and [B,2B) from pred, Hb = (H-7)/4 + 3, Wb = (W-7)/4 + 3 rounded up to even: block
 * (by,bx), channel 16 c + 4 dy + dx holds the scaled pixel (4 by - 2 + dy, 4 bx - 2 + dx) of colour c, zero outside the image.  With the
 * 11x11 weight zero-padded to 12x12 and cut the same way into (64,48,3,3), conv1 of AlexNet (stride 4, pad 2) at (oy,ox) is the 3x3 pad-1
 * convolution of xs at (oy + 1, ox + 1). */
int bem_lpips_prep_f32(const float* ref, const float* pred, float* xs, int B, int H, int W, int mode, void* stream);

/* nn.MaxPool2d(kernel_size=3, stride=2), floor mode, no padding, torch's NaN rule (a NaN in the window is the result): x (planes,H,W) read
 * at x_pstride elements between planes and x_rstride between rows (a cropped view of a wider tensor) -> out (planes,(H-3)/2+1,(W-3)/2+1)
 * contiguous.  H, W >= 3. */
int bem_maxpool3s2_f32(const float* x, int64_t x_pstride, int64_t x_rstride, float* out, int64_t planes, int H, int W, void* stream);

/* Distance head of one layer: feat (2B,C,h,w) at the given batch / channel / row strides, rows b and B + b the two images of pair b; lin (C)
 * the layer's 1x1 weights.  Per pixel in f64: yhat = y * (1 / (sqrt(sum_c y^2) + 1e-10)) for both images, sum_c lin[c] (yhat0 - yhat1)^2; then the
 * mean over pixels from per-workgroup partials added in a fixed order (no atomics: a call repeats bit for bit).  ws: at least
 * bem_lpips_layer_ws_elems(B,h,w) doubles; ws[0,B) is the running sum over layers, started from zero by the call with first != 0 and
 * added to by the others, so the calls of one metric share one ws; out (B) f32 = that sum after this layer. */
int64_t bem_lpips_layer_ws_elems(int B, int h, int w);
int bem_lpips_layer_f32(const float* feat, int64_t f_bstride, int64_t f_cstride, int64_t f_rstride, const float* lin, double* ws,
                        int64_t ws_elems, float* out, int B, int C, int h, int w, int first, void* stream);

/* LPIPS as a loss term (basicsr.losses.LPIPSLoss over bem.autograd.LPIPSFn): loss_weight * mean_b d(ref_b, pred_b) and its gradient with
 * respect to pred, input modes 0 and 2 of bem_lpips_prep_f32.  Each kernel writes every output element once: a call repeats bit for bit. */

/* loss[0] = weight * mean of acc[0,B), acc the f64 running sums in the workspace of the last bem_lpips_layer_f32 call (ws[0,B)). */
int bem_lpips_mean_f32(const double* acc, float* loss, int B, float weight, void* stream);

/* Head backward of one layer, pred rows [B,2B) only; feat / lin / strides as bem_lpips_layer_f32 takes them.  Per pixel in f64 from the f32
 * features: n = sqrt(sum_c y^2), r = 1 / (n + 1e-10), a = y_ref r_ref, b = y_pred r_pred, D_c = -2 lin_c (a_c - b_c) (the two products
 * rounded separately: equal images give exactly 0), g_k = r_pred D_k - y_pred,k (r_pred / n_pred) sum_c b_c D_c, the second term 0 where
 * n_pred = 0; times scale * gmul[0] / (h w) with scale = loss_weight / B and gmul the device scalar dL/dloss (NULL = 1).
 * gin (or NULL): (B,C,h,w) contiguous, the gradient that reaches the same post-ReLU feature from the layer above.
 * dz (B,C,oh,ow) at its batch / channel / row strides: (y_pred > 0) ? gin + g : 0 -- the gradient at the convolution's output, before the
 * ReLU -- at rows [oy0, oy0+h) and columns [ox0, ox0+w), zero at every other position of the oh x ow extent (layer 0: conv1's block grid
 * around its crop, oy0 = ox0 = 1).  A pixel whose pred features are all zero gets 0, where autograd of y / (|y| + eps) gives NaN. */
int bem_lpips_layer_bwd_f32(const float* feat, int64_t f_bstride, int64_t f_cstride, int64_t f_rstride, const float* lin, const float* gin,
                            const float* gmul, float scale, float* dz, int64_t d_bstride, int64_t d_cstride, int64_t d_rstride, int B, int C,
                            int h, int w, int oh, int ow, int oy0, int ox0, void* stream);

/* Backward of bem_maxpool3s2_f32: y (planes,H,W) at y_pstride / y_rstride is the pool's input, dpool (planes,(H-3)/2+1,(W-3)/2+1) the
 * gradient of its output, dy (planes,H,W) contiguous.  A gather: each input pixel adds dpool of those of the up to four windows covering
 * it whose first maximum in row-major order it is (torch's rule; ties go to the first); pixels no window covers get 0.  y is a ReLU
 * output in the loss, but the mask y > 0 is NOT applied here: bem_lpips_layer_bwd_f32 applies it to its gin.  H, W >= 3, H*W < 2^31,
 * planes < 2^31. */
int bem_relu_pool3s2_bwd_f32(const float* y, int64_t y_pstride, int64_t y_rstride, const float* dpool, float* dy, int64_t planes, int H,
                             int W, void* stream);

/* Adjoint of bem_lpips_prep_f32 for the pred rows: gxs (B,48,Hb,Wb) contiguous, the gradient of the block-form operand;
 * dpred[b,c,y,x] = k * gxs[b, 16 c + 4 ((y+2) % 4) + (x+2) % 4, (y+2) / 4, (x+2) / 4] / scale_c (one true f32 division), k = 2 in mode 2
 * and 1 in mode 0.  Mode 1 quantises and has no gradient: refused.  H, W >= 31, H*W < 2^31. */
int bem_lpips_prep_bwd_f32(const float* gxs, float* dpred, int B, int H, int W, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training batches from the device-resident image store (csrc/batch_assemble.hip): Dataset_PairedImage_Mask.__getitem__ for a whole
 * batch in one launch (basicsr/data/paired_image_dataset.py:333-379: utils/img_util.py:196-211 padding, data/transforms.py:228-273
 * data_augmentation, utils/labelnoise.py:55-69 add_label_noise, the cv2.resize condition planes :366-371, img2tensor :375-379).
 *
 * lq_arena / gt_arena: arena_bytes of uint8 each; image i is (H,W,3) RGB at byte table[3i] with H = table[3i+1], W = table[3i+2] (any
 * offset, the arenas are read byte-wise).  plan row j = (image, top, left, mode): the crop [top, top+Sh) x [left, left+Sw) of the image
 * padded 'symmetric' at the bottom / right to at least (Sh, Sw), then rot90(mode / 2) and flipud if mode is odd, / 255.f, written
 * channel-first to lq[j], gt[j] (B,3,Sh,Sw).  noise_steps (bit 0 temperature, 1 brightness, 2 contrast; 0 = off) applies the label noise
 * of noise row j = (t, b, c) to gt: blue * t and red / t in float64, clipped to [0,1], rounded to f32; * b clipped; c * (x - 0.5) + 0.5
 * clipped.  lq_down, gt_down (B,3,Sh/s,Sw/s) = the x1/s INTER_LINEAR planes of the finished lq[j], gt[j], bit for bit what
 * bem_resize_down_f32 returns for them.  table_host / plan_host are host copies of table_dev / plan_dev (n_img rows, B rows): every
 * row is checked against the store on the host before the launch.  s even, Sh % s == Sw % s == 0, or s = 0 with null lq_down / gt_down
 * (no condition planes: whole validation images of any size); modes 2, 3, 6, 7 need Sh == Sw. */
int bem_batch_assemble_u8(const uint8_t* lq_arena, const uint8_t* gt_arena, int64_t arena_bytes, const int64_t* table_host,
                          const int64_t* table_dev, int n_img, const int32_t* plan_host, const int32_t* plan_dev, const float* noise_dev,
                          int noise_steps, int B, int Sh, int Sw, int s, float* lq, float* gt, float* lq_down, float* gt_down, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEM_HIP_H */
