// Pointwise (1x1) channel-mix GEMM, f32 in / f32 out, products on the bf16 matrix cores as a 3-limb expansion.
//
//   out[b][m][p] = act(sum_k W[m][k] * pro(x)[b][k][p] + bias[m]) + res[b][m][p]        (argument block bem_pw_args, include/bem_hip.h)
//
// Why: v_mfma_f32_32x32x2_f32 delivers 64 FLOP / cycle / SIMD, v_mfma_f32_32x32x16_bf16 1024.  Every f32 operand is
// split exactly into three bf16 limbs  v = h + m + l  (round-to-nearest at each step, exact f32 residuals), and a
// product is evaluated as the six limb products of weight >= 2^-16 relative
//        x*w ~ xl*wh + xh*wl + xm*wm + xm*wh + xh*wm + xh*wh          (dropped: xm*wl + xl*wm + xl*wl <= 2^-23 |x w|)
// each of which is exact in the f32 accumulator of the MFMA.  The result carries f32-level error (the dropped terms
// are of the order of one f32 rounding of the product) at 6/16 of the f32-MFMA cost, which moves these GEMMs from
// the matrix pipe to the HBM roofline.  Parity tests hold it to the same tolerances as the native-f32 kernels.
//
// Mapping (NCHW, pixels on lanes):
//   * one wave = 32 * NSUB consecutive pixels; lane l owns pixels p0 + NSUB * (l & 31) + t, t < NSUB (one float2 load
//     per lane and channel for NSUB = 2).  Sub-tile t (pixels with the same t) is one MFMA N-tile.
//   * k-block kb covers input channels 16 kb .. 16 kb + 15; lanes 0-31 hold channels 16 kb + 0..7, lanes 32-63
//     channels 16 kb + 8..15 (the B[k = 8 (l >> 5) + e][n = l & 31] layout of the 32x32x16 instruction).
//   * weights arrive pre-split and pre-packed by bem_pack_pw_weight_x6: Wp[mtile][kb][limb][lane] is one 16-byte
//     vector = W[32 mtile + (lane & 31)][16 kb + 8 (lane >> 5) + e], e = 0..7, so an A operand is one coalesced
//     1 KiB load per (M-tile, k-block, limb), L1/L2 resident.
//   * D layout: column = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (acc_row, x6_common.h).
//   * "resident" kernel: the wave's whole input tile (all K channels, already normalised and split) stays in
//     registers while the wave walks over every M-tile, so x is read once and LayerNorm evaluated once;
//     "stream" kernel (any K; LayerNorm by two more sweeps over x): x is streamed k-block by k-block, ahead of the MFMAs.
//   * "small" kernel (planes of at most 128 pixels, Stage I's 4x4 and 8x8 maps): the k-blocks of a pixel-wave are shared among the four
//     (two) waves of the workgroup, each requests its slice of the weight stream up front, and the partial sums meet in LDS in a fixed
//     order (pw_x6_small_kernel below).  The three forms above give each wave its own pixels, so on such a plane one wave works alone.
#include "bem_common.h"
#include "x6_common.h"
#include <algorithm>

namespace {


struct PwX {
    const float* x1; const float* x2; int C1; int C2; int in_mode;
    const float* ln_w; const float* ln_b; float ln_eps;
    const u32x4* Wp; int64_t w_bstride;       // stride in 16-byte vectors
    const float* bias; int64_t bias_bstride;
    const float* res; const float* prelu; int act;
    float* out; int out_mode; int Win;
    int M; int K; int L; int KB; int MT;
    int mtpb;      // resident kernel: M-tiles per workgroup (grid.y slices M when there are too few pixels to fill the GPU)
};


// Branch-free input fetch: always a clamped, valid address, value masked afterwards.
// Returns pro-input channel ch at this lane's NSUB pixels (pixel index pc clamped by the caller, keep[t] per pixel).
template <int NSUB, bool SUM, bool VEC>
__device__ __forceinline__ void ldx(const PwX& k, int b, int ch, int pc, const bool (&keep)[NSUB], float (&o)[NSUB]) {
    const int chc = min(ch, k.K - 1);
    const bool first = chc < k.C1;
    const float* r1 = k.x1 + ((int64_t)b * k.C1 + (first ? chc : 0)) * k.L;
    const float* r2 = k.x2 + ((int64_t)b * k.C2 + (first ? 0 : chc - k.C1)) * k.L;
    const float* base = first ? r1 : r2;
    const float* sec = k.x2 + ((int64_t)b * k.C2 + chc) * k.L;     // only dereferenced when SUM
    if (NSUB == 2 && VEC) {
        float2 v = *reinterpret_cast<const float2*>(base + pc);
        if (SUM) { const float2 w = *reinterpret_cast<const float2*>(sec + pc); v.x += w.x; v.y += w.y; }
        o[0] = v.x; o[NSUB - 1] = v.y;
    } else {
#pragma unroll
        for (int t = 0; t < NSUB; ++t) {
            const int pi = min(pc + t, k.L - 1);
            o[t] = base[pi];
            if (SUM) o[t] += sec[pi];
        }
    }
    const float mk = ch < k.K ? 1.f : 0.f;
#pragma unroll
    for (int t = 0; t < NSUB; ++t) o[t] = keep[t] ? o[t] * mk : 0.f;
}

// bias comes from LDS (s_bias, zero-filled without a bias), the residual is fetched under ONE uniform branch per batch
// of rows: every global round trip in here is latency the wave cannot hide (2 waves per SIMD), so there is none
// unless a residual is actually present.
template <int MTW, int NSUB, bool VEC>
__device__ __forceinline__ void x6_epilogue_generic(const PwX& k, int b, int mt0, int p, const bool (&keep)[NSUB], int kh,
                                                    const float* __restrict__ s_bias, const f32x16 (&acc)[MTW][NSUB]) {
    const float slope = (k.act == 1) ? k.prelu[0] : 0.f;
    const bool has_res = k.res && k.out_mode == 0;
    const float* resp = k.res + (int64_t)b * k.M * k.L;
    const int pv = VEC ? (keep[0] ? p : 0) : p;
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        if (mt0 + m >= k.MT) continue;
        const int rbase = (mt0 + m) * 32;
#pragma unroll
        for (int rh = 0; rh < 16; rh += 8) {
            float rv[8][NSUB];
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                for (int t = 0; t < NSUB; ++t) rv[r8][t] = 0.f;
            if (has_res) {
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8) {
                    const int r = rh + r8;
                    const float* rp = resp + (int64_t)min(rbase + acc_row(r, kh), k.M - 1) * k.L;
                    if (NSUB == 2 && VEC) {
                        const float2 q = *reinterpret_cast<const float2*>(rp + pv);
                        rv[r8][0] = q.x; rv[r8][NSUB - 1] = q.y;
                    } else {
#pragma unroll
                        for (int t = 0; t < NSUB; ++t) rv[r8][t] = rp[min(pv + t, k.L - 1)];
                    }
                }
            }
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) {
                const int r = rh + r8;
                const int row = rbase + acc_row(r, kh);
                if (row >= k.M) continue;
                const float bv = s_bias[row];
                float o[NSUB];
#pragma unroll
                for (int t = 0; t < NSUB; ++t) {
                    o[t] = acc[m][t][r] + bv;
                    if (k.act == 1) o[t] = o[t] >= 0.f ? o[t] : slope * o[t];
                    o[t] += rv[r8][t];
                }
                if (k.out_mode == 0) {
                    float* op = k.out + ((int64_t)b * k.M + row) * k.L + p;
                    if (NSUB == 2 && VEC) {
                        if (keep[0]) *reinterpret_cast<float2*>(op) = make_float2(o[0], o[NSUB - 1]);
                    } else {
#pragma unroll
                        for (int t = 0; t < NSUB; ++t)
                            if (keep[t]) op[t] = o[t];
                    }
                } else {
                    const int Co = k.M >> 2;
                    const int q = row / Co, co = row - q * Co;
                    const int64_t obase = ((int64_t)b * Co + co) * (4 * (int64_t)k.L);
#pragma unroll
                    for (int t = 0; t < NSUB; ++t) {
                        if (keep[t]) {
                            const int pp = p + t;
                            const int yy = pp / k.Win, xx = pp - yy * k.Win;
                            k.out[obase + (int64_t)(2 * yy + (q >> 1)) * (2 * k.Win) + (2 * xx + (q & 1))] = o[t];
                        }
                    }
                }
            }
        }
    }
}

// out_mode 0 epilogue with the address arithmetic kept off the vector ALU: a row's plane base is wave-uniform (scalar
// registers), the lane contributes one 32-bit element offset computed once (its pixel and its 4-row half), so a store
// is `global_store v_off, v_data, s[base]`; the 16 bias values of an M-tile arrive in registers (x6_load_bias).  PReLU and
// the residual are compile-time variants (chosen by uniform branches in x6_epilogue): without them a value costs one add.
template <int MTW, int NSUB, bool VEC, bool ACT, bool RES>
__device__ __forceinline__ void x6_epilogue_rows(const PwX& k, int b, int mt0, int p, const bool (&keep)[NSUB], int kh,
                                                 const float4 (&bq)[MTW][4], const f32x16 (&acc)[MTW][NSUB]) {
    const float slope = ACT ? k.prelu[0] : 0.f;
    const int pv = VEC ? (keep[0] ? p : 0) : min(p, k.L - 1);
    const uint32_t loff = (uint32_t)(4 * kh) * (uint32_t)k.L + (uint32_t)pv;
    float* outb = k.out + (int64_t)b * k.M * k.L;
    const float* resb = RES ? k.res + (int64_t)b * k.M * k.L : nullptr;
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        if (mt0 + m >= k.MT) continue;
        const int rb = (mt0 + m) * 32;                        // uniform
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // through a VALU copy: a packed add that takes the HIGH register of a freshly loaded pair for its LOW result read the pair's
            // pre-load content in lanes 48..63 (round 3: the M = 32, K = 64 attention-fuse GEMM at 280 workgroups, scripts/dbg_gemm_cat.py;
            // round 2 saw the same with LDS-loaded pairs) -- DESIGN.md section 6.4, scripts/isa_audit.py check 2
            const float bv[4] = {valu_copy(bq[m][g].x), valu_copy(bq[m][g].y), valu_copy(bq[m][g].z), valu_copy(bq[m][g].w)};
            float rv[4][NSUB];
            if (RES) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int urow = rb + 8 * g + i;
                    const float* rp = resb + (int64_t)min(urow, k.M - 1) * k.L;          // uniform plane base, clamped
                    const uint32_t lo = urow + 4 * kh < k.M ? loff : (uint32_t)pv;        // rows >= M (never stored) read a valid row
                    if (NSUB == 2 && VEC) {
                        const float2 q = *reinterpret_cast<const float2*>(rp + lo);
                        rv[i][0] = q.x; rv[i][NSUB - 1] = q.y;
                    } else {
#pragma unroll
                        for (int t = 0; t < NSUB; ++t) rv[i][t] = rp[lo + (pv + t < k.L ? t : 0)];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * g + i;
                const int urow = rb + 8 * g + i;              // uniform; this lane's row = urow + 4 kh
                float o[NSUB];
#pragma unroll
                for (int t = 0; t < NSUB; ++t) {
                    o[t] = acc[m][t][r] + bv[i];
                    if (ACT) o[t] = o[t] >= 0.f ? o[t] : slope * o[t];
                    if (RES) o[t] += rv[i][t];
                }
                float* op = outb + (int64_t)urow * k.L;
                const bool rowok = urow + 4 * kh < k.M;
                if (NSUB == 2 && VEC) {
                    if (keep[0] && rowok) *reinterpret_cast<float2*>(op + loff) = make_float2(o[0], o[NSUB - 1]);
                } else {
#pragma unroll
                    for (int t = 0; t < NSUB; ++t)
                        if (keep[t] && rowok) op[loff + t] = o[t];
                }
            }
        }
    }
}

// This lane's 16 bias values of each M-tile of a group (rows rb + 8 g + 4 kh + i), fetched with the group's first weights
// so that the epilogue finds them in registers.  M % 4 == 0: four 16-byte loads (the half-wave reads one address);
// otherwise scalar reads with clamped rows.  (An LDS copy read back as float4 returned a stale third component for the
// upper half-wave a few times per 10^7 outputs under load; it is used by the generic epilogue only, as scalars.)
template <int MTW>
__device__ __forceinline__ void x6_load_bias(const PwX& k, int b, int mt0, int kh, float4 (&bq)[MTW][4]) {
    const float* gb = k.bias ? k.bias + (int64_t)b * k.bias_bstride : nullptr;      // uniform
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) bq[m][g] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!gb) return;
    if ((k.M & 3) == 0) {
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                bq[m][g] = *reinterpret_cast<const float4*>(gb + min((mt0 + m) * 32 + 8 * g + 4 * kh, k.M - 4));   // rows >= M are never stored
    } else {
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r0 = (mt0 + m) * 32 + 8 * g + 4 * kh;
                bq[m][g] = make_float4(gb[min(r0, k.M - 1)], gb[min(r0 + 1, k.M - 1)], gb[min(r0 + 2, k.M - 1)], gb[min(r0 + 3, k.M - 1)]);
            }
    }
}

template <int MTW, int NSUB, bool VEC>
__device__ __forceinline__ void x6_epilogue(const PwX& k, int b, int mt0, int p, const bool (&keep)[NSUB], int kh,
                                            const float* __restrict__ s_bias, const float4 (&bq)[MTW][4], const f32x16 (&acc)[MTW][NSUB]) {
    if (k.out_mode != 0 || k.M < 8) { x6_epilogue_generic<MTW, NSUB, VEC>(k, b, mt0, p, keep, kh, s_bias, acc); return; }
    const bool act = k.act == 1, res = k.res != nullptr;      // uniform
    if (!act && !res) x6_epilogue_rows<MTW, NSUB, VEC, false, false>(k, b, mt0, p, keep, kh, bq, acc);
    else if (!act) x6_epilogue_rows<MTW, NSUB, VEC, false, true>(k, b, mt0, p, keep, kh, bq, acc);
    else if (!res) x6_epilogue_rows<MTW, NSUB, VEC, true, false>(k, b, mt0, p, keep, kh, bq, acc);
    else x6_epilogue_rows<MTW, NSUB, VEC, true, true>(k, b, mt0, p, keep, kh, bq, acc);
}

// bias of this batch row -> LDS (zeros without a bias); M <= BEM_X6_MAXM
constexpr int BEM_X6_MAXM = 2048;
__device__ __forceinline__ void stage_bias(const PwX& k, int b, float* s_bias) {
    const float* bias = k.bias ? k.bias + (int64_t)b * k.bias_bstride : nullptr;
    for (int i = threadIdx.x; i < k.MT * 32; i += 256) s_bias[i] = (bias && i < k.M) ? bias[i] : 0.f;
}

// ------------------------------------------------------------------------------------------------
// resident: K <= 16 * KBM.  grid (ceil(L / (128 * NSUB)), 1, B), 4 independent waves per workgroup.
// ------------------------------------------------------------------------------------------------
template <int KBM, int NSUB, int MTW, bool SUM, bool VEC>
__global__ __launch_bounds__(256, 2) void pw_x6_res_kernel(PwX k) {
    __shared__ float s_ln[2 * 16 * KBM];
    __shared__ __attribute__((aligned(16))) float s_bias[BEM_X6_MAXM];
    stage_bias(k, blockIdx.z, s_bias);
    for (int i = threadIdx.x; i < 16 * KBM; i += 256) {
        const bool on = k.ln_w && i < k.K;
        s_ln[i] = on ? k.ln_w[min(i, k.K - 1)] : 0.f;
        s_ln[16 * KBM + i] = on ? k.ln_b[min(i, k.K - 1)] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z;
    const int p0 = (xcd_tile(blockIdx.x, gridDim.x) * 4 + wave) * (32 * NSUB);
    const int p = p0 + NSUB * n;
    bool keep[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) keep[t] = p + t < k.L;
    // VEC (L even, p even): both pixels are kept or neither -> read at p or at 0; scalar form: ldx clamps every pixel itself
    const int pc = VEC ? (keep[0] ? p : 0) : p;
    float xr[KBM][8][NSUB];
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
        for (int e = 0; e < 8; ++e) ldx<NSUB, SUM, VEC>(k, b, 16 * kb + 8 * kh + e, pc, keep, xr[kb][e]);
    __syncthreads();                                            // s_ln visible (the only barrier; before any early exit)
    if (p0 >= k.L) return;
    if (k.ln_w) {
        const float inv = 1.f / (float)k.K;
        float mean[NSUB], rstd[NSUB];
#pragma unroll
        for (int t = 0; t < NSUB; ++t) {
            float s = 0.f;
#pragma unroll
            for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
                for (int e = 0; e < 8; ++e) s += xr[kb][e][t];
            s += __shfl_xor(s, 32, 64);
            mean[t] = s * inv;
            float q = 0.f;
#pragma unroll
            for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = (16 * kb + 8 * kh + e < k.K) ? xr[kb][e][t] - mean[t] : 0.f;     // padded channels do not count
                    q = fmaf(d, d, q);
                }
            q += __shfl_xor(q, 32, 64);
            rstd[t] = 1.f / sqrtf(q * inv + k.ln_eps);
        }
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // through a VALU copy: packed-f32 ops must not consume LDS-returned register pairs directly
                const float g = valu_copy(s_ln[16 * kb + 8 * kh + e]), be = valu_copy(s_ln[16 * KBM + 16 * kb + 8 * kh + e]);   // 0 on padded channels
#pragma unroll
                for (int t = 0; t < NSUB; ++t) xr[kb][e][t] = (xr[kb][e][t] - mean[t]) * rstd[t] * g + be;
            }
    }
    u32x4 xl[KBM][NSUB][3];
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
        for (int t = 0; t < NSUB; ++t) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = xr[kb][e][t];
            split8(v, xl[kb][t][0], xl[kb][t][1], xl[kb][t][2]);
        }
    const u32x4* wbase = k.Wp + (int64_t)b * k.w_bstride + lane;
    const int64_t mt_stride = (int64_t)k.KB * 3 * 64;           // vectors per M-tile
    // weights one k-block ahead of the MFMAs, across M-tile groups too (the first block of the next group is requested
    // before the epilogue of this one); k-blocks beyond KB and M-tiles beyond MT re-read a valid block and are masked to zero
    auto load_w = [&](int mt, int kb, u32x4 (&dst)[MTW][3]) {
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const bool ok = kb < k.KB && mt + m < k.MT;
            const u32x4* wp = wbase + (int64_t)(mt + m < k.MT ? mt + m : 0) * mt_stride + (int64_t)min(kb, k.KB - 1) * 3 * 64;
            load_w3_masked(wp, ok ? 0xffffffffu : 0u, dst[m]);
        }
    };
    u32x4 wn[MTW][3];
    const int mt_lo = blockIdx.y * k.mtpb, mt_hi = min(k.MT, mt_lo + k.mtpb);
    load_w(mt_lo, 0, wn);
    for (int mt0 = mt_lo; mt0 < mt_hi; mt0 += MTW) {
        f32x16 acc[MTW][NSUB], alo[MTW][NSUB];
        float4 bq[MTW][4];
        x6_load_bias<MTW>(k, b, mt0, kh, bq);
#pragma unroll
for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int t = 0; t < NSUB; ++t) acc[m][t] = alo[m][t] = zero16();
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb) {
            u32x4 wc[MTW][3];
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int li = 0; li < 3; ++li) wc[m][li] = wn[m][li];
            if (kb + 1 < KBM) load_w(mt0, kb + 1, wn);
            else load_w(mt0 + MTW, 0, wn);
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int t = 0; t < NSUB; ++t) mac6(wc[m], xl[kb][t], acc[m][t], alo[m][t]);
        }
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int t = 0; t < NSUB; ++t) acc[m][t] += alo[m][t];
        x6_epilogue<MTW, NSUB, VEC>(k, b, mt0, p, keep, kh, s_bias, bq, acc);
    }
}

// ------------------------------------------------------------------------------------------------
// resident, weights through LDS: K = 16 * KBM exactly, many M-tiles (level-2 project_in: K 160 -> M 1280).  In pw_x6_res_kernel each
// of the four waves pulls every weight block from L2 for its own 32 pixels, one k-block ahead: 1.2 MB per wave at two waves per SIMD is a
// latency chain (7 TB/s of L2 reads in flight-limited pieces, matrix pipe 15 % busy).  Here the workgroup fetches an M-tile's KBM * 3 KiB of
// weights ONCE by LDS-DMA, a whole M-tile ahead of the MFMAs that read it, and the four waves share it: a quarter of the L2 traffic and
// 30 KiB in flight per workgroup.  One barrier per M-tile; waves beyond the image keep running (masked stores) so that every wave reaches it.
// ------------------------------------------------------------------------------------------------
template <int KBM, bool SUM, bool VEC>
__global__ __launch_bounds__(256, 2) void pw_x6_res_lds_kernel(PwX k) {
    __shared__ float s_ln[2 * 16 * KBM];
    __shared__ __attribute__((aligned(16))) float s_bias[BEM_X6_MAXM];
    __shared__ __attribute__((aligned(16))) u32x4 Ws[2][KBM * 3 * 64];
    stage_bias(k, blockIdx.z, s_bias);
    for (int i = threadIdx.x; i < 16 * KBM; i += 256) {
        const bool on = k.ln_w && i < k.K;
        s_ln[i] = on ? k.ln_w[min(i, k.K - 1)] : 0.f;
        s_ln[16 * KBM + i] = on ? k.ln_b[min(i, k.K - 1)] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z;
    const int p0 = (xcd_tile(blockIdx.x, gridDim.x) * 4 + wave) * 32;
    const int p = p0 + n;
    bool keep[1] = {p < k.L};
    const int pc = VEC ? (keep[0] ? p : 0) : p;
    const int mt_lo = blockIdx.y * k.mtpb, mt_hi = min(k.MT, mt_lo + k.mtpb);
    const u32x4* wsrc = k.Wp + (int64_t)b * k.w_bstride;
    const int64_t mt_stride = (int64_t)KBM * 3 * 64;
    auto dma = [&](int mt, int buf) {                               // KBM * 3 pieces of 1 KiB, dealt round-robin to the four waves
        const u32x4* src = wsrc + (int64_t)mt * mt_stride;
        for (int piece = wave; piece < KBM * 3; piece += 4)
            glds16(src + piece * 64, (uint32_t)lane * 16u, lds_addr(&Ws[buf][piece * 64]));
    };
    dma(mt_lo, 0);
    float xr[KBM][8][1];
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
        for (int e = 0; e < 8; ++e) ldx<1, SUM, VEC>(k, b, 16 * kb + 8 * kh + e, pc, keep, xr[kb][e]);
    __syncthreads();                                                // s_ln, s_bias visible
    if (k.ln_w) {
        const float inv = 1.f / (float)k.K;
        float s = 0.f;
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += xr[kb][e][0];
        s += __shfl_xor(s, 32, 64);
        const float mean = s * inv;
        float q = 0.f;
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = xr[kb][e][0] - mean;
                q = fmaf(d, d, q);
            }
        q += __shfl_xor(q, 32, 64);
        const float rstd = 1.f / sqrtf(q * inv + k.ln_eps);
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float g = valu_copy(s_ln[16 * kb + 8 * kh + e]), be = valu_copy(s_ln[16 * KBM + 16 * kb + 8 * kh + e]);
                xr[kb][e][0] = (xr[kb][e][0] - mean) * rstd * g + be;
            }
    }
    u32x4 xl[KBM][3];
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = xr[kb][e][0];
        split8(v, xl[kb][0], xl[kb][1], xl[kb][2]);
    }
    int buf = 0;
    for (int mt0 = mt_lo; mt0 < mt_hi; ++mt0, buf ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's pieces of M-tile mt0 have landed ...
        __syncthreads();                                            // ... everybody's have, and everybody is done reading the other buffer
        if (mt0 + 1 < mt_hi) dma(mt0 + 1, buf ^ 1);
        f32x16 acc[1][1], alo;
        float4 bq[1][4];
        x6_load_bias<1>(k, b, mt0, kh, bq);
        acc[0][0] = alo = zero16();
        const u32x4* wl = &Ws[buf][lane];
        u32x4 wn[3] = {wl[0], wl[64], wl[128]};
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb) {                         // LDS reads one k-block ahead of the MFMAs, no further (register budget)
            const u32x4 wc[3] = {wn[0], wn[1], wn[2]};
            if (kb + 1 < KBM) {
                wn[0] = wl[((kb + 1) * 3 + 0) * 64]; wn[1] = wl[((kb + 1) * 3 + 1) * 64]; wn[2] = wl[((kb + 1) * 3 + 2) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
            mac6(wc, xl[kb], acc[0][0], alo);
            __builtin_amdgcn_sched_barrier(0);
        }
        acc[0][0] += alo;
        x6_epilogue<1, 1, VEC>(k, b, mt0, p, keep, kh, s_bias, bq, acc);
    }
}

// ------------------------------------------------------------------------------------------------
// stream: any K, no LayerNorm.  grid (ceil(L / 256), ceil(MT / MTW), B); x one k-block ahead of the MFMAs.
// ------------------------------------------------------------------------------------------------
constexpr int BEM_X6_MAXK_LN = 1024;      // LayerNorm parameters of the streaming form live in LDS
template <int MTW, int NSUB, bool SUM, bool VEC, bool LN>
__global__ __launch_bounds__(256, 2) void pw_x6_stream_kernel(PwX k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z, mt0 = blockIdx.y * MTW;
    const int p0 = (xcd_tile(blockIdx.x, gridDim.x) * 4 + wave) * (32 * NSUB);
    __shared__ __attribute__((aligned(16))) float s_bias[BEM_X6_MAXM];
    __shared__ float s_ln[LN ? 2 * BEM_X6_MAXK_LN : 2];
    stage_bias(k, b, s_bias);
    if (LN) {
        for (int i = threadIdx.x; i < k.KB * 16; i += 256) {     // zero scale / shift on the padded channels
            s_ln[i] = i < k.K ? k.ln_w[i] : 0.f;
            s_ln[BEM_X6_MAXK_LN + i] = i < k.K ? k.ln_b[i] : 0.f;
        }
    }
    __syncthreads();                    // the only barrier, before any early exit
    if (p0 >= k.L) return;
    const int p = p0 + NSUB * n;
    bool keep[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) keep[t] = p + t < k.L;
    const int pc = VEC ? (keep[0] ? p : 0) : p;
    auto load_x = [&](int kb, float (&dst)[8][NSUB]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) ldx<NSUB, SUM, VEC>(k, b, 16 * kb + 8 * kh + e, pc, keep, dst[e]);   // channels >= K come back as zeros
    };
    // LayerNorm over K larger than the register-resident forms hold: statistics in a first sweep over the channels
    // (mean, then centred variance -- the second and third reads of x come from L1 / L2), normalisation on the fly below
    float mean[NSUB], rstd[NSUB];
    if (LN) {
        const float inv = 1.f / (float)k.K;
        float s[NSUB];
#pragma unroll
        for (int t = 0; t < NSUB; ++t) s[t] = 0.f;
        for (int kb = 0; kb < k.KB; ++kb) {
            float v[8][NSUB];
            load_x(kb, v);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int t = 0; t < NSUB; ++t) s[t] += v[e][t];
        }
#pragma unroll
        for (int t = 0; t < NSUB; ++t) { s[t] += __shfl_xor(s[t], 32, 64); mean[t] = s[t] * inv; }
        float q[NSUB];
#pragma unroll
        for (int t = 0; t < NSUB; ++t) q[t] = 0.f;
        for (int kb = 0; kb < k.KB; ++kb) {
            float v[8][NSUB];
            load_x(kb, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float mk = (16 * kb + 8 * kh + e < k.K) ? 1.f : 0.f;
#pragma unroll
                for (int t = 0; t < NSUB; ++t) { const float d = (v[e][t] - mean[t]) * mk; q[t] = fmaf(d, d, q[t]); }
            }
        }
#pragma unroll
        for (int t = 0; t < NSUB; ++t) { q[t] += __shfl_xor(q[t], 32, 64); rstd[t] = 1.f / sqrtf(q[t] * inv + k.ln_eps); }
    }
    f32x16 acc[MTW][NSUB], alo[MTW][NSUB];
#pragma unroll
for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int t = 0; t < NSUB; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][t][r] = alo[m][t][r] = 0.f;
    const u32x4* wbase = k.Wp + (int64_t)b * k.w_bstride + lane;
    const int64_t mt_stride = (int64_t)k.KB * 3 * 64;
    auto load_w = [&](int kb, u32x4 (&dst)[MTW][3]) {
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const bool ok = kb < k.KB && mt0 + m < k.MT;
            const u32x4* wp = wbase + (int64_t)(mt0 + m < k.MT ? mt0 + m : 0) * mt_stride + (int64_t)min(kb, k.KB - 1) * 3 * 64;
            load_w3_masked(wp, ok ? 0xffffffffu : 0u, dst[m]);
        }
    };
    // x two k-blocks ahead (the HBM stream: with 2 waves per SIMD one block in flight per wave covers ~4 TB/s at 2 us of
    // latency), weights one ahead (L1 / L2)
    float xn[8][NSUB], xn2[8][NSUB];
    u32x4 wn[MTW][3];
    load_x(0, xn);
    load_x(1, xn2);
    load_w(0, wn);
    for (int kb = 0; kb < k.KB; ++kb) {
        u32x4 xl[NSUB][3], wc[MTW][3];
#pragma unroll
        for (int t = 0; t < NSUB; ++t) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] = xn[e][t];
                if (LN) v[e] = (v[e] - mean[t]) * rstd[t] * valu_copy(s_ln[16 * kb + 8 * kh + e]) + valu_copy(s_ln[BEM_X6_MAXK_LN + 16 * kb + 8 * kh + e]);
            }
            split8(v, xl[t][0], xl[t][1], xl[t][2]);
        }
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int li = 0; li < 3; ++li) wc[m][li] = wn[m][li];
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int t = 0; t < NSUB; ++t) xn[e][t] = xn2[e][t];
        load_x(kb + 2, xn2);         // past the end: clamped channel, masked to zero, never used
        load_w(kb + 1, wn);
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int t = 0; t < NSUB; ++t) mac6(wc[m], xl[t], acc[m][t], alo[m][t]);
    }
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int t = 0; t < NSUB; ++t) acc[m][t] += alo[m][t];
    float4 bq[MTW][4];                  // after the k loop: 16 more live registers per M-tile inside it would spill
    x6_load_bias<MTW>(k, b, mt0, kh, bq);
    x6_epilogue<MTW, NSUB, VEC>(k, b, mt0, p, keep, kh, s_bias, bq, acc);
}

// ------------------------------------------------------------------------------------------------
// small planes: L <= 128 (the 4x4 ... 8x8 maps of Stage I), any K, optional LayerNorm.  grid (1, MT, B): one M-tile per workgroup.
// In the forms above a plane this small leaves one wave of four with pixels, and that wave walks K with one k-block of weights in flight:
// the time follows the k-block count at one memory latency each (~1.1 us), whatever the flops.  Here the plane's PW = 4 / KS pixel-waves
// each share their k-blocks among KS waves: wave w has pixel group w / KS and k-slice w % KS, slice s covers k-blocks
// [s q, min(KB, (s + 1) q)), q = ceil(KB / KS) (a slice may be empty and then adds zeros), and a wave requests its slice BEM_X6_SMALL_D
// k-blocks at a time, weights and x together, before the first MFMA of the chunk: one exposed latency per chunk instead of one per k-block
// (K <= 192 at KS = 4: one in all).  Each wave sums its own hi + lo; slices 1 .. KS - 1 park their accumulators in LDS, one barrier, slice 0
// adds them in the fixed order 1, 2, 3 (bit-reproducible from launch to launch) and runs the common epilogue.  No wave leaves before the
// last barrier.  LayerNorm (32-pixel waves and q <= BEM_X6_SMALL_D only, so that a slice is one chunk held in registers): the slices' partial
// sums, then partial centred squares, meet in LDS (two more barriers, summed in slice order by every wave alike).
// ------------------------------------------------------------------------------------------------
// k-blocks per chunk: with the accumulators of one M-tile this stays inside the 256 registers of two workgroups per CU
constexpr int BEM_X6_SMALL_D = 3;
template <int KS, int NSUB, bool SUM, bool VEC, bool LN>
__global__ __launch_bounds__(256, 2) void pw_x6_small_kernel(PwX k) {
    constexpr int PW = 4 / KS, D = BEM_X6_SMALL_D, MAXK = 16 * 4 * D;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kh = lane >> 5, n = lane & 31;
    const int pg = wave / KS, ks = wave % KS;
    const int b = blockIdx.z, mt0 = blockIdx.y;
    __shared__ __attribute__((aligned(16))) float s_bias[BEM_X6_MAXM];
    __shared__ float s_ln[LN ? 2 * MAXK : 2];
    __shared__ float s_stat[LN ? 2 * 4 * NSUB * 64 : 2];
    __shared__ float s_part[PW * (KS - 1) * NSUB * 16 * 64];
    stage_bias(k, b, s_bias);
    if (LN) {
        for (int i = threadIdx.x; i < k.KB * 16; i += 256) {     // zero scale / shift on the padded channels
            s_ln[i] = i < k.K ? k.ln_w[i] : 0.f;
            s_ln[MAXK + i] = i < k.K ? k.ln_b[i] : 0.f;
        }
    }
    __syncthreads();
    const int p = pg * (32 * NSUB) + NSUB * n;
    bool keep[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) keep[t] = p + t < k.L;
    const int pc = VEC ? (keep[0] ? p : 0) : p;
    const int q = (k.KB + KS - 1) / KS, kb0 = ks * q, kb1 = min(k.KB, kb0 + q);
    const u32x4* wbase = k.Wp + (int64_t)b * k.w_bstride + (int64_t)mt0 * k.KB * 3 * 64 + lane;
    f32x16 acc[1][NSUB], alo[NSUB];
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[0][t] = alo[t] = zero16();
    int kc = kb0;
#pragma nounroll
    do {                                // once even for an empty slice: clamped loads, nothing accumulated, every barrier reached
        u32x4 wv[D][3];
        float xv[D][8][NSUB];
#pragma unroll
        for (int d = 0; d < D; ++d) {   // k-blocks past the slice re-read a valid block: weights masked to zero, x not used
            load_w3_masked(wbase + (int64_t)min(kc + d, k.KB - 1) * 3 * 64, kc + d < kb1 ? 0xffffffffu : 0u, wv[d]);
#pragma unroll
            for (int e = 0; e < 8; ++e) ldx<NSUB, SUM, VEC>(k, b, 16 * (kc + d) + 8 * kh + e, pc, keep, xv[d][e]);   // channels >= K come back as zeros
        }
        float mean[NSUB], rstd[NSUB];
        if (LN) {
            const float inv = 1.f / (float)k.K;
            float* st = s_stat + lane;
#pragma unroll
            for (int t = 0; t < NSUB; ++t) {
                float sm = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d)
                    if (kc + d < kb1) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) sm += xv[d][e][t];
                    }
                sm += __shfl_xor(sm, 32, 64);
                st[((pg * KS + ks) * NSUB + t) * 64] = sm;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < NSUB; ++t) {
                float sm = 0.f;
#pragma unroll
                for (int j = 0; j < KS; ++j) sm += valu_copy(st[((pg * KS + j) * NSUB + t) * 64]);
                mean[t] = sm * inv;
                float sq = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d)
                    if (kc + d < kb1) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float dv = (16 * (kc + d) + 8 * kh + e < k.K) ? xv[d][e][t] - mean[t] : 0.f;     // padded channels do not count
                            sq = fmaf(dv, dv, sq);
                        }
                    }
                sq += __shfl_xor(sq, 32, 64);
                st[(4 * NSUB + (pg * KS + ks) * NSUB + t) * 64] = sq;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < NSUB; ++t) {
                float sq = 0.f;
#pragma unroll
                for (int j = 0; j < KS; ++j) sq += valu_copy(st[(4 * NSUB + (pg * KS + j) * NSUB + t) * 64]);
                rstd[t] = 1.f / sqrtf(sq * inv + k.ln_eps);
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (kc + d < kb1) {
                u32x4 xl[NSUB][3];
#pragma unroll
                for (int t = 0; t < NSUB; ++t) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        v[e] = xv[d][e][t];
                        const int ch = min(16 * (kc + d) + 8 * kh + e, MAXK - 1);
                        if (LN) v[e] = (v[e] - mean[t]) * rstd[t] * valu_copy(s_ln[ch]) + valu_copy(s_ln[MAXK + ch]);
                    }
                    split8(v, xl[t][0], xl[t][1], xl[t][2]);
                }
#pragma unroll
                for (int t = 0; t < NSUB; ++t) mac6(wv[d], xl[t], acc[0][t], alo[t]);
            }
        }
        kc += D;
    } while (kc < kb1);
#pragma unroll
    for (int t = 0; t < NSUB; ++t) acc[0][t] += alo[t];
    float4 bq[1][4];
    x6_load_bias<1>(k, b, mt0, kh, bq);
    float* sp = s_part + (int64_t)(pg * (KS - 1) * NSUB) * 1024 + lane;
    if (ks != 0) {
#pragma unroll
        for (int t = 0; t < NSUB; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) sp[(((ks - 1) * NSUB + t) * 16 + r) * 64] = acc[0][t][r];
    }
    __syncthreads();
    if (ks != 0) return;
#pragma unroll
    for (int j = 1; j < KS; ++j)        // fixed order 1, 2, 3
#pragma unroll
        for (int t = 0; t < NSUB; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][t][r] += valu_copy(sp[(((j - 1) * NSUB + t) * 16 + r) * 64]);
    x6_epilogue<1, NSUB, VEC>(k, b, mt0, p, keep, kh, s_bias, bq, acc);
}

template <int KS, int NSUB>
void launch_small(const PwX& k, dim3 grid, hipStream_t s, bool sum, bool vec, bool ln) {
#define BEM_X6_SMALL(SUM, VEC)                                                              \
    do {                                                                                    \
        if constexpr (NSUB == 1) {                                                          \
            if (ln) { pw_x6_small_kernel<KS, NSUB, SUM, VEC, true><<<grid, 256, 0, s>>>(k); break; }   \
        }                                                                                   \
        pw_x6_small_kernel<KS, NSUB, SUM, VEC, false><<<grid, 256, 0, s>>>(k);              \
    } while (0)
    if (NSUB == 2 && vec && !sum) BEM_X6_SMALL(false, NSUB == 2);       // 32-pixel waves: the scalar-pixel forms, as in BEM_X6_RES(10, 1, *)
    else if (NSUB == 2 && vec) BEM_X6_SMALL(true, NSUB == 2);
    else if (!sum) BEM_X6_SMALL(false, false);
    else BEM_X6_SMALL(true, false);
#undef BEM_X6_SMALL
}

}  // namespace

extern "C" int bem_pw_gemm_x6_f32(const bem_pw_args* a, void* stream) {
    BEM_REQUIRE(a, "pw_gemm_x6: null args");
    BEM_REQUIRE(a->x1 && a->Wp && a->out, "pw_gemm_x6: null tensor");
    BEM_REQUIRE(a->B >= 0 && a->B <= 65535 && a->M > 0 && a->M <= BEM_X6_MAXM && a->K > 0 && a->L >= 0, "pw_gemm_x6: bad shape B=%d M=%d K=%d L=%d", a->B, a->M, a->K, a->L);
    BEM_REQUIRE(a->in_mode >= 0 && a->in_mode <= 2, "pw_gemm_x6: in_mode %d", a->in_mode);
    if (a->in_mode == 0) BEM_REQUIRE(a->K == a->C1, "pw_gemm_x6: K %d != C1 %d", a->K, a->C1);
    if (a->in_mode == 1) BEM_REQUIRE(a->x2 && a->K == a->C1 && a->C1 == a->C2, "pw_gemm_x6: sum mode needs x2 and K == C1 == C2");
    if (a->in_mode == 2) BEM_REQUIRE(a->x2 && a->K == a->C1 + a->C2, "pw_gemm_x6: cat mode needs x2 and K == C1 + C2");
    BEM_REQUIRE((a->ln_w == nullptr) == (a->ln_b == nullptr), "pw_gemm_x6: ln_w / ln_b must both be set or both NULL");
    BEM_REQUIRE(a->act == 0 || (a->act == 1 && a->prelu), "pw_gemm_x6: act %d", a->act);
    BEM_REQUIRE(a->out_mode == 0 || (a->out_mode == 1 && a->M % 4 == 0 && a->Win > 0 && a->L % a->Win == 0 && !a->res),
                "pw_gemm_x6: out_mode %d constraints", a->out_mode);
    BEM_REQUIRE(((uintptr_t)a->Wp & 15) == 0 && a->w_bstride % 4 == 0, "pw_gemm_x6: packed weights must be 16-byte aligned");
    // Plane bases (batch row, channel, output row) are 64-bit and wave-uniform; a lane adds its pixel and, in the row epilogue, its 4-row
    // half: (4 kh L + p) elements as a uint32, 20 L bytes at most.  That offset, not M L, is what has to fit into 32 bits.
    BEM_REQUIRE((int64_t)20 * a->L < (1ll << 32), "pw_gemm_x6: a plane of L = %d pixels exceeds the 32-bit lane offsets of the epilogue (20 L bytes)", a->L);
    const bool ln = a->ln_w != nullptr;
    BEM_REQUIRE(!ln || a->K <= BEM_X6_MAXK_LN, "pw_gemm_x6: LayerNorm prologue supports K <= %d (got %d)", BEM_X6_MAXK_LN, a->K);
    if (a->B == 0 || a->L == 0) return BEM_OK;
    PwX k;
    k.x1 = a->x1; k.x2 = a->x2 ? a->x2 : a->x1; k.C1 = a->C1; k.C2 = a->x2 ? a->C2 : a->C1; k.in_mode = a->in_mode;
    k.ln_w = a->ln_w; k.ln_b = a->ln_b; k.ln_eps = a->ln_eps;
    k.Wp = reinterpret_cast<const u32x4*>(a->Wp); k.w_bstride = a->w_bstride / 4; k.bias = a->bias; k.bias_bstride = a->bias_bstride;
    k.res = a->res; k.prelu = a->prelu; k.act = a->act; k.out = a->out; k.out_mode = a->out_mode; k.Win = a->Win;
    k.M = a->M; k.K = a->K; k.L = a->L; k.KB = cdiv(a->K, 16); k.MT = cdiv(a->M, 32); k.mtpb = k.MT;
    hipStream_t s = (hipStream_t)stream;
    const bool sum = a->in_mode == 1;
    const bool al = (((uintptr_t)a->x1 | (uintptr_t)(a->x2 ? a->x2 : a->x1) | (uintptr_t)a->out | (uintptr_t)(a->res ? a->res : a->out)) & 7) == 0;
    const bool vec = a->L % 2 == 0 && al;
#define BEM_X6_RES(KBM, NSUB, MTW)                                                                       \
    do {                                                                                                 \
        dim3 grid(cdiv(a->L, 128 * NSUB), 1, a->B);                                                      \
        /* few pixels (Stage I's 16x16 maps; 8x8 with LayerNorm, 4x4 and 8x8 at K <= 48: the rest of the 4x4 and 8x8 maps    \
           takes pw_x6_small_kernel), many output rows: slice M over grid.y so that the weight stream of one sample is     \
           pulled by several workgroups (each repeats the cheap LayerNorm of the same pixels) */                           \
        const int64_t wv = (int64_t)a->B * cdiv(a->L, 32 * NSUB);                                        \
        const int groups = cdiv(k.MT, MTW);                                                              \
        const int ny = wv >= 2048 ? 1 : (int)std::min<int64_t>(groups, cdiv64(2048, wv));                \
        k.mtpb = cdiv(groups, ny) * MTW;                                                                 \
        grid.y = cdiv(k.MT, k.mtpb);                                                                     \
        if (NSUB == 2 && vec && !sum) pw_x6_res_kernel<KBM, NSUB, MTW, false, true><<<grid, 256, 0, s>>>(k);   \
        else if (NSUB == 2 && vec) pw_x6_res_kernel<KBM, NSUB, MTW, true, true><<<grid, 256, 0, s>>>(k);       \
        else if (!sum) pw_x6_res_kernel<KBM, NSUB, MTW, false, false><<<grid, 256, 0, s>>>(k);                 \
        else pw_x6_res_kernel<KBM, NSUB, MTW, true, false><<<grid, 256, 0, s>>>(k);                            \
        return bem_check_launch("pw_x6_res");                                                            \
    } while (0)
    // small planes (grid.x would be 1 below and the plane fills at most two pixel-waves): K split over the waves of the workgroup
    // (pw_x6_small_kernel), 4-way for L <= 64, 2-way for L <= 128, 32-pixel waves for L <= 32.  Kept on the forms below, measured with
    // scripts/small_plane_micro.py (B = 64, per-sample weights; parent -> small form):
    //   * K <= 48 (KB <= 3): the one working wave of the resident form already has every k-block in flight at once;
    //   * LayerNorm on 64-pixel waves: level-1 project_in (K 80 -> M 640, 8x8) 27.8 -> 33.1 us -- 20 workgroups per sample that each repeat
    //     the statistics behind two more barriers at 240 registers; in_proj / out_proj there (3 M-tiles) 13.1 -> 12.8 / 14.4 -> 13.7 us, inside
    //     the launch floor of the measurement.  With 32-pixel waves (4x4: K 160 -> 1280 48.7 -> 36.6 us, out_proj 22.8 -> 13.8 us) it is taken
    //     where a wave's slice is one chunk (K <= 192).
    // Without LayerNorm: level-2 project_out (K 640) 52.1 -> 21.5 us, level-1 (K 320) 26.7 -> 13.4 us, the 4x4 up-sampling GEMM 25.3 -> 13.6 us.
    if (a->L <= 128 && k.KB > 3) {
        const int ks = a->L <= 64 ? 4 : 2;
        if (!ln || (a->L <= 32 && cdiv(k.KB, ks) <= BEM_X6_SMALL_D)) {
            const dim3 grid(1, k.MT, a->B);
            if (a->L <= 32) launch_small<4, 1>(k, grid, s, sum, vec, ln);
            else if (ks == 4) launch_small<4, 2>(k, grid, s, sum, vec, ln);
            else launch_small<2, 2>(k, grid, s, sum, vec, ln);
            return bem_check_launch("pw_x6_small");
        }
    }
    // one M-tile at a time where a wave holds two sub-tiles: the accumulator pairs double the register cost of an M-tile
    if (k.KB <= 3) BEM_X6_RES(3, 2, 1);
    if (ln && k.KB <= 5) BEM_X6_RES(5, 2, 1);
    if (ln && k.KB == 10 && k.K == 160 && k.MT >= 8 && (int64_t)a->B * cdiv(a->L, 32) >= 2048) {
        // many M-tiles over a full-width K and enough pixels that a workgroup walks all of them: an M-tile's weights go through LDS once per
        // workgroup (pw_x6_res_lds_kernel; level-2 project_in 335 -> 188 us).  With few pixels (Stage I) M is sliced over grid.y and the
        // per-wave streaming form below is the faster one (50 vs 63 us).
        dim3 grid(cdiv(a->L, 128), 1, a->B);
        k.mtpb = k.MT;
        if (!sum) pw_x6_res_lds_kernel<10, false, false><<<grid, 256, 0, s>>>(k);       // 32 pixels per wave: the scalar-pixel forms, as in BEM_X6_RES(10, 1, *)
        else pw_x6_res_lds_kernel<10, true, false><<<grid, 256, 0, s>>>(k);
        return bem_check_launch("pw_x6_res_lds");
    }
    if (ln && k.KB <= 10) { if (k.MT == 1) BEM_X6_RES(10, 1, 1); else BEM_X6_RES(10, 1, 2); }
#undef BEM_X6_RES
    {
        // two M-tiles per pass over x with 64-pixel waves; every further grid.y slice re-reads the input from L2 (three M-tiles per pass
        // with 32-pixel waves measured 227 us against 219 us for this form at K = 320, M = 80, 64x64)
        const int mtw = k.MT == 1 ? 1 : 2;
        dim3 grid(cdiv(a->L, 256), cdiv(k.MT, mtw), a->B);
#define BEM_X6_STREAM(MTW, LN)                                                                \
    do {                                                                                      \
        if (vec && !sum) pw_x6_stream_kernel<MTW, 2, false, true, LN><<<grid, 256, 0, s>>>(k);   \
        else if (vec) pw_x6_stream_kernel<MTW, 2, true, true, LN><<<grid, 256, 0, s>>>(k);       \
        else if (!sum) pw_x6_stream_kernel<MTW, 2, false, false, LN><<<grid, 256, 0, s>>>(k);    \
        else pw_x6_stream_kernel<MTW, 2, true, false, LN><<<grid, 256, 0, s>>>(k);               \
    } while (0)
        if (ln) { if (mtw == 1) BEM_X6_STREAM(1, true); else BEM_X6_STREAM(2, true); }
        else { if (mtw == 1) BEM_X6_STREAM(1, false); else BEM_X6_STREAM(2, false); }
#undef BEM_X6_STREAM
    }
    return bem_check_launch("pw_x6_stream");
}
