// Dense convolutions on the bf16-limb (x6) matrix cores, the forms BEM_CONV_ROWS and BEM_CONV_TAPS of bem_conv2d_f32 (which shape takes
// which: bem_conv2d_route, conv.hip): the row form (conv_rows_x6_kernel, below) and shifted 1x1 taps (conv_taps_x6_kernel, second half).
// Limb arithmetic and operand layout: x6_common.h and the header of pw_gemm_x6.hip.
//
// Row form: the 4x4 stride-2 pad-1 down-sampling convs of
// the U-Nets (DecompDualBranchDDWavelet_arch.py:40-41) and the 3x3 stride-1 pad-1 convs of the decomposition nets and the first / last layers
// (basicsr/QD/model4.py:181-200, DecompDualBranchDDWavelet_arch.py:190), written for what bounds them:
//     out[co][yo][xo] = act(bias[co] + sum_{ci, ky, kx} W[co][ci][ky][kx] x[ci][S yo - 1 + ky][S xo - 1 + kx]) + res1 + res2
//   * a lane owns NPX = 4 / S neighbouring output pixels of a row: for one input row they need six input columns, 4 S m' - 1 .. + 4.
//     Four of them are ONE aligned 16-byte load per channel (a half-wave reads 512 contiguous bytes of a plane row); the two outer ones are
//     the neighbour lanes' values, moved by DPP wave shifts and zeroed at the row ends, which is exactly the zero padding.  The shifted-tap
//     form this replaces (conv_taps_x6_kernel) issues KS x KS x 16 scalar loads per k-block where this one issues KS x 8 vector loads.
//   * the six columns are split into bf16 limbs once (x6_common.h) and serve all kx taps of all NPX pixels: 6 splits for 8 (4x4) / 12 (3x3)
//     tap uses.
//   * tap weights are KS^2 x the bytes of a 1x1 layer; fetched per wave from L2 they would need ~20 TB/s.  A workgroup stages the
//     3 KS MTW 1-KiB operand blocks of a step (k-block, input row) in LDS by LDS-DMA, double-buffered, requested one step ahead.
//   * the input rows of the next step are requested (into registers) before the matrix work of the current one.
// One workgroup = 4 waves = 128 NPX consecutive output pixels x MTW row blocks of 32 output channels; two workgroups per CU.
// Shapes (conv_rows_shape): Wo / NPX (the lanes of an output row) a power of two <= 32, so that no row crosses a half-wave; Cin % 8 == 0.
// Wp = bem_pack_pw_weight_x6 of the (KS^2, Cout, Cin) tap matrices, tap = KS ky + kx.
#include "bem_common.h"
#include "conv_launch.h"
#include "scan_common.h"
#include "x6_common.h"

namespace {

struct CrX {
    const float* x; int64_t x_bs;
    const u32x4* Wp; const float* bias; const float* res1; const float* res2; float* out;
    int Cin, H, W, Ho, Wo, Cout, KB, MT, wo_shift, relu, mt_first, res1_rep;
};

typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int MTW, int KS, int S>
__global__ __launch_bounds__(256, 2) void conv_rows_x6_kernel(CrX k) {
    constexpr int NPX = 4 / S;                                                         // output pixels of a lane
    constexpr int NP = 3 * KS * MTW;                                                   // 1 KiB pieces of a step: [kx][m][limb]
    __shared__ __attribute__((aligned(16))) u32x4 Ws[2][NP * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z, mt0 = k.mt_first + blockIdx.y * MTW;
    const int Lo = k.Ho * k.Wo, Li = k.H * k.W;
    const int p0 = (xcd_tile(blockIdx.x, gridDim.x) * 4 + wave) * (32 * NPX);
    const int p = p0 + NPX * n;
    const bool live = p < Lo;
    const int pc = live ? p : 0;
    const int yo = pc >> k.wo_shift, xo = pc & (k.Wo - 1);
    const float lmask = xo == 0 ? 0.f : 1.f, rmask = xo == k.Wo - NPX ? 0.f : 1.f;      // the row's first / last lane: padding columns
    const float* xb = k.x + (int64_t)b * k.x_bs;
    const uint32_t voff = 16 * lane, ws_lds = lds_addr(Ws);
    const int NS = KS * k.KB;                                                          // step s = KS kb + r (input row S yo - 1 + r)

    auto dma_w = [&](int s, int buf) {
        const int kb = s / KS, r = s - kb * KS;
#pragma unroll
        for (int t = 0; t < (NP + 3) / 4; ++t) {
            const int pi = wave + 4 * t, kx = pi / (3 * MTW), m = (pi / 3) % MTW, li = pi % 3;
            if (pi < NP)
                glds16(k.Wp + ((((int64_t)(KS * r + kx) * k.MT + (mt0 + m)) * k.KB + kb) * 3 + li) * 64, voff, ws_lds + (buf * NP + pi) * 1024);
        }
    };
    // the 8 channels (16 kb + 8 kh + e) of this lane at input row S yo - 1 + r, own columns S xo .. S xo + 3; rows outside the image: clamped
    // address, zero mask.  Past Cin (a half-filled last k-block) a valid channel is re-read: the packed weights there are zero.
    auto load_x = [&](int s, f32x4v (&dst)[8], float& mk) {
        const int kb = min(s / KS, k.KB - 1), r = s - (s / KS) * KS;
        const int yi = S * yo - 1 + r;
        mk = (live && yi >= 0 && yi < k.H) ? 1.f : 0.f;
        const int off = min(max(yi, 0), k.H - 1) * k.W + S * xo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = min(16 * kb + 8 * kh + e, k.Cin - 1);
            dst[e] = *reinterpret_cast<const f32x4v*>(xb + (int64_t)ch * Li + off);
        }
    };

    f32x16 acc[MTW][NPX], alo[MTW][NPX];
#pragma unroll
for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int t = 0; t < NPX; ++t) acc[m][t] = alo[m][t] = zero16();

    dma_w(0, 0);
    f32x4v xn[8];
    float mkn;
    load_x(0, xn, mkn);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) dma_w(s + 1, (s + 1) & 1);
        // columns S xo - 1 .. S xo + 4 of the 8 channels: the lane's own four, the left neighbour's last and the right neighbour's first
        float col[6][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const f32x4v v = xn[e] * mkn;
            col[1][e] = v[0]; col[2][e] = v[1]; col[3][e] = v[2]; col[4][e] = v[3];
            col[0][e] = dpp_mov<0x138, 0xf>(0.f, v[3]) * lmask;                        // wave_shr 1: lane n takes lane n - 1
            col[5][e] = dpp_mov<0x130, 0xf>(0.f, v[0]) * rmask;                        // wave_shl 1: lane n takes lane n + 1
        }
        load_x(s + 1, xn, mkn);                                                        // past the end: clamped, never used
        u32x4 xl[6][3];
#pragma unroll
        for (int c = 0; c < 6; ++c) split8(col[c], xl[c][0], xl[c][1], xl[c][2]);
        const u32x4* Wc = Ws[s & 1] + lane;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx)
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                const u32x4* wp = Wc + (kx * MTW + m) * 192;
                const u32x4 wl[3] = {wp[0], wp[64], wp[128]};
#pragma unroll
                for (int j = 0; j < NPX; ++j) mac6(wl, xl[S * j + kx], acc[m][j], alo[m][j]);     // pixel j: column S (xo + j) - 1 + kx
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // epilogue: out = relu?(acc + bias) + res1 + res2, rows acc_row(r, kh) of each row block, one 4 NPX-byte access per row.
    // res1 is read at batch row b / res1_rep (one residual row shared by res1_rep output rows): a wave-uniform base, no lane arithmetic
    if (live) {
        typedef float fpx __attribute__((ext_vector_type(NPX)));
        const float lo = k.relu ? 0.f : -3.402823466e38f;
        const int64_t ob = (int64_t)b * k.Cout * Lo + pc;
        const float* r1b = k.res1 + (int64_t)(b / k.res1_rep) * k.Cout * Lo + pc;
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = acc_row(r, kh, (mt0 + m) * 32);
                if (row < k.Cout) {
                    const float bv = k.bias ? k.bias[row] : 0.f;
                    const int64_t o = ob + (int64_t)row * Lo;
                    fpx v;
#pragma unroll
                    for (int j = 0; j < NPX; ++j) v[j] = fmaxf(acc[m][j][r] + alo[m][j][r] + bv, lo);
                    if (k.res1) v += *reinterpret_cast<const fpx*>(r1b + (int64_t)row * Lo);
                    if (k.res2) v += *reinterpret_cast<const fpx*>(k.res2 + o);
                    *reinterpret_cast<fpx*>(k.out + o) = v;
                }
            }
    }
}

}  // namespace

bool conv_rows_shape(int KS, int Cin, int H, int W) {
    const int S = KS == 4 ? 2 : 1, Wo = W / S, lanes = Wo * S / 4;                     // lanes of an output row
    return Cin > 0 && Cin % 8 == 0 && H > 0 && H % S == 0 && W % S == 0 && lanes >= 1 && lanes <= 32 && (Wo & (Wo - 1)) == 0;
}
bool conv_rows_aligned(const float* x, int64_t x_bstride, const float* out, const float* res1, const float* res2) {
    return (((uintptr_t)x | (uintptr_t)out | (uintptr_t)res1 | (uintptr_t)res2) & 15) == 0 && x_bstride % 4 == 0;
}

// KS = 4: the 4x4 stride-2 form; KS = 3: 3x3 stride 1.  Row blocks of output channels in pairs where the registers allow (4x4), singly else.
int conv_rows_launch(int KS, const float* x, int64_t x_bstride, const float* Wp, const float* bias, const float* res1, const float* res2, float* out,
                     int B, int Cin, int H, int W, int Cout, int relu, int res1_rep, void* stream) {
    const char* what = KS == 4 ? "conv4x4s2_x6" : "conv3x3_x6";
    BEM_REQUIRE(x && Wp && out, "%s: null tensor", what);
    BEM_REQUIRE(res1_rep >= 1, "%s: res1_rep %d", what, res1_rep);
    BEM_REQUIRE(B >= 0 && B <= 65535 && Cout > 0 && (KS == 3 || KS == 4) && conv_rows_shape(KS, Cin, H, W), "%s: shape outside the row form", what);
    BEM_REQUIRE(((uintptr_t)Wp & 15) == 0 && conv_rows_aligned(x, x_bstride, out, res1, res2), "%s: alignment (x, packed weights, out and residuals 16 bytes)", what);
    const int S = KS == 4 ? 2 : 1, Ho = H / S, Wo = W / S;
    BEM_REQUIRE((int64_t)Cout * Ho * Wo < (1ll << 30) && (int64_t)Cin * H * W < (1ll << 30), "%s: plane set too large for 32-bit lane offsets", what);
    if (B == 0) return BEM_OK;
    CrX k;
    k.x = x; k.x_bs = x_bstride; k.Wp = reinterpret_cast<const u32x4*>(Wp); k.bias = bias; k.res1 = res1; k.res2 = res2; k.out = out;
    k.Cin = Cin; k.H = H; k.W = W; k.Ho = Ho; k.Wo = Wo; k.Cout = Cout; k.KB = cdiv(Cin, 16); k.MT = cdiv(Cout, 32); k.relu = relu; k.res1_rep = res1_rep;
    k.wo_shift = __builtin_ctz(Wo);
    hipStream_t s = (hipStream_t)stream;
    if (KS == 4) {
        const int pairs = k.MT / 2, nx = cdiv(Ho * Wo, 256);
        if (pairs) {
            k.mt_first = 0;
            conv_rows_x6_kernel<2, 4, 2><<<dim3(nx, pairs, B), 256, 0, s>>>(k);
        }
        if (k.MT & 1) {
            k.mt_first = 2 * pairs;
            conv_rows_x6_kernel<1, 4, 2><<<dim3(nx, 1, B), 256, 0, s>>>(k);
        }
    } else {
        k.mt_first = 0;
        conv_rows_x6_kernel<1, 3, 1><<<dim3(cdiv(Ho * Wo, 512), k.MT, B), 256, 0, s>>>(k);
    }
    return bem_check_launch(what);
}

// ================================================================================================
// Dense convolutions as shifted 1x1 GEMM taps on the same x6 machinery (3x3 stride 1 pad 1, dilated or strided; 5x5 stride 1 pad 2):
//     out[co][p] = relu?( sum_{tap} sum_ci W[co][ci][tap] * x[ci][S*p + tap offset] + bias[co] ) + res1 + res2
// No im2col patch: tap (ky, kx) reads the input pixels of the wave's 64 output pixels straight from global memory (the
// displaced reads of a k-block overlap and are served by L1 / L2), masks the pixels that fall outside the image, splits
// them into bf16 limbs and issues the six limb products against that tap's weight block.  The x loads of the next tap
// are requested before the MFMAs of the current one.  Wp: (KH*KW taps, MT, KB, 3 limbs, 64 lanes) 16-byte vectors =
// bem_pack_pw_weight_x6 of the (KH*KW, Cout, Cin) tap matrices.  Requires an even output width and Cin % 8 == 0.
// ================================================================================================
namespace {

struct CvX {
    const float* x; int64_t x_bs;
    const u32x4* Wp; const float* bias; const float* res1; const float* res2; float* out;
    int Cin, H, W, Ho, Wo, Cout, KB, MT, relu, pad, dil, res1_rep;
};

template <int MTW, int KH, int KW, int S>
__global__ __launch_bounds__(256, 2) void conv_taps_x6_kernel(CvX k) {
    constexpr int NSUB = 2, NTAP = KH * KW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z, mt0 = blockIdx.y * MTW;
    const int Lo = k.Ho * k.Wo, Li = k.H * k.W;
    const int p0 = (xcd_tile(blockIdx.x, gridDim.x) * 4 + wave) * 64;
    if (p0 >= Lo) return;
    const int p = p0 + 2 * n;                       // this lane's two output pixels p, p + 1 (same row: Wo is even)
    const bool live = p < Lo;
    const int pc = live ? p : 0;
    const int yo = pc / k.Wo, xo = pc - yo * k.Wo;
    const int yi0 = yo * S - k.pad, xi0 = xo * S - k.pad;      // input position of tap (0, 0) for the first pixel
    const float* xb = k.x + (int64_t)b * k.x_bs;
    f32x16 acc[MTW][NSUB], alo[MTW][NSUB];
#pragma unroll
for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int t = 0; t < NSUB; ++t) acc[m][t] = alo[m][t] = zero16();
    const u32x4* wbase = k.Wp + lane;
    const int64_t tap_stride = (int64_t)k.MT * k.KB * 3 * 64, mt_stride = (int64_t)k.KB * 3 * 64;
    const int nsteps = k.KB * NTAP;
    // step s = kb * NTAP + tap.  Loads of a step: 8 channels (16 kb + 8 kh + e) at the two input pixels of this tap.
    auto load_x = [&](int s, float (&dst)[8][NSUB], float (&mk)[NSUB]) {
        const int kb = min(s / NTAP, k.KB - 1), tap = s - (s / NTAP) * NTAP;
        const int ky = tap / KW, kx = tap - ky * KW;
        const int yy = yi0 + ky * k.dil, x0 = xi0 + kx * k.dil, x1 = x0 + S;
        const bool rowok = live && yy >= 0 && yy < k.H;
        mk[0] = (rowok && x0 >= 0 && x0 < k.W) ? 1.f : 0.f;
        mk[1] = (rowok && x1 >= 0 && x1 < k.W) ? 1.f : 0.f;
        const int q = yy * k.W + x0;
        // the upper half-wave reads channels + 8; past Cin (a half-filled last k-block) it re-reads the lower half,
        // whose weights there are zero
        const int c0 = 16 * kb, hoff = (c0 + 8 < k.Cin) ? 8 * kh : 0;
        if (S == 1) {
            // the pair (q, q + 1) as ONE 8-byte load (global loads need dword alignment only) at a base clamped into the
            // plane; d = q - base is 0 except at the two ends of the plane, where one of the two pixels is outside anyway
            const int qb = min(max(q, 0), Li - 2), d = q - qb;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* pl = xb + (int64_t)(min(c0 + e, k.Cin - 1 - hoff) + hoff) * Li;
                float2 v;
                __builtin_memcpy(&v, pl + qb, sizeof(v));
                dst[e][0] = d > 0 ? v.y : v.x;
                dst[e][1] = d < 0 ? v.x : v.y;
            }
        } else {
            const int q0 = min(max(q, 0), Li - 1), q1 = min(max(q + S, 0), Li - 1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* pl = xb + (int64_t)(min(c0 + e, k.Cin - 1 - hoff) + hoff) * Li;
                dst[e][0] = pl[q0];
                dst[e][1] = pl[q1];
            }
        }
    };
    auto load_w = [&](int s, u32x4 (&dst)[MTW][3]) {
        const int sc = min(s, nsteps - 1), kb = sc / NTAP, tap = sc - kb * NTAP;
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const bool ok = s < nsteps && mt0 + m < k.MT;
            const u32x4* wp = wbase + tap * tap_stride + (int64_t)(mt0 + m < k.MT ? mt0 + m : 0) * mt_stride + (int64_t)kb * 3 * 64;
            load_w3_masked(wp, ok ? 0xffffffffu : 0u, dst[m]);
        }
    };
    float xn[8][NSUB], mkn[NSUB];
    u32x4 wn[MTW][3];
    load_x(0, xn, mkn);
    load_w(0, wn);
    for (int s = 0; s < nsteps; ++s) {
        u32x4 xl[NSUB][3], wc[MTW][3];
#pragma unroll
        for (int t = 0; t < NSUB; ++t) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = xn[e][t] * mkn[t];
            split8(v, xl[t][0], xl[t][1], xl[t][2]);
        }
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int li = 0; li < 3; ++li) wc[m][li] = wn[m][li];
        load_x(s + 1, xn, mkn);          // past the end: clamped, never used
        load_w(s + 1, wn);
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int t = 0; t < NSUB; ++t) mac6(wc[m], xl[t], acc[m][t], alo[m][t]);
    }
    // epilogue: out = relu?(acc + bias) + res1 + res2, plane bases uniform, one lane offset
    const float lo = k.relu ? 0.f : -3.402823466e38f;
    const uint32_t loff = (uint32_t)(4 * kh) * (uint32_t)Lo + (uint32_t)pc;
    float* outb = k.out + (int64_t)b * k.Cout * Lo;
    const float* r1b = k.res1 ? k.res1 + (int64_t)(b / k.res1_rep) * k.Cout * Lo : nullptr;      // one residual row per res1_rep output rows
    const float* r2b = k.res2 ? k.res2 + (int64_t)b * k.Cout * Lo : nullptr;
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        if (mt0 + m >= k.MT) continue;
        const int rb = (mt0 + m) * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float bv[4], rv[4][NSUB];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int urow = rb + 8 * g + i;
                const int lrow = min(urow + 4 * kh, k.Cout - 1);
                bv[i] = k.bias ? k.bias[lrow] : 0.f;
                rv[i][0] = rv[i][1] = 0.f;
                const uint32_t ro = (uint32_t)lrow * (uint32_t)Lo + (uint32_t)pc;
                if (r1b) { const float2 q = *reinterpret_cast<const float2*>(r1b + ro); rv[i][0] += q.x; rv[i][1] += q.y; }
                if (r2b) { const float2 q = *reinterpret_cast<const float2*>(r2b + ro); rv[i][0] += q.x; rv[i][1] += q.y; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * g + i, urow = rb + 8 * g + i;
                const float o0 = fmaxf(acc[m][0][r] + alo[m][0][r] + bv[i], lo) + rv[i][0];
                const float o1 = fmaxf(acc[m][1][r] + alo[m][1][r] + bv[i], lo) + rv[i][1];
                if (live && urow + 4 * kh < k.Cout) *reinterpret_cast<float2*>(outb + (int64_t)urow * Lo + loff) = make_float2(o0, o1);
            }
        }
    }
}

}  // namespace

int conv_taps_launch(const float* x, int64_t x_bstride, const float* Wp, const float* bias, const float* res1, const float* res2, float* out,
                     int B, int Cin, int H, int W, int Cout, int KH, int stride, int pad, int dil, int relu, int res1_rep, void* stream) {
    const char* what = "conv_taps_x6";
    BEM_REQUIRE(x && Wp && out && res1_rep >= 1, "%s: null tensor or res1_rep < 1", what);
    BEM_REQUIRE(B >= 0 && B <= 65535 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: bad shape", what);
    // "same" padding of the (dilated) window; 1 for the strided 3x3
    BEM_REQUIRE(((KH == 3 && stride == 1 && (dil == 1 || dil == 2)) || (KH == 3 && stride == 2 && dil == 1) || (KH == 5 && stride == 1 && dil == 1)) && pad == dil * (KH - 1) / 2,
                "%s: supported forms are 3x3 s1 (dilation 1 / 2, padding = dilation), 3x3 s2 p1 and 5x5 s1 p2", what);
    const int Ho = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1, Wo = (W + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
    BEM_REQUIRE(Ho > 0 && Wo > 0 && Wo % 2 == 0 && Cin % 8 == 0 && H * W >= 2, "%s: needs an even output width and Cin %% 8 == 0 (got Wo=%d Cin=%d)", what, Wo, Cin);
    BEM_REQUIRE(((uintptr_t)Wp & 15) == 0 && (((uintptr_t)out | (uintptr_t)(res1 ? res1 : out) | (uintptr_t)(res2 ? res2 : out)) & 7) == 0,
                "%s: alignment (packed weights 16 bytes, out / residuals 8 bytes)", what);
    BEM_REQUIRE((int64_t)Cout * Ho * Wo < (1ll << 30) && (int64_t)Cin * H * W < (1ll << 30), "%s: plane set too large for 32-bit lane offsets", what);
    if (B == 0) return BEM_OK;
    CvX k;
    k.x = x; k.x_bs = x_bstride; k.Wp = reinterpret_cast<const u32x4*>(Wp); k.bias = bias; k.res1 = res1; k.res2 = res2; k.out = out;
    k.Cin = Cin; k.H = H; k.W = W; k.Ho = Ho; k.Wo = Wo; k.Cout = Cout; k.KB = cdiv(Cin, 16); k.MT = cdiv(Cout, 32); k.relu = relu; k.pad = pad; k.dil = dil; k.res1_rep = res1_rep;
    const int mtw = k.MT == 1 ? 1 : 2;
    dim3 grid(cdiv(Ho * Wo, 256), cdiv(k.MT, mtw), B);
    hipStream_t s = (hipStream_t)stream;
    if (KH == 5) {
        if (mtw == 1) conv_taps_x6_kernel<1, 5, 5, 1><<<grid, 256, 0, s>>>(k);
        else conv_taps_x6_kernel<2, 5, 5, 1><<<grid, 256, 0, s>>>(k);
    } else if (KH == 3 && stride == 1) {
        if (mtw == 1) conv_taps_x6_kernel<1, 3, 3, 1><<<grid, 256, 0, s>>>(k);
        else conv_taps_x6_kernel<2, 3, 3, 1><<<grid, 256, 0, s>>>(k);
    } else {
        if (mtw == 1) conv_taps_x6_kernel<1, 3, 3, 2><<<grid, 256, 0, s>>>(k);
        else conv_taps_x6_kernel<2, 3, 3, 2><<<grid, 256, 0, s>>>(k);
    }
    return bem_check_launch(what);
}
