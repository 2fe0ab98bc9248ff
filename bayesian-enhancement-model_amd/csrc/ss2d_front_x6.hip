// The front half of an SS2D branch in one kernel (vmamba.py:700-716 up to the scan, with the block's norm :1326):
//     xc = SiLU(dw3x3(W_in LayerNorm2d(x) + b_in) + b_dw)                (B, C, H, W)
//     xd = W_x xc                                                       (B, Mx, H W),  Mx = 4 (R + 2): the x_dbl rows of all four directions
// As separate kernels (LayerNorm + in_proj GEMM, depthwise conv + SiLU, x_proj GEMM) the C-channel tensor t = in_proj(LN(x)) is written and read
// once and xc is read a second time: 5.5 passes of C . P . 4 bytes where x in, xc out and the narrow xd out (2.5 passes) are what is needed.
//
// Mapping (one workgroup = 4 waves = one 4 x 32 pixel tile of one image; tile and LayerNorm prologue: x6_tile.h):
//   * the tile's 6 x 34 halo is 204 pixels = 7 MFMA pixel blocks of 32; wave w owns blocks w and w + 4, LayerNorm-ed and split into three
//     bf16 limbs in registers.
//   * phase A  t (C rows x 204 halo pixels) = W_in xn on the bf16 matrix cores (six exact limb products) + b_in, zero outside the image (the
//              depthwise conv zero-pads t, not x), into LDS as [channel][halo pixel].
//   * phase B  wave w takes tile row w: lane (n, kh) = column n, channels [kh C/2, (kh + 1) C/2) in groups of four -- 3 x 3 window from LDS,
//              nine FMAs, SiLU; xc goes to global memory (128-byte row segments per half-wave) and, as [pixel][channel], to LDS.
//   * phase C  the same wave multiplies its own 32 pixels by W_x (one row block of 32 >= Mx rows): the B operand's 8 channels per lane come
//              back from LDS, are split into limbs and meet the packed weights; rows < Mx are stored.  Phase B and C exchange data inside
//              one wave only: a single barrier (after phase A) per workgroup.
// Weights are read per wave from L2 in operand order (27 KB per workgroup at C = 40).  Requires C <= 48, C % 8 == 0 (two channel halves of
// whole groups of four), Mx <= 32.
#include "bem_common.h"
#include "x6_tile.h"

namespace {

struct SfX {
    const float* x; const float* ln_w; const float* ln_b; float ln_eps;
    const u32x4* Wpi; const float* bi;      // in_proj: x6-packed (C, C) [MT][KB][3][64], bias (C) | NULL
    const float* dww; const float* dwb;     // depthwise (C, 9), (C) | NULL
    const u32x4* Wpx;                       // x_proj: x6-packed (Mx, C), one row block
    float* xc; float* xd;
    int C, Mx, H, W, tx;
};

// base[byte / 4] with a byte offset of type OFF: a wave-uniform base in scalar registers and one 32-bit register per lane address where
// the host has checked max(C, Mx) H W < 2^30 (OFF = uint32_t); the *_wide entry point runs the same source with OFF = uint64_t
template <typename OFF>
__device__ __forceinline__ float at_byte(const float* base, OFF byte) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte);
}
template <typename OFF>
__device__ __forceinline__ void put_byte(float* base, OFF byte, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte) = v;
}

constexpr bool SF_SILU_RCP = true;     // SiLU through v_rcp_f32 + one Newton step; false: bem_silu's IEEE division

// x / (1 + exp(-x)) without the IEEE division sequence: r = rcp(d) refined once (r + r (1 - d r)) is within 1 ulp of 1 / d.  exp(-x) is
// held below 2^116 so that d r never becomes inf * 0: there the result is about x * 2^-115 where the division gives -0 (below 1e-30 for |x| < 1e4).
__device__ __forceinline__ float silu_rcp(float x) {
    const float d = 1.f + bem_fexp(fminf(-x, 80.f));
    const float r = __builtin_amdgcn_rcpf(d);
    return x * fmaf(fmaf(-d, r, 1.f), r, r);
}

// KBM: k-blocks of 16 channels; CR: channel rows kept in LDS (C <= CR <= 16 KBM, CR % 4 == 0) -- 40 for the bench's width, so that two
// workgroups fit a CU next to the staged in_proj operands.  CC: the channel count where the launcher sends one width only to the form
// (<3, 40>, <3, 48>), 0 where it is k.C.  The launcher picks KBM = ceil(C / 16) and C % 8 == 0: a lane's eight channels of a k-block are
// all inside C or all padding, and only the last k-block can hold padding.
template <int KBM, int CR, int CC, typename OFF>
__device__ __forceinline__ void ss2d_front_x6_tile(const SfX& k) {
    constexpr int MTI = (CR + 31) / 32;              // row blocks of in_proj
    constexpr int GS = CR + 4;                       // dwords per pixel row of G (conflict-free 16-byte accesses)
    constexpr int NG = CR / 8;                       // groups of four channels per half-wave, at most
    __shared__ __attribute__((aligned(16))) float T[CR * XT_TS];                       // [channel][halo pixel]
    __shared__ __attribute__((aligned(16))) float G[128 * GS + 8];                     // [tile pixel][channel], eight zeros behind the last pixel
    __shared__ __attribute__((aligned(16))) u32x4 Wil[MTI * KBM * 3 * 64];             // in_proj operands [mt][kb][limb][lane], by LDS-DMA
    __shared__ __attribute__((aligned(16))) float DWl[CR * 12];                        // depthwise taps [channel][9 taps, bias, 2 pad]
    __shared__ float Bil[32 * MTI];                                                          // in_proj bias (zeros without one / past C)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z;
    const int C = CC ? CC : k.C;
    int y0, x0;
    tile_origin(k.tx, y0, x0);
    const int L = k.H * k.W;
    const OFF L4 = (OFF)4 * (OFF)L;
    const float* xb = k.x + (int64_t)b * C * L;

    // in_proj operands: one LDS-DMA copy per workgroup at kernel start (they land under the LayerNorm prologue)
    {
        const uint32_t wl_lds = lds_addr(Wil), voff = 16 * lane;
#pragma unroll
        for (int t = 0; t < (MTI * KBM * 3 + 3) / 4; ++t) {
            const int p = wave + 4 * t;
            if (p < MTI * KBM * 3) glds16(k.Wpi + (int64_t)p * 64, voff, wl_lds + p * 1024);
        }
    }
    // small per-channel parameters into LDS: phase B's lanes of the two half-waves work on different channels.  One thread per channel
    // row (rows past C are zero); the eight zeros of G serve phase C's channel groups past C.
    if (threadIdx.x < CR) {
        const int c = threadIdx.x, cc = min(c, C - 1);
        const float on = c < C ? 1.f : 0.f;
        float w[12];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = k.dww[cc * 9 + t] * on;
        w[9] = k.dwb ? k.dwb[cc] * on : 0.f;
        w[10] = w[11] = 0.f;
        f32x4* dp = reinterpret_cast<f32x4*>(DWl + 12 * c);
#pragma unroll
        for (int q = 0; q < 3; ++q) dp[q] = f32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
    }
    if (threadIdx.x < 32 * MTI) Bil[threadIdx.x] = (k.bi && (int)threadIdx.x < C) ? k.bi[min((int)threadIdx.x, C - 1)] : 0.f;
    if (threadIdx.x < 8) G[128 * GS + threadIdx.x] = 0.f;

    // ---- this wave's halo pixel blocks (w, w + 4): load, LayerNorm over channels, zero outside the image, split into limbs
    u32x4 xl[2][KBM][3];
    float msk[2];
    int hpo[2];
    {
        float lnw[KBM][8], lnb[KBM][8];
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb) {
            const bool von = kb < KBM - 1 || 16 * kb + 8 * kh < C;
            const uint32_t c4 = von ? 32u * kh : 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float w = at_byte(k.ln_w + 16 * kb + e, c4), bb = at_byte(k.ln_b + 16 * kb + e, c4);
                lnw[kb][e] = kb < KBM - 1 ? w : (von ? w : 0.f);
                lnb[kb][e] = kb < KBM - 1 ? bb : (von ? bb : 0.f);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hp = min((wave + 4 * i) * 32 + n, XT_TS - 1);
            hpo[i] = hp;
            const int hy = hp / XT_HW, hx = hp - hy * XT_HW;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
            const bool in = hp < XT_NPH && gy >= 0 && gy < k.H && gx >= 0 && gx < k.W && (wave + 4 * i) < XT_NPB;
            msk[i] = in ? 1.f : 0.f;
            // one offset per lane (channel 8 kh of the pixel); the channel steps (16 kb + e) L4 are wave-uniform
            const OFF off4 = (OFF)4 * (OFF)(min(max(gy, 0), k.H - 1) * k.W + min(max(gx, 0), k.W - 1));
            const OFF a = off4 + (kh ? (OFF)8 * L4 : (OFF)0);
            float xr[KBM][8];
#pragma unroll
            for (int kb = 0; kb < KBM; ++kb) {
                const bool von = kb < KBM - 1 || 16 * kb + 8 * kh < C;
                const OFF ak = kb < KBM - 1 ? a : (von ? a : off4 - (OFF)(16 * kb) * L4);   // padding re-reads channels 0 .. 7
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = at_byte(xb, ak + (OFF)(16 * kb + e) * L4);
                    xr[kb][e] = kb < KBM - 1 ? v : (von ? v : 0.f);
                }
            }
            const float inv = 1.f / (float)C;
            float s = 0.f;
#pragma unroll
            for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
                for (int e = 0; e < 8; ++e) s += xr[kb][e];
            s += __shfl_xor(s, 32, 64);
            const float mean = s * inv;
            float q = 0.f;
#pragma unroll
            for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = (kb < KBM - 1 || 16 * kb + 8 * kh < C) ? xr[kb][e] - mean : 0.f;
                    q = fmaf(d, d, q);
                }
            q += __shfl_xor(q, 32, 64);
            const float rstd = msk[i] / sqrtf(q * inv + k.ln_eps);
#pragma unroll
            for (int kb = 0; kb < KBM; ++kb) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = ((xr[kb][e] - mean) * rstd) * lnw[kb][e] + lnb[kb][e] * msk[i];
                split8(v, xl[i][kb][0], xl[i][kb][1], xl[i][kb][2]);
            }
        }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                                                   // DWl / Bil / Wil visible
    // ---- phase A: t = W_in xn + b_in over the halo, zero outside the image, into T.  Row groups of four from CR on are not kept.
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (wave + 4 * i < XT_NPB) {                                                   // wave-uniform
#pragma unroll
            for (int mt = 0; mt < MTI; ++mt) {
                f32x16 hi = zero16(), lo = zero16();
#pragma unroll
                for (int kb = 0; kb < KBM; ++kb) {
                    const u32x4* wp = Wil + (mt * KBM + kb) * 192 + lane;
                    const u32x4 wl[3] = {wp[0], wp[64], wp[128]};
                    mac6(wl, xl[i][kb], hi, lo);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = acc_row(r, kh, 32 * mt);
                    if (32 * mt + 8 * (r >> 2) < CR) T[row * XT_TS + hpo[i]] = (hi[r] + lo[r] + Bil[row]) * msk[i];
                }
            }
        }
    }
    __syncthreads();

    // x_proj operands: requested now, used after phase B
    u32x4 wx[KBM][3];
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb) {
        const u32x4* wp = k.Wpx + kb * 192 + lane;
#pragma unroll
        for (int li = 0; li < 3; ++li) wx[kb][li] = wp[64 * li];
    }
    // ---- phase B: depthwise 3x3 + SiLU for tile row `wave`; lane = column n, channel half kh, groups of four channels
    const int oy = y0 + wave, ox = x0 + n;
    const bool opix = oy < k.H && ox < k.W;
    const OFF pix4 = (OFF)4 * (OFF)(min(oy, k.H - 1) * k.W + min(ox, k.W - 1));
    const int chalf = C >> 1;                                                          // C % 8 == 0: whole groups of four per half
    float* gp = G + (wave * 32 + n) * GS;
    f32x4 o[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (4 * g < chalf) {                                                           // wave-uniform (compile-time with CC)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = kh * chalf + 4 * g + j;
                const float* tp = T + c * XT_TS + wave * XT_HW + n;                    // halo (wave, n) = window origin of tile pixel (wave, n)
                const f32x4* wv = reinterpret_cast<const f32x4*>(DWl + c * 12);
                const f32x4 w0 = wv[0], w1 = wv[1], w2 = wv[2];
                const float wq[9] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0]};
                float a = w2[1];
#pragma unroll
                for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                    for (int tx = 0; tx < 3; ++tx) a = fmaf(wq[3 * ty + tx], tp[ty * XT_HW + tx], a);
                o[g][j] = SF_SILU_RCP ? silu_rcp(a) : bem_silu(a);
            }
            *reinterpret_cast<f32x4*>(gp + kh * chalf + 4 * g) = o[g];
        }
    }
    if (opix) {                                                                        // xc: one exec mask, 128-byte row segments per half-wave
        float* xcb = k.xc + (int64_t)b * C * L;
        const OFF pc = pix4 + (kh ? (OFF)chalf * L4 : (OFF)0);
#pragma unroll
        for (int g = 0; g < NG; ++g)
            if (4 * g < chalf) {
#pragma unroll
                for (int j = 0; j < 4; ++j) put_byte(xcb, pc + (OFF)(4 * g + j) * L4, o[g][j]);
            }
    }

    // ---- phase C: xd = W_x xc for the same 32 pixels (data crosses the two half-waves of this wave only).  A lane's eight channels of the
    // last k-block that lie past C come from the zeros behind G (their operand weights are zero as well)
    {
        f32x16 hi = zero16(), lo = zero16();
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb) {
            const float* gq = (kb < KBM - 1 || 16 * kb + 8 * kh < C) ? gp + 16 * kb + 8 * kh : G + 128 * GS;
            const f32x4 ga = *reinterpret_cast<const f32x4*>(gq), gb = *reinterpret_cast<const f32x4*>(gq + 4);
            const float v[8] = {ga[0], ga[1], ga[2], ga[3], gb[0], gb[1], gb[2], gb[3]};
            u32x4 gl[3];
            split8(v, gl[0], gl[1], gl[2]);
            mac6(wx[kb], gl, hi, lo);
        }
        if (opix) {
            float* xdb = k.xd + (int64_t)b * k.Mx * L;
            const OFF pd = pix4 + (kh ? (OFF)4 * L4 : (OFF)0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ru = acc_row(r, 0);
                if (ru + 4 * kh < k.Mx) put_byte(xdb, pd + (OFF)ru * L4, hi[r] + lo[r]);
            }
        }
    }
}

template <int KBM, int CR>
__global__ __launch_bounds__(256, 2) void ss2d_front_x6_kernel(SfX k) {
    ss2d_front_x6_tile<KBM, CR, (KBM == 3 ? CR : 0), uint32_t>(k);
}

// max(C, Mx) H W of 2^30 .. 2^31 elements per image: 64-bit byte offsets
template <int KBM, int CR>
__global__ __launch_bounds__(256, 1) void ss2d_front_x6_wide_kernel(SfX k) {
    ss2d_front_x6_tile<KBM, CR, (KBM == 3 ? CR : 0), uint64_t>(k);
}

}  // namespace

extern "C" int bem_ss2d_front_x6_f32(const float* x, const float* ln_w, const float* ln_b, float ln_eps, const float* Wp_in, const float* bias_in,
                                     const float* dww, const float* dwb, const float* Wp_x, float* xc, float* xd, int B, int C, int Mx, int H,
                                     int W, void* stream) {
    BEM_REQUIRE(x && ln_w && ln_b && Wp_in && dww && Wp_x && xc && xd, "ss2d_front_x6: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 65535 && C > 0 && C <= 48 && C % 8 == 0 && Mx > 0 && Mx <= 32 && H > 0 && W > 0,
                "ss2d_front_x6: needs C <= 48, C %% 8 == 0 and Mx <= 32 (got C = %d, Mx = %d)", C, Mx);
    BEM_REQUIRE((((uintptr_t)Wp_in | (uintptr_t)Wp_x) & 15) == 0, "ss2d_front_x6: packed weights must be 16-byte aligned");
    BEM_REQUIRE(x != xc, "ss2d_front_x6: in-place operation is not supported (halo reads)");
    BEM_REQUIRE((int64_t)max(C, Mx) * H * W < (1ll << 31), "ss2d_front_x6: plane set too large for 32-bit offsets");
    if (B == 0) return BEM_OK;
    SfX k;
    k.x = x; k.ln_w = ln_w; k.ln_b = ln_b; k.ln_eps = ln_eps;
    k.Wpi = reinterpret_cast<const u32x4*>(Wp_in); k.bi = bias_in; k.dww = dww; k.dwb = dwb; k.Wpx = reinterpret_cast<const u32x4*>(Wp_x);
    k.xc = xc; k.xd = xd; k.C = C; k.Mx = Mx; k.H = H; k.W = W; k.tx = cdiv(W, XT_TW);
    dim3 grid(k.tx * cdiv(H, XT_TH), 1, B);
    hipStream_t s = (hipStream_t)stream;
    const int KB = cdiv(C, 16);
    // <3, 40> and <3, 48> have their channel count compiled in: C = 40 and C = 48 are the only widths of three k-blocks (C % 8 == 0)
    if ((int64_t)max(C, Mx) * H * W >= (1ll << 30)) {
        if (KB == 1) ss2d_front_x6_wide_kernel<1, 16><<<grid, 256, 0, s>>>(k);
        else if (KB == 2) ss2d_front_x6_wide_kernel<2, 32><<<grid, 256, 0, s>>>(k);
        else if (C == 40) ss2d_front_x6_wide_kernel<3, 40><<<grid, 256, 0, s>>>(k);
        else ss2d_front_x6_wide_kernel<3, 48><<<grid, 256, 0, s>>>(k);
    }
    else if (KB == 1) ss2d_front_x6_kernel<1, 16><<<grid, 256, 0, s>>>(k);
    else if (KB == 2) ss2d_front_x6_kernel<2, 32><<<grid, 256, 0, s>>>(k);
    else if (C == 40) ss2d_front_x6_kernel<3, 40><<<grid, 256, 0, s>>>(k);
    else ss2d_front_x6_kernel<3, 48><<<grid, 256, 0, s>>>(k);
    return bem_check_launch("ss2d_front_x6");
}
