// Decoder up-sampling folded into the fuse GEMM: fuse(cat(up(f), skip)) of a Stage-II decoder level in one kernel.
//
//   up   = ConvTranspose2d(C, C/2, kernel 2, stride 2) with bias bt, weight Wt (C, C/2, 2, 2)
//   fuse = bias-free 1x1 conv (C/2, C) = [Wf1 | Wf2] over cat(up(f), skip)
//
// Both are linear and nothing sits between them, so with the per-phase matrices Wc[a,b] = Wf1 * Wt[:, :, a, b]^T (C/2 x C) and bc = Wf1 * bt
// (composed once per weight version on the host side, bem.modules.fold_up_fuse)
//
//   out[co][2i+a][2j+b] = sum_k Wc[a,b][co][k] f[k][i][j]  +  sum_c Wf2[co][c] skip[c][2i+a][2j+b]  +  bc[co]
//
// and the up-sampled tensor is never written or read: f, skip and out cross memory once each.  Same limb arithmetic as pw_gemm_x6.hip
// (split8, six products, the small products in their own accumulator).
//
// Mapping: one wave = 32 consecutive low-res pixels of one batch row (they may cross low-res row ends: (i, j) is computed once per lane
// from the flattened index); lane l owns pixel p0 + (l & 31), the two lane halves hold the two channel octets of a k-block.  For output row
// parity a the lane reads the skip pair (2j, 2j+1) of row 2i+a as one 8-byte load per channel -- the two values are the B operands of the
// b = 0 and b = 1 phases -- and stores the out pair the same way, so a half-wave touches whole contiguous lines on both sides.  A wave
// does one pass (one a, MTW M-tiles): acc[m][b] as (large, small) pairs = 128 registers at MTW = 2.  The passes over the same pixels are
// neighbouring workgroups (grid.y), so f comes from memory once and from L2 for the others; it is streamed k-block by k-block, two
// blocks ahead of the MFMAs, weights one block ahead.  (Both row parities in one wave, with f held as limbs, does not fit the 256 registers
// of two waves per SIMD at K = 80, and as a loop the compiler parks the loop-invariant addresses of the second pass in scratch.)
// Weights: Wc = bem_pack_pw_weight_x6 of the (4, C/2, C) phase matrices (set = 2a + b), Wf2 = the same of (C/2, C/2).
#include "bem_common.h"
#include "x6_common.h"

namespace {

struct UfX {
    const float* f; const float* skip; const u32x4* Wc; const u32x4* Wf2; const float* bias; float* out;
    int C, Co, w, L;        // input channels, output channels = skip channels = C / 2, low-res width, low-res pixels h * w
    int KB, KB2, MT;        // k-blocks of f (C), k-blocks of skip (Co), M-tiles (Co)
};

// grid (ceil(L / 128), 2 * ceil(MT / MTW), B): y = 2 * M-tile group + output row parity; 4 independent waves per workgroup, no LDS, no barrier
template <int MTW>
__global__ __launch_bounds__(256, 2) void upfuse_x6_kernel(UfX k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kh = lane >> 5, n = lane & 31;
    const int b = blockIdx.z, a = blockIdx.y & 1, mt0 = (blockIdx.y >> 1) * MTW;     // a: output row parity of this pass
    const int p0 = (xcd_tile(blockIdx.x, gridDim.x) * 4 + wave) * 32;
    if (p0 >= k.L) return;
    const int p = p0 + n;
    const bool keep = p < k.L;
    const int pc = keep ? p : k.L - 1;                       // clamped: every address below is valid, lanes past the end store nothing
    const int i = pc / k.w, j = pc - i * k.w;
    const int Lo = 4 * k.L, Wo = 2 * k.w;
    const uint32_t hi_off = (uint32_t)(2 * i) * (uint32_t)Wo + (uint32_t)(2 * j);       // (row 2i, column 2j) of a high-res plane
    const float* fb = k.f + (int64_t)b * k.C * k.L;          // uniform batch-row bases; lane offsets stay below 2^30 (checked at launch)
    const float* sb = k.skip + (int64_t)b * k.Co * Lo;
    float* ob = k.out + (int64_t)b * k.Co * Lo;
    const bool two = MTW == 2 && mt0 + 1 < k.MT;             // uniform: the second M-tile of this group exists

    auto load_f = [&](int kb, float (&dst)[8]) {             // channels >= C come back as zeros; k-blocks past the end are never used
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = 16 * kb + 8 * kh + e;
            const float v = fb[(uint32_t)min(ch, k.C - 1) * (uint32_t)k.L + (uint32_t)pc];
            dst[e] = v * (ch < k.C ? 1.f : 0.f);
        }
    };
    auto load_s = [&](int kb, uint32_t off, float (&dst)[8][2]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = 16 * kb + 8 * kh + e;
            const float2 v = *reinterpret_cast<const float2*>(sb + ((uint32_t)min(ch, k.Co - 1) * (uint32_t)Lo + off));
            const float mk = ch < k.Co ? 1.f : 0.f;
            dst[e][0] = v.x * mk; dst[e][1] = v.y * mk;
        }
    };
    // one (M-tile, k-block) of a packed set: 3 limbs of 1 KiB; M-tiles past MT and k-blocks past the end re-read a valid block that no MFMA uses
    auto load_w = [&](const u32x4* set, int kbn, int kb, u32x4 (&dst)[MTW][3]) {
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const u32x4* wp = set + ((int64_t)min(mt0 + m, k.MT - 1) * kbn + min(kb, kbn - 1)) * (3 * 64) + lane;
#pragma unroll
            for (int li = 0; li < 3; ++li) dst[m][li] = wp[li * 64];
        }
    };
    const int64_t set_stride = (int64_t)k.MT * k.KB * 3 * 64;

    {
        const uint32_t row_off = hi_off + (uint32_t)(a * Wo);
        const int kh4 = 4 * kh;                                  // the lane half's row offset inside an M-tile (epilogue)
        f32x16 acc[MTW][2], alo[MTW][2];
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][t][r] = alo[m][t][r] = 0.f;
        u32x4 wn[MTW][3];
        // ---- skip: Wf2 against the pair's two pixels ----
        {
            float sn[8][2];
            load_s(0, row_off, sn);
            load_w(k.Wf2, k.KB2, 0, wn);
            for (int kb = 0; kb < k.KB2; ++kb) {
                u32x4 xl[2][3], wc[MTW][3];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = sn[e][t];
                    split8(v, xl[t][0], xl[t][1], xl[t][2]);
                }
#pragma unroll
                for (int m = 0; m < MTW; ++m)
#pragma unroll
                    for (int li = 0; li < 3; ++li) wc[m][li] = wn[m][li];
                load_s(kb + 1, row_off, sn);
                load_w(k.Wf2, k.KB2, kb + 1, wn);
#pragma unroll
                for (int m = 0; m < MTW; ++m)
                    if (m == 0 || two) {
#pragma unroll
                        for (int t = 0; t < 2; ++t) mac6(wc[m], xl[t], acc[m][t], alo[m][t]);
                    }
            }
        }
        // ---- f: the phase matrices Wc[a, 0] and Wc[a, 1] against the low-res pixel ----
        {
            const u32x4* w0 = k.Wc + (int64_t)(2 * a) * set_stride;
            const u32x4* w1 = w0 + set_stride;
            float fn[8], fn2[8];
            load_f(0, fn);
            load_f(1, fn2);
            load_w(w0, k.KB, 0, wn);
            for (int kb = 0; kb < k.KB; ++kb) {
                u32x4 xl[3], wc[MTW][3];
                split8(fn, xl[0], xl[1], xl[2]);
#pragma unroll
                for (int e = 0; e < 8; ++e) fn[e] = fn2[e];
                load_f(kb + 2, fn2);
#pragma unroll
                for (int m = 0; m < MTW; ++m)
#pragma unroll
                    for (int li = 0; li < 3; ++li) wc[m][li] = wn[m][li];
                load_w(w1, k.KB, kb, wn);
#pragma unroll
                for (int m = 0; m < MTW; ++m)
                    if (m == 0 || two) mac6(wc[m], xl, acc[m][0], alo[m][0]);
#pragma unroll
                for (int m = 0; m < MTW; ++m)
#pragma unroll
                    for (int li = 0; li < 3; ++li) wc[m][li] = wn[m][li];
                load_w(w0, k.KB, kb + 1, wn);
#pragma unroll
                for (int m = 0; m < MTW; ++m)
                    if (m == 0 || two) mac6(wc[m], xl, acc[m][1], alo[m][1]);
            }
        }
        // ---- epilogue: large + (small + bias), the (b = 0, b = 1) pair as one 8-byte store; plane bases uniform, one lane offset ----
        const uint32_t loff = (uint32_t)kh4 * (uint32_t)Lo + row_off;
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            if (mt0 + m >= k.MT) continue;
            const int rb = (mt0 + m) * 32;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float bv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)                       // through a VALU copy before the packed adds
                    bv[q] = valu_copy(k.bias[min(rb + 8 * g + kh4 + q, k.Co - 1)]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = 4 * g + q, urow = rb + 8 * g + q;       // uniform; this lane's row = urow + kh4
                    // small + bias first: that sum rounds at the size of the bias, so the output carries one rounding at its own size;
                    // (large + small) + bias rounds twice there and doubles the worst-case error of a level
                    const float o0 = acc[m][0][r] + (alo[m][0][r] + bv[q]);
                    const float o1 = acc[m][1][r] + (alo[m][1][r] + bv[q]);
                    if (keep && urow + kh4 < k.Co) *reinterpret_cast<float2*>(ob + (int64_t)urow * Lo + loff) = make_float2(o0, o1);
                }
            }
        }
    }
}

}  // namespace

extern "C" int bem_upfuse_x6_f32(const float* f, const float* skip, const float* Wc_packed, const float* Wf2_packed, const float* bias,
                                 float* out, int B, int Cin, int h, int w, void* stream) {
    BEM_REQUIRE(f && skip && Wc_packed && Wf2_packed && bias && out, "upfuse_x6: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 65535 && Cin >= 2 && Cin % 2 == 0 && h > 0 && w > 0, "upfuse_x6: bad shape B=%d Cin=%d h=%d w=%d", B, Cin, h, w);
    BEM_REQUIRE((int64_t)Cin * h * w < (1ll << 29), "upfuse_x6: Cin * h * w = %lld exceeds the 32-bit lane offsets", (long long)Cin * h * w);
    BEM_REQUIRE((((uintptr_t)Wc_packed | (uintptr_t)Wf2_packed) & 15) == 0, "upfuse_x6: packed weights must be 16-byte aligned");
    BEM_REQUIRE((((uintptr_t)skip | (uintptr_t)out) & 7) == 0 && ((uintptr_t)f & 3) == 0, "upfuse_x6: skip / out must be 8-byte aligned");
    if (B == 0) return BEM_OK;
    UfX k;
    k.f = f; k.skip = skip; k.Wc = reinterpret_cast<const u32x4*>(Wc_packed); k.Wf2 = reinterpret_cast<const u32x4*>(Wf2_packed);
    k.bias = bias; k.out = out;
    k.C = Cin; k.Co = Cin / 2; k.w = w; k.L = h * w;
    k.KB = cdiv(k.C, 16); k.KB2 = cdiv(k.Co, 16); k.MT = cdiv(k.Co, 32);
    BEM_REQUIRE(k.MT <= 65535, "upfuse_x6: Cin %d too wide", Cin);
    hipStream_t s = (hipStream_t)stream;
    if (k.MT == 1) {
        upfuse_x6_kernel<1><<<dim3(cdiv(k.L, 128), 2, B), 256, 0, s>>>(k);
    } else {
        upfuse_x6_kernel<2><<<dim3(cdiv(k.L, 128), 2 * cdiv(k.MT, 2), B), 256, 0, s>>>(k);
    }
    return bem_check_launch("upfuse_x6");
}
