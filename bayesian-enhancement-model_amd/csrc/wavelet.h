// Device functions that two sources must evaluate alike to the bit: iwt4 (wavelet.hip and its backward in backward.hip) and bilinear_at
// (bilinear_up in layout.hip, cond_dwt in wavelet.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void iwt4(float ll, float hl, float lh, float hh, float (&o)[4]) {
    // o[0]=(even row, even col) o[1]=(odd row, even col) o[2]=(even, odd) o[3]=(odd, odd)  (model4.py:26-35)
    ll /= 2; hl /= 2; lh /= 2; hh /= 2;
    o[0] = ll - hl - lh + hh;
    o[1] = ll - hl + lh - hh;
    o[2] = ll + hl - lh - hh;
    o[3] = ll + hl + lh + hh;
}

// PyTorch upsample_bilinear2d, align_corners=False, scale_factor given: src = (dst + 0.5)/s - 0.5 clamped at 0.  Value of output pixel
// (yo, xo) of the H x W plane p enlarged by s = 1 / rs,
//     hy (hx p[y0][x0] + lx p[y0][x1]) + ly (hx p[y1][x0] + lx p[y1][x1]),
// shared by bilinear_up_kernel and cond_dwt_kernel.  Which products are rounded and which are fused is written out (contraction is off
// inside): left to the compiler it depends on the code around the expression, and the two kernels have to agree to the bit.
__device__ __forceinline__ float bilinear_at(const float* __restrict__ p, int H, int W, float rs, int yo, int xo) {
#pragma clang fp contract(off)
    float sy = __builtin_fmaf((float)yo + 0.5f, rs, -0.5f); sy = sy < 0.f ? 0.f : sy;
    float sx = __builtin_fmaf((float)xo + 0.5f, rs, -0.5f); sx = sx < 0.f ? 0.f : sx;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float t0 = __builtin_fmaf(lx, p[(int64_t)y0 * W + x1], hx * p[(int64_t)y0 * W + x0]);
    const float t1 = __builtin_fmaf(hx, p[(int64_t)y1 * W + x0], lx * p[(int64_t)y1 * W + x1]);
    return hy * t0 + ly * t1;
}
