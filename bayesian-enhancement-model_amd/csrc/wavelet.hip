// Quaternion / Haar primitives: the quaternion stack + DWT of an RGB image (and of the enlarged Stage-I conditions), DWT, IWT,
// IWT + Hamilton product, Hamilton products.  Their backward kernels are in backward.hip.
#include "bem_common.h"
#include "wavelet.h"

namespace {

// ---------------------------------------------------------------- quaternion + Haar ----------
// The 8-channel quaternion stack of one RGB sample (QD/model4.py:7-18), into column s of q.
__device__ __forceinline__ void quat_stack(float r, float g, float bl, float (&q)[8][4], int s) {
    const float den = fmaxf(fmaxf(r, g), bl) + 1e-7f;
    q[0][s] = 0.f; q[1][s] = 0.f;
    q[2][s] = r / den; q[3][s] = r;
    q[4][s] = g / den; q[5][s] = g;
    q[6][s] = bl / den; q[7][s] = bl;
}

// Haar butterfly of a 2x2 block q = [(even row, even col), (odd row, even col), (even, odd), (odd, odd)] -> LL, HL, LH, HH (model4.py:216-236)
__device__ __forceinline__ void haar_bands(const float (&q)[4], float (&o)[4]) {
    const float a = q[0] / 2, bb = q[1] / 2, cc = q[2] / 2, d = q[3] / 2;
    o[0] = a + bb + cc + d;
    o[1] = -a - bb + cc + d;
    o[2] = -a + bb - cc + d;
    o[3] = a - bb - cc + d;
}

// One thread per output (half-res) pixel: reads the 2x2 RGB block, forms the 8-channel quaternion
// stack and writes the 4 Haar bands (QD/model4.py:7-18,216-236).
__global__ void quat_dwt_kernel(const float* __restrict__ rgb, int64_t x_bs, float* __restrict__ out, int H, int W,
                                int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int h2 = H >> 1, w2 = W >> 1;
    const int x = (int)(i % w2), y = (int)((i / w2) % h2), b = (int)(i / ((int64_t)w2 * h2));
    const float* p = rgb + (int64_t)b * x_bs;
    const int64_t HW = (int64_t)H * W;
    float q[8][4];   // [channel][a: (even row, even col), b: (odd row, even col), c: (even, odd), d: (odd, odd)]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int yy = 2 * y + (s & 1), xx = 2 * x + (s >> 1);
        quat_stack(p[(int64_t)yy * W + xx], p[HW + (int64_t)yy * W + xx], p[2 * HW + (int64_t)yy * W + xx], q, s);
    }
    const int64_t hw2 = (int64_t)h2 * w2;
    float* o = out + (int64_t)b * 32 * hw2 + (int64_t)y * w2 + x;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float v[4];
        haar_bands(q[c], v);
#pragma unroll
        for (int band = 0; band < 4; ++band) o[(int64_t)(8 * band + c) * hw2] = v[band];
    }
}

__global__ void dwt_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int h2 = H >> 1, w2 = W >> 1;
    const int xx = (int)(i % w2), y = (int)((i / w2) % h2);
    const int c = (int)((i / ((int64_t)w2 * h2)) % C), b = (int)(i / ((int64_t)w2 * h2 * C));
    const float* p = x + ((int64_t)b * C + c) * H * W;
    const float a = p[(int64_t)(2 * y) * W + 2 * xx] / 2, bb = p[(int64_t)(2 * y + 1) * W + 2 * xx] / 2;
    const float cc = p[(int64_t)(2 * y) * W + 2 * xx + 1] / 2, d = p[(int64_t)(2 * y + 1) * W + 2 * xx + 1] / 2;
    const int64_t hw2 = (int64_t)h2 * w2;
    float* o = out + ((int64_t)b * 4 * C + c) * hw2 + (int64_t)y * w2 + xx;
    o[0] = a + bb + cc + d;
    o[(int64_t)C * hw2] = -a - bb + cc + d;
    o[(int64_t)2 * C * hw2] = -a + bb - cc + d;
    o[(int64_t)3 * C * hw2] = a - bb - cc + d;
}

__global__ void iwt_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W, int64_t total) {
    // x (B,4C,H,W) -> out (B,C,2H,2W); one thread per input pixel and channel
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int xx = (int)(i % W), y = (int)((i / W) % H);
    const int c = (int)((i / ((int64_t)W * H)) % C), b = (int)(i / ((int64_t)W * H * C));
    const int64_t hw = (int64_t)H * W;
    const float* p = x + ((int64_t)b * 4 * C + c) * hw + (int64_t)y * W + xx;
    float o[4];
    iwt4(p[0], p[(int64_t)C * hw], p[(int64_t)2 * C * hw], p[(int64_t)3 * C * hw], o);
    float* q = out + ((int64_t)b * C + c) * 4 * hw + (int64_t)(2 * y) * (2 * W) + 2 * xx;
    *reinterpret_cast<float2*>(q) = make_float2(o[0], o[2]);
    *reinterpret_cast<float2*>(q + 2 * W) = make_float2(o[1], o[3]);
}

__device__ __forceinline__ void hamilton_ijk(const float (&p)[4], const float (&q)[4], float (&o)[3]) {
    o[0] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
    o[1] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
    o[2] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

__global__ void iwt_hamilton_kernel(const float* __restrict__ q1w, const float* __restrict__ q2w,
                                    float* __restrict__ out, int h, int w, int64_t total) {
    // q*w (B,16,h,w): channel = band*4 + component.  out (B,3,2h,2w).
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int x = (int)(i % w), y = (int)((i / w) % h), b = (int)(i / ((int64_t)w * h));
    const int64_t hw = (int64_t)h * w;
    const float* a = q1w + (int64_t)b * 16 * hw + (int64_t)y * w + x;
    const float* c = q2w + (int64_t)b * 16 * hw + (int64_t)y * w + x;
    float P[4][4], Q[4][4];   // [component][sub-pixel]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        iwt4(a[(int64_t)k * hw], a[(int64_t)(4 + k) * hw], a[(int64_t)(8 + k) * hw], a[(int64_t)(12 + k) * hw], P[k]);
        iwt4(c[(int64_t)k * hw], c[(int64_t)(4 + k) * hw], c[(int64_t)(8 + k) * hw], c[(int64_t)(12 + k) * hw], Q[k]);
    }
    float res[3][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float pp[4] = {P[0][s], P[1][s], P[2][s], P[3][s]};
        const float qq[4] = {Q[0][s], Q[1][s], Q[2][s], Q[3][s]};
        float o[3];
        hamilton_ijk(pp, qq, o);
        res[0][s] = o[0]; res[1][s] = o[1]; res[2][s] = o[2];
    }
    const int W2 = 2 * w;
    float* op = out + (int64_t)b * 3 * 4 * hw + (int64_t)(2 * y) * W2 + 2 * x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float* o = op + (int64_t)k * 4 * hw;
        *reinterpret_cast<float2*>(o) = make_float2(res[k][0], res[k][2]);
        *reinterpret_cast<float2*>(o + W2) = make_float2(res[k][1], res[k][3]);
    }
}

__global__ void hamilton_kernel(const float* __restrict__ q, float* __restrict__ out, int64_t HW, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int64_t pix = i % HW, b = i / HW;
    const float* p = q + b * 8 * HW + pix;
    const float pp[4] = {p[0], p[HW], p[2 * HW], p[3 * HW]};
    const float qq[4] = {p[4 * HW], p[5 * HW], p[6 * HW], p[7 * HW]};
    float o[3];
    hamilton_ijk(pp, qq, o);
    float* op = out + b * 3 * HW + pix;
    op[0] = o[0]; op[HW] = o[1]; op[2 * HW] = o[2];
}

// all four components (real part first), the reference's hamilton_product (QD/quaternion.py:3-17)
__global__ void hamilton_full_kernel(const float* __restrict__ q1, const float* __restrict__ q2, float* __restrict__ out, int64_t HW, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int64_t pix = i % HW, b = i / HW;
    const float* p = q1 + b * 4 * HW + pix;
    const float* q = q2 + b * 4 * HW + pix;
    const float pp[4] = {p[0], p[HW], p[2 * HW], p[3 * HW]};
    const float qq[4] = {q[0], q[HW], q[2 * HW], q[3 * HW]};
    float o[3];
    hamilton_ijk(pp, qq, o);
    float* op = out + b * 4 * HW + pix;
    op[0] = pp[0] * qq[0] - pp[1] * qq[1] - pp[2] * qq[2] - pp[3] * qq[3];
    op[HW] = o[0]; op[2 * HW] = o[1]; op[3 * HW] = o[2];
}

// quat_dwt(bilinear_up(cond, s)) of the Stage-I conditions (R,3,H,W) without the enlarged image: a thread owns NPX neighbouring pixels of a
// row of the (R,32,H s/2,W s/2) output, interpolates their 2 x 2 NPX x 3 samples from the candidate's 3 H W source values (12 KiB of
// conditions per 8 MiB of output: every read after the first is an L1 hit), and writes each of the 32 planes with one 4 NPX-byte store.
template <int NPX>
__global__ __launch_bounds__(256) void cond_dwt_kernel(const float* __restrict__ cond, float* __restrict__ out, int H, int W, int s, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int h2 = (H * s) >> 1, w2 = (W * s) >> 1, wq = w2 / NPX;
    const int x = (int)(i % wq) * NPX, y = (int)((i / wq) % h2), b = (int)(i / ((int64_t)wq * h2));
    const float rs = 1.f / (float)s;
    const float* p = cond + (int64_t)b * 3 * H * W;
    const int HW = H * W;
    float q[NPX][8][4];
#pragma unroll
    for (int j = 0; j < NPX; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int yy = 2 * y + (t & 1), xx = 2 * (x + j) + (t >> 1);
            quat_stack(bilinear_at(p, H, W, rs, yy, xx), bilinear_at(p + HW, H, W, rs, yy, xx), bilinear_at(p + 2 * HW, H, W, rs, yy, xx), q[j], t);
        }
    typedef float fpx __attribute__((ext_vector_type(NPX)));
    const int64_t hw2 = (int64_t)h2 * w2;
    float* o = out + (int64_t)b * 32 * hw2 + (int64_t)y * w2 + x;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float v[NPX][4];
#pragma unroll
        for (int j = 0; j < NPX; ++j) haar_bands(q[j][c], v[j]);
#pragma unroll
        for (int band = 0; band < 4; ++band) {
            fpx w;
#pragma unroll
            for (int j = 0; j < NPX; ++j) w[j] = v[j][band];
            *reinterpret_cast<fpx*>(o + (int64_t)(8 * band + c) * hw2) = w;
        }
    }
}

}  // namespace

// ================================================================ C ABI =========================
extern "C" int bem_quat_dwt_f32(const float* rgb, int64_t x_bstride, float* out, int B, int H, int W, void* stream) {
    BEM_REQUIRE(rgb && out, "quat_dwt: null tensor");
    BEM_REQUIRE(B >= 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "quat_dwt: H, W must be even (got %d x %d)", H, W);
    if (B == 0) return BEM_OK;
    const int64_t total = (int64_t)B * (H / 2) * (W / 2);
    quat_dwt_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(rgb, x_bstride, out, H, W, total);
    return bem_check_launch("quat_dwt");
}

extern "C" int bem_cond_dwt_f32(const float* cond, float* out, int R, int H, int W, int s, void* stream) {
    BEM_REQUIRE(cond && out, "cond_dwt: null tensor");
    BEM_REQUIRE(R >= 0 && H > 0 && W > 0 && s >= 1 && (int64_t)H * s < (1 << 24) && (int64_t)W * s < (1 << 24) && (H * s) % 2 == 0 && (W * s) % 2 == 0,
                "cond_dwt: the enlarged image (%d x %d times %d) must have even sides", H, W, s);
    if (R == 0) return BEM_OK;
    const int h2 = H * s / 2, w2 = W * s / 2;
    if (w2 % 4 == 0 && ((uintptr_t)out & 15) == 0) {
        const int64_t total = (int64_t)R * h2 * (w2 / 4);
        cond_dwt_kernel<4><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(cond, out, H, W, s, total);
    } else {
        const int64_t total = (int64_t)R * h2 * w2;
        cond_dwt_kernel<1><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(cond, out, H, W, s, total);
    }
    return bem_check_launch("cond_dwt");
}

extern "C" int bem_dwt_f32(const float* x, float* out, int B, int C, int H, int W, void* stream) {
    BEM_REQUIRE(x && out, "dwt: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "dwt: H, W must be even");
    if (B == 0) return BEM_OK;
    const int64_t total = (int64_t)B * C * (H / 2) * (W / 2);
    dwt_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, C, H, W, total);
    return bem_check_launch("dwt");
}

extern "C" int bem_iwt_f32(const float* x, float* out, int B, int C4, int H, int W, void* stream) {
    BEM_REQUIRE(x && out, "iwt: null tensor");
    BEM_REQUIRE(B >= 0 && C4 > 0 && C4 % 4 == 0 && H > 0 && W > 0, "iwt: channels %d must be a multiple of 4", C4);
    if (B == 0) return BEM_OK;
    const int64_t total = (int64_t)B * (C4 / 4) * H * W;
    iwt_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, C4 / 4, H, W, total);
    return bem_check_launch("iwt");
}

extern "C" int bem_iwt_hamilton_f32(const float* q1w, const float* q2w, float* out, int B, int h, int w, void* stream) {
    BEM_REQUIRE(q1w && q2w && out, "iwt_hamilton: null tensor");
    BEM_REQUIRE(B >= 0 && h > 0 && w > 0, "iwt_hamilton: bad shape");
    if (B == 0) return BEM_OK;
    const int64_t total = (int64_t)B * h * w;
    iwt_hamilton_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(q1w, q2w, out, h, w, total);
    return bem_check_launch("iwt_hamilton");
}

extern "C" int bem_hamilton_full_f32(const float* q1, const float* q2, float* out, int B, int H, int W, void* stream) {
    BEM_REQUIRE(q1 && q2 && out && B >= 0 && H > 0 && W > 0, "hamilton_full: bad arguments");
    if (B == 0) return BEM_OK;
    const int64_t total = (int64_t)B * H * W;
    hamilton_full_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(q1, q2, out, (int64_t)H * W, total);
    return bem_check_launch("hamilton_full");
}

extern "C" int bem_hamilton_f32(const float* q, float* out, int B, int H, int W, void* stream) {
    BEM_REQUIRE(q && out, "hamilton: null tensor");
    BEM_REQUIRE(B >= 0 && H > 0 && W > 0, "hamilton: bad shape");
    if (B == 0) return BEM_OK;
    const int64_t total = (int64_t)B * H * W;
    hamilton_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(q, out, (int64_t)H * W, total);
    return bem_check_launch("hamilton");
}
