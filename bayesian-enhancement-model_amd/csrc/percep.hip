// The bandwidth-bound kernels between the convolutions of the VGG19 perceptual loss (basicsr/losses/basic_loss.py:146-238 over
// basicsr/archs/vgg_arch.py:54-161): input normalisation into the 8-channel 2B-row batch and its adjoint, MaxPool2d(2, 2), the fused
// backward of pool(relu(.)), ReLU and its backward.  Every kernel is one pass, writes each output element exactly once (no memset, no
// atomics) and moves 16-byte pieces where the pointers and the row length allow, single floats otherwise.
#include "bem_common.h"

namespace {

static inline bool host_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct VggNorm { float mean[3], std[3]; };

__device__ __forceinline__ float vgg_norm1(float v, float mean, float std, int range_norm) {
    if (range_norm) v = (v + 1.f) / 2.f;
    return (v - mean) / std;                        // a true division: within 1 ulp of torch's (x - mean) / std
}

// xn (2B, 8, HW): rows [0, B) from pred, [B, 2B) from gt, channels 0..2 normalised, 3..7 zero.  One thread per unit of a plane:
// a float4 (VEC: HW % 4 == 0, aligned tensors) or one float.
template <bool VEC>
__global__ __launch_bounds__(256) void vgg_prep_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       float* __restrict__ xn, int B, int64_t HW, VggNorm nm, int range_norm,
                                                       int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    constexpr int E = VEC ? 4 : 1;
    const int64_t U = HW / E;
    const int64_t u = i % U, pc = i / U;
    const int c = (int)(pc & 7), r = (int)(pc >> 3);
    float* o = xn + pc * HW + u * E;
    if (c >= 3) {
        if constexpr (VEC) *reinterpret_cast<float4*>(o) = make_float4(0.f, 0.f, 0.f, 0.f);
        else *o = 0.f;
        return;
    }
    const float* s = (r < B ? pred + (int64_t)r * 3 * HW : gt + (int64_t)(r - B) * 3 * HW) + (int64_t)c * HW + u * E;
    const float mean = nm.mean[c], std = nm.std[c];
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(s);
        *reinterpret_cast<float4*>(o) = make_float4(vgg_norm1(q.x, mean, std, range_norm), vgg_norm1(q.y, mean, std, range_norm),
                                                    vgg_norm1(q.z, mean, std, range_norm), vgg_norm1(q.w, mean, std, range_norm));
    } else {
        *o = vgg_norm1(*s, mean, std, range_norm);
    }
}

__device__ __forceinline__ float vgg_norm_bwd1(float g, float std, int range_norm) {
    g = g / std;
    return range_norm ? g / 2.f : g;
}

// dpred (B, 3, HW) from channels 0..2 of dxn (batch stride dxn_bs)
template <bool VEC>
__global__ __launch_bounds__(256) void vgg_prep_bwd_kernel(const float* __restrict__ dxn, int64_t dxn_bs, float* __restrict__ dpred,
                                                           int64_t HW, VggNorm nm, int range_norm, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    constexpr int E = VEC ? 4 : 1;
    const int64_t U = HW / E;
    const int64_t u = i % U, pc = i / U;
    const int c = (int)(pc % 3);
    const int64_t b = pc / 3;
    const float* s = dxn + b * dxn_bs + (int64_t)c * HW + u * E;
    float* o = dpred + pc * HW + u * E;
    const float std = nm.std[c];
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(s);
        *reinterpret_cast<float4*>(o) = make_float4(vgg_norm_bwd1(q.x, std, range_norm), vgg_norm_bwd1(q.y, std, range_norm),
                                                    vgg_norm_bwd1(q.z, std, range_norm), vgg_norm_bwd1(q.w, std, range_norm));
    } else {
        *o = vgg_norm_bwd1(*s, std, range_norm);
    }
}

// torch's window walk (row-major, `val > max || isnan(val)`): the first maximum wins.  Returns the value, k = its index 0..3.
__device__ __forceinline__ float window_max(float a, float b, float c, float d, int& k) {
    float m = a;
    k = 0;
    if (b > m || b != b) { m = b; k = 1; }
    if (c > m || c != c) { m = c; k = 2; }
    if (d > m || d != d) { m = d; k = 3; }
    return m;
}

// MaxPool2d(2, 2), floor: x (P, H, W) -> out (P, H/2, W/2).  VEC (W % 8 == 0, aligned): four outputs per thread from four float4 loads.
template <bool VEC>
__global__ __launch_bounds__(256) void maxpool2_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int Ho = H >> 1, Wo = W >> 1;
    constexpr int E = VEC ? 4 : 1;
    const int U = Wo / E;                           // units per output row
    const int u = (int)(i % U), oy = (int)((i / U) % Ho);
    const int64_t p = i / ((int64_t)U * Ho);
    const float* r0 = x + (p * H + 2 * oy) * W + 2 * E * u;
    const float* r1 = r0 + W;
    float* o = out + (p * Ho + oy) * Wo + E * u;
    int k;
    if constexpr (VEC) {
        const float4 a0 = *reinterpret_cast<const float4*>(r0), a1 = *reinterpret_cast<const float4*>(r0 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(r1), b1 = *reinterpret_cast<const float4*>(r1 + 4);
        *reinterpret_cast<float4*>(o) = make_float4(window_max(a0.x, a0.y, b0.x, b0.y, k), window_max(a0.z, a0.w, b0.z, b0.w, k),
                                                    window_max(a1.x, a1.y, b1.x, b1.y, k), window_max(a1.z, a1.w, b1.z, b1.w, k));
    } else {
        *o = window_max(r0[0], r0[1], r1[0], r1[1], k);
    }
}

// dy of one window: dpool at the first maximum where y > 0 there, zero elsewhere
__device__ __forceinline__ void window_bwd(float a, float b, float c, float d, float g, float (&o)[4]) {
    int k;
    const float m = window_max(a, b, c, d, k);
    const float v = m <= 0.f ? 0.f : g;                // torch's threshold_backward: x <= 0 ? 0 : grad
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = j == k ? v : 0.f;
}

// Backward of pool(y), y = relu(.), and of that ReLU: y (P, H, W), dpool (P, H/2, W/2) -> dy (P, H, W).  A thread owns its windows and
// the part of a dropped odd row / column next to them, so every dy element has one writer.  VEC (W % 4 == 0, aligned): two windows.
template <bool VEC>
__global__ __launch_bounds__(256) void relu_pool_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dpool,
                                                            float* __restrict__ dy, int H, int W, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int Ho = H >> 1, Wo = W >> 1;
    constexpr int E = VEC ? 2 : 1;                  // windows per thread
    const int U = Wo / E;
    const int u = (int)(i % U), oy = (int)((i / U) % Ho);
    const int64_t p = i / ((int64_t)U * Ho);
    const int64_t row0 = (p * H + 2 * oy) * W;
    const float* r0 = y + row0 + 2 * E * u;
    const float* r1 = r0 + W;
    float* d0 = dy + row0 + 2 * E * u;
    float* d1 = d0 + W;
    const float* g = dpool + (p * Ho + oy) * Wo + E * u;
    const bool last_row = (H & 1) && oy == Ho - 1;
    if constexpr (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(r0), b = *reinterpret_cast<const float4*>(r1);
        const float2 gq = *reinterpret_cast<const float2*>(g);
        float w0[4], w1[4];
        window_bwd(a.x, a.y, b.x, b.y, gq.x, w0);
        window_bwd(a.z, a.w, b.z, b.w, gq.y, w1);
        *reinterpret_cast<float4*>(d0) = make_float4(w0[0], w0[1], w1[0], w1[1]);
        *reinterpret_cast<float4*>(d1) = make_float4(w0[2], w0[3], w1[2], w1[3]);
        if (last_row) *reinterpret_cast<float4*>(d1 + W) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float w0[4];
        window_bwd(r0[0], r0[1], r1[0], r1[1], g[0], w0);
        d0[0] = w0[0]; d0[1] = w0[1]; d1[0] = w0[2]; d1[1] = w0[3];
        const bool last_col = (W & 1) && u == U - 1;
        if (last_col) { d0[2] = 0.f; d1[2] = 0.f; }
        if (last_row) {
            d1[W] = 0.f; d1[W + 1] = 0.f;
            if (last_col) d1[W + 2] = 0.f;
        }
    }
}

// out = dy * (y > 0) (BWD) or max(y, 0) (forward; torch's relu keeps NaN, as does this form).  In place is fine: one thread reads and
// writes the same elements.  Threads [0, nv) move float4s, threads [nv, nv + tail) the single floats behind them.
template <bool BWD>
__global__ __launch_bounds__(256) void relu_kernel(const float* y, const float* dy, float* out, int64_t nv, int64_t n) {
    const int64_t i = bem_gid1d();
    if (i < nv) {
        const float4 a = reinterpret_cast<const float4*>(y)[i];
        float4 r;
        if constexpr (BWD) {
            const float4 g = reinterpret_cast<const float4*>(dy)[i];
            r = make_float4(a.x <= 0.f ? 0.f : g.x, a.y <= 0.f ? 0.f : g.y, a.z <= 0.f ? 0.f : g.z, a.w <= 0.f ? 0.f : g.w);
        } else {
            r = make_float4(a.x <= 0.f ? 0.f : a.x, a.y <= 0.f ? 0.f : a.y, a.z <= 0.f ? 0.f : a.z, a.w <= 0.f ? 0.f : a.w);
        }
        reinterpret_cast<float4*>(out)[i] = r;
        return;
    }
    const int64_t j = 4 * nv + (i - nv);
    if (j >= n) return;
    const float a = y[j];
    if constexpr (BWD) out[j] = a <= 0.f ? 0.f : dy[j];
    else out[j] = a <= 0.f ? 0.f : a;
}

const VggNorm kVggNorm = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};      // vgg_arch.py:135-139
const VggNorm kNoNorm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};                          // use_input_norm = False: (x - 0) / 1 is exact

}  // namespace

// ================================================================ C ABI =========================
extern "C" int bem_vgg_prep_f32(const float* pred, const float* gt, float* xn, int B, int H, int W, int input_norm, int range_norm,
                                void* stream) {
    BEM_REQUIRE(pred && gt && xn, "vgg_prep: null tensor");
    BEM_REQUIRE(B >= 0 && H > 0 && W > 0, "vgg_prep: bad shape");
    const int64_t HW = (int64_t)H * W;
    if (B == 0) return BEM_OK;
    const bool vec = HW % 4 == 0 && host_aligned16(pred) && host_aligned16(gt) && host_aligned16(xn);
    const int64_t total = (int64_t)2 * B * 8 * (vec ? HW / 4 : HW);
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "vgg_prep: tensor too large");
    const VggNorm nm = input_norm ? kVggNorm : kNoNorm;
    if (vec) vgg_prep_kernel<true><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(pred, gt, xn, B, HW, nm, range_norm, total);
    else vgg_prep_kernel<false><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(pred, gt, xn, B, HW, nm, range_norm, total);
    return bem_check_launch("vgg_prep");
}

extern "C" int bem_vgg_prep_bwd_f32(const float* dxn, int64_t dxn_bstride, float* dpred, int B, int H, int W, int input_norm,
                                    int range_norm, void* stream) {
    BEM_REQUIRE(dxn && dpred, "vgg_prep_bwd: null tensor");
    BEM_REQUIRE(B >= 0 && H > 0 && W > 0, "vgg_prep_bwd: bad shape");
    const int64_t HW = (int64_t)H * W;
    BEM_REQUIRE(dxn_bstride >= 3 * HW, "vgg_prep_bwd: batch stride %lld below three planes", (long long)dxn_bstride);
    if (B == 0) return BEM_OK;
    const bool vec = HW % 4 == 0 && dxn_bstride % 4 == 0 && host_aligned16(dxn) && host_aligned16(dpred);
    const int64_t total = (int64_t)B * 3 * (vec ? HW / 4 : HW);
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "vgg_prep_bwd: tensor too large");
    const VggNorm nm = input_norm ? kVggNorm : kNoNorm;
    if (vec) vgg_prep_bwd_kernel<true><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(dxn, dxn_bstride, dpred, HW, nm, range_norm, total);
    else vgg_prep_bwd_kernel<false><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(dxn, dxn_bstride, dpred, HW, nm, range_norm, total);
    return bem_check_launch("vgg_prep_bwd");
}

extern "C" int bem_maxpool2_f32(const float* x, float* out, int64_t planes, int H, int W, void* stream) {
    BEM_REQUIRE(x && out, "maxpool2: null tensor");
    BEM_REQUIRE(planes >= 0 && H >= 2 && W >= 2, "maxpool2: planes of at least 2 x 2 required (got %d x %d)", H, W);
    if (planes == 0) return BEM_OK;
    const bool vec = W % 8 == 0 && host_aligned16(x) && host_aligned16(out);
    const int64_t total = planes * (H / 2) * (vec ? W / 8 : W / 2);
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "maxpool2: tensor too large");
    if (vec) maxpool2_kernel<true><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, H, W, total);
    else maxpool2_kernel<false><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, H, W, total);
    return bem_check_launch("maxpool2");
}

extern "C" int bem_relu_pool_bwd_f32(const float* y, const float* dpool, float* dy, int64_t planes, int H, int W, void* stream) {
    BEM_REQUIRE(y && dpool && dy, "relu_pool_bwd: null tensor");
    BEM_REQUIRE(y != dy && dpool != dy, "relu_pool_bwd: dy may not alias an input");
    BEM_REQUIRE(planes >= 0 && H >= 2 && W >= 2, "relu_pool_bwd: planes of at least 2 x 2 required (got %d x %d)", H, W);
    if (planes == 0) return BEM_OK;
    // W % 4 == 0: rows and the (W / 2)-wide rows of dpool start on 16 / 8 bytes when the tensors do
    const bool vec = W % 4 == 0 && host_aligned16(y) && host_aligned16(dy) && host_aligned16(dpool);
    const int64_t total = planes * (H / 2) * (vec ? W / 4 : W / 2);
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "relu_pool_bwd: tensor too large");
    if (vec) relu_pool_bwd_kernel<true><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(y, dpool, dy, H, W, total);
    else relu_pool_bwd_kernel<false><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(y, dpool, dy, H, W, total);
    return bem_check_launch("relu_pool_bwd");
}

static int relu_launch(bool bwd, const float* y, const float* dy, float* out, int64_t n, void* stream, const char* what) {
    BEM_REQUIRE(y && out && (!bwd || dy), "%s: null tensor", what);
    BEM_REQUIRE(n >= 0, "%s: bad size", what);
    if (n == 0) return BEM_OK;
    const bool vec = host_aligned16(y) && host_aligned16(out) && (!bwd || host_aligned16(dy));
    const int64_t nv = vec ? n / 4 : 0, total = nv + (n - 4 * nv);
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "%s: tensor too large", what);
    if (bwd) relu_kernel<true><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(y, dy, out, nv, n);
    else relu_kernel<false><<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(y, nullptr, out, nv, n);
    return bem_check_launch(what);
}

extern "C" int bem_relu_bwd_f32(const float* y, const float* dy, float* out, int64_t n, void* stream) {
    return relu_launch(true, y, dy, out, n, stream, "relu_bwd");
}

extern "C" int bem_relu_f32(const float* x, float* out, int64_t n, void* stream) {
    return relu_launch(false, x, nullptr, out, n, stream, "relu");
}
