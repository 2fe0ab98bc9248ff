// Bandwidth-bound layout kernels: plane transposes, channel copies / adds, bilinear up-sampling, space-to-depth and pixel shuffle,
// eval.py's image preparation (reflect pad, area down-size) and the 16-bit casts of the scan seam.
#include "bem_common.h"
#include "wavelet.h"

namespace {

// ---------------------------------------------------------------- layout helpers ------------
__global__ __launch_bounds__(256) void transpose_planes_kernel(const float* __restrict__ src, int64_t src_bs,
                                                               float* __restrict__ dst, int64_t dst_bs, int ppb,
                                                               int H, int W) {
    __shared__ float t[32][33];
    const int plane = blockIdx.z;
    const int bq = plane / ppb, pq = plane - bq * ppb;
    const int64_t HW = (int64_t)H * W;
    const float* s = src + (int64_t)bq * src_bs + (int64_t)pq * HW;
    float* d = dst + (int64_t)bq * dst_bs + (int64_t)pq * HW;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                   // clamped addresses: four loads in flight, then the LDS stores
        const int y = min(y0 + ty + 8 * k, H - 1), x = min(x0 + tx, W - 1);
        v[k] = s[(int64_t)y * W + x];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) t[ty + 8 * k][tx] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int x = x0 + ty + k, y = y0 + tx;    // dst is (W, H): row x, column y
        if (x < W && y < H) d[(int64_t)x * H + y] = t[tx][ty + k];
    }
}

__global__ void copy_channels_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                     int64_t dst_bs, int64_t CL, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int64_t b = i / CL, r = i - b * CL;
    dst[b * dst_bs + r] = src[b * src_bs + r];
}

// dst row b takes the channels of src row b / rep: an image's planes handed to its `rep` Monte-Carlo samples in one launch
__global__ void copy_channels_rep_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                         int64_t dst_bs, int64_t CL, int64_t total, int rep) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int64_t b = i / CL, r = i - b * CL;
    dst[b * dst_bs + r] = src[(b / rep) * src_bs + r];
}

__global__ void add_channels_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                    int64_t dst_bs, int64_t CL, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int64_t b = i / CL, r = i - b * CL;
    dst[b * dst_bs + r] += src[b * src_bs + r];
}

__global__ void bilinear_up_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                   int64_t dst_bs, int C, int H, int W, int s, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int Wo = W * s, Ho = H * s;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const int c = (int)((i / ((int64_t)Wo * Ho)) % C), b = (int)(i / ((int64_t)Wo * Ho * C));
    const float rs = 1.f / (float)s;
    const float* p = src + (int64_t)b * src_bs + (int64_t)c * H * W;
    dst[(int64_t)b * dst_bs + ((int64_t)c * Ho + yo) * Wo + xo] = bilinear_at(p, H, W, rs, yo, xo);
}

__global__ void space_to_depth_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W,
                                      int64_t total) {
    // out (B,4C,H/2,W/2): block q = dy + 2*dx  ->  [ee, oe, eo, oo]  (UNet_arch.py:74-78)
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int h2 = H >> 1, w2 = W >> 1;
    const int xx = (int)(i % w2), y = (int)((i / w2) % h2);
    const int cc = (int)((i / ((int64_t)w2 * h2)) % (4 * C)), b = (int)(i / ((int64_t)w2 * h2 * 4 * C));
    const int q = cc / C, c = cc - q * C;
    const int dy = q & 1, dx = q >> 1;
    out[i] = x[(((int64_t)b * C + c) * H + 2 * y + dy) * W + 2 * xx + dx];
}

__global__ void pixel_shuffle2_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W,
                                      int64_t total) {
    // out (B,C,2H,2W)[c][2y+i][2x+j] = x[c*4 + i*2 + j][y][x]
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int Wo = 2 * W, Ho = 2 * H;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const int c = (int)((i / ((int64_t)Wo * Ho)) % C), b = (int)(i / ((int64_t)Wo * Ho * C));
    const int ch = c * 4 + (yo & 1) * 2 + (xo & 1);
    out[i] = x[(((int64_t)b * 4 * C + ch) * H + (yo >> 1)) * W + (xo >> 1)];
}

// ---------------------------------------------------------------- eval.py image preparation --
// reflect-pad bottom/right to (Hp, Wp) (numpy 'reflect': edge pixel not repeated, eval.py:146-153) fused with the
// x1/s INTER_LINEAR condition (eval.py:174): for even s the bilinear taps of output (i, j) are the four pixels
// (s*i + s/2 - 1 .. s*i + s/2, s*j + s/2 - 1 .. s*j + s/2) of the padded image, weight 1/4 each.
__device__ __forceinline__ int reflect_idx(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

__global__ void pad_reflect_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int Hp, int Wp,
                                   int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int xo = (int)(i % Wp), yo = (int)((i / Wp) % Hp);
    const int64_t plane = i / ((int64_t)Wp * Hp);
    out[i] = x[(plane * H + reflect_idx(yo, H)) * W + reflect_idx(xo, W)];
}

__global__ void resize_down_kernel(const float* __restrict__ x, float* __restrict__ out, int Hp, int Wp, int s,
                                   int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int wd = Wp / s, hd = Hp / s;
    const int xo = (int)(i % wd), yo = (int)((i / wd) % hd);
    const int64_t plane = i / ((int64_t)wd * hd);
    const int a = s / 2 - 1;
    const float* p = x + (plane * Hp + (int64_t)yo * s + a) * Wp + (int64_t)xo * s + a;
    out[i] = 0.25f * (p[0] + p[Wp] + p[1] + p[Wp + 1]);
}

}  // namespace

// ================================================================ C ABI =========================
extern "C" int bem_transpose_planes_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride,
                                        int nbatch, int ppb, int H, int W, void* stream) {
    BEM_REQUIRE(src && dst, "transpose_planes: null tensor");
    BEM_REQUIRE(nbatch >= 0 && ppb > 0 && H > 0 && W > 0, "transpose_planes: bad shape");
    BEM_REQUIRE((int64_t)nbatch * ppb <= 65535 && cdiv(H, 32) <= 65535, "transpose_planes: too many planes (%lld)", (long long)nbatch * ppb);
    if (nbatch == 0) return BEM_OK;
    dim3 grid(cdiv(W, 32), cdiv(H, 32), nbatch * ppb);
    transpose_planes_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src, src_bstride, dst, dst_bstride, ppb, H, W);
    return bem_check_launch("transpose_planes");
}

extern "C" int bem_copy_channels_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride, int B,
                                     int C, int L, void* stream) {
    BEM_REQUIRE(src && dst, "copy_channels: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && L >= 0, "copy_channels: bad shape");
    const int64_t total = (int64_t)B * C * L;
    if (total == 0) return BEM_OK;
    copy_channels_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(src, src_bstride, dst, dst_bstride, (int64_t)C * L, total);
    return bem_check_launch("copy_channels");
}

extern "C" int bem_copy_channels_rep_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride, int B, int C, int L, int rep,
                                         void* stream) {
    BEM_REQUIRE(src && dst, "copy_channels_rep: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && L >= 0 && rep >= 1, "copy_channels_rep: bad shape");
    const int64_t total = (int64_t)B * C * L;
    if (total == 0) return BEM_OK;
    copy_channels_rep_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(src, src_bstride, dst, dst_bstride, (int64_t)C * L, total, rep);
    return bem_check_launch("copy_channels_rep");
}

extern "C" int bem_add_channels_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride, int B,
                                    int C, int L, void* stream) {
    BEM_REQUIRE(src && dst, "add_channels: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && L >= 0, "add_channels: bad shape");
    const int64_t total = (int64_t)B * C * L;
    if (total == 0) return BEM_OK;
    add_channels_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(src, src_bstride, dst, dst_bstride, (int64_t)C * L, total);
    return bem_check_launch("add_channels");
}

extern "C" int bem_bilinear_up_f32(const float* src, int64_t src_bstride, float* dst, int64_t dst_bstride, int B, int C,
                                   int H, int W, int s, void* stream) {
    BEM_REQUIRE(src && dst, "bilinear_up: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && s >= 1, "bilinear_up: bad shape");
    const int64_t total = (int64_t)B * C * H * W * s * s;
    if (total == 0) return BEM_OK;
    bilinear_up_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(src, src_bstride, dst, dst_bstride, C, H, W, s, total);
    return bem_check_launch("bilinear_up");
}

extern "C" int bem_space_to_depth_f32(const float* x, float* out, int B, int C, int H, int W, void* stream) {
    BEM_REQUIRE(x && out, "space_to_depth: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "space_to_depth: H, W must be even");
    const int64_t total = (int64_t)B * C * H * W;
    if (total == 0) return BEM_OK;
    space_to_depth_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, C, H, W, total);
    return bem_check_launch("space_to_depth");
}

extern "C" int bem_pixel_shuffle2_f32(const float* x, float* out, int B, int C, int H, int W, void* stream) {
    BEM_REQUIRE(x && out, "pixel_shuffle2: null tensor");
    BEM_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0, "pixel_shuffle2: bad shape");
    const int64_t total = (int64_t)B * C * H * W * 4;
    if (total == 0) return BEM_OK;
    pixel_shuffle2_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, C, H, W, total);
    return bem_check_launch("pixel_shuffle2");
}

extern "C" int bem_pad_reflect_f32(const float* x, float* out, int P, int H, int W, int Hp, int Wp, void* stream) {
    BEM_REQUIRE(x && out, "pad_reflect: null tensor");
    BEM_REQUIRE(P >= 0 && H > 0 && W > 0 && Hp >= H && Wp >= W && Hp - H < H && Wp - W < W, "pad_reflect: pad must be smaller than the image");
    const int64_t total = (int64_t)P * Hp * Wp;
    if (total == 0) return BEM_OK;
    pad_reflect_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, H, W, Hp, Wp, total);
    return bem_check_launch("pad_reflect");
}

extern "C" int bem_resize_down_f32(const float* x, float* out, int P, int Hp, int Wp, int s, void* stream) {
    BEM_REQUIRE(x && out, "resize_down: null tensor");
    BEM_REQUIRE(P >= 0 && s >= 2 && s % 2 == 0 && Hp > 0 && Wp > 0 && Hp % s == 0 && Wp % s == 0, "resize_down: even factor dividing H and W required");
    const int64_t total = (int64_t)P * (Hp / s) * (Wp / s);
    if (total == 0) return BEM_OK;
    resize_down_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, out, Hp, Wp, s, total);
    return bem_check_launch("resize_down");
}

// ------------------------------------------------------------------------------------------------
// 16-bit <-> float32 casts of the operator seam's backward (selective_scan_cuda_oflex.bwd with f16 / bf16 inputs): dtype 1 = float16,
// 2 = bfloat16 (round to nearest even on the way down, like torch's .to()).
// ------------------------------------------------------------------------------------------------
namespace {
__global__ void cast16_to_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n, int dtype) {
    const int64_t i = bem_gid1d();
    if (i >= n) return;
    const uint16_t b = src[i];
    dst[i] = dtype == 1 ? (float)__builtin_bit_cast(_Float16, b) : __builtin_bit_cast(float, (uint32_t)b << 16);
}
__global__ void cast_f32_to16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n, int dtype) {
    const int64_t i = bem_gid1d();
    if (i >= n) return;
    const float v = src[i];
    if (dtype == 1) {
        dst[i] = __builtin_bit_cast(uint16_t, (_Float16)v);
    } else {
        const uint32_t u = __builtin_bit_cast(uint32_t, v);
        dst[i] = (v != v) ? (uint16_t)0x7fc0 : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}
}  // namespace

extern "C" int bem_cast16_to_f32(const void* src, float* dst, int64_t n, int dtype, void* stream) {
    BEM_REQUIRE(src && dst && n >= 0 && (dtype == 1 || dtype == 2), "cast16_to_f32: bad arguments");
    if (n == 0) return BEM_OK;
    cast16_to_f32_kernel<<<GRID1D(n), 256, 0, (hipStream_t)stream>>>((const uint16_t*)src, dst, n, dtype);
    return bem_check_launch("cast16_to_f32");
}
extern "C" int bem_cast_f32_to16(const float* src, void* dst, int64_t n, int dtype, void* stream) {
    BEM_REQUIRE(src && dst && n >= 0 && (dtype == 1 || dtype == 2), "cast_f32_to16: bad arguments");
    if (n == 0) return BEM_OK;
    cast_f32_to16_kernel<<<GRID1D(n), 256, 0, (hipStream_t)stream>>>(src, (uint16_t*)dst, n, dtype);
    return bem_check_launch("cast_f32_to16");
}
