// What runs around the convolutions of LPIPS v0.1 with the AlexNet trunk (Zhang et al. 2018; Enhancement/eval.py:143-145,301-306): the input
// stage (img_as_ubyte, im2tensor, the scaling layer) written straight into the operand of conv1, MaxPool2d(3, 2), and the distance head of
// one layer, and the backward of each of the three for the LPIPS loss term of the training step (the gradient of the second image alone;
// the convolutions' input gradients are convolutions again).  Every kernel writes each output element exactly once (no memset, no
// atomics), so a call repeats bit for bit.
//
// conv1 (11x11, stride 4, pad 2, 3 -> 64) runs as a 3x3 stride-1 pad-1 convolution of 48 channels on the x6 tap machinery (conv_x6.hip):
// the image, padded by 2, is cut into 4x4 blocks, block (by, bx) holds image pixel (4 by - 2 + dy, 4 bx - 2 + dx) of colour c in channel
// 16 c + 4 dy + dx, and the weight is zero-padded to 12x12 and cut the same way, so output pixel (oy, ox) of conv1 is output (oy + 1, ox + 1)
// of the block convolution.  The block image has Ho + 2 rows and Wo + 2 columns rounded up to even (the x6 form needs an even width).
#include "bem_common.h"

namespace {

struct LpipsScale { float shift[3], scale[3]; };
const LpipsScale kLpipsScale = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};      // lpips ScalingLayer

// xs (2B, 48, Hb, Wb): rows [0, B) from ref, [B, 2B) from pred.  One thread per output element; pixels outside the image are the zero
// padding of conv1 (zero after the scaling layer, as nn.Conv2d pads its own input).
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ ref, const float* __restrict__ pred, float* __restrict__ xs,
                                                         int B, int H, int W, int Hb, int Wb, LpipsScale sc, int mode, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int bx = (int)(i % Wb), by = (int)((i / Wb) % Hb);
    const int64_t pc = i / ((int64_t)Wb * Hb);
    const int ch = (int)(pc % 48), r = (int)(pc / 48);
    const int c = ch >> 4, y = 4 * by - 2 + ((ch >> 2) & 3), x = 4 * bx - 2 + (ch & 3);
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
        const int64_t HW = (int64_t)H * W;
        float t = (r < B ? ref + (int64_t)r * 3 * HW : pred + (int64_t)(r - B) * 3 * HW)[c * HW + (int64_t)y * W + x];
        if (mode == 1) t = bem_ubyte(t) / 127.5f - 1.f;         // im2tensor(img_as_ubyte(.))
        else if (mode == 2) t = 2.f * t - 1.f;                  // forward(normalize=True)
        v = (t - sc.shift[c]) / sc.scale[c];                    // true divisions: the f32 value numpy gives for the same expression
    }
    xs[i] = v;
}

// MaxPool2d(3, 2), floor, no padding: x (P, H, W) at plane stride x_ps and row stride x_rs -> out (P, Ho, Wo) contiguous.  torch's window
// walk (row-major from -inf, `val > max || isnan(val)`): a NaN in the window is the result.
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, int64_t x_ps, int64_t x_rs, float* __restrict__ out,
                                                         int Ho, int Wo, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
    const int64_t p = i / ((int64_t)Wo * Ho);
    const float* s = x + p * x_ps + (int64_t)(2 * oy) * x_rs + 2 * ox;
    float m = -INFINITY;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float v = s[ky * x_rs + kx];
            if (v > m || v != v) m = v;
        }
    out[i] = m;
}

// Distance head of one layer, first pass.  f (2B, C, h, w) at batch / channel / row strides; rows b and B + b are the two images.  A
// workgroup owns 64 consecutive pixels of image b (lane = pixel: the loads of a channel are contiguous) and its four waves a quarter of
// the channels each.  Everything in f64: the two channel norms (the waves' partial sums meet in LDS and are added in wave order), then
// sum_c lin[c] (y0 r0 - y1 r1)^2 with r = 1 / (|y| + 1e-10).  The workgroup's sum goes to part[b][blockIdx.x].
constexpr int LP_PX = 64;
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ f, int64_t f_bs, int64_t f_cs, int64_t f_rs,
                                                          const float* __restrict__ lin, double* __restrict__ part, int B, int C, int h, int w) {
    __shared__ double sh[4], nsh[2][4][LP_PX];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = blockIdx.x * LP_PX + lane;
    const bool live = px < h * w;
    const int pxc = live ? px : 0, y = pxc / w, x = pxc - y * w;
    const float* f0 = f + (int64_t)b * f_bs + (int64_t)y * f_rs + x;
    const float* f1 = f0 + (int64_t)B * f_bs;
    double n0 = 0.0, n1 = 0.0;
    for (int c = wave; c < C; c += 4) {
        const double a0 = f0[c * f_cs], a1 = f1[c * f_cs];
        n0 += a0 * a0;
        n1 += a1 * a1;
    }
    nsh[0][wave][lane] = n0;
    nsh[1][wave][lane] = n1;
    __syncthreads();
    n0 = nsh[0][0][lane] + nsh[0][1][lane] + nsh[0][2][lane] + nsh[0][3][lane];
    n1 = nsh[1][0][lane] + nsh[1][1][lane] + nsh[1][2][lane] + nsh[1][3][lane];
    const double r0 = 1.0 / (sqrt(n0) + 1e-10), r1 = 1.0 / (sqrt(n1) + 1e-10);
    double s = 0.0;
    for (int c = wave; c < C; c += 4) {
        double d;
        {
            // two rounded products: contracted into one fma, the difference of equal features would be the rounding error of one of them
#pragma clang fp contract(off)
            const double y0 = (double)f0[c * f_cs] * r0, y1 = (double)f1[c * f_cs] * r1;
            d = y0 - y1;
        }
        s += (double)lin[c] * d * d;
    }
    s = block_sum<4>(live ? s : 0.0, sh);
    if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = s;
}

// Second pass, one workgroup per image: the partials in a fixed order, the mean over pixels added to the f64 running sum acc[b] (started
// from zero when `first`), out[b] = that sum as f32.
__global__ __launch_bounds__(256) void lpips_layer_final_kernel(const double* __restrict__ part, int nblk, double npix, double* __restrict__ acc,
                                                                float* __restrict__ out, int first) {
    __shared__ double sh[4];
    const int b = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += part[(int64_t)b * nblk + i];
    s = block_sum<4>(s, sh);
    if (threadIdx.x == 0) {
        const double a = (first ? 0.0 : acc[b]) + s / npix;
        acc[b] = a;
        out[b] = (float)a;
    }
}

// ---------------------------------------------------------------- backward (the loss term) ------
// Head backward of one layer for the pred rows [B, 2B), in the forward's layout (lane = pixel, channels over the four waves).  With
// n = |y|, r = 1 / (n + 1e-10), a = y0 r0, b = y1 r1 and D_c = -2 lin_c (a_c - b_c), the gradient of the layer's distance with respect to
// the pred feature is g_k = r1 D_k - y1_k (r1 / n1) sum_c b_c D_c (the second term 0 where n1 = 0), times k = scale * gmul / (h w).  Three
// passes over the channels: the norms, sum_c b_c D_c, the write; the waves' partial sums meet in LDS and are added in wave order.
// dz (B, C, oh, ow) at its own strides takes (y1 > 0) ? gin + g : 0 -- the gradient at the convolution's output, before its ReLU -- at
// rows [oy0, oy0 + h) x columns [ox0, ox0 + w), and zero everywhere else (conv1's block grid around its crop).  A workgroup owns 64
// consecutive positions of that extent.
__global__ __launch_bounds__(256) void lpips_layer_bwd_kernel(const float* __restrict__ f, int64_t f_bs, int64_t f_cs, int64_t f_rs,
                                                              const float* __restrict__ lin, const float* __restrict__ gin,
                                                              const float* __restrict__ gmul, double scale, float* __restrict__ dz, int64_t d_bs,
                                                              int64_t d_cs, int64_t d_rs, int B, int C, int h, int w, int oh, int ow, int oy0,
                                                              int ox0) {
    __shared__ double nsh[3][4][LP_PX];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = blockIdx.x * LP_PX + lane;
    const bool inside = px < oh * ow;
    const int py = inside ? px / ow : 0, pxx = inside ? px - py * ow : 0;
    const int y = py - oy0, x = pxx - ox0;
    const bool live = inside && y >= 0 && y < h && x >= 0 && x < w;
    const int yc = live ? y : 0, xc = live ? x : 0;
    const float* f0 = f + (int64_t)b * f_bs + (int64_t)yc * f_rs + xc;
    const float* f1 = f0 + (int64_t)B * f_bs;
    double n0 = 0.0, n1 = 0.0;
    for (int c = wave; c < C; c += 4) {
        const double a0 = f0[c * f_cs], a1 = f1[c * f_cs];
        n0 += a0 * a0;
        n1 += a1 * a1;
    }
    nsh[0][wave][lane] = n0;
    nsh[1][wave][lane] = n1;
    __syncthreads();
    n0 = nsh[0][0][lane] + nsh[0][1][lane] + nsh[0][2][lane] + nsh[0][3][lane];
    n1 = nsh[1][0][lane] + nsh[1][1][lane] + nsh[1][2][lane] + nsh[1][3][lane];
    const double s1 = sqrt(n1);
    const double r0 = 1.0 / (sqrt(n0) + 1e-10), r1 = 1.0 / (s1 + 1e-10);
    // D_c of one channel; the two products stay two roundings (see the forward): equal images give D = 0 exactly
    auto bD = [&](int c, double& bc) {
#pragma clang fp contract(off)
        const double a = (double)f0[c * f_cs] * r0;
        bc = (double)f1[c * f_cs] * r1;
        const double d = a - bc;
        return -2.0 * (double)lin[c] * d;
    };
    double S = 0.0;
    for (int c = wave; c < C; c += 4) {
        double bc;
        const double D = bD(c, bc);
        S += bc * D;
    }
    nsh[2][wave][lane] = S;
    __syncthreads();
    S = nsh[2][0][lane] + nsh[2][1][lane] + nsh[2][2][lane] + nsh[2][3][lane];
    const double q = s1 > 0.0 ? r1 / s1 : 0.0;
    const double k = scale * (gmul ? (double)gmul[0] : 1.0) / ((double)h * (double)w);
    if (!inside) return;
    float* o = dz + (int64_t)b * d_bs + (int64_t)py * d_rs + pxx;
    const float* gi = gin ? gin + (int64_t)b * C * h * w + (int64_t)yc * w + xc : nullptr;
    for (int c = wave; c < C; c += 4) {
        float v = 0.f;
        const float y1 = f1[c * f_cs];
        if (live && y1 > 0.f) {
            double bc;
            const double D = bD(c, bc);
            const double g = (r1 * D - (double)y1 * q * S) * k;
            v = (float)(gi ? (double)gi[(int64_t)c * h * w] + g : g);
        }
        o[c * d_cs] = v;
    }
}

// Backward of MaxPool2d(3, 2) as a gather: y (P, H, W) at plane / row strides is the pool's input, dpool (P, Ho, Wo) the gradient of its
// output, dy (P, H, W) contiguous.  One thread per input pixel: each of the up to four windows that cover it is scanned again in the
// forward's order (row-major, `v > max || isnan(v)`, so the first maximum wins a tie, as in torch), and the pixel adds dpool of the windows
// it wins, rows first.  Rows and columns no window covers get 0.  The mask of the ReLU that made y is not applied here.
__global__ __launch_bounds__(256) void pool3s2_bwd_kernel(const float* __restrict__ y, int64_t y_ps, int64_t y_rs, const float* __restrict__ dpool,
                                                          float* __restrict__ dy, int H, int W, int Ho, int Wo, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H);
    const int64_t p = i / ((int64_t)W * H);
    const float* src = y + p * y_ps;
    const float* dp = dpool + p * (int64_t)Ho * Wo;
    const int oy_hi = min(Ho - 1, iy / 2), ox_hi = min(Wo - 1, ix / 2);
    float acc = 0.f;
    for (int oy = (iy - 1) / 2; oy <= oy_hi; ++oy)
        for (int ox = (ix - 1) / 2; ox <= ox_hi; ++ox) {
            const float* s = src + (int64_t)(2 * oy) * y_rs + 2 * ox;
            float m = -INFINITY;
            int am = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = s[ky * y_rs + kx];
                    if (v > m || v != v) m = v, am = ky * 3 + kx;
                }
            if (2 * oy + am / 3 == iy && 2 * ox + am % 3 == ix) acc += dp[(int64_t)oy * Wo + ox];
        }
    dy[i] = acc;
}

// Adjoint of lpips_prep_kernel for the pred rows: every image pixel sits in exactly one entry of the block layout, so dpred is a gather
// of gxs (B, 48, Hb, Wb), times the 2 of mode 2, divided by the scaling layer's scale (one true division, as the forward's).
__global__ __launch_bounds__(256) void lpips_prep_bwd_kernel(const float* __restrict__ gxs, float* __restrict__ dpred, int H, int W, int Hb, int Wb,
                                                             LpipsScale sc, float k, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int64_t bc = i / ((int64_t)W * H);
    const int c = (int)(bc % 3);
    const int64_t b = bc / 3;
    const int ch = 16 * c + 4 * ((y + 2) & 3) + ((x + 2) & 3);
    dpred[i] = (k * gxs[((b * 48 + ch) * Hb + ((y + 2) >> 2)) * Wb + ((x + 2) >> 2)]) / sc.scale[c];
}

// loss = weight * mean_b acc[b], acc the f64 running sums the last layer's head left in its workspace; one thread, a fixed order.
__global__ void lpips_mean_kernel(const double* __restrict__ acc, float* __restrict__ loss, int B, double weight) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += acc[b];
    loss[0] = (float)(weight * s / (double)B);
}

}  // namespace

// ================================================================ C ABI =========================
extern "C" int bem_lpips_prep_f32(const float* ref, const float* pred, float* xs, int B, int H, int W, int mode, void* stream) {
    BEM_REQUIRE(ref && pred && xs, "lpips_prep: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 32767 && mode >= 0 && mode <= 2, "lpips_prep: bad batch size %d or mode %d", B, mode);
    BEM_REQUIRE(H >= 31 && W >= 31, "lpips_prep: images of at least 31 x 31 required (got %d x %d)", H, W);
    if (B == 0) return BEM_OK;
    const int Hb = (H - 7) / 4 + 3, Wb = (((W - 7) / 4 + 3) + 1) & ~1;
    const int64_t total = (int64_t)2 * B * 48 * Hb * Wb;
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "lpips_prep: tensor too large");
    lpips_prep_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(ref, pred, xs, B, H, W, Hb, Wb, kLpipsScale, mode, total);
    return bem_check_launch("lpips_prep");
}

extern "C" int bem_maxpool3s2_f32(const float* x, int64_t x_pstride, int64_t x_rstride, float* out, int64_t planes, int H, int W, void* stream) {
    BEM_REQUIRE(x && out, "maxpool3s2: null tensor");
    BEM_REQUIRE(planes >= 0 && H >= 3 && W >= 3, "maxpool3s2: planes of at least 3 x 3 required (got %d x %d)", H, W);
    BEM_REQUIRE(x_rstride >= W && x_pstride >= (int64_t)(H - 1) * x_rstride + W, "maxpool3s2: strides %lld / %lld below a %d x %d plane",
                (long long)x_pstride, (long long)x_rstride, H, W);
    if (planes == 0) return BEM_OK;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const int64_t total = planes * Ho * Wo;
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "maxpool3s2: tensor too large");
    maxpool3s2_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(x, x_pstride, x_rstride, out, Ho, Wo, total);
    return bem_check_launch("maxpool3s2");
}

extern "C" int64_t bem_lpips_layer_ws_elems(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return (int64_t)B * (1 + cdiv64((int64_t)h * w, LP_PX));
}

extern "C" int bem_lpips_layer_f32(const float* feat, int64_t f_bstride, int64_t f_cstride, int64_t f_rstride, const float* lin, double* ws,
                                   int64_t ws_elems, float* out, int B, int C, int h, int w, int first, void* stream) {
    BEM_REQUIRE(feat && lin && ws && out, "lpips_layer: null tensor");
    BEM_REQUIRE(h >= 1 && w >= 1, "lpips_layer: planes of at least 1 x 1 required (got %d x %d)", h, w);
    BEM_REQUIRE(B >= 0 && B <= 32767 && C >= 1 && (int64_t)h * w < (1ll << 31) - 256, "lpips_layer: bad shape (B=%d C=%d)", B, C);
    BEM_REQUIRE(f_rstride >= w && f_cstride >= (int64_t)(h - 1) * f_rstride + w && f_bstride >= (int64_t)C * f_cstride,
                "lpips_layer: strides below a (%d, %d, %d) feature", C, h, w);
    if (B == 0) return BEM_OK;
    const int nblk = (int)cdiv64((int64_t)h * w, LP_PX);
    BEM_REQUIRE(ws_elems >= (int64_t)B * (1 + nblk), "lpips_layer: workspace of %lld doubles, need %lld", (long long)ws_elems,
                (long long)B * (1 + nblk));
    hipStream_t s = (hipStream_t)stream;
    double* part = ws + B;                  // ws[0, B): the running f64 sums over layers
    lpips_layer_kernel<<<dim3(nblk, B), 256, 0, s>>>(feat, f_bstride, f_cstride, f_rstride, lin, part, B, C, h, w);
    lpips_layer_final_kernel<<<B, 256, 0, s>>>(part, nblk, (double)h * (double)w, ws, out, first);
    return bem_check_launch("lpips_layer");
}

extern "C" int bem_lpips_mean_f32(const double* acc, float* loss, int B, float weight, void* stream) {
    BEM_REQUIRE(acc && loss, "lpips_mean: null tensor");
    BEM_REQUIRE(B >= 1 && B <= 32767, "lpips_mean: bad batch size %d", B);
    lpips_mean_kernel<<<1, 1, 0, (hipStream_t)stream>>>(acc, loss, B, (double)weight);
    return bem_check_launch("lpips_mean");
}

extern "C" int bem_lpips_layer_bwd_f32(const float* feat, int64_t f_bstride, int64_t f_cstride, int64_t f_rstride, const float* lin,
                                       const float* gin, const float* gmul, float scale, float* dz, int64_t d_bstride, int64_t d_cstride,
                                       int64_t d_rstride, int B, int C, int h, int w, int oh, int ow, int oy0, int ox0, void* stream) {
    BEM_REQUIRE(feat && lin && dz, "lpips_layer_bwd: null tensor");
    BEM_REQUIRE(B >= 1 && B <= 32767 && C >= 1 && h >= 1 && w >= 1, "lpips_layer_bwd: bad shape (B=%d C=%d h=%d w=%d)", B, C, h, w);
    BEM_REQUIRE(oy0 >= 0 && ox0 >= 0 && oh >= 1 && ow >= 1 && (int64_t)oy0 + h <= oh && (int64_t)ox0 + w <= ow &&
                    (int64_t)oh * ow < (1ll << 31) - 256,
                "lpips_layer_bwd: a %d x %d plane at (%d, %d) does not lie in a %d x %d output", h, w, oy0, ox0, oh, ow);
    BEM_REQUIRE(f_rstride >= w && f_cstride >= (int64_t)(h - 1) * f_rstride + w && f_bstride >= (int64_t)C * f_cstride,
                "lpips_layer_bwd: feature strides below a (%d, %d, %d) feature", C, h, w);
    BEM_REQUIRE(d_rstride >= ow && d_cstride >= (int64_t)(oh - 1) * d_rstride + ow && d_bstride >= (int64_t)C * d_cstride,
                "lpips_layer_bwd: output strides below a (%d, %d, %d) tensor", C, oh, ow);
    const int nblk = (int)cdiv64((int64_t)oh * ow, LP_PX);
    lpips_layer_bwd_kernel<<<dim3(nblk, B), 256, 0, (hipStream_t)stream>>>(feat, f_bstride, f_cstride, f_rstride, lin, gin, gmul, (double)scale,
                                                                          dz, d_bstride, d_cstride, d_rstride, B, C, h, w, oh, ow, oy0, ox0);
    return bem_check_launch("lpips_layer_bwd");
}

extern "C" int bem_relu_pool3s2_bwd_f32(const float* y, int64_t y_pstride, int64_t y_rstride, const float* dpool, float* dy, int64_t planes,
                                        int H, int W, void* stream) {
    BEM_REQUIRE(y && dpool && dy, "relu_pool3s2_bwd: null tensor");
    BEM_REQUIRE(planes >= 1 && H >= 3 && W >= 3, "relu_pool3s2_bwd: at least one plane of at least 3 x 3 required (got %lld of %d x %d)",
                (long long)planes, H, W);
    BEM_REQUIRE(y_rstride >= W && y_pstride >= (int64_t)(H - 1) * y_rstride + W, "relu_pool3s2_bwd: strides %lld / %lld below a %d x %d plane",
                (long long)y_pstride, (long long)y_rstride, H, W);
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    BEM_REQUIRE((int64_t)H * W < (1ll << 31) && planes < (1ll << 31), "relu_pool3s2_bwd: tensor too large");
    const int64_t total = planes * H * W;
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "relu_pool3s2_bwd: tensor too large");
    pool3s2_bwd_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(y, y_pstride, y_rstride, dpool, dy, H, W, Ho, Wo, total);
    return bem_check_launch("relu_pool3s2_bwd");
}

extern "C" int bem_lpips_prep_bwd_f32(const float* gxs, float* dpred, int B, int H, int W, int mode, void* stream) {
    BEM_REQUIRE(gxs && dpred, "lpips_prep_bwd: null tensor");
    BEM_REQUIRE(mode != 1, "lpips_prep_bwd: mode 1 (img_as_ubyte quantisation) is not differentiable; modes 0 and 2 have a backward");
    BEM_REQUIRE(B >= 1 && B <= 32767 && (mode == 0 || mode == 2), "lpips_prep_bwd: bad batch size %d or mode %d", B, mode);
    BEM_REQUIRE(H >= 31 && W >= 31, "lpips_prep_bwd: images of at least 31 x 31 required (got %d x %d)", H, W);
    const int Hb = (H - 7) / 4 + 3, Wb = (((W - 7) / 4 + 3) + 1) & ~1;
    BEM_REQUIRE((int64_t)H * W < (1ll << 31), "lpips_prep_bwd: tensor too large");
    const int64_t total = (int64_t)B * 3 * H * W;
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "lpips_prep_bwd: tensor too large");
    lpips_prep_bwd_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(gxs, dpred, H, W, Hb, Wb, kLpipsScale, mode == 2 ? 2.f : 1.f, total);
    return bem_check_launch("lpips_prep_bwd");
}
