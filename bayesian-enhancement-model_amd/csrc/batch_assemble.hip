// One training batch from the device-resident uint8 image store (basicsr/data/paired_image_dataset.py:333-379 of the reference:
// padding, paired_random_crop, random_augmentation, add_label_noise, the x1/scale_down INTER_LINEAR condition planes, img2tensor),
// one launch per step.  The store is two byte arenas (lq, gt) of (H,W,3) RGB images at arbitrary byte offsets -- 37x53x3 is odd -- so
// the source is read byte by byte; every output element is written by exactly one thread (no memset, no atomics).
#include "bem_common.h"

namespace {

struct pix3 { float r, g, b; };

// symmetric padding index (numpy 'symmetric' = cv2.BORDER_REFLECT: the edge pixel is repeated); lands in [0, n) for any i
__device__ __forceinline__ int symm_idx(int i, int n) {
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// Output pixel (y, x) of a sample -> its source pixel in the padded image: flipud undone first, then rot90(k) (numpy, counter-clockwise):
// k=1: out[i][j] = A[j][w-1-i]; k=2: out[i][j] = A[h-1-i][w-1-j]; k=3: out[i][j] = A[h-1-j][i].  Rotating modes have Sh == Sw.
__device__ __forceinline__ int64_t src_byte(int64_t off, int H, int W, int top, int left, int mode, int Sh, int Sw, int y, int x) {
    if (mode & 1) y = Sh - 1 - y;
    int cy, cx;
    switch (mode >> 1) {
        case 0: cy = y; cx = x; break;
        case 1: cy = x; cx = Sw - 1 - y; break;
        case 2: cy = Sh - 1 - y; cx = Sw - 1 - x; break;
        default: cy = Sh - 1 - x; cx = y; break;
    }
    const int py = symm_idx(top + cy, H), px = symm_idx(left + cx, W);
    return off + ((int64_t)py * W + px) * 3;
}

__device__ __forceinline__ pix3 load_pix(const uint8_t* __restrict__ arena, int64_t at) {
    // imfrombytes(float32=True): uint8 -> float32, one correctly rounded division
    return {__fdiv_rn((float)arena[at], 255.f), __fdiv_rn((float)arena[at + 1], 255.f), __fdiv_rn((float)arena[at + 2], 255.f)};
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// utils/labelnoise.py:55-69 in RGB: temperature (float64 product, clipped, rounded to float32; blue * t, red / t), brightness, contrast
// (float32, each clipped).  Every operation is rounded on its own, so the full-size pixel and the taps of the down plane agree bit for bit.
__device__ __forceinline__ pix3 label_noise(pix3 p, float t, float b, float c, int steps) {
    // c * (x - 0.5) + 0.5 is a product rounded to f32 and then a sum, as numpy evaluates it: no fma (the pragma covers the operators
    // written in this body; an arithmetic helper from a header would bring its own contraction mode along)
#pragma clang fp contract(off)
    if (steps & 1) {
        const double td = (double)t;
        p.r = (float)fmin(fmax((double)p.r * (1.0 / td), 0.0), 1.0);
        p.b = (float)fmin(fmax((double)p.b * td, 0.0), 1.0);
        p.g = clip01(p.g);
    }
    if (steps & 2) {
        p.r = clip01(p.r * b); p.g = clip01(p.g * b); p.b = clip01(p.b * b);
    }
    if (steps & 4) {
        const float r = c * (p.r - 0.5f), g = c * (p.g - 0.5f), bl = c * (p.b - 0.5f);
        p.r = clip01(r + 0.5f); p.g = clip01(g + 0.5f); p.b = clip01(bl + 0.5f);
    }
    return p;
}

struct sample {
    int64_t off;
    int H, W, top, left, mode;
    float t, b, c;
};

__device__ __forceinline__ sample read_sample(const int64_t* __restrict__ table, int n_img, const int32_t* __restrict__ plan,
                                              const float* __restrict__ noise, int j) {
    sample s;
    const int img = min(max(plan[4 * j], 0), n_img - 1);       // the host checked the rows; a stale device copy must still stay inside the store
    s.off = table[3 * img]; s.H = (int)table[3 * img + 1]; s.W = (int)table[3 * img + 2];
    s.top = max(plan[4 * j + 1], 0); s.left = max(plan[4 * j + 2], 0); s.mode = plan[4 * j + 3] & 7;
    s.t = noise ? noise[3 * j] : 1.f; s.b = noise ? noise[3 * j + 1] : 1.f; s.c = noise ? noise[3 * j + 2] : 1.f;
    return s;
}

// threads [0, B*Sh*Sw): one full-size pixel of lq and gt (three channels each); threads behind them: one pixel of the two down planes,
// 0.25f * (p[0] + p[W] + p[1] + p[W+1]) at taps s/2-1, s/2 of the finished crop (the sum order of resize_down_kernel).
__global__ void batch_assemble_kernel(const uint8_t* __restrict__ lq_arena, const uint8_t* __restrict__ gt_arena,
                                      const int64_t* __restrict__ table, int n_img, const int32_t* __restrict__ plan,
                                      const float* __restrict__ noise, int steps, int Sh, int Sw, int s,
                                      float* __restrict__ lq, float* __restrict__ gt, float* __restrict__ lq_down,
                                      float* __restrict__ gt_down, int64_t nfull, int64_t total) {
    int64_t i = bem_gid1d();
    if (i >= total) return;
    if (i < nfull) {
        const int x = (int)(i % Sw), y = (int)((i / Sw) % Sh), j = (int)(i / ((int64_t)Sw * Sh));
        const sample sm = read_sample(table, n_img, plan, noise, j);
        const int64_t at = src_byte(sm.off, sm.H, sm.W, sm.top, sm.left, sm.mode, Sh, Sw, y, x);
        const pix3 a = load_pix(lq_arena, at);
        pix3 g = load_pix(gt_arena, at);
        if (steps) g = label_noise(g, sm.t, sm.b, sm.c, steps);
        const int64_t plane = (int64_t)Sh * Sw, o = (int64_t)j * 3 * plane + (int64_t)y * Sw + x;
        lq[o] = a.r; lq[o + plane] = a.g; lq[o + 2 * plane] = a.b;
        gt[o] = g.r; gt[o + plane] = g.g; gt[o + 2 * plane] = g.b;
        return;
    }
    i -= nfull;
    const int hd = Sh / s, wd = Sw / s;
    const int xo = (int)(i % wd), yo = (int)((i / wd) % hd), j = (int)(i / ((int64_t)wd * hd));
    const sample sm = read_sample(table, n_img, plan, noise, j);
    const int y0 = yo * s + s / 2 - 1, x0 = xo * s + s / 2 - 1;
    pix3 a[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                               // p[0], p[W], p[1], p[W+1]
        const int64_t at = src_byte(sm.off, sm.H, sm.W, sm.top, sm.left, sm.mode, Sh, Sw, y0 + (k & 1), x0 + (k >> 1));
        a[k] = load_pix(lq_arena, at);
        g[k] = load_pix(gt_arena, at);
        if (steps) g[k] = label_noise(g[k], sm.t, sm.b, sm.c, steps);
    }
    const int64_t plane = (int64_t)hd * wd, o = (int64_t)j * 3 * plane + (int64_t)yo * wd + xo;
    lq_down[o] = 0.25f * (a[0].r + a[1].r + a[2].r + a[3].r);
    lq_down[o + plane] = 0.25f * (a[0].g + a[1].g + a[2].g + a[3].g);
    lq_down[o + 2 * plane] = 0.25f * (a[0].b + a[1].b + a[2].b + a[3].b);
    gt_down[o] = 0.25f * (g[0].r + g[1].r + g[2].r + g[3].r);
    gt_down[o + plane] = 0.25f * (g[0].g + g[1].g + g[2].g + g[3].g);
    gt_down[o + 2 * plane] = 0.25f * (g[0].b + g[1].b + g[2].b + g[3].b);
}

}  // namespace

// ================================================================ C ABI =========================
extern "C" int bem_batch_assemble_u8(const uint8_t* lq_arena, const uint8_t* gt_arena, int64_t arena_bytes,
                                     const int64_t* table_host, const int64_t* table_dev, int n_img,
                                     const int32_t* plan_host, const int32_t* plan_dev, const float* noise_dev, int noise_steps,
                                     int B, int Sh, int Sw, int s,
                                     float* lq, float* gt, float* lq_down, float* gt_down, void* stream) {
    BEM_REQUIRE(lq_arena && gt_arena && table_host && table_dev && plan_host && plan_dev, "batch_assemble: null store or plan");
    BEM_REQUIRE(lq && gt, "batch_assemble: null output");
    BEM_REQUIRE(s == 0 ? (!lq_down && !gt_down) : (lq_down && gt_down), "batch_assemble: the down planes go with scale_down != 0 only");
    BEM_REQUIRE(B > 0 && B <= 65535 && Sh > 0 && Sw > 0 && Sh <= 16384 && Sw <= 16384, "batch_assemble: batch %d, crop %dx%d out of range", B, Sh, Sw);
    BEM_REQUIRE(s == 0 || (s >= 2 && s % 2 == 0 && Sh % s == 0 && Sw % s == 0), "batch_assemble: scale_down %d must be even and divide the crop %dx%d", s, Sh, Sw);
    BEM_REQUIRE(n_img > 0 && arena_bytes > 0, "batch_assemble: empty store");
    BEM_REQUIRE(noise_steps >= 0 && noise_steps <= 7 && (noise_steps == 0 || noise_dev), "batch_assemble: label-noise steps %d need a factor table", noise_steps);
    for (int i = 0; i < n_img; ++i) {
        const int64_t off = table_host[3 * i], H = table_host[3 * i + 1], W = table_host[3 * i + 2];
        BEM_REQUIRE(H > 0 && W > 0 && H <= 65535 && W <= 65535 && off >= 0 && off <= arena_bytes - H * W * 3,
                    "batch_assemble: image %d (offset %lld, %lldx%lld) outside the store of %lld bytes", i, (long long)off, (long long)H,
                    (long long)W, (long long)arena_bytes);
    }
    for (int j = 0; j < B; ++j) {
        const int32_t img = plan_host[4 * j], top = plan_host[4 * j + 1], left = plan_host[4 * j + 2], mode = plan_host[4 * j + 3];
        BEM_REQUIRE(img >= 0 && img < n_img, "batch_assemble: plan row %d names image %d of %d", j, img, n_img);
        const int64_t H = table_host[3 * img + 1], W = table_host[3 * img + 2];
        BEM_REQUIRE(mode >= 0 && mode <= 7, "batch_assemble: plan row %d has mode %d", j, mode);
        BEM_REQUIRE(!((mode >> 1) & 1) || Sh == Sw, "batch_assemble: plan row %d rotates (mode %d) a %dx%d crop", j, mode, Sh, Sw);
        BEM_REQUIRE(top >= 0 && top <= (H > Sh ? H : Sh) - Sh && left >= 0 && left <= (W > Sw ? W : Sw) - Sw,
                    "batch_assemble: plan row %d crops at (%d, %d) outside image %d (%lldx%lld, crop %dx%d)", j, top, left, img, (long long)H,
                    (long long)W, Sh, Sw);
    }
    const int64_t nfull = (int64_t)B * Sh * Sw, total = nfull + (s ? (int64_t)B * (Sh / s) * (Sw / s) : 0);
    BEM_REQUIRE(cdiv64(total, 256) <= 0x7fffffffLL, "batch_assemble: batch too large for one launch");
    batch_assemble_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(lq_arena, gt_arena, table_dev, n_img, plan_dev, noise_dev, noise_steps,
                                                                          Sh, Sw, s, lq, gt, lq_down, gt_down, nfull, total);
    return bem_check_launch("batch_assemble");
}
