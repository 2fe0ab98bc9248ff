// UIQM and UCIQE (basicsr/metrics/uciqe_uiqm.py, as Enhancement/eval.py:255-260 calls them) for a batch of candidates, entirely on the
// device: img_as_ubyte + OpenCV's 8-bit RGB -> Lab + UCIQE's per-pixel sums, Pillow's fixed-point bicubic resize to width 256 as two passes
// (the second also builds the UICM histograms), the Sobel maxima, the EME / UIConM block terms, UCIQE's chroma-variance pass, and a
// per-candidate finish.  Every float reduction runs in a fixed order (integer atomics only): a score is bit-reproducible and independent of
// the batch around it.
#include "bem_common.h"

// numpy evaluates each f32 / f64 operation on its own: no fused multiply-adds anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int UQ_TILE = 4096;     // pixels per workgroup of the full-resolution passes
constexpr int UQ_W = 256;         // eval.py:257: resized width
constexpr int UQ_WIN = 10;        // eme / _uiconm window
constexpr int UQ_PREC = 22;       // Pillow Resample.c PRECISION_BITS
constexpr int UQ_NRG = 511, UQ_NYB = 1021;
// per-candidate integer counters, zeroed by the call: L histogram, R-G histogram, 2 (Y-B) histogram, max dx^2 + dy^2 per channel
constexpr int UQ_CL = 0, UQ_CRG = 256, UQ_CYB = UQ_CRG + UQ_NRG, UQ_CMAX = UQ_CYB + UQ_NYB, UQ_NCNT = UQ_CMAX + 4;
constexpr int UQ_NLAB = 256 + 3072 + 9;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// img_as_ubyte (eval.py:257,260) + cv2.cvtColor(RGB2LAB) (getUCIQE :45) per pixel; UCIQE's per-pixel terms chr = hypot(a, b) and
// sat = chr / sqrt(chr^2 + lum^2) (:51-53, a and b keep the +128 offset) summed per tile in f64; L levels counted.
// tab: sRGB gamma x 255 x 8 (256), 2^15 f(x) at x = i / 2040 (3072), the 3 x 3 fixed-point XYZ matrix (OpenCV 4.x RGB2Lab_b).
__global__ __launch_bounds__(256) void uiqm_quant_lab_kernel(const float* __restrict__ final, const int* __restrict__ tab, uint8_t* __restrict__ q,
                                                             uint8_t* __restrict__ lab, int* __restrict__ cnt, double* __restrict__ part,
                                                             int64_t hw, int ntiles) {
    __shared__ int lt[UQ_NLAB];
    __shared__ int hist[256];
    __shared__ double red[2][4];
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    for (int i = t; i < UQ_NLAB; i += 256) lt[i] = tab[i];
    hist[t] = 0;
    __syncthreads();
    const int* gam = lt;
    const int* cbrt = lt + 256;
    const int* C = lt + 256 + 3072;
    const float* src = final + (int64_t)b * 3 * hw;
    uint8_t* qo = q + (int64_t)b * 3 * hw;
    uint8_t* lo = lab + (int64_t)b * 3 * hw;
    double sc = 0.0, ss = 0.0;
    for (int k = 0; k < UQ_TILE / 256; ++k) {
        const int64_t p = (int64_t)tile * UQ_TILE + k * 256 + t;
        if (p >= hw) break;
        int u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u[c] = (int)rintf(fminf(fmaxf(src[c * hw + p], 0.f), 1.f) * 255.f);      // img_as_ubyte: rint(255 x), half to even
            qo[c * hw + p] = (uint8_t)u[c];
        }
        const int R = gam[u[0]], G = gam[u[1]], B = gam[u[2]];
        const int fX = cbrt[min(descale(R * C[0] + G * C[1] + B * C[2], 12), 3071)];
        const int fY = cbrt[min(descale(R * C[3] + G * C[4] + B * C[5], 12), 3071)];
        const int fZ = cbrt[min(descale(R * C[6] + G * C[7] + B * C[8], 12), 3071)];
        const int L = sat8(descale(296 * fY - 1336935, 15));
        const int A = sat8(descale(500 * (fX - fY) + (128 << 15), 15));
        const int Bb = sat8(descale(200 * (fY - fZ) + (128 << 15), 15));
        lo[p] = (uint8_t)L; lo[hw + p] = (uint8_t)A; lo[2 * hw + p] = (uint8_t)Bb;
        atomicAdd(&hist[L], 1);
        const double lum = (double)L / 255.0, a = (double)A / 255.0, bb = (double)Bb / 255.0;
        const double chr = sqrt(a * a + bb * bb);
        sc += chr;
        ss += chr / sqrt(chr * chr + lum * lum);
    }
    sc = wave_sum(sc);
    ss = wave_sum(ss);
    if ((t & 63) == 0) { red[0][t >> 6] = sc; red[1][t >> 6] = ss; }
    __syncthreads();
    if (t < 2) part[((int64_t)b * ntiles + tile) * 2 + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
    if (hist[t]) atomicAdd(&cnt[(int64_t)b * UQ_NCNT + UQ_CL + t], hist[t]);
}

// Pillow's ImagingResampleHorizontal_8bpc: out = clip8((2^21 + sum_t in[x0 + t] k[t]) >> 22), uint8.  bounds (n_out, 2) = first source
// index and tap count, k (n_out, K) the fixed-point weights (host-built, both within the source row).
__device__ __forceinline__ uint8_t pil_tap_sum(const uint8_t* __restrict__ src, int64_t stride, const int* __restrict__ bounds,
                                               const int* __restrict__ k, int K, int o) {
    const int x0 = bounds[2 * o], n = bounds[2 * o + 1];
    int acc = 1 << (UQ_PREC - 1);
    for (int i = 0; i < n; ++i) acc += (int)src[(int64_t)(x0 + i) * stride] * k[o * K + i];
    return (uint8_t)min(max(acc >> UQ_PREC, 0), 255);
}

__global__ __launch_bounds__(256) void uiqm_resize_h_kernel(const uint8_t* __restrict__ q, uint8_t* __restrict__ out, const int* __restrict__ bounds,
                                                            const int* __restrict__ k, int K, int h, int w, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int x = (int)(i % UQ_W);
    const int64_t row = i / UQ_W;                   // (b * 3 + c) * h + y
    out[i] = pil_tap_sum(q + row * w, 1, bounds, k, K, x);
}

// Vertical pass (ImagingResampleVertical_8bpc) of the three channels of one pixel, then the UICM histograms of the resized image
// (_uicm :328-333): RG = R - G in [-255, 255], 2 YB = R + G - 2 B in [-510, 510], both exact.
__global__ __launch_bounds__(256) void uiqm_resize_v_kernel(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ rs, const int* __restrict__ bounds,
                                                            const int* __restrict__ k, int K, int h, int Hr, int* __restrict__ cnt) {
    __shared__ int hist[UQ_NRG + UQ_NYB];
    const int t = threadIdx.x, b = blockIdx.y;
    for (int i = t; i < UQ_NRG + UQ_NYB; i += 256) hist[i] = 0;
    __syncthreads();
    const int64_t np_ = (int64_t)Hr * UQ_W;
    const int64_t p = (int64_t)blockIdx.x * 256 + t;
    if (p < np_) {
        const int y = (int)(p / UQ_W), x = (int)(p % UQ_W);
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = pil_tap_sum(tmp + ((int64_t)b * 3 + c) * h * UQ_W + x, UQ_W, bounds, k, K, y);
            rs[((int64_t)b * 3 + c) * np_ + p] = (uint8_t)v[c];
        }
        atomicAdd(&hist[v[0] - v[1] + 255], 1);
        atomicAdd(&hist[UQ_NRG + v[0] + v[1] - 2 * v[2] + 510], 1);
    }
    __syncthreads();
    for (int i = t; i < UQ_NRG + UQ_NYB; i += 256)
        if (hist[i]) atomicAdd(&cnt[(int64_t)b * UQ_NCNT + UQ_CRG + i], hist[i]);
}

// scipy.ndimage.sobel(x, 0) and (x, 1) at one pixel of an (H, 256) uint8 plane, mode 'reflect' (the edge sample repeats): dx^2 + dy^2,
// exact in int (|d| <= 1020).
__device__ __forceinline__ int sobel_m2(const uint8_t* __restrict__ P, int H, int y, int x) {
    const int ym = max(y - 1, 0), yp = min(y + 1, H - 1), xm = max(x - 1, 0), xp = min(x + 1, UQ_W - 1);
    auto at = [&](int yy, int xx) { return (int)P[yy * UQ_W + xx]; };
    const int d0 = (at(yp, xm) - at(ym, xm)) + 2 * (at(yp, x) - at(ym, x)) + (at(yp, xp) - at(ym, xp));
    const int d1 = (at(ym, xp) - at(ym, xm)) + 2 * (at(y, xp) - at(y, xm)) + (at(yp, xp) - at(yp, xm));
    return d0 * d0 + d1 * d1;
}

// max over the plane of dx^2 + dy^2 per channel (np.max(mag) of sobel :347 is the hypot of it: hypot is monotone)
__global__ __launch_bounds__(256) void uiqm_sobel_max_kernel(const uint8_t* __restrict__ rs, int Hr, int* __restrict__ cnt) {
    const int b = blockIdx.y;
    const int64_t np_ = (int64_t)Hr * UQ_W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int m = p < np_ ? sobel_m2(rs + ((int64_t)b * 3 + c) * np_, Hr, (int)(p / UQ_W), (int)(p % UQ_W)) : 0;
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&cnt[(int64_t)b * UQ_NCNT + UQ_CMAX + c], m);
    }
}

// One wave per 10 x 10 block (i, j) of the nx x ny grid (nx = Hr / 10, ny = 25).
// EME (eme :377-398 on np.multiply(sobel(ch), ch), _uism :431-454): the block is extended to the plane's end in the last row / column of
// blocks; edge = f32(f32(mag * f32(255 / max mag)) * ch) with mag = hypotf(dx, dy); term = f32(f32(2 / (nx ny)) * log(f32(max / min))),
// 0 where min or max is 0, NaN for a plane without edges (255 / 0 = inf, 0 * inf = NaN, as numpy).  The log is the correctly rounded
// f32 log (through f64).  -> eme_t (Bn, 3, nx ny), row-major blocks.
// UIConM (_uiconm :488-522): the 10 x 10 x 3 block itself (the image is cropped to whole blocks); top = max - min, bot = max + min;
// term = q log q in f64 with q = f32(top / bot), 0 where top or bot is 0.  -> ucm_t (Bn, nx ny), column-major blocks (the reference's
// loop order).
__global__ __launch_bounds__(256) void uiqm_blocks_kernel(const uint8_t* __restrict__ rs, const int* __restrict__ cnt, float* __restrict__ eme_t,
                                                          double* __restrict__ ucm_t, int Hr, int nx, int ny) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int id = blockIdx.x * 4 + (threadIdx.x >> 6), nb = nx * ny;
    if (id >= nb) return;                           // whole waves only; no barriers below
    const int i = id / ny, j = id % ny;
    const int r0 = i * UQ_WIN, r1 = i < nx - 1 ? r0 + UQ_WIN : Hr;
    const int c0 = j * UQ_WIN, c1 = j < ny - 1 ? c0 + UQ_WIN : UQ_W;
    const int bw = c1 - c0, npx = (r1 - r0) * bw;
    const int64_t np_ = (int64_t)Hr * UQ_W;
    float scale[3], mn[3], mx[3];
    int mx2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mx2[c] = cnt[(int64_t)b * UQ_NCNT + UQ_CMAX + c];
        scale[c] = 255.f / (float)sqrt((double)mx2[c]);
        mn[c] = __builtin_inff();
        mx[c] = -__builtin_inff();
    }
    int umn = 255, umx = 0;
    for (int e = lane; e < npx; e += 64) {
        const int y = r0 + e / bw, x = c0 + e % bw;
        const bool inner = y < r0 + UQ_WIN && x < c0 + UQ_WIN;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* P = rs + ((int64_t)b * 3 + c) * np_;
            const int v = P[y * UQ_W + x];
            const float mag = (float)sqrt((double)sobel_m2(P, Hr, y, x));
            const float edge = (mag * scale[c]) * (float)v;
            mn[c] = fminf(mn[c], edge);
            mx[c] = fmaxf(mx[c], edge);
            if (inner) { umn = min(umn, v); umx = max(umx, v); }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { mn[c] = wave_min(mn[c]); mx[c] = wave_max(mx[c]); }
    umn = wave_min(umn);
    umx = wave_max(umx);
    if (lane != 0) return;
    const float w = (float)(2.0 / (double)nb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float term;
        if (mx2[c] == 0) term = __builtin_nanf("");
        else if (mn[c] == 0.f || mx[c] == 0.f) term = 0.f;
        else term = w * (float)log((double)(mx[c] / mn[c]));
        eme_t[((int64_t)b * 3 + c) * nb + id] = term;
    }
    const float top = (float)(umx - umn), bot = (float)(umx + umn);
    double u = 0.0;
    if (top != 0.f && bot != 0.f) {
        const double qd = (double)(top / bot);
        u = qd * log(qd);
    }
    ucm_t[(int64_t)b * nb + j * nx + i] = u;
}

// UCIQE's chroma term (getUCIQE :55-57): aver_chr = mean(chr) from the first pass's tile sums, then per tile sum |1 - (aver_chr / chr)^2|.
__global__ __launch_bounds__(256) void uiqm_uciqe_var_kernel(const uint8_t* __restrict__ lab, const double* __restrict__ part,
                                                             double* __restrict__ vpart, int64_t hw, int ntiles) {
    __shared__ double sh_mean, red[4];
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    if (t < 64) {
        double s = 0.0;
        for (int i = t; i < ntiles; i += 64) s += part[((int64_t)b * ntiles + i) * 2];
        s = wave_sum(s);
        if (t == 0) sh_mean = s / (double)hw;
    }
    __syncthreads();
    const double m = sh_mean;
    const uint8_t* A = lab + ((int64_t)b * 3 + 1) * hw;
    const uint8_t* Bp = lab + ((int64_t)b * 3 + 2) * hw;
    double s = 0.0;
    for (int k = 0; k < UQ_TILE / 256; ++k) {
        const int64_t p = (int64_t)tile * UQ_TILE + k * 256 + t;
        if (p >= hw) break;
        const double a = (double)A[p] / 255.0, bb = (double)Bp[p] / 255.0;
        const double r = m / sqrt(a * a + bb * bb);
        s += fabs(1.0 - r * r);
    }
    s = wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) vpart[(int64_t)b * ntiles + tile] = ((red[0] + red[1]) + red[2]) + red[3];
}

// mu_a :302-320 from a histogram: the float32 sum of sorted[T_L + 1 : K - T_R] in ascending order (Python's sum over np.float32), times
// f32(1 / (K - T_L - T_R)).  A run of n equal values is added at once while every partial sum of the run stays within f32's exact range
// for multiples of 1/2 (both ends of the run within |s| <= 2^23: the f32 sum is then the exact sum); otherwise it is added value by value in f32, as the reference does.
__device__ float trimmed_mean(const int* __restrict__ h, int nbins, int off, float step, int K) {
    const int tl = (int)ceil(0.1 * (double)K), tr = (int)floor(0.1 * (double)K);
    const int64_t s0 = tl + 1, e0 = K - tr;
    const float weight = (float)(1.0 / (double)(K - tl - tr));
    float s = 0.f;
    int64_t cum = 0;
    for (int i = 0; i < nbins && cum < e0; ++i) {
        const int64_t c = h[i];
        const int64_t n = min(cum + c, e0) - max(cum, s0);
        cum += c;
        if (n <= 0) continue;
        const float v = (float)(i - off) * step;
        const double end = (double)s + (double)n * (double)v;
        if (fabs((double)s) <= 8388608.0 && fabs(end) <= 8388608.0) {
            s = (float)end;
        } else {
            for (int64_t r = 0; r < n; ++r) s = s + v;
        }
    }
    return weight * s;
}

// s_a :322-326: mean over all K pixels of (f32(x - mu))^2 in f64, from the histogram (bins in ascending order)
__device__ double trimmed_var(const int* __restrict__ h, int nbins, int off, float step, float mu, int K) {
    double s = 0.0;
    for (int i = 0; i < nbins; ++i) {
        if (!h[i]) continue;
        const double d = (double)((float)(i - off) * step - mu);
        s += (double)h[i] * (d * d);
    }
    return s / (double)K;
}

// np.histogram(lum, 65536) bin of lum = x (numpy _histograms_impl: index from the scaled offset, then corrected against the linspace edges
// edge_i = i * step + first, edge_65536 = last)
__device__ int np_hist_bin(double x, double first, double last) {
    const double step = (last - first) / 65536.0;
    int i = (int)(((x - first) / (last - first)) * 65536.0);
    if (i == 65536) i -= 1;
    auto edge = [&](int e) { return e == 65536 ? last : (double)e * step + first; };
    if (x < edge(i)) i -= 1;
    if (x >= edge(i + 1) && i != 65535) i += 1;
    return i;
}

// One wave per candidate: UICM from the histograms, the f32 EME sums (eme :398, row-major blocks), the f64 UIConM sum (column-major), UIQM
// with NumPy 2's float32 promotion (getUIQM :532-536: c2 * uism is f32, so is every sum with it); UCIQE's three terms and total (:52-76).
// parts (Bn, 8): uicm, uism, uiconm, uiqm, var_chr, con_lum, aver_sat, uciqe.
__global__ __launch_bounds__(64) void uiqm_final_kernel(const int* __restrict__ cnt, const float* __restrict__ eme_t, const double* __restrict__ ucm_t,
                                                        const double* __restrict__ part, const double* __restrict__ vpart, double* __restrict__ parts,
                                                        double* __restrict__ uiqm, double* __restrict__ uciqe, int Hr, int nb, int64_t hw, int ntiles) {
    __shared__ float mu[2], eme[3];
    __shared__ double sa[2], ucm, conl;
    const int t = threadIdx.x, b = blockIdx.x;
    const int* C = cnt + (int64_t)b * UQ_NCNT;
    const int K = Hr * UQ_W;
    if (t < 2) mu[t] = t == 0 ? trimmed_mean(C + UQ_CRG, UQ_NRG, 255, 1.f, K) : trimmed_mean(C + UQ_CYB, UQ_NYB, 510, 0.5f, K);
    else if (t < 5) {
        const float* e = eme_t + ((int64_t)b * 3 + (t - 2)) * nb;
        float s = 0.f;
        for (int i = 0; i < nb; ++i) s = s + e[i];
        eme[t - 2] = s;
    } else if (t == 5) {
        const double* u = ucm_t + (int64_t)b * nb;
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += u[i];
        ucm = (-1.0 / (double)nb) * s;
    } else if (t == 6) {
        const int* L = C + UQ_CL;
        int lo = 0, hi = 255;
        while (!L[lo]) ++lo;
        while (!L[hi]) --hi;
        double first = (double)lo / 255.0, last = (double)hi / 255.0;
        if (first == last) { first -= 0.5; last += 0.5; }
        const double n = (double)hw;
        int64_t c = 0;
        int ilow = -1, ihigh = -1;
        for (int v = lo; v <= hi && ihigh < 0; ++v) {
            if (!L[v]) continue;
            c += L[v];
            const double cdf = (double)c / n;
            if (ilow < 0 && cdf > 0.01) ilow = np_hist_bin((double)v / 255.0, first, last);
            if (ihigh < 0 && cdf >= 0.99) ihigh = np_hist_bin((double)v / 255.0, first, last);
        }
        conl = (double)(ihigh - 1) / 65535.0 - (double)(ilow - 1) / 65535.0;
    }
    __syncthreads();
    if (t < 2) sa[t] = t == 0 ? trimmed_var(C + UQ_CRG, UQ_NRG, 255, 1.f, mu[0], K) : trimmed_var(C + UQ_CYB, UQ_NYB, 510, 0.5f, mu[1], K);
    __syncthreads();
    double sat = 0.0, var = 0.0;
    {
        double s1 = 0.0, s2 = 0.0;
        for (int i = t; i < ntiles; i += 64) {
            s1 += part[((int64_t)b * ntiles + i) * 2 + 1];
            s2 += vpart[(int64_t)b * ntiles + i];
        }
        sat = wave_sum(s1) / (double)hw;
        var = sqrt(wave_sum(s2) / (double)hw);
    }
    if (t != 0) return;
    const double m0 = (double)mu[0], m1 = (double)mu[1];
    const double uicm = (-0.0268 * sqrt(m0 * m0 + m1 * m1)) + (0.1586 * sqrt(sa[0] + sa[1]));
    const float uism = ((0.299f * eme[0]) + (0.587f * eme[1])) + (0.144f * eme[2]);
    float q = (float)(0.0282 * uicm) + 0.2953f * uism;
    q = q + (float)(3.5753 * ucm);
    const double uc = ((0.4680 * var) + (0.2745 * conl)) + (0.2576 * sat);
    double* P = parts + (int64_t)b * 8;
    P[0] = uicm; P[1] = (double)uism; P[2] = ucm; P[3] = (double)q;
    P[4] = var; P[5] = conl; P[6] = sat; P[7] = uc;
    uiqm[b] = (double)q;
    uciqe[b] = uc;
}

struct UiqmLayout {
    int Hr, nx, ny, nb, ntiles;
    int64_t parts, rs, lab, q, tmp, cnt, part, vpart, eme, ucm, total;   // byte offsets into the workspace
};

UiqmLayout uiqm_layout(int Bn, int h, int w, int Hr) {
    UiqmLayout L;
    L.Hr = Hr;
    L.nx = Hr / UQ_WIN;
    L.ny = UQ_W / UQ_WIN;
    L.nb = L.nx * L.ny;
    const int64_t hw = (int64_t)h * w;
    L.ntiles = (int)cdiv64(hw, UQ_TILE);
    auto up = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    L.parts = 0;
    L.rs = L.parts + up((int64_t)Bn * 8 * 8);
    L.lab = L.rs + up((int64_t)Bn * 3 * Hr * UQ_W);
    L.q = L.lab + up((int64_t)Bn * 3 * hw);
    L.tmp = L.q + up((int64_t)Bn * 3 * hw);
    L.cnt = L.tmp + up((int64_t)Bn * 3 * h * UQ_W);
    L.part = L.cnt + up((int64_t)Bn * UQ_NCNT * 4);
    L.vpart = L.part + up((int64_t)Bn * L.ntiles * 2 * 8);
    L.eme = L.vpart + up((int64_t)Bn * L.ntiles * 8);
    L.ucm = L.eme + up((int64_t)Bn * 3 * L.nb * 4);
    L.total = L.ucm + up((int64_t)Bn * L.nb * 8);
    return L;
}

}  // namespace

extern "C" int64_t bem_uiqm_ws_bytes(int Bn, int h, int w, int Hr) {
    if (Bn < 1 || h < 1 || w < 1 || Hr < UQ_WIN) return 0;
    return uiqm_layout(Bn, h, w, Hr).total;
}

extern "C" int bem_uiqm_uciqe_f32(const float* final, const int* lab_tab, const int* rs_bh, const int* rs_kh, int kh, const int* rs_bv,
                                  const int* rs_kv, int kv, double* uiqm, double* uciqe, void* ws, int64_t ws_bytes, int Bn, int h, int w, int Hr,
                                  void* stream) {
    BEM_REQUIRE(final && lab_tab && rs_bh && rs_kh && rs_bv && rs_kv && uiqm && uciqe && ws, "uiqm_uciqe: null tensor");
    BEM_REQUIRE(Hr >= UQ_WIN, "uiqm_uciqe: the image resized to width 256 must be at least 10 rows high (got %d rows from %d x %d): UIQM needs "
                "one 10 x 10 block", Hr, h, w);
    BEM_REQUIRE(Bn >= 1 && Bn <= 65535 && h >= 1 && w >= 1 && h <= 65535 && w <= 65535 && Hr <= 65535 && kh >= 1 && kv >= 1,
                "uiqm_uciqe: bad arguments");
    BEM_REQUIRE((int64_t)h * w <= ((int64_t)1 << 31) / 4, "uiqm_uciqe: images of at most 2^29 pixels");
    const UiqmLayout L = uiqm_layout(Bn, h, w, Hr);
    BEM_REQUIRE(ws_bytes >= L.total, "uiqm_uciqe: workspace of %lld bytes, %lld needed (bem_uiqm_ws_bytes)", (long long)ws_bytes, (long long)L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    double* parts = (double*)(base + L.parts);
    uint8_t *rs = (uint8_t*)(base + L.rs), *lab = (uint8_t*)(base + L.lab), *q = (uint8_t*)(base + L.q), *tmp = (uint8_t*)(base + L.tmp);
    int* cnt = (int*)(base + L.cnt);
    double *part = (double*)(base + L.part), *vpart = (double*)(base + L.vpart), *ucm = (double*)(base + L.ucm);
    float* eme = (float*)(base + L.eme);
    const int64_t hw = (int64_t)h * w, nrs = (int64_t)Hr * UQ_W, ntmp = (int64_t)Bn * 3 * h * UQ_W;
    if (hipMemsetAsync(cnt, 0, (size_t)Bn * UQ_NCNT * 4, s) != hipSuccess) return bem_check_launch("uiqm_uciqe: memset");
    uiqm_quant_lab_kernel<<<dim3(L.ntiles, Bn), 256, 0, s>>>(final, lab_tab, q, lab, cnt, part, hw, L.ntiles);
    uiqm_resize_h_kernel<<<GRID1D(ntmp), 256, 0, s>>>(q, tmp, rs_bh, rs_kh, kh, h, w, ntmp);
    uiqm_resize_v_kernel<<<dim3((unsigned)cdiv64(nrs, 256), Bn), 256, 0, s>>>(tmp, rs, rs_bv, rs_kv, kv, h, Hr, cnt);
    uiqm_sobel_max_kernel<<<dim3((unsigned)cdiv64(nrs, 256), Bn), 256, 0, s>>>(rs, Hr, cnt);
    uiqm_blocks_kernel<<<dim3(cdiv(L.nb, 4), Bn), 256, 0, s>>>(rs, cnt, eme, ucm, Hr, L.nx, L.ny);
    uiqm_uciqe_var_kernel<<<dim3(L.ntiles, Bn), 256, 0, s>>>(lab, part, vpart, hw, L.ntiles);
    uiqm_final_kernel<<<Bn, 64, 0, s>>>(cnt, eme, ucm, part, vpart, parts, uiqm, uciqe, Hr, L.nb, hw, L.ntiles);
    return bem_check_launch("uiqm_uciqe");
}
