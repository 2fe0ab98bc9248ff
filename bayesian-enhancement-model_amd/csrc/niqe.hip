// NIQE (basicsr/metrics/niqe.py, as Enhancement/eval.py:248-254 calls it: calculate_niqe(pred * 255, crop_border=0)) for a batch
// of candidates, entirely on the device: Y channel + round + crop fused with the 7x7 MSCN, block statistics + AGGD fits, the
// antialiased x0.5 MATLAB-bicubic resize as two passes, MSCN and block fits again at scale 2, and the per-candidate MVG distance.
// Every reduction runs in a fixed order (no float atomics): a score is bit-reproducible and independent of the batch around it.
#include "bem_common.h"

// numpy evaluates each f32 / f64 operation on its own: no fused multiply-adds anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int NQ_BS = 96;        // block size at scale 1 (48 at scale 2)
constexpr int NQ_TH = 16;        // MSCN output tile: 16 rows x 64 columns per 256-thread workgroup
constexpr int NQ_TW = 64;
constexpr int NQ_NF = 36;        // features per block row (18 per scale)
constexpr int NQ_MAX_ROWS = 8192;

// Y of YCbCr on the stored channel order, as metric_util.to_y_channel + color_util.bgr2ycbcr see it (they assume BGR, eval.py passes
// RGB, so the B weight multiplies R): t = f32(f32(p * 255) / 255), y = f64 dot + 16, / 255 -> f32, * 255 -> f32, round half to even.
__device__ __forceinline__ float niqe_luma(const float* __restrict__ rgb, int64_t plane, int64_t off) {
    const float r = rgb[off], g = rgb[plane + off], b = rgb[2 * plane + off];
    const float tr = (r * 255.f) / 255.f, tg = (g * 255.f) / 255.f, tb = (b * 255.f) / 255.f;
    const double y = (((double)tr * 24.966 + (double)tg * 128.553) + (double)tb * 65.481) + 16.0;
    const float y32 = (float)(y / 255.0);
    return rintf(y32 * 255.f);
}

// MSCN of niqe.py: mu = convolve(img, win, 'nearest'), sigma = sqrt(|convolve(img^2, win) - mu^2|), n = (img - mu) / (sigma + 1).
// scipy.ndimage accumulates in f64 and stores f32; borders replicate the (cropped) plane's edge.  FROM_RGB: the plane is the rounded Y
// of the top-left H x W crop of `src` (Bn,3,h,w), and is also written to `yout` for the resize; otherwise `src` is an (Bn,H,W) plane.
template <bool FROM_RGB>
__global__ __launch_bounds__(256) void niqe_mscn_kernel(const float* __restrict__ src, float* __restrict__ yout, float* __restrict__ nout,
                                                        const double* __restrict__ win, int h, int w, int H, int W) {
    __shared__ float tile[NQ_TH + 6][NQ_TW + 6];
    __shared__ double wk[49];
    const int t = threadIdx.x, b = blockIdx.z;
    const int ty0 = blockIdx.y * NQ_TH, tx0 = blockIdx.x * NQ_TW;
    if (t < 49) wk[t] = win[48 - t];                 // convolve = correlate with the flipped window
    for (int i = t; i < (NQ_TH + 6) * (NQ_TW + 6); i += 256) {
        const int r = i / (NQ_TW + 6), c = i % (NQ_TW + 6);
        const int gy = min(max(ty0 + r - 3, 0), H - 1), gx = min(max(tx0 + c - 3, 0), W - 1);
        float v;
        if constexpr (FROM_RGB) v = niqe_luma(src + (int64_t)b * 3 * h * w, (int64_t)h * w, (int64_t)gy * w + gx);
        else v = src[((int64_t)b * H + gy) * W + gx];
        tile[r][c] = v;
    }
    __syncthreads();
    const int c = t % NQ_TW, gx = tx0 + c;
    if (gx >= W) return;
#pragma unroll 1
    for (int r = t / NQ_TW; r < NQ_TH; r += 256 / NQ_TW) {
        const int gy = ty0 + r;
        if (gy >= H) break;
        double m = 0.0, s = 0.0;
#pragma unroll
        for (int k = 0; k < 49; ++k) {
            const float v = tile[r + k / 7][c + k % 7];
            m += wk[k] * (double)v;
            s += wk[k] * (double)(v * v);
        }
        const float v = tile[r + 3][c + 3];
        const float mu = (float)m, s32 = (float)s;
        const float sig = sqrtf(fabsf(s32 - mu * mu));
        const int64_t o = ((int64_t)b * H + gy) * W + gx;
        nout[o] = (v - mu) / (sig + 1.f);
        if constexpr (FROM_RGB) yout[o] = v;
    }
}

// imresize(img / 255, 0.5, antialiasing=True) of matlab_functions.py, H pass: out[o][x] = sum_k wt[o][k] * in[ix[o][k]][x] (the symmetric
// padding is folded into the host-built index table), f32 result.
__global__ __launch_bounds__(256) void niqe_resize_h_kernel(const float* __restrict__ y, float* __restrict__ out, const float* __restrict__ wt,
                                                            const int* __restrict__ ix, int K, int H, int W, int Ho, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int x = (int)(i % W), o = (int)((i / W) % Ho);
    const int64_t b = i / ((int64_t)W * Ho);
    const float* p = y + b * H * W + x;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += (double)wt[o * K + k] * (double)(p[(int64_t)ix[o * K + k] * W] / 255.f);
    out[i] = (float)acc;
}

// W pass, then * 255 (niqe.py's img * 255.) in f32.
__global__ __launch_bounds__(256) void niqe_resize_w_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ wt,
                                                            const int* __restrict__ ix, int K, int W, int Wo, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int o = (int)(i % Wo);
    const float* p = in + (i / Wo) * W;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += (double)wt[o * K + k] * (double)p[ix[o * K + k]];
    out[i] = (float)acc * 255.f;
}

// compute_feature of one block: the AGGD fit (estimate_aggd_param) of the block and of its four paired products with
// np.roll(block, s) (wrapping inside the block), s in (0,1), (1,0), (1,1), (1,-1).  One workgroup per (block, scale, candidate);
// blocks are numbered idx_w-major like niqe.py's loops.  alpha = gam[argmin((r_gam - rhatnorm)^2)] by a brute-force scan of the
// table that keeps np.argmin's semantics: first index on ties, index 0 when rhatnorm is NaN (a block without negative or positive values).
__global__ __launch_bounds__(256) void niqe_feature_kernel(const float* __restrict__ n1, const float* __restrict__ n2, const double* __restrict__ tab,
                                                           int ntab, double* __restrict__ feat, int Hc, int Wc, int nbh, int nb) {
    __shared__ float blk[NQ_BS * NQ_BS];
    __shared__ double part[25][4];
    __shared__ double tot[25];
    __shared__ double bestv[5][4];
    __shared__ int besti[5][4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int row = blockIdx.x, scale = blockIdx.y, b = blockIdx.z;
    const int BS = scale ? NQ_BS / 2 : NQ_BS, H = scale ? Hc / 2 : Hc, W = scale ? Wc / 2 : Wc;
    const float* plane = (scale ? n2 : n1) + (int64_t)b * H * W;
    const int y0 = (row % nbh) * BS, x0 = (row / nbh) * BS;
    for (int i = t; i < BS * BS; i += 256) blk[i] = plane[(int64_t)(y0 + i / BS) * W + x0 + i % BS];
    __syncthreads();
    // per signal: sum v^2 over v < 0, count v < 0, sum v^2 over v > 0, count v > 0, sum |v|
    double acc[25];
#pragma unroll
    for (int q = 0; q < 25; ++q) acc[q] = 0.0;
    for (int p = t; p < BS * BS; p += 256) {
        const int i = p / BS, j = p % BS;
        const float x = blk[p];
        const int im = (i == 0 ? BS : i) - 1, jm = (j == 0 ? BS : j) - 1, jp = (j == BS - 1 ? 0 : j + 1);
        const float v[5] = {x, x * blk[i * BS + jm], x * blk[im * BS + j], x * blk[im * BS + jm], x * blk[im * BS + jp]};
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const double sq = (double)(v[s] * v[s]);
            if (v[s] < 0.f) { acc[5 * s + 0] += sq; acc[5 * s + 1] += 1.0; }
            if (v[s] > 0.f) { acc[5 * s + 2] += sq; acc[5 * s + 3] += 1.0; }
            acc[5 * s + 4] += (double)fabsf(v[s]);
        }
    }
#pragma unroll
    for (int q = 0; q < 25; ++q) {
        const double r = wave_sum(acc[q]);
        if (lane == 0) part[q][wv] = r;
    }
    __syncthreads();
    if (t < 25) tot[t] = ((part[t][0] + part[t][1]) + part[t][2]) + part[t][3];
    __syncthreads();
    const double n = (double)(BS * BS);
    double rn[5], bv[5];
    int bi[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const double lstd = sqrt(tot[5 * s + 0] / tot[5 * s + 1]), rstd = sqrt(tot[5 * s + 2] / tot[5 * s + 3]);
        const double g = lstd / rstd;
        const double ma = tot[5 * s + 4] / n;
        const double rhat = (ma * ma) / ((tot[5 * s + 0] + tot[5 * s + 2]) / n);
        rn[s] = (rhat * (g * g * g + 1.0) * (g + 1.0)) / ((g * g + 1.0) * (g * g + 1.0));
        bv[s] = __builtin_nan("");
        bi[s] = t;
    }
    const double* r_gam = tab + ntab;
    for (int k = t; k < ntab; k += 256) {
        const double r = r_gam[k];
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const double d = r - rn[s], e = d * d;
            if (k == t || e < bv[s]) { bv[s] = e; bi[s] = k; }
        }
    }
    // (value, index) minimum: the other side wins only if strictly smaller, or equal with a lower index; NaN never wins
#pragma unroll
    for (int s = 0; s < 5; ++s) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double ov = __shfl_xor(bv[s], d, BEM_WAVE);
            const int oi = __shfl_xor(bi[s], d, BEM_WAVE);
            if (ov < bv[s] || (ov == bv[s] && oi < bi[s])) { bv[s] = ov; bi[s] = oi; }
        }
        if (lane == 0) { bestv[s][wv] = bv[s]; besti[s][wv] = bi[s]; }
    }
    __syncthreads();
    if (t >= 5) return;
    const int s = t;
    double v = bestv[s][0];
    int k = besti[s][0];
    for (int w2 = 1; w2 < 4; ++w2)
        if (bestv[s][w2] < v || (bestv[s][w2] == v && besti[s][w2] < k)) { v = bestv[s][w2]; k = besti[s][w2]; }
    const double alpha = tab[k], bfac = tab[2 * ntab + k], g21 = tab[3 * ntab + k];
    const double bl = sqrt(tot[5 * s + 0] / tot[5 * s + 1]) * bfac, br = sqrt(tot[5 * s + 2] / tot[5 * s + 3]) * bfac;
    double* f = feat + ((int64_t)b * nb + row) * NQ_NF + scale * 18;
    if (s == 0) {
        f[0] = alpha; f[1] = (bl + br) / 2.0;
    } else {
        f += 2 + 4 * (s - 1);
        f[0] = alpha; f[1] = (br - bl) * g21; f[2] = bl; f[3] = br;
    }
}

// The MVG fit and distance of niqe.py, one wave per candidate: mu_d = nanmean over all rows, cov_d = np.cov (ddof 1) over the NaN-free
// rows, q = sqrt(d^T ((cov_pris + cov_d) / 2)^-1 d) with d = mu_pris - mu_d.  The matrix is SPD (cov_pris SPD, cov_d PSD), so pinv is
// the inverse and q = |L^-1 d| for its Cholesky factor L.  Fewer than 2 NaN-free rows, or a pivot that is not positive: NaN.
__global__ __launch_bounds__(64) void niqe_mvg_kernel(const double* __restrict__ feat, const double* __restrict__ mu_pris,
                                                      const double* __restrict__ cov_pris, double* __restrict__ scores, int nb) {
    __shared__ unsigned char clean[NQ_MAX_ROWS];
    __shared__ double A[NQ_NF][NQ_NF + 1];
    __shared__ double mud[NQ_NF], mc[NQ_NF], d[NQ_NF];
    __shared__ int ncl_s, bad_s;
    const int t = threadIdx.x, b = blockIdx.x;
    const double* F = feat + (int64_t)b * nb * NQ_NF;
    int mine = 0;
    for (int r = t; r < nb; r += 64) {
        bool ok = true;
        for (int c = 0; c < NQ_NF; ++c) ok = ok && !isnan(F[(int64_t)r * NQ_NF + c]);
        clean[r] = ok;
        mine += ok;
    }
    mine = wave_sum(mine);
    if (t == 0) { ncl_s = mine; bad_s = 0; }
    __syncthreads();
    const int ncl = ncl_s;
    if (ncl < 2) {
        if (t == 0) scores[b] = __builtin_nan("");
        return;
    }
    if (t < NQ_NF) {
        double s = 0.0, k = 0.0, sc = 0.0;
        for (int r = 0; r < nb; ++r) {
            const double v = F[(int64_t)r * NQ_NF + t];
            if (!isnan(v)) { s += v; k += 1.0; }
            if (clean[r]) sc += v;
        }
        mud[t] = s / k;
        mc[t] = sc / (double)ncl;
        d[t] = mu_pris[t] - mud[t];
    }
    __syncthreads();
    for (int e = t; e < NQ_NF * NQ_NF; e += 64) {
        const int i = e / NQ_NF, j = e % NQ_NF;
        double s = 0.0;
        for (int r = 0; r < nb; ++r)
            if (clean[r]) s += (F[(int64_t)r * NQ_NF + i] - mc[i]) * (F[(int64_t)r * NQ_NF + j] - mc[j]);
        A[i][j] = (cov_pris[e] + s / (double)(ncl - 1)) / 2.0;
    }
    __syncthreads();
    // right-looking Cholesky (lower triangle), then the forward solve L y = d in place of d
    for (int k = 0; k < NQ_NF; ++k) {
        if (t == 0) {
            const double p = A[k][k];
            if (!(p > 0.0)) bad_s = 1;
            A[k][k] = sqrt(p);
        }
        __syncthreads();
        if (t > k && t < NQ_NF) A[t][k] /= A[k][k];
        __syncthreads();
        const int m = NQ_NF - 1 - k;
        for (int e = t; e < m * m; e += 64) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) A[i][j] -= A[i][k] * A[j][k];
        }
        __syncthreads();
    }
    for (int k = 0; k < NQ_NF; ++k) {
        if (t == 0) d[k] /= A[k][k];
        __syncthreads();
        if (t > k && t < NQ_NF) d[t] -= A[t][k] * d[k];
        __syncthreads();
    }
    if (t == 0) {
        double q = 0.0;
        for (int k = 0; k < NQ_NF; ++k) q += d[k] * d[k];
        scores[b] = bad_s ? __builtin_nan("") : sqrt(q);
    }
}

struct NiqeLayout {
    int Hc, Wc, nbh, nb;
    int64_t y1, n1, t1, y2, n2, feat, total;   // byte offsets into the workspace
};

NiqeLayout niqe_layout(int Bn, int h, int w) {
    NiqeLayout L;
    L.nbh = h / NQ_BS;
    L.Hc = L.nbh * NQ_BS;
    L.Wc = (w / NQ_BS) * NQ_BS;
    L.nb = L.nbh * (w / NQ_BS);
    auto up = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    const int64_t p1 = (int64_t)Bn * L.Hc * L.Wc * 4, p2 = (int64_t)Bn * (L.Hc / 2) * (L.Wc / 2) * 4;
    L.y1 = 0;
    L.n1 = L.y1 + up(p1);
    L.t1 = L.n1 + up(p1);
    L.y2 = L.t1 + up((int64_t)Bn * (L.Hc / 2) * L.Wc * 4);
    L.n2 = L.y2 + up(p2);
    L.feat = L.n2 + up(p2);
    L.total = L.feat + up((int64_t)Bn * L.nb * NQ_NF * 8);
    return L;
}

}  // namespace

extern "C" int64_t bem_niqe_ws_bytes(int Bn, int h, int w) {
    if (Bn < 1 || h < NQ_BS || w < NQ_BS) return 0;
    return niqe_layout(Bn, h, w).total;
}

extern "C" int bem_niqe_f32(const float* final, const double* mu_pris, const double* cov_pris, const double* window, const double* gam_tab,
                            int ntab, const float* rs_wh, const int* rs_ih, int kh, const float* rs_ww, const int* rs_iw, int kw,
                            double* scores, void* ws, int64_t ws_bytes, int Bn, int h, int w, void* stream) {
    BEM_REQUIRE(final && mu_pris && cov_pris && window && gam_tab && rs_wh && rs_ih && rs_ww && rs_iw && scores && ws, "niqe: null tensor");
    BEM_REQUIRE(h >= NQ_BS && w >= NQ_BS, "niqe: images must be at least 96 x 96 (got %d x %d): NIQE needs one 96 x 96 block", h, w);
    BEM_REQUIRE(Bn >= 1 && Bn <= 65535 && ntab >= 1 && kh >= 1 && kw >= 1 && h <= 65535 && w <= 65535, "niqe: bad arguments");
    const NiqeLayout L = niqe_layout(Bn, h, w);
    BEM_REQUIRE(L.nb <= NQ_MAX_ROWS, "niqe: at most %d blocks of 96 x 96 per image", NQ_MAX_ROWS);
    BEM_REQUIRE(ws_bytes >= L.total, "niqe: workspace of %lld bytes, %lld needed (bem_niqe_ws_bytes)", (long long)ws_bytes, (long long)L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    float *y1 = (float*)(base + L.y1), *n1 = (float*)(base + L.n1), *t1 = (float*)(base + L.t1), *y2 = (float*)(base + L.y2), *n2 = (float*)(base + L.n2);
    double* feat = (double*)(base + L.feat);
    const int H2 = L.Hc / 2, W2 = L.Wc / 2;
    niqe_mscn_kernel<true><<<dim3(cdiv(L.Wc, NQ_TW), cdiv(L.Hc, NQ_TH), Bn), 256, 0, s>>>(final, y1, n1, window, h, w, L.Hc, L.Wc);
    const int64_t nh = (int64_t)Bn * H2 * L.Wc, nw = (int64_t)Bn * H2 * W2;
    niqe_resize_h_kernel<<<GRID1D(nh), 256, 0, s>>>(y1, t1, rs_wh, rs_ih, kh, L.Hc, L.Wc, H2, nh);
    niqe_resize_w_kernel<<<GRID1D(nw), 256, 0, s>>>(t1, y2, rs_ww, rs_iw, kw, L.Wc, W2, nw);
    niqe_mscn_kernel<false><<<dim3(cdiv(W2, NQ_TW), cdiv(H2, NQ_TH), Bn), 256, 0, s>>>(y2, nullptr, n2, window, 0, 0, H2, W2);
    niqe_feature_kernel<<<dim3(L.nb, 2, Bn), 256, 0, s>>>(n1, n2, gam_tab, ntab, feat, L.Hc, L.Wc, L.nbh, L.nb);
    niqe_mvg_kernel<<<Bn, 64, 0, s>>>(feat, mu_pris, cov_pris, scores, L.nb);
    return bem_check_launch("niqe");
}
