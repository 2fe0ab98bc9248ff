// Bandwidth-bound helpers: quaternion/Haar primitives, channel-attention statistics + weight folding,
// layout shuffles, bilinear resampling, Bayesian weight sampling, Monte-Carlo loop reductions.
#include "bem_common.h"
#include <algorithm>

thread_local char bem_err_buf[512] = "";
extern "C" const char* bem_last_error(void) { return bem_err_buf; }
extern "C" int bem_abi_version(void) { return 1; }

namespace {

#define GRID1D(n) dim3((unsigned)cdiv64((n), 256))

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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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

__device__ __forceinline__ void iwt4(float ll, float hl, float lh, float hh, float (&o)[4]) {
    // o[0]=(even row, even col) o[1]=(odd row, even col) o[2]=(even, odd) o[3]=(odd, odd)  (model4.py:26-35)
    ll /= 2; hl /= 2; lh /= 2; hh /= 2;
    o[0] = ll - hl - lh + hh;
    o[1] = ll - hl + lh - hh;
    o[2] = ll + hl - lh - hh;
    o[3] = ll + hl + lh + hh;
}

__global__ void iwt_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W, int64_t total) {
    // x (B,4C,H,W) -> out (B,C,2H,2W); one thread per input pixel and channel
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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

// ---------------------------------------------------------------- channel attention ----------
// stats[b] = { S[32][32] = F1 F2^T, s1[32] = F1 1, s2[32] = F2 1 } accumulated in f64.
constexpr int ATT_C = 32;
constexpr int ATT_CHUNK = 2048;
__global__ __launch_bounds__(256) void attn_stats_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                                                         double* __restrict__ stats, int L) {
    __shared__ double t1[ATT_C][65], t2[ATT_C][65];     // converted once when the tile is staged: the product loop is then f64 FMAs only (it was
                                                        // 4 v_cvt_f64_f32 per 4 FMAs: the conversions, not the arithmetic, set the kernel's time)
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * ATT_CHUNK;
    const int i0 = (threadIdx.x >> 4) * 2, j0 = (threadIdx.x & 15) * 2;
    double a00 = 0, a01 = 0, a10 = 0, a11 = 0, r0 = 0, r1 = 0, c0 = 0, c1 = 0;
    const float* F1 = f1 + (int64_t)b * ATT_C * L;
    const float* F2 = f2 + (int64_t)b * ATT_C * L;
    const int pend = min(p0 + ATT_CHUNK, L);
    for (int ps = p0; ps < pend; ps += 64) {
        __syncthreads();
        for (int i = threadIdx.x; i < ATT_C * 64; i += 256) {
            const int c = i >> 6, pp = i & 63;
            const int p = ps + pp;
            t1[c][pp] = p < pend ? (double)F1[(int64_t)c * L + p] : 0.0;
            t2[c][pp] = p < pend ? (double)F2[(int64_t)c * L + p] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int pp = 0; pp < 64; ++pp) {
            const double u0 = t1[i0][pp], u1 = t1[i0 + 1][pp], v0 = t2[j0][pp], v1 = t2[j0 + 1][pp];
            a00 = fma(u0, v0, a00); a01 = fma(u0, v1, a01); a10 = fma(u1, v0, a10); a11 = fma(u1, v1, a11);
            if (j0 == 0) { r0 += u0; r1 += u1; }
            if (i0 == 0) { c0 += v0; c1 += v1; }
        }
    }
    double* S = stats + (int64_t)b * (ATT_C * ATT_C + 2 * ATT_C);
    atomicAdd(&S[i0 * ATT_C + j0], a00);
    atomicAdd(&S[i0 * ATT_C + j0 + 1], a01);
    atomicAdd(&S[(i0 + 1) * ATT_C + j0], a10);
    atomicAdd(&S[(i0 + 1) * ATT_C + j0 + 1], a11);
    if (j0 == 0) { atomicAdd(&S[ATT_C * ATT_C + i0], r0); atomicAdd(&S[ATT_C * ATT_C + i0 + 1], r1); }
    if (i0 == 0) { atomicAdd(&S[ATT_C * ATT_C + ATT_C + j0], c0); atomicAdd(&S[ATT_C * ATT_C + ATT_C + j0 + 1], c1); }
}

// One workgroup of 32x32 threads per image; thread (i, j) owns entry [i][j] of every 32x32 product.
__device__ __forceinline__ double mm(const double (*A)[33], const double (*Bm)[33], int i, int j) {
    double s = 0;
#pragma unroll 8
    for (int k = 0; k < ATT_C; ++k) s = fma(A[i][k], Bm[k][j], s);
    return s;
}

__global__ __launch_bounds__(1024) void attn_fold_kernel(const double* __restrict__ stats, const float* __restrict__ aw,
                                                         const float* __restrict__ fw, const float* __restrict__ fb,
                                                         float* __restrict__ Wp, float* __restrict__ bias_out, int L) {
    __shared__ double X[ATT_C][33], Y[ATT_C][33], Z[ATT_C][33], M1[ATT_C][33], M2[ATT_C][33];
    __shared__ double va[ATT_C], vb[ATT_C], c1[ATT_C], c2[ATT_C], rowred[ATT_C];
    const int i = threadIdx.x >> 5, j = threadIdx.x & 31;
    const int b = blockIdx.x;
    const double* S = stats + (int64_t)b * (ATT_C * ATT_C + 2 * ATT_C);
    const double* s1 = S + ATT_C * ATT_C;
    const double* s2 = s1 + ATT_C;
    constexpr int WSZ = ATT_C * ATT_C + ATT_C;
    auto Wm = [&](int m, int r, int c) -> double { return (double)aw[m * WSZ + r * ATT_C + c]; };
    auto Bv = [&](int m, int r) -> double { return (double)aw[m * WSZ + ATT_C * ATT_C + r]; };
    // indices into attn_w: 0 q1, 1 k2, 2 v2, 3 q2, 4 k1, 5 v1, 6 out1, 7 out2
    const double scale = 1.0 / sqrt((double)ATT_C);
    for (int br = 0; br < 2; ++br) {
        const int mq = br ? 3 : 0, mk = br ? 4 : 1, mv = br ? 5 : 2, mo = br ? 7 : 6;
        const double* sq = br ? s2 : s1;   // sums of the tensor feeding q
        const double* sk = br ? s1 : s2;   // sums of the tensor feeding k
        __syncthreads();
        // X = S (branch 0) or S^T (branch 1);  Y[k][j] = Wk[j][k]  (Wk^T)
        X[i][j] = br ? S[j * ATT_C + i] : S[i * ATT_C + j];
        Y[i][j] = Wm(mk, j, i);
        Z[i][j] = Wm(mq, i, j);
        if (i == 0) {
            double u = 0, t = 0;
            for (int k = 0; k < ATT_C; ++k) { u += Wm(mq, j, k) * sq[k]; t += Wm(mk, j, k) * sk[k]; }
            va[j] = u;   // (Wq sq)[j]
            vb[j] = t;   // (Wk sk)[j]
        }
        __syncthreads();
        const double t1 = mm(Z, X, i, j);          // (Wq S)[i][j]
        __syncthreads();
        Z[i][j] = t1;
        __syncthreads();
        double g = mm(Z, Y, i, j);                 // Wq S Wk^T
        g += va[i] * Bv(mk, j) + Bv(mq, i) * vb[j] + (double)L * Bv(mq, i) * Bv(mk, j);
        g *= scale;
        // row softmax over j
        __syncthreads();
        X[i][j] = g;
        __syncthreads();
        if (j == 0) {
            double m = X[i][0];
            for (int k = 1; k < ATT_C; ++k) m = fmax(m, X[i][k]);
            rowred[i] = m;
        }
        __syncthreads();
        const double e = exp(g - rowred[i]);
        __syncthreads();
        X[i][j] = e;
        __syncthreads();
        if (j == 0) {
            double s = 0;
            for (int k = 0; k < ATT_C; ++k) s += X[i][k];
            rowred[i] = s;
        }
        __syncthreads();
        const double pr = e / rowred[i];
        __syncthreads();
        X[i][j] = pr;                              // attn
        Y[i][j] = Wm(mv, i, j);                    // Wv
        Z[i][j] = Wm(mo, i, j);                    // Wo
        __syncthreads();
        const double pv = mm(X, Y, i, j);          // attn Wv
        if (j == 0) {
            double s = 0;
            for (int k = 0; k < ATT_C; ++k) s += X[i][k] * Bv(mv, k);
            va[i] = s;                             // attn bv
        }
        __syncthreads();
        Y[i][j] = pv;
        __syncthreads();
        const double mres = mm(Z, Y, i, j);        // Wo attn Wv
        if (j == 0) {
            double s = Bv(mo, i);
            for (int k = 0; k < ATT_C; ++k) s += Z[i][k] * va[k];
            (br ? c2 : c1)[i] = s;                 // Wo attn bv + bo
        }
        (br ? M2 : M1)[i][j] = mres;
    }
    __syncthreads();
    // fused = (Wfa + Wfb M2) F1 + (Wfa M1 + Wfb) F2 + (Wfa c1 + Wfb c2 + bf)
    X[i][j] = (double)fw[i * 64 + j];        // Wfa
    Y[i][j] = (double)fw[i * 64 + 32 + j];   // Wfb
    __syncthreads();
    const double left = X[i][j] + mm(Y, M2, i, j);
    const double right = mm(X, M1, i, j) + Y[i][j];
    // natural (32, 64) row-major per image: columns 0..31 act on F1, 32..63 on F2 (the host packs it for the x6 GEMM)
    float* wp = Wp + (int64_t)b * (32 * 64);
    wp[i * 64 + j] = (float)left;
    wp[i * 64 + 32 + j] = (float)right;
    if (j == 0) {
        double s = (double)fb[i];
        for (int k = 0; k < ATT_C; ++k) s += X[i][k] * c1[k] + Y[i][k] * c2[k];
        bias_out[(int64_t)b * 32 + i] = (float)s;
    }
}

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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / CL, r = i - b * CL;
    dst[b * dst_bs + r] = src[b * src_bs + r];
}

// dst row b takes the channels of src row b / rep: an image's planes handed to its `rep` Monte-Carlo samples in one launch
__global__ void copy_channels_rep_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                         int64_t dst_bs, int64_t CL, int64_t total, int rep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / CL, r = i - b * CL;
    dst[b * dst_bs + r] = src[(b / rep) * src_bs + r];
}

__global__ void add_channels_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                    int64_t dst_bs, int64_t CL, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / CL, r = i - b * CL;
    dst[b * dst_bs + r] += src[b * src_bs + r];
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

__global__ void bilinear_up_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                                   int64_t dst_bs, int C, int H, int W, int s, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int Wo = W * s, Ho = H * s;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const int c = (int)((i / ((int64_t)Wo * Ho)) % C), b = (int)(i / ((int64_t)Wo * Ho * C));
    const float rs = 1.f / (float)s;
    const float* p = src + (int64_t)b * src_bs + (int64_t)c * H * W;
    dst[(int64_t)b * dst_bs + ((int64_t)c * Ho + yo) * Wo + xo] = bilinear_at(p, H, W, rs, yo, xo);
}

// quat_dwt(bilinear_up(cond, s)) of the Stage-I conditions (R,3,H,W) without the enlarged image: a thread owns NPX neighbouring pixels of a
// row of the (R,32,H s/2,W s/2) output, interpolates their 2 x 2 NPX x 3 samples from the candidate's 3 H W source values (12 KiB of
// conditions per 8 MiB of output: every read after the first is an L1 hit), and writes each of the 32 planes with one 4 NPX-byte store.
template <int NPX>
__global__ __launch_bounds__(256) void cond_dwt_kernel(const float* __restrict__ cond, float* __restrict__ out, int H, int W, int s, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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

__global__ void space_to_depth_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W,
                                      int64_t total) {
    // out (B,4C,H/2,W/2): block q = dy + 2*dx  ->  [ee, oe, eo, oo]  (UNet_arch.py:74-78)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int xo = (int)(i % Wp), yo = (int)((i / Wp) % Hp);
    const int64_t plane = i / ((int64_t)Wp * Hp);
    out[i] = x[(plane * H + reflect_idx(yo, H)) * W + reflect_idx(xo, W)];
}

__global__ void resize_down_kernel(const float* __restrict__ x, float* __restrict__ out, int Hp, int Wp, int s,
                                   int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int wd = Wp / s, hd = Hp / s;
    const int xo = (int)(i % wd), yo = (int)((i / wd) % hd);
    const int64_t plane = i / ((int64_t)wd * hd);
    const int a = s / 2 - 1;
    const float* p = x + (plane * Hp + (int64_t)yo * s + a) * Wp + (int64_t)xo * s + a;
    out[i] = 0.25f * (p[0] + p[Wp] + p[1] + p[Wp + 1]);
}

// ---------------------------------------------------------------- Bayesian sampling ----------
// stream_add (all three samplers): an optional device-resident addend of the Philox stream id -- the per-iteration part of the id
// ([forward epoch] << 20, see SampleCtx.next_stream) kept in HBM so that a captured HIP graph of the step draws fresh numbers on
// every replay; NULL = the id is complete as passed.
__global__ void randn_kernel(float* __restrict__ out, int64_t total, uint64_t seed, uint64_t stream_id, const uint64_t* __restrict__ stream_add) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (stream_add) stream_id += stream_add[0];
    if (i < total) out[i] = philox_normal(i, seed, stream_id);
}

// one thread = four consecutive elements = one Philox counter block
__global__ void bnn_sample_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                  const float* __restrict__ eps_in, float* __restrict__ out, int64_t n, int64_t total,
                                  uint64_t seed, uint64_t stream_id, const uint64_t* __restrict__ stream_add) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i0 = 4 * j;
    if (i0 >= total) return;
    if (stream_add) stream_id += stream_add[0];
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!eps_in) philox_normal4(j, seed, stream_id, z);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = i0 + q;
        if (i < total) {
            const int64_t e = i % n;
            const float eps = eps_in ? eps_in[i] : z[q];
            out[i] = mu[e] + log1pf(expf(rho[e])) * eps;
        }
    }
}

// ---------------------------------------------------------------- Monte-Carlo loop pieces ----
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sh[w];
    return s;
}

__global__ __launch_bounds__(256) void plane_mean_kernel(const float* __restrict__ x, float* __restrict__ means,
                                                         int Hs, int Ws, int h, int w) {
    __shared__ double sh[4];
    const float* p = x + (int64_t)blockIdx.x * Hs * Ws;
    double s = 0;
    if (w == Ws && (w & 3) == 0 && (((uintptr_t)p) & 15) == 0) {          // whole rows of an aligned plane: 16-byte loads, no index arithmetic
        const float4* p4 = reinterpret_cast<const float4*>(p);
        double s1 = 0, s2 = 0, s3 = 0;
        for (int i = threadIdx.x; i < h * w / 4; i += 256) {
            const float4 v = p4[i];
            s += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        }
        s += s1 + s2 + s3;
    } else {
        for (int i = threadIdx.x; i < h * w; i += 256) s += (double)p[(int64_t)(i / w) * Ws + (i % w)];
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) means[blockIdx.x] = (float)(s / ((double)h * w));
}

__global__ __launch_bounds__(256) void cond_postproc_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ target_mean,
                                                            const float* __restrict__ noise, float* __restrict__ out,
                                                            int hw, int spi, float noise_level) {
    // one workgroup per (sample, channel) plane
    __shared__ double sh[4];
    const int plane = blockIdx.x, bn = plane / 3, ch = plane - bn * 3;
    const float* p = pred + (int64_t)plane * hw;
    float ratio = 1.f;
    if (target_mean) {
        double s = 0;
        for (int i = threadIdx.x; i < hw; i += 256) s += (double)fminf(fmaxf(p[i], 0.f), 1.f);
        s = block_sum(s, sh);
        const float mean_pred = (float)(s / (double)hw);
        ratio = target_mean[(bn / spi) * 3 + ch] / mean_pred;
    }
    for (int i = threadIdx.x; i < hw; i += 256) {
        float c = fminf(fmaxf(p[i], 0.f), 1.f);
        if (target_mean) c = fminf(fmaxf(c * ratio, 0.f), 1.f);
        if (noise) c += noise[(int64_t)plane * hw + i] * noise_level;
        out[(int64_t)plane * hw + i] = c;
    }
}

// Candidate finalisation in three small grids (one workgroup per candidate left 250 of 256 CUs idle):
//   sums   : per (candidate, channel) sum of the clamped crop and of the target      -> ws[bn][ch][0..1]  (f64 atomics)
//   final  : GT-mean ratio from those sums, clipped candidate out, squared error     -> ws[bn][6]
//   psnr   : 10 log10(1 / mse)
constexpr int CF_CHUNK = 4096;
__global__ __launch_bounds__(256) void cand_sums_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        double* __restrict__ ws, int spi, int Hp, int Wp, int h, int w) {
    __shared__ double sh[4];
    const int plane = blockIdx.y, bn = plane / 3, ch = plane - bn * 3;
    const int64_t hw = (int64_t)h * w;
    const float* p = pred + (int64_t)plane * Hp * Wp;
    const float* tg = target + ((int64_t)(bn / spi) * 3 + ch) * hw;
    double sp = 0, st = 0;
    const int i0 = blockIdx.x * CF_CHUNK;
    for (int i = i0 + threadIdx.x; i < i0 + CF_CHUNK && i < hw; i += 256) {
        sp += (double)fminf(fmaxf(p[(int64_t)(i / w) * Wp + (i % w)], 0.f), 1.f);
        st += (double)tg[i];
    }
    sp = block_sum(sp, sh);
    st = block_sum(st, sh);
    if (threadIdx.x == 0) {
        atomicAdd(&ws[(int64_t)bn * 7 + ch * 2], sp);
        atomicAdd(&ws[(int64_t)bn * 7 + ch * 2 + 1], st);
    }
}

__global__ __launch_bounds__(256) void cand_final_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         float* __restrict__ fin, double* __restrict__ ws, int spi, int Hp,
                                                         int Wp, int h, int w, int gt_mean) {
    __shared__ double sh[4];
    const int plane = blockIdx.y, bn = plane / 3, ch = plane - bn * 3;
    const int64_t hw = (int64_t)h * w;
    const float* p = pred + (int64_t)plane * Hp * Wp;
    const float* tg = target ? target + ((int64_t)(bn / spi) * 3 + ch) * hw : nullptr;
    float ratio = 1.f;
    if (gt_mean) {
        const double sp = ws[(int64_t)bn * 7 + ch * 2], st = ws[(int64_t)bn * 7 + ch * 2 + 1];
        ratio = (float)(st / (double)hw) / (float)(sp / (double)hw);
    }
    double mse = 0;
    const int i0 = blockIdx.x * CF_CHUNK;
    for (int i = i0 + threadIdx.x; i < i0 + CF_CHUNK && i < hw; i += 256) {
        float v = fminf(fmaxf(p[(int64_t)(i / w) * Wp + (i % w)], 0.f), 1.f);
        if (gt_mean) v = fminf(fmaxf(v * ratio, 0.f), 1.f);
        fin[(int64_t)plane * hw + i] = v;
        if (tg) {
            const double d = (double)tg[i] - (double)v;
            mse += d * d;
        }
    }
    mse = block_sum(mse, sh);
    if (threadIdx.x == 0 && tg) atomicAdd(&ws[(int64_t)bn * 7 + 6], mse);
}

__global__ void cand_psnr_kernel(const double* __restrict__ ws, float* __restrict__ psnr, int Bn, int64_t hw, int has_target) {
    const int bn = blockIdx.x * blockDim.x + threadIdx.x;
    if (bn >= Bn) return;
    const double m = ws[(int64_t)bn * 7 + 6] / (3.0 * (double)hw);
    psnr[bn] = has_target ? (m == 0 ? 100.f : (float)(10.0 * log10(1.0 / m))) : 0.f;
}

// eval.py:284-285 with psnr_weight = 1: scores = psnr / max(psnr) per image, best = first index of the maximum score
// (python list.index(max(...)) semantics, evaluated in f64 like the reference's python floats).  One thread per image.
__global__ void select_best_kernel(const float* __restrict__ psnr, int* __restrict__ best, float* __restrict__ best_psnr, int B, int N) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = psnr + (int64_t)b * N;
    double m = (double)p[0];
    for (int i = 1; i < N; ++i) m = fmax(m, (double)p[i]);
    int bi = 0;
    double bs = (double)p[0] / m;
    for (int i = 1; i < N; ++i) {
        const double sc = (double)p[i] / m;
        if (sc > bs) { bs = sc; bi = i; }
    }
    best[b] = bi;
    best_psnr[b] = p[bi];
}

__global__ void gather_best_kernel(const float* __restrict__ cand, const int* __restrict__ best, float* __restrict__ out, int N, int64_t chw4) {
    const int b = blockIdx.y;
    const float4* src = reinterpret_cast<const float4*>(cand) + ((int64_t)b * N + best[b]) * chw4;
    float4* dst = reinterpret_cast<float4*>(out) + (int64_t)b * chw4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chw4; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

__global__ void gather_best_scalar_kernel(const float* __restrict__ cand, const int* __restrict__ best, float* __restrict__ out, int N, int64_t chw) {
    const int b = blockIdx.y;
    const float* src = cand + ((int64_t)b * N + best[b]) * chw;
    float* dst = out + (int64_t)b * chw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chw; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ---------------------------------------------------------------- SSIM (Enhancement/utils.py:12-57) ----------
// calculate_ssim(img_as_ubyte(target), img_as_ubyte(pred)): per channel, on the uint8 VALUES rint(255 x) in float64, 11x11 Gaussian
// window (sigma 1.5, cv2.getGaussianKernel(11, 1.5) = normalised exp(-(i - 5)^2 / (2 sigma^2))), "valid" region [5:-5, 5:-5],
// ssim_map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), mean over the region, mean over the 3 channels.
// One workgroup = a 16 x 16 tile of the valid region of one (candidate, channel): both 26 x 26 input tiles staged in LDS.
constexpr int SS_T = 16, SS_K = 11, SS_IN = SS_T + SS_K - 1;
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ pred, const float* __restrict__ target, double* __restrict__ acc,
                                                  int spi, int h, int w) {
    __shared__ float sa[SS_IN][SS_IN + 1], sb[SS_IN][SS_IN + 1];
    __shared__ double gk[SS_K];
    __shared__ double red[4];
    const int vw = w - 10, vh = h - 10;
    const int tiles_x = (vw + SS_T - 1) / SS_T;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int ch = blockIdx.y, bn = blockIdx.z;
    const float* pa = target + ((int64_t)(bn / spi) * 3 + ch) * h * w;     // img1 = target, img2 = candidate
    const float* pb = pred + ((int64_t)bn * 3 + ch) * h * w;
    if (threadIdx.x < SS_K) {
        double sum = 0.0;
        for (int i = 0; i < SS_K; ++i) sum += exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        gk[threadIdx.x] = exp(-(double)((threadIdx.x - 5) * ((int)threadIdx.x - 5)) / (2.0 * 1.5 * 1.5)) / sum;
    }
    for (int i = threadIdx.x; i < SS_IN * SS_IN; i += 256) {
        const int r = i / SS_IN, c = i % SS_IN;
        const int y = min(ty * SS_T + r, h - 1), x = min(tx * SS_T + c, w - 1);
        sa[r][c] = rintf(fminf(fmaxf(pa[(int64_t)y * w + x], 0.f), 1.f) * 255.f);     // img_as_ubyte: rint(255 x), half to even
        sb[r][c] = rintf(fminf(fmaxf(pb[(int64_t)y * w + x], 0.f), 1.f) * 255.f);
    }
    __syncthreads();
    const int oy = threadIdx.x / SS_T, ox = threadIdx.x % SS_T;
    double v = 0.0;
    if (ty * SS_T + oy < vh && tx * SS_T + ox < vw) {
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
        for (int i = 0; i < SS_K; ++i) {
            double r1 = 0, r2 = 0, r11 = 0, r22 = 0, r12 = 0;
#pragma unroll
            for (int j = 0; j < SS_K; ++j) {
                const double a = sa[oy + i][ox + j], b = sb[oy + i][ox + j], g = gk[j];
                r1 += g * a; r2 += g * b; r11 += g * a * a; r22 += g * b * b; r12 += g * a * b;
            }
            const double g = gk[i];
            m1 += g * r1; m2 += g * r2; s11 += g * r11; s22 += g * r22; s12 += g * r12;
        }
        const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
        const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        v = ((2 * m12 + C1) * (2 * (s12 - m12) + C2)) / ((m11 + m22 + C1) * ((s11 - m11) + (s22 - m22) + C2));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc + bn, red[0] + red[1] + red[2] + red[3]);
}
__global__ void ssim_final_kernel(const double* __restrict__ acc, float* __restrict__ out, int Bn, double inv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Bn) out[i] = (float)(acc[i] * inv);
}

// Generalised selection of eval.py:268-297.  rule 0: first maximum of w s1 / max(s1) + (1 - w) s2 / max(s2) (full reference,
// :284-285; s2 = NULL means w = 1); rule 1: first maximum of s1 (no-reference CLIP-IQA, :271); rule 2: first minimum of s1 (NIQE,
// :273-274).  f64 like the reference's python floats; one thread per image.
__global__ void select_scores_kernel(const float* __restrict__ s1, const float* __restrict__ s2, double w, int rule, int* __restrict__ best,
                                     float* __restrict__ best_s1, float* __restrict__ best_s2, int B, int N) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = s1 + (int64_t)b * N;
    const float* q = s2 ? s2 + (int64_t)b * N : nullptr;
    int bi = 0;
    if (rule == 0) {
        double m1 = (double)p[0], m2 = q ? (double)q[0] : 1.0;
        for (int i = 1; i < N; ++i) { m1 = fmax(m1, (double)p[i]); if (q) m2 = fmax(m2, (double)q[i]); }
        double bs = -1e300;
        for (int i = 0; i < N; ++i) {
            const double sc = q ? w * (double)p[i] / m1 + (1.0 - w) * (double)q[i] / m2 : (double)p[i] / m1;
            if (sc > bs) { bs = sc; bi = i; }
        }
    } else {
        double bs = (double)p[0];
        for (int i = 1; i < N; ++i) {
            const double sc = (double)p[i];
            if (rule == 1 ? sc > bs : sc < bs) { bs = sc; bi = i; }
        }
    }
    best[b] = bi;
    if (best_s1) best_s1[b] = p[bi];
    if (best_s2 && q) best_s2[b] = q[bi];
}

// Monte-Carlo mean of eval.py:224-225,308-314: mc = clamp(mean_n clamp(pred_n[:h,:w], 0, 1), 0, 1); with GT-mean the whole image is
// scaled by mean(gray(target)) / mean(gray(mc)), gray = cv2.COLOR_BGR2GRAY of the array as stored (0.114 c0 + 0.587 c1 + 0.299 c2).
__global__ __launch_bounds__(256) void mc_mean_kernel(const float* __restrict__ pred, float* __restrict__ out, double* __restrict__ gsum,
                                                     const float* __restrict__ target, int N, int Hp, int Wp, int h, int w) {
    __shared__ double sh[2][4];
    const int ch = blockIdx.y, b = blockIdx.z;
    const float gw = ch == 0 ? 0.114f : (ch == 1 ? 0.587f : 0.299f);
    double sm = 0.0, st = 0.0;
    const int64_t hw = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        float a = 0.f;
        for (int n = 0; n < N; ++n) a += fminf(fmaxf(pred[(((int64_t)b * N + n) * 3 + ch) * Hp * Wp + (int64_t)y * Wp + x], 0.f), 1.f);
        a = fminf(fmaxf(a / (float)N, 0.f), 1.f);
        out[((int64_t)b * 3 + ch) * hw + i] = a;
        sm += (double)(gw * a);
        if (target) st += (double)(gw * target[((int64_t)b * 3 + ch) * hw + i]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sm += __shfl_xor(sm, d, 64); st += __shfl_xor(st, d, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = sm; sh[1][threadIdx.x >> 6] = st; }
    __syncthreads();
    if (threadIdx.x == 0 && gsum) {
        atomicAdd(gsum + 2 * b, sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
        atomicAdd(gsum + 2 * b + 1, sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
    }
}
__global__ void mc_rescale_kernel(float* __restrict__ out, const double* __restrict__ gsum, int64_t chw, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / chw;
    const float ratio = (float)(gsum[2 * b + 1] / gsum[2 * b]);
    out[i] = fminf(fmaxf(out[i] * ratio, 0.f), 1.f);
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

extern "C" int bem_attn_stats_f64(const float* f1, const float* f2, double* stats, int B, int L, void* stream) {
    BEM_REQUIRE(f1 && f2 && stats, "attn_stats: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 65535 && L > 0, "attn_stats: bad shape");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, sizeof(double) * (size_t)B * (ATT_C * ATT_C + 2 * ATT_C), s) != hipSuccess)
        return bem_check_launch("attn_stats memset");
    dim3 grid(cdiv(L, ATT_CHUNK), B);
    attn_stats_kernel<<<grid, 256, 0, s>>>(f1, f2, stats, L);
    return bem_check_launch("attn_stats");
}

extern "C" int bem_attn_fold_f32(const double* stats, const float* attn_w, const float* fuse_w, const float* fuse_b,
                                 float* Wp_out, float* bias_out, int B, int L, void* stream) {
    BEM_REQUIRE(stats && attn_w && fuse_w && fuse_b && Wp_out && bias_out, "attn_fold: null tensor");
    BEM_REQUIRE(B >= 0 && L > 0, "attn_fold: bad shape");
    if (B == 0) return BEM_OK;
    attn_fold_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(stats, attn_w, fuse_w, fuse_b, Wp_out, bias_out, L);
    return bem_check_launch("attn_fold");
}

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

extern "C" int bem_bnn_sample_f32(const float* mu, const float* rho, const float* eps_in, float* out, int nsets,
                                  int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, void* stream) {
    BEM_REQUIRE(mu && rho && out, "bnn_sample: null tensor");
    BEM_REQUIRE(nsets >= 0 && n >= 0, "bnn_sample: bad shape");
    const int64_t total = (int64_t)nsets * n;
    if (total == 0) return BEM_OK;
    bnn_sample_kernel<<<GRID1D(cdiv64(total, 4)), 256, 0, (hipStream_t)stream>>>(mu, rho, eps_in, out, n, total, seed, stream_id, stream_add);
    return bem_check_launch("bnn_sample");
}

extern "C" int bem_cond_postproc_f32(const float* pred, const float* target_mean, const float* noise, float* out,
                                     int Bn, int h, int w, int samples_per_image, float noise_level, void* stream) {
    BEM_REQUIRE(pred && out, "cond_postproc: null tensor");
    BEM_REQUIRE(Bn >= 0 && h > 0 && w > 0 && samples_per_image >= 1, "cond_postproc: bad shape");
    if (Bn == 0) return BEM_OK;
    cond_postproc_kernel<<<Bn * 3, 256, 0, (hipStream_t)stream>>>(pred, target_mean, noise, out, h * w, samples_per_image, noise_level);
    return bem_check_launch("cond_postproc");
}

extern "C" int bem_plane_mean_f32(const float* x, float* means, int P, int Hs, int Ws, int h, int w, void* stream) {
    BEM_REQUIRE(x && means, "plane_mean: null tensor");
    BEM_REQUIRE(P >= 0 && h > 0 && w > 0 && h <= Hs && w <= Ws, "plane_mean: bad shape");
    if (P == 0) return BEM_OK;
    plane_mean_kernel<<<P, 256, 0, (hipStream_t)stream>>>(x, means, Hs, Ws, h, w);
    return bem_check_launch("plane_mean");
}

extern "C" int bem_candidate_finalize_f32(const float* pred, const float* target, float* final_out, float* psnr,
                                          double* ws, int Bn, int samples_per_image, int Hp, int Wp, int h, int w, int gt_mean,
                                          void* stream) {
    BEM_REQUIRE(pred && final_out && ws, "candidate_finalize: null tensor");
    BEM_REQUIRE(Bn >= 0 && 3 * (int64_t)Bn <= 65535 && samples_per_image >= 1 && h > 0 && w > 0 && h <= Hp && w <= Wp, "candidate_finalize: bad shape");
    BEM_REQUIRE(!gt_mean || target, "candidate_finalize: GT_mean needs a target");
    if (Bn == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, sizeof(double) * 7 * (size_t)Bn, s) != hipSuccess) return bem_check_launch("candidate_finalize memset");
    dim3 grid(cdiv(h * w, CF_CHUNK), 3 * Bn);
    if (gt_mean) cand_sums_kernel<<<grid, 256, 0, s>>>(pred, target, ws, samples_per_image, Hp, Wp, h, w);
    cand_final_kernel<<<grid, 256, 0, s>>>(pred, target, final_out, ws, samples_per_image, Hp, Wp, h, w, gt_mean);
    if (psnr) cand_psnr_kernel<<<cdiv(Bn, 256), 256, 0, s>>>(ws, psnr, Bn, (int64_t)h * w, target != nullptr);
    return bem_check_launch("candidate_finalize");
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

extern "C" int bem_randn_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, void* stream) {
    BEM_REQUIRE(out && n >= 0, "randn: bad arguments");
    if (n == 0) return BEM_OK;
    randn_kernel<<<GRID1D(n), 256, 0, (hipStream_t)stream>>>(out, n, seed, stream_id, stream_add);
    return bem_check_launch("randn");
}

extern "C" int bem_select_best_f32(const float* cand, const float* psnr, int* best, float* best_psnr, float* best_img, int B, int N,
                                   int64_t chw, void* stream) {
    BEM_REQUIRE(psnr && best && best_psnr, "select_best: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && chw >= 0, "select_best: bad shape B=%d N=%d", B, N);
    BEM_REQUIRE((cand == nullptr) == (best_img == nullptr), "select_best: cand and best_img go together");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    select_best_kernel<<<cdiv(B, 64), 64, 0, s>>>(psnr, best, best_psnr, B, N);
    if (cand && chw > 0) {
        const bool v4 = chw % 4 == 0 && (((uintptr_t)cand | (uintptr_t)best_img) & 15) == 0;
        const int64_t n = v4 ? chw / 4 : chw;
        dim3 grid((unsigned)std::min<int64_t>(cdiv64(n, 256), 1024), B);
        if (v4) gather_best_kernel<<<grid, 256, 0, s>>>(cand, best, best_img, N, n);
        else gather_best_scalar_kernel<<<grid, 256, 0, s>>>(cand, best, best_img, N, n);
    }
    return bem_check_launch("select_best");
}

extern "C" int bem_ssim_f32(const float* pred, const float* target, float* ssim, double* ws, int Bn, int samples_per_image, int h, int w, void* stream) {
    BEM_REQUIRE(pred && target && ssim && ws, "ssim: null tensor");
    BEM_REQUIRE(Bn >= 0 && Bn <= 65535 && samples_per_image >= 1 && Bn % samples_per_image == 0 && h > 10 && w > 10, "ssim: bad shape (images larger than the 11x11 window)");
    if (Bn == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, sizeof(double) * Bn, s) != hipSuccess) return bem_check_launch("ssim memset");
    const int tiles = cdiv(h - 10, SS_T) * cdiv(w - 10, SS_T);
    ssim_kernel<<<dim3(tiles, 3, Bn), 256, 0, s>>>(pred, target, ws, samples_per_image, h, w);
    ssim_final_kernel<<<cdiv(Bn, 64), 64, 0, s>>>(ws, ssim, Bn, 1.0 / (3.0 * (double)(h - 10) * (double)(w - 10)));
    return bem_check_launch("ssim");
}

extern "C" int bem_select_scores_f32(const float* cand, const float* s1, const float* s2, float weight, int rule, int* best, float* best_s1,
                                     float* best_s2, float* best_img, int B, int N, int64_t chw, void* stream) {
    BEM_REQUIRE(s1 && best, "select_scores: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && chw >= 0 && rule >= 0 && rule <= 2, "select_scores: bad arguments");
    BEM_REQUIRE((cand == nullptr) == (best_img == nullptr), "select_scores: cand and best_img go together");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    select_scores_kernel<<<cdiv(B, 64), 64, 0, s>>>(s1, s2, (double)weight, rule, best, best_s1, best_s2, B, N);
    if (cand && chw > 0) {
        const bool v4 = chw % 4 == 0 && (((uintptr_t)cand | (uintptr_t)best_img) & 15) == 0;
        const int64_t n = v4 ? chw / 4 : chw;
        dim3 grid((unsigned)std::min<int64_t>(cdiv64(n, 256), 1024), B);
        if (v4) gather_best_kernel<<<grid, 256, 0, s>>>(cand, best, best_img, N, n);
        else gather_best_scalar_kernel<<<grid, 256, 0, s>>>(cand, best, best_img, N, n);
    }
    return bem_check_launch("select_scores");
}

extern "C" int bem_mc_mean_f32(const float* pred, const float* target, float* out, double* ws, int B, int N, int Hp, int Wp, int h, int w,
                               int gt_mean, void* stream) {
    BEM_REQUIRE(pred && out && B >= 0 && B <= 65535 && N >= 1 && h > 0 && w > 0 && h <= Hp && w <= Wp, "mc_mean: bad arguments");
    BEM_REQUIRE(!gt_mean || (target && ws), "mc_mean: GT-mean needs the target and a scratch of 2 B doubles");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (gt_mean && hipMemsetAsync(ws, 0, sizeof(double) * 2 * B, s) != hipSuccess) return bem_check_launch("mc_mean memset");
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv64((int64_t)h * w, 256), 256);
    mc_mean_kernel<<<dim3(gx, 3, B), 256, 0, s>>>(pred, out, gt_mean ? ws : nullptr, gt_mean ? target : nullptr, N, Hp, Wp, h, w);
    if (gt_mean) {
        const int64_t total = (int64_t)B * 3 * h * w;
        mc_rescale_kernel<<<GRID1D(total), 256, 0, s>>>(out, ws, (int64_t)3 * h * w, total);
    }
    return bem_check_launch("mc_mean");
}

// ------------------------------------------------------------------------------------------------
// 16-bit <-> float32 casts of the operator seam's backward (selective_scan_cuda_oflex.bwd with f16 / bf16 inputs): dtype 1 = float16,
// 2 = bfloat16 (round to nearest even on the way down, like torch's .to()).
// ------------------------------------------------------------------------------------------------
namespace {
__global__ void cast16_to_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n, int dtype) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint16_t b = src[i];
    dst[i] = dtype == 1 ? (float)__builtin_bit_cast(_Float16, b) : __builtin_bit_cast(float, (uint32_t)b << 16);
}
__global__ void cast_f32_to16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n, int dtype) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    cast16_to_f32_kernel<<<(unsigned)cdiv64(n, 256), 256, 0, (hipStream_t)stream>>>((const uint16_t*)src, dst, n, dtype);
    return bem_check_launch("cast16_to_f32");
}
extern "C" int bem_cast_f32_to16(const float* src, void* dst, int64_t n, int dtype, void* stream) {
    BEM_REQUIRE(src && dst && n >= 0 && (dtype == 1 || dtype == 2), "cast_f32_to16: bad arguments");
    if (n == 0) return BEM_OK;
    cast_f32_to16_kernel<<<(unsigned)cdiv64(n, 256), 256, 0, (hipStream_t)stream>>>(src, (uint16_t*)dst, n, dtype);
    return bem_check_launch("cast_f32_to16");
}
