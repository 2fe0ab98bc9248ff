// Channel attention of the fusion: f64 statistics of the two feature maps, and the fold of the attention weights into one
// per-image (32, 64) matrix + bias for the x6 GEMM.
#include "bem_common.h"

namespace {

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

}  // namespace

// ================================================================ C ABI =========================
extern "C" int bem_attn_stats_f64(const float* f1, const float* f2, double* stats, int B, int L, void* stream) {
    BEM_REQUIRE(f1 && f2 && stats, "attn_stats: null tensor");
    BEM_REQUIRE(B >= 0 && B <= 65535 && L > 0, "attn_stats: bad shape");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    BEM_ZERO(stats, sizeof(double) * (size_t)B * (ATT_C * ATT_C + 2 * ATT_C), s, "attn_stats");
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
