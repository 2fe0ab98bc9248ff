// Channel attention of the fusion: f64 statistics of the two feature maps, and the fold of the attention weights into one
// per-image (32, 64) matrix + bias for the x6 GEMM.
#include "bem_common.h"

namespace {

// ---------------------------------------------------------------- channel attention ----------
// stats[b] = { S[32][32] = F1 F2^T, s1[32] = F1 1, s2[32] = F2 1 } accumulated in f64.
//
// S goes through v_mfma_f64_16x16x4_f64 (products of f32 values are exact in f64, the sums stay f64): four 16x16 tiles per image, the
// pixels as k.  Lane (c = lane & 15, g = lane >> 4) supplies A[c][k = g] and B[k = g][c]; it loads four consecutive pixels
// pb + 4g .. pb + 4g + 3 of channels c and c + 16 of both maps as float4, and MFMA step s takes component s of all of them, so A and B
// agree on which pixel is k = g of step s.  No LDS in the product loop; the next 16 pixels are loaded ahead of the current 16 MFMAs.
// The channel sums are f64 adds on the same registers (8 adds beside 16 MFMAs of 64 cycles each).
// The four waves of a workgroup take consecutive 16-pixel groups (256 contiguous bytes of every channel row per step) of a `chunk` of
// pixels, join in LDS and add one partial of every statistic to the zeroed `stats`.
constexpr int ATT_C = 32;
constexpr int ATT_STATS = ATT_C * ATT_C + 2 * ATT_C;
constexpr int ATT_CHUNK_MAX = 2048, ATT_CHUNK_MIN = 256;   // pixels per workgroup, multiples of 64 (4 waves x 16 pixels)
constexpr int ATT_MIN_WG = 512;                            // two workgroups per CU: the chunk halves until the launch has that many
using f64x4 = __attribute__((ext_vector_type(4))) double;

// pixels p .. p + 3 of one channel row, zero past pend.  vec: every row base and p are 16-byte aligned and pend - p is a multiple of 4.
__device__ __forceinline__ void att_load4(const float* __restrict__ row, int64_t p, int64_t pend, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 t = p < pend ? *reinterpret_cast<const float4*>(row + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = p + s < pend ? row[p + s] : 0.f;
    }
}

__global__ __launch_bounds__(256) void attn_stats_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                                                         double* __restrict__ stats, int L, int chunk, int vec) {
    __shared__ double part[4][ATT_STATS];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * chunk, pend = min(p0 + chunk, (int64_t)L);
    const float* rows[4] = {f1 + ((int64_t)b * ATT_C + c) * L, f1 + ((int64_t)b * ATT_C + c + 16) * L,
                            f2 + ((int64_t)b * ATT_C + c) * L, f2 + ((int64_t)b * ATT_C + c + 16) * L};
    f64x4 acc[2][2] = {};
    double sum[4] = {0, 0, 0, 0};
    float cur[4][4], nxt[4][4];
    int64_t pb = p0 + wave * 16;                                      // wave-uniform: every lane of the wave runs every MFMA
#pragma unroll
    for (int r = 0; r < 4; ++r) att_load4(rows[r], pb + 4 * g, pend, vec, cur[r]);
    for (; pb < pend; pb += 64) {
#pragma unroll
        for (int r = 0; r < 4; ++r) att_load4(rows[r], pb + 64 + 4 * g, pend, vec, nxt[r]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double a0 = (double)cur[0][s], a1 = (double)cur[1][s], b0 = (double)cur[2][s], b1 = (double)cur[3][s];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            sum[0] += a0; sum[1] += a1; sum[2] += b0; sum[3] += b1;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) cur[r][s] = nxt[r][s];
    }
    // C/D of the f64 MFMA: register q of a lane is row (lane >> 4) + 4 q, column lane & 15 of its tile
    double* mine = part[wave];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int q = 0; q < 4; ++q) mine[(16 * ti + g + 4 * q) * ATT_C + 16 * tj + c] = acc[ti][tj][q];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                     // the four pixel groups g of a channel sit 16 lanes apart
        double v = sum[r];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (g == 0) mine[ATT_C * ATT_C + 16 * r + c] = v;             // s1[c], s1[c + 16], s2[c], s2[c + 16]
    }
    __syncthreads();
    double* S = stats + (int64_t)b * ATT_STATS;
    for (int i = threadIdx.x; i < ATT_STATS; i += 256) atomicAdd(&S[i], (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]));
}

// One workgroup of 32x32 threads per image; thread (i, j) owns entry [i][j] of every 32x32 product.
__device__ __forceinline__ double mm(const double (*A)[33], const double (*Bm)[33], int i, int j) {
    double s = 0;
#pragma unroll 8
    for (int k = 0; k < ATT_C; ++k) s = fma(A[i][k], Bm[k][j], s);
    return s;
}

// Attention dropout (QD/model3.py:98,124-131: nn.Dropout(0.1) on both softmaxed maps, live in train() mode).  Everything after the softmax
// is linear in the map, so the dropout is one factor on the entry thread (i, j) writes to X: keep / (1 - p), in f64.  The keep flag is
// read from `mask` (B, 2, 32, 32; map 0 = attn_1, map 1 = attn_2; 0 or 1) or, without one, drawn from Philox4x32-10 laid out like
// philox_normal4: element e = ((b * 2 + br) * 1024 + i * 32 + j) is word e & 3 of counter block e >> 2 under (seed, stream_id),
// u = (word >> 8) * 2^-24 in [0, 1), kept iff u >= p (compared in f32).  The eval form carries none of it.
template <bool DROP> struct AttDrop {};
template <> struct AttDrop<true> {
    const float* mask;
    float p;
    uint64_t seed, stream_id;
};

template <bool DROP>
__global__ __launch_bounds__(1024) void attn_fold_kernel(const double* __restrict__ stats, const float* __restrict__ aw,
                                                         const float* __restrict__ fw, const float* __restrict__ fb,
                                                         float* __restrict__ Wp, float* __restrict__ bias_out, int L, const AttDrop<DROP> drop) {
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
        if constexpr (DROP) {
            const int64_t el = ((int64_t)b * 2 + br) * (ATT_C * ATT_C) + i * ATT_C + j;
            bool keep;
            if (drop.mask) {
                keep = drop.mask[el] != 0.f;
            } else {
                uint32_t c[4] = {(uint32_t)(el >> 2), (uint32_t)((uint64_t)(el >> 2) >> 32), (uint32_t)drop.stream_id, (uint32_t)(drop.stream_id >> 32)};
                philox4x32_10(c, (uint32_t)drop.seed, (uint32_t)(drop.seed >> 32));
                const uint32_t wd = (el & 2) ? ((el & 1) ? c[3] : c[2]) : ((el & 1) ? c[1] : c[0]);      // selects, not an indexed array
                keep = (float)(wd >> 8) * (1.0f / 16777216.0f) >= drop.p;
            }
            X[i][j] = keep ? pr * (1.0 / (1.0 - (double)drop.p)) : 0.0;   // attn, dropped out
        } else {
            X[i][j] = pr;                          // attn
        }
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
    BEM_ZERO(stats, sizeof(double) * (size_t)B * ATT_STATS, s, "attn_stats");
    int chunk = ATT_CHUNK_MAX;
    while (chunk > ATT_CHUNK_MIN && (int64_t)B * cdiv64(L, chunk) < ATT_MIN_WG) chunk >>= 1;
    // float4 loads need every channel row 16-byte aligned; otherwise (L % 4 != 0: the rows of every second channel are not) scalar loads
    const int vec = L % 4 == 0 && (((uintptr_t)f1 | (uintptr_t)f2) & 15) == 0;
    dim3 grid((unsigned)cdiv64(L, chunk), B);
    attn_stats_kernel<<<grid, 256, 0, s>>>(f1, f2, stats, L, chunk, vec);
    return bem_check_launch("attn_stats");
}

extern "C" int bem_attn_fold_f32(const double* stats, const float* attn_w, const float* fuse_w, const float* fuse_b,
                                 float* Wp_out, float* bias_out, int B, int L, void* stream) {
    BEM_REQUIRE(stats && attn_w && fuse_w && fuse_b && Wp_out && bias_out, "attn_fold: null tensor");
    BEM_REQUIRE(B >= 0 && L > 0, "attn_fold: bad shape");
    if (B == 0) return BEM_OK;
    attn_fold_kernel<false><<<B, 1024, 0, (hipStream_t)stream>>>(stats, attn_w, fuse_w, fuse_b, Wp_out, bias_out, L, AttDrop<false>{});
    return bem_check_launch("attn_fold");
}

extern "C" int bem_attn_fold_drop_f32(const double* stats, const float* attn_w, const float* fuse_w, const float* fuse_b, const float* mask,
                                      float p, uint64_t seed, uint64_t stream_id, float* Wp_out, float* bias_out, int B, int L, void* stream) {
    BEM_REQUIRE(stats && attn_w && fuse_w && fuse_b && Wp_out && bias_out, "attn_fold_drop: null tensor");
    BEM_REQUIRE(B >= 0 && L > 0, "attn_fold_drop: bad shape");
    BEM_REQUIRE(p >= 0.f && p < 1.f, "attn_fold_drop: p must be in [0, 1)");
    if (B == 0) return BEM_OK;
    attn_fold_kernel<true><<<B, 1024, 0, (hipStream_t)stream>>>(stats, attn_w, fuse_w, fuse_b, Wp_out, bias_out, L,
                                                                 AttDrop<true>{mask, p, seed, stream_id});
    return bem_check_launch("attn_fold_drop");
}
