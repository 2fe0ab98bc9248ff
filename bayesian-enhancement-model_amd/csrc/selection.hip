// The eval step's selection tail (eval.py:224-314): condition post-processing, candidate finalisation + PSNR, SSIM, best-candidate
// selection and gather, Monte-Carlo mean.  The no-reference scorers have a file each (niqe.hip, uiqm.hip).
#include "bem_common.h"
#include <algorithm>

namespace {

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
    s = block_sum<4>(s, sh);
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
        s = block_sum<4>(s, sh);
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
    sp = block_sum<4>(sp, sh);
    st = block_sum<4>(st, sh);
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
    mse = block_sum<4>(mse, sh);
    if (threadIdx.x == 0 && tg) atomicAdd(&ws[(int64_t)bn * 7 + 6], mse);
}

__global__ void cand_psnr_kernel(const double* __restrict__ ws, float* __restrict__ psnr, int Bn, int64_t hw, int has_target) {
    const int bn = blockIdx.x * blockDim.x + threadIdx.x;
    if (bn >= Bn) return;
    const double m = ws[(int64_t)bn * 7 + 6] / (3.0 * (double)hw);
    psnr[bn] = has_target ? (m == 0 ? 100.f : (float)(10.0 * log10(1.0 / m))) : 0.f;
}

__global__ void gather_best_kernel(const float* __restrict__ cand, const int* __restrict__ best, float* __restrict__ out, int N, int64_t chw4) {
    const int b = blockIdx.y, k = best[b];
    if (k < 0) return;                                                     // the streaming merge: this image keeps what it has
    const float4* src = reinterpret_cast<const float4*>(cand) + ((int64_t)b * N + k) * chw4;
    float4* dst = reinterpret_cast<float4*>(out) + (int64_t)b * chw4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chw4; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

__global__ void gather_best_scalar_kernel(const float* __restrict__ cand, const int* __restrict__ best, float* __restrict__ out, int N, int64_t chw) {
    const int b = blockIdx.y, k = best[b];
    if (k < 0) return;
    const float* src = cand + ((int64_t)b * N + k) * chw;
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
        sa[r][c] = bem_ubyte(pa[(int64_t)y * w + x]);
        sb[r][c] = bem_ubyte(pb[(int64_t)y * w + x]);
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
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc + bn, red[0] + red[1] + red[2] + red[3]);
}
__global__ void ssim_final_kernel(const double* __restrict__ acc, float* __restrict__ out, int Bn, double inv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Bn) out[i] = (float)(acc[i] * inv);
}

// ---------------------------------------------------------------- per-image selection (eval.py:268-297) ----------
// best = the FIRST index of the best score among an image's N samples, as python's list.index(max(...)) / index(min(...)) gives it,
// compared in f64 like the reference's python floats.  One loop (first_better) serves every rule; a rule is its score and its start:
//   0 weighted : w s1 / max(s1) + (1 - w) s2 / max(s2) (eval.py:284-285 PSNR / SSIM, :277-278 UIQM / UCIQE), s1 / max(s1) without s2.
//                Starts from -1e300 at index 0.
//   1 max      : s1 (CLIP-IQA, :271)          2 min : s1, smaller is better (NIQE, :273-274).
//                Start from element 0, or -- n_done > 0, the streamed merge -- from the running best_score with "no sample of this chunk".
//   3 relative : s1 / max(s1) (:284-285 with psnr_weight = 1, the default PSNR rule).  Starts from element 0.
// The maxima are taken by fmax, which passes NaN over.  This block is the project's statement of the edge cases (the host's is
// bem.scorers.first_index):
//   NaN       : a comparison with NaN is false, so no rule ever moves TO a NaN score.  Rules 1, 2 and 3 start from element 0 and keep a
//               leading NaN (index 0, python's max() / min() likewise); in a merge a NaN running score is kept by every later chunk.
//               Rule 0 starts below every score and passes NaN over: index 0 only when all scores are NaN (python would keep a leading
//               one).  In rule 3 a NaN anywhere but first leaves the maximum to the others; all NaN gives index 0.
//   max == 0  : rules 0 and 3 divide by it: 0 / 0 is NaN and a negative score over 0 is -inf, neither is ever strictly better, so a
//               zero maximum gives index 0 (all-zero scores: PSNR without a target).
//   max < 0   : dividing by a negative maximum turns the order of s1 round in rules 0 and 3 (rule 3: the first MINIMUM wins), as in the reference.
//   ties      : the comparison is strict, the first index wins; a chunked merge changes its choice only for a strictly better score.
enum { RULE_WEIGHTED = 0, RULE_MAX = 1, RULE_MIN = 2, RULE_RELATIVE = 3 };

template <class Score>
__device__ __forceinline__ void first_better(Score score, bool smaller, int i0, int i1, double& bs, int& bi) {
    for (int i = i0; i < i1; ++i) {
        const double sc = score(i);
        if (smaller ? sc < bs : sc > bs) { bs = sc; bi = i; }
    }
}

// One thread per image over its N samples of this call.  best[b] = n_done + index, best_s1 / best_s2 [b] = the chosen sample's scores;
// all three stay as they are where a merge (n_done > 0) finds nothing better.  pick[b] (or NULL) = the row of this call to copy, -1 for none.
__global__ void select_kernel(const float* __restrict__ s1, const float* __restrict__ s2, double w, int rule, int* __restrict__ best,
                              float* __restrict__ best_s1, float* __restrict__ best_s2, int* __restrict__ pick, int B, int N, int n_done) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = s1 + (int64_t)b * N;
    const float* q = s2 ? s2 + (int64_t)b * N : nullptr;
    int bi = 0;
    double bs;
    if (rule == RULE_MAX || rule == RULE_MIN) {
        const auto raw = [&](int i) { return (double)p[i]; };
        if (n_done == 0) bs = raw(0);
        else { bs = (double)best_s1[b]; bi = -1; }
        first_better(raw, rule == RULE_MIN, n_done == 0 ? 1 : 0, N, bs, bi);
    } else {
        double m1 = (double)p[0], m2 = q ? (double)q[0] : 1.0;
        for (int i = 1; i < N; ++i) { m1 = fmax(m1, (double)p[i]); if (q) m2 = fmax(m2, (double)q[i]); }
        const auto rel = [&](int i) { return q ? w * (double)p[i] / m1 + (1.0 - w) * (double)q[i] / m2 : (double)p[i] / m1; };
        const bool lead = rule == RULE_RELATIVE;
        bs = lead ? rel(0) : -1e300;
        first_better(rel, false, lead ? 1 : 0, N, bs, bi);
    }
    if (pick) pick[b] = bi;
    if (bi < 0) return;
    best[b] = n_done + bi;
    if (best_s1) best_s1[b] = p[bi];
    if (best_s2 && q) best_s2[b] = q[bi];
}

// Monte-Carlo mean of eval.py:224-225,308-314: mc = clamp(mean_n clamp(pred_n[:h,:w], 0, 1), 0, 1); with GT-mean the whole image is
// scaled by mean(gray(target)) / mean(gray(mc)), gray = cv2.COLOR_BGR2GRAY of the array as stored (0.114 c0 + 0.587 c1 + 0.299 c2).
// SUMMED: pred is the (B,3,h,w) plane of sums that mc_accum_kernel left (the same additions in the same order), not the N raw outputs.
template <bool SUMMED>
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
        if (SUMMED) a = pred[((int64_t)b * 3 + ch) * hw + i];
        else for (int n = 0; n < N; ++n) a += fminf(fmaxf(pred[(((int64_t)b * N + n) * 3 + ch) * Hp * Wp + (int64_t)y * Wp + x], 0.f), 1.f);
        a = fminf(fmaxf(a / (float)N, 0.f), 1.f);
        out[((int64_t)b * 3 + ch) * hw + i] = a;
        sm += (double)(gw * a);
        if (target) st += (double)(gw * target[((int64_t)b * 3 + ch) * hw + i]);
    }
    sm = wave_sum(sm); st = wave_sum(st);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = sm; sh[1][threadIdx.x >> 6] = st; }
    __syncthreads();
    if (threadIdx.x == 0 && gsum) {
        atomicAdd(gsum + 2 * b, sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
        atomicAdd(gsum + 2 * b + 1, sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
    }
}
__global__ void mc_rescale_kernel(float* __restrict__ out, const double* __restrict__ gsum, int64_t chw, int64_t total) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    const int64_t b = i / chw;
    const float ratio = (float)(gsum[2 * b + 1] / gsum[2 * b]);
    out[i] = fminf(fmaxf(out[i] * ratio, 0.f), 1.f);
}

template <bool SUMMED>
void launch_mc_mean(const float* pred, const float* target, float* out, double* ws, int B, int N, int Hp, int Wp, int h, int w, int gt_mean,
                    hipStream_t s) {
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv64((int64_t)h * w, 256), 256);
    mc_mean_kernel<SUMMED><<<dim3(gx, 3, B), 256, 0, s>>>(pred, out, gt_mean ? ws : nullptr, gt_mean ? target : nullptr, N, Hp, Wp, h, w);
    if (gt_mean) {
        const int64_t total = (int64_t)B * 3 * h * w;
        mc_rescale_kernel<<<GRID1D(total), 256, 0, s>>>(out, ws, (int64_t)3 * h * w, total);
    }
}

// ---------------------------------------------------------------- streamed Monte-Carlo statistics ----------
// V consecutive floats of a row as one access: V = 4 where the row lengths, pitches and pointers are multiples of 16 bytes.
template <int V> struct fvec { float v[V]; };
template <int V> __device__ __forceinline__ fvec<V> ld_vec(const float* p) {
    fvec<V> r;
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; }
    else r.v[0] = *p;
    return r;
}
template <int V> __device__ __forceinline__ void st_vec(float* p, const fvec<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// Welford's update with x as sample number k.  Every operation is rounded to f32 on its own: a contracted d * (x - mean) + m2 would
// make the bits depend on what the compiler fuses, and the state must be a function of the sample sequence alone.
__device__ __forceinline__ void welford_step(float x, float k, float& mean, float& m2) {
#pragma clang fp contract(off)
    const float d = x - mean;
    mean = mean + d / k;
    const float t = d * (x - mean);
    m2 = m2 + t;
}

// One chunk of Nc samples per image into the state planes: thread = V elements of one (image, channel) plane, samples in order.
template <int V>
__global__ __launch_bounds__(256) void mc_accum_kernel(const float* __restrict__ raw, const float* __restrict__ fin, float* __restrict__ sum,
                                                      float* __restrict__ mean, float* __restrict__ m2, int Nc, int n_done, int Hp, int Wp,
                                                      int h, int w) {
    const int ch = blockIdx.y, b = blockIdx.z;
    const int64_t hw = (int64_t)h * w, pitch = (int64_t)Hp * Wp, plane = ((int64_t)b * 3 + ch) * hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw / V; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i * V;
        if (raw) {
            const int64_t at = (e / w) * Wp + (e % w);                    // w % V == 0: the V elements share a row
            fvec<V> a = ld_vec<V>(sum + plane + e);
            for (int n = 0; n < Nc; ++n) {
                const fvec<V> x = ld_vec<V>(raw + (((int64_t)b * Nc + n) * 3 + ch) * pitch + at);
#pragma unroll
                for (int j = 0; j < V; ++j) a.v[j] += fminf(fmaxf(x.v[j], 0.f), 1.f);
            }
            st_vec<V>(sum + plane + e, a);
        }
        if (fin) {
            fvec<V> m = ld_vec<V>(mean + plane + e), q = ld_vec<V>(m2 + plane + e);
            for (int n = 0; n < Nc; ++n) {
                const fvec<V> x = ld_vec<V>(fin + (((int64_t)b * Nc + n) * 3 + ch) * hw + e);
#pragma unroll
                for (int j = 0; j < V; ++j) welford_step(x.v[j], (float)(n_done + n + 1), m.v[j], q.v[j]);
            }
            st_vec<V>(mean + plane + e, m);
            st_vec<V>(m2 + plane + e, q);
        }
    }
}

// std = sqrt(m2 / (N - 1)) (zeros for N = 1) and, per workgroup, the f64 sum of what it wrote: part[b * MC_STD_BLOCKS + block].
// Workgroup k of an image takes elements [k * per, (k + 1) * per): which workgroup sums what depends on the shape alone.
constexpr int MC_STD_BLOCKS = 256;
template <int V>
__global__ __launch_bounds__(256) void mc_std_kernel(const float* __restrict__ m2, float* __restrict__ out, double* __restrict__ part, int N,
                                                    int64_t chw, int64_t per) {
    __shared__ double sh[4];
    const int b = blockIdx.y;
    const float div = (float)(N - 1);
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = std::min<int64_t>(i0 + per, chw / V);
    double s = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        fvec<V> q = ld_vec<V>(m2 + (int64_t)b * chw + i * V);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            q.v[j] = N > 1 ? sqrtf(q.v[j] / div) : 0.f;
            s += (double)q.v[j];
        }
        st_vec<V>(out + (int64_t)b * chw + i * V, q);
    }
    s = block_sum<4>(s, sh);
    if (threadIdx.x == 0) part[(int64_t)b * MC_STD_BLOCKS + blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void mc_std_mean_kernel(const double* __restrict__ part, double* __restrict__ std_mean, int nblk, int64_t chw) {
    __shared__ double sh[4];
    const int b = blockIdx.x;
    double s = (int)threadIdx.x < nblk ? part[(int64_t)b * MC_STD_BLOCKS + threadIdx.x] : 0.0;      // nblk <= MC_STD_BLOCKS = 256 threads
    s = block_sum<4>(s, sh);
    if (threadIdx.x == 0) std_mean[b] = s / (double)chw;
}

// best_img[b] = cand[b][best[b]]: 16-byte copies when the planes allow it
void launch_gather_best(const float* cand, const int* best, float* best_img, int B, int N, int64_t chw, hipStream_t s) {
    const bool v4 = chw % 4 == 0 && (((uintptr_t)cand | (uintptr_t)best_img) & 15) == 0;
    const int64_t n = v4 ? chw / 4 : chw;
    dim3 grid((unsigned)std::min<int64_t>(cdiv64(n, 256), 1024), B);
    if (v4) gather_best_kernel<<<grid, 256, 0, s>>>(cand, best, best_img, N, n);
    else gather_best_scalar_kernel<<<grid, 256, 0, s>>>(cand, best, best_img, N, n);
}

// The checks, the selection launch and the gather of both selection entries.  running: the call continues a BestState (rules 1 / 2 only,
// best_s1 is the running score and is read when n_done > 0).
int launch_select(const char* op, bool running, const float* cand, const float* s1, const float* s2, float weight, int rule, int* best,
                  float* best_s1, float* best_s2, float* best_img, int* pick, int B, int N, int n_done, int64_t chw, void* stream) {
    BEM_REQUIRE(s1 && best && (!running || (best_s1 && pick)), "%s: null tensor", op);
    BEM_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && n_done >= 0 && chw >= 0, "%s: bad arguments B=%d Nc=%d n_done=%d", op, B, N, n_done);
    BEM_REQUIRE(rule >= RULE_WEIGHTED && rule <= RULE_RELATIVE && (rule != RULE_RELATIVE || !s2), "%s: unknown rule %d%s", op, rule,
                rule == RULE_RELATIVE ? " with a second score" : "");
    BEM_REQUIRE(!running || rule == RULE_MAX || rule == RULE_MIN, "%s: rule %d cannot be decided chunk by chunk (1 = max, 2 = min)", op, rule);
    BEM_REQUIRE((cand == nullptr) == (best_img == nullptr), "%s: cand and best_img go together", op);
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    select_kernel<<<cdiv(B, 64), 64, 0, s>>>(s1, s2, (double)weight, rule, best, best_s1, best_s2, pick, B, N, n_done);
    if (cand && chw > 0) launch_gather_best(cand, pick ? pick : best, best_img, B, N, chw, s);
    return bem_check_launch(op);
}

}  // namespace

// ================================================================ C ABI =========================
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
    BEM_ZERO(ws, sizeof(double) * 7 * (size_t)Bn, s, "candidate_finalize");
    dim3 grid(cdiv(h * w, CF_CHUNK), 3 * Bn);
    if (gt_mean) cand_sums_kernel<<<grid, 256, 0, s>>>(pred, target, ws, samples_per_image, Hp, Wp, h, w);
    cand_final_kernel<<<grid, 256, 0, s>>>(pred, target, final_out, ws, samples_per_image, Hp, Wp, h, w, gt_mean);
    if (psnr) cand_psnr_kernel<<<cdiv(Bn, 256), 256, 0, s>>>(ws, psnr, Bn, (int64_t)h * w, target != nullptr);
    return bem_check_launch("candidate_finalize");
}

extern "C" int bem_ssim_f32(const float* pred, const float* target, float* ssim, double* ws, int Bn, int samples_per_image, int h, int w, void* stream) {
    BEM_REQUIRE(pred && target && ssim && ws, "ssim: null tensor");
    BEM_REQUIRE(Bn >= 0 && Bn <= 65535 && samples_per_image >= 1 && Bn % samples_per_image == 0 && h > 10 && w > 10, "ssim: bad shape (images larger than the 11x11 window)");
    if (Bn == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    BEM_ZERO(ws, sizeof(double) * Bn, s, "ssim");
    const int tiles = cdiv(h - 10, SS_T) * cdiv(w - 10, SS_T);
    ssim_kernel<<<dim3(tiles, 3, Bn), 256, 0, s>>>(pred, target, ws, samples_per_image, h, w);
    ssim_final_kernel<<<cdiv(Bn, 64), 64, 0, s>>>(ws, ssim, Bn, 1.0 / (3.0 * (double)(h - 10) * (double)(w - 10)));
    return bem_check_launch("ssim");
}

extern "C" int bem_select_scores_f32(const float* cand, const float* s1, const float* s2, float weight, int rule, int* best, float* best_s1,
                                     float* best_s2, float* best_img, int B, int N, int64_t chw, void* stream) {
    return launch_select("select_scores", false, cand, s1, s2, weight, rule, best, best_s1, best_s2, best_img, nullptr, B, N, 0, chw, stream);
}

extern "C" int bem_mc_mean_f32(const float* pred, const float* target, float* out, double* ws, int B, int N, int Hp, int Wp, int h, int w,
                               int gt_mean, void* stream) {
    BEM_REQUIRE(pred && out && B >= 0 && B <= 65535 && N >= 1 && h > 0 && w > 0 && h <= Hp && w <= Wp, "mc_mean: bad arguments");
    BEM_REQUIRE(!gt_mean || (target && ws), "mc_mean: GT-mean needs the target and a scratch of 2 B doubles");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (gt_mean) BEM_ZERO(ws, sizeof(double) * 2 * B, s, "mc_mean");
    launch_mc_mean<false>(pred, target, out, ws, B, N, Hp, Wp, h, w, gt_mean, s);
    return bem_check_launch("mc_mean");
}

extern "C" int bem_mc_accum_f32(const float* raw, const float* fin, float* sum, float* mean, float* m2, int B, int Nc, int n_done, int Hp, int Wp,
                                int h, int w, void* stream) {
    BEM_REQUIRE(raw || fin, "mc_accum: null tensor (neither raw outputs nor candidates)");
    BEM_REQUIRE(!raw || sum, "mc_accum: null sum plane for the raw outputs");
    BEM_REQUIRE(!fin || (mean && m2), "mc_accum: null mean / m2 plane for the candidates");
    BEM_REQUIRE(B >= 0 && B <= 65535, "mc_accum: at most 65535 images per call, got B=%d", B);
    BEM_REQUIRE(Nc >= 1 && n_done >= 0 && (int64_t)n_done + Nc < (1 << 24), "mc_accum: bad sample counts Nc=%d n_done=%d", Nc, n_done);
    BEM_REQUIRE(h > 0 && w > 0 && h <= Hp && w <= Wp, "mc_accum: bad shape h=%d w=%d of Hp=%d Wp=%d", h, w, Hp, Wp);
    if (B == 0) return BEM_OK;
    const uintptr_t ptrs = (uintptr_t)raw | (uintptr_t)fin | (uintptr_t)sum | (uintptr_t)mean | (uintptr_t)m2;
    const bool v4 = w % 4 == 0 && (!raw || Wp % 4 == 0) && (ptrs & 15) == 0;
    const int64_t n = (int64_t)h * w / (v4 ? 4 : 1);
    dim3 grid((unsigned)std::min<int64_t>(cdiv64(n, 256), 1024), 3, B);
    if (v4) mc_accum_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(raw, fin, sum, mean, m2, Nc, n_done, Hp, Wp, h, w);
    else mc_accum_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(raw, fin, sum, mean, m2, Nc, n_done, Hp, Wp, h, w);
    return bem_check_launch("mc_accum");
}

extern "C" int bem_mc_finish_f32(const float* sum, const float* m2, const float* target, float* mc, float* std, double* std_mean, double* ws,
                                 int B, int N, int h, int w, int gt_mean, void* stream) {
    BEM_REQUIRE(mc || std, "mc_finish: null outputs (neither mc nor std asked for)");
    BEM_REQUIRE(!mc || sum, "mc_finish: mc needs the sum plane");
    BEM_REQUIRE(!std || (m2 && std_mean), "mc_finish: std needs the m2 plane and std_mean");
    BEM_REQUIRE(ws, "mc_finish: null workspace");
    BEM_REQUIRE(B >= 0 && B <= 65535 && N >= 1 && h > 0 && w > 0, "mc_finish: bad arguments B=%d N=%d h=%d w=%d", B, N, h, w);
    BEM_REQUIRE(!(mc && gt_mean) || target, "mc_finish: GT-mean needs the target");
    if (B == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (mc) {
        if (gt_mean) BEM_ZERO(ws, sizeof(double) * 2 * B, s, "mc_finish");
        launch_mc_mean<true>(sum, target, mc, ws, B, N, h, w, h, w, gt_mean, s);
    }
    if (std) {
        const int64_t chw = (int64_t)3 * h * w;
        const bool v4 = chw % 4 == 0 && (((uintptr_t)m2 | (uintptr_t)std) & 15) == 0;
        const int64_t n = chw / (v4 ? 4 : 1);
        const int nblk = (int)std::min<int64_t>(cdiv64(n, 256), MC_STD_BLOCKS);
        double* part = ws + 2 * (int64_t)B;
        if (v4) mc_std_kernel<4><<<dim3(nblk, B), 256, 0, s>>>(m2, std, part, N, chw, cdiv64(n, nblk));
        else mc_std_kernel<1><<<dim3(nblk, B), 256, 0, s>>>(m2, std, part, N, chw, cdiv64(n, nblk));
        mc_std_mean_kernel<<<B, 256, 0, s>>>(part, std_mean, nblk, chw);
    }
    return bem_check_launch("mc_finish");
}

extern "C" int bem_select_merge_f32(const float* cand, const float* scores, int rule, int* best, float* best_score, float* best_img, int* pick,
                                    int B, int Nc, int n_done, int64_t chw, void* stream) {
    return launch_select("select_merge", true, cand, scores, nullptr, 1.f, rule, best, best_score, nullptr, best_img, pick, B, Nc, n_done, chw, stream);
}
