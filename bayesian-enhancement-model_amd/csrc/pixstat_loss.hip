// The four per-pixel statistics of CombinedLoss (basicsr/losses/my_loss.py:51-74) that are neither SSIM nor VGG features, forward and
// backward, on contiguous (B,C,H,W) f32 tensors; a sample is its n1 = C*H*W elements, n = B * n1, d = pred - gt:
//   smooth_l1 = mean(|d| < 1 ? 0.5 d^2 : |d| - 0.5)                                   (my_loss.py:30-31, F.smooth_l1_loss, beta 1)
//   psnr      = 40 - 20 log10(1 / sqrt(mse)),  mse = mean d^2                         (my_loss.py:25-28)
//   color     = mean_b |mean(gt_b) - mean(pred_b)|                                    (my_loss.py:22-23)
//   hist      = mean_k |h_gt[k] / sum h_gt - h_pred[k] / sum h_pred|,  h = torch.histc(x, 256, 0, 1)   (my_loss.py:40-49)
//   loss      = a1 smooth_l1 + a3 hist + a5 psnr + a6 color, a term with a zero alpha left out (not multiplied by 0: psnr may be -inf, hist NaN)
// histc: bin floor(256 x), x == 1 in bin 255, x < 0, x > 1 and NaN not counted.  mse == 0 gives psnr = -inf, a pred or gt with no value
// in [0,1] gives hist = 0/0 = NaN, both as torch does.
//
// Forward, one pass over pred and gt.  A workgroup never crosses a sample, so a sample's sums are the same whatever the rest of the
// batch is and however the grid is scheduled:
//   n1 >  PS_K / 4: a sample is cut into cdiv(n1, PS_K) chunks of PS_K elements (the last one shorter), one workgroup each;
//   n1 <= PS_K / 4: a workgroup takes PS_K / n1 whole samples, a wave per sample (waves stride the workgroup's samples).
// Either way a span [lo, hi) of elements is walked by ps_span: the elements before the first 16-byte boundary and after the last one
// one by one, those between as float4 (n1 = 663 puts the second sample 12 bytes past a boundary).  Sums are f64 per thread, wave_sum /
// block_sum, one f64 partial per workgroup (or wave) and no float atomics; the counts are integers in LDS (one histogram pair per
// wave), merged into the 512 global counters with integer atomics: exact, whatever the order.  The finish kernel (one workgroup) adds
// the partials in a fixed order and evaluates the five values and the backward's record in f64.
//
// Backward, one pass:  dpred = gmul * (c1 clamp(d, -1, 1) + c2 d + cc_b),  record = c1 | c2 | cc_0 .. cc_{B-1} (f64),
//   c1 = a1 / n,   c2 = a5 * 20 / (ln 10 * n * mse)  (0 where mse == 0: torch gives NaN there),   cc_b = -a6 sign(mean gt_b - mean pred_b) / n,
// sign(0) = 0.  The histogram term has no gradient (torch.histc is not differentiable); gt takes none.
#include "bem_common.h"

namespace {

constexpr int PS_K = 4096, PS_SMALL = PS_K / 4, PS_BINS = 256, PS_NW = 4;
constexpr int64_t PS_MAX_N = ((int64_t)1 << 32) - 1;       // the global counters are 32 bits wide
constexpr int PS_HIST_BYTES = 2 * PS_BINS * (int)sizeof(unsigned);
static_assert(PS_HIST_BYTES % sizeof(double) == 0, "the f64 partials follow the counters in the workspace");

// How a (B, n1) batch is dealt to workgroups.  small: spw samples per workgroup, else cps chunks per sample.
struct PsPlan {
    bool small;
    int64_t spw, cps, nwg, nsum;          // nsum: per-sample sum slots = B * cps (cps = 1 when small)
};
PsPlan ps_plan(int64_t B, int64_t n1) {
    PsPlan p;
    p.small = n1 <= PS_SMALL;
    p.spw = p.small ? PS_K / n1 : 1;
    p.cps = p.small ? 1 : cdiv64(n1, PS_K);
    p.nwg = p.small ? cdiv64(B, p.spw) : B * p.cps;
    p.nsum = B * p.cps;
    return p;
}

// Elements [lo, hi) by nt threads, thread t: scalar up to the first multiple of 4 (the tensors' bases are 16-byte aligned when vec),
// float4 up to the last one, scalar for the rest.  one(i, pred[i], gt[i]) returns what is stored to out[i] when STORE.
template <bool STORE, typename F>
__device__ __forceinline__ void ps_span(const float* __restrict__ pred, const float* __restrict__ gt, float* __restrict__ out, int64_t lo,
                                        int64_t hi, int t, int nt, bool vec, F&& one) {
    int64_t a = hi, b = hi;
    if (vec) {
        a = min(hi, (lo + 3) & ~(int64_t)3);
        b = a + ((hi - a) & ~(int64_t)3);
    }
    for (int64_t i = lo + t; i < a; i += nt) {
        const float r = one(i, pred[i], gt[i]);
        if (STORE) out[i] = r;
    }
    for (int64_t i = a + 4 * (int64_t)t; i < b; i += 4 * (int64_t)nt) {
        const float4 p = *reinterpret_cast<const float4*>(pred + i), g = *reinterpret_cast<const float4*>(gt + i);
        float4 r;
        r.x = one(i, p.x, g.x); r.y = one(i + 1, p.y, g.y); r.z = one(i + 2, p.z, g.z); r.w = one(i + 3, p.w, g.w);
        if (STORE) *reinterpret_cast<float4*>(out + i) = r;
    }
    for (int64_t i = b + t; i < hi; i += nt) {
        const float r = one(i, pred[i], gt[i]);
        if (STORE) out[i] = r;
    }
}

__device__ __forceinline__ void ps_count(unsigned* h, float x) {
    if (x >= 0.f && x <= 1.f) atomicAdd(h + min((int)(x * (float)PS_BINS), PS_BINS - 1), 1u);      // NaN fails both comparisons
}

// part[2 wg] = sum smooth_l1, part[2 wg + 1] = sum d^2 of the workgroup's elements; samp[2 s], samp[2 s + 1] = sum pred, sum gt of
// slot s (a chunk of a sample, or a whole small sample); hist[0..255] += counts of pred, hist[256..511] += counts of gt.
template <bool SMALL>
__global__ __launch_bounds__(64 * PS_NW) void pixstat_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  double* __restrict__ part, double* __restrict__ samp,
                                                                  unsigned* __restrict__ hist, int64_t B, int64_t n1, int64_t spw, int64_t cps,
                                                                  bool vec) {
    __shared__ unsigned sh[PS_NW][2][PS_BINS];
    __shared__ double red[PS_NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < PS_NW * 2 * PS_BINS; i += 64 * PS_NW) (&sh[0][0][0])[i] = 0u;
    __syncthreads();
    unsigned* hp = sh[wave][0];
    unsigned* hg = sh[wave][1];
    double s1 = 0.0, s2 = 0.0, sp = 0.0, sg = 0.0;
    auto one = [&](int64_t, float p, float g) {
        const double d = (double)p - (double)g, ad = fabs(d);      // exact
        s1 += ad < 1.0 ? 0.5 * d * d : ad - 0.5;
        s2 = fma(d, d, s2);
        sp += (double)p; sg += (double)g;
        ps_count(hp, p); ps_count(hg, g);
        return 0.f;
    };
    const int64_t wg = blockIdx.x;
    if (SMALL) {
        const int64_t b0 = wg * spw, b1 = min(B, b0 + spw);
        for (int64_t b = b0 + wave; b < b1; b += PS_NW) {
            sp = sg = 0.0;
            ps_span<false>(pred, gt, nullptr, b * n1, (b + 1) * n1, lane, 64, vec, one);
            const double wp = wave_sum(sp), wgt = wave_sum(sg);
            if (lane == 0) { samp[2 * b] = wp; samp[2 * b + 1] = wgt; }
        }
    } else {
        const int64_t b = wg / cps, j = wg - b * cps;
        const int64_t lo = b * n1 + j * PS_K, hi = min((b + 1) * n1, lo + PS_K);
        ps_span<false>(pred, gt, nullptr, lo, hi, t, 64 * PS_NW, vec, one);
        sp = block_sum<PS_NW>(sp, red);
        sg = block_sum<PS_NW>(sg, red);
        if (t == 0) { samp[2 * wg] = sp; samp[2 * wg + 1] = sg; }
    }
    s1 = block_sum<PS_NW>(s1, red);
    s2 = block_sum<PS_NW>(s2, red);              // its barriers also order the LDS counts before the merge below
    if (t == 0) { part[2 * wg] = s1; part[2 * wg + 1] = s2; }
    for (int i = t; i < 2 * PS_BINS; i += 64 * PS_NW) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < PS_NW; ++w) c += (&sh[w][0][0])[i];
        if (c) atomicAdd(hist + i, c);
    }
}

// out = loss | smooth_l1 | mse | psnr | color | hist (f32); rec (or NULL) = c1 | c2 | cc_b (f64).  Thread t adds the partials t, t + 256,
// ... and the samples t, t + 256, ... (each sample's cps slots in order), the 256 sums go through block_sum: the same order every call.
__global__ __launch_bounds__(256) void pixstat_finish_kernel(const double* __restrict__ part, const double* __restrict__ samp,
                                                            const unsigned* __restrict__ hist, float* __restrict__ out, double* __restrict__ rec,
                                                            int64_t nwg, int64_t B, int64_t cps, int64_t n1, double a1, double a3, double a5,
                                                            double a6) {
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double n = (double)B * (double)n1;
    double s1 = 0.0, s2 = 0.0, sc = 0.0;
    for (int64_t i = t; i < nwg; i += 256) { s1 += part[2 * i]; s2 += part[2 * i + 1]; }
    for (int64_t b = t; b < B; b += 256) {
        double sp = 0.0, sg = 0.0;
        for (int64_t j = 0; j < cps; ++j) { sp += samp[2 * (b * cps + j)]; sg += samp[2 * (b * cps + j) + 1]; }
        const double dm = (sg - sp) / (double)n1;              // one division of the difference: equal sums give exactly 0
        sc += fabs(dm);
        if (rec) rec[2 + b] = -a6 * (dm > 0.0 ? 1.0 : (dm < 0.0 ? -1.0 : 0.0)) / n;
    }
    s1 = block_sum<4>(s1, red);
    s2 = block_sum<4>(s2, red);
    sc = block_sum<4>(sc, red);
    const double np = block_sum<4>((double)hist[t], red), ng = block_sum<4>((double)hist[PS_BINS + t], red);     // 256 threads, 256 bins
    const double sh = block_sum<4>(fabs((double)hist[PS_BINS + t] / ng - (double)hist[t] / np), red);
    if (t != 0) return;
    const double sl1 = s1 / n, mse = s2 / n, psnr = 40.0 - 20.0 * log10(1.0 / sqrt(mse)), color = sc / (double)B, hd = sh / PS_BINS;
    double loss = 0.0;
    if (a1 != 0.0) loss += a1 * sl1;
    if (a3 != 0.0) loss += a3 * hd;
    if (a5 != 0.0) loss += a5 * psnr;
    if (a6 != 0.0) loss += a6 * color;
    out[0] = (float)loss; out[1] = (float)sl1; out[2] = (float)mse; out[3] = (float)psnr; out[4] = (float)color; out[5] = (float)hd;
    if (rec) {
        rec[0] = a1 / n;
        rec[1] = mse > 0.0 ? a5 * 20.0 / (2.302585092994045684 * n * mse) : 0.0;
    }
}
static_assert(PS_BINS == 256, "the finish kernel's thread t owns bin t");

template <bool SMALL>
__global__ __launch_bounds__(64 * PS_NW) void pixstat_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  const double* __restrict__ rec, float* __restrict__ dpred, int64_t B, int64_t n1,
                                                                  int64_t spw, int64_t cps, bool vec, const float* __restrict__ gmul) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float gm = gmul ? gmul[0] : 1.f;
    const double c1 = rec[0], c2 = rec[1];
    double cc = 0.0;
    // the f64 sum is rounded once, and gmul multiplies the rounded value: gmul = 3 gives 3 x the gradient exactly
    auto one = [&](int64_t, float p, float g) {
        const double d = (double)p - (double)g;
        return __fmul_rn(gm, (float)fma(c1, fmin(fmax(d, -1.0), 1.0), fma(c2, d, cc)));
    };
    const int64_t wg = blockIdx.x;
    if (SMALL) {
        const int64_t b0 = wg * spw, b1 = min(B, b0 + spw);
        for (int64_t b = b0 + wave; b < b1; b += PS_NW) {
            cc = rec[2 + b];
            ps_span<true>(pred, gt, dpred, b * n1, (b + 1) * n1, lane, 64, vec, one);
        }
    } else {
        const int64_t b = wg / cps, j = wg - b * cps;
        const int64_t lo = b * n1 + j * PS_K, hi = min((b + 1) * n1, lo + PS_K);
        cc = rec[2 + b];
        ps_span<true>(pred, gt, dpred, lo, hi, t, 64 * PS_NW, vec, one);
    }
}

int ps_check(const char* what, int64_t B, int64_t n1) {
    BEM_REQUIRE(B > 0 && n1 > 0, "%s: empty tensor (%lld samples of %lld elements)", what, (long long)B, (long long)n1);
    BEM_REQUIRE(n1 <= PS_MAX_N / B, "%s: %lld x %lld elements would overflow the 32-bit histogram counters (at most %lld per call)", what,
                (long long)B, (long long)n1, (long long)PS_MAX_N);
    return BEM_OK;
}
bool ps_aligned(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }

}  // namespace

extern "C" int bem_pixstat_loss_chunk(void) { return PS_K; }

extern "C" int64_t bem_pixstat_loss_ws_bytes(int64_t B, int64_t n1) {
    if (B <= 0 || n1 <= 0 || n1 > PS_MAX_N / B) return 0;
    const PsPlan p = ps_plan(B, n1);
    return PS_HIST_BYTES + 2 * (int64_t)sizeof(double) * (p.nwg + p.nsum);
}

extern "C" int bem_pixstat_loss_f32(const float* pred, const float* gt, float* out, double* rec, void* ws, int64_t B, int64_t n1, double a1,
                                    double a3, double a5, double a6, void* stream) {
    BEM_REQUIRE(pred && gt && out && ws, "pixstat_loss: null pointer");
    if (int rc = ps_check("pixstat_loss", B, n1)) return rc;
    BEM_REQUIRE(a1 >= 0 && a3 >= 0 && a5 >= 0 && a6 >= 0, "pixstat_loss: negative alpha (%g, %g, %g, %g)", a1, a3, a5, a6);
    const PsPlan p = ps_plan(B, n1);             // n < 2^32, samples above PS_K / 4 elements or workgroups above PS_K / 2: nwg < 2^23
    hipStream_t s = (hipStream_t)stream;
    unsigned* hist = (unsigned*)ws;
    double* part = (double*)((char*)ws + PS_HIST_BYTES);
    double* samp = part + 2 * p.nwg;
    BEM_ZERO(hist, PS_HIST_BYTES, s, "pixstat_loss");
    const bool vec = ps_aligned(pred, gt, nullptr);
    if (p.small) pixstat_fwd_kernel<true><<<(unsigned)p.nwg, 64 * PS_NW, 0, s>>>(pred, gt, part, samp, hist, B, n1, p.spw, p.cps, vec);
    else pixstat_fwd_kernel<false><<<(unsigned)p.nwg, 64 * PS_NW, 0, s>>>(pred, gt, part, samp, hist, B, n1, p.spw, p.cps, vec);
    pixstat_finish_kernel<<<1, 256, 0, s>>>(part, samp, hist, out, rec, p.nwg, B, p.cps, n1, a1, a3, a5, a6);
    return bem_check_launch("pixstat_loss");
}

extern "C" int bem_pixstat_loss_bwd_f32(const float* pred, const float* gt, const double* rec, float* dpred, int64_t B, int64_t n1,
                                        const float* gmul, void* stream) {
    BEM_REQUIRE(pred && gt && rec && dpred, "pixstat_loss_bwd: null pointer");
    if (int rc = ps_check("pixstat_loss_bwd", B, n1)) return rc;
    const PsPlan p = ps_plan(B, n1);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ps_aligned(pred, gt, dpred);
    if (p.small) pixstat_bwd_kernel<true><<<(unsigned)p.nwg, 64 * PS_NW, 0, s>>>(pred, gt, rec, dpred, B, n1, p.spw, p.cps, vec, gmul);
    else pixstat_bwd_kernel<false><<<(unsigned)p.nwg, 64 * PS_NW, 0, s>>>(pred, gt, rec, dpred, B, n1, p.spw, p.cps, vec, gmul);
    return bem_check_launch("pixstat_loss_bwd");
}
