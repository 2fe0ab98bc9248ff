// The deterministic middle of SS2D on small planes (H W <= 256; the 16x16, 8x8 and 4x4 maps of Stage I) as ONE kernel:
//   t (in_proj output) -> depthwise 3x3 + bias + SiLU -> x_proj (all four directions' rows) -> dt_proj / softplus / four-direction scan
//   -> y = (y_dir0 + y_dir2) + (y_dir1 + y_dir3), row-major.
// A sample is served by S workgroups (grid (B, S); S <= 4 for L >= 64, chosen by the host so that the launch fills the chip, 1 below): the
// scans are bound by the VALU rate of a CU (40 channels x 4 directions of E = 4 positions took 16 of the kernel's 30 us on one CU), so each
// workgroup scans C / S of the channels; conv and x_proj need every channel and are computed by each of the S workgroups (on S different
// CUs, so at no cost in time).  Every output is computed by the same instructions whatever S is.
// In a workgroup the sample's xc planes and its x_dbl rows stay in LDS, so neither xc nor x_dbl nor any transposed copy reaches memory, and
// the chain's six dependent launches are one.  The x_proj rows and the scan parameters are copied into LDS at the start as well: the
// phases below are chains of short dependent steps, and a global load inside such a step costs more than the step.  The column
// directions index the LDS planes transposed.
// No atomics: every output is written once by one thread, the result is the same bit for bit from launch to launch.
//
// Phases, a workgroup barrier between two of them:
//   1  depthwise 3x3 + bias + SiLU, t (global; 4 outputs of a row per thread from three float4 row loads and the halo columns) -> PX
//      (the expression and order per output of dwconv3x3_fast_kernel, mode 1); x_proj rows -> WX, dtw / dtb / A / Ds -> PR
//   2  x_dbl[m][p] = sum_c W[m][c] xc[c][p], f32 FMAs in ascending c with a compensated running sum -> XD (rows [dir 0 | dir 2 | dir 1 | dir 3], as the chain's GEMM)
//   3  the scans (coefficients as in ss2d_scan_rows_kernel: softplus and exp(dt A) on one base-2 logarithm)
//        E > 0 (L = 64 E): a wavefront owns a channel; lane l holds the E consecutive positions l E .. l E + E - 1 of a chain and the
//          wavefront scan links the lanes (wave_scan_affine; no cross-wave step).  Orientation 0 stays in registers, orientation 1
//          goes through the channel's own plane of PX (its x values are in registers by then) to come back in row-major order,
//          and the sum is stored.
//        E = 0 (L < 64): a lane walks the chain of one (channel, direction), 4 positions per step, into the direction's row-major
//          result plane;
//   4  E = 0 only: (plane 0 + plane 2) + (plane 1 + plane 3) -> y.
#include "scan_common.h"

namespace {

constexpr int CORE_NT = 1024;                   // 16 wavefronts: 4 per SIMD, at most 128 VGPRs each
constexpr int CORE_LDS_MAX = 160 * 1024;        // LDS of one CU (a workgroup may take all of it)

// LDS floats of one sample: PX (and the four directions' result planes and a 64-entry index table for L < 64) of C L each, XD of 4 (R + 2) L, WX of 4 (R + 2) C, PR of 4 C (R + 3)
__host__ __device__ inline int64_t core_lds_floats(int C, int L, int R) {
    return (L < 64 ? (int64_t)5 * C * L + 64 : (int64_t)C * L) + (int64_t)4 * (R + 2) * (L + C) + (int64_t)4 * C * (R + 3);
}

// the LDS index of scan position q of orientation o (0: row-major, 1: column-major q = col H + row)
__device__ __forceinline__ int core_idx(int q, int o, int H, int W) {
    if (!o) return q;
    const int col = q / H;
    return (q - col * H) * W + col;
}

// Coefficients of G positions (LDS indices idx) of direction k = o + 2 dir of channel c: a = exp(dl A), bb = dl B x, cv = C.
// xd: the direction's (R + 2) rows of XD.
// RT: dt_rank when known at compile time (the R + 2 rows' LDS reads then go out together), 0 = runtime R.
template <int G, int RT>
__device__ __forceinline__ void core_coeffs(const float* xd, const Ss2dDir p, int L, int Rr, const int (&idx)[G], const float (&xv)[G],
                                            float (&a)[G], float (&bb)[G], float (&cv)[G]) {
    const int R = RT ? RT : Rr;
    const float dtb0 = valu_copy(p.dtb);
#pragma unroll
    for (int e = 0; e < G; ++e) a[e] = dtb0;
    auto row = [&](int r) {
        const float w = valu_copy(p.wdt[r]);
#pragma unroll
        for (int e = 0; e < G; ++e) a[e] = fmaf(w, valu_copy(xd[r * L + idx[e]]), a[e]);
    };
    if constexpr (RT > 0) {
#pragma unroll
        for (int r = 0; r < RT; ++r) row(r);
    } else {
        for (int r = 0; r < R; ++r) row(r);
    }
    const float Ak = valu_copy(*p.A);
#pragma unroll
    for (int e = 0; e < G; ++e) {
        const float Bv = valu_copy(xd[R * L + idx[e]]);
        cv[e] = valu_copy(xd[(R + 1) * L + idx[e]]);
        const float lg = softplus_log2(a[e]);          // softplus and exp(dt A) share the base-2 logarithm
        const float dl = lg * BEM_LN2;
        a[e] = __builtin_amdgcn_exp2f(lg * Ak);
        bb[e] = dl * Bv * xv[e];
    }
}

// One direction of a wavefront-owned chain (E positions per lane, scan order = lane order): y = C h + D x, set (REV = false) or added.
template <int E, int RT, bool REV>
__device__ __forceinline__ void core_wave_dir(const float* xd, const Ss2dDir p, int L, int R, const int (&idx)[E], const float (&xv)[E],
                                              float (&y)[E]) {
    float a[E], bb[E], cv[E];
    core_coeffs<E, RT>(xd, p, L, R, idx, xv, a, bb, cv);
    float P = 1.f, S = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = REV ? E - 1 - i : i;
        S = fmaf(a[e], S, bb[e]);
        P = P * a[e];
    }
    const float Dk = valu_copy(p.D);
    float Pe, Se;
    wave_scan_affine<REV>(P, S, Pe, Se);
    float hh = Se;                                     // the chain starts from h = 0
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = REV ? E - 1 - i : i;
        hh = fmaf(a[e], hh, bb[e]);
        const float yv = fmaf(cv[e], hh, Dk * xv[e]);
        y[e] = REV ? y[e] + yv : yv;
    }
}

// A lane-owned chain of L positions (L % 4 == 0), 4 per step, into dst, the direction's row-major result plane.  tr: the LDS index of
// column-major position q (orientation 1), null for orientation 0.
template <int RT, bool REV>
__device__ __forceinline__ void core_lane_dir(const float* xd, const Ss2dDir p, const float* xpl, float* dst, int L, int R, const int* tr) {
    float hh = 0.f;
    const float Dk = valu_copy(p.D);
    for (int j = 0; j < L; j += 4) {
        const int q0 = REV ? L - 4 - j : j;
        int idx[4];
        float xv[4], a[4], bb[4], cv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            idx[e] = tr ? tr[q0 + e] : q0 + e;
            xv[e] = valu_copy(xpl[idx[e]]);
        }
        core_coeffs<4, RT>(xd, p, L, R, idx, xv, a, bb, cv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = REV ? 3 - i : i;
            hh = fmaf(a[e], hh, bb[e]);
            dst[idx[e]] = fmaf(cv[e], hh, Dk * xv[e]);
        }
    }
}

template <int E, int RT>
__global__ __launch_bounds__(CORE_NT) void ss2d_core_small_kernel(
    const float* __restrict__ t, const float* __restrict__ dww, int64_t dww_bs, const float* __restrict__ dwb, int64_t dwb_bs,
    const float* __restrict__ xw, const float* __restrict__ dtw, const float* __restrict__ dtb, const float* __restrict__ A,
    const float* __restrict__ Ds, float* __restrict__ y, int C, int H, int W, int Rr) {
    // this workgroup's channels of the scans: [c_lo, c_hi)
    const int c_lo = (int)(blockIdx.y * C / gridDim.y), c_hi = (int)((blockIdx.y + 1) * C / gridDim.y);
    extern __shared__ __attribute__((aligned(16))) float core_sm[];
    const int R = RT ? RT : Rr;
    const int L = H * W, CL = C * L, M = R + 2;
    float* PX = core_sm;
    float* XD = PX + CL;
    float* WX = XD + 4 * M * L;
    float* PR = WX + 4 * M * C;                        // dtw (4 C R) | dtb (4 C) | A (4 C) | Ds (4 C)
    float* PK = PR + 4 * C * (R + 3);                  // E == 0 only: the result planes of directions 0 .. 3, then the index table
    int* TR = reinterpret_cast<int*>(PK + 4 * CL);
    const float *Pdtw = PR, *Pdtb = PR + 4 * C * R, *PAk = Pdtb + 4 * C, *PDs = PAk + 4 * C;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float* tb = t + b * CL;
    float* yb = y + b * CL;

    // ---- 1: depthwise 3x3 + bias + SiLU: a thread takes 4 outputs of a row (W % 4 == 0).  Rows and columns outside the plane are read
    // at a clamped address and dropped.  The parameter copies go out first: every load of this phase is in flight at once.
    for (int i = tid * 4; i < 4 * M * C; i += CORE_NT * 4) *reinterpret_cast<float4*>(WX + i) = *reinterpret_cast<const float4*>(xw + i);
    for (int i = tid; i < 4 * C * R; i += CORE_NT) PR[i] = dtw[i];
    for (int i = tid; i < 4 * C; i += CORE_NT) {
        PR[4 * C * R + i] = dtb[i];
        PR[4 * C * (R + 1) + i] = A[i];
        PR[4 * C * (R + 2) + i] = Ds[i];
    }
    if (E == 0 && tid < L) TR[tid] = core_idx(tid, 1, H, W);
    {
        const float* wb = dww + b * dww_bs;
        const float* bb = dwb ? dwb + b * dwb_bs : nullptr;
        // per = H W / 4 <= 64 threads cover a plane: thread -> (row, column quad) once, then channels tid / per, + CORE_NT / per, ...
        const int W4 = W >> 2, per = H * W4, cstep = CORE_NT / per, cfirst = tid / per, rem = tid - cfirst * per, py = rem / W4, x0 = (rem - py * W4) * 4;
        for (int c = cfirst; c < C && cfirst < cstep; c += cstep) {
            const float* pl = tb + c * L;
            const float* w9 = wb + c * 9;
            float4 q[3];
            float hl[3], hr[3], wk[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float* row = pl + min(max(py + ky - 1, 0), H - 1) * W;
                q[ky] = *reinterpret_cast<const float4*>(row + x0);
                hl[ky] = row[max(x0 - 1, 0)];
                hr[ky] = row[min(x0 + 4, W - 1)];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) wk[k] = w9[k];
            const float bv = bb ? bb[c] : 0.f;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = py + ky - 1;
                const bool rin = yy >= 0 && yy < H;
                const float v[6] = {rin && x0 > 0 ? hl[ky] : 0.f, rin ? q[ky].x : 0.f, rin ? q[ky].y : 0.f, rin ? q[ky].z : 0.f, rin ? q[ky].w : 0.f,
                                    rin && x0 + 4 < W ? hr[ky] : 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk[ky * 3], v[j], fmaf(wk[ky * 3 + 1], v[j + 1], fmaf(wk[ky * 3 + 2], v[j + 2], acc[j])));
            }
            *reinterpret_cast<float4*>(PX + c * L + py * W + x0) = make_float4(bem_silu(acc[0] + bv), bem_silu(acc[1] + bv), bem_silu(acc[2] + bv), bem_silu(acc[3] + bv));
        }
    }
    __syncthreads();

    // ---- 2: x_proj.  A work item is 4 consecutive rows of one position; the weight rows are read as float4 over c (C % 4 == 0).
    for (int it = tid; it < M * L; it += CORE_NT) {
        const int q = it / L, p = it - q * L;
        const float* w0 = WX + 4 * q * C;
        // ascending c, four products per step; the steps' sums are added with a compensation term (Kahan).  One FMA chain over all of c
        // put the B and C rows 2.2x (mean) / 4.6x (max) further from float64 than the chain's matrix-core GEMM at C = 160 (the error of
        // a running sum grows with its length; a dt near 25 carries the rows' error into y undamped).
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, cmp[4] = {0.f, 0.f, 0.f, 0.f};
        auto step = [&](int c) {
            float xv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[j] = valu_copy(PX[(c + j) * L + p]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 wq = *reinterpret_cast<const float4*>(w0 + i * C + c);
                const float s = fmaf(valu_copy(wq.w), xv[3], fmaf(valu_copy(wq.z), xv[2], fmaf(valu_copy(wq.y), xv[1], valu_copy(wq.x) * xv[0])));
                const float yk = s - cmp[i], tt = acc[i] + yk;
                cmp[i] = (tt - acc[i]) - yk;
                acc[i] = tt;
            }
        };
        int c = 0;
        for (; c + 8 <= C; c += 8) {        // two steps per trip: the second step's LDS reads go out under the first one's arithmetic
            step(c);
            step(c + 4);
        }
        if (c < C) step(c);
#pragma unroll
        for (int i = 0; i < 4; ++i) XD[(4 * q + i) * L + p] = acc[i];
    }
    __syncthreads();

    // ---- 3: the scans.  XD blocks of M rows: [dir 0 | dir 2 | dir 1 | dir 3] = block 2 o + dir of direction k = o + 2 dir
    if constexpr (E > 0) {
        const int lane = tid & (BEM_WAVE - 1);
        const int wave = __builtin_amdgcn_readfirstlane(tid / BEM_WAVE);
        int idx0[E], idx1[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            idx0[e] = lane * E + e;
            idx1[e] = core_idx(lane * E + e, 1, H, W);
        }
        for (int c = c_lo + wave; c < c_hi; c += CORE_NT / BEM_WAVE) {         // wave-uniform: every lane of the wavefront scan is active
            float* xpl = PX + c * L;                                 // read and, for the exchange below, rewritten by this wavefront alone
            float x0[E], x1[E], y0[E], y1[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                x0[e] = valu_copy(xpl[idx0[e]]);
                x1[e] = valu_copy(xpl[idx1[e]]);
            }
            core_wave_dir<E, RT, false>(XD, ss2d_dir(Pdtw, Pdtb, PAk, PDs, 0, C, c, R), L, R, idx0, x0, y0);
            core_wave_dir<E, RT, true>(XD + M * L, ss2d_dir(Pdtw, Pdtb, PAk, PDs, 2, C, c, R), L, R, idx0, x0, y0);
            core_wave_dir<E, RT, false>(XD + 2 * M * L, ss2d_dir(Pdtw, Pdtb, PAk, PDs, 1, C, c, R), L, R, idx1, x1, y1);
            core_wave_dir<E, RT, true>(XD + 3 * M * L, ss2d_dir(Pdtw, Pdtb, PAk, PDs, 3, C, c, R), L, R, idx1, x1, y1);
#pragma unroll
            for (int e = 0; e < E; ++e) xpl[idx1[e]] = y1[e];
            // the lanes of one wavefront exchange through LDS: order the stores above before the loads below
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = y0[e] + valu_copy(xpl[idx0[e]]);
            float* dst = yb + c * L + lane * E;
            if (E == 4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            else if (E == 2) *reinterpret_cast<float2*>(dst) = make_float2(o[0], o[1]);
            else dst[0] = o[0];
        }
    } else {
        const int Cs = c_hi - c_lo;
        for (int u = tid; u < 4 * Cs; u += CORE_NT) {
            const int k = u / Cs, c = c_lo + u - k * Cs, o = k & 1, dir = k >> 1;
            const float* xd = XD + (2 * o + dir) * M * L;
            const Ss2dDir p = ss2d_dir(Pdtw, Pdtb, PAk, PDs, k, C, c, R);
            if (dir) core_lane_dir<RT, true>(xd, p, PX + c * L, PK + k * CL + c * L, L, R, o ? TR : nullptr);
            else core_lane_dir<RT, false>(xd, p, PX + c * L, PK + k * CL + c * L, L, R, o ? TR : nullptr);
        }
        __syncthreads();
        // ---- 4
        for (int i = c_lo * L + tid * 4; i < c_hi * L; i += CORE_NT * 4) {
            float v[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 q = *reinterpret_cast<const float4*>(PK + k * CL + i);
                v[k][0] = valu_copy(q.x); v[k][1] = valu_copy(q.y); v[k][2] = valu_copy(q.z); v[k][3] = valu_copy(q.w);
            }
            *reinterpret_cast<float4*>(yb + i) = make_float4((v[0][0] + v[2][0]) + (v[1][0] + v[3][0]), (v[0][1] + v[2][1]) + (v[1][1] + v[3][1]),
                                                             (v[0][2] + v[2][2]) + (v[1][2] + v[3][2]), (v[0][3] + v[2][3]) + (v[1][3] + v[3][3]));
        }
    }
}

}  // namespace

// d_state 1; W % 4 == 0 (float4 rows); L = H W is 64, 128 or 256 (a wavefront per chain) or below 64 (a lane per chain); C % 4 == 0 (float4
// weight rows); the sample's plane sets, x_dbl rows, x_proj rows and scan parameters within one CU's LDS.
extern "C" int bem_ss2d_core_small_supported(int C, int H, int W, int R) {
    if (C <= 0 || H <= 0 || W <= 0 || R < 1 || C % 4 != 0 || W % 4 != 0 || H > 256 || W > 256) return 0;
    const int L = H * W;
    if (!(L < 64 || L == 64 || L == 128 || L == 256)) return 0;
    return core_lds_floats(C, L, R) * (int64_t)sizeof(float) <= CORE_LDS_MAX;
}

extern "C" int bem_ss2d_core_small_f32(const float* t, const float* dww, int64_t dww_bstride, const float* dwb, int64_t dwb_bstride,
                                       const float* xw, const float* dtw, const float* dtb, const float* A, const float* Ds, float* y,
                                       int B, int C, int H, int W, int R, void* stream) {
    BEM_REQUIRE(t && dww && xw && dtw && dtb && A && Ds && y, "ss2d_core_small: null tensor");
    BEM_REQUIRE(B >= 0 && B <= INT_MAX / 4 && H > 0 && W > 0, "ss2d_core_small: bad shape");
    BEM_REQUIRE(bem_ss2d_core_small_supported(C, H, W, R), "ss2d_core_small: unsupported C=%d plane %dx%d dt_rank %d", C, H, W, R);
    BEM_REQUIRE(dww_bstride == 0 || dww_bstride >= (int64_t)C * 9, "ss2d_core_small: depthwise weight batch stride");
    BEM_REQUIRE(!dwb || dwb_bstride == 0 || dwb_bstride >= C, "ss2d_core_small: depthwise bias batch stride");
    BEM_REQUIRE((((uintptr_t)t | (uintptr_t)y | (uintptr_t)xw) & 15) == 0, "ss2d_core_small: 16-byte alignment");
    if (B == 0) return BEM_OK;
    const int L = H * W;
    const size_t lds = (size_t)core_lds_floats(C, L, R) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    // workgroups per sample: up to 4, as long as the launch stays within the 256 CUs (B = 64 in the eval step: 4).  One for L < 64: there the
    // copies of the x_proj rows and scan parameters are most of a workgroup's traffic (C = 160, 4x4: 64 KB against 10 KB of t), and four
    // of them per sample cost more than the shorter scan phase returns (B = 64: 33.5 us against 28.2 us with one)
    const int S = (L < 64 || B >= 256) ? 1 : (256 / B < 4 ? 256 / B : 4);
#define BEM_CORE(EE, RT) do { set_max_dynamic_lds<&ss2d_core_small_kernel<EE, RT>>(CORE_LDS_MAX);                                       \
        ss2d_core_small_kernel<EE, RT><<<dim3(B, S), CORE_NT, lds, s>>>(t, dww, dww_bstride, dwb, dwb_bstride, xw, dtw, dtb, A, Ds, y, C, H, W, R); } while (0)
    // the dt_ranks of Stage I's three levels (n_feat 40: C = 40 / 80 / 160 at 16x16 / 8x8 / 4x4) are compile-time constants of their forms
    if (L == 256 && R == 3) BEM_CORE(4, 3);
    else if (L == 256) BEM_CORE(4, 0);
    else if (L == 128) BEM_CORE(2, 0);
    else if (L == 64 && R == 5) BEM_CORE(1, 5);
    else if (L == 64) BEM_CORE(1, 0);
    else if (R == 10) BEM_CORE(0, 10);
    else BEM_CORE(0, 0);
#undef BEM_CORE
    return bem_check_launch("ss2d_core_small");
}
