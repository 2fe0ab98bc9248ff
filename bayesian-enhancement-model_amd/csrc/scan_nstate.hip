// Fused SS2D scan for d_state = N > 1 (1 <= N <= 16), forward and backward: the general state size of VMamba's SS2D
// (vmamba.py:251-253, 345-346, 660-671).  Operand layout of bem_ss2d_scan_strided_f32 except that the x_dbl rows of a direction
// are [dt_0..dt_{R-1}, B_0..B_{N-1}, C_0..C_{N-1}] and A is (4C, N).  d_state = 1 keeps the kernels of scan.hip / scan_bwd.hip.
//
// Structure: one wavefront per channel, a workgroup of CB wavefronts per CB channels of one (orientation, image).  A tile is the
// 64 * E consecutive positions the wavefront covers at once; its R + 2N x_dbl rows (dt, B, C) are the same for every channel of the
// image, so the workgroup stages them in LDS once and all CB wavefronts read them there (CB times fewer x_dbl reads than a
// workgroup per channel).  A wavefront scans its own channel with the DPP wavefront scan of scan_common.h, one state after the
// other; the N carries linking successive tiles are wave-uniform registers (NM = 4 / 8 / 16 slots, N of them used).  No cross-wave
// scan, so the only barriers are the two of the LDS staging per tile.
//
// Backward per direction:
//   pass 1  tiles in scan order: the forward states entering every tile (N floats per tile and channel) go to a workspace;
//   pass 2  tiles in reverse scan order: h is rebuilt from the tile's entry states, the adjoint runs as the reverse scan
//           u_t = a_t (C_t dy_t + u_{t+1}), dh_t = C_t dy_t + u_{t+1}, and the x_dbl gradients of the CB channels (dt rows:
//           dz w_r, B rows: dh dl x, C rows: dy h) are summed in an LDS tile before one contiguous global atomic per element.
#include "scan_common.h"

namespace {

constexpr int SN_RMAX = 16;      // dt_rank limit (d_inner <= 256 with dt_rank "auto")
constexpr int SN_NMAX = 16;      // d_state limit

// rows [r0, r1) of a tile of T positions starting at t0 into LDS (zero past L)
template <int T, int NT>
__device__ __forceinline__ void stage_rows(float* __restrict__ tile, const float* __restrict__ xd, int r0, int r1, int64_t t0, int L, bool vec) {
    constexpr int Q = T / 4;
    const int n = (r1 - r0) * Q;
    for (int i = threadIdx.x; i < n; i += NT) {
        const int r = r0 + i / Q, q = i % Q;
        const int64_t t = t0 + 4 * q;
        const float* p = xd + (int64_t)r * L + t;
        float4 v;
        if (vec && t + 4 <= L) v = *reinterpret_cast<const float4*>(p);
        else {
            v.x = t < L ? p[0] : 0.f; v.y = t + 1 < L ? p[1] : 0.f;
            v.z = t + 2 < L ? p[2] : 0.f; v.w = t + 3 < L ? p[3] : 0.f;
        }
        *reinterpret_cast<float4*>(tile + r * T + 4 * q) = v;
    }
}

template <int E>
__device__ __forceinline__ void lds_row(const float* __restrict__ p, float (&v)[E]) {
#pragma unroll
    for (int i = 0; i < E; i += 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
    }
}

// (P, S) of this lane's E maps composed in scan order, then the wavefront scan: returns the state entering the lane's first
// element and advances `carry` to the state leaving the tile.
template <int E, bool REV>
__device__ __forceinline__ float wave_enter(const float (&a)[E], const float (&b)[E], float& carry) {
    float P = 1.f, S = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = REV ? E - 1 - i : i;
        S = fmaf(a[e], S, b[e]);
        P = P * a[e];
    }
    float Pe, Se;
    wave_scan_affine<REV>(P, S, Pe, Se);
    const float Pt = lane_bcast(P, REV ? 0 : BEM_WAVE - 1), St = lane_bcast(S, REV ? 0 : BEM_WAVE - 1);
    const float c0 = carry;
    carry = fmaf(Pt, c0, St);
    return fmaf(Pe, c0, Se);
}

// dt of this lane's E positions: dtb + sum_r w_r dt_row_r (rows from the LDS tile)
template <int E, int T>
__device__ __forceinline__ void tile_dt(const float* __restrict__ tile, const float* __restrict__ wdt, float dtb, int R, int lane, float (&z)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) z[e] = dtb;
    for (int r = 0; r < R; ++r) {
        float v[E];
        lds_row<E>(tile + r * T + lane * E, v);
        const float w = wdt[r];
#pragma unroll
        for (int e = 0; e < E; ++e) z[e] = fmaf(w, v[e], z[e]);
    }
}

template <int NM, int E, int CB, bool REV>
__device__ __forceinline__ void scan_n_dir(float* tile, const float* __restrict__ xr, const float* __restrict__ xd, float* __restrict__ yr,
                                           const float* __restrict__ wdt, float dtb, const float* __restrict__ Ak, float Dk, bool live,
                                           int L, int R, int N) {
    constexpr int T = 64 * E, NT = CB * 64;
    const int lane = threadIdx.x & 63;
    const bool vec = (L % 4 == 0);
    const int ntiles = (L + T - 1) / T, rows = R + 2 * N;
    float A[NM], carry[NM];
#pragma unroll
    for (int n = 0; n < NM; ++n) {
        A[n] = n < N ? Ak[n] : 0.f;
        carry[n] = 0.f;
    }
    for (int jj = 0; jj < ntiles; ++jj) {
        const int j = REV ? ntiles - 1 - jj : jj;
        const int64_t t0 = (int64_t)j * T, te = t0 + lane * E;
        __syncthreads();                                     // every wavefront is done with the previous tile
        stage_rows<T, NT>(tile, xd, 0, rows, t0, L, vec);
        __syncthreads();
        if (!live) continue;                                 // wave-uniform: channel slot past C
        float x[E], dl[E], dlx[E], y[E];
        load_row<E>(xr, te, L, vec, x);
        tile_dt<E, T>(tile, wdt, dtb, R, lane, dl);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            dl[e] = bem_softplus(dl[e]);
            dlx[e] = dl[e] * x[e];
        }
        if (REV) load_row<E>(yr, te, L, vec, y);             // this lane's own stores of the forward direction
#pragma unroll
        for (int e = 0; e < E; ++e) y[e] = REV ? fmaf(Dk, x[e], y[e]) : Dk * x[e];
#pragma unroll
        for (int n = 0; n < NM; ++n) {
            if (n >= N) continue;
            float Bv[E], Cv[E], a[E], bb[E];
            lds_row<E>(tile + (R + n) * T + lane * E, Bv);
            lds_row<E>(tile + (R + N + n) * T + lane * E, Cv);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool ok = te + e < L;
                a[e] = ok ? bem_fexp(dl[e] * A[n]) : 1.f;
                bb[e] = ok ? dlx[e] * Bv[e] : 0.f;
            }
            float hh = wave_enter<E, REV>(a, bb, carry[n]);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int e = REV ? E - 1 - i : i;
                hh = fmaf(a[e], hh, bb[e]);
                y[e] = fmaf(Cv[e], hh, y[e]);
            }
        }
        store_row<E>(yr, te, L, vec, y);
    }
}

// grid (ceil(C / CB) * B * 2), CB wavefronts, dynamic LDS (R + 2N) * 64E floats
template <int NM, int E, int CB>
__global__ __launch_bounds__(CB * 64) void ss2d_scan_n_kernel(
    const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ xd0, const float* __restrict__ xd1,
    const float* __restrict__ dtw, const float* __restrict__ dtb, const float* __restrict__ A, const float* __restrict__ Ds,
    float* __restrict__ y0, float* __restrict__ y1, int Bn, int C, int L, int R, int N, int64_t xbs0, int64_t xbs1) {
    extern __shared__ float tile[];
    const int G = (C + CB - 1) / CB, wi = blockIdx.x;
    const int g = wi % G, b = (wi / G) % Bn, o = wi / (G * Bn);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = g * CB + wave;
    const bool live = c < C;
    const int cc = live ? c : C - 1;                         // parameter reads of an idle slot stay in bounds
    const int64_t row = ((int64_t)b * C + cc) * L;
    const float* xr = (o ? x1 : x0) + row;
    float* yr = (o ? y1 : y0) + row;
    const float* xd = o ? xd1 + (int64_t)b * xbs1 : xd0 + (int64_t)b * xbs0;
    const int kf = o, kr = o + 2;
    scan_n_dir<NM, E, CB, false>(tile, xr, xd, yr, dtw + ((int64_t)kf * C + cc) * R, dtb[kf * C + cc], A + ((int64_t)kf * C + cc) * N,
                                 Ds[kf * C + cc], live, L, R, N);
    scan_n_dir<NM, E, CB, true>(tile, xr, xd + (int64_t)(R + 2 * N) * L, yr, dtw + ((int64_t)kr * C + cc) * R, dtb[kr * C + cc],
                                A + ((int64_t)kr * C + cc) * N, Ds[kr * C + cc], live, L, R, N);
}

// ------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------
template <int NM, int E, int CB, bool REV>
__device__ __forceinline__ void scan_n_dir_bwd(float* tile, float* acc, float* accw, const float* __restrict__ xr, const float* __restrict__ dyr,
                                               const float* __restrict__ xd, float* __restrict__ dxd, float* __restrict__ dxr, float* __restrict__ cws,
                                               const float* __restrict__ wdt, float dtb, const float* __restrict__ Ak, float Dk, bool live, bool first,
                                               int L, int R, int N, float* dAlog_p, float* dDs_p, float* ddtb_p, float* ddtw_p) {
    constexpr int T = 64 * E, NT = CB * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool vec = (L % 4 == 0);
    const int ntiles = (L + T - 1) / T, rows = R + 2 * N;
    float A[NM], carry[NM];
#pragma unroll
    for (int n = 0; n < NM; ++n) {
        A[n] = n < N ? Ak[n] : 0.f;
        carry[n] = 0.f;
    }
    // ---- pass 1: forward states entering every tile (dt and B rows only) ----
    for (int jj = 0; jj < ntiles; ++jj) {
        const int j = REV ? ntiles - 1 - jj : jj;
        const int64_t t0 = (int64_t)j * T, te = t0 + lane * E;
        __syncthreads();
        stage_rows<T, NT>(tile, xd, 0, R + N, t0, L, vec);
        __syncthreads();
        if (!live) continue;
        if (lane == 0) {
#pragma unroll
            for (int n = 0; n < NM; ++n)
                if (n < N) cws[(int64_t)j * N + n] = carry[n];
        }
        float x[E], dl[E], dlx[E];
        load_row<E>(xr, te, L, vec, x);
        tile_dt<E, T>(tile, wdt, dtb, R, lane, dl);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            dl[e] = bem_softplus(dl[e]);
            dlx[e] = dl[e] * x[e];
        }
#pragma unroll
        for (int n = 0; n < NM; ++n) {
            if (n >= N) continue;
            float Bv[E], a[E], bb[E];
            lds_row<E>(tile + (R + n) * T + lane * E, Bv);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool ok = te + e < L;
                a[e] = ok ? bem_fexp(dl[e] * A[n]) : 1.f;
                bb[e] = ok ? dlx[e] * Bv[e] : 0.f;
            }
            (void)wave_enter<E, REV>(a, bb, carry[n]);
        }
    }
    // ---- pass 2: tiles in reverse scan order ----
    float dA[NM];
#pragma unroll
    for (int n = 0; n < NM; ++n) {
        dA[n] = 0.f;
        carry[n] = 0.f;                                      // now the adjoint carry u entering the tile from its successor
    }
    if (threadIdx.x < CB * SN_RMAX) accw[threadIdx.x] = 0.f;
    float accD = 0.f, accB = 0.f;
    for (int jj = ntiles - 1; jj >= 0; --jj) {
        const int j = REV ? ntiles - 1 - jj : jj;
        const int64_t t0 = (int64_t)j * T, te = t0 + lane * E;
        __syncthreads();                                     // previous tile: staged rows read, acc flushed
        stage_rows<T, NT>(tile, xd, 0, rows, t0, L, vec);
        for (int i = threadIdx.x; i < rows * T / 4; i += NT) reinterpret_cast<float4*>(acc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        if (live) {
            float x[E], dy[E], dl[E], dlx[E], sg[E], dx[E], ddl[E];
            load_row<E>(xr, te, L, vec, x);
            load_row<E>(dyr, te, L, vec, dy);
            tile_dt<E, T>(tile, wdt, dtb, R, lane, dl);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float z = dl[e];
                sg[e] = z <= 20.f ? 1.f / (1.f + bem_fexp(-z)) : 1.f;
                dl[e] = bem_softplus(z);
                dlx[e] = dl[e] * x[e];
                dx[e] = Dk * dy[e];
                ddl[e] = 0.f;
                if (te + e < L) {
                    accD = fmaf(dy[e], x[e], accD);
                }
            }
#pragma unroll
            for (int n = 0; n < NM; ++n) {
                if (n >= N) continue;
                const float cin = cws[(int64_t)j * N + n];
                float Bv[E], Cv[E], a[E], bb[E], hm[E], h[E], ar[E], br[E];
                lds_row<E>(tile + (R + n) * T + lane * E, Bv);
                lds_row<E>(tile + (R + N + n) * T + lane * E, Cv);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const bool ok = te + e < L;
                    a[e] = ok ? bem_fexp(dl[e] * A[n]) : 1.f;
                    bb[e] = ok ? dlx[e] * Bv[e] : 0.f;
                    ar[e] = a[e];
                    br[e] = a[e] * Cv[e] * dy[e];
                }
                float cf = cin;
                float hh = wave_enter<E, REV>(a, bb, cf);
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const int e = REV ? E - 1 - i : i;
                    hm[e] = hh;
                    hh = fmaf(a[e], hh, bb[e]);
                    h[e] = hh;
                }
                float u = wave_enter<E, !REV>(ar, br, carry[n]);
                float dB[E], dC[E];
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const int e = REV ? i : E - 1 - i;      // reverse scan order
                    const float dh = fmaf(Cv[e], dy[e], u);
                    u = a[e] * dh;
                    const float dhd = dh * dl[e];
                    dx[e] = fmaf(dhd, Bv[e], dx[e]);
                    ddl[e] = fmaf(dh, fmaf(Bv[e], x[e], A[n] * a[e] * hm[e]), ddl[e]);
                    dA[n] = fmaf(dhd, a[e] * hm[e], dA[n]);
                    dB[e] = dh * dlx[e];
                    dC[e] = dy[e] * h[e];
                }
                float* pb = acc + (R + n) * T + lane * E;
                float* pc = acc + (R + N + n) * T + lane * E;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    atomicAdd(pb + e, dB[e]);
                    atomicAdd(pc + e, dC[e]);
                }
            }
            float dz[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                dz[e] = te + e < L ? ddl[e] * sg[e] : 0.f;
                accB += dz[e];
            }
            for (int r = 0; r < R; ++r) {
                float v[E];
                lds_row<E>(tile + r * T + lane * E, v);
                const float w = wdt[r];
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    s = fmaf(dz[e], v[e], s);
                    atomicAdd(acc + r * T + lane * E + e, dz[e] * w);
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, BEM_WAVE);
                if (lane == 0) accw[wave * SN_RMAX + r] += s;
            }
            if (!first) {
                float prev[E];
                load_row<E>(dxr, te, L, vec, prev);
#pragma unroll
                for (int e = 0; e < E; ++e) dx[e] += prev[e];
            }
            store_row<E>(dxr, te, L, vec, dx);
        }
        __syncthreads();                                     // the CB channels' x_dbl gradients of the tile are in acc
        for (int i = threadIdx.x; i < rows * T; i += NT) {
            const int r = i / T, q = i % T;
            if (t0 + q < L) atomicAdd(dxd + (int64_t)r * L + t0 + q, acc[i]);
        }
    }
    if (live) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            accD += __shfl_xor(accD, d, BEM_WAVE);
            accB += __shfl_xor(accB, d, BEM_WAVE);
        }
#pragma unroll
        for (int n = 0; n < NM; ++n) {
            if (n >= N) continue;
            float s = dA[n];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, BEM_WAVE);
            if (lane == 0) atomicAdd(dAlog_p + n, s * A[n]);   // A = -exp(A_logs): dA_logs = dA * A
        }
        if (lane == 0) {
            atomicAdd(dDs_p, accD);
            atomicAdd(ddtb_p, accB);
        }
        if (lane < R) atomicAdd(ddtw_p + lane, accw[wave * SN_RMAX + lane]);
    }
}

// dynamic LDS: 2 (R + 2N) * 64E floats (staged rows + gradient sums) + CB * SN_RMAX (per-wavefront ddtw sums)
template <int NM, int E, int CB>
__global__ __launch_bounds__(CB * 64) void ss2d_scan_n_bwd_kernel(
    const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ xd0, const float* __restrict__ xd1,
    const float* __restrict__ dy0, const float* __restrict__ dy1, const float* __restrict__ dtw, const float* __restrict__ dtb,
    const float* __restrict__ A, const float* __restrict__ Ds, float* __restrict__ dx0, float* __restrict__ dx1,
    float* __restrict__ dxd0, float* __restrict__ dxd1, float* __restrict__ dAlog, float* __restrict__ dDs, float* __restrict__ ddtw,
    float* __restrict__ ddtb, float* __restrict__ ws, int Bn, int C, int L, int R, int N, int64_t xbs0, int64_t xbs1) {
    extern __shared__ float lds[];
    constexpr int T = 64 * E;
    const int rows = R + 2 * N;
    float* tile = lds;
    float* acc = lds + rows * T;
    float* accw = acc + rows * T;
    const int G = (C + CB - 1) / CB, wi = blockIdx.x;
    const int g = wi % G, b = (wi / G) % Bn, o = wi / (G * Bn);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = g * CB + wave;
    const bool live = c < C;
    const int cc = live ? c : C - 1;
    const int64_t row = ((int64_t)b * C + cc) * L;
    const float* xr = (o ? x1 : x0) + row;
    const float* dyr = (o ? dy1 : dy0) + row;
    float* dxr = (o ? dx1 : dx0) + row;
    const float* xd = o ? xd1 + (int64_t)b * xbs1 : xd0 + (int64_t)b * xbs0;
    float* dxd = (o ? dxd1 : dxd0) + (int64_t)b * 2 * rows * L;
    const int64_t ntiles = (L + T - 1) / T;
    float* cws = ws + (((int64_t)o * Bn + b) * C + cc) * ntiles * N;   // entry states of every tile, one direction at a time
    const int kf = o, kr = o + 2;
    scan_n_dir_bwd<NM, E, CB, false>(tile, acc, accw, xr, dyr, xd, dxd, dxr, cws, dtw + ((int64_t)kf * C + cc) * R, dtb[kf * C + cc],
                                     A + ((int64_t)kf * C + cc) * N, Ds[kf * C + cc], live, true, L, R, N, dAlog + ((int64_t)kf * C + cc) * N,
                                     dDs + kf * C + cc, ddtb + kf * C + cc, ddtw + ((int64_t)kf * C + cc) * R);
    scan_n_dir_bwd<NM, E, CB, true>(tile, acc, accw, xr, dyr, xd + (int64_t)rows * L, dxd + (int64_t)rows * L, dxr, cws,
                                    dtw + ((int64_t)kr * C + cc) * R, dtb[kr * C + cc], A + ((int64_t)kr * C + cc) * N, Ds[kr * C + cc], live,
                                    false, L, R, N, dAlog + ((int64_t)kr * C + cc) * N, dDs + kr * C + cc, ddtb + kr * C + cc,
                                    ddtw + ((int64_t)kr * C + cc) * R);
}

constexpr int SN_E = 4;          // positions per lane: 256-position tiles, float4 rows
constexpr int SN_CB = 8;         // channels (wavefronts) per workgroup: divides the n_feat-40 widths 40 / 80 / 160

template <int NM>
static int launch_fwd(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dtw, const float* dtb, const float* A,
                      const float* Ds, float* y0, float* y1, int B, int C, int L, int R, int N, int64_t xbs0, int64_t xbs1, hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)(R + 2 * N) * 64 * SN_E;
    ss2d_scan_n_kernel<NM, SN_E, SN_CB><<<cdiv(C, SN_CB) * B * 2, SN_CB * 64, lds, s>>>(x0, x1, xd0, xd1, dtw, dtb, A, Ds, y0, y1, B, C, L, R, N,
                                                                                      xbs0, xbs1);
    return bem_check_launch("ss2d_scan_n");
}

template <int NM>
static int launch_bwd(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dy0, const float* dy1, const float* dtw,
                      const float* dtb, const float* A, const float* Ds, float* dx0, float* dx1, float* dxd0, float* dxd1, float* dAlog, float* dDs,
                      float* ddtw, float* ddtb, float* ws, int B, int C, int L, int R, int N, int64_t xbs0, int64_t xbs1, hipStream_t s) {
    constexpr size_t lds_max = sizeof(float) * (2 * (size_t)(SN_RMAX + 2 * NM) * 64 * SN_E + SN_CB * SN_RMAX);
    static_assert(lds_max <= 160 * 1024, "LDS budget");
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ss2d_scan_n_bwd_kernel<NM, SN_E, SN_CB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_max);
        attr_set = true;
    }
    const size_t lds = sizeof(float) * (2 * (size_t)(R + 2 * N) * 64 * SN_E + SN_CB * SN_RMAX);
    ss2d_scan_n_bwd_kernel<NM, SN_E, SN_CB><<<cdiv(C, SN_CB) * B * 2, SN_CB * 64, lds, s>>>(x0, x1, xd0, xd1, dy0, dy1, dtw, dtb, A, Ds, dx0, dx1,
                                                                                          dxd0, dxd1, dAlog, dDs, ddtw, ddtb, ws, B, C, L, R, N,
                                                                                          xbs0, xbs1);
    return bem_check_launch("ss2d_scan_n_bwd");
}

}  // namespace

extern "C" int bem_ss2d_scan_n_supported(int N) { return N >= 1 && N <= SN_NMAX; }

extern "C" int bem_ss2d_scan_n_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dtw, const float* dtb,
                                   const float* A, const float* Ds, float* y0, float* y1, int B, int C, int L, int R, int N,
                                   int64_t xd0_bstride, int64_t xd1_bstride, void* stream) {
    BEM_REQUIRE(x0 && x1 && xd0 && xd1 && dtw && dtb && A && Ds && y0 && y1, "ss2d_scan_n: null tensor");
    BEM_REQUIRE(N >= 1 && N <= SN_NMAX, "ss2d_scan_n: d_state N=%d outside 1..%d", N, SN_NMAX);
    BEM_REQUIRE(B >= 0 && C > 0 && L >= 0 && R >= 1 && R <= SN_RMAX && (int64_t)cdiv(C, SN_CB) * B * 2 < (1ll << 31),
                "ss2d_scan_n: bad shape B=%d C=%d L=%d R=%d (dt_rank <= %d)", B, C, L, R, SN_RMAX);
    const int64_t rows2 = (int64_t)2 * (R + 2 * N) * L;
    const int64_t xbs0 = xd0_bstride ? xd0_bstride : rows2, xbs1 = xd1_bstride ? xd1_bstride : rows2;
    BEM_REQUIRE(xbs0 >= rows2 && xbs1 >= rows2 && (L % 4 != 0 || (xbs0 % 4 == 0 && xbs1 % 4 == 0)), "ss2d_scan_n: x_dbl batch strides");
    if (L % 4 == 0)
        BEM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)xd0 | (uintptr_t)xd1 | (uintptr_t)y0 | (uintptr_t)y1) & 15) == 0,
                    "ss2d_scan_n: 16-byte alignment");
    if (B == 0 || L == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (N <= 4) return launch_fwd<4>(x0, x1, xd0, xd1, dtw, dtb, A, Ds, y0, y1, B, C, L, R, N, xbs0, xbs1, s);
    if (N <= 8) return launch_fwd<8>(x0, x1, xd0, xd1, dtw, dtb, A, Ds, y0, y1, B, C, L, R, N, xbs0, xbs1, s);
    return launch_fwd<16>(x0, x1, xd0, xd1, dtw, dtb, A, Ds, y0, y1, B, C, L, R, N, xbs0, xbs1, s);
}

extern "C" int64_t bem_ss2d_scan_n_bwd_ws_elems(int B, int C, int L, int N) {
    if (B < 0 || C < 0 || L < 0 || N < 1 || N > SN_NMAX) return 0;
    return (int64_t)2 * B * C * cdiv64(L, 64 * SN_E) * N;
}

extern "C" int bem_ss2d_scan_n_bwd_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dy0, const float* dy1,
                                       const float* dtw, const float* dtb, const float* A, const float* Ds, float* dx0, float* dx1, float* dxd0,
                                       float* dxd1, float* dAlog, float* dDs, float* ddtw, float* ddtb, float* ws, int64_t ws_elems, int B, int C,
                                       int L, int R, int N, int64_t xd0_bstride, int64_t xd1_bstride, void* stream) {
    BEM_REQUIRE(x0 && x1 && xd0 && xd1 && dy0 && dy1 && dtw && dtb && A && Ds && dx0 && dx1 && dxd0 && dxd1 && dAlog && dDs && ddtw && ddtb && ws,
                "ss2d_scan_n_bwd: null tensor");
    BEM_REQUIRE(N >= 1 && N <= SN_NMAX, "ss2d_scan_n_bwd: d_state N=%d outside 1..%d", N, SN_NMAX);
    BEM_REQUIRE(B >= 0 && C > 0 && L >= 0 && R >= 1 && R <= SN_RMAX && (int64_t)cdiv(C, SN_CB) * B * 2 < (1ll << 31),
                "ss2d_scan_n_bwd: bad shape B=%d C=%d L=%d R=%d (dt_rank <= %d)", B, C, L, R, SN_RMAX);
    const int64_t rows2 = (int64_t)2 * (R + 2 * N) * L;
    const int64_t xbs0 = xd0_bstride ? xd0_bstride : rows2, xbs1 = xd1_bstride ? xd1_bstride : rows2;
    BEM_REQUIRE(xbs0 >= rows2 && xbs1 >= rows2 && (L % 4 != 0 || (xbs0 % 4 == 0 && xbs1 % 4 == 0)), "ss2d_scan_n_bwd: x_dbl batch strides");
    BEM_REQUIRE(ws_elems >= bem_ss2d_scan_n_bwd_ws_elems(B, C, L, N), "ss2d_scan_n_bwd: workspace of %lld floats, %lld needed", (long long)ws_elems,
                (long long)bem_ss2d_scan_n_bwd_ws_elems(B, C, L, N));
    if (L % 4 == 0)
        BEM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)xd0 | (uintptr_t)xd1 | (uintptr_t)dy0 | (uintptr_t)dy1 | (uintptr_t)dx0 | (uintptr_t)dx1) & 15) == 0,
                    "ss2d_scan_n_bwd: 16-byte alignment");
    if (B == 0 || L == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t nd = sizeof(float) * (size_t)B * rows2;
    if (hipMemsetAsync(dxd0, 0, nd, s) != hipSuccess || hipMemsetAsync(dxd1, 0, nd, s) != hipSuccess) return bem_check_launch("ss2d_scan_n_bwd memset");
#define BEM_SN_BWD(NM) return launch_bwd<NM>(x0, x1, xd0, xd1, dy0, dy1, dtw, dtb, A, Ds, dx0, dx1, dxd0, dxd1, dAlog, dDs, ddtw, ddtb, ws, B, C, L, R, N, xbs0, xbs1, s)
    if (N <= 4) BEM_SN_BWD(4);
    if (N <= 8) BEM_SN_BWD(8);
    BEM_SN_BWD(16);
#undef BEM_SN_BWD
}
