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
        load4<E>(tile + r * T + lane * E, v);
        const float w = wdt[r];
#pragma unroll
        for (int e = 0; e < E; ++e) z[e] = fmaf(w, v[e], z[e]);
    }
}

// coefficients of state n from dl = softplus(dt) and dlx = dl x (shared by the states): a = exp(dl A_n), b = dlx B_n, identity past L
template <int E>
__device__ __forceinline__ void state_coeffs(const float (&dl)[E], const float (&dlx)[E], const float (&Bv)[E], float An, int64_t te, int L,
                                             float (&a)[E], float (&b)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool ok = te + e < L;
        a[e] = ok ? bem_fexp(dl[e] * An) : 1.f;
        b[e] = ok ? dlx[e] * Bv[e] : 0.f;
    }
}

template <int NM, int E, int CB, bool REV>
__device__ __forceinline__ void scan_n_dir(float* tile, const float* __restrict__ xr, const float* __restrict__ xd, float* __restrict__ yr,
                                           const Ss2dDir p, bool live, int L, int R, int N) {
    constexpr int T = 64 * E, NT = CB * 64;
    const float* wdt = p.wdt;
    const float* Ak = p.A;
    const float dtb = p.dtb, Dk = p.D;
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
            load4<E>(tile + (R + n) * T + lane * E, Bv);
            load4<E>(tile + (R + N + n) * T + lane * E, Cv);
            state_coeffs<E>(dl, dlx, Bv, A[n], te, L, a, bb);
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
    const Ss2dItem it = ss2d_item(blockIdx.x, (C + CB - 1) / CB, Bn);
    const int b = it.b, o = it.o;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = it.u * CB + wave;
    const bool live = c < C;
    const int cc = live ? c : C - 1;                         // parameter reads of an idle slot stay in bounds
    const int64_t row = ((int64_t)b * C + cc) * L;
    const float* xr = (o ? x1 : x0) + row;
    float* yr = (o ? y1 : y0) + row;
    const float* xd = o ? xd1 + (int64_t)b * xbs1 : xd0 + (int64_t)b * xbs0;
    scan_n_dir<NM, E, CB, false>(tile, xr, xd, yr, ss2d_dir(dtw, dtb, A, Ds, o, C, cc, R, N), live, L, R, N);
    scan_n_dir<NM, E, CB, true>(tile, xr, xd + (int64_t)(R + 2 * N) * L, yr, ss2d_dir(dtw, dtb, A, Ds, o + 2, C, cc, R, N), live, L, R, N);
}

// ------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------
template <int NM, int E, int CB, bool REV>
__device__ __forceinline__ void scan_n_dir_bwd(float* tile, float* acc, float* accw, const float* __restrict__ xr, const float* __restrict__ dyr,
                                               const float* __restrict__ xd, float* __restrict__ dxd, float* __restrict__ dxr, float* __restrict__ cws,
                                               const Ss2dDir p, bool live, bool first, int L, int R, int N, float* __restrict__ dAlog,
                                               float* __restrict__ dDs, float* __restrict__ ddtb, float* __restrict__ ddtw) {
    constexpr int T = 64 * E, NT = CB * 64;
    const float* wdt = p.wdt;
    const float* Ak = p.A;
    const float dtb = p.dtb, Dk = p.D;
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
            load4<E>(tile + (R + n) * T + lane * E, Bv);
            state_coeffs<E>(dl, dlx, Bv, A[n], te, L, a, bb);
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
                load4<E>(tile + (R + n) * T + lane * E, Bv);
                load4<E>(tile + (R + N + n) * T + lane * E, Cv);
                state_coeffs<E>(dl, dlx, Bv, A[n], te, L, a, bb);
#pragma unroll
                for (int e = 0; e < E; ++e) {
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
                load4<E>(tile + r * T + lane * E, v);
                const float w = wdt[r];
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    s = fmaf(dz[e], v[e], s);
                    atomicAdd(acc + r * T + lane * E + e, dz[e] * w);
                }
                s = wave_sum(s);
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
        accD = wave_sum(accD);
        accB = wave_sum(accB);
#pragma unroll
        for (int n = 0; n < NM; ++n) {
            if (n >= N) continue;
            const float s = wave_sum(dA[n]);
            if (lane == 0) atomicAdd(dAlog + (int64_t)p.kc * N + n, s * A[n]);   // A = -exp(A_logs): dA_logs = dA * A
        }
        if (lane == 0) {
            atomicAdd(dDs + p.kc, accD);
            atomicAdd(ddtb + p.kc, accB);
        }
        if (lane < R) atomicAdd(ddtw + (int64_t)p.kc * R + lane, accw[wave * SN_RMAX + lane]);
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
    const Ss2dItem it = ss2d_item(blockIdx.x, (C + CB - 1) / CB, Bn);
    const int b = it.b, o = it.o;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = it.u * CB + wave;
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
    scan_n_dir_bwd<NM, E, CB, false>(tile, acc, accw, xr, dyr, xd, dxd, dxr, cws, ss2d_dir(dtw, dtb, A, Ds, o, C, cc, R, N), live, true, L, R, N,
                                     dAlog, dDs, ddtb, ddtw);
    scan_n_dir_bwd<NM, E, CB, true>(tile, acc, accw, xr, dyr, xd + (int64_t)rows * L, dxd + (int64_t)rows * L, dxr, cws,
                                    ss2d_dir(dtw, dtb, A, Ds, o + 2, C, cc, R, N), live, false, L, R, N, dAlog, dDs, ddtb, ddtw);
}

constexpr int SN_E = 4;          // positions per lane: 256-position tiles, float4 rows
constexpr int SN_CB = 8;         // channels (wavefronts) per workgroup: divides the n_feat-40 widths 40 / 80 / 160

template <int NM>
static int launch_fwd(const Ss2dArgs& a) {
    const size_t lds = sizeof(float) * (size_t)(a.R + 2 * a.N) * 64 * SN_E;
    ss2d_scan_n_kernel<NM, SN_E, SN_CB><<<cdiv(a.C, SN_CB) * a.B * 2, SN_CB * 64, lds, a.s>>>(SS2D_FWD_OPERANDS(a), a.B, a.C, a.L, a.R, a.N, a.xbs0, a.xbs1);
    return bem_check_launch("ss2d_scan_n");
}

template <int NM>
static int launch_bwd(const Ss2dArgs& a) {
    constexpr size_t lds_max = sizeof(float) * (2 * (size_t)(SN_RMAX + 2 * NM) * 64 * SN_E + SN_CB * SN_RMAX);
    static_assert(lds_max <= 160 * 1024, "LDS budget");
    set_max_dynamic_lds<&ss2d_scan_n_bwd_kernel<NM, SN_E, SN_CB>>((int)lds_max);
    const size_t lds = sizeof(float) * (2 * (size_t)(a.R + 2 * a.N) * 64 * SN_E + SN_CB * SN_RMAX);
    ss2d_scan_n_bwd_kernel<NM, SN_E, SN_CB><<<cdiv(a.C, SN_CB) * a.B * 2, SN_CB * 64, lds, a.s>>>(SS2D_BWD_OPERANDS(a), a.ws, a.B, a.C, a.L, a.R, a.N,
                                                                                                a.xbs0, a.xbs1);
    return bem_check_launch("ss2d_scan_n_bwd");
}

}  // namespace

extern "C" int bem_ss2d_scan_n_supported(int N) { return N >= 1 && N <= SN_NMAX; }

extern "C" int bem_ss2d_scan_n_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dtw, const float* dtb,
                                   const float* A, const float* Ds, float* y0, float* y1, int B, int C, int L, int R, int N,
                                   int64_t xd0_bstride, int64_t xd1_bstride, void* stream) {
    BEM_REQUIRE(N >= 1 && N <= SN_NMAX, "ss2d_scan_n: d_state N=%d outside 1..%d", N, SN_NMAX);
    Ss2dArgs a{};
    a.x0 = x0; a.x1 = x1; a.xd0 = xd0; a.xd1 = xd1; a.dtw = dtw; a.dtb = dtb; a.A = A; a.Ds = Ds;
    a.y0 = y0; a.y1 = y1;
    a.B = B; a.C = C; a.L = L; a.R = R; a.N = N; a.s = (hipStream_t)stream;
    if (const int rc = ss2d_operands_ok("ss2d_scan_n", a, false, true, SN_RMAX, cdiv(C, SN_CB), R + 2 * N, xd0_bstride, xd1_bstride)) return rc;
    if (B == 0 || L == 0) return BEM_OK;
    return N <= 4 ? launch_fwd<4>(a) : N <= 8 ? launch_fwd<8>(a) : launch_fwd<16>(a);
}

extern "C" int64_t bem_ss2d_scan_n_bwd_ws_elems(int B, int C, int L, int N) {
    if (B < 0 || C < 0 || L < 0 || N < 1 || N > SN_NMAX) return 0;
    return (int64_t)2 * B * C * cdiv64(L, 64 * SN_E) * N;
}

extern "C" int bem_ss2d_scan_n_bwd_f32(const float* x0, const float* x1, const float* xd0, const float* xd1, const float* dy0, const float* dy1,
                                       const float* dtw, const float* dtb, const float* A, const float* Ds, float* dx0, float* dx1, float* dxd0,
                                       float* dxd1, float* dAlog, float* dDs, float* ddtw, float* ddtb, float* ws, int64_t ws_elems, int B, int C,
                                       int L, int R, int N, int64_t xd0_bstride, int64_t xd1_bstride, void* stream) {
    BEM_REQUIRE(N >= 1 && N <= SN_NMAX, "ss2d_scan_n_bwd: d_state N=%d outside 1..%d", N, SN_NMAX);
    Ss2dArgs a{};
    a.x0 = x0; a.x1 = x1; a.xd0 = xd0; a.xd1 = xd1; a.dtw = dtw; a.dtb = dtb; a.A = A; a.Ds = Ds;
    a.dy0 = dy0; a.dy1 = dy1; a.dx0 = dx0; a.dx1 = dx1; a.dxd0 = dxd0; a.dxd1 = dxd1; a.dAlog = dAlog; a.dDs = dDs; a.ddtw = ddtw; a.ddtb = ddtb; a.ws = ws;
    a.B = B; a.C = C; a.L = L; a.R = R; a.N = N; a.s = (hipStream_t)stream;
    BEM_REQUIRE(ws, "ss2d_scan_n_bwd: null tensor");
    if (const int rc = ss2d_operands_ok("ss2d_scan_n_bwd", a, true, true, SN_RMAX, cdiv(C, SN_CB), R + 2 * N, xd0_bstride, xd1_bstride)) return rc;
    BEM_REQUIRE(ws_elems >= bem_ss2d_scan_n_bwd_ws_elems(B, C, L, N), "ss2d_scan_n_bwd: workspace of %lld floats, %lld needed", (long long)ws_elems,
                (long long)bem_ss2d_scan_n_bwd_ws_elems(B, C, L, N));
    if (B == 0 || L == 0) return BEM_OK;
    const size_t nd = sizeof(float) * (size_t)B * 2 * (R + 2 * N) * L;
    BEM_ZERO(dxd0, nd, a.s, "ss2d_scan_n_bwd");
    BEM_ZERO(dxd1, nd, a.s, "ss2d_scan_n_bwd");
    return N <= 4 ? launch_bwd<4>(a) : N <= 8 ? launch_bwd<8>(a) : launch_bwd<16>(a);
}
