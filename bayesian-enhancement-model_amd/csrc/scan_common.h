// Shared by the selective-scan kernels (scan.hip, scan_bwd.hip, scan_nstate.hip): block- and wavefront-wide affine-map scan
// primitives, row loads / stores, the fused-SS2D work-item decode, per-direction parameters and scan coefficients, and the host-side
// operand check of the bem_ss2d_scan*_f32 entry points.
#pragma once
#include "bem_common.h"
#include <climits>

namespace {

template <bool REV>
__device__ __forceinline__ float shfl_prev(float v, int d) {
    return REV ? __shfl_down(v, d, BEM_WAVE) : __shfl_up(v, d, BEM_WAVE);
}

// Block-wide composition of per-thread affine maps.  On entry (a[e], b[e]) are the per-position
// coefficients h_t = a_t * h_prev + b_t of this thread's E positions (identity = (1, 0) for padding).
// On exit h[e] holds the state after position e; `carry` (state entering the chunk, uniform) is updated
// to the state leaving the chunk.  agg is LDS scratch of 2*NW floats; contains two barriers.
// block_scan_enter returns the state entering this thread's first position (in scan order) and advances `carry`.
template <int NT, int E, bool REV>
__device__ __forceinline__ float block_scan_enter(const float (&a)[E], const float (&b)[E], float& carry, float* agg) {
    constexpr int NW = NT / BEM_WAVE;
    const int lane = threadIdx.x & (BEM_WAVE - 1);
    const int wave = threadIdx.x / BEM_WAVE;
    const int rl = REV ? (BEM_WAVE - 1 - lane) : lane;   // logical lane in scan order
    float P = 1.f, S = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = REV ? (E - 1 - i) : i;
        S = a[e] * S + b[e];
        P = P * a[e];
    }
    // inclusive wave scan of (P, S): compose(prev, cur) = (Pp*Pc, Pc*Sp + Sc)
#pragma unroll
    for (int d = 1; d < BEM_WAVE; d <<= 1) {
        const float Pp = shfl_prev<REV>(P, d);
        const float Sp = shfl_prev<REV>(S, d);
        if (rl >= d) {
            S = P * Sp + S;
            P = P * Pp;
        }
    }
    float Pe = shfl_prev<REV>(P, 1);
    float Se = shfl_prev<REV>(S, 1);
    if (rl == 0) { Pe = 1.f; Se = 0.f; }
    if (NW > 1) {
        if (rl == BEM_WAVE - 1) { agg[2 * wave] = P; agg[2 * wave + 1] = S; }
        __syncthreads();
    }
    float hw = carry;      // state entering this wave
    float hend = carry;    // state leaving the chunk
    if (NW > 1) {
        const int rw = REV ? (NW - 1 - wave) : wave;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int w = REV ? (NW - 1 - i) : i;
            const float Pw = agg[2 * w], Sw = agg[2 * w + 1];
            hend = Pw * hend + Sw;
            if (i < rw) hw = Pw * hw + Sw;
        }
        __syncthreads();   // agg may be rewritten by the next call
    } else {
        // single wave: total = inclusive value of the last logical lane
        const float Pt = __shfl(P, REV ? 0 : BEM_WAVE - 1, BEM_WAVE);
        const float St = __shfl(S, REV ? 0 : BEM_WAVE - 1, BEM_WAVE);
        hend = Pt * carry + St;
    }
    carry = hend;
    return Pe * hw + Se;       // state entering this thread
}

template <int NT, int E, bool REV>
__device__ __forceinline__ void block_scan_affine(const float (&a)[E], const float (&b)[E], float (&h)[E],
                                                  float& carry, float* agg) {
    float hh = block_scan_enter<NT, E, REV>(a, b, carry, agg);
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = REV ? (E - 1 - i) : i;
        hh = a[e] * hh + b[e];
        h[e] = hh;
    }
}

template <int E>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int64_t t0, int L, bool vec, float (&v)[E]) {
    if (vec && t0 + E <= L) {
#pragma unroll
        for (int i = 0; i < E; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(p + t0 + i);
            v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (t0 + i < L) ? p[t0 + i] : 0.f;
    }
}
// 16-bit inputs of the operator seam (selective_scan_oflex.cpp:166-216 takes f16 / bf16 u, delta, B, C): the same row access, 2 bytes per
// element, converted in registers -- no f32 copy of the tensor is made.
struct bem_half_t { uint16_t b; };
struct bem_bf16_t { uint16_t b; };
__device__ __forceinline__ float bem_to_f32(bem_half_t h) { return (float)__builtin_bit_cast(_Float16, h.b); }
__device__ __forceinline__ float bem_to_f32(bem_bf16_t h) { return __builtin_bit_cast(float, (uint32_t)h.b << 16); }
template <int E, typename T16>
__device__ __forceinline__ void load_row(const T16* __restrict__ p, int64_t t0, int L, bool vec, float (&v)[E]) {
    if (vec && t0 + E <= L) {                       // vec: L % 4 == 0 and the tensor 8-byte aligned -> 8-byte pieces of 4 elements
#pragma unroll
        for (int i = 0; i < E; i += 4) {
            const uint2 q = *reinterpret_cast<const uint2*>(p + t0 + i);
            v[i] = bem_to_f32(T16{(uint16_t)(q.x & 0xffffu)}); v[i + 1] = bem_to_f32(T16{(uint16_t)(q.x >> 16)});
            v[i + 2] = bem_to_f32(T16{(uint16_t)(q.y & 0xffffu)}); v[i + 3] = bem_to_f32(T16{(uint16_t)(q.y >> 16)});
        }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (t0 + i < L) ? bem_to_f32(p[t0 + i]) : 0.f;
    }
}
template <int E>
__device__ __forceinline__ void store_row(float* __restrict__ p, int64_t t0, int L, bool vec, const float (&v)[E]) {
    if (vec && t0 + E <= L) {
#pragma unroll
        for (int i = 0; i < E; i += 4)
            *reinterpret_cast<float4*>(p + t0 + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (t0 + i < L) p[t0 + i] = v[i];
    }
}

// unmasked float4 forms of load_row / store_row (whole tiles, 16-byte aligned rows; also rows of an LDS tile)
template <int E>
__device__ __forceinline__ void load4(const float* p, float (&v)[E]) {
#pragma unroll
    for (int i = 0; i < E; i += 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
    }
}
template <int E>
__device__ __forceinline__ void store4(float* p, const float (&v)[E]) {
#pragma unroll
    for (int i = 0; i < E; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
}

// ------------------------------------------------------------------------------------------------
// Fused SS2D scans: a launch covers 2 orientations x Bn images x n units (channels, or groups of CB channels), unit fastest.
// ------------------------------------------------------------------------------------------------
struct Ss2dItem { int u, b, o; };       // unit (channel c or channel group g), image, orientation
__device__ __forceinline__ Ss2dItem ss2d_item(int wi, int n, int Bn) { return {wi % n, (wi / n) % Bn, wi / (n * Bn)}; }

// Parameters of direction k (0 / 1: orientations 0 / 1 in memory order, 2 / 3: the same reversed) and channel c, from dtw (4, C, R),
// dtb and Ds (4, C) and A (4, C, N); kc = k * C + c also indexes the channel's parameter gradients.
struct Ss2dDir { const float* wdt; float dtb; const float* A; float D; int kc; };
__device__ __forceinline__ Ss2dDir ss2d_dir(const float* __restrict__ dtw, const float* __restrict__ dtb, const float* __restrict__ A,
                                            const float* __restrict__ Ds, int k, int C, int c, int R, int N = 1) {
    const int kc = k * C + c;
    return {dtw + (int64_t)kc * R, dtb[kc], A + (int64_t)kc * N, Ds[kc], kc};
}

// softplus and exp(dt A) on one base-2 logarithm: lg = log2(1 + e^z) (z log2 e beyond softplus' threshold of 20), then
// dt = lg ln 2, exp(dt A) = 2^(A lg) and sigmoid(z) = 1 - 2^-lg
constexpr float BEM_LOG2E = 1.44269504088896340736f, BEM_LN2 = 0.69314718055994530942f;
__device__ __forceinline__ float softplus_log2(float z) {
    return z <= 20.f ? __builtin_amdgcn_logf(1.f + __builtin_amdgcn_exp2f(z * BEM_LOG2E)) : z * BEM_LOG2E;
}

// Scan coefficients of E positions of one direction (d_state 1): z = dtb + sum_r w_r dt_row_r, dl = softplus(z), a = exp(dl A),
// b = dl B x; positions past L get the identity (a, b) = (1, 0).  Bv / Cv are the B and C rows.  The backward uses every output, the
// forward the short form below (outputs that are not used cost nothing).
template <int E>
__device__ __forceinline__ void ss2d_coeffs(const float* __restrict__ xd /* (R+2, L) of one direction */, const float* __restrict__ wdt /* (R) */,
                                            float dtb, float Ak, const float (&x)[E], int64_t t0, int L, int R, bool vec, float (&a)[E],
                                            float (&b)[E], float (&Bv)[E], float (&Cv)[E], float (&dl)[E], float (&z)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) z[e] = 0.f;
    for (int r = 0; r < R; ++r) {
        float v[E];
        load_row<E>(xd + (int64_t)r * L, t0, L, vec, v);
        const float w = wdt[r];
#pragma unroll
        for (int e = 0; e < E; ++e) z[e] = fmaf(w, v[e], z[e]);
    }
    load_row<E>(xd + (int64_t)R * L, t0, L, vec, Bv);
    load_row<E>(xd + (int64_t)(R + 1) * L, t0, L, vec, Cv);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool ok = t0 + e < L;
        z[e] += dtb;
        dl[e] = bem_softplus(z[e]);
        a[e] = ok ? bem_fexp(dl[e] * Ak) : 1.f;
        b[e] = ok ? dl[e] * Bv[e] * x[e] : 0.f;
    }
}
template <int E>
__device__ __forceinline__ void ss2d_coeffs(const float* __restrict__ xd, const float* __restrict__ wdt, float dtb, float Ak, const float (&x)[E],
                                            int64_t t0, int L, int R, bool vec, float (&a)[E], float (&b)[E], float (&Cv)[E]) {
    float Bv[E], dl[E], z[E];
    ss2d_coeffs<E>(xd, wdt, dtb, Ak, x, t0, L, R, vec, a, b, Bv, Cv, dl, z);
}

template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_mov(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                                 CTRL, ROWMASK, 0xf, false));
}
__device__ __forceinline__ float lane_bcast(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// One step of the lane scan of affine maps h -> P h + S: (P, S) <- (P, S) o (P, S)[source lane], i.e. S = P S' + S, P = P P'.
// Both halves are ONE DPP instruction each: the DPP operand is the instruction's own src0, and a lane without a source lane (row
// boundary, masked row) is simply not written -- the identity of the composition.  The builtin form (update_dpp with old = 1 / 0,
// then fma / mul) costs six instructions per step (v_mov old, v_mov_dpp, twice, + fma + mul), a third of the whole scan kernel.
// s_nop 1: a DPP read of a VGPR needs two wait states after the VALU write of that VGPR (gfx9 hazard; the compiler cannot see into
// the asm, and S / P are written by the instruction right before the block).
#define BEM_SCAN_STEP(DPP)                                                                                   \
    asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %1 " DPP "\n\tv_mul_f32_dpp %1, %1, %1 " DPP : "+v"(S), "+v"(P))
// inclusive scan of the per-lane affine maps (P, S) in ascending (REV = false) / descending (REV = true) lane order;
// returns the exclusive map (Pe, Se) of every lane and leaves the wavefront total in lane 63 (0 for REV).
template <bool REV>
__device__ __forceinline__ void wave_scan_affine(float& P, float& S, float& Pe, float& Se) {
    if (!REV) {
        BEM_SCAN_STEP("row_shr:1 row_mask:0xf bank_mask:0xf"); BEM_SCAN_STEP("row_shr:2 row_mask:0xf bank_mask:0xf");
        BEM_SCAN_STEP("row_shr:4 row_mask:0xf bank_mask:0xf"); BEM_SCAN_STEP("row_shr:8 row_mask:0xf bank_mask:0xf");
        BEM_SCAN_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf"); BEM_SCAN_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf");
        asm volatile("s_nop 1");              // the compiler's own DPP moves below read P / S right behind the asm writes
        Pe = dpp_mov<0x138, 0xf>(1.f, P);   // wave_shr 1
        Se = dpp_mov<0x138, 0xf>(0.f, S);
    } else {
        BEM_SCAN_STEP("row_shl:1 row_mask:0xf bank_mask:0xf"); BEM_SCAN_STEP("row_shl:2 row_mask:0xf bank_mask:0xf");
        BEM_SCAN_STEP("row_shl:4 row_mask:0xf bank_mask:0xf"); BEM_SCAN_STEP("row_shl:8 row_mask:0xf bank_mask:0xf");
        const int lane = threadIdx.x & 63;
        {   // rows 0 / 2 append the suffix of rows 1 / 3 (their lane 16 / 48)
            const float P16 = lane_bcast(P, 16), S16 = lane_bcast(S, 16), P48 = lane_bcast(P, 48), S48 = lane_bcast(S, 48);
            const bool take = (lane & 16) == 0;
            const float Pp = take ? ((lane & 32) ? P48 : P16) : 1.f, Sp = take ? ((lane & 32) ? S48 : S16) : 0.f;
            S = fmaf(P, Sp, S);
            P = P * Pp;
        }
        {   // rows 0, 1 append the suffix of rows 2, 3 (lane 32)
            const float P32 = lane_bcast(P, 32), S32 = lane_bcast(S, 32);
            const bool take = lane < 32;
            const float Pp = take ? P32 : 1.f, Sp = take ? S32 : 0.f;
            S = fmaf(P, Sp, S);
            P = P * Pp;
        }
        Pe = dpp_mov<0x130, 0xf>(1.f, P);   // wave_shl 1
        Se = dpp_mov<0x130, 0xf>(0.f, S);
    }
}
#undef BEM_SCAN_STEP

// Cross-wave step of a block scan whose wavefront part ran on wave_scan_affine<REV>: (P, S) is the inclusive map of the lane,
// i.e. the wavefront total sits in lane 63 (lane 0 for REV).  The NW totals go through the LDS slot `ag` (2 NW floats, ONE
// barrier; the caller rotates slots so that a slot is rewritten only after later barriers) and are composed in scan order on
// one 16-lane DPP row.  Returns the state entering this wavefront and advances `carry` (state entering the block) to the state
// leaving it.
template <int NW, bool REV>
__device__ __forceinline__ float cross_wave_affine(float P, float S, float* ag, float& carry) {
    static_assert(NW <= 16, "the cross-wave scan uses one DPP row");
    const int lane = threadIdx.x & (BEM_WAVE - 1), wave = threadIdx.x / BEM_WAVE;
    if (NW == 1) {
        const float Pt = lane_bcast(P, REV ? 0 : BEM_WAVE - 1), St = lane_bcast(S, REV ? 0 : BEM_WAVE - 1);
        const float hw = carry;
        carry = fmaf(Pt, hw, St);
        return hw;
    }
    if (lane == (REV ? 0 : BEM_WAVE - 1)) { ag[2 * wave] = P; ag[2 * wave + 1] = S; }
    __syncthreads();
    const int sl = min(lane, NW - 1), src = REV ? NW - 1 - sl : sl;
    const float Pl = ag[2 * src], Sl = ag[2 * src + 1];
    float Pw = lane < NW ? Pl : 1.f, Sw = lane < NW ? Sl : 0.f;
#define BEM_ROW_STEP(DPP) asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %1 " DPP "\n\tv_mul_f32_dpp %1, %1, %1 " DPP : "+v"(Sw), "+v"(Pw))
    BEM_ROW_STEP("row_shr:1 row_mask:0xf bank_mask:0xf"); BEM_ROW_STEP("row_shr:2 row_mask:0xf bank_mask:0xf");
    if (NW > 4) BEM_ROW_STEP("row_shr:4 row_mask:0xf bank_mask:0xf");
    if (NW > 8) BEM_ROW_STEP("row_shr:8 row_mask:0xf bank_mask:0xf");
#undef BEM_ROW_STEP
    const int rw = REV ? NW - 1 - wave : wave;
    const float Pt = lane_bcast(Pw, NW - 1), St = lane_bcast(Sw, NW - 1);
    const float Px = lane_bcast(Pw, rw > 0 ? rw - 1 : 0), Sx = lane_bcast(Sw, rw > 0 ? rw - 1 : 0);
    const float c0 = carry;
    carry = fmaf(Pt, c0, St);
    return rw > 0 ? fmaf(Px, c0, Sx) : c0;
}

// ------------------------------------------------------------------------------------------------
// host side of the bem_ss2d_scan*_f32 entry points
// ------------------------------------------------------------------------------------------------
// Operands of one fused SS2D launch, forward (y0 / y1) or backward (dy / dx / the gradients); the launch helpers take this.
struct Ss2dArgs {
    const float *x0, *x1, *xd0, *xd1, *dtw, *dtb, *A, *Ds;
    float *y0, *y1;
    const float *dy0, *dy1;
    float *dx0, *dx1, *dxd0, *dxd1, *dAlog, *dDs, *ddtw, *ddtb, *ws;
    hipStream_t s;
    int B, C, L, R, N;
    int64_t xbs0, xbs1;          // x_dbl batch strides, resolved by ss2d_operands_ok (never 0)
};
#define SS2D_FWD_OPERANDS(a) a.x0, a.x1, a.xd0, a.xd1, a.dtw, a.dtb, a.A, a.Ds, a.y0, a.y1
#define SS2D_BWD_OPERANDS(a) a.x0, a.x1, a.xd0, a.xd1, a.dy0, a.dy1, a.dtw, a.dtb, a.A, a.Ds, a.dx0, a.dx1, a.dxd0, a.dxd1, a.dAlog, a.dDs, a.ddtw, a.ddtb

// The checks every entry point makes before it touches the GPU: no null operand (forward: y; backward: dy, dx and the gradients),
// B / C / L / R in range (`units` workgroup units per (orientation, image) must fit a 31-bit grid), the x_dbl batch strides (0 = contiguous:
// 2 * rows_per_dir * L) at least that and, for L % 4 == 0 (float4 rows), multiples of 4, and -- unless the entry point serves unaligned
// tensors with another kernel -- the (B, C, L) and x_dbl tensors on 16 bytes in that case.  Resolves the strides into `a`.
static inline int ss2d_operands_ok(const char* who, Ss2dArgs& a, bool bwd, bool need_align, int rmax, int64_t units, int rows_per_dir,
                                   int64_t xd0_bstride, int64_t xd1_bstride) {
    BEM_REQUIRE(a.x0 && a.x1 && a.xd0 && a.xd1 && a.dtw && a.dtb && a.A && a.Ds, "%s: null tensor", who);
    if (bwd) BEM_REQUIRE(a.dy0 && a.dy1 && a.dx0 && a.dx1 && a.dxd0 && a.dxd1 && a.dAlog && a.dDs && a.ddtw && a.ddtb, "%s: null tensor", who);
    else BEM_REQUIRE(a.y0 && a.y1, "%s: null tensor", who);
    BEM_REQUIRE(a.B >= 0 && a.C > 0 && a.L >= 0 && a.R >= 1 && units * a.B * 2 < (1ll << 31), "%s: bad shape B=%d C=%d L=%d R=%d", who, a.B, a.C,
                a.L, a.R);
    BEM_REQUIRE(a.R <= rmax, "%s: dt_rank R=%d above %d", who, a.R, rmax);
    const int64_t dense = (int64_t)2 * rows_per_dir * a.L;
    a.xbs0 = xd0_bstride ? xd0_bstride : dense;
    a.xbs1 = xd1_bstride ? xd1_bstride : dense;
    const bool vec = a.L % 4 == 0;
    BEM_REQUIRE(a.xbs0 >= dense && a.xbs1 >= dense && (!vec || (a.xbs0 % 4 == 0 && a.xbs1 % 4 == 0)), "%s: x_dbl batch strides", who);
    const uintptr_t bits = (uintptr_t)a.x0 | (uintptr_t)a.x1 | (uintptr_t)a.xd0 | (uintptr_t)a.xd1 |
                           (bwd ? (uintptr_t)a.dy0 | (uintptr_t)a.dy1 | (uintptr_t)a.dx0 | (uintptr_t)a.dx1 : (uintptr_t)a.y0 | (uintptr_t)a.y1);
    BEM_REQUIRE(!(need_align && vec) || (bits & 15) == 0, "%s: 16-byte alignment", who);
    return BEM_OK;
}

// Raises the dynamic-LDS limit of KERNEL, once per process.
template <auto KERNEL>
static inline void set_max_dynamic_lds(int bytes) {
    static bool done = false;
    if (!done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        done = true;
    }
}

}  // namespace
