// Every matrix-core operand packer of the library, and the Bayesian samplers that write operand order directly.  Two formats:
//   * f32 pairs (pack_pw_weight_kernel, bem_pack_pw_weight_f32): natural (nsets, M, K) weights -> (nsets, MT, ceil(K/2), 64 lanes) in the operand
//     order of v_mfma_f32_32x32x2_f32 -- what the implicit-GEMM convolutions of conv.hip (conv2d_mfma*) and the conv weight-gradient kernels consume.
//   * x6, three bf16 limbs (pack_x6_*, bem_pack_pw_weight_x6*): (nsets, MT, KB, 3, 64) 16-byte vectors, the weight operand of the x6 kernels
//     (pw_gemm_x6.hip, conv_x6.hip, gdmlp_x6.hip, ss2d_front_x6.hip, upfuse_x6.hip); the layout is described in the header of pw_gemm_x6.hip.
//     sample_pack_x6_kernel and ebank_sample_kernel draw Bayesian weights (Philox, bem_common.h) and store them in that format.
// The natural-order samplers of the same Philox stream (randn_kernel, bnn_sample_kernel) are here too: every Philox draw is in this file.
#include "bem_common.h"
#include "x6_common.h"

namespace {

__global__ void pack_pw_weight_kernel(const float* __restrict__ W, float* __restrict__ Wp, int M, int K, int MT, int KS) {
    // grid: (ceil(MT*KS*64 / 256), nsets)
    const int64_t per = (int64_t)MT * KS * 64;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    const int lane = (int)(i & 63);
    const int64_t t = i >> 6;
    const int st = (int)(t % KS), mt = (int)(t / KS);
    const int row = mt * 32 + (lane & 31), col = 2 * st + (lane >> 5);
    const int set = blockIdx.y;
    Wp[(int64_t)set * per + i] = (row < M && col < K) ? W[((int64_t)set * M + row) * K + col] : 0.f;
}

// natural (nsets, M, K) f32 -> (nsets, MT, KB, 3, 64) 16-byte vectors of bf16 limbs
__device__ __forceinline__ void pack_x6_item(int64_t i, const float* __restrict__ W, u32x4* __restrict__ Wp, int M, int K, int MT, int KB,
                                             int64_t ss, int64_t rs, int64_t cs) {      // element strides of W over (set, row, k): transposed / sliced views pack in place
    const int lane = (int)(i & 63);
    const int64_t blk = i >> 6;
    const int kb = (int)(blk % KB), mt = (int)((blk / KB) % MT);
    const int64_t set = blk / ((int64_t)KB * MT);
    const int row = mt * 32 + (lane & 31), k0 = kb * 16 + (lane >> 5) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (row < M && k0 + e < K) ? W[set * ss + row * rs + (k0 + e) * cs] : 0.f;
    u32x4 h, m, l;
    split8(v, h, m, l);
    u32x4* o = Wp + ((set * MT + mt) * KB + kb) * 3 * 64 + lane;
    o[0] = h; o[64] = m; o[128] = l;
}

__global__ void pack_x6_kernel(const float* __restrict__ W, u32x4* __restrict__ Wp, int M, int K, int MT, int KB, int64_t total,
                               int64_t ss, int64_t rs, int64_t cs) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    pack_x6_item(i, W, Wp, M, K, MT, KB, ss, rs, cs);
}

// Many (M, K) matrices packed by one launch: job = { source pointer, first float of the packed output in `arena` (multiple of 4), int32 M,
// int32 K, row stride, column stride (elements), work items = ceil(M/32) ceil(K/16) 64 }; blk = { job, first block of 256 work items }.
// A Stage-I training step re-packs the forward and the transposed operand of every Bayesian 1x1 layer (the weights are new draws each
// iteration): ~120 launches of a few KiB otherwise.
struct packjob { const float* src; int64_t out; int32_t M, K; int64_t rs, cs, items, pad0, pad1; };
static_assert(sizeof(packjob) == 8 * 8, "packjob is eight 64-bit words (bem.modules.BayesBank builds it as an int64 table)");

__global__ __launch_bounds__(256) void pack_x6_jobs_kernel(const packjob* __restrict__ jobs, const int32_t* __restrict__ blks, float* __restrict__ arena) {
    const packjob jb = jobs[blks[2 * blockIdx.x]];
    const int64_t i = (int64_t)blks[2 * blockIdx.x + 1] * 256 + threadIdx.x;
    if (i >= jb.items) return;
    pack_x6_item(i, jb.src, reinterpret_cast<u32x4*>(arena + jb.out), jb.M, jb.K, (jb.M + 31) / 32, (jb.K + 15) / 16, 0, jb.rs, jb.cs);
}

// Bayesian weight sets straight into operand order: w[set][row][k] = mu + log1p(exp(rho)) * eps, eps injected or drawn
// with the sampler's own Philox stream (element index i = set*M*K + row*K + k, as bem_bnn_sample_f32 numbers it), split
// and stored like pack_x6_kernel does -- the natural-order copy (one write + one read per weight and sample) is skipped.
// ALIGNED: every lane's first element opens a counter block (g0 & 3 == 0), so 8 elements span two blocks and the third is not in the
// instruction stream; otherwise up to three.  Either way a lane evaluates only the blocks its live elements read -- none for a lane
// of padding (row >= M or k0 >= K), one when four or fewer elements are live.
template <bool ALIGNED>
__device__ __forceinline__ void sample_pack_x6_draw(int64_t set, int mt, int kb, int lane, const float* __restrict__ mu, const float* __restrict__ rho,
                                                    const float* __restrict__ eps_in, u32x4* __restrict__ Wp, int M, int K, int MT, int KB,
                                                    uint64_t seed, uint64_t stream_id, int sigma_given) {
    const int row = mt * 32 + (lane & 31), k0 = kb * 16 + (lane >> 5) * 8;
    float v[8];
    // the lane's 8 consecutive k of one row are 8 consecutive element indices: at most 3 Philox counter blocks
    const int64_t g0 = set * M * K + (int64_t)row * K + k0;
    const int off = ALIGNED ? 0 : (int)(g0 & 3);                          // position of the first element in its block
    const int live = row < M ? min(8, K - k0) : 0;                        // <= 0: the lane holds padding only
    constexpr int NQ = ALIGNED ? 2 : 3;
    float z[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)                                          // block q is read by elements 4q - off .. 4q - off + 3
        if (!eps_in && live > 0 && q <= ((off + live - 1) >> 2)) philox_normal4((g0 >> 2) + q, seed, stream_id, z[q]);
    // mu and sigma of the lane's elements.  Aligned, they are one or two 16-byte vectors per tensor: as eight dword loads each, a wave's
    // load instruction touches 32 rows for 4 bytes apiece, and those cache-line lookups, not the arithmetic, were the kernel's time.
    const int64_t idx0 = (int64_t)row * K + k0;
    float mv[8], sv[8];
    if (ALIGNED && (((uintptr_t)mu | (uintptr_t)rho) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {                                     // live is 0, 4 or 8 here
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (4 * q < live) { a = *reinterpret_cast<const float4*>(mu + idx0 + 4 * q); b = *reinterpret_cast<const float4*>(rho + idx0 + 4 * q); }
            mv[4 * q] = a.x; mv[4 * q + 1] = a.y; mv[4 * q + 2] = a.z; mv[4 * q + 3] = a.w;
            sv[4 * q] = b.x; sv[4 * q + 1] = b.y; sv[4 * q + 2] = b.z; sv[4 * q + 3] = b.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { mv[e] = e < live ? mu[idx0 + e] : 0.f; sv[e] = e < live ? rho[idx0 + e] : 0.f; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = 0.f;
        if (e < live) {
            // z[(off + e) >> 2][(off + e) & 3] with compile-time indices (a runtime index would put z into scratch)
            float zsel;
            if constexpr (ALIGNED) zsel = z[e >> 2][e & 3];
            else zsel = off == 0 ? z[e >> 2][e & 3] : off == 1 ? z[(e + 1) >> 2][(e + 1) & 3]
                      : off == 2 ? z[(e + 2) >> 2][(e + 2) & 3] : z[(e + 3) >> 2][(e + 3) & 3];
            const float eps = eps_in ? eps_in[g0 + e] : zsel;
            // sigma = log1p(exp(rho)) does not depend on the sample: callers that draw many sets pass it precomputed
            v[e] = mv[e] + (sigma_given ? sv[e] : log1pf(expf(sv[e]))) * eps;
        }
    }
    u32x4 h, m, l;
    split8(v, h, m, l);
    u32x4* o = Wp + ((set * MT + mt) * KB + kb) * 3 * 64 + lane;
    o[0] = h; o[64] = m; o[128] = l;
}

__device__ __forceinline__ void sample_pack_x6_item(int64_t i, const float* __restrict__ mu, const float* __restrict__ rho,
                                                    const float* __restrict__ eps_in, u32x4* __restrict__ Wp, int M, int K, int MT, int KB,
                                                    uint64_t seed, uint64_t stream_id, int sigma_given) {
    const int lane = (int)(i & 63);
    // work items come in runs of 256 from a multiple of 256, so a wave holds one 64-lane block: its (set, row tile, k block) is decoded
    // once per wave on the scalar unit instead of three 64-bit divisions per lane
    const uint64_t ub = (uint64_t)(i >> 6);
    const int64_t blk = (int64_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(ub >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)ub));
    const int kb = (int)(blk % KB), mt = (int)((blk / KB) % MT);
    const int64_t set = blk / ((int64_t)KB * MT);
    // K % 4 == 0 makes set M K, row K and k0 multiples of 4 for every lane of the launch (every 1x1 tensor of the Stage-I net): the
    // branch is uniform over the tensor
    if ((K & 3) == 0) sample_pack_x6_draw<true>(set, mt, kb, lane, mu, rho, eps_in, Wp, M, K, MT, KB, seed, stream_id, sigma_given);
    else sample_pack_x6_draw<false>(set, mt, kb, lane, mu, rho, eps_in, Wp, M, K, MT, KB, seed, stream_id, sigma_given);
}

__global__ void sample_pack_x6_kernel(const float* __restrict__ mu, const float* __restrict__ rho, const float* __restrict__ eps_in,
                                      u32x4* __restrict__ Wp, int M, int K, int MT, int KB, int64_t total, uint64_t seed, uint64_t stream_id,
                                      const uint64_t* __restrict__ stream_add, int sigma_given) {
    const int64_t i = bem_gid1d();
    if (i >= total) return;
    if (stream_add) stream_id += stream_add[0];                          // device-resident part of the id (see randn_kernel)
    sample_pack_x6_item(i, mu, rho, eps_in, Wp, M, K, MT, KB, seed, stream_id, sigma_given);
}

// ---------------------------------------------------------------- Bayesian sampling ----------
// stream_add (all three samplers): an optional device-resident addend of the Philox stream id -- the per-iteration part of the id
// ([forward epoch] << 20, see SampleCtx.next_stream) kept in HBM so that a captured HIP graph of the step draws fresh numbers on
// every replay; NULL = the id is complete as passed.
__global__ void randn_kernel(float* __restrict__ out, int64_t total, uint64_t seed, uint64_t stream_id, const uint64_t* __restrict__ stream_add) {
    const int64_t i = bem_gid1d();
    if (stream_add) stream_id += stream_add[0];
    if (i < total) out[i] = philox_normal(i, seed, stream_id);
}

// one thread = four consecutive elements = one Philox counter block
__global__ void bnn_sample_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                  const float* __restrict__ eps_in, float* __restrict__ out, int64_t n, int64_t total,
                                  uint64_t seed, uint64_t stream_id, const uint64_t* __restrict__ stream_add) {
    const int64_t j = bem_gid1d();
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

// ------------------------------------------------------------------------------------------------------------------------
// All Bayesian tensors of a net drawn for a stochastic (eval) forward in ONE launch: the Stage-I net of the Monte-Carlo loop has 60
// Bayesian leaves / 90 tensors, i.e. 90 sampling launches per forward that sit between the layers' own kernels on planes of H/16 x W/16
// pixels, where every dependent launch costs >= 5 us whatever it does.  Segments of a flat output arena:
//   seg = { mu, sig (sigma = log1p(exp(rho)) precomputed for packed 1x1 weights, rho otherwise), first float of the tensor's nsets outputs
//           in the arena, n = elements per set, M, K (packed x6 operand order for the GEMM kernels; K = 0: natural order, as
//           bem_bnn_sample_f32 writes depthwise weights and biases), stream counter, work items, nsets * n }
//   blk = { segment, first work item }: one workgroup = 256 work items of one segment (packed: sample_pack_x6_item; natural: 4 elements)
// Values are those of bem_bnn_sample_pack_x6 (sigma_given) / bem_bnn_sample_f32 for (seed, stream_base + counter).
// ------------------------------------------------------------------------------------------------------------------------
struct ebank_seg { const float* mu; const float* sig; int64_t out; int64_t n; int32_t M, K; uint64_t counter; int64_t items; int64_t total; };
static_assert(sizeof(ebank_seg) == 8 * 8, "ebank_seg is eight 64-bit words (bem.modules.EvalSampleBank builds it as an int64 table)");
struct ebank_blk { int32_t seg; int32_t first; };

__global__ __launch_bounds__(256) void ebank_sample_kernel(const ebank_seg* __restrict__ segs, const ebank_blk* __restrict__ blks,
                                                           float* __restrict__ arena, uint64_t seed, uint64_t stream_base) {
    const ebank_blk bk = blks[blockIdx.x];
    const ebank_seg sg = segs[bk.seg];
    const int64_t i = (int64_t)bk.first * 256 + threadIdx.x;
    if (i >= sg.items) return;
    const uint64_t sid = stream_base + sg.counter;
    float* out = arena + sg.out;
    if (sg.K > 0) {
        sample_pack_x6_item(i, sg.mu, sg.sig, nullptr, reinterpret_cast<u32x4*>(out), sg.M, sg.K, (sg.M + 31) / 32, (sg.K + 15) / 16, seed, sid, 1);
        return;
    }
    const int64_t i0 = 4 * i, total = sg.total;                                       // natural order: total = nsets * n elements
    float z[4];
    philox_normal4(i, seed, sid, z);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t e = i0 + q;
        if (e < total) {
            const int64_t k = e % sg.n;
            out[e] = sg.mu[k] + log1pf(expf(sg.sig[k])) * z[q];
        }
    }
}

}  // namespace

extern "C" int64_t bem_pw_packed_elems(int M, int K) { return (int64_t)cdiv(M, 32) * cdiv(K, 2) * 64; }

extern "C" int bem_pack_pw_weight_f32(const float* W, float* Wp, int nsets, int M, int K, void* stream) {
    BEM_REQUIRE(W && Wp, "pack_pw_weight: null tensor");
    BEM_REQUIRE(nsets >= 0 && nsets <= 65535 && M > 0 && K > 0, "pack_pw_weight: bad shape");
    if (nsets == 0) return BEM_OK;
    const int MT = cdiv(M, 32), KS = cdiv(K, 2);
    dim3 grid((unsigned)cdiv64((int64_t)MT * KS * 64, 256), nsets);
    pack_pw_weight_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(W, Wp, M, K, MT, KS);
    return bem_check_launch("pack_pw_weight");
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

extern "C" int bem_randn_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, void* stream) {
    BEM_REQUIRE(out && n >= 0, "randn: bad arguments");
    if (n == 0) return BEM_OK;
    randn_kernel<<<GRID1D(n), 256, 0, (hipStream_t)stream>>>(out, n, seed, stream_id, stream_add);
    return bem_check_launch("randn");
}

extern "C" int bem_bnn_ebank_sample_f32(const void* segs, const void* blks, int nblk, float* arena, uint64_t seed, uint64_t stream_base,
                                        void* stream) {
    BEM_REQUIRE(segs && blks && arena && nblk > 0, "bnn_ebank_sample: bad arguments");
    BEM_REQUIRE(((uintptr_t)arena & 15) == 0, "bnn_ebank_sample: the arena must be 16-byte aligned");
    ebank_sample_kernel<<<nblk, 256, 0, (hipStream_t)stream>>>((const ebank_seg*)segs, (const ebank_blk*)blks, arena, seed, stream_base);
    return bem_check_launch("bnn_ebank_sample");
}

extern "C" int bem_bnn_sample_pack_x6(const float* mu, const float* rho, const float* eps_in, float* Wp, int nsets, int M, int K,
                                      uint64_t seed, uint64_t stream_id, const uint64_t* stream_add, int sigma_given, void* stream) {
    BEM_REQUIRE(mu && rho && Wp, "bnn_sample_pack_x6: null tensor");
    BEM_REQUIRE(nsets >= 0 && M > 0 && K > 0, "bnn_sample_pack_x6: bad shape");
    BEM_REQUIRE(((uintptr_t)Wp & 15) == 0, "bnn_sample_pack_x6: output must be 16-byte aligned");
    if (nsets == 0) return BEM_OK;
    const int MT = cdiv(M, 32), KB = cdiv(K, 16);
    const int64_t total = (int64_t)nsets * MT * KB * 64;
    sample_pack_x6_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(mu, rho, eps_in, reinterpret_cast<u32x4*>(Wp), M, K, MT, KB,
                                                                                       total, seed, stream_id, stream_add, sigma_given);
    return bem_check_launch("bnn_sample_pack_x6");
}

extern "C" int64_t bem_pw_x6_packed_elems(int M, int K) {       // in floats (4 per 16-byte vector)
    return (int64_t)cdiv(M, 32) * cdiv(K, 16) * 3 * 64 * 4;
}

extern "C" int bem_pack_pw_weight_x6_strided(const float* W, float* Wp, int nsets, int M, int K, int64_t set_stride, int64_t row_stride,
                                             int64_t col_stride, void* stream) {
    BEM_REQUIRE(W && Wp, "pack_pw_weight_x6: null tensor");
    BEM_REQUIRE(nsets >= 0 && M > 0 && K > 0 && set_stride >= 0 && row_stride >= 0 && col_stride >= 0, "pack_pw_weight_x6: bad shape / strides");
    BEM_REQUIRE(((uintptr_t)Wp & 15) == 0, "pack_pw_weight_x6: output must be 16-byte aligned");
    if (nsets == 0) return BEM_OK;
    const int MT = cdiv(M, 32), KB = cdiv(K, 16);
    const int64_t total = (int64_t)nsets * MT * KB * 64;
    pack_x6_kernel<<<GRID1D(total), 256, 0, (hipStream_t)stream>>>(W, reinterpret_cast<u32x4*>(Wp), M, K, MT, KB, total, set_stride,
                                                                                 row_stride, col_stride);
    return bem_check_launch("pack_pw_weight_x6");
}

extern "C" int bem_pack_pw_weight_x6_jobs(const void* jobs, const void* blks, int nblk, float* arena, void* stream) {
    BEM_REQUIRE(jobs && blks && arena && nblk > 0, "pack_pw_weight_x6_jobs: bad arguments");
    BEM_REQUIRE(((uintptr_t)arena & 15) == 0, "pack_pw_weight_x6_jobs: the arena must be 16-byte aligned");
    pack_x6_jobs_kernel<<<nblk, 256, 0, (hipStream_t)stream>>>((const packjob*)jobs, (const int32_t*)blks, arena);
    return bem_check_launch("pack_pw_weight_x6_jobs");
}

extern "C" int bem_pack_pw_weight_x6(const float* W, float* Wp, int nsets, int M, int K, void* stream) {
    return bem_pack_pw_weight_x6_strided(W, Wp, nsets, M, K, (int64_t)M * K, K, 1, stream);
}
