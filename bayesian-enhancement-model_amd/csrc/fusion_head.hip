// Output head of the two-branch Stage-II archs, forward and backward.
//
//   mode 0  fusion = Sequential(Conv2d(6,3,3,p=1), ReLU, Conv2d(3,3,3,p=1)) on cat(out_1, out_2)
//           (TunedModel_arch.py:315-319,406; FusedModel_arch.py:234-238,330)
//   mode 1  (out_1 + out_2) / 2  (TwoBranchNaive_arch.py:268)
//
// Mode 0 forward: one workgroup per TW x TH output tile.  The 6 input planes (3 from each branch output; the cat is never formed) are
// staged with a 2-pixel halo in LDS, h = relu(conv1 + b1) is formed on the tile plus a 1-pixel halo in LDS, then conv2 + b2.  h is ZERO
// outside the image (nn.Conv2d zero-pads h); a tile edge inside the image is no border, there h is the real relu(conv1).
//
// Mode 0 backward: the pre-activation is recomputed from the inputs (the forward saves nothing).  Per tile:
//   dpre = conv2^T(dout) * (pre > 0) on the tile + 1-pixel halo (0 outside the image: h is padding there, not a function of x),
//   dx = conv1^T(dpre) split back into do1 / do2,
//   the tile's share of dw1 / db1 / dw2 / db2: 81 (weight row, kernel row) groups x 3 column chunks, one per thread, summed in LDS in a
//   fixed order and written to a workspace of per-workgroup partials.  A second launch sums the partials per entry in f64 in a fixed
//   order and adds them into dw1 / db1 / dw2 / db2 (the += contract of bem_conv_wgrad_f32).  No float atomics: bitwise reproducible.
#include "bem_common.h"

namespace {

constexpr int FH_CI = 6, FH_CO = 3;                                   // conv1 6 -> 3, conv2 3 -> 3, both 3x3 pad 1
constexpr int FH_NW1 = FH_CO * FH_CI * 9, FH_NW2 = FH_CO * FH_CO * 9;
constexpr int FH_NP = FH_NW1 + FH_CO + FH_NW2 + FH_CO;               // 249 weight-gradient entries: dw1 | db1 | dw2 | db2
constexpr int FH_NT = 256;
constexpr int FH_TW = 64;
constexpr int FH_TH_FWD = 16, FH_TH_BWD = 8;
constexpr int FH_NCH = 3;                                             // column chunks of the weight-gradient sums
constexpr int FH_NG = (FH_NW1 + FH_NW2) / 3;                          // 81 groups of 3 taps (one kernel row)
static_assert(FH_NG * FH_NCH <= FH_NT, "one weight-gradient unit per thread");

template <int TH>
struct Tile {
    static constexpr int XH = TH + 4, XW = FH_TW + 4;                 // input / dout window: 2-pixel halo
    static constexpr int HH = TH + 2, HW = FH_TW + 2;                 // h / dpre window: 1-pixel halo
    static constexpr int XP = XH * XW, HP = HH * HW;
};

__device__ __forceinline__ void tile_origin(int tilesX, int tilesY, int th, int& b, int& y0, int& x0) {
    int t = blockIdx.x;
    const int tx = t % tilesX;
    t /= tilesX;
    y0 = (t % tilesY) * th;
    b = t / tilesY;
    x0 = tx * FH_TW;
}

// 3 planes (plane stride HWp) of the RH x RW window at image (y0, x0) into LDS, zero outside the image
template <int RH, int RW>
__device__ __forceinline__ void stage3(float* __restrict__ dst, const float* __restrict__ src, int64_t HWp, int H, int W, int y0, int x0) {
    for (int i = threadIdx.x; i < 3 * RH * RW; i += FH_NT) {
        const int c = i / (RH * RW), r = (i / RW) % RH, q = i % RW;
        const int y = y0 + r, x = x0 + q;
        float v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) v = src[c * HWp + (int64_t)y * W + x];
        dst[i] = v;
    }
}

// conv1 + b1 at h-window position (r, q): its 3x3 input neighbourhood is rows r..r+2, cols q..q+2 of the input window
template <int TH>
__device__ __forceinline__ void conv1_at(const float* __restrict__ xs, int r, int q, const float* __restrict__ w1, const float* __restrict__ b1,
                                         float (&pre)[FH_CO]) {
    using T = Tile<TH>;
#pragma unroll
    for (int c = 0; c < FH_CO; ++c) pre[c] = b1[c];
#pragma unroll
    for (int i = 0; i < FH_CI; ++i)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float v = valu_copy(xs[(i * T::XH + r + ky) * T::XW + q + kx]);
#pragma unroll
                for (int c = 0; c < FH_CO; ++c) pre[c] = fmaf(w1[((c * FH_CI + i) * 3 + ky) * 3 + kx], v, pre[c]);
            }
}

__global__ __launch_bounds__(FH_NT) void fusion_head_kernel(const float* __restrict__ o1, int64_t bs1, const float* __restrict__ o2, int64_t bs2,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
                                                            int H, int W, int tilesX, int tilesY) {
    constexpr int TH = FH_TH_FWD;
    using T = Tile<TH>;
    __shared__ float xs[FH_CI * T::XP];
    __shared__ float hs[FH_CO * T::HP];
    int b, y0, x0;
    tile_origin(tilesX, tilesY, TH, b, y0, x0);
    const int64_t HWp = (int64_t)H * W;
    stage3<T::XH, T::XW>(xs, o1 + b * bs1, HWp, H, W, y0 - 2, x0 - 2);
    stage3<T::XH, T::XW>(xs + 3 * T::XP, o2 + b * bs2, HWp, H, W, y0 - 2, x0 - 2);
    __syncthreads();
    for (int i = threadIdx.x; i < T::HP; i += FH_NT) {
        const int r = i / T::HW, q = i % T::HW;
        const int y = y0 - 1 + r, x = x0 - 1 + q;
        float pre[FH_CO];
        conv1_at<TH>(xs, r, q, w1, b1, pre);
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
        for (int c = 0; c < FH_CO; ++c) hs[c * T::HP + i] = in && pre[c] > 0.f ? pre[c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * FH_TW; i += FH_NT) {
        const int r = i / FH_TW, q = i % FH_TW;
        const int y = y0 + r, x = x0 + q;
        if (y >= H || x >= W) continue;
        float o[FH_CO];
#pragma unroll
        for (int k = 0; k < FH_CO; ++k) o[k] = b2[k];
#pragma unroll
        for (int c = 0; c < FH_CO; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = valu_copy(hs[(c * T::HH + r + ky) * T::HW + q + kx]);
#pragma unroll
                    for (int k = 0; k < FH_CO; ++k) o[k] = fmaf(w2[((k * FH_CO + c) * 3 + ky) * 3 + kx], v, o[k]);
                }
        float* op = out + (int64_t)b * FH_CO * HWp + (int64_t)y * W + x;
#pragma unroll
        for (int k = 0; k < FH_CO; ++k) op[k * HWp] = o[k];
    }
}

__global__ __launch_bounds__(FH_NT) void fusion_head_bwd_kernel(const float* __restrict__ o1, int64_t bs1, const float* __restrict__ o2, int64_t bs2,
                                                                const float* __restrict__ dout, const float* __restrict__ w1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                float* __restrict__ do1, float* __restrict__ do2, float* __restrict__ ws,
                                                                int nwg, int H, int W, int tilesX, int tilesY) {
    constexpr int TH = FH_TH_BWD;
    using T = Tile<TH>;
    __shared__ float xs[FH_CI * T::XP];          // inputs, 2-pixel halo
    __shared__ float ds[FH_CO * T::XP];          // dout, 2-pixel halo
    __shared__ float hs[FH_CO * T::HP];          // h, 1-pixel halo
    __shared__ float gs[FH_CO * T::HP];          // dpre, 1-pixel halo
    __shared__ float part[FH_NG * FH_NCH * 4];
    int b, y0, x0;
    tile_origin(tilesX, tilesY, TH, b, y0, x0);
    const int64_t HWp = (int64_t)H * W;
    stage3<T::XH, T::XW>(xs, o1 + b * bs1, HWp, H, W, y0 - 2, x0 - 2);
    stage3<T::XH, T::XW>(xs + 3 * T::XP, o2 + b * bs2, HWp, H, W, y0 - 2, x0 - 2);
    stage3<T::XH, T::XW>(ds, dout + (int64_t)b * FH_CO * HWp, HWp, H, W, y0 - 2, x0 - 2);
    __syncthreads();
    // h and dpre on the tile + 1-pixel halo
    for (int i = threadIdx.x; i < T::HP; i += FH_NT) {
        const int r = i / T::HW, q = i % T::HW;
        const int y = y0 - 1 + r, x = x0 - 1 + q;
        float h[FH_CO] = {0.f, 0.f, 0.f}, g[FH_CO] = {0.f, 0.f, 0.f};
        if (y >= 0 && y < H && x >= 0 && x < W) {
            float pre[FH_CO], dh[FH_CO] = {0.f, 0.f, 0.f};
            conv1_at<TH>(xs, r, q, w1, b1, pre);
#pragma unroll
            for (int k = 0; k < FH_CO; ++k)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float v = valu_copy(ds[(k * T::XH + r + 2 - ky) * T::XW + q + 2 - kx]);
#pragma unroll
                        for (int c = 0; c < FH_CO; ++c) dh[c] = fmaf(w2[((k * FH_CO + c) * 3 + ky) * 3 + kx], v, dh[c]);
                    }
#pragma unroll
            for (int c = 0; c < FH_CO; ++c) {
                const bool on = pre[c] > 0.f;                 // threshold_backward: the gradient at exactly 0 is 0
                h[c] = on ? pre[c] : 0.f;
                g[c] = on ? dh[c] : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < FH_CO; ++c) {
            hs[c * T::HP + i] = h[c];
            gs[c * T::HP + i] = g[c];
        }
    }
    __syncthreads();
    // dx = conv1^T(dpre) on the tile
    for (int i = threadIdx.x; i < TH * FH_TW; i += FH_NT) {
        const int r = i / FH_TW, q = i % FH_TW;
        const int y = y0 + r, x = x0 + q;
        if (y >= H || x >= W) continue;
        float dx[FH_CI];
#pragma unroll
        for (int j = 0; j < FH_CI; ++j) dx[j] = 0.f;
#pragma unroll
        for (int c = 0; c < FH_CO; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = valu_copy(gs[(c * T::HH + r + 2 - ky) * T::HW + q + 2 - kx]);
#pragma unroll
                    for (int j = 0; j < FH_CI; ++j) dx[j] = fmaf(w1[((c * FH_CI + j) * 3 + ky) * 3 + kx], v, dx[j]);
                }
        const int64_t o = (int64_t)b * FH_CO * HWp + (int64_t)y * W + x;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            do1[o + j * HWp] = dx[j];
            do2[o + j * HWp] = dx[3 + j];
        }
    }
    // weight-gradient partials of this tile: unit = (group, column chunk); a group is 3 taps of one kernel row
    const int u = threadIdx.x;
    if (u < FH_NG * FH_NCH) {
        const int grp = u / FH_NCH, ch = u % FH_NCH;
        const int q0 = ch * FH_TW / FH_NCH, q1 = (ch + 1) * FH_TW / FH_NCH;
        float acc[3] = {0.f, 0.f, 0.f}, accb = 0.f;
        // dw1 group (c, i, ky): sum_p dpre[c, p] x[i, p + (ky - 1, kx - 1)];  dw2 group (o, c, ky): sum_p dout[o, p] h[c, p + (ky - 1, kx - 1)]
        const float *gp, *xp;
        int gstride, xstride;
        if (grp < FH_NW1 / 3) {
            const int c = grp / (FH_CI * 3), i = (grp / 3) % FH_CI, ky = grp % 3;
            gp = gs + (c * T::HH + 1) * T::HW + 1;                // dpre at tile row 0, col 0
            gstride = T::HW;
            xp = xs + (i * T::XH + 1 + ky) * T::XW + 1;           // x at (row ky - 1, col -1) relative to the tile origin
            xstride = T::XW;
        } else {
            const int g2 = grp - FH_NW1 / 3;
            const int o = g2 / 9, c = (g2 / 3) % 3, ky = g2 % 3;
            gp = ds + (o * T::XH + 2) * T::XW + 2;                // dout at tile row 0, col 0
            gstride = T::XW;
            xp = hs + (c * T::HH + ky) * T::HW;                   // h at (row ky - 1, col -1)
            xstride = T::HW;
        }
        for (int r = 0; r < TH; ++r) {
            const float* g = gp + r * gstride;
            const float* xr = xp + r * xstride;
            float xa = xr[q0], xb = xr[q0 + 1];
            for (int q = q0; q < q1; ++q) {
                const float xc = xr[q + 2];
                const float gv = g[q];
                acc[0] = fmaf(gv, xa, acc[0]);
                acc[1] = fmaf(gv, xb, acc[1]);
                acc[2] = fmaf(gv, xc, acc[2]);
                accb += gv;
                xa = xb;
                xb = xc;
            }
        }
        float* pp = part + u * 4;
        pp[0] = acc[0];
        pp[1] = acc[1];
        pp[2] = acc[2];
        pp[3] = accb;
    }
    __syncthreads();
    if (threadIdx.x < FH_NP) {
        const int e = threadIdx.x;
        int grp, slot;
        if (e < FH_NW1) { grp = e / 3; slot = e % 3; }
        else if (e < FH_NW1 + FH_CO) { grp = (e - FH_NW1) * FH_CI * 3; slot = 3; }                 // db1[c]: group (c, 0, 0)
        else if (e < FH_NW1 + FH_CO + FH_NW2) { const int k = e - FH_NW1 - FH_CO; grp = FH_NW1 / 3 + k / 3; slot = k % 3; }
        else { grp = FH_NW1 / 3 + (e - FH_NW1 - FH_CO - FH_NW2) * 9; slot = 3; }                   // db2[o]: group (o, 0, 0)
        float s = 0.f;
#pragma unroll
        for (int ch = 0; ch < FH_NCH; ++ch) s += part[(grp * FH_NCH + ch) * 4 + slot];
        ws[(int64_t)e * nwg + blockIdx.x] = s;
    }
}

// entry e of [dw1 | db1 | dw2 | db2] += sum over the nwg workgroup partials (f64, fixed order)
__global__ __launch_bounds__(FH_NT) void fusion_head_wsum_kernel(const float* __restrict__ ws, int nwg, float* __restrict__ dw1, float* __restrict__ db1,
                                                                 float* __restrict__ dw2, float* __restrict__ db2) {
    __shared__ double red[FH_NT];
    const int e = blockIdx.x;
    const float* p = ws + (int64_t)e * nwg;
    double s = 0.0;
    for (int j = threadIdx.x; j < nwg; j += FH_NT) s += (double)p[j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = FH_NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* dst;
        if (e < FH_NW1) dst = dw1 + e;
        else if (e < FH_NW1 + FH_CO) dst = db1 + (e - FH_NW1);
        else if (e < FH_NW1 + FH_CO + FH_NW2) dst = dw2 + (e - FH_NW1 - FH_CO);
        else dst = db2 + (e - FH_NW1 - FH_CO - FH_NW2);
        *dst = (float)((double)*dst + red[0]);
    }
}

// mode 1: out = (o1 + o2) / 2; backward: do1 = do2 = dout / 2
template <bool BWD>
__global__ __launch_bounds__(FH_NT) void fusion_mean_kernel(const float* __restrict__ a, int64_t bsa, const float* __restrict__ c, int64_t bsc,
                                                            float* __restrict__ y0, float* __restrict__ y1, int64_t n3, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * FH_NT + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / n3, k = i % n3;
    if (BWD) {
        const float g = a[i] * 0.5f;
        y0[i] = g;
        y1[i] = g;
    } else {
        y0[i] = (a[b * bsa + k] + c[b * bsc + k]) * 0.5f;
    }
}

int check_head(const char* what, int B, int Cin, int Cout, int H, int W, int mode) {
    BEM_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0: conv head, 1: mean)", what, mode);
    BEM_REQUIRE(Cout == FH_CO && Cin == FH_CI, "%s: C_out=%d C_in=%d: only C_out 3 / C_in 6 (out_channels 3 of both branches) are supported",
                what, Cout, Cin);
    BEM_REQUIRE(B >= 0 && H >= 0 && W >= 0 && (int64_t)B * FH_CO * H * W < (1ll << 40), "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    return BEM_OK;
}

int64_t head_tiles(int B, int H, int W, int th, int& tilesX, int& tilesY) {
    tilesX = cdiv(W, FH_TW);
    tilesY = cdiv(H, th);
    return (int64_t)B * tilesX * tilesY;
}

}  // namespace

extern "C" int bem_fusion_head_f32(const float* o1, int64_t o1_bstride, const float* o2, int64_t o2_bstride, const float* w1, const float* b1,
                                   const float* w2, const float* b2, float* out, int B, int Cin, int Cout, int H, int W, int mode, void* stream) {
    BEM_REQUIRE(o1 && o2 && out, "fusion_head: null tensor");
    BEM_REQUIRE(mode != 0 || (w1 && b1 && w2 && b2), "fusion_head: null weight");
    if (int rc = check_head("fusion_head", B, Cin, Cout, H, W, mode)) return rc;
    const int64_t n3 = (int64_t)FH_CO * H * W;
    const int64_t bs1 = o1_bstride ? o1_bstride : n3, bs2 = o2_bstride ? o2_bstride : n3;
    BEM_REQUIRE(bs1 >= n3 && bs2 >= n3, "fusion_head: batch strides %lld / %lld below 3*H*W = %lld", (long long)bs1, (long long)bs2, (long long)n3);
    if (B == 0 || H == 0 || W == 0) return BEM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (mode == 1) {
        const int64_t total = (int64_t)B * n3;
        hipLaunchKernelGGL(fusion_mean_kernel<false>, dim3((unsigned)cdiv64(total, FH_NT)), dim3(FH_NT), 0, s, o1, bs1, o2, bs2, out, nullptr, n3, total);
        return bem_check_launch("fusion_head mean");
    }
    int tx, ty;
    const int64_t nwg = head_tiles(B, H, W, FH_TH_FWD, tx, ty);
    BEM_REQUIRE(nwg < (1ll << 31), "fusion_head: %lld tiles", (long long)nwg);
    hipLaunchKernelGGL(fusion_head_kernel, dim3((unsigned)nwg), dim3(FH_NT), 0, s, o1, bs1, o2, bs2, w1, b1, w2, b2, out, H, W, tx, ty);
    return bem_check_launch("fusion_head");
}

extern "C" int64_t bem_fusion_head_bwd_ws_elems(int B, int H, int W) {
    if (B < 0 || H < 0 || W < 0) return 0;
    int tx, ty;
    return (int64_t)FH_NP * head_tiles(B, H, W, FH_TH_BWD, tx, ty);
}

extern "C" int bem_fusion_head_bwd_f32(const float* o1, int64_t o1_bstride, const float* o2, int64_t o2_bstride, const float* dout,
                                       const float* w1, const float* b1, const float* w2, float* do1, float* do2, float* dw1, float* db1,
                                       float* dw2, float* db2, float* ws, int64_t ws_elems, int B, int Cin, int Cout, int H, int W, int mode,
                                       void* stream) {
    BEM_REQUIRE(dout && do1 && do2, "fusion_head_bwd: null tensor");
    BEM_REQUIRE(mode != 0 || (o1 && o2 && w1 && b1 && w2 && dw1 && db1 && dw2 && db2 && ws), "fusion_head_bwd: null tensor or weight");
    if (int rc = check_head("fusion_head_bwd", B, Cin, Cout, H, W, mode)) return rc;
    const int64_t n3 = (int64_t)FH_CO * H * W;
    hipStream_t s = (hipStream_t)stream;
    if (mode == 1) {
        if (B == 0 || H == 0 || W == 0) return BEM_OK;
        const int64_t total = (int64_t)B * n3;
        hipLaunchKernelGGL(fusion_mean_kernel<true>, dim3((unsigned)cdiv64(total, FH_NT)), dim3(FH_NT), 0, s, dout, n3, nullptr, n3, do1, do2, n3, total);
        return bem_check_launch("fusion_head_bwd mean");
    }
    const int64_t bs1 = o1_bstride ? o1_bstride : n3, bs2 = o2_bstride ? o2_bstride : n3;
    BEM_REQUIRE(bs1 >= n3 && bs2 >= n3, "fusion_head_bwd: batch strides %lld / %lld below 3*H*W = %lld", (long long)bs1, (long long)bs2,
                (long long)n3);
    const int64_t need = bem_fusion_head_bwd_ws_elems(B, H, W);
    BEM_REQUIRE(ws_elems >= need, "fusion_head_bwd: workspace of %lld floats, %lld needed", (long long)ws_elems, (long long)need);
    if (B == 0 || H == 0 || W == 0) return BEM_OK;
    int tx, ty;
    const int64_t nwg = head_tiles(B, H, W, FH_TH_BWD, tx, ty);
    BEM_REQUIRE(nwg < (1ll << 31), "fusion_head_bwd: %lld tiles", (long long)nwg);
    hipLaunchKernelGGL(fusion_head_bwd_kernel, dim3((unsigned)nwg), dim3(FH_NT), 0, s, o1, bs1, o2, bs2, dout, w1, b1, w2, do1, do2, ws, (int)nwg, H,
                       W, tx, ty);
    if (int rc = bem_check_launch("fusion_head_bwd")) return rc;
    hipLaunchKernelGGL(fusion_head_wsum_kernel, dim3(FH_NP), dim3(FH_NT), 0, s, ws, (int)nwg, dw1, db1, dw2, db2);
    return bem_check_launch("fusion_head_bwd wsum");
}
