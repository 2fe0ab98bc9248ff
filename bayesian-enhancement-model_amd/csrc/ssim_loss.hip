// SSIM loss of Stage-II training (basicsr/losses/my_loss.py:37-38: 1 - pytorch_msssim.ssim(y_true, y_pred, data_range=1.0,
// size_average=True)), forward and backward, on f32 tensors in [0,1]: no quantisation (bem_ssim_f32 in selection.hip is the uint8 / f64
// metric of the selection tail, forward only).
//
// Per (b,c) plane, with the normalised 11-tap Gaussian (sigma 1.5) applied separably, rows then columns, over the valid region only
// ((H-10) x (W-10) positions), m1 = G*x, my = G*y, m2 = G*x^2, my2 = G*y^2, m12 = G*xy, C1 = 0.01^2, C2 = 0.03^2:
//   A1 = 2 m1 my + C1    A2 = 2 (m12 - m1 my) + C2    B1 = m1^2 + my^2 + C1    B2 = (m2 - m1^2) + (my2 - my^2) + C2    S = A1 A2 / (B1 B2)
//   loss = weight * (1 - mean S)
// and, x alone taking a gradient, with three coefficient maps on the valid region
//   b = -S / B2    c = 2 A1 / (B1 B2)    a = 2 my (A2 - A1) / (B1 B2) - 2 m1 S (1 / B1 - 1 / B2)
//   dloss/dx = -(weight / Npos) (G^T a + 2 x G^T b + y G^T c),   G^T = the full correlation that takes a valid-region map back to H x W.
//
// Both kernels: one 256-thread workgroup per 32 x 32 tile of one plane, the 42 x 42 halo tiles staged in LDS, a row pass into LDS, a
// column pass into registers in which a thread slides the window down four consecutive rows (14 LDS reads per map for 4 results).
// LDS banking: ds_read_b32 / ds_write_b32 are served per 32-lane half, and in both passes a half reads (writes) 32 consecutive dwords
// of one row -- 32 different banks whatever the row stride -- so the row-pass tiles keep the stride 32; the halo tiles are 42 wide and
// padded to 43 so that the two rows a wave spans while staging (42 is even) do not start on the same bank pair.
// f32 throughout (the per-workgroup sum of S and the final sum are f64), window taps are literals, 32-bit offsets inside a plane and a
// 64-bit plane base.  Planes go through grid.y and grid.z (plane = z * SL_PY + y), so the 65535 limit of one grid dimension is not the
// cap: that is SL_PY * 65535 planes, refused above.
#include "bem_common.h"

namespace {

constexpr int SL_K = 11, SL_T = 32, SL_IN = SL_T + SL_K - 1, SL_INS = SL_IN + 1, SL_R = 4, SL_PY = 32768;
constexpr int64_t SL_MAX_PLANES = (int64_t)SL_PY * 65535;
constexpr float SL_C1 = 0.01f * 0.01f, SL_C2 = 0.03f * 0.03f;
static_assert(SL_T * SL_T == 256 * SL_R && SL_T == 32, "thread t owns column t & 31 and the SL_R rows from SL_R * (t >> 5)");

// exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, evaluated in f64 and rounded to f32; the loops that index it are fully unrolled
__device__ __forceinline__ constexpr float sl_g(int i) {
    constexpr float g[6] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055428e-01f, 2.660117149e-01f};
    return g[i < 6 ? i : 10 - i];
}

__device__ __forceinline__ int64_t sl_plane(int64_t planes) {
    const int64_t p = (int64_t)blockIdx.z * SL_PY + blockIdx.y;
    return p < planes ? p : -1;
}

// Column pass: acc[m][k] = sum_i g[i] rp[m][SL_R * oyg + k + i][ox], the window sliding down the thread's SL_R rows.
template <int NM>
__device__ __forceinline__ void sl_col_pass(const float (*rp)[SL_IN][SL_T], int oyg, int ox, float (&acc)[NM][SL_R]) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int k = 0; k < SL_R; ++k) acc[m][k] = 0.f;
#pragma unroll
    for (int r = 0; r < SL_K + SL_R - 1; ++r)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float v = rp[m][SL_R * oyg + r][ox];
#pragma unroll
            for (int k = 0; k < SL_R; ++k)
                if (r - k >= 0 && r - k < SL_K) acc[m][k] = fmaf(sl_g(r - k), v, acc[m][k]);
        }
}

// part[plane * tiles + tile] = sum of S over the tile's valid positions; coef (or NULL) = a | b | c, each (planes, vh, vw).
__global__ __launch_bounds__(256) void ssim_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, double* __restrict__ part,
                                                           float* __restrict__ coef, int64_t planes, int H, int W, int tiles_x) {
    __shared__ float sx[SL_IN][SL_INS], sy[SL_IN][SL_INS];
    __shared__ float rp[5][SL_IN][SL_T];
    __shared__ double red[4];
    const int64_t p = sl_plane(planes);
    if (p < 0) return;
    const int vh = H - (SL_K - 1), vw = W - (SL_K - 1);
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * SL_T, x0 = tx * SL_T;
    const float* px = pred + p * H * W;
    const float* py = gt + p * H * W;
    for (int i = threadIdx.x; i < SL_IN * SL_IN; i += 256) {
        const int r = i / SL_IN, c = i - r * SL_IN;
        const int gy = y0 + r, gx = x0 + c;
        const bool in = gy < H && gx < W;                      // outside the plane: zeros, read by masked positions only
        sx[r][c] = in ? px[gy * W + gx] : 0.f;
        sy[r][c] = in ? py[gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SL_IN * SL_T; i += 256) {
        const int r = i >> 5, c = i & 31;
        float s1 = 0.f, s2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
        for (int j = 0; j < SL_K; ++j) {
            const float x = sx[r][c + j], y = sy[r][c + j], g = sl_g(j);
            s1 = fmaf(g, x, s1); s2 = fmaf(g, y, s2);
            s11 = fmaf(g, x * x, s11); s22 = fmaf(g, y * y, s22); s12 = fmaf(g, x * y, s12);
        }
        rp[0][r][c] = s1; rp[1][r][c] = s2; rp[2][r][c] = s11; rp[3][r][c] = s22; rp[4][r][c] = s12;
    }
    __syncthreads();
    const int ox = threadIdx.x & 31, oyg = threadIdx.x >> 5;
    float acc[5][SL_R];
    sl_col_pass<5>(rp, oyg, ox, acc);
    const int64_t map = planes * vh * vw;
    float* pa = coef ? coef + p * vh * vw : nullptr;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < SL_R; ++k) {
        const int oy = y0 + SL_R * oyg + k;
        if (oy >= vh || x0 + ox >= vw) continue;
        const float m1 = acc[0][k], my = acc[1][k];
        // the three products and the sums built on them are rounded one by one: for pred == gt A1 == B1 and A2 == B2 bit for bit, and S
        // is one division of the two products (not a multiplication by a rounded reciprocal), so S = 1 and the loss is 0 exactly
        const float p11 = __fmul_rn(m1, m1), p22 = __fmul_rn(my, my), p12 = __fmul_rn(m1, my);
        const float A1 = __fadd_rn(2.f * p12, SL_C1), A2 = __fadd_rn(2.f * __fsub_rn(acc[4][k], p12), SL_C2);
        const float B1 = __fadd_rn(__fadd_rn(p11, p22), SL_C1);
        const float B2 = __fadd_rn(__fadd_rn(__fsub_rn(acc[2][k], p11), __fsub_rn(acc[3][k], p22)), SL_C2);
        const float B12 = __fmul_rn(B1, B2);
        const float iB = 1.f / B12;
        const float S = __fdiv_rn(__fmul_rn(A1, A2), B12);
        sum += (double)S;
        if (pa) {
            const int o = oy * vw + x0 + ox;
            pa[o] = 2.f * my * (A2 - A1) * iB - 2.f * m1 * S * (1.f / B1 - 1.f / B2);
            pa[map + o] = -S / B2;
            pa[2 * map + o] = 2.f * A1 * iB;
        }
    }
    sum = block_sum<4>(sum, red);
    if (threadIdx.x == 0) part[p * gridDim.x + blockIdx.x] = sum;
}

// One workgroup: thread t adds part[t], part[t + 256], ... in that order, the 256 sums go through block_sum: the same order every call.
__global__ __launch_bounds__(256) void ssim_loss_final_kernel(const double* __restrict__ part, int64_t n, float* __restrict__ loss, double weight,
                                                             double npos) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(weight * (1.0 - s / npos));       // a division: npos ones sum to a mean of exactly 1
}

// dpred = gmul * (k * (G^T a + 2 x G^T b + y G^T c)), k = -(weight / Npos).  The tile's pixels (y0 + iy, x0 + ix) take valid positions
// (y0 + iy - 10 + i, x0 + ix - 10 + j), i, j = 0..10, with taps g[10 - i] g[10 - j] = g[i] g[j]: the forward's two passes over halo tiles
// that start 10 positions up and left and hold zeros outside the valid region.
__global__ __launch_bounds__(256) void ssim_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ coef,
                                                           float* __restrict__ dpred, int64_t planes, int H, int W, int tiles_x, float k,
                                                           const float* __restrict__ gmul) {
    __shared__ float sc[3][SL_IN][SL_INS];
    __shared__ float rp[3][SL_IN][SL_T];
    const int64_t p = sl_plane(planes);
    if (p < 0) return;
    const int vh = H - (SL_K - 1), vw = W - (SL_K - 1);
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * SL_T, x0 = tx * SL_T;
    const int64_t map = planes * vh * vw;
    const float* pa = coef + p * vh * vw;
    for (int i = threadIdx.x; i < SL_IN * SL_IN; i += 256) {
        const int r = i / SL_IN, c = i - r * SL_IN;
        const int vy = y0 - (SL_K - 1) + r, vx = x0 - (SL_K - 1) + c;
        const bool in = vy >= 0 && vy < vh && vx >= 0 && vx < vw;
        const int o = in ? vy * vw + vx : 0;
        sc[0][r][c] = in ? pa[o] : 0.f;
        sc[1][r][c] = in ? pa[map + o] : 0.f;
        sc[2][r][c] = in ? pa[2 * map + o] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SL_IN * SL_T; i += 256) {
        const int r = i >> 5, c = i & 31;
        float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < SL_K; ++j)
#pragma unroll
            for (int m = 0; m < 3; ++m) s[m] = fmaf(sl_g(j), sc[m][r][c + j], s[m]);
#pragma unroll
        for (int m = 0; m < 3; ++m) rp[m][r][c] = s[m];
    }
    __syncthreads();
    const int ox = threadIdx.x & 31, oyg = threadIdx.x >> 5;
    float acc[3][SL_R];
    sl_col_pass<3>(rp, oyg, ox, acc);
    const float gm = gmul ? gmul[0] : 1.f;
    const int gx = x0 + ox;
#pragma unroll
    for (int r = 0; r < SL_R; ++r) {
        const int gy = y0 + SL_R * oyg + r;
        if (gy >= H || gx >= W) continue;
        const int64_t o = p * H * W + (gy * W + gx);
        const float x = pred[o], y = gt[o];
        // k * (...) is the gradient of the loss itself; gmul multiplies the rounded value, so gmul = 3 gives 3 x that gradient exactly
        dpred[o] = __fmul_rn(gm, __fmul_rn(k, fmaf(y, acc[2][r], fmaf(2.f * x, acc[1][r], acc[0][r]))));
    }
}

struct SlGrid {
    dim3 grid;
    int tiles_x;
    int64_t nwg;
};
// tiles of a th x tw region in grid.x, planes in grid.y / grid.z
SlGrid sl_grid(int64_t planes, int th, int tw) {
    const int tiles_x = cdiv(tw, SL_T), tiles = tiles_x * cdiv(th, SL_T);
    const unsigned gy = (unsigned)std::min<int64_t>(planes, SL_PY), gz = (unsigned)cdiv64(planes, SL_PY);
    return {dim3((unsigned)tiles, gy, gz), tiles_x, planes * tiles};
}

int sl_check(const char* what, int64_t planes, int H, int W) {
    BEM_REQUIRE(H >= SL_K && W >= SL_K, "%s: %d x %d planes are smaller than the 11x11 window", what, H, W);
    BEM_REQUIRE(planes > 0 && planes <= SL_MAX_PLANES, "%s: %lld planes (1 to %lld per call)", what, (long long)planes, (long long)SL_MAX_PLANES);
    BEM_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "%s: a %d x %d plane is too large for 32-bit offsets", what, H, W);
    return BEM_OK;
}

}  // namespace

extern "C" int bem_ssim_loss_tile(void) { return SL_T; }

extern "C" int64_t bem_ssim_loss_ws_elems(int64_t planes, int H, int W) {
    if (planes <= 0 || H < SL_K || W < SL_K) return 0;
    return sl_grid(planes, H - (SL_K - 1), W - (SL_K - 1)).nwg;
}

extern "C" int bem_ssim_loss_f32(const float* pred, const float* gt, float* loss, float* coef, double* ws, int64_t planes, int H, int W,
                                 float weight, void* stream) {
    BEM_REQUIRE(pred && gt && loss && ws, "ssim_loss: null pointer");
    if (int rc = sl_check("ssim_loss", planes, H, W)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int vh = H - (SL_K - 1), vw = W - (SL_K - 1);
    const SlGrid g = sl_grid(planes, vh, vw);
    ssim_loss_fwd_kernel<<<g.grid, 256, 0, s>>>(pred, gt, ws, coef, planes, H, W, g.tiles_x);
    ssim_loss_final_kernel<<<1, 256, 0, s>>>(ws, g.nwg, loss, (double)weight, (double)planes * vh * vw);
    return bem_check_launch("ssim_loss");
}

extern "C" int bem_ssim_loss_bwd_f32(const float* pred, const float* gt, const float* coef, float* dpred, int64_t planes, int H, int W,
                                     float weight, const float* gmul, void* stream) {
    BEM_REQUIRE(pred && gt && coef && dpred, "ssim_loss_bwd: null pointer");
    if (int rc = sl_check("ssim_loss_bwd", planes, H, W)) return rc;
    const SlGrid g = sl_grid(planes, H, W);
    const float k = (float)(-(double)weight / ((double)planes * (H - (SL_K - 1)) * (W - (SL_K - 1))));
    ssim_loss_bwd_kernel<<<g.grid, 256, 0, (hipStream_t)stream>>>(pred, gt, coef, dpred, planes, H, W, g.tiles_x, k, gmul);
    return bem_check_launch("ssim_loss_bwd");
}
