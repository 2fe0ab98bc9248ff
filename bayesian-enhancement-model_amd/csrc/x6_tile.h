// The 4 x 32 pixel tile with a one-pixel halo that gdmlp_x6.hip and ss2d_front_x6.hip share: geometry and the workgroup's tile origin.
// One workgroup = 4 waves = one tile of one image (blockIdx.z); the 6 x 34 halo is 204 pixels = 7 MFMA pixel blocks of 32, wave w owns blocks
// w and w + 4.  The LayerNorm halo prologue (load with clamped address and mask, normalise, split8) is still written out in each kernel: as
// shared __forceinline__ templates it compiled to different machine code in all nine kernels (profiles/x6_layout_symbols.txt).
#pragma once
#include "x6_common.h"

namespace {

constexpr int XT_TH = 4, XT_TW = 32, XT_HW = XT_TW + 2;
constexpr int XT_NPH = (XT_TH + 2) * XT_HW;          // 204 halo pixels
constexpr int XT_NPB = (XT_NPH + 31) / 32;           // 7 blocks
constexpr int XT_TS = 208;                           // row stride of T (>= 205: the clamp slot of the unused lanes of block 6)

typedef float f32x4 __attribute__((ext_vector_type(4)));

// origin of this workgroup's tile; tx = tiles per image row, grid.x = all tiles of an image
__device__ __forceinline__ void tile_origin(int tx, int& y0, int& x0) {
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tyi = tile / tx, txi = tile - tyi * tx;
    y0 = tyi * XT_TH;
    x0 = txi * XT_TW;
}

}  // namespace
