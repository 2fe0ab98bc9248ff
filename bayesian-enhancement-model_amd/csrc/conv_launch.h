// What conv.hip (bem_conv2d_route, bem_conv2d_f32) uses of conv_x6.hip: the two x6 launchers and the row form's two conditions.
#pragma once
#include <stdint.h>

// the shapes of the row form: KS = 3 (stride 1) W, KS = 4 (stride 2) Wo = W / 2 a power of two of at most 32 lanes of 4 / stride pixels
bool conv_rows_shape(int KS, int Cin, int H, int W);
// 16-byte rows: every pointer given (NULL = absent, or an allocation of the caller's own) and the batch stride of x
bool conv_rows_aligned(const float* x, int64_t x_bstride, const float* out, const float* res1, const float* res2);
int conv_rows_launch(int KS, const float* x, int64_t x_bstride, const float* Wp, const float* bias, const float* res1, const float* res2, float* out,
                     int B, int Cin, int H, int W, int Cout, int relu, int res1_rep, void* stream);
int conv_taps_launch(const float* x, int64_t x_bstride, const float* Wp, const float* bias, const float* res1, const float* res2, float* out,
                     int B, int Cin, int H, int W, int Cout, int KH, int stride, int pad, int dil, int relu, int res1_rep, void* stream);
