// Stand-alone host check of the argument handling of the LPIPS loss entries (bem_lpips_layer_bwd_f32, bem_relu_pool3s2_bwd_f32,
// bem_lpips_prep_bwd_f32, bem_lpips_mean_f32): every call below must be refused on the host, before any launch, so the program needs no
// GPU.  Built with AddressSanitizer / UBSan an overflow in the extent and stride checks aborts the program.
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//       bayesian-enhancement-model_amd/csrc/abi.hip bayesian-enhancement-model_amd/csrc/lpips.hip \
//       tests/host/lpips_bwd_args.cpp -o lpips_bwd_args && ./lpips_bwd_args
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bem_hip.h"

namespace {

int failures = 0;
// device pointers are never dereferenced on the host: any non-null value stands for them
float dummy;
double dummy64;

struct Head {
    const float *feat = &dummy, *lin = &dummy;
    float* dz = &dummy;
    int64_t f_bs = 64 * 35, f_cs = 35, f_rs = 7, d_bs = 64 * 35, d_cs = 35, d_rs = 7;
    int B = 2, C = 64, h = 5, w = 7, oh = 5, ow = 7, oy = 0, ox = 0;
    int run() const {
        return bem_lpips_layer_bwd_f32(feat, f_bs, f_cs, f_rs, lin, nullptr, nullptr, 0.25f, dz, d_bs, d_cs, d_rs, B, C, h, w, oh, ow, oy, ox,
                                       nullptr);
    }
};

void refused(const char* what, int rc, const char* word) {
    const char* msg = bem_last_error();
    const bool ok = rc == BEM_ERR_INVALID && msg && strstr(msg, word);
    printf("%-52s rc=%d  %s  [%s]\n", what, rc, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg ? msg : "");
    failures += !ok;
}

}  // namespace

int main() {
    Head c;
    c.feat = nullptr;
    refused("head: null feature", c.run(), "null");
    c = Head(); c.dz = nullptr;
    refused("head: null output", c.run(), "null");
    c = Head(); c.B = 0;
    refused("head: empty batch", c.run(), "bad shape");
    c = Head(); c.C = -1;
    refused("head: negative channel count", c.run(), "bad shape");
    c = Head(); c.w = 0;
    refused("head: empty plane", c.run(), "bad shape");
    c = Head(); c.oy = 1;
    refused("head: crop one row past the output", c.run(), "does not lie");
    c = Head(); c.ox = -1;
    refused("head: negative origin", c.run(), "does not lie");
    c = Head(); c.oy = INT32_MAX;
    refused("head: origin INT32_MAX", c.run(), "does not lie");
    c = Head(); c.oh = 1 << 16; c.ow = 1 << 16; c.d_rs = 1 << 16; c.d_cs = (int64_t)1 << 32; c.d_bs = (int64_t)1 << 38;
    refused("head: output extent past 2^31 positions", c.run(), "does not lie");
    c = Head(); c.f_rs = 6;
    refused("head: feature row stride below the width", c.run(), "feature strides");
    c = Head(); c.f_bs = 63 * 35;
    refused("head: feature batch stride below C planes", c.run(), "feature strides");
    c = Head(); c.oh = 7; c.ow = 8;
    refused("head: output strides of the crop, not the extent", c.run(), "output strides");

    refused("pool: null gradient", bem_relu_pool3s2_bwd_f32(&dummy, 35, 7, nullptr, &dummy, 1, 5, 7, nullptr), "null");
    refused("pool: no planes", bem_relu_pool3s2_bwd_f32(&dummy, 35, 7, &dummy, &dummy, 0, 5, 7, nullptr), "3 x 3");
    refused("pool: plane below the window", bem_relu_pool3s2_bwd_f32(&dummy, 35, 7, &dummy, &dummy, 1, 5, 2, nullptr), "3 x 3");
    refused("pool: plane stride below the plane", bem_relu_pool3s2_bwd_f32(&dummy, 34, 7, &dummy, &dummy, 1, 5, 7, nullptr), "strides");
    refused("pool: element count past the grid", bem_relu_pool3s2_bwd_f32(&dummy, (int64_t)1 << 40, 1 << 20, &dummy, &dummy, (int64_t)1 << 30,
                                                                        1 << 20, 1 << 20, nullptr), "too large");

    refused("prep: null output", bem_lpips_prep_bwd_f32(&dummy, nullptr, 1, 31, 31, 0, nullptr), "null");
    refused("prep: empty batch", bem_lpips_prep_bwd_f32(&dummy, &dummy, 0, 31, 31, 0, nullptr), "batch size");
    refused("prep: 30 rows", bem_lpips_prep_bwd_f32(&dummy, &dummy, 1, 30, 31, 0, nullptr), "31 x 31");
    refused("prep: 30 columns", bem_lpips_prep_bwd_f32(&dummy, &dummy, 1, 31, 30, 2, nullptr), "31 x 31");
    refused("prep: the quantising mode", bem_lpips_prep_bwd_f32(&dummy, &dummy, 1, 31, 31, 1, nullptr), "mode 1");
    refused("prep: mode 3", bem_lpips_prep_bwd_f32(&dummy, &dummy, 1, 31, 31, 3, nullptr), "mode 3");
    refused("prep: image past the grid", bem_lpips_prep_bwd_f32(&dummy, &dummy, 32767, INT32_MAX, INT32_MAX, 0, nullptr), "too large");

    refused("mean: null sums", bem_lpips_mean_f32(nullptr, &dummy, 1, 1.f, nullptr), "null");
    refused("mean: empty batch", bem_lpips_mean_f32(&dummy64, &dummy, 0, 1.f, nullptr), "batch size");
    printf(failures ? "%d check(s) failed\n" : "all refused on the host\n", failures);
    return failures != 0;
}
