// Stand-alone host check of bem_batch_assemble_u8's argument handling: every call below must be refused on the host, before any launch,
// so the program needs no GPU.  The host tables are heap blocks of exactly the size the entry may read: built with
// AddressSanitizer / UBSan a read past a table or an overflow in the checks aborts the program.
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//       bayesian-enhancement-model_amd/csrc/abi.hip bayesian-enhancement-model_amd/csrc/batch_assemble.hip \
//       tests/host/batch_assemble_args.cpp -o batch_assemble_args && ./batch_assemble_args
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bem_hip.h"

namespace {

int failures = 0;

struct Call {
    std::vector<int64_t> table{0, 37, 53, 37 * 53 * 3, 64, 64, 37 * 53 * 3 + 64 * 64 * 3, 20, 70};
    std::vector<int32_t> plan{0, 5, 21, 7, 1, 32, 32, 2, 2, 0, 38, 0};
    int64_t arena = 37 * 53 * 3 + 64 * 64 * 3 + 20 * 70 * 3;
    int steps = 0, Sh = 32, Sw = 32, s = 16;
    bool noise = false, down = true, outputs = true;

    int run() const {
        // device pointers are never dereferenced on the host: any non-null value stands for them
        static float dummy;
        uint8_t* dev8 = reinterpret_cast<uint8_t*>(&dummy);
        float* out = outputs ? &dummy : nullptr;
        float* dn = down ? &dummy : nullptr;
        return bem_batch_assemble_u8(dev8, dev8, arena, table.data(), reinterpret_cast<const int64_t*>(&dummy), (int)(table.size() / 3),
                                     plan.data(), reinterpret_cast<const int32_t*>(&dummy), noise ? &dummy : nullptr, steps,
                                     (int)(plan.size() / 4), Sh, Sw, s, out, out, dn, dn, nullptr);
    }
};

void refused(const char* what, const Call& c, const char* word) {
    const int rc = c.run();
    const char* msg = bem_last_error();
    const bool ok = rc == BEM_ERR_INVALID && msg && strstr(msg, word);
    printf("%-44s rc=%d  %s  [%s]\n", what, rc, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg ? msg : "");
    failures += !ok;
}

}  // namespace

int main() {
    Call c;
    c.Sh = 16; c.Sw = 32; c.plan = {1, 0, 0, 2};
    refused("rotating mode on a rectangular crop", c, "rotates");
    c = Call(); c.Sh = 16; c.Sw = 32; c.plan = {1, 0, 0, 7};
    refused("rotating + flipped mode on a rectangle", c, "rotates");
    c = Call(); c.s = 12;
    refused("S % s != 0", c, "scale_down");
    c = Call(); c.s = 1; c.Sh = c.Sw = 32;
    refused("odd scale_down", c, "scale_down");
    c = Call(); c.plan[4] = 3;
    refused("image index == n_img", c, "names image");
    c = Call(); c.plan[8] = -1;
    refused("negative image index", c, "names image");
    c = Call(); c.plan[0] = INT32_MAX;
    refused("image index INT32_MAX", c, "names image");
    c = Call(); c.plan[1] = 6;                        // 37 - 32 = 5 is the last row offset
    refused("top past the image", c, "crops at");
    c = Call(); c.plan[10] = 39;                      // 70 - 32 = 38
    refused("left past the image", c, "crops at");
    c = Call(); c.plan[9] = 1;                        // the 20-row image is padded to 32: top must be 0
    refused("top != 0 on an image shorter than the crop", c, "crops at");
    c = Call(); c.plan[3] = 8;
    refused("mode 8", c, "mode");
    c = Call(); c.arena -= 1;
    refused("last image one byte past the arena", c, "outside the store");
    c = Call(); c.table[3] = INT64_MAX - 5;
    refused("image offset near INT64_MAX", c, "outside the store");
    c = Call(); c.table[1] = 1 << 20;
    refused("image height out of range", c, "outside the store");
    c = Call(); c.steps = 7;
    refused("label noise without a factor table", c, "label-noise");
    c = Call(); c.steps = 8; c.noise = true;
    refused("label-noise steps out of range", c, "label-noise");
    c = Call(); c.down = false;
    refused("scale_down without down planes", c, "down planes");
    c = Call(); c.s = 0;
    refused("down planes without scale_down", c, "down planes");
    c = Call(); c.outputs = false;
    refused("null outputs", c, "null output");
    printf(failures ? "%d check(s) failed\n" : "all refused on the host\n", failures);
    return failures != 0;
}
