// csrc/hvd_bit_order.h as a program of its own (tests/test_bit_order_cpu.py builds it with g++ -fsanitize=address,undefined):
// stdin = records of one uint32 sample + 256 * 256 uint32 counts, stdout = per record the sample rule of n = sample (forced and
// not) and the 256 bytes of the chosen order, as text.
#include <stdio.h>

#include <vector>

#include "../../hydrus-video-deduplicator_amd/csrc/hvd_bit_order.h"

int main() {
    std::vector<uint32_t> cooc(256 * 256);
    uint32_t sample = 0;
    while (fread(&sample, 4, 1, stdin) == 1) {
        if (fread(cooc.data(), 4, cooc.size(), stdin) != cooc.size()) return 2;
        uint8_t perm[256];
        hvd::bit_order_from_cooc(cooc.data(), sample, perm);
        const hvd::BitSample f = hvd::bit_order_sample(sample, true), a = hvd::bit_order_sample(sample, false);
        printf("%u %u %u %u %u %u", f.sample, f.stride, f.words, a.sample, a.stride, a.words);
        for (int k = 0; k < 256; ++k) printf(" %d", (int)perm[k]);
        printf("\n");
    }
    return 0;
}
