// hvd_bit_order.h -- the host side of the video search's data-dependent bit order (k_fp4_image.hip: k_bit_rows, k_bit_cooc,
// k_reorder_bits): which hashes of a library are sampled, and which 128 bits the co-occurrence counts of that sample keep for the
// first stage. No HIP in here: any host C++17 compiler takes it, like hvd_mfma_forms.h. The ONE definition of both rules: the
// search (hvd_search.cpp: choose_bit_order) and the tests' entry points (hvd_dev_bit_cooc, hvd_bit_order_from_cooc) call these.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace hvd {

// The sample of a library of n hashes: `sample` hashes (whole 64-hash words, at most 16384), every stride-th one from hash 0 on;
// words = sample / 64. sample = 0: too few hashes to choose an order from (fewer than 4096, or fewer than 64 when forced).
struct BitSample {
    uint32_t sample, stride, words;
};
inline BitSample bit_order_sample(uint32_t n, bool forced) {
    const uint32_t sample = std::min<uint32_t>(n, 16384u) & ~63u;
    if (sample < (forced ? 64u : 4096u)) return {0u, 0u, 0u};
    return {sample, n / sample, sample / 64u};
}

// Which 128 bits should the first stage see? (k_fp4_image.hip: "data-dependent bit order".) cooc[i][j] = number of the `sample`
// hashes with bits i and j both set (diagonal: with bit i set). Pearson correlation of every pair of bits (a constant bit
// correlates fully with everything), then 128 times drop the bit whose summed |correlation| with the bits still in the set is
// largest. perm = the 128 kept bits in ascending order, then the dropped ones: bit k of a rewritten hash is bit perm[k] of the
// original. Deterministic in the counts -- plain double arithmetic in a fixed order, ties by bit number -- so every rank of a
// sharded search arrives at the same order.
inline void bit_order_from_cooc(const uint32_t cooc[256 * 256], uint32_t sample, uint8_t perm[256]) {
    const double N = (double)sample;
    std::vector<double> pr(256), sd(256), a(256 * 256, 0.0), load(256, 0.0);
    for (int i = 0; i < 256; ++i) {
        pr[i] = cooc[(size_t)i * 257] / N;
        sd[i] = std::sqrt(std::max(0.0, pr[i] * (1.0 - pr[i])));
    }
    for (int i = 0; i < 256; ++i)
        for (int j = 0; j < 256; ++j) {
            if (i == j) continue;
            const double r = (sd[i] < 1e-6 || sd[j] < 1e-6) ? 1.0 : (cooc[(size_t)i * 256 + j] / N - pr[i] * pr[j]) / (sd[i] * sd[j]);
            a[(size_t)i * 256 + j] = std::fabs(r);
            load[i] += std::fabs(r);
        }
    bool in[256];
    for (int i = 0; i < 256; ++i) in[i] = true;
    for (int step = 0; step < 128; ++step) {
        int worst = -1;
        for (int i = 0; i < 256; ++i)
            if (in[i] && (worst < 0 || load[i] >= load[worst])) worst = i;  // (ties: the higher bit goes)
        in[worst] = false;
        for (int j = 0; j < 256; ++j) load[j] -= a[(size_t)worst * 256 + j];
    }
    int k = 0;
    for (int i = 0; i < 256; ++i)
        if (in[i]) perm[k++] = (uint8_t)i;
    for (int i = 0; i < 256; ++i)
        if (!in[i]) perm[k++] = (uint8_t)i;
}

}  // namespace hvd
