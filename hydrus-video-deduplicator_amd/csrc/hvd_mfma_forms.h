// hvd_mfma_forms.h -- the matrix-core forms of the all-pairs Hamming pass (k_hamming_mfma.hip) and their tile geometry: the ONE
// list of forms, and the one column-chunk rule. No HIP in here: any host C++17 compiler takes it (tests/native/
// mfma_geometry.cpp builds it alone), and so does the device pass of the kernel files.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hvd {

// The ids are the ABI's variant numbers (include/hvd_mi355x.h) and never change.
enum : int {
    kFormFull = 8,       // 256 bits at once (the reference form)
    kFormFetch = 9,      // 128-bit first stage, survivors fetch their other half (uniform data)
    kFormRegister = 12,  // 128-bit first stage, second stage out of registers (4 tiles; dense data)
    kFormAuto = 13,      // fetch, pair queue or register cascade, chosen per launch by the probe: launches with the fetch form's geometry
    kFormQueue = 18,     // 128-bit first stage, survivors through the panel-mark queue (frame hashes)
};

// One row per launchable form: k_allpairs_mfma<TILES, NBR, S1, RECT, QUEUE>. The order is the order of first instantiation.
struct MfmaForm {
    int id, tiles, nbr, s1;
    bool queue;
};
constexpr MfmaForm kMfmaForms[] = {
    {kFormFull, 8, 4, 4, false},
    {kFormFetch, 8, 2, 2, false},
    {kFormRegister, 4, 4, 2, false},
    {kFormQueue, 8, 2, 2, true},
};
constexpr int kMfmaFormCount = (int)(sizeof(kMfmaForms) / sizeof(kMfmaForms[0]));
constexpr int kMfmaWaves = 4;  // waves of a workgroup, 32 rows x TILES each

// the table's row of a launchable form, the fetch form's for the auto variant; nullptr: not a variant of this pass
constexpr const MfmaForm* mfma_form(int variant) {
    if (variant == kFormAuto) variant = kFormFetch;
    for (int k = 0; k < kMfmaFormCount; ++k)
        if (kMfmaForms[k].id == variant) return &kMfmaForms[k];
    return nullptr;
}
constexpr bool mfma_variant_known(int variant) { return mfma_form(variant) != nullptr; }
constexpr uint32_t mfma_rows_per_wg(const MfmaForm& f) { return 32u * (uint32_t)f.tiles * (uint32_t)kMfmaWaves; }
// 128-bit first stage: needs 128 - 2 * max_dist > 0
constexpr bool mfma_two_stage(int variant) { return mfma_variant_known(variant) && mfma_form(variant)->s1 == 2; }
// The auto variant chooses between the fetch form (few survivors), the register form (many) and a middle form for data with
// common false survivors: another two-stage form (the three share one hit context, whose only form-dependent field is S1), or 0 = none.
constexpr bool mfma_auto_mid_ok(int v) {
    return v == 0 || (mfma_two_stage(v) && v != kFormAuto && v != kFormFetch && v != kFormRegister);
}
constexpr uint32_t kFormAutoMidDefault = kFormQueue;
static_assert(mfma_auto_mid_ok(kFormAutoMidDefault) && !mfma_auto_mid_ok(kFormFull), "auto variant's middle form");

constexpr uint32_t kSuperPanel = 128;  // candidates per LDS super-panel: column chunks are multiples of it (kSuper of the kernel)
constexpr uint32_t kMaxGridY = 65535;

// Rows of an FP4 image: n padded to whole 1024-row tiles, at least one. In 64 bits, so that the geometry is defined for every
// n < 2^32; the 32-bit value is what the kernels take (an image of more than 2^32 - 1024 rows does not exist).
constexpr uint64_t fp4_rows_padded64(uint64_t n) { return ((n ? n : 1u) + 1023u) / 1024u * 1024u; }
inline uint32_t fp4_rows_padded(uint32_t n) { return (uint32_t)fp4_rows_padded64(n); }

// Column chunk of a pass over n_pad columns whose rows make row_blocks workgroup rows: about target_tiles tiles in all, a
// chunk of 256 .. cap columns in whole super-panels -- and never more than 65535 chunks (grid.y).
// The self pass: (8192, "mfma_col_chunk_max" -- or kSelfCapBehindIndex, below); the rectangle: (4096, 4096), enough tiles to fill the chip even when nq is small.
constexpr uint32_t mfma_col_chunk(uint64_t n_pad, uint64_t row_blocks, uint32_t target_tiles, uint32_t cap) {
    if (row_blocks < 1) row_blocks = 1;
    const uint64_t want_cb = (target_tiles + row_blocks - 1) / row_blocks;  // (>= 1)
    uint64_t chunk = (n_pad + want_cb - 1) / want_cb;
    if (chunk < 256) chunk = 256;
    if (chunk > cap) chunk = cap;
    chunk = (chunk + kSuperPanel - 1) / kSuperPanel * kSuperPanel;
    if ((n_pad + chunk - 1) / chunk > kMaxGridY) chunk = ((n_pad + kMaxGridY - 1) / kMaxGridY + kSuperPanel - 1) / kSuperPanel * kSuperPanel;
    return (uint32_t)chunk;
}
constexpr uint32_t kSelfTargetTiles = 8192, kRectTargetTiles = 4096, kRectColChunkMax = 4096;
// The self cap of the auto variant's three launches BEHIND AN INDEX LAUNCH (k_hamming_mfma.hip: launch_auto). Such a pass almost
// always runs on the index, and its matrix-core launches are grids of workgroups that return at once: at 1 M hashes 977 x 16,
// 977 x 16 and 1954 x 16 of them instead of 977 x 123 twice and 1954 x 123 (19 us per pass instead of 108; at 10 M hashes
// 1.3 ms instead of 10.0). Up to ~262 000 hashes the target-tiles rule yields chunks of at most 8192 and nothing differs from the knob's
// default. The cap is what a pass that DOES fall back may pay for long tiles and a coarser cut of the triangle
// (profiles/r21_index_fallback_time.jsonl: 1 M hashes, 5 % of them in one bucket, against the knob's 8192): no cap (chunks
// of 111 232) +6.0 %, 65536 +2.4 %, 32768 +0.0 % -- the coarsest within 3 % plus the spread of the parent's own rounds.
constexpr uint32_t kSelfCapBehindIndex = 65536;

// Geometry of one pass: rows = the nq queries of a rectangle, the n hashes themselves of a self pass; columns = the n hashes.
struct MfmaGeometry {
    uint32_t rows_per_wg, col_chunk;
    uint64_t row_blocks, col_blocks;  // grid.x, and grid.y of a lone rank
};
constexpr MfmaGeometry mfma_geometry(const MfmaForm& f, uint64_t nrows, uint64_t n_pad, bool rect, uint32_t self_cap) {
    const uint32_t rows = mfma_rows_per_wg(f);
    const uint64_t n_rb = (nrows + rows - 1) / rows;
    // (the self pass sizes its chunk by the padded rows: the value hvd_allpairs_tile_geometry hands to the callers that tile by it)
    const uint32_t chunk = rect ? mfma_col_chunk(n_pad, n_rb, kRectTargetTiles, kRectColChunkMax)
                                : mfma_col_chunk(n_pad, (n_pad + rows - 1) / rows, kSelfTargetTiles, self_cap);
    return {rows, chunk, n_rb, (n_pad + chunk - 1) / chunk};
}

}  // namespace hvd
