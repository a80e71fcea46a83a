// Prints the self-pass tile geometry of the auto variant's launches behind an index launch -- csrc/hvd_mfma_forms.h:
// mfma_geometry with the cap kSelfCapBehindIndex -- next to the geometry of every other self pass (the cap of the
// "mfma_col_chunk_max" knob), for tests/test_mfma_geometry_behind_index.py. No HIP: the test builds it with
// g++ -fsanitize=address,undefined and runs it as a program of its own.
// stdin: one case per line, "form n knob_cap". stdout: first "kSelfCapBehindIndex kSelfTargetTiles", then per case
// "rows_per_workgroup row_blocks  chunk grid_y  chunk_behind_index grid_y_behind_index"; "unknown" for a form that is none.
#include <cinttypes>
#include <cstdio>

#include "../../hydrus-video-deduplicator_amd/csrc/hvd_mfma_forms.h"

int main() {
    int form;
    uint64_t n;
    uint32_t cap;
    printf("%" PRIu32 " %" PRIu32 "\n", hvd::kSelfCapBehindIndex, hvd::kSelfTargetTiles);
    while (scanf("%d %" SCNu64 " %" SCNu32, &form, &n, &cap) == 3) {
        const hvd::MfmaForm* f = hvd::mfma_form(form);
        if (!f || n >= (1ull << 32)) {
            puts("unknown");
            continue;
        }
        const uint64_t n_pad = hvd::fp4_rows_padded64(n);
        const hvd::MfmaGeometry knob = hvd::mfma_geometry(*f, n, n_pad, false, cap);
        const hvd::MfmaGeometry idx = hvd::mfma_geometry(*f, n, n_pad, false, hvd::kSelfCapBehindIndex);
        const uint64_t row_blocks = (n_pad + knob.rows_per_wg - 1) / knob.rows_per_wg;  // the rows the chunk rule counts
        printf("%" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu64 "\n", knob.rows_per_wg, row_blocks, knob.col_chunk,
               knob.col_blocks, idx.col_chunk, idx.col_blocks);
    }
    return 0;
}
