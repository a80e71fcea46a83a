// Prints the tile geometry of the matrix-core all-pairs pass as csrc/hvd_mfma_forms.h computes it, for
// tests/test_mfma_geometry.py. The header needs no HIP, so this builds with any host compiler: the test builds it with
// g++ -fsanitize=address,undefined and runs it as a program of its own.
// stdin: one case per line, "form nq nt rect cap" (a self pass: rect 0, nq ignored; cap = the "mfma_col_chunk_max" knob, which
// the rectangle ignores). stdout: "rows_per_workgroup col_chunk grid_y" per case, grid_y of a lone rank; "unknown" for a form
// that is none.
#include <cinttypes>
#include <cstdio>

#include "../../hydrus-video-deduplicator_amd/csrc/hvd_mfma_forms.h"

int main() {
    int form, rect;
    uint64_t nq, nt;
    uint32_t cap;
    while (scanf("%d %" SCNu64 " %" SCNu64 " %d %" SCNu32, &form, &nq, &nt, &rect, &cap) == 5) {
        const hvd::MfmaForm* f = hvd::mfma_form(form);
        if (!f || nt >= (1ull << 32) || nq >= (1ull << 32)) {
            puts("unknown");
            continue;
        }
        const hvd::MfmaGeometry geo = hvd::mfma_geometry(*f, rect ? nq : nt, hvd::fp4_rows_padded64(nt), rect != 0, cap);
        printf("%" PRIu32 " %" PRIu32 " %" PRIu64 "\n", geo.rows_per_wg, geo.col_chunk, geo.col_blocks);
    }
    return 0;
}
