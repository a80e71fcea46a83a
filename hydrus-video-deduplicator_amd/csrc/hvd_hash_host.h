// hvd_hash_host.h -- what a frame-hashing call is, for every door that leads to the PDQ kernels: the host-buffer entries
// (hvd_search.cpp), the device-resident entries (hvd_api.cpp) and the streaming hasher (hvd_stream.cpp). One definition each of
// the frame geometry a call accepts, of the argument checks that recur, of the scratch layout of the plain and rectangle forms
// (the crop ladder has CropsScratch, k_crops.hip) and of the hvd::api_* helpers hvd_api.cpp lends the hasher. Does not see Ctx.
#pragma once
#include "hvd_kernels.h"

namespace hvd {

// hvd_api.cpp
int api_fail(int code, const char* fmt, ...);  // sets the thread's error text, returns code
const float* api_dct_device();                 // nullptr before hvd_init
int api_bind_device();                         // hipSetDevice(bound device) for the calling thread
int api_context();                             // the calling thread's current context of the device group
void api_set_context(int idx);
// Enqueue the PDQ kernels for n > 0 frames on stream s (geometry validated): front-end by geometry, then K1 or, dihedral, the
// 8-hash kernel (k_pdq_dihedral.hip, d_hashes n*8*32 bytes). d_scratch: HashScratch(n, h, w, channels, false).
hipError_t api_launch_hash(const void* d_frames, int64_t n, int h, int w, int channels, void* d_scratch, void* d_hashes,
                           void* d_quality, hipStream_t s, bool dihedral);
// The launch chain of hvd_dev_pdq_hash_frames_rects: frame -> rectangle table, down-sampler inside the rectangles, K1.
// d_scratch: HashScratch(n, h, w, channels, true), 16-byte aligned.
hipError_t api_launch_hash_rects(const void* d_frames, int64_t n, int h, int w, int channels, const void* d_offsets, int64_t V,
                                 const void* d_rects, void* d_scratch, void* d_hashes, void* d_quality, hipStream_t s);
// hvd_dev_content_rects, _color and _detail: every check of theirs, then launch_content_rects on the library stream. d_colors:
// the Color kind's int32[V], nullptr for the others.
int api_content_rects(const RectRule& rule, const void* d_colors, const void* d_frames, int64_t n, int h, int w, int channels,
                      const void* d_offsets, int64_t V, void* d_rects);

/* ---- the frame geometry of a hashing call ---- */
constexpr int kMinSide = 64, kMaxSide = 4096;
inline bool sides_ok(int h, int w) { return h >= kMinSide && w >= kMinSide && h <= kMaxSide && w <= kMaxSide; }
inline bool channels_ok(int channels) { return channels == 1 || channels == 3; }
inline bool geometry_ok(int h, int w, int channels) { return sides_ok(h, w) && channels_ok(channels); }
// 64x64 gray frames are the hash kernel's input as they are; every other geometry goes through 64x64 float planes in scratch
inline bool needs_scratch(int h, int w, int channels) { return !(h == 64 && w == 64 && channels == 1); }
inline bool rect_is_full_frame(const int32_t r[4], int h, int w) { return r[0] == 0 && r[1] == 0 && r[2] == h && r[3] == w; }

/* ---- argument checks that recur: HVD_OK, or the code with the one message ---- */
inline int check_geometry(int h, int w, int channels) {
    if (geometry_ok(h, w, channels)) return HVD_OK;
    return api_fail(HVD_ERR_ARG, "bad frame geometry h=%d w=%d channels=%d (need h,w in [64,4096], channels 1 or 3)", h, w, channels);
}
// a content-rectangle rule (hvd_kernels.h: RectRule), under the names its kind's entries give the level and the count
inline int check_rect_rule(const RectRule& rule, bool with_count = true) {
    static const char* const names[3][2] = {{"black_level", "min_bright"}, {"bar_level", "min_bright"}, {"detail_level", "min_detail"}};
    const char* const* name = names[(int)rule.kind];
    if (rule.level < 0 || rule.level > 254) return api_fail(HVD_ERR_ARG, "%s=%d: need 0..254", name[0], rule.level);
    return !with_count || rule.count >= 1 ? HVD_OK : api_fail(HVD_ERR_ARG, "%s=%d: need >= 1", name[1], rule.count);
}
// hvd_dev_bar_colors: the colour rule's level alone
inline int check_bar_level(int bar_level) { return check_rect_rule({RectKind::Color, bar_level, 0}, false); }
inline int check_dihedral_dct(bool dihedral) {  // the dihedral kernel has K1's strict arithmetic only
    if (!dihedral || g_pdq_dct_mode == 0) return HVD_OK;
    return api_fail(HVD_ERR_STATE, "dihedral hashing has no fma DCT mode: call hvd_set_pdq_dct_mode(0) first");
}

/* ---- scratch of the plain and the rectangle form ---- */
// Byte offsets in the scratch of a call of n frames: 64x64 float planes | the down-sampler's workspace for min(n, 1024) frames
// (none at 64x64) | with_rect_table: the frame -> rectangle table (int4 per frame) at the next multiple of 16 (none at 64x64:
// every rectangle is the full frame there). Read by the size queries and by the launch chains alike.
struct HashScratch {
    size_t planes = 0, ws = 0, table = 0, total = 0;
    HashScratch(int64_t n, int h, int w, int channels, bool with_rect_table) {
        if (!needs_scratch(h, w, channels)) return;
        const bool down = !(h == 64 && w == 64);
        ws = sizeof(float) * 4096 * (size_t)n;
        table = total = ws + (down ? sizeof(float) * (size_t)(n < 1024 ? n : 1024) * pdq_downsample_ws_floats(h, w) : 0);
        if (with_rect_table && down) {
            table = (table + 15) / 16 * 16;
            total = table + pdq_rects_geom_bytes(n);
        }
    }
};

}  // namespace hvd
