// hvd_search.cpp -- the host-buffer entry points of the C-ABI (what the vpdq-shaped shim binds: hash frames, one pair, all pairs,
// video-level search; each fans out over the device group by itself) and the video-level search on the device (K3: key set,
// agreement step, key exchange, fold, emit). Split out of hvd_api.cpp in round 6; shared state: hvd_internal.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "hvd_bit_order.h"
#include "hvd_hash_host.h"
#include "hvd_internal.h"
#include "../../include/hvd_mi355x_bench.h"

using namespace hvdi;

namespace {
constexpr unsigned long long kMatchServerIdleUs = 300;   // the server leaves after this long without a call ...
constexpr unsigned long long kMatchServerLifeUs = 2000;  // ... and after this long in any case (another thread's hipFree / device-wide wait gets its turn)

// fn(rank, result) on every context of the group (run_on_group: one host thread each); the call's result is rank 0's
template <class R, class Fn>
int run_keep_rank0(R& res, const Fn& fn) {
    return run_on_group([&](int r) -> int {
        R mine{};
        if (int rc = fn(r, mine)) return rc;
        if (r == 0) res = std::move(mine);
        return HVD_OK;
    });
}

// the records of a host-buffer entry point, sorted, to out[cap]; *out_count = their true number (total)
template <class T>
int copy_out(std::vector<T>& recs, int64_t total, bool (*less)(const T&, const T&), T* out, int64_t cap, int64_t* out_count,
             const char* what) {
    *out_count = total;
    if (total > cap)
        return fail(HVD_ERR_OVERFLOW, "%s buffer too small: need %lld records, cap %lld", what, (long long)total, (long long)cap);
    std::sort(recs.begin(), recs.end(), less);
    if (!recs.empty()) memcpy(out, recs.data(), sizeof(T) * recs.size());
    return HVD_OK;
}
}  // namespace

extern "C" {

// Frames one batch of a host-buffer hashing entry stages on the device: <= ~1 GiB of them (hvd_debug_set "hash_staging_bytes"
// lowers the limit so that tests reach the multi-batch paths at small shapes), at least one.
static int64_t staging_frames(size_t frame_bytes) {
    const size_t limit = g_hash_staging_bytes ? (size_t)g_hash_staging_bytes : (size_t)1 << 30;
    return std::max<int64_t>(1, (int64_t)(limit / frame_bytes));
}

// One per-frame output of a host-buffer hashing entry: `bytes` per frame, from a pool slot of its own to `host` (NULL: not wanted)
struct FrameOut {
    void* host;
    Ctx::Scr slot;
    size_t bytes;
};

// The batch loop of the host-buffer hashing entries (arguments validated, n > 0): stage at most staging_frames() frames, size
// the pool for that batch once, then per batch upload, enqueue(d_in, m, d_scratch, d_out[]) -- the device entry; d_out[k] is
// outs[k]'s buffer --, download every output and synchronise. scratch_bytes(batch) = 0: the entry needs no scratch (NULL).
static int hash_in_batches(const uint8_t* frames, int64_t n, size_t frame_bytes, const std::function<size_t(int64_t)>& scratch_bytes,
                           std::initializer_list<FrameOut> outs,
                           const std::function<int(const void*, int64_t, void*, void* const*)>& enqueue) {
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    const int64_t batch = std::min(n, staging_frames(frame_bytes));
    void *d_in = nullptr, *d_scr = nullptr, *d_out[4] = {};
    SCR(S_FRAMES, frame_bytes * batch, d_in);
    if (const size_t sb = scratch_bytes(batch)) SCR(S_FSCR, sb, d_scr);
    const FrameOut* out = outs.begin();
    for (size_t k = 0; k < outs.size(); ++k)
        if (int rc = scratch(out[k].slot, out[k].bytes * (size_t)batch, &d_out[k])) return rc;
    for (int64_t f0 = 0; f0 < n; f0 += batch) {
        const int64_t m = std::min(batch, n - f0);
        HIP_TRY(hipMemcpyAsync(d_in, frames + frame_bytes * f0, frame_bytes * m, hipMemcpyHostToDevice, g.stream));
        if (int rc = enqueue(d_in, m, d_scr, d_out)) return rc;
        for (size_t k = 0; k < outs.size(); ++k)
            if (out[k].host)
                HIP_TRY(hipMemcpyAsync((char*)out[k].host + out[k].bytes * f0, d_out[k], out[k].bytes * (size_t)m, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    return HVD_OK;
}

// variants: 1 (the PDQ hash) or 8 (the dihedral hashes, hvd_dev_pdq_hash_frames_dihedral): hash bytes per frame 32 * variants
static int hash_frames_host(const uint8_t* frames, int64_t n, int h, int w, int channels, uint8_t* out_hashes,
                            int32_t* out_quality, int variants = 1) {
    if (int rc = need_ready()) return rc;
    // the whole geometry is checked before anything is sized or allocated for it: an oversized frame is HVD_ERR_ARG,
    // never a failed allocation (HVD_ERR_HIP) of its staging or scratch
    if (n < 0) return fail(HVD_ERR_ARG, "bad frame count n=%lld", (long long)n);
    if (int rc = hvd::check_geometry(h, w, channels)) return rc;
    if (int rc = hvd::check_dihedral_dct(variants != 1)) return rc;
    if (n == 0) return HVD_OK;
    if (!frames || !out_hashes || !out_quality) return fail(HVD_ERR_ARG, "NULL buffer");
    return hash_in_batches(
        frames, n, (size_t)h * w * channels, [&](int64_t batch) { return hvd::HashScratch(batch, h, w, channels, false).total; },
        {{out_hashes, Ctx::S_HASH, 32 * (size_t)variants}, {out_quality, Ctx::S_QUAL, 4}},
        [&](const void* d_in, int64_t m, void* d_scr, void* const* d_out) {
            return (variants == 1 ? hvd_dev_pdq_hash_frames : hvd_dev_pdq_hash_frames_dihedral)(d_in, m, h, w, channels, d_scr,
                                                                                                 d_out[0], d_out[1]);
        });
}

// frames are independent: a group hashes contiguous ranges of them, one per context, no exchange
static int hash_frames_group(const uint8_t* frames, int64_t n, int h, int w, int channels, uint8_t* out_hashes,
                             int32_t* out_quality, int variants = 1) {
    const int W = g_nctx;
    if (W <= 1 || n < 4 * (int64_t)W || !frames || !out_hashes || !out_quality || !hvd::geometry_ok(h, w, channels))
        return hash_frames_host(frames, n, h, w, channels, out_hashes, out_quality, variants);
    const size_t frame_bytes = (size_t)h * w * channels;
    return run_on_group([&](int r) -> int {
        const int64_t per = (n + W - 1) / W, lo = std::min<int64_t>(n, per * r), hi = std::min<int64_t>(n, lo + per);
        return hash_frames_host(frames + frame_bytes * (size_t)lo, hi - lo, h, w, channels, out_hashes + 32 * variants * lo,
                                out_quality + lo, variants);
    });
}

int hvd_pdq_hash_frames_gray_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes,
                                int32_t* out_quality) {
    return hash_frames_group(frames, n, h, w, 1, out_hashes, out_quality);
}

int hvd_pdq_hash_frames_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes,
                                 int32_t* out_quality) {
    return hash_frames_group(frames, n, h, w, 3, out_hashes, out_quality);
}

int hvd_pdq_hash_frames_dihedral_gray_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes8,
                                         int32_t* out_quality) {
    return hash_frames_group(frames, n, h, w, 1, out_hashes8, out_quality, 8);
}

int hvd_pdq_hash_frames_dihedral_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes8,
                                          int32_t* out_quality) {
    return hash_frames_group(frames, n, h, w, 3, out_hashes8, out_quality, 8);
}

// Crop-ladder hashing of host frames. Runs on the calling thread's current context, also under a device group;
// batches as hash_frames_host. The list is checked by the device entry before it asks for a device, so a bad list is
// HVD_ERR_ARG here too, whatever the state.
static int hash_frames_crops_host(const uint8_t* frames, int64_t n, int h, int w, int channels, const int32_t* crops, int K,
                                  uint8_t* out_hashes8, int32_t* out_quality, int32_t* out_crop_quality) {
    if (int rc = hvd_dev_pdq_hash_frames_crops(nullptr, 0, h, w, channels, crops, K, nullptr, nullptr, nullptr, nullptr)) return rc;
    if (n < 0 || n >= (1ll << 31)) return fail(HVD_ERR_ARG, "bad frame count n=%lld", (long long)n);
    if (n == 0) return HVD_OK;
    if (!frames || !out_hashes8 || !out_quality) return fail(HVD_ERR_ARG, "NULL buffer");
    return hash_in_batches(
        frames, n, (size_t)h * w * channels, [&](int64_t batch) { return hvd::pdq_crops_scratch_bytes(batch, h, w, K); },
        {{out_hashes8, Ctx::S_HASH, 256}, {out_quality, Ctx::S_QUAL, 4}, {out_crop_quality, Ctx::S_CQUAL, 32}},
        [&](const void* d_in, int64_t m, void* d_scr, void* const* d_out) {
            return hvd_dev_pdq_hash_frames_crops(d_in, m, h, w, channels, crops, K, d_scr, d_out[0], d_out[1], d_out[2]);
        });
}

int hvd_pdq_hash_frames_crops_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int32_t* crops, int K,
                                      uint8_t* out_hashes8, int32_t* out_quality, int32_t* out_crop_quality) {
    return hash_frames_crops_host(frames, n, h, w, 1, crops, K, out_hashes8, out_quality, out_crop_quality);
}

int hvd_pdq_hash_frames_crops_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int32_t* crops, int K,
                                       uint8_t* out_hashes8, int32_t* out_quality, int32_t* out_crop_quality) {
    return hash_frames_crops_host(frames, n, h, w, 3, crops, K, out_hashes8, out_quality, out_crop_quality);
}

// The batches of the autocrop entry end on video boundaries: from video v0, the end v1 > v0 of the largest run of whole videos
// of at most `limit` frames (a video of its own is always taken: the caller has checked that each fits).
static int64_t videos_that_fit(const int64_t* offsets, int64_t V, int64_t v0, int64_t limit) {
    int64_t v1 = v0 + 1;
    while (v1 < V && offsets[v1 + 1] - offsets[v0] <= limit) ++v1;
    return v1;
}

// Content-rectangle hashing of host frames. Runs on the calling thread's current context, also under a device
// group. Batches end on video boundaries, so a video's rectangle always sees all of its frames.
// bar: with the colour rule -- every batch's colours are the caller's (bar->colors) or found from the batch's
// corners, and the colours used go to bar->out_colors.
struct BarColors {
    const int32_t* colors;  // int32[V] packed, or nullptr: automatic
    int32_t* out_colors;    // int32[V]
};
static int hash_frames_autocrop_host(const uint8_t* frames, int64_t n, int h, int w, int channels, const int64_t* offsets,
                                     int64_t V, const hvd::RectRule& rule, uint8_t* out_hashes, int32_t* out_quality,
                                     int32_t* out_rects, const BarColors* bar = nullptr) {
    if (int rc = need_ready()) return rc;
    if (int rc = hvd::check_geometry(h, w, channels)) return rc;
    if (n < 0 || V < 0 || V >= (1ll << 31) || n >= (1ll << 31)) return fail(HVD_ERR_ARG, "bad counts n=%lld V=%lld", (long long)n, (long long)V);
    if (int rc = hvd::check_rect_rule(rule)) return rc;
    if (V == 0 && n == 0) return HVD_OK;
    if (!offsets) return fail(HVD_ERR_ARG, "NULL offsets");
    if (offsets[0] != 0 || offsets[V] != n) return fail(HVD_ERR_ARG, "offsets must run from 0 to n=%lld", (long long)n);
    for (int64_t v = 0; v < V; ++v)
        if (offsets[v + 1] < offsets[v]) return fail(HVD_ERR_ARG, "offsets decrease at video %lld", (long long)v);
    if (!out_rects || (n > 0 && (!frames || !out_hashes || !out_quality))) return fail(HVD_ERR_ARG, "NULL buffer");
    if (bar && !bar->out_colors) return fail(HVD_ERR_ARG, "NULL buffer");
    if (bar && bar->colors)
        for (int64_t v = 0; v < V; ++v)
            if (bar->colors[v] < 0 || bar->colors[v] > 0xFFFFFF || (channels == 1 && bar->colors[v] > 0xFF))
                return fail(HVD_ERR_ARG, "colour of video %lld is 0x%x: need c0 | c1 << 8 | c2 << 16 (gray: c0 alone)", (long long)v,
                            (unsigned)bar->colors[v]);
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    const size_t frame_bytes = (size_t)h * w * channels;
    const int64_t limit = staging_frames(frame_bytes);
    for (int64_t v = 0; v < V; ++v)
        if (offsets[v + 1] - offsets[v] > limit)
            return fail(HVD_ERR_ARG, "video %lld has %lld frames, more than the %lld that fit the staging limit of %lld bytes at this "
                        "geometry: a video's rectangle needs all of its frames in one batch", (long long)v,
                        (long long)(offsets[v + 1] - offsets[v]), (long long)limit, (long long)(limit * frame_bytes));
    int64_t batch = 0, batch_v = 0;  // the largest batch of whole videos: sizes the pool once
    for (int64_t v0 = 0, v1; v0 < V; v0 = v1) {
        v1 = videos_that_fit(offsets, V, v0, limit);
        batch = std::max<int64_t>(batch, offsets[v1] - offsets[v0]);
        batch_v = std::max<int64_t>(batch_v, v1 - v0);
    }
    void *d_in = nullptr, *d_scr = nullptr, *d_h = nullptr, *d_q = nullptr, *d_off = nullptr, *d_rects = nullptr;
    void *d_colors = nullptr, *d_acc = nullptr;
    if (batch > 0) {
        SCR(S_FRAMES, frame_bytes * batch, d_in);
        if (const size_t sb = hvd::HashScratch(batch, h, w, channels, true).total) SCR(S_FSCR, sb, d_scr);
        SCR(S_HASH, 32 * (size_t)batch, d_h);
        SCR(S_QUAL, 4 * (size_t)batch, d_q);
    }
    SCR(S_OFF, 8 * (size_t)(batch_v + 1), d_off);
    SCR(S_RECTS, 16 * (size_t)batch_v, d_rects);
    if (bar) SCR(S_COLORS, 4 * (size_t)batch_v, d_colors);
    if (bar && !bar->colors) SCR(S_CACC, hvd::bar_colors_scratch_bytes((uint32_t)batch_v), d_acc);
    std::vector<int64_t> local;
    for (int64_t v0 = 0, v1; v0 < V; v0 = v1) {
        v1 = videos_that_fit(offsets, V, v0, limit);
        const int64_t f0 = offsets[v0], m = offsets[v1] - f0, mv = v1 - v0;
        local.assign(offsets + v0, offsets + v1 + 1);
        for (auto& o : local) o -= f0;
        int32_t* rects = out_rects + 4 * v0;
        HIP_TRY(hipMemcpyAsync(d_off, local.data(), 8 * (size_t)(mv + 1), hipMemcpyHostToDevice, g.stream));
        if (m > 0) HIP_TRY(hipMemcpyAsync(d_in, frames + frame_bytes * f0, frame_bytes * m, hipMemcpyHostToDevice, g.stream));
        if (bar && bar->colors) {
            HIP_TRY(hipMemcpyAsync(d_colors, bar->colors + v0, 4 * (size_t)mv, hipMemcpyHostToDevice, g.stream));
        } else if (bar) {
            if (int rc = hvd_dev_bar_colors(d_in, m, h, w, channels, d_off, mv, rule.level, d_acc, d_colors)) return rc;
        }
        if (int rc = hvd::api_content_rects(rule, d_colors, d_in, m, h, w, channels, d_off, mv, d_rects)) return rc;
        if (bar) HIP_TRY(hipMemcpyAsync(bar->out_colors + v0, d_colors, 4 * (size_t)mv, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(rects, d_rects, 16 * (size_t)mv, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (m == 0) continue;
        // every rectangle full: today's path (fused 512x512 kernels included); both are the oracle's bits
        bool full = true;
        for (int64_t v = 0; v < mv && full; ++v) full = hvd::rect_is_full_frame(rects + 4 * v, h, w);
        if (int rc = full ? hvd_dev_pdq_hash_frames(d_in, m, h, w, channels, d_scr, d_h, d_q)
                          : hvd_dev_pdq_hash_frames_rects(d_in, m, h, w, channels, d_off, mv, d_rects, d_scr, d_h, d_q))
            return rc;
        HIP_TRY(hipMemcpyAsync(out_hashes + 32 * f0, d_h, 32 * (size_t)m, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(out_quality + f0, d_q, 4 * (size_t)m, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    return HVD_OK;
}

int hvd_pdq_hash_frames_autocrop_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                         int black_level, int min_bright, uint8_t* out_hashes, int32_t* out_quality,
                                         int32_t* out_rects) {
    return hash_frames_autocrop_host(frames, n, h, w, 1, offsets, V, {hvd::RectKind::Black, black_level, min_bright}, out_hashes, out_quality, out_rects);
}

int hvd_pdq_hash_frames_autocrop_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                          int black_level, int min_bright, uint8_t* out_hashes, int32_t* out_quality,
                                          int32_t* out_rects) {
    return hash_frames_autocrop_host(frames, n, h, w, 3, offsets, V, {hvd::RectKind::Black, black_level, min_bright}, out_hashes, out_quality, out_rects);
}

int hvd_pdq_hash_frames_barcolor_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                         const int32_t* colors, int bar_level, int min_bright, uint8_t* out_hashes,
                                         int32_t* out_quality, int32_t* out_rects, int32_t* out_colors) {
    const BarColors bar{colors, out_colors};
    return hash_frames_autocrop_host(frames, n, h, w, 1, offsets, V, {hvd::RectKind::Color, bar_level, min_bright}, out_hashes, out_quality, out_rects, &bar);
}

int hvd_pdq_hash_frames_barcolor_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                          const int32_t* colors, int bar_level, int min_bright, uint8_t* out_hashes,
                                          int32_t* out_quality, int32_t* out_rects, int32_t* out_colors) {
    const BarColors bar{colors, out_colors};
    return hash_frames_autocrop_host(frames, n, h, w, 3, offsets, V, {hvd::RectKind::Color, bar_level, min_bright}, out_hashes, out_quality, out_rects, &bar);
}

int hvd_pdq_hash_frames_detail_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                       int detail_level, int min_detail, uint8_t* out_hashes, int32_t* out_quality,
                                       int32_t* out_rects) {
    return hash_frames_autocrop_host(frames, n, h, w, 1, offsets, V, {hvd::RectKind::Detail, detail_level, min_detail}, out_hashes, out_quality, out_rects);
}

int hvd_pdq_hash_frames_detail_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                        int detail_level, int min_detail, uint8_t* out_hashes, int32_t* out_quality,
                                        int32_t* out_rects) {
    return hash_frames_autocrop_host(frames, n, h, w, 3, offsets, V, {hvd::RectKind::Detail, detail_level, min_detail}, out_hashes, out_quality, out_rects);
}

// Runs the default all-pairs kernel (FP4-MFMA form) on a host DB -- this context's share of the tiles (rank of world) --
// and fetches up to `cap` unordered records: its own when world == 1, every rank's after the group's exchange otherwise
// (agreement step on the true counts, then the records: RCCL between the devices, or host memory where the group has no RCCL).
// *out_count = the true number of records over all ranks. Device buffers come from the grow-only pool (caller holds h_mu).
static int allpairs_host_raw(const uint8_t* db, int64_t n, const int32_t* group, int max_dist,
                             std::vector<hvd_pair>& recs, int64_t cap, int64_t* out_count, int rank = 0, int world = 1) {
    void* d_pairs = nullptr;
    unsigned long long cnt = 0;
    // Everything up to the exchange runs inside `local`: at world > 1 its result code goes into the agreement step with the
    // count, so that a rank that fails on its own does not leave the others waiting in the exchange (as in vmatch_build).
    auto local = [&]() -> int {
        void *d_db = nullptr, *d_img = nullptr, *d_grp = nullptr;
        unsigned long long* d_cnt = nullptr;
        SCR(S_DB, 32 * (size_t)n, d_db);
        HIP_TRY(hipMemcpyAsync(d_db, db, 32 * (size_t)n, hipMemcpyHostToDevice, g.stream));
        size_t img_bytes = 0;
        if (int rc = hvd_fp4_image_bytes(n, &img_bytes)) return rc;
        SCR(S_IMG, img_bytes, d_img);
        if (int rc = hvd_dev_expand_fp4(d_db, n, d_img)) return rc;
        if (group) {
            SCR(S_GRP, 4 * (size_t)n, d_grp);
            HIP_TRY(hipMemcpyAsync(d_grp, group, 4 * (size_t)n, hipMemcpyHostToDevice, g.stream));
        }
        SCR(S_PAIRS, sizeof(hvd_pair) * (size_t)cap, d_pairs);
        SCR(S_COUNTERS, 64, d_cnt);
        HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, g.stream));
        if (int rc = hvd_dev_allpairs_hamming256_mfma(d_db, d_img, n, group ? d_grp : nullptr, max_dist, rank, world, d_pairs,
                                                      cap, d_cnt, HVD_DEFAULT_VARIANT))
            return rc;
        HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        return HVD_OK;
    };
    const int local_rc = local();
    const size_t mine = (size_t)std::min<unsigned long long>(cnt, (unsigned long long)cap);
    if (world == 1) {
        if (local_rc) return local_rc;
        *out_count = (int64_t)cnt;
        recs.resize(mine);
        if (mine) {
            HIP_TRY(hipMemcpyAsync(recs.data(), d_pairs, sizeof(hvd_pair) * mine, hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipStreamSynchronize(g.stream));
        }
        return HVD_OK;
    }
    // the true counts first (a rank whose own buffer overflowed must not truncate the total), then the records
    std::vector<unsigned long long> counts;
    if (int rc = agree(cnt, local_rc, "all-pairs search", counts)) return rc;
    unsigned long long total = 0;
    for (unsigned long long c : counts) total += c;
    *out_count = (int64_t)total;
    if (total > (unsigned long long)cap) {  // every rank sees the same total: all of them skip the record exchange
        recs.clear();
        return HVD_OK;
    }
    recs.resize((size_t)total);
    int64_t got = 0;
    if (int rc = hvd_comm_allgather_pairs(d_pairs, (int64_t)mine, recs.data(), (int64_t)total, &got)) return rc;
    if (got != (int64_t)total) return fail(HVD_ERR_RCCL, "candidate exchange returned %lld records, expected %llu", (long long)got, total);
    return HVD_OK;
}

int hvd_allpairs_hamming256(const uint8_t* db, int64_t n, const int32_t* group, int max_dist, hvd_pair* out,
                            int64_t cap, int64_t* out_count) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || n >= (1ll << 32) || cap < 0 || !out_count || (cap > 0 && !out))
        return fail(HVD_ERR_ARG, "bad arguments n=%lld cap=%lld", (long long)n, (long long)cap);
    if (max_dist < 0 || max_dist > 256) return fail(HVD_ERR_ARG, "max_dist=%d out of range [0,256]", max_dist);
    *out_count = 0;
    if (n < 2) return HVD_OK;
    if (!db) return fail(HVD_ERR_ARG, "db is NULL");
    struct Found {
        std::vector<hvd_pair> recs;
        int64_t total = 0;
    } res;
    const int W = (g_nctx > 1 && max_dist < 128 && n >= 4096) ? g_nctx : 1;  // small DBs: one device (launch-bound anyway)
    if (W == 1) {
        std::lock_guard<std::recursive_mutex> lk(g.h_mu);
        if (int rc = allpairs_host_raw(db, n, group, max_dist, res.recs, cap, &res.total)) return rc;
    } else {
        // DB replicated on every device of the group, tile (rb, cb) -> context (rb + cb) % W, candidates exchanged
        if (int rc = run_keep_rank0(res, [&](int r, Found& mine) -> int {
                std::lock_guard<std::recursive_mutex> lk(g.h_mu);
                return allpairs_host_raw(db, n, group, max_dist, mine.recs, cap, &mine.total, r, W);
            }))
            return rc;
    }
    return copy_out(res.recs, res.total, pair_less, out, cap, out_count, "pair");
}

// Frame-level hits -> per video pair (a = video of the row frame, b = video of the column frame):
// q_hits = distinct row frames, t_hits = distinct column frames. Output sorted by (a, b).
// Only the popcount route (max_dist >= 128, never used by the reference) still reduces on the host.
static void aggregate_video_hits(const std::vector<hvd_pair>& recs, const int32_t* vid_row, const int32_t* vid_col,
                                 std::vector<hvd_vmatch>& res) {
    struct Key {
        uint32_t a, b, f;
    };
    std::vector<Key> qs(recs.size()), ts(recs.size());
    for (size_t k = 0; k < recs.size(); ++k) {
        const uint32_t va = (uint32_t)vid_row[recs[k].i], vb = (uint32_t)vid_col[recs[k].j];
        qs[k] = Key{va, vb, recs[k].i};
        ts[k] = Key{va, vb, recs[k].j};
    }
    auto less = [](const Key& x, const Key& y) {
        if (x.a != y.a) return x.a < y.a;
        if (x.b != y.b) return x.b < y.b;
        return x.f < y.f;
    };
    std::sort(qs.begin(), qs.end(), less);
    std::sort(ts.begin(), ts.end(), less);
    res.clear();
    size_t qi = 0, ti = 0;
    while (qi < qs.size()) {
        const uint32_t a = qs[qi].a, b = qs[qi].b;
        uint32_t qh = 0, th = 0;
        for (uint32_t last = 0xFFFFFFFFu; qi < qs.size() && qs[qi].a == a && qs[qi].b == b; ++qi)
            if (qs[qi].f != last) {
                last = qs[qi].f;
                ++qh;
            }
        for (uint32_t last = 0xFFFFFFFFu; ti < ts.size() && ts[ti].a == a && ts[ti].b == b; ++ti)
            if (ts[ti].f != last) {
                last = ts[ti].f;
                ++th;
            }
        res.push_back(hvd_vmatch{a, b, qh, th});
    }
}

int hvd_match_two(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb, int max_dist, int32_t* q_hits,
                  int32_t* t_hits) {
    if (int rc = need_ready()) return rc;
    if (na < 0 || nb < 0 || !q_hits || !t_hits || na >= (1ll << 31) || nb >= (1ll << 31))
        return fail(HVD_ERR_ARG, "bad arguments");
    if (max_dist < 0 || max_dist > 256) return fail(HVD_ERR_ARG, "max_dist=%d out of range [0,256]", max_dist);
    *q_hits = 0;
    *t_hits = 0;
    if (na == 0 || nb == 0) return HVD_OK;  // either side empty => no match (db/DedupeDB.py:555-557)
    if (!a || !b) return fail(HVD_ERR_ARG, "NULL hash buffer");
    // The VP-tree issues one such call per visited node (db/vptree.py:737): no malloc/free per call.
    std::lock_guard<std::mutex> lk(g.m_mu);
    const size_t small = hvd::match_two_small_limit();
    if (40 * (size_t)(na + nb) <= small) {
        // operands fit in LDS: the kernel reads them from pinned host memory and writes the counters there, then a
        // sequence word the host polls (a stream synchronisation costs more than the whole kernel)
        if (!g.m_pin) {
            HIP_TRY(hipHostMalloc((void**)&g.m_pin, small + 64, hipHostMallocCoherent));  // (fine-grained: a RUNNING kernel sees the host's stores)
            memset(g.m_pin + small, 0, 64);
        }
        uint8_t* pb = g.m_pin + 32 * (size_t)na;
        volatile int32_t* ph = reinterpret_cast<volatile int32_t*>(g.m_pin + small);
        memcpy(g.m_pin, a, 32 * (size_t)na);
        memcpy(pb, b, 32 * (size_t)nb);
        if (++g.m_seq == 0u) g.m_seq = 1u;  // (unsigned: the step past 0x7FFFFFFF and the wrap are defined; 0 is never a call's number)
        const int32_t seq = (int32_t)g.m_seq;
        if (g_match_server) {
            // Round 5: post the request to the resident match server (k_match_server) and poll for the answer -- no launch and
            // no synchronisation per call while calls come back to back (the VP-tree's pattern); the server is (re)started
            // when it has left (idle for kMatchServerIdleUs) or has never run.
            const uint32_t seq21 = (uint32_t)seq & 0x1FFFFFu;
            auto start_server = [&]() -> int {
                if (!g.m_srv_stream) HIP_TRY(hipStreamCreateWithFlags(&g.m_srv_stream, hipStreamNonBlocking));
                g.m_launch = g.m_launch == 0x7FFFFFFF ? 1 : g.m_launch + 1;
                HIP_TRY(hvd::launch_match_server((const uint32_t*)g.m_pin, (int32_t*)(g.m_pin + small), (seq21 - 1u) & 0x1FFFFFu,
                                                 g.m_launch, 100ull * kMatchServerIdleUs, 100ull * kMatchServerLifeUs, g.m_srv_stream));
                return HVD_OK;
            };
            // ONE 64-bit word carries the whole request: a poll that sees the new sequence number has everything
            const unsigned long long word = ((unsigned long long)seq21 << 43) | ((unsigned long long)(uint32_t)max_dist << 32) |
                                            ((unsigned long long)(uint32_t)na << 16) | (unsigned long long)(uint32_t)nb;
            __atomic_store_n(reinterpret_cast<volatile unsigned long long*>(ph + 4), word, __ATOMIC_RELEASE);
            if (g.m_launch == 0 || __atomic_load_n(&ph[3], __ATOMIC_ACQUIRE) == g.m_launch)
                if (int rc = start_server()) return rc;
            bool seen = false;
            for (int attempt = 0; attempt < 3 && !seen; ++attempt) {
                for (long spin = 0; spin < 40000000; ++spin) {
                    if ((uint32_t)__atomic_load_n(&ph[2], __ATOMIC_ACQUIRE) == seq21) {
                        seen = true;
                        break;
                    }
                    // the server may have left between our look at hdr[3] and its last poll: start another, it finds the request
                    if ((spin & 1023) == 1023 && __atomic_load_n(&ph[3], __ATOMIC_ACQUIRE) == g.m_launch) break;
                }
                if (!seen) {
                    if (__atomic_load_n(&ph[3], __ATOMIC_ACQUIRE) != g.m_launch) break;  // still running and silent: give up below
                    if (int rc = start_server()) return rc;
                }
            }
            if (!seen) {
                HIP_TRY(hipStreamSynchronize(g.m_srv_stream));
                if ((uint32_t)__atomic_load_n(&ph[2], __ATOMIC_ACQUIRE) != seq21) return fail(HVD_ERR_HIP, "match server did not answer");
            }
            *q_hits = ph[0];
            *t_hits = ph[1];
            return HVD_OK;
        }
        HIP_TRY(hvd::launch_match_two_small((const uint32_t*)g.m_pin, (uint32_t)na, (const uint32_t*)pb, (uint32_t)nb,
                                            (uint32_t)max_dist, (int32_t*)(g.m_pin + small), seq, g.stream));
        bool seen = false;
        for (long spin = 0; spin < 4000000; ++spin) {  // ~ms; a failed launch never writes the word
            if (__atomic_load_n(&ph[2], __ATOMIC_ACQUIRE) == seq) {
                seen = true;
                break;
            }
        }
        if (!seen) {
            HIP_TRY(hipStreamSynchronize(g.stream));
            if (__atomic_load_n(&ph[2], __ATOMIC_ACQUIRE) != seq) return fail(HVD_ERR_HIP, "match kernel did not complete");
        }
        *q_hits = ph[0];
        *t_hits = ph[1];
        return HVD_OK;
    }
    if (int rc = grow(&g.m_a, &g.m_a_cap, 32 * (size_t)na)) return rc;
    if (int rc = grow(&g.m_b, &g.m_b_cap, 32 * (size_t)nb)) return rc;
    if (int rc = grow(&g.m_f, &g.m_f_cap, 4 * (size_t)nb)) return rc;
    if (!g.m_o) HIP_TRY(hipMalloc(&g.m_o, 8));
    HIP_TRY(hipMemcpyAsync(g.m_a, a, 32 * (size_t)na, hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipMemcpyAsync(g.m_b, b, 32 * (size_t)nb, hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hvd::launch_match_two((const uint32_t*)g.m_a, (uint32_t)na, (const uint32_t*)g.m_b, (uint32_t)nb,
                                  (uint32_t)max_dist, (uint32_t*)g.m_f, (int32_t*)g.m_o, g.stream));
    int32_t hits[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(hits, g.m_o, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    *q_hits = hits[0];
    *t_hits = hits[1];
    return HVD_OK;
}

/* ------------------------------------------ video-level search on the device (K3) -- */

}  // extern "C"

int hvdi::packed_hashes(Ctx::Scr slot, const void* d_img, uint32_t n, void** d_bits) {
    if (int rc = scratch(slot, 32 * (size_t)n, d_bits)) return rc;
    HIP_TRY(hvd::launch_pack_fp4(d_img, n, *d_bits, g.stream));
    return HVD_OK;
}

namespace {

unsigned long long pow2_at_least(unsigned long long x) {
    unsigned long long p = 1;
    while (p < x) p <<= 1;
    return p;
}

struct VmArgs {
    const void* d_img_q;  // == d_img_t in the symmetric form
    uint32_t nq;
    const void* d_img_t;
    uint32_t nt;
    bool rect;
    const int32_t *d_vid_q, *d_vid_t;    // video index of every frame (== each other in the symmetric form)
    const int32_t *d_excl_q, *d_excl_t;  // rect only: frames with equal values are not compared (nullable)
    int max_dist;                        // [0,127]
    int rank, world;
    int pre_rc = 0;                      // a failure of this rank BEFORE the search (upload): reported through the agreement step
    // the weighted fold (k_vmatch_weighted.hip): int32 per frame of each side (== each other in the symmetric
    // form), both or neither; null: the plain fold. max_weight caps a weight, 0 = no cap.
    const int32_t *d_weight_q = nullptr, *d_weight_t = nullptr;
    uint32_t max_weight = 0;
};

int read_counters(unsigned long long* d_counters, unsigned long long out[4]) {
    HIP_TRY(hipMemcpyAsync(out, d_counters, 32, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

// A hash table of the video search: the scratch slots `tables` share one size -- 4 slots of 8 bytes per key, a power of two, at
// least `floor` (hvd_debug_set "vmatch_slots_log2" forces the first size) -- and each is cleared to its byte; then insert(slots)
// runs. When some insert ran out of probes (c[0] != 0) the tables are rebuilt 4x larger and the same pass runs again.
struct Table {
    Ctx::Scr id;
    int fill;
    void** p;
};
template <class Insert>
int build_table(std::initializer_list<Table> tables, unsigned long long floor, unsigned long long keys, unsigned long long* d_counters,
                unsigned long long c[4], unsigned long long* slots, const Insert& insert) {
    *slots = g.v_force_slots_log2 ? 1ull << g.v_force_slots_log2 : pow2_at_least(std::max(floor, 4ull * keys));
    for (;; *slots *= 4) {
        for (const Table& t : tables)
            if (int rc = scratch(t.id, 8 * *slots, t.p)) return rc;
        for (const Table& t : tables) HIP_TRY(hipMemsetAsync(*t.p, t.fill, 8 * *slots, g.stream));
        HIP_TRY(hipMemsetAsync(d_counters, 0, 32, g.stream));
        if (int rc = insert(*slots)) return rc;
        if (int rc = read_counters(d_counters, c)) return rc;
        if (c[0] == 0) return HVD_OK;
    }
}

// The co-occurrence counts of a library's sample (hvd_bit_order.h: bit_order_sample) into d_cooc, 256 * 256 u32, on the
// context's stream; the transposed sample goes through pool slot S_BROWS (callers hold h_mu).
int count_bit_cooc(const void* d_bits, const hvd::BitSample& s, void* d_cooc) {
    void* d_rows = nullptr;
    SCR(S_BROWS, 8 * 256 * (size_t)s.words, d_rows);
    HIP_TRY(hvd::launch_bit_cooc(d_bits, s.stride, s.words, d_rows, d_cooc, g.stream));
    return HVD_OK;
}

// Which 128 bits should the first stage see? (k_fp4_image.hip: "data-dependent bit order".) The co-occurrence counts of a
// strided sample of the packed hashes, then the rule of hvd_bit_order.h: bit k of a rewritten hash is bit perm[k] of the
// original. Deterministic in the data, so every rank of a sharded search -- the library is replicated -- arrives at the same
// order. *changed = false: too few hashes, keep the order.
int choose_bit_order(const void* d_bits, uint32_t n, bool always, uint8_t perm[256], bool* changed) {
    *changed = false;
    for (int k = 0; k < 256; ++k) perm[k] = (uint8_t)k;
    const hvd::BitSample s = hvd::bit_order_sample(n, always);
    if (!s.sample) return HVD_OK;
    void* d_cooc = nullptr;
    SCR(S_BCOOC, 4 * 256 * 256, d_cooc);
    if (int rc = count_bit_cooc(d_bits, s, d_cooc)) return rc;
    std::vector<uint32_t> cooc(256 * 256);
    HIP_TRY(hipMemcpyAsync(cooc.data(), d_cooc, 4 * cooc.size(), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    hvd::bit_order_from_cooc(cooc.data(), s.sample, perm);
    for (int i = 0; i < 256; ++i) *changed = *changed || perm[i] != i;
    return HVD_OK;
}

// The key set of a video search, where vmatch_keys leaves it: a table (n_src slots, kEmptyKey = free) in the pool -- the local
// set, or the merged one after an exchange -- with n_keys keys.
struct VmKeys {
    const unsigned long long* d_src = nullptr;
    unsigned long long n_src = 0, n_keys = 0;
    unsigned long long* d_counters = nullptr;
};

// Key stage: all-pairs pass in video mode -> set of (frame, video) keys -> [key exchange between ranks]. Overflowing tables
// are rebuilt larger and only the step that overflowed is repeated; the inputs never move. The pair map of the last
// search (S_PKEYS, S_PCNT, g.v_pslots) is not touched.
int vmatch_keys(const VmArgs& v, VmKeys* keys) {
    const bool exchange = g.v_exchange_mode == 1 || (g.v_exchange_mode == 0 && v.world > 1);
    if (exchange && ((!g.comm_ready && !g.host_exchange) || g.world != v.world || g.rank != v.rank))
        return fail(HVD_ERR_STATE, "rank %d of %d needs hvd_comm_init() with the same rank/world first", v.rank, v.world);
    // world > 1: a rank that fails on its own (out of memory while a table regrows, a launch error) must not leave its
    // peers blocked in the all-gathers below. Everything up to the exchange runs inside `local`, whose result code goes into
    // the first agreement step with the key count: every rank learns of a failure anywhere and all of them return.
    unsigned long long* d_counters = nullptr;
    unsigned long long slots = 0;
    unsigned long long* d_set = nullptr;
    unsigned long long c[4] = {0, 0, 0, 0};
    auto local = [&]() -> int {
    if (v.pre_rc) return v.pre_rc;
    SCR(S_COUNTERS, 64, d_counters);
    // the pair-queue form of the all-pairs kernel settles its candidates on PACKED hashes; this entry is handed images only
    void *d_bits_t = nullptr, *d_bits_q = nullptr;
    const void *img_t = v.d_img_t, *img_q = v.d_img_q;
    if (int rc = packed_hashes(Ctx::S_BITS, v.d_img_t, v.nt, &d_bits_t)) return rc;
    if (v.rect)
        if (int rc = packed_hashes(Ctx::S_BITS2, v.d_img_q, v.nq, &d_bits_q)) return rc;
    // Round 5: the search runs on hashes rewritten in a bit order chosen from the library itself (choose_bit_order): the first
    // stage then sees the 128 least entangled bits. Library scratch only -- the caller's image is left as it is -- and the
    // same order for rows and columns, so every distance, and with it every record, is what it was.
    g.v_bit_order_used = 0;
    if (g.v_bit_order == 2 || (g.v_bit_order == 1 && v.nt >= 65536u)) {
        uint8_t perm[256];
        bool changed = false;
        if (int rc = choose_bit_order(d_bits_t, v.nt, g.v_bit_order == 2, perm, &changed)) return rc;
        if (changed) {
            size_t img_bytes = 0;
            void *d_bo = nullptr, *d_io = nullptr;
            if (int rc = hvd_fp4_image_bytes((int64_t)v.nt, &img_bytes)) return rc;
            SCR(S_BITS_O, 32 * (size_t)v.nt, d_bo);
            SCR(S_IMG_O, img_bytes, d_io);
            HIP_TRY(hvd::launch_reorder_bits(d_bits_t, v.nt, perm, d_bo, d_io, g.stream));
            d_bits_t = d_bo;
            img_t = d_io;
            if (v.rect) {
                if (int rc = hvd_fp4_image_bytes((int64_t)v.nq, &img_bytes)) return rc;
                SCR(S_BITS2_O, 32 * (size_t)v.nq, d_bo);
                SCR(S_IMG2_O, img_bytes, d_io);
                HIP_TRY(hvd::launch_reorder_bits(d_bits_q, v.nq, perm, d_bo, d_io, g.stream));
                d_bits_q = d_bo;
                img_q = d_io;
            } else {
                img_q = img_t;
            }
            g.v_bit_order_used = 1;
        }
    }
#ifndef HVD_NO_BENCH_SYMBOLS
    if (g.v_fail_rank == v.rank + 1) return fail(HVD_ERR_HIP, "injected failure on rank %d (hvd_debug_set vmatch_fail_rank)", v.rank);
#endif
    const unsigned long long frames = (unsigned long long)v.nt + (v.rect ? v.nq : 0u);
    return build_table({{Ctx::S_SET, 0xFF, (void**)&d_set}}, 1ull << 16, frames, d_counters, c, &slots, [&](unsigned long long n) -> int {
        hvd::AllPairsArgs a;
        a.d_db = d_bits_t;
        a.d_db_q = d_bits_q;
        a.n = v.nt;
        a.sync_decide = true;  // (this call waits for its result anyway)
        a.d_group = v.rect ? v.d_excl_q : v.d_vid_q;  // symmetric: frames of one video never match each other
        a.max_dist = (uint32_t)v.max_dist;
        a.rank = (uint32_t)v.rank;
        a.world = (uint32_t)v.world;
        a.d_pairs = nullptr;
        a.cap = 0;
        a.d_count = d_counters + 3;
        a.variant = g.v_variant ? g.v_variant : HVD_DEFAULT_VARIANT;
        a.col_chunk = 0;
        a.ctx_id = t_ctx;
        a.sink = hvd::VideoSink{d_set, n - 1, d_counters, v.d_vid_q, v.d_vid_t};
        hipError_t e = v.rect ? hvd::launch_cross_mfma(a, img_q, v.nq, img_t, v.d_excl_t, g.stream)
                              : hvd::launch_allpairs_mfma(a, img_t, g.stream);
        if (e != hipSuccess) return fail(HVD_ERR_HIP, "video-level all-pairs launch: %s", hipGetErrorString(e));
        return HVD_OK;
    });
    };
    const auto t_begin = std::chrono::steady_clock::now();
    auto us_since = [](std::chrono::steady_clock::time_point t0) {
        return (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    };
    const int local_rc = local();  // (ends in read_counters: the stream is drained, host time is device time)
    g.v_us[0] = us_since(t_begin);
    g.v_us[1] = g.v_us[2] = 0;
    if (!exchange && local_rc) return local_rc;
    const auto t_exchange = std::chrono::steady_clock::now();
    const unsigned long long* d_src = d_set;
    unsigned long long n_src = slots, n_keys = c[1];
    if (exchange) {
        // each rank saw only its tiles' hits: all-gather the key lists and de-duplicate (a key may be found twice)
        unsigned long long *d_list = nullptr, *d_all = nullptr, *d_set2 = nullptr, slots2 = 0;
        const int W = g.world;
        std::vector<unsigned long long> counts;
        if (int rc = agree(n_keys, local_rc, "video search", counts)) return rc;
        unsigned long long mx = 1, total = 0;
        for (unsigned long long k : counts) {
            mx = std::max(mx, k);
            total += k;
        }
        // the exchange buffers depend on the gathered counts: allocate, then agree once more before the big all-gather
        const int alloc_rc = [&]() -> int {
            SCR(S_LIST, 8 * mx, d_list);  // this rank's keys, padded with empty keys to the longest list
            SCR(S_LISTALL, 8 * mx * (size_t)W, d_all);
            return HVD_OK;
        }();
        if (int rc = agree(0, alloc_rc, "video key exchange", counts)) return rc;
        HIP_TRY(hipMemsetAsync(d_list, 0xFF, 8 * mx, g.stream));
        HIP_TRY(hipMemsetAsync(d_counters + 2, 0, 8, g.stream));
        HIP_TRY(hvd::launch_set_to_list(d_set, slots, d_list, mx, d_counters + 2, g.stream));
        if (int rc = allgather_bytes(d_list, d_all, 8 * mx)) return rc;
        if (int rc = build_table({{Ctx::S_SET2, 0xFF, (void**)&d_set2}}, 1ull << 16, total, d_counters, c, &slots2,
                                 [&](unsigned long long n) -> int {
                                     HIP_TRY(hvd::launch_list_to_set(d_all, mx * (unsigned long long)W, d_set2, n - 1, d_counters, g.stream));
                                     return HVD_OK;
                                 }))
            return rc;
        d_src = d_set2;
        n_src = slots2;
        n_keys = c[1];
        g.v_us[1] = us_since(t_exchange);
    }
    *keys = VmKeys{d_src, n_src, n_keys, d_counters};
    return HVD_OK;
}

// Key stage, then the fold stage: key set -> pair map with the vPDQ counters, left in the pool for vmatch_emit.
int vmatch_build(const VmArgs& v) {
    VmKeys k;
    if (int rc = vmatch_keys(v, &k)) return rc;
    const auto t_fold = std::chrono::steady_clock::now();
    unsigned long long* d_pkeys = nullptr;
    void* d_pcnt = nullptr;
    unsigned long long pslots = 0, c[4] = {0, 0, 0, 0};
    if (int rc = build_table({{Ctx::S_PKEYS, 0xFF, (void**)&d_pkeys}, {Ctx::S_PCNT, 0, &d_pcnt}}, 1024, k.n_keys, k.d_counters, c,
                             &pslots, [&](unsigned long long n) -> int {
                                 // (both tables were cleared for this pass: a weighted pass that runs again adds to zeroes)
                                 if (v.d_weight_q)
                                     HIP_TRY(hvd::launch_keys_to_pairs_weighted(k.d_src, k.n_src, v.d_vid_q, v.d_vid_t, v.rect,
                                                                                v.d_weight_q, v.d_weight_t, v.max_weight, d_pkeys,
                                                                                d_pcnt, n - 1, k.d_counters, g.stream));
                                 else
                                     HIP_TRY(hvd::launch_keys_to_pairs(k.d_src, k.n_src, v.d_vid_q, v.d_vid_t, v.rect, d_pkeys, d_pcnt,
                                                                       n - 1, k.d_counters, g.stream));
                                 return HVD_OK;
                             }))
        return rc;
    g.v_pslots = pslots;
    g.v_us[2] = (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_fold).count();
    return HVD_OK;
}

// Pair map -> hvd_vmatch records (unordered) in d_out[cap]; *d_count (device uint64) = number of video pairs.
int vmatch_emit(hvd_vmatch* d_out, int64_t cap, unsigned long long* d_count) {
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, g.stream));
    HIP_TRY(hvd::launch_pairs_emit((const unsigned long long*)g.scr[Ctx::S_PKEYS], g.scr[Ctx::S_PCNT], g.v_pslots, d_out,
                                   (unsigned long long)cap, d_count, g.stream));
    return HVD_OK;
}

bool vmatch_less(const hvd_vmatch& x, const hvd_vmatch& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; }

// build + emit into the pool's record buffer, grown until everything fits (only the emit is repeated); unordered
int vmatch_to_host(const VmArgs& v, int64_t expect, std::vector<hvd_vmatch>& res) {
    if (int rc = vmatch_build(v)) return rc;
    unsigned long long* d_counters = nullptr;
    SCR(S_COUNTERS, 64, d_counters);
    int64_t dcap = std::max<int64_t>(1 << 12, expect);
    for (;;) {
        hvd_vmatch* d_out = nullptr;
        SCR(S_VOUT, sizeof(hvd_vmatch) * (size_t)dcap, d_out);
        if (int rc = vmatch_emit(d_out, dcap, d_counters + 3)) return rc;
        unsigned long long cnt = 0;
        HIP_TRY(hipMemcpyAsync(&cnt, d_counters + 3, 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if ((int64_t)cnt > dcap) {
            dcap = (int64_t)cnt;
            continue;
        }
        res.resize((size_t)cnt);
        if (cnt) {
            HIP_TRY(hipMemcpyAsync(res.data(), d_out, sizeof(hvd_vmatch) * (size_t)cnt, hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipStreamSynchronize(g.stream));
        }
        break;
    }
    return HVD_OK;
}

int check_offsets(const int64_t* offsets, int64_t V, int64_t* nf) {
    if (V < 0 || !offsets) return fail(HVD_ERR_ARG, "bad offsets");
    if (offsets[0] != 0) return fail(HVD_ERR_ARG, "offsets[0] must be 0");
    for (int64_t v = 0; v < V; ++v)
        if (offsets[v + 1] < offsets[v]) return fail(HVD_ERR_ARG, "offsets must be non-decreasing");
    *nf = V > 0 ? offsets[V] : 0;
    if (*nf >= (1ll << 32) - 1 || V >= (1ll << 31)) return fail(HVD_ERR_ARG, "too many frames/videos");
    return HVD_OK;
}

// upload one side of a host library: frame hashes -> FP4 image, CSR offsets -> frame->video map
int upload_library(const uint8_t* frames, const int64_t* offsets, int64_t V, int64_t nf, Ctx::Scr s_db, Ctx::Scr s_img,
                   Ctx::Scr s_vid, void** d_img, int32_t** d_vid) {
    void* d_db = nullptr;
    long long* d_off = nullptr;
    if (int rc = scratch(s_db, 32 * (size_t)nf, &d_db)) return rc;
    size_t ib = 0;
    if (int rc = hvd_fp4_image_bytes(nf, &ib)) return rc;
    if (int rc = scratch(s_img, ib, d_img)) return rc;
    if (int rc = scratch(s_vid, 4 * (size_t)nf, (void**)d_vid)) return rc;
    SCR(S_OFF, 8 * (size_t)(V + 1), d_off);
    HIP_TRY(hipMemcpyAsync(d_db, frames, 32 * (size_t)nf, hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipMemcpyAsync(d_off, offsets, 8 * (size_t)(V + 1), hipMemcpyHostToDevice, g.stream));
    if (int rc = hvd_dev_expand_fp4(d_db, nf, *d_img)) return rc;
    HIP_TRY(hvd::launch_video_of_frames(d_off, (uint32_t)V, (unsigned long long)nf, *d_vid, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));  // S_OFF is reused by the other side
    return HVD_OK;
}

/* ---- the video search's operands: one description from the entry to the fold ---- */

// One side of a search as a host entry is handed it. n: the frame count check_offsets finds.
struct HostSide {
    const uint8_t* frames;
    const int64_t* offsets;
    int64_t V;
    const int32_t* ids = nullptr;      // per video, both sides or neither: videos with equal ids are never compared
    const int32_t* weights = nullptr;  // per frame, the weighted search only
    int64_t* out_totals = nullptr;     // int64[V], the weighted search only, nullable
    int64_t n = 0;
};

// One side as it lies in HBM: what a device entry is handed, and what upload_side leaves of a HostSide.
struct DevSide {
    const void* d_img = nullptr;
    int64_t n = 0;
    const void* d_video = nullptr;
    const void* d_excl = nullptr;    // per frame, both sides or neither
    const void* d_weight = nullptr;  // per frame, the weighted search only
};

// What a call asks for besides its sides. A search without a target side is the symmetric one: target side == query side.
struct VmCall {
    int max_dist;
    int dist_limit;           // the entry's largest max_dist: 127, or 256 where the popcount route stands behind it
    bool weighted = false;    // the weighted fold: weights on every side, max_weight caps one (0 = no cap)
    int max_weight = 0;
    int rank = 0, world = 1;
    bool args_first = false;  // a host entry that judges every argument before the library's state (the weighted ones), not after

    static VmCall plain(int max_dist, int dist_limit = 127, int rank = 0, int world = 1) {
        return {max_dist, dist_limit, false, 0, rank, world, false};
    }
    static VmCall with_weights(int max_dist, int max_weight, bool args_first) { return {max_dist, 127, true, max_weight, 0, 1, args_first}; }
};

// where the records go: out[cap] and their count, all in host memory or all in HBM
struct VmOut {
    void* out;
    int64_t cap;
    void* count;
};

// The one place a VmArgs is put together: the symmetric form names its side twice, the rectangle sets `rect`.
VmArgs vm_args(const VmCall& c, const DevSide& q, const DevSide* t) {
    const DevSide& s = t ? *t : q;
    VmArgs v{};
    v.d_img_q = q.d_img, v.nq = (uint32_t)q.n, v.d_img_t = s.d_img, v.nt = (uint32_t)s.n;
    v.rect = t != nullptr;
    v.d_vid_q = (const int32_t*)q.d_video, v.d_vid_t = (const int32_t*)s.d_video;
    v.d_excl_q = (const int32_t*)q.d_excl, v.d_excl_t = (const int32_t*)s.d_excl;
    v.max_dist = c.max_dist, v.rank = c.rank, v.world = c.world;
    if (c.weighted) v.d_weight_q = (const int32_t*)q.d_weight, v.d_weight_t = (const int32_t*)s.d_weight, v.max_weight = (uint32_t)c.max_weight;
    return v;
}

// the scalars every entry shares; o: where the records go (the spread entries have none)
int check_call(const VmCall& c, const VmOut* o) {
    if (c.max_dist < 0 || c.max_dist > c.dist_limit) return fail(HVD_ERR_ARG, "max_dist=%d out of range [0,%d]", c.max_dist, c.dist_limit);
    if (c.max_weight < 0) return fail(HVD_ERR_ARG, "max_weight=%d must not be negative (0 = no cap)", c.max_weight);
    if (c.world < 1 || c.rank < 0 || c.rank >= c.world) return fail(HVD_ERR_ARG, "bad rank/world %d/%d", c.rank, c.world);
    if (o && (o->cap < 0 || !o->count || (o->cap > 0 && !o->out))) return fail(HVD_ERR_ARG, "bad output buffer");
    return HVD_OK;
}

int check_paired(const void* q, const void* t, const char* what) {
    if ((q == nullptr) != (t == nullptr)) return fail(HVD_ERR_ARG, "pass both %s or neither", what);
    return HVD_OK;
}

// The sides of a device entry: sizes, the exclusion maps, and -- unless there is nothing to compare -- what every side needs.
int check_dev_sides(const VmCall& c, const DevSide& q, const DevSide* t, bool* empty) {
    for (const DevSide* s : {&q, t})
        if (s && (s->n < 0 || s->n >= (1ll << 32) - 1)) return fail(HVD_ERR_ARG, "set size %lld out of range", (long long)s->n);
    if (t)
        if (int rc = check_paired(q.d_excl, t->d_excl, "exclusion maps")) return rc;
    *empty = t ? q.n == 0 || t->n == 0 : q.n < 2;
    for (const DevSide* s : {&q, t})
        if (s && !*empty && (!s->d_img || !s->d_video || (c.weighted && !s->d_weight)))
            return fail(HVD_ERR_ARG, "NULL image / video map%s", c.weighted ? " / weights" : "");
    return HVD_OK;
}

// The weights of a host library, before the library asks whether a device is there: one per frame, each at least 1, and per
// video a capped total that the uint32 counters of a record can hold. out_totals: int64[V] or NULL.
int check_weights(const int32_t* weights, const int64_t* offsets, int64_t V, int64_t nf, int max_weight, int64_t* out_totals) {
    if (nf > 0 && !weights) return fail(HVD_ERR_ARG, "weights is NULL");
    for (int64_t v = 0; v < V; ++v) {
        uint64_t total = 0;
        for (int64_t f = offsets[v]; f < offsets[v + 1]; ++f) {
            if (weights[f] < 1) return fail(HVD_ERR_ARG, "weight %d of frame %lld (video %lld): weights are at least 1", weights[f], (long long)f, (long long)v);
            total += (uint64_t)(max_weight > 0 && weights[f] > max_weight ? max_weight : weights[f]);
        }
        if (total > 0xFFFFFFFFull)
            return fail(HVD_ERR_ARG, "video %lld: capped weight total %llu exceeds 2^32 - 1 (the counters are uint32)", (long long)v, (unsigned long long)total);
        if (out_totals) out_totals[v] = (int64_t)total;
    }
    return HVD_OK;
}

// The sides of a host entry: the CSRs (-> n), the frames, then -- weighted -- the weights, whose totals are written last. An
// args-first entry wants the frames of every side that has any; the others only when there is something to compare.
int check_host_sides(const VmCall& c, HostSide& q, HostSide* t, bool* empty) {
    for (HostSide* s : {&q, t})
        if (s)
            if (int rc = check_offsets(s->offsets, s->V, &s->n)) return rc;
    *empty = t ? q.n == 0 || t->n == 0 : q.n < 2;
    for (const HostSide* s : {&q, t})
        if (s && (c.args_first ? s->n > 0 : !*empty) && !s->frames) return fail(HVD_ERR_ARG, "frames is NULL");
    for (const HostSide* s : {&q, t})
        if (s && c.weighted)
            if (int rc = check_weights(s->weights, s->offsets, s->V, s->n, c.max_weight, s->out_totals)) return rc;
    return HVD_OK;
}

// One value per frame from one per video: the form the exclusion maps take on the device.
std::vector<int32_t> frame_ids(const HostSide& s) {
    std::vector<int32_t> ids(s.ids ? (size_t)s.n : 0);
    for (int64_t v = 0; s.ids && v < s.V; ++v)
        for (int64_t f = s.offsets[v]; f < s.offsets[v + 1]; ++f) ids[(size_t)f] = s.ids[v];
    return ids;
}

// One host side into its scratch slots (the query side's, or the target side's): the library, then the weights and the
// per-frame ids where the call has them. The two small copies are not waited for: the caller drains the stream after its last side.
int upload_side(const VmCall& c, const HostSide& s, const std::vector<int32_t>& ids, bool target, DevSide* d) {
    void* d_img = nullptr;
    int32_t *d_vid = nullptr, *d_w = nullptr, *d_ids = nullptr;
    if (int rc = upload_library(s.frames, s.offsets, s.V, s.n, target ? Ctx::S_DB2 : Ctx::S_DB, target ? Ctx::S_IMG2 : Ctx::S_IMG,
                                target ? Ctx::S_VIDT : Ctx::S_VIDQ, &d_img, &d_vid))
        return rc;
    if (c.weighted) {
        if (int rc = scratch(target ? Ctx::S_WT : Ctx::S_WQ, 4 * (size_t)s.n, (void**)&d_w)) return rc;
        HIP_TRY(hipMemcpyAsync(d_w, s.weights, 4 * (size_t)s.n, hipMemcpyHostToDevice, g.stream));
    }
    if (s.ids) {
        if (int rc = scratch(target ? Ctx::S_GRP2 : Ctx::S_GRP, 4 * (size_t)s.n, (void**)&d_ids)) return rc;
        HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), 4 * (size_t)s.n, hipMemcpyHostToDevice, g.stream));
    }
    *d = DevSide{d_img, s.n, d_vid, d_ids, d_w};
    return HVD_OK;
}

// both sides of a host call (t == nullptr: one) on the current context; the stream is drained after the id copies
int upload_sides(const VmCall& c, const HostSide& q, const HostSide* t, const std::vector<int32_t>& ids_q,
                 const std::vector<int32_t>& ids_t, DevSide* dq, DevSide* dt) {
    if (int rc = upload_side(c, q, ids_q, false, dq)) return rc;
    if (t)
        if (int rc = upload_side(c, *t, ids_t, true, dt)) return rc;
    if (q.ids) HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

// The four host searches: judge, upload, search, sort the records out. t == nullptr: the symmetric search.
int vmatch_from_host(const VmCall& c, HostSide q, HostSide* t, const VmOut& o) {
    int64_t* out_count = (int64_t*)o.count;
    if (!c.args_first)
        if (int rc = need_ready()) return rc;
    if (int rc = check_call(c, &o)) return rc;
    if (t)
        if (int rc = check_paired(q.ids, t->ids, "id arrays")) return rc;
    if (!c.args_first) *out_count = 0;
    bool empty = false;
    if (int rc = check_host_sides(c, q, t, &empty)) return rc;
    if (c.args_first) {
        if (int rc = need_ready()) return rc;
        *out_count = 0;
    }
    if (empty) return HVD_OK;
    std::vector<hvd_vmatch> res;
    if (c.max_dist >= 128) {
        // popcount route (a tolerance the reference never uses; the plain symmetric entry alone admits it): frame-level hits
        // reduced on the host
        std::lock_guard<std::recursive_mutex> lk(g.h_mu);
        std::vector<int32_t> vid((size_t)q.n);
        for (int64_t v = 0; v < q.V; ++v)
            for (int64_t f = q.offsets[v]; f < q.offsets[v + 1]; ++f) vid[(size_t)f] = (int32_t)v;
        std::vector<hvd_pair> recs;
        int64_t fcap = std::max<int64_t>(1 << 16, q.n), fcount = 0;
        for (;;) {
            if (int rc = allpairs_host_raw(q.frames, q.n, vid.data(), c.max_dist, recs, fcap, &fcount)) return rc;
            if (fcount <= fcap) break;
            fcap = fcount;
        }
        aggregate_video_hits(recs, vid.data(), vid.data(), res);
    } else {
        const std::vector<int32_t> ids_q = frame_ids(q), ids_t = t ? frame_ids(*t) : std::vector<int32_t>();
        // one rank's share (rank r of W contexts; W = 1: the whole search on the current context). A failed upload returns at
        // once when this context is alone, and travels as pre_rc to the agreement step when it is one of a group.
        auto one = [&](int r, int W, std::vector<hvd_vmatch>& mine) -> int {
            std::lock_guard<std::recursive_mutex> lk(g.h_mu);
            DevSide dq, dt;
            const int up = upload_sides(c, q, t, ids_q, ids_t, &dq, &dt);
            if (W == 1 && up) return up;
            VmCall mine_of = c;
            mine_of.rank = r, mine_of.world = W;
            VmArgs v = vm_args(mine_of, dq, t ? &dt : nullptr);
            v.pre_rc = up;
            return vmatch_to_host(v, q.V, mine);
        };
        // The group: library replicated on every device, tile (rb, cb) -> context (rb + cb) % W, key sets exchanged inside
        // vmatch_build (RCCL all-gather between the devices, host memory where the group has no RCCL); every rank ends up with
        // the whole result, rank 0's is returned. From 4096 frames, in both sets together. Only the plain searches fan out: the
        // weighted ones stay on the calling context, whatever the group (a weighted search over the group is not built).
        const int W = !c.weighted && g_nctx > 1 && q.n + (t ? t->n : 0) >= 4096 ? g_nctx : 1;
        if (W > 1) {
            if (int rc = run_keep_rank0(res, [&](int r, std::vector<hvd_vmatch>& mine) { return one(r, W, mine); })) return rc;
        } else if (int rc = one(0, 1, res)) {
            return rc;
        }
    }
    return copy_out(res, (int64_t)res.size(), vmatch_less, (hvd_vmatch*)o.out, o.cap, out_count, c.weighted ? "weighted video match" : "video match");
}

// The four device searches: nothing to compare zeroes the count, otherwise build + emit; the stream is drained either way.
int vmatch_dev_entry(const VmCall& c, const DevSide& q, const DevSide* t, const VmOut& o) {
    if (int rc = need_ready()) return rc;
    if (int rc = check_call(c, &o)) return rc;
    bool empty = false;
    if (int rc = check_dev_sides(c, q, t, &empty)) return rc;
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    if (empty) {
        HIP_TRY(hipMemsetAsync(o.count, 0, 8, g.stream));
    } else {
        if (int rc = vmatch_build(vm_args(c, q, t))) return rc;
        if (int rc = vmatch_emit((hvd_vmatch*)o.out, o.cap, (unsigned long long*)o.count)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

// The two device spread entries: the key stage of the search on this context alone, then the count per frame. No pair map is
// built, the last search's stays. The rectangle takes either output alone and zeroes by itself where there is nothing to
// compare (unless it accumulates); it launches nothing else on an empty key set. The stream is drained.
int spread_dev_entry(int max_dist, const DevSide& q, const DevSide* t, bool accumulate, void* d_spread_q, void* d_spread_t) {
    if (int rc = need_ready()) return rc;
    if (t ? !d_spread_q && !d_spread_t : q.n > 0 && !d_spread_q) return fail(HVD_ERR_ARG, "NULL spread output");
    const VmCall c = VmCall::plain(max_dist);
    if (int rc = check_call(c, nullptr)) return rc;
    bool empty = false;
    if (int rc = check_dev_sides(c, q, t, &empty)) return rc;
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    VmKeys k;
    if (!empty)
        if (int rc = vmatch_keys(vm_args(c, q, t), &k)) return rc;
    if (t)
        HIP_TRY(hvd::launch_keys_to_spread_cross(k.d_src, k.n_src, (unsigned long long)q.n, (unsigned long long)t->n, accumulate,
                                                 (int32_t*)d_spread_q, (int32_t*)d_spread_t, g.stream));
    else if (!empty)
        HIP_TRY(hvd::launch_keys_to_spread(k.d_src, k.n_src, (unsigned long long)q.n, (int32_t*)d_spread_q, g.stream));
    else if (q.n > 0)
        HIP_TRY(hipMemsetAsync(d_spread_q, 0, 4 * (size_t)q.n, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

// the two host spread entries: every side with frames needs its output; nothing to compare answers zeroes without a device call
int spread_from_host(int max_dist, HostSide q, HostSide* t, int32_t* out_q, int32_t* out_t) {
    if (int rc = need_ready()) return rc;
    const VmCall c = VmCall::plain(max_dist);
    if (int rc = check_call(c, nullptr)) return rc;
    bool empty = false;
    if (int rc = check_host_sides(c, q, t, &empty)) return rc;
    const int64_t nt = t ? t->n : 0;
    if ((q.n > 0 && !out_q) || (nt > 0 && !out_t)) return fail(HVD_ERR_ARG, "out_spread is NULL");
    if (empty) {
        if (q.n > 0) memset(out_q, 0, 4 * (size_t)q.n);
        if (nt > 0) memset(out_t, 0, 4 * (size_t)nt);
        return HVD_OK;
    }
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    DevSide dq, dt;
    int32_t* d_spread = nullptr;
    if (int rc = upload_sides(c, q, t, {}, {}, &dq, &dt)) return rc;
    SCR(S_SPREAD, 4 * (size_t)(q.n + nt), d_spread);
    if (int rc = spread_dev_entry(max_dist, dq, t ? &dt : nullptr, false, d_spread, d_spread + q.n)) return rc;
    HIP_TRY(hipMemcpyAsync(out_q, d_spread, 4 * (size_t)q.n, hipMemcpyDeviceToHost, g.stream));
    if (t) HIP_TRY(hipMemcpyAsync(out_t, d_spread + q.n, 4 * (size_t)nt, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

}  // namespace

extern "C" {

int hvd_vpdq_match_videos(const uint8_t* frames, const int64_t* offsets, int64_t V, int max_dist, hvd_vmatch* out,
                          int64_t cap, int64_t* out_count) {
    return vmatch_from_host(VmCall::plain(max_dist, 256), {frames, offsets, V}, nullptr, {out, cap, out_count});
}

int hvd_vpdq_frame_spread(const uint8_t* frames, const int64_t* offsets, int64_t V, int max_dist, int32_t* out_spread) {
    return spread_from_host(max_dist, {frames, offsets, V}, nullptr, out_spread, nullptr);
}

int hvd_vpdq_match_videos_cross(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* ids_q,
                                const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* ids_t,
                                int max_dist, hvd_vmatch* out, int64_t cap, int64_t* out_count) {
    HostSide t{frames_t, offsets_t, VT, ids_t};
    return vmatch_from_host(VmCall::plain(max_dist), {frames_q, offsets_q, VQ, ids_q}, &t, {out, cap, out_count});
}

int hvd_vpdq_frame_spread_cross(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const uint8_t* frames_t,
                                const int64_t* offsets_t, int64_t VT, int max_dist, int32_t* out_spread_q, int32_t* out_spread_t) {
    HostSide t{frames_t, offsets_t, VT};
    return spread_from_host(max_dist, {frames_q, offsets_q, VQ}, &t, out_spread_q, out_spread_t);
}

/* ---- device-resident forms: hashes / images / maps already in HBM (BASELINE config 5) ---- */

int hvd_dev_video_of_frames(const void* d_offsets, int64_t V, int64_t n, void* d_out_video) {
    if (int rc = need_ready()) return rc;
    if (V < 0 || n < 0 || V >= (1ll << 31) || n >= (1ll << 32) - 1 || !d_offsets || (n > 0 && !d_out_video))
        return fail(HVD_ERR_ARG, "bad arguments");
    HIP_TRY(hvd::launch_video_of_frames((const long long*)d_offsets, (uint32_t)V, (unsigned long long)n, (int32_t*)d_out_video,
                                        g.stream));
    return HVD_OK;
}

int hvd_dev_compact_kept(const void* d_hashes, const void* d_quality, int64_t n, const void* d_offsets, int64_t V,
                         int min_quality, void* d_out_hashes, void* d_out_offsets, void* d_out_video, int64_t* out_kept) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || V < 0 || n >= (1ll << 32) - 1 || V >= (1ll << 31) || !d_offsets || !d_out_offsets || !out_kept)
        return fail(HVD_ERR_ARG, "bad arguments");
    if (n > 0 && (!d_hashes || !d_quality || !d_out_hashes || !d_out_video)) return fail(HVD_ERR_ARG, "NULL device pointer");
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    void* d_scr = nullptr;
    unsigned long long* d_counters = nullptr;
    SCR(S_COMPACT, hvd::compact_scratch_bytes((unsigned long long)n), d_scr);
    SCR(S_COUNTERS, 64, d_counters);
    HIP_TRY(hvd::launch_compact_kept(d_hashes, (const int32_t*)d_quality, (unsigned long long)n, (const long long*)d_offsets,
                                     (uint32_t)V, min_quality, d_out_hashes, (long long*)d_out_offsets, (int32_t*)d_out_video,
                                     d_scr, d_counters + 2, g.stream));
    unsigned long long kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, d_counters + 2, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    *out_kept = (int64_t)kept;
    return HVD_OK;
}

int hvd_dev_compact_kept_dihedral(const void* d_hashes8, const void* d_quality, int64_t n, const void* d_offsets, int64_t V,
                                  int min_quality, int transform_mask, void* d_out_hashes, void* d_out_offsets,
                                  void* d_out_video, void* d_out_qhashes, void* d_out_qvideo, void* d_out_qexcl,
                                  int64_t* out_kept) {
    if (int rc = need_ready()) return rc;
    if (!(transform_mask & 1) || transform_mask < 0 || transform_mask > 0xff)
        return fail(HVD_ERR_ARG, "transform_mask=%d: bits 0..7 only, bit 0 (identity) set", transform_mask);
    const int64_t K = __builtin_popcount((unsigned)transform_mask) - 1;
    if (n < 0 || V < 0 || n >= (1ll << 32) - 1 || V >= (1ll << 31) || V * (K > 0 ? K : 1) >= (1ll << 31) || !d_offsets ||
        !d_out_offsets || !out_kept)
        return fail(HVD_ERR_ARG, "bad arguments");
    if (n > 0 && (!d_hashes8 || !d_quality || !d_out_hashes || !d_out_video)) return fail(HVD_ERR_ARG, "NULL device pointer");
    if (n > 0 && V == 0) return fail(HVD_ERR_ARG, "n=%lld frames in no video", (long long)n);
    if (n > 0 && K > 0 && (!d_out_qhashes || !d_out_qvideo || !d_out_qexcl)) return fail(HVD_ERR_ARG, "NULL query output");
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    void* d_scr = nullptr;
    unsigned long long* d_counters = nullptr;
    SCR(S_COMPACT, hvd::compact_scratch_bytes((unsigned long long)n), d_scr);
    SCR(S_COUNTERS, 64, d_counters);
    HIP_TRY(hvd::launch_compact_kept_dihedral(d_hashes8, (const int32_t*)d_quality, (unsigned long long)n,
                                              (const long long*)d_offsets, (uint32_t)V, min_quality, (uint32_t)transform_mask,
                                              d_out_hashes, (long long*)d_out_offsets, (int32_t*)d_out_video, d_out_qhashes,
                                              (int32_t*)d_out_qvideo, (int32_t*)d_out_qexcl, d_scr, d_counters + 2, g.stream));
    unsigned long long kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, d_counters + 2, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    *out_kept = (int64_t)kept;
    return HVD_OK;
}

int hvd_dev_vpdq_match_videos(const void* d_img, int64_t n, const void* d_video, int max_dist, int rank, int world,
                              void* d_out, int64_t cap, void* d_count) {
    return vmatch_dev_entry(VmCall::plain(max_dist, 127, rank, world), {d_img, n, d_video}, nullptr, {d_out, cap, d_count});
}

int hvd_dev_vpdq_emit_again(void* d_out, int64_t cap, void* d_count) {
    if (int rc = need_ready()) return rc;
    if (cap < 0 || !d_count || (cap > 0 && !d_out)) return fail(HVD_ERR_ARG, "bad output buffer");
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    if (g.v_pslots == 0 || !g.scr[Ctx::S_PKEYS]) return fail(HVD_ERR_STATE, "no video search to emit from: call hvd_dev_vpdq_match_videos[_cross] first");
    if (int rc = vmatch_emit((hvd_vmatch*)d_out, cap, (unsigned long long*)d_count)) return rc;
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

int hvd_dev_vpdq_frame_spread(const void* d_img, int64_t n, const void* d_video, int max_dist, void* d_out_spread) {
    return spread_dev_entry(max_dist, {d_img, n, d_video}, nullptr, false, d_out_spread, nullptr);
}

int hvd_dev_vpdq_frame_spread_cross(const void* d_img_q, int64_t nq, const void* d_video_q, const void* d_img_t, int64_t nt,
                                    const void* d_video_t, int max_dist, int accumulate, void* d_spread_q, void* d_spread_t) {
    const DevSide t{d_img_t, nt, d_video_t};
    return spread_dev_entry(max_dist, {d_img_q, nq, d_video_q}, &t, accumulate != 0, d_spread_q, d_spread_t);
}

int hvd_dev_vpdq_match_videos_cross(const void* d_img_q, int64_t nq, const void* d_video_q, const void* d_excl_q,
                                    const void* d_img_t, int64_t nt, const void* d_video_t, const void* d_excl_t,
                                    int max_dist, int rank, int world, void* d_out, int64_t cap, void* d_count) {
    const DevSide t{d_img_t, nt, d_video_t, d_excl_t};
    return vmatch_dev_entry(VmCall::plain(max_dist, 127, rank, world), {d_img_q, nq, d_video_q, d_excl_q}, &t, {d_out, cap, d_count});
}

/* ---- duration-weighted video search (k_vmatch_weighted.hip) ---- */

int hvd_dev_video_weights(const void* d_weight, const void* d_offsets, int64_t V, int64_t n, int max_weight, void* d_out_totals) {
    if (max_weight < 0) return fail(HVD_ERR_ARG, "max_weight=%d must not be negative (0 = no cap)", max_weight);
    if (n < 0 || V < 0 || n >= (1ll << 32) - 1 || V >= (1ll << 31) || !d_offsets) return fail(HVD_ERR_ARG, "bad arguments");
    if ((n > 0 && !d_weight) || (V > 0 && !d_out_totals)) return fail(HVD_ERR_ARG, "NULL device pointer");
    if (n > 0 && V == 0) return fail(HVD_ERR_ARG, "n=%lld frames in no video", (long long)n);
    if (int rc = need_ready()) return rc;
    HIP_TRY(hvd::launch_video_weights((const int32_t*)d_weight, (const long long*)d_offsets, (uint32_t)V, (unsigned long long)n,
                                      (uint32_t)max_weight, (long long*)d_out_totals, g.stream));
    return HVD_OK;
}

int hvd_dev_vpdq_match_videos_weighted(const void* d_img, int64_t n, const void* d_video, const void* d_weight, int max_weight,
                                       int max_dist, void* d_out, int64_t cap, void* d_count) {
    return vmatch_dev_entry(VmCall::with_weights(max_dist, max_weight, false), {d_img, n, d_video, nullptr, d_weight}, nullptr,
                            {d_out, cap, d_count});
}

int hvd_dev_vpdq_match_videos_cross_weighted(const void* d_img_q, int64_t nq, const void* d_video_q, const void* d_excl_q,
                                             const void* d_weight_q, const void* d_img_t, int64_t nt, const void* d_video_t,
                                             const void* d_excl_t, const void* d_weight_t, int max_weight, int max_dist,
                                             void* d_out, int64_t cap, void* d_count) {
    const DevSide t{d_img_t, nt, d_video_t, d_excl_t, d_weight_t};
    return vmatch_dev_entry(VmCall::with_weights(max_dist, max_weight, false), {d_img_q, nq, d_video_q, d_excl_q, d_weight_q}, &t,
                            {d_out, cap, d_count});
}

// (the two host forms refuse every bad argument before the question whether a device is there: VmCall::args_first)
int hvd_vpdq_match_videos_weighted(const uint8_t* frames, const int64_t* offsets, int64_t V, const int32_t* weights, int max_weight,
                                   int max_dist, hvd_vmatch* out, int64_t cap, int64_t* out_count, int64_t* out_totals) {
    return vmatch_from_host(VmCall::with_weights(max_dist, max_weight, true), {frames, offsets, V, nullptr, weights, out_totals}, nullptr,
                            {out, cap, out_count});
}

int hvd_vpdq_match_videos_cross_weighted(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* ids_q,
                                         const int32_t* weights_q, const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT,
                                         const int32_t* ids_t, const int32_t* weights_t, int max_weight, int max_dist,
                                         hvd_vmatch* out, int64_t cap, int64_t* out_count, int64_t* out_totals_q,
                                         int64_t* out_totals_t) {
    HostSide t{frames_t, offsets_t, VT, ids_t, weights_t, out_totals_t};
    return vmatch_from_host(VmCall::with_weights(max_dist, max_weight, true), {frames_q, offsets_q, VQ, ids_q, weights_q, out_totals_q}, &t,
                            {out, cap, out_count});
}

/* ---- time alignment of listed video pairs (k_valign*.hip) ---- */

int hvd_dev_kept_positions(const void* d_quality, int64_t n, const void* d_offsets, int64_t V, int min_quality, void* d_out_pos) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || V < 0 || n >= (1ll << 32) - 1 || V >= (1ll << 31) || !d_offsets) return fail(HVD_ERR_ARG, "bad arguments");
    if (n > 0 && (!d_quality || !d_out_pos)) return fail(HVD_ERR_ARG, "NULL device pointer");
    if (n > 0 && V == 0) return fail(HVD_ERR_ARG, "n=%lld frames in no video", (long long)n);
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    void* d_scr = nullptr;
    unsigned long long* d_counters = nullptr;
    SCR(S_COMPACT, hvd::compact_scratch_bytes((unsigned long long)n), d_scr);
    SCR(S_COUNTERS, 64, d_counters);
    HIP_TRY(hvd::launch_kept_positions((const int32_t*)d_quality, (unsigned long long)n, (const long long*)d_offsets, (uint32_t)V,
                                       min_quality, (int32_t*)d_out_pos, d_scr, d_counters + 2, g.stream));
    return HVD_OK;
}

/* ---- common-frame filter: rule and position gather (k_spread.hip) ---- */

int hvd_dev_common_frames(const void* d_spread, const void* d_offsets, int64_t V, int64_t n, int max_videos, int max_share,
                          void* d_out_keep) {
    if (int rc = need_ready()) return rc;
    if (max_videos < 0) return fail(HVD_ERR_ARG, "max_videos=%d must not be negative", max_videos);
    if (max_share < 0 || max_share > 100) return fail(HVD_ERR_ARG, "max_share=%d out of range [0,100] (per cent)", max_share);
    if (n < 0 || V < 0 || n >= (1ll << 32) - 1 || V >= (1ll << 31) || !d_offsets) return fail(HVD_ERR_ARG, "bad arguments");
    if (n > 0 && (!d_spread || !d_out_keep)) return fail(HVD_ERR_ARG, "NULL device pointer");
    if (n > 0 && V == 0) return fail(HVD_ERR_ARG, "n=%lld frames in no video", (long long)n);
    HIP_TRY(hvd::launch_common_rule((const int32_t*)d_spread, (const long long*)d_offsets, (uint32_t)V, (unsigned long long)n,
                                    max_videos, max_share, (int32_t*)d_out_keep, g.stream));
    return HVD_OK;
}

int hvd_dev_gather_kept_i32(const void* d_in, const void* d_keep, int64_t n, void* d_out) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || n >= (1ll << 32) - 1) return fail(HVD_ERR_ARG, "n=%lld out of range", (long long)n);
    if (n > 0 && (!d_in || !d_keep || !d_out)) return fail(HVD_ERR_ARG, "NULL device pointer");
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    void* d_scr = nullptr;
    unsigned long long* d_counters = nullptr;
    SCR(S_COMPACT, hvd::compact_scratch_bytes((unsigned long long)n), d_scr);
    SCR(S_COUNTERS, 64, d_counters);
    HIP_TRY(hvd::launch_gather_kept_i32((const int32_t*)d_in, (const int32_t*)d_keep, (unsigned long long)n, (int32_t*)d_out, d_scr,
                                        d_counters + 2, g.stream));
    return HVD_OK;
}

/* ---- static-scene filter: one keyframe per run of near-identical frames (k_runs.hip) ---- */

static int check_run_rule(int max_dist, int max_run) {
    if (max_dist < 0 || max_dist >= 128) return fail(HVD_ERR_ARG, "max_dist=%d out of range [0,127]", max_dist);
    if (max_run < 0 || max_run > (1 << 20)) return fail(HVD_ERR_ARG, "max_run=%d out of range [0,2^20] (0 = no limit)", max_run);
    return HVD_OK;
}

int hvd_dev_frame_runs(const void* d_hashes, const void* d_offsets, int64_t V, int64_t n, int max_dist, int max_run,
                       void* d_out_keep, void* d_out_run) {
    if (int rc = check_run_rule(max_dist, max_run)) return rc;
    if (n < 0 || V < 0 || n >= (1ll << 32) - 1 || V >= (1ll << 31) || !d_offsets) return fail(HVD_ERR_ARG, "bad arguments");
    if (n > 0 && (!d_hashes || !d_out_keep)) return fail(HVD_ERR_ARG, "NULL device pointer");
    if (n > 0 && V == 0) return fail(HVD_ERR_ARG, "n=%lld frames in no video", (long long)n);
    if (int rc = need_ready()) return rc;
    HIP_TRY(hvd::launch_frame_runs(d_hashes, (const long long*)d_offsets, (uint32_t)V, (unsigned long long)n, max_dist, max_run,
                                   (int32_t*)d_out_keep, (int32_t*)d_out_run, g.stream));
    return HVD_OK;
}

int hvd_vpdq_frame_runs(const uint8_t* frames, const int64_t* offsets, int64_t V, int max_dist, int max_run, int32_t* out_keep,
                        int32_t* out_run) {
    // every refusal comes before the question whether a device is there
    if (int rc = check_run_rule(max_dist, max_run)) return rc;
    int64_t nf = 0;
    if (int rc = check_offsets(offsets, V, &nf)) return rc;
    if (nf > 0 && !frames) return fail(HVD_ERR_ARG, "frames is NULL");
    if (nf > 0 && !out_keep) return fail(HVD_ERR_ARG, "out_keep is NULL");
    if (int rc = need_ready()) return rc;
    if (nf == 0) return HVD_OK;
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    void* d_db = nullptr;
    long long* d_off = nullptr;
    int32_t* d_keep = nullptr;
    SCR(S_DB, 32 * (size_t)nf, d_db);
    SCR(S_OFF, 8 * (size_t)(V + 1), d_off);
    SCR(S_SPREAD, 8 * (size_t)nf, d_keep);  // keep flags, then the run words
    int32_t* d_run = out_run ? d_keep + nf : nullptr;
    HIP_TRY(hipMemcpyAsync(d_db, frames, 32 * (size_t)nf, hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipMemcpyAsync(d_off, offsets, 8 * (size_t)(V + 1), hipMemcpyHostToDevice, g.stream));
    if (int rc = hvd_dev_frame_runs(d_db, d_off, V, nf, max_dist, max_run, d_keep, d_run)) return rc;
    HIP_TRY(hipMemcpyAsync(out_keep, d_keep, 4 * (size_t)nf, hipMemcpyDeviceToHost, g.stream));
    if (out_run) HIP_TRY(hipMemcpyAsync(out_run, d_run, 4 * (size_t)nf, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

/* ---- time alignment of listed pairs (k_valign*.hip): hvd::AlignMode says which of the four a call is ---- */

using hvd::AlignMode;
using hvd::AlignOperands;

static int scratch_bytes_entry(const AlignMode& mode, int64_t max_bins, size_t* out_bytes) {
    if (!out_bytes || max_bins < 0 || max_bins > (1ll << 20)) return fail(HVD_ERR_ARG, "max_bins=%lld: need 0..2^20", (long long)max_bins);
    *out_bytes = hvd::alignment_scratch_bytes(mode, (unsigned long long)max_bins);
    return HVD_OK;
}

int hvd_align_scratch_bytes(int64_t max_bins, size_t* out_bytes) { return scratch_bytes_entry(AlignMode::of(false, false), max_bins, out_bytes); }
int hvd_segments_scratch_bytes(int64_t max_bins, size_t* out_bytes) { return scratch_bytes_entry(AlignMode::of(false, true), max_bins, out_bytes); }
int hvd_rates_scratch_bytes(int64_t max_bins, size_t* out_bytes) { return scratch_bytes_entry(AlignMode::of(true, false), max_bins, out_bytes); }
int hvd_rate_segments_scratch_bytes(int64_t max_bins, size_t* out_bytes) { return scratch_bytes_entry(AlignMode::of(true, true), max_bins, out_bytes); }
int hvd_signed_scratch_bytes(int64_t max_bins, size_t* out_bytes) { return scratch_bytes_entry(AlignMode::of_signed(0, 1), max_bins, out_bytes); }
int hvd_loops_scratch_bytes(int64_t max_bins, size_t* out_bytes) { return scratch_bytes_entry(AlignMode::of_loops(1, 1), max_bins, out_bytes); }

static int check_tolerances(int max_dist, int slack) {
    if (max_dist < 0 || max_dist >= 128) return fail(HVD_ERR_ARG, "max_dist=%d out of range [0,127]", max_dist);
    if (slack < 0 || slack > 16) return fail(HVD_ERR_ARG, "slack=%d out of range [0,16]", slack);
    return HVD_OK;
}

// (a loops mode carries max_rounds in max_segments: its limit is HVD_ALIGN_MAX_ROUNDS)
static int check_segment_limits(const AlignMode& mode) {
    const int max_segments = mode.max_segments, min_band_votes = mode.min_band_votes;
    if (mode.loops && (max_segments < 1 || max_segments > HVD_ALIGN_MAX_ROUNDS))
        return fail(HVD_ERR_ARG, "max_rounds=%d out of range [1,%d]", max_segments, HVD_ALIGN_MAX_ROUNDS);
    if (!mode.loops && (max_segments < 1 || max_segments > HVD_ALIGN_MAX_SEGMENTS))
        return fail(HVD_ERR_ARG, "max_segments=%d out of range [1,%d]", max_segments, HVD_ALIGN_MAX_SEGMENTS);
    if (min_band_votes < 1) return fail(HVD_ERR_ARG, "min_band_votes=%d: need >= 1", min_band_votes);
    return HVD_OK;
}

// The device entries: the checks in the order their errors are reported, then the mode's launches. rates / n_rates: the
// list as the caller gave it (rated modes); a broken one travels as (0, 0), the kernel's INT32_MIN records.
static int align_on_device(AlignMode mode, const int32_t* rates, int n_rates, const AlignOperands& op) {
    if (int rc = need_ready()) return rc;
    if (op.VQ < 0 || op.VT < 0 || op.VQ >= (1ll << 31) || op.VT >= (1ll << 31) || op.M < 0) return fail(HVD_ERR_ARG, "bad counts");
    if (int rc = check_tolerances(op.max_dist, op.slack)) return rc;
    if (mode.rated && (!rates || n_rates < 0)) return fail(HVD_ERR_ARG, "rates is NULL or n_rates=%d < 0", n_rates);
    if (mode.segmented)
        if (int rc = check_segment_limits(mode)) return rc;
    if (op.M == 0) return HVD_OK;
    if (!op.offsets_q || !op.offsets_t || !op.pairs || !op.out) return fail(HVD_ERR_ARG, "NULL device pointer");
    // what is read or written 16 bytes at a time: the hashes, the bit words, and the records where the kernel zeroes them so
    const uintptr_t aligned16 = (uintptr_t)op.hashes_q | (uintptr_t)op.hashes_t | (uintptr_t)op.scratch | (mode.records16() ? (uintptr_t)op.out : 0u);
    if (aligned16 & 15u)
        return fail(HVD_ERR_ARG, "%s must be 16-byte aligned", mode.records16() ? "hashes, scratch and records" : "hashes and scratch");
    if (mode.signed_)
        hvd::pack_signed_rate_list(rates, n_rates, &mode.nums, &mode.dens, &mode.revs);
    else if (mode.rated)
        hvd::pack_rate_list(rates, n_rates, &mode.nums, &mode.dens);
    HIP_TRY(hvd::launch_alignment(mode, op, g.stream));
    return HVD_OK;
}

int hvd_dev_vpdq_align_videos(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                              const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                              const void* d_pairs, int64_t M, int max_dist, int slack, void* d_scratch, size_t scratch_bytes,
                              void* d_out) {
    return align_on_device(AlignMode::of(false, false), nullptr, 0,
                           {d_hashes_q, d_offsets_q, VQ, d_pos_q, d_hashes_t, d_offsets_t, VT, d_pos_t, d_pairs, M, max_dist, slack,
                            d_scratch, scratch_bytes, d_out});
}

int hvd_dev_vpdq_align_segments(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                                const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                                const void* d_pairs, int64_t M, int max_dist, int slack, int max_segments, int min_band_votes,
                                void* d_scratch, size_t scratch_bytes, void* d_out) {
    return align_on_device(AlignMode::of(false, true, max_segments, min_band_votes), nullptr, 0,
                           {d_hashes_q, d_offsets_q, VQ, d_pos_q, d_hashes_t, d_offsets_t, VT, d_pos_t, d_pairs, M, max_dist, slack,
                            d_scratch, scratch_bytes, d_out});
}

int hvd_dev_vpdq_align_rates(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                             const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                             const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                             void* d_scratch, size_t scratch_bytes, void* d_out) {
    return align_on_device(AlignMode::of(true, false), rates, n_rates,
                           {d_hashes_q, d_offsets_q, VQ, d_pos_q, d_hashes_t, d_offsets_t, VT, d_pos_t, d_pairs, M, max_dist, slack,
                            d_scratch, scratch_bytes, d_out});
}

int hvd_dev_vpdq_align_rate_segments(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                                     const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                                     const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                                     int max_segments, int min_band_votes, void* d_scratch, size_t scratch_bytes, void* d_out) {
    return align_on_device(AlignMode::of(true, true, max_segments, min_band_votes), rates, n_rates,
                           {d_hashes_q, d_offsets_q, VQ, d_pos_q, d_hashes_t, d_offsets_t, VT, d_pos_t, d_pairs, M, max_dist, slack,
                            d_scratch, scratch_bytes, d_out});
}

int hvd_dev_vpdq_align_signed(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                              const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                              const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                              int max_segments, int min_band_votes, void* d_scratch, size_t scratch_bytes, void* d_out) {
    return align_on_device(AlignMode::of_signed(max_segments, min_band_votes), rates, n_rates,
                           {d_hashes_q, d_offsets_q, VQ, d_pos_q, d_hashes_t, d_offsets_t, VT, d_pos_t, d_pairs, M, max_dist, slack,
                            d_scratch, scratch_bytes, d_out});
}

int hvd_dev_vpdq_align_loops(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                             const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                             const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                             int max_rounds, int min_band_votes, void* d_scratch, size_t scratch_bytes, void* d_out) {
    return align_on_device(AlignMode::of_loops(max_rounds, min_band_votes), rates, n_rates,
                           {d_hashes_q, d_offsets_q, VQ, d_pos_q, d_hashes_t, d_offsets_t, VT, d_pos_t, d_pairs, M, max_dist, slack,
                            d_scratch, scratch_bytes, d_out});
}

// positions of one library: non-negative, strictly increasing inside a video, below 2^20
static int check_positions(const int32_t* pos, const int64_t* offsets, int64_t V, const char* side) {
    if (!pos) return HVD_OK;
    for (int64_t v = 0; v < V; ++v)
        for (int64_t f = offsets[v]; f < offsets[v + 1]; ++f)
            if (pos[f] < 0 || pos[f] >= (1 << 20) || (f > offsets[v] && pos[f] <= pos[f - 1]))
                return fail(HVD_ERR_ARG, "%s positions: frame %lld of video %lld is %d (need >= 0, strictly increasing inside a "
                            "video, below 2^20)", side, (long long)(f - offsets[v]), (long long)v, pos[f]);
    return HVD_OK;
}

// The host-buffer form of the alignments: validate, stage, run, copy the records back. h: the operands as host buffers (no
// scratch). Two steps that hvd_vpdq_cover_videos takes as well. align_check: the list and the limits are judged first; a rated
// mode then judges the other arguments before the library's state, so that a bad call is HVD_ERR_ARG with or without a device,
// the slope-one modes after it (mode.args_first). -> the frames of either library and the largest bins of any pair.
static int align_check(AlignMode& mode, const int32_t* rates, int n_rates, const AlignOperands& h, int64_t* nq_out, int64_t* nt_out,
                       int64_t* max_bins_out) {
    if (mode.signed_ && !hvd::pack_signed_rate_list(rates, n_rates, &mode.nums, &mode.dens, &mode.revs))
        return fail(HVD_ERR_ARG, "rates: need 1..%d pairs (num, den) with 1 <= |num|, den <= 8, no common factor, none listed twice "
                    "with one sign", HVD_ALIGN_MAX_RATES);
    if (mode.rated && !mode.signed_ && !hvd::pack_rate_list(rates, n_rates, &mode.nums, &mode.dens))
        return fail(HVD_ERR_ARG, "rates: need 1..%d pairs (num, den) with 1 <= num, den <= 8, no common factor, none listed twice",
                    HVD_ALIGN_MAX_RATES);
    if (mode.segmented)
        if (int rc = check_segment_limits(mode)) return rc;
    if (!mode.args_first)
        if (int rc = need_ready()) return rc;
    const auto *offsets_q = (const int64_t*)h.offsets_q, *offsets_t = (const int64_t*)h.offsets_t;
    const auto *positions_q = (const int32_t*)h.pos_q, *positions_t = (const int32_t*)h.pos_t;
    const auto* pairs = (const uint32_t*)h.pairs;
    const int64_t VQ = h.VQ, VT = h.VT, M = h.M;
    if (M < 0 || (M > 0 && (!pairs || !h.out))) return fail(HVD_ERR_ARG, "bad pair list / output buffer");
    if (int rc = check_tolerances(h.max_dist, h.slack)) return rc;
    int64_t nq = 0, nt = 0;
    if (int rc = check_offsets(offsets_q, VQ, &nq)) return rc;
    if (int rc = check_offsets(offsets_t, VT, &nt)) return rc;
    if ((nq > 0 && !h.hashes_q) || (nt > 0 && !h.hashes_t)) return fail(HVD_ERR_ARG, "frames is NULL");
    if (int rc = check_positions(positions_q, offsets_q, VQ, "query")) return rc;
    if (int rc = check_positions(positions_t, offsets_t, VT, "target")) return rc;
    auto span = [](const int32_t* pos, const int64_t* off, int64_t v) -> int64_t {
        const int64_t n = off[v + 1] - off[v];
        return n == 0 ? -1 : pos ? (int64_t)pos[off[v + 1] - 1] - pos[off[v]] : n - 1;
    };
    int64_t max_bins = 0;
    for (int64_t p = 0; p < M; ++p) {
        const uint32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        if ((int64_t)a >= VQ || (int64_t)b >= VT)
            return fail(HVD_ERR_ARG, "pair %lld = (%u, %u) is outside the %lld x %lld videos", (long long)p, a, b, (long long)VQ, (long long)VT);
        const int64_t sa = span(positions_q, offsets_q, a), sb = span(positions_t, offsets_t, b);
        if (sa < 0 || sb < 0) continue;  // an empty video: the zero record
        int64_t bins = sa + sb + 1 + 2 * (int64_t)h.slack;
        for (int r = 0; r < n_rates; ++r) {  // the largest bins_r of the list (|num|: a signed list may hold negative ones)
            const int64_t num = std::abs((int64_t)rates[2 * r]), den = rates[2 * r + 1];
            bins = std::max(bins, num * sa + den * sb + 1 + 2 * (int64_t)h.slack * std::max(num, den));
        }
        if (bins > (1ll << 20))
            return fail(HVD_ERR_ARG, "pair %lld = (%u, %u) spans %lld offsets with slack %d: more than the 2^20 histogram bins",
                        (long long)p, a, b, (long long)bins, h.slack);
        max_bins = std::max(max_bins, bins);
    }
    if (mode.args_first)
        if (int rc = need_ready()) return rc;
    *nq_out = nq;
    *nt_out = nt;
    *max_bins_out = max_bins;
    return HVD_OK;
}

// the libraries of an alignment on the device: hashes, CSR offsets, positions or nullptr, per side
struct AlignStaged {
    void *d_hq = nullptr, *d_ht = nullptr;
    long long *d_oq = nullptr, *d_ot = nullptr;
    int32_t *d_pq = nullptr, *d_pt = nullptr;
};

// align_upload: the libraries of h (nq, nt frames) into the library's slots, one upload when both sides are one library. The
// caller holds g.h_mu.
static int align_upload(const AlignOperands& h, int64_t nq, int64_t nt, AlignStaged* st) {
    const auto *offsets_q = (const int64_t*)h.offsets_q, *offsets_t = (const int64_t*)h.offsets_t;
    const auto *positions_q = (const int32_t*)h.pos_q, *positions_t = (const int32_t*)h.pos_t;
    const int64_t VQ = h.VQ, VT = h.VT;
    const bool self = h.hashes_t == h.hashes_q && offsets_t == offsets_q && positions_t == positions_q && VT == VQ;
    auto upload = [&](const void* frames, const int64_t* offsets, int64_t V, int64_t n, const int32_t* pos, Ctx::Scr s_db,
                      Ctx::Scr s_off, Ctx::Scr s_pos, void** d_h, long long** d_o, int32_t** d_p) -> int {
        if (int rc = scratch(s_db, 32 * (size_t)n, d_h)) return rc;
        if (int rc = scratch(s_off, 8 * (size_t)(V + 1), (void**)d_o)) return rc;
        if (n > 0) HIP_TRY(hipMemcpyAsync(*d_h, frames, 32 * (size_t)n, hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(*d_o, offsets, 8 * (size_t)(V + 1), hipMemcpyHostToDevice, g.stream));
        if (pos && n > 0) {
            if (int rc = scratch(s_pos, 4 * (size_t)n, (void**)d_p)) return rc;
            HIP_TRY(hipMemcpyAsync(*d_p, pos, 4 * (size_t)n, hipMemcpyHostToDevice, g.stream));
        }
        return HVD_OK;
    };
    if (int rc = upload(h.hashes_q, offsets_q, VQ, nq, positions_q, Ctx::S_DB, Ctx::S_OFF, Ctx::S_POSQ, &st->d_hq, &st->d_oq, &st->d_pq)) return rc;
    if (self) {
        st->d_ht = st->d_hq;
        st->d_ot = st->d_oq;
        st->d_pt = st->d_pq;
        return HVD_OK;
    }
    return upload(h.hashes_t, offsets_t, VT, nt, positions_t, Ctx::S_DB2, Ctx::S_OFF2, Ctx::S_POST, &st->d_ht, &st->d_ot, &st->d_pt);
}

static int align_from_host(AlignMode mode, const int32_t* rates, int n_rates, const AlignOperands& h) {
    int64_t nq = 0, nt = 0, max_bins = 0;
    if (int rc = align_check(mode, rates, n_rates, h, &nq, &nt, &max_bins)) return rc;
    const int64_t M = h.M;
    if (M == 0) return HVD_OK;
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    AlignStaged st;
    if (int rc = align_upload(h, nq, nt, &st)) return rc;
    void *d_scr = nullptr, *d_pairs = nullptr, *d_out = nullptr;
    SCR(S_APAIRS, 8 * (size_t)M, d_pairs);
    const size_t out_bytes = mode.record_bytes() * (size_t)M;
    SCR(S_AOUT, out_bytes, d_out);
    const size_t sb = hvd::alignment_scratch_bytes(mode, (unsigned long long)max_bins);
    if (sb) SCR(S_ASCR, sb, d_scr);
    HIP_TRY(hipMemcpyAsync(d_pairs, h.pairs, 8 * (size_t)M, hipMemcpyHostToDevice, g.stream));
    if (int rc = align_on_device(mode, rates, n_rates, {st.d_hq, st.d_oq, h.VQ, st.d_pq, st.d_ht, st.d_ot, h.VT, st.d_pt, d_pairs, M, h.max_dist,
                                                        h.slack, d_scr, sb, d_out}))
        return rc;
    HIP_TRY(hipMemcpyAsync(h.out, d_out, out_bytes, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

int hvd_vpdq_align_videos(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                          const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                          const uint32_t* pairs, int64_t M, int max_dist, int slack, hvd_valign* out) {
    return align_from_host(AlignMode::of(false, false), nullptr, 0,
                           {frames_q, offsets_q, VQ, positions_q, frames_t, offsets_t, VT, positions_t, pairs, M, max_dist, slack, nullptr, 0, out});
}

int hvd_vpdq_align_segments(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                            const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                            const uint32_t* pairs, int64_t M, int max_dist, int slack, int max_segments, int min_band_votes,
                            hvd_vsegments* out) {
    return align_from_host(AlignMode::of(false, true, max_segments, min_band_votes), nullptr, 0,
                           {frames_q, offsets_q, VQ, positions_q, frames_t, offsets_t, VT, positions_t, pairs, M, max_dist, slack, nullptr, 0, out});
}

int hvd_vpdq_align_rates(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                         const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                         const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                         hvd_vrate* out) {
    return align_from_host(AlignMode::of(true, false), rates, n_rates,
                           {frames_q, offsets_q, VQ, positions_q, frames_t, offsets_t, VT, positions_t, pairs, M, max_dist, slack, nullptr, 0, out});
}

int hvd_vpdq_align_rate_segments(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                                 const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                                 const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                                 int max_segments, int min_band_votes, hvd_vrsegments* out) {
    return align_from_host(AlignMode::of(true, true, max_segments, min_band_votes), rates, n_rates,
                           {frames_q, offsets_q, VQ, positions_q, frames_t, offsets_t, VT, positions_t, pairs, M, max_dist, slack, nullptr, 0, out});
}

int hvd_vpdq_align_signed(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                          const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                          const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                          int max_segments, int min_band_votes, hvd_vssegments* out) {
    return align_from_host(AlignMode::of_signed(max_segments, min_band_votes), rates, n_rates,
                           {frames_q, offsets_q, VQ, positions_q, frames_t, offsets_t, VT, positions_t, pairs, M, max_dist, slack, nullptr, 0, out});
}

int hvd_vpdq_align_loops(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                         const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                         const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                         int max_rounds, int min_band_votes, hvd_vloops* out) {
    return align_from_host(AlignMode::of_loops(max_rounds, min_band_votes), rates, n_rates,
                           {frames_q, offsets_q, VQ, positions_q, frames_t, offsets_t, VT, positions_t, pairs, M, max_dist, slack, nullptr, 0, out});
}

/* ---- coverage of a video by several others (k_valign_cover.hip): the slope-one alignment with a second output ---- */

static int check_cover_floor(int min_aligned) {
    if (min_aligned < 1) return fail(HVD_ERR_ARG, "min_aligned=%d: need >= 1", min_aligned);
    return HVD_OK;
}

int hvd_cover_scratch_bytes(int64_t n_frames, int64_t max_bins, size_t* out_bytes) {
    if (!out_bytes) return fail(HVD_ERR_ARG, "out_bytes is NULL");
    if (max_bins < 0 || max_bins > (1ll << 20)) return fail(HVD_ERR_ARG, "max_bins=%lld: need 0..2^20", (long long)max_bins);
    if (n_frames < 0 || n_frames >= (1ll << 32) - 1) return fail(HVD_ERR_ARG, "n_frames=%lld out of range", (long long)n_frames);
    *out_bytes = hvd::cover_scratch_bytes((unsigned long long)n_frames, (unsigned long long)max_bins);
    return HVD_OK;
}

int hvd_dev_vpdq_cover_videos(const void* d_hashes, const void* d_offsets, int64_t V, int64_t n_frames, const void* d_pos,
                              const void* d_pairs, int64_t M, int max_dist, int slack, int min_aligned, void* d_scratch,
                              size_t scratch_bytes, void* d_out_align, void* d_out_cover) {
    if (int rc = need_ready()) return rc;
    if (V < 0 || V >= (1ll << 31) || M < 0) return fail(HVD_ERR_ARG, "bad counts");
    if (n_frames < 0 || n_frames >= (1ll << 32) - 1) return fail(HVD_ERR_ARG, "n_frames=%lld out of range", (long long)n_frames);
    if (int rc = check_tolerances(max_dist, slack)) return rc;
    if (int rc = check_cover_floor(min_aligned)) return rc;
    if (V == 0 && M == 0) return HVD_OK;
    if (!d_offsets || (M > 0 && (!d_pairs || !d_out_align)) || (V > 0 && !d_out_cover)) return fail(HVD_ERR_ARG, "NULL device pointer");
    const size_t bitmap_bytes = hvd::cover_bitmap_bytes((unsigned long long)n_frames);
    if (scratch_bytes < bitmap_bytes || (bitmap_bytes && !d_scratch))
        return fail(HVD_ERR_ARG, "scratch of %zu bytes: the bitmap over %lld frames needs %zu (hvd_cover_scratch_bytes)", scratch_bytes,
                    (long long)n_frames, bitmap_bytes);
    if (((uintptr_t)d_hashes | (uintptr_t)d_scratch | (uintptr_t)d_out_cover) & 15u)
        return fail(HVD_ERR_ARG, "hashes, scratch and cover records must be 16-byte aligned");
    HIP_TRY(hvd::launch_valign_cover({{d_hashes, d_offsets, V, d_pos, d_hashes, d_offsets, V, d_pos, d_pairs, M, max_dist, slack, d_scratch,
                                       scratch_bytes, d_out_align},
                                      n_frames, min_aligned, d_out_cover},
                                     g.stream));
    return HVD_OK;
}

int hvd_vpdq_cover_videos(const uint8_t* frames, const int64_t* offsets, int64_t V, const int32_t* positions, const uint32_t* pairs,
                          int64_t M, int max_dist, int slack, int min_aligned, hvd_valign* out_align, hvd_vcover* out_cover) {
    // every refusal comes before the question whether a device is there (as the rate entries: args_first); the checks and the
    // upload are the alignment's, on one library
    if (int rc = check_cover_floor(min_aligned)) return rc;
    if (V > 0 && !out_cover) return fail(HVD_ERR_ARG, "out_cover is NULL");
    AlignMode mode = AlignMode::of(false, false);
    mode.args_first = true;
    const AlignOperands h = {frames, offsets, V, positions, frames, offsets, V, positions, pairs, M, max_dist, slack, nullptr, 0, out_align};
    int64_t nf = 0, nt = 0, max_bins = 0;
    if (int rc = align_check(mode, nullptr, 0, h, &nf, &nt, &max_bins)) return rc;
    if (V == 0) return HVD_OK;
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    AlignStaged st;
    if (int rc = align_upload(h, nf, nt, &st)) return rc;
    // the alignment records, then (16-byte aligned: a record is 48 bytes) the cover records, in one slot
    void *d_scr = nullptr, *d_pairs = nullptr, *d_out = nullptr;
    const size_t align_bytes = sizeof(hvd_valign) * (size_t)M, cover_bytes = sizeof(hvd_vcover) * (size_t)V;
    SCR(S_APAIRS, 8 * (size_t)M, d_pairs);
    SCR(S_AOUT, align_bytes + cover_bytes, d_out);
    void* const d_cover = (char*)d_out + align_bytes;
    const size_t sb = hvd::cover_scratch_bytes((unsigned long long)nf, (unsigned long long)max_bins);
    if (sb) SCR(S_ASCR, sb, d_scr);
    if (M > 0) HIP_TRY(hipMemcpyAsync(d_pairs, pairs, 8 * (size_t)M, hipMemcpyHostToDevice, g.stream));
    if (int rc = hvd_dev_vpdq_cover_videos(st.d_hq, st.d_oq, V, nf, st.d_pq, d_pairs, M, max_dist, slack, min_aligned, d_scr, sb, d_out, d_cover))
        return rc;
    if (M > 0) HIP_TRY(hipMemcpyAsync(out_align, d_out, align_bytes, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipMemcpyAsync(out_cover, d_cover, cover_bytes, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

/* ---- duplicate groups with a keeper: connected components of a pair list (k_group.hip) ---- */

static int check_group_shape(int64_t n_records, int kind, const void* lengths, int threshold, int64_t V) {
    if (V < 1 || V >= (1ll << 31)) return fail(HVD_ERR_ARG, "V=%lld out of range [1,2^31)", (long long)V);
    if (n_records < 0 || n_records >= (1ll << 32)) return fail(HVD_ERR_ARG, "%lld records: need 0..2^32-1", (long long)n_records);
    if (kind != HVD_EDGES_ALL && kind != HVD_EDGES_VMATCH) return fail(HVD_ERR_ARG, "kind=%d: need HVD_EDGES_ALL or HVD_EDGES_VMATCH", kind);
    if (kind == HVD_EDGES_VMATCH) {
        if (!lengths) return fail(HVD_ERR_ARG, "HVD_EDGES_VMATCH needs the lengths");
        if (threshold < 1 || threshold > 100) return fail(HVD_ERR_ARG, "threshold=%d out of range [1,100]", threshold);
    }
    return HVD_OK;
}

static int group_scratch_entry(bool keeper_first, int64_t V, size_t* out_bytes) {
    if (!out_bytes || V < 1 || V >= (1ll << 31)) return fail(HVD_ERR_ARG, "V=%lld out of range [1,2^31)", (long long)V);
    *out_bytes = keeper_first ? hvd::keeper_scratch_bytes((unsigned long long)V) : hvd::group_scratch_bytes((unsigned long long)V);
    return HVD_OK;
}

int hvd_group_scratch_bytes(int64_t V, size_t* out_bytes) { return group_scratch_entry(false, V, out_bytes); }
int hvd_keeper_scratch_bytes(int64_t V, size_t* out_bytes) { return group_scratch_entry(true, V, out_bytes); }

// The device form of both groupings: the checks, then the launches of k_group.hip, or of k_keeper.hip
// (keeper_first; out_rounds may be nullptr) with the answer to rounds that did not settle.
static int group_on_device(bool keeper_first, const hvd::EdgeList& edges, const hvd::GroupsOut& out, int64_t* out_rounds) {
    if (int rc = need_ready()) return rc;
    if (int rc = check_group_shape(edges.n_records, edges.kind, edges.d_lengths, edges.T, edges.V)) return rc;
    if (!out.scratch || !out.node || !out.count || (edges.n_records > 0 && !edges.records) || out.cap < 0 || (out.cap > 0 && !out.groups))
        return fail(HVD_ERR_ARG, "NULL device pointer / bad cap");
    if ((((uintptr_t)edges.records | (uintptr_t)out.groups) & 15u) ||
        (((uintptr_t)out.scratch | (uintptr_t)out.count | (uintptr_t)edges.d_record_count) & 7u))
        return fail(HVD_ERR_ARG, "records and groups must be 16-byte aligned, scratch and counts 8-byte aligned");
    if (!keeper_first) {
        HIP_TRY(hvd::launch_group_edges(edges, out, g.stream));
        return HVD_OK;
    }
    bool settled = false;
    long long rounds = 0;
    HIP_TRY(hvd::launch_keeper_groups(edges, out, g.stream, out_rounds ? &rounds : nullptr, &settled));
    if (!settled)
        return fail(HVD_ERR_STATE, "nodes left undecided after %lld rounds: every round decides one at least", (long long)edges.V);
    if (out_rounds) *out_rounds = (int64_t)rounds;
    return HVD_OK;
}

int hvd_dev_group_edges(const void* d_records, int64_t n_records, const void* d_record_count, int kind, const void* d_lengths,
                        int threshold, int policy_is_min, int64_t V, const void* d_score, void* d_scratch, void* d_out_label,
                        void* d_out_groups, int64_t cap, void* d_out_count) {
    return group_on_device(false, {d_records, n_records, (const unsigned long long*)d_record_count, kind, (const long long*)d_lengths,
                                   threshold, policy_is_min != 0, V, (const uint32_t*)d_score},
                           {d_scratch, (int32_t*)d_out_label, (hvd_group*)d_out_groups, cap, (unsigned long long*)d_out_count}, nullptr);
}

/* ---- keeper-first duplicate groups: every member matches its keeper directly (k_keeper.hip) ---- */

int hvd_dev_keeper_groups(const void* d_records, int64_t n_records, const void* d_record_count, int kind, const void* d_lengths,
                          int threshold, int policy_is_min, int64_t V, const void* d_score, void* d_scratch, void* d_out_keeper,
                          void* d_out_groups, int64_t cap, void* d_out_count, int64_t* out_rounds) {
    return group_on_device(true, {d_records, n_records, (const unsigned long long*)d_record_count, kind, (const long long*)d_lengths,
                                  threshold, policy_is_min != 0, V, (const uint32_t*)d_score},
                           {d_scratch, (int32_t*)d_out_keeper, (hvd_group*)d_out_groups, cap, (unsigned long long*)d_out_count}, out_rounds);
}

// The host-array form of both groupings: everything is judged, the operands go up, the device entry runs, the node array and
// the group records come down. keeper_first: out_node = keeper_of, else the labels.
static int groups_from_host(bool keeper_first, const void* records, int64_t E, int kind, const int64_t* lengths, int threshold,
                            int policy_is_min, int64_t V, const uint32_t* score, int32_t* out_node, hvd_group* out_groups,
                            int64_t cap, int64_t* out_count, int64_t* out_rounds) {
    // the arguments are judged before the library's state is: a bad call is HVD_ERR_ARG with or without a device
    if (int rc = check_group_shape(E, kind, lengths, threshold, V)) return rc;
    if (!out_node || !out_count || (E > 0 && !records) || cap < 0 || (cap > 0 && !out_groups))
        return fail(HVD_ERR_ARG, "NULL pointer / bad cap");
    const uint32_t* w = (const uint32_t*)records;
    for (int64_t e = 0; e < E; ++e)
        if ((int64_t)w[4 * e] >= V || (int64_t)w[4 * e + 1] >= V || w[4 * e] == w[4 * e + 1])
            return fail(HVD_ERR_ARG, "record %lld = (%u, %u) is no edge between two of the %lld nodes", (long long)e, w[4 * e],
                        w[4 * e + 1], (long long)V);
    if (int rc = need_ready()) return rc;
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    void *d_rec = nullptr, *d_len = nullptr, *d_score = nullptr, *d_scr = nullptr, *d_node = nullptr;
    uint8_t* d_out = nullptr;  // the count, then the group records
    SCR(S_GSCR, keeper_first ? hvd::keeper_scratch_bytes((unsigned long long)V) : hvd::group_scratch_bytes((unsigned long long)V), d_scr);
    SCR(S_GLABEL, 4 * (size_t)V, d_node);
    SCR(S_GOUT, 16 + 16 * (size_t)cap, d_out);
    if (E > 0) {
        SCR(S_GREC, 16 * (size_t)E, d_rec);
        HIP_TRY(hipMemcpyAsync(d_rec, records, 16 * (size_t)E, hipMemcpyHostToDevice, g.stream));
    }
    if (kind == HVD_EDGES_VMATCH) {
        SCR(S_GLEN, 8 * (size_t)V, d_len);
        HIP_TRY(hipMemcpyAsync(d_len, lengths, 8 * (size_t)V, hipMemcpyHostToDevice, g.stream));
    }
    if (score) {
        SCR(S_GSCORE, 4 * (size_t)V, d_score);
        HIP_TRY(hipMemcpyAsync(d_score, score, 4 * (size_t)V, hipMemcpyHostToDevice, g.stream));
    }
    void* d_groups = cap > 0 ? d_out + 16 : nullptr;
    if (int rc = group_on_device(keeper_first, {d_rec, E, nullptr, kind, (const long long*)d_len, threshold, policy_is_min != 0, V,
                                                (const uint32_t*)d_score},
                                 {d_scr, (int32_t*)d_node, (hvd_group*)d_groups, cap, (unsigned long long*)d_out}, out_rounds))
        return rc;
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, d_out, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipMemcpyAsync(out_node, d_node, 4 * (size_t)V, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    const unsigned long long n_out = std::min(count, (unsigned long long)cap);
    if (n_out > 0) {
        HIP_TRY(hipMemcpyAsync(out_groups, d_out + 16, 16 * (size_t)n_out, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    *out_count = (int64_t)count;
    if (count > (unsigned long long)cap) return fail(HVD_ERR_OVERFLOW, "%llu groups, room for %lld", count, (long long)cap);
    return HVD_OK;
}

int hvd_group_edges(const void* records, int64_t E, int kind, const int64_t* lengths, int threshold, int policy_is_min, int64_t V,
                    const uint32_t* score, int32_t* out_label, hvd_group* out_groups, int64_t cap, int64_t* out_count) {
    return groups_from_host(false, records, E, kind, lengths, threshold, policy_is_min, V, score, out_label, out_groups, cap,
                            out_count, nullptr);
}

int hvd_keeper_groups(const void* records, int64_t E, int kind, const int64_t* lengths, int threshold, int policy_is_min, int64_t V,
                      const uint32_t* score, int32_t* out_keeper, hvd_group* out_groups, int64_t cap, int64_t* out_count,
                      int64_t* out_rounds) {
    return groups_from_host(true, records, E, kind, lengths, threshold, policy_is_min, V, score, out_keeper, out_groups, cap,
                            out_count, out_rounds);
}

#ifndef HVD_NO_BENCH_SYMBOLS
int hvd_dev_synth_video_frames(void* d_frames, int64_t v0, int64_t n_videos, int frames_per_video, uint64_t seed,
                               const void* d_copy_of) {
    if (int rc = need_ready()) return rc;
    if (v0 < 0 || n_videos < 0 || frames_per_video < 1 || n_videos * (int64_t)frames_per_video >= (1ll << 31))
        return fail(HVD_ERR_ARG, "bad synthetic library shape");
    if (n_videos == 0) return HVD_OK;
    if (!d_frames) return fail(HVD_ERR_ARG, "d_frames is NULL");
    HIP_TRY(hvd::launch_synth_frames64((uint8_t*)d_frames, v0, (uint32_t)frames_per_video,
                                       (unsigned long long)n_videos * (unsigned long long)frames_per_video, seed,
                                       (const int32_t*)d_copy_of, g.stream));
    return HVD_OK;
}

// The pieces of the video search's bit order, one at a time (include/hvd_mi355x_bench.h): the sample rule and the counting
// kernels as choose_bit_order runs them, its rule, the rewrite as vmatch_keys launches it, and packed_hashes' kernel.
int hvd_dev_bit_cooc(const void* d_bits, int64_t n, int force, void* d_cooc, uint32_t* sample, uint32_t* stride) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || n >= (1ll << 32) || !d_cooc || !sample || !stride || (n > 0 && !d_bits)) return fail(HVD_ERR_ARG, "bad arguments");
    std::lock_guard<std::recursive_mutex> lk(g.h_mu);
    const hvd::BitSample s = hvd::bit_order_sample((uint32_t)n, force != 0);
    *sample = s.sample;
    *stride = s.stride;
    if (!s.sample) return HVD_OK;
    if (int rc = count_bit_cooc(d_bits, s, d_cooc)) return rc;
    HIP_TRY(hipStreamSynchronize(g.stream));
    return HVD_OK;
}

int hvd_bit_order_from_cooc(const uint32_t* cooc, uint32_t sample, uint8_t* perm) {
    if (!cooc || !perm || sample == 0) return fail(HVD_ERR_ARG, "bad arguments");
    hvd::bit_order_from_cooc(cooc, sample, perm);
    return HVD_OK;
}

int hvd_dev_reorder_bits(const void* d_bits, int64_t n, const uint8_t* perm, void* d_bits_out, void* d_img) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || n >= (1ll << 32) || !perm || !d_img || (n > 0 && (!d_bits || !d_bits_out))) return fail(HVD_ERR_ARG, "bad arguments");
    bool seen[256] = {};
    for (int k = 0; k < 256; ++k) {
        if (seen[perm[k]]) return fail(HVD_ERR_ARG, "perm is not a permutation of 0..255: %d appears twice", (int)perm[k]);
        seen[perm[k]] = true;
    }
    HIP_TRY(hvd::launch_reorder_bits(d_bits, (uint32_t)n, perm, d_bits_out, d_img, g.stream));
    return HVD_OK;
}

int hvd_dev_pack_fp4(const void* d_img, int64_t n, void* d_bits) {
    if (int rc = need_ready()) return rc;
    if (n < 0 || n >= (1ll << 32) || (n > 0 && (!d_img || !d_bits))) return fail(HVD_ERR_ARG, "bad arguments");
    HIP_TRY(hvd::launch_pack_fp4(d_img, (uint32_t)n, d_bits, g.stream));
    return HVD_OK;
}

#endif  // HVD_NO_BENCH_SYMBOLS

}  // extern "C"
