// hvd_stream.cpp -- streaming frame hasher behind vpdq.VideoHasher (reference
// vpdqpy/vpdqpy.py:113-119): a decoder thread pushes frames one at a time; frames are
// staged in a ring of pinned batch slots; every slot owns a HIP stream on which its batch is
// uploaded (async H2D), hashed (PDQ kernels) and its 36 bytes per frame downloaded. Uploading
// batch k+1 overlaps hashing batch k; push() blocks only when every slot is still in flight,
// which bounds the staging memory like the reference's blocking frame queue
// (vpdqpy.py:115-117). A dihedral hasher (hvd_hasher_create_dihedral) runs the same ring through the dihedral kernel
// and downloads 8 x 32 bytes of hashes per frame.
// An autocrop hasher (hvd_hasher_create_autocrop) hashes inside the video's content rectangle, which is known only
// after the last frame: a batch is uploaded straight into a store of device blocks that keeps the whole video in HBM, and
// behind the upload, on the same stream, k_content_rect folds the batch into the hasher's one rectangle record (an order-free
// atomicMin / atomicMax merge: the slots' streams need no ordering among themselves). finish() closes the rectangle and
// sends every retained frame through the same slot ring once more, this time to be hashed under the rectangle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include <sched.h>

#include "copy_pool.h"
#include "hvd_hash_host.h"

namespace {

// Six slots of (by default) 32 MiB: a slot is refilled only when its previous batch has been hashed and read back, and the kernels
// of a small batch take ~0.25 ms whatever its size -- with three slots of 64 MiB the uploads of the two batches behind it did not
// always cover that (round 5: hash_frame(bytes) 16.9 -> 15.9 us per 512x512 frame, within 2 % of the zero-copy feed).
constexpr int kSlots = 6;

struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint8_t* h_frames = nullptr;   // pinned
    uint8_t* h_hashes = nullptr;   // pinned
    int32_t* h_quality = nullptr;  // pinned
    void* d_frames = nullptr;      // (an autocrop hasher has none: its batches go into the retained store)
    void* d_scratch = nullptr;
    void* d_hashes = nullptr;
    void* d_quality = nullptr;
    int64_t filled = 0;    // frames staged in h_frames
    int64_t in_flight = 0; // frames submitted and not yet collected
    bool results = true;   // ... whose hashes and qualities collect() takes (an autocrop upload has none)
};

// A block of the retained store of an autocrop hasher: frames [0, used) of cap, back to back. A batch never spans blocks.
struct Block {
    uint8_t* d = nullptr;
    int64_t cap = 0, used = 0;
};
constexpr int64_t kDefaultRetained = (int64_t)8 << 30;  // bytes of frames one video may keep in HBM (hvd_hasher_create_autocrop)

}  // namespace

namespace {
hvd::CopyPool g_copy_pool;  // (copy_pool.h)
// where the host side of the feed spends its time, process-wide, in nanoseconds (hvd_debug_get "hasher_ns_copy" / "_submit" /
// "_wait"; reading clears): the frame copies into the ring, the enqueue of a batch (H2D + kernels + D2H + event), the waits for
// a slot whose previous batch is still in flight. Three clock reads per frame (~60 ns).
std::atomic<long long> g_ns_copy{0}, g_ns_submit{0}, g_ns_wait{0};
struct NsScope {
    std::atomic<long long>& acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit NsScope(std::atomic<long long>& a) : acc(a) {}
    ~NsScope() { acc.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(), std::memory_order_relaxed); }
};
}  // namespace
namespace hvd {
long long stream_take_ns(int which) { return (which == 0 ? g_ns_copy : which == 1 ? g_ns_submit : g_ns_wait).exchange(0); }
}

#ifndef HVD_NO_BENCH_SYMBOLS
extern "C" int hvd_debug_parallel_copy(void* dst, const void* src, size_t n, int threads) {
    if ((!dst || !src) && n) return hvd::api_fail(HVD_ERR_ARG, "NULL buffer");
    g_copy_pool.copy((uint8_t*)dst, (const uint8_t*)src, n, threads);
    return HVD_OK;
}
#endif

// Library default of hvd_hasher_set_threads(h, 0): a quarter of the CPUs this process may run on, between 2 and 8 (the pool's
// maximum). Eight threads were never slower than four on the hosts measured and up to 15 % faster where the copy competes
// with the DMA engine for host memory (short bursts leave the memory to the engine: profiles/r05_vh_where.txt, end); a small
// machine keeps its cores for the decoder.
static int default_copy_threads() {
    static const int n = [] {
        int cpus = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) cpus = CPU_COUNT(&set);
        return std::max(2, std::min(1 + hvd::CopyPool::kMaxHelpers, cpus / 4));
    }();
    return n;
}

struct hvd_hasher {
    int ctx = 0;           // the context (device of the group) this hasher was created on: every call runs there
    int copy_threads = default_copy_threads();  // threads that share one frame's copy into the ring (hvd_hasher_set_threads)
    int w = 0, h = 0, channels = 0;
    bool dihedral = false;         // hvd_hasher_create_dihedral: 8 hashes per frame (hash_bytes() = 256)
    int64_t batch = 0;             // frames a slot holds
    int64_t limit = 0;             // frames after which the CURRENT batch is submitted: ramps up to `batch` (first_limit)
    size_t frame_bytes = 0;
    Slot slot[kSlots];
    int cur = 0;
    std::vector<uint8_t> hashes;   // collected results, frame order
    std::vector<int32_t> quality;
    bool acquired = false;         // hvd_hasher_acquire handed out the next frame's slot memory
    int64_t acquired_n = 0;        // ... and hvd_hasher_acquire_n this many frames of it
    // autocrop (hvd_hasher_create_autocrop)
    bool autocrop = false;
    hvd::RectRule rule{};          // the rule of the fold: Black (hvd_hasher_create_autocrop) or Detail (.._autocrop_detail)
    int64_t max_frames = 0;        // frames one video may retain (max_retained_bytes / frame_bytes)
    int64_t taken = 0;             // frames committed since the last finish
    bool rect_closed = false;      // k_rect_finish has turned the accumulators into the rectangle (it must run once)
    std::vector<Block> store;      // the video's frames in HBM, in push order
    void* d_meta = nullptr;        // int32[4] rectangle record (accumulators, then {top, left, height, width}) + int64[2] CSR of one video
    int32_t* d_rect() const { return (int32_t*)d_meta; }
    const long long* d_offsets() const { return (const long long*)((char*)d_meta + 16); }
    size_t hash_bytes() const { return dihedral ? 8 * 32 : 32; }
};

// A video starts on an empty pipeline (the reference makes one hasher per video and finish() drains it, vpdqpy/vpdqpy.py:113-119):
// with full 64 MiB batches the DMA engine idled for the whole first batch's fill time at the start of every video -- 0.94 ms of a
// 5.5 ms video of 300 frames at 512x512 (profiles/r05_vh_where.txt). The first batch of a video is therefore SMALL (4 MiB of
// frames) and the batch size GROWS from submit to submit up to the slot's capacity; finish() starts the ramp again. The growth
// factor matters: the engine uploads batch k while the host fills batch k+1, and the host (4 copy threads: ~10 us per 786 KB
// frame) is only 1.4x faster than the link (13.7 us) -- doubling made every batch of the ramp take longer to fill than its
// predecessor took to upload (0.44 ms of idle link per video); x 1.25 keeps the link busy. Frames of 4 KB never leave the first
// step (1024 of them), so the small-frame path still submits once per video.
static int64_t first_limit(const hvd_hasher* hs) {
    const int64_t f = (int64_t)(((size_t)4 << 20) / hs->frame_bytes);
    return std::max<int64_t>(1, std::min<int64_t>(hs->batch, f));
}
static int64_t next_limit(const hvd_hasher* hs) { return std::min<int64_t>(hs->batch, hs->limit + std::max<int64_t>(1, hs->limit / 4)); }

// A hasher lives on the context it was created on, whatever context the calling thread has selected.
namespace {
struct CtxScope {
    int saved;
    explicit CtxScope(int ctx) : saved(hvd::api_context()) { hvd::api_set_context(ctx); }
    ~CtxScope() {
        hvd::api_set_context(saved);
        (void)hvd::api_bind_device();
    }
};
}  // namespace

#define S_TRY(expr)                                                                                        \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return hvd::api_fail(HVD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

static int collect(hvd_hasher* hs, Slot& s) {
    if (s.in_flight == 0) return HVD_OK;
    {
        NsScope ns(g_ns_wait);
        S_TRY(hipEventSynchronize(s.done));
    }
    if (s.results) {
        hs->hashes.insert(hs->hashes.end(), s.h_hashes, s.h_hashes + hs->hash_bytes() * s.in_flight);
        hs->quality.insert(hs->quality.end(), s.h_quality, s.h_quality + s.in_flight);
    }
    s.in_flight = 0;
    return HVD_OK;
}

// Room for `frames` more frames, back to back, in the last block of the store -- or a new block, of up to one slot set's worth
// of frames (kSlots batches) and never more than the video may still retain. Called when a batch BEGINS, so an allocation
// failure surfaces before the batch's first frame is taken.
static int store_reserve(hvd_hasher* hs, int64_t frames) {
    if (!hs->store.empty() && hs->store.back().used + frames <= hs->store.back().cap) return HVD_OK;
    int64_t held = 0;
    for (const Block& b : hs->store) held += b.used;
    if (!hs->store.empty() && hs->store.back().used == 0) {  // (a parked block too small for this batch)
        (void)hipFree(hs->store.back().d);
        hs->store.pop_back();
    }
    Block b;
    b.cap = std::max<int64_t>(frames, std::min<int64_t>(kSlots * hs->batch, hs->max_frames - held));
    hipError_t e = hipMalloc((void**)&b.d, hs->frame_bytes * (size_t)b.cap);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hvd::api_fail(HVD_ERR_HIP, "retained frame store: %s (%lld frames held)", hipGetErrorString(e), (long long)held);
    }
    hs->store.push_back(b);
    return HVD_OK;
}

// An autocrop batch: upload into the store, fold into the rectangle record behind it. Nothing is hashed yet.
static int submit_retain(hvd_hasher* hs, Slot& s) {
    NsScope ns(g_ns_submit);
    const int64_t m = s.filled;
    if (int rc = store_reserve(hs, m)) return rc;  // (reserved when the batch began: no allocation here)
    Block& b = hs->store.back();
    uint8_t* dst = b.d + hs->frame_bytes * (size_t)b.used;
    S_TRY(hipMemcpyAsync(dst, s.h_frames, hs->frame_bytes * (size_t)m, hipMemcpyHostToDevice, s.stream));
    S_TRY(hvd::launch_rect_fold(hs->rule, nullptr, dst, m, hs->h, hs->w, hs->channels, hs->d_offsets(), 1, hs->d_rect(), s.stream));
    S_TRY(hipEventRecord(s.done, s.stream));
    b.used += m;
    s.in_flight = m;
    s.results = false;
    s.filled = 0;
    hs->limit = next_limit(hs);
    return HVD_OK;
}

// Hash the m frames at src (device memory) on slot s, on its stream and into its buffers -- with the hasher's kernel (plain or
// dihedral), or under_rect: inside the video's rectangle --, download the results, record the event, mark the slot in flight.
static int enqueue_hash(hvd_hasher* hs, Slot& s, const void* src, int64_t m, bool under_rect) {
    S_TRY(under_rect ? hvd::api_launch_hash_rects(src, m, hs->h, hs->w, hs->channels, hs->d_offsets(), 1, hs->d_rect(), s.d_scratch,
                                                  s.d_hashes, s.d_quality, s.stream)
                     : hvd::api_launch_hash(src, m, hs->h, hs->w, hs->channels, s.d_scratch, s.d_hashes, s.d_quality, s.stream, hs->dihedral));
    S_TRY(hipMemcpyAsync(s.h_hashes, s.d_hashes, hs->hash_bytes() * (size_t)m, hipMemcpyDeviceToHost, s.stream));
    S_TRY(hipMemcpyAsync(s.h_quality, s.d_quality, 4 * (size_t)m, hipMemcpyDeviceToHost, s.stream));
    S_TRY(hipEventRecord(s.done, s.stream));
    s.in_flight = m;
    s.results = true;
    return HVD_OK;
}

static int submit(hvd_hasher* hs, Slot& s) {
    if (s.filled == 0) return HVD_OK;
    if (hs->autocrop) return submit_retain(hs, s);
    // a switch to fma while a dihedral video is in progress fails here, before anything of this batch is enqueued (it stays
    // staged), instead of hashing the rest of the video another way
    if (int rc = hvd::check_dihedral_dct(hs->dihedral)) return rc;
    NsScope ns(g_ns_submit);
    S_TRY(hipMemcpyAsync(s.d_frames, s.h_frames, hs->frame_bytes * (size_t)s.filled, hipMemcpyHostToDevice, s.stream));
    if (int rc = enqueue_hash(hs, s, s.d_frames, s.filled, false)) return rc;
    s.filled = 0;
    hs->limit = next_limit(hs);
    return HVD_OK;
}

// The reference creates one VideoHasher per video (vpdqpy/vpdqpy.py:113) and videos come strictly one after the
// other (dedup.py:346-352). Pinning and unpinning 6 x 32 MiB of host memory per video costs more than hashing a
// short video, so a destroyed hasher's slots (pinned staging, device buffers, streams, events) are PARKED and the
// next hvd_hasher_create with the same geometry and kind (plain / dihedral: hash buffers of 32 / 256 bytes per frame) takes
// them over. At most kMaxParked sets are kept (a GUI worker and the CLI never run more than one or two hashers at a time);
// hvd_shutdown() releases them.
namespace {
constexpr size_t kMaxParked = 2;
std::mutex g_park_mu;
std::vector<hvd_hasher*> g_parked;

void free_hasher(hvd_hasher* hs) {
    for (Slot& s : hs->slot) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.h_frames) (void)hipHostFree(s.h_frames);
        if (s.h_hashes) (void)hipHostFree(s.h_hashes);
        if (s.h_quality) (void)hipHostFree(s.h_quality);
        if (s.d_frames) (void)hipFree(s.d_frames);
        if (s.d_scratch) (void)hipFree(s.d_scratch);
        if (s.d_hashes) (void)hipFree(s.d_hashes);
        if (s.d_quality) (void)hipFree(s.d_quality);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    for (Block& b : hs->store) (void)hipFree(b.d);
    if (hs->d_meta) (void)hipFree(hs->d_meta);
    delete hs;
}

// An autocrop hasher before its (next) video: nothing retained, the rectangle record at its initial value. The first block is
// kept for the next video (at most one slot set's worth of frames, what a plain hasher's slots hold in d_frames), the others
// are freed. Every slot is idle when this runs.
int reset_video(hvd_hasher* hs) {
    hs->taken = 0;
    hs->rect_closed = false;
    while (hs->store.size() > 1) {
        (void)hipFree(hs->store.back().d);
        hs->store.pop_back();
    }
    if (!hs->store.empty()) hs->store[0].used = 0;
    S_TRY(hvd::launch_rect_init(hs->d_rect(), 1, hs->slot[0].stream));
    S_TRY(hipStreamSynchronize(hs->slot[0].stream));
    return HVD_OK;
}
}  // namespace

namespace hvd {
void stream_set_copy_nt(int on) { set_copy_nt(on); }   // hvd_debug_set("copy_nt", 0|1)
int stream_copy_nt_level() { return copy_nt_level(); }  // hvd_debug_get("copy_nt"): 0 plain memcpy, 2 AVX2, 3 AVX-512 streaming stores
void stream_release_cache() {
    g_copy_pool.stop();
    std::lock_guard<std::mutex> lk(g_park_mu);
    for (hvd_hasher* hs : g_parked) free_hasher(hs);
    g_parked.clear();
}
}  // namespace hvd

extern "C" {

int hvd_hasher_destroy(hvd_hasher* hs) {
    if (!hs) return HVD_OK;
    CtxScope scope(hs->ctx);
    (void)hvd::api_bind_device();
    bool complete = true;
    for (Slot& s : hs->slot) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        complete = complete && s.stream && s.done && s.h_frames && s.h_hashes && s.h_quality && (s.d_frames || hs->autocrop) &&
                   s.d_hashes && s.d_quality;
        s.filled = s.in_flight = 0;
    }
    if (complete && hs->autocrop && hvd::api_dct_device()) complete = hs->d_meta && reset_video(hs) == HVD_OK;
    if (complete && hvd::api_dct_device()) {  // park it for the next video (never after hvd_shutdown)
        hs->hashes.clear();
        hs->quality.clear();
        hs->cur = 0;
        hs->acquired = false;
        hs->limit = first_limit(hs);
        std::lock_guard<std::mutex> lk(g_park_mu);
        g_parked.push_back(hs);
        if (g_parked.size() > kMaxParked) {
            free_hasher(g_parked.front());
            g_parked.erase(g_parked.begin());
        }
        return HVD_OK;
    }
    free_hasher(hs);
    return HVD_OK;
}

}  // extern "C"

struct AutocropArgs {
    hvd::RectRule rule;
    int64_t max_retained_bytes;
};

static int create_hasher(int width, int height, int channels, int64_t batch_frames, bool dihedral, hvd_hasher** out,
                         const AutocropArgs* ac = nullptr) {
    if (!out) return hvd::api_fail(HVD_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!hvd::api_dct_device()) return hvd::api_fail(HVD_ERR_STATE, "hvd_init() has not been called (no CPU fallback exists)");
    if (int rc = hvd::check_geometry(height, width, channels)) return rc;
    if (batch_frames < 1) return hvd::api_fail(HVD_ERR_ARG, "bad hasher batch of %lld frames", (long long)batch_frames);
    if (int rc = hvd::check_dihedral_dct(dihedral)) return rc;
    if (int rc = ac ? hvd::check_rect_rule(ac->rule) : HVD_OK) return rc;
    const int64_t max_frames =
        !ac ? 0 : (ac->max_retained_bytes > 0 ? ac->max_retained_bytes : kDefaultRetained) / ((int64_t)width * height * channels);
    const auto set_autocrop = [&](hvd_hasher* p) {
        if (!ac) return;
        p->rule = ac->rule;
        p->max_frames = max_frames;
    };
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        for (size_t k = g_parked.size(); k-- > 0;) {
            hvd_hasher* p = g_parked[k];
            if (p->ctx == hvd::api_context() && p->w == width && p->h == height && p->channels == channels && p->batch == batch_frames &&
                p->dihedral == dihedral && p->autocrop == (ac != nullptr)) {
                g_parked.erase(g_parked.begin() + (long)k);
                p->copy_threads = default_copy_threads();
                set_autocrop(p);
                *out = p;
                return HVD_OK;
            }
        }
    }
    if (int rc = hvd::api_bind_device()) return rc;
    hvd_hasher* hs = new hvd_hasher();
    hs->ctx = hvd::api_context();
    hs->w = width;
    hs->h = height;
    hs->channels = channels;
    hs->dihedral = dihedral;
    hs->autocrop = ac != nullptr;
    set_autocrop(hs);
    hs->batch = batch_frames;
    hs->frame_bytes = (size_t)width * height * channels;
    hs->limit = first_limit(hs);
    const size_t scratch = hvd::HashScratch(batch_frames, height, width, channels, ac != nullptr).total;
    for (Slot& s : hs->slot) {
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_frames, hs->frame_bytes * (size_t)batch_frames, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_hashes, hs->hash_bytes() * (size_t)batch_frames, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_quality, 4 * (size_t)batch_frames, hipHostMallocDefault);
        if (e == hipSuccess && !ac) e = hipMalloc(&s.d_frames, hs->frame_bytes * (size_t)batch_frames);
        if (e == hipSuccess && scratch) e = hipMalloc(&s.d_scratch, scratch);
        if (e == hipSuccess) e = hipMalloc(&s.d_hashes, hs->hash_bytes() * (size_t)batch_frames);
        if (e == hipSuccess) e = hipMalloc(&s.d_quality, 4 * (size_t)batch_frames);
        if (e != hipSuccess) {
            free_hasher(hs);
            hvd::stream_release_cache();  // the parked sets may be what exhausted the pinned / device memory
            return hvd::api_fail(HVD_ERR_HIP, "hasher allocation: %s", hipGetErrorString(e));
        }
    }
    if (ac) {
        const long long csr[2] = {0, 0x7FFFFFFF};  // one video that holds every frame of any batch
        hipError_t e = hipMalloc(&hs->d_meta, 32);
        if (e == hipSuccess) e = hipMemcpy((char*)hs->d_meta + 16, csr, 16, hipMemcpyHostToDevice);
        if (e != hipSuccess || reset_video(hs) != HVD_OK) {
            free_hasher(hs);
            return hvd::api_fail(HVD_ERR_HIP, "hasher allocation: %s", hipGetErrorString(e));
        }
    }
    *out = hs;
    return HVD_OK;
}

extern "C" {

int hvd_hasher_create_autocrop(int width, int height, int channels, int64_t batch_frames, int black_level, int min_bright,
                               int64_t max_retained_bytes, hvd_hasher** out) {
    const AutocropArgs ac{{hvd::RectKind::Black, black_level, min_bright}, max_retained_bytes};
    return create_hasher(width, height, channels, batch_frames, false, out, &ac);
}

int hvd_hasher_create_autocrop_detail(int width, int height, int channels, int64_t batch_frames, int detail_level, int min_detail,
                                      int64_t max_retained_bytes, hvd_hasher** out) {
    const AutocropArgs ac{{hvd::RectKind::Detail, detail_level, min_detail}, max_retained_bytes};
    return create_hasher(width, height, channels, batch_frames, false, out, &ac);
}

int hvd_hasher_create(int width, int height, int channels, int64_t batch_frames, hvd_hasher** out) {
    return create_hasher(width, height, channels, batch_frames, false, out);
}

int hvd_hasher_create_dihedral(int width, int height, int channels, int64_t batch_frames, hvd_hasher** out) {
    return create_hasher(width, height, channels, batch_frames, true, out);
}

/* Zero-copy feed: *out_frame is where the NEXT frame (width*height*channels bytes) belongs, inside the
 * pinned batch slot, so a decoder can reformat straight into it (the reference makes a Python bytes copy
 * per frame instead, vpdqpy/vpdqpy.py:118). Blocks only when that slot's previous batch is still being
 * hashed. The frame counts once hvd_hasher_commit() is called; acquire without commit may be repeated. */
int hvd_hasher_acquire(hvd_hasher* hs, uint8_t** out_frame) {
    if (!hs || !out_frame) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher/out_frame");
    CtxScope scope(hs->ctx);
    if (int rc = hvd::api_bind_device()) return rc;
    if (hs->slot[hs->cur].filled >= hs->limit) {  // its submit failed (e.g. HVD_ERR_STATE): submit it before staging past it
        if (int rc = submit(hs, hs->slot[hs->cur])) return rc;
        hs->cur = (hs->cur + 1) % kSlots;
    }
    Slot& s = hs->slot[hs->cur];
    if (s.filled == 0 && s.in_flight) {  // slot being reused: its previous batch must have landed
        if (int rc = collect(hs, s)) return rc;
    }
    if (hs->autocrop) {  // before the frame is taken: the cap, and room in the store for the batch that begins here
        if (hs->taken >= hs->max_frames)
            return hvd::api_fail(HVD_ERR_OVERFLOW, "the video would retain more than %lld frames (max_retained_bytes)",
                                 (long long)hs->max_frames);
        if (s.filled == 0)
            if (int rc = store_reserve(hs, std::min<int64_t>(hs->limit, hs->max_frames - hs->taken))) return rc;
    }
    *out_frame = s.h_frames + hs->frame_bytes * (size_t)s.filled;
    hs->acquired = true;
    hs->acquired_n = 1;
    return HVD_OK;
}

int hvd_hasher_commit(hvd_hasher* hs) {
    if (!hs) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher");
    CtxScope scope(hs->ctx);
    if (!hs->acquired) return hvd::api_fail(HVD_ERR_STATE, "hvd_hasher_commit() without hvd_hasher_acquire()");
    if (int rc = hvd::api_bind_device()) return rc;
    hs->acquired = false;
    ++hs->taken;
    Slot& s = hs->slot[hs->cur];
    if (++s.filled >= hs->limit) {
        if (int rc = submit(hs, s)) return rc;
        hs->cur = (hs->cur + 1) % kSlots;
    }
    return HVD_OK;
}

/* The same for a RUN of frames (ABI 5): *out_frames is where the next frames belong, *out_n (1 <= *out_n <= want) how many
 * fit there back to back -- what is left of the current batch slot. One call, one pointer, k frames: a decoder that fills
 * 64x64 frames pays one FFI round trip per run instead of two per frame. hvd_hasher_commit_n(n) makes the
 * first n of them count (n <= *out_n; n = 0 is legal and gives the run back). */
int hvd_hasher_acquire_n(hvd_hasher* hs, int64_t want, uint8_t** out_frames, int64_t* out_n) {
    if (!hs || !out_frames || !out_n) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher/out_frames/out_n");
    if (want < 1) return hvd::api_fail(HVD_ERR_ARG, "want must be at least 1");
    if (int rc = hvd_hasher_acquire(hs, out_frames)) return rc;
    const Slot& s = hs->slot[hs->cur];
    *out_n = hs->acquired_n = std::min<int64_t>(want, hs->limit - s.filled);
    if (hs->autocrop) *out_n = hs->acquired_n = std::min<int64_t>(*out_n, hs->max_frames - hs->taken);
    return HVD_OK;
}

int hvd_hasher_commit_n(hvd_hasher* hs, int64_t n) {
    if (!hs) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher");
    CtxScope scope(hs->ctx);
    if (!hs->acquired) return hvd::api_fail(HVD_ERR_STATE, "hvd_hasher_commit_n() without hvd_hasher_acquire_n()");
    Slot& s = hs->slot[hs->cur];
    if (n < 0 || n > hs->acquired_n) return hvd::api_fail(HVD_ERR_ARG, "commit of %lld frames, %lld acquired", (long long)n, (long long)hs->acquired_n);
    if (int rc = hvd::api_bind_device()) return rc;
    hs->acquired = false;
    hs->taken += n;
    s.filled += n;
    if (s.filled >= hs->limit) {
        if (int rc = submit(hs, s)) return rc;
        hs->cur = (hs->cur + 1) % kSlots;
    }
    return HVD_OK;
}

/* Copies one frame (width*height*channels bytes) into the ring (acquire + memcpy + commit). The caller's
 * buffer is not kept. */
int hvd_hasher_push(hvd_hasher* hs, const uint8_t* frame) {
    if (!hs || !frame) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher/frame");
    uint8_t* dst = nullptr;
    if (int rc = hvd_hasher_acquire(hs, &dst)) return rc;
    {
        NsScope ns(g_ns_copy);
        g_copy_pool.copy(dst, frame, hs->frame_bytes, hs->copy_threads);
    }
    return hvd_hasher_commit(hs);
}

/* Threads that share the host-side copy of one frame in hvd_hasher_push (the caller included): the counterpart of the
 * reference hasher's worker threads. n <= 0: the library default (4). Frames below ~200 KB are copied by the caller. */
int hvd_hasher_set_threads(hvd_hasher* hs, int n) {
    if (!hs) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher");
    hs->copy_threads = n <= 0 ? default_copy_threads() : std::min(n, 1 + hvd::CopyPool::kMaxHelpers);
    return HVD_OK;
}

}  // extern "C"

// finish() of an autocrop hasher, every upload and fold done: close the rectangle, read its 16 bytes back, then hash the
// retained frames block by block in runs of up to a batch, one run per slot on the slot's stream (its scratch, its result
// buffers), so that kSlots runs are in flight; collect() gathers them in ring order = push order. A full-frame rectangle takes
// the plain kernels (the same bits: a full rectangle is the frame), as the host batch entry does.
static int hash_retained(hvd_hasher* hs, int32_t out_rect[4]) {
    hs->hashes.clear();  // (a finish() that failed on a small `cap` may be repeated)
    hs->quality.clear();
    hipStream_t s0 = hs->slot[0].stream;
    if (!hs->rect_closed) S_TRY(hvd::launch_rect_finish(hs->d_rect(), 1, hs->h, hs->w, s0));
    hs->rect_closed = true;
    S_TRY(hipMemcpyAsync(out_rect, hs->d_rect(), 16, hipMemcpyDeviceToHost, s0));
    S_TRY(hipStreamSynchronize(s0));
    const bool full = hvd::rect_is_full_frame(out_rect, hs->h, hs->w);
    int k = 0;
    for (const Block& b : hs->store) {
        for (int64_t f0 = 0; f0 < b.used; f0 += hs->batch, k = (k + 1) % kSlots) {
            Slot& s = hs->slot[k];
            if (int rc = collect(hs, s)) return rc;
            NsScope ns(g_ns_submit);
            const int64_t m = std::min<int64_t>(hs->batch, b.used - f0);
            if (int rc = enqueue_hash(hs, s, b.d + hs->frame_bytes * (size_t)f0, m, !full)) return rc;
        }
    }
    for (int j = 0; j < kSlots; ++j, k = (k + 1) % kSlots)  // the oldest run still in flight sits in the slot that comes next
        if (int rc = collect(hs, hs->slot[k])) return rc;
    return HVD_OK;
}

/* Flushes the partial batch, waits for everything, returns all hashes / qualities in push
 * order (no quality filtering: that is VideoHasher.finish's policy, vpdqpy.py:119). The hasher
 * is empty afterwards and can be reused for the next video. */
static int finish_hasher(hvd_hasher* hs, bool dihedral, uint8_t* out_hashes, int32_t* out_quality, int64_t cap, int64_t* out_n,
                         int32_t* out_rect = nullptr) {
    if (!hs || !out_n) return hvd::api_fail(HVD_ERR_ARG, "NULL hasher/out_n");
    if (hs->autocrop != (out_rect != nullptr))
        return hvd::api_fail(HVD_ERR_STATE, hs->autocrop ? "an autocrop hasher finishes with hvd_hasher_finish_autocrop()"
                                                         : "hvd_hasher_finish_autocrop() on a hasher without autocrop");
    if (hs->dihedral != dihedral)
        return hvd::api_fail(HVD_ERR_STATE, dihedral ? "hvd_hasher_finish_dihedral() on a plain hasher: use hvd_hasher_finish()"
                                                     : "hvd_hasher_finish() on a dihedral hasher: use hvd_hasher_finish_dihedral()");
    CtxScope scope(hs->ctx);
    if (int rc = hvd::api_bind_device()) return rc;
    hs->acquired = false;
    // Slots are submitted in ring order, so the oldest batch still in flight sits in the slot that will be
    // filled next: with nothing staged in the current slot it is the current slot itself (the frame count was
    // a multiple of the batch size), otherwise push() collected it before staging and the oldest is cur+1.
    Slot& c = hs->slot[hs->cur];
    if (c.filled > 0) {
        for (int k = 1; k <= kSlots; ++k) {
            Slot& s = hs->slot[(hs->cur + k) % kSlots];
            if (&s == &c)
                if (int rc = submit(hs, s)) return rc;  // the partial batch is the youngest
            if (int rc = collect(hs, s)) return rc;
        }
    } else {
        for (int k = 0; k < kSlots; ++k)
            if (int rc = collect(hs, hs->slot[(hs->cur + k) % kSlots])) return rc;
    }
    if (hs->autocrop)
        if (int rc = hash_retained(hs, out_rect)) return rc;
    const int64_t n = (int64_t)hs->quality.size();
    *out_n = n;
    if (n > cap) return hvd::api_fail(HVD_ERR_OVERFLOW, "need room for %lld frames, cap %lld", (long long)n, (long long)cap);
    if (n) {
        if (!out_hashes || !out_quality) return hvd::api_fail(HVD_ERR_ARG, "NULL output");
        memcpy(out_hashes, hs->hashes.data(), hs->hash_bytes() * (size_t)n);
        memcpy(out_quality, hs->quality.data(), 4 * (size_t)n);
    }
    hs->hashes.clear();
    hs->quality.clear();
    hs->cur = 0;
    hs->limit = first_limit(hs);  // the next video starts on an empty pipeline again
    if (hs->autocrop) return reset_video(hs);
    return HVD_OK;
}

extern "C" {

int hvd_hasher_finish(hvd_hasher* hs, uint8_t* out_hashes, int32_t* out_quality, int64_t cap, int64_t* out_n) {
    return finish_hasher(hs, false, out_hashes, out_quality, cap, out_n);
}

/* n*8*32 bytes: a frame's 8 variants back to back, in the dihedral kernel's order (vpdq.TRANSFORMS). */
int hvd_hasher_finish_dihedral(hvd_hasher* hs, uint8_t* out_hashes8, int32_t* out_quality, int64_t cap, int64_t* out_n) {
    return finish_hasher(hs, true, out_hashes8, out_quality, cap, out_n);
}

/* An autocrop hasher's results: hashes and qualities under the video's content rectangle, which goes to out_rect. */
int hvd_hasher_finish_autocrop(hvd_hasher* hs, uint8_t* out_hashes, int32_t* out_quality, int64_t cap, int64_t* out_n,
                               int32_t out_rect[4]) {
    if (!out_rect) return hvd::api_fail(HVD_ERR_ARG, "NULL out_rect");
    return finish_hasher(hs, false, out_hashes, out_quality, cap, out_n, out_rect);
}

int hvd_hasher_pending(hvd_hasher* hs, int64_t* out_frames) {
    if (!hs || !out_frames) return hvd::api_fail(HVD_ERR_ARG, "NULL");
    if (hs->autocrop) {
        *out_frames = hs->taken;
        return HVD_OK;
    }
    int64_t n = (int64_t)hs->quality.size();
    for (Slot& s : hs->slot) n += s.filled + s.in_flight;
    *out_frames = n;
    return HVD_OK;
}

}  // extern "C"
