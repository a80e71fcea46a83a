// k_crops.hip -- crop-ladder PDQ: every frame hashed under the full frame and under K <= 7 call-uniform rectangles,
// for aspect-ratio re-crops and pan-and-scan copies. The per-rectangle body is hvd_rect_dev.h's (one definition with
// k_autocrop_fused.hip's k_down_rect), so a plane is that of the oracle on the contiguous crop, bit for bit.
//
//   k_down_crops       frames up to 512 x 512: one workgroup per frame, an inner loop over the K + 1 rectangles; the first pass
//                      brings the frame in from HBM, the others re-read it from cache. A 64 x 64 rectangle is the crop's luma,
//                      unfiltered (upstream's shortcut), in the same loop. At exactly 512 x 512 the full frame is left to
//                      k_pdq.hip's own front-end, which is nine times faster on it, and the loop takes the crops alone: such a
//                      frame is read twice, once by either kernel.
//   k_crops_table      larger frames: the one-video CSR and the rectangle list in memory, for the generic k_box_scan_rect chain
//                      that launch_pdq_hash_crops runs once per rectangle
//   k_crops_scatter    the n (K + 1) hashes / qualities of launch_pdq_hash64 -> the dihedral layout (8 slots per frame, slots
//                      above K zero), the full frame's quality, the optional per-slot qualities
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_pdq_dev.h"
#include "hvd_rect_dev.h"

namespace hvd {

namespace {

// The rectangles of a call, by value in the kernel arguments (128 bytes): r[0] is the full frame, r[1 .. K] the crops, every
// one {top, left, height, width} inside the frame with both sides >= 64 (checked on the host: crops_valid).
struct CropList {
    int4 r[HVD_MAX_CROPS + 1];
};

// The nrect rectangles of the list under every frame; plane (f, k) -> out64 + (f * nrect + k) * 4096. (Where the full frame
// has a faster front-end of its own, launch_pdq_hash_crops hands over the list without it.) The rectangle state is wave-uniform
// (kernel arguments), the body's switches over the windows are scalar branches.
template <int CH>
__global__ __launch_bounds__(512, 2) void k_down_crops(const uint8_t* __restrict__ frames, int n, int h, int w,
                                                       const CropList crops, int nrect, float* __restrict__ out64) {
    __shared__ float buf[kRMax][kRBufLd];
    __shared__ float cs[kRS][kRCsLd];
    const int y = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    for (int f = blockIdx.x; f < n; f += gridDim.x) {  // (a slab: n <= kCropsSlab)
        const uint8_t* src = frames + (size_t)f * h * w * CH;  // (the body is handed this frame as frame 0)
#pragma unroll 1
        for (int k = 0; k < nrect; ++k) {
            const int4 rc = crops.r[k];
            const int top = rc.x, left = rc.y, hh = rc.z, ww = rc.w;
            const size_t plane = (size_t)(f * nrect + k);
            if (hh == 64 && ww == 64) {
                float* dst = out64 + plane * 4096;
                for (int p = y; p < 4096; p += 512) {
                    const size_t e = (size_t)(top + (p >> 6)) * w + (left + (p & 63));
                    dst[p] = CH == 1 ? luma_gray(src[e]) : luma_rgb((float)src[3 * e], (float)src[3 * e + 1], (float)src[3 * e + 2]);
                }
                continue;
            }
            rect_frame_plane<CH>(src, 0ll, 0, w, top, left, hh, ww, out64, plane, buf, cs, y, wave, lane);
        }
    }
}

// offsets[0 .. 1] = {0, n}: all frames are one video; rects[k] = the k-th rectangle (launch_pdq_downsample_rects' operands)
__global__ __launch_bounds__(64) void k_crops_table(const CropList crops, int nrect, long long n, long long* __restrict__ offsets,
                                                    int4* __restrict__ rects) {
    const int t = threadIdx.x;
    if (t < 2) offsets[t] = t == 0 ? 0 : n;
    if (t < nrect) rects[t] = crops.r[t];
}

// in: hashes / quality of the loop's planes, plane (f, k) at index f * sf + (k - first) * sk; in0 (first = 1 only): those of the
// full frames, frame f at index f. One lane per (frame, slot, 32-bit word of the hash).
__global__ __launch_bounds__(256) void k_crops_scatter(const uint32_t* __restrict__ in_hashes, const int32_t* __restrict__ in_quality,
                                                       const uint32_t* __restrict__ in0_hashes, const int32_t* __restrict__ in0_quality,
                                                       long long n, int nrect, int first, long long sf, long long sk,
                                                       uint32_t* __restrict__ hashes8, int32_t* __restrict__ quality,
                                                       int32_t* __restrict__ crop_quality) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // (f * 8 + slot) * 8 + word
    if (i >= n * 64) return;
    const long long f = i >> 6;
    const int slot = (int)(i >> 3) & 7, word = (int)i & 7;
    const bool live = slot < nrect, full = slot < first;
    const long long p = full ? f : f * sf + (slot - first) * sk;
    hashes8[i] = !live ? 0u : full ? in0_hashes[p * 8 + word] : in_hashes[p * 8 + word];
    if (word == 0) {
        const int32_t q = !live ? 0 : full ? in0_quality[p] : in_quality[p];
        if (slot == 0) quality[f] = q;
        if (crop_quality) crop_quality[f * 8 + slot] = q;
    }
}

CropList crop_list(const int32_t* crops, int K, int h, int w) {
    CropList cl;
    for (int k = 0; k <= HVD_MAX_CROPS; ++k) cl.r[k] = make_int4(0, 0, h, w);
    for (int k = 0; k < K; ++k) cl.r[k + 1] = make_int4(crops[4 * k], crops[4 * k + 1], crops[4 * k + 2], crops[4 * k + 3]);
    return cl;
}

constexpr int64_t kCropsSlab = 1024;  // frames per pass of the rectangle loop over the scratch: <= 8 x 1024 planes of 16 KiB
// ... and per pass of the full-frame front-end of a 512 x 512 call: what fills the chip with k_down512w's lone waves (passes
// of 1 024 frames ran it at two thirds of its rate: DESIGN 4.12)
constexpr int64_t kCropsFullSlab = 3 * kCropsSlab;

size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// Scratch of a call of n frames. One slab of the loop: planes | hashes | qualities | (generic path) workspace | frame table | CSR
// + rectangle list. 512 x 512 only, one pass of the full-frame front-end: planes | hashes | qualities | k_down512w's workspace.
struct CropsScratch {
    size_t planes, hashes, quality, ws, geom, table, planes0, hashes0, quality0, ws0, total;
    CropsScratch(int64_t n, int h, int w, int nrect) {
        const int64_t m = n < kCropsSlab ? n : kCropsSlab;
        const size_t P = (size_t)m * nrect;
        planes = 0;
        hashes = planes + sizeof(float) * 4096 * P;
        quality = hashes + 32 * P;
        ws = up16(quality + 4 * P);
        const bool generic = h > kDownRectMax || w > kDownRectMax;
        // (the generic chain walks its frames 1 024 at a time: launch_pdq_downsample_rects)
        geom = up16(ws + (generic ? sizeof(float) * (size_t)m * pdq_downsample_ws_floats(h, w) : 0));
        table = geom + (generic ? pdq_rects_geom_bytes(m) : 0);
        planes0 = up16(table + (generic ? 16 + 16 * (size_t)(HVD_MAX_CROPS + 1) : 0));
        const size_t F = h == 512 && w == 512 ? (size_t)(n < kCropsFullSlab ? n : kCropsFullSlab) : 0;
        hashes0 = planes0 + sizeof(float) * 4096 * F;
        quality0 = hashes0 + 32 * F;
        ws0 = up16(quality0 + 4 * F);
        total = ws0 + sizeof(float) * pdq_down512_ws_floats((int64_t)F);
    }
};

}  // namespace

bool crops_valid(const int32_t* crops, int K, int h, int w) {
    if (!crops || K < 1 || K > HVD_MAX_CROPS) return false;
    for (int k = 0; k < K; ++k) {
        const int32_t top = crops[4 * k], left = crops[4 * k + 1], hh = crops[4 * k + 2], ww = crops[4 * k + 3];
        if (top < 0 || left < 0 || hh < 64 || ww < 64 || hh > h || ww > w || top > h - hh || left > w - ww) return false;
    }
    return true;
}

size_t pdq_crops_scratch_bytes(int64_t n, int h, int w, int K) {
    return CropsScratch(n, h, w, K + 1).total;
}

// The launch chain of hvd_dev_pdq_hash_frames_crops on stream s (arguments validated: crops_valid, n > 0, 64 <= h, w <= 4096).
// dct: launch_pdq_hash64's table. d_scratch: pdq_crops_scratch_bytes(n, h, w, K), 16-byte aligned.
hipError_t launch_pdq_hash_crops(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const int32_t* crops, int K,
                                 const float* d_dct, void* d_scratch, uint8_t* d_hashes8, int32_t* d_quality,
                                 int32_t* d_crop_quality, hipStream_t s) {
    const int nrect = K + 1;
    const CropList cl = crop_list(crops, K, h, w);
    const bool generic = h > kDownRectMax || w > kDownRectMax;
    if (generic && (jarosz_window(h) > kTW || jarosz_window(w) > kTW)) return hipErrorInvalidValue;
    const CropsScratch lay(n, h, w, nrect);
    char* base_ptr = (char*)d_scratch;
    float* planes = (float*)(base_ptr + lay.planes);
    uint8_t* th = (uint8_t*)(base_ptr + lay.hashes);
    int32_t* tq = (int32_t*)(base_ptr + lay.quality);
    uint8_t* th0 = (uint8_t*)(base_ptr + lay.hashes0);
    int32_t* tq0 = (int32_t*)(base_ptr + lay.quality0);
    const size_t frame_bytes = (size_t)h * w * channels;
    // The full frame of a 512 x 512 call has a front-end of its own at a large fraction of the read loop's rate (k_down512w,
    // DESIGN 4.3), which the rectangle body is far from (11.7 ms against 1.3 ms on 6 144 frames): slot 0 goes
    // there, in passes of its own size, and the loop takes the crops alone. Every other geometry: slot 0 is rectangle 0 of the loop.
    const int first = !generic && h == 512 && w == 512 && g_pdq_fused_down512 ? 1 : 0;
    CropList rest = cl;  // the rectangles the loop takes: all of them, or the crops alone
    for (int k = 0; first && k < K; ++k) rest.r[k] = cl.r[k + 1];
    for (int64_t f0 = 0; f0 < n; f0 += kCropsSlab) {
        const int64_t m = (n - f0) < kCropsSlab ? (n - f0) : kCropsSlab;
        const uint8_t* src = d_frames + frame_bytes * (size_t)f0;
        const int64_t g0 = f0 - f0 % kCropsFullSlab;  // the full-frame pass this slab lies in: frames g0 .. g0 + mf - 1
        if (first && f0 == g0) {
            const int64_t mf = (n - g0) < kCropsFullSlab ? (n - g0) : kCropsFullSlab;
            hipError_t e = launch_pdq_downsample(src, mf, h, w, channels, (float*)(base_ptr + lay.ws0), (float*)(base_ptr + lay.planes0), s);
            if (e == hipSuccess) e = launch_pdq_hash64(base_ptr + lay.planes0, 1, mf, d_dct, th0, tq0, s);
            if (e != hipSuccess) return e;
        }
        long long sf, sk;
        if (!generic) {
            // one workgroup per CU fits by LDS (133 KB); frames beyond the grid are taken in a grid-stride loop
            const unsigned grid = (unsigned)(m < 256 ? m : 256);
            if (channels == 3)
                hipLaunchKernelGGL(k_down_crops<3>, dim3(grid), dim3(512), 0, s, src, (int)m, h, w, rest, nrect - first, planes);
            else
                hipLaunchKernelGGL(k_down_crops<1>, dim3(grid), dim3(512), 0, s, src, (int)m, h, w, rest, nrect - first, planes);
            sf = nrect - first;
            sk = 1;
        } else {
            // correct first, not fast: the generic four passes once per rectangle, planes rectangle-major. The frame table is
            // k_frame_geom's, filled with that one rectangle (every frame lies in the one video of the CSR {0, m}).
            long long* d_off = (long long*)(base_ptr + lay.table);
            const int32_t* d_rects = (const int32_t*)(base_ptr + lay.table + 16);
            hipLaunchKernelGGL(k_crops_table, dim3(1), dim3(64), 0, s, cl, nrect, (long long)m, d_off, (int4*)(base_ptr + lay.table + 16));
            for (int k = 0; k < nrect; ++k) {
                hipError_t e = launch_pdq_downsample_rects(src, m, h, w, channels, d_off, 1u, d_rects + 4 * k, base_ptr + lay.geom,
                                                           (float*)(base_ptr + lay.ws), planes + (size_t)k * m * 4096, s);
                if (e != hipSuccess) return e;
            }
            sf = 1;
            sk = m;
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = launch_pdq_hash64(planes, 1, m * (nrect - first), d_dct, th, tq, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_crops_scatter, dim3((unsigned)((m * 64 + 255) / 256)), dim3(256), 0, s, (const uint32_t*)th, tq,
                           (const uint32_t*)(th0 + 32 * (f0 - g0)), tq0 + (f0 - g0), (long long)m, nrect, first, sf, sk,
                           (uint32_t*)(d_hashes8 + 256 * (size_t)f0), d_quality + f0, d_crop_quality ? d_crop_quality + 8 * f0 : nullptr);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hvd
