// k_autocrop_fused.hip -- content-rectangle PDQ: the four down-sampler passes of k_autocrop.hip's k_box_scan_rect
// in one launch, for frames up to 512 x 512. Same recurrence, same operation order: the 64 x 64 planes are those of the generic
// passes and of the oracle on the contiguous crop, bit for bit. The passes themselves are hvd_rect_dev.h's, shared with k_crops.hip.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_pdq_dev.h"
#include "hvd_rect_dev.h"

namespace hvd {

namespace {

// k_down_rect: hvd_rect_dev.h's frame body under the rectangle geom[f] of every frame. One workgroup of 512 lanes per frame,
// frames beyond the grid in a grid-stride loop. LDS 133 248 bytes, so ONE workgroup per CU (8 waves, 2 per SIMD, <= 256 VGPRs).
template <int CH>
__global__ __launch_bounds__(512, 2) void k_down_rect(const uint8_t* __restrict__ frames, long long n, int h, int w,
                                                      const int4* __restrict__ geom, float* __restrict__ out64) {
    __shared__ float buf[kRMax][kRBufLd];
    __shared__ float cs[kRS][kRCsLd];
    const int y = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    for (long long f = blockIdx.x; f < n; f += gridDim.x) {
        const int4 rc = geom[f];  // inside the frame, both sides in [64, 512] (k_frame_geom)
        const int top = __builtin_amdgcn_readfirstlane(rc.x), left = __builtin_amdgcn_readfirstlane(rc.y);
        const int hh = __builtin_amdgcn_readfirstlane(rc.z), ww = __builtin_amdgcn_readfirstlane(rc.w);
        if (hh == 64 && ww == 64) continue;  // k_luma64_rect's
        rect_frame_plane<CH>(frames, f, h, w, top, left, hh, ww, out64, (size_t)f, buf, cs, y, wave, lane);
    }
}

}  // namespace

// geom: the frame -> rectangle table of k_frame_geom (every record inside the frame, both sides >= 64). Frames whose
// rectangle is 64 x 64 are left to k_luma64_rect.
void launch_down_rect(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const void* d_geom, float* d_out64,
                      hipStream_t s) {
    // one workgroup per CU fits by LDS (133 KB); frames beyond the grid are taken in a grid-stride loop
    const unsigned grid = (unsigned)(n < 256 ? n : 256);
    if (channels == 3)
        hipLaunchKernelGGL(k_down_rect<3>, dim3(grid), dim3(512), 0, s, d_frames, (long long)n, h, w, (const int4*)d_geom, d_out64);
    else
        hipLaunchKernelGGL(k_down_rect<1>, dim3(grid), dim3(512), 0, s, d_frames, (long long)n, h, w, (const int4*)d_geom, d_out64);
}

}  // namespace hvd
