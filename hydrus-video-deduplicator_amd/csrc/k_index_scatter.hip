// k_index_scatter.hip -- the high-byte pass of the pigeonhole index build with a tile's runs laid out in LDS (the build and
// its other kernels: k_hamming_index.hip).
//
// k_index_partition stores each record straight to whichever of the 256 runs its key's high byte selects: a wave's store
// touches ~64 cache lines, and a tile's run of ~16 records is assembled from 16 partial-line writes. This kernel does the
// same pass -- same gate, arguments and result: for every block, partition and tile, the tile's records fill exactly
// their run of rec, in whatever order the atomics give -- but block by block it first orders the tile's 4096 records by
// high byte in LDS (256 counters, ranks from a returning LDS atomic, an exclusive scan, the record stored at lbase[h] + rank)
// and then copies the staged array out with thread e writing staged entry e: the entry's bin comes from the record itself,
// its place from gbase[h] + (e - lbase[h]), so neighbouring lanes write neighbouring records of a run. The hashes are loaded
// once and stay in registers for all 16 blocks; no global atomic, no scratch. hvd_debug_set "index_stage" 0 launches
// k_index_partition instead (launch_index_decide): the independent path of tests/test_gpu_index_scatter.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_index_dev.h"
#include "hvd_kernels.h"

namespace {

using namespace hvd::index_dev;

constexpr uint32_t kTile = 4096u;         // hashes per tile, as k_index_tile_count counted them (k_hamming_index.hip)
constexpr uint32_t kTileThreads = 1024u;  // 16 waves per workgroup, kPer hashes per thread
constexpr uint32_t kPer = kTile / kTileThreads;
static_assert(8u * kTile + 4u * 4u * 256u <= 65536u, "static LDS of k_index_scatter");

// One workgroup per (tile, block group): the grid is (tiles, G), G = 1, 2 or 4 (index_tile_split, k_hamming_index.hip), and
// workgroup (tile, g) does the blocks g 16 / G .. (g + 1) 16 / G - 1 of its tile -- with few tiles (245 at 1 M hashes on 256
// compute units, which hold two of these workgroups each) a second workgroup per tile is worth 6 of 43 us, a third and
// fourth lose 3 (and none is worth anything before the tiles are dealt out as below: the pass then pays for cache lines
// written in pieces, not for waits). A workgroup reads only the words that hold its blocks: the hash in two halves
// (G = 1: the words of the blocks 0 .. 7 now, those of the blocks 8 .. 15 under the copy-out of block 7 -- 16 registers of
// hashes instead of 32, which is what lets 8 waves per SIMD be resident), one half (G = 2) or 8 bytes of it (G = 4).
// Which (tile, group) a workgroup takes: xcd_consecutive (hvd_index_dev.h). A tile's run in a partition is ~16 records at
// any alignment, so its first and last cache line are shared with the runs of the tiles before and behind it; with those
// tiles on the same XCD, at the same block at about the same time, that XCD's L2 puts the line together and writes it
// back once (1 M hashes: 52 -> 43 us with one workgroup per tile).
// Per block three barriers: ranks -> scan -> staged records -> copy-out; the copy-out of block b
// needs none behind it, because nothing it reads (stage, gdelta) is written again before every thread has passed the next
// block's first barrier, which lies behind its own copy-out (gbase for block b + 1 is written between the second and the
// third barrier of block b and read only by the scan between the first and the second).
template <uint32_t G>
__device__ __forceinline__ void scatter_blocks(const uint4* __restrict__ db, uint32_t n, uint32_t ntiles, const uint32_t* __restrict__ tcnt,
                                               const uint32_t* __restrict__ pbase, uint2* __restrict__ rec, uint32_t* bins, uint32_t* lbase,
                                               uint32_t* gdelta, uint32_t* gbase, uint2* stage) {
    constexpr uint32_t kMine = kBlocks / G;                    // blocks of this workgroup
    constexpr uint32_t kHeld = kMine / 2u < 4u ? kMine / 2u : 4u;  // 32-bit words of a hash held at once
    // (tile, group) from the workgroup's place in the grid, consecutive tiles on one XCD: hvd_index_dev.h
    const uint32_t item = xcd_consecutive(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * G);
    const uint32_t tid = threadIdx.x, tile = G == 1u ? item : item % gridDim.x;
    const uint32_t b0 = G == 1u ? 0u : item / gridDim.x * kMine;  // the first of them
    const uint32_t first = tile * kTile;
    const uint32_t held = first < n ? min(kTile, n - first) : 0u;  // records of this tile per block
    if (tid < 256u) bins[tid] = 0u;
    uint32_t w[kPer][kHeld], wn[kPer][kHeld];
    // piece `part` of kHeld words behind the workgroup's first word, b0 / 2
    auto load_words = [&](uint32_t part, uint32_t h[kPer][kHeld]) {
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t i = first + j * kTileThreads + tid;
            if constexpr (kHeld == 4u) {
                const uint4 v = i < n ? db[(size_t)i * 2u + (b0 >> 3) + part] : make_uint4(0u, 0u, 0u, 0u);
                h[j][0] = v.x; h[j][1] = v.y; h[j][2] = v.z; h[j][3] = v.w;
            } else {
                static_assert(kHeld == 2u, "a quarter of a hash's upper or lower half");
                const uint2 v = i < n ? reinterpret_cast<const uint2*>(db)[(size_t)i * 4u + (b0 >> 2) + part] : make_uint2(0u, 0u);
                h[j][0] = v.x; h[j][1] = v.y;
            }
        }
    };
    load_words(0u, w);
    // thread h < 256 fetches the first position of bin h's run inside block b of rec (pbase + the tile's base inside the
    // partition) one block ahead and hands it over in LDS; the first wave scans, lane l the bins 4 l .. 4 l + 3
    const bool scans = tid < 64u, fetches = tid < 256u;
    uint32_t gp = 0u, gt = 0u;  // (their sum is taken where it is used, two barriers behind the loads)
    auto run_base = [&](uint32_t b) {
        gp = pbase[b * 256u + tid];
        gt = tcnt[(size_t)(b * 256u + tid) * ntiles + tile];
    };
    if (fetches) {
        run_base(b0);
        gbase[tid] = gp + gt;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kMine; ++k) {
        const uint32_t b = b0 + k;  // (b0 is even: k says which half of its word block b is)
        uint32_t word[kPer], rank[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            if (k == 2u * kHeld) {
#pragma unroll
                for (uint32_t q = 0; q < kHeld; ++q) w[j][q] = wn[j][q];
            }
            const uint32_t x = w[j][(k >> 1) % kHeld];
            word[j] = (k & 1u) ? (x >> 16 | x << 16) : x;  // key of block b | key of its sibling block << 16
            rank[j] = 0u;
            if (first + j * kTileThreads + tid < n) rank[j] = lds_add(&bins[(word[j] >> 8) & 255u]);
        }
        if (fetches && k + 1u < kMine) run_base(b + 1u);  // in flight under this block's scan and staging
        __syncthreads();
        if (scans) {
            const uint4 c = reinterpret_cast<const uint4*>(bins)[tid];
            reinterpret_cast<uint4*>(bins)[tid] = make_uint4(0u, 0u, 0u, 0u);  // (for the next block's ranks)
            const uint32_t sum = c.x + c.y + c.z + c.w;
            const uint32_t lb = wave_incl_scan(sum, tid) - sum;
            const uint4 l = make_uint4(lb, lb + c.x, lb + c.x + c.y, lb + c.x + c.y + c.z);
            reinterpret_cast<uint4*>(lbase)[tid] = l;
            const uint4 g = reinterpret_cast<const uint4*>(gbase)[tid];
            reinterpret_cast<uint4*>(gdelta)[tid] = make_uint4(g.x - l.x, g.y - l.y, g.z - l.z, g.w - l.w);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t i = first + j * kTileThreads + tid;
            if (i < n) {
                const uint32_t at = lbase[(word[j] >> 8) & 255u] + rank[j];
                if (at < kTile) stage[at] = make_uint2(i, word[j]);  // (always: the bins were counted from these records)
            }
        }
        if (fetches && k + 1u < kMine) gbase[tid] = gp + gt;  // (this block's scan has read gbase: it lies before the last barrier)
        __syncthreads();
        if (k + 1u == 2u * kHeld && k + 1u < kMine) load_words(1u, wn);
        uint2* __restrict__ out = rec + (size_t)b * n;
        uint2 r[kPer];
        uint32_t pos[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) r[j] = stage[j * kTileThreads + tid];  // (entries from `held` on: read, not used)
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) pos[j] = j * kTileThreads + tid + gdelta[(r[j].y >> 8) & 255u];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j)
            if (j * kTileThreads + tid < held && pos[j] < n) out[pos[j]] = r[j];
    }
}

__global__ __launch_bounds__(kTileThreads, 8) void k_index_scatter(const uint4* __restrict__ db, uint32_t n, uint32_t ntiles,
                                                                const uint32_t* __restrict__ tcnt, const uint32_t* __restrict__ pbase,
                                                                uint2* __restrict__ rec, const uint32_t* __restrict__ select) {
    __shared__ alignas(16) uint32_t bins[256];    // records of the tile per high byte; zero between blocks
    __shared__ alignas(16) uint32_t lbase[256];   // the bin's first staged entry
    __shared__ alignas(16) uint32_t gdelta[256];  // gbase[h] - lbase[h] (mod 2^32): staged entry e of bin h goes to rec[b][e + gdelta[h]]
    __shared__ alignas(16) uint32_t gbase[256];   // the first position of the bin's run inside block b of rec
    __shared__ uint2 stage[kTile];
    if (select[hvd::kSelIdxGate] == 0u) return;
    // (the three forms share the tables above: one kernel, whichever grid the host chose)
    if (gridDim.y == 1u) scatter_blocks<1u>(db, n, ntiles, tcnt, pbase, rec, bins, lbase, gdelta, gbase, stage);
    else if (gridDim.y == 2u) scatter_blocks<2u>(db, n, ntiles, tcnt, pbase, rec, bins, lbase, gdelta, gbase, stage);
    else if (gridDim.y == 4u) scatter_blocks<4u>(db, n, ntiles, tcnt, pbase, rec, bins, lbase, gdelta, gbase, stage);
}

}  // namespace

namespace hvd {

hipError_t launch_index_scatter(const uint4* db, uint32_t n, uint32_t ntiles, uint32_t split, const uint32_t* tcnt, const uint32_t* pbase,
                                uint2* rec, const uint32_t* d_select, hipStream_t s) {
    if (split != 1u && split != 2u && split != 4u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_index_scatter, dim3(ntiles, split), dim3(kTileThreads), 0, s, db, n, ntiles, tcnt, pbase, rec, d_select);
    return hipGetLastError();
}

}  // namespace hvd
