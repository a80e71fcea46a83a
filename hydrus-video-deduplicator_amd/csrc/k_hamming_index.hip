// k_hamming_index.hip -- exact pigeonhole index for the auto variant's self all-pairs pass.
//
// Cut the 256 bits into 16 blocks of 16 bits (block b = bits 16b..16b+15 of the packed hash, i.e. half b & 1 of word b >> 1).
// Two hashes within max_dist <= 31 differ in at most 1 bit in at least one block (16 x 2 = 32 > 31); within max_dist <= 15
// they agree in at least one block. With r = 1 (resp. 0) only pairs whose key of some block is within r bits are candidates:
// on uniform hashes ~1/241 of all pairs at 1 M hashes. Every pass rebuilds the index in the context's scratch by a two-level
// counting sort (high byte of the key, then low byte) whose counters live in LDS -- no global atomic per hash, and every
// output region is written from one place:
//   k_index_tile_count  one workgroup per tile of kTile hashes: high-byte digits of all 16 blocks counted in LDS -> tcnt[part][tile]
//   k_index_scan_rows   one wave per partition (block, high byte): exclusive scan over the tiles, the partition's size
//   k_index_scan_parts  one workgroup: every partition's base inside its block, and the list of chunks (a partition larger
//                       than csz entries is cut into several, so that no workgroup sets the length of the passes below)
//   k_index_scatter     (k_index_scatter.hip) the tiles again: record {row, key | sibling key << 16} -> its partition -- the
//                       record carries the whole 32-bit word that holds block b. Block by block the tile's 4096 records
//                       are ranked by a returning LDS atomic, laid out by high byte in LDS and copied out in that order,
//                       so that neighbouring lanes write neighbouring records of a run; with few tiles two workgroups
//                       share a tile's 16 blocks (index_tile_split)
//   k_index_partition   the same pass with every record stored straight from its lane to its run (a wave's store touches
//                       ~64 cache lines): launched instead of k_index_scatter under hvd_debug_set "index_stage" 0, the
//                       independent path of tests/test_gpu_index_scatter.py
//   k_index_order       (k_index_order.hip) one workgroup per partition of at most kOrderMax records: low-byte digits counted,
//                       scanned and ranked in LDS, the partition laid out there in final order and written out as two
//                       contiguous streams -- cnt, off, hw and rows of that partition in one kernel. The three chunk
//                       kernels below skip what it took and serve the larger partitions:
//   k_index_count       one workgroup per chunk: low-byte digits counted in 256 LDS bins
//   k_index_offsets     one workgroup per partition: the chunks' counts -> per-key counts, off[b][h * 256 ..], chunk cursors
//   k_index_stats       a few hundred workgroups of 16 waves stride over the (block, key)s: exact candidates and the longest
//                       work item; a key's count and its 16 neighbours' are loaded at once, for two keys per thread (no
//                       load waits for another), reduced privately, two atomics and a ticket per workgroup; the last workgroup decides
//                       (select[kSelIdxUsed], hvd_kernels.h: index_wins) -- the matrix-core forms return at once when it is set
//   k_index_place       the chunks again: final position from a returning LDS atomic on the bin's cursor; the record's word
//                       -> hw, its row -> rows (the packed DB is not touched)
//   k_index_join        work item (block b, key u): B_u x B_u (positions i < j) and B_u x B_{u ^ (1 << t)} for
//                       the one-bit neighbours above u. First stage on the word that holds block b: a pair within max_dist
//                       has a word within tw = max_dist / 8 bits (8 (tw + 1) > max_dist), and one of that word's two blocks
//                       within tw / 2 = r. Up to kYS y per lane in registers, x through scalar loads (the bucket is contiguous
//                       at a wave-uniform address) that every y of the group meets, xor + popcount + one shift of the
//                       outcome into a per-lane mask per candidate.
//                       Survivors queue up in LDS and are drained 64 at a time: both whole hashes from the packed DB through
//                       rows, the full 256-bit distance, and a pair is emitted only by its CANONICAL block -- the first
//                       block that QUALIFIES (keys within r and word within tw: what lets a candidate reach the full check)
//                       -- so it comes out exactly once, without a dedup pass. A fixed grid: every wave walks runs
//                       of kRun consecutive keys at a grid stride and carries its queue and pair buffer from item to item
// Kernels up to the statistics return at once unless the probe's gate (select[kSelIdxGate]) is set, the last two unless the
// decision is. Nothing waits on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "hvd_index_dev.h"
#include "hvd_kernels.h"

namespace {

using namespace hvd::index_dev;  // kBlocks, kKeys, kParts, orders_whole, lds_add, wave_incl_scan: shared with k_index_order.hip

constexpr uint32_t kWavePairs = 64;  // a wave's pair buffer in LDS (a drain emits at most 64); full -> one atomic reserves room for all of it
constexpr uint32_t kXB = 16;         // x entries per scalar batch of the join: one 64-byte scalar load, one survivor mask per lane
constexpr uint32_t kYS = 4;          // y entries a lane of the join holds at once: a group is 64 kYS entries of an item's y list
static_assert(kYS == 4u && kXB == 16u, "the join packs the masks of two slots, kXB bits each, into a register, and selects among four");
constexpr uint32_t kQueue = 128;    // a wave's survivor queue in LDS (a ring): a push adds at most 64, 64 pending are drained at once
constexpr uint32_t kRun = 4;         // consecutive keys of one block that a wave of the join walks before it strides on
constexpr uint32_t kRuns = 16u * 65536u / kRun;

__device__ __forceinline__ uint32_t key_of(const uint32_t w[8], uint32_t b) { return (w[b >> 1] >> (16u * (b & 1u))) & 0xFFFFu; }

__device__ __forceinline__ void load_words(const uint4* __restrict__ db, uint32_t i, uint32_t w[8]) {
    const uint4 h0 = db[(size_t)i * 2u], h1 = db[(size_t)i * 2u + 1u];
    w[0] = h0.x; w[1] = h0.y; w[2] = h0.z; w[3] = h0.w;
    w[4] = h1.x; w[5] = h1.y; w[6] = h1.z; w[7] = h1.w;
}

constexpr uint32_t kTile = 4096u;                   // hashes per tile: a tile's run in a partition is ~16 records = 128 B
constexpr uint32_t kTileThreads = 1024u;            // 16 waves per workgroup, kTile / kTileThreads hashes per thread
constexpr uint32_t kMinChunk = 4096u;               // a chunk: at most max(kMinChunk, 2 x the mean partition) entries ...
constexpr uint32_t kMaxChunks = kParts + 2048u;     // ... so a pass never has more chunks than this (index_chunk)

// tcnt[part][tile] = the tile's hashes whose key of block (part >> 8) has the high byte (part & 255). Which tile a workgroup
// takes: xcd_consecutive (hvd_index_dev.h) -- a row of tcnt is written 4 bytes per tile, and the tiles whose counts share a
// cache line are counted on one XCD.
__global__ __launch_bounds__(kTileThreads) void k_index_tile_count(const uint4* __restrict__ db, uint32_t n, uint32_t ntiles,
                                                                   uint32_t* __restrict__ tcnt, const uint32_t* __restrict__ select) {
    __shared__ uint32_t bins[kParts];
    if (select[hvd::kSelIdxGate] == 0u) return;
    const uint32_t tid = threadIdx.x, tile = xcd_consecutive(blockIdx.x, ntiles);
    for (uint32_t k = tid; k < kParts; k += kTileThreads) bins[k] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTile / kTileThreads; ++j) {
        const uint32_t i = tile * kTile + j * kTileThreads + tid;
        if (i < n) {
            uint32_t w[8];
            load_words(db, i, w);
#pragma unroll
            for (uint32_t b = 0; b < kBlocks; ++b) (void)lds_add(&bins[b * 256u + (key_of(w, b) >> 8)]);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < kParts; k += kTileThreads) tcnt[(size_t)k * ntiles + tile] = bins[k];
}

// One wave per partition: tcnt[part][.] becomes its exclusive scan over the tiles, ptotal[part] the partition's size.
__global__ __launch_bounds__(256) void k_index_scan_rows(uint32_t* __restrict__ tcnt, uint32_t ntiles, uint32_t* __restrict__ ptotal,
                                                         const uint32_t* __restrict__ select) {
    if (select[hvd::kSelIdxGate] == 0u) return;
    const uint32_t lane = threadIdx.x & 63u, p = blockIdx.x * 4u + (threadIdx.x >> 6);  // < kParts: the grid is exact
    uint32_t* row = tcnt + (size_t)p * ntiles;
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < ntiles; t0 += 64u) {
        const uint32_t t = t0 + lane;
        const uint32_t v = t < ntiles ? row[t] : 0u;
        const uint32_t incl = wave_incl_scan(v, lane);
        if (t < ntiles) row[t] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0u) ptotal[p] = run;
}

// One workgroup, thread t = partitions 4t .. 4t + 3 (wave w = block w): pbase[part] = the partition's first position inside
// its block; pfirst[part] = its first chunk (pfirst[kParts] = chunks of the pass), chunk_p[chunk] = the chunk's partition.
__global__ __launch_bounds__(1024) void k_index_scan_parts(const uint32_t* __restrict__ ptotal, uint32_t csz, uint32_t* __restrict__ pbase,
                                                           uint32_t* __restrict__ pfirst, uint32_t* __restrict__ chunk_p,
                                                           const uint32_t* __restrict__ select) {
    __shared__ uint32_t wsum[16];
    if (select[hvd::kSelIdxGate] == 0u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 tv = reinterpret_cast<const uint4*>(ptotal)[tid];
    const uint32_t tot[4] = {tv.x, tv.y, tv.z, tv.w};
    uint32_t nch[4], size = 0, chunks = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nch[k] = (tot[k] + csz - 1u) / csz;
        size += tot[k];
        chunks += nch[k];
    }
    uint32_t base = wave_incl_scan(size, lane) - size;  // (inside the block: a wave holds exactly one)
    const uint32_t cincl = wave_incl_scan(chunks, lane);
    if (lane == 63u) wsum[wave] = cincl;
    __syncthreads();
    uint32_t first = cincl - chunks;
    for (uint32_t w = 0; w < wave; ++w) first += wsum[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pbase[tid * 4u + k] = base;
        pfirst[tid * 4u + k] = first;
        for (uint32_t c = 0; c < nch[k]; ++c)
            if (first + c < kMaxChunks) chunk_p[first + c] = tid * 4u + k;
        base += tot[k];
        first += nch[k];
    }
    if (tid == 1023u) pfirst[kParts] = min(first, kMaxChunks);
}

// rec[b][pbase + tile base + rank] = {row, key of block b | key of its sibling block b ^ 1 << 16} -- the word that holds block b,
// its own key in the low half whichever half that is: the rank inside the tile's run comes from a returning LDS atomic.
// Block by block, so that the runs a workgroup is filling at any time are few (256 x ~128 B) and soon complete.
__global__ __launch_bounds__(kTileThreads) void k_index_partition(const uint4* __restrict__ db, uint32_t n, uint32_t ntiles,
                                                                  const uint32_t* __restrict__ tcnt, const uint32_t* __restrict__ pbase,
                                                                  uint2* __restrict__ rec, const uint32_t* __restrict__ select) {
    __shared__ uint32_t cur[kParts];
    if (select[hvd::kSelIdxGate] == 0u) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < kParts; k += kTileThreads) cur[k] = pbase[k] + tcnt[(size_t)k * ntiles + blockIdx.x];
    constexpr uint32_t kPer = kTile / kTileThreads;
    uint32_t w[kPer][8];
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t i = blockIdx.x * kTile + j * kTileThreads + tid;
        if (i < n) load_words(db, i, w[j]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t b = 0; b < kBlocks; ++b) {
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const uint32_t i = blockIdx.x * kTile + j * kTileThreads + tid;
            if (i < n) {
                const uint32_t key = key_of(w[j], b);
                const uint32_t pos = lds_add(&cur[b * 256u + (key >> 8)]);
                if (pos < n) rec[(size_t)b * n + pos] = make_uint2(i, key | key_of(w[j], b ^ 1u) << 16);
            }
        }
    }
}

// A chunk's place: partition, block, and its entries [lo, hi) of the partition's records. The chunk kernels serve the
// partitions that k_index_order (k_index_order.hip) left: those of more than kOrderMax records.
struct Chunk {
    uint32_t p, b, lo, hi;
    size_t at;  // the partition's first record inside rec / its first position inside hw and rows (block included)
};
__device__ __forceinline__ bool chunk_of(uint32_t c, uint32_t n, uint32_t csz, const uint32_t* __restrict__ ptotal,
                                         const uint32_t* __restrict__ pbase, const uint32_t* __restrict__ pfirst,
                                         const uint32_t* __restrict__ chunk_p, Chunk* q) {
    if (c >= pfirst[kParts]) return false;
    q->p = chunk_p[c];
    const uint32_t total = ptotal[q->p];
    if (orders_whole(total)) return false;  // k_index_order has ordered this partition
    q->b = q->p >> 8;
    q->lo = (c - pfirst[q->p]) * csz;
    q->hi = min(total, q->lo + csz);
    q->at = (size_t)q->b * n + pbase[q->p];
    return true;
}

// ccount[chunk][low byte] = the chunk's entries with that low byte (the elements are streamed, only the 256 counters are in LDS)
__global__ __launch_bounds__(256) void k_index_count(const uint2* __restrict__ rec, uint32_t n, uint32_t csz,
                                                     const uint32_t* __restrict__ ptotal, const uint32_t* __restrict__ pbase,
                                                     const uint32_t* __restrict__ pfirst, const uint32_t* __restrict__ chunk_p,
                                                     uint32_t* __restrict__ ccount, const uint32_t* __restrict__ select) {
    __shared__ uint32_t bins[256];
    if (select[hvd::kSelIdxGate] == 0u) return;
    Chunk q;
    if (!chunk_of(blockIdx.x, n, csz, ptotal, pbase, pfirst, chunk_p, &q)) return;  // (uniform over the workgroup)
    const uint32_t tid = threadIdx.x;
    bins[tid] = 0u;
    __syncthreads();
    const uint2* __restrict__ r = rec + q.at;
#pragma unroll 4
    for (uint32_t e = q.lo + tid; e < q.hi; e += 256u) (void)lds_add(&bins[r[e].y & 255u]);
    __syncthreads();
    ccount[(size_t)blockIdx.x * 256u + tid] = bins[tid];
}

// One workgroup per partition (b, h), thread t = key h * 256 + t: cnt[b][key] (the statistics read it), off[b][key], and
// ccount[chunk][t] becomes the chunk's cursor: the position inside block b of its first entry with that low byte.
__global__ __launch_bounds__(256) void k_index_offsets(uint32_t n, const uint32_t* __restrict__ ptotal, const uint32_t* __restrict__ pbase,
                                                       const uint32_t* __restrict__ pfirst, uint32_t* __restrict__ ccount,
                                                       uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ select) {
    __shared__ uint32_t wsum[4];
    if (select[hvd::kSelIdxGate] == 0u) return;
    if (orders_whole(ptotal[blockIdx.x])) return;  // k_index_order has written this partition's counts and offsets
    const uint32_t p = blockIdx.x, b = p >> 8, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t c0 = pfirst[p], c1 = min(pfirst[p + 1u], kMaxChunks);
    uint32_t total = 0;
    for (uint32_t c = c0; c < c1; ++c) total += ccount[(size_t)c * 256u + tid];
    const uint32_t incl = wave_incl_scan(total, lane);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    uint32_t pos = pbase[p] + incl - total;
    for (uint32_t w = 0; w < wave; ++w) pos += wsum[w];
    const uint32_t key = (p & 255u) * 256u + tid;
    cnt[b * kKeys + key] = total;
    off[(size_t)b * (kKeys + 1u) + key] = pos;
    if (key == kKeys - 1u) off[(size_t)b * (kKeys + 1u) + kKeys] = n;
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t v = ccount[(size_t)c * 256u + tid];
        ccount[(size_t)c * 256u + tid] = pos;
        pos += v;
    }
}

constexpr uint32_t kStatsGrid = 256u;      // workgroups of the statistics: each ends in two atomics and a ticket
constexpr uint32_t kStatsThreads = 1024u;  // 16 waves: at 256 workgroups four waves per SIMD, each with kStatsPer entries in flight
constexpr uint32_t kStatsPer = 2u;         // entries of a thread whose loads are issued together (2 x 17 loads)

// Candidates of key u in its block: C(c_u, 2) + (r = 1) c_u x c_v over the one-bit neighbours v = u ^ (1 << t) above u --
// the exact number of pairs whose keys of this block are within r, i.e. the pairs the join walks for this work item.
// The kernel waits for its loads and for nothing else (the counts come from the other dies' k_index_order: at best the
// Infinity Cache), so no load depends on another: an entry's own count and its 16 neighbours' counts are loaded
// unconditionally -- a neighbour below u is masked out afterwards -- and kStatsPer entries of a thread are loaded before
// the first is used.
__global__ __launch_bounds__(kStatsThreads) void k_index_stats(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ select,
                                                               const hvd::IndexRule q) {
    if (select[hvd::kSelIdxGate] == 0u) return;
    // the workgroups stride over the kBlocks * kKeys (block, key)s and reduce privately
    unsigned long long cand = 0;
    uint32_t mx = 0;
    const uint32_t stride = gridDim.x * kStatsThreads;
    for (uint32_t t0 = blockIdx.x * kStatsThreads + threadIdx.x; t0 < kBlocks * kKeys; t0 += kStatsPer * stride) {
        uint32_t c[kStatsPer], nb[kStatsPer][16];
#pragma unroll
        for (uint32_t k = 0; k < kStatsPer; ++k) {
            const uint32_t t = min(t0 + k * stride, kBlocks * kKeys - 1u);  // (an entry past the end: loaded, not used)
            const uint32_t u = t & (kKeys - 1u);
            const uint32_t* __restrict__ cb = cnt + (t & ~(kKeys - 1u));
            c[k] = cb[u];
            if (q.r != 0u) {  // (uniform over the grid)
#pragma unroll
                for (uint32_t s = 0; s < 16u; ++s) nb[k][s] = cb[u ^ (1u << s)];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kStatsPer; ++k) {
            const uint32_t t = t0 + k * stride, u = t & (kKeys - 1u);
            if (t >= kBlocks * kKeys) break;
            const unsigned long long cu = c[k];
            unsigned long long ylen = cu;
            cand += cu * (cu - (cu != 0ull)) / 2ull;
            if (q.r != 0u) {
#pragma unroll
                for (uint32_t s = 0; s < 16u; ++s) ylen += ((u >> s) & 1u) == 0u ? nb[k][s] : 0u;
                cand += cu * (ylen - cu);
            }
            // the work item's walk: its wave steps its c x's over a y list of ylen entries (saturated: any such item loses
            // anyway; an empty bucket has no walk)
            mx = max(mx, (uint32_t)min(cu * ylen, 0xFFFFFFFFull));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        cand += __shfl_down(cand, off);
        mx = max(mx, (uint32_t)__shfl_down((int)mx, off));
    }
    constexpr uint32_t kWaves = kStatsThreads / 64u;
    __shared__ unsigned long long part[kWaves];
    __shared__ uint32_t partm[kWaves];
    if ((threadIdx.x & 63u) == 0u) {
        part[threadIdx.x >> 6] = cand;
        partm[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    unsigned long long sum = 0;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        sum += part[w];
        m = max(m, partm[w]);
    }
    unsigned long long* cand_w = reinterpret_cast<unsigned long long*>(select + hvd::kSelIdxCand);
    // (as the probe: the sums travel in returning atomics, and the ticket is taken after they have returned)
    unsigned long long seen = 0;
    if (sum) seen += atomicAdd(cand_w, sum);
    if (m) seen += atomicMax(&select[hvd::kSelIdxMaxWalk], m);
    asm volatile("" ::"v"(seen));
    if (atomicAdd(&select[hvd::kSelIdxTicket], 1u) == gridDim.x - 1u) {
        const unsigned long long total = atomicAdd(cand_w, 0ull);
        const uint32_t big = atomicMax(&select[hvd::kSelIdxMaxWalk], 0u);
        const uint32_t form = atomicAdd(&select[0], 0u);
        select[hvd::kSelIdxUsed] = hvd::index_wins(q, (double)total, (double)big, form) ? 1u : 0u;
    }
}

// hw[b][pos] = the record's word (key of block b | sibling key << 16: what the join compares first), rows[b][pos] = row, in
// key order: pos from a returning LDS atomic on the bin's cursor (order inside a bucket: whatever the atomics give -- the
// join's rule does not depend on it). Records in, words and rows out: the packed DB is not read.
// The chunks of a partition fill its region of hw and rows completely, and nobody else writes there.
__global__ __launch_bounds__(256) void k_index_place(const uint2* __restrict__ rec, uint32_t n, uint32_t csz,
                                                     const uint32_t* __restrict__ ptotal, const uint32_t* __restrict__ pbase,
                                                     const uint32_t* __restrict__ pfirst, const uint32_t* __restrict__ chunk_p,
                                                     const uint32_t* __restrict__ ccount, uint32_t* __restrict__ hw, uint32_t* __restrict__ rows,
                                                     const uint32_t* __restrict__ select) {
    __shared__ uint32_t cur[256];
    if (select[hvd::kSelIdxUsed] == 0u) return;
    Chunk q;
    if (!chunk_of(blockIdx.x, n, csz, ptotal, pbase, pfirst, chunk_p, &q)) return;  // (uniform over the workgroup)
    const uint32_t tid = threadIdx.x;
    cur[tid] = ccount[(size_t)blockIdx.x * 256u + tid];
    __syncthreads();
    const uint2* __restrict__ r = rec + q.at;
    const size_t base = (size_t)q.b * n;
    constexpr uint32_t kU = 4u;  // entries per thread in flight: their loads overlap
    for (uint32_t e0 = q.lo; e0 < q.hi; e0 += 256u * kU) {
        uint2 rc[kU];
        uint32_t pos[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t e = e0 + u * 256u + tid;
            rc[u] = e < q.hi ? r[e] : make_uint2(n, 0u);  // (row n: no entry)
        }
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) pos[u] = rc[u].x < n ? lds_add(&cur[rc[u].y & 255u]) : n;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u)
            if (pos[u] < n) {
                hw[base + pos[u]] = rc[u].y;
                rows[base + pos[u]] = rc[u].x;
            }
    }
}

// The index as the join reads its x side: constant address space, so that a wave-uniform address is read by scalar loads
// (the index is read-only for the whole kernel) and the words reach the xor as scalar operands. A bucket begins at any
// word, so a batch of kXB words is aligned to 4 bytes only.
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef u32x16 u32x16w __attribute__((aligned(4)));
typedef const __attribute__((address_space(4))) uint32_t kxw;
typedef const __attribute__((address_space(4))) u32x16w kx16;

// One candidate of the first stage: fails = fails << 1 | (popcount(x ^ y) > tw). The popcount accumulates onto
// kfail = 2^31 - 1 - tw, so bit 31 of the sum is "more than tw bits differ", and one v_alignbit of {fails, sum} by 31 shifts
// that bit in: xor, popcount, align -- three VALU instructions, no compare and no condition code between them
__device__ __forceinline__ uint32_t word_step(uint32_t fails, uint32_t x, uint32_t y, uint32_t kfail) {
    const uint32_t d = (uint32_t)__popc(x ^ y) + kfail;
    return __builtin_amdgcn_alignbit(fails, d, 31u);
}

struct JoinArgs {
    const uint32_t* off;
    const uint32_t* hw;
    const uint32_t* rows;
    const uint4* db;
    uint32_t n;
    const int32_t* group;
    hvd_pair* out;
    unsigned long long cap;
    unsigned long long* count;
    uint32_t max_dist, r, tw, rank, world;
};

// The join's arguments as read where they are needed: what only a flush or the group filter uses (out, cap, count, group) is
// loaded there, once in thousands of items, and holds no scalar register for the whole kernel (JoinArgs is the kernel's
// first argument: offset 0 of the kernel's argument segment).
__device__ __forceinline__ const JoinArgs* rare_args() {
    const JoinArgs* p = (const JoinArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// A wave's buffered pairs -> global: one atomic reserves room for all of them; beyond `cap` nothing is written but the count
// still grows (the caller reports HVD_ERR_OVERFLOW with the number needed).
__device__ __forceinline__ void flush_wave(const hvd_pair* buf, uint32_t fill, uint32_t lane) {
    const JoinArgs& a = *rare_args();
    unsigned long long base = 0;
    if (lane == 0u) base = atomicAdd(a.count, (unsigned long long)fill);
    base = __shfl(base, 0);
    for (uint32_t k = lane; k < fill; k += 64u)
        if (base + k < a.cap) a.out[base + k] = buf[k];
}

// Work item = (block b, key u); item (b << 16 | u) belongs to rank item mod world. The grid is sized by the device, not by
// the work (index_join_workgroups): wave w of G walks the runs w, w + G, ... of kRun consecutive keys of one block (run = item / kRun, static: no
// workgroup waits for another and no counter is shared), inside a run only the items of its rank (the first one from one
// modulo per run, then steps of world). The offsets of the next item of the sequence are loaded before the current one is
// walked, so no item begins behind a fresh launch and three dependent loads. The survivor queue, the pair buffer and their
// scalar counters live for the whole wave: a drain happens when 64 survivors are pending and once at the wave's end, a
// flush when the pair buffer cannot take a drain's pairs and once at the end. A queue entry CARRIES ITS BLOCK (qblk, a byte
// beside the two positions), so survivors of block b may be drained while the wave walks another block: the rows and the
// ownership verdict come from the entry's block, never from the item being walked. Everything else is per item and is set
// up afresh by walk(): the segment table (incl, delta, ny), the cursor (nzm, ce, dl), the y registers and ylim.
// The y list of an item is
// its own bucket (segment 0) followed by the buckets u ^ (1 << t) > u (r = 1): a group is 64 kYS consecutive entries of it,
// and a lane holds up to kYS y -- slot s = entry 64 s + lane of the group; one word each: the key of block b and, above
// it, the key of its sibling block -- in registers. The loops are group outside, x batch inside, slot innermost: all y
// loads of a group and its first x batch are in flight together, and every x batch is read once per group -- at 1 M
// hashes nearly every y list (~138 entries) is one group -- and meets all slots that hold an entry. The x side is the
// bucket itself, contiguous at a wave-uniform address: kXB words per scalar batch, xor'ed as scalar operands. Per candidate: xor, popcount onto a constant that carries
// "more than tw = max_dist / 8 bits" into bit 31, and that bit shifted into the lane's mask. All kXB words are read whatever the bucket holds,
// but only the quarters of a batch that hold an x are stepped; the mask keeps only the x
// that exist and, inside the own bucket, only those before the lane's y (x index k pairs with a y iff k < ylim). The kernel
// is bound by the instructions its waves issue, not by what they wait for (fetching an item's y, x and rows
// further ahead measured slower, every instruction taken out measured faster), so the loops are written for few of them. A
// candidate's key is within r and its sibling key is unrelated (~8 of 16 bits differ), so about one in a hundred survives
// (same bucket) or one in five hundred (neighbour): the survivors' {x position, y position} inside their block go into the
// wave's queue in LDS -- once per batch for all slots together --, and whenever 64 are pending each lane takes one: both rows, both whole
// hashes from the packed DB, the exact distance, the ownership rule, the group filter, the pair buffer.
// Positions inside the own bucket are the first nu entries of the y list.
__global__ __launch_bounds__(256) void k_index_join(const JoinArgs a, const uint32_t* __restrict__ select) {
    __shared__ hvd_pair pbuf[4][kWavePairs];
    __shared__ uint2 qbuf[4][kQueue];
    __shared__ uint8_t qblk[4][kQueue];
    __shared__ uint32_t yposb[4][kYS * 64u];
    if (select[hvd::kSelIdxUsed] == 0u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wid = blockIdx.x * 4u + wave, nwaves = gridDim.x * 4u;  // (wave-uniform; nothing below synchronises across waves)
    constexpr uint32_t kEnd = 0xFFFFFFFFu;  // no item
    // the first item of this rank in the runs run, run + nwaves, ... (a run shorter than world may hold none)
    auto first_in = [&](uint32_t run) {
        for (; run < kRuns; run += nwaves) {
            const uint32_t i0 = run * kRun, m = i0 % a.world;
            const uint32_t f = i0 + (a.rank >= m ? a.rank - m : a.rank + a.world - m);
            if (f < i0 + kRun) return f;
        }
        return kEnd;
    };
    // an item's offset pairs: lane 0 the bucket itself, lane 1 + t the bucket u ^ (1 << t) if that key lies above u (the
    // other lanes read the bucket's own pair and do not use it)
    auto offsets = [&](uint32_t item, uint32_t* vs, uint32_t* ve) {
        const uint32_t u = item & (kKeys - 1u), t = (lane - 1u) & 15u;
        const bool nb = lane >= 1u && lane <= 16u && a.r != 0u && ((u >> t) & 1u) == 0u;
        const uint32_t* __restrict__ o = a.off + (size_t)(item >> 16) * (kKeys + 1u) + (nb ? u ^ (1u << t) : u);
        *vs = o[0];
        *ve = o[1];
    };
    uint32_t item = first_in(wid);
    if (item == kEnd) return;
    const uint32_t kfail = 0x7FFFFFFFu - a.tw;  // popcount + kfail reaches bit 31 iff popcount > tw
    uint32_t fill = 0;       // wave-uniform: pairs in the buffer
    uint32_t qh = 0, qt = 0;  // wave-uniform: the queue holds entries qh .. qt - 1 (mod kQueue), fewer than 64 between pushes
    hvd_pair* buf = pbuf[wave];
    uint2* queue = qbuf[wave];
    uint8_t* qb = qblk[wave];
    uint32_t* ypl = yposb[wave];

    // the first cnt (<= 64) queued survivors, one per lane: the full check
    auto drain = [&](uint32_t cnt) {
        __builtin_amdgcn_wave_barrier();  // (the pushes are in LDS before the entries are read)
        bool emit = false;
        uint32_t d = 0, ri = 0, rj = 0, eb = 0, dw[8];
        if (lane < cnt) {
            const uint2 e = queue[(qh + lane) & (kQueue - 1u)];
            eb = qb[(qh + lane) & (kQueue - 1u)];  // the entry's block: its positions are inside that block
            const uint32_t* __restrict__ rowb = a.rows + (size_t)eb * a.n;
            ri = rowb[e.x];
            rj = rowb[e.y];
            uint32_t wx[8], wy[8];
            load_words(a.db, ri, wx);
            load_words(a.db, rj, wy);
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                dw[k] = wx[k] ^ wy[k];
                d += (uint32_t)__popc(dw[k]);
            }
            emit = d <= a.max_dist;
        }
        qh += cnt;
        // ownership and the group filter only when some lane of the wave is within max_dist (wave-uniform): about one
        // survivor in seven thousand is on uniform hashes, so almost every drain ends here, after the eight popcounts
        if (!__any(emit)) return;
        if (emit) {
            // bit b2: block b2 qualifies -- its keys are within r and its word within tw (shifted in from the top block down:
            // a constant 1 << b2 per block would hold a vector register each for the whole kernel)
            uint32_t qual = 0;
#pragma unroll
            for (uint32_t b2 = kBlocks; b2-- > 0u;)
                qual = qual << 1 | ((uint32_t)__popc(key_of(dw, b2)) <= a.r && (int32_t)((uint32_t)__popc(dw[b2 >> 1]) + kfail) >= 0 ? 1u : 0u);
            if ((qual & ((1u << eb) - 1u)) != 0u) emit = false;  // an earlier qualifying block owns this pair
            const int32_t* __restrict__ group = rare_args()->group;
            if (emit && group != nullptr && group[ri] == group[rj]) emit = false;
        }
        const unsigned long long em = __ballot(emit);
        const uint32_t m = (uint32_t)__popcll(em);
        if (m == 0u) return;
        if (fill + m > kWavePairs) {
            flush_wave(buf, fill, lane);
            fill = 0;
        }
        if (emit) {
            const uint32_t slot = fill + __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
            hvd_pair rec;
            rec.i = min(ri, rj);
            rec.j = max(ri, rj);
            rec.dist = d;
            rec.pad = 0;
            buf[slot] = rec;
        }
        fill += m;
    };
    // One item, its offset pairs in vstart / vend: every value below is the item's own.
    auto walk = [&](uint32_t item, uint32_t vstart, uint32_t vend) {
        const uint32_t b = item >> 16, u = item & (kKeys - 1u);
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)vstart);
        const uint32_t nu = (uint32_t)__builtin_amdgcn_readfirstlane((int)vend) - s0;
        if (nu == 0u) return;
        const bool seg = lane == 0u || (lane <= 16u && a.r != 0u && ((u >> ((lane - 1u) & 15u)) & 1u) == 0u);
        const uint32_t sstart = seg ? vstart : 0u;
        const uint32_t ssize = seg ? vend - vstart : 0u;
        // inclusive scan over the lanes 0 .. 16 in the data path (no LDS, no index registers): four shifts inside the row of
        // 16 lanes, then lane 15 onto the row above
        uint32_t incl = ssize;
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, true);  // row_shr:1
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, true);  // row_shr:2
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, true);  // row_shr:4
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, true);  // row_shr:8
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, true);  // row_bcast:15 onto rows 1 and 3
        const int delta = (int)sstart - (int)(incl - ssize);  // position = p + delta for an entry p of this segment
        // (segment s ends at the incl of lane s, the last one, 16, at ny; the lanes 17 .. 31 hold ny too, the rest is not read)
        const uint32_t ny = (uint32_t)__builtin_amdgcn_readlane((int)incl, 16);
        const size_t base = (size_t)b * a.n;
        const uint32_t* __restrict__ hb = a.hw + base;
        // (a batch reads kXB words whatever the bucket holds: at most kXB - 1 words past the block's last position, and behind
        // the last block's hw lie the rows, 16 n >= 32 words, in the same allocation)
        kxw* xb = (kxw*)(a.hw + base + s0);
        // The y side of a group: a lane holds up to kYS y -- slot s is entry g0 + 64 s + lane of the y list --, their words,
        // their positions inside block b and ylim: x index k pairs with the y iff k < ylim, inside the bucket (the first nu
        // entries) only the x before it (positions i < j), past the list none.
        // The positions are needed only when a survivor is pushed, by a slot that differs from lane to lane: they wait in
        // LDS (ypl[64 s + lane]: a lane reads what it wrote itself) and hold no register under the steps.
        uint32_t yw[kYS], ylim[kYS];
        // One batch of kXB x words (x index k0 ..) against the first NS slots (wave-uniform: the slots that hold an entry):
        // bit 4 nq - 1 - j of a slot's mask = x k0 + j survives; two slots' masks to a register, the even slot below. Only
        // the quarters of the batch that hold an x are stepped (wave-uniform: the bucket's last batch is short, and the mean
        // bucket of 15 at 1 M hashes fills 70 % of whole batches, 93 % of quarters): nq, the shift and every quarter branch
        // once per batch, whatever NS is.
        auto steps = [&](auto ns_tag, const u32x16& x, uint32_t k0, uint32_t* m01, uint32_t* m23) {
            constexpr uint32_t NS = decltype(ns_tag)::value;
            uint32_t fails[NS];
#pragma unroll
            for (uint32_t s = 0; s < NS; ++s) fails[s] = 0u;
            const uint32_t nq = min(kXB / 4u, (nu - k0 + 3u) / 4u);
#pragma unroll
            for (uint32_t s = 0; s < NS; ++s)
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) fails[s] = word_step(fails[s], x[j], yw[s], kfail);
            if (nq > 1u) {
#pragma unroll
                for (uint32_t s = 0; s < NS; ++s)
#pragma unroll
                    for (uint32_t j = 4u; j < 8u; ++j) fails[s] = word_step(fails[s], x[j], yw[s], kfail);
                if (nq > 2u) {
#pragma unroll
                    for (uint32_t s = 0; s < NS; ++s)
#pragma unroll
                        for (uint32_t j = 8u; j < 12u; ++j) fails[s] = word_step(fails[s], x[j], yw[s], kfail);
                    if (nq > 3u) {
#pragma unroll
                        for (uint32_t s = 0; s < NS; ++s)
#pragma unroll
                            for (uint32_t j = 12u; j < 16u; ++j) fails[s] = word_step(fails[s], x[j], yw[s], kfail);
                    }
                }
            }
            // after 4 nq steps the outcome of x k0 + j is at bit 4 nq - 1 - j, and there it stays (the push knows nq): the
            // y pairs with the first c x of the batch, the top c of those 4 nq bits (c <= 4 nq, since ylim <= nu)
            const uint32_t sh = kXB - 4u * nq, top = 0xFFFF0000u >> sh, all = 0xFFFFu >> sh;
            uint32_t mask[kYS];
#pragma unroll
            for (uint32_t s = 0; s < kYS; ++s) {
                mask[s] = 0u;
                if (s < NS) {
                    const int c = min(max((int)ylim[s] - (int)k0, 0), (int)kXB);
                    mask[s] = ~fails[s] & (top >> c) & all;
                }
            }
            *m01 = mask[0] | mask[1] << 16;
            *m23 = mask[2] | mask[3] << 16;
        };
        // The survivors of one batch, all slots together: one per lane and turn, so at most 64 join the fewer than 64
        // pending and the push always fits (a batch without a survivor in any slot leaves at once: one compare and one
        // branch). A lane takes its lowest mask bit: bit t of m01 (else of m23) is slot t / 16 (+ 2), x k0 + 4 nq - 1 - t % 16.
        auto push = [&](uint32_t k0, uint32_t m01, uint32_t m23) {
            if (!__any((m01 | m23) != 0u)) return;
            const uint32_t xtop = s0 + k0 + min(kXB, (nu - k0 + 3u) & ~3u) - 1u;  // the position of the x at bit 0 of a mask
            do {
                const bool has = (m01 | m23) != 0u;
                const unsigned long long bal = __ballot(has);
                if (has) {
                    const uint32_t slot = (qt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))) &
                                          (kQueue - 1u);
                    const bool lo = m01 != 0u;
                    const uint32_t t = (uint32_t)__builtin_ctz(lo ? m01 : m23);
                    const bool up = t >= kXB;
                    const uint32_t yp = ypl[64u * ((lo ? 0u : 2u) + (up ? 1u : 0u)) + lane];
                    queue[slot] = make_uint2(xtop - (t & (kXB - 1u)), yp);
                    qb[slot] = (uint8_t)b;
                    if (lo) m01 &= m01 - 1u;
                    else m23 &= m23 - 1u;
                }
                qt += (uint32_t)__popcll(bal);
                if (qt - qh >= 64u) drain(64u);
            } while (__any((m01 | m23) != 0u));
        };
        // The position inside block b of the entries q0 + lane of the y list, for the slots in their order: p + the delta of
        // the entry's segment. The cursor -- all of it wave-uniform -- only moves forward over the segments that hold an
        // entry (nzm: those still ahead): ce is the end of the current one, dl its delta. Every lane takes the current delta;
        // for each segment that begins inside the slot, at lane ce - q0, the lanes from there on take that one's instead:
        // its end and delta read from the lane that holds them, one add and one select by a lane mask made by a scalar shift.
        // No compare per lane, nothing for an empty segment, and one add for a slot inside a long segment.
        uint32_t nzm = (uint32_t)__ballot(ssize != 0u) & 0x1FFFEu;  // (segment 0 is the bucket: nu > 0, and it is the current one)
        uint32_t ce = nu;
        int dl = (int)s0;
        auto locate = [&](uint32_t q0) {
            const uint32_t p = q0 + lane;
            uint32_t yp = (uint32_t)((int)p + dl);
            const uint32_t lim = min(q0 + 64u, ny);
            while (ce < lim) {  // (an end below ny: a further segment holds an entry; q0 <= ce, the slot's first entry is the current segment's or ce itself)
                const unsigned long long from = ~0ull << (ce - q0);
                const int cs = __builtin_ctz(nzm);
                nzm &= nzm - 1u;
                ce = (uint32_t)__builtin_amdgcn_readlane((int)incl, cs);
                dl = __builtin_amdgcn_readlane(delta, cs);
                // (the select takes the scalar mask as it is: written in C++ it would need a compare per lane to make one)
                const uint32_t moved = (uint32_t)((int)p + dl);
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(yp) : "v"(moved), "s"(from));
            }
            return yp;
        };
        uint32_t g0 = 0;
        do {  // (ny >= nu > 0: at least one group, and its slot 0 holds an entry)
            // the slots that hold an entry (wave-uniform), located in their order -- the cursor only moves forward --, and
            // all their y loads and the first x batch in flight together
            const uint32_t ns = min(kYS, (ny - g0 + 63u) / 64u);
#pragma unroll
            for (uint32_t s = 0; s < kYS; ++s) {
                yw[s] = 0u;
                ylim[s] = 0u;
                if (s < ns) {
                    const uint32_t p = g0 + 64u * s + lane;
                    const uint32_t yp = locate(g0 + 64u * s);
                    if (p < ny) yw[s] = hb[yp];
                    ylim[s] = p >= ny ? 0u : min(p, nu);
                    ypl[64u * s + lane] = yp;
                }
            }
            u32x16 x = *(kx16*)xb;
            for (uint32_t k0 = 0;;) {  // every x batch is loaded once per group and meets all its slots
                uint32_t m01, m23;
                if (ns > 2u) {
                    if (ns > 3u) steps(std::integral_constant<uint32_t, 4u>(), x, k0, &m01, &m23);
                    else steps(std::integral_constant<uint32_t, 3u>(), x, k0, &m01, &m23);
                } else {
                    if (ns > 1u) steps(std::integral_constant<uint32_t, 2u>(), x, k0, &m01, &m23);
                    else steps(std::integral_constant<uint32_t, 1u>(), x, k0, &m01, &m23);
                }
                push(k0, m01, m23);
                k0 += kXB;
                if (k0 >= nu) break;
                x = *(kx16*)(xb + k0);
            }
            g0 += 64u * kYS;
        } while (g0 < ny);
    };
    uint32_t vstart, vend;
    offsets(item, &vstart, &vend);
    for (;;) {
        // the next item of the sequence: the next one of this rank inside the run, or the first of the wave's next run
        uint32_t next = item + a.world;
        if ((next ^ item) >= kRun) next = first_in(item / kRun + nwaves);
        uint32_t vstart_n = 0u, vend_n = 0u;
        if (next != kEnd) offsets(next, &vstart_n, &vend_n);  // in flight under this item's walk
        walk(item, vstart, vend);
        if (next == kEnd) break;
        item = next;
        vstart = vstart_n;
        vend = vend_n;
    }
    if (qt != qh) drain(qt - qh);
    if (fill != 0u) flush_wave(buf, fill, lane);
}

}  // namespace

namespace hvd {

int g_allpairs_index = -1;
int g_allpairs_index_fail = 0;
int g_index_join_wgs = 0;
int g_index_stage = 1;
int g_index_tile_split = 0;

// per-context scratch: per-key counts [16][65536], offsets [16][65537], words [16][n] x 4 B, rows [16][n] x 4 B -- in this
// order: the join's scalar batch reads up to 15 words past a bucket's end, which behind the last block's words are rows --;
// for the build: partition records [16][n] x 8 B, tile counts [4096][tiles], and per partition / chunk: sizes, bases, first
// chunks, the chunk list and the chunks' low-byte counts (cursors). 16 B per hash and block: 0.27 GB at 1 M, 2.6 GB at 10 M
struct IndexScratch {
    void* p = nullptr;
    size_t cap = 0;
};
constexpr int kMaxIdxCtx = 16;
static IndexScratch g_idx[kMaxIdxCtx];
static std::mutex g_idx_mu;

static size_t off_words() { return ((size_t)kBlocks * (kKeys + 1u) + 3u) & ~(size_t)3u; }
static uint32_t index_tiles(uint32_t n) { return (n + kTile - 1u) / kTile; }
// Entries per chunk: at least twice the mean partition (n / 256), so the 16 n entries of a pass make at most 4096 + 2048 chunks.
static uint32_t index_chunk(uint32_t n) { return max(kMinChunk, 2u * ((n + 255u) / 256u)); }
static size_t tcnt_words(uint32_t n) { return ((size_t)kParts * index_tiles(n) + 3u) & ~(size_t)3u; }
constexpr size_t kPartWords = 3u * kParts + 4u + kMaxChunks;  // ptotal, pbase, pfirst (+ 1, padded), chunk_p
static size_t index_bytes(uint32_t n) {
    return 4u * (size_t)kBlocks * kKeys + 4u * off_words() + (size_t)kBlocks * n * 4u + (size_t)kBlocks * n * 4u +
           (size_t)kBlocks * n * 8u + 4u * tcnt_words(n) + 4u * kPartWords + 4u * (size_t)kMaxChunks * 256u;
}
struct IndexPtrs {
    uint32_t* cnt;
    uint32_t* off;
    uint32_t* hw;
    uint32_t* rows;
    uint2* rec;
    uint32_t *tcnt, *ptotal, *pbase, *pfirst, *chunk_p, *ccount;
};
static IndexPtrs index_ptrs(int ctx_id, uint32_t n) {
    char* p = (char*)g_idx[ctx_id].p;
    IndexPtrs q;
    q.cnt = (uint32_t*)p;
    q.off = (uint32_t*)(p + 4u * (size_t)kBlocks * kKeys);
    q.hw = (uint32_t*)(p + 4u * (size_t)kBlocks * kKeys + 4u * off_words());
    q.rows = q.hw + (size_t)kBlocks * n;
    q.rec = (uint2*)(q.rows + (size_t)kBlocks * n);  // (32 n words behind a 16-byte boundary: aligned)
    q.tcnt = (uint32_t*)(q.rec + (size_t)kBlocks * n);
    q.ptotal = q.tcnt + tcnt_words(n);
    q.pbase = q.ptotal + kParts;
    q.pfirst = q.pbase + kParts;
    q.chunk_p = q.pfirst + kParts + 4u;
    q.ccount = q.chunk_p + kMaxChunks;
    return q;
}

bool index_eligible(const AllPairsArgs& a, bool rect, uint32_t* r) {
    if (g_allpairs_index == 0 || rect || a.sink.set != nullptr || a.d_db == nullptr || a.max_dist > 31u || a.n < 2u) return false;
    if (a.ctx_id < 0 || a.ctx_id >= kMaxIdxCtx) return false;
    *r = a.max_dist >= 16u ? 1u : 0u;
    // (a small DB never pays for the index's fixed cost: no scratch, no launches; any matrix-core form may be the probe's)
    return g_allpairs_index == 1 || index_wins(index_rule(a, *r), 0.0, 0.0, 0u);
}

IndexRule index_rule(const AllPairsArgs& a, uint32_t r) {
    IndexRule q;
    q.pairs = (double)a.n * (double)(a.n - 1u) / 2.0;
    q.n = (double)a.n;
    q.r = r;
    q.force = g_allpairs_index == 1 ? 1u : 0u;
    q.world = a.world;
    // (DESIGN 4.1, 1 M uniform hashes on MI355X: form 9 18.1 ms = 36 fs per comparison, forms 18 / 12 +4 / +11 %. From the
    // kernel trace of the join with fewer instructions per item (profiles/r17_index_kernel_stats_after.csv): join 0.638 ms
    // for 2.075e9 candidates = 0.31 ps each; the counting sort, the statistics and the place pass -- every kernel between
    // probe and join -- 0.352 ms, of which ~0.03 ms do not depend on n (the scans over 4096 partitions, the grid of 6144
    // chunks): 0.32 ns per hash, kept at 0.33, and those 30 us next to the 40 us of launches. To re-derive after a change
    // of these kernels: ps_cand = join time / candidates, ps_hash = (every kernel between probe and join - what of them
    // does not depend on n) / n, ps_crit from the crowded DB of scripts/gpu_index_join_time.py (profiles/r17_index_join_time.jsonl): 200 000 hashes,
    // 5 000 of them in one bucket, a longest walk of 25.15e6 pairs, 8.07 .. 8.13 ms per call of which ~0.2 ms are what
    // the other terms price and ~0.4 ms copies: 0.30 ns per pair, 19 ns per step of 64 -- rounded up, which errs towards
    // the matrix cores. The wave that walks the crowded bucket also walks the other 15 items of its sequence, ~50 us at
    // 1 M: the terms ADD, which prices that.
    // With the partitions that fit LDS ordered whole (k_index_order.hip; profiles/r21_index_kernel_stats_after.csv): every
    // kernel between probe and join 0.245 ms, of which 0.025 ms do not depend on n (the two scans and the three chunk
    // kernels, whose workgroups all return): 0.22 ns per hash. That is the price up to ~1.4 M uniform hashes, which is where
    // the rule decides anything: beyond, the partitions outgrow kOrderMax and a hash costs the 0.33 ns of the chunk kernels
    // again, 1 ms more at 10 M than this term says, in a pass that wins by a factor of forty. fixed_ns: those 25 us, 43 us
    // of launches (one more) and the three fall-back launches on their coarse grid, 19 us: 87 us, rounded up.
    // With the high-byte pass staged in LDS (k_index_scatter.hip) and the statistics free of dependent loads
    // (profiles/r22_index_kernel_stats_after.csv): every kernel between probe and join 0.157 ms. Of these the two scans and
    // the three chunk kernels, 25 us, do not depend on n, and neither do the statistics, 17 us, which load all 16 x 65 536
    // counts whatever n is: the tile count, the scatter and the order pass, 0.116 ms, are 0.12 ns per hash. fixed_ns: those
    // 42 us, 43 us of launches (as many as before) and 21 us of fall-back launches: 106 us, rounded up.
    // With a lane's y in groups of kYS slots and every x batch read once per group (profiles/r24_kernel_stats_after.csv,
    // profiles/r24_index_join_time.jsonl): join 0.601 ms for 2.075e9 candidates = 0.29 ps each; the crowded DB 5.83 .. 5.85
    // ms per call, less the same ~0.6 ms, over 25.15e6 pairs = 0.21 ns per pair, rounded up.
    // With the tiles dealt to the XCDs in consecutive ranges and two workgroups per tile in the scatter
    // (profiles/r25_kernel_stats_after.csv): the tile count 12.8, the scatter 37.2 and the order pass 49.7 us, 0.100 ms =
    // 0.10 ns per hash; the kernels whose length does not depend on n and the launches are what they were: fixed_ns stays)
    q.fs_mfma_fetch = 36.0f;
    q.fs_mfma_other = 40.0f;
    q.ps_cand = 0.29f;
    q.ps_hash = 100.0f;
    q.ps_crit = 220.0f;
    q.fixed_ns = 110000.0f;
    return q;
}

hipError_t index_reserve(int ctx_id, uint32_t n) {
    if (ctx_id < 0 || ctx_id >= kMaxIdxCtx) return hipErrorInvalidValue;
    if (g_allpairs_index_fail == ctx_id + 1) return hipErrorOutOfMemory;
    std::lock_guard<std::mutex> lk(g_idx_mu);
    IndexScratch& s = g_idx[ctx_id];
    const size_t need = index_bytes(n);
    if (s.cap >= need) return hipSuccess;
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess) return e;
    // (keep a quarter of what is free for everything else; the old buffer is given back first)
    if ((double)need > 0.75 * (double)(free_b + s.cap)) return hipErrorOutOfMemory;
    if (s.p) {
        (void)hipFree(s.p);  // (waits for the device -- an earlier pass may still read it; the launch lock is not held here)
        s.p = nullptr;
        s.cap = 0;
    }
    e = hipMalloc(&s.p, need);
    if (e != hipSuccess) {
        s.p = nullptr;
        (void)hipGetLastError();  // (the pass goes on without the index: leave no sticky error behind)
        return e;
    }
    s.cap = need;
    return hipSuccess;
}

static hipError_t device_cus(int* cus) {
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (hipError_t e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev)) return e;
    return *cus > 0 ? hipSuccess : hipErrorInvalidDevice;
}

// Block groups per tile of k_index_scatter: its grid is (tiles, G). A tile is 4096 hashes whatever n is, so a DB of 1 M
// hashes has 245 of them for 256 compute units that each hold two of these workgroups: with one workgroup per tile some
// compute units stand idle and the others have nobody to cover a workgroup's barrier waits. G = 2 below kTileWgsPerCu
// workgroups per compute unit, G = 1 from there on (256 compute units: 4.2 M hashes), where the tiles alone fill the chip
// several times over and the launch is what it was before the split. Measured (with the tiles dealt to the
// XCDs by xcd_consecutive): the scatter 43 -> 37 us at 1 M, 83 -> 78 at 2 M, 198 -> 180 at 4 M; G = 4 46 us at 1 M, which
// is why the rule never gives it ("index_tile_split" 4 still launches it). k_index_tile_count is not split: on (tiles, 2)
// it took 15.4 us for 13.3, on (tiles, 4) 22.4. From n and the compute units alone: every rank of a pass on like devices
// takes the same grid, and G never rises with n.
constexpr uint32_t kTileWgsPerCu = 4u;
uint32_t index_tile_split(uint32_t n, uint32_t cus) {
    const unsigned long long tiles = ((unsigned long long)n + kTile - 1u) / kTile, want = (unsigned long long)kTileWgsPerCu * cus;
    return tiles >= want ? 1u : 2u;
}

// The front of the build, up to the partition records: tile counts, the two scans, the high-byte pass. tcnt_raw (tests
// only, or nullptr) receives the tile counts as k_index_tile_count left them, before k_index_scan_rows turns them into bases.
static hipError_t launch_index_tiles(const uint4* db, uint32_t n, uint32_t* tcnt, uint32_t* tcnt_raw, uint32_t* ptotal, uint32_t* pbase,
                                     uint32_t* pfirst, uint32_t* chunk_p, uint2* rec, const uint32_t* d_select, hipStream_t s) {
    const uint32_t tiles = index_tiles(n), csz = index_chunk(n);
    uint32_t split = (uint32_t)g_index_tile_split;
    if (split == 0u) {
        int cus = 0;
        if (hipError_t e = device_cus(&cus)) return e;
        split = index_tile_split(n, (uint32_t)cus);
    }
    hipLaunchKernelGGL(k_index_tile_count, dim3(tiles), dim3(kTileThreads), 0, s, db, n, tiles, tcnt, d_select);
    if (tcnt_raw != nullptr) {
        if (hipError_t e = hipMemcpyAsync(tcnt_raw, tcnt, 4u * (size_t)kParts * tiles, hipMemcpyDeviceToDevice, s)) return e;
    }
    hipLaunchKernelGGL(k_index_scan_rows, dim3(kParts / 4u), dim3(256), 0, s, tcnt, tiles, ptotal, d_select);
    hipLaunchKernelGGL(k_index_scan_parts, dim3(1), dim3(1024), 0, s, ptotal, csz, pbase, pfirst, chunk_p, d_select);
    if (g_index_stage != 0) return launch_index_scatter(db, n, tiles, split, tcnt, pbase, rec, d_select, s);
    hipLaunchKernelGGL(k_index_partition, dim3(tiles), dim3(kTileThreads), 0, s, db, n, tiles, tcnt, pbase, rec, d_select);
    return hipGetLastError();
}

hipError_t index_tiles_debug(const void* d_db, uint32_t n, const uint32_t* d_select, uint32_t* d_tcnt_raw, uint32_t* d_tcnt, uint32_t* d_parts,
                             void* d_rec, hipStream_t s) {
    return launch_index_tiles((const uint4*)d_db, n, d_tcnt, d_tcnt_raw, d_parts, d_parts + kParts, d_parts + 2u * kParts,
                              d_parts + 3u * kParts + 4u, (uint2*)d_rec, d_select, s);
}

hipError_t launch_index_decide(const AllPairsArgs& a, uint32_t* d_select, const IndexRule& q, hipStream_t s) {
    const IndexPtrs p = index_ptrs(a.ctx_id, a.n);
    const uint32_t csz = index_chunk(a.n);
    if (hipError_t e = launch_index_tiles((const uint4*)a.d_db, a.n, p.tcnt, nullptr, p.ptotal, p.pbase, p.pfirst, p.chunk_p, p.rec, d_select, s))
        return e;
    if (hipError_t e = launch_index_order(p.rec, a.n, p.ptotal, p.pbase, p.cnt, p.off, p.hw, p.rows, d_select, s)) return e;
    hipLaunchKernelGGL(k_index_count, dim3(kMaxChunks), dim3(256), 0, s, p.rec, a.n, csz, p.ptotal, p.pbase, p.pfirst, p.chunk_p,
                       p.ccount, d_select);
    hipLaunchKernelGGL(k_index_offsets, dim3(kParts), dim3(256), 0, s, a.n, p.ptotal, p.pbase, p.pfirst, p.ccount, p.cnt, p.off, d_select);
    hipLaunchKernelGGL(k_index_stats, dim3(kStatsGrid), dim3(kStatsThreads), 0, s, p.cnt, d_select, q);
    return hipGetLastError();
}

// Workgroups of the join: 64 per compute unit (the compute units from the device's attributes), eight times what the device
// holds at once -- 8 workgroups of 4 waves per compute unit, 8 waves per SIMD --, and never more waves than there are runs.
// Measured on 1 M uniform hashes (profiles/r16_index_join_grid.txt): with exactly the resident number the
// waves of a SIMD do not advance alike -- the oldest is served first --, they end one after the other and the slots stand
// empty behind them (3.96 of 8 occupied, the join slower than one wave per item); with several workgroups per slot the
// hardware's dispatcher fills every slot that frees, and a wave still walks 16 items. The grid only sets how the runs are
// dealt out: any number of workgroups walks every item once ("index_join_wgs" n: exactly n). Up to 2^20 hashes that is the
// grid. Above, an item grows with n and a wave of the fixed grid lives for milliseconds (at 10 M: eight generations of ~6 ms
// waves, and the last one of each holds its slot while the others stand empty), so the grid grows with n -- the fixed number
// times n / 2^20, rounded up -- until every wave walks one run.
hipError_t index_join_workgroups(uint32_t n, uint32_t* wgs) {
    if (g_index_join_wgs > 0) {
        *wgs = (uint32_t)g_index_join_wgs;
        return hipSuccess;
    }
    int cus = 0;
    if (hipError_t e = device_cus(&cus)) return e;
    const unsigned long long scale = n > (1u << 20) ? ((unsigned long long)n + (1u << 20) - 1u) >> 20 : 1u;
    *wgs = (uint32_t)min((unsigned long long)cus * 64u * scale, (unsigned long long)(kRuns / 4u));
    return hipSuccess;
}

hipError_t launch_index_join(const AllPairsArgs& a, uint32_t* d_select, uint32_t r, hipStream_t s) {
    const IndexPtrs p = index_ptrs(a.ctx_id, a.n);
    hipLaunchKernelGGL(k_index_place, dim3(kMaxChunks), dim3(256), 0, s, p.rec, a.n, index_chunk(a.n), p.ptotal, p.pbase, p.pfirst,
                       p.chunk_p, p.ccount, p.hw, p.rows, d_select);
    JoinArgs j;
    j.off = p.off;
    j.hw = p.hw;
    j.rows = p.rows;
    j.db = (const uint4*)a.d_db;
    j.n = a.n;
    j.group = a.d_group;
    j.out = a.d_pairs;
    j.cap = a.cap;
    j.count = a.d_count;
    j.max_dist = a.max_dist;
    j.r = r;
    j.tw = a.max_dist / 8u;  // a pair within max_dist has a word within tw bits, and one of its two blocks within tw / 2 = r
    j.rank = a.rank;
    j.world = a.world;
    uint32_t wgs = 0;
    if (hipError_t e = index_join_workgroups(a.n, &wgs)) return e;
    hipLaunchKernelGGL(k_index_join, dim3(wgs), dim3(256), 0, s, j, (const uint32_t*)d_select);
    return hipGetLastError();
}

void index_release() {
    std::lock_guard<std::mutex> lk(g_idx_mu);
    for (IndexScratch& s : g_idx) {
        if (s.p) (void)hipFree(s.p);
        s = IndexScratch();
    }
}

}  // namespace hvd
