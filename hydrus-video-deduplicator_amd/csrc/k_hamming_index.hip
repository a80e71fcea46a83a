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
//   k_index_partition   the tiles again: rank from a returning LDS atomic, record {row, key} -> its partition (short runs)
//   k_index_count       one workgroup per chunk: low-byte digits counted in 256 LDS bins
//   k_index_offsets     one workgroup per partition: the chunks' counts -> per-key counts, off[b][h * 256 ..], chunk cursors
//   k_index_stats       a few hundred workgroups stride over the (block, key)s: exact candidates and the longest work item,
//                       reduced privately, two atomics and a ticket per workgroup; the last workgroup decides
//                       (select[kSelIdxUsed], hvd_kernels.h: index_wins) -- the matrix-core forms return at once when it is set
//   k_index_place       the chunks again: final position from a returning LDS atomic on the bin's cursor; rows, and the 16-byte
//                       half of the hash that does NOT hold block b (words 4..7 for b < 8, words 0..3 otherwise), gathered
//                       from the packed DB -> hc
//   k_index_join        one wave per work item (block b, key u): B_u x B_u (positions i < j) and B_u x B_{u ^ (1 << t)} for
//                       the one-bit neighbours above u. First stage on the indexed half: y in registers, x through scalar
//                       loads (the bucket is contiguous at a wave-uniform address), one survivor test per batch of x. Survivors
//                       fetch the other halves from the packed DB through rows; the full 256-bit distance, and a pair is
//                       emitted only by its CANONICAL block -- the first block whose keys are within r -- so it comes out
//                       exactly once, without a dedup pass
// Kernels up to the statistics return at once unless the probe's gate (select[kSelIdxGate]) is set, the last two unless the
// decision is. Nothing waits on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "hvd_kernels.h"

namespace {

constexpr uint32_t kBlocks = 16, kKeys = 65536;
constexpr uint32_t kWavePairs = 64;  // a wave's pair buffer in LDS (a step emits at most 64); full -> one atomic reserves room for all of it
constexpr uint32_t kXB = 4;          // x entries per scalar batch of the join: one survivor test per batch

__device__ __forceinline__ uint32_t key_of(const uint32_t w[8], uint32_t b) { return (w[b >> 1] >> (16u * (b & 1u))) & 0xFFFFu; }

__device__ __forceinline__ void load_words(const uint4* __restrict__ db, uint32_t i, uint32_t w[8]) {
    const uint4 h0 = db[(size_t)i * 2u], h1 = db[(size_t)i * 2u + 1u];
    w[0] = h0.x; w[1] = h0.y; w[2] = h0.z; w[3] = h0.w;
    w[4] = h1.x; w[5] = h1.y; w[6] = h1.z; w[7] = h1.w;
}

constexpr uint32_t kParts = kBlocks * 256u;       // partitions: (block, high byte of the key)
constexpr uint32_t kTile = 4096u;                   // hashes per tile: a tile's run in a partition is ~16 records = 128 B
constexpr uint32_t kTileThreads = 1024u;            // 16 waves per workgroup, kTile / kTileThreads hashes per thread
constexpr uint32_t kMinChunk = 4096u;               // a chunk: at most max(kMinChunk, 2 x the mean partition) entries ...
constexpr uint32_t kMaxChunks = kParts + 2048u;     // ... so a pass never has more chunks than this (index_chunk)

__device__ __forceinline__ uint32_t lds_add(uint32_t* p) {
    return __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(v, d);
        if (lane >= (uint32_t)d) v += y;
    }
    return v;
}

// tcnt[part][tile] = the tile's hashes whose key of block (part >> 8) has the high byte (part & 255)
__global__ __launch_bounds__(kTileThreads) void k_index_tile_count(const uint4* __restrict__ db, uint32_t n, uint32_t ntiles,
                                                                   uint32_t* __restrict__ tcnt, const uint32_t* __restrict__ select) {
    __shared__ uint32_t bins[kParts];
    if (select[hvd::kSelIdxGate] == 0u) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < kParts; k += kTileThreads) bins[k] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTile / kTileThreads; ++j) {
        const uint32_t i = blockIdx.x * kTile + j * kTileThreads + tid;
        if (i < n) {
            uint32_t w[8];
            load_words(db, i, w);
#pragma unroll
            for (uint32_t b = 0; b < kBlocks; ++b) (void)lds_add(&bins[b * 256u + (key_of(w, b) >> 8)]);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < kParts; k += kTileThreads) tcnt[(size_t)k * ntiles + blockIdx.x] = bins[k];
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

// rec[b][pbase + tile base + rank] = {row, key of block b}: the rank inside the tile's run comes from a returning LDS atomic.
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
                if (pos < n) rec[(size_t)b * n + pos] = make_uint2(i, key);
            }
        }
    }
}

// A chunk's place: partition, block, and its entries [lo, hi) of the partition's records.
struct Chunk {
    uint32_t p, b, lo, hi;
    size_t at;  // the partition's first record inside rec / its first position inside hc and rows (block included)
};
__device__ __forceinline__ bool chunk_of(uint32_t c, uint32_t n, uint32_t csz, const uint32_t* __restrict__ ptotal,
                                         const uint32_t* __restrict__ pbase, const uint32_t* __restrict__ pfirst,
                                         const uint32_t* __restrict__ chunk_p, Chunk* q) {
    if (c >= pfirst[kParts]) return false;
    q->p = chunk_p[c];
    q->b = q->p >> 8;
    q->lo = (c - pfirst[q->p]) * csz;
    q->hi = min(ptotal[q->p], q->lo + csz);
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
__global__ __launch_bounds__(256) void k_index_offsets(uint32_t n, const uint32_t* __restrict__ pbase, const uint32_t* __restrict__ pfirst,
                                                       uint32_t* __restrict__ ccount, uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ select) {
    __shared__ uint32_t wsum[4];
    if (select[hvd::kSelIdxGate] == 0u) return;
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

constexpr uint32_t kStatsGrid = 256u;  // workgroups of the statistics: each ends in two atomics and a ticket

// Candidates of key u in its block: C(c_u, 2) + (r = 1) c_u x c_v over the one-bit neighbours v = u ^ (1 << t) above u --
// the exact number of pairs whose keys of this block are within r, i.e. the pairs the join walks for this work item.
__global__ __launch_bounds__(256) void k_index_stats(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ select,
                                                     const hvd::IndexRule q) {
    if (select[hvd::kSelIdxGate] == 0u) return;
    // the workgroups stride over the kBlocks * kKeys (block, key)s (a multiple of the grid's threads) and reduce privately
    unsigned long long cand = 0;
    uint32_t mx = 0;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < kBlocks * kKeys; t += gridDim.x * 256u) {
        const uint32_t u = t & (kKeys - 1u);
        const uint32_t* cb = cnt + (t & ~(kKeys - 1u));
        const unsigned long long c = cb[u];
        unsigned long long ylen = c;
        cand += c * (c - (c != 0ull)) / 2ull;
        if (q.r != 0u && c != 0ull) {
#pragma unroll
            for (uint32_t s = 0; s < 16u; ++s)
                if (((u >> s) & 1u) == 0u) ylen += cb[u ^ (1u << s)];
            cand += c * (ylen - c);
        }
        // the work item's walk: its wave steps its c x's over a y list of ylen entries (saturated: any such item loses anyway)
        mx = max(mx, (uint32_t)min(c * ylen, 0xFFFFFFFFull));
    }
    for (int off = 32; off > 0; off >>= 1) {
        cand += __shfl_down(cand, off);
        mx = max(mx, (uint32_t)__shfl_down((int)mx, off));
    }
    __shared__ unsigned long long part[4];
    __shared__ uint32_t partm[4];
    if ((threadIdx.x & 63u) == 0u) {
        part[threadIdx.x >> 6] = cand;
        partm[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    const unsigned long long sum = part[0] + part[1] + part[2] + part[3];
    const uint32_t m = max(max(partm[0], partm[1]), max(partm[2], partm[3]));
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

// hc[b][pos] = the 16-byte half of the hash that does not hold block b (gathered from the packed DB: words 4..7 for b < 8,
// words 0..3 otherwise -- the half the join compares first), rows[b][pos] = row, in key order: pos from a returning
// LDS atomic on the bin's cursor (order inside a bucket: whatever the atomics give -- the join's rule does not depend on it).
// The chunks of a partition fill its region of hc and rows completely, and nobody else writes there.
__global__ __launch_bounds__(256) void k_index_place(const uint4* __restrict__ db, const uint2* __restrict__ rec, uint32_t n, uint32_t csz,
                                                     const uint32_t* __restrict__ ptotal, const uint32_t* __restrict__ pbase,
                                                     const uint32_t* __restrict__ pfirst, const uint32_t* __restrict__ chunk_p,
                                                     const uint32_t* __restrict__ ccount, uint4* __restrict__ hc, uint32_t* __restrict__ rows,
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
    const uint32_t sa = q.b < 8u ? 1u : 0u;
    constexpr uint32_t kU = 4u;  // entries per thread in flight: their gathers overlap
    for (uint32_t e0 = q.lo; e0 < q.hi; e0 += 256u * kU) {
        uint32_t row[kU], low[kU], pos[kU];
        uint4 h[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t e = e0 + u * 256u + tid;
            const uint2 rc = e < q.hi ? r[e] : make_uint2(n, 0u);
            row[u] = rc.x;  // (n: no entry)
            low[u] = rc.y & 255u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t g = min(row[u], n - 1u);
            h[u] = db[(size_t)g * 2u + sa];
        }
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) pos[u] = row[u] < n ? lds_add(&cur[low[u]]) : n;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u)
            if (pos[u] < n) {
                hc[base + pos[u]] = h[u];
                rows[base + pos[u]] = row[u];
            }
    }
}

__device__ __forceinline__ uint32_t popc4(const uint4& x, const uint4& y) {
    return __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
}

// The index as the join reads its x side: constant address space, so that a wave-uniform address is read by scalar loads
// (the index is read-only for the whole kernel) and the words reach the xor as scalar operands.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x4 kx4;

// acc + popcount(v) in one instruction (the compiler, left alone, counts three of the four words from zero and adds up after)
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t v, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(acc));
    return r;
}
__device__ __forceinline__ uint32_t popc4s(const u32x4 x, const uint4& y) {
    return bcnt_acc(x.w ^ y.w, bcnt_acc(x.z ^ y.z, bcnt_acc(x.y ^ y.y, __popc(x.x ^ y.x))));
}

struct JoinArgs {
    const uint32_t* off;
    const uint4* hc;
    const uint32_t* rows;
    const uint4* db;
    uint32_t n;
    const int32_t* group;
    hvd_pair* out;
    unsigned long long cap;
    unsigned long long* count;
    uint32_t max_dist, r, rank, world;
};

// A wave's buffered pairs -> global: one atomic reserves room for all of them; beyond `cap` nothing is written but the count
// still grows (the caller reports HVD_ERR_OVERFLOW with the number needed).
__device__ __forceinline__ void flush_wave(const JoinArgs& a, const hvd_pair* buf, uint32_t fill, uint32_t lane) {
    unsigned long long base = 0;
    if (lane == 0u) base = atomicAdd(a.count, (unsigned long long)fill);
    base = __shfl(base, 0);
    for (uint32_t k = lane; k < fill; k += 64u)
        if (base + k < a.cap) a.out[base + k] = buf[k];
}

// One batch of kXB x entries against the wave's 64 y: does any lane come within max_dist of any of them on the indexed half?
// All kXB entries are read at once, whatever the bucket holds: one past its end can only raise a false alarm, which the walk
// one by one (over the bucket's entries only) puts right. OWN: the round overlaps the item's own bucket, where x index k
// pairs with a y only if k < ylim (<= the bucket's size).
template <bool OWN>
__device__ __forceinline__ bool batch_hit(kx4* xp, const uint4& ya, uint32_t max_dist, uint32_t k0, uint32_t ylim) {
    u32x4 x[kXB];
#pragma unroll
    for (uint32_t j = 0; j < kXB; ++j) x[j] = xp[j];
    uint32_t d[kXB];
#pragma unroll
    for (uint32_t j = 0; j < kXB; ++j) d[j] = popc4s(x[j], ya);
    if (OWN) {
        bool c = false;
#pragma unroll
        for (uint32_t j = 0; j < kXB; ++j) c |= d[j] <= max_dist && k0 + j < ylim;
        return __any(c);
    }
    uint32_t m = d[0];
#pragma unroll
    for (uint32_t j = 1; j < kXB; ++j) m = min(m, d[j]);
    return __any(m <= max_dist);
}

// Work item = (block b, key u), one wave each; item (b << 16 | u) belongs to rank item mod world. The y list of an item is
// its own bucket (segment 0) followed by the buckets u ^ (1 << t) > u (r = 1): lanes take 64 consecutive entries of it per
// round and hold their y -- the 128 bits that do NOT hold block b, which is all the index stores -- in registers; the next
// round's y is loaded before the current round's x loop. The x side is the bucket itself, contiguous at a wave-uniform
// address: kXB entries per scalar batch, xor'ed as scalar operands, one survivor test per batch. A candidate's key agrees and
// its other bits are unrelated (~64 of 128 differ), so a batch with a lane within max_dist is rare: only then are its x
// looked at one by one, and the lanes that pass fetch the other 128 bits of both hashes from the packed DB through rows.
// Positions inside the own bucket are the first nu entries of the y list: only the rounds with p0 < nu pay for the i < j rule.
__global__ __launch_bounds__(256) void k_index_join(const JoinArgs a, const uint32_t* __restrict__ select) {
    __shared__ hvd_pair pbuf[4][kWavePairs];
    if (select[hvd::kSelIdxUsed] == 0u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t item = (blockIdx.x * 4u + wave) * a.world + a.rank;
    if (item >= kBlocks * kKeys) return;  // (wave-uniform; nothing below synchronises across waves)
    const uint32_t b = item >> 16, u = item & (kKeys - 1u);
    const uint32_t* __restrict__ offb = a.off + (size_t)b * (kKeys + 1u);
    // the bucket's and the 16 neighbours' offset pairs, all issued before the first of them is needed
    // segments: lane 0 the bucket itself, lane 1 + t the bucket u ^ (1 << t) if that key lies above u
    const bool nb = lane >= 1u && lane <= 16u && a.r != 0u && ((u >> ((lane - 1u) & 15u)) & 1u) == 0u;
    const uint32_t v = nb ? u ^ (1u << ((lane - 1u) & 15u)) : u;
    const uint32_t vstart = offb[v], vend = offb[v + 1u];
    const uint32_t s0 = offb[u], nu = offb[u + 1u] - s0;
    if (nu == 0u) return;
    const uint32_t sstart = lane == 0u || nb ? vstart : 0u;
    const uint32_t ssize = lane == 0u || nb ? vend - vstart : 0u;
    uint32_t incl = ssize;
    for (int d = 1; d < 32; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += y;
    }
    const int delta = (int)sstart - (int)(incl - ssize);  // position = p + delta for an entry p of this segment
    uint32_t ends[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) ends[s] = (uint32_t)__builtin_amdgcn_readlane((int)incl, s);
    const uint32_t ny = (uint32_t)__builtin_amdgcn_readlane((int)incl, 16);
    const size_t base = (size_t)b * a.n;
    const uint4* __restrict__ hb = a.hc + base;
    // (a batch reads kXB entries whatever the bucket holds: at most kXB - 1 entries past the block's last position, and behind
    // the last block's hc lie the rows, 64 B per hash, in the same allocation)
    kx4* xb = (kx4*)(a.hc + base + s0);
    const uint32_t sa = b < 8u ? 1u : 0u;  // the 16-B half that does not hold block b: the one in hc
    uint32_t fill = 0;                    // wave-uniform
    hvd_pair* buf = pbuf[wave];

    // x entry k of the bucket against the wave's y, one by one: the batch had a lane within max_dist
    auto examine = [&](uint32_t k, const uint4& ya, uint32_t ypos, uint32_t ylim) {
        const u32x4 xv = xb[k];
        const uint4 xa = make_uint4(xv.x, xv.y, xv.z, xv.w);
        const uint32_t d0 = popc4(xa, ya);
        const bool c = d0 <= a.max_dist && k < ylim;
        if (!__any(c)) return;
        bool emit = false;
        uint32_t d = 0, i = 0, j = 0;
        if (c) {
            const uint32_t ri = a.rows[base + s0 + k], rj = a.rows[base + ypos];
            const uint4 xo = a.db[(size_t)ri * 2u + (sa ^ 1u)], yo = a.db[(size_t)rj * 2u + (sa ^ 1u)];
            d = d0 + popc4(xo, yo);
            emit = d <= a.max_dist;
            if (emit) {
                const uint4 lo_x = sa ? xo : xa, hi_x = sa ? xa : xo, lo_y = sa ? yo : ya, hi_y = sa ? ya : yo;
                const uint32_t dw[8] = {lo_x.x ^ lo_y.x, lo_x.y ^ lo_y.y, lo_x.z ^ lo_y.z, lo_x.w ^ lo_y.w,
                                        hi_x.x ^ hi_y.x, hi_x.y ^ hi_y.y, hi_x.z ^ hi_y.z, hi_x.w ^ hi_y.w};
                uint32_t within = 0;  // bit b2: the keys of block b2 are within r
#pragma unroll
                for (uint32_t b2 = 0; b2 < kBlocks; ++b2) within |= (uint32_t)__popc(key_of(dw, b2)) <= a.r ? 1u << b2 : 0u;
                if ((within & ((1u << b) - 1u)) != 0u) emit = false;  // an earlier block within r owns this pair
            }
            if (emit && a.group != nullptr && a.group[ri] == a.group[rj]) emit = false;
            i = min(ri, rj);
            j = max(ri, rj);
        }
        const unsigned long long em = __ballot(emit);
        const uint32_t m = (uint32_t)__popcll(em);
        if (m == 0u) return;
        if (fill + m > kWavePairs) {
            flush_wave(a, buf, fill, lane);
            fill = 0;
        }
        if (emit) {
            const uint32_t slot = fill + __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
            hvd_pair rec;
            rec.i = i;
            rec.j = j;
            rec.dist = d;
            rec.pad = 0;
            buf[slot] = rec;
        }
        fill += m;
    };
    // the whole bucket against one round's y
    auto walk = [&](auto own, const uint4& ya, uint32_t ypos, uint32_t ylim) {
        constexpr bool kOwn = decltype(own)::value;
        for (uint32_t k0 = 0; k0 < nu; k0 += kXB) {
            const uint32_t nvalid = min(kXB, nu - k0);
            const bool hit = batch_hit<kOwn>(xb + k0, ya, a.max_dist, k0, ylim);
            if (__builtin_expect(hit, 0))
                for (uint32_t j = 0; j < nvalid; ++j) examine(k0 + j, ya, ypos, ylim);
        }
    };
    // entry p of the y list: its segment and its position inside block b
    auto locate = [&](uint32_t p, uint32_t* seg) {
        uint32_t sg = 0;
#pragma unroll
        for (int s = 0; s < 16; ++s) sg += p >= ends[s] ? 1u : 0u;
        *seg = sg;
        return (uint32_t)((int)p + __shfl(delta, (int)sg));
    };
    uint32_t seg, ypos = locate(lane, &seg);
    uint4 ya = make_uint4(0u, 0u, 0u, 0u);
    if (lane < ny) ya = hb[ypos];
    for (uint32_t p0 = 0; p0 < ny; p0 += 64u) {
        const uint32_t p = p0 + lane;
        uint32_t seg_n;
        const uint32_t ypos_n = locate(p + 64u, &seg_n);
        asm volatile("" ::"v"(ya.x), "v"(ya.y), "v"(ya.z), "v"(ya.w));  // (this round's y has arrived before the next one's load is issued)
        uint4 ya_n = make_uint4(0u, 0u, 0u, 0u);
        if (p + 64u < ny) ya_n = hb[ypos_n];  // the next round's y: in flight under this round's x loop
        // x index k pairs with this y iff k < ylim: inside the bucket only the x before it (positions i < j)
        const uint32_t ylim = p >= ny ? 0u : seg == 0u ? p : nu;
        if (p0 < nu)
            walk(std::true_type(), ya, ypos, ylim);
        else
            walk(std::false_type(), ya, ypos, ylim);
        seg = seg_n;
        ypos = ypos_n;
        ya = ya_n;
    }
    if (fill != 0u) flush_wave(a, buf, fill, lane);
}

}  // namespace

namespace hvd {

int g_allpairs_index = -1;
int g_allpairs_index_fail = 0;

// per-context scratch: per-key counts [16][65536], offsets [16][65537], half-hash copies [16][n] x 16 B, rows [16][n]; for the
// build: partition records [16][n] x 8 B, tile counts [4096][tiles], and per partition / chunk: sizes, bases, first chunks,
// the chunk list and the chunks' low-byte counts (cursors)
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
    return 4u * (size_t)kBlocks * kKeys + 4u * off_words() + (size_t)kBlocks * n * 16u + (size_t)kBlocks * n * 4u +
           (size_t)kBlocks * n * 8u + 4u * tcnt_words(n) + 4u * kPartWords + 4u * (size_t)kMaxChunks * 256u;
}
struct IndexPtrs {
    uint32_t* cnt;
    uint32_t* off;
    uint4* hc;
    uint32_t* rows;
    uint2* rec;
    uint32_t *tcnt, *ptotal, *pbase, *pfirst, *chunk_p, *ccount;
};
static IndexPtrs index_ptrs(int ctx_id, uint32_t n) {
    char* p = (char*)g_idx[ctx_id].p;
    IndexPtrs q;
    q.cnt = (uint32_t*)p;
    q.off = (uint32_t*)(p + 4u * (size_t)kBlocks * kKeys);
    q.hc = (uint4*)(p + 4u * (size_t)kBlocks * kKeys + 4u * off_words());
    q.rows = (uint32_t*)((char*)q.hc + (size_t)kBlocks * n * 16u);
    q.rec = (uint2*)(q.rows + (size_t)kBlocks * n);  // (16 n words behind a 16-byte boundary: aligned)
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
    // (DESIGN 4.1, 1 M uniform hashes on MI355X: form 9 18.1 ms = 36 fs per comparison, forms 18 / 12 +4 / +11 %; join 2.0 ms
    // for 2.075e9 candidates; the counting sort, the statistics and the place pass 0.93 ms, of which ~0.03 ms do not depend
    // on n (the scans over 4096 partitions, the grid of 6144 chunks): 0.9 ns per hash, and those 30 us next to the 40 us of
    // launches; the longest work item's wave takes ~30 ns per step of 64 pairs. These are the figures of the full-width
    // index with the LDS-staged join: the half-width index and the scalar-x join have not been profiled yet, so ps_cand and
    // ps_hash are the old, costlier ones -- the rule can only be too cautious about the index until they are re-derived)
    q.fs_mfma_fetch = 36.0f;
    q.fs_mfma_other = 40.0f;
    q.ps_cand = 1.0f;
    q.ps_hash = 900.0f;
    q.ps_crit = 500.0f;
    q.fixed_ns = 70000.0f;
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

hipError_t launch_index_decide(const AllPairsArgs& a, uint32_t* d_select, const IndexRule& q, hipStream_t s) {
    const IndexPtrs p = index_ptrs(a.ctx_id, a.n);
    const uint32_t tiles = index_tiles(a.n), csz = index_chunk(a.n);
    const uint4* db = (const uint4*)a.d_db;
    hipLaunchKernelGGL(k_index_tile_count, dim3(tiles), dim3(kTileThreads), 0, s, db, a.n, tiles, p.tcnt, d_select);
    hipLaunchKernelGGL(k_index_scan_rows, dim3(kParts / 4u), dim3(256), 0, s, p.tcnt, tiles, p.ptotal, d_select);
    hipLaunchKernelGGL(k_index_scan_parts, dim3(1), dim3(1024), 0, s, p.ptotal, csz, p.pbase, p.pfirst, p.chunk_p, d_select);
    hipLaunchKernelGGL(k_index_partition, dim3(tiles), dim3(kTileThreads), 0, s, db, a.n, tiles, p.tcnt, p.pbase, p.rec, d_select);
    hipLaunchKernelGGL(k_index_count, dim3(kMaxChunks), dim3(256), 0, s, p.rec, a.n, csz, p.ptotal, p.pbase, p.pfirst, p.chunk_p,
                       p.ccount, d_select);
    hipLaunchKernelGGL(k_index_offsets, dim3(kParts), dim3(256), 0, s, a.n, p.pbase, p.pfirst, p.ccount, p.cnt, p.off, d_select);
    hipLaunchKernelGGL(k_index_stats, dim3(kStatsGrid), dim3(256), 0, s, p.cnt, d_select, q);
    return hipGetLastError();
}

hipError_t launch_index_join(const AllPairsArgs& a, uint32_t* d_select, uint32_t r, hipStream_t s) {
    const IndexPtrs p = index_ptrs(a.ctx_id, a.n);
    hipLaunchKernelGGL(k_index_place, dim3(kMaxChunks), dim3(256), 0, s, (const uint4*)a.d_db, p.rec, a.n, index_chunk(a.n), p.ptotal,
                       p.pbase, p.pfirst, p.chunk_p, p.ccount, p.hc, p.rows, d_select);
    JoinArgs j;
    j.off = p.off;
    j.hc = p.hc;
    j.rows = p.rows;
    j.db = (const uint4*)a.d_db;
    j.n = a.n;
    j.group = a.d_group;
    j.out = a.d_pairs;
    j.cap = a.cap;
    j.count = a.d_count;
    j.max_dist = a.max_dist;
    j.r = r;
    j.rank = a.rank;
    j.world = a.world;
    const uint32_t items = (kBlocks * kKeys + a.world - 1u - a.rank) / a.world;  // this rank's items: rank, rank + world, ...
    hipLaunchKernelGGL(k_index_join, dim3((items + 3u) / 4u), dim3(256), 0, s, j, (const uint32_t*)d_select);
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
