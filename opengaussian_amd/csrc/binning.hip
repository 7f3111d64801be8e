// Tile lists of the rasterizer for gfx950: tile-range detection, the counting sort by tile, the per-tile depth sort and the
// key export.  Integer work, no float math.  The general uint32 scan and radix sort the rasterizer
// shares with the rest of the library are in radix_sort.hip.
//
// Sort strategy (DESIGN.md "binning"): the reference sorts D=(Gaussian,tile) duplicates on a 64-bit
// key (tile<<32 | depth bits) -- 6 byte-digit passes over D.  Here duplicates are emitted in Gaussian-index
// order, grouped by tile id alone, and one launch then sorts each tile's short list by (depth, Gaussian index) in LDS
// (tile_depth_sort_kernel): bit-identical order -- depth ascending inside a tile, ties by Gaussian index, whatever
// order the list arrived in.  The grouping is ONE counting pass on the whole tile id for the default streaming pass
// (tile_count_kernel .. tile_place_kernel: the keys are read twice, only the values move, once), and a stable
// radix sort (ceil(log2 T / 8) = 2 passes over D at 1080p) for full_binning, grids past the LDS histogram and lists
// too short for the count table.
// Grouped passes (up to 2^31 virtual tiles of a few entries) and the small path instead sort the P
// Gaussians by depth once and emit the duplicates in that order.
#include <stddef.h>

#include <atomic>

#include "block_scan.h"
#include "ogs_common.h"

namespace ogs {

namespace {

constexpr int kRangeItems = 4;               // consecutive keys per thread: one 16-byte load + the key in front of them
__global__ __launch_bounds__(kBlock) void tile_ranges_kernel(const uint32_t* __restrict__ tile_keys, int64_t D_cap,
                                                             const uint32_t* __restrict__ n_dev,
                                                             uint2* __restrict__ ranges) {
    const int64_t D = n_dev ? min((int64_t)*n_dev, D_cap) : D_cap;
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRangeItems;
    if (i0 >= D) return;
    uint32_t k[kRangeItems];
    if (i0 + kRangeItems <= D) {
        const uint4 v = *reinterpret_cast<const uint4*>(tile_keys + i0);      // the key buffers are 256-byte aligned
        k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < kRangeItems; ++j) k[j] = i0 + j < D ? tile_keys[i0 + j] : 0u;
    }
    uint32_t prev = i0 > 0 ? tile_keys[i0 - 1] : 0u;
#pragma unroll
    for (int j = 0; j < kRangeItems; ++j) {
        const int64_t i = i0 + j;
        if (i < D) {
            const uint32_t cur = k[j];
            if (i == 0) {
                ranges[cur].x = 0;
            } else if (prev != cur) {
                ranges[prev].y = (uint32_t)i;
                ranges[cur].x = (uint32_t)i;
            }
            if (i == D - 1) ranges[cur].y = (uint32_t)D;
            prev = cur;
        }
    }
}

// ---- counting sort by tile ("tile count" path) ----------------------------------------------------------------------------
// The default streaming pass (capi.hip::render_impl) needs no stable tile sort: tile_depth_sort_kernel orders ties by id itself,
// so the pairs only have to reach their tile's segment, in any order.  That is one counting pass on the whole tile id:
//   tile_count_kernel        the emitted keys [0, n) are cut into B contiguous chunks; workgroup b counts its chunk's keys per
//                            tile in an LDS histogram of `tiles` words and writes row b of the (B + 1) x tiles table (coalesced);
//   tile_count_scan_kernel   per tile: every cnt[b][t] -> its exclusive prefix over b, the column's total -> row B;
//   tile_place_kernel        workgroup (p, s), G consecutive chunks x a slice of the tiles: exclusive scan of the totals in LDS
//                            (the tiles' range starts: 32 KB from L2 and a thousand-thread scan cost less than a launch of its
//                            own), cursors from its table rows; it re-reads its chunks, position of a kept pair of its slice =
//                            LDS atomicAdd on its tile's cursor.  Staged (long lists): the position is a slot of an LDS buffer,
//                            written out afterwards with consecutive lanes on consecutive list slots; otherwise one 4-byte
//                            store of the value per pair.  No key is written.  The workgroups p = 0 also write ranges[t] =
//                            (start, end), (0, 0) for an empty tile (what tile_ranges_kernel leaves), one the total to `kept`.
// No global atomic, no look-back, no waiting between workgroups.  A dropped pair (kDropKey) fails the one `key < tiles` test, as
// would a key outside the grid, so no LDS word outside the histogram is ever addressed.
// chunk length = ceil(n / B) rounded up to the trip (kCountTrip keys: one 16-byte load per thread), from the device's n.
constexpr int kCountBlock = 1024;              // threads: the per-workgroup work on the `tiles` words (clear, row, scan) is 4x shorter
constexpr int kCountItems = 4;
constexpr int kCountTrip = kCountBlock * kCountItems;
constexpr int kCountScanCols = 64, kCountScanGroups = 16;         // column scan: 64 tiles x 16 groups of rows per workgroup
constexpr int kPlaceUnroll = 2;                // trips whose loads tile_place_kernel issues before its first LDS atomic
constexpr int kPlaceEntryBytes = 6;            // a staged entry: the value and its 16-bit tile index inside the slice

// [begin, end) of `group` consecutive chunks from chunk p * group on, out of nchunks (the last of them may be short or empty)
__device__ __forceinline__ void tile_chunk_span(const uint32_t* __restrict__ n_dev, int64_t n_cap, int nchunks, int p, int group,
                                                int64_t& begin, int64_t& end) {
    const int64_t n = n_dev ? min((int64_t)*n_dev, n_cap) : n_cap;
    const int64_t per = (n + nchunks - 1) / nchunks;
    const int64_t chunk = (per + kCountTrip - 1) / kCountTrip * kCountTrip;
    begin = min(n, (int64_t)p * group * chunk);
    end = min(n, begin + (int64_t)group * chunk);
}

__device__ __forceinline__ void tile_count_chunk(const uint32_t* __restrict__ n_dev, int64_t n_cap, int nchunks, int64_t& begin,
                                                 int64_t& end) {
    tile_chunk_span(n_dev, n_cap, nchunks, (int)blockIdx.x, 1, begin, end);
}

__global__ __launch_bounds__(kCountBlock) void tile_count_kernel(const uint32_t* __restrict__ keys, int64_t n_cap,
                                                                 const uint32_t* __restrict__ n_dev, int tiles,
                                                                 uint32_t* __restrict__ table /*[gridDim.x + 1][tiles]*/) {
    extern __shared__ uint32_t count_lds[];                       // [tiles]
    int64_t begin, end;
    tile_count_chunk(n_dev, n_cap, (int)gridDim.x, begin, end);
    for (int t = threadIdx.x; t < tiles; t += kCountBlock) count_lds[t] = 0u;
    __syncthreads();
    for (int64_t i0 = begin + (int64_t)threadIdx.x * kCountItems; i0 < end; i0 += kCountTrip) {
        uint32_t k[kCountItems];
        if (i0 + kCountItems <= end) {                            // begin is a multiple of the trip: 16-byte aligned
            const uint4 v = *reinterpret_cast<const uint4*>(keys + i0);
            k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < kCountItems; ++j) k[j] = i0 + j < end ? keys[i0 + j] : kDropKey;
        }
#pragma unroll
        for (int j = 0; j < kCountItems; ++j)
            if (k[j] < (uint32_t)tiles) atomicAdd(&count_lds[k[j]], 1u);
    }
    __syncthreads();
    uint32_t* row = table + (size_t)blockIdx.x * tiles;
    for (int t = threadIdx.x; t < tiles; t += kCountBlock) row[t] = count_lds[t];
}

// Thread (g, c) owns tile blockIdx.x * 64 + c and the rows [g R, (g + 1) R), R = ceil(B / 16): it sums them, the 16 sums of a
// column are scanned through LDS, and a second walk over the same rows (L2-resident) leaves the exclusive prefixes.  A wave
// reads 64 consecutive words of a row per step.  Row `nrows` of the table receives the totals.
__global__ __launch_bounds__(kCountScanCols * kCountScanGroups) void tile_count_scan_kernel(uint32_t* __restrict__ table, int nrows,
                                                                                            int tiles) {
    __shared__ uint32_t part[kCountScanGroups][kCountScanCols];
    const int c = threadIdx.x & (kCountScanCols - 1), g = threadIdx.x / kCountScanCols;
    const int t = blockIdx.x * kCountScanCols + c;
    const int per = (nrows + kCountScanGroups - 1) / kCountScanGroups;
    const int r0 = min(nrows, g * per), r1 = min(nrows, r0 + per);
    uint32_t sum = 0;
    if (t < tiles) {
#pragma unroll 8
        for (int r = r0; r < r1; ++r) sum += table[(size_t)r * tiles + t];
    }
    part[g][c] = sum;
    __syncthreads();
    uint32_t run = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kCountScanGroups; ++j) {
        const uint32_t v = part[j][c];
        if (j < g) run += v;
        total += v;
    }
    if (t >= tiles) return;
    if (g == 0) table[(size_t)nrows * tiles + t] = total;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) {
        uint32_t* p = table + (size_t)r * tiles + t;
        const uint32_t v = *p;
        *p = run;
        run += v;
    }
}

// The walk of tile_place_kernel over its keys [begin, end): a pair whose key lies in the slice [ulo, ulo + unt) takes the next
// slot of its tile's LDS cursor -- kStaged: a slot of the staging buffer, where the value and the tile's index inside the slice
// go; otherwise the global slot, where the value goes.  The values are loaded beside the keys, 16 bytes per thread, whatever the
// slice keeps of them: a load that waits for the key test cost 3-5 us at S = 2 and 4.
template <bool kStaged>
__device__ __forceinline__ void tile_place_walk(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t begin,
                                                int64_t end, bool reverse, uint32_t ulo, uint32_t unt, uint32_t* cur,
                                                uint32_t* stage, uint16_t* stile, uint32_t stage_words, uint32_t* __restrict__ out,
                                                uint32_t out_cap) {
    const int64_t len = end - begin;
    for (int64_t i0 = (int64_t)threadIdx.x * kCountItems; i0 < len; i0 += (int64_t)kPlaceUnroll * kCountTrip) {
        uint32_t k[kPlaceUnroll][kCountItems], v[kPlaceUnroll][kCountItems];
#pragma unroll
        for (int u = 0; u < kPlaceUnroll; ++u) {
            const int64_t iu = i0 + (int64_t)u * kCountTrip;
            if (!reverse && begin + iu + kCountItems <= end) {        // begin is a multiple of the trip: 16-byte aligned
                const uint4 kk = *reinterpret_cast<const uint4*>(keys + begin + iu);
                const uint4 vv = *reinterpret_cast<const uint4*>(vals + begin + iu);
                k[u][0] = kk.x - ulo; k[u][1] = kk.y - ulo; k[u][2] = kk.z - ulo; k[u][3] = kk.w - ulo;
                v[u][0] = vv.x; v[u][1] = vv.y; v[u][2] = vv.z; v[u][3] = vv.w;
            } else {
#pragma unroll
                for (int j = 0; j < kCountItems; ++j) {
                    const int64_t i = reverse ? end - 1 - (iu + j) : begin + iu + j;
                    const bool in = iu + j < len;
                    k[u][j] = in ? keys[i] - ulo : kDropKey;
                    v[u][j] = in ? vals[i] : 0u;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kPlaceUnroll; ++u) {
#pragma unroll
            for (int j = 0; j < kCountItems; ++j) {
                if (k[u][j] < unt) {
                    const uint32_t pos = atomicAdd(&cur[k[u][j]], 1u);
                    if (kStaged) {
                        if (pos < stage_words) {
                            stage[pos] = v[u][j];
                            stile[pos] = (uint16_t)k[u][j];
                        }
                    } else if (pos < out_cap) {
                        out[pos] = v[u][j];
                    }
                }
            }
        }
    }
}

// Workgroup (p, s) = (blockIdx.x, blockIdx.y) places the pairs of place chunk p -- the count chunks [p G, min((p + 1) G, B)), one
// contiguous stretch of the keys -- that fall into tile slice s: the ceil(tiles / S) tiles from s ceil(tiles / S) on (the last
// slices may be short or empty).  The table's rows are exclusive prefixes over b with the totals in row B, so the workgroup's
// first slot of tile t is start[t] + table[p G][t] and its pair count table[min((p + 1) G, B)][t] - table[p G][t]; start[t] is
// the sum of the totals in front of the slice plus a scan inside it.
//   staged   (stage_words > 0 and the workgroup's pair count, known before a key is read, fits): the LDS cursor of a tile starts
//            at the tile's run start inside the staging buffer; the value and the tile's 16-bit index j inside the slice go to
//            entry atomicAdd(&cur[j], 1).  After the walk thread i takes staged entry i and stores its value at delta[j] + i
//            (delta = first global slot - run start): consecutive lanes write consecutive list slots.  (Finding j by bisection
//            over the run ends instead of keeping it cost 3-5 us: DESIGN 3i.)
//   direct   (otherwise): the cursor is the global slot, the value is stored from the walk, one 4-byte store per pair.
// LDS: cur[ceil(tiles / S)], and with stage_words > 0 also delta[ceil(tiles / S)], stage[stage_words] and the 16-bit
// stile[stage_words].
// The workgroups p = 0 write ranges[t] of their slice ((0, 0) for an empty tile), workgroup (0, S - 1) -- whose slice, empty or
// not, ends at the last tile -- writes the grand total to `kept`; neither duty depends on the chunk holding a key.
// reverse (tests only): the chunk is walked back to front, so that equal-depth pairs reach their tile in descending id order.
// out_cap: size of `out`; a position is below the kept total <= n <= out_cap by construction, the test only keeps a table that
// something else damaged from turning into a stray store (as does `pos < stage_words` for the staging buffer).
__global__ __launch_bounds__(kCountBlock) void tile_place_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                 int64_t n_cap, const uint32_t* __restrict__ n_dev, int tiles,
                                                                 int nrows, int group, uint32_t stage_words,
                                                                 const uint32_t* __restrict__ table, uint2* __restrict__ ranges,
                                                                 uint32_t* __restrict__ kept, uint32_t* __restrict__ out,
                                                                 uint32_t out_cap, bool reverse) {
    extern __shared__ uint32_t count_lds[];
    __shared__ uint32_t wave_sums[3][kCountBlock / kWave];
    const int p = blockIdx.x, slices = gridDim.y;
    const int per_slice = (tiles + slices - 1) / slices;
    const int t_lo = min(tiles, (int)blockIdx.y * per_slice), nt = min(tiles, t_lo + per_slice) - t_lo;
    int64_t begin, end;
    tile_chunk_span(n_dev, n_cap, nrows, p, group, begin, end);
    if (begin >= end && p != 0) return;                           // block-uniform; the workgroups p = 0 write the ranges whatever n is
    const bool may_stage = stage_words > 0;
    uint32_t* cur = count_lds;                                    // totals -> run starts / global slots -> cursors
    uint32_t* delta = cur + per_slice;                            // pair counts -> first global slot - run start
    uint32_t* stage = delta + per_slice;
    const uint32_t* totals = table + (size_t)nrows * tiles;
    const uint32_t* row = table + (size_t)p * group * tiles + t_lo;
    const uint32_t* row_end = table + (size_t)min(nrows, (p + 1) * group) * tiles + t_lo;
    uint32_t front = 0;                                           // this thread's share of the totals in front of the slice
    for (int t = threadIdx.x; t < t_lo; t += kCountBlock) front += totals[t];
    for (int j = threadIdx.x; j < nt; j += kCountBlock) {
        cur[j] = totals[t_lo + j];
        if (may_stage) delta[j] = row_end[j] - row[j];
    }
    __syncthreads();
    // a thread scans `per` consecutive tiles; per is odd, so the lanes of a wave walk different LDS banks
    const int per = ((nt + kCountBlock - 1) / kCountBlock) | 1;
    const int j0 = min(nt, (int)threadIdx.x * per), j1 = min(nt, j0 + per);
    uint32_t sum = 0, mine = 0;
    for (int j = j0; j < j1; ++j) {
        sum += cur[j];
        if (may_stage) mine += delta[j];
    }
    const uint32_t inc = wave_inclusive_scan(sum), inc_mine = wave_inclusive_scan(mine), inc_front = wave_inclusive_scan(front);
    if (lane_id() == kWave - 1) {
        wave_sums[0][threadIdx.x >> 6] = inc;
        wave_sums[1][threadIdx.x >> 6] = inc_mine;
        wave_sums[2][threadIdx.x >> 6] = inc_front;
    }
    __syncthreads();
    uint32_t run = inc - sum, run_mine = inc_mine - mine, total = 0, need = 0;
#pragma unroll
    for (int w = 0; w < kCountBlock / kWave; ++w) {
        const uint32_t a = wave_sums[0][w], b = wave_sums[1][w];
        if (w < (int)(threadIdx.x >> 6)) { run += a; run_mine += b; }
        total += a + wave_sums[2][w];
        run += wave_sums[2][w];
        need += b;
    }
    const bool staged = may_stage && need <= stage_words;         // block-uniform: every pair of the workgroup has a staging slot
    for (int j = j0; j < j1; ++j) {
        const uint32_t cnt = cur[j], c = may_stage ? delta[j] : 0u;
        if (p == 0) ranges[t_lo + j] = cnt ? make_uint2(run, run + cnt) : make_uint2(0u, 0u);
        if (staged) {
            cur[j] = run_mine;
            delta[j] = run - run_mine;
        } else {
            cur[j] = run;
        }
        run += cnt;
        run_mine += c;
    }
    if (p == 0 && blockIdx.y == gridDim.y - 1 && threadIdx.x == 0) *kept = total;
    if (begin >= end || nt == 0 || (may_stage && need == 0)) return;   // block-uniform: nothing of this chunk lies in this slice
    __syncthreads();
    for (int j = threadIdx.x; j < nt; j += kCountBlock) (staged ? delta : cur)[j] += row[j];
    __syncthreads();
    const uint32_t ulo = (uint32_t)t_lo, unt = (uint32_t)nt;      // key - ulo < unt: inside the slice (a dropped pair never is)
    uint16_t* stile = reinterpret_cast<uint16_t*>(stage + stage_words);
    if (!staged) {
        tile_place_walk<false>(keys, vals, begin, end, reverse, ulo, unt, cur, stage, stile, stage_words, out, out_cap);
        return;
    }
    tile_place_walk<true>(keys, vals, begin, end, reverse, ulo, unt, cur, stage, stile, stage_words, out, out_cap);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < need; i += kCountBlock) {   // consecutive lanes, consecutive slots of a run
        const uint32_t pos = delta[min((int)stile[i], nt - 1)] + i;
        if (pos < out_cap) out[pos] = stage[i];
    }
}

// ---- per-tile depth order ----------------------------------------------------------------------------------------------
// A tile's segment of the point list holds its Gaussians in id order after the stable radix tile sort (duplicate_kernel emits
// the pairs in Gaussian-index order), in no particular order after the counting sort by tile.  Either way the segment is permuted
// in place into (depth key, Gaussian id) order: stable LSD passes on the 32-bit key, then a look at the ties ("Ties", below),
// which re-sorts the few lists whose equal keys did not come out in id order.  The keys are gathered from the compact per-Gaussian key array preprocess wrote
// (4 B per Gaussian), by the id in the value; the reach flag (bit 31) travels with the value.  Only the bits that differ inside
// the tile are sorted on: [lowest, highest differing bit] in ceil(span / 8) passes of <= 8 bits.
// A workgroup takes four tiles (tile_order[4b .. 4b+3]):
//   * lists up to kWaveSortCap entries: one wave each, no workgroup barrier -- the common case (S1M: ~440 entries).  These need no
//     stable pass at all, (key, id) being a total order: one bucket pass and a ranking inside each bucket (wave_bucket_rank), the
//     LSD passes below only for a list whose largest bucket is long (clustered depths, many equal keys);
//   * then, one after the other, its lists up to kTileSortCap entries: all four waves, in LDS;
//   * longer lists: the same four-wave ranking on chunks of kTileSortCap entries, passes ping-pong between the segment and
//     the same positions of `scratch` (a D-sized buffer the tile sort left free), a histogram pass over the list per digit.
// Ranking inside a wave: every lane ORs its lane bit into the 64-bit match mask of its digit (LDS), reads the mask back -- the
// lanes with the same digit -- and the lowest of them adds their count to the wave's running digit count.  One LDS round trip
// per item whatever the digit width (a ballot per digit bit cost ~40 VALU per item).  Entry e of a wave's share is item e / 64,
// lane e % 64; with several waves the share of wave w is [w * chunk, (w + 1) * chunk), chunk = 64 * ceil(m / 256), so
// (wave, item, lane) order is memory order, which is what stability needs.
constexpr int kTileSortWaves = kBlock / kWave;
struct TileSortLds {
    uint32_t hist[kTileSortWaves][256];     // per wave: running digit counts, then digit starts / wave offsets
    uint32_t dig_start[256];                // four-wave ranking: workgroup-local start of every digit
    uint32_t base[256];                     // long lists: output position of the next entry of each digit
    uint32_t scan_sums[4];
    uint32_t red[2];                        // AND / OR of a four-wave tile's keys
    uint2 range[kTileSortWaves];            // the workgroup's four tiles
    uint32_t kv[2 * kTileSortCap];          // keys, values; while a pass ranks, the 256 match masks of wave w (2 KB) alias the
                                            // start of quarter w
};
// explicit LDS pointers: volatile / atomic accesses through generic ones stay generic (flat), and one such form ended in an
// invalid instruction
typedef __attribute__((address_space(3))) volatile uint32_t LdsWord;
typedef __attribute__((address_space(3))) unsigned long long LdsMask;
static_assert(offsetof(TileSortLds, kv) % 8 == 0, "a wave's quarter of kv is read as 64-bit pairs");
__device__ __forceinline__ LdsWord* lds_words(uint32_t* p) { return (LdsWord*)p; }
__device__ __forceinline__ LdsMask* wave_masks(TileSortLds& sm, int wave) { return (LdsMask*)(sm.kv + wave * 2 * kWaveSortCap); }

// zero a wave's 256 digit counts and 256 match masks (wave-local)
__device__ __forceinline__ void wave_rank_clear(LdsWord* hist, LdsMask* masks) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hist[lane + j * kWave] = 0u;
        __hip_atomic_store(&masks[lane + j * kWave], 0ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    __builtin_amdgcn_wave_barrier();
}

// Stable ranking of a wave's items on digit (key >> shift) & mask: rank[i] = the wave's earlier entries with the same digit
// (+ the count it had before), hist[d] += the wave's entries of digit d.  Item i, lane l is entry first + 64 i + l, valid below m.
// The masks start zeroed and are left zeroed.
__device__ __forceinline__ void wave_rank(LdsWord* hist, LdsMask* masks, const uint32_t (&key)[kTileSortItems],
                                          uint32_t (&rank)[kTileSortItems], int ipl, int first, int m, int shift,
                                          uint32_t mask) {
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned long long me = 1ull << lane;
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;                                  // wave-uniform
        const bool valid = first + i * kWave + lane < m;
        const uint32_t d = (key[i] >> shift) & mask;
        if (valid) __hip_atomic_fetch_or(&masks[d], me, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_wave_barrier();
        const unsigned long long peers =
            valid ? __hip_atomic_load(&masks[d], __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_WAVEFRONT) : 0ull;
        const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
        uint32_t pre = 0;
        if (valid) pre = hist[d];
        __builtin_amdgcn_wave_barrier();
        if (valid && r == 0) {
            hist[d] = pre + (uint32_t)__popcll(peers);
            __hip_atomic_store(&masks[d], 0ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        __builtin_amdgcn_wave_barrier();
        rank[i] = pre + r;
    }
}

// Item i of this lane: entry e = first + 64 i of list[0, m), and its key.  All loads first, then all key gathers, with no
// lane-dependent branch in between: every item's load is in flight at once (a guarded load + gather per item made the compiler
// wait for each one in turn).  Lanes past the end load the last entry again: a copy of a valid key changes no AND / OR, and the
// ranking leaves those lanes out.  BY_ID (the id passes of a long list): the sort word is the id itself, nothing is gathered.
template <bool BY_ID = false>
__device__ __forceinline__ void load_items(const uint32_t* __restrict__ list, const uint32_t* __restrict__ depth_keys,
                                           uint32_t (&key)[kTileSortItems], uint32_t (&val)[kTileSortItems], int ipl, int first,
                                           int m) {
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;                                  // wave-uniform
        val[i] = list[min(first + i * kWave, m - 1)];
    }
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;
        key[i] = BY_ID ? val[i] & kGidMask : depth_keys[val[i] & kGidMask];
    }
}

// AND ^ OR over the wave of the first ipl sort words of every lane (`keep` masks them): the bits that differ in the list
__device__ __forceinline__ void wave_and_or(const uint32_t (&w)[kTileSortItems], int ipl, uint32_t keep, uint32_t& k_and,
                                            uint32_t& k_or) {
    k_and = 0xFFFFFFFFu; k_or = 0u;
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;
        k_and &= w[i] & keep;
        k_or |= w[i] & keep;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        k_and &= (uint32_t)__shfl_xor((int)k_and, d, kWave);
        k_or |= (uint32_t)__shfl_xor((int)k_or, d, kWave);
    }
}

// Ties.  The list may arrive in any order (the counting sort by tile is not stable), so after the key passes equal keys need not
// be in id order.  Every list path then holds the sorted list where entry e can see entry e + 1 and asks one question per entry:
// same key as the next one AND a larger id?  No such pair anywhere (nearly every tile: ties are a few hundred pairs per frame)
// and the list is final.  Otherwise the list is sorted by id first -- the same LSD passes, on the differing bits of
// val & kGidMask -- and the key passes run again: stable, so equal keys now keep the id order.  Linear in the list whatever the
// input; a list of ONE key skips the key passes on both sides.
__device__ __forceinline__ bool tie_out_of_order(uint32_t k0, uint32_t v0, uint32_t k1, uint32_t v1) {
    return k0 == k1 && (v0 & kGidMask) > (v1 & kGidMask);
}

// Four-wave ranking of one chunk of m entries (caller: a workgroup barrier since the key / value space was last read).
// Afterwards rank[i] + hist[wave][d] is an entry's position among the chunk's entries of digit d, dig_start[d] the chunk-local
// start of digit d.  Returns the chunk's count of digit `threadIdx.x`.
__device__ __forceinline__ uint32_t tile_sort_rank(TileSortLds& sm, const uint32_t (&key)[kTileSortItems],
                                                   uint32_t (&rank)[kTileSortItems], int ipl, int chunk, int m, int shift,
                                                   uint32_t mask) {
    const int tid = threadIdx.x, wave = tid >> 6;
    LdsWord* hist = lds_words(sm.hist[wave]);
    LdsMask* masks = wave_masks(sm, wave);
    wave_rank_clear(hist, masks);
    wave_rank(hist, masks, key, rank, ipl, wave * chunk, m, shift, mask);
    __syncthreads();
    uint32_t run_len = 0;
#pragma unroll
    for (int w = 0; w < kTileSortWaves; ++w) {
        const uint32_t t = sm.hist[w][tid];
        sm.hist[w][tid] = run_len;
        run_len += t;
    }
    uint32_t total;
    sm.dig_start[tid] = block_exclusive_scan(run_len, total, sm.scan_sums);
    __syncthreads();
    return run_len;
}

// The wave's LSD passes over the bits `diff` of the sort words `sel` (the keys, or the values for the id passes: their ids lie
// below the reach flag, and diff never holds that bit), key / value pairs moved through the wave's quarter of the LDS space.
// The sorted list is left there; reload_last: and in the registers again, entry i * 64 + lane in item i.
__device__ __forceinline__ void wave_lsd_passes(LdsWord* hist, LdsMask* masks, LdsWord* wk, LdsWord* wv,
                                                const uint32_t (&sel)[kTileSortItems], uint32_t (&key)[kTileSortItems],
                                                uint32_t (&val)[kTileSortItems], uint32_t (&rank)[kTileSortItems], int ipl,
                                                int n, uint32_t diff, bool reload_last) {
    const int lane = threadIdx.x & (kWave - 1);
    const int lo = __builtin_ctz(diff), hi = 31 - __builtin_clz(diff);
    const int npass = (hi - lo + 8) / 8;
    const int per = (hi - lo + npass) / npass;                   // ceil(span / npass) <= 8
    for (int p = 0; p < npass; ++p) {
        const int shift = lo + p * per, bits = min(per, hi + 1 - shift);
        const uint32_t mask = (1u << bits) - 1u;
        wave_rank_clear(hist, masks);
        wave_rank(hist, masks, sel, rank, ipl, 0, n, shift, mask);
        // digit starts: lane l scans digits 4l .. 4l + 3
        uint32_t c[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = hist[4 * lane + j]; sum += c[j]; }
        uint32_t run = wave_inclusive_scan(sum) - sum;
#pragma unroll
        for (int j = 0; j < 4; ++j) { hist[4 * lane + j] = run; run += c[j]; }
        __builtin_amdgcn_wave_barrier();
        // positions first (every item's LDS read in flight at once), then the guarded writes
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            rank[i] += hist[(sel[i] >> shift) & mask];
        }
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            if (i * kWave + lane < n) {
                wk[rank[i]] = key[i];
                wv[rank[i]] = val[i];
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (p + 1 < npass || reload_last) {
#pragma unroll
            for (int i = 0; i < kTileSortItems; ++i) {
                if (i >= ipl) continue;
                const int e = min(i * kWave + lane, n - 1);     // lanes past the end: a copy, left out of the ranking
                key[i] = wk[e];
                val[i] = wv[e];
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Timing probes of the one-wave path.  They give WRONG lists by construction, so the switches exist only in a
// -DOGS_EXPERIMENTS variant build; the shipped library compiles all three to `false`.
#if defined(OGS_EXPERIMENTS) && defined(OGS_TSORT_LOADS_ONLY)
constexpr bool kTsortLoadsOnly = true;       // loads, key gathers, AND / OR; nothing ranked, nothing written
#else
constexpr bool kTsortLoadsOnly = false;
#endif
#if defined(OGS_EXPERIMENTS) && defined(OGS_TSORT_SKIP_PASSES)
constexpr bool kTsortSkipPasses = true;      // the list goes through LDS and out again in the order it came in
#else
constexpr bool kTsortSkipPasses = false;
#endif
#if defined(OGS_EXPERIMENTS) && defined(OGS_TSORT_LSD_ONLY)
constexpr bool kTsortLsdOnly = true;         // the bucket path compiled out: the LSD passes alone (right lists)
#else
constexpr bool kTsortLsdOnly = false;
#endif

// min / max over the wave of the first ipl sort words of every lane (`keep` masks them)
__device__ __forceinline__ void wave_min_max(const uint32_t (&w)[kTileSortItems], int ipl, uint32_t keep, uint32_t& w_min,
                                             uint32_t& w_max) {
    w_min = 0xFFFFFFFFu; w_max = 0u;
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;
        w_min = min(w_min, w[i] & keep);
        w_max = max(w_max, w[i] & keep);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        w_min = min(w_min, (uint32_t)__shfl_xor((int)w_min, d, kWave));
        w_max = max(w_max, (uint32_t)__shfl_xor((int)w_max, d, kWave));
    }
}

typedef __attribute__((address_space(3))) uint32_t LdsCount;
typedef __attribute__((address_space(3))) volatile unsigned long long LdsPair;

// The ranking loop of wave_bucket_rank over the first IPL items of every lane, without a branch inside a step (a guard per
// item cost more than the step's reads).  cw: the bucket's count << 16 | the entries found smaller so far -- 0 for an item that
// takes no part, which then reads some entry of the list and counts nothing.  t < count  <=>  (t << 16 | 0xFFFF) < cw, whatever
// cw's low half (below the count) holds.  The reads of a step are independent of each other and of the step before.
constexpr int kRankGroup = 8;                  // reads in flight per lane
template <int IPL>
__device__ __forceinline__ void bucket_rank_steps(LdsPair* pairs, const unsigned long long (&mine)[kTileSortItems],
                                                  const uint32_t (&st)[kTileSortItems], uint32_t (&cw)[kTileSortItems], int cmax,
                                                  int n) {
#pragma unroll 1
    for (int t = 0; t < cmax; ++t) {
        const uint32_t tt = ((uint32_t)t << 16) | 0xFFFFu;
#pragma unroll
        for (int g = 0; g < IPL; g += kRankGroup) {
            unsigned long long other[kRankGroup];
#pragma unroll
            for (int i = g; i < min(IPL, g + kRankGroup); ++i)
                other[i - g] = pairs[min((int)st[i] + t, n - 1)];                       // past the bucket: not counted
#pragma unroll
            for (int i = g; i < min(IPL, g + kRankGroup); ++i)
                cw[i] += (tt < cw[i] && other[i - g] < mine[i]) ? 1u : 0u;              // against itself: 0
        }
    }
}

// One-wave path, lists of distinct (key, id): one bucket pass that is NOT stable, then every entry is ranked inside its bucket on
// the total order (key, id).  The digit is (key - the list's smallest key) >> shift, the shift that leaves kBucketBits bits of
// the list's key range (the ids' when the list has ONE key): monotone, so bucket d holds only entries smaller than those of
// bucket d + 1, and at least half of the buckets lie inside the range -- the top differing bits of two floats either side of a
// power of two are their exponents, two buckets for the whole list.  An entry takes its slot with one LDS atomic with return
// (all of a lane's atomics are in flight at once), the counts are scanned into bucket starts, (key, id word) pairs go to
// start + slot, and the final position is start + the bucket's entries that compare less: the same for any arrival order.
// The id word is the value rotated by one, the id above the reach flag: ids are distinct, so the words order as the ids do.
// Returns false with nothing moved (key / val untouched) when the largest bucket holds more than bucket_cap entries -- the
// ranking loop costs its length for the whole wave -- and the caller then runs the LSD passes; true with the values in wv.
constexpr int kBucketBits = 8;                 // 256 counts per wave: TileSortLds::hist, nothing new in LDS
__device__ __forceinline__ bool wave_bucket_rank(LdsWord* hist, LdsWord* wk, LdsWord* wv, const uint32_t (&key)[kTileSortItems],
                                                 const uint32_t (&val)[kTileSortItems], int ipl, int n, int bucket_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t w_min, w_max;
    wave_min_max(key, ipl, 0xFFFFFFFFu, w_min, w_max);
    const bool by_id = __builtin_amdgcn_readfirstlane((int)w_min) == __builtin_amdgcn_readfirstlane((int)w_max);     // wave-uniform
    if (by_id) wave_min_max(val, ipl, kGidMask, w_min, w_max);
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_min);
    const uint32_t range = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_max) - base;
    if (range == 0u) return false;                               // (a list of ONE id: not a tile's list; the passes leave it alone)
    const int shift = max(0, 32 - __builtin_clz(range) - kBucketBits);           // range >> shift < 1 << kBucketBits
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[lane + j * kWave] = 0u;
    __builtin_amdgcn_wave_barrier();
    uint32_t slot[kTileSortItems];
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;                                  // wave-uniform
        const uint32_t d = ((by_id ? val[i] & kGidMask : key[i]) - base) >> shift;
        slot[i] = 0u;
        if (i * kWave + lane < n)
            slot[i] = __hip_atomic_fetch_add((LdsCount*)(hist + d), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    __builtin_amdgcn_wave_barrier();
    // bucket starts: lane l scans digits 4l .. 4l + 3; the largest count decides the path
    uint32_t c[4], sum = 0, big = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = hist[4 * lane + j]; sum += c[j]; big = max(big, c[j]); }
    uint32_t run = wave_inclusive_scan(sum) - sum;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) big = max(big, (uint32_t)__shfl_xor((int)big, d, kWave));
    const int cmax = __builtin_amdgcn_readfirstlane((int)big);
    if (cmax > bucket_cap) return false;
#pragma unroll
    for (int j = 0; j < 4; ++j) { hist[4 * lane + j] = run | (c[j] << 10); run += c[j]; }        // start < 1024 where count > 0
    __builtin_amdgcn_wave_barrier();
    // n pairs: the whole quarter at n = kWaveSortCap.  A lane past the end holds a copy of the last entry, which is never
    // scattered and takes no part in the ranking
    LdsPair* pairs = (LdsPair*)wk;
    unsigned long long mine[kTileSortItems];
    uint32_t st[kTileSortItems], cw[kTileSortItems];
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {                   // start | count << 10 | slot << 21 in one register
        if (i >= ipl) continue;
        slot[i] = hist[((by_id ? val[i] & kGidMask : key[i]) - base) >> shift] | (slot[i] << 21);
    }
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        uint32_t s_i = 0u, c_i = 0u;                             // an item past ipl takes no part (and is not read below
        unsigned long long m_i = 0ull;                           // unless its group of the ranking loop holds a live one)
        if (i < ipl) {
            const bool valid = i * kWave + lane < n;
            c_i = valid ? ((slot[i] >> 10) & 0x7FFu) << 16 : 0u;
            s_i = slot[i] & 0x3FFu;
            m_i = ((unsigned long long)key[i] << 32) | (unsigned long long)((val[i] << 1) | (val[i] >> 31));
            if (valid) pairs[s_i + (slot[i] >> 21)] = m_i;
        }
        st[i] = s_i; cw[i] = c_i; mine[i] = m_i;
    }
    __builtin_amdgcn_wave_barrier();
    if (ipl <= 4) bucket_rank_steps<4>(pairs, mine, st, cw, cmax, n);
    else if (ipl <= 8) bucket_rank_steps<8>(pairs, mine, st, cw, cmax, n);
    else if (ipl <= 12) bucket_rank_steps<12>(pairs, mine, st, cw, cmax, n);
    else bucket_rank_steps<kTileSortItems>(pairs, mine, st, cw, cmax, n);
    __builtin_amdgcn_wave_barrier();                             // every pair has been read: the values may overwrite them
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;
        const uint32_t w = (uint32_t)mine[i];                    // the value back from its id word
        if (i * kWave + lane < n) wv[st[i] + (cw[i] & 0xFFFFu)] = (w >> 1) | (w << 31);
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// One wave sorts a list of 2 .. kWaveSortCap entries in its quarter of the key / value space: buckets and the ranking inside
// them when no bucket holds more than bucket_cap entries, otherwise the stable LSD passes and the look at the ties.
__device__ __forceinline__ void wave_sort_list(TileSortLds& sm, uint32_t* __restrict__ seg, int n,
                                               const uint32_t* __restrict__ depth_keys, int bucket_cap) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    LdsWord* wk = lds_words(sm.kv + wave * 2 * kWaveSortCap);
    LdsWord* wv = wk + kWaveSortCap;
    LdsWord* hist = lds_words(sm.hist[wave]);
    LdsMask* masks = wave_masks(sm, wave);
    uint32_t key[kTileSortItems], val[kTileSortItems], rank[kTileSortItems];
    const int ipl = (n + kWave - 1) / kWave;
    load_items(seg, depth_keys, key, val, ipl, lane, n);
    uint32_t k_and, k_or;
    wave_and_or(key, ipl, 0xFFFFFFFFu, k_and, k_or);
    const uint32_t kdiff = (uint32_t)__builtin_amdgcn_readfirstlane((int)(k_and ^ k_or));
    if (kTsortLoadsOnly) {
        if (kdiff == 0x5A5A5A5Au) seg[0] = key[0];               // (keeps the loads alive)
        return;
    }
    if (kTsortSkipPasses) {
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            if (i * kWave + lane < n) { wk[i * kWave + lane] = key[i]; wv[i * kWave + lane] = val[i]; }
        }
        __builtin_amdgcn_wave_barrier();
        for (int j = lane; j < n; j += kWave) seg[j] = wv[j];
        return;
    }
    if (!kTsortLsdOnly && wave_bucket_rank(hist, wk, wv, key, val, ipl, n, bucket_cap)) {
        for (int j = lane; j < n; j += kWave) seg[j] = wv[j];
        return;
    }
    if (kdiff != 0u) {
        wave_lsd_passes(hist, masks, wk, wv, key, key, val, rank, ipl, n, kdiff, false);
    } else {                                                     // one key for the whole list: only the id order is open
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            if (i * kWave + lane < n) { wk[i * kWave + lane] = key[i]; wv[i * kWave + lane] = val[i]; }
        }
        __builtin_amdgcn_wave_barrier();
    }
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kTileSortItems; ++i) {
        if (i >= ipl) continue;
        const int e = min(i * kWave + lane, n - 2);              // n >= 2; lanes past the end repeat the last pair
        if (wk[e] == wk[e + 1]) bad |= (wv[e] & kGidMask) > (wv[e + 1] & kGidMask);       // (the values: rarely read)
    }
    if (__ballot(bad) != 0ull) {                                 // wave-uniform
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            const int e = min(i * kWave + lane, n - 1);
            key[i] = wk[e];
            val[i] = wv[e];
        }
        __builtin_amdgcn_wave_barrier();
        wave_and_or(val, ipl, kGidMask, k_and, k_or);
        const uint32_t gdiff = (uint32_t)__builtin_amdgcn_readfirstlane((int)(k_and ^ k_or));      // != 0: the ids of a tile differ
        if (gdiff != 0u) wave_lsd_passes(hist, masks, wk, wv, val, key, val, rank, ipl, n, gdiff, kdiff != 0u);
        if (kdiff != 0u) wave_lsd_passes(hist, masks, wk, wv, key, key, val, rank, ipl, n, kdiff, false);
    } else if (kdiff == 0u) {
        return;                                                  // already in id order: nothing moved
    }
    for (int j = lane; j < n; j += kWave) seg[j] = wv[j];
}

// AND / OR over the workgroup of one word pair per thread, through sm.red; returns AND ^ OR, the OR comes back in all_or
__device__ __forceinline__ uint32_t block_and_or(TileSortLds& sm, uint32_t k_and, uint32_t k_or, uint32_t& all_or) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        k_and &= (uint32_t)__shfl_xor((int)k_and, d, kWave);
        k_or |= (uint32_t)__shfl_xor((int)k_or, d, kWave);
    }
    __syncthreads();                                             // the last reduction has been read
    if (tid < 2) sm.red[tid] = tid == 0 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    if ((tid & (kWave - 1)) == 0) { atomicAnd(&sm.red[0], k_and); atomicOr(&sm.red[1], k_or); }
    __syncthreads();
    all_or = sm.red[1];
    return sm.red[0] ^ all_or;
}

// The workgroup's LSD passes over the bits `diff` of the sort words `sel` (keys, or values for the id passes) of a list of
// n <= kTileSortCap entries held in registers, entry wave * chunk + 64 i + lane in item i.  The sorted list is left in the
// key / value space (a barrier behind it); reload_last: and in the registers again.
__device__ __forceinline__ void block_lsd_passes(TileSortLds& sm, const uint32_t (&sel)[kTileSortItems],
                                                 uint32_t (&key)[kTileSortItems], uint32_t (&val)[kTileSortItems],
                                                 uint32_t (&rank)[kTileSortItems], int ipl, int chunk, int n, uint32_t diff,
                                                 bool reload_last) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = __builtin_ctz(diff), hi = 31 - __builtin_clz(diff);
    const int npass = (hi - lo + 8) / 8;
    const int per = (hi - lo + npass) / npass;
    uint32_t* const sk = sm.kv;
    uint32_t* const sv = sm.kv + kTileSortCap;
    for (int p = 0; p < npass; ++p) {
        const int shift = lo + p * per, bits = min(per, hi + 1 - shift);
        const uint32_t mask = (1u << bits) - 1u;
        tile_sort_rank(sm, sel, rank, ipl, chunk, n, shift, mask);
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            const uint32_t d = (sel[i] >> shift) & mask;
            rank[i] += sm.dig_start[d] + sm.hist[wave][d];
        }
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            if (wave * chunk + i * kWave + lane < n) {
                sk[rank[i]] = key[i];
                sv[rank[i]] = val[i];
            }
        }
        __syncthreads();
        if (p + 1 < npass || reload_last) {
#pragma unroll
            for (int i = 0; i < kTileSortItems; ++i) {
                if (i >= ipl) continue;
                const int e = min(wave * chunk + i * kWave + lane, n - 1);
                key[i] = sk[e];
                val[i] = sv[e];
            }
            __syncthreads();                                     // read before the next pass' masks overwrite the space
        }
    }
}

// Long list (more than kTileSortCap entries): the LSD passes over the bits `diff` of the sort words stream the list through the
// chunk ranking, global memory in and out, ping-pong between seg and alt; the sorted list ends in seg, complete for the whole
// workgroup.  BY_ID: the sort word of a value is its id, otherwise the depth key gathered by it.
template <bool BY_ID>
__device__ __forceinline__ void long_lsd_passes(TileSortLds& sm, uint32_t* __restrict__ seg, uint32_t* __restrict__ alt, int n,
                                                const uint32_t* __restrict__ depth_keys, uint32_t diff) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t key[kTileSortItems], val[kTileSortItems], rank[kTileSortItems];
    const int lo = __builtin_ctz(diff), hi = 31 - __builtin_clz(diff);
    const int npass = (hi - lo + 8) / 8;
    const int per = (hi - lo + npass) / npass;
    for (int p = 0; p < npass; ++p) {
        const int shift = lo + p * per, bits = min(per, hi + 1 - shift);
        const uint32_t mask = (1u << bits) - 1u;
        const uint32_t* __restrict__ src = (p & 1) ? alt : seg;
        uint32_t* __restrict__ dst = (p & 1) ? seg : alt;
        sm.base[tid] = 0u;
        __syncthreads();
        for (int j = tid; j < n; j += kBlock) {
            const uint32_t v = src[j] & kGidMask;
            atomicAdd(&sm.base[((BY_ID ? v : depth_keys[v]) >> shift) & mask], 1u);
        }
        __syncthreads();
        uint32_t total;
        const uint32_t start = block_exclusive_scan(sm.base[tid], total, sm.scan_sums);
        sm.base[tid] = start;
        for (int c0 = 0; c0 < n; c0 += kTileSortCap) {
            const int m = min(kTileSortCap, n - c0);
            const int ipl = (m + kBlock - 1) / kBlock, chunk = ipl * kWave;
            load_items<BY_ID>(src + c0, depth_keys, key, val, ipl, wave * chunk + lane, m);
            const uint32_t cnt = tile_sort_rank(sm, key, rank, ipl, chunk, m, shift, mask);
#pragma unroll
            for (int i = 0; i < kTileSortItems; ++i) {
                if (i >= ipl) continue;
                if (wave * chunk + i * kWave + lane < m) {
                    const uint32_t d = (key[i] >> shift) & mask;
                    dst[sm.base[d] + sm.hist[wave][d] + rank[i]] = val[i];
                }
            }
            __syncthreads();                                     // every read of base[] and hist[] of this chunk is done
            sm.base[tid] += cnt;
        }
        __syncthreads();                                         // dst complete (workgroup-scope fence) before it is read as src
    }
    if (npass & 1) {
        for (int j = tid; j < n; j += kBlock) seg[j] = alt[j];
        __syncthreads();
    }
}

// The whole workgroup sorts one list of more than kWaveSortCap entries.
__device__ __forceinline__ void block_sort_list(TileSortLds& sm, uint32_t* __restrict__ seg, uint32_t* __restrict__ alt, int n,
                                                const uint32_t* __restrict__ depth_keys) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t any;
    __syncthreads();                                             // the previous list's use of the LDS is over
    if (n <= kTileSortCap) {
        uint32_t key[kTileSortItems], val[kTileSortItems], rank[kTileSortItems];
        uint32_t* const sk = sm.kv;
        uint32_t* const sv = sm.kv + kTileSortCap;
        const int ipl = (n + kBlock - 1) / kBlock, chunk = ipl * kWave;
        load_items(seg, depth_keys, key, val, ipl, wave * chunk + lane, n);
        uint32_t k_and = 0xFFFFFFFFu, k_or = 0u;
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            k_and &= key[i];
            k_or |= key[i];
        }
        const uint32_t kdiff = block_and_or(sm, k_and, k_or, any);           // block-uniform, as everything decided from it
        if (kdiff != 0u) {
            block_lsd_passes(sm, key, key, val, rank, ipl, chunk, n, kdiff, false);
        } else {                                                 // one key for the whole list: only the id order is open
#pragma unroll
            for (int i = 0; i < kTileSortItems; ++i) {
                if (i >= ipl) continue;
                const int e = wave * chunk + i * kWave + lane;
                if (e < n) { sk[e] = key[i]; sv[e] = val[i]; }
            }
            __syncthreads();
        }
        bool bad = false;
#pragma unroll
        for (int i = 0; i < kTileSortItems; ++i) {
            if (i >= ipl) continue;
            const int e = min(wave * chunk + i * kWave + lane, n - 2);
            if (sk[e] == sk[e + 1]) bad |= (sv[e] & kGidMask) > (sv[e + 1] & kGidMask);
        }
        block_and_or(sm, 0xFFFFFFFFu, bad ? 1u : 0u, any);
        if (any != 0u) {
            k_and = 0xFFFFFFFFu; k_or = 0u;
#pragma unroll
            for (int i = 0; i < kTileSortItems; ++i) {
                if (i >= ipl) continue;
                const int e = min(wave * chunk + i * kWave + lane, n - 1);
                key[i] = sk[e];
                val[i] = sv[e];
                k_and &= val[i] & kGidMask;
                k_or |= val[i] & kGidMask;
            }
            const uint32_t gdiff = block_and_or(sm, k_and, k_or, any);       // (its barriers: the reads above are done)
            if (gdiff != 0u) block_lsd_passes(sm, val, key, val, rank, ipl, chunk, n, gdiff, kdiff != 0u);
            if (kdiff != 0u) block_lsd_passes(sm, key, key, val, rank, ipl, chunk, n, kdiff, false);
        } else if (kdiff == 0u) {
            return;                                              // already in id order: nothing moved
        }
        for (int j = tid; j < n; j += kBlock) seg[j] = sv[j];
        return;
    }

    uint32_t k_and = 0xFFFFFFFFu, k_or = 0u;
    for (int j = tid; j < n; j += kBlock) {
        const uint32_t k = depth_keys[seg[j] & kGidMask];
        k_and &= k;
        k_or |= k;
    }
    const uint32_t kdiff = block_and_or(sm, k_and, k_or, any);
    if (kdiff != 0u) long_lsd_passes<false>(sm, seg, alt, n, depth_keys, kdiff);
    bool bad = false;
    k_and = 0xFFFFFFFFu; k_or = 0u;
    for (int j = tid; j < n; j += kBlock) {
        const uint32_t v0 = seg[j], v1 = seg[min(j + 1, n - 1)];
        bad |= tie_out_of_order(depth_keys[v0 & kGidMask], v0, depth_keys[v1 & kGidMask], v1);
        k_and &= v0 & kGidMask;
        k_or |= v0 & kGidMask;
    }
    const uint32_t gdiff = block_and_or(sm, k_and, k_or | (bad ? 0x80000000u : 0u), any) & kGidMask;     // bit 31: the flag
    if ((any & 0x80000000u) == 0u || gdiff == 0u) return;
    long_lsd_passes<true>(sm, seg, alt, n, depth_keys, gdiff);
    if (kdiff != 0u) long_lsd_passes<false>(sm, seg, alt, n, depth_keys, kdiff);
}


__global__ __launch_bounds__(kBlock) void tile_depth_sort_kernel(const uint2* __restrict__ ranges, int tiles,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 uint32_t* __restrict__ point_list,
                                                                 const uint32_t* __restrict__ depth_keys,
                                                                 uint32_t* __restrict__ scratch, int bucket_cap) {
    __shared__ TileSortLds sm;
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x < kTileSortWaves) {
        const int b = blockIdx.x * kTileSortWaves + threadIdx.x;
        sm.range[threadIdx.x] = b < tiles ? ranges[tile_order ? tile_order[b] : (uint32_t)b] : make_uint2(0u, 0u);
    }
    __syncthreads();
    // (readfirstlane: the list bounds are uniform -- the addresses then live in SGPRs, not in 2 VGPRs per item)
    const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)sm.range[wave].x);
    const int n = __builtin_amdgcn_readfirstlane((int)(sm.range[wave].y - sm.range[wave].x));
    if (n >= 2 && n <= kWaveSortCap) wave_sort_list(sm, point_list + x, n, depth_keys, bucket_cap);
#pragma unroll 1
    for (int w = 0; w < kTileSortWaves; ++w) {
        const uint32_t xw = (uint32_t)__builtin_amdgcn_readfirstlane((int)sm.range[w].x);
        const int nw = __builtin_amdgcn_readfirstlane((int)(sm.range[w].y - sm.range[w].x));
        if (nw > kWaveSortCap) block_sort_list(sm, point_list + xw, scratch + xw, nw, depth_keys);        // block-uniform
    }
}

__global__ __launch_bounds__(kBlock) void export_keys_kernel(const uint2* __restrict__ ranges,
                                                             const uint32_t* __restrict__ point_list,
                                                             const float4* __restrict__ rec, int recv4,
                                                             uint64_t* __restrict__ keys_out) {
    const uint32_t tile = blockIdx.x;
    const uint2 r = ranges[tile];
    for (uint32_t i = r.x + threadIdx.x; i < r.y; i += kBlock) {
        const uint32_t gid = point_list[i] & kGidMask;          // top bit: "reaches the tile" flag (ogs_common.h)
        const uint32_t bits = __float_as_uint(rec[(size_t)gid * recv4].z);
        keys_out[i] = ((uint64_t)tile << 32) | bits;
    }
}

}  // namespace

int launch_tile_ranges(const uint32_t* tile_keys_sorted, int64_t D, uint2* ranges, int64_t tiles, hipStream_t s,
                       int debug, const uint32_t* n_dev, bool already_zeroed) {
    if (!already_zeroed) OGS_HIP_CHECK(hipMemsetAsync(ranges, 0, (size_t)tiles * sizeof(uint2), s));
    if (D <= 0) return OGS_OK;
    const int grid = (int)((D + (int64_t)kBlock * kRangeItems - 1) / ((int64_t)kBlock * kRangeItems));
    OGS_LAUNCH(tile_ranges_kernel, dim3(grid), dim3(kBlock), 0, s, tile_keys_sorted, D, n_dev, ranges);
    OGS_LAUNCH_CHECK(debug, s);
    return OGS_OK;
}

// test hooks (ogs_raster_tile_count_debug): a forced chunk count, a reversed walk in tile_place_kernel
static int g_tile_count_force = 0;
static bool g_tile_place_reverse = false;
void tile_count_debug(int force_blocks, int reverse) {
    if (force_blocks >= 0) g_tile_count_force = force_blocks;
    if (reverse >= 0) g_tile_place_reverse = reverse != 0;
}
int tile_count_trip() { return kCountTrip; }

// B, the number of chunks (= workgroups of tile_count_kernel), or 0: the pass takes the radix sort.
// The table of (B + 1) x tiles words (B rows of counts, one of totals) lives in a D-word key buffer; one chunk per trip of
// keys at the most.
int tile_count_blocks(int64_t D, int64_t tiles) {
    if (tiles < 1 || tiles > kTileCountMaxTiles || D < 2 * tiles) return 0;
    const int64_t trips = (D + kCountTrip - 1) / kCountTrip;
    int64_t B = g_tile_count_force > 0 ? g_tile_count_force : (trips < kTileCountBlocks ? trips : kTileCountBlocks);
    if (B > D / tiles - 1) B = D / tiles - 1;
    return (int)B;
}

// test hooks (ogs_raster_tile_place_debug): forced G (count chunks per place chunk), S (tile slices) and staging words; 0: the rule
static int g_tile_place_group = 0, g_tile_place_slices = 0, g_tile_place_stage = 0;
void tile_place_debug(int group, int slices, int stage_words) {
    if (group >= 0) g_tile_place_group = group;
    if (slices >= 0) g_tile_place_slices = slices;
    if (stage_words >= 0) g_tile_place_stage = stage_words;
}

constexpr size_t kPlaceLdsBytes = 160 * 1024 - 256;               // dynamic: what one workgroup may declare less the kernel's static words
constexpr int kPlaceMaxSlices = 1024;                             // what the hook may force
constexpr int kPlaceGrid = 256, kPlaceOwnSlices = 4;              // the rule: workgroups to fill the chip with, slices at the most
constexpr int kPlaceStageTrips = 2;                               // and the trips a chunk has room for before it stages

// The grid of tile_place_kernel for a pass of B count chunks: ceil(B / G) place chunks x S slices, and its staging words
// (0: every workgroup stores straight from the walk).  From what the host knows -- the capacity D, the grid, B -- and the hooks.
// DESIGN 3i has the sweep behind the rule.
TilePlacePlan tile_place_plan(int64_t D, int64_t tiles, int B) {
    TilePlacePlan pl = {0, 0, 0, 0};
    if (B < 1 || tiles < 1) return pl;
    // The rule: a pass whose chunks have room for kPlaceStageTrips trips or more (the streaming workloads from 2.6 M pairs up, at
    // B = 128) stages, with G = 1 and as many slices, kPlaceOwnSlices at the most, as make the grid the size of the chip.  The
    // kernel's time is one workgroup's chain of trips: longer place chunks (G > 1) lose more than their longer runs save, a second
    // slice halves the staged entries per workgroup.  Shorter chunks (one trip each below kTileCountBlocks chunks; 0.44 M pairs
    // over 2500 tiles at B = 128) keep the direct path, G = S = 1, where the sweep found nothing to gain.
    const bool rule = D >= (int64_t)kPlaceStageTrips * kCountTrip * B;
    int G = 1, S = 1;
    if (rule) S = kPlaceGrid / B < 1 ? 1 : kPlaceGrid / B > kPlaceOwnSlices ? kPlaceOwnSlices : kPlaceGrid / B;
    if (g_tile_place_group > 0) G = g_tile_place_group;
    if (g_tile_place_slices > 0) S = g_tile_place_slices < kPlaceMaxSlices ? g_tile_place_slices : kPlaceMaxSlices;
    if (G > B) G = B;
    const int64_t per_slice = (tiles + S - 1) / S;
    const int64_t room = ((int64_t)kPlaceLdsBytes - 8 * per_slice) / kPlaceEntryBytes;     // > 0: tiles <= kTileCountMaxTiles
    // no more words than a place chunk has pairs: G chunks of ceil(D / B) pairs rounded up to the trip
    const int64_t span = G * (((D + B - 1) / B + kCountTrip - 1) / kCountTrip * kCountTrip);
    int64_t W = g_tile_place_stage > 0 ? g_tile_place_stage : (rule || G > 1 || S > 1) ? span : 0;
    if (W > room) W = room;
    pl.group = G;
    pl.chunks = (B + G - 1) / G;
    pl.slices = S;
    pl.stage_words = (uint32_t)W;
    return pl;
}

int launch_tile_count_binning(const uint32_t* keys, const uint32_t* vals, int64_t D, const uint32_t* n_dev, int B, int64_t tiles,
                              uint32_t* table, uint2* ranges, uint32_t* kept, uint32_t* point_list, hipStream_t s, int debug) {
    if (B < 1 || tiles < 1 || tiles > kTileCountMaxTiles || ((int64_t)B + 1) * tiles > D) {
        set_error("tile_count_binning: B=%d tiles=%lld D=%lld", B, (long long)tiles, (long long)D); return OGS_ERR_INVALID_ARG;
    }
    const size_t lds = (size_t)tiles * sizeof(uint32_t);
    OGS_LAUNCH(tile_count_kernel, dim3(B), dim3(kCountBlock), lds, s, keys, D, n_dev, (int)tiles, table);
    OGS_LAUNCH_CHECK(debug, s);
    const int cols = (int)((tiles + kCountScanCols - 1) / kCountScanCols);
    OGS_LAUNCH(tile_count_scan_kernel, dim3(cols), dim3(kCountScanCols * kCountScanGroups), 0, s, table, B, (int)tiles);
    OGS_LAUNCH_CHECK(debug, s);
    const TilePlacePlan pl = tile_place_plan(D, tiles, B);
    const size_t per_slice = (size_t)((tiles + pl.slices - 1) / pl.slices);
    const size_t place_lds = pl.stage_words ? (8 * per_slice + (size_t)kPlaceEntryBytes * pl.stage_words + 15) / 16 * 16
                                            : per_slice * sizeof(uint32_t);
    if (place_lds > 48 * 1024) {                                  // the function's dynamic LDS limit is raised once per device
        static std::atomic<bool> raised[64];
        int dev = 0;
        OGS_HIP_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_relaxed)) {
            OGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tile_place_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPlaceLdsBytes));
            if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_relaxed);
        }
    }
    OGS_LAUNCH(tile_place_kernel, dim3(pl.chunks, pl.slices), dim3(kCountBlock), place_lds, s, keys, vals, D, n_dev, (int)tiles, B,
               pl.group, pl.stage_words, (const uint32_t*)table, ranges, kept, point_list, (uint32_t)D, g_tile_place_reverse);
    OGS_LAUNCH_CHECK(debug, s);
    return OGS_OK;
}

// test hook (ogs_raster_tile_sort_debug): the forced bucket cap of the one-wave path; 0: the rule
static int g_tile_sort_bucket_cap = 0;
void tile_sort_debug(int bucket_cap) {
    if (bucket_cap >= 0) g_tile_sort_bucket_cap = bucket_cap;
}
int tile_sort_bucket_cap() { return g_tile_sort_bucket_cap > 0 ? g_tile_sort_bucket_cap : kWaveBucketCap; }

int launch_tile_depth_sort(const uint2* ranges, int64_t tiles, const uint32_t* tile_order, uint32_t* point_list,
                           const uint32_t* depth_keys, uint32_t* scratch, hipStream_t s, int debug) {
    if (tiles <= 0) return OGS_OK;
    if (tiles >= (1ll << 31)) { set_error("tile_depth_sort: %lld tiles", (long long)tiles); return OGS_ERR_UNSUPPORTED; }
    const unsigned grid = (unsigned)((tiles + kTileSortWaves - 1) / kTileSortWaves);
    OGS_LAUNCH(tile_depth_sort_kernel, dim3(grid), dim3(kBlock), 0, s, ranges, (int)tiles, tile_order, point_list, depth_keys,
               scratch, tile_sort_bucket_cap());
    OGS_LAUNCH_CHECK(debug, s);
    return OGS_OK;
}

int launch_export_keys(const uint2* ranges, int tiles, const uint32_t* point_list, const float4* rec, int recv4,
                       uint64_t* keys_out, hipStream_t s) {
    OGS_LAUNCH(export_keys_kernel, dim3(tiles), dim3(kBlock), 0, s, ranges, point_list, rec, recv4, keys_out);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // namespace ogs
