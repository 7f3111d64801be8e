// Exact k-means++ (D^2) seeding for the wide k-means, with triangle-inequality pruning (include/ogs_kmeans.h, "wide seeding").
//
// Round r picks one row by an integer draw over per-row masses, makes it centre r, and lowers every row's squared distance to its
// nearest centre so far.  Per round, all on the caller's stream, nothing read back:
//   seed_pick_kernel   one workgroup: scans the per-block mass sums, finds the block, then the row inside it; writes rows[r], C[r]
//   seed_cc_kernel     dist(C[r], C[j]) for j < r (pruning only)
//   seed_row_kernel    a wave reads d2 / ids of 64 rows (8 bytes a row), applies the bound per lane, and only the rows that fail it
//                      are streamed: the whole wave on one row (D > 128), or sub-wave groups of G lanes on 64 / G rows.  The new
//                      centre sits in registers.  Then the block's integer mass sum: one writer per element, no atomics.
// dist() is ONE summation order for every D, alignment and group size: element j goes to accumulator j mod 256 (lane (j mod 256) / 4,
// component j mod 4), each accumulator adds in ascending j, then a binary tree over the 256 accumulators (pairs q, q ^ 1, then q ^ 2,
// ...): inside a lane (a0 + a1) + (a2 + a3), then an xor butterfly over the lanes.  Accumulators past D hold exact zeros, so a group
// of G >= D / 4 lanes computes the same bits as the whole wave.  Compiled with -ffp-contract=off: differences first, no FMA.
#include "ogs_common.h"
#include "../../include/ogs_kmeans.h"

namespace ogs {
namespace {

constexpr int kSeedRows = 256;                   // rows of one row-pass workgroup (a chunk of 64 per wave) and of one block sum: small, so
                                                 // that 500 k rows already fill the card with waves
constexpr int kSeedChunks = kSeedRows / kBlock;
constexpr int kSeedPick = 1024;                  // threads of the pick workgroup
static_assert(kSeedRows % kBlock == 0 && kSeedRows <= kSeedPick, "whole chunks per wave; one pick scan covers a block's rows");

struct SeedState {
    int32_t E;          // frexp exponent of the largest mass value: E0 before round 0, E of the rounds r >= 1 after it
    int32_t done;       // set by the pick that found no mass left
    int32_t seeded;     // the round that found none (valid when done)
    int32_t pad;
};

struct SeedTmp {
    SeedState* st;
    uint64_t* beval;    // [nb] (row, round) pairs evaluated by block b, summed over the rounds r >= 1
    uint64_t* bsum;     // [nb] integer mass of block b
    float* bmax;        // [nb] largest mass value of block b
    float* cc;          // [k]  dist(C[r], C[j]) of the current round
    float* d2;          // [N]  used when the caller passes no d2
    int32_t* ids;       // [N]  used when the caller passes no ids
    size_t head, bytes; // head: the bytes cleared at the start of a call (st, beval)
    static int64_t blocks(int64_t N) { return (N + kSeedRows - 1) / kSeedRows; }
    static SeedTmp carve(void* p, int64_t N, int k) {
        Carver c(p);
        SeedTmp t;
        const size_t nb = (size_t)blocks(N);
        t.st = c.take<SeedState>(1);
        t.beval = c.take<uint64_t>(nb);
        t.head = c.off;
        t.bsum = c.take<uint64_t>(nb);
        t.bmax = c.take<float>(nb);
        t.cc = c.take<float>((size_t)k);
        t.d2 = c.take<float>((size_t)N);
        t.ids = c.take<int32_t>((size_t)N);
        t.bytes = c.off;
        return t;
    }
};

bool seed_sizes_ok(int64_t N, int D, int k) {
    return N >= 0 && N < ((int64_t)1 << 31) && D >= 1 && (size_t)D <= ogs_kmeans_wide_max_dim() && k >= 1 &&
           (size_t)k <= ogs_kmeans_wide_max_k();
}

// lanes that share one row: the power of two >= ceil(D / 4), at most the wave
int seed_group(int D) {
    int G = 1;
    while (G < kWave && 4 * G < D) G <<= 1;
    return G;
}

__device__ __forceinline__ uint64_t seed_rand64(uint64_t seed, uint32_t r) {       // splitmix64
    uint64_t z = seed + (uint64_t)(r + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// mass value of row i: w_i (round 0: d2 == nullptr) or fl32(w_i * d2_i)
__device__ __forceinline__ float seed_value(const float* __restrict__ w, const float* __restrict__ d2, int64_t i) {
    return (w ? w[i] : 1.f) * (d2 ? d2[i] : 1.f);
}
// its integer mass q_i = floor(ldexp(value, 31 - E)) < 2^31
__device__ __forceinline__ uint64_t seed_mass(float value, int E) { return (uint64_t)(uint32_t)floorf(ldexpf(value, 31 - E)); }

// The pruning rule (header: "Pruning").  d = d2_i, b = dist(C[r], C[ids_i]); true when dist(y_i, C[r]) >= d is certain.
__device__ __forceinline__ bool seed_skip(float d, float b) {
    return d == 0.f || (d >= 0x1p-100f && b * (1.f - 0x1p-10f) >= 4.f * d * (1.f + 0x1p-10f));
}

// four elements j0 .. j0 + 3 of a row of D floats, zeros past D; vec: the row starts on a 16-byte boundary
__device__ __forceinline__ float4 seed_load4(const float* __restrict__ p, int j0, int D, bool vec) {
    if (vec && j0 + 3 < D) return *reinterpret_cast<const float4*>(p + j0);
    float4 v;
    v.x = j0 < D ? p[j0] : 0.f;
    v.y = j0 + 1 < D ? p[j0 + 1] : 0.f;
    v.z = j0 + 2 < D ? p[j0 + 2] : 0.f;
    v.w = j0 + 3 < D ? p[j0 + 3] : 0.f;
    return v;
}

struct SeedCentre {
    float4 v[4];        // lane g of a group of G: elements 4 g + t * 4 G + (0 .. 3)
    __device__ __forceinline__ void load(const float* __restrict__ c, int D, int G, int g) {
        const bool vec = (reinterpret_cast<uintptr_t>(c) & 15u) == 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = seed_load4(c, 4 * g + t * 4 * G, D, vec);
    }
};

// A lane's share of one row, in two steps so that the loads of two rows are in flight before either is used:
// fetch() issues the loads, partial() is this lane's share of dist(s * x, c): its four accumulators, folded (a0 + a1) + (a2 + a3)
struct SeedRow {
    float4 v[4];
    float s;
    __device__ __forceinline__ void fetch(const float* __restrict__ x, float scale, int D, int G, int g) {
        const bool vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
        s = scale;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = seed_load4(x, 4 * g + t * 4 * G, D, vec);
    }
    __device__ __forceinline__ float partial(const SeedCentre& c) const {
        float4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float dx = s * v[t].x - c.v[t].x, dy = s * v[t].y - c.v[t].y, dz = s * v[t].z - c.v[t].z, dw = s * v[t].w - c.v[t].w;
            a.x = a.x + dx * dx;
            a.y = a.y + dy * dy;
            a.z = a.z + dz * dz;
            a.w = a.w + dw * dw;
        }
        return (a.x + a.y) + (a.z + a.w);
    }
};
// the tree over the lanes of a group; every lane of the group ends with the same bits
__device__ __forceinline__ float seed_fold(float v, int G) {
    for (int m = 1; m < G; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    for (int m = kWave / 2; m > 0; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}

// value: per block the largest w_i (* d2_i); sum: per block the sum of the integer masses under the exponent in st
template <bool SUM>
__global__ __launch_bounds__(kBlock) void seed_mass_kernel(const float* __restrict__ w, const float* __restrict__ d2, int64_t N,
                                                           const SeedState* __restrict__ st, float* __restrict__ bmax,
                                                           uint64_t* __restrict__ bsum) {
    __shared__ uint64_t part_s[kBlock / kWave];
    __shared__ float part_m[kBlock / kWave];
    const int E = SUM ? st->E : 0;
    float mx = 0.f;
    uint64_t sum = 0;
    for (int c = 0; c < kSeedChunks; ++c) {
        const int64_t i = (int64_t)blockIdx.x * kSeedRows + c * kBlock + threadIdx.x;
        if (i < N) {
            const float v = seed_value(w, d2, i);
            if (SUM) sum += seed_mass(v, E);
            else mx = fmaxf(mx, v);
        }
    }
    if (SUM) sum = wave_sum_u64(sum);
    else for (int m = kWave / 2; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if (lane_id() == 0) {
        part_s[threadIdx.x / kWave] = sum;
        part_m[threadIdx.x / kWave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (SUM) bsum[blockIdx.x] = (part_s[0] + part_s[1]) + (part_s[2] + part_s[3]);
        else bmax[blockIdx.x] = fmaxf(fmaxf(part_m[0], part_m[1]), fmaxf(part_m[2], part_m[3]));
    }
}

// E = frexp exponent of the largest block maximum (0 for 0)
__global__ __launch_bounds__(kBlock) void seed_exp_kernel(const float* __restrict__ bmax, int64_t nb, SeedState* __restrict__ st) {
    __shared__ float part[kBlock / kWave];
    float mx = 0.f;
    for (int64_t b = threadIdx.x; b < nb; b += kBlock) mx = fmaxf(mx, bmax[b]);
    for (int m = kWave / 2; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if (lane_id() == 0) part[threadIdx.x / kWave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        int e = 0;
        (void)frexpf(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])), &e);
        st->E = e;
    }
}

// inclusive scan over the kSeedPick threads of the pick workgroup; the total is buf[0][kSeedPick - 1] afterwards
__device__ __forceinline__ uint64_t seed_scan(uint64_t v, uint64_t (*buf)[kSeedPick]) {
    const int tid = threadIdx.x;
    int cur = 0;
    __syncthreads();                     // whoever still reads the previous scan
    buf[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < kSeedPick; off <<= 1) {
        uint64_t x = buf[cur][tid];
        if (tid >= off) x += buf[cur][tid - off];
        buf[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    static_assert(kSeedPick == 1024, "ten steps: the result ends in buf[0]");
    return buf[0][tid];
}

__global__ __launch_bounds__(kSeedPick) void seed_pick_kernel(const float* __restrict__ X, const float* __restrict__ w,
                                                              const float* __restrict__ scale, const float* __restrict__ d2, int64_t N,
                                                              int D, int r, uint64_t seed, const uint64_t* __restrict__ bsum, int64_t nb,
                                                              SeedState* __restrict__ st, float* __restrict__ C,
                                                              int32_t* __restrict__ rows) {
    __shared__ uint64_t buf[2][kSeedPick];
    __shared__ int64_t sh_block, sh_row;
    __shared__ uint64_t sh_rem;
    const int tid = threadIdx.x;
    const int done = st->done, E = st->E;
    if (done) {
        if (tid == 0) rows[r] = -1;
        return;
    }
    // every thread sums a run of blocks; the scan of the runs finds the run, a walk of the run finds the block
    const int64_t L = (nb + kSeedPick - 1) / kSeedPick;
    const int64_t lo = (int64_t)tid * L < nb ? (int64_t)tid * L : nb, hi = lo + L < nb ? lo + L : nb;
    if (tid == 0) {
        sh_block = 0;
        sh_row = -1;
        sh_rem = 0;
    }
    uint64_t seg = 0;
    for (int64_t b = lo; b < hi; ++b) seg += bsum[b];
    const uint64_t incl = seed_scan(seg, buf);
    const uint64_t T = buf[0][kSeedPick - 1];
    if (T == 0) {                                       // uniform: no mass left, the call ends here
        if (tid == 0) {
            st->done = 1;
            st->seeded = r;
            rows[r] = -1;
        }
        return;
    }
    const uint64_t t = __umul64hi(seed_rand64(seed, (uint32_t)r), T);         // < T
    uint64_t acc = incl - seg;
    if (seg > 0 && acc <= t && t < incl) {              // exactly one thread
        for (int64_t b = lo; b < hi; ++b) {
            const uint64_t s = bsum[b];
            if (t < acc + s) {
                sh_block = b;
                sh_rem = t - acc;
                break;
            }
            acc += s;
        }
    }
    __syncthreads();
    const int64_t i = sh_block * kSeedRows + tid;
    const uint64_t rem = sh_rem;
    const uint64_t q = tid < kSeedRows && i < N ? seed_mass(seed_value(w, d2, i), E) : 0;
    const uint64_t incl2 = seed_scan(q, buf);
    if (q > 0 && incl2 - q <= rem && rem < incl2) {     // the smallest row whose inclusive prefix exceeds the draw
        sh_row = i;
        rows[r] = (int32_t)i;
    }
    __syncthreads();
    const int64_t row = sh_row;
    if (row < 0) {                                      // the sums and the masses disagree: cannot happen, and must not index X
        if (tid == 0) {
            st->done = 1;
            st->seeded = r;
            rows[r] = -1;
        }
        return;
    }
    const float s = scale ? scale[row] : 1.f;
    for (int j = tid; j < D; j += kSeedPick) C[(int64_t)r * D + j] = s * X[row * D + j];
}

__global__ __launch_bounds__(kBlock) void seed_cc_kernel(const float* __restrict__ C, int D, int G, int r, float* __restrict__ cc,
                                                         const SeedState* __restrict__ st) {
    if (st->done) return;
    const int g = threadIdx.x & (G - 1);
    const int64_t j = (int64_t)blockIdx.x * (kBlock / G) + (int)threadIdx.x / G;
    SeedCentre c;
    c.load(C + (int64_t)r * D, D, G, g);
    SeedRow x;
    x.fetch(C + (j < r ? j : (int64_t)r) * D, 1.f, D, G, g);      // past the last earlier centre: the new one, its result unused
    const float v = seed_fold(x.partial(c), G);
    if (j < r && g == 0) cc[j] = v;
}

// FIRST: round 0, every row takes dist(y_i, C[0]) and id 0, no masses (E is not known yet).  Otherwise round r >= 1.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void seed_row_kernel(const float* __restrict__ X, const float* __restrict__ w,
                                                          const float* __restrict__ scale, int64_t N, int D, int G, int r, int prune,
                                                          const float* __restrict__ C, const float* __restrict__ cc,
                                                          float* __restrict__ d2, int32_t* __restrict__ ids,
                                                          const SeedState* __restrict__ st, uint64_t* __restrict__ bsum,
                                                          uint64_t* __restrict__ beval) {
    __shared__ int list[kBlock / kWave][kWave];          // per wave: the lanes whose rows are evaluated, in lane order
    __shared__ uint64_t part_s[kBlock / kWave];
    __shared__ uint32_t part_e[kBlock / kWave];
    if (st->done) return;
    const int E = st->E;
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    const int g = lane & (G - 1), sub = lane / G, per = kWave / G;       // per: rows a wave evaluates at a time
    SeedCentre c;
    c.load(C + (int64_t)r * D, D, G, g);
    uint64_t msum = 0;
    uint32_t nev = 0;
    for (int ch = 0; ch < kSeedChunks; ++ch) {
        const int64_t base = (int64_t)blockIdx.x * kSeedRows + (wave * kSeedChunks + ch) * kWave;
        if (base >= N) break;                            // the same for the whole wave
        const int64_t i = base + lane;
        const bool valid = i < N;
        float d = 0.f;
        int id = 0;
        if (!FIRST && valid) {
            d = d2[i];
            id = ids[i];
        }
        bool need = valid;
        if (!FIRST && prune && valid) need = !seed_skip(d, cc[id]);
        const uint64_t mask = __ballot(need);
        const int cnt = __popcll(mask);
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        if (need) list[wave][pos] = lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float nd = d;
        // two steps of `per` rows at a time, both steps' loads issued before either is used; a slot past the last row repeats
        // the last row (cnt >= 1 here) and nobody takes its result
        for (int t = 0; t < cnt; t += 2 * per) {
            const int pa = t + sub, pb = pa + per;
            const int64_t ra = base + list[wave][pa < cnt ? pa : cnt - 1], rb = base + list[wave][pb < cnt ? pb : cnt - 1];
            SeedRow a, b;
            a.fetch(X + ra * D, scale ? scale[ra] : 1.f, D, G, g);
            b.fetch(X + rb * D, scale ? scale[rb] : 1.f, D, G, g);
            const float va = seed_fold(a.partial(c), G), vb = seed_fold(b.partial(c), G);
            const int slot = pos - t;                    // where this lane's own row sits in this trip, if it does
            const float ga = __shfl(va, (slot * G) & (kWave - 1)), gb = __shfl(vb, ((slot - per) * G) & (kWave - 1));
            if (need && slot >= 0 && slot < per) nd = ga;
            if (need && slot >= per && slot < 2 * per) nd = gb;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                 // the list is read before the next chunk rewrites it
        if (FIRST) {
            if (valid) {
                d2[i] = nd;
                ids[i] = 0;
            }
        } else {
            if (need && nd < d) {                        // strictly closer: ties stay with the earlier centre
                d = nd;
                d2[i] = nd;
                ids[i] = r;
            }
            if (valid) msum += seed_mass((w ? w[i] : 1.f) * d, E);
            nev += (uint32_t)cnt;
        }
    }
    if (FIRST) return;
    msum = wave_sum_u64(msum);
    if (lane == 0) {
        part_s[wave] = msum;
        part_e[wave] = nev;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = (part_s[0] + part_s[1]) + (part_s[2] + part_s[3]);
        beval[blockIdx.x] += (uint64_t)part_e[0] + part_e[1] + part_e[2] + part_e[3];
    }
}

__global__ __launch_bounds__(kBlock) void seed_stats_kernel(const uint64_t* __restrict__ beval, int64_t nb, int64_t N, int k,
                                                            const SeedState* __restrict__ st, int64_t* __restrict__ stats) {
    __shared__ uint64_t part[kBlock / kWave];
    uint64_t ev = 0;
    for (int64_t b = threadIdx.x; b < nb; b += kBlock) ev += beval[b];
    ev = wave_sum_u64(ev);
    if (lane_id() == 0) part[threadIdx.x / kWave] = ev;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t seeded = st->done ? st->seeded : k;
        const int64_t evaluated = (int64_t)((part[0] + part[1]) + (part[2] + part[3]));
        stats[0] = seeded;
        stats[1] = evaluated;
        stats[2] = seeded > 0 ? N * (seeded - 1) - evaluated : 0;
        stats[3] = 0;
    }
}

}  // namespace
}  // namespace ogs

using namespace ogs;

extern "C" {

size_t ogs_kmeans_wide_seed_rows(void) { return kSeedRows; }

size_t ogs_kmeans_wide_seed_tmp_bytes(int64_t N, int32_t D, int32_t k) {
    return seed_sizes_ok(N, D, k) ? SeedTmp::carve(nullptr, N, k).bytes : 0;
}

int ogs_kmeans_wide_seed(const float* X, const float* w, const float* row_scale, int64_t N, int32_t D, int32_t k, uint64_t seed,
                         int32_t prune, float* C, int32_t* rows, int32_t* ids, float* d2, int64_t* stats, void* tmp, size_t tmp_bytes,
                         void* stream) {
    if (!seed_sizes_ok(N, D, k)) {
        set_error("kmeans_wide_seed: bad sizes (N=%lld D=%d k=%d; N < 2^31, 1 <= D <= %zu, 1 <= k <= %zu)", (long long)N, D, k,
                  ogs_kmeans_wide_max_dim(), ogs_kmeans_wide_max_k());
        return OGS_ERR_INVALID_ARG;
    }
    if (N == 0) return OGS_OK;
    if (!X || !C || !rows) { set_error("kmeans_wide_seed: NULL pointer"); return OGS_ERR_INVALID_ARG; }
    const SeedTmp t = SeedTmp::carve(tmp, N, k);
    if (!tmp || tmp_bytes < t.bytes || (reinterpret_cast<uintptr_t>(tmp) & 15u) != 0) {
        set_error("kmeans_wide_seed: tmp (16-byte aligned) has %zu bytes, %zu needed (ogs_kmeans_wide_seed_tmp_bytes)",
                  tmp ? tmp_bytes : (size_t)0, t.bytes);
        return OGS_ERR_INVALID_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nb = SeedTmp::blocks(N);
    const int G = seed_group(D);
    float* dd = d2 ? d2 : t.d2;
    int32_t* ii = ids ? ids : t.ids;
    const dim3 grid((unsigned)nb), block(kBlock);

    OGS_HIP_CHECK(hipMemsetAsync(tmp, 0, t.head, s));
    // round 0: masses from the weights alone
    OGS_LAUNCH_NAMED("seed_max_kernel", (seed_mass_kernel<false>), grid, block, 0, s, w, (const float*)nullptr, N,
                     (const SeedState*)t.st, t.bmax, t.bsum);
    OGS_LAUNCH(seed_exp_kernel, dim3(1), block, 0, s, (const float*)t.bmax, nb, t.st);
    OGS_LAUNCH_NAMED("seed_sum_kernel", (seed_mass_kernel<true>), grid, block, 0, s, w, (const float*)nullptr, N,
                     (const SeedState*)t.st, t.bmax, t.bsum);
    OGS_LAUNCH(seed_pick_kernel, dim3(1), dim3(kSeedPick), 0, s, X, w, row_scale, (const float*)nullptr, N, D, 0, seed,
               (const uint64_t*)t.bsum, nb, t.st, C, rows);
    OGS_LAUNCH_NAMED("seed_row0_kernel", (seed_row_kernel<true>), grid, block, 0, s, X, w, row_scale, N, D, G, 0, 0, (const float*)C,
                     (const float*)t.cc, dd, ii, (const SeedState*)t.st, t.bsum, t.beval);
    OGS_LAUNCH_CHECK(0, s);
    if (k > 1) {
        // the exponent of every later round, then the masses round 1 draws from
        OGS_LAUNCH_NAMED("seed_max_kernel", (seed_mass_kernel<false>), grid, block, 0, s, w, (const float*)dd, N,
                         (const SeedState*)t.st, t.bmax, t.bsum);
        OGS_LAUNCH(seed_exp_kernel, dim3(1), block, 0, s, (const float*)t.bmax, nb, t.st);
        OGS_LAUNCH_NAMED("seed_sum_kernel", (seed_mass_kernel<true>), grid, block, 0, s, w, (const float*)dd, N,
                         (const SeedState*)t.st, t.bmax, t.bsum);
    }
    for (int r = 1; r < k; ++r) {
        OGS_LAUNCH(seed_pick_kernel, dim3(1), dim3(kSeedPick), 0, s, X, w, row_scale, (const float*)dd, N, D, r, seed,
                   (const uint64_t*)t.bsum, nb, t.st, C, rows);
        if (prune) {
            const unsigned cb = (unsigned)(((int64_t)r * G + kBlock - 1) / kBlock);
            OGS_LAUNCH(seed_cc_kernel, dim3(cb), block, 0, s, (const float*)C, D, G, r, t.cc, (const SeedState*)t.st);
        }
        OGS_LAUNCH_NAMED("seed_row_kernel", (seed_row_kernel<false>), grid, block, 0, s, X, w, row_scale, N, D, G, r, prune,
                         (const float*)C, (const float*)t.cc, dd, ii, (const SeedState*)t.st, t.bsum, t.beval);
    }
    if (stats) OGS_LAUNCH(seed_stats_kernel, dim3(1), block, 0, s, (const uint64_t*)t.beval, nb, N, k, (const SeedState*)t.st, stats);
    OGS_LAUNCH_CHECK(0, s);
    return OGS_OK;
}

}  // extern "C"
