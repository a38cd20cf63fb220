// rt_order.hpp -- rt_ray_order / rt_ray_order_device: a coherent order for a batch of arbitrary rays, computed on the device
// (DESIGN.md 4.10).  order[j] is the index of the ray lane j should carry: the STABLE ascending sort of one 32-bit key per ray, so it is
// unique, deterministic and a permutation of 0 .. n-1.  The walks that take an order are k_query_rays_ordered (rt_query.hpp),
// k_multihit_rays_ordered (rt_multihit.hpp) and k_trace_rays_ordered (rt_trace.hpp).
//
// The key (include/rtrace_hip.h states it; rust_tracer_amd.ray_keys restates it in numpy, bit for bit).  Everything is computed in
// double -- an f32 ray converts exactly -- with + - *, comparisons, truncation and powers of two only, so both sides round alike:
//   box     lo[a], hi[a] = min / max of pos[a] over the batch; ext = the largest hi[a] - lo[a]
//   scale   0 when ext == 0 (one origin: every origin bit 0), else 2^(3 - e) with e = max(E - 1022, -1000), E the biased exponent
//           field of ext: ext < 2^e, so every (pos[a] - lo[a]) * scale lies in [0, 8)
//   cell    c[a] = trunc(clamp((pos[a] - lo[a]) * scale, 0, 7)): 3 bits per axis
//   axis    the component of dir with the largest |value| (the lowest one on a tie); sign = that component < 0
//   q[b]    trunc(clamp((dir[(axis + 1 + b) % 3] + 1) * 512, 0, 1023)), b = 0, 1: 10 bits each
//   key     morton3(c[0], c[1], c[2]) << 23 | (2 * axis + sign) << 20 | morton2(q[0], q[1])          (bit i of c[0] at 3i, of q[0] at 2i)
//
// The sort is a least-significant-digit radix sort of (key, index) pairs, four 8-bit digits.  Per pass: k_sort_hist counts the digits of
// each block's contiguous slice into table[digit][block], k_sort_scan (a block per digit) turns the table into exclusive offsets, k_sort_scatter walks the
// slice again 256 keys at a time and ranks equal digits inside a wave with ballots (eight ballots give a lane its peers; its rank is
// the peers below it) and across the four waves through LDS -- equal digits keep their order, which is what makes the passes compose.
// k_ray_keys also counts every digit of every key (four 256-bin histograms of the whole batch): a pass whose digit is the same for all
// keys moves nothing and is skipped (k_sort_plan decides on the device; a camera's rays have no origin bits).  Indices are 32-bit
// (n <= 2^32 - 1), slice bounds 64-bit; at most kSortMaxBlocks slices, so the table is 1 MB whatever n is.
#pragma once
#include "rt_kernels.hpp"

namespace rt {

constexpr unsigned kSortThreads = 256;       // four waves
constexpr unsigned kSortMaxBlocks = 1024;    // slices of a pass
constexpr unsigned kSortTile = 2048;         // the least a slice holds (a multiple of kSortThreads)

// Doubles as unsigned integers of the same order: min / max become atomicMax, whatever order the waves arrive in.
__device__ __forceinline__ unsigned long long order_enc(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double order_dec(unsigned long long e)
{
    return __longlong_as_double((long long)((e >> 63) ? (e & ~(1ull << 63)) : ~e));
}

// enc[a] = max over the batch of ~order_enc(pos[a]) (the minimum), enc[3 + a] = max of order_enc(pos[a]); starts as zeroes.
struct RayBox { unsigned long long enc[6]; };

// skip[p]: pass p's digit is the same for every key; done[p]: passes in front of p that moved data (the pass reads buffer done[p] & 1;
// done[p] == 0: the indices are still 0 .. n-1 and are not read).
struct SortPlan { unsigned skip[4]; unsigned done[4]; };

struct SortArgs {
    unsigned *keys[2];
    unsigned *idx[2];
    unsigned *table;            // [256][n_blocks]
    const unsigned *totals;     // [4][256]: how often each value of each key byte occurs in the batch
    const SortPlan *plan;
    unsigned *order_out;        // where the last pass leaves the indices
    unsigned n, per_block, n_blocks;
};

template <typename T>
__global__ __launch_bounds__(kSortThreads) void k_ray_box(const T *__restrict__ rays, unsigned n, RayBox *box)
{
    unsigned long long m[6] = { 0, 0, 0, 0, 0, 0 };
    const unsigned long long stride = (unsigned long long)gridDim.x * kSortThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSortThreads + threadIdx.x; i < n; i += stride) {
        const T *r = rays + 6 * i;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long e = order_enc((double)r[a]);
            m[a] = ~e > m[a] ? ~e : m[a];
            m[3 + a] = e > m[3 + a] ? e : m[3 + a];
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(m[a], o, 64);
            m[a] = v > m[a] ? v : m[a];
        }
        if ((threadIdx.x & 63u) == 0u) atomicMax(&box->enc[a], m[a]);
    }
}

__device__ __forceinline__ unsigned spread2(unsigned v)      // bit i of a 10-bit value to bit 2i
{
    v &= 0x3FFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

__device__ __forceinline__ unsigned spread3(unsigned v)      // bit i of a 3-bit value to bit 3i
{
    return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4);
}

__device__ __forceinline__ unsigned clamp_trunc(double v, double top)
{
    v = v >= 0.0 ? v : 0.0;              // (also NaN)
    v = v < top ? v : top;
    return (unsigned)v;
}

// The key of the header, from the decoded box.
__device__ __forceinline__ unsigned ray_key(double px, double py, double pz, double dx, double dy, double dz, double lx, double ly, double lz,
                                            double scale)
{
    const unsigned cx = clamp_trunc((px - lx) * scale, 7.0), cy = clamp_trunc((py - ly) * scale, 7.0), cz = clamp_trunc((pz - lz) * scale, 7.0);
    const double ax = dx < 0.0 ? -dx : dx, ay = dy < 0.0 ? -dy : dy, az = dz < 0.0 ? -dz : dz;
    unsigned axis = 0;
    double best = ax;
    if (ay > best) { axis = 1; best = ay; }
    if (az > best) axis = 2;
    const double dom = axis == 0 ? dx : axis == 1 ? dy : dz;
    const double u = axis == 0 ? dy : axis == 1 ? dz : dx, w = axis == 0 ? dz : axis == 1 ? dx : dy;
    const unsigned qu = clamp_trunc((u + 1.0) * 512.0, 1023.0), qw = clamp_trunc((w + 1.0) * 512.0, 1023.0);
    const unsigned code = 2u * axis + (dom < 0.0 ? 1u : 0u);
    return ((spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2)) << 23) | (code << 20) | spread2(qu) | (spread2(qw) << 1);
}

// One key per ray (keys[i]) and, in totals[4][256], how often each value of each of the key's four bytes occurs in the batch.
template <typename T>
__global__ __launch_bounds__(kSortThreads) void k_ray_keys(const T *__restrict__ rays, unsigned n, const RayBox *__restrict__ box,
                                                           unsigned *__restrict__ keys, unsigned *totals)
{
    __shared__ unsigned h[4 * 256];
    for (unsigned k = threadIdx.x; k < 4 * 256; k += kSortThreads) h[k] = 0;
    __syncthreads();
    const double lx = order_dec(~box->enc[0]), ly = order_dec(~box->enc[1]), lz = order_dec(~box->enc[2]);
    const double ex = order_dec(box->enc[3]) - lx, ey = order_dec(box->enc[4]) - ly, ez = order_dec(box->enc[5]) - lz;
    double ext = ex;
    if (ey > ext) ext = ey;
    if (ez > ext) ext = ez;
    int e = (int)(((unsigned long long)__double_as_longlong(ext) >> 52) & 0x7FFull) - 1022;
    if (e < -1000) e = -1000;
    const double scale = ext > 0.0 ? __longlong_as_double((long long)(1023 + 3 - e) << 52) : 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kSortThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSortThreads + threadIdx.x; i < n; i += stride) {
        const T *r = rays + 6 * i;
        const unsigned key = ray_key((double)r[0], (double)r[1], (double)r[2], (double)r[3], (double)r[4], (double)r[5], lx, ly, lz, scale);
        keys[i] = key;
#pragma unroll
        for (unsigned p = 0; p < 4; ++p) atomicAdd(&h[p * 256 + ((key >> (8 * p)) & 255u)], 1u);
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < 4 * 256; k += kSortThreads)
        if (h[k]) atomicAdd(&totals[k], h[k]);
}

// One block of 256 threads: which passes move data.
__global__ __launch_bounds__(kSortThreads) void k_sort_plan(const unsigned *__restrict__ totals, unsigned n, SortPlan *plan)
{
    unsigned done = 0;
    for (unsigned p = 0; p < 4; ++p) {
        const int same = __syncthreads_or(totals[p * 256 + threadIdx.x] == n ? 1 : 0);
        if (threadIdx.x == 0) { plan->skip[p] = same ? 1u : 0u; plan->done[p] = done; }
        done += same ? 0u : 1u;
    }
}

__global__ __launch_bounds__(kSortThreads) void k_sort_hist(SortArgs a, unsigned pass)
{
    if (a.plan->skip[pass]) return;
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned *__restrict__ src = a.keys[a.plan->done[pass] & 1u];
    const unsigned long long begin = (unsigned long long)blockIdx.x * a.per_block;
    const unsigned long long end = begin + a.per_block < a.n ? begin + a.per_block : a.n;
    for (unsigned long long i = begin + threadIdx.x; i < end; i += kSortThreads) atomicAdd(&h[(src[i] >> (8 * pass)) & 255u], 1u);
    __syncthreads();
    a.table[threadIdx.x * a.n_blocks + blockIdx.x] = h[threadIdx.x];
}

// table[digit][block] -> where each slice's keys of each digit go: the exclusive scan of the table in that order.  One block per digit:
// the keys with a smaller digit come first (their number: the batch's digit totals k_ray_keys left), then this digit's keys of the
// slices in front -- a row of at most kSortMaxBlocks counts, four per thread, scanned through LDS.
__global__ __launch_bounds__(kSortThreads) void k_sort_scan(SortArgs a, unsigned pass)
{
    if (a.plan->skip[pass]) return;
    __shared__ unsigned part[kSortThreads];
    const unsigned d = blockIdx.x, t = threadIdx.x;
    part[t] = t < d ? a.totals[pass * 256 + t] : 0u;
    __syncthreads();
    for (unsigned o = kSortThreads / 2; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    const unsigned base = part[0];
    __syncthreads();
    constexpr unsigned kPer = kSortMaxBlocks / kSortThreads;
    unsigned *const row = a.table + d * a.n_blocks;
    unsigned v[kPer], sum = 0;
#pragma unroll
    for (unsigned j = 0; j < kPer; ++j) {
        const unsigned k = t * kPer + j;
        v[j] = k < a.n_blocks ? row[k] : 0u;
        sum += v[j];
    }
    part[t] = sum;
    __syncthreads();
    for (unsigned o = 1; o < kSortThreads; o <<= 1) {
        const unsigned below = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += below;
        __syncthreads();
    }
    unsigned run = base + part[t] - sum;
#pragma unroll
    for (unsigned j = 0; j < kPer; ++j) {
        const unsigned k = t * kPer + j;
        if (k < a.n_blocks) row[k] = run;
        run += v[j];
    }
}

__global__ __launch_bounds__(kSortThreads) void k_sort_scatter(SortArgs a, unsigned pass)
{
    const bool last = pass == 3u;
    const unsigned done = a.plan->done[pass];
    const bool iota = done == 0u;
    const unsigned *__restrict__ src_k = a.keys[done & 1u];
    const unsigned *__restrict__ src_i = a.idx[done & 1u];
    unsigned *__restrict__ dst_k = a.keys[(done + 1u) & 1u];
    unsigned *__restrict__ dst_i = last ? a.order_out : a.idx[(done + 1u) & 1u];
    const unsigned long long begin = (unsigned long long)blockIdx.x * a.per_block;
    const unsigned long long end = begin + a.per_block < a.n ? begin + a.per_block : a.n;
    if (a.plan->skip[pass]) {
        if (last)                                                    // nothing moves: the order is what the passes before left
            for (unsigned long long i = begin + threadIdx.x; i < end; i += kSortThreads) a.order_out[i] = iota ? (unsigned)i : src_i[i];
        return;
    }
    __shared__ unsigned base[256];
    __shared__ unsigned cnt[kSortThreads / 64][256];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    base[threadIdx.x] = a.table[threadIdx.x * a.n_blocks + blockIdx.x];
    for (unsigned long long first = begin; first < end; first += kSortThreads) {          // (block-uniform)
#pragma unroll
        for (unsigned w = 0; w < kSortThreads / 64; ++w) cnt[w][threadIdx.x] = 0;
        __syncthreads();
        const unsigned long long i = first + threadIdx.x;
        const bool valid = i < end;
        const unsigned key = valid ? src_k[i] : 0u;
        const unsigned d = (key >> (8 * pass)) & 255u;
        unsigned long long peers = __ballot(valid);                  // the valid lanes of this wave with the same digit
#pragma unroll
        for (unsigned b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) cnt[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (valid) {
            unsigned pos = base[d] + rank;
            for (unsigned w = 0; w < wave; ++w) pos += cnt[w][d];
            if (pos < a.n) {                                         // (always: the offsets are the scan of this very count)
                dst_i[pos] = iota ? (unsigned)i : src_i[i];
                if (!last) dst_k[pos] = key;
            }
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (unsigned w = 0; w < kSortThreads / 64; ++w) add += cnt[w][threadIdx.x];
        base[threadIdx.x] += add;                                    // (cnt[.][t] is read and zeroed by thread t alone)
    }
}

}  // namespace rt
