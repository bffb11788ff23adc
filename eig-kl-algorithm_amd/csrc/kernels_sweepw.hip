// The weighted sweep cut of a Fiedler vector (ctx_sweepw.cpp; the rule:
// eigkl.h): the profile in net weights, the prefix weight of
// every split, and the choice of the best split among those whose two sides
// weigh at most L_max.  The sort, pos and the 32-bit scan of the count profile
// are kernels_sweep.hip's, through their launchers; this is a translation unit
// of its own, so that file's code objects are what they were without it.
//
// Nothing here waits inside a launch: every kernel reads only what earlier
// launches on the stream wrote.  Everything is integer work, and no result
// depends on the order workgroups or atomics arrive in: the only atomics are
// integer adds into the two difference arrays, which commute (modulo 2^64 and
// 2^32), and the choice is a reduction under a strict total order.  Weights
// and structure are read with plain loads and never written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

// ---------------------------------------------------------------------------
// Profile: k_sweep_spans' layout (a thread takes its net when it has at most
// WP_SHORT pins, the wave takes a longer one with a shuffle min / max), and per
// net with lo < hi four adds: +c(e) at lo + 1 and -c(e) at hi + 1 of the int64
// difference array (two's complement: the sums are exact modulo 2^64 and the
// profile itself is at most the sum of all c(e) <= 2^62), +1 and -1 into the
// count difference array.  cw null: every c(e) is 1.
constexpr int WP_THREADS = 256, WP_SHORT = 8;

__global__ __launch_bounds__(WP_THREADS) void k_sweepw_spans(long long nets, const int64_t* __restrict__ net_ptr,
                                                             const int32_t* __restrict__ pins,
                                                             const int32_t* __restrict__ cw,
                                                             const int32_t* __restrict__ pos, int n,
                                                             u64* __restrict__ diffw, unsigned* __restrict__ diff,
                                                             unsigned* __restrict__ span_part) {
    __shared__ unsigned ws[WP_THREADS / 64];
    const int t = threadIdx.x, l = t & 63;
    const long long e = blockIdx.x * (long long)WP_THREADS + t;
    unsigned spans = 0u;  // this thread's nets (lane 0: also the wave's long nets)
    auto emit = [&](int lo, int hi, u64 c) {
        if (lo < hi && lo >= 0 && hi < n) {  // (ranks lie in [0, n): the bounds hold for any pos[] a sort left)
            atomicAdd(&diffw[lo + 1], c);
            atomicAdd(&diffw[hi + 1], 0ull - c);
            atomicAdd(&diff[lo + 1], 1u);
            atomicAdd(&diff[hi + 1], 0xFFFFFFFFu);
            spans += 1u;
        }
    };
    int64_t p0 = 0, p1 = 0;
    u64 c = 1ull;
    if (e < nets) {
        p0 = net_ptr[e];
        p1 = net_ptr[e + 1];
        if (cw) c = u64(cw[e]);
    }
    const bool is_long = p1 - p0 > WP_SHORT;
    if (p1 - p0 >= 2 && !is_long) {
        const int r0 = pos[pins[p0]];
        int lo = r0, hi = r0;
        for (int64_t p = p0 + 1; p < p1; p += 4) {
            int r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = p + u < p1 ? pos[pins[p + u]] : r0;  // past the net: the first pin
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                lo = min(lo, r[u]);
                hi = max(hi, r[u]);
            }
        }
        emit(lo, hi, c);
    }
    // the wave's long nets, one after the other (the ballot is wave-uniform)
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(p0, src, 64), q1 = __shfl(p1, src, 64);
        const u64 qc = __shfl(c, src, 64);
        int lo = INT32_MAX, hi = -1;
        for (int64_t p = q0 + l; p < q1; p += 64) {
            const int r = pos[pins[p]];
            lo = min(lo, r);
            hi = max(hi, r);
        }
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        if (l == 0) emit(lo, hi, qc);
    }
    for (int o = 32; o > 0; o >>= 1) spans += __shfl_xor(spans, o, 64);
    if (l == 0) ws[t >> 6] = spans;
    __syncthreads();
    if (t == 0) span_part[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// pw[0] = 0 and pw[r + 1] = w(order[r]): the inclusive scan of pw is P.  w
// null: every w(v) is 1.
__global__ __launch_bounds__(WP_THREADS) void k_sweepw_gather(const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ w, int n,
                                                              u64* __restrict__ pw) {
    const long long r = (long long)blockIdx.x * WP_THREADS + threadIdx.x;
    if (r == 0) pw[0] = 0ull;
    if (r < n) {
        const int32_t v = order[r];
        u64 x = 0ull;
        if (v >= 0 && v < n) x = w ? u64(w[v]) : 1ull;  // (always, for the order a sort left)
        pw[r + 1] = x;
    }
}

// ---------------------------------------------------------------------------
// Inclusive prefix sum of 64-bit words (sums modulo 2^64), in place, three
// launches as the 32-bit scan of kernels_sweep.hip: the sum of every
// SWEEPW_SCAN_BLOCK-word block, one workgroup's exclusive scan of those sums,
// then every block scans its words again from its sum's offset.
//
// The scan of the block sums is one workgroup that walks them SWEEPW_SCAN_TOP
// at a step and carries the running total from step to step, so it has no
// limit of its own: count <= 2^31 - 1 words (n <= 2^31 - 2) are at most 2^20
// block sums, 4,096 steps.  Up to SWEEPW_SCAN_TOP block sums (count <= 524,288)
// it is a single step and the carry is never used; from 524,289 words on the
// carry path runs.
constexpr int SC_THREADS = 256, SC_PER = SWEEPW_SCAN_BLOCK / SC_THREADS, SC_WAVES = SC_THREADS / 64;
static_assert(SWEEPW_SCAN_BLOCK % SC_THREADS == 0, "a block is whole rows of the workgroup");
static_assert(SWEEPW_SCAN_TOP == SC_THREADS, "the top scan takes one block sum a thread a step");

__device__ __forceinline__ u64 wave_inclusive64(u64 x, int l) {
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if (l >= o) x += y;
    }
    return x;
}

__global__ __launch_bounds__(SC_THREADS) void k_scan64_sums(const u64* __restrict__ in, long long count,
                                                            u64* __restrict__ bsum) {
    __shared__ u64 ws[SC_WAVES];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * SWEEPW_SCAN_BLOCK;
    u64 s = 0ull;
#pragma unroll
    for (int u = 0; u < SC_PER; ++u) {
        const long long i = base + u * SC_THREADS + t;
        if (i < count) s += in[i];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((t & 63) == 0) ws[t >> 6] = s;
    __syncthreads();
    if (t == 0) bsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ __launch_bounds__(SC_THREADS) void k_scan64_top(u64* __restrict__ bsum, int nb) {
    __shared__ u64 ws[SC_WAVES];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    u64 carry = 0ull;
    for (int c0 = 0; c0 < nb; c0 += SC_THREADS) {
        const int i = c0 + t;
        const u64 x = i < nb ? bsum[i] : 0ull;
        const u64 inc = wave_inclusive64(x, l);
        if (l == 63) ws[w] = inc;
        __syncthreads();
        u64 before = 0ull;
        for (int q = 0; q < SC_WAVES; ++q) before += q < w ? ws[q] : 0ull;
        if (i < nb) bsum[i] = carry + before + inc - x;
        carry += ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}

// thread t scans the block's words [t * SC_PER, (t + 1) * SC_PER)
__global__ __launch_bounds__(SC_THREADS) void k_scan64_apply(u64* __restrict__ data, long long count,
                                                             const u64* __restrict__ bsum) {
    __shared__ u64 ws[SC_WAVES];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const long long first = (long long)blockIdx.x * SWEEPW_SCAN_BLOCK + (long long)t * SC_PER;
    u64 x[SC_PER], s = 0ull;
#pragma unroll
    for (int u = 0; u < SC_PER; ++u) {
        x[u] = first + u < count ? data[first + u] : 0ull;
        s += x[u];
    }
    const u64 inc = wave_inclusive64(s, l);
    if (l == 63) ws[w] = inc;
    __syncthreads();
    u64 run = bsum[blockIdx.x] + inc - s;
    for (int q = 0; q < SC_WAVES; ++q) run += q < w ? ws[q] : 0ull;
#pragma unroll
    for (int u = 0; u < SC_PER; ++u) {
        run += x[u];
        if (first + u < count) data[first + u] = run;
    }
}

// ---------------------------------------------------------------------------
// Choice: one reduction over the splits s = 1 .. n - 1.  A split's key is
//   feasible:    (profile_w[s],          |2 P[s] - W|, s)
//   infeasible:  (2^63 + |2 P[s] - W|,   profile_w[s], s)
// compared lexicographically: a strict total order (every tie ends in s) that
// places every feasible split before every infeasible one (profile_w <= 2^62
// and |2 P - W| <= W <= 2^62 leave bit 63 free), so the least key is the
// rule's s* whether the window is empty or not, and the reduction's shape does
// not matter.  The same pass carries the least and the greatest feasible s
// (min / max, which commute): s_lo, s_hi, and feasible = there is one.
// Per-workgroup partials, then one workgroup.
constexpr int SL_THREADS = 256;
constexpr unsigned SL_NONE = 0xFFFFFFFFu;  // no split (s never reaches it: n <= INT32_MAX - 1)
constexpr int SL_WORDS = 5;                // a partial: k1, k2, s, lo, hi

struct Pick {
    u64 k1, k2;
    unsigned s;       // SL_NONE: none yet
    unsigned lo, hi;  // the least / greatest feasible split seen (SL_NONE / 0: none)
};

__device__ __forceinline__ void pick_merge(Pick& a, u64 k1, u64 k2, unsigned s, unsigned lo, unsigned hi) {
    if (s != SL_NONE) {
        const bool first = k1 != a.k1 ? k1 < a.k1 : (k2 != a.k2 ? k2 < a.k2 : s < a.s);
        if (a.s == SL_NONE || first) {
            a.k1 = k1;
            a.k2 = k2;
            a.s = s;
        }
    }
    a.lo = min(a.lo, lo);
    a.hi = max(a.hi, hi);
}

// the workgroup's pick in thread 0
__device__ __forceinline__ void pick_block(Pick& a, u64 (*wk)[SL_THREADS / 64], unsigned (*wu)[SL_THREADS / 64]) {
    const int t = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
        const u64 k1 = __shfl_xor(a.k1, o, 64), k2 = __shfl_xor(a.k2, o, 64);
        const unsigned s = __shfl_xor(a.s, o, 64), lo = __shfl_xor(a.lo, o, 64), hi = __shfl_xor(a.hi, o, 64);
        pick_merge(a, k1, k2, s, lo, hi);
    }
    if ((t & 63) == 0) {
        wk[0][t >> 6] = a.k1;
        wk[1][t >> 6] = a.k2;
        wu[0][t >> 6] = a.s;
        wu[1][t >> 6] = a.lo;
        wu[2][t >> 6] = a.hi;
    }
    __syncthreads();
    if (t == 0)
        for (int q = 1; q < SL_THREADS / 64; ++q) pick_merge(a, wk[0][q], wk[1][q], wu[0][q], wu[1][q], wu[2][q]);
}

__global__ __launch_bounds__(SL_THREADS) void k_sweepw_select(const u64* __restrict__ profw,
                                                              const u64* __restrict__ prefix, unsigned n, u64 total,
                                                              u64 max_part, u64* __restrict__ part) {
    __shared__ u64 wk[2][SL_THREADS / 64];
    __shared__ unsigned wu[3][SL_THREADS / 64];
    Pick a{0ull, 0ull, SL_NONE, SL_NONE, 0u};
    const u64 step = u64(gridDim.x) * SL_THREADS;
    for (u64 s = 1ull + u64(blockIdx.x) * SL_THREADS + threadIdx.x; s < u64(n); s += step) {
        const u64 p = prefix[s], c = profw[s];
        const u64 twice = 2ull * p, d = twice >= total ? twice - total : total - twice;
        // (p <= W for the prefix a scan left; a greater one would wrap to a side above L_max)
        const bool feasible = p <= max_part && total - p <= max_part;
        pick_merge(a, feasible ? c : (1ull << 63) | d, feasible ? d : c, unsigned(s), feasible ? unsigned(s) : SL_NONE,
                   feasible ? unsigned(s) : 0u);
    }
    pick_block(a, wk, wu);
    if (threadIdx.x == 0) {
        u64* out = part + size_t(SL_WORDS) * blockIdx.x;
        out[0] = a.k1;
        out[1] = a.k2;
        out[2] = a.s;
        out[3] = a.lo;
        out[4] = a.hi;
    }
}

// rec = {s*, feasible, s_lo, s_hi, profile_w[s*], profile[s*], profile_w[n / 2],
//        the nets with lo < hi, P[s*], P[n]}
__global__ __launch_bounds__(SL_THREADS) void k_sweepw_finish(const u64* __restrict__ part, int nparts,
                                                              const u64* __restrict__ profw,
                                                              const u64* __restrict__ prefix,
                                                              const unsigned* __restrict__ profile, unsigned n,
                                                              const unsigned* __restrict__ span_part, int nspan,
                                                              long long* __restrict__ rec) {
    __shared__ u64 wk[2][SL_THREADS / 64];
    __shared__ unsigned wu[3][SL_THREADS / 64];
    __shared__ u64 sp[SL_THREADS / 64];
    const int t = threadIdx.x;
    Pick a{0ull, 0ull, SL_NONE, SL_NONE, 0u};
    for (int b = t; b < nparts; b += SL_THREADS) {
        const u64* in = part + size_t(SL_WORDS) * b;
        pick_merge(a, in[0], in[1], unsigned(in[2]), unsigned(in[3]), unsigned(in[4]));
    }
    u64 spans = 0ull;
    for (int b = t; b < nspan; b += SL_THREADS) spans += span_part[b];
    for (int o = 32; o > 0; o >>= 1) spans += __shfl_xor(spans, o, 64);
    if ((t & 63) == 0) sp[t >> 6] = spans;
    pick_block(a, wk, wu);  // (its barrier also publishes sp)
    if (t == 0) {
        const bool any = a.s != SL_NONE, feasible = a.lo != SL_NONE;
        rec[0] = any ? (long long)a.s : -1ll;
        rec[1] = feasible ? 1ll : 0ll;
        rec[2] = feasible ? (long long)a.lo : 0ll;
        rec[3] = feasible ? (long long)a.hi : 0ll;
        rec[4] = any ? (long long)profw[a.s] : 0ll;
        rec[5] = any ? (long long)profile[a.s] : 0ll;
        rec[6] = (long long)profw[n / 2u];
        rec[7] = (long long)(sp[0] + sp[1] + sp[2] + sp[3]);
        rec[8] = any ? (long long)prefix[a.s] : 0ll;
        rec[9] = (long long)prefix[n];
    }
}
static_assert(SWEEPW_REC == 10, "the record k_sweepw_finish writes");

// ---------------------------------------------------------------------------
// launchers
void sweepw_spans(hipStream_t s, int64_t nets, const int64_t* net_ptr, const int32_t* pins, const int32_t* cw,
                  const int32_t* pos, int n, u64* diffw, unsigned* diff, unsigned* span_part) {
    if (nets <= 0) return;
    hipLaunchKernelGGL(k_sweepw_spans, dim3(unsigned((nets + WP_THREADS - 1) / WP_THREADS)), dim3(WP_THREADS), 0, s,
                       (long long)nets, net_ptr, pins, cw, pos, n, diffw, diff, span_part);
}

void sweepw_gather(hipStream_t s, const int32_t* order, const int32_t* w, int n, u64* pw) {
    hipLaunchKernelGGL(k_sweepw_gather, dim3((n + WP_THREADS - 1) / WP_THREADS), dim3(WP_THREADS), 0, s, order, w, n, pw);
}

size_t sweepw_scan_tmp_words(long long count) { return size_t((count + SWEEPW_SCAN_BLOCK - 1) / SWEEPW_SCAN_BLOCK) + 1; }

void sweepw_scan(hipStream_t s, u64* data, long long count, u64* tmp) {
    if (count <= 0) return;
    const int nb = int((count + SWEEPW_SCAN_BLOCK - 1) / SWEEPW_SCAN_BLOCK);
    hipLaunchKernelGGL(k_scan64_sums, dim3(nb), dim3(SC_THREADS), 0, s, data, count, tmp);
    hipLaunchKernelGGL(k_scan64_top, dim3(1), dim3(SC_THREADS), 0, s, tmp, nb);
    hipLaunchKernelGGL(k_scan64_apply, dim3(nb), dim3(SC_THREADS), 0, s, data, count, tmp);
}

int sweepw_select_blocks(int n) {
    return int(std::max<int64_t>(1, std::min<int64_t>(SWEEP_SELECT_MAX_BLOCKS, (int64_t(n) - 1 + SL_THREADS - 1) / SL_THREADS)));
}

void sweepw_select(hipStream_t s, const u64* profw, const u64* prefix, const unsigned* profile, int n, u64 total,
                   u64 max_part, u64* part, const unsigned* span_part, int nspan, long long* rec) {
    const int nb = sweepw_select_blocks(n);
    hipLaunchKernelGGL(k_sweepw_select, dim3(nb), dim3(SL_THREADS), 0, s, profw, prefix, unsigned(n), total, max_part,
                       part);
    hipLaunchKernelGGL(k_sweepw_finish, dim3(1), dim3(SL_THREADS), 0, s, part, nb, profw, prefix, profile, unsigned(n),
                       span_part, nspan, rec);
}

}  // namespace dev
}  // namespace ek
