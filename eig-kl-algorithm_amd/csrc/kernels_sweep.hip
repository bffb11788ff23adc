// The sweep cuts of a Fiedler vector (ctx_sweep.cpp; the rules: eigkl.h,
// DESIGN.md §10 and §13): a stable radix sort of the nodes by (ord(v), id),
// the net-cut profile of every prefix split, in net counts and in net weights,
// the prefix weight of every split, and the two choices: the best split inside
// the count sweep's balance window, and the weighted sweep's best split among
// those whose two sides weigh at most L_max.  A translation unit of its own:
// the code objects of the bipartitioner's kernels are what they were without
// it.
//
// Nothing here waits inside a launch: every kernel reads only what earlier
// launches on the stream wrote.  Everything is integer work, and no result
// depends on the order workgroups or atomics arrive in: the only atomics are
// integer adds into counters (histograms, the two difference arrays), which
// commute (modulo 2^32 and 2^64), positions inside a tile come from ballots
// and popcounts, and each choice is a reduction under a strict total order.
// Weights and structure are read with plain loads and never written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

// the radix order of the select (rank_key, kernels_kway.hip): sign flipped,
// negatives inverted, so -0 sorts before +0
__device__ __forceinline__ u64 sweep_key(double v) {
    const u64 u = static_cast<u64>(__double_as_longlong(v));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// ---------------------------------------------------------------------------
// Sort: least-significant-digit radix sort of the 64-bit keys, 8 bits a pass,
// the node id as payload.  A tile is SW_TILE consecutive elements, element
// base + u * 256 + t held by thread t as its u-th: the tile's elements in
// index order are (row u, wave, lane) ascending.
constexpr int SW_THREADS = 256, SW_PER = SWEEP_TILE / SW_THREADS, SW_WAVES = SW_THREADS / 64;
constexpr int SW_GROUPS = SW_PER * SW_WAVES;  // (row, wave) groups of 64 consecutive elements
constexpr int SW_DIGITS = 256, SW_PASSES = 8;
static_assert(SWEEP_TILE % SW_THREADS == 0, "a tile is whole rows of the workgroup");

// keys[i] = ord(v[i]), ids[i] = i, and ghist[p * 256 + d] += the keys whose
// digit p is d (ghist zero before the launch): a digit all n keys share marks
// a pass the host skips
__global__ __launch_bounds__(SW_THREADS) void k_sweep_keys(const double* __restrict__ v, int n, u64* __restrict__ keys,
                                                           int32_t* __restrict__ ids, unsigned* __restrict__ ghist) {
    __shared__ unsigned h[SW_PASSES * SW_DIGITS];
    const int t = threadIdx.x;
    for (int j = t; j < SW_PASSES * SW_DIGITS; j += SW_THREADS) h[j] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SWEEP_TILE;
#pragma unroll
    for (int u = 0; u < SW_PER; ++u) {
        const long long i = base + u * SW_THREADS + t;
        if (i < n) {
            const u64 k = sweep_key(v[i]);
            keys[i] = k;
            ids[i] = int32_t(i);
#pragma unroll
            for (int p = 0; p < SW_PASSES; ++p) atomicAdd(&h[p * SW_DIGITS + int((k >> (8 * p)) & 255ull)], 1u);
        }
    }
    __syncthreads();
    for (int j = t; j < SW_PASSES * SW_DIGITS; j += SW_THREADS)
        if (h[j]) atomicAdd(&ghist[j], h[j]);
}

// table[d * ntiles + tile] = the tile's keys whose digit (at `shift`) is d:
// digit-major, so the exclusive scan of the flat table is where each (digit,
// tile) run starts in the output
__global__ __launch_bounds__(SW_THREADS) void k_sweep_hist(const u64* __restrict__ keys, int n, int shift, int ntiles,
                                                           unsigned* __restrict__ table) {
    __shared__ unsigned h[SW_DIGITS];
    const int t = threadIdx.x;
    h[t] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SWEEP_TILE;
#pragma unroll
    for (int u = 0; u < SW_PER; ++u) {
        const long long i = base + u * SW_THREADS + t;
        if (i < n) atomicAdd(&h[int((keys[i] >> shift) & 255ull)], 1u);
    }
    __syncthreads();
    table[size_t(t) * size_t(ntiles) + blockIdx.x] = h[t];
}

// The stable scatter of one pass.  An element's place among the tile's equal
// digits: the lanes before it in its wave that hold the digit (eight ballots
// match the digit's bits, a popcount below the lane), plus the digit's count
// in the (row, wave) groups before its own (cnt, summed per digit in group
// order).  No arrival order anywhere, as in k_rank_place.
__global__ __launch_bounds__(SW_THREADS) void k_sweep_scatter(const u64* __restrict__ keys_in,
                                                              const int32_t* __restrict__ ids_in, int n, int shift,
                                                              int ntiles, const unsigned* __restrict__ table,
                                                              u64* __restrict__ keys_out,
                                                              int32_t* __restrict__ ids_out) {
    __shared__ unsigned cnt[SW_GROUPS][SW_DIGITS];
    __shared__ unsigned start[SW_DIGITS];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    for (int g = 0; g < SW_GROUPS; ++g) cnt[g][t] = 0u;
    start[t] = table[size_t(t) * size_t(ntiles) + blockIdx.x];
    __syncthreads();
    const long long base = (long long)blockIdx.x * SWEEP_TILE;
    const u64 lanes_before = (1ull << l) - 1ull;
    u64 k[SW_PER];
    int32_t id[SW_PER];
    unsigned rk[SW_PER];
    bool valid[SW_PER];
#pragma unroll
    for (int u = 0; u < SW_PER; ++u) {
        const long long i = base + u * SW_THREADS + t;
        valid[u] = i < n;
        k[u] = valid[u] ? keys_in[i] : 0ull;
        id[u] = valid[u] ? ids_in[i] : 0;
        const unsigned d = unsigned((k[u] >> shift) & 255ull);
        // the lanes of this wave that hold a key (past the end: none) with digit d
        const u64 vb = __ballot(valid[u]);
        u64 m = valid[u] ? vb : ~vb;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
        rk[u] = unsigned(__popcll(m & lanes_before));
        if (valid[u] && rk[u] == 0u) cnt[u * SW_WAVES + w][d] = unsigned(__popcll(m));
    }
    __syncthreads();
    {  // thread t: digit t's counts become the counts of the groups before each
        unsigned run = 0u;
        for (int g = 0; g < SW_GROUPS; ++g) {
            const unsigned x = cnt[g][t];
            cnt[g][t] = run;
            run += x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SW_PER; ++u) {
        if (!valid[u]) continue;
        const unsigned d = unsigned((k[u] >> shift) & 255ull);
        const unsigned dest = start[d] + cnt[u * SW_WAVES + w][d] + rk[u];
        if (dest < unsigned(n)) {  // (always, for a table that sums to n)
            keys_out[dest] = k[u];
            ids_out[dest] = id[u];
        }
    }
}

__global__ __launch_bounds__(SW_THREADS) void k_sweep_pos(const int32_t* __restrict__ order, int n,
                                                          int32_t* __restrict__ pos) {
    const long long r = (long long)blockIdx.x * SW_THREADS + threadIdx.x;
    if (r < n) {
        const int32_t v = order[r];
        if (v >= 0 && v < n) pos[v] = int32_t(r);
    }
}

// ---------------------------------------------------------------------------
// Prefix sum of 32- or 64-bit words (sums modulo 2^32 or 2^64: a difference
// array's -1 is all ones), in place, three launches: the sum of every
// SWEEP_SCAN_BLOCK-word block, one workgroup's exclusive scan of those sums,
// then every block scans its words again from its sum's offset.
//
// The scan of the block sums is one workgroup that walks them SC_THREADS at a
// step and carries the running total from step to step, so it has no limit of
// its own: count <= 2^31 - 1 words (n <= 2^31 - 2) are at most 2^20 block
// sums, 4,096 steps.  Up to SC_THREADS block sums (count <= 524,288) it is a
// single step and the carry is never used; from 524,289 words on the carry
// path runs.
constexpr int SC_THREADS = 256, SC_PER = SWEEP_SCAN_BLOCK / SC_THREADS, SC_WAVES = SC_THREADS / 64;
static_assert(SWEEP_SCAN_BLOCK % SC_THREADS == 0, "a block is whole rows of the workgroup");

template <class T>
__device__ __forceinline__ T wave_inclusive(T x, int l) {
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (l >= o) x += y;
    }
    return x;
}

template <class T>
__global__ __launch_bounds__(SC_THREADS) void k_scan_sums(const T* __restrict__ in, long long count,
                                                          T* __restrict__ bsum) {
    __shared__ T ws[SC_WAVES];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * SWEEP_SCAN_BLOCK;
    T s = 0;
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

template <class T>
__global__ __launch_bounds__(SC_THREADS) void k_scan_top(T* __restrict__ bsum, int nb) {
    __shared__ T ws[SC_WAVES];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    T carry = 0;
    for (int c0 = 0; c0 < nb; c0 += SC_THREADS) {
        const int i = c0 + t;
        const T x = i < nb ? bsum[i] : T(0);
        const T inc = wave_inclusive(x, l);
        if (l == 63) ws[w] = inc;
        __syncthreads();
        T before = 0;
        for (int q = 0; q < SC_WAVES; ++q) before += q < w ? ws[q] : T(0);
        if (i < nb) bsum[i] = carry + before + inc - x;
        carry += ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}

// thread t scans the block's words [t * SC_PER, (t + 1) * SC_PER).  mode: an
// int, not zero for the inclusive scan, or Inclusive where no caller wants the
// other (the 64-bit scan): that instantiation loads and selects nothing.
struct Inclusive {};

template <class T, class Mode>
__global__ __launch_bounds__(SC_THREADS) void k_scan_apply(T* __restrict__ data, long long count,
                                                           const T* __restrict__ bsum, Mode mode) {
    __shared__ T ws[SC_WAVES];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const long long first = (long long)blockIdx.x * SWEEP_SCAN_BLOCK + (long long)t * SC_PER;
    T x[SC_PER], s = 0;
#pragma unroll
    for (int u = 0; u < SC_PER; ++u) {
        x[u] = first + u < count ? data[first + u] : T(0);
        s += x[u];
    }
    const T inc = wave_inclusive(s, l);
    if (l == 63) ws[w] = inc;
    __syncthreads();
    T run = bsum[blockIdx.x] + inc - s;
    for (int q = 0; q < SC_WAVES; ++q) run += q < w ? ws[q] : T(0);
#pragma unroll
    for (int u = 0; u < SC_PER; ++u) {
        T out;
        if constexpr (std::is_same_v<Mode, Inclusive>) out = run + x[u];
        else out = mode ? run + x[u] : run;
        run += x[u];
        if (first + u < count) data[first + u] = out;
    }
}

// ---------------------------------------------------------------------------
// Profile: per net the least and greatest rank of its pins, +1 at lo + 1 and
// -1 at hi + 1 of the count difference array (n + 1 words, zero before the
// launch).  Laid out as k_kway_metrics: a thread takes its net when it has at
// most SP_SHORT pins, the wave takes a longer one with a shuffle min / max.
// span_part[block] = the block's nets with lo < hi.
//
// The weighted sweep's instantiation (W = NetWeights) adds +c(e) at lo + 1 and
// -c(e) at hi + 1 of the int64 difference array (two's complement: the sums
// are exact modulo 2^64 and the profile itself is at most the sum of all c(e)
// <= 2^62); cw null: every c(e) is 1.  The count sweep's (W = NoWeights)
// carries no weight at all.
constexpr int SP_THREADS = 256, SP_SHORT = 8;

struct NoWeights {};
struct NetWeights {
    const int32_t* cw;
    u64* diffw;
};

template <class W>
__global__ __launch_bounds__(SP_THREADS) void k_sweep_spans(long long nets, const int64_t* __restrict__ net_ptr,
                                                            const int32_t* __restrict__ pins,
                                                            const int32_t* __restrict__ pos, int n,
                                                            unsigned* __restrict__ diff,
                                                            unsigned* __restrict__ span_part, W wt) {
    constexpr bool WT = std::is_same_v<W, NetWeights>;
    __shared__ unsigned ws[SP_THREADS / 64];
    const int t = threadIdx.x, l = t & 63;
    const long long e = blockIdx.x * (long long)SP_THREADS + t;
    unsigned spans = 0u;  // this thread's nets (lane 0: also the wave's long nets)
    auto emit = [&](int lo, int hi, [[maybe_unused]] u64 c) {
        if (lo < hi && lo >= 0 && hi < n) {  // (ranks lie in [0, n): the bounds hold for any pos[] a sort left)
            if constexpr (WT) {
                atomicAdd(&wt.diffw[lo + 1], c);
                atomicAdd(&wt.diffw[hi + 1], 0ull - c);
            }
            atomicAdd(&diff[lo + 1], 1u);
            atomicAdd(&diff[hi + 1], 0xFFFFFFFFu);
            spans += 1u;
        }
    };
    int64_t p0 = 0, p1 = 0;
    u64 c = 1ull;  // (read by the weighted instantiation only)
    if (e < nets) {
        p0 = net_ptr[e];
        p1 = net_ptr[e + 1];
        if constexpr (WT)
            if (wt.cw) c = u64(wt.cw[e]);
    }
    const bool is_long = p1 - p0 > SP_SHORT;
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
        u64 qc = 1ull;
        if constexpr (WT) qc = __shfl(c, src, 64);
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
__global__ __launch_bounds__(SP_THREADS) void k_sweepw_gather(const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ w, int n,
                                                              u64* __restrict__ pw) {
    const long long r = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (r == 0) pw[0] = 0ull;
    if (r < n) {
        const int32_t v = order[r];
        u64 x = 0ull;
        if (v >= 0 && v < n) x = w ? u64(w[v]) : 1ull;  // (always, for the order a sort left)
        pw[r + 1] = x;
    }
}

// ---------------------------------------------------------------------------
// The two choices: each a reduction of the splits under its rule's order, a
// strict total order (every tie ends in the smaller s), so the order of the
// reduction does not matter.  Per-workgroup partials, then one workgroup,
// which also adds up span_part.
constexpr int SL_THREADS = 256;
constexpr unsigned SL_NONE = 0xFFFFFFFFu;  // no split (s never reaches it: n <= INT32_MAX - 1)

// ---------------------------------------------------------------------------
// The count sweep's choice, over the window s_lo .. s_hi.

// p s (n - s) as two 64-bit words: p < 2^32, q = s (n - s) < 2^62
__device__ __forceinline__ void mul_p_q(unsigned p, u64 q, u64& hi, u64& lo) {
    const u64 a = u64(p) * (q & 0xFFFFFFFFull);  // < 2^64
    const u64 b = u64(p) * (q >> 32);            // < 2^62
    const u64 mid = b + (a >> 32);
    hi = mid >> 32;
    lo = (mid << 32) | (a & 0xFFFFFFFFull);
}

__device__ __forceinline__ bool sweep_better(unsigned pa, unsigned sa, unsigned pb, unsigned sb, unsigned n,
                                             int objective) {
    if (objective == 0) {
        if (pa != pb) return pa < pb;
    } else {  // pa / (sa (n - sa)) < pb / (sb (n - sb)), cross-multiplied
        u64 ah, al, bh, bl;
        mul_p_q(pa, u64(sb) * u64(n - sb), ah, al);
        mul_p_q(pb, u64(sa) * u64(n - sa), bh, bl);
        if (ah != bh) return ah < bh;
        if (al != bl) return al < bl;
    }
    const long long xa = 2ll * sa - n, xb = 2ll * sb - n;
    const long long da = xa < 0 ? -xa : xa, db = xb < 0 ? -xb : xb;
    if (da != db) return da < db;
    return sa < sb;
}

__device__ __forceinline__ void sweep_pick(unsigned& p, unsigned& s, unsigned p2, unsigned s2, unsigned n,
                                           int objective) {
    if (s2 == SL_NONE) return;
    if (s == SL_NONE || sweep_better(p2, s2, p, s, n, objective)) {
        p = p2;
        s = s2;
    }
}

// the workgroup's best in thread 0
__device__ __forceinline__ void sweep_block_best(unsigned& p, unsigned& s, unsigned n, int objective,
                                                 unsigned (*ws)[SL_THREADS / 64]) {
    const int t = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned p2 = __shfl_xor(p, o, 64), s2 = __shfl_xor(s, o, 64);
        sweep_pick(p, s, p2, s2, n, objective);
    }
    if ((t & 63) == 0) {
        ws[0][t >> 6] = p;
        ws[1][t >> 6] = s;
    }
    __syncthreads();
    if (t == 0)
        for (int q = 1; q < SL_THREADS / 64; ++q) sweep_pick(p, s, ws[0][q], ws[1][q], n, objective);
}

// thread t's share of the sum of span_part[0:nspan), the nets with lo < hi
__device__ __forceinline__ u64 span_share(const unsigned* __restrict__ span_part, int nspan, int t) {
    u64 spans = 0ull;
    for (int b = t; b < nspan; b += SL_THREADS) spans += span_part[b];
    return spans;
}

__global__ __launch_bounds__(SL_THREADS) void k_sweep_select(const unsigned* __restrict__ profile, unsigned n,
                                                             unsigned s_lo, unsigned s_hi, int objective,
                                                             unsigned* __restrict__ part) {
    __shared__ unsigned ws[2][SL_THREADS / 64];
    unsigned p = 0u, s = SL_NONE;
    const u64 step = u64(gridDim.x) * SL_THREADS;
    for (u64 c = u64(s_lo) + u64(blockIdx.x) * SL_THREADS + threadIdx.x; c <= u64(s_hi); c += step)
        sweep_pick(p, s, profile[c], unsigned(c), n, objective);
    sweep_block_best(p, s, n, objective, ws);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = p;
        part[2 * blockIdx.x + 1] = s;
    }
}

// rec = {s*, profile[s*], profile[n / 2], the nets with lo < hi}
__global__ __launch_bounds__(SL_THREADS) void k_sweep_finish(const unsigned* __restrict__ part, int nparts,
                                                             const unsigned* __restrict__ profile, unsigned n,
                                                             int objective, const unsigned* __restrict__ span_part,
                                                             int nspan, long long* __restrict__ rec) {
    __shared__ unsigned ws[2][SL_THREADS / 64];
    __shared__ u64 sp[SL_THREADS / 64];
    const int t = threadIdx.x;
    unsigned p = 0u, s = SL_NONE;
    for (int b = t; b < nparts; b += SL_THREADS) sweep_pick(p, s, part[2 * b], part[2 * b + 1], n, objective);
    u64 spans = span_share(span_part, nspan, t);
    for (int o = 32; o > 0; o >>= 1) spans += __shfl_xor(spans, o, 64);
    if ((t & 63) == 0) sp[t >> 6] = spans;
    sweep_block_best(p, s, n, objective, ws);  // (its barrier also publishes sp)
    if (t == 0) {
        rec[0] = s == SL_NONE ? -1ll : (long long)s;
        rec[1] = (long long)p;
        rec[2] = (long long)profile[n / 2u];
        rec[3] = (long long)(sp[0] + sp[1] + sp[2] + sp[3]);
    }
}

// ---------------------------------------------------------------------------
// The weighted sweep's choice: one reduction over the splits s = 1 .. n - 1.
// A split's key is
//   feasible:    (profile_w[s],   D[s], s)
//   infeasible:  (2^63 + D[s],    profile_w[s], s)
// with D[s] = |2 P[s] - W + (L0 - L1)|, the slack difference under the per-side
// bounds (L0, L1) of §16 (feasible: P[s] <= L1 and W - P[s] <= L0); §13's one
// bound is L0 = L1 = L_max, where D[s] = |2 P[s] - W|.  The keys are
// compared lexicographically: a strict total order (every tie ends in s) that
// places every feasible split before every infeasible one (profile_w <= 2^62
// and D <= 2^62 leave bit 63 free: D <= W <= 2^62 under one bound, D <= 2 W <=
// 2^62 under two, whose entries ask W <= 2^61), so the least key is the
// rule's s* whether the window is empty or not, and the reduction's shape does
// not matter.  The same pass carries the least and the greatest feasible s
// (min / max, which commute): s_lo, s_hi, and feasible = there is one.
constexpr int SL_WORDS = 5;  // a partial: k1, k2, s, lo, hi

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
                                                              u64 bound0, u64 bound1, u64* __restrict__ part) {
    __shared__ u64 wk[2][SL_THREADS / 64];
    __shared__ unsigned wu[3][SL_THREADS / 64];
    Pick a{0ull, 0ull, SL_NONE, SL_NONE, 0u};
    const u64 step = u64(gridDim.x) * SL_THREADS;
    for (u64 s = 1ull + u64(blockIdx.x) * SL_THREADS + threadIdx.x; s < u64(n); s += step) {
        const u64 p = prefix[s], c = profw[s];
        // the slack difference |(W - p - L0) - (p - L1)| (§16) as |(2 p + L0) - (W + L1)|: both terms stay below
        // 2^64, and with L0 = L1 = L_max it is §13's |2 p - W|
        const u64 x = 2ull * p + bound0, y = total + bound1, d = x >= y ? x - y : y - x;
        // (p <= W for the prefix a scan left; a greater one would wrap to a side above its bound)
        const bool feasible = p <= bound1 && total - p <= bound0;
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
    u64 spans = span_share(span_part, nspan, t);
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
int sweep_tiles(int n) { return (n + SWEEP_TILE - 1) / SWEEP_TILE; }

size_t sweep_scan_tmp_words(long long count) { return size_t((count + SWEEP_SCAN_BLOCK - 1) / SWEEP_SCAN_BLOCK) + 1; }

template <class T>
void sweep_scan(hipStream_t s, T* data, long long count, bool inclusive, T* tmp) {
    constexpr bool WIDE = std::is_same_v<T, u64>;  // no caller wants the exclusive 64-bit scan: none is compiled
    if (WIDE && !inclusive) fail(EK_EINVAL, "sweep_scan: the 64-bit scan is inclusive only");
    if (count <= 0) return;
    const int nb = int((count + SWEEP_SCAN_BLOCK - 1) / SWEEP_SCAN_BLOCK);
    hipLaunchKernelGGL(k_scan_sums<T>, dim3(nb), dim3(SC_THREADS), 0, s, data, count, tmp);
    hipLaunchKernelGGL(k_scan_top<T>, dim3(1), dim3(SC_THREADS), 0, s, tmp, nb);
    if constexpr (WIDE) {
        hipLaunchKernelGGL((k_scan_apply<T, Inclusive>), dim3(nb), dim3(SC_THREADS), 0, s, data, count, tmp, Inclusive{});
    } else {
        hipLaunchKernelGGL((k_scan_apply<T, int>), dim3(nb), dim3(SC_THREADS), 0, s, data, count, tmp, inclusive ? 1 : 0);
    }
}
template void sweep_scan(hipStream_t, unsigned*, long long, bool, unsigned*);
template void sweep_scan(hipStream_t, u64*, long long, bool, u64*);

void sweep_keys(hipStream_t s, const double* v, int n, u64* keys, int32_t* ids, unsigned* ghist) {
    hipLaunchKernelGGL(k_sweep_keys, dim3(sweep_tiles(n)), dim3(SW_THREADS), 0, s, v, n, keys, ids, ghist);
}

void sweep_sort_pass(hipStream_t s, int n, int pass, const u64* keys_in, const int32_t* ids_in, u64* keys_out,
                     int32_t* ids_out, unsigned* table, unsigned* scan_tmp) {
    const int nt = sweep_tiles(n);
    hipLaunchKernelGGL(k_sweep_hist, dim3(nt), dim3(SW_THREADS), 0, s, keys_in, n, 8 * pass, nt, table);
    sweep_scan(s, table, (long long)SW_DIGITS * nt, false, scan_tmp);
    hipLaunchKernelGGL(k_sweep_scatter, dim3(nt), dim3(SW_THREADS), 0, s, keys_in, ids_in, n, 8 * pass, nt, table,
                       keys_out, ids_out);
}

void sweep_pos(hipStream_t s, const int32_t* order, int n, int32_t* pos) {
    hipLaunchKernelGGL(k_sweep_pos, dim3((n + SW_THREADS - 1) / SW_THREADS), dim3(SW_THREADS), 0, s, order, n, pos);
}

int sweep_span_blocks(int64_t nets) { return int((nets + SP_THREADS - 1) / SP_THREADS); }

void sweep_spans(hipStream_t s, int64_t nets, const int64_t* net_ptr, const int32_t* pins, const int32_t* pos, int n,
                 unsigned* diff, unsigned* span_part, const int32_t* cw, u64* diffw) {
    if (nets <= 0) return;
    const dim3 grid(unsigned(sweep_span_blocks(nets)));
    if (diffw)
        hipLaunchKernelGGL(k_sweep_spans<NetWeights>, grid, dim3(SP_THREADS), 0, s, (long long)nets, net_ptr, pins, pos, n,
                           diff, span_part, NetWeights{cw, diffw});
    else
        hipLaunchKernelGGL(k_sweep_spans<NoWeights>, grid, dim3(SP_THREADS), 0, s, (long long)nets, net_ptr, pins, pos, n,
                           diff, span_part, NoWeights{});
}

void sweepw_gather(hipStream_t s, const int32_t* order, const int32_t* w, int n, u64* pw) {
    hipLaunchKernelGGL(k_sweepw_gather, dim3((n + SP_THREADS - 1) / SP_THREADS), dim3(SP_THREADS), 0, s, order, w, n, pw);
}

int sweep_select_blocks(int64_t window) {
    return int(std::min<int64_t>(SWEEP_SELECT_MAX_BLOCKS, (window + SL_THREADS - 1) / SL_THREADS));
}

void sweep_select(hipStream_t s, const unsigned* profile, int n, int64_t s_lo, int64_t s_hi, int objective,
                  unsigned* part, const unsigned* span_part, int nspan, long long* rec) {
    const int nb = sweep_select_blocks(s_hi - s_lo + 1);
    hipLaunchKernelGGL(k_sweep_select, dim3(nb), dim3(SL_THREADS), 0, s, profile, unsigned(n), unsigned(s_lo),
                       unsigned(s_hi), objective, part);
    hipLaunchKernelGGL(k_sweep_finish, dim3(1), dim3(SL_THREADS), 0, s, part, nb, profile, unsigned(n), objective,
                       span_part, nspan, rec);
}

int sweepw_select_blocks(int n) {
    return int(std::max<int64_t>(1, std::min<int64_t>(SWEEP_SELECT_MAX_BLOCKS, (int64_t(n) - 1 + SL_THREADS - 1) / SL_THREADS)));
}

void sweepw_select(hipStream_t s, const u64* profw, const u64* prefix, const unsigned* profile, int n, u64 total,
                   u64 bound0, u64 bound1, u64* part, const unsigned* span_part, int nspan, long long* rec) {
    const int nb = sweepw_select_blocks(n);
    hipLaunchKernelGGL(k_sweepw_select, dim3(nb), dim3(SL_THREADS), 0, s, profw, prefix, unsigned(n), total, bound0,
                       bound1, part);
    hipLaunchKernelGGL(k_sweepw_finish, dim3(1), dim3(SL_THREADS), 0, s, part, nb, profw, prefix, profile, unsigned(n),
                       span_part, nspan, rec);
}

}  // namespace dev
}  // namespace ek
