// The multi-node clustering of the coarsening (ek_cluster, ctx_cluster.cpp;
// DESIGN.md §20): the kernels.  A translation unit of its own: the code
// objects of every other unit's kernels are what they were without it.  The
// nets' scores and the nodes' entry counts are the matching's
// (match_prepare, kernels_match.hip).
//
// Before the rounds, once:
//   k_cluster_init      node -> rep = v, S = w, grown = 0
// A round is six launches and a scan on one stream, each reading only what
// the ones before it wrote, so nothing waits inside a launch:
//   k_cluster_propose   node -> t(u), sigma(u): the greatest (score, then smaller root) entry
//   k_cluster_incoming  node -> in[t(u)] = 1 (the same value from every writer)
//   k_cluster_resolve   node -> mover[u], count[t(u)] += 1
//   exclusive_scan      (kernels_build.hip) count -> off
//   k_cluster_scatter   mover -> seg[off[t(u)] + its place]; the place varies run to run, the segment's set does not
//   k_cluster_accept    mover -> acc[u]: the weight of the segment's members ranked at or before u fits
//   k_cluster_apply     accepted u -> rep[u], S[t(u)] += w(u), grown[]
// After the last round:
//   k_cluster_roots, the exclusive scan, k_cluster_rank
// Everything is integer.  k_cluster_propose reads rep[], S[] and grown[], and
// only k_cluster_apply writes them, so every step sees the state at the
// round's start.  The only atomics are integer adds: the counters, count[],
// the scatter cursor (whose returned place decides where in its segment a
// mover is stored, never whether), and S[].
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

namespace {

constexpr int CT = CLUSTER_THREADS;

__global__ __launch_bounds__(CT) void k_cluster_init(int n, const int32_t* __restrict__ w, int32_t* __restrict__ rep,
                                                     long long* __restrict__ S, int* __restrict__ grown) {
    const long long v = blockIdx.x * (long long)CT + threadIdx.x;
    if (v >= n) return;
    rep[v] = int32_t(v);
    S[v] = w[v];
    grown[v] = 0;
}

// the running best entry of one node: the greatest score, then the smaller root
struct Best {
    long long s = -1;
    int r = -1;
    __device__ __forceinline__ void take(long long os, int orr) {
        if (os > s || (os == s && orr < r)) {
            s = os;
            r = orr;
        }
    }
};

// the entries of u on net e.  A net whose score is below the best so far
// cannot change it and is skipped unread.
__device__ __forceinline__ void walk_net(const ClusterDev& d, int e, int u, long long room, Best& b) {
    const long long s = d.score[e];
    if (s < 0 || s < b.s) return;
    const int64_t q1 = d.net_ptr[e + 1];
    for (int64_t q = d.net_ptr[e]; q < q1; ++q) {
        const int v = d.pins[q];
        if (v == u) continue;
        const int r = d.rep[v];
        if (d.S[r] <= room) b.take(s, r);
    }
}

// A single node of at most MATCH_SHORT entries is its thread's; a longer one
// is taken by the whole wave afterwards, the lanes striding over its nets, as
// in k_match_propose.  The round's per-node scratch is reset here.
__global__ __launch_bounds__(CT) void k_cluster_propose(ClusterDev d) {
    const int l = threadIdx.x & 63;
    const long long u = blockIdx.x * (long long)CT + threadIdx.x;
    int64_t i0 = 0, i1 = 0;
    long long room = -1;
    int cnt = 0;
    if (u < d.n && d.rep[u] == int(u) && !d.grown[u]) {
        cnt = d.entries[u];
        room = d.cap - d.w[u];
        i0 = d.inc_ptr[u];
        i1 = d.inc_ptr[u + 1];
    }
    const bool is_long = cnt > MATCH_SHORT;
    Best b;
    if (cnt > 0 && !is_long)
        for (int64_t i = i0; i < i1; ++i) walk_net(d, d.inc[i], int(u), room, b);
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(i0, src, 64), q1 = __shfl(i1, src, 64);
        const long long qroom = __shfl(room, src, 64);
        const int qu = int(u - l + src);
        Best w;
        for (int64_t i = q0 + l; i < q1; i += 64) walk_net(d, d.inc[i], qu, qroom, w);
        for (int o = 32; o > 0; o >>= 1) {
            const long long os = __shfl_xor(w.s, o, 64);
            const int orr = __shfl_xor(w.r, o, 64);
            if (os >= 0) w.take(os, orr);
        }
        if (l == src) b = w;
    }
    if (u < d.n) {
        d.t[u] = b.r;
        d.sigma[u] = b.s;
        d.in[u] = 0;
        d.mover[u] = 0;
        d.acc[u] = 0;
        d.count[u] = 0;
        d.cursor[u] = 0;
    }
}

// slot[0] += the proposers
__global__ __launch_bounds__(CT) void k_cluster_incoming(int n, const int32_t* __restrict__ t, int* __restrict__ in,
                                                         u64* __restrict__ slot) {
    const long long u = blockIdx.x * (long long)CT + threadIdx.x;
    const int r = u < n ? t[u] : -1;
    if (r >= 0) in[r] = 1;
    const u64 bp = __ballot(r >= 0);
    if ((threadIdx.x & 63) == 0 && bp) atomicAdd(&slot[0], u64(__popcll(bp)));
}

// u moves iff it proposed, nobody proposed to it or it is the larger id of a
// mutual pair, and its target is not the larger id of a mutual pair (a target
// that leaves): t(u), t(t(u)), t(t(t(u))).  slot[1] += the movers.
__global__ __launch_bounds__(CT) void k_cluster_resolve(int n, const int32_t* __restrict__ t, const int* __restrict__ in,
                                                        int* __restrict__ mover, int* __restrict__ count,
                                                        u64* __restrict__ slot) {
    const long long u = blockIdx.x * (long long)CT + threadIdx.x;
    bool mv = false;
    if (u < n) {
        const int r = t[u];
        if (r >= 0) {
            const int tr = t[r];  // -1 when r is not single
            const bool ml_u = tr == int(u) && int(u) > r;
            const bool ml_r = tr >= 0 && r > tr && t[tr] == r;
            mv = (in[u] == 0 || ml_u) && !ml_r;
            if (mv) {
                mover[u] = 1;
                atomicAdd(&count[r], 1);
            }
        }
    }
    const u64 bm = __ballot(mv);
    if ((threadIdx.x & 63) == 0 && bm) atomicAdd(&slot[1], u64(__popcll(bm)));
}

__global__ __launch_bounds__(CT) void k_cluster_scatter(int n, const int32_t* __restrict__ t, const int* __restrict__ mover,
                                                        const long long* __restrict__ off, int* __restrict__ cursor,
                                                        int32_t* __restrict__ seg) {
    const long long u = blockIdx.x * (long long)CT + threadIdx.x;
    if (u >= n || !mover[u]) return;
    const int r = t[u];
    seg[off[r] + atomicAdd(&cursor[r], 1)] = int32_t(u);
}

// x ranks at or before u in their destination's order: sigma descending, then id ascending
__device__ __forceinline__ bool at_or_before(long long sx, int x, long long su, int u) {
    return sx > su || (sx == su && x <= u);
}

// One thread a slot of seg[].  Its mover u is accepted iff the weights of the
// members of u's segment that rank at or before u sum to at most cap - S(r): a
// sum over a set, so the place of the members inside the segment does not
// matter.  A segment of at most CLUSTER_SHORT movers is summed by the thread,
// a longer one by the whole wave afterwards, the lanes striding over it.
__global__ __launch_bounds__(CT) void k_cluster_accept(ClusterDev d, const long long* __restrict__ movers_total) {
    const int l = threadIdx.x & 63;
    const long long p = blockIdx.x * (long long)CT + threadIdx.x;
    const long long total = *movers_total;  // off[n]
    int u = -1, r = -1;
    long long b0 = 0, b1 = 0, su = -1, room = -1;
    if (p < total) {
        u = d.seg[p];
        r = d.t[u];
        b0 = d.off[r];
        b1 = d.off[r + 1];
        su = d.sigma[u];
        room = d.cap - d.S[r];
    }
    const bool is_long = b1 - b0 > CLUSTER_SHORT;
    long long sum = 0;
    if (u >= 0 && !is_long)
        for (long long i = b0; i < b1; ++i) {
            const int x = d.seg[i];
            if (at_or_before(d.sigma[x], x, su, u)) sum += d.w[x];
        }
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const long long q0 = __shfl(b0, src, 64), q1 = __shfl(b1, src, 64), qs = __shfl(su, src, 64);
        const int qu = __shfl(u, src, 64);
        long long part = 0;
        for (long long i = q0 + l; i < q1; i += 64) {
            const int x = d.seg[i];
            if (at_or_before(d.sigma[x], x, qs, qu)) part += d.w[x];
        }
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if (l == src) sum = part;
    }
    if (u >= 0 && sum <= room) d.acc[u] = 1;
}

// slot[2] += the joins
__global__ __launch_bounds__(CT) void k_cluster_apply(ClusterDev d, u64* __restrict__ slot) {
    const long long u = blockIdx.x * (long long)CT + threadIdx.x;
    const bool a = u < d.n && d.acc[u];
    if (a) {
        const int r = d.t[u];
        d.rep[u] = r;
        atomicAdd(reinterpret_cast<u64*>(&d.S[r]), u64(d.w[u]));
        d.grown[u] = 1;
        d.grown[r] = 1;
    }
    const u64 ba = __ballot(a);
    if ((threadIdx.x & 63) == 0 && ba) atomicAdd(&slot[2], u64(__popcll(ba)));
}

__global__ __launch_bounds__(CT) void k_cluster_roots(int n, const int32_t* __restrict__ rep, int* __restrict__ flag) {
    const long long v = blockIdx.x * (long long)CT + threadIdx.x;
    if (v < n) flag[v] = rep[v] == int(v) ? 1 : 0;
}

__global__ __launch_bounds__(CT) void k_cluster_rank(int n, const int32_t* __restrict__ rep,
                                                     const long long* __restrict__ rank, int32_t* __restrict__ cluster) {
    const long long v = blockIdx.x * (long long)CT + threadIdx.x;
    if (v < n) cluster[v] = int32_t(rank[rep[v]]);
}

unsigned blocks_of(long long count) { return unsigned((count + CT - 1) / CT); }

}  // namespace

void cluster_init(hipStream_t s, const ClusterDev& d) {
    hipLaunchKernelGGL(k_cluster_init, dim3(blocks_of(d.n)), dim3(CT), 0, s, d.n, d.w, d.rep, d.S, d.grown);
}

void cluster_round(hipStream_t s, const ClusterDev& d, u64* slot) {
    const dim3 grid(blocks_of(d.n)), block(CT);
    hipLaunchKernelGGL(k_cluster_propose, grid, block, 0, s, d);
    hipLaunchKernelGGL(k_cluster_incoming, grid, block, 0, s, d.n, d.t, d.in, slot);
    hipLaunchKernelGGL(k_cluster_resolve, grid, block, 0, s, d.n, d.t, d.in, d.mover, d.count, slot);
    exclusive_scan(s, d.count, d.n, d.off, d.tiles);
    hipLaunchKernelGGL(k_cluster_scatter, grid, block, 0, s, d.n, d.t, d.mover, d.off, d.cursor, d.seg);
    // a slot of seg[] a thread: at most n movers, the slots past off[n] idle
    hipLaunchKernelGGL(k_cluster_accept, grid, block, 0, s, d, d.off + d.n);
    hipLaunchKernelGGL(k_cluster_apply, grid, block, 0, s, d, slot);
}

void cluster_number(hipStream_t s, const ClusterDev& d) {
    const dim3 grid(blocks_of(d.n)), block(CT);
    hipLaunchKernelGGL(k_cluster_roots, grid, block, 0, s, d.n, d.rep, d.count);
    exclusive_scan(s, d.count, d.n, d.off, d.tiles);
    hipLaunchKernelGGL(k_cluster_rank, grid, block, 0, s, d.n, d.rep, d.off, d.cluster);
}

}  // namespace dev
}  // namespace ek
