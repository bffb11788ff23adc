// The heavy-edge matching of the coarsening (ek_match, ctx_match.cpp): the
// kernels.  A translation unit of its own: the code objects of the
// bipartitioner's, the k-way path's and the refinements' kernels are what
// they were without it.
//
// Before the rounds, once:
//   k_match_scores   net  -> score(e), -1 for a net above max_net
//   k_match_entries  node -> its entry count (the propose kernel's hand-over)
// A round is two launches on one stream, the second reading only what the
// first wrote, so nothing waits inside a launch:
//   k_match_propose  node -> p(u): the greatest (score, then smaller v) entry
//   k_match_accept   node -> mate[] of the mutual proposals, the counters
// After the last round:
//   k_match_leader, the exclusive scan of kernels_build.hip, k_match_cluster
// Everything is integer.  k_match_propose only reads mate[] and
// k_match_accept only writes it, so every proposal sees the state at the
// round's start.  The only atomics are integer adds into the counters, whose
// sums do not depend on the order they arrive in.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

namespace {

constexpr int MT = MATCH_THREADS;

__global__ __launch_bounds__(MT) void k_match_scores(int nets, int max_net, const int64_t* __restrict__ net_ptr,
                                                     const int32_t* __restrict__ cw, long long* __restrict__ score,
                                                     u64* __restrict__ eligible) {
    const long long e = blockIdx.x * (long long)MT + threadIdx.x;
    bool ok = false;
    if (e < nets) {
        const long long size = net_ptr[e + 1] - net_ptr[e];  // >= 2 distinct pins
        ok = size <= max_net;
        score[e] = ok ? ((long long)cw[e] << 20) / (size - 1) : -1ll;
    }
    const u64 b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(eligible, u64(__popcll(b)));
}

__global__ __launch_bounds__(MT) void k_match_entries(int n, const int64_t* __restrict__ inc_ptr,
                                                      const int32_t* __restrict__ inc,
                                                      const int64_t* __restrict__ net_ptr,
                                                      const long long* __restrict__ score,
                                                      int32_t* __restrict__ entries) {
    const long long u = blockIdx.x * (long long)MT + threadIdx.x;
    if (u >= n) return;
    long long c = 0;
    for (int64_t i = inc_ptr[u]; i < inc_ptr[u + 1]; ++i) {
        const int e = inc[i];
        if (score[e] >= 0) c += net_ptr[e + 1] - net_ptr[e] - 1;
    }
    entries[u] = int32_t(c < INT32_MAX ? c : INT32_MAX);
}

// the running best entry of one node: the greatest score, then the smaller v
struct Best {
    long long s = -1;
    int v = -1;
    __device__ __forceinline__ void take(long long os, int ov) {
        if (os > s || (os == s && ov < v)) {
            s = os;
            v = ov;
        }
    }
};

// the entries of u on net e.  A net whose score is below the best so far
// cannot change it and is skipped unread.
__device__ __forceinline__ void walk_net(const MatchDev& d, int e, int u, long long room, Best& b) {
    const long long s = d.score[e];
    if (s < 0 || s < b.s) return;
    const int64_t q1 = d.net_ptr[e + 1];
    for (int64_t q = d.net_ptr[e]; q < q1; ++q) {
        const int v = d.pins[q];
        if (v != u && d.mate[v] < 0 && d.w[v] <= room) b.take(s, v);
    }
}

// A node of at most MATCH_SHORT entries is its thread's; a longer one is
// taken by the whole wave afterwards, the lanes striding over its nets (a net
// is at most max_net pins long), as in k_kway_metrics and k_refine_masks.
__global__ __launch_bounds__(MT) void k_match_propose(MatchDev d) {
    const int l = threadIdx.x & 63;
    const long long u = blockIdx.x * (long long)MT + threadIdx.x;
    int64_t i0 = 0, i1 = 0;
    long long room = -1;
    int cnt = 0;
    if (u < d.n && d.mate[u] < 0) {
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
            const int ov = __shfl_xor(w.v, o, 64);
            if (os >= 0) w.take(os, ov);
        }
        if (l == src) b = w;
    }
    if (u < d.n) d.prop[u] = b.v;
}

// u and p(u) are matched iff p(p(u)) = u; the smaller id of the two commits
// both entries.  slot[0] += the proposers, slot[1] += the pairs.
__global__ __launch_bounds__(MT) void k_match_accept(int n, const int32_t* __restrict__ prop,
                                                     int32_t* __restrict__ mate, u64* __restrict__ slot) {
    const long long u = blockIdx.x * (long long)MT + threadIdx.x;
    const int p = u < n ? prop[u] : -1;
    const bool pair = p > u && prop[p] == int(u);
    if (pair) {
        mate[u] = p;
        mate[p] = int(u);
    }
    const u64 bp = __ballot(p >= 0), bm = __ballot(pair);
    if ((threadIdx.x & 63) == 0 && bp) {
        atomicAdd(&slot[0], u64(__popcll(bp)));
        if (bm) atomicAdd(&slot[1], u64(__popcll(bm)));
    }
}

__global__ __launch_bounds__(MT) void k_match_leader(int n, const int32_t* __restrict__ mate, int* __restrict__ flag) {
    const long long v = blockIdx.x * (long long)MT + threadIdx.x;
    if (v < n) flag[v] = mate[v] < 0 || v < mate[v] ? 1 : 0;
}

__global__ __launch_bounds__(MT) void k_match_cluster(int n, const int32_t* __restrict__ mate,
                                                      const long long* __restrict__ rank,
                                                      int32_t* __restrict__ cluster) {
    const long long v = blockIdx.x * (long long)MT + threadIdx.x;
    if (v >= n) return;
    const int m = mate[v];
    cluster[v] = int32_t(rank[m >= 0 && m < v ? m : v]);
}

unsigned blocks_of(long long count) { return unsigned((count + MT - 1) / MT); }

}  // namespace

void match_prepare(hipStream_t s, const MatchDev& d, u64* eligible) {
    hipLaunchKernelGGL(k_match_scores, dim3(blocks_of(d.nets)), dim3(MT), 0, s, d.nets, d.max_net, d.net_ptr, d.cw,
                       d.score, eligible);
    hipLaunchKernelGGL(k_match_entries, dim3(blocks_of(d.n)), dim3(MT), 0, s, d.n, d.inc_ptr, d.inc, d.net_ptr, d.score,
                       d.entries);
}

void match_round(hipStream_t s, const MatchDev& d, u64* slot) {
    hipLaunchKernelGGL(k_match_propose, dim3(blocks_of(d.n)), dim3(MT), 0, s, d);
    hipLaunchKernelGGL(k_match_accept, dim3(blocks_of(d.n)), dim3(MT), 0, s, d.n, d.prop, d.mate, slot);
}

void match_cluster(hipStream_t s, const MatchDev& d) {
    hipLaunchKernelGGL(k_match_leader, dim3(blocks_of(d.n)), dim3(MT), 0, s, d.n, d.mate, d.flag);
    exclusive_scan(s, d.flag, d.n, d.rank, d.tiles);
    hipLaunchKernelGGL(k_match_cluster, dim3(blocks_of(d.n)), dim3(MT), 0, s, d.n, d.mate, d.rank, d.cluster);
}

}  // namespace dev
}  // namespace ek
