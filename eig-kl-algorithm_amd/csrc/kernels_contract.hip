// The contraction of a hypergraph along a cluster map on the device
// (ek_hgr_contract_device, ctx_contract.cpp; the rule: DESIGN.md §14, §19): the
// kernels.  A translation unit of its own: the code objects of every other
// kernel are what they were without it.
//
//   k_ct_weights  node    -> its weight into its cluster's sum, integer adds
//   k_ct_nodes    cluster -> the coarse node weight; unhit / too heavy: err
//   k_ct_map      net, a wave each -> the distinct clusters of its pins, first
//                 occurrence first, their count, and the low hash_bits bits of
//                 an order-independent 64-bit signature of the set: the key
//   the stable radix sort of kernels_sweep.hip on (key, net id): nets of one
//                 key become one run, ascending by id
//   k_ct_rep      net -> the least net of its run with the SAME SET, compared
//                 pin by pin (the key only says where to look); c(e) is added
//                 to that net's sum; keep[e] = the net is its own class's least
//   the exclusive scan of kernels_build.hip over keep[] and over the kept sizes
//   k_ct_write    kept net, a wave each -> net_ptr, net_w and the pins
//
// Every launch reads only what an earlier launch wrote, so nothing waits inside
// a launch.  Everything is integer; the only atomics are integer adds, whose
// sums do not depend on the order they arrive in, and every other word is
// written by exactly one thread whatever the schedule.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

namespace {

constexpr int CT = CONTRACT_THREADS;
constexpr int CT_WAVES = CT / 64;

__global__ __launch_bounds__(CT) void k_ct_weights(int n, int nc, const int32_t* __restrict__ cluster,
                                                   const int32_t* __restrict__ w, u64* __restrict__ wsum,
                                                   int* __restrict__ hits) {
    const long long v = blockIdx.x * (long long)CT + threadIdx.x;
    if (v >= n) return;
    const int k = cluster[v];
    if (k < 0 || k >= nc) return;  // (the host checked the range before the launch)
    atomicAdd(&wsum[k], u64(w ? w[v] : 1));
    atomicAdd(&hits[k], 1);
}

__global__ __launch_bounds__(CT) void k_ct_nodes(int nc, const u64* __restrict__ wsum, const int* __restrict__ hits,
                                                 int32_t* __restrict__ node_w, int* __restrict__ err) {
    const long long k = blockIdx.x * (long long)CT + threadIdx.x;
    if (k >= nc) return;
    const u64 s = wsum[k];
    if (hits[k] == 0) atomicAdd(&err[0], 1);
    if (s > u64(INT32_MAX)) atomicAdd(&err[1], 1);
    node_w[k] = int32_t(s > u64(INT32_MAX) ? u64(INT32_MAX) : s);
}

// splitmix64's finalizer: the signature is the wrapping sum of it over the set
__device__ __forceinline__ u64 mix64(u64 x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// One wave a net.  The raw pins are taken 64 at a time; lane l's pin is a first
// occurrence iff no earlier pin of the net maps to the same cluster: the lanes
// below it in this step (shuffles), and, from the second step on (a net of more
// than 64 raw pins), the pins of the steps before, each lane walking them (the
// loads are the same address in every lane).  Its place among the distinct pins
// is the distinct pins of the steps before plus the first occurrences below it.
__global__ __launch_bounds__(CT) void k_ct_map(ContractDev d) {
    const int l = threadIdx.x & 63;
    const long long e = blockIdx.x * (long long)CT_WAVES + (threadIdx.x >> 6);
    if (e >= d.nets) return;  // (the whole wave)
    const int64_t p0 = d.net_ptr[e], p1 = d.net_ptr[e + 1];
    const u64 below = (1ull << l) - 1ull;
    long long count = 0;
    u64 sig = 0ull;
    for (int64_t base = p0; base < p1; base += 64) {
        const int64_t p = base + l;
        const bool have = p < p1;
        const int c = have ? d.cluster[d.pins[p]] : -1;
        bool first = have;
        for (int64_t q = p0; q < base && first; ++q)
            if (d.cluster[d.pins[q]] == c) first = false;
        const int m = int(p1 - base < 64 ? p1 - base : 64);
        for (int j = 0; j < m; ++j) {
            const int cj = __shfl(c, j, 64);
            if (j < l && cj == c) first = false;
        }
        const u64 b = __ballot(first);
        if (first) {
            d.dpins[p0 + count + __popcll(b & below)] = c;
            sig += mix64(u64(uint32_t(c)));
        }
        count += __popcll(b);
    }
    for (int o = 32; o > 0; o >>= 1) sig += __shfl_xor(sig, o, 64);
    if (l == 0) {
        d.dsz[e] = int(count);
        d.key[0][e] = d.hash_bits >= 64 ? sig : sig & ((1ull << d.hash_bits) - 1ull);
        d.ids[0][e] = int32_t(e);
    }
}

// the distinct pins of e and f, m each: the same set iff every pin of e is one of f's
__device__ __forceinline__ bool same_set(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int m) {
    for (int i = 0; i < m; ++i) {
        const int x = a[i];
        bool found = false;
        for (int j = 0; j < m && !found; ++j) found = b[j] == x;
        if (!found) return false;
    }
    return true;
}

// Position i of the sorted (key, id) order.  The run of i's key starts at the
// key's lower bound; the nets before i in the run have smaller ids, in ascending
// order, so the first of them with e's set is the least net of e's class.
__global__ __launch_bounds__(CT) void k_ct_rep(ContractDev d, const u64* __restrict__ skey,
                                               const int32_t* __restrict__ sid) {
    const long long i = blockIdx.x * (long long)CT + threadIdx.x;
    if (i >= d.nets) return;
    const int e = sid[i];
    const int m = d.dsz[e];
    if (m < 2) {  // dropped
        d.keep[e] = 0;
        d.ksz[e] = 0;
        return;
    }
    const u64 key = skey[i];
    long long lo = 0, hi = i;  // the first position in [0, i] whose key is not below `key`
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skey[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const int32_t* mine = d.dpins + d.net_ptr[e];
    int rep = e;
    for (long long j = lo; j < i; ++j) {
        const int f = sid[j];
        if (d.dsz[f] == m && same_set(mine, d.dpins + d.net_ptr[f], m)) {
            rep = f;
            break;
        }
    }
    atomicAdd(&d.csum[rep], u64(d.cw ? d.cw[e] : 1));
    d.keep[e] = rep == e ? 1 : 0;
    d.ksz[e] = rep == e ? m : 0;
}

__global__ __launch_bounds__(CT) void k_ct_write(ContractDev d) {
    const int l = threadIdx.x & 63;
    const long long e = blockIdx.x * (long long)CT_WAVES + (threadIdx.x >> 6);
    if (e >= d.nets || !d.keep[e]) return;  // (the whole wave)
    const long long at = d.idx[e], o = d.off[e];
    const int m = d.dsz[e];
    const int32_t* src = d.dpins + d.net_ptr[e];
    for (int j = l; j < m; j += 64) d.out_pins[o + j] = src[j];
    if (l == 0) {
        const u64 c = d.csum[e];
        if (c > u64(INT32_MAX)) atomicAdd(&d.err[2], 1);
        d.out_ptr[at] = o;
        d.out_w[at] = int32_t(c > u64(INT32_MAX) ? u64(INT32_MAX) : c);
    }
}

unsigned blocks_of(long long count, int per) { return unsigned((count + per - 1) / per); }

}  // namespace

void contract_nodes(hipStream_t s, const ContractDev& d) {
    hipLaunchKernelGGL(k_ct_weights, dim3(blocks_of(d.n, CT)), dim3(CT), 0, s, d.n, d.nc, d.cluster, d.w, d.wsum, d.hits);
    hipLaunchKernelGGL(k_ct_nodes, dim3(blocks_of(d.nc, CT)), dim3(CT), 0, s, d.nc, d.wsum, d.hits, d.node_w, d.err);
}

void contract_nets(hipStream_t s, const ContractDev& d) {
    hipLaunchKernelGGL(k_ct_map, dim3(blocks_of(d.nets, CT_WAVES)), dim3(CT), 0, s, d);
    // bytes above the grouping bits are zero in every key: their passes would move nothing
    int cur = 0;
    for (int pass = 0; pass < (d.hash_bits + 7) / 8; ++pass) {
        sweep_sort_pass(s, d.nets, pass, d.key[cur], d.ids[cur], d.key[cur ^ 1], d.ids[cur ^ 1], d.table, d.scan_tmp);
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_ct_rep, dim3(blocks_of(d.nets, CT)), dim3(CT), 0, s, d, d.key[cur], d.ids[cur]);
    exclusive_scan(s, d.keep, d.nets, d.idx, d.tiles);
    exclusive_scan(s, d.ksz, d.nets, d.off, d.tiles);
    hipLaunchKernelGGL(k_ct_write, dim3(blocks_of(d.nets, CT_WAVES)), dim3(CT), 0, s, d);
}

}  // namespace dev
}  // namespace ek
