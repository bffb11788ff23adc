// k-way rebalancing, the second half of the Jet rule (ek_kway_rebalance,
// ctx_kway_rebalance.cpp): the kernels of a round that are its
// own.  A translation unit of its own: the code objects of every other path's
// kernels are what they were without it.
//
// A round is eight launches on one stream, each reading only what the launches
// before it wrote, nothing waiting inside a launch:
//   k_refine_masks     net   -> Lambda(e), U(e)                 (kernels_refine.hip)
//   k_rebal_gain       node  -> key (g + 2^31, ~id) and target of every node of
//                               positive weight in an overweight part that fits
//                               some other part; the keys, appended to list A
//   k_refine_w_select  part  -> thr_a[a] over list A grouped by the node's OWN
//                               part, under the room x(a) - 1: the first key at
//                               which the running weight reaches x(a), + 1
//                                                               (kernels_refine_w.hip)
//   k_rebal_evict      A     -> list B: the keys >= thr_a[a] - 1
//   k_refine_w_select  part  -> thr[b] over list B grouped by target, under the
//                               room L_b - S(b)                 (kernels_refine_w.hip)
//   k_rebal_apply      B     -> part[], the part weights, the round's moves
//   k_rebal_excess     1 wg  -> X and the next round's x(a) - 1
// Everything is integer; the only atomics are integer adds (the counters, the
// part weights, the select's LDS histogram) and the lists' appends by a
// counter.  A list's ORDER depends on the order the waves arrive in, but
// nothing reads it as an order: keys are unique, and both the evicted set of a
// part and the accepted set of a part are "the keys >= a threshold".
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

constexpr int RB_THREADS = 256, RB_WAVES = RB_THREADS / 64;

// k_jet_gain's shape: one wave per node, 64 nodes at a time; lane l owns parts
// l, l + 64, l + 128, l + 192 and adds c(e) of each incident net whose Lambda
// holds its part into four counters, every lane alike adds c(e) into r where
// U(e) holds the node's own part and into D.  All of them are at most D(v) <=
// 2^31 - 1, and g = (r - D) + c in that order stays inside int32.  The wave
// takes a node iff its part is overweight (S(a) > L_a, the weights of the
// round's start) and w(v) > 0; a node on no net is taken too, its counters stay
// 0 and its target is the smallest part that fits.  There is no lock and no
// filter.  The target is the fitting part of greatest g WHATEVER ITS SIGN: the
// lanes' maximum runs over the biased gain g + 2^31, which is at least 1 for
// every g >= -(2^31 - 1), so 0 stands for "fits nowhere".  An overweight part
// fits nothing (S(b) + w > L_b already).  The proposer's key goes to list A at
// the position an integer counter gives (slot[1], also the round's proposers).
__global__ __launch_bounds__(RB_THREADS) void k_rebal_gain(
    int n, const int64_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc, const int32_t* __restrict__ cw,
    const int32_t* __restrict__ w, const uint8_t* __restrict__ part, const u64* __restrict__ masks,
    const long long* __restrict__ S, const long long* __restrict__ L, int k, u64* __restrict__ key,
    uint8_t* __restrict__ tgt, u64* __restrict__ list, u64* __restrict__ slot) {
    const int l = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)RB_THREADS + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * RB_WAVES;
    long long sb[4], lb[4];  // a part past k: S = 0, L = -1, closed for every weight
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = l + 64 * j;
        sb[j] = b < k ? S[b] : 0ll;
        lb[j] = b < k ? L[b] : -1ll;
    }
    for (long long base = wave * 64; base < n; base += waves * 64) {
        const long long v = base + l;
        int64_t i0 = 0, i1 = 0;
        int a = 0, wv = 0;
        bool over = false;
        if (v < n) {
            i0 = inc_ptr[v];
            i1 = inc_ptr[v + 1];
            a = part[v];
            wv = w[v];
            over = S[a] > L[a];
        }
        u64 mykey = 0;
        int mytgt = 0;
        u64 todo = __ballot(over && wv > 0);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const int64_t q0 = __shfl(i0, src, 64), q1 = __shfl(i1, src, 64);
            const int pa = __shfl(a, src, 64);
            const long long pw = __shfl(wv, src, 64);
            const int wa = pa >> 6, sa = pa & 63;
            int c0 = 0, c1 = 0, c2 = 0, c3 = 0, r = 0, dsum = 0;
            for (int64_t i = q0; i < q1; i += 64) {
                const bool have = i + l < q1;
                const int mine = have ? inc[i + l] : 0;
                const int minew = have ? cw[mine] : 0;
                const int cnt = q1 - i < 64 ? int(q1 - i) : 64;
                for (int j = 0; j < cnt; ++j) {
                    const u64* __restrict__ m = masks + 8ll * __shfl(mine, j, 64);
                    const int ce = __shfl(minew, j, 64);
                    c0 += (m[0] >> l) & 1ull ? ce : 0;
                    c1 += (m[1] >> l) & 1ull ? ce : 0;
                    c2 += (m[2] >> l) & 1ull ? ce : 0;
                    c3 += (m[3] >> l) & 1ull ? ce : 0;
                    r += (m[4 + wa] >> sa) & 1ull ? ce : 0;
                    dsum += ce;
                }
            }
            const int base_g = r - dsum;
            const int c[4] = {c0, c1, c2, c3};
            u64 best = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = l + 64 * j, g = base_g + c[j];
                const bool open = sb[j] + pw <= lb[j];
                const u64 x = open && b != pa ? (u64(unsigned(g) + 0x80000000u) << 8) | u64(255 - b) : 0ull;
                best = x > best ? x : best;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const u64 x = __shfl_xor(best, o, 64);
                best = x > best ? x : best;
            }
            if (l == src && best) {
                mykey = ((best >> 8) << 32) | u64(~unsigned(v));
                mytgt = 255 - int(best & 255ull);
            }
        }
        if (v < n) {
            key[v] = mykey;
            tgt[v] = uint8_t(mytgt);
        }
        if (mykey) list[atomicAdd(&slot[1], 1ull)] = mykey;
    }
}

// thr_a[a] is k_refine_w_select's answer under the room x(a) - 1: ~0 for a part
// that is not overweight (none of its nodes is on the list), 1 when all the
// proposers of a together weigh less than x(a) (all are evicted), otherwise the
// first key that does not fit x(a) - 1, + 1.  Every proposer weighs at least 1,
// so that key is the one at which the running weight reaches x(a): it is the
// last evicted one, and E(a) is "the keys >= thr_a[a] - 1".  An evicted key
// goes to list B at the position an integer counter gives (slot[3], also the
// round's evicted).
__global__ __launch_bounds__(RB_THREADS) void k_rebal_evict(const u64* __restrict__ list, const uint8_t* __restrict__ part,
                                                            const u64* __restrict__ thr_a, u64* __restrict__ list_b,
                                                            u64* __restrict__ slot) {
    const long long m = (long long)slot[1];
    for (long long i = blockIdx.x * (long long)RB_THREADS + threadIdx.x; i < m;
         i += (long long)gridDim.x * RB_THREADS) {
        const u64 x = list[i];
        const unsigned v = ~unsigned(x);
        if (x >= thr_a[part[v]] - 1ull) list_b[atomicAdd(&slot[3], 1ull)] = x;
    }
}

// The accepted nodes move; the part weights follow by 64-bit integer adds (the
// subtraction as the add of the two's complement); slot[0] gets the round's
// moves.  Every node of list B weighs at least 1.
__global__ __launch_bounds__(RB_THREADS) void k_rebal_apply(const u64* __restrict__ list_b,
                                                            const uint8_t* __restrict__ tgt,
                                                            const int32_t* __restrict__ w, const u64* __restrict__ thr,
                                                            uint8_t* __restrict__ part, u64* __restrict__ S,
                                                            u64* __restrict__ slot) {
    const long long m = (long long)slot[3];
    unsigned moved = 0;
    for (long long i = blockIdx.x * (long long)RB_THREADS + threadIdx.x; i < m;
         i += (long long)gridDim.x * RB_THREADS) {
        const u64 x = list_b[i];
        const unsigned v = ~unsigned(x);
        const int b = tgt[v];
        if (x >= thr[b]) {
            const u64 wv = u64(w[v]);
            atomicAdd(&S[part[v]], 0ull - wv);
            atomicAdd(&S[b], wv);
            part[v] = uint8_t(b);
            ++moved;
        }
    }
    for (int o = 32; o > 0; o >>= 1) moved += __shfl_xor(moved, o, 64);
    if ((threadIdx.x & 63) == 0 && moved) atomicAdd(&slot[0], u64(moved));
}

// One workgroup, thread p for part p: x(p) = max(0, S(p) - L_p); room[p] = x(p)
// - 1 for an overweight part, -1 elsewhere and past k (the source select's
// room); slot[2] = X, the sum of the x(p).
__global__ __launch_bounds__(RB_THREADS) void k_rebal_excess(int k, const long long* __restrict__ S,
                                                             const long long* __restrict__ L,
                                                             long long* __restrict__ room, u64* __restrict__ slot) {
    __shared__ u64 red[RB_WAVES];
    static_assert(RB_THREADS == 256, "one part a thread");
    const int t = threadIdx.x;
    long long x = 0;
    if (t < k) {
        const long long d = S[t] - L[t];
        x = d > 0 ? d : 0ll;
    }
    room[t] = x - 1ll;
    u64 sum = u64(x);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((t & 63) == 0) red[t >> 6] = sum;
    __syncthreads();
    if (t == 0) slot[2] = red[0] + red[1] + red[2] + red[3];
}

void rebal_excess(hipStream_t s, const RebalDev& d, u64* rec) {
    hipLaunchKernelGGL(k_rebal_excess, dim3(1), dim3(RB_THREADS), 0, s, d.r.k, d.r.S, d.r.L, d.room, rec);
}

void rebal_round(hipStream_t s, const RebalDev& d, u64* rec) {
    const RefineWDev& r = d.r;
    if (r.nets > 0) refine_masks(s, r.nets, r.net_ptr, r.pins, r.part, r.masks);
    hipLaunchKernelGGL(k_rebal_gain, dim3(refine_node_blocks(r.n)), dim3(RB_THREADS), 0, s, r.n, r.inc_ptr, r.inc, r.cw,
                       r.w, r.part, r.masks, r.S, r.L, r.k, r.key, r.tgt, r.list, rec);
    // E(a): list A (rec[1] keys) grouped by the node's own part, under the room x(a) - 1 ("S" = 0, "L" = room)
    refine_w_select(s, r.k, r.list, r.part, r.w, d.zero, d.room, rec, d.thr_a);
    hipLaunchKernelGGL(k_rebal_evict, dim3(256), dim3(RB_THREADS), 0, s, r.list, r.part, d.thr_a, d.list_b, rec);
    // the accepted: list B (rec[3] keys) grouped by target, under the real S and L
    refine_w_select(s, r.k, d.list_b, r.tgt, r.w, r.S, r.L, rec + 2, r.thr);
    hipLaunchKernelGGL(k_rebal_apply, dim3(256), dim3(RB_THREADS), 0, s, d.list_b, r.tgt, r.w, r.thr, r.part,
                       reinterpret_cast<u64*>(r.S), rec);
    rebal_excess(s, d, rec);
}

}  // namespace dev
}  // namespace ek
