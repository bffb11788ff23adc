// Weighted k-way connectivity refinement under per-part weight bounds
// (ek_kway_refine_w, ctx_kway_refine_w.cpp): the kernels of a
// round that read weights.  A translation unit of its own: the code objects of
// every other path's kernels are what they were without it.
//
// A round keeps the shape of kernels_refine.hip's: six launches on one stream,
// each reading only what the launches before it wrote, nothing waiting inside a
// launch:
//   k_refine_masks     net  -> Lambda(e), U(e)                  (kernels_refine.hip)
//   k_refine_w_gain    node -> key (g, ~id) and target, g in units of c(e),
//                              the fit test S(b) + w(v) <= L_b per node
//   k_refine_winner    net  -> the largest key among its pins   (kernels_refine.hip)
//   k_refine_indep     node -> the independent candidates' list (kernels_refine.hip)
//   k_refine_w_select  part -> thr[b]: the first rejected key of the part, + 1
//   k_refine_w_apply   list -> part[], the part weights, the round's counters
// Everything is integer; the only atomics are integer adds (the counters, the
// part weights, the select's LDS histogram of summed weights), whose sums do not
// depend on the order they arrive in.  The accepted set of a part is "the keys
// >= thr[b]": keys are unique (they carry the node id), so the longest prefix
// of the (g descending, id ascending) order that fits is a set of keys above a
// threshold, found without a sort.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

constexpr int RW_THREADS = 256, RW_WAVES = RW_THREADS / 64;

// One wave per node, 64 nodes at a time, as k_refine_gain: lane j loads node
// base + j's incidence range, part and weight, the wave then takes the nodes
// one after the other.  Lane l owns parts l, l + 64, l + 128, l + 192; it adds
// c(e) of each incident net whose Lambda holds its part into four counters, and
// every lane alike adds c(e) into r where U(e) holds the node's own part and
// into D.  The net's weight is loaded with its index (lane i's incidence
// entry) and travels with it through the shuffle.  All of r, D and the
// counters are at most D(v) <= 2^31 - 1 (weights_prepare), and g = (r - D) + c
// in that order stays inside int32.  A part is open for the node iff S(b) +
// w(v) <= L_b, in 64 bits; each lane loads its four S and L once (the round
// reads the weights of its start: k_refine_w_apply runs after every reader).
__global__ __launch_bounds__(RW_THREADS) void k_refine_w_gain(
    int n, const int64_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc, const int32_t* __restrict__ cw,
    const int32_t* __restrict__ w, const uint8_t* __restrict__ part, const u64* __restrict__ masks,
    const long long* __restrict__ S, const long long* __restrict__ L, int k, u64* __restrict__ key,
    uint8_t* __restrict__ tgt, u64* __restrict__ slot) {
    const int l = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)RW_THREADS + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * RW_WAVES;
    long long sb[4], lb[4];  // a part past k: S = 0, L = -1, closed for every weight
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = l + 64 * j;
        sb[j] = b < k ? S[b] : 0ll;
        lb[j] = b < k ? L[b] : -1ll;
    }
    unsigned found = 0;  // this lane's candidates
    for (long long base = wave * 64; base < n; base += waves * 64) {
        const long long v = base + l;
        int64_t i0 = 0, i1 = 0;
        int a = 0, wv = 0;
        if (v < n) {
            i0 = inc_ptr[v];
            i1 = inc_ptr[v + 1];
            a = part[v];
            wv = w[v];
        }
        u64 mykey = 0;
        int mytgt = 0;
        u64 todo = __ballot(i1 > i0);
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
                const u64 x = open && b != pa && g > 0 ? (u64(unsigned(g)) << 8) | u64(255 - b) : 0ull;
                best = x > best ? x : best;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const u64 x = __shfl_xor(best, o, 64);
                best = x > best ? x : best;
            }
            if (l == src && best) {
                mykey = ((best >> 8) << 32) | u64(~unsigned(v));
                mytgt = 255 - int(best & 255ull);
                ++found;
            }
        }
        if (v < n) {
            key[v] = mykey;
            tgt[v] = uint8_t(mytgt);
        }
    }
    for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o, 64);
    if (l == 0 && found) atomicAdd(&slot[0], u64(found));
}

// One workgroup per part b, room = L_b - S(b): thr[b] = the smallest key the
// part accepts.  room < 0: nothing targets the part (the fit test).  The whole
// list of the part weighs at most room: 1, every key.  Otherwise the accepted
// set is the longest prefix of the (g descending, id ascending) order, i.e. of
// the keys descending, whose summed weight is at most room, and thr is its
// first rejected key + 1: a radix descent, eight bits a pass from the top, over
// a 256-bin LDS histogram of the SUMMED WEIGHTS of the keys under the prefix
// fixed so far.  Every thread walks the same bins from 255 down with the
// running sum acc of what is already taken: a bin with acc + h <= room is taken
// whole, the first that does not fit (h > 0, so it holds a key) is the next
// byte.  After the last pass that bin is one key, the first rejected one.
// Keys of weight 0 add nothing: those above the first rejected key lie in bins
// that were taken or above it inside its bin, those below it are below thr.
__global__ __launch_bounds__(RW_THREADS) void k_refine_w_select(const u64* __restrict__ list,
                                                                const uint8_t* __restrict__ tgt,
                                                                const int32_t* __restrict__ w,
                                                                const long long* __restrict__ S,
                                                                const long long* __restrict__ L,
                                                                const u64* __restrict__ slot, u64* __restrict__ thr) {
    __shared__ u64 hist[256];
    __shared__ u64 red[RW_WAVES];
    static_assert(RW_THREADS == 256, "one histogram bin a thread");
    const int t = threadIdx.x, b = blockIdx.x;
    const long long m = (long long)slot[1];
    const long long room_s = L[b] - S[b];
    if (room_s < 0) {
        if (t == 0) thr[b] = ~0ull;
        return;
    }
    const u64 room = u64(room_s);
    u64 mine = 0;
    for (long long i = t; i < m; i += RW_THREADS) {
        const unsigned v = ~unsigned(list[i]);
        mine += tgt[v] == b ? u64(w[v]) : 0ull;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((t & 63) == 0) red[t >> 6] = mine;
    __syncthreads();
    const u64 have = red[0] + red[1] + red[2] + red[3];
    if (have <= room) {
        if (t == 0) thr[b] = 1ull;
        return;
    }
    u64 prefix = 0, fixed = 0, acc = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[t] = 0ull;
        __syncthreads();
        for (long long i = t; i < m; i += RW_THREADS) {
            const u64 x = list[i];
            const unsigned v = ~unsigned(x);
            if ((x & fixed) == prefix && tgt[v] == b) {
                const u64 wv = u64(w[v]);
                if (wv) atomicAdd(&hist[unsigned(x >> shift) & 255u], wv);
            }
        }
        __syncthreads();
        unsigned d = 255;
        for (; d > 0; --d) {  // the bins under the prefix weigh more than room - acc together, so one does not fit
            const u64 h = hist[d];
            if (acc + h > room) break;
            acc += h;
        }
        prefix |= u64(d) << shift;
        fixed |= 255ull << shift;
        __syncthreads();
    }
    if (t == 0) thr[b] = prefix + 1ull;
}

// The accepted nodes move; the part weights follow by 64-bit integer adds (the
// subtraction as the add of the two's complement); slot[2] and slot[3] get the
// round's moves and gain.
__global__ __launch_bounds__(RW_THREADS) void k_refine_w_apply(const u64* __restrict__ list,
                                                               const uint8_t* __restrict__ tgt,
                                                               const int32_t* __restrict__ w,
                                                               const u64* __restrict__ thr, uint8_t* __restrict__ part,
                                                               u64* __restrict__ S, u64* __restrict__ slot) {
    const long long m = (long long)slot[1];
    unsigned moved = 0;
    u64 gain = 0;
    for (long long i = blockIdx.x * (long long)RW_THREADS + threadIdx.x; i < m; i += (long long)gridDim.x * RW_THREADS) {
        const u64 x = list[i];
        const unsigned v = ~unsigned(x);
        const int b = tgt[v];
        if (x >= thr[b]) {
            const u64 wv = u64(w[v]);
            if (wv) {
                atomicAdd(&S[part[v]], 0ull - wv);
                atomicAdd(&S[b], wv);
            }
            part[v] = uint8_t(b);
            ++moved;
            gain += x >> 32;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        moved += __shfl_xor(moved, o, 64);
        gain += __shfl_xor(gain, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && moved) {
        atomicAdd(&slot[2], u64(moved));
        atomicAdd(&slot[3], gain);
    }
}

void refine_w_round(hipStream_t s, const RefineWDev& d, u64* slot) {
    refine_masks(s, d.nets, d.net_ptr, d.pins, d.part, d.masks);
    hipLaunchKernelGGL(k_refine_w_gain, dim3(refine_node_blocks(d.n)), dim3(RW_THREADS), 0, s, d.n, d.inc_ptr, d.inc, d.cw,
                       d.w, d.part, d.masks, d.S, d.L, d.k, d.key, d.tgt, slot);
    refine_winner(s, d.nets, d.net_ptr, d.pins, d.key, d.win);
    refine_indep(s, d.n, d.inc_ptr, d.inc, d.key, d.win, d.list, slot);
    hipLaunchKernelGGL(k_refine_w_select, dim3(unsigned(d.k)), dim3(RW_THREADS), 0, s, d.list, d.tgt, d.w, d.S, d.L, slot,
                       d.thr);
    hipLaunchKernelGGL(k_refine_w_apply, dim3(256), dim3(RW_THREADS), 0, s, d.list, d.tgt, d.w, d.thr, d.part,
                       reinterpret_cast<u64*>(d.S), slot);
}

// The select by itself, with refine_w_round's grid: the Jet iteration
// (kernels_jet.hip) puts it between its own afterburner and apply kernels.
void refine_w_select(hipStream_t s, int k, const u64* list, const uint8_t* tgt, const int32_t* w, const long long* S,
                     const long long* L, const u64* slot, u64* thr) {
    hipLaunchKernelGGL(k_refine_w_select, dim3(unsigned(k)), dim3(RW_THREADS), 0, s, list, tgt, w, S, L, slot, thr);
}

}  // namespace dev
}  // namespace ek
