// k-way connectivity refinement (ek_kway_refine, ctx_kway.cpp): the kernels of one
// round.  A translation unit of its own: the code objects of the
// bipartitioner's and the k-way path's kernels are what they were without it.
//
// A round is six launches on one stream, each reading only what the launches
// before it wrote, so nothing waits inside a launch:
//   k_refine_masks   net  -> Lambda(e), U(e): two 256-bit masks, 64 B a net
//   k_refine_gain    node -> key (g, ~id) and target; 0: not a candidate
//   k_refine_winner  net  -> the largest key among its pins
//   k_refine_indep   node -> the independent candidates' keys, appended to a list
//   k_refine_select  part -> the smallest accepted key of the part
//   k_refine_apply   list -> part[], the part sizes, the round's counters
// Everything is integer.  The only atomics are integer adds (counters, list
// positions, part sizes), whose sums do not depend on the order they arrive
// in; the list's ORDER does, but nothing reads it as an order: the accepted
// set of a part is "the keys >= the part's threshold key", and keys are
// unique (they carry the node id).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

constexpr int RF_THREADS = 256, RF_WAVES = RF_THREADS / 64, RF_SHORT = 8;
constexpr int RF_MAX_BLOCKS = 2048;  // 8 workgroups a CU; the node kernels stride beyond

// seen1: parts with >= 1 pin; seen2: parts with >= 2 (no dynamic index: the
// words stay in registers)
struct PinMask {
    u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    __device__ __forceinline__ void set(unsigned p) {
        const u64 bit = 1ull << (p & 63u);
        const unsigned q = p >> 6;
        const u64 x0 = q == 0u ? bit : 0ull, x1 = q == 1u ? bit : 0ull, x2 = q == 2u ? bit : 0ull,
                  x3 = q == 3u ? bit : 0ull;
        b0 |= a0 & x0;
        b1 |= a1 & x1;
        b2 |= a2 & x2;
        b3 |= a3 & x3;
        a0 |= x0;
        a1 |= x1;
        a2 |= x2;
        a3 |= x3;
    }
    // this lane's partial joined with lane ^ o's
    __device__ __forceinline__ void join(int o) {
        const u64 c0 = __shfl_xor(a0, o, 64), c1 = __shfl_xor(a1, o, 64), c2 = __shfl_xor(a2, o, 64),
                  c3 = __shfl_xor(a3, o, 64);
        b0 |= __shfl_xor(b0, o, 64) | (a0 & c0);
        b1 |= __shfl_xor(b1, o, 64) | (a1 & c1);
        b2 |= __shfl_xor(b2, o, 64) | (a2 & c2);
        b3 |= __shfl_xor(b3, o, 64) | (a3 & c3);
        a0 |= c0;
        a1 |= c1;
        a2 |= c2;
        a3 |= c3;
    }
    __device__ __forceinline__ void store(u64* __restrict__ m) const {
        m[0] = a0;
        m[1] = a1;
        m[2] = a2;
        m[3] = a3;
        m[4] = a0 & ~b0;
        m[5] = a1 & ~b1;
        m[6] = a2 & ~b2;
        m[7] = a3 & ~b3;
    }
};

// The nets hold distinct pins (refine_prepare), so a part's second bit means a
// second node.  A net of at most RF_SHORT pins is its thread's; a longer one
// is taken by the whole wave afterwards, as in k_kway_metrics.
__global__ __launch_bounds__(RF_THREADS) void k_refine_masks(int nets, const int64_t* __restrict__ net_ptr,
                                                             const int32_t* __restrict__ pins,
                                                             const uint8_t* __restrict__ part,
                                                             u64* __restrict__ masks) {
    const int l = threadIdx.x & 63;
    const long long e = blockIdx.x * (long long)RF_THREADS + threadIdx.x;
    int64_t p0 = 0, p1 = 0;
    if (e < nets) {
        p0 = net_ptr[e];
        p1 = net_ptr[e + 1];
    }
    const bool is_long = p1 - p0 > RF_SHORT;
    if (e < nets && !is_long) {
        PinMask m;
        for (int64_t p = p0; p < p1; ++p) m.set(part[pins[p]]);
        m.store(masks + 8 * e);
    }
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(p0, src, 64), q1 = __shfl(p1, src, 64);
        PinMask m;
        for (int64_t p = q0 + l; p < q1; p += 64) m.set(part[pins[p]]);
        for (int o = 32; o > 0; o >>= 1) m.join(o);
        if (l == 0) m.store(masks + 8 * (e - l + src));
    }
}

// One wave per node, 64 nodes at a time: lane j loads node base + j's
// incidence range and part, the wave then takes the nodes one after the
// other.  Lane l owns parts l, l + 64, l + 128, l + 192 and adds the bits of
// each incident net's Lambda into four counters; r is counted by every lane
// alike.  The target is the wave maximum of (g, 255 - b) over the eligible
// parts, so ties go to the smaller b.
__global__ __launch_bounds__(RF_THREADS) void k_refine_gain(int n, const int64_t* __restrict__ inc_ptr,
                                                            const int32_t* __restrict__ inc,
                                                            const uint8_t* __restrict__ part,
                                                            const u64* __restrict__ masks,
                                                            const int* __restrict__ sizes, int k, int lmax,
                                                            u64* __restrict__ key, uint8_t* __restrict__ tgt,
                                                            u64* __restrict__ slot) {
    const int l = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)RF_THREADS + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * RF_WAVES;
    bool open[4];  // parts that may receive
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = l + 64 * j;
        open[j] = b < k && sizes[b] < lmax;
    }
    unsigned found = 0;  // this lane's candidates
    for (long long base = wave * 64; base < n; base += waves * 64) {
        const long long v = base + l;
        int64_t i0 = 0, i1 = 0;
        int a = 0;
        if (v < n) {
            i0 = inc_ptr[v];
            i1 = inc_ptr[v + 1];
            a = part[v];
        }
        u64 mykey = 0;
        int mytgt = 0;
        u64 todo = __ballot(i1 > i0);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const int64_t q0 = __shfl(i0, src, 64), q1 = __shfl(i1, src, 64);
            const int pa = __shfl(a, src, 64);
            const int wa = pa >> 6, sa = pa & 63;
            int c0 = 0, c1 = 0, c2 = 0, c3 = 0, r = 0;
            for (int64_t i = q0; i < q1; i += 64) {
                const int mine = i + l < q1 ? inc[i + l] : 0;
                const int cnt = q1 - i < 64 ? int(q1 - i) : 64;
                for (int j = 0; j < cnt; ++j) {
                    const u64* __restrict__ m = masks + 8ll * __shfl(mine, j, 64);
                    c0 += int((m[0] >> l) & 1ull);
                    c1 += int((m[1] >> l) & 1ull);
                    c2 += int((m[2] >> l) & 1ull);
                    c3 += int((m[3] >> l) & 1ull);
                    r += int((m[4 + wa] >> sa) & 1ull);
                }
            }
            const int base_g = r - int(q1 - q0);
            const int c[4] = {c0, c1, c2, c3};
            u64 best = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = l + 64 * j, g = base_g + c[j];
                const u64 x = open[j] && b != pa && g > 0 ? (u64(unsigned(g)) << 8) | u64(255 - b) : 0ull;
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

// win[e] = the largest key among net e's pins (0: no candidate on it).
__global__ __launch_bounds__(RF_THREADS) void k_refine_winner(int nets, const int64_t* __restrict__ net_ptr,
                                                              const int32_t* __restrict__ pins,
                                                              const u64* __restrict__ key, u64* __restrict__ win) {
    const int l = threadIdx.x & 63;
    const long long e = blockIdx.x * (long long)RF_THREADS + threadIdx.x;
    int64_t p0 = 0, p1 = 0;
    if (e < nets) {
        p0 = net_ptr[e];
        p1 = net_ptr[e + 1];
    }
    const bool is_long = p1 - p0 > RF_SHORT;
    if (e < nets && !is_long) {
        u64 w = 0;
        for (int64_t p = p0; p < p1; ++p) {
            const u64 x = key[pins[p]];
            w = x > w ? x : w;
        }
        win[e] = w;
    }
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(p0, src, 64), q1 = __shfl(p1, src, 64);
        u64 w = 0;
        for (int64_t p = q0 + l; p < q1; p += 64) {
            const u64 x = key[pins[p]];
            w = x > w ? x : w;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const u64 x = __shfl_xor(w, o, 64);
            w = x > w ? x : w;
        }
        if (l == 0) win[e - l + src] = w;
    }
}

// A candidate is independent iff every net it is on names it the winner.  64
// nodes a wave at a time; the candidates among them one after the other, the
// lanes striding over the node's nets.  The list position comes from an
// integer counter (slot[1], also the round's independent count).
__global__ __launch_bounds__(RF_THREADS) void k_refine_indep(int n, const int64_t* __restrict__ inc_ptr,
                                                             const int32_t* __restrict__ inc,
                                                             const u64* __restrict__ key,
                                                             const u64* __restrict__ win, u64* __restrict__ list,
                                                             u64* __restrict__ slot) {
    const int l = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)RF_THREADS + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * RF_WAVES;
    for (long long base = wave * 64; base < n; base += waves * 64) {
        const long long v = base + l;
        u64 kv = 0;
        int64_t i0 = 0, i1 = 0;
        if (v < n) kv = key[v];
        if (kv) {
            i0 = inc_ptr[v];
            i1 = inc_ptr[v + 1];
        }
        bool indep = false;
        u64 todo = __ballot(kv != 0ull);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const int64_t q0 = __shfl(i0, src, 64), q1 = __shfl(i1, src, 64);
            const u64 kq = __shfl(kv, src, 64);
            bool lost = false;
            for (int64_t i = q0 + l; i < q1; i += 64) lost |= win[inc[i]] != kq;
            if (__ballot(lost) == 0ull && l == src) indep = true;
        }
        if (indep) list[atomicAdd(&slot[1], 1ull)] = kv;
    }
}

// One workgroup per part b: thr[b] = the smallest key the part accepts.  With
// room for all of its independent candidates that is 1 (every key); otherwise
// the key of rank `room` from the top, found by a radix select over the list,
// eight bits a pass from the top (the histogram adds are integer).  Keys are
// unique, so exactly `room` keys are >= it: the first `room` in (g descending,
// id ascending) order.
__global__ __launch_bounds__(RF_THREADS) void k_refine_select(const u64* __restrict__ list,
                                                              const uint8_t* __restrict__ tgt,
                                                              const int* __restrict__ sizes, int lmax,
                                                              const u64* __restrict__ slot, u64* __restrict__ thr) {
    __shared__ unsigned hist[256];
    __shared__ unsigned red[RF_WAVES];
    const int t = threadIdx.x, b = blockIdx.x;
    const long long m = (long long)slot[1];
    const long long room = (long long)lmax - sizes[b];
    if (room <= 0) {  // (nothing targets a full part)
        if (t == 0) thr[b] = ~0ull;
        return;
    }
    unsigned mine = 0;
    for (long long i = t; i < m; i += RF_THREADS) mine += tgt[~unsigned(list[i])] == b ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((t & 63) == 0) red[t >> 6] = mine;
    __syncthreads();
    const long long have = (long long)red[0] + red[1] + red[2] + red[3];
    if (have <= room) {
        if (t == 0) thr[b] = 1ull;
        return;
    }
    u64 prefix = 0, fixed = 0;
    unsigned want = unsigned(room);  // rank from the top among the keys matching prefix, 1-based
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for (long long i = t; i < m; i += RF_THREADS) {
            const u64 x = list[i];
            if ((x & fixed) == prefix && tgt[~unsigned(x)] == b) atomicAdd(&hist[unsigned(x >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned d = 255;
        for (;; --d) {  // every thread walks the same counts; have > room, so the walk ends
            const unsigned h = hist[d];
            if (h >= want || d == 0) break;
            want -= h;
        }
        prefix |= u64(d) << shift;
        fixed |= 255ull << shift;
        __syncthreads();
    }
    if (t == 0) thr[b] = prefix;
}

// The accepted nodes move; the part sizes follow; slot[2] and slot[3] get the
// round's moves and gain.
__global__ __launch_bounds__(RF_THREADS) void k_refine_apply(const u64* __restrict__ list,
                                                             const uint8_t* __restrict__ tgt,
                                                             const u64* __restrict__ thr, uint8_t* __restrict__ part,
                                                             int* __restrict__ sizes, u64* __restrict__ slot) {
    const long long m = (long long)slot[1];
    unsigned moved = 0;
    u64 gain = 0;
    for (long long i = blockIdx.x * (long long)RF_THREADS + threadIdx.x; i < m; i += (long long)gridDim.x * RF_THREADS) {
        const u64 x = list[i];
        const unsigned v = ~unsigned(x);
        const int b = tgt[v];
        if (x >= thr[b]) {
            atomicSub(&sizes[part[v]], 1);
            atomicAdd(&sizes[b], 1);
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

void refine_round(hipStream_t s, const RefineDev& d, u64* slot) {
    const unsigned net_blocks = unsigned((d.nets + RF_THREADS - 1) / RF_THREADS);
    const long long node_waves = (d.n + 63ll) / 64;
    const unsigned node_blocks = unsigned(std::min<long long>((node_waves + RF_WAVES - 1) / RF_WAVES, RF_MAX_BLOCKS));
    hipLaunchKernelGGL(k_refine_masks, dim3(net_blocks), dim3(RF_THREADS), 0, s, d.nets, d.net_ptr, d.pins, d.part,
                       d.masks);
    hipLaunchKernelGGL(k_refine_gain, dim3(node_blocks), dim3(RF_THREADS), 0, s, d.n, d.inc_ptr, d.inc, d.part, d.masks,
                       d.sizes, d.k, d.lmax, d.key, d.tgt, slot);
    hipLaunchKernelGGL(k_refine_winner, dim3(net_blocks), dim3(RF_THREADS), 0, s, d.nets, d.net_ptr, d.pins, d.key,
                       d.win);
    hipLaunchKernelGGL(k_refine_indep, dim3(node_blocks), dim3(RF_THREADS), 0, s, d.n, d.inc_ptr, d.inc, d.key, d.win,
                       d.list, slot);
    hipLaunchKernelGGL(k_refine_select, dim3(unsigned(d.k)), dim3(RF_THREADS), 0, s, d.list, d.tgt, d.sizes, d.lmax,
                       slot, d.thr);
    hipLaunchKernelGGL(k_refine_apply, dim3(256), dim3(RF_THREADS), 0, s, d.list, d.tgt, d.thr, d.part, d.sizes, slot);
}

// The launches that read no weights, one by one, with refine_round's grids:
// the weighted round (kernels_refine_w.hip) puts its own gain, select and
// apply kernels between them.
unsigned refine_node_blocks(int n) {
    const long long node_waves = (n + 63ll) / 64;
    return unsigned(std::max<long long>(std::min<long long>((node_waves + RF_WAVES - 1) / RF_WAVES, RF_MAX_BLOCKS), 1));
}

void refine_masks(hipStream_t s, int nets, const int64_t* net_ptr, const int32_t* pins, const uint8_t* part, u64* masks) {
    hipLaunchKernelGGL(k_refine_masks, dim3(unsigned((nets + RF_THREADS - 1) / RF_THREADS)), dim3(RF_THREADS), 0, s, nets,
                       net_ptr, pins, part, masks);
}

void refine_winner(hipStream_t s, int nets, const int64_t* net_ptr, const int32_t* pins, const u64* key, u64* win) {
    hipLaunchKernelGGL(k_refine_winner, dim3(unsigned((nets + RF_THREADS - 1) / RF_THREADS)), dim3(RF_THREADS), 0, s, nets,
                       net_ptr, pins, key, win);
}

void refine_indep(hipStream_t s, int n, const int64_t* inc_ptr, const int32_t* inc, const u64* key, const u64* win,
                  u64* list, u64* slot) {
    hipLaunchKernelGGL(k_refine_indep, dim3(refine_node_blocks(n)), dim3(RF_THREADS), 0, s, n, inc_ptr, inc, key, win,
                       list, slot);
}

}  // namespace dev
}  // namespace ek
