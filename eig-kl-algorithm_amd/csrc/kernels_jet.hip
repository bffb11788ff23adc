// Parallel weighted k-way refinement that can leave a local minimum, the Jet
// rule on the connectivity metric (ek_kway_jet, ctx_kway_jet.cpp; DESIGN.md
// §18): the kernels of an iteration that are its own.  A translation unit of
// its own: the code objects of every other path's kernels are what they were
// without it.
//
// An iteration up to its moves is five launches on one stream, each reading
// only what the launches before it wrote, nothing waiting inside a launch:
//   k_refine_masks     net  -> Lambda(e), U(e)                  (kernels_refine.hip)
//   k_jet_gain         node -> key (g + 2^31, ~id) and target of every unlocked
//                              node that has an open part and passes the filter
//   k_jet_after        node -> g' with the better-ranked candidates moved; the
//                              passing candidates' keys, appended to a list
//   k_refine_w_select  part -> thr[b]: the first rejected key of the part, + 1
//                                                               (kernels_refine_w.hip)
//   k_jet_apply        list -> part[], the part weights, the next iteration's
//                              locks, the iteration's moves
// Everything is integer; the only atomics are integer adds (the counters, the
// part weights, the select's LDS histogram) and the list's appends by a
// counter.  The list's ORDER depends on the order the waves arrive in, but
// nothing reads it as an order: keys are unique, and the accepted set of a part
// is "the keys >= thr[b]".
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

constexpr int JET_THREADS = 256, JET_WAVES = JET_THREADS / 64;

// k_refine_w_gain's shape: one wave per node, 64 nodes at a time; lane l owns
// parts l, l + 64, l + 128, l + 192 and adds c(e) of each incident net whose
// Lambda holds its part into four counters, every lane alike adds c(e) into r
// where U(e) holds the node's own part and into D.  All of them are at most
// D(v) <= 2^31 - 1, and g = (r - D) + c in that order stays inside int32.
// Three things differ.  A locked node (it moved in the iteration before) and a
// node on no net propose nothing.  The target is the open part of greatest g
// WHATEVER ITS SIGN: the lanes' maximum runs over the biased gain g + 2^31,
// which is at least 1 for every g >= -(2^31 - 1), so 0 stands for "no open
// part".  The node is a candidate iff g >= 0 or -g den < num (D - r), both
// sides in 64 bits (each factor is below 2^31); its key carries the biased
// gain, so it is never 0 either.
__global__ __launch_bounds__(JET_THREADS) void k_jet_gain(
    int n, const int64_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc, const int32_t* __restrict__ cw,
    const int32_t* __restrict__ w, const uint8_t* __restrict__ part, const uint8_t* __restrict__ lock,
    const u64* __restrict__ masks, const long long* __restrict__ S, const long long* __restrict__ L, int k, int neg_num,
    int neg_den, u64* __restrict__ key, uint8_t* __restrict__ tgt, u64* __restrict__ slot) {
    const int l = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)JET_THREADS + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * JET_WAVES;
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
        bool free = false;
        if (v < n) {
            i0 = inc_ptr[v];
            i1 = inc_ptr[v + 1];
            a = part[v];
            wv = w[v];
            free = lock[v] == 0;
        }
        u64 mykey = 0;
        int mytgt = 0;
        u64 todo = __ballot(i1 > i0 && free);
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
                const unsigned biased = unsigned(best >> 8);
                const long long g = (long long)biased - 0x80000000ll;
                if (g >= 0 || -g * (long long)neg_den < (long long)neg_num * (long long)(dsum - r)) {
                    mykey = (u64(biased) << 32) | u64(~unsigned(v));
                    mytgt = 255 - int(best & 255ull);
                    ++found;
                }
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

// The afterburner.  64 nodes a wave at a time, the candidates among them one
// after the other, one wave each.  The wave walks the candidate's nets (lane i
// loads incidence entry i with the net's weight and pin range, which travel
// through the shuffle); over one net the lanes stride its pins, and a lane reads
// the pin's key and holds it to be where its proposal points when that key is
// greater than the candidate's (a key of 0, no candidate, never is), where it
// is otherwise.  Two ballots a net say whether any other pin is held to be in
// the candidate's own part a and in its target t; g' gains c(e) for a net that
// leaves a and loses c(e) for one that enters t.  g' is a sum of +-c(e) over
// the node's nets, inside [-D, D], so it fits int32.  The pins read are those
// of the candidates' nets: the kernel's work is the sum over the candidates of
// the sizes of their nets.  A passing key (g' >= 0) goes to the list at the
// position an integer counter gives (slot[1], also the iteration's passing
// count).
__global__ __launch_bounds__(JET_THREADS) void k_jet_after(
    int n, const int64_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc, const int64_t* __restrict__ net_ptr,
    const int32_t* __restrict__ pins, const int32_t* __restrict__ cw, const uint8_t* __restrict__ part,
    const u64* __restrict__ key, const uint8_t* __restrict__ tgt, u64* __restrict__ list, u64* __restrict__ slot) {
    const int l = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)JET_THREADS + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * JET_WAVES;
    for (long long base = wave * 64; base < n; base += waves * 64) {
        const long long v = base + l;
        u64 kv = 0;
        int64_t i0 = 0, i1 = 0;
        int a = 0, t = 0;
        if (v < n) kv = key[v];
        if (kv) {
            i0 = inc_ptr[v];
            i1 = inc_ptr[v + 1];
            a = part[v];
            t = tgt[v];
        }
        bool pass = false;
        u64 todo = __ballot(kv != 0ull);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const int64_t q0 = __shfl(i0, src, 64), q1 = __shfl(i1, src, 64);
            const u64 kq = __shfl(kv, src, 64);
            const int qa = __shfl(a, src, 64), qt = __shfl(t, src, 64);
            const int vq = int(base) + src;
            int g2 = 0;
            for (int64_t i = q0; i < q1; i += 64) {
                const bool have = i + l < q1;
                const int mine = have ? inc[i + l] : 0;
                const int minew = have ? cw[mine] : 0;
                const int64_t mine0 = have ? net_ptr[mine] : 0, mine1 = have ? net_ptr[mine + 1] : 0;
                const int cnt = q1 - i < 64 ? int(q1 - i) : 64;
                for (int j = 0; j < cnt; ++j) {
                    const int ce = __shfl(minew, j, 64);
                    const int64_t p0 = __shfl(mine0, j, 64), p1 = __shfl(mine1, j, 64);
                    bool in_a = false, in_t = false;
                    for (int64_t p = p0 + l; p < p1; p += 64) {
                        const int u = pins[p];
                        if (u != vq) {
                            const int pu = key[u] > kq ? tgt[u] : part[u];
                            in_a |= pu == qa;
                            in_t |= pu == qt;
                        }
                    }
                    const bool none_a = __ballot(in_a) == 0ull, none_t = __ballot(in_t) == 0ull;
                    g2 += (none_a ? ce : 0) - (none_t ? ce : 0);
                }
            }
            if (l == src && g2 >= 0) pass = true;
        }
        if (pass) list[atomicAdd(&slot[1], 1ull)] = kv;
    }
}

// The accepted nodes move; the part weights follow by 64-bit integer adds (the
// subtraction as the add of the two's complement); the nodes get their lock of
// the next iteration; slot[2] gets the iteration's moves.
__global__ __launch_bounds__(JET_THREADS) void k_jet_apply(const u64* __restrict__ list, const uint8_t* __restrict__ tgt,
                                                           const int32_t* __restrict__ w, const u64* __restrict__ thr,
                                                           uint8_t* __restrict__ part, u64* __restrict__ S,
                                                           uint8_t* __restrict__ lock_next, u64* __restrict__ slot) {
    const long long m = (long long)slot[1];
    unsigned moved = 0;
    for (long long i = blockIdx.x * (long long)JET_THREADS + threadIdx.x; i < m;
         i += (long long)gridDim.x * JET_THREADS) {
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
            lock_next[v] = 1;
            ++moved;
        }
    }
    for (int o = 32; o > 0; o >>= 1) moved += __shfl_xor(moved, o, 64);
    if ((threadIdx.x & 63) == 0 && moved) atomicAdd(&slot[2], u64(moved));
}

void jet_iteration(hipStream_t s, const JetDev& d, u64* slot) {
    const RefineWDev& r = d.r;
    const unsigned node_blocks = refine_node_blocks(r.n);
    refine_masks(s, r.nets, r.net_ptr, r.pins, r.part, r.masks);
    hipLaunchKernelGGL(k_jet_gain, dim3(node_blocks), dim3(JET_THREADS), 0, s, r.n, r.inc_ptr, r.inc, r.cw, r.w, r.part,
                       d.lock, r.masks, r.S, r.L, r.k, d.neg_num, d.neg_den, r.key, r.tgt, slot);
    hipLaunchKernelGGL(k_jet_after, dim3(node_blocks), dim3(JET_THREADS), 0, s, r.n, r.inc_ptr, r.inc, r.net_ptr, r.pins,
                       r.cw, r.part, r.key, r.tgt, r.list, slot);
    refine_w_select(s, r.k, r.list, r.tgt, r.w, r.S, r.L, slot, r.thr);
    hipLaunchKernelGGL(k_jet_apply, dim3(256), dim3(JET_THREADS), 0, s, r.list, r.tgt, r.w, r.thr, r.part,
                       reinterpret_cast<u64*>(r.S), d.lock_next, slot);
}

}  // namespace dev
}  // namespace ek
