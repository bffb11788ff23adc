// Fiduccia-Mattheyses refinement of a bipartition on the integer net cut
// (ctx_fm.cpp; the rules: eigkl.h).  A translation
// unit of its own: the code objects of the bipartitioner's kernels are what
// they were without it.
//
// Every kernel is a template over its argument struct: FmDev is the
// unweighted rule, FmwDev (WT below) the weighted one, which differs where an
// `if constexpr (WT)` says so: c(e) in place of 1 in the gains and the cut,
// w(top) in the fit test, 64-bit side weights, L_max and d, a second sum in
// the counts, the sides' weights in the rollback.  The weights (cw, w) and the
// structure are never written on the device and are read with plain loads; the
// unweighted instantiation reads no weight.
//
// Everything is integer work and no result depends on the order waves or
// atomics arrive in: the atomics are integer adds (gains, counts, the sides'
// weights in the rollback), bit sets / clears of distinct bits, and a list of
// dirty chunks whose order does not matter (every listed chunk is rescanned
// before the next choice).  k_fm_pass waits on nothing outside its one
// workgroup: its loop runs at most once per node and its phases are separated
// by workgroup barriers only.
//
// State a pass changes (gains, counts, side and lock bitmaps, global chunk
// keys) is read and written with relaxed agent-scope atomics, so a wave never
// reads a line its CU cached before another wave's update.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

namespace {

using u64 = unsigned long long;

template <class T>
__device__ __forceinline__ T ld(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void st(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned bit_of(const unsigned* words, unsigned v) { return (ld(words + (v >> 5)) >> (v & 31u)) & 1u; }

__device__ __forceinline__ u64 wave_max(u64 k) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 x = __shfl_xor(k, o, 64);
        k = x > k ? x : k;
    }
    return k;
}
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the barrier between two phases of the pass: this wave's stores and atomics
// have reached L2 (vmcnt(0), gfx9 encoding) before any wave goes on to read them
__device__ __forceinline__ void wg_barrier() {
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
}

constexpr int FC_THREADS = 256, FC_SHORT = 8;  // a thread takes a net of <= FC_SHORT pins, the wave a longer one
constexpr int FG_LONG = 32;                    // a thread takes a node of <= FG_LONG nets, the wave one of more

template <class D>
constexpr bool weighted = std::is_same_v<D, FmwDev>;

}  // namespace

// ---------------------------------------------------------------------------
// cnt(e, 0), cnt(e, 1) of every net and the number of cut nets, laid out as
// k_kway_metrics and k_sweep_spans.  state[3] += the block's cut nets;
// weighted: state[3] += the block's weighted cut (a 64-bit sum over the
// block), state[4] += its cut nets.
template <class D>
__global__ __launch_bounds__(FC_THREADS) void k_fm_counts(D d) {
    constexpr bool WT = weighted<D>;
    __shared__ unsigned ws[FC_THREADS / 64];
    __shared__ u64 wsw[WT ? FC_THREADS / 64 : 1];
    const int t = threadIdx.x, l = t & 63;
    const long long e = blockIdx.x * (long long)FC_THREADS + t;
    unsigned cut = 0u;                 // this thread's cut nets (lane 0: also the wave's long nets)
    [[maybe_unused]] u64 cutw = 0ull;  // and their weight
    int64_t p0 = 0, p1 = 0;
    if (e < d.nets) {
        p0 = d.net_ptr[e];
        p1 = d.net_ptr[e + 1];
    }
    const bool is_long = p1 - p0 > FC_SHORT;
    if (e < d.nets && !is_long) {
        unsigned c1 = 0u;
        for (int64_t p = p0; p < p1; ++p) c1 += bit_of(d.side, unsigned(d.pins[p]));
        const unsigned c0 = unsigned(p1 - p0) - c1;
        d.cnt[2 * e] = c0;
        d.cnt[2 * e + 1] = c1;
        cut += c0 > 0u && c1 > 0u;
        if constexpr (WT) {
            if (c0 > 0u && c1 > 0u) cutw += u64(d.cw[e]);
        }
    }
    u64 todo = __ballot(is_long);
    while (todo) {  // the wave's long nets, one after the other (the ballot is wave-uniform)
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(p0, src, 64), q1 = __shfl(p1, src, 64);
        const long long f = e - l + src;
        unsigned c1 = 0u;
        for (int64_t p = q0 + l; p < q1; p += 64) c1 += bit_of(d.side, unsigned(d.pins[p]));
        c1 = wave_sum(c1);
        if (l == 0) {
            const unsigned c0 = unsigned(q1 - q0) - c1;
            d.cnt[2 * f] = c0;
            d.cnt[2 * f + 1] = c1;
            cut += c0 > 0u && c1 > 0u;
            if constexpr (WT) {
                if (c0 > 0u && c1 > 0u) cutw += u64(d.cw[f]);
            }
        }
    }
    cut = wave_sum(cut);
    if constexpr (WT) cutw = wave_sum(cutw);
    if (l == 0) {
        ws[t >> 6] = cut;
        if constexpr (WT) wsw[t >> 6] = cutw;
    }
    __syncthreads();
    if (t == 0) {
        const unsigned all = ws[0] + ws[1] + ws[2] + ws[3];
        if constexpr (WT) {
            if (all) {
                atomicAdd(reinterpret_cast<u64*>(d.state + 3), wsw[0] + wsw[1] + wsw[2] + wsw[3]);
                atomicAdd(reinterpret_cast<u64*>(d.state + 4), u64(all));
            }
        } else {
            if (all) atomicAdd(reinterpret_cast<u64*>(d.state + 3), u64(all));
        }
    }
}

// ---------------------------------------------------------------------------
// g(v) = sum of c(e) over {e on v : cnt(e, a) = 1} - sum of c(e) over {e on v :
// cnt(e, 1 - a) = 0}, a = v's side; c(e) = 1 unweighted.  Each sum is at most
// 2^31 - 1 (weighted: checked on the host), so 32-bit arithmetic holds them.
template <class D>
__global__ __launch_bounds__(256) void k_fm_gains(D d) {
    auto c_of = [&](int64_t e) -> unsigned {
        if constexpr (weighted<D>) return unsigned(d.cw[e]);
        else return 1u;
    };
    const int t = threadIdx.x, l = t & 63;
    const long long v = blockIdx.x * 256ll + t;
    int64_t i0 = 0, i1 = 0;
    unsigned a = 0u;
    if (v < d.n) {
        i0 = d.inc_ptr[v];
        i1 = d.inc_ptr[v + 1];
        a = bit_of(d.side, unsigned(v));
    }
    const bool is_long = i1 - i0 > FG_LONG;
    if (v < d.n && !is_long) {
        int g = 0;
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t e = d.inc[i];
            const int c = int(c_of(e));
            g += (ld(d.cnt + 2 * e + a) == 1u ? c : 0) - (ld(d.cnt + 2 * e + (1u - a)) == 0u ? c : 0);
        }
        d.gain[v] = g;
    }
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t j0 = __shfl(i0, src, 64), j1 = __shfl(i1, src, 64);
        const unsigned b = __shfl(a, src, 64);
        unsigned up = 0u, dn = 0u;
        for (int64_t i = j0 + l; i < j1; i += 64) {
            const int64_t e = d.inc[i];
            const unsigned c = c_of(e);
            up += ld(d.cnt + 2 * e + b) == 1u ? c : 0u;
            dn += ld(d.cnt + 2 * e + (1u - b)) == 0u ? c : 0u;
        }
        up = wave_sum(up);
        dn = wave_sum(dn);
        if (l == 0) d.gain[v - l + src] = int(up) - int(dn);
    }
}

// ---------------------------------------------------------------------------
// One pass, one workgroup, one launch.
//
// Selection: chunk c of side s has the key max over its unlocked nodes v of
// ((g(v) + 2^31) << 32 | ~v), 0 when it has none: the greatest key is the
// greatest gain and among equals the smallest id.  LDSK: the 2 * nchunks keys,
// the dirty bitmap and the dirty list are in LDS (nchunks <= FM_LDS_CHUNKS);
// otherwise in global memory.  A move marks the chunk of every node whose gain
// or lock it changed; only those are rescanned (a wave a chunk) before the
// next choice, which reduces the chunk keys over the workgroup.  A side has a
// candidate iff S[1 - a] + w(top) <= L_max (unweighted: w = 1, which is s[1 -
// a] < L_max); weighted, that is one more dependent load a move.  Of two
// candidates: the greater g, then the larger / heavier side, then the smaller
// id.
//
// Gains after moving v from a to b: per net e of v (a wave a net), with F =
// cnt(e, a) and T = cnt(e, b) read before the change and c = c(e) (1
// unweighted): T = 0: +c for every other pin; T = 1: -c for the pin on b; then
// F - 1 = 0: -c for every other pin; F - 1 = 1: +c for the other pin on a.  A
// net with none of the four touches no pin.  Locked pins are skipped:
// k_fm_gains recomputes every gain before the next pass.
template <class D, bool LDSK>
__global__ __launch_bounds__(FM_THREADS) void k_fm_pass(D d, int stall, long long mlog_at, long long* rec) {
    constexpr bool WT = weighted<D>;
    using S = std::conditional_t<WT, long long, int>;  // a side's size or weight, and d
    constexpr int W = FM_THREADS / 64;
    __shared__ u64 s_keys[LDSK ? 2 * FM_LDS_CHUNKS : 2];
    __shared__ unsigned s_dirty[LDSK ? FM_LDS_CHUNKS / 32 : 1];
    __shared__ int s_dlist[LDSK ? FM_LDS_CHUNKS : 1];
    __shared__ u64 s_red[2 * W];
    __shared__ int s_nd;
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int nck = d.nchunks;
    u64* keys;
    unsigned* dirty;
    int* dlist;
    if constexpr (LDSK) {
        keys = s_keys;
        dirty = s_dirty;
        dlist = s_dlist;
    } else {
        keys = d.gkeys;
        dirty = d.gdirty;
        dlist = d.gdlist;
    }
    auto ldk = [&](const u64* p) -> u64 {
        if constexpr (LDSK) return *p;
        else return ld(p);
    };
    auto stk = [&](u64* p, u64 k) {
        if constexpr (LDSK) *p = k;
        else st(p, k);
    };
    auto mark = [&](int c) {
        const unsigned bit = 1u << (c & 31);
        if (atomicOr(&dirty[c >> 5], bit) & bit) return;
        const int at = atomicAdd(&s_nd, 1);  // (a chunk is listed once between two rescans: at < nck)
        if (at < nck) {
            if constexpr (LDSK) dlist[at] = c;
            else st(dlist + at, c);
        }
    };
    auto rescan = [&](int c) {  // the calling wave
        u64 k0 = 0ull, k1 = 0ull;
        const long long base = (long long)c * FM_CHUNK;
#pragma unroll
        for (int j = 0; j < FM_CHUNK / 64; ++j) {
            const long long v = base + j * 64 + l;
            if (v < d.n && !bit_of(d.lock, unsigned(v))) {
                const unsigned g = unsigned(ld(d.gain + v)) + 0x80000000u;
                const u64 k = (u64(g) << 32) | u64(~unsigned(v));
                if (bit_of(d.side, unsigned(v))) k1 = k > k1 ? k : k1;
                else k0 = k > k0 ? k : k0;
            }
        }
        k0 = wave_max(k0);
        k1 = wave_max(k1);
        if (l == 0) {
            stk(keys + c, k0);
            stk(keys + nck + c, k1);
            atomicAnd(&dirty[c >> 5], ~(1u << (c & 31)));
        }
    };

    // the pass's start: locks = the nodes of no net, nothing dirty, every key scanned
    const long long nwords = ((long long)d.n + 31) / 32;
    for (long long i = t; i < nwords; i += FM_THREADS) st(d.lock + i, d.lock0[i]);
    for (int i = t; i < (nck + 31) / 32; i += FM_THREADS) {
        if constexpr (LDSK) dirty[i] = 0u;
        else st(dirty + i, 0u);
    }
    if (t == 0) s_nd = 0;
    wg_barrier();
    for (int c = w; c < nck; c += W) rescan(c);
    wg_barrier();

    long long cut = d.state[0];
    S s0 = S(d.state[1]), s1 = S(d.state[2]);
    // weighted: the sides' bounds L0 = d.lmax, L1 = d.lmax1 (§12: equal; §16: a pair), the slack S_a - L_a of a
    // side, and d = |slack 0 - slack 1|; with L0 = L1 these are L_max, the order of the weights and |S0 - S1|
    [[maybe_unused]] S skew = 0;
    if constexpr (WT) skew = d.lmax - d.lmax1;
    auto dist = [&](S x, S y) {
        if constexpr (WT) {
            const S z = x - y - skew;
            return z < 0 ? -z : z;
        } else {
            return x > y ? x - y : y - x;
        }
    };
    long long c_best = cut;
    S d_best = dist(s0, s1);
    [[maybe_unused]] S s0_best = s0;
    int t_best = 0, tt = 0;
    bool bad = false;
    while (tt < d.n) {  // (a node moves at most once a pass)
        // the sides' best keys
        u64 m0 = 0ull, m1 = 0ull;
        for (int c = t; c < nck; c += FM_THREADS) {
            const u64 x = ldk(keys + c), y = ldk(keys + nck + c);
            m0 = x > m0 ? x : m0;
            m1 = y > m1 ? y : m1;
        }
        m0 = wave_max(m0);
        m1 = wave_max(m1);
        if (l == 0) {
            s_red[w] = m0;
            s_red[W + w] = m1;
        }
        wg_barrier();
        m0 = 0ull;
        m1 = 0ull;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            m0 = s_red[q] > m0 ? s_red[q] : m0;
            m1 = s_red[W + q] > m1 ? s_red[W + q] : m1;
        }
        // the top nodes' weights and the choice (the same in every thread)
        const unsigned v0 = ~unsigned(m0), v1 = ~unsigned(m1);
        S w0 = 1, w1 = 1;
        if constexpr (WT) {  // a key that names no node is caught before its weight is read
            if ((m0 != 0ull && v0 >= unsigned(d.n)) || (m1 != 0ull && v1 >= unsigned(d.n))) {
                bad = true;
                break;
            }
            w0 = m0 != 0ull ? d.w[v0] : 0;
            w1 = m1 != 0ull ? d.w[v1] : 0;
        }
        S into1 = d.lmax;  // the bound of the side that side 0's top node would enter; into0: side 1's
        if constexpr (WT) into1 = d.lmax1;
        const S into0 = d.lmax;
        const bool have0 = s1 + w0 <= into1 && m0 != 0ull, have1 = s0 + w1 <= into0 && m1 != 0ull;
        if (!have0 && !have1) break;
        const int g0 = int(unsigned(m0 >> 32) - 0x80000000u), g1 = int(unsigned(m1 >> 32) - 0x80000000u);
        const S k0 = s0 - skew, k1 = s1;  // (the slacks, both shifted by L1: their order is the slacks')
        unsigned a;  // the side the node leaves
        if (have0 && have1) a = g0 != g1 ? unsigned(g1 > g0) : k0 != k1 ? unsigned(k1 > k0) : unsigned(v1 < v0);
        else a = have1 ? 1u : 0u;
        const unsigned v = a ? v1 : v0;
        const int g = a ? g1 : g0;
        const S wv = a ? w1 : w0;
        if constexpr (!WT) {
            if (v >= unsigned(d.n)) {
                bad = true;
                break;
            }
        }
        // the move
        cut -= g;
        s0 += a ? wv : -wv;
        s1 += a ? -wv : wv;
        ++tt;
        if (t == 0) {
            atomicXor(d.side + (v >> 5), 1u << (v & 31u));
            atomicOr(d.lock + (v >> 5), 1u << (v & 31u));
            d.pass_nodes[tt - 1] = int32_t(v);
            const long long at = mlog_at + tt - 1;
            if (d.mlog && at < d.mlog_cap) d.mlog[at] = ek_fm_move{int32_t(v), g, cut};
            mark(int(v / FM_CHUNK));
        }
        const S dd = dist(s0, s1);
        if (cut < c_best || (cut == c_best && dd < d_best)) {
            c_best = cut;
            d_best = dd;
            if constexpr (!WT) s0_best = s0;
            t_best = tt;
        }
        // the gains of the free pins of v's nets, and the counts
        const int64_t i0 = d.inc_ptr[v], i1 = d.inc_ptr[v + 1];
        for (int64_t i = i0 + w; i < i1; i += W) {
            const int64_t e = d.inc[i];
            unsigned F = 0u, T = 0u;
            if (l == 0) {
                F = ld(d.cnt + 2 * e + a);
                T = ld(d.cnt + 2 * e + (1u - a));
                st(d.cnt + 2 * e + a, F - 1u);
                st(d.cnt + 2 * e + (1u - a), T + 1u);
            }
            F = __shfl(F, 0, 64);
            T = __shfl(T, 0, 64);
            const bool all_up = T == 0u, one_to = T == 1u, all_dn = F == 1u, one_from = F == 2u;
            if (!(all_up || one_to || all_dn || one_from)) continue;
            int c = 1;
            if constexpr (WT) c = d.cw[e];
            const int64_t p1 = d.net_ptr[e + 1];
            for (int64_t p = d.net_ptr[e] + l; p < p1; p += 64) {
                const unsigned u = unsigned(d.pins[p]);
                if (u == v || bit_of(d.lock, u)) continue;
                const unsigned su = bit_of(d.side, u);
                int dl = 0;
                if (all_up) dl += c;
                else if (one_to && su != a) dl -= c;
                if (all_dn) dl -= c;
                else if (one_from && su == a) dl += c;
                if (dl) {
                    atomicAdd(d.gain + u, dl);
                    mark(int(u / FM_CHUNK));
                }
            }
        }
        if (stall > 0 && tt - t_best >= stall) break;
        wg_barrier();
        const int nd = min(s_nd, nck);
        for (int j = w; j < nd; j += W) {
            int c;
            if constexpr (LDSK) c = dlist[j];
            else c = ld(dlist + j);
            if (c >= 0 && c < nck) rescan(c);
        }
        wg_barrier();
        if (t == 0) s_nd = 0;
    }
    if (t == 0) {
        rec[0] = bad ? -1 : tt;
        rec[1] = t_best;
        rec[2] = c_best;
        rec[3] = d_best;
        if (!bad) {
            d.state[0] = c_best;
            if constexpr (WT) {  // (the weights as after the last move: k_fm_rollback takes the undone moves' back)
                d.state[1] = s0;
                d.state[2] = s1;
            } else {
                d.state[1] = s0_best;
                d.state[2] = (long long)s0 + s1 - s0_best;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// A wave per undone move: the node's side bit flipped back, its nets' counts
// and, weighted, the sides' weights (state[1], state[2]) with it.  The entries
// are distinct nodes, so each bit flips once; the counts and the weights
// change by integer adds.
template <class D>
__global__ __launch_bounds__(256) void k_fm_rollback(D d, int first, int count) {
    const int l = threadIdx.x & 63;
    const long long j = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (j >= count) return;
    const int32_t vs = d.pass_nodes[first + j];
    if (vs < 0 || vs >= d.n) return;
    const unsigned v = unsigned(vs);
    unsigned b = l == 0 ? bit_of(d.side, v) : 0u;  // where it is now
    b = __shfl(b, 0, 64);
    const int64_t i1 = d.inc_ptr[v + 1];
    for (int64_t i = d.inc_ptr[v] + l; i < i1; i += 64) {
        const int64_t e = d.inc[i];
        atomicAdd(d.cnt + 2 * e + b, 0xFFFFFFFFu);
        atomicAdd(d.cnt + 2 * e + (1u - b), 1u);
    }
    if (l == 0) {
        if constexpr (weighted<D>) {
            const u64 wv = u64(d.w[v]);
            if (wv) {
                atomicAdd(reinterpret_cast<u64*>(d.state + 1 + b), 0ull - wv);
                atomicAdd(reinterpret_cast<u64*>(d.state + 2 - b), wv);
            }
        }
        atomicXor(d.side + (v >> 5), 1u << (v & 31u));
    }
}

// ---------------------------------------------------------------------------
template <class D>
void fm_counts(hipStream_t s, const D& d) {
    const unsigned nb = unsigned((int64_t(d.nets) + FC_THREADS - 1) / FC_THREADS);
    hipLaunchKernelGGL(k_fm_counts<D>, dim3(nb), dim3(FC_THREADS), 0, s, d);
}

template <class D>
void fm_gains(hipStream_t s, const D& d) {
    const unsigned nb = unsigned((int64_t(d.n) + 255) / 256);
    hipLaunchKernelGGL(k_fm_gains<D>, dim3(nb), dim3(256), 0, s, d);
}

template <class D>
void fm_pass(hipStream_t s, const D& d, int stall, long long mlog_at, long long* rec) {
    if (d.nchunks <= FM_LDS_CHUNKS) hipLaunchKernelGGL((k_fm_pass<D, true>), dim3(1), dim3(FM_THREADS), 0, s, d, stall, mlog_at, rec);
    else hipLaunchKernelGGL((k_fm_pass<D, false>), dim3(1), dim3(FM_THREADS), 0, s, d, stall, mlog_at, rec);
}

template <class D>
void fm_rollback(hipStream_t s, const D& d, int first, int count) {
    if (count <= 0) return;
    const unsigned nb = unsigned((int64_t(count) + 3) / 4);
    hipLaunchKernelGGL(k_fm_rollback<D>, dim3(nb), dim3(256), 0, s, d, first, count);
}

template void fm_counts(hipStream_t, const FmDev&);
template void fm_counts(hipStream_t, const FmwDev&);
template void fm_gains(hipStream_t, const FmDev&);
template void fm_gains(hipStream_t, const FmwDev&);
template void fm_pass(hipStream_t, const FmDev&, int, long long, long long*);
template void fm_pass(hipStream_t, const FmwDev&, int, long long, long long*);
template void fm_rollback(hipStream_t, const FmDev&, int, int);
template void fm_rollback(hipStream_t, const FmwDev&, int, int);

}  // namespace dev
}  // namespace ek
