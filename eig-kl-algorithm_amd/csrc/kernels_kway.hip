// k-way partitioning (kway.cpp): the rank split of a Fiedler vector at a rank
// other than the median, and the k-way quality metrics of a part vector.
// A translation unit of its own: the code objects of the bipartitioner's
// kernels (kernels_kl.hip and the others) are what they were without it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ek_internal.hpp"

namespace ek {
namespace dev {

using u64 = unsigned long long;

// ---------------------------------------------------------------------------
// Rank split: side 1 takes the n1 nodes smallest in the key (ord(v[i]), i).
// The radix select of the median split (split_select, kernels_kl.hip) gives
// K, the key at rank n1 - 1.  Every key below K goes to side 1, and of the
// keys equal to K the `need` = n1 - #{key < K} smallest node ids.  Which ids
// those are is decided by position alone: k_rank_count counts the keys below
// and equal to K per 1024-node block, and k_rank_place ranks every equal key
// by the equal keys of the blocks before it (every block sums those counts in
// the same order) plus a ballot prefix inside the block.  No atomics, so the
// result does not depend on the order the workgroups arrive in.  It then
// places the remain[] lists in node order, plist and the initial sides as
// k_split_place does for the median split.

// the radix order of the select (ord_key, kernels_kl.hip): sign flipped,
// negatives inverted, so -0 sorts before +0
__device__ __forceinline__ u64 rank_key(double v) {
    const u64 u = static_cast<u64>(__double_as_longlong(v));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

constexpr int RK_THREADS = 256, RK_PER = 4, RK_BLOCK = RK_THREADS * RK_PER, RK_WAVES = RK_THREADS / 64;

__global__ __launch_bounds__(RK_THREADS) void k_rank_count(const double* __restrict__ v, int n,
                                                           const u64* __restrict__ key, unsigned* __restrict__ blt,
                                                           unsigned* __restrict__ beq) {
    __shared__ unsigned ws[2][RK_WAVES];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * RK_BLOCK;
    const u64 K = *key;
    unsigned clt = 0, ceq = 0;
#pragma unroll
    for (int u = 0; u < RK_PER; ++u) {
        const long long i = base + u * RK_THREADS + t;
        if (i < n) {
            const u64 k = rank_key(v[i]);
            clt += k < K ? 1u : 0u;
            ceq += k == K ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        clt += __shfl_xor(clt, o, 64);
        ceq += __shfl_xor(ceq, o, 64);
    }
    if ((t & 63) == 0) {
        ws[0][t >> 6] = clt;
        ws[1][t >> 6] = ceq;
    }
    __syncthreads();
    if (t == 0) {
        blt[blockIdx.x] = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
        beq[blockIdx.x] = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
    }
}

__global__ __launch_bounds__(RK_THREADS) void k_rank_place(const double* __restrict__ v, int n,
                                                           const u64* __restrict__ key, unsigned n1, int nb,
                                                           const unsigned* __restrict__ blt,
                                                           const unsigned* __restrict__ beq,
                                                           int32_t* __restrict__ order0, int32_t* __restrict__ order1,
                                                           uint32_t* __restrict__ plist, uint8_t* __restrict__ side,
                                                           unsigned* __restrict__ n0_out) {
    __shared__ unsigned red[3][RK_WAVES];
    __shared__ unsigned ceq_s[RK_PER][RK_WAVES], c0_s[RK_PER][RK_WAVES];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const long long base = (long long)blockIdx.x * RK_BLOCK;
    const u64 K = *key;
    // keys below K in all blocks; keys below / equal to K in the blocks before
    unsigned lt_all = 0, lt_bef = 0, eq_bef = 0;
    for (int b = t; b < nb; b += RK_THREADS) {
        const unsigned x = blt[b];
        lt_all += x;
        if (b < int(blockIdx.x)) {
            lt_bef += x;
            eq_bef += beq[b];
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lt_all += __shfl_xor(lt_all, o, 64);
        lt_bef += __shfl_xor(lt_bef, o, 64);
        eq_bef += __shfl_xor(eq_bef, o, 64);
    }
    if (l == 0) {
        red[0][w] = lt_all;
        red[1][w] = lt_bef;
        red[2][w] = eq_bef;
    }
    bool valid[RK_PER], lt[RK_PER], eq[RK_PER];
    u64 meq[RK_PER];
#pragma unroll
    for (int u = 0; u < RK_PER; ++u) {
        const long long i = base + u * RK_THREADS + t;
        valid[u] = i < n;
        const u64 k = valid[u] ? rank_key(v[i]) : 0ull;
        lt[u] = valid[u] && k < K;
        eq[u] = valid[u] && k == K;
        meq[u] = __ballot(eq[u]);
        if (l == 0) ceq_s[u][w] = unsigned(__popcll(meq[u]));
    }
    __syncthreads();
    lt_all = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    lt_bef = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    eq_bef = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    // K is the key at rank n1 - 1, so fewer than n1 keys lie below it
    // (n1 == 0: the host passes K = 0, below which no key lies)
    const unsigned need = n1 - lt_all;
    const u64 lanes_before = (1ull << l) - 1ull;
    // side 0 = not among the n1 smallest; the nodes of a 256-node row are in
    // id order across the waves, the rows in order u
    bool f[RK_PER];
    u64 m0[RK_PER];
    unsigned rows_eq = eq_bef;  // equal keys before row u
#pragma unroll
    for (int u = 0; u < RK_PER; ++u) {
        unsigned r = rows_eq;
        for (int q = 0; q < RK_WAVES; ++q) {
            if (q < w) r += ceq_s[u][q];
            rows_eq += ceq_s[u][q];
        }
        r += unsigned(__popcll(meq[u] & lanes_before));
        const bool s1 = lt[u] || (eq[u] && r < need);
        f[u] = valid[u] && !s1;
        m0[u] = __ballot(f[u]);
        if (l == 0) c0_s[u][w] = unsigned(__popcll(m0[u]));
    }
    __syncthreads();
    // side-0 nodes in the blocks before this one: its nodes less its side-1 ones
    const unsigned eq1_bef = eq_bef < need ? eq_bef : need;
    unsigned rows0 = unsigned(base) - (lt_bef + eq1_bef);
#pragma unroll
    for (int u = 0; u < RK_PER; ++u) {
        unsigned p0 = rows0;
        for (int q = 0; q < RK_WAVES; ++q) {
            if (q < w) p0 += c0_s[u][q];
            rows0 += c0_s[u][q];
        }
        p0 += unsigned(__popcll(m0[u] & lanes_before));
        if (valid[u]) {
            const uint32_t i = uint32_t(base + u * RK_THREADS + t);
            if (f[u]) {
                order0[p0] = int32_t(i);
                plist[i] = p0;
                side[i] = 0;
            } else {
                const uint32_t p1 = i - p0;
                order1[p1] = int32_t(i);
                plist[i] = p1 | 0x80000000u;
                side[i] = 1;
            }
        }
    }
    if (blockIdx.x == gridDim.x - 1 && t == 0) *n0_out = rows0;
}

size_t rank_tmp_bytes(int n) { return size_t(2) * (size_t((n + RK_BLOCK - 1) / RK_BLOCK) + 1) * sizeof(unsigned); }

void rank_partition(hipStream_t s, void* tmp, const double* v, int n, const u64* key, unsigned n1, int32_t* order0,
                    int32_t* order1, uint32_t* plist, uint8_t* side, unsigned* n0_out) {
    const int nb = (n + RK_BLOCK - 1) / RK_BLOCK;
    unsigned* blt = static_cast<unsigned*>(tmp);
    unsigned* beq = blt + nb + 1;
    hipLaunchKernelGGL(k_rank_count, dim3(nb), dim3(RK_THREADS), 0, s, v, n, key, blt, beq);
    hipLaunchKernelGGL(k_rank_place, dim3(nb), dim3(RK_THREADS), 0, s, v, n, key, n1, nb, blt, beq, order0, order1,
                       plist, side, n0_out);
}

// ---------------------------------------------------------------------------
// k-way metrics.  lambda_e = the distinct parts among net e's pins, counted
// as the bits of a 256-bit mask each thread keeps as four 64-bit words in
// registers (k <= 256).  A thread handles its net when it has at most
// KM_SHORT pins (96 % of the nets of the generator's distribution), the pin
// ids loaded four at a time as k_net_cut loads them; a longer net is taken by
// the whole wave afterwards, its lanes striding over the pins and the mask
// words OR-reduced across the wave.  As in k_net_cut each workgroup stores
// its three sums (part[j * gridDim.x + block]; cut nets, connectivity, SOED)
// and the host adds them: adds on one counter serialise at the memory side.
constexpr int KM_THREADS = 256, KM_SHORT = 8;

struct PartMask {
    u64 m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    __device__ __forceinline__ void set(unsigned p) {  // (no dynamic index: the words stay in registers)
        const u64 b = 1ull << (p & 63u);
        const unsigned q = p >> 6;
        m0 |= q == 0u ? b : 0ull;
        m1 |= q == 1u ? b : 0ull;
        m2 |= q == 2u ? b : 0ull;
        m3 |= q == 3u ? b : 0ull;
    }
    __device__ __forceinline__ unsigned count() const {
        return unsigned(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
    }
};

__global__ __launch_bounds__(KM_THREADS) void k_kway_metrics(long long nets, const int64_t* __restrict__ net_ptr,
                                                             const int32_t* __restrict__ pins,
                                                             const uint8_t* __restrict__ part,
                                                             unsigned* __restrict__ out) {
    __shared__ unsigned ws[3][KM_THREADS / 64];
    const int t = threadIdx.x, l = t & 63;
    const long long e = blockIdx.x * (long long)KM_THREADS + t;
    unsigned cut = 0, conn = 0, soed = 0;  // this thread's nets (lane 0: also the wave's long nets)
    auto add = [&](unsigned lambda) {
        if (lambda >= 2u) {
            cut += 1u;
            conn += lambda - 1u;
            soed += lambda;
        }
    };
    int64_t p0 = 0, p1 = 0;
    if (e < nets) {
        p0 = net_ptr[e];
        p1 = net_ptr[e + 1];
    }
    const bool is_long = p1 - p0 > KM_SHORT;
    if (p1 - p0 >= 2 && !is_long) {
        PartMask m;
        const int v0 = pins[p0];
        m.set(part[v0]);
        for (int64_t p = p0 + 1; p < p1; p += 4) {
            int v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p + u < p1 ? pins[p + u] : v0;  // past the net: the first pin
#pragma unroll
            for (int u = 0; u < 4; ++u) m.set(part[v[u]]);
        }
        add(m.count());
    }
    // the wave's long nets, one after the other (the ballot is wave-uniform)
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(p0, src, 64), q1 = __shfl(p1, src, 64);
        PartMask m;
        for (int64_t p = q0 + l; p < q1; p += 64) m.set(part[pins[p]]);
        for (int o = 32; o > 0; o >>= 1) {
            m.m0 |= __shfl_xor(m.m0, o, 64);
            m.m1 |= __shfl_xor(m.m1, o, 64);
            m.m2 |= __shfl_xor(m.m2, o, 64);
            m.m3 |= __shfl_xor(m.m3, o, 64);
        }
        if (l == 0) add(m.count());
    }
    for (int o = 32; o > 0; o >>= 1) {
        cut += __shfl_xor(cut, o, 64);
        conn += __shfl_xor(conn, o, 64);
        soed += __shfl_xor(soed, o, 64);
    }
    if (l == 0) {
        ws[0][t >> 6] = cut;
        ws[1][t >> 6] = conn;
        ws[2][t >> 6] = soed;
    }
    __syncthreads();
    if (t < 3) {
        const unsigned* c = ws[t];
        out[size_t(t) * gridDim.x + blockIdx.x] = c[0] + c[1] + c[2] + c[3];
    }
}

// The weighted sibling (ek_kway_metrics_w): the same walk over the nets, with
// c(e) (cw null: 1) in a fourth sum, the weighted connectivity sum c(e)
// (lambda_e - 1).  Every sum is 64-bit, reduced over the wave and the workgroup
// and added to out[0..3] (zero before) with one integer atomic each per
// workgroup that has something to add: integer adds commute, so the totals do
// not depend on the order the workgroups arrive in.
__global__ __launch_bounds__(KM_THREADS) void k_kway_metrics_w(long long nets, const int64_t* __restrict__ net_ptr,
                                                               const int32_t* __restrict__ pins,
                                                               const int32_t* __restrict__ cw,
                                                               const uint8_t* __restrict__ part,
                                                               u64* __restrict__ out) {
    __shared__ u64 ws[4][KM_THREADS / 64];
    const int t = threadIdx.x, l = t & 63;
    const long long e = blockIdx.x * (long long)KM_THREADS + t;
    u64 cut = 0, conn = 0, connw = 0, soed = 0;  // this thread's nets (lane 0: also the wave's long nets)
    auto add = [&](unsigned lambda, long long net) {
        if (lambda >= 2u) {
            cut += 1ull;
            conn += lambda - 1u;
            connw += u64(cw ? cw[net] : 1) * (lambda - 1u);
            soed += lambda;
        }
    };
    int64_t p0 = 0, p1 = 0;
    if (e < nets) {
        p0 = net_ptr[e];
        p1 = net_ptr[e + 1];
    }
    const bool is_long = p1 - p0 > KM_SHORT;
    if (p1 - p0 >= 2 && !is_long) {
        PartMask m;
        for (int64_t p = p0; p < p1; ++p) m.set(part[pins[p]]);
        add(m.count(), e);
    }
    // the wave's long nets, one after the other (the ballot is wave-uniform)
    u64 todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int64_t q0 = __shfl(p0, src, 64), q1 = __shfl(p1, src, 64);
        PartMask m;
        for (int64_t p = q0 + l; p < q1; p += 64) m.set(part[pins[p]]);
        for (int o = 32; o > 0; o >>= 1) {
            m.m0 |= __shfl_xor(m.m0, o, 64);
            m.m1 |= __shfl_xor(m.m1, o, 64);
            m.m2 |= __shfl_xor(m.m2, o, 64);
            m.m3 |= __shfl_xor(m.m3, o, 64);
        }
        if (l == 0) add(m.count(), e - l + src);
    }
    for (int o = 32; o > 0; o >>= 1) {
        cut += __shfl_xor(cut, o, 64);
        conn += __shfl_xor(conn, o, 64);
        connw += __shfl_xor(connw, o, 64);
        soed += __shfl_xor(soed, o, 64);
    }
    if (l == 0) {
        ws[0][t >> 6] = cut;
        ws[1][t >> 6] = conn;
        ws[2][t >> 6] = connw;
        ws[3][t >> 6] = soed;
    }
    __syncthreads();
    if (t < 4) {
        const u64* c = ws[t];
        const u64 sum = c[0] + c[1] + c[2] + c[3];
        if (sum) atomicAdd(out + t, sum);
    }
}

// out[p] (256 words, zero before) += the weight of the nodes of part p (w null:
// 1 a node): a workgroup sums its nodes into 256 LDS words, then adds the
// non-zero ones to out.  Integer atomics only.
__global__ __launch_bounds__(KM_THREADS) void k_kway_part_weights(long long n, const uint8_t* __restrict__ part,
                                                                  const int32_t* __restrict__ w, u64* __restrict__ out) {
    __shared__ u64 acc[256];
    const int t = threadIdx.x;
    static_assert(KM_THREADS == 256, "one LDS word a thread");
    acc[t] = 0ull;
    __syncthreads();
    const long long v = blockIdx.x * (long long)KM_THREADS + t;
    if (v < n) {
        const u64 x = w ? u64(w[v]) : 1ull;
        if (x) atomicAdd(&acc[part[v]], x);
    }
    __syncthreads();
    if (acc[t]) atomicAdd(out + t, acc[t]);
}

int kway_metrics_blocks(int64_t nets) { return int((nets + KM_THREADS - 1) / KM_THREADS); }

void kway_metrics_w(hipStream_t s, int64_t nets, const int64_t* net_ptr, const int32_t* pins, const int32_t* cw,
                    int64_t n, const uint8_t* part, const int32_t* w, u64* out) {
    if (nets > 0)
        hipLaunchKernelGGL(k_kway_metrics_w, dim3(unsigned(kway_metrics_blocks(nets))), dim3(KM_THREADS), 0, s,
                           (long long)nets, net_ptr, pins, cw, part, out);
    if (n > 0)
        hipLaunchKernelGGL(k_kway_part_weights, dim3(unsigned((n + KM_THREADS - 1) / KM_THREADS)), dim3(KM_THREADS), 0, s,
                           (long long)n, part, w, out + 4);
}

void kway_metrics(hipStream_t s, int64_t nets, const int64_t* net_ptr, const int32_t* pins, const uint8_t* part,
                  unsigned* out) {
    if (nets <= 0) return;
    hipLaunchKernelGGL(k_kway_metrics, dim3(unsigned(kway_metrics_blocks(nets))), dim3(KM_THREADS), 0, s,
                       (long long)nets, net_ptr, pins, part, out);
}

}  // namespace dev
}  // namespace ek
