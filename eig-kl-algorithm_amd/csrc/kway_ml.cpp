// k-way partitioning by recursive multilevel bisection under per-side weight
// bounds (ek_partition_kway_ml) and its host-only pieces: the
// bounds of one bisection and the weighted k-way metrics.
//
// Host code over the C-ABI, as kway.cpp and multilevel.cpp are.  The recursion
// is kway.cpp's (depth first, side 0 before side 1, one bisection at a time on
// the one context); a bisection is ek_multilevel_bipartition_b on the block's
// induced sub-hypergraph, which carries the block's node and net weights, under
// the bounds ek_kway_bisect_bounds gives the block.  tests/test_gpu_kwayml.py
// composes the same recursion from the same entries and compares.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "ek_internal.hpp"

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

void chk(int rc) {
    if (rc != EK_OK) throw ek::Error{rc};  // ek_last_error() already holds the message
}

using Hgr = std::unique_ptr<ek_hgr, void (*)(ek_hgr*)>;

int ceil_log2(int32_t k) {
    int d = 0;
    while ((int64_t(1) << d) < k) ++d;
    return d;
}

int64_t weight_of(const ek_hgr& h) {
    if (h.node_w.empty()) return h.nodes;
    int64_t w = 0;
    for (const int32_t x : h.node_w) w += x;
    return w;
}

struct KwayMl {
    ek_ctx* ctx;
    ek_kway_ml_opts o;
    double mult;
    int32_t* part;
    ek_kway_ml_result r{};

    // h: the block; ids: the original id of each of its nodes (null: the root)
    void bisect(const ek_hgr& h, const int32_t* ids, int32_t k, int32_t base, int level) {
        const int64_t n = h.nodes;
        if (k == 1 || n < 2) {  // a final part, or a block too small to split: every node to `base`
            for (int64_t i = 0; i < n; ++i) part[ids ? ids[size_t(i)] : i] = base;
            return;
        }
        const auto tb = clk::now();
        const int32_t kl = (k + 1) / 2, kr = k / 2;
        int64_t L[2];
        const int64_t wb = weight_of(h);
        chk(ek_kway_bisect_bounds(wb, k, r.part_bound, mult, L));
        // Wb > k Lk (only below a bisection that had no feasible split): the cap k_s Lk cannot hold both sides, so
        // the block is split by its shares alone (part_bound = Wb never binds) and its parts end above Lk
        if (L[0] + L[1] < wb) chk(ek_kway_bisect_bounds(wb, k, wb, mult, L));
        std::vector<uint8_t> sides(static_cast<size_t>(n));
        ek_ml_result mr{};
        chk(ek_multilevel_bipartition_b(ctx, &h, &o.ml, o.flags, L, sides.data(), &mr));
        ++r.bisections;
        r.coarsest_fallbacks += mr.coarsest_fallback;
        r.infeasible_sweeps += mr.sweep_feasible ? 0 : 1;
        r.levels_total += mr.levels;
        for (int l = 0; l <= mr.levels; ++l) r.fm_moves += mr.fm_moves[l];
        r.t_match += mr.t_match;
        r.t_contract += mr.t_contract;
        r.t_lanczos += mr.t_lanczos;
        r.t_sweep += mr.t_sweep;
        r.t_fm += mr.t_fm;
        const double d = since(tb);
        r.t_ml += d;
        if (level < EK_KWAY_LEVELS) r.t_level[level] += d;
        for (int s = 0; s < 2; ++s) {
            const int32_t ks = s ? kr : kl, bs = s ? base + kl : base;
            int64_t ns = 0;
            for (int64_t i = 0; i < n; ++i) ns += sides[size_t(i)] == s;
            if (ks == 1 || ns < 2) {
                for (int64_t i = 0; i < n; ++i)
                    if (sides[size_t(i)] == s) part[ids ? ids[size_t(i)] : i] = bs;
                continue;
            }
            const auto ti = clk::now();
            std::vector<uint8_t> keep(static_cast<size_t>(n));
            for (int64_t i = 0; i < n; ++i) keep[size_t(i)] = sides[size_t(i)] == s;
            ek_hgr* sub = nullptr;
            chk(ek_hgr_induce(&h, keep.data(), &sub, nullptr));
            Hgr sg(sub, ek_hgr_free);
            std::vector<int32_t> sid;
            sid.reserve(size_t(ns));
            for (int64_t i = 0; i < n; ++i)
                if (keep[size_t(i)]) sid.push_back(ids ? ids[size_t(i)] : int32_t(i));
            const double di = since(ti);
            r.t_induce += di;
            if (level + 1 < EK_KWAY_LEVELS) r.t_level[level + 1] += di;
            bisect(*sub, sid.data(), ks, bs, level + 1);
        }
    }
};

void partition(ek_ctx* ctx, const ek_hgr& h, const ek_kway_ml_opts* opts, int32_t* part_out, ek_kway_ml_result* result) {
    const auto t0 = clk::now();
    ek_kway_ml_opts o;
    ek_kway_ml_default_opts(&o);
    if (opts) o = *opts;
    int rank = 0, nranks = 1;
    ek::ctx_ranks(ctx, &rank, &nranks);
    if (nranks > 1)
        ek::fail(EK_ESTATE, "ek_partition_kway_ml: a multi-rank context (%d ranks); k-way runs on one", nranks);
    if (o.k < 2 || o.k > 256) ek::fail(EK_EINVAL, "ek_partition_kway_ml: k = %d outside [2, 256]", int(o.k));
    if (!std::isfinite(o.imbalance) || o.imbalance < 0.0)
        ek::fail(EK_EINVAL, "ek_partition_kway_ml: imbalance %g (finite and >= 0)", o.imbalance);
    if (h.nodes > INT32_MAX - 1) ek::fail(EK_EINVAL, "ek_partition_kway_ml: %lld nodes", (long long)h.nodes);
    const int depth = ceil_log2(o.k);
    KwayMl km{ctx, o, depth == 1 ? 1.0 + o.imbalance : std::pow(1.0 + o.imbalance, 1.0 / depth), part_out,
              ek_kway_ml_result{}};
    ek_kway_ml_result& r = km.r;
    r.k = o.k;
    r.total_weight = weight_of(h);
    r.part_bound = ek::refine_max_part(r.total_weight, o.k, o.imbalance);
    km.bisect(h, nullptr, o.k, 0, 0);
    const auto t = clk::now();
    std::vector<int64_t> m(size_t(4 + o.k), 0);
    std::vector<int64_t> nodes_in(size_t(o.k), 0);
    for (int64_t i = 0; i < h.nodes; ++i) ++nodes_in[size_t(part_out[i])];
    if (h.nodes > 0) chk(ek_kway_metrics_w(ctx, &h, part_out, o.k, m.data()));
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.connectivity_w = m[2];
    r.soed = m[3];
    r.part_w_min = *std::min_element(m.begin() + 4, m.end());
    r.part_w_max = *std::max_element(m.begin() + 4, m.end());
    for (int32_t p = 0; p < o.k; ++p) {
        r.parts_over_bound += m[size_t(4 + p)] > r.part_bound;
        r.empty_parts += nodes_in[size_t(p)] == 0;
    }
    r.t_metrics = since(t);
    r.t_total = since(t0);
    if (result) *result = r;
}

}  // namespace

namespace ek {
// `gKL2 <in> -EIG --k N --kway-multilevel EPS [--ml-coarse N] [--ml-weighted-laplacian]` (cli.cpp refers to it weakly);
// coarse_nodes <= 0, stall < 0: the defaults
int kway_ml_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                         int coarse_nodes, int max_passes, int stall, int32_t flags, ek_kway_ml_result* r);
int kway_ml_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                         int coarse_nodes, int max_passes, int stall, int32_t flags, ek_kway_ml_result* r) {
    ek_kway_ml_opts o;
    ek_kway_ml_default_opts(&o);
    o.k = k;
    o.imbalance = imbalance;
    o.flags = flags;
    o.write_results = 1;
    if (coarse_nodes > 0) o.ml.coarse_nodes = coarse_nodes;
    o.ml.fm.max_passes = max_passes;
    if (stall >= 0) o.ml.fm.stall = stall;
    if (lanczos) o.ml.lanczos = *lanczos;
    return ek_partition_kway_ml_file(ctx, path, &o, nullptr, r);
}
}  // namespace ek

extern "C" {

int ek_kway_bisect_bounds(int64_t Wb, int32_t kb, int64_t part_bound, double mult, int64_t out[2]) {
    EK_TRY
    if (!out) ek::fail(EK_EINVAL, "ek_kway_bisect_bounds: null argument");
    if (Wb < 0 || Wb > (int64_t(1) << 61)) ek::fail(EK_EINVAL, "ek_kway_bisect_bounds: block weight %lld", (long long)Wb);
    if (kb < 2 || kb > 256) ek::fail(EK_EINVAL, "ek_kway_bisect_bounds: kb = %d outside [2, 256]", int(kb));
    if (part_bound < 0) ek::fail(EK_EINVAL, "ek_kway_bisect_bounds: part bound %lld", (long long)part_bound);
    if (!std::isfinite(mult) || mult < 1.0) ek::fail(EK_EINVAL, "ek_kway_bisect_bounds: mult %g (finite and >= 1)", mult);
    const int32_t ks[2] = {(kb + 1) / 2, kb / 2};
    for (int s = 0; s < 2; ++s) {
        // ceil(Wb k_s / kb) in 128 bits, floor(mult . ) as refine_max_part takes its floor; then the two caps
        const __int128 num = __int128(Wb) * ks[s];
        const int64_t share = int64_t((num + kb - 1) / kb);
        const double scaled = std::floor(mult * double(share));
        int64_t l = scaled >= 9.2e18 ? INT64_MAX : int64_t(scaled);
        const __int128 cap = __int128(part_bound) * ks[s];
        if (cap < l) l = int64_t(cap);
        out[s] = std::min(l, Wb);
    }
    return EK_OK;
    EK_CATCH
}

int ek_kway_metrics_w_host(const ek_hgr* h, const int32_t* part, int32_t k, int64_t* out) {
    EK_TRY
    if (!h || !out || k < 1 || k > 256 || (h->nodes > 0 && !part)) ek::fail(EK_EINVAL, "ek_kway_metrics_w_host: bad argument");
    std::vector<int64_t> m(size_t(4 + k), 0);
    for (int64_t v = 0; v < h->nodes; ++v) {
        if (part[v] < 0 || part[v] >= k)
            ek::fail(EK_EINVAL, "ek_kway_metrics_w_host: part %d of node %lld outside [0, %d)", part[v], (long long)v, k);
        m[size_t(4 + part[v])] += h->node_w.empty() ? 1 : h->node_w[size_t(v)];
    }
    std::vector<uint8_t> seen(static_cast<size_t>(k));
    for (int64_t e = 0; e < h->nets; ++e) {
        std::fill(seen.begin(), seen.end(), uint8_t(0));
        int64_t lambda = 0;
        for (int64_t p = h->net_ptr[size_t(e)]; p < h->net_ptr[size_t(e) + 1]; ++p) {
            uint8_t& s = seen[size_t(part[h->pins[size_t(p)]])];
            lambda += !s;
            s = 1;
        }
        if (lambda >= 2) {
            ++m[0];
            m[1] += lambda - 1;
            m[2] += (h->net_w.empty() ? 1 : int64_t(h->net_w[size_t(e)])) * (lambda - 1);
            m[3] += lambda;
        }
    }
    std::copy(m.begin(), m.end(), out);
    return EK_OK;
    EK_CATCH
}

void ek_kway_ml_default_opts(ek_kway_ml_opts* o) {
    if (!o) return;
    *o = ek_kway_ml_opts{};
    o->k = 2;
    o->imbalance = 0.03;
    ek_ml_default_opts(&o->ml);
}

int ek_partition_kway_ml(ek_ctx* ctx, const ek_hgr* h, const ek_kway_ml_opts* opts, int32_t* part_out,
                         ek_kway_ml_result* result) {
    EK_TRY
    if (!ctx || !h || (h->nodes > 0 && !part_out)) ek::fail(EK_EINVAL, "ek_partition_kway_ml: null argument");
    partition(ctx, *h, opts, part_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_partition_kway_ml_file(ek_ctx* ctx, const char* path, const ek_kway_ml_opts* opts, int32_t* part_out,
                              ek_kway_ml_result* result) {
    EK_TRY
    if (!ctx || !path) ek::fail(EK_EINVAL, "ek_partition_kway_ml_file: null argument");
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    Hgr hg(h, ek_hgr_free);
    std::vector<int32_t> own;
    if (!part_out) {
        own.resize(size_t(h->nodes));
        part_out = own.data();
    }
    ek_kway_ml_result r{};
    partition(ctx, *h, opts, part_out, &r);
    if (opts && opts->write_results) ek::write_part_file(path, opts->out_dir, r.k, h->nodes, part_out);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
