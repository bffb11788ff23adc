// Direct k-way multilevel partitioning (ek_partition_kway_direct, DESIGN.md
// §19): ONE coarsening of the whole hypergraph, the recursive driver of §16 on
// the small coarsest level only, then the Jet refinement (§18) once per level on
// the way back up.  No FM runs on any large level.
//
// Host code over the C-ABI, as kway_ml.cpp and multilevel.cpp are: every step
// is an entry point with a checker of its own, so the driver is a composition
// and nothing else, and tests/test_gpu_kway_direct.py composes the same cycle
// from the same entries and compares.  The contraction is a seam: the device's
// (ek_hgr_contract_device) or, under EK_KWAY_DIRECT_HOST_CONTRACT, the host's
// (ek_hgr_contract); the two give the same hypergraph byte for byte, so the
// flag changes the time and nothing else.
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

// rb: null for ek_partition_kway_direct_ex; otherwise the rebalancing step of
// ek_partition_kway_direct_rb before every level's Jet, and its record
void partition(ek_ctx* ctx, const ek_hgr& h, const ek_kway_direct_opts* opts, int32_t coarsening, int32_t* part_out,
               ek_kway_direct_result* result, ek_kway_direct_rb_result* rb = nullptr) {
    const auto t0 = clk::now();
    ek_kway_direct_opts o;
    ek_kway_direct_default_opts(&o);
    if (opts) o = *opts;
    int rank = 0, nranks = 1;
    ek::ctx_ranks(ctx, &rank, &nranks);
    if (nranks > 1)
        ek::fail(EK_ESTATE, "ek_partition_kway_direct: a multi-rank context (%d ranks); k-way runs on one", nranks);
    if (o.k < 2 || o.k > 256) ek::fail(EK_EINVAL, "ek_partition_kway_direct: k = %d outside [2, 256]", int(o.k));
    if (!std::isfinite(o.imbalance) || o.imbalance < 0.0)
        ek::fail(EK_EINVAL, "ek_partition_kway_direct: imbalance %g (finite and >= 0)", o.imbalance);
    if (o.flags & ~int32_t(EK_KWAY_DIRECT_HOST_CONTRACT | EK_KWAY_DIRECT_WEIGHTED_LAPLACIAN))
        ek::fail(EK_EINVAL, "ek_partition_kway_direct: unknown flag bits 0x%x", unsigned(o.flags));
    if (h.nodes > INT32_MAX - 1) ek::fail(EK_EINVAL, "ek_partition_kway_direct: %lld nodes", (long long)h.nodes);
    if (coarsening != EK_COARSEN_MATCH && coarsening != EK_COARSEN_CLUSTER)
        ek::fail(EK_EINVAL, "ek_partition_kway_direct: coarsening %d (EK_COARSEN_MATCH or EK_COARSEN_CLUSTER)", int(coarsening));
    if (o.coarse_nodes <= 0) o.coarse_nodes = std::max(512, 128 * o.k);
    if (o.max_levels < 1 || o.max_levels > EK_ML_LEVELS) o.max_levels = EK_ML_LEVELS;
    ek_kway_direct_result r{};
    r.k = o.k;
    for (int64_t v = 0; v < h.nodes; ++v) r.total_weight += h.node_w.empty() ? 1 : h.node_w[size_t(v)];
    r.part_bound = ek::refine_max_part(r.total_weight, o.k, o.imbalance);
    if (o.match.max_cluster <= 0) {
        // a cluster never outweighs the slack of one part, Lk - ceil(W / k); 4 W /
        // coarse_nodes keeps the coarsest level's nodes comparable (multilevel.cpp)
        const int64_t share = (r.total_weight + o.k - 1) / o.k;
        const int64_t per = (4 * r.total_weight + o.coarse_nodes - 1) / o.coarse_nodes;
        o.match.max_cluster = std::max<int64_t>(1, std::min(per, std::max<int64_t>(1, r.part_bound - share)));
    }
    r.max_cluster = o.match.max_cluster;

    // coarsen: level[l] is H_(l+1), cluster[l] maps H_l's nodes onto it
    std::vector<Hgr> level;
    std::vector<std::vector<int32_t>> cluster;
    const ek_hgr* cur = &h;
    auto dims = [&](int l, const ek_hgr* g) { chk(ek_hgr_dims(g, &r.nets[l], &r.nodes[l], &r.pins[l])); };
    dims(0, cur);
    while (cur->nodes > o.coarse_nodes && r.levels < o.max_levels) {
        auto t = clk::now();
        std::vector<int32_t> cl(static_cast<size_t>(cur->nodes));
        ek_match_result mr{};
        if (coarsening == EK_COARSEN_CLUSTER) {  // §20: the same seam, the clustering's rounds and joins
            ek_cluster_result cr{};
            chk(ek_cluster(ctx, cur, &o.match, nullptr, cl.data(), nullptr, 0, &cr));
            mr.n_coarse = cr.n_coarse;
            mr.rounds = cr.rounds;
            mr.pairs = cr.joins;
        } else {
            chk(ek_match(ctx, cur, &o.match, nullptr, cl.data(), nullptr, 0, &mr));
        }
        r.t_match += since(t);
        if (10 * mr.n_coarse > 9 * cur->nodes) break;  // less than 10 % fewer nodes: not worth a level
        t = clk::now();
        ek_hgr* next = nullptr;
        if (o.flags & EK_KWAY_DIRECT_HOST_CONTRACT) chk(ek_hgr_contract(cur, cl.data(), mr.n_coarse, &next));
        else chk(ek_hgr_contract_device(ctx, cur, cl.data(), mr.n_coarse, nullptr, &next));
        r.t_contract += since(t);
        r.match_rounds[r.levels] = mr.rounds;
        r.match_pairs[r.levels] = mr.pairs;
        level.emplace_back(next, ek_hgr_free);
        cluster.push_back(std::move(cl));
        cur = next;
        dims(++r.levels, cur);
    }

    // the coarsest level's partition
    const int L = r.levels;
    auto t = clk::now();
    std::vector<int32_t> part(static_cast<size_t>(cur->nodes), 0);
    {
        ek_kway_ml_opts io = o.initial;
        io.k = o.k;
        io.imbalance = o.imbalance;
        io.flags = o.flags & EK_KWAY_DIRECT_WEIGHTED_LAPLACIAN ? EK_ML_WEIGHTED_LAPLACIAN : 0;
        io.write_results = 0;
        io.out_dir = nullptr;
        ek_kway_ml_result ir{};
        chk(ek_partition_kway_ml(ctx, cur, &io, part.data(), &ir));
        r.initial_fallbacks = ir.coarsest_fallbacks;
        r.infeasible_sweeps = ir.infeasible_sweeps;
    }
    r.t_initial = since(t);

    // refine, project, refine ... down to H_0
    ek_kway_jet_opts jo = o.jet;
    jo.k = o.k;
    jo.imbalance = o.imbalance;
    ek_kway_rebalance_opts bo;
    ek_kway_rebalance_default_opts(&bo);
    bo.k = o.k;
    bo.imbalance = o.imbalance;
    ek_kway_direct_rb_result br{};
    std::vector<int64_t> pw(size_t(4 + o.k));
    for (int l = L; l >= 0; --l) {
        const ek_hgr* g = l ? level[size_t(l) - 1].get() : &h;
        if (l < L) {
            const std::vector<int32_t>& cl = cluster[size_t(l)];
            std::vector<int32_t> fine(cl.size());
            for (size_t i = 0; i < cl.size(); ++i) fine[i] = part[size_t(cl[i])];
            part.swap(fine);
        }
        if (rb) {  // the level's weights; the rebalancer only if a part is above Lk
            t = clk::now();
            chk(ek_kway_metrics_w_host(g, part.data(), o.k, pw.data()));
            for (int32_t p = 0; p < o.k; ++p)
                if (pw[size_t(4 + p)] > r.part_bound) {
                    ++br.over_before[l];
                    br.excess_before[l] += pw[size_t(4 + p)] - r.part_bound;
                }
            br.excess_after[l] = br.excess_before[l];
            if (br.over_before[l] > 0) {
                ek_kway_rebalance_result rr{};
                chk(ek_kway_rebalance(ctx, g, &bo, nullptr, part.data(), nullptr, 0, &rr));
                br.rb_rounds[l] = rr.rounds;
                br.rb_moves[l] = rr.moves;
                br.excess_after[l] = rr.excess;
            }
            br.t_rebalance += since(t);
        }
        t = clk::now();
        ek_kway_jet_result jr{};
        chk(ek_kway_jet(ctx, g, &jo, nullptr, part.data(), nullptr, 0, &jr));
        r.t_jet += since(t);
        r.conn_w_before[l] = jr.connectivity_w_before;
        r.conn_w_after[l] = jr.connectivity_w;
        r.jet_iters[l] = jr.iters;
        r.jet_moves[l] = jr.moves;
    }

    t = clk::now();
    std::vector<int64_t> m(size_t(4 + o.k), 0);
    std::vector<int64_t> nodes_in(size_t(o.k), 0);
    for (int64_t i = 0; i < h.nodes; ++i) ++nodes_in[size_t(part[size_t(i)])];
    if (h.nodes > 0) chk(ek_kway_metrics_w(ctx, &h, part.data(), o.k, m.data()));
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
    std::copy(part.begin(), part.end(), part_out);
    r.t_total = since(t0);
    if (result) *result = r;
    if (rb) *rb = br;
}

}  // namespace

namespace ek {
// `gKL2 <in> -EIG --k N --kway-direct EPS [--ml-coarse N] [--jet-iters I] [--contract-host]
// [--ml-weighted-laplacian] [--coarsen match|cluster]` (cli.cpp refers to it weakly); coarse_nodes <= 0, max_iters <= 0:
// the defaults
int kway_direct_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int coarse_nodes, int max_iters, int32_t flags, int32_t coarsening, ek_kway_direct_result* r);
int kway_direct_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int coarse_nodes, int max_iters, int32_t flags, int32_t coarsening, ek_kway_direct_result* r) {
    ek_kway_direct_opts o;
    ek_kway_direct_default_opts(&o);
    o.k = k;
    o.imbalance = imbalance;
    o.flags = flags;
    o.write_results = 1;
    if (coarse_nodes > 0) o.coarse_nodes = coarse_nodes;
    if (max_iters > 0) o.jet.max_iters = max_iters;
    if (lanczos) o.initial.ml.lanczos = *lanczos;
    return ek_partition_kway_direct_file_ex(ctx, path, &o, coarsening, nullptr, r);
}

// the same through ek_partition_kway_direct_rb_file, for `--kway-direct EPS --rebalance`
int kway_direct_rb_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                int coarse_nodes, int max_iters, int32_t flags, int32_t coarsening,
                                ek_kway_direct_result* r, ek_kway_direct_rb_result* rb);
int kway_direct_rb_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                int coarse_nodes, int max_iters, int32_t flags, int32_t coarsening,
                                ek_kway_direct_result* r, ek_kway_direct_rb_result* rb) {
    ek_kway_direct_opts o;
    ek_kway_direct_default_opts(&o);
    o.k = k;
    o.imbalance = imbalance;
    o.flags = flags;
    o.write_results = 1;
    if (coarse_nodes > 0) o.coarse_nodes = coarse_nodes;
    if (max_iters > 0) o.jet.max_iters = max_iters;
    if (lanczos) o.initial.ml.lanczos = *lanczos;
    return ek_partition_kway_direct_rb_file(ctx, path, &o, coarsening, nullptr, r, rb);
}
}  // namespace ek

extern "C" {

void ek_kway_direct_default_opts(ek_kway_direct_opts* o) {
    if (!o) return;
    *o = ek_kway_direct_opts{};
    o->k = 2;
    o->imbalance = 0.03;
    o->coarse_nodes = 0;  // max(512, 128 k)
    o->max_levels = EK_ML_LEVELS;
    ek_match_default_opts(&o->match);
    o->match.max_cluster = 0;  // from W, Lk and coarse_nodes
    ek_kway_ml_default_opts(&o->initial);
    ek_kway_jet_default_opts(&o->jet);
}

int ek_partition_kway_direct(ek_ctx* ctx, const ek_hgr* h, const ek_kway_direct_opts* opts, int32_t* part_out,
                             ek_kway_direct_result* result) {
    return ek_partition_kway_direct_ex(ctx, h, opts, EK_COARSEN_MATCH, part_out, result);
}

int ek_partition_kway_direct_ex(ek_ctx* ctx, const ek_hgr* h, const ek_kway_direct_opts* opts, int32_t coarsening,
                                int32_t* part_out, ek_kway_direct_result* result) {
    EK_TRY
    if (!ctx || !h || (h->nodes > 0 && !part_out)) ek::fail(EK_EINVAL, "ek_partition_kway_direct: null argument");
    partition(ctx, *h, opts, coarsening, part_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_partition_kway_direct_file(ek_ctx* ctx, const char* path, const ek_kway_direct_opts* opts, int32_t* part_out,
                                  ek_kway_direct_result* result) {
    return ek_partition_kway_direct_file_ex(ctx, path, opts, EK_COARSEN_MATCH, part_out, result);
}

int ek_partition_kway_direct_file_ex(ek_ctx* ctx, const char* path, const ek_kway_direct_opts* opts, int32_t coarsening,
                                     int32_t* part_out, ek_kway_direct_result* result) {
    EK_TRY
    if (!ctx || !path) ek::fail(EK_EINVAL, "ek_partition_kway_direct_file: null argument");
    if (coarsening != EK_COARSEN_MATCH && coarsening != EK_COARSEN_CLUSTER)  // before the file is read
        ek::fail(EK_EINVAL, "ek_partition_kway_direct_file: coarsening %d (EK_COARSEN_MATCH or EK_COARSEN_CLUSTER)", int(coarsening));
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    Hgr hg(h, ek_hgr_free);
    std::vector<int32_t> own;
    if (!part_out) {
        own.resize(size_t(h->nodes));
        part_out = own.data();
    }
    ek_kway_direct_result r{};
    partition(ctx, *h, opts, coarsening, part_out, &r);
    if (opts && opts->write_results) ek::write_part_file(path, opts->out_dir, r.k, h->nodes, part_out);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_partition_kway_direct_rb(ek_ctx* ctx, const ek_hgr* h, const ek_kway_direct_opts* opts, int32_t coarsening,
                                int32_t* part_out, ek_kway_direct_result* result, ek_kway_direct_rb_result* rb) {
    EK_TRY
    if (!ctx || !h || (h->nodes > 0 && !part_out)) ek::fail(EK_EINVAL, "ek_partition_kway_direct_rb: null argument");
    ek_kway_direct_rb_result br{};
    partition(ctx, *h, opts, coarsening, part_out, result, &br);
    if (rb) *rb = br;
    return EK_OK;
    EK_CATCH
}

int ek_partition_kway_direct_rb_file(ek_ctx* ctx, const char* path, const ek_kway_direct_opts* opts, int32_t coarsening,
                                     int32_t* part_out, ek_kway_direct_result* result, ek_kway_direct_rb_result* rb) {
    EK_TRY
    if (!ctx || !path) ek::fail(EK_EINVAL, "ek_partition_kway_direct_rb_file: null argument");
    if (coarsening != EK_COARSEN_MATCH && coarsening != EK_COARSEN_CLUSTER)  // before the file is read
        ek::fail(EK_EINVAL, "ek_partition_kway_direct_rb_file: coarsening %d (EK_COARSEN_MATCH or EK_COARSEN_CLUSTER)",
                 int(coarsening));
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    Hgr hg(h, ek_hgr_free);
    std::vector<int32_t> own;
    if (!part_out) {
        own.resize(size_t(h->nodes));
        part_out = own.data();
    }
    ek_kway_direct_result r{};
    ek_kway_direct_rb_result br{};
    partition(ctx, *h, opts, coarsening, part_out, &r, &br);
    if (opts && opts->write_results) ek::write_part_file(path, opts->out_dir, r.k, h->nodes, part_out);
    if (result) *result = r;
    if (rb) *rb = br;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
