// The multilevel bipartition (ek_multilevel_bipartition): host code over the
// C-ABI, as kway.cpp is.  Coarsen by matching (ek_match) and contraction
// (ek_hgr_contract) while a level still shrinks, split the coarsest level
// spectrally under the node weights (ek_lanczos_fiedler, ek_sweep_cut_wb), then
// refine on the way back up (ek_fm_refine_wb at every level), both under the
// sides' bounds: the symmetric L_max, where they are ek_sweep_cut_w and
// ek_fm_refine_w, or the pair of ek_multilevel_bipartition_b.  No KL anywhere:
// it swaps pairs and ignores weights.  Every step is an entry
// point with a host checker of its own, so the driver is a composition and
// nothing else: tests/test_gpu_multilevel.py composes the same V-cycle from the
// checkers and compares.
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

// flags & EK_ML_WEIGHTED_LAPLACIAN: the coarsest level's Laplacian carries H_L's
// net weights (ek_spmv_setup_pins_w); nothing else changes.
// bounds: the sides' bounds (L0, L1) of ek_multilevel_bipartition_b (DESIGN.md
// §16); null: the symmetric bound L_max = floor((1 + imbalance) ceil(W / 2)) of
// the other entries, under which the bounded sweep and FM are §13's and §12's.
void bipartition(ek_ctx* ctx, const ek_hgr& h, const ek_ml_opts* opts, int32_t flags, const int64_t* bounds,
                 uint8_t* side_out, ek_ml_result* result) {
    const auto t0 = clk::now();
    if (flags & ~int32_t(EK_ML_WEIGHTED_LAPLACIAN))
        ek::fail(EK_EINVAL, "ek_multilevel_bipartition_ex: unknown flag bits 0x%x", unsigned(flags));
    ek_ml_opts o;
    ek_ml_default_opts(&o);
    if (opts) o = *opts;
    int rank = 0, nranks = 1;
    ek::ctx_ranks(ctx, &rank, &nranks);
    if (nranks > 1)
        ek::fail(EK_ESTATE, "ek_multilevel_bipartition: a multi-rank context (%d ranks); it runs on one", nranks);
    if (!bounds && (!std::isfinite(o.imbalance) || o.imbalance < 0.0))
        ek::fail(EK_EINVAL, "ek_multilevel_bipartition: imbalance %g (finite and >= 0)", o.imbalance);
    if (o.coarse_nodes < 8) o.coarse_nodes = 8;
    if (o.max_levels < 1 || o.max_levels > EK_ML_LEVELS) o.max_levels = EK_ML_LEVELS;
    ek_ml_result r{};
    for (int64_t v = 0; v < h.nodes; ++v) r.total_weight += h.node_w.empty() ? 1 : h.node_w[size_t(v)];
    int64_t B[2];  // what the sweep and FM are given: within [0, W] (a bound above W holds nothing more)
    if (bounds) {
        ek::bounds_check("ek_multilevel_bipartition_b", r.total_weight, bounds);
        B[0] = bounds[0];
        B[1] = bounds[1];
        r.max_part = std::max(B[0], B[1]);
    } else {
        r.max_part = ek::refine_max_part(r.total_weight, 2, o.imbalance);
        B[0] = B[1] = std::min(r.max_part, r.total_weight);
    }
    if (o.match.max_cluster <= 0) {
        // a node no heavier than L0 + L1 - W + 1 (2 L_max - W + 1) cannot make
        // the weighted sweep jump over its window (§13, §16); 4 W / coarse_nodes
        // keeps the coarsest level's nodes comparable
        const int64_t per = (4 * r.total_weight + o.coarse_nodes - 1) / o.coarse_nodes;
        const int64_t room = bounds ? B[0] + B[1] - r.total_weight + 1 : 2 * r.max_part - r.total_weight + 1;
        o.match.max_cluster = std::max<int64_t>(1, std::min(room, per));
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
        chk(ek_match(ctx, cur, &o.match, nullptr, cl.data(), nullptr, 0, &mr));
        r.t_match += since(t);
        if (10 * mr.n_coarse > 9 * cur->nodes) break;  // less than 10 % fewer nodes: not worth a level
        t = clk::now();
        ek_hgr* next = nullptr;
        chk(ek_hgr_contract(cur, cl.data(), mr.n_coarse, &next));
        r.t_contract += since(t);
        r.match_rounds[r.levels] = mr.rounds;
        r.match_pairs[r.levels] = mr.pairs;
        level.emplace_back(next, ek_hgr_free);
        cluster.push_back(std::move(cl));
        cur = next;
        dims(++r.levels, cur);
    }

    // the coarsest level's split
    const int L = r.levels;
    const int64_t nc = cur->nodes;
    std::vector<double> v(static_cast<size_t>(nc));
    bool edges = false;  // a net of >= 2 pins (a contracted level's nets all are)
    for (int64_t e = 0; e < cur->nets && !edges; ++e) edges = cur->net_ptr[size_t(e) + 1] - cur->net_ptr[size_t(e)] >= 2;
    bool spectral = edges && nc >= (o.lanczos.deflate ? 4 : 6);  // (below it ek_lanczos_fiedler answers EK_EINVAL)
    if (spectral) {
        const auto t = clk::now();
        if (flags & EK_ML_WEIGHTED_LAPLACIAN) chk(ek::spmv_setup_hgr_w(ctx, *cur, nullptr));
        else chk(ek_spmv_setup_pins(ctx, nc, cur->nets, cur->net_ptr.data(), cur->pins.data(), nullptr));
        double lambda = 0.0;
        ek_lanczos_stats st{};
        const int rc = ek_lanczos_fiedler(ctx, &o.lanczos, &lambda, v.data(), &st);
        r.t_lanczos = since(t);
        if (rc == EK_ENOCONV) spectral = false;
        else chk(rc);
    }
    if (!spectral) {  // the k-way path's fallback: the split by node index
        r.coarsest_fallback = 1;
        for (int64_t i = 0; i < nc; ++i) v[size_t(i)] = -double(i);
    }
    auto t = clk::now();
    ek_sweep_opts so;
    ek_sweep_default_opts(&so);
    ek_sweep_wb_result sr{};
    chk(ek_sweep_cut_wb(ctx, cur, v.data(), &so, B, nullptr, nullptr, nullptr, &sr));
    r.sweep_feasible = sr.feasible;
    std::vector<uint8_t> side(static_cast<size_t>(nc));
    chk(ek_rank_split(nc, v.data(), sr.n1, side.data()));
    r.t_sweep = since(t);

    // refine, project, refine ... down to H_0
    for (int l = L; l >= 0; --l) {
        const ek_hgr* g = l ? level[size_t(l) - 1].get() : &h;
        if (l < L) {
            const std::vector<int32_t>& cl = cluster[size_t(l)];
            std::vector<uint8_t> fine(cl.size());
            for (size_t i = 0; i < cl.size(); ++i) fine[i] = side[size_t(cl[i])];
            side.swap(fine);
        }
        t = clk::now();
        ek_fm_wb_result fr{};
        chk(ek_fm_refine_wb(ctx, g, &o.fm, B, side.data(), nullptr, 0, nullptr, 0, &fr));
        r.t_fm += since(t);
        r.cut_before[l] = fr.cut_before;
        r.cut_after[l] = fr.cut;
        r.fm_moves[l] = fr.moves_kept;
    }
    int64_t m[4];
    chk(ek_bipart_metrics_host(&h, side.data(), m));
    r.cut = m[0];
    r.cut_nets = m[1];
    r.w0 = m[2];
    r.w1 = m[3];
    for (uint8_t s : side) ++(s ? r.n1 : r.n0);
    std::copy(side.begin(), side.end(), side_out);
    r.t_total = since(t0);
    if (result) *result = r;
}

}  // namespace

namespace ek {
// `gKL2 <in> -EIG --multilevel EPS [--ml-weighted-laplacian]` (cli.cpp refers to it weakly); coarse_nodes <= 0,
// stall < 0: the defaults; flags: ek_multilevel_bipartition_file_ex's
int ml_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, double imbalance, int coarse_nodes,
                    int max_passes, int stall, int32_t flags, ek_ml_result* r);
int ml_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, double imbalance, int coarse_nodes,
                    int max_passes, int stall, int32_t flags, ek_ml_result* r) {
    ek_ml_opts o;
    ek_ml_default_opts(&o);
    o.imbalance = imbalance;
    if (coarse_nodes > 0) o.coarse_nodes = coarse_nodes;
    o.fm.max_passes = max_passes;
    if (stall >= 0) o.fm.stall = stall;
    if (lanczos) o.lanczos = *lanczos;
    return ek_multilevel_bipartition_file_ex(ctx, path, &o, nullptr, flags, nullptr, r);
}
}  // namespace ek

extern "C" {

void ek_ml_default_opts(ek_ml_opts* o) {
    if (!o) return;
    *o = ek_ml_opts{};
    o->imbalance = 0.03;
    o->coarse_nodes = 512;
    o->max_levels = EK_ML_LEVELS;
    ek_match_default_opts(&o->match);
    o->match.max_cluster = 0;  // from W, L_max and coarse_nodes
    ek_fm_default_opts(&o->fm);
    ek_lanczos_default_opts(&o->lanczos);
}

int ek_multilevel_bipartition(ek_ctx* ctx, const ek_hgr* h, const ek_ml_opts* opts, uint8_t* side_out,
                              ek_ml_result* result) {
    return ek_multilevel_bipartition_ex(ctx, h, opts, 0, side_out, result);
}

int ek_multilevel_bipartition_ex(ek_ctx* ctx, const ek_hgr* h, const ek_ml_opts* opts, int32_t flags, uint8_t* side_out,
                                 ek_ml_result* result) {
    EK_TRY
    if (!ctx || !h || (h->nodes > 0 && !side_out)) ek::fail(EK_EINVAL, "ek_multilevel_bipartition: null argument");
    bipartition(ctx, *h, opts, flags, nullptr, side_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_multilevel_bipartition_b(ek_ctx* ctx, const ek_hgr* h, const ek_ml_opts* opts, int32_t flags,
                                const int64_t bounds[2], uint8_t* side_out, ek_ml_result* result) {
    EK_TRY
    if (!ctx || !h || !bounds || (h->nodes > 0 && !side_out))
        ek::fail(EK_EINVAL, "ek_multilevel_bipartition_b: null argument");
    bipartition(ctx, *h, opts, flags, bounds, side_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_multilevel_bipartition_file(ek_ctx* ctx, const char* path, const ek_ml_opts* opts, const char* out_dir,
                                   uint8_t* side_out, ek_ml_result* result) {
    return ek_multilevel_bipartition_file_ex(ctx, path, opts, out_dir, 0, side_out, result);
}

int ek_multilevel_bipartition_file_ex(ek_ctx* ctx, const char* path, const ek_ml_opts* opts, const char* out_dir,
                                      int32_t flags, uint8_t* side_out, ek_ml_result* result) {
    EK_TRY
    if (!ctx || !path) ek::fail(EK_EINVAL, "ek_multilevel_bipartition_file: null argument");
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    Hgr hg(h, ek_hgr_free);
    std::vector<uint8_t> own;
    if (!side_out) {
        own.resize(size_t(h->nodes));
        side_out = own.data();
    }
    bipartition(ctx, *h, opts, flags, nullptr, side_out, result);
    const std::vector<int32_t> part(side_out, side_out + h->nodes);
    ek::write_part_file(path, out_dir, 2, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
