// Fiduccia-Mattheyses refinement of a bipartition on the integer net cut,
// unweighted and weighted: the host pieces.
//
// ek_fm_refine_host and ek_fm_refine_w_host are the checkers of the device
// paths (ek_fm_refine, ek_fm_refine_w: ctx_fm.cpp + kernels_fm.hip).  They are
// one single-threaded pass loop (fm_host_passes), written from the rules
// (eigkl.h) and not from the kernels: an ordered set of
// (gain, id) per side where the device keeps chunk keys, and after a move the
// gain of every free pin of the moved node's nets recomputed from its
// definition where the device applies the critical-net deltas.  Host and
// device share only what is input: L_max (refine_max_part), the participating
// nets with their distinct pins and the node -> net incidence
// (refine_prepare), the argument checks (fm_check) and, weighted, the weights
// and their range rules (fmw_prepare, fmw.cpp).  Each checker counts the cut
// before and after with code that is not the loop's: ek_kway_metrics_host,
// and ek_bipart_metrics_host weighted.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "ek_internal.hpp"

namespace {
using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

void chk(int rc) {
    if (rc != EK_OK) throw ek::Error{rc};
}

// what the passes leave: the result's counters, the tracked cut, the sides' sizes or weights, and their time
// (taken before the loop's sets and arrays are freed)
struct FmPasses {
    int32_t passes = 0, passes_run = 0;
    int64_t moves_tried = 0, moves_kept = 0, cut = 0, S[2] = {0, 0};
    double t_passes = 0.0;
};

// Steps 1-5 of the rule, pass after pass, on side[] from the cut `cut`.  WT =
// false is the unweighted rule (cw and w are not read: every c(e) and w(v) is
// 1), WT = true the weighted one with c(e) = cw[e] per participating net and
// w(v) = w[v].  L[s] is the most side s may hold: L_max twice under §11 and
// §12, the per-side bounds of §16 otherwise, where the balance key is the slack
// difference |(S0 - L[0]) - (S1 - L[1])| and equal gains go to the side of less
// slack; with L[0] = L[1] both are §12's (|S0 - S1|, the heavier side).
// Everything the loop changes but side[] and the logs is a local
// of this frame, returned by value, and the input arrays are reached through
// local pointers: side[] is of a character type, so a store to it could alias
// whatever is read through a reference, which would then be read again.
template <bool WT>
FmPasses fm_host_passes(const char* who, const ek::RefineInput& in, const ek_fm_opts& o, const int32_t* cw,
                        const int32_t* w, int64_t n, const int64_t* bounds, int64_t cut, uint8_t* side, int64_t* pass_log,
                        int64_t log_passes, ek_fm_move* move_log, int64_t move_cap) {
    const auto tp = clk::now();
    FmPasses r;
    int64_t S[2] = {0, 0};
    const int64_t L[2] = {bounds[0], bounds[1]};
    auto slack_diff = [&S, &L] { return std::llabs((S[0] - L[0]) - (S[1] - L[1])); };
    auto w_of = [w](int32_t v) -> int64_t {
        if constexpr (WT) return w[size_t(v)];
        else return 1;
    };
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    const int64_t *const net_ptr = in.net_ptr.data(), *const inc_ptr = in.inc_ptr.data();
    const int32_t *const pins = in.pins.data(), *const inc = in.inc.data();
    const int32_t max_passes = o.max_passes, stall = o.stall;
    for (int64_t v = 0; v < n; ++v) S[side[v]] += w_of(int32_t(v));
    std::vector<int32_t> cnt_v(size_t(nets) * 2, 0);
    int32_t* const cnt = cnt_v.data();  // cnt(e, s)
    for (int64_t e = 0; e < nets; ++e)
        for (int64_t p = net_ptr[e]; p < net_ptr[e + 1]; ++p) ++cnt[e * 2 + side[pins[p]]];
    // g(v) from its definition, on the current state
    auto gain_of = [=](int32_t v) {
        const int a = side[v];
        int64_t g = 0;
        for (int64_t i = inc_ptr[v]; i < inc_ptr[v + 1]; ++i) {
            const int32_t* c = cnt + size_t(inc[i]) * 2;
            const int dg = (c[a] == 1) - (c[1 - a] == 0);
            if constexpr (WT) g += int64_t(cw[inc[i]]) * dg;
            else g += dg;
        }
        return g;
    };
    auto flip = [=, &S](int32_t v) {
        const int a = side[v];
        for (int64_t i = inc_ptr[v]; i < inc_ptr[v + 1]; ++i) {
            --cnt[size_t(inc[i]) * 2 + size_t(a)];
            ++cnt[size_t(inc[i]) * 2 + size_t(1 - a)];
        }
        S[a] -= w_of(v);
        S[1 - a] += w_of(v);
        side[v] = uint8_t(1 - a);
    };
    using Key = std::pair<int64_t, int32_t>;  // (-g, id): begin() is the greatest gain, then the smallest id
    std::set<Key> free_[2];
    std::vector<int64_t> gain(static_cast<size_t>(n), 0);
    std::vector<uint8_t> locked(static_cast<size_t>(n), 0);
    std::vector<int64_t> seen(static_cast<size_t>(n), -1);
    std::vector<int32_t> moved;
    int64_t stamp = 0;
    for (;;) {
        if (max_passes > 0 && r.passes >= max_passes) break;
        // 1. unlock; a node on no participating net never moves
        free_[0].clear();
        free_[1].clear();
        for (int64_t v = 0; v < n; ++v) {
            locked[size_t(v)] = inc_ptr[v] == inc_ptr[v + 1];
            if (locked[size_t(v)]) continue;
            gain[size_t(v)] = gain_of(int32_t(v));
            free_[side[v]].insert({-gain[size_t(v)], int32_t(v)});
        }
        moved.clear();
        int64_t t = 0, t_best = 0, c_best = cut, d_best = slack_diff();
        for (;;) {
            // 2. the candidates: a side's top node, when the other side has room for it (only the top is tried;
            // unweighted, that is while the other side has room)
            int pick = -1;
            Key k[2];
            for (int a = 0; a < 2; ++a) {
                if (free_[a].empty()) continue;
                k[a] = *free_[a].begin();
                if (S[1 - a] + w_of(k[a].second) > L[1 - a]) continue;
                if (pick < 0) pick = a;
                else if (k[a].first != k[pick].first) pick = k[a].first < k[pick].first ? a : pick;  // the greater g
                else if (S[a] - L[a] != S[pick] - L[pick])  // the side of less slack (one bound: holding more / the heavier)
                    pick = S[a] - L[a] > S[pick] - L[pick] ? a : pick;
                else pick = k[a].second < k[pick].second ? a : pick;         // the smaller id
            }
            if (pick < 0) break;
            // 3. move and lock
            const int32_t v = k[pick].second;
            const int64_t g = -k[pick].first;
            free_[pick].erase(free_[pick].begin());
            locked[size_t(v)] = 1;
            flip(v);
            moved.push_back(v);
            ++t;
            cut -= g;
            const int64_t d = slack_diff();
            if (r.moves_tried < move_cap && move_log) move_log[r.moves_tried] = ek_fm_move{v, int32_t(g), cut};
            ++r.moves_tried;
            if (cut < c_best || (cut == c_best && d < d_best)) {
                c_best = cut;
                d_best = d;
                t_best = t;
            }
            // the free pins of v's nets: their gains again from the definition
            ++stamp;
            for (int64_t i = inc_ptr[v]; i < inc_ptr[v + 1]; ++i) {
                const int64_t e = inc[i];
                for (int64_t p = net_ptr[e]; p < net_ptr[e + 1]; ++p) {
                    const int32_t u = pins[p];
                    if (locked[size_t(u)] || seen[size_t(u)] == stamp) continue;
                    seen[size_t(u)] = stamp;
                    const int64_t gu = gain_of(u);
                    if (gu == gain[size_t(u)]) continue;
                    free_[side[u]].erase({-gain[size_t(u)], u});
                    gain[size_t(u)] = gu;
                    free_[side[u]].insert({-gu, u});
                }
            }
            // 4. the stall test
            if (stall > 0 && t - t_best >= stall) break;
        }
        // 5. back to the best prefix
        for (int64_t j = t; j > t_best; --j) flip(moved[size_t(j) - 1]);
        cut = c_best;
        if (pass_log && r.passes_run < log_passes) {
            int64_t* row = pass_log + 4 * int64_t(r.passes_run);
            row[0] = t;
            row[1] = t_best;
            row[2] = c_best;
            row[3] = d_best;
        }
        if (r.passes_run == INT32_MAX) ek::fail(EK_EINVAL, "%s: more than 2^31 - 1 passes", who);
        ++r.passes_run;
        r.moves_kept += t_best;
        if (t_best == 0) break;
        ++r.passes;
    }
    r.cut = cut;
    r.S[0] = S[0];
    r.S[1] = S[1];
    r.t_passes = since(tp);
    return r;
}

template <class R>
void fm_host_counters(const FmPasses& p, R& r) {
    r.passes = p.passes;
    r.passes_run = p.passes_run;
    r.moves_tried = p.moves_tried;
    r.moves_kept = p.moves_kept;
    r.t_passes = p.t_passes;
}

// The weighted checker under the sides' bounds L (§12: L_max twice; §16: L0, L1),
// R = ek_fm_w_result or ek_fm_wb_result with n, W and its bound fields set: the
// cut before and after counted by ek_bipart_metrics_host, the passes between.
template <class R>
void fmw_host_run(const char* who, const ek_hgr* h, const ek::FmwInput& fi, const int64_t* L, clk::time_point t0,
                  uint8_t* side, int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, R& r) {
    const int64_t n = h->nodes;
    int64_t m[4];
    chk(ek_bipart_metrics_host(h, side, m));
    r.cut_before = m[0];
    r.cut_nets_before = m[1];
    r.t_setup = since(t0);

    const FmPasses p = fm_host_passes<true>(who, fi.in, fi.opts, fi.cw.data(), fi.w.data(), n, L, r.cut_before, side,
                                            pass_log, log_passes, move_log, move_cap);
    fm_host_counters(p, r);

    const auto tm = clk::now();
    chk(ek_bipart_metrics_host(h, side, m));
    r.cut = m[0];
    r.cut_nets = m[1];
    r.w0 = m[2];
    r.w1 = m[3];
    for (int64_t v = 0; v < n; ++v) ++(side[v] ? r.n1 : r.n0);
    if (r.cut != p.cut || r.w0 != p.S[0] || r.w1 != p.S[1])
        ek::fail(EK_EINVAL, "%s: tracked cut %lld and weights %lld | %lld, counted %lld and %lld | %lld", who,
                 (long long)p.cut, (long long)p.S[0], (long long)p.S[1], (long long)r.cut, (long long)r.w0, (long long)r.w1);
    r.t_metrics = since(tm);
}
}  // namespace

namespace ek {

ek_fm_opts fm_check(const char* who, const ek_hgr* h, const ek_fm_opts* opts, const uint8_t* side) {
    ek_fm_opts o;
    ek_fm_default_opts(&o);
    if (opts) o = *opts;
    if (!h || (h->nodes > 0 && !side)) fail(EK_EINVAL, "%s: null argument", who);
    if (!std::isfinite(o.imbalance) || o.imbalance < 0.0)
        fail(EK_EINVAL, "%s: imbalance %g (finite and >= 0)", who, o.imbalance);
    if (h->nodes > INT32_MAX - 1) fail(EK_EINVAL, "%s: %lld nodes", who, (long long)h->nodes);
    for (int64_t i = 0; i < h->nodes; ++i)
        if (side[i] > 1) fail(EK_EINVAL, "%s: side %d of node %lld outside {0, 1}", who, int(side[i]), (long long)i);
    return o;
}

int sweep_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, int32_t limit, double imbalance,
                       int ratio, ek_sweep_result* sr, ek_kl_result* kr, double* lambda, ek_lanczos_stats* st);

namespace {
ek_fm_opts cli_opts(double imbalance, int max_passes, int stall) {
    ek_fm_opts fo;
    ek_fm_default_opts(&fo);
    fo.imbalance = imbalance;
    fo.max_passes = max_passes;
    if (stall >= 0) fo.stall = stall;  // (< 0: the default)
    return fo;
}

// the sides of KL's best prefix, the FM refinement on the device (refine:
// ek_fm_refine or ek_fm_refine_w), then results/<base>.part.2
template <class Refine, class R>
void cli_refine(ek_ctx* ctx, const char* path, const ek_hgr* h, const ek_fm_opts& fo, Refine refine, R* fr) {
    std::vector<uint8_t> sides(static_cast<size_t>(h->nodes));
    chk(ek_kl_sides(ctx, 1, sides.data()));
    chk(refine(ctx, h, &fo, sides.data(), nullptr, 0, nullptr, 0, fr));
    std::vector<int32_t> part(sides.begin(), sides.end());
    write_part_file(path, nullptr, 2, h->nodes, part.data());
}
}  // namespace

// `gKL2 <in> -EIG [--sweep EPS [--sweep-ratio]] --fm EPS` (cli.cpp refers to it
// weakly): the bipartition as without --fm (ek_solve_file, its results file
// included) or from the sweep cut, then cli_refine
int fm_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                    double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr, ek_fm_result* fr);
int fm_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                    double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr, ek_fm_result* fr) {
    EK_TRY
    if (!ctx || !path || !so || !sr || !kr || !fr) fail(EK_EINVAL, "fm: null argument");
    const ek_fm_opts fo = cli_opts(imbalance, max_passes, stall);
    if (sweep)
        chk(sweep_file_for_cli(ctx, path, &so->lanczos, so->limit, sweep_eps, ratio, sr, kr, nullptr, nullptr));
    else {
        ek_solve_result res{};
        chk(ek_solve_file(ctx, path, so, nullptr, 0, &res));
        *kr = res.kl;
    }
    ek_hgr* h = nullptr;
    chk(ek_hgr_read(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    cli_refine(ctx, path, h, fo, ek_fm_refine, fr);
    return EK_OK;
    EK_CATCH
}

// `gKL2 <in> -EIG [--sweep EPS [--sweep-ratio]] --fm EPS --weighted` (cli.cpp
// refers to it weakly): fm_file_for_cli with the hMETIS reader and the
// weighted refinement.  Lanczos, the split and KL work on the structure alone.
int fmw_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                     double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr,
                     ek_fm_w_result* fr);
int fmw_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                     double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr,
                     ek_fm_w_result* fr) {
    EK_TRY
    if (!ctx || !path || !so || !sr || !kr || !fr) fail(EK_EINVAL, "fmw: null argument");
    const ek_fm_opts fo = cli_opts(imbalance, max_passes, stall);
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    // The steps before FM take the hypergraph this reader gave them, not the file (ek_hgr_read would take the net
    // weights for pins): what ek_solve_file and sweep_file_for_cli do after their own read.
    int rank = 0, nranks = 1;
    ctx_ranks(ctx, &rank, &nranks);
    const std::function<ek_ctx*()> get = [ctx] { return ctx; };
    if (sweep) {
        ek_sweep_opts wo;
        ek_sweep_default_opts(&wo);
        wo.objective = ratio ? 1 : 0;
        wo.imbalance = sweep_eps;
        if (h->nodes < 2) fail(EK_EINVAL, "sweep: %lld nodes", (long long)h->nodes);
        chk(spmv_setup_hgr(ctx, *h, nullptr));
        double lam = 0.0;
        ek_lanczos_stats ls{};
        chk(ek_lanczos_fiedler(ctx, &so->lanczos, &lam, nullptr, &ls));
        ThreadStatus ts = kl_graph_host(&get, h, kl_graph_threads(false));
        if (ts.code != EK_OK) fail(ts.code, "KL graph setup: %s", ts.msg.c_str());
        chk(ek_kl_set_partition_fiedler_sweep(ctx, h, &wo, sr));
        chk(ek_kl_run(ctx, so->limit, nullptr, 0, kr));
    } else {
        ek_solve_result res{};
        solve(get, rank, nranks, *h, std::string(path).substr(std::string(path).find_last_of('/') + 1), *so, nullptr, 0,
              res);
        *kr = res.kl;
    }
    cli_refine(ctx, path, h, fo, ek_fm_refine_w, fr);
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

// stall = 1000 is a choice of the rule's parameter (a pass gives up 1000 moves
// after its best prefix), not a measured optimum
void ek_fm_default_opts(ek_fm_opts* o) {
    if (!o) return;
    o->imbalance = 0.03;
    o->max_passes = 0;
    o->stall = 1000;
}

int ek_fm_refine_host(const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side, int64_t* pass_log, int64_t log_passes,
                      ek_fm_move* move_log, int64_t move_cap, ek_fm_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    const ek_fm_opts o = ek::fm_check("ek_fm_refine_host", h, opts, side);
    const int64_t n = h->nodes;
    ek::RefineInput in;
    ek::refine_prepare(*h, in);
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    ek_fm_result r{};
    r.n = n;
    r.max_part = ek::refine_max_part(n, 2, o.imbalance);
    std::vector<int32_t> part(side, side + n);
    int64_t m[3] = {0, 0, 0};
    if (nets > 0) chk(ek_kway_metrics_host(nets, in.net_ptr.data(), in.pins.data(), part.data(), 2, m));
    r.cut_before = m[0];
    r.t_setup = since(t0);

    const int64_t L[2] = {r.max_part, r.max_part};
    const FmPasses p = fm_host_passes<false>("ek_fm_refine_host", in, o, nullptr, nullptr, n, L, r.cut_before, side, pass_log,
                                             log_passes, move_log, move_cap);
    fm_host_counters(p, r);

    const auto tm = clk::now();
    r.n0 = p.S[0];
    r.n1 = p.S[1];
    m[0] = 0;
    part.assign(side, side + n);
    if (nets > 0) chk(ek_kway_metrics_host(nets, in.net_ptr.data(), in.pins.data(), part.data(), 2, m));
    r.cut = m[0];
    if (r.cut != p.cut)
        ek::fail(EK_EINVAL, "ek_fm_refine_host: tracked cut %lld, counted %lld", (long long)p.cut, (long long)r.cut);
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_fm_refine_w_host(const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side, int64_t* pass_log, int64_t log_passes,
                        ek_fm_move* move_log, int64_t move_cap, ek_fm_w_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::FmwInput fi;
    ek::fmw_prepare("ek_fm_refine_w_host", h, opts, side, fi);
    ek_fm_w_result r{};
    r.n = h->nodes;
    r.total_weight = fi.total;
    r.max_part = fi.max_part;
    const int64_t L[2] = {fi.max_part, fi.max_part};
    fmw_host_run("ek_fm_refine_w_host", h, fi, L, t0, side, pass_log, log_passes, move_log, move_cap, r);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_fm_refine_wb_host(const ek_hgr* h, const ek_fm_opts* opts, const int64_t bounds[2], uint8_t* side, int64_t* pass_log,
                         int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_wb_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::FmwInput fi;
    ek::fmwb_prepare("ek_fm_refine_wb_host", h, opts, bounds, side, fi);
    ek_fm_wb_result r{};
    r.n = h->nodes;
    r.total_weight = fi.total;
    r.bound0 = bounds[0];
    r.bound1 = bounds[1];
    fmw_host_run("ek_fm_refine_wb_host", h, fi, bounds, t0, side, pass_log, log_passes, move_log, move_cap, r);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
