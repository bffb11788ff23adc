// The weighted Fiduccia-Mattheyses refinement (node weights under the balance
// bound, net weights in the cut): the host pieces.
//
// ek_fm_refine_w_host is the checker of the device path (ek_fm_refine_w,
// ctx_fmw.cpp + kernels_fmw.hip).  Like ek_fm_refine_host (fm.cpp) it is
// single-threaded and written from the rule (eigkl.h): an
// ordered set of (gain, id) per side, and after a move the gain of every free
// pin of the moved node's nets recomputed from its definition.  It stands
// beside the unweighted checker, which is untouched.  The two ends share only
// what is input (fmw_prepare).  ek_bipart_metrics_host is written apart from
// both: it walks the hypergraph's own pins, not the prepared input.
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

constexpr int64_t W_LIMIT = int64_t(1) << 62;  // of W and of the sum of all c(e)
}  // namespace

namespace ek {

void fmw_prepare(const char* who, const ek_hgr* h, const ek_fm_opts* opts, const uint8_t* side, FmwInput& out) {
    out.opts = fm_check(who, h, opts, side);
    refine_prepare(*h, out.in);
    const int64_t n = h->nodes, nets = int64_t(out.in.net_ptr.size()) - 1;
    // c(e) of the participating nets: refine_prepare keeps, in file order, the nets of >= 2 distinct pins
    out.cw.assign(size_t(nets), 1);
    if (!h->net_w.empty()) {
        std::vector<int64_t> stamp(size_t(n), -1);
        int64_t at = 0;
        for (int64_t e = 0; e < h->nets; ++e) {
            int distinct = 0;
            for (int64_t p = h->net_ptr[size_t(e)]; p < h->net_ptr[size_t(e) + 1] && distinct < 2; ++p) {
                const int32_t v = h->pins[size_t(p)];
                if (stamp[size_t(v)] == e) continue;
                stamp[size_t(v)] = e;
                ++distinct;
            }
            if (distinct >= 2) out.cw[size_t(at++)] = h->net_w[size_t(e)];
        }
        if (at != nets) fail(EK_EINVAL, "%s: %lld participating nets, %lld weights", who, (long long)nets, (long long)at);
    }
    if (h->node_w.empty()) out.w.assign(size_t(n), 1);
    else out.w = h->node_w;
    int64_t total = 0, csum = 0;
    for (int64_t v = 0; v < n; ++v) {
        if (out.w[size_t(v)] < 0) fail(EK_EINVAL, "%s: weight %d of node %lld", who, out.w[size_t(v)], (long long)v);
        total += out.w[size_t(v)];
    }
    for (int64_t e = 0; e < nets; ++e) {
        if (out.cw[size_t(e)] < 1) fail(EK_EINVAL, "%s: net weight %d", who, out.cw[size_t(e)]);
        csum += out.cw[size_t(e)];
    }
    // (int32 weights over fewer than 2^31 nodes and nets stay below both limits; the rule states them all the same)
    if (total > W_LIMIT || csum > W_LIMIT) fail(EK_EINVAL, "%s: total weight above 2^62", who);
    for (int64_t v = 0; v < n; ++v) {
        int64_t on = 0;
        for (int64_t i = out.in.inc_ptr[size_t(v)]; i < out.in.inc_ptr[size_t(v) + 1]; ++i)
            on += out.cw[size_t(out.in.inc[size_t(i)])];
        if (on > INT32_MAX)
            fail(EK_EINVAL, "%s: the nets on node %lld weigh %lld (at most 2^31 - 1: gains are int32)", who, (long long)v,
                 (long long)on);
    }
    out.total = total;
    out.max_part = refine_max_part(total, 2, out.opts.imbalance);
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
    ek_fm_opts fo;
    ek_fm_default_opts(&fo);
    fo.imbalance = imbalance;
    fo.max_passes = max_passes;
    if (stall >= 0) fo.stall = stall;  // (< 0: the default)
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
    std::vector<uint8_t> sides(static_cast<size_t>(h->nodes));
    chk(ek_kl_sides(ctx, 1, sides.data()));
    chk(ek_fm_refine_w(ctx, h, &fo, sides.data(), nullptr, 0, nullptr, 0, fr));
    std::vector<int32_t> part(sides.begin(), sides.end());
    write_part_file(path, nullptr, 2, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

int ek_bipart_metrics_host(const ek_hgr* h, const uint8_t* side, int64_t out[4]) {
    EK_TRY
    if (!h || !out || (h->nodes > 0 && !side)) ek::fail(EK_EINVAL, "ek_bipart_metrics_host: null argument");
    const int64_t n = h->nodes;
    int64_t m[4] = {0, 0, 0, 0};
    for (int64_t v = 0; v < n; ++v) {
        if (side[v] > 1) ek::fail(EK_EINVAL, "ek_bipart_metrics_host: side %d of node %lld outside {0, 1}", int(side[v]), (long long)v);
        m[2 + side[v]] += h->node_w.empty() ? 1 : h->node_w[size_t(v)];
    }
    std::vector<int64_t> last(size_t(n), -1);  // the last net that counted the node
    for (int64_t e = 0; e < h->nets; ++e) {
        int64_t on[2] = {0, 0};
        for (int64_t p = h->net_ptr[size_t(e)]; p < h->net_ptr[size_t(e) + 1]; ++p) {
            const int32_t v = h->pins[size_t(p)];
            if (last[size_t(v)] == e) continue;
            last[size_t(v)] = e;
            ++on[side[v]];
        }
        if (on[0] > 0 && on[1] > 0) {  // (a cut net has two distinct pins)
            m[0] += h->net_w.empty() ? 1 : h->net_w[size_t(e)];
            ++m[1];
        }
    }
    std::copy(m, m + 4, out);
    return EK_OK;
    EK_CATCH
}

int ek_fm_refine_w_host(const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side, int64_t* pass_log, int64_t log_passes,
                        ek_fm_move* move_log, int64_t move_cap, ek_fm_w_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::FmwInput fi;
    ek::fmw_prepare("ek_fm_refine_w_host", h, opts, side, fi);
    const ek_fm_opts& o = fi.opts;
    const ek::RefineInput& in = fi.in;
    const int64_t n = h->nodes;
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    ek_fm_w_result r{};
    r.n = n;
    r.total_weight = fi.total;
    r.max_part = fi.max_part;
    int64_t m[4];
    chk(ek_bipart_metrics_host(h, side, m));
    r.cut_before = m[0];
    r.cut_nets_before = m[1];
    r.t_setup = since(t0);

    const auto tp = clk::now();
    int64_t S[2] = {0, 0};
    for (int64_t v = 0; v < n; ++v) S[side[v]] += fi.w[size_t(v)];
    std::vector<int32_t> cnt(size_t(nets) * 2, 0);  // cnt(e, s)
    for (int64_t e = 0; e < nets; ++e)
        for (int64_t p = in.net_ptr[size_t(e)]; p < in.net_ptr[size_t(e) + 1]; ++p)
            ++cnt[size_t(e) * 2 + side[in.pins[size_t(p)]]];
    // g(v) from its definition, on the current state
    auto gain_of = [&](int32_t v) {
        const int a = side[v];
        int64_t g = 0;
        for (int64_t i = in.inc_ptr[size_t(v)]; i < in.inc_ptr[size_t(v) + 1]; ++i) {
            const size_t e = size_t(in.inc[size_t(i)]);
            g += int64_t(fi.cw[e]) * ((cnt[e * 2 + size_t(a)] == 1) - (cnt[e * 2 + size_t(1 - a)] == 0));
        }
        return g;
    };
    auto flip = [&](int32_t v) {
        const int a = side[v];
        for (int64_t i = in.inc_ptr[size_t(v)]; i < in.inc_ptr[size_t(v) + 1]; ++i) {
            --cnt[size_t(in.inc[size_t(i)]) * 2 + size_t(a)];
            ++cnt[size_t(in.inc[size_t(i)]) * 2 + size_t(1 - a)];
        }
        S[a] -= fi.w[size_t(v)];
        S[1 - a] += fi.w[size_t(v)];
        side[v] = uint8_t(1 - a);
    };
    using Key = std::pair<int64_t, int32_t>;  // (-g, id): begin() is the greatest gain, then the smallest id
    std::set<Key> free_[2];
    std::vector<int64_t> gain(static_cast<size_t>(n), 0);
    std::vector<uint8_t> locked(static_cast<size_t>(n), 0);
    std::vector<int64_t> seen(static_cast<size_t>(n), -1);
    std::vector<int32_t> moved;
    int64_t cut = r.cut_before, stamp = 0;
    for (;;) {
        if (o.max_passes > 0 && r.passes >= o.max_passes) break;
        // 1. unlock; a node on no participating net never moves
        free_[0].clear();
        free_[1].clear();
        for (int64_t v = 0; v < n; ++v) {
            locked[size_t(v)] = in.inc_ptr[size_t(v)] == in.inc_ptr[size_t(v) + 1];
            if (locked[size_t(v)]) continue;
            gain[size_t(v)] = gain_of(int32_t(v));
            free_[side[v]].insert({-gain[size_t(v)], int32_t(v)});
        }
        moved.clear();
        int64_t t = 0, t_best = 0, c_best = cut, d_best = std::llabs(S[0] - S[1]);
        for (;;) {
            // 2. the candidates: a side's top node, when the other side has room for it (only the top is tried)
            int pick = -1;
            Key k[2];
            for (int a = 0; a < 2; ++a) {
                if (free_[a].empty()) continue;
                k[a] = *free_[a].begin();
                if (S[1 - a] + fi.w[size_t(k[a].second)] > fi.max_part) continue;
                if (pick < 0) pick = a;
                else if (k[a].first != k[pick].first) pick = k[a].first < k[pick].first ? a : pick;  // the greater g
                else if (S[a] != S[pick]) pick = S[a] > S[pick] ? a : pick;                          // the heavier side
                else pick = k[a].second < k[pick].second ? a : pick;                                 // the smaller id
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
            const int64_t d = std::llabs(S[0] - S[1]);
            if (r.moves_tried < move_cap && move_log) move_log[r.moves_tried] = ek_fm_move{v, int32_t(g), cut};
            ++r.moves_tried;
            if (cut < c_best || (cut == c_best && d < d_best)) {
                c_best = cut;
                d_best = d;
                t_best = t;
            }
            // the free pins of v's nets: their gains again from the definition
            ++stamp;
            for (int64_t i = in.inc_ptr[size_t(v)]; i < in.inc_ptr[size_t(v) + 1]; ++i) {
                const int64_t e = in.inc[size_t(i)];
                for (int64_t p = in.net_ptr[size_t(e)]; p < in.net_ptr[size_t(e) + 1]; ++p) {
                    const int32_t u = in.pins[size_t(p)];
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
            if (o.stall > 0 && t - t_best >= o.stall) break;
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
        if (r.passes_run == INT32_MAX) ek::fail(EK_EINVAL, "ek_fm_refine_w_host: more than 2^31 - 1 passes");
        ++r.passes_run;
        r.moves_kept += t_best;
        if (t_best == 0) break;
        ++r.passes;
    }
    r.t_passes = since(tp);

    const auto tm = clk::now();
    chk(ek_bipart_metrics_host(h, side, m));
    r.cut = m[0];
    r.cut_nets = m[1];
    r.w0 = m[2];
    r.w1 = m[3];
    for (int64_t v = 0; v < n; ++v) ++(side[v] ? r.n1 : r.n0);
    if (r.cut != cut || r.w0 != S[0] || r.w1 != S[1])
        ek::fail(EK_EINVAL, "ek_fm_refine_w_host: tracked cut %lld and weights %lld | %lld, counted %lld and %lld | %lld",
                 (long long)cut, (long long)S[0], (long long)S[1], (long long)r.cut, (long long)r.w0, (long long)r.w1);
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
