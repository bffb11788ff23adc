// Fiduccia-Mattheyses refinement of a bipartition on the integer net cut: the
// host pieces.
//
// ek_fm_refine_host is the checker of the device path (ek_fm_refine,
// ctx_fm.cpp + kernels_fm.hip).  It is single-threaded and written from the
// rule (eigkl.h), not from the kernels: an ordered set of
// (gain, id) per side where the device keeps chunk keys, and after a move the
// gain of every pin of the moved node's nets recomputed from its definition
// where the device applies the critical-net deltas.  The two share only what
// is input: L_max (refine_max_part), the participating nets with their
// distinct pins and the node -> net incidence (refine_prepare), and the
// argument checks (fm_check).
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

// `gKL2 <in> -EIG [--sweep EPS [--sweep-ratio]] --fm EPS` (cli.cpp refers to it
// weakly): the bipartition as without --fm (ek_solve_file, its results file
// included) or from the sweep cut, the sides of KL's best prefix, the FM
// refinement on the device, then results/<base>.part.2
int fm_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                    double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr, ek_fm_result* fr);
int sweep_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, int32_t limit, double imbalance,
                       int ratio, ek_sweep_result* sr, ek_kl_result* kr, double* lambda, ek_lanczos_stats* st);
int fm_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                    double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr, ek_fm_result* fr) {
    EK_TRY
    if (!ctx || !path || !so || !sr || !kr || !fr) fail(EK_EINVAL, "fm: null argument");
    ek_fm_opts fo;
    ek_fm_default_opts(&fo);
    fo.imbalance = imbalance;
    fo.max_passes = max_passes;
    if (stall >= 0) fo.stall = stall;  // (< 0: the default)
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
    std::vector<uint8_t> sides(static_cast<size_t>(h->nodes));
    chk(ek_kl_sides(ctx, 1, sides.data()));
    chk(ek_fm_refine(ctx, h, &fo, sides.data(), nullptr, 0, nullptr, 0, fr));
    std::vector<int32_t> part(sides.begin(), sides.end());
    write_part_file(path, nullptr, 2, h->nodes, part.data());
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

    const auto tp = clk::now();
    int64_t size[2] = {0, 0};
    for (int64_t v = 0; v < n; ++v) ++size[side[v]];
    std::vector<int32_t> cnt(size_t(nets) * 2, 0);  // cnt(e, s)
    for (int64_t e = 0; e < nets; ++e)
        for (int64_t p = in.net_ptr[size_t(e)]; p < in.net_ptr[size_t(e) + 1]; ++p)
            ++cnt[size_t(e) * 2 + side[in.pins[size_t(p)]]];
    // g(v) from its definition, on the current state
    auto gain_of = [&](int32_t v) {
        const int a = side[v];
        int64_t g = 0;
        for (int64_t i = in.inc_ptr[size_t(v)]; i < in.inc_ptr[size_t(v) + 1]; ++i) {
            const int32_t* c = &cnt[size_t(in.inc[size_t(i)]) * 2];
            g += (c[a] == 1) - (c[1 - a] == 0);
        }
        return g;
    };
    auto flip = [&](int32_t v) {
        const int a = side[v];
        for (int64_t i = in.inc_ptr[size_t(v)]; i < in.inc_ptr[size_t(v) + 1]; ++i) {
            --cnt[size_t(in.inc[size_t(i)]) * 2 + size_t(a)];
            ++cnt[size_t(in.inc[size_t(i)]) * 2 + size_t(1 - a)];
        }
        --size[a];
        ++size[1 - a];
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
        int64_t t = 0, t_best = 0, c_best = cut, d_best = std::llabs(size[0] - size[1]);
        for (;;) {
            // 2. the candidates: a side gives one while the other side has room
            int pick = -1;
            Key k[2];
            for (int a = 0; a < 2; ++a) {
                if (size[1 - a] >= r.max_part || free_[a].empty()) continue;
                k[a] = *free_[a].begin();
                if (pick < 0) pick = a;
                else if (k[a].first != k[pick].first) pick = k[a].first < k[pick].first ? a : pick;  // the greater g
                else if (size[a] != size[pick]) pick = size[a] > size[pick] ? a : pick;  // the side holding more
                else pick = k[a].second < k[pick].second ? a : pick;                        // the smaller id
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
            const int64_t d = std::llabs(size[0] - size[1]);
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
        if (r.passes_run == INT32_MAX) ek::fail(EK_EINVAL, "ek_fm_refine_host: more than 2^31 - 1 passes");
        ++r.passes_run;
        r.moves_kept += t_best;
        if (t_best == 0) break;
        ++r.passes;
    }
    r.t_passes = since(tp);

    const auto tm = clk::now();
    r.n0 = size[0];
    r.n1 = size[1];
    m[0] = 0;
    part.assign(side, side + n);
    if (nets > 0) chk(ek_kway_metrics_host(nets, in.net_ptr.data(), in.pins.data(), part.data(), 2, m));
    r.cut = m[0];
    if (r.cut != cut) ek::fail(EK_EINVAL, "ek_fm_refine_host: tracked cut %lld, counted %lld", (long long)cut, (long long)r.cut);
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
