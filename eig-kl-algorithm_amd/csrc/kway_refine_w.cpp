// Weighted k-way connectivity refinement under per-part weight bounds: the
// host pieces.
//
// ek_kway_refine_w_host is the checker of the device path (ek_kway_refine_w,
// ctx_kway_refine_w.cpp + kernels_refine_w.hip).  It is written from the rule
// (eigkl.h), one plain loop per step of a round: per-net part counters where
// the device keeps bit masks, a sort and a prefix walk per part where the
// device selects a threshold key.  The two share only what is input, not
// algorithm (refine_w_prepare: the argument checks, weights_prepare and the
// bounds), and nothing here calls into kway_refine.cpp's round code.
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
    if (rc != EK_OK) throw ek::Error{rc};
}
}  // namespace

namespace ek {

void refine_w_prepare(const char* who, const ek_hgr* h, const ek_kway_refine_opts* opts, const int64_t* bounds,
                      const int32_t* part, RefineWInput& out) {
    ek_kway_refine_opts o;
    ek_kway_refine_default_opts(&o);
    if (opts) o = *opts;
    if (bounds) o.imbalance = 0.0;  // ignored: the bounds stand in its place
    out.opts = refine_check(who, h, &o, part);
    out.total = weights_prepare(who, h, out);
    const int k = out.opts.k;
    if (bounds) {
        for (int p = 0; p < k; ++p)
            if (bounds[p] < 0) fail(EK_EINVAL, "%s: bound %lld of part %d", who, (long long)bounds[p], p);
        out.bound.assign(bounds, bounds + k);
    } else {
        out.bound.assign(size_t(k), refine_max_part(out.total, k, out.opts.imbalance));
    }
}

// `gKL2 <in> -EIG --k N --kway-multilevel EPS --refine-weighted EPS2` (cli.cpp
// refers to it weakly): the hMETIS reading of the file, ek_partition_kway_ml,
// then ek_kway_refine_w under the uniform bound at EPS2, then
// results/<base>.part.<N> with the refined vector
// (the first nine arguments are kway_ml_file_for_cli's, kway_ml.cpp)
int kway_ml_refine_w_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                  int coarse_nodes, int max_passes, int stall, int32_t flags, double refine_imbalance,
                                  int max_rounds, ek_kway_ml_result* mr, ek_kway_refine_w_result* rr);
int kway_ml_refine_w_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                  int coarse_nodes, int max_passes, int stall, int32_t flags, double refine_imbalance,
                                  int max_rounds, ek_kway_ml_result* mr, ek_kway_refine_w_result* rr) {
    EK_TRY
    if (!std::isfinite(refine_imbalance) || refine_imbalance < 0.0)
        fail(EK_EINVAL, "--refine-weighted takes an imbalance >= 0");
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    ek_kway_ml_opts o;
    ek_kway_ml_default_opts(&o);
    o.k = k;
    o.imbalance = imbalance;
    o.flags = flags;
    if (coarse_nodes > 0) o.ml.coarse_nodes = coarse_nodes;
    o.ml.fm.max_passes = max_passes;
    if (stall >= 0) o.ml.fm.stall = stall;
    if (lanczos) o.ml.lanczos = *lanczos;
    ek_kway_refine_opts ro;
    ek_kway_refine_default_opts(&ro);
    ro.k = k;
    ro.imbalance = refine_imbalance;
    ro.max_rounds = max_rounds;
    std::vector<int32_t> part(size_t(h->nodes));
    chk(ek_partition_kway_ml(ctx, h, &o, part.data(), mr));
    chk(ek_kway_refine_w(ctx, h, &ro, nullptr, part.data(), nullptr, 0, rr));
    write_part_file(path, nullptr, k, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

int ek_kway_refine_w_host(const ek_hgr* h, const ek_kway_refine_opts* opts, const int64_t* bounds, int32_t* part,
                          int64_t* round_log, int64_t log_rounds, ek_kway_refine_w_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::RefineWInput in;
    ek::refine_w_prepare("ek_kway_refine_w_host", h, opts, bounds, part, in);
    const int64_t n = h->nodes;
    const int k = in.opts.k;
    const std::vector<int64_t>&net_ptr = in.in.net_ptr, &inc_ptr = in.in.inc_ptr, &L = in.bound;
    const std::vector<int32_t>&pins = in.in.pins, &inc = in.in.inc, &cw = in.cw, &w = in.w;
    const int64_t nets = int64_t(net_ptr.size()) - 1;
    ek_kway_refine_w_result r{};
    r.k = k;
    r.total_weight = in.total;
    r.bound_min = *std::min_element(L.begin(), L.end());
    r.bound_max = *std::max_element(L.begin(), L.end());
    std::vector<int64_t> m(size_t(4 + k));
    chk(ek_kway_metrics_w_host(h, part, k, m.data()));
    r.connectivity_w_before = m[2];
    r.t_setup = since(t0);

    const auto tr = clk::now();
    const size_t ks = size_t(k), ns = size_t(n), es = size_t(nets);
    std::vector<int64_t> S(m.begin() + 4, m.end());  // the parts' weights
    std::vector<int32_t> phi(es * ks);               // distinct pins of net e in part p
    std::vector<int64_t> gain(ns), cnt(ks);
    std::vector<int32_t> target(ns), winner(es);
    std::vector<std::vector<int32_t>> into(ks);  // independent candidates per target
    while (nets > 0 && !(in.opts.max_rounds > 0 && r.rounds >= in.opts.max_rounds)) {
        // Phi(e, p)
        std::fill(phi.begin(), phi.end(), 0);
        for (int64_t e = 0; e < nets; ++e)
            for (int64_t p = net_ptr[size_t(e)]; p < net_ptr[size_t(e) + 1]; ++p)
                ++phi[size_t(e) * ks + size_t(part[pins[size_t(p)]])];
        // (a) gains and (b) targets among the parts the node fits into; gain 0: not a candidate
        int64_t candidates = 0;
        for (int64_t v = 0; v < n; ++v) {
            gain[size_t(v)] = 0;
            const int64_t i0 = inc_ptr[size_t(v)], i1 = inc_ptr[size_t(v) + 1];
            if (i1 == i0) continue;
            const int a = part[v];
            int64_t rv = 0, D = 0;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t i = i0; i < i1; ++i) {
                const int32_t e = inc[size_t(i)];
                const int32_t* f = &phi[size_t(e) * ks];
                const int64_t c = cw[size_t(e)];
                D += c;
                if (f[a] == 1) rv += c;
                for (int b = 0; b < k; ++b)
                    if (f[b] > 0) cnt[size_t(b)] += c;
            }
            int64_t best = 0;
            int bt = -1;
            for (int b = 0; b < k; ++b) {
                if (b == a || S[size_t(b)] + w[size_t(v)] > L[size_t(b)]) continue;
                const int64_t g = (rv - D) + cnt[size_t(b)];
                if (bt < 0 || g > best) {
                    best = g;
                    bt = b;
                }
            }
            if (bt >= 0 && best > 0) {
                gain[size_t(v)] = best;
                target[size_t(v)] = bt;
                ++candidates;
            }
        }
        // the winner of every net: greatest gain, then smallest id (-1: no candidate pin)
        for (int64_t e = 0; e < nets; ++e) {
            int32_t win = -1;
            for (int64_t p = net_ptr[size_t(e)]; p < net_ptr[size_t(e) + 1]; ++p) {
                const int32_t v = pins[size_t(p)];
                if (gain[size_t(v)] <= 0) continue;
                if (win < 0 || gain[size_t(v)] > gain[size_t(win)] || (gain[size_t(v)] == gain[size_t(win)] && v < win))
                    win = v;
            }
            winner[size_t(e)] = win;
        }
        // the independent candidates, by target
        int64_t independent = 0;
        for (auto& l : into) l.clear();
        for (int64_t v = 0; v < n; ++v) {
            if (gain[size_t(v)] <= 0) continue;
            bool all = true;
            for (int64_t i = inc_ptr[size_t(v)]; i < inc_ptr[size_t(v) + 1] && all; ++i)
                all = winner[size_t(inc[size_t(i)])] == int32_t(v);
            if (all) {
                into[size_t(target[size_t(v)])].push_back(int32_t(v));
                ++independent;
            }
        }
        // (c) per part: gain descending, id ascending; the longest prefix that fits, not a greedy skip
        int64_t accepted = 0, G = 0;
        for (int b = 0; b < k; ++b) {
            auto& l = into[size_t(b)];
            std::sort(l.begin(), l.end(), [&](int32_t x, int32_t y) {
                return gain[size_t(x)] != gain[size_t(y)] ? gain[size_t(x)] > gain[size_t(y)] : x < y;
            });
            const int64_t room = L[size_t(b)] - S[size_t(b)];
            int64_t acc = 0;
            size_t take = 0;
            while (take < l.size() && acc + w[size_t(l[take])] <= room) acc += w[size_t(l[take++])];
            l.resize(take);
            for (int32_t v : l) G += gain[size_t(v)];
            accepted += int64_t(take);
        }
        if (accepted == 0) break;
        // (d) the moves
        for (int b = 0; b < k; ++b)
            for (int32_t v : into[size_t(b)]) {
                S[size_t(part[v])] -= w[size_t(v)];
                S[size_t(b)] += w[size_t(v)];
                part[v] = b;
            }
        if (round_log && r.rounds < log_rounds) {
            int64_t* row = round_log + 4 * int64_t(r.rounds);
            row[0] = candidates;
            row[1] = independent;
            row[2] = accepted;
            row[3] = G;
        }
        ++r.rounds;
        r.moves += accepted;
        r.gain_total += G;
    }
    r.t_rounds = since(tr);

    const auto tm = clk::now();
    r.part_w_min = *std::min_element(S.begin(), S.end());
    r.part_w_max = *std::max_element(S.begin(), S.end());
    for (int p = 0; p < k; ++p) r.parts_over_bound += S[size_t(p)] > L[size_t(p)];
    chk(ek_kway_metrics_w_host(h, part, k, m.data()));
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.connectivity_w = m[2];
    r.soed = m[3];
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
