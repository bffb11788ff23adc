// k-way rebalancing, the second half of the Jet rule: the host pieces
// (DESIGN.md §21).
//
// ek_kway_rebalance_host is the checker of the device path (ek_kway_rebalance,
// ctx_kway_rebalance.cpp + kernels_rebalance.hip).  It is written from the rule
// (eigkl.h), one plain loop per step of a round: per-net part counters where
// the device keeps bit masks, (gain, id) pairs compared as pairs where the
// device packs keys, a sort and a prefix walk per source part and per target
// part where the device selects threshold keys.  The two share only what is
// input (rebalance_prepare: refine_w_prepare), and nothing here calls into any
// refiner's round code.
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

ek_kway_rebalance_opts rebalance_prepare(const char* who, const ek_hgr* h, const ek_kway_rebalance_opts* opts,
                                         const int64_t* bounds, const int32_t* part, RefineWInput& out) {
    ek_kway_rebalance_opts o;
    ek_kway_rebalance_default_opts(&o);
    if (opts) o = *opts;
    ek_kway_refine_opts ro;
    ek_kway_refine_default_opts(&ro);
    ro.k = o.k;
    ro.imbalance = o.imbalance;
    refine_w_prepare(who, h, &ro, bounds, part, out);
    return o;
}

// `gKL2 <in> -EIG --k N --kway-multilevel EPS --rebalance-to EPS2 [--refine-jet
// EPS3]` (cli.cpp refers to it weakly): the hMETIS reading of the file,
// ek_partition_kway_ml, ek_kway_rebalance under the uniform bound at EPS2, then
// (jet_imbalance >= 0) ek_kway_jet under the uniform bound at EPS3, then
// results/<base>.part.<N> with the final vector
// (the first nine arguments are kway_ml_file_for_cli's, kway_ml.cpp)
int kway_ml_rebalance_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                   int coarse_nodes, int max_passes, int stall, int32_t flags, double rb_imbalance,
                                   double jet_imbalance, int max_iters, ek_kway_ml_result* mr,
                                   ek_kway_rebalance_result* rr, ek_kway_jet_result* jr);
int kway_ml_rebalance_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                   int coarse_nodes, int max_passes, int stall, int32_t flags, double rb_imbalance,
                                   double jet_imbalance, int max_iters, ek_kway_ml_result* mr,
                                   ek_kway_rebalance_result* rr, ek_kway_jet_result* jr) {
    EK_TRY
    if (!std::isfinite(rb_imbalance) || rb_imbalance < 0.0) fail(EK_EINVAL, "--rebalance-to takes an imbalance >= 0");
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
    ek_kway_rebalance_opts bo;
    ek_kway_rebalance_default_opts(&bo);
    bo.k = k;
    bo.imbalance = rb_imbalance;
    std::vector<int32_t> part(size_t(h->nodes));
    chk(ek_partition_kway_ml(ctx, h, &o, part.data(), mr));
    chk(ek_kway_rebalance(ctx, h, &bo, nullptr, part.data(), nullptr, 0, rr));
    if (jet_imbalance >= 0.0) {
        ek_kway_jet_opts jo;
        ek_kway_jet_default_opts(&jo);
        jo.k = k;
        jo.imbalance = jet_imbalance;
        jo.max_iters = max_iters;
        chk(ek_kway_jet(ctx, h, &jo, nullptr, part.data(), nullptr, 0, jr));
    }
    write_part_file(path, nullptr, k, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

void ek_kway_rebalance_default_opts(ek_kway_rebalance_opts* o) {
    if (!o) return;
    o->k = 2;
    o->max_rounds = 0;
    o->imbalance = 0.03;
}

int ek_kway_rebalance_host(const ek_hgr* h, const ek_kway_rebalance_opts* opts, const int64_t* bounds, int32_t* part,
                           int64_t* round_log, int64_t log_rounds, ek_kway_rebalance_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::RefineWInput in;
    const ek_kway_rebalance_opts o = ek::rebalance_prepare("ek_kway_rebalance_host", h, opts, bounds, part, in);
    const int64_t n = h->nodes;
    const int k = o.k;
    const std::vector<int64_t>&net_ptr = in.in.net_ptr, &inc_ptr = in.in.inc_ptr, &L = in.bound;
    const std::vector<int32_t>&pins = in.in.pins, &inc = in.in.inc, &cw = in.cw, &w = in.w;
    const int64_t nets = int64_t(net_ptr.size()) - 1;
    const size_t ks = size_t(k), ns = size_t(n), es = size_t(nets);
    ek_kway_rebalance_result r{};
    r.k = k;
    r.total_weight = in.total;
    r.bound_min = *std::min_element(L.begin(), L.end());
    r.bound_max = *std::max_element(L.begin(), L.end());
    std::vector<int64_t> m(size_t(4 + k));
    chk(ek_kway_metrics_w_host(h, part, k, m.data()));
    r.connectivity_w_before = m[2];
    std::vector<int64_t> S(m.begin() + 4, m.end());
    auto excess = [&](int64_t* over) {
        int64_t X = 0;
        *over = 0;
        for (size_t p = 0; p < ks; ++p)
            if (S[p] > L[p]) {
                X += S[p] - L[p];
                ++*over;
            }
        return X;
    };
    int64_t over = 0;
    int64_t X = excess(&over);
    r.parts_over_before = over;
    r.excess_before = X;
    r.t_setup = since(t0);

    const auto tr = clk::now();
    std::vector<int32_t> phi(es * ks);  // distinct pins of net e in part p
    std::vector<int64_t> gain(ns), cnt(ks);
    std::vector<int32_t> target(ns);
    std::vector<std::vector<int32_t>> from(ks), into(ks);  // proposers per source, evicted per target
    // u's proposal is ranked before v's: greater gain, then the smaller id
    auto before = [&](int32_t u, int32_t v) {
        return gain[size_t(u)] != gain[size_t(v)] ? gain[size_t(u)] > gain[size_t(v)] : u < v;
    };
    while (X > 0) {
        // Phi(e, p)
        std::fill(phi.begin(), phi.end(), 0);
        for (int64_t e = 0; e < nets; ++e)
            for (int64_t p = net_ptr[size_t(e)]; p < net_ptr[size_t(e) + 1]; ++p)
                ++phi[size_t(e) * ks + size_t(part[pins[size_t(p)]])];
        // (a) the proposals of the overweight parts' nodes
        int64_t proposers = 0;
        for (auto& l : from) l.clear();
        for (auto& l : into) l.clear();
        for (int64_t v = 0; v < n; ++v) {
            const int a = part[v];
            if (S[size_t(a)] <= L[size_t(a)] || w[size_t(v)] <= 0) continue;
            int64_t rv = 0, D = 0;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t i = inc_ptr[size_t(v)]; i < inc_ptr[size_t(v) + 1]; ++i) {
                const int32_t e = inc[size_t(i)];
                const int32_t* f = &phi[size_t(e) * ks];
                const int64_t c = cw[size_t(e)];
                D += c;
                if (f[a] == 1) rv += c;
                for (int b = 0; b < k; ++b)
                    if (f[b] > 0) cnt[size_t(b)] += c;
            }
            int64_t g = 0;
            int bt = -1;
            for (int b = 0; b < k; ++b) {
                if (b == a || S[size_t(b)] + w[size_t(v)] > L[size_t(b)]) continue;
                const int64_t gb = (rv - D) + cnt[size_t(b)];
                if (bt < 0 || gb > g) {
                    g = gb;
                    bt = b;
                }
            }
            if (bt < 0) continue;
            gain[size_t(v)] = g;
            target[size_t(v)] = bt;
            from[size_t(a)].push_back(int32_t(v));
            ++proposers;
        }
        // (b) per overweight part: the shortest prefix of the rank order that reaches the excess
        int64_t evicted = 0;
        for (int a = 0; a < k; ++a) {
            auto& l = from[size_t(a)];
            if (l.empty()) continue;
            std::sort(l.begin(), l.end(), before);
            const int64_t x = S[size_t(a)] - L[size_t(a)];
            int64_t acc = 0;
            size_t take = 0;
            while (take < l.size() && acc < x) acc += w[size_t(l[take++])];
            for (size_t i = 0; i < take; ++i) into[size_t(target[size_t(l[i])])].push_back(l[i]);
            evicted += int64_t(take);
        }
        // (c) per target: rank order; the longest prefix that fits, not a greedy skip
        int64_t moved = 0;
        for (int b = 0; b < k; ++b) {
            auto& l = into[size_t(b)];
            std::sort(l.begin(), l.end(), before);
            const int64_t room = L[size_t(b)] - S[size_t(b)];
            int64_t acc = 0;
            size_t take = 0;
            while (take < l.size() && acc + w[size_t(l[take])] <= room) acc += w[size_t(l[take++])];
            l.resize(take);
            moved += int64_t(take);
        }
        if (moved == 0) break;  // (e): neither counted nor logged
        // (d) the moves
        for (int b = 0; b < k; ++b)
            for (int32_t v : into[size_t(b)]) {
                S[size_t(part[v])] -= w[size_t(v)];
                S[size_t(b)] += w[size_t(v)];
                part[v] = b;
            }
        X = excess(&over);
        if (round_log && r.rounds < log_rounds) {
            int64_t* row = round_log + 4 * int64_t(r.rounds);
            row[0] = proposers;
            row[1] = evicted;
            row[2] = moved;
            row[3] = X;
        }
        if (r.rounds == INT32_MAX) ek::fail(EK_EINVAL, "ek_kway_rebalance_host: 2^31 rounds");
        ++r.rounds;
        r.moves += moved;
        if (o.max_rounds > 0 && r.rounds == o.max_rounds) break;
    }
    r.t_rounds = since(tr);

    const auto tm = clk::now();
    chk(ek_kway_metrics_w_host(h, part, k, m.data()));
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.connectivity_w = m[2];
    r.soed = m[3];
    r.part_w_min = *std::min_element(m.begin() + 4, m.end());
    r.part_w_max = *std::max_element(m.begin() + 4, m.end());
    for (int p = 0; p < k; ++p)
        if (m[size_t(4 + p)] > L[size_t(p)]) {
            ++r.parts_over_bound;
            r.excess += m[size_t(4 + p)] - L[size_t(p)];
        }
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
