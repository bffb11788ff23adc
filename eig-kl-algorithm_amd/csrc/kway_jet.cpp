// Parallel weighted k-way refinement that can leave a local minimum, the Jet
// rule on the connectivity metric: the host pieces.
//
// ek_kway_jet_host is the checker of the device path (ek_kway_jet,
// ctx_kway_jet.cpp + kernels_jet.hip).  It is written from the rule (eigkl.h),
// one plain loop per step of an iteration: per-net part counters where the
// device keeps bit masks, (gain, id) pairs compared as pairs where the device
// packs keys, a per-net walk with two flags where the device takes two ballots,
// a sort and a prefix walk per part where the device selects a threshold key,
// a recount of the objective with a stamp per part where the device runs the
// metrics kernel.  The two share only what is input (jet_prepare:
// refine_w_prepare and the checks of the new options), and nothing here calls
// into the other refiners' round code.
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

ek_kway_jet_opts jet_prepare(const char* who, const ek_hgr* h, const ek_kway_jet_opts* opts, const int64_t* bounds,
                             const int32_t* part, RefineWInput& out) {
    ek_kway_jet_opts o;
    ek_kway_jet_default_opts(&o);
    if (opts) o = *opts;
    ek_kway_refine_opts ro;
    ek_kway_refine_default_opts(&ro);
    ro.k = o.k;
    ro.imbalance = o.imbalance;
    refine_w_prepare(who, h, &ro, bounds, part, out);
    if (o.neg_num < 0 || o.neg_den < 1)
        fail(EK_EINVAL, "%s: the negative-gain filter %d / %d (neg_num >= 0, neg_den >= 1)", who, int(o.neg_num),
             int(o.neg_den));
    if (o.patience < 1) fail(EK_EINVAL, "%s: patience %d (>= 1)", who, int(o.patience));
    return o;
}

// `gKL2 <in> -EIG --k N --kway-multilevel EPS --refine-jet EPS2` (cli.cpp
// refers to it weakly): the hMETIS reading of the file, ek_partition_kway_ml,
// then ek_kway_jet under the uniform bound at EPS2, then
// results/<base>.part.<N> with the refined vector
// (the first nine arguments are kway_ml_file_for_cli's, kway_ml.cpp)
int kway_ml_jet_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int coarse_nodes, int max_passes, int stall, int32_t flags, double jet_imbalance,
                             int max_iters, ek_kway_ml_result* mr, ek_kway_jet_result* jr);
int kway_ml_jet_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int coarse_nodes, int max_passes, int stall, int32_t flags, double jet_imbalance,
                             int max_iters, ek_kway_ml_result* mr, ek_kway_jet_result* jr) {
    EK_TRY
    if (!std::isfinite(jet_imbalance) || jet_imbalance < 0.0) fail(EK_EINVAL, "--refine-jet takes an imbalance >= 0");
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
    ek_kway_jet_opts jo;
    ek_kway_jet_default_opts(&jo);
    jo.k = k;
    jo.imbalance = jet_imbalance;
    jo.max_iters = max_iters;
    std::vector<int32_t> part(size_t(h->nodes));
    chk(ek_partition_kway_ml(ctx, h, &o, part.data(), mr));
    chk(ek_kway_jet(ctx, h, &jo, nullptr, part.data(), nullptr, 0, jr));
    write_part_file(path, nullptr, k, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

void ek_kway_jet_default_opts(ek_kway_jet_opts* o) {
    if (!o) return;
    o->k = 2;
    o->max_iters = 0;
    o->patience = 12;
    o->neg_num = 1;
    o->neg_den = 4;
    o->pad = 0;
    o->imbalance = 0.03;
}

int ek_kway_jet_host(const ek_hgr* h, const ek_kway_jet_opts* opts, const int64_t* bounds, int32_t* part,
                     int64_t* iter_log, int64_t log_iters, ek_kway_jet_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::RefineWInput in;
    const ek_kway_jet_opts o = ek::jet_prepare("ek_kway_jet_host", h, opts, bounds, part, in);
    const int64_t n = h->nodes;
    const int k = o.k;
    const std::vector<int64_t>&net_ptr = in.in.net_ptr, &inc_ptr = in.in.inc_ptr, &L = in.bound;
    const std::vector<int32_t>&pins = in.in.pins, &inc = in.in.inc, &cw = in.cw, &w = in.w;
    const int64_t nets = int64_t(net_ptr.size()) - 1;
    ek_kway_jet_result r{};
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
    std::vector<int32_t> cur(part, part + n);        // the state; part[] holds the snapshot
    std::vector<int64_t> S(m.begin() + 4, m.end());  // the parts' weights of the state
    std::vector<int32_t> phi(es * ks);               // distinct pins of net e in part p
    std::vector<int64_t> gain(ns), cnt(ks);
    std::vector<int32_t> target(ns);
    std::vector<uint8_t> cand(ns), locked(ns, 0), moved(ns);
    std::vector<int64_t> seen(ks, -1);           // the recount: the last stamp that met the part
    int64_t stamp = 0;                           // one per net and recount
    std::vector<std::vector<int32_t>> into(ks);  // passing candidates per target
    // u's proposal is ranked before v's: greater gain, then the smaller id
    auto before = [&](int32_t u, int32_t v) {
        return gain[size_t(u)] != gain[size_t(v)] ? gain[size_t(u)] > gain[size_t(v)] : u < v;
    };
    int64_t best = r.connectivity_w_before, stale = 0, last_accepted = 0;
    while (nets > 0) {
        // Phi(e, p)
        std::fill(phi.begin(), phi.end(), 0);
        for (int64_t e = 0; e < nets; ++e)
            for (int64_t p = net_ptr[size_t(e)]; p < net_ptr[size_t(e) + 1]; ++p)
                ++phi[size_t(e) * ks + size_t(cur[size_t(pins[size_t(p)])])];
        // (a) the proposals: the open part of greatest gain whatever its sign, then the filter
        int64_t candidates = 0;
        for (int64_t v = 0; v < n; ++v) {
            cand[size_t(v)] = 0;
            const int64_t i0 = inc_ptr[size_t(v)], i1 = inc_ptr[size_t(v) + 1];
            if (i1 == i0 || locked[size_t(v)]) continue;
            const int a = cur[size_t(v)];
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
            if (g >= 0 || -g * int64_t(o.neg_den) < int64_t(o.neg_num) * (D - rv)) {
                cand[size_t(v)] = 1;
                gain[size_t(v)] = g;
                target[size_t(v)] = bt;
                ++candidates;
            }
        }
        // (b) the afterburner: every better-ranked candidate on a shared net counts as moved
        int64_t passed = 0;
        for (auto& l : into) l.clear();
        for (int64_t v = 0; v < n; ++v) {
            if (!cand[size_t(v)]) continue;
            const int a = cur[size_t(v)], t = target[size_t(v)];
            int64_t g2 = 0;
            for (int64_t i = inc_ptr[size_t(v)]; i < inc_ptr[size_t(v) + 1]; ++i) {
                const int32_t e = inc[size_t(i)];
                bool in_a = false, in_t = false;
                for (int64_t p = net_ptr[size_t(e)]; p < net_ptr[size_t(e) + 1]; ++p) {
                    const int32_t u = pins[size_t(p)];
                    if (u == int32_t(v)) continue;
                    const int pu = cand[size_t(u)] && before(u, int32_t(v)) ? target[size_t(u)] : cur[size_t(u)];
                    in_a |= pu == a;
                    in_t |= pu == t;
                }
                g2 += int64_t(cw[size_t(e)]) * (int(!in_a) - int(!in_t));
            }
            if (g2 >= 0) {
                into[size_t(t)].push_back(int32_t(v));
                ++passed;
            }
        }
        // (c) per part: rank order; the longest prefix that fits, not a greedy skip
        int64_t accepted = 0;
        for (int b = 0; b < k; ++b) {
            auto& l = into[size_t(b)];
            std::sort(l.begin(), l.end(), before);
            const int64_t room = L[size_t(b)] - S[size_t(b)];
            int64_t acc = 0;
            size_t take = 0;
            while (take < l.size() && acc + w[size_t(l[take])] <= room) acc += w[size_t(l[take++])];
            l.resize(take);
            accepted += int64_t(take);
        }
        // (d) the moves; exactly the moved nodes are locked during the next iteration
        std::fill(moved.begin(), moved.end(), 0);
        for (int b = 0; b < k; ++b)
            for (int32_t v : into[size_t(b)]) {
                S[size_t(cur[size_t(v)])] -= w[size_t(v)];
                S[size_t(b)] += w[size_t(v)];
                cur[size_t(v)] = b;
                moved[size_t(v)] = 1;
            }
        locked.swap(moved);
        // (e) the objective, recounted over the prepared nets
        int64_t X = 0;
        for (int64_t e = 0; e < nets; ++e) {
            int64_t lambda = 0;
            ++stamp;
            for (int64_t p = net_ptr[size_t(e)]; p < net_ptr[size_t(e) + 1]; ++p) {
                const size_t q = size_t(cur[size_t(pins[size_t(p)])]);
                if (seen[q] != stamp) {
                    seen[q] = stamp;
                    ++lambda;
                }
            }
            X += int64_t(cw[size_t(e)]) * (lambda - 1);
        }
        if (iter_log && r.iters < log_iters) {
            int64_t* row = iter_log + 4 * int64_t(r.iters);
            row[0] = candidates;
            row[1] = passed;
            row[2] = accepted;
            row[3] = X;
        }
        if (r.iters == INT32_MAX) ek::fail(EK_EINVAL, "ek_kway_jet_host: 2^31 iterations");
        ++r.iters;
        r.moves += accepted;
        if (X < best) {
            best = X;
            r.best_iter = r.iters;
            std::copy(cur.begin(), cur.end(), part);
            stale = 0;
        } else {
            ++stale;
        }
        // (f)
        const bool idle = accepted == 0 && last_accepted == 0;
        last_accepted = accepted;
        if (stale == o.patience || (o.max_iters > 0 && r.iters == o.max_iters) || idle) break;
    }
    r.t_iters = since(tr);

    const auto tm = clk::now();
    chk(ek_kway_metrics_w_host(h, part, k, m.data()));
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.connectivity_w = m[2];
    r.soed = m[3];
    r.part_w_min = *std::min_element(m.begin() + 4, m.end());
    r.part_w_max = *std::max_element(m.begin() + 4, m.end());
    for (int p = 0; p < k; ++p) r.parts_over_bound += m[size_t(4 + p)] > L[size_t(p)];
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
