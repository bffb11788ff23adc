// Coarsening by multi-node clustering, the host piece: ek_cluster_host, the
// checker of the device path (ek_cluster, ctx_cluster.cpp +
// kernels_cluster.hip).  It is written from the rule (eigkl.h),
// one plain loop per step of a round, not from the kernels.  The two share
// only what is input: the matching's argument checks and the participating
// nets with their weights (match_check).
#include <algorithm>
#include <chrono>
#include <vector>

#include "ek_internal.hpp"

namespace {
using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }
}  // namespace

extern "C" {

int ek_cluster_host(const ek_hgr* h, const ek_match_opts* opts, int32_t* rep_out, int32_t* cluster_out,
                    int64_t* round_log, int64_t log_rounds, ek_cluster_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::WeightedInput wi;
    const ek_match_opts o = ek::match_check("ek_cluster_host", h, opts, wi);
    const ek::RefineInput& in = wi.in;
    const int64_t n = h->nodes, nets = int64_t(in.net_ptr.size()) - 1;
    ek_cluster_result r{};
    r.n = n;
    std::vector<int64_t> score(static_cast<size_t>(nets), -1);  // -1: not eligible
    for (int64_t e = 0; e < nets; ++e) {
        const int64_t size = in.net_ptr[size_t(e) + 1] - in.net_ptr[size_t(e)];
        if (size > o.max_net) continue;
        score[size_t(e)] = (int64_t(wi.cw[size_t(e)]) << 20) / (size - 1);
        ++r.eligible_nets;
    }
    r.t_setup = since(t0);

    const auto tr = clk::now();
    const size_t N = static_cast<size_t>(n);
    std::vector<int32_t> rep(N), t(N);
    std::vector<int64_t> S(N), sigma(N);
    std::vector<uint8_t> grown(N, 0), inc(N), mover(N);
    for (int64_t v = 0; v < n; ++v) {
        rep[size_t(v)] = int32_t(v);
        S[size_t(v)] = wi.w[size_t(v)];
    }
    std::vector<std::pair<int32_t, int32_t>> order;  // (destination, mover)
    std::vector<int32_t> accepted;
    for (;;) {
        if (o.max_rounds > 0 && r.rounds >= o.max_rounds) break;
        // 1. propose
        int64_t proposers = 0;
        for (int64_t u = 0; u < n; ++u) {
            t[size_t(u)] = -1;
            sigma[size_t(u)] = -1;
            if (rep[size_t(u)] != u || grown[size_t(u)]) continue;
            for (int64_t i = in.inc_ptr[size_t(u)]; i < in.inc_ptr[size_t(u) + 1]; ++i) {
                const int32_t e = in.inc[size_t(i)];
                const int64_t s = score[size_t(e)];
                if (s < 0) continue;
                for (int64_t q = in.net_ptr[size_t(e)]; q < in.net_ptr[size_t(e) + 1]; ++q) {
                    const int32_t v = in.pins[size_t(q)];
                    if (v == u) continue;
                    const int32_t root = rep[size_t(v)];
                    if (S[size_t(root)] + wi.w[size_t(u)] > o.max_cluster) continue;
                    if (s > sigma[size_t(u)] || (s == sigma[size_t(u)] && root < t[size_t(u)])) {
                        sigma[size_t(u)] = s;
                        t[size_t(u)] = root;
                    }
                }
            }
            proposers += t[size_t(u)] >= 0;
        }
        // 2. incoming
        std::fill(inc.begin(), inc.end(), uint8_t(0));
        for (int64_t u = 0; u < n; ++u)
            if (t[size_t(u)] >= 0) inc[size_t(t[size_t(u)])] = 1;
        // 3. resolve
        auto ml = [&](int64_t x) {  // the larger id of a mutual pair
            const int32_t z = t[size_t(x)];
            return z >= 0 && t[size_t(z)] == x && x > z;
        };
        order.clear();
        for (int64_t u = 0; u < n; ++u) {
            const int32_t dst = t[size_t(u)];
            mover[size_t(u)] = dst >= 0 && (!inc[size_t(u)] || ml(u)) && !ml(dst);
            if (mover[size_t(u)]) order.emplace_back(dst, int32_t(u));
        }
        // 4. accept: per destination the longest fitting prefix of (score descending, id ascending)
        std::sort(order.begin(), order.end(), [&](const auto& a, const auto& b) {
            if (a.first != b.first) return a.first < b.first;
            if (sigma[size_t(a.second)] != sigma[size_t(b.second)]) return sigma[size_t(a.second)] > sigma[size_t(b.second)];
            return a.second < b.second;
        });
        accepted.clear();
        int64_t sum = 0;
        for (size_t i = 0; i < order.size(); ++i) {
            if (i == 0 || order[i].first != order[i - 1].first) sum = 0;
            sum += wi.w[size_t(order[i].second)];
            if (sum <= o.max_cluster - S[size_t(order[i].first)]) accepted.push_back(order[i].second);
        }
        if (accepted.empty()) break;
        // 5. apply
        for (const int32_t u : accepted) {
            const int32_t root = t[size_t(u)];
            rep[size_t(u)] = root;
            S[size_t(root)] += wi.w[size_t(u)];
            grown[size_t(u)] = grown[size_t(root)] = 1;
        }
        if (round_log && r.rounds < log_rounds) {
            round_log[3 * int64_t(r.rounds)] = proposers;
            round_log[3 * int64_t(r.rounds) + 1] = int64_t(order.size());
            round_log[3 * int64_t(r.rounds) + 2] = int64_t(accepted.size());
        }
        ++r.rounds;
        r.joins += int64_t(accepted.size());
    }
    // roots in ascending id order
    int32_t roots = 0;
    std::vector<int32_t> rank(N), cluster(N);
    for (int64_t v = 0; v < n; ++v)
        if (rep[size_t(v)] == v) {
            rank[size_t(v)] = roots++;
            r.heaviest = std::max(r.heaviest, S[size_t(v)]);
        }
    for (int64_t v = 0; v < n; ++v) cluster[size_t(v)] = rank[size_t(rep[size_t(v)])];
    r.n_coarse = roots;
    r.t_rounds = since(tr);
    if (rep_out) std::copy(rep.begin(), rep.end(), rep_out);
    if (cluster_out) std::copy(cluster.begin(), cluster.end(), cluster_out);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
