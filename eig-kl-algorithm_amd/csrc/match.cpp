// Coarsening, the host pieces: the heavy-edge matching's checker and the
// contraction of a hypergraph along a cluster map.
//
// ek_match_host is the checker of the device path (ek_match, ctx_match.cpp +
// kernels_match.hip).  It is written from the rule (eigkl.h),
// one plain loop per step of a round, not from the kernels.  The two share
// only what is input: the argument checks and the participating nets with
// their weights (match_check).  ek_hgr_contract is what the device contraction
// (ek_hgr_contract_device, ctx_contract.cpp) must equal byte for byte.
#include <algorithm>
#include <chrono>
#include <memory>
#include <unordered_map>
#include <vector>

#include "ek_internal.hpp"

namespace {
using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }
}  // namespace

namespace ek {

ek_match_opts match_check(const char* who, const ek_hgr* h, const ek_match_opts* opts, WeightedInput& in) {
    ek_match_opts o;
    ek_match_default_opts(&o);
    if (opts) o = *opts;
    if (!h) fail(EK_EINVAL, "%s: null argument", who);
    if (o.max_net < 2) o.max_net = 2;
    if (o.max_cluster < 1) fail(EK_EINVAL, "%s: max_cluster %lld (at least 1)", who, (long long)o.max_cluster);
    if (h->nodes > INT32_MAX - 1) fail(EK_EINVAL, "%s: %lld nodes", who, (long long)h->nodes);
    weights_prepare(who, h, in);
    return o;
}

}  // namespace ek

extern "C" {

void ek_match_default_opts(ek_match_opts* o) {
    if (!o) return;
    o->max_net = 64;
    o->max_rounds = 8;
    o->max_cluster = 2;
}

int ek_match_host(const ek_hgr* h, const ek_match_opts* opts, int32_t* mate_out, int32_t* cluster_out,
                  int64_t* round_log, int64_t log_rounds, ek_match_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    ek::WeightedInput wi;
    const ek_match_opts o = ek::match_check("ek_match_host", h, opts, wi);
    const ek::RefineInput& in = wi.in;
    const int64_t n = h->nodes, nets = int64_t(in.net_ptr.size()) - 1;
    ek_match_result r{};
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
    std::vector<int32_t> mate(static_cast<size_t>(n), -1), p(static_cast<size_t>(n));
    for (;;) {
        if (o.max_rounds > 0 && r.rounds >= o.max_rounds) break;
        int64_t proposers = 0, pairs = 0;
        for (int64_t u = 0; u < n; ++u) {
            p[size_t(u)] = -1;
            if (mate[size_t(u)] >= 0) continue;
            int64_t best = -1;
            for (int64_t i = in.inc_ptr[size_t(u)]; i < in.inc_ptr[size_t(u) + 1]; ++i) {
                const int32_t e = in.inc[size_t(i)];
                const int64_t s = score[size_t(e)];
                if (s < 0) continue;
                for (int64_t q = in.net_ptr[size_t(e)]; q < in.net_ptr[size_t(e) + 1]; ++q) {
                    const int32_t v = in.pins[size_t(q)];
                    if (v == u || mate[size_t(v)] >= 0) continue;
                    if (int64_t(wi.w[size_t(u)]) + wi.w[size_t(v)] > o.max_cluster) continue;
                    if (s > best || (s == best && v < p[size_t(u)])) {
                        best = s;
                        p[size_t(u)] = v;
                    }
                }
            }
            proposers += p[size_t(u)] >= 0;
        }
        for (int64_t u = 0; u < n; ++u) {
            const int32_t v = p[size_t(u)];
            if (v > u && p[size_t(v)] == u) {
                mate[size_t(u)] = v;
                mate[size_t(v)] = int32_t(u);
                ++pairs;
            }
        }
        if (pairs == 0) break;
        if (round_log && r.rounds < log_rounds) {
            round_log[2 * int64_t(r.rounds)] = proposers;
            round_log[2 * int64_t(r.rounds) + 1] = pairs;
        }
        ++r.rounds;
        r.pairs += pairs;
    }
    // leaders in ascending id order
    int32_t leaders = 0;
    std::vector<int32_t> cluster(static_cast<size_t>(n));
    for (int64_t v = 0; v < n; ++v) {
        const int32_t m = mate[size_t(v)];
        cluster[size_t(v)] = m >= 0 && m < v ? cluster[size_t(m)] : leaders++;
    }
    r.n_coarse = leaders;
    r.t_rounds = since(tr);
    if (mate_out) std::copy(mate.begin(), mate.end(), mate_out);
    if (cluster_out) std::copy(cluster.begin(), cluster.end(), cluster_out);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_hgr_contract(const ek_hgr* h, const int32_t* cluster, int64_t n_coarse, ek_hgr** out) {
    EK_TRY
    if (!h || !out || (h->nodes > 0 && !cluster)) ek::fail(EK_EINVAL, "ek_hgr_contract: null argument");
    const int64_t n = h->nodes;
    if (n_coarse < 0 || n_coarse > n) ek::fail(EK_EINVAL, "ek_hgr_contract: %lld clusters of %lld nodes", (long long)n_coarse, (long long)n);
    auto c = std::make_unique<ek_hgr>();
    c->nodes = n_coarse;
    std::vector<int64_t> wsum(static_cast<size_t>(n_coarse), 0);
    std::vector<uint8_t> hit(static_cast<size_t>(n_coarse), 0);
    for (int64_t v = 0; v < n; ++v) {
        const int32_t k = cluster[v];
        if (k < 0 || k >= n_coarse)
            ek::fail(EK_EINVAL, "ek_hgr_contract: cluster %d of node %lld outside [0, %lld)", k, (long long)v, (long long)n_coarse);
        hit[size_t(k)] = 1;
        wsum[size_t(k)] += h->node_w.empty() ? 1 : h->node_w[size_t(v)];
    }
    c->node_w.resize(size_t(n_coarse));
    for (int64_t k = 0; k < n_coarse; ++k) {
        if (!hit[size_t(k)]) ek::fail(EK_EINVAL, "ek_hgr_contract: no node maps to cluster %lld", (long long)k);
        if (wsum[size_t(k)] > INT32_MAX)
            ek::fail(EK_EINVAL, "ek_hgr_contract: cluster %lld weighs %lld (at most 2^31 - 1)", (long long)k, (long long)wsum[size_t(k)]);
        c->node_w[size_t(k)] = int32_t(wsum[size_t(k)]);
    }
    // A net's identity is its sorted pin set; the table maps a hash of it to
    // the kept nets with that hash, each compared pin by pin.
    std::vector<int64_t> ptr(1, 0), csum;     // the kept nets: pins in first-occurrence order, summed weights
    std::vector<int32_t> pins, sorted, scratch;
    std::vector<int64_t> sptr(1, 0);          // the same nets' sorted pins
    std::unordered_multimap<uint64_t, int64_t> seen;
    std::vector<int64_t> stamp(static_cast<size_t>(n_coarse), -1);  // the last net that listed the cluster
    for (int64_t e = 0; e < h->nets; ++e) {
        const size_t first = pins.size();
        for (int64_t p = h->net_ptr[size_t(e)]; p < h->net_ptr[size_t(e) + 1]; ++p) {
            const int32_t k = cluster[h->pins[size_t(p)]];
            if (stamp[size_t(k)] == e) continue;
            stamp[size_t(k)] = e;
            pins.push_back(k);
        }
        const size_t size = pins.size() - first;
        if (size < 2) {
            pins.resize(first);
            continue;
        }
        scratch.assign(pins.begin() + int64_t(first), pins.end());
        std::sort(scratch.begin(), scratch.end());
        uint64_t hash = 1469598103934665603ull;  // FNV-1a over the sorted pins
        for (int32_t k : scratch) hash = (hash ^ uint64_t(uint32_t(k))) * 1099511628211ull;
        const int64_t ce = h->net_w.empty() ? 1 : h->net_w[size_t(e)];
        int64_t same = -1;
        const auto range = seen.equal_range(hash);
        for (auto it = range.first; it != range.second && same < 0; ++it) {
            const int64_t f = it->second;
            if (size_t(sptr[size_t(f) + 1] - sptr[size_t(f)]) == size &&
                std::equal(scratch.begin(), scratch.end(), sorted.begin() + sptr[size_t(f)]))
                same = f;
        }
        if (same >= 0) {
            csum[size_t(same)] += ce;
            pins.resize(first);
            continue;
        }
        seen.emplace(hash, int64_t(csum.size()));
        csum.push_back(ce);
        ptr.push_back(int64_t(pins.size()));
        sorted.insert(sorted.end(), scratch.begin(), scratch.end());
        sptr.push_back(int64_t(sorted.size()));
    }
    c->nets = int64_t(csum.size());
    c->net_ptr.assign(ptr.begin(), ptr.end());
    c->pins.assign(pins.begin(), pins.end());
    c->net_w.resize(csum.size());
    for (size_t e = 0; e < csum.size(); ++e) {
        if (csum[e] > INT32_MAX)
            ek::fail(EK_EINVAL, "ek_hgr_contract: merged net %lld weighs %lld (at most 2^31 - 1)", (long long)e, (long long)csum[e]);
        c->net_w[e] = int32_t(csum[e]);
    }
    *out = c.release();
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
