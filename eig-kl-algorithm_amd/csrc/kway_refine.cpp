// k-way connectivity refinement under a maximum part size: the host pieces.
//
// ek_kway_refine_host is the checker of the device path (ek_kway_refine,
// ctx_kway.cpp + kernels_refine.hip).  It is written from the rule (eigkl.h,
// DESIGN.md §9), one plain loop per step of a round, not from the kernels:
// per-part counters where the device keeps bit masks, a sort where the device
// selects a threshold key.  The two share only what is input, not algorithm:
// L_max (refine_max_part), the participating nets with their distinct pins and
// the node -> net incidence (refine_prepare), and the argument checks.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
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

int64_t refine_max_part(int64_t n, int32_t k, double imbalance) {
    const double x = (1.0 + imbalance) * double((n + k - 1) / k);
    return x >= 9.0e18 ? INT64_MAX : int64_t(std::floor(x));
}

ek_kway_refine_opts refine_check(const char* who, const ek_hgr* h, const ek_kway_refine_opts* opts,
                                 const int32_t* part) {
    ek_kway_refine_opts o;
    ek_kway_refine_default_opts(&o);
    if (opts) o = *opts;
    if (!h || (h->nodes > 0 && !part)) fail(EK_EINVAL, "%s: null argument", who);
    if (o.k < 2 || o.k > 256) fail(EK_EINVAL, "%s: k = %d outside [2, 256]", who, int(o.k));
    if (!std::isfinite(o.imbalance) || o.imbalance < 0.0)
        fail(EK_EINVAL, "%s: imbalance %g (finite and >= 0)", who, o.imbalance);
    if (h->nodes > INT32_MAX - 1) fail(EK_EINVAL, "%s: %lld nodes", who, (long long)h->nodes);
    for (int64_t i = 0; i < h->nodes; ++i)
        if (part[i] < 0 || part[i] >= o.k)
            fail(EK_EINVAL, "%s: part %d of node %lld outside [0, %d)", who, part[i], (long long)i, int(o.k));
    return o;
}

void refine_prepare(const ek_hgr& h, RefineInput& in) {
    const int64_t n = h.nodes;
    in.net_ptr.assign(1, 0);
    in.pins.clear();
    in.pins.reserve(h.pins.size());
    std::vector<int64_t> stamp(size_t(n), -1);  // the last net that listed the node
    for (int64_t e = 0; e < h.nets; ++e) {
        const size_t first = in.pins.size();
        for (int64_t p = h.net_ptr[size_t(e)]; p < h.net_ptr[size_t(e) + 1]; ++p) {
            const int32_t v = h.pins[size_t(p)];
            if (stamp[size_t(v)] == e) continue;
            stamp[size_t(v)] = e;
            in.pins.push_back(v);
        }
        if (in.pins.size() - first >= 2) in.net_ptr.push_back(int64_t(in.pins.size()));
        else in.pins.resize(first);
    }
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    if (nets > INT32_MAX - 1) fail(EK_EINVAL, "k-way refinement: %lld nets", (long long)nets);
    in.inc_ptr.assign(size_t(n) + 1, 0);
    for (int32_t v : in.pins) ++in.inc_ptr[size_t(v) + 1];
    for (int64_t v = 0; v < n; ++v) in.inc_ptr[size_t(v) + 1] += in.inc_ptr[size_t(v)];
    in.inc.resize(in.pins.size());
    std::vector<int64_t> at(in.inc_ptr.begin(), in.inc_ptr.end() - 1);
    for (int64_t e = 0; e < nets; ++e)
        for (int64_t p = in.net_ptr[size_t(e)]; p < in.net_ptr[size_t(e) + 1]; ++p)
            in.inc[size_t(at[size_t(in.pins[size_t(p)])]++)] = int32_t(e);
}

// `gKL2 <in> -EIG --k N --refine EPS` (cli.cpp refers to it weakly): the
// partition, the refinement on the device, then results/<base>.part.<N>
int kway_refine_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int max_rounds, ek_kway_result* kr, ek_kway_refine_result* rr);
int kway_refine_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int max_rounds, ek_kway_result* kr, ek_kway_refine_result* rr) {
    EK_TRY
    ek_hgr* h = nullptr;
    chk(ek_hgr_read(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    ek_kway_opts ko;
    ek_kway_default_opts(&ko);
    ko.k = k;
    if (lanczos) ko.lanczos = *lanczos;
    ek_kway_refine_opts ro;
    ek_kway_refine_default_opts(&ro);
    ro.k = k;
    ro.imbalance = imbalance;
    ro.max_rounds = max_rounds;
    if (!std::isfinite(imbalance) || imbalance < 0.0) fail(EK_EINVAL, "--refine takes an imbalance >= 0");
    std::vector<int32_t> part(size_t(h->nodes));
    chk(ek_partition_kway(ctx, h, &ko, part.data(), kr));
    chk(ek_kway_refine(ctx, h, &ro, part.data(), nullptr, 0, rr));
    write_part_file(path, nullptr, k, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

void ek_kway_refine_default_opts(ek_kway_refine_opts* o) {
    if (!o) return;
    o->k = 2;
    o->max_rounds = 0;
    o->imbalance = 0.03;
}

int ek_kway_refine_host(const ek_hgr* h, const ek_kway_refine_opts* opts, int32_t* part, int64_t* round_log,
                        int64_t log_rounds, ek_kway_refine_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    const ek_kway_refine_opts o = ek::refine_check("ek_kway_refine_host", h, opts, part);
    const int64_t n = h->nodes;
    const int k = o.k;
    ek::RefineInput in;
    ek::refine_prepare(*h, in);
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    ek_kway_refine_result r{};
    r.k = k;
    r.max_part = ek::refine_max_part(n, k, o.imbalance);
    int64_t m[3];
    chk(ek_kway_metrics_host(nets, in.net_ptr.data(), in.pins.data(), part, k, m));
    r.connectivity_before = m[1];
    r.t_setup = since(t0);

    const auto tr = clk::now();
    const size_t ks = size_t(k), ns = size_t(n), es = size_t(nets);
    std::vector<int64_t> size(ks, 0);
    for (int64_t v = 0; v < n; ++v) ++size[size_t(part[v])];
    std::vector<int32_t> phi(es * ks);  // pins of net e in part p
    std::vector<int64_t> gain(ns), cnt(ks);
    std::vector<int32_t> target(ns), winner(es);
    std::vector<std::vector<int32_t>> into(ks);  // independent candidates per target
    for (;;) {
        if (o.max_rounds > 0 && r.rounds >= o.max_rounds) break;
        // Phi(e, p)
        std::fill(phi.begin(), phi.end(), 0);
        for (int64_t e = 0; e < nets; ++e)
            for (int64_t p = in.net_ptr[size_t(e)]; p < in.net_ptr[size_t(e) + 1]; ++p)
                ++phi[size_t(e) * size_t(k) + size_t(part[in.pins[size_t(p)]])];
        // targets and gains; gain 0: not a candidate
        int64_t candidates = 0;
        for (int64_t v = 0; v < n; ++v) {
            gain[size_t(v)] = 0;
            const int64_t i0 = in.inc_ptr[size_t(v)], i1 = in.inc_ptr[size_t(v) + 1], deg = i1 - i0;
            if (deg == 0) continue;
            const int a = part[v];
            int64_t rv = 0;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t i = i0; i < i1; ++i) {
                const int32_t* f = &phi[size_t(in.inc[size_t(i)]) * size_t(k)];
                rv += f[a] == 1;
                for (int b = 0; b < k; ++b) cnt[size_t(b)] += f[b] > 0;
            }
            int64_t best = 0;
            int bt = -1;
            for (int b = 0; b < k; ++b) {
                if (b == a || size[size_t(b)] >= r.max_part) continue;
                const int64_t g = rv + cnt[size_t(b)] - deg;
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
            int32_t w = -1;
            for (int64_t p = in.net_ptr[size_t(e)]; p < in.net_ptr[size_t(e) + 1]; ++p) {
                const int32_t v = in.pins[size_t(p)];
                if (gain[size_t(v)] <= 0) continue;
                if (w < 0 || gain[size_t(v)] > gain[size_t(w)] || (gain[size_t(v)] == gain[size_t(w)] && v < w)) w = v;
            }
            winner[size_t(e)] = w;
        }
        // the independent candidates, by target
        int64_t independent = 0;
        for (auto& l : into) l.clear();
        for (int64_t v = 0; v < n; ++v) {
            if (gain[size_t(v)] <= 0) continue;
            bool all = true;
            for (int64_t i = in.inc_ptr[size_t(v)]; i < in.inc_ptr[size_t(v) + 1] && all; ++i)
                all = winner[size_t(in.inc[size_t(i)])] == int32_t(v);
            if (all) {
                into[size_t(target[size_t(v)])].push_back(int32_t(v));
                ++independent;
            }
        }
        // per part: gain descending, id ascending, while there is room
        int64_t accepted = 0, G = 0;
        for (int b = 0; b < k; ++b) {
            auto& l = into[size_t(b)];
            std::sort(l.begin(), l.end(), [&](int32_t x, int32_t y) {
                return gain[size_t(x)] != gain[size_t(y)] ? gain[size_t(x)] > gain[size_t(y)] : x < y;
            });
            const int64_t room = std::max<int64_t>(r.max_part - size[size_t(b)], 0);
            if (int64_t(l.size()) > room) l.resize(size_t(room));
            for (int32_t v : l) G += gain[size_t(v)];
            accepted += int64_t(l.size());
        }
        if (accepted == 0) break;
        for (int b = 0; b < k; ++b)
            for (int32_t v : into[size_t(b)]) {
                --size[size_t(part[v])];
                ++size[size_t(b)];
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
    r.part_min = *std::min_element(size.begin(), size.end());
    r.part_max = *std::max_element(size.begin(), size.end());
    chk(ek_kway_metrics_host(nets, in.net_ptr.data(), in.pins.data(), part, k, m));
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.soed = m[2];
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
