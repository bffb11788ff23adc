// The sweep cuts of a Fiedler vector, by net count under a balance tolerance
// and by net weight under a node-weight bound: the host pieces.
//
// ek_sweep_cut_host and ek_sweep_cut_w_host are the checkers of the device
// paths (ek_sweep_cut, ek_sweep_cut_w; ctx_sweep.cpp + kernels_sweep.hip).
// They are single-threaded and written from the rules (eigkl.h, DESIGN.md §10
// and §13), not from the kernels: a std::sort on (key, id) where the device
// runs a radix sort, one loop over each net's pins, difference arrays and
// running sums where the device scans, and linear passes for the choice: with
// 128-bit products where the count sweep's kernels reduce with two 64-bit
// words, and one pass for the window and one for the choice where the weighted
// sweep's run one keyed reduction.  Host and device share only the argument
// checks, the count sweep's window and the weighted sweep's L_max (sweep_check,
// sweep_window, sweepw_check); the two checkers share the order and a net's
// span, which the two rules state in the same words.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
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

using Keyed = std::vector<std::pair<uint64_t, int32_t>>;

// the order: keyed ascending by (ord(v[i]), i), the keys compared, never the
// doubles; pos[keyed[r].second] = r
void order_by_key(const double* v, int64_t n, Keyed& keyed, std::vector<int32_t>& pos) {
    keyed.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) keyed[size_t(i)] = {ek::ord_key(v[i]), int32_t(i)};
    std::sort(keyed.begin(), keyed.end());
    pos.resize(static_cast<size_t>(n));
    for (int64_t rnk = 0; rnk < n; ++rnk) pos[size_t(keyed[size_t(rnk)].second)] = int32_t(rnk);
}

// the least and the greatest rank of net e's pins; false: the net has fewer
// than two pins or all of them at one rank, and is cut by no split
bool net_span(const ek_hgr* h, int64_t e, const std::vector<int32_t>& pos, int32_t& lo, int32_t& hi) {
    const int64_t p0 = h->net_ptr[size_t(e)], p1 = h->net_ptr[size_t(e) + 1];
    if (p1 - p0 < 2) return false;
    lo = INT32_MAX, hi = -1;
    for (int64_t p = p0; p < p1; ++p) {
        const int32_t x = pos[size_t(h->pins[size_t(p)])];
        lo = std::min(lo, x);
        hi = std::max(hi, x);
    }
    return lo != hi;
}
// what the weighted sweep's steps leave, under either bound form
struct SweepWCore {
    int64_t n0 = 0, n1 = 0, s_lo = 0, s_hi = 0, feasible = 0, w0 = 0, w1 = 0, cut = 0, cut_nets = 0, cut_half = 0,
            spanning_nets = 0;
    double t_sort = 0.0, t_profile = 0.0, t_select = 0.0;
    template <class R>
    void store(R& r) const {
        r.n0 = n0, r.n1 = n1, r.s_lo = s_lo, r.s_hi = s_hi, r.feasible = feasible, r.w0 = w0, r.w1 = w1, r.cut = cut;
        r.cut_nets = cut_nets, r.cut_half = cut_half, r.spanning_nets = spanning_nets;
        r.t_sort = t_sort, r.t_profile = t_profile, r.t_select = t_select;
    }
};

// Steps 1-5 of the weighted rule (§13) under the per-side bounds of §16: side 1
// of split s may weigh at most l1, side 0 at most l0, and the balance key is
// the slack difference |(W - P - l0) - (P - l1)| = |2 P - W + (l0 - l1)|.  With
// l0 = l1 = L_max this is §13 word for word.
void sweepw_host_core(const ek_hgr* h, const double* v, int64_t W, int64_t l0, int64_t l1, int32_t* order_out,
                      int64_t* profile_out, int64_t* prefix_out, SweepWCore& r) {
    const int64_t n = h->nodes;

    // 1. order
    auto t = clk::now();
    Keyed keyed;
    std::vector<int32_t> pos;
    order_by_key(v, n, keyed, pos);
    r.t_sort = since(t);

    // 2. the weighted and the count profile: +c / +1 at lo + 1, -c / -1 at hi + 1, inclusive prefix sums
    // 3. P[s]: the running sum of w(order[r])
    t = clk::now();
    std::vector<int64_t> profw(static_cast<size_t>(n) + 1, 0), prof(static_cast<size_t>(n) + 1, 0),
        prefix(static_cast<size_t>(n) + 1, 0);
    for (int64_t e = 0; e < h->nets; ++e) {
        int32_t lo = 0, hi = 0;
        if (!net_span(h, e, pos, lo, hi)) continue;
        const int64_t c = h->net_w.empty() ? 1 : h->net_w[size_t(e)];
        ++r.spanning_nets;
        profw[size_t(lo) + 1] += c;
        profw[size_t(hi) + 1] -= c;
        ++prof[size_t(lo) + 1];
        --prof[size_t(hi) + 1];
    }
    for (int64_t s = 1; s <= n; ++s) {
        profw[size_t(s)] += profw[size_t(s) - 1];
        prof[size_t(s)] += prof[size_t(s) - 1];
        const int32_t node = keyed[size_t(s) - 1].second;
        prefix[size_t(s)] = prefix[size_t(s) - 1] + (h->node_w.empty() ? 1 : h->node_w[size_t(node)]);
    }
    r.t_profile = since(t);

    // 4. the window; 5. the choice.  |2 P - W + (l0 - l1)| <= 2 W <= 2^63: 128 bits hold every step
    t = clk::now();
    auto dist = [&](int64_t s) {
        const __int128 x = 2 * __int128(prefix[size_t(s)]) - W + (l0 - l1);
        return uint64_t(x < 0 ? -x : x);
    };
    auto is_feasible = [&](int64_t s) { return prefix[size_t(s)] <= l1 && W - prefix[size_t(s)] <= l0; };
    for (int64_t s = 1; s <= n - 1; ++s)
        if (is_feasible(s)) {
            if (!r.feasible) r.s_lo = s;
            r.s_hi = s;
            r.feasible = 1;
        }
    int64_t best = r.feasible ? r.s_lo : 1;
    if (r.feasible) {
        for (int64_t s = r.s_lo + 1; s <= r.s_hi; ++s) {  // least (profile_w, D, s): a later s only when strictly less
            if (profw[size_t(s)] != profw[size_t(best)] ? profw[size_t(s)] < profw[size_t(best)] : dist(s) < dist(best))
                best = s;
        }
    } else {
        for (int64_t s = 2; s <= n - 1; ++s) {  // least (D, profile_w, s)
            if (dist(s) != dist(best) ? dist(s) < dist(best) : profw[size_t(s)] < profw[size_t(best)]) best = s;
        }
    }
    r.n1 = best;
    r.n0 = n - best;
    r.w1 = prefix[size_t(best)];
    r.w0 = W - r.w1;
    r.cut = profw[size_t(best)];
    r.cut_nets = prof[size_t(best)];
    r.cut_half = profw[size_t(n / 2)];
    r.t_select = since(t);

    if (order_out)
        for (int64_t rnk = 0; rnk < n; ++rnk) order_out[rnk] = keyed[size_t(rnk)].second;
    if (profile_out) std::copy(profw.begin(), profw.end(), profile_out);
    if (prefix_out) std::copy(prefix.begin(), prefix.end(), prefix_out);
}
}  // namespace

namespace ek {

ek_sweep_opts sweep_check(const char* who, const ek_hgr* h, const double* v, const ek_sweep_opts* opts) {
    ek_sweep_opts o;
    ek_sweep_default_opts(&o);
    if (opts) o = *opts;
    if (!h || !v) fail(EK_EINVAL, "%s: null argument", who);
    if (h->nodes < 2 || h->nodes > INT32_MAX - 1) fail(EK_EINVAL, "%s: %lld nodes (2 .. 2^31 - 2)", who, (long long)h->nodes);
    if (h->nets > INT32_MAX) fail(EK_EINVAL, "%s: %lld nets", who, (long long)h->nets);
    if (!std::isfinite(o.imbalance) || o.imbalance < 0.0)
        fail(EK_EINVAL, "%s: imbalance %g (finite and >= 0)", who, o.imbalance);
    if (o.objective != 0 && o.objective != 1)
        fail(EK_EINVAL, "%s: objective %d (0: minimum cut, 1: ratio cut)", who, int(o.objective));
    return o;
}

void sweep_window(int64_t n, double imbalance, ek_sweep_result& r) {
    r.n = n;
    r.max_part = refine_max_part(n, 2, imbalance);
    r.s_lo = std::max<int64_t>(1, n - r.max_part);
    r.s_hi = std::min<int64_t>(n - 1, r.max_part);
}

ek_sweep_opts sweepw_check(const char* who, const ek_hgr* h, const double* v, const ek_sweep_opts* opts,
                           ek_sweep_w_result& r) {
    const ek_sweep_opts o = sweep_check(who, h, v, opts);
    if (o.objective != 0)
        fail(EK_EINVAL, "%s: objective %d (the weighted sweep has the minimum cut only)", who, int(o.objective));
    const int64_t n = h->nodes;
    if (!h->node_w.empty() && int64_t(h->node_w.size()) != n)
        fail(EK_EINVAL, "%s: %lld node weights for %lld nodes", who, (long long)h->node_w.size(), (long long)n);
    if (!h->net_w.empty() && int64_t(h->net_w.size()) != h->nets)
        fail(EK_EINVAL, "%s: %lld net weights for %lld nets", who, (long long)h->net_w.size(), (long long)h->nets);
    int64_t total = h->node_w.empty() ? n : 0, csum = h->net_w.empty() ? h->nets : 0;
    for (const int32_t w : h->node_w) {
        if (w < 0) fail(EK_EINVAL, "%s: node weight %d", who, w);
        total += w;
    }
    for (const int32_t c : h->net_w) {
        if (c < 1) fail(EK_EINVAL, "%s: net weight %d", who, c);
        csum += c;
    }
    // (int32 weights over fewer than 2^31 nodes and nets stay below both limits; the rule states them all the same)
    if (total > W_LIMIT || csum > W_LIMIT) fail(EK_EINVAL, "%s: total weight above 2^62", who);
    r = ek_sweep_w_result{};
    r.n = n;
    r.total_weight = total;
    r.max_part = refine_max_part(total, 2, o.imbalance);
    return o;
}

ek_sweep_opts sweepwb_check(const char* who, const ek_hgr* h, const double* v, const ek_sweep_opts* opts,
                            const int64_t bounds[2], ek_sweep_wb_result& r) {
    ek_sweep_opts o;
    ek_sweep_default_opts(&o);
    if (opts) o = *opts;
    o.imbalance = 0.0;  // ignored: the bounds stand in its place
    ek_sweep_w_result w{};
    sweepw_check(who, h, v, &o, w);
    if (!bounds) fail(EK_EINVAL, "%s: null bounds", who);
    bounds_check(who, w.total_weight, bounds);
    r = ek_sweep_wb_result{};
    r.n = w.n;
    r.total_weight = w.total_weight;
    r.bound0 = bounds[0];
    r.bound1 = bounds[1];
    return o;
}

void bounds_check(const char* who, int64_t W, const int64_t bounds[2]) {
    if (W > (int64_t(1) << 61)) fail(EK_EINVAL, "%s: total weight %lld above 2^61", who, (long long)W);
    for (int s = 0; s < 2; ++s)
        if (bounds[s] < 0 || bounds[s] > W)
            fail(EK_EINVAL, "%s: bound %d = %lld outside [0, W = %lld]", who, s, (long long)bounds[s], (long long)W);
    if (bounds[0] + bounds[1] < W)  // (both at most 2^61: the sum is exact)
        fail(EK_EINVAL, "%s: bounds %lld + %lld below W = %lld", who, (long long)bounds[0], (long long)bounds[1],
             (long long)W);
}

// `gKL2 <in> -EIG --sweep EPS [--sweep-ratio]` (cli.cpp refers to it weakly):
// the file, the Laplacian on the device, Lanczos, the KL graph and nets, the
// sweep split, the KL loop, then the best prefix into results/<base>.part.2
int sweep_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, int32_t limit, double imbalance,
                       int ratio, ek_sweep_result* sr, ek_kl_result* kr, double* lambda, ek_lanczos_stats* st);
int sweep_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, int32_t limit, double imbalance,
                       int ratio, ek_sweep_result* sr, ek_kl_result* kr, double* lambda, ek_lanczos_stats* st) {
    EK_TRY
    if (!ctx || !path || !sr || !kr) fail(EK_EINVAL, "sweep: null argument");
    ek_hgr* h = nullptr;
    chk(ek_hgr_read(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    ek_sweep_opts so;
    ek_sweep_default_opts(&so);
    so.objective = ratio ? 1 : 0;
    so.imbalance = imbalance;
    if (h->nodes < 2) fail(EK_EINVAL, "sweep: %lld nodes", (long long)h->nodes);
    chk(spmv_setup_hgr(ctx, *h, nullptr));
    double lam = 0.0;
    ek_lanczos_stats ls{};
    chk(ek_lanczos_fiedler(ctx, lanczos, &lam, nullptr, &ls));
    if (lambda) *lambda = lam;
    if (st) *st = ls;
    const std::function<ek_ctx*()> get = [ctx] { return ctx; };
    ThreadStatus ts = kl_graph_host(&get, h, kl_graph_threads(false));
    if (ts.code != EK_OK) fail(ts.code, "KL graph setup: %s", ts.msg.c_str());
    chk(ek_kl_set_partition_fiedler_sweep(ctx, h, &so, sr));
    chk(ek_kl_run(ctx, limit, nullptr, 0, kr));
    std::vector<uint8_t> sides(static_cast<size_t>(h->nodes));
    chk(ek_kl_sides(ctx, 1, sides.data()));
    std::vector<int32_t> part(sides.begin(), sides.end());
    write_part_file(path, nullptr, 2, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

// `gKL2 <in> -EIG --sweep EPS --sweep-weighted --fm EPS --weighted [--no-kl]`
// (cli.cpp refers to it weakly): the hMETIS reading of the file, the Laplacian
// on the device, Lanczos, then the weighted sweep split.  With KL: the KL
// graph and nets, the split into the context, the KL loop and the sides of its
// best prefix.  Without: the sides ek_rank_split(v, n1) as they are (KL swaps
// pairs and ignores weights, so it can leave the bound the sweep kept).  Then
// ek_fm_refine_w and results/<base>.part.2.
int sweepw_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, double sweep_eps, int no_kl,
                        double imbalance, int max_passes, int stall, ek_sweep_w_result* sr, ek_kl_result* kr,
                        ek_fm_w_result* fr);
int sweepw_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, double sweep_eps, int no_kl,
                        double imbalance, int max_passes, int stall, ek_sweep_w_result* sr, ek_kl_result* kr,
                        ek_fm_w_result* fr) {
    EK_TRY
    if (!ctx || !path || !so || !sr || !kr || !fr) fail(EK_EINVAL, "sweepw: null argument");
    ek_fm_opts fo;
    ek_fm_default_opts(&fo);
    fo.imbalance = imbalance;
    fo.max_passes = max_passes;
    if (stall >= 0) fo.stall = stall;  // (< 0: the default)
    ek_hgr* h = nullptr;
    chk(ek_hgr_read_weighted(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    if (h->nodes < 2) fail(EK_EINVAL, "sweepw: %lld nodes", (long long)h->nodes);
    ek_sweep_opts wo;
    ek_sweep_default_opts(&wo);
    wo.imbalance = sweep_eps;
    chk(spmv_setup_hgr(ctx, *h, nullptr));
    double lam = 0.0;
    ek_lanczos_stats ls{};
    std::vector<uint8_t> sides(static_cast<size_t>(h->nodes));
    *kr = ek_kl_result{};
    if (no_kl) {
        std::vector<double> v(static_cast<size_t>(h->nodes));
        chk(ek_lanczos_fiedler(ctx, &so->lanczos, &lam, v.data(), &ls));
        chk(ek_sweep_cut_w(ctx, h, v.data(), &wo, nullptr, nullptr, nullptr, sr));
        chk(ek_rank_split(h->nodes, v.data(), sr->n1, sides.data()));
    } else {
        chk(ek_lanczos_fiedler(ctx, &so->lanczos, &lam, nullptr, &ls));
        const std::function<ek_ctx*()> get = [ctx] { return ctx; };
        ThreadStatus ts = kl_graph_host(&get, h, kl_graph_threads(false));
        if (ts.code != EK_OK) fail(ts.code, "KL graph setup: %s", ts.msg.c_str());
        chk(ek_kl_set_partition_fiedler_sweep_w(ctx, h, &wo, sr));
        chk(ek_kl_run(ctx, so->limit, nullptr, 0, kr));
        chk(ek_kl_sides(ctx, 1, sides.data()));
    }
    chk(ek_fm_refine_w(ctx, h, &fo, sides.data(), nullptr, 0, nullptr, 0, fr));
    std::vector<int32_t> part(sides.begin(), sides.end());
    write_part_file(path, nullptr, 2, h->nodes, part.data());
    return EK_OK;
    EK_CATCH
}

}  // namespace ek

extern "C" {

void ek_sweep_default_opts(ek_sweep_opts* o) {
    if (!o) return;
    o->objective = 0;
    o->pad = 0;
    o->imbalance = 0.03;
}

int ek_sweep_cut_host(const ek_hgr* h, const double* v, const ek_sweep_opts* opts, int32_t* order_out,
                      int32_t* profile_out, ek_sweep_result* result) {
    EK_TRY
    const ek_sweep_opts o = ek::sweep_check("ek_sweep_cut_host", h, v, opts);
    const int64_t n = h->nodes;
    ek_sweep_result r{};
    ek::sweep_window(n, o.imbalance, r);

    // 1. order
    auto t = clk::now();
    Keyed keyed;
    std::vector<int32_t> pos;
    order_by_key(v, n, keyed, pos);
    r.t_sort = since(t);

    // 2. profile: +1 at lo + 1, -1 at hi + 1, an inclusive prefix sum
    t = clk::now();
    std::vector<int64_t> prof(static_cast<size_t>(n) + 1, 0);
    for (int64_t e = 0; e < h->nets; ++e) {
        int32_t lo = 0, hi = 0;
        if (!net_span(h, e, pos, lo, hi)) continue;
        ++r.spanning_nets;
        ++prof[size_t(lo) + 1];
        --prof[size_t(hi) + 1];
    }
    for (int64_t s = 1; s <= n; ++s) prof[size_t(s)] += prof[size_t(s) - 1];
    r.t_profile = since(t);

    // 3./4. the window's best split
    t = clk::now();
    auto dist = [n](int64_t s) { return std::llabs(2 * s - n); };
    auto better = [&](int64_t a, int64_t b) {  // a strictly before b
        const int64_t pa = prof[size_t(a)], pb = prof[size_t(b)];
        if (o.objective == 0) {
            if (pa != pb) return pa < pb;
        } else {
            using u128 = unsigned __int128;
            const u128 x = u128(uint64_t(pa)) * uint64_t(b) * uint64_t(n - b);
            const u128 y = u128(uint64_t(pb)) * uint64_t(a) * uint64_t(n - a);
            if (x != y) return x < y;
        }
        if (dist(a) != dist(b)) return dist(a) < dist(b);
        return a < b;
    };
    int64_t best = r.s_lo;
    for (int64_t s = r.s_lo + 1; s <= r.s_hi; ++s)
        if (better(s, best)) best = s;
    r.n1 = best;
    r.n0 = n - best;
    r.cut = prof[size_t(best)];
    r.cut_mid = prof[size_t(n / 2)];
    r.t_select = since(t);

    if (order_out)
        for (int64_t rnk = 0; rnk < n; ++rnk) order_out[rnk] = keyed[size_t(rnk)].second;
    if (profile_out)
        for (int64_t s = 0; s <= n; ++s) profile_out[s] = int32_t(prof[size_t(s)]);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_sweep_cut_w_host(const ek_hgr* h, const double* v, const ek_sweep_opts* opts, int32_t* order_out,
                        int64_t* profile_out, int64_t* prefix_out, ek_sweep_w_result* result) {
    EK_TRY
    ek_sweep_w_result r{};
    ek::sweepw_check("ek_sweep_cut_w_host", h, v, opts, r);
    SweepWCore c;
    sweepw_host_core(h, v, r.total_weight, r.max_part, r.max_part, order_out, profile_out, prefix_out, c);
    c.store(r);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_sweep_cut_wb_host(const ek_hgr* h, const double* v, const ek_sweep_opts* opts, const int64_t bounds[2],
                         int32_t* order_out, int64_t* profile_out, int64_t* prefix_out, ek_sweep_wb_result* result) {
    EK_TRY
    ek_sweep_wb_result r{};
    ek::sweepwb_check("ek_sweep_cut_wb_host", h, v, opts, bounds, r);
    SweepWCore c;
    sweepw_host_core(h, v, r.total_weight, r.bound0, r.bound1, order_out, profile_out, prefix_out, c);
    c.store(r);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
