// Sweep cut of a Fiedler vector under a balance tolerance: the host pieces.
//
// ek_sweep_cut_host is the checker of the device path (ek_sweep_cut,
// ctx_sweep.cpp + kernels_sweep.hip).  It is single-threaded and written from
// the rule (eigkl.h), not from the kernels: a std::sort on
// (key, id) where the device runs a radix sort, one loop over each net's pins,
// a difference array and one linear pass with 128-bit products where the
// device reduces with two 64-bit words.  The two share only the argument
// checks and the window (sweep_check, sweep_window).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
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

// the radix order of the device select (ord_key, kway.cpp)
inline uint64_t ord_key(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
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

    // 1. order: ascending (ord(v[i]), i); the keys are compared, never the doubles
    auto t = clk::now();
    std::vector<std::pair<uint64_t, int32_t>> keyed(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) keyed[size_t(i)] = {ord_key(v[i]), int32_t(i)};
    std::sort(keyed.begin(), keyed.end());
    std::vector<int32_t> pos(static_cast<size_t>(n));
    for (int64_t rnk = 0; rnk < n; ++rnk) pos[size_t(keyed[size_t(rnk)].second)] = int32_t(rnk);
    r.t_sort = since(t);

    // 2. profile: +1 at lo + 1, -1 at hi + 1, an inclusive prefix sum
    t = clk::now();
    std::vector<int64_t> prof(static_cast<size_t>(n) + 1, 0);
    for (int64_t e = 0; e < h->nets; ++e) {
        const int64_t p0 = h->net_ptr[size_t(e)], p1 = h->net_ptr[size_t(e) + 1];
        if (p1 - p0 < 2) continue;
        int32_t lo = INT32_MAX, hi = -1;
        for (int64_t p = p0; p < p1; ++p) {
            const int32_t x = pos[size_t(h->pins[size_t(p)])];
            lo = std::min(lo, x);
            hi = std::max(hi, x);
        }
        if (lo == hi) continue;
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

}  // extern "C"
