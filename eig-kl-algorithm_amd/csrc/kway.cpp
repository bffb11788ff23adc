// k-way partitioning by recursive spectral bisection (ek_partition_kway) and
// its host-only pieces: the size plan, the rank split, the k-way metrics.
//
// The recursion is depth first, side 0 before side 1, one bisection at a time
// on the one context.  Sibling bisections are NOT run on concurrent streams or
// contexts: the Lanczos launches wait inside the launch for other workgroups
// of their own grid ("in-launch waits"), which holds only while
// that grid is resident, and a second kernel beside them can take the compute
// units the waited-for workgroups need.
//
// Each bisection is solve()'s -EIG path (solve.cpp) on the block's induced
// sub-hypergraph with the rank split in place of the median split: the KL
// adjacency starts on its host thread (kl_graph_host, shared with solve())
// and hides behind the device Laplacian build and the Lanczos solve.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <filesystem>
#include <future>
#include <numeric>
#include <string>
#include <vector>

#include "ek_internal.hpp"

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

void chk(int rc) {
    if (rc != EK_OK) throw ek::Error{rc};  // ek_last_error() already holds the message
}

void plan(int64_t n, int32_t k, int64_t* sizes) {
    if (k == 1) {
        sizes[0] = n;
        return;
    }
    const int32_t kl = (k + 1) / 2, kr = k / 2;
    const int64_t n1 = n * kr / k;
    plan(n - n1, kl, sizes);
    plan(n1, kr, sizes + kl);
}

void check_kn(const char* who, int64_t n, int32_t k) {
    if (k < 2 || k > 256) ek::fail(EK_EINVAL, "%s: k = %d outside [2, 256]", who, int(k));
    if (n < 2 * int64_t(k) || n > INT32_MAX - 1)
        ek::fail(EK_EINVAL, "%s: %lld nodes for k = %d (at least 2 per part)", who, (long long)n, int(k));
}

struct Kway {
    ek_ctx* ctx;
    ek_kway_opts o;
    int32_t* part;
    ek_kway_result r{};
    std::function<ek_ctx*()> get_ctx;

    // h: the block; ids: the original id of each of its nodes (null: the root)
    void bisect(const ek_hgr& h, const int32_t* ids, int32_t k, int32_t base, int level) {
        const auto tb = clk::now();
        const int64_t n = h.nodes;
        const int32_t kl = (k + 1) / 2, kr = k / 2;
        const int64_t n1 = n * kr / k, n0 = n - n1;
        bool edges = false;  // a net of >= 2 pins (an induced block's nets all are)
        for (int64_t e = 0; e < h.nets && !edges; ++e) edges = h.net_ptr[size_t(e) + 1] - h.net_ptr[size_t(e)] >= 2;
        // ek_lanczos_fiedler needs ncv = min(n/2, n - 1) > nev (1 deflated, 2
        // not): below 4 nodes (6 undeflated) it answers EK_EINVAL, "graph too
        // small", which is no EK_ENOCONV, so such a block takes the index split
        const int64_t lanczos_min = o.lanczos.deflate ? 4 : 6;
        bool spectral = edges && n >= std::max<int64_t>(o.min_spectral, lanczos_min);
        std::vector<uint8_t> sides(static_cast<size_t>(n));
        std::future<ek::ThreadStatus> kg;
        if (edges) kg = std::async(std::launch::async, ek::kl_graph_host, &get_ctx, &h, ek::kl_graph_threads(spectral));
        if (spectral) {
            const auto t = clk::now();
            int rc = ek::spmv_setup_hgr(ctx, h, nullptr);
            double lambda = 0.0;
            ek_lanczos_stats st{};
            if (rc == EK_OK) rc = ek_lanczos_fiedler(ctx, &o.lanczos, &lambda, nullptr, &st);
            r.t_lanczos += since(t);
            if (rc == EK_ENOCONV) spectral = false;
            else if (rc != EK_OK) {
                const std::string msg = ek_last_error();
                kg.wait();  // the adjacency thread is using the context
                ek::fail(rc, "%s", msg.c_str());
            } else r.matvecs += st.matvecs;
        }
        const auto t = clk::now();
        if (edges) {
            ek::ThreadStatus st = kg.get();
            if (st.code != EK_OK) ek::fail(st.code, "KL graph setup: %s", st.msg.c_str());
        }
        if (!spectral) {
            // deterministic fallback: the block's first n0 nodes to side 0 (the
            // rank split of the descending node index), so part ids ascend
            // with node ids
            ++r.fallback_splits;
            for (int64_t i = 0; i < n; ++i) sides[size_t(i)] = i >= n0;
            if (edges) chk(ek_kl_set_partition_bits(ctx, n, sides.data()));
        } else {
            chk(ek_kl_set_partition_fiedler_rank(ctx, n1, nullptr, nullptr));
        }
        if (edges) {
            ek_kl_result kr_{};
            chk(ek_kl_run(ctx, o.limit, nullptr, 0, &kr_));
            r.kl_swaps += kr_.iterations;
            chk(ek_kl_sides(ctx, 1, sides.data()));
        }
        r.t_kl += since(t);
        // KL swaps pairs: the planned sizes hold
        const int64_t got1 = std::accumulate(sides.begin(), sides.end(), int64_t(0));
        if (got1 != n1)
            ek::fail(EK_ESTATE, "k-way bisection: side 1 holds %lld nodes, planned %lld", (long long)got1, (long long)n1);
        if (level < EK_KWAY_LEVELS) r.t_level[level] += since(tb);
        for (int s = 0; s < 2; ++s) {
            const int32_t ks = s ? kr : kl, bs = s ? base + kl : base;
            if (ks == 1) {
                for (int64_t i = 0; i < n; ++i)
                    if (sides[size_t(i)] == s) part[ids ? ids[size_t(i)] : i] = bs;
                continue;
            }
            const auto ti = clk::now();
            std::vector<uint8_t> keep(static_cast<size_t>(n));
            for (int64_t i = 0; i < n; ++i) keep[size_t(i)] = sides[size_t(i)] == s;
            ek_hgr* sub = nullptr;
            chk(ek_hgr_induce(&h, keep.data(), &sub, nullptr));
            std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> sg(sub, ek_hgr_free);
            std::vector<int32_t> sid;
            sid.reserve(size_t(s ? n1 : n0));
            for (int64_t i = 0; i < n; ++i)
                if (keep[size_t(i)]) sid.push_back(ids ? ids[size_t(i)] : int32_t(i));
            const double d = since(ti);
            r.t_induce += d;
            if (level + 1 < EK_KWAY_LEVELS) r.t_level[level + 1] += d;
            bisect(*sub, sid.data(), ks, bs, level + 1);
        }
    }
};

void partition(ek_ctx* ctx, const ek_hgr& h, const ek_kway_opts* opts, int32_t* part_out, ek_kway_result* result) {
    const auto t0 = clk::now();
    ek_kway_opts o;
    ek_kway_default_opts(&o);
    if (opts) o = *opts;
    if (o.min_spectral <= 0) o.min_spectral = 32;
    int rank = 0, nranks = 1;
    ek::ctx_ranks(ctx, &rank, &nranks);
    if (nranks > 1) ek::fail(EK_ESTATE, "ek_partition_kway: a multi-rank context (%d ranks); k-way runs on one", nranks);
    check_kn("ek_partition_kway", h.nodes, o.k);
    Kway kw{ctx, o, part_out, ek_kway_result{}, [ctx] { return ctx; }};
    kw.bisect(h, nullptr, o.k, 0, 0);
    ek_kway_result& r = kw.r;
    r.k = o.k;
    r.bisections = o.k - 1;
    std::vector<int64_t> cnt(size_t(o.k), 0);
    for (int64_t i = 0; i < h.nodes; ++i) ++cnt[size_t(part_out[i])];
    r.part_min = *std::min_element(cnt.begin(), cnt.end());
    r.part_max = *std::max_element(cnt.begin(), cnt.end());
    const auto t = clk::now();
    int64_t m[3] = {0, 0, 0};
    chk(ek_kway_metrics(ctx, h.nets, h.net_ptr.data(), h.pins.data(), part_out, o.k, m));
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.soed = m[2];
    r.t_metrics = since(t);
    r.t_total = since(t0);
    if (result) *result = r;
}

}  // namespace

namespace ek {
// `gKL2 <in> -EIG --k N` (cli.cpp refers to it weakly)
int kway_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, ek_kway_result* r);
int kway_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, ek_kway_result* r) {
    ek_kway_opts ko;
    ek_kway_default_opts(&ko);
    ko.k = k;
    ko.write_results = 1;
    if (lanczos) ko.lanczos = *lanczos;
    return ek_partition_kway_file(ctx, path, &ko, nullptr, r);
}

void write_part_file(const char* hgr_path, const char* out_dir, int32_t k, int64_t nodes, const int32_t* part) {
    namespace fs = std::filesystem;
    const fs::path dir = (out_dir && out_dir[0] ? fs::path(out_dir) : fs::path()) / "results";
    std::error_code ec;
    fs::create_directories(dir, ec);
    const std::string out = (dir / (fs::path(hgr_path).filename().string() + ".part." + std::to_string(k))).string();
    std::string text;
    text.reserve(size_t(nodes) * 4);
    for (int64_t i = 0; i < nodes; ++i) text += std::to_string(part[i]) + "\n";
    FILE* f = std::fopen(out.c_str(), "w");
    if (!f) fail(EK_EIO, "Error: Cannot open output file %s (%s)", out.c_str(), std::strerror(errno));
    const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
    if ((std::fclose(f) != 0) || !ok) fail(EK_EIO, "short write to %s", out.c_str());
}
}  // namespace ek

extern "C" {

int ek_kway_plan(int64_t n, int32_t k, int64_t* part_sizes) {
    EK_TRY
    if (!part_sizes) ek::fail(EK_EINVAL, "ek_kway_plan: null argument");
    check_kn("ek_kway_plan", n, k);
    plan(n, k, part_sizes);
    return EK_OK;
    EK_CATCH
}

int ek_rank_split(int64_t n, const double* v, int64_t n1, uint8_t* bits_out) {
    EK_TRY
    if (n <= 0 || !v || !bits_out || n1 < 0 || n1 > n) ek::fail(EK_EINVAL, "ek_rank_split: bad argument");
    if (n1 == 0 || n1 == n) {
        std::memset(bits_out, n1 ? 1 : 0, size_t(n));
        return EK_OK;
    }
    // the key at rank n1 - 1, the keys below it, then the equal keys in id
    // order: the device kernels' steps (kernels_kway.hip)
    std::vector<uint64_t> key(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) key[size_t(i)] = ek::ord_key(v[i]);
    std::vector<uint64_t> tmp(key);
    std::nth_element(tmp.begin(), tmp.begin() + (n1 - 1), tmp.end());
    const uint64_t K = tmp[size_t(n1 - 1)];
    int64_t below = 0;
    for (int64_t i = 0; i < n; ++i) below += key[size_t(i)] < K;
    int64_t need = n1 - below;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t x = key[size_t(i)];
        bits_out[i] = x < K || (x == K && need-- > 0) ? 1 : 0;
    }
    return EK_OK;
    EK_CATCH
}

int ek_kway_metrics_host(int64_t nets, const int64_t* net_ptr, const int32_t* pins, const int32_t* part, int32_t k,
                         int64_t out[3]) {
    EK_TRY
    if (nets < 0 || !net_ptr || !out || k < 1 || k > 256 || (net_ptr[nets] > 0 && (!pins || !part)))
        ek::fail(EK_EINVAL, "ek_kway_metrics_host: bad argument");
    int64_t cut = 0, conn = 0, soed = 0;
    for (int64_t e = 0; e < nets; ++e) {
        uint64_t m[4] = {0, 0, 0, 0};
        for (int64_t p = net_ptr[e]; p < net_ptr[e + 1]; ++p) {
            const int32_t q = part[pins[p]];
            if (q < 0 || q >= k) ek::fail(EK_EINVAL, "ek_kway_metrics_host: part %d of node %d outside [0, %d)", q, pins[p], k);
            m[q >> 6] |= uint64_t(1) << (q & 63);
        }
        const int lambda = __builtin_popcountll(m[0]) + __builtin_popcountll(m[1]) + __builtin_popcountll(m[2]) +
                           __builtin_popcountll(m[3]);
        if (lambda >= 2) {
            ++cut;
            conn += lambda - 1;
            soed += lambda;
        }
    }
    out[0] = cut;
    out[1] = conn;
    out[2] = soed;
    return EK_OK;
    EK_CATCH
}

void ek_kway_default_opts(ek_kway_opts* o) {
    if (!o) return;
    *o = ek_kway_opts{};
    o->k = 2;
    o->min_spectral = 32;
    o->limit = -1;
    o->write_results = 0;
    o->out_dir = nullptr;
    ek_lanczos_default_opts(&o->lanczos);
}

int ek_partition_kway(ek_ctx* ctx, const ek_hgr* h, const ek_kway_opts* opts, int32_t* part_out,
                      ek_kway_result* result) {
    EK_TRY
    if (!ctx || !h || !part_out) ek::fail(EK_EINVAL, "ek_partition_kway: null argument");
    partition(ctx, *h, opts, part_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_partition_kway_file(ek_ctx* ctx, const char* path, const ek_kway_opts* opts, int32_t* part_out,
                           ek_kway_result* result) {
    EK_TRY
    if (!ctx || !path) ek::fail(EK_EINVAL, "ek_partition_kway_file: null argument");
    ek_hgr* h = nullptr;
    chk(ek_hgr_read(path, &h));
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    std::vector<int32_t> own;
    if (!part_out) {
        own.resize(size_t(h->nodes));
        part_out = own.data();
    }
    ek_kway_result r{};
    partition(ctx, *h, opts, part_out, &r);
    if (opts && opts->write_results) ek::write_part_file(path, opts->out_dir, r.k, h->nodes, part_out);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
