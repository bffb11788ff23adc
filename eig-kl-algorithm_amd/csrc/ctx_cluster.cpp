// The clustering entry of libeigkl_hip.so (ek_cluster; kernels_cluster.hip).
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

// The launches of a round, then ONE 8-byte read (the round's joins) to learn
// whether to go on.  The rounds' three counters stay in a device log of CL_LOG
// rounds, read in bulk when it is full and at the end.  Every buffer is local
// to the call: the context keeps nothing.
int ek_cluster(ek_ctx* c, const ek_hgr* h, const ek_match_opts* opts, int32_t* rep_out, int32_t* cluster_out,
               int64_t* round_log, int64_t log_rounds, ek_cluster_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "ek_cluster: a multi-rank context (%d ranks); the clustering runs on one", c->nranks);
    ek::WeightedInput wi;
    const ek_match_opts o = ek::match_check("ek_cluster", h, opts, wi);
    const ek::RefineInput& in = wi.in;
    const int64_t n = h->nodes, nets = int64_t(in.net_ptr.size()) - 1;
    ek_cluster_result r{};
    r.n = r.n_coarse = n;
    if (nets == 0) {  // nothing to join along: every node its own cluster
        for (int64_t v = 0; v < n; ++v) {
            if (rep_out) rep_out[v] = int32_t(v);
            if (cluster_out) cluster_out[v] = int32_t(v);
            r.heaviest = std::max<int64_t>(r.heaviest, wi.w[size_t(v)]);
        }
        r.t_setup = since(t0);
        if (result) *result = r;
        return EK_OK;
    }
    hipStream_t s = c->stream;
    constexpr int64_t CL_LOG = 1024;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_cw, d_w, d_score, d_entries, d_rep, d_S, d_grown, d_t, d_sigma, d_in, d_mover,
        d_acc, d_count, d_cursor, d_off, d_tiles, d_seg, d_cluster, d_log, d_elig;
    upload(d_ptr, in.net_ptr.data(), in.net_ptr.size(), s);
    upload(d_pins, in.pins.data(), in.pins.size(), s);
    upload(d_iptr, in.inc_ptr.data(), in.inc_ptr.size(), s);
    upload(d_inc, in.inc.data(), in.inc.size(), s);
    upload(d_cw, wi.cw.data(), wi.cw.size(), s);
    upload(d_w, wi.w.data(), wi.w.size(), s);
    const size_t N = size_t(n);
    d_score.ensure(size_t(nets) * 8);
    d_entries.ensure(N * 4);
    d_rep.ensure(N * 4);
    d_S.ensure(N * 8);
    d_grown.ensure(N * sizeof(int));
    d_t.ensure(N * 4);
    d_sigma.ensure(N * 8);
    d_in.ensure(N * sizeof(int));
    d_mover.ensure(N * sizeof(int));
    d_acc.ensure(N * sizeof(int));
    d_count.ensure(N * sizeof(int));
    d_cursor.ensure(N * sizeof(int));
    d_off.ensure((N + 1) * 8);
    d_tiles.ensure(size_t((n + 1023) / 1024) * 8);
    d_seg.ensure(N * 4);
    d_cluster.ensure(N * 4);
    d_log.ensure(size_t(CL_LOG) * 24);
    d_elig.ensure(8);
    HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(CL_LOG) * 24, s));
    HIPCHK(hipMemsetAsync(d_elig.p, 0, 8, s));
    ek::dev::MatchDev m{};  // the matching's set-up kernels: score[] and entries[]
    m.n = int(n);
    m.nets = int(nets);
    m.max_net = o.max_net;
    m.cap = o.max_cluster;
    m.net_ptr = d_ptr.as<int64_t>();
    m.inc_ptr = d_iptr.as<int64_t>();
    m.pins = d_pins.as<int32_t>();
    m.inc = d_inc.as<int32_t>();
    m.cw = d_cw.as<int32_t>();
    m.w = d_w.as<int32_t>();
    m.score = d_score.as<long long>();
    m.entries = d_entries.as<int32_t>();
    ek::dev::ClusterDev d{};
    d.n = int(n);
    d.cap = o.max_cluster;
    d.net_ptr = m.net_ptr;
    d.inc_ptr = m.inc_ptr;
    d.pins = m.pins;
    d.inc = m.inc;
    d.w = m.w;
    d.score = m.score;
    d.entries = m.entries;
    d.rep = d_rep.as<int32_t>();
    d.S = d_S.as<long long>();
    d.grown = d_grown.as<int>();
    d.t = d_t.as<int32_t>();
    d.sigma = d_sigma.as<long long>();
    d.in = d_in.as<int>();
    d.mover = d_mover.as<int>();
    d.acc = d_acc.as<int>();
    d.count = d_count.as<int>();
    d.cursor = d_cursor.as<int>();
    d.off = d_off.as<long long>();
    d.tiles = d_tiles.as<long long>();
    d.seg = d_seg.as<int32_t>();
    d.cluster = d_cluster.as<int32_t>();
    ek::dev::match_prepare(s, m, d_elig.as<unsigned long long>());
    ek::dev::cluster_init(s, d);
    HIPCHK(hipGetLastError());
    unsigned long long eligible = 0;
    HIPCHK(hipMemcpyAsync(&eligible, d_elig.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    r.eligible_nets = int64_t(eligible);
    r.t_setup = since(t0);

    const auto tr = clk::now();
    std::vector<unsigned long long> log;  // 3 a round, the rounds that joined
    auto flush = [&](int64_t rows) {
        const size_t at = log.size();
        log.resize(at + size_t(rows) * 3);
        if (rows) HIPCHK(hipMemcpyAsync(log.data() + at, d_log.p, size_t(rows) * 24, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    };
    for (;;) {
        if (o.max_rounds > 0 && r.rounds >= o.max_rounds) break;
        const int64_t at = int64_t(r.rounds) % CL_LOG;
        if (at == 0 && r.rounds > 0) {
            flush(CL_LOG);
            HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(CL_LOG) * 24, s));
        }
        unsigned long long* slot = d_log.as<unsigned long long>() + 3 * at;
        ek::dev::cluster_round(s, d, slot);
        HIPCHK(hipGetLastError());
        unsigned long long joins = 0;
        HIPCHK(hipMemcpyAsync(&joins, slot + 2, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (joins == 0) break;  // (not counted: its slot is never read)
        // every counted round joins at least one of the n - 1 nodes that can
        if (int64_t(r.rounds) + 1 > n - 1) ek::fail(EK_EHIP, "ek_cluster: %d rounds joined among %lld nodes", r.rounds + 1, (long long)n);
        ++r.rounds;
    }
    flush(int64_t(r.rounds) - int64_t(log.size() / 3));
    for (int64_t i = 0; i < r.rounds; ++i) r.joins += int64_t(log[size_t(i) * 3 + 2]);
    if (round_log)
        for (int64_t i = 0; i < std::min<int64_t>(r.rounds, log_rounds) * 3; ++i) round_log[i] = int64_t(log[size_t(i)]);
    ek::dev::cluster_number(s, d);
    HIPCHK(hipGetLastError());
    long long clusters = 0;
    std::vector<int32_t> rep(N);
    std::vector<long long> S(N);
    HIPCHK(hipMemcpyAsync(&clusters, d.off + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rep.data(), d_rep.p, N * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(S.data(), d_S.p, N * 8, hipMemcpyDeviceToHost, s));
    if (cluster_out) HIPCHK(hipMemcpyAsync(cluster_out, d_cluster.p, N * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int64_t v = 0; v < n; ++v)
        if (rep[size_t(v)] == v) r.heaviest = std::max<int64_t>(r.heaviest, S[size_t(v)]);
    if (rep_out) std::copy(rep.begin(), rep.end(), rep_out);
    r.n_coarse = clusters;
    r.t_rounds = since(tr);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
