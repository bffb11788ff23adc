// The matching entry of libeigkl_hip.so (ek_match; kernels_match.hip).
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

// Two launches a round, then ONE 8-byte read (the round's pairs) to learn
// whether to go on.  The rounds' two counters stay in a device log of MT_LOG
// rounds, read in bulk when it is full and at the end.  Every buffer is local
// to the call: the context keeps nothing.
int ek_match(ek_ctx* c, const ek_hgr* h, const ek_match_opts* opts, int32_t* mate_out, int32_t* cluster_out,
             int64_t* round_log, int64_t log_rounds, ek_match_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "ek_match: a multi-rank context (%d ranks); the matching runs on one", c->nranks);
    ek::WeightedInput wi;
    const ek_match_opts o = ek::match_check("ek_match", h, opts, wi);
    const ek::RefineInput& in = wi.in;
    const int64_t n = h->nodes, nets = int64_t(in.net_ptr.size()) - 1;
    ek_match_result r{};
    r.n = r.n_coarse = n;
    if (nets == 0) {  // nothing to match along: every node its own cluster
        for (int64_t v = 0; v < n; ++v) {
            if (mate_out) mate_out[v] = -1;
            if (cluster_out) cluster_out[v] = int32_t(v);
        }
        r.t_setup = since(t0);
        if (result) *result = r;
        return EK_OK;
    }
    hipStream_t s = c->stream;
    constexpr int64_t MT_LOG = 1024;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_cw, d_w, d_score, d_entries, d_mate, d_prop, d_flag, d_rank, d_tiles, d_cluster,
        d_log, d_elig;
    upload(d_ptr, in.net_ptr.data(), in.net_ptr.size(), s);
    upload(d_pins, in.pins.data(), in.pins.size(), s);
    upload(d_iptr, in.inc_ptr.data(), in.inc_ptr.size(), s);
    upload(d_inc, in.inc.data(), in.inc.size(), s);
    upload(d_cw, wi.cw.data(), wi.cw.size(), s);
    upload(d_w, wi.w.data(), wi.w.size(), s);
    d_score.ensure(size_t(nets) * 8);
    d_entries.ensure(size_t(n) * 4);
    d_mate.ensure(size_t(n) * 4);
    d_prop.ensure(size_t(n) * 4);
    d_flag.ensure(size_t(n) * sizeof(int));
    d_rank.ensure((size_t(n) + 1) * 8);
    d_tiles.ensure(size_t((n + 1023) / 1024) * 8);
    d_cluster.ensure(size_t(n) * 4);
    d_log.ensure(size_t(MT_LOG) * 16);
    d_elig.ensure(8);
    HIPCHK(hipMemsetAsync(d_mate.p, 0xff, size_t(n) * 4, s));  // -1: unmatched
    HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(MT_LOG) * 16, s));
    HIPCHK(hipMemsetAsync(d_elig.p, 0, 8, s));
    ek::dev::MatchDev d{};
    d.n = int(n);
    d.nets = int(nets);
    d.max_net = o.max_net;
    d.cap = o.max_cluster;
    d.net_ptr = d_ptr.as<int64_t>();
    d.inc_ptr = d_iptr.as<int64_t>();
    d.pins = d_pins.as<int32_t>();
    d.inc = d_inc.as<int32_t>();
    d.cw = d_cw.as<int32_t>();
    d.w = d_w.as<int32_t>();
    d.score = d_score.as<long long>();
    d.entries = d_entries.as<int32_t>();
    d.mate = d_mate.as<int32_t>();
    d.prop = d_prop.as<int32_t>();
    d.flag = d_flag.as<int>();
    d.rank = d_rank.as<long long>();
    d.tiles = d_tiles.as<long long>();
    d.cluster = d_cluster.as<int32_t>();
    ek::dev::match_prepare(s, d, d_elig.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    unsigned long long eligible = 0;
    HIPCHK(hipMemcpyAsync(&eligible, d_elig.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    r.eligible_nets = int64_t(eligible);
    r.t_setup = since(t0);

    const auto tr = clk::now();
    std::vector<unsigned long long> log;  // 2 a round, the rounds that matched
    auto flush = [&](int64_t rows) {
        const size_t at = log.size();
        log.resize(at + size_t(rows) * 2);
        if (rows) HIPCHK(hipMemcpyAsync(log.data() + at, d_log.p, size_t(rows) * 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    };
    for (;;) {
        if (o.max_rounds > 0 && r.rounds >= o.max_rounds) break;
        const int64_t at = int64_t(r.rounds) % MT_LOG;
        if (at == 0 && r.rounds > 0) {
            flush(MT_LOG);
            HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(MT_LOG) * 16, s));
        }
        unsigned long long* slot = d_log.as<unsigned long long>() + 2 * at;
        ek::dev::match_round(s, d, slot);
        HIPCHK(hipGetLastError());
        unsigned long long pairs = 0;
        HIPCHK(hipMemcpyAsync(&pairs, slot + 1, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (pairs == 0) break;  // (not counted: its slot is never read)
        // every counted round matches at least one pair of the n / 2 there can be
        if (2 * (int64_t(r.rounds) + 1) > n) ek::fail(EK_EHIP, "ek_match: %d rounds matched among %lld nodes", r.rounds + 1, (long long)n);
        ++r.rounds;
    }
    flush(int64_t(r.rounds) - int64_t(log.size() / 2));
    for (int64_t i = 0; i < r.rounds; ++i) r.pairs += int64_t(log[size_t(i) * 2 + 1]);
    if (round_log)
        for (int64_t i = 0; i < std::min<int64_t>(r.rounds, log_rounds) * 2; ++i) round_log[i] = int64_t(log[size_t(i)]);
    ek::dev::match_cluster(s, d);
    HIPCHK(hipGetLastError());
    long long clusters = 0;
    HIPCHK(hipMemcpyAsync(&clusters, d.rank + n, 8, hipMemcpyDeviceToHost, s));
    if (mate_out) HIPCHK(hipMemcpyAsync(mate_out, d_mate.p, size_t(n) * 4, hipMemcpyDeviceToHost, s));
    if (cluster_out) HIPCHK(hipMemcpyAsync(cluster_out, d_cluster.p, size_t(n) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    r.n_coarse = clusters;
    r.t_rounds = since(tr);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
