// The weighted k-way refinement entry of libeigkl_hip.so (ek_kway_refine_w,
// DESIGN.md §17; kernels_refine_w.hip and the weight-free launches of
// kernels_refine.hip).
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

// As ek_kway_refine: six launches a round, then ONE 8-byte read (the round's
// accepted moves) to learn whether to go on; the rounds' four counters stay in
// a device log of RF_LOG rounds, read in bulk when it is full and at the end.
// The metrics before and after are ek_kway_metrics_w's kernels over the
// prepared nets (a net of fewer than 2 distinct pins has lambda = 1 and adds
// nothing to any of them); their record also recounts the parts' weights, which
// the final one holds against the weights the rounds kept.  Every buffer is
// local to the call: the context keeps nothing.
int ek_kway_refine_w(ek_ctx* c, const ek_hgr* h, const ek_kway_refine_opts* opts, const int64_t* bounds, int32_t* part,
                     int64_t* round_log, int64_t log_rounds, ek_kway_refine_w_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1)
        ek::fail(EK_ESTATE, "ek_kway_refine_w: a multi-rank context (%d ranks); k-way runs on one", c->nranks);
    ek::RefineWInput in;
    ek::refine_w_prepare("ek_kway_refine_w", h, opts, bounds, part, in);
    const ek_kway_refine_opts& o = in.opts;
    const int64_t n = h->nodes, nets = int64_t(in.in.net_ptr.size()) - 1;
    const size_t ks = size_t(o.k);
    ek_kway_refine_w_result r{};
    r.k = o.k;
    r.total_weight = in.total;
    r.bound_min = *std::min_element(in.bound.begin(), in.bound.end());
    r.bound_max = *std::max_element(in.bound.begin(), in.bound.end());
    std::vector<long long> S(256, 0), L(256, -1);
    for (int64_t i = 0; i < n; ++i) S[size_t(part[i])] += in.w[size_t(i)];
    for (size_t p = 0; p < ks; ++p) L[p] = in.bound[p];
    auto weights = [&] {
        r.part_w_min = *std::min_element(S.begin(), S.begin() + o.k);
        r.part_w_max = *std::max_element(S.begin(), S.begin() + o.k);
        r.parts_over_bound = 0;
        for (size_t p = 0; p < ks; ++p) r.parts_over_bound += S[p] > L[p];
    };
    weights();
    if (nets == 0) {  // nothing to refine, nothing cut
        r.t_setup = since(t0);
        if (result) *result = r;
        return EK_OK;
    }
    hipStream_t s = c->stream;
    std::vector<uint8_t> part8(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) part8[size_t(i)] = uint8_t(part[i]);
    constexpr int64_t RF_LOG = 1024;
    constexpr size_t MET_WORDS = 4 + 256;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_cw, d_w, d_part, d_S, d_L, d_masks, d_key, d_win, d_list, d_thr, d_tgt, d_log,
        d_met;
    upload(d_ptr, in.in.net_ptr.data(), in.in.net_ptr.size(), s);
    upload(d_pins, in.in.pins.data(), in.in.pins.size(), s);
    upload(d_iptr, in.in.inc_ptr.data(), in.in.inc_ptr.size(), s);
    upload(d_inc, in.in.inc.data(), in.in.inc.size(), s);
    upload(d_cw, in.cw.data(), in.cw.size(), s);
    upload(d_w, in.w.data(), in.w.size(), s);
    upload(d_part, part8.data(), part8.size(), s);
    upload(d_S, S.data(), S.size(), s);
    upload(d_L, L.data(), L.size(), s);
    d_masks.ensure(size_t(nets) * 64);
    d_key.ensure(size_t(n) * 8);
    d_win.ensure(size_t(nets) * 8);
    d_list.ensure(size_t(n) * 8);
    d_thr.ensure(256 * 8);
    d_tgt.ensure(size_t(n));
    d_log.ensure(size_t(RF_LOG) * 32);
    d_met.ensure(MET_WORDS * 8);
    HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(RF_LOG) * 32, s));
    long long met[MET_WORDS];
    auto metrics = [&] {
        HIPCHK(hipMemsetAsync(d_met.p, 0, MET_WORDS * 8, s));
        ek::dev::kway_metrics_w(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_cw.as<int32_t>(), n,
                                d_part.as<uint8_t>(), d_w.as<int32_t>(), d_met.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(met, d_met.p, sizeof met, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    };
    metrics();
    r.connectivity_w_before = met[2];
    r.t_setup = since(t0);

    const auto tr = clk::now();
    ek::dev::RefineWDev d{};
    d.n = int(n);
    d.nets = int(nets);
    d.k = o.k;
    d.net_ptr = d_ptr.as<int64_t>();
    d.inc_ptr = d_iptr.as<int64_t>();
    d.pins = d_pins.as<int32_t>();
    d.inc = d_inc.as<int32_t>();
    d.cw = d_cw.as<int32_t>();
    d.w = d_w.as<int32_t>();
    d.part = d_part.as<uint8_t>();
    d.S = d_S.as<long long>();
    d.L = d_L.as<long long>();
    d.masks = d_masks.as<unsigned long long>();
    d.key = d_key.as<unsigned long long>();
    d.win = d_win.as<unsigned long long>();
    d.list = d_list.as<unsigned long long>();
    d.thr = d_thr.as<unsigned long long>();
    d.tgt = d_tgt.as<uint8_t>();
    std::vector<unsigned long long> log;  // 4 a round, the rounds that moved
    auto flush = [&](int64_t rows) {
        const size_t at = log.size();
        log.resize(at + size_t(rows) * 4);
        if (rows) HIPCHK(hipMemcpyAsync(log.data() + at, d_log.p, size_t(rows) * 32, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    };
    for (;;) {
        if (o.max_rounds > 0 && r.rounds >= o.max_rounds) break;
        const int64_t at = int64_t(r.rounds) % RF_LOG;
        if (at == 0 && r.rounds > 0) {
            flush(RF_LOG);
            HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(RF_LOG) * 32, s));
        }
        unsigned long long* slot = d_log.as<unsigned long long>() + 4 * at;
        ek::dev::refine_w_round(s, d, slot);
        HIPCHK(hipGetLastError());
        unsigned long long accepted = 0;
        HIPCHK(hipMemcpyAsync(&accepted, slot + 2, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (accepted == 0) break;
        // every moving round lowers the weighted connectivity by at least 1
        if (r.rounds >= r.connectivity_w_before || r.rounds == INT32_MAX)
            ek::fail(EK_EHIP, "ek_kway_refine_w: %d rounds moved from a weighted connectivity of %lld", r.rounds + 1,
                     (long long)r.connectivity_w_before);
        ++r.rounds;
    }
    flush(int64_t(r.rounds) - int64_t(log.size() / 4));
    r.t_rounds = since(tr);

    const auto tm = clk::now();
    for (int64_t i = 0; i < r.rounds; ++i) {
        r.moves += int64_t(log[size_t(i) * 4 + 2]);
        r.gain_total += int64_t(log[size_t(i) * 4 + 3]);
    }
    if (round_log)
        for (int64_t i = 0; i < std::min<int64_t>(r.rounds, log_rounds) * 4; ++i) round_log[i] = int64_t(log[size_t(i)]);
    HIPCHK(hipMemcpyAsync(part8.data(), d_part.p, part8.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(S.data(), d_S.p, S.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    metrics();  // (drains the stream: the two copies have landed)
    for (size_t p = 0; p < ks; ++p)
        if (S[p] != met[4 + p])
            ek::fail(EK_EHIP, "ek_kway_refine_w: part %d weighs %lld after the rounds, %lld recounted", int(p), S[p],
                     met[4 + p]);
    for (int64_t i = 0; i < n; ++i) part[i] = part8[size_t(i)];
    weights();
    r.cut_nets = met[0];
    r.connectivity = met[1];
    r.connectivity_w = met[2];
    r.soed = met[3];
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
