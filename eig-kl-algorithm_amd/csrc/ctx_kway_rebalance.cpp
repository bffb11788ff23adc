// The k-way rebalancing entry of libeigkl_hip.so (ek_kway_rebalance, DESIGN.md
// §21; kernels_rebalance.hip, the masks launch of kernels_refine.hip, the
// select of kernels_refine_w.hip and the weighted metrics of kernels_kway.hip).
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

// A round is one clear (its 32-byte record) and the eight launches of
// rebal_round, then ONE 32-byte read: the round's moves, proposers, X after it
// and evicted nodes.  The host keeps the log and the stop rule.  X falls by at
// least 1 every round that moves, so a run has at most X_0 of them: one more is
// EK_EHIP, not a loop.  The metrics before and after are ek_kway_metrics_w's
// kernels over the prepared nets; their record also recounts the parts'
// weights, which the final state's is held against the weights the rounds kept.
// Every buffer is local to the call: the context keeps nothing.
int ek_kway_rebalance(ek_ctx* c, const ek_hgr* h, const ek_kway_rebalance_opts* opts, const int64_t* bounds,
                      int32_t* part, int64_t* round_log, int64_t log_rounds, ek_kway_rebalance_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1)
        ek::fail(EK_ESTATE, "ek_kway_rebalance: a multi-rank context (%d ranks); k-way runs on one", c->nranks);
    ek::RefineWInput in;
    const ek_kway_rebalance_opts o = ek::rebalance_prepare("ek_kway_rebalance", h, opts, bounds, part, in);
    const int64_t n = h->nodes, nets = int64_t(in.in.net_ptr.size()) - 1;
    const size_t ks = size_t(o.k);
    ek_kway_rebalance_result r{};
    r.k = o.k;
    r.total_weight = in.total;
    r.bound_min = *std::min_element(in.bound.begin(), in.bound.end());
    r.bound_max = *std::max_element(in.bound.begin(), in.bound.end());
    std::vector<long long> S(256, 0), L(256, -1), zero(256, 0);
    for (int64_t i = 0; i < n; ++i) S[size_t(part[i])] += in.w[size_t(i)];
    for (size_t p = 0; p < ks; ++p) L[p] = in.bound[p];
    auto excess = [&](const long long* sw, int64_t* over) {
        long long X = 0;
        *over = 0;
        for (size_t p = 0; p < ks; ++p)
            if (sw[p] > L[p]) {
                X += sw[p] - L[p];
                ++*over;
            }
        return X;
    };
    const long long X0 = excess(S.data(), &r.parts_over_before);
    r.excess_before = X0;

    hipStream_t s = c->stream;
    std::vector<uint8_t> part8(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) part8[size_t(i)] = uint8_t(part[i]);
    constexpr size_t MET_WORDS = 4 + 256, REC_WORDS = 4;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_cw, d_w, d_part, d_S, d_L, d_zero, d_room, d_masks, d_key, d_list, d_listb, d_thr,
        d_thra, d_tgt, d_rec, d_met;
    upload(d_ptr, in.in.net_ptr.data(), in.in.net_ptr.size(), s);
    upload(d_pins, in.in.pins.data(), in.in.pins.size(), s);
    upload(d_cw, in.cw.data(), in.cw.size(), s);
    upload(d_w, in.w.data(), in.w.size(), s);
    upload(d_part, part8.data(), part8.size(), s);
    d_met.ensure(MET_WORDS * 8);
    long long met[MET_WORDS];
    auto metrics = [&]() {
        HIPCHK(hipMemsetAsync(d_met.p, 0, MET_WORDS * 8, s));
        ek::dev::kway_metrics_w(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_cw.as<int32_t>(), n,
                                d_part.as<uint8_t>(), d_w.as<int32_t>(), d_met.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(met, d_met.p, sizeof met, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    };
    metrics();
    r.connectivity_w_before = met[2];
    for (size_t p = 0; p < ks; ++p)
        if (S[p] != met[4 + p])
            ek::fail(EK_EHIP, "ek_kway_rebalance: part %d weighs %lld at the start, %lld counted on the device", int(p),
                     S[p], met[4 + p]);
    r.t_setup = since(t0);

    const auto tr = clk::now();
    if (X0 > 0) {
        upload(d_iptr, in.in.inc_ptr.data(), in.in.inc_ptr.size(), s);
        upload(d_inc, in.in.inc.data(), in.in.inc.size(), s);
        upload(d_S, S.data(), S.size(), s);
        upload(d_L, L.data(), L.size(), s);
        upload(d_zero, zero.data(), zero.size(), s);
        d_room.ensure(256 * 8);
        d_masks.ensure(size_t(nets) * 64);
        d_key.ensure(size_t(n) * 8);
        d_list.ensure(size_t(n) * 8);
        d_listb.ensure(size_t(n) * 8);
        d_thr.ensure(256 * 8);
        d_thra.ensure(256 * 8);
        d_tgt.ensure(size_t(n));
        d_rec.ensure(REC_WORDS * 8);
        ek::dev::RebalDev d{};
        d.r.n = int(n);
        d.r.nets = int(nets);
        d.r.k = o.k;
        d.r.net_ptr = d_ptr.as<int64_t>();
        d.r.inc_ptr = d_iptr.as<int64_t>();
        d.r.pins = d_pins.as<int32_t>();
        d.r.inc = d_inc.as<int32_t>();
        d.r.cw = d_cw.as<int32_t>();
        d.r.w = d_w.as<int32_t>();
        d.r.part = d_part.as<uint8_t>();
        d.r.S = d_S.as<long long>();
        d.r.L = d_L.as<long long>();
        d.r.masks = d_masks.as<unsigned long long>();
        d.r.key = d_key.as<unsigned long long>();
        d.r.list = d_list.as<unsigned long long>();
        d.r.thr = d_thr.as<unsigned long long>();
        d.r.tgt = d_tgt.as<uint8_t>();
        d.list_b = d_listb.as<unsigned long long>();
        d.thr_a = d_thra.as<unsigned long long>();
        d.room = d_room.as<long long>();
        d.zero = d_zero.as<long long>();
        unsigned long long* rec = d_rec.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(rec, 0, REC_WORDS * 8, s));
        ek::dev::rebal_excess(s, d, rec);  // the first round's rooms
        long long X = X0;
        while (X > 0) {
            HIPCHK(hipMemsetAsync(rec, 0, REC_WORDS * 8, s));
            ek::dev::rebal_round(s, d, rec);
            HIPCHK(hipGetLastError());
            long long got[REC_WORDS];
            HIPCHK(hipMemcpyAsync(got, rec, sizeof got, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            const long long moved = got[0];
            if (moved == 0) break;  // neither counted nor logged
            if (r.rounds >= X0 || got[2] >= X)
                ek::fail(EK_EHIP, "ek_kway_rebalance: round %lld left the excess at %lld after %lld (%lld at the start)",
                         (long long)r.rounds + 1, got[2], X, X0);
            X = got[2];
            if (round_log && r.rounds < log_rounds) {
                int64_t* row = round_log + 4 * int64_t(r.rounds);
                row[0] = got[1];
                row[1] = got[3];
                row[2] = moved;
                row[3] = X;
            }
            if (r.rounds == INT32_MAX) ek::fail(EK_EHIP, "ek_kway_rebalance: 2^31 rounds");
            ++r.rounds;
            r.moves += moved;
            if (o.max_rounds > 0 && r.rounds == o.max_rounds) break;
        }
        HIPCHK(hipMemcpyAsync(S.data(), d_S.p, S.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    }
    r.t_rounds = since(tr);

    const auto tm = clk::now();
    HIPCHK(hipMemcpyAsync(part8.data(), d_part.p, part8.size(), hipMemcpyDeviceToHost, s));
    metrics();  // the final state (drains the stream: the copies have landed)
    for (size_t p = 0; p < ks; ++p)
        if (S[p] != met[4 + p])
            ek::fail(EK_EHIP, "ek_kway_rebalance: part %d weighs %lld after the rounds, %lld recounted", int(p), S[p],
                     met[4 + p]);
    for (int64_t i = 0; i < n; ++i) part[i] = part8[size_t(i)];
    r.excess = excess(met + 4, &r.parts_over_bound);
    r.part_w_min = *std::min_element(met + 4, met + 4 + o.k);
    r.part_w_max = *std::max_element(met + 4, met + 4 + o.k);
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
