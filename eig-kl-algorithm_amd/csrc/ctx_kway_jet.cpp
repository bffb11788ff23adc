// The Jet refinement entry of libeigkl_hip.so (ek_kway_jet, DESIGN.md §18;
// kernels_jet.hip, the masks launch of kernels_refine.hip, the select of
// kernels_refine_w.hip and the weighted metrics of kernels_kway.hip).
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

// An iteration is two clears (its 64-byte record, the next lock array), the
// five launches of jet_iteration and the metrics launch over the prepared nets,
// which recounts X_i; then ONE 64-byte read: the iteration's candidates,
// passing candidates and accepted moves, and the four metrics.  The host keeps
// the log, the best X and the stop rule; when X_i improves, the part vector is
// copied to the snapshot device to device, in stream order before the next
// iteration's first launch.  The metrics before and after are
// ek_kway_metrics_w's kernels (a net of fewer than 2 distinct pins has lambda =
// 1 and adds nothing to any of them); their record also recounts the parts'
// weights, which the last state's is held against the weights the iterations
// kept.  Every buffer is local to the call: the context keeps nothing.
int ek_kway_jet(ek_ctx* c, const ek_hgr* h, const ek_kway_jet_opts* opts, const int64_t* bounds, int32_t* part,
                int64_t* iter_log, int64_t log_iters, ek_kway_jet_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "ek_kway_jet: a multi-rank context (%d ranks); k-way runs on one", c->nranks);
    ek::RefineWInput in;
    const ek_kway_jet_opts o = ek::jet_prepare("ek_kway_jet", h, opts, bounds, part, in);
    const int64_t n = h->nodes, nets = int64_t(in.in.net_ptr.size()) - 1;
    const size_t ks = size_t(o.k);
    ek_kway_jet_result r{};
    r.k = o.k;
    r.total_weight = in.total;
    r.bound_min = *std::min_element(in.bound.begin(), in.bound.end());
    r.bound_max = *std::max_element(in.bound.begin(), in.bound.end());
    std::vector<long long> S(256, 0), L(256, -1);
    for (int64_t i = 0; i < n; ++i) S[size_t(part[i])] += in.w[size_t(i)];
    for (size_t p = 0; p < ks; ++p) L[p] = in.bound[p];
    auto weights = [&](const long long* sw) {
        r.part_w_min = *std::min_element(sw, sw + o.k);
        r.part_w_max = *std::max_element(sw, sw + o.k);
        r.parts_over_bound = 0;
        for (size_t p = 0; p < ks; ++p) r.parts_over_bound += sw[p] > L[p];
    };
    if (nets == 0) {  // nothing to refine, nothing cut
        weights(S.data());
        r.t_setup = since(t0);
        if (result) *result = r;
        return EK_OK;
    }
    hipStream_t s = c->stream;
    std::vector<uint8_t> part8(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) part8[size_t(i)] = uint8_t(part[i]);
    constexpr size_t MET_WORDS = 4 + 256, REC_WORDS = 8;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_cw, d_w, d_part, d_snap, d_S, d_L, d_masks, d_key, d_list, d_thr, d_tgt, d_lock0,
        d_lock1, d_rec, d_met;
    upload(d_ptr, in.in.net_ptr.data(), in.in.net_ptr.size(), s);
    upload(d_pins, in.in.pins.data(), in.in.pins.size(), s);
    upload(d_iptr, in.in.inc_ptr.data(), in.in.inc_ptr.size(), s);
    upload(d_inc, in.in.inc.data(), in.in.inc.size(), s);
    upload(d_cw, in.cw.data(), in.cw.size(), s);
    upload(d_w, in.w.data(), in.w.size(), s);
    upload(d_part, part8.data(), part8.size(), s);
    upload(d_snap, part8.data(), part8.size(), s);
    upload(d_S, S.data(), S.size(), s);
    upload(d_L, L.data(), L.size(), s);
    d_masks.ensure(size_t(nets) * 64);
    d_key.ensure(size_t(n) * 8);
    d_list.ensure(size_t(n) * 8);
    d_thr.ensure(256 * 8);
    d_tgt.ensure(size_t(n));
    d_lock0.ensure(size_t(n));
    d_lock1.ensure(size_t(n));
    d_rec.ensure(REC_WORDS * 8);
    d_met.ensure(MET_WORDS * 8);
    HIPCHK(hipMemsetAsync(d_lock0.p, 0, size_t(n), s));
    long long met[MET_WORDS];
    auto metrics = [&](const DBuf& of) {
        HIPCHK(hipMemsetAsync(d_met.p, 0, MET_WORDS * 8, s));
        ek::dev::kway_metrics_w(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_cw.as<int32_t>(), n,
                                of.as<uint8_t>(), d_w.as<int32_t>(), d_met.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(met, d_met.p, sizeof met, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    };
    metrics(d_part);
    r.connectivity_w_before = met[2];
    r.t_setup = since(t0);

    const auto tr = clk::now();
    ek::dev::JetDev d{};
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
    d.neg_num = o.neg_num;
    d.neg_den = o.neg_den;
    uint8_t* lock = d_lock0.as<uint8_t>();
    uint8_t* lock_next = d_lock1.as<uint8_t>();
    unsigned long long* rec = d_rec.as<unsigned long long>();
    long long best = r.connectivity_w_before, stale = 0, last_accepted = 0;
    for (;;) {
        HIPCHK(hipMemsetAsync(rec, 0, REC_WORDS * 8, s));
        HIPCHK(hipMemsetAsync(lock_next, 0, size_t(n), s));
        d.lock = lock;
        d.lock_next = lock_next;
        ek::dev::jet_iteration(s, d, rec);
        ek::dev::kway_metrics_w(s, nets, d.r.net_ptr, d.r.pins, d.r.cw, 0, d.r.part, d.r.w, rec + 4);
        HIPCHK(hipGetLastError());
        long long got[REC_WORDS];
        HIPCHK(hipMemcpyAsync(got, rec, sizeof got, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const long long accepted = got[2], X = got[6];
        if (iter_log && r.iters < log_iters) {
            int64_t* row = iter_log + 4 * int64_t(r.iters);
            row[0] = got[0];
            row[1] = got[1];
            row[2] = accepted;
            row[3] = X;
        }
        if (r.iters == INT32_MAX) ek::fail(EK_EHIP, "ek_kway_jet: 2^31 iterations");
        ++r.iters;
        r.moves += accepted;
        if (X < best) {
            best = X;
            r.best_iter = r.iters;
            HIPCHK(hipMemcpyAsync(d_snap.p, d_part.p, size_t(n), hipMemcpyDeviceToDevice, s));
            stale = 0;
        } else {
            ++stale;
        }
        std::swap(lock, lock_next);
        const bool idle = accepted == 0 && last_accepted == 0;
        last_accepted = accepted;
        if (stale == o.patience || (o.max_iters > 0 && r.iters == o.max_iters) || idle) break;
    }
    r.t_iters = since(tr);

    const auto tm = clk::now();
    HIPCHK(hipMemcpyAsync(S.data(), d_S.p, S.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    metrics(d_part);  // the last state (drains the stream: the copy has landed)
    for (size_t p = 0; p < ks; ++p)
        if (S[p] != met[4 + p])
            ek::fail(EK_EHIP, "ek_kway_jet: part %d weighs %lld after the iterations, %lld recounted", int(p), S[p],
                     met[4 + p]);
    HIPCHK(hipMemcpyAsync(part8.data(), d_snap.p, part8.size(), hipMemcpyDeviceToHost, s));
    if (r.best_iter != r.iters) metrics(d_snap);
    else HIPCHK(hipStreamSynchronize(s));
    if (met[2] != best)
        ek::fail(EK_EHIP, "ek_kway_jet: the snapshot's weighted connectivity is %lld, %lld when it was taken", met[2], best);
    for (int64_t i = 0; i < n; ++i) part[i] = part8[size_t(i)];
    weights(met + 4);
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
