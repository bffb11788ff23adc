// Weighted FM refinement entry of libeigkl_hip.so (kernels_fmw.hip; the rule
// and the host checker: fmw.cpp).  Beside ek_fm_refine (ctx_fm.cpp), which is
// untouched.
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

// The weighted FM refinement on the device, driven as ek_fm_refine is.
// Set-up: the counts, the weighted cut and the cut nets (k_fmw_counts).  A
// pass: the gains (k_fmw_gains), the pass (k_fmw_pass, one workgroup, one
// launch), ONE 32-byte read of its record, then the rollback of the moves past
// its best prefix (k_fmw_rollback), which also takes their weights back.  The
// move log, the sides and the sides' weights are read once at the end.  Every
// buffer is local to the call: the context keeps nothing.
int ek_fm_refine_w(ek_ctx* c, const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side, int64_t* pass_log,
                   int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_w_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "ek_fm_refine_w: a multi-rank context (%d ranks); FM runs on one", c->nranks);
    ek::FmwInput fi;
    ek::fmw_prepare("ek_fm_refine_w", h, opts, side, fi);
    const ek_fm_opts& o = fi.opts;
    const ek::RefineInput& in = fi.in;
    const int64_t n = h->nodes;
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    ek_fm_w_result r{};
    r.n = n;
    r.total_weight = fi.total;
    r.max_part = fi.max_part;
    int64_t S[2] = {0, 0}, size[2] = {0, 0};
    for (int64_t i = 0; i < n; ++i) {
        S[side[i]] += fi.w[size_t(i)];
        ++size[side[i]];
    }
    r.w0 = S[0];
    r.w1 = S[1];
    r.n0 = size[0];
    r.n1 = size[1];
    if (nets == 0) {  // nothing can move, nothing is cut: the one pass the rule runs keeps nothing
        if (pass_log && log_passes > 0) {
            pass_log[0] = pass_log[1] = pass_log[2] = 0;
            pass_log[3] = std::llabs(S[0] - S[1]);
        }
        r.passes_run = 1;
        r.t_setup = since(t0);
        if (result) *result = r;
        return EK_OK;
    }
    hipStream_t s = c->stream;
    const size_t words = (size_t(n) + 31) / 32;
    std::vector<unsigned> side_w(words, 0u), lock0(words, 0u);
    for (int64_t i = 0; i < n; ++i) {
        if (side[i]) side_w[size_t(i) >> 5] |= 1u << (i & 31);
        if (in.inc_ptr[size_t(i)] == in.inc_ptr[size_t(i) + 1]) lock0[size_t(i) >> 5] |= 1u << (i & 31);
    }
    const int64_t nchunks = (n + ek::dev::FM_CHUNK - 1) / ek::dev::FM_CHUNK;
    const bool gk = nchunks > ek::dev::FM_LDS_CHUNKS;
    const int64_t cap = move_log ? std::max<int64_t>(move_cap, 0) : 0;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_cw, d_w, d_side, d_lock, d_lock0, d_gain, d_cnt, d_state, d_nodes, d_mlog, d_keys,
        d_dirty, d_dlist, d_rec;
    upload(d_ptr, in.net_ptr.data(), in.net_ptr.size(), s);
    upload(d_pins, in.pins.data(), in.pins.size(), s);
    upload(d_iptr, in.inc_ptr.data(), in.inc_ptr.size(), s);
    upload(d_inc, in.inc.data(), in.inc.size(), s);
    upload(d_cw, fi.cw.data(), fi.cw.size(), s);
    upload(d_w, fi.w.data(), fi.w.size(), s);
    upload(d_side, side_w.data(), words, s);
    upload(d_lock0, lock0.data(), words, s);
    d_lock.ensure(words * sizeof(unsigned));
    d_gain.ensure(size_t(n) * sizeof(int32_t));
    d_cnt.ensure(size_t(nets) * 2 * sizeof(unsigned));
    d_nodes.ensure(size_t(n) * sizeof(int32_t));
    d_rec.ensure(4 * sizeof(long long));
    if (cap) d_mlog.ensure(size_t(cap) * sizeof(ek_fm_move));
    if (gk) {
        d_keys.ensure(size_t(nchunks) * 2 * sizeof(unsigned long long));
        d_dirty.ensure((size_t(nchunks) + 31) / 32 * sizeof(unsigned));
        d_dlist.ensure(size_t(nchunks) * sizeof(int32_t));
    }
    long long state[5] = {0, (long long)S[0], (long long)S[1], 0, 0};
    upload(d_state, state, 5, s);
    ek::dev::FmwDev d{};
    d.n = int(n);
    d.nets = int(nets);
    d.nchunks = int(nchunks);
    d.lmax = r.max_part;
    d.net_ptr = d_ptr.as<int64_t>();
    d.inc_ptr = d_iptr.as<int64_t>();
    d.pins = d_pins.as<int32_t>();
    d.inc = d_inc.as<int32_t>();
    d.cw = d_cw.as<int32_t>();
    d.w = d_w.as<int32_t>();
    d.side = d_side.as<unsigned>();
    d.lock = d_lock.as<unsigned>();
    d.lock0 = d_lock0.as<unsigned>();
    d.gain = d_gain.as<int32_t>();
    d.cnt = d_cnt.as<unsigned>();
    d.state = d_state.as<long long>();
    d.pass_nodes = d_nodes.as<int32_t>();
    d.mlog = cap ? d_mlog.as<ek_fm_move>() : nullptr;
    d.mlog_cap = cap;
    d.gkeys = gk ? d_keys.as<unsigned long long>() : nullptr;
    d.gdirty = gk ? d_dirty.as<unsigned>() : nullptr;
    d.gdlist = gk ? d_dlist.as<int32_t>() : nullptr;
    // the weighted cut and the cut nets of the sides as they are (state[3], state[4], zero before)
    auto counted_cut = [&](int64_t& cut_nets) -> int64_t {
        HIPCHK(hipMemsetAsync(d.state + 3, 0, 2 * sizeof(long long), s));
        ek::dev::fmw_counts(s, d);
        HIPCHK(hipGetLastError());
        long long got[2] = {-1, -1};
        HIPCHK(hipMemcpyAsync(got, d.state + 3, sizeof got, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        cut_nets = got[1];
        return got[0];
    };
    r.cut_before = counted_cut(r.cut_nets_before);
    state[0] = r.cut_before;
    HIPCHK(hipMemcpyAsync(d.state, state, sizeof(long long), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (state[] is this frame's)
    r.t_setup = since(t0);

    const auto tp = clk::now();
    int64_t cut = r.cut_before, dist = std::llabs(S[0] - S[1]);
    for (;;) {
        if (o.max_passes > 0 && r.passes >= o.max_passes) break;
        ek::dev::fmw_gains(s, d);
        HIPCHK(hipGetLastError());
        ek::dev::fmw_pass(s, d, o.stall, (long long)r.moves_tried, d_rec.as<long long>());
        HIPCHK(hipGetLastError());
        long long rec[4] = {-1, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(rec, d_rec.p, sizeof rec, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // the record against what the rule allows: 0 <= t* <= t <= n, (c, d) never above the pass's start
        if (rec[0] < 0 || rec[0] > n || rec[1] < 0 || rec[1] > rec[0] || rec[2] < 0 || rec[2] > cut ||
            (rec[1] == 0 && (rec[2] != cut || rec[3] != dist)) || (rec[1] > 0 && rec[2] == cut && rec[3] >= dist))
            ek::fail(EK_EHIP, "ek_fm_refine_w: pass %d reported %lld moves, best prefix %lld, cut %lld, |S0 - S1| %lld from "
                     "cut %lld, |S0 - S1| %lld", r.passes_run + 1, rec[0], rec[1], rec[2], rec[3], (long long)cut,
                     (long long)dist);
        ek::dev::fmw_rollback(s, d, int(rec[1]), int(rec[0] - rec[1]));
        HIPCHK(hipGetLastError());
        if (pass_log && r.passes_run < log_passes)
            for (int j = 0; j < 4; ++j) pass_log[4 * int64_t(r.passes_run) + j] = rec[j];
        if (r.passes_run == INT32_MAX) ek::fail(EK_EINVAL, "ek_fm_refine_w: more than 2^31 - 1 passes");
        ++r.passes_run;
        r.moves_tried += rec[0];
        r.moves_kept += rec[1];
        cut = rec[2];
        dist = rec[3];
        if (rec[1] == 0) break;
        ++r.passes;
    }
    HIPCHK(hipStreamSynchronize(s));
    r.t_passes = since(tp);

    const auto tm = clk::now();
    HIPCHK(hipMemcpyAsync(state, d.state, 3 * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(side_w.data(), d_side.p, words * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (cap && r.moves_tried > 0)
        HIPCHK(hipMemcpyAsync(move_log, d_mlog.p, size_t(std::min(cap, r.moves_tried)) * sizeof(ek_fm_move),
                              hipMemcpyDeviceToHost, s));
    r.cut = counted_cut(r.cut_nets);  // (drains the stream: the copies have landed)
    for (int64_t i = 0; i < n; ++i) side[i] = uint8_t((side_w[size_t(i) >> 5] >> (i & 31)) & 1u);
    // the sides' weights again from the sides read back, against the device's
    S[0] = S[1] = size[0] = size[1] = 0;
    for (int64_t i = 0; i < n; ++i) {
        S[side[i]] += fi.w[size_t(i)];
        ++size[side[i]];
    }
    if (r.cut != cut || state[0] != cut || state[1] != S[0] || state[2] != S[1] || std::llabs(S[0] - S[1]) != dist)
        ek::fail(EK_EHIP, "ek_fm_refine_w: the passes left a cut of %lld and weights %lld | %lld, the sides count %lld and "
                 "%lld | %lld", (long long)cut, state[1], state[2], (long long)r.cut, (long long)S[0], (long long)S[1]);
    r.w0 = S[0];
    r.w1 = S[1];
    r.n0 = size[0];
    r.n1 = size[1];
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
