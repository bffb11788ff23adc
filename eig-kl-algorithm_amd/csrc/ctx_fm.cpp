// FM refinement entries of libeigkl_hip.so, unweighted and weighted
// (kernels_fm.hip; the rules and the host checkers: fm.cpp).
#include <type_traits>

#include "ctx.hpp"

using namespace ek::rt;

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

void fm_check_ctx(const char* who, ek_ctx* c) {
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "%s: a multi-rank context (%d ranks); FM runs on one", who, c->nranks);
}

// what fm_device hands its caller's final check
struct FmEnd {
    const unsigned* side_w;  // the side bitmap read back
    long long state[3];      // the device's cut and the sides' sizes or weights
    int64_t cut, dist;       // (c, d) of the last pass's record
};

void unpack_sides(const unsigned* side_w, int64_t n, uint8_t* side) {
    for (int64_t i = 0; i < n; ++i) side[i] = uint8_t((side_w[size_t(i) >> 5] >> (i & 31)) & 1u);
}

// The FM refinement on the device under either rule: D = FmDev with R =
// ek_fm_result, or D = FmwDev with R = ek_fm_w_result and the weights in fi
// (null otherwise: the unweighted run uploads none).  S: the sizes or weights
// of the sides given, L: the sides' bounds (L_max twice, or the pair of §16, where
// d is the slack difference |(S0 - L0) - (S1 - L1)|); r.n is set.  Set-up: the counts and the
// cut (k_fm_counts).  A pass: the gains (k_fm_gains), the pass (k_fm_pass, one
// workgroup, one launch), ONE 32-byte read of its record, then the rollback of
// the moves past its best prefix (k_fm_rollback).  The move log, the sides and
// state[0..2] are read once at the end, and the cut is counted again into r;
// final(FmEnd) is then the caller's consistency check and its unpacking of the
// sides, inside t_metrics as the read-back is.  Every buffer is local to the
// call: the context keeps nothing.  With no net nothing runs, final included:
// the one pass the rule runs keeps nothing.
template <class D, class R, class Final>
void fm_device(const char* who, ek_ctx* c, const ek::RefineInput& in, const ek_fm_opts& o, const ek::FmwInput* fi,
               const uint8_t* side, const int64_t S[2], const int64_t L[2], clk::time_point t0, int64_t* pass_log, int64_t log_passes,
               ek_fm_move* move_log, int64_t move_cap, R& r, Final final) {
    constexpr bool WT = std::is_same_v<D, ek::dev::FmwDev>;
    constexpr int NCUT = WT ? 2 : 1;  // fm_counts' words of state, from state[3]
    const int64_t n = r.n, nets = int64_t(in.net_ptr.size()) - 1;
    if (nets == 0) {  // nothing can move, nothing is cut
        if (pass_log && log_passes > 0) {
            pass_log[0] = pass_log[1] = pass_log[2] = 0;
            pass_log[3] = std::llabs((S[0] - L[0]) - (S[1] - L[1]));
        }
        r.passes_run = 1;
        r.t_setup = since(t0);
        return;
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
    if constexpr (WT) {
        upload(d_cw, fi->cw.data(), fi->cw.size(), s);
        upload(d_w, fi->w.data(), fi->w.size(), s);
    }
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
    long long state[3 + NCUT] = {0, (long long)S[0], (long long)S[1]};
    upload(d_state, state, 3 + NCUT, s);
    D d{};
    d.n = int(n);
    d.nets = int(nets);
    d.nchunks = int(nchunks);
    if constexpr (WT) {
        d.cw = d_cw.as<int32_t>();
        d.w = d_w.as<int32_t>();
        d.lmax = L[0];
        d.lmax1 = L[1];
    } else {
        d.lmax = int(std::min<int64_t>(L[0], INT32_MAX));
    }
    d.net_ptr = d_ptr.as<int64_t>();
    d.inc_ptr = d_iptr.as<int64_t>();
    d.pins = d_pins.as<int32_t>();
    d.inc = d_inc.as<int32_t>();
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
    // the cut of the sides as they are and, weighted, their cut nets (state[3..], zero before)
    auto counted_cut = [&](int64_t& cut, [[maybe_unused]] int64_t* cut_nets) {
        HIPCHK(hipMemsetAsync(d.state + 3, 0, NCUT * sizeof(long long), s));
        ek::dev::fm_counts(s, d);
        HIPCHK(hipGetLastError());
        long long got[NCUT];
        std::fill(got, got + NCUT, -1ll);
        HIPCHK(hipMemcpyAsync(got, d.state + 3, sizeof got, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        cut = got[0];
        if constexpr (WT) *cut_nets = got[1];
    };
    if constexpr (WT) counted_cut(r.cut_before, &r.cut_nets_before);
    else counted_cut(r.cut_before, nullptr);
    state[0] = r.cut_before;
    HIPCHK(hipMemcpyAsync(d.state, state, sizeof(long long), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (state[] is this frame's)
    r.t_setup = since(t0);

    const auto tp = clk::now();
    const char* dname = WT ? (L[0] == L[1] ? "|S0 - S1|" : "slack difference") : "|s0 - s1|";
    int64_t cut = r.cut_before, dist = std::llabs((S[0] - L[0]) - (S[1] - L[1]));
    for (;;) {
        if (o.max_passes > 0 && r.passes >= o.max_passes) break;
        ek::dev::fm_gains(s, d);
        HIPCHK(hipGetLastError());
        ek::dev::fm_pass(s, d, o.stall, (long long)r.moves_tried, d_rec.as<long long>());
        HIPCHK(hipGetLastError());
        long long rec[4] = {-1, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(rec, d_rec.p, sizeof rec, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // the record against what the rule allows: 0 <= t* <= t <= n, (c, d) never above the pass's start
        if (rec[0] < 0 || rec[0] > n || rec[1] < 0 || rec[1] > rec[0] || rec[2] < 0 || rec[2] > cut ||
            (rec[1] == 0 && (rec[2] != cut || rec[3] != dist)) || (rec[1] > 0 && rec[2] == cut && rec[3] >= dist))
            ek::fail(EK_EHIP, "%s: pass %d reported %lld moves, best prefix %lld, cut %lld, %s %lld from cut %lld, %s %lld",
                     who, r.passes_run + 1, rec[0], rec[1], rec[2], dname, rec[3], (long long)cut, dname, (long long)dist);
        ek::dev::fm_rollback(s, d, int(rec[1]), int(rec[0] - rec[1]));
        HIPCHK(hipGetLastError());
        if (pass_log && r.passes_run < log_passes)
            for (int j = 0; j < 4; ++j) pass_log[4 * int64_t(r.passes_run) + j] = rec[j];
        if (r.passes_run == INT32_MAX) ek::fail(EK_EINVAL, "%s: more than 2^31 - 1 passes", who);
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
    FmEnd end{side_w.data(), {0, 0, 0}, cut, dist};
    HIPCHK(hipMemcpyAsync(end.state, d.state, 3 * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(side_w.data(), d_side.p, words * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (cap && r.moves_tried > 0)
        HIPCHK(hipMemcpyAsync(move_log, d_mlog.p, size_t(std::min(cap, r.moves_tried)) * sizeof(ek_fm_move),
                              hipMemcpyDeviceToHost, s));
    // (drains the stream: the copies have landed)
    if constexpr (WT) counted_cut(r.cut, &r.cut_nets);
    else counted_cut(r.cut, nullptr);
    final(end);
    r.t_metrics = since(tm);
}

// The weighted refinement on the device under the sides' bounds L, R =
// ek_fm_w_result or ek_fm_wb_result with n, W and its bound fields set; the
// sides read back are measured again on the host and held against the device's
// weights and its last d.
template <class R>
void fmw_device(const char* who, ek_ctx* c, const ek_hgr* h, const ek::FmwInput& fi, const int64_t L[2],
                clk::time_point t0, uint8_t* side, int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log,
                int64_t move_cap, R& r) {
    const int64_t n = h->nodes;
    int64_t S[2], size[2];
    auto measure = [&] {  // the sides' weights and node counts from side[]
        S[0] = S[1] = size[0] = size[1] = 0;
        for (int64_t i = 0; i < n; ++i) {
            S[side[i]] += fi.w[size_t(i)];
            ++size[side[i]];
        }
        r.w0 = S[0];
        r.w1 = S[1];
        r.n0 = size[0];
        r.n1 = size[1];
    };
    measure();
    fm_device<ek::dev::FmwDev>(who, c, fi.in, fi.opts, &fi, side, S, L, t0, pass_log, log_passes, move_log, move_cap, r,
                               [&](const FmEnd& e) {
        unpack_sides(e.side_w, n, side);
        measure();  // again from the sides read back, against the device's
        if (r.cut != e.cut || e.state[0] != e.cut || e.state[1] != S[0] || e.state[2] != S[1] ||
            std::llabs((S[0] - L[0]) - (S[1] - L[1])) != e.dist)
            ek::fail(EK_EHIP, "%s: the passes left a cut of %lld and weights %lld | %lld, the sides count %lld and %lld | "
                     "%lld", who, (long long)e.cut, e.state[1], e.state[2], (long long)r.cut, (long long)S[0],
                     (long long)S[1]);
    });
}

}  // namespace

extern "C" {

int ek_fm_refine(ek_ctx* c, const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side, int64_t* pass_log,
                 int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    fm_check_ctx("ek_fm_refine", c);
    const ek_fm_opts o = ek::fm_check("ek_fm_refine", h, opts, side);
    const int64_t n = h->nodes;
    ek::RefineInput in;
    ek::refine_prepare(*h, in);
    ek_fm_result r{};
    r.n = n;
    r.max_part = ek::refine_max_part(n, 2, o.imbalance);
    int64_t size[2] = {0, 0};
    for (int64_t i = 0; i < n; ++i) ++size[side[i]];
    r.n0 = size[0];
    r.n1 = size[1];
    const int64_t L[2] = {r.max_part, r.max_part};
    fm_device<ek::dev::FmDev>("ek_fm_refine", c, in, o, nullptr, side, size, L, t0, pass_log, log_passes, move_log, move_cap,
                              r, [&](const FmEnd& e) {
        if (r.cut != e.cut || e.state[0] != e.cut || e.state[1] + e.state[2] != n)
            ek::fail(EK_EHIP, "ek_fm_refine: the passes left a cut of %lld, the sides' nets count %lld (sizes %lld + %lld of "
                     "%lld)", (long long)e.cut, (long long)r.cut, e.state[1], e.state[2], (long long)n);
        unpack_sides(e.side_w, n, side);
        r.n0 = e.state[1];
        r.n1 = e.state[2];
    });
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_fm_refine_w(ek_ctx* c, const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side, int64_t* pass_log,
                   int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_w_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    fm_check_ctx("ek_fm_refine_w", c);
    ek::FmwInput fi;
    ek::fmw_prepare("ek_fm_refine_w", h, opts, side, fi);
    ek_fm_w_result r{};
    r.n = h->nodes;
    r.total_weight = fi.total;
    r.max_part = fi.max_part;
    const int64_t L[2] = {fi.max_part, fi.max_part};
    fmw_device("ek_fm_refine_w", c, h, fi, L, t0, side, pass_log, log_passes, move_log, move_cap, r);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_fm_refine_wb(ek_ctx* c, const ek_hgr* h, const ek_fm_opts* opts, const int64_t bounds[2], uint8_t* side,
                    int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log, int64_t move_cap,
                    ek_fm_wb_result* result) {
    EK_TRY
    const auto t0 = clk::now();
    fm_check_ctx("ek_fm_refine_wb", c);
    ek::FmwInput fi;
    ek::fmwb_prepare("ek_fm_refine_wb", h, opts, bounds, side, fi);
    ek_fm_wb_result r{};
    r.n = h->nodes;
    r.total_weight = fi.total;
    r.bound0 = bounds[0];
    r.bound1 = bounds[1];
    fmw_device("ek_fm_refine_wb", c, h, fi, bounds, t0, side, pass_log, log_passes, move_log, move_cap, r);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
