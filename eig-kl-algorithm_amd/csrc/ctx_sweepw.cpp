// Weighted sweep cut entries of libeigkl_hip.so (kernels_sweepw.hip; the sort:
// ctx_sweep.cpp; the rule and the host checker: sweepw.cpp).
#include "ctx.hpp"

using namespace ek::rt;

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }
using u64 = unsigned long long;

// The weighted sweep cut of v (device, n doubles) over h's nets and weights;
// r comes from sweepw_check (n, W, L_max).  Every buffer is local to the call.
// Host synchronisations: the sort's two, one after the profiles and P (for
// their time), one for the 80-byte result record; order, profile_w and P are
// read only when asked for.
void sweepw_on_device(ek_ctx* c, const ek_hgr* h, const double* v, ek_sweep_w_result r, int32_t* order_out,
                      int64_t* profile_out, int64_t* prefix_out, ek_sweep_w_result* result) {
    hipStream_t s = c->stream;
    const int64_t n = h->nodes;
    const int ni = int(n);

    // sort
    auto t = clk::now();
    SweepSort st;
    sweep_sort(c, v, n, st);
    const int32_t* order = st.order();
    r.t_sort = since(t);

    // the two profiles and the prefix weight
    t = clk::now();
    DBuf d_ptr, d_pins, d_cw, d_w, profw, prof, prefix, span, tmp64;
    const int64_t nets = h->nets;
    const int nspan = nets > 0 ? ek::dev::sweep_span_blocks(nets) : 0;
    const size_t words = size_t(n) + 1;
    profw.ensure(words * sizeof(u64));
    prof.ensure(words * sizeof(unsigned));
    prefix.ensure(words * sizeof(u64));
    span.ensure(size_t(std::max(nspan, 1)) * sizeof(unsigned));
    tmp64.ensure(ek::dev::sweepw_scan_tmp_words(n + 1) * sizeof(u64));
    HIPCHK(hipMemsetAsync(profw.p, 0, words * sizeof(u64), s));
    HIPCHK(hipMemsetAsync(prof.p, 0, words * sizeof(unsigned), s));
    if (nets > 0) {
        upload(d_ptr, h->net_ptr.data(), size_t(nets) + 1, s);
        upload(d_pins, h->pins.data(), size_t(h->net_ptr[size_t(nets)]), s);
        if (!h->net_w.empty()) upload(d_cw, h->net_w.data(), size_t(nets), s);
        ek::dev::sweepw_spans(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_cw.as<int32_t>(),
                              st.pos.as<int32_t>(), ni, profw.as<u64>(), prof.as<unsigned>(), span.as<unsigned>());
        HIPCHK(hipGetLastError());
    }
    ek::dev::sweepw_scan(s, profw.as<u64>(), n + 1, tmp64.as<u64>());
    HIPCHK(hipGetLastError());
    ek::dev::sweep_scan(s, prof.as<unsigned>(), n + 1, true, st.scan_tmp.as<unsigned>());
    HIPCHK(hipGetLastError());
    if (!h->node_w.empty()) upload(d_w, h->node_w.data(), size_t(n), s);
    ek::dev::sweepw_gather(s, order, d_w.as<int32_t>(), ni, prefix.as<u64>());
    HIPCHK(hipGetLastError());
    ek::dev::sweepw_scan(s, prefix.as<u64>(), n + 1, tmp64.as<u64>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    r.t_profile = since(t);

    // choice
    t = clk::now();
    DBuf part, rec;
    part.ensure(size_t(5) * size_t(ek::dev::sweepw_select_blocks(ni)) * sizeof(u64));
    rec.ensure(ek::dev::SWEEPW_REC * sizeof(long long));
    ek::dev::sweepw_select(s, profw.as<u64>(), prefix.as<u64>(), prof.as<unsigned>(), ni, u64(r.total_weight),
                           u64(r.max_part), part.as<u64>(), span.as<unsigned>(), nspan, rec.as<long long>());
    HIPCHK(hipGetLastError());
    long long out[ek::dev::SWEEPW_REC] = {-1};
    HIPCHK(hipMemcpyAsync(out, rec.p, sizeof out, hipMemcpyDeviceToHost, s));
    if (order_out) HIPCHK(hipMemcpyAsync(order_out, order, size_t(n) * 4, hipMemcpyDeviceToHost, s));
    if (profile_out) HIPCHK(hipMemcpyAsync(profile_out, profw.p, words * 8, hipMemcpyDeviceToHost, s));
    if (prefix_out) HIPCHK(hipMemcpyAsync(prefix_out, prefix.p, words * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    r.t_select = since(t);
    if (out[0] < 1 || out[0] > n - 1)
        ek::fail(EK_EHIP, "weighted sweep cut: split %lld outside 1..%lld", out[0], (long long)(n - 1));
    if (out[1] != 0 && (out[0] < out[2] || out[0] > out[3]))
        ek::fail(EK_EHIP, "weighted sweep cut: split %lld outside the window [%lld, %lld]", out[0], out[2], out[3]);
    if (out[9] != r.total_weight)
        ek::fail(EK_EHIP, "weighted sweep cut: the prefix weights end at %lld, W = %lld", out[9], (long long)r.total_weight);
    r.n1 = out[0];
    r.n0 = n - out[0];
    r.feasible = out[1];
    r.s_lo = out[2];
    r.s_hi = out[3];
    r.cut = out[4];
    r.cut_nets = out[5];
    r.cut_half = out[6];
    r.spanning_nets = out[7];
    r.w1 = out[8];
    r.w0 = r.total_weight - out[8];
    if (result) *result = r;
}

}  // namespace

extern "C" {

int ek_sweep_cut_w(ek_ctx* c, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts, int32_t* order_out,
                   int64_t* profile_out, int64_t* prefix_out, ek_sweep_w_result* result) {
    EK_TRY
    check_ctx(c);
    ek_sweep_w_result r{};
    ek::sweepw_check("ek_sweep_cut_w", h, v_host, opts, r);
    DBuf v;
    upload(v, v_host, size_t(h->nodes), c->stream);
    sweepw_on_device(c, h, v.as<double>(), r, order_out, profile_out, prefix_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_fiedler_sweep_w(ek_ctx* c, const ek_hgr* h, const ek_sweep_opts* opts,
                                        ek_sweep_w_result* result) {
    EK_TRY
    check_ctx(c);
    if (c->nranks > 1)
        ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_sweep_w: a multi-rank context (%d ranks); the sweep runs on one",
                 c->nranks);
    if (!c->kl.graph_ready) ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_sweep_w before ek_kl_graph_setup");
    const int64_t n = c->kl.n;
    if (c->fied_n != n || n < 2)
        ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_sweep_w: no Fiedler vector of %lld entries on this context",
                 (long long)n);
    if (!h || h->nodes != n)
        ek::fail(EK_EINVAL, "ek_kl_set_partition_fiedler_sweep_w: a hypergraph of %lld nodes, the KL graph has %lld",
                 h ? (long long)h->nodes : 0ll, (long long)n);
    const double* v = c->fied.as<double>();
    ek_sweep_w_result r{};
    ek::sweepw_check("ek_kl_set_partition_fiedler_sweep_w", h, v, opts, r);
    sweepw_on_device(c, h, v, r, nullptr, nullptr, nullptr, &r);
    // the rank split at n1 = s*: the state ek_kl_set_partition_fiedler_rank leaves, by that call itself
    int64_t n0 = 0, n1 = 0;
    const int rc = ek_kl_set_partition_fiedler_rank(c, r.n1, &n0, &n1);
    if (rc != EK_OK) return rc;
    if (n1 != r.n1)
        ek::fail(EK_EHIP, "weighted sweep split: side 1 got %lld nodes, expected %lld", (long long)n1, (long long)r.n1);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
