// Sweep cut entries of libeigkl_hip.so (kernels_sweep.hip; the rule and the
// host checker: sweep.cpp).
#include "ctx.hpp"

using namespace ek::rt;

// The stable radix sort of the n keys (ord(v[i]), i) and its inverse, for both
// sweep cuts.  One host synchronisation inside: the 8-KiB read of the passes'
// digit counts (a pass whose digit all keys share is skipped); one at the end.
void ek::rt::sweep_sort(ek_ctx* c, const double* v, int64_t n, SweepSort& out) {
    hipStream_t s = c->stream;
    const int ni = int(n);
    const int nt = ek::dev::sweep_tiles(ni);
    const long long table_words = 256ll * nt;
    DBuf (&keys)[2] = out.keys, (&ids)[2] = out.ids;
    DBuf &ghist = out.ghist, &table = out.table, &scan_tmp = out.scan_tmp, &pos = out.pos;
    for (int b = 0; b < 2; ++b) {
        keys[b].ensure(size_t(n) * 8);
        ids[b].ensure(size_t(n) * 4);
    }
    ghist.ensure(8 * 256 * sizeof(unsigned));
    table.ensure(size_t(table_words) * sizeof(unsigned));
    scan_tmp.ensure(std::max(ek::dev::sweep_scan_tmp_words(table_words), ek::dev::sweep_scan_tmp_words(n + 1)) *
                    sizeof(unsigned));
    pos.ensure(size_t(n) * 4);
    HIPCHK(hipMemsetAsync(ghist.p, 0, 8 * 256 * sizeof(unsigned), s));
    ek::dev::sweep_keys(s, v, ni, keys[0].as<unsigned long long>(), ids[0].as<int32_t>(), ghist.as<unsigned>());
    HIPCHK(hipGetLastError());
    std::vector<unsigned> gh(8 * 256);
    HIPCHK(hipMemcpyAsync(gh.data(), ghist.p, gh.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int cur = 0;
    for (int pass = 0; pass < 8; ++pass) {
        int64_t total = 0;
        bool one_digit = false;
        for (int d = 0; d < 256; ++d) {
            total += gh[size_t(pass) * 256 + size_t(d)];
            one_digit = one_digit || int64_t(gh[size_t(pass) * 256 + size_t(d)]) == n;
        }
        if (total != n) ek::fail(EK_EHIP, "sweep sort: pass %d counted %lld of %lld keys", pass, (long long)total, (long long)n);
        if (one_digit) continue;  // the pass would move nothing
        ek::dev::sweep_sort_pass(s, ni, pass, keys[cur].as<unsigned long long>(), ids[cur].as<int32_t>(),
                                 keys[cur ^ 1].as<unsigned long long>(), ids[cur ^ 1].as<int32_t>(),
                                 table.as<unsigned>(), scan_tmp.as<unsigned>());
        HIPCHK(hipGetLastError());
        cur ^= 1;
    }
    out.cur = cur;
    ek::dev::sweep_pos(s, out.order(), ni, pos.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
}

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

// The sweep cut of v (device, n doubles) over h's nets.  Every buffer is local
// to the call.  Host synchronisations: one 8-KiB read of the passes' digit
// counts (a pass whose digit all keys share is skipped), one after the
// profile (for its time), one for the 32-byte result record; order and
// profile are read only when asked for.
void sweep_on_device(ek_ctx* c, const ek_hgr* h, const double* v, const ek_sweep_opts& o, int32_t* order_out,
                     int32_t* profile_out, ek_sweep_result* result) {
    hipStream_t s = c->stream;
    const int64_t n = h->nodes;
    const int ni = int(n);
    ek_sweep_result r{};
    ek::sweep_window(n, o.imbalance, r);

    // sort
    auto t = clk::now();
    SweepSort st;
    sweep_sort(c, v, n, st);
    const int32_t* order = st.order();
    DBuf &scan_tmp = st.scan_tmp, &pos = st.pos;
    r.t_sort = since(t);

    // profile
    t = clk::now();
    DBuf d_ptr, d_pins, prof, span;
    const int64_t nets = h->nets;
    const int nspan = nets > 0 ? ek::dev::sweep_span_blocks(nets) : 0;
    prof.ensure((size_t(n) + 1) * sizeof(unsigned));
    span.ensure(size_t(std::max(nspan, 1)) * sizeof(unsigned));
    HIPCHK(hipMemsetAsync(prof.p, 0, (size_t(n) + 1) * sizeof(unsigned), s));
    if (nets > 0) {
        upload(d_ptr, h->net_ptr.data(), size_t(nets) + 1, s);
        upload(d_pins, h->pins.data(), size_t(h->net_ptr[size_t(nets)]), s);
        ek::dev::sweep_spans(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), pos.as<int32_t>(), ni,
                             prof.as<unsigned>(), span.as<unsigned>());
        HIPCHK(hipGetLastError());
    }
    ek::dev::sweep_scan(s, prof.as<unsigned>(), n + 1, true, scan_tmp.as<unsigned>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    r.t_profile = since(t);

    // choice
    t = clk::now();
    DBuf part, rec;
    part.ensure(size_t(2) * size_t(ek::dev::sweep_select_blocks(r.s_hi - r.s_lo + 1)) * sizeof(unsigned));
    rec.ensure(4 * sizeof(long long));
    ek::dev::sweep_select(s, prof.as<unsigned>(), ni, r.s_lo, r.s_hi, o.objective, part.as<unsigned>(),
                          span.as<unsigned>(), nspan, rec.as<long long>());
    HIPCHK(hipGetLastError());
    long long out[4] = {-1, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, rec.p, sizeof out, hipMemcpyDeviceToHost, s));
    if (order_out) HIPCHK(hipMemcpyAsync(order_out, order, size_t(n) * 4, hipMemcpyDeviceToHost, s));
    if (profile_out) HIPCHK(hipMemcpyAsync(profile_out, prof.p, (size_t(n) + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    r.t_select = since(t);
    if (out[0] < r.s_lo || out[0] > r.s_hi)
        ek::fail(EK_EHIP, "sweep cut: split %lld outside the window [%lld, %lld]", out[0], (long long)r.s_lo,
                 (long long)r.s_hi);
    r.n1 = out[0];
    r.n0 = n - out[0];
    r.cut = out[1];
    r.cut_mid = out[2];
    r.spanning_nets = out[3];
    if (result) *result = r;
}

}  // namespace

extern "C" {

int ek_sweep_cut(ek_ctx* c, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts, int32_t* order_out,
                 int32_t* profile_out, ek_sweep_result* result) {
    EK_TRY
    check_ctx(c);
    const ek_sweep_opts o = ek::sweep_check("ek_sweep_cut", h, v_host, opts);
    DBuf v;
    upload(v, v_host, size_t(h->nodes), c->stream);
    sweep_on_device(c, h, v.as<double>(), o, order_out, profile_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_fiedler_sweep(ek_ctx* c, const ek_hgr* h, const ek_sweep_opts* opts, ek_sweep_result* result) {
    EK_TRY
    check_ctx(c);
    if (c->nranks > 1)
        ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_sweep: a multi-rank context (%d ranks); the sweep runs on one",
                 c->nranks);
    if (!c->kl.graph_ready) ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_sweep before ek_kl_graph_setup");
    const int64_t n = c->kl.n;
    if (c->fied_n != n || n < 2)
        ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_sweep: no Fiedler vector of %lld entries on this context",
                 (long long)n);
    if (!h || h->nodes != n)
        ek::fail(EK_EINVAL, "ek_kl_set_partition_fiedler_sweep: a hypergraph of %lld nodes, the KL graph has %lld",
                 h ? (long long)h->nodes : 0ll, (long long)n);
    const double* v = c->fied.as<double>();
    const ek_sweep_opts o = ek::sweep_check("ek_kl_set_partition_fiedler_sweep", h, v, opts);
    ek_sweep_result r{};
    sweep_on_device(c, h, v, o, nullptr, nullptr, &r);
    // the rank split at n1 = s*: the state ek_kl_set_partition_fiedler_rank leaves, by that call itself
    int64_t n0 = 0, n1 = 0;
    const int rc = ek_kl_set_partition_fiedler_rank(c, r.n1, &n0, &n1);
    if (rc != EK_OK) return rc;
    if (n1 != r.n1) ek::fail(EK_EHIP, "sweep split: side 1 got %lld nodes, expected %lld", (long long)n1, (long long)r.n1);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
