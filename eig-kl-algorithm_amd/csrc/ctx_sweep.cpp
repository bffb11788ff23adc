// Sweep cut entries of libeigkl_hip.so, by net count and weighted
// (kernels_sweep.hip; the rules and the host checkers: sweep.cpp).
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
using u64 = unsigned long long;

// what the profile stage leaves on the device
struct SweepProfile {
    DBuf d_ptr, d_pins, d_cw, prof, profw, span, tmp64;
    int nspan = 0;  // words of span: 0 with no net
};

// The profile stage of both sweep cuts, enqueued on s after the sort st of h's
// n nodes: h's nets go up, the span kernel fills the count difference array
// (prof, n + 1 words, zero before) and span, and the scan turns prof into the
// count profile.  weighted: the net weights go up too, the same launch fills
// the int64 difference array (profw), and its scan, ahead of prof's, turns it
// into profile_w; tmp64 is left for further 64-bit scans over n + 1 words.
// No host synchronisation.
void sweep_profile(const SweepSort& st, const ek_hgr* h, hipStream_t s, bool weighted, SweepProfile& p) {
    const int64_t n = h->nodes, nets = h->nets;
    const size_t words = size_t(n) + 1;
    p.nspan = nets > 0 ? ek::dev::sweep_span_blocks(nets) : 0;
    if (weighted) {
        p.profw.ensure(words * sizeof(u64));
        p.tmp64.ensure(ek::dev::sweep_scan_tmp_words(n + 1) * sizeof(u64));
    }
    p.prof.ensure(words * sizeof(unsigned));
    p.span.ensure(size_t(std::max(p.nspan, 1)) * sizeof(unsigned));
    if (weighted) HIPCHK(hipMemsetAsync(p.profw.p, 0, words * sizeof(u64), s));
    HIPCHK(hipMemsetAsync(p.prof.p, 0, words * sizeof(unsigned), s));
    if (nets > 0) {
        upload(p.d_ptr, h->net_ptr.data(), size_t(nets) + 1, s);
        upload(p.d_pins, h->pins.data(), size_t(h->net_ptr[size_t(nets)]), s);
        if (weighted && !h->net_w.empty()) upload(p.d_cw, h->net_w.data(), size_t(nets), s);
        ek::dev::sweep_spans(s, nets, p.d_ptr.as<int64_t>(), p.d_pins.as<int32_t>(), st.pos.as<int32_t>(), int(n),
                             p.prof.as<unsigned>(), p.span.as<unsigned>(), p.d_cw.as<int32_t>(), p.profw.as<u64>());
        HIPCHK(hipGetLastError());
    }
    if (weighted) {
        ek::dev::sweep_scan(s, p.profw.as<u64>(), n + 1, true, p.tmp64.as<u64>());
        HIPCHK(hipGetLastError());
    }
    ek::dev::sweep_scan(s, p.prof.as<unsigned>(), n + 1, true, st.scan_tmp.as<unsigned>());
    HIPCHK(hipGetLastError());
}

// The sweep cut of v (device, n doubles) over h's nets.  Every buffer is local
// to the call.  Host synchronisations: the sort's two, one after the profile
// (for its time), one for the 32-byte result record; order and profile are
// read only when asked for.
void sweep_on_device(ek_ctx* c, const ek_hgr* h, const double* v, const ek_sweep_opts& o, int32_t* order_out,
                     int32_t* profile_out, ek_sweep_result* result) {
    hipStream_t s = c->stream;
    const int64_t n = h->nodes;
    ek_sweep_result r{};
    ek::sweep_window(n, o.imbalance, r);

    // sort
    auto t = clk::now();
    SweepSort st;
    sweep_sort(c, v, n, st);
    r.t_sort = since(t);

    // profile
    t = clk::now();
    SweepProfile pf;
    sweep_profile(st, h, s, false, pf);
    HIPCHK(hipStreamSynchronize(s));
    r.t_profile = since(t);

    // choice
    t = clk::now();
    DBuf part, rec;
    part.ensure(size_t(2) * size_t(ek::dev::sweep_select_blocks(r.s_hi - r.s_lo + 1)) * sizeof(unsigned));
    rec.ensure(4 * sizeof(long long));
    ek::dev::sweep_select(s, pf.prof.as<unsigned>(), int(n), r.s_lo, r.s_hi, o.objective, part.as<unsigned>(),
                          pf.span.as<unsigned>(), pf.nspan, rec.as<long long>());
    HIPCHK(hipGetLastError());
    long long out[4] = {-1, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, rec.p, sizeof out, hipMemcpyDeviceToHost, s));
    if (order_out) HIPCHK(hipMemcpyAsync(order_out, st.order(), size_t(n) * 4, hipMemcpyDeviceToHost, s));
    if (profile_out) HIPCHK(hipMemcpyAsync(profile_out, pf.prof.p, (size_t(n) + 1) * 4, hipMemcpyDeviceToHost, s));
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

// The weighted sweep cut of v (device, n doubles) over h's nets and weights
// under the sides' bounds l0, l1; r comes from sweepw_check (n, W, L_max = l0 =
// l1) or sweepwb_check (n, W, L0, L1).  Every buffer is local to the call.
// Host synchronisations: the sort's two, one after the profiles and P (for
// their time), one for the 80-byte result record; order, profile_w and P are
// read only when asked for.
template <class R>
void sweepw_on_device(ek_ctx* c, const ek_hgr* h, const double* v, R r, int64_t l0, int64_t l1, int32_t* order_out,
                      int64_t* profile_out, int64_t* prefix_out, R* result) {
    hipStream_t s = c->stream;
    const int64_t n = h->nodes;
    const int ni = int(n);
    const size_t words = size_t(n) + 1;

    // sort
    auto t = clk::now();
    SweepSort st;
    sweep_sort(c, v, n, st);
    r.t_sort = since(t);

    // the two profiles and the prefix weight
    t = clk::now();
    SweepProfile pf;
    DBuf d_w, prefix;
    prefix.ensure(words * sizeof(u64));
    sweep_profile(st, h, s, true, pf);
    if (!h->node_w.empty()) upload(d_w, h->node_w.data(), size_t(n), s);
    ek::dev::sweepw_gather(s, st.order(), d_w.as<int32_t>(), ni, prefix.as<u64>());
    HIPCHK(hipGetLastError());
    ek::dev::sweep_scan(s, prefix.as<u64>(), n + 1, true, pf.tmp64.as<u64>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    r.t_profile = since(t);

    // choice
    t = clk::now();
    DBuf part, rec;
    part.ensure(size_t(5) * size_t(ek::dev::sweepw_select_blocks(ni)) * sizeof(u64));
    rec.ensure(ek::dev::SWEEPW_REC * sizeof(long long));
    ek::dev::sweepw_select(s, pf.profw.as<u64>(), prefix.as<u64>(), pf.prof.as<unsigned>(), ni, u64(r.total_weight),
                           u64(l0), u64(l1), part.as<u64>(), pf.span.as<unsigned>(), pf.nspan, rec.as<long long>());
    HIPCHK(hipGetLastError());
    long long out[ek::dev::SWEEPW_REC] = {-1};
    HIPCHK(hipMemcpyAsync(out, rec.p, sizeof out, hipMemcpyDeviceToHost, s));
    if (order_out) HIPCHK(hipMemcpyAsync(order_out, st.order(), size_t(n) * 4, hipMemcpyDeviceToHost, s));
    if (profile_out) HIPCHK(hipMemcpyAsync(profile_out, pf.profw.p, words * 8, hipMemcpyDeviceToHost, s));
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

// What the two ek_kl_set_partition_fiedler_sweep* entries ask of the context
// and of h before they sweep; returns the context's Fiedler vector (device)
const double* sweep_split_vector(const char* who, ek_ctx* c, const ek_hgr* h) {
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "%s: a multi-rank context (%d ranks); the sweep runs on one", who, c->nranks);
    if (!c->kl.graph_ready) ek::fail(EK_ESTATE, "%s before ek_kl_graph_setup", who);
    const int64_t n = c->kl.n;
    if (c->fied_n != n || n < 2)
        ek::fail(EK_ESTATE, "%s: no Fiedler vector of %lld entries on this context", who, (long long)n);
    if (!h || h->nodes != n)
        ek::fail(EK_EINVAL, "%s: a hypergraph of %lld nodes, the KL graph has %lld", who, h ? (long long)h->nodes : 0ll,
                 (long long)n);
    return c->fied.as<double>();
}

// the rank split at n1 = s*: the state ek_kl_set_partition_fiedler_rank
// leaves, by that call itself; what: "sweep split" or "weighted sweep split"
int sweep_split_at(ek_ctx* c, const char* what, int64_t s_star) {
    int64_t n0 = 0, n1 = 0;
    const int rc = ek_kl_set_partition_fiedler_rank(c, s_star, &n0, &n1);
    if (rc != EK_OK) return rc;
    if (n1 != s_star) ek::fail(EK_EHIP, "%s: side 1 got %lld nodes, expected %lld", what, (long long)n1, (long long)s_star);
    return EK_OK;
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

int ek_sweep_cut_w(ek_ctx* c, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts, int32_t* order_out,
                   int64_t* profile_out, int64_t* prefix_out, ek_sweep_w_result* result) {
    EK_TRY
    check_ctx(c);
    ek_sweep_w_result r{};
    ek::sweepw_check("ek_sweep_cut_w", h, v_host, opts, r);
    DBuf v;
    upload(v, v_host, size_t(h->nodes), c->stream);
    sweepw_on_device(c, h, v.as<double>(), r, r.max_part, r.max_part, order_out, profile_out, prefix_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_sweep_cut_wb(ek_ctx* c, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts, const int64_t bounds[2],
                    int32_t* order_out, int64_t* profile_out, int64_t* prefix_out, ek_sweep_wb_result* result) {
    EK_TRY
    check_ctx(c);
    ek_sweep_wb_result r{};
    ek::sweepwb_check("ek_sweep_cut_wb", h, v_host, opts, bounds, r);
    DBuf v;
    upload(v, v_host, size_t(h->nodes), c->stream);
    sweepw_on_device(c, h, v.as<double>(), r, r.bound0, r.bound1, order_out, profile_out, prefix_out, result);
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_fiedler_sweep(ek_ctx* c, const ek_hgr* h, const ek_sweep_opts* opts, ek_sweep_result* result) {
    EK_TRY
    const double* v = sweep_split_vector("ek_kl_set_partition_fiedler_sweep", c, h);
    const ek_sweep_opts o = ek::sweep_check("ek_kl_set_partition_fiedler_sweep", h, v, opts);
    ek_sweep_result r{};
    sweep_on_device(c, h, v, o, nullptr, nullptr, &r);
    const int rc = sweep_split_at(c, "sweep split", r.n1);
    if (rc != EK_OK) return rc;
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_fiedler_sweep_w(ek_ctx* c, const ek_hgr* h, const ek_sweep_opts* opts,
                                        ek_sweep_w_result* result) {
    EK_TRY
    const double* v = sweep_split_vector("ek_kl_set_partition_fiedler_sweep_w", c, h);
    ek_sweep_w_result r{};
    ek::sweepw_check("ek_kl_set_partition_fiedler_sweep_w", h, v, opts, r);
    sweepw_on_device(c, h, v, r, r.max_part, r.max_part, nullptr, nullptr, nullptr, &r);
    const int rc = sweep_split_at(c, "weighted sweep split", r.n1);
    if (rc != EK_OK) return rc;
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"

