// k-way metrics and connectivity refinement entries of libeigkl_hip.so.
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

int ek_kway_metrics(ek_ctx* c, int64_t nets, const int64_t* net_ptr, const int32_t* pins, const int32_t* part_host,
                    int32_t k, int64_t out[3]) {
    EK_TRY
    check_ctx(c);
    if (nets < 0 || !net_ptr || !out || k < 1 || k > 256 || net_ptr[0] != 0 || (net_ptr[nets] > 0 && (!pins || !part_host)))
        ek::fail(EK_EINVAL, "ek_kway_metrics: bad argument");
    const int64_t npins = net_ptr[nets];
    for (int64_t e = 0; e < nets; ++e)
        if (net_ptr[e + 1] < net_ptr[e]) ek::fail(EK_EINVAL, "ek_kway_metrics: net_ptr not monotone");
    int32_t top = -1;
    for (int64_t p = 0; p < npins; ++p) {
        if (pins[p] < 0) ek::fail(EK_EINVAL, "ek_kway_metrics: pin %d", pins[p]);
        top = std::max(top, pins[p]);
    }
    out[0] = out[1] = out[2] = 0;
    if (nets == 0 || npins == 0) return EK_OK;
    const int64_t nodes = int64_t(top) + 1;
    std::vector<uint8_t> part8(static_cast<size_t>(nodes));
    for (int64_t i = 0; i < nodes; ++i) {
        if (part_host[i] < 0 || part_host[i] >= k)
            ek::fail(EK_EINVAL, "ek_kway_metrics: part %d of node %lld outside [0, %d)", part_host[i], (long long)i, k);
        part8[size_t(i)] = uint8_t(part_host[i]);
    }
    hipStream_t s = c->stream;
    const int nb = ek::dev::kway_metrics_blocks(nets);
    DBuf d_ptr, d_pins, d_part, d_out;
    upload(d_ptr, net_ptr, size_t(nets) + 1, s);
    upload(d_pins, pins, size_t(npins), s);
    upload(d_part, part8.data(), size_t(nodes), s);
    d_out.ensure(size_t(3) * size_t(nb) * sizeof(unsigned));
    ek::dev::kway_metrics(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_part.as<uint8_t>(), d_out.as<unsigned>());
    HIPCHK(hipGetLastError());
    std::vector<unsigned> parts(size_t(3) * size_t(nb));
    HIPCHK(hipMemcpyAsync(parts.data(), d_out.p, parts.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int j = 0; j < 3; ++j)
        for (int b = 0; b < nb; ++b) out[j] += int64_t(parts[size_t(j) * size_t(nb) + size_t(b)]);
    return EK_OK;
    EK_CATCH
}

// The weighted metrics on the device: two launches (the nets, the nodes) into
// one record of 4 + 256 int64 words, read once.  Every buffer is local to the
// call.
int ek_kway_metrics_w(ek_ctx* c, const ek_hgr* h, const int32_t* part, int32_t k, int64_t* out) {
    EK_TRY
    check_ctx(c);
    if (!h || !out || k < 1 || k > 256 || (h->nodes > 0 && !part)) ek::fail(EK_EINVAL, "ek_kway_metrics_w: bad argument");
    const int64_t n = h->nodes, nets = h->nets;
    if (n > INT32_MAX - 1) ek::fail(EK_EINVAL, "ek_kway_metrics_w: %lld nodes", (long long)n);
    if ((!h->node_w.empty() && int64_t(h->node_w.size()) != n) || (!h->net_w.empty() && int64_t(h->net_w.size()) != nets))
        ek::fail(EK_EINVAL, "ek_kway_metrics_w: weight arrays of the wrong length");
    std::vector<uint8_t> part8(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        if (part[i] < 0 || part[i] >= k)
            ek::fail(EK_EINVAL, "ek_kway_metrics_w: part %d of node %lld outside [0, %d)", part[i], (long long)i, k);
        part8[size_t(i)] = uint8_t(part[i]);
    }
    std::fill(out, out + 4 + k, int64_t(0));
    if (n == 0) return EK_OK;
    const int64_t npins = nets > 0 ? h->net_ptr[size_t(nets)] : 0;
    hipStream_t s = c->stream;
    constexpr size_t WORDS = 4 + 256;
    DBuf d_ptr, d_pins, d_cw, d_w, d_part, d_out;
    if (nets > 0) upload(d_ptr, h->net_ptr.data(), size_t(nets) + 1, s);
    if (npins > 0) upload(d_pins, h->pins.data(), size_t(npins), s);
    if (nets > 0 && !h->net_w.empty()) upload(d_cw, h->net_w.data(), size_t(nets), s);
    if (!h->node_w.empty()) upload(d_w, h->node_w.data(), size_t(n), s);
    upload(d_part, part8.data(), size_t(n), s);
    d_out.ensure(WORDS * sizeof(unsigned long long));
    HIPCHK(hipMemsetAsync(d_out.p, 0, WORDS * sizeof(unsigned long long), s));
    ek::dev::kway_metrics_w(s, npins > 0 ? nets : 0, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_cw.as<int32_t>(), n,
                            d_part.as<uint8_t>(), d_w.as<int32_t>(), d_out.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    long long got[WORDS];
    HIPCHK(hipMemcpyAsync(got, d_out.p, sizeof got, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int j = 0; j < 4 + k; ++j) out[j] = got[j];
    return EK_OK;
    EK_CATCH
}

// The k-way refinement on the device (kernels_refine.hip): six launches a
// round, then ONE 8-byte read (the round's accepted moves) to learn whether to
// go on.  The rounds' four counters stay in a device log of RF_LOG rounds,
// read in bulk when it is full and at the end.  Every buffer is local to the
// call: the context keeps nothing.
int ek_kway_refine(ek_ctx* c, const ek_hgr* h, const ek_kway_refine_opts* opts, int32_t* part, int64_t* round_log,
                   int64_t log_rounds, ek_kway_refine_result* result) {
    EK_TRY
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t0 = clk::now();
    check_ctx(c);
    if (c->nranks > 1)
        ek::fail(EK_ESTATE, "ek_kway_refine: a multi-rank context (%d ranks); k-way runs on one", c->nranks);
    const ek_kway_refine_opts o = ek::refine_check("ek_kway_refine", h, opts, part);
    const int64_t n = h->nodes;
    ek::RefineInput in;
    ek::refine_prepare(*h, in);
    const int64_t nets = int64_t(in.net_ptr.size()) - 1;
    ek_kway_refine_result r{};
    r.k = o.k;
    r.max_part = ek::refine_max_part(n, o.k, o.imbalance);
    std::vector<int> sizes(256, 0);
    for (int64_t i = 0; i < n; ++i) ++sizes[size_t(part[i])];
    auto minmax = [&] {
        r.part_min = *std::min_element(sizes.begin(), sizes.begin() + o.k);
        r.part_max = *std::max_element(sizes.begin(), sizes.begin() + o.k);
    };
    minmax();
    if (nets == 0) {  // nothing to refine, nothing cut
        r.t_setup = since(t0);
        if (result) *result = r;
        return EK_OK;
    }
    hipStream_t s = c->stream;
    std::vector<uint8_t> part8(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) part8[size_t(i)] = uint8_t(part[i]);
    constexpr int64_t RF_LOG = 1024;
    DBuf d_ptr, d_pins, d_iptr, d_inc, d_part, d_sizes, d_masks, d_key, d_win, d_list, d_thr, d_tgt, d_log, d_met;
    upload(d_ptr, in.net_ptr.data(), in.net_ptr.size(), s);
    upload(d_pins, in.pins.data(), in.pins.size(), s);
    upload(d_iptr, in.inc_ptr.data(), in.inc_ptr.size(), s);
    upload(d_inc, in.inc.data(), in.inc.size(), s);
    upload(d_part, part8.data(), part8.size(), s);
    upload(d_sizes, sizes.data(), sizes.size(), s);
    d_masks.ensure(size_t(nets) * 64);
    d_key.ensure(size_t(n) * 8);
    d_win.ensure(size_t(nets) * 8);
    d_list.ensure(size_t(n) * 8);
    d_thr.ensure(256 * 8);
    d_tgt.ensure(size_t(n));
    d_log.ensure(size_t(RF_LOG) * 32);
    HIPCHK(hipMemsetAsync(d_log.p, 0, size_t(RF_LOG) * 32, s));
    const int nb = ek::dev::kway_metrics_blocks(nets);
    d_met.ensure(size_t(3) * size_t(nb) * sizeof(unsigned));
    std::vector<unsigned> partial(size_t(3) * size_t(nb));
    auto metrics = [&](int64_t m[3]) {
        ek::dev::kway_metrics(s, nets, d_ptr.as<int64_t>(), d_pins.as<int32_t>(), d_part.as<uint8_t>(),
                              d_met.as<unsigned>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(partial.data(), d_met.p, partial.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int j = 0; j < 3; ++j) {
            m[j] = 0;
            for (int b = 0; b < nb; ++b) m[j] += int64_t(partial[size_t(j) * size_t(nb) + size_t(b)]);
        }
    };
    int64_t m[3];
    metrics(m);
    r.connectivity_before = m[1];
    r.t_setup = since(t0);

    const auto tr = clk::now();
    ek::dev::RefineDev d{};
    d.n = int(n);
    d.nets = int(nets);
    d.k = o.k;
    d.lmax = int(std::min<int64_t>(r.max_part, INT32_MAX));
    d.net_ptr = d_ptr.as<int64_t>();
    d.inc_ptr = d_iptr.as<int64_t>();
    d.pins = d_pins.as<int32_t>();
    d.inc = d_inc.as<int32_t>();
    d.part = d_part.as<uint8_t>();
    d.sizes = d_sizes.as<int>();
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
        ek::dev::refine_round(s, d, slot);
        HIPCHK(hipGetLastError());
        unsigned long long accepted = 0;
        HIPCHK(hipMemcpyAsync(&accepted, slot + 2, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (accepted == 0) break;
        // every moving round lowers the connectivity by at least 1
        if (r.rounds >= r.connectivity_before || r.rounds == INT32_MAX)
            ek::fail(EK_EHIP, "ek_kway_refine: %d rounds moved from a connectivity of %lld", r.rounds + 1,
                     (long long)r.connectivity_before);
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
    HIPCHK(hipMemcpyAsync(sizes.data(), d_sizes.p, sizes.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    metrics(m);  // (drains the stream: the two copies have landed)
    for (int64_t i = 0; i < n; ++i) part[i] = part8[size_t(i)];
    minmax();
    r.cut_nets = m[0];
    r.connectivity = m[1];
    r.soed = m[2];
    r.t_metrics = since(tm);
    if (result) *result = r;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
