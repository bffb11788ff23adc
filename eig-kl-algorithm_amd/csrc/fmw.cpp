// The weighted Fiduccia-Mattheyses refinement (node weights under the balance
// bound, net weights in the cut): its input and its metrics.
//
// fmw_prepare is all that the weighted checker and the weighted device path
// (fm.cpp, ctx_fm.cpp) share; ek_fm_refine_host and ek_fm_refine never call
// it and ignore the weights.  Its part that needs no sides, weights_prepare,
// is also the matching's input (match.cpp).  ek_bipart_metrics_host is written apart from
// the FM code: it walks the hypergraph's own pins, not the prepared input.
#include <algorithm>
#include <vector>

#include "ek_internal.hpp"

namespace {
constexpr int64_t W_LIMIT = int64_t(1) << 62;  // of W and of the sum of all c(e)
}  // namespace

namespace ek {

int64_t weights_prepare(const char* who, const ek_hgr* h, WeightedInput& out) {
    refine_prepare(*h, out.in);
    const int64_t n = h->nodes, nets = int64_t(out.in.net_ptr.size()) - 1;
    // c(e) of the participating nets: refine_prepare keeps, in file order, the nets of >= 2 distinct pins
    out.cw.assign(size_t(nets), 1);
    if (!h->net_w.empty()) {
        std::vector<int64_t> stamp(size_t(n), -1);
        int64_t at = 0;
        for (int64_t e = 0; e < h->nets; ++e) {
            int distinct = 0;
            for (int64_t p = h->net_ptr[size_t(e)]; p < h->net_ptr[size_t(e) + 1] && distinct < 2; ++p) {
                const int32_t v = h->pins[size_t(p)];
                if (stamp[size_t(v)] == e) continue;
                stamp[size_t(v)] = e;
                ++distinct;
            }
            if (distinct >= 2) out.cw[size_t(at++)] = h->net_w[size_t(e)];
        }
        if (at != nets) fail(EK_EINVAL, "%s: %lld participating nets, %lld weights", who, (long long)nets, (long long)at);
    }
    if (h->node_w.empty()) out.w.assign(size_t(n), 1);
    else out.w = h->node_w;
    int64_t total = 0, csum = 0;
    for (int64_t v = 0; v < n; ++v) {
        if (out.w[size_t(v)] < 0) fail(EK_EINVAL, "%s: weight %d of node %lld", who, out.w[size_t(v)], (long long)v);
        total += out.w[size_t(v)];
    }
    for (int64_t e = 0; e < nets; ++e) {
        if (out.cw[size_t(e)] < 1) fail(EK_EINVAL, "%s: net weight %d", who, out.cw[size_t(e)]);
        csum += out.cw[size_t(e)];
    }
    // (int32 weights over fewer than 2^31 nodes and nets stay below both limits; the rule states them all the same)
    if (total > W_LIMIT || csum > W_LIMIT) fail(EK_EINVAL, "%s: total weight above 2^62", who);
    for (int64_t v = 0; v < n; ++v) {
        int64_t on = 0;
        for (int64_t i = out.in.inc_ptr[size_t(v)]; i < out.in.inc_ptr[size_t(v) + 1]; ++i)
            on += out.cw[size_t(out.in.inc[size_t(i)])];
        if (on > INT32_MAX)
            fail(EK_EINVAL, "%s: the nets on node %lld weigh %lld (at most 2^31 - 1: gains are int32)", who, (long long)v,
                 (long long)on);
    }
    return total;
}

void fmw_prepare(const char* who, const ek_hgr* h, const ek_fm_opts* opts, const uint8_t* side, FmwInput& out) {
    out.opts = fm_check(who, h, opts, side);
    out.total = weights_prepare(who, h, out);
    out.max_part = refine_max_part(out.total, 2, out.opts.imbalance);
}

void fmwb_prepare(const char* who, const ek_hgr* h, const ek_fm_opts* opts, const int64_t bounds[2], const uint8_t* side,
                  FmwInput& out) {
    ek_fm_opts o;
    ek_fm_default_opts(&o);
    if (opts) o = *opts;
    o.imbalance = 0.0;  // ignored: the bounds stand in its place
    if (!bounds) fail(EK_EINVAL, "%s: null bounds", who);
    out.opts = fm_check(who, h, &o, side);
    out.total = weights_prepare(who, h, out);
    bounds_check(who, out.total, bounds);
    out.max_part = std::max(bounds[0], bounds[1]);
}

}  // namespace ek

extern "C" {

int ek_bipart_metrics_host(const ek_hgr* h, const uint8_t* side, int64_t out[4]) {
    EK_TRY
    if (!h || !out || (h->nodes > 0 && !side)) ek::fail(EK_EINVAL, "ek_bipart_metrics_host: null argument");
    const int64_t n = h->nodes;
    int64_t m[4] = {0, 0, 0, 0};
    for (int64_t v = 0; v < n; ++v) {
        if (side[v] > 1) ek::fail(EK_EINVAL, "ek_bipart_metrics_host: side %d of node %lld outside {0, 1}", int(side[v]), (long long)v);
        m[2 + side[v]] += h->node_w.empty() ? 1 : h->node_w[size_t(v)];
    }
    std::vector<int64_t> last(size_t(n), -1);  // the last net that counted the node
    for (int64_t e = 0; e < h->nets; ++e) {
        int64_t on[2] = {0, 0};
        for (int64_t p = h->net_ptr[size_t(e)]; p < h->net_ptr[size_t(e) + 1]; ++p) {
            const int32_t v = h->pins[size_t(p)];
            if (last[size_t(v)] == e) continue;
            last[size_t(v)] = e;
            ++on[side[v]];
        }
        if (on[0] > 0 && on[1] > 0) {  // (a cut net has two distinct pins)
            m[0] += h->net_w.empty() ? 1 : h->net_w[size_t(e)];
            ++m[1];
        }
    }
    std::copy(m, m + 4, out);
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
