// The device contraction entry of libeigkl_hip.so (ek_hgr_contract_device;
// kernels_contract.hip; the rule and the host path: match.cpp ek_hgr_contract).
#include "ctx.hpp"

using namespace ek::rt;

extern "C" {

void ek_contract_default_opts(ek_contract_opts* o) {
    if (!o) return;
    o->hash_bits = 64;
    o->pad = 0;
}

// The fine hypergraph, the map and the weights go up, the launches of
// kernels_contract.hip follow on the context's stream, and the host reads twice:
// the error counters with the coarse net and pin counts, then the coarse arrays
// at those sizes.  One device allocation holds every buffer and is local to the
// call: the context keeps nothing.
int ek_hgr_contract_device(ek_ctx* c, const ek_hgr* h, const int32_t* cluster, int64_t n_coarse,
                           const ek_contract_opts* opts, ek_hgr** out) {
    EK_TRY
    check_ctx(c);
    if (c->nranks > 1)
        ek::fail(EK_ESTATE, "ek_hgr_contract_device: a multi-rank context (%d ranks); the contraction runs on one", c->nranks);
    if (!h || !out || (h->nodes > 0 && !cluster)) ek::fail(EK_EINVAL, "ek_hgr_contract_device: null argument");
    ek_contract_opts o;
    ek_contract_default_opts(&o);
    if (opts) o = *opts;
    if (o.hash_bits < 1 || o.hash_bits > 64)
        ek::fail(EK_EINVAL, "ek_hgr_contract_device: hash_bits %d outside [1, 64]", int(o.hash_bits));
    const int64_t n = h->nodes, nets = h->nets;
    if (n_coarse < 0 || n_coarse > n)
        ek::fail(EK_EINVAL, "ek_hgr_contract_device: %lld clusters of %lld nodes", (long long)n_coarse, (long long)n);
    if (n > INT32_MAX - 1 || nets > INT32_MAX - 1)
        ek::fail(EK_EINVAL, "ek_hgr_contract_device: %lld nodes, %lld nets", (long long)n, (long long)nets);
    for (int64_t v = 0; v < n; ++v)  // (the kernels index by it)
        if (cluster[v] < 0 || cluster[v] >= n_coarse)
            ek::fail(EK_EINVAL, "ek_hgr_contract_device: cluster %d of node %lld outside [0, %lld)", cluster[v], (long long)v,
                     (long long)n_coarse);
    auto res = std::make_unique<ek_hgr>();
    res->nodes = n_coarse;
    res->net_ptr.assign(1, 0);
    if (n == 0) {  // no node, so no pin: every net is dropped
        *out = res.release();
        return EK_OK;
    }
    const int64_t raw = nets > 0 ? h->net_ptr[size_t(nets)] : 0;
    const bool with_nets = nets > 0 && raw > 0;
    const bool has_w = !h->node_w.empty(), has_cw = !h->net_w.empty();

    // one allocation; the words that must be zero first, side by side
    size_t bytes = 0;
    auto take = [&](size_t b) {
        const size_t at = bytes;
        bytes += (b + 255) / 256 * 256;
        return at;
    };
    const size_t un = size_t(n), unc = size_t(n_coarse), une = with_nets ? size_t(nets) : 0, uraw = with_nets ? size_t(raw) : 0;
    const int nt = with_nets ? ek::dev::sweep_tiles(int(nets)) : 0;
    const size_t table_words = 256 * size_t(nt);
    const size_t z_wsum = take(unc * 8), z_hits = take(unc * 4), z_csum = take(une * 8), z_err = take(16);
    const size_t zero_bytes = bytes;
    const size_t a_cluster = take(un * 4), a_w = take(has_w ? un * 4 : 0), a_node_w = take(unc * 4);
    const size_t a_ptr = take((une + 1) * 8), a_pins = take(uraw * 4), a_cw = take(has_cw ? une * 4 : 0);
    const size_t a_dpins = take(uraw * 4), a_dsz = take(une * 4);
    const size_t a_key0 = take(une * 8), a_key1 = take(une * 8), a_id0 = take(une * 4), a_id1 = take(une * 4);
    const size_t a_table = take(table_words * 4), a_scan = take(ek::dev::sweep_scan_tmp_words((long long)table_words) * 4);
    const size_t a_keep = take(une * 4), a_ksz = take(une * 4), a_idx = take((une + 1) * 8), a_off = take((une + 1) * 8);
    const size_t a_tiles = take(((une + 1023) / 1024 + 1) * 8);
    const size_t a_optr = take(une * 8), a_opins = take(uraw * 4), a_ow = take(une * 4);
    DBuf arena;
    arena.ensure(bytes);
    char* base = arena.as<char>();
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(base, 0, zero_bytes, s));
    auto up = [&](size_t at, const void* src, size_t b) {
        if (b) HIPCHK(hipMemcpyAsync(base + at, src, b, hipMemcpyHostToDevice, s));
    };
    up(a_cluster, cluster, un * 4);
    if (has_w) up(a_w, h->node_w.data(), un * 4);
    if (with_nets) {
        up(a_ptr, h->net_ptr.data(), (une + 1) * 8);
        up(a_pins, h->pins.data(), uraw * 4);
        if (has_cw) up(a_cw, h->net_w.data(), une * 4);
    }
    ek::dev::ContractDev d{};
    d.n = int(n);
    d.nc = int(n_coarse);
    d.nets = int(une);
    d.hash_bits = o.hash_bits;
    d.net_ptr = reinterpret_cast<const int64_t*>(base + a_ptr);
    d.pins = reinterpret_cast<const int32_t*>(base + a_pins);
    d.cluster = reinterpret_cast<const int32_t*>(base + a_cluster);
    d.w = has_w ? reinterpret_cast<const int32_t*>(base + a_w) : nullptr;
    d.cw = has_cw ? reinterpret_cast<const int32_t*>(base + a_cw) : nullptr;
    d.wsum = reinterpret_cast<unsigned long long*>(base + z_wsum);
    d.hits = reinterpret_cast<int*>(base + z_hits);
    d.node_w = reinterpret_cast<int32_t*>(base + a_node_w);
    d.dpins = reinterpret_cast<int32_t*>(base + a_dpins);
    d.dsz = reinterpret_cast<int*>(base + a_dsz);
    d.key[0] = reinterpret_cast<unsigned long long*>(base + a_key0);
    d.key[1] = reinterpret_cast<unsigned long long*>(base + a_key1);
    d.ids[0] = reinterpret_cast<int32_t*>(base + a_id0);
    d.ids[1] = reinterpret_cast<int32_t*>(base + a_id1);
    d.table = reinterpret_cast<unsigned*>(base + a_table);
    d.scan_tmp = reinterpret_cast<unsigned*>(base + a_scan);
    d.csum = reinterpret_cast<unsigned long long*>(base + z_csum);
    d.keep = reinterpret_cast<int*>(base + a_keep);
    d.ksz = reinterpret_cast<int*>(base + a_ksz);
    d.idx = reinterpret_cast<long long*>(base + a_idx);
    d.off = reinterpret_cast<long long*>(base + a_off);
    d.tiles = reinterpret_cast<long long*>(base + a_tiles);
    d.out_ptr = reinterpret_cast<int64_t*>(base + a_optr);
    d.out_pins = reinterpret_cast<int32_t*>(base + a_opins);
    d.out_w = reinterpret_cast<int32_t*>(base + a_ow);
    d.err = reinterpret_cast<int*>(base + z_err);
    ek::dev::contract_nodes(s, d);
    HIPCHK(hipGetLastError());
    if (with_nets) {
        ek::dev::contract_nets(s, d);
        HIPCHK(hipGetLastError());
    }
    int err[3] = {0, 0, 0};
    long long kept = 0, kept_pins = 0;
    HIPCHK(hipMemcpyAsync(err, d.err, sizeof err, hipMemcpyDeviceToHost, s));
    if (with_nets) {
        HIPCHK(hipMemcpyAsync(&kept, d.idx + une, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&kept_pins, d.off + une, 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (err[0]) ek::fail(EK_EINVAL, "ek_hgr_contract_device: no node maps to %d of the %lld clusters", err[0], (long long)n_coarse);
    if (err[1]) ek::fail(EK_EINVAL, "ek_hgr_contract_device: %d clusters weigh more than 2^31 - 1", err[1]);
    if (err[2]) ek::fail(EK_EINVAL, "ek_hgr_contract_device: %d merged nets weigh more than 2^31 - 1", err[2]);
    if (kept < 0 || kept > nets || kept_pins < 0 || kept_pins > raw)
        ek::fail(EK_EHIP, "ek_hgr_contract_device: %lld nets of %lld pins out of %lld of %lld", kept, kept_pins,
                 (long long)nets, (long long)raw);
    res->nets = kept;
    res->node_w.resize(unc);
    res->net_ptr.resize(size_t(kept) + 1);
    res->pins.resize(size_t(kept_pins));
    res->net_w.resize(size_t(kept));
    HIPCHK(hipMemcpyAsync(res->node_w.data(), d.node_w, unc * 4, hipMemcpyDeviceToHost, s));
    if (kept) {
        HIPCHK(hipMemcpyAsync(res->net_ptr.data(), d.out_ptr, size_t(kept) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(res->pins.data(), d.out_pins, size_t(kept_pins) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(res->net_w.data(), d.out_w, size_t(kept) * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    res->net_ptr[size_t(kept)] = kept_pins;
    *out = res.release();
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
