// KL driver of libeigkl_hip.so: graph and net setup, the device median and
// rank splits, the swap loop's run and its sides.
#include "ctx.hpp"

using namespace ek::rt;

// ---------------------------------------------------------------------------
// KL driver (KL(), cKL.cpp:288-406)
extern "C" {

int ek_kl_graph_setup(ek_ctx* c, int64_t n, const int32_t* rowptr, const int32_t* col, const float* w) {
    EK_TRY
    check_ctx(c);
    ek::PhaseTimer pt("kl_graph_setup");
    if (n <= 0 || n > INT32_MAX || !rowptr || !col || !w) ek::fail(EK_EINVAL, "ek_kl_graph_setup: bad argument");
    const int64_t nnz = rowptr[n];
    for (int64_t r = 0; r < n; ++r)
        if (rowptr[r + 1] < rowptr[r]) ek::fail(EK_EINVAL, "ek_kl_graph_setup: rowptr not monotone");
    {
        std::atomic<bool> bad{false};
        ek::parallel_for(nnz, [&](int64_t lo, int64_t hi) {
            for (int64_t p = lo; p < hi; ++p)
                if (col[p] < 0 || col[p] >= n) bad = true;
        });
        if (bad) ek::fail(EK_EINVAL, "ek_kl_graph_setup: column out of range");
    }
    pt.mark("checks");
    hipStream_t s = c->kstream;
    // not ready until this setup has finished: a failure part-way must not
    // leave the previous graph's flags over this one's sizes
    c->kl.graph_ready = false;
    c->kl.part_ready = false;
    c->kl.n = n;
    c->kl.rowptr_h.assign(rowptr, rowptr + n + 1);
    Uploader up(c, s, (size_t(n) + 1) * 4 + size_t(nnz) * 8 + size_t(nnz) * 4);
    up.put(c->kl.rowptr, rowptr, size_t(n) + 1);
    // 16 zero entries of tail padding: the swap loop reads rows 16 at a time unconditionally
    c->kl.col.ensure((size_t(nnz) + 16) * 4);
    c->kl.w.ensure((size_t(nnz) + 16) * 4);
    HIPCHK(hipMemsetAsync(c->kl.col.as<int32_t>() + nnz, 0, 16 * 4, s));
    HIPCHK(hipMemsetAsync(c->kl.w.as<float>() + nnz, 0, 16 * 4, s));
    if (nnz) {
        // (the staging copies on the host threads: ~9 MB at ibm18 shape)
        unsigned char* const dc = up.buf + up.off;
        unsigned char* const dw = dc + size_t(nnz) * 4;
        ek::parallel_for(nnz, [&](int64_t lo, int64_t hi) {
            std::memcpy(dc + size_t(lo) * 4, col + lo, size_t(hi - lo) * 4);
            std::memcpy(dw + size_t(lo) * 4, w + lo, size_t(hi - lo) * 4);
        });
        HIPCHK(hipMemcpyAsync(c->kl.col.p, dc, size_t(nnz) * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->kl.w.p, dw, size_t(nnz) * 4, hipMemcpyHostToDevice, s));
        up.off += size_t(nnz) * 8;
    }
    pt.mark("CSR staged");
    // inline neighbour-row segments for the swap loop: weight-coded (128 B per
    // entry) when the distinct weights fit the code bits and the LDS table,
    // else plain (256 B per entry); skipped past 32 GB.  EK_KL_NOSEGC=1 at
    // setup: plain (A/B, tests).
    std::vector<uint32_t> kw;
    std::vector<float> wdict;
    int wcolbits = 0;
    c->kl.segc_ok = !env_set("EK_KL_NOSEGC") &&
                    size_t(nnz) * ek::dev::KL_SEGC_PIECES * sizeof(ek::dev::KLInfo) <= (size_t(32) << 30) &&
                    ek::dev::kl_weight_codes(n, nnz, col, w, kw, wdict, wcolbits);
    pt.mark("weight codes");
    c->kl.seg_ok = !c->kl.segc_ok && size_t(nnz) * ek::dev::KL_SEG_LANES * sizeof(ek::dev::KLInfo) <= (size_t(32) << 30);
    if (c->kl.segc_ok) {
        DBuf dkw;
        up.put(dkw, kw.data(), kw.size());
        upload(c->kl.wdict, wdict.data(), wdict.size(), s);
        c->kl.nwd = int(wdict.size());
        c->kl.wcolbits = wcolbits;
        c->kl.seg.reset();
        c->kl.segc.ensure(size_t(std::max<int64_t>(nnz, 1)) * ek::dev::KL_SEGC_PIECES * sizeof(ek::dev::KLInfo));
        ek::dev::kl_build_segc(s, nnz, c->kl.rowptr.as<int32_t>(), c->kl.col.as<int32_t>(), dkw.as<uint32_t>(),
                               c->kl.segc.as<ek::dev::KLInfo>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));  // dkw is freed at scope end
    }
    if (c->kl.seg_ok) {
        c->kl.segc.reset();
        c->kl.seg.ensure(size_t(std::max<int64_t>(nnz, 1)) * ek::dev::KL_SEG_LANES * sizeof(ek::dev::KLInfo));
        ek::dev::kl_build_seg(s, nnz, c->kl.rowptr.as<int32_t>(), c->kl.col.as<int32_t>(), c->kl.w.as<float>(),
                              c->kl.seg.as<ek::dev::KLInfo>());
        HIPCHK(hipGetLastError());
    }
    c->kl.side.ensure(size_t(n));
    c->kl.side_init.ensure(size_t(n));
    // (also the side / locked bitmaps of the on-chip loop when they exceed
    // its LDS budget: 2 ceil(n/32) words, k_kl_swap_loop<.., GB>)
    c->kl.locked.ensure(std::max(size_t(n), size_t((n + 31) / 32) * 8 + 64));
    c->kl.plist.ensure(size_t(n) * 4);
    c->kl.sides_tmp.ensure(size_t(n));
    c->kl.cutpart.ensure(size_t((n + 255) / 256) * 8);
    c->kl.cut0.ensure(16);
    c->kl.out.ensure(sizeof(ek::dev::KLOut));
    c->kl.count.ensure(64);
    pt.mark("segments queued");
    HIPCHK(hipStreamSynchronize(s));
    pt.mark("synchronised");
    c->kl.graph_ready = true;
    c->kl.part_ready = false;
    return EK_OK;
    EK_CATCH
}

int ek_kl_nets_setup(ek_ctx* c, int64_t nets, const int64_t* net_ptr, const int32_t* pins) {
    EK_TRY
    check_ctx(c);
    if (nets < 0 || !net_ptr || (net_ptr[nets] > 0 && !pins)) ek::fail(EK_EINVAL, "ek_kl_nets_setup: bad argument");
    c->kl.nets = nets;
    Uploader up(c, c->kstream, (size_t(nets) + 1) * 8 + size_t(net_ptr[nets]) * 4);
    up.put(c->kl.netptr, net_ptr, size_t(nets) + 1);
    up.put(c->kl.pins, pins, size_t(net_ptr[nets]));
    c->kl.count.ensure(size_t(3) * size_t(ek::dev::net_cut_blocks(nets)) * sizeof(unsigned));  // ek_kl_run's cut partials
    HIPCHK(hipStreamSynchronize(c->kstream));
    return EK_OK;
    EK_CATCH
}

}  // extern "C"

namespace {
// The rest of the partition setup once remain[] lists, plist and the initial
// sides are on the device (uploaded, or split there from the Fiedler vector)
void partition_on_device(ek_ctx* c, int64_t n0, int64_t n1) {
    hipStream_t s = c->stream;
    const int64_t n = c->kl.n;
    c->kl.n0 = n0;
    c->kl.n1 = n1;
    // row descriptors: by position {node, rowptr, rowlen} and by node {rowptr,
    // rowlen, plist}, built on the device from the lists just uploaded (the
    // by-position arrays are padded to whole chunks with zero descriptors, and
    // the gains with NaN = invalid keys, so the chunk scans load unconditionally)
    {
        c->kl.pinfo0.ensure(size_t(chunk_pad(n0)) * sizeof(ek::dev::KLInfo));
        c->kl.pinfo1.ensure(size_t(chunk_pad(n1)) * sizeof(ek::dev::KLInfo));
        c->kl.nd.ensure(size_t(std::max<int64_t>(n, 1)) * sizeof(ek::dev::KLInfo));
        ek::dev::kl_build_desc(s, int(n), int(n0), int(n1), int(chunk_pad(n0)), int(chunk_pad(n1)),
                               c->kl.order0.as<int32_t>(), c->kl.order1.as<int32_t>(), c->kl.plist.as<uint32_t>(),
                               c->kl.rowptr.as<int32_t>(), c->kl.pinfo0.as<ek::dev::KLInfo>(),
                               c->kl.pinfo1.as<ek::dev::KLInfo>(), c->kl.nd.as<ek::dev::KLInfo>());
        HIPCHK(hipGetLastError());
        const int64_t nnz = c->kl.rowptr_h[size_t(n)];
        c->kl.aux.ensure(size_t(std::max<int64_t>(nnz, 1)) * sizeof(ek::dev::KLInfo));
        ek::dev::kl_build_aux(s, nnz, c->kl.col.as<int32_t>(), c->kl.nd.as<ek::dev::KLInfo>(),
                              c->kl.aux.as<ek::dev::KLInfo>());
        HIPCHK(hipGetLastError());
        c->kl.cinfo0.ensure(size_t((n0 + ek::dev::KL_CHUNK - 1) / ek::dev::KL_CHUNK + 1) * sizeof(ek::dev::KLInfo));
        c->kl.cinfo1.ensure(size_t((n1 + ek::dev::KL_CHUNK - 1) / ek::dev::KL_CHUNK + 1) * sizeof(ek::dev::KLInfo));
    }
    c->kl.gp0.ensure(size_t(chunk_pad(n0)) * 4);
    c->kl.gp1.ensure(size_t(chunk_pad(n1)) * 4);
    HIPCHK(hipMemsetAsync(c->kl.gp0.p, 0xFF, c->kl.gp0.bytes, s));  // NaN padding
    HIPCHK(hipMemsetAsync(c->kl.gp1.p, 0xFF, c->kl.gp1.bytes, s));
    c->kl.ckey0.ensure(size_t((n0 + ek::dev::KL_CHUNK - 1) / ek::dev::KL_CHUNK + 1) * 8);
    c->kl.ckey1.ensure(size_t((n1 + ek::dev::KL_CHUNK - 1) / ek::dev::KL_CHUNK + 1) * 8);
    c->kl.log.ensure(size_t(std::max<int64_t>(1, std::min(n0, n1))) * sizeof(ek_swap));
    HIPCHK(hipStreamSynchronize(s));
    c->kl.part_ready = true;
}

}  // namespace

extern "C" {

int ek_kl_set_partition(ek_ctx* c, const int32_t* order0, int64_t n0, const int32_t* order1, int64_t n1) {
    EK_TRY
    check_ctx(c);
    if (!c->kl.graph_ready) ek::fail(EK_ESTATE, "ek_kl_set_partition before ek_kl_graph_setup");
    const int64_t n = c->kl.n;
    if (n0 < 0 || n1 < 0 || n0 + n1 != n || (n0 && !order0) || (n1 && !order1))
        ek::fail(EK_EINVAL, "ek_kl_set_partition: the two lists must cover all %lld nodes", (long long)n);
    std::vector<uint8_t> side(size_t(n), 2);
    std::vector<uint32_t> plist(size_t(n), 0);
    for (int64_t i = 0; i < n0; ++i) {
        const int32_t u = order0[i];
        if (u < 0 || u >= n || side[size_t(u)] != 2) ek::fail(EK_EINVAL, "ek_kl_set_partition: bad/duplicate node %d", u);
        side[size_t(u)] = 0;
        plist[size_t(u)] = uint32_t(i);
    }
    for (int64_t i = 0; i < n1; ++i) {
        const int32_t u = order1[i];
        if (u < 0 || u >= n || side[size_t(u)] != 2) ek::fail(EK_EINVAL, "ek_kl_set_partition: bad/duplicate node %d", u);
        side[size_t(u)] = 1;
        plist[size_t(u)] = uint32_t(i) | 0x80000000u;
    }
    hipStream_t s = c->stream;
    c->kl.part_ready = false;  // the lists are rewritten from here on
    Uploader up(c, s, size_t(n0) * 4 + size_t(n1) * 4 + size_t(n) + size_t(n) * 4);
    up.put(c->kl.order0, order0, size_t(n0));
    up.put(c->kl.order1, order1, size_t(n1));
    up.put(c->kl.side_init, side.data(), size_t(n));
    up.put(c->kl.plist, plist.data(), size_t(n));
    partition_on_device(c, n0, n1);
    return EK_OK;
    EK_CATCH
}

int ek_fiedler_set(ek_ctx* c, int64_t n, const double* v_host) {
    EK_TRY
    check_ctx(c);
    if (c->nranks > 1) ek::fail(EK_ESTATE, "ek_fiedler_set: a multi-rank context (%d ranks); the splits run on one", c->nranks);
    if (n < 1 || n > INT32_MAX - 1 || !v_host) ek::fail(EK_EINVAL, "ek_fiedler_set: bad argument");
    {
        // a NaN has no place in the select's order, and a solve never leaves one
        std::atomic<bool> bad{false};
        ek::parallel_for(n, [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; ++i)
                if (v_host[i] != v_host[i]) bad = true;
        });
        if (bad) ek::fail(EK_EINVAL, "ek_fiedler_set: NaN in the vector");
    }
    hipStream_t s = c->stream;
    c->fied_n = 0;  // as a solve does: no vector until this one is whole on the device
    upload(c->fied, v_host, size_t(n), s);
    HIPCHK(hipStreamSynchronize(s));
    c->fied_n = n;
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_fiedler(ek_ctx* c, double* median_out, int64_t* n0_out, int64_t* n1_out) {
    EK_TRY
    check_ctx(c);
    if (!c->kl.graph_ready) ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler before ek_kl_graph_setup");
    const int64_t n = c->kl.n;
    if (c->fied_n != n || n < 1)
        ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler: no Fiedler vector of %lld entries on this context",
                 (long long)n);
    if (n > INT32_MAX - 1) ek::fail(EK_EINVAL, "ek_kl_set_partition_fiedler: %lld nodes", (long long)n);
    hipStream_t s = c->stream;
    const int ni = int(n);
    const double* v = c->fied.as<double>();
    const size_t tb = ek::dev::split_tmp_bytes(ni);
    c->sp_tmp.ensure(tb);
    c->sp_out.ensure(64);
    // the median: ranks n/2 (and n/2 - 1 for even n, their mean), the values
    // nth_element gives ek_median_split (a radix select on the device)
    const unsigned hi = unsigned(n / 2), lo = n % 2 == 0 ? hi - 1 : hi;
    auto* keys = c->sp_out.as<unsigned long long>();
    ek::dev::split_select(s, c->sp_tmp.p, v, ni, lo, hi, keys);
    unsigned long long kk[2] = {0ull, 0ull};
    HIPCHK(hipMemcpyAsync(kk, keys, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double mid[2] = {ek::dev::key_value(kk[0]), ek::dev::key_value(kk[1])};
    const double med = n % 2 == 0 ? (mid[0] + mid[1]) / 2.0 : mid[0];
    c->kl.part_ready = false;  // the lists are rewritten from here on: a failure must not leave the old partition's flag
    c->kl.order0.ensure(size_t(n) * 4);
    c->kl.order1.ensure(size_t(n) * 4);
    c->kl.side_init.ensure(size_t(n));
    c->kl.plist.ensure(size_t(n) * 4);
    unsigned* n0_dev = reinterpret_cast<unsigned*>(c->sp_out.as<unsigned long long>() + 2);
    ek::dev::split_partition(s, c->sp_tmp.p, v, ni, med, c->kl.order0.as<int32_t>(), c->kl.order1.as<int32_t>(),
                             c->kl.plist.as<uint32_t>(), c->kl.side_init.as<uint8_t>(), n0_dev);
    HIPCHK(hipGetLastError());
    unsigned n0u = 0;
    HIPCHK(hipMemcpyAsync(&n0u, n0_dev, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t n0 = int64_t(n0u);
    partition_on_device(c, n0, n - n0);
    if (median_out) *median_out = med;
    if (n0_out) *n0_out = n0;
    if (n1_out) *n1_out = n - n0;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"

namespace {
// The rank split of v (device, n doubles) into the given lists: the key at
// rank n1 - 1 by the median split's radix select, then kernels_kway.hip's
// count and place.  Returns the side-0 count (one synchronisation).
int64_t rank_split_on_device(ek_ctx* c, const double* v, int64_t n, int64_t n1, int32_t* order0, int32_t* order1,
                             uint32_t* plist, uint8_t* side) {
    hipStream_t s = c->stream;
    const int ni = int(n);
    c->sp_tmp.ensure(ek::dev::split_tmp_bytes(ni));
    c->sp_out.ensure(64);
    c->rk_tmp.ensure(ek::dev::rank_tmp_bytes(ni));
    auto* keys = c->sp_out.as<unsigned long long>();
    if (n1 > 0) ek::dev::split_select(s, c->sp_tmp.p, v, ni, unsigned(n1 - 1), unsigned(n1 - 1), keys);
    else HIPCHK(hipMemsetAsync(keys, 0, 16, s));  // key 0: nothing lies below it, none of its equals is needed
    unsigned* n0_dev = reinterpret_cast<unsigned*>(keys + 2);
    ek::dev::rank_partition(s, c->rk_tmp.p, v, ni, keys, unsigned(n1), order0, order1, plist, side, n0_dev);
    HIPCHK(hipGetLastError());
    unsigned n0u = 0;
    HIPCHK(hipMemcpyAsync(&n0u, n0_dev, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (int64_t(n0u) != n - n1)
        ek::fail(EK_EHIP, "rank split: side 0 got %u nodes, expected %lld", n0u, (long long)(n - n1));
    return int64_t(n0u);
}
}  // namespace

extern "C" {

int ek_rank_split_device(ek_ctx* c, int64_t n, const double* v_host, int64_t n1, uint8_t* bits_out) {
    EK_TRY
    check_ctx(c);
    if (n <= 0 || n > INT32_MAX - 1 || !v_host || !bits_out || n1 < 0 || n1 > n)
        ek::fail(EK_EINVAL, "ek_rank_split_device: bad argument");
    hipStream_t s = c->stream;
    DBuf v, o0, o1, pl, sd;
    upload(v, v_host, size_t(n), s);
    o0.ensure(size_t(n) * 4);
    o1.ensure(size_t(n) * 4);
    pl.ensure(size_t(n) * 4);
    sd.ensure(size_t(n));
    rank_split_on_device(c, v.as<double>(), n, n1, o0.as<int32_t>(), o1.as<int32_t>(), pl.as<uint32_t>(),
                         sd.as<uint8_t>());
    HIPCHK(hipMemcpyAsync(bits_out, sd.p, size_t(n), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_fiedler_rank(ek_ctx* c, int64_t n1, int64_t* n0_out, int64_t* n1_out) {
    EK_TRY
    check_ctx(c);
    if (!c->kl.graph_ready) ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_rank before ek_kl_graph_setup");
    const int64_t n = c->kl.n;
    if (c->fied_n != n || n < 2)
        ek::fail(EK_ESTATE, "ek_kl_set_partition_fiedler_rank: no Fiedler vector of %lld entries on this context",
                 (long long)n);
    if (n > INT32_MAX - 1) ek::fail(EK_EINVAL, "ek_kl_set_partition_fiedler_rank: %lld nodes", (long long)n);
    if (n1 < 1 || n1 >= n)
        ek::fail(EK_EINVAL, "ek_kl_set_partition_fiedler_rank: n1 = %lld outside [1, %lld)", (long long)n1, (long long)n);
    c->kl.part_ready = false;  // as in ek_kl_set_partition_fiedler
    c->kl.order0.ensure(size_t(n) * 4);
    c->kl.order1.ensure(size_t(n) * 4);
    c->kl.side_init.ensure(size_t(n));
    c->kl.plist.ensure(size_t(n) * 4);
    const int64_t n0 = rank_split_on_device(c, c->fied.as<double>(), n, n1, c->kl.order0.as<int32_t>(),
                                            c->kl.order1.as<int32_t>(), c->kl.plist.as<uint32_t>(),
                                            c->kl.side_init.as<uint8_t>());
    partition_on_device(c, n0, n - n0);
    if (n0_out) *n0_out = n0;
    if (n1_out) *n1_out = n - n0;
    return EK_OK;
    EK_CATCH
}

int ek_kl_set_partition_bits(ek_ctx* c, int64_t n, const uint8_t* bits) {
    EK_TRY
    if (n < 0 || (n && !bits)) ek::fail(EK_EINVAL, "ek_kl_set_partition_bits: bad argument");
    std::vector<int32_t> o[2];
    o[0].reserve(size_t(n) / 2 + 1);
    o[1].reserve(size_t(n) / 2 + 1);
    for (int64_t i = 0; i < n; ++i) {
        if (bits[i] > 1) ek::fail(EK_EINVAL, "ek_kl_set_partition_bits: bit %d at node %lld", int(bits[i]), (long long)i);
        o[bits[i]].push_back(int32_t(i));
    }
    return ek_kl_set_partition(c, o[0].data(), int64_t(o[0].size()), o[1].data(), int64_t(o[1].size()));
    EK_CATCH
}

int ek_kl_partition_copy(ek_ctx* c, int32_t* order0_out, int32_t* order1_out, uint32_t* plist_out, uint8_t* side_out,
                         int64_t* n0_out, int64_t* n1_out) {
    EK_TRY
    check_ctx(c);
    if (!c->kl.graph_ready || !c->kl.part_ready) ek::fail(EK_ESTATE, "ek_kl_partition_copy: no partition is set");
    hipStream_t s = c->stream;
    const size_t n = size_t(c->kl.n), n0 = size_t(c->kl.n0), n1 = size_t(c->kl.n1);
    if (order0_out && n0) HIPCHK(hipMemcpyAsync(order0_out, c->kl.order0.p, n0 * 4, hipMemcpyDeviceToHost, s));
    if (order1_out && n1) HIPCHK(hipMemcpyAsync(order1_out, c->kl.order1.p, n1 * 4, hipMemcpyDeviceToHost, s));
    if (plist_out) HIPCHK(hipMemcpyAsync(plist_out, c->kl.plist.p, n * 4, hipMemcpyDeviceToHost, s));
    if (side_out) HIPCHK(hipMemcpyAsync(side_out, c->kl.side_init.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n0_out) *n0_out = c->kl.n0;
    if (n1_out) *n1_out = c->kl.n1;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"

namespace {

ek::dev::KLDev kl_dev(ek_ctx* c) {
    ek::dev::KLDev d;
    d.n = int(c->kl.n);
    d.nnz = c->kl.rowptr_h.empty() ? 0 : c->kl.rowptr_h.back();
    d.rowptr = c->kl.rowptr.as<int32_t>();
    d.col = c->kl.col.as<int32_t>();
    d.w = c->kl.w.as<float>();
    d.side = c->kl.side.as<uint8_t>();
    d.side_init = c->kl.side_init.as<uint8_t>();
    d.locked = c->kl.locked.as<uint8_t>();
    d.gp0 = c->kl.gp0.as<float>();
    d.gp1 = c->kl.gp1.as<float>();
    d.order0 = c->kl.order0.as<int32_t>();
    d.order1 = c->kl.order1.as<int32_t>();
    d.plist = c->kl.plist.as<uint32_t>();
    d.pinfo0 = c->kl.pinfo0.as<ek::dev::KLInfo>();
    d.pinfo1 = c->kl.pinfo1.as<ek::dev::KLInfo>();
    d.nd = c->kl.nd.as<ek::dev::KLInfo>();
    d.cinfo0 = c->kl.cinfo0.as<ek::dev::KLInfo>();
    d.cinfo1 = c->kl.cinfo1.as<ek::dev::KLInfo>();
    d.aux = c->kl.aux.as<ek::dev::KLInfo>();
    const bool noseg = env_set("EK_KL_NOSEG");  // env: A/B, no inline segments at all
    d.seg = c->kl.seg_ok && !noseg ? c->kl.seg.as<ek::dev::KLInfo>() : nullptr;
    d.segc = c->kl.segc_ok && !noseg ? c->kl.segc.as<ek::dev::KLInfo>() : nullptr;
    d.wdict = c->kl.wdict.as<float>();
    d.nwd = c->kl.nwd;
    d.wcolbits = c->kl.wcolbits;
    d.n0 = int(c->kl.n0);
    d.n1 = int(c->kl.n1);
    d.nck0 = int((c->kl.n0 + ek::dev::KL_CHUNK - 1) / ek::dev::KL_CHUNK);
    d.nck1 = int((c->kl.n1 + ek::dev::KL_CHUNK - 1) / ek::dev::KL_CHUNK);
    d.ckey0 = c->kl.ckey0.as<unsigned long long>();
    d.ckey1 = c->kl.ckey1.as<unsigned long long>();
    d.cut_part = c->kl.cutpart.as<double>();
    d.cut0 = c->kl.cut0.as<float>();
    return d;
}

}  // namespace

extern "C" int ek_kl_run(ek_ctx* c, int32_t limit, ek_swap* log_out, int64_t cap, ek_kl_result* res) {
    EK_TRY
    check_ctx(c);
    if (!c->kl.graph_ready || !c->kl.part_ready) ek::fail(EK_ESTATE, "ek_kl_run before graph/partition setup");
    hipStream_t s = c->stream;
    const int64_t n = c->kl.n;
    const int lim = limit >= 0 ? limit : int(std::log2(double(n))) + 5;  // cKL.cpp:303
    const auto d = kl_dev(c);
    hipEvent_t e0, e1, e2;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventCreate(&e2));
    struct G {
        hipEvent_t a, b, c;
        ~G() {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
            (void)hipEventDestroy(c);
        }
    } guard{e0, e1, e2};
    const long long dcap = std::max<int64_t>(1, std::min(c->kl.n0, c->kl.n1));
    auto* out = c->kl.out.as<ek::dev::KLOut>();
    HIPCHK(hipEventRecord(e0, s));
    HIPCHK(hipMemcpyAsync(c->kl.side.p, c->kl.side_init.p, size_t(n), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync(c->kl.locked.p, 0, size_t(n), s));
    ek::dev::kl_prepare(s, d);
    HIPCHK(hipEventRecord(e1, s));
    ek::dev::kl_loop(s, d, lim, c->kl.log.as<ek_swap>(), dcap, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e2, s));
    // integer net cuts: initial, best prefix, final
    const bool nets = c->kl.nets > 0;
    const int ncb = nets ? ek::dev::net_cut_blocks(c->kl.nets) : 0;
    std::vector<unsigned> cparts(size_t(3) * size_t(ncb));
    if (nets) {  // one pass over the pins for all three; per-workgroup counts, added here
        ek::dev::kl_replay(s, int(n), c->kl.side_init.as<uint8_t>(), c->kl.log.as<ek_swap>(), &out->best_iter, dcap,
                           c->kl.sides_tmp.as<uint8_t>());
        ek::dev::net_cut(s, c->kl.nets, c->kl.netptr.as<int64_t>(), c->kl.pins.as<int32_t>(),
                         c->kl.side_init.as<uint8_t>(), c->kl.sides_tmp.as<uint8_t>(), c->kl.side.as<uint8_t>(),
                         c->kl.count.as<unsigned>());
    }
    ek::dev::KLOut ho{};
    HIPCHK(hipMemcpyAsync(&ho, out, sizeof ho, hipMemcpyDeviceToHost, s));
    if (nets)
        HIPCHK(hipMemcpyAsync(cparts.data(), c->kl.count.p, cparts.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ho.status == 3u)
        ek::fail(EK_EHIP, "KL swap loop: an in-launch wait gave up (EK_KL_PIPE=0 runs the loop without them)");
    unsigned long long hc[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k)
        for (int b = 0; b < ncb; ++b) hc[k] += cparts[size_t(k) * size_t(ncb) + size_t(b)];
    if (log_out && cap > 0) {
        const int64_t k = std::min<int64_t>(cap, ho.iterations);
        if (k) HIPCHK(hipMemcpy(log_out, c->kl.log.p, size_t(k) * sizeof(ek_swap), hipMemcpyDeviceToHost));
    }
    if (res) {
        float loop_ms = 0.f, prep_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&prep_ms, e0, e1));
        HIPCHK(hipEventElapsedTime(&loop_ms, e1, e2));
        res->iterations = ho.iterations;
        res->initial_cut = ho.initial_cut;
        res->best_cut = ho.best_cut;
        res->final_cut = ho.final_cut;
        res->best_iter = ho.best_iter;
        res->net_cut_initial = nets ? int64_t(hc[0]) : -1;
        res->net_cut_best = nets ? int64_t(hc[1]) : -1;
        res->net_cut_final = nets ? int64_t(hc[2]) : -1;
        res->loop_ms = loop_ms;
        if (env_set("EK_KL_PROF") && ho.prof[13] == 0x9199ull) {  // the overlapped loop (k_kl_swap_pipe)
            const double sw = double(std::max<long long>(1, ho.iterations)), gs = double(std::max<unsigned long long>(1, ho.prof[2]));
            std::fprintf(stderr, "[kl-pipe] %lld swaps: speculated %.1f %%, hits %.1f %%; loop %.0f cycles/swap\n",
                         (long long)ho.iterations, 100.0 * double(ho.prof[0]) / sw, 100.0 * double(ho.prof[1]) / gs,
                         double(ho.prof[12]) / sw);
            std::fprintf(stderr, "[kl-pipe] gain wave 0, cycles/swap: pair wait %.0f, P %.0f, speculative rows %.0f (per "
                         "speculation), pair->barrier1 %.0f\n", double(ho.prof[3]) / gs, double(ho.prof[4]) / gs,
                         double(ho.prof[5]) / double(std::max<unsigned long long>(1, ho.prof[0])), double(ho.prof[6]) / gs);
            std::fprintf(stderr, "[kl-pipe] W wave, cycles/swap: barrier-2 wait %.0f, selection %.0f, pair->barrier1 %.0f, "
                         "G2 span %.0f; G2a wave's G2 span %.0f\n", double(ho.prof[7]) / sw, double(ho.prof[8]) / sw,
                         double(ho.prof[9]) / sw, double(ho.prof[10]) / sw, double(ho.prof[11]) / sw);
        } else if (env_set("EK_KL_PROF")) {
            static const char* names[12] = {"select", "G1-key", "bar1", "G2a", "G2bc", "bar2", "G1-aux", "G1-sum",
                                            "n_stale", "n_late+tail", "G1-load", "G1-look"};
            std::fprintf(stderr, "[kl] %lld swaps, us/swap:", (long long)ho.iterations);
            for (int i = 0; i < 12; ++i)
                std::fprintf(stderr, " %s %.3f", names[i], ho.prof[i] * 0.01 / std::max<long long>(1, ho.iterations));
            std::fprintf(stderr, "\n");
            if (ho.prof[15])
                std::fprintf(stderr, "[kl] in-loop shader clock %.0f MHz\n", double(ho.prof[14]) / (double(ho.prof[15]) * 0.01));
            if (ho.warr[0] || ho.warr[8]) {
                const double cyc_ns = ho.prof[15] ? double(ho.prof[15]) * 10.0 / double(ho.prof[14]) : 1.0 / 2.4;
                const double f = 1e-3 * cyc_ns / double(std::max<long long>(1, ho.iterations));
                std::fprintf(stderr, "[kl] per wave, us after its loop top: selection done / barrier 1 / G2a done / barrier 2:\n");
                std::fprintf(stderr, "[kl] prefetch predicted node1 in %.1f %%, node2 in %.1f %% of swaps\n",
                             100.0 * double(ho.warr[40]) / double(std::max<long long>(1, ho.iterations)),
                             100.0 * double(ho.warr[41]) / double(std::max<long long>(1, ho.iterations)));
                for (int w = 0; w < 8; ++w)
                    std::fprintf(stderr, "[kl]   w%d %.3f %.3f %.3f %.3f  (G2a reads consumed %.3f)\n", w,
                                 f * double(ho.warr[24 + w]), f * double(ho.warr[w]), f * double(ho.warr[16 + w]),
                                 f * double(ho.warr[8 + w]), f * double(ho.warr[32 + w]));
            }
        }
        res->total_ms = double(loop_ms) + double(prep_ms);
    }
    return EK_OK;
    EK_CATCH
}

extern "C" int ek_kl_sides(ek_ctx* c, int32_t which, uint8_t* sides_out) {
    EK_TRY
    check_ctx(c);
    if (!c->kl.part_ready || !sides_out) ek::fail(EK_ESTATE, "ek_kl_sides: nothing to report");
    hipStream_t s = c->stream;
    const int64_t n = c->kl.n;
    const uint8_t* src = c->kl.side_init.as<uint8_t>();
    if (which == 2) src = c->kl.side.as<uint8_t>();
    if (which == 1) {
        const long long dcap = std::max<int64_t>(1, std::min(c->kl.n0, c->kl.n1));
        ek::dev::kl_replay(s, int(n), c->kl.side_init.as<uint8_t>(), c->kl.log.as<ek_swap>(),
                           &c->kl.out.as<ek::dev::KLOut>()->best_iter, dcap, c->kl.sides_tmp.as<uint8_t>());
        src = c->kl.sides_tmp.as<uint8_t>();
    }
    HIPCHK(hipMemcpyAsync(sides_out, src, size_t(n), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return EK_OK;
    EK_CATCH
}
