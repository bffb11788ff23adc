// SpMV set-up of libeigkl_hip.so (host rows, or the Laplacian built on the
// device from the pins; coded CSR, column panels, the sharded owned-slot
// rows) and the ek_spmv* entries, benches and queries.
#include "ctx.hpp"

using namespace ek::rt;

namespace ek::rt {

ek::dev::SpmvMat spmv_mat(const ek_ctx* c) {
    ek::dev::SpmvMat m;
    m.nblocks = c->nrb_spmv;
    if (c->pn_G > 0) {
        m.panel.G = c->pn_G;
        m.panel.P = c->pn_P;
        m.panel.pb = c->pn_pb;
        m.panel.max_rows = c->pn_max_rows;
        m.panel.ndict = c->pn_ndict;
        m.panel.wrow = c->pn_wrow.as<int32_t>();
        m.panel.start = c->pn_start.as<long long>();
        m.panel.word = c->pn_word.as<uint32_t>();
        m.panel.rid = c->pn_rid.as<uint16_t>();
        m.dict = c->dict.as<double>();
        return m;
    }
    m.block_nnz = c->block_nnz;
    m.has_long = c->spmv_long;
    m.desc = c->rb.as<int32_t>();
    m.rowptr = c->rowptr.as<int32_t>();
    if (c->colbits > 0) {
        m.colbits = c->colbits;
        m.pk = c->pk.as<uint32_t>();
        m.rel = c->rel.as<uint16_t>();
        m.dict = c->dict.as<double>();
    } else {
        m.col = c->col.as<int32_t>();
        m.val = c->val.as<double>();
    }
    return m;
}

// the owned-slot rows (c->own_*): plain CSR over local columns, x = the rank's f
ek::dev::SpmvMat own_mat(const ek_ctx* c) {
    ek::dev::SpmvMat m;
    m.nblocks = c->own_nrb;
    m.block_nnz = 512;
    m.desc = c->own_rb.as<int32_t>();
    m.rowptr = c->own_rowptr.as<int32_t>();
    m.col = c->own_col.as<int32_t>();
    m.val = c->own_val.as<double>();
    return m;
}

}  // namespace ek::rt

namespace {

// The column-panel form when x outgrows an XCD's L2 (EK_SPMV_PANEL=0/1 forces
// it off/on; default: x > 8 MB, the 10x synthetic.  At 2x (3.2 MB) the two
// forms took the same time inside the solve, 29 vs 30 us, and the 1x x
// stays in every L2: tools/panel_lab.py)
bool want_panels(const ek_ctx* c) {
    return env_flag("EK_SPMV_PANEL", x_extent(c) * 8 > (int64_t(8) << 20));
}

// Build the panel layout from this rank's coded CSR on the device (rowptr_d,
// pk_d: (code << colbits) | col words); rowptr_h is the host copy.  False
// when the codes do not fit beside the panel column bits.
bool build_panels(ek_ctx* c, hipStream_t s, const int32_t* rowptr_h, const int32_t* rowptr_d, const uint32_t* pk_d,
                  int colbits, int64_t ncodes) {
    const int64_t X = x_extent(c);
    int pb = 17;  // 1 MB of x per panel (EK_PANEL_PB: lab override)
    if (const int e = env_int("EK_PANEL_PB", 0); e >= 10 && e <= 24) pb = e;
    while (((X + (int64_t(1) << pb) - 1) >> pb) > ek::dev::MAX_PANELS) ++pb;
    if (pb >= 32 || ncodes > (int64_t(1) << (32 - pb))) return false;
    const int P = int((X + (int64_t(1) << pb) - 1) >> pb);
    const int64_t nnz = rowptr_h[c->nrows];
    // The most workgroups (<= 8 per CU) that are all resident at once, so they
    // walk the panels together (a straggling second round of workgroups
    // measured 90 -> 124 us at 10x): each holds its rows' accumulators in LDS.
    std::vector<int32_t> wr;
    int G = 0, max_rows = 1;
    for (int per_cu = 8; per_cu >= 1; --per_cu) {
        wr = ek::dev::panel_row_ranges(rowptr_h, c->nrows, per_cu * c->num_cu);
        G = int(wr.size()) - 1;
        max_rows = 1;
        for (int w = 0; w < G; ++w) max_rows = std::max(max_rows, wr[size_t(w) + 1] - wr[size_t(w)]);
        const int fit = int(std::min<size_t>(8, (160 * 1024) / (ek::dev::panel_lds_bytes(max_rows, int(ncodes)) + 1024)));
        if (G <= fit * c->num_cu) break;
    }
    upload(c->pn_wrow, wr.data(), wr.size(), s);
    DBuf cnt, tiles;
    cnt.ensure(size_t(G) * P * 4 + 4);
    tiles.ensure((size_t(G) * P / 1024 + 4) * 8);
    c->pn_start.ensure((size_t(G) * P + 1) * 8);
    c->pn_word.ensure(size_t(std::max<int64_t>(nnz, 1)) * 4);
    c->pn_rid.ensure(size_t(std::max<int64_t>(nnz, 1)) * 2);
    ek::dev::panel_count(s, G, rowptr_d, pk_d, colbits, c->pn_wrow.as<int32_t>(), pb, P, cnt.as<int>());
    ek::dev::exclusive_scan(s, cnt.as<int>(), (long long)G * P, c->pn_start.as<long long>(), tiles.as<long long>());
    ek::dev::panel_fill(s, G, rowptr_d, pk_d, colbits, c->pn_wrow.as<int32_t>(), pb, P, c->pn_start.as<long long>(),
                        c->pn_word.as<uint32_t>(), c->pn_rid.as<uint16_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));  // the temporaries and the host row ranges go out of scope
    c->pn_G = G;
    c->pn_P = P;
    c->pn_pb = pb;
    c->pn_max_rows = max_rows;
    c->pn_ndict = int(ncodes);
    c->nrb_spmv = G;  // the alpha partials: one per workgroup
    c->mat_bytes = nnz * 6 + int64_t(G) * P * 8 + int64_t(wr.size()) * 4 + ncodes * 8;
    return true;
}

// Global column -> the all-gather layout (host copy of k_remap_cols)
void remap_cols_host(const ek_ctx* c, const int32_t* col, int64_t nnz, std::vector<int32_t>& out) {
    out.resize(size_t(nnz));
    const auto& off = c->shard_off;
    ek::parallel_for(nnz, [&](int64_t lo, int64_t hi) {
        for (int64_t p = lo; p < hi; ++p) {
            const int64_t g = col[p];
            const int r = int(std::upper_bound(off.begin() + 1, off.end() - 1, g) - (off.begin() + 1));
            out[size_t(p)] = int32_t(r * c->slot + (g - off[size_t(r)]));
        }
    });
}

// The owned-slot rows of a sharded context (factorize_mr overlaps their SpMV
// with the all-gather): row blocks over the local CSR own_rowptr_h, the
// stream and events of the overlapped step.
void own_finish(ek_ctx* c, const std::vector<int32_t>& orp) {
    auto rbv = ek::dev::spmv_row_blocks(orp.data(), c->nrows, 512);
    c->own_nrb = int(rbv.size() / 4);
    upload(c->own_rb, rbv.data(), rbv.size(), c->stream);
    c->yown.ensure(size_t(std::max<int64_t>(c->nrows, 1)) * 8);
    if (!c->gstream) HIPCHK(hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking));
    for (auto& e : c->ag_ev)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->own_ready = true;
}

// ... from the host rows (columns already in the slot layout)
void own_build_host(ek_ctx* c, const int32_t* rowptr, const int32_t* col, const double* val) {
    c->own_ready = false;
    const int64_t lo = c->rank * c->slot, hi = lo + c->nrows;
    std::vector<int32_t> orp(size_t(c->nrows) + 1, 0), oc;
    std::vector<double> ov;
    for (int64_t r = 0; r < c->nrows; ++r) {
        for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p)
            if (col[p] >= lo && col[p] < hi) {
                oc.push_back(int32_t(col[p] - lo));
                ov.push_back(val[p]);
            }
        orp[size_t(r) + 1] = int32_t(oc.size());
    }
    c->own_nnz = int64_t(oc.size());
    upload(c->own_rowptr, orp.data(), orp.size(), c->stream);
    // (a rank of no rows has no owned entry, and an empty vector no data to copy one from)
    upload(c->own_col, oc.data(), oc.size(), c->stream);
    upload(c->own_val, ov.data(), ov.size(), c->stream);
    own_finish(c, orp);
}

// ... from the device rows (ek_spmv_setup_pins: c->rowptr / col / val, columns remapped)
void own_build_dev(ek_ctx* c, hipStream_t s, long long* tiles) {
    c->own_ready = false;
    const int lo = int(c->rank * c->slot), hi = int(lo + c->nrows);
    const size_t nr = size_t(c->nrows);
    DBuf cnt, offs;
    cnt.ensure((nr + 1) * 4);
    offs.ensure((nr + 1) * 8);
    const long long tot = ek::dev::own_split(s, (long long)nr, c->rowptr.as<int>(), c->col.as<int>(),
                                             c->val.as<double>(), lo, hi, cnt.as<int>(), offs.as<long long>(), tiles,
                                             nullptr, nullptr, nullptr);
    c->own_nnz = tot;
    c->own_rowptr.ensure((nr + 1) * 4);
    c->own_col.ensure(size_t(std::max<long long>(tot, 1)) * 4);
    c->own_val.ensure(size_t(std::max<long long>(tot, 1)) * 8);
    if (nr == 0) HIPCHK(hipMemsetAsync(c->own_rowptr.p, 0, 4, s));  // (own_split launches nothing: own_build_host's {0})
    ek::dev::own_split(s, (long long)nr, c->rowptr.as<int>(), c->col.as<int>(), c->val.as<double>(), lo, hi,
                       cnt.as<int>(), offs.as<long long>(), tiles, c->own_rowptr.as<int>(), c->own_col.as<int>(),
                       c->own_val.as<double>());
    std::vector<int32_t> orp(nr + 1);
    HIPCHK(hipMemcpyAsync(orp.data(), c->own_rowptr.p, (nr + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    own_finish(c, orp);
}

// ek_spmv_setup's body, the shard map given; also the device build's host
// fallback, which one rank may take alone.  Sharded, it makes halo_build's
// collectives: a rank that takes the fallback returns before the device
// path's own halo_build, so every rank still makes exactly one call (checked
// there).  A rank that fails before that call leaves its peers in the
// setup's all-gather, as any collective setup does.
void spmv_setup_rows(ek_ctx* c, int64_t n, const std::vector<int64_t>& off, const int32_t* rowptr, const int32_t* col,
                     const double* val) {
    set_shard(c, n, off);
    const int64_t nrows = c->nrows;
    if (rowptr[0] != 0) ek::fail(EK_EINVAL, "ek_spmv_setup: rowptr[0] must be 0 (local rows)");
    ek::PhaseTimer pt("spmv_setup");
    const int64_t nnz = rowptr[nrows];
    for (int64_t r = 0; r < nrows; ++r)
        if (rowptr[r + 1] < rowptr[r]) ek::fail(EK_EINVAL, "ek_spmv_setup: rowptr not monotone");
    for (int64_t p = 0; p < nnz; ++p)
        if (col[p] < 0 || col[p] >= n) ek::fail(EK_EINVAL, "ek_spmv_setup: column %d out of range", col[p]);
    std::vector<int32_t> colx;  // sharded: the columns in the all-gather layout
    c->own_ready = false;
    if (c->mr) {
        remap_cols_host(c, col, nnz, colx);
        col = colx.data();
        own_build_host(c, rowptr, col, val);
        halo_build(c, colx.data(), nnz);  // (the owned rows were taken in the slot layout)
    }
    c->n = n;
    c->nnz = nnz;
    // dictionary-coded entries unless EK_SPMV_PLAIN is set or the values do not fit
    std::vector<uint32_t> pkv;
    std::vector<double> dictv;
    int colbits = 0;
    const bool plain = env_flag("EK_SPMV_PLAIN", false);
    pt.mark("validate");
    const bool packed = !plain &&
                        ek::dev::spmv_pack(x_extent(c), nnz, col, val, pkv, dictv, colbits);
    pt.mark("pack");
    // 512-nnz blocks (tools/spmv_lab.hip for plain CSR; for the coded form,
    // 1024-nnz segments measured 14.3 against 12.7 us inside the solve)
    c->pn_G = 0;
    if (packed && nrows > 0 && want_panels(c)) {  // (no rows: no panel workgroups; the one empty row block)
        DBuf rp_d, pk_d;
        upload(c->dict, dictv.data(), dictv.size(), c->stream);
        upload(rp_d, rowptr, size_t(nrows) + 1, c->stream);
        upload(pk_d, pkv.data(), pkv.size(), c->stream);
        if (build_panels(c, c->stream, rowptr, rp_d.as<int32_t>(), pk_d.as<uint32_t>(), colbits, int64_t(dictv.size()))) {
            c->colbits = colbits;
            c->pk.reset();
            c->rel.reset();
            c->col.reset();
            c->val.reset();
            c->rowptr.reset();
            c->rb.reset();
            pt.mark("panels");
            return;
        }
    }
    c->block_nnz = ek::dev::SPMV_SEG_NNZ;  // (coded or plain: the same row blocks, so the same sums)
    auto rbv = ek::dev::spmv_row_blocks(rowptr, nrows, c->block_nnz);
    c->nrb_spmv = int(rbv.size() / 4);
    c->spmv_long = false;
    for (size_t bk = 0; bk < rbv.size() / 4; ++bk) c->spmv_long = c->spmv_long || rbv[4 * bk + 3] > c->block_nnz;
    c->colbits = packed ? colbits : 0;
    if (packed) {
        std::vector<uint32_t> segv;
        std::vector<uint16_t> relv;
        pt.mark("row blocks");
        ek::dev::spmv_segment(rbv, rowptr, pkv, c->block_nnz, segv, relv);  // long rows: desc nnz0 -> overflow area
        pt.mark("segments");
        upload(c->pk, segv.data(), segv.size(), c->stream);
        upload(c->rel, relv.data(), relv.size(), c->stream);
        upload(c->dict, dictv.data(), dictv.size(), c->stream);
        c->mat_bytes = int64_t(segv.size() * 4 + relv.size() * 2 + dictv.size() * 8 + rbv.size() * 4);
        c->col.reset();
        c->val.reset();
        c->rowptr.reset();
    } else {
        upload(c->rowptr, rowptr, size_t(nrows) + 1, c->stream);
        upload(c->col, col, size_t(nnz), c->stream);
        upload(c->val, val, size_t(nnz), c->stream);
        c->mat_bytes = 12 * nnz + 4 * (nrows + 1);
        c->pk.reset();
        c->rel.reset();
        c->dict.reset();
    }
    upload(c->rb, rbv.data(), rbv.size(), c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    pt.mark("upload");
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// SpMV seam (SparseSymMatProd::perform_op, cEIG.cpp:194)
// Sharded: the ranks' row ranges are learned with one all-gather of
// (row0, nrows) over the comm seam and must tile [0, n) in rank order (equal
// blocks from ek_shard_rows or the nnz-balanced ek_shard_map alike).
int ek_spmv_setup(ek_ctx* c, int64_t n, int64_t row0, int64_t nrows, const int32_t* rowptr, const int32_t* col,
                  const double* val) {
    EK_TRY
    check_ctx(c);
    if (n <= 0 || row0 < 0 || nrows < 0 || row0 + nrows > n || !rowptr || (nrows && (!col || !val)))
        ek::fail(EK_EINVAL, "ek_spmv_setup: bad argument");
    std::vector<int64_t> off{0, n};
    if (c->mr) {
        c->scal.ensure(64);
        c->xexp.ensure(size_t(2 * c->nranks) * 8);
        const double mine[2] = {double(row0), double(nrows)};
        HIPCHK(hipMemcpyAsync(c->scal.p, mine, 16, hipMemcpyHostToDevice, c->stream));
        allgather(c, c->scal.as<double>(), 2, c->xexp.as<double>());
        std::vector<double> all(size_t(2 * c->nranks));
        HIPCHK(hipMemcpyAsync(all.data(), c->xexp.p, all.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        off.assign(size_t(c->nranks) + 1, 0);
        for (int r = 0; r < c->nranks; ++r) {
            if (int64_t(all[size_t(2 * r)]) != off[size_t(r)])
                ek::fail(EK_EINVAL, "ek_spmv_setup: rank %d's rows start at %lld, not where rank %d's end (%lld)", r,
                         (long long)all[size_t(2 * r)], r - 1, (long long)off[size_t(r)]);
            off[size_t(r) + 1] = off[size_t(r)] + int64_t(all[size_t(2 * r) + 1]);
        }
        if (off.back() != n) ek::fail(EK_EINVAL, "ek_spmv_setup: the ranks' rows cover %lld of %lld", (long long)off.back(), (long long)n);
    } else if (row0 != 0 || nrows != n) {
        ek::fail(EK_EINVAL, "ek_spmv_setup: a single context owns all %lld rows", (long long)n);
    }
    spmv_setup_rows(c, n, off, rowptr, col, val);
    return EK_OK;
    EK_CATCH
}

int ek_spmv_dims(ek_ctx* c, int64_t* n, int64_t* row0, int64_t* nrows) {
    EK_TRY
    check_ctx(c);
    if (n) *n = c->n;
    if (row0) *row0 = c->row0;
    if (nrows) *nrows = c->nrows;
    return EK_OK;
    EK_CATCH
}

// the body of ek_spmv_setup_pins; trusted_raw >= 0: the pins come from an
// ek_hgr (every constructor validates them: ranges, monotone offsets) whose
// reader counted the raw entries, so the two input scans (~0.25 ms at the
// headline, bound by reading 4.3 MB) are skipped.  net_w (nets values, or
// null: the unweighted build and its kernels): the net-weighted Laplacian of
// ek_spmv_setup_pins_w, on the device and in every fallback below;
// trusted_w: an ek_hgr's weights, >= 1 by construction
static int spmv_setup_pins_impl(ek_ctx* c, int64_t n, int64_t nets, const int64_t* net_ptr, const int32_t* pins,
                                const int32_t* net_w, bool trusted_w, int32_t* on_device, int64_t trusted_raw) {
    EK_TRY
    check_ctx(c);
    if (n <= 0 || n > INT32_MAX || nets < 0 || !net_ptr || (net_ptr[nets] > 0 && !pins) || net_ptr[0] != 0)
        ek::fail(EK_EINVAL, "ek_spmv_setup_pins: bad argument");
    if (net_w && !trusted_w)
        for (int64_t e = 0; e < nets; ++e)
            if (net_w[e] < 1)
                ek::fail(EK_EINVAL, "ek_spmv_setup_pins_w: weight %d of net %lld (>= 1)", net_w[e], (long long)e);
    const int64_t npins = net_ptr[nets];
    if (npins > INT32_MAX) ek::fail(EK_EINVAL, "ek_spmv_setup_pins: too many pins");
    ek::PhaseTimer pt("spmv_setup_pins");
    // (both scans branch-free; the error paths re-scan)
    int64_t raw_bound = trusted_raw;  // raw entries: every pin of a net of k >= 2 pins sees k - 1 others
    if (trusted_raw < 0) {
        raw_bound = 0;
        bool non_monotone = false;
        for (int64_t e = 0; e < nets; ++e) {
            const int64_t k = net_ptr[e + 1] - net_ptr[e];
            non_monotone |= k < 0;
            raw_bound += k >= 2 ? k * (k - 1) : 0;
        }
        if (non_monotone) ek::fail(EK_EINVAL, "ek_spmv_setup_pins: net_ptr not monotone");
    }
    // this rank's rows: the nnz-balanced shard map, computed from the pins
    // identically on every rank (no collective)
    std::vector<int64_t> off(size_t(c->nranks) + 1, 0);
    off[1] = n;
    if (c->mr) {
        const int rc = ek_shard_map(n, nets, net_ptr, pins, c->nranks, off.data());
        if (rc != EK_OK) throw ek::Error{rc};
    }
    const int64_t row0 = off[size_t(c->rank)], nrows = off[size_t(c->rank) + 1] - row0;
    pt.mark("raw bound, shard map");
    hipStream_t s = c->stream;
    auto host_fallback = [&](const char* why) {
        if (env_set("EK_TRACE")) std::fprintf(stderr, "[spmv_setup_pins] host build: %s\n", why);
        ek_hgr h;
        h.nets = nets;
        h.nodes = n;
        h.net_ptr.assign(net_ptr, net_ptr + nets + 1);
        h.pins.assign(pins, pins + npins);
        if (net_w) h.net_w.assign(net_w, net_w + nets);
        ek_csr L;
        ek::build_laplacian_rows(h, row0, row0 + nrows, L, net_w != nullptr);
        spmv_setup_rows(c, n, off, L.rowptr.data(), L.col.data(), L.val64.data());
        if (on_device) *on_device = 0;
    };
    if (env_set("EK_HOST_LAPLACIAN")) {
        host_fallback("EK_HOST_LAPLACIAN");
        return EK_OK;
    }
    if (trusted_raw < 0) {
        int32_t lo = INT32_MAX, hi = INT32_MIN;
        for (int64_t p = 0; p < npins; ++p) {
            lo = std::min(lo, pins[p]);
            hi = std::max(hi, pins[p]);
        }
        if (npins > 0 && (lo < 0 || int64_t(hi) >= n))
            for (int64_t p = 0; p < npins; ++p)  // the first offender, for the message
                if (pins[p] < 0 || pins[p] >= n) ek::fail(EK_EINVAL, "ek_spmv_setup_pins: pin %d out of range", pins[p]);
    }
    pt.mark("input checks");
    {
        Uploader up(c, s, (size_t(nets) + 1) * 8 + size_t(std::max<int64_t>(npins, 1)) * 4 +
                              (net_w ? size_t(std::max<int64_t>(nets, 1)) * 4 : 0));
        up.put(c->lb_netptr, net_ptr, size_t(nets) + 1);
        up.put(c->lb_pins, pins, size_t(npins));  // (no pins: an allocation all the same, nothing read from `pins`)
        if (net_w) up.put(c->lb_cw, net_w, size_t(nets));
    }
    pt.mark("pins staged");
    const size_t nr = size_t(nrows);
    ek::dev::LapBuild b;
    b.nets = nets;
    b.r0 = row0;
    b.r1 = row0 + nrows;
    b.net_ptr = c->lb_netptr.as<int64_t>();
    b.pins = c->lb_pins.as<int32_t>();
    b.cw = net_w ? c->lb_cw.as<int32_t>() : nullptr;
    c->lb_icnt.ensure((nr + 1) * 4);
    c->lb_rcnt.ensure((nr + 1) * 4);
    c->lb_cur.ensure((nr + 1) * 4);
    c->lb_cnt.ensure(16);
    HIPCHK(hipMemsetAsync(c->lb_icnt.p, 0, (nr + 1) * 4, s));
    HIPCHK(hipMemsetAsync(c->lb_rcnt.p, 0, (nr + 1) * 4, s));
    HIPCHK(hipMemsetAsync(c->lb_cur.p, 0, (nr + 1) * 4, s));
    HIPCHK(hipMemsetAsync(c->lb_cnt.p, 0, 16, s));
    c->lb_ip.ensure((nr + 1) * 8);
    c->lb_rp.ensure((nr + 1) * 8);
    c->lb_off.ensure((nr + 1) * 8);
    constexpr int TSIZE = 1 << 16;  // dictionary table slots (power of two)
    c->lb_tiles.ensure((std::max<size_t>(nr, TSIZE) / 1024 + 2) * 8);
    c->lb_inc.ensure(size_t(std::max<int64_t>(npins, 1)) * 8);
    const size_t raw = size_t(std::max<int64_t>(raw_bound, 1));
    c->lb_scol.ensure(raw * 4);
    c->lb_sval.ensure(raw * 8);
    c->lb_tval.ensure(raw * 8);
    c->lb_ulen.ensure((nr + 1) * 4);
    c->lb_len.ensure((nr + 1) * 4);
    c->lb_diag.ensure((nr + 1) * 8);
    c->lb_long.ensure((nr + 1) * 4);
    b.icnt = c->lb_icnt.as<int>();
    b.rcnt = c->lb_rcnt.as<int>();
    b.cur = c->lb_cur.as<int>();
    b.ip = c->lb_ip.as<long long>();
    b.rp = c->lb_rp.as<long long>();
    b.inc = c->lb_inc.as<int32_t>();
    b.scol = c->lb_scol.as<int>();
    b.sval = c->lb_sval.as<double>();
    b.tval = c->lb_tval.as<double>();
    b.ulen = c->lb_ulen.as<int>();
    b.len = c->lb_len.as<int>();
    b.diag = c->lb_diag.as<double>();
    b.long_rows = c->lb_long.as<int>();
    b.counters = c->lb_cnt.as<int>();
    long long* tiles = c->lb_tiles.as<long long>();
    ek::dev::lap_count(s, b);
    ek::dev::exclusive_scan(s, b.icnt, int64_t(nr), b.ip, tiles);
    ek::dev::exclusive_scan(s, b.rcnt, int64_t(nr), b.rp, tiles);
    ek::dev::lap_fill_rows(s, b);
    int cnt_h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt_h, b.counters, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // k_rows counted the rows past the LDS sort: none of their lengths was
    // written (the buffers come from hipMalloc as they are), so the host
    // build is taken before the scan of b.len and k_row_write would read them
    if (cnt_h[1] > 0) {
        host_fallback("a row longer than the LDS sort");
        return EK_OK;
    }
    ek::dev::lap_long_rows(s, b, cnt_h[0]);
    ek::dev::exclusive_scan(s, b.len, int64_t(nr), c->lb_off.as<long long>(), tiles);
    // CSR on the device: rowptr (local), col, val; at most raw + nrows entries
    c->rowptr.ensure((nr + 1) * 4);
    c->col.ensure((raw + nr) * 4);
    c->val.ensure((raw + nr) * 8);
    ek::dev::lap_write(s, b, c->lb_off.as<long long>(), c->rowptr.as<int>(), c->col.as<int>(), c->val.as<double>());
    std::vector<int32_t> rowptr(nr + 1);
    HIPCHK(hipMemcpyAsync(rowptr.data(), c->rowptr.p, (nr + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cnt_h, b.counters, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    pt.mark("rows on device");
    if (cnt_h[1] > 0) {
        host_fallback("a row longer than the LDS sort");
        return EK_OK;
    }
    const int64_t nnz = rowptr[nr];
    set_shard(c, n, off);
    c->n = n;
    c->nnz = nnz;
    const std::vector<long long> offll(off.begin(), off.end());  // (alive until the stream is drained below)
    c->own_ready = false;
    if (c->mr) {  // global columns -> the all-gather layout (monotone: rows stay sorted)
        upload(c->off_d, offll.data(), offll.size(), s);
        ek::dev::remap_cols(s, nnz, c->col.as<int>(), c->off_d.as<long long>(), c->nranks, c->slot);
        own_build_dev(c, s, tiles);
        // the halo layout is worked out on the host from this rank's columns
        std::vector<int32_t> ch(size_t(std::max<int64_t>(nnz, 1)));
        if (nnz) HIPCHK(hipMemcpyAsync(ch.data(), c->col.p, size_t(nnz) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (halo_build(c, ch.data(), nnz) && nnz)
            HIPCHK(hipMemcpyAsync(c->col.p, ch.data(), size_t(nnz) * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        pt.mark("halo layout");
    }
    // the same greedy row blocks as the host path (ek_spmv_setup)
    int colbits = 1;
    while (colbits < 31 && (int64_t(1) << colbits) < x_extent(c)) ++colbits;
    bool packed = !env_flag("EK_SPMV_PLAIN", false) && colbits <= 28;
    int64_t ncodes = 0;
    if (packed) {
        c->lb_table.ensure(size_t(TSIZE) * 8);
        c->lb_flags.ensure(size_t(TSIZE) * 4);
        c->lb_codes.ensure((size_t(TSIZE) + 1) * 8);
        ek::dev::dict_build(s, nnz, c->val.as<double>(), c->lb_table.as<unsigned long long>(), TSIZE,
                            b.counters + 1, c->lb_flags.as<int>(), c->lb_codes.as<long long>(), tiles);
        long long nd = 0;
        HIPCHK(hipMemcpyAsync(&nd, c->lb_codes.as<long long>() + TSIZE, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cnt_h, b.counters, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ncodes = nd;
        packed = cnt_h[1] == 0 && nd <= TSIZE / 2 && nd <= (int64_t(1) << (32 - colbits));
    }
    c->pn_G = 0;
    if (packed && nrows > 0 && want_panels(c)) {  // (no rows: no panel workgroups; the one empty row block)
        DBuf pk_d;
        c->dict.ensure(size_t(std::max<int64_t>(ncodes, 1)) * 8);
        ek::dev::dict_values(s, c->lb_table.as<unsigned long long>(), TSIZE, c->lb_codes.as<long long>(),
                             c->dict.as<double>());
        pk_d.ensure(size_t(std::max<int64_t>(nnz, 1)) * 4);
        ek::dev::encode_words(s, nnz, c->col.as<int>(), c->val.as<double>(), c->lb_table.as<unsigned long long>(), TSIZE,
                              c->lb_codes.as<long long>(), colbits, pk_d.as<uint32_t>());
        if (build_panels(c, s, rowptr.data(), c->rowptr.as<int32_t>(), pk_d.as<uint32_t>(), colbits, ncodes)) {
            c->colbits = colbits;
            pt.mark("panels");
            if (on_device) *on_device = 1;
            return EK_OK;
        }
    }
    c->block_nnz = ek::dev::SPMV_SEG_NNZ;  // (coded or plain: the same row blocks, so the same sums)
    auto rbv = ek::dev::spmv_row_blocks(rowptr.data(), nrows, c->block_nnz);
    c->nrb_spmv = int(rbv.size() / 4);
    c->spmv_long = false;
    for (size_t bk = 0; bk < rbv.size() / 4; ++bk) c->spmv_long = c->spmv_long || rbv[4 * bk + 3] > c->block_nnz;
    if (packed) {
        const size_t nb = size_t(c->nrb_spmv), SEG = size_t(ek::dev::SPMV_SEG_NNZ);
        size_t over = 0;  // long rows: overflow area after the segments (spmv_segment's layout)
        for (size_t bk = 0; bk < nb; ++bk)
            if (size_t(rbv[4 * bk + 3]) > SEG) {
                rbv[4 * bk + 2] = int32_t(nb * SEG + over);
                over += size_t(rbv[4 * bk + 3]);
            }
        c->pk.ensure((nb * SEG + over) * 4);
        c->rel.ensure(nb * ek::dev::SPMV_REL_STRIDE * 2);
        c->dict.ensure(size_t(std::max<int64_t>(ncodes, 1)) * 8);
        upload(c->rb, rbv.data(), rbv.size(), s);
        ek::dev::dict_values(s, c->lb_table.as<unsigned long long>(), TSIZE, c->lb_codes.as<long long>(),
                             c->dict.as<double>());
        ek::dev::encode_segments(s, int(nb), c->rb.as<int32_t>(), c->rowptr.as<int>(), c->col.as<int>(),
                                 c->val.as<double>(), c->lb_table.as<unsigned long long>(), TSIZE,
                                 c->lb_codes.as<long long>(), colbits, c->pk.as<uint32_t>(), c->rel.as<uint16_t>());
        c->colbits = colbits;
        c->mat_bytes = int64_t((nb * SEG + over) * 4 + nb * ek::dev::SPMV_REL_STRIDE * 2 + size_t(ncodes) * 8 +
                               rbv.size() * 4);
    } else {
        upload(c->rb, rbv.data(), rbv.size(), s);
        c->colbits = 0;
        c->mat_bytes = 12 * nnz + 4 * (nrows + 1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    pt.mark("blocks + coding");
    if (on_device) *on_device = 1;
    return EK_OK;
    EK_CATCH
}

int ek_spmv_setup_pins(ek_ctx* c, int64_t n, int64_t nets, const int64_t* net_ptr, const int32_t* pins,
                       int32_t* on_device) {
    return spmv_setup_pins_impl(c, n, nets, net_ptr, pins, nullptr, false, on_device, -1);
}

int ek_spmv_setup_pins_w(ek_ctx* c, int64_t n, int64_t nets, const int64_t* net_ptr, const int32_t* pins,
                         const int32_t* net_w, int32_t* on_device) {
    return spmv_setup_pins_impl(c, n, nets, net_ptr, pins, net_w, false, on_device, -1);
}

// x is the global n-vector; a sharded context reads it through its padded
// all-gather layout, so the ranks' slices are copied into that first (into a
// buffer of its own, not the solve's scratch: one ek_spmv at a time per
// sharded context, on any stream)
int ek_spmv(ek_ctx* c, const double* x, double* y, void* stream) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_spmv before ek_spmv_setup");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const double* xs = x;
    if (c->halo) {  // the compact halo layout, gathered from the global x
        if (c->spx.bytes < size_t(x_extent(c)) * 8) ek::fail(EK_ESTATE, "ek_spmv: shard layout not set up");
        ek::dev::gather_idx(s, x, c->hx_gidx.as<int>(), (long long)x_extent(c), c->spx.as<double>());
        xs = c->spx.as<double>();
    } else if (c->mr) {
        if (c->spx.bytes < size_t(x_extent(c)) * 8) ek::fail(EK_ESTATE, "ek_spmv: shard layout not set up");
        for (int r = 0; r < c->nranks; ++r) {
            const int64_t a = c->shard_off[size_t(r)], b = c->shard_off[size_t(r) + 1];
            if (b > a)
                HIPCHK(hipMemcpyAsync(c->spx.as<double>() + r * c->slot, x + a, size_t(b - a) * 8,
                                      hipMemcpyDeviceToDevice, s));
        }
        xs = c->spx.as<double>();
    }
    ek::dev::spmv(s, spmv_mat(c), xs, y, nullptr, nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return EK_OK;
    EK_CATCH
}

int ek_spmv_host(ek_ctx* c, const double* x, double* y) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_spmv_host before ek_spmv_setup");
    DBuf dx, dy;
    std::vector<double> xp;  // sharded: the padded all-gather layout (or the halo layout)
    if (c->halo) {
        xp.assign(size_t(x_extent(c)), 0.0);
        for (size_t t = 0; t < xp.size(); ++t)
            if (c->hx_gidx_h[t] >= 0) xp[t] = x[c->hx_gidx_h[t]];
        x = xp.data();
    } else if (c->mr) {
        xp.assign(size_t(x_extent(c)), 0.0);
        for (int r = 0; r < c->nranks; ++r)
            std::copy(x + c->shard_off[size_t(r)], x + c->shard_off[size_t(r) + 1], xp.begin() + r * c->slot);
        x = xp.data();
    }
    upload(dx, x, size_t(x_extent(c)), c->stream);
    dy.ensure(size_t(std::max<int64_t>(c->nrows, 1)) * 8);
    ek::dev::spmv(c->stream, spmv_mat(c), dx.as<double>(), dy.as<double>(), nullptr, nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    if (c->nrows) HIPCHK(hipMemcpyAsync(y, dy.p, size_t(c->nrows) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return EK_OK;
    EK_CATCH
}

int ek_spmv_gather_bench(ek_ctx* c, int iters, double* avg_us) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_spmv_gather_bench before ek_spmv_setup");
    if (iters <= 0 || !avg_us) ek::fail(EK_EINVAL, "ek_spmv_gather_bench: bad argument");
    hipStream_t s = c->stream;
    const size_t X = size_t(x_extent(c));
    DBuf x, sink;
    x.ensure(X * 8);
    sink.ensure(size_t(std::max(std::max(c->nrb_spmv, c->pn_G), 1)) * 8);
    std::vector<double> h(X);
    for (size_t i = 0; i < X; ++i) h[i] = double((i * 2654435761u) % 1000u) / 1000.0 - 0.5;
    HIPCHK(hipMemcpyAsync(x.p, h.data(), X * 8, hipMemcpyHostToDevice, s));
    const auto m = spmv_mat(c);
    // EK_GATHER_MODE (lab, kernels_spmv.hip k_lab_gather_step): 1 the gather +
    // a skipped step's update as two launches, 2 as one grid with an in-launch
    // wait, 3 the update alone; 0 (default) the gather-only ceiling
    const int mode = env_int("EK_GATHER_MODE", 0);
    DBuf part, ctr, wv, fv, fpart;
    const int R = int(std::max<int64_t>(c->nrows, 1));
    if (mode) {
        if (mode < 0 || mode > 3 || !m.pk || m.panel.G > 0 || c->mr)
            ek::fail(EK_EINVAL, "EK_GATHER_MODE %d: the single-context coded CSR form only", mode);
        if (mode == 2 && m.nblocks > ek::dev::lab_step_capacity())
            ek::fail(EK_EINVAL, "EK_GATHER_MODE 2: %d blocks exceed the %d resident at once", m.nblocks,
                     ek::dev::lab_step_capacity());
        part.ensure(size_t(m.nblocks) * 8);
        ctr.ensure(66 * 64 * 4);
        wv.ensure(size_t(R) * 3 * 8);
        fv.ensure(size_t(R) * 8);
        fpart.ensure(size_t(m.nblocks) * 8);
        HIPCHK(hipMemsetAsync(part.p, 0, part.bytes, s));
        HIPCHK(hipMemsetAsync(ctr.p, 0, ctr.bytes, s));
        HIPCHK(hipMemsetAsync(wv.p, 0, wv.bytes, s));
    }
    unsigned gen = 0;
    auto launch = [&] {
        if (!mode) return ek::dev::spmv_gather_only(s, m, x.as<double>(), sink.as<double>());
        ++gen;
        const double* w = wv.as<double>();
        ek::dev::lab_gather_step(s, m, mode, x.as<double>(), part.as<double>(), ctr.as<unsigned>(),
                                 gen, R, w, w + R, w + 2 * size_t(R), fv.as<double>(),
                                 fpart.as<double>());
    };
    for (int i = 0; i < 10; ++i) launch();
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) launch();
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    *avg_us = 1e3 * double(ms) / iters;
    return EK_OK;
    EK_CATCH
}

int ek_spmv_bench(ek_ctx* c, int iters, int fused, double* avg_us) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_spmv_bench before ek_spmv_setup");
    if (iters <= 0 || !avg_us) ek::fail(EK_EINVAL, "ek_spmv_bench: bad argument");
    // (a sharded context: this rank's rows over the padded all-gather layout,
    // x synthetic in every slot; no collective — bench.py's per-shard leg)
    hipStream_t s = c->stream;
    const size_t X = size_t(x_extent(c)), R = size_t(std::max<int64_t>(c->nrows, 1));
    DBuf x, y, vcol, apart, fn2;
    x.ensure(X * 8);
    y.ensure(R * 8);
    vcol.ensure(R * 8);
    apart.ensure(size_t(std::max(c->nrb_spmv, 1)) * 8);
    fn2.ensure(8);
    std::vector<double> h(X);
    for (size_t i = 0; i < X; ++i) h[i] = double((i * 2654435761u) % 1000u) / 1000.0 - 0.5;
    double nrm = 0.0;
    for (double v : h) nrm += v * v;
    HIPCHK(hipMemcpyAsync(x.p, h.data(), X * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(fn2.p, &nrm, 8, hipMemcpyHostToDevice, s));
    // this rank's rows of x
    const double* fsrc = x.as<double>() + (c->halo ? size_t(c->hx_base[size_t(c->rank)]) : c->mr ? size_t(c->rank * c->slot) : 0);
    // fused == 2: also the Lanczos step's finalize folded into the prologue
    // (||f||^2 from the update's one value, block 0 publishing alpha / offd)
    // and the ||w||^2 partials of partial reorthogonalisation: the SpMV exactly
    // as the solve launches it
    DBuf scratch, wp;
    ek::dev::StepFin fin;
    if (fused == 2) {
        scratch.ensure(64 * 8);
        wp.ensure(size_t(std::max(c->nrb_spmv, 1)) * 8);
        std::vector<double> sv(64, 0.0);
        sv[0] = nrm;   // fast: ||f||^2
        sv[1] = nrm;   // fn2_i
        sv[2] = 0.5;   // a3
        sv[3] = std::nan("");  // bov (no override)
        HIPCHK(hipMemcpyAsync(scratch.p, sv.data(), 64 * 8, hipMemcpyHostToDevice, s));
        double* sc = scratch.as<double>();
        fin.npart = sc + 40;
        fin.nb = 1;
        fin.fast = sc;
        fin.fn2_out = sc + 8;
        fin.h2 = sc + 16;
        fin.step = 1;
        fin.alpha = sc + 24;
        fin.offd = sc + 32;
        fin.a3 = sc + 2;
        fin.fn2_i = sc + 1;
        fin.bov_i = sc + 3;
        fin.wpart = wp.as<double>();
    }
    auto launch = [&] {
        if (fused)
            ek::dev::spmv(s, spmv_mat(c), x.as<double>(), y.as<double>(), fn2.as<double>(), fsrc,
                          vcol.as<double>(), apart.as<double>(), fused == 2 ? &fin : nullptr);
        else
            ek::dev::spmv(s, spmv_mat(c), x.as<double>(), y.as<double>(), nullptr, nullptr, nullptr, nullptr);
    };
    for (int i = 0; i < 10; ++i) launch();
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) launch();
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    *avg_us = 1e3 * double(ms) / iters;
    return EK_OK;
    EK_CATCH
}

int64_t ek_spmv_bytes(ek_ctx* c) {
    if (!c) return 0;
    return 12 * c->nnz + 4 * (c->nrows + 1) + 8 * c->n + 8 * c->nrows;
}

int ek_spmv_format(ek_ctx* c, int32_t* packed, int64_t* stored_bytes) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_spmv_format before ek_spmv_setup");
    // coded: segments (padding included) + row starts + table + descriptors; plain: CSR
    const int64_t mat = c->mat_bytes;
    if (packed) *packed = c->colbits > 0 ? 1 : 0;
    if (stored_bytes) *stored_bytes = mat + 8 * c->n + 8 * c->nrows;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"

namespace ek {
// ek_spmv_setup_pins for an ek_hgr's pins (valid by construction), with the
// raw-entry count its reader made when known
int spmv_setup_hgr(ek_ctx* c, const ek_hgr& h, int32_t* on_device) {
    return spmv_setup_pins_impl(c, h.nodes, h.nets, h.net_ptr.data(), h.pins.data(), nullptr, false, on_device,
                                h.raw_pairs);
}
int spmv_setup_hgr_w(ek_ctx* c, const ek_hgr& h, int32_t* on_device) {
    return spmv_setup_pins_impl(c, h.nodes, h.nets, h.net_ptr.data(), h.pins.data(),
                                h.net_w.empty() ? nullptr : h.net_w.data(), true, on_device, h.raw_pairs);
}
}  // namespace ek
