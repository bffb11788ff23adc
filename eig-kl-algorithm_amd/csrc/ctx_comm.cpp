// The collectives seam of libeigkl_hip.so (RCCL or the host-staged exchange)
// and its timing, the shard map and the halo exchange of the sharded SpMV.
#include "ctx.hpp"

using namespace ek::rt;

namespace {

double* stage_for(ek_ctx* c, size_t doubles) {
    if (c->stage_doubles < doubles) {
        if (c->stage) HIPCHK(hipHostFree(c->stage));
        c->stage = nullptr;
        c->stage_doubles = 0;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->stage), doubles * 8, hipHostMallocDefault));
        c->stage_doubles = doubles;
    }
    return c->stage;
}

struct CommTimer {  // host-observed time of one collective (kind 0: an exchange of f, 1: an all-reduce)
    ek_ctx* c;
    int kind;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~CommTimer() {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        c->comm_ms += ms;
        if (!c->comm_time) return;
        (kind ? c->ar_ms : c->x_ms) += ms;
        ++(kind ? c->ar_timed : c->x_timed);
    }
};

// Device-side timing of the RCCL collectives of a sharded solve (comm_time:
// the solve's time_spmv): a pair of events from the context's pool around
// one exchange (kind 0) or all-reduce (kind 1) on its stream.  Their elapsed
// time holds the wait for the peers, i.e. what the step pays for the
// collective.  comm_collect sums them once the solve has drained.
int comm_mark(ek_ctx* c, hipStream_t st) {
    if (!c->comm_time || !c->comm) return -1;
    while (c->cm_used + 2 > c->cm_ev.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        c->cm_ev.push_back(e);
    }
    const int i = int(c->cm_used);
    c->cm_used += 2;
    HIPCHK(hipEventRecord(c->cm_ev[size_t(i)], st));
    return i;
}

void comm_done(ek_ctx* c, int i, int kind, hipStream_t st) {
    if (i < 0) return;
    HIPCHK(hipEventRecord(c->cm_ev[size_t(i) + 1], st));
    c->cm_rec.emplace_back(kind, i);
}

void comm_reset(ek_ctx* c) {
    if (c->comm) ncclCommDestroy(c->comm);
    c->comm = nullptr;
    c->host_ag = nullptr;
    c->host_ar = nullptr;
    c->host_user = nullptr;
    c->nranks = 1;
    c->rank = 0;
    c->mr = false;
}

// EK_COMM_FORCE=1: a 1-rank communicator still takes the multi-rank path
bool comm_forced() { return env_flag("EK_COMM_FORCE", false); }

inline int64_t gt_round(int64_t x) { return round_up(std::max<int64_t>(x, 1), ek::dev::GT_ROWS); }

}  // namespace

namespace ek::rt {

void comm_collect(ek_ctx* c) {
    for (const auto& r : c->cm_rec) {
        HIPCHK(hipEventSynchronize(c->cm_ev[size_t(r.second) + 1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->cm_ev[size_t(r.second)], c->cm_ev[size_t(r.second) + 1]));
        (r.first ? c->ar_ms : c->x_ms) += double(ms);
        ++(r.first ? c->ar_timed : c->x_timed);
    }
    c->cm_rec.clear();
    c->cm_used = 0;
}

// In-place sum all-reduce of `count` device doubles, ordered on the context
// stream.  RCCL: enqueued on the stream.  Host-staged: stream drained, the
// operand staged through pinned memory around the caller's collective.
void allreduce(ek_ctx* c, double* p, size_t count) {
    if (!c->mr || !count) return;
    ++c->n_ar;
    if (c->comm) {
        const int e = comm_mark(c, c->stream);
        NCCLCHK(ncclAllReduce(p, p, count, ncclDouble, ncclSum, c->comm, c->stream));
        comm_done(c, e, 1, c->stream);
        return;
    }
    CommTimer t{c, 1};
    double* h = stage_for(c, count);
    HIPCHK(hipMemcpyAsync(h, p, count * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->host_ar(c->host_user, h, int64_t(count)) != 0) ek::fail(EK_ECOMM, "host all-reduce callback failed");
    HIPCHK(hipMemcpyAsync(p, h, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // the staging buffer is reused by the next collective
}

// recv[r*count .. (r+1)*count) = rank r's send block (rank-major), on the
// stream (default: the context's).
void allgather(ek_ctx* c, const double* send, size_t count, double* recv, hipStream_t st) {
    ++c->n_ag;
    if (!st) st = c->stream;
    if (c->comm) {
        const int e = comm_mark(c, st);
        NCCLCHK(ncclAllGather(send, recv, count, ncclDouble, c->comm, st));
        comm_done(c, e, 0, st);
        return;
    }
    CommTimer t{c, 0};
    const size_t tot = count * size_t(c->nranks);
    double* h = stage_for(c, count + tot);
    HIPCHK(hipMemcpyAsync(h, send, count * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c->host_ag(c->host_user, h, int64_t(count), h + count) != 0)
        ek::fail(EK_ECOMM, "host all-gather callback failed");
    HIPCHK(hipMemcpyAsync(recv, h + count, tot * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
}

// The shard map `off` (nranks + 1 offsets tiling [0, n)) becomes the
// context's: its rows, the largest slice (nloc) and the all-gather slot.
void set_shard(ek_ctx* c, int64_t n, const std::vector<int64_t>& off) {
    if (int(off.size()) != c->nranks + 1 || off[0] != 0 || off.back() != n)
        ek::fail(EK_EINVAL, "shard map does not tile [0, %lld)", (long long)n);
    int64_t mx = 0;
    for (int r = 0; r < c->nranks; ++r) {
        if (off[size_t(r) + 1] < off[size_t(r)]) ek::fail(EK_EINVAL, "shard map not monotone");
        mx = std::max(mx, off[size_t(r) + 1] - off[size_t(r)]);
    }
    c->shard_off = off;
    c->halo = false;
    c->halo_calls = 0;
    c->hx_exchanges = c->hx_sends = c->hx_recvs = 0;
    c->x_ms = c->ar_ms = 0.0;
    c->x_timed = c->ar_timed = 0;
    c->row0 = off[size_t(c->rank)];
    c->nrows = off[size_t(c->rank) + 1] - c->row0;
    c->nloc = c->mr ? mx : n;
    // sharded: the Lanczos vectors' rows (ldv) + 64, the rank's ||f||^2 at [ldv]
    c->slot = c->mr ? gt_round(mx) + 64 : n;
    if (c->mr && c->slot * c->nranks > INT32_MAX) ek::fail(EK_EINVAL, "sharded vector layout exceeds int32");
    // (allocated here, not inside ek_spmv: a reallocation there could free
    // memory that work queued earlier still reads)
    if (c->mr) c->spx.ensure(size_t(c->slot * c->nranks) * 8);
}

// The column space the SpMV reads: global ids, the padded all-gather layout,
// or the compact halo layout
int64_t x_extent(const ek_ctx* c) { return c->halo ? c->hx_base.back() : c->mr ? c->slot * c->nranks : c->n; }

// The halo layout from this rank's columns in the slot layout (col, host, nnz
// entries; remapped in place when the halo exchange is taken).  One
// all-gather of the request counts (every rank then takes the same decision)
// and one of the request lists: setup only.  Collective: every rank of a
// sharded context calls it exactly once per setup, after set_shard (the host
// rows of spmv_setup_rows, or the device build's, whichever the rank took).
bool halo_build(ek_ctx* c, int32_t* col, int64_t nnz) {
    c->halo = false;
    if (c->mr && ++c->halo_calls != 1)
        ek::fail(EK_ESTATE, "halo_build called %d times in one setup (a collective: once per rank)", c->halo_calls);
    if (!c->mr || c->nranks > ek::dev::MAX_HALO_RANKS) return false;
    if (!env_flag("EK_MR_HALO", true)) return false;
    const int R = c->nranks, me = c->rank;
    const int64_t S = c->slot;
    const auto& off = c->shard_off;
    // which rows of each other rank this rank's columns read
    std::vector<std::vector<int32_t>> pos(static_cast<size_t>(R));
    for (int q = 0; q < R; ++q)
        if (q != me) pos[size_t(q)].assign(size_t(off[size_t(q) + 1] - off[size_t(q)]), -1);
    for (int64_t p = 0; p < nnz; ++p) {
        const int q = int(col[p] / S);
        if (q != me) pos[size_t(q)][size_t(col[p] - q * S)] = 0;
    }
    std::vector<std::vector<int32_t>> req(static_cast<size_t>(R));
    for (int q = 0; q < R; ++q) {
        auto& pq = pos[size_t(q)];
        for (size_t l = 0; l < pq.size(); ++l)
            if (pq[l] == 0) {
                pq[l] = int32_t(req[size_t(q)].size());
                req[size_t(q)].push_back(int32_t(l));
            }
    }
    // C[r * R + q] = rows rank r reads from rank q
    c->scal.ensure(64);
    DBuf cnt_d, all_d;
    cnt_d.ensure(size_t(R) * 8);
    all_d.ensure(size_t(R) * size_t(R) * 8);
    std::vector<double> mine(static_cast<size_t>(R), 0.0), C(size_t(R) * size_t(R));
    for (int q = 0; q < R; ++q) mine[size_t(q)] = double(req[size_t(q)].size());
    HIPCHK(hipMemcpyAsync(cnt_d.p, mine.data(), size_t(R) * 8, hipMemcpyHostToDevice, c->stream));
    allgather(c, cnt_d.as<double>(), size_t(R), all_d.as<double>());
    HIPCHK(hipMemcpyAsync(C.data(), all_d.p, C.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    auto Cat = [&](int r, int q) { return int64_t(C[size_t(r) * size_t(R) + size_t(q)]); };
    int64_t tot_halo = 0, lmax = 0;
    for (int r = 0; r < R; ++r) {
        int64_t lr = 0;
        for (int q = 0; q < R; ++q)
            if (q != r) {
                tot_halo += Cat(r, q) + 1;
                lr += Cat(r, q);
            }
        lmax = std::max(lmax, lr);
    }
    const int64_t full = int64_t(R) * int64_t(R - 1) * S;
    // (one forced rank: nothing to exchange either way; the slot layout)
    const bool use = env_flag("EK_MR_HALO", R > 1 && double(tot_halo) <= 0.75 * double(full));
    if (!use) return false;
    // the request lists, padded to the longest: rank r's request from this
    // rank starts at sum_{q < me, q != r} C[r][q] of r's list
    std::vector<double> lst(size_t(std::max<int64_t>(lmax, 1)), 0.0), lall(size_t(std::max<int64_t>(lmax, 1)) * R);
    {
        size_t o = 0;
        for (int q = 0; q < R; ++q)
            for (int32_t l : req[size_t(q)]) lst[o++] = double(l);
        DBuf ld, la;
        ld.ensure(lst.size() * 8);
        la.ensure(lall.size() * 8);
        HIPCHK(hipMemcpyAsync(ld.p, lst.data(), lst.size() * 8, hipMemcpyHostToDevice, c->stream));
        allgather(c, ld.as<double>(), lst.size(), la.as<double>());
        HIPCHK(hipMemcpyAsync(lall.data(), la.p, lall.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    const int32_t ldv = int32_t(S - 64);  // f[ldv]: the rank's ||f||^2 partial (the Lanczos vectors' ld)
    std::vector<int32_t> sidx;
    c->hx_scnt.assign(size_t(R), 0);
    c->hx_soff.assign(size_t(R), 0);
    for (int r = 0; r < R; ++r) {
        if (r == me) continue;
        int64_t o = 0;
        for (int q = 0; q < me; ++q)
            if (q != r) o += Cat(r, q);
        c->hx_soff[size_t(r)] = int64_t(sidx.size());
        c->hx_scnt[size_t(r)] = Cat(r, me);
        for (int64_t k = 0; k < Cat(r, me); ++k) sidx.push_back(int32_t(lall[size_t(r) * size_t(lst.size()) + size_t(o + k)]));
        sidx.push_back(ldv);
    }
    c->hx_nsend = int64_t(sidx.size());
    c->hx_rcnt.assign(size_t(R), 0);
    c->hx_base.assign(size_t(R) + 1, 0);
    std::vector<int32_t> pidx(static_cast<size_t>(R));
    for (int q = 0; q < R; ++q) {
        c->hx_rcnt[size_t(q)] = q == me ? c->nrows : Cat(me, q);
        pidx[size_t(q)] = int32_t(c->hx_base[size_t(q)] + c->hx_rcnt[size_t(q)]);  // q's partial: the block end
        c->hx_base[size_t(q) + 1] = c->hx_base[size_t(q)] + c->hx_rcnt[size_t(q)] + 1;
    }
    // host-staged exchange: q's sbuf lists its messages to r = 0, 1, ... (r != q)
    c->hx_src.assign(size_t(R), 0);
    c->hx_smax = 1;
    for (int q = 0; q < R; ++q) {
        int64_t o = 0;
        for (int r = 0; r < R; ++r) {
            if (r == q) continue;
            if (r == me) c->hx_src[size_t(q)] = o;
            o += Cat(r, q) + 1;
        }
        c->hx_smax = std::max(c->hx_smax, o);
    }
    // the columns, remapped (monotone: rows stay sorted)
    const int64_t base_me = c->hx_base[size_t(me)];
    for (int64_t p = 0; p < nnz; ++p) {
        const int q = int(col[p] / S);
        const int64_t l = col[p] - q * S;
        col[p] = int32_t(q == me ? base_me + l : c->hx_base[size_t(q)] + pos[size_t(q)][size_t(l)]);
    }
    // X's global rows (ek_spmv with a global x)
    c->hx_gidx_h.assign(size_t(c->hx_base.back()), -1);
    for (int q = 0; q < R; ++q) {
        const int64_t b = c->hx_base[size_t(q)];
        if (q == me)
            for (int64_t k = 0; k < c->nrows; ++k) c->hx_gidx_h[size_t(b + k)] = int32_t(c->row0 + k);
        else
            for (size_t k = 0; k < req[size_t(q)].size(); ++k)
                c->hx_gidx_h[size_t(b) + k] = int32_t(off[size_t(q)] + req[size_t(q)][k]);
    }
    if (sidx.empty()) sidx.push_back(0);  // (one forced rank: no messages; a valid upload)
    upload(c->hx_sidx, sidx.data(), sidx.size(), c->stream);
    upload(c->hx_gidx, c->hx_gidx_h.data(), c->hx_gidx_h.size(), c->stream);
    upload(c->hx_pidx, pidx.data(), pidx.size(), c->stream);
    c->hx_sbuf.ensure(size_t(std::max(c->hx_smax, c->hx_nsend)) * 8);
    c->hx_X.ensure(size_t(std::max<int64_t>(c->hx_base.back(), 1)) * 8);
    if (!c->comm) c->hx_gbuf.ensure(size_t(c->hx_smax) * size_t(R) * 8);
    HIPCHK(hipMemsetAsync(c->hx_sbuf.p, 0, c->hx_sbuf.bytes, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->halo = true;
    return true;
}

// One halo exchange of src (this rank's rows, its ||f||^2 partial at
// src[ldv]) into the compact x (c->hx_X), on stream st: the pack (each
// peer's message in sbuf: the rows it reads, closed by this rank's partial;
// the own block and partial straight into X), then ONE RCCL message to and
// one from every peer in one group — block q of X is exactly q's message,
// rows then partial — or, staged through the host, an all-gather of every
// rank's (padded) messages of which this rank copies its one piece per peer
// into the same block.  Counted as the step's one all-gather.
void halo_exchange(ek_ctx* c, const double* src, hipStream_t st) {
    const int R = c->nranks, me = c->rank;
    double* X = c->hx_X.as<double>();
    double* sb = c->hx_sbuf.as<double>();
    const int64_t bme = c->hx_base[size_t(me)];
    ek::dev::halo_pack(st, src, int(c->slot - 64), c->hx_sidx.as<int>(), c->hx_nsend, sb, X, bme, c->nrows,
                       X + bme + c->nrows);
    ++c->hx_exchanges;
    if (c->comm) {
        ++c->n_ag;
        if (R == 1) return;
        const int e = comm_mark(c, st);
        NCCLCHK(ncclGroupStart());
        for (int q = 0; q < R; ++q) {
            if (q == me) continue;
            const int64_t sc = c->hx_scnt[size_t(q)], rc = c->hx_rcnt[size_t(q)];
            NCCLCHK(ncclSend(sb + c->hx_soff[size_t(q)], size_t(sc + 1), ncclDouble, q, c->comm, st));
            NCCLCHK(ncclRecv(X + c->hx_base[size_t(q)], size_t(rc + 1), ncclDouble, q, c->comm, st));
            ++c->hx_sends;
            ++c->hx_recvs;
        }
        NCCLCHK(ncclGroupEnd());
        comm_done(c, e, 0, st);
        return;
    }
    if (R == 1) {
        ++c->n_ag;
        return;
    }
    double* g = c->hx_gbuf.as<double>();
    allgather(c, sb, size_t(c->hx_smax), g, st);
    c->hx_sends += R - 1;  // (this rank's messages ride in its all-gather block)
    for (int q = 0; q < R; ++q)
        if (q != me) {
            const double* m = g + size_t(q) * size_t(c->hx_smax) + c->hx_src[size_t(q)];
            HIPCHK(hipMemcpyAsync(X + c->hx_base[size_t(q)], m, size_t(c->hx_rcnt[size_t(q)] + 1) * 8,
                                  hipMemcpyDeviceToDevice, st));
            ++c->hx_recvs;
        }
}

}  // namespace ek::rt

extern "C" {

int ek_comm_unique_id(void* id128) {
    EK_TRY
    if (!id128) ek::fail(EK_EINVAL, "null id buffer");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    std::memcpy(id128, &id, sizeof id);
    return EK_OK;
    EK_CATCH
}

int ek_comm_init(ek_ctx* c, int nranks, int rank, const void* id128) {
    EK_TRY
    check_ctx(c);
    if (nranks < 1 || rank < 0 || rank >= nranks || !id128) ek::fail(EK_EINVAL, "ek_comm_init: bad argument");
    comm_reset(c);
    const bool mr = nranks > 1 || comm_forced();
    if (mr) {  // (nranks 1 under EK_COMM_FORCE: a real one-rank RCCL communicator)
        ncclUniqueId id;
        std::memcpy(&id, id128, sizeof id);
        NCCLCHK(ncclCommInitRank(&c->comm, nranks, id, rank));
    }
    c->nranks = nranks;
    c->rank = rank;
    c->mr = mr;
    c->n = 0;  // the shard map changed: ek_spmv_setup again
    return EK_OK;
    EK_CATCH
}

int ek_comm_init_host(ek_ctx* c, int nranks, int rank, ek_allgather_fn ag, ek_allreduce_fn ar, void* user) {
    EK_TRY
    check_ctx(c);
    const bool mr = nranks > 1 || comm_forced();
    if (nranks < 1 || rank < 0 || rank >= nranks || (mr && (!ag || !ar)))
        ek::fail(EK_EINVAL, "ek_comm_init_host: bad argument");
    comm_reset(c);
    c->nranks = nranks;
    c->rank = rank;
    c->mr = mr;
    c->host_ag = ag;
    c->host_ar = ar;
    c->host_user = user;
    c->n = 0;
    return EK_OK;
    EK_CATCH
}

int ek_comm_stats(ek_ctx* c, int64_t* exchanges, int64_t* sends, int64_t* recvs, double* exchange_ms,
                  int64_t* exchanges_timed, double* allreduce_ms, int64_t* allreduces_timed) {
    EK_TRY
    check_ctx(c);
    if (exchanges) *exchanges = c->hx_exchanges;
    if (sends) *sends = c->hx_sends;
    if (recvs) *recvs = c->hx_recvs;
    if (exchange_ms) *exchange_ms = c->x_ms;
    if (exchanges_timed) *exchanges_timed = c->x_timed;
    if (allreduce_ms) *allreduce_ms = c->ar_ms;
    if (allreduces_timed) *allreduces_timed = c->ar_timed;
    return EK_OK;
    EK_CATCH
}

int ek_spmv_exchange(ek_ctx* c, int32_t* halo, int64_t* recv_doubles, int64_t* send_doubles) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_spmv_exchange before ek_spmv_setup");
    int64_t rv = 0, sd = 0;
    if (c->halo) {
        for (int q = 0; q < c->nranks; ++q)
            if (q != c->rank) {
                rv += c->hx_rcnt[size_t(q)] + 1;
                sd += c->hx_scnt[size_t(q)] + 1;
            }
    } else if (c->mr) {
        rv = (c->nranks - 1) * c->slot;
        sd = (c->nranks - 1) * c->slot;
    }
    if (halo) *halo = c->halo ? 1 : 0;
    if (recv_doubles) *recv_doubles = rv;
    if (send_doubles) *send_doubles = sd;
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
