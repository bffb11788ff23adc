// What the runtime files of libeigkl_hip.so share (host code over the HIP
// runtime + RCCL): the error macros, the owning device buffer, the pinned
// upload staging, struct ek_ctx and the helpers that cross the files.
// Included by them only:
//   ctx.cpp          the context's lifetime, streams, the Uploader
//   ctx_comm.cpp     collectives and their timing, shard map, halo exchange
//   ctx_spmv.cpp     SpMV set-up (host rows / device Laplacian build), ek_spmv*
//   ctx_lanczos.cpp  the implicitly restarted Lanczos, ek_lanczos_fiedler
//   ctx_kl.cpp, ctx_kway.cpp, ctx_kway_refine_w.cpp, ctx_kway_jet.cpp, ctx_sweep.cpp, ctx_fm.cpp   the partition drivers
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <limits>
#include <map>
#include <memory>
#include <tuple>

#include "ek_internal.hpp"

#define HIPCHK(call)                                                                                 \
    do {                                                                                             \
        const hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                      \
            (void)hipGetLastError(); /* a failed call leaves no sticky error for the next entry */    \
            ek::fail(EK_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                            \
    } while (0)
#define NCCLCHK(call)                                                                                 \
    do {                                                                                              \
        const ncclResult_t r_ = (call);                                                               \
        if (r_ != ncclSuccess) ek::fail(EK_ECOMM, "%s failed: %s", #call, ncclGetErrorString(r_));    \
    } while (0)

namespace ek::rt {

// Owning device allocation.
struct DBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void ensure(size_t b) {
        if (b <= bytes && p) return;
        reset();
        HIPCHK(hipMalloc(&p, b ? b : 16));
        bytes = b;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

template <class T>
void upload(DBuf& d, const T* h, size_t n, hipStream_t s) {
    d.ensure(n * sizeof(T));
    if (n) HIPCHK(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, s));
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline int64_t chunk_pad(int64_t n) { return std::max<int64_t>(round_up(n, ek::dev::KL_CHUNK_PAD), ek::dev::KL_CHUNK_PAD); }

// The EK_* environment switches, one spelling per meaning.  Each reads the
// variable when called (tests switch them inside one process).
// set at all, whatever the value
inline bool env_set(const char* k) { return std::getenv(k) != nullptr; }
// on/off: the first character is not '0'; unset or empty: dflt
inline bool env_flag(const char* k, bool dflt) {
    const char* e = std::getenv(k);
    return e && e[0] ? e[0] != '0' : dflt;
}
// an integer; unset or empty: dflt
inline int env_int(const char* k, int dflt) {
    const char* e = std::getenv(k);
    return e && e[0] ? std::atoi(e) : dflt;
}

}  // namespace ek::rt

// Setup uploads through the context's pinned staging: a copy from pageable
// memory makes the runtime pin (or bounce) the user pages on every call,
// which on freshly parsed arrays costs milliseconds; a memcpy into pinned
// memory and an async DMA do not.  The caller sizes the arena for all the
// uploads of one setup call and drains the stream before the next call.
// The main stream and the KL stream each have an arena of their own: the KL
// graph setup runs on ek_solve_file's host thread while the main thread
// uploads the pins for the Laplacian build.
struct Uploader {
    ek_ctx* c;
    hipStream_t s;
    unsigned char*& buf;  // c->up (main stream) or c->kup (KL stream)
    size_t& cap;
    size_t off = 0;
    Uploader(ek_ctx* ctx, hipStream_t st, size_t total);
    template <class T>
    void put(ek::rt::DBuf& d, const T* h, size_t n);
};

struct ek_ctx {
    using DBuf = ek::rt::DBuf;
    int device = 0;
    int num_cu = 256;  // compute units (the panel SpMV's resident workgroups)
    hipStream_t stream = nullptr;
    // the KL graph's setup (ek_kl_graph_setup / ek_kl_nets_setup) runs on its
    // own stream: ek_solve_file calls it from its host thread while the
    // Lanczos solve occupies `stream`
    hipStream_t kstream = nullptr;
    // RCCL, or the host-staged exchange of ek_comm_init_host
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    // the sharded layout and exchange (slot-padded all-gather, the one-all-
    // reduce step): nranks > 1, or a forced 1-rank communicator (EK_COMM_FORCE,
    // which runs the RCCL production path on one GPU: tests)
    bool mr = false;
    ek_allgather_fn host_ag = nullptr;
    ek_allreduce_fn host_ar = nullptr;
    void* host_user = nullptr;
    double* stage = nullptr;  // pinned staging of the host-staged exchange
    size_t stage_doubles = 0;
    unsigned char* up = nullptr;  // pinned staging of the setup uploads on `stream` (see Uploader)
    size_t up_bytes = 0;
    unsigned char* kup = nullptr;  // ... and on `kstream`
    size_t kup_bytes = 0;
    double comm_ms = 0.0;     // host-observed time inside collectives (current solve)
    int64_t n_ag = 0, n_ar = 0;  // collectives issued (current solve; sharded contexts)
    // Laplacian rows owned by this context.  Sharded: rank r owns
    // [shard_off[r], shard_off[r+1]) (nnz-balanced, so the slices differ);
    // nloc = the largest slice; each rank's f is all-gathered into a slot of
    // `slot` doubles (its rows, zero padding, its ||f||^2 partial at [ldv]),
    // and the matrix's columns are remapped to that padded layout.
    int64_t n = 0, row0 = 0, nrows = 0, nloc = 0, nnz = 0;
    std::vector<int64_t> shard_off;
    int64_t slot = 0;
    DBuf off_d, xexp;
    DBuf spx;  // ek_spmv's x in the all-gather layout (sharded), sized when the shard map is set
    // The halo exchange of the sharded step (halo_build): instead of every
    // rank's whole slot, each rank receives only the rows of f its columns
    // read, into a compact x: block q (ranks in order) holds the rows of rank
    // q this rank reads, ascending (its own block: all its rows), then q's
    // ||f||^2 partial at the block end (hx_pidx[q]): one message per peer, the
    // sender's packed rows closed by its partial.  The columns are remapped
    // monotonically to it, so rows stay sorted and every product is summed in
    // the same order as over the slot layout: the same bits.  Used where it
    // moves fewer bytes than the all-gather (EK_MR_HALO=0/1 forces either).
    bool halo = false;
    int halo_calls = 0;  // halo_build calls since the shard map was set (exactly one per setup: it is collective)
    std::vector<int64_t> hx_base;             // nranks + 1: block q at [hx_base[q], hx_base[q+1]), its partial last
    std::vector<int64_t> hx_rcnt;             // rows received from q (own: nrows); the block is hx_rcnt[q] + 1
    std::vector<int64_t> hx_scnt, hx_soff;    // rows sent to q, and that message's offset in hx_sbuf (+1: the partial)
    std::vector<int64_t> hx_src;              // host-staged: q's message to this rank inside q's (padded) sbuf
    std::vector<int32_t> hx_gidx_h;           // X[t]'s global row (-1: a partial slot)
    int64_t hx_nsend = 0, hx_smax = 0;
    DBuf hx_sidx, hx_sbuf, hx_X, hx_pidx, hx_gidx, hx_gbuf;
    // exchange accounting (sharded solves): exchanges, point-to-point
    // messages posted, and (with timing on) the exchanges' and all-reduces'
    // durations on the device (HIP events around them on their streams) or,
    // host-staged, as the host saw them
    int64_t hx_exchanges = 0, hx_sends = 0, hx_recvs = 0;
    double x_ms = 0.0, ar_ms = 0.0;
    int64_t x_timed = 0, ar_timed = 0;
    bool comm_time = false;
    std::vector<hipEvent_t> cm_ev;            // event pool, reused across solves
    std::vector<std::pair<int, int>> cm_rec;  // (kind: 0 exchange, 1 all-reduce; first event) of this solve
    size_t cm_used = 0;
    // the owned-slot part of a sharded rank's rows (plain CSR, local column
    // ids), summed while the all-gather of the other slots runs on `gstream`
    DBuf own_rowptr, own_col, own_val, own_rb, yown;
    int own_nrb = 0;
    int64_t own_nnz = 0;
    bool own_ready = false;
    hipStream_t gstream = nullptr;
    hipEvent_t ag_ev[2] = {nullptr, nullptr};
    // the column-panel form of the SpMV (pn_G > 0; kernels_panel.hip)
    int pn_G = 0, pn_P = 0, pn_pb = 0, pn_max_rows = 0, pn_ndict = 0;
    DBuf pn_wrow, pn_start, pn_word, pn_rid;
    int block_nnz = 1024, nrb_spmv = 0;
    bool spmv_long = true;  // a row block is one row longer than block_nnz (the SpMV's vector mode)
    DBuf rb, rowptr, col, val, pk, rel, dict;
    int colbits = 0;  // > 0: the dictionary-coded matrix (pk, dict) is the one the SpMV reads
    int64_t mat_bytes = 0;  // bytes of the matrix arrays one SpMV reads, as stored
    // Lanczos workspace
    DBuf V, Vn, f, w, xfull, part, h1, h2, alpha, offd, fn2, npart, apart, Qd, scal, bov;
    DBuf V32, Vn32;  // the basis's fp32 shadow (ek_lanczos_opts::basis32) and its restart buffer
    DBuf fbk;        // launches whose fp32-shadow update fell back to V (a device counter)
    DBuf actr;  // the SpMV's last-block counter (alpha hand-off), zero between launches
    DBuf gctr;  // the projection's column-group counters (k_gemvt hand-off), zero between launches
    // partial reorthogonalisation (reorth 3): the SpMV's ||w||^2 partials, the
    // omega ring (3 x OMEGA_LD), k_pro's state and its per-step decisions
    DBuf wpart, omega, prost, pflags;
    DBuf cflag;  // the sharded step's cancellation flags (update_mr), one double per step
    // HIP graphs of the single-context Lanczos step chunks (factorize_fused),
    // keyed by (first step, end, run start, V, V32): captured on a chunk's
    // second launch, replayed from its third; dropped when any buffer or
    // parameter the launches carry changes (lz_sig)
    std::map<std::tuple<int, int, int, const void*, const void*>, hipGraphExec_t> lz_graphs;
    std::map<std::tuple<int, int, int, const void*, const void*>, int> lz_seen;
    std::vector<uint64_t> lz_sig;
    // ctx_kl.cpp's
    struct Kl {
        // KL state
        int64_t n = 0, n0 = 0, n1 = 0, nets = 0;
        DBuf rowptr, col, w, side, side_init, locked, gp0, gp1, order0, order1, plist, pinfo0, pinfo1, nd, cinfo0, cinfo1,
            ckey0, ckey1, aux, seg, cutpart, cut0, log, out, sides_tmp, count, netptr, pins;
        bool graph_ready = false, part_ready = false, seg_ok = false, segc_ok = false;
        DBuf segc, wdict;
        int nwd = 0, wcolbits = 0;
        std::vector<int32_t> rowptr_h;  // host copy (row descriptors)
    } kl;
    // device build of the Laplacian rows (ek_spmv_setup_pins)
    DBuf lb_netptr, lb_pins, lb_icnt, lb_rcnt, lb_cur, lb_ip, lb_rp, lb_tiles, lb_inc, lb_scol, lb_sval, lb_tval,
        lb_ulen, lb_len, lb_diag, lb_long, lb_cnt, lb_off, lb_table, lb_flags, lb_codes;
    DBuf lb_cw;  // the net weights beside the pins (ek_spmv_setup_pins_w)
    std::vector<hipEvent_t> spmv_ev;   // SpMV timing events, created once per context
    double* pin = nullptr;             // pinned host staging (Ritz vector + residual rows)
    size_t pin_doubles = 0;
    // mid-cycle convergence checks of the Lanczos driver: a copy stream, two
    // pinned slots of {alpha, offd, fn2} and their events (created on first use)
    hipStream_t cstream = nullptr;
    hipEvent_t chk_done[2] = {nullptr, nullptr}, chk_copied[2] = {nullptr, nullptr};
    hipEvent_t fin_ev = nullptr;  // the final Ritz vector's host copy landed
    double* chk_pin = nullptr;
    // the checks' completion words (EK_CHK_POLL): one per slot, 256 B apart, in
    // pinned host memory the check's gather writes last; the host polls them
    unsigned* chk_word = nullptr;
    unsigned chk_seq = 0;
    double* q_pin = nullptr;  // pinned staging of the restart's Q (MAX_NCV x (MAX_NCV + 1)), then the kept
                              // projected matrix for k_pro (2 x (MAX_NCV + 2))
    // the last Fiedler vector as returned (normalised, sign fixed), kept on
    // the device for ek_kl_set_partition_fiedler, and that split's scratch
    DBuf fied, sp_out, sp_tmp;
    int64_t fied_n = 0;
    DBuf rk_tmp;  // the rank split's per-block counts (ek_kl_set_partition_fiedler_rank)
};

template <class T>
void Uploader::put(ek::rt::DBuf& d, const T* h, size_t n) {
    d.ensure(n * sizeof(T));
    if (!n) return;
    off = (off + 63) / 64 * 64;
    if (off + n * sizeof(T) > cap) ek::fail(EK_EINVAL, "upload staging overflow");
    std::memcpy(buf + off, h, n * sizeof(T));
    HIPCHK(hipMemcpyAsync(d.p, buf + off, n * sizeof(T), hipMemcpyHostToDevice, s));
    off += n * sizeof(T);
}

namespace ek::rt {

inline void set_device(ek_ctx* c) { HIPCHK(hipSetDevice(c->device)); }

inline ek_ctx* check_ctx(ek_ctx* c) {
    if (!c) ek::fail(EK_EINVAL, "null ek_ctx");
    set_device(c);
    return c;
}

// What crosses the runtime files (each is commented where it is defined);
// hidden: internal to the library, not part of its dynamic symbols.
#pragma GCC visibility push(hidden)
// ctx_comm.cpp: the collectives seam, the shard map and the halo exchange
void allreduce(ek_ctx* c, double* p, size_t count);
void allgather(ek_ctx* c, const double* send, size_t count, double* recv, hipStream_t st = nullptr);
void comm_collect(ek_ctx* c);
void set_shard(ek_ctx* c, int64_t n, const std::vector<int64_t>& off);
int64_t x_extent(const ek_ctx* c);
bool halo_build(ek_ctx* c, int32_t* col, int64_t nnz);
void halo_exchange(ek_ctx* c, const double* src, hipStream_t st);
// ctx_spmv.cpp: the matrix as the SpMV launches take it
ek::dev::SpmvMat spmv_mat(const ek_ctx* c);
ek::dev::SpmvMat own_mat(const ek_ctx* c);
// ctx_sweep.cpp: the sort of the sweep cuts (ek_sweep_cut, ek_sweep_cut_w):
// order[r] the node at rank r of v (device, n doubles) and pos[order[r]] = r;
// scan_tmp is left large enough for sweep_scan over n + 1 words
struct SweepSort {
    DBuf keys[2], ids[2], ghist, table, scan_tmp, pos;
    int cur = 0;
    const int32_t* order() const { return ids[cur].as<int32_t>(); }
};
void sweep_sort(ek_ctx* c, const double* v, int64_t n, SweepSort& out);
#pragma GCC visibility pop

}  // namespace ek::rt
