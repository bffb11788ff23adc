/*
 * eigkl.h — C-ABI of libeigkl_hip.so, the MI355X (gfx950) EIG+KL hypergraph
 * bipartitioner.  Plain pointers and sizes only; no torch / HIP types.
 *
 * The reference (yhinai/EIG-KL-Algorithm) has no library or FFI: its seams
 * are (1) the process/CLI + file boundary of cEIG/cKL/gKL/gKL2,
 * (2) Spectra's MatOp `perform_op(x_in, y_out)` consumed by SymEigsSolver at
 * cEIG.cpp:194-198, (3) gKL's `gpuConnections(...)` gain seam at
 * gKL.cu:188-227 driven by the KL loop at cKL.cpp:334-390.  Each entry point
 * below names the reference interface it replaces.
 *
 * Conventions: every int-returning call returns EK_OK (0) or a negative
 * ek_status; ek_last_error() gives a thread-local message.  The library never
 * calls exit() (unlike CHECK_CUDA at gKL.cu:87-94).  A context is bound to
 * one GPU and is not thread-safe; use one host thread (or process) per GPU.
 * There is NO CPU fallback: GPU entry points fail with EK_EHIP when no
 * gfx950 device is usable.
 */
#ifndef EIGKL_H
#define EIGKL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum ek_status {
    EK_OK = 0,
    EK_EINVAL = -1,  /* bad argument / malformed input file */
    EK_EIO = -2,     /* file cannot be opened / written */
    EK_EHIP = -3,    /* HIP runtime error or no usable GPU */
    EK_ENOMEM = -4,
    EK_ENOCONV = -5, /* eigensolver did not converge ("Eigenvalue computation failed", cEIG.cpp:200-202) */
    EK_ESTATE = -6,  /* call out of order (e.g. ek_kl_run before ek_kl_graph_setup) */
    EK_ECOMM = -7    /* RCCL error */
};

const char* ek_last_error(void);
const char* ek_version(void);
/* The struct layouts of this header (ek_lanczos_opts / _stats, ek_solve_opts,
 * ek_swap ...) carry no size field; a binding checks ek_abi_version() ==
 * EIGKL_ABI_VERSION before passing any of them.  Bumped whenever a public
 * struct changes layout (4: reorth_thresh, the stats' projected_steps /
 * reprojected / ortho_max, and reorth 3 as the default). */
#define EIGKL_ABI_VERSION 4
int ek_abi_version(void);

/* ------------------------------------------------------------------ */
/* Hypergraph ingest (host, no GPU)                                     */
/* ------------------------------------------------------------------ */
typedef struct ek_hgr ek_hgr;

/* Read a .hgr file: header "nets nodes", then one line per net of 1-based
 * pins.  Replaces the per-executable readers cEIG.cpp:177-182,91-101 and
 * cKL.cpp:84-116 (same line semantics: exactly `nets` lines are read). */
int ek_hgr_read(const char* path, ek_hgr** out);
/* Seeded ISPD98-shaped synthetic circuit: floor(201920*mult) nodes,
 * floor(210613*mult) nets, net sizes {2:84,3:2,4:6,5:2,6:4,8:2}/100, distinct
 * sorted pins.  Replaces circuit_generator.py:41-59 (whose RNG is unseeded). */
int ek_hgr_generate(double multiplier, uint64_t seed, ek_hgr** out);
/* Build from 0-based pins: net e owns pins[net_ptr[e] .. net_ptr[e+1]). */
int ek_hgr_from_pins(int64_t nets, int64_t nodes, const int64_t* net_ptr, const int32_t* pins,
                     ek_hgr** out);
/* Largest connected component of the pin graph (nets with >= 2 pins join
 * their pins; the largest component, ties to the one holding the smallest
 * node id), as a new hypergraph: its nets in file order, nodes renumbered in
 * ascending original id.  node_map (nodes of h, may be NULL) gets the new id
 * or -1.  No reference counterpart: the connected ibm18-scale workload the
 * disconnected synthetic lacks (SURVEY §0 finding 8). */
int ek_hgr_largest_component(const ek_hgr* h, ek_hgr** out, int32_t* node_map);
/* Write in the reference .hgr text format (circuit_generator.py:61-68). */
int ek_hgr_write(const ek_hgr* h, const char* path);
int ek_hgr_dims(const ek_hgr* h, int64_t* nets, int64_t* nodes, int64_t* pins);
int ek_hgr_copy_pins(const ek_hgr* h, int64_t* net_ptr /* nets+1 */, int32_t* pins /* pins */);
void ek_hgr_free(ek_hgr* h);

/* Optional weights.  A hypergraph may carry a node weight w(v) >= 0 per node
 * and a net weight c(e) >= 1 per net (int32); an absent array stands for all
 * ones.  Only the weighted FM refinement, the weighted sweep cut
 * (ek_sweep_cut_w*), the matching, the multilevel paths over them
 * (ek_multilevel_bipartition*, ek_partition_kway_ml), the weighted k-way
 * refinements (ek_kway_refine_w*, ek_kway_jet*) and the weighted metrics read them: the Laplacian, the KL graph, the Lanczos solve, the median, rank
 * and count-sweep splits, KL, ek_partition_kway, ek_kway_refine and
 * ek_fm_refine work on the structure alone.  ek_hgr_write writes a
 * weighted hypergraph in the hMETIS form below (fmt, the net weights, the node
 * weight lines) and an unweighted one as before; ek_hgr_induce and
 * ek_hgr_largest_component carry the kept nodes' and the surviving nets'
 * weights over.  No reference counterpart. */
/* Copies node_w (nodes values) and net_w (nets values) into h; a NULL pointer
 * clears that array.  EK_EINVAL for a node weight < 0 or a net weight < 1 (h
 * is then unchanged). */
int ek_hgr_set_weights(ek_hgr* h, const int32_t* node_w, const int32_t* net_w);
/* 1 / 0 per array h carries.  Either pointer may be NULL. */
int ek_hgr_weights(const ek_hgr* h, int32_t* has_node_w, int32_t* has_net_w);
/* The weights, 1s for an absent array.  Either pointer may be NULL. */
int ek_hgr_copy_weights(const ek_hgr* h, int32_t* node_w_out /* nodes */, int32_t* net_w_out /* nets */);
/* The hMETIS reading of a .hgr file.  Lines beginning with '%' are comments
 * anywhere.  Header "nets nodes [fmt]", fmt absent, 0, 1, 10 or 11.  Then
 * `nets` net lines of 1-based pins, each beginning with the net's weight when
 * fmt is 1 or 11; then, when fmt is 10 or 11, `nodes` lines of one node weight
 * each.  Without net weights a blank or missing net line is an empty net, as
 * in ek_hgr_read.  EK_EINVAL for any other fmt, a token that is no unsigned
 * integer (a negative weight among them), a missing or zero net weight, a pin
 * outside [1, nodes], a weight above INT32_MAX, a blank node weight line or
 * too few of them.  ek_hgr_read is not this reader: it keeps the reference's
 * line semantics and ignores a third header token. */
int ek_hgr_read_weighted(const char* path, ek_hgr** out);
/* out[0] = the weighted cut, the sum of c(e) over the cut nets; out[1] = the
 * cut nets; out[2], out[3] = W_0, W_1, the node weight on side 0 and side 1.
 * The conventions are the FM rule's: only nets with at least 2 distinct pins
 * count, a repeated pin once.  side: one byte in {0, 1} per node (EK_EINVAL
 * otherwise).  Written apart from the FM code: it is what the tests hold the
 * weighted FM to. */
int ek_bipart_metrics_host(const ek_hgr* h, const uint8_t* side /* nodes */, int64_t out[4]);

/* ------------------------------------------------------------------ */
/* Clique expansions (host, no GPU)                                     */
/* ------------------------------------------------------------------ */
typedef struct ek_csr ek_csr;

/* fp64 clique Laplacian, -2/|e| per pin pair, diagonal = -(row sum); rows
 * with ascending columns, diagonal included.  Replaces initializeMatrix,
 * cEIG.cpp:86-133. */
int ek_laplacian_build(const ek_hgr* h, ek_csr** out);
/* Rows [row0, row0+nrows) only (global column ids): one rank's shard of the
 * sharded Lanczos, as ek_shard_rows assigns it. */
int ek_laplacian_build_rows(const ek_hgr* h, int64_t row0, int64_t nrows, ek_csr** out);
/* The net-weighted clique Laplacian: ek_laplacian_build[_rows]
 * with one replacement — a net e of k = |e| >= 2 pins (repeated pins counted)
 * gives each ordered pin pair the fp64 value -(double(2 c(e)) / double(k)),
 * c(e) = h's net weight (1 where h carries none), in place of -(2.0 / k).
 * 2 c(e) <= 2^32 is exact, so the value is one correctly rounded division;
 * with c(e) = 1 it is the unweighted value bit for bit, and on an h without
 * net weights these return the arrays of ek_laplacian_build[_rows].  Order of
 * the sums, diagonal, isolated rows: as there.  Node weights do not enter.
 * No reference counterpart. */
int ek_laplacian_build_w(const ek_hgr* h, ek_csr** out);
int ek_laplacian_build_rows_w(const ek_hgr* h, int64_t row0, int64_t nrows, ek_csr** out);
/* fp32 KL adjacency, w = 1/(|e|-1) accumulated in net order; each row holds
 * its forward (upper-triangle) entries in the iteration order of cKL's
 * std::unordered_map<uint32_t,float> (libstdc++ _Hashtable, emulated), then
 * its backward entries by ascending id — the exact summation order of
 * connections(), cKL.cpp:225-251.  Replaces InitializeSparsMatrix,
 * cKL.cpp:84-149. */
int ek_kl_graph_build(const ek_hgr* h, ek_csr** out);
/* nrows, nnz, value size in bytes (8 = fp64 Laplacian, 4 = fp32 KL graph). */
int ek_csr_dims(const ek_csr* c, int64_t* nrows, int64_t* nnz, int32_t* value_bytes);
/* Copy out: rowptr[nrows+1], col[nnz], val[nnz] (double* or float*),
 * nfwd[nrows] (KL graph: forward entries per row; may be NULL). */
int ek_csr_copy(const ek_csr* c, int32_t* rowptr, int32_t* col, void* val, int32_t* nfwd);
void ek_csr_free(ek_csr* c);

/* 1-D row-block partition for the sharded Lanczos: rank r owns
 * rows [row0, row0+nrows) with nrows <= nloc (equal padded blocks). */
int ek_shard_rows(int64_t n, int nranks, int rank, int64_t* row0, int64_t* nrows, int64_t* nloc);
/* The nnz-balanced partition (SURVEY §8e "1-D row block partition balanced
 * by nnz"), the one ek_spmv_setup_pins uses: rank r owns rows
 * [row_offsets[r], row_offsets[r+1]) (nranks + 1 offsets), cut where the
 * prefix of the Laplacian rows' entries (1 + sum over the row's nets of
 * |e| - 1: initializeMatrix's triplets, cEIG.cpp:86-133) reaches r/nranks of
 * the total.  Deterministic: every rank computes the same map.  No reference
 * counterpart (the reference has no multi-GPU path). */
int ek_shard_map(int64_t n, int64_t nets, const int64_t* net_ptr, const int32_t* pins, int nranks,
                 int64_t* row_offsets);

/* ------------------------------------------------------------------ */
/* GPU context                                                          */
/* ------------------------------------------------------------------ */
typedef struct ek_ctx ek_ctx;

int ek_init(int device, ek_ctx** out);
void ek_destroy(ek_ctx* ctx);
/* The context's hipStream_t (every kernel of this context runs on it). */
int ek_get_stream(ek_ctx* ctx, void** stream_out);
/* Wait for everything queued on the context's stream. */
int ek_synchronize(ek_ctx* ctx);
int ek_device_count(int* count);

/* RCCL over xGMI: one process per GPU.  Rank 0 calls ek_comm_unique_id and
 * ships the 128 bytes to the other ranks (e.g. torch.distributed broadcast). */
int ek_comm_unique_id(void* id128);
/* Resets the context's row ownership: call ek_spmv_setup afterwards. */
int ek_comm_init(ek_ctx* ctx, int nranks, int rank, const void* id128);
/* Host-staged exchange instead of RCCL (no reference counterpart; the
 * reference has no multi-GPU path).  Every collective of the sharded Lanczos
 * drains the context stream, copies its operand to pinned host memory, calls
 * the caller's collective and copies the result back.  Lets several ranks
 * share one GPU (RCCL refuses that) and lets any host transport (e.g.
 * torch.distributed gloo) drive the exchange: the multi-rank tests and
 * debugging.  RCCL (ek_comm_init) is the production path.  Callbacks return
 * 0 on success; recv holds nranks*count doubles, rank-major. */
typedef int (*ek_allgather_fn)(void* user, const double* send, int64_t count, double* recv);
typedef int (*ek_allreduce_fn)(void* user, double* buf, int64_t count); /* in-place sum */
int ek_comm_init_host(ek_ctx* ctx, int nranks, int rank, ek_allgather_fn allgather, ek_allreduce_fn allreduce,
                      void* user);

/* ------------------------------------------------------------------ */
/* SpMV seam: Spectra SparseSymMatProd<double>::perform_op, cEIG.cpp:194  */
/* ------------------------------------------------------------------ */
/* Upload the Laplacian rows this context owns.  n = global size; rowptr has
 * nrows+1 entries starting at 0; col holds global column ids.  Host arrays
 * are copied; the caller keeps ownership.  Sharded contexts: every rank
 * calls it; the ranks' [row0, row0+nrows) must tile [0, n) in rank order
 * (learned with one all-gather; ek_shard_map or ek_shard_rows).  A rank
 * may own no rows (nrows 0, rowptr = {0}): it takes part in every
 * collective, and ek_spmv / ek_lanczos_fiedler give it what they give the
 * other ranks (an empty y; the same pair). */
int ek_spmv_setup(ek_ctx* ctx, int64_t n, int64_t row0, int64_t nrows, const int32_t* rowptr,
                  const int32_t* col, const double* val);
/* The same rows built on the GPU straight from the hypergraph's pins (net e
 * owns pins[net_ptr[e] .. net_ptr[e+1]), 0-based): the clique Laplacian of
 * initializeMatrix (cEIG.cpp:86-133) assembled by device kernels into the
 * SpMV's coded form, the rows of this context's shard only (ek_shard_map).
 * The values and the row blocks are the host build's (ek_laplacian_build),
 * so every SpMV and Lanczos result is bit-identical to ek_spmv_setup on
 * those rows.  Falls back to the host build for a row too long for the
 * device sort (or with EK_HOST_LAPLACIAN set); *on_device (may be NULL)
 * tells which ran. */
int ek_spmv_setup_pins(ek_ctx* ctx, int64_t n, int64_t nets, const int64_t* net_ptr, const int32_t* pins,
                       int32_t* on_device);
/* ek_spmv_setup_pins for the net-weighted Laplacian of ek_laplacian_build_w:
 * net_w holds nets values >= 1 (EK_EINVAL otherwise); NULL stands for all
 * ones and is ek_spmv_setup_pins exactly.  Bit-identical to ek_spmv_setup on
 * the rows of ek_laplacian_build_rows_w; every fallback (a row past the
 * device sort, EK_HOST_LAPLACIAN, EK_SPMV_PLAIN, a value set that outgrows
 * the dictionary -> plain CSR) carries the weights.  The shard map of a
 * multi-rank context stays ek_shard_map's: structural, the same on every
 * rank. */
int ek_spmv_setup_pins_w(ek_ctx* ctx, int64_t n, int64_t nets, const int64_t* net_ptr, const int32_t* pins,
                         const int32_t* net_w /* nets values >= 1; NULL: all ones */, int32_t* on_device);
/* The rows the context owns after the last ek_spmv_setup (any of the
 * pointers may be NULL). */
int ek_spmv_dims(ek_ctx* ctx, int64_t* n, int64_t* row0, int64_t* nrows);
/* y[0:nrows] = L[row0:row0+nrows, :] x.  x_dev: n doubles, y_dev: nrows
 * doubles, device pointers borrowed.  stream = hipStream_t or NULL (ctx
 * stream).  Asynchronous. */
int ek_spmv(ek_ctx* ctx, const double* x_dev, double* y_dev, void* stream);
/* Same with host buffers (x: n, y: nrows); synchronous. */
int ek_spmv_host(ek_ctx* ctx, const double* x, double* y);
/* Algorithmic (compulsory) bytes of one ek_spmv over the owned rows, SURVEY
 * §8d: 12*nnz (col+val) + 4*(nrows+1) (rowptr) + 8*n (x read once) +
 * 8*nrows (y).  Single GPU: 12 nnz + 4(n+1) + 16 n. */
int64_t ek_spmv_bytes(ek_ctx* ctx);
/* Storage form the SpMV reads (no reference counterpart; the reference keeps
 * an Eigen CSC of fp64 values, cEIG.cpp:49-50).  *packed = 1 when the entries
 * are dictionary-coded 32-bit words (column | code of the exact fp64 value in
 * a per-matrix table; bit-identical products), 0 for plain CSR (int32 col +
 * fp64 val; chosen when the distinct values overflow the code bits, or with
 * EK_SPMV_PLAIN=1 at setup).  *stored_bytes = bytes of one launch as stored:
 * entries + table + rowptr + 8*n (x) + 8*nrows (y).  Either pointer may be
 * NULL. */
int ek_spmv_format(ek_ctx* ctx, int32_t* packed, int64_t* stored_bytes);
/* The sharded step's exchange of f as set up: *halo = 1 when each rank
 * receives only the rows its columns read (point-to-point messages in one
 * RCCL group), 0 for the all-gather of whole slots; the doubles this rank
 * receives and sends per Lanczos step (each message carries the sender's
 * ||f||^2 partial).  A single context: 0, 0, 0.  No reference counterpart
 * (the reference has no sharded path). */
int ek_spmv_exchange(ek_ctx* ctx, int32_t* halo, int64_t* recv_doubles, int64_t* send_doubles);
/* The sharded Lanczos solves' exchange accounting since the last
 * ek_spmv_setup: exchanges of f (one per Lanczos step) and the point-to-point
 * messages this rank posted (halo form: ONE send and ONE receive per peer per
 * exchange, each message the rows the receiver reads closed by the sender's
 * ||f||^2 partial; host-staged: its pieces of the one all-gather).  With
 * ek_lanczos_opts::time_spmv set on a solve, that solve's collectives are
 * also timed: *exchange_ms over *exchanges_timed exchanges of f (RCCL: HIP
 * events around the send/recv group or all-gather on its stream, waits for
 * the peers included; host-staged: the host's view of the callback round
 * trip) and *allreduce_ms over *allreduces_timed all-reduces.  The timings
 * are reset by ek_spmv_setup and by a timed solve.  Any pointer may be NULL.
 * No reference counterpart (the reference has no sharded path). */
int ek_comm_stats(ek_ctx* ctx, int64_t* exchanges, int64_t* sends, int64_t* recvs, double* exchange_ms,
                  int64_t* exchanges_timed, double* allreduce_ms, int64_t* allreduces_timed);
/* Back-to-back SpMV launches on context-owned buffers, timed with HIP events
 * around the batch: *avg_us = average per launch (a sharded context: this
 * rank's rows over the all-gather layout, no collective).  fused = 2: also the
 * solve's folded finalize and ||w||^2 partials (the SpMV as the Lanczos step
 * launches it).  fused = 1 times the
 * Lanczos form (y scaled by 1/||x||, basis column + alpha partials written:
 * + 16*nrows bytes over ek_spmv_bytes).  Measurement helper for bench.py's
 * size sweep; no reference counterpart. */
int ek_spmv_bench(ek_ctx* ctx, int iters, int fused, double* avg_us);
/* The gather-only ceiling of the context's SpMV (a roofline
 * fraction read against its access pattern's own limit): back-to-back
 * launches of a kernel with the SpMV's grid that streams the same matrix words
 * (segments or column panels) and makes the same x and value-table gathers in
 * the same order, summing the products in registers: no row reduction, no y,
 * no epilogue.  *avg_us as in ek_spmv_bench.  No reference counterpart. */
int ek_spmv_gather_bench(ek_ctx* ctx, int iters, double* avg_us);

/* ------------------------------------------------------------------ */
/* Lanczos / Fiedler: Spectra SymEigsSolver(op, 2, min(100,n/2)),        */
/* compute(SmallestAlge), cEIG.cpp:194-207                               */
/* ------------------------------------------------------------------ */
typedef struct {
    int32_t ncv;        /* <= 0: min(80, n/2) under partial reorthogonalisation
                           (reorth 3, the default) below 1M rows, else
                           min(100, n/2) (cEIG.cpp:195) */
    int32_t maxit;      /* restarts; <= 0: 1000 (Spectra default) */
    double tol;         /* <= 0: 1e-10 (Spectra default) */
    int32_t deflate;    /* 1 (default): deflate the constant null vector, nev=1;
                           0: Spectra-equivalent nev=2, Fiedler = 2nd smallest */
    int32_t time_spmv;  /* 1: bracket every SpMV launch with HIP events (stats) */
    int32_t reorth;     /* 3 (default): partial reorthogonalisation — the three-term
                           recurrence, and the full classical Gram-Schmidt pass of 1
                           only on the steps Simon's omega recurrence asks for (loss of
                           orthogonality estimate > reorth_thresh), the step after each,
                           every cycle's first and last step (single context and
                           sharded alike; the sharded step all-reduces alpha and
                           ||w||^2 first).  CHANGED DEFAULT (EIGKL_ABI_VERSION 4): rounds 1-3
                           defaulted to 1.  1: that pass on every step (Spectra's
                           full reorthogonalisation, the reference's algorithm;
                           `--spectra` / `--reorth full` on the CLI); 2: CGS2 (twice)
                           from the matvec; 0: as 1 */
    int32_t check_every; /* after the first restart cycle, test Spectra's convergence
                            criterion on the projected matrix every this many steps
                            (and stop there) instead of at cycle ends only; 0: cycle
                            ends only (Spectra's schedule).  Default 8. */
    int32_t basis32;     /* 1 (default): the reorthogonalisation's update f = f' - V h reads
                            an fp32 shadow of the basis when sum|h| <= 2^-29 ||f'|| (its
                            effect then stays below fp64 rounding), else V;
                            0: always the fp64 basis.  Single-context steps only. */
    int32_t alpha_last;  /* 0 (default): every projection workgroup re-reduces the SpMV's
                            alpha = v_i . w partials; 1: the SpMV's last workgroup does
                            (a serial tail on the SpMV; the same bits) */
    int32_t keep_min;    /* implicit restarts keep at least this many vectors (floor on
                            Spectra's nev_adjusted, which on these Laplacians often keeps
                            2-4: DESIGN.md); < 0 (default): ncv / 5; 0: Spectra's rule */
    double reorth_thresh; /* reorth 3: project when the estimated |v_{i+1}^T v_j| exceeds
                             this; <= 0 (default): 1e-10 (Simon's
                             sqrt(DBL_EPSILON) lets the loss compound across implicit
                             restarts) */
} ek_lanczos_opts;

typedef struct {
    int32_t restarts;
    int32_t matvecs;
    int32_t converged;
    double residual;      /* ||L v - lambda v||_2 of the returned vector */
    double total_ms;      /* wall time of the solve */
    double spmv_ms;       /* sum of SpMV launch durations (time_spmv=1) */
    int32_t spmv_timed;   /* SpMV launches timed */
    double comm_ms;       /* time inside RCCL calls (host-observed, sharded) */
    int32_t allgathers;   /* collectives issued by this rank during the solve (sharded; */
    int32_t allreduces;   /* one of each per Lanczos step, plus restarts/injections/end) */
    int32_t update32_steps;     /* steps whose update was enqueued with the fp32 shadow */
    int32_t update32_fallbacks; /* ... of which took the fp64 basis (the accuracy test failed) */
    int32_t projected_steps;    /* steps that ran the Gram-Schmidt pass (= matvecs unless reorth 3) */
    int32_t reprojected;        /* sharded steps whose f' cancelled (||f'||^2 < 2^-20 ||w||^2) and
                                   whose next vector was projected again (a second CGS pass) */
    double ortho_max;           /* EK_LANCZOS_ORTHO=1: max |[V u0]^T [V u0] - I| at the restarts */
} ek_lanczos_stats;

void ek_lanczos_default_opts(ek_lanczos_opts* o);
/* Fiedler pair of the Laplacian given to ek_spmv_setup.  v_host_out: n
 * doubles (full vector on every rank when sharded).  Sign: the entry of
 * largest magnitude is made positive (cKL bit parity for odd n
 * may need ek_align_sign against the reference file). */
int ek_lanczos_fiedler(ek_ctx* ctx, const ek_lanczos_opts* o, double* lambda_out, double* v_host_out,
                       ek_lanczos_stats* stats);

/* ------------------------------------------------------------------ */
/* Median split + EIG file (cEIG.cpp:55-65, 209-220)                    */
/* ------------------------------------------------------------------ */
/* median (even n: mean of the two middle values), bits[i] = (median > v[i]). */
int ek_median_split(int64_t n, const double* v, double* median_out, uint8_t* bits_out);
/* Flip v if its dot product with ref is negative (--sign-ref). */
int ek_align_sign(int64_t n, double* v, const double* ref);
/* pre_saved_EIG/<base>_out.txt writer / reader (%.12g; cEIG.cpp:213-220,
 * read as cKL.cpp:155-174).  The reader returns remain[] lists in file order. */
int ek_eig_write(const char* path, int64_t n, double lambda, double median, const uint8_t* bits,
                 const double* v);
int ek_eig_read(const char* path, int64_t n, double* lambda, double* median, uint8_t* bits, double* v,
                int32_t* order0, int64_t* n0, int32_t* order1, int64_t* n1);

/* ------------------------------------------------------------------ */
/* KL: KL() cKL.cpp:288-406; GPU gain seam gpuConnections gKL.cu:188-227 */
/* ------------------------------------------------------------------ */
typedef struct {
    uint32_t iter;       /* 1-based (cKL.cpp:371) */
    uint32_t node_left;  /* node1: argmax gain over remain[0] (cKL.cpp:341-347) */
    uint32_t node_right; /* node2: argmin gain over remain[1] (cKL.cpp:349-355) */
    float max_gain, min_gain;
    float gain;          /* maxGain - minGain - 2 w(node1,node2) (cKL.cpp:360) */
    float cut;           /* running fp32 cut (cKL.cpp:362) */
    uint32_t pad;
} ek_swap;

typedef struct {
    int64_t iterations;
    float initial_cut, best_cut, final_cut;
    int64_t best_iter;   /* first iteration reaching best_cut (0 = initial) */
    int64_t net_cut_initial, net_cut_best, net_cut_final; /* integer hyperedge cuts */
    double loop_ms;      /* device time of the swap loop */
    double total_ms;     /* device time of gain scan + loop + cuts */
} ek_kl_result;

/* Upload the KL graph (from ek_kl_graph_build, or any rows in cKL order). */
int ek_kl_graph_setup(ek_ctx* ctx, int64_t n, const int32_t* rowptr, const int32_t* col, const float* w);
/* Upload the hypergraph pins (for the integer net cut). */
int ek_kl_nets_setup(ek_ctx* ctx, int64_t nets, const int64_t* net_ptr, const int32_t* pins);
/* Initial remain[] lists (shuffleSparceMatrix, cKL.cpp:151-197): positions
 * are list order; the sides are split[0] = order0, split[1] = order1. */
int ek_kl_set_partition(ek_ctx* ctx, const int32_t* order0, int64_t n0, const int32_t* order1, int64_t n1);
/* The random branch of shuffleSparceMatrix (cKL.cpp:176-192), host only:
 * nodes 0..n-1 shuffled by std::shuffle with std::mt19937(seed) (the
 * reference seeds it from std::random_device; the seed makes it
 * reproducible), the first n/2 to remain[0] (order0, n/2 entries), the rest
 * to remain[1] (order1, n - n/2 entries). */
int ek_random_split(int64_t n, uint32_t seed, int32_t* order0, int32_t* order1);
/* The -EIG branch of shuffleSparceMatrix (cKL.cpp:155-174): node i goes to
 * split[bits[i]] in ascending node order (the EIG file's line order). */
int ek_kl_set_partition_bits(ek_ctx* ctx, int64_t n, const uint8_t* bits);
/* The -EIG branch of ek_solve_file on the device: the median split of the
 * Fiedler vector the last ek_lanczos_fiedler on this context returned (kept
 * on the device, normalised and sign-fixed as v_out), with the remain[]
 * lists in node order — the lists ek_median_split + ek_kl_set_partition_bits
 * give on the host (cEIG.cpp:204-209 median, cKL.cpp:155-174 lists), without
 * the vector's round trip.  median_out, n0_out, n1_out may be null. */
int ek_kl_set_partition_fiedler(ek_ctx* ctx, double* median_out, int64_t* n0_out, int64_t* n1_out);
/* Uploads v_host (n doubles) as the context's Fiedler vector: exactly the
 * state a successful ek_lanczos_fiedler leaves for ek_kl_set_partition_fiedler
 * and its _rank / _sweep kin.  The test seam of the device splits: it drives
 * them with a chosen vector.  EK_EINVAL for n < 1, n > INT32_MAX - 1, a null
 * pointer or any NaN in v_host (a NaN has no place in the select's order, and
 * a solve never leaves one; infinities and signed zeros are ordered and
 * accepted).  EK_ESTATE on a multi-rank context.  No reference counterpart. */
int ek_fiedler_set(ek_ctx* ctx, int64_t n, const double* v_host);
/* Copies back what the last ek_kl_set_partition* call left on the device: the
 * remain[] lists (order0: n0 node ids, order1: n1), plist (node i's position
 * in its list, bit 31 set on side 1) and the initial sides (n bytes).  The
 * swap loop never rewrites them, so a later ek_kl_run changes nothing here.
 * Any pointer may be null.  EK_ESTATE when no partition is set.
 * No reference counterpart. */
int ek_kl_partition_copy(ek_ctx* ctx, int32_t* order0_out /* n0 */, int32_t* order1_out /* n1 */,
                         uint32_t* plist_out /* n */, uint8_t* side_out /* n */, int64_t* n0_out, int64_t* n1_out);
/* Run the swap loop to termination on the device (one persistent
 * workgroup; no host round trip per iteration).  limit < 0: floor(log2 n)+5
 * (cKL.cpp:303).  log_out may be NULL. */
int ek_kl_run(ek_ctx* ctx, int32_t limit, ek_swap* log_out, int64_t cap, ek_kl_result* res);
/* Side of every node: which = 0 initial, 1 best prefix, 2 final. */
int ek_kl_sides(ek_ctx* ctx, int32_t which, uint8_t* sides_out);

/* ------------------------------------------------------------------ */
/* Whole path, .hgr in -> results/ out, in-process: the body of          */
/* gKL2 <in> -EIG (GPU Fiedler split) and cKL/gKL <in> (random split),   */
/* main() + KL() of cKL.cpp:288-468 with cEIG.cpp:138-237 in front.      */
/* ------------------------------------------------------------------ */
typedef struct {
    int32_t eig;          /* 1: Fiedler split on the GPU (gKL2 -EIG); 0: random split (seed) */
    uint32_t seed;        /* random split: std::mt19937 seed (ek_random_split) */
    int32_t write_results;/* 1: results/<base>_KL_CutSize[_EIG]_output.txt under out_dir */
    int32_t limit;        /* KL termination limit; < 0: floor(log2 n)+5 (cKL.cpp:303) */
    const char* out_dir;  /* NULL: the CWD (the reference's convention) */
    const char* sign_ref; /* optional pre_saved_EIG file whose sign the Fiedler vector takes */
    ek_lanczos_opts lanczos;
} ek_solve_opts;

typedef struct {
    int64_t nets, nodes, pins;
    double lambda, median;
    ek_lanczos_stats lanczos; /* eig = 1 */
    ek_kl_result kl;          /* rank 0 only */
    /* wall seconds of the phases on this rank (host clock); t_lanczos
     * includes t_spmv_setup (the rows' coding and upload) */
    double t_read, t_laplacian, t_lanczos, t_split, t_kl_graph_wait, t_kl_setup, t_kl, t_write, t_total;
    double t_spmv_setup;
} ek_solve_result;

void ek_solve_default_opts(ek_solve_opts* o);
/* Multi-rank contexts (ek_comm_init*): every rank calls it with the same
 * file; the Lanczos rows are sharded (each rank builds and uploads its own
 * rows), the KL loop and the results file are rank 0's.  log_out (may be
 * NULL, cap entries) receives rank 0's swap log. */
int ek_solve_file(ek_ctx* ctx, const char* path, const ek_solve_opts* o, ek_swap* log_out, int64_t cap,
                  ek_solve_result* res);

/* ------------------------------------------------------------------ */
/* k-way partitioning by recursive spectral bisection.  No reference     */
/* counterpart anywhere in this section: the reference stops at two      */
/* sides (cKL.cpp:151-197 splits once).                                  */
/* ------------------------------------------------------------------ */
/* The part sizes the recursion produces (host only).  A block of n' nodes
 * that must become k' parts splits into side 0 with kL = ceil(k'/2) parts
 * (ids [base, base+kL)) and side 1 with kR = floor(k'/2) parts (ids
 * [base+kL, base+k')); side 1 gets n1 = floor(n' kR / k') nodes, side 0 the
 * other n0 = n' - n1.  By induction every final part holds floor(n/k) or
 * ceil(n/k) nodes: if floor(n'/k') <= n'/k' <= ceil(n'/k') then n1/kR =
 * floor(n' kR/k')/kR lies in [floor(n'/k'), n'/k'] and n0/kL = ceil(n'
 * kL/k')/kL in [n'/k', ceil(n'/k')], so both sides keep the same floor and
 * ceiling as bounds of their own mean.  EK_EINVAL unless 2 <= k <= 256 and
 * n >= 2k.  No reference counterpart. */
int ek_kway_plan(int64_t n, int32_t k, int64_t* part_sizes /* k */);
/* bits[i] = 1 for exactly the n1 nodes smallest in the key (ord(v[i]), i):
 * ord is the order of the device's radix select (the fp64 bit patterns as a
 * radix sort orders them: -0 before +0), ties broken by ascending node id.
 * The orientation is ek_median_split's (median > v[i] gives bit 1).
 * 0 <= n1 <= n.  No reference counterpart. */
int ek_rank_split(int64_t n, const double* v, int64_t n1, uint8_t* bits_out);
/* The sub-hypergraph on the nodes with keep[i] != 0, renumbered in ascending
 * original id: every net restricted to its kept pins (so the clique weights
 * of the sub-hypergraph use the restricted size: net splitting), nets left
 * with fewer than 2 pins dropped, surviving nets in file order, pins in
 * their original order.  node_map (nodes of h, may be NULL) gets the new id
 * or -1, as ek_hgr_largest_component's.  EK_EINVAL when nothing is kept.
 * No reference counterpart. */
int ek_hgr_induce(const ek_hgr* h, const uint8_t* keep /* nodes */, ek_hgr** out, int32_t* node_map);
/* Exact k-way quality of part[] (a part id in [0, k) per node, k <= 256),
 * with lambda_e the number of distinct parts among net e's pins:
 * out[0] = cut nets (lambda_e >= 2), out[1] = connectivity, the sum of
 * (lambda_e - 1), out[2] = SOED, the sum of lambda_e over the cut nets.
 * Host only.  No reference counterpart. */
int ek_kway_metrics_host(int64_t nets, const int64_t* net_ptr, const int32_t* pins, const int32_t* part, int32_t k,
                         int64_t out[3]);
/* ek_rank_split run by the device kernels on an uploaded copy of v_host (the
 * radix select for the key at rank n1 - 1, a count of the keys below it, the
 * equal keys taken in id order): the same bits.  The test seam of those
 * kernels; needs no other setup on the context.  No reference counterpart. */
int ek_rank_split_device(ek_ctx* ctx, int64_t n, const double* v_host, int64_t n1, uint8_t* bits_out);
/* ek_kl_set_partition_fiedler with the rank split instead of the median
 * split: side 1 (remain[1]) gets the n1 nodes ek_rank_split marks in the
 * Fiedler vector the last ek_lanczos_fiedler left on the device, the lists in
 * node order, no host round trip.  1 <= n1 < n.  n0_out / n1_out may be NULL.
 * No reference counterpart. */
int ek_kl_set_partition_fiedler_rank(ek_ctx* ctx, int64_t n1, int64_t* n0_out, int64_t* n1_out);
/* ek_kway_metrics_host on the GPU (part_host is read up to the largest pin).
 * No reference counterpart. */
int ek_kway_metrics(ek_ctx* ctx, int64_t nets, const int64_t* net_ptr, const int32_t* pins,
                    const int32_t* part_host, int32_t k, int64_t out[3]);

typedef struct {
    int32_t k;            /* number of parts, 2..256 */
    int32_t min_spectral; /* blocks with fewer nodes are split by node index, not spectrally; default 32;
                           * values below 4 act as 4 (6 with lanczos.deflate = 0): the smallest block
                           * ek_lanczos_fiedler accepts */
    int32_t limit;        /* KL termination limit of every bisection, as ek_solve_opts::limit */
    int32_t write_results;/* ek_partition_kway_file: 1 writes results/<base>.part.<k> under out_dir */
    const char* out_dir;  /* NULL: the CWD */
    ek_lanczos_opts lanczos; /* for every bisection */
} ek_kway_opts;

#define EK_KWAY_LEVELS 8 /* depth of the recursion at k = 256 */
typedef struct {
    int32_t k;
    int32_t bisections;      /* k - 1 */
    int32_t fallback_splits; /* bisections split by node index (small block, no nets, or EK_ENOCONV) */
    int32_t pad;
    int64_t part_min, part_max;           /* smallest / largest part, in nodes */
    int64_t cut_nets, connectivity, soed; /* ek_kway_metrics of part_out */
    int64_t matvecs, kl_swaps;            /* totals over the bisections */
    /* wall seconds (host clock): the sub-hypergraphs, Laplacian build +
     * Lanczos, KL (adjacency wait, split, loop, sides), the metrics, all */
    double t_induce, t_lanczos, t_kl, t_metrics, t_total;
    double t_level[EK_KWAY_LEVELS]; /* per recursion level (root = 0), its blocks' induce + bisections */
} ek_kway_result;

void ek_kway_default_opts(ek_kway_opts* o);
/* k-way partition of h by recursive bisection on this context, depth first,
 * side 0 before side 1, one bisection at a time: the induced sub-hypergraph
 * (ek_hgr_induce), its Laplacian built on the device (ek_spmv_setup_pins),
 * the Fiedler vector (ek_lanczos_fiedler), the rank split at the block's
 * ek_kway_plan size, then the KL loop on the block (ek_kl_run, best prefix).
 * KL swaps pairs, so the planned sizes are exact in part_out (one id in
 * [0, k) per node of h).  A block below min_spectral nodes (or below the 4
 * nodes, 6 undeflated, that ek_lanczos_fiedler needs), one with no net
 * of >= 2 pins, or one whose Lanczos returns EK_ENOCONV is split by node
 * index instead (its first n0 nodes to side 0; KL still runs when the block
 * has nets); any other error ends the call.  EK_ESTATE on a multi-rank
 * context (ek_comm_init* with nranks > 1).  result may be NULL.
 * No reference counterpart. */
int ek_partition_kway(ek_ctx* ctx, const ek_hgr* h, const ek_kway_opts* opts, int32_t* part_out /* nodes */,
                      ek_kway_result* result);
/* The same from a .hgr file; part_out may be NULL.  With write_results:
 * results/<base>.part.<k> under out_dir, one part id per line in node order
 * (the hMETIS partition-file convention).  No reference counterpart. */
int ek_partition_kway_file(ek_ctx* ctx, const char* path, const ek_kway_opts* opts, int32_t* part_out,
                           ek_kway_result* result);

/* ------------------------------------------------------------------ */
/* k-way connectivity refinement under a maximum part size.  No          */
/* reference counterpart (the reference stops at two sides).             */
/* ------------------------------------------------------------------ */
/* A deterministic, synchronous, integer-only refinement of the connectivity
 * sum(lambda_e - 1) of a part vector.  Only nets with at
 * least 2 distinct pins take part; a node repeated inside a net counts once.
 * L_max = floor((1 + imbalance) ceil(n / k)); a part receives nodes only
 * while it is below L_max, and there is no lower bound on a part's size.  One
 * round, all of it read from the state at the round's start: every node takes
 * as target the part b (below L_max, not its own) of greatest gain g = r + c_b
 * - deg (r: its nets in which it is its part's only pin; c_b: its nets with a
 * pin in b), ties to the smaller b, and is a candidate when g > 0; the winner
 * of a net is its candidate pin of greatest g, ties to the smaller id; a
 * candidate that wins every net it is on is independent; per target part the
 * independent candidates in (g descending, id ascending) order are accepted
 * while the part has room.  Accepted nodes share no net, so the connectivity
 * falls by exactly the sum of their g.  Rounds repeat until one accepts
 * nothing (that round is not counted) or max_rounds rounds have moved. */
typedef struct {
    int32_t k;          /* number of parts, 2..256 */
    int32_t max_rounds; /* <= 0: until a round accepts nothing */
    double imbalance;   /* epsilon >= 0; default 0.03 */
} ek_kway_refine_opts;

typedef struct {
    int32_t k;
    int32_t rounds;             /* rounds that moved at least one node */
    int64_t moves;              /* accepted moves over all rounds */
    int64_t gain_total;         /* sum of the rounds' gains = connectivity_before - connectivity */
    int64_t max_part;           /* L_max */
    int64_t part_min, part_max; /* smallest / largest part after the run, in nodes */
    int64_t connectivity_before;
    int64_t cut_nets, connectivity, soed; /* ek_kway_metrics of the refined vector */
    double t_setup, t_rounds, t_metrics;  /* wall seconds (host clock) */
} ek_kway_refine_result;

void ek_kway_refine_default_opts(ek_kway_refine_opts* o);
/* The refinement on the host (no GPU): the checker of ek_kway_refine, written
 * from the rule.  part_inout: one id in [0, k) per node of h, refined in
 * place.  round_log (may be NULL) receives four values per round, for the
 * first log_rounds rounds: candidates, independent candidates, accepted
 * moves, the round's gain.  EK_EINVAL for k outside 2..256, a part id outside
 * [0, k), imbalance < 0 or not finite.  A part already above L_max is not an
 * error: it never receives. */
int ek_kway_refine_host(const ek_hgr* h, const ek_kway_refine_opts* opts, int32_t* part_inout, int64_t* round_log,
                        int64_t log_rounds, ek_kway_refine_result* result);
/* The same on the GPU: the same part vector, round log and result integers.
 * The host reads one 8-byte counter per round.  EK_ESTATE on a multi-rank
 * context.  Keeps nothing on the context: any other call may follow. */
int ek_kway_refine(ek_ctx* ctx, const ek_hgr* h, const ek_kway_refine_opts* opts, int32_t* part_inout,
                   int64_t* round_log, int64_t log_rounds, ek_kway_refine_result* result);

/* ------------------------------------------------------------------ */
/* Sweep cut of the Fiedler vector under a balance tolerance (Hagen-Kahng */
/* EIG1's split).  No reference counterpart anywhere in this section: the  */
/* reference splits at the median only (cEIG.cpp:204-209).                 */
/* ------------------------------------------------------------------ */
/* The rule, all integers, every tie broken by ids.  The n
 * nodes of h (2 <= n <= INT32_MAX - 1) are sorted ascending by the key
 * (ord(v[i]), i), ord as in ek_rank_split: order[r] is the node at rank r.
 * Split s (0 <= s <= n) puts the s nodes of rank below s on side 1: the bits
 * of ek_rank_split(v, s).  profile[s] = the nets with a pin on either side of
 * split s = #{e : lo_e < s <= hi_e}, lo_e / hi_e the least / greatest rank of
 * net e's pins (profile[0] = profile[n] = 0).  With L_max = floor((1 +
 * imbalance) ceil(n / 2)) the window is s_lo = max(1, n - L_max) .. s_hi =
 * min(n - 1, L_max); it always holds floor(n / 2).  The chosen s* is the
 * window's least under: objective 0 (minimum cut) the lexicographic order of
 * (profile[s], |2s - n|, s); objective 1 (ratio cut) a before b when
 * profile[a] b (n - b) < profile[b] a (n - a), compared exactly, equal ratios
 * by (|2s - n|, s).  Side 1 gets n1 = s* nodes, side 0 the other n0. */
typedef struct {
    int32_t objective; /* 0: minimum cut; 1: ratio cut c / (|A| |B|) */
    int32_t pad;
    double imbalance;  /* epsilon >= 0; default 0.03 */
} ek_sweep_opts;

typedef struct {
    int64_t n, n0, n1;     /* nodes; side 0 and side 1 of the chosen split (n1 = s*) */
    int64_t s_lo, s_hi;    /* the window */
    int64_t max_part;      /* L_max */
    int64_t cut;           /* profile[s*] */
    int64_t cut_mid;       /* profile[floor(n / 2)] */
    int64_t spanning_nets; /* nets with lo < hi */
    double t_sort, t_profile, t_select; /* wall seconds (host clock) */
} ek_sweep_result;

/* objective 0, imbalance 0.03.  No reference counterpart. */
void ek_sweep_default_opts(ek_sweep_opts* o);
/* The sweep cut on the host (no GPU): the checker of ek_sweep_cut, single
 * threaded and written from the rule.  v: n doubles (any bit patterns: ord is
 * a total order).  order_out (n) and profile_out (n + 1) may be NULL.
 * EK_EINVAL for n < 2, imbalance < 0 or not finite, an objective outside
 * {0, 1}.  No reference counterpart. */
int ek_sweep_cut_host(const ek_hgr* h, const double* v, const ek_sweep_opts* opts, int32_t* order_out,
                      int32_t* profile_out, ek_sweep_result* result);
/* The same on the GPU, on an uploaded copy of v_host: the same order, profile
 * and result integers.  The host reads back the result record, and order /
 * profile only when asked for them.  The test seam of the kernels, as
 * ek_rank_split_device is; every buffer is local to the call and the context
 * keeps nothing.  No reference counterpart. */
int ek_sweep_cut(ek_ctx* ctx, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts, int32_t* order_out,
                 int32_t* profile_out, ek_sweep_result* result);
/* The sweep cut of the Fiedler vector the last ek_lanczos_fiedler left on the
 * device, then ek_kl_set_partition_fiedler_rank(ctx, result.n1): the context
 * is in exactly the state that call leaves.  EK_ESTATE before
 * ek_kl_graph_setup, without a Fiedler vector of the KL graph's size, or on a
 * multi-rank context; EK_EINVAL when h's node count is not the KL graph's.
 * result may be NULL.  No reference counterpart. */
int ek_kl_set_partition_fiedler_sweep(ek_ctx* ctx, const ek_hgr* h, const ek_sweep_opts* opts,
                                      ek_sweep_result* result);

/* ------------------------------------------------------------------ */
/* The weighted sweep cut: net weights in the profile, node weights in  */
/* the window.  No reference counterpart.                               */
/* ------------------------------------------------------------------ */
/* The rule is the rule above with these replacements.  w(v)
 * is the node weight and c(e) the net weight of h (1 where h carries no such
 * array), W = sum of w(v).  The order, order[r] and the meaning of split s are
 * unchanged.
 * (a) Profile: profile_w[s] = the sum of c(e) over {e : lo_e < s <= hi_e},
 * int64, profile_w[0] = profile_w[n] = 0.  The count profile of the rule above
 * is kept beside it, only to report the cut nets at the chosen split.
 * (b) Prefix weight: P[s] = the sum of w(order[r]) over r < s, int64, P[0] = 0
 * and P[n] = W.  Side 1 of split s weighs P[s], side 0 W - P[s].
 * (c) Window: L_max = floor((1 + imbalance) ceil(W / 2)), the bound of
 * ek_fm_refine_w.  Split s (1 <= s <= n - 1) is feasible iff P[s] <= L_max and
 * W - P[s] <= L_max.  P is non-decreasing, so the feasible splits are one
 * contiguous range s_lo..s_hi.  The range is certainly non-empty when max w(v)
 * <= 2 L_max - W + 1: the feasible values of P are the integers of [W - L_max,
 * L_max], 2 L_max - W + 1 >= 1 of them, and a walk from P[0] = 0 to P[n] = W
 * whose steps are no longer than that count cannot jump over them: the first s
 * with P[s] >= W - L_max has P[s] <= (W - L_max - 1) + (2 L_max - W + 1) =
 * L_max; that s is neither 0 nor n unless L_max >= W, and then every split is
 * feasible.  The range can be empty, for example when one node is heavier than
 * L_max.
 * (d) Choice.  Window not empty: feasible = 1 and s* is the window's least
 * split under (profile_w[s], |2 P[s] - W|, s).  Window empty: feasible = 0,
 * s_lo = s_hi = 0, and s* is the least split of 1..n-1 under (|2 P[s] - W|,
 * profile_w[s], s), the closest the order comes to balance; this is not an
 * error, as a start above L_max is none for ek_fm_refine_w.  Nodes of weight 0
 * make P flat; the last key s keeps the order strict.
 * (e) No ratio objective: its exact comparison would need products of three
 * 62-bit numbers.  objective = 1 is EK_EINVAL in the weighted entries.
 * Ranges, each EK_EINVAL: 2 <= n <= 2^31 - 2; W and the sum of all c(e) at
 * most 2^62 (as for ek_fm_refine_w; int32 weights cannot in fact exceed it);
 * imbalance finite and >= 0.
 * With every weight 1, profile_w is the profile, P[s] = s, and the window and
 * the choice are those of the rule above (objective 0). */
typedef struct {
    int64_t n, n0, n1;        /* nodes; side 0 and side 1 of the chosen split (n1 = s*) */
    int64_t s_lo, s_hi;       /* the feasible splits (0, 0 when there is none) */
    int64_t feasible;         /* 1: the window is not empty */
    int64_t total_weight;     /* W */
    int64_t max_part;         /* L_max */
    int64_t w0, w1;           /* the sides' weights at s*: W - P[s*], P[s*] */
    int64_t cut;              /* profile_w[s*] */
    int64_t cut_nets;         /* the count profile at s* */
    int64_t cut_half;         /* profile_w[floor(n / 2)] */
    int64_t spanning_nets;    /* nets with lo < hi */
    double t_sort, t_profile, t_select; /* wall seconds (host clock) */
} ek_sweep_w_result;

/* The weighted sweep cut on the host (no GPU): the checker of ek_sweep_cut_w,
 * single threaded and written from the rule; it shares with the device path
 * only the argument checks and L_max.  ek_sweep_opts is reused (objective must
 * be 0).  order_out (n), profile_out (profile_w, n + 1 int64) and prefix_out
 * (P, n + 1 int64) may be NULL.  EK_EINVAL as listed above. */
int ek_sweep_cut_w_host(const ek_hgr* h, const double* v, const ek_sweep_opts* opts, int32_t* order_out,
                        int64_t* profile_out /* n + 1 */, int64_t* prefix_out /* n + 1 */, ek_sweep_w_result* result);
/* The same on the GPU, on an uploaded copy of v_host: the same order, profile,
 * prefix and result integers.  The host reads back the result record, and the
 * three arrays only when asked for them.  Every buffer is local to the call
 * and the context keeps nothing. */
int ek_sweep_cut_w(ek_ctx* ctx, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts, int32_t* order_out,
                   int64_t* profile_out /* n + 1 */, int64_t* prefix_out /* n + 1 */, ek_sweep_w_result* result);
/* The weighted sweep cut of the Fiedler vector the last ek_lanczos_fiedler left
 * on the device, then ek_kl_set_partition_fiedler_rank(ctx, result.n1): the
 * context is in exactly the state that call leaves.  EK_ESTATE and EK_EINVAL
 * as for ek_kl_set_partition_fiedler_sweep (and objective 1: EK_EINVAL).
 * result may be NULL. */
int ek_kl_set_partition_fiedler_sweep_w(ek_ctx* ctx, const ek_hgr* h, const ek_sweep_opts* opts,
                                        ek_sweep_w_result* result);

/* ------------------------------------------------------------------ */
/* Fiduccia-Mattheyses refinement of a bipartition on the integer net    */
/* cut, under a balance tolerance.  No reference counterpart anywhere in */
/* this section: the reference's only refinement is the KL swap loop.    */
/* ------------------------------------------------------------------ */
/* The rule, all integers, every tie broken by sizes or ids.
 * Only nets with at least 2 distinct pins take part; a node repeated inside a
 * net counts once.  deg(v): those nets on v; a node of deg 0 never moves.
 * cnt(e, s): the pins of e on side s; the cut is #{e : cnt(e, 0) > 0 and
 * cnt(e, 1) > 0}.  L_max = floor((1 + imbalance) ceil(n / 2)).  For v on side
 * a, g(v) = #{e on v : cnt(e, a) = 1} - #{e on v : cnt(e, 1 - a) = 0}, always
 * of the current state: moving v lowers the cut by exactly g(v).
 * One pass: (1) unlock every node; t = 0, c_0 = the cut, d_0 = |s_0 - s_1|
 * (s: the sides' node counts).  (2) Side a has a candidate iff s[1 - a] <
 * L_max and it holds an unlocked node of deg > 0: that side's unlocked node of
 * greatest g, ties to the smaller id.  Of two candidates the one of greater g
 * moves; equal g: the one whose side holds more nodes; equal sizes: the
 * smaller id.  No candidate ends the pass.  (3) The node moves and is locked:
 * t += 1, c_t = c_(t-1) - g, d_t = |s_0 - s_1|.  The best prefix t* is the
 * least t that minimises (c_t, d_t) lexicographically.  (4) With stall > 0 the
 * pass ends when t - t* >= stall.  (5) Moves t* + 1 .. t are undone.
 * A pass counts iff t* > 0.  The run ends with the first pass of t* = 0, or
 * after max_passes counted passes; (c, d) falls strictly with every counted
 * pass.  A side already above L_max is not an error: it never receives.  With
 * imbalance 0 and even n both sides are full when they are equal, and nothing
 * moves: an FM pass needs slack (an odd n has one node of it). */
typedef struct {
    double imbalance;   /* epsilon >= 0; default 0.03 */
    int32_t max_passes; /* <= 0: until a pass keeps nothing; default 0 */
    int32_t stall;      /* <= 0: a pass runs until no node can move; default 1000,
                         * a choice of the rule's parameter, not a measurement */
} ek_fm_opts;

typedef struct {
    int32_t node; /* the node moved */
    int32_t gain; /* its g when it moved */
    int64_t cut;  /* the cut after the move */
} ek_fm_move;

typedef struct {
    int64_t n, max_part;             /* nodes; L_max */
    int32_t passes, passes_run;      /* counted passes (t* > 0); passes run (at most one more) */
    int64_t moves_tried, moves_kept; /* sum of t and of t* over the passes run */
    int64_t cut_before, cut;         /* the net cut of the sides given and of the sides returned */
    int64_t n0, n1;                  /* the sides' node counts after the run */
    double t_setup, t_passes, t_metrics; /* wall seconds (host clock) */
} ek_fm_result;

/* imbalance 0.03, max_passes 0, stall 1000. */
void ek_fm_default_opts(ek_fm_opts* o);
/* The refinement on the host (no GPU): the checker of ek_fm_refine, single
 * threaded and written from the rule; after a move it recomputes the gains of
 * the pins of the moved node's nets from their definition.  side_inout: one
 * byte in {0, 1} per node of h, refined in place.  pass_log (may be NULL)
 * receives four values per pass run, the last uncounted one included, for the
 * first log_passes passes: moves tried, t*, the cut and |s_0 - s_1| after the
 * rollback.  move_log (may be NULL) receives every move tried, in order, over
 * all passes, the first move_cap of them.  EK_EINVAL for a side outside
 * {0, 1}, imbalance < 0 or not finite, more than INT32_MAX - 1 nodes. */
int ek_fm_refine_host(const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side_inout /* nodes */, int64_t* pass_log,
                      int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_result* result);
/* The same on the GPU: the same bytes in side_inout, pass_log and move_log and
 * the same result integers.  One persistent workgroup runs a pass in one
 * launch; the host reads one 32-byte record per pass, and the move log and
 * the sides once at the end.  EK_ESTATE on a multi-rank context.  Every
 * buffer is local to the call and the context keeps nothing: any other call
 * may follow. */
int ek_fm_refine(ek_ctx* ctx, const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side_inout /* nodes */,
                 int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_result* result);

/* ------------------------------------------------------------------ */
/* The weighted FM refinement: node weights under the balance bound, net */
/* weights in the cut.  No reference counterpart.                        */
/* ------------------------------------------------------------------ */
/* The rule is the rule above with four replacements.  w(v) is
 * the node weight and c(e) the net weight of h (1 where h carries no such
 * array), W = sum of w(v), S_0 and S_1 the sides' weights; the cut is the sum
 * of c(e) over the cut nets.
 * (a) Gain: g(v) = sum of c(e) over {e on v : cnt(e, a) = 1} - sum of c(e)
 * over {e on v : cnt(e, 1 - a) = 0}: moving v lowers the weighted cut by
 * exactly g(v).  (b) Bound: L_max = floor((1 + imbalance) ceil(W / 2)).
 * (c) Candidate: side a's top node is its unlocked node of deg > 0 of greatest
 * g, ties to the smaller id; it is side a's candidate iff S[1 - a] + w(top) <=
 * L_max.  Only the top node is tried: a top node that does not fit leaves its
 * side without a candidate until the state changes, even when a lighter node
 * of lower gain would fit (a choice of the rule: selection stays a pure
 * max-key reduction).  (d) Of two candidates the greater g moves; equal g:
 * the one from the heavier side (greater S_a); equal weights: the smaller id.
 * d_t = |S_0 - S_1|.  Everything else (the best prefix over (c_t, d_t), stall,
 * the rollback, counted passes, termination) is the unweighted rule word for
 * word, and with every weight 1 this is that rule exactly.
 * Ranges, each EK_EINVAL: the sum of c(e) over the participating nets on any
 * one node is at most 2^31 - 1 (gains are int32); W and the sum of all c(e)
 * are at most 2^62 (int64 with room to spare; int32 weights and counts cannot
 * in fact exceed it); sides, imbalance and node count as for ek_fm_refine. */
typedef struct {
    int64_t n, total_weight, max_part; /* nodes; W; L_max */
    int32_t passes, passes_run;        /* counted passes (t* > 0); passes run (at most one more) */
    int64_t moves_tried, moves_kept;   /* sum of t and of t* over the passes run */
    int64_t cut_before, cut;           /* the weighted cut of the sides given and of the sides returned */
    int64_t cut_nets_before, cut_nets; /* the cut nets of the same */
    int64_t w0, w1, n0, n1;            /* the sides' weights and node counts after the run */
    double t_setup, t_passes, t_metrics; /* wall seconds (host clock) */
} ek_fm_w_result;

/* The weighted refinement on the host (no GPU): the checker of ek_fm_refine_w,
 * single threaded and written from the rule, the gains of the pins of the
 * moved node's nets recomputed from their definition after every move.
 * Arguments as ek_fm_refine_host; ek_fm_opts and ek_fm_move are reused: a
 * move's gain is the weighted g, its cut the weighted cut, and a pass_log row
 * is moves tried, t*, the weighted cut and |S_0 - S_1| after the rollback. */
int ek_fm_refine_w_host(const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side_inout /* nodes */, int64_t* pass_log,
                        int64_t log_passes, ek_fm_move* move_log, int64_t move_cap, ek_fm_w_result* result);
/* The same on the GPU: the same bytes in side_inout, pass_log and move_log and
 * the same result integers.  The weighted instantiation of the unweighted
 * path's kernels (kernels_fm.hip); one record read per pass, the log and the
 * sides once at the end.  EK_ESTATE on a multi-rank context.  Every buffer is
 * local to the call and the context keeps nothing. */
int ek_fm_refine_w(ek_ctx* ctx, const ek_hgr* h, const ek_fm_opts* opts, uint8_t* side_inout /* nodes */,
                   int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log, int64_t move_cap,
                   ek_fm_w_result* result);

/* ------------------------------------------------------------------ */
/* Coarsening: a heavy-edge matching, the contraction it defines, and   */
/* the multilevel bipartition over them.  No reference counterpart.     */
/* ------------------------------------------------------------------ */
/* The matching rule, all integers, every tie broken by ids.
 * The input is the FM rules': the nets with at least 2 distinct pins, each pin
 * once; w(v) and c(e) of h, 1 where h carries no such array.  Net e is
 * eligible iff its distinct size |e| <= max_net; score(e) = floor(c(e) 2^20 /
 * (|e| - 1)), int64.  Every node starts unmatched (mate -1).
 * One round, all of it read from the state at the round's start: (1) every
 * unmatched u looks at the entries (e, v) with e eligible, u and v pins of e,
 * v != u, v unmatched and w(u) + w(v) <= max_cluster; p(u) is the v of the
 * entry of greatest (score(e), then smaller v), -1 without an entry.  A pair's
 * score is that of its best shared net, not a sum over its shared nets.  (2) u
 * and v are matched iff p(u) = v and p(v) = u.
 * The run ends with the first round that matches nothing (not counted, not
 * logged) or after max_rounds rounds.  While a feasible pair exists a round
 * matches one (the entry of greatest score whose smaller id is least proposes
 * both ways), so max_rounds <= 0 ends at a maximal matching.
 * The cluster of a node is itself and its mate; the cluster's leader is its
 * least id; cluster[v] = the rank of v's leader among all leaders in ascending
 * id order; n_coarse = the number of leaders. */
typedef struct {
    int32_t max_net;     /* default 64; values below 2 act as 2 */
    int32_t max_rounds;  /* default 8; <= 0: until a round matches nothing */
    int64_t max_cluster; /* the greatest w(u) + w(v) of a pair; >= 1 (ek_match_default_opts: 2) */
} ek_match_opts;

typedef struct {
    int64_t n, n_coarse, pairs; /* nodes; clusters; matched pairs = n - n_coarse */
    int32_t rounds, pad;        /* rounds that matched at least one pair */
    int64_t eligible_nets;
    double t_setup, t_rounds;   /* wall seconds (host clock) */
} ek_match_result;

void ek_match_default_opts(ek_match_opts* o);
/* The matching on the host (no GPU): the checker of ek_match, single threaded
 * and written from the rule.  mate_out and cluster_out: one value per node of
 * h, either may be NULL.  round_log (may be NULL) receives two values per
 * round, for the first log_rounds rounds: proposers (p(u) >= 0) and pairs.
 * EK_EINVAL for max_cluster < 1, more than INT32_MAX - 1 nodes, and the weight
 * ranges of ek_fm_refine_w. */
int ek_match_host(const ek_hgr* h, const ek_match_opts* opts, int32_t* mate_out, int32_t* cluster_out,
                  int64_t* round_log, int64_t log_rounds, ek_match_result* result);
/* The same on the GPU: the same mate, cluster, round log and result integers.
 * Two launches a round; the host reads one 8-byte counter per round.
 * EK_ESTATE on a multi-rank context.  Every buffer is local to the call and
 * the context keeps nothing. */
int ek_match(ek_ctx* ctx, const ek_hgr* h, const ek_match_opts* opts, int32_t* mate_out, int32_t* cluster_out,
             int64_t* round_log, int64_t log_rounds, ek_match_result* result);

/* The clustering rule: a coarsening in which a node may join a
 * cluster of more than two nodes.  All integers, every tie broken by ids.  The
 * input, the options (ek_match_opts: max_cluster >= 1 bounds a cluster's
 * weight), eligibility and score(e) are the matching's.
 * State: rep[v], initially v; S(r), the weight of the cluster whose root is r
 * (int64, initially w(r)).  A node u is single iff rep[u] = u and nothing has
 * joined it.  A root never moves once something has joined it; a node that
 * has joined never moves again.
 * One round, every step reading the state at the round's start:
 * (1) Propose.  Every single u looks at the entries (e, v) with e eligible, u
 *     and v pins of e, v != u, r = rep[v] and S(r) + w(u) <= max_cluster; t(u)
 *     is the r of the entry of greatest (score(e), then smaller r), sigma(u)
 *     that score; -1 without an entry and for a node that is not single.
 * (2) Incoming.  in[v] = 1 iff some u has t(u) = v.
 * (3) Resolve.  ml(x): t(x) = z >= 0, t(z) = x and x > z (the larger id of a
 *     mutual pair of singles).  u is a mover iff t(u) = r >= 0, (in[u] = 0 or
 *     ml(u)) and not ml(r): a single that others propose to stays put unless
 *     it is the larger of a mutual pair, and a node whose target is itself
 *     leaving waits a round.
 * (4) Accept.  Per destination r the movers with t = r are ordered by (sigma
 *     descending, id ascending); a mover is accepted iff the sum of w over
 *     the order up to and including it is at most max_cluster - S(r).
 * (5) Apply.  Accepted u: rep[u] = r, S(r) += w(u); u and r are single no more.
 * The run ends with the first round that accepts nothing (not counted, not
 * logged) or after max_rounds rounds.  A round with a proposer accepts at
 * least one node, so max_rounds <= 0 ends where no single node fits into a
 * cluster it shares an eligible net with.  Every cluster of more than one node
 * weighs at most max_cluster.  cluster[v] = the rank of rep[v] among the roots
 * (rep[x] = x) in ascending id order; n_coarse = the number of roots. */
typedef struct {
    int64_t n, n_coarse, joins; /* nodes; clusters; accepted moves = n - n_coarse */
    int32_t rounds, pad;        /* rounds that accepted at least one node */
    int64_t eligible_nets;
    int64_t heaviest;           /* the greatest S(r) over the roots (a single node may outweigh max_cluster) */
    double t_setup, t_rounds;   /* wall seconds (host clock) */
} ek_cluster_result;

/* The clustering on the host (no GPU): the checker of ek_cluster, single
 * threaded and written from the rule.  rep_out and cluster_out: one value per
 * node of h, either may be NULL.  round_log (may be NULL) receives three values
 * per round, for the first log_rounds rounds: proposers (t(u) >= 0), movers and
 * joins.  opts NULL: ek_match_default_opts.  EK_EINVAL as ek_match_host. */
int ek_cluster_host(const ek_hgr* h, const ek_match_opts* opts, int32_t* rep_out, int32_t* cluster_out,
                    int64_t* round_log, int64_t log_rounds, ek_cluster_result* result);
/* The same on the GPU: the same rep, cluster, round log and result integers,
 * whatever order the workgroups run in.  The host reads one 8-byte counter per
 * round.  EK_ESTATE on a multi-rank context.  Every buffer is local to the call
 * and the context keeps nothing. */
int ek_cluster(ek_ctx* ctx, const ek_hgr* h, const ek_match_opts* opts, int32_t* rep_out, int32_t* cluster_out,
               int64_t* round_log, int64_t log_rounds, ek_cluster_result* result);

/* The contraction of h along cluster (host only): any map of h's nodes onto
 * [0, n_coarse) that hits every value.  A coarse node weighs the sum of its
 * nodes' w(v).  Every net of h, in file order, is mapped through cluster, its
 * pins made distinct in first-occurrence order; a net left with fewer than 2
 * pins is dropped; nets with the same pin set merge into the first of them,
 * their c(e) summed.  The result always carries both weight arrays.  The
 * weighted cut and the side weights of any coarse side vector s' equal those
 * of s'(cluster(.)) on h (ek_bipart_metrics_host out[0], out[2], out[3]; the
 * cut NETS differ: merged nets count once).  EK_EINVAL for
 * a cluster id outside [0, n_coarse), an id no node maps to, or a summed
 * weight above INT32_MAX. */
int ek_hgr_contract(const ek_hgr* h, const int32_t* cluster /* nodes */, int64_t n_coarse, ek_hgr** out);

/* The multilevel bipartition.  H_0 = h.  While H_l holds more
 * than coarse_nodes nodes and l < max_levels: ek_match, then ek_hgr_contract;
 * the new level is dropped and coarsening ends when it shrinks by less than
 * 10 % (10 n_(l+1) > 9 n_l).  On the coarsest H_L: ek_spmv_setup_pins,
 * ek_lanczos_fiedler, ek_sweep_cut_w at `imbalance`, sides = ek_rank_split(v,
 * n1); without a net of >= 2 pins, below the nodes ek_lanczos_fiedler accepts,
 * or on EK_ENOCONV, v[i] = -i instead (coarsest_fallback = 1).  Then
 * ek_fm_refine_w on H_L, and for l = L - 1 .. 0 the sides projected through
 * cluster_l and ek_fm_refine_w on H_l.  No KL: it swaps pairs and ignores
 * weights.  Lanczos sees the coarse structure only, not its weights. */
#define EK_ML_LEVELS 32 /* the most coarse levels; the per-level arrays also hold the input, level 0 */
typedef struct {
    double imbalance;     /* epsilon >= 0; default 0.03; overwrites fm.imbalance */
    int32_t coarse_nodes; /* coarsening stops at this many nodes; default 512; values below 8 act as 8 */
    int32_t max_levels;   /* default and maximum EK_ML_LEVELS; values outside [1, EK_ML_LEVELS] act as it */
    ek_match_opts match;  /* max_cluster <= 0 (default): max(1, min(2 L_max - W + 1, ceil(4 W / coarse_nodes))),
                           * the first term being the condition under which ek_sweep_cut_w has a feasible split */
    ek_fm_opts fm;
    ek_lanczos_opts lanczos;
} ek_ml_opts;

typedef struct {
    int32_t levels;            /* L: the coarse levels kept; level l of the arrays below is H_l, 0 <= l <= L */
    int32_t coarsest_fallback; /* 1: the coarsest split came from v[i] = -i */
    int64_t nodes[EK_ML_LEVELS + 1], nets[EK_ML_LEVELS + 1], pins[EK_ML_LEVELS + 1];
    int64_t match_rounds[EK_ML_LEVELS + 1], match_pairs[EK_ML_LEVELS + 1]; /* of the matching H_l -> H_(l+1), l < L */
    int64_t cut_before[EK_ML_LEVELS + 1], cut_after[EK_ML_LEVELS + 1];     /* weighted cut around H_l's FM */
    int64_t fm_moves[EK_ML_LEVELS + 1];                                    /* moves that FM kept */
    int64_t sweep_feasible;    /* the coarsest sweep's `feasible` */
    int64_t max_cluster;       /* the matching's bound as used */
    int64_t total_weight, max_part;  /* W; L_max = floor((1 + imbalance) ceil(W / 2)) */
    int64_t cut, cut_nets, w0, w1, n0, n1; /* ek_bipart_metrics_host of side_out on h, and the sides' node counts */
    double t_match, t_contract, t_lanczos, t_sweep, t_fm, t_total; /* wall seconds (host clock) */
} ek_ml_result;

void ek_ml_default_opts(ek_ml_opts* o);
/* side_out: one byte in {0, 1} per node of h.  EK_ESTATE on a multi-rank
 * context; EK_EINVAL as the entries it calls.  result may be NULL. */
int ek_multilevel_bipartition(ek_ctx* ctx, const ek_hgr* h, const ek_ml_opts* opts, uint8_t* side_out /* nodes */,
                              ek_ml_result* result);
/* The same on the hMETIS reading of a file (ek_hgr_read_weighted), written to
 * results/<base>.part.2 under out_dir (NULL: the CWD), one side per line in
 * node order.  side_out may be NULL. */
int ek_multilevel_bipartition_file(ek_ctx* ctx, const char* path, const ek_ml_opts* opts, const char* out_dir,
                                   uint8_t* side_out, ek_ml_result* result);
/* As the two above.  flags = 0: exactly they.  flags & EK_ML_WEIGHTED_LAPLACIAN:
 * the coarsest level's ek_spmv_setup_pins is ek_spmv_setup_pins_w with H_L's
 * net weights (the summed c(e) of the nets ek_hgr_contract merged), so Lanczos
 * sees them; nothing else in the V-cycle changes.  EK_EINVAL for any other
 * flag bit. */
#define EK_ML_WEIGHTED_LAPLACIAN 1
int ek_multilevel_bipartition_ex(ek_ctx* ctx, const ek_hgr* h, const ek_ml_opts* opts, int32_t flags,
                                 uint8_t* side_out /* nodes */, ek_ml_result* result);
int ek_multilevel_bipartition_file_ex(ek_ctx* ctx, const char* path, const ek_ml_opts* opts, const char* out_dir,
                                      int32_t flags, uint8_t* side_out, ek_ml_result* result);

/* ------------------------------------------------------------------ */
/* Per-side weight bounds: the weighted sweep, the weighted FM and the   */
/* V-cycle under B = (L0, L1), and the k-way partition by recursive       */
/* multilevel bisection over them.  No reference          */
/* counterpart.                                                           */
/* ------------------------------------------------------------------ */
/* bounds[s] = L_s is the greatest weight side s may hold.  0 <= L_s <= W, L0 +
 * L1 >= W and W <= 2^61, each EK_EINVAL otherwise (a caller clamps a looser
 * bound to W).  The slack difference of side weights (S0, S1) is D(S0, S1) =
 * |(S0 - L0) - (S1 - L1)|; with L0 = L1 it is |S0 - S1|.
 *
 * The bounded sweep is the rule of ek_sweep_cut_w with three replacements.
 * Split s is feasible iff P[s] <= L1 and W - P[s] <= L0 (side 1 of split s
 * weighs P[s]).  Wherever that rule compares |2 P[s] - W| it compares D(W -
 * P[s], P[s]) = |2 P[s] - W + (L0 - L1)|, in the feasible choice and in the
 * fallback alike.  The feasible splits are one contiguous range, certainly not
 * empty when max w(v) <= L0 + L1 - W + 1.  opts->imbalance is ignored and
 * objective must be 0.  With L0 = L1 = floor((1 + eps) ceil(W / 2)) the
 * entries reproduce ek_sweep_cut_w* at imbalance eps exactly. */
typedef struct {
    int64_t n, n0, n1;        /* nodes; side 0 and side 1 of the chosen split (n1 = s*) */
    int64_t s_lo, s_hi;       /* the feasible splits (0, 0 when there is none) */
    int64_t feasible;         /* 1: the window is not empty */
    int64_t total_weight;     /* W */
    int64_t bound0, bound1;   /* L0, L1 */
    int64_t w0, w1;           /* the sides' weights at s*: W - P[s*], P[s*] */
    int64_t cut;              /* profile_w[s*] */
    int64_t cut_nets;         /* the count profile at s* */
    int64_t cut_half;         /* profile_w[floor(n / 2)] */
    int64_t spanning_nets;    /* nets with lo < hi */
    double t_sort, t_profile, t_select; /* wall seconds (host clock) */
} ek_sweep_wb_result;
/* The checker: single threaded, written from the rule.  Arguments as
 * ek_sweep_cut_w_host plus the bounds. */
int ek_sweep_cut_wb_host(const ek_hgr* h, const double* v, const ek_sweep_opts* opts, const int64_t bounds[2],
                         int32_t* order_out, int64_t* profile_out /* n + 1 */, int64_t* prefix_out /* n + 1 */,
                         ek_sweep_wb_result* result);
/* The same on the GPU: the same order, profile_w, P and result integers. */
int ek_sweep_cut_wb(ek_ctx* ctx, const ek_hgr* h, const double* v_host, const ek_sweep_opts* opts,
                    const int64_t bounds[2], int32_t* order_out, int64_t* profile_out /* n + 1 */,
                    int64_t* prefix_out /* n + 1 */, ek_sweep_wb_result* result);

/* The bounded FM is the rule of ek_fm_refine_w with these replacements.
 * (c) side a's top node is a candidate iff S[1 - a] + w(top) <= L_(1-a).
 * d_t = D(S_0, S_1).  (d) on equal g the candidate whose side has less slack
 * (greater S_a - L_a) moves, then the smaller id.  A side already above its
 * bound never receives.  opts->imbalance is ignored.  A pass_log row ends with
 * D after the rollback.  With L0 = L1 = floor((1 + eps) ceil(W / 2)) the
 * entries reproduce ek_fm_refine_w* at imbalance eps exactly. */
typedef struct {
    int64_t n, total_weight, bound0, bound1; /* nodes; W; L0, L1 */
    int32_t passes, passes_run;        /* counted passes (t* > 0); passes run (at most one more) */
    int64_t moves_tried, moves_kept;   /* sum of t and of t* over the passes run */
    int64_t cut_before, cut;           /* the weighted cut of the sides given and of the sides returned */
    int64_t cut_nets_before, cut_nets; /* the cut nets of the same */
    int64_t w0, w1, n0, n1;            /* the sides' weights and node counts after the run */
    double t_setup, t_passes, t_metrics; /* wall seconds (host clock) */
} ek_fm_wb_result;
int ek_fm_refine_wb_host(const ek_hgr* h, const ek_fm_opts* opts, const int64_t bounds[2], uint8_t* side_inout /* nodes */,
                         int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log, int64_t move_cap,
                         ek_fm_wb_result* result);
int ek_fm_refine_wb(ek_ctx* ctx, const ek_hgr* h, const ek_fm_opts* opts, const int64_t bounds[2],
                    uint8_t* side_inout /* nodes */, int64_t* pass_log, int64_t log_passes, ek_fm_move* move_log,
                    int64_t move_cap, ek_fm_wb_result* result);

/* ek_multilevel_bipartition_ex with ek_sweep_cut_wb and ek_fm_refine_wb in
 * place of ek_sweep_cut_w and ek_fm_refine_w.  opts->imbalance is ignored.
 * The default max_cluster is max(1, min(L0 + L1 - W + 1, ceil(4 W /
 * coarse_nodes))).  result->max_part reports max(L0, L1). */
int ek_multilevel_bipartition_b(ek_ctx* ctx, const ek_hgr* h, const ek_ml_opts* opts, int32_t flags,
                                const int64_t bounds[2], uint8_t* side_out /* nodes */, ek_ml_result* result);

/* The bounds of one bisection of the k-way recursion (host).  A block of
 * weight Wb destined for kb >= 2 parts splits as ek_kway_plan does: side 0
 * gets k_0 = ceil(kb / 2) parts, side 1 k_1 = floor(kb / 2).  out[s] = min(k_s
 * part_bound, floor(mult ceil(Wb k_s / kb))), then clamped to Wb.  If Wb <= kb
 * part_bound then out[0] + out[1] >= Wb, and a side within out[s] satisfies
 * that premise for its own bisections.  EK_EINVAL for Wb < 0,
 * kb outside 2..256, part_bound < 0, mult not finite or < 1, a null out. */
int ek_kway_bisect_bounds(int64_t Wb, int32_t kb, int64_t part_bound, double mult, int64_t out[2]);

/* out[0] = cut nets (lambda_e >= 2), out[1] = the connectivity sum(lambda_e -
 * 1), out[2] = the weighted connectivity sum c(e)(lambda_e - 1), out[3] = SOED,
 * out[4 + p] = the node weight of part p, p < k.  lambda_e and the nets that
 * count: the conventions of ek_kway_metrics_host.  Weights: h's, 1 where it
 * carries none.  EK_EINVAL for k outside 1..256 or a part id outside [0, k). */
int ek_kway_metrics_w_host(const ek_hgr* h, const int32_t* part /* nodes */, int32_t k, int64_t* out /* 4 + k */);
/* The same on the GPU (int64 sums by integer atomics). */
int ek_kway_metrics_w(ek_ctx* ctx, const ek_hgr* h, const int32_t* part /* nodes */, int32_t k,
                      int64_t* out /* 4 + k */);

typedef struct {
    int32_t k;             /* number of parts, 2..256 */
    int32_t flags;         /* ek_multilevel_bipartition_ex's */
    double imbalance;      /* epsilon >= 0; default 0.03: part_bound = floor((1 + eps) ceil(W / k)) */
    int32_t write_results; /* ek_partition_kway_ml_file: 1 writes results/<base>.part.<k> under out_dir */
    int32_t pad;
    const char* out_dir;   /* NULL: the CWD */
    ek_ml_opts ml;         /* coarse_nodes, max_levels, match, fm, lanczos of every bisection; ml.imbalance is ignored */
} ek_kway_ml_opts;

typedef struct {
    int32_t k;
    int32_t bisections;         /* bisections run (blocks of >= 2 nodes destined for >= 2 parts) */
    int32_t coarsest_fallbacks; /* of which split their coarsest level by node index */
    int32_t infeasible_sweeps;  /* of which had no feasible sweep split */
    int64_t total_weight, part_bound; /* W; Lk = floor((1 + imbalance) ceil(W / k)) */
    int64_t part_w_min, part_w_max;   /* lightest / heaviest part */
    int64_t parts_over_bound, empty_parts; /* parts above Lk; parts of no node */
    int64_t cut_nets, connectivity, connectivity_w, soed; /* ek_kway_metrics_w of part_out */
    int64_t levels_total, fm_moves;   /* coarse levels and kept FM moves, summed over the bisections */
    /* wall seconds (host clock): the sub-hypergraphs, the bisections, the metrics, all; the bisections' phases */
    double t_induce, t_ml, t_metrics, t_total;
    double t_match, t_contract, t_lanczos, t_sweep, t_fm;
    double t_level[EK_KWAY_LEVELS]; /* per recursion level (root = 0), its blocks' induce + bisections */
} ek_kway_ml_result;

void ek_kway_ml_default_opts(ek_kway_ml_opts* o);
/* k-way partition of h by recursive multilevel bisection, depth first, side 0
 * before side 1, as ek_partition_kway recurses: a block is ek_hgr_induce'd
 * (weights carried), its bounds come from ek_kway_bisect_bounds with
 * part_bound = Lk and mult = (1 + imbalance)^(1 / ceil(log2 k)) (1 + imbalance
 * itself when ceil(log2 k) = 1), and it is bisected by
 * ek_multilevel_bipartition_b.  A block of fewer than 2 nodes gives all its
 * nodes the id `base` with no bisection.  Empty parts are allowed and counted.
 * With unit node weights every part weighs at most Lk; with arbitrary weights a
 * part may end above it (parts_over_bound), which is reported, not an error.
 * EK_ESTATE on a multi-rank context; EK_EINVAL unless 2 <= k <= 256.  result
 * may be NULL.  Keeps nothing on the context beyond what its pieces do. */
int ek_partition_kway_ml(ek_ctx* ctx, const ek_hgr* h, const ek_kway_ml_opts* opts, int32_t* part_out /* nodes */,
                         ek_kway_ml_result* result);
/* The same on the hMETIS reading of a file (ek_hgr_read_weighted); part_out
 * may be NULL.  With write_results: results/<base>.part.<k> under out_dir. */
int ek_partition_kway_ml_file(ek_ctx* ctx, const char* path, const ek_kway_ml_opts* opts, int32_t* part_out,
                              ek_kway_ml_result* result);

/* ------------------------------------------------------------------ */
/* Weighted k-way connectivity refinement under per-part weight bounds. */
/* No reference counterpart.                                             */
/* ------------------------------------------------------------------ */
/* The rule of ek_kway_refine on the weighted connectivity sum c(e)(lambda_e -
 * 1) of a part vector, with node weights under the bounds.
 * Input as ek_fm_refine_w: the nets with at least 2 distinct pins, each pin
 * once; w(v) >= 0 and c(e) >= 1, 1 where h carries no such array; W = sum w(v);
 * D(v) = the sum of c(e) over v's nets, at most 2^31 - 1; W and the sum of all
 * c(e) at most 2^62.  S(p) is the weight of part p.  L_p, the bound of part p,
 * is bounds[p] when bounds is given (k values, each >= 0; opts->imbalance is
 * then ignored), otherwise floor((1 + imbalance) ceil(W / k)) for every part,
 * ek_partition_kway_ml's part_bound.  One round, all of it read from the state
 * at the round's start, with these replacements in ek_kway_refine's:
 *  (a) r(v) = the sum of c(e) over v's nets in which v is its part's only pin,
 *      c(v,b) the same over its nets with a pin in b, g(v,b) = (r(v) - D(v)) +
 *      c(v,b), in that order inside int32: what moving v alone to b takes off
 *      the weighted connectivity;
 *  (b) part b (not v's own) is open for v iff S(b) + w(v) <= L_b; the target is
 *      the open part of greatest g, ties to the smaller b, and v is a candidate
 *      iff that g > 0;
 *  (c) winners and independence as there; per part b the independent candidates
 *      with target b in (g descending, id ascending) order, and the accepted set
 *      is the LONGEST PREFIX of that order whose summed w(v) is at most L_b -
 *      S(b): a node that does not fit ends the part's intake for the round, even
 *      when a lighter, later one would fit; nodes of weight 0 directly after the
 *      last fitting node are accepted, those after the first rejected are not;
 *  (d) accepted nodes move; rounds repeat until one accepts nothing (not
 *      counted, not logged) or max_rounds rounds have moved.
 * Accepted nodes share no net, so the weighted connectivity falls by exactly the
 * round's gain.  No part ends above max(L_p, its initial S(p)); a part already
 * above its bound never receives, not even a node of weight 0; there is no
 * lower bound on a part's weight.  With every weight 1 and no bounds the rule is
 * ek_kway_refine's word for word. */
typedef struct {
    int32_t k, rounds;                     /* rounds that moved at least one node */
    int64_t moves, gain_total;             /* accepted moves; connectivity_w_before - connectivity_w */
    int64_t total_weight;                  /* W */
    int64_t bound_min, bound_max;          /* least / greatest L_p as used */
    int64_t part_w_min, part_w_max;        /* after the run */
    int64_t parts_over_bound;              /* parts with S(p) > L_p after the run */
    int64_t connectivity_w_before;
    int64_t cut_nets, connectivity, connectivity_w, soed; /* ek_kway_metrics_w of the result */
    double t_setup, t_rounds, t_metrics;   /* wall seconds (host clock) */
} ek_kway_refine_w_result;

/* The refinement on the host (no GPU): the checker of ek_kway_refine_w, single
 * threaded and written from the rule.  Arguments as ek_kway_refine_host
 * (ek_kway_refine_opts is reused), plus bounds (k values, or NULL).  EK_EINVAL
 * as there, plus a bound < 0 and the weight ranges above. */
int ek_kway_refine_w_host(const ek_hgr* h, const ek_kway_refine_opts* opts, const int64_t* bounds /* k, or NULL */,
                          int32_t* part_inout, int64_t* round_log, int64_t log_rounds, ek_kway_refine_w_result* result);
/* The same on the GPU: the same part vector, round log and result integers.
 * Six launches a round; the host reads one 8-byte counter per round.  EK_ESTATE
 * on a multi-rank context.  Keeps nothing on the context: every buffer is local
 * to the call. */
int ek_kway_refine_w(ek_ctx* ctx, const ek_hgr* h, const ek_kway_refine_opts* opts, const int64_t* bounds,
                     int32_t* part_inout, int64_t* round_log, int64_t log_rounds, ek_kway_refine_w_result* result);

/* ------------------------------------------------------------------ */
/* Parallel weighted k-way refinement that can leave a local minimum    */
/* (the Jet rule on the connectivity metric).  No reference counterpart. */
/* ------------------------------------------------------------------ */
/* Input, weights, S(p) and the bounds L_p exactly as ek_kway_refine_w
 * (DESIGN.md §18).  State: the part vector, S and one lock per node, all clear
 * at the start.  Everything is integer, ties are broken by ids, and iteration
 * i = 1, 2, ... reads only the state at its start:
 *  (a) for an unlocked v on at least one net, a = part(v): r(v), c(v,b) and
 *      g(v,b) = (r - D) + c(v,b) as ek_kway_refine_w's (a).  The target t(v) is
 *      the open part (S(b) + w(v) <= L_b, b != a) of greatest g, ties to the
 *      smaller b, WHATEVER THE SIGN of g.  v is a candidate iff it has an open
 *      part and either g >= 0 or -g neg_den < neg_num (D(v) - r(v)), in int64.
 *      Its key is K(v) = ((g + 2^31) << 32) | ~id: never 0, unique, ordered by
 *      (g descending, id ascending);
 *  (b) the afterburner: for a candidate v and a pin u != v of one of its nets,
 *      p'(u) = t(u) if u is a candidate with K(u) > K(v), else part(u);
 *      g'(v) = the sum over v's nets e of c(e) ([no u in e \ {v} has p'(u) = a]
 *      - [no u in e \ {v} has p'(u) = t(v)]); v passes iff g'(v) >= 0.  A
 *      better-ranked candidate counts as moved whether or not it passes;
 *  (c) per part b the passing candidates with target b in K-descending order;
 *      the accepted set is the longest prefix whose summed w is at most L_b -
 *      S(b), ek_kway_refine_w's (c) word for word;
 *  (d) accepted nodes move; exactly they are locked during iteration i + 1;
 *  (e) X_i is the weighted connectivity recounted after the moves (accepted
 *      nodes may share nets, so it is not X_{i-1} minus the gains); X_0 is the
 *      start's.  If X_i < best (strictly): best = X_i, best_iter = i, the part
 *      vector is kept as the snapshot and since = 0; otherwise ++since;
 *  (f) stop after iteration i when since == patience, or i == max_iters (when
 *      > 0), or iterations i and i - 1 both accepted nothing ("iteration 0"
 *      accepted nothing): no node is locked then and i + 1 would repeat i.
 * With no net of 2 distinct pins the call returns at once (0 iterations).  The
 * result is the SNAPSHOT, the start itself when nothing improved, and the
 * result's part weights and metrics are recounted from it.  Its weighted
 * connectivity is at most the start's; no part ends above max(L_p, its initial
 * S(p)); a single iteration may raise the objective. */
typedef struct {
    int32_t k;         /* number of parts, 2..256 */
    int32_t max_iters; /* <= 0: none */
    int32_t patience;  /* iterations without a new best before the stop, >= 1; default 12 */
    int32_t neg_num;   /* the negative-gain filter neg_num / neg_den: >= 0, default 1 */
    int32_t neg_den;   /* >= 1, default 4 */
    int32_t pad;
    double imbalance;  /* epsilon >= 0 of the uniform bound; default 0.03; ignored with bounds */
} ek_kway_jet_opts;
void ek_kway_jet_default_opts(ek_kway_jet_opts* opts);

typedef struct {
    int32_t k, iters, best_iter, pad;      /* iterations run; the one the result is the state after (0: the start) */
    int64_t moves;                         /* accepted moves over all iterations, those rolled back among them */
    int64_t total_weight;                  /* W */
    int64_t bound_min, bound_max;          /* least / greatest L_p as used */
    int64_t connectivity_w_before;         /* X_0 */
    int64_t cut_nets, connectivity, connectivity_w, soed; /* ek_kway_metrics_w of the result */
    int64_t part_w_min, part_w_max;        /* of the result */
    int64_t parts_over_bound;              /* parts of the result with S(p) > L_p */
    double t_setup, t_iters, t_metrics;    /* wall seconds (host clock) */
} ek_kway_jet_result;

/* The refinement on the host (no GPU): the checker of ek_kway_jet, single
 * threaded and written from the rule.  part_inout: the start on entry, the
 * snapshot on return.  iter_log (may be NULL) gets four values per iteration,
 * for the first log_iters iterations: candidates, passing candidates, accepted
 * moves and X_i; every iteration that ran is logged, the last included.
 * EK_EINVAL as ek_kway_refine_w_host, plus neg_num < 0, neg_den < 1 and
 * patience < 1. */
int ek_kway_jet_host(const ek_hgr* h, const ek_kway_jet_opts* opts, const int64_t* bounds /* k, or NULL */,
                     int32_t* part_inout, int64_t* iter_log, int64_t log_iters, ek_kway_jet_result* result);
/* The same on the GPU: the same part vector, iteration log and result integers.
 * Six launches an iteration; the host reads one 64-byte record per iteration.
 * EK_ESTATE on a multi-rank context.  Keeps nothing on the context: every
 * buffer is local to the call. */
int ek_kway_jet(ek_ctx* ctx, const ek_hgr* h, const ek_kway_jet_opts* opts, const int64_t* bounds,
                int32_t* part_inout, int64_t* iter_log, int64_t log_iters, ek_kway_jet_result* result);

/* ------------------------------------------------------------------ */
/* Direct k-way multilevel: one coarsening, the Jet refinement at every  */
/* level, contraction on the device.  No reference        */
/* counterpart.                                                           */
/* ------------------------------------------------------------------ */
typedef struct {
    int32_t hash_bits; /* the low bits of a net's 64-bit set signature that group the nets, 1..64; default 64 */
    int32_t pad;
} ek_contract_opts;
void ek_contract_default_opts(ek_contract_opts* opts);
/* ek_hgr_contract on the GPU: the same hypergraph byte for byte (nodes, nets,
 * net_ptr, pins, node_w, net_w) and the same EK_EINVAL cases (an id outside
 * [0, n_coarse), an unhit cluster, a cluster or merged-net weight above 2^31 -
 * 1, a null argument), plus hash_bits outside 1..64.  Nets are grouped by the
 * low hash_bits bits of an order-independent signature of their distinct pin
 * set; inside a group two nets merge only after their sets compared equal pin
 * by pin, so the result does not depend on hash_bits (a small value only makes
 * the groups, and the call, larger).  Integer arithmetic and integer atomic adds
 * only; the result does not depend on the order threads run in.  EK_ESTATE on a
 * multi-rank context.  Keeps nothing on the context: every buffer is local to
 * the call.  opts may be NULL. */
int ek_hgr_contract_device(ek_ctx* ctx, const ek_hgr* h, const int32_t* cluster /* nodes */, int64_t n_coarse,
                           const ek_contract_opts* opts, ek_hgr** out);

#define EK_KWAY_DIRECT_HOST_CONTRACT 1     /* ek_hgr_contract in place of ek_hgr_contract_device */
#define EK_KWAY_DIRECT_WEIGHTED_LAPLACIAN 2 /* EK_ML_WEIGHTED_LAPLACIAN for the initial partition */
typedef struct {
    int32_t k;             /* number of parts, 2..256 */
    int32_t flags;         /* EK_KWAY_DIRECT_*; any other bit: EK_EINVAL */
    double imbalance;      /* epsilon >= 0; default 0.03: part_bound Lk = floor((1 + eps) ceil(W / k)) */
    int32_t coarse_nodes;  /* coarsening stops at this many nodes; <= 0 (default): max(512, 128 k) */
    int32_t max_levels;    /* default and maximum EK_ML_LEVELS; values outside [1, EK_ML_LEVELS] act as it */
    ek_match_opts match;   /* max_cluster <= 0 (default): max(1, min(ceil(4 W / coarse_nodes), max(1, Lk - ceil(W / k)))) */
    ek_kway_ml_opts initial; /* the coarsest level's partition: its ml is used; k, flags, imbalance, write_results
                              * and out_dir are overwritten */
    ek_kway_jet_opts jet;  /* every level's refinement: max_iters, patience, neg_num, neg_den are used; k and imbalance
                            * are overwritten */
    int32_t write_results; /* ek_partition_kway_direct_file: 1 writes results/<base>.part.<k> under out_dir */
    int32_t pad;
    const char* out_dir;   /* NULL: the CWD */
} ek_kway_direct_opts;

typedef struct {
    int32_t k;
    int32_t levels;            /* L: the coarse levels kept; level l of the arrays below is H_l, 0 <= l <= L */
    int32_t initial_fallbacks; /* the initial partition's coarsest_fallbacks */
    int32_t infeasible_sweeps; /* the initial partition's infeasible_sweeps */
    int64_t nodes[EK_ML_LEVELS + 1], nets[EK_ML_LEVELS + 1], pins[EK_ML_LEVELS + 1];
    int64_t match_rounds[EK_ML_LEVELS + 1], match_pairs[EK_ML_LEVELS + 1]; /* of the matching H_l -> H_(l+1), l < L */
    int64_t conn_w_before[EK_ML_LEVELS + 1], conn_w_after[EK_ML_LEVELS + 1]; /* weighted connectivity around H_l's Jet */
    int64_t jet_iters[EK_ML_LEVELS + 1], jet_moves[EK_ML_LEVELS + 1];
    int64_t total_weight, part_bound, max_cluster; /* W; Lk; the matching's bound as used */
    int64_t part_w_min, part_w_max, parts_over_bound, empty_parts;
    int64_t cut_nets, connectivity, connectivity_w, soed; /* ek_kway_metrics_w of part_out on h */
    double t_match, t_contract, t_initial, t_jet, t_metrics, t_total; /* wall seconds (host clock) */
} ek_kway_direct_result;

void ek_kway_direct_default_opts(ek_kway_direct_opts* opts);
/* k-way partition of h by one multilevel cycle.  W = sum w(v), Lk = floor((1 +
 * imbalance) ceil(W / k)).  (1) Coarsen as ek_multilevel_bipartition does:
 * while H_l has more than coarse_nodes nodes and l < max_levels, ek_match; stop
 * if 10 n_(l+1) > 9 n_l; otherwise contract (ek_hgr_contract_device, or
 * ek_hgr_contract under EK_KWAY_DIRECT_HOST_CONTRACT: the same hypergraph).
 * (2) ek_partition_kway_ml of the coarsest H_L with the same k and imbalance.
 * (3) ek_kway_jet on H_L under the uniform bound, then for l = L - 1 .. 0:
 * part_l[v] = part_(l+1)[cluster_l[v]] and ek_kway_jet on H_l.  (4) The final
 * integers are ek_kway_metrics_w's on h.  conn_w_before[l] = conn_w_after[l +
 * 1]; conn_w_after[l] <= conn_w_before[l]; projection keeps every part's
 * weight; no part ends above max(Lk, its weight after the initial partition),
 * and one above Lk is reported in parts_over_bound, not an error.  EK_ESTATE on
 * a multi-rank context; EK_EINVAL for k outside 2..256, an imbalance that is
 * negative or not finite, an unknown flag bit.  result may be NULL. */
int ek_partition_kway_direct(ek_ctx* ctx, const ek_hgr* h, const ek_kway_direct_opts* opts, int32_t* part_out /* nodes */,
                             ek_kway_direct_result* result);
/* The same on the hMETIS reading of a file (ek_hgr_read_weighted); part_out
 * may be NULL.  With write_results: results/<base>.part.<k> under out_dir. */
int ek_partition_kway_direct_file(ek_ctx* ctx, const char* path, const ek_kway_direct_opts* opts, int32_t* part_out,
                                  ek_kway_direct_result* result);
/* The same with the coarsening of step (1) chosen.  EK_COARSEN_MATCH is
 * ek_partition_kway_direct itself, byte for byte.  EK_COARSEN_CLUSTER calls
 * ek_cluster where the loop calls ek_match, under the same
 * opts.match, the same max_cluster default, the same 10 % rule and the same
 * contraction; match_rounds and match_pairs of the result then hold the
 * clustering's rounds and joins.  Any other value: EK_EINVAL. */
#define EK_COARSEN_MATCH 0
#define EK_COARSEN_CLUSTER 1
int ek_partition_kway_direct_ex(ek_ctx* ctx, const ek_hgr* h, const ek_kway_direct_opts* opts, int32_t coarsening,
                                int32_t* part_out /* nodes */, ek_kway_direct_result* result);
int ek_partition_kway_direct_file_ex(ek_ctx* ctx, const char* path, const ek_kway_direct_opts* opts, int32_t coarsening,
                                     int32_t* part_out, ek_kway_direct_result* result);

/* ------------------------------------------------------------------ */
/* k-way rebalancing: bring overweight parts under their bounds (DESIGN.md */
/* §21, the second half of the Jet rule).  No reference counterpart.       */
/* ------------------------------------------------------------------ */
/* Input, weights, S(p) and the bounds L_p exactly as ek_kway_refine_w.  O =
 * {p : S(p) > L_p}, the excess x(p) = max(0, S(p) - L_p), X = sum x(p).  With O
 * empty the call returns the start (0 rounds).  Everything is integer, ties are
 * broken by ids, and round i = 1, 2, ... reads only the state at its start:
 *  (a) v proposes iff a = part(v) is in O and w(v) > 0 (nodes on no net too:
 *      every g is 0).  g(v,b) = (r - D) + c(v,b) as ek_kway_refine_w's (a); the
 *      target t(v) is the part b != a with S(b) + w(v) <= L_b of greatest g,
 *      ties to the smaller b, whatever the sign of g (no part of O fits).  v is
 *      a proposer iff such a part exists; K(v) = ((g + 2^31) << 32) | ~id;
 *  (b) per a in O the proposers of a in K-descending order: E(a) is the
 *      shortest prefix whose summed w reaches x(a), all of them when their
 *      total stays below it;
 *  (c) per part b the nodes of the union of the E(a) with target b in
 *      K-descending order: the accepted set is the longest prefix whose summed
 *      w is at most L_b - S(b), ek_kway_refine_w's (c);
 *  (d) accepted nodes move; evicted nodes that were not accepted stay and
 *      propose again against the new S;
 *  (e) stop when O is empty after the round, when a round accepted nothing
 *      (that round is neither counted nor logged), or after max_rounds rounds
 *      (when > 0).
 * Every logged round lowers X by at least 1; a part at or below its bound never
 * ends above it; a part above its bound never receives.  A part still above
 * its bound at the end (parts_over_bound, not an error) has no node of
 * positive weight that fits any other part, unless max_rounds stopped the run.
 * There is no promise about the weighted connectivity: it may rise, and the
 * result carries both values, recounted from the start and the final state. */
typedef struct {
    int32_t k;          /* number of parts, 2..256 */
    int32_t max_rounds; /* <= 0: none */
    double imbalance;   /* epsilon >= 0 of the uniform bound; default 0.03; ignored with bounds */
} ek_kway_rebalance_opts;
void ek_kway_rebalance_default_opts(ek_kway_rebalance_opts* opts);

typedef struct {
    int32_t k, rounds;                          /* rounds that moved a node */
    int64_t moves;                              /* accepted moves over all rounds */
    int64_t total_weight;                       /* W */
    int64_t bound_min, bound_max;               /* least / greatest L_p as used */
    int64_t parts_over_before, parts_over_bound; /* |O| of the start / of the result */
    int64_t excess_before, excess;              /* X of the start / of the result */
    int64_t connectivity_w_before;              /* of the start */
    int64_t connectivity_w;                     /* of the result; may exceed the start's */
    int64_t cut_nets, connectivity, soed;       /* ek_kway_metrics_w of the result */
    int64_t part_w_min, part_w_max;             /* of the result */
    double t_setup, t_rounds, t_metrics;        /* wall seconds (host clock) */
} ek_kway_rebalance_result;

/* The rebalancing on the host (no GPU): the checker of ek_kway_rebalance,
 * single threaded and written from the rule.  part_inout: the start on entry,
 * the final state on return.  round_log (may be NULL) gets four values per
 * logged round, for the first log_rounds rounds: proposers, evicted nodes,
 * moved nodes and X after the round.  EK_EINVAL as ek_kway_refine_w_host. */
int ek_kway_rebalance_host(const ek_hgr* h, const ek_kway_rebalance_opts* opts, const int64_t* bounds /* k, or NULL */,
                           int32_t* part_inout, int64_t* round_log, int64_t log_rounds,
                           ek_kway_rebalance_result* result);
/* The same on the GPU: the same part vector, round log and result integers.
 * Eight launches a round; the host reads one 32-byte record per round.
 * EK_ESTATE on a multi-rank context; EK_EHIP if the rounds pass the excess of
 * the start (every round lowers X) or the weights kept differ from a recount.
 * Keeps nothing on the context: every buffer is local to the call. */
int ek_kway_rebalance(ek_ctx* ctx, const ek_hgr* h, const ek_kway_rebalance_opts* opts, const int64_t* bounds,
                      int32_t* part_inout, int64_t* round_log, int64_t log_rounds, ek_kway_rebalance_result* result);

/* ek_partition_kway_direct_ex with a rebalancing step: at every level, after
 * the initial partition or the projection and before ek_kway_jet, if any part
 * is above Lk, ek_kway_rebalance under the uniform bound.  Level l of the
 * arrays is H_l: the parts above Lk and (excess_before) their excess when the
 * level was reached, the rebalancer's rounds and moves, the excess it left.
 * When no level starts above its bound, part_out and every integer of result
 * equal ek_partition_kway_direct_ex's.  rb may be NULL. */
typedef struct {
    int64_t over_before[EK_ML_LEVELS + 1], excess_before[EK_ML_LEVELS + 1];
    int64_t rb_rounds[EK_ML_LEVELS + 1], rb_moves[EK_ML_LEVELS + 1];
    int64_t excess_after[EK_ML_LEVELS + 1];
    double t_rebalance; /* wall seconds (host clock), inside result's t_total */
} ek_kway_direct_rb_result;
int ek_partition_kway_direct_rb(ek_ctx* ctx, const ek_hgr* h, const ek_kway_direct_opts* opts, int32_t coarsening,
                                int32_t* part_out /* nodes */, ek_kway_direct_result* result,
                                ek_kway_direct_rb_result* rb);
int ek_partition_kway_direct_rb_file(ek_ctx* ctx, const char* path, const ek_kway_direct_opts* opts, int32_t coarsening,
                                     int32_t* part_out, ek_kway_direct_result* result, ek_kway_direct_rb_result* rb);

/* ------------------------------------------------------------------ */
/* Drop-in CLIs: argv exactly as cEIG.cpp:138-237 / cKL.cpp:424-468 /    */
/* gKL.cu:672-713 / gKL2.cu:989-1033, outputs relative to the CWD.       */
/* tool = "cEIG" | "cKL" | "gKL" | "gKL2".  Returns the process exit code. */
/* ------------------------------------------------------------------ */
int ek_cli_main(const char* tool, int argc, char** argv);
/* As ek_cli_main.  flags & EK_CLI_NO_TEARDOWN: the GPU context is not
 * destroyed on return (every output is written and every stream drained
 * first); for an executable that then ends with _exit, leaving the context
 * to the process exit instead of the runtime's orderly teardown. */
#define EK_CLI_NO_TEARDOWN 1
int ek_cli_main_ex(const char* tool, int argc, char** argv, int flags);

#ifdef __cplusplus
}
#endif
#endif /* EIGKL_H */
