// Drop-in command-line tools cEIG / cKL / gKL / gKL2 (ek_cli_main).
//
// argv and outputs follow the reference executables, relative to the CWD:
//   cEIG <in.hgr>          -> pre_saved_EIG/<base>_out.txt   (cEIG.cpp:138-237)
//   cKL  <in.hgr> [-EIG]   -> results/<base>_KL_CutSize[_EIG]_output.txt
//                             (-EIG reads pre_saved_EIG/<base>_out.txt; cKL.cpp:424-468)
//   gKL  <in.hgr> [-EIG]   -> same as cKL (gKL.cu:672-713 computes the same
//                             KL on the GPU but with different, racy
//                             semantics; SURVEY §0 finding 3 — this alias
//                             keeps the cKL semantics, the parity target)
//   gKL2 <in.hgr> [-EIG]   -> -EIG computes the Fiedler split in-process on
//                             the GPU (gKL2.cu:989-1033 used a non-Fiedler
//                             power iteration; this uses the Lanczos solver)
// All of them create results/ and pre_saved_EIG/.  Every compute step runs
// on the GPU through the C-ABI; there is no CPU path.  Additive flags:
//   --device D  --seed S (random init)  --sign-ref FILE  --no-deflate
//   --ncv N  --tol T  --quiet
//   --spectra            the Lanczos of the reference's Spectra SymEigsSolver
//                        (cEIG.cpp:195-198): a full reorthogonalisation every
//                        step, restarts keeping Spectra's nev_adjusted, fp64
//                        basis reads (ek_lanczos_opts reorth 1, keep_min 0,
//                        basis32 0); default: partial reorthogonalisation, the
//                        ncv/5 restart floor and the fp32 basis shadow
//   --reorth full|partial  only the reorthogonalisation rule
//   --k N                gKL2 <in.hgr> -EIG only: N-way partition by recursive
//                        spectral bisection (ek_partition_kway_file) instead of
//                        the bipartition -> results/<base>.part.<N>, one part
//                        id per line in node order
//   --refine EPS         with --k: then the k-way connectivity refinement on
//                        the device (ek_kway_refine) with imbalance EPS; the
//                        refined vector is what results/<base>.part.<N> holds,
//                        and one more line beginning "refine:" is printed
//   --refine-rounds R    at most R rounds of it (default: until none moves)
//   --sweep EPS          gKL2 <in.hgr> -EIG only, not with --k: the sweep cut of
//                        the Fiedler vector under imbalance EPS
//                        (ek_kl_set_partition_fiedler_sweep) instead of the median
//                        split, then the KL loop -> results/<base>.part.2, one
//                        side per line in node order; one line beginning
//                        "sweep:" is printed
//   --sweep-ratio        with --sweep: the ratio cut c / (|A| |B|) instead of the
//                        minimum cut
//   --fm EPS             gKL2 <in.hgr> -EIG only, not with --k, alone or after
//                        --sweep: the bipartition as without it, then the FM
//                        refinement of the sides of KL's best prefix on the
//                        device (ek_fm_refine) with imbalance EPS ->
//                        results/<base>.part.2; one more line beginning "fm:"
//   --fm-passes P        with --fm: at most P counted passes (default: until one
//                        keeps nothing)
//   --fm-stall S         with --fm: a pass ends S moves after its best prefix
//                        (default 1000; 0: it runs until no node can move)
//   --weighted           with --fm: the file is read as hMETIS reads it
//                        (ek_hgr_read_weighted: fmt 0, 1, 10 or 11, '%' comments)
//                        and the refinement is the weighted one (ek_fm_refine_w):
//                        node weights under the bound, net weights in the cut.
//                        Lanczos, the split and KL ignore the weights.  The line
//                        printed begins "fmw:" instead of "fm:"
//   --sweep-weighted     with --sweep, --fm and --weighted, not with
//                        --sweep-ratio: the weighted sweep cut
//                        (ek_kl_set_partition_fiedler_sweep_w: net weights in the
//                        profile, node weights in the window) instead of the count
//                        sweep; the line printed begins "sweepw:" instead of
//                        "sweep:"
//   --no-kl              with --sweep-weighted: no KL graph and no KL loop (KL
//                        swaps pairs and ignores weights, so it can leave the
//                        bound); the sweep's sides go straight to ek_fm_refine_w
//   --multilevel EPS     gKL2 <in.hgr> -EIG only, not with --k, --sweep or --fm:
//                        the multilevel bipartition (ek_multilevel_bipartition_file)
//                        with imbalance EPS on the hMETIS reading of the file:
//                        matching and contraction down to --ml-coarse N nodes
//                        (default 512), the weighted sweep cut of the coarsest
//                        level's Fiedler vector, the weighted FM refinement at
//                        every level (--fm-passes, --fm-stall apply) ->
//                        results/<base>.part.2; one line beginning "ml:"
//   --kway-multilevel EPS  gKL2 <in.hgr> -EIG --k N only, in place of
//                        --multilevel (which keeps refusing --k), not with
//                        --refine: the N-way partition by recursive multilevel
//                        bisection under per-side weight bounds
//                        (ek_partition_kway_ml_file) with imbalance EPS;
//                        --ml-coarse, --ml-weighted-laplacian, --fm-passes and
//                        --fm-stall apply -> results/<base>.part.<N>; one line
//                        beginning "k-way-ml:"
//   --refine-weighted EPS2  with --kway-multilevel: then the weighted k-way
//                        refinement on the device (ek_kway_refine_w) on the same
//                        reading of the file, under the uniform bound
//                        floor((1 + EPS2) ceil(W / N)); --refine-rounds applies;
//                        the refined vector is what results/<base>.part.<N>
//                        holds, and one more line beginning "refine-w:" is
//                        printed
//   --refine-jet EPS2    with --kway-multilevel: then the Jet refinement on the
//                        device (ek_kway_jet, defaults: patience 12, filter 1/4)
//                        on the same reading of the file, under the uniform
//                        bound floor((1 + EPS2) ceil(W / N)); --jet-iters I
//                        limits its iterations; excludes --refine-weighted; the
//                        refined vector is what results/<base>.part.<N> holds,
//                        and one more line beginning "refine-jet:" is printed
//   --kway-direct EPS    gKL2 <in.hgr> -EIG --k N only: the direct k-way
//                        multilevel partition (ek_partition_kway_direct_file) with
//                        imbalance EPS, on the hMETIS reading of the file: one
//                        coarsening, the recursive driver on the coarsest level,
//                        the Jet refinement at every level; --ml-coarse N,
//                        --jet-iters I and --ml-weighted-laplacian apply;
//                        --contract-host contracts on the host; --coarsen
//                        match|cluster chooses the coarsening (the matching by
//                        default, DESIGN.md §20's clustering); excludes every
//                        other partitioner and refinement flag; one line
//                        beginning "kway-direct:", results/<base>.part.<N>
//   --rebalance          with --kway-direct: ek_partition_kway_direct_rb_file, the
//                        rebalancing (ek_kway_rebalance) before the
//                        Jet refinement of every level that starts above the
//                        bound; one more line beginning "rebalance:"
//   --rebalance-to EPS2  with --kway-multilevel: then ek_kway_rebalance under
//                        floor((1 + EPS2) ceil(W / N)), before --refine-jet if
//                        given; excludes --refine-weighted; one more line
//                        beginning "rebalance:"
//   --ml-weighted-laplacian  with --multilevel: the coarsest level's Laplacian
//                        carries its net weights (EK_ML_WEIGHTED_LAPLACIAN,
//                        -(2 c(e) / |e|) per pin pair); the "ml:" line ends
//                        with one more field, "wlap=1"
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstring>
#include <filesystem>
#include <future>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ek_internal.hpp"

// kway.cpp: ek_partition_kway_file with the results file on, for `--k`.  A weak
// reference, so that the host sources still link without the k-way unit (the
// sanitizer harness builds a fixed list of them); --k then fails cleanly.
namespace ek {
int kway_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, ek_kway_result* r)
    __attribute__((weak));
// kway_refine.cpp: the same followed by ek_kway_refine, for `--k N --refine EPS`
int kway_refine_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int max_rounds, ek_kway_result* kr, ek_kway_refine_result* rr) __attribute__((weak));
// sweep.cpp: the bipartition from the sweep cut, for `--sweep EPS`
int sweep_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, int32_t limit, double imbalance,
                       int ratio, ek_sweep_result* sr, ek_kl_result* kr, double* lambda, ek_lanczos_stats* st)
    __attribute__((weak));
// fm.cpp: the bipartition (the sweep's when asked for), then ek_fm_refine, for `--fm EPS`
// (stall < 0: the default)
int fm_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                    double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr, ek_fm_result* fr)
    __attribute__((weak));
// fm.cpp: the same on the hMETIS reading of the file, with ek_fm_refine_w, for `--fm EPS --weighted`
int fmw_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, int sweep, double sweep_eps, int ratio,
                     double imbalance, int max_passes, int stall, ek_sweep_result* sr, ek_kl_result* kr,
                     ek_fm_w_result* fr) __attribute__((weak));
// sweep.cpp: the weighted sweep split (no_kl: without the KL loop), then ek_fm_refine_w, for
// `--sweep EPS --sweep-weighted --fm EPS --weighted [--no-kl]`
// (stall < 0: the default)
int sweepw_file_for_cli(ek_ctx* ctx, const char* path, const ek_solve_opts* so, double sweep_eps, int no_kl,
                        double imbalance, int max_passes, int stall, ek_sweep_w_result* sr, ek_kl_result* kr,
                        ek_fm_w_result* fr) __attribute__((weak));
// multilevel.cpp: ek_multilevel_bipartition_file, for `--multilevel EPS`
// (coarse_nodes <= 0, stall < 0: the defaults)
int ml_file_for_cli(ek_ctx* ctx, const char* path, const ek_lanczos_opts* lanczos, double imbalance, int coarse_nodes,
                    int max_passes, int stall, int32_t flags, ek_ml_result* r) __attribute__((weak));
// kway_ml.cpp: ek_partition_kway_ml_file with the results file on, for `--k N --kway-multilevel EPS`
int kway_ml_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                         int coarse_nodes, int max_passes, int stall, int32_t flags, ek_kway_ml_result* r)
    __attribute__((weak));
// kway_refine_w.cpp: ek_partition_kway_ml on the hMETIS reading of the file, then ek_kway_refine_w, then the
// results file, for `--k N --kway-multilevel EPS --refine-weighted EPS2`
int kway_ml_refine_w_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                  int coarse_nodes, int max_passes, int stall, int32_t flags, double refine_imbalance,
                                  int max_rounds, ek_kway_ml_result* mr, ek_kway_refine_w_result* rr)
    __attribute__((weak));
// kway_jet.cpp: the same with ek_kway_jet in place of ek_kway_refine_w, for
// `--k N --kway-multilevel EPS --refine-jet EPS2`
int kway_ml_jet_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int coarse_nodes, int max_passes, int stall, int32_t flags, double jet_imbalance,
                             int max_iters, ek_kway_ml_result* mr, ek_kway_jet_result* jr) __attribute__((weak));
// kway_direct.cpp: ek_partition_kway_direct_file with the results file on, for `--k N --kway-direct EPS`
// (coarse_nodes <= 0, max_iters <= 0: the defaults)
int kway_direct_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                             int coarse_nodes, int max_iters, int32_t flags, int32_t coarsening, ek_kway_direct_result* r)
    __attribute__((weak));
// kway_direct.cpp: the same through ek_partition_kway_direct_rb_file, for `--k N --kway-direct EPS --rebalance`
int kway_direct_rb_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                int coarse_nodes, int max_iters, int32_t flags, int32_t coarsening,
                                ek_kway_direct_result* r, ek_kway_direct_rb_result* rb) __attribute__((weak));
// kway_rebalance.cpp: ek_partition_kway_ml on the hMETIS reading of the file, then ek_kway_rebalance at
// rb_imbalance, then (jet_imbalance >= 0) ek_kway_jet, then the results file, for `--k N --kway-multilevel EPS
// --rebalance-to EPS2 [--refine-jet EPS3]`
int kway_ml_rebalance_file_for_cli(ek_ctx* ctx, const char* path, int k, const ek_lanczos_opts* lanczos, double imbalance,
                                   int coarse_nodes, int max_passes, int stall, int32_t flags, double rb_imbalance,
                                   double jet_imbalance, int max_iters, ek_kway_ml_result* mr,
                                   ek_kway_rebalance_result* rr, ek_kway_jet_result* jr) __attribute__((weak));
}

namespace {

struct Opts {
    std::string tool, input;
    bool eig = false, quiet = false, have_seed = false, deflate = true, teardown = true;
    int device = 0, ncv = 0;
    int kway = 0;  // --k N (0: the bipartition)
    bool refine = false;  // --refine EPS
    double refine_eps = 0.0;
    int refine_rounds = 0;  // --refine-rounds R (0: no limit)
    bool sweep = false, sweep_ratio = false;  // --sweep EPS, --sweep-ratio
    double sweep_eps = 0.0;
    bool fm = false, fm_sub = false;  // --fm EPS; --fm-passes or --fm-stall seen
    double fm_eps = 0.0;
    int fm_passes = 0, fm_stall = -1;  // (-1: the default)
    bool weighted = false;             // --weighted
    bool sweep_weighted = false, no_kl = false;  // --sweep-weighted, --no-kl
    bool ml = false, ml_sub = false;  // --multilevel EPS; --ml-coarse or --ml-weighted-laplacian seen
    bool ml_wlap = false;             // --ml-weighted-laplacian
    bool kml = false;                 // --kway-multilevel EPS (sets ml and ml_eps too): with --k, the k-way driver
    bool refine_w = false;            // --refine-weighted EPS2 (with --kway-multilevel)
    double refine_w_eps = 0.0;
    bool jet = false, jet_sub = false;  // --refine-jet EPS2 (with --kway-multilevel); --jet-iters seen
    double jet_eps = 0.0;
    int jet_iters = 0;  // --jet-iters I (0: no limit)
    bool kd = false, kd_host = false;  // --kway-direct EPS (with --k); --contract-host (with --kway-direct)
    double kd_eps = 0.0;
    bool kd_coarsen = false;  // --coarsen match|cluster seen (with --kway-direct)
    int kd_cluster = 0;       // EK_COARSEN_MATCH | EK_COARSEN_CLUSTER
    bool rb = false;          // --rebalance (with --kway-direct)
    bool rbt = false;         // --rebalance-to EPS2 (with --kway-multilevel)
    double rbt_eps = 0.0;
    double ml_eps = 0.0;
    int ml_coarse = 0;  // --ml-coarse N (0: the default)
    bool spectra = false;
    int reorth = 0;  // 0: default (partial)
    double tol = 0.0;
    uint64_t seed = 0;
    std::string sign_ref;
};

using clk = std::chrono::steady_clock;
double secs(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

void mkdirs() {
    ::mkdir("results", 0755);
    ::mkdir("pre_saved_EIG", 0755);
}

std::string base_name(const std::string& p) { return std::filesystem::path(p).filename().string(); }

struct Fail {
    std::string msg;
};
void check(int rc, const char* what) {
    if (rc != EK_OK) throw Fail{std::string(what) + ": " + ek_last_error()};
}

// Context creation (HIP runtime + device init) is the slowest fixed cost of
// a short run, so it starts on a helper thread at process start and
// overlaps the .hgr parse and the clique expansions.
struct CtxInit {
    std::thread th;
    ek_ctx* ctx = nullptr;
    int rc = EK_OK;
    std::string err;
    bool teardown = true;  // false: the context is left to the process exit (EK_CLI_NO_TEARDOWN)
    explicit CtxInit(int device, bool td = true) : teardown(td) {
        th = std::thread([this, device] {
            ek::cold_stamp("ctx_init_start");
            rc = ek_init(device, &ctx);
            ek::cold_stamp("ctx_init_done");
            if (rc != EK_OK) err = ek_last_error();
        });
    }
    std::once_flag joined;  // get() is called from the solve's thread and the KL adjacency's
    ek_ctx* get() {
        std::call_once(joined, [this] {
            if (th.joinable()) th.join();
        });
        if (rc != EK_OK) throw Fail{"GPU init: " + err};
        return ctx;
    }
    ~CtxInit() {
        if (th.joinable()) th.join();
        ek::cold_stamp("ctx_destroy_start");
        if (ctx && teardown) ek_destroy(ctx);
        ek::cold_stamp("ctx_destroy_done");
    }
};

struct Phases {  // wall-clock phase log for the non-quiet summary
    std::vector<std::pair<std::string, double>> t;
    clk::time_point last = clk::now();
    void mark(const char* name) {
        t.emplace_back(name, secs(last));
        last = clk::now();
    }
    void print() const {
        std::printf("%-24s:", "Phases (s)");
        for (const auto& p : t) std::printf(" %s %.3f", p.first.c_str(), p.second);
        std::printf("\n");
    }
};

ek_solve_opts solve_opts(const Opts& o) {
    ek_solve_opts so;
    ek_solve_default_opts(&so);
    so.lanczos.deflate = o.deflate ? 1 : 0;
    if (o.ncv > 0) so.lanczos.ncv = o.ncv;
    if (o.tol > 0) so.lanczos.tol = o.tol;
    if (o.spectra) {  // Spectra SymEigsSolver's rule set
        so.lanczos.reorth = 1;
        so.lanczos.keep_min = 0;
        so.lanczos.basis32 = 0;
    }
    if (o.reorth) so.lanczos.reorth = o.reorth;
    so.sign_ref = o.sign_ref.empty() ? nullptr : o.sign_ref.c_str();
    so.seed = o.have_seed ? uint32_t(o.seed) : std::random_device{}();  // cKL.cpp:179-180 when unseeded
    return so;
}

int run_eig(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    Phases ph;
    const std::string outfile = "pre_saved_EIG/" + base_name(o.input) + "_out.txt";
    if (!o.quiet) {
        std::printf("\n============= Initialization =============\n");
        std::printf("Device: HIP gfx950 #%d (libeigkl_hip %s)\n", o.device, ek_version());
    }
    ek_hgr* h = nullptr;
    check(ek_hgr_read(o.input.c_str(), &h), "Error opening input file");
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    int64_t nets = 0, nodes = 0;
    ek_hgr_dims(h, &nets, &nodes, nullptr);
    if (!o.quiet) std::printf("\nProblem Size:\n  - Nets: %lld\n  - Nodes: %lld\n", (long long)nets, (long long)nodes);
    if (!o.quiet) std::printf("\nComputing eigenvalues (GPU Lanczos)...\n");
    ph.mark("read");
    double lambda = 0, tl = 0, tz = 0;
    std::vector<double> v;
    ek_lanczos_stats st{};
    const ek_solve_opts so = solve_opts(o);
    try {
        // the context initialises on its thread while the Laplacian is built
        ek::fiedler_vector(ci.get(), 0, 1, *h, so, lambda, v, st, &tl, &tz);
    } catch (const ek::Error& e) {
        if (e.code == EK_ENOCONV) throw Fail{"Eigenvalue computation failed"};  // cEIG.cpp:200-202
        throw Fail{std::string("Lanczos: ") + ek_last_error()};
    }
    ph.mark("laplacian+lanczos");
    double med = 0;
    std::vector<uint8_t> bits(static_cast<size_t>(nodes));
    check(ek_median_split(nodes, v.data(), &med, bits.data()), "median");
    check(ek_eig_write(outfile.c_str(), nodes, lambda, med, bits.data(), v.data()), "write");
    ph.mark("write");
    if (!o.quiet) {
        ph.print();
        std::printf("  - lambda_1: %.12g  (restarts %d, matvecs %d, residual %.3g, %.3f s on GPU)\n", lambda,
                    st.restarts, st.matvecs, st.residual, st.total_ms / 1000.0);
        std::printf("\n============= Summary =============\n");
        std::printf("Execution time: %.3f seconds\n", secs(t0));
        std::printf("Results written to: %s\n", outfile.c_str());
        std::printf("================================\n\n");
    }
    return 0;
}

int run_kl(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    const std::string base = base_name(o.input);
    if (!o.quiet) std::printf("\n============= Reading Input File ==============\n");
    ek_hgr* h = nullptr;
    check(ek_hgr_read(o.input.c_str(), &h), "Error opening file");
    std::unique_ptr<ek_hgr, void (*)(ek_hgr*)> hg(h, ek_hgr_free);
    const double t_read = secs(t0);
    ek::cold_stamp("read_done");
    int64_t nets = 0, nodes = 0;
    ek_hgr_dims(h, &nets, &nodes, nullptr);
    if (!o.quiet)
        std::printf("Circuit Statistics\n  - Total Nets : %lld\n  - Total Nodes: %lld\n", (long long)nets,
                    (long long)nodes);
    // initial partition (shuffleSparceMatrix, cKL.cpp:151-197): gKL2 -EIG
    // computes the Fiedler split in-process, cKL/gKL -EIG read the EIG file
    ek_solve_opts so = solve_opts(o);
    so.eig = o.eig ? (o.tool == "gKL2" ? 1 : 2) : 0;
    ek_solve_result r{};
    try {
        ek::solve([&ci] { return ci.get(); }, 0, 1, *h, base, so, nullptr, 0, r);
        ek::cold_stamp("solve_done");
    } catch (const ek::Error& e) {
        if (e.code == EK_ENOCONV) throw Fail{"Eigenvalue computation failed"};
        const std::string msg = ek_last_error();
        throw Fail{msg.rfind("Error", 0) == 0 ? msg : "KL: " + msg};
    }
    if (!o.quiet) {
        if (so.eig == 1)
            std::printf("EIG (GPU Lanczos): lambda_1 %.12g, %d matvecs, %.3f s\n", r.lambda, r.lanczos.matvecs,
                        r.lanczos.total_ms / 1000.0);
        std::printf("\n=============== Final Results =================\n");
        std::printf("%-24s: %lld\n", "Total iterations", (long long)r.kl.iterations);
        std::printf("%-24s: %.2f\n", "Initial cut size", double(r.kl.initial_cut));
        std::printf("%-24s: %.2f\n", "Best cut size achieved", double(r.kl.best_cut));
        std::printf("%-24s: %.2f%%\n", "Overall improvement", 100.0 * (1.0 - double(r.kl.best_cut) / double(r.kl.initial_cut)));
        std::printf("%-24s: %lld (iteration %lld)\n", "Net cut @ best prefix", (long long)r.kl.net_cut_best,
                    (long long)r.kl.best_iter);
        std::printf("%-24s: %.3f ms (device)\n", "KL loop", r.kl.loop_ms);
        std::printf("%-24s: %.3f seconds\n", "Total runtime", secs(t0));
        std::printf("%-24s: read %.3f laplacian %.3f lanczos %.3f split %.3f kl-graph-wait %.3f kl-setup %.3f kl %.3f "
                    "write %.3f\n", "Phases (s)", t_read, r.t_laplacian, r.t_lanczos, r.t_split, r.t_kl_graph_wait,
                    r.t_kl_setup, r.t_kl, r.t_write);
    }
    return 0;
}

// gKL2 <in.hgr> -EIG --k N: one summary line, results/<base>.part.<N>
int run_kway(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    const ek_solve_opts so = solve_opts(o);
    if (!ek::kway_file_for_cli) throw Fail{"this build carries no k-way path"};
    ek_kway_result r{};
    ek_kway_refine_result rr{};
    if (o.refine) {
        if (!ek::kway_refine_file_for_cli) throw Fail{"this build carries no k-way refinement"};
        check(ek::kway_refine_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.refine_eps, o.refine_rounds,
                                           &r, &rr), "k-way partition");
    } else
        check(ek::kway_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, &r), "k-way partition");
    std::printf("k-way: k %d, part sizes %lld..%lld, cut nets %lld, connectivity %lld, SOED %lld, %.3f s -> "
                "results/%s.part.%d\n", r.k, (long long)r.part_min, (long long)r.part_max, (long long)r.cut_nets,
                (long long)r.connectivity, (long long)r.soed, secs(t0), base_name(o.input).c_str(), r.k);
    if (o.refine)
        std::printf("refine: imbalance %g (max part %lld), %d rounds, %lld moves, connectivity %lld -> %lld, cut nets "
                    "%lld, SOED %lld, part sizes %lld..%lld, %.3f s\n", o.refine_eps, (long long)rr.max_part, rr.rounds,
                    (long long)rr.moves, (long long)rr.connectivity_before, (long long)rr.connectivity,
                    (long long)rr.cut_nets, (long long)rr.soed, (long long)rr.part_min, (long long)rr.part_max,
                    rr.t_setup + rr.t_rounds + rr.t_metrics);
    return 0;
}

// gKL2 <in.hgr> -EIG --sweep EPS [--sweep-ratio]: one summary line, results/<base>.part.2
int run_sweep(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    const ek_solve_opts so = solve_opts(o);
    if (!ek::sweep_file_for_cli) throw Fail{"this build carries no sweep cut"};
    ek_sweep_result r{};
    ek_kl_result kr{};
    double lambda = 0.0;
    ek_lanczos_stats st{};
    check(ek::sweep_file_for_cli(ci.get(), o.input.c_str(), &so.lanczos, so.limit, o.sweep_eps, o.sweep_ratio ? 1 : 0, &r,
                                 &kr, &lambda, &st), "sweep cut");
    std::printf("sweep: imbalance %g (%s), window %lld..%lld (max part %lld), n1 %lld, cut_mid %lld, cut %lld, "
                "net_cut_best %lld (KL: %lld swaps, best prefix %lld), %.3f s -> results/%s.part.2\n", o.sweep_eps,
                o.sweep_ratio ? "ratio cut" : "minimum cut", (long long)r.s_lo, (long long)r.s_hi, (long long)r.max_part,
                (long long)r.n1, (long long)r.cut_mid, (long long)r.cut, (long long)kr.net_cut_best,
                (long long)kr.iterations, (long long)kr.best_iter, secs(t0), base_name(o.input).c_str());
    return 0;
}

constexpr const char* FM_USAGE =
    "Usage: gKL2 <input_file> -EIG [--sweep <imbalance> [--sweep-ratio]] --fm <imbalance> [--fm-passes <P>] "
    "[--fm-stall <S>]  (--fm needs gKL2 and -EIG, and excludes --k; --fm-passes and --fm-stall need --fm)\n";
constexpr const char* FMW_USAGE =
    "Usage: gKL2 <input_file> -EIG [--sweep <imbalance> [--sweep-ratio]] --fm <imbalance> --weighted [--fm-passes <P>] "
    "[--fm-stall <S>]  (--weighted needs --fm and excludes --k; the file is read as hMETIS reads it, fmt 0, 1, 10 or "
    "11; the FM refinement weighs nodes and nets, while Lanczos, the split and KL ignore the weights)\n";
constexpr const char* SWEEPW_USAGE =
    "Usage: gKL2 <input_file> -EIG --sweep <imbalance> --sweep-weighted --fm <imbalance> --weighted [--no-kl] "
    "[--fm-passes <P>] [--fm-stall <S>]  (--sweep-weighted needs gKL2, -EIG, --sweep, --fm and --weighted, and excludes "
    "--sweep-ratio and --k: the sweep cut weighs nets in its profile and nodes in its window; --no-kl needs "
    "--sweep-weighted: the sweep's sides go to the weighted FM refinement without the KL loop)\n";

// gKL2 <in.hgr> -EIG [--sweep EPS] --fm EPS: the usual output (or the sweep's line), one line beginning "fm:",
// results/<base>.part.2
int run_fm(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    ek_solve_opts so = solve_opts(o);
    so.eig = 1;
    if (!ek::fm_file_for_cli) throw Fail{"this build carries no FM refinement"};
    ek_sweep_result sr{};
    ek_kl_result kr{};
    ek_fm_result fr{};
    auto print_sweep_and_kl = [&] {
        if (o.sweep)
            std::printf("sweep: imbalance %g (%s), window %lld..%lld (max part %lld), n1 %lld, cut_mid %lld, cut %lld\n",
                        o.sweep_eps, o.sweep_ratio ? "ratio cut" : "minimum cut", (long long)sr.s_lo, (long long)sr.s_hi,
                        (long long)sr.max_part, (long long)sr.n1, (long long)sr.cut_mid, (long long)sr.cut);
        std::printf("kl: net_cut_best %lld (%lld swaps, best prefix %lld)\n", (long long)kr.net_cut_best,
                    (long long)kr.iterations, (long long)kr.best_iter);
    };
    if (o.weighted) {
        ek_fm_w_result wr{};
        if (o.sweep_weighted) {
            if (!ek::sweepw_file_for_cli) throw Fail{"this build carries no weighted sweep cut"};
            ek_sweep_w_result wsr{};
            check(ek::sweepw_file_for_cli(ci.get(), o.input.c_str(), &so, o.sweep_eps, o.no_kl ? 1 : 0, o.fm_eps,
                                          o.fm_passes, o.fm_stall, &wsr, &kr, &wr), "weighted sweep cut");
            std::printf("sweepw: imbalance %g, window %lld..%lld (max_part %lld), feasible %lld, n1 %lld, w0 %lld | w1 %lld, "
                        "total_weight %lld, cut_half %lld, cut %lld, cut_nets %lld\n", o.sweep_eps, (long long)wsr.s_lo,
                        (long long)wsr.s_hi, (long long)wsr.max_part, (long long)wsr.feasible, (long long)wsr.n1,
                        (long long)wsr.w0, (long long)wsr.w1, (long long)wsr.total_weight, (long long)wsr.cut_half,
                        (long long)wsr.cut, (long long)wsr.cut_nets);
            if (!o.no_kl)
                std::printf("kl: net_cut_best %lld (%lld swaps, best prefix %lld)\n", (long long)kr.net_cut_best,
                            (long long)kr.iterations, (long long)kr.best_iter);
        } else {
            if (!ek::fmw_file_for_cli) throw Fail{"this build carries no weighted FM refinement"};
            check(ek::fmw_file_for_cli(ci.get(), o.input.c_str(), &so, o.sweep ? 1 : 0, o.sweep_eps, o.sweep_ratio ? 1 : 0,
                                       o.fm_eps, o.fm_passes, o.fm_stall, &sr, &kr, &wr), "weighted FM refinement");
            print_sweep_and_kl();
        }
        std::printf("fmw: imbalance %g, cut_before %lld, cut %lld, cut_nets_before %lld, cut_nets %lld, passes %d, moves "
                    "kept %lld / tried %lld, w0 %lld, w1 %lld, total_weight %lld, max_part %lld, n0 %lld, n1 %lld, %.6f s "
                    "(fmw), %.3f s -> results/%s.part.2\n", o.fm_eps, (long long)wr.cut_before, (long long)wr.cut,
                    (long long)wr.cut_nets_before, (long long)wr.cut_nets, wr.passes, (long long)wr.moves_kept,
                    (long long)wr.moves_tried, (long long)wr.w0, (long long)wr.w1, (long long)wr.total_weight,
                    (long long)wr.max_part, (long long)wr.n0, (long long)wr.n1, wr.t_setup + wr.t_passes + wr.t_metrics,
                    secs(t0), base_name(o.input).c_str());
        return 0;
    }
    check(ek::fm_file_for_cli(ci.get(), o.input.c_str(), &so, o.sweep ? 1 : 0, o.sweep_eps, o.sweep_ratio ? 1 : 0, o.fm_eps,
                              o.fm_passes, o.fm_stall, &sr, &kr, &fr), "FM refinement");
    print_sweep_and_kl();
    std::printf("fm: imbalance %g, cut_before %lld, cut %lld, passes %d, moves kept %lld / tried %lld, n0 %lld, n1 %lld, "
                "max_part %lld, %.6f s (fm), %.3f s -> results/%s.part.2\n", o.fm_eps, (long long)fr.cut_before,
                (long long)fr.cut, fr.passes, (long long)fr.moves_kept, (long long)fr.moves_tried, (long long)fr.n0,
                (long long)fr.n1, (long long)fr.max_part, fr.t_setup + fr.t_passes + fr.t_metrics, secs(t0),
                base_name(o.input).c_str());
    return 0;
}

constexpr const char* ML_USAGE =
    "Usage: gKL2 <input_file> -EIG --multilevel <imbalance> [--ml-coarse <N>] [--fm-passes <P>] [--fm-stall <S>]  "
    "(--multilevel needs gKL2 and -EIG, and excludes --k, --sweep and --fm; --ml-coarse needs --multilevel; the file "
    "is read as hMETIS reads it)\n"
    "Usage: gKL2 <input_file> -EIG --k <parts> --kway-multilevel <imbalance> [--ml-coarse <N>] "
    "[--ml-weighted-laplacian]  (the k-way partition by recursive multilevel bisection; needs --k with 2 <= parts <= "
    "256, excludes --multilevel and --refine)\n"
    "Usage: gKL2 <input_file> -EIG --k <parts> --kway-multilevel <imbalance> --refine-weighted <imbalance> "
    "[--refine-rounds <R>]  (then the weighted k-way refinement under floor((1 + imbalance) ceil(W / parts)); needs "
    "--kway-multilevel; the refine-w: line follows)\n"
    "Usage: gKL2 <input_file> -EIG --k <parts> --kway-multilevel <imbalance> --refine-jet <imbalance> "
    "[--jet-iters <I>]  (then the Jet refinement under floor((1 + imbalance) ceil(W / parts)); needs "
    "--kway-multilevel, excludes --refine-weighted; the refine-jet: line follows)\n"
    "Usage: gKL2 <input_file> -EIG --k <parts> --kway-multilevel <imbalance> --rebalance-to <imbalance> "
    "[--refine-jet <imbalance>]  (then the rebalancing under floor((1 + imbalance) ceil(W / parts)), before the Jet "
    "refinement if any; needs --kway-multilevel, excludes --refine-weighted; the rebalance: line follows)\n"
    "Usage: gKL2 <input_file> -EIG --multilevel <imbalance> --ml-weighted-laplacian  (the coarsest level's Laplacian "
    "carries its net weights, -(2 c(e) / |e|) per pin pair; needs --multilevel; the ml: line ends with wlap=1)\n";

// gKL2 <in.hgr> -EIG --multilevel EPS: one summary line beginning "ml:", results/<base>.part.2
int run_ml(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    const ek_solve_opts so = solve_opts(o);
    if (!ek::ml_file_for_cli) throw Fail{"this build carries no multilevel path"};
    ek_ml_result r{};
    check(ek::ml_file_for_cli(ci.get(), o.input.c_str(), &so.lanczos, o.ml_eps, o.ml_coarse, o.fm_passes, o.fm_stall,
                              o.ml_wlap ? EK_ML_WEIGHTED_LAPLACIAN : 0, &r),
          "multilevel bipartition");
    std::printf("ml: imbalance %g, levels %d, coarsest_nodes %lld, max_cluster %lld, fallback %d, feasible %lld, "
                "coarsest_cut %lld, cut %lld, cut_nets %lld, w0 %lld, w1 %lld, total_weight %lld, max_part %lld, n0 %lld, "
                "n1 %lld, %.3f s (match %.3f, contract %.3f, lanczos %.3f, sweep %.3f, fm %.3f), %.3f s -> "
                "results/%s.part.2%s\n", o.ml_eps, r.levels, (long long)r.nodes[r.levels], (long long)r.max_cluster,
                r.coarsest_fallback, (long long)r.sweep_feasible, (long long)r.cut_before[r.levels], (long long)r.cut,
                (long long)r.cut_nets, (long long)r.w0, (long long)r.w1, (long long)r.total_weight, (long long)r.max_part,
                (long long)r.n0, (long long)r.n1, r.t_total, r.t_match, r.t_contract, r.t_lanczos, r.t_sweep, r.t_fm,
                secs(t0), base_name(o.input).c_str(), o.ml_wlap ? ", wlap=1" : "");
    return 0;
}

// gKL2 <in.hgr> -EIG --k N --kway-multilevel EPS: one summary line beginning "k-way-ml:", results/<base>.part.<N>
int run_kway_ml(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    const ek_solve_opts so = solve_opts(o);
    if (!ek::kway_ml_file_for_cli) throw Fail{"this build carries no multilevel k-way path"};
    ek_kway_ml_result r{};
    ek_kway_refine_w_result rr{};
    ek_kway_jet_result jr{};
    ek_kway_rebalance_result br{};
    if (o.rbt) {
        if (!ek::kway_ml_rebalance_file_for_cli) throw Fail{"this build carries no k-way rebalancing"};
        check(ek::kway_ml_rebalance_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.ml_eps, o.ml_coarse,
                                                 o.fm_passes, o.fm_stall, o.ml_wlap ? EK_ML_WEIGHTED_LAPLACIAN : 0,
                                                 o.rbt_eps, o.jet ? o.jet_eps : -1.0, o.jet_iters, &r, &br, &jr),
              "multilevel k-way partition and rebalancing");
    } else if (o.jet) {
        if (!ek::kway_ml_jet_file_for_cli) throw Fail{"this build carries no Jet refinement"};
        check(ek::kway_ml_jet_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.ml_eps, o.ml_coarse,
                                           o.fm_passes, o.fm_stall, o.ml_wlap ? EK_ML_WEIGHTED_LAPLACIAN : 0, o.jet_eps,
                                           o.jet_iters, &r, &jr),
              "multilevel k-way partition and Jet refinement");
    } else if (o.refine_w) {
        if (!ek::kway_ml_refine_w_file_for_cli) throw Fail{"this build carries no weighted k-way refinement"};
        check(ek::kway_ml_refine_w_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.ml_eps, o.ml_coarse,
                                                o.fm_passes, o.fm_stall, o.ml_wlap ? EK_ML_WEIGHTED_LAPLACIAN : 0,
                                                o.refine_w_eps, o.refine_rounds, &r, &rr),
              "multilevel k-way partition and weighted refinement");
    } else {
        check(ek::kway_ml_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.ml_eps, o.ml_coarse,
                                       o.fm_passes, o.fm_stall, o.ml_wlap ? EK_ML_WEIGHTED_LAPLACIAN : 0, &r),
              "multilevel k-way partition");
    }
    std::printf("k-way-ml: k %d, imbalance %g, bisections %d, fallbacks %d, infeasible %d, total_weight %lld, part_bound "
                "%lld, part weights %lld..%lld, over_bound %lld, empty %lld, cut nets %lld, connectivity %lld, "
                "connectivity_w %lld, SOED %lld, levels %lld, fm_moves %lld, %.3f s (induce %.3f, match %.3f, contract "
                "%.3f, lanczos %.3f, sweep %.3f, fm %.3f, metrics %.3f), %.3f s -> results/%s.part.%d%s\n", r.k, o.ml_eps,
                r.bisections, r.coarsest_fallbacks, r.infeasible_sweeps, (long long)r.total_weight, (long long)r.part_bound,
                (long long)r.part_w_min, (long long)r.part_w_max, (long long)r.parts_over_bound, (long long)r.empty_parts,
                (long long)r.cut_nets, (long long)r.connectivity, (long long)r.connectivity_w, (long long)r.soed,
                (long long)r.levels_total, (long long)r.fm_moves, r.t_total, r.t_induce, r.t_match, r.t_contract,
                r.t_lanczos, r.t_sweep, r.t_fm, r.t_metrics, secs(t0), base_name(o.input).c_str(), r.k,
                o.ml_wlap ? ", wlap=1" : "");
    if (o.refine_w)
        std::printf("refine-w: imbalance %g (bound %lld), %d rounds, %lld moves, connectivity_w %lld -> %lld, cut nets "
                    "%lld, part weights %lld..%lld, over_bound %lld, %.3f s\n", o.refine_w_eps, (long long)rr.bound_max,
                    rr.rounds, (long long)rr.moves, (long long)rr.connectivity_w_before, (long long)rr.connectivity_w,
                    (long long)rr.cut_nets, (long long)rr.part_w_min, (long long)rr.part_w_max,
                    (long long)rr.parts_over_bound, rr.t_setup + rr.t_rounds + rr.t_metrics);
    if (o.rbt)
        std::printf("rebalance: imbalance %g (bound %lld), levels rebalanced %d, %d rounds, %lld moves, excess %lld -> "
                    "%lld, over_bound %lld -> %lld, connectivity_w %lld -> %lld, %.3f s\n", o.rbt_eps,
                    (long long)br.bound_max, br.parts_over_before > 0 ? 1 : 0, br.rounds, (long long)br.moves,
                    (long long)br.excess_before, (long long)br.excess, (long long)br.parts_over_before,
                    (long long)br.parts_over_bound, (long long)br.connectivity_w_before, (long long)br.connectivity_w,
                    br.t_setup + br.t_rounds + br.t_metrics);
    if (o.jet)
        std::printf("refine-jet: imbalance %g (bound %lld), %d iterations, best %d, %lld moves, connectivity_w %lld -> "
                    "%lld, cut nets %lld, part weights %lld..%lld, over_bound %lld, %.3f s\n", o.jet_eps,
                    (long long)jr.bound_max, jr.iters, jr.best_iter, (long long)jr.moves,
                    (long long)jr.connectivity_w_before, (long long)jr.connectivity_w, (long long)jr.cut_nets,
                    (long long)jr.part_w_min, (long long)jr.part_w_max, (long long)jr.parts_over_bound,
                    jr.t_setup + jr.t_iters + jr.t_metrics);
    return 0;
}

constexpr const char* KD_USAGE =
    "Usage: gKL2 <input_file> -EIG --k <parts> --kway-direct <imbalance> [--ml-coarse <N>] [--jet-iters <I>] "
    "[--contract-host] [--ml-weighted-laplacian] [--coarsen match|cluster] [--rebalance]  (the direct k-way multilevel partition: one "
    "coarsening, the Jet refinement at every level; needs --k with 2 <= parts <= 256 and an imbalance >= 0; excludes "
    "--kway-multilevel, --multilevel, --refine, --refine-weighted, --refine-jet, --sweep and --fm; --contract-host "
    "contracts on the host; --coarsen cluster coarsens by multi-node clustering, match (the default) by matching; "
    "--rebalance rebalances a level that starts above the bound before its Jet refinement, and the rebalance: line "
    "follows; the file is read as hMETIS reads it)\n";

// gKL2 <in.hgr> -EIG --k N --kway-direct EPS: one summary line beginning "kway-direct:", results/<base>.part.<N>
int run_kway_direct(const Opts& o) {
    const auto t0 = clk::now();
    CtxInit ci(o.device, o.teardown);
    const ek_solve_opts so = solve_opts(o);
    if (!ek::kway_direct_file_for_cli) throw Fail{"this build carries no direct k-way path"};
    ek_kway_direct_result r{};
    ek_kway_direct_rb_result rb{};
    const int32_t flags = (o.kd_host ? EK_KWAY_DIRECT_HOST_CONTRACT : 0) | (o.ml_wlap ? EK_KWAY_DIRECT_WEIGHTED_LAPLACIAN : 0);
    if (o.rb) {
        if (!ek::kway_direct_rb_file_for_cli) throw Fail{"this build carries no k-way rebalancing"};
        check(ek::kway_direct_rb_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.kd_eps, o.ml_coarse,
                                              o.jet_iters, flags, o.kd_cluster, &r, &rb),
              "direct k-way partition with rebalancing");
    } else {
        check(ek::kway_direct_file_for_cli(ci.get(), o.input.c_str(), o.kway, &so.lanczos, o.kd_eps, o.ml_coarse,
                                           o.jet_iters, flags, o.kd_cluster, &r),
              "direct k-way partition");
    }
    long long iters = 0, moves = 0;
    for (int l = 0; l <= r.levels; ++l) {
        iters += r.jet_iters[l];
        moves += r.jet_moves[l];
    }
    std::printf("kway-direct: k %d, imbalance %g, levels %d, coarsest_nodes %lld, max_cluster %lld, fallbacks %d, "
                "infeasible %d, total_weight %lld, part_bound %lld, part weights %lld..%lld, over_bound %lld, empty %lld, "
                "cut nets %lld, connectivity %lld, connectivity_w %lld (initial %lld), SOED %lld, jet iterations %lld, "
                "jet moves %lld, contract %s, coarsen %s, %.3f s (match %.3f, contract %.3f, initial %.3f, jet %.3f, metrics %.3f), "
                "%.3f s -> results/%s.part.%d%s\n", r.k, o.kd_eps, r.levels, (long long)r.nodes[r.levels],
                (long long)r.max_cluster, r.initial_fallbacks, r.infeasible_sweeps, (long long)r.total_weight,
                (long long)r.part_bound, (long long)r.part_w_min, (long long)r.part_w_max, (long long)r.parts_over_bound,
                (long long)r.empty_parts, (long long)r.cut_nets, (long long)r.connectivity, (long long)r.connectivity_w,
                (long long)r.conn_w_before[r.levels], (long long)r.soed, iters, moves, o.kd_host ? "host" : "device",
                o.kd_cluster == EK_COARSEN_CLUSTER ? "cluster" : "match", r.t_total, r.t_match, r.t_contract, r.t_initial, r.t_jet, r.t_metrics, secs(t0),
                base_name(o.input).c_str(), r.k, o.ml_wlap ? ", wlap=1" : "");
    if (o.rb) {
        long long levels = 0, rounds = 0, rmoves = 0;
        for (int l = 0; l <= r.levels; ++l) {
            levels += rb.over_before[l] > 0;
            rounds += rb.rb_rounds[l];
            rmoves += rb.rb_moves[l];
        }
        std::printf("rebalance: levels rebalanced %lld, %lld rounds, %lld moves, excess left %lld, %.3f s\n", levels,
                    rounds, rmoves, (long long)rb.excess_after[0], rb.t_rebalance);
    }
    return 0;
}

}  // namespace

extern "C" int ek_cli_main(const char* tool_c, int argc, char** argv) {
    return ek_cli_main_ex(tool_c, argc, argv, 0);
}

extern "C" int ek_cli_main_ex(const char* tool_c, int argc, char** argv, int flags) {
    ek::cold_stamp("main");
    Opts o;
    o.tool = tool_c ? tool_c : "cKL";
    o.teardown = !(flags & EK_CLI_NO_TEARDOWN);
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* flag) -> std::string {
            if (i + 1 >= argc) throw Fail{std::string("missing value for ") + flag};
            return argv[++i];
        };
        try {
            if (a == "--device") o.device = std::stoi(need("--device"));
            else if (a == "--seed") {
                o.seed = std::stoull(need("--seed"));
                o.have_seed = true;
            } else if (a == "--sign-ref") o.sign_ref = need("--sign-ref");
            else if (a == "--no-deflate") o.deflate = false;
            else if (a == "--ncv") o.ncv = std::stoi(need("--ncv"));
            else if (a == "--tol") o.tol = std::stod(need("--tol"));
            else if (a == "--quiet") o.quiet = true;
            else if (a == "--k") {
                o.kway = std::stoi(need("--k"));
                if (o.kway < 2) throw Fail{"--k takes a part count of at least 2"};
            }
            else if (a == "--refine") {
                o.refine_eps = std::stod(need("--refine"));
                o.refine = true;
                if (!std::isfinite(o.refine_eps) || o.refine_eps < 0) throw Fail{"--refine takes an imbalance >= 0"};
            } else if (a == "--refine-rounds") o.refine_rounds = std::stoi(need("--refine-rounds"));
            else if (a == "--refine-weighted") {
                o.refine_w = true;  // (before the value: a missing or bad one ends in the usage text below)
                o.refine_w_eps = std::stod(need("--refine-weighted"));
                if (!std::isfinite(o.refine_w_eps) || o.refine_w_eps < 0)
                    throw Fail{"--refine-weighted takes an imbalance >= 0"};
            }
            else if (a == "--refine-jet") {
                o.jet = true;  // (before the value, as --refine-weighted)
                o.jet_eps = std::stod(need("--refine-jet"));
                if (!std::isfinite(o.jet_eps) || o.jet_eps < 0) throw Fail{"--refine-jet takes an imbalance >= 0"};
            } else if (a == "--jet-iters") {
                o.jet_sub = true;
                o.jet_iters = std::stoi(need("--jet-iters"));
            }
            else if (a == "--sweep") {
                o.sweep_eps = std::stod(need("--sweep"));
                o.sweep = true;
                if (!std::isfinite(o.sweep_eps) || o.sweep_eps < 0) throw Fail{"--sweep takes an imbalance >= 0"};
            } else if (a == "--sweep-ratio") o.sweep_ratio = true;
            else if (a == "--fm") {
                o.fm_eps = std::stod(need("--fm"));
                o.fm = true;
                if (!std::isfinite(o.fm_eps) || o.fm_eps < 0) throw Fail{"--fm takes an imbalance >= 0"};
            } else if (a == "--fm-passes") {
                o.fm_passes = std::stoi(need("--fm-passes"));
                o.fm_sub = true;
            } else if (a == "--fm-stall") {
                o.fm_stall = std::stoi(need("--fm-stall"));
                o.fm_sub = true;
                if (o.fm_stall < 0) throw Fail{"--fm-stall takes a move count >= 0"};
            }
            else if (a == "--weighted") o.weighted = true;
            else if (a == "--sweep-weighted") o.sweep_weighted = true;
            else if (a == "--no-kl") o.no_kl = true;
            else if (a == "--multilevel") {
                if (o.kml) throw Fail{"--kway-multilevel stands in place of --multilevel"};
                o.ml_eps = std::stod(need("--multilevel"));
                o.ml = true;
                if (!std::isfinite(o.ml_eps) || o.ml_eps < 0) throw Fail{"--multilevel takes an imbalance >= 0"};
            } else if (a == "--kway-multilevel") {
                if (o.ml && !o.kml) throw Fail{"--kway-multilevel stands in place of --multilevel"};
                o.ml_eps = std::stod(need("--kway-multilevel"));
                o.ml = o.kml = true;
                if (!std::isfinite(o.ml_eps) || o.ml_eps < 0) throw Fail{"--kway-multilevel takes an imbalance >= 0"};
            } else if (a == "--kway-direct") {
                o.kd = true;  // (before the value, as --refine-weighted)
                o.kd_eps = std::stod(need("--kway-direct"));
                if (!std::isfinite(o.kd_eps) || o.kd_eps < 0) throw Fail{"--kway-direct takes an imbalance >= 0"};
            } else if (a == "--contract-host") o.kd_host = true;
            else if (a == "--rebalance") o.rb = true;
            else if (a == "--rebalance-to") {
                o.rbt = true;  // (before the value, as --refine-weighted)
                o.rbt_eps = std::stod(need("--rebalance-to"));
                if (!std::isfinite(o.rbt_eps) || o.rbt_eps < 0) throw Fail{"--rebalance-to takes an imbalance >= 0"};
            }
            else if (a == "--coarsen") {
                o.kd_coarsen = true;  // (before the value, as --refine-weighted)
                const std::string v = need("--coarsen");
                if (v == "match") o.kd_cluster = EK_COARSEN_MATCH;
                else if (v == "cluster") o.kd_cluster = EK_COARSEN_CLUSTER;
                else throw Fail{"--coarsen takes match or cluster"};
            }
            else if (a == "--ml-coarse") {
                o.ml_coarse = std::stoi(need("--ml-coarse"));
                o.ml_sub = true;
                if (o.ml_coarse < 1) throw Fail{"--ml-coarse takes a node count of at least 1"};
            } else if (a == "--ml-weighted-laplacian") o.ml_wlap = o.ml_sub = true;
            else if (a == "--spectra") o.spectra = true;
            else if (a == "--reorth") {
                const std::string v = need("--reorth");
                if (v == "full") o.reorth = 1;
                else if (v == "partial") o.reorth = 3;
                else throw Fail{"--reorth takes full or partial"};
            }
            else pos.push_back(a);
        } catch (const Fail& e) {
            std::fprintf(stderr, "Error: %s\n", e.msg.c_str());
            if (a.rfind("--fm", 0) == 0) std::printf("%s", FM_USAGE);
            if (a.rfind("--m", 0) == 0 || a == "--kway-multilevel" || a == "--refine-weighted" || a == "--refine-jet" ||
                a == "--jet-iters" || a == "--rebalance-to")
                std::printf("%s", ML_USAGE);
            if (a == "--kway-direct" || a == "--coarsen") std::printf("%s", KD_USAGE);
            return 1;
        } catch (...) {
            std::fprintf(stderr, "Error: bad value for %s\n", a.c_str());
            if (a.rfind("--fm", 0) == 0) std::printf("%s", FM_USAGE);
            if (a.rfind("--m", 0) == 0 || a == "--kway-multilevel" || a == "--refine-weighted" || a == "--refine-jet" ||
                a == "--jet-iters" || a == "--rebalance-to")
                std::printf("%s", ML_USAGE);
            if (a == "--kway-direct" || a == "--coarsen") std::printf("%s", KD_USAGE);
            return 1;
        }
    }
    try {
        // the direct k-way path: refused with any other partitioner or refinement; --rebalance needs it
        if (o.kd || o.kd_host || o.kd_coarsen || o.rb) {
            if (!o.kd || o.rbt || o.kway < 2 || o.kway > 256 || o.ml || o.kml || o.refine || o.refine_w || o.jet || o.sweep ||
                o.sweep_ratio || o.fm || o.fm_sub || o.weighted || o.sweep_weighted || o.no_kl || o.tool != "gKL2" ||
                !(pos.size() == 2 && pos[1] == "-EIG")) {
                std::printf("%s", KD_USAGE);
                return 1;
            }
            mkdirs();
            o.input = pos[0];
            o.eig = true;
            return run_kway_direct(o);
        }
        if (o.refine_w && !o.kml) {  // --refine-weighted follows --kway-multilevel only
            std::printf("%s", ML_USAGE);
            return 1;
        }
        if (o.rbt && (!o.kml || o.refine_w)) {  // --rebalance-to follows --kway-multilevel only
            std::printf("%s", ML_USAGE);
            return 1;
        }
        // --refine-jet follows --kway-multilevel only and stands in place of --refine-weighted; --jet-iters needs it
        if ((o.jet || o.jet_sub) && (!o.jet || !o.kml || o.refine_w)) {
            std::printf("%s", ML_USAGE);
            return 1;
        }
        if (o.ml || o.ml_sub) {
            if (!o.ml || (o.kml ? o.kway < 2 || o.kway > 256 : o.kway != 0) || o.refine || o.sweep || o.sweep_ratio || o.fm || o.weighted || o.sweep_weighted ||
                o.no_kl || o.tool != "gKL2" || !(pos.size() == 2 && pos[1] == "-EIG")) {
                std::printf("%s", ML_USAGE);
                return 1;
            }
            mkdirs();
            o.input = pos[0];
            o.eig = true;
            return o.kml ? run_kway_ml(o) : run_ml(o);
        }
        if ((o.sweep_weighted || o.no_kl) &&
            (!o.sweep_weighted || !o.sweep || !o.fm || !o.weighted || o.sweep_ratio || o.kway || o.tool != "gKL2" ||
             !(pos.size() == 2 && pos[1] == "-EIG"))) {
            std::printf("%s", SWEEPW_USAGE);
            return 1;
        }
        if ((o.sweep || o.sweep_ratio) && o.tool != "gKL2") {
            std::printf("Usage: gKL2 <input_file> -EIG --sweep <imbalance> [--sweep-ratio]  (--sweep needs gKL2)\n");
            return 1;
        }
        if (o.weighted && (!o.fm || o.kway || o.tool != "gKL2")) {
            std::printf("%s", FMW_USAGE);
            return 1;
        }
        if ((o.fm || o.fm_sub) && o.tool != "gKL2") {
            std::printf("%s", FM_USAGE);
            return 1;
        }
        if (o.tool == "cEIG") {
            mkdirs();  // cEIG.cpp:148-149
            if (pos.size() != 1) throw Fail{"Usage: ./EIG <input_file>"};
            o.input = pos[0];
            return run_eig(o);
        }
        mkdirs();  // cKL.cpp:428-429
        if (pos.empty() || pos.size() > 2) {
            std::printf("Usage: %s <input_file> [-EIG]\n", argc > 0 ? argv[0] : o.tool.c_str());
            return 1;
        }
        o.input = pos[0];
        o.eig = pos.size() == 2 && pos[1] == "-EIG";
        if (o.refine && !o.kway) {
            std::printf("Usage: gKL2 <input_file> -EIG --k <parts> --refine <imbalance>  (--refine needs --k)\n");
            return 1;
        }
        if (o.fm || o.fm_sub) {
            if (!o.fm || o.kway || !o.eig || (o.sweep_ratio && !o.sweep)) {
                std::printf("%s", FM_USAGE);
                return 1;
            }
            return run_fm(o);
        }
        if (o.sweep || o.sweep_ratio) {
            if (!o.sweep || o.kway || o.tool != "gKL2" || !o.eig) {
                std::printf("Usage: gKL2 <input_file> -EIG --sweep <imbalance> [--sweep-ratio]  (--sweep needs gKL2 and "
                            "-EIG, and excludes --k; --sweep-ratio needs --sweep)\n");
                return 1;
            }
            return run_sweep(o);
        }
        if (o.kway) {
            if (o.tool != "gKL2" || !o.eig) {
                std::printf("Usage: gKL2 <input_file> -EIG --k <parts>  (--k needs gKL2 and -EIG)\n");
                return 1;
            }
            return run_kway(o);
        }
        return run_kl(o);
    } catch (const Fail& e) {
        std::fprintf(stderr, e.msg.rfind("Error", 0) == 0 ? "%s\n" : "Error: %s\n", e.msg.c_str());
        return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error occurred: %s\n", e.what());
        return 1;
    }
}
