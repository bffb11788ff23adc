// The implicitly restarted Lanczos driver of libeigkl_hip.so (Spectra's
// SymEigsSolver restated; host code over the HIP runtime + RCCL).
#include "ctx.hpp"

#ifndef EK_UPD_RED_MAX_NRB
#define EK_UPD_RED_MAX_NRB 256  // row blocks up to which the update workgroups sum the partials themselves
#endif

using namespace ek::rt;

extern "C" {

// ---------------------------------------------------------------------------
// Lanczos (Spectra SymEigsSolver restated, cEIG.cpp:194-207)
void ek_lanczos_default_opts(ek_lanczos_opts* o) {
    if (!o) return;
    o->ncv = 0;
    o->maxit = 1000;
    o->tol = 1e-10;
    o->deflate = 1;
    o->time_spmv = 0;
    o->reorth = 3;
    o->check_every = 8;
    o->basis32 = 1;
    o->alpha_last = 0;
    o->keep_min = -1;
    o->reorth_thresh = 0.0;
}

}  // extern "C"

namespace {

// Spectra SymEigsBase::nev_adjusted (ARPACK dsaup2's count of converged
// unwanted values).  "Converged" = |last component| < machine epsilon: with
// the 10 x DBL_MIN bound (an exact-zero test) the restarts kept 50 vectors
// and ibm10 took 11,006 matvecs instead of 1,201, the 1x synthetic 2,683
// instead of 507 (tools/lanczos_trace.py)
// arpack_half: ARPACK's (and Spectra's) jump to ncv/2 kept vectors when
// nothing else counts (false: the caller's floor decides instead)
int nev_adjusted(int nev, int ncv, int nconv, const std::vector<double>& est, bool arpack_half = true) {
    const double eps = std::numeric_limits<double>::epsilon();
    int nev_new = nev;
    for (int i = nev; i < ncv; ++i)
        if (std::fabs(est[size_t(i)]) < eps) ++nev_new;
    nev_new += std::min(nconv, (ncv - nev_new) / 2);
    if (arpack_half && nev_new == 1 && ncv >= 6) nev_new = ncv / 2;
    else if (arpack_half && nev_new == 1 && ncv > 2) nev_new = 2;
    if (nev_new > ncv - 1) nev_new = ncv - 1;
    return nev_new;
}

struct Lanczos {
    ek_ctx* c;
    hipStream_t s;
    int m, ldv, nrb, nub, has_u0, nreal;
    double u0val;
    bool time_spmv;
    std::vector<hipEvent_t> ev;
    double spmv_ms = 0.0;
    int spmv_timed = 0, matvecs = 0;

    double* V() { return c->V.as<double>(); }
    double* col(int j) { return V() + size_t(j) * ldv; }

    // x for the matvec: the full vector (gathered when sharded, in the padded
    // slot layout the matrix's columns were remapped to)
    const double* gather_f() {
        if (!c->mr) return c->f.as<double>();
        if (c->halo) {
            halo_exchange(c, c->f.as<double>(), s);
            return c->hx_X.as<double>();
        }
        allgather(c, c->f.as<double>(), size_t(c->slot), c->xfull.as<double>());
        return c->xfull.as<double>();
    }

    void reduce_scalar(double* dst) {  // dst = allreduce(sum npart[0:nub])
        ek::dev::finalize_step(s, c->npart.as<double>(), nub, dst, nullptr, nullptr, -1, nullptr, nullptr);
        allreduce(c, dst, 1);
    }

    // Lanczos steps i = k .. m-1 (Spectra Lanczos::factorize_from), with the
    // deflated constant vector u0 in every projection.
    //   reorth 1: three-term recurrence f' = w - alpha v_i - beta_i v_{i-1}
    //             (alpha from the SpMV's fused partials), then ONE classical
    //             Gram-Schmidt pass f = f' - V (V^T f'): 2 passes over V;
    //   reorth 2: CGS2 from w (twice is enough): 4 passes over V.
    // H(i,i) / H(i-1,i) take the projections as corrections (Spectra's
    // H += V^T f after its re-orthogonalisation).
    int reorth = 1;
    // the update reads the fp32 shadow V32 (single-context fused step; k_update B32)
    bool b32 = false;
    // alpha reduced by the SpMV's last workgroup (else by every projection workgroup)
    bool alpha_last = true;
    // the basis passes read V (and V32) non-temporally: a basis larger than
    // the MALL would otherwise evict the matrix and x every pass
    bool nt = false;
    int u32_steps = 0;
    // partial reorthogonalisation (reorth 3, single context): k_pro decides
    // per step whether the projection and the update run (Simon's omega
    // recurrence against thresh; eps1 = eps sqrt(n), its rounding term)
    bool pro = false;
    double pro_thresh = 0.0, pro_eps1 = 0.0;
    int pro_cgw = 0;  // ProLaunch::cgw (EK_PRO_CGW)
    bool pro_cgw_env = false;  // EK_PRO_CGW set: no fitting to the resident grid
    // the decision inside the projection launch (no k_pro launch; needs the
    // projection's hand-off, upd_red 2).  EK_PRO_INLAUNCH=0: the k_pro launch
    bool proi = false;
    // ... and the update's workgroups in the projection launch (no update
    // launch: a skipped step is two launches).  EK_PRO_MERGE=0: its own launch
    bool pro_merge = false;
    unsigned* pro_pub() { return reinterpret_cast<unsigned*>(c->pflags.as<char>() + pro_pub_off()); }
    size_t pro_pub_off() const { return (size_t(m + 2) * 4 + 255) / 256 * 256; }
    float* V32() { return b32 ? c->V32.as<float>() : nullptr; }
    float* col32(int j) { return b32 ? c->V32.as<float>() + size_t(j) * ldv : nullptr; }
    int seg0 = 0;  // first step of the current run of steps (cycle start or injected vector)
    // a mid-cycle check wanted at the end of the next factorize() chunk
    // (chk_dst != null): factorize_fused folds its copy into the chunk's last
    // SpMV (StepFin::chk_*) and sets chk_folded; other forms leave it to the
    // k_chk_gather launch
    double* chk_dst = nullptr;
    unsigned* chk_word = nullptr;
    const unsigned* chk_seq_src = nullptr;
    int chk_b = 0;
    bool chk_folded = false;
    // steps [k, kend) of a run that started at seg0 (the driver enqueues a
    // cycle in chunks to check convergence between them)
    void factorize(int k, int kend) {
        // EK_LANCZOS_UNFUSED: run the sharded step sequence on one GPU (tests)
        static const bool unfused = env_set("EK_LANCZOS_UNFUSED");
        if (reorth == 1) {
            if (!c->mr && !unfused) return graphs && !time_spmv ? factorize_graph(k, kend) : factorize_fused(k, kend);
            if (pro) return factorize_mr_pro(k, kend);
            return factorize_mr(k, kend);
        }
        double* fn2 = c->fn2.as<double>();
        for (int i = k; i < kend; ++i) {  // reorth 2: CGS2 from the matvec
            const double* x = gather_f();
            const bool timed = spmv_timed_step(i);
            ek::dev::spmv(s, spmv_mat(c), x, c->w.as<double>(), fn2 + i, c->f.as<double>(), col(i), nullptr, nullptr,
                          timed ? ev[size_t(2 * (i - seg0))] : nullptr, timed ? ev[size_t(2 * (i - seg0) + 1)] : nullptr);
            ++matvecs;
            const int nc = i + 1, tot = nc + has_u0;
            ek::dev::gemvt(s, ldv, nrb, V(), nc, has_u0, u0val, nreal, c->w.as<double>(), c->part.as<double>());
            ek::dev::reduce_cols(s, c->part.as<double>(), nrb, tot, c->h1.as<double>());
            allreduce(c, c->h1.as<double>(), size_t(tot));
            ek::dev::update(s, ldv, V(), nc, has_u0, u0val, nreal, c->h1.as<double>(), c->w.as<double>(),
                            c->f.as<double>(), nullptr);
            ek::dev::gemvt(s, ldv, nrb, V(), nc, has_u0, u0val, nreal, c->f.as<double>(), c->part.as<double>());
            ek::dev::reduce_cols(s, c->part.as<double>(), nrb, tot, c->h2.as<double>());
            allreduce(c, c->h2.as<double>(), size_t(tot));
            ek::dev::update(s, ldv, V(), nc, has_u0, u0val, nreal, c->h2.as<double>(), c->f.as<double>(),
                            c->f.as<double>(), c->npart.as<double>());
            ek::dev::finalize_step(s, c->npart.as<double>(), nub, fn2 + i + 1, c->h1.as<double>(),
                                   c->h2.as<double>(), i, c->alpha.as<double>(), c->offd.as<double>());
            allreduce(c, fn2 + i + 1, 1);
        }
        HIPCHK(hipGetLastError());
    }

    // The sharded step (reorth 1), ONE all-gather and ONE all-reduce:
    //  1. the rank's ||f||^2 partial goes into its all-gather slot (f[ldv]);
    //  2. all-gather f -> x (every rank's rows + every rank's ||f||^2);
    //  3. SpMV on the owned rows; its prologue sums the ranks' ||f||^2 in rank
    //     order (the same bits on every rank): w = L f/||f||, v_i = f/||f||;
    //  4. gemvt3: V^T w, V^T v_i, V^T v_{i-1} in one sweep of V;
    //  5. ONE all-reduce of the three column-sum vectors;
    //  6. update_mr: alpha = (V^T w)_i, f' = w - alpha v_i - beta v_{i-1},
    //     h = V^T w - alpha V^T v_i - beta V^T v_{i-1} (= V^T f'),
    //     f = f' - V h, and H's alpha[i], offd[i].
    // The single-GPU step reduces alpha before forming f' and projects f'
    // itself (two dependent reductions); here V^T f' comes from the linearity
    // of the projection, computed from the same sweep, so its error is
    // eps ||w|| instead of eps ||f'|| (the orthogonality of f to V is then a
    // few ulps x ||w||/||f||; it does not compound, because f' is still formed
    // by direct subtraction).  Not bit-identical to the single-GPU step; within
    // the Fiedler tolerances on every golden (tests).
    // overlap (sharded): the owned-slot SpMV runs on the context stream while
    // the all-gather runs on gstream; the halo SpMV then starts from its sums
    bool overlap = false;
    // The exchange of one sharded step: this rank's ||f||^2 partial (from the
    // update's npart) into its slot, f to every rank, and the SpMV's
    // prologue operands in fin (the ranks' partials, in rank order; with the
    // overlap, the owned slot's rows summed while the all-gather runs).
    // Returns the x the SpMV reads.
    const double* exchange_f(int i, ek::dev::StepFin& fin) {
        double* f = c->f.as<double>();
        ek::dev::finalize_step(s, c->npart.as<double>(), nub, f + ldv, nullptr, nullptr, -1, nullptr, nullptr);
        const double* x = f;
        if (c->halo) {  // only the rows each rank reads, into the compact x (its partials inside)
            if (overlap) {
                HIPCHK(hipEventRecord(c->ag_ev[0], s));
                HIPCHK(hipStreamWaitEvent(c->gstream, c->ag_ev[0], 0));
                ek::dev::spmv(s, own_mat(c), f, c->yown.as<double>(), nullptr, nullptr, nullptr, nullptr);
                halo_exchange(c, f, c->gstream);
                HIPCHK(hipEventRecord(c->ag_ev[1], c->gstream));
                HIPCHK(hipStreamWaitEvent(s, c->ag_ev[1], 0));
                fin.own_lo = int(c->hx_base[size_t(c->rank)]);
                fin.own_hi = int(c->hx_base[size_t(c->rank)] + c->nrows);
                fin.ybase = c->yown.as<double>();
            } else {
                halo_exchange(c, f, s);
            }
            x = c->hx_X.as<double>();
            fin.npart = x;  // the ranks' partials at their block ends
            fin.nidx = c->hx_pidx.as<int>();
            fin.nb = c->nranks;
            fin.nstride = 1;
            fin.fn2_out = c->fn2.as<double>() + i;
            return x;
        }
        if (c->mr && overlap) {
            // f (with this rank's ||f||^2 partial at f[ldv]) is final: the
            // all-gather goes out on gstream, and the owned slot's rows are
            // summed meanwhile (unscaled: ||f|| comes with the all-gather)
            HIPCHK(hipEventRecord(c->ag_ev[0], s));
            HIPCHK(hipStreamWaitEvent(c->gstream, c->ag_ev[0], 0));
            ek::dev::spmv(s, own_mat(c), f, c->yown.as<double>(), nullptr, nullptr, nullptr, nullptr);
            allgather(c, f, size_t(c->slot), c->xfull.as<double>(), c->gstream);
            HIPCHK(hipEventRecord(c->ag_ev[1], c->gstream));
            HIPCHK(hipStreamWaitEvent(s, c->ag_ev[1], 0));
            x = c->xfull.as<double>();
            fin.own_lo = int(c->rank * c->slot);
            fin.own_hi = int(c->rank * c->slot + c->nrows);
            fin.ybase = c->yown.as<double>();
        } else if (c->mr) {
            allgather(c, f, size_t(c->slot), c->xfull.as<double>());
            x = c->xfull.as<double>();
        }
        fin.npart = x + ldv;
        fin.nb = c->nranks;
        fin.nstride = int(c->slot);
        fin.fn2_out = c->fn2.as<double>() + i;
        return x;
    }

    void factorize_mr(int k, int kend) {
        double* fn2 = c->fn2.as<double>();
        double* f = c->f.as<double>();
        for (int i = k; i < kend; ++i) {
            ek::dev::StepFin fin;
            const double* x = exchange_f(i, fin);
            const bool timed = spmv_timed_step(i);
            ek::dev::spmv(s, spmv_mat(c), x, c->w.as<double>(), nullptr, f, col(i), nullptr, &fin,
                          timed ? ev[size_t(2 * (i - seg0))] : nullptr, timed ? ev[size_t(2 * (i - seg0) + 1)] : nullptr);
            ++matvecs;
            const int nc = i + 1, tot = nc + has_u0;
            ek::dev::gemvt3(s, ldv, nrb, V(), nc, has_u0, u0val, nreal, c->w.as<double>(), col(i),
                            i > 0 ? col(i - 1) : col(i), c->part.as<double>());
            // (+ ||w||^2: the cancellation test of update_mr)
            ek::dev::reduce_cols(s, c->part.as<double>(), nrb, 3 * tot + 1, c->h2.as<double>());
            allreduce(c, c->h2.as<double>(), size_t(3 * tot + 1));
            ek::dev::update_mr(s, ldv, V(), nc, has_u0, u0val, nreal, c->h2.as<double>(), c->w.as<double>(), col(i),
                               i > 0 ? col(i - 1) : nullptr, fn2 + i, c->bov.as<double>() + i, f,
                               c->npart.as<double>(), c->alpha.as<double>(), c->offd.as<double>(),
                               c->cflag.as<double>(), mr_cancel);
        }
        if (kend == m) reduce_scalar(fn2 + m);  // the cycle's last residual norm
        HIPCHK(hipGetLastError());
    }

    // The sharded step under partial reorthogonalisation (reorth 3; VERDICT
    // r4 next-3).  The single-context PRO step needs alpha_i and ||w||^2
    // before it decides, and the decision before it projects, so the step has
    // two reductions:
    //  1. exchange_f: the all-gather of f (every rank's ||f||^2 partial with it);
    //  2. SpMV: w = L f/||f||, v_i, and per-block partials of alpha and ||w||^2;
    //  3. this rank's (alpha, ||w||^2) -> ONE all-reduce of 2 doubles;
    //  4. k_pro on the global sums: Simon's omega recurrence runs replicated on
    //     every rank (the same alpha, T and state everywhere: the same decision);
    //  5. the projection of f' = w - alpha v_i - beta v_{i-1} (f' formed per row
    //     and stored to f; on a skipped step only that, and ||f'||^2);
    //  6. ONE all-reduce of the column sums h (+ ||f'||^2): issued on every step,
    //     since the host cannot see the device's decision without waiting for
    //     it; a skipped step's kernels have no basis pass and its h entries
    //     the finalize reads are exact zeros;
    //  7. the update f = f' - V h (a skipped step: nothing; ||f||^2 = ||f'||^2
    //     reaches the next SpMV as one global value).
    // A skipped step is the all-gather, the SpMV, two small all-reduces and no
    // pass over V; a projecting one adds the two basis passes (the sharded
    // reorth-1 step always made them, through k_gemvt3 / k_update_mr).  f' is
    // projected directly (not by linearity as in factorize_mr), so there is no
    // cancellation to repair.  H's alpha[i] / offd[i] are written by step i+1's
    // SpMV prologue (the single-context lag) or the cycle's closing finalize.
    void factorize_mr_pro(int k, int kend) {
        double* fn2 = c->fn2.as<double>();
        double* f = c->f.as<double>();
        double* a3 = c->scal.as<double>() + 2;
        double* fast = c->scal.as<double>() + 4;  // ||f||^2 of a skipped step for the next SpMV (NaN: the partials)
        double* aw = c->scal.as<double>() + 6;    // (alpha, ||w||^2): this rank's, then all-reduced
        const double* bov = c->bov.as<double>();
        double* h2 = c->h2.as<double>();
        for (int i = k; i < kend; ++i) {
            ek::dev::StepFin fin;
            const double* x = exchange_f(i, fin);
            fin.wpart = c->wpart.as<double>();
            if (i > seg0) {  // step i-1's finalize in this SpMV's prologue; ||f||^2 from its update when not NaN
                fin.fast = fast;
                fin.h2 = h2;
                fin.step = i - 1;
                fin.alpha = c->alpha.as<double>();
                fin.offd = c->offd.as<double>();
                fin.a3 = a3;
                fin.fn2_i = fn2 + i - 1;
                fin.bov_i = bov + i - 1;
            }
            const bool timed = spmv_timed_step(i);
            ek::dev::spmv(s, spmv_mat(c), x, c->w.as<double>(), nullptr, f, col(i), c->apart.as<double>(), &fin,
                          timed ? ev[size_t(2 * (i - seg0))] : nullptr, timed ? ev[size_t(2 * (i - seg0) + 1)] : nullptr);
            ++matvecs;
            ek::dev::sum_pair(s, c->apart.as<double>(), c->wpart.as<double>(), c->nrb_spmv, aw);
            allreduce(c, aw, 2);
            ek::dev::pro_step(s, aw, aw + 1, 1, a3, fn2 + i, bov + i, c->alpha.as<double>(), c->offd.as<double>(),
                              c->omega.as<double>(), c->prost.as<ek::dev::ProState>(), c->pflags.as<int>(), i, seg0, m,
                              pro_thresh, pro_eps1);
            const int* flag = c->pflags.as<int>() + i;
            const int nc = i + 1, tot = nc + has_u0;
            ek::dev::gemvt_tt(s, ldv, nrb, V(), nc, has_u0, u0val, nreal, c->w.as<double>(), a3, col(i),
                              i > 0 ? col(i - 1) : nullptr, fn2 + i, bov + i, f, c->part.as<double>(), nullptr, nullptr,
                              0, nullptr, nullptr, nt, flag, nullptr, nullptr);
            ek::dev::reduce_cols(s, c->part.as<double>(), nrb, tot + 1, h2);  // (+ ||f'||^2)
            allreduce(c, h2, size_t(tot + 1));
            ek::dev::update(s, ldv, V(), nc, has_u0, u0val, nreal, h2, f, f, c->npart.as<double>(), nullptr, nullptr,
                            fast, nt, flag);
        }
        if (kend == m) {  // the cycle's last step (always projected): its finalize and residual norm
            ek::dev::finalize_step(s, c->npart.as<double>(), nub, fn2 + m, nullptr, h2, m - 1, c->alpha.as<double>(),
                                   c->offd.as<double>(), a3, fn2 + m - 1, bov + m - 1);
            allreduce(c, fn2 + m, 1);
        }
        HIPCHK(hipGetLastError());
    }

    // Single GPU, reorth 1: four launches per step.  The SpMV also runs the
    // previous step's finalize (||f||^2, alpha, beta) and the update reduces
    // the projection partials itself (same column-sum order as k_reduce_cols,
    // so the fused and unfused paths give identical bits).  Folding the
    // three-term recurrence into the projection was measured slower: every
    // column tile re-reads w, v_i and v_{i-1}.  Step i > seg0 finalizes step
    // i - 1 in its SpMV, also across chunks; the last step of the cycle is
    // finalized by its own launch.
    // Who sums the projection partials (nrb row blocks per column): every
    // update workgroup itself (k_update<true>: no launch, but each of the
    // ldv/512 workgroups reads all tot x nrb partials, quadratic in n) or one
    // k_reduce_cols launch ahead of k_update<false> (same col_sum2 order, the
    // same bits).  EK_UPD_RED=0/1 forces either (A/B).
    // 0: a k_reduce_cols launch; 1: every update workgroup; 2: the
    // projection's last workgroup per column group (k_gemvt hand-off, the
    // default up to 256 row blocks).  EK_UPD_RED=0/1/2 forces one (A/B; all
    // three give the same bits).
    static int upd_reduces(int nrb) {
        const char* e = std::getenv("EK_UPD_RED");
        if (e && e[0]) return e[0] - '0';
        return nrb <= EK_UPD_RED_MAX_NRB ? 2 : 0;
    }
    void factorize_fused(int k, int kend) {
        // EK_LANCZOS_TT=0: the separate three-term launch (A/B; the same bits)
        static const bool tt_fused = env_flag("EK_LANCZOS_TT", true);
        double* fn2 = c->fn2.as<double>();
        double* a3 = c->scal.as<double>() + 2;
        const double* bov = c->bov.as<double>();
        // (partial reorthogonalisation: a skipped step has no partials for
        // every update workgroup to reduce, so the update_r form is not used)
        const int upd_red = pro && upd_reduces(nrb) == 1 ? 0 : upd_reduces(nrb);
        // ||f||^2 for the next SpMV from the update (or, on a skipped step, ||f'||^2)
        double* fast = (b32 || pro) ? c->scal.as<double>() + 4 : nullptr;
        const bool tt = tt_fused || pro;
        unsigned* gctr = upd_red == 2 ? c->gctr.as<unsigned>() : nullptr;
        double* hoff = upd_red == 2 ? c->h2.as<double>() : nullptr;
        const bool inl = pro && proi && upd_red == 2;
        static const bool pro_apart = env_set("EK_PRO_APART");  // (lab: k_pro + alpha re-reduced in the projection)
        ek::dev::ProLaunch pl;
        if (inl) {
            pl.wpart = c->wpart.as<double>();
            pl.alpha = c->alpha.as<double>();
            pl.offd = c->offd.as<double>();
            pl.omega = c->omega.as<double>();
            pl.st = c->prost.as<ek::dev::ProState>();
            pl.flags = c->pflags.as<int>();
            pl.pub = pro_pub();
            pl.a3 = a3;
            pl.seg0 = seg0;
            pl.m = m;
            pl.thresh = pro_thresh;
            pl.eps1 = pro_eps1;
            pl.cgw = pro_cgw;
            // tickets (dispatch-order independence): a launch whose grid is
            // not all resident at once takes them (pl.cap); EK_PRO_TICKETS=1
            // on every launch, =0 on none (logical index = blockIdx: A/B)
            static const int tickets = env_flag("EK_PRO_TICKETS", false) ? 2 : env_flag("EK_PRO_TICKETS", true) ? 1 : 0;
            if (tickets) pl.tix = pro_pub() + size_t(ek::dev::PRO_PUB_WORDS) * ek::dev::PRO_PUB_STRIDE;
            if (tickets == 1) {
                pl.cap = ek::dev::gemvt_pro_capacity(nt, c->nrb_spmv > 12 * 256, pro_merge, pro_merge && b32,
                                                     c->num_cu);
                // the most workgroups per row block (<= pro_cgw) with which the
                // cycle's widest launch is still resident at once: its launches
                // then need no tickets (the headline: 8 -> 2, +0.2 ms a solve,
                // against +1.0 ms for tickets on every launch;
                // profiles/r06/dispatch_order_ab.txt)
                const int ncg_max = (m + has_u0 + ek::dev::GT_COLS - 1) / ek::dev::GT_COLS;
                auto grid = [&](int cg) { return ek::dev::gemvt_pro_grid(nrb, std::min(ncg_max, cg), ldv, pro_merge); };
                int cg = pl.cgw;  // (0: one workgroup per tile, left as it is; EK_PRO_CGW: as set)
                while (!pro_cgw_env && cg > 1 && grid(cg) > pl.cap) --cg;
                if (!pro_cgw_env && cg > 0 && grid(cg) <= pl.cap) pl.cgw = cg;
            }
            pl.rev = env_set("EK_DISPATCH_REVERSE") ? 1 : 0;
            if (pro_merge) {
                pl.merged = 1;
                pl.npart = c->npart.as<double>();
                pl.V32 = V32();
                pl.fb = b32 ? c->fbk.as<unsigned>() : nullptr;
            }
        }
        const bool mrg = inl && pro_merge;
        for (int i = k; i < kend; ++i) {
            ek::dev::StepFin fin;
            if (i > seg0) {
                fin.npart = c->npart.as<double>();
                fin.nb = nub;
                fin.fn2_out = fn2 + i;
                fin.h2 = c->h2.as<double>();
                fin.step = i - 1;
                fin.alpha = c->alpha.as<double>();
                fin.offd = c->offd.as<double>();
                fin.a3 = a3;
                fin.fn2_i = fn2 + i - 1;
                fin.bov_i = bov + i - 1;
                fin.fast = fast;  // the update's ||f||^2 (or NaN)
            }
            if (pro) fin.wpart = c->wpart.as<double>();  // ||w||^2 partials for k_pro (also at i == seg0)
            if (mrg) fin.pub_rearm = pro_pub();  // (the merged update's words and done counter)
            if (chk_dst && i == kend - 1 && i > seg0) {  // the check's copy, in this SpMV's block 0
                fin.chk_dst = chk_dst;
                fin.chk_word = chk_word;
                fin.chk_seq_src = chk_seq_src;
                fin.chk_b = chk_b;
                fin.chk_m = m;
                fin.chk_fn2 = fn2;
                chk_folded = true;
            }
            const bool timed = spmv_timed_step(i);
            // the SpMV's last block also reduces alpha into a3 (k_three_term's bits)
            ek::dev::spmv(s, spmv_mat(c), c->f.as<double>(), c->w.as<double>(), fn2 + i, c->f.as<double>(), col(i),
                          c->apart.as<double>(), (i > seg0 || pro) ? &fin : nullptr,
                          timed ? ev[size_t(2 * (i - seg0))] : nullptr, timed ? ev[size_t(2 * (i - seg0) + 1)] : nullptr,
                          !pro && tt_fused && alpha_last ? a3 : nullptr, c->actr.as<unsigned>());
            ++matvecs;
            const int nc = i + 1;
            // partial reorthogonalisation: alpha, and whether this step projects
            const int* flag = pro ? c->pflags.as<int>() + i : nullptr;
            if (pro && !inl)
                ek::dev::pro_step(s, c->apart.as<double>(), c->wpart.as<double>(), c->nrb_spmv, a3, fn2 + i, bov + i,
                                  c->alpha.as<double>(), c->offd.as<double>(), c->omega.as<double>(),
                                  c->prost.as<ek::dev::ProState>(), c->pflags.as<int>(), i, seg0, m, pro_thresh, pro_eps1);
            if (tt) {  // the projection of f' = w - alpha v_i - beta v_{i-1}, formed per row (and stored to f)
                ek::dev::gemvt_tt(s, ldv, nrb, V(), nc, has_u0, u0val, nreal, c->w.as<double>(), a3, col(i),
                                  i > 0 ? col(i - 1) : nullptr, fn2 + i, bov + i, c->f.as<double>(), c->part.as<double>(),
                                  col32(i),
                                  inl || pro_apart || !(alpha_last || pro) ? c->apart.as<double>() : nullptr, c->nrb_spmv,
                                  gctr, hoff, nt, flag, pro ? fast : nullptr, inl ? &pl : nullptr);
            } else {
                ek::dev::three_term(s, ldv, c->apart.as<double>(), c->nrb_spmv, a3, c->w.as<double>(), col(i),
                                    i > 0 ? col(i - 1) : nullptr, fn2 + i, bov + i, c->f.as<double>(), col32(i));
                ek::dev::gemvt(s, ldv, nrb, V(), nc, has_u0, u0val, nreal, c->f.as<double>(), c->part.as<double>(),
                               b32 ? 1 : 0, gctr, hoff, nt);
            }
            // (b32: ||f'||^2 rides along as one more column of the partials)
            unsigned* fb = b32 ? c->fbk.as<unsigned>() : nullptr;
            // (b32: the update also leaves ||f||^2 = ||f'||^2 - ||h||^2 for the next SpMV)
            if (mrg) {
                // (the update ran inside the projection launch)
            } else if (upd_red == 2) {  // h (and ||f'||^2) reduced by the projection
                ek::dev::update(s, ldv, V(), nc, has_u0, u0val, nreal, c->h2.as<double>(), c->f.as<double>(),
                                c->f.as<double>(), c->npart.as<double>(), V32(), fb, fast, nt, flag,
                                inl ? pro_pub() : nullptr);
            } else if (upd_red == 1) {
                ek::dev::update_r(s, ldv, V(), nc, has_u0, u0val, nreal, c->part.as<double>(), nrb, c->h2.as<double>(),
                                  c->f.as<double>(), c->f.as<double>(), c->npart.as<double>(), V32(), fb, fast, nt);
            } else {
                ek::dev::reduce_cols(s, c->part.as<double>(), nrb, nc + has_u0 + ((b32 || pro) ? 1 : 0),
                                     c->h2.as<double>());
                ek::dev::update(s, ldv, V(), nc, has_u0, u0val, nreal, c->h2.as<double>(), c->f.as<double>(),
                                c->f.as<double>(), c->npart.as<double>(), V32(), fb, fast, nt, flag);
            }
            if (b32) ++u32_steps;
        }
        if (kend == m)
            ek::dev::finalize_step(s, c->npart.as<double>(), nub, fn2 + m, nullptr, c->h2.as<double>(), m - 1,
                                   c->alpha.as<double>(), c->offd.as<double>(), a3, fn2 + m - 1, bov + m - 1);
        HIPCHK(hipGetLastError());
    }

    // The sharded step projects f' by linearity (V^T f' = V^T w - alpha V^T v_i
    // - beta V^T v_{i-1}), exact to eps ||w||.  When f' cancelled (update_mr's
    // cflag: ||f'||^2 < mr_cancel ||w||^2, near an invariant subspace) that is
    // not small against ||f'||, and v_{j1} = f_{j1}/||f_{j1}|| would carry a
    // loss of orthogonality of eps ||w|| / beta_{j1}.  The driver sees the flag
    // at its next check and re-projects: f = v_{j1} (unit; or f_m itself at
    // the cycle's end, j1 == m) against V[:, :j1] and u0 — one more CGS pass,
    // the CGS2 path's second pass — with Spectra's H += V^T f correction
    // (scaled by beta_{j1}: f_{j1} = beta_{j1} v_{j1}) and T(j1, j1-1) =
    // beta_{j1} ||f|| through the beta override; the cycle continues at j1.
    // beta_j1: sqrt(fn2[j1]) as the run left it (host copy); returns the
    // corrections (h[j1-1], h[j1-2]) to add to the host's T.
    std::pair<double, double> repair(int j1, double beta_j1) {
        double* f = c->f.as<double>();
        double* fn2 = c->fn2.as<double>();
        const double sc = j1 < m ? beta_j1 : 1.0;
        if (j1 < m) HIPCHK(hipMemcpyAsync(f, col(j1), size_t(ldv) * 8, hipMemcpyDeviceToDevice, s));
        ek::dev::gemvt(s, ldv, nrb, V(), j1, has_u0, u0val, nreal, f, c->part.as<double>());
        ek::dev::reduce_cols(s, c->part.as<double>(), nrb, j1 + has_u0, c->h1.as<double>());
        allreduce(c, c->h1.as<double>(), size_t(j1 + has_u0));
        ek::dev::update(s, ldv, V(), j1, has_u0, u0val, nreal, c->h1.as<double>(), f, f, c->npart.as<double>());
        reduce_scalar(fn2 + j1);
        double hh[2] = {0.0, 0.0}, n2 = 0.0;
        HIPCHK(hipMemcpyAsync(hh, c->h1.as<double>() + std::max(j1 - 2, 0), size_t(std::min(j1, 2)) * 8,
                              hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&n2, fn2 + j1, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const double h1 = sc * (j1 >= 2 ? hh[1] : hh[0]), h2 = j1 >= 2 ? sc * hh[0] : 0.0;  // h[j1-1], h[j1-2]
        // device T entries (the host's are corrected by the caller)
        double a = 0.0, o = 0.0;
        HIPCHK(hipMemcpyAsync(&a, c->alpha.as<double>() + j1 - 1, 8, hipMemcpyDeviceToHost, s));
        if (j1 >= 2) HIPCHK(hipMemcpyAsync(&o, c->offd.as<double>() + j1 - 1, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        a += h1;
        o += h2;
        HIPCHK(hipMemcpyAsync(c->alpha.as<double>() + j1 - 1, &a, 8, hipMemcpyHostToDevice, s));
        if (j1 >= 2) HIPCHK(hipMemcpyAsync(c->offd.as<double>() + j1 - 1, &o, 8, hipMemcpyHostToDevice, s));
        if (j1 < m) {
            const double bo = beta_j1 * std::sqrt(std::max(0.0, n2));
            HIPCHK(hipMemcpyAsync(c->bov.as<double>() + j1, &bo, 8, hipMemcpyHostToDevice, s));
        }
        HIPCHK(hipStreamSynchronize(s));  // (host operands)
        ++repairs;
        return {h1, h2};
    }
    int repairs = 0;
    double mr_cancel = 0x1p-20;

    // The single-context step chunk as a HIP graph.  Eager, the host spends
    // ~10 us per kernel launch, so a partially reorthogonalised step (four
    // launches, ~26 us of kernels when it skips the basis passes) waited for
    // its launches (tools/trace_gaps.py: the GPU idle between kernels).  A
    // chunk's launches depend only on (k, kend, seg0) and the context's
    // buffers, so its graph is captured the second time the chunk is run and
    // replayed from then on: the restart cycles repeat the same chunks, and a
    // service's solves all of them.  (The first time it runs eagerly: a
    // one-shot process does not pay for captures it never replays.)
    bool graphs = false;
    void factorize_graph(int k, int kend) {
        const auto key = std::make_tuple(k, kend, seg0, static_cast<const void*>(V()), static_cast<const void*>(V32()));
        auto it = c->lz_graphs.find(key);
        if (it == c->lz_graphs.end()) {
            if (++c->lz_seen[key] < 2) return factorize_fused(k, kend);
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
            try {
                factorize_fused(k, kend);  // (recorded, not run; its host counters advance here)
            } catch (...) {
                (void)hipStreamEndCapture(s, &g);
                if (g) (void)hipGraphDestroy(g);
                throw;
            }
            HIPCHK(hipStreamEndCapture(s, &g));
            hipGraphExec_t ex = nullptr;
            const hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            HIPCHK(e);
            it = c->lz_graphs.emplace(key, ex).first;
        } else {
            matvecs += kend - k;
            if (b32) u32_steps += kend - k;
            // (the replayed launches carry the check's fold exactly when the
            // captured ones did: factorize_fused's condition, constant per chunk)
            if (chk_dst && kend - 1 > seg0) chk_folded = true;
        }
        HIPCHK(hipGraphLaunch(it->second, s));
    }

    // Invariant subspace found at step j1-1 (||f|| collapsed, as on a graph
    // with several components): continue the sequence from a fresh random
    // vector orthogonal to V[:, :j1] and u0, with H(j1, j1-1) = 0 — Spectra's
    // Lanczos::factorize_from restart-on-breakdown.  The vector is generated
    // over GLOBAL indices so every rank builds the same one.
    // The sequence is the Lehmer generator st <- 48271 st mod (2^31 - 1) from
    // st0; the device kernel jumps ahead to each global row (a host loop over
    // the rows, plus the copy, took ~0.6 ms of GPU idle per injection).
    void inject(int j1, int tag) {
        const uint64_t st0 = 2654435761ull * uint64_t(tag) % 2147483647ull + 1;
        double* f = c->f.as<double>();
        ek::dev::inject_random(s, f, ldv, c->row0, c->nrows, st0);
        for (int pass = 0; pass < 2; ++pass) {
            ek::dev::gemvt(s, ldv, nrb, V(), j1, has_u0, u0val, nreal, f, c->part.as<double>());
            ek::dev::reduce_cols(s, c->part.as<double>(), nrb, j1 + has_u0, c->h1.as<double>());
            allreduce(c, c->h1.as<double>(), size_t(j1 + has_u0));
            ek::dev::update(s, ldv, V(), j1, has_u0, u0val, nreal, c->h1.as<double>(), f, f,
                            pass == 1 ? c->npart.as<double>() : nullptr);
        }
        reduce_scalar(c->fn2.as<double>() + j1);
        HIPCHK(hipMemsetAsync(c->bov.as<double>() + j1, 0, 8, s));  // beta_j1 = +0.0
    }

    // pinned slot i of the mid-cycle checks: alpha[m], offd[m], fn2[m]
    // (four regions: alpha, offd, fn2 at m-based offsets; the sharded step's
    // cancellation flags at CHK_FLAGS)
    static constexpr size_t CHK_FLAGS = 3 * size_t(ek::dev::MAX_NCV + 2);
    double* chk_slot(int i) { return c->chk_pin + size_t(i) * 4 * size_t(ek::dev::MAX_NCV + 2); }

    // The SpMV's kernel timestamps are taken on every 4th step of a cycle: a
    // launch with timing events costs the host ~7 us more, which the timed
    // solve would otherwise carry on every step.  The sample starts at the
    // cycle's second step: the first SpMV after a restart (1 in 100 of the
    // launches) follows the V <- VQ stream and would be 1 in 25 of the sample.
    static constexpr int SPMV_SAMPLE = 4;
    bool spmv_timed_step(int i) const {
        return time_spmv && (i - seg0) % SPMV_SAMPLE == 1 && size_t(2 * (i - seg0) + 1) < ev.size();
    }

    // the timed SpMVs of steps [seg0, kend) (the steps launched in this run)
    void collect_spmv_times(int kend) {
        if (!time_spmv) return;
        HIPCHK(hipStreamSynchronize(s));
        for (int i = seg0; i < kend && size_t(2 * (i - seg0) + 1) < ev.size(); ++i) {
            if (!spmv_timed_step(i)) continue;
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[size_t(2 * (i - seg0))], ev[size_t(2 * (i - seg0) + 1)]));
            spmv_ms += ms;
            ++spmv_timed;
        }
    }
};

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

// One solve of ek_lanczos_fiedler: the plan (the options and every EK_*
// switch the solve honours, resolved), the host's copy of the projected
// matrix and the restart state, and the solve's stages in the order the entry
// function calls them.  The device step sequences are struct Lanczos's.
struct Solve {
    ek_ctx* c;
    hipStream_t s;
    ek_lanczos_opts o;
    Lanczos L{};
    const Clock::time_point t0 = Clock::now();
    // the plan
    int64_t n = 0;
    bool deflate = true;
    int nev = 1, m = 0, maxit = 0, keep_min = 0;
    size_t ldv = 0;
    double tol = 0.0, eps23 = 0.0, beta_eps = 0.0;
    bool trace = false, ortho_check = false, mr_step = false, chk_kernel = true, chk_poll = true;
    // the projected matrix T (diagonal d, off-diagonal e), its Ritz values and
    // their last components, and the cycle's read-back
    std::vector<double> d, e, theta, zl, alpha_h, offd_h, fn2_h;
    std::vector<ek::QRot> rots;
    std::vector<double> qscratch;
    int k = 0, restarts = 0, nconv = 0, injected = 0;
    double fn2_k = 1.0;  // ||f_k||^2 entering a cycle (after an implicit restart: the restart's residual)
    bool converged = false;
    int mf = 0;  // steps the returned Ritz pair is taken from (< m: converged at a mid-cycle check)
    double ortho_max = 0.0;
    double host_restart_ms = 0.0, device_cycle_ms = 0.0, host_qr_ms = 0.0;  // EK_LANCZOS_TRACE diagnostics
    double host_ql_ms = 0.0, restart_sync_ms = 0.0;
    Clock::time_point th;  // the host's restart work began (the cycle's device work was read back)
    unsigned chk_seq_of[2] = {0u, 0u};
    bool cycle_reset = false;  // the restart already queued the resets cycle() starts with
    // the Ritz pair as the finish stages see it: the value, the vector in
    // pinned host memory and contiguous over the global rows on the device
    double lambda = 0.0;
    double* v = nullptr;
    double* xc = nullptr;

    // the caller's outputs (each may be null)
    struct Result {
        double* lambda;
        double* v;
        ek_lanczos_stats* stats;
    };

    Solve(ek_ctx* ctx, const ek_lanczos_opts* opts) : c(ctx), s(ctx->stream) {
        ek_lanczos_default_opts(&o);
        if (opts) o = *opts;
        c->comm_ms = 0.0;
        c->n_ag = c->n_ar = 0;
        c->comm_time = o.time_spmv && c->mr;
        c->cm_rec.clear();
        c->cm_used = 0;
        if (c->comm_time) c->x_ms = c->ar_ms = 0.0, c->x_timed = c->ar_timed = 0;
        c->fied_n = 0;  // any earlier vector is void once a solve starts; set again only on success
    }

    double anorm() const {
        double a = 1.0;
        for (int i = 0; i < m; ++i) a = std::max(a, std::fabs(d[size_t(i)]) + (i > 0 ? std::fabs(e[size_t(i - 1)]) : 0.0));
        return a;
    }

    // Every option and switch of the solve, resolved; no device call.
    void plan() {
        n = c->n;
        deflate = o.deflate != 0;
        nev = deflate ? 1 : 2;
        // ncv: the reference's min(100, n/2) (cEIG.cpp:195) for the full and CGS2
        // passes.  Under partial reorthogonalisation (reorth 3, the default) a
        // step costs ~ncv only when it projects, and a restart's host QL and QR
        // shifts cost ~ncv^2 with the GPU idle, so below a million rows, where a
        // restart weighs most against the steps, a smaller basis pays: min(80,
        // n/2) (round 5, tools/ncv_ab.py, profiles/r05/ncv_ab_r05*.txt: headline
        // 17.6 -> 16.7 ms, ibm10 38.7 -> 37.7, the 2x LCC 36.8 -> 35.2, the 5x
        // LCC 54.0 -> 51.2, ibm01 7.6 -> 6.9; 64-72 lose on ibm10).  Above it
        // the steps dominate and the basis's convergence decides: the 10x
        // synthetic (disconnected: its null space) took 838 matvecs at 80 against
        // 394 at 100 (tools/ncv10_lab.py, profiles/r05/ncv10.txt)
        // reorth 3: partial reorthogonalisation, on the single-context step and
        // on the sharded one (factorize_mr_pro; the CGS2 step always projects).
        // EK_REORTH=1|3 overrides (A/B).
        const int reorth_mode = env_int("EK_REORTH", o.reorth);
        const int ncv_dflt = reorth_mode == 3 && n < 1000000 ? 80 : 100;
        m = o.ncv > 0 ? o.ncv : int(std::min<int64_t>(ncv_dflt, n / 2));
        m = int(std::min<int64_t>(m, n - (deflate ? 1 : 0)));
        if (m > ek::dev::MAX_NCV) ek::fail(EK_EINVAL, "ncv %d exceeds %d", m, ek::dev::MAX_NCV);
        if (m <= nev) ek::fail(EK_EINVAL, "graph too small for ncv=%d (n=%lld)", m, (long long)n);
        mf = m;
        tol = o.tol > 0 ? o.tol : 1e-10;
        maxit = o.maxit > 0 ? o.maxit : 1000;
        eps23 = std::pow(std::numeric_limits<double>::epsilon(), 2.0 / 3.0);
        trace = env_set("EK_LANCZOS_TRACE");
        ortho_check = env_set("EK_LANCZOS_ORTHO");

        L.c = c;
        L.s = c->stream;
        L.m = m;
        L.ldv = int(round_up(std::max<int64_t>(c->nloc, 1), ek::dev::GT_ROWS));
        L.nrb = L.ldv / ek::dev::GT_ROWS;
        L.nub = L.ldv / ek::dev::UPD_ROWS;
        L.has_u0 = deflate ? 1 : 0;
        L.nreal = int(c->nrows);
        L.u0val = 1.0 / std::sqrt(double(n));
        L.time_spmv = o.time_spmv != 0;
        L.reorth = o.reorth == 2 ? 2 : 1;
        L.pro = reorth_mode == 3 && L.reorth == 1 && !env_set("EK_LANCZOS_UNFUSED");
        // threshold 1e-10, not Simon's sqrt(eps): across implicit restarts the
        // kept Ritz block carries the basis's loss of orthogonality into the next
        // cycle, and the dropped projection coefficients (O(threshold) beta) stay
        // in the Lanczos relation.  tools/pro_model.py on ibm10 (15 restarts):
        // sqrt(eps) -> max|V^T V - I| 1e-7, residual 2e-9, lambda off by 5e-10;
        // 1e-9 -> 3e-8, 1.4e-9; 1e-10 -> 1.4e-10, 1.9e-10 (full: 5e-14, 1e-12),
        // 44 % of the steps projected; the headline LCC 32 %, residual unchanged
        L.pro_thresh = o.reorth_thresh > 0 ? o.reorth_thresh : 1e-10;
        L.pro_eps1 = std::numeric_limits<double>::epsilon() * std::sqrt(double(n));
        // (the in-launch decision and merged update: single context only; the
        // sharded step all-reduces alpha and ||w||^2 before its k_pro launch.
        // Their spin-waits assume workgroups are dispatched in index order, which
        // HIP does not promise: every wait is bounded, the first to give up aborts
        // the launch's other waiters (kernels_lanczos.hip pro_poll), and the solve
        // fails with EK_EHIP.  EK_PRO_INLAUNCH=0 runs the step with no in-launch
        // wait at all.)
        if (L.pro && !c->mr) L.proi = env_flag("EK_PRO_INLAUNCH", true);
        if (L.proi) L.pro_merge = env_flag("EK_PRO_MERGE", true);
        // column groups walked per projection workgroup: about 850 projection
        // workgroups, at least 3 per row block (the 1.15x LCC, 207 row blocks:
        // 4; ibm01 / ibm10: one workgroup per tile as before).  A skipped step
        // then dispatches ~850 + 422 workgroups instead of up to ~3,100 (headline
        // Lanczos 20.4 -> 19.4 ms; ibm10 and ibm01 lost 3-10 % at 3-4 per row
        // block: too few workgroups for the projecting steps;
        // profiles/r04/cgw/).  Round 5: with column group 0 dispatched first the
        // other groups' workgroups cost a skipped step little (they read the
        // decision and return), so more of them, which a projecting step uses,
        // pay: at least 8 per row block (headline Lanczos 17.93-18.05 ms at 4,
        // 17.67-17.72 at 6, 17.53-17.61 at 8, 17.66-17.70 at one per tile;
        // profiles/r05/pro/cgw_ab*.txt).  EK_PRO_CGW overrides (0: one workgroup
        // per tile)
        L.pro_cgw = std::max(8, 850 / std::max(1, L.nrb));
        if (const char* e = std::getenv("EK_PRO_CGW"); e && e[0]) {
            L.pro_cgw = std::atoi(e);
            L.pro_cgw_env = true;
        }
        ldv = size_t(L.ldv);
        // the fp32 shadow: single-context three-term steps (the sharded and CGS2
        // steps project w itself, where h is not small)
        // (EK_BASIS32=0|1 / EK_ALPHA_LAST=0|1 override the options: A/B runs)
        L.b32 = env_flag("EK_BASIS32", o.basis32 != 0) && !c->mr && L.reorth == 1 &&
                !env_set("EK_LANCZOS_UNFUSED");
        L.alpha_last = env_flag("EK_ALPHA_LAST", o.alpha_last != 0);
        // non-temporal basis passes once the fp64 basis exceeds 768 MB (3x the
        // 256 MB MALL): it cannot stay there, and sweeping it through evicts the
        // matrix and x between SpMVs.  10x synthetic (1.6 GB): 404 -> 380 us per
        // matvec; at 300 MB (the 2x synthetics) the basis still profits from the
        // MALL (LCC 59.3 -> 61.2 ms with them).  EK_V_NT=0/1 forces either.
        L.nt = env_flag("EK_V_NT", ldv * size_t(m + 1) * 8 > (size_t(768) << 20));
        // the step chunks' graphs (EK_LANCZOS_GRAPH=0: eager launches, A/B), kept
        // while every buffer and parameter their launches carry is unchanged
        // (graph_signature)
        L.graphs = env_flag("EK_LANCZOS_GRAPH", true) && !c->mr && L.reorth == 1;
        // the restart's floor on the kept vectors (EK_KEEP_MIN overrides: A/B)
        keep_min = env_set("EK_KEEP_MIN")    ? std::atoi(std::getenv("EK_KEEP_MIN"))
                   : o.keep_min < 0          ? m / 5
                                             : o.keep_min;
        beta_eps = std::numeric_limits<double>::epsilon() * std::sqrt(double(n));
        // the sharded step's re-projection of a cancelled f' (Lanczos::repair);
        // EK_LANCZOS_UNFUSED runs that step (and its flags) on a single context too
        mr_step = (c->mr || env_set("EK_LANCZOS_UNFUSED")) && L.reorth == 1 && !L.pro;
        // the owned-slot / halo split of the sharded SpMV (EK_MR_OVERLAP=0: one
        // SpMV after the all-gather, the round-3 step; A/B and tests)
        L.overlap = c->mr && c->own_ready && env_flag("EK_MR_OVERLAP", true);
        if (mr_step)
            if (const char* e = std::getenv("EK_MR_CANCEL"); e && e[0]) L.mr_cancel = std::atof(e);  // (tests)
        chk_kernel = env_flag("EK_CHK_KERNEL", true);
        // The mid-cycle check's gather on the compute stream itself, followed by
        // a completion word the host polls (EK_CHK_POLL=0: the event on the
        // compute stream, the gather on the copy stream, an event the host waits
        // on).  The event was a barrier packet that drained the compute queue at
        // every chunk boundary (~12 us each, ~57 a solve); a kernel in the stream
        // is not.  The word is the gather's last store, made after every store of
        // the slot is released to the system (k_chk_gather).
        chk_poll = chk_kernel && env_flag("EK_CHK_POLL", true);

        d.assign(size_t(m), 0.0);
        e.assign(size_t(m), 0.0);
        theta.resize(size_t(m));
        zl.resize(size_t(m));
        alpha_h.resize(size_t(m + 1));
        offd_h.resize(size_t(m + 1));
        fn2_h.resize(size_t(m + 2));
    }

    // The solve's device buffers, sized, and the hand-off counters zeroed.
    void size_workspace() {
        c->V.ensure(ldv * size_t(m + 1) * 8);
        c->Vn.ensure(ldv * size_t(m + 1) * 8);
        if (L.b32) {
            c->V32.ensure(ldv * size_t(m + 1) * 4);
            c->Vn32.ensure(ldv * size_t(m + 1) * 4);
            c->fbk.ensure(64);
            HIPCHK(hipMemsetAsync(c->fbk.p, 0, 4, c->stream));
        }
        // f: + 64 (the sharded step's all-gather slot carries the rank's ||f||^2 at [ldv])
        if (c->mr && c->slot != int64_t(ldv) + 64) ek::fail(EK_ESTATE, "shard slot %lld != ldv + 64", (long long)c->slot);
        c->f.ensure((ldv + 64) * 8);
        c->w.ensure(ldv * 8);
        if (c->mr) c->xfull.ensure(size_t(c->slot) * size_t(c->nranks) * 8);
        c->part.ensure(3 * size_t(m + 2) * size_t(L.nrb) * 8);  // x 3: gemvt3 (sharded step)
        c->h1.ensure(size_t(m + 2) * 8);
        c->h2.ensure(3 * size_t(m + 2) * 8);
        c->alpha.ensure(size_t(m + 1) * 8);
        c->offd.ensure(size_t(m + 1) * 8);
        c->fn2.ensure(size_t(m + 2) * 8);
        c->bov.ensure(size_t(m + 2) * 8);
        c->npart.ensure(size_t(L.nub) * 8);
        c->apart.ensure(size_t(std::max(c->nrb_spmv, 1)) * 8);
        c->Qd.ensure(size_t(m) * size_t(m + 1) * 8);
        c->scal.ensure(64);
        // the hand-off counters are zero between launches; re-armed here too, so a
        // launch that died part-way cannot leave them out of step for this solve
        c->actr.ensure((ek::dev::ALPHA_SUB + 1) * 256);
        HIPCHK(hipMemsetAsync(c->actr.p, 0, c->actr.bytes, s));
        c->gctr.ensure(size_t(ek::dev::GT_HANDOFF_UINTS) * 4);
        HIPCHK(hipMemsetAsync(c->gctr.p, 0, c->gctr.bytes, s));
        if (L.pro) {
            c->wpart.ensure(size_t(std::max(c->nrb_spmv, 1)) * 8);
            c->omega.ensure(3 * size_t(ek::dev::OMEGA_LD) * 8);
            c->prost.ensure(sizeof(ek::dev::ProState));
            // + the in-launch decision's words (PRO_PUB lines of 256 B), zero between launches
            // + the tickets of the in-launch jobs (8 lines of 256 B after them)
            c->pflags.ensure(L.pro_pub_off() + size_t(ek::dev::PRO_PUB_WORDS + 8) * 256);
            HIPCHK(hipMemsetAsync(c->prost.p, 0, sizeof(ek::dev::ProState), s));
            HIPCHK(hipMemsetAsync(L.pro_pub(), 0, size_t(ek::dev::PRO_PUB_WORDS + 8) * 256, s));
        }
        if (mr_step) c->cflag.ensure(size_t(m + 2) * 8);  // (update_mr writes one flag per step)
    }

    // The graph cache's signature: every buffer and parameter the captured
    // launches carry.  A change drops the stale graphs.
    void graph_signature() {
        if (!L.graphs) return;
        const int tt_env = env_set("EK_LANCZOS_TT") ? 1 : 0;
        auto pv = [](const void* p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); };
        auto db = [](double x) {
            uint64_t u;
            std::memcpy(&u, &x, 8);
            return u;
        };
        // (V / Vn and V32 / Vn32 swap at every restart: the pairs, not their order)
        std::vector<uint64_t> sig{std::min(pv(c->V.p), pv(c->Vn.p)), std::max(pv(c->V.p), pv(c->Vn.p)),
                                  std::min(pv(c->V32.p), pv(c->Vn32.p)), std::max(pv(c->V32.p), pv(c->Vn32.p)),
                                  pv(c->f.p), pv(c->w.p),
                                  pv(c->part.p), pv(c->h1.p), pv(c->h2.p), pv(c->alpha.p), pv(c->offd.p), pv(c->fn2.p),
                                  pv(c->bov.p), pv(c->npart.p), pv(c->apart.p), pv(c->scal.p), pv(c->fbk.p),
                                  pv(c->actr.p), pv(c->gctr.p), pv(c->wpart.p), pv(c->omega.p), pv(c->prost.p),
                                  pv(c->pflags.p), pv(c->rb.p), pv(c->pk.p), pv(c->rel.p), pv(c->dict.p), pv(c->col.p),
                                  pv(c->val.p), pv(c->rowptr.p), pv(c->pn_wrow.p), pv(c->pn_start.p), pv(c->pn_word.p),
                                  pv(c->pn_rid.p), uint64_t(m), uint64_t(L.ldv), uint64_t(L.nreal), uint64_t(c->n),
                                  uint64_t(c->nrb_spmv), uint64_t(c->pn_G), uint64_t(c->colbits), uint64_t(L.has_u0),
                                  uint64_t(L.b32), uint64_t(L.pro), uint64_t(L.proi), uint64_t(L.pro_merge), uint64_t(L.nt), uint64_t(L.alpha_last),
                                  uint64_t(tt_env), db(L.pro_thresh),
                                  db(L.pro_eps1), db(L.u0val)};
        if (sig != c->lz_sig) {
            for (auto& g : c->lz_graphs) HIPCHK(hipGraphExecDestroy(g.second));
            c->lz_graphs.clear();
            c->lz_seen.clear();
            c->lz_sig = std::move(sig);
        }
    }

    // The pad rows and vectors zeroed, and what is created once per context:
    // the mid-cycle checks' stream, events and pinned slots, the SpMV timing
    // events.
    void arm_workspace() {
        // padded rows must be exactly 0 (only those: every kernel writes real
        // rows before it reads them, and no kernel writes a padded row nonzero)
        ek::dev::zero_pad_rows(s, c->V.as<double>(), L.ldv, L.nreal, m + 1);
        ek::dev::zero_pad_rows(s, c->Vn.as<double>(), L.ldv, L.nreal, m + 1);
        HIPCHK(hipMemsetAsync(c->w.p, 0, c->w.bytes, s));
        HIPCHK(hipMemsetAsync(c->f.p, 0, c->f.bytes, s));
        if (c->mr) HIPCHK(hipMemsetAsync(c->xfull.p, 0, c->xfull.bytes, s));
        if (!c->cstream) {  // mid-cycle check resources, created once per context
            HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
            // chk_done orders the check's copy (cstream, same device) after a
            // chunk: a device-scope release is all it needs.  With the default
            // system-scope fence every chunk boundary left the compute queue idle
            // for the fence's L2 write-back (6-15 us at each of ~58 boundaries a
            // solve, kernel trace).  EK_CHK_FENCE: 0 system (the HIP default), 1
            // device-scope release (default), 2 no fence
            static const int chk_fence = env_int("EK_CHK_FENCE", 1);
            const unsigned done_flags = hipEventDisableTiming | (chk_fence == 1   ? hipEventReleaseToDevice
                                                                 : chk_fence == 2 ? hipEventDisableSystemFence
                                                                                  : 0u);
            for (int i = 0; i < 2; ++i) {
                HIPCHK(hipEventCreateWithFlags(&c->chk_done[i], done_flags));
                HIPCHK(hipEventCreateWithFlags(&c->chk_copied[i], hipEventDisableTiming));
            }
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->chk_pin), 2 * 4 * size_t(ek::dev::MAX_NCV + 2) * 8,
                                 hipHostMallocDefault));
            // [slot * 64]: the completion words; [128 + slot * 64]: the sequence
            // numbers the folded copy stores (written by the host before the chunk)
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->chk_word), 4 * 256, hipHostMallocCoherent));
            std::memset(c->chk_word, 0, 4 * 256);
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->q_pin),
                                 (size_t(ek::dev::MAX_NCV) * size_t(ek::dev::MAX_NCV + 1) + 2 * size_t(ek::dev::MAX_NCV + 2)) * 8,
                                 hipHostMallocDefault));
        }
        if (L.time_spmv) {  // created once per context: ~200 creations per solve cost milliseconds
            while (c->spmv_ev.size() < size_t(2 * m)) {
                hipEvent_t e;
                HIPCHK(hipEventCreate(&e));
                c->spmv_ev.push_back(e);
            }
            L.ev.assign(c->spmv_ev.begin(), c->spmv_ev.begin() + 2 * m);
        }
    }

    // start vector: Park-Miller LCG over GLOBAL indices (identical on every
    // rank), values in [-0.5, 0.5) like Spectra's SimpleRandom; deflated.
    // Generated on the device (jump-ahead per element, the same doubles as
    // the sequential host loop it replaces, without its ~1 ms and the upload).
    void start_vector() {
        ek::dev::start_vector(s, L.ldv, (long long)c->row0, int(c->nrows), c->f.as<double>());
        double* sc = c->scal.as<double>();
        if (deflate) {
            ek::dev::sum_partial(s, L.ldv, c->f.as<double>(), L.nreal, c->npart.as<double>(), 0);
            L.reduce_scalar(sc);
            ek::dev::scale_sub_mean(s, L.ldv, c->f.as<double>(), L.nreal, sc, 1.0 / double(n));
        }
        ek::dev::sum_partial(s, L.ldv, c->f.as<double>(), L.nreal, c->npart.as<double>(), 1);
        L.reduce_scalar(c->fn2.as<double>());
    }

    // the host's wait for a slot's completion word (bounded: a kernel that
    // never ran must fail the solve, not hang the host)
    void chk_wait(int sl, unsigned seq) {
        volatile unsigned* w = c->chk_word + size_t(sl) * 64;
        const auto t0 = Clock::now();
        for (unsigned spin = 0; *w != seq; ++spin) {
            if ((spin & 1023u) == 1023u) {
                if (Clock::now() - t0 > std::chrono::seconds(20))
                    ek::fail(EK_EHIP, "Lanczos: a mid-cycle check's completion word never arrived");
                const hipError_t qe = hipStreamQuery(s);  // (a faulted stream ends the wait)
                if (qe != hipSuccess && qe != hipErrorNotReady) HIPCHK(qe);
                if (qe == hipSuccess && *w != seq)  // (the stream drained: the word can no longer arrive)
                    ek::fail(EK_EHIP, "Lanczos: the stream finished without a mid-cycle check's completion word "
                                      "(slot %d: %u, expected %u)", sl, *w, seq);
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }

    double t_row(int i) const { return std::fabs(d[size_t(i)]) + (i > 0 ? std::fabs(e[size_t(i - 1)]) : 0.0); }

    // The first step i in [max(from, 1), last] whose ||f_i|| (fn2v[i], squared)
    // is no more than beta_eps ||T||, or -1.  ||T|| is `an`, the norm over every
    // step the caller read; on the sharded step that projects by linearity
    // (mr_step) it is the norm of the steps before i instead.  The launches run
    // on past a breakdown, on the normalised rounding noise of f, which that
    // step's projection (exact to eps ||w||, not eps ||f'||) leaves far from
    // orthogonal to V: beta then grows geometrically from step to step, and
    // after some twenty such steps (ncv 32 on a star or K_n of 64 nodes) the
    // norm over all of them had put the threshold above the ||f_1|| of sound
    // steps, a "breakdown at step 1" that no injected vector could clear.
    int first_breakdown(int from, int last, double an, const double* fn2v) const {
        double ap = 1.0;
        int seen = 0;  // ap covers steps [0, seen): only the steps before the one tested are read
        for (int i = std::max(from, 1); i <= last; ++i) {
            for (; seen < i; ++seen) ap = std::max(ap, t_row(seen));
            if (!(std::sqrt(std::max(0.0, fn2v[i])) > beta_eps * (mr_step ? ap : an))) return i;
        }
        return -1;
    }

    // What ends a run of steps before the cycle does.
    struct Found {
        int j1 = -1;          // breakdown at step j1 (||f_j1|| collapsed)
        int jr = -1;          // re-projection at step jr (the sharded step's f' cancelled)
        double beta_r = 0.0;  // ||f_jr|| as the run left it (a re-projection's scale)
        int jconv = -1;       // > 0: converged on the projected matrix of the first jconv steps (mid-cycle check)
    };

    // The chunk [.., b) ends with a polled check: the slot's sequence number,
    // and (opt-in) the check's copy folded into the chunk's last SpMV.
    void arm_polled_check(int slot, int b) {
        chk_seq_of[slot] = ++c->chk_seq;
        c->chk_word[128 + size_t(slot) * 64] = chk_seq_of[slot];  // (read by the kernel at run time)
        L.chk_dst = L.chk_slot(slot);
        L.chk_word = c->chk_word + size_t(slot) * 64;
        L.chk_seq_src = c->chk_word + 128 + size_t(slot) * 64;
        L.chk_b = b;
        L.chk_folded = false;
        // EK_CHK_FOLD=1: the copy rides in block 0 of the chunk's last
        // SpMV instead of its own k_chk_gather launch (opt-in: same
        // bits, no measurable gain on the headline, r06w A/B)
        static const bool fold = [] {
            const char* e = std::getenv("EK_CHK_FOLD");
            return e && e[0] == '1';
        }();
        if (!fold || mr_step) L.chk_dst = nullptr, L.chk_folded = false;
    }

    // The check of the chunk that ended at b < m, queued behind it: {alpha,
    // offd, fn2} of its steps into pinned slot `slot`.  Returns the last step
    // the slot is complete for.
    int queue_check(int slot, int b) {
        if (chk_poll) {  // the chunk's last SpMV (or a gather after it), then the completion word
            if (!L.chk_folded) {
                ek::dev::chk_gather(s, c->alpha.as<double>(), c->offd.as<double>(), c->fn2.as<double>(),
                                    mr_step ? c->cflag.as<double>() : nullptr, b, m, L.CHK_FLAGS,
                                    L.chk_slot(slot), -1, c->chk_word + size_t(slot) * 64, chk_seq_of[slot]);
            }
            L.chk_dst = nullptr;
            L.chk_folded = false;
            return b - 1;
        }
        double* pinned = L.chk_slot(slot);
        HIPCHK(hipEventRecord(c->chk_done[slot], s));
        HIPCHK(hipStreamWaitEvent(c->cstream, c->chk_done[slot], 0));
        if (chk_kernel) {  // one launch writing the pinned slot (device-accessible host memory)
            ek::dev::chk_gather(c->cstream, c->alpha.as<double>(), c->offd.as<double>(), c->fn2.as<double>(),
                                mr_step ? c->cflag.as<double>() : nullptr, b, m, L.CHK_FLAGS, pinned);
        } else {  // (EK_CHK_KERNEL=0: one DMA blit per array)
            HIPCHK(hipMemcpyAsync(pinned, c->alpha.p, size_t(b) * 8, hipMemcpyDeviceToHost, c->cstream));
            HIPCHK(hipMemcpyAsync(pinned + m, c->offd.p, size_t(b) * 8, hipMemcpyDeviceToHost, c->cstream));
            HIPCHK(hipMemcpyAsync(pinned + 2 * m, c->fn2.p, size_t(b) * 8, hipMemcpyDeviceToHost, c->cstream));
            if (mr_step)
                HIPCHK(hipMemcpyAsync(pinned + L.CHK_FLAGS, c->cflag.p, size_t(b) * 8, hipMemcpyDeviceToHost,
                                      c->cstream));
        }
        HIPCHK(hipEventRecord(c->chk_copied[slot], c->cstream));
        return b - 1;  // complete: alpha, offd of steps < b - 1 (the fused finalize lags one step), fn2 <= b - 1
    }

    // The host's test of a queued check, complete for steps up to j (while the
    // next chunk runs): a breakdown, a cancelled f' or convergence on the
    // projected matrix of the first j steps ends the run (true).
    bool eval_check(int j, int slot, int from, Found& f) {
        if (chk_poll) chk_wait(slot, chk_seq_of[slot]);
        else HIPCHK(hipEventSynchronize(c->chk_copied[slot]));
        const double* pa = L.chk_slot(slot);
        for (int i = from; i < j; ++i) {
            d[size_t(i)] = pa[i];
            if (i > 0) e[size_t(i - 1)] = pa[m + i];
        }
        double an = 1.0;
        for (int i = 0; i < j; ++i) an = std::max(an, t_row(i));
        f.j1 = first_breakdown(from, j, an, pa + 2 * m);
        for (int i = from; mr_step && i < j && f.jr < 0; ++i)
            if (pa[L.CHK_FLAGS + size_t(i)] != 0.0) {
                f.jr = i + 1;
                f.beta_r = std::sqrt(std::max(0.0, pa[2 * m + f.jr]));
            }
        if (f.j1 >= 0 || f.jr >= 0) return true;
        // only the nev smallest Ritz values and their last components
        // (bisection + inverse iteration: ~70 us at j = 100 against
        // ~370 us for all j by QL; with partial reorthogonalisation a
        // chunk of steps is shorter than the QL took, and the GPU
        // waited for the check before the next chunk's launches)
        if (!ek::tridiag_smallest(j, d.data(), e.data(), std::min(nev, j), theta.data(), zl.data()))
            ek::fail(EK_ENOCONV, "tridiagonal eigensolver failed");
        const double fj = std::sqrt(std::max(0.0, pa[2 * m + j]));
        int nc = 0;
        for (int i = 0; i < nev && i < j; ++i)
            if (std::fabs(zl[size_t(i)]) * fj < tol * std::max(eps23, std::fabs(theta[size_t(i)]))) ++nc;
        if (trace)
            std::fprintf(stderr, "[lanczos]   check j=%d theta0=%.15g est0=%.3e\n", j, theta[0],
                         std::fabs(zl[0]) * fj);
        if (nc >= nev) f.jconv = j;
        return nc >= nev;
    }

    // Steps [from, m) enqueued, until a check ends the run.
    // After the first cycle the cycle is enqueued in chunks; the host
    // tests the projected matrix of each chunk (its {alpha, offd,
    // fn2} copied on a second stream into a pinned slot) while the GPU
    // runs the next one: a converged Ritz pair stops the cycle there,
    // a collapsed residual is injected without running the rest of
    // the cycle on a zero vector.
    Found run_chunks(int from) {
        // (about 0.5 ms of GPU work per chunk: the host's check of one
        // chunk and its launches of the next must fit in the chunk the GPU
        // is running.  The step time is modelled from n, not measured, so
        // the stopping step and the result bits do not depend on timing:
        // ~12 us + 0.23 ns per row, 15 us at ibm01, 58 us at ibm18 shape.)
        const int chunk = (restarts > 0 && o.check_every > 0)
                              ? std::max({2, int(o.check_every), int(std::ceil(500.0 / (12.0 + 2.3e-4 * double(n))))})
                              : m;
        Found f;
        int a = from, launched = from;
        int pend = -1, pend_slot = 0, slot = 0;
        while (a < m) {
            const int b = std::min(m, a + chunk);
            if (b < m && chk_poll) arm_polled_check(slot, b);  // this chunk ends with a check: its copy rides on the chunk's last SpMV
            L.factorize(a, b);
            launched = b;
            const int cur = b < m ? queue_check(slot, b) : -1;
            // the previous chunk's check, while this chunk runs
            if (pend >= 0 && eval_check(pend, pend_slot, from, f)) break;
            pend = cur;
            pend_slot = slot;
            slot ^= 1;
            a = b;
        }
        L.collect_spmv_times(launched);
        return f;
    }

    // The whole cycle ran: its projected matrix and residuals (pinned slot 0:
    // no check copy is in flight at the cycle's end), and the breakdown or
    // cancelled f' the checks have not seen yet.
    void read_cycle(int from, Found& f) {
        double* pin0 = L.chk_slot(0);
        if (chk_kernel) {
            ek::dev::chk_gather(s, c->alpha.as<double>(), c->offd.as<double>(), c->fn2.as<double>(), nullptr, m,
                                m, 0, pin0, m + 1);
        } else {
            HIPCHK(hipMemcpyAsync(pin0, c->alpha.p, size_t(m) * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(pin0 + m, c->offd.p, size_t(m) * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(pin0 + 2 * m, c->fn2.p, size_t(m + 1) * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        std::copy(pin0, pin0 + m, alpha_h.begin());
        std::copy(pin0 + m, pin0 + 2 * m, offd_h.begin());
        std::copy(pin0 + 2 * m, pin0 + 3 * m + 1, fn2_h.begin());
        for (int i = from; i < m; ++i) {
            d[size_t(i)] = alpha_h[size_t(i)];
            if (i > 0) e[size_t(i - 1)] = offd_h[size_t(i)];
        }
        f.j1 = first_breakdown(from, m - 1, anorm(), fn2_h.data());
        if (mr_step && f.j1 < 0) {
            std::vector<double> cf(static_cast<size_t>(m));
            HIPCHK(hipMemcpyAsync(cf.data(), c->cflag.p, size_t(m) * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int i = from; i < m && f.jr < 0; ++i)
                if (cf[size_t(i)] != 0.0) {
                    f.jr = i + 1;
                    f.beta_r = std::sqrt(std::max(0.0, fn2_h[size_t(f.jr)]));
                }
        }
    }

    // One cycle: steps k .. m-1, re-run from a fresh vector after a breakdown
    // and from the re-projected one after a cancelled f'.  Returns jconv > 0
    // when a mid-cycle check converged on the first jconv steps (mf); else -1
    // with the cycle's d, e and fn2_h read back for the restart.
    int cycle() {
        if (!cycle_reset) {
            HIPCHK(hipMemsetAsync(c->bov.p, 0xFF, c->bov.bytes, s));  // NaN: no beta override
            if (mr_step) HIPCHK(hipMemsetAsync(c->cflag.p, 0, c->cflag.bytes, s));
        }
        cycle_reset = false;
        const auto tc = Clock::now();
        int cycle_breakdowns = 0;  // bounded per cycle: each one moves the factorisation forward
        int from = k;
        // After an implicit restart the residual f_k can collapse (the kept
        // Ritz space is invariant, seen on the 2x synthetic): a zero column k
        // would leave a spurious exact-zero Ritz pair whose vector is zero, so
        // the cycle starts from a fresh vector at k instead of running on it.
        if (k > 0 && !(std::sqrt(std::max(0.0, fn2_k)) > beta_eps * anorm())) {
            if (trace) std::fprintf(stderr, "[lanczos] restart residual collapsed at %d (|f|^2=%.3e)\n", k, fn2_k);
            ++cycle_breakdowns;
            L.inject(k, ++injected);
        }
        for (;;) {
            L.seg0 = from;
            Found f = run_chunks(from);
            if (f.jconv > 0) {
                HIPCHK(hipStreamSynchronize(s));
                device_cycle_ms += ms_since(tc);
                converged = true;
                mf = f.jconv;
                return f.jconv;
            }
            if (f.j1 < 0 && f.jr < 0) {
                read_cycle(from, f);
                if (f.j1 < 0 && f.jr < 0) break;
            } else {
                HIPCHK(hipStreamSynchronize(s));  // the chunk launched beyond the breakdown / cancellation
            }
            if (f.j1 >= 0 && (f.jr < 0 || f.j1 <= f.jr)) {
                if (trace) std::fprintf(stderr, "[lanczos] breakdown at step %d\n", f.j1);
                if (++cycle_breakdowns > m) ek::fail(EK_ENOCONV, "Lanczos: repeated breakdown within one cycle");
                L.inject(f.j1, ++injected);
                from = f.j1;
            } else {
                const int jr = f.jr;
                if (trace) std::fprintf(stderr, "[lanczos] cancelled f' at step %d: re-projected\n", jr - 1);
                const auto corr = L.repair(jr, f.beta_r);
                d[size_t(jr - 1)] += corr.first;
                if (jr >= 2) e[size_t(jr - 2)] += corr.second;
                HIPCHK(hipMemsetAsync(c->cflag.as<double>() + jr - 1, 0, 8, s));
                if (jr == m) {  // f_m re-projected in place: the cycle's residual norm again
                    HIPCHK(hipMemcpyAsync(&fn2_h[size_t(m)], c->fn2.as<double>() + m, 8, hipMemcpyDeviceToHost, s));
                    HIPCHK(hipStreamSynchronize(s));
                    break;
                }
                from = jr;
            }
        }
        th = Clock::now();
        device_cycle_ms += std::chrono::duration<double, std::milli>(th - tc).count();
        return -1;
    }

    // The full cycle's Ritz values and Spectra's num_converged over the wanted ones.
    bool ritz_converged() {
        if (!ek::tridiag_eig(m, d.data(), e.data(), theta.data(), zl.data(), nullptr))
            ek::fail(EK_ENOCONV, "tridiagonal eigensolver failed");
        host_ql_ms += ms_since(th);
        const double fnorm = std::sqrt(std::max(0.0, fn2_h[size_t(m)]));
        if (!std::isfinite(fnorm)) ek::fail(EK_ENOCONV, "Lanczos breakdown (non-finite residual)");
        nconv = 0;
        for (int i = 0; i < nev; ++i) {  // Spectra num_converged
            const double thresh = tol * std::max(eps23, std::fabs(theta[size_t(i)]));
            if (std::fabs(zl[size_t(i)]) * fnorm < thresh) ++nconv;
        }
        if (trace)
            std::fprintf(stderr, "[lanczos] restart %d k=%d theta0=%.15g est0=%.3e theta1=%.15g fnorm=%.3e\n", restarts,
                         k, theta[0], std::fabs(zl[0]) * fnorm, theta[1], fnorm);
        converged = nconv >= nev;
        return converged;
    }

    // EK_LANCZOS_ORTHO=1 (tests): max |[V u0]^T [V u0] - I| over the
    // cycle's basis at every restart (one projection per column)
    void probe_orthogonality() {
        std::vector<double> hh(size_t(m + L.has_u0));
        for (int j = 0; j < m; ++j) {
            ek::dev::gemvt(s, L.ldv, L.nrb, L.V(), m, L.has_u0, L.u0val, L.nreal, L.col(j), c->part.as<double>());
            ek::dev::reduce_cols(s, c->part.as<double>(), L.nrb, m + L.has_u0, c->h1.as<double>());
            allreduce(c, c->h1.as<double>(), size_t(m + L.has_u0));  // (sharded: each rank's rows)
            HIPCHK(hipMemcpyAsync(hh.data(), c->h1.p, hh.size() * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int q = 0; q < m + L.has_u0; ++q)
                ortho_max = std::max(ortho_max, std::fabs(hh[size_t(q)] - (q == j ? 1.0 : 0.0)));
        }
    }

    // implicit restart with the m-knew unwanted Ritz values as shifts
    // (a fixed restart size of 8, 12 or 20 kept vectors, or a cap of 10-30,
    // was no better over ibm01 / industry2 / ibm10 / the 1x synthetic and
    // its largest component, and some sizes lost 3-12x on one of them)
    void restart() {
        if (ortho_check) probe_orthogonality();
        const bool floor_on = keep_min > 0 && std::fabs(theta[size_t(nev - 1)]) > 1e-8 * anorm();
        // Where the floor applies, it replaces ARPACK's jump to ncv/2 kept
        // vectors (taken when no unwanted Ritz estimate is below eps): which
        // side of eps those estimates fall on is rounding noise, and the jump
        // turned the headline's 6 restarts into 9 (50 kept instead of 20, the
        // same 527 matvecs: 20.0 -> 18.5 ms, tools/restart_ab.py,
        // profiles/r05/restart_ab_keephalf.txt).  EK_KEEP_HALF=1 keeps it.
        const char* kh_env = std::getenv("EK_KEEP_HALF");
        const bool keep_half = kh_env && kh_env[0] == '1';
        int knew = nev_adjusted(nev, m, nconv, zl, !floor_on || keep_half);
        // a floor on Spectra's count: its rule keeps ncv/2 when no unwanted
        // Ritz value has converged but only 1 + (those with |e_m^T y| < eps)
        // otherwise, 2-4 vectors on these Laplacians, and a restart that
        // keeps 3 of 100 throws the subspace away (the 1.15x LCC: 755
        // matvecs with Spectra's rule, 527 with a floor of 20; tools/restart_ab.py)
        // Not when the wanted Ritz value is numerically zero: a disconnected
        // graph, whose null space is degenerate; there keeping more vectors
        // slowed convergence to a null vector (10x synthetic: 362 matvecs
        // with Spectra's rule, 756 with a floor of 10, 994 with 20; the 1x
        // and 2x synthetics likewise)
        if (floor_on) knew = std::max(knew, std::min(keep_min, m - 1));
        if (trace) std::fprintf(stderr, "[lanczos]   keep %d (matvecs so far %d)\n", knew, L.matvecs);
        std::vector<double> dd(d), ee(e);
        const auto tq0 = Clock::now();
        // the unwanted Ritz values as shifts; of Q only the kept columns and
        // the residual's are used: formed right to left from the rotations
        // (ek::accumulate_q).  (A device form that applied the rotations with
        // one workgroup, k_apply_rots, lost: ~9k dependent rotations took 1.36
        // ms per restart against ~0.3 ms on the host for all of Q.)
        rots.clear();
        ek::tridiag_qr_shifts(m, dd.data(), ee.data(), theta.data() + knew, m - knew, rots);
        double* Q = c->q_pin;  // pinned: the upload below is a plain DMA
        ek::accumulate_q(m, rots, knew + 1, Q, qscratch);
        const double sigma = Q[size_t(knew - 1) * m + size_t(m - 1)];  // Q(m-1, knew-1)
        host_qr_ms += ms_since(tq0);
        // the restart's transfers and the next cycle's resets are queued with
        // the GEMM, all through pinned staging, so the one synchronisation
        // below waits for the device work alone (as pageable copies between
        // host wake-ups they left the GPU idle ~30 us a restart): Q, the kept
        // projected matrix and the beta-override reset in one launch that
        // reads the staging directly (three blits and a fill before)
        double* kp = c->q_pin + size_t(ek::dev::MAX_NCV) * size_t(ek::dev::MAX_NCV + 1);
        double* fn2_pin = kp + 2 * (ek::dev::MAX_NCV + 2) - 1;  // (kp uses [0, 2 knew))
        if (L.pro) {  // the kept projected matrix, for k_pro's omega recurrence (alpha[j], offd[j] of j < knew)
            for (int i = 0; i < knew; ++i) kp[i] = dd[size_t(i)];
            for (int i = 1; i < knew; ++i) kp[knew + i] = ee[size_t(i - 1)];
        }
        ek::dev::restart_upload(s, Q, m * (knew + 1), c->Qd.as<double>(), L.pro ? kp : nullptr, knew,
                                c->alpha.as<double>(), c->offd.as<double>(), c->bov.as<double>(),
                                int(c->bov.bytes / 8));
        const double hk = ee[size_t(knew - 1)];  // H(knew, knew-1)
        ek::dev::gemm_vq(s, L.ldv, L.V(), m, c->Qd.as<double>(), knew + 1, c->Vn.as<double>(),
                         L.b32 ? c->Vn32.as<float>() : nullptr);
        ek::dev::axpby_norm(s, L.ldv, c->f.as<double>(), sigma, c->Vn.as<double>() + size_t(knew) * ldv, hk,
                            c->npart.as<double>());
        L.reduce_scalar(c->fn2.as<double>() + knew);
        HIPCHK(hipMemcpyAsync(fn2_pin, c->fn2.as<double>() + knew, 8, hipMemcpyDeviceToHost, s));
        if (mr_step) HIPCHK(hipMemsetAsync(c->cflag.p, 0, c->cflag.bytes, s));  // the next cycle's flags
        cycle_reset = true;
        std::swap(c->V.p, c->Vn.p);
        std::swap(c->V.bytes, c->Vn.bytes);
        if (L.b32) {
            std::swap(c->V32.p, c->Vn32.p);
            std::swap(c->V32.bytes, c->Vn32.bytes);
        }
        const auto tsy = Clock::now();
        HIPCHK(hipStreamSynchronize(s));  // Q upload buffer reused next restart; fn2_k read (and k_pro's staging)
        fn2_k = *fn2_pin;
        restart_sync_ms += ms_since(tsy);
        if (L.pro && env_set("EK_PRO_TRACE")) {  // (lab: the cycle's per-step decisions)
            std::vector<int> fl(static_cast<size_t>(m));
            HIPCHK(hipMemcpy(fl.data(), c->pflags.p, size_t(m) * 4, hipMemcpyDeviceToHost));
            std::string row;
            for (int i = k; i < m; ++i) row += fl[size_t(i)] ? '1' : '0';
            std::fprintf(stderr, "[pro] cycle from %d: %s\n", k, row.c_str());
            for (int i = k; i < m; ++i)
                std::fprintf(stderr, "[pro] %d d %a e %a\n", i, d[size_t(i)], i + 1 < m ? e[size_t(i)] : 0.0);
        }
        for (int i = 0; i < knew; ++i) d[size_t(i)] = dd[size_t(i)];
        for (int i = 0; i + 1 < knew; ++i) e[size_t(i)] = ee[size_t(i)];
        k = knew;
        host_restart_ms += ms_since(th);
    }

    void trace_times() const {
        if (trace)
            std::fprintf(stderr, "[lanczos] factorization cycles %.3f ms, restarts %.3f ms (of which QL %.3f ms, QR shifts "
                         "%.3f ms, waiting for the restart's device work %.3f ms)\n",
                         device_cycle_ms, host_restart_ms, host_ql_ms, host_qr_ms, restart_sync_ms);
    }

    // |x|^2 of the Ritz vector on the host; zero or not finite fails the solve
    // (drain: work is still queued on the stream, which the failure waits out)
    double norm2_or_fail(bool drain) {
        double nx2 = 0.0;
        for (int64_t i = 0; i < n; ++i) nx2 += v[i] * v[i];
        if (!(nx2 > 0.0) || !std::isfinite(nx2)) {
            if (drain) HIPCHK(hipStreamSynchronize(s));
            ek::fail(EK_ENOCONV, "Lanczos: the Ritz vector is zero or not finite (|x|^2 = %g)", nx2);
        }
        return nx2;
    }

    // deterministic sign: the entry of largest magnitude (first on ties) is positive
    double signed_scale(double inv) const {
        int64_t imax = 0;
        for (int64_t i = 1; i < n; ++i)
            if (std::fabs(v[i]) > std::fabs(v[imax])) imax = i;
        return v[imax] < 0 ? -inv : inv;
    }

    // the in-launch hand-offs' waits are bounded: any that gave up fails the solve
    static void fail_on_timeouts(int timeouts) {
        if (timeouts)
            ek::fail(EK_EHIP, "Lanczos: %d in-launch wait(s) of the partially reorthogonalised step gave up "
                              "(EK_PRO_INLAUNCH=0 runs the step without them)", timeouts);
    }

    // the caller's lambda, vector and stats of a solve known good
    void deliver(const Result& out, double sgn, double r2, int projected_steps, int32_t update32_fallbacks) {
        c->comm_time = false;
        if (out.lambda) *out.lambda = lambda;
        if (out.v)
            for (int64_t i = 0; i < n; ++i) out.v[i] = v[i] * sgn;
        if (ek_lanczos_stats* stats = out.stats) {
            stats->restarts = restarts;
            stats->matvecs = L.matvecs;
            stats->converged = 1;
            stats->residual = std::sqrt(r2);
            stats->total_ms = ms_since(t0);
            stats->spmv_ms = L.spmv_ms;
            stats->spmv_timed = L.spmv_timed;
            stats->comm_ms = c->comm_ms;
            stats->allgathers = int32_t(c->n_ag);
            stats->allreduces = int32_t(c->n_ar);
            stats->update32_steps = L.u32_steps;
            stats->update32_fallbacks = update32_fallbacks;
            stats->projected_steps = projected_steps;
            stats->reprojected = L.repairs;
            stats->ortho_max = ortho_max;
        }
    }

    // The Ritz vector of the wanted value, gathered to the global layout and
    // on its way to the host, and the residual's SpMV queued; then the form
    // of the context normalises, fixes the sign and hands the vector over.
    void finish(const Result& out) {
        // Ritz vector of the wanted value (ascending: [0] is the null pair unless deflated)
        const int want = deflate ? 0 : 1;
        std::vector<double> Z(size_t(mf) * mf);
        ek::tridiag_eig(mf, d.data(), e.data(), theta.data(), zl.data(), Z.data());
        lambda = theta[size_t(want)];
        HIPCHK(hipMemcpyAsync(c->Qd.p, Z.data() + size_t(want) * mf, size_t(mf) * 8, hipMemcpyHostToDevice, s));
        double* xloc = c->Vn.as<double>();
        ek::dev::gemm_vq(s, L.ldv, L.V(), mf, c->Qd.as<double>(), 1, xloc);
        // full vector on every rank; copied out through pinned staging kept by the
        // context (pageable copies of these 2 x 8n bytes cost ~0.5 ms a solve)
        // (+ tail: the final step's small read-backs, below: one residual partial
        // per 512 rows, then the in-launch waits' state and the fallback count in
        // the last 8 doubles; at least 4,096 so small graphs keep one allocation)
        const size_t tail = std::max<size_t>(4096, (size_t(std::max(L.nub, 0)) + 8 + 63) & ~size_t(63));
        const size_t need = size_t(n) + size_t(std::max<int64_t>(c->nrows, 1)) + tail;
        if (c->pin_doubles < need) {
            if (c->pin) HIPCHK(hipHostFree(c->pin));
            c->pin = nullptr;
            c->pin_doubles = 0;
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->pin), need * 8, hipHostMallocDefault));
            c->pin_doubles = need;
        }
        v = c->pin;
        double* xg = xloc;  // the vector as the SpMV reads it
        xc = xloc;          // ... and contiguous over the global rows
        if (c->mr) {  // the padded slot layout, then compacted
            allgather(c, xloc, size_t(c->slot), c->xfull.as<double>());
            xg = c->xfull.as<double>();
            c->xexp.ensure(size_t(n) * 8);
            xc = c->xexp.as<double>();
            for (int r = 0; r < c->nranks; ++r) {
                const int64_t a = c->shard_off[size_t(r)], b = c->shard_off[size_t(r) + 1];
                if (b > a)
                    HIPCHK(hipMemcpyAsync(xc + a, xg + r * c->slot, size_t(b - a) * 8, hipMemcpyDeviceToDevice, s));
            }
            if (c->halo) {  // the residual's SpMV reads the compact layout: from the full vector, no collective
                ek::dev::gather_idx(s, xc, c->hx_gidx.as<int>(), (long long)x_extent(c), c->hx_X.as<double>());
                xg = c->hx_X.as<double>();
            }
        }
        HIPCHK(hipMemcpyAsync(v, xc, size_t(n) * 8, hipMemcpyDeviceToHost, s));
        const bool fin_fast = !c->mr;
        if (fin_fast) {
            if (!c->fin_ev) HIPCHK(hipEventCreateWithFlags(&c->fin_ev, hipEventDisableTiming));
            HIPCHK(hipEventRecord(c->fin_ev, s));
        }
        // residual ||L x - lambda x|| on the owned rows
        ek::dev::spmv(s, spmv_mat(c), xg, c->w.as<double>(), nullptr, nullptr, nullptr, nullptr);
        if (fin_fast) finish_single(out, tail);
        else finish_sharded(out);
    }

    // single context: the residual (a diagnostic) is reduced on the device
    // while the host scales the vector, and the final read-backs (residual
    // partials, the in-launch waits' state, the fp64-fallback count) land with
    // ONE synchronisation after fiedler_scale is queued.  (Reading the
    // 1.7 MB residual vector back, summing it on the host and syncing three
    // times left the GPU idle ~0.35 ms a solve at the headline.)
    void finish_single(const Result& out, size_t tail) {
        double* rpart = c->pin + size_t(n) + size_t(std::max<int64_t>(c->nrows, 1));  // nub <= tail - 8
        ek::dev::ProState* ps_pin = reinterpret_cast<ek::dev::ProState*>(rpart + tail - 8);
        unsigned* fb_pin = reinterpret_cast<unsigned*>(rpart + tail - 2);
        static_assert(sizeof(ek::dev::ProState) <= 6 * sizeof(double), "ProState overlaps the fallback count");
        ek::dev::resid_partial(s, L.ldv, c->w.as<double>(), xc, lambda, int(c->nrows), c->npart.as<double>());
        HIPCHK(hipMemcpyAsync(rpart, c->npart.p, size_t(L.nub) * 8, hipMemcpyDeviceToHost, s));
        if (L.pro) HIPCHK(hipMemcpyAsync(ps_pin, c->prost.p, sizeof(ek::dev::ProState), hipMemcpyDeviceToHost, s));
        if (L.b32) HIPCHK(hipMemcpyAsync(fb_pin, c->fbk.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventSynchronize(c->fin_ev));
        const double inv = 1.0 / std::sqrt(norm2_or_fail(true));
        const double sgn = signed_scale(inv);
        c->fied.ensure(size_t(n) * 8);
        c->fied_n = 0;  // set only once the solve is known good (a failed solve leaves no vector)
        ek::dev::fiedler_scale(s, xc, sgn, int(n), c->fied.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        if (L.proi) fail_on_timeouts(ps_pin->timeouts);
        c->fied_n = n;
        double rs = 0.0;
        for (int b = 0; b < L.nub; ++b) rs += rpart[b];
        const double r2 = rs * inv * inv;
        if (c->comm_time) comm_collect(c);
        deliver(out, sgn, r2, L.pro ? ps_pin->projected : L.matvecs, L.b32 ? int32_t(*fb_pin) : 0);
    }

    // sharded (or host-staged): the residual rows come back to the host, and
    // the ranks' sums are all-reduced
    void finish_sharded(const Result& out) {
        double* y = c->pin + n;
        if (c->nrows) HIPCHK(hipMemcpyAsync(y, c->w.p, size_t(c->nrows) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        double r2 = 0.0;
        const double inv = 1.0 / std::sqrt(norm2_or_fail(false));
        for (int64_t i = 0; i < c->nrows; ++i) {
            const double t = (y[i] - lambda * v[c->row0 + i]) * inv;
            r2 += t * t;
        }
        if (c->mr) {
            double* sc = c->scal.as<double>();
            HIPCHK(hipMemcpyAsync(sc, &r2, 8, hipMemcpyHostToDevice, s));
            allreduce(c, sc, 1);
            HIPCHK(hipMemcpyAsync(&r2, sc, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (L.proi) {
            ek::dev::ProState ps{};
            HIPCHK(hipMemcpyAsync(&ps, c->prost.p, sizeof(ps), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            fail_on_timeouts(ps.timeouts);
        }
        const double sgn = signed_scale(inv);
        c->fied.ensure(size_t(n) * 8);
        ek::dev::fiedler_scale(s, xc, sgn, int(n), c->fied.as<double>());
        HIPCHK(hipGetLastError());
        c->fied_n = n;
        if (c->comm_time) {
            HIPCHK(hipStreamSynchronize(s));
            comm_collect(c);
        }
        int projected = L.matvecs;  // every step projects unless partial reorthogonalisation ran
        int32_t fallbacks = 0;
        if (out.stats && L.pro) {
            ek::dev::ProState ps{};
            HIPCHK(hipMemcpyAsync(&ps, c->prost.p, sizeof(ps), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            projected = ps.projected;
        }
        if (out.stats && L.b32) {
            unsigned fbn = 0;
            HIPCHK(hipMemcpyAsync(&fbn, c->fbk.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            fallbacks = int32_t(fbn);
        }
        deliver(out, sgn, r2, projected, fallbacks);
    }
};

}  // namespace

extern "C" int ek_lanczos_fiedler(ek_ctx* c, const ek_lanczos_opts* opts, double* lambda_out, double* v_out,
                                  ek_lanczos_stats* stats) {
    EK_TRY
    check_ctx(c);
    if (!c->n) ek::fail(EK_ESTATE, "ek_lanczos_fiedler before ek_spmv_setup");
    Solve S(c, opts);
    S.plan();
    S.size_workspace();
    S.graph_signature();
    S.arm_workspace();
    S.start_vector();
    for (;;) {
        if (S.cycle() > 0) break;  // converged at a mid-cycle check
        if (S.ritz_converged() || ++S.restarts >= S.maxit) break;
        S.restart();
    }
    S.trace_times();
    if (!S.converged)
        ek::fail(EK_ENOCONV, "Eigenvalue computation failed: %d of %d Ritz pairs converged after %d restarts", S.nconv,
                 S.nev, S.restarts);
    S.finish({lambda_out, v_out, stats});
    return EK_OK;
    EK_CATCH
}

