// Host side of the smplify optimiser: work space, closure evaluation, the two backends of the device L-BFGS, C ABI.
//
// Reference: net/smplify/run.py:6-34 (smplify_runner: pre-check, optimise, per-frame update mask) and
// net/smplify/temporal_smplify.py:97-196 (parameters, closure, torch.optim.LBFGS). One closure evaluation is
// H2D of the parameter vector (300 B/frame), two kernels (rc_smplify.hip), D2H of the gradient and the per-frame loss
// terms (312 B/frame) -- so with RC_SMPLIFY_HOST_LBFGS=1, which runs rc_lbfgs.h on host vectors. By default the vectors
// stay on the device: rc_lbfgs_dev.h holds that optimiser once, and this file gives it a backend for one row at a time
// (rc_smplify_run) and one for a row of a lock-step batch (rc_smplify_run_batch). rc_lbfgs_device_probe (diagnostic) drives the same two
// backends through the same helpers (run_single_row, carve_batch, run_batch_rows) on a synthetic closure that tests restate exactly.
#include "../../include/robustcap_hip.h"
#include "rc_internal.h"
#include "rc_lbfgs_dev.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <sys/mman.h>
#include <ucontext.h>
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

constexpr size_t kPriorLd = 72, kPriorMat = 8 * 69 * kPriorLd;   // rc_smplify.hip: SM_PLD

struct SmplifyState {
    DevBuf<float> means, prec, lognll;                                // device; prec = [2][8][69][72]: P, then P + P^T, rows padded
    bool have_prior = false;
    int64_t cap = 0;                                                  // frames the buffers below hold
    DevBuf<float> x, grad;                                            // [cap*75] flat [aa | tran]
    DevBuf<float> ref3d, imu_aa, mj, proj, joint;
    DevBuf<float> terms;                                              // [3*cap] frame | imu | smooth losses
    DevBuf<int> argmin;
    DevBuf<float> prior_ll, prior_g;                                  // [cap], [cap*69]: outputs of the prior kernel
    DevBuf<float> fk;                                                 // [cap*432]: rotations of the forward kernel's primal
    DevBuf<float> res0, res1, Kd;                                     // residuals [cap,33] before / after, K on the device
    PinBuf<float> h_x, h_grad, h_terms, h_res;                        // pinned
    HipEvent ev0, ev1;
    double device_ms = 0.0;
    // device-resident L-BFGS (SingleRow): vectors of the optimiser, job table and partial sums of the inner products
    int64_t lb_cap = 0;                                               // frames the buffers below hold
    int lb_pairs = 0;                                                 // curvature pairs they hold
    DevBuf<float> xt, dir, gslot, Sv, Yv;                             // [n], [n], [6][n], [pairs][n] x 2
    DevBuf<VecJob> jobs_d; PinBuf<VecJob> jobs_h;                     // device / pinned
    DevBuf<double> part_d; PinBuf<double> part_h;
    const float* ref3d_override = nullptr;                            // rc_smplify_set_ref3d: caller-owned [T,33,3], next run only
    // arenas of rc_smplify_run_batch (grow-only: a second evaluation of the same size allocates nothing)
    DevBuf<char> batch_dev;
    PinBuf<char> batch_pin;
    size_t batch_dev_cap = 0, batch_pin_cap = 0;
};

namespace {

int state_of(rc_ctx* ctx, SmplifyState** out) {
    SmplifyOwner& s = rc_ctx_smplify(ctx);
    if (!s) {                                                         // (kept only once complete)
        SmplifyOwner f(new SmplifyState());
        HIP_TRY(ctx, rc_alloc_all(f->means, 8 * 69, f->prec, 2 * kPriorMat, f->lognll, 8, f->Kd, 9));
        HIP_TRY(ctx, hipEventCreate(rc_out(f->ev0)));
        HIP_TRY(ctx, hipEventCreate(rc_out(f->ev1)));
        s = std::move(f);
    }
    *out = s.get();
    return RC_OK;
}

int reserve(rc_ctx* ctx, SmplifyState* s, int64_t T) {
    const size_t n = (size_t)T;
    HIP_TRY(ctx, rc_grow(s->cap, n, n, s->x, n * 75, s->grad, n * 75, s->ref3d, n * 99, s->imu_aa, n * 18, s->mj, n * 99, s->proj, n * 66,
                         s->joint, n * 72, s->terms, n * 3, s->argmin, n, s->prior_ll, n, s->prior_g, n * 69, s->fk, n * 432, s->res0, n * 33,
                         s->res1, n * 33, s->h_x, n * 75, s->h_grad, n * 75, s->h_terms, n * 3, s->h_res, n * 66));
    return RC_OK;
}

// what one row lends a closure evaluation (SmplifyState and RowBuf both fill it); the prior comes from the context's state
struct RowPtrs {
    const float *kp, *ref3d, *imu_aa;
    float *mj, *proj, *terms, *prior_ll, *prior_g, *fk;               // terms: [3 T] frame | imu | smooth
    int* argmin;
    const float* K;
    int64_t T;
};
RowPtrs ptrs_of(SmplifyState* s, const float* kp, const float* ref3d, const float* imu_aa, const float* K, int64_t T) {
    return RowPtrs{kp, ref3d, imu_aa, s->mj.get(), s->proj.get(), s->terms.get(), s->prior_ll.get(), s->prior_g.get(), s->fk.get(), s->argmin.get(), K, T};
}

// closure at x (flat [aa | tran]) into grad
SmplifyArgs make_args(const SmplifyState* prior, const RowPtrs& p, const float* x, float* grad, unsigned long long ign_mask) {
    const int64_t T = p.T;
    SmplifyArgs A{};
    A.aa = x; A.tran = x + T * 72;
    A.kp = p.kp; A.ref3d = p.ref3d; A.imu_aa = p.imu_aa;
    A.means = prior->means.get(); A.prec = prior->prec.get(); A.prec_sym = prior->prec.get() + kPriorMat; A.lognll = prior->lognll.get();
    A.mj = p.mj; A.proj = p.proj;
    A.frame_loss = p.terms; A.imu_loss = p.terms + T; A.smooth_loss = p.terms + 2 * T;
    A.argmin = p.argmin; A.prior_ll = p.prior_ll; A.prior_g = p.prior_g; A.fk = p.fk;
    A.grad_aa = grad; A.grad_tran = grad + T * 72;
    for (int q = 0; q < 9; ++q) A.K[q] = p.K[q];
    A.ign_mask = ign_mask;
    A.T = (int)T;
    return A;
}

// total loss from the per-frame terms (losses.py:57-87): the IMU term is summed over the sequence and then added to
// EVERY frame before the final sum, i.e. it counts T times.
double total_loss(const float* terms, int64_t T) {
    double f = 0.0, imu = 0.0, sm = 0.0;
    for (int64_t t = 0; t < T; ++t) { f += terms[t]; imu += terms[T + t]; sm += terms[2 * T + t]; }
    return f + (double)T * imu + sm;
}

void set_info(rc_smplify_info* info, const rc::Lbfgs<float>::Result& r) {      // of a row that was optimised
    info->status = 1;
    info->n_iter = r.n_iter; info->n_eval = r.n_eval;
    info->first_loss = r.first_loss; info->final_loss = r.loss;
}

float frame_mean(const float* r) {                                    // torch mean(dim=-1) of 33 fp32 values
    float acc = 0.0f;
    for (int v = 0; v < 33; ++v) acc += r[v];
    return acc / 33.0f;
}

// ---------------------------------------------------------------------------------- L-BFGS with device-resident vectors
// rc_lbfgs_dev.h holds the algorithm; here are its two backends, which differ only in how a request reaches the device: SingleRow
// (rc_smplify_run) launches it at once on the SmplifyState buffers, BatchRow (rc_smplify_run_batch) hands it to the batch's executor.
// Per closure evaluation the host reads back the loss and five inner products (one kernel of partial sums), per iteration the Gram
// entries of the new curvature pair. No parameter or gradient vector crosses PCIe; round 2 moved 2 x 180 KB per evaluation and ran
// the recursion over 45,000-element host vectors (10 of the 13.8 ms per 600-frame row).
using Dev = rc::LbfgsDev<float>;
const int kSlots = Dev::kSlots, kSlotJobs = 5;

// RC_LBFGS_HISTORY: curvature pairs kept (default: torch's history_size, 100); read per call, by both formulations
int lbfgs_history_env() {
    const char* v = std::getenv("RC_LBFGS_HISTORY");
    const int h = v && *v ? std::atoi(v) : 100;
    return h < 1 ? 1 : h;
}

// curvature pairs the device formulation keeps (RC_LBFGS_HISTORY shrinks it for A/B tests); it holds one more physical slot
int lbfgs_pairs(int max_iter) { return std::max(1, std::min(std::min(max_iter, RC_LBFGS_MAX_PAIRS), lbfgs_history_env())); }

Dev::Options lbfgs_options(float lr, int max_iter) {
    Dev::Options o;
    o.lr = lr; o.max_iter = max_iter; o.max_eval = max_iter * 5 / 4; o.history_size = lbfgs_pairs(max_iter);
    return o;
}

// a job's partial sums (one per 4,096-element block), added in block order
double part_sum(const double* p, int nb, bool is_max) {
    double r = p[0];
    for (int b = 1; b < nb; ++b) r = is_max ? std::max(r, p[b]) : r + p[b];
    return r;
}

// the five inner products of an evaluation into gradient slot g with direction d -- g.d, max |g|, sum |g|, max |d|, g.g -- as jobs
// (op 0: sum a b, 1: max |a|, 2: sum |a|) and read back into Dev::Eval
const int kSlotOp[kSlotJobs] = {0, 1, 2, 1, 0};
template <class Job, class... Tail>
void slot_jobs(Job* j, const float* g, const float* d, Tail... tail) {
    const float *a[kSlotJobs] = {g, g, g, d, g}, *b[kSlotJobs] = {d, nullptr, nullptr, nullptr, g};
    for (int q = 0; q < kSlotJobs; ++q) j[q] = Job{a[q], b[q], kSlotOp[q], 0, tail...};
}
void read_slot(Dev::Eval& e, const double* part, int stride, int nb) {
    float* out[kSlotJobs] = {&e.gtd, &e.gmax, &e.gsum, &e.dmax, &e.gg};
    for (int q = 0; q < kSlotJobs; ++q) *out[q] = (float)part_sum(part + (size_t)q * stride, nb, kSlotOp[q] == 1);
}

// both backends: a direction's terms as the kernel's argument, a basis index as an address in the row's Sv / Yv / gslot
template <class Backend>
VecComb make_comb(const Backend& be, const Dev::Term* terms, int n_terms) {
    VecComb comb{};
    comb.n_vec = n_terms;
    for (int i = 0; i < n_terms; ++i) { comb.v[i] = be.vec(terms[i].vec); comb.c[i] = terms[i].coef; }
    return comb;
}
float* basis_vec(float* Sv, float* Yv, float* gslot, size_t n, int P, int i) {
    return i >= 2 * P ? gslot + (size_t)(i - 2 * P) * n : (i >= P ? Yv + (size_t)(i - P) * n : Sv + (size_t)i * n);
}

int reserve_lbfgs(rc_ctx* ctx, SmplifyState* s, int64_t T, int pairs) {
    if (T <= s->lb_cap && pairs <= s->lb_pairs) return RC_OK;
    s->lb_cap = 0; s->lb_pairs = 0;                                   // (capacity in frames AND pairs: either one short grows everything)
    const size_t n = (size_t)T * 75, nb = (n + 4095) / 4096;
    const size_t max_jobs = (size_t)kSlots * kSlotJobs + 6 * (size_t)pairs + 8;
    HIP_TRY(ctx, rc_grow(s->lb_cap, (size_t)T, (size_t)T, s->xt, n, s->dir, n, s->gslot, kSlots * n, s->Sv, (size_t)pairs * n, s->Yv, (size_t)pairs * n,
                         s->jobs_d, max_jobs, s->part_d, max_jobs * nb, s->jobs_h, max_jobs, s->part_h, max_jobs * nb));
    s->lb_pairs = pairs;
    return RC_OK;
}

// backend of rc_smplify_run: the state's buffers, every request launched at once. s->x is updated in place.
struct SingleRow {
    SmplifyState* s; const BodyConst* body; RowPtrs ptrs;
    int P;                                                            // physical pair slots
    hipStream_t st; unsigned long long ign;
    size_t n; int nb;                                                 // 75 T, 4,096-element blocks of a vector
    bool synthetic = false;                                           // rc_lbfgs_device_probe: the synthetic closure fills the slot and the terms
    hipError_t herr = hipSuccess;
    static constexpr int var0 = kSlots * kSlotJobs;                   // first job of the per-iteration (Gram) part of the table

    float* vec(int i) const { return basis_vec(s->Sv.get(), s->Yv.get(), s->gslot.get(), n, P, i); }
    // fixed part of the job table: the five products of every gradient slot
    bool begin() {
        for (int k = 0; k < kSlots; ++k) slot_jobs(s->jobs_h.get() + k * kSlotJobs, vec(2 * P + k), s->dir.get());
        herr = hipMemcpyAsync(s->jobs_d.get(), s->jobs_h.get(), (size_t)var0 * sizeof(VecJob), hipMemcpyHostToDevice, st);
        return herr == hipSuccess;
    }
    void dots(int job0, int n_jobs) {                                 // launch and read-back of jobs [job0, job0 + n_jobs)
        rc_launch_vec_dots(s->jobs_d.get() + job0, n_jobs, (long long)n, s->part_d.get() + (size_t)job0 * nb, st);
        if (herr == hipSuccess) herr = hipMemcpyAsync(s->part_h.get() + (size_t)job0 * nb, s->part_d.get() + (size_t)job0 * nb,
                                                      (size_t)n_jobs * nb * sizeof(double), hipMemcpyDeviceToHost, st);
    }
    bool eval(float t, int k, Dev::Eval& e) {
        const float* xp = s->x.get();
        if (t != 0.0f) { rc_launch_vec_axpy(s->x.get(), s->dir.get(), t, s->xt.get(), (long long)n, st); xp = s->xt.get(); }
        herr = hipEventRecord(s->ev0.get(), st);
        if (synthetic) rc_launch_syn_closure(make_args(s, ptrs, xp, vec(2 * P + k), ign), st);
        else rc_launch_smplify(make_args(s, ptrs, xp, vec(2 * P + k), ign), body, st);
        if (herr == hipSuccess) herr = hipEventRecord(s->ev1.get(), st);
        dots(k * kSlotJobs, kSlotJobs);
        if (herr == hipSuccess) herr = hipMemcpyAsync(s->h_terms.get(), s->terms.get(), (size_t)ptrs.T * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
        if (herr == hipSuccess) herr = hipStreamSynchronize(st);
        if (herr == hipSuccess) herr = hipGetLastError();
        if (herr != hipSuccess) return false;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s->ev0.get(), s->ev1.get()) == hipSuccess) s->device_ms += ms;
        e.f = (float)total_loss(s->h_terms.get(), ptrs.T);
        read_slot(e, s->part_h.get() + (size_t)k * kSlotJobs * nb, nb, nb);
        return true;
    }
    void direction(const Dev::Term* terms, int n_terms) { rc_launch_vec_comb(make_comb(*this, terms, n_terms), s->dir.get(), (long long)n, st); }
    void accept(float t) { rc_launch_vec_axpy(s->x.get(), s->dir.get(), t, s->x.get(), (long long)n, st); }   // (element-wise, in place)
    bool pair(int c, int g_new, int g_old, float t, const Dev::Want* want, int n_want, double* out) {
        rc_launch_vec_pair(vec(2 * P + g_new), vec(2 * P + g_old), s->dir.get(), t, vec(P + c), vec(c), (long long)n, st);
        for (int q = 0; q < n_want; ++q) s->jobs_h[var0 + q] = VecJob{vec(want[q].a), vec(want[q].b), 0, 0};
        herr = hipMemcpyAsync(s->jobs_d.get() + var0, s->jobs_h.get() + var0, (size_t)n_want * sizeof(VecJob), hipMemcpyHostToDevice, st);
        dots(var0, n_want);
        if (herr == hipSuccess) herr = hipStreamSynchronize(st);
        if (herr != hipSuccess) return false;
        for (int q = 0; q < n_want; ++q) out[q] = part_sum(s->part_h.get() + (size_t)(var0 + q) * nb, nb, false);
        return true;
    }
    bool flush() { return true; }
};

// the optimiser of one row on the state's buffers (rc_smplify_run, and rc_lbfgs_device_probe with backend 0): s->x holds the start
// and, afterwards, the result
int run_single_row(rc_ctx* ctx, SmplifyState* s, const BodyConst* body, const RowPtrs& ptrs, bool synthetic, const Dev::Options& opt,
                   hipStream_t st, Dev::Result& r) {
    const size_t n = (size_t)ptrs.T * 75;
    const int P = opt.history_size + 1;
    if (int rc = reserve_lbfgs(ctx, s, ptrs.T, P)) return rc;
    SingleRow be{s, body, ptrs, P, st, rc_ctx_ign_mask(ctx), n, (int)((n + 4095) / 4096), synthetic};
    if (!be.begin() || !Dev::minimize(be, opt, r))
        return rc_ctx_fail(ctx, RC_ERR_HIP, (std::string("smplify L-BFGS: ") + hipGetErrorString(be.herr)).c_str());
    return RC_OK;
}

// ================================================================== lock-step batch of rows (rc_smplify_run_batch, round 4)
// evaluate.py:86-90 refines the (sequence, camera) rows of an evaluation one after another; they are independent optimisation
// problems. Round 3 drove them from host threads, one context and stream each: ~300 HIP calls per row contend for the runtime,
// 72 rows of 600 frames took 0.19-0.23 s however many threads ran. Here every row's optimiser (rc::LbfgsDev on a BatchRow, as a fiber
// of the caller's thread -- a stack of its own, see RowBatch::fibers) hands its next device request -- "evaluate the closure at
// x + t d into gradient slot k", or "form the curvature pair and these inner products" -- to ONE executor; when every live row has
// asked, the executor runs all requests with one launch per kind over all rows (descriptor tables in device memory, the row from
// blockIdx.y), one read-back, one synchronisation, and resumes the rows. A round costs what its largest kernel costs; per row the
// arithmetic is the same chain of operations as alone, so n_iter / n_eval / losses are those of the one-row-at-a-time run.
struct RowBuf {                       // device vectors of one row (carved from the batch's arena)
    int64_t T = 0;
    size_t n = 0;                     // 75 T
    int nb = 0;                       // 4,096-element blocks of a vector
    float *x = nullptr, *xt = nullptr, *dir = nullptr, *gslot = nullptr, *Sv = nullptr, *Yv = nullptr;
    float *ref3d = nullptr, *imu_aa = nullptr, *mj = nullptr, *proj = nullptr, *joint = nullptr, *res0 = nullptr, *res1 = nullptr;
    float* terms = nullptr;           // [3 T] frame | imu | smooth, device (inside the terms arena)
    const float* terms_h = nullptr;   // the same region of the pinned copy
    int* argmin = nullptr;
    float *prior_ll = nullptr, *prior_g = nullptr, *fk = nullptr;
    float *h_res0 = nullptr, *h_res1 = nullptr;   // pinned [33 T] each: residual before / after
    float K[9];
    const float* kp = nullptr;
};

RowPtrs ptrs_of(const RowBuf& b) { return RowPtrs{b.kp, b.ref3d, b.imu_aa, b.mj, b.proj, b.terms, b.prior_ll, b.prior_g, b.fk, b.argmin, b.K, b.T}; }

struct RowReq {
    int kind = 0;                     // 1: closure evaluation, 2: curvature pair + inner products, 3: pending update of x only
    bool has_comb = false;            // dir = combination, in front of everything else (start of a line search)
    VecComb comb{};
    bool accept = false;              // x += accept_t * dir (the step the previous line search accepted)
    float accept_t = 0.0f;
    float t = 0.0f;                   // kind 1: evaluate at x + t * dir into gradient slot k
    int k = 0;
    const float *g_new = nullptr, *g_old = nullptr;   // kind 2: y = g_new - g_old -> yv, s = pair_t * dir -> sv
    float *yv = nullptr, *sv = nullptr;
    float pair_t = 0.0f;
    std::vector<VecJobN> jobs;        // inner products wanted (kind 1: the slot's five, kind 2: the Gram entries)
    int job0 = 0;                     // filled by the executor: first job of this row in the round's table
    int arg0 = -1;                    // ... and, kind 1, the row's entry of the round's closure table (its total loss comes back there)
};

class RowBatch {
  public:
    rc_ctx* ctx = nullptr;
    const BodyConst* body = nullptr;
    SmplifyState* prior = nullptr;
    hipStream_t st = nullptr;
    unsigned long long ign = 0;
    std::vector<RowBuf> row;
    int T_max = 0, nb_max = 0, max_jobs = 0;
    size_t n_max = 0;
    // arenas
    char* dev = nullptr; size_t dev_bytes = 0;
    char* pin = nullptr; size_t pin_bytes = 0;
    SmplifyArgs *args_d = nullptr, *args_h = nullptr;
    VecOp *ops_d = nullptr, *ops_h = nullptr;
    VecCombRow *comb_d = nullptr, *comb_h = nullptr;
    VecJobN *jobs_d = nullptr, *jobs_h = nullptr;
    double *part_d = nullptr, *part_h = nullptr;
    float *terms_d = nullptr, *terms_h = nullptr;
    double *total_d = nullptr, *total_h = nullptr;                       // total loss per closure-table entry of the round
    bool device_totals = true;                                           // RC_SMPLIFY_DEVICE_TOTALS=0: read the per-frame terms back and add them on the host (A/B)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;                              // (the events and the arenas belong to the context's SmplifyState)
    double device_ms = 0.0, round_ms = 0.0;                              // closure kernels (events) / wall time inside run_round
    int rounds = 0;
    int max_round_jobs = 0;                                              // the largest job table a round sent
    bool synthetic = false;                                              // rc_lbfgs_device_probe: the synthetic closure fills the slots and the terms
    std::vector<RowReq*> pending;                                        // the live rows' next requests
    hipError_t herr = hipSuccess;
    // Several live rows run as fibers: every row's optimiser on a stack of its own inside the CALLER's thread; submit() switches back to
    // the scheduler in run_batch_rows, which runs the round when every live row has asked and resumes them one after another. No thread
    // is created, woken or left spinning (72 condition-variable wake-ups cost 0.27 ms per round, 8.7 of config 3's 40 ms). One live row
    // runs inline: its request is the round.
    bool fibers = false;
    ucontext_t sched{};
    std::vector<ucontext_t> fctx;

    const double* part_of(const RowReq& q, int j) const { return part_h + (size_t)(q.job0 + j) * nb_max; }   // partial sums of the request's job j
    // hand in the row's request and come back when the round it belongs to has run; false = a HIP call failed
    bool submit(int r, RowReq* q) {
        pending[r] = q;
        if (fibers) swapcontext(&fctx[r], &sched);
        else run_round();
        return herr == hipSuccess;
    }
    void leave(int r) { pending[r] = nullptr; }

    void run_round() {                                                   // (every live row is waiting)
        const auto t_round = std::chrono::steady_clock::now();
        int n_args = 0, n_ops = 0, n_comb = 0, n_jobs = 0;
        for (size_t r = 0; r < row.size(); ++r) {
            RowReq* q = pending[r];
            if (!q) continue;
            const RowBuf& b = row[r];
            if (q->has_comb) { comb_h[n_comb].c = q->comb; comb_h[n_comb].out = b.dir; comb_h[n_comb].n = (long long)b.n; ++n_comb; }
            if (q->accept) ops_h[n_ops++] = VecOp{b.x, b.dir, nullptr, b.x, nullptr, q->accept_t, 0, (long long)b.n};
            if (q->kind == 1) {
                const float* xp = b.x;
                if (q->t != 0.0f) { ops_h[n_ops++] = VecOp{b.x, b.dir, nullptr, b.xt, nullptr, q->t, 0, (long long)b.n}; xp = b.xt; }
                q->arg0 = n_args;
                args_h[n_args++] = make_args(prior, ptrs_of(b), xp, b.gslot + (size_t)q->k * b.n, ign);
            } else if (q->kind == 2) {
                ops_h[n_ops++] = VecOp{q->g_new, q->g_old, b.dir, q->yv, q->sv, q->pair_t, 1, (long long)b.n};
            }
            q->job0 = n_jobs;
            for (const VecJobN& j : q->jobs) jobs_h[n_jobs++] = j;
        }
        auto up = [&](void* d, const void* h, size_t bytes) {
            if (bytes && herr == hipSuccess) herr = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st);
        };
        up(comb_d, comb_h, (size_t)n_comb * sizeof(VecCombRow));
        up(ops_d, ops_h, (size_t)n_ops * sizeof(VecOp));
        up(args_d, args_h, (size_t)n_args * sizeof(SmplifyArgs));
        up(jobs_d, jobs_h, (size_t)n_jobs * sizeof(VecJobN));
        // A row's accept / evaluation-point / pair operations read dir: the combination that WRITES dir goes first. Within the
        // op table a row's accept (x += t d) stands in front of whatever reads x.
        rc_launch_vec_comb_rows(comb_d, n_comb, (long long)n_max, st);
        // two op launches: updates of x first (the evaluation point x + t d of the same request reads the new x)
        {
            int n_acc = 0;
            for (int i = 0; i < n_ops; ++i) if (ops_h[i].kind == 0 && ops_h[i].out == ops_h[i].a) ++n_acc;
            if (n_acc > 0 && n_acc < n_ops) {                            // partition: in-place updates | the rest (stable)
                std::vector<VecOp> a, b;
                for (int i = 0; i < n_ops; ++i) ((ops_h[i].kind == 0 && ops_h[i].out == ops_h[i].a) ? a : b).push_back(ops_h[i]);
                std::copy(a.begin(), a.end(), ops_h);
                std::copy(b.begin(), b.end(), ops_h + a.size());
                up(ops_d, ops_h, (size_t)n_ops * sizeof(VecOp));
                rc_launch_vec_ops(ops_d, n_acc, (long long)n_max, st);
                rc_launch_vec_ops(ops_d + n_acc, n_ops - n_acc, (long long)n_max, st);
            } else rc_launch_vec_ops(ops_d, n_ops, (long long)n_max, st);
        }
        if (n_args > 0) {
            if (herr == hipSuccess) herr = hipEventRecord(ev0, st);
            if (synthetic) rc_launch_syn_closure_rows(args_d, n_args, T_max, st);
            else rc_launch_smplify_rows(args_d, n_args, T_max, body, st);
            if (herr == hipSuccess) herr = hipEventRecord(ev1, st);
            if (device_totals) rc_launch_smplify_totals(args_d, n_args, total_d, st);
        }
        rc_launch_vec_dots_rows(jobs_d, n_jobs, nb_max, part_d, st);
        if (n_jobs > 0 && herr == hipSuccess)
            herr = hipMemcpyAsync(part_h, part_d, (size_t)n_jobs * nb_max * sizeof(double), hipMemcpyDeviceToHost, st);
        if (n_args > 0 && herr == hipSuccess)
            herr = device_totals ? hipMemcpyAsync(total_h, total_d, (size_t)n_args * sizeof(double), hipMemcpyDeviceToHost, st)
                                 : hipMemcpyAsync(terms_h, terms_d, row.size() * (size_t)3 * T_max * sizeof(float), hipMemcpyDeviceToHost, st);
        if (herr == hipSuccess) herr = hipStreamSynchronize(st);
        if (herr == hipSuccess) herr = hipGetLastError();
        if (n_args > 0 && herr == hipSuccess) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) device_ms += ms;
        }
        ++rounds;
        max_round_jobs = std::max(max_round_jobs, n_jobs);
        round_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_round).count();
    }
};

// backend of rc_smplify_run_batch for row r: every request goes to the batch's executor. The direction and the accepted step are not
// requests of their own: they ride in front of the next one (or of the final flush), so that a round is one request per row.
struct BatchRow {
    RowBatch& B; const int r; const RowBuf& b;
    const int P;                                                      // physical pair slots
    RowReq q;
    bool have_comb = false, have_accept = false;                      // pending: dir = comb, x += accept_t * dir
    VecComb comb{};
    float accept_t = 0.0f;

    float* vec(int i) const { return basis_vec(b.Sv, b.Yv, b.gslot, b.n, P, i); }
    bool submit(int kind) {
        q.kind = kind;
        q.has_comb = have_comb; if (have_comb) q.comb = comb;
        q.accept = have_accept; q.accept_t = accept_t;
        have_comb = false; have_accept = false;
        return B.submit(r, &q);
    }
    bool eval(float t, int k, Dev::Eval& e) {
        q.t = t; q.k = k;
        q.jobs.resize(kSlotJobs);
        slot_jobs(q.jobs.data(), vec(2 * P + k), b.dir, (long long)b.n);
        if (!submit(1)) return false;
        e.f = (float)(B.device_totals ? B.total_h[q.arg0] : total_loss(b.terms_h, b.T));
        read_slot(e, B.part_of(q, 0), B.nb_max, b.nb);
        return true;
    }
    void direction(const Dev::Term* terms, int n_terms) { comb = make_comb(*this, terms, n_terms); have_comb = true; }   // with the next evaluation
    void accept(float t) { have_accept = true; accept_t = t; }           // x += t d: with the next request (or the final flush)
    bool pair(int c, int g_new, int g_old, float t, const Dev::Want* want, int n_want, double* out) {
        q.g_new = vec(2 * P + g_new); q.g_old = vec(2 * P + g_old); q.pair_t = t;
        q.yv = vec(P + c); q.sv = vec(c);
        q.jobs.clear();
        for (int i = 0; i < n_want; ++i) q.jobs.push_back(VecJobN{vec(want[i].a), vec(want[i].b), 0, 0, (long long)b.n});
        if (!submit(2)) return false;
        for (int i = 0; i < n_want; ++i) out[i] = part_sum(B.part_of(q, i), b.nb, false);
        return true;
    }
    bool flush() { have_comb = false; q.jobs.clear(); return !have_accept || submit(3); }   // the last accepted step
};

void lbfgs_batch_row(RowBatch& B, int r, float lr, int max_iter, Dev::Result& res, char& ok) {
    struct Leave { RowBatch& B; int r; ~Leave() { B.leave(r); } } on_exit{B, r};
    const Dev::Options o = lbfgs_options(lr, max_iter);
    BatchRow be{B, r, B.row[r], o.history_size + 1};
    ok = Dev::minimize(be, o, res) ? 1 : 0;
}

}  // namespace

void rc_smplify_free(SmplifyState* s) { delete s; }

extern "C" {

int rc_smplify_set_prior(rc_ctx* ctx, const float* means, const float* prec, const float* nllw) {
    if (!ctx) return RC_ERR_INVALID;
    if (!means || !prec || !nllw) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_set_prior: null buffer");
    SmplifyState* s = nullptr;
    if (int rc = state_of(ctx, &s)) return rc;
    float lg[8];
    for (int m = 0; m < 8; ++m) {
        if (!(nllw[m] > 0.0f)) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_set_prior: nll_weights must be positive");
        lg[m] = logf(nllw[m]);
    }
    HIP_TRY(ctx, hipMemcpy(s->means.get(), means, 8 * 69 * sizeof(float), hipMemcpyHostToDevice));
    // rows padded to 72 floats (32-byte aligned for the prior kernel's scalar loads); the second half is P + P^T, the matrix of the
    // gradient of d^T P d (the fp32 sum the gradient kernel used to form per element)
    std::vector<float> pad(2 * kPriorMat, 0.0f);
    for (int m = 0; m < 8; ++m)
        for (int i = 0; i < 69; ++i)
            for (int j = 0; j < 69; ++j) {
                const float a = prec[((size_t)m * 69 + i) * 69 + j], b = prec[((size_t)m * 69 + j) * 69 + i];
                pad[((size_t)m * 69 + i) * kPriorLd + j] = a;
                pad[kPriorMat + ((size_t)m * 69 + i) * kPriorLd + j] = a + b;
            }
    HIP_TRY(ctx, hipMemcpy(s->prec.get(), pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(s->lognll.get(), lg, sizeof(lg), hipMemcpyHostToDevice));
    s->have_prior = true;
    return RC_OK;
}

int rc_smplify_set_ref3d(rc_ctx* ctx, const float* ref3d) {
    if (!ctx) return RC_ERR_INVALID;
    SmplifyState* s = nullptr;
    if (int rc = state_of(ctx, &s)) return rc;
    s->ref3d_override = ref3d;
    return RC_OK;
}

int rc_smplify_run(rc_ctx* ctx, const float* pose, const float* tran, const float* kp, const float* imu_ori, const float* K,
                   int64_t T, float lr, int32_t max_iter, float loss_threshold, float* pose_out, float* tran_out,
                   uint8_t* update, rc_smplify_info* info, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const auto t_begin = std::chrono::steady_clock::now();
    const BodyConst* body = rc_ctx_body(ctx);
    if (!body) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_smplify_run: body not set");
    SmplifyState* s = nullptr;
    if (int rc = state_of(ctx, &s)) return rc;
    if (!s->have_prior) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_smplify_run: prior not set (rc_smplify_set_prior)");
    if (T <= 0 || T > 0x7fffffff / 99 || max_iter < 1 || !(lr >= 0.0f))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_run: bad arguments");
    if (!pose || !tran || !kp || !imu_ori || !K || !pose_out || !tran_out || !update || !info)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_run: null buffer");
    if (int rc = reserve(ctx, s, T)) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::memset(info, 0, sizeof(*info));
    std::memset(update, 0, (size_t)T);
    s->device_ms = 0.0;

    // pre-check (run.py:24-29): mean residual of the FIRST frame against the threshold
    HIP_TRY(ctx, hipMemcpyAsync(s->Kd.get(), K, 9 * sizeof(float), hipMemcpyHostToDevice, st));
    rc_launch_residual(body, pose, tran, kp, s->Kd.get(), 100.0f, rc_ctx_ign_mask(ctx), s->res0.get(), T, st);
    HIP_TRY(ctx, hipMemcpyAsync(s->h_res.get(), s->res0.get(), (size_t)T * 33 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (frame_mean(s->h_res.get()) > loss_threshold) {
        if (pose_out != pose) HIP_TRY(ctx, hipMemcpyAsync(pose_out, pose, (size_t)T * 216 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (tran_out != tran) HIP_TRY(ctx, hipMemcpyAsync(tran_out, tran, (size_t)T * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        info->status = 0;
        info->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        return RC_OK;
    }

    // parameters and constants of the closure (temporal_smplify.py:111-139)
    rc_launch_R2aa(pose, s->x.get(), T * 24, st);                                            // body_pose = axis-angle of the prediction
    HIP_TRY(ctx, hipMemcpyAsync(s->x.get() + T * 72, tran, (size_t)T * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc_launch_R2aa(imu_ori, s->imu_aa.get(), T * 6, st);
    if (s->ref3d_override) {                                                           // see rc_smplify_set_ref3d
        HIP_TRY(ctx, hipMemcpyAsync(s->ref3d.get(), s->ref3d_override, (size_t)T * 99 * sizeof(float), hipMemcpyDeviceToDevice, st));
        s->ref3d_override = nullptr;
    } else {
        rc_launch_body_fk(body, pose, tran, nullptr, s->joint.get(), s->ref3d.get(), T, st);      // preserved 3D landmarks
    }
    HIP_TRY(ctx, hipMemcpyAsync(s->h_x.get(), s->x.get(), (size_t)T * 75 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    using L = rc::Lbfgs<float>;
    const size_t n = (size_t)T * 75;
    const RowPtrs ptrs = ptrs_of(s, kp, s->ref3d.get(), s->imu_aa.get(), K, T);
    const L::Options opt = lbfgs_options(lr, max_iter);
    L::Result r;
    const char* hv = std::getenv("RC_SMPLIFY_HOST_LBFGS");            // read per call: tests flip it
    if (!(hv && std::atoi(hv) != 0)) {
        // the optimiser's vectors stay on the device (rc_lbfgs_dev.h on a SingleRow); s->x.get() is updated in place
        if (int rc = run_single_row(ctx, s, body, ptrs, false, opt, st, r)) return rc;
    } else {
        // RC_SMPLIFY_HOST_LBFGS=1: round 2's formulation (vectors on the host, rc_lbfgs.h run as is) for A/B runs
        L::Vec x(s->h_x.get(), s->h_x.get() + n);
        int hip_rc = RC_OK;
        const SmplifyArgs A = make_args(s, ptrs, s->x.get(), s->grad.get(), rc_ctx_ign_mask(ctx));
        L::Objective closure = [&](const L::Vec& xv, L::Vec& g) -> float {
            std::memcpy(s->h_x.get(), xv.data(), n * sizeof(float));
            hipError_t e = hipMemcpyAsync(s->x.get(), s->h_x.get(), n * sizeof(float), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(s->ev0.get(), st);
            rc_launch_smplify(A, body, st);
            if (e == hipSuccess) e = hipEventRecord(s->ev1.get(), st);
            if (e == hipSuccess) e = hipMemcpyAsync(s->h_grad.get(), s->grad.get(), n * sizeof(float), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(s->h_terms.get(), s->terms.get(), (size_t)T * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) e = hipGetLastError();
            if (e != hipSuccess) {
                if (hip_rc == RC_OK) hip_rc = rc_ctx_fail(ctx, RC_ERR_HIP, (std::string("smplify closure: ") + hipGetErrorString(e)).c_str());
                std::fill(g.begin(), g.end(), 0.0f);            // zero gradient terminates the search
                return 0.0f;
            }
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, s->ev0.get(), s->ev1.get()) == hipSuccess) s->device_ms += ms;
            std::memcpy(g.data(), s->h_grad.get(), n * sizeof(float));
            return (float)total_loss(s->h_terms.get(), T);
        };
        L::Options host_opt = opt;
        host_opt.history_size = lbfgs_history_env();
        r = L::minimize(closure, x, host_opt);
        if (hip_rc != RC_OK) return hip_rc;
        std::memcpy(s->h_x.get(), x.data(), n * sizeof(float));
        HIP_TRY(ctx, hipMemcpyAsync(s->x.get(), s->h_x.get(), n * sizeof(float), hipMemcpyHostToDevice, st));
    }

    // results (temporal_smplify.py:188-196, run.py:31-34): rotation matrices, new residual, per-frame update mask
    rc_launch_aa2R(s->x.get(), pose_out, T * 24, st);
    HIP_TRY(ctx, hipMemcpyAsync(tran_out, s->x.get() + T * 72, (size_t)T * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc_launch_residual(body, pose_out, tran_out, kp, s->Kd.get(), 100.0f, rc_ctx_ign_mask(ctx), s->res1.get(), T, st);
    HIP_TRY(ctx, hipMemcpyAsync(s->h_res.get() + T * 33, s->res1.get(), (size_t)T * 33 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipGetLastError());
    for (int64_t t = 0; t < T; ++t) update[t] = frame_mean(s->h_res.get() + (T + t) * 33) < frame_mean(s->h_res.get() + t * 33) ? 1 : 0;
    set_info(info, r);
    info->device_ms = s->device_ms;
    info->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return RC_OK;
}

namespace {
struct FiberArg { RowBatch* B; int r; float lr; int max_iter; Dev::Result* res; char* ok; };
void fiber_main(unsigned lo, unsigned hi) {
    FiberArg* a = reinterpret_cast<FiberArg*>(((uintptr_t)hi << 32) | (uintptr_t)lo);
    lbfgs_batch_row(*a->B, a->r, a->lr, a->max_iter, *a->res, *a->ok);
}

// rows and arenas of a batch (rc_smplify_run_batch, rc_lbfgs_device_probe with backend 1, and one row without pairs for
// rc_smplify_loss_grad): every row's geometry, then two arenas
// (device, pinned) carved into the rows' vectors and the round's tables. K_host: [n_rows, 9]; kp: per row, what RowBuf::kp lends the closure.
struct BatchCarve { size_t r0_begin = 0, r1_begin = 0, r_bytes = 0, p_r0 = 0, p_r1 = 0, o_io = 0, p_io = 0; };
int carve_batch(rc_ctx* ctx, SmplifyState* s0, RowBatch& B, int n_rows, const int64_t* T_rows, const float* K_host, const float* const* kp,
                int P, BatchCarve& c) {
    B.row.resize((size_t)n_rows);
    B.pending.assign((size_t)n_rows, nullptr);
    B.max_jobs = 6 * P + 8;
    for (int r = 0; r < n_rows; ++r) {
        RowBuf& b = B.row[r];
        b.T = T_rows[r]; b.n = (size_t)b.T * 75; b.nb = (int)((b.n + 4095) / 4096);
        for (int e = 0; e < 9; ++e) b.K[e] = K_host[9 * r + e];
        b.kp = kp[r];
        B.T_max = std::max(B.T_max, (int)b.T);
        B.n_max = std::max(B.n_max, b.n);
        B.nb_max = std::max(B.nb_max, b.nb);
    }
    // ---- two arenas (device, pinned), carved: two allocations for the whole batch
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t dev_need = 0, pin_need = 0;
    auto dtake = [&](size_t bytes) { const size_t o = dev_need; dev_need += al(bytes); return o; };
    auto ptake = [&](size_t bytes) { const size_t o = pin_need; pin_need += al(bytes); return o; };
    struct Off { size_t x, xt, dir, gs, Sv, Yv, ref, imu, mj, proj, joint, r0, r1, am, pl, pg, fk; };
    std::vector<Off> off((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const size_t n = B.row[r].n, T = (size_t)B.row[r].T;
        Off& o = off[r];
        o.x = dtake(n * 4); o.xt = dtake(n * 4); o.dir = dtake(n * 4); o.gs = dtake(kSlots * n * 4);
        o.Sv = dtake((size_t)P * n * 4); o.Yv = dtake((size_t)P * n * 4);
        o.ref = dtake(T * 99 * 4); o.imu = dtake(T * 18 * 4); o.mj = dtake(T * 99 * 4); o.proj = dtake(T * 66 * 4); o.joint = dtake(T * 72 * 4);
        o.am = dtake(T * 4); o.pl = dtake(T * 4); o.pg = dtake(T * 69 * 4); o.fk = dtake(T * 432 * 4);
    }
    // the residuals of all rows in one span each (one read-back per span; the pinned copies mirror the offsets)
    const size_t r0_begin = c.r0_begin = dev_need;
    for (int r = 0; r < n_rows; ++r) off[r].r0 = dtake((size_t)B.row[r].T * 33 * 4);
    const size_t r_bytes = c.r_bytes = dev_need - r0_begin, r1_begin = c.r1_begin = dev_need;
    for (int r = 0; r < n_rows; ++r) off[r].r1 = dtake((size_t)B.row[r].T * 33 * 4);
    const size_t p_r0 = c.p_r0 = ptake(r_bytes), p_r1 = c.p_r1 = ptake(r_bytes);
    const size_t nr = (size_t)n_rows;
    c.o_io = dtake(nr * sizeof(SmplifyRowIO)); c.p_io = ptake(nr * sizeof(SmplifyRowIO));
    const size_t o_args = dtake(nr * sizeof(SmplifyArgs)), o_ops = dtake(3 * nr * sizeof(VecOp)), o_comb = dtake(nr * sizeof(VecCombRow));
    const size_t o_jobs = dtake(nr * B.max_jobs * sizeof(VecJobN)), o_part = dtake(nr * B.max_jobs * (size_t)B.nb_max * sizeof(double));
    const size_t o_terms = dtake(nr * 3 * (size_t)B.T_max * 4);
    const size_t o_total = dtake(nr * sizeof(double)), p_total = ptake(nr * sizeof(double));
    const size_t p_args = ptake(nr * sizeof(SmplifyArgs)), p_ops = ptake(3 * nr * sizeof(VecOp)), p_comb = ptake(nr * sizeof(VecCombRow));
    const size_t p_jobs = ptake(nr * B.max_jobs * sizeof(VecJobN)), p_part = ptake(nr * B.max_jobs * (size_t)B.nb_max * sizeof(double));
    const size_t p_terms = ptake(nr * 3 * (size_t)B.T_max * 4);
    HIP_TRY(ctx, rc_grow(s0->batch_dev_cap, dev_need, dev_need, s0->batch_dev, dev_need));
    HIP_TRY(ctx, rc_grow(s0->batch_pin_cap, pin_need, pin_need, s0->batch_pin, pin_need));
    B.dev = s0->batch_dev.get(); B.pin = s0->batch_pin.get();
    B.dev_bytes = dev_need; B.pin_bytes = pin_need;
    B.ev0 = s0->ev0.get(); B.ev1 = s0->ev1.get();
    B.args_d = (SmplifyArgs*)(B.dev + o_args); B.ops_d = (VecOp*)(B.dev + o_ops); B.comb_d = (VecCombRow*)(B.dev + o_comb);
    B.jobs_d = (VecJobN*)(B.dev + o_jobs); B.part_d = (double*)(B.dev + o_part); B.terms_d = (float*)(B.dev + o_terms);
    B.args_h = (SmplifyArgs*)(B.pin + p_args); B.ops_h = (VecOp*)(B.pin + p_ops); B.comb_h = (VecCombRow*)(B.pin + p_comb);
    B.jobs_h = (VecJobN*)(B.pin + p_jobs); B.part_h = (double*)(B.pin + p_part); B.terms_h = (float*)(B.pin + p_terms);
    B.total_d = (double*)(B.dev + o_total); B.total_h = (double*)(B.pin + p_total);
    if (const char* e = std::getenv("RC_SMPLIFY_DEVICE_TOTALS"); e && *e == '0') B.device_totals = false;
    for (int r = 0; r < n_rows; ++r) {
        RowBuf& b = B.row[r];
        const Off& o = off[r];
        auto f = [&](size_t q) { return (float*)(B.dev + q); };
        b.x = f(o.x); b.xt = f(o.xt); b.dir = f(o.dir); b.gslot = f(o.gs); b.Sv = f(o.Sv); b.Yv = f(o.Yv);
        b.ref3d = f(o.ref); b.imu_aa = f(o.imu); b.mj = f(o.mj); b.proj = f(o.proj); b.joint = f(o.joint); b.res0 = f(o.r0); b.res1 = f(o.r1);
        b.argmin = (int*)(B.dev + o.am); b.prior_ll = f(o.pl); b.prior_g = f(o.pg); b.fk = f(o.fk);
        b.h_res0 = (float*)(B.pin + p_r0 + (o.r0 - r0_begin));
        b.h_res1 = (float*)(B.pin + p_r1 + (o.r1 - r1_begin));
        b.terms = B.terms_d + (size_t)r * 3 * B.T_max;
        b.terms_h = B.terms_h + (size_t)r * 3 * B.T_max;
    }
    return RC_OK;
}

// the optimisers of the live rows: one row inline, several as a fiber each, the device work in lock-step rounds
int run_batch_rows(rc_ctx* ctx, RowBatch& B, const std::vector<int>& live, float lr, int max_iter, std::vector<Dev::Result>& res) {
    const int n_rows = (int)B.row.size();
    res.assign((size_t)n_rows, Dev::Result());
    std::vector<char> ok((size_t)n_rows, 0);
    if (live.size() == 1) {
        lbfgs_batch_row(B, live[0], lr, max_iter, res[live[0]], ok[live[0]]);
    } else if (!live.empty()) {
        B.fibers = true;
        B.fctx.resize((size_t)n_rows);
        // a stack per row with an inaccessible page below it (round-4 advice: in one plain array an overflow ran silently into the
        // neighbouring row's stack; now it faults at the guard page)
        constexpr size_t kStack = 256u << 10;
        const size_t page = (size_t)sysconf(_SC_PAGESIZE), slot = kStack + page;
        struct Stacks {
            void* p = MAP_FAILED; size_t n = 0;
            ~Stacks() { if (p != MAP_FAILED) munmap(p, n); }
        } stacks;
        stacks.n = slot * live.size();
        stacks.p = mmap(nullptr, stacks.n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (stacks.p == MAP_FAILED) return rc_ctx_fail(ctx, RC_ERR_HIP, "smplify batch: cannot map the rows' stacks");
        for (size_t i = 0; i < live.size(); ++i) (void)mprotect((char*)stacks.p + i * slot, page, PROT_NONE);
        std::vector<FiberArg> fa(live.size());
        for (size_t i = 0; i < live.size(); ++i) {
            const int r = live[i];
            fa[i] = FiberArg{&B, r, lr, (int)max_iter, &res[r], &ok[r]};
            getcontext(&B.fctx[r]);
            B.fctx[r].uc_stack.ss_sp = (char*)stacks.p + i * slot + page;
            B.fctx[r].uc_stack.ss_size = kStack;
            B.fctx[r].uc_link = &B.sched;
            const uintptr_t p = (uintptr_t)&fa[i];
            makecontext(&B.fctx[r], (void (*)())fiber_main, 2, (unsigned)(p & 0xffffffffu), (unsigned)(p >> 32));
        }
        std::vector<int> run(live);
        while (!run.empty()) {
            for (int r : run) swapcontext(&B.sched, &B.fctx[r]);          // to the row's next request, or to its end
            run.clear();
            for (int r : live) if (B.pending[r]) run.push_back(r);
            if (!run.empty()) B.run_round();                              // every live row is waiting
        }
    }
    if (B.herr != hipSuccess) return rc_ctx_fail(ctx, RC_ERR_HIP, (std::string("smplify batch: ") + hipGetErrorString(B.herr)).c_str());
    for (int r : live) if (!ok[r]) return rc_ctx_fail(ctx, RC_ERR_HIP, "smplify batch: a row's optimiser did not finish");
    return RC_OK;
}
}  // namespace

int rc_smplify_loss_grad(rc_ctx* ctx, const float* x, const float* kp, const float* ref3d, const float* imu_aa, const float* K,
                         int64_t T, double* loss, float* grad, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const BodyConst* body = rc_ctx_body(ctx);
    if (!body) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_smplify_loss_grad: body not set");
    SmplifyState* s = nullptr;
    if (int rc = state_of(ctx, &s)) return rc;
    if (!s->have_prior) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_smplify_loss_grad: prior not set (rc_smplify_set_prior)");
    if (T < 0 || T > 0x7fffffff / 99 || !loss) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_loss_grad: bad arguments");
    if (T == 0) { *loss = 0.0; return RC_OK; }
    if (!x || !kp || !ref3d || !imu_aa || !K || !grad) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_loss_grad: null buffer");
    hipStream_t st = (hipStream_t)stream;
    RowBatch B;                                                       // a batch of one row without curvature pairs: the closure's work space
    BatchCarve cv;
    if (int rc = carve_batch(ctx, s, B, 1, &T, K, &kp, 0, cv)) return rc;
    RowBuf& b = B.row[0];
    b.ref3d = const_cast<float*>(ref3d); b.imu_aa = const_cast<float*>(imu_aa);   // (only read)
    B.args_h[0] = make_args(s, ptrs_of(b), x, grad, rc_ctx_ign_mask(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(B.args_d, B.args_h, sizeof(SmplifyArgs), hipMemcpyHostToDevice, st));
    rc_launch_smplify_rows(B.args_d, 1, (int)T, body, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(B.terms_h, B.terms_d, (size_t)T * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *loss = total_loss(b.terms_h, T);
    return RC_OK;
}

int rc_smplify_run_batch(rc_ctx* ctx, int32_t n_rows, const int64_t* T_rows, const float* const* pose, const float* const* tran,
                         const float* const* kp, const float* const* imu_ori, const float* K_host, float lr, int32_t max_iter,
                         float loss_threshold, float* const* pose_out, float* const* tran_out, uint8_t* const* update_host,
                         rc_smplify_info* infos, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const auto t_begin = std::chrono::steady_clock::now();
    const BodyConst* body = rc_ctx_body(ctx);
    if (!body) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_smplify_run_batch: body not set");
    SmplifyState* s0 = nullptr;
    if (int rc = state_of(ctx, &s0)) return rc;
    if (!s0->have_prior) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_smplify_run_batch: prior not set (rc_smplify_set_prior)");
    if (n_rows < 0 || max_iter < 1 || !(lr >= 0.0f)) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_run_batch: bad arguments");
    if (n_rows == 0) return RC_OK;
    if (!T_rows || !pose || !tran || !kp || !imu_ori || !K_host || !pose_out || !tran_out || !update_host || !infos)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_run_batch: null buffer");
    for (int r = 0; r < n_rows; ++r)
        if (T_rows[r] <= 0 || T_rows[r] > 0x7fffffff / 99 || !pose[r] || !tran[r] || !kp[r] || !imu_ori[r] || !pose_out[r] || !tran_out[r] || !update_host[r])
            return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_smplify_run_batch: bad row");
    hipStream_t st = (hipStream_t)stream;
    const int P = lbfgs_pairs(max_iter) + 1;

    RowBatch B;
    B.ctx = ctx; B.body = body; B.prior = s0; B.st = st; B.ign = rc_ctx_ign_mask(ctx);
    BatchCarve cv;
    if (int rc = carve_batch(ctx, s0, B, n_rows, T_rows, K_host, kp, P, cv)) return rc;
    const size_t nr = (size_t)n_rows, r0_begin = cv.r0_begin, r1_begin = cv.r1_begin, r_bytes = cv.r_bytes, p_r0 = cv.p_r0, p_r1 = cv.p_r1,
                 o_io = cv.o_io, p_io = cv.p_io;
    // ---- set-up of every row in ONE launch: residual of the initial pose (the pre-check, run.py:24-29, reads its first frame),
    // optimiser parameters, IMU orientations as axis-angle, joints and preserved landmarks (temporal_smplify.py:111-139)
    SmplifyRowIO* io_h = (SmplifyRowIO*)(B.pin + p_io);
    SmplifyRowIO* io_d = (SmplifyRowIO*)(B.dev + o_io);
    for (int r = 0; r < n_rows; ++r) {
        RowBuf& b = B.row[r];
        std::memset(&infos[r], 0, sizeof(infos[r]));
        std::memset(update_host[r], 0, (size_t)b.T);
        SmplifyRowIO& io = io_h[r];
        io.pose = pose[r]; io.tran = tran[r]; io.kp = kp[r]; io.imu_ori = imu_ori[r];
        io.x = b.x; io.imu_aa = b.imu_aa; io.joint = b.joint; io.ref3d = b.ref3d; io.res0 = b.res0; io.res1 = b.res1;
        io.pose_out = pose_out[r]; io.tran_out = tran_out[r];
        for (int e = 0; e < 9; ++e) io.K[e] = b.K[e];
        io.T = (int)b.T; io.live = 0;
    }
    HIP_TRY(ctx, hipMemcpyAsync(io_d, io_h, nr * sizeof(SmplifyRowIO), hipMemcpyHostToDevice, st));
    rc_launch_smplify_begin_rows(io_d, n_rows, B.T_max, body, 100.0f, B.ign, st);
    HIP_TRY(ctx, hipMemcpyAsync(B.pin + p_r0, B.dev + r0_begin, r_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::vector<int> live;
    for (int r = 0; r < n_rows; ++r) {
        RowBuf& b = B.row[r];
        if (frame_mean(b.h_res0) > loss_threshold) {
            if (pose_out[r] != pose[r]) HIP_TRY(ctx, hipMemcpyAsync(pose_out[r], pose[r], (size_t)b.T * 216 * sizeof(float), hipMemcpyDeviceToDevice, st));
            if (tran_out[r] != tran[r]) HIP_TRY(ctx, hipMemcpyAsync(tran_out[r], tran[r], (size_t)b.T * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
            infos[r].status = 0;
            continue;
        }
        live.push_back(r);
        io_h[r].live = 1;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipGetLastError());
    const auto t_opt = std::chrono::steady_clock::now();
    std::vector<Dev::Result> res;
    if (int rc = run_batch_rows(ctx, B, live, lr, max_iter, res)) return rc;
    const auto t_res = std::chrono::steady_clock::now();
    // ---- results in ONE launch: rotations, translation, residual after; then the per-frame update mask (run.py:31-34)
    if (!live.empty()) {
        HIP_TRY(ctx, hipMemcpyAsync(io_d, io_h, nr * sizeof(SmplifyRowIO), hipMemcpyHostToDevice, st));
        rc_launch_smplify_end_rows(io_d, n_rows, B.T_max, body, 100.0f, B.ign, st);
        HIP_TRY(ctx, hipMemcpyAsync(B.pin + p_r1, B.dev + r1_begin, r_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipGetLastError());
    const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (const char* e = std::getenv("RC_SMPLIFY_TRACE"); e && *e == '1') {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "[rc_smplify_run_batch] rows %d live %zu: setup %.2f ms, optimisers %.2f ms (%d rounds, %.2f ms inside the executor, closure kernels %.2f ms), results %.2f ms\n",
                     n_rows, live.size(), ms(t_begin, t_opt), ms(t_opt, t_res), B.rounds, B.round_ms, B.device_ms, host_ms - ms(t_begin, t_res));
    }
    for (int r = 0; r < n_rows; ++r) {
        infos[r].host_ms = host_ms;                                       // of the whole batch
        infos[r].device_ms = B.device_ms;
    }
    for (int r : live) {
        RowBuf& b = B.row[r];
        for (int64_t t = 0; t < b.T; ++t) update_host[r][t] = frame_mean(b.h_res1 + t * 33) < frame_mean(b.h_res0 + t * 33) ? 1 : 0;
        set_info(&infos[r], res[r]);
        infos[r].reserved = B.rounds;
    }
    return RC_OK;
}

int rc_lbfgs_device_probe(rc_ctx* ctx, int32_t backend, int32_t n_rows, const int64_t* T_rows, const float* const* x0, const float* const* a,
                          const float* const* b, float lr, int32_t max_iter, float* const* x_out, rc_smplify_info* infos, float* losses,
                          int64_t cap, int32_t* max_jobs, int32_t* rounds, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    SmplifyState* s = nullptr;
    if (int rc = state_of(ctx, &s)) return rc;
    if ((backend != 0 && backend != 1) || n_rows < 0 || max_iter < 1 || !(lr >= 0.0f) || cap < 0)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_lbfgs_device_probe: bad arguments");
    if (max_jobs) *max_jobs = 0;
    if (rounds) *rounds = 0;
    if (n_rows == 0) return RC_OK;
    if (!T_rows || !x0 || !a || !b || !x_out || !infos || (cap > 0 && !losses))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_lbfgs_device_probe: null buffer");
    for (int r = 0; r < n_rows; ++r)
        if (T_rows[r] <= 0 || T_rows[r] > 0x7fffffff / 99 || !x0[r] || !a[r] || !b[r] || !x_out[r])
            return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_lbfgs_device_probe: bad row");
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> K((size_t)n_rows * 9, 0.0f);                   // K[0] = 0.5 / T: the synthetic closure's IMU weight
    for (int r = 0; r < n_rows; ++r) K[(size_t)9 * r] = 0.5f / (float)T_rows[r];
    std::vector<Dev::Result> res((size_t)n_rows);
    if (backend == 0) {
        const Dev::Options opt = lbfgs_options(lr, max_iter);
        for (int r = 0; r < n_rows; ++r) {
            const int64_t T = T_rows[r];
            if (int rc = reserve(ctx, s, T)) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(s->x.get(), x0[r], (size_t)T * 75 * sizeof(float), hipMemcpyDeviceToDevice, st));
            const RowPtrs ptrs = ptrs_of(s, a[r], b[r], s->imu_aa.get(), K.data() + (size_t)9 * r, T);
            if (int rc = run_single_row(ctx, s, nullptr, ptrs, true, opt, st, res[r])) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(x_out[r], s->x.get(), (size_t)T * 75 * sizeof(float), hipMemcpyDeviceToDevice, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
    } else {
        RowBatch B;
        B.ctx = ctx; B.body = nullptr; B.prior = s; B.st = st; B.ign = rc_ctx_ign_mask(ctx); B.synthetic = true;
        BatchCarve cv;
        if (int rc = carve_batch(ctx, s, B, n_rows, T_rows, K.data(), a, lbfgs_pairs(max_iter) + 1, cv)) return rc;
        std::vector<int> live;
        for (int r = 0; r < n_rows; ++r) {
            RowBuf& row = B.row[r];
            row.ref3d = const_cast<float*>(b[r]);                     // (only read)
            HIP_TRY(ctx, hipMemcpyAsync(row.x, x0[r], row.n * sizeof(float), hipMemcpyDeviceToDevice, st));
            live.push_back(r);
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (int rc = run_batch_rows(ctx, B, live, lr, max_iter, res)) return rc;
        for (int r = 0; r < n_rows; ++r)
            HIP_TRY(ctx, hipMemcpyAsync(x_out[r], B.row[r].x, B.row[r].n * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (max_jobs) *max_jobs = B.max_round_jobs;
        if (rounds) *rounds = B.rounds;
    }
    HIP_TRY(ctx, hipGetLastError());
    for (int r = 0; r < n_rows; ++r) {
        std::memset(&infos[r], 0, sizeof(infos[r]));
        set_info(&infos[r], res[r]);
        for (int64_t i = 0; i < cap; ++i) losses[(size_t)r * cap + i] = i < (int64_t)res[r].losses.size() ? res[r].losses[(size_t)i] : 0.0f;
    }
    return RC_OK;
}

int rc_lbfgs_minimize(rc_objective_fn objective, void* user, int64_t n, double* x, double lr, int32_t max_iter, int32_t max_eval,
                      int32_t history, double tol_grad, double tol_change, int32_t* n_iter, int32_t* n_eval, double* losses,
                      int64_t cap) {
    if (!objective || !x || n <= 0 || max_iter < 1 || max_eval < 1 || history < 1) return RC_ERR_INVALID;
    using L = rc::Lbfgs<double>;
    L::Vec xv(x, x + n);
    L::Objective fn = [&](const L::Vec& p, L::Vec& g) { return objective(user, p.data(), g.data(), n); };
    L::Options o;
    o.lr = lr; o.max_iter = max_iter; o.max_eval = max_eval; o.history_size = history;
    o.tolerance_grad = tol_grad; o.tolerance_change = tol_change;
    const L::Result r = L::minimize(fn, xv, o);
    std::memcpy(x, xv.data(), (size_t)n * sizeof(double));
    if (n_iter) *n_iter = r.n_iter;
    if (n_eval) *n_eval = r.n_eval;
    if (losses) {
        for (int64_t i = 0; i < cap; ++i) losses[i] = i < (int64_t)r.losses.size() ? r.losses[(size_t)i] : 0.0;
    }
    return RC_OK;
}

}  // extern "C"
