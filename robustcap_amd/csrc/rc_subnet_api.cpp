// Host side of the sub-net forward over ragged sequences (include/robustcap_hip.h: rc_subnet_forward, rc_init_net_forward;
// articulate/utils/torch/rnn.py:121-133 and :195-219). Kernels: rc_subnet.hip.
//
// Sequences are sorted by length, longest first (pack_padded_sequence(enforce_sorted=False)), so the sequences still running at time
// t are the prefix of n_t rows. The frames of a time chunk are laid out step after step, the n_t rows of step t from row off[t]:
//   pack x -> relu(linear1) -> x-half of layer 0 over every frame -> per step: layer 0 on the active prefix
//          -> x-half of layer 1 over every frame -> per step: layer 1 -> linear2 over every frame, scattered to the caller's rows.
// A chunk holds as many steps as keep its buffers within RC_SUBNET_SCRATCH_BYTES; more sequences than one step's worth of rows fit
// there are run as independent groups. The recurrent state of a group lives in buffers of its own (two copies of h per layer: step
// t reads copy (t - 1) & 1 and writes copy t & 1, so a sequence that has ended keeps its last h in copy (T_i - 1) & 1).
//
// Training of one sub-net (articulate/utils/torch/train.py:117-122): rc_subnet_forward_tape is the same forward on the same plan, which
// also copies the chunk's sequence buffers to the caller's rows (acts) and records every step's gate activations and c in plan order
// (tape); rc_subnet_backward walks the plan's chunks and steps backwards. Its only sequential part, dh_rec = dG(t + 1) . W_hh, is the
// same kernel on the layer's transposed pack (built on the device from the fp32 packing, on first use) with the cell's backward as
// its epilogue; dG . W_ih of a whole chunk is one tall launch per layer. Weight gradients are reductions over all frames and are left
// to the caller (robustcap_amd/train.py).
//
// Dropout (rnn.py:115,130-131 and torch.nn.LSTM's dropout; the *_train entries with p > 0): rc_dropout.hip's kernel between the launches
// above, keyed by the caller's row so the plan does not move the mask. Forward: in place on relu(linear1) (site 0), and h of layer 0
// -> the buffer relu(linear1) has just left, which layer 1's x half then reads (site 1; the recurrent h stays whole). Backward: in
// place on dG1 . W_ih1 (site 1); d_a leaves unmasked and the caller applies site 0. With p = 0 no such launch is made.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "rc_internal.h"
#include "../../include/robustcap_hip.h"

struct SubnetState {                 // (grow-only buffers; the context's destruction waits for the device before releasing them)
    DevBuf<float> buf;               // per-chunk buffers (X | relu(linear1) = h of layer 1 | x halves | h of layer 0)
    size_t buf_floats = 0;
    DevBuf<float> st;                // recurrent state of a group: per layer two copies of h [npad, H] and c [npad, H]
    size_t st_floats = 0;
    StagedTable<int, 1, 1> plan;     // rank -> sequence, final copy per rank, row maps of every frame of the call (room for what is needed, no more)
    HipEvent done;                   // the end of the last call's work (a call on another stream waits for it: the scratch is shared)
    long long calls = 0, frames = 0, chunks = 0;
    // backward through time
    DevBuf<float> bst;               // state of a group: per layer two copies of dG [npad, 4H] (rc_pk), d_final_h [npad, H], carried dc [npad, H]
    size_t bst_floats = 0;
    struct TPack { DevBuf<float> W; DevBuf<uint16_t> Ws; long long epoch = -1; } tp[6][2];   // transposed operand per net and layer
    // weight gradients (rc_subnet_weight_grads)
    DevBuf<float> wg_part;           // partial sums of a launch cut into parts: [parts][padded M][padded N]
    size_t wg_part_floats = 0;
    DevBuf<double> wg_colsum;        // ... and of a bias sum: [parts][M]
    size_t wg_colsum_doubles = 0;
    int wg_parts = 0;                // rc_set_subnet_wgrad_parts: 0 = from the tile count
    // training batches (rc_subnet_batch, rc_subnet_batch_parts)
    StagedTable<long long, 4> batch_tab;   // [n] first corpus frame | [n + 1] first output frame of every sample (parts: per kind, with ext)
    DevBuf<float> bcam;              // kind world: Rcw | t of every sample [n, 12]
    size_t bcam_floats = 0;
    // the corpus builders (rc_subnet_corpus): sample table and cameras; one pinned copy, its event recorded behind the call's kernel: a call
    // waits for the one before it, and the cameras live under the table's event
    StagedTable<long long, 1> corpus_tab;  // [n] field frame | [n] keypoint frame | [n + 1] output row of every sample
    DevBuf<float> ccam;              // [n, 22] K^-1 | rows 0 .. 2 of T_cw | occlusion flag
    PinBuf<float> ccam_h;
    size_t ccam_n = 0;
    int cus = 0;                     // compute units of the device (asked once)
};

void rc_subnet_free(SubnetState* s) { delete s; }

void rc_subnet_retranspose(SubnetState* S, int ni, const float* const Wl[2], int H, long long epoch, hipStream_t s) {
    if (!S) return;
    for (int l = 0; l < 2; ++l) {
        SubnetState::TPack& t = S->tp[ni][l];
        if (t.W && t.epoch == epoch) rc_launch_subnet_transpose(Wl[l], H, t.W.get(), t.Ws.get(), s);
    }
}

namespace {

inline long long r16(long long x) { return (x + 15) / 16 * 16; }

SubnetState* state(rc_ctx* ctx) {
    SubnetOwner& s = rc_ctx_subnet(ctx);
    if (!s) s.reset(new SubnetState());
    return s.get();
}

SubGemm dense(const SubnetDense& d, const float* A, int M, float* out, int ldo, bool packed, bool relu, const int* out_map) {
    SubGemm g{};
    g.A = A; g.lda = d.Kp; g.a_koff = 0; g.M = M;
    g.W = d.W; g.Ws = d.Ws; g.Kp = d.Kp; g.ncb = d.Np / 16; g.c0 = 0; g.c1 = 4; g.N = d.N;
    g.epi = relu ? RC_SG_RELU : RC_SG_DENSE; g.bias = d.b;
    g.out = out; g.ldo = ldo; g.out_packed = packed ? 1 : 0; g.out_map = out_map;
    return g;
}

// ---- host plan, shared by every entry: ranks by length (longest first), start rows, groups, chunks, row maps ----------------------
struct Chunk {
    int g0, g1, t0, t1;              // ranks [g0, g1) of the group, steps [t0, t1)
    long long frame0;                // first plan row of the chunk
    std::vector<long long> off;      // off[t - t0]: first row of step t within the chunk; off.back(): rows of the chunk
    int next_rows;                   // rows of the group still running at step t1 (0 at the group's end)
};
struct Plan {
    long long total = 0, max_rows = 0;
    int max_group = 0;
    std::vector<Chunk> chunks;
    std::vector<int> ih;             // [n] rank -> sequence | [n] final copy per rank | [total] plan row -> caller's row
};

// rows_max: rows of a chunk (and ranks of a group) at most, a multiple of 16
bool make_plan(int n, const int32_t* lengths, long long rows_max, Plan& P) {
    std::vector<long long> start(n);
    long long total = 0;
    for (int i = 0; i < n; ++i) { start[i] = total; total += lengths[i]; }
    std::vector<int> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return lengths[a] > lengths[b]; });
    P.total = total;
    P.ih.assign(2 * (size_t)n + (size_t)total, 0);
    int* iperm = P.ih.data();
    int* ipar = P.ih.data() + n;
    int* imap = P.ih.data() + 2 * (size_t)n;
    long long frame = 0;
    for (int r = 0; r < n; ++r) { iperm[r] = perm[r]; ipar[r] = (lengths[perm[r]] - 1) & 1; }
    for (int g0 = 0; g0 < n; g0 += (int)rows_max) {
        const int g1 = (int)std::min<long long>(n, g0 + rows_max);
        P.max_group = std::max(P.max_group, g1 - g0);
        const int tmax = lengths[perm[g0]];
        int active = g1 - g0;                                             // n_t of the group
        for (int t = 0; t < tmax;) {
            Chunk c{g0, g1, t, t, frame, {}, 0};
            long long rows = 0;
            while (t < tmax) {
                while (active > 0 && lengths[perm[g0 + active - 1]] <= t) --active;
                if (rows > 0 && rows + active > rows_max) break;
                c.off.push_back(rows);
                for (int r = 0; r < active; ++r) imap[frame + rows + r] = (int)(start[perm[g0 + r]] + t);
                rows += active;
                ++t;
            }
            c.t1 = t;
            c.next_rows = t < tmax ? active : 0;
            c.off.push_back(rows);
            frame += rows;
            P.max_rows = std::max(P.max_rows, rows);
            P.chunks.push_back(std::move(c));
        }
    }
    return frame == total;
}

// rows of a chunk at most: X, relu(linear1) | h of layer 1, x halves (4H), h of layer 0 per row within RC_SUBNET_SCRATCH_BYTES. The backward
// pass needs less per row (dG 4H, dh from above H) and runs on the same plan.
long long plan_rows_max(const SubnetNet& w) {
    const long long row_bytes = 4ll * (w.lin1.Kp + 6ll * w.H);
    return std::max(16ll, RC_SUBNET_SCRATCH_BYTES / row_bytes / 16 * 16);
}

long long tape_floats(const SubnetNet& w, int n, long long total) { return 2ll * n * w.H + 10ll * total * w.H; }

// the bytes from p to the end of its allocation (-1: not a device allocation)
long long device_extent(const void* p) {
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (long long)((const char*)base + size - (const char*)p);
}
// the device allocation behind p holds at least `bytes` from p on
bool dev_holds(const void* p, long long bytes) { return device_extent(p) >= bytes; }

// The sub-net entries run the six-product kernels of rc_subnet.hip; gemm mode 2 (two rounded bf16 terms, three products) has no
// instantiation of them: refused, not run in another arithmetic than the context's.
int refuse_mode2(rc_ctx* ctx, const std::string& what) {
    if (rc_ctx_gemm_mode(ctx) != 2) return RC_OK;
    return rc_ctx_fail(ctx, RC_ERR_INVALID, (what + ": not available in gemm mode 2 (rc_set_gemm_mode 0 or 1 for the sub-net entries)").c_str());
}

// validates what every entry takes; on RC_OK: *ni, *w
int check_args(rc_ctx* ctx, const char* what, const char* net, int32_t n, const int32_t* lengths_host, bool others_null, int* ni, SubnetNet* w) {
    const std::string f(what);
    if (!net || !lengths_host || others_null) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + ": null argument").c_str());
    *ni = rc_ctx_net_index(net);
    if (*ni < 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + ": unknown net " + net).c_str());
    if (n < 1) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + ": no sequences").c_str());
    for (int i = 0; i < n; ++i)
        if (lengths_host[i] < 1) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + ": every sequence needs at least one frame").c_str());
    if (rc_ctx_subnet_net(ctx, *ni, w)) return rc_ctx_fail(ctx, RC_ERR_STATE, (f + ": weights not finalized").c_str());
    return RC_OK;
}

// the call's turn at the shared scratch, the plan's upload
int upload_plan(rc_ctx* ctx, SubnetState* S, const Plan& P, hipStream_t st) {
    const std::vector<int>& ih = P.ih;
    HIP_TRY(ctx, S->plan.grow(ih.size()));                                // (with the scratch: releasing the old table waits for the work that still reads it)
    int* host = nullptr;
    HIP_TRY(ctx, S->plan.stage(ih.size(), &host));                        // the previous call's upload has left the pinned copy
    std::copy(ih.begin(), ih.end(), host);
    HIP_TRY(ctx, S->plan.upload(ih.size(), st));
    HIP_TRY(ctx, S->plan.record(st));
    return RC_OK;
}

bool valid_p(float p) { return p >= 0.0f && p < 1.0f; }

// acts, tape: both null (rc_subnet_forward) or both set (rc_subnet_forward_tape); drop.p > 0: the train-mode forward
int forward_impl(rc_ctx* ctx, const char* what, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                 const float* init_h, const float* init_c, float* final_h, float* final_c, float* acts, float* tape, bool record,
                 const DropoutKey& drop, hipStream_t st) {
    int ni;
    SubnetNet w;
    if (int rc = check_args(ctx, what, net, n, lengths_host, !x || !y || (record && (!acts || !tape)), &ni, &w)) return rc;
    if (!valid_p(drop.p)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string(what) + ": p outside [0, 1)").c_str());
    const bool dropping = drop.p > 0.0f;
    if (int rc = refuse_mode2(ctx, what)) return rc;
    const int split = rc_ctx_gemm_split(ctx);
    SubnetState* S = state(ctx);
    const int H = w.H, Kp1 = w.lin1.Kp;
    Plan P;
    if (!make_plan(n, lengths_host, plan_rows_max(w), P)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string(what) + ": internal plan mismatch").c_str());
    const long long total = P.total;
    if (record && (!dev_holds(tape, 4 * tape_floats(w, n, total)) || !dev_holds(acts, 12ll * total * H)))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string(what) + ": acts or tape smaller than the call needs (rc_subnet_tape_floats)").c_str());

    // ---- scratch (grow-only) and the upload of the plan -----------------------------------------------------------------------------
    // The scratch is shared by every call of the context: a call on another stream than the previous one waits for that call's work.
    if (S->done) HIP_TRY(ctx, hipStreamWaitEvent(st, S->done.get(), 0));
    else HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(S->done), hipEventDisableTiming));
    // (grow-only scratch, contents not kept; releasing the old buffer waits for the work that still reads it)
    const long long R = r16(P.max_rows), G = r16(P.max_group);
    const size_t n_buf = (size_t)(R * (Kp1 + 6ll * H)), n_st = (size_t)(6 * G * H);
    HIP_TRY(ctx, rc_grow(S->buf_floats, n_buf, n_buf, S->buf, n_buf));
    HIP_TRY(ctx, rc_grow(S->st_floats, n_st, n_st, S->st, n_st));
    if (int rc = upload_plan(ctx, S, P, st)) return rc;

    float* X = S->buf.get();                       // [R, Kp1]  packed input
    float* A1 = X + R * Kp1;                 // [R, H]    relu(linear1); then h of layer 1 (A1 is dead once layer 0's x half is formed)
    float* PRE = A1 + R * H;                 // [R, 4H]   x half of the layer being stepped
    float* H0 = PRE + R * 4 * H;             // [R, H]    h of layer 0
    const long long ps = G * H, hl = 3 * G * H;   // state: per layer [copy 0 | copy 1 | c]
    float* hst = S->st.get();
    float* cst = hst + 2 * G * H;
    // tape: init_c by rank [2, n, H] | per layer: gate activations [total, 4H], c [total, H], rows in plan order
    float* tape_l[2] = {nullptr, nullptr};
    if (record) for (int l = 0; l < 2; ++l) tape_l[l] = tape + 2ll * n * H + l * 5ll * total * H;

    // final_* of the group of ranks [g0, g1): every rank's h from the copy its last step wrote
    auto finish = [&](int g0, int g1) {
        rc_launch_subnet_state(hst, hl, ps, S->plan.get() + n + g0, cst, hl, final_h, final_c, S->plan.get() + g0, g1 - g0, n, H, 0, st);
    };
    int g0 = -1, g1 = -1;
    for (const Chunk& c : P.chunks) {
        const long long M = c.off.back();
        const int* map = S->plan.get() + 2 * (size_t)n + c.frame0;
        if (c.g0 != g0) {                    // a new group: its state from init_* (or zeros)
            if (g0 >= 0) finish(g0, g1);
            g0 = c.g0; g1 = c.g1;
            rc_launch_subnet_state(hst, hl, ps, nullptr, cst, hl, const_cast<float*>(init_h), const_cast<float*>(init_c), S->plan.get() + g0,
                                   g1 - g0, n, H, 1, st);
            if (record) rc_launch_subnet_bstate(nullptr, tape + (long long)g0 * H, (long long)n * H, nullptr, init_c, nullptr, S->plan.get() + g0,
                                                g1 - g0, n, H, 1, st);
        }
        rc_launch_subnet_pack(x, w.in, map, X, Kp1, (int)M, st);
        rc_launch_subnet_gemm(dense(w.lin1, X, (int)M, A1, H, true, true, nullptr), split, 1, st);
        if (dropping) rc_launch_dropout_pk(A1, A1, M, H, map, 0, drop, st);
        if (record) rc_launch_subnet_unpack(A1, H, map, acts, H, (int)M, st);
        for (int l = 0; l < 2; ++l) {
            SubGemm half{};
            if (l == 1 && dropping) rc_launch_dropout_pk(H0, A1, M, H, map, 1, drop, st);   // (A1 is dead until layer 1's first step)
            half.A = l == 0 || dropping ? A1 : H0; half.lda = H; half.a_koff = 0; half.M = (int)M;
            half.W = w.Wl[l]; half.Ws = w.Wls[l]; half.Kp = 2 * H; half.ncb = 4 * H / 16; half.c0 = 0; half.c1 = 2; half.N = 4 * H;
            half.epi = RC_SG_HALF; half.out = PRE; half.ldo = 4 * H;
            rc_launch_subnet_gemm(half, split, 1, st);
            for (int t = c.t0; t < c.t1; ++t) {
                const long long o = c.off[t - c.t0];
                SubGemm s{};
                s.A = hst + l * hl + ((t - 1) & 1) * ps; s.lda = H; s.a_koff = H; s.M = (int)(c.off[t - c.t0 + 1] - o);
                s.W = w.Wl[l]; s.Ws = w.Wls[l]; s.Kp = 2 * H; s.ncb = 4 * H / 16; s.c0 = 2; s.c1 = 4; s.N = 4 * H;
                s.epi = RC_SG_LSTM; s.bias = w.bl[l];
                s.pre = PRE + o * 4 * H; s.ldp = 4 * H; s.H = H;
                s.cst = cst + l * hl; s.hout = hst + l * hl + (t & 1) * ps;
                s.hseq = l == 0 ? H0 : A1; s.hseq_row0 = o;
                if (record) {
                    s.tape_g = tape_l[l] + (c.frame0 + o) * 4 * H;
                    s.tape_c = tape_l[l] + 4 * total * H + (c.frame0 + o) * H;
                }
                rc_launch_subnet_gemm(s, split, 0, st);
            }
            if (record) rc_launch_subnet_unpack(l == 0 ? H0 : A1, H, map, acts + (l + 1) * total * H, H, (int)M, st);
        }
        rc_launch_subnet_gemm(dense(w.lin2, A1, (int)M, y, w.out, false, false, map), split, 1, st);
        S->chunks += 1;
    }
    finish(g0, g1);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(S->done.get(), st));
    S->calls += 1;
    S->frames += total;
    return RC_OK;
}

// drop.p > 0: the backward of the train-mode forward with the same (p, seed, call)
int backward_impl(rc_ctx* ctx, const char* what, const char* net, int32_t n, const int32_t* lengths_host, const float* tape,
                  const float* d_h1, const float* d_final_h, const float* d_final_c, float* d_gates, float* d_a, float* d_init_h,
                  float* d_init_c, const DropoutKey& drop, hipStream_t st) {
    int ni;
    SubnetNet w;
    if (int rc = check_args(ctx, what, net, n, lengths_host, !tape || !d_h1 || !d_gates || !d_a, &ni, &w)) return rc;
    if (!valid_p(drop.p)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string(what) + ": p outside [0, 1)").c_str());
    if (int rc = refuse_mode2(ctx, what)) return rc;
    const int split = rc_ctx_gemm_split(ctx);
    SubnetState* S = state(ctx);
    const int H = w.H;
    Plan P;
    if (!make_plan(n, lengths_host, plan_rows_max(w), P)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string(what) + ": internal plan mismatch").c_str());
    const long long total = P.total;
    if (!dev_holds(tape, 4 * tape_floats(w, n, total)) || !dev_holds(d_h1, 4ll * total * H) || !dev_holds(d_gates, 32ll * total * H) ||
        !dev_holds(d_a, 4ll * total * H))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string(what) + ": tape, d_h1, d_gates or d_a smaller than the call needs").c_str());

    if (S->done) HIP_TRY(ctx, hipStreamWaitEvent(st, S->done.get(), 0));
    else HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(S->done), hipEventDisableTiming));
    const long long R = r16(P.max_rows), G = r16(P.max_group);
    const size_t n_buf = (size_t)(R * 5ll * H), n_bst = (size_t)(20 * G * H);
    HIP_TRY(ctx, rc_grow(S->buf_floats, n_buf, n_buf, S->buf, n_buf));
    HIP_TRY(ctx, rc_grow(S->bst_floats, n_bst, n_bst, S->bst, n_bst));
    // the transposed operands: built from the fp32 packing on first use and after a reload (rc_update_subnet_weights rewrites them itself)
    const long long epoch = rc_ctx_weights_epoch(ctx);
    for (int l = 0; l < 2; ++l) {
        SubnetState::TPack& t = S->tp[ni][l];
        if (t.epoch == epoch) continue;
        if (!t.W) HIP_TRY(ctx, rc_alloc_all(t.W, (size_t)8 * H * H, t.Ws, (size_t)24 * H * H));
        rc_launch_subnet_transpose(w.Wl[l], H, t.W.get(), t.Ws.get(), st);
        t.epoch = epoch;
    }
    if (int rc = upload_plan(ctx, S, P, st)) return rc;

    float* DG = S->buf.get();                 // [R, 4H] rc_pk: dG of the layer being stepped, every frame of the chunk
    float* DH = DG + R * 4 * H;               // [R, H]: layer 0's dh from above = dG1 . W_ih1
    const long long ls = 10 * G * H, cps = 4 * G * H;   // state: per layer [dG copy 0 | dG copy 1 | d_final_h | dc]
    float* bst = S->bst.get();
    const float* tape_l[2] = {tape + 2ll * n * H, tape + 2ll * n * H + 5ll * total * H};
    const long long wh_f = 4ll * H * H, wh_s = 12ll * H * H;             // the W_hh columns [H, 2H) of a transposed pack
    auto gemm = [&](int l, const float* A, int M, bool hh) {
        const SubnetState::TPack& t = S->tp[ni][l];
        SubGemm g{};
        g.A = A; g.lda = 4 * H; g.a_koff = 0; g.M = M;
        g.W = t.W.get() + (hh ? wh_f : 0); g.Ws = t.Ws.get() + (hh ? wh_s : 0);
        g.Kp = 4 * H; g.ncb = H / 16; g.c0 = 0; g.c1 = 4; g.N = H; g.H = H;
        return g;
    };
    for (size_t ci = P.chunks.size(); ci-- > 0;) {
        const Chunk& c = P.chunks[ci];
        const long long M = c.off.back();
        const int* perm = S->plan.get() + c.g0;
        const int* map = S->plan.get() + 2 * (size_t)n + c.frame0;
        const int nr = c.g1 - c.g0;
        if (c.next_rows == 0)                // the group's last chunk: its state from d_final_* (or zeros)
            rc_launch_subnet_bstate(bst + 2 * cps, bst + 2 * cps + G * H, ls, d_final_h, d_final_c, nullptr, perm, nr, n, H, 1, st);
        for (int l = 1; l >= 0; --l) {
            float* sl = bst + l * ls;
            for (int t = c.t1 - 1; t >= c.t0; --t) {
                const long long o = c.off[t - c.t0];
                SubGemm s = gemm(l, sl + ((t + 1) & 1) * cps, (int)(c.off[t - c.t0 + 1] - o), true);
                s.epi = RC_SG_BSTEP;
                s.n_next = t + 1 < c.t1 ? (int)(c.off[t - c.t0 + 2] - c.off[t - c.t0 + 1]) : c.next_rows;
                s.dfin_h = sl + 2 * cps;
                s.dh_above = l == 1 ? d_h1 : DH + o * H;
                s.dha_map = l == 1 ? map + o : nullptr;
                s.tape_g = const_cast<float*>(tape_l[l]) + (c.frame0 + o) * 4 * H;
                s.tape_c = const_cast<float*>(tape_l[l]) + 4 * total * H + (c.frame0 + o) * H;
                if (t > c.t0) s.c_prev = tape_l[l] + 4 * total * H + (c.frame0 + c.off[t - c.t0 - 1]) * H;
                else if (t > 0) {
                    const Chunk& p = P.chunks[ci - 1];                    // (the same group: its chunks are consecutive, in time order)
                    s.c_prev = tape_l[l] + 4 * total * H + (p.frame0 + p.off[p.off.size() - 2]) * H;
                } else s.c_prev = tape + ((long long)l * n + c.g0) * H;
                s.cst = sl + 2 * cps + G * H;
                s.hout = sl + (t & 1) * cps;
                s.hseq = DG; s.hseq_row0 = o;
                s.dgates = d_gates + l * total * 4 * H; s.out_map = map + o;
                rc_launch_subnet_gemm_bwd(s, split, 0, st);
            }
            if (c.t0 == 0 && d_init_h) {     // dh_rec of "step -1": dG(0) . W_hh, to the caller's sequences
                SubGemm s = gemm(l, sl, nr, true);
                s.epi = RC_SG_BPLAIN; s.out = d_init_h + (long long)l * n * H; s.ldo = H; s.out_map = perm;
                rc_launch_subnet_gemm_bwd(s, split, 0, st);
            }
            SubGemm tall = gemm(l, DG, (int)M, false);
            tall.epi = RC_SG_BPLAIN; tall.ldo = H;
            if (l == 1) tall.out = DH;
            else { tall.out = d_a; tall.out_map = map; }
            rc_launch_subnet_gemm_bwd(tall, split, 1, st);
            if (l == 1 && drop.p > 0.0f) rc_launch_dropout_rows(DH, DH, M, H, map, 1, drop, st);
        }
        if (c.t0 == 0 && d_init_c)
            rc_launch_subnet_bstate(nullptr, bst + 2 * cps + G * H, ls, nullptr, nullptr, d_init_c, perm, nr, n, H, 0, st);
        S->chunks += 1;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(S->done.get(), st));
    S->calls += 1;
    S->frames += total;
    return RC_OK;
}

// ---- weight gradients: four launches of rc_wgrad.hip's kernel (LSTM layers 0 and 1, linear2, linear1), each followed by the in-order
// sum of its partial sums when its frames were cut into parts, and by the column sums of its A operand (the bias gradients) ---------------------------------------------------------------
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// appends a segment (its own column tiles) unless its output is null
void add_seg(WgradLaunch& L, int kind, const float* src, const float* init, int ld, int ncols, float* out, int ldo) {
    if (!out) return;
    WgradSeg& s = L.seg[L.nseg++];
    s = WgradSeg{};
    s.kind = kind; s.src = src; s.init = init; s.ld = ld; s.ncols = ncols; s.out = out; s.ldo = ldo;
    s.tile0 = L.ntiles_n;
    s.vec = ld % 4 == 0 && aligned16(src) && aligned16(init);
    L.ntiles_n += (ncols + RC_WG_TILE - 1) / RC_WG_TILE;
}

int weight_grads_impl(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, const float* acts,
                      const float* init_h, const float* dy, const float* d_gates, const float* d_p, const DropoutKey& drop,
                      void* const* outs, hipStream_t st) {
    const std::string what = "rc_subnet_weight_grads";
    int ni;
    SubnetNet w;
    if (int rc = check_args(ctx, what.c_str(), net, n, lengths_host, !x || !acts || !dy || !d_gates || !d_p || !outs, &ni, &w)) return rc;
    if (!valid_p(drop.p)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (what + ": p outside [0, 1)").c_str());
    const int H = w.H, in = w.in, out = w.out;
    long long F = 0;
    for (int i = 0; i < n; ++i) F += lengths_host[i];
    if (F >= (1ll << 31)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (what + ": 2^31 frames or more").c_str());
    if (!dev_holds(x, 4 * F * in) || !dev_holds(acts, 12 * F * H) || !dev_holds(dy, 4 * F * out) || !dev_holds(d_gates, 32 * F * H) ||
        !dev_holds(d_p, 4 * F * H) || (init_h && !dev_holds(init_h, 8ll * n * H)))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (what + ": an operand smaller than the call needs").c_str());
    // the twelve outputs: per LSTM layer weight_ih, weight_hh, bias_ih, bias_hh; linear1.weight, .bias; linear2.weight, .bias
    const long long numel[12] = {4ll * H * H, 4ll * H * H, 4ll * H, 4ll * H, 4ll * H * H, 4ll * H * H, 4ll * H, 4ll * H,
                                 (long long)H * in, H, (long long)out * H, out};
    float* o[12];
    for (int i = 0; i < 12; ++i) {
        o[i] = static_cast<float*>(outs[i]);
        if (o[i] && !dev_holds(o[i], 4 * numel[i])) return rc_ctx_fail(ctx, RC_ERR_INVALID, (what + ": an output smaller than its tensor").c_str());
    }
    if (int rc = refuse_mode2(ctx, what)) return rc;
    const int split = rc_ctx_gemm_split(ctx);
    SubnetState* S = state(ctx);
    if (!S->cus) {
        int dev = 0, cus = 0;
        HIP_TRY(ctx, hipGetDevice(&dev));
        HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        S->cus = std::max(1, cus);
    }

    WgradLaunch L[4];
    struct ColSum { const float* A; int lda, M; float *out, *out2; int parts, bpp; } cs[4];      // the bias gradients beside each launch
    auto begin = [&](int q, const float* A, int lda, int M, float* bias, float* bias2) {
        WgradLaunch& l = L[q];
        l = WgradLaunch{};
        l.A = A; l.lda = lda; l.M = M; l.F = F;
        l.a_vec = lda % 4 == 0 && aligned16(A);
        l.ntiles_m = (M + RC_WG_TILE - 1) / RC_WG_TILE;
        l.T = (unsigned)llrint((double)drop.p * 4294967296.0);            // rc_dropout.hip's threshold and scale
        l.scale = (float)(1.0 / (1.0 - (double)drop.p));
        l.key = make_uint2((uint32_t)drop.seed, (uint32_t)(drop.seed >> 32));
        l.call = drop.call;
        cs[q] = ColSum{A, lda, M, bias, bias2, 1, 1};
    };
    for (int l = 0; l < 2; ++l) {        // in_0 = acts[0] as stored; in_1 = acts[1] dropped at site 1 while loaded; h_prev_l from acts[l + 1]
        begin(l, d_gates + l * F * 4 * H, 4 * H, 4 * H, o[4 * l + 2], o[4 * l + 3]);
        add_seg(L[l], l == 1 && drop.p > 0.0f ? RC_WG_MASKED : RC_WG_ROWS, acts + l * F * H, nullptr, H, H, o[4 * l], H);
        add_seg(L[l], RC_WG_SHIFT, acts + (l + 1) * F * H, init_h ? init_h + (long long)l * n * H : nullptr, H, H, o[4 * l + 1], H);
    }
    begin(2, dy, out, out, o[11], nullptr);
    add_seg(L[2], RC_WG_ROWS, acts + 2 * F * H, nullptr, H, H, o[10], H);
    begin(3, d_p, H, H, o[9], nullptr);
    add_seg(L[3], RC_WG_ROWS, x, nullptr, in, in, o[8], in);

    // parts: enough workgroups to fill the device, whole 256-frame blocks each, at most RC_WG_MAX_PARTS
    const long long nblk = (F + RC_WG_BLOCK - 1) / RC_WG_BLOCK;
    // among 1 .. 16 parts (a forced count: that one) the one whose launch takes the fewest rounds of the device times blocks per part --
    // more parts both fill a launch of few tiles and trim the last, part-filled round of a launch of many; ties go to fewer parts
    auto cut = [&](long long workgroups, int* parts, int* bpp) {
        const long long pmax = std::max(1ll, std::min<long long>(S->wg_parts > 0 ? S->wg_parts : RC_WG_MAX_PARTS, nblk));
        long long best = -1;
        for (long long p = S->wg_parts > 0 ? pmax : 1; p <= pmax; ++p) {
            const long long b = (nblk + p - 1) / p, pe = (nblk + b - 1) / b;
            const long long cost = (workgroups * pe + S->cus - 1) / S->cus * b;
            if (best < 0 || cost < best) { best = cost; *parts = (int)pe; *bpp = (int)b; }
        }
    };
    size_t need = 0, need_cs = 0;
    for (int q = 0; q < 4; ++q) {
        WgradLaunch& l = L[q];
        if (l.nseg) {
            const long long tiles = (long long)l.ntiles_m * l.ntiles_n;
            cut(tiles, &l.parts, &l.blocks_per_part);
            if (l.parts > 1) need = std::max(need, (size_t)(l.parts * tiles * RC_WG_TILE * RC_WG_TILE));
        }
        if (cs[q].out || cs[q].out2) {
            cut((cs[q].M + 63) / 64, &cs[q].parts, &cs[q].bpp);
            if (cs[q].parts > 1) need_cs = std::max(need_cs, (size_t)cs[q].parts * cs[q].M);
        }
    }

    if (S->done) HIP_TRY(ctx, hipStreamWaitEvent(st, S->done.get(), 0));
    else HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(S->done), hipEventDisableTiming));
    HIP_TRY(ctx, rc_grow(S->wg_part_floats, need, need, S->wg_part, need));
    HIP_TRY(ctx, rc_grow(S->wg_colsum_doubles, need_cs, need_cs, S->wg_colsum, need_cs));
    Plan P;                              // only its index table: per frame the sequence it opens, or -1
    P.ih.assign((size_t)F, -1);
    long long row = 0;
    for (int i = 0; i < n; ++i) { P.ih[(size_t)row] = i; row += lengths_host[i]; }
    if (int rc = upload_plan(ctx, S, P, st)) return rc;
    for (int q = 0; q < 4; ++q) {
        WgradLaunch& l = L[q];
        if (l.nseg) {
            l.first = S->plan.get();
            l.partial = S->wg_part.get();
            rc_launch_wgrad(l, split, st);
            if (l.parts > 1) rc_launch_wgrad_reduce(l, st);
        }
        if (cs[q].out || cs[q].out2)
            rc_launch_wgrad_colsum(cs[q].A, cs[q].lda, cs[q].M, F, cs[q].parts, cs[q].bpp, S->wg_colsum.get(), cs[q].out, cs[q].out2, st);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(S->done.get(), st));
    return rc_ctx_mark_eager(ctx, st);
}

}  // namespace

extern "C" {

int rc_subnet_weight_grads(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, const float* acts,
                           const float* init_h, const float* dy, const float* d_gates, const float* d_p, float p, uint64_t seed,
                           uint32_t call, void* const* outs_dev, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    return weight_grads_impl(ctx, net, n, lengths_host, x, acts, init_h, dy, d_gates, d_p, DropoutKey{p, seed, call}, outs_dev,
                             (hipStream_t)stream);
}

int rc_set_subnet_wgrad_parts(rc_ctx* ctx, int32_t parts) {
    if (!ctx) return RC_ERR_INVALID;
    if (parts < 0 || parts > RC_WG_MAX_PARTS) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_set_subnet_wgrad_parts: 0 (from the tile count) .. 16");
    state(ctx)->wg_parts = parts;
    return RC_OK;
}

int rc_subnet_forward(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                      const float* init_h, const float* init_c, float* final_h, float* final_c, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    return forward_impl(ctx, "rc_subnet_forward", net, n, lengths_host, x, y, init_h, init_c, final_h, final_c, nullptr, nullptr, false,
                        DropoutKey{0.0f, 0, 0}, (hipStream_t)stream);
}

int rc_subnet_forward_tape(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                           const float* init_h, const float* init_c, float* final_h, float* final_c, float* acts, float* tape,
                           void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    return forward_impl(ctx, "rc_subnet_forward_tape", net, n, lengths_host, x, y, init_h, init_c, final_h, final_c, acts, tape, true,
                        DropoutKey{0.0f, 0, 0}, (hipStream_t)stream);
}

int rc_subnet_forward_train(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                            const float* init_h, const float* init_c, float* final_h, float* final_c, float* acts, float* tape, float p,
                            uint64_t seed, uint32_t call, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    return forward_impl(ctx, "rc_subnet_forward_train", net, n, lengths_host, x, y, init_h, init_c, final_h, final_c, acts, tape, true,
                        DropoutKey{p, seed, call}, (hipStream_t)stream);
}

int rc_subnet_tape_floats(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, int64_t* floats) {
    if (!ctx) return RC_ERR_INVALID;
    int ni;
    SubnetNet w;
    if (int rc = check_args(ctx, "rc_subnet_tape_floats", net, n, lengths_host, !floats, &ni, &w)) return rc;
    long long total = 0;
    for (int i = 0; i < n; ++i) total += lengths_host[i];
    *floats = tape_floats(w, n, total);
    return RC_OK;
}

int rc_subnet_backward(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* tape, const float* d_h1,
                       const float* d_final_h, const float* d_final_c, float* d_gates, float* d_a, float* d_init_h, float* d_init_c,
                       void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    return backward_impl(ctx, "rc_subnet_backward", net, n, lengths_host, tape, d_h1, d_final_h, d_final_c, d_gates, d_a, d_init_h,
                         d_init_c, DropoutKey{0.0f, 0, 0}, (hipStream_t)stream);
}

int rc_subnet_backward_train(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* tape, const float* d_h1,
                             const float* d_final_h, const float* d_final_c, float* d_gates, float* d_a, float* d_init_h,
                             float* d_init_c, float p, uint64_t seed, uint32_t call, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    return backward_impl(ctx, "rc_subnet_backward_train", net, n, lengths_host, tape, d_h1, d_final_h, d_final_c, d_gates, d_a, d_init_h,
                         d_init_c, DropoutKey{p, seed, call}, (hipStream_t)stream);
}

int rc_dropout_apply(rc_ctx* ctx, const float* src, float* dst, int64_t rows, int32_t cols, int32_t site, float p, uint64_t seed,
                     uint32_t call, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    if (!src || !dst) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_dropout_apply: null argument");
    if (rows < 1 || rows >= (1ll << 32) || cols < 4 || cols % 4 != 0 || rows > (1ll << 60) / cols)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_dropout_apply: 1 <= rows < 2^32 and cols a positive multiple of 4");
    if (!valid_p(p) || (site != 0 && site != 1)) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_dropout_apply: p in [0, 1) and site 0 or 1");
    const long long bytes = 4ll * rows * cols;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) || !dev_holds(src, bytes) || !dev_holds(dst, bytes))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_dropout_apply: src and dst are 16-byte aligned device buffers of rows * cols floats");
    hipStream_t st = (hipStream_t)stream;
    if (p > 0.0f) rc_launch_dropout_rows(src, dst, rows, cols, nullptr, site, DropoutKey{p, seed, call}, st);
    else if (src != dst) HIP_TRY(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

// (input width, label width) of a "plain" sample: the sub-net's input and output (net/sig_mp.py:52-81), in kNets order
static const int kBatchWidth[6][2] = {{72, 69}, {141, 3}, {171, 69}, {240, 3}, {141, 144}, {141, 2}};
// augment_fn: noisy columns counted from the end of the row (0: none) and sigma (net/sig_mp.py:360-363, 438-442, 578-581, 701-703, 792-795)
static const struct { int cols; float sigma; } kBatchNoise[6] = {{0, 0.f}, {69, 0.04f}, {0, 0.f}, {69, 0.03f}, {141, 0.03f}, {69, 0.03f}};
// generate_random_rotation_matrix_constrained(y, p, r) of the AMASS samples (net/sig_mp.py:528, :657), degrees
static const BatchCamera kBatchCamera4 = {-180.f, 180.f, -30.f, 30.f, -5.f, 5.f};
static const BatchCamera kBatchCamera6 = {-90.f, 90.f, -30.f, 30.f, -5.f, 5.f};

// One sample of rc_subnet_batch / rc_subnet_batch_parts against the conditions named in `ask`, in the order they stand here: both entries
// refuse with the same words behind their own prefix f, and each asks in its own order.
enum { ASK_SPAN = 1, ASK_AUGMENT = 2, ASK_POOL = 4, ASK_DRAW = 8 };
struct BatchSample { bool world; int augment; const float* conf_pool; int pool_rows; long long off, len; int W, Wl; long long data_bytes, label_bytes; };
static int check_sample(rc_ctx* ctx, const std::string& f, int ask, const BatchSample& s) {
    auto refuse = [&](const std::string& why) { return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + why).c_str()); };
    if ((ask & ASK_SPAN) && (s.len < 1 || s.off < 0)) return refuse("every sample needs an offset >= 0 and at least one frame");
    if ((ask & ASK_SPAN) && (s.off + s.len > (1ll << 40) || (s.off + s.len) * 4 * s.W > s.data_bytes || (s.off + s.len) * 4 * s.Wl > s.label_bytes))
        return refuse("a sample ends past the corpus buffers");
    if ((ask & ASK_AUGMENT) && s.world && !s.augment) return refuse("a world sample has no un-augmented form (the camera is part of it)");
    if ((ask & ASK_POOL) && s.world && (!s.conf_pool || s.pool_rows < 1)) return refuse("kind world needs a confidence pool");
    if ((ask & ASK_DRAW) && s.world && s.len > s.pool_rows)
        return refuse("a sample of " + std::to_string(s.len) + " frames cannot draw distinct rows from a pool of " + std::to_string(s.pool_rows));
    return RC_OK;
}
// ... and the frames of all samples together
static int check_total(rc_ctx* ctx, const std::string& f, long long F) {
    return F >= (1ll << 31) ? rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "2^31 frames or more").c_str()) : RC_OK;
}
// what both entries do in front of filling their table: the pinned copy for nt entries (*th), then the device table and the camera
// scratch of nw world samples grown, each behind a synchronisation of `st` (kernels of earlier calls may still read the old ones)
static int stage_batch_table(rc_ctx* ctx, SubnetState* S, size_t nt, size_t nw, hipStream_t st, long long** th) {
    HIP_TRY(ctx, S->batch_tab.stage(nt, th));
    if (!S->batch_tab.holds(nt)) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, S->batch_tab.grow(nt));
    }
    if (12 * nw > S->bcam_floats) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, rc_grow(S->bcam_floats, 12 * nw, 24 * nw, S->bcam, 24 * nw));
    }
    return RC_OK;
}

int rc_subnet_batch(rc_ctx* ctx, const char* net, int32_t kind, const float* data, const float* label, int32_t n,
                    const int64_t* offsets_host, const int32_t* lengths_host, const float* conf_pool, int32_t pool_rows, int32_t augment,
                    uint64_t seed, uint32_t call, float* x_out, float* label_out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string f = "rc_subnet_batch: ";
    if (!net || !data || !label || !offsets_host || !lengths_host || !x_out || !label_out)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "null argument").c_str());
    const int ni = rc_ctx_net_index(net);
    if (ni < 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "unknown net " + net).c_str());
    if (kind != RC_BATCH_PLAIN && kind != RC_BATCH_WORLD) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "kind 0 (plain) or 1 (world)").c_str());
    const bool world = kind == RC_BATCH_WORLD;
    const bool rnn4 = ni == 2, rnn6 = ni == 3;
    if (world && !rnn4 && !rnn6) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "kind world is rnn4's and rnn6's, not " + net + "'s").c_str());
    const int W = world ? 171 : kBatchWidth[ni][0], Wl = world ? 72 : kBatchWidth[ni][1];
    const int Wo = kBatchWidth[ni][0], Wlo = kBatchWidth[ni][1];
    BatchSample s{world, augment, conf_pool, pool_rows, 0, 0, W, Wl, 0, 0};
    if (int rc = check_sample(ctx, f, ASK_AUGMENT, s)) return rc;
    if (n <= 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "no samples").c_str());
    if (int rc = check_sample(ctx, f, ASK_POOL, s)) return rc;
    // the extents of the caller's allocations, asked once each
    auto extent = device_extent;
    s.data_bytes = extent(data);
    s.label_bytes = extent(label);
    long long F = 0;
    for (int i = 0; i < n; ++i) {
        s.off = offsets_host[i];
        s.len = lengths_host[i];
        if (int rc = check_sample(ctx, f, ASK_SPAN | ASK_DRAW, s)) return rc;
        F += s.len;
    }
    if (int rc = check_total(ctx, f, F)) return rc;
    if (extent(x_out) < 4 * F * Wo || extent(label_out) < 4 * F * Wlo || (world && extent(conf_pool) < 4ll * pool_rows * 33))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "an output or the pool ends before its extent").c_str());
    hipStream_t st = (hipStream_t)stream;
    SubnetState* S = state(ctx);
    // ---- the table: pinned slot -> device, on `stream`
    const size_t nt = 2 * (size_t)n + 1;
    long long* th = nullptr;
    if (int rc = stage_batch_table(ctx, S, nt, world ? (size_t)n : 0, st, &th)) return rc;
    long long at = 0;
    for (int i = 0; i < n; ++i) { th[i] = offsets_host[i]; th[n + i] = at; at += lengths_host[i]; }
    th[2 * (size_t)n] = at;
    HIP_TRY(ctx, S->batch_tab.upload(nt, st));
    HIP_TRY(ctx, S->batch_tab.record(st));
    const BatchKey key{seed, call};
    if (world) {
        rc_launch_batch_world(rnn4 ? 1 : 0, data, label, S->batch_tab.get(), n, F, rnn4 ? kBatchCamera4 : kBatchCamera6, S->bcam.get(), conf_pool,
                              pool_rows, kBatchNoise[ni].sigma, key, x_out, label_out, st);
    } else {
        const int noisy = augment ? kBatchNoise[ni].cols : 0;
        rc_launch_batch_plain(data, label, S->batch_tab.get(), n, F, W, Wl, W - noisy, kBatchNoise[ni].sigma, key, x_out, label_out, st);
    }
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

int rc_subnet_batch_parts(rc_ctx* ctx, const char* net, int32_t n_parts, const int32_t* kinds_host, const float* const* data_parts,
                          const float* const* label_parts, const float* conf_pool, int32_t pool_rows, int32_t n, const int32_t* part_host,
                          const int64_t* offsets_host, const int32_t* lengths_host, int32_t augment, uint64_t seed, uint32_t call,
                          float* x_out, float* label_out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string f = "rc_subnet_batch_parts: ";
    if (!net || !kinds_host || !data_parts || !label_parts || !part_host || !offsets_host || !lengths_host || !x_out || !label_out)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "null argument").c_str());
    const int ni = rc_ctx_net_index(net);
    if (ni < 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "unknown net " + net).c_str());
    if (n_parts <= 0 || n <= 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "no parts or no samples").c_str());
    const bool rnn4 = ni == 2, rnn6 = ni == 3;
    const int Wo = kBatchWidth[ni][0], Wlo = kBatchWidth[ni][1];
    std::vector<long long> data_bytes((size_t)n_parts), label_bytes((size_t)n_parts);
    for (int p = 0; p < n_parts; ++p) {
        if (kinds_host[p] != RC_BATCH_PLAIN && kinds_host[p] != RC_BATCH_WORLD)
            return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "kind 0 (plain) or 1 (world)").c_str());
        if (kinds_host[p] == RC_BATCH_WORLD && !rnn4 && !rnn6)
            return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "kind world is rnn4's and rnn6's, not " + net + "'s").c_str());
        if (!data_parts[p] || !label_parts[p]) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "null part").c_str());
        data_bytes[p] = device_extent(data_parts[p]);
        label_bytes[p] = device_extent(label_parts[p]);
    }
    long long F = 0;
    int nw = 0;
    for (int i = 0; i < n; ++i) {
        const int p = part_host[i];
        if (p < 0 || p >= n_parts) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "a sample of a part that is not there").c_str());
        const bool world = kinds_host[p] == RC_BATCH_WORLD;
        const int W = world ? 171 : Wo, Wl = world ? 72 : Wlo;
        const long long len = lengths_host[i];
        const BatchSample s{world, augment, conf_pool, pool_rows, offsets_host[i], len, W, Wl, data_bytes[p], label_bytes[p]};
        if (int rc = check_sample(ctx, f, ASK_SPAN | ASK_AUGMENT | ASK_POOL | ASK_DRAW, s)) return rc;
        nw += world ? 1 : 0;
        F += len;
    }
    if (int rc = check_total(ctx, f, F)) return rc;
    if (device_extent(x_out) < 4 * F * Wo || device_extent(label_out) < 4 * F * Wlo || (nw && device_extent(conf_pool) < 4ll * pool_rows * 33))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "an output or the pool ends before its extent").c_str());
    hipStream_t st = (hipStream_t)stream;
    SubnetState* S = state(ctx);
    // ---- one table for both launches: per kind [m] corpus frame | [m + 1] the launch's own output frames | ext [4 m] (rc_internal.h)
    const int np = n - nw;
    const size_t nt = 6 * (size_t)n + 2;
    long long* th = nullptr;
    if (int rc = stage_batch_table(ctx, S, nt, (size_t)nw, st, &th)) return rc;
    long long* tab_k[2] = {th, th + (6 * (size_t)np + 1)};
    const int m_k[2] = {np, nw};
    int at_k[2] = {0, 0};
    long long F_k[2] = {0, 0}, at = 0;
    for (int i = 0; i < n; ++i) {
        const int p = part_host[i], k = kinds_host[p] == RC_BATCH_WORLD ? 1 : 0, m = m_k[k], j = at_k[k]++;
        long long* t = tab_k[k];
        long long* ext = t + 2 * (size_t)m + 1;
        t[j] = offsets_host[i];
        t[m + j] = F_k[k];
        ext[j] = i;
        ext[m + j] = at;
        ext[2 * (size_t)m + j] = (long long)(uintptr_t)data_parts[p];
        ext[3 * (size_t)m + j] = (long long)(uintptr_t)label_parts[p];
        F_k[k] += lengths_host[i];
        at += lengths_host[i];
    }
    tab_k[0][2 * (size_t)np] = F_k[0];
    tab_k[1][2 * (size_t)nw] = F_k[1];
    HIP_TRY(ctx, S->batch_tab.upload(nt, st));
    HIP_TRY(ctx, S->batch_tab.record(st));
    const long long* dev_k[2] = {S->batch_tab.get(), S->batch_tab.get() + (6 * (size_t)np + 1)};
    const BatchKey key{seed, call};
    if (np) {
        const int noisy = augment ? kBatchNoise[ni].cols : 0;
        rc_launch_batch_plain(nullptr, nullptr, dev_k[0], np, F_k[0], Wo, Wlo, Wo - noisy, kBatchNoise[ni].sigma, key, x_out, label_out, st,
                              dev_k[0] + 2 * (size_t)np + 1);
    }
    if (nw)
        rc_launch_batch_world(rnn4 ? 1 : 0, nullptr, nullptr, dev_k[1], nw, F_k[1], rnn4 ? kBatchCamera4 : kBatchCamera6, S->bcam.get(),
                              conf_pool, pool_rows, kBatchNoise[ni].sigma, key, x_out, label_out, st, dev_k[1] + 2 * (size_t)nw + 1);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

int rc_subnet_corpus(rc_ctx* ctx, const char* net, int32_t source, int32_t n_seq, const int32_t* seq_frames_host, int64_t frames,
                     const float* pose, const float* imu_acc, const float* imu_ori, const float* joint3d, const float* tran,
                     const float* sync_3d_mp, int32_t n_samples, const int32_t* sample_seq_host, const int32_t* sample_occ_host,
                     const float* cam_K_host, const float* cam_T_host, const float* kp, int64_t kp_frames, float image_w, float image_h,
                     float* x_out, float* label_out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string f = "rc_subnet_corpus: ";
    if (!net || !seq_frames_host || !x_out || !label_out) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "null argument").c_str());
    const int ni = rc_ctx_net_index(net);
    if (ni < 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "unknown net " + net).c_str());
    if (source != RC_CORPUS_AIST && source != RC_CORPUS_AMASS)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "source 0 (AIST) or 1 (AMASS)").c_str());
    const bool amass = source == RC_CORPUS_AMASS, cam_net = ni == 2 || ni == 3;
    if (ni == 5 && !amass) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "the reference has no AIST corpus for rnn8").c_str());
    const int mode = !cam_net ? 0 : (amass ? 2 : 1);
    if (!imu_acc || !imu_ori || !joint3d || (mode == 0 && !pose) || (mode == 1 && ni == 3 && !tran) || (mode == 2 && !sync_3d_mp) ||
        (mode == 1 && (!sample_seq_host || !cam_K_host || !cam_T_host || !kp)))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "a field this corpus reads is null").c_str());
    const BodyConst* body = rc_ctx_body(ctx);
    if (ni == 4 && !body) return rc_ctx_fail(ctx, RC_ERR_STATE, (f + "rnn7's labels need the body (rc_set_body)").c_str());
    if (n_seq <= 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "no sequences").c_str());
    std::vector<long long> first((size_t)n_seq);
    long long total = 0;
    for (int i = 0; i < n_seq; ++i) {
        if (seq_frames_host[i] < 3)
            return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "a sequence of fewer than 3 frames has no row ([1:-1] of it is empty)").c_str());
        first[i] = total;
        total += seq_frames_host[i];
    }
    if (total != frames) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "the sequence table does not sum to the buffers' frames").c_str());
    if (mode != 1) {
        if (sample_seq_host || (n_samples != 0 && n_samples != n_seq))
            return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "only the AIST corpora of rnn4 and rnn6 have view samples").c_str());
        n_samples = n_seq;
    }
    if (n_samples <= 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "no samples").c_str());
    const int n = n_samples;
    long long R = 0, kp_total = 0;
    for (int s = 0; s < n; ++s) {
        const int q = mode == 1 ? sample_seq_host[s] : s;
        if (q < 0 || q >= n_seq) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "a sample of a sequence that is not there").c_str());
        R += seq_frames_host[q] - 2;
        kp_total += seq_frames_host[q];
    }
    if (mode == 1 && kp_total != kp_frames)
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "the sample table does not sum to the keypoint buffer's frames").c_str());
    if (R >= (1ll << 31)) return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "2^31 rows or more").c_str());
    if (mode == 1 && !(std::isfinite(image_w) && std::isfinite(image_h)))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "image size not finite").c_str());
    std::vector<CamConst> cams;
    if (mode == 1) {
        cams.resize((size_t)n);
        float g[3];
        for (int s = 0; s < n; ++s)
            if (!rc_camera_constants(cam_K_host + 9 * (size_t)s, cam_T_host + 16 * (size_t)s, &cams[s], g))
                return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "camera of sample " + std::to_string(s) + " is not finite or K is singular").c_str());
    }
    const int W = mode == 2 ? 171 : kBatchWidth[ni][0], Wl = mode == 2 ? 72 : kBatchWidth[ni][1];
    auto holds = [](const float* p, long long rows, int width) { return !p || device_extent(p) >= 4 * rows * width; };
    if (!holds(pose, total, 72) || !holds(imu_acc, total, 18) || !holds(imu_ori, total, 54) || !holds(joint3d, total, 72) ||
        !holds(tran, total, 3) || !holds(sync_3d_mp, total, 99) || (mode == 1 && !holds(kp, kp_total, 99)) || !holds(x_out, R, W) ||
        !holds(label_out, R, Wl))
        return rc_ctx_fail(ctx, RC_ERR_INVALID, (f + "a field or an output ends before its extent").c_str());
    hipStream_t st = (hipStream_t)stream;
    SubnetState* S = state(ctx);
    const size_t nt = 3 * (size_t)n + 1, nc = 22 * (size_t)n;
    long long* th = nullptr;
    HIP_TRY(ctx, S->corpus_tab.stage(nt, &th));                                            // the call before this one has left the tables:
    if (!S->corpus_tab.holds(nt)) HIP_TRY(ctx, S->corpus_tab.grow(nt));                    // that wait is what the device tables grow behind
    if (mode == 1) HIP_TRY(ctx, rc_grow(S->ccam_n, nc, 2 * nc, S->ccam, 2 * nc, S->ccam_h, 2 * nc));
    long long row = 0, kf = 0;
    for (int s = 0; s < n; ++s) {
        const int q = mode == 1 ? sample_seq_host[s] : s;
        th[s] = first[q];
        th[n + s] = kf;
        th[2 * (size_t)n + s] = row;
        row += seq_frames_host[q] - 2;
        kf += seq_frames_host[q];
    }
    th[3 * (size_t)n] = row;
    HIP_TRY(ctx, S->corpus_tab.upload(nt, st));
    if (mode == 1) {
        float* ch = S->ccam_h.get();
        for (int s = 0; s < n; ++s) {
            float* c = ch + 22 * (size_t)s;
            for (int q = 0; q < 9; ++q) c[q] = cams[s].Kinv[q];
            for (int q = 0; q < 12; ++q) c[9 + q] = cam_T_host[16 * (size_t)s + q];
            c[21] = (sample_occ_host && sample_occ_host[s]) ? 1.0f : 0.0f;
        }
        HIP_TRY(ctx, hipMemcpyAsync(S->ccam.get(), ch, nc * sizeof(float), hipMemcpyHostToDevice, st));
    }
    CorpusArgs a{};
    a.pose = pose; a.acc = imu_acc; a.ori = imu_ori; a.joint = joint3d; a.tran = tran; a.mp = sync_3d_mp; a.kp = kp;
    a.tab = S->corpus_tab.get(); a.cams = S->ccam.get(); a.body = body;
    a.n = n; a.net = ni; a.amass = amass ? 1 : 0; a.W = W; a.Wl = Wl; a.R = R;
    a.sx = image_w; a.sy = image_h; a.x = x_out; a.y = label_out;
    rc_launch_subnet_corpus(mode, a, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, S->corpus_tab.record(st));                                                // behind the kernel: it reads the cameras too
    return RC_OK;
}

int rc_init_net_forward(rc_ctx* ctx, int32_t n, const float* v, float* out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    if (n < 1 || !v || !out) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_init_net_forward: n >= 1 rows and non-null buffers");
    SubnetDense d[3];
    if (rc_ctx_init_net(ctx, d)) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_init_net_forward: weights not finalized");
    if (int rc = refuse_mode2(ctx, "rc_init_net_forward")) return rc;
    const int split = rc_ctx_gemm_split(ctx);
    hipStream_t st = (hipStream_t)stream;
    SubnetState* S = state(ctx);
    const long long per_row = d[0].Kp + d[1].Kp + d[2].Kp;               // packed v | hidden 1 | hidden 2
    const long long rows_max = std::max(16ll, RC_SUBNET_SCRATCH_BYTES / (4 * per_row) / 16 * 16);
    const long long R = r16(std::min<long long>(n, rows_max));
    if (S->done) HIP_TRY(ctx, hipStreamWaitEvent(st, S->done.get(), 0));
    else HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(S->done), hipEventDisableTiming));
    const size_t n_buf = (size_t)(R * per_row);
    HIP_TRY(ctx, rc_grow(S->buf_floats, n_buf, n_buf, S->buf, n_buf));
    float* X = S->buf.get();
    float* h1 = X + R * d[0].Kp;
    float* h2 = h1 + R * d[1].Kp;
    for (long long r0 = 0; r0 < n; r0 += rows_max) {
        const int M = (int)std::min<long long>(n - r0, rows_max);
        rc_launch_subnet_pack(v + r0 * d[0].K, d[0].K, nullptr, X, d[0].Kp, M, st);
        rc_launch_subnet_gemm(dense(d[0], X, M, h1, d[1].Kp, true, true, nullptr), split, 1, st);
        rc_launch_subnet_gemm(dense(d[1], h1, M, h2, d[2].Kp, true, true, nullptr), split, 1, st);
        rc_launch_subnet_gemm(dense(d[2], h2, M, out + r0 * d[2].N, d[2].N, false, false, nullptr), split, 1, st);
        S->chunks += 1;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(S->done.get(), st));
    S->calls += 1;
    S->frames += n;
    return RC_OK;
}

int rc_get_subnet_stats(rc_ctx* ctx, int64_t* calls, int64_t* frames, int64_t* chunks, int64_t* scratch_bytes) {
    if (!ctx) return RC_ERR_INVALID;
    const SubnetState* s = rc_ctx_subnet(ctx).get();
    if (calls) *calls = s ? s->calls : 0;
    if (frames) *frames = s ? s->frames : 0;
    if (chunks) *chunks = s ? s->chunks : 0;
    if (scratch_bytes) *scratch_bytes = s ? (int64_t)(4 * (s->buf_floats + s->st_floats + s->plan.capacity())) : 0;
    return RC_OK;
}

}  // extern "C"
