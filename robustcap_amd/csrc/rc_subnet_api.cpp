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
#include <hip/hip_runtime.h>
#include <algorithm>
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
    DevBuf<int> ibuf;                // rank -> sequence, final copy per rank, row maps of every frame of the call
    size_t ibuf_ints = 0;
    PinBuf<int> ihost;               // pinned staging of ibuf
    size_t ihost_ints = 0;
    HipEvent ev;                     // the last upload from ihost
    HipEvent done;                   // the end of the last call's work (a call on another stream waits for it: the scratch is shared)
    long long calls = 0, frames = 0, chunks = 0;
};

void rc_subnet_free(SubnetState* s) { delete s; }

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

}  // namespace

extern "C" {

int rc_subnet_forward(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                      const float* init_h, const float* init_c, float* final_h, float* final_c, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    if (!net || !lengths_host || !x || !y) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_subnet_forward: null argument");
    const int ni = rc_ctx_net_index(net);
    if (ni < 0) return rc_ctx_fail(ctx, RC_ERR_INVALID, (std::string("rc_subnet_forward: unknown net ") + net).c_str());
    if (n < 1) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_subnet_forward: no sequences");
    for (int i = 0; i < n; ++i)
        if (lengths_host[i] < 1) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_subnet_forward: every sequence needs at least one frame");
    SubnetNet w;
    if (rc_ctx_subnet_net(ctx, ni, &w)) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_subnet_forward: weights not finalized");
    const int split = rc_ctx_gemm_split(ctx);
    hipStream_t st = (hipStream_t)stream;
    SubnetState* S = state(ctx);
    const int H = w.H, Kp1 = w.lin1.Kp;

    // ---- host plan: ranks by length (longest first), start rows, groups, chunks, row maps ----------------------------------------
    std::vector<long long> start(n);
    long long total = 0;
    for (int i = 0; i < n; ++i) { start[i] = total; total += lengths_host[i]; }
    std::vector<int> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return lengths_host[a] > lengths_host[b]; });
    const long long row_bytes = 4ll * (Kp1 + 6ll * H);                   // X, relu(linear1) | h of layer 1, x halves (4H), h of layer 0
    const long long rows_max = std::max(16ll, RC_SUBNET_SCRATCH_BYTES / row_bytes / 16 * 16);
    struct Chunk { int g0, g1, t0, t1; long long frame0; std::vector<long long> off; };   // off[t - t0]: first row of step t
    std::vector<Chunk> chunks;
    std::vector<int> ih(2 * (size_t)n + (size_t)total);
    int* iperm = ih.data();
    int* ipar = ih.data() + n;
    int* imap = ih.data() + 2 * (size_t)n;
    long long frame = 0, max_rows = 0;
    int max_group = 0;
    for (int r = 0; r < n; ++r) { iperm[r] = perm[r]; ipar[r] = (lengths_host[perm[r]] - 1) & 1; }
    for (int g0 = 0; g0 < n; g0 += (int)rows_max) {
        const int g1 = (int)std::min<long long>(n, g0 + rows_max);
        max_group = std::max(max_group, g1 - g0);
        const int tmax = lengths_host[perm[g0]];
        int active = g1 - g0;                                             // n_t of the group
        for (int t = 0; t < tmax;) {
            Chunk c{g0, g1, t, t, frame, {}};
            long long rows = 0;
            while (t < tmax) {
                while (active > 0 && lengths_host[perm[g0 + active - 1]] <= t) --active;
                if (rows > 0 && rows + active > rows_max) break;
                c.off.push_back(rows);
                for (int r = 0; r < active; ++r) imap[frame + rows + r] = (int)(start[perm[g0 + r]] + t);
                rows += active;
                ++t;
            }
            c.t1 = t;
            c.off.push_back(rows);
            frame += rows;
            max_rows = std::max(max_rows, rows);
            chunks.push_back(std::move(c));
        }
    }
    if (frame != total) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_subnet_forward: internal plan mismatch");

    // ---- scratch (grow-only) and the upload of the plan -----------------------------------------------------------------------------
    // The scratch is shared by every call of the context: a call on another stream than the previous one waits for that call's work.
    if (S->done) HIP_TRY(ctx, hipStreamWaitEvent(st, S->done.get(), 0));
    else HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(S->done), hipEventDisableTiming));
    // (grow-only scratch, contents not kept; releasing the old buffer waits for the work that still reads it)
    const long long R = r16(max_rows), G = r16(max_group);
    const size_t n_buf = (size_t)(R * (Kp1 + 6ll * H)), n_st = (size_t)(6 * G * H);
    HIP_TRY(ctx, rc_grow(S->buf_floats, n_buf, n_buf, S->buf, n_buf));
    HIP_TRY(ctx, rc_grow(S->st_floats, n_st, n_st, S->st, n_st));
    HIP_TRY(ctx, rc_grow(S->ibuf_ints, ih.size(), ih.size(), S->ibuf, ih.size()));
    if (S->ev) HIP_TRY(ctx, hipEventSynchronize(S->ev.get()));            // the previous call's upload has left the staging buffer
    else HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(S->ev), hipEventDisableTiming));
    HIP_TRY(ctx, rc_grow(S->ihost_ints, ih.size(), ih.size(), S->ihost, ih.size()));
    std::copy(ih.begin(), ih.end(), S->ihost.get());
    HIP_TRY(ctx, hipMemcpyAsync(S->ibuf.get(), S->ihost.get(), ih.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(S->ev.get(), st));

    float* X = S->buf.get();                       // [R, Kp1]  packed input
    float* A1 = X + R * Kp1;                 // [R, H]    relu(linear1); then h of layer 1 (A1 is dead once layer 0's x half is formed)
    float* PRE = A1 + R * H;                 // [R, 4H]   x half of the layer being stepped
    float* H0 = PRE + R * 4 * H;             // [R, H]    h of layer 0
    const long long ps = G * H, hl = 3 * G * H;   // state: per layer [copy 0 | copy 1 | c]
    float* hst = S->st.get();
    float* cst = hst + 2 * G * H;

    // final_* of the group of ranks [g0, g1): every rank's h from the copy its last step wrote
    auto finish = [&](int g0, int g1) {
        rc_launch_subnet_state(hst, hl, ps, S->ibuf.get() + n + g0, cst, hl, final_h, final_c, S->ibuf.get() + g0, g1 - g0, n, H, 0, st);
    };
    int g0 = -1, g1 = -1;
    for (const Chunk& c : chunks) {
        const long long M = c.off.back();
        const int* map = S->ibuf.get() + 2 * (size_t)n + c.frame0;
        if (c.g0 != g0) {                    // a new group: its state from init_* (or zeros)
            if (g0 >= 0) finish(g0, g1);
            g0 = c.g0; g1 = c.g1;
            rc_launch_subnet_state(hst, hl, ps, nullptr, cst, hl, const_cast<float*>(init_h), const_cast<float*>(init_c), S->ibuf.get() + g0,
                                   g1 - g0, n, H, 1, st);
        }
        rc_launch_subnet_pack(x, w.in, map, X, Kp1, (int)M, st);
        rc_launch_subnet_gemm(dense(w.lin1, X, (int)M, A1, H, true, true, nullptr), split, 1, st);
        for (int l = 0; l < 2; ++l) {
            SubGemm half{};
            half.A = l == 0 ? A1 : H0; half.lda = H; half.a_koff = 0; half.M = (int)M;
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
                rc_launch_subnet_gemm(s, split, 0, st);
            }
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

int rc_init_net_forward(rc_ctx* ctx, int32_t n, const float* v, float* out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    if (n < 1 || !v || !out) return rc_ctx_fail(ctx, RC_ERR_INVALID, "rc_init_net_forward: n >= 1 rows and non-null buffers");
    SubnetDense d[3];
    if (rc_ctx_init_net(ctx, d)) return rc_ctx_fail(ctx, RC_ERR_STATE, "rc_init_net_forward: weights not finalized");
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
    if (scratch_bytes) *scratch_bytes = s ? (int64_t)(4 * (s->buf_floats + s->st_floats + s->ibuf_ints)) : 0;
    return RC_OK;
}

}  // extern "C"
