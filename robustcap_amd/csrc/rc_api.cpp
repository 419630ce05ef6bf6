// C ABI of librobustcap_hip.so (see include/robustcap_hip.h): context, weight repacking, the per-frame launch plan, body / mesh / metrics
// state and the op wrappers. (The GEMM problem builders and the gate-GEMM launcher: rc_gemm_api.cpp.)
//
// Host logic only; all arithmetic runs in the .hip files. The frame-stepped launch plan of one frame (step_impl) mirrors the
// data flow of Net.forward_online (net/sig_mp.py:113-274), with the vision updater of frame t-1 executed at the start of frame t:
//   prep -> {rnn6, rnn4} transition steps of rows whose deferred updater step must precede this frame's own step
//                                          (3 fused launches: linear1, LSTM l0, LSTM l1; usually a handful of rows)
//        -> {rnn4 (+ rows whose deferred step merges into it), rnn2}          (4 fused launches: + linear2)
//        -> [first frame: rnn6 on every row, L155-156]
//        -> fuse -> {rnn6 (+ merged deferred rows), rnn3, rnn7, rnn8, rnn2.init_net}          (4 fused launches)
//        -> tail (fusion logic, FK, landmarks; marks the rows whose updater step is now pending)
// Independent sub-nets share a launch ("problems" of one gate-GEMM grid). 8-14 kernel launches per frame, no host
// synchronisation. rc_sequence runs whole calls on the per-row-cursor wavefront engine instead (rc_sequence_api.cpp): the same
// stages skewed over consecutive ticks and a ring of slots, two or three wide launches per tick on one to three streams. Both
// plans only say which problems go out together: building and launching them is rc_gemm_api.cpp's (its declarations in rc_ctx.h).
#include "../../include/robustcap_hip.h"
#include "rc_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

static thread_local std::string g_create_error;

int fail(rc_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

namespace {

const int kInit[3][2] = {{69, 512}, {512, 1024}, {1024, 2048}};

// MFMA-B fragment order (v_mfma_f32_16x16x4_f32): for 16-column block cb and 16-wide k-chunk q, lane l = kq*16 + j
// holds the float4 W'[cb*16 + j][16q + 4kq + 0..3]; blocks are laid out [cb][q][lane][4] so that a wave's K slice of
// a column block is one contiguous stream of 1 KiB pieces. getW(n, k) returns the (padded) logical weight W'[n][k].
// (both packings run over the 16-column blocks on up to 8 host threads: a context packs 63 M weights twice, ~3.5 s on one thread,
// and bench.py / the tests create a dozen contexts)
template <typename Body>
void for_column_blocks(int n_cb, Body body) {
    const int nt = std::max(1, std::min({8, n_cb / 8, (int)std::thread::hardware_concurrency()}));
    if (nt <= 1) { for (int cb = 0; cb < n_cb; ++cb) body(cb); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([=] { for (int cb = t; cb < n_cb; cb += nt) body(cb); });
    for (std::thread& x : th) x.join();
}

template <typename F>
std::vector<float> pack_weights(int Np, int Kp, F getW) {
    std::vector<float> out((size_t)Np * Kp);
    const int Q = Kp / RC_KC;
    for_column_blocks(Np / 16, [&](int cb) {
        for (int q = 0; q < Q; ++q)
            for (int l = 0; l < 64; ++l) {
                const int kq = l >> 4, j = l & 15;
                float* d = &out[(((size_t)cb * Q + q) * 64 + l) * 4];
                for (int s = 0; s < 4; ++s) d[s] = getW(cb * 16 + j, RC_KC * q + 4 * kq + s);
            }
    });
    return out;
}

// The same matrix as three bf16 planes for the split-bf16 products (rc_gemm.hip: mma_kblock). fp32 w = hi + mid + lo
// exactly (truncation split, 8 + 8 + 8 significant bits). Layout [cb][kb][plane][lane][8]: for 16-column block cb and
// 32-wide k-block kb, lane l = kq*16 + j holds, of column cb*16 + j, the eight k = 32 kb + {4 kq .. 4 kq + 3} and
// 32 kb + 16 + {4 kq .. 4 kq + 3} -- the k a lane of the A operand finds in its two rc_pk float4 of that k-block.
template <typename F>
std::vector<uint16_t> pack_weights_split(int Np, int Kp, F getW) {
    std::vector<uint16_t> out((size_t)Np * Kp * 3);
    const int Qs = Kp / 32;
    for_column_blocks(Np / 16, [&](int cb) {
        for (int kb = 0; kb < Qs; ++kb)
            for (int l = 0; l < 64; ++l) {
                const int kq = l >> 4, j = l & 15;
                for (int e = 0; e < 8; ++e) {
                    const int k = 32 * kb + (e < 4 ? 4 * kq + e : 16 + 4 * kq + (e - 4));
                    const float w = getW(cb * 16 + j, k);
                    uint32_t u;
                    std::memcpy(&u, &w, 4);
                    const uint32_t uh = u & 0xffff0000u;
                    float fh;
                    std::memcpy(&fh, &uh, 4);
                    const float r1 = w - fh;
                    uint32_t u1;
                    std::memcpy(&u1, &r1, 4);
                    const uint32_t um = u1 & 0xffff0000u;
                    float fm;
                    std::memcpy(&fm, &um, 4);
                    const float r2 = r1 - fm;
                    uint32_t u2;
                    std::memcpy(&u2, &r2, 4);
                    const size_t base = (((size_t)cb * Qs + kb) * 3) * 512 + (size_t)l * 8 + e;
                    out[base] = (uint16_t)(uh >> 16);
                    out[base + 512] = (uint16_t)(um >> 16);
                    out[base + 1024] = (uint16_t)(u2 >> 16);
                }
            }
    });
    return out;
}

int upload16(rc_ctx* ctx, void** dst, const std::vector<uint16_t>& v) {
    uint16_t* q = nullptr;
    if (int rc = dev_alloc(ctx, &q, v.size(), false)) return rc;
    HIP_TRY(ctx, hipMemcpy(q, v.data(), v.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    *dst = q;
    return RC_OK;
}

int upload(rc_ctx* ctx, float** dst, const std::vector<float>& v) {
    if (int rc = dev_alloc(ctx, dst, v.size(), false)) return rc;
    HIP_TRY(ctx, hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return RC_OK;
}

int make_dense(rc_ctx* ctx, Dense& d, const std::vector<float>& W, const std::vector<float>& b, int N, int K) {
    // narrow outputs (linear2: N = 2..144) use 16 x 32 tiles, wide ones (linear1, init_net) 32 x 64
    d.mr = N <= 160 ? 1 : 2; d.nc = N <= 160 ? 2 : 4;
    d.N = N; d.K = K; d.Kp = round_up(K, RC_KALIGN); d.Np = round_up(N, 16 * d.nc);
    auto get = [&](int n, int k) -> float { return (n < N && k < K) ? W[(size_t)n * K + k] : 0.0f; };
    std::vector<float> bp(d.Np, 0.0f);
    for (int n = 0; n < N; ++n) bp[n] = b[n];
    if (int rc = upload(ctx, &d.W, pack_weights(d.Np, d.Kp, get))) return rc;
    if (int rc = upload16(ctx, &d.Ws, pack_weights_split(d.Np, d.Kp, get))) return rc;
    if (N <= 160) if (int rc = upload(ctx, &d.Wrm, W)) return rc;
    return upload(ctx, &d.b, bp);
}

const std::vector<float>* staged(rc_ctx* ctx, const std::string& key, size_t numel) {
    auto it = ctx->staged.find(key);
    if (it == ctx->staged.end() || it->second.size() != numel) return nullptr;
    return &it->second;
}

int net_index(const char* name) {
    for (int i = 0; i < 6; ++i) if (!std::strcmp(name, kNets[i].name)) return i;
    return -1;
}

}  // namespace

static int run_stage(rc_ctx* ctx, const std::vector<Stage>& nets, bool with_lin2, const std::vector<GemmProblem>* extra, hipStream_t st, bool fp32 = false) {
    for (int phase = 0; phase < (with_lin2 ? 4 : 3); ++phase) {
        std::vector<GemmProblem> ps;
        for (const Stage& s : nets) {
            if (phase == 0) ps.push_back(lin1_problem(ctx, s));
            else if (phase == 3) ps.push_back(lin2_problem(ctx, s));
            else ps.push_back(lstm_problem(ctx, s, phase - 1));
        }
        if (extra && phase < (int)extra->size()) ps.push_back((*extra)[phase]);
        // linear2 launches are latency chains of a few k-blocks per wave, not MFMA time: on the fp32-input kernel (deeper
        // prefetch, 4 B instead of 6 B per weight) they are 2 us shorter each at batch 256 (r03c), and bitwise fma chains.
        // (linear1 likewise, -1.8 us, but sequence mode runs linear1 inside a split-product launch: kept equal, bit for bit.)
        const bool f = fp32 || phase == 3;
        if (int rc = launch_problems(ctx, ps, nullptr, st, f)) return rc;
    }
    return RC_OK;
}

rc_params_dev dev_params(const rc_params& p) {
    rc_params_dev d{};
    d.conf_lo = p.conf_lo; d.conf_hi = p.conf_hi; d.tran_filter_num = p.tran_filter_num;
    d.contact_threshold = p.contact_threshold; d.distance_threshold = p.distance_threshold;
    d.height_threshold = p.height_threshold;
    d.use_flat_floor = p.use_flat_floor; d.use_vision_updater = p.use_vision_updater;
    d.use_imu_updater = p.use_imu_updater; d.live = p.live; d.update_vision_freq = p.update_vision_freq;
    d.use_reproj_opt = p.use_reproj_opt; d.smooth = p.smooth;
    return d;
}

int step_impl(rc_ctx* ctx, const FrameIO& io, uint32_t flags, hipStream_t st, bool with_tr, bool skip_prep,
              const FrameIO* next_io,     // skip_prep / next_io: the previous / this frame's tail runs the next prep
              int n_live) {                    // rc_sequence_rows: rows that have this frame (-1: all of them)
    const int B = ctx->B;
    const FrameBuffers& fb = ctx->fb;
    const rc_params_dev prm = dev_params(ctx->prm);
    const int first = (flags & RC_FLAG_FIRST_FRAME) ? 1 : 0;
    // Some rows have ended: the prep gives the others RC_ROW2_VALID, which selects the rows of the nets that step on every frame (as in
    // a ring slot of the wavefront engine), and the tiles are picked for the rows that are left. All rows alive: the launches of rc_sequence.
    const bool some_ended = io.len && n_live >= 0 && n_live < B;
    // Tiles for the rows that are left (1: those of the full batch; A/B runs). The opposite of the wavefront engine's choice (collect), both
    // measured on 72 rows x 600 with lengths on [150, 600]: 157.9 ms against 175.4 ms here (profiles/ragged_sequence_bench.txt).
    static const bool rows_as_padded = tune_env("RC_SEQ_STEPPED_ROWS_AS_PADDED", 0) != 0;
    auto every = [&](int net, const float* x, int ldx, Out y) {
        Stage s{net, some_ended ? (int)RC_ROW2_VALID : 0, x, ldx, y, some_ended ? fb.flags2 : nullptr};
        if (some_ended && !rows_as_padded) s.rows_hint = n_live;
        return s;
    };
    auto merged = [&](Stage s) { if (some_ended && !rows_as_padded) s.rows_hint = n_live; return s; };

    if (!skip_prep) rc_launch_prep(fb, io, prm, B, first, st);
    // deferred vision updater of the previous frame (L264-271) for rows that step again now: rnn6 then rnn4 in the
    // reference, independent nets here. State-only, linear2 skipped; usually no row qualifies and the tiles exit.
    if (ctx->prm.use_vision_updater && with_tr) {
        Stage t6{N6, (int)RC_ROW2_TR, fb.x6l, 256, Out{nullptr, 0, 0, false}, fb.flags2};
        Stage t4{N4, (int)RC_ROW2_TR, fb.x4l, 256, Out{nullptr, 0, 0, false}, fb.flags2};
        t6.rows_hint = t4.rows_hint = 8;  // regime changes: a handful of rows per frame -> narrow tiles
        // In the context's product arithmetic: the per-row-cursor engine runs the same two steps inside the slot's own rnn4 /
        // rnn6 launches, and a row's result must not depend on the engine (or on the batch) it runs in.
        if (int rc = run_stage(ctx, {t6, t4}, false, nullptr, st)) return rc;
    }
    // inertial pose branch (L144) + visual pose branch (L153); rnn4 also takes the rows whose deferred updater
    // step is still pending and that do not step on camera keypoints this frame (they read x4l)
    // (longest tiles first: the short ones of the other nets then fill the gaps at the end of the launch)
    if (int rc = run_stage(ctx, {merged(Stage{N4, (int)RC_ROW2_M4, fb.x4, 256, Out{fb.x6, 256, 171, true}, fb.flags2, fb.x4l,
                                              (int)RC_ROW_VIS, (int)RC_ROW_VIS}),
                                 every(N2, fb.x2, 128, Out{fb.x3, 256, 72, true})}, true, nullptr, st)) return rc;
    if (first) {                                                           // L155-156: rnn6 on every row
        if (int rc = run_stage(ctx, {every(N6, fb.x6, 256, Out{fb.pc, 4, 0, false})}, true, nullptr, st)) return rc;
    }
    rc_launch_fuse(fb, io, prm, B, st);
    // velocity, visual translation, pose, contact (L145, L161/165, L169-170) + rnn2.init_net (L181-182)
    std::vector<GemmProblem> init;
    if (ctx->prm.use_imu_updater) {
        init.push_back(dense_problem(ctx, ctx->init[0], seg(fb.xi, 128, 0), Out{ctx->hid1, 512, 0, true}, true, RC_ROW_REACH, fb.flags, nullptr, false));
        init.push_back(dense_problem(ctx, ctx->init[1], seg(ctx->hid1, 512, 0), Out{ctx->hid2, 1024, 0, true}, true, RC_ROW_REACH, fb.flags, nullptr, false));
        init.push_back(dense_problem(ctx, ctx->init[2], seg(ctx->hid2, 1024, 0), Out{fb.init_out, 2048, 0, false}, false, RC_ROW_REACH, fb.flags, nullptr, false));
    }
    if (int rc = run_stage(ctx, {merged(Stage{N6, (int)RC_ROW2_M6, fb.x6, 256, Out{fb.pc, 4, 0, false}, fb.flags2, fb.x6l,
                                              (int)RC_ROW_PC, (int)RC_ROW_PC}),
                                 every(N3, fb.x3, 256, Out{fb.vr, 4, 0, false}),
                                 every(N7, fb.x78, 256, Out{fb.r6d, 144, 0, false}), every(N8, fb.x78, 256, Out{fb.contact, 2, 0, false})},
                           true, &init, st)) return rc;
    // tail: fusion logic + landmarks; rows in the occluded regime get their updater inputs (x6l, x4l) and a
    // pending mark -- the two sub-net steps themselves run at the start of the next frame (or in rc_get_state)
    rc_launch_tail(fb, io, prm, ctx->body, B, first, st, next_io);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

int tune_env(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

namespace {

// run every pending (deferred) updater step now: state then equals the reference's at the end of its frame
int flush_pending(rc_ctx* ctx, hipStream_t st) {
    if (int rc = live_discard_ahead(ctx)) return rc;
    if (!ctx->have_weights || !ctx->prm.use_vision_updater) return RC_OK;
    const FrameBuffers& fb = ctx->fb;
    rc_launch_flush_flags(fb, ctx->B, st);
    return run_stage(ctx, {Stage{N6, (int)RC_ROW2_FLUSH, fb.x6l, 256, Out{nullptr, 0, 0, false}, fb.flags2},
                           Stage{N4, (int)RC_ROW2_FLUSH, fb.x4l, 256, Out{nullptr, 0, 0, false}, fb.flags2}}, false, nullptr, st);
}

// grow-only device scratch of the mesh sweeps (rc_metrics.hip); a reallocation waits for whatever still reads the old one
int sweep_scratch(rc_ctx* ctx, size_t floats, hipStream_t st) {
    if (floats <= ctx->sweep_scratch_cap) return RC_OK;
    (void)st;
    HIP_TRY(ctx, hipDeviceSynchronize());          // the scratch is shared by entry points that take independent stream arguments
    HIP_TRY(ctx, rc_grow(ctx->sweep_scratch_cap, floats, floats, ctx->sweep_scratch, floats));
    return RC_OK;
}

// Skinning is linear in the joint transforms: a regressed keypoint sum_v Jr[k,v] sum_j w[v,j] (G_j x_v + T_j) equals
// sum_j (G_j M[k,j] + T_j m[k,j]) with the pose-independent M[k,j] = sum_v Jr[k,v] w[v,j] x_v, m[k,j] = sum_v Jr[k,v] w[v,j]
// (float64 here, once per mesh / regressor / root) -- evaluate.py:122-125 without touching a vertex per frame.
int fold_regressor(rc_ctx* ctx) {
    const int V = ctx->mesh_V, nk = ctx->mesh_nk;
    std::vector<double> acc((size_t)nk * 24 * 4, 0.0);
    for (int k = 0; k < nk; ++k)
        for (int v = 0; v < V; ++v) {
            const double jw = ctx->mesh_Jr_h[(size_t)k * V + v];
            if (jw == 0.0) continue;
            const double x[3] = {(double)ctx->mesh_vt_h[3 * (size_t)v] - ctx->jroot_h[0], (double)ctx->mesh_vt_h[3 * (size_t)v + 1] - ctx->jroot_h[1],
                                 (double)ctx->mesh_vt_h[3 * (size_t)v + 2] - ctx->jroot_h[2]};
            for (int j = 0; j < 24; ++j) {
                const double ww = jw * ctx->mesh_w_h[(size_t)v * 24 + j];
                double* a = &acc[((size_t)k * 24 + j) * 4];
                a[0] += ww * x[0]; a[1] += ww * x[1]; a[2] += ww * x[2]; a[3] += ww;
            }
        }
    std::vector<float> kM(acc.begin(), acc.end());
    if (!ctx->mesh_kM) if (int rc = dev_alloc(ctx, &ctx->mesh_kM, (size_t)17 * 24 * 4, false)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());                    // nothing in flight may still read the old fold
    HIP_TRY(ctx, hipMemcpy(ctx->mesh_kM, kM.data(), kM.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->fold_dirty = false;
    return RC_OK;
}

// The mesh fit of rc_aligned_metrics needs sum_v p_v t_v^T, sum_v p_v and sum_v |p_v|^2 of two skinned meshes; with p_v = sum_j w[v,j] A_j x~_v
// (A_j = [G_j | T_j], x~_v = (x_v, 1)) they are bilinear in the 24 transforms, through the pose-independent
//   C[j,k] = sum_v w[v,j] w[v,k] x~_v x~_v^T (4x4)   and   m_j = sum_v w[v,j] x~_v
// (float64 here, in vertex order, once per mesh / root). Only pairs j <= k with a non-zero C are kept: C[k,j] = C[j,k], and SMPL's four
// weights per vertex leave most of the 300 pairs empty. Device layout: 24 x 4 doubles m, then the AlignPair list.
int fold_align(rc_ctx* ctx) {
    const int V = ctx->mesh_V;
    std::vector<double> C((size_t)24 * 24 * 16, 0.0), m((size_t)24 * 4, 0.0);
    for (int v = 0; v < V; ++v) {
        const double x[4] = {(double)ctx->mesh_vt_h[3 * (size_t)v] - ctx->jroot_h[0], (double)ctx->mesh_vt_h[3 * (size_t)v + 1] - ctx->jroot_h[1],
                             (double)ctx->mesh_vt_h[3 * (size_t)v + 2] - ctx->jroot_h[2], 1.0};
        int nz[24], n_nz = 0;
        for (int j = 0; j < 24; ++j)
            if (ctx->mesh_w_h[(size_t)v * 24 + j] != 0.0f) nz[n_nz++] = j;
        for (int a = 0; a < n_nz; ++a) {
            const int j = nz[a];
            const double wj = ctx->mesh_w_h[(size_t)v * 24 + j];
            for (int c = 0; c < 4; ++c) m[(size_t)j * 4 + c] += wj * x[c];
            for (int b = a; b < n_nz; ++b) {
                const int k = nz[b];
                const double ww = wj * (double)ctx->mesh_w_h[(size_t)v * 24 + k];
                double* cc = &C[((size_t)j * 24 + k) * 16];
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) cc[4 * r + c] += ww * (x[r] * x[c]);
            }
        }
    }
    std::vector<AlignPair> pairs;
    for (int j = 0; j < 24; ++j)
        for (int k = j; k < 24; ++k) {
            const double* cc = &C[((size_t)j * 24 + k) * 16];
            bool any = false;
            for (int i = 0; i < 16; ++i) any = any || cc[i] != 0.0;
            if (!any) continue;
            AlignPair p{};
            p.j = j;
            p.k = k;
            for (int i = 0; i < 16; ++i) p.c[i] = cc[i];
            pairs.push_back(p);
        }
    const size_t head = m.size() * sizeof(double), bytes = head + pairs.size() * sizeof(AlignPair);
    HIP_TRY(ctx, hipDeviceSynchronize());                    // nothing in flight may still read the old fold
    HIP_TRY(ctx, rc_grow(ctx->align_fold_bytes, bytes, bytes, ctx->align_fold, bytes));
    HIP_TRY(ctx, hipMemcpy(ctx->align_fold.get(), m.data(), head, hipMemcpyHostToDevice));
    if (!pairs.empty()) HIP_TRY(ctx, hipMemcpy(ctx->align_fold.get() + head, pairs.data(), pairs.size() * sizeof(AlignPair), hipMemcpyHostToDevice));
    ctx->align_pairs = (int)pairs.size();
    ctx->align_dirty = false;
    return RC_OK;
}

}  // namespace

int check_ready(rc_ctx* ctx) {
    if (!ctx) return RC_ERR_INVALID;
    if (!ctx->have_weights) return fail(ctx, RC_ERR_STATE, "weights not finalized (rc_finalize_weights)");
    if (!ctx->have_body) return fail(ctx, RC_ERR_STATE, "body constants not set (rc_set_body)");
    return RC_OK;
}


// =============================================================================================== C ABI
const BodyConst* rc_ctx_body(rc_ctx* ctx) { return ctx->have_body ? ctx->body : nullptr; }
int rc_ctx_fail(rc_ctx* ctx, int code, const char* msg) { return fail(ctx, code, msg); }
static SubnetDense subnet_dense(const Dense& d) { return SubnetDense{d.W, d.Ws, d.b, d.K, d.N, d.Kp, d.Np}; }
int rc_ctx_subnet_net(rc_ctx* ctx, int ni, SubnetNet* o) {
    if (!ctx->have_weights) return RC_ERR_STATE;
    const NetDev& n = ctx->net[ni];
    o->lin1 = subnet_dense(n.lin1); o->lin2 = subnet_dense(n.lin2);
    for (int l = 0; l < 2; ++l) { o->Wl[l] = n.Wl[l]; o->Wls[l] = n.Wls[l]; o->bl[l] = n.bl[l]; }
    o->in = n.in; o->H = n.H; o->out = n.out;
    return RC_OK;
}
int rc_ctx_init_net(rc_ctx* ctx, SubnetDense out[3]) {
    if (!ctx->have_weights) return RC_ERR_STATE;
    for (int q = 0; q < 3; ++q) out[q] = subnet_dense(ctx->init[q]);
    return RC_OK;
}
int rc_ctx_net_index(const char* name) { return net_index(name); }
long long rc_ctx_weights_epoch(rc_ctx* ctx) { return ctx->weights_epoch; }
int rc_ctx_mark_eager(rc_ctx* ctx, hipStream_t st) { return mark_eager(ctx, st); }
int rc_ctx_flush_pending(rc_ctx* ctx, hipStream_t st) { return flush_pending(ctx, st); }
SubnetOwner& rc_ctx_subnet(rc_ctx* ctx) { return ctx->subnet; }
SmplifyOwner& rc_ctx_smplify(rc_ctx* ctx) { return ctx->smplify; }
unsigned long long rc_ctx_ign_mask(rc_ctx* ctx) { return ctx->ign_mask; }


extern "C" {

int rc_default_params(int32_t live, rc_params* out) {
    if (!out) return RC_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->conf_lo = live ? 0.85 : 0.7;            // net/sig_mp.py:28, 91-93
    out->conf_hi = live ? 0.9 : 0.8;
    out->contact_threshold = 0.7f;
    out->distance_threshold = 10.0f;
    out->height_threshold = 0.15f;
    out->tran_filter_num = live ? 0.01 : 0.05;
    out->use_flat_floor = 1; out->use_vision_updater = 1; out->use_imu_updater = 1;
    out->live = live ? 1 : 0;
    out->update_vision_freq = 30;
    out->use_reproj_opt = 0;                    // net/sig_mp.py:32
    out->smooth = 1.0f;                         // net/sig_mp.py:30
    return RC_OK;
}

int rc_create(int32_t batch, int32_t live, rc_ctx** out) {
    if (!out || batch < 1 || batch > 65535) return fail(nullptr, RC_ERR_INVALID, "rc_create: bad batch");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, RC_ERR_HIP, "rc_create: no HIP device");
    rc_ctx* ctx = new rc_ctx();
    ctx->B = batch;
    ctx->Bp = round_up(batch, RC_MT);
    (void)hipGetDevice(&ctx->dev);
    rc_default_params(live, &ctx->prm);
    live_create(ctx);
    seq_create(ctx);
    if (int rc = gemm_create(ctx)) { rc_destroy(ctx); return rc; }      // (a tile knob that does not fit: the message is rc_last_error(nullptr)'s)
    const size_t B = (size_t)batch, Bp = (size_t)ctx->Bp;
    int rc = RC_OK;
    FrameBuffers& fb = ctx->fb;
#define A(ptr, n) if (!rc) rc = dev_alloc(ctx, &(ptr), (n))
    for (int i = 0; i < 6 && !rc; ++i) {
        NetDev& n = ctx->net[i];
        n.in = kNets[i].in; n.H = kNets[i].H; n.out = kNets[i].out;
        // tile shape per net (see rc_gemm.hip): 32 rows x 16/32/40 units = 256 tiles per layer at batch 256. The
        // 64-row shapes (4 x 5, 4 x 4) load 20-25 % fewer operand bytes but measured no faster (63.2 vs 64.8 us for an
        // rnn4 layer) and coarsen the row compaction of masked stages (bench 535k vs 573k body-frames/s): not used.
        n.mr = 2;
        n.nc = n.H == 1280 ? 10 : (n.H == 1024 ? 8 : 4);
        A(n.h, 2 * RC_HBUF * Bp * n.H); A(n.c, 2 * B * n.H); A(n.steps, B); A(n.x1, Bp * n.H);
        A(n.part, (size_t)(n.H / 4) * RC_LIVE_MAXB * round_up(n.out, 4));
    }
    A(ctx->hid1, Bp * 512); A(ctx->hid2, Bp * 1024); A(ctx->xtmp, Bp * 256);
    A(fb.x2, Bp * 128); A(fb.x3, Bp * 256); A(fb.x4, Bp * 256); A(fb.x6, Bp * 256); A(fb.x78, Bp * 256);
    A(fb.x4l, Bp * 256); A(fb.x6l, Bp * 256); A(fb.xi, Bp * 128);
    A(fb.vr, B * 4); A(fb.pc, B * 4); A(fb.r6d, B * 144); A(fb.contact, B * 2); A(fb.init_out, B * 2048);
    A(fb.flags, B); A(fb.flags2, B); A(fb.pend, B); A(fb.regime, B); A(fb.kconf, B); A(fb.gravity, B * 3);
    A(fb.last_pfoot, B * 6); A(fb.last_tran, B * 3); A(fb.floor, B * 33); A(fb.j_temp, B * 99);
    A(fb.has_last, B); A(fb.n_floor, B); A(fb.first_reach, B); A(fb.uv_count, B); A(fb.trace, B * 8);
    A(ctx->body, 1);
#undef A
    if (rc) { g_create_error = ctx->err; rc_destroy(ctx); return rc; }
    fb.h2 = ctx->net[N2].h; fb.c2 = ctx->net[N2].c; fb.steps2 = ctx->net[N2].steps;
    fb.h2_par_stride = (long long)Bp * 512; fb.h2_layer_stride = (long long)RC_HBUF * Bp * 512; fb.c2_layer_stride = (long long)B * 512;
    std::vector<float> g(B * 3);
    for (size_t b = 0; b < B; ++b) { g[3 * b] = -0.0029f; g[3 * b + 1] = 0.9980f; g[3 * b + 2] = -0.0273f; }   // sig_mp.py:36
    std::vector<int> ones(B, 1);
    if (hipMemcpy(fb.gravity, g.data(), g.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(fb.first_reach, ones.data(), B * 4, hipMemcpyHostToDevice) != hipSuccess) {
        g_create_error = "rc_create: hipMemcpy failed"; rc_destroy(ctx); return RC_ERR_HIP;
    }
    *out = ctx;
    return RC_OK;
}

int rc_destroy(rc_ctx* ctx) {
    if (!ctx) return RC_OK;
    rc_live_end(ctx);
    (void)hipDeviceSynchronize();        // every buffer, stream and event of the context is released by its owner in ~rc_ctx
    delete ctx;
    return RC_OK;
}

const char* rc_last_error(const rc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rc_get_params(const rc_ctx* ctx, rc_params* out) {
    if (!ctx || !out) return RC_ERR_INVALID;
    *out = ctx->prm;
    return RC_OK;
}
int rc_set_params(rc_ctx* ctx, const rc_params* p) {
    if (!ctx || !p) return RC_ERR_INVALID;
    if (!(p->conf_hi > p->conf_lo) || p->update_vision_freq < 0) return fail(ctx, RC_ERR_INVALID, "rc_set_params: bad range");
    ctx->prm = *p;
    return RC_OK;
}

int rc_load_weight(rc_ctx* ctx, const char* key, const float* host, int64_t numel) {
    if (!ctx || !key || !host || numel <= 0) return RC_ERR_INVALID;
    // validate the key against the reference state_dict layout
    std::string k(key);
    int64_t want = -1;
    for (int i = 0; i < 6 && want < 0; ++i) {
        const NetSpec& s = kNets[i];
        const std::string p = std::string(s.name) + ".";
        if (k.compare(0, p.size(), p)) continue;
        const std::string r = k.substr(p.size());
        const int64_t H = s.H;
        if (r == "linear1.weight") want = H * s.in;
        else if (r == "linear1.bias") want = H;
        else if (r == "linear2.weight") want = (int64_t)s.out * H;
        else if (r == "linear2.bias") want = s.out;
        else if (r == "rnn.weight_ih_l0" || r == "rnn.weight_hh_l0" || r == "rnn.weight_ih_l1" || r == "rnn.weight_hh_l1") want = 4 * H * H;
        else if (r == "rnn.bias_ih_l0" || r == "rnn.bias_hh_l0" || r == "rnn.bias_ih_l1" || r == "rnn.bias_hh_l1") want = 4 * H;
        else if (i == N2) {
            for (int q = 0; q < 3; ++q) {
                if (r == "init_net." + std::to_string(2 * q) + ".weight") want = (int64_t)kInit[q][0] * kInit[q][1];
                if (r == "init_net." + std::to_string(2 * q) + ".bias") want = kInit[q][1];
            }
        }
    }
    if (want < 0) return fail(ctx, RC_ERR_UNKNOWN_KEY, "rc_load_weight: unknown key " + k);
    if (want != numel) return fail(ctx, RC_ERR_INVALID, "rc_load_weight: " + k + " expects " + std::to_string(want) + " values");
    ctx->staged[k].assign(host, host + numel);
    ctx->have_weights = false;
    return RC_OK;
}

static int finalize_weights_impl(rc_ctx* ctx);

int rc_finalize_weights(rc_ctx* ctx) {
    if (!ctx) return RC_ERR_INVALID;
    // A captured live frame has the old weight pointers baked into its kernel arguments: drop it (the next live step
    // re-captures). Then wait for everything in flight and release the previous packed weights -- a reload must not
    // leak a 242 MB copy per call.
    rc_live_end(ctx);
    HIP_TRY(ctx, hipDeviceSynchronize());
    ctx->weight_allocs.clear();
    gemm_planes2_released(ctx);
    ctx->have_weights = false;
    seq_weights_changed(ctx);
    ctx->weights_epoch += 1;
    ctx->alloc_weights = true;
    int rc = finalize_weights_impl(ctx);
    if (rc == RC_OK) rc = gemm_planes2_ensure(ctx);          // a context in gemm mode 2: its planes, from the new packings
    ctx->alloc_weights = false;
    return rc;
}

// One sub-net's tensors, already on the device, into every device array finalize_weights_impl derives from them -- in place, so every pointer
// held by the launch tables, the sequence engine and a captured live frame stays valid. Order of tensors_dev: the sub-net's keys of
// Net.state_dict() (per layer weight_ih, weight_hh, bias_ih, bias_hh; linear1 weight, bias; linear2 weight, bias; rnn2: init_net 0, 2, 4).
int rc_update_subnet_weights(rc_ctx* ctx, const char* net, const void* const* tensors_dev, int32_t count, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    if (!net || !tensors_dev) return fail(ctx, RC_ERR_INVALID, "rc_update_subnet_weights: null argument");
    const int ni = net_index(net);
    if (ni < 0) return fail(ctx, RC_ERR_INVALID, std::string("rc_update_subnet_weights: unknown net ") + net);
    const int want = ni == N2 ? 18 : 12;
    if (count != want) return fail(ctx, RC_ERR_INVALID, "rc_update_subnet_weights: " + std::string(net) + " has " + std::to_string(want) + " tensors");
    for (int i = 0; i < count; ++i)
        if (!tensors_dev[i]) return fail(ctx, RC_ERR_INVALID, "rc_update_subnet_weights: null tensor");
    if (!ctx->have_weights) return fail(ctx, RC_ERR_STATE, "rc_update_subnet_weights: weights not finalized");
    hipStream_t st = (hipStream_t)stream;
    auto T = [&](int i) { return static_cast<const float*>(tensors_dev[i]); };
    // ordered after everything the context has enqueued on any of its streams (and what a live session computed ahead is dropped) ...
    live_forget_last_frame(ctx);
    if (int rc = live_discard_ahead(ctx)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    NetDev& n = ctx->net[ni];
    auto dense = [&](Dense& d, const float* W, const float* b) -> int {
        rc_launch_repack_dense(W, d.N, d.K, d.Np, d.Kp, d.W, d.Ws, st);
        if (d.Wrm) HIP_TRY(ctx, hipMemcpyAsync(d.Wrm, W, (size_t)d.N * d.K * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d.b, b, (size_t)d.N * sizeof(float), hipMemcpyDeviceToDevice, st));   // (the padding stays zero)
        return RC_OK;
    };
    for (int l = 0; l < 2; ++l) rc_launch_repack_lstm(T(4 * l), T(4 * l + 1), T(4 * l + 2), T(4 * l + 3), n.H, n.Wl[l], n.Wls[l], n.bl[l], st);
    if (int rc = dense(n.lin1, T(8), T(9))) return rc;
    if (int rc = dense(n.lin2, T(10), T(11))) return rc;
    if (ni == N2)
        for (int q = 0; q < 3; ++q)
            if (int rc = dense(ctx->init[q], T(12 + 2 * q), T(13 + 2 * q))) return rc;
    rc_subnet_retranspose(ctx->subnet.get(), ni, n.Wl, n.H, ctx->weights_epoch, st);
    gemm_planes2_refresh(ctx, ni, st);
    HIP_TRY(ctx, hipGetLastError());
    // ... and before anything enqueued later, on whatever stream
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return RC_OK;
}

// elements of tensor i of sub-net ni, in rc_update_subnet_weights's order
static long long subnet_tensor_numel(int ni, int i) {
    const NetSpec& s = kNets[ni];
    const long long H = s.H;
    if (i < 8) return (i & 3) < 2 ? 4 * H * H : 4 * H;
    if (i < 12) return i == 8 ? H * s.in : i == 9 ? H : i == 10 ? (long long)s.out * H : s.out;
    const int q = (i - 12) / 2;
    return (i & 1) ? kInit[q][1] : (long long)kInit[q][0] * kInit[q][1];
}

// One clipped Adam step of ONE sub-net and the repack of rc_update_subnet_weights, fused (kernels: rc_optim.hip). Stream-ordered like any
// eager entry: every entry leaves the context's internal streams joined to its caller's stream, so work enqueued on `stream` here follows
// all of it; only an open live session (captured frames on a private stream, perhaps one queued ahead) takes rc_update_subnet_weights's
// synchronising order.
int rc_subnet_optim_step(rc_ctx* ctx, const char* net, const void* const* params_dev, const void* const* grads_dev,
                         const void* const* exp_avg_dev, const void* const* exp_avg_sq_dev, int32_t count, double lr, double beta1,
                         double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2, double max_norm,
                         float* norm_out_dev, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const char* what = "rc_subnet_optim_step: ";
    if (!net || !params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev || !norm_out_dev)
        return fail(ctx, RC_ERR_INVALID, std::string(what) + "null argument");
    const int ni = net_index(net);
    if (ni < 0) return fail(ctx, RC_ERR_INVALID, std::string(what) + "unknown net " + net);
    const int want = ni == N2 ? 18 : 12;
    if (count != want) return fail(ctx, RC_ERR_INVALID, what + std::string(net) + " has " + std::to_string(want) + " tensors");
    for (int i = 0; i < count; ++i)
        if (!params_dev[i] || !exp_avg_dev[i] || !exp_avg_sq_dev[i]) return fail(ctx, RC_ERR_INVALID, std::string(what) + "null parameter or moment tensor");
    if (!(bias_correction1 > 0.0) || !(bias_correction2 > 0.0)) return fail(ctx, RC_ERR_INVALID, std::string(what) + "bias corrections must be positive");
    if (!ctx->have_weights) return fail(ctx, RC_ERR_STATE, std::string(what) + "weights not finalized");
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->optim_partial) {           // once, for the largest sub-net: never regrown, so no later call frees a buffer in use
        long long most = 0;
        for (int j = 0; j < 6; ++j) {
            long long b = 0;
            for (int i = 0; i < (j == N2 ? 18 : 12); ++i) b += (subnet_tensor_numel(j, i) + RC_OPTIM_CHUNK - 1) / RC_OPTIM_CHUNK;
            most = std::max(most, b);
        }
        HIP_TRY(ctx, rc_alloc(ctx->optim_partial, (size_t)most));
    }
    OptimNorm nrm{};
    nrm.count = count;
    int blocks = 0;
    for (int i = 0; i < count; ++i) {
        nrm.g[i] = static_cast<const float*>(grads_dev[i]);
        nrm.n[i] = subnet_tensor_numel(ni, i);
        nrm.block0[i] = blocks;
        if (nrm.g[i]) blocks += (int)((nrm.n[i] + RC_OPTIM_CHUNK - 1) / RC_OPTIM_CHUNK);
    }
    nrm.block0[count] = blocks;
    OptimScalars a{};
    a.step_size = (float)(lr / bias_correction1); a.bc2_sqrt = (float)std::sqrt(bias_correction2);
    a.beta1 = (float)beta1; a.one_m_beta1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.one_m_beta2 = (float)(1.0 - beta2);
    a.eps = (float)eps; a.weight_decay = (float)weight_decay;
    auto T = [&](int i) {
        return OptimTensor{static_cast<float*>(const_cast<void*>(params_dev[i])), static_cast<const float*>(grads_dev[i]),
                           static_cast<float*>(const_cast<void*>(exp_avg_dev[i])), static_cast<float*>(const_cast<void*>(exp_avg_sq_dev[i]))};
    };
    for (int i : {0, 1, 4, 5}) {         // the LSTM matrices move as 16-byte pieces
        const OptimTensor t = T(i);
        if (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15)
            return fail(ctx, RC_ERR_INVALID, std::string(what) + "the LSTM weight tensors must be 16-byte aligned");
    }
    live_forget_last_frame(ctx);
    const bool live = live_session_open(ctx);
    if (live) {
        if (int rc = live_discard_ahead(ctx)) return rc;
        HIP_TRY(ctx, hipDeviceSynchronize());
    }
    rc_launch_optim_norm(nrm, blocks, ctx->optim_partial.get(), (float)max_norm, norm_out_dev, st);
    NetDev& n = ctx->net[ni];
    auto dense = [&](Dense& d, int i) { rc_launch_optim_dense(T(i), T(i + 1), d.N, d.K, d.Np, d.Kp, d.W, d.Ws, d.Wrm, d.b, a, norm_out_dev, st); };
    for (int l = 0; l < 2; ++l)
        rc_launch_optim_lstm(T(4 * l), T(4 * l + 1), T(4 * l + 2), T(4 * l + 3), n.H, n.Wl[l], n.Wls[l], n.bl[l], a, norm_out_dev, st);
    dense(n.lin1, 8);
    dense(n.lin2, 10);
    if (ni == N2)
        for (int q = 0; q < 3; ++q) dense(ctx->init[q], 12 + 2 * q);
    rc_subnet_retranspose(ctx->subnet.get(), ni, n.Wl, n.H, ctx->weights_epoch, st);
    gemm_planes2_refresh(ctx, ni, st);
    HIP_TRY(ctx, hipGetLastError());
    if (live) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return RC_OK;
    }
    return mark_eager(ctx, st);
}

// The loss of the training iteration (kernels: rc_loss.hip). Touches nothing of the context but its partial sums, so it is ordered by the
// caller's stream alone.
int rc_subnet_loss(rc_ctx* ctx, int32_t kind, const float* x, const float* y, int64_t frames, int32_t width, const float* aux_dev,
                   float* value_dev, float* dx_dev, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string what = "rc_subnet_loss: ";
    bool fits = false;
    switch (kind) {
        case RC_LOSS_MSE: fits = width == 69 || width == 3; break;
        case RC_LOSS_BCE_LOGITS: fits = width == 2; break;
        case RC_LOSS_WINDOW_MSE: fits = width == 3; break;
        case RC_LOSS_POSE_FK: fits = width == 144; break;
        default: return fail(ctx, RC_ERR_INVALID, what + "unknown kind " + std::to_string(kind));
    }
    if (!fits) return fail(ctx, RC_ERR_INVALID, what + "width " + std::to_string(width) + " does not fit kind " + std::to_string(kind));
    if (frames <= 0) return fail(ctx, RC_ERR_INVALID, what + "frames must be positive");
    if (kind == RC_LOSS_WINDOW_MSE && frames < 60)
        return fail(ctx, RC_ERR_INVALID, what + "window_mse needs at least 60 frames (" + std::to_string(frames) +
                                             " given: no window of 60 frames exists and the reference's value is the NaN of an empty mean)");
    if (kind == RC_LOSS_POSE_FK && !ctx->have_body) return fail(ctx, RC_ERR_INVALID, what + "pose_fk: body not set");
    if (kind == RC_LOSS_BCE_LOGITS && !aux_dev) return fail(ctx, RC_ERR_INVALID, what + "bce_logits: pos_weight missing");
    if (!x || !y || !value_dev) return fail(ctx, RC_ERR_INVALID, what + "null argument");
    if (kind != RC_LOSS_WINDOW_MSE && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)dx_dev) & 15))
        return fail(ctx, RC_ERR_INVALID, what + "x, y and dx must be 16-byte aligned");
    if (!ctx->loss_partial) HIP_TRY(ctx, rc_alloc(ctx->loss_partial, (size_t)RC_LOSS_MAX_PARTIALS));     // once: never regrown
    rc_launch_subnet_loss(kind, ctx->body, x, y, frames, width, aux_dev, ctx->loss_partial.get(), value_dev, dx_dev, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

// The validation pass's metric (train.py:94-101,124-131: `eval_fn(net(d), l)` per validation batch), for ALL batches of a concatenated
// output at once (kernels: rc_loss.hip). Like rc_subnet_loss it touches nothing of the context but its own partial sums and group table.
int rc_subnet_eval(rc_ctx* ctx, int32_t kind, const float* x, const float* y, int32_t groups, const int64_t* group_frames_host,
                   int32_t width, const float* aux_dev, float* values_dev, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string what = "rc_subnet_eval: ";
    bool fits = false;
    switch (kind) {
        case RC_LOSS_MSE: fits = width == 69 || width == 3; break;
        case RC_LOSS_BCE_LOGITS: fits = width == 2; break;
        case RC_LOSS_WINDOW_MSE: fits = width == 3; break;
        case RC_LOSS_POSE_FK: fits = width == 144; break;
        case RC_EVAL_POSITION_ERROR: fits = width >= 3 && width % 3 == 0; break;
        default: return fail(ctx, RC_ERR_INVALID, what + "unknown kind " + std::to_string(kind));
    }
    if (!fits) return fail(ctx, RC_ERR_INVALID, what + "width " + std::to_string(width) + " does not fit kind " + std::to_string(kind));
    if (groups < 1 || groups > RC_EVAL_MAX_GROUPS)
        return fail(ctx, RC_ERR_INVALID, what + std::to_string(groups) + " groups: 1 .. " + std::to_string(RC_EVAL_MAX_GROUPS) + " expected");
    if (!x || !y || !values_dev || !group_frames_host) return fail(ctx, RC_ERR_INVALID, what + "null argument");
    const int64_t least = kind == RC_LOSS_WINDOW_MSE ? 60 : 1;
    long long F = 0;
    for (int g = 0; g < groups; ++g) {
        const int64_t f = group_frames_host[g];
        if (f < least || f > (1ll << 40))
            return fail(ctx, RC_ERR_INVALID, what + "group " + std::to_string(g) + " has " + std::to_string(f) + " frames: at least " +
                                                 std::to_string(least) + " expected" +
                                                 (kind == RC_LOSS_WINDOW_MSE ? " (window_mse: below, no window of 60 frames exists)" : ""));
        F += f;
        if (F > (1ll << 40)) return fail(ctx, RC_ERR_INVALID, what + "group " + std::to_string(g) + " ends past 2^40 frames");
    }
    if (kind == RC_LOSS_POSE_FK && !ctx->have_body) return fail(ctx, RC_ERR_INVALID, what + "pose_fk: body not set");
    if (kind == RC_LOSS_BCE_LOGITS && !aux_dev) return fail(ctx, RC_ERR_INVALID, what + "bce_logits: pos_weight missing");
    const bool pieces = kind == RC_LOSS_MSE || kind == RC_LOSS_BCE_LOGITS || kind == RC_LOSS_POSE_FK;
    if (pieces && (((uintptr_t)x | (uintptr_t)y) & 15)) return fail(ctx, RC_ERR_INVALID, what + "x and y must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    // ---- the group table: pinned slot -> device, on `stream`
    const size_t G = (size_t)groups;
    EvalGroup* th = nullptr;
    HIP_TRY(ctx, ctx->eval_tab.stage(G, &th));
    long long at = 0, blocks = 0;
    for (int g = 0; g < groups; ++g) {
        th[g].frame0 = at;
        th[g].frames = group_frames_host[g];
        th[g].blk0 = (int)blocks;
        rc_eval_group(kind, width, &th[g]);
        at += th[g].frames;
        blocks += th[g].nblk;
    }
    if (!ctx->eval_tab.holds(G) || (size_t)blocks > ctx->eval_partial_n) {                   // (kernels of earlier calls may still use the old buffers)
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, ctx->eval_tab.grow(G));
        HIP_TRY(ctx, rc_grow(ctx->eval_partial_n, (size_t)blocks, 2 * (size_t)blocks, ctx->eval_partial, 2 * (size_t)blocks));
    }
    HIP_TRY(ctx, ctx->eval_tab.upload(G, st));
    HIP_TRY(ctx, ctx->eval_tab.record(st));
    rc_launch_subnet_eval(kind, ctx->body, ctx->eval_tab.get(), groups, blocks, x, y, width, aux_dev, ctx->eval_partial.get(), values_dev, st);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

static int finalize_weights_impl(rc_ctx* ctx) {
    for (int i = 0; i < 6; ++i) {
        const NetSpec& s = kNets[i];
        NetDev& n = ctx->net[i];
        const std::string p = std::string(s.name) + ".";
        const size_t H = s.H;
        auto need = [&](const std::string& r, size_t numel) { return staged(ctx, p + r, numel); };
        const auto *w1 = need("linear1.weight", H * s.in), *b1 = need("linear1.bias", H);
        const auto *w2 = need("linear2.weight", (size_t)s.out * H), *b2 = need("linear2.bias", s.out);
        if (!w1 || !b1 || !w2 || !b2) return fail(ctx, RC_ERR_STATE, "rc_finalize_weights: missing linear weights of " + p);
        if (int rc = make_dense(ctx, n.lin1, *w1, *b1, s.H, s.in)) return rc;
        if (int rc = make_dense(ctx, n.lin2, *w2, *b2, s.out, s.H)) return rc;
        for (int l = 0; l < 2; ++l) {
            const std::string sl = std::to_string(l);
            const auto *wi = need("rnn.weight_ih_l" + sl, 4 * H * H), *wh = need("rnn.weight_hh_l" + sl, 4 * H * H);
            const auto *bi = need("rnn.bias_ih_l" + sl, 4 * H), *bh = need("rnn.bias_hh_l" + sl, 4 * H);
            if (!wi || !wh || !bi || !bh) return fail(ctx, RC_ERR_STATE, "rc_finalize_weights: missing LSTM weights of " + p);
            // 16-column block cb = hidden units 4 cb .. 4 cb + 3, each with its gates (i, f, g, o) in four consecutive
            // columns: column n' <-> torch row g*H + 4*cb + u (torch gate order i,f,g,o). Independent of the tile width,
            // so few-row stages can run narrow tiles on the same weights; the epilogue reads a unit's gates as one float4.
            auto orig = [&](int np) { const int cb = np / 16, u = (np % 16) / 4, g = np % 4; return (size_t)g * H + 4 * cb + u; };
            auto get = [&](int np, int k) -> float {
                const size_t r = orig(np);
                return k < (int)H ? (*wi)[r * H + k] : (*wh)[r * H + (k - H)];
            };
            std::vector<float> bp(4 * H);
            for (size_t np = 0; np < 4 * H; ++np) bp[np] = (*bi)[orig((int)np)] + (*bh)[orig((int)np)];
            if (int rc = upload(ctx, &n.Wl[l], pack_weights(4 * s.H, 2 * s.H, get))) return rc;
            if (int rc = upload16(ctx, &n.Wls[l], pack_weights_split(4 * s.H, 2 * s.H, get))) return rc;
            if (int rc = upload(ctx, &n.bl[l], bp)) return rc;
        }
    }
    for (int q = 0; q < 3; ++q) {
        const std::string p = "rnn2.init_net." + std::to_string(2 * q) + ".";
        const auto *w = staged(ctx, p + "weight", (size_t)kInit[q][0] * kInit[q][1]), *b = staged(ctx, p + "bias", kInit[q][1]);
        if (!w || !b) return fail(ctx, RC_ERR_STATE, "rc_finalize_weights: missing " + p);
        if (int rc = make_dense(ctx, ctx->init[q], *w, *b, kInit[q][1], kInit[q][0])) return rc;
    }
    ctx->have_weights = true;
    // the sequence engine's ring, streams and tables (booked as context allocations, not as packed weights: a reload frees the latter)
    const bool aw = ctx->alloc_weights;
    ctx->alloc_weights = false;
    const int rc_pre = seq_prepare(ctx);
    ctx->alloc_weights = aw;
    if (rc_pre) return rc_pre;
    HIP_TRY(ctx, hipDeviceSynchronize());
    // the ~254 MB host copy is not kept: a later partial reload has to pass every tensor again (the Python host keeps
    // references to the caller's own arrays for that, robustcap_amd/net/sig_mp.py: load_state_dict)
    std::map<std::string, std::vector<float>>().swap(ctx->staged);
    return RC_OK;
}

int rc_set_body(rc_ctx* ctx, const int32_t* parent, const float* J, const float* w33, const float* v33) {
    if (!ctx || !parent || !J || !w33 || !v33) return RC_ERR_INVALID;
    BodyConst b{};
    for (int i = 0; i < 24; ++i) {
        b.parent[i] = i == 0 ? 0 : parent[i];
        if (i > 0 && (parent[i] < 0 || parent[i] >= i)) return fail(ctx, RC_ERR_INVALID, "rc_set_body: parent[i] must be in [0, i)");
        b.level[i] = i == 0 ? 0 : b.level[parent[i]] + 1;
        if (b.level[i] > 9) return fail(ctx, RC_ERR_INVALID, "rc_set_body: kinematic tree deeper than 9");
        if (i > 0) {
            int& n = b.nchild[parent[i]];
            if (n >= 4) return fail(ctx, RC_ERR_INVALID, "rc_set_body: a joint with more than 4 children");
            b.child[parent[i]][n++] = i;
        }
    }
    for (int i = 0; i < 24; ++i)
        for (int c = 0; c < 3; ++c) {
            b.jroot[c] = J[c];
            b.jrest[i][c] = J[3 * i + c] - J[c];                                   // model.py:87
            b.bone[i][c] = i == 0 ? b.jrest[0][c] : (J[3 * i + c] - J[c]) - (J[3 * parent[i] + c] - J[c]);   // spatial.py:148-167
        }
    for (int v = 0; v < 33; ++v) {
        b.override_joint[v] = -1;
        for (int c = 0; c < 3; ++c) b.v33[v][c] = v33[3 * v + c] - J[c];
        for (int j = 0; j < 24; ++j) b.w33[v][j] = w33[24 * v + j];
    }
    const int ov[12][2] = {{11, 16}, {12, 17}, {13, 18}, {14, 19}, {15, 20}, {16, 21},      // sig_mp.py:295-298
                           {23, 1},  {24, 2},  {25, 4},  {26, 5},  {27, 7},  {28, 8}};
    for (auto& o : ov) b.override_joint[o[0]] = o[1];
    HIP_TRY(ctx, hipMemcpy(ctx->body, &b, sizeof(b), hipMemcpyHostToDevice));
    ctx->have_body = true;
    for (int c = 0; c < 3; ++c) ctx->jroot_h[c] = b.jroot[c];
    ctx->fold_dirty = true;
    ctx->align_dirty = true;
    return RC_OK;
}

int rc_set_gravity(rc_ctx* ctx, const float* g) {
    if (!ctx || !g) return RC_ERR_INVALID;
    HIP_TRY(ctx, hipMemcpy(ctx->fb.gravity, g, (size_t)ctx->B * 3 * sizeof(float), hipMemcpyHostToDevice));
    return RC_OK;
}

int rc_reset(rc_ctx* ctx, const uint8_t* row_mask, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    live_forget_last_frame(ctx, true);
    float* h[6]; float* c[6]; int H[6];
    for (int i = 0; i < 6; ++i) { h[i] = ctx->net[i].h; c[i] = ctx->net[i].c; H[i] = ctx->net[i].H; }
    rc_launch_reset(ctx->fb, h, c, H, row_mask, ctx->B, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return mark_eager(ctx, (hipStream_t)stream);
}

int rc_step(rc_ctx* ctx, const float* j2dc, const float* accc, const float* oric, const float* first_tran, uint32_t flags,
            float* pose_out, float* tran_out, void* stream) {
    if (int rc = check_ready(ctx)) return rc;
    live_forget_last_frame(ctx);                       // the live path's host-side flag mirror no longer knows the last frame
    if (!j2dc || !accc || !oric || !pose_out || !tran_out) return fail(ctx, RC_ERR_INVALID, "rc_step: null buffer");
    FrameIO io{j2dc, accc, oric, first_tran, pose_out, tran_out, 99, 18, 54, 216, 3};
    if (int rc = step_impl(ctx, io, flags, (hipStream_t)stream)) return rc;
    return mark_eager(ctx, (hipStream_t)stream);
}

int rc_r6d_to_rotmat(const float* r6d, float* R, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!r6d || !R || n < 0) return RC_ERR_INVALID;
    rc_launch_r6d(r6d, R, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_axis_angle_to_rotmat(const float* aa, float* R, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!aa || !R || n < 0) return RC_ERR_INVALID;
    rc_launch_aa2R(aa, R, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_rotmat_to_axis_angle(const float* R, float* aa, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!aa || !R || n < 0) return RC_ERR_INVALID;
    rc_launch_R2aa(R, aa, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_rotmat_to_r6d(const float* R, float* r6d, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!R || !r6d || n < 0) return RC_ERR_INVALID;
    rc_launch_rotmat_to_r6d(R, r6d, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_angle_between(const float* R1, const float* R2, float* out, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!R1 || !R2 || !out || n < 0) return RC_ERR_INVALID;
    rc_launch_angle_between(R1, R2, out, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_lerp(const float* a, const float* b, double t, float* out, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!a || !b || !out || n < 0) return RC_ERR_INVALID;
    rc_launch_lerp(a, b, (float)(1.0 - t), (float)t, out, n, (hipStream_t)stream);     // general.py:24: a * (1 - t) + b * t
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_normalize_rows(const float* x, float* out, float* norm, int64_t rows, int32_t width, void* stream) {
    if (rows == 0) return RC_OK;
    if (!x || !out || rows < 0 || width < 1) return RC_ERR_INVALID;
    rc_launch_normalize_rows(x, out, norm, rows, width, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_bbox_normalise(const float* kp, float* out, int64_t n, void* stream) {
    if (n == 0) return RC_OK;
    if (!kp || !out || n < 0) return RC_ERR_INVALID;
    rc_launch_bbox_normalise(kp, out, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_conf_mean(const float* j2dc, int64_t n, double lo, double hi, float* mean, int8_t* code, void* stream) {
    if (n == 0) return RC_OK;
    if (!j2dc || (!mean && !code) || n < 0 || n > INT32_MAX) return RC_ERR_INVALID;
    rc_launch_scan_conf(j2dc, 99, (int)n, 1, lo, hi, (signed char*)code, (hipStream_t)stream, mean);    // the planner's kernel
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_fk_r(rc_ctx* ctx, const float* Rl, float* Rg, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_fk_r: body not set") : RC_ERR_INVALID;
    if (n < 0 || (n > 0 && (!Rl || !Rg))) return fail(ctx, RC_ERR_INVALID, "rc_fk_r: bad argument");
    rc_launch_fk_r(ctx->body, Rl, Rg, n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_bone_to_joint(rc_ctx* ctx, const float* bone, float* joint, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_bone_to_joint: body not set") : RC_ERR_INVALID;
    if (n < 0 || (n > 0 && (!bone || !joint))) return fail(ctx, RC_ERR_INVALID, "rc_bone_to_joint: bad argument");
    rc_launch_bone_to_joint(ctx->body, bone, joint, n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_joint_to_bone(rc_ctx* ctx, const float* joint, float* bone, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_joint_to_bone: body not set") : RC_ERR_INVALID;
    if (n < 0 || (n > 0 && (!bone || !joint))) return fail(ctx, RC_ERR_INVALID, "rc_joint_to_bone: bad argument");
    rc_launch_joint_to_bone(ctx->body, joint, bone, n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_zero_pose(rc_ctx* ctx, float* joint, float* vert, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_zero_pose: body not set") : RC_ERR_INVALID;
    if (!joint) return fail(ctx, RC_ERR_INVALID, "rc_zero_pose: null buffer");
    if (vert && ctx->mesh_V == 0) return fail(ctx, RC_ERR_STATE, "rc_zero_pose: vertices need rc_set_mesh");
    rc_launch_zero_pose(ctx->body, ctx->mesh_vt, ctx->mesh_V, joint, vert, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_shape_body(rc_ctx* ctx, const float* v_template, const float* shapedirs, const float* J_regressor, const float* beta,
                  int32_t V, float* verts_out, float* joints_out) {
    if (!ctx) return RC_ERR_INVALID;
    if (!v_template || !shapedirs || !J_regressor || !beta || !verts_out || !joints_out || V < 1)
        return fail(ctx, RC_ERR_INVALID, "rc_shape_body: bad argument");
    const size_t n = (size_t)V;
    DevBuf<float> vt, sd, jr, bt, v, j;
    int rc = RC_OK;
    auto up = [&](DevBuf<float>& d, const float* h, size_t count) {
        if (rc) return;
        if (rc_alloc(d, count) != hipSuccess || (h && hipMemcpy(d.get(), h, count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))
            rc = fail(ctx, RC_ERR_HIP, "rc_shape_body: device buffer");
    };
    up(vt, v_template, n * 3); up(sd, shapedirs, n * 30); up(jr, J_regressor, n * 24); up(bt, beta, 10);
    up(v, nullptr, n * 3); up(j, nullptr, 72);
    if (!rc) {
        rc_launch_shape_body(vt.get(), sd.get(), bt.get(), jr.get(), V, v.get(), j.get(), nullptr);
        if (hipMemcpy(verts_out, v.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(joints_out, j.get(), 72 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, RC_ERR_HIP, "rc_shape_body: read back");
    }
    return rc;
}
int rc_ik_r(rc_ctx* ctx, const float* Rg, float* Rl, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_ik_r: body not set") : RC_ERR_INVALID;
    rc_launch_ik(ctx->body, Rg, Rl, n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_fk_bone(rc_ctx* ctx, const float* Rg, float* joints, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_fk_bone: body not set") : RC_ERR_INVALID;
    rc_launch_fk_bone(ctx->body, Rg, joints, n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_body_fk(rc_ctx* ctx, const float* pose, const float* tran, float* grot, float* joint, float* j33, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_body_fk: body not set") : RC_ERR_INVALID;
    if (n == 0) return RC_OK;
    if (n < 0 || !pose || !tran || !joint || !j33) return fail(ctx, RC_ERR_INVALID, "rc_body_fk: null buffer");
    rc_launch_body_fk(ctx->body, pose, tran, grot, joint, j33, n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_set_mesh(rc_ctx* ctx, const float* vt, const float* w, int32_t V) {
    if (!ctx || !vt || !w || V <= 0) return RC_ERR_INVALID;
    if (ctx->mesh_V != V) {                                 // a second call with the same V (shape change) reuses the buffers
        if (int rc = dev_alloc(ctx, &ctx->mesh_vt, (size_t)V * 3, false)) return rc;
        if (int rc = dev_alloc(ctx, &ctx->mesh_w, (size_t)V * 24, false)) return rc;
    }
    HIP_TRY(ctx, hipDeviceSynchronize());                    // nothing in flight may still read the old mesh
    HIP_TRY(ctx, hipMemcpy(ctx->mesh_vt, vt, (size_t)V * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->mesh_w, w, (size_t)V * 24 * sizeof(float), hipMemcpyHostToDevice));
    if (ctx->mesh_V != V) { ctx->mesh_Jr_h.clear(); ctx->mesh_nk = 0; }      // a regressor of another vertex count is void
    ctx->mesh_V = V;
    ctx->mesh_vt_h.assign(vt, vt + (size_t)V * 3);
    ctx->mesh_w_h.assign(w, w + (size_t)V * 24);
    ctx->fold_dirty = true;
    ctx->align_dirty = true;
    return RC_OK;
}
int rc_body_mesh(rc_ctx* ctx, const float* pose, const float* tran, float* vert, int64_t n, void* stream) {
    if (!ctx || !ctx->have_body || ctx->mesh_V == 0) return ctx ? fail(ctx, RC_ERR_STATE, "rc_body_mesh: rc_set_body / rc_set_mesh first") : RC_ERR_INVALID;
    if (n == 0) return RC_OK;
    if (!pose || !tran || !vert || n < 0) return fail(ctx, RC_ERR_INVALID, "rc_body_mesh: bad argument");
    const int64_t chunk = 65536;
    if (int rc = sweep_scratch(ctx, (size_t)rc_body_mesh_scratch_floats(std::min(n, chunk)), (hipStream_t)stream)) return rc;
    for (int64_t a = 0; a < n; a += chunk) {
        const int64_t m = std::min(chunk, n - a);
        rc_launch_body_mesh(ctx->body, ctx->mesh_vt, ctx->mesh_w, ctx->mesh_V, pose + a * 216, tran + a * 3, vert + a * ctx->mesh_V * 3, m,
                            ctx->sweep_scratch.get(), (hipStream_t)stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_set_regressor(rc_ctx* ctx, const float* Jr, int32_t n_rows, int32_t n_used) {
    if (!ctx) return RC_ERR_INVALID;
    if (ctx->mesh_V == 0) return fail(ctx, RC_ERR_STATE, "rc_set_regressor: rc_set_mesh first");
    if (!Jr || n_used < 1 || n_used > n_rows || n_used > 17) return fail(ctx, RC_ERR_INVALID, "rc_set_regressor: 1 <= n_used <= min(n_rows, 17)");
    ctx->mesh_Jr_h.assign(Jr, Jr + (size_t)n_used * ctx->mesh_V);
    ctx->mesh_nk = n_used;
    ctx->fold_dirty = true;
    return RC_OK;
}
int rc_mesh_metrics(rc_ctx* ctx, const float* pose, const float* gt_pose, int64_t n, float* per_frame, double* mean_host, void* stream) {
    if (!ctx || !ctx->have_body || ctx->mesh_V == 0) return ctx ? fail(ctx, RC_ERR_STATE, "rc_mesh_metrics: rc_set_body / rc_set_mesh first") : RC_ERR_INVALID;
    if (n <= 0 || !pose || !gt_pose || !per_frame) return fail(ctx, RC_ERR_INVALID, "rc_mesh_metrics: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const bool have_reg = ctx->mesh_nk > 0 && !ctx->mesh_Jr_h.empty();
    if (have_reg && ctx->fold_dirty) if (int rc = fold_regressor(ctx)) return rc;
    const int64_t chunk = 65536;
    if (int rc = sweep_scratch(ctx, (size_t)rc_mesh_metrics_scratch_floats(ctx->mesh_V, std::min(n, chunk)), st)) return rc;
    for (int64_t a = 0; a < n; a += chunk) {
        const int64_t m = std::min(chunk, n - a);
        rc_launch_mesh_metrics(ctx->body, ctx->mesh_vt, ctx->mesh_w, ctx->mesh_V, have_reg ? ctx->mesh_kM : nullptr, have_reg ? ctx->mesh_nk : 24,
                               pose + a * 216, gt_pose + a * 216, per_frame + a * 3, m, ctx->sweep_scratch.get(), st);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (mean_host) {                                       // evaluate.py:131-133: the three means over the sequence
        std::vector<float> h((size_t)n * 3);
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), per_frame, h.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) acc[c] += h[(size_t)i * 3 + c];
        for (int c = 0; c < 3; ++c) mean_host[c] = acc[c] / (double)n;
    }
    return RC_OK;
}
// FullMotionEvaluator (articulate/evaluator.py:317-394) of every group of a concatenated batch (kernels: rc_motion.hip). It touches nothing
// of the context but its own scratch, partial sums and group table.
int rc_motion_metrics(rc_ctx* ctx, const float* pose_p, const float* tran_p, const float* pose_t, const float* tran_t, int64_t n,
                      int32_t groups, const int64_t* group_frames_host, int32_t fps, int32_t align_joint, uint32_t joint_mask, uint32_t flags,
                      float* out, float* per_joint, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string what = "rc_motion_metrics: ";
    if (n == 0 && groups == 0) return RC_OK;
    if (n < 0 || n >= (1ll << 31)) return fail(ctx, RC_ERR_INVALID, what + "n must be in 0 .. 2^31 - 1");
    if (groups < 1) return fail(ctx, RC_ERR_INVALID, what + "groups must be positive");
    if (!pose_p || !pose_t || !out || !group_frames_host) return fail(ctx, RC_ERR_INVALID, what + "null argument");
    if (fps < 1) return fail(ctx, RC_ERR_INVALID, what + "fps must be positive");
    if (align_joint < 0 || align_joint > 23) return fail(ctx, RC_ERR_INVALID, what + "align_joint must be in 0 .. 23");
    if (joint_mask >> 24) return fail(ctx, RC_ERR_INVALID, what + "joint_mask has bits past joint 23");
    if (flags & ~(uint32_t)RC_MOTION_NO_MESH) return fail(ctx, RC_ERR_INVALID, what + "unknown flag");
    long long F = 0, blocks = 0;
    for (int g = 0; g < groups; ++g) {
        const int64_t f = group_frames_host[g];
        if (f < 1 || f > n) return fail(ctx, RC_ERR_INVALID, what + "group " + std::to_string(g) + " has " + std::to_string(f) + " frames: 1 .. n expected");
        F += f;
        blocks += (f + RC_MOTION_FG - 1) / RC_MOTION_FG;
    }
    if (F != n) return fail(ctx, RC_ERR_INVALID, what + "the groups hold " + std::to_string(F) + " frames, n is " + std::to_string(n));
    const bool mesh = !(flags & RC_MOTION_NO_MESH);
    if (!ctx->have_body) return fail(ctx, RC_ERR_STATE, what + "rc_set_body first");
    if (mesh && ctx->mesh_V == 0) return fail(ctx, RC_ERR_STATE, what + "rc_set_mesh first (or pass RC_MOTION_NO_MESH)");
    hipStream_t st = (hipStream_t)stream;
    // ---- the group table: pinned slot -> device, on `stream`
    const size_t G = (size_t)groups;
    MotionGroup* th = nullptr;
    HIP_TRY(ctx, ctx->motion_tab.stage(G, &th));
    long long at = 0, blk = 0;
    for (int g = 0; g < groups; ++g) {
        th[g].frame0 = at;
        th[g].frames = group_frames_host[g];
        th[g].blk0 = (int)blk;
        th[g].nblk = (int)((th[g].frames + RC_MOTION_FG - 1) / RC_MOTION_FG);
        at += th[g].frames;
        blk += th[g].nblk;
    }
    const size_t need_s = (size_t)rc_motion_scratch_floats(n), need_p = (size_t)rc_motion_partial_doubles(ctx->mesh_V, blocks, groups, mesh);
    if (!ctx->motion_tab.holds(G) || need_s > ctx->motion_scratch_n || need_p > ctx->motion_partial_n) {   // (kernels of earlier calls may still use the old buffers)
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, ctx->motion_tab.grow(G));
        HIP_TRY(ctx, rc_grow(ctx->motion_scratch_n, need_s, need_s, ctx->motion_scratch, need_s));
        HIP_TRY(ctx, rc_grow(ctx->motion_partial_n, need_p, need_p, ctx->motion_partial, need_p));
    }
    HIP_TRY(ctx, ctx->motion_tab.upload(G, st));
    HIP_TRY(ctx, ctx->motion_tab.record(st));
    rc_launch_motion_metrics(ctx->body, ctx->mesh_vt, ctx->mesh_w, ctx->mesh_V, ctx->motion_tab.get(), groups, blocks, pose_p, tran_p, pose_t,
                             tran_t, n, fps, align_joint, joint_mask, mesh, ctx->motion_scratch.get(), ctx->motion_partial.get(), out, per_joint, st);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
// art.math.svd_rotate (angular.py:144-184) on point sets; context-free like rc_procrustes_error
int rc_svd_rotate(const float* src, const float* dst, int64_t n, int32_t m, uint32_t what, float* R, float* t, float* s, float* moved,
                  void* stream) {
    if (n < 0 || n >= (1ll << 31) || m < 1 || (what & ~(uint32_t)(RC_ALIGN_R | RC_ALIGN_T | RC_ALIGN_S))) return RC_ERR_INVALID;
    if (n == 0) return RC_OK;
    if (!src || !dst || (!R && !t && !s && !moved)) return RC_ERR_INVALID;
    rc_launch_svd_rotate(src, dst, n, m, what, R, t, s, moved, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
// PerJointErrorEvaluator / MeshErrorEvaluator with align_joint -1 .. -5 (articulate/evaluator.py:195-209, 298-312) of every group of a
// concatenated batch (kernels: rc_align.hip). It touches nothing of the context but its own fold, scratch, partial sums and group table.
int rc_aligned_metrics(rc_ctx* ctx, const float* pose_p, const float* pose_t, int64_t n, int32_t groups, const int64_t* group_frames_host,
                       uint32_t what, uint32_t flags, float* joint_err, float* mesh_err, float* per_frame, float* xform, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string name = "rc_aligned_metrics: ";
    if (n == 0 && groups == 0) return RC_OK;
    if (n < 0 || n >= (1ll << 31)) return fail(ctx, RC_ERR_INVALID, name + "n must be in 0 .. 2^31 - 1");
    if (groups < 1) return fail(ctx, RC_ERR_INVALID, name + "groups must be positive");
    if (!pose_p || !pose_t || !group_frames_host) return fail(ctx, RC_ERR_INVALID, name + "null argument");
    if (!joint_err && !mesh_err && !per_frame && !xform) return fail(ctx, RC_ERR_INVALID, name + "no output asked for");
    if (what == 0 || (what & ~(uint32_t)(RC_ALIGN_R | RC_ALIGN_T | RC_ALIGN_S)))
        return fail(ctx, RC_ERR_INVALID, name + "what must combine RC_ALIGN_R, RC_ALIGN_T, RC_ALIGN_S");
    if (flags & ~(uint32_t)RC_MOTION_NO_MESH) return fail(ctx, RC_ERR_INVALID, name + "unknown flag");
    long long F = 0, blocks = 0;
    for (int g = 0; g < groups; ++g) {
        const int64_t f = group_frames_host[g];
        if (f < 1 || f > n) return fail(ctx, RC_ERR_INVALID, name + "group " + std::to_string(g) + " has " + std::to_string(f) + " frames: 1 .. n expected");
        F += f;
        blocks += (f + RC_MOTION_FG - 1) / RC_MOTION_FG;
    }
    if (F != n) return fail(ctx, RC_ERR_INVALID, name + "the groups hold " + std::to_string(F) + " frames, n is " + std::to_string(n));
    const bool mesh = !(flags & RC_MOTION_NO_MESH);
    if (!ctx->have_body) return fail(ctx, RC_ERR_STATE, name + "rc_set_body first");
    if (mesh && ctx->mesh_V == 0) return fail(ctx, RC_ERR_STATE, name + "rc_set_mesh first (or pass RC_MOTION_NO_MESH)");
    hipStream_t st = (hipStream_t)stream;
    if (mesh && ctx->align_dirty) if (int rc = fold_align(ctx)) return rc;      // once per mesh / body: synchronises the device
    const size_t G = (size_t)groups;
    MotionGroup* th = nullptr;
    HIP_TRY(ctx, ctx->align_tab.stage(G, &th));
    long long at = 0, blk = 0;
    for (int g = 0; g < groups; ++g) {
        th[g].frame0 = at;
        th[g].frames = group_frames_host[g];
        th[g].blk0 = (int)blk;
        th[g].nblk = (int)((th[g].frames + RC_MOTION_FG - 1) / RC_MOTION_FG);
        at += th[g].frames;
        blk += th[g].nblk;
    }
    const size_t need_s = (size_t)rc_align_scratch_floats(n), need_p = (size_t)rc_align_partial_doubles(ctx->mesh_V, n, mesh);
    if (!ctx->align_tab.holds(G) || need_s > ctx->align_scratch_n || need_p > ctx->align_partial_n) {   // (kernels of earlier calls may still use the old buffers)
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, ctx->align_tab.grow(G));
        HIP_TRY(ctx, rc_grow(ctx->align_scratch_n, need_s, need_s, ctx->align_scratch, need_s));
        HIP_TRY(ctx, rc_grow(ctx->align_partial_n, need_p, need_p, ctx->align_partial, need_p));
    }
    HIP_TRY(ctx, ctx->align_tab.upload(G, st));
    HIP_TRY(ctx, ctx->align_tab.record(st));
    const double* fold_m = reinterpret_cast<const double*>(ctx->align_fold.get());
    const AlignPair* pairs = reinterpret_cast<const AlignPair*>(ctx->align_fold.get() + 24 * 4 * sizeof(double));
    rc_launch_aligned_metrics(ctx->body, ctx->mesh_vt, ctx->mesh_w, ctx->mesh_V, fold_m, pairs, ctx->align_pairs, ctx->align_tab.get(), groups,
                              blocks, pose_p, pose_t, n, what, mesh, ctx->align_scratch.get(), ctx->align_partial.get(), joint_err, mesh_err,
                              per_frame, xform, st);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_syn_acc(const float* v, int64_t T, int64_t width, int32_t smooth_n, float* acc, void* stream) {
    if (T < 0 || width < 1 || smooth_n < 0) return RC_ERR_INVALID;                       // smooth_n 0 and 1: the plain stencil (n // 2 == 0)
    if (T == 0) return RC_OK;
    if (!v || !acc) return RC_ERR_INVALID;
    if (smooth_n / 2 != 0 && T < 2 * (int64_t)smooth_n + 1) return RC_ERR_INVALID;     // the reference raises here
    rc_launch_syn_acc(v, acc, T, width, smooth_n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_synth_imu(rc_ctx* ctx, const float* pose, const float* tran, const int32_t* vertex_ids, const int32_t* joint_ids, int64_t T,
                 int32_t smooth_n, float* imu_ori, float* imu_acc, float* joint3d, float* vert6, void* stream) {
    if (!ctx || !ctx->have_body || ctx->mesh_V == 0) return ctx ? fail(ctx, RC_ERR_STATE, "rc_synth_imu: rc_set_body / rc_set_mesh first") : RC_ERR_INVALID;
    if (T == 0) return RC_OK;
    if (T < 0 || !pose || !tran || !vertex_ids || !joint_ids || !imu_ori || !imu_acc || !vert6 || smooth_n < 0)
        return fail(ctx, RC_ERR_INVALID, "rc_synth_imu: bad argument");
    if (smooth_n / 2 != 0 && T < 2 * (int64_t)smooth_n + 1) return fail(ctx, RC_ERR_INVALID, "rc_synth_imu: needs at least 2 * smooth_n + 1 frames");
    for (int i = 0; i < 6; ++i)
        if (vertex_ids[i] < 0 || vertex_ids[i] >= ctx->mesh_V || joint_ids[i] < 0 || joint_ids[i] > 23)
            return fail(ctx, RC_ERR_INVALID, "rc_synth_imu: vertex / joint id out of range");
    hipStream_t st = (hipStream_t)stream;
    rc_launch_imu_frames(ctx->body, ctx->mesh_vt, ctx->mesh_w, vertex_ids, joint_ids, pose, tran, imu_ori, joint3d, vert6, T, st);
    rc_launch_syn_acc(vert6, imu_acc, T, 18, smooth_n, st);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
int rc_procrustes_error(const float* S1, const float* S2, int64_t n, int32_t n_points, float* err, void* stream) {
    if (n < 0 || n_points < 1) return RC_ERR_INVALID;
    if (n == 0) return RC_OK;
    if (!S1 || !S2 || !err) return RC_ERR_INVALID;
    rc_launch_procrustes(S1, S2, n_points, err, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_position_error(const float* p, const float* t, int64_t n, float* dist, double* mean_host, void* stream) {
    if (n <= 0 || !p || !t || !dist) return RC_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    rc_launch_point_distance(p, t, dist, n, st);
    if (hipGetLastError() != hipSuccess) return RC_ERR_HIP;
    if (mean_host) {
        std::vector<float> h((size_t)n);
        if (hipMemcpyAsync(h.data(), dist, h.size() * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) return RC_ERR_HIP;
        if (hipStreamSynchronize(st) != hipSuccess) return RC_ERR_HIP;
        double acc = 0.0;
        for (float v : h) acc += v;
        *mean_host = acc / (double)n;
    }
    return RC_OK;
}
int rc_set_ignored_landmarks(rc_ctx* ctx, const int32_t* ids, int32_t n) {
    if (!ctx || n < 0 || (n > 0 && !ids)) return RC_ERR_INVALID;
    unsigned long long m = 0;
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] > 32) return fail(ctx, RC_ERR_INVALID, "rc_set_ignored_landmarks: id outside 0..32");
        m |= 1ull << ids[i];
    }
    ctx->ign_mask = m;
    return RC_OK;
}
int rc_reproj_residual(rc_ctx* ctx, const float* pose, const float* tran, const float* kp, const float* K, float sigma, float* loss,
                       int64_t T, void* stream) {
    if (!ctx || !ctx->have_body) return ctx ? fail(ctx, RC_ERR_STATE, "rc_reproj_residual: body not set") : RC_ERR_INVALID;
    if (T == 0) return RC_OK;
    if (T < 0 || !pose || !tran || !kp || !K || !loss) return fail(ctx, RC_ERR_INVALID, "rc_reproj_residual: null buffer");
    rc_launch_residual(ctx->body, pose, tran, kp, K, sigma, ctx->ign_mask, loss, T, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

int rc_lstm_step(rc_ctx* ctx, const char* net, const float* x, const uint8_t* row_mask, float* y, void* stream) {
    if (!ctx || !net || !x || !y) return RC_ERR_INVALID;
    if (!ctx->have_weights) return fail(ctx, RC_ERR_STATE, "rc_lstm_step: weights not finalized");
    const int ni = net_index(net);
    if (ni < 0) return fail(ctx, RC_ERR_INVALID, std::string("rc_lstm_step: unknown net ") + net);
    hipStream_t st = (hipStream_t)stream;
    const NetDev& n = ctx->net[ni];
    if (int rc = flush_pending(ctx, st)) return rc;
    // stage x into the zero-padded rc_pk-ordered [B, 256] buffer the GEMM reads
    rc_launch_pack_rows(x, n.in, n.in, ctx->xtmp, 256, ctx->B, st);
    Stage s{ni, row_mask ? 255 : 0, ctx->xtmp, 256, Out{y, n.out, 0, false}};
    for (int phase = 0; phase < 4; ++phase) {
        GemmProblem p = phase == 0 ? lin1_problem(ctx, s) : (phase == 3 ? lin2_problem(ctx, s) : lstm_problem(ctx, s, phase - 1));
        if (int rc = launch_problems(ctx, {p}, row_mask, st)) return rc;
    }
    return mark_eager(ctx, st);
}

namespace {
// K^-1 by the adjugate in double (the reference uses torch's float32 LU inverse, evaluate.py:34,70), R_cw, gravity.
// Refused (false, nothing written): a non-finite entry of K or of the upper 3 x 4 of T_cw, det K == 0, an entry of K^-1 that is
// not finite once rounded to float -- each would turn every frame of the row into NaN.
bool camera_constants(const float* K, const float* Tcw, CamConst* cam, float* g_out) {
    for (int q = 0; q < 9; ++q) if (!std::isfinite(K[q])) return false;
    for (int q = 0; q < 12; ++q) if (!std::isfinite(Tcw[q])) return false;
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (det == 0.0) return false;
    const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                           (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                           (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
    for (int q = 0; q < 9; ++q) if (!std::isfinite((float)inv[q])) return false;
    for (int q = 0; q < 9; ++q) cam->Kinv[q] = (float)inv[q];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) cam->R[3 * r + q] = Tcw[4 * r + q];
    for (int r = 0; r < 3; ++r) g_out[r] = -cam->R[3 * r + 1];            // R_cw [0, -1, 0], evaluate.py:73
    return true;
}
}  // namespace

int rc_camera_inputs(const float* kp, const float* acc, const float* ori, const float* K, const float* Tcw, float* j2dc,
                     float* accc, float* oric, float* g_out, int64_t n, void* stream) {
    if (!K || !Tcw || !g_out || n < 0) return RC_ERR_INVALID;
    if (n > 0 && (!kp || !acc || !ori || !j2dc || !accc || !oric)) return RC_ERR_INVALID;    // before g_out is written
    CamConst cam;
    if (!camera_constants(K, Tcw, &cam, g_out)) return RC_ERR_INVALID;
    if (n == 0) return RC_OK;
    rc_launch_camera_inputs(kp, acc, ori, cam, j2dc, accc, oric, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}

int rc_camera_inputs_rows(const float* kp_norm, const float* imu_acc_w, const float* imu_ori_w, const int32_t* seq_of_row,
                          const int32_t* len, const float* K_host, const float* Tcw_host, float image_w, float image_h,
                          int32_t n_rows, int32_t Tmax, float* j2dc, float* accc, float* oric, float* gravity_out_host,
                          void* cam_scratch, void* stream) {
    if (n_rows < 0 || Tmax < 0 || !K_host || !Tcw_host || !gravity_out_host || !cam_scratch) return RC_ERR_INVALID;
    if (n_rows == 0 || Tmax == 0) return RC_OK;
    if (!kp_norm || !imu_acc_w || !imu_ori_w || !seq_of_row || !len || !j2dc || !accc || !oric) return RC_ERR_INVALID;
    std::vector<CamConst> cams((size_t)n_rows);
    std::vector<float> grav(3 * (size_t)n_rows);                          // handed out only once every row has passed
    for (int r = 0; r < n_rows; ++r)
        if (!camera_constants(K_host + 9 * (size_t)r, Tcw_host + 16 * (size_t)r, &cams[r], grav.data() + 3 * (size_t)r)) return RC_ERR_INVALID;
    std::copy(grav.begin(), grav.end(), gravity_out_host);
    hipStream_t st = (hipStream_t)stream;
    // cam_scratch: DEVICE buffer of n_rows * 72 bytes owned by the caller (the library allocates nothing here)
    if (hipMemcpyAsync(cam_scratch, cams.data(), cams.size() * sizeof(CamConst), hipMemcpyHostToDevice, st) != hipSuccess) return RC_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return RC_ERR_HIP;        // `cams` is a stack-lifetime staging buffer
    rc_launch_camera_inputs_rows(kp_norm, imu_acc_w, imu_ori_w, seq_of_row, len, (const CamConst*)cam_scratch, image_w, image_h, n_rows,
                                 Tmax, j2dc, accc, oric, st);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}

int rc_get_state(rc_ctx* ctx, const char* net, float* h_host, float* c_host, void* stream) {
    if (!ctx || !net || !h_host || !c_host) return RC_ERR_INVALID;
    const int ni = net_index(net);
    if (ni < 0) return fail(ctx, RC_ERR_INVALID, std::string("rc_get_state: unknown net ") + net);
    if (int rc = flush_pending(ctx, (hipStream_t)stream)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    const NetDev& n = ctx->net[ni];
    const size_t B = ctx->B, Bp = ctx->Bp, H = n.H;
    std::vector<float> h(2 * RC_HBUF * Bp * H);
    std::vector<int> steps(B);
    HIP_TRY(ctx, hipMemcpy(h.data(), n.h, h.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(steps.data(), n.steps, B * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(c_host, n.c, 2 * B * H * 4, hipMemcpyDeviceToHost));
    for (size_t l = 0; l < 2; ++l)
        for (size_t b = 0; b < B; ++b) {
            const float* src = h.data() + (l * RC_HBUF + (steps[b] % RC_HBUF)) * Bp * H;
            for (size_t e = 0; e < H; ++e) h_host[(l * B + b) * H + e] = src[rc_pk((long long)b, (int)e, (int)H)];
        }
    return RC_OK;
}

int rc_get_fusion_state(rc_ctx* ctx, int32_t* out_host, void* stream) {
    if (!ctx || !out_host) return RC_ERR_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    const size_t B = ctx->B;
    std::vector<int> a(B), b(B), c(B), d(B);
    std::vector<unsigned char> e(B);
    HIP_TRY(ctx, hipMemcpy(a.data(), ctx->fb.has_last, B * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(b.data(), ctx->fb.n_floor, B * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(c.data(), ctx->fb.first_reach, B * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(d.data(), ctx->fb.uv_count, B * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(e.data(), ctx->fb.pend, B, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < B; ++r) {
        out_host[5 * r] = a[r]; out_host[5 * r + 1] = b[r]; out_host[5 * r + 2] = c[r]; out_host[5 * r + 3] = d[r]; out_host[5 * r + 4] = e[r];
    }
    return RC_OK;
}

int rc_get_trace(rc_ctx* ctx, int32_t* trace_host, void* stream) {
    if (!ctx || !trace_host) return RC_ERR_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(ctx, hipMemcpy(trace_host, ctx->fb.trace, (size_t)ctx->B * 8 * 4, hipMemcpyDeviceToHost));
    return RC_OK;
}

}  // extern "C"

// camera_constants for rc_subnet_corpus (rc_subnet_api.cpp): one inverse, one refusal
bool rc_camera_constants(const float* K, const float* Tcw, CamConst* cam, float* g_out) { return camera_constants(K, Tcw, cam, g_out); }
