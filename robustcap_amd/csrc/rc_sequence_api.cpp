// The sequence engine behind rc_sequence / rc_sequence_rows: the launch planner (plan_sequence, plan_wave), the per-row-cursor wavefront engine
// with its three stream schedules (stream_tick) and the resident layer-step segment (run_resident_segment). Host logic only: this file schedules
// a call over ticks; building and launching the GEMM problems of a tick is rc_gemm_api.cpp's, and the declarations under "rc_gemm_api.cpp" in
// rc_ctx.h are all the engine takes from there. Everything it owns is a member of SeqEngine, behind rc_ctx::seq -- except the ring slots' buffers and
// x1_alt[2], which dev_alloc books with the context's other state (the live self-check saves and restores exactly those).
#include "../../include/robustcap_hip.h"
#include "rc_ctx.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#define RC_SPLIT_MAIN_MIN_BATCH 48  // wavefront engine: the tick's wide launches on streams of their own from this many rows (pick_wave_engine)

namespace {

// ====================================================================================== sequence mode of rc_sequence
// Stages of a frame in the wavefront engine below (stage s of the ring slot started at tick e runs at tick e + s):
//   0 prep | 1 linear1{rnn2,rnn4} | 2,3 LSTM l0,l1 {rnn2,rnn4} | 4 linear2{rnn2,rnn4} then fuse |
//   5 linear1{rnn6,rnn3,rnn7,rnn8} (+ init_net layer 0) | 6,7 LSTM l0,l1 (+ init_net layers 1, 2) | 8 linear2 then tail
// linear2, fuse and tail are consecutive kernels of ONE tick on the second stream, so a frame is 9 ticks deep.
// Launch groups of a tick: G_BIG = rnn6's and rnn4's layer steps (+ init_net), G_REST = the H = 512 nets' eight layer steps + the six
// linear1 -- each a whole number of rounds of equal 64-row tiles at batch 256 -- and G_LIN2 = linear2 (16-row tiles, fp32-input kernel),
// which runs with the per-row kernels prep / fuse / tail on a context-owned second stream. Three engines issue them (pick_wave_engine,
// stream_tick; docs/DESIGN_HISTORY.md has the measurements behind each):
//   plain (batch < RC_SPLIT_MAIN_MIN_BATCH: a tick is launch latency, every further stream adds hand-overs): G_BIG then G_REST on the
//          caller's stream, the second stream's hand-over in front of G_REST (of G_BIG in a tick with init_net problems);
//   split (from that batch, contexts not on the shared-weight kernel): G_BIG on the caller's stream, G_REST on wide2_stream, up to a tick ahead;
//   tri   (contexts on the shared-weight kernel, lds_context): rnn4 | rnn6 | the H = 512 nets on the caller's stream | wide2_stream |
//          wide3_stream, {linear1, init_net} at the head of the second stream's tick; rnn6 and init_net move from G_BIG to G_REST (w2_group).
// On top of tri, rc_set_resident replaces the three layer-step streams by ONE launch per segment (run_resident_segment).
// (Weight-streaming launches BESIDE the wide ones stretch those: linear1 rides in a wide launch.)
enum { SEQ_STEPPED_TR = 0, SEQ_STEPPED = 1 };
const int kRing = 16;

enum { G_BIG = 0, G_REST = 1, G_LIN2 = 2 };
struct TickStage { int kind; int net; int stage; int group; };   // kind: 0 linear1, 1 LSTM l0, 2 LSTM l1, 3 linear2; group: plain / split (tri: w2_group)
const TickStage kTick[RC_TICK_PROB] = {
    {1, N4, 2, G_BIG}, {2, N4, 3, G_BIG}, {1, N6, 6, G_BIG}, {2, N6, 7, G_BIG},
    {1, N2, 2, G_REST}, {2, N2, 3, G_REST}, {1, N3, 6, G_REST}, {2, N3, 7, G_REST}, {1, N7, 6, G_REST}, {2, N7, 7, G_REST}, {1, N8, 6, G_REST}, {2, N8, 7, G_REST},
    {0, N4, 1, G_REST}, {0, N2, 1, G_REST}, {0, N6, 5, G_REST}, {0, N3, 5, G_REST}, {0, N7, 5, G_REST}, {0, N8, 5, G_REST},
    {3, N4, 4, G_LIN2}, {3, N2, 4, G_LIN2}, {3, N6, 8, G_LIN2}, {3, N3, 8, G_LIN2}, {3, N7, 8, G_LIN2}, {3, N8, 8, G_LIN2}};
const int kFuseStage = 4, kTailStage = 8, kInitStage = 5;

}  // namespace

#pragma GCC visibility push(hidden)

// Streams stand in front of every event: default destruction releases the events first. (rc_destroy has synchronised the device.)
struct SeqEngine {
    // knobs: seq_create, rc_set_sequence_mode, rc_set_resident
    int seq_mode = 1;                    // 0 = always frame-stepped, 1 = plan per call (cost estimate), 2 = wavefront whenever long enough
    int seq_min_frames = 8;              // calls shorter than this are neither planned nor skewed (no pre-pass, no synchronisation)
    double cost_tick_us = 1.0, cost_tick_small_us = 13.0, cost_frame_us = 285.0, cost_tr_us = 55.0;   // engine choice (plan_wave): scale of the
                                                         // per-layer tick estimate, hand-over per tick, frame-stepped frame, its transition launches
    bool resident_on = false;            // rc_set_resident / RC_SEQ_RESIDENT
    int resident_wgs = 224;              // workgroups of the resident kernel (RC_SEQ_RESIDENT_WGS; the CUs it leaves run the second stream)
    // streams of a tick beside the caller's (stream_tick; caller's stream: plain both wide launches | split {rnn6, rnn4, init_net} | tri rnn4)
    HipStream aux_stream;                // the second stream, every engine: prep, linear2, fuse, tail; tri also {linear1, init_net} at the head of its tick
    HipStream wide2_stream;              // plain: unused | split: {H = 512 nets, linear1} | tri: rnn6
    HipStream wide3_stream;              // tri only: the H = 512 nets
    HipEvent ev_main[8], ev_aux[8], ev_wide2[4];   // [tick & 3]: the last wide launch of the caller's stream | the end of aux_stream's tick | wide2_stream's
                                                   // launch is done (ev_main[6], [7]: the engine's streams join the caller's)
    HipEvent ev_head[4], ev_wide3[4];    // tri only: {linear1, init_net} at the head of aux_stream's tick | wide3_stream's launch is done
    // per-row-cursor wavefront engine (run_wave2_segment)
    bool ring2_ready = false;
    bool ring2_failed = false;           // ensure_wave2_buffers failed once: not retried
    FrameBuffers ring2[kRing]{};         // ring slots: inter-stage buffers, updater inputs, frame index and step numbers per row
    float* x1_alt[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // second relu(linear1) buffer per net
    float* x1_alt2[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // third relu(linear1) buffer per net (linear1 runs up to a tick ahead of its readers)
    std::vector<GemmProblem> wave2_prob; // [16 slots][W2_PROB]
    bool wave2_valid = false;
    // tables of a planned call (reserve_plan_tables)
    DevBuf<signed char> scan_codes_d;    // [cap] regime code per (frame, row)
    PinBuf<signed char> scan_codes_h;    // pinned
    PinBuf<int> scan_state_h;            // pinned: first_reach[B] then pend[B] (as ints)
    size_t scan_cap = 0;
    DevBuf<int> frame_at_d;              // [cap] host plan: frame every row starts at every tick
    PinBuf<int> frame_at_h;              // pinned
    size_t frame_at_cap = 0;
    // rc_sequence_rows: the call's per-row lengths [B]. Two pinned copies: a call only ever waits for the upload of the call BEFORE the
    // previous one, which has long run.
    StagedTable<int, 2, 1> row_len;
    // resident layer-step kernel of the wavefront engine (run_resident_segment)
    DevBuf<ResidentTick> res_ticks_d;    // [res_cap]
    PinBuf<ResidentTick> res_ticks_h;    // pinned
    DevBuf<int> res_ints_d;              // item_base [res_cap + 1] | done [res_cap][RC_RES_MAXP] | tick_done [res_cap] | head, flag_l1, flag_tail, abort
    PinBuf<int> res_base_h;              // pinned: item_base
    PinBuf<int> res_abort_h;             // pinned: the abort word of the last segment (allocated with the first resident segment, kept with the context)
    size_t res_cap = 0;
    long long stat_wave_frames = 0, stat_stepped_frames = 0, stat_ticks = 0;
    long long stat_row_frames = 0;       // row-frames computed by sequence calls (rc_get_sequence_row_frames)
    long long stat_resident_segments = 0, stat_resident_aborts = 0;
};

void rc_seq_free(SeqEngine* e) { delete e; }

void seq_create(rc_ctx* ctx) {
    ctx->seq.reset(new SeqEngine());
    SeqEngine& e = *ctx->seq;
    e.seq_mode = tune_env("RC_SEQ_MODE", 1);          // 0 frame-stepped, 1 plan + cost estimate, 2 wavefront whenever long enough
    if (e.seq_mode < 0 || e.seq_mode > 2) e.seq_mode = 1;
    e.cost_tick_us = tune_env("RC_COST_TICK_PCT", 100) / 100.0;
    e.cost_tick_small_us = tune_env("RC_COST_HANDOVER_US", (int)e.cost_tick_small_us);
    e.cost_frame_us = tune_env("RC_COST_FRAME_US", (int)e.cost_frame_us);
    e.cost_tr_us = tune_env("RC_COST_TR_US", (int)e.cost_tr_us);
    e.resident_on = tune_env("RC_SEQ_RESIDENT", 0) != 0;
    e.resident_wgs = tune_env("RC_SEQ_RESIDENT_WGS", e.resident_wgs);
}
void seq_weights_changed(rc_ctx* ctx) { ctx->seq->wave2_valid = false; }   // the launch tables hold weight pointers
bool seq_is_engine_stream(const rc_ctx* ctx, hipStream_t st) { return st == ctx->seq->aux_stream.get(); }

#pragma GCC visibility pop

namespace {

// Frame-stepped launch plan of a rc_sequence call from the regime codes (pure host logic, exposed as rc_plan_sequence for
// tests): the three transition launches are needed on the frames where some row carries a deferred updater step INTO a frame
// it steps on camera keypoints (net/sig_mp.py:264-271 then L149-153).
// len (rc_sequence_rows; may be null): row b has frames 0 .. len[b] - 1 only -- a row that has ended asks for nothing and keeps its mark.
void plan_sequence(const signed char* codes, int B, int T, const int* pend, bool first_frame, bool use_vision_updater, unsigned char* mode,
                   const int* len = nullptr) {
    std::vector<unsigned char> pd(B);
    for (int b = 0; b < B; ++b) pd[b] = pend[b] != 0;
    for (int t = 0; t < T; ++t) {
        const signed char* c = codes + (size_t)t * B;
        bool need_tr = false;
        const bool ff = t == 0 && first_frame;
        for (int b = 0; b < B; ++b) {
            if (len && t >= len[b]) continue;
            if (pd[b] && (c[b] >= 1 || ff)) need_tr = true;                    // rnn4 steps on the camera keypoints (L149)
            pd[b] = (c[b] == 0 && use_vision_updater) ? 1 : 0;                 // L264 (non-live)
        }
        mode[t] = need_tr ? SEQ_STEPPED_TR : SEQ_STEPPED;
    }
}


// ============================================================== per-row-cursor wavefront engine
// The vision updater (net/sig_mp.py:264-271) feeds the END of a frame (landmarks of the tail) back into rnn6 / rnn4, so a row's next
// camera step has to wait for it. Rows are independent, so such a row simply LAGS the batch: every row has its own
// frame cursor.
//   * tick k initialises ring slot k % 16: row r starts its next frame there, or nothing (a bubble) when that frame has to
//     wait. The slot carries, per row, the frame index and the step number of every sub-net step the frame takes, so the stages
//     of a row's frames can be in flight at different step counts while the row's counters move on;
//   * the stages are those of the frame-stepped launch plan (step_impl) skewed over the ring: stage s of the slot initialised
//     at tick e runs at tick e + s with the slot's row flags selecting its rows (the stateless row compaction of the GEMM);
//   * an occluded frame's two updater steps RIDE the slot that is initialised at the tick its tail runs (tail = stage 8 ->
//     slot e + 8): the tail writes their inputs into that slot's x4l / x6l and marks the row there, and the steps merge into
//     that slot's own rnn4 / rnn6 launches exactly like the "merged deferred rows" of the frame-stepped plan. The row's next
//     VISIBLE frame may start at tick e + 9 at the earliest (its rnn4 / rnn6 layer steps then follow the rider's by one tick);
//     a further occluded frame starts at e + 1 as usual: an occlusion costs a row 8 ticks of lag once, at its end;
//   * the one-shot init_net (L178-183) writes rnn2's state in the tail: the row's next frame starts at e + 7;
//   * a step left pending by the frames before the segment rides slot 0; the last frame of the segment leaves its updater step
//     pending in the context's own buffers, as the frame-stepped path does.
// The host plans all of it from the regime codes of the pre-pass (plan_wave: pure host logic, exposed as rc_plan_wave) and
// uploads one table, frame_at[tick][row]; per tick it launches only the problems that have rows (collect), with tile shapes picked
// from the exact row counts (ticks that only serve lagging rows stream the weights through 16/32-row tiles).
// Arithmetic per row is that of the frame-stepped plan, operation for operation: outputs and states are bitwise equal.
enum { W2_INIT0 = RC_TICK_PROB, W2_INIT1, W2_INIT2, W2_PROB };
const int kRideStage = kTailStage;              // an updater rides the slot initialised at the tick its frame's tail runs
const int kRiderSpan = 8;                      // ... and its last launch (rnn6 l1, stage 7 of that slot) is 7 ticks later

struct WavePlan {
    int n_ticks = 0;                           // ticks to launch
    int n_prep = 0;                            // ticks [0, n_prep) initialise a slot (a row starts a frame or a rider joins)
    std::vector<int> frame_at;                 // [n_prep][B]
    std::vector<int> n_valid, n_vis, n_rider, n_reach;   // rows per slot (index = tick that initialises it)
    double est_wave_us = 0.0, est_stepped_us = 0.0;
    int lag_max = 0;                           // largest lag of a row's last frame behind the batch (ticks)
    std::vector<int> n_done;                   // rc_sequence_rows: rows whose frames have all started before slot k (empty: a uniform plan)
    int done(int k) const { return k >= 0 && k < (int)n_done.size() ? n_done[k] : 0; }
};

// t0: first frame of the segment (1 when frame 0 takes first_frame / first_tran and runs frame-stepped); first_reach / pend:
// the rows' state in front of frame t0. len (rc_sequence_rows; may be null = T for every row): row b runs frames t0 .. len[b] - 1 of
// the segment; its last frame leaves its updater step pending while the other rows go on, and a row without a frame books nothing.
void plan_wave(const signed char* codes, int B, int T, int t0, const int* first_reach, const int* pend, bool use_imu_updater,
               bool use_vision_updater, const double* cost, WavePlan& P, const int* len = nullptr) {
    const int n_frames = T - t0;
    std::vector<int> n_live((size_t)(n_frames > 0 ? n_frames : 0), 0);      // rows that have frame t0 + i
    std::vector<int> entry((size_t)B * (n_frames > 0 ? n_frames : 0));
    auto grow = [&](int tick) {
        if ((int)P.n_valid.size() <= tick) { P.n_valid.resize(tick + 1, 0); P.n_vis.resize(tick + 1, 0); P.n_rider.resize(tick + 1, 0); P.n_reach.resize(tick + 1, 0); }
    };
    int need = 0, n_prep = 0;
    P.lag_max = 0;
    std::vector<int> done_from;                                             // per row: first slot at which the row has ended
    std::vector<unsigned char> tr_frame((size_t)(n_frames > 0 ? n_frames : 0), 0);
    for (int b = 0; b < B; ++b) {
        int e_prev = -1, ready_any = 0, ready_vis = 0;
        bool fr = first_reach[b] != 0;
        bool pd = pend[b] != 0 && use_vision_updater;
        const int Tb = len ? std::min(len[b], T) : T;                       // this row's end
        if (len) done_from.push_back(Tb <= t0 ? 0 : -1);
        if (Tb <= t0) continue;
        if (pd) { grow(0); P.n_rider[0] += 1; ready_vis = 1; need = std::max(need, kRiderSpan); n_prep = std::max(n_prep, 1); }
        for (int f = t0; f < Tb; ++f) {
            const int c = codes[(size_t)f * B + b];
            const bool vis = c >= 1;
            n_live[f - t0] += 1;
            int e = std::max(e_prev + 1, ready_any);
            if (vis) e = std::max(e, ready_vis);
            entry[(size_t)b * n_frames + (f - t0)] = e;
            grow(e);
            P.n_valid[e] += 1;
            if (vis) P.n_vis[e] += 1;
            if (pd && vis) tr_frame[f - t0] = 1;                            // frame-stepped plan: transition launches on this frame
            if (fr && c == 2 && use_imu_updater) { fr = false; P.n_reach[e] += 1; ready_any = e + kRideStage - 1; }   // L178-183
            pd = c == 0 && use_vision_updater;                              // L264
            if (pd && f != Tb - 1) {
                const int ride = e + kRideStage;
                grow(ride);
                P.n_rider[ride] += 1;
                ready_vis = ride + 1;
                need = std::max(need, ride + kRiderSpan);
                n_prep = std::max(n_prep, ride + 1);
            }
            need = std::max(need, e + kRideStage + 1);
            n_prep = std::max(n_prep, e + 1);
            e_prev = e;
        }
        P.lag_max = std::max(P.lag_max, e_prev - (Tb - t0 - 1));
        if (len) done_from.back() = e_prev + 1;
    }
    P.n_ticks = need;
    P.n_prep = n_prep;
    grow(n_prep > 0 ? n_prep - 1 : 0);
    P.frame_at.assign((size_t)n_prep * B, -1);
    P.n_done.clear();
    if (len) {
        P.n_done.assign((size_t)n_prep + 1, 0);
        for (int d : done_from) if (d <= n_prep) P.n_done[d] += 1;
        for (int k = 1; k <= n_prep; ++k) P.n_done[k] += P.n_done[k - 1];
    }
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < (len ? std::min(len[b], T) : T) - t0; ++i) P.frame_at[(size_t)entry[(size_t)b * n_frames + i] * B + b] = t0 + i;
    // cost model for the engine choice. A tick = the stream hand-over + its layer steps: a layer step with >= 96 rows costs its
    // round of wide tiles (rnn4 43 us, rnn6 27.5 us, an H = 512 net 8 us: profiles/r03_timeline_mixed.txt), with fewer rows it
    // streams its weights through small tiles (~0.45 of that); cost[0] scales the whole estimate (1.0 = these figures).
    P.est_wave_us = 0.0;
    {
        const double layer_us[3] = {43.0, 27.5, 8.0};                     // rnn4 | rnn6 | H = 512 net, per layer step
        for (int k = 0; k < P.n_ticks; ++k) {
            double t = cost[1];
            auto add = [&](int stage, double us, bool big_nets) {
                const int e = k - stage;
                if (e < 0 || e >= n_prep) return;
                const int rows = big_nets ? P.n_vis[e] + P.n_rider[e] : P.n_valid[e];
                if (rows > 0) t += rows >= 96 ? us : 0.45 * us;
            };
            for (int l = 0; l < 2; ++l) {
                add(2 + l, layer_us[0], true);  add(2 + l, layer_us[2], false);                  // rnn4, rnn2
                add(6 + l, layer_us[1], true);  add(6 + l, 3 * layer_us[2], false);              // rnn6, rnn3 + rnn7 + rnn8
            }
            add(1, 3.0, false); add(5, 3.0, false);                                              // linear1 tiles
            P.est_wave_us += t * cost[0];
        }
    }
    P.est_stepped_us = 0.0;
    // A frame-stepped frame with every row (or >= 96 rows, the wide-tile bound above) costs cost[2]; with fewer rows its launches stream the
    // weights through small tiles, down to the same 0.45 of it; a frame that no row has is not launched.
    // (The share is NOT a measured constant: no ragged frame-stepped timing went into it. It is the wave model's small-tile factor, made
    // continuous in the row count, and it only has to rank the two engines for a long thin tail.)
    const int rows_full = std::min(B, 96);
    for (int i = 0; i < n_frames; ++i) {
        if (n_live[i] == 0) continue;
        const double share = n_live[i] >= rows_full ? 1.0 : 0.45 + 0.55 * n_live[i] / rows_full;
        P.est_stepped_us += cost[2] * share + (tr_frame[i] ? cost[3] : 0.0);
    }
}

static int ensure_wave2_buffers_once(rc_ctx* ctx) {
    const size_t B = (size_t)ctx->B, Bp = (size_t)ctx->Bp;
    for (int s = 0; s < kRing; ++s) {
        FrameBuffers f = ctx->fb;                      // state pointers are shared; the per-frame buffers get their own slot
        int rc = RC_OK;
#define A(ptr, n) if (!rc) rc = dev_alloc(ctx, &(ptr), (n))
        A(f.x2, Bp * 128); A(f.x3, Bp * 256); A(f.x4, Bp * 256); A(f.x6, Bp * 256); A(f.x78, Bp * 256); A(f.xi, Bp * 128);
        A(f.x4l, Bp * 256); A(f.x6l, Bp * 256);
        A(f.vr, B * 4); A(f.pc, B * 4); A(f.r6d, B * 144); A(f.contact, B * 2);
        A(f.flags, B); A(f.flags2, B); A(f.regime, B); A(f.kconf, B); A(f.frame, B); A(f.wsteps, 6 * B);
#undef A
        if (rc) return rc;
        ctx->seq->ring2[s] = f;
    }
    for (int i = 0; i < 6; ++i) {
        if (int rc = dev_alloc(ctx, &ctx->seq->x1_alt[i], Bp * ctx->net[i].H)) return rc;
        if (int rc = dev_alloc(ctx, &ctx->seq->x1_alt2[i], Bp * ctx->net[i].H)) return rc;
    }
    {
        // RC_SEQ_H512_PRIO: queue priority of wide2_stream (-1 lowest, +1 highest, 0 default). With the shared-weight kernel the caller's
        // stream carries the longest items of a tick (rnn4: the chain h(t) -> h(t + 1) is one item long); the other streams' are the filler.
        const int want = tune_env("RC_SEQ_H512_PRIO", 0);
        int lo = 0, hi = 0;
        if (want != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            HIP_TRY(ctx, hipStreamCreateWithPriority(rc_out(ctx->seq->wide2_stream), hipStreamNonBlocking, want < 0 ? lo : hi));
        else
            HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(ctx->seq->wide2_stream), hipStreamNonBlocking));
    }
    {
        // RC_SEQ_AUX_PRIO: -1 lowest / +1 highest queue priority for the second stream (0: default) -- its short kernels share the
        // CUs with the wide tiles of the caller's stream
        const int want = tune_env("RC_SEQ_AUX_PRIO", 0);
        int lo = 0, hi = 0;
        if (want != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            HIP_TRY(ctx, hipStreamCreateWithPriority(rc_out(ctx->seq->aux_stream), hipStreamNonBlocking, want < 0 ? lo : hi));
        else
            HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(ctx->seq->aux_stream), hipStreamNonBlocking));
    }
    HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(ctx->seq->wide3_stream), hipStreamNonBlocking));
    for (int i = 0; i < 8; ++i) {
        // device-scope release: the hand-over is between two streams of this GPU
        const unsigned evf = hipEventDisableTiming | hipEventReleaseToDevice;
        HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->seq->ev_main[i]), evf));
        HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->seq->ev_aux[i]), evf));
        if (i < 4) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->seq->ev_wide2[i]), evf));
        if (i < 4) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->seq->ev_head[i]), evf));
        if (i < 4) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->seq->ev_wide3[i]), evf));
    }
    ctx->seq->ring2_ready = true;
    ctx->seq->wave2_valid = false;
    return RC_OK;
}

// Ring slots, the two extra streams and the hand-over events of the wavefront engine: allocated once. A failure half-way (out of memory)
// is final for the context: the slots already allocated stay owned by it (rc_destroy frees them) and later calls report the error
// instead of allocating all 16 slots and the streams a second time on top of the partial set.
int ensure_wave2_buffers(rc_ctx* ctx) {
    if (ctx->seq->ring2_ready) return RC_OK;
    if (ctx->seq->ring2_failed) return fail(ctx, RC_ERR_STATE, "wavefront engine: its buffers could not be allocated earlier (out of memory?)");
    const int rc = ensure_wave2_buffers_once(ctx);
    if (rc != RC_OK) ctx->seq->ring2_failed = true;
    return rc;
}

// GEMM problems of every ring slot: problem q (kTick order, then the three init_net layers) working on slot sl. Rows come from
// the slot's flag bytes as in step_impl; tile shapes and row-tile counts are filled in per tick from the plan's row counts.
int build_wave2_problems(rc_ctx* ctx) {
    ctx->seq->wave2_prob.assign((size_t)kRing * W2_PROB, GemmProblem{});
    const int B = ctx->B;
    for (int sl = 0; sl < kRing; ++sl) {
        const FrameBuffers& fb = ctx->seq->ring2[sl];
        for (int q = 0; q < RC_TICK_PROB; ++q) {
            const TickStage& ts = kTick[q];
            const NetDev& n = ctx->net[ts.net];
            float* x1 = (sl & 1) ? ctx->seq->x1_alt[ts.net] : n.x1;
            Stage st{ts.net, (int)RC_ROW2_VALID, nullptr, 256, Out{nullptr, 0, 0, false}, fb.flags2};
            switch (ts.net) {
                case N4: st.x = fb.x4; st.y = Out{fb.x6, 256, 171, true}; st.flag_bit = (int)RC_ROW2_M4; st.x_alt = fb.x4l;
                         st.sel_bit = (int)RC_ROW_VIS; st.out_bit = (int)RC_ROW_VIS; break;
                case N2: st.x = fb.x2; st.ldx = 128; st.y = Out{fb.x3, 256, 72, true}; break;
                case N6: st.x = fb.x6; st.y = Out{fb.pc, 4, 0, false}; st.flag_bit = (int)RC_ROW2_M6; st.x_alt = fb.x6l;
                         st.sel_bit = (int)RC_ROW_PC; st.out_bit = (int)RC_ROW_PC; break;
                case N3: st.x = fb.x3; st.y = Out{fb.vr, 4, 0, false}; break;
                case N7: st.x = fb.x78; st.y = Out{fb.r6d, 144, 0, false}; break;
                default: st.x = fb.x78; st.y = Out{fb.contact, 2, 0, false}; break;
            }
            GemmProblem p = ts.kind == 0 ? lin1_problem(ctx, st) : (ts.kind == 3 ? lin2_problem(ctx, st) : lstm_problem(ctx, st, ts.kind - 1));
            if (ts.kind == 0) { p.out = x1; p.sel_flags = fb.flags; }
            if (ts.kind == 1) p.seg[0].base = x1;
            if (ts.kind == 3) p.out_flags = fb.flags;
            p.steps = fb.wsteps + (size_t)ts.net * B;                         // the step number travels with the slot
            p.open_step = 0; p.step_off = 0;
            ctx->seq->wave2_prob[(size_t)sl * W2_PROB + q] = p;
        }
        ctx->seq->wave2_prob[(size_t)sl * W2_PROB + W2_INIT0] = dense_problem(ctx, ctx->init[0], seg(fb.xi, 128, 0), Out{ctx->hid1, 512, 0, true}, true, RC_ROW_REACH, fb.flags, nullptr, false);
        ctx->seq->wave2_prob[(size_t)sl * W2_PROB + W2_INIT1] = dense_problem(ctx, ctx->init[1], seg(ctx->hid1, 512, 0), Out{ctx->hid2, 1024, 0, true}, true, RC_ROW_REACH, fb.flags, nullptr, false);
        ctx->seq->wave2_prob[(size_t)sl * W2_PROB + W2_INIT2] = dense_problem(ctx, ctx->init[2], seg(ctx->hid2, 1024, 0), Out{ctx->fb.init_out, 2048, 0, false}, false, RC_ROW_REACH, fb.flags, nullptr, false);
    }
    ctx->seq->wave2_valid = true;
    return RC_OK;
}

// stage of problem q (beyond kTick the init_net layers: beside linear1 / LSTM l0 / l1 of the second half)
inline int w2_stage(int q) { return q < RC_TICK_PROB ? kTick[q].stage : kInitStage + (q - W2_INIT0); }

// Which engine issues the ticks of a context (the table in front of kTick says what each puts on which stream).
enum WaveEngine { ENG_PLAIN, ENG_SPLIT, ENG_TRI };
WaveEngine pick_wave_engine(const rc_ctx* c) {
    if (c->B < RC_SPLIT_MAIN_MIN_BATCH) return ENG_PLAIN;
    return lds_context(c) ? ENG_TRI : ENG_SPLIT;
}
// ... and whether the layer steps of a whole segment go out as ONE launch of the resident kernel (run_resident_segment)
bool resident_segment(const rc_ctx* c, WaveEngine eng, const WavePlan& P) {
    // (gemm mode 2 has no resident instantiation: such a context ignores the setting and runs its segments on the three streams)
    return eng == ENG_TRI && c->seq->resident_on && gemm_mode(c) != 2 && c->B <= 256 && P.n_ticks > 0 && resident_launch_fits_timing(c);
}
// launch group of problem q: in the tri engine rnn6's layer steps and init_net leave the caller's stream to rnn4
inline int w2_group(int q, bool tri) {
    if (q >= RC_TICK_PROB) return tri ? G_REST : G_BIG;
    return (tri && kTick[q].net == N6 && kTick[q].group == G_BIG) ? G_REST : kTick[q].group;
}

// 64-row tile shapes (16-row x 16-column blocks) of the wide launches: rnn4 | rnn6 | the H = 512 nets. One stream for both wide launches
// (plain): rnn4 on 64 x 80 tiles, 256 per layer = whole rounds of the CUs; beside a launch on another stream the 64 x 128 tile's fewer
// operand bytes per MFMA win.
struct WaveTiles { int t4[2], t6[2], t5[2]; };
WaveTiles wave_tiles(WaveEngine eng) {
    WaveTiles t{{4, eng == ENG_PLAIN ? 5 : 8}, {4, 8}, {4, 8}};
    tile_env("RC_SEQ_RNN4", &t.t4[0], &t.t4[1]);
    tile_env("RC_SEQ_RNN6", &t.t6[0], &t.t6[1]);
    tile_env("RC_SEQ_H512", &t.t5[0], &t.t5[1]);
    return t;
}

// the plan's table frame_at [ticks][B], device + pinned (grow-only: the caller makes sure nothing in flight reads it)
int reserve_frame_at(rc_ctx* ctx, size_t need, size_t want) {
    HIP_TRY(ctx, rc_grow(ctx->seq->frame_at_cap, need, want, ctx->seq->frame_at_d, want, ctx->seq->frame_at_h, want));
    return RC_OK;
}

// The problems of launch group g that have rows at tick k, with tile shapes picked from the exact row counts.
std::vector<GemmProblem> collect(const rc_ctx* ctx, const WavePlan& P, WaveEngine eng, const WaveTiles& tiles, int k, int g) {
    // rows of a problem from which it runs 64-row tiles (split products): a half-filled 64-row tile still halves the weight bytes of two 32-row tiles
    static const int tile64_rows = tune_env("RC_SEQ_TILE64_ROWS", 33);
    static const bool rows_as_padded = tune_env("RC_SEQ_ROWS_AS_PADDED", 1) != 0;      // 0: choose for the rows that are left (A/B runs)
    const int B = ctx->B;
    std::vector<GemmProblem> ps;
    for (int qi = 0; qi < W2_PROB; ++qi) {
        const int q = qi < 4 ? (qi ^ 2) : qi;                                 // rnn6 (kTick 2, 3) in front of rnn4 (0, 1): longest tiles first
        if (w2_group(q, eng == ENG_TRI) != g) continue;
        const int e = k - w2_stage(q);
        if (e < 0 || e >= P.n_prep) continue;
        const int net = q < RC_TICK_PROB ? kTick[q].net : -1;
        const int kind = q < RC_TICK_PROB ? kTick[q].kind : 4;                 // 4: init_net layer
        const int riders = P.n_rider[e];
        const int rows = kind == 4 ? P.n_reach[e] : ((net == N4 || net == N6) ? P.n_vis[e] + riders : P.n_valid[e]);
        if (rows <= 0) continue;
        // Kernel and tile shape of a problem are chosen for `rows_k` rows. In a plan with per-row ends (rc_sequence_rows) that is the count
        // the PADDED call would have at this slot -- a padding row is occluded: it steps every net, rnn4 / rnn6 as a rider -- so a batch
        // that thins out stays on the kernel and tiles of the full batch; the row tiles still follow the rows that are there.
        const int rows_k = kind == 4 ? rows : rows + (rows_as_padded ? P.done(e) : 0);
        GemmProblem p = ctx->seq->wave2_prob[(size_t)(e % kRing) * W2_PROB + q];
        if (kind == 0 || kind == 1) {                                          // relu(linear1) of the frame started at tick e: one of three buffers
            float* x1 = e % 3 == 0 ? ctx->net[net].x1 : (e % 3 == 1 ? ctx->seq->x1_alt[net] : ctx->seq->x1_alt2[net]);
            if (kind == 0) p.out = x1; else p.seg[0].base = x1;
        }
        if (kind == 1 || kind == 2) {
            const NetDev& n = ctx->net[net];
            int mr, nc;
            if (lds_problem(ctx, rows_k)) {                                    // the shared-weight kernel (rc_gemm_lds.hip)
                mr = 16; nc = 8;
            } else if (gemm_split(ctx) && rows_k >= tile64_rows) {              // (split products: the K loop is operand-bound, 64-row tiles)
                const int* t = n.H == 512 ? tiles.t5 : (n.H == 1024 ? tiles.t6 : tiles.t4);
                mr = t[0]; nc = t[1];
            } else {
                pick_tile(n.H, rows_k, &mr, &nc);
            }
            p.mr = mr; p.nc = nc; p.n_tiles = n.H / (4 * nc);
        } else if (kind == 0 || kind == 4) {
            if (rows_k <= 16) { p.mr = 1; p.nc = 1; p.n_tiles = (p.N + 15) / 16; }
            else if (kind == 0 && gemm_split(ctx) && rows_k >= tile64_rows) {
                // linear1 rides in a wide launch behind its 256 LSTM tiles: as 544 tiles of 32 x 64 (K = 128 / 256: two k-blocks, i.e. all
                // prologue and epilogue) it added two rounds, ~18 us of a 245 us tick; 136 tiles of 64 x 128 add one
                const int np = round_up(p.N, 64);
                if (np % 128 == 0) { p.mr = 4; p.nc = 8; p.n_tiles = np / 128; }
            }
        }
        p.m_tiles = (rows + 16 * p.mr - 1) / (16 * p.mr);
        if (rows == B && kind != 4) {                                          // every row: no compaction needed
            p.flags = nullptr; p.flag_bit = 0;
            if (riders == 0 && (net == N4 || net == N6) && P.n_vis[e] == B) {
                p.alt_base = nullptr; p.sel_flags = nullptr; p.sel_bit = 0; p.out_flags = nullptr; p.out_bit = 0;
            }
        }
        ps.push_back(p);
    }
    // Filling and draining ticks (and ticks of lagging rows) carry fewer problems per launch: when the launch would leave
    // half of the CUs without a tile, the 64 x 128 tiles are cut to 64 x 64 (twice the tiles, half as long each).
    if (g != G_LIN2) {
        int total = 0;
        for (const GemmProblem& p : ps) total += p.n_tiles * p.m_tiles;
        if (total > 0 && total <= 128)
            for (GemmProblem& p : ps)
                if (p.epi == RC_EPI_LSTM && p.mr == 4 && p.nc == 8) { p.nc = 4; p.n_tiles *= 2; }
    }
    return ps;
}

struct WaveSeg {                               // one segment on the wavefront engine: what its ticks share
    rc_ctx* ctx; const WavePlan& P; const FrameIO& io0; hipStream_t st, aux;          // caller's stream, second stream
    WaveEngine eng; WaveTiles tiles; rc_params_dev prm; WavePrep wp; WaveTail wt;
    int rows(const std::vector<int>& v, int tick) const { return tick >= 0 && tick < P.n_prep ? v[tick] : 0; }   // of the slot initialised at `tick`
    std::vector<GemmProblem> group(int k, int g) const { return collect(ctx, P, eng, tiles, k, g); }
};

// prep of tick k on the second stream: initialises ring slot k % 16 (before the tick's tail, whose target slot it is)
void wave_prep(WaveSeg& S, int k) {
    if (k >= S.P.n_prep) return;
    S.wp.frame_at = S.ctx->seq->frame_at_d.get() + (size_t)k * S.ctx->B;
    S.wp.first_tick = k == 0 ? 1 : 0;
    rc_launch_prep_wave(S.ctx->seq->ring2[k % kRing], S.io0, S.prm, S.ctx->B, S.wp, S.aux);
}

// linear2 of stages 4 and 8 on the second stream (fp32-input kernel, as in run_stage), then their consumers fuse and tail -- ONE launch where
// `merge` allows and both have rows. `signal` (may be null) rides on the last kernel where there is a tail and is recorded behind the chain otherwise.
int wave_lin2_fuse_tail(WaveSeg& S, int k, bool merge, hipEvent_t signal) {
    rc_ctx* ctx = S.ctx;
    const int B = ctx->B;
    if (int rc = launch_problems(ctx, S.group(k, G_LIN2), nullptr, S.aux, true)) return rc;
    const bool fuse = S.rows(S.P.n_valid, k - kFuseStage) > 0, tail = S.rows(S.P.n_valid, k - kTailStage) > 0;
    bool merged = false, carried = false;
    if (tail) {
        const FrameBuffers& tgt = ctx->seq->ring2[k % kRing];
        S.wt.x4l = tgt.x4l; S.wt.x6l = tgt.x6l; S.wt.flags2 = tgt.flags2; S.wt.wsteps = tgt.wsteps;
    }
    if (merge && fuse && tail)
        merged = carried = rc_launch_fuse_tail(ctx->seq->ring2[(k - kTailStage) % kRing], ctx->seq->ring2[(k - kFuseStage) % kRing], S.io0, S.prm, ctx->body, B, S.wt, S.aux, signal);
    if (!merged && fuse) rc_launch_fuse(ctx->seq->ring2[(k - kFuseStage) % kRing], S.io0, S.prm, B, S.aux);
    if (!merged && tail) {
        rc_launch_tail(ctx->seq->ring2[(k - kTailStage) % kRing], S.io0, S.prm, ctx->body, B, 0, S.aux, nullptr, &S.wt, signal);
        carried = true;
    }
    if (signal && !carried) HIP_TRY(ctx, hipEventRecord(signal, S.aux));
    return RC_OK;
}

inline int wave_wait(rc_ctx* ctx, int k, hipStream_t s, std::initializer_list<hipEvent_t> waits) {   // events of tick k - 1: tick 0 has none; null = none
    if (k > 0) for (hipEvent_t w : waits) if (w) HIP_TRY(ctx, hipStreamWaitEvent(s, w, 0));
    return RC_OK;
}

// One wide launch of tick k: the problems `ps` on stream s behind `waits`. `signal` rides on the launch itself where one goes out
// (launch_problems) and is recorded behind it otherwise.
int wave_issue(rc_ctx* ctx, int k, hipStream_t s, std::initializer_list<hipEvent_t> waits, const std::vector<GemmProblem>& ps, hipEvent_t signal) {
    if (int rc = wave_wait(ctx, k, s, waits)) return rc;
    bool carried = false;
    if (int rc = launch_problems(ctx, ps, nullptr, s, false, signal, &carried)) return rc;
    if (signal && !carried) HIP_TRY(ctx, hipEventRecord(signal, s));
    return RC_OK;
}

// Tick k of the three stream engines. Events with index e belong to this tick, with ep to the previous one; each line reads
// stream <- {what it waits for}, what it launches, what it signals. tests/test_wave_streams.py models exactly these edges.
int stream_tick(WaveSeg& S, int k) {
    rc_ctx* ctx = S.ctx;
    const int e = k & 3, ep = (k + 3) & 3;
    hipStream_t st = S.st, aux = S.aux, w2 = ctx->seq->wide2_stream.get(), w3 = ctx->seq->wide3_stream.get();
    hipEvent_t main_p = ctx->seq->ev_main[ep].get(), aux_p = ctx->seq->ev_aux[ep].get(), w2_p = ctx->seq->ev_wide2[ep].get(), w3_p = ctx->seq->ev_wide3[ep].get(),
               head_p = ctx->seq->ev_head[ep].get();
    hipEvent_t main_e = ctx->seq->ev_main[e].get(), aux_e = ctx->seq->ev_aux[e].get(), w2_e = ctx->seq->ev_wide2[e].get(), w3_e = ctx->seq->ev_wide3[e].get(),
               head_e = ctx->seq->ev_head[e].get();
    bool init_now = false;                                                     // init_net problems in this tick
    for (int q = W2_INIT0; q < W2_PROB; ++q) init_now = init_now || S.rows(S.P.n_reach, k - w2_stage(q)) > 0;
    if (S.eng == ENG_TRI) {
        // {linear1, init_net} read what the second stream wrote in tick k - 1 and nothing else: the head of its tick. prep reads no layer
        // step either: in front of the waits. Then each net's chain h(t) -> h(t + 1) on a stream of its own, behind the previous linear1.
        std::vector<GemmProblem> l1, rnn6, h512;
        for (const GemmProblem& p : S.group(k, G_REST)) (p.epi != RC_EPI_LSTM ? l1 : (p.H == 1024 ? rnn6 : h512)).push_back(p);
        if (int rc = wave_issue(ctx, k, aux, {}, l1, head_e)) return rc;
        wave_prep(S, k);
        if (int rc = wave_wait(ctx, k, aux, {w3_p, main_p, w2_p})) return rc;
        if (int rc = wave_lin2_fuse_tail(S, k, true, aux_e)) return rc;
        if (int rc = wave_issue(ctx, k, w2, {head_p}, rnn6, w2_e)) return rc;
        // The H = 512 nets NEED linear1(k - 1) like the other two, and the END of the second stream's previous tick only behind an init_net
        // state write of its tail (rnn2 l0): RC_SEQ_H5_EARLY=1 issues exactly that (the edges tests/test_wave_streams.py models) and is
        // slower -- the three layer-step launches do better in step with each other (profiles/r06_resident_notes.txt). Default: the end, always.
        static const int h5_early = tune_env("RC_SEQ_H5_EARLY", 0);
        const bool early = h5_early && S.rows(S.P.n_reach, k - 1 - kTailStage) == 0;
        if (int rc = wave_issue(ctx, k, w3, {early ? head_p : aux_p}, h512, w3_e)) return rc;
        if (int rc = wave_issue(ctx, k, st, {head_p}, S.group(k, G_BIG), main_e)) return rc;
    } else if (S.eng == ENG_SPLIT) {
        // {H = 512 nets, linear1} only needs the second stream's previous tick and its own predecessor, {rnn6, rnn4} only the previous
        // linear1 (init_net also the previous fuse): the former runs up to a tick ahead and fills the CUs the latter's last round leaves idle
        if (int rc = wave_wait(ctx, k, aux, {main_p, w2_p})) return rc;
        wave_prep(S, k);
        if (int rc = wave_lin2_fuse_tail(S, k, false, aux_e)) return rc;
        if (int rc = wave_issue(ctx, k, w2, {aux_p}, S.group(k, G_REST), w2_e)) return rc;
        if (int rc = wave_issue(ctx, k, st, {w2_p, init_now ? aux_p : nullptr}, S.group(k, G_BIG), main_e)) return rc;
    } else {
        // Both wide launches on the caller's stream. Only linear1 and init_net READ what the second stream wrote in the previous tick: the
        // wait stands in front of the launch that holds them, and {rnn6, rnn4} follows the previous tick without a barrier packet
        // (legal with the third copy of the hidden state, RC_HBUF: it WRITES h where linear2 of the previous tick still reads)
        if (int rc = wave_wait(ctx, k, aux, {main_p})) return rc;
        wave_prep(S, k);
        if (int rc = wave_lin2_fuse_tail(S, k, false, aux_e)) return rc;
        if (int rc = wave_issue(ctx, k, st, {init_now ? aux_p : nullptr}, S.group(k, G_BIG), nullptr)) return rc;
        if (int rc = wave_issue(ctx, k, st, {init_now ? nullptr : aux_p}, S.group(k, G_REST), main_e)) return rc;
    }
    ctx->seq->stat_ticks += 1;
    return RC_OK;
}

// ---- resident layer-step kernel ----------------------------------------------------------------------------------------------------
// On streams, a tick's layer steps are launches: every launch ends in a drain of the CUs it held, starts behind an event, and its
// workgroups queue for CUs against the other streams' (profiles/r06_lds_kernel_notes.txt, r06_timeline_tri_high.txt). Here ONE launch
// carries the layer steps of the whole segment (rc_gemm_lds.hip: rc_gemm_resident_kernel): its workgroups take items tick after tick from
// a queue in device memory, ordered by counters instead of events, and leave the other CUs to the second stream, whose chain [init_net] ->
// prep -> [all items of the previous tick] -> linear2 -> fuse -> tail talks to the layer steps through one flag and one counter per tick.
// Same items, same arithmetic: bitwise the streams' result.
struct ResidentWords { int *item_base, *done, *tick_done, *words; };           // res_ints_d; words: head, (unused), flag_tail, abort

// The table: per tick its layer steps AND its linear1 problems as items (as launches on the CUs the resident kernel leaves they took 86-197 us
// of every tick, profiles/r06_timeline_resident_l1_*.txt), slab region = tick % 4 (a tick starts behind every item of the tick before the
// previous one), and what each problem reads of the previous tick. init_net's layers stay launches of the second stream: init_l[tick].
int build_resident_ticks(WaveSeg& S, std::vector<std::vector<GemmProblem>>& init_l) {
    rc_ctx* ctx = S.ctx;
    int run = 0;
    for (int k = 0; k < S.P.n_ticks; ++k) {
        std::vector<GemmProblem> ls;
        for (int g : {G_BIG, G_REST})
            for (GemmProblem& p : S.group(k, g)) {
                if (p.epi == RC_EPI_LSTM) { p.mr = 16; p.nc = 8; }
                else if (p.epi == RC_EPI_RELU && p.out_packed && p.N % 128 == 0 && p.Kp % 128 == 0 && p.out_bit == 0 && p.out_col0 == 0 && p.seg[0].par_mode == 0 &&
                         p.out != ctx->hid1 && p.out != ctx->hid2) { }
                else { init_l[k].push_back(p); continue; }
                p.m_tiles = 1;                                                 // (B <= 256: one row tile, whatever the tick's row count)
                ls.push_back(p);
            }
        ResidentTick& T = ctx->seq->res_ticks_h[k];
        LdsRegion region{};
        if (int rc = lds_region(ctx, (size_t)(k & 3), &region)) return rc;
        size_t tiles = 0;
        T.B = ctx->B;
        T.n = build_lds_problems(ctx, ls, nullptr, region.slab, region.tickets, T.p, RC_RES_MAXP, &T.n_items, &tiles, true);
        if (T.n != (int)ls.size()) return fail(ctx, RC_ERR_INVALID, "resident engine: more problems in a tick than its table holds");
        if (tiles > region.tiles) return fail(ctx, RC_ERR_INVALID, "resident engine: more tiles in a tick than a slab region holds");
        const bool tail_wrote = S.rows(S.P.n_reach, k - 1 - kTailStage) > 0;
        for (int i = 0; i < RC_RES_MAXP; ++i) {
            T.dep[i][0] = T.dep[i][1] = -1; T.dep_items[i][0] = T.dep_items[i][1] = 0;
            T.need_tail[i] = 0;
            if (i >= T.n) continue;
            const bool lstm = T.p[i].epi == RC_EPI_LSTM;
            T.need_tail[i] = lstm ? ((tail_wrote && T.p[i].H == 512) ? 1 : 0) : 1;
            if (k == 0 || !lstm) continue;
            const ResidentTick& Tp = ctx->seq->res_ticks_h[k - 1];
            for (int j = 0; j < Tp.n; ++j) {
                const int items_j = (j + 1 < Tp.n ? Tp.p[j + 1].wg_base : Tp.n_items) - Tp.p[j].wg_base;
                const bool lstm_j = Tp.p[j].epi == RC_EPI_LSTM;
                if (lstm_j && Tp.p[j].hstate == T.p[i].hstate) { T.dep[i][0] = j; T.dep_items[i][0] = items_j; }                           // its own h(t - 1), c
                if ((const float*)(lstm_j ? Tp.p[j].hstate : Tp.p[j].out) == T.p[i].seg[0].base) { T.dep[i][1] = j; T.dep_items[i][1] = items_j; }   // layer 0's h | relu(linear1)
            }
        }
        ctx->seq->res_base_h[k] = run;
        run += T.n_items;
    }
    ctx->seq->res_base_h[S.P.n_ticks] = run;
    return RC_OK;
}

int run_resident_segment(WaveSeg& S) {
    rc_ctx* ctx = S.ctx;
    hipStream_t st = S.st, aux = S.aux;
    const int res_wgs = std::min(240, std::max(8, ctx->seq->resident_wgs));
    LdsRegion pool{};
    if (int rc = lds_region(ctx, 0, &pool)) return rc;                             // (the pool is allocated in front of everything else the segment needs)
    if (!ctx->seq->res_abort_h) {                                                  // (read by the next rc_sequence call: kept until rc_destroy)
        HIP_TRY(ctx, rc_alloc(ctx->seq->res_abort_h, 1));
        ctx->seq->res_abort_h[0] = 0;
    }
    const size_t nt = (size_t)S.P.n_ticks;
    if (nt > ctx->seq->res_cap) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        const size_t cap = nt + nt / 4 + 64;
        HIP_TRY(ctx, rc_grow(ctx->seq->res_cap, nt, cap, ctx->seq->res_ticks_d, cap, ctx->seq->res_ticks_h, cap,
                             ctx->seq->res_ints_d, cap * (RC_RES_MAXP + 2) + 1 + 4 + 16, ctx->seq->res_base_h, cap + 1));   // (+ 16: the sums of a -DRC_RES_PROF build)
    }
    const size_t cap = ctx->seq->res_cap;
    ResidentWords W{};
    W.item_base = ctx->seq->res_ints_d.get(); W.done = W.item_base + cap + 1; W.tick_done = W.done + cap * RC_RES_MAXP; W.words = W.tick_done + cap;
    std::vector<std::vector<GemmProblem>> init_l(nt);
    if (int rc = build_resident_ticks(S, init_l)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->seq->res_ticks_d.get(), ctx->seq->res_ticks_h.get(), nt * sizeof(ResidentTick), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(W.item_base, ctx->seq->res_base_h.get(), (nt + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(W.done, 0, (cap * (RC_RES_MAXP + 1) + 4 + 16) * sizeof(int), st));
    HIP_TRY(ctx, hipEventRecord(ctx->seq->ev_main[6].get(), st));
    HIP_TRY(ctx, hipStreamWaitEvent(aux, ctx->seq->ev_main[6].get(), 0));
    ResidentArgs R{};
    R.ticks = ctx->seq->res_ticks_d.get(); R.item_base = W.item_base; R.n_ticks = S.P.n_ticks;
    R.head = W.words; R.done = W.done; R.tick_done = W.tick_done;
    R.flag_tail = W.words + 2; R.abort = W.words + 3;
    R.spin_bound = (unsigned long long)std::max(1, tune_env("RC_SEQ_RESIDENT_BOUND_MS", 2000)) * 100000ull;   // wall_clock64: 100 MHz
    if (int rc = timed_launch(ctx, st, LAUNCH_RESIDENT, [&] { rc_launch_gemm_resident(R, res_wgs, st); })) return rc;
    count_resident_launch(ctx);
    // second stream, tick k: [init_net] -> prep -> [every item of tick k - 1] -> linear2 -> fuse -> tail -> flag_tail = k + 1
    for (int k = 0; k < S.P.n_ticks; ++k) {
        if (int rc = launch_problems(ctx, init_l[k], nullptr, aux, false)) return rc;
        wave_prep(S, k);
        if (k > 0) rc_launch_flag_wait(W.tick_done + (k - 1), ctx->seq->res_ticks_h[k - 1].n_items, W.words + 3, R.spin_bound, aux);
        if (int rc = wave_lin2_fuse_tail(S, k, false, nullptr)) return rc;
        rc_launch_flag_set(W.words + 2, k + 1, aux);
        ctx->seq->stat_ticks += 1;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->seq->ev_aux[0].get(), aux));
    HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->seq->ev_aux[0].get(), 0));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->seq->res_abort_h.get(), W.words + 3, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipGetLastError());
#ifdef RC_RES_PROF
    {   // profiling builds (tools/probe_resprof.so): where the resident workgroups' time went, per item
        HIP_TRY(ctx, hipStreamSynchronize(st));
        unsigned long long ph[5];
        const unsigned long long* pd = (const unsigned long long*)(((unsigned long long)(W.words + 4) + 7ull) & ~7ull);
        if (hipMemcpy(ph, pd, sizeof(ph), hipMemcpyDeviceToHost) == hipSuccess && ph[2] > 0)
            std::fprintf(stderr, "[res prof] %d ticks, %llu items on %d workgroups; per item: wait %.2f us, item %.2f us, release %.2f us, take %.2f us; per workgroup %.2f ms\n",
                         S.P.n_ticks, ph[2], res_wgs, ph[0] / 100.0 / ph[2], ph[1] / 100.0 / ph[2], ph[3] / 100.0 / ph[2], ph[4] / 100.0 / ph[2],
                         (ph[0] + ph[1] + ph[3] + ph[4]) / 100.0 / 1000.0 / res_wgs);
    }
#endif
    ctx->seq->stat_resident_segments += 1;
    return RC_OK;
}

// Frames t0 .. t_last of a rc_sequence call on the wavefront engine: upload the plan's table, let the engine's streams join the caller's,
// issue every tick (or the resident segment), and let the caller's stream wait for the last tick of every other stream.
int run_wave2_segment(rc_ctx* ctx, const WavePlan& P, const FrameIO& io0, int t0, int t_last, hipStream_t st) {
    const int B = ctx->B;
    const size_t need = (size_t)P.n_prep * B;                                  // the plan's table: frame every row starts at every tick
    if (need > ctx->seq->frame_at_cap) {
        HIP_TRY(ctx, hipDeviceSynchronize());                               // nothing in flight (on any of the engine's streams) may still read the old table
        if (int rc = reserve_frame_at(ctx, need, need + need / 4 + 4096)) return rc;
    }
    std::memcpy(ctx->seq->frame_at_h.get(), P.frame_at.data(), need * sizeof(int));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->seq->frame_at_d.get(), ctx->seq->frame_at_h.get(), need * sizeof(int), hipMemcpyHostToDevice, st));

    const WaveEngine eng = pick_wave_engine(ctx);
    WaveSeg S{ctx, P, io0, st, ctx->seq->aux_stream.get(), eng, wave_tiles(eng), dev_params(ctx->prm), WavePrep{}, WaveTail{}};
    for (int i = 0; i < 6; ++i) S.wp.steps[i] = ctx->net[i].steps;
    S.wp.cx4l = ctx->fb.x4l; S.wp.cx6l = ctx->fb.x6l; S.wp.t0 = t0;
    S.wt.on = 1; S.wt.t_last = t_last;
    S.wt.steps4 = ctx->net[N4].steps; S.wt.steps6 = ctx->net[N6].steps;
    S.wt.cx4l = ctx->fb.x4l; S.wt.cx6l = ctx->fb.x6l;
    hipStream_t w2 = ctx->seq->wide2_stream.get(), w3 = ctx->seq->wide3_stream.get();
    HIP_TRY(ctx, hipEventRecord(ctx->seq->ev_main[7].get(), st));                    // the engine's streams join (also: the table upload)
    HIP_TRY(ctx, hipStreamWaitEvent(S.aux, ctx->seq->ev_main[7].get(), 0));
    if (eng != ENG_PLAIN) HIP_TRY(ctx, hipStreamWaitEvent(w2, ctx->seq->ev_main[7].get(), 0));
    if (eng == ENG_TRI) HIP_TRY(ctx, hipStreamWaitEvent(w3, ctx->seq->ev_main[7].get(), 0));
    if (resident_segment(ctx, eng, P)) {
        if (int rc = run_resident_segment(S)) return rc;
    } else {
        for (int k = 0; k < P.n_ticks; ++k) if (int rc = stream_tick(S, k)) return rc;
        const int last = (P.n_ticks - 1) & 3;
        if (P.n_ticks > 0) {
            HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->seq->ev_aux[last].get(), 0));
            if (eng != ENG_PLAIN) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->seq->ev_wide2[last].get(), 0));
            if (eng == ENG_TRI) {
                HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->seq->ev_head[last].get(), 0));
                HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->seq->ev_wide3[last].get(), 0));
                HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->seq->ev_main[last].get(), 0));
            }
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->seq->stat_wave_frames += t_last - t0 + 1;
    return RC_OK;
}

// pinned + device tables of a planned rc_sequence call of T frames: regime codes [T][B], the rows' state, frame_at [ticks][B]
int reserve_plan_tables(rc_ctx* ctx, int T) {
    const size_t B = (size_t)ctx->B;
    const size_t need = B * (size_t)T;
    HIP_TRY(ctx, rc_grow(ctx->seq->scan_cap, need, need, ctx->seq->scan_codes_d, need, ctx->seq->scan_codes_h, need));
    if (!ctx->seq->scan_state_h) HIP_TRY(ctx, rc_alloc(ctx->seq->scan_state_h, B * 3));
    const size_t fneed = B * ((size_t)T + 64);                                  // ticks of a T-frame plan: T + pipeline depth + lag
    return reserve_frame_at(ctx, fneed, fneed);
}

}  // namespace

// rc_finalize_weights: everything the engine allocates on first use -- the 16 ring slots, its three streams and 28 events, the launch tables,
// the plan's pinned tables for calls of up to 1024 frames -- is set up THERE, not inside the first planned rc_sequence call (which used to cost
// that call 13 ms inside its caller's timed region). Longer calls still grow the tables once; a context whose mode is switched on later
// allocates in its first planned call (sequence_impl).
int seq_prepare(rc_ctx* ctx) {
    if (!ctx->seq->seq_mode || ctx->prm.live) return RC_OK;
    if (int rc = ensure_wave2_buffers(ctx)) return rc;
    if (int rc = build_wave2_problems(ctx)) return rc;
    return reserve_plan_tables(ctx, 1024);
}

// =============================================================================================== C ABI
extern "C" {

// rc_sequence (len == nullptr) and rc_sequence_rows: frames [off, off + T) of a call whose per-row lengths are len[B] (HOST; their device
// copy is ctx->seq->row_len), the pointers standing at frame `off`. Row b has frames 0 .. min(len[b] - off, T) - 1 of this piece.
static int sequence_impl(rc_ctx* ctx, int32_t T, const int32_t* len, int32_t off, const float* j2dc, int64_t rs_j2d, const float* accc,
                         int64_t rs_acc, const float* oric, int64_t rs_ori, const float* first_tran, uint32_t flags, float* pose_out,
                         int64_t rs_pose, float* tran_out, int64_t rs_tran, void* stream) {
    std::vector<int> rows_len;                                              // this piece's per-row lengths (empty: every row runs every frame)
    if (len) {
        rows_len.resize(ctx->B);
        int longest = 0;
        bool same = true;
        for (int b = 0; b < ctx->B; ++b) {
            rows_len[b] = std::max(0, std::min(len[b] - off, T));
            longest = std::max(longest, rows_len[b]);
            same = same && rows_len[b] == rows_len[0];
        }
        if (longest == 0) return RC_OK;                                     // no row has a frame here: nothing is enqueued
        T = longest;                                                        // frames that no row has are not launched
        if (same) rows_len.clear();                                         // ... and rows of one length are a uniform call
    }
    const int* L = rows_len.empty() ? nullptr : rows_len.data();
    const int* len_d = L ? ctx->seq->row_len.get() : nullptr;
    // Very long calls are planned in pieces: the plan's tables (regime codes, frame_at) grow with batch x frames, and a piece
    // boundary costs one pipeline drain (8 of 4,096 ticks) and one more read-back.
    const int32_t kMaxPlanFrames = std::max(8, tune_env("RC_SEQ_MAX_PLAN_FRAMES", 4096));     // (read per call: tests shrink it)
    if (T > kMaxPlanFrames && ctx->seq->seq_mode && !ctx->prm.live) {
        for (int32_t a = 0; a < T; a += kMaxPlanFrames) {
            const int32_t n = std::min(kMaxPlanFrames, T - a);
            if (int rc = sequence_impl(ctx, n, L ? len : nullptr, off + a, j2dc + (int64_t)a * 99, rs_j2d, accc + (int64_t)a * 18, rs_acc, oric + (int64_t)a * 54, rs_ori,
                                     a == 0 ? first_tran : nullptr, a == 0 ? flags : 0u, pose_out + (int64_t)a * 216, rs_pose,
                                     tran_out + (int64_t)a * 3, rs_tran, stream)) return rc;
        }
        return RC_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    auto io_at = [&](int t) {
        return FrameIO{j2dc + (int64_t)t * 99, accc + (int64_t)t * 18, oric + (int64_t)t * 54, t == 0 ? first_tran : nullptr,
                       pose_out + (int64_t)t * 216, tran_out + (int64_t)t * 3, rs_j2d, rs_acc, rs_ori, rs_pose, rs_tran, len_d, off + t};
    };
    std::vector<int> n_live;                                                // rows that have frame t (the host knows: tile choice)
    if (L) {
        n_live.assign((size_t)T + 1, 0);
        for (int b = 0; b < ctx->B; ++b) n_live[L[b]] += 1;                 // rows ending at t ...
        for (int t = T - 1, run = n_live[T]; t >= 0; --t) { const int ends = n_live[t]; n_live[t] = run; run += ends; }   // ... -> rows with L > t
        n_live.resize(T);
    }
    {
        long long rf = 0;
        if (L) for (int b = 0; b < ctx->B; ++b) rf += L[b]; else rf = (long long)ctx->B * T;
        ctx->seq->stat_row_frames += rf;
    }
    // Launch plan: with sequence mode on (and not live: the landmark refresh counter is not modelled on the host) one
    // pre-pass classifies every (frame, row), the host reads the codes back ONCE per call (the only synchronisation of
    // `stream` in this call) and picks, per frame, the wavefront engine, or the frame-stepped launches with or without
    // the three transition launches.
    std::vector<unsigned char> mode((size_t)(T > 0 ? T : 0), (unsigned char)SEQ_STEPPED_TR);
    const int B = ctx->B;
    WavePlan wplan;
    int wave2_from = -1;                    // first frame of the per-row-cursor segment (it runs to the end of the call)
    // (calls shorter than min_frames are not planned at all: no pre-pass, no synchronisation, fully asynchronous)
    const int w0 = ((flags & RC_FLAG_FIRST_FRAME) || first_tran) ? 1 : 0;   // a frame that takes first_frame / first_tran runs frame-stepped
    if (ctx->seq->seq_mode && !ctx->prm.live && T >= 2 && T - w0 >= std::max(1, ctx->seq->seq_min_frames)) {
        // ring, second stream and launch tables are set up by the first planned call (a warm-up call pays for them)
        if (int rc = ensure_wave2_buffers(ctx)) return rc;
        if (!ctx->seq->wave2_valid) if (int rc = build_wave2_problems(ctx)) return rc;
        const size_t need = (size_t)B * T;
        if (need > ctx->seq->scan_cap || !ctx->seq->scan_state_h) {
            HIP_TRY(ctx, hipStreamSynchronize(st));                             // nothing in flight may still read the old tables
            if (int rc = reserve_plan_tables(ctx, T)) return rc;
        }
        rc_launch_scan_conf(j2dc, rs_j2d, B, T, ctx->prm.conf_lo, ctx->prm.conf_hi, ctx->seq->scan_codes_d.get(), st, nullptr, len_d, off);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->seq->scan_codes_h.get(), ctx->seq->scan_codes_d.get(), need, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->seq->scan_state_h.get(), ctx->fb.first_reach, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
        unsigned char* pend_b = reinterpret_cast<unsigned char*>(ctx->seq->scan_state_h.get() + 2 * B);     // pinned, like the other two
        HIP_TRY(ctx, hipMemcpyAsync(pend_b, ctx->fb.pend, (size_t)B, hipMemcpyDeviceToHost, st));
        {   // a blocking wait wakes up tens of microseconds late: poll for a bounded while first (the stream may still hold
            // milliseconds of earlier frames, which a sleeping wait serves better)
            const auto t_spin = std::chrono::steady_clock::now();
            static const int spin = tune_env("RC_SEQ_SPIN", 1);
            while (spin && hipStreamQuery(st) == hipErrorNotReady &&
                   std::chrono::steady_clock::now() - t_spin < std::chrono::microseconds(300)) { }
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ctx->seq->res_abort_h && ctx->seq->res_abort_h[0]) {                           // (the copy sits behind the segment on this stream)
            ctx->seq->stat_resident_aborts += 1;
            ctx->seq->res_abort_h[0] = 0;
            return fail(ctx, RC_ERR_STATE, "resident layer-step kernel: a wait ran out in the previous call (its outputs and the recurrent state are invalid); "
                                           "RC_SEQ_RESIDENT=0 selects the stream engine");
        }
        for (int b = 0; b < B; ++b) ctx->seq->scan_state_h[B + b] = pend_b[b];
        const bool ff = (flags & RC_FLAG_FIRST_FRAME) != 0;
        const bool imu = ctx->prm.use_imu_updater != 0, vup = ctx->prm.use_vision_updater != 0;
        {
            // per-row-cursor engine on frames [w0, T): the rows' state in front of frame w0
            std::vector<int> fr(ctx->seq->scan_state_h.get(), ctx->seq->scan_state_h.get() + B), pd(ctx->seq->scan_state_h.get() + B, ctx->seq->scan_state_h.get() + 2 * B);
            if (w0) {
                for (int b = 0; b < B; ++b) {
                    if (L && L[b] < 1) continue;                                 // the row has no frame 0: its state stays
                    const int c = ctx->seq->scan_codes_h[b];
                    if (fr[b] && c == 2 && imu) fr[b] = 0;
                    pd[b] = (c == 0 && vup) ? 1 : 0;
                }
            }
            const double cost[4] = {ctx->seq->cost_tick_us, ctx->seq->cost_tick_small_us, ctx->seq->cost_frame_us, ctx->seq->cost_tr_us};
            plan_wave(ctx->seq->scan_codes_h.get(), B, T, w0, fr.data(), pd.data(), imu, vup, cost, wplan, L);
            if (ctx->seq->seq_mode == 2 || wplan.est_wave_us < wplan.est_stepped_us) wave2_from = w0;
            static const bool dbg = tune_env("RC_SEQ_DEBUG", 0) != 0;
            if (dbg) std::fprintf(stderr, "rc_sequence plan: T=%d ticks=%d lag_max=%d est_wave=%.0f us est_stepped=%.0f us -> %s\n", T, wplan.n_ticks,
                                  wplan.lag_max, wplan.est_wave_us, wplan.est_stepped_us, wave2_from >= 0 ? "wavefront" : "frame-stepped");
        }
        plan_sequence(ctx->seq->scan_codes_h.get(), B, T, ctx->seq->scan_state_h.get() + B, ff, vup, mode.data(), L);    // transition-launch marks of stepped frames
    }
    bool prep_done = false;                 // the previous frame's tail kernel already ran this frame's prep
    for (int t = 0; t < T;) {
        if (t == wave2_from) {
            FrameIO io0 = io_at(0);
            io0.first_tran = nullptr;
            if (int rc = run_wave2_segment(ctx, wplan, io0, t, T - 1, st)) return rc;
            t = T;
        } else {
            // consecutive frame-stepped frames: tail(t) and prep(t + 1) are back to back on the stream and per row, so
            // one wave does both (one launch boundary and the prep kernel's start-up latency less per frame)
            const bool chain = t + 1 < T && t + 1 != wave2_from;
            const FrameIO next = chain ? io_at(t + 1) : FrameIO{};
            if (int rc = step_impl(ctx, io_at(t), t == 0 ? flags : 0u, st, mode[t] == SEQ_STEPPED_TR, prep_done, chain ? &next : nullptr,
                                   L ? n_live[t] : -1)) return rc;
            prep_done = chain;
            ctx->seq->stat_stepped_frames += 1;
            ++t;
        }
    }
    return mark_eager(ctx, st);
}

int rc_sequence(rc_ctx* ctx, int32_t T, const float* j2dc, int64_t rs_j2d, const float* accc, int64_t rs_acc, const float* oric,
                int64_t rs_ori, const float* first_tran, uint32_t flags, float* pose_out, int64_t rs_pose, float* tran_out,
                int64_t rs_tran, void* stream) {
    if (int rc = check_ready(ctx)) return rc;
    if (T == 0) return RC_OK;                                               // (evaluate.py:75-83 over no frames: nothing happens, whatever the pointers)
    live_forget_last_frame(ctx);
    if (T < 0 || !j2dc || !accc || !oric || !pose_out || !tran_out) return fail(ctx, RC_ERR_INVALID, "rc_sequence: bad argument");
    return sequence_impl(ctx, T, nullptr, 0, j2dc, rs_j2d, accc, rs_acc, oric, rs_ori, first_tran, flags, pose_out, rs_pose, tran_out, rs_tran, stream);
}

int rc_sequence_rows(rc_ctx* ctx, int32_t T, const int32_t* len_host, const float* j2dc, int64_t rs_j2d, const float* accc, int64_t rs_acc,
                     const float* oric, int64_t rs_ori, const float* first_tran, uint32_t flags, float* pose_out, int64_t rs_pose,
                     float* tran_out, int64_t rs_tran, void* stream) {
    if (int rc = check_ready(ctx)) return rc;
    if (T < 0 || !len_host || !j2dc || !accc || !oric || !pose_out || !tran_out) return fail(ctx, RC_ERR_INVALID, "rc_sequence_rows: bad argument");
    const size_t B = (size_t)ctx->B;
    for (size_t b = 0; b < B; ++b)
        if (len_host[b] < 0 || len_host[b] > T) return fail(ctx, RC_ERR_INVALID, "rc_sequence_rows: a row's length is outside 0 .. T");
    if (T == 0) return RC_OK;
    live_forget_last_frame(ctx);
    hipStream_t st = (hipStream_t)stream;
    // the lengths travel once per call: pinned copy -> device copy on `stream`, in front of everything that reads them
    StagedTable<int, 2, 1>& row_len = ctx->seq->row_len;
    int* len_h = nullptr;
    HIP_TRY(ctx, row_len.stage(B, &len_h));                                        // (a copy's first call creates its event and has nothing to wait for)
    if (!row_len.holds(B)) HIP_TRY(ctx, row_len.grow(B));                          // the context's first call: no earlier one reads the table
    std::memcpy(len_h, len_host, B * sizeof(int));
    HIP_TRY(ctx, row_len.upload(B, st));
    HIP_TRY(ctx, row_len.record(st));
    return sequence_impl(ctx, T, len_h, 0, j2dc, rs_j2d, accc, rs_acc, oric, rs_ori, first_tran, flags, pose_out, rs_pose, tran_out, rs_tran, stream);
}

int rc_get_sequence_row_frames(rc_ctx* ctx, int64_t* body_frames) {
    if (!ctx || !body_frames) return RC_ERR_INVALID;
    *body_frames = ctx->seq->stat_row_frames;
    return RC_OK;
}

int rc_set_sequence_mode(rc_ctx* ctx, int32_t mode, int32_t min_frames) {
    if (!ctx || mode < 0 || mode > 2 || min_frames < 1) return ctx ? fail(ctx, RC_ERR_INVALID, "rc_set_sequence_mode: mode 0|1|2, min_frames >= 1") : RC_ERR_INVALID;
    ctx->seq->seq_mode = mode;
    ctx->seq->seq_min_frames = min_frames;
    return RC_OK;
}

int rc_get_sequence_stats(rc_ctx* ctx, int64_t* wave_frames, int64_t* stepped_frames, int64_t* ticks) {
    if (!ctx) return RC_ERR_INVALID;
    if (wave_frames) *wave_frames = ctx->seq->stat_wave_frames;
    if (stepped_frames) *stepped_frames = ctx->seq->stat_stepped_frames;
    if (ticks) *ticks = ctx->seq->stat_ticks;
    return RC_OK;
}

int rc_set_resident(rc_ctx* ctx, int32_t enable, int32_t workgroups) {
    if (!ctx) return RC_ERR_INVALID;
    ctx->seq->resident_on = enable != 0;
    if (workgroups > 0) ctx->seq->resident_wgs = workgroups;
    return RC_OK;
}

int rc_get_resident_stats(rc_ctx* ctx, int64_t* segments, int64_t* aborts) {
    if (!ctx) return RC_ERR_INVALID;
    if (segments) *segments = ctx->seq->stat_resident_segments;
    if (aborts) *aborts = ctx->seq->stat_resident_aborts;
    return RC_OK;
}

int rc_plan_sequence(const int8_t* codes, int32_t B, int32_t T, const int32_t* pend, uint32_t flags, int32_t use_vision_updater,
                     uint8_t* mode_out) {
    if (!codes || !pend || !mode_out || B < 1 || T < 0) return RC_ERR_INVALID;
    plan_sequence(reinterpret_cast<const signed char*>(codes), B, T, pend, (flags & RC_FLAG_FIRST_FRAME) != 0, use_vision_updater != 0, mode_out);
    return RC_OK;
}

static int plan_wave_abi(const int8_t* codes, int32_t B, int32_t T, int32_t t0, const int32_t* len, const int32_t* first_reach,
                         const int32_t* pend, int32_t use_imu_updater, int32_t use_vision_updater, int32_t* frame_at, int64_t frame_at_cap,
                         int32_t* n_ticks, int32_t* n_prep, int32_t* counts, double* est_us) {
    if (!codes || !first_reach || !pend || !n_ticks || !n_prep || B < 1 || T < 1 || t0 < 0 || t0 >= T) return RC_ERR_INVALID;
    WavePlan P;
    const double cost[4] = {1.0, 13.0, 285.0, 55.0};
    plan_wave(reinterpret_cast<const signed char*>(codes), B, T, t0, first_reach, pend, use_imu_updater != 0, use_vision_updater != 0, cost, P, len);
    *n_ticks = P.n_ticks;
    *n_prep = P.n_prep;
    if (est_us) { est_us[0] = P.est_wave_us; est_us[1] = P.est_stepped_us; }
    if (!frame_at || (int64_t)P.frame_at.size() > frame_at_cap) return RC_ERR_INVALID;
    std::memcpy(frame_at, P.frame_at.data(), P.frame_at.size() * sizeof(int));
    if (counts)
        for (int k = 0; k < P.n_prep; ++k) {
            counts[k] = P.n_valid[k]; counts[P.n_prep + k] = P.n_vis[k];
            counts[2 * P.n_prep + k] = P.n_rider[k]; counts[3 * P.n_prep + k] = P.n_reach[k];
        }
    return RC_OK;
}

int rc_plan_wave(const int8_t* codes, int32_t B, int32_t T, int32_t t0, const int32_t* first_reach, const int32_t* pend,
                 int32_t use_imu_updater, int32_t use_vision_updater, int32_t* frame_at, int64_t frame_at_cap, int32_t* n_ticks,
                 int32_t* n_prep, int32_t* counts, double* est_us) {
    return plan_wave_abi(codes, B, T, t0, nullptr, first_reach, pend, use_imu_updater, use_vision_updater, frame_at, frame_at_cap, n_ticks, n_prep,
                         counts, est_us);
}

int rc_plan_wave_rows(const int8_t* codes, int32_t B, int32_t T, int32_t t0, const int32_t* len, const int32_t* first_reach,
                      const int32_t* pend, int32_t use_imu_updater, int32_t use_vision_updater, int32_t* frame_at, int64_t frame_at_cap,
                      int32_t* n_ticks, int32_t* n_prep, int32_t* counts, double* est_us) {
    if (!len || B < 1) return RC_ERR_INVALID;
    for (int b = 0; b < B; ++b) if (len[b] < 0 || len[b] > T) return RC_ERR_INVALID;
    return plan_wave_abi(codes, B, T, t0, len, first_reach, pend, use_imu_updater, use_vision_updater, frame_at, frame_at_cap, n_ticks, n_prep,
                         counts, est_us);
}

}  // extern "C"
