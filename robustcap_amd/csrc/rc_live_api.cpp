// The live session of a context (rc_live_begin / rc_live_step / rc_live_end): one camera frame per call (live_server.py:40-48), on a private
// stream, from pinned staging buffers. Host logic only: the frame is the launch plan of rc_api.cpp (step_impl) captured twice -- with and
// without the transition launches -- and, for batch <= RC_LIVE_MAXB, the lean plan of rc_live.hip as a third capture and as pre-built AQL
// packets on a queue of the session's own (rc_aql.cpp). This is the only file that talks to that queue and to the mailboxes in
// host-writable device memory. Everything the session owns is a member of LiveSession, released in the reverse order of declaration.
#include "../../include/robustcap_hip.h"
#include "rc_ctx.h"

#if defined(__x86_64__) || defined(_M_X64)
#include <immintrin.h>
#define RC_STORE_FENCE() _mm_sfence()          // posted writes to the device's BAR leave the write-combining buffers in program order
#else
#define RC_STORE_FENCE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#endif

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

using LiveClock = std::chrono::steady_clock;
using AqlOwner = std::unique_ptr<AqlChain, RcRelease<rc_aql_destroy>>;   // (the release waits for a pre-step still in flight and tells a waiting K1 to leave)

// The frame's staging buffers. Inputs [j2dc B*99 | accc B*18 | oric B*54], outputs [pose B*216 | tran B*3], one pinned pair and one device pair.
// Small batches: the frame kernels read the 684 B / body of inputs and write the 876 B of outputs straight from / to the pinned host
// buffers (two copy nodes and their barriers cost more than the PCIe reads). Larger batches keep H2D -> frame -> D2H.
struct LiveIO {
    enum { kJ2d = 99, kAcc = 18, kOri = 54, kPose = 216, kTran = 3,
           kIn = 171, kOut = 219,                   // floats per row: kJ2d + kAcc + kOri, kPose + kTran
           kOffAcc = kJ2d, kOffOri = kJ2d + kAcc, kOffTran = kPose };
    static_assert(kIn == kJ2d + kAcc + kOri && kOut == kPose + kTran, "row layout");
    size_t B = 0;
    PinBuf<float> in_h, out_h;                      // pinned + mapped: [B, kIn] and [B, kOut]
    DevBuf<float> in_d, out_d, ft_d;                // ft_d: first_tran [B, 3]
    float *in_io = nullptr, *out_io = nullptr;      // what the frame kernels read / write (device copy or mapped host memory)
    bool zero_copy = false;

    FrameIO frame_io_at(const float* in, const float* first_tran = nullptr) const {      // inputs at `in` (a mailbox program's live in the chain's memory)
        return FrameIO{in, in + B * kOffAcc, in + B * kOffOri, first_tran, out_io, out_io + B * kOffTran, kJ2d, kAcc, kOri, kPose, kTran};
    }
    FrameIO frame_io(const float* first_tran) const { return frame_io_at(in_io, first_tran); }
    hipError_t stage_in(hipStream_t st) const {
        return zero_copy ? hipSuccess : hipMemcpyAsync(in_d.get(), in_h.get(), B * kIn * sizeof(float), hipMemcpyHostToDevice, st);
    }
    hipError_t stage_out(hipStream_t st) const {
        return zero_copy ? hipSuccess : hipMemcpyAsync(out_h.get(), out_d.get(), B * kOut * sizeof(float), hipMemcpyDeviceToHost, st);
    }
    // One frame as a graph: stage-in, body() (enqueues the frame on st; false = it failed and has said why), stage-out. The capture is always
    // ended: the stream must not stay in capture mode. Returns what failed (empty: exec is ready).
    template <class Body> std::string capture(hipStream_t st, Body body, HipGraph& graph, HipGraphExec& exec) const {
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return std::string("hipStreamBeginCapture: ") + hipGetErrorString(e);
        (void)stage_in(st);
        const bool ok = body();
        (void)stage_out(st);
        e = hipStreamEndCapture(st, rc_out(graph));
        if (!ok) return "the frame's launches failed";
        if (e != hipSuccess) return std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
        e = hipGraphInstantiate(rc_out(exec), graph.get(), nullptr, nullptr, 0);
        return e == hipSuccess ? std::string() : std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
    }
};

// The lean frame as pre-built AQL packets on a queue of its own (rc_aql.cpp), and everything that means something only while that chain
// exists: dropping the chain is assigning a fresh LivePackets.
struct LivePackets {
    AqlOwner chain;
    int prog_lean = -1, prog_lean_pre = -1, prog_pre = -1;            // programs of the chain: the frame, the frame on a pre-step's partial sums, the pre-step
    int prog_spin[2] = {-1, -1}, prog_spin_pre[2] = {-1, -1};         // the two frame programs once more per mailbox (frames queued ahead alternate between two)
    volatile unsigned* spin_mb = nullptr;                             // mailboxes, host-writable device memory of the chain's: [32 par] command, [32 par + 16] decision
    float* spin_in = nullptr;                                         // the frame's inputs, same allocation
    int spin_pending = -1;                                            // program whose first kernel is waiting
    int spin_pending_par = 0, spin_next_par = 0;                      // its mailbox / the next one's
    unsigned long long spin_pending_seq = 0;                          // its frame number on the chain
    bool spin_valid = false;                                          // nothing has touched weights / state since it was launched
};

// What rc_live_end carries over into the fresh session: the knobs (read once per context), the cumulative counters and profile sums, and the
// ordering between the eager entry points (caller's stream) and the live frames (private stream).
struct LiveKept {
    HipEvent eager_ev;
    bool eager_dirty = false;
    bool eager = false;                             // RC_LIVE_EAGER=1 (tuning): frames enqueued directly, no graph replay
    int lean = 1;                                   // RC_LIVE_LEAN: 0 = the frame-stepped plan for every live frame
    int lean_nc = 1;                                // RC_LIVE_LEAN_NC: 16-column blocks per LSTM tile (1 or 2)
    int aql_on = 1;                                 // RC_LIVE_AQL: 0 = lean frames by hipGraphLaunch only, 2 = also under a tool on the HSA queues
    // the idle-time pre-step (rc_live.hip: rc_live_pre): the recurrent halves of the next frame's layer steps, computed behind a frame
    // when the caller leaves the device idle between frames (a 60 fps stream: 16.6 ms)
    int prestep = 1;                                // RC_LIVE_PRESTEP: 0 = never
    double prestep_idle_us = 500.0;                 // RC_LIVE_PRESTEP_IDLE_US: idle time in front of a frame from which the next pre-step is enqueued
    bool arm = true;                                // RC_LIVE_ARM=0 switches it off: a paced caller leaves a barrier packet waiting at the head of the queue
    // RC_LIVE_SPIN: the first kernel of the NEXT lean frame is launched at the end of rc_live_step and waits on the device for the frame (rc_live.hip).
    // Opt-in since round 6: a paced caller's waiting kernel keeps ~84 workgroups polling between frames -- fine on a dedicated box, hostile on
    // a shared one. 1: behind frames of a paced caller, 2: behind every lean frame
    bool spin = false, spin_always = false;
    bool spin_b2b = true;                           // RC_LIVE_SPIN_B2B: a back-to-back caller's next frame is queued while this one runs, its K1 beside it
    bool blind = false;                             // RC_LIVE_MIRROR_BLIND=1 (tests): no host-side mirror of the transition / init_net flags
    long long stat_lean = 0, stat_full = 0;
    long long stat_replayed = 0;                    // lean frames whose own check (K1) found them off the lean plan: replayed on the full capture
    long long stat_pre = 0;
    long long stat_spin = 0, stat_spin_lost = 0;    // frames that started from a waiting K1 / waiting K1s sent away or timed out
    double prof_us[4] = {0.0, 0.0, 0.0, 0.0};       // host time of rc_live_step: staging + choice | enqueue | wait | copy out (sums, lean frames)
    long long prof_n = 0;
    double prof_last[6] = {0, 0, 0, 0, 0, 0};       // the same split of the most recent lean frame + {started from a waiting kernel, used a pre-step}
    std::string aql_note;                           // why the AQL path is not in use (empty when it is)
};

struct FrameCall;       // one rc_live_step call

// Members in the reverse of the order they must go in: the packet chain before the buffers its packets read, every graph exec before its
// graph, the stream last.
struct LiveSession : LiveKept {
    explicit LiveSession(LiveKept&& kept) : LiveKept(std::move(kept)) {}
    HipStream stream;
    HipGraph graph;                                 // the frame-stepped plan with the three transition launches ...
    HipGraphExec exec;
    HipGraph graph_notr;                            // ... and without them
    HipGraphExec exec_notr;
    HipGraph graph_lean;                            // the lean frame (rc_live.hip): seven launches for the steady-state frame of a small batch
    HipGraphExec exec_lean;
    LiveIO io;
    PinBuf<int> status_h;                           // pinned + mapped: set by a lean frame that met a transition step or an init_net trigger
    DevBuf<int> abort_d;                            // LiveFrame.abort
    DevBuf<float> pre_buf;                          // [tiles of the twelve layer steps][2 waves][64 lanes][4]
    PinBuf<unsigned> spin_state_h;                  // pinned + mapped, [4 par]: 3 = the waiting kernel gave up
    LiveFrame frame{};
    std::string lean_wide;                          // RC_LIVE_LEAN_NC=2: the 16 x 32-tile layer-step kernels of the captured lean plan, by name
    LivePackets aql;
    // nothing below owns anything
    std::vector<unsigned char> maybe_pend;          // host-side, conservative: row may carry a deferred updater step
    std::vector<unsigned char> may_reach;           // host-side, conservative: the row may still trigger init_net (L178-183)
    bool prev_known = false;                        // the two vectors describe the frame in front of the next one
    bool pre_valid = false;                         // a pre-step of the CURRENT state is in the queue (or done)
    bool have_return = false;
    LiveClock::time_point last_return{};

    void queue_ahead(bool with_pre, bool beside);
    int settle_queued_frame(rc_ctx* ctx, FrameCall& f);
    int run_aql_frame(rc_ctx* ctx, FrameCall& f);
    int run_frame(rc_ctx* ctx, FrameCall& f);
    int wait_frame(rc_ctx* ctx, const FrameCall& f);
    int replay_if_offplan(rc_ctx* ctx, const FrameCall& f);
    void after_frame(const FrameCall& f);
};

void rc_live_free(LiveSession* s) { delete s; }

void live_create(rc_ctx* ctx) {
    LiveKept k;
    (void)hipEventCreateWithFlags(rc_out(k.eager_ev), hipEventDisableTiming);      // (without it the live graph does not wait for eager work)
    k.eager = tune_env("RC_LIVE_EAGER", 0) != 0;
    k.lean = tune_env("RC_LIVE_LEAN", 1);
    k.lean_nc = tune_env("RC_LIVE_LEAN_NC", 1) == 2 ? 2 : 1;
    k.aql_on = tune_env("RC_LIVE_AQL", 1);
    k.prestep = tune_env("RC_LIVE_PRESTEP", 1);
    k.prestep_idle_us = (double)tune_env("RC_LIVE_PRESTEP_IDLE_US", 500);
    k.arm = tune_env("RC_LIVE_ARM", 1) != 0;
    k.spin = tune_env("RC_LIVE_SPIN", 0) != 0;
    k.spin_always = tune_env("RC_LIVE_SPIN", 0) >= 2;
    k.spin_b2b = tune_env("RC_LIVE_SPIN_B2B", 1) != 0;
    k.blind = tune_env("RC_LIVE_MIRROR_BLIND", 0) != 0;
    ctx->live.reset(new LiveSession(std::move(k)));
}

// The chain goes (its release waits for whatever is still in flight before the ring and the argument blocks go), and with it every program
// id, the mailboxes in its memory and the frame queued ahead; no pre-step is valid and the mirror forgets the last frame. The lean graph
// stays: frames replay it.
static void drop_chain(LiveSession& s, std::string note) {
    s.aql = LivePackets{};
    s.pre_valid = false;
    s.prev_known = false;
    s.aql_note = std::move(note);
}

void live_forget_last_frame(rc_ctx* ctx, bool rows_reset) {
    ctx->live->prev_known = false;
    if (rows_reset) ctx->live->may_reach.assign(ctx->B, 1);
}

// A frame queued ahead of its inputs (RC_LIVE_SPIN / the back-to-back queue-ahead: its first kernel polls a mailbox on the device) is sent
// away and waited for BEFORE anything else touches the context: its kernels change nothing once dismissed (LiveFrame.abort -- K4 skips
// its relu(linear1) store as well since round 6), but a kernel left polling would hold CUs through a long rc_sequence and leave 100 ms later.
static int dismiss_queued_frame(rc_ctx* ctx) {
    LiveSession& s = *ctx->live;
    LivePackets& a = s.aql;
    if (a.spin_pending < 0 || !a.chain || !a.spin_mb) return RC_OK;
    const int par = a.spin_pending_par;
    a.spin_mb[32 * par] = 2u;
    RC_STORE_FENCE();
    const int arc = rc_aql_wait_frame(a.chain.get());
    s.spin_state_h[4 * par] = 0;
    s.stat_spin_lost += 1;
    a.spin_pending = -1;
    return arc == 0 ? RC_OK : fail(ctx, RC_ERR_HIP, "the live frame queued ahead did not leave");
}

int live_discard_ahead(rc_ctx* ctx) {
    ctx->live->pre_valid = false;        // the state the pre-step read is no longer the state the next live frame starts from
    ctx->live->aql.spin_valid = false;
    return dismiss_queued_frame(ctx);
}

// Eager work was enqueued on the caller's stream `st`: the next live-graph replay (private stream) must wait for it.
// (The other direction needs nothing: rc_live_step synchronises its stream before it returns.)
int mark_eager(rc_ctx* ctx, hipStream_t st) {
    if (int rc = live_discard_ahead(ctx)) return rc;
    LiveSession& s = *ctx->live;
    if (!s.eager_ev) return RC_OK;
    HIP_TRY(ctx, hipEventRecord(s.eager_ev.get(), st));
    s.eager_dirty = true;
    return RC_OK;
}

bool live_session_open(const rc_ctx* ctx) { return (bool)ctx->live->exec; }

struct FrameCall {
    const float* first_tran;
    uint32_t flags;
    double idle_us;          // how long the caller left the device alone since the previous frame returned: a 60 fps stream idles 16.6 ms, a benchmark loop none
    bool waited_eager;       // the stream was ordered behind eager work on the caller's stream (e.g. reset_states() just before this frame)
    bool need_tr;
    bool lean;               // the frame takes the lean plan
    bool use_pre;            // ... on the partial sums of the pre-step behind the previous frame
    bool spin_go = false;    // ... from the first kernel that was waiting for it
    bool aql_done = false;   // it ran on the packet chain and has retired
};

// the next frame queued ahead (all seven packets; its first kernel waits on the device for the command word): mailbox and give-up mark cleared first
void LiveSession::queue_ahead(const bool with_pre, const bool beside) {
    const int par = aql.spin_next_par;
    const int prog = (with_pre && aql.prog_spin_pre[par] >= 0) ? aql.prog_spin_pre[par] : aql.prog_spin[par];
    aql.spin_mb[32 * par] = 0u; aql.spin_mb[32 * par + 16] = 0u;
    RC_STORE_FENCE();
    spin_state_h[4 * par] = 0;
    if (rc_aql_submit_ahead(aql.chain.get(), prog, beside ? 1 : 0) == 0) {
        aql.spin_pending = prog; aql.spin_pending_par = par; aql.spin_pending_seq = rc_aql_seq(aql.chain.get());
        aql.spin_next_par = par ^ 1; aql.spin_valid = true;
    }
}

// A first kernel launched ahead of this frame (RC_LIVE_SPIN) is waiting on the device: it takes the frame if the frame is what it was
// launched for (lean, same program, nothing touched weights or state since, and it has not given up); otherwise it is sent away.
int LiveSession::settle_queued_frame(rc_ctx* ctx, FrameCall& f) {
    if (aql.spin_pending < 0 || !aql.chain) return RC_OK;
    const int par = aql.spin_pending_par;
    const int want = f.use_pre ? aql.prog_spin_pre[par] : aql.prog_spin[par];
    const bool gone = __atomic_load_n(spin_state_h.get() + 4 * par, __ATOMIC_ACQUIRE) == 3u;
    f.spin_go = f.lean && !gone && aql.spin_valid && aql.spin_pending == want && !f.waited_eager;
    if (f.spin_go) {
        std::memcpy(aql.spin_in, io.in_h.get(), io.B * LiveIO::kIn * sizeof(float));
        RC_STORE_FENCE();
        aql.spin_mb[32 * par] = 1u;                                    // go: behind the inputs (stores to the device are posted in order; 0.1 us of host time)
        RC_STORE_FENCE();
        return RC_OK;
    }
    // skip: the kernel leaves and the six behind it change nothing (LiveFrame.abort); frames on this queue are ordered behind them, a
    // frame on the HIP stream waits for them here (a kernel that has given up is no longer there to read the word)
    aql.spin_mb[32 * par] = 2u;
    RC_STORE_FENCE();
    if (!f.lean && rc_aql_wait_frame(aql.chain.get()) != 0) return fail(ctx, RC_ERR_HIP, "rc_live_step: the frame queued ahead did not leave");
    spin_state_h[4 * par] = 0;
    stat_spin_lost += 1;
    aql.spin_pending = -1;
    return RC_OK;
}

// a lean frame on the packet chain: submitted (or released, if its first kernel was waiting) and waited for
int LiveSession::run_aql_frame(rc_ctx* ctx, FrameCall& f) {
    AqlChain* chain = aql.chain.get();
    if (f.waited_eager) HIP_TRY(ctx, hipStreamSynchronize(stream.get()));        // the AQL queue is not ordered behind the stream: wait here
    int arc = 0;
    const int plain = f.use_pre ? aql.prog_lean_pre : aql.prog_lean;
    const int my_par = aql.spin_pending_par;
    unsigned long long my_seq = aql.spin_pending_seq;
    if (f.spin_go) aql.spin_pending = -1;
    else { arc = rc_aql_submit_ahead(chain, plain, 0); my_seq = rc_aql_seq(chain); }
    // A back-to-back caller (no idle time in front of this call): the NEXT frame is queued now, its first kernel beside this frame's last ones --
    // when the caller comes back that kernel has its arguments and weights and is polling. (A paced caller's is queued behind the pre-step, after_frame.)
    if (arc == 0 && spin_b2b && aql.prog_spin[0] >= 0 && aql.spin_pending < 0 && f.idle_us < prestep_idle_us) queue_ahead(false, true);
    if (arc == 0) arc = rc_aql_wait_seq(chain, my_seq);
    if (f.spin_go && arc == 0 && __atomic_load_n(spin_state_h.get() + 4 * my_par, __ATOMIC_ACQUIRE) == 3u) {
        // the waiting kernel gave up in the very moment the frame arrived: the six kernels behind it have changed nothing
        // (LiveFrame.abort) -- the frame runs on the ordinary program, in front of which nothing may be waiting
        spin_state_h[4 * my_par] = 0;
        stat_spin_lost += 1;
        if (aql.spin_pending >= 0) { aql.spin_mb[32 * aql.spin_pending_par] = 2u; RC_STORE_FENCE(); aql.spin_pending = -1; stat_spin_lost += 1; }
        arc = rc_aql_run(chain, plain);
    } else if (f.spin_go && arc == 0) stat_spin += 1;
    if (arc != 0) {
        // The frame did not retire in time (a tool on the queue, a wedged device): the chain is dropped and the following frames replay the
        // captured graph of the same seven kernels. THIS frame's state is unknown: the caller gets the error.
        drop_chain(*this, "an AQL frame did not complete: back on hipGraphLaunch");
        return fail(ctx, RC_ERR_HIP, "rc_live_step: the AQL frame did not complete (later frames use the graph replay)");
    }
    f.aql_done = true;
    return RC_OK;
}

// the frame is enqueued: sequence start | lean | frame-stepped, directly | frame-stepped, one of the two captures
int LiveSession::run_frame(rc_ctx* ctx, FrameCall& f) {
    hipStream_t st = stream.get();
    if (!(f.lean && aql.chain) && aql.chain) {
        // this frame runs on the HIP stream: a pre-step still in the HSA queue must not read the state while the frame rewrites it
        if (rc_aql_wait_background(aql.chain.get()) != 0) return fail(ctx, RC_ERR_HIP, "rc_live_step: the pre-step did not complete");
    }
    if (f.first_tran || (f.flags & RC_FLAG_FIRST_FRAME)) {           // sequence start: ordinary enqueue path
        HIP_TRY(ctx, io.stage_in(st));
        if (f.first_tran) HIP_TRY(ctx, hipMemcpyAsync(io.ft_d.get(), f.first_tran, io.B * LiveIO::kTran * sizeof(float), hipMemcpyHostToDevice, st));
        if (int rc = step_impl(ctx, io.frame_io(f.first_tran ? io.ft_d.get() : nullptr), f.flags, st)) return rc;
        HIP_TRY(ctx, io.stage_out(st));
    } else if (f.lean) {
        if (aql.chain) { if (int rc = run_aql_frame(ctx, f)) return rc; }
        else if (eager) rc_launch_live_frame(frame, st);
        else HIP_TRY(ctx, hipGraphLaunch(exec_lean.get(), st));
        stat_lean += 1;
    } else if (eager) {                                              // tuning (RC_LIVE_EAGER=1): the 11-14 launches enqueued directly
        HIP_TRY(ctx, io.stage_in(st));
        if (int rc = step_impl(ctx, io.frame_io(nullptr), 0u, st, f.need_tr)) return rc;
        HIP_TRY(ctx, io.stage_out(st));
    } else {
        HIP_TRY(ctx, hipGraphLaunch(f.need_tr ? exec.get() : exec_notr.get(), st));
    }
    return RC_OK;
}

// A frame is ~100 us of GPU work: poll for its completion instead of sleeping on the stream (the blocking wait's wake-up
// costs a sizeable fraction of that); after ~2 ms fall back to the blocking call.
int LiveSession::wait_frame(rc_ctx* ctx, const FrameCall& f) {
    if (f.aql_done) return RC_OK;
    hipStream_t st = stream.get();
    const auto t_spin = LiveClock::now();
    hipError_t q;
    while ((q = hipStreamQuery(st)) == hipErrorNotReady) {
        if (LiveClock::now() - t_spin > std::chrono::milliseconds(2)) break;
    }
    if (q != hipSuccess && q != hipErrorNotReady) return fail(ctx, RC_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
    (void)hipGetLastError();
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return RC_OK;
}

// The lean plan's own check (rc_live_k1) found the frame off the plan -- a transition step or an init_net trigger the host-side
// mirror did not foresee. Its kernels have changed nothing (LiveFrame.abort): the frame runs again on the full capture,
// from the inputs still staged in the pinned buffer.
int LiveSession::replay_if_offplan(rc_ctx* ctx, const FrameCall& f) {
    if (!f.lean) stat_full += 1;
    if (!(f.lean && status_h[0] != 0)) return RC_OK;
    status_h[0] = 0;
    stat_lean -= 1;
    stat_full += 1;
    stat_replayed += 1;
    HIP_TRY(ctx, hipGraphLaunch(exec.get(), stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(stream.get()));
    return RC_OK;
}

// The pre-step of the NEXT frame, behind this one in the queue, when the caller paces its frames (the idle time in front of this call
// says so): it streams half of the weights while the device would otherwise idle, and a caller that comes back at once -- a
// throughput loop -- would only wait for it. Then the next frame queued ahead (RC_LIVE_SPIN), or the arm packet.
void LiveSession::after_frame(const FrameCall& f) {
    AqlChain* chain = aql.chain.get();
    if (chain && aql.prog_pre >= 0 && f.idle_us >= prestep_idle_us) {
        if (rc_aql_submit(chain, aql.prog_pre) == 0) { pre_valid = true; stat_pre += 1; }
    }
    if (chain && spin && aql.prog_spin[0] >= 0 && aql.spin_pending < 0 && f.lean && f.idle_us < 50000.0 && (spin_always || f.idle_us >= prestep_idle_us)) {
        queue_ahead(pre_valid, false);                                  // (RC_LIVE_SPIN) behind this frame and its pre-step
    } else if (chain && arm && aql.spin_pending < 0 && f.idle_us >= prestep_idle_us) (void)rc_aql_arm(chain);
}

#pragma GCC visibility pop

// Begin-time self-check of the AQL packet chain (round-4/5 review): ONE lean frame on a fixed synthetic input, once as the graph replay
// of the captured launches and once as the pre-built packets on the context's own HSA queue, from the same state -- every small device
// buffer of the context (recurrent state, fusion state, scratch; weights excluded) is saved first and put back after each run, so the
// check leaves no trace. Outputs must agree bit for bit (same kernels, same arguments); if they do not, or the chain does not retire, the
// chain is dropped and live frames replay the graph (rc_get_live_backend tells). RC_LIVE_AQL_SELFCHECK=0 skips it, =2 forces the
// mismatch path (tests/test_gpu_live.py). live_server.py:40-48 is the loop this protects.
std::string live_selfcheck(rc_ctx* ctx) {
    static const int mode = std::getenv("RC_LIVE_AQL_SELFCHECK") ? std::atoi(std::getenv("RC_LIVE_AQL_SELFCHECK")) : 1;
    LiveSession& s = *ctx->live;
    if (mode == 0 || !s.aql.chain || s.aql.prog_lean < 0 || !s.exec_lean || !s.io.zero_copy) return std::string();
    const size_t B = ctx->B, n_in = B * LiveIO::kIn, n_out = B * LiveIO::kOut;
    float *in_h = s.io.in_h.get(), *out_h = s.io.out_h.get();
    hipStream_t st = s.stream.get();
    if (hipDeviceSynchronize() != hipSuccess) return "self-check: device synchronisation failed";
    // save
    const size_t kMaxBytes = 8u << 20;
    std::vector<std::pair<void*, size_t>> regs;
    size_t total = 0;
    for (const auto& r : ctx->alloc_bytes) if (r.second <= kMaxBytes) { regs.push_back(r); total += r.second; }
    std::vector<char> save(total);
    size_t off = 0;
    for (const auto& r : regs) { if (hipMemcpy(save.data() + off, r.first, r.second, hipMemcpyDeviceToHost) != hipSuccess) return "self-check: state read-back failed"; off += r.second; }
    auto restore = [&]() -> bool {
        size_t o = 0;
        for (const auto& r : regs) { if (hipMemcpy(r.first, save.data() + o, r.second, hipMemcpyHostToDevice) != hipSuccess) return false; o += r.second; }
        s.status_h[0] = 0;
        return hipDeviceSynchronize() == hipSuccess;
    };
    // a mid-confidence frame (no init_net trigger, no deferred updater step): identity orientations, small accelerations, a plausible skeleton
    std::vector<float> in_keep(in_h, in_h + n_in), out_keep(out_h, out_h + n_out);
    for (size_t b = 0; b < B; ++b) {
        float* j = in_h + b * LiveIO::kJ2d;
        for (int k = 0; k < 33; ++k) { j[3 * k] = 0.05f * (float)((k * 7) % 11 - 5) / 5.0f; j[3 * k + 1] = 0.08f * (float)((k * 5) % 13 - 6) / 6.0f; j[3 * k + 2] = 0.75f; }
        float* a = in_h + B * LiveIO::kOffAcc + b * LiveIO::kAcc;
        for (int k = 0; k < LiveIO::kAcc; ++k) a[k] = 0.01f * (float)(k % 5 - 2);
        float* o = in_h + B * LiveIO::kOffOri + b * LiveIO::kOri;
        for (int k = 0; k < LiveIO::kOri; ++k) o[k] = (k % 9 == 0 || k % 9 == 4 || k % 9 == 8) ? 1.0f : 0.0f;
    }
    std::string verdict;
    std::vector<float> out_graph(n_out), out_aql(n_out);
    int status_graph = 0, status_aql = 0;
    for (size_t q = 0; q < n_out; ++q) out_h[q] = -7.0f;
    if (hipGraphLaunch(s.exec_lean.get(), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) verdict = "self-check: graph replay of the lean frame failed";
    status_graph = s.status_h[0];
    std::copy(out_h, out_h + n_out, out_graph.begin());
    if (!restore() && verdict.empty()) verdict = "self-check: state restore failed";
    if (verdict.empty()) {
        for (size_t q = 0; q < n_out; ++q) out_h[q] = -7.0f;
        if (rc_aql_run(s.aql.chain.get(), s.aql.prog_lean) != 0) verdict = "self-check: the packet chain did not retire";
        status_aql = s.status_h[0];
        std::copy(out_h, out_h + n_out, out_aql.begin());
        if (mode == 2) { uint32_t u; std::memcpy(&u, &out_aql[0], 4); u ^= 1u; std::memcpy(&out_aql[0], &u, 4); }      // forced mismatch (test hook)
        if (!restore() && verdict.empty()) verdict = "self-check: state restore failed";
    }
    std::copy(in_keep.begin(), in_keep.end(), in_h);
    std::copy(out_keep.begin(), out_keep.end(), out_h);
    if (verdict.empty() && (status_graph != status_aql || std::memcmp(out_graph.data(), out_aql.data(), n_out * sizeof(float)) != 0)) {
        verdict = "self-check: packet chain and graph replay disagree on the probe frame";
    }
    return verdict;
}

// ------------------------------------------------------------------------------------------ rc_live_begin
namespace {

int allocate_and_map(rc_ctx* ctx, LiveSession& s) {
    LiveIO& io = s.io;
    const size_t B = io.B = ctx->B;
    HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(s.stream), hipStreamNonBlocking));
    HIP_TRY(ctx, rc_alloc(io.in_h, B * LiveIO::kIn, hipHostMallocMapped));
    HIP_TRY(ctx, rc_alloc(io.out_h, B * LiveIO::kOut, hipHostMallocMapped));
    HIP_TRY(ctx, rc_alloc_all(io.in_d, B * LiveIO::kIn, io.out_d, B * LiveIO::kOut, io.ft_d, B * LiveIO::kTran));
    io.zero_copy = B <= 16;
    io.in_io = io.in_d.get();
    io.out_io = io.out_d.get();
    if (io.zero_copy) {
        HIP_TRY(ctx, hipHostGetDevicePointer((void**)&io.in_io, io.in_h.get(), 0));
        HIP_TRY(ctx, hipHostGetDevicePointer((void**)&io.out_io, io.out_h.get(), 0));
    }
    return RC_OK;
}

// One capture of the frame-stepped plan, with or without the three transition launches. rc_live_step replays the short one
// when the host can rule out that any row carries a deferred updater step into a frame it steps on camera data.
int capture_full(rc_ctx* ctx, LiveSession& s, bool with_tr, HipGraph& graph, HipGraphExec& exec) {
    hipStream_t st = s.stream.get();
    int rc = RC_OK;
    const std::string what = s.io.capture(st, [&] {
        LiveLaunchScope live_frame(ctx);
        rc = step_impl(ctx, s.io.frame_io(nullptr), 0u, st, with_tr);
        return rc == RC_OK;
    }, graph, exec);
    if (rc) return rc;                                                 // (step_impl has recorded its message)
    return what.empty() ? RC_OK : fail(ctx, RC_ERR_HIP, what);
}

// The lean plan of the steady-state frame (rc_live.hip): seven launches. rc_live_step replays it when the frame needs neither a
// transition step nor init_net and is not a sequence start; every other frame takes the full captures.
// Returns why the lean frame is not available (empty: it is captured, `plan` holds its seven launches).
std::string setup_lean(rc_ctx* ctx, LiveSession& s, std::vector<LiveKernel>& plan) {
    if (rc_alloc(s.status_h, 1, hipHostMallocMapped) != hipSuccess) return "lean frame: status word allocation failed";
    s.status_h[0] = 0;
    if (rc_alloc(s.abort_d, 16) != hipSuccess || hipMemset(s.abort_d.get(), 0, 64) != hipSuccess) return "lean frame: abort word allocation failed";
    LiveFrame& F = s.frame;
    F = LiveFrame{};
    for (int i = 0; i < 6; ++i) {
        const NetDev& n = ctx->net[i];
        LiveNet& l = F.net[i];
        l.W1 = n.lin1.W; l.b1 = n.lin1.b;
        for (int q = 0; q < 2; ++q) { l.Wl[q] = n.Wl[q]; l.bl[q] = n.bl[q]; }
        l.W2 = n.lin2.Wrm; l.b2 = n.lin2.b;
        l.x1 = n.x1; l.h = n.h; l.c = n.c; l.part = n.part; l.steps = n.steps;
        l.H = n.H; l.out = n.out; l.outp = round_up(n.out, 4); l.Kp1 = n.lin1.Kp;
        l.BpH = (long long)ctx->Bp * n.H;
    }
    F.fb = ctx->fb; F.io = s.io.frame_io(nullptr); F.prm = dev_params(ctx->prm); F.body = ctx->body; F.B = ctx->B; F.nc = s.lean_nc;
    if (hipHostGetDevicePointer((void**)&F.status, s.status_h.get(), 0) != hipSuccess) return "lean frame: status word not mapped";
    F.abort = s.abort_d.get();
    if (rc_live_plan(F, plan.data()) != RC_LIVE_KERNELS) return "lean frame: sub-net sizes these kernels are not compiled for";
    if (F.nc == 2) {                                                   // (what the plan holds, not what the switch asked for: rc_get_live_backend tells)
        s.lean_wide = "lean LSTM tiles 16 x 32:";
        for (int i : {1, 2, 4, 5}) s.lean_wide += std::string(" ") + plan[i].name;
    }
    hipStream_t st = s.stream.get();
    const std::string what = s.io.capture(st, [&] { rc_launch_live_frame(F, st); return true; }, s.graph_lean, s.exec_lean);
    return what.empty() ? what : "lean frame: " + what;
}

// The pre-step and the frame that starts from its partial sums: two more programs on the same queue; without them (an allocation or a
// symbol failed) the chain simply keeps the one frame program.
void add_prestep_programs(LiveSession& s) {
    LivePackets& a = s.aql;
    const LiveFrame& F = s.frame;
    const size_t nf = (size_t)rc_live_pre_floats(F);
    if (rc_alloc(s.pre_buf, nf) != hipSuccess || hipMemset(s.pre_buf.get(), 0, nf * sizeof(float)) != hipSuccess) {
        s.pre_buf.reset(); (void)hipGetLastError();
        return;
    }
    std::vector<LiveKernel> plan2(RC_LIVE_KERNELS), plan3(2);
    const int n3 = rc_live_pre_plan(F, s.pre_buf.get(), plan3.data());
    if (rc_live_plan(F, plan2.data(), s.pre_buf.get()) != RC_LIVE_KERNELS || n3 < 1) return;
    a.prog_lean_pre = rc_aql_add(a.chain.get(), plan2.data(), RC_LIVE_KERNELS, 1, nullptr, 0);
    if (a.prog_lean_pre >= 0) a.prog_pre = rc_aql_add(a.chain.get(), plan3.data(), n3, 0, nullptr, 0);
    if (a.prog_pre < 0) a.prog_lean_pre = -1;
}

// RC_LIVE_SPIN / the back-to-back queue-ahead: the frame programs once more with the inputs and a mailbox in host-writable device memory;
// their first kernel is launched ahead of the frame and waits there (rc_live_k1).
void add_mailbox_programs(LiveSession& s) {
    LivePackets& a = s.aql;
    void* shared = nullptr;
    unsigned* state_d = nullptr;
    if (rc_aql_alloc_shared(a.chain.get(), 4096 + s.io.B * LiveIO::kIn * sizeof(float), &shared) != 0 ||
        rc_alloc(s.spin_state_h, 16, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&state_d, s.spin_state_h.get(), 0) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    for (int q = 0; q < 16; ++q) s.spin_state_h[q] = 0;
    a.spin_mb = (volatile unsigned*)shared;
    a.spin_in = (float*)((char*)shared + 4096);
    for (int q = 0; q < 64; ++q) a.spin_mb[q] = 0u;
    LiveFrame Fs = s.frame;
    Fs.io = s.io.frame_io_at(a.spin_in);
    std::vector<LiveKernel> ps(RC_LIVE_KERNELS);
    bool ok = true;
    for (int par = 0; par < 2 && ok; ++par) {                   // two mailboxes (and give-up marks): the next frame is queued while this one may still be read
        Fs.spin_mb = (unsigned*)shared + 32 * par; Fs.spin_state = state_d + 4 * par;
        if (rc_live_plan(Fs, ps.data()) == RC_LIVE_KERNELS) a.prog_spin[par] = rc_aql_add(a.chain.get(), ps.data(), RC_LIVE_KERNELS, 1, nullptr, 0);
        ok = a.prog_spin[par] >= 0;
        if (ok && a.prog_lean_pre >= 0 && rc_live_plan(Fs, ps.data(), s.pre_buf.get()) == RC_LIVE_KERNELS)
            a.prog_spin_pre[par] = rc_aql_add(a.chain.get(), ps.data(), RC_LIVE_KERNELS, 1, nullptr, 0);
    }
    if (!ok) a.prog_spin[0] = a.prog_spin[1] = -1;
    if (a.prog_spin_pre[0] < 0 || a.prog_spin_pre[1] < 0) a.prog_spin_pre[0] = a.prog_spin_pre[1] = -1;
    if (ok) rc_aql_set_mailbox(a.chain.get(), a.spin_mb);
    else { a.spin_mb = nullptr; a.spin_in = nullptr; (void)hipGetLastError(); }
}

// ... and the same seven dispatches as pre-built AQL packets (rc_aql.cpp); without them the lean graph is replayed, and the note says why.
// Not under a tool that intercepts the HSA queues (rocprofv3's interception crashes on packets written straight into the ring --
// ROCm 7.2; traces then show the graph replay of the same kernels; a debugger's or tracer's runtime hooks are treated alike).
// RC_LIVE_AQL=2 insists.
void setup_chain(rc_ctx* ctx, LiveSession& s, const std::vector<LiveKernel>& plan) {
    const char* preload = std::getenv("LD_PRELOAD");
    bool tool = std::getenv("ROCP_TOOL_LIBRARIES") || std::getenv("HSA_TOOLS_LIB") || std::getenv("ROCPROFILER_REGISTER_FORCE_LOAD") ||
                std::getenv("ROCR_DEBUG_AGENT") || std::getenv("HSA_ENABLE_DEBUG");
    for (const char* sub : {"rocprof", "roctracer", "rocm-debug", "rocgdb", "omnitrace", "rocprofiler"}) tool = tool || (preload && std::strstr(preload, sub));
    if (tool && s.aql_on == 1) { s.aql_note = "a profiling / debugging tool intercepts the HSA queues"; return; }
    if (!(s.aql_on && s.io.zero_copy && !s.eager)) { s.aql_note = "switched off"; return; }
    LivePackets& a = s.aql;
    char msg[256] = {0};
    AqlChain* chain = nullptr;
    if (rc_aql_create(ctx->dev, &chain, msg, (int)sizeof(msg)) != 0) { s.aql_note = msg; return; }
    a.chain.reset(chain);
    if ((a.prog_lean = rc_aql_add(a.chain.get(), plan.data(), (int)plan.size(), 1, msg, (int)sizeof(msg))) < 0) { drop_chain(s, msg); return; }
}

// ------------------------------------------------------------------------------------------ rc_live_step
// Host-side, CONSERVATIVE mirror of two device flags (rc_prep_kernel): a row needs a transition step iff it carries
// a deferred updater step (previous frame had c <= lo) and steps on camera data now (c > lo or first frame). The
// margin covers the difference between this double mean and the device's float32 mean in the reference's order
// (rc_conf_mean33); any doubt selects the full graph, where unneeded transition tiles simply exit.
struct Mirror {
    bool need_tr;            // some row may need a transition step in this frame
    bool maybe_reach;        // some row may trigger init_net in this frame (c >= hi on a row that has not yet, L178-183)
};
Mirror mirror_flags(const float* j2dc, uint32_t flags, const rc_params& prm, std::vector<unsigned char>& maybe_pend, std::vector<unsigned char>& may_reach) {
    Mirror m{false, false};
    const double lo = prm.conf_lo, hi = prm.conf_hi, margin = 1e-4;
    const size_t B = maybe_pend.size();
    if (may_reach.size() != B) may_reach.assign(B, 1);
    for (size_t b = 0; b < B; ++b) {
        double acc = 0.0;
        for (int k = 0; k < 33; ++k) acc += (double)j2dc[(b * 33 + k) * 3 + 2];
        const double c = acc / 33.0;
        const bool maybe_vis = !(c < lo - margin) || (flags & RC_FLAG_FIRST_FRAME);
        if (maybe_pend[b] && maybe_vis) m.need_tr = true;
        maybe_pend[b] = (prm.use_vision_updater && !(c > lo + margin)) ? 1 : 0;
        if (prm.use_imu_updater && may_reach[b]) {
            if (!(c < hi - margin)) m.maybe_reach = true;
            if (c > hi + margin) may_reach[b] = 0;          // it fires in this frame at the latest (frames like this one never take the lean plan)
        }
    }
    return m;
}

}  // namespace

extern "C" {

// Everything the session owns goes with it, the packet chain first (LiveSession); the knobs, the counters and the order behind eager work stay.
int rc_live_end(rc_ctx* ctx) {
    if (!ctx) return RC_ERR_INVALID;
    ctx->live.reset(new LiveSession(std::move(static_cast<LiveKept&>(*ctx->live))));
    return RC_OK;
}

int rc_live_begin(rc_ctx* ctx) {
    if (int rc = check_ready(ctx)) return rc;
    rc_live_end(ctx);
    LiveSession& s = *ctx->live;
    s.maybe_pend.assign(ctx->B, 1);
    s.may_reach.assign(ctx->B, 1);
    if (int rc = allocate_and_map(ctx, s)) return rc;
    TimingSuspended untimed(ctx);                                      // (no captured launch carries a timing pair; restored on every exit path)
    if (int rc = capture_full(ctx, s, true, s.graph, s.exec)) return rc;
    if (int rc = capture_full(ctx, s, false, s.graph_notr, s.exec_notr)) return rc;
    // (fp32-MFMA contexts only: the lean kernels stream the fp32 weights, a context switched to split products keeps one arithmetic)
    // The lean plan is an OPTION on top of the two captures above: whatever fails in here (an allocation, its capture, the AQL chain) leaves
    // the context on those captures with a note (rc_get_live_backend), and never fails rc_live_begin (round-4 advice).
    if (!(s.lean && s.io.B <= RC_LIVE_MAXB && !gemm_split(ctx))) return RC_OK;
    s.aql_note.clear();
    std::vector<LiveKernel> plan(RC_LIVE_KERNELS);
    const std::string why = setup_lean(ctx, s, plan);
    if (!why.empty()) {                                                // back to the two full captures
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s.stream.get(), &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) { HipGraph g; (void)hipStreamEndCapture(s.stream.get(), rc_out(g)); }
        (void)hipGetLastError();
        s.exec_lean.reset(); s.graph_lean.reset();
        s.lean_wide.clear();
        s.aql_note = why;
        return RC_OK;
    }
    setup_chain(ctx, s, plan);
    if (!s.aql.chain) return RC_OK;
    if (s.prestep && s.frame.nc == 1) add_prestep_programs(s);
    if ((s.spin || s.spin_b2b) && RC_LIVE_KERNELS * 6 + 8 <= 64) add_mailbox_programs(s);
    const std::string bad = live_selfcheck(ctx);
    if (!bad.empty()) drop_chain(s, bad);                              // the lean graph stays: frames replay it
    return RC_OK;
}

int rc_live_step(rc_ctx* ctx, const float* j2dc, const float* accc, const float* oric, const float* first_tran, uint32_t flags,
                 float* pose, float* tran) {
    if (!ctx || !ctx->live->exec) return ctx ? fail(ctx, RC_ERR_STATE, "rc_live_step: call rc_live_begin first") : RC_ERR_INVALID;
    if (!j2dc || !accc || !oric || !pose || !tran) return fail(ctx, RC_ERR_INVALID, "rc_live_step: null buffer");
    LiveSession& s = *ctx->live;
    const size_t B = s.io.B;
    const auto t_in = LiveClock::now();
    FrameCall f{first_tran, flags, s.have_return ? std::chrono::duration<double, std::micro>(t_in - s.last_return).count() : 0.0, false, false, false, false};
    if (s.eager_dirty) {
        HIP_TRY(ctx, hipStreamWaitEvent(s.stream.get(), s.eager_ev.get(), 0));
        s.eager_dirty = false;
        f.waited_eager = true;
    }
    float* in_h = s.io.in_h.get();
    std::memcpy(in_h, j2dc, B * LiveIO::kJ2d * sizeof(float));
    std::memcpy(in_h + B * LiveIO::kOffAcc, accc, B * LiveIO::kAcc * sizeof(float));
    std::memcpy(in_h + B * LiveIO::kOffOri, oric, B * LiveIO::kOri * sizeof(float));
    Mirror m = mirror_flags(j2dc, flags, ctx->prm, s.maybe_pend, s.may_reach);
    if (!s.prev_known) m.need_tr = true;                               // an unknown previous frame selects the full graph
    s.prev_known = true;
    if (s.blind) m = Mirror{false, false};                             // tests: every frame is offered to the lean plan, whose own check decides
    f.need_tr = m.need_tr;
    f.lean = s.exec_lean && !m.need_tr && !m.maybe_reach && !first_tran && !(flags & RC_FLAG_FIRST_FRAME);
    const auto t_staged = LiveClock::now();
    f.use_pre = f.lean && s.aql.chain && s.pre_valid && s.aql.prog_lean_pre >= 0;
    s.pre_valid = false;                                               // (whatever this frame is, it moves the state on)
    if (int rc = s.settle_queued_frame(ctx, f)) return rc;
    if (int rc = s.run_frame(ctx, f)) return rc;
    const auto t_enq = LiveClock::now();
    if (int rc = s.wait_frame(ctx, f)) return rc;
    if (int rc = s.replay_if_offplan(ctx, f)) return rc;
    const auto t_done = LiveClock::now();
    std::memcpy(pose, s.io.out_h.get(), B * LiveIO::kPose * sizeof(float));
    std::memcpy(tran, s.io.out_h.get() + B * LiveIO::kOffTran, B * LiveIO::kTran * sizeof(float));
    s.after_frame(f);
    if (f.lean) {
        const auto us = [](LiveClock::time_point a, LiveClock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        const double split[6] = {us(t_in, t_staged), us(t_staged, t_enq), us(t_enq, t_done), us(t_done, LiveClock::now()), f.spin_go ? 1.0 : 0.0, f.use_pre ? 1.0 : 0.0};
        for (int q = 0; q < 4; ++q) s.prof_us[q] += split[q];
        for (int q = 0; q < 6; ++q) s.prof_last[q] = split[q];
        s.prof_n += 1;
    }
    s.last_return = LiveClock::now();
    s.have_return = true;
    return RC_OK;
}

int rc_get_live_backend(rc_ctx* ctx, int32_t* lean_captured, int32_t* aql, char* note, int32_t note_len) {
    if (!ctx) return RC_ERR_INVALID;
    if (lean_captured) *lean_captured = ctx->live->exec_lean ? 1 : 0;
    if (aql) *aql = ctx->live->aql.chain ? 1 : 0;
    // (the default plan of 16 x 16 tiles adds nothing: an empty note still means "the packet chain is in use")
    const LiveSession& s = *ctx->live;
    if (note && note_len > 0) std::snprintf(note, (size_t)note_len, "%s%s%s", s.aql_note.c_str(), (!s.aql_note.empty() && !s.lean_wide.empty()) ? "; " : "", s.lean_wide.c_str());
    return RC_OK;
}

int rc_get_live_prestep(rc_ctx* ctx, int64_t* presteps, int32_t* available) {
    if (!ctx) return RC_ERR_INVALID;
    if (presteps) *presteps = ctx->live->stat_pre;
    if (available) *available = (ctx->live->aql.chain && ctx->live->aql.prog_pre >= 0) ? 1 : 0;
    return RC_OK;
}

int rc_get_live_spin(rc_ctx* ctx, int64_t* taken, int64_t* lost) {
    if (!ctx) return RC_ERR_INVALID;
    if (taken) *taken = ctx->live->stat_spin;
    if (lost) *lost = ctx->live->stat_spin_lost;
    return RC_OK;
}

int rc_get_live_replayed(rc_ctx* ctx, int64_t* frames) {
    if (!ctx || !frames) return RC_ERR_INVALID;
    *frames = ctx->live->stat_replayed;
    return RC_OK;
}

int rc_get_live_last_profile(rc_ctx* ctx, double* us6) {
    if (!ctx || !us6) return RC_ERR_INVALID;
    for (int q = 0; q < 6; ++q) us6[q] = ctx->live->prof_last[q];
    return RC_OK;
}
int rc_get_live_profile(rc_ctx* ctx, double* avg_us4) {
    if (!ctx || !avg_us4) return RC_ERR_INVALID;
    for (int q = 0; q < 4; ++q) avg_us4[q] = ctx->live->prof_n ? ctx->live->prof_us[q] / (double)ctx->live->prof_n : 0.0;
    return RC_OK;
}

int rc_get_live_stats(rc_ctx* ctx, int64_t* lean_frames, int64_t* full_frames) {
    if (!ctx) return RC_ERR_INVALID;
    if (lean_frames) *lean_frames = ctx->live->stat_lean;
    if (full_frames) *full_frames = ctx->live->stat_full;
    return RC_OK;
}

}  // extern "C"
