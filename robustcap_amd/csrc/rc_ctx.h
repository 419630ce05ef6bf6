// The context behind the C ABI, for the files that work on all of it: rc_api.cpp (context, weights, frame-stepped plan, op wrappers),
// rc_gemm_api.cpp (problem builders, gate-GEMM launcher), rc_sequence_api.cpp (the sequence engine), rc_live_api.cpp (the live session)
// rc_prepare_api.cpp (the shape space and the motion preparation) and rc_rowstate_api.cpp (row state: save, load, rc_set_state).
// (rc_smplify_api.cpp and rc_subnet_api.cpp see it through the rc_ctx_* accessors of rc_internal.h.)
#pragma once
#include "../../include/robustcap_hip.h"
#include "rc_internal.h"

#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

struct NetSpec { const char* name; int in, H, out; };
const NetSpec kNets[6] = {{"rnn2", 72, 512, 69},  {"rnn3", 141, 512, 3},   {"rnn4", 171, 1280, 69},
                          {"rnn6", 240, 1024, 3}, {"rnn7", 141, 512, 144}, {"rnn8", 141, 512, 2}};
enum { N2 = 0, N3 = 1, N4 = 2, N6 = 3, N7 = 4, N8 = 5 };

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct Dense {       // packed dense layer
    float* W = nullptr; float* b = nullptr;
    void* Ws = nullptr;                  // split-bf16 planes of W
    float* Wrm = nullptr;                // narrow layers (linear2): the matrix as loaded, row-major [N][K] (rc_live.hip)
    int K = 0, N = 0, Kp = 0, Np = 0;
    int mr = 2, nc = 4;                  // tile shape: 16*mr rows x 16*nc columns
};
struct NetDev {
    Dense lin1, lin2;
    float* Wl[2] = {nullptr, nullptr};   // LSTM layers, K' = 2H, N' = 4H (tile-interleaved gates)
    void* Wls[2] = {nullptr, nullptr};   // their split-bf16 planes
    float* bl[2] = {nullptr, nullptr};
    float* h = nullptr;                  // [layer][copy of RC_HBUF][B][H]
    float* c = nullptr;                  // [layer][B][H]
    int* steps = nullptr;                // [B]
    float* x1 = nullptr;                 // relu(linear1) scratch [B][H]
    float* part = nullptr;               // lean live frame: per-tile partial sums of linear2 [H / 4][RC_LIVE_MAXB][outp]
    int in = 0, H = 0, out = 0;
    int nc = 4;                          // 16-column blocks per LSTM tile (4*nc hidden units x 4 gates)
    int mr = 2;                          // 16-row blocks per LSTM tile
};

struct rc_ctx {
    int B = 0;
    int Bp = 0;                          // B rounded up to the 32-row tile (row count of rc_pk buffers)
    int dev = 0;
    rc_params prm{};
    NetDev net[6];
    Dense init[3];
    float *hid1 = nullptr, *hid2 = nullptr, *xtmp = nullptr;
    FrameBuffers fb{};
    BodyConst* body = nullptr;
    float *mesh_vt = nullptr, *mesh_w = nullptr;      // full mesh (metrics only): v_template [V,3], weights [V,24]
    int mesh_V = 0;
    float* mesh_kM = nullptr;                         // keypoint regressor folded with the skinning data [n_used][24][4] (metrics only)
    int mesh_nk = 0;
    std::vector<float> mesh_vt_h, mesh_w_h, mesh_Jr_h; // host copies: the fold is recomputed when mesh, regressor or root change
    float jroot_h[3] = {0.f, 0.f, 0.f};
    bool fold_dirty = false;
    DevBuf<float> sweep_scratch;                      // per-frame transforms + slab partial sums of the mesh sweeps (grow-only)
    size_t sweep_scratch_cap = 0;
    unsigned long long ign_mask = RC_IGN_DEFAULT;     // smplify: landmarks with zeroed confidence
    bool have_body = false, have_weights = false;
    long long weights_epoch = 0;         // counts rc_finalize_weights (rc_subnet_backward: its transposed packs are derived from the packings)
    std::map<std::string, std::vector<float>> staged;    // host copy of the tensors loaded since the last rc_finalize_weights
                                                         // (released there: a context does not hold 254 MB of host memory)
    std::vector<DevBuf<char>> allocs;
    std::vector<std::pair<void*, size_t>> alloc_bytes;   // (pointer, bytes) of every dev_alloc that is not a weight: state + scratch
    std::vector<DevBuf<char>> weight_allocs;   // packed weights of the current rc_finalize_weights (freed by the next one)
    bool alloc_weights = false;          // dev_alloc books into weight_allocs
    std::string err;
    LiveOwner live;                      // the live session: stream, captures, packet chain, host mirror, knobs and counters (rc_live_api.cpp)
    SeqOwner seq;                        // the sequence engine of rc_sequence: planner's tables, ring, streams and events, resident tables, knobs and counters (rc_sequence_api.cpp)
    GemmOwner gemm;                      // the gate-GEMM launcher: arithmetic mode, tile and shared-weight knobs, slab pool, launch timing and counters (rc_gemm_api.cpp)
    SmplifyOwner smplify;                // optimiser work space (rc_smplify_api.cpp)
    SubnetOwner subnet;                  // scratch of rc_subnet_forward (rc_subnet_api.cpp)
    DevBuf<double> optim_partial;        // rc_subnet_optim_step: per-workgroup sums of squares of the gradient norm, sized once for the largest sub-net
    DevBuf<double> loss_partial;         // rc_subnet_loss: RC_LOSS_MAX_PARTIALS per-workgroup sums, allocated by the first call
    // rc_subnet_eval: per-workgroup sums of all groups (grow-only, its own: not loss_partial) and the group table
    DevBuf<double> eval_partial;
    size_t eval_partial_n = 0;
    StagedTable<EvalGroup, 4> eval_tab;
    // rc_motion_metrics: per-frame scratch, per-block (mean, M2) pairs (grow-only) and the group table
    DevBuf<float> motion_scratch;
    size_t motion_scratch_n = 0;
    DevBuf<double> motion_partial;
    size_t motion_partial_n = 0;
    StagedTable<MotionGroup, 4> motion_tab;
    // rc_aligned_metrics: the mesh fold (24 x 4 doubles m_j, then the listed pairs; rebuilt behind rc_set_mesh / rc_set_body), per-frame
    // scratch, per-(frame, slab) sums (grow-only) and the group table
    DevBuf<char> align_fold;
    size_t align_fold_bytes = 0;
    int align_pairs = 0;
    bool align_dirty = true;
    DevBuf<float> align_scratch;
    size_t align_scratch_n = 0;
    DevBuf<double> align_partial;
    size_t align_partial_n = 0;
    StagedTable<MotionGroup, 4> align_tab;
    // rc_set_shape_space / rc_prepare_motions (rc_prepare_api.cpp): the folded shape basis and the 39 picked vertices (one allocation, `prep_sp`
    // points into it), the per-sequence rest records, the IMU-vertex scratch of a call without vert6_out (grow-only) and the sequence table
    DevBuf<float> prep_space;
    PrepShapeSpace prep_sp{};
    int prep_V = 0;                      // mesh_V of the rc_set_shape_space call; 0: none yet
    bool prep_basis = false;             // it came with shapedirs and J_regressor: betas may be given
    DevBuf<PrepRest> prep_rest;
    size_t prep_rest_n = 0;
    DevBuf<float> prep_vert6;
    size_t prep_vert6_n = 0;
    StagedTable<PrepSeq, 4> prep_tab;
    // rc_prepare_camera_motions: per-sequence camera / detector offsets and the camera rows themselves (checked on the host, then sent)
    StagedTable<PrepCam, 4> cam_tab;
    StagedTable<PrepCamRow, 4> cam_rows;
    // rc_save_rows / rc_load_rows (rc_rowstate_api.cpp): the listed rows by 16-row block, sized once for every block of the context
    StagedTable<RowGroup, 4> row_tab;
};

#pragma GCC visibility push(hidden)
// rc_api.cpp
int fail(rc_ctx* ctx, int code, const std::string& msg);      // records the message (ctx == nullptr: for rc_last_error(nullptr)), returns code
int tune_env(const char* name, int dflt);
int check_ready(rc_ctx* ctx);
rc_params_dev dev_params(const rc_params& p);
int step_impl(rc_ctx* ctx, const FrameIO& io, uint32_t flags, hipStream_t st, bool with_tr = true, bool skip_prep = false,
              const FrameIO* next_io = nullptr, int n_live = -1);
template <typename T>
int dev_alloc(rc_ctx* ctx, T** p, size_t count, bool zero = true) {
    DevBuf<char> q;
    HIP_TRY(ctx, rc_alloc(q, count * sizeof(T)));
    if (zero) HIP_TRY(ctx, hipMemset(q.get(), 0, count * sizeof(T)));
    *p = reinterpret_cast<T*>(q.get());
    if (!ctx->alloc_weights) ctx->alloc_bytes.emplace_back(q.get(), count * sizeof(T));      // (what live_selfcheck saves and puts back: state + scratch)
    (ctx->alloc_weights ? ctx->weight_allocs : ctx->allocs).push_back(std::move(q));
    return RC_OK;
}
// rc_gemm_api.cpp: what the other three files take from the problem builders and the gate-GEMM launcher, and nothing beyond that
int gemm_create(rc_ctx* ctx);                                 // rc_create: every launcher knob (RC_GEMM_SPLIT, RC_LDS_*, RC_TILE_*, RC_LIVE_NT_MASK) is read
                                                              // here, once per context; a tile width that does not divide H fails (no HIP call)
struct Out { float* p; int ld; int col0; bool packed; };   // destination of a dense layer
struct Stage {                 // which rows of which net, reading which (rc_pk) input buffer, writing where
    int net; int flag_bit; const float* x; int ldx; Out y;
    const unsigned char* flags = nullptr;      // row-selection byte array (default: fb.flags)
    const float* x_alt = nullptr;              // input of rows lacking sel_bit in fb.flags (deferred updater step)
    int sel_bit = 0;
    int out_bit = 0;                           // linear2 writes only rows with this bit in fb.flags
    int rows_hint = -1;                        // expected active rows (-1 = the whole batch): picks the LSTM tile shape
};
GemmSeg seg(const float* base, int ld, int K, int mode = RC_PAR_NONE, long long stride = 0);
GemmProblem dense_problem(const rc_ctx* ctx, const Dense& d, GemmSeg a, Out out, bool relu, int flag_bit, const unsigned char* flags, int* steps,
                          bool open_step);
GemmProblem lin1_problem(const rc_ctx* c, const Stage& s);
GemmProblem lstm_problem(const rc_ctx* c, const Stage& s, int layer);
GemmProblem lin2_problem(const rc_ctx* c, const Stage& s);
bool tile_env(const char* name, int* mr, int* nc);
void pick_tile(int H, int rows, int* mr, int* nc);
bool gemm_split(const rc_ctx* c);                             // the context's products are NOT fp32: split-bf16 partial products (rc_set_gemm_mode 1 or 2)
int gemm_mode(const rc_ctx* c);                               // rc_get_gemm_mode: 0 fp32 MFMA, 1 six products of three truncated planes, 2 three products of two rounded planes
// Mode 2's weight planes (two round-to-nearest bf16 planes per matrix, 4 B per weight), built on the device from the fp32 packings.
// A context that never enters mode 2 has none. They live with the packed weights (rc_finalize_weights releases both) and are rewritten
// in place, on the caller's stream, by whatever rewrites a sub-net's packings in place.
void gemm_planes2_released(rc_ctx* ctx);                      // rc_finalize_weights freed the packed weights, the planes with them
int gemm_planes2_ensure(rc_ctx* ctx);                         // mode 2 and finalized weights: allocate and build what is missing (synchronises the device)
void gemm_planes2_refresh(rc_ctx* ctx, int net, hipStream_t st);   // sub-net `net`'s packings were rewritten on st: its planes follow, where the context has any
// "This problem runs on the shared-weight kernel (rc_gemm_lds.hip)": a CONTEXT takes it (and the tri engine) in split-product mode from
// RC_LDS_MIN_BATCH rows, a PROBLEM inside such a context from RC_LDS_MIN_ROWS rows.
bool lds_context(const rc_ctx* c);
bool lds_problem(const rc_ctx* c, int rows);
// Region r (< 12) of the shared-weight kernel's pool, which is allocated with the first call: the half-sum slabs and tickets of the launches
// that may be in flight at once (launch_problems rotates through all of them, the resident table uses tick & 3), and the tiles a region holds.
struct LdsRegion { float* slab; int* tickets; size_t tiles; };
int lds_region(rc_ctx* ctx, size_t r, LdsRegion* out);
int build_lds_problems(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, float* slab, int* tickets,
                       LdsProblem* out, int max_p, int* items, size_t* tiles_out, bool resident_order = false);
int launch_problems(rc_ctx* ctx, std::vector<GemmProblem> ps, const unsigned char* flags_override, hipStream_t st, bool fp32 = false,
                    hipEvent_t stop = nullptr, bool* launched = nullptr);
// One gate-GEMM launch with an event pair round it where rc_gemm_timing asks for one: mode 1 times every kind, mode 2 all but the small-tile
// kernel's, mode 3 only the shared-weight and resident kernels'. `issue` launches on st and nothing else.
enum LaunchKind { LAUNCH_SHARED, LAUNCH_WIDE, LAUNCH_SMALL, LAUNCH_RESIDENT };
int timed_launch_impl(rc_ctx* ctx, hipStream_t st, LaunchKind kind, void (*issue)(void*), void* arg);
template <class F> int timed_launch(rc_ctx* ctx, hipStream_t st, LaunchKind kind, F&& issue) {
    return timed_launch_impl(ctx, st, kind, [](void* f) { (*static_cast<std::remove_reference_t<F>*>(f))(); }, &issue);
}
bool resident_launch_fits_timing(const rc_ctx* c);            // false while a timing mode is on that also covers launches the resident segment replaces
void count_resident_launch(rc_ctx* ctx);                      // the resident kernel's launch counts with the shared-weight kernel's (rc_get_launch_stats)
// Scope guards: while one lives, launches are those of a live frame being captured / launched (GemmLaunch.live) | no launch is timed, and
// the previous setting returns on every exit path.
struct LiveLaunchScope { rc_ctx* ctx; explicit LiveLaunchScope(rc_ctx* c); ~LiveLaunchScope(); };
struct TimingSuspended { rc_ctx* ctx; bool was; explicit TimingSuspended(rc_ctx* c); ~TimingSuspended(); };
// rc_sequence_api.cpp
void seq_create(rc_ctx* ctx);                                 // rc_create: the RC_SEQ_* / RC_COST_* knobs are read here, once per context
int seq_prepare(rc_ctx* ctx);                                 // rc_finalize_weights: ring, streams, launch tables, the plan's tables for 1024 frames
void seq_weights_changed(rc_ctx* ctx);                        // ... and in front of it: the launch tables hold pointers to the old weights
bool seq_is_engine_stream(const rc_ctx* ctx, hipStream_t st); // st is the engine's second stream (the launcher's debug self-test keeps off it)
// rc_live_api.cpp
void live_create(rc_ctx* ctx);                                // rc_create: the RC_LIVE_* knobs are read here, once per context (RC_LIVE_NT_MASK: gemm_create)
void live_forget_last_frame(rc_ctx* ctx, bool rows_reset = false);   // an eager entry is about to move the state: the host mirror no longer knows
                                                              // the last frame (rows_reset: and any row may trigger init_net again)
int live_discard_ahead(rc_ctx* ctx);                          // what the session computed or queued ahead of the next frame no longer holds
int mark_eager(rc_ctx* ctx, hipStream_t st);                  // live_discard_ahead + the next live frame waits for the work just enqueued on st
bool live_session_open(const rc_ctx* ctx);                    // between rc_live_begin and rc_live_end: captured frames and a packet chain read the weights
#pragma GCC visibility pop
