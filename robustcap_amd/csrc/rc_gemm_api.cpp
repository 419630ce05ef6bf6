// The gate-GEMM launcher of a context: the GEMM problem builders, the tile choice, the shared-weight kernel's slab pool, launch_problems, the
// timing of launches and the launch counters, with the C ABI entry points that set and read them. Host logic only. Everything it owns is a
// member of GemmLauncher, behind rc_ctx::gemm; the declarations under "rc_gemm_api.cpp" in rc_ctx.h are all that rc_api.cpp (frame-stepped
// plan), rc_sequence_api.cpp (wavefront and resident engines) and rc_live_api.cpp (captured frames) take from here.
#include "../../include/robustcap_hip.h"
#include "rc_ctx.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// From this batch on a context defaults to the split-bf16 products. Round 2 (frame-stepped launches only) put the break-even
// at 192 rows; with the wavefront engine a tick is two merged launches that fill the chip at any batch and the split won from
// ~80 rows; with 64-row tiles from 33 rows of a problem it wins from 48 (mixed, 128-frame calls, body-frames/s, split vs fp32
// MFMA: batch 40 329k vs 344k, 48 434k vs 410k, 64 556k vs 417k, 72 486k vs 339k). 64-row tiles for the FRAME-STEPPED full-batch
// stages stay tied to 192 rows (below that they leave CUs without a tile).
#define RC_SPLIT_MIN_BATCH 48
#define RC_TILE64_MIN_BATCH 192

#ifndef RC_NC1280
#define RC_NC1280 10      // 16-column blocks per rnn4 LSTM tile (probe builds: 8 lets two workgroups share a CU's LDS)
#endif

const int kLdsRegions = 12;               // launches whose half sums can be in flight at once (three streams, a tick ahead: <= 6)

#pragma GCC visibility push(hidden)

// The event pool stands behind nothing that outlives it: default destruction is fine. (rc_destroy has synchronised the device.)
struct GemmLauncher {
    int mode = 0;                        // rc_set_gemm_mode: 0 fp32 MFMA, 1 split-bf16 products (three truncated planes, six products), 2 two rounded planes, three products
    // mode 2: a matrix's three-plane packing (the Ws of every problem builder) -> its two-plane packing, swapped in where a launch is laid out.
    // Empty until the context first enters mode 2 with finalized weights; the buffers are booked with the packed weights.
    std::map<const void*, void*> planes2;
    bool live_launch = false;            // set while a live frame is captured / launched (GemmLaunch.live)
    unsigned live_nt_mask = 63u;         // RC_LIVE_NT_MASK: sub-nets (bit = kNets index) whose weights a live frame streams with non-temporal loads
    // LSTM tile shapes of full-batch stages (0 = pick_tile), RC_TILE_RNN4 / _RNN6 / _S2H512 / _RNN2. Full-batch LSTM stages (batch >= 128),
    // measured on MI355X with the split-bf16 products (profiles/r02_tile_sweep.txt): rnn4 64 x 80, rnn6 64 x 128, rnn3 / rnn7 / rnn8 64 x 64,
    // rnn2 32 x 64 (beside rnn4's 256 tiles a 64-row rnn2 tile only lengthens the launch). 64-row tiles halve the weight bytes a CU pulls per
    // product -- with the MFMA time cut 2.7x the K loop is operand-bound -- and the number of tile prologues / reductions / epilogues.
    int tile4[2] = {4, 5}, tile6[2] = {4, 8}, tile378[2] = {4, 4}, tile2[2] = {0, 0};
    int trace_next = 0;                  // tile-trace slot counter (tools/tile_trace.py)
    // timing of the gate GEMM launches (rc_gemm_timing)
    bool timing = false;
    int timing_mode = 1;                 // 1: every gate-GEMM launch, 2: all but the small-tile kernel's, 3: only the shared-weight and resident kernels' (is_timed)
    std::vector<std::pair<HipEvent, HipEvent>> ev_pool;
    size_t ev_used = 0;
    double timed_ms = 0.0;
    double timed_busy_ms = 0.0;          // time with at least one timed launch running (launches on two streams overlap)
    long long timed_launches = 0;
    // counters (rc_get_launch_stats, rc_get_launch_stats_w32)
    long long stat_wide_launches = 0;    // launches of the wide-tile kernels
    long long stat_lds_launches = 0;     // launches of the shared-weight kernel and of the resident kernel
    long long stat_w32_launches = 0;     // of the wide launches: those on rc_gemm_split48_w32_kernel (contexts of 33-64 rows)
    // shared-weight gate GEMM (rc_gemm_lds.hip): LSTM layer steps of >= lds_min_rows rows in split-product mode
    // Two thresholds (round 6, second session; tools/ab_batch.py): a CONTEXT takes the shared-weight kernel and the three-stream tick from
    // lds_min_batch rows (batch 64 loses a sixth with them: 688k -> 576k mixed), and inside such a context a PROBLEM runs on it from
    // lds_min_rows rows (the rnn4 / rnn6 problems of a mixed batch hold only the rows that see the camera). One threshold of 160 for both
    // (first session) left batch 96-128 on the 64-row tiles: batch 128 mixed 858k -> 933k, all-visible 1,073k -> 1,173k; 96: 691k -> 752k.
    int lds_min_rows = 64;               // RC_LDS_MIN_ROWS (0 = never); default: half the batch, within 64 .. 160 (batch 256: 128 = 160 within the noise, 64 costs 0.7 %)
    int lds_min_batch = 65;              // RC_LDS_MIN_BATCH: batch 72 / 80 / 88 mixed 528 / 587 / 653k on 64-row tiles (two row tiles, the second mostly padding) -> 585 / 654 / 691k;
                                         // 64 rows and fewer keep the one-reader 64-row launches (688k against 576k)
    int lds_ksplit[3] = {1, 2, 2};       // RC_LDS_KSPLIT_512 / _1024 / _1280: workgroups per tile (1: both K halves in one workgroup; the H = 512
                                         // nets' items are short -- 2 x 16 k-blocks -- and a hand-over per tile costs more than it levels: +1 %)
    bool lds_block_pick = true;          // RC_LDS_BLOCK_PICK (0 = always the compacted row list): one-tile contexts (<= 256 rows) pick the rows of a flagged problem
                                         // by 16-row storage block where that costs the busiest SIMD no extra block -- aligned activation loads
    DevBuf<float> lds_slab;              // [kLdsRegions][lds_region_tiles][RC_LDS_SLAB_FLOATS]: half sums in flight, one region per launch
    DevBuf<int> lds_tickets;             // [kLdsRegions][lds_region_tiles]
    size_t lds_region_tiles = 0;
    unsigned lds_rot = 0;                // launch_lds: the region of the next launch
};

void rc_gemm_free(GemmLauncher* g) { delete g; }

static int default_gemm_mode(int rows) { return tune_env("RC_GEMM_SPLIT", rows >= RC_SPLIT_MIN_BATCH ? 1 : 0) != 0 ? 1 : 0; }   // (never 2: mode 2 is asked for, not defaulted to)

// the mode a new context of that many rows starts in: the default, or 2 where RC_GEMM_SPLIT=2 asks for it (rc_initial_gemm_mode)
static int initial_gemm_mode(int rows) { return tune_env("RC_GEMM_SPLIT", -1) == 2 ? 2 : default_gemm_mode(rows); }

int gemm_create(rc_ctx* ctx) {
    ctx->gemm.reset(new GemmLauncher());
    GemmLauncher& g = *ctx->gemm;
    const int batch = ctx->B;
    g.mode = initial_gemm_mode(batch);                      // RC_GEMM_SPLIT=2: the context starts in mode 2 (planes: rc_finalize_weights)
    g.live_nt_mask = (unsigned)tune_env("RC_LIVE_NT_MASK", 63);
    g.lds_min_rows = tune_env("RC_LDS_MIN_ROWS", std::min(160, std::max(64, batch / 2)));
    g.lds_min_batch = tune_env("RC_LDS_MIN_BATCH", g.lds_min_batch);
    g.lds_block_pick = tune_env("RC_LDS_BLOCK_PICK", 1) != 0;
    g.lds_ksplit[0] = tune_env("RC_LDS_KSPLIT_512", 1) == 1 ? 1 : 2;
    // rnn6: one workgroup per tile up to 160 rows (batch 80 / 128 mixed 642 -> 675k / 910 -> 956k, 128 all-visible 1,123 -> 1,165k, 160: +1.4 %),
    // the K halves on two workgroups above (batch 256: 1,400 vs 1,384k all-visible, 1,189 vs 1,182k mixed)
    g.lds_ksplit[1] = tune_env("RC_LDS_KSPLIT_1024", batch <= 160 ? 1 : 2) == 1 ? 1 : 2;
    g.lds_ksplit[2] = tune_env("RC_LDS_KSPLIT_1280", 2) == 1 ? 1 : 2;
    // lstm_problem runs H / (4 nc) column tiles: a width that does not divide H (4x5 / 2x10 on H = 512 or 1024) would leave the
    // last units of every layer step uncomputed -- rejected here rather than run
    const struct { const char* knob; int* tile; int H; } tiles[4] = {{"RC_TILE_RNN6", g.tile6, 1024}, {"RC_TILE_S2H512", g.tile378, 512},
                                                                     {"RC_TILE_RNN2", g.tile2, 512}, {"RC_TILE_RNN4", g.tile4, 1280}};
    for (const auto& t : tiles) tile_env(t.knob, &t.tile[0], &t.tile[1]);
    for (const auto& t : tiles)
        if (t.tile[1] > 0 && t.H % (4 * t.tile[1]) != 0)
            return fail(nullptr, RC_ERR_INVALID, std::string("rc_create: ") + t.knob + " tile width of " + std::to_string(4 * t.tile[1]) +
                                                 " units does not divide H = " + std::to_string(t.H));
    return RC_OK;
}

bool gemm_split(const rc_ctx* c) { return c->gemm->mode != 0; }
int gemm_mode(const rc_ctx* c) { return c->gemm->mode; }
bool lds_context(const rc_ctx* c) { return c->gemm->mode != 0 && c->gemm->lds_min_rows > 0 && c->B >= c->gemm->lds_min_batch; }
bool lds_problem(const rc_ctx* c, int rows) { return lds_context(c) && rows >= c->gemm->lds_min_rows; }

LiveLaunchScope::LiveLaunchScope(rc_ctx* c) : ctx(c) { ctx->gemm->live_launch = true; }
LiveLaunchScope::~LiveLaunchScope() { ctx->gemm->live_launch = false; }
TimingSuspended::TimingSuspended(rc_ctx* c) : ctx(c), was(c->gemm->timing) { ctx->gemm->timing = false; }
TimingSuspended::~TimingSuspended() { ctx->gemm->timing = was; }

// ------------------------------------------------------------------------------------------ problem builders
GemmSeg seg(const float* base, int ld, int K, int mode, long long stride) {
    GemmSeg s{};
    s.base = base; s.ld = ld; s.K = K; s.par_mode = mode; s.par_stride = stride;
    return s;
}

GemmProblem dense_problem(const rc_ctx* ctx, const Dense& d, GemmSeg a, Out out, bool relu, int flag_bit,
                          const unsigned char* flags, int* steps, bool open_step) {
    GemmProblem p{};
    a.K = d.Kp;
    p.seg[0] = a;
    p.seg[1] = seg(a.base, a.ld, 0);
    p.W = d.W; p.Ws = d.Ws; p.bias = d.b; p.out = out.p; p.ldo = out.ld; p.N = d.N; p.out_col0 = out.col0; p.out_packed = out.packed ? 1 : 0;
    p.steps = steps; p.flags = flags; p.flag_bit = flag_bit;
    p.epi = relu ? RC_EPI_RELU : RC_EPI_DENSE;
    p.open_step = open_step ? 1 : 0;
    // batch <= 16 (live mode): every launch of the frame is weight streaming -> 16 x 16 tiles throughout (twice the workgroups and the 8-deep load pipeline), which also
    // keeps each launch homogeneous so that it runs on the high-occupancy small-tile kernel
    // narrow layers (linear2, N <= 160) also run 16 x 16 tiles at any batch: +0.7 % on the bench over 16 x 32
    const bool narrow = ctx->B <= 16 || d.N <= 160;
    const int mr = narrow ? 1 : d.mr, nc = narrow ? 1 : d.nc;
    p.n_tiles = nc == 1 ? (d.N + 15) / 16 : d.Np / (16 * nc);          // 16-wide tiles: skip the all-padding ones
    p.m_tiles = (ctx->B + 16 * mr - 1) / (16 * mr); p.Kp = d.Kp; p.nc = nc; p.mr = mr;
    return p;
}

// LSTM tile shape (16*mr rows x 4*nc units) for a stage expected to touch `rows` rows: wide tiles when the row tiles
// alone fill the chip, narrow ones (more column tiles, each streaming a slice of the weights) when few rows are active.
// "4x8"-style tuning knob from the environment (A/B runs of tile shapes without a rebuild); false if unset / malformed
bool tile_env(const char* name, int* mr, int* nc) {
    const char* v = std::getenv(name);
    int a = 0, b = 0;
    if (!v || std::sscanf(v, "%dx%d", &a, &b) != 2) return false;
    const int code = a * 16 + b;
    for (int ok : {2 * 16 + 4, 4 * 16 + 4, 8 * 16 + 4, 2 * 16 + 8, 4 * 16 + 8, 2 * 16 + 10, 4 * 16 + 5})
        if (code == ok) { *mr = a; *nc = b; return true; }
    return false;
}

void pick_tile(int H, int rows, int* mr, int* nc) {
    if (rows >= 128) { *mr = 2; *nc = H == 1280 ? RC_NC1280 : (H == 1024 ? 8 : 4); return; }
    if (rows > 16) { *mr = 2; *nc = rows >= 64 ? 4 : 2; if (*nc == 2) { *mr = 1; } return; }
    *mr = 1; *nc = 1;
}

GemmProblem lin1_problem(const rc_ctx* c, const Stage& s) {
    const NetDev& n = c->net[s.net];
    GemmProblem p = dense_problem(c, n.lin1, seg(s.x, s.ldx, 0), Out{n.x1, n.H, 0, true}, true, s.flag_bit,
                                  s.flags ? s.flags : c->fb.flags, n.steps, true);
    if (s.rows_hint >= 0 && s.rows_hint <= 16) {      // few-row stage: 16 x 16 tiles like its LSTM launches (small-tile kernel)
        p.mr = 1; p.nc = 1; p.n_tiles = (n.lin1.N + 15) / 16;
    }
    if (s.rows_hint >= 0 && s.rows_hint < c->B) p.m_tiles = (s.rows_hint + 16 * p.mr - 1) / (16 * p.mr);
    p.alt_base = s.x_alt; p.sel_flags = c->fb.flags; p.sel_bit = s.x_alt ? s.sel_bit : 0;
    p.nt = (c->gemm->live_nt_mask >> s.net) & 1u;
    return p;
}
GemmProblem lstm_problem(const rc_ctx* c, const Stage& s, int layer) {
    const GemmLauncher& g = *c->gemm;
    const NetDev& n = c->net[s.net];
    const long long BH = (long long)c->Bp * n.H;
    GemmProblem p{};
    if (layer == 0) p.seg[0] = seg(n.x1, n.H, n.H);
    else p.seg[0] = seg(n.h, n.H, n.H, RC_PAR_DST, BH);                     // h of layer 0, just written
    p.seg[1] = seg(n.h + layer * RC_HBUF * BH, n.H, n.H, RC_PAR_SRC, BH);   // own h, previous step
    p.W = n.Wl[layer]; p.Ws = n.Wls[layer]; p.bias = n.bl[layer];
    p.hstate = n.h + layer * RC_HBUF * BH; p.cstate = n.c + layer * (long long)c->B * n.H; p.h_par_stride = BH; p.H = n.H;
    p.steps = n.steps; p.flags = s.flags ? s.flags : c->fb.flags; p.flag_bit = s.flag_bit;
    p.epi = RC_EPI_LSTM;
    int mr, nc;
    pick_tile(n.H, s.rows_hint < 0 ? c->B : s.rows_hint, &mr, &nc);
    if (s.rows_hint < 0 && c->B >= RC_TILE64_MIN_BATCH) {  // below that, 64-row tiles leave CUs without a tile
        // Second stage of a frame {rnn6, rnn3, rnn7, rnn8}: 64-row tiles. 128 CUs run the 128 rnn6 tiles (64 x 128) while
        // the other 128 run the 3 x 128 tiles (64 x 64) of the H = 512 nets in three rounds of a third of that length each,
        // instead of one round of 32 x 128 tiles followed by three rounds of 32 x 64 tiles: half as many tile prologues /
        // reductions / epilogues, fewer operand bytes per MFMA, and the launch still ends level.
        if (s.net == N6 && g.tile6[0]) { mr = g.tile6[0]; nc = g.tile6[1]; }
        if ((s.net == N3 || s.net == N7 || s.net == N8) && g.tile378[0]) { mr = g.tile378[0]; nc = g.tile378[1]; }
        if (s.net == N2 && g.tile2[0]) { mr = g.tile2[0]; nc = g.tile2[1]; }
        if (s.net == N4 && g.tile4[0]) { mr = g.tile4[0]; nc = g.tile4[1]; }
    }
    const int rows = s.rows_hint < 0 ? c->B : (s.rows_hint < c->B ? s.rows_hint : c->B);
    if (lds_problem(c, rows)) { mr = 16; nc = 8; }
    p.n_tiles = n.H / (4 * nc); p.m_tiles = (rows + 16 * mr - 1) / (16 * mr); p.Kp = 2 * n.H; p.nc = nc; p.mr = mr;
    p.nt = (g.live_nt_mask >> s.net) & 1u;
    return p;
}
GemmProblem lin2_problem(const rc_ctx* c, const Stage& s) {
    const NetDev& n = c->net[s.net];
    const long long BH = (long long)c->Bp * n.H;
    GemmProblem p = dense_problem(c, n.lin2, seg(n.h + RC_HBUF * BH, n.H, 0, RC_PAR_DST, BH), s.y, false, s.flag_bit,
                                  s.flags ? s.flags : c->fb.flags, n.steps, false);
    p.out_flags = c->fb.flags; p.out_bit = s.out_bit;
    p.nt = 1;
    return p;
}

// ------------------------------------------------------------------------------------------ mode 2's weight planes
namespace {
struct PackedMatrix { const float* W; const void* Ws; int Np, Kp; };
// every matrix a gate-GEMM problem can name (net < 0: all of them; init_net travels with rnn2)
std::vector<PackedMatrix> packed_matrices(const rc_ctx* ctx, int net) {
    std::vector<PackedMatrix> m;
    for (int i = 0; i < 6; ++i) {
        if (net >= 0 && i != net) continue;
        const NetDev& n = ctx->net[i];
        m.push_back({n.lin1.W, n.lin1.Ws, n.lin1.Np, n.lin1.Kp});
        m.push_back({n.lin2.W, n.lin2.Ws, n.lin2.Np, n.lin2.Kp});
        for (int l = 0; l < 2; ++l) m.push_back({n.Wl[l], n.Wls[l], 4 * n.H, 2 * n.H});
        if (i == N2)
            for (int q = 0; q < 3; ++q) m.push_back({ctx->init[q].W, ctx->init[q].Ws, ctx->init[q].Np, ctx->init[q].Kp});
    }
    return m;
}
}  // namespace

void gemm_planes2_released(rc_ctx* ctx) { ctx->gemm->planes2.clear(); }

int gemm_planes2_ensure(rc_ctx* ctx) {
    GemmLauncher& g = *ctx->gemm;
    if (g.mode != 2 || !ctx->have_weights || !g.planes2.empty()) return RC_OK;
    HIP_TRY(ctx, hipDeviceSynchronize());
    const bool booked = ctx->alloc_weights;
    ctx->alloc_weights = true;                                   // freed with the packings they were made from
    int rc = RC_OK;
    for (const PackedMatrix& m : packed_matrices(ctx, -1)) {
        uint16_t* q = nullptr;
        if ((rc = dev_alloc(ctx, &q, (size_t)m.Np * m.Kp * 2, false)) != RC_OK) break;
        rc_launch_planes2(m.W, q, m.Np, m.Kp, nullptr);
        g.planes2[m.Ws] = q;
    }
    ctx->alloc_weights = booked;
    if (rc == RC_OK && hipGetLastError() != hipSuccess) rc = fail(ctx, RC_ERR_HIP, "mode-2 weight planes: launch failed");
    if (rc == RC_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(ctx, RC_ERR_HIP, "mode-2 weight planes: build failed");
    if (rc != RC_OK) g.planes2.clear();                          // (what was allocated stays booked with the weights; nothing points at it)
    return rc;
}

void gemm_planes2_refresh(rc_ctx* ctx, int net, hipStream_t st) {
    GemmLauncher& g = *ctx->gemm;
    if (g.planes2.empty()) return;
    for (const PackedMatrix& m : packed_matrices(ctx, net)) {
        const auto it = g.planes2.find(m.Ws);
        if (it != g.planes2.end()) rc_launch_planes2(m.W, it->second, m.Np, m.Kp, st);
    }
}

// mode 2: the problems of a launch read the two-plane packings. false: a matrix without planes (the launch must not go out)
template <class P>
static bool to_planes2(const GemmLauncher& g, P* p, int n) {
    for (int i = 0; i < n; ++i) {
        const auto it = g.planes2.find(p[i].Ws);
        if (it == g.planes2.end()) return false;
        p[i].Ws = it->second;
    }
    return true;
}

// ------------------------------------------------------------------------------------------ slab pool, timing
// slabs + tickets of the shared-weight kernel: allocated on first use, sized for the widest launch of this context
static int ensure_lds_pool(rc_ctx* ctx) {
    GemmLauncher& g = *ctx->gemm;
    if (g.lds_slab) return RC_OK;
    const size_t m_tiles = ((size_t)ctx->B + 255) / 256;
    const size_t tiles = 320 * m_tiles;    // all twelve layer steps in one launch: 2 x (40 + 32 + 4 x 16) column tiles per row tile; + 34 of linear1 (resident kernel)
    HIP_TRY(ctx, rc_alloc(g.lds_slab, (size_t)kLdsRegions * tiles * RC_LDS_SLAB_FLOATS));
    HIP_TRY(ctx, rc_alloc(g.lds_tickets, (size_t)kLdsRegions * tiles));
    HIP_TRY(ctx, hipMemset(g.lds_tickets.get(), 0, (size_t)kLdsRegions * tiles * sizeof(int)));   // (the kernel leaves every ticket at zero)
    g.lds_region_tiles = tiles;
    return RC_OK;
}

int lds_region(rc_ctx* ctx, size_t r, LdsRegion* out) {
    if (int rc = ensure_lds_pool(ctx)) return rc;
    const GemmLauncher& g = *ctx->gemm;
    out->slab = g.lds_slab.get() + r * g.lds_region_tiles * RC_LDS_SLAB_FLOATS;
    out->tickets = g.lds_tickets.get() + r * g.lds_region_tiles;
    out->tiles = g.lds_region_tiles;
    return RC_OK;
}

static bool timing_pair(GemmLauncher& g, hipEvent_t* a, hipEvent_t* b) {
    if (g.ev_used == g.ev_pool.size()) {
        std::pair<HipEvent, HipEvent> ev;
        if (hipEventCreate(rc_out(ev.first)) != hipSuccess || hipEventCreate(rc_out(ev.second)) != hipSuccess) return false;
        g.ev_pool.push_back(std::move(ev));
    }
    const auto& ev = g.ev_pool[g.ev_used++];
    *a = ev.first.get(); *b = ev.second.get();
    return true;
}

// which launches a timing mode covers (GemmLauncher::timing_mode)
static bool is_timed(const GemmLauncher& g, LaunchKind kind) {
    if (!g.timing) return false;
    if (g.timing_mode == 3) return kind == LAUNCH_SHARED || kind == LAUNCH_RESIDENT;
    return !(g.timing_mode == 2 && kind == LAUNCH_SMALL);
}
bool resident_launch_fits_timing(const rc_ctx* c) { return !(c->gemm->timing && c->gemm->timing_mode != 3); }
void count_resident_launch(rc_ctx* ctx) { ctx->gemm->stat_lds_launches += 1; }

// (an event the launch itself carries rides on the dispatch as in an untimed run: the instrumented pass issues the same tick)
int timed_launch_impl(rc_ctx* ctx, hipStream_t st, LaunchKind kind, void (*issue)(void*), void* arg) {
    hipEvent_t a = nullptr, b = nullptr;
    if (is_timed(*ctx->gemm, kind) && !timing_pair(*ctx->gemm, &a, &b)) return fail(ctx, RC_ERR_HIP, "hipEventCreate");
    if (a) HIP_TRY(ctx, hipEventRecord(a, st));
    issue(arg);
    if (b) HIP_TRY(ctx, hipEventRecord(b, st));
    return RC_OK;
}

// ------------------------------------------------------------------------------------------ shared-weight launches
// The problems `ps` (LSTM layer steps; for the resident kernel also relu(linear1)) as ONE launch of the shared-weight kernel: longest items
// first, every problem's item range padded to a multiple of 8; *items = work items (workgroups) of the launch, *tiles = slab tiles it uses.
// resident_order: the linear1 items between the rnn4 / rnn6 items and those of the H = 512 nets (build_resident_ticks).
int build_lds_problems(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, float* slab, int* tickets,
                       LdsProblem* out, int max_p, int* items, size_t* tiles_out, bool resident_order) {
    std::vector<GemmProblem> ord(ps);
    auto key = [&](const GemmProblem& g) -> int {
        if (g.epi == RC_EPI_LSTM) return (resident_order && g.H == 512) ? 0 : g.Kp;
        return 1;                                                              // linear1: K' = 128 / 256
    };
    std::stable_sort(ord.begin(), ord.end(), [&](const GemmProblem& a, const GemmProblem& b) { return key(a) > key(b); });
    if ((int)ord.size() > max_p) return 0;
    int base = 0;
    size_t tiles = 0;
    for (size_t i = 0; i < ord.size(); ++i) {
        const GemmProblem& g = ord[i];
        LdsProblem& p = out[i];
        p = LdsProblem{};
        p.seg[0] = g.seg[0]; p.seg[1] = g.seg[1];
        p.Ws = g.Ws; p.bias = g.bias; p.hstate = g.hstate; p.cstate = g.cstate; p.steps = g.steps;
        p.flags = flags_override ? flags_override : g.flags; p.flag_bit = g.flag_bit;
        p.h_par_stride = g.h_par_stride; p.H = g.H; p.step_off = g.step_off;
        p.m_tiles = g.m_tiles; p.Qs = g.Kp / 32;
        p.epi = g.epi;
        p.block_pick = ctx->gemm->lds_block_pick && ctx->B <= 256 && g.m_tiles == 1 ? 1 : 0;
        if (g.epi == RC_EPI_LSTM) {
            p.n_tiles = g.H / 32;
            p.ksplit = ctx->gemm->lds_ksplit[g.H == 512 ? 0 : (g.H == 1024 ? 1 : 2)];
        } else {
            // relu(linear1): ONE input of K' columns as two halves (rc_pk: 16 columns = 256 floats further)
            const long long half = (long long)(g.Kp / 32) * 256;
            p.seg[0].K = g.Kp / 2;
            p.seg[1] = p.seg[0]; p.seg[1].base = g.seg[0].base + half;
            p.alt[0] = g.alt_base; p.alt[1] = g.alt_base ? g.alt_base + half : nullptr;
            p.sel_flags = g.sel_flags; p.sel_bit = g.alt_base ? g.sel_bit : 0;
            p.out = g.out; p.ldo = g.ldo;
            p.n_tiles = g.N / 128;
            p.ksplit = 1;
        }
        p.wg_base = base;
        p.slab = slab + tiles * RC_LDS_SLAB_FLOATS; p.tickets = tickets + tiles;
        tiles += (size_t)p.n_tiles * p.m_tiles;
        base += round_up(p.n_tiles * p.m_tiles * p.ksplit, 8);
    }
    *items = base; *tiles_out = tiles;
    return (int)ord.size();
}
static void build_lds_launch(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, const LdsRegion& region,
                             LdsLaunch& L, int* items, size_t* tiles_out) {
    L = LdsLaunch{};
    L.B = ctx->B;
    L.n = build_lds_problems(ctx, ps, flags_override, region.slab, region.tickets, L.p, RC_LDS_MAXP, items, tiles_out);
}

// LSTM layer steps on the shared-weight kernel (rc_gemm_lds.hip): problems marked mr = 16
static int launch_lds(rc_ctx* ctx, const std::vector<GemmProblem>& ps_in, const unsigned char* flags_override, hipStream_t st, hipEvent_t stop, bool* launched) {
    // RC_DBG_REPLICATE=n (tools/lds_load_probe.sh; timing only -- the copies write the same outputs): the launch carries every problem n
    // times: how long one and the same item takes with 1x, 2x, 3x, 4x as many CUs in a K loop beside it
    static const int replicate = std::getenv("RC_DBG_REPLICATE") ? std::atoi(std::getenv("RC_DBG_REPLICATE")) : 1;
    std::vector<GemmProblem> ps(ps_in);
    for (int r = 1; r < replicate && (int)ps.size() + (int)ps_in.size() <= RC_LDS_MAXP; ++r) ps.insert(ps.end(), ps_in.begin(), ps_in.end());
    LdsRegion region{};
    if (int rc = lds_region(ctx, ctx->gemm->lds_rot % kLdsRegions, &region)) return rc;
    ctx->gemm->lds_rot += 1;
    LdsLaunch L{};
    int base = 0;
    size_t tiles = 0;
    build_lds_launch(ctx, ps, flags_override, region, L, &base, &tiles);
    if (tiles > region.tiles) return fail(ctx, RC_ERR_INVALID, "shared-weight launch: more tiles than its slab region holds");
    const int planes = ctx->gemm->mode == 2 ? 2 : 3;
    if (planes == 2 && !to_planes2(*ctx->gemm, L.p, L.n)) return fail(ctx, RC_ERR_STATE, "gemm mode 2: a matrix has no weight planes");
    ctx->gemm->stat_lds_launches += 1;
    if (int rc = timed_launch(ctx, st, LAUNCH_SHARED, [&] { rc_launch_gemm_lds(L, base, st, stop, planes); })) return rc;
    if (launched && stop) *launched = true;
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

// ------------------------------------------------------------------------------------------ wide and small launches
// The problems of one launch of the wide-tile / small-tile kernels, laid out: XCD-aligned problems first so that (block id % 8) is the XCD
// for them, every problem's workgroups from a multiple of 8, the caller's row flags where it overrides them, the tile-trace slot.
// Returns the workgroups of the launch; -1: more problems than a launch holds, -2: mode 2 and a matrix without planes.
static int lay_out_launch(const rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, int mode, GemmLaunch& L) {
    L = GemmLaunch{};
    L.B = ctx->B;
    L.split = mode;
    L.live = ctx->gemm->live_launch ? 1 : 0;
    if ((int)ps.size() > RC_MAX_PROB) return -1;
    int base = 0;
    for (int unaligned = 0; unaligned < 2; ++unaligned)
        for (const GemmProblem& q : ps) {
            if (((q.n_tiles & 7) != 0) != (unaligned != 0)) continue;
            GemmProblem& p = L.p[L.n++];
            p = q;
            p.wg_base = base;
            if (flags_override) p.flags = flags_override;
            base += round_up(p.n_tiles * p.m_tiles, 8);
            p.trace_base = ctx->gemm->trace_next;
        }
    if (mode == 2 && !to_planes2(*ctx->gemm, L.p, L.n)) return -2;
    return base;
}

// RC_DBG_DENSE_ITEMS=1 -- self-test of the resident kernel's relu(linear1) items (tests/test_gpu_resident.py): every linear1 launch of the
// frame-stepped path first runs as ONE tick of the resident kernel, then as the launch of the wide-tile kernel it is; the two results
// must agree bit for bit wherever the launch wrote (stderr: one line per problem).
static bool dense_items_selftest_wanted(rc_ctx* ctx, const std::vector<GemmProblem>& ps, hipStream_t st, bool fp32) {
    static const int on = std::getenv("RC_DBG_DENSE_ITEMS") ? std::atoi(std::getenv("RC_DBG_DENSE_ITEMS")) : 0;
    if (!on || ctx->gemm->mode != 1 || fp32 || ctx->B > 256 || seq_is_engine_stream(ctx, st) || (int)ps.size() > RC_RES_MAXP) return false;
    for (const GemmProblem& p : ps)
        if (!(p.epi == RC_EPI_RELU && p.out_packed && p.N % 128 == 0 && p.Kp % 128 == 0 && p.out_bit == 0 && p.out_col0 == 0 && p.seg[0].par_mode == 0)) return false;
    return true;
}
static int dense_items_selftest(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, hipStream_t st) {
    LdsRegion region{};
    if (int rc = lds_region(ctx, 0, &region)) return rc;
    const int n_ints = 2 + RC_RES_MAXP + 1 + 4;
    DevBuf<ResidentTick> tk_d;                                               // (a debugging path: its tables live for this call)
    DevBuf<int> ints_d;
    HIP_TRY(ctx, rc_alloc_all(tk_d, 1, ints_d, n_ints));
    ResidentTick T{};
    std::vector<GemmProblem> q(ps);
    for (GemmProblem& p : q) p.m_tiles = 1;
    size_t tiles = 0;
    T.B = ctx->B;
    T.n = build_lds_problems(ctx, q, flags_override, region.slab, region.tickets, T.p, RC_RES_MAXP, &T.n_items, &tiles, true);
    for (int i = 0; i < RC_RES_MAXP; ++i) T.dep[i][0] = T.dep[i][1] = -1;
    const int base[2] = {0, T.n_items};
    const size_t Bp = (size_t)ctx->Bp;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (const GemmProblem& p : ps) HIP_TRY(ctx, hipMemset(p.out, 0xff, Bp * p.N * sizeof(float)));
    HIP_TRY(ctx, hipMemcpy(tk_d.get(), &T, sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(ints_d.get(), 0, n_ints * sizeof(int)));
    HIP_TRY(ctx, hipMemcpy(ints_d.get(), base, sizeof(base), hipMemcpyHostToDevice));
    ResidentArgs R{};
    R.ticks = tk_d.get(); R.item_base = ints_d.get(); R.n_ticks = 1;
    R.done = ints_d.get() + 2; R.tick_done = ints_d.get() + 2 + RC_RES_MAXP; R.head = ints_d.get() + 3 + RC_RES_MAXP; R.flag_tail = R.head + 1; R.abort = R.head + 2;
    R.spin_bound = 100000ull * 100;
    rc_launch_gemm_resident(R, 64, st);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::vector<std::vector<float>> got(ps.size());
    for (size_t i = 0; i < ps.size(); ++i) {
        got[i].resize(Bp * ps[i].N);
        HIP_TRY(ctx, hipMemcpy(got[i].data(), ps[i].out, got[i].size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemset(ps[i].out, 0xff, got[i].size() * sizeof(float)));
    }
    {   // the launch itself (it also opens the step)
        GemmLaunch L{};
        const int wg = lay_out_launch(ctx, ps, flags_override, 1, L);
        if (wg < 0) return fail(ctx, RC_ERR_INVALID, "too many fused problems");
        rc_launch_gemm(L, wg, st, nullptr);
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    for (size_t i = 0; i < ps.size(); ++i) {
        std::vector<float> ref(got[i].size());
        HIP_TRY(ctx, hipMemcpy(ref.data(), ps[i].out, ref.size() * sizeof(float), hipMemcpyDeviceToHost));
        size_t bad = 0, written = 0;
        for (size_t e = 0; e < ref.size(); ++e) {
            uint32_t r, g;
            std::memcpy(&r, &ref[e], 4); std::memcpy(&g, &got[i][e], 4);
            if (r == 0xffffffffu && g == 0xffffffffu) continue;                 // neither wrote it (rows the launch does not select)
            ++written;
            if (r != g) ++bad;
        }
        std::fprintf(stderr, "[dbg dense] N %d Kp %d alt %d: %zu of %zu written elements differ\n", ps[i].N, ps[i].Kp, ps[i].alt_base ? 1 : 0, bad, written);
    }
    return RC_OK;
}

// stop: event to be signalled by this launch's completion; *launched tells the caller whether a kernel went out that carries it
int launch_problems(rc_ctx* ctx, std::vector<GemmProblem> ps, const unsigned char* flags_override, hipStream_t st, bool fp32, hipEvent_t stop,
                    bool* launched) {
    GemmLauncher& g = *ctx->gemm;
    if (launched) *launched = false;
    if (ps.empty()) return RC_OK;
    if (dense_items_selftest_wanted(ctx, ps, st, fp32)) return dense_items_selftest(ctx, ps, flags_override, st);
    // LSTM layer steps marked for the shared-weight kernel (mr = 16) leave in a launch of their own behind the rest (everything
    // handed to one call is independent of everything else in it); outside split-product mode they take the 64 x 128 tile instead
    {
        std::vector<GemmProblem> lds, rest;
        for (GemmProblem& p : ps) {
            if (p.mr == 16) {
                if (g.mode != 0 && !fp32 && p.epi == RC_EPI_LSTM && (int)lds.size() < RC_LDS_MAXP) { lds.push_back(p); continue; }
                p.mr = 4; p.nc = 8; p.m_tiles *= 4;
            }
            rest.push_back(p);
        }
        if (!lds.empty()) {
            if (!rest.empty()) if (int rc = launch_problems(ctx, rest, flags_override, st, fp32)) return rc;
            return launch_lds(ctx, lds, flags_override, st, stop, launched);
        }
    }
    if ((int)ps.size() > RC_MAX_PROB) {        // (a tri tick of a mixed batch: linear1 + init_net + the few-row layer steps) two launches
        std::vector<GemmProblem> head(ps.begin(), ps.begin() + RC_MAX_PROB), tail(ps.begin() + RC_MAX_PROB, ps.end());
        if (int rc = launch_problems(ctx, head, flags_override, st, fp32)) return rc;
        return launch_problems(ctx, tail, flags_override, st, fp32, stop, launched);
    }
    GemmLaunch L{};
    const int base = lay_out_launch(ctx, ps, flags_override, fp32 ? 0 : g.mode, L);
    if (base == -2) return fail(ctx, RC_ERR_STATE, "gemm mode 2: a matrix has no weight planes");
    if (base < 0) return fail(ctx, RC_ERR_INVALID, "too many fused problems");
    g.trace_next = (g.trace_next + base) & 0x3fffffff;
    const bool small = rc_gemm_is_small(L);
    if (!small) g.stat_wide_launches += 1;
    if (rc_gemm_is_w32(L)) g.stat_w32_launches += 1;
    if (int rc = timed_launch(ctx, st, small ? LAUNCH_SMALL : LAUNCH_WIDE, [&] { rc_launch_gemm(L, base, st, stop); })) return rc;
    if (launched && stop) *launched = true;
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

#pragma GCC visibility pop

// =============================================================================================== C ABI
int rc_ctx_gemm_split(rc_ctx* ctx) { return ctx->gemm->mode != 0 ? 1 : 0; }
int rc_ctx_gemm_mode(rc_ctx* ctx) { return ctx->gemm->mode; }

extern "C" {

int rc_set_gemm_mode(rc_ctx* ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 2)
        return ctx ? fail(ctx, RC_ERR_INVALID, "rc_set_gemm_mode: 0 (fp32 MFMA), 1 (split-bf16, six products) or 2 (two rounded bf16 terms, three products)") : RC_ERR_INVALID;
    if (mode == ctx->gemm->mode) return RC_OK;
    rc_live_end(ctx);                                           // a captured frame has the kernel choice baked in
    const int was = ctx->gemm->mode;
    ctx->gemm->mode = mode;
    if (int rc = gemm_planes2_ensure(ctx)) { ctx->gemm->mode = was; return rc; }   // (before rc_finalize_weights: built there)
    return RC_OK;
}
int rc_get_gemm_mode(const rc_ctx* ctx) { return ctx ? ctx->gemm->mode : RC_ERR_INVALID; }
// (honours RC_GEMM_SPLIT like rc_create does: a sharded run pins every shard to this value)
int rc_default_gemm_mode(int32_t total_rows) { return default_gemm_mode(total_rows); }
int rc_initial_gemm_mode(int32_t total_rows) { return initial_gemm_mode(total_rows); }

int rc_get_launch_stats_w32(rc_ctx* ctx, int64_t* w32_launches) {
    if (!ctx || !w32_launches) return RC_ERR_INVALID;
    *w32_launches = ctx->gemm->stat_w32_launches;
    return RC_OK;
}

int rc_get_launch_stats(rc_ctx* ctx, int64_t* tick_launches, int64_t* other_wide_launches) {
    if (!ctx) return RC_ERR_INVALID;
    if (tick_launches) *tick_launches = ctx->gemm->stat_lds_launches;   // round 6: launches of the shared-weight kernel (rc_gemm_lds_kernel); round 5 counted its
                                                                        // one-launch-per-tick kernel here (removed: profiles/r06_tick_path_removed.diff)
    if (other_wide_launches) *other_wide_launches = ctx->gemm->stat_wide_launches;
    return RC_OK;
}

int rc_gemm_timing(rc_ctx* ctx, int32_t enable) {
    if (!ctx) return RC_ERR_INVALID;
    GemmLauncher& g = *ctx->gemm;
    g.timing = enable != 0;
    if (enable) g.timing_mode = enable == 2 ? 2 : (enable == 3 ? 3 : 1);   // (3 used to fall through to 1: every gate-GEMM launch was timed and averaged as if it were the shared-weight kernel's)
    if (enable) { g.ev_used = 0; g.timed_ms = 0.0; g.timed_launches = 0; g.timed_busy_ms = 0.0; }
    return RC_OK;
}
int rc_gemm_timing_read(rc_ctx* ctx, double* total_ms, int64_t* launches) {
    if (!ctx || !total_ms || !launches) return RC_ERR_INVALID;
    GemmLauncher& g = *ctx->gemm;
    // The wavefront engine runs the two wide launches of a tick on two streams: their durations overlap. Beside the sum, the time
    // during which AT LEAST ONE timed launch was running (union of the intervals, against the first event as the common origin).
    std::vector<std::pair<double, double>> iv;
    iv.reserve(g.ev_used);
    for (size_t i = 0; i < g.ev_used; ++i) {
        HIP_TRY(ctx, hipEventSynchronize(g.ev_pool[i].second.get()));
        float ms = 0.f, t0 = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, g.ev_pool[i].first.get(), g.ev_pool[i].second.get()));
        if (i > 0) HIP_TRY(ctx, hipEventElapsedTime(&t0, g.ev_pool[0].first.get(), g.ev_pool[i].first.get()));
        iv.emplace_back((double)t0, (double)t0 + ms);
        g.timed_ms += ms;
        g.timed_launches += 1;
    }
    std::sort(iv.begin(), iv.end());
    double lo = 0.0, hi = -1.0;
    for (const auto& x : iv) {
        if (hi < lo || x.first > hi) { if (hi > lo) g.timed_busy_ms += hi - lo; lo = x.first; hi = x.second; }
        else if (x.second > hi) hi = x.second;
    }
    if (hi > lo) g.timed_busy_ms += hi - lo;
    g.ev_used = 0;
    *total_ms = g.timed_ms;
    *launches = g.timed_launches;
    return RC_OK;
}
int rc_gemm_timing_busy(rc_ctx* ctx, double* busy_ms) {
    if (!ctx || !busy_ms) return RC_ERR_INVALID;
    *busy_ms = ctx->gemm->timed_busy_ms;
    return RC_OK;
}

}  // extern "C"
