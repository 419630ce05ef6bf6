// C ABI of librobustcap_hip.so (see include/robustcap_hip.h): context, weight repacking, per-frame launch plan.
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
// synchronisation. rc_sequence runs whole calls on the per-row-cursor wavefront engine instead (run_wave2_segment below): the
// same stages skewed over consecutive ticks and a ring of slots, two or three wide launches per tick on one to three streams.
#include "../../include/robustcap_hip.h"
#include "rc_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

// From this batch on a context defaults to the split-bf16 products. Round 2 (frame-stepped launches only) put the break-even
// at 192 rows; with the wavefront engine a tick is two merged launches that fill the chip at any batch and the split won from
// ~80 rows; with 64-row tiles from 33 rows of a problem it wins from 48 (mixed, 128-frame calls, body-frames/s, split vs fp32
// MFMA: batch 40 329k vs 344k, 48 434k vs 410k, 64 556k vs 417k, 72 486k vs 339k). 64-row tiles for the FRAME-STEPPED full-batch
// stages stay tied to 192 rows (below that they leave CUs without a tile).
#define RC_SPLIT_MAIN_MIN_BATCH 48  // wavefront engine: the tick's wide launches on streams of their own from this many rows (pick_wave_engine)
#define RC_SPLIT_MIN_BATCH 48
#define RC_TILE64_MIN_BATCH 192

#ifndef RC_NC1280
#define RC_NC1280 10      // 16-column blocks per rnn4 LSTM tile (probe builds: 8 lets two workgroups share a CU's LDS)
#endif

static thread_local std::string g_create_error;

int fail(rc_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

namespace {

const int kInit[3][2] = {{69, 512}, {512, 1024}, {1024, 2048}};

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

// ------------------------------------------------------------------------------------------ problem builders
GemmSeg seg(const float* base, int ld, int K, int mode = RC_PAR_NONE, long long stride = 0) {
    GemmSeg s{};
    s.base = base; s.ld = ld; s.K = K; s.par_mode = mode; s.par_stride = stride;
    return s;
}

struct Out { float* p; int ld; int col0; bool packed; };   // destination of a dense layer

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

struct Stage {                 // which rows of which net, reading which (rc_pk) input buffer, writing where
    int net; int flag_bit; const float* x; int ldx; Out y;
    const unsigned char* flags = nullptr;      // row-selection byte array (default: fb.flags)
    const float* x_alt = nullptr;              // input of rows lacking sel_bit in fb.flags (deferred updater step)
    int sel_bit = 0;
    int out_bit = 0;                           // linear2 writes only rows with this bit in fb.flags
    int rows_hint = -1;                        // expected active rows (-1 = the whole batch): picks the LSTM tile shape
};

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

// "This problem runs on the shared-weight kernel (rc_gemm_lds.hip)": a CONTEXT takes it (and the tri engine) in split-product mode from
// lds_min_batch rows, a PROBLEM inside such a context from lds_min_rows rows.
inline bool lds_context(const rc_ctx* c) { return c->gemm_split && c->lds_min_rows > 0 && c->B >= c->lds_min_batch; }
inline bool lds_problem(const rc_ctx* c, int rows) { return lds_context(c) && rows >= c->lds_min_rows; }

GemmProblem lin1_problem(const rc_ctx* c, const Stage& s) {
    const NetDev& n = c->net[s.net];
    GemmProblem p = dense_problem(c, n.lin1, seg(s.x, s.ldx, 0), Out{n.x1, n.H, 0, true}, true, s.flag_bit,
                                  s.flags ? s.flags : c->fb.flags, n.steps, true);
    if (s.rows_hint >= 0 && s.rows_hint <= 16) {      // few-row stage: 16 x 16 tiles like its LSTM launches (small-tile kernel)
        p.mr = 1; p.nc = 1; p.n_tiles = (n.lin1.N + 15) / 16;
    }
    if (s.rows_hint >= 0 && s.rows_hint < c->B) p.m_tiles = (s.rows_hint + 16 * p.mr - 1) / (16 * p.mr);
    p.alt_base = s.x_alt; p.sel_flags = c->fb.flags; p.sel_bit = s.x_alt ? s.sel_bit : 0;
    p.nt = (c->live_nt_mask >> s.net) & 1u;
    return p;
}
GemmProblem lstm_problem(const rc_ctx* c, const Stage& s, int layer) {
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
        if (s.net == N6 && c->tile6[0]) { mr = c->tile6[0]; nc = c->tile6[1]; }
        if ((s.net == N3 || s.net == N7 || s.net == N8) && c->tile378[0]) { mr = c->tile378[0]; nc = c->tile378[1]; }
        if (s.net == N2 && c->tile2[0]) { mr = c->tile2[0]; nc = c->tile2[1]; }
        if (s.net == N4 && c->tile4[0]) { mr = c->tile4[0]; nc = c->tile4[1]; }
    }
    const int rows = s.rows_hint < 0 ? c->B : (s.rows_hint < c->B ? s.rows_hint : c->B);
    if (lds_problem(c, rows)) { mr = 16; nc = 8; }
    p.n_tiles = n.H / (4 * nc); p.m_tiles = (rows + 16 * mr - 1) / (16 * mr); p.Kp = 2 * n.H; p.nc = nc; p.mr = mr;
    p.nt = (c->live_nt_mask >> s.net) & 1u;
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

const int kLdsRegions = 12;               // launches whose half sums can be in flight at once (three streams, a tick ahead: <= 6)

// slabs + tickets of the shared-weight kernel: allocated on first use, sized for the widest launch of this context
int ensure_lds_pool(rc_ctx* ctx) {
    if (ctx->lds_slab) return RC_OK;
    const size_t m_tiles = ((size_t)ctx->B + 255) / 256;
    const size_t tiles = 320 * m_tiles;    // all twelve layer steps in one launch: 2 x (40 + 32 + 4 x 16) column tiles per row tile; + 34 of linear1 (resident kernel)
    HIP_TRY(ctx, rc_alloc(ctx->lds_slab, (size_t)kLdsRegions * tiles * RC_LDS_SLAB_FLOATS));
    HIP_TRY(ctx, rc_alloc(ctx->lds_tickets, (size_t)kLdsRegions * tiles));
    HIP_TRY(ctx, hipMemset(ctx->lds_tickets.get(), 0, (size_t)kLdsRegions * tiles * sizeof(int)));   // (the kernel leaves every ticket at zero)
    ctx->lds_region_tiles = tiles;
    return RC_OK;
}

bool timing_pair(rc_ctx* ctx, hipEvent_t* a, hipEvent_t* b) {
    if (ctx->ev_used == ctx->ev_pool.size()) {
        std::pair<HipEvent, HipEvent> ev;
        if (hipEventCreate(rc_out(ev.first)) != hipSuccess || hipEventCreate(rc_out(ev.second)) != hipSuccess) return false;
        ctx->ev_pool.push_back(std::move(ev));
    }
    const auto& ev = ctx->ev_pool[ctx->ev_used++];
    *a = ev.first.get(); *b = ev.second.get();
    return true;
}

// The problems `ps` (LSTM layer steps; for the resident kernel also relu(linear1)) as ONE launch of the shared-weight kernel: longest items
// first, every problem's item range padded to a multiple of 8; *items = work items (workgroups) of the launch, *tiles = slab tiles it uses.
// resident_order: the linear1 items between the rnn4 / rnn6 items and those of the H = 512 nets (build_resident_ticks).
int build_lds_problems(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, float* slab, int* tickets,
                       LdsProblem* out, int max_p, int* items, size_t* tiles_out, bool resident_order = false) {
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
        if (g.epi == RC_EPI_LSTM) {
            p.n_tiles = g.H / 32;
            p.ksplit = ctx->lds_ksplit[g.H == 512 ? 0 : (g.H == 1024 ? 1 : 2)];
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
void build_lds_launch(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, float* slab, int* tickets,
                      LdsLaunch& L, int* items, size_t* tiles_out) {
    L = LdsLaunch{};
    L.B = ctx->B;
    L.n = build_lds_problems(ctx, ps, flags_override, slab, tickets, L.p, RC_LDS_MAXP, items, tiles_out);
}

// LSTM layer steps on the shared-weight kernel (rc_gemm_lds.hip): problems marked mr = 16
int launch_lds(rc_ctx* ctx, const std::vector<GemmProblem>& ps_in, const unsigned char* flags_override, hipStream_t st, hipEvent_t stop, bool* launched) {
    if (int rc = ensure_lds_pool(ctx)) return rc;
    // RC_DBG_REPLICATE=n (tools/lds_load_probe.sh; timing only -- the copies write the same outputs): the launch carries every problem n
    // times: how long one and the same item takes with 1x, 2x, 3x, 4x as many CUs in a K loop beside it
    static const int replicate = std::getenv("RC_DBG_REPLICATE") ? std::atoi(std::getenv("RC_DBG_REPLICATE")) : 1;
    std::vector<GemmProblem> ps(ps_in);
    for (int r = 1; r < replicate && (int)ps.size() + (int)ps_in.size() <= RC_LDS_MAXP; ++r) ps.insert(ps.end(), ps_in.begin(), ps_in.end());
    LdsLaunch L{};
    const size_t region = ctx->lds_rot++ % kLdsRegions;
    float* slab = ctx->lds_slab.get() + region * ctx->lds_region_tiles * RC_LDS_SLAB_FLOATS;
    int* tickets = ctx->lds_tickets.get() + region * ctx->lds_region_tiles;
    int base = 0;
    size_t tiles = 0;
    build_lds_launch(ctx, ps, flags_override, slab, tickets, L, &base, &tiles);
    if (tiles > ctx->lds_region_tiles) return fail(ctx, RC_ERR_INVALID, "shared-weight launch: more tiles than its slab region holds");
    ctx->stat_lds_launches += 1;
    if (ctx->timing) {
        hipEvent_t a, b;
        if (!timing_pair(ctx, &a, &b)) return fail(ctx, RC_ERR_HIP, "hipEventCreate");
        HIP_TRY(ctx, hipEventRecord(a, st));
        rc_launch_gemm_lds(L, base, st, stop);      // (the hand-over event rides on the dispatch as in an untimed run: the instrumented pass issues the same tick)
        if (launched && stop) *launched = true;
        HIP_TRY(ctx, hipEventRecord(b, st));
    } else {
        rc_launch_gemm_lds(L, base, st, stop);
        if (launched && stop) *launched = true;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

// RC_DBG_DENSE_ITEMS=1 -- self-test of the resident kernel's relu(linear1) items (tests/test_gpu_resident.py): every linear1 launch of the
// frame-stepped path first runs as ONE tick of the resident kernel, then as the launch of the wide-tile kernel it is; the two results
// must agree bit for bit wherever the launch wrote (stderr: one line per problem).
bool dense_items_selftest_wanted(rc_ctx* ctx, const std::vector<GemmProblem>& ps, hipStream_t st, bool fp32) {
    static const int on = std::getenv("RC_DBG_DENSE_ITEMS") ? std::atoi(std::getenv("RC_DBG_DENSE_ITEMS")) : 0;
    if (!on || !ctx->gemm_split || fp32 || ctx->B > 256 || st == ctx->aux_stream.get() || (int)ps.size() > RC_RES_MAXP) return false;
    for (const GemmProblem& p : ps)
        if (!(p.epi == RC_EPI_RELU && p.out_packed && p.N % 128 == 0 && p.Kp % 128 == 0 && p.out_bit == 0 && p.out_col0 == 0 && p.seg[0].par_mode == 0)) return false;
    return true;
}
int dense_items_selftest(rc_ctx* ctx, const std::vector<GemmProblem>& ps, const unsigned char* flags_override, hipStream_t st) {
    if (int rc = ensure_lds_pool(ctx)) return rc;
    const int n_ints = 2 + RC_RES_MAXP + 1 + 4;
    DevBuf<ResidentTick> tk_d;                                               // (a debugging path: its tables live for this call)
    DevBuf<int> ints_d;
    HIP_TRY(ctx, rc_alloc_all(tk_d, 1, ints_d, n_ints));
    ResidentTick T{};
    std::vector<GemmProblem> q(ps);
    for (GemmProblem& p : q) p.m_tiles = 1;
    size_t tiles = 0;
    T.B = ctx->B;
    T.n = build_lds_problems(ctx, q, flags_override, ctx->lds_slab.get(), ctx->lds_tickets.get(), T.p, RC_RES_MAXP, &T.n_items, &tiles, true);
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
        L.B = ctx->B; L.split = 1; L.live = ctx->live_launch ? 1 : 0;
        int wg = 0;
        std::vector<GemmProblem> ordered;
        for (auto& p : ps) if ((p.n_tiles & 7) == 0) ordered.push_back(p);
        for (auto& p : ps) if ((p.n_tiles & 7) != 0) ordered.push_back(p);
        for (size_t i = 0; i < ordered.size(); ++i) {
            ordered[i].wg_base = wg;
            if (flags_override) ordered[i].flags = flags_override;
            wg += round_up(ordered[i].n_tiles * ordered[i].m_tiles, 8);
            ordered[i].trace_base = ctx->trace_next;
            L.p[i] = ordered[i];
        }
        L.n = (int)ordered.size();
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

// stop: event to be signalled by this launch's completion (used only when the launch is not being timed); *launched tells the
// caller whether a kernel went out at all
int launch_problems(rc_ctx* ctx, std::vector<GemmProblem> ps, const unsigned char* flags_override, hipStream_t st, bool fp32 = false,
                    hipEvent_t stop = nullptr, bool* launched = nullptr) {
    if (launched) *launched = false;
    if (ps.empty()) return RC_OK;
    if (dense_items_selftest_wanted(ctx, ps, st, fp32)) return dense_items_selftest(ctx, ps, flags_override, st);
    // LSTM layer steps marked for the shared-weight kernel (mr = 16) leave in a launch of their own behind the rest (everything
    // handed to one call is independent of everything else in it); outside split-product mode they take the 64 x 128 tile instead
    {
        std::vector<GemmProblem> lds, rest;
        for (GemmProblem& p : ps) {
            if (p.mr == 16) {
                if (ctx->gemm_split && !fp32 && p.epi == RC_EPI_LSTM && (int)lds.size() < RC_LDS_MAXP) { lds.push_back(p); continue; }
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
    L.B = ctx->B;
    L.split = (ctx->gemm_split && !fp32) ? 1 : 0;
    L.live = ctx->live_launch ? 1 : 0;
    // XCD-aligned problems first so that (block id % 8) is the XCD for them
    std::vector<GemmProblem> ordered;
    for (auto& p : ps) if ((p.n_tiles & 7) == 0) ordered.push_back(p);
    for (auto& p : ps) if ((p.n_tiles & 7) != 0) ordered.push_back(p);
    if ((int)ordered.size() > RC_MAX_PROB) return fail(ctx, RC_ERR_INVALID, "too many fused problems");
    int base = 0;
    for (size_t i = 0; i < ordered.size(); ++i) {
        ordered[i].wg_base = base;
        if (flags_override) ordered[i].flags = flags_override;
        base += round_up(ordered[i].n_tiles * ordered[i].m_tiles, 8);
        ordered[i].trace_base = ctx->trace_next;
        L.p[i] = ordered[i];
    }
    L.n = (int)ordered.size();
    ctx->trace_next = (ctx->trace_next + base) & 0x3fffffff;
    if (!rc_gemm_is_small(L)) ctx->stat_wide_launches += 1;
    if (rc_gemm_is_w32(L)) ctx->stat_w32_launches += 1;
    if (ctx->timing && ctx->timing_mode != 3 && !(ctx->timing_mode == 2 && rc_gemm_is_small(L))) {
        hipEvent_t a, b;
        if (!timing_pair(ctx, &a, &b)) return fail(ctx, RC_ERR_HIP, "hipEventCreate");
        HIP_TRY(ctx, hipEventRecord(a, st));
        rc_launch_gemm(L, base, st, stop);
        if (launched && stop) *launched = true;
        HIP_TRY(ctx, hipEventRecord(b, st));
    } else {
        rc_launch_gemm(L, base, st, stop);
        if (launched && stop) *launched = true;
    }
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

int run_stage(rc_ctx* ctx, const std::vector<Stage>& nets, bool with_lin2, const std::vector<GemmProblem>* extra, hipStream_t st, bool fp32 = false) {
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

}  // namespace

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

int tune_env(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

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
        ctx->ring2[s] = f;
    }
    for (int i = 0; i < 6; ++i) {
        if (int rc = dev_alloc(ctx, &ctx->x1_alt[i], Bp * ctx->net[i].H)) return rc;
        if (int rc = dev_alloc(ctx, &ctx->x1_alt2[i], Bp * ctx->net[i].H)) return rc;
    }
    {
        // RC_SEQ_H512_PRIO: queue priority of wide2_stream (-1 lowest, +1 highest, 0 default). With the shared-weight kernel the caller's
        // stream carries the longest items of a tick (rnn4: the chain h(t) -> h(t + 1) is one item long); the other streams' are the filler.
        const int want = tune_env("RC_SEQ_H512_PRIO", 0);
        int lo = 0, hi = 0;
        if (want != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            HIP_TRY(ctx, hipStreamCreateWithPriority(rc_out(ctx->wide2_stream), hipStreamNonBlocking, want < 0 ? lo : hi));
        else
            HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(ctx->wide2_stream), hipStreamNonBlocking));
    }
    {
        // RC_SEQ_AUX_PRIO: -1 lowest / +1 highest queue priority for the second stream (0: default) -- its short kernels share the
        // CUs with the wide tiles of the caller's stream
        const int want = tune_env("RC_SEQ_AUX_PRIO", 0);
        int lo = 0, hi = 0;
        if (want != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            HIP_TRY(ctx, hipStreamCreateWithPriority(rc_out(ctx->aux_stream), hipStreamNonBlocking, want < 0 ? lo : hi));
        else
            HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(ctx->aux_stream), hipStreamNonBlocking));
    }
    HIP_TRY(ctx, hipStreamCreateWithFlags(rc_out(ctx->wide3_stream), hipStreamNonBlocking));
    for (int i = 0; i < 8; ++i) {
        // device-scope release: the hand-over is between two streams of this GPU
        const unsigned evf = hipEventDisableTiming | hipEventReleaseToDevice;
        HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->ev_main[i]), evf));
        HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->ev_aux[i]), evf));
        if (i < 4) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->ev_wide2[i]), evf));
        if (i < 4) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->ev_head[i]), evf));
        if (i < 4) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ctx->ev_wide3[i]), evf));
    }
    ctx->ring2_ready = true;
    ctx->wave2_valid = false;
    return RC_OK;
}

// Ring slots, the two extra streams and the hand-over events of the wavefront engine: allocated once. A failure half-way (out of memory)
// is final for the context: the slots already allocated stay owned by it (rc_destroy frees them) and later calls report the error
// instead of allocating all 16 slots and the streams a second time on top of the partial set.
int ensure_wave2_buffers(rc_ctx* ctx) {
    if (ctx->ring2_ready) return RC_OK;
    if (ctx->ring2_failed) return fail(ctx, RC_ERR_STATE, "wavefront engine: its buffers could not be allocated earlier (out of memory?)");
    const int rc = ensure_wave2_buffers_once(ctx);
    if (rc != RC_OK) ctx->ring2_failed = true;
    return rc;
}

// GEMM problems of every ring slot: problem q (kTick order, then the three init_net layers) working on slot sl. Rows come from
// the slot's flag bytes as in step_impl; tile shapes and row-tile counts are filled in per tick from the plan's row counts.
int build_wave2_problems(rc_ctx* ctx) {
    ctx->wave2_prob.assign((size_t)kRing * W2_PROB, GemmProblem{});
    const int B = ctx->B;
    for (int sl = 0; sl < kRing; ++sl) {
        const FrameBuffers& fb = ctx->ring2[sl];
        for (int q = 0; q < RC_TICK_PROB; ++q) {
            const TickStage& ts = kTick[q];
            const NetDev& n = ctx->net[ts.net];
            float* x1 = (sl & 1) ? ctx->x1_alt[ts.net] : n.x1;
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
            ctx->wave2_prob[(size_t)sl * W2_PROB + q] = p;
        }
        ctx->wave2_prob[(size_t)sl * W2_PROB + W2_INIT0] = dense_problem(ctx, ctx->init[0], seg(fb.xi, 128, 0), Out{ctx->hid1, 512, 0, true}, true, RC_ROW_REACH, fb.flags, nullptr, false);
        ctx->wave2_prob[(size_t)sl * W2_PROB + W2_INIT1] = dense_problem(ctx, ctx->init[1], seg(ctx->hid1, 512, 0), Out{ctx->hid2, 1024, 0, true}, true, RC_ROW_REACH, fb.flags, nullptr, false);
        ctx->wave2_prob[(size_t)sl * W2_PROB + W2_INIT2] = dense_problem(ctx, ctx->init[2], seg(ctx->hid2, 1024, 0), Out{ctx->fb.init_out, 2048, 0, false}, false, RC_ROW_REACH, fb.flags, nullptr, false);
    }
    ctx->wave2_valid = true;
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
    return eng == ENG_TRI && c->resident_on && c->B <= 256 && P.n_ticks > 0 && !(c->timing && c->timing_mode != 3);
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
    HIP_TRY(ctx, rc_grow(ctx->frame_at_cap, need, want, ctx->frame_at_d, want, ctx->frame_at_h, want));
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
        GemmProblem p = ctx->wave2_prob[(size_t)(e % kRing) * W2_PROB + q];
        if (kind == 0 || kind == 1) {                                          // relu(linear1) of the frame started at tick e: one of three buffers
            float* x1 = e % 3 == 0 ? ctx->net[net].x1 : (e % 3 == 1 ? ctx->x1_alt[net] : ctx->x1_alt2[net]);
            if (kind == 0) p.out = x1; else p.seg[0].base = x1;
        }
        if (kind == 1 || kind == 2) {
            const NetDev& n = ctx->net[net];
            int mr, nc;
            if (lds_problem(ctx, rows_k)) {                                    // the shared-weight kernel (rc_gemm_lds.hip)
                mr = 16; nc = 8;
            } else if (ctx->gemm_split && rows_k >= tile64_rows) {               // (split products: the K loop is operand-bound, 64-row tiles)
                const int* t = n.H == 512 ? tiles.t5 : (n.H == 1024 ? tiles.t6 : tiles.t4);
                mr = t[0]; nc = t[1];
            } else {
                pick_tile(n.H, rows_k, &mr, &nc);
            }
            p.mr = mr; p.nc = nc; p.n_tiles = n.H / (4 * nc);
        } else if (kind == 0 || kind == 4) {
            if (rows_k <= 16) { p.mr = 1; p.nc = 1; p.n_tiles = (p.N + 15) / 16; }
            else if (kind == 0 && ctx->gemm_split && rows_k >= tile64_rows) {
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
    S.wp.frame_at = S.ctx->frame_at_d.get() + (size_t)k * S.ctx->B;
    S.wp.first_tick = k == 0 ? 1 : 0;
    rc_launch_prep_wave(S.ctx->ring2[k % kRing], S.io0, S.prm, S.ctx->B, S.wp, S.aux);
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
        const FrameBuffers& tgt = ctx->ring2[k % kRing];
        S.wt.x4l = tgt.x4l; S.wt.x6l = tgt.x6l; S.wt.flags2 = tgt.flags2; S.wt.wsteps = tgt.wsteps;
    }
    if (merge && fuse && tail)
        merged = carried = rc_launch_fuse_tail(ctx->ring2[(k - kTailStage) % kRing], ctx->ring2[(k - kFuseStage) % kRing], S.io0, S.prm, ctx->body, B, S.wt, S.aux, signal);
    if (!merged && fuse) rc_launch_fuse(ctx->ring2[(k - kFuseStage) % kRing], S.io0, S.prm, B, S.aux);
    if (!merged && tail) {
        rc_launch_tail(ctx->ring2[(k - kTailStage) % kRing], S.io0, S.prm, ctx->body, B, 0, S.aux, nullptr, &S.wt, signal);
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
    hipStream_t st = S.st, aux = S.aux, w2 = ctx->wide2_stream.get(), w3 = ctx->wide3_stream.get();
    hipEvent_t main_p = ctx->ev_main[ep].get(), aux_p = ctx->ev_aux[ep].get(), w2_p = ctx->ev_wide2[ep].get(), w3_p = ctx->ev_wide3[ep].get(),
               head_p = ctx->ev_head[ep].get();
    hipEvent_t main_e = ctx->ev_main[e].get(), aux_e = ctx->ev_aux[e].get(), w2_e = ctx->ev_wide2[e].get(), w3_e = ctx->ev_wide3[e].get(),
               head_e = ctx->ev_head[e].get();
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
    ctx->stat_ticks += 1;
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
        ResidentTick& T = ctx->res_ticks_h[k];
        const size_t region = (size_t)(k & 3);
        size_t tiles = 0;
        T.B = ctx->B;
        T.n = build_lds_problems(ctx, ls, nullptr, ctx->lds_slab.get() + region * ctx->lds_region_tiles * RC_LDS_SLAB_FLOATS,
                                 ctx->lds_tickets.get() + region * ctx->lds_region_tiles, T.p, RC_RES_MAXP, &T.n_items, &tiles, true);
        if (T.n != (int)ls.size()) return fail(ctx, RC_ERR_INVALID, "resident engine: more problems in a tick than its table holds");
        if (tiles > ctx->lds_region_tiles) return fail(ctx, RC_ERR_INVALID, "resident engine: more tiles in a tick than a slab region holds");
        const bool tail_wrote = S.rows(S.P.n_reach, k - 1 - kTailStage) > 0;
        for (int i = 0; i < RC_RES_MAXP; ++i) {
            T.dep[i][0] = T.dep[i][1] = -1; T.dep_items[i][0] = T.dep_items[i][1] = 0;
            T.need_tail[i] = 0;
            if (i >= T.n) continue;
            const bool lstm = T.p[i].epi == RC_EPI_LSTM;
            T.need_tail[i] = lstm ? ((tail_wrote && T.p[i].H == 512) ? 1 : 0) : 1;
            if (k == 0 || !lstm) continue;
            const ResidentTick& Tp = ctx->res_ticks_h[k - 1];
            for (int j = 0; j < Tp.n; ++j) {
                const int items_j = (j + 1 < Tp.n ? Tp.p[j + 1].wg_base : Tp.n_items) - Tp.p[j].wg_base;
                const bool lstm_j = Tp.p[j].epi == RC_EPI_LSTM;
                if (lstm_j && Tp.p[j].hstate == T.p[i].hstate) { T.dep[i][0] = j; T.dep_items[i][0] = items_j; }                           // its own h(t - 1), c
                if ((const float*)(lstm_j ? Tp.p[j].hstate : Tp.p[j].out) == T.p[i].seg[0].base) { T.dep[i][1] = j; T.dep_items[i][1] = items_j; }   // layer 0's h | relu(linear1)
            }
        }
        ctx->res_base_h[k] = run;
        run += T.n_items;
    }
    ctx->res_base_h[S.P.n_ticks] = run;
    return RC_OK;
}

int run_resident_segment(WaveSeg& S) {
    rc_ctx* ctx = S.ctx;
    hipStream_t st = S.st, aux = S.aux;
    const int res_wgs = std::min(240, std::max(8, ctx->resident_wgs));
    if (int rc = ensure_lds_pool(ctx)) return rc;
    if (!ctx->res_abort_h) {                                                  // (read by the next rc_sequence call: kept until rc_destroy)
        HIP_TRY(ctx, rc_alloc(ctx->res_abort_h, 1));
        ctx->res_abort_h[0] = 0;
    }
    const size_t nt = (size_t)S.P.n_ticks;
    if (nt > ctx->res_cap) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        const size_t cap = nt + nt / 4 + 64;
        HIP_TRY(ctx, rc_grow(ctx->res_cap, nt, cap, ctx->res_ticks_d, cap, ctx->res_ticks_h, cap,
                             ctx->res_ints_d, cap * (RC_RES_MAXP + 2) + 1 + 4 + 16, ctx->res_base_h, cap + 1));   // (+ 16: the sums of a -DRC_RES_PROF build)
    }
    const size_t cap = ctx->res_cap;
    ResidentWords W{};
    W.item_base = ctx->res_ints_d.get(); W.done = W.item_base + cap + 1; W.tick_done = W.done + cap * RC_RES_MAXP; W.words = W.tick_done + cap;
    std::vector<std::vector<GemmProblem>> init_l(nt);
    if (int rc = build_resident_ticks(S, init_l)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->res_ticks_d.get(), ctx->res_ticks_h.get(), nt * sizeof(ResidentTick), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(W.item_base, ctx->res_base_h.get(), (nt + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(W.done, 0, (cap * (RC_RES_MAXP + 1) + 4 + 16) * sizeof(int), st));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_main[6].get(), st));
    HIP_TRY(ctx, hipStreamWaitEvent(aux, ctx->ev_main[6].get(), 0));
    ResidentArgs R{};
    R.ticks = ctx->res_ticks_d.get(); R.item_base = W.item_base; R.n_ticks = S.P.n_ticks;
    R.head = W.words; R.done = W.done; R.tick_done = W.tick_done;
    R.flag_tail = W.words + 2; R.abort = W.words + 3;
    R.spin_bound = (unsigned long long)std::max(1, tune_env("RC_SEQ_RESIDENT_BOUND_MS", 2000)) * 100000ull;   // wall_clock64: 100 MHz
    {
        hipEvent_t ta = nullptr, tb = nullptr;
        if (ctx->timing && !timing_pair(ctx, &ta, &tb)) return fail(ctx, RC_ERR_HIP, "hipEventCreate");
        if (ta) HIP_TRY(ctx, hipEventRecord(ta, st));
        rc_launch_gemm_resident(R, res_wgs, st);
        if (tb) HIP_TRY(ctx, hipEventRecord(tb, st));
    }
    ctx->stat_lds_launches += 1;
    // second stream, tick k: [init_net] -> prep -> [every item of tick k - 1] -> linear2 -> fuse -> tail -> flag_tail = k + 1
    for (int k = 0; k < S.P.n_ticks; ++k) {
        if (int rc = launch_problems(ctx, init_l[k], nullptr, aux, false)) return rc;
        wave_prep(S, k);
        if (k > 0) rc_launch_flag_wait(W.tick_done + (k - 1), ctx->res_ticks_h[k - 1].n_items, W.words + 3, R.spin_bound, aux);
        if (int rc = wave_lin2_fuse_tail(S, k, false, nullptr)) return rc;
        rc_launch_flag_set(W.words + 2, k + 1, aux);
        ctx->stat_ticks += 1;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_aux[0].get(), aux));
    HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_aux[0].get(), 0));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->res_abort_h.get(), W.words + 3, sizeof(int), hipMemcpyDeviceToHost, st));
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
    ctx->stat_resident_segments += 1;
    return RC_OK;
}

// Frames t0 .. t_last of a rc_sequence call on the wavefront engine: upload the plan's table, let the engine's streams join the caller's,
// issue every tick (or the resident segment), and let the caller's stream wait for the last tick of every other stream.
int run_wave2_segment(rc_ctx* ctx, const WavePlan& P, const FrameIO& io0, int t0, int t_last, hipStream_t st) {
    if (int rc = ensure_wave2_buffers(ctx)) return rc;
    if (!ctx->wave2_valid) if (int rc = build_wave2_problems(ctx)) return rc;
    const int B = ctx->B;
    const size_t need = (size_t)P.n_prep * B;                                  // the plan's table: frame every row starts at every tick
    if (need > ctx->frame_at_cap) {
        HIP_TRY(ctx, hipDeviceSynchronize());                               // nothing in flight (on any of the engine's streams) may still read the old table
        if (int rc = reserve_frame_at(ctx, need, need + need / 4 + 4096)) return rc;
    }
    std::memcpy(ctx->frame_at_h.get(), P.frame_at.data(), need * sizeof(int));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->frame_at_d.get(), ctx->frame_at_h.get(), need * sizeof(int), hipMemcpyHostToDevice, st));

    const WaveEngine eng = pick_wave_engine(ctx);
    WaveSeg S{ctx, P, io0, st, ctx->aux_stream.get(), eng, wave_tiles(eng), dev_params(ctx->prm), WavePrep{}, WaveTail{}};
    for (int i = 0; i < 6; ++i) S.wp.steps[i] = ctx->net[i].steps;
    S.wp.cx4l = ctx->fb.x4l; S.wp.cx6l = ctx->fb.x6l; S.wp.t0 = t0;
    S.wt.on = 1; S.wt.t_last = t_last;
    S.wt.steps4 = ctx->net[N4].steps; S.wt.steps6 = ctx->net[N6].steps;
    S.wt.cx4l = ctx->fb.x4l; S.wt.cx6l = ctx->fb.x6l;
    hipStream_t w2 = ctx->wide2_stream.get(), w3 = ctx->wide3_stream.get();
    HIP_TRY(ctx, hipEventRecord(ctx->ev_main[7].get(), st));                    // the engine's streams join (also: the table upload)
    HIP_TRY(ctx, hipStreamWaitEvent(S.aux, ctx->ev_main[7].get(), 0));
    if (eng != ENG_PLAIN) HIP_TRY(ctx, hipStreamWaitEvent(w2, ctx->ev_main[7].get(), 0));
    if (eng == ENG_TRI) HIP_TRY(ctx, hipStreamWaitEvent(w3, ctx->ev_main[7].get(), 0));
    if (resident_segment(ctx, eng, P)) {
        if (int rc = run_resident_segment(S)) return rc;
    } else {
        for (int k = 0; k < P.n_ticks; ++k) if (int rc = stream_tick(S, k)) return rc;
        const int last = (P.n_ticks - 1) & 3;
        if (P.n_ticks > 0) {
            HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_aux[last].get(), 0));
            if (eng != ENG_PLAIN) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_wide2[last].get(), 0));
            if (eng == ENG_TRI) {
                HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_head[last].get(), 0));
                HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_wide3[last].get(), 0));
                HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_main[last].get(), 0));
            }
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->stat_wave_frames += t_last - t0 + 1;
    return RC_OK;
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

// pinned + device tables of a planned rc_sequence call of T frames: regime codes [T][B], the rows' state, frame_at [ticks][B]
int reserve_plan_tables(rc_ctx* ctx, int T) {
    const size_t B = (size_t)ctx->B;
    const size_t need = B * (size_t)T;
    HIP_TRY(ctx, rc_grow(ctx->scan_cap, need, need, ctx->scan_codes_d, need, ctx->scan_codes_h, need));
    if (!ctx->scan_state_h) HIP_TRY(ctx, rc_alloc(ctx->scan_state_h, B * 3));
    const size_t fneed = B * ((size_t)T + 64);                                  // ticks of a T-frame plan: T + pipeline depth + lag
    return reserve_frame_at(ctx, fneed, fneed);
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
int rc_ctx_gemm_split(rc_ctx* ctx) { return ctx->gemm_split ? 1 : 0; }
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
    ctx->gemm_split = tune_env("RC_GEMM_SPLIT", batch >= RC_SPLIT_MIN_BATCH ? 1 : 0) != 0;
    live_create(ctx);
    ctx->seq_mode = tune_env("RC_SEQ_MODE", 1);          // 0 frame-stepped, 1 plan + cost estimate, 2 wavefront whenever long enough
    if (ctx->seq_mode < 0 || ctx->seq_mode > 2) ctx->seq_mode = 1;
    ctx->cost_tick_us = tune_env("RC_COST_TICK_PCT", 100) / 100.0;
    ctx->cost_tick_small_us = tune_env("RC_COST_HANDOVER_US", (int)ctx->cost_tick_small_us);
    ctx->cost_frame_us = tune_env("RC_COST_FRAME_US", (int)ctx->cost_frame_us);
    ctx->cost_tr_us = tune_env("RC_COST_TR_US", (int)ctx->cost_tr_us);
    ctx->lds_min_rows = tune_env("RC_LDS_MIN_ROWS", std::min(160, std::max(64, batch / 2)));
    ctx->lds_min_batch = tune_env("RC_LDS_MIN_BATCH", ctx->lds_min_batch);
    ctx->resident_on = tune_env("RC_SEQ_RESIDENT", 0) != 0;
    ctx->resident_wgs = tune_env("RC_SEQ_RESIDENT_WGS", ctx->resident_wgs);
    ctx->lds_ksplit[0] = tune_env("RC_LDS_KSPLIT_512", 1) == 1 ? 1 : 2;
    // rnn6: one workgroup per tile up to 160 rows (batch 80 / 128 mixed 642 -> 675k / 910 -> 956k, 128 all-visible 1,123 -> 1,165k, 160: +1.4 %),
    // the K halves on two workgroups above (batch 256: 1,400 vs 1,384k all-visible, 1,189 vs 1,182k mixed)
    ctx->lds_ksplit[1] = tune_env("RC_LDS_KSPLIT_1024", batch <= 160 ? 1 : 2) == 1 ? 1 : 2;
    ctx->lds_ksplit[2] = tune_env("RC_LDS_KSPLIT_1280", 2) == 1 ? 1 : 2;
    // Full-batch LSTM stages (batch >= 128), measured on MI355X with the split-bf16 products (profiles/r02_tile_sweep.txt):
    // rnn4 64 x 80, rnn6 64 x 128, rnn3 / rnn7 / rnn8 64 x 64, rnn2 32 x 64 (beside rnn4's 256 tiles a 64-row rnn2 tile
    // only lengthens the launch). 64-row tiles halve the weight bytes a CU pulls per product -- with the MFMA time cut 2.7x
    // the K loop is operand-bound -- and the number of tile prologues / reductions / epilogues.
    ctx->tile4[0] = 4; ctx->tile4[1] = 5;
    ctx->tile6[0] = 4; ctx->tile6[1] = 8;
    ctx->tile378[0] = 4; ctx->tile378[1] = 4;
    tile_env("RC_TILE_RNN6", &ctx->tile6[0], &ctx->tile6[1]);
    tile_env("RC_TILE_S2H512", &ctx->tile378[0], &ctx->tile378[1]);
    tile_env("RC_TILE_RNN2", &ctx->tile2[0], &ctx->tile2[1]);
    tile_env("RC_TILE_RNN4", &ctx->tile4[0], &ctx->tile4[1]);
    // lstm_problem runs H / (4 nc) column tiles: a width that does not divide H (4x5 / 2x10 on H = 512 or 1024) would leave the
    // last units of every layer step uncomputed -- rejected here rather than run
    const struct { const char* knob; int nc, H; } tiles[4] = {{"RC_TILE_RNN6", ctx->tile6[1], 1024}, {"RC_TILE_S2H512", ctx->tile378[1], 512},
                                                              {"RC_TILE_RNN2", ctx->tile2[1], 512}, {"RC_TILE_RNN4", ctx->tile4[1], 1280}};
    for (const auto& t : tiles)
        if (t.nc > 0 && t.H % (4 * t.nc) != 0) {
            rc_destroy(ctx);
            return fail(nullptr, RC_ERR_INVALID, std::string("rc_create: ") + t.knob + " tile width of " + std::to_string(4 * t.nc) +
                                                 " units does not divide H = " + std::to_string(t.H));
        }
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
    ctx->have_weights = false;
    ctx->wave2_valid = false;            // the sequence-mode launch tables hold weight pointers
    ctx->alloc_weights = true;
    const int rc = finalize_weights_impl(ctx);
    ctx->alloc_weights = false;
    return rc;
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
    // Everything the sequence engine allocates on first use -- the 16 ring slots, its two streams and 20 events, the launch tables, the
    // plan's pinned tables for calls of up to 1024 frames -- is set up HERE, not inside the first planned rc_sequence call (which used
    // to cost that call 13 ms inside its caller's timed region: round-3 verdict). Longer calls still grow the tables once.
    // (booked as context allocations, not as packed weights: a reload frees the latter)
    const bool aw = ctx->alloc_weights;
    ctx->alloc_weights = false;
    int rc_pre = RC_OK;
    if (ctx->seq_mode && !ctx->prm.live) {
        rc_pre = ensure_wave2_buffers(ctx);
        if (!rc_pre) rc_pre = build_wave2_problems(ctx);
        if (!rc_pre) rc_pre = reserve_plan_tables(ctx, 1024);
    }
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

// rc_sequence (len == nullptr) and rc_sequence_rows: frames [off, off + T) of a call whose per-row lengths are len[B] (HOST; their device
// copy is ctx->row_len_d), the pointers standing at frame `off`. Row b has frames 0 .. min(len[b] - off, T) - 1 of this piece.
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
    const int* len_d = L ? ctx->row_len_d.get() : nullptr;
    // Very long calls are planned in pieces: the plan's tables (regime codes, frame_at) grow with batch x frames, and a piece
    // boundary costs one pipeline drain (8 of 4,096 ticks) and one more read-back.
    const int32_t kMaxPlanFrames = std::max(8, tune_env("RC_SEQ_MAX_PLAN_FRAMES", 4096));     // (read per call: tests shrink it)
    if (T > kMaxPlanFrames && ctx->seq_mode && !ctx->prm.live) {
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
        ctx->stat_row_frames += rf;
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
    if (ctx->seq_mode && !ctx->prm.live && T >= 2 && T - w0 >= std::max(1, ctx->seq_min_frames)) {
        // ring, second stream and launch tables are set up by the first planned call (a warm-up call pays for them)
        if (int rc = ensure_wave2_buffers(ctx)) return rc;
        if (!ctx->wave2_valid) if (int rc = build_wave2_problems(ctx)) return rc;
        const size_t need = (size_t)B * T;
        if (need > ctx->scan_cap || !ctx->scan_state_h) {
            HIP_TRY(ctx, hipStreamSynchronize(st));                             // nothing in flight may still read the old tables
            if (int rc = reserve_plan_tables(ctx, T)) return rc;
        }
        rc_launch_scan_conf(j2dc, rs_j2d, B, T, ctx->prm.conf_lo, ctx->prm.conf_hi, ctx->scan_codes_d.get(), st, nullptr, len_d, off);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->scan_codes_h.get(), ctx->scan_codes_d.get(), need, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->scan_state_h.get(), ctx->fb.first_reach, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
        unsigned char* pend_b = reinterpret_cast<unsigned char*>(ctx->scan_state_h.get() + 2 * B);     // pinned, like the other two
        HIP_TRY(ctx, hipMemcpyAsync(pend_b, ctx->fb.pend, (size_t)B, hipMemcpyDeviceToHost, st));
        {   // a blocking wait wakes up tens of microseconds late: poll for a bounded while first (the stream may still hold
            // milliseconds of earlier frames, which a sleeping wait serves better)
            const auto t_spin = std::chrono::steady_clock::now();
            static const int spin = tune_env("RC_SEQ_SPIN", 1);
            while (spin && hipStreamQuery(st) == hipErrorNotReady &&
                   std::chrono::steady_clock::now() - t_spin < std::chrono::microseconds(300)) { }
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ctx->res_abort_h && ctx->res_abort_h[0]) {                           // (the copy sits behind the segment on this stream)
            ctx->stat_resident_aborts += 1;
            ctx->res_abort_h[0] = 0;
            return fail(ctx, RC_ERR_STATE, "resident layer-step kernel: a wait ran out in the previous call (its outputs and the recurrent state are invalid); "
                                           "RC_SEQ_RESIDENT=0 selects the stream engine");
        }
        for (int b = 0; b < B; ++b) ctx->scan_state_h[B + b] = pend_b[b];
        const bool ff = (flags & RC_FLAG_FIRST_FRAME) != 0;
        const bool imu = ctx->prm.use_imu_updater != 0, vup = ctx->prm.use_vision_updater != 0;
        {
            // per-row-cursor engine on frames [w0, T): the rows' state in front of frame w0
            std::vector<int> fr(ctx->scan_state_h.get(), ctx->scan_state_h.get() + B), pd(ctx->scan_state_h.get() + B, ctx->scan_state_h.get() + 2 * B);
            if (w0) {
                for (int b = 0; b < B; ++b) {
                    if (L && L[b] < 1) continue;                                 // the row has no frame 0: its state stays
                    const int c = ctx->scan_codes_h[b];
                    if (fr[b] && c == 2 && imu) fr[b] = 0;
                    pd[b] = (c == 0 && vup) ? 1 : 0;
                }
            }
            const double cost[4] = {ctx->cost_tick_us, ctx->cost_tick_small_us, ctx->cost_frame_us, ctx->cost_tr_us};
            plan_wave(ctx->scan_codes_h.get(), B, T, w0, fr.data(), pd.data(), imu, vup, cost, wplan, L);
            if (ctx->seq_mode == 2 || wplan.est_wave_us < wplan.est_stepped_us) wave2_from = w0;
            static const bool dbg = tune_env("RC_SEQ_DEBUG", 0) != 0;
            if (dbg) std::fprintf(stderr, "rc_sequence plan: T=%d ticks=%d lag_max=%d est_wave=%.0f us est_stepped=%.0f us -> %s\n", T, wplan.n_ticks,
                                  wplan.lag_max, wplan.est_wave_us, wplan.est_stepped_us, wave2_from >= 0 ? "wavefront" : "frame-stepped");
        }
        plan_sequence(ctx->scan_codes_h.get(), B, T, ctx->scan_state_h.get() + B, ff, vup, mode.data(), L);    // transition-launch marks of stepped frames
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
            ctx->stat_stepped_frames += 1;
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
    for (HipEvent& ev : ctx->row_len_ev)                                      // (before the capacity moves: a failure here is retried whole)
        if (!ev) HIP_TRY(ctx, hipEventCreateWithFlags(rc_out(ev), hipEventDisableTiming));
    const unsigned turn = ctx->row_len_turn++ & 1u;
    if (B > ctx->row_len_cap) HIP_TRY(ctx, rc_grow(ctx->row_len_cap, B, B, ctx->row_len_d, B, ctx->row_len_h, 2 * B));
    else HIP_TRY(ctx, hipEventSynchronize(ctx->row_len_ev[turn].get()));      // this half's last upload (two calls ago) has left it
    int* len_h = ctx->row_len_h.get() + turn * B;
    std::memcpy(len_h, len_host, B * sizeof(int));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->row_len_d.get(), len_h, B * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(ctx->row_len_ev[turn].get(), st));
    return sequence_impl(ctx, T, len_h, 0, j2dc, rs_j2d, accc, rs_acc, oric, rs_ori, first_tran, flags, pose_out, rs_pose, tran_out, rs_tran, stream);
}

int rc_get_sequence_row_frames(rc_ctx* ctx, int64_t* body_frames) {
    if (!ctx || !body_frames) return RC_ERR_INVALID;
    *body_frames = ctx->stat_row_frames;
    return RC_OK;
}

int rc_set_gemm_mode(rc_ctx* ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 1) return ctx ? fail(ctx, RC_ERR_INVALID, "rc_set_gemm_mode: 0 (fp32 MFMA) or 1 (split-bf16 products)") : RC_ERR_INVALID;
    if ((mode != 0) != ctx->gemm_split) rc_live_end(ctx);      // a captured frame has the kernel choice baked in
    ctx->gemm_split = mode != 0;
    return RC_OK;
}
int rc_get_gemm_mode(const rc_ctx* ctx) { return ctx ? (ctx->gemm_split ? 1 : 0) : RC_ERR_INVALID; }
// (honours RC_GEMM_SPLIT like rc_create does: a sharded run pins every shard to this value)
int rc_default_gemm_mode(int32_t total_rows) { return tune_env("RC_GEMM_SPLIT", total_rows >= RC_SPLIT_MIN_BATCH ? 1 : 0) != 0 ? 1 : 0; }

int rc_set_sequence_mode(rc_ctx* ctx, int32_t mode, int32_t min_frames) {
    if (!ctx || mode < 0 || mode > 2 || min_frames < 1) return ctx ? fail(ctx, RC_ERR_INVALID, "rc_set_sequence_mode: mode 0|1|2, min_frames >= 1") : RC_ERR_INVALID;
    ctx->seq_mode = mode;
    ctx->seq_min_frames = min_frames;
    return RC_OK;
}

int rc_get_sequence_stats(rc_ctx* ctx, int64_t* wave_frames, int64_t* stepped_frames, int64_t* ticks) {
    if (!ctx) return RC_ERR_INVALID;
    if (wave_frames) *wave_frames = ctx->stat_wave_frames;
    if (stepped_frames) *stepped_frames = ctx->stat_stepped_frames;
    if (ticks) *ticks = ctx->stat_ticks;
    return RC_OK;
}

int rc_set_resident(rc_ctx* ctx, int32_t enable, int32_t workgroups) {
    if (!ctx) return RC_ERR_INVALID;
    ctx->resident_on = enable != 0;
    if (workgroups > 0) ctx->resident_wgs = workgroups;
    return RC_OK;
}

int rc_get_resident_stats(rc_ctx* ctx, int64_t* segments, int64_t* aborts) {
    if (!ctx) return RC_ERR_INVALID;
    if (segments) *segments = ctx->stat_resident_segments;
    if (aborts) *aborts = ctx->stat_resident_aborts;
    return RC_OK;
}

int rc_get_launch_stats_w32(rc_ctx* ctx, int64_t* w32_launches) {
    if (!ctx || !w32_launches) return RC_ERR_INVALID;
    *w32_launches = ctx->stat_w32_launches;
    return RC_OK;
}

int rc_get_launch_stats(rc_ctx* ctx, int64_t* tick_launches, int64_t* other_wide_launches) {
    if (!ctx) return RC_ERR_INVALID;
    if (tick_launches) *tick_launches = ctx->stat_lds_launches;   // round 6: launches of the shared-weight kernel (rc_gemm_lds_kernel); round 5 counted its
                                                                  // one-launch-per-tick kernel here (removed: profiles/r06_tick_path_removed.diff)
    if (other_wide_launches) *other_wide_launches = ctx->stat_wide_launches;
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
    if (!pose || !tran || !joint || !j33) return fail(ctx, RC_ERR_INVALID, "rc_body_fk: null buffer");
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
int rc_syn_acc(const float* v, int64_t T, int64_t width, int32_t smooth_n, float* acc, void* stream) {
    if (T < 0 || width < 1 || smooth_n < 1) return RC_ERR_INVALID;
    if (T == 0) return RC_OK;
    if (!v || !acc) return RC_ERR_INVALID;
    if (smooth_n / 2 != 0 && T < 2 * (int64_t)smooth_n + 1) return RC_ERR_INVALID;     // the reference raises here
    rc_launch_syn_acc(v, acc, T, width, smooth_n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RC_OK : RC_ERR_HIP;
}
int rc_synth_imu(rc_ctx* ctx, const float* pose, const float* tran, const int32_t* vertex_ids, const int32_t* joint_ids, int64_t T,
                 int32_t smooth_n, float* imu_ori, float* imu_acc, float* joint3d, float* vert6, void* stream) {
    if (!ctx || !ctx->have_body || ctx->mesh_V == 0) return ctx ? fail(ctx, RC_ERR_STATE, "rc_synth_imu: rc_set_body / rc_set_mesh first") : RC_ERR_INVALID;
    if (T <= 0 || !pose || !tran || !vertex_ids || !joint_ids || !imu_ori || !imu_acc || !vert6 || smooth_n < 1)
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
    if (!pose || !tran || !kp || !K || !loss) return fail(ctx, RC_ERR_INVALID, "rc_reproj_residual: null buffer");
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
// K^-1 by the adjugate in double (the reference uses torch's float32 LU inverse, evaluate.py:34,70), R_cw, gravity
bool camera_constants(const float* K, const float* Tcw, CamConst* cam, float* g_out) {
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (det == 0.0) return false;
    const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                           (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                           (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
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
    CamConst cam;
    if (!camera_constants(K, Tcw, &cam, g_out)) return RC_ERR_INVALID;
    if (n == 0) return RC_OK;
    if (!kp || !acc || !ori || !j2dc || !accc || !oric) return RC_ERR_INVALID;
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
    for (int r = 0; r < n_rows; ++r)
        if (!camera_constants(K_host + 9 * (size_t)r, Tcw_host + 16 * (size_t)r, &cams[r], gravity_out_host + 3 * (size_t)r)) return RC_ERR_INVALID;
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

int rc_gemm_timing(rc_ctx* ctx, int32_t enable) {
    if (!ctx) return RC_ERR_INVALID;
    ctx->timing = enable != 0;
    if (enable) ctx->timing_mode = enable == 2 ? 2 : (enable == 3 ? 3 : 1);   // (3 used to fall through to 1: every gate-GEMM launch was timed and averaged as if it were the shared-weight kernel's)
    if (enable) { ctx->ev_used = 0; ctx->timed_ms = 0.0; ctx->timed_launches = 0; ctx->timed_busy_ms = 0.0; }
    return RC_OK;
}
int rc_gemm_timing_read(rc_ctx* ctx, double* total_ms, int64_t* launches) {
    if (!ctx || !total_ms || !launches) return RC_ERR_INVALID;
    // The wavefront engine runs the two wide launches of a tick on two streams: their durations overlap. Beside the sum, the time
    // during which AT LEAST ONE timed launch was running (union of the intervals, against the first event as the common origin).
    std::vector<std::pair<double, double>> iv;
    iv.reserve(ctx->ev_used);
    for (size_t i = 0; i < ctx->ev_used; ++i) {
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_pool[i].second.get()));
        float ms = 0.f, t0 = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_pool[i].first.get(), ctx->ev_pool[i].second.get()));
        if (i > 0) HIP_TRY(ctx, hipEventElapsedTime(&t0, ctx->ev_pool[0].first.get(), ctx->ev_pool[i].first.get()));
        iv.emplace_back((double)t0, (double)t0 + ms);
        ctx->timed_ms += ms;
        ctx->timed_launches += 1;
    }
    std::sort(iv.begin(), iv.end());
    double lo = 0.0, hi = -1.0;
    for (const auto& x : iv) {
        if (hi < lo || x.first > hi) { if (hi > lo) ctx->timed_busy_ms += hi - lo; lo = x.first; hi = x.second; }
        else if (x.second > hi) hi = x.second;
    }
    if (hi > lo) ctx->timed_busy_ms += hi - lo;
    ctx->ev_used = 0;
    *total_ms = ctx->timed_ms;
    *launches = ctx->timed_launches;
    return RC_OK;
}
int rc_gemm_timing_busy(rc_ctx* ctx, double* busy_ms) {
    if (!ctx || !busy_ms) return RC_ERR_INVALID;
    *busy_ms = ctx->timed_busy_ms;
    return RC_OK;
}

}  // extern "C"
