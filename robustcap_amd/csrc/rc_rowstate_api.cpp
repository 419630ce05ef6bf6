// Row state of a running context: rc_row_state_bytes, rc_save_rows, rc_load_rows (one record per row, rc_rowstate.hip) and rc_set_state.
// The host's part is the checking: the kernels take every index from the row table built here and from nowhere else.
#include "rc_ctx.h"

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace {

// segments of a record in record order (rc_internal.h: RowSeg) and the record's length in words
RowStateArgs rowstate_args(const rc_ctx* ctx) {
    RowStateArgs a{};
    const long long B = ctx->B, Bp = ctx->Bp;
    int s = 0, off = 0;
    for (int i = 0; i < 6; ++i) {
        const NetDev& n = ctx->net[i];
        for (int l = 0; l < 2; ++l) {
            a.seg[s++] = RowSeg{n.h + (long long)l * RC_HBUF * Bp * n.H, n.steps, Bp * n.H, n.H, off, RC_RS_PK, 0};
            off += n.H;
            a.seg[s++] = RowSeg{n.c + (long long)l * B * n.H, nullptr, 0, n.H, off, RC_RS_ROWS, 0};
            off += n.H;
        }
    }
    a.seg[s++] = RowSeg{ctx->fb.x4l, nullptr, 0, 256, off, RC_RS_PK, 0};
    off += 256;
    a.seg[s++] = RowSeg{ctx->fb.x6l, nullptr, 0, 256, off, RC_RS_PK, 0};
    off += 256;
    a.seg[s++] = RowSeg{nullptr, nullptr, 0, RC_ROWSTATE_SMALL, off, RC_RS_SMALL, 0};
    off += RC_ROWSTATE_SMALL;
    a.fb = ctx->fb;
    a.rec_words = off;
    return a;
}
static_assert(RC_ROWSTATE_SEGS == 6 * 2 * 2 + 3 && RC_ROWSTATE_SMALL % 4 == 0, "record segments");

long long record_bytes() {
    long long w = 512 + RC_ROWSTATE_SMALL;
    for (const NetSpec& n : kNets) w += 4ll * n.H;
    return 4 * w;
}

// Checks `io` against the context and, for n > 0, builds the row table in a pinned copy and sends it on io->stream. *groups = 0: nothing to do.
int stage_rows(rc_ctx* ctx, const rc_row_io* io, const char* who, int* groups) {
    *groups = 0;
    const std::string what = std::string(who) + ": ";
    if (!io) return fail(ctx, RC_ERR_INVALID, what + "null descriptor");
    if (!ctx->have_weights) return fail(ctx, RC_ERR_STATE, what + "weights not finalized (rc_finalize_weights)");
    const int B = ctx->B, n = io->n;
    if (n < 0 || n > B) return fail(ctx, RC_ERR_INVALID, what + "n = " + std::to_string(n) + " outside 0 .. batch = " + std::to_string(B));
    if (n == 0) return RC_OK;
    if (!io->blob) return fail(ctx, RC_ERR_INVALID, what + "null blob");
    if (io->bytes_per_row != record_bytes())
        return fail(ctx, RC_ERR_INVALID, what + "bytes_per_row = " + std::to_string(io->bytes_per_row) + ", this context's records have " +
                                             std::to_string(record_bytes()) + " (format " + std::to_string(RC_ROW_STATE_FORMAT) + ")");
    if ((uintptr_t)io->blob & 15) return fail(ctx, RC_ERR_INVALID, what + "the blob must be 16-byte aligned");
    std::vector<std::pair<int, int>> rr((size_t)n);                       // (row, record), then ascending by row
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n; ++i) {
        const int r = io->rows ? io->rows[i] : i;
        if (r < 0 || r >= B) return fail(ctx, RC_ERR_INVALID, what + "rows[" + std::to_string(i) + "] = " + std::to_string(r) + " outside 0 .. batch - 1");
        if (seen[r]) return fail(ctx, RC_ERR_INVALID, what + "row " + std::to_string(r) + " listed twice");
        seen[r] = 1;
        rr[i] = {r, i};
    }
    std::sort(rr.begin(), rr.end());
    const size_t max_groups = ((size_t)B + 15) / 16;
    RowGroup* th = nullptr;
    HIP_TRY(ctx, ctx->row_tab.stage(max_groups, &th));
    int G = 0;
    for (int i = 0; i < n; ++i) {
        if (i == 0 || (rr[i].first >> 4) != (rr[i - 1].first >> 4)) { th[G] = RowGroup{}; ++G; }
        RowGroup& g = th[G - 1];
        g.row[g.m] = rr[i].first;
        g.rec[g.m] = rr[i].second;
        g.m += 1;
    }
    // the device table is sized once, for every 16-row block of the context, by the context's first call (no kernel reads it yet): it never
    // grows behind a kernel, so no call waits for one
    if (!ctx->row_tab.holds(max_groups)) HIP_TRY(ctx, ctx->row_tab.grow(max_groups));
    hipStream_t st = (hipStream_t)io->stream;
    HIP_TRY(ctx, ctx->row_tab.upload((size_t)G, st));
    HIP_TRY(ctx, ctx->row_tab.record(st));
    *groups = G;
    return RC_OK;
}

}  // namespace

extern "C" {

int rc_row_state_bytes(rc_ctx* ctx, int64_t* bytes_per_row, int32_t* format) {
    if (!ctx) return RC_ERR_INVALID;
    if (bytes_per_row) *bytes_per_row = record_bytes();
    if (format) *format = RC_ROW_STATE_FORMAT;
    return RC_OK;
}

int rc_save_rows(rc_ctx* ctx, const rc_row_io* io) {
    if (!ctx) return RC_ERR_INVALID;
    int G = 0;
    if (int rc = stage_rows(ctx, io, "rc_save_rows", &G)) return rc;
    if (G == 0) return RC_OK;
    rc_launch_rowstate(rowstate_args(ctx), ctx->row_tab.get(), G, static_cast<float*>(io->blob), false, (hipStream_t)io->stream);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

int rc_load_rows(rc_ctx* ctx, const rc_row_io* io) {
    if (!ctx) return RC_ERR_INVALID;
    int G = 0;
    if (int rc = stage_rows(ctx, io, "rc_load_rows", &G)) return rc;
    if (G == 0) return RC_OK;
    live_forget_last_frame(ctx, true);                 // the rows' last frame, pending marks and first_reach are no longer what the live mirror saw
    rc_launch_rowstate(rowstate_args(ctx), ctx->row_tab.get(), G, static_cast<float*>(io->blob), true, (hipStream_t)io->stream);
    HIP_TRY(ctx, hipGetLastError());
    return mark_eager(ctx, (hipStream_t)io->stream);
}

int rc_set_state(rc_ctx* ctx, const char* net, const float* h_host, const float* c_host, const uint8_t* row_mask_host) {
    if (!ctx || !net) return RC_ERR_INVALID;
    const int ni = rc_ctx_net_index(net);
    if (ni < 0) return fail(ctx, RC_ERR_INVALID, std::string("rc_set_state: unknown net ") + net);
    if (!ctx->have_weights) return fail(ctx, RC_ERR_STATE, "rc_set_state: weights not finalized (rc_finalize_weights)");
    if (!h_host && !c_host) return RC_OK;
    const NetDev& n = ctx->net[ni];
    const size_t B = ctx->B, H = n.H, half = 2 * B * H;
    HIP_TRY(ctx, hipDeviceSynchronize());              // behind all work of the device, whichever stream it is on
    hipStream_t st = nullptr;                          // the context's default stream
    live_forget_last_frame(ctx);
    if (int rc = rc_ctx_flush_pending(ctx, st)) return rc;
    DevBuf<float> stage;
    DevBuf<unsigned char> mask;
    HIP_TRY(ctx, rc_alloc(stage, 2 * half));
    if (row_mask_host) {
        HIP_TRY(ctx, rc_alloc(mask, B));
        HIP_TRY(ctx, hipMemcpy(mask.get(), row_mask_host, B, hipMemcpyHostToDevice));
    }
    if (h_host) HIP_TRY(ctx, hipMemcpy(stage.get(), h_host, half * sizeof(float), hipMemcpyHostToDevice));
    if (c_host) HIP_TRY(ctx, hipMemcpy(stage.get() + half, c_host, half * sizeof(float), hipMemcpyHostToDevice));
    rc_launch_set_state(h_host ? stage.get() : nullptr, c_host ? stage.get() + half : nullptr, mask.get(), n.steps, n.h, n.c, ctx->B,
                        (long long)ctx->Bp * n.H, n.H, st);
    HIP_TRY(ctx, hipGetLastError());
    if (int rc = mark_eager(ctx, st)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));            // (the staging buffers are released behind it)
    return RC_OK;
}

}  // extern "C"
