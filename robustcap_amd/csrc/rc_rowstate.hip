// Row state on gfx950: the gather (context -> records) and the scatter (records -> context) behind rc_save_rows / rc_load_rows, and the
// element-wise write of rc_set_state. The reference keeps all of this in Python attributes of one Net per body (net/sig_mp.py:85-104,
// the RNN modules' (h, c) of L126-129); here a row's state is spread over the context's per-row arrays and moves as one record.
//
// Pure data movement, about 72 KB per row, so the thread mapping is the whole design. Grid: x = one GROUP (the listed rows of one 16-row
// block of the context, RowGroup), y = one SEGMENT of the record (RowSeg: a layer's h, a layer's c, x4l, x6l, the small block). The rows of
// a block are handled by ONE workgroup per segment because of where h lives: in rc_pk order the 16 rows of a block share every 256-byte
// piece [k-quad][row & 15][4] -- a row owns 16 bytes of it. With the m listed rows of the group as the FAST index of the work item
// (item i: row slot i % m, k-quad i / m) consecutive lanes read consecutive 16-byte pieces of one 256-byte piece: all 16 rows listed, a
// wave's dwordx4 access to the context is one contiguous 1 KiB (the ideal of the coalescing rule) and every line is fetched once; one
// row listed, the lanes run along k and the record side is the contiguous one, while the context side touches 16 bytes in every 256 --
// the partial lines that rc_pk costs a lone row, which no mapping removes. On the record side a row slot's pieces of one wave instruction
// are 64 / m consecutive k-quads: 64-byte runs at m = 16, 1 KiB at m = 1. c and the small block are row-major on both sides and take the
// row slot as the SLOW index. Plain vector loads and stores throughout; every index comes from the host-checked table.
#include "rc_internal.h"

template <bool LOAD> __device__ __forceinline__ void rs_move4(float* ctx_p, float* rec_p) {
    float4* a = reinterpret_cast<float4*>(ctx_p);
    float4* b = reinterpret_cast<float4*>(rec_p);
    if (LOAD) *a = *b; else *b = *a;
}
template <bool LOAD> __device__ __forceinline__ void rs_move1(unsigned* ctx_p, unsigned* rec_p) {
    if (LOAD) *ctx_p = *rec_p; else *rec_p = *ctx_p;
}

template <bool LOAD>
__global__ __launch_bounds__(256) void rc_rowstate_kernel(RowStateArgs a, const RowGroup* __restrict__ groups, float* blob) {
    __shared__ int s_row[16], s_rec[16], s_copy[16];
    const RowGroup* g = groups + blockIdx.x;
    const RowSeg sg = a.seg[blockIdx.y];
    const int m = g->m, tid = threadIdx.x;
    if (tid < m) {
        const int row = g->row[tid];
        s_row[tid] = row;
        s_rec[tid] = g->rec[tid];
        s_copy[tid] = (sg.kind == RC_RS_PK && sg.steps) ? sg.steps[row] % RC_HBUF : 0;
    }
    __syncthreads();
    if (sg.kind == RC_RS_PK) {
        const int items = m * (sg.ld >> 2);
        for (int i = tid; i < items; i += 256) {
            const int e = i % m, q = i / m;
            const int row = s_row[e];
            float* cp = sg.base + s_copy[e] * sg.copy_stride + rc_pk(row, 4 * q, sg.ld);
            float* rp = blob + s_rec[e] * a.rec_words + sg.rec_off + 4 * q;
            rs_move4<LOAD>(cp, rp);
        }
    } else if (sg.kind == RC_RS_ROWS) {
        const int Q = sg.ld >> 2, items = m * Q;
        for (int i = tid; i < items; i += 256) {
            const int e = i / Q, q = i % Q;
            float* cp = sg.base + (long long)s_row[e] * sg.ld + 4 * q;
            float* rp = blob + s_rec[e] * a.rec_words + sg.rec_off + 4 * q;
            rs_move4<LOAD>(cp, rp);
        }
    } else {
        const FrameBuffers& fb = a.fb;
        for (int i = tid; i < m * RC_ROWSTATE_SMALL; i += 256) {
            const int e = i / RC_ROWSTATE_SMALL, w = i % RC_ROWSTATE_SMALL;
            const int row = s_row[e];
            unsigned* rp = reinterpret_cast<unsigned*>(blob + s_rec[e] * a.rec_words + sg.rec_off) + w;
            void* cp = nullptr;
            if (w < 99) cp = fb.j_temp + row * 99 + w;
            else if (w < 132) cp = fb.floor + row * 33 + (w - 99);
            else if (w < 138) cp = fb.last_pfoot + row * 6 + (w - 132);
            else if (w < 141) cp = fb.last_tran + row * 3 + (w - 138);
            else if (w < 144) cp = fb.gravity + row * 3 + (w - 141);
            else if (w == 144) cp = fb.has_last + row;
            else if (w == 145) cp = fb.n_floor + row;
            else if (w == 146) cp = fb.first_reach + row;
            else if (w == 147) cp = fb.uv_count + row;
            else if (w == 148) {                                           // the pending mark is a byte in the context, a word in the record
                if (LOAD) fb.pend[row] = (unsigned char)*rp; else *rp = (unsigned)fb.pend[row];
                continue;
            } else if (w < 157) cp = fb.trace + row * 8 + (w - 149);
            else {                                                         // padding: zero in every record, never read
                if (!LOAD) *rp = 0u;
                continue;
            }
            rs_move1<LOAD>(static_cast<unsigned*>(cp), rp);
        }
    }
}

// rc_set_state: element (layer, row, e) of the caller's row-major [2, B, H] into the copy of h the row's counter designates / into c
__global__ __launch_bounds__(256) void rc_set_state_kernel(const float* __restrict__ hs, const float* __restrict__ cs,
                                                           const unsigned char* __restrict__ mask, const int* __restrict__ steps, float* h,
                                                           float* c, int B, long long BpH, int H) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2ll * B * H) return;
    const int l = (int)(idx / ((long long)B * H)), row = (int)((idx / H) % B), e = (int)(idx % H);
    if (mask && !mask[row]) return;
    if (hs) h[(l * RC_HBUF + steps[row] % RC_HBUF) * BpH + rc_pk(row, e, H)] = hs[idx];
    if (cs) c[idx] = cs[idx];
}

void rc_launch_rowstate(const RowStateArgs& a, const RowGroup* groups, int n_groups, float* blob, bool load, hipStream_t st) {
    if (n_groups <= 0) return;
    const dim3 grid((unsigned)n_groups, RC_ROWSTATE_SEGS), block(256);
    if (load) hipLaunchKernelGGL(rc_rowstate_kernel<true>, grid, block, 0, st, a, groups, blob);
    else hipLaunchKernelGGL(rc_rowstate_kernel<false>, grid, block, 0, st, a, groups, blob);
}

void rc_launch_set_state(const float* hs, const float* cs, const unsigned char* mask, const int* steps, float* h, float* c, int B,
                         long long BpH, int H, hipStream_t st) {
    const long long n = 2ll * B * H;
    hipLaunchKernelGGL(rc_set_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, hs, cs, mask, steps, h, c, B, BpH, H);
}
