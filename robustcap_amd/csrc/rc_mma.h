// MFMA building blocks of the gate GEMMs (rc_gemm.hip, rc_subnet.hip): one definition of the operand fragments and of the
// product chains, so that every kernel that forms a sum with them forms it with the same instructions in the same order.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MR, int NC>
struct Frag {                 // one chunk (16 k): a float4 per lane for each of the MR row blocks and NC column blocks
    f32x4 a[MR];
    f32x4 b[NC];
};

template <int MR, int NC, bool NTL = false>
__device__ __forceinline__ void load_chunk(Frag<MR, NC>& f, const float* const (&pa)[MR], long long aoff, const float* pb,
                                           long long bstride) {
#pragma unroll
    for (int r = 0; r < MR; ++r)
        f.a[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff);
#pragma unroll
    for (int j = 0; j < NC; ++j)
        {
            if constexpr (NTL) f.b[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pb + j * bstride));
            else f.b[j] = *reinterpret_cast<const f32x4*>(pb + j * bstride);
        }
}

template <int MR, int NC>
__device__ __forceinline__ void mma_chunk(const Frag<MR, NC>& f, f32x4 (&acc)[MR][NC]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
#pragma unroll
            for (int r = 0; r < MR; ++r) {
                acc[r][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[r][s], f.b[j][s], acc[r][j], 0, 0, 0);
            }
        }
    }
}

// ---- split-bf16 products (GemmLaunch.split) -----------------------------------------------------------------------------
// An fp32 value is EXACTLY the sum of three bf16 numbers (8 + 8 + 8 significant bits, truncation split: hi = top 16 bits of
// a, mid = top 16 bits of a - hi, lo = a - hi - mid), and a bf16 x bf16 product is exact in fp32. The gate GEMM then runs on
// v_mfma_f32_16x16x32_bf16 (17 cycles per 16x16x32 block against 8 x 32 cycles of v_mfma_f32_16x16x4_f32) as RC_SPLIT_PRODUCTS
// partial products per block pair with fp32 accumulation: 6 keep every term down to 2^-16 of the product (hi.hi, hi.mid,
// mid.hi, mid.mid, hi.lo, lo.hi; what is dropped is <= 2^-23 of a product, below the fp32 rounding of the running sum that
// the fp32 instruction makes as well), 9 keep all of them (the products are then exact; only the order of the fp32
// additions differs from an fma chain). Weights are split once on the host (three bf16 planes, 6 B per weight), activations
// on the fly (they stay fp32 everywhere else). One k-block = 32 k = two 16-k chunks of the rc_pk layout: lane (kq, i) holds
// k = 32 kb + {4 kq .. 4 kq + 3} and 32 kb + 16 + {4 kq .. 4 kq + 3} -- the same 8 k for the A and the B operand.
#ifndef RC_SPLIT_PRODUCTS
#define RC_SPLIT_PRODUCTS 6
#endif
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#ifndef RC_SPLIT_W32
#define RC_SPLIT_W32 0        // 1: the weights stream as fp32 too (the fp32 packing, 4 B instead of 6 B per weight) and are split in the K
#endif                        // loop like the activations: fewer operand bytes per MFMA for 36 more VALU per column block and k-block
#define RC_WPL (RC_SPLIT_W32 ? 2 : 3)          // 1-KiB pieces per column block and k-block: two fp32 chunks, or three bf16 planes
// W32 (round 5: a template parameter as well as the build macro): the launches whose weight slices have ONE reader -- every problem a single
// 64-row tile per slice, i.e. contexts of 48-64 rows -- are pure weight streams, and 4 B per weight beat 6 B + no split (measured in round 4 with
// the macro: batch 48 +13 %, 64 +7 %; at 256 rows, four readers per slice through the L2, -7 %). Bitwise the same products either way.
// NP = planes per operand: 3 (mode 1, the truncation split above) or 2 (mode 2, split2_rn below: two round-to-nearest terms)
template <int MR, int NC, bool W32 = (RC_SPLIT_W32 != 0), int NP = 3>
struct FragS {                // one k-block (32 k): fp32 activations (two float4 per row block), NP weight planes per column block
    static constexpr int WPL = (W32 || NP == 2) ? 2 : 3;      // 1-KiB pieces per column block: two fp32 chunks (W32, mode 1 only), or NP planes
    f32x4 a0[MR], a1[MR];
    u32x4 b[NC][WPL];
};

template <int MR, int NC, bool W32, int NP>
__device__ __forceinline__ void load_kblock(FragS<MR, NC, W32, NP>& f, const float* const (&pa)[MR], long long aoff, const u32x4* pb,
                                            long long bstride) {
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        f.a0[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff);
        f.a1[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff + 256);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int p = 0; p < FragS<MR, NC, W32, NP>::WPL; ++p) f.b[j][p] = pb[j * bstride + p * 64];
}

// a = hi + mid + lo exactly; each output packs 8 bf16 (element e in the low / high half of dword e / 2).
// Two elements per step on float2 values: the two subtractions of a pair compile to one v_pk_add_f32 each (9 VALU ops per
// pair instead of 11: the K loop issues its VALU work beside the MFMAs at 2-3 cycles per instruction).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3(const f32x4& x0, const f32x4& x1, u32x4& h, u32x4& m, u32x4& l) {
    const f32x2 a[4] = {f32x2{x0[0], x0[1]}, f32x2{x0[2], x0[3]}, f32x2{x1[0], x1[1]}, f32x2{x1[2], x1[3]}};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const u32x2 ua = __builtin_bit_cast(u32x2, a[d]);
        const f32x2 r1 = a[d] - __builtin_bit_cast(f32x2, ua & 0xffff0000u);          // a - hi, exact
        const u32x2 um = __builtin_bit_cast(u32x2, r1);
        const f32x2 r2 = r1 - __builtin_bit_cast(f32x2, um & 0xffff0000u);            // a - hi - mid, exact
        const u32x2 ul = __builtin_bit_cast(u32x2, r2);
        // bytes {hi[3], hi[2], lo[3], lo[2]} of the pair = the two truncated bf16
        h[d] = __builtin_amdgcn_perm(ua[1], ua[0], 0x07060302u);
        m[d] = __builtin_amdgcn_perm(um[1], um[0], 0x07060302u);
        l[d] = __builtin_amdgcn_perm(ul[1], ul[0], 0x07060302u);
    }
}

// Mode 2 (rc_set_gemm_mode): a ~ hi + mid, two bf16 terms by ROUNDING -- hi = RN_bf16(a) (round to nearest, ties to even: v_cvt_pk_bf16_f32),
// mid = RN_bf16(a - hi); the subtraction is exact in fp32 and nothing below mid is kept: |a - hi - mid| <= 2^-17 |a| (hi within 2^-9 |a|
// of a, mid within 2^-9 of that remainder). A block pair is then THREE products (mma_kblock: a_mid.w_hi, a_hi.w_mid, a_hi.w_hi) and
// a . w is off by at most about 3 x 2^-16 |a . w| for finite operands (a_mid.w_mid, <= 2^-16, is not formed; each operand's own
// remainder adds <= 2^-17). |a| within half a bf16 ulp of FLT_MAX rounds to inf where the truncation of mode 1 did not; a NaN stays a NaN.
// The device builds the weight planes of this mode with this very function (rc_planes2_kernel, rc_gemm.hip).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2_rn(const f32x4& x0, const f32x4& x1, u32x4& h, u32x4& m) {
    const f32x2 a[4] = {f32x2{x0[0], x0[1]}, f32x2{x0[2], x0[3]}, f32x2{x1[0], x1[1]}, f32x2{x1[2], x1[3]}};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned uh = __builtin_bit_cast(unsigned, __builtin_convertvector(a[d], bf16x2));     // element e in the low / high half
        const f32x2 r = a[d] - __builtin_bit_cast(f32x2, u32x2{uh << 16, uh & 0xffff0000u});         // a - hi, exact
        h[d] = uh;
        m[d] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
    }
}

template <int MR, int NC, bool W32, int NP>
__device__ __forceinline__ void load_kblock_b(FragS<MR, NC, W32, NP>& f, const u32x4* pb, long long bstride) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int p = 0; p < FragS<MR, NC, W32, NP>::WPL; ++p) f.b[j][p] = pb[j * bstride + p * 64];
}
template <int MR, int NC, bool W32, int NP>
__device__ __forceinline__ void load_kblock_a(FragS<MR, NC, W32, NP>& f, const float* const (&pa)[MR], long long aoff) {
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        f.a0[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff);
        f.a1[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff + 256);
    }
}

template <int MR, int NC, bool W32, int NP>
__device__ __forceinline__ void mma_kblock(const FragS<MR, NC, W32, NP>& f, f32x4 (&acc)[MR][NC]) {
    u32x4 wp[NP][NC];             // the column blocks' planes: hi, mid(, lo)
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if constexpr (NP == 2) {
            static_assert(!W32, "mode 2 reads its planes: 4 B per weight as they are");
            wp[0][j] = f.b[j][0]; wp[1][j] = f.b[j][1];
        } else {
            if constexpr (W32) split3(__builtin_bit_cast(f32x4, f.b[j][0]), __builtin_bit_cast(f32x4, f.b[j][1]), wp[0][j], wp[1][j], wp[2][j]);
            else { wp[0][j] = f.b[j][0]; wp[1][j] = f.b[j][1]; wp[2][j] = f.b[j][2]; }
        }
    }
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        // small terms first; consecutive MFMAs go to different accumulators (NC of them between two uses of one)
#define RC_PROD(AV, PL)                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < NC; ++j)                                                                        \
        acc[r][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AV, __builtin_bit_cast(bf16x8, wp[PL][j]), acc[r][j], 0, 0, 0);
        if constexpr (NP == 2) {
            u32x4 uh, um;
            split2_rn(f.a0[r], f.a1[r], uh, um);
            const bf16x8 ah = __builtin_bit_cast(bf16x8, uh), am = __builtin_bit_cast(bf16x8, um);
            RC_PROD(am, 0) RC_PROD(ah, 1) RC_PROD(ah, 0)
        } else {
            u32x4 uh, um, ul;
            split3(f.a0[r], f.a1[r], uh, um, ul);
            const bf16x8 ah = __builtin_bit_cast(bf16x8, uh), am = __builtin_bit_cast(bf16x8, um), al = __builtin_bit_cast(bf16x8, ul);
#if RC_SPLIT_PRODUCTS == 9
            RC_PROD(al, 2) RC_PROD(am, 2) RC_PROD(al, 1)
#endif
            RC_PROD(al, 0) RC_PROD(ah, 2) RC_PROD(am, 1) RC_PROD(am, 0) RC_PROD(ah, 1) RC_PROD(ah, 0)
        }
#undef RC_PROD
    }
}
