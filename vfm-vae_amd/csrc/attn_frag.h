// MFMA fragment plumbing shared by the attention kernels (attention.hip, attention_f32.hip, xattn.hip,
// qwen.hip): the 64 x 64 bf16 tile image in LDS, operand fragments as f32x6 / f32x3 pieces, the
// transposed ds_read_tr16_b64 read, the accumulator-entry to row mapping and the transposed epilogues.
// Only what at least two of those files use lives here; a helper of one file stays in that file. qwen.hip
// has 208-B unswizzled rows: it takes the types, the scalar helpers and the bf16 epilogue, not the tile.
#pragma once

#include "vfm_common.h"

namespace vfm {
namespace attn {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int WAVES = 4;
constexpr int TT = 64;           // rows per tile image
constexpr int ROWB = 64 * 2;     // bytes per bf16 row image (head dim 64)
constexpr int IMG = TT * ROWB;   // bytes per tile image

// byte offset of 16-B chunk `ch` (0..7) of row `row` in a [64][64 x bf16] tile image: 128-B rows, the
// chunks XOR-swizzled by (row>>1)&7 so the 32-row ds_read_b128 and the ds_read_b64_tr_b16 are
// conflict-free
__device__ __forceinline__ int kv_off(int row, int ch) { return row * ROWB + 16 * (ch ^ ((row >> 1) & 7)); }

// accumulator entry i (0..15) of a 32 x 32 MFMA block on a lane of wave half hh holds this row of the block
__device__ __forceinline__ constexpr int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// (lo, hi) -> packed bf16 pair, RNE: one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(vfm_f2{lo, hi}, vfm_bf16x2));
}

__device__ __forceinline__ float xchg32(float v) {
    // value of lane l^32 (the other half of the wave)
    return __int_as_float(__shfl_xor(__float_as_int(v), 32));
}

// one operand fragment as its NP bf16 pieces
template <int NP>
struct Frag {
    bf16x8 p[NP];
};

// 8 floats -> NP bf16x8 pieces
template <int NP>
__device__ __forceinline__ Frag<NP> split8(const float* x) {
    uint32_t q[4][NP];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_pieces<NP>(x[2 * j], x[2 * j + 1], q[j]);
    Frag<NP> f;
#pragma unroll
    for (int p = 0; p < NP; ++p) f.p[p] = __builtin_bit_cast(bf16x8, make_uint4(q[0][p], q[1][p], q[2][p], q[3][p]));
    return f;
}

// B-operand fragments (k step s of a 32-row accumulator block): elements 8s .. 8s+7
template <int NP, int S>
__device__ __forceinline__ Frag<NP> split_acc(const f32x16& a) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = a[8 * S + j];
    return split8<NP>(x);
}

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// c += a * b over the piece products (Terms<NP>, smallest first)
template <int NP>
__device__ __forceinline__ f32x16 mfmaN(const Frag<NP>& a, const Frag<NP>& b, f32x16 c) {
#pragma unroll
    for (int t = 0; t < Terms<NP>::N; ++t) c = mfma(a.p[Terms<NP>::a(t)], b.p[Terms<NP>::b(t)], c);
    return c;
}

// the same with the smaller piece products into their own accumulator cs and hi.hi alone into c
// (for the long reductions over keys / queries: full-magnitude roundings as in an fp32 GEMM of
// exact products; cs is added once at the end)
template <int NP>
__device__ __forceinline__ void mfmaN2(const Frag<NP>& a, const Frag<NP>& b, f32x16& c, f32x16& cs) {
#pragma unroll
    for (int t = 0; t < Terms<NP>::N - 1; ++t) cs = mfma(a.p[Terms<NP>::a(t)], b.p[Terms<NP>::b(t)], cs);
    c = mfma(a.p[0], b.p[0], c);
}

// A operand, rows of the tile images (piece p at img + p IMG): row `row`, k = d = 16s + 8hh .. +7
template <int NP>
__device__ __forceinline__ Frag<NP> rd_row(const unsigned char* img, int row, int s, int hh) {
    Frag<NP> f;
#pragma unroll
    for (int p = 0; p < NP; ++p) f.p[p] = *reinterpret_cast<const bf16x8*>(img + p * IMG + kv_off(row, 2 * s + hh));
    return f;
}

// A operand, transposed: rows = d of block db, k = tile rows of 32-row block blk, step s, in the
// k order of an accumulator block used as B operand (split_acc<s>). Lane roles of the two
// ds_read_tr16_b64 (element half e = 0, 1): lane 4 tq + tp of its 16-lane group reads row
// 32 blk + 16 s + 8 e + 4 hh + tq,  d = 32 db + 16 g1 + 4 tp
struct TrLane {
    int g1, tq, tp, hh;
};
// (TrLane of a lane: {(lane >> 4) & 1, (lane >> 2) & 3, lane & 3, lane >> 5}). One image:
__device__ __forceinline__ bf16x8 rd_tr1(const unsigned char* img, const TrLane& t, int blk, int s, int db) {
    const int d = 32 * db + 16 * t.g1 + 4 * t.tp;
    const int r0 = 32 * blk + 16 * s + 4 * t.hh + t.tq;
    const int o0 = kv_off(r0, d >> 3) + 8 * (t.tp & 1);
    const int o1 = kv_off(r0 + 8, d >> 3) + 8 * (t.tp & 1);
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o0));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o1));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}
// the NP pieces (piece p at img + p IMG)
template <int NP>
__device__ __forceinline__ Frag<NP> rd_tr(const unsigned char* img, const TrLane& t, int blk, int s, int db) {
    const int d = 32 * db + 16 * t.g1 + 4 * t.tp;
    const int r0 = 32 * blk + 16 * s + 4 * t.hh + t.tq;
    const int o0 = kv_off(r0, d >> 3) + 8 * (t.tp & 1);
    const int o1 = kv_off(r0 + 8, d >> 3) + 8 * (t.tp & 1);
    Frag<NP> f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + p * IMG + o0));
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + p * IMG + o1));
        f.p[p] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
    }
    return f;
}

// register staging of one 64 x 64 fp32 tile: thread t holds row t>>2, d = 16 (t&3) .. +15
// (zeros for d >= hd or a row that is not there)
struct Stage {
    float4 v[4];
};
template <int NP>
__device__ __forceinline__ void stage_store(const Stage& s, unsigned char* img, int tid) {
    const int r = tid >> 2, q = tid & 3;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float x[8] = {s.v[2 * c].x, s.v[2 * c].y, s.v[2 * c].z, s.v[2 * c].w,
                            s.v[2 * c + 1].x, s.v[2 * c + 1].y, s.v[2 * c + 1].z, s.v[2 * c + 1].w};
        const Frag<NP> f = split8<NP>(x);
#pragma unroll
        for (int p = 0; p < NP; ++p) *reinterpret_cast<bf16x8*>(img + p * IMG + kv_off(r, 2 * q + c)) = f.p[p];
    }
}

// store a transposed accumulator pair (rows d, lane = row of the output): out[row][d] = f * acc, d < hd
__device__ __forceinline__ void store_tr(float* p, const f32x16* acc, int hh, float f, int hd) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
        if (32 * db < hd)
#pragma unroll
        for (int gi = 0; gi < 4; ++gi)
            *reinterpret_cast<float4*>(p + 32 * db + 8 * gi + 4 * hh) =
                make_float4(acc[db][4 * gi] * f, acc[db][4 * gi + 1] * f, acc[db][4 * gi + 2] * f, acc[db][4 * gi + 3] * f);
}
// one 32-row d block of it in bf16, as packed pairs: out[row][d] = bf16(inv * acc), d < nd (a multiple of
// 8). The block is taken by value: read through a pointer to the accumulator array, the packed multiplies
// of the callers come out with their operands commuted
__device__ __forceinline__ void store_tr_bf16(__hip_bfloat16* op, f32x16 acc, int hh, float inv, int nd) {
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
        if (8 * gi >= nd) continue;
        uint2 w;
        w.x = pack_bf16(acc[4 * gi + 0] * inv, acc[4 * gi + 1] * inv);
        w.y = pack_bf16(acc[4 * gi + 2] * inv, acc[4 * gi + 3] * inv);
        *reinterpret_cast<uint2*>(op + 8 * gi + 4 * hh) = w;
    }
}

// ---- host side: [B, N, H, d] views by their element strides (batch, token, head)
struct Strides {
    long long b, n, h;
};
inline Strides mk(const long long* s) { return Strides{s[0], s[1], s[2]}; }
// every stride a multiple of `mult` elements (16-B rows: 4 floats, 8 bf16)
inline bool strides_ok(const long long* s, int mult) {
    if (!s) return false;
    for (int i = 0; i < 3; ++i)
        if (s[i] % mult) return false;
    return true;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace attn
}  // namespace vfm
