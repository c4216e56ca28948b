// Kernels of the frozen Qwen2.5-VL vision tower for gfx950 (networks/utils/vfms/qwen_utils.py).
//
// Reference: HF Qwen2_5_VisionTransformerPretrainedModel under bf16 autocast, as the reference wrapper
// networks/utils/vfms/qwen_utils.py:204-261 runs it. Four ops the other towers' kernels do not cover:
//   * varlen RoPE attention, head dim 80, block-diagonal over a cu_seqlens list (windows / whole images);
//   * RMSNorm rows on a stream of the compute dtype (plain and fused with the residual add);
//   * SwiGLU rows over the padded gate | up GEMM output;
//   * the patch gather: normalised image -> patch rows in window order.
//
// ---- varlen RoPE attention -------------------------------------------------------------------------
// The arithmetic is csrc/attention.hip's, on the helpers of csrc/attn_frag.h: swapped QK^T (S^T = K . Q^T,
// v_mfma_f32_32x32x16_bf16, one query per lane), exp2-domain online softmax in fp32, P rounded to bf16 as the B operand of O^T = V^T . P^T.
// Differences:
//   * head dim 80 = 5 k-steps of 16 for QK^T; the PV product runs over 96 = 3 x 32 output rows, the V tile
//     rows zero-padded from 80 to 96 in LDS (1/6 of the PV MFMAs multiply zeros);
//   * RoPE as q and k are loaded: x cos + rotate_half(x) sin in fp32 (two rounded products and a rounded
//     sum, as torch evaluates it), rounded to bf16 before QK^T. Element d pairs with d +- 40 and the table
//     entries d and d + 40 are equal (the duplicated [T, 80] form), so one item = 8 elements of the low
//     half, their 8 partners of the high half and 8 cos / 8 sin values: each K chunk is read once;
//   * segments: the query tiles are fixed 32-row slices of the packed token axis, NOT per-segment tiles.
//     Every lane owns one query, finds its segment [lo, hi) by a binary search of cu_seqlens (device
//     memory, no host sync, grid = f(T) only) and masks keys outside it. A workgroup stages the key tiles
//     of the union of its queries' segments, starting at the union's first key, and each wave skips the
//     tiles that do not meet its own queries' range. So a 64-token window costs one 64-key tile for each
//     of its two 32-query waves, whatever the workgroup size, and ragged edge windows (4 / 16 / 32
//     tokens) share a tile with their neighbours instead of taking a workgroup each.
//   * workgroup sizes, chosen on the host from the longest segment (a hint, not a condition of correctness):
//     2 waves (64 queries = one full window, its single key tile staged once with all loads in flight
//     together) where the longest segment is <= 64 keys: a larger workgroup over several 64-token windows
//     would stage all their keys for all its waves; 8 waves (256 queries) where segments are >= 512 keys:
//     the K / V / table traffic per query limits the kernel, and a 256-query tile halves it against the
//     4-wave form (1024-key segments: 0.41 ms against 0.68 ms, tools_dev/qwenbench.py); 4 waves (128
//     queries) in between. With 4 or 8 waves the next tile's global loads are in flight during the math. A
//     1-wave form (32 queries, no register prefetch) exists for A/B (VFM_QWEN_ATTN_WAVES).
// Keys outside a query's segment get p = exp2(-inf) = 0 exactly, so they add 0 x v to the output: the
// result does not depend on other segments' (finite) K / V.
#include <stdlib.h>

#include "attn_frag.h"

namespace {

using namespace vfm;
// by name: the tile constants and the swizzled kv_off of attn_frag.h are for 128-B rows, not this file's
using attn::bf16x8; using attn::s16x4; using attn::f32x16; using attn::lds_s16x4; using attn::mfma;
using attn::acc_row; using attn::pack_bf16; using attn::xchg32; using attn::store_tr_bf16;

constexpr int HD = 80;            // head dim
constexpr int HALF = HD / 2;      // rotary pairing distance
constexpr int KT = 64;            // keys per tile
constexpr int ROWB = 208;         // bytes per K / V row in LDS: 96 bf16 (80 + 16 zero pad) + 16 B skew
constexpr int NITEM = KT * 5;     // staging items per tile: (key, low-half chunk c) -> chunks c and c + 5

struct VarlenArgs {
    const __hip_bfloat16* qkv;    // [T, 3, H, 80]
    const float* cos;             // [T, 80]
    const float* sin;             // [T, 80]
    const int* cu;                // [S + 1]
    __hip_bfloat16* o;            // [T, H * 80]
    int T, H, S;
    float c;                      // scale * log2(e)
};

// byte offset of 16-B chunk `ch` (0..12) of key row `key`: unswizzled 208-B rows
__device__ __forceinline__ int kv_off(int key, int ch) { return key * ROWB + 16 * ch; }

__device__ __forceinline__ void unpack8(const uint4& u, float* f) {
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
    f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
    f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
}

// bf16(x cos + sgn * partner * sin) of 8 elements: sgn = -1 for the low half (rotate_half = -x[d + 40]),
// +1 for the high half (x[d - 40]); separately rounded products and sum, as torch's fp32 expression
__device__ __forceinline__ uint4 rope8(const uint4& x, const uint4& partner, const float* cs, const float* sn,
                                       float sgn) {
    float a[8], b[8], r[8];
    unpack8(x, a);
    unpack8(partner, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = __fadd_rn(__fmul_rn(a[i], cs[i]), __fmul_rn(sgn * b[i], sn[i]));
    uint4 o;
    o.x = pack_bf16(r[0], r[1]); o.y = pack_bf16(r[2], r[3]);
    o.z = pack_bf16(r[4], r[5]); o.w = pack_bf16(r[6], r[7]);
    return o;
}

struct Stage {
    uint4 kl, kh, vl, vh;
    float4 c0, c1, s0, s1;
};

template <int NW>
__global__ __launch_bounds__(64 * NW, NW >= 8 ? 1 : 2) void rope_attn_varlen_d80(VarlenArgs a) {
    constexpr int NT = 64 * NW;
    constexpr int QB = 32 * NW;
    constexpr int NIT = (NITEM + NT - 1) / NT;     // staging items per thread
    constexpr bool PF = NW >= 2;                   // a tile's loads all in flight at once, the next tile's during the math
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KT * ROWB];   // K tile | V tile
    __shared__ int wrange[2 * NW];
    unsigned char* ks = lds;
    unsigned char* vs = lds + KT * ROWB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int h = blockIdx.y;
    const int T = a.T, H = a.H;
    const int q_row = blockIdx.x * QB + 32 * wave + r;
    const long long tok = 3LL * H * HD;            // elements per token of the packed projection
    const __hip_bfloat16* qb = a.qkv + (long long)h * HD;
    const __hip_bfloat16* kb = qb + (long long)H * HD;
    const __hip_bfloat16* vb = kb + (long long)H * HD;

    // ---- this lane's query and its segment [lo, hi)
    int lo = 0, hi = 0;
    if (q_row < T && a.S > 0) {
        int s0 = 0, s1 = a.S;                      // largest s in [0, S) with cu[s] <= q_row
        while (s1 - s0 > 1) {
            const int mid = (s0 + s1) >> 1;
            if (a.cu[mid] <= q_row) s0 = mid; else s1 = mid;
        }
        const int c0 = max(a.cu[s0], 0), c1 = min(a.cu[s0 + 1], T);
        if (c0 <= q_row && q_row < c1) { lo = c0; hi = c1; }
    }
    const bool valid = hi > lo;
    int wlo = valid ? lo : 0x7fffffff, whi = valid ? hi : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, off));
        whi = max(whi, __shfl_xor(whi, off));
    }
    if (lane == 0) { wrange[2 * wave] = wlo; wrange[2 * wave + 1] = whi; }
    // zero pad of the V rows (d 80..95), written once: the staging only writes chunks 0..9
    for (int i = tid; i < 2 * KT; i += NT)
        *reinterpret_cast<uint4*>(vs + kv_off(i >> 1, 10 + (i & 1))) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    int glo = 0x7fffffff, ghi = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { glo = min(glo, wrange[2 * w]); ghi = max(ghi, wrange[2 * w + 1]); }
    const int ntile = ghi > glo ? (ghi - glo + KT - 1) / KT : 0;

    // ---- Q^T B-operand fragments with RoPE: lane holds Q[q_row][16 s + 8 hh .. + 7], s = 0..4
    bf16x8 qf[5];
    {
        const int qr = valid ? q_row : 0;
        const __hip_bfloat16* qp = qb + (long long)qr * tok;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int c = 2 * s + hh;              // 16-B chunk 0..9 of the head
            const int cl = c < 5 ? c : c - 5;      // its table chunk
            const int pc = c < 5 ? c + 5 : c - 5;  // partner chunk
            uint4 o = make_uint4(0, 0, 0, 0);
            if (valid) {
                const uint4 x = *reinterpret_cast<const uint4*>(qp + 8 * c);
                const uint4 p = *reinterpret_cast<const uint4*>(qp + 8 * pc);
                float cs[8], sn[8];
                const float* cp = a.cos + (long long)qr * HD + 8 * cl;
                const float* sp = a.sin + (long long)qr * HD + 8 * cl;
                *reinterpret_cast<float4*>(cs) = *reinterpret_cast<const float4*>(cp);
                *reinterpret_cast<float4*>(cs + 4) = *reinterpret_cast<const float4*>(cp + 4);
                *reinterpret_cast<float4*>(sn) = *reinterpret_cast<const float4*>(sp);
                *reinterpret_cast<float4*>(sn + 4) = *reinterpret_cast<const float4*>(sp + 4);
                o = rope8(x, p, cs, sn, c < 5 ? -1.f : 1.f);
            }
            qf[s] = __builtin_bit_cast(bf16x8, o);
        }
    }

    // ---- staging: item it = (key it / 5, chunk c = it % 5) moves K / V chunks c and c + 5 of that key
    auto load_item = [&](int kbase, int it, Stage& st) {
        const int key = kbase + it / 5, c = it % 5;
        if (it < NITEM && key >= 0 && key < T) {
            const __hip_bfloat16* kp = kb + (long long)key * tok + 8 * c;
            const __hip_bfloat16* vp = vb + (long long)key * tok + 8 * c;
            st.kl = *reinterpret_cast<const uint4*>(kp);
            st.kh = *reinterpret_cast<const uint4*>(kp + HALF);
            st.vl = *reinterpret_cast<const uint4*>(vp);
            st.vh = *reinterpret_cast<const uint4*>(vp + HALF);
            const float* cp = a.cos + (long long)key * HD + 8 * c;
            const float* sp = a.sin + (long long)key * HD + 8 * c;
            st.c0 = *reinterpret_cast<const float4*>(cp);
            st.c1 = *reinterpret_cast<const float4*>(cp + 4);
            st.s0 = *reinterpret_cast<const float4*>(sp);
            st.s1 = *reinterpret_cast<const float4*>(sp + 4);
        } else {
            st.kl = st.kh = st.vl = st.vh = make_uint4(0, 0, 0, 0);
            st.c0 = st.c1 = st.s0 = st.s1 = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_item = [&](int it, const Stage& st) {
        if (it >= NITEM) return;
        const int row = it / 5, c = it % 5;
        const float cs[8] = {st.c0.x, st.c0.y, st.c0.z, st.c0.w, st.c1.x, st.c1.y, st.c1.z, st.c1.w};
        const float sn[8] = {st.s0.x, st.s0.y, st.s0.z, st.s0.w, st.s1.x, st.s1.y, st.s1.z, st.s1.w};
        *reinterpret_cast<uint4*>(ks + kv_off(row, c)) = rope8(st.kl, st.kh, cs, sn, -1.f);
        *reinterpret_cast<uint4*>(ks + kv_off(row, c + 5)) = rope8(st.kh, st.kl, cs, sn, 1.f);
        *reinterpret_cast<uint4*>(vs + kv_off(row, c)) = st.vl;
        *reinterpret_cast<uint4*>(vs + kv_off(row, c + 5)) = st.vh;
    };

    // transposed-read lane roles of V (TrLane / rd_tr1 of attn_frag.h, written out here for the 208-B rows:
    // through rd_tr1 with this layout the offset arithmetic compiles to other instructions): lane 4q + p of
    // its 16-lane group reads key 32 kb + 16 s + 8 e + 4 hh + q,  d = 32 db + 16 g1 + 4 p
    const int g1 = (lane >> 4) & 1, tq = (lane >> 2) & 3, tp = lane & 3;

    f32x16 oacc[3];
    oacc[0] = f32x16{};
    oacc[1] = f32x16{};
    oacc[2] = f32x16{};
    float m_run = -INFINITY, l_run = 0.f;
    const float c = a.c;

    Stage pre[PF ? NIT : 1];
    if constexpr (PF) {
        if (ntile > 0) {
#pragma unroll
            for (int u = 0; u < NIT; ++u) load_item(glo, tid + u * NT, pre[u]);
        }
    }
    for (int t = 0; t < ntile; ++t) {
        const int kbase = glo + t * KT;
        if constexpr (PF) {
#pragma unroll
            for (int u = 0; u < NIT; ++u) store_item(tid + u * NT, pre[u]);
        } else {
#pragma unroll 1
            for (int u = 0; u < NIT; ++u) {
                Stage st;
                load_item(kbase, tid + u * NT, st);
                store_item(tid + u * NT, st);
            }
        }
        __syncthreads();
        if constexpr (PF) {
            if (t + 1 < ntile) {
#pragma unroll
                for (int u = 0; u < NIT; ++u) load_item(kbase + KT, tid + u * NT, pre[u]);
            }
        }
        if (whi > kbase && wlo < kbase + KT) {      // wave-uniform: some query of this wave sees this tile
            // ---- S^T = K . Q^T for two 32-key blocks
            f32x16 sacc[2];
#pragma unroll
            for (int kbk = 0; kbk < 2; ++kbk) {
                sacc[kbk] = f32x16{};
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + kv_off(32 * kbk + r, 2 * s + hh));
                    sacc[kbk] = mfma(kf, qf[s], sacc[kbk]);
                }
            }
            // ---- keys outside this lane's segment
            if (!__all(lo <= kbase && hi >= kbase + KT)) {
#pragma unroll
                for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = kbase + 32 * kbk + acc_row(i, hh);
                        if (key < lo || key >= hi) sacc[kbk][i] = -INFINITY;
                    }
            }
            // ---- online softmax (query = this lane's column; keys split over lane and lane^32)
            float mx = sacc[0][0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, sacc[0][i]);
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[1][i]);
            mx = fmaxf(mx, xchg32(mx));
            const float m_new = fmaxf(m_run, mx * c);
            const float m_s = m_new == -INFINITY ? 0.f : m_new;   // no key of this lane yet: p = 0, not NaN
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_s);
            m_run = m_new;
            float ls = 0.f;
            uint32_t pk[2][8];
#pragma unroll
            for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                    const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[kbk][i], c, -m_s));
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[kbk][i + 1], c, -m_s));
                    ls += p0 + p1;
                    pk[kbk][i >> 1] = pack_bf16(p0, p1);
                }
            l_run = l_run * alpha + ls;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                oacc[0][i] *= alpha;
                oacc[1][i] *= alpha;
                oacc[2][i] *= alpha;
            }
            // ---- O^T += V^T . P^T (d blocks 0..2: rows 80..95 of the third are the zero pad)
#pragma unroll
            for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    uint4 pv;
                    pv.x = pk[kbk][4 * s + 0];
                    pv.y = pk[kbk][4 * s + 1];
                    pv.z = pk[kbk][4 * s + 2];
                    pv.w = pk[kbk][4 * s + 3];
                    const bf16x8 pf = __builtin_bit_cast(bf16x8, pv);
#pragma unroll
                    for (int db = 0; db < 3; ++db) {
                        const int d = 32 * db + 16 * g1 + 4 * tp;
                        const int key0 = 32 * kbk + 16 * s + 4 * hh + tq;
                        const int o0 = kv_off(key0, d >> 3) + 8 * (tp & 1);
                        const int o1 = kv_off(key0 + 8, d >> 3) + 8 * (tp & 1);
                        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vs + o0));
                        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vs + o1));
                        const bf16x8 vf =
                            __builtin_bit_cast(bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
                        oacc[db] = mfma(vf, pf, oacc[db]);
                    }
                }
        }
        __syncthreads();
    }

    // ---- epilogue: O[q_row][d] = O^T[d][q_row] / l
    const float l = l_run + xchg32(l_run);
    if (valid && l > 0.f) {
        const float inv = 1.f / l;
        __hip_bfloat16* op = a.o + (long long)q_row * H * HD + (long long)h * HD;
#pragma unroll
        for (int db = 0; db < 3; ++db) store_tr_bf16(op + 32 * db, oacc[db], hh, inv, HD - 32 * db);   // cut at d = 80
    }
}

// ---- RMSNorm rows ------------------------------------------------------------------------------------
// HF Qwen2_5_VLRMSNorm on a stream of dtype T (bf16 under autocast, fp32 otherwise): statistics and the
// normalisation in fp32, one rounding to T at the end. Fused form: h_out = T(h + delta) first, and the norm
// reads that rounded h_out (what the next op of the reference sees). One wave per row, up to 8 float4
// chunks per lane in registers.
struct RmsArgs {
    const void* h;
    const void* delta;    // or null
    void* h_out;          // or null
    const float* w;       // [D]
    void* y;              // or null (residual add only)
    int rows, D;
    float eps;
};

template <class T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<__hip_bfloat16>(float v) {
    return __bfloat162float(__float2bfloat16(v));
}

template <class T>
__device__ __forceinline__ void ld4(const T* p, float* v);
template <>
__device__ __forceinline__ void ld4<__hip_bfloat16>(const __hip_bfloat16* p, float* v) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(u.x << 16);
    v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16);
    v[3] = __uint_as_float(u.y & 0xffff0000u);
}
template <>
__device__ __forceinline__ void ld4<float>(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <class T>
__device__ __forceinline__ void st4(T* p, const float* v);
template <>
__device__ __forceinline__ void st4<__hip_bfloat16>(__hip_bfloat16* p, const float* v) {
    uint2 u;
    u.x = pack_bf16(v[0], v[1]);
    u.y = pack_bf16(v[2], v[3]);
    *reinterpret_cast<uint2*>(p) = u;
}
template <>
__device__ __forceinline__ void st4<float>(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

template <class T, int NCH>
__global__ __launch_bounds__(256) void rms_rows(RmsArgs a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int lane = threadIdx.x & 63;
    const int D = a.D;
    const long long off = (long long)row * D;
    const T* hp = reinterpret_cast<const T*>(a.h) + off;
    float v[NCH][4];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = (j * 64 + lane) * 4;
        if (c0 < D) ld4(hp + c0, v[j]);
        else v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.f;
    }
    if (a.delta) {
        const T* dp = reinterpret_cast<const T*>(a.delta) + off;
        T* op = a.h_out ? reinterpret_cast<T*>(a.h_out) + off : nullptr;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 4;
            if (c0 < D) {
                float d[4];
                ld4(dp + c0, d);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[j][i] = rnd<T>(v[j][i] + d[i]);
                if (op) st4(op + c0, v[j]);
            }
        }
    }
    if (!a.y) return;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) q = fmaf(v[j][i], v[j][i], q);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)D + a.eps);
    T* yp = reinterpret_cast<T*>(a.y) + off;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = (j * 64 + lane) * 4;
        if (c0 < D) {
            const float4 wv = *reinterpret_cast<const float4*>(a.w + c0);
            float o[4];
            o[0] = wv.x * (v[j][0] * rstd);
            o[1] = wv.y * (v[j][1] * rstd);
            o[2] = wv.z * (v[j][2] * rstd);
            o[3] = wv.w * (v[j][3] * rstd);
            st4(yp + c0, o);
        }
    }
}

template <class T>
int rms_dispatch(RmsArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.rows + 3) / 4)), blk(256);
    switch ((a.D + 255) / 256) {
    case 1: VFM_LAUNCH((rms_rows<T, 1>), grid, blk, 0, st, a); break;
    case 2: VFM_LAUNCH((rms_rows<T, 2>), grid, blk, 0, st, a); break;
    case 3: VFM_LAUNCH((rms_rows<T, 3>), grid, blk, 0, st, a); break;
    case 4: VFM_LAUNCH((rms_rows<T, 4>), grid, blk, 0, st, a); break;
    case 5: VFM_LAUNCH((rms_rows<T, 5>), grid, blk, 0, st, a); break;
    case 6: VFM_LAUNCH((rms_rows<T, 6>), grid, blk, 0, st, a); break;
    case 7: VFM_LAUNCH((rms_rows<T, 7>), grid, blk, 0, st, a); break;
    case 8: VFM_LAUNCH((rms_rows<T, 8>), grid, blk, 0, st, a); break;
    default: return VFM_NO_KERNEL;
    }
    return launch_status();
}

// ---- SwiGLU rows: out[t, c] = T(T(silu(g)) * u), g = gu[t, c], u = gu[t, Ip + c]; columns I..Ip zero -----------
template <class T>
__global__ __launch_bounds__(256) void swiglu_rows(const T* __restrict__ gu, T* __restrict__ out, long long groups,
                                                   int I, int Ip) {
    const int gpr = Ip / 4;                       // 4-element groups per row
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups;
         g += (long long)gridDim.x * blockDim.x) {
        const long long row = g / gpr;
        const int c0 = (int)(g - row * gpr) * 4;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (c0 < I) {
            float gv[4], uv[4];
            ld4(gu + row * 2 * Ip + c0, gv);
            ld4(gu + row * 2 * Ip + Ip + c0, uv);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < I) o[i] = rnd<T>(gv[i] / (1.f + __expf(-gv[i]))) * uv[i];
        }
        st4(out + row * Ip + c0, o);
    }
}

// ---- patch gather: out[t, c 196 + i 14 + j] = img[b, c, P py + i, P px + j] for the patch idx[t] = (b gh + py) gw + px;
// columns K..Kp zero ---------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void patch_gather(const float* __restrict__ img, const int* __restrict__ idx,
                                                    T* __restrict__ out, int B, int H, int W, int P, int rows, int K,
                                                    int Kp) {
    const int t = blockIdx.x;
    const int gh = H / P, gw = W / P;
    const int pid = idx[t];
    const bool ok = pid >= 0 && pid < B * gh * gw;
    const int b = ok ? pid / (gh * gw) : 0;
    const int rem = ok ? pid - b * gh * gw : 0;
    const int py = rem / gw, px = rem - py * gw;
    const int PP = P * P;
    for (int k = threadIdx.x; k < Kp; k += blockDim.x) {
        float v = 0.f;
        if (ok && k < K) {
            const int ch = k / PP, r2 = k - ch * PP;
            const int i = r2 / P, j = r2 - i * P;
            v = img[(((long long)b * 3 + ch) * H + (py * P + i)) * W + (px * P + j)];
        }
        st(out + (long long)t * Kp + k, v);
    }
}

}  // namespace

extern "C" int vfm_rope_attention_varlen(const void* qkv, const float* cos, const float* sin, const int* cu_seqlens,
                                         void* o, int T, int H, int head_dim, int S, float scale, int max_seqlen,
                                         void* stream) {
    if (head_dim != HD) return VFM_NO_KERNEL;
    if (!qkv || !cos || !sin || !cu_seqlens || !o || T <= 0 || H <= 0 || H > 65535 || S <= 0) return VFM_ERR_ARGS;
    if (((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)o) % 16) return VFM_ERR_ARGS;
    VarlenArgs a;
    a.qkv = (const __hip_bfloat16*)qkv;
    a.cos = cos;
    a.sin = sin;
    a.cu = cu_seqlens;
    a.o = (__hip_bfloat16*)o;
    a.T = T;
    a.H = H;
    a.S = S;
    a.c = scale * 1.4426950408889634f;
    // waves per workgroup: 2 (64 queries = one full window) where no segment is longer than a key tile; 8 (256
    // queries: half the K / V / table traffic per query of the 4-wave form) where segments hold at least two
    // such workgroups; 4 in between and when the longest segment is unknown. VFM_QWEN_ATTN_WAVES=1|2|4|8 forces
    // one (A/B)
    int nw = max_seqlen <= 0 ? 4 : max_seqlen <= KT ? 2 : max_seqlen >= 512 ? 8 : 4;
    if (const char* e = getenv("VFM_QWEN_ATTN_WAVES")) {
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8) nw = v;
    }
    const dim3 grid((T + 32 * nw - 1) / (32 * nw), H);
    if (nw == 1) VFM_LAUNCH(rope_attn_varlen_d80<1>, grid, dim3(64), 0, (hipStream_t)stream, a);
    else if (nw == 2) VFM_LAUNCH(rope_attn_varlen_d80<2>, grid, dim3(128), 0, (hipStream_t)stream, a);
    else if (nw == 4) VFM_LAUNCH(rope_attn_varlen_d80<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else VFM_LAUNCH(rope_attn_varlen_d80<8>, grid, dim3(512), 0, (hipStream_t)stream, a);
    return launch_status();
}

extern "C" int vfm_rms_norm_rows(const void* h, const void* delta, void* h_out, const float* w, void* y, int dtype,
                                 int rows, int D, float eps, void* stream) {
    if (dtype != VFM_F32 && dtype != VFM_BF16) return VFM_NO_KERNEL;
    if (D <= 0 || D % 4 || D > 2048) return VFM_NO_KERNEL;
    if (!h || rows <= 0 || (y && !w) || (!y && !(delta && h_out))) return VFM_ERR_ARGS;
    const int al = dtype == VFM_F32 ? 16 : 8;
    if (((uintptr_t)h | (uintptr_t)delta | (uintptr_t)h_out | (uintptr_t)y) % al || (uintptr_t)w % 16)
        return VFM_ERR_ARGS;
    RmsArgs a;
    a.h = h; a.delta = delta; a.h_out = h_out; a.w = w; a.y = y;
    a.rows = rows; a.D = D; a.eps = eps;
    if (dtype == VFM_F32) return rms_dispatch<float>(a, (hipStream_t)stream);
    return rms_dispatch<__hip_bfloat16>(a, (hipStream_t)stream);
}

extern "C" int vfm_swiglu_rows(const void* gu, void* out, int dtype, int rows, int I, int Ip, void* stream) {
    if (dtype != VFM_F32 && dtype != VFM_BF16) return VFM_NO_KERNEL;
    if (!gu || !out || rows <= 0 || I <= 0 || Ip < I) return VFM_ERR_ARGS;
    if (Ip % 4) return VFM_NO_KERNEL;
    const int al = dtype == VFM_F32 ? 16 : 8;
    if (((uintptr_t)gu | (uintptr_t)out) % al) return VFM_ERR_ARGS;
    const long long groups = (long long)rows * (Ip / 4);
    const unsigned nb = (unsigned)((groups + 255) / 256 < 65536 * 4 ? (groups + 255) / 256 : 65536 * 4);
    if (dtype == VFM_F32)
        VFM_LAUNCH(swiglu_rows<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)gu, (float*)out,
                   groups, I, Ip);
    else
        VFM_LAUNCH(swiglu_rows<__hip_bfloat16>, dim3(nb), dim3(256), 0, (hipStream_t)stream,
                   (const __hip_bfloat16*)gu, (__hip_bfloat16*)out, groups, I, Ip);
    return launch_status();
}

extern "C" int vfm_patch_gather(const float* img, const int* idx, void* out, int dtype_out, int B, int H, int W,
                                int P, int rows, int K, int Kp, void* stream) {
    if (dtype_out != VFM_F32 && dtype_out != VFM_BF16) return VFM_NO_KERNEL;
    if (!img || !idx || !out || B <= 0 || H <= 0 || W <= 0 || P <= 0 || rows <= 0) return VFM_ERR_ARGS;
    if (H % P || W % P || K != 3 * P * P || Kp < K) return VFM_ERR_ARGS;
    if ((long long)B * 3 * H * W >= (1LL << 31)) return VFM_NO_KERNEL;
    if (dtype_out == VFM_F32)
        VFM_LAUNCH(patch_gather<float>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, img, idx,
                   (float*)out, B, H, W, P, rows, K, Kp);
    else
        VFM_LAUNCH(patch_gather<__hip_bfloat16>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, img, idx,
                   (__hip_bfloat16*)out, B, H, W, P, rows, K, Kp);
    return launch_status();
}
