// Attention over a SHORT key list under a key-padding mask: the SigLIP2 text tower's self-attention
// (bf16, forward only) and the decoder's text cross-attention with its learned null key / value (fp32,
// forward + backward, reference networks/utils/gigagan_utils.py:94-146 CrossAttention.forward).
//
// Neither attention.hip nor attention_f32.hip takes a mask, and their register budgets are tuned; these
// kernels are separate and use that the key list is short (the SigLIP text length is 64, so at most
// 128 keys here): K and V of one (batch, head) are staged in LDS ONCE, all scores of a query live in
// registers at the same time, and the softmax is the plain two-pass one (no streaming loop over key
// tiles, no online rescaling).
//
//   xattn_keymask_fwd (vfm_attention_keymask_fwd): q, k, v, o bf16 [B, N, H, 64] views as vfm_attention_fwd,
//       N <= 128, key_mask uint8 [B, N] (non-zero = attend) or null. fp32 statistics, P rounded to bf16 for
//       P.V, masked keys get probability exactly 0.
//   xattn_fwd / xattn_dq / xattn_dkdv / xattn_combine / xattn_dnull (vfm_cross_attention_f32_*): fp32 with
//       gradients on the fp32-equivalent f32x6 piece products of vfm_common.h (f32x3 opt-in), in the
//       operand layouts of attention_f32.hip. q [B, Nq, H, d] (strided), kv [B, L, 2, H, d] (the to_kv
//       linear's output read in place: all of k before all of v), null_kv [2, H, d], key_mask uint8 [B, L]
//       or null. Key 0 of every (b, h) is the null key / value, keys 1..L the text tokens; L + 1 <= 128,
//       d in {32, 64}.
//
// Validity of key j of sample b:  j == 0: !(key_mask && mask_null);  j >= 1: !key_mask || key_mask[b][j-1].
// mask_null = 0 never masks the null key. mask_null = 1 is what the reference module computes when it
// is given a mask: it prepends a FALSE column to the boolean mask, so the null key takes part only in
// the unmasked call. Every (sample) must keep at least one valid key (the tokenizer always emits EOS);
// a query with none is outside the contract (its outputs are NaN).
//
// Gradients without floating-point atomics: dQ has its own pass (queries on lanes, which also writes
// delta = rowsum(dO . O) into the workspace). dK / dV: keys on lanes, one workgroup per (chunk of
// 64-query tiles, head, sample) holding all <= 128 keys, writing its partial [Nk, 2, d] into the
// workspace; xattn_combine sums the chunks in index order into dkv (rows of masked keys: exact zeros)
// and xattn_dnull sums key 0 over (sample, chunk) in index order. The chunk count depends on the shape
// alone, so two runs agree bit for bit. At the training shape (B = 32, H = 8) there are 256 (b, h)
// pairs for 256 CUs and one chunk: the partial is the result.
//
// Tile images, operand fragments and the transposed reads are those of attn_frag.h, shared with
// attention_f32.hip / attention.hip; only the row-pointer loads and the key-validity bits are this file's.
#include "attn_frag.h"

namespace {

using namespace vfm;
using namespace vfm::attn;

constexpr int HD = 64;
constexpr int RB = 32 * WAVES;   // rows (queries or keys) owned by a workgroup
constexpr int MAXK = 128;        // keys (null key included) a workgroup holds
constexpr int CHUNK_TARGET = 256;   // workgroups the dK / dV pass aims for (a shape-only constant)

struct XArgs {
    const float *q, *kv, *null_kv, *o, *dout;
    const unsigned char* mask;
    float *out, *lse, *delta, *dq, *part;
    Strides sq, so, sdo, sdq;
    int B, H, Nq, L, Nk;   // Nk = L + 1
    int hd;
    int mask_null;
    int tpc;               // 64-query tiles per dK / dV chunk
    float c;               // scale * log2(e)
    float scale;
};

__device__ __forceinline__ bool key_valid(const unsigned char* mask, int mask_null, int L, int b, int j) {
    if (j > L) return false;
    if (!mask) return true;
    if (j == 0) return !mask_null;
    return mask[(long long)b * L + (j - 1)] != 0;
}

// row j of K (which = 0) or V (which = 1) of (b, h): the null row for j == 0, else text token j - 1
__device__ __forceinline__ const float* key_row(const XArgs& a, int b, int h, int j, int which) {
    return j == 0 ? a.null_kv + ((long long)which * a.H + h) * a.hd
                  : a.kv + ((((long long)b * a.L + (j - 1)) * 2 + which) * a.H + h) * a.hd;
}

// load this thread's part of one fp32 row into the register staging (Stage of attn_frag.h); zeros for
// d >= hd or a null row pointer
__device__ __forceinline__ void stage_row(Stage& s, const float* row, int hd, int tid) {
    const int d0 = 16 * (tid & 3);
    if (row && d0 < hd) {
        const float4* p = reinterpret_cast<const float4*>(row + d0);
#pragma unroll
        for (int u = 0; u < 4; ++u) s.v[u] = p[u];
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) s.v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// all keys of (b, h) -> LDS: tile t of K at lds + t NP IMG, of V at lds + (NT + t) NP IMG
template <int NP, int NT>
__device__ __forceinline__ void stage_keys(const XArgs& a, unsigned char* lds, int b, int h, int tid) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = TT * t + (tid >> 2);
        Stage sk, sv;
        stage_row(sk, j < a.Nk ? key_row(a, b, h, j, 0) : nullptr, a.hd, tid);
        stage_row(sv, j < a.Nk ? key_row(a, b, h, j, 1) : nullptr, a.hd, tid);
        stage_store<NP>(sk, lds + t * NP * IMG, tid);
        stage_store<NP>(sv, lds + (NT + t) * NP * IMG, tid);
    }
}

// per-lane operand: one fp32 row (null: zeros), d = 16s + 8hh .. +7 (zero for d >= hd), raw and split
__device__ __forceinline__ void load_raw(const float* row, int hd, int hh, float (*x)[8]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (row && 16 * s < hd) {
            const float4 u = *reinterpret_cast<const float4*>(row + 16 * s + 8 * hh);
            const float4 w = *reinterpret_cast<const float4*>(row + 16 * s + 8 * hh + 4);
            x[s][0] = u.x; x[s][1] = u.y; x[s][2] = u.z; x[s][3] = u.w;
            x[s][4] = w.x; x[s][5] = w.y; x[s][6] = w.z; x[s][7] = w.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[s][j] = 0.f;
        }
    }
}
template <int NP>
__device__ __forceinline__ void load_fixed(const float* row, int hd, int hh, Frag<NP>* f) {
    float x[4][8];
    load_raw(row, hd, hh, x);
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = split8<NP>(x[s]);
}

// validity bits of the keys of tile t (bit = key - 64 t), the same in every wave
__device__ __forceinline__ unsigned long long valid_bits(const unsigned char* mask, int mask_null, int L, int b, int t,
                                                         int lane) {
    return __ballot(key_valid(mask, mask_null, L, b, TT * t + lane));
}
// accumulator entry i of key block kbk holds key 32 kbk + acc_row(i, hh) of its tile; vh = the tile's bits
// already shifted down by 4 hh
__device__ __forceinline__ bool bit_of(unsigned long long vh, int kbk, int i) {
    return (vh >> (32 * kbk + acc_row(i, 0))) & 1ull;
}

// ---------------------------------------------------------------------------------------------
// forward: workgroup = 4 waves x 32 queries of one (b, h); queries on lanes (S^T = K Q^T)
template <int NP, int NT>
__global__ __launch_bounds__(64 * WAVES) void xattn_fwd(XArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int Nq = a.Nq, Nk = a.Nk, hd = a.hd;
    const int q_row = blockIdx.x * RB + 32 * wave + r;
    const TrLane tl{(lane >> 4) & 1, (lane >> 2) & 3, lane & 3, hh};

    unsigned long long vh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) vh[t] = valid_bits(a.mask, a.mask_null, a.L, b, t, lane) >> (4 * hh);
    Frag<NP> qf[4];
    load_fixed<NP>(q_row < Nq ? a.q + (long long)b * a.sq.b + (long long)q_row * a.sq.n + (long long)h * a.sq.h : nullptr,
                   hd, hh, qf);
    stage_keys<NP, NT>(a, lds, b, h, tid);
    __syncthreads();

    f32x16 sacc[2 * NT];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk) {
            f32x16 s = f32x16{};
            if (TT * t + 32 * kbk < Nk) {
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    if (16 * st < hd) s = mfmaN<NP>(rd_row<NP>(lds + t * NP * IMG, 32 * kbk + r, st, hh), qf[st], s);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = bit_of(vh[t], kbk, i) ? s[i] : -INFINITY;
                mx = fmaxf(mx, s[i]);
            }
            sacc[2 * t + kbk] = s;
        }
    mx = fmaxf(mx, xchg32(mx));
    const float c = a.c;
    const float m = mx * c;
    float ls = 0.f;
#pragma unroll
    for (int u = 0; u < 2 * NT; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float p = __builtin_amdgcn_exp2f(fmaf(sacc[u][i], c, -m));
            sacc[u][i] = p;
            ls += p;
        }
    f32x16 oacc[2] = {f32x16{}, f32x16{}}, oaccs[2] = {f32x16{}, f32x16{}};
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
            if (TT * t + 32 * kbk < Nk) {
                const Frag<NP> pf[2] = {split_acc<NP, 0>(sacc[2 * t + kbk]), split_acc<NP, 1>(sacc[2 * t + kbk])};
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int db = 0; db < 2; ++db)
                        if (32 * db < hd)
                            mfmaN2<NP>(rd_tr<NP>(lds + (NT + t) * NP * IMG, tl, kbk, st, db), pf[st], oacc[db], oaccs[db]);
            }
    oacc[0] += oaccs[0];
    oacc[1] += oaccs[1];
    const float l = ls + xchg32(ls);
    if (q_row < Nq) {
        store_tr(a.out + (long long)b * a.so.b + (long long)q_row * a.so.n + (long long)h * a.so.h, oacc, hh, 1.f / l, hd);
        if (hh == 0) a.lse[((long long)b * a.H + h) * Nq + q_row] = m + __log2f(l);
    }
}

// ---------------------------------------------------------------------------------------------
// dQ (and delta): queries on lanes; P^T recomputed from lse, dP^T = V dO^T, dS^T = P^T (dP^T - delta),
// dQ^T += K^T dS^T
template <int NP, int NT>
__global__ __launch_bounds__(64 * WAVES) void xattn_dq(XArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int Nq = a.Nq, Nk = a.Nk, hd = a.hd;
    const int q_row = blockIdx.x * RB + 32 * wave + r;
    const bool ok = q_row < Nq;
    const TrLane tl{(lane >> 4) & 1, (lane >> 2) & 3, lane & 3, hh};

    unsigned long long vh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) vh[t] = valid_bits(a.mask, a.mask_null, a.L, b, t, lane) >> (4 * hh);
    Frag<NP> qf[4], of[4];
    load_fixed<NP>(ok ? a.q + (long long)b * a.sq.b + (long long)q_row * a.sq.n + (long long)h * a.sq.h : nullptr, hd, hh,
                   qf);
    const long long rix = ((long long)b * a.H + h) * Nq + (ok ? q_row : 0);
    float dlt = 0.f;
    {
        float xo[4][8], xd[4][8];
        load_raw(ok ? a.o + (long long)b * a.so.b + (long long)q_row * a.so.n + (long long)h * a.so.h : nullptr, hd, hh, xo);
        load_raw(ok ? a.dout + (long long)b * a.sdo.b + (long long)q_row * a.sdo.n + (long long)h * a.sdo.h : nullptr, hd,
                 hh, xd);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) dlt = fmaf(xo[s][j], xd[s][j], dlt);
            of[s] = split8<NP>(xd[s]);
        }
        dlt += xchg32(dlt);
        if (ok && hh == 0) a.delta[rix] = dlt;
    }
    const float lse = ok ? a.lse[rix] : INFINITY;
    stage_keys<NP, NT>(a, lds, b, h, tid);
    __syncthreads();

    f32x16 dq[2] = {f32x16{}, f32x16{}}, dqs[2] = {f32x16{}, f32x16{}};
    const float c = a.c;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
            if (TT * t + 32 * kbk < Nk) {
                const unsigned char* kimg = lds + t * NP * IMG;
                const unsigned char* vimg = lds + (NT + t) * NP * IMG;
                f32x16 s = f32x16{}, dp = f32x16{};
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    if (16 * st < hd) {
                        s = mfmaN<NP>(rd_row<NP>(kimg, 32 * kbk + r, st, hh), qf[st], s);
                        dp = mfmaN<NP>(rd_row<NP>(vimg, 32 * kbk + r, st, hh), of[st], dp);
                    }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = bit_of(vh[t], kbk, i) ? __builtin_amdgcn_exp2f(fmaf(s[i], c, -lse)) : 0.f;
                    s[i] = p * (dp[i] - dlt);
                }
                const Frag<NP> df[2] = {split_acc<NP, 0>(s), split_acc<NP, 1>(s)};
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int db = 0; db < 2; ++db)
                        if (32 * db < hd) mfmaN2<NP>(rd_tr<NP>(kimg, tl, kbk, st, db), df[st], dq[db], dqs[db]);
            }
    dq[0] += dqs[0];
    dq[1] += dqs[1];
    if (ok)
        store_tr(a.dq + (long long)b * a.sdq.b + (long long)q_row * a.sdq.n + (long long)h * a.sdq.h, dq, hh, a.scale, hd);
}

// ---------------------------------------------------------------------------------------------
// dK / dV partials: keys on lanes (wave w owns keys 32 w .. +31 of the <= 128), Q / dO streamed in
// 64-query tiles of this workgroup's chunk; S = Q K^T, P, dP = dO V^T, dS, dV^T += dO^T P, dK^T += Q^T dS
template <int NP>
__global__ __launch_bounds__(64 * WAVES) void xattn_dkdv(XArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * NP * IMG + 2 * TT * 4];
    unsigned char *qimg = lds, *oimg = lds + NP * IMG;
    float* lse_s = reinterpret_cast<float*>(lds + 2 * NP * IMG);
    float* dlt_s = lse_s + TT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int Nq = a.Nq, Nk = a.Nk, hd = a.hd;
    const int key = 32 * wave + r;
    const bool active = 32 * wave < Nk;          // wave-uniform: this wave owns at least one key
    const bool valid = key_valid(a.mask, a.mask_null, a.L, b, key);
    const TrLane tl{(lane >> 4) & 1, (lane >> 2) & 3, lane & 3, hh};

    const float* qb = a.q + (long long)b * a.sq.b + (long long)h * a.sq.h;
    const float* ob = a.dout + (long long)b * a.sdo.b + (long long)h * a.sdo.h;
    const float* lb = a.lse + ((long long)b * a.H + h) * Nq;
    const float* db_ = a.delta + ((long long)b * a.H + h) * Nq;
    Frag<NP> kf[4], vf[4];
    load_fixed<NP>(key < Nk ? key_row(a, b, h, key, 0) : nullptr, hd, hh, kf);
    load_fixed<NP>(key < Nk ? key_row(a, b, h, key, 1) : nullptr, hd, hh, vf);

    f32x16 dk[2] = {f32x16{}, f32x16{}}, dv[2] = {f32x16{}, f32x16{}};
    const float c = a.c;
    const int T = (Nq + TT - 1) / TT;
    const int t0 = chunk * a.tpc, t1 = min(T, t0 + a.tpc);
    for (int t = t0; t < t1; ++t) {
        const int q0 = t * TT, qr = q0 + (tid >> 2);
        Stage sq, so;
        stage_row(sq, qr < Nq ? qb + (long long)qr * a.sq.n : nullptr, hd, tid);
        stage_row(so, qr < Nq ? ob + (long long)qr * a.sdo.n : nullptr, hd, tid);
        stage_store<NP>(sq, qimg, tid);
        stage_store<NP>(so, oimg, tid);
        if (tid < TT) {
            const bool ok = q0 + tid < Nq;
            lse_s[tid] = ok ? lb[q0 + tid] : INFINITY;
            dlt_s[tid] = ok ? db_[q0 + tid] : 0.f;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int qbk = 0; qbk < 2; ++qbk) {
                f32x16 s = f32x16{}, dp = f32x16{};
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    if (16 * st < hd) {
                        s = mfmaN<NP>(rd_row<NP>(qimg, 32 * qbk + r, st, hh), kf[st], s);
                        dp = mfmaN<NP>(rd_row<NP>(oimg, 32 * qbk + r, st, hh), vf[st], dp);
                    }
                // rows of this lane's accumulator entries: 32 qbk + 8 gi + 4 hh + (0..3)
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) {
                    const float4 Lq = *reinterpret_cast<const float4*>(lse_s + 32 * qbk + 8 * gi + 4 * hh);
                    const float4 Dq = *reinterpret_cast<const float4*>(dlt_s + 32 * qbk + 8 * gi + 4 * hh);
                    const float Ls[4] = {Lq.x, Lq.y, Lq.z, Lq.w}, Ds[4] = {Dq.x, Dq.y, Dq.z, Dq.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 4 * gi + j;
                        const float p = valid ? __builtin_amdgcn_exp2f(fmaf(s[i], c, -Ls[j])) : 0.f;
                        s[i] = p;
                        dp[i] = p * (dp[i] - Ds[j]);
                    }
                }
                {
                    const Frag<NP> pf[2] = {split_acc<NP, 0>(s), split_acc<NP, 1>(s)};
#pragma unroll
                    for (int st = 0; st < 2; ++st)
#pragma unroll
                        for (int d = 0; d < 2; ++d)
                            if (32 * d < hd) dv[d] = mfmaN<NP>(rd_tr<NP>(oimg, tl, qbk, st, d), pf[st], dv[d]);
                }
                const Frag<NP> df[2] = {split_acc<NP, 0>(dp), split_acc<NP, 1>(dp)};
#pragma unroll
                for (int st = 0; st < 2; ++st)
#pragma unroll
                    for (int d = 0; d < 2; ++d)
                        if (32 * d < hd) dk[d] = mfmaN<NP>(rd_tr<NP>(qimg, tl, qbk, st, d), df[st], dk[d]);
            }
        }
        __syncthreads();
    }
    if (key < Nk) {
        float* p = a.part + (((((long long)chunk * a.B + b) * a.H + h) * Nk + key) * 2) * hd;
        store_tr(p, dk, hh, a.scale, hd);
        store_tr(p + hd, dv, hh, 1.f, hd);
    }
}

// dkv[b, l, w, h, :] = sum over chunks (index order) of part[chunk, b, h, l + 1, w, :]; masked keys: zeros.
// One thread per float4.
__global__ __launch_bounds__(256) void xattn_combine(XArgs a, float* dkv, int chunks, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int d4n = a.hd / 4;
    long long x = idx;
    const int d4 = (int)(x % d4n); x /= d4n;
    const int h = (int)(x % a.H); x /= a.H;
    const int w = (int)(x % 2); x /= 2;
    const int l = (int)(x % a.L);
    const int b = (int)(x / a.L);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (key_valid(a.mask, a.mask_null, a.L, b, l + 1)) {
        for (int ch = 0; ch < chunks; ++ch) {
            const float4 v = *reinterpret_cast<const float4*>(
                a.part + ((((((long long)ch * a.B + b) * a.H + h) * a.Nk + (l + 1)) * 2 + w) * a.hd + 4 * d4));
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    *reinterpret_cast<float4*>(dkv + idx * 4) = s;
}

// dnull[w, h, :] = sum over samples, then chunks (index order) of part[chunk, b, h, 0, w, :]
__global__ __launch_bounds__(256) void xattn_dnull(XArgs a, float* dnull, int chunks, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int d4n = a.hd / 4;
    const int d4 = idx % d4n, h = (idx / d4n) % a.H, w = idx / (d4n * a.H);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(a.mask && a.mask_null)) {
        for (int b = 0; b < a.B; ++b)
            for (int ch = 0; ch < chunks; ++ch) {
                const float4 v = *reinterpret_cast<const float4*>(
                    a.part + ((((((long long)ch * a.B + b) * a.H + h) * a.Nk + 0) * 2 + w) * a.hd + 4 * d4));
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
    }
    *reinterpret_cast<float4*>(dnull + (long long)idx * 4) = s;
}

// ---------------------------------------------------------------------------------------------
// bf16 self-attention forward under a key mask: attention.hip's layouts with all N <= 128 keys in LDS
struct KmArgs {
    const __hip_bfloat16 *q, *k, *v;
    __hip_bfloat16* o;
    const unsigned char* mask;
    Strides sq, sk, sv, so;
    int N, H;
    float c;
};

template <int NT>
__global__ __launch_bounds__(64 * WAVES) void xattn_keymask_fwd(KmArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * NT * IMG];   // K tiles | V tiles
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int N = a.N;
    const int q_row = 32 * wave + r;
    const TrLane tl{(lane >> 4) & 1, (lane >> 2) & 3, lane & 3, hh};

    const __hip_bfloat16* qb = a.q + (long long)b * a.sq.b + (long long)h * a.sq.h;
    const __hip_bfloat16* kb = a.k + (long long)b * a.sk.b + (long long)h * a.sk.h;
    const __hip_bfloat16* vb = a.v + (long long)b * a.sv.b + (long long)h * a.sv.h;

    unsigned long long vh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = TT * t + lane;
        vh[t] = __ballot(j < N && (!a.mask || a.mask[(long long)b * N + j] != 0)) >> (4 * hh);
    }
    bf16x8 qf[4];
    {
        const bool ok = q_row < N;
        const __hip_bfloat16* qp = qb + (long long)(ok ? q_row : 0) * a.sq.n + 8 * hh;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            qf[s] = __builtin_bit_cast(bf16x8, ok ? *reinterpret_cast<const uint4*>(qp + 16 * s) : make_uint4(0, 0, 0, 0));
    }
    // staging: thread t moves chunks t and t + 256 of each 64 x 8-chunk tile
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = (tid >> 3) + 32 * u, ch = tid & 7, key = TT * t + row;
            uint4 kx = make_uint4(0, 0, 0, 0), vx = make_uint4(0, 0, 0, 0);
            if (key < N) {
                kx = *reinterpret_cast<const uint4*>(kb + (long long)key * a.sk.n + 8 * ch);
                vx = *reinterpret_cast<const uint4*>(vb + (long long)key * a.sv.n + 8 * ch);
            }
            *reinterpret_cast<uint4*>(lds + t * IMG + kv_off(row, ch)) = kx;
            *reinterpret_cast<uint4*>(lds + (NT + t) * IMG + kv_off(row, ch)) = vx;
        }
    __syncthreads();

    f32x16 sacc[2 * NT];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk) {
            f32x16 s = f32x16{};
            if (TT * t + 32 * kbk < N) {
#pragma unroll
                for (int st = 0; st < 4; ++st)
                    s = mfma(*reinterpret_cast<const bf16x8*>(lds + t * IMG + kv_off(32 * kbk + r, 2 * st + hh)), qf[st], s);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = bit_of(vh[t], kbk, i) ? s[i] : -INFINITY;
                mx = fmaxf(mx, s[i]);
            }
            sacc[2 * t + kbk] = s;
        }
    mx = fmaxf(mx, xchg32(mx));
    const float c = a.c, m = mx * c;
    float ls = 0.f;
    f32x16 oacc[2] = {f32x16{}, f32x16{}};
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk) {
            uint32_t pk[8];
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[2 * t + kbk][i], c, -m));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[2 * t + kbk][i + 1], c, -m));
                ls += p0 + p1;
                pk[i >> 1] = pack_bf16(p0, p1);
            }
            if (TT * t + 32 * kbk < N) {
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const bf16x8 pf =
                        __builtin_bit_cast(bf16x8, make_uint4(pk[4 * st], pk[4 * st + 1], pk[4 * st + 2], pk[4 * st + 3]));
#pragma unroll
                    for (int db = 0; db < 2; ++db) oacc[db] = mfma(rd_tr1(lds + (NT + t) * IMG, tl, kbk, st, db), pf, oacc[db]);
                }
            }
        }
    const float l = ls + xchg32(ls);
    if (q_row < N) {
        const float inv = 1.f / l;
        __hip_bfloat16* op = a.o + (long long)b * a.so.b + (long long)q_row * a.so.n + (long long)h * a.so.h;
#pragma unroll
        for (int db = 0; db < 2; ++db) store_tr_bf16(op + 32 * db, oacc[db], hh, inv, HD - 32 * db);
    }
}

// ---------------------------------------------------------------------------------------------
// grid limits (B, H on grid y / z) and index arithmetic in int (Nq + tile, L + 1)
bool dims_ok(int B, int H, int Nq, int L) {
    return B > 0 && H > 0 && Nq > 0 && L > 0 && B <= 65535 && H <= 65535 && Nq <= (1 << 30) && L <= (1 << 30);
}

int check_shape(int B, int H, int Nq, int L, int head_dim, int precision) {
    if (head_dim != HD && head_dim != 32) return VFM_NO_KERNEL;
    if (precision != VFM_F32 && precision != VFM_F32X3) return VFM_ERR_ARGS;
    if (!dims_ok(B, H, Nq, L)) return VFM_ERR_ARGS;
    if (L + 1 > MAXK) return VFM_NO_KERNEL;
    return VFM_OK;
}

// 64-query tiles per dK / dV workgroup and the number of such chunks: enough chunks for ~CHUNK_TARGET
// workgroups, a function of the shape alone
void plan_chunks(int B, int H, int Nq, int* tpc, int* chunks) {
    const long long T = (Nq + TT - 1) / TT, bh = (long long)B * H;
    long long want = (CHUNK_TARGET + bh - 1) / bh;
    if (want < 1) want = 1;
    if (want > T) want = T;
    *tpc = (int)((T + want - 1) / want);
    *chunks = (int)((T + *tpc - 1) / *tpc);
}
long long delta_floats(int B, int H, int Nq) { return (((long long)B * H * Nq + 3) / 4) * 4; }

// dynamic LDS above 64 KB needs the attribute once per device and kernel instantiation
#define XA_LAUNCH(kern, grid, ldsb, st, a)                                                                    \
    do {                                                                                                      \
        static bool attr_[MAXDEV] = {};                                                                       \
        const int dv_ = cur_dev();                                                                            \
        if (!attr_[dv_]) {                                                                                    \
            (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(ldsb)); \
            attr_[dv_] = true;                                                                                \
        }                                                                                                     \
        VFM_LAUNCH(kern, grid, dim3(64 * WAVES), ldsb, st, a);                                                \
    } while (0)

}  // namespace

extern "C" int vfm_attention_keymask_fwd(const void* q, const void* k, const void* v, const void* key_mask, void* o,
                                         int B, int H, int N, int head_dim, const long long* sq, const long long* sk,
                                         const long long* sv, const long long* so, float scale, void* stream) {
    if (head_dim != HD) return VFM_NO_KERNEL;
    if (B <= 0 || H <= 0 || N <= 0 || B > 65535 || H > 65535) return VFM_ERR_ARGS;
    if (N > MAXK) return VFM_NO_KERNEL;
    if (!q || !k || !v || !o) return VFM_ERR_ARGS;
    // 16-B vector loads of 8 bf16: every row start must be 16-B aligned (unit stride along d)
    if (!strides_ok(sq, 8) || !strides_ok(sk, 8) || !strides_ok(sv, 8) || !strides_ok(so, 8)) return VFM_ERR_ARGS;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o)) return VFM_ERR_ARGS;
    KmArgs a{};
    a.q = (const __hip_bfloat16*)q; a.k = (const __hip_bfloat16*)k; a.v = (const __hip_bfloat16*)v;
    a.o = (__hip_bfloat16*)o;
    a.mask = (const unsigned char*)key_mask;
    a.sq = mk(sq); a.sk = mk(sk); a.sv = mk(sv); a.so = mk(so);
    a.N = N; a.H = H;
    a.c = scale * 1.4426950408889634f;
    const dim3 grid(1, H, B);
    if (N <= TT) VFM_LAUNCH(xattn_keymask_fwd<1>, grid, dim3(64 * WAVES), 0, (hipStream_t)stream, a);
    else VFM_LAUNCH(xattn_keymask_fwd<2>, grid, dim3(64 * WAVES), 0, (hipStream_t)stream, a);
    return launch_status();
}

extern "C" long long vfm_cross_attention_f32_workspace_floats(int B, int H, int Nq, int L, int head_dim) {
    if (!dims_ok(B, H, Nq, L)) return VFM_ERR_ARGS;
    if ((head_dim != HD && head_dim != 32) || L + 1 > MAXK) return VFM_NO_KERNEL;
    int tpc, chunks;
    plan_chunks(B, H, Nq, &tpc, &chunks);
    return delta_floats(B, H, Nq) + (long long)chunks * B * H * (L + 1) * 2 * head_dim;
}

extern "C" int vfm_cross_attention_f32_fwd(const void* q, const void* kv, const void* null_kv, const void* key_mask,
                                           void* o, void* lse, int B, int H, int Nq, int L, int head_dim,
                                           const long long* sq, const long long* so, float scale, int mask_null,
                                           int precision, void* stream) {
    int rc = check_shape(B, H, Nq, L, head_dim, precision);
    if (rc != VFM_OK) return rc;
    if (!q || !kv || !null_kv || !o || !lse) return VFM_ERR_ARGS;
    if (!strides_ok(sq, 4) || !strides_ok(so, 4)) return VFM_ERR_ARGS;
    if (!aligned16(q) || !aligned16(kv) || !aligned16(null_kv) || !aligned16(o)) return VFM_ERR_ARGS;
    XArgs a{};
    a.q = (const float*)q; a.kv = (const float*)kv; a.null_kv = (const float*)null_kv;
    a.mask = (const unsigned char*)key_mask;
    a.out = (float*)o; a.lse = (float*)lse;
    a.sq = mk(sq); a.so = mk(so);
    a.B = B; a.H = H; a.Nq = Nq; a.L = L; a.Nk = L + 1; a.hd = head_dim;
    a.mask_null = mask_null != 0;
    a.scale = scale;
    a.c = scale * 1.4426950408889634f;
    const dim3 grid((Nq + RB - 1) / RB, H, B);
    hipStream_t st = (hipStream_t)stream;
    const int nt = a.Nk <= TT ? 1 : 2;
    if (precision == VFM_F32) {
        if (nt == 1) XA_LAUNCH((xattn_fwd<3, 1>), grid, 2 * 1 * 3 * IMG, st, a);
        else XA_LAUNCH((xattn_fwd<3, 2>), grid, 2 * 2 * 3 * IMG, st, a);
    } else {
        if (nt == 1) XA_LAUNCH((xattn_fwd<2, 1>), grid, 2 * 1 * 2 * IMG, st, a);
        else XA_LAUNCH((xattn_fwd<2, 2>), grid, 2 * 2 * 2 * IMG, st, a);
    }
    return launch_status();
}

extern "C" int vfm_cross_attention_f32_bwd(const void* q, const void* kv, const void* null_kv, const void* key_mask,
                                           const void* o, const void* dout, const void* lse, void* workspace, void* dq,
                                           void* dkv, void* dnull, int B, int H, int Nq, int L, int head_dim,
                                           const long long* sq, const long long* so, const long long* sdo,
                                           const long long* sdq, float scale, int mask_null, int precision,
                                           void* stream) {
    int rc = check_shape(B, H, Nq, L, head_dim, precision);
    if (rc != VFM_OK) return rc;
    if (!q || !kv || !null_kv || !o || !dout || !lse || !workspace || !dq || !dkv || !dnull) return VFM_ERR_ARGS;
    const long long* ss[4] = {sq, so, sdo, sdq};
    for (const long long* s : ss)
        if (!strides_ok(s, 4)) return VFM_ERR_ARGS;
    const void* ps[9] = {q, kv, null_kv, o, dout, workspace, dq, dkv, dnull};
    for (const void* p : ps)
        if (!aligned16(p)) return VFM_ERR_ARGS;
    XArgs a{};
    a.q = (const float*)q; a.kv = (const float*)kv; a.null_kv = (const float*)null_kv;
    a.mask = (const unsigned char*)key_mask;
    a.o = (const float*)o; a.dout = (const float*)dout; a.lse = (float*)lse;
    a.delta = (float*)workspace;
    a.part = (float*)workspace + delta_floats(B, H, Nq);
    a.dq = (float*)dq;
    a.sq = mk(sq); a.so = mk(so); a.sdo = mk(sdo); a.sdq = mk(sdq);
    a.B = B; a.H = H; a.Nq = Nq; a.L = L; a.Nk = L + 1; a.hd = head_dim;
    a.mask_null = mask_null != 0;
    a.scale = scale;
    a.c = scale * 1.4426950408889634f;
    int chunks;
    plan_chunks(B, H, Nq, &a.tpc, &chunks);
    hipStream_t st = (hipStream_t)stream;
    const dim3 gq((Nq + RB - 1) / RB, H, B), gk(chunks, H, B);
    const int nt = a.Nk <= TT ? 1 : 2;
    if (precision == VFM_F32) {
        if (nt == 1) XA_LAUNCH((xattn_dq<3, 1>), gq, 2 * 1 * 3 * IMG, st, a);
        else XA_LAUNCH((xattn_dq<3, 2>), gq, 2 * 2 * 3 * IMG, st, a);
        VFM_LAUNCH(xattn_dkdv<3>, gk, dim3(64 * WAVES), 0, st, a);
    } else {
        if (nt == 1) XA_LAUNCH((xattn_dq<2, 1>), gq, 2 * 1 * 2 * IMG, st, a);
        else XA_LAUNCH((xattn_dq<2, 2>), gq, 2 * 2 * 2 * IMG, st, a);
        VFM_LAUNCH(xattn_dkdv<2>, gk, dim3(64 * WAVES), 0, st, a);
    }
    const long long total = (long long)B * L * 2 * H * (head_dim / 4);
    VFM_LAUNCH(xattn_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, (float*)dkv, chunks, total);
    const int ntot = 2 * H * (head_dim / 4);
    VFM_LAUNCH(xattn_dnull, dim3((ntot + 255) / 256), dim3(256), 0, st, a, (float*)dnull, chunks, ntot);
    return launch_status();
}
