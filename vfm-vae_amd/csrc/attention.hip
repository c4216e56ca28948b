// Fused multi-head self-attention forward (flash-style), bf16 in/out, fp32 softmax.
//
// Replaces `F.scaled_dot_product_attention(q, k, v)` inside the frozen ViT towers
// (HF SiglipAttention under bf16 autocast, reference networks/utils/vfms/siglip2_utils.py:121;
// DINOv2 / CLIP towers of configs 0 and 3): O = softmax(Q K^T * scale) V per (batch, head),
// head dim 64, any token count N, no mask, no dropout. Forward only: the towers run frozen
// under no_grad.
//
// Layout: Q, K, V, O are [B, N, H, 64] views with element strides (batch, token, head) and
// unit stride along the head dim. The SigLIP tower passes its packed
// qkv GEMM output [B, N, 3, H, 64] directly (stride_n = 3*H*64), so no q/k/v split or
// transpose copies are made, and O lands in the [B, N, H*64] layout the output projection
// reads.
//
// Structure (MI355X_MICROARCH.md / cdna_hip_programming.md App. B "Fused attention prefill"):
//   * workgroup = 4 waves = 128 query rows of one (b, h); wave = 32 query rows;
//   * per 64-key tile, K and V are staged in LDS (128-B rows, 16-B chunks XOR-swizzled by
//     (key>>1)&7 so the 32-row ds_read_b128 of K and the ds_read_b64_tr_b16 of V are
//     conflict-free), the next tile's global loads issued before the current tile's math
//     (register staging, written to LDS after the barrier);
//   * swapped QK^T: S^T = K . Q^T with v_mfma_f32_32x32x16_bf16 puts one query per lane
//     (column) and its keys in the 16 accumulator registers, so the row max / row sum are
//     lane-local plus one exchange with lane^32;
//   * O^T = V^T . P^T: the bf16-converted S^T registers ARE the B operand (accumulator-as-
//     operand, k order permuted to match), V^T fragments come from transposed LDS reads, and
//     the online-softmax rescale of O^T is lane-local (query on the lane);
//   * exp2 domain: t = s * scale * log2(e); p = exp2(t - m); l summed from fp32 p, P rounded
//     to bf16 for the PV product (as flash attention on the reference's GPUs).
#include "attn_frag.h"

namespace {

using namespace vfm;
using namespace vfm::attn;

constexpr int HD = 64;        // head dim
constexpr int QB = 32 * WAVES;  // query rows per workgroup
constexpr int KT = TT;        // keys per tile

struct AttnArgs {
    const __hip_bfloat16* q;
    const __hip_bfloat16* k;
    const __hip_bfloat16* v;
    __hip_bfloat16* o;
    Strides sq, sk, sv, so;
    int N, H;
    float c;  // scale * log2(e)
};

__global__ __launch_bounds__(64 * WAVES, 2) void attn_fwd_d64(AttnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KT * ROWB];  // K tile | V tile
    unsigned char* ks = lds;
    unsigned char* vs = lds + KT * ROWB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int N = a.N;
    const int q_row = blockIdx.x * QB + 32 * wave + r;

    const __hip_bfloat16* qb = a.q + (long long)b * a.sq.b + (long long)h * a.sq.h;
    const __hip_bfloat16* kb = a.k + (long long)b * a.sk.b + (long long)h * a.sk.h;
    const __hip_bfloat16* vb = a.v + (long long)b * a.sv.b + (long long)h * a.sv.h;

    // Q^T B-operand fragments: lane holds Q[q_row][16s + 8hh .. +7], s = 0..3
    bf16x8 qf[4];
    {
        const bool ok = q_row < N;
        const __hip_bfloat16* qp = qb + (long long)(ok ? q_row : 0) * a.sq.n + 8 * hh;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 v4 = ok ? *reinterpret_cast<const uint4*>(qp + 16 * s) : make_uint4(0, 0, 0, 0);
            qf[s] = __builtin_bit_cast(bf16x8, v4);
        }
    }

    // staging: thread t moves chunks t and t+256 of each 64 x 8-chunk tile
    const int st_key0 = tid >> 3, st_ch = tid & 7;
    uint4 kreg[2], vreg[2];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int key = t * KT + st_key0 + 32 * u;
            if (key < N) {
                kreg[u] = *reinterpret_cast<const uint4*>(kb + (long long)key * a.sk.n + 8 * st_ch);
                vreg[u] = *reinterpret_cast<const uint4*>(vb + (long long)key * a.sv.n + 8 * st_ch);
            } else {
                kreg[u] = make_uint4(0, 0, 0, 0);
                vreg[u] = make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int off = kv_off(st_key0 + 32 * u, st_ch);
            *reinterpret_cast<uint4*>(ks + off) = kreg[u];
            *reinterpret_cast<uint4*>(vs + off) = vreg[u];
        }
    };

    const TrLane tl{(lane >> 4) & 1, (lane >> 2) & 3, lane & 3, hh};   // transposed-read lane roles of V

    f32x16 oacc[2];
    oacc[0] = f32x16{};
    oacc[1] = f32x16{};
    float m_run = -INFINITY, l_run = 0.f;
    const float c = a.c;

    const int T = (N + KT - 1) / KT;
    load_tile(0);
    for (int t = 0; t < T; ++t) {
        store_tile();
        __syncthreads();
        if (t + 1 < T) load_tile(t + 1);

        // ---- S^T = K . Q^T for two 32-key blocks
        f32x16 sacc[2];
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk) {
            sacc[kbk] = f32x16{};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + kv_off(32 * kbk + r, 2 * s + hh));
                sacc[kbk] = mfma(kf, qf[s], sacc[kbk]);
            }
        }
        // ---- mask keys beyond N (last tile only)
        const int kbase = t * KT;
        if (kbase + KT > N) {
#pragma unroll
            for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (kbase + 32 * kbk + acc_row(i, hh) >= N) sacc[kbk][i] = -INFINITY;
        }
        // ---- online softmax (query = this lane's column; keys split over lane and lane^32)
        float mx = sacc[0][0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, sacc[0][i]);
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[1][i]);
        mx = fmaxf(mx, xchg32(mx));
        const float m_new = fmaxf(m_run, mx * c);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float ls = 0.f;
        uint32_t pk[2][8];
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[kbk][i], c, -m_new));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[kbk][i + 1], c, -m_new));
                ls += p0 + p1;
                pk[kbk][i >> 1] = pack_bf16(p0, p1);
            }
        l_run = l_run * alpha + ls;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            oacc[0][i] *= alpha;
            oacc[1][i] *= alpha;
        }
        // ---- O^T += V^T . P^T
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
                for (int db = 0; db < 2; ++db) oacc[db] = mfma(rd_tr1(vs, tl, kbk, s, db), pf, oacc[db]);
            }
        __syncthreads();
    }

    // ---- epilogue: O[q_row][d] = O^T[d][q_row] / l
    const float l = l_run + xchg32(l_run);
    if (q_row < N) {
        const float inv = 1.f / l;
        __hip_bfloat16* op = a.o + (long long)b * a.so.b + (long long)q_row * a.so.n + (long long)h * a.so.h;
#pragma unroll
        for (int db = 0; db < 2; ++db) store_tr_bf16(op + 32 * db, oacc[db], hh, inv, HD - 32 * db);
    }
}

}  // namespace

extern "C" int vfm_attention_fwd(const void* q, const void* k, const void* v, void* o, int B, int H, int N,
                                 int head_dim, const long long* sq, const long long* sk, const long long* sv,
                                 const long long* so, float scale, void* stream) {
    if (head_dim != HD) return VFM_NO_KERNEL;
    if (!q || !k || !v || !o || !sq || !sk || !sv || !so) return VFM_ERR_ARGS;
    if (B <= 0 || H <= 0 || N <= 0 || B > 65535 || H > 65535) return VFM_ERR_ARGS;
    // 16-B vector loads of 8 bf16: every row start must be 16-B aligned (unit stride along d)
    if (!strides_ok(sq, 8) || !strides_ok(sk, 8) || !strides_ok(sv, 8) || !strides_ok(so, 8)) return VFM_ERR_ARGS;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o)) return VFM_ERR_ARGS;
    AttnArgs a;
    a.q = (const __hip_bfloat16*)q;
    a.k = (const __hip_bfloat16*)k;
    a.v = (const __hip_bfloat16*)v;
    a.o = (__hip_bfloat16*)o;
    a.sq = mk(sq); a.sk = mk(sk); a.sv = mk(sv); a.so = mk(so);
    a.N = N;
    a.H = H;
    a.c = scale * 1.4426950408889634f;
    dim3 grid((N + QB - 1) / QB, H, B);
    VFM_LAUNCH(attn_fwd_d64, grid, dim3(64 * WAVES), 0, (hipStream_t)stream, a);
    return launch_status();
}
