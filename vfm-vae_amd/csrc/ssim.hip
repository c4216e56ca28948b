// Gaussian SSIM loss (mean over the valid 11x11 windows) and its gradient: the stage-2 fine-tuning
// loss and the evaluation tool's SSIM figure (training/loss.py SSIM, the restatement of the
// torchmetrics StructuralSimilarityIndexMeasure the reference builds at training/loss.py:150-152 and
// calls on clamped images at :257-260).
//
// The torch formulation reflect-pads by 5, filters five planes (p, t, p^2, t^2, pt) with the 121-tap
// window, drops a 5-wide border of the map and takes the mean. A kept pixel's window never leaves the
// image, so the result is the mean of the VALID correlation of the unpadded planes, an (H-10) x (W-10)
// map per plane; the window g (x) g is separable (rows, then columns: 11 + 11 taps).
//
//   forward   p = clamp(preds), t = clamp(target);  G = valid separable filter
//             mp = G p, mt = G t, epp = G p^2, ett = G t^2, ept = G pt
//             a1 = 2 mp mt + c1, a2 = 2 (ept - mp mt) + c2, b1 = mp^2 + mt^2 + c1,
//             b2 = (epp - mp^2) + (ett - mt^2) + c2,  S = (a1 a2) / (b1 b2),  out = sum S / N
//   backward  d_ept = 2 a1 / (b1 b2),  d_epp = -S / b2,
//             d_mp  = 2 mt (a2 - a1) / (b1 b2) + 2 mp S (1 / b2 - 1 / b1)
//             dpreds = dout / N [lo <= preds <= hi] (G^T d_mp + 2 p G^T d_epp + t G^T d_ept)
//             (G^T: full correlation of the maps, zero outside the valid region). S is symmetric in
//             (p, t): the gradient to target is the same kernel with the two images swapped.
//
// ssim_fwd: one block per (plane, TH x TW tile of the map). The (TH+10) x (TW+10) patches of both
// images are staged in LDS once (clamped on the way in), the row pass writes the five quantities
// to LDS, the column pass forms S and the block reduces it in a fixed order to one partial;
// ssim_finish sums the partials in a fixed order. No atomics: two runs agree bitwise.
// ssim_bwd: one block per (plane, TH x TW tile of the image), recomputing from the two images: patches
// of (TH+20) x (TW+20), the five quantities on the (TH+10) x (TW+10) map neighbourhood of the tile, the
// three derivative maps, then the two G^T passes. Nothing is saved between forward and backward.
//
// LDS traffic bounds both kernels, so each pass reads an input once per thread and slides the window
// in registers. Row passes: a thread makes four adjacent outputs from 16-byte reads of one row;
// consecutive lanes walk DOWN a column of such quads, and every row stride is an odd number of quads,
// so the lanes of a 16-byte access fall on distinct slots. Column passes: a lane owns a column and a
// run of rows, consecutive lanes read consecutive dwords of a row: no bank conflicts.
#include "vfm_common.h"

namespace {

using namespace vfm;

constexpr int K = 11;        // window length
constexpr int R = K - 1;     // rows / columns a window reaches beyond its first
constexpr int TH = 16, TW = 32;
constexpr int NT = 256;
constexpr int CG = NT / TW;  // row groups of a column pass over a TW-wide array
static_assert(TW % 4 == 0 && TH % CG == 0 && NT % 64 == 0, "tile / block shape");

typedef float f4 __attribute__((ext_vector_type(4)));

struct Taps { float g[K]; };
struct Consts { float c1, c2, lo, hi; int clamp; };

// smallest odd number of quads (4 floats) covering w floats
constexpr int odd_quads(int w) { return ((w + 3) / 4) | 1; }

// torch.clamp semantics: NaN passes through (see clamp_lv in posterior.hip)
__device__ __forceinline__ float clamp_px(float v, const Consts& c) {
    return (!c.clamp || v != v) ? v : fminf(fmaxf(v, c.lo), c.hi);
}

// Stage NR rows of 4 PQ pixels of both images, first pixel (y0, x0) (may be negative); pixels outside
// the image are clamp(0) (they only reach map positions outside the valid region, which are dropped).
// All of a thread's loads are issued before the first is used: a block's life is otherwise a chain of
// global-memory round trips, one per loop iteration.
template <int NR, int PQ>
__device__ __forceinline__ void stage(const float* __restrict__ pp, const float* __restrict__ tp, float* sp, float* st,
                                      int y0, int x0, int H, int W, const Consts& c) {
    constexpr int PW = 4 * PQ, N = NR * PW, IT = (N + NT - 1) / NT;
    float a[IT], b[IT];
#pragma unroll
    for (int n = 0; n < IT; ++n) {
        const int i = threadIdx.x + n * NT;
        const int r = i / PW, y = y0 + r, x = x0 + (i - r * PW);
        const bool in = i < N && y >= 0 && y < H && x >= 0 && x < W;
        const long long o = (long long)y * W + x;
        a[n] = in ? pp[o] : 0.f;
        b[n] = in ? tp[o] : 0.f;
    }
#pragma unroll
    for (int n = 0; n < IT; ++n) {
        const int i = threadIdx.x + n * NT;
        if (i < N) {
            sp[i] = clamp_px(a[n], c);
            st[i] = clamp_px(b[n], c);
        }
    }
}

__device__ __forceinline__ void load16(const float* s, float* x) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const f4 v = reinterpret_cast<const f4*>(s)[n];
        x[4 * n] = v.x; x[4 * n + 1] = v.y; x[4 * n + 2] = v.z; x[4 * n + 3] = v.w;
    }
}

// Row pass: q[j][r][c] = sum_k g[k] f_j[r][c + k] for f = (p, t, p^2, t^2, pt) and c < 4 OQ, four
// adjacent c per thread (patch rows of PQ quads, q rows of QQ quads, plane stride NR * 4 QQ). mp / mt
// and epp / ett / ept each run the same operations in the same order, so identical images give
// identical means and identical second moments.
template <int NR, int PQ, int OQ, int QQ>
__device__ __forceinline__ void row_pass(const float* sp, const float* st, float* q, const Taps& w) {
    static_assert(PQ >= OQ + 3 && QQ >= OQ, "a thread reads 16 floats from its first output's column");
    constexpr int PL = NR * 4 * QQ;
    for (int i = threadIdx.x; i < NR * OQ; i += NT) {
        const int cq = i / NR, r = i - cq * NR;
        float x[16], y[16];
        load16(sp + (r * PQ + cq) * 4, x);
        load16(st + (r * PQ + cq) * 4, y);
        float xx[K + 3], yy[K + 3], xy[K + 3];
#pragma unroll
        for (int n = 0; n < K + 3; ++n) {
            xx[n] = x[n] * x[n];
            yy[n] = y[n] * y[n];
            xy[n] = x[n] * y[n];
        }
        f4 a[5] = {};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float g = w.g[k];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                a[0][n] = fmaf(g, x[n + k], a[0][n]);
                a[1][n] = fmaf(g, y[n + k], a[1][n]);
                a[2][n] = fmaf(g, xx[n + k], a[2][n]);
                a[3][n] = fmaf(g, yy[n + k], a[3][n]);
                a[4][n] = fmaf(g, xy[n + k], a[4][n]);
            }
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) *reinterpret_cast<f4*>(q + j * PL + (r * QQ + cq) * 4) = a[j];
    }
}

// Column pass of NQ planes (plane stride PL, row stride S) at column c for the RPT output rows from
// r0: each of the RPT + R input rows is read once. Output row o = sum_k g[k] q[r0 + o + k], or with
// FLIP (the transposed pass) sum_k g[k] q[r0 + o + R - k]. Rows past `last` read row `last` instead:
// they only feed output rows the caller drops.
template <int NQ, int RPT, bool FLIP>
__device__ __forceinline__ void col_pass(const float* q, int PL, int S, int r0, int c, int last, const Taps& w,
                                         float (*v)[NQ]) {
#pragma unroll
    for (int o = 0; o < RPT; ++o)
#pragma unroll
        for (int j = 0; j < NQ; ++j) v[o][j] = 0.f;
#pragma unroll
    for (int rr = 0; rr < RPT + R; ++rr) {
        const int row = min(r0 + rr, last);
        float x[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) x[j] = q[j * PL + row * S + c];
#pragma unroll
        for (int o = 0; o < RPT; ++o) {
            const int k = FLIP ? o + R - rr : rr - o;
            if (k >= 0 && k <= R) {
#pragma unroll
                for (int j = 0; j < NQ; ++j) v[o][j] = fmaf(w.g[k], x[j], v[o][j]);
            }
        }
    }
}

struct Point { float S, a1, a2, b1, b2; };

// S at one map position from (mp, mt, epp, ett, ept). Every product and sum is rounded on its own, as
// the torch formulation's are: then p == t gives a1 == b1 and a2 == b2 bitwise and S == 1 exactly (a
// fused 2 mp mt + c1 would differ from mp^2 + mt^2 + c1 in the last bit).
__device__ __forceinline__ Point ssim_point(const float* v, const Consts& c) {
#pragma clang fp contract(off)
    const float mp = v[0], mt = v[1];
    const float mpp = mp * mp, mtt = mt * mt, mpt = mp * mt;
    const float spp = v[2] - mpp, stt = v[3] - mtt, spt = v[4] - mpt;
    Point r;
    r.a1 = 2.f * mpt + c.c1;
    r.a2 = 2.f * spt + c.c2;
    r.b1 = mpp + mtt + c.c1;
    r.b2 = spp + stt + c.c2;
    r.S = (r.a1 * r.a2) / (r.b1 * r.b2);
    return r;
}

__global__ __launch_bounds__(NT) void ssim_fwd(const float* __restrict__ preds, const float* __restrict__ target,
                                               float* __restrict__ partials, Taps w, Consts c, int H, int W,
                                               int tiles_x, int tiles_y) {
    constexpr int NR = TH + R, OQ = TW / 4, PQ = odd_quads(TW + R + 2), QQ = odd_quads(TW), S = 4 * QQ, PL = NR * S;
    constexpr int RPT = TH / CG;
    __shared__ __attribute__((aligned(16))) float sp[NR * 4 * PQ], st[NR * 4 * PQ], q[5 * PL];
    __shared__ float red[NT / 64];
    const unsigned tpp = (unsigned)tiles_x * tiles_y;
    const unsigned plane = blockIdx.x / tpp, tile = blockIdx.x - plane * tpp;
    const int y0 = (int)(tile / tiles_x) * TH, x0 = (int)(tile % tiles_x) * TW;
    const long long base = (long long)plane * H * W;
    stage<NR, PQ>(preds + base, target + base, sp, st, y0, x0, H, W, c);
    __syncthreads();
    row_pass<NR, PQ, OQ, QQ>(sp, st, q, w);
    __syncthreads();
    const int col = threadIdx.x % TW, r0 = threadIdx.x / TW * RPT;
    float v[RPT][5];
    col_pass<5, RPT, false>(q, PL, S, r0, col, NR - 1, w, v);
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const bool valid = y0 + r0 + o < H - R && x0 + col < W - R;
        const float s = ssim_point(v[o], c).S;
        acc += valid ? s : 0.f;
    }
    // fixed-order block sum: lanes of a wave by halving shuffles, then the four waves in order
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(NT) void ssim_finish(const float* __restrict__ partials, int n, double inv_n,
                                                  float* __restrict__ out) {
    __shared__ double red[NT];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) acc += (double)partials[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(red[0] * inv_n);
}

__global__ __launch_bounds__(NT) void ssim_bwd(const float* __restrict__ preds, const float* __restrict__ target,
                                               const float* __restrict__ dout, float* __restrict__ dpreds, Taps w,
                                               Consts c, float inv_n, int H, int W, int tiles_x, int tiles_y) {
    constexpr int NR = TH + 2 * R;                      // patch rows
    constexpr int MH = TH + R, MW = TW + R;             // map neighbourhood of the tile
    constexpr int OQ = (MW + 3) / 4, PQ = odd_quads(4 * OQ + 12), QQ = odd_quads(MW), S = 4 * QQ, PL = NR * S;
    constexpr int MQ = odd_quads(TW + 12), MS = 4 * MQ, ML = MH * MS;      // derivative maps [3][MH][MS]
    constexpr int RQ = odd_quads(TW), RS = 4 * RQ, RL = MH * RS;           // their G^T row pass [3][MH][RS]
    constexpr int NWV = NT / 64, RPM = (MH + NWV - 1) / NWV;               // map rows per wave: a lane owns a column
    constexpr int RPT = TH / CG;
    static_assert(MS <= 64 && MS >= MW, "one lane per map column");
    static_assert(3 * ML + 3 * RL <= 5 * PL, "derivative maps and their row pass reuse the row-pass buffer");
    __shared__ __attribute__((aligned(16))) float sp[NR * 4 * PQ], st[NR * 4 * PQ], q[5 * PL];
    const unsigned tpp = (unsigned)tiles_x * tiles_y;
    const unsigned plane = blockIdx.x / tpp, tile = blockIdx.x - plane * tpp;
    const int y0 = (int)(tile / tiles_x) * TH, x0 = (int)(tile % tiles_x) * TW;
    const long long base = (long long)plane * H * W;
    stage<NR, PQ>(preds + base, target + base, sp, st, y0 - R, x0 - R, H, W, c);
    __syncthreads();
    row_pass<NR, PQ, OQ, QQ>(sp, st, q, w);
    __syncthreads();
    // derivative maps at map position (y0 - R + il, x0 - R + lane), zero outside the valid map; held in
    // registers until every thread has read the row-pass buffer they then overwrite
    const int lane = threadIdx.x & 63, m0 = (threadIdx.x >> 6) * RPM;
    float d[RPM][3];
#pragma unroll
    for (int o = 0; o < RPM; ++o) d[o][0] = d[o][1] = d[o][2] = 0.f;
    if (lane < MW) {
        float v[RPM][5];
        col_pass<5, RPM, false>(q, PL, S, m0, lane, NR - 1, w, v);
        const int mx = x0 - R + lane;
#pragma unroll
        for (int o = 0; o < RPM; ++o) {
            const int il = m0 + o, my = y0 - R + il;
            if (il < MH && my >= 0 && my < H - R && mx >= 0 && mx < W - R) {
                const Point s = ssim_point(v[o], c);
                const float inv = 1.f / (s.b1 * s.b2);
                d[o][0] = 2.f * v[o][1] * (s.a2 - s.a1) * inv + 2.f * v[o][0] * s.S * (1.f / s.b2 - 1.f / s.b1);
                d[o][1] = -s.S / s.b2;
                d[o][2] = 2.f * s.a1 * inv;
            }
        }
    }
    __syncthreads();
    float* m = q;               // [3][MH][MS] derivative maps (columns from MW on are zero)
    float* rr = q + 3 * ML;     // [3][MH][RS] their G^T row pass
    if (lane < MS) {
#pragma unroll
        for (int o = 0; o < RPM; ++o) {
            const int il = m0 + o;
            if (il < MH) {
                m[il * MS + lane] = d[o][0];
                m[ML + il * MS + lane] = d[o][1];
                m[2 * ML + il * MS + lane] = d[o][2];
            }
        }
    }
    __syncthreads();
    // the tile's raw preds (the clamp mask), requested ahead of the two G^T passes that hide the trip
    const int xl = threadIdx.x % TW, r0 = threadIdx.x / TW * RPT, x = x0 + xl;
    float raw[RPT];
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int y = y0 + r0 + o;
        raw[o] = (y < H && x < W) ? preds[base + (long long)y * W + x] : 0.f;
    }
    // G^T rows: image column x0 + xl collects map columns x0 + xl - k, local xl + R - k; four adjacent xl
    // per thread
    for (int i = threadIdx.x; i < MH * (TW / 4); i += NT) {
        const int cq = i / MH, il = i - cq * MH;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float x[16];
            load16(m + j * ML + (il * MQ + cq) * 4, x);
            f4 a = {};
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int n = 0; n < 4; ++n) a[n] = fmaf(w.g[k], x[n + R - k], a[n]);
            *reinterpret_cast<f4*>(rr + j * RL + (il * RQ + cq) * 4) = a;
        }
    }
    __syncthreads();
    const float scale = dout[0] * inv_n;
    // G^T columns: image row y0 + yl collects map rows y0 + yl - k, local yl + R - k
    float v[RPT][3];
    col_pass<3, RPT, true>(rr, RL, RS, r0, xl, MH - 1, w, v);
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int yl = r0 + o, y = y0 + yl;
        if (y < H && x < W) {
            const int po = (yl + R) * 4 * PQ + xl + R;
            const long long go = base + (long long)y * W + x;
            const float g = scale * (v[o][0] + 2.f * sp[po] * v[o][1] + st[po] * v[o][2]);
            // torch's clamp backward: the gradient passes where lo <= preds <= hi (inclusive)
            dpreds[go] = (!c.clamp || (raw[o] >= c.lo && raw[o] <= c.hi)) ? g : 0.f;
        }
    }
}

// Blocks of a launch with one block per (plane, TH x TW tile of an h x w grid), or -1 when they do not
// fit the grid's x dimension.
long long blocks_for(int B, int C, int h, int w, int* tiles_x, int* tiles_y) {
    *tiles_x = (w + TW - 1) / TW;
    *tiles_y = (h + TH - 1) / TH;
    const long long tpp = (long long)*tiles_x * *tiles_y;
    const long long planes = (long long)B * C;
    if (tpp > 0x7fffffffLL || planes > 0x7fffffffLL / tpp) return -1;
    return planes * tpp;
}

int check_args(const void* a, const void* b, const void* c, const void* d, const float* taps, int ksize, int B, int C,
               int H, int W) {
    if (!a || !b || !c || !d || !taps || B <= 0 || C <= 0 || H < K || W < K) return VFM_ERR_ARGS;
    return ksize == K ? VFM_OK : VFM_NO_KERNEL;
}

Taps make_taps(const float* taps) {
    Taps w;
    for (int k = 0; k < K; ++k) w.g[k] = taps[k];
    return w;
}

}  // namespace

extern "C" int vfm_ssim_fwd_partials(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H < K || W < K) return VFM_ERR_ARGS;
    int tx, ty;
    const long long n = blocks_for(B, C, H - R, W - R, &tx, &ty);
    return n < 0 ? VFM_ERR_ARGS : (int)n;
}

extern "C" int vfm_ssim_fwd(const float* preds, const float* target, float* partials, float* out, const float* taps,
                            int ksize, float c1, float c2, float lo, float hi, int clamp, int B, int C, int H, int W,
                            void* stream) {
    const int rc = check_args(preds, target, partials, out, taps, ksize, B, C, H, W);
    if (rc != VFM_OK) return rc;
    int tx, ty;
    const long long blocks = blocks_for(B, C, H - R, W - R, &tx, &ty);
    if (blocks < 0) return VFM_ERR_ARGS;
    const Consts c{c1, c2, lo, hi, clamp};
    const double n = (double)B * C * (H - R) * (W - R);
    VFM_LAUNCH(ssim_fwd, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, preds, target, partials,
               make_taps(taps), c, H, W, tx, ty);
    VFM_LAUNCH(ssim_finish, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float*)partials, (int)blocks, 1.0 / n,
               out);
    return launch_status();
}

extern "C" int vfm_ssim_bwd(const float* preds, const float* target, const float* dout, float* dpreds,
                            const float* taps, int ksize, float c1, float c2, float lo, float hi, int clamp, int B,
                            int C, int H, int W, void* stream) {
    const int rc = check_args(preds, target, dout, dpreds, taps, ksize, B, C, H, W);
    if (rc != VFM_OK) return rc;
    int tx, ty;
    const long long blocks = blocks_for(B, C, H, W, &tx, &ty);
    if (blocks < 0) return VFM_ERR_ARGS;
    const Consts c{c1, c2, lo, hi, clamp};
    const double n = (double)B * C * (H - R) * (W - R);
    VFM_LAUNCH(ssim_bwd, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, preds, target, dout, dpreds,
               make_taps(taps), c, (float)(1.0 / n), H, W, tx, ty);
    return launch_status();
}
