// Nearest neighbours by inner product without the N x N Gram matrix, and the CKNNA sums over the
// neighbour lists: the device side of tools/evaluate_alignment/metrics.py (reference
// tools/evaluate_alignment/metrics.py:191-260: two dense fp32 Gram matrices, torch.topk on clones of
// them, three pairs of scattered N x N masks and hsic_unbiased with a full N x N . N x N torch.mm, three
// times).
//
// gram_topk_kernel: "Gram row block x all columns, keep the k best per row" -- a GEMM that never writes
// its output. A workgroup (256 threads, 2 x 2 waves) owns BM = 128 rows and walks the BN = 128 wide
// column tiles of its split. Both operands are K-contiguous rows of the same matrix, staged as in
// sgemm.hip ([k][outer] images, one ds_read_b128 per four k-steps) and multiplied on
// v_mfma_f32_32x32x2_f32: exact fp32 products, one accumulator per score over the whole K loop, so a
// score's bits do not depend on the tile or split it is computed in. After a tile's K loop the
// accumulators go to an LDS score tile (it aliases the staging buffers):
//   phase 1, all threads: thread (row, half) compares its 64 scores with the row's k-th value and
//            leaves a 64-bit candidate mask; columns >= N and the diagonal are cleared here;
//   phase 2, the 128 row owners: walk the set bits in ascending column order; a candidate fills the
//            row's list in LDS ([slot][row], unordered) or replaces its worst entry, and the owner finds
//            the new worst (k independent LDS reads). Past the first few tiles few bits are set.
// Order: descending value, equal values by ascending index (-0.0 == 0.0). Columns arrive in ascending
// order, so a candidate has to beat the k-th value strictly, and the worst entry is the one with the
// lowest value and, among equal values, the highest index. The next column tile's first K-tile is
// loaded into registers before the selection, which hides its latency.
// Each split writes its rows' lists in order (an entry's place is the number of entries ahead of it;
// (-inf, INT_MAX) where the split has fewer than k columns) to the workspace; topk_merge selects the
// final k of a row from its `splits` sorted lists in the same order. Device memory is
// O(N D + splits N k). Splits are column-tile aligned, so the row blocks of a small N still fill the chip.
//
// cknna kernels: with M(i) the intersection of row i's two lists, the three hsic_unbiased calls need
// only, for (A, B) in ((M o K, M o L), (M_K o K, M_K o K), (M_L o L, M_L o L)):
//   cross   = sum_{(i,j) in M, (j,i) in M} A_ij B_ji        (the sum(K~ o L~^T) term)
//   sums    = sum A . sum B
//   product = sum_i sum_{j in M(i)} A_ij rowsum(B)_j        (= sum(A @ B))
// all in fp64: cknna_rowsums (per row), cknna_rows (per row, fixed-order block sums) and cknna_finish
// (block partials in a fixed order). No atomics: two runs agree bitwise.
#include "vfm_common.h"

#include <limits.h>

namespace {

using namespace vfm;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int BM = 128, BN = 128, BK = 32, NT = 256;
constexpr int SS = BN + 1;                 // score tile row stride (floats): rows on distinct banks
constexpr int MAXK = 64, MAXSPLITS = 64;
constexpr int TARGET_WG = 512;             // two workgroups on each of 256 CUs

struct KnnArgs {
    const float* f;
    long long ld;
    int N, D, k, excl;
    int splits, tps, ctiles;               // column tiles per split, column tiles in all
    int vec;                               // rows loadable as 16-B chunks
    float* val;                            // [splits][N][k] (the output itself when splits == 1)
    int* idx;
};

// One operand tile (128 rows x 32 k) global -> registers -> LDS image [2][128][16] (sgemm.hip's K-contiguous
// staging): half hh = k / 16, row, s = k % 16 contiguous, the four 16-B slots of a row XOR-swizzled by
// (row >> 2) & 3, 16 pad floats before half 1. MFMA k-step s pairs k = s (lanes 0-31) with k = 16 + s.
struct Stage {
    static constexpr int HALF = BM * 16 + 16;
    static constexpr int FLOATS = 2 * HALF;
    static constexpr int PER = BM * BK / 4 / NT;
    float4 r[PER];

    __device__ __forceinline__ void load(const KnnArgs& a, unsigned row0, int k0, int tid) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int c = tid + NT * u;
            const unsigned o = row0 + (c >> 3);
            const int k = k0 + (c & 7) * 4;
            const float* p = a.f + (long long)o * a.ld + k;
            if (a.vec) {
                // branch-free bounds: an out-of-range chunk loads the matrix's first chunk and is zeroed
                const bool ok = o < (unsigned)a.N && k < a.D;
                const float4 v = *reinterpret_cast<const float4*>(ok ? p : a.f);
                r[u] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float e[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) e[i] = (o < (unsigned)a.N && k + i < a.D) ? p[i] : 0.f;
                r[u] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    }

    __device__ __forceinline__ void store(float* img, int tid) const {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int c = tid + NT * u, row = c >> 3, kk = (c & 7) * 4, ss = kk & 15;
            *reinterpret_cast<float4*>(img + (kk >> 4) * HALF + row * 16 + 4 * ((ss >> 2) ^ ((row >> 2) & 3))) = r[u];
        }
    }

    // fragments of k-steps 4q .. 4q + 3 of the lane's row (orow + (lane & 31))
    __device__ __forceinline__ static float4 quad(const float* img, int lane, int orow, int q) {
        const int row = orow + (lane & 31);
        return *reinterpret_cast<const float4*>(img + (lane >> 5) * HALF + row * 16 + 4 * (q ^ ((row >> 2) & 3)));
    }
};

constexpr int STAGE = 2 * Stage::FLOATS;                       // both operands of one K-tile
static_assert(2 * STAGE >= BM * SS, "the score tile aliases the two staging buffers");
constexpr int TILE_FLOATS = 2 * STAGE;
constexpr size_t LDS_FIXED = (size_t)TILE_FLOATS * 4 + 2 * BM * sizeof(u64) + BM * 4;
inline size_t lds_bytes(int k) { return LDS_FIXED + (size_t)k * BM * 8; }

__global__ __launch_bounds__(NT, 2) void gram_topk_kernel(KnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u64* cmask = reinterpret_cast<u64*>(lds + TILE_FLOATS);    // [2][BM]
    float* thr = reinterpret_cast<float*>(cmask + 2 * BM);     // [BM]: the row's k-th value (-inf: list not full)
    float* lval = thr + BM;                                    // [k][BM]
    int* lidx = reinterpret_cast<int*>(lval + a.k * BM);       // [k][BM]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const unsigned m0 = blockIdx.x * (unsigned)BM;
    const int split = blockIdx.y;
    const int ct0 = split * a.tps, ct1 = min(a.ctiles, ct0 + a.tps);
    const int kt = (a.D + BK - 1) / BK;
    const float NEG = -__builtin_inff();

    int cnt = 0, worst = 0;                                    // entries in the list of row tid (owners: tid < BM)
                                                               // and, once it is full, the slot of its worst one
    if (tid < BM) thr[tid] = NEG;

    Stage sa, sb;
    sa.load(a, m0, 0, tid);
    sb.load(a, (unsigned)ct0 * BN, 0, tid);
    for (int ct = ct0; ct < ct1; ++ct) {
        const unsigned n0 = (unsigned)ct * BN;
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

        sa.store(lds, tid);
        sb.store(lds + Stage::FLOATS, tid);
        __syncthreads();
        for (int u = 0; u < kt; ++u) {
            // K-tile u + 1 travels to registers while tile u is multiplied, then into the other stage
            // (last read in iteration u - 1, which every wave left through the barrier)
            if (u + 1 < kt) {
                sa.load(a, m0, (u + 1) * BK, tid);
                sb.load(a, n0, (u + 1) * BK, tid);
            }
            const float* cur = lds + (u & 1) * STAGE;
            float4 fa[2][2], fb[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[0][i] = Stage::quad(cur, lane, 64 * wm + 32 * i, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[0][j] = Stage::quad(cur + Stage::FLOATS, lane, 64 * wn + 32 * j, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q + 1 < 4) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) fa[(q + 1) & 1][i] = Stage::quad(cur, lane, 64 * wm + 32 * i, q + 1);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        fb[(q + 1) & 1][j] = Stage::quad(cur + Stage::FLOATS, lane, 64 * wn + 32 * j, q + 1);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q & 1][i][e], fb[q & 1][j][e],
                                                                            acc[i][j], 0, 0, 0);
            }
            if (u + 1 < kt) {
                float* nxt = lds + ((u + 1) & 1) * STAGE;
                sa.store(nxt, tid);
                sb.store(nxt + Stage::FLOATS, tid);
            }
            __syncthreads();
        }

        if (ct + 1 < ct1) {
            if (kt > 1) sa.load(a, m0, 0, tid);                // one K-tile: sa still holds the row block
            sb.load(a, n0 + BN, 0, tid);
        }
        // acc[i][j][e] = <f[m0 + m], f[n0 + n]>: m = 64 wm + 32 i + (e & 3) + 8 (e >> 2) + 4 (lane >> 5),
        // n = 64 wn + 32 j + (lane & 31). The K loop ended on a barrier: the staging buffers are free.
        {
            const int r = lane & 31, hh = lane >> 5;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int m = 64 * wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hh;
                        lds[m * SS + 64 * wn + 32 * j + r] = acc[i][j][e];
                    }
        }
        __syncthreads();

        // phase 1: candidate mask of (row, half)
        {
            const int row = tid & (BM - 1), half = tid >> 7;
            const unsigned gi = m0 + row, c0 = n0 + 64 * half;
            const float t = thr[row];
            const float* s = lds + row * SS + 64 * half;
            u64 m = 0;
#pragma unroll 16
            for (int c = 0; c < 64; ++c) m |= (u64)(s[c] > t) << c;
            u64 ok = 0;
            if (gi < (unsigned)a.N && c0 < (unsigned)a.N) {
                const unsigned nc = (unsigned)a.N - c0;
                ok = nc >= 64 ? ~0ull : (1ull << nc) - 1;
                if (a.excl && gi >= c0 && gi - c0 < 64) ok &= ~(1ull << (gi - c0));
            }
            cmask[half * BM + row] = m & ok;
        }
        __syncthreads();

        // phase 2: the row owners insert their candidates, ascending column
        if (tid < BM) {
            const int k = a.k;
            float cur = thr[tid];
            for (int half = 0; half < 2; ++half) {
                u64 m = cmask[half * BM + tid];
                while (m) {
                    const int c = __builtin_ctzll(m) + 64 * half;
                    m &= m - 1;
                    const float v = lds[tid * SS + c];
                    if (cnt == k && !(v > cur)) continue;
                    // a list that is not full grows; a full one replaces its worst entry
                    const int p = cnt < k ? cnt++ : worst;
                    lval[p * BM + tid] = v;
                    lidx[p * BM + tid] = (int)(n0 + c);
                    if (cnt == k) {
                        // the new worst entry: lowest value, among equal values the highest index (k independent
                        // LDS reads; a sorted list would cost a dependent read per shifted entry)
                        int wi = -1;
                        for (int q = 0; q < k; ++q) {
                            const float vq = lval[q * BM + tid];
                            const int iq = lidx[q * BM + tid];
                            if (q == 0 || vq < cur || (vq == cur && iq > wi)) { cur = vq; wi = iq; worst = q; }
                        }
                    }
                }
            }
            thr[tid] = cur;
        }
        __syncthreads();                                       // the next tile's staging overwrites the scores
    }

    if (tid < BM && m0 + tid < (unsigned)a.N) {
        const long long base = ((long long)split * a.N + (m0 + tid)) * a.k;
        // the list is unordered: an entry's place is the number of entries ahead of it (indices are distinct)
        for (int p = 0; p < cnt; ++p) {
            const float v = lval[p * BM + tid];
            const int i = lidx[p * BM + tid];
            int rank = 0;
            for (int q = 0; q < cnt; ++q) {
                const float vq = lval[q * BM + tid];
                rank += (vq > v || (vq == v && lidx[q * BM + tid] < i)) ? 1 : 0;
            }
            a.val[base + rank] = v;
            a.idx[base + rank] = i;
        }
        for (int p = cnt; p < a.k; ++p) {
            a.val[base + p] = NEG;
            a.idx[base + p] = INT_MAX;
        }
    }
}

// Row r's final k from its S sorted partial lists: k rounds of "best head", one thread per row, the heads'
// positions in LDS. Descending value, equal values by ascending index; the padding (index INT_MAX) never wins.
__global__ __launch_bounds__(128) void topk_merge(const float* __restrict__ wv, const int* __restrict__ wi, int N, int k,
                                                  int S, float* __restrict__ val, int* __restrict__ idx) {
    __shared__ unsigned char pos[MAXSPLITS][128];
    const int t = threadIdx.x;
    const long long row = (long long)blockIdx.x * 128 + t;
    if (row >= N) return;
    for (int s = 0; s < S; ++s) pos[s][t] = 0;
    for (int o = 0; o < k; ++o) {
        float bv = 0.f;
        int bi = INT_MAX, bs = -1;
        for (int s = 0; s < S; ++s) {
            const int p = pos[s][t];
            if (p >= k) continue;
            const long long at = ((long long)s * N + row) * k + p;
            const int i = wi[at];
            if (i == INT_MAX) continue;
            const float v = wv[at];
            if (bs < 0 || v > bv || (v == bv && i < bi)) { bv = v; bi = i; bs = s; }
        }
        if (bs < 0) {                                          // fewer than k columns in all: the launcher refuses it
            val[row * k + o] = -__builtin_inff();
            idx[row * k + o] = -1;
            continue;
        }
        val[row * k + o] = bv;
        idx[row * k + o] = bi;
        ++pos[bs][t];
    }
}

bool plan_splits(int N, int k, int splits, int* chosen, int* tps_out) {
    if (N < 1 || k < 1 || k > MAXK || splits < 0) return false;
    const int ctiles = (int)(((long long)N + BN - 1) / BN), rblocks = (int)(((long long)N + BM - 1) / BM);
    const int smax = ctiles < MAXSPLITS ? ctiles : MAXSPLITS;
    int s = splits < smax ? splits : smax;
    if (splits == 0) {
        // the fewest splits whose grid fills at least 0.9 of its rounds of TARGET_WG resident workgroups (553
        // workgroups would run as one full round and one of 41), else the best-filled grid
        double best = -1.0;
        for (int c = 1; c <= smax; ++c) {
            const int t = (ctiles + c - 1) / c;
            const long long wgs = (long long)rblocks * ((ctiles + t - 1) / t);
            const double fill = (double)wgs / (double)((wgs + TARGET_WG - 1) / TARGET_WG * TARGET_WG);
            if (fill > best) { best = fill; s = c; }
            if (fill >= 0.9) break;
        }
    }
    const int tps = (ctiles + s - 1) / s;
    *chosen = (ctiles + tps - 1) / tps;                        // no empty split
    *tps_out = tps;
    return true;
}

// ---------------------------------------------------------------------------------------- CKNNA sums

constexpr int CN = 256;                    // rows per block
constexpr int NQ = 10;                     // per-row quantities, see cknna_rows

// position of `want` in the k indices at p, or -1
__device__ __forceinline__ int find(const int* __restrict__ p, int k, int want) {
    int at = -1;
    for (int q = 0; q < k; ++q)
        if (p[q] == want && at < 0) at = q;
    return at;
}

// rs[0] = sum_p K_ip, rs[1] = sum_p L_ip, rs[2] = sum_{p in M(i)} K_ip, rs[3] = sum_{p in M(i)} L_ip
__global__ __launch_bounds__(CN) void cknna_rowsums(const int* __restrict__ iK, const float* __restrict__ vK,
                                                    const int* __restrict__ iL, const float* __restrict__ vL, int N, int k,
                                                    double* __restrict__ rs) {
    const long long i = (long long)blockIdx.x * CN + threadIdx.x;
    if (i >= N) return;
    const int *ik = iK + i * k, *il = iL + i * k;
    const float *vk = vK + i * k, *vl = vL + i * k;
    double sk = 0, sl = 0, skm = 0, slm = 0;
    for (int p = 0; p < k; ++p) {
        sk += (double)vk[p];
        if (find(il, k, ik[p]) >= 0) skm += (double)vk[p];
    }
    for (int p = 0; p < k; ++p) {
        sl += (double)vl[p];
        if (find(ik, k, il[p]) >= 0) slm += (double)vl[p];
    }
    rs[i] = sk;
    rs[(long long)N + i] = sl;
    rs[2LL * N + i] = skm;
    rs[3LL * N + i] = slm;
}

// Per row: 0 cross KL, 1 product KL, 2 cross KK, 3 product KK, 4 cross LL, 5 product LL, 6-9 the row's four sums
// (rs order); summed over the block's rows in a fixed order into part[block][NQ].
__global__ __launch_bounds__(CN) void cknna_rows(const int* __restrict__ iK, const float* __restrict__ vK,
                                                 const int* __restrict__ iL, const float* __restrict__ vL, int N, int k,
                                                 const double* __restrict__ rs, double* __restrict__ part) {
    __shared__ double red[CN / 64][NQ];
    const long long i = (long long)blockIdx.x * CN + threadIdx.x;
    double q[NQ] = {};
    if (i < N) {
        const int *ik = iK + i * k, *il = iL + i * k;
        const float *vk = vK + i * k, *vl = vL + i * k;
        for (int p = 0; p < k; ++p) {
            const int j = ik[p];
            if (j < 0 || j >= N) continue;
            const double v = (double)vk[p];
            const long long jb = (long long)j * k;
            const int back = find(iK + jb, k, (int)i);         // (j, i) in M_K
            if (back >= 0) q[2] += v * (double)vK[jb + back];
            q[3] += v * rs[j];
            if (find(il, k, j) >= 0) {                         // (i, j) in M
                const int backl = find(iL + jb, k, (int)i);
                if (back >= 0 && backl >= 0) q[0] += v * (double)vL[jb + backl];
                q[1] += v * rs[3LL * N + j];
            }
        }
        for (int p = 0; p < k; ++p) {
            const int j = il[p];
            if (j < 0 || j >= N) continue;
            const double v = (double)vl[p];
            const long long jb = (long long)j * k;
            const int back = find(iL + jb, k, (int)i);
            if (back >= 0) q[4] += v * (double)vL[jb + back];
            q[5] += v * rs[(long long)N + j];
        }
        for (int c = 0; c < 4; ++c) q[6 + c] = rs[(long long)c * N + i];
    }
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) q[c] += __shfl_down(q[c], s, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = q[c];
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int c = threadIdx.x;
        part[(long long)blockIdx.x * NQ + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// out[3 h + (0 cross, 1 sum A . sum B, 2 product)], h = 0 (M o K, M o L), 1 (M_K o K twice), 2 (M_L o L twice)
__global__ __launch_bounds__(CN) void cknna_finish(const double* __restrict__ part, int blocks, double* __restrict__ out) {
    __shared__ double red[CN / 64][NQ];
    double q[NQ] = {};
    for (int b = threadIdx.x; b < blocks; b += CN)
#pragma unroll
        for (int c = 0; c < NQ; ++c) q[c] += part[(long long)b * NQ + c];
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) q[c] += __shfl_down(q[c], s, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = q[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[NQ];
        for (int c = 0; c < NQ; ++c) t[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        out[0] = t[0]; out[1] = t[8] * t[9]; out[2] = t[1];
        out[3] = t[2]; out[4] = t[6] * t[6]; out[5] = t[3];
        out[6] = t[4]; out[7] = t[7] * t[7]; out[8] = t[5];
    }
}

}  // namespace

extern "C" long long vfm_gram_topk_ws(int N, int k, int splits, int* chosen) {
    int s, tps;
    if (!plan_splits(N, k, splits, &s, &tps)) return VFM_ERR_ARGS;
    if (chosen) *chosen = s;
    return s > 1 ? (long long)s * N * k * 8 : 0;
}

extern "C" int vfm_gram_topk(const float* feats, long long ld, int N, int D, int k, int exclude_self, int splits,
                             int* idx, float* val, void* ws, void* stream) {
    if (!feats || !idx || !val || N < 1 || D < 1 || k < 1 || ld < D || splits < 0) return VFM_ERR_ARGS;
    if ((long long)k > (long long)N - (exclude_self ? 1 : 0)) return VFM_ERR_ARGS;
    if (k > MAXK) return VFM_NO_KERNEL;
    KnnArgs a;
    if (!plan_splits(N, k, splits, &a.splits, &a.tps)) return VFM_ERR_ARGS;
    if (a.splits > 1 && !ws) return VFM_ERR_ARGS;
    a.f = feats; a.ld = ld; a.N = N; a.D = D; a.k = k; a.excl = exclude_self ? 1 : 0;
    a.ctiles = (int)(((long long)N + BN - 1) / BN);
    a.vec = !(D % 4 || ld % 4 || ((uintptr_t)feats % 16));
    float* wv = static_cast<float*>(ws);
    int* wi = reinterpret_cast<int*>(wv + (long long)a.splits * N * k);
    a.val = a.splits > 1 ? wv : val;
    a.idx = a.splits > 1 ? wi : idx;
    static bool attr[MAXDEV] = {};
    const int dv = cur_dev();
    if (!attr[dv]) {
        (void)hipFuncSetAttribute((const void*)gram_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes(MAXK));
        attr[dv] = true;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned rblocks = (unsigned)(((long long)N + BM - 1) / BM);
    VFM_LAUNCH(gram_topk_kernel, dim3(rblocks, a.splits), dim3(NT), lds_bytes(k), st, a);
    if (a.splits > 1)
        VFM_LAUNCH(topk_merge, dim3((unsigned)(((long long)N + 127) / 128)), dim3(128), 0, st, (const float*)wv,
                   (const int*)wi, N, k, a.splits, val, idx);
    return launch_status();
}

extern "C" long long vfm_cknna_terms_ws(int N) {
    if (N < 1) return VFM_ERR_ARGS;
    const long long blocks = ((long long)N + CN - 1) / CN;
    return (4LL * N + NQ * blocks) * 8;
}

extern "C" int vfm_cknna_terms(const int* idxK, const float* valK, const int* idxL, const float* valL, int N, int k,
                               double* out, void* ws, void* stream) {
    if (!idxK || !valK || !idxL || !valL || !out || !ws || N < 1 || k < 1 || k > N) return VFM_ERR_ARGS;
    if (k > MAXK) return VFM_NO_KERNEL;
    const unsigned blocks = (unsigned)(((long long)N + CN - 1) / CN);
    double* rs = static_cast<double*>(ws);
    double* part = rs + 4LL * N;
    hipStream_t st = (hipStream_t)stream;
    VFM_LAUNCH(cknna_rowsums, dim3(blocks), dim3(CN), 0, st, idxK, valK, idxL, valL, N, k, rs);
    VFM_LAUNCH(cknna_rows, dim3(blocks), dim3(CN), 0, st, idxK, valK, idxL, valL, N, k, (const double*)rs, part);
    VFM_LAUNCH(cknna_finish, dim3(1), dim3(CN), 0, st, (const double*)part, (int)blocks, out);
    return launch_status();
}
