// Improved precision / recall without the distance matrix: the device side of metrics/precision_recall.py
// (reference metrics/precision_recall.py:21-63: 10 000 x 10 000 torch.cdist blocks, cloned, copied to the
// host block by block, `kthvalue(nhood_size + 1)` and `(dist <= kth).any(dim=1)` there).
//
// dist_kernel<MODE>: "row block x all columns of its split" as in knn.hip -- a GEMM that never writes its
// output. A workgroup (256 threads, 2 x 2 waves) owns BM = 128 rows and walks BN = 128 wide column tiles.
// Both operands are K-contiguous fp16 rows, staged per 32-wide K-tile into LDS ([row][40 halves], the next
// K-tile travelling to registers during the products) and multiplied on v_mfma_f32_32x32x16_f16: fp16 x fp16
// products are exact in fp32, one fp32 accumulator per pair over the whole of D, so a distance's bits do not
// depend on the tile or split it is computed in. d2 = max((|a|^2 + |b|^2) - 2 a.b, 0) in fp32, the squared
// norms from row_norms (fp32, fixed order).
//   RADIUS: the rows are a slice of the column matrix. d2 goes to an LDS score tile (it aliases the staging
//     buffer); phase 1 (all threads): thread (row, half) leaves a 64-bit mask of the columns below the row's
//     current (k + 1)-th smallest value; phase 2 (128 row owners): the candidates fill the row's list in LDS
//     ([slot][row], values only: a tie needs no order) or replace its largest entry. Each split writes its
//     rows' lists ascending (+inf padded) to the workspace; radius_merge takes the (k + 1)-th smallest of a
//     row's lists, and stores half(sqrtf(d2)): sqrtf is correctly rounded and monotone, so this is the
//     reference's `dist.float().kthvalue(k + 1).values.half()`.
//   HITS: rows are probes, columns the manifold. hit(i) |= sqrtf(d2(i, j)) <= float(radii[j]), kept as one
//     flag per row in LDS (wave ballots); a workgroup stops walking columns once all its rows have hit.
//     Each split writes a byte per row; hits_finish ORs the splits and leaves the mean of the flags
//     (count / P in fp32, as `pred.float().mean()`) on the device. Integer counts: no order dependence.
#include "vfm_common.h"

namespace {

using namespace vfm;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int BM = 128, BN = 128, BK = 32, NT = 256;
constexpr int LDH = BK + 8;                // staged row stride in halves (80 B: 16-B aligned, banks spread)
constexpr int SS = BN + 1;                 // score tile row stride (floats)
constexpr int MAXK1 = 64, MAXSPLITS = 64;  // k + 1 <= 64: the LDS list bound knn.hip has
constexpr int TARGET_WG = 512;

enum { RADIUS = 0, HITS = 1 };

struct DistArgs {
    const __half* p;                       // rows [P][ldp]
    const __half* m;                       // columns [N][ldm]
    long long ldp, ldm;
    int P, N, D, k1;
    int tps, ctiles;                       // column tiles per split, column tiles in all
    int vec;                               // both matrices loadable as 16-B chunks
    const float* np;                       // [P] squared norms of the rows
    const float* nm;                       // [N] squared norms of the columns
    const __half* rad;                     // HITS: [N]
    float* part;                           // RADIUS: [splits][P][k1]
    unsigned char* hpart;                  // HITS: [splits][P]
};

// one operand K-tile (128 rows x 32 halves) global -> registers -> LDS [row][LDH]
struct Stage {
    static constexpr int HALVES = BM * LDH;
    static constexpr int PER = BM * BK / 8 / NT;               // 16-B chunks per thread
    uint4 r[PER];

    __device__ __forceinline__ void load(const __half* f, long long ld, int rows, int D, int vec, unsigned row0, int k0,
                                         int tid) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int c = tid + NT * u;
            const unsigned o = row0 + (c >> 2);
            const int k = k0 + (c & 3) * 8;
            const __half* p = f + (long long)o * ld + k;
            if (vec) {
                // branch-free bounds: an out-of-range chunk loads the matrix's first chunk and is zeroed
                const bool ok = o < (unsigned)rows && k < D;
                const uint4 v = *reinterpret_cast<const uint4*>(ok ? p : f);
                r[u] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
            } else {
                unsigned short e[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    e[i] = (o < (unsigned)rows && k + i < D) ? *reinterpret_cast<const unsigned short*>(p + i) : 0;
                r[u] = make_uint4(e[0] | (unsigned)e[1] << 16, e[2] | (unsigned)e[3] << 16, e[4] | (unsigned)e[5] << 16,
                                  e[6] | (unsigned)e[7] << 16);
            }
        }
    }

    __device__ __forceinline__ void store(__half* img, int tid) const {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int c = tid + NT * u;
            *reinterpret_cast<uint4*>(img + (c >> 2) * LDH + (c & 3) * 8) = r[u];
        }
    }

    // k-step s (16 wide) fragment of the lane's row orow + (lane & 31): k = 16 s + 8 (lane >> 5) + 0..7
    __device__ __forceinline__ static f16x8 frag(const __half* img, int lane, int orow, int s) {
        return *reinterpret_cast<const f16x8*>(img + (orow + (lane & 31)) * LDH + 16 * s + 8 * (lane >> 5));
    }
};

constexpr int STAGE_BYTES = 2 * Stage::HALVES * 2;             // both operands of one K-tile
constexpr int TILE_BYTES = BM * SS * 4;                        // RADIUS: the score tile aliases the staging buffer
static_assert(TILE_BYTES >= STAGE_BYTES, "the score tile covers the staging buffer");
// after the tile / staging area: np of the block's rows [BM], then per mode
//   RADIUS: cmask [2][BM] u64, thr [BM], list [k1][BM]      HITS: hit [BM] int
inline size_t lds_bytes(int mode, int k1) {
    return mode == RADIUS ? (size_t)TILE_BYTES + BM * 4 + 2 * BM * 8 + BM * 4 + (size_t)k1 * BM * 4
                          : (size_t)STAGE_BYTES + BM * 4 + BM * 4;
}

template <int MODE>
__global__ __launch_bounds__(NT, 2) void dist_kernel(DistArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __half* sA = reinterpret_cast<__half*>(smem);
    __half* sB = sA + Stage::HALVES;
    float* score = reinterpret_cast<float*>(smem);
    float* rown = reinterpret_cast<float*>(smem + (MODE == RADIUS ? TILE_BYTES : STAGE_BYTES));   // [BM]
    u64* cmask = reinterpret_cast<u64*>(rown + BM);            // RADIUS [2][BM]
    float* thr = reinterpret_cast<float*>(cmask + 2 * BM);     // RADIUS [BM]: the row's largest kept value
    float* lval = thr + BM;                                    // RADIUS [k1][BM]
    int* hit = reinterpret_cast<int*>(rown + BM);              // HITS [BM]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const unsigned m0 = blockIdx.x * (unsigned)BM;
    const int split = blockIdx.y;
    const int ct0 = split * a.tps, ct1 = min(a.ctiles, ct0 + a.tps);
    const int kt = (a.D + BK - 1) / BK;
    const float INF = __builtin_inff();

    int cnt = 0, worst = 0;                                    // RADIUS row owners (tid < BM): entries, slot of the largest
    if (tid < BM) {
        rown[tid] = m0 + tid < (unsigned)a.P ? a.np[m0 + tid] : 0.f;
        if (MODE == RADIUS) thr[tid] = INF;
        else hit[tid] = m0 + tid < (unsigned)a.P ? 0 : 1;      // rows past the end never keep the block walking
    }
    __syncthreads();

    Stage sa, sb;
    for (int ct = ct0; ct < ct1; ++ct) {
        const unsigned n0 = (unsigned)ct * BN;
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

        sa.load(a.p, a.ldp, a.P, a.D, a.vec, m0, 0, tid);
        sb.load(a.m, a.ldm, a.N, a.D, a.vec, n0, 0, tid);
        for (int u = 0; u < kt; ++u) {
            sa.store(sA, tid);
            sb.store(sB, tid);
            __syncthreads();
            if (u + 1 < kt) {                                  // K-tile u + 1 travels while tile u is multiplied
                sa.load(a.p, a.ldp, a.P, a.D, a.vec, m0, (u + 1) * BK, tid);
                sb.load(a.m, a.ldm, a.N, a.D, a.vec, n0, (u + 1) * BK, tid);
            }
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
                f16x8 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = Stage::frag(sA, lane, 64 * wm + 32 * i, s);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = Stage::frag(sB, lane, 64 * wn + 32 * j, s);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();                                   // every wave has read tile u: the stage is free
        }

        // acc[i][j][e] = <p[m0 + m], m[n0 + n]>: m = 64 wm + 32 i + (e & 3) + 8 (e >> 2) + 4 (lane >> 5),
        // n = 64 wn + 32 j + (lane & 31)
        const int r = lane & 31, hh = lane >> 5;
        float nb[2], rd[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned gn = n0 + 64 * wn + 32 * j + r;
            const bool ok = gn < (unsigned)a.N;
            nb[j] = ok ? a.nm[gn] : 0.f;
            if (MODE == HITS) rd[j] = ok ? __half2float(a.rad[gn]) : -1.f;   // a column past the end never hits
        }
        if (MODE == RADIUS) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int m = 64 * wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hh;
                        score[m * SS + 64 * wn + 32 * j + r] = fmaxf((rown[m] + nb[j]) - 2.f * acc[i][j][e], 0.f);
                    }
            __syncthreads();

            // phase 1: candidate mask of (row, half)
            {
                const int row = tid & (BM - 1), half = tid >> 7;
                const unsigned gi = m0 + row, c0 = n0 + 64 * half;
                const float t = thr[row];
                const float* s = score + row * SS + 64 * half;
                u64 m = 0;
#pragma unroll 16
                for (int c = 0; c < 64; ++c) m |= (u64)(s[c] < t) << c;
                u64 ok = 0;
                if (gi < (unsigned)a.P && c0 < (unsigned)a.N) {
                    const unsigned nc = (unsigned)a.N - c0;
                    ok = nc >= 64 ? ~0ull : (1ull << nc) - 1;
                }
                cmask[half * BM + row] = m & ok;
            }
            __syncthreads();

            // phase 2: the row owners insert their candidates
            if (tid < BM) {
                const int k1 = a.k1;
                float cur = thr[tid];
                for (int half = 0; half < 2; ++half) {
                    u64 m = cmask[half * BM + tid];
                    while (m) {
                        const int c = __builtin_ctzll(m) + 64 * half;
                        m &= m - 1;
                        const float v = score[tid * SS + c];
                        if (cnt == k1 && !(v < cur)) continue;
                        const int p = cnt < k1 ? cnt++ : worst;
                        lval[p * BM + tid] = v;
                        if (cnt == k1) {                       // the new largest entry (k1 independent LDS reads)
                            cur = lval[tid];
                            worst = 0;
                            for (int q = 1; q < k1; ++q) {
                                const float vq = lval[q * BM + tid];
                                if (vq > cur) { cur = vq; worst = q; }
                            }
                        }
                    }
                }
                thr[tid] = cur;
            }
            __syncthreads();                                   // the next tile's staging overwrites the scores
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = 64 * wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    const float na = rown[m];
                    bool h = false;
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        h |= sqrtf(fmaxf((na + nb[j]) - 2.f * acc[i][j][e], 0.f)) <= rd[j];
                    const u64 b = __ballot(h);                 // lanes 0-31: row m of hh = 0, lanes 32-63: hh = 1
                    if (lane == 0) {
                        const int mlo = 64 * wm + 32 * i + (e & 3) + 8 * (e >> 2);
                        if (b & 0xffffffffull) hit[mlo] = 1;   // the two column waves may both store the same 1
                        if (b >> 32) hit[mlo + 4] = 1;
                    }
                }
            __syncthreads();
            const int all = __syncthreads_and(tid < BM ? hit[tid] : 1);
            if (all) break;                                    // uniform over the block
        }
    }

    if (MODE == RADIUS) {
        if (tid < BM && m0 + tid < (unsigned)a.P) {
            float* out = a.part + ((long long)split * a.P + (m0 + tid)) * a.k1;
            // ascending; an entry's place is the number of entries ahead of it (equal values by slot)
            for (int p = 0; p < cnt; ++p) {
                const float v = lval[p * BM + tid];
                int rank = 0;
                for (int q = 0; q < cnt; ++q) {
                    const float vq = lval[q * BM + tid];
                    rank += (vq < v || (vq == v && q < p)) ? 1 : 0;
                }
                out[rank] = v;
            }
            for (int p = cnt; p < a.k1; ++p) out[p] = INF;
        }
    } else {
        if (tid < BM && m0 + tid < (unsigned)a.P) a.hpart[(long long)split * a.P + (m0 + tid)] = (unsigned char)hit[tid];
    }
}

// |x_r|^2 in fp32: one wave per row, lane l sums k = l, l + 64, ... in order, then a fixed shuffle tree
__global__ __launch_bounds__(NT) void row_norms(const __half* __restrict__ f, long long ld, int N, int D,
                                                float* __restrict__ out) {
    const long long row = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const __half* p = f + row * ld;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float v = __half2float(p[k]);
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) out[row] = s;
}

// the k1-th smallest of a row's S ascending lists: k1 rounds of "smallest head", one thread per row
__global__ __launch_bounds__(128) void radius_merge(const float* __restrict__ part, int N, int k1, int S,
                                                    __half* __restrict__ radii) {
    __shared__ unsigned char pos[MAXSPLITS][128];
    const int t = threadIdx.x;
    const long long row = (long long)blockIdx.x * 128 + t;
    if (row >= N) return;
    for (int s = 0; s < S; ++s) pos[s][t] = 0;
    float last = __builtin_inff();
    for (int o = 0; o < k1; ++o) {
        float bv = __builtin_inff();
        int bs = 0;
        for (int s = 0; s < S; ++s) {
            const int p = pos[s][t];
            if (p >= k1) continue;
            const float v = part[((long long)s * N + row) * k1 + p];
            if (v < bv) { bv = v; bs = s; }
        }
        last = bv;                                             // +inf only with fewer than k1 columns: refused above
        ++pos[bs][t];
    }
    radii[row] = __float2half(sqrtf(last));
}

__global__ __launch_bounds__(NT) void hits_finish(const unsigned char* __restrict__ hpart, int P, int S,
                                                  unsigned char* __restrict__ hits, float* __restrict__ mean) {
    __shared__ unsigned red[NT / 64];
    unsigned n = 0;
    for (long long i = threadIdx.x; i < P; i += NT) {
        unsigned char h = 0;
        for (int s = 0; s < S; ++s) h |= hpart[(long long)s * P + i];
        hits[i] = h;
        n += h;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0;
        for (int w = 0; w < NT / 64; ++w) tot += red[w];
        *mean = (float)tot / (float)P;
    }
}

// the fewest column splits whose grid fills >= 0.9 of its rounds of TARGET_WG workgroups (knn.hip's rule)
bool plan_splits(long long rows, long long cols, int splits, int* chosen, int* tps_out) {
    if (rows < 1 || cols < 1 || splits < 0 || rows >= (1LL << 31) || cols >= (1LL << 31)) return false;
    const int ctiles = (int)((cols + BN - 1) / BN);
    const long long rblocks = (rows + BM - 1) / BM;
    const int smax = ctiles < MAXSPLITS ? ctiles : MAXSPLITS;
    int s = splits < smax ? splits : smax;
    if (splits == 0) {
        double best = -1.0;
        for (int c = 1; c <= smax; ++c) {
            const int t = (ctiles + c - 1) / c;
            const long long wgs = rblocks * ((ctiles + t - 1) / t);
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

inline long long align16(long long b) { return (b + 15) / 16 * 16; }

template <int MODE>
void launch_dist(const DistArgs& a, int splits, hipStream_t st) {
    static bool attr[MAXDEV] = {};
    const int dv = cur_dev();
    if (!attr[dv]) {
        (void)hipFuncSetAttribute((const void*)dist_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes(MODE, MAXK1));
        attr[dv] = true;
    }
    const unsigned rblocks = (unsigned)(((long long)a.P + BM - 1) / BM);
    VFM_LAUNCH(dist_kernel<MODE>, dim3(rblocks, splits), dim3(NT), lds_bytes(MODE, a.k1), st, a);
}

bool vec_ok(const void* p, long long ld, int D) { return !(D % 8 || ld % 8 || ((uintptr_t)p % 16)); }

}  // namespace

extern "C" long long vfm_knn_radius_ws(int N, int k, int nrows, int splits, int* chosen) {
    int s, tps;
    if (k < 0 || k + 1 > MAXK1 || nrows > N || !plan_splits(nrows, N, splits, &s, &tps)) return VFM_ERR_ARGS;
    if (chosen) *chosen = s;
    return align16((long long)N * 4) + (long long)s * nrows * (k + 1) * 4;
}

extern "C" int vfm_knn_radius(const void* feats, long long ld, int N, int D, int k, int row0, int nrows, int splits,
                              void* radii, void* ws, void* stream) {
    if (!feats || !radii || !ws || N < 1 || D < 1 || k < 0 || ld < D || splits < 0) return VFM_ERR_ARGS;
    if (row0 < 0 || nrows < 1 || (long long)row0 + nrows > (long long)N) return VFM_ERR_ARGS;
    if ((long long)k + 1 > (long long)N) return VFM_ERR_ARGS;
    if (k + 1 > MAXK1) return VFM_NO_KERNEL;
    int s, tps;
    if (!plan_splits(nrows, N, splits, &s, &tps)) return VFM_ERR_ARGS;
    float* norms = static_cast<float*>(ws);
    DistArgs a = {};
    a.m = static_cast<const __half*>(feats);
    a.p = a.m + (long long)row0 * ld;
    a.ldp = a.ldm = ld;
    a.P = nrows; a.N = N; a.D = D; a.k1 = k + 1; a.tps = tps;
    a.ctiles = (int)(((long long)N + BN - 1) / BN);
    a.vec = vec_ok(feats, ld, D);                              // ld % 8 == 0: the row slice is aligned as well
    a.nm = norms;
    a.np = norms + row0;
    a.part = reinterpret_cast<float*>(static_cast<char*>(ws) + align16((long long)N * 4));
    hipStream_t st = (hipStream_t)stream;
    VFM_LAUNCH(row_norms, dim3((unsigned)(((long long)N + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, a.m, ld, N, D, norms);
    launch_dist<RADIUS>(a, s, st);
    VFM_LAUNCH(radius_merge, dim3((unsigned)(((long long)nrows + 127) / 128)), dim3(128), 0, st, (const float*)a.part,
               nrows, k + 1, s, static_cast<__half*>(radii));
    return launch_status();
}

extern "C" long long vfm_manifold_hits_ws(int P, int N, int splits, int* chosen) {
    int s, tps;
    if (!plan_splits(P, N, splits, &s, &tps)) return VFM_ERR_ARGS;
    if (chosen) *chosen = s;
    return align16((long long)P * 4) + align16((long long)N * 4) + (long long)s * P;
}

extern "C" int vfm_manifold_hits(const void* probes, long long ldp, int P, const void* manifold, long long ldm, int N,
                                 int D, const void* radii, int splits, unsigned char* hits, float* mean, void* ws,
                                 void* stream) {
    if (!probes || !manifold || !radii || !hits || !mean || !ws || P < 1 || N < 1 || D < 1 || ldp < D || ldm < D ||
        splits < 0)
        return VFM_ERR_ARGS;
    int s, tps;
    if (!plan_splits(P, N, splits, &s, &tps)) return VFM_ERR_ARGS;
    char* w = static_cast<char*>(ws);
    float* np = reinterpret_cast<float*>(w);
    float* nm = reinterpret_cast<float*>(w + align16((long long)P * 4));
    DistArgs a = {};
    a.p = static_cast<const __half*>(probes);
    a.m = static_cast<const __half*>(manifold);
    a.ldp = ldp; a.ldm = ldm;
    a.P = P; a.N = N; a.D = D; a.k1 = 0; a.tps = tps;
    a.ctiles = (int)(((long long)N + BN - 1) / BN);
    a.vec = vec_ok(probes, ldp, D) && vec_ok(manifold, ldm, D);
    a.np = np; a.nm = nm;
    a.rad = static_cast<const __half*>(radii);
    a.hpart = reinterpret_cast<unsigned char*>(w + align16((long long)P * 4) + align16((long long)N * 4));
    hipStream_t st = (hipStream_t)stream;
    VFM_LAUNCH(row_norms, dim3((unsigned)(((long long)P + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, a.p, ldp, P, D, np);
    VFM_LAUNCH(row_norms, dim3((unsigned)(((long long)N + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, a.m, ldm, N, D, nm);
    launch_dist<HITS>(a, s, st);
    VFM_LAUNCH(hits_finish, dim3(1), dim3(NT), 0, st, (const unsigned char*)a.hpart, P, s, hits, mean);
    return launch_status();
}
