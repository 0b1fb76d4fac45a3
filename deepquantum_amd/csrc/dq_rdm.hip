// k-wire cross reduction on the matrix cores (3 <= k <= 10): the reduced density matrix of a set of wires when both
// inputs are one state, the matrix cotangent of a dense gate otherwise.
//
//     out[b, a, c] = sum_r  gy[b, dep_T(a) | dep_R(r) | cmask] * conj(x[b, dep_T(c) | dep_R(r) | cmask])
//
// T = the k target bits (matrix MSB = targets[0]), the controls fixed at 1, R = the other n - k - nc bits.  A complex
// GEMM C = Y X^H with M = N = 2^k and a contraction of K = 2^(n-k-nc).  Same instructions as dq_dense.hip:
// v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, four real products per complex block (Cr += Yr Xr + Yi Xi,
// Ci += Yi Xr - Yr Xi).  Y and X have the same operand layout (row on lane & 15, contraction on lane >> 4).
//
// Geometry.  Internally the matrix index is re-ordered so that its bit q is the q-th lowest target position; the finish
// kernel maps it back to the caller's order.  An output tile is TT x TT (TT = 64, or 32 / 16 for k = 5 / k <= 4, rows
// past 2^k padded with zeros) and covers the tile's lowest internal row bits.  A stage is a chunk of KC = 1024 / TT
// contraction indices taken from the LOWEST rest bits, so the sub-cube a stage loads (tile target bits + chunk rest
// bits, 1024 amplitudes per operand) is read in runs of at least 16 amplitudes whatever the target positions (the
// lowest index bit outside the sub-cube has every tile bit or every chunk bit below it; a control bit excepted).
// Thread t loads sub-cube elements t + 256 i (i < 4), the element's bits ordered by index position: consecutive lanes,
// consecutive addresses.  Its offsets are computed once per thread; a chunk moves a uniform base over the remaining
// rest bits (next subset of a mask: two scalar operations).  Chunks go through LDS as re / im planes, the next one
// already in flight in registers while the MFMAs of this one run (the scheme of dq_dense.hip).
//
// Waves: TT = 64 -- 2 x 2 waves of 32 x 32; TT = 32 / 16 -- every wave owns the whole tile and a quarter of each
// chunk's contraction, the four partial tiles added through LDS in a fixed order.  complex64 accumulates at most 4096
// terms in f32 (RDM_FLUSH chunks), then adds into double registers.  Every workgroup writes one fixed-order partial
// (one output tile, one contraction split) and the finish kernel adds the splits in a fixed order: no atomics, bitwise
// reproducible.  x == gy (a reduced density matrix) computes only the tiles on or above the diagonal, a diagonal tile
// loads its operand once, and the finish kernel writes the lower triangle as the exact conjugate of the upper one:
// the result is exactly Hermitian.
#include "dq_common.hpp"

namespace dq {

namespace {

constexpr int RDM_THREADS = 256;
constexpr int RDM_SUB = 10;            // log2 (TT * KC): sub-cube bits of one stage
constexpr int RDM_KMIN = 3, RDM_KMAX = 10;
constexpr int RDM_FLUSH = 256;         // complex64: chunks between f32 -> double flushes (<= 4096 terms per accumulator)
constexpr int RDM_TARGET_WG = 2048;    // contraction splits until this many workgroups (8 per CU) ...
constexpr int RDM_MIN_CHUNKS = 4;      // ... while every split keeps this many chunks

struct RdmGeom {
    int n, k, tbits;
    int sub_pos[RDM_SUB];      // element bit j -> index bit position (-1: padding, the element is zero)
    int sub_kind[RDM_SUB];     // element bit j -> internal row bit (0 .. tbits-1), or 16 + chunk bit
    int hi_tpos[RDM_KMAX];     // internal row bits tbits .. k-1 (the tile index) -> positions
    int nhi;
    int umap[RDM_KMAX];        // caller's matrix bit k-1-i (targets[i]) -> internal row bit
    uint64_t cmask;            // control bits
    uint64_t rest_hi;          // rest bits above the chunk
    uint64_t nch;              // chunks per split
    int nt;                    // tiles per matrix side
    int dt;                    // valid rows of a tile (min(2^k, TT))
    int ntl;                   // tile slots per (sample, split)
    int nsplit;
    int herm;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Mfma;
template <> struct Mfma<float> {
    using acc_t = f32x4;
    static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int l, int reg) { return (l >> 4) * 4 + reg; }
};
template <> struct Mfma<double> {
    using acc_t = f64x4;
    static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int l, int reg) { return (l >> 4) + 4 * reg; }   // (f64 has its own map)
};

// tile index -> offset of its high internal row bits
__device__ __forceinline__ uint64_t tile_offset(int t, const RdmGeom& g) {
    uint64_t o = 0;
    for (int q = 0; q < g.nhi; ++q) o |= (uint64_t)((t >> q) & 1) << g.hi_tpos[q];
    return o;
}

// part: [batch, nsplit, ntl, dt, dt] complex double.  grid = (ntl, nsplit, batch)
template <typename T, int TT>
__global__ __launch_bounds__(RDM_THREADS) void rdmk_kernel(const cx<T>* __restrict__ x, const cx<T>* __restrict__ gy,
                                                           RdmGeom g, double* __restrict__ part) {
    constexpr int KC = 1024 / TT;
    constexpr int WR = TT == 64 ? 2 : 1, WK = 4 / (WR * WR), WT = TT / WR, BB = WT / 16;
    constexpr int KS = KC / 4 / WK;                          // k steps of 4 per wave per chunk
    constexpr int LDA = KC + ((KC & 31) ? 1 : 17);           // row stride = 17 mod 32: conflict-free operand reads
    constexpr int PL = TT * LDA;
    constexpr int E = TT * KC / RDM_THREADS;                 // 4 elements per operand per thread
    constexpr int SM_T = 4 * PL * (int)sizeof(T), SM_R = WK > 1 ? TT * TT * 2 * 8 : 0;
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    __shared__ double smem[(SM_T > SM_R ? SM_T : SM_R) / 8];
    T* sYr = reinterpret_cast<T*>(smem);
    T* sYi = sYr + PL;
    T* sXr = sYi + PL;
    T* sXi = sXr + PL;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = WR == 2 ? (wave & 1) : 0, wc = WR == 2 ? (wave >> 1) : 0, wk = WR == 2 ? 0 : wave;
    const int l15 = lane & 15, l4 = lane >> 4;

    // tile (ti, tj): row-major, or the upper triangle row by row when Hermitian
    int ti = 0, tj = 0;
    {
        int t = (int)blockIdx.x;
        if (g.herm) {
            while (t >= g.nt - ti) {
                t -= g.nt - ti;
                ++ti;
            }
            tj = ti + t;
        } else {
            ti = t / g.nt;
            tj = t % g.nt;
        }
    }
    const bool diag = g.herm && ti == tj;     // one operand: X's planes are Y's
    const uint64_t sample = (uint64_t)blockIdx.z << g.n;
    const cx<T>* pg = gy + sample + tile_offset(ti, g);
    const cx<T>* px = x + sample + tile_offset(tj, g);

    // this thread's sub-cube elements: LDS slot, offset, zero padding
    int sidx[E];
    uint64_t off[E];
    unsigned okm = 0;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = tid + RDM_THREADS * i;
        int rl = 0, cl = 0;
        uint64_t o = g.cmask;
        bool ok = true;
        for (int j = 0; j < RDM_SUB; ++j) {
            const int bit = (e >> j) & 1;
            const int kind = g.sub_kind[j];
            if (kind >= 16) cl |= bit << (kind - 16);
            else rl |= bit << kind;
            if (g.sub_pos[j] >= 0) o |= (uint64_t)bit << g.sub_pos[j];
            else if (bit) ok = false;
        }
        sidx[i] = rl * LDA + cl;
        off[i] = o;
        okm |= (ok ? 1u : 0u) << i;
    }

    // first chunk of this split: deposit its index into the rest bits above the chunk
    uint64_t cbase = 0;
    {
        const uint64_t c0 = (uint64_t)blockIdx.y * g.nch;
        uint64_t m = g.rest_hi;
        for (int j = 0; m; ++j) {
            const uint64_t low = m & (~m + 1ull);
            if ((c0 >> j) & 1ull) cbase |= low;
            m ^= low;
        }
    }

    cx<T> qy[E], qx[E];
    auto fetch = [&](uint64_t cb) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < E; ++i) qy[i] = ((okm >> i) & 1u) ? pg[cb | off[i]] : mk<T>(0, 0);
        if (!diag) {
#pragma unroll
            for (int i = 0; i < E; ++i) qx[i] = ((okm >> i) & 1u) ? px[cb | off[i]] : mk<T>(0, 0);
        }
    };
    auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < E; ++i) {
            sYr[sidx[i]] = qy[i].x;
            sYi[sidx[i]] = qy[i].y;
        }
        if (!diag) {
#pragma unroll
            for (int i = 0; i < E; ++i) {
                sXr[sidx[i]] = qx[i].x;
                sXi[sidx[i]] = qx[i].y;
            }
        }
    };
    const T* oXr = diag ? sYr : sXr;
    const T* oXi = diag ? sYi : sXi;

    acc_t cr[BB][BB], ci[BB][BB];
    double dr[BB][BB][4], di[BB][BB][4];
#pragma unroll
    for (int a = 0; a < BB; ++a)
#pragma unroll
        for (int b = 0; b < BB; ++b) {
            cr[a][b] = ci[a][b] = acc_t{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) dr[a][b][r] = di[a][b][r] = 0.0;
        }
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < BB; ++a)
#pragma unroll
            for (int b = 0; b < BB; ++b) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dr[a][b][r] += (double)cr[a][b][r];
                    di[a][b][r] += (double)ci[a][b][r];
                }
                cr[a][b] = ci[a][b] = acc_t{0, 0, 0, 0};
            }
    };

    fetch(cbase);
    for (uint64_t c = 0; c < g.nch; ++c) {
        __syncthreads();                            // everybody is done with the previous chunk
        stash();
        __syncthreads();
        if (c + 1 < g.nch) {                        // the next chunk is in flight while the matrix cores work
            cbase = (cbase - g.rest_hi) & g.rest_hi;
            fetch(cbase);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int kk = (wk * KS + s) * 4 + l4;
            T ar[BB], ai[BB], nar[BB], br[BB], bi[BB];
#pragma unroll
            for (int a = 0; a < BB; ++a) {          // A[i = l & 15][k = l >> 4] = Y
                const int r = wr * WT + a * 16 + l15;
                ar[a] = sYr[r * LDA + kk];
                ai[a] = sYi[r * LDA + kk];
                nar[a] = -ar[a];
            }
#pragma unroll
            for (int b = 0; b < BB; ++b) {          // B[k = l >> 4][j = l & 15] = conj(X)^T
                const int r = wc * WT + b * 16 + l15;
                br[b] = oXr[r * LDA + kk];
                bi[b] = oXi[r * LDA + kk];
            }
#pragma unroll
            for (int a = 0; a < BB; ++a)
#pragma unroll
                for (int b = 0; b < BB; ++b) {
                    cr[a][b] = M::run(ar[a], br[b], cr[a][b]);
                    ci[a][b] = M::run(ai[a], br[b], ci[a][b]);
                }
#pragma unroll
            for (int a = 0; a < BB; ++a)
#pragma unroll
                for (int b = 0; b < BB; ++b) {
                    cr[a][b] = M::run(ai[a], bi[b], cr[a][b]);
                    ci[a][b] = M::run(nar[a], bi[b], ci[a][b]);
                }
        }
        if constexpr (sizeof(T) == 4)
            if ((c & (RDM_FLUSH - 1)) == RDM_FLUSH - 1) flush();
    }
    if constexpr (sizeof(T) == 4) flush();
    else {
#pragma unroll
        for (int a = 0; a < BB; ++a)
#pragma unroll
            for (int b = 0; b < BB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dr[a][b][r] = cr[a][b][r];
                    di[a][b][r] = ci[a][b][r];
                }
    }

    const int dt = g.dt;
    double* dst = part + ((((uint64_t)blockIdx.z * g.nsplit + blockIdx.y) * g.ntl + blockIdx.x) * (uint64_t)(dt * dt)) * 2;
    if constexpr (WK == 1) {
#pragma unroll
        for (int a = 0; a < BB; ++a)
#pragma unroll
            for (int b = 0; b < BB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = wr * WT + a * 16 + M::row(lane, r), j = wc * WT + b * 16 + l15;
                    if (i < dt && j < dt) {
                        dst[(i * dt + j) * 2] = dr[a][b][r];
                        dst[(i * dt + j) * 2 + 1] = di[a][b][r];
                    }
                }
    } else {
        // the waves' partial tiles, added in wave order through LDS (the staging planes are free again)
        double* red = smem;
#pragma unroll
        for (int w = 0; w < WK; ++w) {
            __syncthreads();
            if (wave == w) {
#pragma unroll
                for (int a = 0; a < BB; ++a)
#pragma unroll
                    for (int b = 0; b < BB; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = a * 16 + M::row(lane, r), j = b * 16 + l15;
                            double* p = red + (i * TT + j) * 2;
                            p[0] = w == 0 ? dr[a][b][r] : p[0] + dr[a][b][r];
                            p[1] = w == 0 ? di[a][b][r] : p[1] + di[a][b][r];
                        }
            }
        }
        __syncthreads();
        for (int e = tid; e < dt * dt; e += RDM_THREADS) {
            const int i = e / dt, j = e % dt;
            dst[e * 2] = red[(i * TT + j) * 2];
            dst[e * 2 + 1] = red[(i * TT + j) * 2 + 1];
        }
    }
}

// out[b, a, c] (caller's order) = sum over the splits, in split order; the Hermitian route mirrors the lower triangle
__global__ __launch_bounds__(RDM_THREADS) void rdmk_finish_kernel(const double* __restrict__ part, RdmGeom g,
                                                                   double* __restrict__ out) {
    const int D = 1 << g.k;
    const int idx = blockIdx.x * RDM_THREADS + threadIdx.x;
    if (idx >= D * D) return;
    const uint64_t b = blockIdx.y;
    const int a = idx >> g.k, c = idx & (D - 1);
    int ai = 0, ci = 0;
    for (int i = 0; i < g.k; ++i) {
        ai |= ((a >> (g.k - 1 - i)) & 1) << g.umap[i];
        ci |= ((c >> (g.k - 1 - i)) & 1) << g.umap[i];
    }
    bool mirror = false;
    if (g.herm && ai > ci) {
        const int t = ai;
        ai = ci;
        ci = t;
        mirror = true;
    }
    const int dt = g.dt;
    const int ti = ai / dt, tj = ci / dt, li = ai % dt, lj = ci % dt;
    const int slot = g.herm ? ti * g.nt - ti * (ti - 1) / 2 + (tj - ti) : ti * g.nt + tj;
    const uint64_t tsz = (uint64_t)dt * dt;
    const double* p = part + ((b * g.nsplit * g.ntl + slot) * tsz + (uint64_t)(li * dt + lj)) * 2;
    double re = 0.0, im = 0.0;
    for (int s = 0; s < g.nsplit; ++s) {
        re += p[0];
        im += p[1];
        p += g.ntl * tsz * 2;
    }
    if (g.herm && ai == ci) im = 0.0;
    double* o = out + (b * (uint64_t)(D * D) + idx) * 2;
    o[0] = re;
    o[1] = mirror ? -im : im;
}

int rdm_tile(int k) { return k >= 6 ? 64 : (k == 5 ? 32 : 16); }

// contraction splits and workspace (doubles); depends on the shape only
int64_t rdm_plan(int n, int k, int nc, int64_t batch, bool c128, bool herm, int* nsplit_out, uint64_t* nch_out) {
    const int TT = rdm_tile(k), tbits = __builtin_ctz(TT), cbits = RDM_SUB - tbits;
    const int64_t D = 1ll << k;
    const int dt = (int)(D < TT ? D : TT), nt = (int)(D / dt);
    const int64_t ntl = herm ? (int64_t)nt * (nt + 1) / 2 : (int64_t)nt * nt;
    const int R = n - k - nc;
    const uint64_t total = R > cbits ? 1ull << (R - cbits) : 1ull;
    const int64_t per_split = batch * ntl * dt * dt * 2;
    const int64_t state_bytes = (batch << n) * (c128 ? 16 : 8);
    const int64_t budget = (batch * D * D * 16 + state_bytes / 100) / 8;     // (output + workspace <= 2 x output + 1 %)
    int64_t ns = 1;
    while ((uint64_t)(ns * 2) * RDM_MIN_CHUNKS <= total && per_split * ns * 2 <= budget && batch * ntl * ns < RDM_TARGET_WG)
        ns *= 2;
    if (nsplit_out) *nsplit_out = (int)ns;
    if (nch_out) *nch_out = total / (uint64_t)ns;
    return per_split * ns;
}

template <typename T>
int rdmk_cross_impl(const void* x, const void* gy, int n, const int* targets, int k, const int* controls, int nc,
                    int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    if (!x || !gy || !out || batch < 1 || batch > 65535) {
        set_error("dq_rdmk_cross: bad argument (null pointer, or batch=%lld outside [1, 65535])", (long long)batch);
        return DQ_ERR_ARG;
    }
    if (k < RDM_KMIN || k > RDM_KMAX) {
        set_error("dq_rdmk_cross: k=%d unsupported (%d..%d)", k, RDM_KMIN, RDM_KMAX);
        return DQ_ERR_UNSUPPORTED;
    }
    int rc = validate_bits(n, targets, k, controls, nc);
    if (rc) return rc;
    const bool herm = x == gy;
    int nsplit = 1;
    uint64_t nch = 1;
    const int64_t need = rdm_plan(n, k, nc, batch, sizeof(T) == 8, herm, &nsplit, &nch) * (int64_t)sizeof(double);
    if (!ws || ws_bytes < need) {
        set_error("dq_rdmk_cross: workspace of %lld bytes, %lld needed (dq_rdmk_ws_bytes)", (long long)ws_bytes,
                  (long long)need);
        return DQ_ERR_ARG;
    }
    const int TT = rdm_tile(k), tbits = __builtin_ctz(TT), cbits = RDM_SUB - tbits;
    const int D = 1 << k, R = n - k - nc;
    RdmGeom g{};
    g.n = n;
    g.k = k;
    g.tbits = tbits;
    // target positions ascending = internal row bits; the caller's bit k-1-i is targets[i]
    int spos[RDM_KMAX];
    for (int i = 0; i < k; ++i) spos[i] = targets[i];
    for (int i = 1; i < k; ++i)
        for (int j = i; j > 0 && spos[j - 1] > spos[j]; --j) {
            const int t = spos[j];
            spos[j] = spos[j - 1];
            spos[j - 1] = t;
        }
    for (int i = 0; i < k; ++i)
        for (int q = 0; q < k; ++q)
            if (spos[q] == targets[i]) g.umap[i] = q;
    uint64_t used = 0;
    for (int i = 0; i < k; ++i) used |= 1ull << targets[i];
    for (int i = 0; i < nc; ++i) {
        used |= 1ull << controls[i];
        g.cmask |= 1ull << controls[i];
    }
    int rpos[40], nr = 0;
    for (int p = 0; p < n; ++p)
        if (!((used >> p) & 1ull)) rpos[nr++] = p;
    (void)R;
    // sub-cube bits: the real ones by position, then the padding
    int pos[RDM_SUB], kind[RDM_SUB], m = 0;
    for (int q = 0; q < tbits && q < k; ++q) pos[m] = spos[q], kind[m++] = q;
    for (int q = 0; q < cbits && q < nr; ++q) pos[m] = rpos[q], kind[m++] = 16 + q;
    for (int i = 1; i < m; ++i)
        for (int j = i; j > 0 && pos[j - 1] > pos[j]; --j) {
            int t = pos[j];
            pos[j] = pos[j - 1];
            pos[j - 1] = t;
            t = kind[j];
            kind[j] = kind[j - 1];
            kind[j - 1] = t;
        }
    for (int q = k; q < tbits; ++q) pos[m] = -1, kind[m++] = q;
    for (int q = nr; q < cbits; ++q) pos[m] = -1, kind[m++] = 16 + q;
    for (int j = 0; j < RDM_SUB; ++j) g.sub_pos[j] = pos[j], g.sub_kind[j] = kind[j];
    g.nhi = k > tbits ? k - tbits : 0;
    for (int q = 0; q < g.nhi; ++q) g.hi_tpos[q] = spos[tbits + q];
    for (int q = cbits; q < nr; ++q) g.rest_hi |= 1ull << rpos[q];
    g.nch = nch;
    g.dt = D < TT ? D : TT;
    g.nt = D / g.dt;
    g.ntl = herm ? g.nt * (g.nt + 1) / 2 : g.nt * g.nt;
    g.nsplit = nsplit;
    g.herm = herm ? 1 : 0;

    hipStream_t s = as_stream(stream);
    const cx<T>* px = static_cast<const cx<T>*>(x);
    const cx<T>* pgy = static_cast<const cx<T>*>(gy);
    double* part = static_cast<double*>(ws);
    const dim3 grid((unsigned)g.ntl, (unsigned)nsplit, (unsigned)batch);
    if (TT == 64) hipLaunchKernelGGL((rdmk_kernel<T, 64>), grid, dim3(RDM_THREADS), 0, s, px, pgy, g, part);
    else if (TT == 32) hipLaunchKernelGGL((rdmk_kernel<T, 32>), grid, dim3(RDM_THREADS), 0, s, px, pgy, g, part);
    else hipLaunchKernelGGL((rdmk_kernel<T, 16>), grid, dim3(RDM_THREADS), 0, s, px, pgy, g, part);
    hipLaunchKernelGGL(rdmk_finish_kernel, dim3((unsigned)((D * D + RDM_THREADS - 1) / RDM_THREADS), (unsigned)batch),
                       dim3(RDM_THREADS), 0, s, part, g, out);
    return check_launch("dq_rdmk_cross");
}

}  // namespace
}  // namespace dq

extern "C" int64_t dq_rdmk_ws_bytes(int n, int k, int nc, int64_t batch, int is_c128, int hermitian) {
    if (k < dq::RDM_KMIN || k > dq::RDM_KMAX || nc < 0 || n < k + nc || n > 40 || batch < 1) return -1;
    return dq::rdm_plan(n, k, nc, batch, is_c128 != 0, hermitian != 0, nullptr, nullptr) * (int64_t)sizeof(double);
}

extern "C" int dq_rdmk_cross_c64(const void* x, const void* gy, int n, const int* targets, int k, const int* controls,
                                 int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::rdmk_cross_impl<float>(x, gy, n, targets, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_rdmk_cross_c128(const void* x, const void* gy, int n, const int* targets, int k, const int* controls,
                                  int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::rdmk_cross_impl<double>(x, gy, n, targets, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
