// Every sample against every sample: the Gram matrix of two batches of states and linear combinations of a batch.
//
//     dq_gram_*      G[i, j] = sum_x conj(A[i, x]) B[j, x]        A (M, 2^n), B (N, 2^n)  ->  complex128 (M, N)
//     dq_combine_*   Y[m, x] = sum_j C[m, j] S[j, x]              S (N, 2^n), C complex128 (M, N)  ->  Y (M, 2^n)
//
// Both are products of a small matrix and a very tall one: one complex multiply-add per basis index and pair of rows, on
// the matrix cores with exact f32 / f64 products (v_mfma_f32_16x16x4_f32, v_mfma_f64_16x16x4_f64, as dq_dense.hip).  Neither
// splits a state into planes: re and im stay interleaved as stored, and the complex product is two real ones,
//     Re G = A_f . B_f^T          Im G = A_f . (J B_f)^T          J : (re, im) -> (im, -re)
//     Y_f  = C_re . S_f + C_im . (J' S_f)                         J': (re, im) -> (-im, re)
// over the rows as vectors of reals (A_f ..): J and J' are a choice of register and one sign flip inside the lane that
// loaded the pair.
//
// Gram.  A workgroup of 4 waves owns a tile of GR_TILE = 32 rows of A against 32 rows of B (2 x 2 blocks of 16 x 16; up to
// 16 rows on a side the launch uses one block there) and strides over units of x.  The MFMA's row index is the sample, its
// k index runs over the reals of a row: lane (i = l & 15, q = l >> 4) owns GR_VECS = 4 consecutive 16-byte vectors of row
// i -- its segment, 8 complex64 / 4 complex128 columns -- per step, a wave 16 vectors of each row per step (its share: 32 /
// 16 columns), a workgroup GR_STEPS = 4 steps of each wave per unit (512 / 256 columns).  Step s of wave w in unit u is
// vector ((u * 4 + s) * 4 + w) * 16 of the rows.  Real f of the lane's 16 (8) is one MFMA for Re and one for Im per pair
// of blocks, both operands in the same k order.  A lane whose row or vector does not exist feeds 0 and loads nothing: where
// the whole step exists the four loads of a block sit under one test of the row and both operands' loads go out before the
// first MFMA (gram_step), only the tail of a short row tests every vector.
//     complex64:  an f32 accumulator chains the 4 steps of a unit -- 4 steps x 16 MFMAs x 4 = GR_CHAIN = 256 real terms
//                 -- and is then added into a double accumulator; everything after that is in double.
//     complex128: products and sums in f64 on the matrix cores, from the first to the last unit of the wave.
// After its units the workgroup adds its waves in the order 0..3 through LDS and writes the tile's 32 x 32 partial sums to
// the workspace; gram_finish_kernel adds the workgroups of an entry in the order of their index.  No atomics; every sum in
// a fixed order that depends on n, the dtype and the number of workgroups per tile (below) alone: bitwise reproducible,
// and an entry's bits do not depend on the other rows of the launch or on the row's place in it, as long as the number of
// tile pairs is the same (M, N <= 32: one pair).
// Workgroups per tile pair: min(units, GR_BLOCKS, max(1, GR_BLOCKS / pairs)): one pair is spread over the device, a
// thousand pairs (the kernel-methods regime) take a workgroup each and write one partial.
// Rows beyond a tile are tiled: grid = (slice of x, tile of A, tile of B); every row of A is then read ceil(N / 32) times
// and every row of B ceil(M / 32) times.
// A == B with M == N (the self-Gram): tiles with tile_a <= tile_b only (half the reads; a row is read ceil(M / 32) / 2 + 1/2
// times), a diagonal tile loads its rows once and uses them for both operands, the finish kernel mirrors the rest as the
// exact conjugate and writes the diagonal's imaginary part as 0.
//
// Combine.  A workgroup owns CB_TILE = 32 output rows (one or two blocks of 16) and strides over units of 64 vectors, a
// wave taking 16 vectors (256 bytes of every row).  Lane (c = l & 15, k = l >> 4) loads vector c of input row j0 + k: the
// MFMA's row index is the real column (real e of the lane's vector in MFMA e), its k index the input row -- four input
// rows per MFMA -- and its column index the output row, whose coefficient (re for S_f, im for J' S_f) the lane reads from
// an LDS copy of the tile's coefficients, rounded once to the states' precision.  A lane's results are whole 16-byte
// vectors of one output row.  The kernel loops over any N in chunks of CB_CHUNK = 64 input rows (one chunk: the table is
// staged once per workgroup; more: once per unit and chunk); the chain of an output element is 2 N real terms.  S is read
// ceil(M / 32) times, Y written once.
#include "dq_stream.hpp"

namespace dq {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Mfma;
template <> struct Mfma<float> {
    using acc_t = f32x4;
    static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D element `reg` of lane group q = l >> 4: the row inside the 16 x 16 block (the column is l & 15)
    static __device__ __forceinline__ int row(int q, int reg) { return q * 4 + reg; }
};
template <> struct Mfma<double> {
    using acc_t = f64x4;
    static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int q, int reg) { return q + 4 * reg; }   // (f64 has its own map)
};

constexpr int GR_TILE = 32;                             // rows of a tile, either side
constexpr int GR_VECS = 4;                              // 16-byte vectors of a lane per step
constexpr int GR_STEPS = 4;                             // steps of a wave per unit
constexpr int GR_WAVES = 4;
constexpr int GR_WAVE_VECS = 4 * GR_VECS;               // vectors of a row a wave takes per step
constexpr int GR_UNIT_VECS = GR_STEPS * GR_WAVES * GR_WAVE_VECS;      // vectors of a row per workgroup and iteration
constexpr int GR_CHAIN = GR_STEPS * GR_VECS * 4 * 4;    // real terms an f32 accumulator chains (complex64)
constexpr unsigned GR_BLOCKS = 1024;                    // most workgroups per tile pair
constexpr int GR_ENTRIES = GR_TILE * GR_TILE;

constexpr int CB_TILE = 32;                             // output rows of a workgroup
constexpr int CB_CHUNK = 64;                            // input rows whose coefficients LDS holds
constexpr int CB_WAVE_VECS = 16;
constexpr int CB_UNIT_VECS = 4 * CB_WAVE_VECS;
constexpr int CB_AHEAD = 4;                             // groups of four input rows whose loads are in flight together
constexpr unsigned CB_BLOCKS = 2048;                    // most workgroups per tile of output rows

template <typename T> __device__ __forceinline__ T vec_real(const typename Vec16<T>::type& q, int e);
template <> __device__ __forceinline__ float vec_real<float>(const float4& q, int e) {
    return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w;
}
template <> __device__ __forceinline__ double vec_real<double>(const double2& q, int e) { return e == 0 ? q.x : q.y; }

__device__ __forceinline__ float4 vec_zero(float4*) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ double2 vec_zero(double2*) { return make_double2(0.0, 0.0); }

// The lane's vectors of one block of rows for a step: all of them under ONE test of the row where the step is whole (the
// loads go out together), each under its own test in the tail of a short row.  A lane without the row loads nothing.
template <typename Q, bool WHOLE>
__device__ __forceinline__ void gram_load(const Q* row, bool ok, uint64_t v0, uint64_t nvec, Q (&x)[GR_VECS]) {
#pragma unroll
    for (int v = 0; v < GR_VECS; ++v) x[v] = vec_zero((Q*)nullptr);
    if constexpr (WHOLE) {
        if (ok) {
#pragma unroll
            for (int v = 0; v < GR_VECS; ++v) x[v] = row[v0 + v];
        }
    } else {
#pragma unroll
        for (int v = 0; v < GR_VECS; ++v)
            if (ok && v0 + v < nvec) x[v] = row[v0 + v];
    }
}

// One step of a wave: the loads of both operands first, then two MFMAs per real and pair of blocks.  SAME: a diagonal
// tile of the self-Gram -- the rows of A are the B operand as they are, nothing is loaded or copied for it.
template <typename T, int BA, int BB, bool SAME, bool WHOLE>
__device__ __forceinline__ void gram_step(const typename Vec16<T>::type* const (&ra)[BA], const typename Vec16<T>::type* const (&rb)[BB],
                                          const bool (&oka)[BA], const bool (&okb)[BB], uint64_t v0, uint64_t nvec,
                                          typename Mfma<T>::acc_t (&acc)[BA][BB][2]) {
    using Q = typename Vec16<T>::type;
    constexpr int VE = 16 / (int)sizeof(T);             // reals of a vector
    constexpr int NF = GR_VECS * VE;                    // reals of a lane per step
    Q xa[BA][GR_VECS], xb[SAME ? 1 : BB][GR_VECS];
#pragma unroll
    for (int p = 0; p < BA; ++p) gram_load<Q, WHOLE>(ra[p], oka[p], v0, nvec, xa[p]);
    if constexpr (!SAME) {
#pragma unroll
        for (int p = 0; p < BB; ++p) gram_load<Q, WHOLE>(rb[p], okb[p], v0, nvec, xb[p]);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        T b[BB], jb[BB];
#pragma unroll
        for (int p = 0; p < BB; ++p) {
            const Q& x = SAME ? xa[p < BA ? p : 0][f / VE] : xb[SAME ? 0 : p][f / VE];
            b[p] = vec_real<T>(x, f % VE);
            // J b: (re, im) -> (im, -re)
            jb[p] = (f & 1) ? -vec_real<T>(x, f % VE - 1) : vec_real<T>(x, f % VE + 1);
        }
#pragma unroll
        for (int pa = 0; pa < BA; ++pa) {
            const T a = vec_real<T>(xa[pa][f / VE], f % VE);
#pragma unroll
            for (int pb = 0; pb < BB; ++pb) {
                acc[pa][pb][0] = Mfma<T>::run(a, b[pb], acc[pa][pb][0]);
                acc[pa][pb][1] = Mfma<T>::run(a, jb[pb], acc[pa][pb][1]);
            }
        }
    }
}

// BA x BB blocks of 16 x 16 of the tile are computed (rows beyond them do not exist)
template <typename T, int BA, int BB>
__global__ __launch_bounds__(256) void gram_kernel(const typename Vec16<T>::type* __restrict__ A,
                                                   const typename Vec16<T>::type* __restrict__ B, int M, int N, uint64_t nvec,
                                                   uint64_t units, int self, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    using acc_t = typename Mfma<T>::acc_t;
    constexpr bool F32 = sizeof(T) == 4;
    __shared__ double sh[GR_WAVES - 1][GR_ENTRIES];     // one of re / im at a time

    const unsigned ta = blockIdx.y, tb = blockIdx.z;
    if (self && ta > tb) return;                        // (the finish kernel mirrors it)
    const bool diag = self && ta == tb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;

    const Q* ra[BA];
    const Q* rb[BB];
    bool oka[BA], okb[BB];
#pragma unroll
    for (int p = 0; p < BA; ++p) {
        const int64_t row = (int64_t)ta * GR_TILE + p * 16 + i;
        oka[p] = row < M;
        ra[p] = A + (uint64_t)(oka[p] ? row : 0) * nvec;
    }
#pragma unroll
    for (int p = 0; p < BB; ++p) {
        const int64_t row = (int64_t)tb * GR_TILE + p * 16 + i;
        okb[p] = row < N;
        rb[p] = B + (uint64_t)(okb[p] ? row : 0) * nvec;
    }

    acc_t acc[BA][BB][2];
    double wide[BA][BB][2][4];                          // complex64 only
#pragma unroll
    for (int pa = 0; pa < BA; ++pa)
#pragma unroll
        for (int pb = 0; pb < BB; ++pb)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[pa][pb][c][r] = 0;
                    wide[pa][pb][c][r] = 0.0;
                }

    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
#pragma unroll 1
        for (int s = 0; s < GR_STEPS; ++s) {
            const uint64_t w0 = ((u * GR_STEPS + s) * GR_WAVES + wave) * GR_WAVE_VECS;
            if (w0 >= nvec) break;                      // (uniform over the wave: nothing of this step exists)
            const uint64_t v0 = w0 + (uint64_t)(q * GR_VECS);
            // uniform over the wave: the whole step exists (no guard per vector) or it is the tail of a short row
            const bool whole = w0 + GR_WAVE_VECS <= nvec;
            if (diag) {
                if constexpr (BA == BB) {
                    if (whole) gram_step<T, BA, BB, true, true>(ra, rb, oka, okb, v0, nvec, acc);
                    else gram_step<T, BA, BB, true, false>(ra, rb, oka, okb, v0, nvec, acc);
                }
            } else if (whole) {
                gram_step<T, BA, BB, false, true>(ra, rb, oka, okb, v0, nvec, acc);
            } else {
                gram_step<T, BA, BB, false, false>(ra, rb, oka, okb, v0, nvec, acc);
            }
        }
        if constexpr (F32) {                            // the chain ends here: GR_CHAIN real terms
#pragma unroll
            for (int pa = 0; pa < BA; ++pa)
#pragma unroll
                for (int pb = 0; pb < BB; ++pb)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            wide[pa][pb][c][r] += (double)acc[pa][pb][c][r];
                            acc[pa][pb][c][r] = 0;
                        }
        }
    }

    // the waves in the order 0..3, then the workgroup's partial sums of the tile
    double* part = ws + (((uint64_t)ta * gridDim.z + tb) * gridDim.x + blockIdx.x) * (uint64_t)(GR_ENTRIES * 2);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int pa = 0; pa < BA; ++pa)
#pragma unroll
            for (int pb = 0; pb < BB; ++pb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = (pa * 16 + Mfma<T>::row(q, r)) * GR_TILE + pb * 16 + i;
                    double val;
                    if constexpr (F32) val = wide[pa][pb][c][r];
                    else val = (double)acc[pa][pb][c][r];
                    if (wave > 0) sh[wave - 1][e] = val;
                    else wide[pa][pb][c][r] = val;
                }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int pa = 0; pa < BA; ++pa)
#pragma unroll
                for (int pb = 0; pb < BB; ++pb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int e = (pa * 16 + Mfma<T>::row(q, r)) * GR_TILE + pb * 16 + i;
                        double val = wide[pa][pb][c][r];
                        for (int w = 0; w < GR_WAVES - 1; ++w) val += sh[w][e];
                        part[e * 2 + c] = val;
                    }
        }
        __syncthreads();
    }
}

// out[i, j] = the sum of the nblk partial sums of its tile, in the order of the workgroups; the self-Gram's lower
// triangle as the conjugate of the upper one, its diagonal real
__global__ __launch_bounds__(256) void gram_finish_kernel(const double* __restrict__ ws, unsigned nblk, int M, int N,
                                                          unsigned tiles_b, int self, double* __restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (uint64_t)M * (uint64_t)N) return;
    const int64_t i = (int64_t)(idx / (uint64_t)N), j = (int64_t)(idx % (uint64_t)N);
    const bool mirror = self && i > j;
    const int64_t si = mirror ? j : i, sj = mirror ? i : j;
    const uint64_t pair = (uint64_t)(si / GR_TILE) * tiles_b + (uint64_t)(sj / GR_TILE);
    const double* p = ws + pair * nblk * (uint64_t)(GR_ENTRIES * 2) + (uint64_t)(((si % GR_TILE) * GR_TILE + sj % GR_TILE) * 2);
    double re = 0.0, im = 0.0;
    for (unsigned b = 0; b < nblk; ++b) {
        re += p[(uint64_t)b * (GR_ENTRIES * 2)];
        im += p[(uint64_t)b * (GR_ENTRIES * 2) + 1];
    }
    if (mirror) im = -im;
    if (self && i == j) im = 0.0;
    out[2 * idx] = re;
    out[2 * idx + 1] = im;
}

// BM blocks of 16 output rows are computed
template <typename T, int BM>
__global__ __launch_bounds__(256) void combine_kernel(const typename Vec16<T>::type* __restrict__ S,
                                                      const double2* __restrict__ C, typename Vec16<T>::type* __restrict__ Y,
                                                      int M, int N, uint64_t nvec, uint64_t units) {
    using Q = typename Vec16<T>::type;
    using acc_t = typename Mfma<T>::acc_t;
    constexpr int VE = 16 / (int)sizeof(T);
    __shared__ cx<T> tab[CB_CHUNK][CB_TILE];            // [input row of the chunk][output row of the tile]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, k = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * CB_TILE;
    const int nchunks = (N + CB_CHUNK - 1) / CB_CHUNK;

    auto stage = [&](int j0) {                          // the coefficients of input rows [j0, j0 + CB_CHUNK), rounded once
        for (int idx = threadIdx.x; idx < CB_CHUNK * CB_TILE; idx += 256) {
            const int jj = idx / CB_TILE, mm = idx % CB_TILE;
            double2 z = make_double2(0.0, 0.0);
            if (j0 + jj < N && m0 + mm < M) z = C[(uint64_t)(m0 + mm) * (uint64_t)N + (uint64_t)(j0 + jj)];
            tab[jj][mm] = mk<T>((T)z.x, (T)z.y);
        }
    };
    if (nchunks == 1) {
        stage(0);
        __syncthreads();
    }

    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint64_t w0 = (u * 4 + (uint64_t)wave) * CB_WAVE_VECS;
        const uint64_t v = w0 + (uint64_t)c;
        const bool okv = v < nvec;
        acc_t acc[BM][VE];
#pragma unroll
        for (int p = 0; p < BM; ++p)
#pragma unroll
            for (int e = 0; e < VE; ++e)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[p][e][r] = 0;

        for (int ch = 0; ch < nchunks; ++ch) {
            if (nchunks > 1) {
                __syncthreads();
                stage(ch * CB_CHUNK);
                __syncthreads();
            }
            const int j0 = ch * CB_CHUNK;
            const int rows = N - j0 < CB_CHUNK ? N - j0 : CB_CHUNK;
            const int ngroups = (rows + 3) / 4;
            if (w0 < nvec) {                            // (uniform over the wave)
                for (int g0 = 0; g0 < ngroups; g0 += CB_AHEAD) {
                    Q x[CB_AHEAD];
#pragma unroll
                    for (int t = 0; t < CB_AHEAD; ++t) {
                        const int jj = (g0 + t) * 4 + k;
                        x[t] = vec_zero((Q*)nullptr);
                        if (okv && jj < rows) x[t] = S[(uint64_t)(j0 + jj) * nvec + v];
                    }
#pragma unroll
                    for (int t = 0; t < CB_AHEAD; ++t) {
                        if (g0 + t < ngroups) {
                            const int jj = (g0 + t) * 4 + k;
                            cx<T> cf[BM];
#pragma unroll
                            for (int p = 0; p < BM; ++p) cf[p] = tab[jj][p * 16 + c];
#pragma unroll
                            for (int e = 0; e < VE; ++e) {
                                const T s = vec_real<T>(x[t], e);
                                const T js = (e & 1) ? vec_real<T>(x[t], e - 1) : -vec_real<T>(x[t], e + 1);      // J' s
#pragma unroll
                                for (int p = 0; p < BM; ++p) {
                                    acc[p][e] = Mfma<T>::run(s, cf[p].x, acc[p][e]);
                                    acc[p][e] = Mfma<T>::run(js, cf[p].y, acc[p][e]);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (w0 < nvec) {
#pragma unroll
            for (int p = 0; p < BM; ++p) {
                const int64_t m = m0 + p * 16 + c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint64_t vo = w0 + (uint64_t)Mfma<T>::row(k, r);
                    if (m < M && vo < nvec) {
                        Q y;
                        if constexpr (VE == 4) y = make_float4(acc[p][0][r], acc[p][1][r], acc[p][2][r], acc[p][3][r]);
                        else y = make_double2(acc[p][0][r], acc[p][1][r]);
                        Y[(uint64_t)m * nvec + vo] = y;
                    }
                }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------
constexpr int64_t GR_MAX_ROWS = 65535ll * GR_TILE;      // tiles are a grid dimension
constexpr uint64_t GR_MAX_ENTRIES = 1ull << 32;         // of a Gram: the finish kernel's grid, a thread per entry

bool rows_ok(int64_t M, int64_t N, bool gram) {
    if (M < 1 || M > GR_MAX_ROWS || N < 1 || N > GR_MAX_ROWS) return false;
    return !gram || (uint64_t)M * (uint64_t)N <= GR_MAX_ENTRIES;
}

uint64_t row_vectors(int n, bool is_c128) { return is_c128 ? 1ull << n : 1ull << (n - 1); }

int check_shape(const char* what, int n, int64_t M, int64_t N, bool is_c128, bool gram) {
    const int nmin = is_c128 ? 0 : 1;
    if (n < nmin || n > 40) {
        set_error("%s: n=%d out of range [%d, 40]", what, n, nmin);
        return DQ_ERR_ARG;
    }
    if (!rows_ok(M, N, gram)) {
        set_error("%s: %lld x %lld rows outside [1, %lld]%s", what, (long long)M, (long long)N, (long long)GR_MAX_ROWS,
                  gram ? ", or more than 2^32 entries" : "");
        return DQ_ERR_ARG;
    }
    return DQ_OK;
}

struct GramGrid {
    unsigned tiles_a, tiles_b, nblk;
    uint64_t units;
};

GramGrid gram_grid(int n, int64_t M, int64_t N, bool is_c128) {
    GramGrid g;
    g.tiles_a = (unsigned)((M + GR_TILE - 1) / GR_TILE);
    g.tiles_b = (unsigned)((N + GR_TILE - 1) / GR_TILE);
    g.units = (row_vectors(n, is_c128) + GR_UNIT_VECS - 1) / GR_UNIT_VECS;
    const uint64_t pairs = (uint64_t)g.tiles_a * g.tiles_b;
    uint64_t nblk = pairs >= GR_BLOCKS ? 1 : GR_BLOCKS / pairs;
    if (nblk > g.units) nblk = g.units;
    g.nblk = (unsigned)nblk;
    return g;
}

int64_t gram_ws_bytes(int n, int64_t M, int64_t N, bool is_c128) {
    const GramGrid g = gram_grid(n, M, N, is_c128);
    return (int64_t)g.tiles_a * g.tiles_b * g.nblk * (int64_t)(GR_ENTRIES * 2 * sizeof(double));
}

template <typename T, int BA, int BB>
void gram_launch(const void* A, const void* B, int M, int N, uint64_t nvec, const GramGrid& g, int self, double* ws, hipStream_t s) {
    using Q = typename Vec16<T>::type;
    hipLaunchKernelGGL((gram_kernel<T, BA, BB>), dim3(g.nblk, g.tiles_a, g.tiles_b), dim3(256), 0, s, (const Q*)A, (const Q*)B, M, N,
                       nvec, g.units, self, ws);
}

template <typename T>
int gram_impl(const void* A, const void* B, int n, int64_t M, int64_t N, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = C128 ? "dq_gram_c128" : "dq_gram_c64";
    if (!A || !B || !out || !ws) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    if (misaligned(A) || misaligned(B) || misaligned(ws) || (reinterpret_cast<uintptr_t>(out) & 7)) {
        set_error("%s: a, b and ws must be 16-byte aligned, out 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (int rc = check_shape(what, n, M, N, C128, true)) return rc;
    const int64_t need = gram_ws_bytes(n, M, N, C128);
    if (ws_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (dq_gram_ws_bytes)", what, (long long)ws_bytes, (long long)need);
        return DQ_ERR_ARG;
    }
    const uint64_t row_bytes = row_vectors(n, C128) * 16;
    const uint64_t out_bytes = (uint64_t)M * (uint64_t)N * 16;
    const uintptr_t o = reinterpret_cast<uintptr_t>(out), w = reinterpret_cast<uintptr_t>(ws);
    auto hits = [](uintptr_t p, uint64_t pb, uintptr_t r, uint64_t rbytes) { return p < r + rbytes && r < p + pb; };
    const uintptr_t a = reinterpret_cast<uintptr_t>(A), b = reinterpret_cast<uintptr_t>(B);
    if (hits(o, out_bytes, a, (uint64_t)M * row_bytes) || hits(o, out_bytes, b, (uint64_t)N * row_bytes) ||
        hits(w, (uint64_t)need, a, (uint64_t)M * row_bytes) || hits(w, (uint64_t)need, b, (uint64_t)N * row_bytes) ||
        hits(o, out_bytes, w, (uint64_t)need)) {
        set_error("%s: out, ws and the states overlap", what);
        return DQ_ERR_ARG;
    }
    const GramGrid g = gram_grid(n, M, N, C128);
    const int self = (A == B && M == N) ? 1 : 0;
    const uint64_t nvec = row_vectors(n, C128);
    hipStream_t s = as_stream(stream);
    const bool a1 = M <= 16, b1 = N <= 16;
    if (a1 && b1) gram_launch<T, 1, 1>(A, B, (int)M, (int)N, nvec, g, self, (double*)ws, s);
    else if (a1) gram_launch<T, 1, 2>(A, B, (int)M, (int)N, nvec, g, self, (double*)ws, s);
    else if (b1) gram_launch<T, 2, 1>(A, B, (int)M, (int)N, nvec, g, self, (double*)ws, s);
    else gram_launch<T, 2, 2>(A, B, (int)M, (int)N, nvec, g, self, (double*)ws, s);
    if (int rc = check_launch(what)) return rc;
    const uint64_t entries = (uint64_t)M * (uint64_t)N;
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, (const double*)ws, g.nblk, (int)M,
                       (int)N, g.tiles_b, self, out);
    return check_launch(what);
}

template <typename T>
int combine_impl(const void* S, const double* C, void* Y, int n, int64_t M, int64_t N, dq_stream_t stream) {
    using Q = typename Vec16<T>::type;
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = C128 ? "dq_combine_c128" : "dq_combine_c64";
    if (!S || !C || !Y) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    if (misaligned(S) || misaligned(Y)) {
        set_error("%s: in and out must be 16-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (misaligned(C)) {
        set_error("%s: coef must be 16-byte aligned (complex128 entries)", what);
        return DQ_ERR_ARG;
    }
    if (int rc = check_shape(what, n, M, N, C128, false)) return rc;
    const uint64_t nvec = row_vectors(n, C128);
    const uint64_t row_bytes = nvec * 16;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(S), y0 = reinterpret_cast<uintptr_t>(Y), c0 = reinterpret_cast<uintptr_t>(C);
    const uint64_t sb = (uint64_t)N * row_bytes, yb = (uint64_t)M * row_bytes, cb = (uint64_t)M * (uint64_t)N * 16;
    if (y0 < s0 + sb && s0 < y0 + yb) {
        set_error("%s: in and out overlap (out of place only)", what);
        return DQ_ERR_ARG;
    }
    if (y0 < c0 + cb && c0 < y0 + yb) {
        set_error("%s: coef and out overlap", what);
        return DQ_ERR_ARG;
    }
    const uint64_t units = (nvec + CB_UNIT_VECS - 1) / CB_UNIT_VECS;
    const unsigned tiles = (unsigned)((M + CB_TILE - 1) / CB_TILE);
    const dim3 grid((unsigned)(units < CB_BLOCKS ? units : CB_BLOCKS), tiles);
    hipStream_t s = as_stream(stream);
    if (M <= 16)
        hipLaunchKernelGGL((combine_kernel<T, 1>), grid, dim3(256), 0, s, (const Q*)S, (const double2*)C, (Q*)Y, (int)M, (int)N, nvec, units);
    else
        hipLaunchKernelGGL((combine_kernel<T, 2>), grid, dim3(256), 0, s, (const Q*)S, (const double2*)C, (Q*)Y, (int)M, (int)N, nvec, units);
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int64_t dq_gram_ws_bytes(int n, int64_t rows_a, int64_t rows_b, int is_c128) {
    if (n < (is_c128 ? 0 : 1) || n > 40 || !dq::rows_ok(rows_a, rows_b, true)) return -1;
    return dq::gram_ws_bytes(n, rows_a, rows_b, is_c128 != 0);
}

extern "C" int dq_gram_geometry(int is_c128, int* tile_rows, int* chain, int* lane_cols, int* wave_cols, int* unit_cols,
                                int* max_blocks) {
    if (!tile_rows || !chain || !lane_cols || !wave_cols || !unit_cols || !max_blocks) {
        dq::set_error("dq_gram_geometry: null pointer");
        return DQ_ERR_ARG;
    }
    const int per_vec = is_c128 ? 1 : 2;                // amplitudes of a 16-byte vector
    *tile_rows = dq::GR_TILE;
    *chain = is_c128 ? 0 : dq::GR_CHAIN;
    *lane_cols = dq::GR_VECS * per_vec;
    *wave_cols = dq::GR_WAVE_VECS * per_vec;
    *unit_cols = dq::GR_UNIT_VECS * per_vec;
    *max_blocks = (int)dq::GR_BLOCKS;
    return DQ_OK;
}

extern "C" int dq_gram_c64(const void* a, const void* b, int n, int64_t rows_a, int64_t rows_b, double* out, void* ws, int64_t ws_bytes,
                           dq_stream_t stream) {
    return dq::gram_impl<float>(a, b, n, rows_a, rows_b, out, ws, ws_bytes, stream);
}
extern "C" int dq_gram_c128(const void* a, const void* b, int n, int64_t rows_a, int64_t rows_b, double* out, void* ws, int64_t ws_bytes,
                            dq_stream_t stream) {
    return dq::gram_impl<double>(a, b, n, rows_a, rows_b, out, ws, ws_bytes, stream);
}
extern "C" int dq_combine_c64(const void* in, const double* coef, void* out, int n, int64_t rows_out, int64_t rows_in,
                              dq_stream_t stream) {
    return dq::combine_impl<float>(in, coef, out, n, rows_out, rows_in, stream);
}
extern "C" int dq_combine_c128(const void* in, const double* coef, void* out, int n, int64_t rows_out, int64_t rows_in,
                               dq_stream_t stream) {
    return dq::combine_impl<double>(in, coef, out, n, rows_out, rows_in, stream);
}
