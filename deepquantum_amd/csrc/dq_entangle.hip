// One-body reductions for entanglement measures: the single-wire cross reduction T(phi, psi) for every wire at once,
// and its reverse-mode partner, the sum of one-wire operators W(psi; M).  Replaces the n permute-copies and 3n inner
// products of qmath.meyer_wallach_measure (qmath.py:874-890) and the 4^n density matrix of
// meyer_wallach_measure_brennen (qmath.py:941-965) with a fixed number of reads of the state.
//
// Geometry.  A pass owns tiles of 2^m amplitudes (m = 12; 11 for a complex128 cross reduction, whose two staged
// states would not fit 64 KiB of LDS otherwise): the low s index bits, contiguous, plus g = m - s gathered bits at
// the consecutive positions lo .. lo + g - 1.  Pass 0 is the contiguous tile (s = m, g = 0) and settles every wire
// whose bit lies inside it, plus the diagonal (p0, p1) of every other wire from per-tile sums.  Each further pass
// gathers up to g = m - s high bits (s >= 4 for complex64, s >= 3 for complex128: a 128-B line of contiguous
// amplitudes) and settles their coherences.  Reads: 1 + ceil((n - 12) / 8) for complex64, 1 + ceil((n - 12) / 9) for
// complex128 (1 + ceil((n - 11) / 8) for its cross reduction).
//
// Inside a tile, thread t of 256 holds the amplitudes at tile index t + 256 k (k < 16) in registers: pairs along tile
// bits 8..11 are register pairs, pairs along tile bits 0..7 take the partner from the LDS copy of the tile.
// Accumulation is in double precision (the at most 8 pair products of one bit within one tile are summed in the
// state's precision first); every workgroup writes a fixed-order row of partial sums and a second kernel
// adds the rows in a fixed order -- no atomics, so results are bitwise reproducible.
#include "dq_common.hpp"

namespace dq {

namespace {

constexpr int ENT_THREADS = 256;
constexpr int ENT_MAXM = 12;
constexpr int ENT_ROW = ENT_MAXM * 8;   // doubles per workgroup row: per tile bit T00, T01, T10, T11 (re, im)
constexpr int ENT_MAXN = 40;
constexpr int ENT_MAXPASS = 8;
constexpr int ENT_WAVES = ENT_THREADS / 64;

struct EntPass {
    int m;       // tile bits
    int s;       // contiguous low bits of the tile
    int lo;      // global position of the first gathered bit (== s when g == 0)
    int jlo;     // first tile bit whose pairs this pass reduces / applies
    int first;   // pass 0: diagonals and per-tile sums (reduction), diagonal term (apply)
    int n;
    uint32_t jmask;  // tile bits jlo .. m - 1
    uint64_t ntiles;
};

__device__ __forceinline__ uint64_t tile_base(const EntPass& g, uint64_t o) {
    const int g_bits = g.m - g.s;
    const int mid = g.lo - g.s;           // outer bits below the gathered range
    return ((o & ((1ull << mid) - 1ull)) << g.s) | ((o >> mid) << (g.lo + g_bits));
}

__device__ __forceinline__ uint64_t tile_index(const EntPass& g, uint64_t base, int l) {
    return base | (uint64_t)(l & ((1 << g.s) - 1)) | ((uint64_t)(l >> g.s) << g.lo);
}

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed-order sum over the workgroup; every thread gets the result
__device__ __forceinline__ double bsum(double v, double* red) {
    v = wsum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// conj(a) * b accumulated in R (double, or the state's precision for the few terms of one tile)
template <typename V, typename R> __device__ __forceinline__ void cjmac(const V& a, const V& b, R& re, R& im) {
    const R ar = a.x, ai = a.y, br = b.x, bi = b.y;
    re = fma(ar, br, fma(ai, bi, re));
    im = fma(ar, bi, fma(-ai, br, im));
}

// ---- the cross reduction, one pass ---------------------------------------------------------------------------------
// part: [batch, gridDim.x, ENT_MAXM, 8] doubles, row of tile bit j = (T00, T01, T10, T11) over this workgroup's tiles,
// only the bits this pass reduces are written (T00 / T11 in pass 0 only).  tsum (pass 0, n > m): [batch, ntiles, 2],
// sum over the tile of conj(bra) ket.  A tile smaller than the LDS tile (n < m) is padded with zeros.
template <typename T, bool CROSS>
__global__ __launch_bounds__(ENT_THREADS) void rdm1_pass_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                EntPass g, double* __restrict__ part,
                                                                double* __restrict__ tsum) {
    constexpr int TB = (sizeof(T) == 8 && CROSS) ? 11 : 12;
    constexpr int KS = 1 << (TB - 8);        // slots per thread: tile index t + 256 k
    __shared__ cx<T> lds[(CROSS ? 2 : 1) << TB];
    __shared__ double tred[2][4];
    cx<T>* sk = lds;
    cx<T>* sb = CROSS ? lds + (1 << TB) : lds;
    const int t = threadIdx.x;
    const int tile = 1 << g.m;
    const uint64_t dim = 1ull << g.n;
    const cx<T>* kb = ket + blockIdx.y * dim;
    const cx<T>* bb = bra + blockIdx.y * dim;

    double c01r[TB], c01i[TB], c10r[TB], c10i[TB];
    double d0r[TB - 8], d0i[TB - 8], d1r[TB - 8], d1i[TB - 8];   // pass 0: diagonal along the register bits
    double dtr = 0, dti = 0;                  // pass 0: this thread's total (its thread bits settle the rest)
#pragma unroll
    for (int j = 0; j < TB; ++j) c01r[j] = c01i[j] = c10r[j] = c10i[j] = 0;
#pragma unroll
    for (int r = 0; r < TB - 8; ++r) d0r[r] = d0i[r] = d1r[r] = d1i[r] = 0;

    for (uint64_t o = blockIdx.x; o < g.ntiles; o += gridDim.x) {
        const uint64_t base = tile_base(g, o);
        cx<T> rk[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int l = t + k * ENT_THREADS;
            const bool in = l < tile;        // (n < m: the tile is padded with zeros; the read stays inside it)
            const uint64_t gi = tile_index(g, base, in ? l : 0);
            rk[k] = kb[gi];
            cx<T> rb = CROSS ? bb[gi] : rk[k];
            if (!in) rk[k] = rb = mk<T>(0, 0);
            sk[l] = rk[k];
            if (CROSS) sb[l] = rb;
        }
        __syncthreads();
        if (g.first) {
            double tr = 0, ti = 0;
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                double pr = 0, pi = 0;
                cjmac(CROSS ? sb[t + k * ENT_THREADS] : rk[k], rk[k], pr, pi);
                tr += pr;
                ti += pi;
#pragma unroll
                for (int r = 0; r < TB - 8; ++r) {
                    if ((k >> r) & 1) {
                        d1r[r] += pr;
                        d1i[r] += pi;
                    } else {
                        d0r[r] += pr;
                        d0i[r] += pi;
                    }
                }
            }
            dtr += tr;
            dti += ti;
            if (g.ntiles > 1) {
                tr = wsum(tr);
                ti = wsum(ti);
                if ((t & 63) == 0) {
                    tred[0][t >> 6] = tr;
                    tred[1][t >> 6] = ti;
                }
            }
        }
        // pairs (i, i') along tile bit j: T01 += conj(bra_i) ket_i', T10 += conj(bra_i') ket_i
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            if (!((g.jmask >> j) & 1)) continue;
            // this tile's pairs summed in the state's precision (at most 8 terms), then added in double
            T s01r = 0, s01i = 0, s10r = 0, s10i = 0;
            if (j >= 8) {                     // register pairs
                const int rb = (j - 8) & 3;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    if ((k >> rb) & 1) continue;
                    const int k1 = k | (1 << rb);
                    cjmac(CROSS ? sb[t + k * ENT_THREADS] : rk[k], rk[k1], s01r, s01i);
                    if (CROSS) cjmac(sb[t + k1 * ENT_THREADS], rk[k], s10r, s10i);
                }
            } else {
                // partner from LDS; the thread whose bit j is 0 takes the lower half of the slots, its partner the
                // upper half: every pair once, no idle lanes
                const bool hi = (t >> j) & 1;
#pragma unroll
                for (int k = 0; k < KS / 2; ++k) {
                    const int ko = hi ? k + KS / 2 : k;
                    const cx<T> own = hi ? rk[k + KS / 2] : rk[k];
                    const int lp = (t ^ (1 << j)) + ko * ENT_THREADS;
                    const cx<T> pk = sk[lp];
                    if (!CROSS) {
                        if (hi) cjmac(pk, own, s01r, s01i);
                        else cjmac(own, pk, s01r, s01i);
                    } else {
                        const cx<T> ob = sb[t + ko * ENT_THREADS];
                        const cx<T> pb = sb[lp];
                        cjmac(hi ? pb : ob, hi ? own : pk, s01r, s01i);
                        cjmac(hi ? ob : pb, hi ? pk : own, s10r, s10i);
                    }
                }
            }
            c01r[j] += s01r;
            c01i[j] += s01i;
            if (CROSS) {
                c10r[j] += s10r;
                c10i[j] += s10i;
            }
        }
        __syncthreads();
        if (g.first && g.ntiles > 1 && t == 0) {
            double* d = tsum + (blockIdx.y * g.ntiles + o) * 2;
            d[0] = (tred[0][0] + tred[0][1]) + (tred[0][2] + tred[0][3]);
            d[1] = (tred[1][0] + tred[1][1]) + (tred[1][2] + tred[1][3]);
        }
    }

    // per bit and component: wave sums, then the four waves in a fixed order -- one row per workgroup
    __shared__ double wred[ENT_WAVES][ENT_ROW];
    const int w = t >> 6;
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        if (!((g.jmask >> j) & 1)) continue;
        double v[8];
        v[2] = c01r[j];
        v[3] = c01i[j];
        v[4] = CROSS ? c10r[j] : 0;
        v[5] = CROSS ? c10i[j] : 0;
        v[0] = v[1] = v[6] = v[7] = 0;
        if (g.first) {
            if (j >= 8) {
                v[0] = d0r[(j - 8) % (TB - 8)];
                v[1] = d0i[(j - 8) % (TB - 8)];
                v[6] = d1r[(j - 8) % (TB - 8)];
                v[7] = d1i[(j - 8) % (TB - 8)];
            } else {
                const bool hi = (t >> j) & 1;
                v[0] = hi ? 0 : dtr;
                v[1] = hi ? 0 : dti;
                v[6] = hi ? dtr : 0;
                v[7] = hi ? dti : 0;
            }
        }
        double r[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool need = (g.first || (c >= 2 && c < 6)) && (CROSS || c < 4 || c > 5);
            r[c] = need ? wsum(v[c]) : 0;
        }
        if (!CROSS) {                        // T10 = conj(T01) when bra == ket
            r[4] = r[2];
            r[5] = -r[3];
        }
        if ((t & 63) == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c) wred[w][j * 8 + c] = r[c];
        }
    }
    __syncthreads();
    if (t < ENT_ROW && ((g.jmask >> (t >> 3)) & 1)) {
        double* row = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ENT_ROW;
        row[t] = (wred[0][t] + wred[1][t]) + (wred[2][t] + wred[3][t]);
    }
}

// Where wire bit p was settled: the row offset of its pass in `part`, the pass's workgroups per sample and tile bit.
struct EntFinish {
    int n;
    int m0;
    uint64_t ntiles0;
    int64_t off[ENT_MAXN];
    int nwg[ENT_MAXN];
    int j[ENT_MAXN];
};

// out: [batch, n, 2, 2] complex128, indexed by WIRE (wire k = bit n - 1 - k).  Grid (n, batch).
__global__ __launch_bounds__(ENT_THREADS) void rdm1_finish_kernel(const double* __restrict__ part,
                                                                  const double* __restrict__ tsum, EntFinish f,
                                                                  double* __restrict__ out) {
    __shared__ double red[4];
    const int p = blockIdx.x, t = threadIdx.x;
    const uint64_t b = blockIdx.y;
    const int nwg = f.nwg[p], j = f.j[p];
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double* rows = part + f.off[p] + (size_t)b * nwg * ENT_ROW + j * 8;
    for (int w = t; w < nwg; w += ENT_THREADS) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] += rows[(size_t)w * ENT_ROW + c];
    }
    if (p >= f.m0) {                         // diagonal of a wire outside the tile: sums of whole tiles
        const int q = p - f.m0;
        const double* ts = tsum + b * f.ntiles0 * 2;
        for (uint64_t o = t; o < f.ntiles0; o += ENT_THREADS) {
            const int a = (o >> q) & 1;
            v[a ? 6 : 0] += ts[o * 2];
            v[a ? 7 : 1] += ts[o * 2 + 1];
        }
    }
    double* dst = out + ((b * f.n + (f.n - 1 - p)) * 4) * 2;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double s = bsum(v[c], red);
        if (t == 0) dst[c] = s;
    }
}

// ---- the sum of one-wire operators, one pass --------------------------------------------------------------------------
// out[i] = sum_p sum_c M_p[bit_p(i), c] psi[i with bit p = c], M_p the 2x2 of wire n - 1 - p ([batch, n, 2, 2]
// complex128).  Pass 0 writes out with the diagonal of every wire and the pairs along its tile bits; a gathered pass
// reads out back and adds the pairs along its gathered bits.
template <typename T>
__global__ __launch_bounds__(ENT_THREADS) void wire_sum_pass_kernel(const cx<T>* __restrict__ psi, cx<T>* __restrict__ out,
                                                                    const double* __restrict__ mats, EntPass g) {
    constexpr int KS = 1 << (ENT_MAXM - 8);
    __shared__ cx<T> sk[1 << ENT_MAXM];
    __shared__ cx<T> sm[ENT_MAXM][4];        // the operator of tile bit j
    __shared__ cx<T> sdiag[ENT_MAXN][2];     // pass 0: diagonal of every wire bit
    const int t = threadIdx.x;
    const int tile = 1 << g.m;
    const uint64_t dim = 1ull << g.n;
    const cx<T>* src = psi + blockIdx.y * dim;
    cx<T>* dst = out + blockIdx.y * dim;
    const double* mb = mats + (size_t)blockIdx.y * g.n * 8;
    if (t < g.m * 4) {
        const int j = t >> 2, e = t & 3;
        const int p = j < g.s ? j : g.lo + (j - g.s);
        const double* q = mb + ((g.n - 1 - p) * 4 + e) * 2;
        sm[j][e] = mk<T>((T)q[0], (T)q[1]);
    }
    if (g.first && t < g.n * 2) {
        const int p = t >> 1, a = t & 1;
        const double* q = mb + ((g.n - 1 - p) * 4 + a * 3) * 2;
        sdiag[p][a] = mk<T>((T)q[0], (T)q[1]);
    }
    __syncthreads();

    for (uint64_t o = blockIdx.x; o < g.ntiles; o += gridDim.x) {
        const uint64_t base = tile_base(g, o);
        cx<T> rk[KS], acc[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int l = t + k * ENT_THREADS;
            const bool in = l < tile;
            rk[k] = src[tile_index(g, base, in ? l : 0)];
            if (!in) rk[k] = mk<T>(0, 0);
            sk[l] = rk[k];
        }
        if (g.first) {
            cx<T> dconst = mk<T>(0, 0);
            for (int p = g.m; p < g.n; ++p) dconst = cadd(dconst, sdiag[p][(base >> p) & 1]);
            cx<T> dlow = dconst;             // thread bits 0..7
            for (int j = 0; j < 8 && j < g.m; ++j) dlow = cadd(dlow, sm[j][((t >> j) & 1) * 3]);
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                cx<T> d = dlow;
#pragma unroll
                for (int j = 8; j < ENT_MAXM; ++j)
                    if (j < g.m) d = cadd(d, sm[j][((k >> (j - 8)) & 1) * 3]);
                acc[k] = cmul(d, rk[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const int l = t + k * ENT_THREADS;
                acc[k] = dst[tile_index(g, base, l < tile ? l : 0)];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < ENT_MAXM; ++j) {
            if (!((g.jmask >> j) & 1)) continue;
            if (j >= 8) {
                const int rb = (j - 8) & 3;
                const cx<T> m01 = sm[j][1], m10 = sm[j][2];
#pragma unroll
                for (int k = 0; k < KS; ++k) acc[k] = cfma(((k >> rb) & 1) ? m10 : m01, rk[k ^ (1 << rb)], acc[k]);
            } else {
                const cx<T> mo = sm[j][((t >> j) & 1) ? 2 : 1];
                const int tp = t ^ (1 << j);
#pragma unroll
                for (int k = 0; k < KS; ++k) acc[k] = cfma(mo, sk[tp + k * ENT_THREADS], acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int l = t + k * ENT_THREADS;
            if (l < tile) dst[tile_index(g, base, l)] = acc[k];
        }
        __syncthreads();
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
int ent_tile_bits(bool c128, bool cross) { return (c128 && cross) ? 11 : 12; }

// The passes for n qubits: pass 0 the contiguous tile, then the high bits in groups of g (a gathered pass keeps the
// contiguous s = m - g >= s_min low bits so every row it reads is at least one 128-B line).
int ent_plan(int n, bool c128, bool cross, EntPass* passes) {
    const int M = ent_tile_bits(c128, cross);
    const int m0 = n < M ? n : M;
    const int gmax = M - (c128 ? 3 : 4);
    int np = 0;
    passes[np++] = EntPass{m0, m0, m0, 0, 1, n, (1u << m0) - 1u, 1ull << (n - m0)};
    for (int lo = m0; lo < n; lo += gmax) {
        const int gb = (n - lo) < gmax ? (n - lo) : gmax;
        passes[np++] = EntPass{M, M - gb, lo, M - gb, 0, n, ((1u << M) - 1u) & ~((1u << (M - gb)) - 1u), 1ull << (n - M)};
    }
    return np;
}

int ent_nwg(const EntPass& p, int64_t batch) {
    uint64_t want = (2048 + (uint64_t)batch - 1) / (uint64_t)batch;
    if (want < 1) want = 1;
    return (int)(p.ntiles < want ? p.ntiles : want);
}

int64_t ent_ws_doubles(int n, int64_t batch, bool c128, bool cross, int64_t* tsum_off) {
    EntPass ps[ENT_MAXPASS];
    const int np = ent_plan(n, c128, cross, ps);
    int64_t total = 0;
    for (int i = 0; i < np; ++i) total += batch * (int64_t)ent_nwg(ps[i], batch) * ENT_ROW;
    if (tsum_off) *tsum_off = total;
    if (ps[0].ntiles > 1) total += batch * (int64_t)ps[0].ntiles * 2;
    return total;
}

bool ent_args_ok(const char* what, const void* a, const void* b, const void* c, int n, int64_t batch) {
    if (!a || !b || !c || n < 1 || n > ENT_MAXN || batch < 1 || batch > 65535) {
        set_error("%s: bad argument (n=%d batch=%lld; 1 <= n <= %d, 1 <= batch <= 65535, no null pointers)", what, n,
                  (long long)batch, ENT_MAXN);
        return false;
    }
    return true;
}

template <typename T>
int rdm1_cross_impl(const void* bra, const void* ket, int n, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                    dq_stream_t stream) {
    if (!ent_args_ok("dq_rdm1_cross", bra, ket, out, n, batch)) return DQ_ERR_ARG;
    const bool c128 = sizeof(T) == 8, cross = bra != ket;
    int64_t tsum_off = 0;
    const int64_t need = ent_ws_doubles(n, batch, c128, cross, &tsum_off) * (int64_t)sizeof(double);
    if (!ws || ws_bytes < need) {
        set_error("dq_rdm1_cross: workspace of %lld bytes, %lld needed (dq_rdm1_ws_bytes)", (long long)ws_bytes,
                  (long long)need);
        return DQ_ERR_ARG;
    }
    EntPass ps[ENT_MAXPASS];
    const int np = ent_plan(n, c128, cross, ps);
    double* part = static_cast<double*>(ws);
    double* tsum = part + tsum_off;
    EntFinish f{};
    f.n = n;
    f.m0 = ps[0].m;
    f.ntiles0 = ps[0].ntiles;
    hipStream_t s = as_stream(stream);
    int64_t off = 0;
    for (int i = 0; i < np; ++i) {
        const int nwg = ent_nwg(ps[i], batch);
        if (cross)
            hipLaunchKernelGGL((rdm1_pass_kernel<T, true>), dim3((unsigned)nwg, (unsigned)batch), dim3(ENT_THREADS), 0, s,
                               static_cast<const cx<T>*>(bra), static_cast<const cx<T>*>(ket), ps[i], part + off, tsum);
        else
            hipLaunchKernelGGL((rdm1_pass_kernel<T, false>), dim3((unsigned)nwg, (unsigned)batch), dim3(ENT_THREADS), 0, s,
                               static_cast<const cx<T>*>(bra), static_cast<const cx<T>*>(ket), ps[i], part + off, tsum);
        for (int j = ps[i].jlo; j < ps[i].m; ++j) {
            const int p = j < ps[i].s ? j : ps[i].lo + (j - ps[i].s);
            f.off[p] = off;
            f.nwg[p] = nwg;
            f.j[p] = j;
        }
        off += batch * (int64_t)nwg * ENT_ROW;
    }
    hipLaunchKernelGGL(rdm1_finish_kernel, dim3((unsigned)n, (unsigned)batch), dim3(ENT_THREADS), 0, s, part, tsum, f, out);
    return check_launch("dq_rdm1_cross");
}

template <typename T>
int wire_sum_impl(const void* psi, void* out, const double* mats, int n, int64_t batch, dq_stream_t stream) {
    if (!ent_args_ok("dq_apply_wire_sum", psi, out, mats, n, batch)) return DQ_ERR_ARG;
    const uintptr_t bytes = (uintptr_t)batch * (sizeof(cx<T>) << n);
    const uintptr_t a = (uintptr_t)psi, b = (uintptr_t)out;
    if (a < b + bytes && b < a + bytes) {
        set_error("dq_apply_wire_sum: out must not alias psi");
        return DQ_ERR_ARG;
    }
    EntPass ps[ENT_MAXPASS];
    const int np = ent_plan(n, sizeof(T) == 8, false, ps);
    hipStream_t s = as_stream(stream);
    for (int i = 0; i < np; ++i) {
        const int nwg = ent_nwg(ps[i], batch);
        hipLaunchKernelGGL(wire_sum_pass_kernel<T>, dim3((unsigned)nwg, (unsigned)batch), dim3(ENT_THREADS), 0, s,
                           static_cast<const cx<T>*>(psi), static_cast<cx<T>*>(out), mats, ps[i]);
    }
    return check_launch("dq_apply_wire_sum");
}

}  // namespace
}  // namespace dq

extern "C" int64_t dq_rdm1_ws_bytes(int n, int64_t batch, int is_c128, int cross) {
    if (n < 1 || n > dq::ENT_MAXN || batch < 1) return -1;
    return dq::ent_ws_doubles(n, batch, is_c128 != 0, cross != 0, nullptr) * (int64_t)sizeof(double);
}

extern "C" int dq_rdm1_cross_c64(const void* bra, const void* ket, int n, int64_t batch, double* out, void* ws,
                                 int64_t ws_bytes, dq_stream_t stream) {
    return dq::rdm1_cross_impl<float>(bra, ket, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_rdm1_cross_c128(const void* bra, const void* ket, int n, int64_t batch, double* out, void* ws,
                                  int64_t ws_bytes, dq_stream_t stream) {
    return dq::rdm1_cross_impl<double>(bra, ket, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_apply_wire_sum_c64(const void* psi, void* out, const double* mats, int n, int64_t batch,
                                     dq_stream_t stream) {
    return dq::wire_sum_impl<float>(psi, out, mats, n, batch, stream);
}
extern "C" int dq_apply_wire_sum_c128(const void* psi, void* out, const double* mats, int n, int64_t batch,
                                      dq_stream_t stream) {
    return dq::wire_sum_impl<double>(psi, out, mats, n, batch, stream);
}
