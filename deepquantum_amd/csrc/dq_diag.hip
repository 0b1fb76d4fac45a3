// Diagonal operators on any number of wires: one multiplication per amplitude, one read and one write of the state.
//
//     sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j)            (bits[0] = the table index's most significant bit)
//     dq_apply_diag : out[b, i] = diag[b, sub(i)] * in[b, i]
//     dq_apply_cost : out[b, i] = exp(-i t[b] cost[sub(i)]) * in[b, i]        (DQ_COST_PHASE)
//                     out[b, i] = s[b] cost[sub(i)] * in[b, i]                (DQ_COST_SCALE)
//     dq_cost_cross : out[b] = sum_i cost[sub(i)] conj(bra[b, i]) ket[b, i]
// on the amplitudes whose control bits are all 1; the others pass through (diag, PHASE), are left out (cross) or come
// out as 0 (SCALE: the cotangent of a sum that leaves them out).
//
// Geometry.  That of dq_stream.hpp with a vector as the item: a chunk is a unit of 1024 vectors, 16 KiB.
//
// Gather.  dq_stream.hpp's: sub() in runs of consecutive positions split at the chunk size, the low runs evaluated once
// per lane before the loop (ST_UNROLL * 2 table offsets per lane at most), the high runs once per chunk in scalar
// arithmetic.  A chunk whose high control bits are not all set is copied (or skipped, in place) without a table
// access.  With bits = n-1 .. 0 and no controls sub(i) = i: the table is read with vector loads beside the state and
// nothing is gathered (the IDENT instantiations).
//
// Phase.  The angle is double(t) * double(cost) for both precisions, turned into a fraction of a turn in double
// (times 1 / 2 pi, minus the nearest integer); only that fraction, in [-1/2, 1/2], goes to sincospi in the state's
// real precision.  The kernel builds no table of phases; the host may (backend.apply_cost runs this kernel on a vector
// of ones over the table bits and hands the result to dq_apply_diag where that measured faster).  DESIGN.md section 4.8
// has the instruction count against the bytes.
//
// Reduction.  Lanes accumulate in double over their chunks; the rest is dq_stream.hpp's fixed-order scheme.
#include "dq_stream.hpp"

namespace dq {

namespace {

enum { MODE_DIAG = 0, MODE_PHASE = 1, MODE_SCALE = 2 };

__device__ __forceinline__ void sincos_turns(float halfturns, float* s, float* c) { sincospif(halfturns, s, c); }
__device__ __forceinline__ void sincos_turns(double halfturns, double* s, double* c) { sincospi(halfturns, s, c); }

// exp(-i t c): the angle and its reduction to a fraction of a turn in double, sine and cosine in T
template <typename T> __device__ __forceinline__ cx<T> phase_of(double t, double c) {
    double r = (t * c) * 0.15915494309189533577;        // turns
    r -= rint(r);                                       // [-1/2, 1/2]
    T s, co;
    sincos_turns((T)(2.0 * r), &s, &co);
    return mk<T>(co, -s);
}

// The factor of one amplitude from its table entry.
template <typename T, int MODE> struct Factor;
template <typename T> struct Factor<T, MODE_DIAG> {
    using entry = cx<T>;
    static __device__ __forceinline__ cx<T> of(entry d, double, double) { return d; }
};
template <typename T> struct Factor<T, MODE_PHASE> {
    using entry = T;
    static __device__ __forceinline__ cx<T> of(entry c, double t, double) { return phase_of<T>(t, (double)c); }
};
template <typename T> struct Factor<T, MODE_SCALE> {
    using entry = T;
    static __device__ __forceinline__ cx<T> of(entry c, double sr, double si) {
        return mk<T>((T)(sr * (double)c), (T)(si * (double)c));
    }
};

// The VEC table entries beside vector v of the state (sub(i) = i), in one load.
template <typename E, int VEC> __device__ __forceinline__ void load_beside(const E* tab, uint64_t v, E (&d)[VEC]) {
    struct alignas(VEC * sizeof(E)) Row { E e[VEC]; };
    const Row r = reinterpret_cast<const Row*>(tab)[v];
#pragma unroll
    for (int e = 0; e < VEC; ++e) d[e] = r.e[e];
}

// in and out may be the same buffer: no __restrict__ on them
template <typename T, int MODE, bool IDENT>
__global__ __launch_bounds__(ST_THREADS) void diag_apply_kernel(const cx<T>* in, cx<T>* out, const void* __restrict__ table,
                                                                int64_t table_bstride, const double* __restrict__ par, Gather g,
                                                                int n, uint64_t nchunks) {
    using Q = typename Vec16<T>::type;
    using F = Factor<T, MODE>;
    using E = typename F::entry;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;            // amplitudes of a chunk
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    const E* tab = static_cast<const E*>(table) + b * (uint64_t)table_bstride;
    double p0 = 0.0, p1 = 0.0;
    if (MODE == MODE_PHASE) p0 = par[b];
    if (MODE == MODE_SCALE) { p0 = par[2 * b]; p1 = par[2 * b + 1]; }
    LaneLow<VEC> ll;
    if (!IDENT) lane_low<VEC>(g, SBITS, ll);
    const uint64_t ch = g.cmask >> SBITS;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        Q q[ST_UNROLL];
        E d[ST_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) q[u] = src[v];
        }
        if (!IDENT && (chunk & ch) != ch) {             // a high control bit is 0: the whole chunk passes through (is zero)
            if (MODE == MODE_SCALE || src != dst) {
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u) {
                    const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
                    if (v < nvec) dst[v] = MODE == MODE_SCALE ? Q{} : q[u];
                }
            }
            continue;
        }
        const uint64_t high = IDENT ? 0 : chunk_high(g, SBITS, chunk);
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                if (IDENT) {
                    load_beside<E, VEC>(tab, v, d[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) d[u][e] = tab[high | ll.sub[u][e]];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                Q r = MODE == MODE_SCALE ? Q{} : q[u];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (IDENT || ((ll.ok >> (u * VEC + e)) & 1u)) vec_set(r, e, cmul(F::of(d[u][e], p0, p1), vec_get<T>(q[u], e)));
                }
                dst[v] = r;
            }
        }
    }
}

// ws[b, blockIdx.x] = this workgroup's part of sum_i cost[sub(i)] conj(bra_i) ket_i
template <typename T, bool SAME, bool IDENT>
__global__ __launch_bounds__(ST_THREADS) void cost_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                const T* __restrict__ cost, Gather g, int n, uint64_t nchunks,
                                                                double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    LaneLow<VEC> ll;
    if (!IDENT) lane_low<VEC>(g, SBITS, ll);
    const uint64_t ch = g.cmask >> SBITS;
    double re = 0.0, im = 0.0;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (!IDENT && (chunk & ch) != ch) continue;     // (uniform over the workgroup)
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        const uint64_t high = IDENT ? 0 : chunk_high(g, SBITS, chunk);
        Q qk[ST_UNROLL], qb[ST_UNROLL];
        T c[ST_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                qk[u] = pk[v];
                if (!SAME) qb[u] = pb[v];
                if (IDENT) {
                    load_beside<T, VEC>(cost, v, c[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) c[u][e] = cost[high | ll.sub[u][e]];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (IDENT || ((ll.ok >> (u * VEC + e)) & 1u)) {
                        const cx<T> k = vec_get<T>(qk[u], e);
                        const double kr = (double)k.x, ki = (double)k.y, w = (double)c[u][e];
                        if (SAME) {
                            re = fma(w, kr * kr + ki * ki, re);
                        } else {
                            const cx<T> a = vec_get<T>(qb[u], e);
                            const double ar = (double)a.x, ai = (double)a.y;
                            re = fma(w, ar * kr + ai * ki, re);
                            im = fma(w, ar * ki - ai * kr, im);
                        }
                    }
                }
            }
        }
    }
    write_partial(re, im, sh, ws);
}

template <typename T, int MODE>
int apply_impl(const char* what, const void* in, void* out, const void* table, int64_t table_bstride, const double* par, int n,
               const int* bits, int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), SAME_OR_DISJOINT)) return rc;
    if (!table || misaligned(table) || (MODE != MODE_DIAG && (!par || (reinterpret_cast<uintptr_t>(par) & 7)))) {
        set_error("%s: the table must be non-null and 16-byte aligned, the parameters non-null and 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    Gather g;
    bool ident;
    if (int rc = plan_gather(what, n, bits, k, controls, nc, batch, C128, &g, &ident)) return rc;
    if (table_bstride != 0 && table_bstride != (int64_t)1 << k) {
        set_error("%s: table batch stride %lld, 0 (shared) or 2^k expected", what, (long long)table_bstride);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const dim3 grid(blocks_of(nvec), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    hipStream_t s = as_stream(stream);
    if (ident)
        hipLaunchKernelGGL((diag_apply_kernel<T, MODE, true>), grid, dim3(ST_THREADS), 0, s, pi, po, table, table_bstride, par, g, n,
                           units_of(nvec));
    else
        hipLaunchKernelGGL((diag_apply_kernel<T, MODE, false>), grid, dim3(ST_THREADS), 0, s, pi, po, table, table_bstride, par, g, n,
                           units_of(nvec));
    return check_launch(what);
}

template <typename T>
int cost_impl(const void* in, void* out, const void* cost, const double* par, int op, int n, const int* bits, int k,
              const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    if (op == DQ_COST_PHASE)
        return apply_impl<T, MODE_PHASE>("dq_apply_cost", in, out, cost, 0, par, n, bits, k, controls, nc, batch, stream);
    if (op == DQ_COST_SCALE)
        return apply_impl<T, MODE_SCALE>("dq_apply_cost", in, out, cost, 0, par, n, bits, k, controls, nc, batch, stream);
    set_error("dq_apply_cost: op=%d is neither DQ_COST_PHASE nor DQ_COST_SCALE", op);
    return DQ_ERR_ARG;
}

template <typename T>
int cross_impl(const void* bra, const void* ket, const void* cost, int n, const int* bits, int k, const int* controls, int nc,
               int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_cost_cross";
    Gather g;
    bool ident;
    if (int rc = plan_gather(what, n, bits, k, controls, nc, batch, C128, &g, &ident)) return rc;
    if (int rc = check_cross(what, bra, ket, cost, true, out, ws, ws_bytes, n, batch, C128)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = blocks_of(nvec);
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    const T* pc = static_cast<const T*>(cost);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    const bool same = bra == ket;
#define DQ_CROSS(SAME, ID) \
    hipLaunchKernelGGL((cost_cross_kernel<T, SAME, ID>), grid, dim3(ST_THREADS), 0, s, pb, pk, pc, g, n, units_of(nvec), part)
    if (same && ident) DQ_CROSS(true, true);
    else if (same) DQ_CROSS(true, false);
    else if (ident) DQ_CROSS(false, true);
    else DQ_CROSS(false, false);
#undef DQ_CROSS
    return finish_cross(what, part, nblk, batch, out, s);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_diag_c64(const void* in, void* out, const void* diag, int64_t diag_batch_stride, int n, const int* bits,
                                 int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::apply_impl<float, dq::MODE_DIAG>("dq_apply_diag", in, out, diag, diag_batch_stride, nullptr, n, bits, k, controls, nc,
                                                batch, stream);
}
extern "C" int dq_apply_diag_c128(const void* in, void* out, const void* diag, int64_t diag_batch_stride, int n, const int* bits,
                                  int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::apply_impl<double, dq::MODE_DIAG>("dq_apply_diag", in, out, diag, diag_batch_stride, nullptr, n, bits, k, controls, nc,
                                                 batch, stream);
}

extern "C" int dq_apply_cost_c64(const void* in, void* out, const void* cost, const double* t, int op, int n, const int* bits,
                                 int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::cost_impl<float>(in, out, cost, t, op, n, bits, k, controls, nc, batch, stream);
}
extern "C" int dq_apply_cost_c128(const void* in, void* out, const void* cost, const double* t, int op, int n, const int* bits,
                                  int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::cost_impl<double>(in, out, cost, t, op, n, bits, k, controls, nc, batch, stream);
}

extern "C" int64_t dq_cost_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross) {
    (void)cross;        // bra != ket reads twice as much and writes the same partial sums
    return dq::cross_ws_bytes_or_refuse(n, batch, is_c128 != 0);
}

extern "C" int dq_cost_cross_c64(const void* bra, const void* ket, const void* cost, int n, const int* bits, int k,
                                 const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                 dq_stream_t stream) {
    return dq::cross_impl<float>(bra, ket, cost, n, bits, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_cost_cross_c128(const void* bra, const void* ket, const void* cost, int n, const int* bits, int k,
                                  const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                  dq_stream_t stream) {
    return dq::cross_impl<double>(bra, ket, cost, n, bits, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
