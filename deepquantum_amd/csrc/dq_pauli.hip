// Pauli strings on any number of wires: a a-plus-c-P combination and a cross reduction, one read (and one write) of the
// state whatever the weight of the string.
//
//     (P psi)[i] = i^ny * (-1)^popc((i ^ x) & z) * psi[i ^ x]          x = xmask, z = zmask, ny = popc(x & z)
//     dq_apply_pauli_axpby : out[b, i] = a[b] in[b, i] + c[b] (P in_b)[i]
//     dq_pauli_cross       : out[b] = sum_i conj(bra[b, i]) (P ket_b)[i]
// on the amplitudes whose control bits are all 1; the others pass through (GATE), come out as 0 (MAP: the cotangent of
// the sum that leaves them out) or are left out (cross).  The controls are disjoint from x | z, so both ends of a pair
// i, i ^ x are inside the controls or both are outside.
//
// Geometry.  That of dq_stream.hpp; vx = x >> VB is the flip over vector indices and x0 (complex64 only) the flip
// inside a vector, a swap of registers.  Both kernels are written once, with the item as the template parameter PAIR:
//   * vx != 0: the item is a PAIR of vectors.  Pair P of the 2^(nv - 1) pairs of a sample is
//         vA = P with a zero inserted at the top set bit of vx,        vB = vA ^ vx
//     so every vector belongs to exactly one pair whatever vx is -- a flip above, inside or across any tile size is
//     the same line of code.  A lane owns ST_UNROLL = 4 pairs per iteration: it loads both ends of all four (eight
//     loads in flight), computes both outputs of each and stores both.  Nobody else reads or writes them: in == out
//     is safe, and the traffic is one read and one write.
//   * vx == 0 (x = 0, or complex64 x = 1): no partner, the item is a vector: the partner of an amplitude is itself
//     or (complex64, x0) its neighbour in the vector.
//
// Arithmetic.  i^ny and the sign are a swap and two negations of components; a and c arrive as doubles and are
// rounded once to the state's real precision.  No table, no trigonometry.
//
// Reduction.  Lanes accumulate in double over their items; the rest is dq_stream.hpp's fixed-order scheme.  bra == ket
// loads each pair once and adds both of its terms.
#include "dq_stream.hpp"

namespace dq {

namespace {

struct Pauli {
    uint64_t vx;                                        // xmask over vector indices
    uint64_t z, cmask;                                  // over amplitude indices
    int top;                                            // the top set bit of vx (unused when vx == 0)
    int x0;                                             // complex64: bit 0 of xmask, the flip inside a vector
    int ny;                                             // popc(xmask & zmask) mod 4
};

// i^ny (-1)^popc(j & z) s: what the source amplitude s at index j contributes to (P psi)[j ^ x]
template <typename V> __device__ __forceinline__ V pauli_term(V s, uint64_t j, const Pauli& p) {
    const bool neg = (__popcll(j & p.z) & 1) != 0;
    const bool odd = (p.ny & 1) != 0;
    const bool nre = neg != (p.ny == 1 || p.ny == 2), nim = neg != (p.ny == 2 || p.ny == 3);
    V r;
    r.x = odd ? s.y : s.x;
    r.y = odd ? s.x : s.y;
    r.x = nre ? -r.x : r.x;
    r.y = nim ? -r.y : r.y;
    return r;
}

// a own + c w inside the controls; outside them own (GATE) or 0 (MAP)
template <typename T, int MODE> __device__ __forceinline__ cx<T> combine(cx<T> own, cx<T> w, cx<T> a, cx<T> c, bool ok) {
    if (!ok) return MODE == DQ_PAULI_MAP ? mk<T>((T)0, (T)0) : own;
    return mk<T>(a.x * own.x - a.y * own.y + c.x * w.x - c.y * w.y, a.x * own.y + a.y * own.x + c.x * w.y + c.y * w.x);
}

template <typename T> __device__ __forceinline__ void load_coef(const double* coef, uint64_t b, cx<T>& a, cx<T>& c) {
    a = mk<T>((T)coef[4 * b], (T)coef[4 * b + 1]);
    c = mk<T>((T)coef[4 * b + 2], (T)coef[4 * b + 3]);
}

// The first (PAIR: lower) vector of item `it`
template <bool PAIR> __device__ __forceinline__ uint64_t item_vector(uint64_t it, const Pauli& p) {
    return PAIR ? insert_zero(it, p.top) : it;
}

// in and out may be the same buffer: no __restrict__ on them
template <typename T, int MODE, bool PAIR>
__global__ __launch_bounds__(ST_THREADS) void pauli_axpby_kernel(const cx<T>* in, cx<T>* out, const double* __restrict__ coef,
                                                                 Pauli p, int n, uint64_t items) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    cx<T> a, c;
    load_coef<T>(coef, b, a, c);
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < items; unit += gridDim.x) {
        const uint64_t i0 = (unit << ST_UNIT_BITS) + threadIdx.x;
        Q qa[ST_UNROLL], qb[ST_UNROLL];                 // (qb: PAIR only)
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
                const uint64_t va = item_vector<PAIR>(it, p);
                qa[u] = src[va];
                if constexpr (PAIR) qb[u] = src[va ^ p.vx];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
                const uint64_t va = item_vector<PAIR>(it, p), vb = PAIR ? va ^ p.vx : va;
                const Q& qo = PAIR ? qb[u] : qa[u];     // where the partners of qa's amplitudes are
                Q ra, rb;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int f = VEC == 2 ? e ^ p.x0 : 0;          // the partner's element
                    const uint64_t ia = (va << VB) | (uint64_t)e, ja = (vb << VB) | (uint64_t)f, jb = (va << VB) | (uint64_t)f;
                    const bool ok = (ia & p.cmask) == p.cmask;      // (the same for both ends)
                    vec_set(ra, e, combine<T, MODE>(vec_get<T>(qa[u], e), pauli_term(vec_get<T>(qo, f), ja, p), a, c, ok));
                    if constexpr (PAIR)
                        vec_set(rb, e, combine<T, MODE>(vec_get<T>(qb[u], e), pauli_term(vec_get<T>(qa[u], f), jb, p), a, c, ok));
                }
                dst[va] = ra;
                if constexpr (PAIR) dst[vb] = rb;
            }
        }
    }
}

// (re, im) += conj(a) w, in double
template <typename V> __device__ __forceinline__ void cross_add(V a, V w, bool ok, double& re, double& im) {
    if (ok) {
        const double ar = (double)a.x, ai = (double)a.y, wr = (double)w.x, wi = (double)w.y;
        re = fma(ar, wr, fma(ai, wi, re));
        im = fma(ar, wi, fma(-ai, wr, im));
    }
}

// ws[b, blockIdx.x] = this workgroup's part of sum_i conj(bra_i) (P ket)_i
template <typename T, bool SAME, bool PAIR>
__global__ __launch_bounds__(ST_THREADS) void pauli_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                 Pauli p, int n, uint64_t items, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    double re = 0.0, im = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < items; unit += gridDim.x) {
        const uint64_t i0 = (unit << ST_UNIT_BITS) + threadIdx.x;
        Q ka[ST_UNROLL], kb[ST_UNROLL], ba[ST_UNROLL], bb[ST_UNROLL];           // (kb, bb: PAIR only; ba, bb: !SAME only)
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
                const uint64_t va = item_vector<PAIR>(it, p), vb = va ^ p.vx;
                ka[u] = pk[va];
                if constexpr (PAIR) kb[u] = pk[vb];
                if constexpr (!SAME) ba[u] = pb[va];
                if constexpr (!SAME && PAIR) bb[u] = pb[vb];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
                const uint64_t va = item_vector<PAIR>(it, p), vb = PAIR ? va ^ p.vx : va;
                const Q& ko = PAIR ? kb[u] : ka[u];     // where the partners of ka's amplitudes are
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int f = VEC == 2 ? e ^ p.x0 : 0;
                    const uint64_t ia = (va << VB) | (uint64_t)e, ja = (vb << VB) | (uint64_t)f, jb = (va << VB) | (uint64_t)f;
                    const bool ok = (ia & p.cmask) == p.cmask;
                    cross_add(vec_get<T>(SAME ? ka[u] : ba[u], e), pauli_term(vec_get<T>(ko, f), ja, p), ok, re, im);
                    if constexpr (PAIR)
                        cross_add(vec_get<T>(SAME ? kb[u] : bb[u], e), pauli_term(vec_get<T>(ka[u], f), jb, p), ok, re, im);
                }
            }
        }
    }
    write_partial(re, im, sh, ws);
}

// Validates the masks and the controls and splits the string for the kernels.
int plan_pauli(const char* what, uint64_t xmask, uint64_t zmask, int n, const int* controls, int nc, int64_t batch, bool is_c128,
               Pauli* p) {
    if (int rc = validate_bits(n, nullptr, 0, controls, nc)) return rc;
    if (n < 64 && ((xmask | zmask) >> n) != 0) {
        set_error("%s: xmask=0x%llx / zmask=0x%llx have bits at or above n=%d", what, (unsigned long long)xmask,
                  (unsigned long long)zmask, n);
        return DQ_ERR_ARG;
    }
    if (int rc = check_batch(what, batch)) return rc;
    *p = Pauli{};
    p->cmask = control_mask(controls, nc);
    if (p->cmask & (xmask | zmask)) {
        set_error("%s: a control lies inside the Pauli string (controls 0x%llx, string 0x%llx)", what,
                  (unsigned long long)p->cmask, (unsigned long long)(xmask | zmask));
        return DQ_ERR_ARG;
    }
    const int vb = is_c128 ? 0 : 1;
    p->vx = xmask >> vb;
    p->x0 = is_c128 ? 0 : (int)(xmask & 1ull);
    p->z = zmask;
    p->ny = __builtin_popcountll(xmask & zmask) & 3;
    p->top = p->vx ? 63 - __builtin_clzll(p->vx) : 0;
    return DQ_OK;
}

template <typename T>
int axpby_impl(const void* in, void* out, uint64_t xmask, uint64_t zmask, const double* coef, int mode, int n, const int* controls,
               int nc, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_pauli_axpby";
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), SAME_OR_DISJOINT)) return rc;
    if (!coef || (reinterpret_cast<uintptr_t>(coef) & 7)) {
        set_error("%s: coef must be non-null and 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (mode != DQ_PAULI_GATE && mode != DQ_PAULI_MAP) {
        set_error("%s: mode=%d is neither DQ_PAULI_GATE nor DQ_PAULI_MAP", what, mode);
        return DQ_ERR_ARG;
    }
    Pauli p;
    if (int rc = plan_pauli(what, xmask, zmask, n, controls, nc, batch, C128, &p)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const uint64_t items = p.vx ? nvec >> 1 : nvec;
    const dim3 grid(blocks_of(items), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    hipStream_t s = as_stream(stream);
#define DQ_AXPBY(MODE, PAIR) \
    hipLaunchKernelGGL((pauli_axpby_kernel<T, MODE, PAIR>), grid, dim3(ST_THREADS), 0, s, pi, po, coef, p, n, items)
    if (p.vx && mode == DQ_PAULI_GATE) DQ_AXPBY(DQ_PAULI_GATE, true);
    else if (p.vx) DQ_AXPBY(DQ_PAULI_MAP, true);
    else if (mode == DQ_PAULI_GATE) DQ_AXPBY(DQ_PAULI_GATE, false);
    else DQ_AXPBY(DQ_PAULI_MAP, false);
#undef DQ_AXPBY
    return check_launch(what);
}

template <typename T>
int cross_impl(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls, int nc, int64_t batch,
               double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_pauli_cross";
    Pauli p;
    if (int rc = plan_pauli(what, xmask, zmask, n, controls, nc, batch, C128, &p)) return rc;
    if (int rc = check_cross(what, bra, ket, nullptr, false, out, ws, ws_bytes, n, batch, C128)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const uint64_t items = p.vx ? nvec >> 1 : nvec;
    const unsigned nblk = blocks_of(items);             // (at most what the workspace was sized for)
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    const bool same = bra == ket;
#define DQ_CROSS(SAME, PAIR) \
    hipLaunchKernelGGL((pauli_cross_kernel<T, SAME, PAIR>), grid, dim3(ST_THREADS), 0, s, pb, pk, p, n, items, part)
    if (p.vx && same) DQ_CROSS(true, true);
    else if (p.vx) DQ_CROSS(false, true);
    else if (same) DQ_CROSS(true, false);
    else DQ_CROSS(false, false);
#undef DQ_CROSS
    return finish_cross(what, part, nblk, batch, out, s);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_pauli_axpby_c64(const void* in, void* out, uint64_t xmask, uint64_t zmask, const double* coef, int mode,
                                        int n, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::axpby_impl<float>(in, out, xmask, zmask, coef, mode, n, controls, nc, batch, stream);
}
extern "C" int dq_apply_pauli_axpby_c128(const void* in, void* out, uint64_t xmask, uint64_t zmask, const double* coef, int mode,
                                         int n, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::axpby_impl<double>(in, out, xmask, zmask, coef, mode, n, controls, nc, batch, stream);
}

extern "C" int64_t dq_pauli_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross) {
    (void)cross;        // bra != ket reads twice as much and writes the same partial sums
    return dq::cross_ws_bytes_or_refuse(n, batch, is_c128 != 0);
}

extern "C" int dq_pauli_cross_c64(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls,
                                  int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::cross_impl<float>(bra, ket, xmask, zmask, n, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_pauli_cross_c128(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls,
                                   int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::cross_impl<double>(bra, ket, xmask, zmask, n, controls, nc, batch, out, ws, ws_bytes, stream);
}
