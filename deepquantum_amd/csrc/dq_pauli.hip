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
// Geometry.  A lane moves 16 bytes (two complex64 or one complex128 amplitude) per load; vx = x >> VB is the flip over
// vector indices and x0 (complex64 only) the flip inside a vector, a swap of registers.
//   * vx != 0: the unit of work is a PAIR of vectors.  Pair P of the 2^(nv - 1) pairs of a sample is
//         vA = P with a zero inserted at the top set bit of vx,        vB = vA ^ vx
//     so every vector belongs to exactly one pair whatever vx is -- a flip above, inside or across any tile size is
//     the same line of code.  A lane owns PL_UNROLL = 4 pairs per iteration: it loads both ends of all four (eight
//     loads in flight), computes both outputs of each and stores both.  Nobody else reads or writes them: in == out
//     is safe, and the traffic is one read and one write.
//   * vx == 0 (x = 0, or complex64 x = 1): no partner, a lane owns four vectors per iteration.
// A workgroup of 256 lanes takes a unit of 1024 pairs (vectors) per iteration, at most PL_BLOCKS workgroups per sample
// stride over the units; the sample is the grid's y dimension.
//
// Arithmetic.  i^ny and the sign are a swap and two negations of components; a and c arrive as doubles and are
// rounded once to the state's real precision.  No table, no trigonometry.
//
// Reduction.  As in dq_diag.hip: lanes accumulate in double, a wave adds its lanes with an xor butterfly, lane 0 adds
// the four waves in order and writes the workgroup's partial sum; a second kernel adds a sample's partial sums the
// same way.  No atomics, every sum in a fixed order: bitwise reproducible.  bra == ket loads each pair once and adds
// both of its terms.
#include "dq_common.hpp"

namespace dq {

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_UNROLL = 4;                            // pairs (vx != 0) or vectors (vx == 0) per lane and iteration
constexpr int PL_UNIT_BITS = 10;                        // log2(PL_THREADS * PL_UNROLL)
constexpr unsigned PL_BLOCKS = 2048;                    // workgroups per sample striding over its units

struct Pauli {
    uint64_t vx;                                        // xmask over vector indices
    uint64_t z, cmask;                                  // over amplitude indices
    int top;                                            // the top set bit of vx (unused when vx == 0)
    int x0;                                             // complex64: bit 0 of xmask, the flip inside a vector
    int ny;                                             // popc(xmask & zmask) mod 4
};

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<double> { using type = double2; };

template <typename T> __device__ __forceinline__ cx<T> vec_get(const typename Vec16<T>::type& q, int e);
template <> __device__ __forceinline__ float2 vec_get<float>(const float4& q, int e) {
    return e ? make_float2(q.z, q.w) : make_float2(q.x, q.y);
}
template <> __device__ __forceinline__ double2 vec_get<double>(const double2& q, int) { return q; }
__device__ __forceinline__ void vec_set(float4& q, int e, float2 a) {
    if (e) { q.z = a.x; q.w = a.y; } else { q.x = a.x; q.y = a.y; }
}
__device__ __forceinline__ void vec_set(double2& q, int, double2 a) { q = a; }

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

// vx != 0.  in and out may be the same buffer: no __restrict__ on them
template <typename T, int MODE>
__global__ __launch_bounds__(PL_THREADS) void pauli_pair_kernel(const cx<T>* in, cx<T>* out, const double* __restrict__ coef,
                                                                Pauli p, int n, uint64_t npairs) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    cx<T> a, c;
    load_coef<T>(coef, b, a, c);
    for (uint64_t unit = blockIdx.x; (unit << PL_UNIT_BITS) < npairs; unit += gridDim.x) {
        const uint64_t p0 = (unit << PL_UNIT_BITS) + threadIdx.x;
        Q qa[PL_UNROLL], qb[PL_UNROLL];
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t pr = p0 + (uint64_t)(u * PL_THREADS);
            if (pr < npairs) {
                const uint64_t va = insert_zero(pr, p.top);
                qa[u] = src[va];
                qb[u] = src[va ^ p.vx];
            }
        }
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t pr = p0 + (uint64_t)(u * PL_THREADS);
            if (pr < npairs) {
                const uint64_t va = insert_zero(pr, p.top), vb = va ^ p.vx;
                Q ra, rb;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int f = VEC == 2 ? e ^ p.x0 : 0;          // the partner's element
                    const uint64_t ia = (va << VB) | (uint64_t)e, ja = (vb << VB) | (uint64_t)f, jb = (va << VB) | (uint64_t)f;
                    const bool ok = (ia & p.cmask) == p.cmask;      // (the same for both ends)
                    vec_set(ra, e, combine<T, MODE>(vec_get<T>(qa[u], e), pauli_term(vec_get<T>(qb[u], f), ja, p), a, c, ok));
                    vec_set(rb, e, combine<T, MODE>(vec_get<T>(qb[u], e), pauli_term(vec_get<T>(qa[u], f), jb, p), a, c, ok));
                }
                dst[va] = ra;
                dst[vb] = rb;
            }
        }
    }
}

// vx == 0: the partner is the amplitude itself or (complex64, x0) its neighbour in the vector
template <typename T, int MODE>
__global__ __launch_bounds__(PL_THREADS) void pauli_self_kernel(const cx<T>* in, cx<T>* out, const double* __restrict__ coef,
                                                                Pauli p, int n, uint64_t nvec) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    cx<T> a, c;
    load_coef<T>(coef, b, a, c);
    for (uint64_t unit = blockIdx.x; (unit << PL_UNIT_BITS) < nvec; unit += gridDim.x) {
        const uint64_t v0 = (unit << PL_UNIT_BITS) + threadIdx.x;
        Q q[PL_UNROLL];
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * PL_THREADS);
            if (v < nvec) q[u] = src[v];
        }
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * PL_THREADS);
            if (v < nvec) {
                Q r;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int f = VEC == 2 ? e ^ p.x0 : 0;
                    const uint64_t i = (v << VB) | (uint64_t)e, j = (v << VB) | (uint64_t)f;
                    const bool ok = (i & p.cmask) == p.cmask;
                    vec_set(r, e, combine<T, MODE>(vec_get<T>(q[u], e), pauli_term(vec_get<T>(q[u], f), j, p), a, c, ok));
                }
                dst[v] = r;
            }
        }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the workgroup's sum of (re, im), in thread 0; fixed order
__device__ __forceinline__ void block_sum(double& re, double& im, double (*sh)[2]) {
    re = wave_sum(re);
    im = wave_sum(im);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[wave][0] = re;
        sh[wave][1] = im;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        re = sh[0][0];
        im = sh[0][1];
        for (int w = 1; w < PL_THREADS / 64; ++w) {
            re += sh[w][0];
            im += sh[w][1];
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

__device__ __forceinline__ void write_partial(double re, double im, double (*sh)[2], double* ws) {
    block_sum(re, im, sh);
    if (threadIdx.x == 0) {
        double* part = ws + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        part[0] = re;
        part[1] = im;
    }
}

// ws[b, blockIdx.x] = this workgroup's part of sum_i conj(bra_i) (P ket)_i, vx != 0
template <typename T, bool SAME>
__global__ __launch_bounds__(PL_THREADS) void pauli_cross_pair_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                      Pauli p, int n, uint64_t npairs, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    __shared__ double sh[PL_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    double re = 0.0, im = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << PL_UNIT_BITS) < npairs; unit += gridDim.x) {
        const uint64_t p0 = (unit << PL_UNIT_BITS) + threadIdx.x;
        Q ka[PL_UNROLL], kb[PL_UNROLL], ba[PL_UNROLL], bb[PL_UNROLL];
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t pr = p0 + (uint64_t)(u * PL_THREADS);
            if (pr < npairs) {
                const uint64_t va = insert_zero(pr, p.top), vb = va ^ p.vx;
                ka[u] = pk[va];
                kb[u] = pk[vb];
                if (!SAME) {
                    ba[u] = pb[va];
                    bb[u] = pb[vb];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t pr = p0 + (uint64_t)(u * PL_THREADS);
            if (pr < npairs) {
                const uint64_t va = insert_zero(pr, p.top), vb = va ^ p.vx;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int f = VEC == 2 ? e ^ p.x0 : 0;
                    const uint64_t ia = (va << VB) | (uint64_t)e, ja = (vb << VB) | (uint64_t)f, jb = (va << VB) | (uint64_t)f;
                    const bool ok = (ia & p.cmask) == p.cmask;
                    cross_add(vec_get<T>(SAME ? ka[u] : ba[u], e), pauli_term(vec_get<T>(kb[u], f), ja, p), ok, re, im);
                    cross_add(vec_get<T>(SAME ? kb[u] : bb[u], e), pauli_term(vec_get<T>(ka[u], f), jb, p), ok, re, im);
                }
            }
        }
    }
    write_partial(re, im, sh, ws);
}

// the same with vx == 0
template <typename T, bool SAME>
__global__ __launch_bounds__(PL_THREADS) void pauli_cross_self_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                      Pauli p, int n, uint64_t nvec, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    __shared__ double sh[PL_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    double re = 0.0, im = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << PL_UNIT_BITS) < nvec; unit += gridDim.x) {
        const uint64_t v0 = (unit << PL_UNIT_BITS) + threadIdx.x;
        Q qk[PL_UNROLL], qb[PL_UNROLL];
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * PL_THREADS);
            if (v < nvec) {
                qk[u] = pk[v];
                if (!SAME) qb[u] = pb[v];
            }
        }
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * PL_THREADS);
            if (v < nvec) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int f = VEC == 2 ? e ^ p.x0 : 0;
                    const uint64_t i = (v << VB) | (uint64_t)e, j = (v << VB) | (uint64_t)f;
                    cross_add(vec_get<T>(SAME ? qk[u] : qb[u], e), pauli_term(vec_get<T>(qk[u], f), j, p), (i & p.cmask) == p.cmask,
                              re, im);
                }
            }
        }
    }
    write_partial(re, im, sh, ws);
}

// out[b] = the sum of the nparts partial sums of sample b
__global__ __launch_bounds__(PL_THREADS) void pauli_cross_finish_kernel(const double* __restrict__ ws, unsigned nparts,
                                                                        double* __restrict__ out) {
    __shared__ double sh[PL_THREADS / 64][2];
    const uint64_t b = blockIdx.x;
    double re = 0.0, im = 0.0;
    for (unsigned q = threadIdx.x; q < nparts; q += PL_THREADS) {
        re += ws[(b * nparts + q) * 2];
        im += ws[(b * nparts + q) * 2 + 1];
    }
    block_sum(re, im, sh);
    if (threadIdx.x == 0) {
        out[2 * b] = re;
        out[2 * b + 1] = im;
    }
}

unsigned blocks_of(uint64_t items) {
    const uint64_t units = (items + (1ull << PL_UNIT_BITS) - 1) >> PL_UNIT_BITS;
    return (unsigned)(units < PL_BLOCKS ? units : PL_BLOCKS);
}

uint64_t vectors_of(int n, bool is_c128) { return 1ull << (n - (is_c128 ? 0 : 1)); }          // (n >= 1)

// Validates the masks and the controls and splits the string for the kernels.
int plan_pauli(const char* what, uint64_t xmask, uint64_t zmask, int n, const int* controls, int nc, int64_t batch, bool is_c128,
               Pauli* p) {
    if (int rc = validate_bits(n, nullptr, 0, controls, nc)) return rc;
    if (n < 64 && ((xmask | zmask) >> n) != 0) {
        set_error("%s: xmask=0x%llx / zmask=0x%llx have bits at or above n=%d", what, (unsigned long long)xmask,
                  (unsigned long long)zmask, n);
        return DQ_ERR_ARG;
    }
    if (batch < 1 || batch > 65535) {
        set_error("%s: batch=%lld outside [1, 65535]", what, (long long)batch);
        return DQ_ERR_ARG;
    }
    *p = Pauli{};
    for (int c = 0; c < nc; ++c) p->cmask |= 1ull << controls[c];
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

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

template <typename T>
int axpby_impl(const void* in, void* out, uint64_t xmask, uint64_t zmask, const double* coef, int mode, int n, const int* controls,
               int nc, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_pauli_axpby";
    if (!in || !out || !coef) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    if (mode != DQ_PAULI_GATE && mode != DQ_PAULI_MAP) {
        set_error("%s: mode=%d is neither DQ_PAULI_GATE nor DQ_PAULI_MAP", what, mode);
        return DQ_ERR_ARG;
    }
    Pauli p;
    if (int rc = plan_pauli(what, xmask, zmask, n, controls, nc, batch, C128, &p)) return rc;
    if (misaligned(in) || misaligned(out) || (reinterpret_cast<uintptr_t>(coef) & 7)) {
        set_error("%s: in and out must be 16-byte aligned, coef 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const uint64_t items = p.vx ? nvec >> 1 : nvec;
    const dim3 grid(blocks_of(items), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    hipStream_t s = as_stream(stream);
#define DQ_AXPBY(KERNEL, MODE) hipLaunchKernelGGL((KERNEL<T, MODE>), grid, dim3(PL_THREADS), 0, s, pi, po, coef, p, n, items)
    if (p.vx && mode == DQ_PAULI_GATE) DQ_AXPBY(pauli_pair_kernel, DQ_PAULI_GATE);
    else if (p.vx) DQ_AXPBY(pauli_pair_kernel, DQ_PAULI_MAP);
    else if (mode == DQ_PAULI_GATE) DQ_AXPBY(pauli_self_kernel, DQ_PAULI_GATE);
    else DQ_AXPBY(pauli_self_kernel, DQ_PAULI_MAP);
#undef DQ_AXPBY
    return check_launch(what);
}

int64_t cross_ws_bytes(int n, int64_t batch, bool is_c128) {
    return batch * (int64_t)blocks_of(vectors_of(n, is_c128)) * 2 * (int64_t)sizeof(double);
}

template <typename T>
int cross_impl(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls, int nc, int64_t batch,
               double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_pauli_cross";
    if (!bra || !ket || !out || !ws) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    Pauli p;
    if (int rc = plan_pauli(what, xmask, zmask, n, controls, nc, batch, C128, &p)) return rc;
    if (misaligned(bra) || misaligned(ket) || misaligned(ws) || (reinterpret_cast<uintptr_t>(out) & 7)) {
        set_error("%s: bra, ket and ws must be 16-byte aligned, out 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    const int64_t need = cross_ws_bytes(n, batch, C128);
    if (ws_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (dq_pauli_cross_ws_bytes)", what, (long long)ws_bytes, (long long)need);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const uint64_t items = p.vx ? nvec >> 1 : nvec;
    const unsigned nblk = blocks_of(items);             // (at most what the workspace was sized for)
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    const bool same = bra == ket;
#define DQ_CROSS(KERNEL, SAME) hipLaunchKernelGGL((KERNEL<T, SAME>), grid, dim3(PL_THREADS), 0, s, pb, pk, p, n, items, part)
    if (p.vx && same) DQ_CROSS(pauli_cross_pair_kernel, true);
    else if (p.vx) DQ_CROSS(pauli_cross_pair_kernel, false);
    else if (same) DQ_CROSS(pauli_cross_self_kernel, true);
    else DQ_CROSS(pauli_cross_self_kernel, false);
#undef DQ_CROSS
    hipLaunchKernelGGL(pauli_cross_finish_kernel, dim3((unsigned)batch), dim3(PL_THREADS), 0, s, part, nblk, out);
    return check_launch(what);
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
    if (n < 1 || n > 40 || batch < 1 || batch > 65535) return -1;
    return dq::cross_ws_bytes(n, batch, is_c128 != 0);
}

extern "C" int dq_pauli_cross_c64(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls,
                                  int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::cross_impl<float>(bra, ket, xmask, zmask, n, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_pauli_cross_c128(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls,
                                   int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::cross_impl<double>(bra, ket, xmask, zmask, n, controls, nc, batch, out, ws, ws_bytes, stream);
}
