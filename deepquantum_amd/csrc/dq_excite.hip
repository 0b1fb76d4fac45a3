// Excitation gates (Givens rotations) that touch only their subspace: an a-plus-c-K combination and a cross reduction
// over the pairs of one pattern pair, reading and writing nothing else.
//
//     K = E - E^dagger, E an excitation |amask pattern> -> |the other pattern> on the bits of xmask.  For every i0 with
//     i0 & xmask == amask and every control bit 1, i1 = i0 ^ xmask and sigma = (-1)^(negate + popc(i0 & zmask)):
//         (K psi)[i1] = sigma psi[i0]          (K psi)[i0] = -sigma psi[i1]          (K psi)[i] = 0 elsewhere
//     dq_apply_excite_axpby : out[b, i] = a[b] in[b, i] + c[b] (K in_b)[i]       on i0, i1 of every pair
//     dq_excite_cross       : out[b] = sum_i conj(bra[b, i]) (K ket_b)[i]
// The pairs are 2 / 2^(popc(xmask) + nc) of the state; the kernels load and store the 16-byte vectors that hold one of
// them and no others.  An amplitude that shares a vector with a pair's end without being one (complex64, bit 0 fixed)
// is a bystander: it is copied bitwise (GATE) or comes out as 0 (MAP).
//
// Geometry.  That of dq_stream.hpp, over the FREE bits only.  The fixed bits are xmask | controls; vx = xmask >> VB is
// the flip over vector indices and x0 (complex64) the flip inside a vector.  The item index runs over the free
// vector-index bits: vector vA = deposit(item) | pattern, vB = vA ^ vx.  The host cuts the deposit into runs of
// consecutive free positions and splits them at the size of a unit (dq_stream.hpp's Gather, read the other way round:
// src is a bit of the item index, dst one of the vector index): the runs below depend on the lane alone and are
// evaluated once, before the loop, the runs above on the unit alone -- scalar arithmetic, once per iteration.  The
// parity of i0 & zmask splits the same way.
//   * vx != 0: the item is a PAIR of vectors.  A lane owns ST_UNROLL = 4 pairs per iteration: eight loads in flight,
//     both outputs of each computed and stored.  Nobody else reads or writes them: in == out is safe.
//   * vx == 0 (complex64, xmask == 1): both ends lie in one vector, the item is that vector.
//
// Arithmetic.  a and c arrive as doubles and are rounded once to the state's real precision; sigma is a negation.  No
// table, no trigonometry.
//
// Reduction.  Lanes accumulate in double over their items; the rest is dq_stream.hpp's fixed-order scheme.  bra == ket
// loads each pair once.
#include "dq_stream.hpp"

namespace dq {

namespace {

struct Excite {
    Gather dep;                                         // item index -> free vector-index bits (cmask unused)
    uint64_t vpat;                                      // the fixed bits of vA: (amask | controls) >> VB
    uint64_t vx;                                        // xmask over vector indices
    uint64_t z;                                         // zmask over amplitude indices
    int x0;                                             // complex64: bit 0 of xmask, the flip inside a vector
    int m0, p0;                                         // complex64: bit 0 is fixed / its value at i0
    int negate;                                         // sigma's sign where i0 & zmask == 0
    int map;                                            // bystanders come out as 0
};

// the lane's part of the deposit: item bits below the unit size
__device__ __forceinline__ uint64_t deposit_low(const Gather& g, uint64_t low) {
    uint64_t v = 0;
    for (int r = 0; r < g.nlow; ++r) v |= ((low >> g.src[r]) & ((1ull << g.len[r]) - 1ull)) << g.dst[r];
    return v;
}

// What a lane keeps across the loop: the low part of vA of each of its items and the parity that part gives i0 & zmask.
template <int VB> struct ExciteLane {
    uint64_t low[ST_UNROLL];
    unsigned par;                                       // bit u
};

template <int VB> __device__ __forceinline__ void excite_lane(const Excite& p, ExciteLane<VB>& ln) {
    ln.par = 0;
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        ln.low[u] = deposit_low(p.dep, (uint64_t)(u * ST_THREADS + (int)threadIdx.x));
        ln.par |= (unsigned)(__popcll((ln.low[u] << VB) & p.z) & 1) << u;
    }
}

template <typename T> __device__ __forceinline__ void load_coef(const double* coef, uint64_t b, cx<T>& a, cx<T>& c) {
    a = mk<T>((T)coef[4 * b], (T)coef[4 * b + 1]);
    c = mk<T>((T)coef[4 * b + 2], (T)coef[4 * b + 3]);
}

template <typename V> __device__ __forceinline__ V signed_amp(V s, bool neg) {
    V r;
    r.x = neg ? -s.x : s.x;
    r.y = neg ? -s.y : s.y;
    return r;
}

// a own + c w
template <typename T> __device__ __forceinline__ cx<T> combine(cx<T> own, cx<T> w, cx<T> a, cx<T> c) {
    return mk<T>(a.x * own.x - a.y * own.y + c.x * w.x - c.y * w.y, a.x * own.y + a.y * own.x + c.x * w.y + c.y * w.x);
}

// in and out may be the same buffer: no __restrict__ on them
template <typename T, bool PAIR>
__global__ __launch_bounds__(ST_THREADS) void excite_axpby_kernel(const cx<T>* in, cx<T>* out, const double* __restrict__ coef,
                                                                  Excite p, int n, uint64_t items) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    cx<T> a, c;
    load_coef<T>(coef, b, a, c);
    ExciteLane<VB> ln;
    excite_lane<VB>(p, ln);
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < items; unit += gridDim.x) {
        const uint64_t i0 = (unit << ST_UNIT_BITS) + threadIdx.x;
        const uint64_t hi = chunk_high(p.dep, ST_UNIT_BITS, unit) | p.vpat;
        const int hpar = (__popcll((hi << VB) & p.z) & 1) ^ p.negate;
        Q qa[ST_UNROLL], qb[ST_UNROLL];                 // (qb: PAIR only)
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            if (i0 + (uint64_t)(u * ST_THREADS) < items) {
                const uint64_t va = hi | ln.low[u];
                qa[u] = src[va];
                if constexpr (PAIR) qb[u] = src[va ^ p.vx];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            if (i0 + (uint64_t)(u * ST_THREADS) < items) {
                const uint64_t va = hi | ln.low[u];
                Q ra = qa[u], rb = PAIR ? qb[u] : qa[u];
                if (p.map) ra = rb = Q{};
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (VEC == 2 && (e & p.m0) != p.p0) continue;           // a bystander, or the other end
                    const int f = VEC == 2 ? e ^ p.x0 : 0;                  // the partner's element
                    const bool neg = ((hpar ^ (int)(ln.par >> u) ^ (VEC == 2 ? e & (int)p.z : 0)) & 1) != 0;
                    const cx<T> x0 = vec_get<T>(qa[u], e), x1 = vec_get<T>(PAIR ? qb[u] : qa[u], f);
                    vec_set(ra, e, combine<T>(x0, signed_amp(x1, !neg), a, c));
                    if constexpr (PAIR) vec_set(rb, f, combine<T>(x1, signed_amp(x0, neg), a, c));
                    else vec_set(ra, f, combine<T>(x1, signed_amp(x0, neg), a, c));
                }
                dst[va] = ra;
                if constexpr (PAIR) dst[va ^ p.vx] = rb;
            }
        }
    }
}

// (re, im) += conj(a) w, in double
template <typename V> __device__ __forceinline__ void cross_add(V a, V w, double& re, double& im) {
    const double ar = (double)a.x, ai = (double)a.y, wr = (double)w.x, wi = (double)w.y;
    re = fma(ar, wr, fma(ai, wi, re));
    im = fma(ar, wi, fma(-ai, wr, im));
}

// ws[b, blockIdx.x] = this workgroup's part of sum_i conj(bra_i) (K ket)_i
template <typename T, bool SAME, bool PAIR>
__global__ __launch_bounds__(ST_THREADS) void excite_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                  Excite p, int n, uint64_t items, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    ExciteLane<VB> ln;
    excite_lane<VB>(p, ln);
    double re = 0.0, im = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < items; unit += gridDim.x) {
        const uint64_t i0 = (unit << ST_UNIT_BITS) + threadIdx.x;
        const uint64_t hi = chunk_high(p.dep, ST_UNIT_BITS, unit) | p.vpat;
        const int hpar = (__popcll((hi << VB) & p.z) & 1) ^ p.negate;
        Q ka[ST_UNROLL], kb[ST_UNROLL], ba[ST_UNROLL], bb[ST_UNROLL];           // (kb, bb: PAIR only; ba, bb: !SAME only)
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            if (i0 + (uint64_t)(u * ST_THREADS) < items) {
                const uint64_t va = hi | ln.low[u], vb = va ^ p.vx;
                ka[u] = pk[va];
                if constexpr (PAIR) kb[u] = pk[vb];
                if constexpr (!SAME) ba[u] = pb[va];
                if constexpr (!SAME && PAIR) bb[u] = pb[vb];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            if (i0 + (uint64_t)(u * ST_THREADS) < items) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (VEC == 2 && (e & p.m0) != p.p0) continue;
                    const int f = VEC == 2 ? e ^ p.x0 : 0;
                    const bool neg = ((hpar ^ (int)(ln.par >> u) ^ (VEC == 2 ? e & (int)p.z : 0)) & 1) != 0;
                    const cx<T> k0 = vec_get<T>(ka[u], e), k1 = vec_get<T>(PAIR ? kb[u] : ka[u], f);
                    const cx<T> b0 = vec_get<T>(SAME ? ka[u] : ba[u], e);
                    const cx<T> b1 = vec_get<T>(SAME ? (PAIR ? kb[u] : ka[u]) : (PAIR ? bb[u] : ba[u]), f);
                    cross_add(b1, signed_amp(k0, neg), re, im);              // conj(bra[i1]) (K ket)[i1]
                    cross_add(b0, signed_amp(k1, !neg), re, im);             // conj(bra[i0]) (K ket)[i0]
                }
            }
        }
    }
    write_partial(re, im, sh, ws);
}

// Validates the masks and the controls and builds the deposit; *items = the pairs of a sample over vector indices.
int plan_excite(const char* what, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate, int n, const int* controls, int nc,
                int64_t batch, bool is_c128, Excite* p, uint64_t* items) {
    if (int rc = validate_bits(n, nullptr, 0, controls, nc)) return rc;
    if (int rc = check_batch(what, batch)) return rc;
    if (((xmask | zmask) >> n) != 0) {
        set_error("%s: xmask=0x%llx / zmask=0x%llx have bits at or above n=%d", what, (unsigned long long)xmask,
                  (unsigned long long)zmask, n);
        return DQ_ERR_ARG;
    }
    if (xmask == 0) {
        set_error("%s: xmask == 0: an excitation flips at least one bit", what);
        return DQ_ERR_ARG;
    }
    if (amask & ~xmask) {
        set_error("%s: amask=0x%llx is not a subset of xmask=0x%llx", what, (unsigned long long)amask, (unsigned long long)xmask);
        return DQ_ERR_ARG;
    }
    if (zmask & xmask) {
        set_error("%s: zmask=0x%llx and xmask=0x%llx share a bit (fold fixed bits into negate)", what, (unsigned long long)zmask,
                  (unsigned long long)xmask);
        return DQ_ERR_ARG;
    }
    if (negate != 0 && negate != 1) {
        set_error("%s: negate=%d is neither 0 nor 1", what, negate);
        return DQ_ERR_ARG;
    }
    const uint64_t cmask = control_mask(controls, nc);
    if (cmask & (xmask | zmask)) {
        set_error("%s: a control lies inside the masks (controls 0x%llx, xmask | zmask 0x%llx; fold fixed bits into negate)", what,
                  (unsigned long long)cmask, (unsigned long long)(xmask | zmask));
        return DQ_ERR_ARG;
    }
    *p = Excite{};
    const int vb = is_c128 ? 0 : 1;
    const uint64_t fixed = xmask | cmask;
    p->vpat = (amask | cmask) >> vb;
    p->vx = xmask >> vb;
    p->z = zmask;
    p->x0 = is_c128 ? 0 : (int)(xmask & 1ull);
    p->m0 = is_c128 ? 0 : (int)(fixed & 1ull);
    p->p0 = is_c128 ? 0 : (int)((amask | cmask) & 1ull);
    p->negate = negate;
    // runs of consecutive free vector-index positions, in ascending order, split at the unit size of the item index
    Gather& g = p->dep;
    int j = 0;                                          // the next bit of the item index
    for (int pos = 0; pos < n - vb;) {
        if ((fixed >> (pos + vb)) & 1ull) {
            ++pos;
            continue;
        }
        int len = 1;
        while (pos + len < n - vb && !((fixed >> (pos + len + vb)) & 1ull)) ++len;
        int src = j, dst = pos, left = len;
        if (src < ST_UNIT_BITS && src + left > ST_UNIT_BITS) {
            const int ll = ST_UNIT_BITS - src;
            g.src[g.nruns] = (uint8_t)src, g.len[g.nruns] = (uint8_t)ll, g.dst[g.nruns] = (uint8_t)dst;
            ++g.nruns;
            src += ll, dst += ll, left -= ll;
        }
        g.src[g.nruns] = (uint8_t)src, g.len[g.nruns] = (uint8_t)left, g.dst[g.nruns] = (uint8_t)dst;
        ++g.nruns;
        j += len;
        pos += len;
    }
    for (int r = 0; r < g.nruns; ++r) g.nlow += g.src[r] < ST_UNIT_BITS;
    *items = 1ull << j;
    return DQ_OK;
}

template <typename T>
int axpby_impl(const void* in, void* out, const double* coef, int mode, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate,
               int n, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_excite_axpby";
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), SAME_OR_DISJOINT)) return rc;
    if (!coef || (reinterpret_cast<uintptr_t>(coef) & 7)) {
        set_error("%s: coef must be non-null and 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (mode != DQ_EXCITE_GATE && mode != DQ_EXCITE_MAP) {
        set_error("%s: mode=%d is neither DQ_EXCITE_GATE nor DQ_EXCITE_MAP", what, mode);
        return DQ_ERR_ARG;
    }
    Excite p;
    uint64_t items;
    if (int rc = plan_excite(what, xmask, amask, zmask, negate, n, controls, nc, batch, C128, &p, &items)) return rc;
    p.map = mode == DQ_EXCITE_MAP;
    const dim3 grid(blocks_of(items), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    hipStream_t s = as_stream(stream);
    if (p.vx) hipLaunchKernelGGL((excite_axpby_kernel<T, true>), grid, dim3(ST_THREADS), 0, s, pi, po, coef, p, n, items);
    else hipLaunchKernelGGL((excite_axpby_kernel<T, false>), grid, dim3(ST_THREADS), 0, s, pi, po, coef, p, n, items);
    return check_launch(what);
}

template <typename T>
int cross_impl(const void* bra, const void* ket, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate, int n,
               const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_excite_cross";
    Excite p;
    uint64_t items;
    if (int rc = plan_excite(what, xmask, amask, zmask, negate, n, controls, nc, batch, C128, &p, &items)) return rc;
    if (int rc = check_cross(what, bra, ket, nullptr, false, out, ws, ws_bytes, n, batch, C128)) return rc;
    const unsigned nblk = blocks_of(items);             // (at most what the workspace was sized for: items <= vectors)
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    const bool same = bra == ket;
#define DQ_CROSS(SAME, PAIR) \
    hipLaunchKernelGGL((excite_cross_kernel<T, SAME, PAIR>), grid, dim3(ST_THREADS), 0, s, pb, pk, p, n, items, part)
    if (p.vx && same) DQ_CROSS(true, true);
    else if (p.vx) DQ_CROSS(false, true);
    else if (same) DQ_CROSS(true, false);
    else DQ_CROSS(false, false);
#undef DQ_CROSS
    return finish_cross(what, part, nblk, batch, out, s);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_excite_axpby_c64(const void* in, void* out, const double* coef, int mode, uint64_t xmask, uint64_t amask,
                                         uint64_t zmask, int negate, int n, const int* controls, int nc, int64_t batch,
                                         dq_stream_t stream) {
    return dq::axpby_impl<float>(in, out, coef, mode, xmask, amask, zmask, negate, n, controls, nc, batch, stream);
}
extern "C" int dq_apply_excite_axpby_c128(const void* in, void* out, const double* coef, int mode, uint64_t xmask, uint64_t amask,
                                          uint64_t zmask, int negate, int n, const int* controls, int nc, int64_t batch,
                                          dq_stream_t stream) {
    return dq::axpby_impl<double>(in, out, coef, mode, xmask, amask, zmask, negate, n, controls, nc, batch, stream);
}

extern "C" int64_t dq_excite_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross) {
    (void)cross;        // bra != ket reads twice as much and writes the same partial sums
    return dq::cross_ws_bytes_or_refuse(n, batch, is_c128 != 0);
}

extern "C" int dq_excite_cross_c64(const void* bra, const void* ket, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate, int n,
                                   const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                   dq_stream_t stream) {
    return dq::cross_impl<float>(bra, ket, xmask, amask, zmask, negate, n, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_excite_cross_c128(const void* bra, const void* ket, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate, int n,
                                    const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                    dq_stream_t stream) {
    return dq::cross_impl<double>(bra, ket, xmask, amask, zmask, negate, n, controls, nc, batch, out, ws, ws_bytes, stream);
}
