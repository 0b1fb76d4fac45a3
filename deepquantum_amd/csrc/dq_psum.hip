// Sums of Pauli strings, H = sum_t h_t P_t with real h_t: a a-plus-c-H combination and a cross reduction, the whole
// Hamiltonian in ONE launch each.
//
//     dq_apply_psum_axpby : out[b, i] = a[b] in[b, i] + c[b] (H in_b)[i]            (out of place only)
//     dq_psum_cross       : out[b] = sum_i conj(bra[b, i]) (H ket_b)[i]
//     dq_pauli_sum_cheb_step : next[b, i] = alpha[b] (H cur_b)[i] + beta[b] cur[b, i] + gamma[b] prev[b, i],
//                              acc[b, i] += delta[b] next[b, i]                     (next may be prev)
//     dq_pauli_sum_lanczos_step : next as in the Chebyshev step (no acc),  out[b] = (Re <cur_b, next_b>, |next_b|^2)
//     dq_lanczos_update      : w[b, i] += e[b] v[b, i],  acc[b, i] += d[b] v[b, i],  out[b] = (|w_b|^2, Re <v_b, w_b>)
// The third is one order of the Chebyshev expansion of exp(-i t H) (backend.apply_psum_evolve), the last two are the two
// launches of a Lanczos step (backend.psum_lanczos).
//
// What is written once.  The walk over the groups that applies H is one function, gather_h, templated on the
// accumulator's complex type; psum_axpby_kernel, psum_cross_kernel (in double) and psum_lanczos_step_kernel call it.  The
// third and the fourth entry point are the same three-term recurrence -- the gather over `cur`, the other two vectors read
// and written at the lane's own vectors -- with a running sum, or with the two sums the host needs reduced in the same
// launch.  They are two kernels all the same, and psum_cheb_step_kernel keeps a gather loop of its own: the shared forms
// measured slower (see there).  The fifth is a plain stream with the same two sums.  On the host the two steps are one
// function, step_impl.
//
// The terms are grouped by flip mask.  For the group with mask x
//     (G_x psi)[i] = w_x(i ^ x) psi[i ^ x],      w_x(j) = sum_{t in group} h_t i^{ny_t} (-1)^popc(j & z_t)
// and every i^{ny_t} is real or imaginary, so w_x(j) = wr(j) + i wi(j) with two real signed sums.  The table (device
// memory, built once per Hamiltonian by the caller) holds, for G groups and T terms,
//     xmasks[G]; bounds[2G + 1]: the start of group g's real-weight terms, bounds[2g], of its imaginary-weight terms,
//     bounds[2g + 1], and their end, bounds[2g + 2]; zmasks[T]; weights[T], the sign of i^{ny_t} folded in.
//
// Geometry.  That of dq_stream.hpp, in GATHER form: the item is an OUTPUT vector, never a pair.  For its ST_UNROLL output
// vectors a lane walks the groups: it loads the partner vectors v ^ (x >> VB) (four loads in flight), swaps the elements
// of a complex64 vector when bit 0 of x is set, sums wr and wi at the source index of each amplitude over the group's
// terms, multiplies once per group and amplitude, and accumulates.  Nobody reads what another lane writes only because
// in and out are disjoint.  The traffic is G + 1 reads of the state -- the group with no flip over vector indices reuses
// the own vector -- and one write.
//
// The group and term loops are uniform over the workgroup: the table comes in through scalar loads.  A z mask is split
// at the unit size: the part at or above it meets the unit's index, which is uniform -- a scalar parity folded into the
// weight's sign -- and only the low 10 (complex128) or 11 (complex64) bits cost vector instructions, five per term and
// amplitude (and, bit count, shift into the sign bit, xor, add).
//
// Safety.  Every x is masked with 2^n - 1 and every bound clamped to [0, T] in the kernel (scalar, once per group):
// whatever the table holds, no load leaves the sample or the table.  A lane whose vector lies beyond a small sample
// loads vector 0's partners and stores nothing.
//
// Reduction.  The sums over the terms are formed in the state's precision, the products and the sum over groups and
// amplitudes in double; the rest is dq_stream.hpp's fixed-order scheme.
#include "dq_stream.hpp"

namespace dq {

namespace {

struct PsumTable {
    const uint64_t* __restrict__ xmasks;
    const int* __restrict__ bounds;
    const uint64_t* __restrict__ zmasks;
    const double* __restrict__ weights;
    int ngroups, nterms;
};

// w[u][e] = sum over the terms [t0, t1) of weights[t] (-1)^popc(j & zmasks[t]) for the source indices j = (jhigh, jlow[u][e])
template <typename T, int VEC>
__device__ __forceinline__ void signed_sum(const PsumTable& tb, int t0, int t1, int sbits, uint64_t jhigh,
                                           const unsigned (&jlow)[ST_UNROLL][VEC], T (&w)[ST_UNROLL][VEC]) {
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) w[u][e] = (T)0;
    for (int t = t0; t < t1; ++t) {
        const uint64_t z = tb.zmasks[t];
        const unsigned zlow = (unsigned)z & ((1u << sbits) - 1u);
        const T h = (T)flip_sign(tb.weights[t], (unsigned)__popcll(jhigh & (z >> sbits)));      // (uniform)
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) w[u][e] += flip_sign(h, (unsigned)__popc(jlow[u][e] & zlow));
    }
}

// What a lane holds of group g: the partner vectors q and the weights wr + i wi at the source index of each amplitude.
// OWN: `own` holds the lane's own vectors of the same state (else those of another state, which nothing here reads).
template <typename T, int VEC, bool OWN, typename Q>
__device__ __forceinline__ void load_group(const PsumTable& tb, int g, int n, const Q* __restrict__ src, uint64_t unit,
                                           const uint64_t (&vec)[ST_UNROLL], const Q (&own)[ST_UNROLL], Q (&q)[ST_UNROLL], int& x0,
                                           T (&wr)[ST_UNROLL][VEC], T (&wi)[ST_UNROLL][VEC]) {
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int sbits = ST_UNIT_BITS + VB;
    const uint64_t x = tb.xmasks[g] & ((1ull << n) - 1ull);
    const uint64_t vx = x >> VB;
    x0 = (int)(x & (uint64_t)VB);
    if (OWN && vx == 0) {
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) q[u] = own[u];
    } else {
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) q[u] = src[vec[u] ^ vx];
    }
    unsigned jlow[ST_UNROLL][VEC];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            jlow[u][e] = ((((unsigned)(u * ST_THREADS) + threadIdx.x) << VB | (unsigned)e) ^ (unsigned)x) & ((1u << sbits) - 1u);
    const uint64_t jhigh = unit ^ (x >> sbits);
    const int t0 = min(max(tb.bounds[2 * g], 0), tb.nterms), t1 = min(max(tb.bounds[2 * g + 1], 0), tb.nterms),
              t2 = min(max(tb.bounds[2 * g + 2], 0), tb.nterms);
    signed_sum<T, VEC>(tb, t0, t1, sbits, jhigh, jlow, wr);
    signed_sum<T, VEC>(tb, t1, t2, sbits, jhigh, jlow, wi);
}

// The lane's vectors of unit `unit`; one that lies beyond the sample is replaced by vector 0 and marked in `live`.
__device__ __forceinline__ unsigned unit_vectors(uint64_t unit, uint64_t nvec, uint64_t (&vec)[ST_UNROLL]) {
    unsigned live = 0;
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const uint64_t v = (unit << ST_UNIT_BITS) + (uint64_t)(u * ST_THREADS) + threadIdx.x;
        if (v < nvec) live |= 1u << u;
        vec[u] = v < nvec ? v : 0;
    }
    return live;
}

// A complex number in the accumulator's type A: itself, or (the cross reduction over a complex64 state) widened to double
template <typename A, typename C>
__device__ __forceinline__ A widen(C c) {
    A r;
    r.x = c.x;
    r.y = c.y;
    return r;
}

// THE gather: h[u][e] = (H src) at the lane's amplitudes of unit `unit`, summed over the groups in their order with one cfma
// per group and amplitude, in A = cx<T>, or in double2 with both factors widened first.  OWN, `own`: as load_group has them.
template <typename T, int VEC, bool OWN, typename Q, typename A>
__device__ __forceinline__ void gather_h(const PsumTable& tb, int n, const Q* __restrict__ src, uint64_t unit,
                                         const uint64_t (&vec)[ST_UNROLL], const Q (&own)[ST_UNROLL], A (&h)[ST_UNROLL][VEC]) {
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) h[u][e] = widen<A>(mk<T>((T)0, (T)0));
    // The own vectors as VALUES, read before the loop.  This function is optimised on its own before it is inlined, and q
    // is a local of it: with `own` read inside load_group's branch the compiler merges "q = own[u]" and "q = src[..]" into
    // one load through a selected pointer -- a flat load, and the caller's own vectors in scratch memory (80 bytes a lane;
    // profiles/psum_core/resource_usage.txt has both forms).
    Q mine[ST_UNROLL];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) mine[u] = own[u];
    for (int g = 0; g < tb.ngroups; ++g) {
        Q q[ST_UNROLL];
        T wr[ST_UNROLL][VEC], wi[ST_UNROLL][VEC];
        int x0;
        load_group<T, VEC, OWN>(tb, g, n, src, unit, vec, mine, q, x0, wr, wi);
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                h[u][e] = cfma(widen<A>(mk<T>(wr[u][e], wi[u][e])), widen<A>(vec_get<T>(q[u], e ^ x0)), h[u][e]);
    }
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void psum_axpby_kernel(const cx<T>* __restrict__ in, cx<T>* __restrict__ out,
                                                                const double* __restrict__ coef, PsumTable tb, int n,
                                                                uint64_t nvec) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    const cx<T> a = mk<T>((T)coef[4 * b], (T)coef[4 * b + 1]), c = mk<T>((T)coef[4 * b + 2], (T)coef[4 * b + 3]);
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < nvec; unit += gridDim.x) {
        uint64_t vec[ST_UNROLL];
        const unsigned live = unit_vectors(unit, nvec, vec);
        Q own[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) own[u] = src[vec[u]];
        cx<T> h[ST_UNROLL][VEC];
        gather_h<T, VEC, true>(tb, n, src, unit, vec, own, h);
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            Q r;
#pragma unroll
            for (int e = 0; e < VEC; ++e) vec_set(r, e, cfma(c, h[u][e], cmul(a, vec_get<T>(own[u], e))));
            if (live >> u & 1u) dst[vec[u]] = r;
        }
    }
}

// One order of a Chebyshev recurrence in H and its running sum:
//     next = alpha (H cur) + beta cur + gamma prev,      acc += delta next
// The gather is psum_axpby_kernel's, over `cur` alone; prev, next and acc are touched at the lane's own vectors only, so
// next may be prev (each lane has read its vectors of prev before it writes them).  The own vectors of prev and acc are
// loaded AFTER the group loop: held across it they would be 32 more live registers (see profiles/evolve/resource_usage.txt).
// SAME: next is prev, and prev is then read through `next` -- so that every pointer of either instantiation is __restrict__
// in earnest.  Without that the compiler cannot tell the stores from the table and reads the table with vector loads in
// the term loop instead of scalar ones: measured 1.4 to 1.9 times one psum_axpby launch where this form is at 0.97 to 1.20.
// coef = [batch][5] doubles (alpha, beta, gamma, Re delta, Im delta), rounded once to the state's real precision.
// This kernel keeps its OWN copy of gather_h's loop and of the recurrence that psum_lanczos_step_kernel has, on purpose.
// Written as one kernel with the Lanczos step on gather_h, the tail chosen at compile time, it had the same registers and
// the same term loop, and its complex128 SAME instantiation measured 0.6 to 1.6 per cent slower in every run where the
// term loop bounds the time; on gather_h alone it compiles to that same code (profiles/psum_core/README.md, ab.txt).
// Keep the two in step by hand.
template <typename T, bool SAME>
__global__ __launch_bounds__(ST_THREADS) void psum_cheb_step_kernel(const cx<T>* __restrict__ cur, const cx<T>* __restrict__ prev,
                                                                    cx<T>* __restrict__ next, cx<T>* __restrict__ acc,
                                                                    const double* __restrict__ coef, PsumTable tb, int n,
                                                                    uint64_t nvec) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(cur + (b << n));
    Q* pnext = reinterpret_cast<Q*>(next + (b << n));
    const Q* pprev = SAME ? pnext : reinterpret_cast<const Q*>(prev + (b << n));
    Q* pacc = reinterpret_cast<Q*>(acc + (b << n));
    const T alpha = (T)coef[5 * b], beta = (T)coef[5 * b + 1], gamma = (T)coef[5 * b + 2];
    const cx<T> delta = mk<T>((T)coef[5 * b + 3], (T)coef[5 * b + 4]);
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < nvec; unit += gridDim.x) {
        uint64_t vec[ST_UNROLL];
        const unsigned live = unit_vectors(unit, nvec, vec);
        Q own[ST_UNROLL];
        cx<T> h[ST_UNROLL][VEC];                        // (H cur) at the lane's amplitudes
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            own[u] = src[vec[u]];
#pragma unroll
            for (int e = 0; e < VEC; ++e) h[u][e] = mk<T>((T)0, (T)0);
        }
        for (int g = 0; g < tb.ngroups; ++g) {
            Q q[ST_UNROLL];
            T wr[ST_UNROLL][VEC], wi[ST_UNROLL][VEC];
            int x0;
            load_group<T, VEC, true>(tb, g, n, src, unit, vec, own, q, x0, wr, wi);
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) h[u][e] = cfma(mk<T>(wr[u][e], wi[u][e]), vec_get<T>(q[u], e ^ x0), h[u][e]);
        }
        Q p[ST_UNROLL], s[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {           // (a lane beyond a small sample reads vector 0 and stores nothing)
            p[u] = pprev[vec[u]];
            s[u] = pacc[vec[u]];
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            Q r, t;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const cx<T> o = vec_get<T>(own[u], e), pv = vec_get<T>(p[u], e);
                const cx<T> y = mk<T>(fma(gamma, pv.x, fma(beta, o.x, alpha * h[u][e].x)),
                                      fma(gamma, pv.y, fma(beta, o.y, alpha * h[u][e].y)));
                vec_set(r, e, y);
                vec_set(t, e, cfma(delta, y, vec_get<T>(s[u], e)));
            }
            if (live >> u & 1u) {
                pnext[vec[u]] = r;
                pacc[vec[u]] = t;
            }
        }
    }
}

// One half of a Lanczos step in H, with the two sums the host needs of it:
//     next = alpha (H cur) + beta cur + gamma prev,      ws[b, blockIdx.x] = this workgroup's part of
//     ( sum_i Re conj(cur_i) next_i ,  sum_i |next_i|^2 )
// psum_cheb_step_kernel without its running sum: the same gather over `cur` (gather_h), prev loaded after the group loop, the same
// SAME split (every pointer __restrict__ in earnest, see above).  The sums are taken over `next` AS STORED -- after the
// rounding to the state's precision -- with products and sums in double, so the host's record describes the vectors that
// exist.  A lane beyond a small sample stores nothing and adds nothing (`live`).
// coef = [batch][3] doubles (alpha, beta, gamma), rounded once to the state's real precision.
template <typename T, bool SAME>
__global__ __launch_bounds__(ST_THREADS) void psum_lanczos_step_kernel(const cx<T>* __restrict__ cur, const cx<T>* __restrict__ prev,
                                                                       cx<T>* __restrict__ next, const double* __restrict__ coef,
                                                                       PsumTable tb, int n, uint64_t nvec, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(cur + (b << n));
    Q* pnext = reinterpret_cast<Q*>(next + (b << n));
    const Q* pprev = SAME ? pnext : reinterpret_cast<const Q*>(prev + (b << n));
    const T alpha = (T)coef[3 * b], beta = (T)coef[3 * b + 1], gamma = (T)coef[3 * b + 2];
    double dot = 0.0, nrm = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < nvec; unit += gridDim.x) {
        uint64_t vec[ST_UNROLL];
        const unsigned live = unit_vectors(unit, nvec, vec);
        Q own[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) own[u] = src[vec[u]];
        cx<T> h[ST_UNROLL][VEC];                        // (H cur) at the lane's amplitudes
        gather_h<T, VEC, true>(tb, n, src, unit, vec, own, h);
        Q p[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) p[u] = pprev[vec[u]];      // (a lane beyond a small sample reads vector 0)
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            Q r;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const cx<T> o = vec_get<T>(own[u], e), pv = vec_get<T>(p[u], e);
                const cx<T> y = mk<T>(fma(gamma, pv.x, fma(beta, o.x, alpha * h[u][e].x)),
                                      fma(gamma, pv.y, fma(beta, o.y, alpha * h[u][e].y)));
                vec_set(r, e, y);
                if (live >> u & 1u) {
                    const double yr = (double)y.x, yi = (double)y.y;
                    dot = fma((double)o.x, yr, fma((double)o.y, yi, dot));
                    nrm = fma(yr, yr, fma(yi, yi, nrm));
                }
            }
            if (live >> u & 1u) pnext[vec[u]] = r;
        }
    }
    write_partial(dot, nrm, sh, ws);
}

// The other half of a Lanczos step, a pure stream over the lane's own vectors (no gather):
//     w += e v  (in place),      acc += d v  (HAS_ACC),      ws[b, blockIdx.x] = this workgroup's part of
//     ( sum_i |w_i|^2 ,  sum_i Re conj(v_i) w_i )     over the updated w as stored
// coef = [batch][2] doubles (e, d), real, rounded once to the state's real precision.  v, w and acc pairwise disjoint.
template <typename T, bool HAS_ACC>
__global__ __launch_bounds__(ST_THREADS) void lanczos_update_kernel(const cx<T>* __restrict__ v, cx<T>* __restrict__ w,
                                                                    cx<T>* __restrict__ acc, const double* __restrict__ coef,
                                                                    int n, uint64_t nvec, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* pv = reinterpret_cast<const Q*>(v + (b << n));
    Q* pw = reinterpret_cast<Q*>(w + (b << n));
    Q* pa = HAS_ACC ? reinterpret_cast<Q*>(acc + (b << n)) : nullptr;
    const T ce = (T)coef[2 * b], cd = (T)coef[2 * b + 1];
    double nrm = 0.0, dot = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < nvec; unit += gridDim.x) {
        uint64_t vec[ST_UNROLL];
        const unsigned live = unit_vectors(unit, nvec, vec);
        Q qv[ST_UNROLL], qw[ST_UNROLL], qa[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            qv[u] = pv[vec[u]];
            qw[u] = pw[vec[u]];
            if (HAS_ACC) qa[u] = pa[vec[u]];
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            Q r, s;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const cx<T> x = vec_get<T>(qv[u], e), y0 = vec_get<T>(qw[u], e);
                const cx<T> y = mk<T>(fma(ce, x.x, y0.x), fma(ce, x.y, y0.y));
                vec_set(r, e, y);
                if (HAS_ACC) {
                    const cx<T> a0 = vec_get<T>(qa[u], e);
                    vec_set(s, e, mk<T>(fma(cd, x.x, a0.x), fma(cd, x.y, a0.y)));
                }
                if (live >> u & 1u) {
                    const double yr = (double)y.x, yi = (double)y.y;
                    nrm = fma(yr, yr, fma(yi, yi, nrm));
                    dot = fma((double)x.x, yr, fma((double)x.y, yi, dot));
                }
            }
            if (live >> u & 1u) {
                pw[vec[u]] = r;
                if (HAS_ACC) pa[vec[u]] = s;
            }
        }
    }
    write_partial(nrm, dot, sh, ws);
}

// ws[b, blockIdx.x] = this workgroup's part of sum_i conj(bra_i) (H ket)_i
template <typename T, bool SAME>
__global__ __launch_bounds__(ST_THREADS) void psum_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                PsumTable tb, int n, uint64_t nvec, double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    double re = 0.0, im = 0.0;
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < nvec; unit += gridDim.x) {
        uint64_t vec[ST_UNROLL];
        const unsigned live = unit_vectors(unit, nvec, vec);
        Q own[ST_UNROLL];                               // the bra's vectors: with SAME the ket's own as well
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) own[u] = pb[vec[u]];
        double2 hk[ST_UNROLL][VEC];                     // (H ket) at the lane's amplitudes, in double
        gather_h<T, VEC, SAME>(tb, n, pk, unit, vec, own, hk);
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (live >> u & 1u) {
                    const cx<T> o = vec_get<T>(own[u], e);
                    const double ar = (double)o.x, ai = (double)o.y;
                    re = fma(ar, hk[u][e].x, fma(ai, hk[u][e].y, re));
                    im = fma(ar, hk[u][e].y, fma(-ai, hk[u][e].x, im));
                }
            }
    }
    write_partial(re, im, sh, ws);
}

// The four arrays of the table: non-null, aligned to their element, at least one group and one term
int check_table(const char* what, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks, const double* weights,
                int ngroups, int nterms, PsumTable* tb) {
    if (!xmasks || !bounds || !zmasks || !weights) {
        set_error("%s: null table pointer", what);
        return DQ_ERR_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(xmasks) & 7) || (reinterpret_cast<uintptr_t>(zmasks) & 7) ||
        (reinterpret_cast<uintptr_t>(weights) & 7) || (reinterpret_cast<uintptr_t>(bounds) & 3)) {
        set_error("%s: xmasks, zmasks and weights must be 8-byte aligned, bounds 4-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (ngroups < 1) {
        set_error("%s: ngroups=%d, at least one group is needed", what, ngroups);
        return DQ_ERR_ARG;
    }
    if (nterms < 1) {
        set_error("%s: nterms=%d, at least one term is needed", what, nterms);
        return DQ_ERR_ARG;
    }
    *tb = PsumTable{xmasks, bounds, zmasks, weights, ngroups, nterms};
    return DQ_OK;
}

template <typename T>
int axpby_impl(const void* in, void* out, const double* coef, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks,
               const double* weights, int ngroups, int nterms, int n, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_psum_axpby";
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), DISJOINT)) return rc;
    if (int rc = check_coef(what, coef)) return rc;
    PsumTable tb;
    if (int rc = check_table(what, xmasks, bounds, zmasks, weights, ngroups, nterms, &tb)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    hipLaunchKernelGGL((psum_axpby_kernel<T>), dim3(blocks_of(nvec), (unsigned)batch), dim3(ST_THREADS), 0, as_stream(stream),
                       static_cast<const cx<T>*>(in), static_cast<cx<T>*>(out), coef, tb, n, nvec);
    return check_launch(what);
}

// The Chebyshev step (SUMS false: out and ws unused) and the Lanczos step (SUMS true: no acc, which is null).  cur is only
// read and is gathered from: apart from everything that is written.  acc is read and written at own vectors only but must
// be nobody else's; next may be prev, since each lane reads its vectors of prev before it writes them.
template <typename T, bool SUMS>
int step_impl(const char* what, const void* cur, const void* prev, void* next, void* acc, const double* coef,
              const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
              int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    enum { CUR, PREV, NEXT, ACC };
    const StateBuf bufs[] = {{"cur", cur}, {"prev", prev}, {"next", next}, {"acc", acc}};
    const ApartRule with_acc[] = {{CUR, NEXT, DISJOINT}, {ACC, CUR, DISJOINT}, {ACC, PREV, DISJOINT}, {ACC, NEXT, DISJOINT},
                                  {NEXT, PREV, SAME_OR_DISJOINT}};
    const ApartRule without[] = {{CUR, NEXT, DISJOINT}, {NEXT, PREV, SAME_OR_DISJOINT}};        // (the first three buffers only)
    if (int rc = check_buffers(what, bufs, SUMS ? 3 : 4, SUMS ? without : with_acc, SUMS ? 2 : 5, 1, n, batch, sizeof(cx<T>)))
        return rc;
    if (int rc = check_coef(what, coef)) return rc;
    PsumTable tb;
    if (int rc = check_table(what, xmasks, bounds, zmasks, weights, ngroups, nterms, &tb)) return rc;
    if (SUMS) {
        if (int rc = check_out_ws(what, out, ws)) return rc;
        if (int rc = check_cross_ws(what, ws_bytes, n, batch, C128, "dq_psum_cross_ws_bytes")) return rc;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = blocks_of(nvec);
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pc = static_cast<const cx<T>*>(cur);
    cx<T>* pn = static_cast<cx<T>*>(next);
    const cx<T>* pp = prev == next ? nullptr : static_cast<const cx<T>*>(prev);     // (SAME: prev is read through next)
    hipStream_t s = as_stream(stream);
    if constexpr (SUMS) {
        double* part = static_cast<double*>(ws);
        if (prev == next) hipLaunchKernelGGL((psum_lanczos_step_kernel<T, true>), grid, dim3(ST_THREADS), 0, s, pc, pp, pn, coef, tb, n, nvec, part);
        else hipLaunchKernelGGL((psum_lanczos_step_kernel<T, false>), grid, dim3(ST_THREADS), 0, s, pc, pp, pn, coef, tb, n, nvec, part);
        return finish_cross(what, part, nblk, batch, out, s);
    } else {
        cx<T>* pa = static_cast<cx<T>*>(acc);
        if (prev == next) hipLaunchKernelGGL((psum_cheb_step_kernel<T, true>), grid, dim3(ST_THREADS), 0, s, pc, pp, pn, pa, coef, tb, n, nvec);
        else hipLaunchKernelGGL((psum_cheb_step_kernel<T, false>), grid, dim3(ST_THREADS), 0, s, pc, pp, pn, pa, coef, tb, n, nvec);
        return check_launch(what);
    }
}

// v is only read, w and acc are read and written at each lane's own vectors: the three pairwise disjoint; acc may be null.
template <typename T>
int lanczos_update_impl(const void* v, void* w, void* acc, const double* coef, int n, int64_t batch, double* out, void* ws,
                        int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_lanczos_update";
    enum { V, W, ACC };
    const StateBuf bufs[] = {{"v", v}, {"w", w}, {"acc", acc, true}};
    const ApartRule rules[] = {{V, W, DISJOINT}, {ACC, V, DISJOINT}, {ACC, W, DISJOINT}};
    if (int rc = check_buffers(what, bufs, 3, rules, 3, 1, n, batch, sizeof(cx<T>))) return rc;
    if (int rc = check_coef(what, coef)) return rc;
    if (int rc = check_out_ws(what, out, ws)) return rc;
    if (int rc = check_cross_ws(what, ws_bytes, n, batch, C128, "dq_psum_cross_ws_bytes")) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = blocks_of(nvec);
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pv = static_cast<const cx<T>*>(v);
    cx<T>* pw = static_cast<cx<T>*>(w);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    if (acc) hipLaunchKernelGGL((lanczos_update_kernel<T, true>), grid, dim3(ST_THREADS), 0, s, pv, pw, static_cast<cx<T>*>(acc), coef, n, nvec, part);
    else hipLaunchKernelGGL((lanczos_update_kernel<T, false>), grid, dim3(ST_THREADS), 0, s, pv, pw, static_cast<cx<T>*>(nullptr), coef, n, nvec, part);
    return finish_cross(what, part, nblk, batch, out, s);
}

template <typename T>
int cross_impl(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks,
               const double* weights, int ngroups, int nterms, int n, int64_t batch, double* out, void* ws, int64_t ws_bytes,
               dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_psum_cross";
    if (n < 1 || n > 40) {
        set_error("%s: n=%d out of range [1, 40]", what, n);
        return DQ_ERR_ARG;
    }
    if (int rc = check_batch(what, batch)) return rc;
    PsumTable tb;
    if (int rc = check_table(what, xmasks, bounds, zmasks, weights, ngroups, nterms, &tb)) return rc;
    if (int rc = check_cross(what, bra, ket, nullptr, false, out, ws, ws_bytes, n, batch, C128)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = blocks_of(nvec);
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    if (bra == ket) hipLaunchKernelGGL((psum_cross_kernel<T, true>), grid, dim3(ST_THREADS), 0, s, pb, pk, tb, n, nvec, part);
    else hipLaunchKernelGGL((psum_cross_kernel<T, false>), grid, dim3(ST_THREADS), 0, s, pb, pk, tb, n, nvec, part);
    return finish_cross(what, part, nblk, batch, out, s);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_psum_axpby_c64(const void* in, void* out, const double* coef, const uint64_t* xmasks, const int* bounds,
                                       const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
                                       int64_t batch, dq_stream_t stream) {
    return dq::axpby_impl<float>(in, out, coef, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, stream);
}
extern "C" int dq_apply_psum_axpby_c128(const void* in, void* out, const double* coef, const uint64_t* xmasks, const int* bounds,
                                        const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
                                        int64_t batch, dq_stream_t stream) {
    return dq::axpby_impl<double>(in, out, coef, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, stream);
}

extern "C" int dq_pauli_sum_cheb_step_c64(const void* cur, const void* prev, void* next, void* acc, const double* coef,
                                     const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks, const double* weights,
                                     int ngroups, int nterms, int n, int64_t batch, dq_stream_t stream) {
    return dq::step_impl<float, false>("dq_pauli_sum_cheb_step", cur, prev, next, acc, coef, xmasks, bounds, zmasks, weights, ngroups, nterms, n,
                                       batch, nullptr, nullptr, 0, stream);
}
extern "C" int dq_pauli_sum_cheb_step_c128(const void* cur, const void* prev, void* next, void* acc, const double* coef,
                                      const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks, const double* weights,
                                      int ngroups, int nterms, int n, int64_t batch, dq_stream_t stream) {
    return dq::step_impl<double, false>("dq_pauli_sum_cheb_step", cur, prev, next, acc, coef, xmasks, bounds, zmasks, weights, ngroups, nterms, n,
                                       batch, nullptr, nullptr, 0, stream);
}

extern "C" int dq_pauli_sum_lanczos_step_c64(const void* cur, const void* prev, void* next, const double* coef, const uint64_t* xmasks,
                                             const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms,
                                             int n, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::step_impl<float, true>("dq_pauli_sum_lanczos_step", cur, prev, next, nullptr, coef, xmasks, bounds, zmasks, weights, ngroups,
                                      nterms, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_pauli_sum_lanczos_step_c128(const void* cur, const void* prev, void* next, const double* coef, const uint64_t* xmasks,
                                              const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms,
                                              int n, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::step_impl<double, true>("dq_pauli_sum_lanczos_step", cur, prev, next, nullptr, coef, xmasks, bounds, zmasks, weights, ngroups,
                                      nterms, n, batch, out, ws, ws_bytes, stream);
}

extern "C" int dq_lanczos_update_c64(const void* v, void* w, void* acc, const double* coef, int n, int64_t batch, double* out,
                                     void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::lanczos_update_impl<float>(v, w, acc, coef, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_lanczos_update_c128(const void* v, void* w, void* acc, const double* coef, int n, int64_t batch, double* out,
                                      void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::lanczos_update_impl<double>(v, w, acc, coef, n, batch, out, ws, ws_bytes, stream);
}

extern "C" int64_t dq_psum_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross) {
    (void)cross;        // bra != ket reads one vector more per item and writes the same partial sums
    return dq::cross_ws_bytes_or_refuse(n, batch, is_c128 != 0);
}

extern "C" int dq_psum_cross_c64(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds,
                                 const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n, int64_t batch,
                                 double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::cross_impl<float>(bra, ket, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_psum_cross_c128(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds,
                                  const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n, int64_t batch,
                                  double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::cross_impl<double>(bra, ket, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, out, ws, ws_bytes, stream);
}
