// Quantum jumps on state vectors: a whole layer of one-wire monomial operators, every sample of a batch with its own,
// in one pass -- and the weight of such a layer in one read.
//
// A Kraus operator that is diagonal or anti-diagonal is K = i^m X^x diag(f0, f1) with f0, f1 real.  A tensor product of
// such operators over any set of wires is a generalized permutation:
//
//     dq_apply_jump            out[b, i ^ x] = i^m s prod_p F[b, p, bit_p(i)] in[b, i]
//     dq_apply_jump, transpose out[b, i]     = (-i)^m s prod_p F[b, p, bit_p(i)] in[b, i ^ x]        (the adjoint map)
//     dq_jump_cross            out[b]        = sum_i prod_p G[b, p, bit_p(i)] conj(bra[b, i]) ket[b, i]
//
// with F[b] = (n, 2) doubles indexed by the index-bit position p and the value of that bit, x = xmask[b], m = phase[b],
// s = scale[b], all read on the device: nothing of a sample's record is known to the host.
//
// One loop serves both maps of dq_apply_jump.  Seen from the output index q they are
//     out[q] = i^m' s prod_p F'[p, bit_p(q)] in[q ^ x]
// with F'[p, c] = F[p, c ^ bit_p(x)] and m' = m (the factors belong to the source index q ^ x), or F' = F and m' = -m
// (transposed): the workgroup applies the flip once, when it stages F[b] in LDS.
//
// Geometry.  That of dq_stream.hpp with an output vector as the item: units of 1024 vectors, the sample as grid y.
//
// The factor path.  No table is read from memory per amplitude.  An amplitude's index is (unit, u, lane, e): e the
// element within a complex64 vector (bit 0), lane the next eight bits, u the two unroll bits, unit the rest.
//   * (u, lane, e): the product over those index bits is formed once per lane before the loop, ST_UNROLL * VEC factors
//     kept in registers (eight for complex64, four for complex128);
//   * unit: uniform over the workgroup.  Its bits are cut into three groups of 8; the workgroup builds one product
//     table of 256 entries per group in LDS in its prologue (3 KiB in float, 6 KiB in double), and a unit's factor is
//     three LDS reads at a uniform address and two multiplications, made wave-uniform with readfirstlane.  24 unit bits
//     reach n = 34 (complex128) / 35 (complex64); n <= 34 is the limit of both.
// A unit whose uniform factor is exactly 0 -- the jump of an amplitude damping on a high wire whose bit is 0 there -- is
// zero-filled without a load (dq_apply_jump) or skipped (dq_jump_cross).  Zeros on low bits are per lane and still load.
// Traffic: one write and at most one read; one read (two with bra != ket) for the weight.
//
// Exactness.  The bits of x at or above the vector bit go into the load address (lines are permuted, never split); bit 0
// of a complex64 state swaps the halves of the loaded vector in registers.  i^m swaps re and im and flips signs bit for
// bit (flip_sign), it is never a complex multiplication.  An amplitude is multiplied once by a real number that is a
// product of at most n + 1 rounded factors: with every factor +-1 and s == 1 the pass is bit-exact.
//
// In place.  A lane reads vector v ^ (x >> VB) and writes vector v: in == out is safe only with x == 0.  The host cannot
// see x, so the caller says whether xmask may hold one (`may_flip`); with may_flip == 0 the kernel does not read xmask.
//
// Reduction.  dq_jump_cross builds its tables and accumulates in double; the rest is dq_stream.hpp's fixed-order scheme.
#include "dq_stream.hpp"

namespace dq {

namespace {

constexpr int JUMP_MAX_N = 34;
constexpr int JUMP_GROUPS = 3;                          // groups of 8 unit bits, one LDS table each
constexpr int JUMP_MAX_POS = ST_UNIT_BITS + 1 + 8 * JUMP_GROUPS;       // index-bit positions the factor path covers

__device__ __forceinline__ float uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ double uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// What a workgroup keeps of its sample's factors: the staged (flipped) F' and the product tables of the unit bits.
template <typename TT> struct JumpTables {
    TT f[JUMP_MAX_POS][2];
    TT tab[JUMP_GROUPS][256];
};

// Stages F'[p, c] = F[p, c ^ bit_p(fx)] (1 at positions >= n), builds the three tables and returns, in lu, the lane's own
// product over the bits below the unit size for each of its ST_UNROLL * VEC amplitudes.  Ends with a barrier.
template <typename TT, int VEC>
__device__ __forceinline__ void jump_prologue(const double* __restrict__ F, int n, uint64_t fx, JumpTables<TT>& t,
                                              TT (&lu)[ST_UNROLL][VEC]) {
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;
    if (threadIdx.x < 2 * JUMP_MAX_POS) {
        const int p = (int)threadIdx.x >> 1, c = (int)threadIdx.x & 1;
        t.f[p][c] = p < n ? (TT)F[2 * p + (c ^ (int)((fx >> p) & 1ull))] : (TT)1;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < JUMP_GROUPS; ++g) {
        TT prod = (TT)1;
#pragma unroll
        for (int j = 0; j < 8; ++j) prod *= t.f[SBITS + 8 * g + j][(threadIdx.x >> j) & 1u];
        t.tab[g][threadIdx.x] = prod;
    }
    TT lane = (TT)1;
#pragma unroll
    for (int j = 0; j < 8; ++j) lane *= t.f[VB + j][(threadIdx.x >> j) & 1u];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const TT lu0 = lane * (t.f[VB + 8][u & 1] * t.f[VB + 9][u >> 1]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) lu[u][e] = VB ? lu0 * t.f[0][e] : lu0;
    }
    __syncthreads();
}

// the factor of a unit: uniform over the workgroup
template <typename TT> __device__ __forceinline__ TT unit_factor(const JumpTables<TT>& t, uint64_t chunk) {
    return uniform(t.tab[0][chunk & 255u] * t.tab[1][(chunk >> 8) & 255u] * t.tab[2][(chunk >> 16) & 255u]);
}

// i^m (f a): re and im swapped for odd m, signs flipped bit for bit
template <typename T> __device__ __forceinline__ cx<T> turned(cx<T> a, T f, unsigned m) {
    const T re = f * a.x, im = f * a.y;
    const unsigned sr = ((m + 1u) >> 1) & 1u, si = (m >> 1) & 1u;
    return (m & 1u) ? mk<T>(flip_sign(im, sr), flip_sign(re, si)) : mk<T>(flip_sign(re, sr), flip_sign(im, si));
}

// in and out may be the same buffer (may_flip == 0): no __restrict__ on them
template <typename T>
__global__ __launch_bounds__(ST_THREADS) void jump_apply_kernel(const cx<T>* in, cx<T>* out, const double* __restrict__ F,
                                                                const int64_t* __restrict__ xmask,
                                                                const int64_t* __restrict__ phase,
                                                                const double* __restrict__ scale, int n, int transpose,
                                                                int may_flip, uint64_t nchunks) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    __shared__ JumpTables<T> t;
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    // the sample's record, uniform over the workgroup; whatever it holds is cut to what there is
    const uint64_t x = may_flip ? (uint64_t)xmask[b] & ((1ull << n) - 1ull) : 0ull;
    const unsigned m = (unsigned)(transpose ? -phase[b] : phase[b]) & 3u;
    const T s = (T)scale[b];
    T lu[ST_UNROLL][VEC];
    jump_prologue<T, VEC>(F + b * (uint64_t)(2 * n), n, transpose ? 0ull : x, t, lu);
    const uint64_t xv = x >> VB;                        // the part of x in the load address
    const int swap = VB ? (int)(x & 1ull) : 0;

    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        const T g = unit_factor(t, chunk);
        if (g == (T)0) {                                // nothing of the unit survives: no load
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
                if (v < nvec) dst[v] = Q{};
            }
            continue;
        }
        const T gs = g * s;
        Q q[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) q[u] = src[v ^ xv];
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                Q r;
#pragma unroll
                for (int e = 0; e < VEC; ++e) vec_set(r, e, turned<T>(vec_get<T>(q[u], e ^ swap), gs * lu[u][e], m));
                dst[v] = r;
            }
        }
    }
}

// ws[b, blockIdx.x] = this workgroup's part of sum_i prod_p G[p, bit_p(i)] conj(bra_i) ket_i
template <typename T, bool SAME>
__global__ __launch_bounds__(ST_THREADS) void jump_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                const double* __restrict__ G, int n, uint64_t nchunks,
                                                                double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    __shared__ JumpTables<double> t;
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    double lu[ST_UNROLL][VEC];
    jump_prologue<double, VEC>(G + b * (uint64_t)(2 * n), n, 0ull, t, lu);
    double re = 0.0, im = 0.0;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const double g = unit_factor(t, chunk);
        if (g == 0.0) continue;                         // (uniform over the workgroup)
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        Q qk[ST_UNROLL], qb[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                qk[u] = pk[v];
                if (!SAME) qb[u] = pb[v];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const cx<T> k = vec_get<T>(qk[u], e);
                    const double kr = (double)k.x, ki = (double)k.y, w = g * lu[u][e];
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
    write_partial(re, im, sh, ws);
}

// ---- host side -----------------------------------------------------------------------------------
int check_jump_n(const char* what, int n) {
    if (n >= 1 && n <= JUMP_MAX_N) return DQ_OK;
    set_error("%s: n=%d out of range [1, %d] (three product tables of 8 bits above a unit)", what, n, JUMP_MAX_N);
    return DQ_ERR_ARG;
}

template <typename T>
int jump_apply_impl(const void* in, void* out, const double* factors, const int64_t* xmask, const int64_t* phase,
                    const double* scale, int n, int transpose, int may_flip, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_jump";
    // in place only where the caller promises x == 0: a lane then owns the vector it reads and writes
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), may_flip ? DISJOINT : SAME_OR_DISJOINT)) return rc;
    if (int rc = check_jump_n(what, n)) return rc;
    if (!factors || !phase || !scale || (may_flip && !xmask)) {
        set_error("%s: null pointer (factors, phase, scale, or xmask with may_flip)", what);
        return DQ_ERR_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(factors) | reinterpret_cast<uintptr_t>(xmask) | reinterpret_cast<uintptr_t>(phase) |
         reinterpret_cast<uintptr_t>(scale)) & 7) {
        set_error("%s: factors, xmask, phase and scale must be 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const dim3 grid(blocks_of(nvec), (unsigned)batch);
    hipLaunchKernelGGL((jump_apply_kernel<T>), grid, dim3(ST_THREADS), 0, as_stream(stream), static_cast<const cx<T>*>(in),
                       static_cast<cx<T>*>(out), factors, xmask, phase, scale, n, transpose ? 1 : 0, may_flip ? 1 : 0, units_of(nvec));
    return check_launch(what);
}

template <typename T>
int jump_cross_impl(const void* bra, const void* ket, const double* weights, int n, int64_t batch, double* out, void* ws,
                    int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_jump_cross";
    if (int rc = check_cross_buffers(what, bra, ket, nullptr, false, out, ws)) return rc;
    if (int rc = check_jump_n(what, n)) return rc;
    if (int rc = check_batch(what, batch)) return rc;
    if (!weights || (reinterpret_cast<uintptr_t>(weights) & 7)) {
        set_error("%s: weights must be non-null and 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (int rc = check_cross_ws(what, ws_bytes, n, batch, C128)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = blocks_of(nvec);
    const dim3 grid(nblk, (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    if (bra == ket)
        hipLaunchKernelGGL((jump_cross_kernel<T, true>), grid, dim3(ST_THREADS), 0, s, pb, pk, weights, n, units_of(nvec), part);
    else
        hipLaunchKernelGGL((jump_cross_kernel<T, false>), grid, dim3(ST_THREADS), 0, s, pb, pk, weights, n, units_of(nvec), part);
    return finish_cross(what, part, nblk, batch, out, s);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_jump_c64(const void* in, void* out, const double* factors, const int64_t* xmask, const int64_t* phase,
                                 const double* scale, int n, int transpose, int may_flip, int64_t batch, dq_stream_t stream) {
    return dq::jump_apply_impl<float>(in, out, factors, xmask, phase, scale, n, transpose, may_flip, batch, stream);
}
extern "C" int dq_apply_jump_c128(const void* in, void* out, const double* factors, const int64_t* xmask, const int64_t* phase,
                                  const double* scale, int n, int transpose, int may_flip, int64_t batch, dq_stream_t stream) {
    return dq::jump_apply_impl<double>(in, out, factors, xmask, phase, scale, n, transpose, may_flip, batch, stream);
}

extern "C" int64_t dq_jump_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross) {
    (void)cross;        // bra != ket reads twice as much and writes the same partial sums
    if (n > dq::JUMP_MAX_N) return -1;
    return dq::cross_ws_bytes_or_refuse(n, batch, is_c128 != 0);
}

extern "C" int dq_jump_cross_c64(const void* bra, const void* ket, const double* weights, int n, int64_t batch, double* out,
                                 void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::jump_cross_impl<float>(bra, ket, weights, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_jump_cross_c128(const void* bra, const void* ket, const double* weights, int n, int64_t batch, double* out,
                                  void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::jump_cross_impl<double>(bra, ket, weights, n, batch, out, ws, ws_bytes, stream);
}
