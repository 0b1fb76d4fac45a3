// Every string of a sum of Pauli strings on its own, in ONE launch:
//
//     dq_pauli_terms_cross : out[b, t] = s_t c_t sum_i conj(bra[b, i]) (-1)^popc((i ^ x_t) & z_t) ket[b, i ^ x_t]
//
// for the T terms of a table as dq_psum.hip takes it (dq_psum_table.hpp), in table order; c_t is 1 for a term of the
// real-weight class and i for one of the imaginary-weight class, s_t the sign bit of weights[t].  The magnitude of a weight
// is not read: the caller multiplies by sign(h_t), which is exact, and holds the bare <bra|P_t|ket>.
//
// Why a kernel of its own.  dq_psum.hip's signed_sum costs five vector instructions per term and amplitude, which is right
// for ONE sum over the terms.  For T results it would be T reductions.  Here the sign patterns of a unit are shared: a term
// with sign mask z needs sum_j (-1)^popc(j & z) p[j] over the unit's products p, which is entry z of the Walsh-Hadamard
// transform of p.  One transform of the unit serves every term of the group, whatever their number.
//
// Geometry.  That of dq_stream.hpp in gather form, as psum_cross_kernel has it: a unit is 1024 vectors -- 2^sbits
// amplitudes, sbits = 11 (complex64) / 10 (complex128) -- and 256 lanes hold four vectors each.  Units are the outer loop,
// groups the inner one: the lane's own bra vectors are loaded once per unit, the partner vectors v ^ (x >> VB) of the ket
// once per group and unit, those of the next group requested before the transform of this one.  The traffic is G + 1 reads
// of a state, or G where bra is ket and a group has no flip over vectors.
//
// Per group and unit:
//   1. p[j] = conj(bra[j]) ket[j ^ x] at the lane's amplitudes, in double (complex64 products are exact there).  A lane
//      whose vector lies beyond a small sample holds zeros.
//   2. The transform of the unit's 2^sbits products, in place and in natural order.  Amplitude j of the unit is
//      (u, wave, lane, e): e the element of a complex64 vector (bit 0), six lane bits, two wave bits, two unroll bits on
//      top (bits 9, 10; complex128: 8, 9).  The in-lane bits (e, u) are butterflies in registers; the lane bits are
//      cross-lane moves -- DPP within a row of 16 lanes, __shfl_xor across rows (lane_xor) -- the upper lane of a pair
//      taking other - own; then the lane stores its values to LDS and the two wave
//      bits are one radix-4 butterfly per four LDS entries, each owned by one thread.
//   3. Thread tau owns terms tau, tau + 256, .. of the group.  For a term it reads W[z & (2^sbits - 1)] -- one LDS read --
//      flips the sign by popc(unit & (z >> sbits)) + popc(x & z) + the table's sign bit, all uniform over the unit,
//      turns the value by i for the imaginary class, and adds it to the term's accumulator in double.
// Three barriers per group and unit: before the wave stage, before the term reads, before the next stores.
//
// Accumulators.  One double2 per term and workgroup, in LDS, sized to the launch (dynamic shared memory, 16 bytes a
// term).  LDS and not workspace slots: an accumulator is read and written once per unit of its workgroup, which would be a
// round trip to L2 per term and unit; in LDS it costs what the W read next to it costs, and the workspace is written once,
// at the end.  The price is the cap on a launch's terms, dq_pauli_terms_max() = 1024: with the 32 KiB of W that is 48 KiB of
// LDS for complex64 (three workgroups a CU), 32 KiB for complex128.  The host cuts longer tables (backend.pauli_terms_cross).
// A term has one owner and is added to in the order of the workgroup's units: no atomics, a fixed order.
//
// Finish.  Every workgroup writes its T partial sums to ws[b, workgroup, 0..T); terms_finish_kernel adds the workgroups of
// a (sample, term) pair in index order.  Bitwise reproducible, and a sample's bits depend on n and the table alone.
// Workgroups per sample: min(units, TM_BLOCKS = 1024), so ws is batch * min(2^(n - sbits), 1024) * T * 16 bytes: never
// more than T / 1024 of the ket it was computed from, 16 MiB per sample at the most.
//
// Safety, as in dq_psum.hip.  Every x is masked with 2^n - 1, every bound clamped to [0, T], the W index masked to the
// unit; a term index that reaches an accumulator lies in [0, T) by the clamp.  A lane beyond a small sample loads vector
// 0's partners.  Whatever the table holds, no load or LDS access leaves the sample, the table, W or the T accumulators.
#include "dq_psum_table.hpp"

namespace dq {

namespace {

constexpr unsigned TM_BLOCKS = 1024;                    // workgroups per sample striding over its units
constexpr int TM_MAX_TERMS = 1024;                      // accumulators of a launch: 16 KiB of LDS

unsigned terms_blocks_of(uint64_t nvec) {
    const uint64_t units = units_of(nvec);
    return (unsigned)(units < TM_BLOCKS ? units : TM_BLOCKS);
}

int64_t terms_ws_bytes(int n, int64_t batch, bool is_c128, int nterms) {
    return batch * (int64_t)terms_blocks_of(vectors_of(n, is_c128)) * nterms * (int64_t)sizeof(double2);
}

// The lane's partner vectors of the group with flip mask x (masked): ket[v ^ (x >> VB)], or, where the bra is the ket and
// the flip stays inside a vector, the own vectors
template <int VB, bool SAME, typename Q>
__device__ __forceinline__ void load_partners(const Q* __restrict__ pk, uint64_t x, const uint64_t (&vec)[ST_UNROLL],
                                              const Q (&own)[ST_UNROLL], Q (&q)[ST_UNROLL]) {
    const uint64_t vx = x >> VB;
    if (SAME && vx == 0) {
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) q[u] = own[u];
    } else {
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) q[u] = pk[vec[u] ^ vx];
    }
}

__device__ __forceinline__ double2 add2(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 sub2(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// (a, b) -> (a + b, a - b)
__device__ __forceinline__ void butterfly(double2& a, double2& b) {
    const double2 s = add2(a, b);
    b = sub2(a, b);
    a = s;
}

// v of lane (lane ^ O).  Offsets 1 and 2 are one DPP quad permutation, 4 and 8 two DPP moves (a quad reversal then a
// reversal of the half row is ^ 3 ^ 7 = ^ 4; the reversals of the row and of the half row are ^ 15 ^ 7 = ^ 8): register
// moves, where __shfl_xor goes through the LDS crossbar, which this kernel's other stages already fill.  16 and 32 cross
// the rows and take __shfl_xor.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false));
}
template <int O>
__device__ __forceinline__ double lane_xor(double v) {
    constexpr int QUAD_X1 = 0xB1, QUAD_X2 = 0x4E, QUAD_X3 = 0x1B, ROW_MIRROR = 0x140, ROW_HALF_MIRROR = 0x141;
    if constexpr (O == 1) return dpp_move<QUAD_X1>(v);
    else if constexpr (O == 2) return dpp_move<QUAD_X2>(v);
    else if constexpr (O == 4) return dpp_move<ROW_HALF_MIRROR>(dpp_move<QUAD_X3>(v));
    else if constexpr (O == 8) return dpp_move<ROW_HALF_MIRROR>(dpp_move<ROW_MIRROR>(v));
    else return __shfl_xor(v, O, 64);
}

// The butterfly over lane bit log2(O): the upper lane of a pair takes other - own
template <int O, int VEC>
__device__ __forceinline__ void lane_stage(double2 (&v)[ST_UNROLL][VEC], unsigned lane) {
    const double sg = (lane & (unsigned)O) ? -1.0 : 1.0;
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double ox = lane_xor<O>(v[u][e].x), oy = lane_xor<O>(v[u][e].y);
            v[u][e].x = fma(sg, v[u][e].x, ox);
            v[u][e].y = fma(sg, v[u][e].y, oy);
        }
}

template <typename T, bool SAME>
__global__ __launch_bounds__(ST_THREADS) void terms_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                                 PsumTable tb, int n, uint64_t nvec, double2* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int sbits = ST_UNIT_BITS + VB;
    constexpr int WB = 6 + VB;                          // the lower wave bit of an amplitude's index in the unit
    __shared__ double2 W[1 << sbits];
    extern __shared__ double2 acc[];                    // [tb.nterms]
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const uint64_t b = blockIdx.y;
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    const Q* pb = SAME ? pk : reinterpret_cast<const Q*>(bra + (b << n));
    const uint64_t nmask = (1ull << n) - 1ull;
    for (int t = (int)tid; t < tb.nterms; t += ST_THREADS) acc[t] = make_double2(0.0, 0.0);
    __syncthreads();
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < nvec; unit += gridDim.x) {
        uint64_t vec[ST_UNROLL];
        const unsigned live = unit_vectors(unit, nvec, vec);
        Q own[ST_UNROLL], q[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) own[u] = pb[vec[u]];
        uint64_t x = tb.xmasks[0] & nmask;
        load_partners<VB, SAME>(pk, x, vec, own, q);
        for (int g = 0; g < tb.ngroups; ++g) {
            // 1. the products at the lane's amplitudes
            const int x0 = (int)(x & (uint64_t)VB);
            double2 v[ST_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const cx<T> a = vec_get<T>(own[u], e), k = vec_get<T>(q[u], e ^ x0);
                    const double ar = (double)a.x, ai = (double)a.y, kr = (double)k.x, ki = (double)k.y;
                    v[u][e] = (live >> u & 1u) ? make_double2(fma(ar, kr, ai * ki), fma(ar, ki, -(ai * kr))) : make_double2(0.0, 0.0);
                }
            // the next group's partners, in flight across the transform
            const uint64_t xcur = x;
            if (g + 1 < tb.ngroups) {
                x = tb.xmasks[g + 1] & nmask;
                load_partners<VB, SAME>(pk, x, vec, own, q);
            }
            // 2. the transform: in-lane bits, lane bits, wave bits
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u)
                if constexpr (VEC == 2) butterfly(v[u][0], v[u][1]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                butterfly(v[0][e], v[1][e]);
                butterfly(v[2][e], v[3][e]);
                butterfly(v[0][e], v[2][e]);
                butterfly(v[1][e], v[3][e]);
            }
            lane_stage<1>(v, lane);
            lane_stage<2>(v, lane);
            lane_stage<4>(v, lane);
            lane_stage<8>(v, lane);
            lane_stage<16>(v, lane);
            lane_stage<32>(v, lane);
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) W[(((unsigned)(u * ST_THREADS) + tid) << VB) | (unsigned)e] = v[u][e];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < (1 << sbits) / (4 * ST_THREADS); ++k) {
                const unsigned r = tid + (unsigned)(k * ST_THREADS);
                const unsigned base = (r & ((1u << WB) - 1u)) | (r >> WB) << (WB + 2);
                double2 a0 = W[base], a1 = W[base | 1u << WB], a2 = W[base | 2u << WB], a3 = W[base | 3u << WB];
                butterfly(a0, a1);
                butterfly(a2, a3);
                butterfly(a0, a2);
                butterfly(a1, a3);
                W[base] = a0;
                W[base | 1u << WB] = a1;
                W[base | 2u << WB] = a2;
                W[base | 3u << WB] = a3;
            }
            __syncthreads();
            // 3. the group's terms, one owner each
            const int t0 = min(max(tb.bounds[2 * g], 0), tb.nterms), t1 = min(max(tb.bounds[2 * g + 1], 0), tb.nterms),
                      t2 = min(max(tb.bounds[2 * g + 2], 0), tb.nterms);
            for (int t = t0 + (int)tid; t < t2; t += ST_THREADS) {
                const uint64_t z = tb.zmasks[t];
                const double2 w = W[(unsigned)z & ((1u << sbits) - 1u)];
                const unsigned par = ((unsigned)__popcll(unit & (z >> sbits)) + (unsigned)__popcll(xcur & z) +
                                      ((unsigned)__double2hiint(tb.weights[t]) >> 31)) & 1u;
                const double2 r = t >= t1 ? make_double2(-w.y, w.x) : w;
                acc[t] = add2(acc[t], make_double2(flip_sign(r.x, par), flip_sign(r.y, par)));
            }
            __syncthreads();
        }
    }
    double2* part = ws + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * (uint64_t)tb.nterms;
    for (int t = (int)tid; t < tb.nterms; t += ST_THREADS) part[t] = acc[t];
}

// out[b, t] = the sum over the nparts workgroups of sample b, in index order, of ws[b, p, t]
__global__ __launch_bounds__(ST_THREADS) void terms_finish_kernel(const double2* __restrict__ ws, unsigned nparts, int nterms,
                                                                  double2* __restrict__ out) {
    const int t = (int)(blockIdx.x * ST_THREADS + threadIdx.x);
    if (t >= nterms) return;
    const double2* src = ws + (uint64_t)blockIdx.y * nparts * (uint64_t)nterms + (uint64_t)t;
    double2 s = make_double2(0.0, 0.0);
#pragma unroll 8
    for (unsigned p = 0; p < nparts; ++p) s = add2(s, src[(uint64_t)p * (uint64_t)nterms]);
    out[(uint64_t)blockIdx.y * (uint64_t)nterms + (uint64_t)t] = s;
}

template <typename T>
int terms_impl(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks,
               const double* weights, int ngroups, int nterms, int n, int64_t batch, double* out, void* ws, int64_t ws_bytes,
               dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_pauli_terms_cross";
    if (n < 1 || n > 40) {
        set_error("%s: n=%d out of range [1, 40]", what, n);
        return DQ_ERR_ARG;
    }
    if (int rc = check_batch(what, batch)) return rc;
    PsumTable tb;
    if (int rc = check_table(what, xmasks, bounds, zmasks, weights, ngroups, nterms, &tb)) return rc;
    if (nterms > TM_MAX_TERMS) {
        set_error("%s: nterms=%d, a launch takes at most %d terms (dq_pauli_terms_max)", what, nterms, TM_MAX_TERMS);
        return DQ_ERR_ARG;
    }
    if (int rc = check_cross_buffers(what, bra, ket, nullptr, false, out, ws)) return rc;
    const int64_t need = terms_ws_bytes(n, batch, C128, nterms);
    if (ws_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (dq_pauli_terms_ws_bytes)", what, (long long)ws_bytes, (long long)need);
        return DQ_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(out) & 15) {
        set_error("%s: out must be 16-byte aligned", what);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = terms_blocks_of(nvec);
    const dim3 grid(nblk, (unsigned)batch);
    const size_t lds = (size_t)nterms * sizeof(double2);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double2* part = static_cast<double2*>(ws);
    hipStream_t s = as_stream(stream);
    if (bra == ket) hipLaunchKernelGGL((terms_cross_kernel<T, true>), grid, dim3(ST_THREADS), lds, s, pb, pk, tb, n, nvec, part);
    else hipLaunchKernelGGL((terms_cross_kernel<T, false>), grid, dim3(ST_THREADS), lds, s, pb, pk, tb, n, nvec, part);
    hipLaunchKernelGGL(terms_finish_kernel, dim3((unsigned)((nterms + ST_THREADS - 1) / ST_THREADS), (unsigned)batch), dim3(ST_THREADS),
                       0, s, part, nblk, nterms, reinterpret_cast<double2*>(out));
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int dq_pauli_terms_max(void) { return dq::TM_MAX_TERMS; }

extern "C" int64_t dq_pauli_terms_ws_bytes(int n, int64_t batch, int is_c128, int cross, int nterms) {
    (void)cross;        // bra != ket reads one vector more per item and writes the same partial sums
    if (n < 1 || n > 40 || batch < 1 || batch > 65535 || nterms < 1 || nterms > dq::TM_MAX_TERMS) return -1;
    return dq::terms_ws_bytes(n, batch, is_c128 != 0, nterms);
}

extern "C" int dq_pauli_terms_cross_c64(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds,
                                        const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n, int64_t batch,
                                        double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::terms_impl<float>(bra, ket, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_pauli_terms_cross_c128(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds,
                                         const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n, int64_t batch,
                                         double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    return dq::terms_impl<double>(bra, ket, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, out, ws, ws_bytes, stream);
}
