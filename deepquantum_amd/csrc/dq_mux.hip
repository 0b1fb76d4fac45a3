// Multiplexed (uniformly controlled) one-qubit gates on any number of select wires: for every value s of k select bits
// its own 2x2 matrix M[s] on one target bit, one read and one write of the state whatever k is.
//
//     sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j)            (bits[0] = the table index's most significant bit)
//     dq_apply_mux : (out[b, i0], out[b, i1]) = M[sub(i0)] (in[b, i0], in[b, i1])
// for every pair i0 (target bit 0), i1 = i0 | 1 << target whose control bits are all 1; the other amplitudes pass through
// bitwise.  The select bits, the controls and the target are disjoint, so sub() and the control test are the same at
// both ends of a pair.  One table for the whole batch, in the state's precision:
//     DQ_MUX_U  : an entry is u00 u01 u10 u11, complex (32 / 64 bytes)
//     DQ_MUX_RY : an entry is (c, s), real, M = [[c, -s], [s, c]] (8 / 16 bytes)
// dagger = 1 applies M^+ from the same table (U: the conjugates with u01 and u10 exchanged; RY: -s).  No trigonometry.
//
// Safety.  sub(i) < 2^k by construction and no address depends on data: whatever the table holds, every access stays
// inside the table and the sample.
//
// Geometry.  That of dq_stream.hpp with the pair as the item, as in dq_pauli.hip with xmask = 1 << target:
//   * the target has a bit tv over vector indices (complex128 always; complex64 with target >= 1): item `it` of the
//     2^(nv - 1) items of a sample is the PAIR of vectors
//         vA = it with a zero inserted at tv,        vB = vA | 1 << tv
//     and holds VEC pairs of amplitudes, element e of vA with element e of vB;
//   * complex64 with target 0 (INNER): the pair sits inside one vector, the item is that vector and holds one pair.
// A lane owns both ends of every pair it touches: in == out is safe, and the traffic is one read and one write.
//
// Pair space.  All table arithmetic is done on the (n - 1)-bit index of a pair, the amplitude index with the target bit
// removed: select and control positions above the target move down by one (the host does that, plan_mux).  The pair
// index of element e of item `it` is (it << PB) | e with PB = log2(pairs of an item) -- the shape the amplitude index
// of a vector has in dq_diag.hip -- so dq_stream.hpp's Gather carries over unchanged: the runs below a unit of items
// are evaluated once per lane before the loop, the runs above once per unit in scalar arithmetic, and the control mask
// is split the same way.  A unit whose high control bits are not all set is copied (or skipped, in place) without a
// table access.  Per unit a lane issues all of its table loads, then all of its state loads, then computes, then stores.
// No LDS.
#include "dq_stream.hpp"

namespace dq {

namespace {

struct Mux {
    Gather g;                                           // over pair space
    int tv;                                             // the target's bit over vector indices (unused when INNER)
    int dagger;
};

template <typename T, int KIND> struct MuxEntry;
template <typename T> struct alignas(2 * sizeof(T)) MuxEntry<T, DQ_MUX_RY> { T c, s; };
template <typename T> struct alignas(16) MuxEntry<T, DQ_MUX_U> { cx<T> u00, u01, u10, u11; };

// (r0, r1) = M (a0, a1), or M^+ (a0, a1): sg = -1 and dg = true
template <typename T>
__device__ __forceinline__ void mux_pair(const MuxEntry<T, DQ_MUX_RY>& m, bool, T sg, cx<T> a0, cx<T> a1, cx<T>& r0, cx<T>& r1) {
    const T s = sg * m.s;
    r0 = mk<T>(m.c * a0.x - s * a1.x, m.c * a0.y - s * a1.y);
    r1 = mk<T>(s * a0.x + m.c * a1.x, s * a0.y + m.c * a1.y);
}
template <typename T>
__device__ __forceinline__ void mux_pair(const MuxEntry<T, DQ_MUX_U>& m, bool dg, T sg, cx<T> a0, cx<T> a1, cx<T>& r0, cx<T>& r1) {
    const cx<T> m00 = mk<T>(m.u00.x, sg * m.u00.y), m11 = mk<T>(m.u11.x, sg * m.u11.y);
    const cx<T> m01 = mk<T>(dg ? m.u10.x : m.u01.x, sg * (dg ? m.u10.y : m.u01.y));
    const cx<T> m10 = mk<T>(dg ? m.u01.x : m.u10.x, sg * (dg ? m.u01.y : m.u10.y));
    r0 = cadd(cmul(m00, a0), cmul(m01, a1));
    r1 = cadd(cmul(m10, a0), cmul(m11, a1));
}

// in and out may be the same buffer: no __restrict__ on them
template <typename T, int KIND, bool INNER>
__global__ __launch_bounds__(ST_THREADS) void mux_kernel(const cx<T>* in, cx<T>* out, const void* __restrict__ table, Mux p, int n,
                                                         uint64_t items) {
    using Q = typename Vec16<T>::type;
    using E = MuxEntry<T, KIND>;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int PV = INNER ? 1 : VEC;                 // pairs of an item
    constexpr int PB = PV == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + PB;            // pairs of a unit
    const uint64_t b = blockIdx.y;
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    const E* tab = static_cast<const E*>(table);
    const bool dg = p.dagger != 0;
    const T sg = dg ? (T)-1 : (T)1;
    LaneLow<PV> ll;
    lane_low<PV>(p.g, SBITS, ll);
    const uint64_t ch = p.g.cmask >> SBITS;
    for (uint64_t unit = blockIdx.x; (unit << ST_UNIT_BITS) < items; unit += gridDim.x) {
        const uint64_t i0 = (unit << ST_UNIT_BITS) + threadIdx.x;
        Q qa[ST_UNROLL], qb[ST_UNROLL];                 // (qb: !INNER only)
        if ((unit & ch) != ch) {                        // a high control bit is 0: the whole unit passes through
            if (src != dst) {
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u) {
                    const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
                    if (it < items) {
                        const uint64_t va = INNER ? it : insert_zero(it, p.tv);
                        qa[u] = src[va];
                        if constexpr (!INNER) qb[u] = src[va | (1ull << p.tv)];
                    }
                }
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u) {
                    const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
                    if (it < items) {
                        const uint64_t va = INNER ? it : insert_zero(it, p.tv);
                        dst[va] = qa[u];
                        if constexpr (!INNER) dst[va | (1ull << p.tv)] = qb[u];
                    }
                }
            }
            continue;
        }
        const uint64_t high = chunk_high(p.g, SBITS, unit);
        E m[ST_UNROLL][PV];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
#pragma unroll
                for (int e = 0; e < PV; ++e) m[u][e] = tab[high | ll.sub[u][e]];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
                const uint64_t va = INNER ? it : insert_zero(it, p.tv);
                qa[u] = src[va];
                if constexpr (!INNER) qb[u] = src[va | (1ull << p.tv)];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
            if (it < items) {
                const uint64_t va = INNER ? it : insert_zero(it, p.tv);
                Q ra = qa[u], rb;
                if constexpr (!INNER) rb = qb[u];
#pragma unroll
                for (int e = 0; e < PV; ++e) {
                    if ((ll.ok >> (u * PV + e)) & 1u) {
                        cx<T> r0, r1;
                        if constexpr (INNER) {
                            mux_pair<T>(m[u][e], dg, sg, vec_get<T>(qa[u], 0), vec_get<T>(qa[u], 1), r0, r1);
                            vec_set(ra, 0, r0);
                            vec_set(ra, 1, r1);
                        } else {
                            mux_pair<T>(m[u][e], dg, sg, vec_get<T>(qa[u], e), vec_get<T>(qb[u], e), r0, r1);
                            vec_set(ra, e, r0);
                            vec_set(rb, e, r1);
                        }
                    }
                }
                dst[va] = ra;
                if constexpr (!INNER) dst[va | (1ull << p.tv)] = rb;
            }
        }
    }
}

// Validates everything, before any HIP call, and moves the select bits and the controls to pair space.
template <typename T>
int plan_mux(const char* what, const void* in, const void* out, const void* table, int kind, int dagger, int n, int target,
             const int* bits, int k, const int* controls, int nc, int64_t batch, Mux* p, bool* inner) {
    constexpr bool C128 = sizeof(T) == 8;
    if (int rc = check_states(what, in, out, 2, n, batch, sizeof(cx<T>), SAME_OR_DISJOINT)) return rc;
    if (!table || misaligned(table)) {
        set_error("%s: the table must be non-null and 16-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (k < 1 || k > n - 1) {
        set_error("%s: k=%d outside [1, n - 1] (n=%d)", what, k, n);
        return DQ_ERR_ARG;
    }
    if (kind != DQ_MUX_U && kind != DQ_MUX_RY) {
        set_error("%s: kind=%d is neither DQ_MUX_U nor DQ_MUX_RY", what, kind);
        return DQ_ERR_ARG;
    }
    if (dagger != 0 && dagger != 1) {
        set_error("%s: dagger=%d is neither 0 nor 1", what, dagger);
        return DQ_ERR_ARG;
    }
    if (target < 0 || target >= n) {
        set_error("%s: target %d out of range [0, %d)", what, target, n);
        return DQ_ERR_ARG;
    }
    if (int rc = validate_bits(n, bits, k, controls, nc)) return rc;
    int pbits[40], pctl[40];                            // (k + nc <= n <= 40 from here on)
    for (int j = 0; j < k + nc; ++j) {
        const int q = j < k ? bits[j] : controls[j - k];
        if (q == target) {
            set_error("%s: bit position %d is the target and a %s", what, q, j < k ? "select bit" : "control");
            return DQ_ERR_ARG;
        }
        (j < k ? pbits[j] : pctl[j - k]) = q > target ? q - 1 : q;
    }
    *inner = !C128 && target == 0;
    // a unit is 2^ST_UNIT_BITS items of one pair (complex128, INNER: the split plan_gather makes for complex128) or two
    bool ident;
    if (int rc = plan_gather(what, n - 1, pbits, k, pctl, nc, batch, C128 || *inner, &p->g, &ident)) return rc;
    p->tv = *inner ? 0 : target - (C128 ? 0 : 1);
    p->dagger = dagger;
    return DQ_OK;
}

template <typename T>
int mux_impl(const void* in, void* out, const void* table, int kind, int dagger, int n, int target, const int* bits, int k,
             const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_mux";
    Mux p;
    bool inner;
    if (int rc = plan_mux<T>(what, in, out, table, kind, dagger, n, target, bits, k, controls, nc, batch, &p, &inner)) return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const uint64_t items = inner ? nvec : nvec >> 1;
    const dim3 grid(blocks_of(items), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    hipStream_t s = as_stream(stream);
#define DQ_MUX(KIND, INNER) \
    hipLaunchKernelGGL((mux_kernel<T, KIND, INNER>), grid, dim3(ST_THREADS), 0, s, pi, po, table, p, n, items)
    if constexpr (C128) {
        if (kind == DQ_MUX_U) DQ_MUX(DQ_MUX_U, false);
        else DQ_MUX(DQ_MUX_RY, false);
    } else {
        if (kind == DQ_MUX_U && inner) DQ_MUX(DQ_MUX_U, true);
        else if (kind == DQ_MUX_U) DQ_MUX(DQ_MUX_U, false);
        else if (inner) DQ_MUX(DQ_MUX_RY, true);
        else DQ_MUX(DQ_MUX_RY, false);
    }
#undef DQ_MUX
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_mux_c64(const void* in, void* out, const void* table, int kind, int dagger, int n, int target,
                                const int* bits, int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::mux_impl<float>(in, out, table, kind, dagger, n, target, bits, k, controls, nc, batch, stream);
}
extern "C" int dq_apply_mux_c128(const void* in, void* out, const void* table, int kind, int dagger, int n, int target,
                                 const int* bits, int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::mux_impl<double>(in, out, table, kind, dagger, n, target, bits, k, controls, nc, batch, stream);
}
