// SELECT over Pauli strings: sum_s |s><s| (x) c_s P_s, the string P_s = (x_s, z_s) with the phase c_s = i^q_s on the wires
// outside k select bits, for every value s of the select bits -- the middle of a linear combination of unitaries -- in
// one read and one write of the state whatever the number of strings.  A signed, phased gather:
//
//     s = sub(i)                                       (sub() over bits[0..k) as in dq_stream.hpp, bits[0] = its MSB)
//     (x, z, q) = table[s],   x &= free,   j = i ^ x
//     dq_apply_select_pauli : out[b, i] = i^q (-1)^popc(j & z) in[b, j]
// on the amplitudes whose control bits are all 1; the others are copied.  free = (2^n - 1) & ~(select bits | control
// bits), so an amplitude and its source have the same s and are both inside the controls or both outside.  Out of place
// only: the partner of a vector is another lane's.
//
// The table has 2^k entries of two uint64 (16 bytes, one load): word0 = x | q << 62, word1 = z.  i^q with q already
// holding the i^ny of the string's Y factors: whoever builds the table folds them in (backend.SelectTable).
//
// Exactness.  i^q (-1)^p is one of 1, i, -1, -i: re and im are swapped and their sign bits flipped, never multiplied.
// The result is exact in both precisions, and an entry with x = z = q = 0 copies its amplitudes bit for bit.
//
// Safety.  x is masked with `free` in the kernel and sub() cannot leave [0, 2^k): whatever the table holds, no load
// leaves the sample or the table, and a wrong table gives a wrong state, nothing else.  z is used as it stands (a sign).
//
// Geometry.  That of dq_stream.hpp with an OUTPUT vector as the item: a unit is 1024 vectors, every store a coalesced
// 16-byte store.  Per unit a lane issues all of its table loads, then all of its loads of the state, then computes, then
// stores.  A unit whose high control bits are not all set is copied with no table access.  No LDS.
//
// One kernel, three instantiations per precision (complex128 has no SPLIT):
//   UNIFORM  every select bit at or above the unit size: s is uniform over the workgroup, the entry comes in through
//            scalar loads once per unit; partner vectors vec ^ (x >> VB) as 16-byte loads; a complex64 vector whose
//            partner differs in index bit 0 has its two elements swapped (e ^ x0).
//   LANE     some select bit below the unit size, but index bit 0 of a complex64 state neither a select bit nor a
//            control: the low part of s is the lane's (lane_low, once before the loop), one entry per vector from the
//            table in global memory (2^k * 16 bytes: it lives in L2); loads are still 16 bytes.
//   SPLIT    complex64 with index bit 0 a select bit or a control: the two elements of an output vector have different
//            entries, or one of them is copied -- two entries and two 8-byte loads per output vector.
#include "dq_stream.hpp"

namespace dq {

namespace {

enum SelectMode { SEL_UNIFORM, SEL_LANE, SEL_SPLIT };

struct Select {
    Gather g;
    uint64_t free;                                      // the index bits a string may flip
};

struct Entry {
    uint64_t x, z;
    unsigned q;
};

__device__ __forceinline__ Entry entry_of(ulonglong2 w, uint64_t free) { return Entry{w.x & free, w.y, (unsigned)(w.x >> 62)}; }

// The power of i that amplitude (unit, low) takes from its source j = i ^ x: q + 2 popc(j & z) mod 4.  The part of j at or
// above the unit size meets the unit's index (scalar where the entry is uniform), the part below it the lane's.
template <int SBITS> __device__ __forceinline__ unsigned power_of(const Entry& en, uint64_t unit, unsigned low) {
    const unsigned par = (unsigned)__popcll((unit ^ (en.x >> SBITS)) & (en.z >> SBITS)) +
                         (unsigned)__popc((low ^ (unsigned)en.x) & (unsigned)en.z & ((1u << SBITS) - 1u));
    return (en.q + 2u * par) & 3u;
}

// i^q a: a swap and two sign flips
template <typename T> __device__ __forceinline__ cx<T> turn(cx<T> a, unsigned q) {
    const bool swap = q & 1u;
    return mk<T>(flip_sign(swap ? a.y : a.x, ((q + 1u) >> 1) & 1u), flip_sign(swap ? a.x : a.y, q >> 1));
}

template <typename T, int MODE>
__global__ __launch_bounds__(ST_THREADS) void select_pauli_kernel(const cx<T>* __restrict__ in, cx<T>* __restrict__ out,
                                                                  const ulonglong2* __restrict__ table, Select p, int n,
                                                                  uint64_t nunits) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;            // amplitudes of a unit
    constexpr int PER = MODE == SEL_SPLIT ? VEC : 1;    // entries, and loads, of an output vector
    static_assert(MODE != SEL_SPLIT || VEC == 2, "a complex128 vector is one amplitude");
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* own = reinterpret_cast<const Q*>(in + (b << n));
    const cx<T>* amp = in + (b << n);
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    LaneLow<VEC> ll;
    lane_low<VEC>(p.g, SBITS, ll);
    const uint64_t ch = p.g.cmask >> SBITS;
    for (uint64_t unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const uint64_t v0 = (unit << ST_UNIT_BITS) + threadIdx.x;
        if ((unit & ch) != ch) {                        // a high control bit is 0: the whole unit is copied
            copy_chunk(own, dst, v0, nvec);
            continue;
        }
        const uint64_t high = chunk_high(p.g, SBITS, unit);
        // every load below is made by every lane, at a place that is valid whatever the lane (a sample smaller than a
        // unit leaves lanes without a vector: they load vector 0): only the stores are guarded
        Entry en[ST_UNROLL][PER];
        if constexpr (MODE == SEL_UNIFORM) {
            const Entry one = entry_of(table[high], p.free);        // (uniform: scalar loads)
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) en[u][0] = one;
        } else {
            ulonglong2 w[ST_UNROLL][PER];
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
                for (int e = 0; e < PER; ++e) w[u][e] = table[high | ll.sub[u][e]];
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u)
#pragma unroll
                for (int e = 0; e < PER; ++e) en[u][e] = entry_of(w[u][e], p.free);
        }
        Q r[ST_UNROLL];
        if constexpr (MODE == SEL_SPLIT) {
            cx<T> q[ST_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const uint64_t i = (v << VB) | (uint64_t)e;
                    const uint64_t a = ((ll.ok >> (u * VEC + e)) & 1u) ? i ^ en[u][e].x : i;
                    q[u][e] = amp[v < nvec ? a : 0];
                }
            }
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const unsigned low = ((unsigned)(u * ST_THREADS) + threadIdx.x) << VB | (unsigned)e;
                    const unsigned pw = ((ll.ok >> (u * VEC + e)) & 1u) ? power_of<SBITS>(en[u][e], unit, low) : 0u;
                    vec_set(r[u], e, turn<T>(q[u][e], pw));
                }
            }
        } else {
            // (index bit 0 of a complex64 state is neither a select bit nor a control: the elements of a vector share
            // their entry and their control test, those of element 0)
            Q q[ST_UNROLL];
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
                const uint64_t a = ((ll.ok >> (u * VEC)) & 1u) ? v ^ (en[u][0].x >> VB) : v;
                q[u] = own[v < nvec ? a : 0];
            }
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const bool ok = (ll.ok >> (u * VEC)) & 1u;
                const int x0 = ok ? (int)(en[u][0].x & (uint64_t)VB) : 0;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const unsigned low = ((unsigned)(u * ST_THREADS) + threadIdx.x) << VB | (unsigned)e;
                    const unsigned pw = ok ? power_of<SBITS>(en[u][0], unit, low) : 0u;
                    vec_set(r[u], e, turn<T>(vec_get<T>(q[u], e ^ x0), pw));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) dst[v] = r[u];
        }
    }
}

template <typename T>
int select_impl(const void* in, void* out, const uint64_t* table, int n, const int* bits, int k, const int* controls, int nc,
                int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_select_pauli";
    if (k < 1 || k > n || k > 31) {                     // (first: its text names n, and at n = 40 most pairs of pointers overlap)
        set_error("%s: k=%d outside [1, min(n, 31)] (n=%d)", what, k, n);
        return DQ_ERR_ARG;
    }
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), DISJOINT)) return rc;
    if (!table || misaligned(table)) {
        set_error("%s: the table must be non-null and 16-byte aligned", what);
        return DQ_ERR_ARG;
    }
    Select p;
    bool ident;
    if (int rc = plan_gather(what, n, bits, k, controls, nc, batch, C128, &p.g, &ident)) return rc;
    uint64_t smask = 0;
    for (int j = 0; j < k; ++j) smask |= 1ull << bits[j];
    p.free = ((1ull << n) - 1ull) & ~(smask | p.g.cmask);
    const uint64_t nvec = vectors_of(n, C128);
    const dim3 grid(blocks_of(nvec), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    const ulonglong2* pt = reinterpret_cast<const ulonglong2*>(table);
    hipStream_t s = as_stream(stream);
#define DQ_SELECT(MODE) \
    hipLaunchKernelGGL((select_pauli_kernel<T, MODE>), grid, dim3(ST_THREADS), 0, s, pi, po, pt, p, n, units_of(nvec))
    if constexpr (C128) {
        if (p.g.nlow == 0) DQ_SELECT(SEL_UNIFORM);
        else DQ_SELECT(SEL_LANE);
    } else {
        if ((smask | p.g.cmask) & 1ull) DQ_SELECT(SEL_SPLIT);
        else if (p.g.nlow == 0) DQ_SELECT(SEL_UNIFORM);
        else DQ_SELECT(SEL_LANE);
    }
#undef DQ_SELECT
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_select_pauli_c64(const void* in, void* out, const uint64_t* table, int n, const int* bits, int k,
                                         const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::select_impl<float>(in, out, table, n, bits, k, controls, nc, batch, stream);
}
extern "C" int dq_apply_select_pauli_c128(const void* in, void* out, const uint64_t* table, int n, const int* bits, int k,
                                          const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::select_impl<double>(in, out, table, n, bits, k, controls, nc, batch, stream);
}

extern "C" int dq_select_pauli_unit_bits(int is_c128) { return dq::ST_UNIT_BITS + (is_c128 ? 0 : 1); }
