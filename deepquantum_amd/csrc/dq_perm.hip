// Basis-state permutations on any number of wires: |x> -> |perm(x)> on k index bits, one read and one write of the
// state and no arithmetic on the amplitudes at all.
//
//     sub(i)    = sum_j bit_{bits[j]}(i) << (k - 1 - j)            (bits[0] = the table index's most significant bit)
//     put(i, v) = i with those k bits replaced by the bits of v, so that sub(put(i, v)) = v
//     dq_apply_permutation : out[b, j] = in[b, put(j, src[sub(j)])]          (gather form, src = perm^-1)
// on the amplitudes whose control bits are all 1; the others are copied.  The controls are disjoint from the table
// bits, so an amplitude and its source are both inside the controls or both outside.  Out of place only: for a general
// table nobody owns both ends of a cycle.  Amplitudes are moved as bits, never as numbers.
//
// Safety.  A table entry is masked with 2^k - 1 before use and put() touches the table bits alone: whatever the table
// holds, every load stays inside the sample.  A table that is no bijection gives a wrong state, nothing else.
//
// Geometry.  That of dq_stream.hpp with a vector as the item: a chunk is a unit of 1024 vectors, 16 KiB.  A lane owns
// output vectors, so every store is a coalesced 16-byte store.
//
// Elements.  What moves as one piece: a whole vector (WIDE: complex128 always; complex64 when index bit 0 is neither a
// table bit nor a control, so that the two amplitudes of a vector share their source vector) or one complex64 amplitude
// (8-byte loads, two per vector).
//
// GATHER (any table bits).  sub() through dq_stream.hpp's Gather: the low runs once per lane before the loop, the high
// runs once per chunk in scalar arithmetic.  put() scatters the entry back over the same runs.  A lane's ST_UNROLL * 2
// table loads at most are all issued before the first is used, then all of its loads of the state before the first store.
// A chunk whose high control bits are not all set is copied with vector loads and no table access.
//
// LOCAL (every table bit below the chunk size; controls anywhere).  The source of an element lies in the element's own
// chunk at a place that depends on the lane alone: it is worked out once, before the loop.  Per chunk: coalesced vector
// loads, a linear image of the chunk in LDS (16 KiB), one barrier, one LDS read per element at its source -- the widest
// naturally aligned read an element allows, ds_read_b128 for WIDE and ds_read_b64 otherwise, which both bank over the full
// 64-dword row; what conflicts remain are the table's -- and coalesced stores.  No table access inside the loop.
#include <type_traits>

#include "dq_stream.hpp"

namespace dq {

namespace {

struct Perm {
    Gather g;
    uint64_t tmask;                                     // the table bits over amplitude indices
    uint32_t kmask;                                     // 2^k - 1
};

// the bits of table entry v at the table's index positions: sub(scatter(v)) = v
__device__ __forceinline__ uint64_t scatter(const Gather& g, uint32_t v) {
    uint64_t s = 0;
    for (int r = 0; r < g.nruns; ++r) s |= (((uint64_t)v >> g.dst[r]) & ((1ull << g.len[r]) - 1ull)) << g.src[r];
    return s;
}

template <typename T, bool WIDE> struct Elem {
    using Q = typename Vec16<T>::type;
    static constexpr int VEC = 16 / (int)sizeof(cx<T>);
    static constexpr int VB = VEC == 2 ? 1 : 0;
    static constexpr int PER = WIDE ? 1 : VEC;          // elements of a vector
    static constexpr int EB = WIDE ? VB : 0;            // amplitude-index bits inside an element
    using type = typename std::conditional<WIDE, Q, cx<T>>::type;
};

__device__ __forceinline__ float4 join_pair(const float2 (&q)[2]) { return make_float4(q[0].x, q[0].y, q[1].x, q[1].y); }

template <typename T, bool WIDE>
__device__ __forceinline__ typename Vec16<T>::type vector_of(const typename Elem<T, WIDE>::type (&q)[Elem<T, WIDE>::PER]) {
    if constexpr (WIDE) return q[0];
    else return join_pair(q);
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(ST_THREADS) void perm_gather_kernel(const cx<T>* __restrict__ in, cx<T>* __restrict__ out,
                                                                 const uint32_t* __restrict__ table, Perm p, int n,
                                                                 uint64_t nchunks) {
    using EL = Elem<T, WIDE>;
    using Q = typename EL::Q;
    using E = typename EL::type;
    constexpr int VEC = EL::VEC, VB = EL::VB, PER = EL::PER, EB = EL::EB;
    constexpr int SBITS = ST_UNIT_BITS + VB;            // amplitudes of a chunk
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* own = reinterpret_cast<const Q*>(in + (b << n));
    const E* src = reinterpret_cast<const E*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    LaneLow<VEC> ll;
    lane_low<VEC>(p.g, SBITS, ll);
    const uint64_t ch = p.g.cmask >> SBITS;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        if ((chunk & ch) != ch) {                       // a high control bit is 0: the whole chunk is copied
            copy_chunk(own, dst, v0, nvec);
            continue;
        }
        const uint64_t high = chunk_high(p.g, SBITS, chunk);
        const uint64_t base = (chunk << SBITS) & ~p.tmask;
        // every load below is made by every lane, at a place that is valid whatever the lane (a sample smaller than a
        // chunk leaves lanes without a vector): nothing stands between the loads, and only the stores are guarded
        uint32_t t[ST_UNROLL][PER];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < PER; ++e) t[u][e] = table[high | ll.sub[u][e]] & p.kmask;
        }
        E q[ST_UNROLL][PER];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const uint64_t low = ((uint64_t)(u * ST_THREADS + (int)threadIdx.x) << VB) | (uint64_t)e;
                const uint64_t moved = base | (low & ~p.tmask) | scatter(p.g, t[u][e]);
                uint64_t a = ((ll.ok >> (u * VEC + e)) & 1u) ? moved : ((chunk << SBITS) | low);
                a = v < nvec ? a : 0;
                q[u][e] = src[a >> EB];
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) dst[v] = vector_of<T, WIDE>(q[u]);
        }
    }
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(ST_THREADS) void perm_local_kernel(const cx<T>* __restrict__ in, cx<T>* __restrict__ out,
                                                                const uint32_t* __restrict__ table, Perm p, int n,
                                                                uint64_t nchunks) {
    using EL = Elem<T, WIDE>;
    using Q = typename EL::Q;
    using E = typename EL::type;
    constexpr int VEC = EL::VEC, VB = EL::VB, PER = EL::PER, EB = EL::EB;
    constexpr int SBITS = ST_UNIT_BITS + VB;
    __shared__ Q image[1 << ST_UNIT_BITS];              // the chunk, linearly
    const E* elems = reinterpret_cast<const E*>(image);
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* own = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    // where each of the lane's elements comes from inside its chunk (every run is a low run)
    const uint64_t cl = p.g.cmask & ((1ull << SBITS) - 1ull);
    unsigned from[ST_UNROLL][PER];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const uint64_t low = ((uint64_t)(u * ST_THREADS + (int)threadIdx.x) << VB) | (uint64_t)e;
            uint64_t s = 0;
            for (int r = 0; r < p.g.nruns; ++r) s |= ((low >> p.g.src[r]) & ((1ull << p.g.len[r]) - 1ull)) << p.g.dst[r];
            const uint64_t moved = (low & ~p.tmask) | scatter(p.g, table[s] & p.kmask);
            from[u][e] = (unsigned)(((low & cl) == cl ? moved : low) >> EB);        // (inside the image whatever the lane)
        }
    }
    const uint64_t ch = p.g.cmask >> SBITS;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        if ((chunk & ch) != ch) {                       // a high control bit is 0: the whole chunk is copied (uniform)
            copy_chunk(own, dst, v0, nvec);
            continue;
        }
        // (a sample smaller than a chunk: the lanes without a vector load the last one and write it behind the sample's
        // part of the image, where nobody reads: no load and no LDS access is guarded, only the stores are)
        Q q[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            q[u] = own[v < nvec ? v : nvec - 1];
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) image[u * ST_THREADS + (int)threadIdx.x] = q[u];
        __syncthreads();
        E x[ST_UNROLL][PER];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < PER; ++e) x[u][e] = elems[from[u][e]];
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) dst[v] = vector_of<T, WIDE>(x[u]);
        }
        __syncthreads();                                // (the image is written again in the next iteration)
    }
}

// Validates everything, before any HIP call, and splits the table bits for the kernels.
template <typename T>
int plan_perm(const char* what, const void* in, const void* out, const uint32_t* table, int n, const int* bits, int k,
              const int* controls, int nc, int64_t batch, int path, Perm* p, bool* local) {
    constexpr bool C128 = sizeof(T) == 8;
    if (k < 1 || k > n || k > 31) {                     // (first: its text names n, and at n = 40 most pairs of pointers overlap)
        set_error("%s: k=%d outside [1, min(n, 31)] (n=%d)", what, k, n);
        return DQ_ERR_ARG;
    }
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), DISJOINT)) return rc;
    if (!table || (reinterpret_cast<uintptr_t>(table) & 3)) {
        set_error("%s: the table must be non-null and 4-byte aligned", what);
        return DQ_ERR_ARG;
    }
    bool ident;
    if (int rc = plan_gather(what, n, bits, k, controls, nc, batch, C128, &p->g, &ident)) return rc;
    if (path != DQ_PERM_AUTO && path != DQ_PERM_GATHER && path != DQ_PERM_LOCAL) {
        set_error("%s: path=%d is none of DQ_PERM_AUTO, DQ_PERM_GATHER, DQ_PERM_LOCAL", what, path);
        return DQ_ERR_ARG;
    }
    const int sbits = ST_UNIT_BITS + (C128 ? 0 : 1);
    p->tmask = 0;
    for (int j = 0; j < k; ++j) p->tmask |= 1ull << bits[j];
    p->kmask = (uint32_t)((1ull << k) - 1ull);
    const bool fits = (p->tmask >> sbits) == 0;
    if (path == DQ_PERM_LOCAL && !fits) {
        set_error("%s: DQ_PERM_LOCAL needs every table bit below %d (dq_permutation_local_bits)", what, sbits);
        return DQ_ERR_ARG;
    }
    // Where both paths apply AUTO takes LOCAL.  On the same tables at batch 4 (complex64 n = 28 / complex128 n = 27; k = 4
    // with bit 0 free, k = 4 with bit 0 a table bit, a random table over all the low bits of a chunk) LOCAL took 0.94 to
    // 0.95 / 0.98 to 1.00 of the time of dq_apply_diag_* on the same buffers and GATHER 1.04, 1.69, 2.10 / 1.14, 1.14,
    // 1.58: LOCAL is the faster in every class, so there is no threshold (tools/bench_perm.py, profiles/perm/, DESIGN.md
    // section 4.10).
    *local = path == DQ_PERM_LOCAL || (path == DQ_PERM_AUTO && fits);
    return DQ_OK;
}

template <typename T>
int perm_impl(const void* in, void* out, const uint32_t* table, int n, const int* bits, int k, const int* controls, int nc,
              int64_t batch, int path, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_permutation";
    Perm p;
    bool local;
    if (int rc = plan_perm<T>(what, in, out, table, n, bits, k, controls, nc, batch, path, &p, &local)) return rc;
    const bool wide = C128 || ((p.tmask | p.g.cmask) & 1ull) == 0;
    const uint64_t nvec = vectors_of(n, C128);
    const dim3 grid(blocks_of(nvec), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    hipStream_t s = as_stream(stream);
#define DQ_PERM(KERNEL, WIDE) \
    hipLaunchKernelGGL((KERNEL<T, WIDE>), grid, dim3(ST_THREADS), 0, s, pi, po, table, p, n, units_of(nvec))
    if constexpr (C128) {
        if (local) DQ_PERM(perm_local_kernel, true);
        else DQ_PERM(perm_gather_kernel, true);
    } else {
        if (local && wide) DQ_PERM(perm_local_kernel, true);
        else if (local) DQ_PERM(perm_local_kernel, false);
        else if (wide) DQ_PERM(perm_gather_kernel, true);
        else DQ_PERM(perm_gather_kernel, false);
    }
#undef DQ_PERM
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_permutation_c64(const void* in, void* out, const uint32_t* src, int n, const int* bits, int k,
                                        const int* controls, int nc, int64_t batch, int path, dq_stream_t stream) {
    return dq::perm_impl<float>(in, out, src, n, bits, k, controls, nc, batch, path, stream);
}
extern "C" int dq_apply_permutation_c128(const void* in, void* out, const uint32_t* src, int n, const int* bits, int k,
                                         const int* controls, int nc, int64_t batch, int path, dq_stream_t stream) {
    return dq::perm_impl<double>(in, out, src, n, bits, k, controls, nc, batch, path, stream);
}

extern "C" int dq_permutation_local_bits(int is_c128) { return dq::ST_UNIT_BITS + (is_c128 ? 0 : 1); }
