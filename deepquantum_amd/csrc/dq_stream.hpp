// The core of the streaming primitives (dq_diag.hip, dq_pauli.hip, dq_perm.hip, dq_mux.hip, dq_muxgrad.hip): kernels that read a state once in
// 16-byte vectors, do a little arithmetic per amplitude (or none) and either write the state back or reduce it to one
// complex number per sample.
// Each including file gets its own copy of what is here (the library is built without relocatable device code).
//
// Geometry.  A lane moves 16 bytes (two complex64 or one complex128 amplitude) per load, a workgroup of ST_THREADS
// lanes takes ST_UNROLL items per lane and iteration -- a unit of 2^ST_UNIT_BITS items, every load of the unit in
// flight before the first use -- and at most ST_BLOCKS workgroups per sample stride over the units; the sample is the
// grid's y dimension.  An item is whatever the primitive gives a lane to own: a vector, or a pair of vectors.
//
// Reduction.  Lanes accumulate in double over their units, a wave adds its lanes with an xor butterfly (offsets 1, 2,
// 4, .., 32), wave 0's first lane adds the four waves in order 0..3 and writes the workgroup's partial sum
// (write_partial); cross_finish_kernel then adds the partial sums of a sample, strided by ST_THREADS over the lanes,
// the same way.  No atomics, every sum in a fixed order: bitwise reproducible, and that promise lives here alone.
// (dq_muxgrad.hip reduces per bin of select values, not per sample: its fixed orders are its own and stand in its header.)
// The reductions of dq_reduce.hip (a __shfl_down tree from offset 32 downward: another order of additions, other
// bits), dq_entangle.hip, dq_sample.hip and dq_rdm.hip (shaped by their own tiles) are deliberately not built on this.
#pragma once
#include <string.h>
#include "dq_common.hpp"

namespace dq {

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_UNROLL = 4;                            // items per lane and iteration
constexpr int ST_UNIT_BITS = 10;                        // log2(ST_THREADS * ST_UNROLL): items of a unit
constexpr unsigned ST_BLOCKS = 2048;                    // workgroups per sample striding over its units

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

// h with its sign flipped where par is 1: exact, bit for bit (dq_psum.hip, dq_select.hip)
__device__ __forceinline__ float flip_sign(float h, unsigned par) { return __uint_as_float(__float_as_uint(h) ^ (par << 31)); }
__device__ __forceinline__ double flip_sign(double h, unsigned par) {
    return __hiloint2double(__double2hiint(h) ^ (int)(par << 31), __double2loint(h));
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
        for (int w = 1; w < ST_THREADS / 64; ++w) {
            re += sh[w][0];
            im += sh[w][1];
        }
    }
}

// ws[blockIdx.y, blockIdx.x] = the workgroup's sum.  re and im are summed in the caller's own variables, as the kernels
// of dq_diag.hip always did: taken by value, four cost_cross_kernel instantiations are scheduled differently.
__device__ __forceinline__ void write_partial(double& re, double& im, double (*sh)[2], double* ws) {
    block_sum(re, im, sh);
    if (threadIdx.x == 0) {
        double* part = ws + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        part[0] = re;
        part[1] = im;
    }
}

// out[b] = the sum of the nparts partial sums of sample b
__global__ __launch_bounds__(ST_THREADS) void cross_finish_kernel(const double* __restrict__ ws, unsigned nparts,
                                                                  double* __restrict__ out) {
    __shared__ double sh[ST_THREADS / 64][2];
    const uint64_t b = blockIdx.x;
    double re = 0.0, im = 0.0;
    for (unsigned p = threadIdx.x; p < nparts; p += ST_THREADS) {
        re += ws[(b * nparts + p) * 2];
        im += ws[(b * nparts + p) * 2 + 1];
    }
    block_sum(re, im, sh);
    if (threadIdx.x == 0) {
        out[2 * b] = re;
        out[2 * b + 1] = im;
    }
}

// ---- gather over a list of index bits (dq_diag.hip, dq_perm.hip, dq_mux.hip) -------------------------
// sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j) is OR-separable over the index bits.  The host cuts the bit list into
// runs of consecutive positions (a run is one shift, one mask, one shift) and splits them at the size of a unit of
// vectors: the runs below it depend on the lane alone and are evaluated once, before the loop; the runs above depend on
// the unit's index alone, which is uniform over the workgroup: scalar arithmetic, once per iteration.  The control mask
// is split the same way.
constexpr int ST_MAX_RUNS = 42;                         // 40 single bits, one of them split at the unit size

// sub(i) = OR over the runs of ((i >> src) & (2^len - 1)) << dst; runs [0, nlow) lie below the unit size, the rest
// at or above it.
struct Gather {
    int nruns, nlow;
    uint8_t src[ST_MAX_RUNS], len[ST_MAX_RUNS], dst[ST_MAX_RUNS];
    uint64_t cmask;
};

// What a lane keeps across the loop: the low part of sub() and the low control test of each of its amplitudes.
template <int VEC> struct LaneLow {
    uint64_t sub[ST_UNROLL][VEC];
    unsigned ok;                                        // bit u * VEC + e
};

template <int VEC>
__device__ __forceinline__ void lane_low(const Gather& g, int sbits, LaneLow<VEC>& ll) {
    constexpr int VB = VEC == 2 ? 1 : 0;
    const uint64_t cl = g.cmask & ((1ull << sbits) - 1ull);
    ll.ok = 0;
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const uint64_t low = ((uint64_t)(u * ST_THREADS + (int)threadIdx.x) << VB) | (uint64_t)e;
            uint64_t s = 0;
            for (int r = 0; r < g.nlow; ++r) s |= ((low >> g.src[r]) & ((1ull << g.len[r]) - 1ull)) << g.dst[r];
            ll.sub[u][e] = s;
            if ((low & cl) == cl) ll.ok |= 1u << (u * VEC + e);
        }
    }
}

// the unit's part of sub() (uniform over the workgroup)
__device__ __forceinline__ uint64_t chunk_high(const Gather& g, int sbits, uint64_t chunk) {
    uint64_t s = 0;
    for (int r = g.nlow; r < g.nruns; ++r) s |= ((chunk >> (g.src[r] - sbits)) & ((1ull << g.len[r]) - 1ull)) << g.dst[r];
    return s;
}

// the lane's vectors of a unit as they are: all loads, then all stores (dq_perm.hip, dq_select.hip: a unit outside the
// high controls)
template <typename Q> __device__ __forceinline__ void copy_chunk(const Q* own, Q* dst, uint64_t v0, uint64_t nvec) {
    Q q[ST_UNROLL];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
        q[u] = own[v < nvec ? v : nvec - 1];            // (no load is guarded, only the stores are)
    }
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
        if (v < nvec) dst[v] = q[u];
    }
}

// ---- host side ---------------------------------------------------------------------------------
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// the sample is the grid's y dimension
int check_batch(const char* what, int64_t batch) {
    if (batch >= 1 && batch <= 65535) return DQ_OK;
    set_error("%s: batch=%lld outside [1, 65535]", what, (long long)batch);
    return DQ_ERR_ARG;
}

// What a state-to-state primitive allows of its two buffers: a kernel whose lanes own what they read and write takes
// in == out, one that reads where another lane writes (the permutation) does not; a shifted overlap is safe for nobody.
enum Alias { SAME_OR_DISJOINT, DISJOINT };

// Do two ranges of `bytes` bytes share a byte that `alias` does not let them share?
bool clash(const void* p, const void* q, uint64_t bytes, Alias alias) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), o = reinterpret_cast<uintptr_t>(q);
    return (alias == DISJOINT || a != o) && (a > o ? a - o : o - a) < bytes;
}

// One of the state buffers of a primitive, batch * 2^n amplitudes long; an `optional` one may be null
struct StateBuf {
    const char* name;
    const void* p;
    bool optional = false;
};

// What two of them (indices into the primitive's list) may share
struct ApartRule {
    int p, q;
    Alias alias;
};

// The state buffers of a primitive, in the order of the refusals: non-null (but for the optional ones), 16-byte aligned, n
// in [nmin, 40], the batch, then the rules in their order, each over the ranges [p, p + batch * 2^n) (a rule with a null
// buffer says nothing).  `tail` ends the message of a DISJOINT clash.
int check_buffers(const char* what, const StateBuf* bufs, int nbufs, const ApartRule* rules, int nrules, int nmin, int n,
                  int64_t batch, size_t amp_bytes, const char* tail = "") {
    char names[128] = "";                               // "cur, prev, next and acc"
    bool null = false, skew = false;
    for (int i = 0; i < nbufs; ++i) {
        null |= !bufs[i].p && !bufs[i].optional;
        skew |= misaligned(bufs[i].p);
        const size_t at = strlen(names);
        snprintf(names + at, sizeof names - at, "%s%s", i == 0 ? "" : i == nbufs - 1 ? " and " : ", ", bufs[i].name);
    }
    if (null) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    if (skew) {
        set_error("%s: %s must be 16-byte aligned", what, names);
        return DQ_ERR_ARG;
    }
    if (n < nmin || n > 40) {
        set_error("%s: n=%d out of range [%d, 40]", what, n, nmin);
        return DQ_ERR_ARG;
    }
    if (int rc = check_batch(what, batch)) return rc;
    const uint64_t bytes = ((uint64_t)batch << n) * amp_bytes;
    for (int r = 0; r < nrules; ++r) {
        const StateBuf &p = bufs[rules[r].p], &q = bufs[rules[r].q];
        if (!p.p || !q.p || !clash(p.p, q.p, bytes, rules[r].alias)) continue;
        set_error("%s: %s and %s overlap%s", what, p.name, q.name, rules[r].alias == DISJOINT ? tail : " without being equal");
        return DQ_ERR_ARG;
    }
    return DQ_OK;
}

// in and out of a state-to-state primitive: the two buffers of check_buffers under `alias`
int check_states(const char* what, const void* in, const void* out, int nmin, int n, int64_t batch, size_t amp_bytes,
                 Alias alias) {
    const StateBuf bufs[] = {{"in", in}, {"out", out}};
    const ApartRule rule{0, 1, alias};
    return check_buffers(what, bufs, 2, &rule, 1, nmin, n, batch, amp_bytes, " (out of place only)");
}

// The coefficients of a launch, [batch][k] doubles on the device
int check_coef(const char* what, const double* coef) {
    if (coef && !(reinterpret_cast<uintptr_t>(coef) & 7)) return DQ_OK;
    set_error("%s: coef must be non-null and 8-byte aligned", what);
    return DQ_ERR_ARG;
}

uint64_t control_mask(const int* controls, int nc) {
    uint64_t m = 0;
    for (int c = 0; c < nc; ++c) m |= 1ull << controls[c];
    return m;
}

// Validates the lists and builds the runs; `ident`: bits = n-1 .. 0 and no controls.
int plan_gather(const char* what, int n, const int* bits, int k, const int* controls, int nc, int64_t batch, bool is_c128,
                Gather* g, bool* ident) {
    if (k < 1) {
        set_error("%s: k=%d, at least one table bit is needed", what, k);
        return DQ_ERR_ARG;
    }
    if (int rc = validate_bits(n, bits, k, controls, nc)) return rc;
    if (int rc = check_batch(what, batch)) return rc;
    const int sbits = ST_UNIT_BITS + (is_c128 ? 0 : 1);
    *g = Gather{};
    g->cmask = control_mask(controls, nc);
    *ident = nc == 0 && k == n;
    for (int j = 0; j < k && *ident; ++j) *ident = bits[j] == n - 1 - j;
    // runs of consecutive positions, split at the unit size
    struct Run { int src, len, dst; };
    Run low[ST_MAX_RUNS], high[ST_MAX_RUNS];
    int nl = 0, nh = 0;
    for (int j = 0; j < k;) {
        int e = j;
        while (e + 1 < k && bits[e + 1] == bits[e] - 1) ++e;
        Run r{bits[e], e - j + 1, k - 1 - e};
        if (r.src < sbits && r.src + r.len > sbits) {
            const int ll = sbits - r.src;
            low[nl++] = Run{r.src, ll, r.dst};
            high[nh++] = Run{sbits, r.len - ll, r.dst + ll};
        } else if (r.src < sbits) {
            low[nl++] = r;
        } else {
            high[nh++] = r;
        }
        j = e + 1;
    }
    g->nlow = nl;
    g->nruns = nl + nh;
    for (int r = 0; r < nl + nh; ++r) {
        const Run& x = r < nl ? low[r] : high[r - nl];
        g->src[r] = (uint8_t)x.src;
        g->len[r] = (uint8_t)x.len;
        g->dst[r] = (uint8_t)x.dst;
    }
    return DQ_OK;
}

uint64_t vectors_of(int n, bool is_c128) { return 1ull << (n - (is_c128 ? 0 : 1)); }          // (n >= 1)

uint64_t units_of(uint64_t items) { return (items + (1ull << ST_UNIT_BITS) - 1) >> ST_UNIT_BITS; }

unsigned blocks_of(uint64_t items) {
    const uint64_t units = units_of(items);
    return (unsigned)(units < ST_BLOCKS ? units : ST_BLOCKS);
}

// The workspace of a cross reduction: one partial sum per workgroup, sized for a sample's vectors as items (a
// primitive whose items are pairs launches half as many workgroups and leaves the rest unused).
int64_t cross_ws_bytes(int n, int64_t batch, bool is_c128) {
    return batch * (int64_t)blocks_of(vectors_of(n, is_c128)) * 2 * (int64_t)sizeof(double);
}

// what the <what>_ws_bytes exports return: -1 outside the ranges of n and batch
int64_t cross_ws_bytes_or_refuse(int n, int64_t batch, bool is_c128) {
    if (n < 1 || n > 40 || batch < 1 || batch > 65535) return -1;
    return cross_ws_bytes(n, batch, is_c128);
}

// `what` names the entry point; `sizer` the function that sizes its workspace, <what>_ws_bytes where none is given
int check_cross_ws(const char* what, int64_t ws_bytes, int n, int64_t batch, bool is_c128, const char* sizer = nullptr) {
    const int64_t need = cross_ws_bytes(n, batch, is_c128);
    if (ws_bytes >= need) return DQ_OK;
    set_error("%s: workspace of %lld bytes, %lld needed (%s%s)", what, (long long)ws_bytes, (long long)need, sizer ? sizer : what,
              sizer ? "" : "_ws_bytes");
    return DQ_ERR_ARG;
}

// out and ws of a kernel that leaves two sums per sample and whose states are not a bra and a ket (those go through
// check_buffers): non-null, ws 16-byte and out 8-byte aligned -- check_cross_buffers's checks of the two; check_cross_ws
// sizes ws for both.
int check_out_ws(const char* what, const double* out, const void* ws) {
    if (!out || !ws) {
        set_error("%s: null pointer (out, ws)", what);
        return DQ_ERR_ARG;
    }
    if (misaligned(ws) || (reinterpret_cast<uintptr_t>(out) & 7)) {
        set_error("%s: ws must be 16-byte aligned, out 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    return DQ_OK;
}

// The pointers of a cross reduction: bra, ket, the table (where the primitive has one: `has_table`) and ws non-null and
// 16-byte aligned, out non-null and 8-byte aligned.  (On its own for a primitive that sizes its workspace itself.)
int check_cross_buffers(const char* what, const void* bra, const void* ket, const void* table, bool has_table, const double* out,
                        const void* ws) {
    if (!bra || !ket || (has_table && !table) || !out || !ws) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    if (misaligned(bra) || misaligned(ket) || (has_table && misaligned(table)) || misaligned(ws) ||
        (reinterpret_cast<uintptr_t>(out) & 7)) {
        set_error("%s: bra, ket, the table and ws must be 16-byte aligned, out 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    return DQ_OK;
}

// The buffers of a cross reduction, once n and the batch are validated: check_cross_buffers, and ws large enough.
int check_cross(const char* what, const void* bra, const void* ket, const void* table, bool has_table, const double* out,
                const void* ws, int64_t ws_bytes, int n, int64_t batch, bool is_c128) {
    if (int rc = check_cross_buffers(what, bra, ket, table, has_table, out, ws)) return rc;
    return check_cross_ws(what, ws_bytes, n, batch, is_c128);
}

// out[b] = the sum of the nparts partial sums that the first kernel left in ws[b, :]
int finish_cross(const char* what, const double* ws, unsigned nparts, int64_t batch, double* out, hipStream_t s) {
    hipLaunchKernelGGL(cross_finish_kernel, dim3((unsigned)batch), dim3(ST_THREADS), 0, s, ws, nparts, out);
    return check_launch(what);
}

}  // namespace
}  // namespace dq
