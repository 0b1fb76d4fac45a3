// Mid-circuit measurement: the draw of an outcome per sample from a marginal table, and the collapse X^x Z^z P_o of the
// state onto it, every sample of a batch onto its own outcome with its own Pauli correction, in one pass.
//
//     sub(i)     = sum_j bit_{bits[j]}(i) << (k - 1 - j)        (bits[0] = the outcome's most significant bit)
//     scatter(o) = the index with o's bits at `bits` and 0 elsewhere;  M = scatter(2^k - 1)
//     ext(i)     = i with the k measured bits squeezed out (n - k bits)
//     sigma(i)   = (-1)^popcount(i & z)
//
//     FULL            out[j] = s sigma(j ^ x) in[j ^ x]   where sub(j ^ x) == o,  0 elsewhere
//     FULL, transpose out[i] = s sigma(i) in[i ^ x]       where sub(i) == o,      0 elsewhere
//     DROP            out[t] = s sigma(i) in[i],          i the kept index with ext(i ^ (x & ~M)) == t     (2^(n-k) amplitudes)
//     DROP, transpose out[i] = s sigma(i) in[ext(i ^ x)]  where sub(i) == o,      0 elsewhere              (2^(n-k) -> 2^n)
// with (o, x, z, s) = rec[b], read on the device.  The map has real entries, so the transpose is what a backward pass runs.
//
// One loop serves the four maps.  Seen from the output index p, each of them is
//     out[p] = s (-1)^(popcount(p & zs) ^ c) in[map(p) ^ xs]    where (p & M) == kv
// with map = the identity (FULL), the deposit of p's bits into the kept positions (DROP) or ext (DROP transposed) --
// all three linear over xor, so x moves out of the map -- and xs, zs, c, kv uniform over the workgroup:
//     FULL            xs = x              zs = z       c = popcount(x & z)   kv = scatter(o) ^ (x & M)
//     FULL, transpose xs = x              zs = z       c = 0                 kv = scatter(o)
//     DROP            xs = x & ~M | s(o)  zs = ext(z)  c = popcount(xs & z)  every p is kept
//     DROP, transpose xs = ext(x)         zs = z       c = 0                 kv = scatter(o)
//
// Geometry.  That of dq_stream.hpp with an OUTPUT vector as the item: workgroups stride over units of 1024 output
// vectors, every store is a full 16-byte store of a coalesced wave, and a source vector is loaded only where the
// output vector holds a kept amplitude.  The measured bits at or above the unit size are tested on the unit's index,
// in scalar arithmetic: a unit outside the kept slice is zero-filled without a load and without a lane predicate.  The
// measured bits below it are tested per lane, once, before the loop (four bits of a mask); they are coherent in runs of
// 2^(lowest measured bit) amplitudes.  The bits of xs at or above the vector bit are xor-ed into the load address --
// lines are permuted, never split -- and bit 0 of a complex64 state swaps the halves of the loaded vector in registers.
// With bit 0 measured in complex64 (the LOW0 instantiations) a vector holds one kept and one dropped amplitude: the
// kept one comes from an 8-byte load and the other half is written as 0; in DROP the two halves of an output vector
// come from two 8-byte loads.  map() is evaluated in runs of consecutive kept positions, split at the unit size as
// dq_stream.hpp's gather is: the low runs once per lane, the high runs once per unit.
// Traffic: one write of the output and 1 / 2^k of a read.  No LDS, no atomics, nothing but rec is read twice.
//
// Exactness.  The sign is flipped bit for bit and the scale is one multiplication by s rounded to the state's real
// precision: s == 1 without masks copies the kept slice bit for bit, and everything outside it is +0.
//
// In place.  A lane reads vector (v ^ xs >> 1) and writes vector v: with x == 0 and FULL they are the same vector and
// in == out is safe.  The host cannot see x, so the caller says whether rec may carry one (`may_flip`); with
// may_flip == 0 the kernel does not read xmask at all.
//
// The draw.  One workgroup per sample over the 2^k <= 2^20 entries of its marginal: every lane adds a contiguous
// segment in index order, lane 0 adds the 256 segment sums in order, the first segment whose inclusive sum exceeds
// u T and that holds a non-zero entry is walked again in index order.  Entries of probability 0 are excluded by value
// and a residual that rounding carried beyond the last sum ends at the last non-zero entry: never an outcome of
// probability 0, never one outside [0, 2^k) -- the promises of dq_sample.hip.  Every sum in a fixed order.
#include <stddef.h>
#include "dq_stream.hpp"

namespace dq {

namespace {

enum { COL_FULL = 0, COL_SQUEEZE = 1, COL_EXPAND = 2 };        // the map of the loop: identity, deposit, ext

constexpr int COL_MAX_K = 20;

struct Measured {
    int k;
    uint8_t pos[COL_MAX_K];                             // bits[0 .. k): most significant bit of the outcome first
};

// OR over the runs [lo, hi) of ((i >> src) & (2^len - 1)) << dst
__device__ __forceinline__ uint64_t map_runs(const Gather& g, int lo, int hi, uint64_t i, int shift) {
    uint64_t s = 0;
    for (int r = lo; r < hi; ++r) s |= ((i >> (g.src[r] - shift)) & ((1ull << g.len[r]) - 1ull)) << g.dst[r];
    return s;
}

// the same runs read backwards: the inverse map on the bits it covers
__device__ __forceinline__ uint64_t unmap_runs(const Gather& g, uint64_t i) {
    uint64_t s = 0;
    for (int r = 0; r < g.nruns; ++r) s |= ((i >> g.dst[r]) & ((1ull << g.len[r]) - 1ull)) << g.src[r];
    return s;
}

template <typename T> __device__ __forceinline__ cx<T> scaled(cx<T> a, T s, uint64_t q, uint64_t zs, unsigned c) {
    const unsigned par = ((unsigned)__popcll(q & zs) ^ c) & 1u;
    return mk<T>(flip_sign(s * a.x, par), flip_sign(s * a.y, par));
}

// in and out may be the same buffer (FULL without x): no __restrict__ on them
template <typename T, int MODE, bool LOW0>
__global__ __launch_bounds__(ST_THREADS) void collapse_kernel(const cx<T>* in, cx<T>* out, const DqCollapseRec* __restrict__ rec,
                                                              Measured m, Gather g, int n, int transpose, int may_flip,
                                                              uint64_t nchunks) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;            // amplitudes of a unit
    static_assert(!LOW0 || VB == 1, "bit 0 splits a vector of complex64 only");
    const uint64_t b = blockIdx.y;
    const int nout = MODE == COL_SQUEEZE ? n - m.k : n;
    const int nin = MODE == COL_EXPAND ? n - m.k : n;
    const uint64_t nvec = 1ull << (nout - VB);
    const cx<T>* src = in + (b << nin);
    Q* dst = reinterpret_cast<Q*>(out + (b << nout));

    // the sample's record, uniform over the workgroup; whatever it holds is cut to the index bits there are
    const uint64_t full = (1ull << n) - 1ull;
    const uint64_t o = (uint64_t)rec[b].outcome & ((1ull << m.k) - 1ull);
    const uint64_t x = may_flip ? rec[b].xmask & full : 0ull;
    const uint64_t z = rec[b].zmask & full;
    const T s = (T)rec[b].scale;
    uint64_t M = 0, ov = 0;
    for (int j = 0; j < m.k; ++j) {
        M |= 1ull << m.pos[j];
        ov |= ((o >> (m.k - 1 - j)) & 1ull) << m.pos[j];
    }
    uint64_t xs, zs, kv;
    unsigned c = 0;
    if (MODE == COL_FULL) {
        xs = x;
        zs = z;
        kv = transpose ? ov : ov ^ (x & M);
        c = transpose ? 0u : (unsigned)__popcll(x & z);
    } else if (MODE == COL_SQUEEZE) {
        xs = (x & ~M) | ov;
        zs = unmap_runs(g, z);
        kv = 0;
        c = (unsigned)__popcll(xs & z);
    } else {
        xs = map_runs(g, 0, g.nruns, x, 0);
        zs = z;
        kv = ov;
    }
    const uint64_t Mv = MODE == COL_SQUEEZE ? 0ull : LOW0 ? M & ~1ull : M;      // what decides whether a vector is kept
    const uint64_t kvv = kv & Mv;
    const int ek = (int)(kv & 1ull);                    // LOW0: the kept half of a vector (FULL, EXPAND)
    const int f0 = __ffsll((long long)~M) - 1;          // LOW0, SQUEEZE: where bit 0 of the output index goes

    // the lane's part of map() and of the kept test, once
    uint64_t mlow[ST_UNROLL];
    unsigned okl = 0;
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const uint64_t low = (uint64_t)(u * ST_THREADS + (int)threadIdx.x) << VB;
        mlow[u] = MODE == COL_FULL ? low : map_runs(g, 0, g.nlow, low, 0);
        if ((low & Mv) == (kvv & ((1ull << SBITS) - 1ull))) okl |= 1u << u;
    }
    const uint64_t Mh = Mv >> SBITS, kvh = kvv >> SBITS;

    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        if ((chunk & Mh) != kvh) {                      // a measured bit above the unit is wrong: nothing of it is kept
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
                if (v < nvec) dst[v] = Q{};
            }
            continue;
        }
        const uint64_t mhigh = MODE == COL_FULL ? chunk << SBITS : map_runs(g, g.nlow, g.nruns, chunk, SBITS);
        Q q[ST_UNROLL];
        cx<T> h[ST_UNROLL][2];                          // LOW0: the halves, loaded one by one
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec && ((okl >> u) & 1u)) {
                const uint64_t a = (mhigh | mlow[u]) ^ xs;          // the source of the vector's first amplitude
                if (!LOW0) {
                    q[u] = reinterpret_cast<const Q*>(src)[a >> VB];
                } else if (MODE == COL_SQUEEZE) {
                    h[u][0] = src[a];
                    h[u][1] = src[a ^ (1ull << f0)];
                } else {
                    h[u][0] = src[MODE == COL_FULL ? a ^ (uint64_t)ek : a];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                Q r = Q{};
                if ((okl >> u) & 1u) {
                    const uint64_t p0 = v << VB;
                    if (!LOW0) {
                        const int swap = VB ? (int)(xs & 1ull) : 0;
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            vec_set(r, e, scaled<T>(vec_get<T>(q[u], e ^ swap), s, p0 | (uint64_t)e, zs, c));
                    } else if (MODE == COL_SQUEEZE) {
                        vec_set(r, 0, scaled<T>(h[u][0], s, p0, zs, c));
                        vec_set(r, 1, scaled<T>(h[u][1], s, p0 | 1ull, zs, c));
                    } else {
                        vec_set(r, ek, scaled<T>(h[u][0], s, p0 | (uint64_t)ek, zs, c));
                    }
                }
                dst[v] = r;
            }
        }
    }
}

// ---- the draw ------------------------------------------------------------------------------------
constexpr int DRAW_THREADS = 256;

__global__ __launch_bounds__(DRAW_THREADS) void measure_draw_kernel(const double* __restrict__ probs, const double* __restrict__ u,
                                                                    const int64_t* __restrict__ forced,
                                                                    const uint64_t* __restrict__ fx,
                                                                    const uint64_t* __restrict__ fz, int k,
                                                                    DqCollapseRec* __restrict__ rec) {
    __shared__ double pre[DRAW_THREADS];                // inclusive sums of the segments
    __shared__ int first[DRAW_THREADS / 64], lastnz[DRAW_THREADS / 64];
    const uint64_t b = blockIdx.x;
    const int64_t count = (int64_t)1 << k;
    const double* p = probs + b * (uint64_t)count;
    const int64_t seg = (count + DRAW_THREADS - 1) / DRAW_THREADS;
    const int64_t lo = (int64_t)threadIdx.x * seg, hi = lo + seg < count ? lo + seg : count;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum = 0.0;
    int64_t mylast = -1;                                // the segment's last entry of non-zero probability
    for (int64_t i = lo; i < hi; ++i) {
        const double v = p[i];
        sum += v;
        if (v > 0.0) mylast = i;
    }
    pre[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int t = 0; t < DRAW_THREADS; ++t) {
            run += pre[t];
            pre[t] = run;
        }
    }
    __syncthreads();
    const double total = pre[DRAW_THREADS - 1];
    const double r = (u ? u[b] : 0.0) * total;
    const unsigned long long nz = __ballot(mylast >= 0);
    const unsigned long long above = __ballot(pre[threadIdx.x] > r) & nz;
    if (lane == 0) {
        first[wave] = above ? wave * 64 + __ffsll((long long)above) - 1 : DRAW_THREADS;
        lastnz[wave] = nz ? wave * 64 + 63 - __clzll((long long)nz) : -1;
    }
    __syncthreads();
    int pick = DRAW_THREADS, tail = -1;
    for (int w = 0; w < DRAW_THREADS / 64; ++w) {
        pick = first[w] < pick ? first[w] : pick;
        tail = lastnz[w] > tail ? lastnz[w] : tail;
    }
    if (pick == DRAW_THREADS) pick = tail;              // at or beyond the last sum: the last segment that holds anything
    const int64_t want = forced ? forced[b] : -1;
    if ((int)threadIdx.x != (want >= 0 || pick < 0 ? 0 : pick)) return;
    int64_t o = 0;
    double po = 0.0;
    if (want >= 0) {                                    // a forced outcome, cut to k bits; beyond them it has probability 0
        o = want & (count - 1);
        po = want < count ? p[o] : 0.0;
    } else if (pick >= 0) {
        double run = threadIdx.x ? pre[threadIdx.x - 1] : 0.0;
        o = mylast;
        for (int64_t i = lo; i < hi; ++i) {
            const double v = p[i];
            run += v;
            if (v > 0.0 && run > r) {
                o = i;
                break;
            }
        }
        po = p[o];
    }
    const bool live = po > 0.0 && total > 0.0;
    DqCollapseRec out;
    out.outcome = o;
    out.xmask = fx ? fx[o] : 0ull;
    out.zmask = fz ? fz[o] : 0ull;
    out.scale = live ? 1.0 / sqrt(po) : 0.0;
    out.prob = live ? po / total : 0.0;
    rec[b] = out;
}

// ---- host side -----------------------------------------------------------------------------------
// The runs of consecutive kept positions, low to high: `deposit` maps the compact index to the full one (src = compact),
// otherwise the full index to the compact one (src = full).  Split at `sbits` of the source side, the low runs first.
void plan_runs(uint64_t kept, int n, int sbits, bool deposit, Gather* g) {
    *g = Gather{};
    struct Run { int src, len, dst; };
    Run low[ST_MAX_RUNS], high[ST_MAX_RUNS];
    int nl = 0, nh = 0, compact = 0;
    for (int f = 0; f < n;) {
        if (!((kept >> f) & 1ull)) { ++f; continue; }
        int e = f;
        while (e + 1 < n && ((kept >> (e + 1)) & 1ull)) ++e;
        const int len = e - f + 1;
        const Run r = deposit ? Run{compact, len, f} : Run{f, len, compact};
        if (r.src < sbits && r.src + r.len > sbits) {
            const int ll = sbits - r.src;
            low[nl++] = Run{r.src, ll, r.dst};
            high[nh++] = Run{sbits, r.len - ll, r.dst + ll};
        } else if (r.src < sbits) {
            low[nl++] = r;
        } else {
            high[nh++] = r;
        }
        compact += len;
        f = e + 1;
    }
    g->nlow = nl;
    g->nruns = nl + nh;
    for (int r = 0; r < nl + nh; ++r) {
        const Run& x = r < nl ? low[r] : high[r - nl];
        g->src[r] = (uint8_t)x.src;
        g->len[r] = (uint8_t)x.len;
        g->dst[r] = (uint8_t)x.dst;
    }
}

template <typename T>
int collapse_impl(const void* in, void* out, const void* rec, int n, const int* bits, int k, int layout, int transpose,
                  int may_flip, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_collapse";
    if (!in || !out || !rec) {
        set_error("%s: null pointer", what);
        return DQ_ERR_ARG;
    }
    if (misaligned(in) || misaligned(out) || (reinterpret_cast<uintptr_t>(rec) & 7)) {
        set_error("%s: in and out must be 16-byte aligned, rec 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (k < 1 || k > COL_MAX_K) {
        set_error("%s: k=%d outside [1, %d] (a full-register measurement is dq_sample_*'s)", what, k, COL_MAX_K);
        return DQ_ERR_ARG;
    }
    if (n < 1 || n > 40) {
        set_error("%s: n=%d out of range [1, 40]", what, n);
        return DQ_ERR_ARG;
    }
    if (int rc = validate_bits(n, bits, k, nullptr, 0)) return rc;
    if (int rc = check_batch(what, batch)) return rc;
    if (layout != DQ_COLLAPSE_FULL && layout != DQ_COLLAPSE_DROP) {
        set_error("%s: layout=%d is neither DQ_COLLAPSE_FULL nor DQ_COLLAPSE_DROP", what, layout);
        return DQ_ERR_ARG;
    }
    if (layout == DQ_COLLAPSE_DROP && k == n) {
        set_error("%s: DQ_COLLAPSE_DROP of all %d wires leaves no state (k < n is needed)", what, n);
        return DQ_ERR_ARG;
    }
    const int mode = layout == DQ_COLLAPSE_FULL ? COL_FULL : transpose ? COL_EXPAND : COL_SQUEEZE;
    const int nin = mode == COL_EXPAND ? n - k : n, nout = mode == COL_SQUEEZE ? n - k : n;
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), o = reinterpret_cast<uintptr_t>(out);
    const uint64_t bytes_in = ((uint64_t)batch << nin) * sizeof(cx<T>), bytes_out = ((uint64_t)batch << nout) * sizeof(cx<T>);
    if (a == o && mode == COL_FULL) {
        if (may_flip) {
            set_error("%s: in place with an x table (a lane reads where another writes): out of place only", what);
            return DQ_ERR_ARG;
        }
    } else if (a < o + bytes_out && o < a + bytes_in) {
        set_error("%s: in and out overlap%s", what, mode == COL_FULL ? " without being equal" : " (out of place only)");
        return DQ_ERR_ARG;
    }
    const uintptr_t r = reinterpret_cast<uintptr_t>(rec);
    if (r < o + bytes_out && o < r + (uint64_t)batch * sizeof(DqCollapseRec)) {
        set_error("%s: rec and out overlap", what);
        return DQ_ERR_ARG;
    }
    Measured m{};
    m.k = k;
    uint64_t mask = 0;
    for (int j = 0; j < k; ++j) {
        m.pos[j] = (uint8_t)bits[j];
        mask |= 1ull << bits[j];
    }
    Gather g{};
    if (mode != COL_FULL) plan_runs(~mask & ((1ull << n) - 1ull), n, ST_UNIT_BITS + (C128 ? 0 : 1), mode == COL_SQUEEZE, &g);
    const uint64_t nvec = vectors_of(nout, C128);
    const dim3 grid(blocks_of(nvec), (unsigned)batch);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    const DqCollapseRec* pr = static_cast<const DqCollapseRec*>(rec);
    hipStream_t s = as_stream(stream);
    const bool low0 = !C128 && (mask & 1ull);
#define DQ_COLLAPSE(MODE, LOW0) \
    hipLaunchKernelGGL((collapse_kernel<T, MODE, LOW0>), grid, dim3(ST_THREADS), 0, s, pi, po, pr, m, g, n, transpose ? 1 : 0, \
                       may_flip ? 1 : 0, units_of(nvec))
    if constexpr (C128) {
        if (mode == COL_FULL) DQ_COLLAPSE(COL_FULL, false);
        else if (mode == COL_SQUEEZE) DQ_COLLAPSE(COL_SQUEEZE, false);
        else DQ_COLLAPSE(COL_EXPAND, false);
    } else {
        if (mode == COL_FULL && low0) DQ_COLLAPSE(COL_FULL, true);
        else if (mode == COL_FULL) DQ_COLLAPSE(COL_FULL, false);
        else if (mode == COL_SQUEEZE && low0) DQ_COLLAPSE(COL_SQUEEZE, true);
        else if (mode == COL_SQUEEZE) DQ_COLLAPSE(COL_SQUEEZE, false);
        else if (low0) DQ_COLLAPSE(COL_EXPAND, true);
        else DQ_COLLAPSE(COL_EXPAND, false);
    }
#undef DQ_COLLAPSE
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int dq_collapse_rec_layout(int* out, int max) {
    const int v[] = {(int)sizeof(DqCollapseRec), (int)offsetof(DqCollapseRec, outcome), (int)offsetof(DqCollapseRec, xmask),
                     (int)offsetof(DqCollapseRec, zmask), (int)offsetof(DqCollapseRec, scale), (int)offsetof(DqCollapseRec, prob)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < max && out; ++i) out[i] = v[i];
    return n;
}

extern "C" int dq_measure_draw(const double* probs, const double* u, const int64_t* forced, const uint64_t* fx, const uint64_t* fz,
                               int k, int64_t batch, void* rec, dq_stream_t stream) {
    const char* what = "dq_measure_draw";
    if (!probs || !rec || (!u && !forced)) {
        dq::set_error("%s: null pointer (probs, rec, or both of u and forced)", what);
        return DQ_ERR_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(forced) |
         reinterpret_cast<uintptr_t>(fx) | reinterpret_cast<uintptr_t>(fz) | reinterpret_cast<uintptr_t>(rec)) & 7) {
        dq::set_error("%s: every pointer must be 8-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (k < 1 || k > dq::COL_MAX_K) {
        dq::set_error("%s: k=%d outside [1, %d] (a full-register measurement is dq_sample_*'s)", what, k, dq::COL_MAX_K);
        return DQ_ERR_ARG;
    }
    if (int rc = dq::check_batch(what, batch)) return rc;
    hipLaunchKernelGGL(dq::measure_draw_kernel, dim3((unsigned)batch), dim3(dq::DRAW_THREADS), 0, dq::as_stream(stream), probs, u,
                       forced, fx, fz, k, static_cast<DqCollapseRec*>(rec));
    return dq::check_launch(what);
}

extern "C" int dq_apply_collapse_c64(const void* in, void* out, const void* rec, int n, const int* bits, int k, int layout,
                                     int transpose, int may_flip, int64_t batch, dq_stream_t stream) {
    return dq::collapse_impl<float>(in, out, rec, n, bits, k, layout, transpose, may_flip, batch, stream);
}
extern "C" int dq_apply_collapse_c128(const void* in, void* out, const void* rec, int n, const int* bits, int k, int layout,
                                      int transpose, int may_flip, int64_t batch, dq_stream_t stream) {
    return dq::collapse_impl<double>(in, out, rec, n, bits, k, layout, transpose, may_flip, batch, stream);
}
