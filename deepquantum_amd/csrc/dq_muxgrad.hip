// The binned cross reduction of the multiplexed one-qubit gates (dq_mux.hip): one complex number per sample AND per value
// of the k select bits -- what the gradient with respect to the 2^k angles of a multiplexed rotation is made of.
//
//     sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j)            (bits[0] = the most significant bit of s)
//     dq_mux_cross : out[b, s] = sum over the amplitudes i with sub(i) = s of conj(bra[b, i]) (G ket_b)[i]
// inside the controls, G = the one-qubit Pauli `axis` (I, X, Y, Z) on bit `target`.  The select bits, the controls and the
// target are disjoint, so both ends of a pair i0, i1 = i0 | 1 << target lie in the same bin, inside the controls or not.
//
// Safety.  No address depends on data: the bin of an amplitude is a function of its index alone.  s < 2^k by
// construction, and every workspace index is (sample, workgroup of the bin group, s).
//
// Geometry.  That of dq_mux.hip: the item is the pair (a pair of vectors; complex64 with target 0, INNER: the one vector
// that holds the pair), all bin arithmetic is done on the (n - 1)-bit pair index, and a unit is 2^ST_UNIT_BITS items =
// 2^P pairs, P = ST_UNIT_BITS + (1 for complex64 unless INNER).  dq_stream.hpp's Gather splits sub() at the unit:
//   * the low part depends on the lane slot (u, e) alone -- slot (u, e) of lane t holds pair (u * ST_THREADS + t) << PB | e
//     of every unit -- so a slot stays in ONE low bin for the whole loop and gets its own accumulator, in double;
//   * the high part depends on the unit.  Units are enumerated as (hv, r): hv over the kh select bits at or above the
//     unit, r over the unit-index bits that are neither select bits nor controls, both deposited into the unit number
//     with the high control bits set.  A unit whose high control bits are not all set is never formed, hence never read.
// A task is (hv, g): workgroup g of the G that share the bin group hv strides over r = g, g + G, ..; G is a power of
// two, at most ST_BLOCKS >> kh and at most 2^19 >> k (the partial sums of a sample stay within 8 MiB).  A workgroup
// takes the tasks blockIdx.x, blockIdx.x + gridDim.x, ..
//
// Reduction, per task, every sum in a fixed order (no atomics: two calls return the same bits, bin by bin):
//   1. in the wave, an xor butterfly over the lane bits that are not select bits (a + b = b + a: both lanes hold the same
//      bits afterwards);
//   2. all 2^P slot sums go to LDS (16 / 32 KiB); for each of the 2^kl low bins one lane adds, in ascending order, the
//      slots of its bin whose free lane bits are 0 -- at most 32 terms (2 wave bits, 2 unroll bits, the element bit) --
//      and writes the task's partial sum ws[b, g, s], s = high | low in final positions; G = 1: out[b, s] directly;
//   3. G > 1: mux_cross_finish_kernel, one wave per (b, s): lane l adds ws[b, g, s] for g = l, l + 64, .., then the
//      butterfly of dq_stream.hpp.
// bra == ket loads each pair once.
#include "dq_stream.hpp"

namespace dq {

namespace {

constexpr int MXC_I = 0, MXC_X = 1, MXC_Y = 2, MXC_Z = 3;
constexpr unsigned MXC_MAX_GRID = ST_BLOCKS;            // workgroups per sample striding over the tasks
constexpr int MXC_WS_BITS = 19;                         // G << k <= 2^19 partial sums per sample

struct MuxCross {
    Gather g;                                           // over pair space
    int tv;                                             // the target's bit over vector indices (unused when INNER)
    int axis, k;
    uint64_t lowsel;                                    // the select positions below the unit, over its P pair bits
    uint64_t usel, ufree, uctl;                         // over unit-index bits: select, neither select nor control, control
    int kh, rb, gb;                                     // popc(usel), popc(ufree), log2(G)
};

// the bits of v, least significant first, put at the set positions of mask, lowest first
__host__ __device__ __forceinline__ uint64_t deposit(uint64_t v, uint64_t mask) {
    uint64_t r = 0;
    for (; mask; mask &= mask - 1ull) {
        if (v & 1ull) r |= mask & (~mask + 1ull);
        v >>= 1;
    }
    return r;
}

// (re, im) += conj(a0) (G v)_0 + conj(a1) (G v)_1, in double
template <typename V> __device__ __forceinline__ void mux_cross_add(V a0, V a1, V v0, V v1, int axis, double& re, double& im) {
    const double a0r = (double)a0.x, a0i = (double)a0.y, a1r = (double)a1.x, a1i = (double)a1.y;
    const double v0r = (double)v0.x, v0i = (double)v0.y, v1r = (double)v1.x, v1i = (double)v1.y;
    double w0r, w0i, w1r, w1i;                          // G v at both ends
    if (axis == MXC_X) {
        w0r = v1r; w0i = v1i; w1r = v0r; w1i = v0i;
    } else if (axis == MXC_Y) {                         // (Y v)_0 = -i v_1, (Y v)_1 = i v_0
        w0r = v1i; w0i = -v1r; w1r = -v0i; w1i = v0r;
    } else if (axis == MXC_Z) {
        w0r = v0r; w0i = v0i; w1r = -v1r; w1i = -v1i;
    } else {
        w0r = v0r; w0i = v0i; w1r = v1r; w1i = v1i;
    }
    re = fma(a0r, w0r, fma(a0i, w0i, re));
    im = fma(a0r, w0i, fma(-a0i, w0r, im));
    re = fma(a1r, w1r, fma(a1i, w1i, re));
    im = fma(a1r, w1i, fma(-a1i, w1r, im));
}

template <typename T, bool SAME, bool INNER>
__global__ __launch_bounds__(ST_THREADS) void mux_cross_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                               MuxCross p, int n, uint64_t items, double* __restrict__ ws,
                                                               double* __restrict__ out) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int PV = INNER ? 1 : VEC;                 // pairs of an item
    constexpr int PB = PV == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + PB;            // pairs of a unit
    __shared__ double sh[1 << SBITS][2];
    const uint64_t b = blockIdx.y;
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    LaneLow<PV> ll;
    lane_low<PV>(p.g, SBITS, ll);
    const int kl = __popcll(p.lowsel);
    // the slot bits a lane of step 2 adds over: wave and unroll bits and the element bit, where they are no select bits
    const uint64_t redmask = ~p.lowsel & ((((1ull << SBITS) - 1ull) & ~((64ull << PB) - 1ull)) | (uint64_t)PB);
    const uint64_t nred = 1ull << __popcll(redmask);
    const uint64_t tasks = 1ull << (p.kh + p.gb), G = 1ull << p.gb, nr = 1ull << p.rb;
    for (uint64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
        const uint64_t hv = task >> p.gb, g = task & (G - 1ull);
        const uint64_t ubase = deposit(hv, p.usel) | p.uctl;
        double re[ST_UNROLL][PV], im[ST_UNROLL][PV];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < PV; ++e) re[u][e] = im[u][e] = 0.0;
        }
        for (uint64_t r = g; r < nr; r += G) {
            const uint64_t unit = ubase | deposit(r, p.ufree);
            const uint64_t i0 = (unit << ST_UNIT_BITS) + threadIdx.x;
            Q ka[ST_UNROLL], kb[ST_UNROLL], ba[ST_UNROLL], bb[ST_UNROLL];       // (kb, bb: !INNER only; ba, bb: !SAME only)
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
                if (it < items) {
                    const uint64_t va = INNER ? it : insert_zero(it, p.tv), vb = va | (1ull << p.tv);
                    ka[u] = pk[va];
                    if constexpr (!INNER) kb[u] = pk[vb];
                    if constexpr (!SAME) ba[u] = pb[va];
                    if constexpr (!SAME && !INNER) bb[u] = pb[vb];
                }
            }
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t it = i0 + (uint64_t)(u * ST_THREADS);
                if (it < items) {
#pragma unroll
                    for (int e = 0; e < PV; ++e) {
                        if ((ll.ok >> (u * PV + e)) & 1u) {
                            if constexpr (INNER)
                                mux_cross_add(vec_get<T>(SAME ? ka[u] : ba[u], 0), vec_get<T>(SAME ? ka[u] : ba[u], 1),
                                              vec_get<T>(ka[u], 0), vec_get<T>(ka[u], 1), p.axis, re[u][e], im[u][e]);
                            else
                                mux_cross_add(vec_get<T>(SAME ? ka[u] : ba[u], e), vec_get<T>(SAME ? kb[u] : bb[u], e),
                                              vec_get<T>(ka[u], e), vec_get<T>(kb[u], e), p.axis, re[u][e], im[u][e]);
                        }
                    }
                }
            }
        }
        // 1. the lanes of a wave that share a bin
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (!((p.lowsel >> (j + PB)) & 1ull)) {
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
                    for (int e = 0; e < PV; ++e) {
                        re[u][e] += __shfl_xor(re[u][e], 1 << j, 64);
                        im[u][e] += __shfl_xor(im[u][e], 1 << j, 64);
                    }
                }
            }
        }
        // 2. the slots of a bin, through LDS
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < PV; ++e) {
                const int slot = ((u * ST_THREADS + (int)threadIdx.x) << PB) | e;
                sh[slot][0] = re[u][e];
                sh[slot][1] = im[u][e];
            }
        }
        __syncthreads();
        const uint64_t high = chunk_high(p.g, SBITS, ubase);
        for (uint64_t lb = threadIdx.x; lb < (1ull << kl); lb += ST_THREADS) {
            const uint64_t base = deposit(lb, p.lowsel);
            double sr = 0.0, si = 0.0;
            for (uint64_t j = 0; j < nred; ++j) {
                const uint64_t slot = base | deposit(j, redmask);
                sr += sh[slot][0];
                si += sh[slot][1];
            }
            uint64_t s = high;
            for (int q = 0; q < p.g.nlow; ++q) s |= ((base >> p.g.src[q]) & ((1ull << p.g.len[q]) - 1ull)) << p.g.dst[q];
            double* dst = p.gb ? ws + ((((b * G + g) << p.k) | s) << 1) : out + (((b << p.k) | s) << 1);
            dst[0] = sr;
            dst[1] = si;
        }
        __syncthreads();                                // (the next task writes the slots again)
    }
}

// out[b, s] = the sum over g of ws[b, g, s]; one wave per (b, s)
__global__ __launch_bounds__(ST_THREADS) void mux_cross_finish_kernel(const double* __restrict__ ws, int k, unsigned G,
                                                                      uint64_t bins, double* __restrict__ out) {
    const uint64_t bin = (uint64_t)blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);        // b << k | s
    if (bin >= bins) return;                            // (the whole wave)
    const uint64_t b = bin >> k, s = bin & ((1ull << k) - 1ull);
    double re = 0.0, im = 0.0;
    for (unsigned g = threadIdx.x & 63; g < G; g += 64) {
        const double* part = ws + ((((b * G + g) << k) | s) << 1);
        re += part[0];
        im += part[1];
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if ((threadIdx.x & 63) == 0) {
        out[2 * bin] = re;
        out[2 * bin + 1] = im;
    }
}

// G of the sizing function: an upper bound of every plan's G for (n, k), whatever the positions
unsigned mux_cross_gmax(int n, int k) {
    const int ub = n - 1 - ST_UNIT_BITS;
    uint64_t G = ub <= 0 ? 1ull : (ub >= 11 ? (uint64_t)ST_BLOCKS : 1ull << ub);
    while (G > 1 && (k >= MXC_WS_BITS || (G << k) > (1ull << MXC_WS_BITS))) G >>= 1;
    return (unsigned)G;
}

int64_t mux_cross_ws_bytes(int n, int k, int64_t batch) {
    const unsigned G = mux_cross_gmax(n, k);
    return G > 1 ? (batch * (int64_t)G << k) * 2 * (int64_t)sizeof(double) : 16;
}

// Validates everything, before any HIP call, moves the select bits and the controls to pair space and enumerates the units.
template <typename T>
int plan_mux_cross(const char* what, const void* bra, const void* ket, int axis, int n, int target, const int* bits, int k,
                   const int* controls, int nc, int64_t batch, const double* out, const void* ws, int64_t ws_bytes, MuxCross* p,
                   bool* inner) {
    constexpr bool C128 = sizeof(T) == 8;
    if (n < 2 || n > 40) {
        set_error("%s: n=%d out of range [2, 40]", what, n);
        return DQ_ERR_ARG;
    }
    if (int rc = check_batch(what, batch)) return rc;
    if (k < 1 || k > n - 1) {
        set_error("%s: k=%d outside [1, n - 1] (n=%d)", what, k, n);
        return DQ_ERR_ARG;
    }
    if (axis < MXC_I || axis > MXC_Z) {
        set_error("%s: axis=%d is none of DQ_MUX_AXIS_I / X / Y / Z", what, axis);
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
    if (int rc = check_cross_buffers(what, bra, ket, nullptr, false, out, ws)) return rc;
    const int64_t need = mux_cross_ws_bytes(n, k, batch);
    if (ws_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (%s_ws_bytes)", what, (long long)ws_bytes, (long long)need, what);
        return DQ_ERR_ARG;
    }
    *inner = !C128 && target == 0;
    bool ident;
    if (int rc = plan_gather(what, n - 1, pbits, k, pctl, nc, batch, C128 || *inner, &p->g, &ident)) return rc;
    p->tv = *inner ? 0 : target - (C128 ? 0 : 1);
    p->axis = axis;
    p->k = k;
    const int sbits = ST_UNIT_BITS + (C128 || *inner ? 0 : 1);
    const int ub = n - 1 > sbits ? n - 1 - sbits : 0;   // bits of a unit's index
    uint64_t sel = 0;
    for (int j = 0; j < k; ++j) sel |= 1ull << pbits[j];
    const uint64_t umask = (1ull << ub) - 1ull;
    p->lowsel = sel & ((1ull << sbits) - 1ull);
    p->usel = (sel >> sbits) & umask;
    p->uctl = (p->g.cmask >> sbits) & umask;
    p->ufree = umask & ~(p->usel | p->uctl);
    p->kh = __builtin_popcountll(p->usel);
    p->rb = __builtin_popcountll(p->ufree);
    int gb = p->rb;                                     // G = 2^gb workgroups per bin group
    const int most = p->kh >= 11 ? 0 : 11 - p->kh;      // (ST_BLOCKS = 2^11)
    if (gb > most) gb = most;
    while (gb > 0 && (k >= MXC_WS_BITS || gb + k > MXC_WS_BITS)) --gb;
    p->gb = gb;
    return DQ_OK;
}

template <typename T>
int mux_cross_impl(const void* bra, const void* ket, int axis, int n, int target, const int* bits, int k, const int* controls,
                   int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_mux_cross";
    MuxCross p;
    bool inner;
    if (int rc = plan_mux_cross<T>(what, bra, ket, axis, n, target, bits, k, controls, nc, batch, out, ws, ws_bytes, &p, &inner))
        return rc;
    const uint64_t nvec = vectors_of(n, C128);
    const uint64_t items = inner ? nvec : nvec >> 1;
    const uint64_t tasks = 1ull << (p.kh + p.gb);
    const dim3 grid((unsigned)(tasks < MXC_MAX_GRID ? tasks : MXC_MAX_GRID), (unsigned)batch);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    const bool same = bra == ket;
#define DQ_MUX_CROSS(SAME, INNER) \
    hipLaunchKernelGGL((mux_cross_kernel<T, SAME, INNER>), grid, dim3(ST_THREADS), 0, s, pb, pk, p, n, items, part, out)
    if constexpr (C128) {
        if (same) DQ_MUX_CROSS(true, false);
        else DQ_MUX_CROSS(false, false);
    } else {
        if (same && inner) DQ_MUX_CROSS(true, true);
        else if (same) DQ_MUX_CROSS(true, false);
        else if (inner) DQ_MUX_CROSS(false, true);
        else DQ_MUX_CROSS(false, false);
    }
#undef DQ_MUX_CROSS
    if (p.gb == 0) return check_launch(what);
    if (int rc = check_launch(what)) return rc;
    const uint64_t bins = (uint64_t)batch << k;
    hipLaunchKernelGGL(mux_cross_finish_kernel, dim3((unsigned)((bins + ST_THREADS / 64 - 1) / (ST_THREADS / 64))), dim3(ST_THREADS), 0,
                       s, part, k, 1u << p.gb, bins, out);
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int64_t dq_mux_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross, int k) {
    (void)is_c128;      // both precisions accumulate in double
    (void)cross;        // bra != ket reads twice as much and writes the same partial sums
    if (n < 2 || n > 40 || batch < 1 || batch > 65535 || k < 1 || k > n - 1) return -1;
    return dq::mux_cross_ws_bytes(n, k, batch);
}

extern "C" int dq_mux_cross_c64(const void* bra, const void* ket, int axis, int n, int target, const int* bits, int k,
                                const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                dq_stream_t stream) {
    return dq::mux_cross_impl<float>(bra, ket, axis, n, target, bits, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_mux_cross_c128(const void* bra, const void* ket, int axis, int n, int target, const int* bits, int k,
                                 const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                 dq_stream_t stream) {
    return dq::mux_cross_impl<double>(bra, ket, axis, n, target, bits, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
