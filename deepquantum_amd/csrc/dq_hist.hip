// The distribution of a tabulated cost: a reduction binned through a table lookup, and the streaming pass that is its
// cotangent.
//
//     sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j)            (bits[0] = the table index's most significant bit)
//     dq_cost_hist    : out[b, v] = sum over i inside the controls with bin[sub(i)] = v of conj(bra[b, i]) ket[b, i]
//     dq_apply_binned : out[b, i] = g[b, bin[sub(i)]] * in[b, i] inside the controls, 0 outside (the DQ_COST_SCALE
//                       convention: the cotangent of a sum that leaves those amplitudes out)
// `bin` is a table of 2^k uint16 entries shared by the batch, every entry < V <= HS_MAX_BINS = 1024.  uint16 because the
// table is streamed beside the state when bits = n-1 .. 0: two bytes per amplitude are a quarter of a complex64 state's
// traffic, an int32 table would be half of it.
//
// Safety.  The bin of an amplitude is data, so it is clamped to V - 1 before it indexes LDS (the Python side refuses a
// table with an entry >= V when it builds it); table indices are sub(i) < 2^k by construction and every workspace index
// is (sample, workgroup, v < V).
//
// Geometry and gather.  dq_stream.hpp's: a lane moves 16 bytes per load, a workgroup iteration a unit of 1024 vectors;
// sub() is split at the unit into a part per lane slot (kept across the loop) and a part per unit (scalar).  A lane has
// S = 8 (complex64) or 4 (complex128) slots (u, e).
//
// Histogram.  The bins live in LDS, in double, one private copy per wave and within a wave C = 2^cbits copies, lane l
// using copy l mod C: entry (v << cbits | copy) of the wave's region.  C is the largest power of two <= 64 that keeps
// the workgroup's 4 * C * V * 16 bytes within 32 KiB (V = 2: 64 copies, a lane of its own each; V = 37: 8; V = 200: 2),
// and 1 beyond that (V = 1024: 64 KiB, the whole of what a launch may ask for without an attribute).
//   * Runs in registers.  While the unit part of sub() does not change, a slot stays in one bin: the lane adds its
//     products in double in a register per slot and touches LDS only when the unit part changes (and at the end).
//     Before it does, slots that differ only in index bits outside `bits` and the controls are added in registers, and
//     lanes that differ only in such bits are added with an xor butterfly (a + b = b + a: both hold the same bits); one
//     lane of each class goes on.  With bits = n-1 .. 0 every amplitude has a bin of its own and every unit is flushed.
//   * Fixed order, no atomics.  A flush takes the slots in order; for a slot, the lanes of a wave that hit the same entry
//     are found with one ballot per bit of the bin (peers), ranked by lane number, and added in rounds: in round r the
//     lanes of rank r read, add and write their entry -- no two of them share one.  LDS operations of a wave execute in
//     order, so round r + 1 reads what round r wrote.  The sum of an entry is therefore ordered by (flush, slot, lane):
//     a function of the data and the geometry alone.  The price is the ballots (log2 V per slot) and the rounds (the
//     largest number of lanes of a copy in one bin); DESIGN.md section 4.23 has what that costs against dq_cost_cross.
//   * The workgroup's partial sums: thread v adds entry v of wave 0..3, copies 0..C-1 in that order, into
//     ws[b, workgroup, v]; hist_finish_kernel adds the workgroups of (b, v), strided by 64 over a wave's lanes, then the
//     butterfly of dq_stream.hpp.  At most 2^19 / V workgroups per sample: the partial sums stay within 8 MiB a sample.
// bra == ket loads the state once and never forms an imaginary part: it is +0.
#include "dq_stream.hpp"

namespace dq {

namespace {

using bin_t = uint16_t;

constexpr int HS_MAX_BINS = 1024;
constexpr int HS_WAVES = ST_THREADS / 64;
constexpr int HS_LDS_BUDGET = 32 << 10;                 // bytes of bins per workgroup that the copies may fill
constexpr int HS_WS_BITS = 19;                          // workgroups * V <= 2^19 partial sums per sample

// The VEC table entries beside vector v of the state (sub(i) = i), in one load.
template <typename E, int VEC> __device__ __forceinline__ void load_beside(const E* tab, uint64_t v, E (&d)[VEC]) {
    struct alignas(VEC * sizeof(E)) Row { E e[VEC]; };
    const Row r = reinterpret_cast<const Row*>(tab)[v];
#pragma unroll
    for (int e = 0; e < VEC; ++e) d[e] = r.e[e];
}

// log2 of the copies of a wave's bins
int hist_copy_bits(int V) {
    int cb = 6;
    while (cb > 0 && (HS_WAVES * V * 16 << cb) > HS_LDS_BUDGET) --cb;
    return cb;
}

unsigned hist_blocks(uint64_t nvec, int V) {
    const unsigned nb = blocks_of(nvec), cap = (1u << HS_WS_BITS) / (unsigned)V;
    return nb < cap ? nb : cap;
}

int64_t hist_ws_bytes(int n, int64_t batch, bool is_c128, int V) {
    return batch * (int64_t)hist_blocks(vectors_of(n, is_c128), V) * V * 2 * (int64_t)sizeof(double);
}

// The index bits below the unit that are neither table bits nor controls: amplitudes that differ only there share a bin.
uint64_t hist_free_low(const int* bits, int k, uint64_t cmask, int sbits) {
    uint64_t sel = 0;
    for (int j = 0; j < k; ++j) sel |= 1ull << bits[j];
    return ~sel & ~cmask & ((1ull << sbits) - 1ull);
}

// One flush of a lane's S slot sums into its wave's bins (see the header of this file).  `red`: hist_free_low.
template <int S, int VB, bool SAME, bool IDENT>
__device__ __forceinline__ void hist_flush(double (&are)[S], double (&aim)[S], const unsigned (&cur)[S], unsigned valid,
                                           uint64_t red, uint64_t grp, unsigned copy, int cbits, int vbits,
                                           volatile double* mine) {
    constexpr int VEC = 1 << VB;
    const unsigned lane = threadIdx.x & 63u;
    if (!IDENT) {
        // slots that share a bin: the element bit, then the two unroll bits
        if (VB && (red & 1ull)) {
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                are[u * VEC] += are[u * VEC + VEC - 1];
                if (!SAME) aim[u * VEC] += aim[u * VEC + VEC - 1];
                if (VB) valid &= ~(1u << (u * VEC + 1));
            }
        }
#pragma unroll
        for (int ub = 0; ub < 2; ++ub) {
            if ((red >> (VB + 8 + ub)) & 1ull) {
#pragma unroll
                for (int u = 0; u < ST_UNROLL; ++u) {
                    if (u & (1 << ub)) continue;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int lo = u * VEC + e, hi = (u | (1 << ub)) * VEC + e;
                        are[lo] += are[hi];
                        if (!SAME) aim[lo] += aim[hi];
                        valid &= ~(1u << hi);
                    }
                }
            }
        }
        // lanes that share a bin
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if ((red >> (j + VB)) & 1ull) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    are[s] += __shfl_xor(are[s], 1 << j, 64);
                    if (!SAME) aim[s] += __shfl_xor(aim[s], 1 << j, 64);
                }
                if ((lane >> j) & 1u) valid = 0;
            }
        }
    }
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool act = (valid >> s) & 1u;
        const unsigned v = cur[s];
        uint64_t peers = grp & __ballot(act);
        for (int j = 0; j < vbits; ++j) {
            const bool bit = (v >> j) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned rank = (unsigned)__popcll(peers & below);
        volatile double* entry = mine + 2 * ((v << cbits) | copy);
        for (unsigned r = 0; __ballot(act && rank >= r) != 0ull; ++r) {
            if (act && rank == r) {
                entry[0] = entry[0] + are[s];
                if (!SAME) entry[1] = entry[1] + aim[s];
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ws[b, blockIdx.x, v] = this workgroup's part of out[b, v]
template <typename T, bool SAME, bool IDENT>
__global__ __launch_bounds__(ST_THREADS) void cost_hist_kernel(const cx<T>* __restrict__ bra, const cx<T>* __restrict__ ket,
                                                               const bin_t* __restrict__ bin, Gather g, uint64_t red, int n,
                                                               uint64_t nchunks, int V, int cbits, int vbits,
                                                               double* __restrict__ ws) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;
    constexpr int S = ST_UNROLL * VEC;
    extern __shared__ double hs_lds[];                  // [wave][V << cbits][2]
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* pb = reinterpret_cast<const Q*>(bra + (b << n));
    const Q* pk = reinterpret_cast<const Q*>(ket + (b << n));
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned per_wave = (unsigned)V << cbits, copy = lane & ((1u << cbits) - 1u);
    const uint64_t grp = cbits == 6 ? 1ull << lane : (~0ull / ((1ull << (1u << cbits)) - 1ull)) << copy;
    volatile double* mine = hs_lds + 2 * (size_t)(wave * per_wave);
    for (unsigned i = lane; i < 2 * per_wave; i += 64) mine[i] = 0.0;
    LaneLow<VEC> ll;
    if (!IDENT) lane_low<VEC>(g, SBITS, ll);
    const uint64_t ch = g.cmask >> SBITS;
    double are[S], aim[S];
    unsigned cur[S], valid = 0;
    bool have = false;
    uint64_t prev = 0;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (!IDENT && (chunk & ch) != ch) continue;     // (uniform over the workgroup)
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        const uint64_t high = IDENT ? 0 : chunk_high(g, SBITS, chunk);
        const bool fresh = IDENT || !have || high != prev;      // (uniform) the slots move to other bins
        Q qk[ST_UNROLL], qb[ST_UNROLL];
        bin_t t[ST_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                qk[u] = pk[v];
                if (!SAME) qb[u] = pb[v];
                if (IDENT) {
                    load_beside<bin_t, VEC>(bin, v, t[u]);
                } else if (fresh) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) t[u][e] = bin[high | ll.sub[u][e]];
                }
            }
        }
        if (fresh) {
            if (have) hist_flush<S, VB, SAME, IDENT>(are, aim, cur, valid, red, grp, copy, cbits, vbits, mine);
            valid = 0;
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int s = u * VEC + e;
                    are[s] = aim[s] = 0.0;
                    const bool ok = v < nvec && (IDENT || ((ll.ok >> s) & 1u));
                    const unsigned tv = ok ? (unsigned)t[u][e] : 0u;
                    cur[s] = tv < (unsigned)V ? tv : (unsigned)V - 1u;
                    if (ok) valid |= 1u << s;
                }
            }
            have = true;
            prev = high;
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int s = u * VEC + e;
                if ((valid >> s) & 1u) {
                    const cx<T> kk = vec_get<T>(qk[u], e);
                    const double kr = (double)kk.x, ki = (double)kk.y;
                    if (SAME) {
                        are[s] += kr * kr + ki * ki;
                    } else {
                        const cx<T> a = vec_get<T>(qb[u], e);
                        const double ar = (double)a.x, ai = (double)a.y;
                        are[s] += ar * kr + ai * ki;
                        aim[s] += ar * ki - ai * kr;
                    }
                }
            }
        }
    }
    if (have) hist_flush<S, VB, SAME, IDENT>(are, aim, cur, valid, red, grp, copy, cbits, vbits, mine);
    __syncthreads();
    double* part = ws + ((b * gridDim.x + blockIdx.x) * (uint64_t)V) * 2;
    for (unsigned v = threadIdx.x; v < (unsigned)V; v += ST_THREADS) {
        double re = 0.0, im = 0.0;
        for (unsigned w = 0; w < (unsigned)HS_WAVES; ++w) {
            const double* e = hs_lds + 2 * (size_t)(w * per_wave + (v << cbits));
            for (unsigned c = 0; c < (1u << cbits); ++c) {
                re += e[2 * c];
                if (!SAME) im += e[2 * c + 1];
            }
        }
        part[2 * v] = re;
        part[2 * v + 1] = im;
    }
}

// out[b, v] = the sum over the workgroups p of ws[b, p, v]; one wave per (b, v)
__global__ __launch_bounds__(ST_THREADS) void hist_finish_kernel(const double* __restrict__ ws, unsigned nparts, int V,
                                                                 uint64_t bins, double* __restrict__ out) {
    const uint64_t bin = (uint64_t)blockIdx.x * HS_WAVES + (threadIdx.x >> 6);        // b * V + v
    if (bin >= bins) return;                            // (the whole wave)
    const uint64_t b = bin / (uint64_t)V, v = bin % (uint64_t)V;
    double re = 0.0, im = 0.0;
    for (unsigned p = threadIdx.x & 63; p < nparts; p += 64) {
        const double* part = ws + ((b * nparts + p) * (uint64_t)V + v) * 2;
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

// in and out may be the same buffer: no __restrict__ on them
template <typename T, bool IDENT>
__global__ __launch_bounds__(ST_THREADS) void apply_binned_kernel(const cx<T>* in, cx<T>* out, const bin_t* __restrict__ bin,
                                                                  const double* __restrict__ gtab, Gather g, int n,
                                                                  uint64_t nchunks, int V) {
    using Q = typename Vec16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int SBITS = ST_UNIT_BITS + VB;
    extern __shared__ double hs_lds[];                  // g[b]: [V][2]
    const uint64_t b = blockIdx.y;
    const uint64_t nvec = 1ull << (n - VB);
    const Q* src = reinterpret_cast<const Q*>(in + (b << n));
    Q* dst = reinterpret_cast<Q*>(out + (b << n));
    for (unsigned i = threadIdx.x; i < 2u * (unsigned)V; i += ST_THREADS) hs_lds[i] = gtab[b * 2ull * (uint64_t)V + i];
    __syncthreads();
    LaneLow<VEC> ll;
    if (!IDENT) lane_low<VEC>(g, SBITS, ll);
    const uint64_t ch = g.cmask >> SBITS;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t v0 = (chunk << ST_UNIT_BITS) + threadIdx.x;
        if (!IDENT && (chunk & ch) != ch) {             // a high control bit is 0: the whole chunk is zero, unread
#pragma unroll
            for (int u = 0; u < ST_UNROLL; ++u) {
                const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
                if (v < nvec) dst[v] = Q{};
            }
            continue;
        }
        const uint64_t high = IDENT ? 0 : chunk_high(g, SBITS, chunk);
        Q q[ST_UNROLL];
        bin_t t[ST_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                q[u] = src[v];
                if (IDENT) {
                    load_beside<bin_t, VEC>(bin, v, t[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) t[u][e] = bin[high | ll.sub[u][e]];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)(u * ST_THREADS);
            if (v < nvec) {
                Q r{};
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (IDENT || ((ll.ok >> (u * VEC + e)) & 1u)) {
                        const unsigned tv = t[u][e];
                        const double* f = hs_lds + 2 * (tv < (unsigned)V ? tv : (unsigned)V - 1u);
                        const cx<T> x = vec_get<T>(q[u], e);
                        const double xr = (double)x.x, xi = (double)x.y, fr = f[0], fi = f[1];
                        vec_set(r, e, mk<T>((T)(fr * xr - fi * xi), (T)(fr * xi + fi * xr)));
                    }
                }
                dst[v] = r;
            }
        }
    }
}

int check_bins(const char* what, int V) {
    if (V >= 1 && V <= HS_MAX_BINS) return DQ_OK;
    set_error("%s: V=%d bins outside [1, %d] (dq_cost_hist_max_bins)", what, V, HS_MAX_BINS);
    return DQ_ERR_ARG;
}

template <typename T>
int hist_impl(const void* bra, const void* ket, const void* bin, int V, int n, const int* bits, int k, const int* controls, int nc,
              int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    constexpr int SBITS = ST_UNIT_BITS + (C128 ? 0 : 1);
    const char* what = "dq_cost_hist";
    const StateBuf bufs[] = {{"bra", bra}, {"ket", ket}};
    if (int rc = check_buffers(what, bufs, 2, nullptr, 0, 1, n, batch, sizeof(cx<T>))) return rc;
    if (int rc = check_bins(what, V)) return rc;
    Gather g;
    bool ident;
    if (int rc = plan_gather(what, n, bits, k, controls, nc, batch, C128, &g, &ident)) return rc;
    if (!bin || misaligned(bin)) {
        set_error("%s: the bin table must be non-null and 16-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (int rc = check_out_ws(what, out, ws)) return rc;
    const int64_t need = hist_ws_bytes(n, batch, C128, V);
    if (ws_bytes < need) {
        set_error("%s: workspace of %lld bytes, %lld needed (%s_ws_bytes)", what, (long long)ws_bytes, (long long)need, what);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const unsigned nblk = hist_blocks(nvec, V);
    const dim3 grid(nblk, (unsigned)batch);
    const int cbits = hist_copy_bits(V);
    int vbits = 0;
    while ((1 << vbits) < V) ++vbits;
    const size_t lds = (size_t)HS_WAVES * ((size_t)V << cbits) * 2 * sizeof(double);
    const uint64_t red = hist_free_low(bits, k, g.cmask, SBITS);
    const cx<T>* pb = static_cast<const cx<T>*>(bra);
    const cx<T>* pk = static_cast<const cx<T>*>(ket);
    const bin_t* pt = static_cast<const bin_t*>(bin);
    double* part = static_cast<double*>(ws);
    hipStream_t s = as_stream(stream);
    const bool same = bra == ket;
#define DQ_HIST(SAME, ID)                                                                                                    \
    hipLaunchKernelGGL((cost_hist_kernel<T, SAME, ID>), grid, dim3(ST_THREADS), lds, s, pb, pk, pt, g, red, n, units_of(nvec), V, \
                       cbits, vbits, part)
    if (same && ident) DQ_HIST(true, true);
    else if (same) DQ_HIST(true, false);
    else if (ident) DQ_HIST(false, true);
    else DQ_HIST(false, false);
#undef DQ_HIST
    if (int rc = check_launch(what)) return rc;
    const uint64_t bins = (uint64_t)batch * (uint64_t)V;
    hipLaunchKernelGGL(hist_finish_kernel, dim3((unsigned)((bins + HS_WAVES - 1) / HS_WAVES)), dim3(ST_THREADS), 0, s, part, nblk, V,
                       bins, out);
    return check_launch(what);
}

template <typename T>
int binned_impl(const void* in, void* out, const void* bin, const double* gtab, int V, int n, const int* bits, int k,
                const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_binned";
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), SAME_OR_DISJOINT)) return rc;
    if (int rc = check_bins(what, V)) return rc;
    Gather g;
    bool ident;
    if (int rc = plan_gather(what, n, bits, k, controls, nc, batch, C128, &g, &ident)) return rc;
    if (!bin || misaligned(bin) || !gtab || misaligned(gtab)) {
        set_error("%s: the bin table and g must be non-null and 16-byte aligned", what);
        return DQ_ERR_ARG;
    }
    const uint64_t nvec = vectors_of(n, C128);
    const dim3 grid(blocks_of(nvec), (unsigned)batch);
    const size_t lds = (size_t)V * 2 * sizeof(double);
    const cx<T>* pi = static_cast<const cx<T>*>(in);
    cx<T>* po = static_cast<cx<T>*>(out);
    const bin_t* pt = static_cast<const bin_t*>(bin);
    hipStream_t s = as_stream(stream);
    if (ident)
        hipLaunchKernelGGL((apply_binned_kernel<T, true>), grid, dim3(ST_THREADS), lds, s, pi, po, pt, gtab, g, n, units_of(nvec), V);
    else
        hipLaunchKernelGGL((apply_binned_kernel<T, false>), grid, dim3(ST_THREADS), lds, s, pi, po, pt, gtab, g, n, units_of(nvec), V);
    return check_launch(what);
}

}  // namespace
}  // namespace dq

extern "C" int dq_cost_hist_max_bins(void) { return dq::HS_MAX_BINS; }

extern "C" int64_t dq_cost_hist_ws_bytes(int n, int64_t batch, int is_c128, int cross, int V) {
    (void)cross;        // bra != ket reads twice as much and writes the same partial sums
    if (n < 1 || n > 40 || batch < 1 || batch > 65535 || V < 1 || V > dq::HS_MAX_BINS) return -1;
    return dq::hist_ws_bytes(n, batch, is_c128 != 0, V);
}

extern "C" int dq_cost_hist_c64(const void* bra, const void* ket, const void* bin, int V, int n, const int* bits, int k,
                                const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                dq_stream_t stream) {
    return dq::hist_impl<float>(bra, ket, bin, V, n, bits, k, controls, nc, batch, out, ws, ws_bytes, stream);
}
extern "C" int dq_cost_hist_c128(const void* bra, const void* ket, const void* bin, int V, int n, const int* bits, int k,
                                 const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                                 dq_stream_t stream) {
    return dq::hist_impl<double>(bra, ket, bin, V, n, bits, k, controls, nc, batch, out, ws, ws_bytes, stream);
}

extern "C" int dq_apply_binned_c64(const void* in, void* out, const void* bin, const double* g, int V, int n, const int* bits,
                                   int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::binned_impl<float>(in, out, bin, g, V, n, bits, k, controls, nc, batch, stream);
}
extern "C" int dq_apply_binned_c128(const void* in, void* out, const void* bin, const double* g, int V, int n, const int* bits,
                                    int k, const int* controls, int nc, int64_t batch, dq_stream_t stream) {
    return dq::binned_impl<double>(in, out, bin, g, V, n, bits, k, controls, nc, batch, stream);
}
