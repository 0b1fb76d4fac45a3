// The quantum Fourier transform on any list of wires as FFT stages: a length-2^m DFT over the value read from the wires,
// ceil(m / group) reads and writes of the state where the gate sequence (m Hadamards, m (m - 1) / 2 controlled phases)
// needs a pass of the fused kernel per ~72 gates.
//
// Convention.  bits[0..m) are index-bit positions, bits[0] the most significant bit of the transformed number (wire i of
// the list).  The swap-free transform -- the gate sequence without its final swaps -- leaves bit b_i of the result on
// wire i, where y = sum_i b_i 2^i: the bits of y come out reversed over the list.
//
// Stages.  Cut the list into consecutive groups G_1 .. G_r, G_p = wires i0 .. i1.  The swap-free circuit is S_r .. S_1,
//     S_p = D_p F_p,   F_p = the swap-free transform on the wires of G_p alone,
//     D_p = exp(2 pi i (A B mod 2^s) / 2^s),   s = m - i0,   A = sum_{i in G_p} b_i 2^(i - i0),
//                                              B = sum_{j > i1} x_j 2^(m - 1 - j)
// (the controlled phases from later wires onto the group commute with everything the group still does).  The inverse is
// S_1^+ .. S_r^+, S_p^+ = F_p^+ conj(D_p).  The same identity, applied inside a group, splits F_p into register stages.
//
// Work split.  One workgroup of 256 lanes owns a tile of 2^tb amplitudes, tb = min(T, n), T = 12 (complex64) / 11
// (complex128): 32 KiB of LDS.  The tile's index bits are the group's positions plus riders: the index bits of a 128-byte
// line (the lowest 4 / 3) that the group does not cover, so that every lane moves 16-byte vectors and every line is read
// and written whole.  A group therefore takes T wires less the line bits it misses; the host cuts the list greedily under
// that rule (cut_groups).  Only the last group of a list can be short; its tile is filled up with the lowest other index
// bits so that a tile is always 2^tb amplitudes.  A stage reads and writes its own tile only: in == out is allowed.
//
// Data movement.  Tile-local index t has the tile's positions in ascending order (t -> offset in the sample: `sc`, the
// tile's number -> its base: `sb`, both lists of runs in a Gather of dq_stream.hpp, used as a deposit).  On the way into
// LDS the amplitude moves to its canonical index l = [riders | group], the group's wires in significance order in the low
// g bits (`pl`), and back on the way out (`ps`).  Where the whole list is one group, the bit reversal of the swap form is
// nothing but another `ps`.
//
// Local transform.  The low g bits of l are cut into windows of 4 bits, [0, 4), [4, 8), [8, 12).  Per window a lane holds
// the 16 amplitudes that differ in the window's bits in registers and runs the radix-16 decimation-in-frequency butterfly
// on them (radix 8 / 4 / 2 where the group ends inside the window: the other registers are riders that the lane carries
// along), then the phases exp(2 pi i A' B' / 2^(lo + r)) that tie the window's wires to the group's lower bits B' -- the
// same for all 16 registers: w^1, w^2, w^4, w^8, each from its own exactly reduced 12-bit exponent e as root[e >> 6] *
// root'[e & 63] (two LDS tables of 64 roots of unity, one sincospi per entry, filled once per workgroup), and every w^A'
// one product of {1, w1, w2, w1 w2} x {1, w4, w8, w4 w8}.  Between windows the tile is transposed through
// LDS.  The LDS index is swizzled, phys = l ^ ((l >> 4 ^ l >> 8) & 15): in every window the lanes of a wave differ in the
// two nibbles that are not the window's, consecutive lanes in the lower of them, so for every register the 16 consecutive
// lanes that LDS serves together hit 16 different columns (8- or 16-byte) whichever window is being worked on -- no bank
// conflicts in the transposes by construction, and no padding.  (The scatter of the load and the gather of the store
// follow the wire list: for a descending list they are conflict-free for the same reason, a shuffled list pays there.)
//
// Twiddles D_p.  The exponent is reduced in integers: (A B) mod 2^s with A < 2^12 and B < 2^40 fits 64 bits; s <= 40 and
// the quotient by 2^s is exact in double.  B = B_out + B_rid: the later wires outside the tile (uniform over the
// workgroup, read from the tile's number through `gb`) and the riders that are later wires (at most the line bits, the
// low `rho` bits of the rider field of l).  The group field c of l is cut into two halves, A = rev(c) being additive over
// them; per tile two LDS tables over (half of c, B_rid) of at most 256 entries each are filled, every entry by its own
// sincospi in double of its own reduced angle, rounded once to the state's precision, the scale 2^(-g/2) folded into the
// first.  An amplitude's twiddle is table0 * table1, then one product with the amplitude.  No running product, no
// sincos of an unreduced angle.  The last group has no twiddle: B = 0.
#include "dq_stream.hpp"

namespace dq {

namespace {

constexpr int QFT_THREADS = 256;
constexpr int QFT_TABLE = 256;                          // entries of one twiddle table
constexpr int QFT_FLAG_INVERSE = 1, QFT_FLAG_SWAPS = 2;

constexpr int qft_tile_bits(bool c128) { return c128 ? 11 : 12; }
constexpr int qft_line_bits(bool c128) { return c128 ? 3 : 4; }           // a 128-byte line in amplitudes

struct QftStage {
    Gather sc, sb, pl, ps, gb;                          // lists of runs, see the header (nlow and cmask unused)
    int tb, g, rho, s, has_tw;
    uint8_t rsh[4];                                     // weight (a shift) in B of rider bit k of l, k < rho
};

__device__ __forceinline__ uint64_t runs_of(const Gather& g, uint64_t x) {
    uint64_t s = 0;
    for (int r = 0; r < g.nruns; ++r) s |= ((x >> g.src[r]) & ((1ull << g.len[r]) - 1ull)) << g.dst[r];
    return s;
}

// runs_of for the vector number u * 256 of a lane's u-th vector, u < 8: OR-separable over the three bits of u, so three
// evaluations (uniform: scalar arithmetic) serve the eight vectors
struct UPart {
    uint64_t v[3];
};
__device__ __forceinline__ UPart upart_of(const Gather& g, int shift) {
    UPart p;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.v[k] = runs_of(g, 1ull << (shift + k));
    return p;
}
__device__ __forceinline__ uint64_t at_u(const UPart& p, int u) {
    return ((u & 1) ? p.v[0] : 0ull) | ((u & 2) ? p.v[1] : 0ull) | ((u & 4) ? p.v[2] : 0ull);
}

__device__ __forceinline__ unsigned swz(unsigned l) { return l ^ (((l >> 4) ^ (l >> 8)) & 15u); }

__device__ __forceinline__ void sincospi_of(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ void sincospi_of(double x, double* s, double* c) { sincospi(x, s, c); }

// a * exp(2 pi i j / 16): j is a constant wherever this is called (fully unrolled loops), the switch folds
template <typename T> __device__ __forceinline__ cx<T> mul_root16(cx<T> a, int j) {
    constexpr double C1 = 0.92387953251128674, S1 = 0.38268343236508977, H = 0.70710678118654752;
    constexpr double co[16] = {1, C1, H, S1, 0, -S1, -H, -C1, -1, -C1, -H, -S1, 0, S1, H, C1};
    constexpr double si[16] = {0, S1, H, C1, 1, C1, H, S1, 0, -S1, -H, -C1, -1, -C1, -H, -S1};
    j &= 15;
    switch (j) {
        case 0: return a;
        case 4: return mk<T>(-a.y, a.x);
        case 8: return mk<T>(-a.x, -a.y);
        case 12: return mk<T>(a.y, -a.x);
        case 2: return mk<T>((a.x - a.y) * (T)H, (a.x + a.y) * (T)H);
        case 6: return mk<T>((-a.x - a.y) * (T)H, (a.x - a.y) * (T)H);
        case 10: return mk<T>((a.y - a.x) * (T)H, (-a.x - a.y) * (T)H);
        case 14: return mk<T>((a.x + a.y) * (T)H, (a.y - a.x) * (T)H);
        default: return cmul(a, mk<T>((T)co[j], (T)si[j]));
    }
}

constexpr int rev_bits(int v, int r) {
    int o = 0;
    for (int k = 0; k < r; ++k) o |= ((v >> k) & 1) << (r - 1 - k);
    return o;
}

// One window on a lane's 16 registers: the swap-free transform on register-index bits [0, R) (bit R - 1 the most
// significant wire), unscaled, and the phases exp(2 pi i A' bp / 2^(lo + R)), A' = rev_R(e), that tie it to the lower
// group bits bp < 2^lo; INV: the conjugate phases first, then the butterflies undone (unscaled as well: times 2 a bit).
template <typename T, bool INV, int R>
__device__ __forceinline__ void window(cx<T> (&a)[16], int lo, unsigned bp, const cx<T> (*root)[64]) {
    cx<T> tw[1 << R];
    if (lo > 0) {
        cx<T> w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[k] = mk<T>((T)1, (T)0);
            if (k < R) {
                // (2^k bp) mod 2^(lo + R) as a fraction of 12 bits: exact; its root from the two halves of the fraction
                const unsigned e = ((bp << k) << (12 - lo - R)) & 4095u;
                w[k] = cmul(root[0][e >> 6], root[1][e & 63u]);
            }
        }
        const cx<T> low[4] = {mk<T>((T)1, (T)0), w[0], w[1], cmul(w[0], w[1])};
        const cx<T> high[4] = {mk<T>((T)1, (T)0), w[2], w[3], cmul(w[2], w[3])};
#pragma unroll
        for (int v = 0; v < (1 << R); ++v) tw[v] = (v >> 2) == 0 ? low[v & 3] : (v & 3) == 0 ? high[v >> 2] : cmul(low[v & 3], high[v >> 2]);
    }
    if constexpr (INV) {
        if (lo > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) a[e] = cmul(a[e], tw[rev_bits(e & ((1 << R) - 1), R)]);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e & (1 << k)) continue;
                const cx<T> u = a[e], v = mul_root16<T>(a[e | (1 << k)], -((e & ((1 << k) - 1)) << (3 - k)));
                a[e] = mk<T>(u.x + v.x, u.y + v.y);
                a[e | (1 << k)] = mk<T>(u.x - v.x, u.y - v.y);
            }
        }
    } else {
#pragma unroll
        for (int k = R - 1; k >= 0; --k) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e & (1 << k)) continue;
                const cx<T> p = a[e], q = a[e | (1 << k)];
                a[e] = mk<T>(p.x + q.x, p.y + q.y);
                a[e | (1 << k)] = mul_root16<T>(mk<T>(p.x - q.x, p.y - q.y), (e & ((1 << k) - 1)) << (3 - k));
            }
        }
        if (lo > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) a[e] = cmul(a[e], tw[rev_bits(e & ((1 << R) - 1), R)]);
        }
    }
}

// The stage's twiddle (or, for the last group, its bare scale) on the amplitude at canonical index l
template <typename T>
__device__ __forceinline__ cx<T> twiddled(cx<T> a, unsigned l, const QftStage& p, const cx<T> (*tab)[QFT_TABLE], T scale) {
    if (!p.has_tw) return mk<T>(a.x * scale, a.y * scale);
    const int hl = p.g >> 1;
    const unsigned c = l & ((1u << p.g) - 1u), rid = (l >> p.g) & ((1u << p.rho) - 1u);
    const unsigned i0 = (((c & ((1u << hl) - 1u)) << p.rho) | rid) & (QFT_TABLE - 1);
    const unsigned i1 = (((c >> hl) << p.rho) | rid) & (QFT_TABLE - 1);
    return cmul(a, cmul(tab[0][i0], tab[1][i1]));
}

template <typename T, bool INV>
__global__ __launch_bounds__(QFT_THREADS) void qft_stage_kernel(const cx<T>* in, cx<T>* out, QftStage p, int n) {
    using Q = typename Vec16<T>::type;
    constexpr bool C128 = sizeof(T) == 8;
    constexpr int VEC = 16 / (int)sizeof(cx<T>);
    constexpr int VB = VEC == 2 ? 1 : 0;
    constexpr int TB = qft_tile_bits(C128);
    constexpr int NU = (1 << (TB - VB)) / QFT_THREADS;  // vectors of a lane: 8
    static_assert(NU == 8, "UPart splits u into three bits");
    __shared__ cx<T> tile[1 << TB];
    __shared__ cx<T> tab[2][QFT_TABLE];
    __shared__ cx<T> root[2][64];                       // exp(+-2 pi i k / 64), exp(+-2 pi i k / 4096), k < 64
    const unsigned lane = threadIdx.x;
    const unsigned lmask = (1u << p.tb) - 1u;
    const uint64_t tau = blockIdx.x;
    const uint64_t smask = (1ull << n) - 1ull;
    const uint64_t base = runs_of(p.sb, tau) & smask;
    const cx<T>* src = in + ((uint64_t)blockIdx.y << n);
    cx<T>* dst = out + ((uint64_t)blockIdx.y << n);
    const T scale = (T)exp2(-0.5 * (double)p.g);

    if (p.g > 4 && lane < 128) {                        // (a group inside the lowest window has no phases of its own)
        T sn, cs;
        sincospi_of((T)(lane & 63u) * (T)(lane < 64 ? 2.0 / 64.0 : 2.0 / 4096.0), &sn, &cs);
        root[lane >> 6][lane & 63u] = mk<T>(cs, INV ? -sn : sn);
    }
    if (p.has_tw) {
        // the two tables over (half of the group field, later-wire riders): one sincospi in double per entry
        const uint64_t bout = runs_of(p.gb, tau);
        const int hl = p.g >> 1;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int bits = (half ? p.g - hl : hl) + p.rho;
            if (lane < (1u << bits) && lane < QFT_TABLE) {
                const unsigned rid = lane & ((1u << p.rho) - 1u);
                const uint64_t c = (uint64_t)(lane >> p.rho) << (half ? hl : 0);
                const uint64_t a = __brevll(c) >> (64 - p.g);                     // A = rev_g(c)
                uint64_t bb = bout;
                for (int k = 0; k < p.rho; ++k) bb |= (uint64_t)((rid >> k) & 1u) << p.rsh[k];
                const uint64_t e = (a * bb) & ((1ull << p.s) - 1ull);             // (A B) mod 2^s, A < 2^12, B < 2^40
                double s, c2;
                sincospi(ldexp((double)e, 1 - p.s), &s, &c2);
                const double f = half ? 1.0 : (double)scale;
                tab[half][lane] = mk<T>((T)(c2 * f), (T)((INV ? -s : s) * f));
            }
        }
    }

    // ---- load: 16-byte vectors, whole lines, each amplitude to its canonical place in LDS
    const unsigned nvec = 1u << (p.tb - VB);
    const uint64_t off_lane = runs_of(p.sc, (uint64_t)lane << VB);
    const unsigned pl_lane = (unsigned)runs_of(p.pl, (uint64_t)lane << VB);
    const unsigned pl_e1 = VB ? (unsigned)runs_of(p.pl, 1ull) : 0u;
    Q q[NU];
    {
        const UPart su = upart_of(p.sc, 8 + VB);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const uint64_t off = (base | off_lane | at_u(su, u)) & smask;
            if (u * QFT_THREADS + lane < nvec) q[u] = reinterpret_cast<const Q*>(src)[off >> VB];
        }
    }
    if (INV && p.has_tw) __syncthreads();               // the tables are read below
    const UPart lu = upart_of(p.pl, 8 + VB);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u * QFT_THREADS + lane >= nvec) continue;
        const unsigned pu = pl_lane | (unsigned)at_u(lu, u);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned l = (pu | (e ? pl_e1 : 0u)) & lmask;
            cx<T> a = vec_get<T>(q[u], e);
            if constexpr (INV) a = twiddled<T>(a, l, p, tab, scale);
            tile[swz(l)] = a;
        }
    }

    // ---- the windows, the most significant first (INV: last)
    const int nwin = (p.tb + 3) >> 2;
    for (int i = 0; i < nwin; ++i) {
        const int w = INV ? i : nwin - 1 - i;
        const int lo = 4 * w;
        const int ww = p.tb - lo < 4 ? p.tb - lo : 4;
        const int r = p.g - lo < 0 ? 0 : p.g - lo < ww ? p.g - lo : ww;
        if (r == 0) continue;                           // (uniform: the window holds riders only)
        __syncthreads();
        const unsigned nchunks = 1u << (p.tb - ww);
        for (unsigned c = lane; c < nchunks; c += QFT_THREADS) {
            const unsigned bp = c & ((1u << lo) - 1u);
            const unsigned l0 = ((c >> lo) << (lo + ww)) | bp;
            cx<T> a[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) a[e] = e < (1 << ww) ? tile[swz((l0 | ((unsigned)e << lo)) & lmask)] : mk<T>((T)0, (T)0);
            switch (r) {
                case 1: window<T, INV, 1>(a, lo, bp, root); break;
                case 2: window<T, INV, 2>(a, lo, bp, root); break;
                case 3: window<T, INV, 3>(a, lo, bp, root); break;
                default: window<T, INV, 4>(a, lo, bp, root); break;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e < (1 << ww)) tile[swz((l0 | ((unsigned)e << lo)) & lmask)] = a[e];
        }
    }
    __syncthreads();

    // ---- store: gather from LDS, twiddle, 16-byte vectors
    const unsigned ps_lane = (unsigned)runs_of(p.ps, (uint64_t)lane << VB);
    const unsigned ps_e1 = VB ? (unsigned)runs_of(p.ps, 1ull) : 0u;
    const UPart su = upart_of(p.sc, 8 + VB), du = upart_of(p.ps, 8 + VB);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u * QFT_THREADS + lane >= nvec) continue;
        const uint64_t off = (base | off_lane | at_u(su, u)) & smask;
        const unsigned pu = ps_lane | (unsigned)at_u(du, u);
        Q r;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned l = (pu | (e ? ps_e1 : 0u)) & lmask;
            cx<T> a = tile[swz(l)];
            if constexpr (!INV) a = twiddled<T>(a, l, p, tab, scale);
            vec_set(r, e, a);
        }
        reinterpret_cast<Q*>(dst)[off >> VB] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------
// first[k] = the list index at which group k starts, first[ngroups] = m; returns ngroups.  A group takes wires while
// its wires and the line bits it misses fit the tile.
int cut_groups(int n, const int* bits, int m, bool c128, int* first) {
    const int tb = qft_tile_bits(c128) < n ? qft_tile_bits(c128) : n;
    const int lb = qft_line_bits(c128) < n ? qft_line_bits(c128) : n;
    int ng = 0;
    for (int i = 0; i < m;) {
        first[ng++] = i;
        uint64_t mask = 0;
        for (int g = 0; i < m; ++g, ++i) {
            const uint64_t with = mask | 1ull << bits[i];
            const int missing = lb - __builtin_popcountll(with & ((1ull << lb) - 1ull));
            if (g + 1 + missing > tb) break;
            mask = with;
        }
    }
    first[ng] = m;
    return ng;
}

// src -> dst, merged into the last run where both continue it
void add_run(Gather* g, int src, int dst) {
    if (g->nruns > 0) {
        const int r = g->nruns - 1;
        if (g->src[r] + g->len[r] == src && g->dst[r] + g->len[r] == dst) {
            ++g->len[r];
            return;
        }
    }
    g->src[g->nruns] = (uint8_t)src;
    g->len[g->nruns] = 1;
    g->dst[g->nruns] = (uint8_t)dst;
    ++g->nruns;
}

// The stage of the group of wires [i0, i1) of the list; `swaps`: the store takes the bits reversed (one group only)
void plan_stage(int n, const int* bits, int m, int i0, int i1, bool c128, bool swaps, QftStage* st) {
    *st = QftStage{};
    const int tb = qft_tile_bits(c128) < n ? qft_tile_bits(c128) : n;
    const int lb = qft_line_bits(c128) < n ? qft_line_bits(c128) : n;
    const int g = i1 - i0;
    int wire_at[40];                                    // the list index of the wire at a position, -1: none
    for (int p = 0; p < n; ++p) wire_at[p] = -1;
    for (int i = 0; i < m; ++i) wire_at[bits[i]] = i;
    uint64_t gmask = 0;
    for (int i = i0; i < i1; ++i) gmask |= 1ull << bits[i];
    uint64_t tmask = gmask;
    int count = g;
    for (int p = 0; p < lb; ++p)
        if (!((tmask >> p) & 1ull)) tmask |= 1ull << p, ++count;
    for (int p = 0; p < n && count < tb; ++p)           // (the last group only: cut_groups fills the others)
        if (!((tmask >> p) & 1ull)) tmask |= 1ull << p, ++count;
    // canonical LDS bit of every tile position: the group in significance order below, later-wire riders, other riders
    int lbit[40], lbit_out[40];
    for (int i = i0; i < i1; ++i) lbit[bits[i]] = g - 1 - (i - i0);
    int next = g, rho = 0;
    for (int p = 0; p < n; ++p)
        if (((tmask & ~gmask) >> p) & 1ull && wire_at[p] >= i1 && rho < 4) {
            st->rsh[rho++] = (uint8_t)(m - 1 - wire_at[p]);
            lbit[p] = next++;
        }
    for (int p = 0; p < n; ++p)
        if (((tmask & ~gmask) >> p) & 1ull && !(wire_at[p] >= i1)) lbit[p] = next++;
    for (int p = 0; p < n; ++p) lbit_out[p] = lbit[p];
    if (swaps)
        for (int i = i0; i < i1; ++i) lbit_out[bits[i]] = lbit[bits[i1 - 1 - (i - i0)]];
    int q = 0, qb = 0;
    for (int p = 0; p < n; ++p) {
        if ((tmask >> p) & 1ull) {
            add_run(&st->sc, q, p);
            add_run(&st->pl, q, lbit[p]);
            add_run(&st->ps, q, lbit_out[p]);
            ++q;
        } else {
            add_run(&st->sb, qb, p);
            if (wire_at[p] >= i1) add_run(&st->gb, qb, m - 1 - wire_at[p]);
            ++qb;
        }
    }
    st->tb = tb;
    st->g = g;
    st->rho = rho;
    st->s = m - i0;
    st->has_tw = i1 < m;
}

int qft_check_list(const char* what, int n, const int* bits, int m) {
    if (n < 1 || n > 40 || m < 1 || m > n) {
        set_error("%s: m=%d outside [1, n] or n=%d outside [1, 40]", what, m, n);
        return DQ_ERR_ARG;
    }
    return validate_bits(n, bits, m, nullptr, 0);
}

template <typename T>
int qft_impl(const void* in, void* out, int n, const int* bits, int m, int flags, int64_t batch, dq_stream_t stream) {
    constexpr bool C128 = sizeof(T) == 8;
    const char* what = "dq_apply_qft";
    if (int rc = check_states(what, in, out, 1, n, batch, sizeof(cx<T>), SAME_OR_DISJOINT)) return rc;
    if (int rc = qft_check_list(what, n, bits, m)) return rc;
    if (flags < 0 || flags > (QFT_FLAG_INVERSE | QFT_FLAG_SWAPS)) {
        set_error("%s: inverse=%d is not a combination of 1 (inverse) and 2 (swaps)", what, flags);
        return DQ_ERR_ARG;
    }
    int first[41];
    const int ng = cut_groups(n, bits, m, C128, first);
    const bool inv = flags & QFT_FLAG_INVERSE, swaps = flags & QFT_FLAG_SWAPS;
    if (swaps && ng > 1) {
        set_error("%s: the swap form runs inside the kernel for one stage only, this list takes %d (dq_qft_passes)", what, ng);
        return DQ_ERR_ARG;
    }
    hipStream_t s = as_stream(stream);
    const cx<T>* from = static_cast<const cx<T>*>(in);
    cx<T>* to = static_cast<cx<T>*>(out);
    for (int k = 0; k < ng; ++k) {
        const int grp = inv ? ng - 1 - k : k;
        QftStage st;
        plan_stage(n, bits, m, first[grp], first[grp + 1], C128, swaps, &st);
        if (inv) {                                      // the adjoint takes the reversed bits on its way in
            const Gather t = st.pl;
            st.pl = st.ps;
            st.ps = t;
        }
        const dim3 grid((unsigned)(1ull << (n - st.tb)), (unsigned)batch);
        if (inv) hipLaunchKernelGGL((qft_stage_kernel<T, true>), grid, dim3(QFT_THREADS), 0, s, from, to, st, n);
        else hipLaunchKernelGGL((qft_stage_kernel<T, false>), grid, dim3(QFT_THREADS), 0, s, from, to, st, n);
        if (int rc = check_launch(what)) return rc;
        from = to;                                      // the stages after the first run in place on out
    }
    return DQ_OK;
}

}  // namespace
}  // namespace dq

extern "C" int dq_apply_qft_c64(const void* in, void* out, int n, const int* bits, int m, int inverse, int64_t batch,
                                dq_stream_t stream) {
    return dq::qft_impl<float>(in, out, n, bits, m, inverse, batch, stream);
}
extern "C" int dq_apply_qft_c128(const void* in, void* out, int n, const int* bits, int m, int inverse, int64_t batch,
                                 dq_stream_t stream) {
    return dq::qft_impl<double>(in, out, n, bits, m, inverse, batch, stream);
}

extern "C" int dq_qft_tile_bits(int is_c128) { return dq::qft_tile_bits(is_c128 != 0); }

extern "C" int dq_qft_passes(int n, const int* bits, int m, int is_c128) {
    if (dq::qft_check_list("dq_qft_passes", n, bits, m)) return -1;
    int first[41];
    return dq::cut_groups(n, bits, m, is_c128 != 0, first);
}
