// Shot sampling by inverse CDF without a 2^n-element temporary: raw outcomes for explicit uniforms.
//
//     p_j = |psi[b, j]|^2,  C(i) = sum_{j <= i} p_j,  T = C(2^n - 1)
//     out[b, s] = the smallest i with C(i) > u[b, s] * T
//
// All arithmetic is double for both precisions (a complex64 amplitude is converted before it is squared).  The state
// need not be normalised.
//
// Tree.  Level 0 is the amplitudes (2^n squares); level l holds the sums of 64 consecutive level-(l-1) entries,
// 2^(n - 6 l) of them, up to level nlev = ceil(n / 6) - 1, the first with at most 64 entries: the root group, of
// 2^(n - 6 nlev) entries (2 .. 64; every other group is full).  n <= 6 has no tree: the amplitudes are the root
// group.  The workspace holds levels 1 .. nlev, each as [batch][2^(n - 6 l)] doubles: 2^n / 63 doubles per sample.
//
// Build.  One workgroup per chunk of 4096 amplitudes (one level-2 entry), grid-stride, 16-byte loads: a wave-load
// covers one group (complex128) or two (complex64), a wave owns 16 groups and has all its loads in flight before the
// first sum.  A group is added in a fixed order (the lane's own amplitudes, then an xor butterfly over the lanes of
// the group), the 64 level-1 sums of the chunk go through LDS and wave 0 adds them the same way into the level-2
// entry.  Levels 3 .. nlev: one wave per entry, one small launch per level.
//
// Descent.  One wavefront owns one shot.  At each level lane l loads child l of the current group (512 coalesced
// bytes), the wave takes an inclusive scan in double, picks the first child whose inclusive sum exceeds the residual,
// subtracts that child's exclusive sum and goes down; the last level scans 64 squared amplitudes.  The scan adds in
// another order than the build, so a residual can end at or beyond the last inclusive sum of a group by a few ulps:
// then the last child with a non-zero value is taken, never one outside the group.  Children with a zero value are
// masked out of the choice (the scan's sums need not be monotone to the last bit), so an index with p_i == 0 is never
// returned whatever the rounding, and the index is in [0, 2^n) by construction.  No atomics, no host
// synchronisation, every sum in a fixed order: bitwise reproducible.
#include "dq_common.hpp"

namespace dq {

namespace {

constexpr int SMP_THREADS = 256;
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_MAX_LEVELS = 6;            // n = 40: ceil(40 / 6) - 1
constexpr unsigned SMP_BUILD_BLOCKS = 2048;  // 8 workgroups per CU striding over the chunks
constexpr unsigned SMP_MAX_GRID = 65535;     // workgroups of the descent and the upper levels; more work is strided over

struct SampleGeom {
    int n;
    int nlev;                          // tree levels (0: n <= 6)
    int root;                          // entries of the root group
    uint64_t off[SMP_MAX_LEVELS + 1];  // level l (1 .. nlev) starts at ws + off[l], [batch][2^(n - 6 l)]
};

int sample_levels(int n) { return (n + 5) / 6 - 1; }

// doubles of workspace: levels 1 .. nlev for every sample
int64_t sample_plan(int n, int64_t batch, SampleGeom* g) {
    const int nlev = sample_levels(n);
    int64_t total = 0;
    if (g) {
        g->n = n;
        g->nlev = nlev;
        g->root = 1 << (n - 6 * nlev);
    }
    for (int l = 1; l <= nlev; ++l) {
        if (g) g->off[l] = (uint64_t)total;
        total += batch << (n - 6 * l);
    }
    return total;
}

// The sum over the lanes of a group of `W` lanes (W = 32 or 64), the same bits in every lane of the group.
template <int W>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = 1; o < W; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Inclusive scan over the 64 lanes.
__device__ __forceinline__ double wave_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

template <typename T> struct Quad;    // 16 bytes of amplitudes
template <> struct Quad<float> {
    using type = float4;
    static __device__ __forceinline__ double sq(const float4& q) {
        return ((double)q.x * (double)q.x + (double)q.y * (double)q.y) +
               ((double)q.z * (double)q.z + (double)q.w * (double)q.w);
    }
};
template <> struct Quad<double> {
    using type = double2;
    static __device__ __forceinline__ double sq(const double2& q) { return q.x * q.x + q.y * q.y; }
};

// Levels 1 and 2 from one read of the state.  grid-stride over batch * 2^max(n - 12, 0) chunks.
template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_build_kernel(const cx<T>* __restrict__ psi, SampleGeom g,
                                                                   uint64_t nchunks, double* __restrict__ ws) {
    using Q = typename Quad<T>::type;
    constexpr int GPL = 16 / (int)sizeof(cx<T>);     // groups per wave-load: 2 (complex64) or 1
    constexpr int GW = 64 / GPL;                     // lanes of a group
    constexpr int ITERS = 16 / GPL;                  // wave-loads per wave and chunk
    __shared__ double s1[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cbits = g.n > 12 ? g.n - 12 : 0;                 // chunks per sample
    const int gpc = g.n >= 12 ? 64 : 1 << (g.n - 6);           // level-1 groups of a chunk (n >= 7: at least 2)
    const int g0 = wave * 16;
    // this lane's level-1 entry of the wave's 16: lane (i, half h) of wave-load i keeps group GPL i + h
    const int slot = GPL == 2 ? 2 * (lane & 31) + (lane >> 5) : lane;
    const bool keeper = slot < 16 && g0 + slot < gpc;
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint64_t b = chunk >> cbits, c = chunk & ((1ull << cbits) - 1ull);
        const Q* p = reinterpret_cast<const Q*>(psi + (b << g.n) + (c << 12) + (uint64_t)g0 * 64);
        Q q[ITERS];
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            if (g0 + i * GPL < gpc) q[i] = p[i * 64 + lane];
            else q[i] = Q{};
        }
        double mine = 0.0;
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            const double s = group_sum<GW>(Quad<T>::sq(q[i]));
            if ((lane & (GW - 1)) == i) mine = s;
        }
        if (keeper) ws[g.off[1] + (b << (g.n - 6)) + (c << 6) + (uint64_t)(g0 + slot)] = mine;
        if (g.nlev >= 2) {              // (then every chunk is full)
            if (slot < 16) s1[g0 + slot] = mine;
            __syncthreads();
            if (wave == 0) {
                const double s = group_sum<64>(s1[lane]);
                if (lane == 0) ws[g.off[2] + (b << (g.n - 12)) + c] = s;
            }
            __syncthreads();
        }
    }
}

// dst[e] = the sum of src[64 e .. 64 e + 63]: one wave per entry (levels 3 and up; the batch rows are contiguous)
__global__ __launch_bounds__(SMP_THREADS) void sample_upper_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                   uint64_t count) {
    const int lane = threadIdx.x & 63;
    for (uint64_t e = (uint64_t)blockIdx.x * SMP_WAVES + (threadIdx.x >> 6); e < count; e += (uint64_t)gridDim.x * SMP_WAVES) {
        const double s = group_sum<64>(src[e * 64 + lane]);
        if (lane == 0) dst[e] = s;
    }
}

// One wave per shot: t = b * shots + s, strided over when batch * shots exceeds the grid.
template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_descend_kernel(const cx<T>* __restrict__ psi, SampleGeom g,
                                                                     const double* __restrict__ ws, const double* __restrict__ u,
                                                                     uint64_t shots, uint64_t total, int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (uint64_t t = (uint64_t)blockIdx.x * SMP_WAVES + (threadIdx.x >> 6); t < total; t += (uint64_t)gridDim.x * SMP_WAVES) {
        const uint64_t b = t / shots;
        uint64_t grp = 0;
        double r = 0.0;
        for (int l = g.nlev; l >= 0; --l) {
            const int cnt = l == g.nlev ? g.root : 64;
            double v = 0.0;
            if (lane < cnt) {
                if (l > 0) {
                    v = ws[g.off[l] + (b << (g.n - 6 * l)) + grp * 64 + lane];
                } else {
                    const cx<T> a = psi[(b << g.n) + grp * 64 + lane];
                    v = (double)a.x * (double)a.x + (double)a.y * (double)a.y;
                }
            }
            const double inc = wave_scan(v, lane);
            if (l == g.nlev) r = u[t] * __shfl(inc, 63, 64);
            // (the scan's sums are not monotone to the last bit: a zero entry is excluded by its value, not by its sum)
            const unsigned long long nz = __ballot(v > 0.0);
            const unsigned long long above = __ballot(inc > r) & nz;
            int c;
            if (above) c = __ffsll((long long)above) - 1;
            else c = nz ? 63 - __clzll((long long)nz) : 0;      // at or beyond the end of the group: its last non-zero entry
            const double before = __shfl_up(inc, 1, 64);
            r = fmax(r - __shfl(lane ? before : 0.0, c, 64), 0.0);
            grp = grp * 64 + (uint64_t)c;
        }
        if (lane == 0) out[t] = (int64_t)grp;
    }
}

template <typename T>
int sample_impl(const void* psi, int n, int64_t batch, const double* u, int64_t shots, int64_t* out, void* ws,
                int64_t ws_bytes, dq_stream_t stream) {
    if (!psi || !u || !out) {
        set_error("dq_sample: null pointer (psi, u or out)");
        return DQ_ERR_ARG;
    }
    if (n < 1 || n > 40 || batch < 1 || batch > 65535 || shots < 1) {
        set_error("dq_sample: bad argument (n=%d outside [1, 40], batch=%lld outside [1, 65535] or shots=%lld < 1)", n,
                  (long long)batch, (long long)shots);
        return DQ_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(psi) & 15) {
        set_error("dq_sample: psi must be 16-byte aligned");
        return DQ_ERR_ARG;
    }
    SampleGeom g{};
    const int64_t need = sample_plan(n, batch, &g) * (int64_t)sizeof(double);
    if (need > 0 && (!ws || ws_bytes < need)) {
        set_error("dq_sample: workspace of %lld bytes, %lld needed (dq_sample_ws_bytes)", (long long)ws_bytes, (long long)need);
        return DQ_ERR_ARG;
    }
    hipStream_t s = as_stream(stream);
    const cx<T>* p = static_cast<const cx<T>*>(psi);
    double* tree = static_cast<double*>(ws);
    if (g.nlev >= 1) {
        const uint64_t nchunks = (uint64_t)batch << (n > 12 ? n - 12 : 0);
        const unsigned nb = (unsigned)(nchunks < SMP_BUILD_BLOCKS ? nchunks : SMP_BUILD_BLOCKS);
        hipLaunchKernelGGL(sample_build_kernel<T>, dim3(nb), dim3(SMP_THREADS), 0, s, p, g, nchunks, tree);
        for (int l = 3; l <= g.nlev; ++l) {
            const uint64_t count = (uint64_t)batch << (n - 6 * l);
            const uint64_t wg = (count + SMP_WAVES - 1) / SMP_WAVES;
            hipLaunchKernelGGL(sample_upper_kernel, dim3((unsigned)(wg < SMP_MAX_GRID ? wg : SMP_MAX_GRID)), dim3(SMP_THREADS),
                               0, s, tree + g.off[l - 1], tree + g.off[l], count);
        }
    }
    const uint64_t total = (uint64_t)batch * (uint64_t)shots;
    const uint64_t wg = (total + SMP_WAVES - 1) / SMP_WAVES;
    hipLaunchKernelGGL(sample_descend_kernel<T>, dim3((unsigned)(wg < SMP_MAX_GRID ? wg : SMP_MAX_GRID)), dim3(SMP_THREADS), 0, s,
                       p, g, tree, u, (uint64_t)shots, total, out);
    return check_launch("dq_sample");
}

}  // namespace
}  // namespace dq

extern "C" int64_t dq_sample_ws_bytes(int n, int64_t batch, int is_c128) {
    (void)is_c128;      // the tree holds doubles for both precisions
    if (n < 1 || n > 40 || batch < 1 || batch > 65535) return -1;
    return dq::sample_plan(n, batch, nullptr) * (int64_t)sizeof(double);
}

extern "C" int dq_sample_c64(const void* psi, int n, int64_t batch, const double* u, int64_t shots, int64_t* out, void* ws,
                             int64_t ws_bytes, dq_stream_t stream) {
    return dq::sample_impl<float>(psi, n, batch, u, shots, out, ws, ws_bytes, stream);
}
extern "C" int dq_sample_c128(const void* psi, int n, int64_t batch, const double* u, int64_t shots, int64_t* out, void* ws,
                              int64_t ws_bytes, dq_stream_t stream) {
    return dq::sample_impl<double>(psi, n, batch, u, shots, out, ws, ws_bytes, stream);
}
