// The table of a sum of Pauli strings as the kernels of dq_psum.hip and dq_terms.hip take it (include/dq_hip.h section 13
// describes the four arrays), its host-side check, and the lane's vectors of a unit in their gather geometry.
#pragma once
#include "dq_stream.hpp"

namespace dq {

namespace {

struct PsumTable {
    const uint64_t* __restrict__ xmasks;
    const int* __restrict__ bounds;
    const uint64_t* __restrict__ zmasks;
    const double* __restrict__ weights;
    int ngroups, nterms;
};

// The lane's vectors of unit `unit`; one that lies beyond the sample is replaced by vector 0 and marked in `live`.
__device__ __forceinline__ unsigned unit_vectors(uint64_t unit, uint64_t nvec, uint64_t (&vec)[ST_UNROLL]) {
    unsigned live = 0;
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const uint64_t v = (unit << ST_UNIT_BITS) + (uint64_t)(u * ST_THREADS) + threadIdx.x;
        if (v < nvec) live |= 1u << u;
        vec[u] = v < nvec ? v : 0;
    }
    return live;
}

// The four arrays of the table: non-null, aligned to their element, at least one group and one term
int check_table(const char* what, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks, const double* weights,
                int ngroups, int nterms, PsumTable* tb) {
    if (!xmasks || !bounds || !zmasks || !weights) {
        set_error("%s: null table pointer", what);
        return DQ_ERR_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(xmasks) & 7) || (reinterpret_cast<uintptr_t>(zmasks) & 7) ||
        (reinterpret_cast<uintptr_t>(weights) & 7) || (reinterpret_cast<uintptr_t>(bounds) & 3)) {
        set_error("%s: xmasks, zmasks and weights must be 8-byte aligned, bounds 4-byte aligned", what);
        return DQ_ERR_ARG;
    }
    if (ngroups < 1) {
        set_error("%s: ngroups=%d, at least one group is needed", what, ngroups);
        return DQ_ERR_ARG;
    }
    if (nterms < 1) {
        set_error("%s: nterms=%d, at least one term is needed", what, nterms);
        return DQ_ERR_ARG;
    }
    *tb = PsumTable{xmasks, bounds, zmasks, weights, ngroups, nterms};
    return DQ_OK;
}

}  // namespace
}  // namespace dq
