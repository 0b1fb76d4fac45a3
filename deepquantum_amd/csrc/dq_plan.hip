// Host-side core of the pass planner (deepquantum_amd/fusion.py): the dry run of a pass over the commutation DAG of a
// gate list.  The planner asks "how many gates would a pass that owns this set of qubits retire from this front?"
// a few hundred thousand times per circuit (beam search over tiles, one candidate qubit at a time); in Python that was
// 10-12 s for the headline circuit, here it is a tight loop over flat arrays.  No device code; the reference has no
// counterpart (it applies gates one by one, circuit.py:261).
#include "dq_common.hpp"
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include <stdlib.h>
#include <string.h>

namespace {

// The DAG is READ-ONLY once made: any number of searches may walk it at the same time, each with a Scratch of its own.
struct Dag {
    int n;
    std::vector<int> succ_off, succ;
    std::vector<uint64_t> targets;      // qubits the gate needs inside the tile (0 for diagonal gates: they run anywhere)
    std::vector<uint8_t> fusable;
};

// What a dry run writes.  `cur` holds -1 for every gate between dry runs (in-degree not touched).
struct Scratch {
    std::vector<int> cur, touched, stack;
    std::vector<int> front;                     // an OPEN dry run (open_front): the gates left stuck, in no particular order
    std::vector<std::pair<int, int>> undo;      // ... and what a trial extension changed in `cur` (gate, value before)
    int* retired = nullptr;                     // when set: closure lists the gates it retires here, in order
    explicit Scratch(int n) : cur((size_t)n, -1) {}
};

// (the one-call entry points: a scratch per calling thread, grown to the largest DAG it has seen)
Scratch& local_scratch(int n) {
    static thread_local Scratch sc(0);
    if ((int)sc.cur.size() < n) sc.cur.assign((size_t)n, -1);
    return sc;
}

// Exactly fusion._closure: depth-first from `ready` (last first), a gate retires while fewer than `cap` have, it is
// fusable and its targets lie in `tile`; successors whose in-degree reaches 0 are pushed in list order.
int closure(const Dag& d, Scratch& sc, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, int* stuck,
            int* nstuck, int* changed_idx, int* changed_val, int* nchanged) {
    sc.stack.assign(ready, ready + nready);
    sc.touched.clear();
    int count = 0, ns = 0;
    while (!sc.stack.empty()) {
        const int i = sc.stack.back();
        sc.stack.pop_back();
        if (count >= cap || !d.fusable[i] || (d.targets[i] & ~tile)) {
            if (stuck) stuck[ns] = i;
            ++ns;
            continue;
        }
        if (sc.retired) sc.retired[count] = i;
        ++count;
        for (int e = d.succ_off[i]; e < d.succ_off[i + 1]; ++e) {
            const int s = d.succ[e];
            if (sc.cur[s] < 0) {                // first touch: take the caller's value
                sc.cur[s] = indeg[s];
                sc.touched.push_back(s);
            }
            if (--sc.cur[s] == 0) sc.stack.push_back(s);
        }
    }
    if (nstuck) *nstuck = ns;
    int nc = 0;
    for (int s : sc.touched) {
        if (changed_idx) {
            changed_idx[nc] = s;
            changed_val[nc] = sc.cur[s];
        }
        ++nc;
        sc.cur[s] = -1;
    }
    if (nchanged) *nchanged = nc;
    return count;
}

// The INCREMENTAL dry run.  A tile grows one qubit at a time and every candidate qubit is tried, so the dry run of the
// tile so far is kept OPEN -- the in-degrees it changed stay in `cur`, the gates it left stuck in `front` -- and a larger
// tile only EXTENDS it: the gates of the front that now fit retire, and whatever they free.  While fewer than `cap` gates
// have retired the retired SET does not depend on the order of the walk (it is the least fixed point), so the count is that
// of `closure` from scratch, min(cap, size of the set); the ORDER of the front differs, which is why the beam still takes
// the tile it finally chose through `closure`.
int open_front(const Dag& d, Scratch& sc, uint64_t tile, int cap, const int* indeg, const int* ready, int nready) {
    sc.stack.assign(ready, ready + nready);
    sc.touched.clear();
    sc.front.clear();
    int count = 0;
    while (!sc.stack.empty()) {
        const int i = sc.stack.back();
        sc.stack.pop_back();
        if (count >= cap || !d.fusable[i] || (d.targets[i] & ~tile)) {
            sc.front.push_back(i);
            continue;
        }
        ++count;
        for (int e = d.succ_off[i]; e < d.succ_off[i + 1]; ++e) {
            const int s = d.succ[e];
            if (sc.cur[s] < 0) {
                sc.cur[s] = indeg[s];
                sc.touched.push_back(s);
            }
            if (--sc.cur[s] == 0) sc.stack.push_back(s);
        }
    }
    return count;
}

// Extend the open dry run (`count` gates retired so far, fewer than `cap`) to `tile`, a superset of its tile; returns the
// new count.  commit = false: a trial, everything is put back; true: the open dry run is now that of `tile`.
int extend_front(const Dag& d, Scratch& sc, uint64_t tile, int cap, const int* indeg, int count, bool commit) {
    sc.stack.clear();
    sc.undo.clear();
    size_t keep = 0;
    for (size_t k = 0; k < sc.front.size(); ++k) {
        const int i = sc.front[k];
        if (d.fusable[i] && !(d.targets[i] & ~tile)) sc.stack.push_back(i);
        else if (commit) sc.front[keep++] = i;
    }
    if (commit) sc.front.resize(keep);
    while (!sc.stack.empty()) {
        if (count >= cap) {             // full: the rest stays at the front
            if (commit) sc.front.insert(sc.front.end(), sc.stack.begin(), sc.stack.end());
            break;
        }
        const int i = sc.stack.back();
        sc.stack.pop_back();
        ++count;
        for (int e = d.succ_off[i]; e < d.succ_off[i + 1]; ++e) {
            const int s = d.succ[e];
            if (!commit) sc.undo.emplace_back(s, sc.cur[s]);
            if (sc.cur[s] < 0) {
                sc.cur[s] = indeg[s];
                if (commit) sc.touched.push_back(s);
            }
            if (--sc.cur[s] == 0) {
                if (d.fusable[s] && !(d.targets[s] & ~tile)) sc.stack.push_back(s);
                else if (commit) sc.front.push_back(s);
            }
        }
    }
    for (size_t k = sc.undo.size(); k-- > 0;) sc.cur[sc.undo[k].first] = sc.undo[k].second;
    return count;
}

void close_front(Scratch& sc) {
    for (int s : sc.touched) sc.cur[s] = -1;
    sc.touched.clear();
    sc.front.clear();
}

// The qubits outside `tile` that the fusable gates of the open front wait for (order[0 .. nq)), with how many wait for each.
int front_wants(const Dag& d, const Scratch& sc, uint64_t tile, int* w, int* order) {
    int nq = 0;
    for (int i : sc.front) {
        if (!d.fusable[i]) continue;
        uint64_t miss = d.targets[i] & ~tile;
        while (miss) {
            const int q = __builtin_ctzll(miss);
            miss &= miss - 1;
            if (w[q]++ == 0) order[nq++] = q;
        }
    }
    return nq;
}

// Self-check of the incremental dry run (dq_dag_plan_verify): every count is also taken from scratch.
std::atomic<int> g_verify{0};
std::atomic<long long> g_compared{0}, g_mismatch{0};

}  // namespace

extern "C" void* dq_dag_create(int n_ops, const int* succ_off, const int* succ, const uint64_t* target_mask,
                               const uint8_t* fusable) {
    if (n_ops < 0 || !succ_off || (!succ && succ_off[n_ops] > 0) || !target_mask || !fusable) {
        dq::set_error("dq_dag_create: null pointer");
        return nullptr;
    }
    Dag* d = new Dag;
    d->n = n_ops;
    d->succ_off.assign(succ_off, succ_off + n_ops + 1);
    d->succ.assign(succ, succ + succ_off[n_ops]);
    d->targets.assign(target_mask, target_mask + n_ops);
    d->fusable.assign(fusable, fusable + n_ops);
    return d;
}

extern "C" void dq_dag_destroy(void* dag) { delete static_cast<Dag*>(dag); }

extern "C" int dq_dag_closure(void* dag, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, int* stuck,
                              int* nstuck, int* changed_idx, int* changed_val, int* nchanged) {
    if (!dag || !indeg || (nready > 0 && !ready)) {
        dq::set_error("dq_dag_closure: null pointer");
        return DQ_ERR_ARG;
    }
    const Dag& d = *static_cast<const Dag*>(dag);
    return closure(d, local_scratch(d.n), tile, cap, indeg, ready, nready, stuck, nstuck, changed_idx, changed_val, nchanged);
}

extern "C" int dq_dag_rank(void* dag, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, const int* cand,
                           int ncand, int* counts) {
    if (!dag || !indeg || (nready > 0 && !ready) || (ncand > 0 && (!cand || !counts))) {
        dq::set_error("dq_dag_rank: null pointer");
        return DQ_ERR_ARG;
    }
    const Dag& d = *static_cast<const Dag*>(dag);
    Scratch& sc = local_scratch(d.n);
    for (int c = 0; c < ncand; ++c)
        counts[c] = closure(d, sc, tile | (1ull << cand[c]), cap, indeg, ready, nready, nullptr, nullptr, nullptr, nullptr, nullptr);
    return DQ_OK;
}

// One growth step of fusion._grow_tile in one call: the dry run with `tile`, the qubits outside it that the gates left
// stuck at the front are waiting for (cand_q, with how many gates wait for each: cand_w), and for every such qubit the
// dry run with the tile plus that qubit (cand_count), each an extension of the first.  Returns the number of candidates;
// *base = gates retired with `tile`.
extern "C" int dq_dag_grow_step(void* dag, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, int* base,
                                int* cand_q, int* cand_w, int* cand_count) {
    if (!dag || !indeg || (nready > 0 && !ready) || !base || !cand_q || !cand_w || !cand_count) {
        dq::set_error("dq_dag_grow_step: null pointer");
        return DQ_ERR_ARG;
    }
    const Dag& d = *static_cast<const Dag*>(dag);
    Scratch& sc = local_scratch(d.n);
    *base = open_front(d, sc, tile, cap, indeg, ready, nready);
    int w[64] = {0}, order[64];
    int nq = front_wants(d, sc, tile, w, order);
    if (*base >= cap) nq = 0;
    for (int c = 0; c < nq; ++c) {
        cand_q[c] = order[c];
        cand_w[c] = w[order[c]];
        cand_count[c] = extend_front(d, sc, tile | (1ull << order[c]), cap, indeg, *base, false);
    }
    close_front(sc);
    return nq;
}

// ---------------------------------------------------------------------------------------------------------------------
// The whole beam search of fusion._plan_tiles in one call, optionally PRICED.
//
// The pass-cost model.  ONE place for its constants; fusion.py reads them through dq_plan_pass_ms.  A FULL pass of the headline
// (n = 28, batch 16, complex64: 68.7 GB moved) takes  max(11.1, 5.8 + 1.71e-3 * VALU instructions per tile)  milliseconds,
// and a pass that moves less -- behind |0..0>, or a smaller state -- that times its share of those bytes:
//     ms = bytes moved * max(FLOOR_MS_PER_BYTE, FIXED_MS_PER_BYTE + VALU_MS_PER_BYTE * VALU instructions per tile)
//  - slope and intercept: profiles/r05/pass_cost_model.txt, the straight line through the full passes of the headline above
//    the plateau (residual 0.24 ms rms);
//  - floor: profiles/r06/passes_headline.txt, the lightest full passes: 11.1 ms for 68.7 GB (6.2 TB/s).
// Nobody has measured them for complex128: its tile holds as many bytes as a complex64 tile (2^11 x 16 = 2^12 x 8), so the
// complex64 figures are used per byte as they stand.  The model leaves out what the last pass pays for restoring the
// canonical order (3 ms on the headline): every schedule has one such pass.
namespace {

constexpr double kHeadlineBytes = 68719476736.0;                 // 16 samples x 2^28 amplitudes x 8 bytes, read + written
constexpr double kFixedMsPerByte = 5.8 / kHeadlineBytes;
constexpr double kValuMsPerByte = 1.71e-3 / kHeadlineBytes;
constexpr double kFloorMsPerByte = 11.1 / kHeadlineBytes;
constexpr double kTileBytes = 32768.0;
// Layout changes (dq_plan_pass_ms_trips; the VALU count is then the one with controls outside the tile weighted,
// dq_wave_pass_cost_ctrl): what the thirteen full passes of the headline took beyond the line above, against the number of
// layout changes among their records (3, 4 or 5): 0.316 +- 0.061 ms each, nothing left over at 2.54 of them; residual of
// the model on those passes 0.36 -> 0.16 ms rms (profiles/r08/pass_cost_trips.txt).
constexpr double kTripMsPerByte = 0.316 / kHeadlineBytes;
constexpr double kTripNeutral = 2.54;

double pass_ms(double valu, double bytes_moved) {
    const double alu = kFixedMsPerByte + kValuMsPerByte * valu;
    return bytes_moved * (alu > kFloorMsPerByte ? alu : kFloorMsPerByte);
}


// random.Random(seed).randrange(n) of CPython for 0 <= seed < 2^32 and n < 2^32: MT19937 seeded by init_by_array with the
// one-word key {seed}; randrange(n) draws getrandbits(bit_length(n)) = next word >> (32 - k) until the value is below n.
struct PyRandom {
    uint32_t mt[624];
    int idx;
    explicit PyRandom(uint32_t seed) {
        mt[0] = 19650218u;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        int i = 1;
        for (int k = 624; k; --k) {         // (key length 1: j stays 0)
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + seed;
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        for (int k = 623; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
        idx = 624;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int k = 0; k < 624; ++k) {
                const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
    uint32_t randrange(uint32_t n) {
        const int k = 32 - __builtin_clz(n);
        uint32_t r;
        do r = next() >> (32 - k); while (r >= n);
        return r;
    }
};

struct Cand {
    int c, w, q;
};

struct PlanCtx {
    const Dag* d;
    const DqPlanParams* prm;
    PyRandom rng;
    Scratch sc, check;          // (check: the from-scratch counts of the self-check)
    std::vector<int> stuck, cidx, cval;
    PlanCtx(const Dag* d_, const DqPlanParams* p)
        : d(d_), prm(p), rng((uint32_t)p->seed), sc(d_->n), check(d_->n), stuck((size_t)d_->n + 1), cidx((size_t)d_->n + 1), cval((size_t)d_->n + 1) {}

    // (self-check: `count` and, where given, the open front against the dry run from scratch)
    void verify(uint64_t tile, const std::vector<int>& indeg, const std::vector<int>& ready, int count, bool front) {
        int ns = 0;
        const int want = closure(*d, check, tile, prm->cap, indeg.data(), ready.data(), (int)ready.size(), stuck.data(), &ns, nullptr, nullptr, nullptr);
        bool ok = want == count;
        if (ok && front && count < prm->cap) {
            std::vector<int> a(stuck.begin(), stuck.begin() + ns), b(sc.front);
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            ok = a == b;
        }
        ++g_compared;
        if (!ok) ++g_mismatch;
    }

    // fusion._grow_tile
    uint64_t grow(uint64_t low, int hcap, const std::vector<int>& indeg, const std::vector<int>& ready, bool jitter, bool has_prev,
                  uint64_t prev, int need, uint64_t start = 0) {
        const int cap = prm->cap;
        const bool checking = g_verify.load() != 0;
        uint64_t chosen = start;        // (qubits the tile must hold whatever the gates ask for)
        const uint64_t farmask = prm->far_bit < 64 ? ~((1ull << prm->far_bit) - 1ull) : 0ull;
        // the dry run of the tile so far stays open from one step to the next: every step only extends it
        int base = -1;
        while (__builtin_popcountll(chosen) < hcap) {
            const uint64_t tile = low | chosen;
            if (base < 0) base = open_front(*d, sc, tile, cap, indeg.data(), ready.data(), (int)ready.size());
            if (checking) verify(tile, indeg, ready, base, true);
            if (base >= cap) break;
            int w[64] = {0}, order[64];
            const int nq = front_wants(*d, sc, tile, w, order);
            const bool far_spent = prm->max_far >= 0 && __builtin_popcountll(chosen & farmask) >= prm->max_far;
            const bool only_prev = has_prev && hcap - __builtin_popcountll(chosen) <= need - __builtin_popcountll(chosen & prev);
            Cand cands[64];
            int nc = 0;
            for (int c = 0; c < nq; ++c) {
                const int q = order[c];
                if (far_spent && q >= prm->far_bit) continue;
                if (only_prev && !((prev >> q) & 1ull)) continue;
                cands[nc].q = q;
                cands[nc].w = w[q];
                cands[nc].c = extend_front(*d, sc, tile | (1ull << q), cap, indeg.data(), base, false);
                if (checking) verify(tile | (1ull << q), indeg, ready, cands[nc].c, false);
                ++nc;
            }
            if (!nc) break;
            // descending by (count, waiting gates, -qubit)
            std::sort(cands, cands + nc, [](const Cand& a, const Cand& b) {
                if (a.c != b.c) return a.c > b.c;
                if (a.w != b.w) return a.w > b.w;
                return a.q < b.q;
            });
            const int pick = jitter ? (int)rng.randrange((uint32_t)(nc < 3 ? nc : 3)) : 0;
            chosen |= 1ull << cands[pick].q;
            base = extend_front(*d, sc, low | chosen, cap, indeg.data(), base, true);
        }
        close_front(sc);
        if (has_prev) {
            uint64_t rest = prev & ~chosen;
            while (rest) {
                if (__builtin_popcountll(chosen & prev) >= need || __builtin_popcountll(chosen) >= hcap) break;
                chosen |= rest & (~rest + 1ull);
                rest &= rest - 1;
            }
        }
        return chosen;
    }
};

struct BeamState {
    int done;
    double ms;
    uint64_t zero;              // qubits still known to be |0> (priced search)
    std::vector<int> indeg, ready;
    std::vector<uint64_t> hist;
    uint64_t prev;
};

}  // namespace

extern "C" double dq_plan_pass_ms(double valu, double bytes_moved) { return pass_ms(valu, bytes_moved); }

extern "C" double dq_plan_pass_ms_trips(double valu, double bytes_moved, int trips) {
    return pass_ms(valu, bytes_moved) + bytes_moved * kTripMsPerByte * ((double)trips - kTripNeutral);
}

namespace {

// One beam search.
int plan_one(const Dag& d, const DqPlanParams* prm, const int* indeg, const int* ready, int nready,
             uint64_t* tiles_out, int max_tiles, double* model_ms) {
    if (prm->width < 1 || prm->branch < 1 || prm->hcap < 0 || prm->hcap + prm->free_low > 64 || (prm->priced && !prm->gate_valu) ||
        prm->seed < 0 || prm->seed > 0xffffffffll) {
        dq::set_error("dq_dag_plan: bad parameters");
        return DQ_ERR_ARG;
    }
    PlanCtx ctx(&d, prm);
    Scratch& sc = ctx.sc;
    const int cap = prm->cap, L = prm->free_low;
    const uint64_t lowmask = prm->low;
    std::vector<BeamState> beam(1), nxt;
    beam[0].done = 0;
    beam[0].ms = 0.0;
    beam[0].zero = prm->known_zero;
    beam[0].indeg.assign(indeg, indeg + d.n);
    beam[0].ready.assign(ready, ready + nready);
    beam[0].prev = lowmask;
    std::vector<int> retired((size_t)d.n + 1);
    for (;;) {
        nxt.clear();
        for (const BeamState& st : beam) {
            if (st.done >= d.n) {
                const int len = (int)st.hist.size();
                if (len > max_tiles) {
                    dq::set_error("dq_dag_plan: %d passes, room for %d", len, max_tiles);
                    return DQ_ERR_ARG;
                }
                for (int i = 0; i < len; ++i) tiles_out[i] = st.hist[i];
                if (model_ms) *model_ms = st.ms;
                return len;
            }
            uint64_t seen[128];
            int nseen = 0;
            const int nb = prm->width > 1 ? prm->branch : 1;
            for (int b = 0; b < nb && b < 64; ++b) {
                uint64_t bits, whole;
                if (L) {
                    bits = ctx.grow(0, prm->hcap + L, st.indeg, st.ready, b != 0, true, st.prev, L);
                    whole = bits;
                } else {
                    bits = ctx.grow(lowmask, prm->hcap, st.indeg, st.ready, b != 0, false, 0, 0);
                    whole = lowmask | bits;
                }
                bool dup = false;
                for (int k = 0; k < nseen; ++k) dup = dup || seen[k] == bits;
                if (dup) continue;
                seen[nseen++] = bits;
                int ns = 0, nc = 0, nret = 0;
                sc.retired = prm->priced ? retired.data() : nullptr;
                int count = closure(d, sc, whole, cap, st.indeg.data(), st.ready.data(), (int)st.ready.size(), ctx.stuck.data(), &ns,
                                    ctx.cidx.data(), ctx.cval.data(), &nc);
                if (prm->priced && L && st.done + count >= d.n && __builtin_popcountll(whole | lowmask) > prm->hcap + L) {
                    // this tile would end the circuit, but the LAST pass restores the canonical order and needs the qubits
                    // that belong on the contiguous low bits in its tile: no room for them here, so the tile is grown again
                    // around them (it may then leave gates for one more pass)
                    bits = ctx.grow(0, prm->hcap + L, st.indeg, st.ready, b != 0, true, st.prev, L, lowmask);
                    whole = bits;
                    dup = false;
                    for (int k = 0; k < nseen; ++k) dup = dup || seen[k] == bits;
                    if (dup) { sc.retired = nullptr; continue; }
                    seen[nseen++] = bits;
                    count = closure(d, sc, whole, cap, st.indeg.data(), st.ready.data(), (int)st.ready.size(), ctx.stuck.data(), &ns,
                                    ctx.cidx.data(), ctx.cval.data(), &nc);
                }
                sc.retired = nullptr;
                nret = count;
                nxt.emplace_back();
                BeamState& o = nxt.back();
                o.indeg = st.indeg;
                for (int k = 0; k < nc; ++k) o.indeg[ctx.cidx[k]] = ctx.cval[k];
                o.ready.assign(ctx.stuck.begin(), ctx.stuck.begin() + ns);
                o.hist = st.hist;
                o.ms = st.ms;
                o.zero = st.zero;
                if (count == 0) {       // nothing fusable at the front: the lowest ready gate runs on its own
                    int at = 0;
                    for (int k = 1; k < ns; ++k)
                        if (o.ready[k] < o.ready[at]) at = k;
                    const int i = o.ready[at];
                    o.ready.erase(o.ready.begin() + at);
                    for (int e = d.succ_off[i]; e < d.succ_off[i + 1]; ++e)
                        if (--o.indeg[d.succ[e]] == 0) o.ready.push_back(d.succ[e]);
                    o.done = st.done + 1;
                    o.hist.push_back(~0ull);
                    o.prev = st.prev;
                    if (prm->priced) {      // a gate on its own reads and writes the whole state
                        o.ms += pass_ms(0.0, 2.0 * kTileBytes * prm->tiles_full);
                        o.zero &= ~d.targets[i];
                    }
                    break;
                }
                o.done = st.done + count;
                o.hist.push_back(bits);
                o.prev = whole;
                if (prm->priced) {
                    // the estimate: per-gate costs by kind and mode + a fixed part per pass; the pass runs the tiles in which
                    // no known-|0> qubit outside its tile is 1 and reads, of each, what known-|0> qubits inside leave
                    double valu = prm->pass_valu;
                    uint64_t hit = 0;
                    for (int k = 0; k < nret; ++k) {
                        const int g_ = retired[k];
                        valu += prm->gate_valu[g_];
                        hit |= d.targets[g_];
                    }
                    const uint64_t z = st.zero & ~lowmask;
                    const int outside = __builtin_popcountll(z & ~whole), inside = __builtin_popcountll(z & whole);
                    const double tiles = prm->tiles_full / (double)(1ull << outside);
                    o.ms += pass_ms(valu, tiles * kTileBytes * (1.0 + 1.0 / (double)(1ull << inside)));
                    o.zero = st.zero & ~hit;        // known |0> until a non-diagonal gate targets it
                }
            }
        }
        if (prm->priced == 2) {
            // against a known rate (ms per gate of a schedule already in hand): the states that are the most AHEAD of it
            const double rate = prm->rate;
            std::stable_sort(nxt.begin(), nxt.end(), [rate](const BeamState& a, const BeamState& b) {
                const double ra = a.ms - rate * (double)a.done, rb = b.ms - rate * (double)b.done;
                if (ra != rb) return ra < rb;
                return a.done > b.done;
            });
        } else if (prm->priced)
            std::stable_sort(nxt.begin(), nxt.end(), [](const BeamState& a, const BeamState& b) {
                const double ra = a.ms * (double)b.done, rb = b.ms * (double)a.done;      // ms per retired gate, cross-multiplied
                if (ra != rb) return ra < rb;
                return a.done > b.done;
            });
        else
            std::stable_sort(nxt.begin(), nxt.end(), [](const BeamState& a, const BeamState& b) { return a.done > b.done; });
        if ((int)nxt.size() > prm->width) nxt.resize((size_t)prm->width);
        beam.swap(nxt);
        if (beam.empty()) {
            dq::set_error("dq_dag_plan: the beam ran empty");
            return DQ_ERR_ARG;
        }
    }
}

}  // namespace

extern "C" int dq_dag_plan(void* dag, const DqPlanParams* prm, const int* indeg, const int* ready, int nready, uint64_t* tiles_out,
                           int max_tiles, double* model_ms) {
    if (!dag || !prm || !indeg || (nready > 0 && !ready) || !tiles_out) {
        dq::set_error("dq_dag_plan: null pointer");
        return DQ_ERR_ARG;
    }
    return plan_one(*static_cast<const Dag*>(dag), prm, indeg, ready, nready, tiles_out, max_tiles, model_ms);
}

// Threads of dq_dag_plan_many: min(hardware threads, 16, searches); DQ_PLAN_THREADS overrides (1: one after the other).
extern "C" int dq_plan_threads(int nplans) {
    int t = (int)std::thread::hardware_concurrency();
    if (t < 1) t = 1;
    if (t > 16) t = 16;
    if (const char* e = getenv("DQ_PLAN_THREADS")) {
        const int v = atoi(e);
        if (v >= 1) t = v;
    }
    if (t > nplans) t = nplans;
    return t < 1 ? 1 : t;
}

extern "C" int dq_dag_plan_many(void* dag, const DqPlanParams* prms, int nplans, const int* indeg,
                                const int* ready, int nready, uint64_t* tiles_out, int max_tiles, int* counts, double* model_ms) {
    if (!dag || (nplans > 0 && (!prms || !tiles_out || !counts)) || !indeg || (nready > 0 && !ready) || nplans < 0 || max_tiles < 0) {
        dq::set_error("dq_dag_plan_many: null pointer");
        return DQ_ERR_ARG;
    }
    const Dag& d = *static_cast<const Dag*>(dag);
    // the searches are independent (each seeds its own generator from its own parameters) and every result goes to its own
    // place, so the outcome does not depend on how many threads share them out
    std::atomic<int> next{0};
    std::vector<std::string> errors((size_t)nplans);
    auto work = [&]() {
        for (int k = next++; k < nplans; k = next++) {
            try {
                counts[k] = plan_one(d, prms + k, indeg, ready, nready, tiles_out + (size_t)k * (size_t)max_tiles, max_tiles,
                                     model_ms ? model_ms + k : nullptr);
                if (counts[k] < 0) errors[(size_t)k] = dq_last_error();      // (the message lives in the worker's thread)
            } catch (const std::exception& e) {        // (out of memory: reported like any other failure, not thrown across a thread)
                counts[k] = DQ_ERR_ARG;
                try { errors[(size_t)k] = std::string("dq_dag_plan_many: ") + e.what(); } catch (...) {}
            } catch (...) {
                counts[k] = DQ_ERR_ARG;
            }
        }
    };
    const int nthreads = dq_plan_threads(nplans);
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < nthreads; ++t) pool.emplace_back(work);
    } catch (...) {     // (no more threads to be had: the ones there are, and this one, share the work)
    }
    work();
    for (std::thread& t : pool) t.join();
    for (int k = 0; k < nplans; ++k)
        if (counts[k] < 0) {
            dq::set_error("%s (search %d)", errors[(size_t)k].c_str(), k);
            return counts[k];
        }
    return DQ_OK;
}

extern "C" int64_t dq_dag_plan_verify(int enable, int64_t* compared) {
    g_verify.store(enable ? 1 : 0);
    if (compared) *compared = (int64_t)g_compared.load();
    const int64_t bad = (int64_t)g_mismatch.load();
    if (enable) {
        g_compared.store(0);
        g_mismatch.store(0);
    }
    return bad;
}
