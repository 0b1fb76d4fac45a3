/*
 * dq_hip.h -- C ABI of libdqhip.so, the MI355X (gfx950) statevector backend.
 *
 * This is the drop-in boundary for the QubitCircuit hot path of TuringQ/deepquantum.  The
 * reference has no FFI of its own (it is pure Python/PyTorch); every entry point below replaces
 * one Python-level seam of the reference, cited as <file:line> relative to the reference tree
 * (src/deepquantum/...).  The Python host (deepquantum_amd/_lib.py) binds these with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *   - All data pointers are DEVICE pointers unless the parameter is documented "host".
 *   - A state is `batch` contiguous vectors of 2^n interleaved complex numbers
 *     (c64 = 2 x float, c128 = 2 x double), index bit p <-> wire (n-1-p): wire 0 is the most
 *     significant bit of the flat amplitude index (operation.py:45-55, qmath.py:497-505).
 *   - `targets`/`controls` are bit positions (LSB = 0), host arrays.  targets[0] is the MOST
 *     significant bit of the gate-matrix index (qmath.py:502-503, wires[0] = matrix MSB).
 *   - Gate matrices are row-major 2^k x 2^k complex in the state's precision, DEVICE memory,
 *     `mat_batch_stride` = elements (complex numbers) between the matrices of consecutive batch
 *     samples (0 = one matrix shared by the whole batch; this is the vmap case of
 *     circuit.py:232-240).
 *   - Every call enqueues on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     returns without synchronising.  The library keeps no device memory and no global mutable
 *     state besides a thread-local error string; it is re-entrant.  The one exception is an A/B MEASUREMENT
 *     knob, not part of the data path's contract: dq_set_dense_path sets a process-wide (atomic) integer that
 *     later launches of every thread read; results never depend on it.
 *   - Return value: DQ_OK (0) or a negative DqStatus; dq_last_error() describes the failure.
 *     No exception crosses the ABI.
 */
#ifndef DQ_HIP_H
#define DQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dq_stream_t; /* hipStream_t */

typedef enum {
    DQ_OK = 0,
    DQ_ERR_ARG = -1,         /* invalid argument (bad bit index, overlap, null pointer, ...) */
    DQ_ERR_LAUNCH = -2,      /* HIP runtime reported an error at launch */
    DQ_ERR_UNSUPPORTED = -3  /* valid request outside what this build implements */
} DqStatus;

#define DQ_ABI_VERSION 30

int dq_abi_version(void);
/* Thread-local, never NULL. */
const char* dq_last_error(void);
/* What the compiled library believes the descriptor structs below look like: sizeof(DqFusedGate), sizeof(DqFusedRound),
 * sizeof(DqFusedPass), then the offsets of DqFusedPass::rounds, gates, load_slot_off, store_high_pos, store_tb,
 * slots -- at most `max` values written to `out`; returns how many there are.  Lets a binding check its own struct
 * definitions against the library instead of against numbers typed in by hand. */
int dq_struct_layout(int* out, int max);
/* Fills CU count, LDS bytes per workgroup, total global memory of the current device. */
int dq_device_info(int* cu_count, int64_t* lds_per_block, int64_t* global_mem);

/* ------------------------------------------------------------------------------------------
 * 1. Single gate application.  Replaces qmath.evolve_state (qmath.py:485-506) and
 *    Gate.op_state_control (operation.py:203-219): psi' = (U on targets, conditioned on all
 *    controls = 1) psi.  in == out is allowed (each amplitude group is private to one thread)
 *    when k <= 4; for k > 4, in and out must not alias.  k <= 10.
 * ------------------------------------------------------------------------------------------ */
int dq_apply_gate_c64(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                      const int* targets, int k, const int* controls, int nc, int64_t batch,
                      dq_stream_t stream);
int dq_apply_gate_c128(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                       const int* targets, int k, const int* controls, int nc, int64_t batch,
                       dq_stream_t stream);

/* Dense gates on 5..10 targets run as a GEMM on the matrix cores (csrc/dq_dense.hip; exact f32 / f64 MFMA).  A/B knob:
 * 0 = the round-1 kernel (one thread per output amplitude, VALU), 1 = MFMA (default). */
int dq_set_dense_path(int mfma);

/* ------------------------------------------------------------------------------------------
 * 2. Fused pass.  Replaces a run of consecutive Gate.forward calls inside
 *    nn.Sequential(self.operators) (circuit.py:261, operation.py:274-289): one HBM read + one HBM
 *    write of the state applies every gate of the pass.  A pass owns `m` "tile" index bits: the
 *    low `L` bits (contiguous, for coalescing) plus `h = m - L` gathered high bits; each
 *    workgroup stages one 2^m tile (registers + LDS) and walks the pass's rounds.  A round names
 *    R register-slot bits (tile-local positions); gates of the round act on register slots.
 *    The host scheduler (deepquantum_amd/fusion.py) builds these descriptors.
 *
 *    Geometry (dq_fused_geometry): the WAVE TILE.  complex64: m = 12, 6 register slots; complex128: m = 11, 5 slots;
 *    64 threads: ONE wavefront owns a tile (64 lanes x 64 / 32 amplitudes in registers), a workgroup is four
 *    independent waves, and a pass has no workgroup barrier at all; a layout change between rounds goes through a small
 *    wave-private LDS buffer.  The library derives everything below the level of "which tile bits are register slots
 *    in which round" itself (csrc/dq_wave.hip translates the descriptor into the kernel's records): the order of a
 *    round's slots and of its thread bits is the host's to choose freely.  Every DqFusedKind below runs there, in both
 *    precisions.  (ABI <= 20 also had workgroup-tile geometries -- m = 13 / 12 with 4 slots, 512 / 256 threads, the
 *    tile staged in LDS between rounds -- with handler ids, LDS offset tables and in-wave exchange records in this
 *    descriptor; they went with ABI 21.)
 * ------------------------------------------------------------------------------------------ */
#define DQ_FUSED_MAX_HIGH 12
#define DQ_FUSED_MAX_LOW 8      /* contiguous low tile bits: L <= 8 */
#define DQ_FUSED_MAX_ROUNDS 24
#define DQ_FUSED_MAX_GATES 128   /* (ABI <= 23: 80) */
#define DQ_FUSED_MAX_SLOTS 6

typedef enum {
    DQ_FG_GEN1 = 0,  /* general 2x2 on register slot q                       */
    DQ_FG_X1 = 1,    /* Pauli-X / CNOT / Toffoli: swap the pair of slot q     */
    DQ_FG_DIAG1 = 2, /* diagonal 2x2 (Z,S,T,Rz,P,CZ...) target anywhere      */
    DQ_FG_GEN2 = 3,  /* general 4x4 on register slots q (matrix MSB) and q2 */
    DQ_FG_DIAG2 = 4, /* diagonal 4x4 (Rzz...) both targets anywhere           */
    DQ_FG_RESERVED5 = 5, /* (ABI <= 20: an in-wave exchange record of the workgroup-tile kernels; refused) */
    DQ_FG_GRAD = 6,  /* not a gate: a reduction for the reverse sweep of the adjoint method (dq_apply_fused_grad_c64 / _c128).
                        The state is psi and the cotangent lambda side by side along ONE extra index bit (register slot
                        q2: 0 = psi, 1 = lambda); the record adds  G[a][b] = sum lambda[target = a] conj(psi[target = b])
                        (target = register slot q; the sum runs over everything else, restricted to the controls being
                        1) to row `reserved` of the caller's accumulator.  No matrix, no handler id.
                        `loc` says which of the eight real sums the record forms:
                        0 all; 1 Re G only (the trainable gate's matrix is real); 2 Re (G00 + G11), left in Re G00, and
                        Im (G01 + G10), left in Im G01 (a matrix a I + i b X: a Pauli-X rotation); 3 G00 and G11 only
                        (a diagonal matrix); 4 Im (G01 + G10) alone, left in Im G01 (a UNITARY a I + i b X whose gradient
                        is only ever taken along the rotation: the trace part cancels).  The OTHER components of the row are left untouched -- nothing is added to
                        them, so a caller that zeroed the accumulator reads zeros there and may use the whole row in
                        linear algebra (executor._first_order multiplies the 2x2 row by U^-dagger) */
    DQ_FG_EXPZ = 7   /* not a gate: the expectation value of a Z string taken from the registers, so that a circuit's
                        <Z..Z> observables cost no extra read of the state (replaces qmath.expectation qmath.py:830-860
                        for Z-type observables): adds  sum_i (-1)^popc(i & zmask) |a_i|^2  to component 0 of row
                        `reserved` of the accumulator of a dq_apply_fused_grad_* call.  The Z bits are given like
                        controls: reg_cmask (register slots), thr_cmask (tile-local bits on lanes), out_cmask (index
                        bits outside the tile).  Wave-tile geometries only.  No matrix */
} DqFusedKind;

typedef enum { DQ_LOC_REG = 0, DQ_LOC_THR = 1, DQ_LOC_OUT = 2 } DqBitLoc;

/* Structure of a GEN1 matrix, promised by the host from the gate class (never from values: that would
 * need a device sync): the kernel skips the multiplications by the exact zeros. */
typedef enum {
    DQ_MODE_GENERAL = 0,
    DQ_MODE_REAL = 1, /* all four entries real: H, Ry, X, Z ... */
    DQ_MODE_RX = 2,   /* a I + i b X (a, b real): Rx and products of such.  For an UNCONTROLLED gate of this mode in a
                         complex64 pass (fast id 8..11) the caller hands over, in place of the matrix, the block
                         { (f_re, f_im), (0, t), (-, -), (flag, -) }:  f = a and t = b / a, flag = 0  if |a| >= |b|,
                         f = i b and t = -a / b, flag = 1  otherwise -- the kernel applies [[1, it], [it, 1]]
                         resp. [[it, 1], [1, it]] (three packed operations per amplitude pair instead of four) and
                         multiplies the pass's deferred scalar by f (fusion.defer_rx builds the block) */
    DQ_MODE_HAD = 3,  /* s * [[1, 1], [1, -1]], s real: Hadamard.  The kernel takes sums and differences and
                         applies the product of the factors s of a pass once, at its end */
    DQ_MODE_XREAL = 4, /* GEN2 only (ABI 24): a REAL 4x4 matrix that is non-zero only where the parities of the row and
                         the column index agree -- a 2x2 block on (00, 11) and one on (01, 10).  The superoperator
                         sum K (x) conj(K) of every non-diagonal channel of channel.py:16-383 (bit flip, bit-phase flip,
                         depolarizing, Pauli, amplitude damping, generalized amplitude damping) on the (row, column) bit
                         pair of its wire.  The other entries are never read */
    DQ_MODE_XCPLX = 5 /* GEN2 only (ABI 24): the same shape -- a 2x2 block on (00, 11), one on (01, 10) -- with COMPLEX
                         entries: exp(-i theta XX / 2), exp(-i theta YY / 2), exp(-i theta (XX + YY) / 4)
                         (gate.py:2085-2390) and their controlled forms */
} DqFusedMode;

typedef struct {
    uint8_t kind;       /* DqFusedKind */
    uint8_t q;          /* GEN/X: register slot of the (first) target; DIAG: position per loc */
    uint8_t q2;         /* GEN2: slot of the second target (matrix LSB); DIAG2: position per loc2 */
    uint8_t loc;        /* DIAG1/2: DqBitLoc of target 1 (REG: q = slot, THR: q = tile-local bit,
                           OUT: q = global bit position); GEN1: DqFusedMode of the matrix; GEN2: GENERAL or
                           REAL (real 4x4, exact zeros skipped: channel superoperators) */
    uint8_t loc2;       /* DIAG2: same for target 2 */
    uint8_t reg_cmask;  /* controls that are register slots (bit s = slot s) */
    uint16_t thr_cmask; /* controls that are thread bits (tile-local bit positions) */
    uint32_t mat;       /* offset (in complex numbers) of this gate's matrix inside `mats` */
    uint32_t fast;      /* must be DQ_FAST_NONE (ABI <= 20: handler id of the workgroup-tile kernels' jump table) */
    uint64_t out_cmask; /* controls outside the tile (global bit positions) */
    uint32_t mat_advance; /* complex numbers this gate occupies in `mats` (0 for X1): the matrices of a pass
                             lie back to back in gate order, mat(i+1) = mat(i) + mat_advance(i), so the kernel
                             fetches gate i's matrix together with its record instead of after decoding it */
    uint32_t reserved;  /* DQ_FG_GRAD, DQ_FG_EXPZ: row of the accumulator; otherwise 0 (pads the record to 32 bytes: one
                           s_load_dwordx8 per gate) */
} DqFusedGate;          /* 32 bytes */
#define DQ_FAST_NONE 0xFFFFFFFFu
/* `mats` must be readable for DQ_MAT_PAD complex numbers past the last matrix of a pass (prefetch). */
#define DQ_MAT_PAD 16

#define DQ_FUSED_MAX_TBITS 9
#define DQ_FUSED_MAX_BLK 24      /* block-index bits: n - m <= 24 */
typedef struct {
    uint8_t rb[DQ_FUSED_MAX_SLOTS]; /* tile-local bit position of register slot s (any order; the I/O layouts of the
                                       pass header are ascending) */
    uint8_t tb[DQ_FUSED_MAX_TBITS]; /* tile-local bit position of thread-index bit i (the other m - slots
                                       tile bits, in an order the host picks to avoid LDS bank conflicts) */
    uint8_t flags;                  /* DQ_ROUND_TRANSPOSE: the layout (rb, tb) differs from the one the registers are in
                                       when the round starts (the previous round's, or the load layout for round 0);
                                       DQ_ROUND_TRANSPOSE_AFTER (last round only): it differs from the store layout.
                                       dq_apply_fused_* recomputes and checks them. */
    uint8_t gate_begin, gate_end;   /* [begin, end) into gates[] */
} DqFusedRound;                     /* 18 bytes */
#define DQ_ROUND_TRANSPOSE 0x01u
#define DQ_ROUND_TRANSPOSE_AFTER 0x02u

typedef struct {
    uint8_t m, L, h, nrounds;
    uint8_t high_pos[DQ_FUSED_MAX_HIGH];        /* global bit of tile bit L+i, any order */
    uint8_t high_sorted[DQ_FUSED_MAX_HIGH];     /* the same positions ascending (tile -> base) */
    /* Register slots (tile-local, ascending) of the layouts used for the global load and the global
     * store.  An I/O layout keeps tile bit 0 as slot 0 for c64 (16 B per lane) and otherwise only
     * gathered bits (>= L) as slots; its thread bits are the remaining tile bits in ascending order,
     * so a wave instruction always moves >= 2^L contiguous amplitudes. */
    uint8_t load_rb[DQ_FUSED_MAX_SLOTS];
    uint8_t store_rb[DQ_FUSED_MAX_SLOTS];
    DqFusedRound rounds[DQ_FUSED_MAX_ROUNDS];
    uint32_t mat_base;                          /* = gates[0].mat (also aligns gates[] to 32 bytes) */
    DqFusedGate gates[DQ_FUSED_MAX_GATES];
    /* Host-precomputed addressing of the two I/O layouts: offset (in amplitudes, inside one state) that
     * register slot s contributes, i.e. 2^(global bit of tile bit load_rb[s]); saves the kernel a scalar
     * loop per slot per tile. */
    uint64_t load_slot_off[DQ_FUSED_MAX_SLOTS];
    uint64_t store_slot_off[DQ_FUSED_MAX_SLOTS];
    /* Where the pass WRITES.  A pass may store its tile -- and its block index -- to other index bits (>= L) than
     * it read them from: a bit permutation of the state on the way out, so that the qubits of the NEXT pass already
     * sit in cheap (near) positions when that pass gathers them (scattered writes are nearly free on this memory
     * system, gathered reads are not: DESIGN.md).  store_high_pos[i] = global bit that tile bit L + i is written
     * to; store_blk_pos[j] = global bit that bit j of the block index (= the j-th lowest non-tile bit on the READ
     * side) is written to.  Together a permutation of [L, n).  In-place passes (in == out) must use the read
     * positions (store_high_pos == high_pos, store_blk_pos ascending): anything else needs in != out.
     * store_slot_off is in write positions. */
    uint8_t store_high_pos[DQ_FUSED_MAX_HIGH];
    uint8_t store_blk_pos[DQ_FUSED_MAX_BLK];
    /* The low tile bits move too: tile bit i < L is written to global bit store_low_pos[i] (identity for an in-place
     * pass), so that the NEXT pass may find other qubits on its contiguous low bits -- every pass then chooses all m
     * tile qubits freely instead of sharing L fixed ones with every other pass, provided the qubits it wants on its low
     * bits were in the tile of the pass before (which must write them as contiguous runs).  store_low_pos,
     * store_high_pos and store_blk_pos together are a permutation of [0, n).  The store layout is explicit for the
     * same reason: register slots store_rb (any tile bits; complex64: the tile bit of slot 0 must be written to
     * global bit 0, a lane stores two adjacent amplitudes) and thread bits store_tb (the other tile bits; the host
     * puts the tile bits written to global bits 1 .. L-1 on the lowest lane bits: 128 contiguous bytes per 8 lanes). */
    uint8_t store_low_pos[DQ_FUSED_MAX_LOW];
    uint8_t store_tb[DQ_FUSED_MAX_TBITS];
    uint8_t slots;                              /* register slots per thread of the geometry the pass was planned for
                                                   (dq_fused_geometry); with m it selects the kernel */
} DqFusedPass;

/* The tile geometry of each precision (m = slots + log2(threads)): variant 0; DQ_ERR_ARG for any other. */
int dq_fused_geometry(int is_c128, int variant, int* m, int* slots, int* threads);
/* Host-side core of the pass planner (no device code; deepquantum_amd/fusion.py drives it): dry runs of a pass over the
 * commutation DAG of a gate list.  dq_dag_create copies the DAG: successors of gate i = succ[succ_off[i] .. succ_off[i+1]),
 * target_mask[i] = the qubits gate i needs inside the tile (0: it runs anywhere, e.g. a diagonal gate), fusable[i] = may it
 * enter a fused pass at all.  dq_dag_closure retires, depth-first from the `ready` gates, every fusable gate whose
 * targets lie in `tile` (bit mask over qubits) while fewer than `cap` have retired; returns how many did, and optionally
 * the gates left stuck at the front and the in-degrees it changed (index / value pairs; `indeg` itself is not written).
 * dq_dag_rank does the count for tile | (1 << cand[c]), every c.  A handle is not thread-safe (it carries scratch). */
void* dq_dag_create(int n_ops, const int* succ_off, const int* succ, const uint64_t* target_mask, const uint8_t* fusable);
void dq_dag_destroy(void* dag);
int dq_dag_closure(void* dag, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, int* stuck, int* nstuck,
                   int* changed_idx, int* changed_val, int* nchanged);
int dq_dag_rank(void* dag, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, const int* cand, int ncand,
                int* counts);
/* One growth step of a tile: *base = dq_dag_closure(tile); the qubits outside the tile that the stuck gates wait for
 * (cand_q, cand_w = how many gates wait for each; arrays of 64), and cand_count = dq_dag_closure(tile | qubit) for each.
 * Returns the number of candidates (0 when the pass is full: *base >= cap). */
int dq_dag_grow_step(void* dag, uint64_t tile, int cap, const int* indeg, const int* ready, int nready, int* base, int* cand_q,
                     int* cand_w, int* cand_count);
/* ABI 29.  The whole beam search over tiles in one call (fusion._plan_tiles: every beam state -- a front of the DAG -- is
 * extended by the greedy tile and by branch - 1 randomised ones, `width` states survive), from the front (indeg, ready).
 * Writes one mask per pass to tiles_out -- the gathered qubits, or with free_low = L > 0 the WHOLE tile, which then shares
 * at least L qubits with the tile before (the first with `low`); ~0 = a gate that runs on its own -- and returns how many.
 * priced = 0: the states that have retired the most gates survive (the tile lists of the Python search, seed for seed).
 * priced = 1: a state also carries modelled milliseconds (dq_plan_pass_ms), and the states with the least modelled time per
 * retired gate survive (equal: more gates).  A tile's price there is an estimate: pass_valu + the gate_valu of the gates it
 * retires for the VALU side, and for the memory side the qubits of `known_zero` that no non-diagonal gate has targeted yet
 * -- outside the tile each halves the tiles that run, inside it each halves what a tile reads.  tiles_full = tiles of a
 * full pass (all samples).  *model_ms (may be NULL) = the estimate for the returned plan. */
typedef struct DqPlanParams {
    uint64_t low;        /* the contiguous low qubits */
    uint64_t known_zero; /* priced: qubits known to be |0> in the input */
    int64_t seed;        /* of the randomised branches, 0 .. 2^32 - 1 */
    int32_t hcap, cap, width, branch;
    int32_t far_bit, max_far; /* at most max_far gathered qubits >= far_bit; max_far < 0: no limit */
    int32_t free_low, priced;
    const float* gate_valu; /* priced: VALU instructions per tile of every gate (dq_wave_gate_valu) */
    double pass_valu;       /* priced: ... of a pass's layout changes */
    double tiles_full;
    double rate; /* priced = 2: milliseconds per gate of a schedule in hand; the states most ahead of that rate survive */
} DqPlanParams;
int dq_dag_plan(void* dag, const DqPlanParams* prm, const int* indeg, const int* ready, int nready, uint64_t* tiles_out,
                int max_tiles, double* model_ms);
/* Several beam searches in ONE call, shared out among threads (dq_plan_threads): search k takes prms[k] and writes its
 * masks to tiles_out[k * max_tiles ..], how many to counts[k] and its estimate to model_ms[k] (may be NULL).  The searches
 * are independent and each result has its own place, so the outcome is the same for any number of threads.  The DAG is only
 * read.  Returns 0, or the status of the first search that failed (also when one ran out of memory). */
int dq_dag_plan_many(void* dag, const DqPlanParams* prms, int nplans, const int* indeg,
                     const int* ready, int nready, uint64_t* tiles_out, int max_tiles, int* counts, double* model_ms);
/* Threads dq_dag_plan_many uses for `nplans` searches: min(hardware threads, 16, nplans); the environment variable
 * DQ_PLAN_THREADS overrides the first two (1: one search after the other). */
int dq_plan_threads(int nplans);
/* Test hook.  The searches extend the dry run of a growing tile instead of repeating it; while enabled every count (and
 * the front, where one is kept) is ALSO taken from scratch and compared.  Returns the mismatches so far and writes the
 * comparisons made to *compared (may be NULL); enable != 0 then restarts both counts.  The switch and the counts are
 * process-wide: searches of other threads that run meanwhile are compared and counted too. */
int64_t dq_dag_plan_verify(int enable, int64_t* compared);
/* The pass-cost model (constants and their sources: csrc/dq_plan.hip): milliseconds of a wave-tile pass that executes `valu`
 * VALU instructions per tile and moves `bytes_moved` bytes (all samples together). */
double dq_plan_pass_ms(double valu, double bytes_moved);
/* ... and with the term for `trips` layout changes among the pass's records (dq_wave_pass_cost_ctrl). */
double dq_plan_pass_ms_trips(double valu, double bytes_moved, int trips);

/* The deferred form of the uncontrolled Rx-like gates of a complex64 pass (DQ_MODE_RX above), in place, in the matrix
 * buffer the passes will read: for every sample b < batch and every k < count the block of four complex numbers at
 * mats[b * mat_batch_stride + index[k]] -- { a, i b, i b, a } of the matrix a I + i b X -- becomes { f, i t, -, flag }.
 * `index`: DEVICE array of int64 offsets (complex numbers), e.g. fusion.rx_defer_positions of a schedule.  One launch;
 * host code that prepares matrix buffers for dq_apply_fused_c64 itself calls this instead of re-deriving the form
 * (no reference counterpart: the reference multiplies by the full matrix, gate.py:1443-1448). */
int dq_defer_rx_c64(void* mats, int64_t mat_batch_stride, const int64_t* index, int64_t count, int64_t batch,
                    dq_stream_t stream);

/* Test hook, no device needed: the kernel-side descriptor the library derives for a wave-tile pass (`pass`: HOST
 * pointer, complex64, m = 12, 6 slots) as raw bytes -- 80 bytes of slot offsets (load, store: 5 x 8 each), 6 + 6 + 6
 * words (byte shift of every lane bit on the load side / the store side, what it adds to the thread's tile-local base),
 * record bytes, matrix base, 24 + 24 index positions of the tile number's bits (read, write), one word for
 * dq_apply_fused_zext_* (`known_zero`; bits 0..5: how many bits the tile number has, 8..13 / 16..21: register slots /
 * lane bits that are not loaded), 2 + 2 words for dq_apply_fused_slice_* (index bits held fixed, OR-ed into every tile's
 * read / write base; zero here) + 3 reserved words, then the 32-byte records (word 0 = handler id, csrc/dq_wave_asm.inc).  At most `max_bytes` are copied to `out` (may be NULL); returns the size,
 * or a negative DqStatus.  tests/_wave_emulator.py executes such a descriptor on the CPU. */
int dq_wave_descriptor(const DqFusedPass* pass, int n, uint64_t known_zero, void* out, int max_bytes);
/* ABI 29, no device needed: what the pass-cost model needs to know of `pass` run on a state whose index bits `known_zero`
 * (read side) are |0>.  *valu = VALU instructions a wave executes per tile: the generated per-handler table
 * (dq_wave_handler_valu) summed over the pass's records; *bytes_moved = bytes read + written PER SAMPLE, from the
 * descriptor's zero-extension word: the tiles that run are written whole and read less what known-|0> bits inside the tile
 * leave unloaded.  Either may be NULL. */
int dq_wave_pass_cost(const DqFusedPass* pass, int n, uint64_t known_zero, int64_t* valu, double* bytes_moved);
/* No device needed: dq_wave_pass_cost's count with every one-target gate or X record whose controls lie OUTSIDE the tile
 * weighted by the share of the tiles that execute its body (the kernel branches round it elsewhere): a half per control bit not in
 * `known_zero`; *trips = the layout changes among the pass's records.  Either may be NULL. */
int dq_wave_pass_cost_ctrl(const DqFusedPass* pass, int n, uint64_t known_zero, double* valu, int* trips);
/* One entry of that table (tools/gen_wave_asm.py, gen_wave_asm64.py: handler_valu); -1 for an id the kernel does not have. */
int dq_wave_handler_valu(int is_c128, int id);
/* The planner's per-gate estimate: the table's entry for a gate of `opclass` on a middle slot -- 0 diagonal, 1 + mode a
 * 2x2 matrix without controls (mode 0 .. 3), 5 a 2x2 matrix with controls, 6 X, 7 X with controls, 8 a layout change of the
 * widest kind; -1 otherwise. */
int dq_wave_gate_valu(int is_c128, int opclass);
/* `pass` is a HOST pointer; it is copied into the kernel argument segment.  in == out allowed.
 * Requires n >= pass->m. */
int dq_apply_fused_c64(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                       int64_t batch, const DqFusedPass* pass, dq_stream_t stream);
int dq_apply_fused_c128(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                        int64_t batch, const DqFusedPass* pass, dq_stream_t stream);
/* Same, with `in` = ONE state of 2^n amplitudes shared by all `batch` outputs (in != out): the first pass of a
 * batched circuit reads the initial state directly, where the reference's vmap (circuit.py:238) materialises a
 * copy per sample. */
int dq_apply_fused_bcast_c64(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                             int64_t batch, const DqFusedPass* pass, dq_stream_t stream);
int dq_apply_fused_bcast_c128(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                              int64_t batch, const DqFusedPass* pass, dq_stream_t stream);

/* Same pass on an input in which the index bits of `known_zero` (bit mask, READ side of the pass) are known to be |0>:
 * the circuit's own initial state |0..0> (the reference's default, circuit.py:49 `init_state='zeros'`) and the passes
 * right behind it, while the qubits the circuit has not touched yet still factor out as |0>.
 *   - `in` is not read where one of these bits is 1; it need not be initialised there.  Inside the tile the registers of
 *     those halves are zero; tiles in which a known-zero bit OUTSIDE the tile is 1 are all zero and are skipped: neither
 *     read, computed nor written.
 *   - `out` is therefore left untouched where a known-zero bit outside the tile is 1 (at the position the pass writes that
 *     bit to): those bits are still known zero for the next pass; the tile's own bits are not any more.
 *   - none of the pass's L contiguous low bits may be named (a lane loads them in one piece), nor a bit >= n.
 * in_batch_stride: 2^n, or 0 = ONE input state shared by all `batch` outputs (as dq_apply_fused_bcast_*).
 * The first pass of the 28-qubit headline circuit then touches one tile per sample, the second 2^8, the third is
 * write-only: three of nineteen passes for the price of the third one's stores (deepquantum_amd/fusion.py,
 * zero_state_masks). */
int dq_apply_fused_zext_c64(const void* in, int64_t in_batch_stride, void* out, const void* mats, int64_t mat_batch_stride,
                            int n, int64_t batch, const DqFusedPass* pass, uint64_t known_zero, dq_stream_t stream);
int dq_apply_fused_zext_c128(const void* in, int64_t in_batch_stride, void* out, const void* mats, int64_t mat_batch_stride,
                             int n, int64_t batch, const DqFusedPass* pass, uint64_t known_zero, dq_stream_t stream);

/* ABI 25.  ONE SLICE of a pass: only the tiles whose index bits `slice_mask` (read side) equal `slice_value` run;
 * 2^popcount(slice_mask) such launches are the whole pass, bit for bit.  `slice_mask` names index bits < n OUTSIDE the
 * tile of the pass (not its contiguous low bits, not its gathered bits) and outside `known_zero`; `slice_value` is a subset
 * of it.  Gates controlled by such a bit see its value.  For the index-bit-sharded state (distributed.py:57-202 of the
 * reference exchanges whole shards gate by gate): the last pass in front of a k-qubit exchange is launched slice by
 * slice -- each slice's part of every chunk leaves for its peer while the next slice computes -- and the first pass
 * behind it starts with the first slice that has arrived. */
int dq_apply_fused_slice_c64(const void* in, int64_t in_batch_stride, void* out, const void* mats, int64_t mat_batch_stride,
                             int n, int64_t batch, const DqFusedPass* pass, uint64_t known_zero, uint64_t slice_mask,
                             uint64_t slice_value, dq_stream_t stream);
int dq_apply_fused_slice_c128(const void* in, int64_t in_batch_stride, void* out, const void* mats, int64_t mat_batch_stride,
                              int n, int64_t batch, const DqFusedPass* pass, uint64_t known_zero, uint64_t slice_mask,
                              uint64_t slice_value, dq_stream_t stream);

/* Reverse sweep of the adjoint method in fused passes (replaces the backward of autograd through circuit.py:261, one
 * matmul backward per gate -- qmath.py:504 -- with one saved state per gate).  `in` / `out` hold, per sample, psi and
 * the cotangent lambda as ONE state of n index bits in which one bit tells them apart; the pass un-applies gates from
 * both at once (the caller supplies the adjoint matrices) and its DQ_FG_GRAD records reduce, at the right moments of
 * the sweep, sum lambda (x) conj(psi) onto a trainable gate's target.  `grads` = DEVICE double [batch, ngrads, 8],
 * ADDED to (the caller zeroes it once per sweep): row r = Re, Im of G[0][0], G[0][1], G[1][0], G[1][1] of the record
 * with reserved = r.  Workgroups accumulate in LDS over their tiles (float32 sums for complex64, float64 for
 * complex128) and add to `grads` once.  complex128: wave-tile geometry only (m = 11, 5 slots). */
int dq_apply_fused_grad_c64(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                            int64_t batch, const DqFusedPass* pass, double* grads, int64_t ngrads, dq_stream_t stream);
int dq_apply_fused_grad_c128(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n,
                             int64_t batch, const DqFusedPass* pass, double* grads, int64_t ngrads, dq_stream_t stream);

/* ABI 24: a pass with more records than the kernel-argument segment holds (112: gates and reductions, two or four per
 * layout change).  A reverse sweep has a reduction in front of every trainable gate, and what bounded its passes was
 * the NUMBER of records, not the tile: the 28-qubit training step takes 23 passes of up to 104 instead of 32 of up to 72.
 * The kernel reads such a pass's records from DEVICE memory:
 *   dq_wave_records   (host, no GPU needed) writes the records of `pass` as the kernel reads them -- 32 bytes each -- to
 *                     the HOST buffer `out` (at most max_bytes; out = NULL: none) and returns their size in bytes, or a
 *                     negative DqStatus;
 *   dq_apply_fused_grad_ext_*   run the pass with those records at the DEVICE address `records` (the caller copied them
 *                     there; `records_bytes` must be what dq_wave_records returned for this pass and n).  They must stay
 *                     valid until the pass has run -- captured in a HIP graph: until its last replay.
 * Everything else as dq_apply_fused_grad_*. */
int64_t dq_wave_records(const DqFusedPass* pass, int n, void* out, int64_t max_bytes);
int dq_apply_fused_grad_ext_c64(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n, int64_t batch,
                                const DqFusedPass* pass, const void* records, int64_t records_bytes, double* grads,
                                int64_t ngrads, dq_stream_t stream);
int dq_apply_fused_grad_ext_c128(const void* in, void* out, const void* mats, int64_t mat_batch_stride, int n, int64_t batch,
                                 const DqFusedPass* pass, const void* records, int64_t records_bytes, double* grads,
                                 int64_t ngrads, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 3. Reductions.  Results are written to DEVICE memory in double precision.
 *    `ws` is a caller-owned device workspace of at least dq_reduce_ws_bytes(batch) bytes.
 * ------------------------------------------------------------------------------------------ */
int64_t dq_reduce_ws_bytes(int64_t batch);

/* out[b] = Re <psi_b| P |psi_b>, P = Pauli string given as bit masks (a Y sets its bit in both
 * xmask and zmask).  Replaces qmath.expectation (qmath.py:830-860) + Observable.forward
 * (layer.py:127-165): one read of the state instead of one gate pass per Pauli factor + bmm. */
int dq_expect_pauli_c64(const void* psi, uint64_t xmask, uint64_t zmask, int n, int64_t batch,
                        double* out, void* ws, dq_stream_t stream);
int dq_expect_pauli_c128(const void* psi, uint64_t xmask, uint64_t zmask, int n, int64_t batch,
                         double* out, void* ws, dq_stream_t stream);

/* k <= 32 Z-type strings (xmask = 0) in ONE read of the state: `zmasks` is a HOST array; `nblocks` workgroups stride
 * over the state and each writes one row of partial sums: out = DEVICE double [batch, nblocks, k], fully overwritten;
 * the caller adds the nblocks rows.  A Hamiltonian of many ZZ terms (examples/qaoa.py:31-44: one observable per
 * edge, each a separate pass in qmath.expectation) costs one pass. */
int dq_expect_zmulti_c64(const void* psi, const uint64_t* zmasks, int k, int n, int64_t batch, double* out, int nblocks,
                         dq_stream_t stream);
int dq_expect_zmulti_c128(const void* psi, const uint64_t* zmasks, int k, int n, int64_t batch, double* out, int nblocks,
                          dq_stream_t stream);
/* out[b, i] = psi[b, i] * sum_j coef[b, j] (-1)^{popc(i & zmasks[j])}  (coef: DEVICE double [batch, k]): the
 * gradient of the above, i.e. (sum_j coef_j Z-string_j) |psi>, in one read + one write.  out may be psi. */
int dq_scale_zsigns_c64(const void* psi, void* out, const uint64_t* zmasks, int k, const double* coef, int n,
                        int64_t batch, dq_stream_t stream);
int dq_scale_zsigns_c128(const void* psi, void* out, const uint64_t* zmasks, int k, const double* coef, int n,
                         int64_t batch, dq_stream_t stream);

/* out[2b], out[2b+1] = Re, Im of <bra_b|ket_b> over `count` amplitudes.
 * Replaces inner_product_dist's local part (distributed.py:288-291) and `state.mH @ x`. */
int dq_inner_c64(const void* bra, const void* ket, int64_t count, int64_t batch, double* out, void* ws,
                 dq_stream_t stream);
int dq_inner_c128(const void* bra, const void* ket, int64_t count, int64_t batch, double* out, void* ws,
                  dq_stream_t stream);

/* probs[b, i] = |psi[b, i]|^2 in the state's real precision (qmath.py:624). */
int dq_probs_c64(const void* psi, void* probs, int64_t count, dq_stream_t stream);
int dq_probs_c128(const void* psi, void* probs, int64_t count, dq_stream_t stream);

/* Marginal distribution over `nw` bit positions (host array, bits[0] = MSB of the outcome index):
 * out[b, o] = sum over the other bits of |psi|^2, double precision, out must be zeroed by the
 * caller.  1 <= nw <= n <= 40, batch <= 65535, psi 16-byte aligned.  A workgroup owns 2^12 amplitudes (the low index
 * bits plus the lowest unmeasured ones) with a histogram in LDS over the measured bits among them: reads are coalesced
 * whatever the measured bits are.  Replaces the permute/reshape/sum of qmath.py:626. */
int dq_marginal_c64(const void* psi, int n, const int* bits, int nw, int64_t batch, double* out,
                    dq_stream_t stream);
int dq_marginal_c128(const void* psi, int n, const int* bits, int nw, int64_t batch, double* out,
                     dq_stream_t stream);

/* Gradient of a gate matrix: gU[b, i, j] += sum_groups gy[i] * conj(x[j]) over the amplitude groups
 * whose controls are all 1 (the matmul backward of qmath.py:504 / operation.py:216).  k <= 2.
 * gU is DEVICE double-precision complex [batch, 2^k, 2^k], zeroed by the caller. */
int dq_gate_grad_c64(const void* x, const void* gy, int n, const int* targets, int k, const int* controls,
                     int nc, int64_t batch, double* gU, dq_stream_t stream);
int dq_gate_grad_c128(const void* x, const void* gy, int n, const int* targets, int k, const int* controls,
                      int nc, int64_t batch, double* gU, dq_stream_t stream);

/* The same quantity for SEVERAL single-target gates on one pair of states, in one read of both (the reverse sweep of
 * the adjoint autograd node asks for all trainable gates of a circuit layer at once): gate g has target
 * targets[g] and controls ctrl_bits[ctrl_begin[g] .. ctrl_begin[g+1]).  Per call at most 8 gates (c64) / 4 (c128)
 * whose targets above bit 3 (c64) / 2 (c128) number at most 7, and n >= 11 (c64) / 10 (c128): DQ_ERR_UNSUPPORTED
 * otherwise (callers fall back to dq_gate_grad_*).  `nblocks` workgroups stride over the 2^(n-11) (c64) / 2^(n-10)
 * (c128) tiles; each writes ONE row of partial sums: out = DEVICE double complex [batch, nblocks, ngates, 2, 2], fully
 * overwritten; the caller adds the nblocks rows. */
int dq_gate_grad_multi_c64(const void* x, const void* gy, int n, int ngates, const int* targets, const int* ctrl_begin,
                           const int* ctrl_bits, int64_t batch, double* out, int nblocks, dq_stream_t stream);
int dq_gate_grad_multi_c128(const void* x, const void* gy, int n, int ngates, const int* targets, const int* ctrl_begin,
                            const int* ctrl_bits, int64_t batch, double* out, int nblocks, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 4. Shard exchange helpers for the index-bit-partitioned state (distributed.py:57-202).
 *    `nl` = number of local qubits (shard = 2^nl amplitudes per batch sample).
 * ------------------------------------------------------------------------------------------ */
/* packed[b, c] = amps[b, expand(c)] where expand() inserts, at the bit positions set in `mask`,
 * the corresponding bits of `value` (mask/value over local bit positions).  Replaces the
 * arange/boolean-mask gather of distributed.py:109-117, 150-155. */
int dq_pack_c64(const void* amps, void* packed, int nl, uint64_t mask, uint64_t value, int64_t batch,
                dq_stream_t stream);
int dq_pack_c128(const void* amps, void* packed, int nl, uint64_t mask, uint64_t value, int64_t batch,
                 dq_stream_t stream);
/* amps[b, expand(c)] = a * x[b, c] + bcoef * y[b, c]; coef = DEVICE pointer to 2 complex numbers
 * {a, bcoef} per batch sample (coef_batch_stride in complex numbers, 0 = shared) in the state's
 * precision.  With y == NULL: amps[b, expand(c)] = x[b, c] (pure scatter, SWAP local<->global).
 * Replaces distributed.py:70, 126, 157. */
int dq_unpack_axpby_c64(void* amps, const void* x, const void* y, const void* coef, int64_t coef_batch_stride,
                        int nl, uint64_t mask, uint64_t value, int64_t batch, dq_stream_t stream);
int dq_unpack_axpby_c128(void* amps, const void* x, const void* y, const void* coef, int64_t coef_batch_stride,
                         int nl, uint64_t mask, uint64_t value, int64_t batch, dq_stream_t stream);

/* out[b, i] = in[b, sigma(i)] with sigma(i) = sum_p bit_p(i) << src_of_dst[p] (host array of nl entries, a
 * permutation of 0..nl-1): re-labels the local qubits of a shard in one read + one write.  in != out.
 * Used by the all-to-all qubit remap (swap k global qubits with k local ones in ONE exchange step over all
 * xGMI links instead of the reference's one pairwise exchange per gate, distributed.py:57-202) and to restore
 * the canonical order (the reshape/transpose copy of local_swap_gate, distributed.py:48-54). */
int dq_permute_bits_c64(const void* in, void* out, int nl, const int* src_of_dst, int64_t batch,
                        dq_stream_t stream);
int dq_permute_bits_c128(const void* in, void* out, int nl, const int* src_of_dst, int64_t batch,
                         dq_stream_t stream);

/* ABI 24.  Two arrays of `count` amplitudes side by side along a NEW index bit 0: out[2 i] = a[i], out[2 i + 1] = b[i] --
 * how a fused reverse sweep (dq_apply_fused_grad_*) wants psi and the cotangent lambda, i.e. the final state of
 * circuit.py:261 and the gradient autograd hands back for it -- and the way back: out[i] = in[2 i + which].  `count`
 * even (all samples of a batch at once: count = batch * 2^n); out of place; full coalesced lines both ways.  All
 * buffers 16-byte aligned (a complex64 view at an odd element offset is not: DQ_ERR_ARG). */
int dq_interleave_c64(const void* a, const void* b, void* out, int64_t count, dq_stream_t stream);
int dq_interleave_c128(const void* a, const void* b, void* out, int64_t count, dq_stream_t stream);
int dq_deinterleave_c64(const void* in, void* out, int64_t count, int which, dq_stream_t stream);
int dq_deinterleave_c128(const void* in, void* out, int64_t count, int which, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 5. One-body reductions for entanglement measures (ABI 26; csrc/dq_entangle.hip).  Replace the permute-copies and
 *    inner products of qmath.meyer_wallach_measure / linear_map_mw / generalized_distance (qmath.py:874-938) and the
 *    4^n density matrix of meyer_wallach_measure_brennen (qmath.py:941-965).  Wire k is index bit n - 1 - k.
 *    1 <= n <= 40, 1 <= batch <= 65535.
 * ------------------------------------------------------------------------------------------ */
/* Bytes of device workspace dq_rdm1_cross_* needs (cross != 0: bra != ket); -1 on a bad argument. */
int64_t dq_rdm1_ws_bytes(int n, int64_t batch, int is_c128, int cross);
/* out[b, k, a, c] = sum over the other wires of conj(bra[b, a on wire k, rest]) * ket[b, c on wire k, rest]:
 * DEVICE complex128 [batch, n, 2, 2], fully overwritten.  bra == ket reads the state once per pass.  Passes: 1 +
 * ceil((n - 12) / 8) (complex64), 1 + ceil((n - 12) / 9) (complex128; its cross reduction 1 + ceil((n - 11) / 8)).
 * Workgroups write fixed-order partial sums into `ws` (at least dq_rdm1_ws_bytes bytes) and a second kernel adds
 * them: no atomics, results are bitwise reproducible. */
int dq_rdm1_cross_c64(const void* bra, const void* ket, int n, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                      dq_stream_t stream);
int dq_rdm1_cross_c128(const void* bra, const void* ket, int n, int64_t batch, double* out, void* ws, int64_t ws_bytes,
                       dq_stream_t stream);
/* out[b] = sum_k (mats[b, k] acting on wire k) psi[b]; mats: DEVICE complex128 [batch, n, 2, 2].  The reverse mode of
 * dq_rdm1_cross_*.  Same passes as dq_rdm1_cross_* with bra == ket: the first writes out, later ones read psi and add
 * into out.  out must not alias psi. */
int dq_apply_wire_sum_c64(const void* psi, void* out, const double* mats, int n, int64_t batch, dq_stream_t stream);
int dq_apply_wire_sum_c128(const void* psi, void* out, const double* mats, int n, int64_t batch, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 6. k-wire cross reduction on the matrix cores (ABI 27; csrc/dq_rdm.hip).  The reduced density matrix of k wires
 *    (x == gy) and the matrix cotangent of a dense gate on 3..10 wires, without copying the state:
 *        out[b, a, c] = sum_r gy[b, dep_T(a) | dep_R(r) | cmask] * conj(x[b, dep_T(c) | dep_R(r) | cmask])
 *    T = the k target bits (matrix MSB = targets[0]), controls fixed at 1, R = the other n - k - nc bits.
 *    3 <= k <= 10 (any other k: DQ_ERR_UNSUPPORTED), any n >= k + nc up to 40, 1 <= batch <= 65535.
 * ------------------------------------------------------------------------------------------ */
/* Bytes of device workspace dq_rdmk_cross_* needs (hermitian != 0: x == gy); -1 on a bad argument.  At most twice the
 * output plus 1 % of the state. */
int64_t dq_rdmk_ws_bytes(int n, int k, int nc, int64_t batch, int is_c128, int hermitian);
/* out: DEVICE complex128 [batch, 2^k, 2^k], fully overwritten (the caller does not zero it).  x == gy computes the
 * tiles on or above the diagonal and writes the rest as their exact conjugate: the result is exactly Hermitian.
 * Workgroups write fixed-order partial sums into `ws` (at least dq_rdmk_ws_bytes bytes) and a second kernel adds them:
 * no atomics, results are bitwise reproducible. */
int dq_rdmk_cross_c64(const void* x, const void* gy, int n, const int* targets, int k, const int* controls, int nc,
                      int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
int dq_rdmk_cross_c128(const void* x, const void* gy, int n, const int* targets, int k, const int* controls, int nc,
                       int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 7. Shot sampling by inverse CDF (ABI 28; csrc/dq_sample.hip).  Replaces the |psi|^2 temporary and the
 *    torch.multinomial calls of qmath.measure / block_sample (qmath.py:543-638) where raw outcomes are wanted.
 *        p_j = |psi[b, j]|^2,  C(i) = sum_{j <= i} p_j,  T = C(2^n - 1)   (double for both precisions)
 *        out[b, s] = the smallest i with C(i) > u[b, s] * T
 *    The state need not be normalised.  An index with p_i == 0 is never returned and a result is always in [0, 2^n),
 *    whatever the rounding.  1 <= n <= 40, 1 <= batch <= 65535, 1 <= shots; psi 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
/* Bytes of device workspace dq_sample_* needs (a 64-ary tree of partial sums: 2^n / 63 doubles per sample, nothing for
 * n <= 6; at most 2 % of the state); -1 on a bad argument. */
int64_t dq_sample_ws_bytes(int n, int64_t batch, int is_c128);
/* u: DEVICE double [batch, shots] in [0, 1); out: DEVICE int64 [batch, shots], flat amplitude indices (wire 0 = the
 * most significant bit), fully overwritten.  `ws` (at least dq_sample_ws_bytes bytes; may be NULL when that is 0) is
 * rebuilt from one read of the state on every call.  No atomics, no host synchronisation: bitwise reproducible. */
int dq_sample_c64(const void* psi, int n, int64_t batch, const double* u, int64_t shots, int64_t* out, void* ws,
                  int64_t ws_bytes, dq_stream_t stream);
int dq_sample_c128(const void* psi, int n, int64_t batch, const double* u, int64_t shots, int64_t* out, void* ws,
                   int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 8. Diagonal operators on any number of wires (ABI 30; csrc/dq_diag.hip): one multiplication per amplitude, one read
 *    and one write of the state whatever k is -- what UAnyGate / HamiltonianGate need a dense 4^k matrix and k <= 10
 *    for (gate.py:2745-3024), and what a QAOA cost layer spells as one Rzz per edge (examples/qaoa.py:31-44).
 *        sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j)
 *    `bits`: HOST array of k distinct index-bit positions, bits[0] = the table index's most significant bit (as in
 *    dq_marginal_*); `controls` / `nc` as in dq_apply_gate_*: an amplitude whose control bits are not all 1 passes
 *    through unchanged (diag, PHASE) or is left out of the sum (cross).  1 <= k, k + nc <= n <= 40, 1 <= batch <= 65535; state
 *    and table pointers 16-byte aligned.  bits = n-1 .. 0 without controls streams the table beside the state (no
 *    gather).
 * ------------------------------------------------------------------------------------------ */
/* out[b, i] = diag[b * diag_batch_stride + sub(i)] * in[b, i]; diag: DEVICE complex in the state's precision, 2^k entries
 * per table; diag_batch_stride = 0 (one table for the batch) or 2^k.  in == out is allowed (a lane owns the vectors it
 * reads and writes); any other overlap of [in, in + batch * 2^n) and [out, ..) is refused (DQ_ERR_ARG, "overlap"). */
int dq_apply_diag_c64(const void* in, void* out, const void* diag, int64_t diag_batch_stride, int n, const int* bits, int k,
                      const int* controls, int nc, int64_t batch, dq_stream_t stream);
int dq_apply_diag_c128(const void* in, void* out, const void* diag, int64_t diag_batch_stride, int n, const int* bits, int k,
                       const int* controls, int nc, int64_t batch, dq_stream_t stream);

#define DQ_COST_PHASE 0
#define DQ_COST_SCALE 1
/* cost: DEVICE real table in the state's real precision, 2^k entries, shared by the batch.
 *   op = DQ_COST_PHASE: out[b, i] = exp(-i t[b] cost[sub(i)]) * in[b, i], t = DEVICE double [batch].  The angle is
 *        double(t) * double(cost), reduced to a fraction of a turn in double for BOTH precisions; sine and cosine of that
 *        fraction in the state's real precision (an angle of 1e4 rad formed in float is off by more than 1e-4).
 *   op = DQ_COST_SCALE: out[b, i] = s[b] * cost[sub(i)] * in[b, i], s = DEVICE double [batch][2] (re, im): the
 *        cotangent of dq_cost_cross_*, which leaves the amplitudes outside the controls out of its sum -- so here, and
 *        only here, they come out as 0 instead of passing through.
 * in == out is allowed (a lane owns the vectors it reads and writes); any other overlap is refused (DQ_ERR_ARG,
 * "overlap"). */
int dq_apply_cost_c64(const void* in, void* out, const void* cost, const double* t, int op, int n, const int* bits, int k,
                      const int* controls, int nc, int64_t batch, dq_stream_t stream);
int dq_apply_cost_c128(const void* in, void* out, const void* cost, const double* t, int op, int n, const int* bits, int k,
                       const int* controls, int nc, int64_t batch, dq_stream_t stream);

/* Bytes of device workspace dq_cost_cross_* needs (one partial sum per workgroup and sample: at most 32 KiB per
 * sample; `cross` != 0: bra != ket, the same amount); -1 on a bad argument. */
int64_t dq_cost_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross);
/* out[b] = sum over i with controls = 1 of cost[sub(i)] * conj(bra[b, i]) * ket[b, i]: DEVICE double [batch][2] (re, im),
 * fully overwritten, accumulated in double.  bra == ket reads the state once: <C>, imaginary part exactly 0.
 * Workgroups write fixed-order partial sums into `ws` (at least dq_cost_cross_ws_bytes bytes, 16-byte aligned) and a
 * second kernel adds them: no atomics, results are bitwise reproducible. */
int dq_cost_cross_c64(const void* bra, const void* ket, const void* cost, int n, const int* bits, int k, const int* controls,
                      int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
int dq_cost_cross_c128(const void* bra, const void* ket, const void* cost, int n, const int* bits, int k, const int* controls,
                       int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 9. Pauli strings on any number of wires (csrc/dq_pauli.hip; added within ABI 30, presence is checked by symbol): the
 *    non-diagonal half of section 8 -- exp(-i theta/2 P) = cos(theta/2) - i sin(theta/2) P, what HamiltonianGate needs
 *    a dense 4^span matrix and a span <= 10 for (gate.py:2867-3024) -- in one read and one write of the state whatever
 *    the weight of P.
 *        (P psi)[i] = i^ny * (-1)^popc((i ^ xmask) & zmask) * psi[i ^ xmask],   ny = popc(xmask & zmask)
 *    `xmask` / `zmask` over index bits as in dq_expect_pauli_* (a Y sets its bit in both); `controls` / `nc` as in
 *    dq_apply_gate_*, disjoint from xmask | zmask.  1 <= n <= 40, 1 <= batch <= 65535; state pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define DQ_PAULI_GATE 0
#define DQ_PAULI_MAP 1
/* out[b, i] = a[b] * in[b, i] + c[b] * (P in_b)[i] on the amplitudes whose control bits are all 1; coef = DEVICE double
 * [batch][4] = (Re a, Im a, Re c, Im c), rounded once to the state's real precision.
 *   mode = DQ_PAULI_GATE: the amplitudes outside the controls pass through bitwise.
 *   mode = DQ_PAULI_MAP:  they come out as 0 (the cotangent of dq_pauli_cross_*, which leaves them out).
 * in == out is allowed (one unit of work owns both ends of a pair i, i ^ xmask); any other overlap is refused
 * (DQ_ERR_ARG, "overlap"). */
int dq_apply_pauli_axpby_c64(const void* in, void* out, uint64_t xmask, uint64_t zmask, const double* coef, int mode, int n,
                             const int* controls, int nc, int64_t batch, dq_stream_t stream);
int dq_apply_pauli_axpby_c128(const void* in, void* out, uint64_t xmask, uint64_t zmask, const double* coef, int mode, int n,
                              const int* controls, int nc, int64_t batch, dq_stream_t stream);

/* Bytes of device workspace dq_pauli_cross_* needs (one partial sum per workgroup and sample: at most 32 KiB per
 * sample, whatever the masks; `cross` != 0: bra != ket, the same amount); -1 on a bad argument. */
int64_t dq_pauli_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross);
/* out[b] = sum over i with controls = 1 of conj(bra[b, i]) * (P ket_b)[i]: DEVICE double [batch][2] (re, im), fully
 * overwritten, accumulated in double.  bra == ket reads the state once; xmask = zmask = 0 is the inner product over the
 * controlled amplitudes.  Workgroups write fixed-order partial sums into `ws` (at least dq_pauli_cross_ws_bytes bytes,
 * 16-byte aligned) and a second kernel adds them: no atomics, results are bitwise reproducible. */
int dq_pauli_cross_c64(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls, int nc,
                       int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
int dq_pauli_cross_c128(const void* bra, const void* ket, uint64_t xmask, uint64_t zmask, int n, const int* controls, int nc,
                        int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 10. Basis-state permutations on any number of wires (csrc/dq_perm.hip; added within ABI 30, presence is checked by
 *     symbol): the classical reversible maps |x> -> |perm(x)> -- bit oracles, modular arithmetic, shifts -- in one read and
 *     one write of the state, with no arithmetic: amplitudes are copied bit for bit.
 *         sub(i) as in section 8; put(i, v) = i with the k table bits replaced by the bits of v (sub(put(i, v)) = v)
 *         out[b, j] = in[b, put(j, src[sub(j)])]     where all control bits of j are 1, in[b, j] elsewhere
 *     `src`: DEVICE table of 2^k entries, the INVERSE of perm (gather form), shared by the batch, 4-byte aligned.  Every
 *     entry is masked with 2^k - 1 before use: a table that is no bijection gives a wrong state and never a load outside
 *     the sample.  `bits` / `controls` / `nc` as in section 8.  1 <= n <= 40, 1 <= k <= min(n, 31), 1 <= batch <= 65535;
 *     state pointers 16-byte aligned.  OUT OF PLACE ONLY: [in, in + batch * 2^n) and [out, ..) must not overlap.
 *     `path`: DQ_PERM_GATHER always applies; DQ_PERM_LOCAL (the permutation stays inside a 16-KiB chunk, which goes
 *     through LDS) needs every table bit below dq_permutation_local_bits; DQ_PERM_AUTO takes LOCAL where it applies.
 * ------------------------------------------------------------------------------------------ */
#define DQ_PERM_AUTO 0
#define DQ_PERM_GATHER 1
#define DQ_PERM_LOCAL 2
int dq_apply_permutation_c64(const void* in, void* out, const uint32_t* src, int n, const int* bits, int k, const int* controls,
                             int nc, int64_t batch, int path, dq_stream_t stream);
int dq_apply_permutation_c128(const void* in, void* out, const uint32_t* src, int n, const int* bits, int k, const int* controls,
                              int nc, int64_t batch, int path, dq_stream_t stream);
/* log2 of the amplitudes of a LOCAL chunk: 11 (complex64) / 10 (complex128). */
int dq_permutation_local_bits(int is_c128);

/* ------------------------------------------------------------------------------------------
 * 11. Multiplexed (uniformly controlled) one-qubit gates on any number of select wires (csrc/dq_mux.hip; added within
 *     ABI 30, presence is checked by symbol): for every value of k select bits its own 2x2 matrix on one target bit --
 *     the non-diagonal sibling of section 8 -- in one read and one write of the state whatever k is.
 *         sub(i) as in section 8, over the select bits `bits`
 *         (out[b, i0], out[b, i1]) = M[sub(i0)] (in[b, i0], in[b, i1])      i0: target bit 0, i1 = i0 | 1 << target
 *     where all control bits are 1; the other amplitudes pass through bitwise.  `table`: DEVICE, 2^k entries in the
 *     state's precision, 16-byte aligned, shared by the batch:
 *         kind = DQ_MUX_U:  an entry is u00 u01 u10 u11, complex (32 / 64 bytes)
 *         kind = DQ_MUX_RY: an entry is (c, s), real, M = [[c, -s], [s, c]] (8 / 16 bytes)
 *     dagger = 1 applies the conjugate transpose of every entry from the same table.  The kernel does no trigonometry,
 *     and no address depends on the table's contents.  `bits`, `controls` and `target` are pairwise distinct positions;
 *     2 <= n <= 40, 1 <= k <= n - 1, 1 <= batch <= 65535; state pointers 16-byte aligned.  in == out is allowed (one unit
 *     of work owns both ends of a pair); any other overlap is refused.
 * ------------------------------------------------------------------------------------------ */
#define DQ_MUX_U 0
#define DQ_MUX_RY 1
int dq_apply_mux_c64(const void* in, void* out, const void* table, int kind, int dagger, int n, int target, const int* bits,
                     int k, const int* controls, int nc, int64_t batch, dq_stream_t stream);
int dq_apply_mux_c128(const void* in, void* out, const void* table, int kind, int dagger, int n, int target, const int* bits,
                      int k, const int* controls, int nc, int64_t batch, dq_stream_t stream);

/* The binned cross reduction (csrc/dq_muxgrad.hip; added within ABI 30, presence is checked by symbol): what the gradient
 * with respect to the 2^k angles of a multiplexed rotation is made of.  G = the one-qubit Pauli `axis` on bit `target`:
 *     out[b, s] = sum over i with sub(i) = s and controls = 1 of conj(bra[b, i]) * (G ket_b)[i]
 * DEVICE double [batch][2^k][2] (re, im), fully overwritten, accumulated in double.  bra == ket reads the state once.
 * `bits`, `controls`, `target`, n, k and batch as for dq_apply_mux_*.  Workgroups write fixed-order partial sums per bin
 * into `ws` (at least dq_mux_cross_ws_bytes bytes, 16-byte aligned) and a second kernel adds them: no atomics, results
 * are bitwise reproducible bin by bin.  No address depends on data. */
#define DQ_MUX_AXIS_I 0
#define DQ_MUX_AXIS_X 1
#define DQ_MUX_AXIS_Y 2
#define DQ_MUX_AXIS_Z 3
/* Bytes of device workspace dq_mux_cross_* needs for k select bits, wherever they lie (at most 8 MiB per sample, 16
 * bytes where one workgroup owns every bin; `is_c128` and `cross` change nothing); -1 on a bad argument. */
int64_t dq_mux_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross, int k);
int dq_mux_cross_c64(const void* bra, const void* ket, int axis, int n, int target, const int* bits, int k, const int* controls,
                     int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
int dq_mux_cross_c128(const void* bra, const void* ket, int axis, int n, int target, const int* bits, int k, const int* controls,
                      int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 12. Excitation gates -- Givens rotations between two bit patterns -- that touch only their subspace
 *     (csrc/dq_excite.hip; added within ABI 30, presence is checked by symbol).  K = E - E^dagger for an excitation E
 *     between the patterns `amask` and `xmask ^ amask` of the bits of `xmask`; exp(theta K) = I + sin(theta) K +
 *     (1 - cos(theta)) K^2 is a = cos(theta), c = sin(theta) below.  For every i0 with i0 & xmask == amask and every
 *     control bit 1, i1 = i0 ^ xmask and sigma = (-1)^(negate + popc(i0 & zmask)):
 *         (K psi)[i1] = sigma * psi[i0]        (K psi)[i0] = -sigma * psi[i1]        (K psi)[i] = 0 elsewhere
 *     xmask != 0 of any weight; amask a subset of xmask; zmask (the Jordan-Wigner string over the free bits) and the
 *     controls disjoint from xmask and from each other -- a caller folds the zmask bits that fall on fixed bits into
 *     `negate` (0 or 1).  1 <= n <= 40, 1 <= batch <= 65535; state pointers 16-byte aligned.  The pairs are
 *     2 / 2^(popc(xmask) + nc) of the state, and the kernels read and write only the 16-byte vectors that hold an end
 *     of a pair.
 * ------------------------------------------------------------------------------------------ */
#define DQ_EXCITE_GATE 0
#define DQ_EXCITE_MAP 1
/* out[b, i] = a[b] * in[b, i] + c[b] * (K in_b)[i] for i = i0, i1 of every pair; coef = DEVICE double [batch][4] =
 * (Re a, Im a, Re c, Im c), rounded once to the state's real precision.  NOTHING ELSE OF `out` IS WRITTEN: with
 * in == out that is the gate in place; with a disjoint `out` the caller fills the rest first (a copy of `in` for the gate,
 * zeros for the cotangent map).  An amplitude that shares a 16-byte vector with an end of a pair without being one
 * (complex64, bit 0 fixed) is copied bitwise from `in` (mode = DQ_EXCITE_GATE) or written as 0 (DQ_EXCITE_MAP).  Any
 * overlap of in and out other than in == out is refused (DQ_ERR_ARG, "overlap"). */
int dq_apply_excite_axpby_c64(const void* in, void* out, const double* coef, int mode, uint64_t xmask, uint64_t amask,
                              uint64_t zmask, int negate, int n, const int* controls, int nc, int64_t batch, dq_stream_t stream);
int dq_apply_excite_axpby_c128(const void* in, void* out, const double* coef, int mode, uint64_t xmask, uint64_t amask,
                               uint64_t zmask, int negate, int n, const int* controls, int nc, int64_t batch, dq_stream_t stream);

/* Bytes of device workspace dq_excite_cross_* needs (one partial sum per workgroup and sample: at most 32 KiB per
 * sample, whatever the masks; `cross` != 0: bra != ket, the same amount); -1 on a bad argument. */
int64_t dq_excite_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross);
/* out[b] = sum_i conj(bra[b, i]) * (K ket_b)[i]: DEVICE double [batch][2] (re, im), fully overwritten, accumulated in
 * double, reading only the pairs.  bra == ket reads each pair once (the real part is then 0 up to rounding: K is
 * anti-Hermitian).  Workgroups write fixed-order partial sums into `ws` (at least dq_excite_cross_ws_bytes bytes,
 * 16-byte aligned) and a second kernel adds them: no atomics, results are bitwise reproducible. */
int dq_excite_cross_c64(const void* bra, const void* ket, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate, int n,
                        const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
int dq_excite_cross_c128(const void* bra, const void* ket, uint64_t xmask, uint64_t amask, uint64_t zmask, int negate, int n,
                         const int* controls, int nc, int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 13. Sums of Pauli strings (csrc/dq_psum.hip; added within ABI 30, presence is checked by symbol): H = sum_t h_t P_t
 *     with real h_t and P_t = (x_t, z_t) as in section 9, the whole sum in ONE launch.  The terms are grouped by flip
 *     mask; for the group with mask x
 *         (G_x psi)[i] = w_x(i ^ x) psi[i ^ x],      w_x(j) = sum_{t in group} h_t i^{ny_t} (-1)^popc(j & z_t)
 *     and H = sum_x G_x.  The table is four DEVICE arrays, shared by the batch, for `ngroups` groups and `nterms` terms:
 *         xmasks[ngroups]        uint64, the flip mask of each group
 *         bounds[2 ngroups + 1]  int32: group g's terms with a real i^{ny_t} are [bounds[2g], bounds[2g+1]), those with
 *                                an imaginary one [bounds[2g+1], bounds[2g+2])
 *         zmasks[nterms]         uint64
 *         weights[nterms]        double: h_t with the sign of i^{ny_t} (real terms) or of i^{ny_t} / i (imaginary terms)
 *     The kernels mask every xmask with 2^n - 1 and clamp every bound to [0, nterms]: a wrong table gives a wrong state
 *     and never a load outside the sample or the table.  1 <= n <= 40, 1 <= batch <= 65535, ngroups >= 1, nterms >= 1;
 *     state pointers 16-byte aligned, xmasks / zmasks / weights 8-byte and bounds 4-byte aligned.  The state is read
 *     ngroups + 1 times (once less where a group has no flip over 16-byte vectors) whatever nterms is.
 * ------------------------------------------------------------------------------------------ */
/* out[b, i] = a[b] * in[b, i] + c[b] * (H in_b)[i]; coef = DEVICE double [batch][4] = (Re a, Im a, Re c, Im c), rounded
 * once to the state's real precision.  OUT OF PLACE ONLY: [in, in + batch * 2^n) and [out, ..) must not overlap
 * (DQ_ERR_ARG, "overlap"). */
int dq_apply_psum_axpby_c64(const void* in, void* out, const double* coef, const uint64_t* xmasks, const int* bounds,
                            const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n, int64_t batch,
                            dq_stream_t stream);
int dq_apply_psum_axpby_c128(const void* in, void* out, const double* coef, const uint64_t* xmasks, const int* bounds,
                             const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n, int64_t batch,
                             dq_stream_t stream);

/* Bytes of device workspace dq_psum_cross_* needs (one partial sum per workgroup and sample: at most 32 KiB per sample,
 * whatever the table; `cross` != 0: bra != ket, the same amount); -1 on a bad argument. */
int64_t dq_psum_cross_ws_bytes(int n, int64_t batch, int is_c128, int cross);
/* out[b] = sum_i conj(bra[b, i]) * (H ket_b)[i]: DEVICE double [batch][2] (re, im), fully overwritten.  The sums over a
 * group's terms are formed in the state's precision, everything after them in double.  bra == ket loads the own vector
 * once and reuses it for the group without a flip.  Workgroups write fixed-order partial sums into `ws` (at least
 * dq_psum_cross_ws_bytes bytes, 16-byte aligned) and a second kernel adds them: no atomics, results are bitwise
 * reproducible. */
int dq_psum_cross_c64(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks,
                      const double* weights, int ngroups, int nterms, int n, int64_t batch, double* out, void* ws,
                      int64_t ws_bytes, dq_stream_t stream);
int dq_psum_cross_c128(const void* bra, const void* ket, const uint64_t* xmasks, const int* bounds, const uint64_t* zmasks,
                       const double* weights, int ngroups, int nterms, int n, int64_t batch, double* out, void* ws,
                       int64_t ws_bytes, dq_stream_t stream);

/* One order of a Chebyshev recurrence in H and its running sum, in one launch:
 *     next[b, i] = alpha[b] * (H cur_b)[i] + beta[b] * cur[b, i] + gamma[b] * prev[b, i]
 *     acc[b, i] += delta[b] * next[b, i]
 * coef = DEVICE double [batch][5] = (alpha, beta, gamma, Re delta, Im delta): alpha, beta, gamma real, delta complex,
 * rounded once to the state's real precision; 8-byte aligned.  `cur` is only read (ngroups + 1 times, as above); prev,
 * next and acc are read and written at each lane's own vectors, once each.  Which buffers may share memory, each being
 * [p, p + batch * 2^n):
 *     next == prev is allowed (phi_{k+1} written over phi_{k-1}); a shifted overlap of the two is not;
 *     cur must be disjoint from next and from acc;  acc must be disjoint from cur, prev and next.
 * Everything else is DQ_ERR_ARG, "<a> and <b> overlap".  prev is not written unless it is next. */
int dq_pauli_sum_cheb_step_c64(const void* cur, const void* prev, void* next, void* acc, const double* coef, const uint64_t* xmasks,
                          const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
                          int64_t batch, dq_stream_t stream);
int dq_pauli_sum_cheb_step_c128(const void* cur, const void* prev, void* next, void* acc, const double* coef, const uint64_t* xmasks,
                           const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
                           int64_t batch, dq_stream_t stream);

/* The two launches of a three-term Lanczos step in H (added within ABI 30, presence is checked by symbol).  Both leave two
 * real sums per sample in out = DEVICE double [batch][2], fully overwritten: products and sums in double over the values
 * AS STORED (after rounding to the state's precision), workgroups' partial sums in a fixed order through `ws` (at least
 * dq_psum_cross_ws_bytes(n, batch, is_c128, 0) bytes, 16-byte aligned) and a second kernel: no atomics, bitwise
 * reproducible.  out 8-byte aligned.
 *
 * dq_pauli_sum_lanczos_step_*:
 *     next[b, i] = alpha[b] * (H cur_b)[i] + beta[b] * cur[b, i] + gamma[b] * prev[b, i]
 *     out[b]     = ( sum_i Re conj(cur[b, i]) next[b, i] ,  sum_i |next[b, i]|^2 )
 * coef = DEVICE double [batch][3] = (alpha, beta, gamma), real, rounded once to the state's real precision; 8-byte
 * aligned.  `cur` is only read (ngroups + 1 times, as above); prev is read and next written at each lane's own vectors.
 * next == prev is allowed, a shifted overlap of the two is not; cur must be disjoint from next: everything else is
 * DQ_ERR_ARG, "<a> and <b> overlap".  prev is never null (the first step passes zeros) and not written unless it is next. */
int dq_pauli_sum_lanczos_step_c64(const void* cur, const void* prev, void* next, const double* coef, const uint64_t* xmasks,
                                  const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
                                  int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
int dq_pauli_sum_lanczos_step_c128(const void* cur, const void* prev, void* next, const double* coef, const uint64_t* xmasks,
                                   const int* bounds, const uint64_t* zmasks, const double* weights, int ngroups, int nterms, int n,
                                   int64_t batch, double* out, void* ws, int64_t ws_bytes, dq_stream_t stream);
/* dq_lanczos_update_*: a stream over the lane's own vectors, no table:
 *     w[b, i]   += e[b] * v[b, i]                      (in place)
 *     acc[b, i] += d[b] * v[b, i]                      (only when acc is non-null)
 *     out[b]     = ( sum_i |w[b, i]|^2 ,  sum_i Re conj(v[b, i]) w[b, i] )       over the updated w
 * coef = DEVICE double [batch][2] = (e, d), real, rounded once to the state's real precision; 8-byte aligned.  v is only
 * read.  v, w and acc (where given) are 16-byte aligned and pairwise disjoint (DQ_ERR_ARG, "<a> and <b> overlap").
 * 1 <= n <= 40, 1 <= batch <= 65535. */
int dq_lanczos_update_c64(const void* v, void* w, void* acc, const double* coef, int n, int64_t batch, double* out, void* ws,
                          int64_t ws_bytes, dq_stream_t stream);
int dq_lanczos_update_c128(const void* v, void* w, void* acc, const double* coef, int n, int64_t batch, double* out, void* ws,
                           int64_t ws_bytes, dq_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 14. SELECT over Pauli strings (csrc/dq_select.hip; added within ABI 30, presence is checked by symbol): the operator
 *     sum_s |s><s| (x) c_s P_s of a linear combination of unitaries -- for every value s of k select bits its own Pauli
 *     string P_s = (x_s, z_s) as in section 9 with a phase c_s = i^q_s on the other wires -- in one read and one write of
 *     the state whatever the number of strings.
 *         sub(i) as in section 8; free = (2^n - 1) & ~(select bits | control bits)
 *         s = sub(i),  (x, z, q) = table[s],  x &= free,  j = i ^ x
 *         out[b, i] = i^q * (-1)^popc(j & z) * in[b, j]     where all control bits of i are 1, in[b, i] elsewhere
 *     `table`: DEVICE table of 2^k entries of two uint64, shared by the batch, 16-byte aligned:
 *         word0 = x | q << 62          (the flip mask over index bits; q in 0..3, the i^ny of the Y factors folded in)
 *         word1 = z                    (the sign mask over index bits)
 *     x is masked with `free` in the kernel: a wrong table gives a wrong state and never a load outside the sample, and an
 *     amplitude and its source always share s and the controls.  The factor is applied by swapping re and im and flipping
 *     sign bits: the result is exact, and an entry with x = z = q = 0 copies bit for bit.  `bits` / `controls` / `nc` as in
 *     section 8.  1 <= n <= 40, 1 <= k <= min(n, 31), 1 <= batch <= 65535; state pointers 16-byte aligned.
 *     OUT OF PLACE ONLY: [in, in + batch * 2^n) and [out, ..) must not overlap.
 * ------------------------------------------------------------------------------------------ */
int dq_apply_select_pauli_c64(const void* in, void* out, const uint64_t* table, int n, const int* bits, int k,
                              const int* controls, int nc, int64_t batch, dq_stream_t stream);
int dq_apply_select_pauli_c128(const void* in, void* out, const uint64_t* table, int n, const int* bits, int k,
                               const int* controls, int nc, int64_t batch, dq_stream_t stream);
/* log2 of the amplitudes of a unit of 1024 16-byte vectors: 11 (complex64) / 10 (complex128).  Select bits at or above it
 * are uniform over a workgroup (the entry is read once per unit); below it every vector reads its own entry. */
int dq_select_pauli_unit_bits(int is_c128);

/* ------------------------------------------------------------------------------------------
 * 15. Every sample against every sample (csrc/dq_gram.hip; added within ABI 30, presence is checked by symbol): the Gram
 *     matrix of two batches of states and linear combinations of a batch, on the matrix cores with exact f32 / f64
 *     products.  Rows are contiguous, 2^n amplitudes each; 1 <= n <= 40 for complex64, 0 <= n <= 40 for complex128 (a
 *     row is at least one 16-byte vector); 1 <= rows <= 65535 * 32 on either side (a tile of 32 rows is a grid dimension),
 *     and a Gram of at most 2^32 entries.
 * ------------------------------------------------------------------------------------------ */
/* The geometry of dq_gram_*: rows of a tile; `chain`, the number of real terms an f32 accumulator sums before it is added
 * into a double (complex64; 0 for complex128, whose sums are f64 throughout); the columns (amplitudes) of a lane's segment,
 * of a wave's share of a step and of a workgroup's unit per iteration; the most workgroups a tile pair is spread over. */
int dq_gram_geometry(int is_c128, int* tile_rows, int* chain, int* lane_cols, int* wave_cols, int* unit_cols, int* max_blocks);
/* Bytes of device workspace dq_gram_* needs (32 x 32 partial sums per workgroup); -1 on a bad argument. */
int64_t dq_gram_ws_bytes(int n, int64_t rows_a, int64_t rows_b, int is_c128);
/* out[i, j] = sum_x conj(a[i, x]) * b[j, x]: DEVICE double [rows_a][rows_b][2] (re, im), fully overwritten, 8-byte
 * aligned; a, b and ws 16-byte aligned.  Up to 32 x 32 rows every row is read once; beyond that rows are tiled and a row
 * of a is read ceil(rows_b / 32) times, a row of b ceil(rows_a / 32) times.  a == b with rows_a == rows_b is the
 * self-Gram: tiles on and above the diagonal only, a diagonal tile's rows loaded once for both operands, the lower
 * triangle written as the exact conjugate of the upper one and the diagonal's imaginary part as 0.  complex64: products
 * and sums in f32 for at most `chain` real terms, everything after that in double; complex128: f64 throughout.
 * Workgroups write fixed-order partial sums into `ws` (at least dq_gram_ws_bytes bytes) and a second kernel adds them: no
 * atomics, results are bitwise reproducible, and an entry's bits depend on its two rows, n and the number of tile pairs
 * alone.  a and b are only read and may share memory in any way; out and ws must overlap neither them nor each other
 * (DQ_ERR_ARG, "out, ws and the states overlap"). */
int dq_gram_c64(const void* a, const void* b, int n, int64_t rows_a, int64_t rows_b, double* out, void* ws, int64_t ws_bytes,
                dq_stream_t stream);
int dq_gram_c128(const void* a, const void* b, int n, int64_t rows_a, int64_t rows_b, double* out, void* ws, int64_t ws_bytes,
                 dq_stream_t stream);
/* out[m, x] = sum_j coef[m, j] * in[j, x]: in (rows_in, 2^n), out (rows_out, 2^n) in the states' dtype, both 16-byte
 * aligned; coef = DEVICE complex128 [rows_out][rows_in] as (re, im) doubles, 16-byte aligned, rounded once to the states'
 * real precision; products and sums on the matrix cores in that precision, 2 * rows_in real terms per output element.
 * `in` is read ceil(rows_out / 32) times, `out` written once, whatever rows_in.
 * OUT OF PLACE ONLY: [in, in + rows_in * 2^n) and [out, out + rows_out * 2^n) must not overlap ("in and out overlap"),
 * nor may out and coef. */
int dq_combine_c64(const void* in, const double* coef, void* out, int n, int64_t rows_out, int64_t rows_in, dq_stream_t stream);
int dq_combine_c128(const void* in, const double* coef, void* out, int n, int64_t rows_out, int64_t rows_in, dq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DQ_HIP_H */
