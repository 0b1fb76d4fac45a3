"""The launch paths of the wave-tile pass kernel (csrc/dq_wave.hip: wave_launch and the prologue / epilogue of
wave_pass_kernel), one row per path and shape -- TEST INFRASTRUCTURE ONLY; runs on whatever device it is given.

What `wave_launch` decides from the size of a job (mirror: `_launch_geometry.wave_pass`):
  A  two tiles per wave in a launch with DQ_FG_GRAD records (tiles * batch >= 16384), one atomic per workgroup
  B  the same for a forward pass whose only reductions are DQ_FG_EXPZ records
  C  the same with the records in device memory (more than 112 of them)
  D  XCD-aware tile numbers at one tile per wave (grid.x % 8 == 0); D2: kept at two tiles per wave
  E  the regrouping of a launch whose samples share ONE input state (grid.x % 8 == 0)
  F  streaming loads and stores (a state of 1 GiB and more); Fs: stores only, for a shared input
  G  fewer tiles than waves (n = m, m + 1) in a reducing launch
  H  known-zero bits outside the tile move the thresholds of D (H8: grid.x = 8, mapping on; H4: grid.x = 4, off)

A row is a seeded gate list, scheduled by `fusion.schedule` into passes that all run at the row's shape; `step_info` says
of every pass what the mirror says of its launch, and a row's `paths` must each be reached by one of its passes.  Every
pass writes into an output pre-filled with NaN; the accumulator of the reductions starts at 0.5 and row 0 is named by no
record.

Two criteria:
  exact rows  amplitudes with real and imaginary parts in {-1, 0, 1}, X gates with controls of every kind, diagonal gates
              with entries in {1, -1, i, -i}, and the reductions: every product is a small integer, a workgroup's float32
              accumulator holds at most 8 tile lives x 4096 terms x 2 = 65536 < 2^24, the double atomics are exact.  State
              and sums satisfy `torch.equal` with the reference at any size.
  rounding rows  seeded random gates of every kind on Haar-like states.  Amplitudes: |got_i - ref_i| <= tau S_i with
              S = |U_G| .. |U_1| |x| and tau = the sum over the row's passes of `_handler_cases.tau_amplitudes` (the bound
              of one pass as it stands; an earlier pass's error is carried through the later gates inside the same
              bound).  Sums: |got - ref| <= (tau_r + 2 tau_c) S, `_handler_cases.tau_reduction` as it stands: tau_r the
              summation's own share ((M + 2) u, doubled for DQ_FG_GRAD; 1e-12 for complex128), tau_c the amplitude bound
              of all passes up to and including the record's, S the sum over the absolute values of the terms.

The reference (`reference`) applies the gates in complex128 on the device with `_grid_refs.apply_gate`, one by one in the
order the passes execute them (a valid order of the circuit: test_pass_paths_cpu.py holds it against the oracle applying
the caller's order), and takes the sums where the pass takes them.

Negative controls, from reference tensors only (`corruptions`):
  (i)   the tile that wave 0 of workgroup 0 walks second (one tile per wave: the tile of wave 1; a pass of one tile: that
        tile) -- its output left at what the last pass read (NaN, the output's fill, where the last pass changes nothing
        there), its terms dropped from every sum of sample 0;
  (ii)  shared input: the output tiles of samples 0 and 1 of tile 0 exchanged;
  (iii) streaming: amplitude 1 of sample 0 (complex64: the second amplitude of a 16-byte store; complex128 stores one
        amplitude in 16 bytes, there it is a store gone to the next but one place) exchanged with the second amplitude of
        the nearest later pair that holds another value.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import random
from dataclasses import dataclass, replace

import numpy as np
import torch

import _grid_refs as R
import _handler_cases as hc
import _launch_geometry as G
import _wave_emulator as emu
from deepquantum_amd import _lib, backend, fusion
from deepquantum_amd.fusion import PrimOp
from test_wave_cpu import random_ops

C128 = torch.complex128
UNITS = (1, -1, 1j, -1j)
X2 = torch.tensor([[0, 1], [1, 0]], dtype=C128)


def tile_bits(is128):
    return 11 if is128 else 12


@dataclass(frozen=True)
class Row:
    paths: tuple              # keys of PATHS: each is reached by one pass of the row
    n: int
    batch: int
    is128: bool
    kind: str                 # 'exact' | 'round'
    mode: str                 # 'fwd' | 'grad' (DQ_FG_GRAD records) | 'expz' (five Z strings) | 'ext' (a long sweep)
    seed: int = 0
    shared: bool = False      # ONE input state for the batch, per-sample matrices
    zero_bits: int = 0        # known-zero index bits outside the first pass's tile
    floor: tuple = ()         # paths of which the row is the smallest shape: one qubit less does not reach them

    @property
    def id(self):
        extra = ('-shared' if self.shared else '') + (f'-kz{self.zero_bits}' if self.zero_bits else '')
        return f'{"+".join(self.paths)}-{self.kind}-{self.mode}-n{self.n}-b{self.batch}-{"c128" if self.is128 else "c64"}{extra}'

    @property
    def reducing(self):
        return self.mode != 'fwd'


#: path -> what the mirror (and the pass's records) must say of a pass that reaches it
PATHS = {
    'A': lambda g: g['has_grad'] and not g['ext'] and g['tpw'] == 2 and g['second_stride'] == g['grid_x'] * 4,
    'A1': lambda g: g['has_grad'] and not g['ext'] and g['tpw'] == 1,            # (the twin just below the threshold)
    'B': lambda g: g['reducing'] and g['has_expz'] and g['only_expz'] and g['tpw'] == 2,
    'C': lambda g: g['ext'] and g['has_grad'] and g['tpw'] == 2,
    'D': lambda g: g['xcd'] == 31 and g['tpw'] == 1,
    'D2': lambda g: g['xcd'] == 31 and g['tpw'] == 2,
    'E': lambda g: g['regroup'] and g['xcd'] == 0,
    'F': lambda g: g['nt_loads'] and g['nt_stores'],
    'Fs': lambda g: g['regroup'] and g['nt_stores'] and not g['nt_loads'],
    'ADF': lambda g: PATHS['A'](g) and PATHS['D2'](g) and PATHS['F'](g),
    'G': lambda g: g['reducing'] and g['idle_waves'] > 0,
    'H8': lambda g: g['zero_bits'] > 0 and g['grid_x'] == 8 and g['xcd'] == 31,
    'H4': lambda g: g['zero_bits'] > 0 and g['grid_x'] == 4 and g['xcd'] == 0,
    'EH': lambda g: g['zero_bits'] > 0 and g['regroup'],
}


def _rows():
    out = []
    for is128 in (False, True):
        d = int(is128)          # (a complex128 tile is one bit smaller and an amplitude twice as large: every shape moves by one)

        def row(paths, n, batch, kind, mode, seed, **kw):
            out.append(Row(tuple(paths), n - d, batch, is128, kind, mode, seed, **kw))

        # A: a (psi, lambda) pair state of 512 MiB in four shapes; the last has ONE tile per sample (second_stride = 4)
        row(['A', 'D2'], 26, 1, 'exact', 'grad', 1, floor=('A',))
        row(['A', 'D2'], 22, 16, 'exact', 'grad', 2, floor=('A',))
        row(['A', 'D2'], 19, 128, 'exact', 'grad', 3, floor=('A',))
        row(['A'], 12, 16384, 'exact', 'grad', 4)
        row(['A1'], 25, 1, 'exact', 'grad', 1)
        row(['A', 'D2'], 26, 1, 'round', 'grad', 5)
        row(['A', 'D2'], 22, 16, 'round', 'grad', 6)
        # B: five Z strings out of a forward pass
        row(['B'], 26, 1, 'exact', 'expz', 7, floor=('B',))
        row(['B'], 22, 16, 'exact', 'expz', 8, floor=('B',))
        row(['B'], 26, 1, 'round', 'expz', 9)
        # C: a long sweep pass, records in device memory
        row(['C'], 26, 1, 'exact', 'ext', 10, floor=('C',))
        row(['C'], 26, 1, 'round', 'ext', 11)
        # D: XCD-aware tile numbers at one tile per wave, grid.x = 8, 16, 64
        for n, fl in ((17, ('D',)), (18, ()), (20, ())):
            for b in (1, 3):
                row(['D'], n, b, 'exact', 'fwd', 12 + n, floor=fl)
        row(['D'], 17, 3, 'round', 'fwd', 40)
        row(['D'], 20, 1, 'round', 'fwd', 41)
        # E: one shared input, per-sample matrices
        for b in (2, 3, 5, 16):
            row(['E'], 17, b, 'exact', 'fwd', 50 + b, shared=True, floor=('E',))
        row(['E'], 19, 3, 'exact', 'fwd', 60, shared=True)
        row(['E', 'EH'], 18, 3, 'exact', 'fwd', 61, shared=True, zero_bits=1)
        row(['E'], 17, 3, 'round', 'fwd', 62, shared=True)
        row(['E'], 17, 5, 'round', 'fwd', 63, shared=True)
        # F: 1 GiB
        row(['F', 'D'], 27, 1, 'exact', 'fwd', 70, floor=('F',))
        row(['F', 'D'], 27, 1, 'round', 'fwd', 71)
        row(['Fs'], 23, 16, 'exact', 'fwd', 72, shared=True, floor=('Fs',))
        row(['ADF'], 27, 1, 'exact', 'grad', 73, floor=('ADF',))
        # G: fewer tiles than waves, reducing
        for n in (12, 13):
            row(['G'], n, 2, 'exact', 'grad', 80 + n)
            row(['G'], n, 2, 'round', 'grad', 90 + n)
        # H: known-zero bits outside the tile on one gate list
        row(['H8'], 20, 2, 'exact', 'fwd', 100, zero_bits=3)
        row(['H4'], 20, 2, 'exact', 'fwd', 100, zero_bits=4)
    return out


ROWS = _rows()
#: the rows of the knob test (test_pass_paths_gpu.py): DQ_WAVE_GRAD_TPW = 8 walks more than two tiles only from
#: tiles * batch = 65536 on, DQ_WAVE_TPW = 2 two tiles from 16384 on; both grids are multiples of 16 (DQ_WAVE_XCD = 2)
KNOB_ROWS = [Row(('A', 'D2'), 24, 16, False, 'exact', 'grad', 110), Row(('D',), 22, 16, False, 'exact', 'fwd', 111)]


#: the settings of the knob test: one fresh process each; each is the whole environment change
KNOBS = [{'DQ_WAVE_NT': str(v)} for v in range(4)] + [{'DQ_WAVE_TILE_ORDER': 'read'}] + \
    [{'DQ_WAVE_XCD': v} for v in ('0', '2', '64')] + [{'DQ_WAVE_TPW': '2'}, {'DQ_WAVE_GRAD_TPW': '1'}, {'DQ_WAVE_GRAD_TPW': '8'},
                                                    {'DQ_WAVE_EXPZ_TPW': '1'}, {'DQ_WAVE_XCD_TPW': '0'}]


def shrunk(row):
    """The row at n <= 14 (13 for complex128) and at most five samples, same seed: for the CPU backend."""
    m = tile_bits(row.is128)
    n = min(row.n, m + 2)
    return replace(row, n=n, batch=min(row.batch, 5), zero_bits=min(row.zero_bits, n - m), paths=(), floor=())


# ---- gate lists ---------------------------------------------------------------------------------------------------------------
def exact_ops(n, ngates, seed):
    """X with 0..3 controls anywhere and diagonal gates on one or two targets with entries in {1, -1, i, -i}."""
    rng = random.Random(seed)
    ops, mats, off = [], [], 0
    for _ in range(ngates):
        kind = rng.choice(['x', 'x', 'diag', 'diag2'])
        nc = rng.choice([0, 0, 1, 1, 2, 3])
        k = 2 if kind == 'diag2' else 1
        bits = rng.sample(range(n), k + nc)
        if kind == 'x':
            ops.append(PrimOp('x', (bits[0],), tuple(bits[1:]), off, 0))
            mats.append(X2.reshape(-1))
        else:
            ops.append(PrimOp('diag', tuple(bits[:k]), tuple(bits[k:]), off, 0))
            mats.append(torch.diag(torch.tensor([rng.choice(UNITS) for _ in range(1 << k)], dtype=C128)).reshape(-1))
        off += (1 << k) ** 2
    return ops, torch.cat(mats)


def sweep_ops(base_ops, n, seed, share, targets=None):
    """A reverse sweep's gate list over the pair state (index bit 0 tells psi from lambda, every gate moves up one bit): a
    DQ_FG_GRAD record of a random variant, target (one of ``targets``, default any) and 0..2 controls anywhere in front of a
    ``share`` of the gates; rows from 1."""
    rng = random.Random(1000 + seed)
    ops, rows = [], 0
    for op in base_ops:
        if rng.random() < share:
            q = rng.choice(targets) if targets else 1 + rng.randrange(n - 1)
            ctrl = tuple(rng.sample([c for c in range(1, n) if c != q], rng.choice([0, 0, 1, 2])))
            rows += 1
            ops.append(PrimOp('grad', (q, 0), ctrl, 0, rows | (rng.randrange(5) << fusion.GRAD_VARIANT_SHIFT)))
        ops.append(PrimOp(op.kind, tuple(t + 1 for t in op.targets), tuple(c + 1 for c in op.controls), op.mat, op.mode))
    return ops, rows


def spread(ops, pos):
    """The gate list with qubit j moved to index bit pos[j]."""
    return [PrimOp(op.kind, tuple(pos[t] for t in op.targets), tuple(pos[c] for c in op.controls), op.mat, op.mode) for op in ops]


def long_pass_bits(n, seed):
    """Eight index bits of an (n - 1)-bit state that fit ONE tile whatever the geometry: the two lowest and six others, the
    top bit among them.  A sweep over gates on these alone is cut by the record cap, not by the tile."""
    rng = random.Random(3000 + seed)
    return [0, 1] + sorted(rng.sample(range(4, n - 2), 5)) + [n - 2]


def z_strings(n):
    return [1, 1 << (n - 1), (1 << (n - 1)) | 1, 0b1011 << (n // 2), (1 << n) - 1]


def per_sample_matrices(row, ops, mats):
    """(batch, total): exact rows draw every diagonal entry per sample from {1, -1, i, -i}; rounding rows give every
    diagonal gate a phase and every Rx-like gate an angle per sample (the structure a mode promises stays)."""
    rng = random.Random(2000 + row.seed)
    out = mats.unsqueeze(0).repeat(row.batch, 1)
    for b in range(row.batch):
        for op in ops:
            d = 1 << op.k
            if op.kind == 'diag' and row.kind == 'exact':
                out[b, op.mat:op.mat + d * d] = torch.diag(torch.tensor([rng.choice(UNITS) for _ in range(d)], dtype=C128)).reshape(-1)
            elif op.kind == 'diag':
                out[b, op.mat:op.mat + d * d] *= np.exp(1j * rng.uniform(0, 6.28))
            elif op.kind == 'gen' and op.mode == 2:
                c = np.cos(rng.uniform(0, 3.14))
                s = (1 - c * c) ** 0.5
                out[b, op.mat:op.mat + 4] = torch.tensor([c, -1j * s, -1j * s, c], dtype=C128)
    return out


@dataclass
class Plan:
    ops: list
    src_mats: torch.Tensor    # the caller's matrices in the row's precision: (total,) or (batch, total)
    steps: list
    nrows: int                # reduction rows 1 .. nrows; row 0 is named by no record
    kz: int                   # known-zero mask of the first pass


def plan(row):
    n = row.n
    nrows = 0
    nq = 8 if row.mode == 'ext' else n - (row.mode == 'grad')
    if row.kind == 'exact':
        ops, mats = exact_ops(nq, {'fwd': 40, 'expz': 40, 'grad': 30, 'ext': 150}[row.mode], row.seed)
    else:
        ops, mats = random_ops(nq, {'fwd': 60, 'expz': 60, 'grad': 40, 'ext': 150}[row.mode], row.seed)
        mats = mats.to(C128)
    if row.mode == 'ext':
        pos = long_pass_bits(n, row.seed)
        ops, nrows = sweep_ops(spread(ops, pos), n, row.seed, 0.5, targets=[p + 1 for p in pos])
    elif row.mode == 'grad':
        ops, nrows = sweep_ops(ops, n, row.seed, 0.5)
    elif row.mode == 'expz':
        for zm in z_strings(n):
            nrows += 1
            ops.append(PrimOp('expz', (), tuple(q for q in range(n) if (zm >> q) & 1), 0, nrows, 0, tuple(range(n))))
    geom = fusion.default_geometry(row.is128)
    geom.plan_min_bits = 11
    geom.permute_store = not row.reducing or row.mode == 'expz'       # (a sweep runs over one pair state: unpermuted)
    if row.mode == 'ext':
        geom.max_gates = 104                                          # the record cap of a sweep (executor.CONFIG['sweep_max_gates'])
    steps = fusion.schedule(ops, n, geom)
    want = (5, 11) if row.is128 else (6, 12)
    assert all(isinstance(s, fusion.FusedStep) and (s.desc.slots, s.desc.m) == want for s in steps)
    cdt = C128 if row.is128 else torch.complex64
    if row.shared:
        mats = per_sample_matrices(row, ops, mats)
    kz = 0
    if row.zero_bits:
        d = steps[0].desc
        tile = set(range(d.L)) | {d.high_pos[i] for i in range(d.h)}
        kz = sum(1 << p for p in [p for p in range(n - 1, -1, -1) if p not in tile][:row.zero_bits])
    return Plan(ops, mats.to(cdt), steps, nrows, kz)


def input_state(row, device):
    """(batch or 1, 2^n) in the row's precision, made on ``device`` from the row's seed."""
    g = torch.Generator(device=device).manual_seed(7000 + row.seed)
    nb = 1 if row.shared else row.batch
    cdt = C128 if row.is128 else torch.complex64
    if row.kind == 'exact':
        v = torch.randint(-1, 2, (nb, 1 << row.n, 2), generator=g, device=device, dtype=torch.int8)
        return torch.view_as_complex(v.to(torch.float64 if row.is128 else torch.float32))
    v = torch.randn(nb, 1 << row.n, 2, generator=g, device=device, dtype=torch.float64)
    x = torch.view_as_complex(v)
    return (x / x.norm(dim=-1, keepdim=True)).to(cdt)


# ---- what the mirror says of every pass ------------------------------------------------------------------------------------
def records_bytes(desc, n):
    nb = _lib.load().dq_wave_records(C.byref(desc), n, None, 0)
    assert nb > 0 and nb % 32 == 0
    return int(nb)


def takes_device_records(desc, n):
    return desc.rounds[desc.nrounds - 1].gate_end > 72 and records_bytes(desc, n) > 32 * backend.KERNARG_RECORDS


def step_info(row, pl):
    """One dict per pass: `_launch_geometry.wave_pass` of its launch plus what its records are (has_grad, has_expz, ext) and
    the library's own tile count (the zext word of `dq_wave_descriptor`)."""
    out = []
    for si, st in enumerate(pl.steps):
        kinds = {pl.ops[i].kind for i in st.ops}
        has_grad = 'grad' in kinds
        # the rule of backend._device_records, which itself asks the CUDA runtime for a capture and so needs a GPU: more than
        # 72 gates and reductions, and records that do not fit the kernel-argument segment.  run_kernel holds it to this.
        ext = row.reducing and takes_device_records(st.desc, row.n)
        zb = row.zero_bits if si == 0 else 0
        g = G.wave_pass(row.n, row.batch, row.is128, grad=row.reducing, only_expz=row.reducing and not has_grad and not ext, ext=ext,
                        shared_input=row.shared and si == 0, zero_bits_outside=zb)
        kp = emu.descriptor(st.desc, row.n, pl.kz if si == 0 else 0)
        nb = kp.zext & 63
        g.update(reducing=row.reducing, has_grad=has_grad, has_expz='expz' in kinds, ext=ext, zero_bits=zb,
                 only_expz=row.reducing and not has_grad and not ext, lib_tiles=1 << nb,
                 store_blk=[kp.store_blk_pos[j] for j in range(nb)])
        out.append(g)
    return out


def victim_tile(g):
    """The tile of control (i)."""
    if g['tpw'] == 2 and g['second_stride'] < g['tiles']:
        return g['second_stride']
    return 1 if g['tiles'] > 1 else 0


def dead_written(st, kz, n):
    """Index bits on the WRITE side of pass ``st`` where a known-zero bit outside its tile lands (nothing is written where
    one of them is 1)."""
    d = st.desc
    tile = set(range(d.L)) | {d.high_pos[i] for i in range(d.h)}
    blk = [p for p in range(d.L, n) if p not in tile]
    return [d.store_blk_pos[j] for j, p in enumerate(blk) if (kz >> p) & 1]


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def run_kernel(row, pl, x):
    """The row's passes through `backend.apply_fused` on the device of ``x`` -> (state, accumulator or None).  Every output
    starts as NaN; where a known-zero pass must not write it must still be NaN afterwards and is then set to zero."""
    dev = x.device
    km = fusion.kernel_matrices(pl.steps, pl.ops, pl.src_mats).to(dev)
    stride = km.shape[1] if km.ndim == 2 and km.shape[0] > 1 else 0
    md = km.reshape(-1).contiguous()
    acc = torch.full((row.batch, pl.nrows + 1, 8), 0.5, dtype=torch.float64, device=dev) if row.reducing else None
    idx = torch.arange(1 << row.n, device=dev)
    cur = x
    for si, st in enumerate(pl.steps):
        out = torch.full((row.batch, 1 << row.n), float('nan'), dtype=x.dtype, device=dev)
        kz = pl.kz if si == 0 else 0
        src = cur
        if kz and not row.shared:
            src = cur.clone()
            src[:, (idx & kz) != 0] = float('nan')            # (must not be read)
        backend.apply_fused(src, md, stride, st.desc, out=out, grads=acc, known_zero=kz)
        if row.reducing and x.is_cuda:      # (what the backend did with the records is what step_info said it would)
            took = any(t is not None for t in st.desc.__dict__.get('_dev_records', {}).values())
            assert took == takes_device_records(st.desc, row.n), (row.id, si)
        if kz:
            wmask = sum(1 << p for p in dead_written(st, kz, row.n))
            dead = (idx & wmask) != 0
            assert bool(torch.isnan(out[:, dead].real).all()), 'a tile that a known-zero bit excludes was written'
            out[:, dead] = 0
        cur = out
    return cur, acc


def digest(state, acc):
    h = hashlib.sha256()
    for t in (state, acc):
        if t is not None:
            h.update(torch.view_as_real(t).cpu().numpy().tobytes() if t.is_complex() else t.cpu().numpy().tobytes())
    return h.hexdigest()


# ---- the reference ------------------------------------------------------------------------------------------------------------
class _Tau:
    def __init__(self, is128, ops):
        self.is128 = is128
        self.cfg = type('cfg', (), {'ops': ops})


def reference(row, pl, x, info, order=None):
    """-> dict(out, abs, acc, bound, before_last, drop): the final state in complex128, the gates applied to absolute values
    (rounding rows), the accumulator rows (B, nrows + 1, 8; NaN where nothing is added), the bound of every formed
    component (rounding rows), the state in front of the last pass and the victim tiles' share of every sum of sample 0.
    ``order``: op indices to apply instead of the passes' own order (no per-pass results then)."""
    dev = x.device
    nb, n = row.batch, row.n
    rm = pl.src_mats.to(C128).to(dev)
    rm = rm if rm.ndim == 2 else rm.unsqueeze(0)
    idx_all = torch.arange(1 << n, device=dev)
    cur = x.to(C128).expand(nb, -1).clone()
    if pl.kz:
        assert bool((cur[:, (idx_all & pl.kz) != 0] == 0).all())
    rounding = row.kind == 'round'
    ab = cur.abs().to(C128) if rounding else None
    acc = torch.full((nb, pl.nrows + 1, 8), float('nan'), dtype=torch.float64, device=dev)
    bound = torch.full_like(acc, float('nan'))
    drop = torch.zeros_like(acc)
    before_last = None
    u = hc.U[False]
    tau_cum = 0.0
    groups = [(si, st.ops) for si, st in enumerate(pl.steps)] if order is None else [(None, order)]
    for si, op_ids in groups:
        if si is not None:
            if si == len(pl.steps) - 1:
                before_last = cur.clone()
            tau_cum += hc.tau_amplitudes(_Tau(row.is128, [pl.ops[i] for i in op_ids]))
            g = info[si]
            held = dead_written(pl.steps[si], pl.kz, n) if si == 0 and pl.kz else ()
            vidx, vfree = R.tile_indices(n, g['store_blk'], victim_tile(g), dev, held)
        for oi in op_ids:
            op = pl.ops[oi]
            if op.kind == 'grad':
                r, variant = op.mode & fusion.GRAD_ROW_MASK, op.mode >> fusion.GRAD_VARIANT_SHIFT
                t, s = op.targets
                gs, sa = R.grad_sums(cur, t, s, op.controls)
                acc[:, r], sabs = R.grad_components(gs, sa, variant)
                if rounding:
                    base = hc.TAU_SUM if row.is128 else 2 * (hc.M_GRAD + 2) * u
                    bound[:, r] = (base + 2 * tau_cum) * sabs
                if si is not None:
                    assert not pl.steps[si].permutes
                    tg, ta = R.tile_grad_sums(cur[:1], vidx, vfree, t, s, op.controls)
                    drop[0, r] = torch.nan_to_num(R.grad_components(tg, ta, variant)[0][0])
            elif op.kind == 'expz':
                r = op.mode
                zm = sum(1 << q for q in op.controls)
                val, sp = R.expect_z_multi(cur, [zm])
                acc[:, r, 0] = val[:, 0]
                if rounding:
                    base = hc.TAU_SUM if row.is128 else (hc.M_EXPZ + 2) * u
                    bound[:, r, 0] = (base + 2 * tau_cum) * sp[:, 0]
                if si is not None:
                    assert si == len(pl.steps) - 1, 'the Z strings come out of the last pass'
                    drop[0, r, 0] = (R.probabilities(cur[0, vidx]) * R.z_sign(vidx, zm)).sum()
            else:
                d = 1 << op.k
                m = X2.to(dev) if op.kind == 'x' else rm[:, op.mat:op.mat + d * d].reshape(-1, d, d)
                cur = R.apply_gate(cur, m, list(op.targets), list(op.controls))[0]
                if rounding:
                    ab = R.apply_gate(ab, m.abs().to(C128), list(op.targets), list(op.controls))[0]
    return dict(out=cur, abs=None if ab is None else ab.real, acc=acc, bound=bound, before_last=before_last, drop=drop,
                tau=tau_cum, victim=(vidx if order is None else None))


# ---- criteria -----------------------------------------------------------------------------------------------------------------
INF = float('inf')


def state_ratio(row, got, ref):
    """exact rows: 0 if bit for bit equal, else inf; rounding rows: max |got - ref| / (tau S), inf for a NaN."""
    g = got.to(C128)
    if row.kind == 'exact':
        return 0.0 if torch.equal(torch.view_as_real(g), torch.view_as_real(ref['out'])) else INF
    ratio = (g - ref['out']).abs() / (ref['tau'] * ref['abs'])
    return float(torch.nan_to_num(ratio, nan=INF).max())


def acc_ratio(row, acc, ref):
    """inf unless exactly the components the reference forms changed; exact rows: 0 if those equal the reference, else
    inf; rounding rows: max |got - ref| / bound."""
    formed = ~torch.isnan(ref['acc'])
    if not bool((acc[~formed] == 0.5).all()):
        return INF
    if not bool(formed.any()):
        return 0.0
    if row.kind == 'exact':
        return 0.0 if bool((acc[formed] == ref['acc'][formed] + 0.5).all()) else INF
    ratio = (acc[formed] - 0.5 - ref['acc'][formed]).abs() / ref['bound'][formed]
    return float(torch.nan_to_num(ratio, nan=INF).max())


def corruptions(row, pl, ref, info):
    """[(what, state, accumulator or None)]: the reference's results as a wrong launch path would leave them."""
    out = []
    good = ref['out']
    acc = None if not row.reducing else torch.where(torch.isnan(ref['acc']), 0.5, ref['acc'] + 0.5)
    v = ref['victim']
    bad = good.clone()
    bad[0, v] = ref['before_last'][0, v]
    if torch.equal(torch.view_as_real(bad), torch.view_as_real(good)):      # (the last pass is the identity on this tile: what an
        bad[0, v] = float('nan')                                            # unwalked tile of these out-of-place passes holds)
    bad_acc = None if acc is None else acc - ref['drop']
    out.append(('i', bad, bad_acc))
    if row.shared:
        t0, _ = R.tile_indices(row.n, info[-1]['store_blk'], 0, good.device)
        bad = good.clone()
        bad[0, t0], bad[1, t0] = good[1, t0], good[0, t0]
        out.append(('ii', bad, acc))
    if any(g['nt_stores'] for g in info):
        other = next(j for j in range(3, 1 << row.n, 2) if bool(good[0, j] != good[0, 1]))     # (an exact row's may be equal)
        bad = good.clone()
        bad[0, 1], bad[0, other] = good[0, other], good[0, 1]
        out.append(('iii', bad, acc))
    return out


def run_row(row, device, check_paths=True):
    """Runs the row on ``device`` and asserts its paths, its criterion and the negative controls; -> dict of the measured
    ratios (state, sums, whether the sums alone reject control (i))."""
    pl = plan(row)
    info = step_info(row, pl)
    for g in info:
        assert g['tiles'] == g['lib_tiles'], (row.id, g)
    if check_paths:
        for p in row.paths:
            assert any(PATHS[p](g) for g in info), f'{row.id}: no pass reaches path {p}: {info}'
    x = input_state(row, device)
    if pl.kz:
        x[:, (torch.arange(1 << row.n, device=device) & pl.kz) != 0] = 0
    x0 = x.clone()
    got, acc = run_kernel(row, pl, x)
    assert torch.equal(torch.view_as_real(x), torch.view_as_real(x0)), f'{row.id}: the input changed'
    ref = reference(row, pl, x, info)
    res = dict(state=state_ratio(row, got, ref), sums=None, sums_reject_i=None)
    assert res['state'] <= 1.0, f'{row.id}: state, worst |got - ref| / (tau S) = {res["state"]:.3e}'
    if row.reducing:
        assert bool((acc[:, 0] == 0.5).all()), f'{row.id}: a row no record names changed'
        res['sums'] = acc_ratio(row, acc, ref)
        assert res['sums'] <= 1.0, f'{row.id}: sums, worst |got - ref| / bound = {res["sums"]:.3e}'
    for what, bad, bad_acc in corruptions(row, pl, ref, info):
        assert state_ratio(row, bad, ref) > 1.0, f'{row.id}: the state criterion does not see corruption ({what})'
        if what == 'i' and row.reducing and bool((ref['drop'] != 0).any()):
            res['sums_reject_i'] = acc_ratio(row, bad_acc, ref) > 1.0
            assert res['sums_reject_i'] or row.kind == 'round', f'{row.id}: the exact sums do not see a dropped tile'
    return res
