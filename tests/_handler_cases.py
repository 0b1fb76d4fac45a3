"""One minimal pass per handler body of the wave-tile kernel -- TEST INFRASTRUCTURE ONLY, no GPU.

The handler id of a gate depends on the PHYSICAL register slot the translator (csrc/dq_wave.hip, wave_translate) has put
its tile bit in, which the host does not choose.  So nothing is predicted here: `configs` enumerates small passes
deterministically -- one or two hand-chosen rounds through ``fusion._finalize``; the gate under test with its target on
every tile bit in turn and its controls on a register slot / a lane bit / outside the tile; for trips and swaps a first
round that only forces a layout and a second that needs another slot set, with and without a re-labelling store
(``wpos``) -- `_handler_census.ids` says which ids each contains, and `cases` keeps for every id (and for every feature of
a family) the configuration with the fewest records.  Bound of the enumeration: at most 4000 configurations per
precision (asserted), each translated once on the host; it runs on first use and is cached.

Sizes: n = m + 1 (m = 12 / 11: two tiles, one index bit outside the tile); n = m + 2 where a diagonal gate needs two tile
selectors.  The default tile is index bits 0 .. m-1, so tile-local and index bits coincide below m.

Matrices (`matrices`): random unitaries from the QR of a float64 complex Gaussian (real 2x2 matrices and blocks: four
unrelated entries, see `_unitary`), ROUNDED TO THE KERNEL'S PRECISION FIRST -- the reference uses the rounded values -- and of exactly the structure a mode promises; the X-shaped 4x4 modes of
complex64 carry non-zero garbage in the entries their bodies promise never to read, which the reference zeroes.

`reference` applies the same gates one by one in complex128 with plain index arithmetic, and in parallel to absolute
values (`|U| |x|`: what each output element was summed from), and forms the reductions' sums."""

from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

import _handler_census as census
import _wave_emulator as emu
from deepquantum_amd import fusion
from deepquantum_amd.fusion import PrimOp

MAX_CONFIGS = 4000
U = {False: 2.0 ** -24, True: 2.0 ** -53}

#: Handler ids no valid DqFusedPass reaches, with the lines of wave_translate (csrc/dq_wave.hip) that exclude them.  An id
#: may only be listed here with such a citation; `test_handler_census_cpu` checks that none of them is reached after all.
#: the only statements of wave_translate that emit a swap record, and its third use of swap_id (an index offset into the 4x4
#: bodies, not a record); test_handler_census_cpu.py holds them against the text of csrc/dq_wave.hip
SWAP_SITES = ('sw.w[0] = (uint32_t)W::swap_id(0, ps);', 'rec.w[0] = (uint32_t)W::swap_id(0, s0);')
SWAP_OFFSET_USE = 'rec.w[0] = (uint32_t)(body + (W::swap_id(a, b) - W::ID_SWAP));'
_SWAP_WHY = (f'wave_translate only ever emits swap_id(0, s): `{SWAP_SITES[0]}` (the psi / lambda bit of a DQ_FG_GRAD record back '
             f'to slot 0) and `{SWAP_SITES[1]}` (the store layout of complex64); the third use, `{SWAP_OFFSET_USE}`, is an '
             'index offset into the 4x4 bodies, not a swap record')


def unreachable(is128):
    g = emu.gen(is128)
    return {g.ID_SWAP + i: _SWAP_WHY for i, (a, _) in enumerate(g.SWAP_PAIRS) if a != 0}


UNREACHABLE = {'c64': unreachable(False), 'c128': unreachable(True)}


@dataclass
class Config:
    label: str
    n: int
    ops: list
    rounds: list                  # [(index bits that must be register slots, [op indices])]
    wpos: list | None = None
    nrows: int = 0
    pure: bool = False            # only X gates: every record moves amplitudes, nothing rounds
    keep: bool = False            # a case of its own whatever the search prefers (a reduction behind deferred factors)


@dataclass
class Case:
    hid: int
    cfg: Config
    is128: bool
    records: list = field(default_factory=list)
    batched: bool = False
    seed: int = 0

    @property
    def name(self):
        return f'{census.name(self.hid, self.is128)} [{self.cfg.label}]'


class _Ops:
    def __init__(self):
        self.ops, self.off, self.rows = [], 0, 0

    def gen(self, t, c=(), mode=0):
        self.ops.append(PrimOp('gen', (t,), tuple(c), self.off, mode))
        self.off += 4
        return len(self.ops) - 1

    def gen2(self, t1, t2, c=(), mode=0):
        self.ops.append(PrimOp('gen', (t1, t2), tuple(c), self.off, mode))
        self.off += 16
        return len(self.ops) - 1

    def x(self, t, c=()):
        self.ops.append(PrimOp('x', (t,), tuple(c), 0, 0))
        return len(self.ops) - 1

    def diag(self, ts, c=()):
        self.ops.append(PrimOp('diag', tuple(ts), tuple(c), self.off, 0))
        self.off += (1 << len(ts)) ** 2
        return len(self.ops) - 1

    def grad(self, t, s, c=(), variant=0):
        self.ops.append(PrimOp('grad', (t, s), tuple(c), 0, self.rows | (variant << fusion.GRAD_VARIANT_SHIFT)))
        self.rows += 1
        return len(self.ops) - 1

    def expz(self, zbits, n):
        self.ops.append(PrimOp('expz', (), tuple(zbits), 0, self.rows, 0, tuple(range(n))))
        self.rows += 1
        return len(self.ops) - 1


def _one_round(label, n, o, slots, **kw):
    return Config(label, n, o.ops, [(sorted(set(slots)), list(range(len(o.ops))))], nrows=o.rows, **kw)


def configs(is128):
    """The bounded, deterministic enumeration (see the module docstring)."""
    geom = fusion.default_geometry(is128)
    m, R, vb, L = geom.m, geom.slots, geom.vb, geom.min_low
    n, out = m + 1, m
    io = list(range(vb)) + list(range(m - (R - vb), m))          # the default I/O layout's slots
    lane = 1 if vb else 0                                          # always a lane bit of an I/O layout
    lane2 = lane + 1

    def other(*used):          # a default-slot bit that is none of `used`
        return next(b for b in reversed(io) if b not in used)

    # ---- one-target gates: dense (four promised structures), X, diagonal -------------------------------------------------
    for t in range(m):
        lc = lane if t != lane else lane2
        rc = other(t)
        ctrls = [('none', (), ()), ('lane', (lc,), ()), ('out', (out,), ()), ('reg', (rc,), (rc,)), ('reg+lane', (rc, lc), (rc,)),
                 ('reg+out', (rc, out), (rc,)), ('reg2', (rc, other(t, rc)), (rc, other(t, rc))),
                 ('reg2+lane', (rc, other(t, rc), lc), (rc, other(t, rc))), ('reg2+out', (rc, other(t, rc), out), (rc, other(t, rc)))]
        for cn, cb, cs in ctrls:
            for mode in range(4):
                o = _Ops()
                o.gen(t, cb, mode)
                yield _one_round(f'gen mode={mode} t={t} ctl={cn}', n, o, [t, *cs])
            o = _Ops()
            o.x(t, cb)
            yield _one_round(f'x t={t} ctl={cn}', n, o, [t, *cs], pure=True)
            o = _Ops()
            o.diag([t], cb)
            yield _one_round(f'diag t={t} ctl={cn}', n, o, [t, *cs])
            o = _Ops()
            o.diag([t], cb)
            yield _one_round(f'diag t={t} on a lane ctl={cn}', n, o, [other(t), *cs])
    for t in io:                                                   # X with one register control: every (target, control) pair
        for c in io:
            if c != t:
                o = _Ops()
                o.x(t, (c,))
                yield _one_round(f'x t={t} ctl=reg {c}', n, o, [t, c], pure=True)
    for cn, cb, cs in [('none', (), ()), ('reg', (io[-1],), (io[-1],)), ('lane', (lane2,), ())]:
        o = _Ops()
        o.diag([out], cb)
        yield _one_round(f'diag t=outside ctl={cn}', n, o, [io[-2], *cs])
    # ---- diagonal gates on two targets -----------------------------------------------------------------------------------
    n2 = m + 2
    for t in io:
        rc = other(t)
        for cn, cb, cs in [('none', (), ()), ('reg', (rc,), (rc,)), ('lane', (lane2,), ())]:
            for pn, p, ps in [('reg', other(t, rc), True), ('lane', lane, False), ('out', m, False)]:
                for first in (0, 1):
                    o = _Ops()
                    o.diag([t, p] if first == 0 else [p, t], cb)
                    yield _one_round(f'diag2 reg t={t} + {pn} order={first} ctl={cn}', n2, o, [t, *cs] + ([p] if ps else []))
    for (an, a), (bn, b) in itertools.permutations([('lane', lane), ('lane2', lane2), ('out', m), ('out2', m + 1)], 2):
        for cn, cb, cs in [('none', (), ()), ('reg', (io[-1],), (io[-1],)), ('out', (m + 1,), ())]:
            if set(cb) & {a, b}:
                continue
            o = _Ops()
            o.diag([a, b], cb)
            yield _one_round(f'diag2 {an} + {bn} ctl={cn}', n2, o, [io[-2], *cs])
    # ---- dense gates on two targets: every slot pair, both target orders, four promised structures --------------------------
    for t1, t2 in itertools.permutations(io, 2):
        rc = other(t1, t2)
        for mode in (0, 1, 4, 5):
            for cn, cb, cs in [('none', (), ()), ('lane', (lane,), ()), ('out', (out,), ()), ('reg', (rc,), (rc,))]:
                if cn != 'none' and (t1 + t2 + mode) % 3:          # (controls on a third of the pairs)
                    continue
                o = _Ops()
                o.gen2(t1, t2, cb, mode)
                yield _one_round(f'gen2 mode={mode} t=({t1},{t2}) ctl={cn}', n, o, [t1, t2, *cs])
    # ---- reductions of the reverse sweep: five variants, behind nothing / a Hadamard / a deferred Rx -----------------------
    for t in [b for b in io if b != 0] + [L - 1]:
        for variant in range(5):
            rc = other(t, 0)
            hb = other(t, 0, rc)
            for cn, cb, cs in [('none', (), ()), ('reg', (rc,), (rc,)), ('lane', (lane2,), ()), ('out', (out,), ())]:
                for pre in ('none', 'had', 'rx', 'had+rx'):
                    if cn != 'none' and pre not in ('none', 'had+rx'):
                        continue
                    o = _Ops()
                    if 'had' in pre:
                        o.gen(hb, (), 3)
                    if 'rx' in pre:
                        o.gen(t, (), 2)
                    o.grad(t, 0, cb, variant)
                    yield _one_round(f'grad variant={variant} t={t} ctl={cn} behind={pre}', n, o, [t, 0, hb, *cs],
                                     keep=t == io[-1] and pre == 'had+rx' and cn in ('none', 'reg'))
    # ---- <Z..Z> from the registers -----------------------------------------------------------------------------------------
    for zn, zb in [('reg', (io[-1],)), ('lane', (lane,)), ('out', (out,)), ('reg+lane+out', (io[-1], io[-2], lane, lane2, out)),
                   ('all', tuple(range(n))), ('reg+lane', (io[-1], lane)), ('lane+out', (lane, out))]:
        for pre in ('none', 'had', 'rx'):
            o = _Ops()
            if pre == 'had':
                o.gen(io[-3], (), 3)
            if pre == 'rx':
                o.gen(io[-3], (), 2)
            o.expz(zb, n)
            yield _one_round(f'expz z={zn} behind={pre}', n, o, [io[-1], io[-2], io[-3]], keep=zn == 'reg+lane+out' and pre != 'none')
    # ---- layout changes: a first round in the default layout, a second that drops k of its slots for lane bits ----------------
    lanes0 = [b for b in range(m) if b not in io]
    wposes = [('', None)]
    for a, b in [(lanes0[0], lanes0[1]), (0, lanes0[0]), (0, io[-1]), (lanes0[0], io[-1]), (io[1], io[-1]), (io[-1], out), (0, L)]:
        w = list(range(n))
        w[a], w[b] = b, a
        wposes.append((f' store {a}<->{b}', w))
    for wn, w in wposes:
        o = _Ops()
        yield Config(f'x in the default layout{wn}', n, o.ops, [(io, [o.x(io[-1]), o.x(io[-2])])], w, pure=True)
    for k in range(1, emu.gen(is128).MAXK + 1):
        for drop in itertools.combinations(io, k):
            for inc in ([lanes0[:k]] if lanes0[:k] == lanes0[-k:] else [lanes0[:k], lanes0[-k:]]):
                second = [b for b in io if b not in drop] + list(inc)
                for wn, w in (wposes if k == 1 else wposes[:1]):
                    o = _Ops()
                    a, b = o.x(second[0]), o.x(second[-1])
                    yield Config(f'layout {io} -> drop {list(drop)} for {list(inc)}{wn}', n, o.ops, [(io, [a]), (second, [b])], w, pure=True)
    # ---- a reduction whose psi / lambda bit is not on slot 0: it comes back there by a swap -------------------------------------
    for d in io:                       # (slots = the default ones without d, plus index bit 0: it takes the lowest slot that leaves)
        for t in [b for b in io if b not in (d, 0)][:2]:
            o = _Ops()
            o.grad(t, 0, (), 0)
            yield _one_round(f'grad t={t} in slots {[0] + [b for b in io if b != d]}', n, o, [0] + [b for b in io if b != d])
        first = [b for b in io if b != d and b != 0][:R - 2] + lanes0[-2:]
        t = first[0]
        o = _Ops()
        a = o.x(first[-1])
        b = o.grad(t, 0, (), 0)
        yield Config(f'layout {first} then grad t={t}', n, o.ops, [(first, [a]), ([0, t], [b])], nrows=o.rows)


def build(cfg, is128):
    """The FusedStep of a configuration (a fresh descriptor every time: layout_matrices writes into it)."""
    geom = fusion.default_geometry(is128)
    rounds = [fusion._Round(slots=list(s), ops=list(i)) for s, i in cfg.rounds]
    ops = [PrimOp(op.kind, op.targets, op.controls, op.mat, op.mode, 0, op.order) for op in cfg.ops]
    return fusion._finalize(ops, cfg.n, geom, set(), rounds, cfg.wpos), ops


@functools.lru_cache(maxsize=None)
def cases(is128):
    """[Case]: for every reachable handler id the configuration with the fewest records that contains it, then one more per
    (family, feature) that those do not show.  Movement families take configurations made of X gates only."""
    best, feat, kept = {}, {}, []
    count = 0
    for cfg in configs(is128):
        count += 1
        step, _ = build(cfg, is128)          # (every configuration is a pass the geometry carries out: an error is an error)
        recs = census.ids(step.desc, cfg.n, is128)
        if cfg.keep:
            kept.append(Case([r for r in recs if r.family in ('GRAD', 'EXPZ')][-1].hid, cfg, is128, recs))
        for r in recs:
            key = (r.family in census.MOVES and not cfg.pure, len(recs))
            if r.hid not in best or key < best[r.hid][0]:
                best[r.hid] = (key, cfg, recs)
            for f in r.features:
                if (r.family, f) not in feat or key < feat[(r.family, f)][0]:
                    feat[(r.family, f)] = (key, cfg, recs, r.hid)
    assert count <= MAX_CONFIGS, count
    out = [Case(hid, cfg, is128, recs) for hid, (_, cfg, recs) in sorted(best.items())]
    shown = {(r.family, f) for c in out for r in c.records if r.hid == c.hid for f in r.features}
    for (fam, f), (_, cfg, recs, hid) in sorted(feat.items()):
        if (fam, f) not in shown:
            out.append(Case(hid, cfg, is128, recs))
            shown |= {(r.family, f2) for r in recs if r.hid == hid for f2 in r.features}
    out += kept
    for i, c in enumerate(out):
        c.seed = 1000 + i
        c.batched = i % 2 == 0          # per-sample matrices (mat_batch_stride != 0) in every other case
    return out


# ---- matrices ---------------------------------------------------------------------------------------------------------------
def _round_to(a, is128):
    return a if is128 else a.astype(np.complex64).astype(np.complex128)


def _unitary(rng, d, real=False):
    a = rng.standard_normal((d, d)) + (0 if real else 1j * rng.standard_normal((d, d)))
    if real and d == 2:
        # NOT orthogonal: a real orthogonal 2x2 is a rotation (m00 = m11) or a reflection (m01 = m10, all the QR of a 2x2
        # ever gives), and a body that reads one entry for the other would compute the same.  Four unrelated real entries,
        # scaled to spectral norm 1 -- real is all the mode promises
        return (a / np.linalg.norm(a, 2)).astype(np.complex128)
    return np.linalg.qr(a)[0].astype(np.complex128)


XSHAPE = np.array([[(i ^ j) in (0, 3) for j in range(4)] for i in range(4)])


def matrices(case, nb=2):
    """(src, ref): the caller's matrix buffer (Bm, total), rounded to the precision, and what the reference applies (the
    entries a body promises not to read zeroed).  Bm = nb for a batched case, else 1."""
    bm = nb if case.batched else 1
    total = max(1, sum((1 << op.k) ** 2 for op in case.cfg.ops if op.kind in ('gen', 'diag')))
    src, ref = np.zeros((bm, total), np.complex128), np.zeros((bm, total), np.complex128)
    for oi, op in enumerate(case.cfg.ops):
        if op.kind not in ('gen', 'diag'):
            continue
        d = 1 << op.k
        for s in range(bm):
            rng = np.random.default_rng([case.seed, oi, s])
            garbage = None
            if op.kind == 'diag':
                mtx = np.diag(np.exp(1j * rng.uniform(0, 2 * np.pi, d)))
            elif op.k == 1:
                if op.mode == 0:
                    mtx = _unitary(rng, 2)
                elif op.mode == 1:
                    mtx = _unitary(rng, 2, real=True)
                elif op.mode == 2:      # a I + i b X: |a| >= |b| and |a| < |b| in turn (the two forms of the deferred block)
                    phi = rng.uniform(0.1, 0.6) if (case.seed + oi + s) % 2 == 0 else rng.uniform(1.0, 1.4)
                    a, b = np.cos(phi), -np.sin(phi)
                    mtx = np.array([[a, 1j * b], [1j * b, a]])
                else:
                    sgn = 1.0 if s == 0 else -1.0
                    mtx = sgn * 2 ** -0.5 * np.array([[1, 1], [1, -1]], np.complex128)
            else:
                if op.mode == 0:
                    mtx = _unitary(rng, 4)
                elif op.mode == 1:
                    mtx = _unitary(rng, 4, real=True)
                else:
                    mtx = np.zeros((4, 4), np.complex128)
                    for blk in ([0, 3], [1, 2]):
                        mtx[np.ix_(blk, blk)] = _unitary(rng, 2, real=op.mode == 4)
                    if not case.is128:      # (complex128 has no X-shaped bodies: its real / general bodies read every entry)
                        garbage = np.where(XSHAPE, 0, rng.standard_normal((4, 4)) + (0 if op.mode == 4 else 1j * rng.standard_normal((4, 4))))
            mtx = _round_to(mtx.astype(np.complex128), case.is128)
            ref[s, op.mat:op.mat + d * d] = mtx.reshape(-1)
            src[s, op.mat:op.mat + d * d] = (mtx if garbage is None else mtx + _round_to(garbage, case.is128)).reshape(-1)
    return src, ref


def state(case, nb=2, seed_shift=0):
    """(nb, 2^n) complex128: a seeded random normalised state, rounded to the precision."""
    rng = np.random.default_rng([case.seed, 77 + seed_shift])
    x = rng.standard_normal((nb, 1 << case.cfg.n)) + 1j * rng.standard_normal((nb, 1 << case.cfg.n))
    return _round_to(x / np.linalg.norm(x, axis=-1, keepdims=True), case.is128)


def kernel_inputs(case, src):
    """(step, kernel matrix buffer as a torch tensor of the precision, mat_batch_stride)."""
    import torch

    step, ops = build(case.cfg, case.is128)
    dt = torch.complex128 if case.is128 else torch.complex64
    km = fusion.kernel_matrices([step], ops, torch.from_numpy(src).to(dt))
    return step, km, (km.shape[1] if km.shape[0] > 1 else 0)


# ---- the complex128 reference ---------------------------------------------------------------------------------------------
def apply_np(x, mtx, targets, controls):
    """x (B, N) -> the gate applied: mtx (Bm, d, d), Bm in (1, B); targets in matrix order, MSB first."""
    nn = x.shape[1]
    idx = np.arange(nn)
    sel = np.ones(nn, bool)
    for c in controls:
        sel &= ((idx >> c) & 1) == 1
    for t in targets:
        sel &= ((idx >> t) & 1) == 0
    base = idx[sel]
    k = len(targets)
    rows = [base | sum(((r >> (k - 1 - i)) & 1) << t for i, t in enumerate(targets)) for r in range(1 << k)]
    xin = np.stack([x[:, r] for r in rows], axis=1)                 # (B, d, cols)
    y = np.einsum('brc,bcn->brn', np.broadcast_to(mtx, (x.shape[0],) + mtx.shape[1:]), xin)
    out = x.copy()
    for r, ix in enumerate(rows):
        out[:, ix] = y[:, r]
    return out


def relabel(x, wpos):
    idx = np.arange(x.shape[1])
    dest = sum(((idx >> p) & 1) << w for p, w in enumerate(wpos))
    out = np.empty_like(x)
    out[:, dest] = x
    return out


def grad_sums(x, t, s, controls):
    """G[a][b] = sum lambda[t = a] conj(psi[t = b]) (index bit s: 0 = psi, 1 = lambda), controls all 1: (B, 2, 2)."""
    idx = np.arange(x.shape[1])
    sel = (((idx >> t) & 1) == 0) & (((idx >> s) & 1) == 0)
    for c in controls:
        sel &= ((idx >> c) & 1) == 1
    base = idx[sel]
    g = np.zeros((x.shape[0], 2, 2), np.complex128)
    for a in range(2):
        for b in range(2):
            g[:, a, b] = (x[:, base | (a << t) | (1 << s)] * np.conj(x[:, base | (b << t)])).sum(-1)
    return g


def grad_components(g, variant, absolute=False):
    """The eight components a DQ_FG_GRAD record of this variant adds (include/dq_hip.h); NaN = left untouched.  With
    ``absolute``, ``g`` holds the sums over absolute values and every formed component gets the sum it was formed from."""
    full = np.stack([g[:, 0, 0].real, g[:, 0, 0].imag, g[:, 0, 1].real, g[:, 0, 1].imag,
                     g[:, 1, 0].real, g[:, 1, 0].imag, g[:, 1, 1].real, g[:, 1, 1].imag], axis=1)
    if absolute:
        full = np.repeat(np.stack([g[:, 0, 0], g[:, 0, 1], g[:, 1, 0], g[:, 1, 1]], axis=1).real, 2, axis=1)
    out = np.full_like(full, np.nan)
    if variant == 0:
        out[:] = full
    elif variant == 1:
        out[:, 0::2] = full[:, 0::2]
    elif variant == 2:
        out[:, 0] = full[:, 0] + full[:, 6]
        out[:, 3] = full[:, 3] + full[:, 5]
    elif variant == 3:
        out[:, [0, 1, 6, 7]] = full[:, [0, 1, 6, 7]]
    else:
        out[:, 3] = full[:, 3] + full[:, 5]
    return out


def reference(case, x, ref_mats, ops=None):
    """The pass in complex128, gate by gate: {'out', 'abs' (the same gates applied to absolute values), 'acc' (B, rows, 8;
    NaN where nothing is added), 'acc_abs', 'touched' (bool mask of the amplitudes some gate's controls include)}."""
    cfg = case.cfg
    ops = cfg.ops if ops is None else ops
    order = [i for _, idx in cfg.rounds for i in idx]
    nb = x.shape[0]
    cur, ab = x.copy(), np.abs(x).astype(np.complex128)
    acc = np.full((nb, cfg.nrows, 8), np.nan)
    acc_abs = np.full((nb, cfg.nrows, 8), np.nan)
    idx = np.arange(x.shape[1])
    touched = np.zeros(x.shape[1], bool)
    for oi in order:
        op = ops[oi]
        if op.kind == 'grad':
            row, variant = op.mode & fusion.GRAD_ROW_MASK, op.mode >> fusion.GRAD_VARIANT_SHIFT
            acc[:, row] = grad_components(grad_sums(cur, op.targets[0], op.targets[1], op.controls), variant)
            acc_abs[:, row] = grad_components(grad_sums(ab, op.targets[0], op.targets[1], op.controls), variant, absolute=True)
            continue
        if op.kind == 'expz':
            par = np.zeros(x.shape[1], np.int64)
            for q in op.controls:
                par ^= (idx >> q) & 1
            p = cur.real ** 2 + cur.imag ** 2
            acc[:, op.mode, 0] = (p * (1.0 - 2.0 * par)).sum(-1)
            acc_abs[:, op.mode, 0] = (ab.real ** 2).sum(-1)
            continue
        d = 1 << op.k
        if op.kind == 'x':
            mtx = np.array([[[0, 1], [1, 0]]], np.complex128)
        else:
            mtx = ref_mats[:, op.mat:op.mat + d * d].reshape(-1, d, d)
        cur = apply_np(cur, mtx, op.targets, op.controls)
        ab = apply_np(ab, np.abs(mtx).astype(np.complex128), op.targets, op.controls)
        hit = np.ones(x.shape[1], bool)
        for c in op.controls:
            hit &= ((idx >> c) & 1) == 1
        touched |= hit
    if cfg.wpos is not None:
        cur, ab = relabel(cur, cfg.wpos), relabel(ab, cfg.wpos)
    return {'out': cur, 'abs': ab.real, 'acc': acc, 'acc_abs': acc_abs, 'touched': touched}


# ---- the derived bounds -------------------------------------------------------------------------------------------------
def gamma(k, is128):
    u = U[is128]
    return k * u / (1 - k * u)


def roundings(op, is128):
    """(r, deferred): how many roundings one real component of an output amplitude of this gate can pass through.

    A component of  y_i = sum_j u_ij x_j  (k terms) is a real dot product of 2k products (k where the matrix is promised
    real and the body reads no imaginary part), each rounded once and added in at most 2k - 1 further roundings -- fused
    multiply-adds and any order of summation only lower this --: gamma_2k resp. gamma_k relative to  sum |products| <=
    (|U| |x|)_i  (Cauchy-Schwarz on the real and imaginary parts).  A product with an exact zero is exact, so the count
    holds whatever structure the matrix has.  X moves round nothing.
    The deferred forms: Hadamard = one addition, Rx = the division t = b / a on the host, the product t x and one addition;
    each also takes part in forming the pass's factor (one complex product: two roundings)."""
    if op.kind in ('x', 'grad', 'expz'):
        return 0, False
    k = 1 << op.k
    if op.kind == 'diag':
        return 2, False
    uncontrolled = not op.controls
    if op.k == 1:
        if op.mode == 3 and uncontrolled:
            return 1 + 2, True
        if op.mode == 2 and uncontrolled and not is128:
            return 3 + 2, True
        return (2 if op.mode == 1 and uncontrolled else 4), False
    if op.mode == 1:
        return 4, False
    if op.mode == 4:
        return (4 if is128 else 2), False
    if op.mode == 5:
        return (8 if is128 else 4), False
    return 2 * k, False


def tau_amplitudes(case, ops=None):
    """|got_i - ref_i| <= tau (|U_G| .. |U_1| |x|)_i to first order: the roundings of the pass's arithmetic records summed (an
    earlier record's error is carried through the later ones inside the same bound), two more for the multiplication by the
    pass's deferred factor where there is one, times sqrt 2 from the two components of a complex number."""
    r, deferred = 0, False
    for op in (case.cfg.ops if ops is None else ops):
        ri, di = roundings(op, case.is128)
        r, deferred = r + ri, deferred or di
    return 2 ** 0.5 * gamma(r + (2 if deferred else 0), case.is128)


#: float additions a term of a complex64 reduction passes through before the promotion to double (tools/gen_wave_asm.py):
#: grad_code: 16 register groups x 2 v_pk_fma_f32 into one accumulator per lane (32), the reduce-scatter over the four lane
#: bits of a row (4), ds_add_f32 of 4 lanes per component and tile into the LDS accumulator, which the workgroup's 4 waves
#: share over up to 2 tiles each (32); three roundings of |f|^2 (two to form it, one to apply it).  The reduced variants
#: add less.  expz_code: 64 v_pk_fma_f32 per lane, 3 to combine the four partial sums, 64 lanes x 4 waves x 2 tiles
#: ds_add_f32 into one word, the same three for |f|^2.
M_GRAD = 32 + 4 + 32 + 3
M_EXPZ = 64 + 3 + 512 + 3
TAU_SUM = 1e-12          # complex128: double accumulation from exact products' inputs, only the order differs


def tau_reduction(case, kind):
    """complex64: (m + 2) u per real sum, doubled for a component formed from a complex entry (test_grid_paths_gpu,
    test_gate_grad_multi_tile_loop); both precisions: plus twice the amplitude bound of the records in front (the sums are
    bilinear in amplitudes that already carry it)."""
    carried = 2 * tau_amplitudes(case)
    if case.is128:
        return TAU_SUM + carried
    u = U[False]
    return (2 * (M_GRAD + 2) * u if kind == 'grad' else (M_EXPZ + 2) * u) + carried
