"""Which handler bodies of the wave-tile kernel a pass runs -- TEST INFRASTRUCTURE ONLY, no GPU.

The kernel (csrc/dq_wave.hip) jumps on word 0 of every 32-byte record to one generated body.  This module decodes the
records the library itself derives from a ``DqFusedPass`` (``dq_wave_descriptor`` through ``_wave_emulator.descriptor``;
``dq_wave_records`` for passes whose records live in device memory) into handler ids, names them from the generators'
own constants (``ID_*``, ``TRIP_MASKS``, ``SWAP_PAIRS``, ``GRAD_VARIANTS``: nothing is typed in here, so a precision
without a family simply has no such names) and lists, per record, the words that select a path INSIDE its body -- the
record's *features*, read exactly as ``_wave_emulator.run_pass`` reads them."""

from __future__ import annotations

import ctypes as C
from collections import namedtuple

import _wave_emulator as emu
from deepquantum_amd import _lib

Record = namedtuple('Record', 'hid family words features')

MOVES = ('X_U', 'X_C', 'X_R', 'X_R1', 'TRIP0', 'TRIP', 'SWAP')          # families that only move amplitudes


def families(is128):
    """[(name, first id, one past the last id)] in id order, from the generator's ID_* constants."""
    g = emu.gen(is128)
    starts = sorted((getattr(g, k), k[3:]) for k in dir(g) if k.startswith('ID_') and isinstance(getattr(g, k), int) and getattr(g, k) >= 0)
    return [(nm, lo, (starts[i + 1][0] if i + 1 < len(starts) else g.NIDS)) for i, (lo, nm) in enumerate(starts)]


def family(hid, is128):
    for nm, lo, hi in families(is128):
        if lo <= hid < hi:
            return nm, hid - lo
    raise ValueError(f'handler id {hid} outside range(NIDS)')


def name(hid, is128):
    g = emu.gen(is128)
    fam, off = family(hid, is128)
    R = g.R
    if fam == 'GEN_U':
        return f'GEN_U mode={off // R} slot={off % R}'
    if fam in ('GEN_C', 'GEN_R', 'X_U', 'X_C', 'X_R'):
        return f'{fam} slot={off}'
    if fam == 'X_R1':
        q, cc = divmod(off, R - 1)
        return f'X_R1 q={q} c={cc if cc < q else cc + 1}'
    if fam == 'TRIP':
        return f'TRIP mask={g.TRIP_MASKS[off]:0{R}b}'
    if fam == 'SWAP':
        return 'SWAP pair=(%d,%d)' % g.SWAP_PAIRS[off]
    if fam in ('DIAG1', 'DIAG2'):
        masked, v = divmod(off, R + 1)
        return f'{fam} {"all" if v == 0 else f"slot={v - 1}"}{" masked" if masked else ""}'
    if fam == 'GRAD':
        variant, q = divmod(off, R - 1)
        return f'GRAD variant={variant} slot={q + 1}'
    if fam.startswith('GEN2'):
        a, b = g.SWAP_PAIRS[off]
        return f'{fam} pair=({a},{b})'
    return fam          # TRIP0, EXPZ


def features(hid, w, is128):
    """The path selectors of a record beside its id (see the module docstring)."""
    g = emu.gen(is128)
    fam, off = family(hid, is128)
    f = set()
    if fam in ('TRIP0', 'TRIP', 'SWAP'):
        return frozenset()
    if fam == 'EXPZ':
        regs = w[5] | w[7]
        f.add('reg_signs' if regs else 'no_reg_signs')
        f.add('lane_parity' if w[1] else 'no_lane_parity')
        f.add('tile_parity' if (w[2] | w[3]) else 'no_tile_parity')
        if regs and w[1] and (w[2] | w[3]):
            f.add('all_three')
        return frozenset(f)
    f.add('lane_ctl' if w[1] else 'no_lane_ctl')
    f.add('out_ctl' if (w[2] | w[3]) else 'no_out_ctl')
    if fam in ('GEN_R', 'X_R'):
        f.add('partial_mask' if w[5] != (1 << (g.NA // 2)) - 1 else 'full_mask')
    if fam.startswith('GEN2') or fam == 'GRAD':
        f.add('partial_mask' if w[5] != (1 << (g.NA // 4)) - 1 else 'full_mask')
    if fam.startswith('GEN2'):
        f.add(f'w6={int(bool(w[6]))}')
    if fam in ('DIAG1', 'DIAG2'):
        kinds = {0: 'none', 1: 'lane', 2: 'tile'}
        f.add('selA=' + kinds[(w[5] >> 6) & 3])
        f.add('selB=' + kinds[(w[5] >> 14) & 3])
        f.add('masked' if off >= g.R + 1 else 'unmasked')
    return frozenset(f)


def _decode(words, is128):
    g = emu.gen(is128)
    out, i = [], 0
    while i < len(words):
        w = tuple(words[i])
        i += 1
        fam, _ = family(w[0], is128)
        out.append(Record(w[0], fam, w, features(w[0], w, is128)))
        if g.ID_TRIP0 <= w[0] < g.ID_SWAP:          # a trip is two records: the second holds the LDS addresses
            i += 1
    return out


def ids(desc, n, is128, known_zero=0):
    """The records of a pass as [Record], in execution order."""
    kp = emu.descriptor(desc, n, known_zero)
    return _decode([list(kp.rec[i]) for i in range(kp.nrec_bytes // 32)], is128)


def ids_ext(desc, n, is128):
    """The same through ``dq_wave_records`` (passes with more records than the kernel arguments hold)."""
    lib = _lib.load()
    nb = lib.dq_wave_records(C.byref(desc), n, None, 0)
    if nb <= 0:
        raise RuntimeError(lib.dq_last_error().decode())
    buf = (C.c_uint32 * (nb // 4))()
    assert lib.dq_wave_records(C.byref(desc), n, buf, nb) == nb
    return _decode([list(buf[8 * i:8 * i + 8]) for i in range(nb // 32)], is128)


def zext_word(desc, n, known_zero):
    """(log2 tiles, dead register slots, dead lane bits) of a zero-extended launch (WaveKernPass::zext)."""
    z = emu.descriptor(desc, n, known_zero).zext
    return z & 63, (z >> 8) & 63, (z >> 16) & 63
