"""The case table of test_entangle_paths_gpu.py: one row per path of the one-wire entanglement kernels (dq_entangle.hip:
``rdm1_pass_kernel`` in four instantiations with ``rdm1_finish_kernel``, ``wire_sum_pass_kernel`` in two) at the smallest
shape that reaches it, with what the row claims about the plan.  test_entangle_paths_cpu.py asserts every claim from the
mirror (_launch_geometry.entangle_launch), which it holds against the built library; the GPU test asserts it again
before it runs the row.

A PATH is a predicate over the mirror (``PATHS``); ``APPLIES`` names the instantiations a path must have a row for.

The criteria.  Exact: amplitudes (and wire-sum operators) with integer parts in -2 .. 2, ``torch.equal`` -- every
float32 intermediate of the kernels is then an integer float32 holds (a tile's at most 8 pair products sum to at most 64;
a wire-sum output is at most 16 n), every double one is below 2^53.  Rounding: Gaussian normalised states; rdm1 wire by
wire |got - ref| <= tau S (TAU_SUM in complex128; complex64 TAU_RDM1_C64, the figure test_grid_paths_gpu.py derives for
its third-pass case), wire_sum by TAU_AMP of max |ref| per sample."""

from __future__ import annotations

from dataclasses import dataclass, field

import _launch_geometry as G
from _handler_cases import TAU_SUM                                           # noqa: F401  (1e-12: sums in double)

#: complex64: a tile's (at most 8) pair products along one bit are summed in float before the double accumulation
#: (dq_entangle.hip, file header) -- about (8 + 2) u S per component, u = 2^-24; doubled for a complex entry
TAU_RDM1_C64 = 2 * (8 + 2) * 2.0**-24

MAX_BATCH = 32768            # backend.MAX_BATCH: the samples of one launch (the library takes up to 65535, grid.y)

INSTANTIATIONS = {
    'rdm1-c64-same': dict(kernel='rdm1', c128=False, cross=False),
    'rdm1-c64-cross': dict(kernel='rdm1', c128=False, cross=True),
    'rdm1-c128-same': dict(kernel='rdm1', c128=True, cross=False),
    'rdm1-c128-cross': dict(kernel='rdm1', c128=True, cross=True),          # the 11-bit tile
    'wire_sum-c64': dict(kernel='wire_sum', c128=False, cross=False),
    'wire_sum-c128': dict(kernel='wire_sum', c128=True, cross=False),
}


@dataclass(frozen=True)
class Case:
    path: str
    inst: str
    n: int
    batch: int
    claims: dict = field(hash=False, compare=False)     # entries of the mirror this row stands for (lists: one per pass)

    @property
    def name(self):
        return f'{self.path}-{self.inst}-n{self.n}-b{self.batch}'

    @property
    def kernel(self):
        return INSTANTIATIONS[self.inst]['kernel']

    @property
    def c128(self):
        return INSTANTIATIONS[self.inst]['c128']

    @property
    def cross(self):
        return INSTANTIATIONS[self.inst]['cross']

    @property
    def seed(self):
        """Of the exact inputs: a function of the shape alone, so that rows of one shape share their states."""
        return 1 + 1009 * self.n + self.batch


def slices(batch: int) -> list[tuple[int, int]]:
    """backend.rdm1_cross / backend.apply_wire_sum: the launches of one call, MAX_BATCH samples at a time."""
    return [(lo, min(lo + MAX_BATCH, batch)) for lo in range(0, batch, MAX_BATCH)]


def launch(case: Case) -> dict:
    """The mirror of the row's first (largest) launch."""
    return G.entangle_launch(case.n, min(case.batch, MAX_BATCH), case.c128, case.cross)


def _vias(p):
    return {via for _, _, via in p['settles']}


def _gathered(plan, count):
    """``count`` passes, all but the first gathered, one tile per workgroup (the tile-loop paths have rows of their own)."""
    ps = plan['passes']
    return (len(ps) == count and not ps[0]['gathered'] and all(p['gathered'] and not p['first'] for p in ps[1:])
            and all(p['iterations'] == 1 and p['nwg'] == p['ntiles'] for p in ps))


#: path -> predicate(case, mirror of its launch)
PATHS = {
    # the tile is smaller than the 256 threads: threads past it hold zeros and pair with zeros
    'pad-sub-workgroup': lambda c, g: g['pad'] == 'sub_workgroup' and len(g['passes']) == 1 and (1 << g['m0']) < 256,
    # some of a thread's register slots lie past the tile
    'pad-sub-tile': lambda c, g: g['pad'] == 'sub_tile' and len(g['passes']) == 1 and 256 <= (1 << g['m0']) < (1 << g['M']),
    # one pass over one whole tile: no per-tile sums
    'one-full-tile': lambda c, g: g['pad'] is None and len(g['passes']) == 1 and g['passes'][0]['ntiles'] == 1
    and 'tile_sums' not in g['diag'],
    # one gathered pass of one bit, a register bit; the diagonal of that wire from the sums of two tiles; tile_base with an
    # outer bit below the gathered range
    'gather-one-bit': lambda c, g: _gathered(g, 2) and g['passes'][1]['gathered'] == 1 and g['passes'][1]['s'] == g['M'] - 1
    and _vias(g['passes'][1]) == {'reg'} and g['passes'][0]['ntiles'] == 2 and g['diag'].count('tile_sums') == 1
    and g['passes'][1]['lo'] - g['passes'][1]['s'] > 0,
    # every register bit gathered, none through LDS
    'gather-register-bits': lambda c, g: _gathered(g, 2) and g['passes'][1]['gathered'] == g['M'] - 8 and g['passes'][1]['s'] == 8
    and _vias(g['passes'][1]) == {'reg'} and [j for _, j, _ in g['passes'][1]['settles']] == list(range(8, g['M'])),
    # the widest gather: s at its minimum, LDS-partner pairs inside a gathered pass
    'gather-max-width': lambda c, g: _gathered(g, 2) and g['passes'][1]['gathered'] == g['gmax']
    and g['passes'][1]['s'] == g['M'] - g['gmax'] == (3 if c.c128 else 4) and _vias(g['passes'][1]) == {'lds', 'reg'},
    # three passes, the last one bit at lo = M + gmax; both strided loops of rdm1_finish_kernel take a second stride
    'second-gathered-pass': lambda c, g: _gathered(g, 3) and g['passes'][2]['gathered'] == 1
    and g['passes'][2]['lo'] == g['M'] + g['gmax'] and g['passes'][1]['gathered'] == g['gmax']
    and g['finish'] == dict(rows=True, tile_sums=True) and all(p['nwg'] == p['ntiles'] > 256 for p in g['passes']),
    # the tile loop with workgroups of different tile counts
    'tile-loop-ragged': lambda c, g: all(p['ragged'] and p['nwg'] == 3 and p['iterations'] >= 2 for p in g['passes'])
    and len(g['passes']) == 2,
    # one workgroup per sample walks every tile
    'one-workgroup-all-tiles': lambda c, g: all(p['nwg'] == 1 and p['iterations'] == p['ntiles'] > 1 for p in g['passes'])
    and len(g['passes']) == 2,
    # backend's loop over MAX_BATCH: two full slices and a last one of two samples, more samples than one grid holds
    'batch-slices': lambda c, g: c.batch > 65535 and [hi - lo for lo, hi in slices(c.batch)] == [MAX_BATCH, MAX_BATCH, 2],
}

ALL = tuple(INSTANTIATIONS)
#: the instantiations every path needs a row for
APPLIES = {path: ALL for path in PATHS}
APPLIES['one-workgroup-all-tiles'] = ('rdm1-c64-same', 'wire_sum-c64', 'rdm1-c128-cross')


def _rows():
    rows = []
    for inst, d in INSTANTIATIONS.items():
        plan = G.entangle_passes(1, d['c128'], d['cross'])
        m, gmax = plan['M'], plan['gmax']
        smin = m - gmax

        def add(path, n, batch, **claims):
            rows.append(Case(path, inst, n, batch, claims))

        for n in (1, 5):
            add('pad-sub-workgroup', n, 3, m=[n], s=[n], ntiles=[1], nwg=[1])
        for n in (9, m - 1):
            add('pad-sub-tile', n, 3, m=[n], s=[n], ntiles=[1], nwg=[1])
        add('one-full-tile', m, 3, m=[m], s=[m], gathered=[0], ntiles=[1], nwg=[1])
        add('gather-one-bit', m + 1, 3, m=[m, m], s=[m, m - 1], lo=[m, m], jlo=[0, m - 1], gathered=[0, 1], ntiles=[2, 2], nwg=[2, 2])
        add('gather-register-bits', 2 * m - 8, 2, s=[m, 8], lo=[m, m], jlo=[0, 8], gathered=[0, m - 8],
            ntiles=[1 << (m - 8)] * 2, nwg=[1 << (m - 8)] * 2)
        add('gather-max-width', m + gmax, 1, s=[m, smin], lo=[m, m], jlo=[0, smin], gathered=[0, gmax],
            ntiles=[1 << gmax] * 2, nwg=[1 << gmax] * 2, iterations=[1, 1])
        add('second-gathered-pass', m + gmax + 1, 1, s=[m, smin, m - 1], lo=[m, m, m + gmax], jlo=[0, smin, m - 1],
            gathered=[0, gmax, 1], ntiles=[2 << gmax] * 3, nwg=[2 << gmax] * 3, iterations=[1, 1, 1])
        if m == 12:
            add('tile-loop-ragged', 14, 700, ntiles=[4, 4], nwg=[3, 3], iterations=[2, 2], tiles_per_wg=[[2, 1, 1]] * 2,
                last_tile_wg0=[3, 3], gathered=[0, 2])
        else:
            add('tile-loop-ragged', 14, 700, ntiles=[8, 8], nwg=[3, 3], iterations=[3, 3], tiles_per_wg=[[3, 3, 2]] * 2,
                last_tile_wg0=[6, 6], gathered=[0, 3])
        if inst in APPLIES['one-workgroup-all-tiles']:
            add('one-workgroup-all-tiles', m + 1, 2048, ntiles=[2, 2], nwg=[1, 1], iterations=[2, 2], last_tile_wg0=[1, 1],
                gathered=[0, 1])
        add('batch-slices', 2, 65538, m=[2], ntiles=[1], nwg=[1])
    return rows


CASES = _rows()

#: the shapes the issue lists, spelled out: (path, instantiation) -> (n, batch) -- asserted against CASES on the CPU
LISTED = {
    ('gather-register-bits', 'rdm1-c64-same'): (16, 2), ('gather-register-bits', 'rdm1-c128-cross'): (14, 2),
    ('gather-max-width', 'rdm1-c64-same'): (20, 1), ('gather-max-width', 'rdm1-c64-cross'): (20, 1),
    ('gather-max-width', 'wire_sum-c64'): (20, 1), ('gather-max-width', 'rdm1-c128-same'): (21, 1),
    ('gather-max-width', 'wire_sum-c128'): (21, 1), ('gather-max-width', 'rdm1-c128-cross'): (19, 1),
    ('second-gathered-pass', 'rdm1-c64-same'): (21, 1), ('second-gathered-pass', 'rdm1-c64-cross'): (21, 1),
    ('second-gathered-pass', 'wire_sum-c64'): (21, 1), ('second-gathered-pass', 'rdm1-c128-same'): (22, 1),
    ('second-gathered-pass', 'wire_sum-c128'): (22, 1), ('second-gathered-pass', 'rdm1-c128-cross'): (20, 1),
    ('one-full-tile', 'rdm1-c128-cross'): (11, 3), ('one-full-tile', 'rdm1-c128-same'): (12, 3),
    ('gather-one-bit', 'rdm1-c128-cross'): (12, 3), ('gather-one-bit', 'wire_sum-c128'): (13, 3),
    ('pad-sub-tile', 'rdm1-c128-cross'): (10, 3), ('pad-sub-tile', 'rdm1-c64-cross'): (11, 3),
    ('tile-loop-ragged', 'rdm1-c128-cross'): (14, 700), ('tile-loop-ragged', 'wire_sum-c64'): (14, 700),
    ('one-workgroup-all-tiles', 'rdm1-c64-same'): (13, 2048), ('one-workgroup-all-tiles', 'wire_sum-c64'): (13, 2048),
    ('one-workgroup-all-tiles', 'rdm1-c128-cross'): (12, 2048),
    ('batch-slices', 'rdm1-c64-same'): (2, 65538), ('batch-slices', 'wire_sum-c128'): (2, 65538),
}


def passes_of_control(case: Case, plan: dict) -> list[tuple[int, int, int]]:
    """The rdm1 negative control: per pass, (pass, tile, its index bits) of the tile that workgroup 0 takes in its last
    iteration."""
    return [(i, p['last_tile_wg0'], G.ent_tile_base(p, p['last_tile_wg0'])) for i, p in enumerate(plan['passes'])]
