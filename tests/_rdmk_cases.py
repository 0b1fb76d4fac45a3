"""The case table of test_rdmk_paths_gpu.py: one row per path of ``dq_rdmk_cross_*`` (dq_rdm.hip), at the smallest shape
that reaches it, with what the row claims about the plan.  test_rdmk_paths_cpu.py asserts every claim from the mirror
(_launch_geometry.rdmk), which it holds against the built library; the GPU test asserts it again before it runs the row.

Targets are scattered and unsorted (matrix MSB = targets[0]); targets and controls hold index bit 0 or bit n - 1 (mostly
both), and some of them sit among the rest bits above the chunk, so that the chunk walk and the deposit of a split's
first chunk run over a mask with holes (``has_holes``, asserted for every row).

The criteria.  Exact: integer amplitudes, ``torch.equal``.  Rounding: |got - ref| <= tau * S elementwise, S the same sum
over |gy| |x|.  complex128: TAU_SUM, the figure of test_grid_paths_gpu.py for sums in double.  complex64: TAU_C64, derived
from the accumulation DESIGN 4.6 documents and not from the kernel: _grid_refs.f32_chain adds float32 products in k order
over windows of 4096 contraction indices and the windows in float64.  On the rows' own inputs (first sample, two diagonal
and two off-diagonal elements) its worst ratio to S is 9.1e-7, on a diagonal element of a Hermitian row, where every
term is positive (2.6e-7 .. 4.3e-7 at K = 2^20 .. 2^23, 5.3e-7 .. 9.1e-7 at K = 2^14, where four windows average less; 9e-9
and less where x and gy are independent and the terms cancel).  DESIGN 4.6 used to quote 3.5e-7 for one such chain.  The
kernel's order inside an MFMA and across its four waves is not the emulation's, hence a margin of 8: 8 * 9.1e-7 = 7.3e-6,
rounded up to one digit.  The same chain never flushed is at 2.8e-2 of S at K = 2^23 (3.7e-3 at K = 2^21)."""

from __future__ import annotations

from dataclasses import dataclass, field


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    targets: tuple
    controls: tuple
    batch: int
    herm: bool                 # x is gy: the Hermitian route (upper-triangle tiles, mirrored by the finish kernel)
    c128: bool
    claims: dict = field(hash=False, compare=False)     # entries of _launch_geometry.rdmk this row stands for
    big: bool = False          # takes its states from the module's shared 8-GiB inputs
    rounding: bool = True      # also run with random normalised states (complex128 only where K <= 2^16)

    @property
    def k(self):
        return len(self.targets)

    @property
    def nc(self):
        return len(self.controls)


def _c(name, n, targets, controls, batch, herm, c128, claims, **kw):
    return Case(name, n, tuple(targets), tuple(controls), batch, herm, c128, claims, **kw)


SMALL_FLUSH = dict(flush_then_more=True, flushes=2, nch=512, ntl=1)
CASES = [
    # 16 x 16 tile: rows padded (k = 3), the f32 flush followed by 256 more chunks, four waves added through LDS
    _c('t16-k3-herm', 26, [25, 0, 13], [], 8, True, False, dict(tile=16, pad_rows=True, nsplit=256, **SMALL_FLUSH), big=True),
    _c('t16-k4-herm', 26, [24, 0, 25, 16], [], 16, True, False, dict(tile=16, pad_rows=False, nsplit=128, **SMALL_FLUSH),
       big=True),
    _c('t16-k4-cross', 26, [3, 0, 25, 9], [], 16, False, False, dict(tile=16, nsplit=128, **SMALL_FLUSH), big=True),
    # 32 x 32 tile
    _c('t32-k5-cross', 26, [25, 2, 23, 11, 21], [], 16, False, False, dict(tile=32, nsplit=128, **SMALL_FLUSH), big=True),
    _c('t32-k5-herm', 26, [0, 14, 5, 25, 8], [], 16, True, False, dict(tile=32, nsplit=128, **SMALL_FLUSH), big=True),
    # one control, on index bit 0 and on the top bit: 256 chunks, the flush falls on the last chunk and the one after the
    # loop adds an empty accumulator
    _c('t16-k4-ctl0-cross', 26, [12, 25, 4, 1], [0], 16, False, False,
       dict(tile=16, nsplit=128, nch=256, flushes=1, flush_then_more=False), big=True),
    _c('t16-k4-ctltop-herm', 26, [22, 0, 24, 10], [25], 16, True, False,
       dict(tile=16, nsplit=128, nch=256, flushes=1, flush_then_more=False), big=True),
    _c('t32-k5-ctl0-herm', 26, [25, 6, 17, 3, 9], [0], 16, True, False,
       dict(tile=32, nsplit=128, nch=256, flushes=1, flush_then_more=False), big=True),
    _c('t32-k5-ctltop-cross', 26, [1, 24, 0, 15, 20], [25], 16, False, False,
       dict(tile=32, nsplit=128, nch=256, flushes=1, flush_then_more=False), big=True),
    # 64 x 64 tiles: splits x tiles x batch in the workspace.  Hermitian: upper triangle, mirror, diagonal tiles
    _c('t64-k7-herm', 21, [20, 3, 11, 0, 17, 8, 14], [], 2, True, False,
       dict(tile=64, nsplit=2, ntl=3, nt=2, nch=512, flush_then_more=True)),
    _c('t64-k8-herm', 22, [5, 21, 0, 19, 9, 13, 2, 16], [], 2, True, False,
       dict(tile=64, nsplit=2, ntl=10, nt=4, nch=512, flush_then_more=True)),
    _c('t64-k10-herm', 24, [23, 1, 12, 0, 20, 7, 15, 4, 18, 10], [], 2, True, False,
       dict(tile=64, nsplit=2, ntl=136, nt=16, nch=512, flush_then_more=True)),
    # cross: every tile, row-major
    _c('t64-k8-cross', 24, [0, 23, 6, 21, 11, 3, 17, 14], [], 2, False, False,
       dict(tile=64, nsplit=2, ntl=16, nt=4, nch=2048, flushes=8, flush_then_more=True)),
    _c('t64-k8-cross-c128', 23, [22, 4, 0, 18, 9, 13, 2, 20], [], 2, False, True,
       dict(tile=64, nsplit=2, ntl=16, nch=1024, flushes=0)),
    _c('t64-k10-herm-c128', 23, [3, 22, 0, 16, 8, 19, 11, 5, 21, 13], [], 2, True, True,
       dict(tile=64, nsplit=2, ntl=136, nch=256)),
    # many splits of one tile, complex128 (K = 2^16, 2^15)
    _c('t64-k6-splits-c128', 22, [21, 0, 9, 15, 4, 18], [], 2, True, True, dict(tile=64, nsplit=8, ntl=1, nch=512)),
    _c('t32-k5-splits-c128', 20, [7, 19, 0, 12, 16], [], 2, False, True, dict(tile=32, nsplit=8, ntl=1, nch=128)),
    # complex128 at large K: the exact criterion only (a complex128 sum of 2^22 terms rounds too close to 1e-12)
    _c('t16-k3-c128-exact', 25, [0, 24, 11], [], 4, False, True, dict(tile=16, pad_rows=True, terms=1 << 22, nsplit=512, nch=128),
       rounding=False),
    _c('t32-k5-c128-exact', 25, [24, 8, 22, 0, 19], [23], 4, True, True, dict(tile=32, terms=1 << 19, nsplit=256, nch=64),
       rounding=False),
]

TAU_SUM = 1e-12
TAU_C64 = 8e-6
FLUSH_WINDOW = 4096        # contraction indices an f32 accumulator takes before it is added into double

#: the complex64 row with the longest contraction: it carries the condition that an f32 chain never flushed is rejected
LARGEST_K = max((c for c in CASES if c.rounding and not c.c128), key=lambda c: c.n - c.k - c.nc)

#: how the two shared inputs of the ``big`` rows are shaped: (16, 2^26) complex64, 8 GiB each
BIG_N, BIG_BATCH = 26, 16


def rest_hi(case: Case, chunk_bits: int) -> list[int]:
    """The rest bits above the chunk (dq_rdm.hip: RdmGeom.rest_hi), ascending."""
    rest = [p for p in range(case.n) if p not in case.targets and p not in case.controls]
    return rest[chunk_bits:]


def has_holes(case: Case, chunk_bits: int) -> bool:
    """A target or control lies between two rest bits above the chunk."""
    hi = rest_hi(case, chunk_bits)
    return bool(hi) and hi != list(range(hi[0], hi[0] + len(hi)))
