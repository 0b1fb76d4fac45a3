"""Mirrors of the launchers' grid arithmetic, for the large-grid tests (test_grid_paths_gpu.py) and the path-by-path tests
(test_pass_paths_*.py, test_rdmk_paths_*.py, test_gate_paths_*.py, test_reduce_paths_*.py, test_entangle_paths_*.py).

Each function copies what one launcher in ``deepquantum_amd/csrc`` (or ``backend.py``) computes from a shape: how many
workgroups it launches and so how many times a workgroup goes round its loop, whether the streaming (non-temporal)
instantiation is picked, how many passes a plan has.  A GPU case asserts from these that its shape reaches the path it
claims; test_grid_paths_cpu.py checks the mirrors against the thresholds they stand for and, where the library reports
the arithmetic itself (``dq_rdm1_ws_bytes``), against the library.  If a constant in a launcher changes, the mirror here
must change with it, or the cases stop claiming what they cover -- loudly."""

from __future__ import annotations

GIB = 1 << 30


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _csize(c128: bool) -> int:
    return 16 if c128 else 8


# ---- dq_dense.hip, apply_dense_mfma (k = 5..10 on the matrix cores) -----------------------------------------------------
def dense(n: int, k: int, nc: int, batch: int, c128: bool, shared: bool, bit0_used: bool, *, dense_nt: int | None = None,
          dense5: int = 1, dense5_blocks: int = 0, dense_big: int = 0, dense_rows_fast: int = 1, launch: bool = False) -> dict:
    """dq_dense.hip:380-435.  ``bit0_used``: index bit 0 is a target or a control.  Returns the route ('dense56', 'staged1'
    = apply_dense_mfma_kernel<T, 1>, 'staged2' = <T, 2>, 'big128' = <T, 2, NT, 4, 4>), whether the non-temporal
    instantiation runs, and for dense56 the column groups, the groups one pass of the grid covers and the loop iterations
    of a workgroup.

    The keywords stand for the process-wide knobs DQ_DENSE_NT (None: unset), DQ_DENSE5, DQ_DENSE5_BLOCKS, DQ_DENSE_BIG and
    DQ_DENSE_ROWS_FAST as the launcher parses them (atoi), at their defaults unless given.  With ``launch`` (or any knob
    off its default) the dict also holds the launch itself: ``grid`` (x, y, z), ``rows_fast`` (bit 30 of the shift word:
    row tiles vary fastest), ``ncols``, ``col_shift`` (-1: per-sample matrices) and ``row_tile`` / ``col_tile`` (rows of U
    and columns a workgroup -- dense56: a wave -- owns at a time)."""
    d = 1 << k
    colbits = n - k - nc
    ncols = (batch if shared else 1) << colbits
    shift = colbits if shared else -1                                         # dq_dense.hip:390
    gz = 1 if shared else batch
    nt = dense_nt != 0 if dense_nt is not None and dense_nt >= 0 else (batch << n) * _csize(c128) >= GIB      # dq_dense.hip:393-394
    more = launch or (dense_nt, dense5, dense5_blocks, dense_big, dense_rows_fast) != (None, 1, 0, 0, 1)
    cpl = 1 if c128 else 2
    cg = 16 * cpl
    if (d == 32 or (d == 64 and not c128)) and dense5 and ncols % cg == 0 and (c128 or not bit0_used):     # dq_dense.hip:399
        ngroups = ncols // cg
        resident = 256 * (3 if (not c128 and d == 32) else 2)               # dq_dense.hip:403
        per_wg = 4 if d == 32 else 2
        blocks = min(_cdiv(ngroups, per_wg), dense5_blocks if dense5_blocks > 0 else resident)      # dq_dense.hip:405
        per_pass = blocks * per_wg
        out = dict(route='dense56', nt=nt, ngroups=ngroups, col_group=cg, per_pass=per_pass,
                   iterations=_cdiv(ngroups, per_pass))
        extra = dict(grid=(blocks, gz, 1), rows_fast=False, row_tile=32, col_tile=cg)
    elif d == 32:                                                             # dq_dense.hip:414
        out = dict(route='staged1', nt=nt, iterations=1)
        extra = dict(grid=(_cdiv(ncols, 128), 1, gz), rows_fast=False, row_tile=32, col_tile=128)
    elif not c128 and d >= 256 and dense_big and ncols % 128 == 0:            # dq_dense.hip:421
        out = dict(route='big128', nt=nt, iterations=1)
        extra = dict(grid=(ncols // 128, d // 128, gz), rows_fast=shared, row_tile=128, col_tile=128)
    else:
        out = dict(route='staged2', nt=nt, iterations=1)
        extra = dict(grid=(_cdiv(ncols, 64), d // 64, gz), rows_fast=bool(dense_rows_fast) and shared,      # dq_dense.hip:430-432
                     row_tile=64, col_tile=64)
    if more:
        out.update(extra, ncols=ncols, col_shift=shift)
    return out


# ---- dq_gate.hip, apply_small_kernel (k <= 4) -----------------------------------------------------------------------------
def small_gate(n: int, k: int, nc: int, c128: bool, bit0_used: bool, in_place: bool) -> dict:
    """dq_gate.hip:187-226.  ``wide``: the complex64 instantiation that takes the two groups differing in index bit 0 per
    thread (k <= 3, bit 0 neither target nor control, at least one free bit); ``groups``: what the grid is sized for --
    pairs of groups when wide; ``blocks`` workgroups of 256 per sample and the ``iterations`` of their grid-stride loop;
    ``copy``: copy_uncontrolled_kernel runs first (out of place with controls)."""
    assert 1 <= k <= 4
    na = k + nc
    groups = 1 << (n - na)                                                    # dq_gate.hip:194
    wide = not c128 and k <= 3 and na < 16 and n - na >= 1 and not bit0_used   # dq_gate.hip:198
    if wide:
        groups >>= 1
    blocks = min(_cdiv(groups, 256), 1 << 20)                                 # dq_gate.hip:206-207
    return dict(wide=wide, groups=groups, blocks=blocks, iterations=_cdiv(groups, blocks * 256),
                copy=not in_place and nc > 0)                                 # dq_gate.hip:188


# ---- dq_gate.hip, copy_uncontrolled_kernel (controlled gates out of place) ----------------------------------------------
def copy_uncontrolled(n: int, batch: int) -> dict:
    """dq_gate.hip:190 / :237: one grid over all batch * 2^n amplitudes, at most 65536 workgroups of 256."""
    total = batch << n
    blocks = min(_cdiv(total, 256), 65536)
    return dict(blocks=blocks, iterations=_cdiv(total, blocks * 256))


# ---- dq_reduce.hip ------------------------------------------------------------------------------------------------------
RED_BLOCKS, RED_THREADS = 1024, 256                                          # dq_reduce.hip:15-16


def red_blocks(work: int) -> int:
    """dq_reduce.hip:311."""
    return max(1, min(_cdiv(work, RED_THREADS), RED_BLOCKS))


def expect_pauli(n: int, xmask: int) -> dict:
    """dq_reduce.hip:327-331: pairs of amplitudes for strings with an X or Y factor, single amplitudes otherwise."""
    work = 1 << (n - 1) if xmask else 1 << n
    nb = red_blocks(work)
    return dict(blocks=nb, items=work, iterations=_cdiv(work, nb * RED_THREADS))


def inner(count: int) -> dict:
    """dq_reduce.hip:594."""
    nb = red_blocks(count)
    return dict(blocks=nb, iterations=_cdiv(count, nb * RED_THREADS))


def scale_zsigns(n: int) -> dict:
    """dq_reduce.hip:575-577 (the matrix-core kernel, n >= 8): 1024 amplitudes per workgroup and iteration."""
    assert n >= 8
    nb = max(1, min((1 << n) >> 10, 2048))
    return dict(blocks=nb, chunk=1024, iterations=_cdiv(1 << n, nb * 1024))


def scale_zsigns_waves(n: int) -> dict:
    """dq_reduce.hip:512 (scale_zsigns_mfma_kernel): wave w of workgroup b starts at amplitude (4 b + w) << 8 and has no
    work when that lies past the state.  ``idle_waves``: (workgroup, wave) pairs that never enter the loop."""
    g = scale_zsigns(n)
    idle = [(b, w) for b in range(g['blocks']) for w in range(4) if (b * 4 + w) << 8 >= 1 << n]
    return dict(g, idle_waves=idle)


def expect_zmulti(n: int, c128: bool) -> dict:
    """backend.py:361 picks the workgroups; dq_reduce.hip (expect_zmulti_mfma_kernel) reads U slices of 256 amplitudes
    per workgroup and iteration, U = 8 (complex64) / 4 (complex128).  ``slices``: per workgroup, the slice numbers u of
    its FIRST iteration that lie inside the state (dq_reduce.hip:415-420: i0 + 256 u < 2^n; the same for its four waves,
    256 divides 2^n from n = 8 on); ``idle_blocks``: workgroups whose first slice is already past the end."""
    nb = max(1, min(2048, (1 << n) // 1024))
    u = 4 if c128 else 8
    out = dict(blocks=nb, window=u * RED_THREADS, iterations=_cdiv(1 << n, u * nb * RED_THREADS), u=u)
    if n >= 8 and nb <= 64:                                                   # (the table is for the small shapes)
        out['slices'] = [[s for s in range(u) if b * u * RED_THREADS + s * RED_THREADS < 1 << n] for b in range(nb)]
        out['idle_blocks'] = [b for b, s in enumerate(out['slices']) if not s]
    return out


def probs(count: int) -> dict:
    """dq_reduce.hip:610-611: one grid over all batch * 2^n amplitudes."""
    nb = min(_cdiv(count, 256), 65536)
    return dict(blocks=nb, iterations=_cdiv(count, nb * 256))


def marginal(n: int, bits: list[int], batch: int, c128: bool) -> dict:
    """dq_reduce.hip:634-691: the chunk's bits, and ``run``: how many bits of the chunk number a workgroup loops over
    (2^run chunks each).  ``chunk_bits``: the index bits inside a chunk; ``cpos``: the chunk number's bits, low first;
    ``low`` / ``c``: the contiguous run and the chunk's size in bits; ``nlo`` / ``nhi``: measured bits inside / outside the
    chunk; ``qmask``, ``exclusive``: as in MargGeom; ``run_bits``: unmeasured bits outside the chunk (``run`` before the cut
    of :691); ``geom``: the whole MargGeom (dq_reduce.hip:156-164) in the padded form the kernel receives."""
    vec = 1 if c128 else 2
    c = min(n, 12)
    low = min(n, 8 - vec)
    nw = len(bits)
    measured = sum(1 << b for b in bits)
    out_of = {b: nw - 1 - i for i, b in enumerate(bits)}
    cand = [b for b in range(low, n) if not (measured >> b) & 1]
    cand += [b for o in range(nw) for b in range(low, n) if (measured >> b) & 1 and out_of[b] == o]
    in_chunk = set(range(low)) | set(cand[:c - low])
    cpos, run = [], 0
    for pas in (0, 1):
        for b in range(n):
            if b not in in_chunk and ((measured >> b) & 1) == pas:
                cpos.append(b)
                run += pas == 0
    while run > 0 and (1 << (n - c - run)) * batch < 2048:                    # dq_reduce.hip:691
        run -= 1
    # the whole MargGeom as the kernel receives it (dq_reduce.hip:156-164), pads included: :642-645
    pos, local_of, nxt = [62] * 12, {}, 0
    for b in range(low):                                                      # :658-662
        pos[b], local_of[b] = b, b
    for pas in (0, 1):                                                        # :663-668: the thread-held bits 8..11 first
        for x in (range(8, c) if pas == 0 else range(low, min(c, 8))):
            pos[x], local_of[cand[nxt]] = cand[nxt], x
            nxt += 1
    assert set(local_of) == in_chunk
    lo_x, lo_out, hi_pos, hi_out, qmask = [], [], [], [], 0
    for o in range(nw):                                                       # :670-682
        b = bits[nw - 1 - o]
        if b in in_chunk:
            lo_x.append(local_of[b])
            lo_out.append(o)
            if local_of[b] >= 8:
                qmask |= 1 << (local_of[b] - 8)
        else:
            hi_pos.append(b)
            hi_out.append(o)
    nlo, nhi = len(lo_x), len(hi_pos)
    geom = dict(c=c, nlo=nlo, run=run, exclusive=int(nhi == n - c), qmask=qmask, pos=pos,       # :683
                cpos=cpos + [63] * (28 - len(cpos)), lo_x=lo_x + [31] * (12 - nlo), lo_out=lo_out + [0] * (12 - nlo),
                hi_pos=hi_pos + [63] * (40 - nhi), hi_out=hi_out + [0] * (40 - nhi))
    return dict(run=run, chunk_bits=sorted(in_chunk), cpos=cpos, blocks=1 << (n - c - run), low=low, c=c, nlo=nlo, nhi=nhi,
                qmask=qmask, exclusive=bool(geom['exclusive']), run_bits=sum(not (measured >> b) & 1 for b in cpos),
                lds_bytes=8 << nlo, geom=geom)


def gate_grad(n: int, k: int, nc: int) -> dict:
    """dq_reduce.hip:920-922: amplitude groups (2^(n-k-nc)) over at most 512 workgroups of 256."""
    groups = 1 << (n - k - nc)
    nb = min(_cdiv(groups, RED_THREADS), 512)
    return dict(blocks=nb, groups=groups, iterations=_cdiv(groups, nb * RED_THREADS))


def gate_grad_multi(n: int, c128: bool, gates) -> list[dict]:
    """backend.py:489-517 (how the gates are packed into launches and the workgroups) and dq_reduce.hip:818-859 (the
    tile's bits: the low L, the launch's targets at or above L, then the lowest free bits above L).  One dict per
    launch: its gate indices, the tile bits (ascending), the tiles and how many a workgroup visits at most, ``route``
    ('tile'; below the tile backend.py:491 goes gate by gate: one dict per gate, route 'gate_grad'), ``high_sorted`` (the
    gathered bits), ``high_targets`` (those of them that are targets), ``outside`` (the index bits that number the tiles) and
    ``desc``: tbit / cin / cout of every gate as the launcher fills GradMultiDesc."""
    tile, per_call, low = (10, 4, 3) if c128 else (11, 8, 4)
    if n < tile:                                                              # backend.py:491: gate by gate through gate_grad
        return [dict(route='gate_grad', gates=[i]) for i in range(len(gates))]
    nblocks = min(1 << (n - tile), 1536)
    out, start = [], 0
    while start < len(gates):
        stop, high = start, set()
        while stop < len(gates) and stop - start < per_call:
            t = int(gates[stop][0])
            if t >= low and t not in high and len(high) == tile - low:
                break
            if t >= low:
                high.add(t)
            stop += 1
        hb, p = set(high), low
        while len(hb) < tile - low:
            if p not in hb:
                hb.add(p)
            p += 1
        ntiles = 1 << (n - tile)
        tile_bits = sorted(set(range(low)) | hb)
        local = {p: q for q, p in enumerate(tile_bits)}                       # dq_reduce.hip:852-864
        desc = []
        for gi in range(start, stop):                                         # :865-878: tbit, cin, cout of every gate
            t, ctrl = int(gates[gi][0]), [int(q) for q in gates[gi][1]]
            desc.append(dict(tbit=local[t], cin=sum(1 << local[q] for q in ctrl if q in local),
                             cout=sum(1 << q for q in ctrl if q not in local)))
        out.append(dict(route='tile', gates=list(range(start, stop)), tile_bits=tile_bits, blocks=nblocks,
                        ntiles=ntiles, iterations=_cdiv(ntiles, nblocks), pairs_per_thread=(1 << (tile - 1)) // RED_THREADS,
                        high_sorted=sorted(hb), high_targets=sorted(high), outside=[p for p in range(n) if p not in tile_bits],
                        desc=desc))
        start = stop
    return out


# ---- dq_entangle.hip: rdm1_cross / apply_wire_sum ------------------------------------------------------------------------
ENT_ROW = 12 * 8                                                             # dq_entangle.hip:27


def ent_plan(n: int, c128: bool, cross: bool) -> list[dict]:
    """dq_entangle.hip:376-395 (ent_plan, ent_nwg) for ONE batch: the passes, their tiles and workgroups."""
    m = 11 if (c128 and cross) else 12
    m0 = min(n, m)
    gmax = m - (3 if c128 else 4)
    passes = [dict(ntiles=1 << (n - m0))]
    lo = m0
    while lo < n:
        passes.append(dict(ntiles=1 << (n - m)))
        lo += gmax
    return passes


def ent_nwg(ntiles: int, batch: int) -> int:
    return min(ntiles, max(1, _cdiv(2048, batch)))


def entangle(n: int, batch: int, c128: bool, cross: bool) -> dict:
    ps = ent_plan(n, c128, cross)
    nwg = [ent_nwg(p['ntiles'], batch) for p in ps]
    return dict(passes=len(ps), ntiles=[p['ntiles'] for p in ps], nwg=nwg,
                iterations=[_cdiv(p['ntiles'], w) for p, w in zip(ps, nwg)])


def rdm1_ws_bytes(n: int, batch: int, c128: bool, cross: bool) -> int:
    """dq_entangle.hip:397-405 (ent_ws_doubles): one row of ENT_ROW doubles per workgroup and pass, plus the tile sums of
    pass 0 when it has more than one tile."""
    ps = ent_plan(n, c128, cross)
    total = sum(batch * ent_nwg(p['ntiles'], batch) * ENT_ROW for p in ps)
    if ps[0]['ntiles'] > 1:
        total += batch * ps[0]['ntiles'] * 2
    return 8 * total


def entangle_passes(n: int, c128: bool, cross: bool) -> dict:
    """dq_entangle.hip:376-391 (ent_tile_bits, ent_plan) in full, for the path-by-path tests (_entangle_cases.py).  The
    wire-sum kernel plans with ``cross`` False: its tile is always 12 bits.

    ``M``: the LDS tile's bits (12; 11 for the complex128 cross reduction), ``m0`` = min(n, M), ``gmax`` the most bits a
    pass gathers, ``pad``: 'sub_workgroup' (n < 8: threads past the tile hold zeros), 'sub_tile' (8 <= n < M: register
    slots past the tile hold zeros) or None.  ``diag[p]``: where the diagonal of wire bit p comes from, 'tile' (p < m0)
    or 'tile_sums' (the per-tile sums of pass 0).  ``passes``: per pass m, s, lo, jlo, gathered = m - s, ntiles, first,
    and ``settles``: the (wire bit p, tile bit j, via) whose pairs it reduces / applies, via = 'lds' for j < 8 (the
    partner read from the LDS tile) and 'reg' for j >= 8 (a register pair of the thread's slots t + 256 k)."""
    m_tile = 11 if (c128 and cross) else 12                                   # dq_entangle.hip:376
    m0 = min(n, m_tile)
    gmax = m_tile - (3 if c128 else 4)                                        # :383

    def one(m, s, lo, jlo, ntiles, first):                                    # (EntPass, :32-41; jmask = tile bits jlo .. m - 1)
        settles = [(j if j < s else lo + (j - s), j, 'lds' if j < 8 else 'reg') for j in range(jlo, m)]      # :448-449
        return dict(m=m, s=s, lo=lo, jlo=jlo, gathered=m - s, ntiles=ntiles, first=first, settles=settles)

    passes = [one(m0, m0, m0, 0, 1 << (n - m0), True)]                        # :385
    lo = m0
    while lo < n:                                                             # :386-389
        gb = min(n - lo, gmax)
        passes.append(one(m_tile, m_tile - gb, lo, m_tile - gb, 1 << (n - m_tile), False))
        lo += gmax
    return dict(M=m_tile, m0=m0, gmax=gmax, pad='sub_workgroup' if n < 8 else ('sub_tile' if n < m_tile else None),
                diag=['tile' if p < m0 else 'tile_sums' for p in range(n)], passes=passes)


def entangle_launch(n: int, batch: int, c128: bool, cross: bool) -> dict:
    """entangle_passes with ent_nwg (dq_entangle.hip:393-397) for ONE launch of ``batch`` <= 65535 samples.  Every pass
    gains ``nwg`` (workgroups per sample), ``iterations`` (of the busiest workgroup's tile loop, :104 / :319), ``ragged``
    (workgroups with different tile counts), ``tiles_per_wg`` and ``last_tile_wg0`` (the tile workgroup 0 takes in its
    last iteration).  ``finish``: whether the two strided loops of rdm1_finish_kernel (256 threads) take a second
    stride: ``rows`` (:268, over the workgroup rows of some pass: nwg > 256) and ``tile_sums`` (:275, ntiles0 > 256)."""
    plan = entangle_passes(n, c128, cross)
    for p in plan['passes']:
        nwg = ent_nwg(p['ntiles'], batch)
        per = [len(range(w, p['ntiles'], nwg)) for w in range(nwg)] if nwg <= 4096 else None
        p.update(nwg=nwg, iterations=_cdiv(p['ntiles'], nwg), ragged=p['ntiles'] % nwg != 0, tiles_per_wg=per,
                 last_tile_wg0=((p['ntiles'] - 1) // nwg) * nwg)
    nt0 = plan['passes'][0]['ntiles']
    plan['finish'] = dict(rows=any(p['nwg'] > 256 for p in plan['passes']), tile_sums=nt0 > 1 and nt0 > 256)
    return plan


def ent_tile_base(p: dict, o: int) -> int:
    """dq_entangle.hip:43-47 (tile_base): the index bits of tile number ``o`` of pass ``p`` -- its low lo - s bits sit
    between the contiguous part and the gathered range, the rest above the gathered range."""
    mid = p['lo'] - p['s']
    return ((o & ((1 << mid) - 1)) << p['s']) | ((o >> mid) << (p['lo'] + p['gathered']))


def ent_tile_index(p: dict, base: int, l: int) -> int:                        # noqa: E741
    """dq_entangle.hip:49-51 (tile_index): the amplitude index of tile-local index ``l``."""
    return base | (l & ((1 << p['s']) - 1)) | ((l >> p['s']) << p['lo'])


# ---- dq_rdm.hip: rdmk_cross (k = 3..10 on the matrix cores) ----------------------------------------------------------------
RDM_SUB, RDM_FLUSH, RDM_TARGET_WG, RDM_MIN_CHUNKS = 10, 256, 2048, 4         # dq_rdm.hip:36-40


def rdmk(n: int, k: int, nc: int, batch: int, c128: bool, herm: bool) -> dict:
    """dq_rdm.hip, rdm_tile / rdm_plan / rdmk_cross_impl for ONE launch (batch <= 65535).  ``tile``: TT, ``dt`` its valid
    rows, ``nt`` tiles per side, ``ntl`` tile slots; ``kc`` contraction indices per chunk (the lowest ``chunk_bits`` rest
    bits), ``chunks`` in all, ``nsplit`` x ``nch`` of them per workgroup (splits = the top bits of the chunk number).
    ``flushes``: f32 -> double flushes inside the chunk loop (complex64 only; one more follows the loop), ``flush_then_more``:
    one of them is followed by further chunks.  ``pad_rows``: 2^k < TT; ``pad_chunk``: fewer rest bits than chunk bits."""
    tt = 64 if k >= 6 else (32 if k == 5 else 16)
    tbits = tt.bit_length() - 1
    cbits = RDM_SUB - tbits
    d = 1 << k
    dt = min(d, tt)
    nt = d // dt
    ntl = nt * (nt + 1) // 2 if herm else nt * nt
    r = n - k - nc
    total = 1 << (r - cbits) if r > cbits else 1
    per_split = batch * ntl * dt * dt * 2
    budget = (batch * d * d * 16 + (batch << n) * _csize(c128) // 100) // 8
    ns = 1
    while ns * 2 * RDM_MIN_CHUNKS <= total and per_split * ns * 2 <= budget and batch * ntl * ns < RDM_TARGET_WG:
        ns *= 2
    nch = total // ns
    return dict(tile=tt, dt=dt, nt=nt, ntl=ntl, kc=1 << cbits, chunk_bits=cbits, chunks=total, nsplit=ns, nch=nch,
                terms=1 << r, workgroups=batch * ntl * ns,
                flushes=0 if c128 else nch // RDM_FLUSH, flush_then_more=not c128 and nch > RDM_FLUSH,
                pad_rows=d < tt, pad_chunk=r < cbits, ws_bytes=8 * per_split * ns)


# ---- dq_dist.hip: permute_bits, pack, unpack_axpby -------------------------------------------------------------------------
def permute(nl: int, src_of_dst, batch: int, c128: bool, lds: bool = True) -> dict:
    """dq_dist.hip:198-259: the variant ('lds', 'tiled_pair', 'tiled', 'elementwise'), its workgroups, their loop
    iterations and (tiled kernels) the streaming flag.  ``lds`` False: under DQ_PERMUTE_LDS=0 (the LDS kernel is off)."""
    low_in_place = all(src_of_dst[p] < 5 for p in range(min(5, nl)))
    if nl >= 12 and not low_in_place and lds:
        ntile = 1 << (nl - 10)
        nblk = min(ntile, 256 * 16)
        return dict(variant='lds', blocks=nblk, iterations=_cdiv(ntile, nblk), nt=False)
    if nl >= 12:
        pair = not c128 and src_of_dst[0] == 0
        ntile = 1 << (nl - (1 if pair else 0) - 10)
        nblk = min(ntile, 256 * 16)
        return dict(variant='tiled_pair' if pair else 'tiled', blocks=nblk, iterations=_cdiv(ntile, nblk),
                    nt=(batch << nl) * _csize(c128) >= GIB)
    nb = min(_cdiv(1 << nl, 256), 65536)
    return dict(variant='elementwise', blocks=nb, iterations=_cdiv(1 << nl, nb * 256), nt=False)


def pack(nl: int, mask: int) -> dict:
    """dq_dist.hip:290-292 (pack) and :308-310 (unpack_axpby): one thread per packed amplitude, at most 65536 workgroups."""
    count = 1 << (nl - bin(mask).count('1'))
    nb = min(_cdiv(count, 256), 65536)
    return dict(blocks=nb, iterations=_cdiv(count, nb * 256))


# ---- dq_wave.hip: wave_launch and the prologue of wave_pass_kernel ---------------------------------------------------------
WAVE_TPW_FLOOR = 2048                                                        # dq_wave.hip:649 / :652


def wave_pass(n: int, batch: int, c128: bool, *, grad: bool = False, only_expz: bool = False, ext: bool = False,
              shared_input: bool = False, zero_bits_outside: int = 0, slice_bits: int = 0, env: dict | None = None) -> dict:
    """dq_wave.hip, wave_launch (:619-687) and the kernel's prologue (:137-175), for the default environment (no DQ_WAVE_*
    variable set) or, with ``env``, under the measurement knobs it names (DQ_WAVE_NT, _XCD, _TPW, _GRAD_TPW, _EXPZ_TPW,
    _XCD_TPW as strings, parsed like atoi; DQ_WAVE_TILE_ORDER changes which index bit a tile-number bit stands for, not the
    launch).  ``grad``: a reducing launch (``grads`` given: the GRAD instantiation); ``only_expz``: it holds no
    DQ_FG_GRAD record; ``ext``: its records lie in device memory; ``shared_input``: ONE input state for the batch
    (in_bstride = 0); ``zero_bits_outside`` / ``slice_bits``: known-zero / held index bits outside the tile.

    tiles, tpw (tiles a wave walks), grid_x, xcd (the value of bits 18..22 of the flag word: 31 or 0), regroup (the
    shared-input renumbering of :141-146 runs), nt_loads / nt_stores (what the body is told, :205), idle_waves (waves of the
    last workgroup of a sample that find no first tile, :173) and second_stride (what :174 adds to a wave's tile number
    for its second and every later walk; None at tpw = 1: the sum is formed but the walk it leads to is past the tile
    count).  xcd under DQ_WAVE_XCD = C > 1: log2(C) + 1 where grid.x % (8 C) == 0."""
    env = env or {}
    knob = lambda name, default: int(env.get('DQ_WAVE_' + name, default))                              # noqa: E731
    m = 11 if c128 else 12                                                    # :46 / :61 (W::M)
    tiles = 1 << (n - m - zero_bits_outside - slice_bits)                     # :382-397 (nb), :637
    tpw = 1
    if grad:                                                                  # :639
        cap = knob('EXPZ_TPW', 2) if only_expz else knob('GRAD_TPW', 2)       # :642 / :644 / :648 (gcap, zcap: 2 by default)
        assert not (ext and only_expz)                                        # :645 (records in device memory: never only_expz)
        while tpw < cap and (tiles * batch) // (8 * tpw) >= WAVE_TPW_FLOOR:   # :649
            tpw *= 2
    else:
        while tpw < knob('TPW', 1) and (tiles * batch) // (8 * tpw) >= WAVE_TPW_FLOOR:      # :651-652 (idle by default)
            tpw *= 2
    grid_x = _cdiv(tiles, 4 * tpw)                                            # :654
    nt_bits = knob('NT', 3 if (batch << n) * _csize(c128) >= GIB else 0) & 3   # :665-667 (bit 0 loads, bit 1 stores)
    xcd_env, xcd = knob('XCD', 1), 0                                          # :668, :672
    if xcd_env and not shared_input and (tpw == 1 or knob('XCD_TPW', 1)):     # :677
        if xcd_env == 1 and grid_x % 8 == 0:                                  # :678
            xcd = 31
        elif xcd_env > 1 and xcd_env & (xcd_env - 1) == 0 and grid_x % (8 * xcd_env) == 0:     # :679-680
            xcd = xcd_env.bit_length()
    regroup = shared_input and grid_x % 8 == 0                                # :141
    per_wg = 4 * tpw
    walked = grid_x * 4                                                       # first-walk tile numbers 0 .. walked - 1 (:159)
    return dict(tiles=tiles, tpw=tpw, grid_x=grid_x, xcd=xcd, regroup=regroup,
                nt_loads=bool(nt_bits & 1) and not shared_input, nt_stores=bool(nt_bits & 2),      # :205 (a shared input: no streaming loads)
                idle_waves=max(0, walked - tiles),                            # :173 at the first tile
                second_stride=_cdiv(tiles, per_wg) * 4 if tpw >= 2 else None)  # :174


def wave_grid_visits(geo: dict, batch: int) -> list[tuple[int, int]]:
    """The kernel's index arithmetic (:138-175) re-done for every workgroup and wave of the grid ``geo`` describes: the
    (sample, tile) pairs it visits, in any order, duplicates kept."""
    gx, tiles, tpw = geo['grid_x'], geo['tiles'], geo['tpw']
    lper = 2 + (tpw.bit_length() - 1)                                         # :172
    stride = ((tiles + (1 << lper) - 1) >> lper) * 4                          # :174
    step = geo['second_stride'] if geo['second_stride'] is not None else stride     # (the mirror's own line is what is walked)
    assert step > 0
    out = []
    for by in range(batch):
        for bx in range(gx):
            grp, sample = bx, by                                              # :138
            if geo['regroup']:                                                # :141-146
                lin = by * gx + bx
                group, r = divmod(lin, 8 * batch)
                sample, grp = r >> 3, group * 8 + (r & 7)
            xv = geo['xcd']
            if xv:                                                            # :151-157
                q, j = bx >> 3, bx & 7
                if xv == 31:
                    grp = j * (gx >> 3) + q
                else:
                    grp = ((q >> (xv - 1)) << (xv + 2)) + (j << (xv - 1)) + (q & ((1 << (xv - 1)) - 1))
            for wave in range(4):
                t = grp * 4 + wave                                            # :159
                while t < tiles:                                              # :173
                    out.append((sample, t))
                    t += step                                                 # :174
    return out
