"""The exchange scheduler of a sharded circuit: the commutation-DAG order of the gates, the first
placement behind reset(), which qubits trade places at every remap, the eviction rule and the number of virtual rank bits.

Everything here is a pure function of the gate list's STRUCTURE (`structure`: per gate (kind, targets, controls, mode,
order), no matrices) and of the planner's settings (`Knobs`, built by `distributed._knobs` from CONFIG and MODEL): every
rank computes the same schedule, and the results are memoised on exactly those arguments.  Placements are physical bit
positions per logical qubit (``ph[q] >= L``: rank bit ``ph[q] - L``).  `distributed` runs the schedule; `dry_remaps` walks
it without data, for the choices made ahead of a run and for `distributed.count_exchange_steps`."""

from __future__ import annotations

from functools import lru_cache
from itertools import combinations
from typing import NamedTuple, Sequence

#: index bits below this are the contiguous low bits of a complex64 tile (fusion.default_geometry: min_low = 4; 3 for
#: complex128 -- the stricter bound serves both): `fusion._place_writes` folds a final permutation only if it fixes them
UNFOLDABLE_BELOW = 4

_INF = 1 << 60


class Knobs(NamedTuple):
    """Every setting the planner reads; part of every memoised result's key."""
    horizon: int                 # CONFIG['horizon']: how far `next_use` looks ahead
    reorder: bool                # CONFIG['reorder']
    initial_placement: bool      # CONFIG['initial_placement']
    first_exchange_local: bool   # CONFIG['first_exchange_local']
    evict_foldable: bool         # the eviction rule in force (CONFIG['evict_foldable'] resolved)
    model: tuple                 # sorted(MODEL.items()): the cost model of `modelled_cost`


def structure(prims) -> tuple:
    """What the exchange schedule of a gate list depends on (no matrices): the planner's input."""
    return tuple((p.kind, tuple(p.targets), tuple(p.controls), p.mode, tuple(p.order)) for p in prims)


def next_use(st: tuple, start: int, n: int, horizon: int) -> list[int]:
    """Index of the next gate (>= start, within ``horizon``) acting NON-diagonally on each logical qubit (inf if none)."""
    nxt = [_INF] * n
    left = n
    for j in range(start, min(len(st), start + horizon)):
        kind, targets = st[j][:2]
        if kind == 'diag':
            continue
        for t in targets:
            if nxt[t] == _INF:
                nxt[t] = j
                left -= 1
        if left == 0:
            break
    return nxt


def evict(ph: Sequence[int], nxt: Sequence[int], waiting, n: int, L: int, v: int, foldable: bool):
    """THE eviction rule: which qubits hold the far positions after a remap.  Farthest next use ``nxt`` first (Belady);
    ties: keep what already is global (less traffic), then qubits above the contiguous run of a tile, then canonical
    order.  With ``foldable`` (CONFIG['evict_foldable']) a local qubit on the contiguous low bits of a tile -- a fused
    pass's permuted store cannot move it: its remap would cost a re-labelling pass of its own -- is evicted only when
    nothing else is left (shards of at least a tile).

    ``v`` virtual rank bits (positions L .. L + v - 1; L = bits of a row): the two classes of far positions are re-filled
    SEPARATELY -- virtual ones when a qubit in ``waiting`` (the targets that wait for a remap) sits on one, real ones
    otherwise; the other class stays where it is.  Returns (leaving, entering, the new set of the class's qubits)."""
    if v:
        on_virtual = any(L <= ph[t] < L + v for t in waiting)
        mine = (lambda p_: L <= p_ < L + v) if on_virtual else (lambda p_: p_ >= L + v)
    else:
        mine = lambda p_: p_ >= L                 # noqa: E731
    is_glob = [mine(ph[q]) for q in range(n)]
    frozen = [ph[q] >= L and not is_glob[q] for q in range(n)]
    low = UNFOLDABLE_BELOW if (foldable and L >= 12) else 0
    cand = sorted((q for q in range(n) if not frozen[q]),
                  key=lambda q: (1 if (not is_glob[q] and ph[q] < low) else 0, -nxt[q], 0 if is_glob[q] else 1, 0 if ph[q] >= 4 else 1, -q))
    new_global = set(cand[:sum(is_glob)])
    leaving = [q for q in range(n) if is_glob[q] and q not in new_global]
    entering = [q for q in new_global if not is_glob[q]]
    return leaving, entering, new_global


def plan_remap(ph: Sequence[int], st: tuple, i: int, n: int, L: int, v: int, knobs: Knobs) -> list[tuple[int, int]]:
    """Which qubits trade places so that gate ``i`` of the (ordered) structure ``st`` becomes local (`evict`): [(leaving
    logical qubit, entering logical qubit)].  ``v``: a remap trades real rank bits only or virtual ones only -- virtual
    first when gate ``i`` waits for one; the caller comes back for the other class if the gate still is not local."""
    kind, targets = st[i][:2]
    needed = set(targets) if kind != 'diag' else set()
    leaving, entering, new_global = evict(ph, next_use(st, i, n, knobs.horizon), needed, n, L, v, knobs.evict_foldable)
    assert not (needed & new_global), 'gate needs more local qubits than a shard has'
    assert len(leaving) == len(entering) and leaving, 'remap requested although the gate is local'
    # a canonical global qubit (logical bit L + j) prefers its own rank bit j: cheaper to canonicalise later
    pairs, free_enter = [], list(entering)
    for lq in leaving:
        pick = next((eq for eq in free_enter if eq == ph[lq]), free_enter[0])
        free_enter.remove(pick)
        pairs.append((lq, pick))
    return pairs


def relabel(ph: list[int], pairs, L: int, slice_bits: Sequence[int] = ()) -> tuple[list, list[int], list[int]]:
    """THE re-labelling of a remap; updates ``ph``.  ``pairs`` go in ascending order of the rank bit they vacate
    (ascending peer rank); the entering qubits move to the top k local bits (chunk index = their joint value) with the
    local bits ``slice_bits`` right below them (`distributed._remap_sliced`), the other local qubits keep their order.
    Then entering qubit i takes rank bit rbits[i] and leaving qubit i local bit L - k + i.  Returns (sorted pairs, rbits,
    out_perm: source local bit -> destination local bit)."""
    pairs = sorted(pairs, key=lambda pr: ph[pr[0]])
    k = len(pairs)
    rbits = [ph[lq] - L for lq, _ in pairs]
    ent = [ph[eq] for _, eq in pairs]
    src_of_dst = [b for b in range(L) if b not in ent and b not in slice_bits] + list(slice_bits) + ent
    out_perm = [0] * L
    for d, sp in enumerate(src_of_dst):
        out_perm[sp] = d
    for q, p_ in enumerate(ph):
        if p_ < L:
            ph[q] = out_perm[p_]
    for i, (lq, eq) in enumerate(pairs):
        ph[eq] = L + rbits[i]
        ph[lq] = L - k + i
    return pairs, rbits, out_perm


@lru_cache(maxsize=16)
def order_indices(st: tuple, ph0: tuple, n: int, L: int, v: int, knobs: Knobs) -> tuple[int, ...]:
    """The gate list in an order that needs far fewer exchanges: list scheduling over the commutation DAG of the
    circuit (`fusion._Dag`: two gates commute when on every shared qubit both act diagonally, or both as functions of
    X) -- every gate that is ready and local under the current placement runs; only when ALL ready gates wait for a
    qubit on the rank bits does a remap happen (simulated with `evict`, swapping the qubits in place).
    In program order a gate on a global qubit stops everything behind it, although most of what follows neither
    depends on it nor touches that qubit: on the benchmark circuit (depth 40) the exchange steps go 15 -> 4 (2 ranks),
    20 -> 5 (4), 22 -> 5 (8 ranks) and the bytes on the wire down by 73-78 %.  The re-ordering is exact (commuting
    operators).  Memoised (round 6: 10 ms of host time for the 1360 gates of the n = 34 benchmark circuit, in front of
    the step's first launch)."""
    from . import fusion

    dag = fusion._Dag([fusion.PrimOp(kind, targets, controls, 0, mode) for kind, targets, controls, mode, _ in st], n)
    ph = list(ph0)
    retired = [False] * len(st)
    order: list[int] = []
    while dag.done < dag.n_ops:
        progressed = True
        while progressed:
            progressed = False
            for i in list(dag.ready):
                kind, targets = st[i][:2]
                if kind == 'diag' or all(ph[t] < L for t in targets):
                    order.append(i)
                    dag.retire(i)
                    retired[i] = True
                    progressed = True
        if dag.done >= dag.n_ops:
            break
        # every ready gate has a target on the rank bits: new global qubits = the ones not needed for longest
        nxt = [_INF] * n
        left = n
        for j in range(dag.ready[0], len(st)):
            if retired[j] or st[j][0] == 'diag':
                continue
            for t in st[j][1]:
                if nxt[t] == _INF:
                    nxt[t] = j
                    left -= 1
            if left == 0:
                break
        waits = {t for i in dag.ready if st[i][0] != 'diag' for t in st[i][1]}
        leaving, entering, _ = evict(ph, nxt, waits, n, L, v, knobs.evict_foldable)
        if not leaving:          # (cannot happen: some ready gate has a global target, and its next use is now)
            i = dag.ready[0]
            order.append(i)
            dag.retire(i)
            retired[i] = True
            continue
        for lq, eq in zip(leaving, entering):
            ph[lq], ph[eq] = ph[eq], ph[lq]
    return tuple(order)


def canonical_round(ph: Sequence[int], n: int, L: int) -> list[tuple[int, int]]:
    """The pairs of one exchange round of `distributed.canonicalize` (none: the rank bits are canonical): every misplaced
    rank bit trades with its owner, or with a filler while the owner itself sits on another rank bit."""
    pairs, used = [], set()
    for lq in (q for q in range(n) if ph[q] >= L and ph[q] != q):
        owner = ph[lq]                              # logical qubit that belongs on this rank bit
        pick = owner if (ph[owner] < L and owner not in used) else next(q for q in range(L) if ph[q] < L and q not in used)
        used.add(pick)
        pairs.append((lq, pick))
    return pairs


def dry_remaps(st: tuple, ph0: Sequence[int], n: int, lr: int, v: int, knobs: Knobs, restore: bool = False,
               reorder: bool = True) -> tuple[int, float, tuple]:
    """THE dry walk of the remap schedule from placement ``ph0`` (no data): (exchanges of real rank bits, their volume in
    shards, trace).  The trace has one (k, trades real rank bits, the re-labelling in front of it can ride on a pass: no
    entering qubit on the contiguous low bits of a tile) per remap, in order.  ``restore``: plus the exchanges of the
    canonicalisation at the end of a drop-in forward (``keep_layout=False``).  ``reorder``: the gates in commutation-DAG
    order first."""
    L = lr + v
    ph = list(ph0)
    if reorder:
        st = tuple(st[j] for j in order_indices(st, tuple(ph), n, lr, v, knobs))
    steps, vol, trace, i = 0, 0.0, [], 0
    while i < len(st):
        kind, targets = st[i][:2]
        if kind == 'diag' or all(ph[t] < lr for t in targets):
            i += 1
            continue
        pairs = plan_remap(ph, st, i, n, lr, v, knobs)
        foldable = all(ph[eq] >= UNFOLDABLE_BELOW for _, eq in pairs) or lr < 12
        # (a virtual remap is re-labelled here like a real exchange; the live `distributed._remap_virtual` only swaps the
        # two positions)
        _, rbits, _ = relabel(ph, pairs, lr)
        real = rbits[0] >= v
        assert all((r >= v) == real for r in rbits), 'a remap trades real OR virtual rank bits'
        trace.append((len(pairs), real, foldable))
        if real:
            steps += 1
            vol += 1 - 0.5**len(pairs)
    if restore:
        cs, cv = 0, 0.0
        for _ in range(4):
            pairs = canonical_round(ph, n, L)
            if not pairs:
                break
            relabel(ph, pairs, L)
            cs, cv = cs + 1, cv + (1 - 0.5 ** len(pairs))
        steps, vol = steps + cs, vol + cv
    return steps, vol, tuple(trace)


@lru_cache(maxsize=32)
def initial_placement(st: tuple, n: int, L: int, v: int, restore: bool, knobs: Knobs) -> tuple[int, ...]:
    """Where the qubits of a circuit that starts from |0..0> should sit at the start: |0..0> is the same vector under
    every permutation of the qubits (rank 0 holds the one non-zero amplitude at local index 0 in any of them), so the
    FIRST placement costs nothing -- no exchange, not even a re-labelling pass.  Candidates: the reference layout
    (wires 0 .. g-1 on the rank bits -- a layered circuit needs them within its first layer) and the placements that put
    g of the g + 3 qubits whose first non-diagonal gate comes last (farthest next use, asked at gate 0) on the rank bits
    and the next v on the virtual ones; each is dry-run through the whole remap schedule (`dry_remaps`, ~10 ms) and the
    one with the fewest exchanges wins -- the reference layout unless another one saves a whole exchange.  Never worse
    than the reference start, typically one exchange and one stretch boundary less (n = 34 on 8 ranks: 5 -> 4
    exchanges, 35 -> 33 passes).  ``restore`` (a drop-in forward, ``keep_layout=False``) charges every candidate the
    exchanges of the canonicalisation at its end too, so that "never worse than the reference start" holds for the step
    as it runs."""
    g = n - L
    canonical = tuple(range(n))
    if g <= 0 or not st:
        return canonical
    nxt = next_use(st, 0, n, knobs.horizon)
    order = sorted(range(n), key=lambda q: (-nxt[q], 0 if q >= L else 1, -q))
    lr = L - v
    best = (dry_remaps(st, canonical, n, lr, v, knobs, restore)[:2], 0, canonical)
    for ci, pick in enumerate(combinations(order[:g + 3], g)):
        ph = list(canonical)
        rest = [q for q in order if q not in pick]
        for positions, want in ((range(L, n), list(pick)), (range(lr, L), rest[:v])):
            have = [q for q in range(n) if ph[q] in positions]
            leaving = [q for q in have if q not in want]
            entering = [q for q in want if q not in have]
            for lq, eq in zip(leaving, entering):
                ph[lq], ph[eq] = ph[eq], ph[lq]
        cand = (dry_remaps(st, ph, n, lr, v, knobs, restore)[:2], ci + 1, ph)
        # (fewer EXCHANGES, not merely less volume: a placement that only trims the volume was measured to cost more in
        # passes and un-folded re-labellings than it saves on the wire -- rehearsal of n = 34 / 8 ranks with virtual bits)
        if cand[0][0] < best[0][0] or (cand[0][0] == best[0][0] and best[1] > 0 and cand[0] < best[0]):
            best = cand
    return tuple(best[2])


def modelled_cost(trace: Sequence[tuple], v: int, first_is_local: bool, model) -> float:
    """Cost of a remap schedule (a `dry_remaps` trace) in passes over the shard, by ``model`` (`distributed.MODEL`)."""
    wire_pass = model['pass_GBs'] / (2.0 * model['link_GBs'])       # one shard over ONE link, in passes
    cost, first = 0.0, first_is_local and v == 0
    for k, real, foldable in trace:
        cost += model['boundary_passes']
        if not foldable:
            cost += 1.0             # a re-labelling pass of its own in front of the exchange
        if real:
            if first:               # the first exchange behind reset() without the wire: a copy of 2^-k and a memset
                cost += 0.5
            else:
                cost += wire_pass / (1 << k) * (0.5 ** v)
            first = False
    return cost


def candidate_cost(st: tuple, n: int, L: int, v: int, fresh: bool, restore: bool, knobs: Knobs) -> tuple[float, tuple]:
    """(modelled cost, trace) of the circuit's schedule with ``v`` virtual rank bits under ``knobs``, dry-run from the
    placement it would start from (``fresh``: behind reset())."""
    ph = initial_placement(st, n, L, v, restore, knobs) if (fresh and knobs.initial_placement) else tuple(range(n))
    # (the dry walk re-orders even with CONFIG['reorder'] off, when the live run keeps program order)
    trace = dry_remaps(st, ph, n, L - v, v, knobs)[2]
    return modelled_cost(trace, v, fresh and knobs.first_exchange_local, dict(knobs.model)), trace


@lru_cache(maxsize=16)
def choose_eviction(st: tuple, n: int, L: int, v: int, fresh: bool, restore: bool, knobs: Knobs) -> bool:
    """CONFIG['evict_foldable'] = None: both eviction rules priced by `candidate_cost`, the cheaper one wins (ties: the
    foldable rule)."""
    cost = {rule: candidate_cost(st, n, L, v, fresh, restore, knobs._replace(evict_foldable=rule))[0] for rule in (True, False)}
    return cost[True] <= cost[False] + 1e-9


@lru_cache(maxsize=16)
def choose_virtual_bits(st: tuple, n: int, L: int, candidates: tuple, fresh: bool, restore: bool,
                        knobs: Knobs) -> tuple[int, tuple]:
    """CONFIG['virtual_bits'] = None: the candidate v that `candidate_cost` prices lowest (ties: the smaller v), and per
    candidate (v, cost in passes, remaps of real rank bits, of virtual ones, re-labelling passes of their own)."""
    best, rows = None, []
    for v in candidates:
        if L - v < 1:
            continue
        cost, trace = candidate_cost(st, n, L, v, fresh, restore, knobs)
        rows.append((v, cost, sum(1 for t in trace if t[1]), sum(1 for t in trace if not t[1]), sum(1 for t in trace if not t[2])))
        if best is None or cost < best[1] - 1e-9:
            best = (v, cost)
    return (best[0] if best else 0), tuple(rows)


def slice_qubits(ph: Sequence[int], st: tuple, i: int, n: int, L: int, pairs, nbits: int, horizon: int) -> list[int]:
    """The qubits the passes around the exchange ``pairs`` are sliced by: local, staying local, movable by a permuted store,
    and -- after the evicted ones -- needed LAST (farthest next non-diagonal use from gate ``i`` on): neither the gates
    left for the last pass in front of the exchange nor the first ones behind it have any business with them."""
    if nbits <= 0:
        return []
    nxt = next_use(st, i, n, horizon)
    leaving_local = {eq for _, eq in pairs}
    cand = sorted((q for q in range(n) if UNFOLDABLE_BELOW <= ph[q] < L and q not in leaving_local), key=lambda q: (-nxt[q], -q))
    return cand[:nbits]
