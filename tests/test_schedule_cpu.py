"""The exchange scheduler (deepquantum_amd/schedule.py) without a GPU.

``test_schedule_is_pinned``: the schedules of the benchmark generator (depth 40, seed 1234) -- first placement, commutation-DAG
order, the dry walk's trace, the pairs of every remap, ``count_exchange_steps``, the virtual-bits table and the eviction
choice -- for seven (n, g), v = 0, 1, 2 and both eviction rules, as a sha1 of their canonical JSON per case.  The pins were
made at commit 0f03612, before the planner moved into its own module: the move changed no schedule."""

from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from deepquantum_amd import distributed as D, schedule as S  # noqa: E402
from deepquantum_amd.executor import Prim  # noqa: E402

FT = (False, True)

#: '{n}-{g}-{v}-{eviction rule}': sha1 (first 16 hex digits) of the case's canonical JSON
PINS = {
    '9-2-0-1': '9c18fcbd42aa013c', '9-2-0-0': '9c18fcbd42aa013c', '9-2-1-1': '325682428dccb9b8',
    '9-2-1-0': '325682428dccb9b8', '9-2-2-1': '13383cca45f15603', '9-2-2-0': '13383cca45f15603',
    '17-1-0-1': '4a1c184e47b9414b', '17-1-0-0': 'bf570f3c408190c6', '17-1-1-1': '12eb7088e7c40f59',
    '17-1-1-0': '107fc978280bbe33', '17-1-2-1': '70cd7e0fe60e3397', '17-1-2-0': '938bd1e0ef28fb07',
    '20-2-0-1': '176504f77bc82e16', '20-2-0-0': '9657b867fdeb80f4', '20-2-1-1': '40df4f11d3eec0fa',
    '20-2-1-0': '0c02811ee82fcb8e', '20-2-2-1': 'aa64d11b4d1747dc', '20-2-2-0': '83a6a87d5955d346',
    '24-3-0-1': '6a11cf69cbc3bcc5', '24-3-0-0': '544f76fde53f03ce', '24-3-1-1': '731ae0cfaadc94d3',
    '24-3-1-0': '6f492c6b0e07ca53', '24-3-2-1': '8345737ce33e9ad8', '24-3-2-0': '01f7862bf281986c',
    '29-1-0-1': '4daf21f3b5890984', '29-1-0-0': '469c188ee730e7b3', '29-1-1-1': '73be1a3cb5d9ce47',
    '29-1-1-0': '63e1cf5dfcbc866d', '29-1-2-1': '28494a44dd7050f5', '29-1-2-0': '4fd91c0380d88a8e',
    '31-3-0-1': '19226b7e0bd3687d', '31-3-0-0': 'cbeb3bc7a17a7455', '31-3-1-1': '6408098c201a56fc',
    '31-3-1-0': '46ab7c2b9ea86693', '31-3-2-1': 'c2fd26ac2cbba267', '31-3-2-0': 'fd9301381dfc89e5',
    '34-3-0-1': 'dd7c6a50f5e3f9e9', '34-3-0-0': 'c9dc742b3faba2a5', '34-3-1-1': '51c96deb1904369b',
    '34-3-1-0': 'd3c43f2645f5bce3', '34-3-2-1': '428ab6906d8a47be', '34-3-2-0': 'fca6b65352539356',
}


def gate_prims(n: int, depth: int = 40, seed: int = 1234) -> list[Prim]:
    out = []
    for op in bench.random_circuit_spec(n, depth, seed):
        if op[0] == 'cnot':
            out.append(Prim('x', None, (n - 1 - op[2],), (n - 1 - op[1],), 0))
        else:
            out.append(Prim('gen', None, (n - 1 - op[1],), (), 3 if op[0] == 'h' else 2))
    return out


def walk_pairs(st, ph, n, lr, v, knobs):
    """The pairs of every remap of the schedule from placement ``ph``, as the live run plans them, and the placement at
    the end."""
    st = tuple(st[j] for j in S.order_indices(st, tuple(ph), n, lr, v, knobs))
    ph, out, i = list(ph), [], 0
    while i < len(st):
        kind, targets = st[i][:2]
        if kind == 'diag' or all(ph[t] < lr for t in targets):
            i += 1
            continue
        pairs, _, _ = S.relabel(ph, S.plan_remap(ph, st, i, n, lr, v, knobs), lr)
        out.append(pairs)
    return out, ph


def case(prims, n, g, v, rule, monkeypatch):
    L, lr = n - g, n - g - v
    knobs = D._knobs(rule)
    st = S.structure(prims)
    canon = tuple(range(n))
    place = [S.initial_placement(st, n, L, v, r, knobs) for r in FT]
    order = [S.order_indices(st, ph0, n, lr, v, knobs) for ph0 in (canon, place[0])]
    dry = [S.dry_remaps(st, ph0, n, lr, v, knobs, restore=r) for ph0 in (canon, place[0]) for r in FT]
    pairs, ph_end = walk_pairs(st, place[0], n, lr, v, knobs)
    count = [D.count_exchange_steps(prims, n, g, virtual_bits=v, reorder=ro, placement=pl, evict=rule) for ro in FT for pl in FT]
    monkeypatch.setitem(D.LAST_RUN, 'evict_foldable', rule)         # (the table prices with the last run's rule)
    vbits = [D.virtual_bits_table(prims, n, L, fresh=f, restore=r) for f in FT for r in FT]
    evict = [D.choose_eviction(prims, n, L, v, fresh=f, restore=r) for f in FT for r in FT]
    return {'placement': place, 'order': order, 'dry': dry, 'pairs': pairs, 'ph_end': ph_end, 'count': count,
            'vbits': vbits, 'evict': evict}


def test_schedule_is_pinned(monkeypatch):
    got, readable = {}, {}
    for n, g in ((9, 2), (17, 1), (20, 2), (24, 3), (29, 1), (31, 3), (34, 3)):
        prims = gate_prims(n)
        for v in (0, 1, 2):
            for rule in (True, False):
                d = json.loads(json.dumps(case(prims, n, g, v, rule, monkeypatch), sort_keys=True))
                got[f'{n}-{g}-{v}-{int(rule)}'] = hashlib.sha1(json.dumps(d, sort_keys=True).encode()).hexdigest()[:16]
                if n == 34:
                    readable[(v, rule)] = d['count'][3]
    # the n = 34 / 8-rank step (reorder and free first placement): 4 exchanges, 3.5 shards; with two virtual bits 9 remaps
    # (5 of them virtual) under the foldable rule, 10 under the other
    for rule in FT:
        assert (readable[(0, rule)]['remap_steps'], readable[(0, rule)]['remap_volume']) == (4, 3.5)
    assert (readable[(2, True)]['remap_steps'], readable[(2, True)]['virtual_steps']) == (9, 5)
    assert (readable[(2, False)]['remap_steps'], readable[(2, False)]['virtual_steps']) == (10, 5)
    assert got == PINS, {k: v for k, v in got.items() if PINS.get(k) != v}


def _answers(prims, n, g):
    L = n - g
    return json.dumps([D.virtual_bits_table(prims, n, L, fresh=True, restore=False),
                       [D.choose_eviction(prims, n, L, v, fresh=True) for v in (0, 1)],
                       D.initial_placement(prims, n, L, 0), D.initial_placement(prims, n, L, 1, restore=True),
                       D.count_exchange_steps(prims, n, g, reorder=True, placement=True),
                       D.count_exchange_steps(prims, n, g, virtual_bits=1, reorder=True, placement=True),
                       [prims.index(p) for p in D._order_for_remaps(prims, list(range(n)), n, L)]], sort_keys=True)


def _clear_caches():
    for f in (S.order_indices, S.initial_placement, S.choose_eviction, S.choose_virtual_bits):
        f.cache_clear()


def test_toggled_knobs_answer_like_a_fresh_process(monkeypatch):
    """Every planner setting is part of every memoised answer's key: toggled in-process, the planner answers what it
    answers with empty caches (stale orders, v and eviction choices after toggling 'horizon' or 'reorder')."""
    n, g = 20, 2
    prims = gate_prims(n)
    base = _answers(prims, n, g)
    changed = set()
    for where, key, value in ((D.CONFIG, 'horizon', 24), (D.CONFIG, 'reorder', False), (D.CONFIG, 'initial_placement', False),
                              (D.CONFIG, 'first_exchange_local', False), (D.MODEL, 'link_GBs', 15.0),
                              (D.LAST_RUN, 'evict_foldable', False)):
        assert _answers(prims, n, g) == base                    # (warm caches with the default settings)
        monkeypatch.setitem(where, key, value)
        toggled = _answers(prims, n, g)
        _clear_caches()
        assert _answers(prims, n, g) == toggled, key
        if toggled != base:
            changed.add(key)
        monkeypatch.undo()
        _clear_caches()
    assert {'horizon', 'link_GBs', 'evict_foldable'} <= changed, changed
