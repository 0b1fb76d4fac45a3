"""Schedules made from PRICED plans (fusion._plan_tiles_native with prices, both rankings) on the GPU, through the C ABI,
against the complex128 oracle: the forward of random circuits at n = 13 and 14 -- one and four tiles per sample for
complex64 -- batch 3, both precisions, on random states and behind |0..0> (the zero-extended passes of a priced plan)."""

import numpy as np
import pytest
import torch

from deepquantum_amd import backend, fusion

from test_planner_priced_cpu import _geom, hrc_ops, priced_steps
from test_wave_cpu import random_ops, reference
from test_zero_state_cpu import _written_dead

pytestmark = pytest.mark.gpu
TOL = {False: 1e-4, True: 1e-10}
PREC = pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
CASES = pytest.mark.parametrize('n,ngates,seed,free_low,rate,hrc', [(13, 150, 11, True, None, False), (14, 220, 12, True, None, True),
                                                                     (14, 200, 13, True, 5e-4, False), (13, 160, 14, False, 5e-4, True)])
BATCH = 3


def dev():
    return torch.device('cuda', 0)


_made = {}


def _case(n, ngates, seed, free_low, rate, hrc, is128):
    """(ops, matrices, steps, reference on a random state, reference on |0..0>) of a case, made once."""
    key = (n, ngates, seed, free_low, rate, hrc, is128)
    if key not in _made:
        dtype = torch.complex128 if is128 else torch.complex64
        ops, mats = hrc_ops(n, ngates, seed) if hrc else random_ops(n, ngates, seed)
        mats = mats.to(dtype)
        steps = priced_steps(ops, n, _geom(is128), free_low, rate)
        if steps is None:
            steps = priced_steps(ops, n, _geom(is128), False, rate)
        assert steps is not None and all(isinstance(s, fusion.FusedStep) for s in steps) and len(steps) >= 2
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(BATCH, 1 << n, generator=g, dtype=torch.float64) + 1j * torch.randn(BATCH, 1 << n, generator=g, dtype=torch.float64)
        x = (x / x.norm(dim=-1, keepdim=True)).to(dtype)
        x0 = torch.zeros(1, 1 << n, dtype=dtype)
        x0[0, 0] = 1
        _made[key] = (ops, mats, steps, x, reference(x, ops, mats), reference(x0, ops, mats))
    return _made[key]


@PREC
@CASES
def test_priced_plan_forward(n, ngates, seed, free_low, rate, hrc, is128):
    ops, mats, steps, x, ref, _ref0 = _case(n, ngates, seed, free_low, rate, hrc, is128)
    md = fusion.kernel_matrices(steps, ops, mats).to(dev())
    cur = x.to(dev())
    for st in steps:
        nxt = torch.empty_like(cur)
        backend.apply_fused(cur, md, 0, st.desc, out=nxt)
        cur = nxt
    err = (cur.cpu() - ref).abs().max().item()
    assert err < TOL[is128], err


@PREC
@CASES
def test_priced_plan_behind_the_zero_state(n, ngates, seed, free_low, rate, hrc, is128):
    """Every pass under its known-zero mask: the input NaN wherever such a bit is 1, the output full of a sentinel that
    survives exactly where the kernel has nothing to write."""
    ops, mats, steps, _x, _ref, ref0 = _case(n, ngates, seed, free_low, rate, hrc, is128)
    dtype = torch.complex128 if is128 else torch.complex64
    masks = fusion.zero_state_masks(steps, n)
    assert masks is not None and sum(1 for k in masks if k) >= 1
    md = fusion.kernel_matrices(steps, ops, mats).to(dev())
    idx = torch.arange(1 << n, dtype=torch.int64, device=dev())
    nan, sentinel = complex(float('nan'), float('nan')), complex(7.0, -7.0)
    cur = torch.zeros(BATCH, 1 << n, dtype=dtype)
    cur[:, 0] = 1
    cur = cur.to(dev())
    for st, kz in zip(steps, masks):
        if kz:
            src = cur.clone()
            src[:, (idx & kz) != 0] = nan
            out = torch.full((BATCH, 1 << n), sentinel, dtype=dtype, device=dev())
            backend.apply_fused(src, md, 0, st.desc, out=out, known_zero=kz)
            untouched = torch.from_numpy(_written_dead(st, kz, n, np.arange(1 << n, dtype=np.int64))).to(dev())
            assert bool((out[:, untouched] == sentinel).all()) and not bool((out[:, ~untouched] == sentinel).any())
            assert not bool(torch.isnan(out.real).any())
            cur = out
        else:
            assert not bool((cur == sentinel).any())
            nxt = torch.empty_like(cur)
            backend.apply_fused(cur, md, 0, st.desc, out=nxt)
            cur = nxt
    err = (cur.cpu() - ref0).abs().max().item()
    assert err < TOL[is128], err
