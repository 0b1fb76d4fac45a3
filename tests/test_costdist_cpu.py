"""Cost distributions, CVaR and the Gibbs objective under the CPU test double: binning, wire-to-bit mapping, CVaR, refusals."""

import itertools
import os
import re

import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops, qmath
from _hist_ref import binned_ref, hist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
EDGES = [(i, j) for i, j in itertools.combinations(range(N), 2) if (i * 7 + j * 3) % 4 != 0]


def maxcut_table():
    # -(number of cut edges): the sum over the edges of (z_i z_j - 1) / 2
    return qmath.ising_cost(N, [(0.5, [i, j]) for i, j in EDGES], dtype=torch.float64) - 0.5 * len(EDGES)


def rand_state(batch, seed=0):
    return torch.randn(batch, 1 << N, dtype=torch.complex128, generator=torch.Generator().manual_seed(seed))


def sorted_cvar(p, c, alpha, upper=False):
    order = torch.argsort(c, descending=upper)
    p, c, left, val = p[order] / p.sum(), c[order], alpha, 0.0
    for pi, ci in zip(p.tolist(), c.tolist()):
        take = min(pi, left)
        val, left = val + take * ci, left - take
    return val / alpha


def test_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    names = ['dq_cost_hist_max_bins', 'dq_cost_hist_ws_bytes'] + [f'dq_{f}_{s}' for f in ('cost_hist', 'apply_binned') for s in ('c64', 'c128')]
    for name in names:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and re.search(rf'\b{name}\(', text)
    assert backend.cost_hist_max_bins() >= 1024


def test_stand_ins_follow_the_definition(cpu_backend):
    n, bits, controls, nbins = 5, (0, 4, 2), (1,), 6
    x, y = rand_state(2, 1)[:, :32].contiguous(), rand_state(2, 2)[:, :32].contiguous()
    tab = torch.tensor([5, 0, 3, 3, 1, 0, 2, 5])
    assert torch.allclose(backend.cost_hist(x, y, tab, nbins, bits, controls), hist_ref(x, y, tab, nbins, n, bits, controls)[0], atol=1e-14)
    g = torch.randn(2, nbins, dtype=torch.complex128, generator=torch.Generator().manual_seed(3))
    assert torch.allclose(backend.apply_binned(x, g, tab, bits, controls), binned_ref(x, g, tab, n, bits, controls), atol=1e-14)
    xg, gg = x.clone().requires_grad_(), g.clone().requires_grad_()
    assert torch.autograd.gradgradcheck(lambda a, b: ops.apply_binned(a, b, tab, bits, controls), (xg, gg))
    with pytest.raises(ValueError, match=r'\[0, 6\)'):
        backend.cost_hist(x, y, tab + 1, nbins, bits, controls)
    with pytest.raises(ValueError, match='constant'):
        ops.cost_hist(x, y, torch.zeros(8, requires_grad=True), nbins, bits, controls)


def test_cost_distribution_against_a_dictionary(cpu_backend):
    c = maxcut_table()
    psi = rand_state(3)
    values, probs = qmath.cost_distribution(psi, N, c)
    for b in range(3):
        want = {}
        for i in range(1 << N):
            want[float(c[i])] = want.get(float(c[i]), 0.0) + abs(complex(psi[b, i])) ** 2
        assert values.tolist() == sorted(want) and probs.shape == (3, len(want))
        assert torch.allclose(probs[b], torch.tensor([want[v] for v in sorted(want)], dtype=torch.float64), atol=1e-12)
    # wires[0] is the most significant bit of the entry index; a single state gives (V,)
    v2, p2 = qmath.cost_distribution(psi[0], N, torch.tensor([0.0, 1.0, 1.0, 3.0]), wires=[6, 1])
    i = torch.arange(1 << N)
    entry = (((i >> (N - 1 - 6)) & 1) << 1) | ((i >> (N - 1 - 1)) & 1)
    mass = psi[0].abs() ** 2
    assert v2.tolist() == [0.0, 1.0, 3.0] and p2.shape == (3,)
    assert torch.allclose(p2, torch.stack([mass[entry == 0].sum(), mass[(entry == 1) | (entry == 2)].sum(), mass[entry == 3].sum()]))


@pytest.mark.parametrize('tail', ['lower', 'upper'])
@pytest.mark.parametrize('alpha', [0.05, 0.3, 1.0])
def test_cvar_against_sorting_the_outcomes(cpu_backend, alpha, tail):
    c = maxcut_table()
    psi = rand_state(2, 4) * 1.7                 # not normalised: CVaR is taken on the normalised distribution
    got = qmath.cvar_cost(psi, N, c, alpha, tail=tail)
    for b in range(2):
        p = psi[b].abs() ** 2
        assert abs(float(got[b]) - sorted_cvar(p, c, alpha, tail == 'upper')) < 1e-12
        if alpha == 1.0:
            assert abs(float(got[b]) - float(qmath.expectation_cost(psi[b] / psi[b].norm(), N, c))) < 1e-12
    # alpha = 0.3 splits its threshold bin: the bins strictly below it hold less than alpha, with it more
    values, probs = qmath.cost_distribution(psi[0], N, c)
    cdf = (probs / probs.sum()).cumsum(0)
    t = int((cdf < 0.3).sum())
    assert (cdf[t - 1] if t else 0.0) < 0.3 - 1e-3 and cdf[t] > 0.3 + 1e-3


def test_cvar_gradient_through_a_two_layer_qaoa_circuit(cpu_backend):
    c = maxcut_table()
    cir = dq.QubitCircuit(N)
    cir.hlayer()
    for _ in range(2):
        cir.cost_phase(c)
        cir.rxlayer()
    cir.to(torch.double)
    params = [p for p in cir.parameters() if p.requires_grad]

    def value():
        cir()
        return cir.cvar_cost(c, 0.3) + 0.1 * qmath.gibbs_cost(cir.state, N, c, 0.5).sum()

    torch.autograd.backward(value().sum())
    eps, worst = 1e-6, 0.0
    with torch.no_grad():
        for p in params:
            for j in range(min(p.numel(), 3)):
                flat = p.view(-1)
                flat[j] += eps
                up = float(value().sum())
                flat[j] -= 2 * eps
                down = float(value().sum())
                flat[j] += eps
                worst = max(worst, abs((up - down) / (2 * eps) - float(p.grad.view(-1)[j])))
    assert len(params) >= 4 and worst < 1e-7


def test_binning_by_edges_and_the_cap(cpu_backend):
    c = maxcut_table()
    psi = rand_state(1, 6)
    edges = torch.tensor([-20.0, -12.0, -9.0, 0.0])
    values, probs = qmath.cost_distribution(psi, N, c, bins=edges)
    mass = psi[0].abs() ** 2
    want = torch.stack([mass[(c >= lo) & ((c < hi) | (hi == 0.0))].sum() for lo, hi in zip(edges[:-1].tolist(), edges[1:].tolist())])
    assert values.tolist() == [-16.0, -10.5, -4.5] and torch.allclose(probs[0], want, atol=1e-12)
    assert abs(float(qmath.cvar_cost(psi, N, c, 1.0, bins=edges)) - float((want * values).sum() / want.sum())) < 1e-12
    prepared = qmath.cost_bins(c, edges)
    assert torch.equal(qmath.cost_distribution(psi, N, prepared)[1], probs)
    with pytest.raises(ValueError, match=rf'max_bins = {backend.cost_hist_max_bins()}.*bins='):
        qmath.cost_distribution(torch.ones(1 << 11, dtype=torch.complex128), 11, torch.arange(1 << 11, dtype=torch.float64))
    with pytest.raises(ValueError, match='outside the edges'):
        qmath.cost_distribution(psi, N, c, bins=[-3.0, 0.0])


def test_refusals():
    c = torch.zeros(4)
    dm = dq.QubitCircuit(2, den_mat=True)
    dm.state = torch.eye(4, dtype=torch.complex64)
    sharded = dq.DistributedQubitCircuit.__new__(dq.DistributedQubitCircuit)
    for cir in (dm, sharded):
        with pytest.raises(NotImplementedError, match='cost_distribution'):
            cir.cost_distribution(c)
        with pytest.raises(NotImplementedError, match='cvar_cost'):
            cir.cvar_cost(c, 0.5)
    with pytest.raises(ValueError, match='alpha'):
        qmath.cvar_cost(torch.ones(4) + 0j, 2, c, 0.0)
