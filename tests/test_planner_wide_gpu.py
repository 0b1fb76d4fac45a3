"""The wide, newly priced pass planner on the GPU: `QubitCircuit` forward with the big-state planner settings forced on
(executor.CONFIG['plan_wide']) at n = 14, 15, 16 -- the smallest sizes with at least two passes and free low bits --
against the complex128 oracle, from the circuit's own |0..0> (zero-state passes) and from a random state."""

import pytest
import torch

import bench
import deepquantum_amd as dq
from oracle import statevec_oracle as oracle

pytestmark = pytest.mark.gpu

BATCH, DEPTH = 2, 20
_REF: dict = {}


def _reference(n):
    """Computed once per size, in complex128: (spec, angles, random input, result behind |0..0>, result behind the input)."""
    if n not in _REF:
        spec = bench.random_circuit_spec(n, DEPTH, 100 + n)
        _cir, data = bench.build_circuit(dq, n, spec, BATCH, torch.complex128, torch.device('cpu'))
        g = torch.Generator().manual_seed(n)
        x = torch.randn(BATCH, 1 << n, generator=g, dtype=torch.float64) + 1j * torch.randn(BATCH, 1 << n, generator=g, dtype=torch.float64)
        x = x / x.norm(dim=-1, keepdim=True)
        _REF[n] = (spec, data, x, oracle.run_spec(n, spec, dtype=torch.complex128, data=data),
                   oracle.run_spec(n, spec, dtype=torch.complex128, data=data, state=x.clone()))
    return _REF[n]


def _rel(out, ref):
    """The largest relative error of a sample: |out - ref| / |ref| in the 2-norm."""
    diff = out.reshape(BATCH, -1).cpu().to(torch.complex128) - ref
    return (diff.norm(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.fixture
def wide(monkeypatch):
    monkeypatch.setitem(dq.executor.CONFIG, 'plan_wide', True)


@pytest.mark.parametrize('dtype,tol', [(torch.complex64, 1e-4), (torch.complex128, 1e-10)], ids=['c64', 'c128'])
@pytest.mark.parametrize('n', [14, 15, 16])
def test_forward_with_the_wide_search(wide, n, dtype, tol):
    spec, data, x, ref_zero, ref_state = _reference(n)
    dev = torch.device('cuda', 0)
    cir, _ = bench.build_circuit(dq, n, spec, BATCH, dtype, dev)
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    with torch.no_grad():
        out = cir(data.to(dev, real))
        assert dq.executor.LAST_RUN['passes'] >= 2, 'the fused passes did not run'
        err = _rel(out, ref_zero)
        print(f'n = {n} {dtype} behind |0..0>: relative error {err:.3e}, passes {dq.executor.LAST_RUN["passes"]}')
        assert err < tol
        out = cir(data.to(dev, real), state=x.to(dev, dtype).reshape(BATCH, -1, 1))
        assert dq.executor.LAST_RUN['passes'] >= 2
        err = _rel(out, ref_state)
        print(f'n = {n} {dtype} behind a random state: relative error {err:.3e}')
        assert err < tol
