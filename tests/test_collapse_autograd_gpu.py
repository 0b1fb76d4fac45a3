"""Derivatives of ``ops.collapse`` on the GPU: gradcheck / gradgradcheck in the state and in the scale (complex128, n = 5,
both layouts, masks on), and the complex64 backward at a several-unit shape against the complex128 one at 1e-4."""

import pytest
import torch

from deepquantum_amd import ops

pytestmark = pytest.mark.gpu

BITS = [3, 0]
OUTCOME, XMASK, ZMASK = [2, 1, 3], [0b10100, 0b00001, 0b01010], [0b00110, 0b11001, 0b10000]


def node(layout, bits=BITS):
    o, x, z = (torch.tensor(v, device='cuda') for v in (OUTCOME, XMASK, ZMASK))
    return lambda state, scale: ops.collapse(state, bits, o, scale, x, z, layout=layout)


@pytest.mark.parametrize('layout', ['full', 'drop'])
def test_gradcheck_and_gradgradcheck(layout):
    torch.manual_seed(0)
    state = torch.randn(3, 32, dtype=torch.complex128, device='cuda', requires_grad=True)
    scale = (torch.rand(3, dtype=torch.float64, device='cuda') + 0.5).requires_grad_()
    assert torch.autograd.gradcheck(node(layout), (state, scale), atol=1e-8)
    assert torch.autograd.gradgradcheck(node(layout), (state, scale), atol=1e-8)


@pytest.mark.parametrize('layout', ['full', 'drop'])
def test_complex64_backward_at_a_several_unit_shape(layout):
    torch.manual_seed(1)
    bits = [12, 0]
    state = torch.randn(3, 1 << 13, dtype=torch.complex128, device='cuda')
    scale = torch.rand(3, dtype=torch.float64, device='cuda') + 0.5
    grads = {}
    for dtype in (torch.complex64, torch.complex128):
        x, s = state.to(dtype).requires_grad_(), scale.clone().requires_grad_()
        y = node(layout, bits)(x, s)
        w = torch.linspace(0.5, 1.5, y.shape[1], device='cuda', dtype=y.real.dtype)
        ((y.abs() ** 2) * w).sum().backward()
        grads[dtype] = (x.grad.to(torch.complex128), s.grad)
    for lo, hi in zip(grads[torch.complex64], grads[torch.complex128]):
        assert (lo - hi).abs().max().item() <= 1e-4 * hi.abs().max().item()
    with pytest.raises(RuntimeError, match='vmap'):
        torch.vmap(lambda v: ops.collapse(v, bits, torch.tensor(OUTCOME, device='cuda'), scale))(state.to(torch.complex64)[None])
