"""The CPU twin of test_stream_autograd_gpu.py: the same case tables, checks and closed-form references
(tests/_stream_grad_cases.py, tests/_stream_grad_ref.py) through the plain-torch stand-ins of ``backend`` under the CPU
test double.  It validates the references, and the rules of the nodes as far as they do not depend on a kernel; the
stand-ins do not care about alignment, so what ``ops`` hands a kernel is asserted on the helper itself.  The trainable
multiplexers (``_MuxAxpby`` / ``_MuxCross`` / ``_MuxRot``) are the family 'muxgrad' of the tables; the negative controls of
their per-bin criterion need no node at all and run here."""

import pytest
import torch

from deepquantum_amd import ops

import _stream_grad_cases as cases

DEVICE = 'cpu'


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('family,name', cases.CASE_IDS, ids=[f'{f}-{n}' for f, n in cases.CASE_IDS])
def test_vjp_and_jvp_against_the_closed_forms(cpu_backend, family, name, dt):
    for node in cases.nodes_of(family, name, dt):
        cases.check_forward(node, dt, DEVICE)
        cases.check_vjp(node, dt, DEVICE)
        cases.check_jvp(node, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('family', list(cases.FAMILIES))
def test_vmap_folds_into_the_batch_bit_for_bit(cpu_backend, family, dt):
    cases.vmap_checks(family, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('family', list(cases.FAMILIES))
def test_cotangent_and_state_layouts(cpu_backend, family, dt):
    for node in cases.nodes_of(family, cases.LAYOUT_CASE[family], dt):
        cases.check_layouts(node, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_a_loss_over_cat_hands_the_node_a_cotangent_at_offset_1(cpu_backend, dt):
    cases.check_cat_loss(dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_the_per_bin_criterion_rejects_four_wrong_rules(dt):
    cases.negative_controls(dt)


def test_the_backward_of_cat_yields_a_contiguous_cotangent_at_offset_1():
    """What the layout cases imitate: the cotangent that ``cat([h, y.reshape(-1)])`` passes to the node that made y."""
    seen = []

    class Spy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            seen.append((g.is_contiguous(), g.storage_offset(), g.data_ptr() % 16))
            return g

    x = torch.randn(2, 8, dtype=torch.complex64, requires_grad=True)
    h = torch.ones(1, dtype=torch.complex64)
    torch.cat([h, Spy.apply(x).reshape(-1)]).abs().pow(2).sum().backward()
    assert seen == [(True, 1, 8)]


def test_what_a_kernel_gets_is_16_byte_aligned():
    """``ops._kernel_arg`` -- what every streaming node passes to ``backend`` as a state -- copies a tensor whose data
    pointer is not 16-byte aligned (the entry points refuse it) and leaves every other tensor alone."""
    flat = torch.arange(33, dtype=torch.float32).to(torch.complex64)
    assert flat.data_ptr() % 16 == 0
    odd = flat[1:].reshape(2, 16)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    got = ops._kernel_arg(odd)
    assert got.data_ptr() % 16 == 0 and got.is_contiguous() and torch.equal(got, odd)
    even = flat[2:18].reshape(1, 16)
    assert even.data_ptr() % 16 == 0 and ops._kernel_arg(even) is even
    wide = torch.zeros(9, dtype=torch.complex128)[1:].reshape(1, 8)                 # complex128: every element offset is aligned
    assert ops._kernel_arg(wide) is wide
    lazy = odd.conj()                                                                # a pending conjugation is resolved on the way
    got = ops._kernel_arg(lazy)
    assert not got.is_conj() and got.data_ptr() % 16 == 0 and torch.equal(got, odd.conj().resolve_conj())
