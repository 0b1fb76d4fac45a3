"""The derivatives of the streaming nodes of ``ops`` on the MI355X -- ``_CostPhase``, ``_CostCross``, ``_CostScale``,
``_DiagMul``, ``_GenAxpby`` / ``_GenCross`` / ``_GenRot`` for Pauli strings and for excitations, ``_PermuteBasis``,
``_MuxApply``, ``_MuxAxpby`` / ``_MuxCross`` / ``_MuxRot`` (the trainable multiplexers: a row of 2^k parameters, shared or one
per sample, and reductions judged bin by bin) -- at the shapes of the families' kernel tests, in complex64 and
complex128: the forward, reverse mode, forward mode and ``torch.vmap`` against the closed forms of
tests/_stream_grad_ref.py (numpy complex128, built from the forward references alone).  The cases, the criteria and the checks are in tests/_stream_grad_cases.py, which test_stream_autograd_cpu.py runs
through the plain-torch stand-ins as well.

The layout cases hand the nodes what autograd hands them: an expanded cotangent, a strided one, one that is contiguous at
element offset 1 of a flat buffer (a complex64 pointer at 8 mod 16, which the kernels' entry points refuse before any
launch and ``ops`` therefore copies), and states at such an offset -- through the streaming families only, whose entry
points validate alignment."""

import pytest

import _stream_grad_cases as cases

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('family,name', cases.CASE_IDS, ids=[f'{f}-{n}' for f, n in cases.CASE_IDS])
def test_vjp_and_jvp_against_the_closed_forms(family, name, dt):
    for node in cases.nodes_of(family, name, dt):
        cases.check_forward(node, dt, DEVICE)
        cases.check_vjp(node, dt, DEVICE)
        cases.check_jvp(node, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('family', list(cases.FAMILIES))
def test_vmap_folds_into_the_batch_bit_for_bit(family, dt):
    cases.vmap_checks(family, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('family', list(cases.FAMILIES))
def test_cotangent_and_state_layouts(family, dt):
    for node in cases.nodes_of(family, cases.LAYOUT_CASE[family], dt):
        cases.check_layouts(node, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_a_loss_over_cat_hands_the_node_a_cotangent_at_offset_1(dt):
    cases.check_cat_loss(dt, DEVICE)
