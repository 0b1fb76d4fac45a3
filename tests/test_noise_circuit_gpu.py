"""``qmath.apply_noise_layer`` and ``cir.noise_layer`` on the GPU: the checks of ``tests/test_noise_cpu.py`` that take a device,
run on the kernels (forced outcomes against dense Kraus products, the draw rule, trajectories against the density matrix)."""

import pytest

from test_noise_cpu import NAMES, check_draw_rule, check_forced_outcomes, check_trajectories

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', NAMES)
def test_forced_outcomes_are_the_dense_kraus_products(name):
    check_forced_outcomes(name, 'cuda')


def test_draw_rule():
    check_draw_rule('cuda')


@pytest.mark.parametrize('name', NAMES)
def test_trajectories_average_to_the_density_matrix(name):
    check_trajectories(name, 'cuda')
