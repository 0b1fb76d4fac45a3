"""What the large-grid GPU tests (test_grid_paths_gpu.py) stand on, checked without a GPU:

- the launch-geometry mirrors (_launch_geometry.py) against the thresholds where each launcher changes path, and the
  entanglement plan against the workspace size the built library reports (``dq_rdm1_ws_bytes`` is a function of the
  per-pass workgroup counts);
- every complex128 reference of _grid_refs.py against the CPU oracle or the CPU test backend at small n, so that the bit
  and matrix-index conventions the GPU cases compare with are established, not assumed."""

import random

import pytest
import torch

import _grid_refs as R
import _launch_geometry as G
from _cpu_backend import CpuTestBackend
from deepquantum_amd import _lib
from oracle import statevec_oracle as oracle
from test_entanglement_gpu import explicit_rdm1_cross, explicit_wire_sum
from test_rdm_gpu import explicit_cross


# ---- the mirrors ---------------------------------------------------------------------------------------------------------
def test_dense_mirror_thresholds():
    # apply_dense56_kernel, k = 5: a second loop iteration from n = 20 with batch 4 (complex64, shared U: 4096 groups vs
    # 768 workgroups x 4), n = 22 with batch 2 (per-sample U), n = 20 with batch 2 (complex128, shared U)
    assert G.dense(19, 5, 0, 4, False, True, False)['iterations'] == 1
    g = G.dense(20, 5, 0, 4, False, True, False)
    assert (g['route'], g['ngroups'], g['per_pass'], g['iterations']) == ('dense56', 4096, 3072, 2)
    assert G.dense(21, 5, 0, 2, False, False, False)['iterations'] == 1
    assert G.dense(22, 5, 0, 2, False, False, False)['iterations'] == 2
    assert G.dense(19, 5, 0, 2, True, True, False)['iterations'] == 1
    assert G.dense(20, 5, 0, 2, True, True, True) == dict(route='dense56', nt=False, ngroups=4096, col_group=16,
                                                          per_pass=2048, iterations=2)
    # k = 6 complex64: n = 21, batch 2 (2048 groups vs 512 workgroups x 2); complex128 k = 6 stays on the staged kernel
    assert G.dense(20, 6, 0, 2, False, True, False)['iterations'] == 1
    assert G.dense(21, 6, 0, 2, False, True, False)['iterations'] == 2
    assert G.dense(21, 6, 0, 2, True, True, False)['route'] == 'staged2'
    # complex64 with bit 0 among the targets / controls: the staged kernels
    assert G.dense(20, 5, 0, 4, False, True, True)['route'] == 'staged1'
    assert G.dense(20, 8, 1, 1, False, True, False)['route'] == 'staged2'
    # the non-temporal instantiations from 1 GiB: complex64 n = 27, complex128 n = 26
    assert not G.dense(26, 5, 0, 1, False, True, False)['nt'] and G.dense(27, 5, 0, 1, False, True, False)['nt']
    assert not G.dense(25, 5, 0, 1, True, True, False)['nt'] and G.dense(26, 6, 0, 1, True, True, False)['nt']


def test_reduction_mirror_thresholds():
    # the copy of uncontrolled amplitudes and probs loop above batch * 2^n = 2^24
    assert G.copy_uncontrolled(24, 1)['iterations'] == 1 and G.copy_uncontrolled(25, 1)['iterations'] == 2
    assert G.probs(1 << 24)['iterations'] == 1 and G.probs(1 << 25)['iterations'] == 2
    # gate_grad: k = 1 from n = 19, k = 2 with one control from n = 21
    assert G.gate_grad(18, 1, 0)['iterations'] == 1 and G.gate_grad(19, 1, 0)['iterations'] == 2
    assert G.gate_grad(20, 2, 1)['iterations'] == 1 and G.gate_grad(21, 2, 1)['iterations'] == 2
    assert G.gate_grad(20, 1, 0)['iterations'] == 4 and G.gate_grad(22, 2, 1)['iterations'] == 4
    # gate_grad_multi: complex64 n = 22, complex128 n = 21 (more tiles than 1536 workgroups)
    assert G.gate_grad_multi(21, False, [(0, ())])[0]['iterations'] == 1
    assert G.gate_grad_multi(22, False, [(0, ())])[0]['iterations'] == 2
    assert G.gate_grad_multi(20, True, [(0, ())])[0]['iterations'] == 1
    assert G.gate_grad_multi(21, True, [(0, ())])[0]['iterations'] == 2
    launches = G.gate_grad_multi(22, False, [(t, ()) for t in (4, 5, 6, 7, 8, 9, 10, 11, 0)])
    assert [la['gates'] for la in launches] == [[0, 1, 2, 3, 4, 5, 6], [7, 8]]      # 7 distinct high targets per tile
    assert launches[0]['tile_bits'] == list(range(11))
    # expect_pauli / inner: X and Y strings from n = 20, Z strings and inner from n = 19
    assert G.expect_pauli(19, 1)['iterations'] == 1 and G.expect_pauli(20, 1)['iterations'] == 2
    assert G.expect_pauli(18, 0)['iterations'] == 1 and G.expect_pauli(19, 0)['iterations'] == 2
    assert G.inner(1 << 18)['iterations'] == 1 and G.inner(1 << 19)['iterations'] == 2
    # scale_z_signs from n = 22; expect_z_multi complex128 from n = 22, complex64 from n = 23
    assert G.scale_zsigns(21)['iterations'] == 1 and G.scale_zsigns(22)['iterations'] == 2
    assert G.expect_zmulti(21, True)['iterations'] == 1 and G.expect_zmulti(22, True)['iterations'] == 2
    assert G.expect_zmulti(22, False)['iterations'] == 1 and G.expect_zmulti(23, False)['iterations'] == 2
    # marginal chunk runs: n = 24 with batch 1 or n = 22 with batch 4 (not n = 23 / 21)
    for c128 in (False, True):
        assert G.marginal(23, [22], 1, c128)['run'] == 0 and G.marginal(24, [23], 1, c128)['run'] == 1
        assert G.marginal(21, [20], 4, c128)['run'] == 0 and G.marginal(22, [21], 4, c128)['run'] == 1
    # (a chunk takes unmeasured bits first: with every bit above the contiguous part measured there is nothing to run over)
    assert G.marginal(24, list(range(23, 6, -1)), 1, False)['run'] == 0


def test_relayout_mirror_thresholds():
    ident = list(range(24))
    swap = [1, 0] + list(range(2, 24))
    lds = list(range(1, 24)) + [0]
    assert G.permute(23, list(range(23)), 1, False)['iterations'] == 1
    assert G.permute(24, ident, 1, False) == dict(variant='tiled_pair', blocks=4096, iterations=2, nt=False)
    assert G.permute(23, swap[:1] + [0] + list(range(2, 23)), 1, False)['iterations'] == 2
    assert G.permute(24, swap, 1, False)['variant'] == 'tiled'
    assert G.permute(24, ident, 1, True)['variant'] == 'tiled'
    assert G.permute(22, lds[:21] + [0], 1, False) == dict(variant='lds', blocks=4096, iterations=1, nt=False)
    assert G.permute(23, list(range(1, 23)) + [0], 1, False)['iterations'] == 2
    assert G.permute(26, list(range(26)), 1, False)['nt'] is False and G.permute(27, list(range(27)), 1, False)['nt']
    assert G.pack(25, 1)['iterations'] == 1 and G.pack(26, 1)['iterations'] == 2 and G.pack(26, 3)['iterations'] == 1


def test_entanglement_plan_against_the_library():
    # three passes and a tile loop from n = 23 with batch 2 (2048 tiles per pass, 1024 workgroups); the complex128 cross
    # reduction on its 11-bit tile: 4096 tiles per pass
    assert G.entangle(20, 1, False, False)['passes'] == 2
    e = G.entangle(23, 2, False, False)
    assert e['passes'] == 3 and e['ntiles'] == [2048] * 3 and e['nwg'] == [1024] * 3 and e['iterations'] == [2] * 3
    assert G.entangle(23, 2, True, True)['ntiles'] == [4096] * 3 and G.entangle(23, 2, True, True)['passes'] == 3
    assert G.entangle(22, 2, False, False)['iterations'] == [1, 1, 1]
    lib = _lib.load()
    for n in (1, 5, 11, 12, 13, 16, 20, 21, 23, 24, 26, 30):
        for batch in (1, 2, 3, 7, 2048, 3000):
            for c128 in (False, True):
                for cross in (False, True):
                    assert lib.dq_rdm1_ws_bytes(n, batch, int(c128), int(cross)) == G.rdm1_ws_bytes(n, batch, c128, cross), \
                        (n, batch, c128, cross)


# ---- the references against the oracle -----------------------------------------------------------------------------------
def _state(b, n, seed, dtype=torch.complex128):
    g = torch.Generator().manual_seed(seed)
    x = torch.view_as_complex(torch.randn(b, 1 << n, 2, generator=g, dtype=torch.float64))
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def _unitary(k, b, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.view_as_complex(torch.randn(b, 1 << k, 1 << k, 2, generator=g, dtype=torch.float64))
    return torch.linalg.qr(a)[0]


def _close(a, b, tol=1e-12):
    assert float((a.to(torch.complex128) - b.to(torch.complex128)).abs().max()) < tol


@pytest.mark.parametrize('n', [7, 10])
def test_references_against_the_oracle(n):
    rng = random.Random(n)
    be = CpuTestBackend()
    x, y = _state(3, n, 1), _state(3, n, 2)
    # apply_gate: shared and per-sample matrices, unsorted targets, controls, bit 0 and the top bit
    for targets, controls in (([3, 0, 5], []), ([n - 1, 2], [0]), (rng.sample(range(n), 5), []), ([4, 1, 3, 2, 5], [n - 1, 0])):
        for u in (_unitary(len(targets), 1, n)[0], _unitary(len(targets), 3, n + 1)):
            got, xm, ym = R.apply_gate(x, u, targets, controls)
            _close(got, oracle.apply_gate_bits(x, u, targets, controls))
            assert xm.shape == ym.shape == (3, 1 << len(targets), 1 << (n - len(targets) - len(controls)))
            _close(R.gate_matrix_view(x, targets, controls).reshape(xm.shape), xm)
    # gate_grad (k = 1, 2, controls) and the share of one gate_grad_multi tile (all tiles add up to the whole)
    for targets, controls in (([0], []), ([n - 1], [1]), ([2, 5], [0]), ([n - 1, 0], [3, 4])):
        _close(explicit_cross(x, y, targets, controls), be.gate_grad(x, y, targets, controls))
    tile_bits = [0, 1, 3, 5]
    for t, c in ((3, ()), (1, (5,)), (0, (n - 1,)), (5, (2, 0))):
        whole = sum(R.tile_cross(x, y, tile_bits, tile, t, c) for tile in range(1 << (n - len(tile_bits))))
        _close(whole, be.gate_grad(x, y, [t], list(c)))
    # expect_pauli: every phase i^ny, X on bit 0 and the top bit, and a Z-only string; S bounds the value
    for xmask, zmask in ((1 | 1 << (n - 1), 0), (1 | 1 << (n - 1), 1 << 3), (0b111, 0b001), (0b1011, 0b1011), (1 << (n - 1) | 5, 1 << (n - 1) | 5 | 8),
                         (0, 0b10010), (0, 0)):
        val, s = R.expect_pauli(x, xmask, zmask)
        _close(val, be.expect_pauli(x, xmask, zmask))
        assert (val.abs() <= s + 1e-12).all()
    ip, s = R.inner(x, y)
    _close(ip, torch.stack([torch.vdot(x[b], y[b]) for b in range(3)]))
    assert (ip.abs() <= s).all()
    masks = [1, 1 << (n - 1), (1 << n) - 1, 0b1010110 & ((1 << n) - 1)]
    zm, s = R.expect_z_multi(x, masks)
    _close(zm, torch.stack([be.expect_pauli(x, 0, z) for z in masks], dim=1))
    _close(s[:, 0], torch.ones(3, dtype=torch.float64))
    # scale_z_signs: sum_k c_k Z-string_k |x> by Z gates of the oracle
    coef = torch.randn(3, len(masks), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want = torch.zeros_like(x)
    z = oracle.fixed_matrix('z').to(torch.complex128)
    for k, m in enumerate(masks):
        t = x
        for p in range(n):
            if (m >> p) & 1:
                t = oracle.apply_gate_bits(t, z, [p])
        want += coef[:, k : k + 1] * t
    _close(R.scale_z_signs(x, masks, coef), want)
    # marginals (bits[0] = outcome MSB) and probabilities
    for bits in ([n - 1], [0, n - 1, 3], [2, n - 1, 0, 4, 1, 5, 3]):
        _close(R.marginal(x, bits), be.marginal(x, bits))
    _close(R.probabilities(x), oracle.probabilities(x))
    # the relayout indices
    for perm in (list(range(n))[::-1], rng.sample(range(n), n), list(range(1, n)) + [0]):
        out = torch.empty_like(x)
        _close(x[:, R.src_index(n, perm, 'cpu')], be.permute_bits(x, perm, out))
    for mask, value in ((1 << (n - 1), 1 << (n - 1)), (0b101, 0b001)):
        _close(x[:, R.expand_index(n, mask, value, 'cpu')], be.pack(x, mask, value))
    # the entanglement references: T_k[a, c] = conj(G[a, c]) with G = gate_grad(ket, bra, [k]); the wire sum by gates
    t, s = R.rdm1_cross(y, x)
    _close(t, explicit_rdm1_cross(y, x))
    _close(s.to(torch.complex128), explicit_rdm1_cross(y.abs(), x.abs()))
    for k in range(n):
        _close(t[:, k], be.gate_grad(x, y, [n - 1 - k], []).conj())     # (wire k = index bit n - 1 - k)
    mats = torch.view_as_complex(torch.randn(3, n, 2, 2, 2, generator=torch.Generator().manual_seed(4), dtype=torch.float64))
    want = sum(oracle.apply_gate_bits(x, mats[:, k], [n - 1 - k]) for k in range(n))
    _close(explicit_wire_sum(x, mats), want)
