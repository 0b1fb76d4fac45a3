"""The host side that the streaming primitives share (csrc/dq_stream.hpp's checkers; backend._check_out, _finish_table,
_slices), without a GPU: the library's refusals are reached with made-up aligned pointers that are never dereferenced,
the wrappers run on the CPU test double."""

import numpy as np
import pytest
import torch

from deepquantum_amd import _lib, backend

N, BATCH = 3, 2                                          # 2 samples of 8 amplitudes: 128 (complex64) / 256 (complex128) bytes
P, Q, T = 1 << 20, 1 << 30, 4096                        # aligned non-null "pointers", far apart
ENTRIES = ('diag', 'cost_phase', 'cost_scale', 'pauli_axpby', 'permutation', 'mux')
SAME_OR_DISJOINT = ('diag', 'cost_phase', 'cost_scale', 'pauli_axpby', 'mux')


def call(entry, suffix, inp, out, batch=BATCH, later_bad=False):
    """The entry point on n = 3 with valid arguments; ``later_bad``: with one argument wrong that is looked at after the two
    state buffers (a table bit out of range, for the Pauli string a mask bit at or above n).  Returns (rc, text)."""
    lib, ia = _lib.load(), _lib.int_array
    bits, none = ia([3] if later_bad else [1]), ia([])
    if entry == 'diag':
        rc = getattr(lib, f'dq_apply_diag_{suffix}')(inp, out, T, 0, N, bits, 1, none, 0, batch, None)
    elif entry in ('cost_phase', 'cost_scale'):
        op = _lib.COST_PHASE if entry == 'cost_phase' else _lib.COST_SCALE
        rc = getattr(lib, f'dq_apply_cost_{suffix}')(inp, out, T, T, op, N, bits, 1, none, 0, batch, None)
    elif entry == 'pauli_axpby':
        rc = getattr(lib, f'dq_apply_pauli_axpby_{suffix}')(inp, out, 8 if later_bad else 1, 0, T, _lib.PAULI_GATE, N, none, 0, batch,
                                                            None)
    elif entry == 'permutation':
        rc = getattr(lib, f'dq_apply_permutation_{suffix}')(inp, out, T, N, bits, 1, none, 0, batch, _lib.PERM_AUTO, None)
    else:
        rc = getattr(lib, f'dq_apply_mux_{suffix}')(inp, out, T, _lib.MUX_U, 0, N, 0, bits, 1, none, 0, batch, None)
    return rc, lib.dq_last_error().decode()


LATER_WORD = {'pauli_axpby': 'at or above'}             # every other entry point: 'out of range'


@pytest.mark.parametrize('suffix,nbytes', [('c64', 128), ('c128', 256)])
@pytest.mark.parametrize('entry', ENTRIES)
def test_library_refuses_a_shifted_overlap_and_nothing_else(entry, suffix, nbytes):
    for inp, out in ((P, P + nbytes - 16), (P + nbytes - 16, P)):
        rc, text = call(entry, suffix, inp, out)
        assert rc == -1 and 'overlap' in text, text
    # the same buffer and the buffer right behind it are not overlaps: the refusal is the later argument's
    word = LATER_WORD.get(entry, 'out of range')
    for inp, out in ((P, P + nbytes), (P + nbytes, P)):
        rc, text = call(entry, suffix, inp, out, later_bad=True)
        assert rc == -1 and word in text and 'overlap' not in text, text
    rc, text = call(entry, suffix, P, P, later_bad=True)
    if entry in SAME_OR_DISJOINT:
        assert rc == -1 and word in text and 'overlap' not in text, text
    else:                                               # the permutation is out of place only
        assert rc == -1 and 'overlap' in text, text


@pytest.mark.parametrize('suffix', ['c64', 'c128'])
@pytest.mark.parametrize('entry', ENTRIES)
def test_library_checks_the_two_states_the_same_way_everywhere(entry, suffix):
    for kw, word in ((dict(inp=None, out=Q), 'null'), (dict(inp=P, out=None), 'null'), (dict(inp=P + 8, out=Q), 'aligned'),
                     (dict(inp=P, out=Q + 8), 'aligned'), (dict(inp=P, out=Q, batch=0), 'batch'),
                     (dict(inp=P, out=Q, batch=65536), 'batch')):
        rc, text = call(entry, suffix, **kw)
        assert rc == -1 and word in text, (kw, text)


def tt(a):
    return torch.from_numpy(np.asarray(a))


def wrappers():
    """name -> f(state, out) for a (2, 16) complex128 state, every other argument valid"""
    g = torch.Generator().manual_seed(3)
    d = torch.randn(4, dtype=torch.complex128, generator=g)
    c = torch.randn(4, dtype=torch.float64, generator=g)
    t = torch.tensor([0.3, -1.1], dtype=torch.float64)
    s = torch.tensor([0.5 + 0.25j, -2.0j], dtype=torch.complex128)
    u = torch.linalg.qr(torch.randn(4, 2, 2, dtype=torch.complex128, generator=g))[0]
    return {
        'apply_diag': lambda x, out: backend.apply_diag(x, d, (2, 0), (), out=out),
        'apply_cost[phase]': lambda x, out: backend.apply_cost(x, c, t, (2, 0), (), 'phase', out=out),
        'apply_cost[scale]': lambda x, out: backend.apply_cost(x, c, s, (2, 0), (), 'scale', out=out),
        'apply_pauli_axpby': lambda x, out: backend.apply_pauli_axpby(x, 0b0110, 0b0011, s, 1j * s, (), 'gate', out=out),
        'apply_pauli_rot': lambda x, out: backend.apply_pauli_rot(x, 0b0110, 0b0011, t, (), out=out),
        'apply_permutation': lambda x, out: backend.apply_permutation(x, torch.tensor([2, 0, 3, 1]), (2, 0), (), out=out),
        'apply_mux': lambda x, out: backend.apply_mux(x, u, 'u', 1, (2, 0), (), out=out),
    }


@pytest.mark.parametrize('name', list(wrappers()))
def test_wrappers_check_out_the_same_way_everywhere(cpu_backend, name):
    f = wrappers()[name]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, dtype=torch.complex128, generator=g)
    keep = x.clone()
    y = f(x, None)
    assert y is not x and y.data_ptr() != x.data_ptr() and y.shape == x.shape and y.dtype == x.dtype and torch.equal(x, keep)
    out = torch.empty_like(x)
    assert f(x, out) is out and torch.equal(out, y)
    for bad in (torch.zeros(2, 8, dtype=x.dtype), torch.zeros(2, 16, dtype=torch.complex64), torch.zeros(2, 32, dtype=x.dtype)[:, ::2]):
        with pytest.raises(ValueError, match='shape'):
            f(x, bad)
    flat = torch.zeros(40, dtype=torch.complex128)
    for a, b in ((flat[:32], flat[8:]), (flat[8:], flat[:32])):         # shifted by 8 amplitudes inside one storage
        with pytest.raises(ValueError, match='overlaps'):
            f(a.reshape(2, 16), b.reshape(2, 16))
    assert not flat.any() and torch.equal(x, keep)                      # a refusal writes nothing
    if name == 'apply_permutation':
        with pytest.raises(ValueError, match='out of place'):
            f(x, x)
        assert torch.equal(x, keep)
    else:
        assert f(x, x) is x and torch.equal(x, y)


def test_slices(monkeypatch):
    assert backend.MAX_BATCH == 32768
    for b in (1, 2, 3, 32768, 32769, 65538):
        assert list(backend._slices(b)) == [(lo, min(lo + backend.MAX_BATCH, b)) for lo in range(0, b, backend.MAX_BATCH)]
    assert list(backend._slices(0)) == []
    assert list(backend._slices(32768)) == [(0, 32768)]
    assert list(backend._slices(32769)) == [(0, 32768), (32768, 32769)]
    assert list(backend._slices(65538)) == [(0, 32768), (32768, 65536), (65536, 65538)]
    assert list(backend._slices(65538, 65535)) == [(0, 65535), (65535, 65538)]             # marginal, sample_indices
    monkeypatch.setattr(backend, 'MAX_BATCH', 2)                        # read when called, not when defined
    assert list(backend._slices(5)) == [(0, 2), (2, 4), (4, 5)]
    for b in (1, 2, 3):
        assert list(backend._slices(b)) == [(lo, min(lo + 2, b)) for lo in range(0, b, 2)]
    assert list(backend._slices(5, 65535)) == [(0, 5)]


def test_finish_table_refuses_a_table_that_requires_grad(cpu_backend):
    x = torch.zeros(1, 4, dtype=torch.complex64)
    tab = torch.ones(2, dtype=torch.float64)
    got = backend._finish_table(tab, x, torch.float32, 'here')
    assert got.dtype == torch.float32 and got.is_contiguous() and got.device == x.device
    lazy = torch.ones(2, dtype=torch.complex128).conj()
    assert lazy.is_conj() and not backend._finish_table(lazy, x, torch.complex64, 'here').is_conj()
    with pytest.raises(ValueError, match='here: the table is a constant'):
        backend._finish_table(tab.clone().requires_grad_(), x, torch.float32, 'here')
