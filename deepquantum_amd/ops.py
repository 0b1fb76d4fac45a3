"""Autograd-aware wrappers around the HIP kernels.

The reference differentiates its dense path with stock autograd through permute/reshape/matmul/cat
(SURVEY section 3C).  Here every gate application is one ``torch.autograd.Function`` whose backward is
again a gate kernel (``U^dagger`` applied to the cotangent) plus a small reduction for the matrix
gradient, so ``loss.backward()`` through ``QubitCircuit`` works unchanged while every sweep over the
state stays a single HBM-bound HIP launch.

Every backward here is itself written with differentiable operations of this module (the matrix gradient is the
``_GateGrad`` node, whose own backward is two gate applications; the cotangent of an expectation value is a gate
application), so ``create_graph=True`` -- ``torch.autograd.functional.hessian`` over a circuit, which the reference
gets from stock autograd (examples/benchmarks/gradient_benchmark.py:147-163) -- differentiates to any order.
"""

from __future__ import annotations

import dataclasses
from typing import Callable, Sequence

import torch

from torch.autograd import forward_ad as _fwad

from . import _functorch, backend


def _is_batched(t: torch.Tensor) -> bool:
    """True inside a ``torch.vmap`` transform (the tensor is a functorch BatchedTensor)."""
    return _functorch.is_batched(t)


#: PyTorch releases the probes below were checked against (tests/test_api_cpu.py::test_functorch_probes_are_guarded names
#: them too).  They read functorch's interpreter stack through private modules; on a release where those moved, the
#: probes answer "unknown" and every caller takes its conservative route (per-gate nodes, no refusal).
FUNCTORCH_PROBES_CHECKED_ON = _functorch.CHECKED_ON


def transform_stack() -> list[str] | None:
    """The ``torch.func`` transforms this call runs under, outermost first, as 'Vmap' / 'Grad' / 'Jvp' / ... -- or None
    when this PyTorch does not let us look (the private interpreter stack moved)."""
    return _functorch.transform_stack()


def forward_ad_active() -> bool | None:
    """True inside a ``torch.autograd.forward_ad.dual_level()`` (None: cannot tell)."""
    try:
        return _fwad._current_level >= 0
    except Exception:           # noqa: BLE001
        return None


def _single_forward_level() -> None:
    """Called by every ``jvp`` rule.  Forward over forward (``jacfwd(jacfwd(f))``, a ``jvp`` inside a ``jvp``) through ANY
    ``autograd.Function`` gives silently wrong numbers in this PyTorch (2.10: the tensors a rule saved for forward mode
    lose the outer level's tangents -- a two-line Function that multiplies shows it), so it is refused by name; forward
    over reverse (``torch.func.hessian``), reverse over forward and reverse over reverse are right.  (Where the
    interpreter stack cannot be read the rule goes ahead: the refusal is a courtesy, not a correctness device.)"""
    stack = transform_stack()
    if stack is not None and sum(t == 'Jvp' for t in stack) >= 2:
        raise RuntimeError('deepquantum_amd: nested forward-mode differentiation (jacfwd(jacfwd(f)), jvp inside jvp) through '
                           'autograd.Function nodes is not reliable in this PyTorch; use torch.func.hessian(f) (forward over '
                           'reverse) or torch.func.jacrev(torch.func.jacrev(f)) instead.')


def _plain(t: torch.Tensor) -> torch.Tensor:
    """The tensor with no pending conjugation / negation (cotangents that passed through ``conj()`` or ``.real`` of a
    forward-mode rule carry them lazily): what a kernel may read through a raw pointer.  Free when there is none."""
    return t.resolve_conj().resolve_neg()


def _kernel_arg(t: torch.Tensor) -> torch.Tensor:
    """A state or a cotangent as the streaming kernels (diagonal, Pauli, excitation, permutation, multiplexer) read it:
    :func:`_plain`, and 16-byte aligned.  Their entry points move 16-byte vectors and refuse any other pointer before a
    launch; autograd produces such tensors on its own -- the backward of ``cat([h, y.reshape(-1)])`` hands the node that
    made y a contiguous complex64 cotangent at element offset 1, 8 bytes off -- and nobody can ``clone()`` a cotangent, so a
    misaligned tensor is copied here, as ``backend._finish_table`` copies a misaligned table.  Every forward of the
    streaming nodes passes its states through this, and every backward, jvp and vmap rule is written with those nodes:
    the one place.  Free (one pointer test) for what an allocator returns."""
    t = _plain(t)
    return t.clone() if t.data_ptr() % 16 else t


def _is_wrapped(t: torch.Tensor | None) -> bool:
    """True inside any ``torch.func`` transform (vmap, grad, vjp, jacrev, jvp ...): the tensor is a functorch wrapper -- no
    data pointer, and only the per-gate nodes (``setup_context`` style, with ``vmap`` and ``jvp`` rules) may see it.  Also
    True for a dual tensor of plain forward-mode AD (``torch.autograd.forward_ad``): a raw kernel would drop its tangent."""
    if t is None:
        return False
    if _functorch.is_wrapped_tensor(t):
        return True
    if forward_ad_active() is False:
        return False
    return _fwad.unpack_dual(t).tangent is not None


def _polar_scale(ref: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """Per-sample factor s (a constant: detached) that brings ``d`` to the size of ``ref``, for the forward-mode rules
    that get a bilinear quantity by polarisation, f(ref + s d) - f(ref - s d) = 4 s Re <ref| . |d>: taken with s = 1 the
    difference of two quadratics cancels catastrophically when |d| << |ref| (complex64: a tangent scaled by 1e-7 came
    back 49 % off); with |s d| = |ref| the round-off is that of one reduction, relative to |ref| |d|, whatever the
    tangent's scale -- a JVP has to be linear in its tangent."""
    with torch.no_grad():
        nr = torch.linalg.vector_norm(ref.detach(), dim=-1, keepdim=True)
        nd = torch.linalg.vector_norm(d.detach(), dim=-1, keepdim=True)
        ok = (nd > 0) & (nr > 0)
        return torch.where(ok, nr / torch.where(ok, nd, torch.ones_like(nd)), torch.ones_like(nd))


def _jvp_two_slots(fn, x0, x1, t0, t1):
    """The tangent of ``fn(x0, x1)`` for an ``fn`` that is linear (or anti-linear) in each of its two slots: the function
    itself with one slot replaced by its tangent, ``fn(t0, x1) + fn(x0, t1)``; a tangent that is None is left out."""
    out = None
    if t0 is not None:
        out = fn(t0, x1)
    if t1 is not None:
        term = fn(x0, t1)
        out = term if out is None else out + term
    return out


class _ApplyGate(torch.autograd.Function):
    """y = (U on targets | controls) x  for x: (B, 2**n), U: (Bm, D, D).

    Written in the ``setup_context`` style so that it composes with ``torch.func`` transforms; the
    ``vmap`` rule folds the mapped dimension into the kernels' batch dimension (per-sample matrix stride),
    which is what lets ``torch.vmap`` over a circuit -- the reference's batching mechanism,
    circuit.py:232-240 -- run on the same kernels."""

    @staticmethod
    def forward(state: torch.Tensor, mats: torch.Tensor, targets: tuple, controls: tuple) -> torch.Tensor:
        return backend.apply_gate(_plain(state), _plain(mats), targets, controls)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, mats, targets, controls = inputs
        ctx.targets, ctx.controls = targets, controls
        ctx.save_for_backward(state, mats)
        ctx.save_for_forward(state, mats)

    @staticmethod
    def jvp(ctx, state_t, mats_t, _targets_t, _controls_t):
        _single_forward_level()
        # forward mode (torch.func.jvp / jacfwd / hessian): d(U x) = U dx + dU x, the second term on the controlled
        # subspace only -- two gate applications
        state, mats = ctx.saved_tensors
        out = None
        if state_t is not None:
            out = apply_gate(state_t, mats, ctx.targets, ctx.controls)
        if mats_t is not None:
            term = apply_masked(state, mats_t, ctx.targets, ctx.controls)
            out = term if out is None else out + term
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        state, mats = ctx.saved_tensors
        gy = gy.contiguous()
        gstate = gmats = None
        if ctx.needs_input_grad[0]:
            # d/dx of y = U x  ->  U^H gy on the same targets / controls (other amplitudes: identity)
            gstate = apply_gate(gy, mats.mH.resolve_conj().contiguous(), ctx.targets, ctx.controls)
        if ctx.needs_input_grad[1]:
            g = gate_grad(state, gy, ctx.targets, ctx.controls)  # (B, D, D) complex128; a node of its own
            if mats.shape[0] == 1 and g.shape[0] > 1:
                g = g.sum(dim=0, keepdim=True)
            gmats = g.to(mats.dtype)
        return gstate, gmats, None, None

    @staticmethod
    def vmap(info, in_dims, state, mats, targets, controls):
        sd, md = in_dims[0], in_dims[1]
        v = info.batch_size
        state = state.movedim(sd, 0) if sd is not None else state.unsqueeze(0).expand(v, *state.shape)
        b = state.shape[1]
        if md is not None:
            mats = mats.movedim(md, 0)
            d = mats.shape[-1]
            mats = mats.expand(v, b, d, d).reshape(v * b, d, d)
        elif mats.shape[0] > 1:
            mats = mats.unsqueeze(0).expand(v, *mats.shape).reshape(v * b, *mats.shape[1:])
        out = _ApplyGate.apply(state.reshape(v * b, -1).contiguous(), mats.resolve_conj().contiguous(), targets, controls)
        return out.reshape(v, b, -1), 0


def apply_gate(
    state: torch.Tensor, mats: torch.Tensor, targets: Sequence[int], controls: Sequence[int] = ()
) -> torch.Tensor:
    """Differentiable single-gate application on a contiguous (B, 2**n) state.

    ``mats`` is (D, D) or (Bm, D, D) with Bm in {1, B}; it is cast to the state's dtype (the reference
    multiplies a matrix and a state of the same dtype because ``.to()`` converts both,
    operation.py:156-169)."""
    if mats.ndim == 2:
        mats = mats.unsqueeze(0)
    if mats.dtype != state.dtype:
        mats = mats.to(state.dtype)
    if not _is_batched(state) and not state.is_contiguous():
        state = state.contiguous()
    return _ApplyGate.apply(state, mats, tuple(int(t) for t in targets), tuple(int(c) for c in controls))


def apply_masked(
    state: torch.Tensor, mats: torch.Tensor, targets: Sequence[int], controls: Sequence[int] = ()
) -> torch.Tensor:
    """``mats`` applied on the amplitudes whose control bits are all set, ZERO elsewhere (a controlled gate leaves
    those alone instead): P_c (M on targets) x.  Differentiable.  With controls it is the difference of two controlled
    applications -- (x + P_c (M - 1) x) - (x - P_c x) -- exact in floating point: outside the controlled subspace both
    terms are x itself, inside the second one is 0."""
    if not controls:
        return apply_gate(state, mats, targets, ())
    return apply_gate(state, mats, targets, controls) - apply_gate(state, torch.zeros_like(mats), targets, controls)


class _GateGrad(torch.autograd.Function):
    """G[b] = sum over the controlled amplitude groups of gy (outer) conj(x): (B, D, D) complex128 -- the matrix
    cotangent of ``_ApplyGate`` (one read of both states, ``dq_gate_grad_*``).  G is linear in gy and anti-linear in
    x, so its own backward is two masked gate applications: the cotangent of gy is (gG on targets) x, the cotangent
    of x is (gG^H on targets) gy, both on the controlled subspace only."""

    @staticmethod
    def forward(x: torch.Tensor, gy: torch.Tensor, targets: tuple, controls: tuple) -> torch.Tensor:
        return backend.gate_grad(_plain(x), _plain(gy), targets, controls)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, gy, ctx.targets, ctx.controls = inputs
        ctx.save_for_backward(x, gy)
        ctx.save_for_forward(x, gy)

    @staticmethod
    def jvp(ctx, x_t, gy_t, _targets_t, _controls_t):
        _single_forward_level()
        x, gy = ctx.saved_tensors           # G is linear in gy and anti-linear in x
        return _jvp_two_slots(lambda u, v: gate_grad(u, v, ctx.targets, ctx.controls), x, gy, x_t, gy_t)

    @staticmethod
    def backward(ctx, gg: torch.Tensor):
        x, gy = ctx.saved_tensors
        gx = ggy = None
        m = gg.to(x.dtype)
        if ctx.needs_input_grad[0]:
            gx = apply_masked(gy, m.mH.resolve_conj().contiguous(), ctx.targets, ctx.controls)
        if ctx.needs_input_grad[1]:
            ggy = apply_masked(x, m.contiguous(), ctx.targets, ctx.controls)
        return gx, ggy, None, None

    @staticmethod
    def vmap(info, in_dims, x, gy, targets, controls):
        v = info.batch_size
        x = x.movedim(in_dims[0], 0) if in_dims[0] is not None else x.unsqueeze(0).expand(v, *x.shape)
        gy = gy.movedim(in_dims[1], 0) if in_dims[1] is not None else gy.unsqueeze(0).expand(v, *gy.shape)
        b = x.shape[1]
        out = _GateGrad.apply(x.reshape(v * b, -1).contiguous(), gy.reshape(v * b, -1).contiguous(), targets, controls)
        return out.reshape(v, b, *out.shape[1:]), 0


def gate_grad(
    x: torch.Tensor, gy: torch.Tensor, targets: Sequence[int], controls: Sequence[int] = ()
) -> torch.Tensor:
    """Differentiable sum gy (outer) conj(x) over the amplitude groups of a gate: complex128 (B, D, D)."""
    if not _is_batched(x) and not x.is_contiguous():
        x = x.contiguous()
    if not _is_batched(gy) and not gy.is_contiguous():
        gy = gy.contiguous()
    return _GateGrad.apply(x, gy, tuple(int(t) for t in targets), tuple(int(c) for c in controls))


class _ExpectPauli(torch.autograd.Function):
    """Re <psi|P|psi> per batch sample, P a Pauli string given by bit masks."""

    @staticmethod
    def forward(state: torch.Tensor, xmask: int, zmask: int) -> torch.Tensor:
        return backend.expect_pauli(_plain(state), xmask, zmask).to(state.real.dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, ctx.xmask, ctx.zmask = inputs
        ctx.save_for_backward(state)
        ctx.save_for_forward(state)

    @staticmethod
    def jvp(ctx, state_t, _xmask_t, _zmask_t):
        _single_forward_level()
        (state,) = ctx.saved_tensors        # d Re<psi|P|psi> = 2 Re <P psi|d psi>
        ppsi = apply_pauli(state, ctx.xmask, ctx.zmask, differentiable=True)
        return (2.0 * (ppsi.conj() * state_t).sum(dim=-1).real).to(state.real.dtype)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        (state,) = ctx.saved_tensors
        # L = psi^H P psi with P Hermitian: dL/d(conj psi) = P psi; PyTorch's convention for a real loss
        # of a complex tensor is grad = 2 * dL/d(conj psi).
        # (P psi through the differentiable gate applications, so that a second derivative sees it)
        # (under create_graph only; a first-order backward takes all factors in one fused pass)
        legacy = _functorch.is_legacy_batched
        if (not torch.is_grad_enabled() and state.ndim == 2 and not _is_batched(state) and not _is_wrapped(g)
                and not _is_wrapped(state) and not legacy(g) and not legacy(state) and _functorch.no_transforms()):
            return apply_pauli(state, ctx.xmask, ctx.zmask, scale=2.0 * g), None, None
        ppsi = apply_pauli(state, ctx.xmask, ctx.zmask, differentiable=torch.is_grad_enabled())
        return (2.0 * g).to(state.real.dtype).unsqueeze(-1) * ppsi, None, None

    @staticmethod
    def vmap(info, in_dims, state, xmask, zmask):
        v = info.batch_size
        state = state.movedim(in_dims[0], 0)
        b = state.shape[1]
        out = _ExpectPauli.apply(state.reshape(v * b, -1).contiguous(), xmask, zmask)
        return out.reshape(v, b), 0


_PAULI = {}


def _pauli_mats(dtype: torch.dtype, device: torch.device) -> dict[str, torch.Tensor]:
    key = (dtype, device)
    if key not in _PAULI:
        _PAULI[key] = {
            'x': torch.tensor([[0, 1], [1, 0]], dtype=dtype, device=device),
            'y': torch.tensor([[0, -1j], [1j, 0]], dtype=dtype, device=device),
            'z': torch.tensor([[1, 0], [0, -1]], dtype=dtype, device=device),
        }
    return _PAULI[key]


def apply_pauli(state: torch.Tensor, xmask: int, zmask: int, differentiable: bool = False,
                scale: torch.Tensor | None = None) -> torch.Tensor:
    """P|psi> for a Pauli string (``differentiable``: through the autograd-aware gate applications).  ``scale`` (real, one
    number per sample; not with ``differentiable``): s P|psi> -- the factor rides on the matrix of the first Pauli instead
    of costing a read and a write of the state of its own (the cotangent 2 g P psi of an expectation value)."""
    mats = _pauli_mats(state.dtype, state.device)
    n = state.shape[-1].bit_length() - 1
    factors = [(p, 'y' if (xmask >> p) & (zmask >> p) & 1 else ('x' if (xmask >> p) & 1 else 'z'))
               for p in range(n) if ((xmask | zmask) >> p) & 1]
    if scale is not None:
        assert not differentiable and state.ndim == 2 and not _is_batched(state)
        if not factors:
            return state * scale.to(state.real.dtype).reshape(-1, 1)
        from . import executor

        s_ = scale.to(state.real.dtype).reshape(-1, 1, 1)
        kinds = {'x': 'gen', 'y': 'gen', 'z': 'diag'}          # (a scaled X is no bit flip any more)
        first = mats[factors[0][1]] * s_                         # (B, 2, 2), or (1, 2, 2)
        prims = [executor.Prim(kinds[factors[0][1]], first if first.shape[0] > 1 else first[0], (factors[0][0],), (), unitary=False)]
        prims += [executor.Prim({'x': 'x', 'y': 'gen', 'z': 'diag'}[c], mats[c], (p,), ()) for p, c in factors[1:]]
        with torch.no_grad():
            return executor.run(state.detach(), prims)
    if not differentiable and len(factors) >= 2 and not _is_batched(state) and state.ndim == 2:
        # all factors in one fused pass (the reference applies them one after the other, qmath.py:846-856: a read and a
        # write of the state EACH -- <X..X> on n qubits, the observable of its own gradient benchmark, cost n of them)
        from . import executor

        kinds = {'x': 'x', 'y': 'gen', 'z': 'diag'}
        prims = [executor.Prim(kinds[c], mats[c], (p,), ()) for p, c in factors]
        with torch.no_grad():
            return executor.run(state.detach(), prims)
    out = state
    for p, c in factors:
        out = apply_gate(out, mats[c], [p], []) if differentiable else backend.apply_gate(out, mats[c], [p], [])
    return out if out is not state else state.clone()


def expect_pauli(state: torch.Tensor, xmask: int, zmask: int) -> torch.Tensor:
    """Differentiable Re <psi_b|P|psi_b>, real (B,) in the state's real precision."""
    if not _is_batched(state) and not state.is_contiguous():
        state = state.contiguous()
    return _ExpectPauli.apply(state, int(xmask), int(zmask))


class _Marginal(torch.autograd.Function):
    """p[b, k] = sum over amplitudes whose ``bits`` spell k of |psi_b|^2 (bits[0] = MSB of k)."""

    @staticmethod
    def forward(state: torch.Tensor, bits: tuple) -> torch.Tensor:
        return backend.marginal(_plain(state), bits).to(state.real.dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, ctx.bits = inputs
        ctx.save_for_backward(state)
        ctx.save_for_forward(state)

    @staticmethod
    def jvp(ctx, state_t, _bits_t):
        _single_forward_level()
        (state,) = ctx.saved_tensors        # by polarisation: |psi + s d|^2 - |psi - s d|^2 = 4 s Re conj(psi) d
        s = _polar_scale(state, state_t)    # (|s d| = |psi|: see `_polar_scale`)
        d = state_t * s
        return (marginal(state + d, ctx.bits) - marginal(state - d, ctx.bits)) * (0.5 / s)

    @staticmethod
    def vmap(info, in_dims, state, bits):
        v = info.batch_size
        state = state.movedim(in_dims[0], 0)
        b = state.shape[1]
        out = _Marginal.apply(state.reshape(v * b, -1).contiguous(), bits)
        return out.reshape(v, b, -1), 0

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        (state,) = ctx.saved_tensors
        # d p_k / d conj(psi_i) = psi_i [bits(i) = k]; real loss of a complex tensor: grad = 2 * that,
        # i.e. a diagonal "gate" diag(2 g[b, :]) on the measured bits
        diag = (2.0 * g).to(state.dtype).diag_embed()
        return apply_gate(state, diag.contiguous(), ctx.bits, ()), None


def marginal(state: torch.Tensor, bits: Sequence[int]) -> torch.Tensor:
    """Differentiable marginal distribution over ``bits`` of a contiguous (B, 2**n) state."""
    if not state.is_contiguous():
        state = state.contiguous()
    return _Marginal.apply(state, tuple(int(b) for b in bits))


class _ExpectZMulti(torch.autograd.Function):
    """Re <psi_b| Z-string_k |psi_b> for K Z-type strings: (B, K), one read of the state per 32 strings."""

    @staticmethod
    def forward(state: torch.Tensor, zmasks: tuple) -> torch.Tensor:
        return backend.expect_z_multi(_plain(state), zmasks).to(state.real.dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, ctx.zmasks = inputs
        ctx.save_for_backward(state)
        ctx.save_for_forward(state)

    @staticmethod
    def jvp(ctx, state_t, _zmasks_t):
        _single_forward_level()
        (state,) = ctx.saved_tensors        # P_k real diagonal: d <psi|P_k|psi> = 2 Re <psi|P_k|d psi>, by polarisation
        s = _polar_scale(state, state_t)    # (|s d| = |psi|: see `_polar_scale`)
        d = state_t * s
        return (expect_z_multi(state + d, ctx.zmasks) - expect_z_multi(state - d, ctx.zmasks)) * (0.5 / s)

    @staticmethod
    def vmap(info, in_dims, state, zmasks):
        v = info.batch_size
        state = state.movedim(in_dims[0], 0)
        b = state.shape[1]
        out = _ExpectZMulti.apply(state.reshape(v * b, -1).contiguous(), zmasks)
        return out.reshape(v, b, -1), 0

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        (state,) = ctx.saved_tensors
        # L = sum_k g_k psi^H P_k psi with P_k diagonal: grad = 2 (sum_k g_k P_k) psi, one read + one write
        return scale_z_signs(state, ctx.zmasks, 2.0 * g), None


class _ScaleZSigns(torch.autograd.Function):
    """out[b, i] = (sum_k w[b, k] s_k(i)) psi[b, i] with s_k(i) = (-1)^popcount(i & zmask_k): the cotangent of
    ``_ExpectZMulti`` as a node of its own, so that second derivatives exist.  Linear in psi (real diagonal factor:
    its cotangent is the same scaling of the incoming cotangent) and in w (d/dw_k = Re <g| P_k |psi>, taken by
    polarisation from the Z-string reduction itself)."""

    @staticmethod
    def forward(state: torch.Tensor, zmasks: tuple, w: torch.Tensor) -> torch.Tensor:
        return backend.scale_z_signs(_plain(state), zmasks, w)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, ctx.zmasks, w = inputs
        ctx.save_for_backward(state, w)
        ctx.save_for_forward(state, w)

    @staticmethod
    def jvp(ctx, state_t, _zmasks_t, w_t):
        _single_forward_level()
        state, w = ctx.saved_tensors        # linear in psi and in w
        return _jvp_two_slots(lambda s, v: scale_z_signs(s, ctx.zmasks, v), state, w, state_t, w_t)

    @staticmethod
    def vmap(info, in_dims, state, zmasks, w):
        v = info.batch_size
        state = state.movedim(in_dims[0], 0) if in_dims[0] is not None else state.unsqueeze(0).expand(v, *state.shape)
        w = w.movedim(in_dims[2], 0) if in_dims[2] is not None else w.unsqueeze(0).expand(v, *w.shape)
        b = state.shape[1]
        out = _ScaleZSigns.apply(state.reshape(v * b, -1).contiguous(), zmasks, w.reshape(v * b, -1).contiguous())
        return out.reshape(v, b, -1), 0

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        state, w = ctx.saved_tensors
        g = g.contiguous()
        gstate = gw = None
        if ctx.needs_input_grad[0]:
            gstate = scale_z_signs(g, ctx.zmasks, w)
        if ctx.needs_input_grad[2]:
            # Re <g| P |psi> = (<s g + psi| P |s g + psi> - <s g - psi| P |s g - psi>) / (4 s), |s g| = |psi|
            s = _polar_scale(state, g)
            gs = g * s
            gw = ((expect_z_multi(gs + state, ctx.zmasks) - expect_z_multi(gs - state, ctx.zmasks)) * (0.25 / s)).to(w.dtype)
        return gstate, None, gw


def scale_z_signs(state: torch.Tensor, zmasks: Sequence[int], w: torch.Tensor) -> torch.Tensor:
    """Differentiable (sum_k w_k P_k) psi for Z-type strings P_k, w real (B, K)."""
    if not state.is_contiguous():
        state = state.contiguous()
    return _ScaleZSigns.apply(state, tuple(int(z) for z in zmasks), w)


def expect_z_multi(state: torch.Tensor, zmasks: Sequence[int]) -> torch.Tensor:
    """Differentiable expectation values of several Z-type Pauli strings at once: real (B, K)."""
    if not state.is_contiguous():
        state = state.contiguous()
    return _ExpectZMulti.apply(state, tuple(int(z) for z in zmasks))


def _fold(x: torch.Tensor, d: int | None, v: int) -> torch.Tensor:
    """The vmapped dimension of ``x`` (at ``d``; None: not mapped) folded into its batch dimension."""
    x = x.movedim(d, 0) if d is not None else x.unsqueeze(0).expand(v, *x.shape)
    return x.reshape(v * x.shape[1], *x.shape[2:]).contiguous()


def _vmap_states(cls, what: str, info, in_dims, args: tuple, folded: tuple = (), tables: tuple = ()):
    """The ``vmap`` rule of a state-to-state Function ``cls``: the mapped dimension of the state (``args[0]``) and of the
    per-sample arguments at ``folded`` goes into the batch dimension, the constant tables at ``tables`` must not be
    mapped, and the result is unfolded again."""
    for i in tables:
        _unmapped_table(in_dims[i], what)
    v = info.batch_size
    args = list(args)
    for i in (0, *folded):
        args[i] = _fold(args[i], in_dims[i], v)
    out = cls.apply(*args)
    return out.reshape(v, -1, out.shape[-1]), 0


def _vmap_cross(cls, what: str, info, in_dims, args: tuple, tables: tuple = ()):
    """The ``vmap`` rule of a cross Function ``cls(bra, ket, ...)``: as :func:`_vmap_states`, and a bra that is the ket
    mapped the same way stays the same tensor (one read of the state)."""
    for i in tables:
        _unmapped_table(in_dims[i], what)
    v = info.batch_size
    bra, ket = args[:2]
    kf = _fold(ket, in_dims[1], v)
    bf = kf if bra is ket and in_dims[0] == in_dims[1] else _fold(bra, in_dims[0], v)
    return cls.apply(bf, kf, *args[2:]).reshape(v, -1), 0


class _Rdm1Cross(torch.autograd.Function):
    """T[b, k, a, c] = sum_rest conj(bra[a on wire k, rest]) ket[c on wire k, rest]: complex128 (B, n, 2, 2), every wire
    at once (``dq_rdm1_cross_*``; bra and ket the same tensor: one read of the state per pass).  T is anti-linear in
    bra and linear in ket, so its cotangents are sums of one-wire operators: bra gets W(ket; conj(G)), ket gets
    W(bra; G^T) (per-wire transpose) -- ``_WireSum`` nodes, whose own backward is again this node: derivatives of any
    order."""

    @staticmethod
    def forward(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
        pk = _plain(ket)
        return backend.rdm1_cross(pk if bra is ket else _plain(bra), pk)

    @staticmethod
    def setup_context(ctx, inputs, output):
        bra, ket = inputs
        ctx.same = bra is ket
        ctx.save_for_backward(bra, ket)
        ctx.save_for_forward(bra, ket)

    @staticmethod
    def jvp(ctx, bra_t, ket_t):
        _single_forward_level()
        bra, ket = ctx.saved_tensors
        return _jvp_two_slots(rdm1_cross, bra, ket, bra_t, ket_t)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        bra, ket = ctx.saved_tensors
        g = g.to(torch.complex128)
        if ctx.same:                           # one sum of one-wire operators for both slots of the one tensor
            return wire_sum(ket, g.conj() + g.transpose(-1, -2)), None
        gbra = wire_sum(ket, g.conj()) if ctx.needs_input_grad[0] else None
        gket = wire_sum(bra, g.transpose(-1, -2)) if ctx.needs_input_grad[1] else None
        return gbra, gket

    @staticmethod
    def vmap(info, in_dims, bra, ket):
        v = info.batch_size
        same = bra is ket and in_dims[0] == in_dims[1]
        kf = _fold(ket, in_dims[1], v)
        bf = kf if same else _fold(bra, in_dims[0], v)
        out = _Rdm1Cross.apply(bf, kf)
        return out.reshape(v, -1, *out.shape[1:]), 0


class _WireSum(torch.autograd.Function):
    """W(psi; M) = sum_k (M_k on wire k) psi for M complex (B, n, 2, 2): the state's dtype (``dq_apply_wire_sum_*``).
    Linear in psi (cotangent: W(g; M^H), per-wire conjugate transpose) and in M (cotangent: T(psi, g)^T, the cross
    reduction)."""

    @staticmethod
    def forward(state: torch.Tensor, mats: torch.Tensor) -> torch.Tensor:
        return backend.apply_wire_sum(_plain(state), _plain(mats))

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, mats = inputs
        ctx.save_for_backward(state, mats)
        ctx.save_for_forward(state, mats)

    @staticmethod
    def jvp(ctx, state_t, mats_t):
        _single_forward_level()
        state, mats = ctx.saved_tensors
        return _jvp_two_slots(wire_sum, state, mats, state_t, mats_t)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        state, mats = ctx.saved_tensors
        gstate = gmats = None
        if ctx.needs_input_grad[0]:
            gstate = wire_sum(g, mats.mH)
        if ctx.needs_input_grad[1]:
            gmats = rdm1_cross(state, g).transpose(-1, -2).to(mats.dtype)
        return gstate, gmats

    @staticmethod
    def vmap(info, in_dims, state, mats):
        v = info.batch_size
        sf = _fold(state, in_dims[0], v)
        out = _WireSum.apply(sf, _fold(mats, in_dims[1], v))
        return out.reshape(v, -1, out.shape[-1]), 0


def _no_legacy(*ts: torch.Tensor) -> None:
    legacy = _functorch.is_legacy_batched
    if any(legacy(t) for t in ts):
        raise RuntimeError('deepquantum_amd: the entanglement reductions do not run under the legacy vmap of '
                           'torch.autograd.functional.jacobian / hessian(vectorize=True); use vectorize=False or '
                           'torch.func.jacrev / hessian')


def _flat_arg(x: torch.Tensor) -> torch.Tensor:
    return x if _is_batched(x) or x.is_contiguous() else x.contiguous()


def _cross_pair(bra: torch.Tensor, ket: torch.Tensor, what: str = '') -> tuple[torch.Tensor, torch.Tensor]:
    """What every public cross reduction does with its two states: no legacy vmap, one dtype (``what``: the function's
    name in front of the message), both flat -- and a bra that is the ket stays the same tensor (one read of the state)."""
    _no_legacy(bra, ket)
    if bra.dtype != ket.dtype:
        raise ValueError((what and what + ': ') + 'bra and ket must have one dtype')
    same = bra is ket
    ket = _flat_arg(ket)
    return (ket if same else _flat_arg(bra)), ket


def rdm1_cross(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """Differentiable one-body cross reduction of two (B, 2**n) states, complex128 (B, n, 2, 2), indexed by wire:
    ``rdm1_cross(psi, psi)[b, k].T`` is the reduced density matrix of wire k (pass the same tensor twice: one read)."""
    return _Rdm1Cross.apply(*_cross_pair(bra, ket))


def wire_sum(state: torch.Tensor, mats: torch.Tensor) -> torch.Tensor:
    """Differentiable sum of one-wire operators, ``sum_k (mats[:, k] on wire k) state`` for a (B, 2**n) state and
    complex (B, n, 2, 2) matrices indexed by wire."""
    _no_legacy(state, mats)
    if not mats.is_complex():
        mats = mats.to(torch.complex128)
    if not _is_batched(state) and not state.is_contiguous():
        state = state.contiguous()
    if not _is_batched(mats):
        mats = mats.resolve_conj().resolve_neg().contiguous()
    return _WireSum.apply(state, mats)


# ---- diagonal operators on any number of wires (csrc/dq_diag.hip) -------------------------------------------------------
# Three operations with a real table c over the index bits `bits` (sub(i): backend.apply_diag), closed under
# differentiation -- every backward and every jvp below is written with the other two -- so derivatives of any order
# exist by construction:
#     phase(x, c, t)[i] = exp(-i t c[sub(i)]) x[i]        (outside the controls: x[i])
#     cross(a, b, c)    = sum_i c[sub(i)] conj(a[i]) b[i] (outside the controls: left out)
#     scale(x, c, s)[i] = s c[sub(i)] x[i]                (outside the controls: 0)
# The tables are constants: they carry no gradient.
def _const_table(table: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(table, torch.Tensor):
        raise ValueError(f'{what}: the table must be a tensor, got {type(table).__name__}')
    if table.requires_grad:
        raise ValueError(f'{what}: the table is a constant -- gradients with respect to its entries are not supported; '
                         'detach() it')
    return table


def _unmapped_table(in_dim, what: str) -> None:
    if in_dim is not None:
        raise RuntimeError(f'deepquantum_amd: {what} under torch.vmap: the table must not be a mapped argument')


def _per_sample(p: torch.Tensor, batch: int, dtype: torch.dtype, what: str) -> torch.Tensor:
    """A 0-d, (1,) or (B,) parameter as (B,) in ``dtype`` (differentiably: a shared value gets the sum of the samples'
    gradients from ``expand``)."""
    p = p.to(dtype).reshape(-1)
    if p.shape[0] == 1 and batch != 1:
        p = p.expand(batch)
    if p.shape[0] != batch:
        raise ValueError(f'{what}: one parameter, or one per sample ({batch}), expected; got {p.shape[0]}')
    return p


class _CostPhase(torch.autograd.Function):
    """y = exp(-i t c) x with t real (B,): cotangents gx = phase(gy, c, -t) and gt = Im cross(gy, y, c) (dy/dt = -i c y on
    the controlled amplitudes, 0 elsewhere -- which cross leaves out)."""

    @staticmethod
    def forward(state: torch.Tensor, cost: torch.Tensor, t: torch.Tensor, bits: tuple, controls: tuple) -> torch.Tensor:
        return backend.apply_cost(_kernel_arg(state), cost, _plain(t), bits, controls, 'phase')

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, cost, t, ctx.bits, ctx.controls = inputs
        ctx.save_for_backward(state, cost, t)
        ctx.save_for_forward(state, cost, t)

    @staticmethod
    def jvp(ctx, state_t, _cost_t, t_t, _bits_t, _controls_t):
        _single_forward_level()
        state, cost, t = ctx.saved_tensors
        out = None
        if state_t is not None:
            out = cost_phase(state_t, cost, t, ctx.bits, ctx.controls)
        if t_t is not None:
            y = cost_phase(state, cost, t, ctx.bits, ctx.controls)
            term = cost_scale(y, cost, -1j * t_t.to(torch.complex128), ctx.bits, ctx.controls)
            out = term if out is None else out + term
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        state, cost, t = ctx.saved_tensors
        gstate = gt = None
        if ctx.needs_input_grad[0]:
            gstate = cost_phase(gy, cost, -t, ctx.bits, ctx.controls)
        if ctx.needs_input_grad[2]:
            y = cost_phase(state, cost, t, ctx.bits, ctx.controls)
            gt = cost_cross(gy, y, cost, ctx.bits, ctx.controls).imag.to(t.dtype)
        return gstate, None, gt, None, None

    @staticmethod
    def vmap(info, in_dims, state, cost, t, bits, controls):
        return _vmap_states(_CostPhase, 'cost_phase', info, in_dims, (state, cost, t, bits, controls), folded=(2,), tables=(1,))


class _CostCross(torch.autograd.Function):
    """z = sum_i c conj(a_i) b_i, complex128 (B,): anti-linear in a, linear in b; cotangents g_b = scale(a, c, gz) and
    g_a = scale(b, c, conj(gz))."""

    @staticmethod
    def forward(bra: torch.Tensor, ket: torch.Tensor, cost: torch.Tensor, bits: tuple, controls: tuple) -> torch.Tensor:
        pk = _kernel_arg(ket)
        return backend.cost_cross(pk if bra is ket else _kernel_arg(bra), pk, cost, bits, controls)

    @staticmethod
    def setup_context(ctx, inputs, output):
        bra, ket, cost, ctx.bits, ctx.controls = inputs
        ctx.save_for_backward(bra, ket, cost)
        ctx.save_for_forward(bra, ket, cost)

    @staticmethod
    def jvp(ctx, bra_t, ket_t, _cost_t, _bits_t, _controls_t):
        _single_forward_level()
        bra, ket, cost = ctx.saved_tensors
        return _jvp_two_slots(lambda u, v: cost_cross(u, v, cost, ctx.bits, ctx.controls), bra, ket, bra_t, ket_t)

    @staticmethod
    def backward(ctx, gz: torch.Tensor):
        bra, ket, cost = ctx.saved_tensors
        gz = gz.to(torch.complex128)
        gbra = cost_scale(ket, cost, gz.conj(), ctx.bits, ctx.controls) if ctx.needs_input_grad[0] else None
        gket = cost_scale(bra, cost, gz, ctx.bits, ctx.controls) if ctx.needs_input_grad[1] else None
        return gbra, gket, None, None, None

    @staticmethod
    def vmap(info, in_dims, bra, ket, cost, bits, controls):
        return _vmap_cross(_CostCross, 'cost_cross', info, in_dims, (bra, ket, cost, bits, controls), tables=(2,))


class _CostScale(torch.autograd.Function):
    """y = s c x with s complex128 (B,), 0 outside the controls: cotangents gx = scale(gy, c, conj(s)) and
    gs = cross(x, gy, c)."""

    @staticmethod
    def forward(state: torch.Tensor, cost: torch.Tensor, s: torch.Tensor, bits: tuple, controls: tuple) -> torch.Tensor:
        return backend.apply_cost(_kernel_arg(state), cost, _plain(s), bits, controls, 'scale')

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, cost, s, ctx.bits, ctx.controls = inputs
        ctx.save_for_backward(state, cost, s)
        ctx.save_for_forward(state, cost, s)

    @staticmethod
    def jvp(ctx, state_t, _cost_t, s_t, _bits_t, _controls_t):
        _single_forward_level()
        state, cost, s = ctx.saved_tensors
        return _jvp_two_slots(lambda x, v: cost_scale(x, cost, v, ctx.bits, ctx.controls), state, s, state_t, s_t)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        state, cost, s = ctx.saved_tensors
        gstate = gs = None
        if ctx.needs_input_grad[0]:
            gstate = cost_scale(gy, cost, s.conj(), ctx.bits, ctx.controls)
        if ctx.needs_input_grad[2]:
            gs = cost_cross(state, gy, cost, ctx.bits, ctx.controls).to(s.dtype)
        return gstate, None, gs, None, None

    @staticmethod
    def vmap(info, in_dims, state, cost, s, bits, controls):
        return _vmap_states(_CostScale, 'cost_scale', info, in_dims, (state, cost, s, bits, controls), folded=(2,), tables=(1,))


class _DiagMul(torch.autograd.Function):
    """y = d[sub(i)] x with a complex table d, (2^k,) or one per sample (B, 2^k): linear in x, cotangent
    gx = diag_mul(gy, conj(d))."""

    @staticmethod
    def forward(state: torch.Tensor, diag: torch.Tensor, bits: tuple, controls: tuple) -> torch.Tensor:
        return backend.apply_diag(_kernel_arg(state), _plain(diag), bits, controls)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _state, diag, ctx.bits, ctx.controls = inputs
        ctx.save_for_backward(diag)
        ctx.save_for_forward(diag)

    @staticmethod
    def jvp(ctx, state_t, _diag_t, _bits_t, _controls_t):
        _single_forward_level()
        (diag,) = ctx.saved_tensors
        return diag_mul(state_t, diag, ctx.bits, ctx.controls)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        (diag,) = ctx.saved_tensors
        return diag_mul(gy, diag.conj(), ctx.bits, ctx.controls), None, None, None

    @staticmethod
    def vmap(info, in_dims, state, diag, bits, controls):
        if in_dims[1] is None and diag.ndim == 2 and diag.shape[0] > 1:         # one table per sample: per folded sample
            diag = diag.unsqueeze(0).expand(info.batch_size, *diag.shape).reshape(-1, diag.shape[-1])
        return _vmap_states(_DiagMul, 'diag_mul', info, in_dims, (state, diag, bits, controls), tables=(1,))


def _bit_args(bits: Sequence[int], controls: Sequence[int]) -> tuple[tuple, tuple]:
    return tuple(int(b) for b in bits), tuple(int(c) for c in controls)


def cost_phase(state: torch.Tensor, cost: torch.Tensor, t: torch.Tensor, bits: Sequence[int],
               controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable ``exp(-i t diag(cost))`` on a (B, 2**n) state: ``cost`` a constant real table (2^k,) over the index
    bits ``bits`` (``bits[0]`` = its most significant bit), ``t`` real, one value or one per sample.  One read and one
    write of the state whatever k is.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(state, t)
    cost = _const_table(cost, 'cost_phase')
    bits, controls = _bit_args(bits, controls)
    t = _per_sample(t, state.shape[-2], torch.float64, 'cost_phase')
    return _CostPhase.apply(_flat_arg(state), cost, t, bits, controls)


def cost_cross(bra: torch.Tensor, ket: torch.Tensor, cost: torch.Tensor, bits: Sequence[int],
               controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable ``sum_i cost[sub(i)] conj(bra_i) ket_i`` of two (B, 2**n) states: complex128 (B,).  Pass the same
    tensor twice for ``<C>`` (one read of the state; the imaginary part is exactly 0).
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    bra, ket = _cross_pair(bra, ket, 'cost_cross')
    cost = _const_table(cost, 'cost_cross')
    bits, controls = _bit_args(bits, controls)
    return _CostCross.apply(bra, ket, cost, bits, controls)


def cost_scale(state: torch.Tensor, cost: torch.Tensor, s: torch.Tensor, bits: Sequence[int],
               controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable ``s diag(cost)`` on a (B, 2**n) state, ``s`` complex, one value or one per sample; amplitudes
    outside the controls come out as 0 (the cotangent of :func:`cost_cross`).
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(state, s)
    cost = _const_table(cost, 'cost_scale')
    bits, controls = _bit_args(bits, controls)
    s = _per_sample(s, state.shape[-2], torch.complex128, 'cost_scale')
    return _CostScale.apply(_flat_arg(state), cost, s, bits, controls)


def diag_mul(state: torch.Tensor, diag: torch.Tensor, bits: Sequence[int], controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable (in the state) diagonal operator: ``diag`` a constant complex table (2^k,) or (B, 2^k) over the
    index bits ``bits``; amplitudes outside the controls pass through.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(state)
    diag = _const_table(diag, 'diag_mul')
    bits, controls = _bit_args(bits, controls)
    return _DiagMul.apply(_flat_arg(state), diag, bits, controls)


# ---- a generator on its support: Pauli strings (csrc/dq_pauli.hip) and excitations (csrc/dq_excite.hip) -----------------
# A family is a linear map G that acts on a support S of the index space -- the amplitudes inside the controls, or the
# pairs of an excitation -- and is 0 elsewhere, with G^dagger = s G, s = +1 or -1.  A spec names one G of the family.  Two
# operations closed under differentiation -- every backward and every jvp below is written with them -- so derivatives of
# any order exist by construction, and the rotation as a node of its own on top of them:
#     axpby(x; a, c)[i] = a x[i] + c (G x)[i] on S        (elsewhere: x[i] in 'gate' mode, 0 in 'map' mode)
#     cross(u, v)       = sum_i conj(u[i]) (G v)[i]       (which is a sum over S)
#     rot(x; theta)     = exp(r theta G) x = axpby(x; alpha(theta), beta(theta)) in 'gate' mode, theta real
# The rules, for a, c, the cotangent gz of cross complex128 (B,) and theta real (B,):
#     axpby:  gx = axpby(gy; conj a, s conj c) in the same mode;  gc = <G x, gy> = s cross(x, gy);  ga = the inner product
#             <x, gy> over S, which the family says how to get (`inner`).  A tangent in a or c moves S only: a 'map' term.
#     cross:  anti-linear in u, linear in v:  g_u = map(v; 0, conj gz),  g_v = G^dagger u gz = map(u; 0, s gz).
#     rot:    y = U x with U^dagger = rot(-theta):  gx = rot(gy; -theta);  dy/dtheta = r G y on S and 0 elsewhere -- a 'map'
#             term of y -- so gtheta = Re(conj(r) cross(gy, y)).  U is a function of G and commutes with it, so
#             cross(gy, U x) = cross(U^dagger gy, x) = cross(gx, x): the cross takes the two tensors the backward holds
#             already and y is not formed again -- one rotation and one cross per backward.
# A family supplies, besides its name and its three backend functions, the four facts the rules leave open: s, `inner`,
# r (`rate`, applied to the angle's tangent) and the read-out of gtheta (`gtheta`, in the family's own arithmetic).
@dataclasses.dataclass(frozen=True, eq=False)
class _Generator:
    """What differs between the families.  The nodes take it as a non-tensor argument with the hashable spec, as ONE pair
    ``gen = (family, spec)``: every positional argument of an ``autograd.Function`` costs about two microseconds per call
    (its signature is bound anew each time), and a rotation forward plus backward is three such calls."""

    name: str           # 'pauli' / 'excite': '<name>_axpby', '<name>_cross', '<name>_rot' in error and vmap messages
    sign: int           # s: G^dagger = s G
    axpby: str          # the names of the three functions of `backend`, looked up there at call time (tests wrap them)
    cross: str
    rot: str | None     # (None, as `rate` and `gtheta`: a family without a rotation)
    spread: Callable    # spec -> (leading, trailing): backend.f(<states>, *leading, <parameters>, *trailing[, mode])
    inner: Callable     # (gen, x, gy, like) -> <x, gy> over the support, complex128 (B,), like ``like``
    rate: Callable | None       # theta_t -> r theta_t, complex128
    gtheta: Callable | None     # cross(gx, x) -> gtheta, real
    rot_tail: Callable = lambda spec: ()        # spec -> what `rot` alone takes after everything else (a tolerance)

    def adjoint(self, t: torch.Tensor) -> torch.Tensor:
        """s t"""
        return t if self.sign > 0 else -t


class _GenAxpby(torch.autograd.Function):
    """y = a x + c G x with a, c complex128 (B,): see the rules above."""

    @staticmethod
    def forward(state: torch.Tensor, a: torch.Tensor, c: torch.Tensor, gen: tuple, mode: str) -> torch.Tensor:
        fam, spec = gen
        leading, trailing = fam.spread(spec)
        return getattr(backend, fam.axpby)(_kernel_arg(state), *leading, _plain(a), _plain(c), *trailing, mode)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, a, c, ctx.gen, ctx.mode = inputs
        ctx.save_for_backward(state, a, c)
        ctx.save_for_forward(state, a, c)

    @staticmethod
    def jvp(ctx, state_t, a_t, c_t, *_):
        _single_forward_level()
        state, a, c = ctx.saved_tensors
        out = None
        if state_t is not None:
            out = _gen_axpby(ctx.gen, state_t, a, c, ctx.mode)
        if a_t is not None or c_t is not None:
            zero = torch.zeros_like(a)
            term = _gen_axpby(ctx.gen, state, zero if a_t is None else a_t, zero if c_t is None else c_t, 'map')
            out = term if out is None else out + term
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        gen = ctx.gen
        fam = gen[0]
        state, a, c = ctx.saved_tensors
        gstate = ga = gc = None
        if ctx.needs_input_grad[0]:
            gstate = _gen_axpby(gen, gy, a.conj(), fam.adjoint(c.conj()), ctx.mode)
        if ctx.needs_input_grad[1]:
            ga = fam.inner(gen, state, gy, a).to(a.dtype)
        if ctx.needs_input_grad[2]:
            gc = fam.adjoint(_gen_cross(gen, state, gy)).to(c.dtype)
        return gstate, ga, gc, None, None

    @staticmethod
    def vmap(info, in_dims, state, a, c, gen, mode):
        return _vmap_states(_GenAxpby, gen[0].name + '_axpby', info, in_dims, (state, a, c, gen, mode), folded=(1, 2))


class _GenCross(torch.autograd.Function):
    """z = sum_i conj(u_i) (G v)_i, complex128 (B,): see the rules above."""

    @staticmethod
    def forward(bra: torch.Tensor, ket: torch.Tensor, gen: tuple) -> torch.Tensor:
        fam, spec = gen
        pk = _kernel_arg(ket)
        leading, trailing = fam.spread(spec)
        return getattr(backend, fam.cross)(pk if bra is ket else _kernel_arg(bra), pk, *leading, *trailing)

    @staticmethod
    def setup_context(ctx, inputs, output):
        bra, ket, ctx.gen = inputs
        ctx.save_for_backward(bra, ket)
        ctx.save_for_forward(bra, ket)

    @staticmethod
    def jvp(ctx, bra_t, ket_t, *_):
        _single_forward_level()
        bra, ket = ctx.saved_tensors
        return _jvp_two_slots(lambda u, v: _gen_cross(ctx.gen, u, v), bra, ket, bra_t, ket_t)

    @staticmethod
    def backward(ctx, gz: torch.Tensor):
        gen = ctx.gen
        bra, ket = ctx.saved_tensors
        gz = gz.to(torch.complex128)
        zero = torch.zeros_like(gz)
        gbra = gket = None
        if ctx.needs_input_grad[0]:
            gbra = _gen_axpby(gen, ket, zero, gz.conj(), 'map')
        if ctx.needs_input_grad[1]:
            gket = _gen_axpby(gen, bra, zero, gen[0].adjoint(gz), 'map')
        return gbra, gket, None

    @staticmethod
    def vmap(info, in_dims, bra, ket, gen):
        return _vmap_cross(_GenCross, gen[0].name + '_cross', info, in_dims, (bra, ket, gen))


class _GenRot(torch.autograd.Function):
    """y = exp(r theta G) x, theta real (B,): see the rules above -- one rotation and one cross per backward."""

    @staticmethod
    def forward(state: torch.Tensor, theta: torch.Tensor, gen: tuple) -> torch.Tensor:
        fam, spec = gen
        leading, trailing = fam.spread(spec)
        return getattr(backend, fam.rot)(_kernel_arg(state), *leading, _plain(theta), *trailing, *fam.rot_tail(spec))

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, theta, ctx.gen = inputs
        ctx.save_for_backward(state, theta)
        ctx.save_for_forward(state, theta)

    @staticmethod
    def jvp(ctx, state_t, theta_t, *_):
        _single_forward_level()
        gen = ctx.gen
        state, theta = ctx.saved_tensors
        out = None
        if state_t is not None:
            out = _gen_rot(gen, state_t, theta)
        if theta_t is not None:
            y = _gen_rot(gen, state, theta)
            rate = gen[0].rate(theta_t)
            term = _gen_axpby(gen, y, torch.zeros_like(rate), rate, 'map')
            out = term if out is None else out + term
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        gen = ctx.gen
        state, theta = ctx.saved_tensors
        gstate = _gen_rot(gen, gy, -theta)
        gtheta = None
        if ctx.needs_input_grad[1]:
            gtheta = gen[0].gtheta(_gen_cross(gen, gstate, state)).to(theta.dtype)
        return (gstate if ctx.needs_input_grad[0] else None), gtheta, None

    @staticmethod
    def vmap(info, in_dims, state, theta, gen):
        return _vmap_states(_GenRot, gen[0].name + '_rot', info, in_dims, (state, theta, gen), folded=(1,))


def _sample_param(p, state: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
    if not isinstance(p, torch.Tensor):
        p = torch.as_tensor(p, device=state.device)
    return _per_sample(p, state.shape[-2], dtype, what)


# (the three operations of a generator ``gen = (family, spec)``, the spec in the form the nodes keep: what the public
# functions below and the rules above call)
def _gen_axpby(gen: tuple, state: torch.Tensor, a, c, mode: str) -> torch.Tensor:
    what = gen[0].name + '_axpby'
    _no_legacy(state)
    if mode not in ('gate', 'map'):
        raise ValueError(f"{what}: mode must be 'gate' or 'map', got {mode!r}")
    a = _sample_param(a, state, torch.complex128, what)
    c = _sample_param(c, state, torch.complex128, what)
    return _GenAxpby.apply(_flat_arg(state), a, c, gen, mode)


def _gen_cross(gen: tuple, bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    return _GenCross.apply(*_cross_pair(bra, ket, gen[0].name + '_cross'), gen)


def _gen_rot(gen: tuple, state: torch.Tensor, theta) -> torch.Tensor:
    _no_legacy(state)
    theta = _sample_param(theta, state, torch.float64, gen[0].name + '_rot')
    return _GenRot.apply(_flat_arg(state), theta, gen)


# Pauli strings: P = (xmask, zmask) over index bits, a Y in both, (P x)[i] = i^ny (-1)^popc((i ^ xmask) & zmask) x[i ^ xmask];
# the support is the amplitudes inside the controls, and the spec is (xmask, zmask, controls).  P is Hermitian, the inner
# product over the controls is the cross of the empty string, and rot = exp(-i theta/2 P) = axpby(cos(theta/2),
# -i sin(theta/2)): r = -i/2, gtheta = 1/2 Im cross.
_PAULI_STRINGS = _Generator(
    name='pauli', sign=+1, axpby='apply_pauli_axpby', cross='pauli_cross', rot='apply_pauli_rot',
    spread=lambda spec: (spec[:2], spec[2:]),
    inner=lambda gen, x, gy, like: _gen_cross((gen[0], (0, 0, gen[1][2])), x, gy),
    rate=lambda theta_t: -0.5j * theta_t.to(torch.complex128),
    gtheta=lambda z: 0.5 * z.imag,
)


def _excite_inner(gen: tuple, x: torch.Tensor, gy: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    kgy = _gen_axpby(gen, gy, torch.zeros_like(like), torch.ones_like(like), 'map')
    return -_gen_cross(gen, x, kgy)


# Excitations: K = E - E^dagger over the pairs of a spec (xmask, amask, zmask, negate, controls), real and anti-symmetric;
# the support is the pairs.  K^3 = -K, so -K^2 projects onto the pairs and the inner product over them is -cross(x, K gy),
# one 'map' axpby more; rot = exp(theta K) = axpby(cos(theta), sin(theta)): r = 1, gtheta = Re cross.
_EXCITATIONS = _Generator(
    name='excite', sign=-1, axpby='apply_excite_axpby', cross='excite_cross', rot='apply_excite_rot',
    spread=lambda spec: ((spec,), ()),
    inner=_excite_inner,
    rate=lambda theta_t: theta_t.to(torch.complex128),
    gtheta=lambda z: z.real,
)


# Sums of Pauli strings (csrc/dq_psum.hip): H = sum_t h_t P_t with real h_t is Hermitian and its support is the whole state --
# 'gate' and 'map' coincide -- so the inner product is the cross of the empty Pauli string without controls.  The spec is
# (`backend.PsumTable`, tol): tol is the tolerance of the rotation and reaches `rot` alone (`rot_tail`).  exp(-i t H) is
# not a combination of I and H, but it is a short sum of Chebyshev polynomials of H (`backend.apply_psum_evolve`), a
# function of H that commutes with it as the rules ask: r = -i, gtheta = Re(-i cross) = Im cross.
_PAULI_SUMS = _Generator(
    name='psum', sign=+1, axpby='apply_psum_axpby', cross='psum_cross', rot='apply_psum_evolve',
    spread=lambda spec: ((spec[0],), ()),
    inner=lambda gen, x, gy, like: _gen_cross((_PAULI_STRINGS, (0, 0, ())), x, gy),
    rate=lambda t_t: -1j * t_t.to(torch.complex128),
    gtheta=lambda z: z.imag,
    rot_tail=lambda spec: (spec[1],) if len(spec) < 3 or spec[2] is None else (spec[1], None, spec[2]),     # (tol[, out, bounds])
)


def _psum_table(H, what: str) -> backend.PsumTable:
    table = getattr(H, 'table', H)
    if not isinstance(table, backend.PsumTable):
        raise ValueError(f'{what}: H must be a PauliSum (or its backend.PsumTable), got {type(H).__name__}')
    return table


def psum_axpby(state: torch.Tensor, a, c, H) -> torch.Tensor:
    """Differentiable ``a x + c H x`` on a (B, 2**n) state for the sum of Pauli strings ``H`` (a ``PauliSum``); ``a``, ``c``
    complex, one value or one per sample.  One launch, G + 1 reads and one write of the state for G flip masks, whatever
    the number of strings; the coefficients of H are constants.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_axpby((_PAULI_SUMS, (_psum_table(H, 'psum_axpby'), None)), state, a, c, 'gate')


def psum_cross(bra: torch.Tensor, ket: torch.Tensor, H) -> torch.Tensor:
    """Differentiable ``sum_i conj(bra_i) (H ket)_i`` of two (B, 2**n) states for the sum of Pauli strings ``H`` (a
    ``PauliSum``): complex128 (B,), one launch.  Pass the same tensor twice for ``<H>`` (the own vectors are read once).
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_cross((_PAULI_SUMS, (_psum_table(H, 'psum_cross'), None)), bra, ket)


def psum_evolve(state: torch.Tensor, t, H, tol: float | None = None, bounds: tuple[float, float] | None = None) -> torch.Tensor:
    """Differentiable ``exp(-i t H) x`` on a (B, 2**n) state for the sum of Pauli strings ``H`` (a ``PauliSum``), ``t`` real,
    one value or one per sample: a Chebyshev expansion accurate to ``tol`` (default 1e-6 for complex64 states, 1e-12 for
    complex128) uniformly in ``t`` -- no Trotter error -- in about ``norm_bound |t|`` plus a few dozen launches of one read
    of the state per flip mask each (``backend.apply_psum_evolve``, which reads ``t`` on the host).  Differentiable to any
    order in the state and in ``t``: the backward is one evolution by ``-t`` and one ``psum_cross``.
    ``bounds=(lo, hi)``: an interval that holds the spectrum of H (``PauliSum.spectral_bounds``), in place of the rigorous
    and loose ``constant -+ norm_bound``: fewer orders; it travels with ``tol``, so the backward uses the same one.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    if tol is None:
        tol = 1e-12 if state.dtype == torch.complex128 else 1e-6
    tol = float(tol)
    if not (tol > 0.0 and tol < float('inf')):
        raise ValueError(f'psum_evolve: tol must be a positive number, got {tol}')
    if not isinstance(t, torch.Tensor):                 # (a Python float is a double: not through the default float32)
        t = torch.tensor(t, dtype=torch.float64, device=state.device)
    table = _psum_table(H, 'psum_evolve')
    if bounds is None:
        return _gen_rot((_PAULI_SUMS, (table, tol)), state, t)
    backend._evolve_window(table, bounds, 'psum_evolve')                           # (refused here, by name, once)
    return _gen_rot((_PAULI_SUMS, (table, tol, (float(bounds[0]), float(bounds[1])))), state, t)


def _pauli_masks(xmask: int, zmask: int, controls: Sequence[int]) -> tuple[int, int, tuple]:
    return int(xmask), int(zmask), tuple(int(c) for c in controls)


def pauli_axpby(state: torch.Tensor, xmask: int, zmask: int, a, c, controls: Sequence[int] = (),
                mode: str = 'gate') -> torch.Tensor:
    """Differentiable ``a x + c P x`` on a (B, 2**n) state for the Pauli string ``P = (xmask, zmask)`` over index bits (a Y
    sets its bit in both); ``a``, ``c`` complex, one value or one per sample.  Amplitudes outside the controls pass
    through (``mode='gate'``) or come out as 0 (``mode='map'``, the cotangent of :func:`pauli_cross`).  One read and one
    write of the state whatever the weight of P.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_axpby((_PAULI_STRINGS, _pauli_masks(xmask, zmask, controls)), state, a, c, mode)


def pauli_cross(bra: torch.Tensor, ket: torch.Tensor, xmask: int, zmask: int, controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable ``sum_i conj(bra_i) (P ket)_i`` of two (B, 2**n) states over the amplitudes inside the controls:
    complex128 (B,).  Pass the same tensor twice for ``<P>`` (one read of the state); ``xmask = zmask = 0`` is the
    inner product.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_cross((_PAULI_STRINGS, _pauli_masks(xmask, zmask, controls)), bra, ket)


def pauli_rot(state: torch.Tensor, xmask: int, zmask: int, theta, controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable ``exp(-i theta/2 P)`` on a (B, 2**n) state: ``theta`` real, one value or one per sample; cosine and
    sine of ``theta / 2`` are formed in double for both precisions.  One read and one write of the state.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_rot((_PAULI_STRINGS, _pauli_masks(xmask, zmask, controls)), state, theta)


def _excite_spec(spec) -> tuple:
    """(xmask, amask, zmask, negate, controls) with plain ints and a tuple of controls: hashable, and what the nodes keep."""
    if not isinstance(spec, (tuple, list)) or len(spec) not in (4, 5):
        raise ValueError(f'an excitation spec is (xmask, amask, zmask, negate[, controls]), got {spec!r}')
    return (*(int(v) for v in spec[:4]), tuple(int(c) for c in spec[4]) if len(spec) == 5 else ())


def excite_axpby(state: torch.Tensor, spec, a, c, mode: str = 'gate') -> torch.Tensor:
    """Differentiable ``a x + c K x`` on the pairs of the excitation ``spec = (xmask, amask, zmask, negate[, controls])``
    of a (B, 2**n) state (:func:`backend.apply_excite_axpby`); ``a``, ``c`` complex, one value or one per sample.
    Amplitudes outside the pairs pass through (``mode='gate'``) or come out as 0 (``mode='map'``, the cotangent of
    :func:`excite_cross`).
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_axpby((_EXCITATIONS, _excite_spec(spec)), state, a, c, mode)


def excite_cross(bra: torch.Tensor, ket: torch.Tensor, spec) -> torch.Tensor:
    """Differentiable ``sum_i conj(bra_i) (K ket)_i`` of two (B, 2**n) states over the pairs of ``spec``: complex128 (B,).
    Pass the same tensor twice to read each pair once (the real part is then 0 up to rounding).
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_cross((_EXCITATIONS, _excite_spec(spec)), bra, ket)


def excite_rot(state: torch.Tensor, spec, theta) -> torch.Tensor:
    """Differentiable ``exp(theta K)`` -- a Givens rotation by the FULL angle theta in every pair of ``spec`` -- on a
    (B, 2**n) state: ``theta`` real, one value or one per sample; cosine and sine are formed in double for both
    precisions.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _gen_rot((_EXCITATIONS, _excite_spec(spec)), state, theta)


# ---- basis-state permutations on any number of wires (csrc/dq_perm.hip) --------------------------------------------------
# P |x> = |perm(x)> on the table bits, inside the controls: a real permutation matrix, so its adjoint is its inverse.  One
# operation closed under differentiation: the backward and the jvp are the function itself.
class _PermuteBasis(torch.autograd.Function):
    """y = P x, in gather form y[j] = x[put(j, inv[sub(j)])] with inv = perm^-1: linear in x, cotangent gx = P^T gy -- the
    permutation by the inverse table, which is the same function with the two tables swapped."""

    @staticmethod
    def forward(state: torch.Tensor, perm: torch.Tensor, inv: torch.Tensor, bits: tuple, controls: tuple) -> torch.Tensor:
        return backend.apply_permutation(_kernel_arg(state), _plain(inv), bits, controls)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _state, perm, inv, ctx.bits, ctx.controls = inputs
        ctx.save_for_backward(perm, inv)
        ctx.save_for_forward(perm, inv)

    @staticmethod
    def jvp(ctx, state_t, *_):
        _single_forward_level()
        perm, inv = ctx.saved_tensors
        return _PermuteBasis.apply(_flat_arg(state_t), perm, inv, ctx.bits, ctx.controls)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        perm, inv = ctx.saved_tensors
        return _PermuteBasis.apply(_flat_arg(gy), inv, perm, ctx.bits, ctx.controls), None, None, None, None

    @staticmethod
    def vmap(info, in_dims, state, perm, inv, bits, controls):
        return _vmap_states(_PermuteBasis, 'permute_basis', info, in_dims, (state, perm, inv, bits, controls), tables=(1, 2))


def invert_table(perm: torch.Tensor) -> torch.Tensor:
    """perm^-1 of a bijection of range(len(perm)) (not checked here: ``PermutationGate`` checks what it is given)."""
    inv = torch.empty_like(perm)
    inv[perm.long()] = torch.arange(perm.shape[0], dtype=perm.dtype, device=perm.device)
    return inv


def permute_basis(state: torch.Tensor, perm: torch.Tensor, bits: Sequence[int], controls: Sequence[int] = (),
                  inv: torch.Tensor | None = None) -> torch.Tensor:
    """Differentiable (in the state) basis-state permutation ``|x> -> |perm(x)>`` on a (B, 2**n) state: ``perm`` a constant
    integer table of 2^k entries, a bijection of ``range(2^k)``, over the index bits ``bits`` (``bits[0]`` = its most
    significant bit); amplitudes outside the controls pass through.  One read and one write of the state, amplitudes
    copied bit for bit.  ``inv``: perm^-1 where the caller holds it already (it is formed here otherwise).
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(state)
    for t in (perm, inv):
        if t is not None and (not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.ndim != 1):
            raise ValueError('permute_basis: the table must be a 1-D integer tensor')
    bits, controls = _bit_args(bits, controls)
    if inv is None:
        inv = invert_table(perm)
    return _PermuteBasis.apply(_flat_arg(state), perm, inv, bits, controls)


# ---- SELECT over Pauli strings (csrc/dq_select.hip) ------------------------------------------------------------------------
# S = sum_s |s><s| (x) c_s P_s on the select bits and the wires its strings touch, inside the controls: linear in the state,
# unitary, and its adjoint is the same map with every phase conjugated -- the other table of a backend.SelectTable.  One
# operation closed under differentiation: the backward is the function itself with the two tables swapped, the jvp the
# function itself.
class _SelectPauli(torch.autograd.Function):
    """y = S x from the table ``words``: linear in x, cotangent gx = S^dagger gy -- the same function from ``dagger``."""

    @staticmethod
    def forward(state: torch.Tensor, words: torch.Tensor, dagger: torch.Tensor, bits: tuple, controls: tuple) -> torch.Tensor:
        return backend.apply_select_pauli(_kernel_arg(state), words, bits, controls)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _state, words, dagger, ctx.bits, ctx.controls = inputs
        ctx.save_for_backward(words, dagger)
        ctx.save_for_forward(words, dagger)

    @staticmethod
    def jvp(ctx, state_t, *_):
        _single_forward_level()
        words, dagger = ctx.saved_tensors
        return _SelectPauli.apply(_flat_arg(state_t), words, dagger, ctx.bits, ctx.controls)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        words, dagger = ctx.saved_tensors
        return _SelectPauli.apply(_flat_arg(gy), dagger, words, ctx.bits, ctx.controls), None, None, None, None

    @staticmethod
    def vmap(info, in_dims, state, words, dagger, bits, controls):
        return _vmap_states(_SelectPauli, 'select_pauli', info, in_dims, (state, words, dagger, bits, controls), tables=(1, 2))


def select_pauli(state: torch.Tensor, table: 'backend.SelectTable', bits: Sequence[int], controls: Sequence[int] = (),
                 dagger: bool = False) -> torch.Tensor:
    """Differentiable (in the state, to any order) SELECT ``sum_s |s><s| (x) c_s P_s`` on a (B, 2**n) state: ``table`` a
    constant :class:`backend.SelectTable` of 2^k strings with their powers of i, read by the value s of the index bits
    ``bits`` (``bits[0]`` = its most significant bit); amplitudes outside the controls pass through; ``dagger``: the
    adjoint.  One read and one write of the state whatever the number of strings, exact.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(state)
    if not isinstance(table, backend.SelectTable):
        raise ValueError(f'select_pauli: the table must be a backend.SelectTable, got {type(table).__name__}')
    bits, controls = _bit_args(bits, controls)
    if len(bits) != table.k:
        raise ValueError(f'select_pauli: the table is over {table.k} select bits, got {len(bits)}')
    words, other = table.on(state.device, dagger)
    return _SelectPauli.apply(_flat_arg(state), words, other, bits, controls)


# ---- multiplexed one-qubit gates on any number of select wires (csrc/dq_mux.hip) -----------------------------------------
# M = sum_s |s><s| (x) M[s] on the select bits and the target, inside the controls: linear in the state, and its adjoint is
# the same map with every entry daggered -- which the kernel applies from the same table.  One operation closed under
# differentiation: the backward and the jvp are the function itself.
class _MuxApply(torch.autograd.Function):
    """y = M x: cotangent gx = M^+ gy, the same function with ``dagger`` toggled; the tangent is M x_t."""

    @staticmethod
    def forward(state: torch.Tensor, table: torch.Tensor, kind: str, target: int, bits: tuple, controls: tuple,
                dagger: bool) -> torch.Tensor:
        return backend.apply_mux(_kernel_arg(state), _plain(table), kind, target, bits, controls, dagger)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _state, table, ctx.kind, ctx.target, ctx.bits, ctx.controls, ctx.dagger = inputs
        ctx.save_for_backward(table)
        ctx.save_for_forward(table)

    @staticmethod
    def jvp(ctx, state_t, *_):
        _single_forward_level()
        (table,) = ctx.saved_tensors
        return _MuxApply.apply(_flat_arg(state_t), table, ctx.kind, ctx.target, ctx.bits, ctx.controls, ctx.dagger)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        (table,) = ctx.saved_tensors
        gx = _MuxApply.apply(_flat_arg(gy), table, ctx.kind, ctx.target, ctx.bits, ctx.controls, not ctx.dagger)
        return gx, None, None, None, None, None, None

    @staticmethod
    def vmap(info, in_dims, state, table, kind, target, bits, controls, dagger):
        return _vmap_states(_MuxApply, 'mux_apply', info, in_dims, (state, table, kind, target, bits, controls, dagger),
                            tables=(1,))


def mux_apply(state: torch.Tensor, table: torch.Tensor, kind: str, target: int, bits: Sequence[int],
              controls: Sequence[int] = (), dagger: bool = False) -> torch.Tensor:
    """Differentiable (in the state) multiplexed one-qubit gate on a (B, 2**n) state: for every value of the select bits
    ``bits`` (``bits[0]`` = the table index's most significant bit) its own 2x2 matrix on index bit ``target``; amplitudes
    outside the controls pass through.  ``kind='u'``: ``table`` a constant complex (2^k, 2, 2); ``kind='ry'``: a constant
    real (2^k, 2) of rows (c, s), M = [[c, -s], [s, c]].  ``dagger`` applies the conjugate transposes from the same table.
    One read and one write of the state whatever k is.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(state)
    table = _const_table(table, 'mux_apply')
    if kind not in ('u', 'ry'):
        raise ValueError(f"mux_apply: kind must be 'u' or 'ry', got {kind!r}")
    bits, controls = _bit_args(bits, controls)
    return _MuxApply.apply(_flat_arg(state), table, kind, int(target), bits, controls, bool(dagger))


# ---- trainable multiplexed rotations: per-select coefficients and angles (csrc/dq_mux.hip, csrc/dq_muxgrad.hip) ---------
# G = the one-qubit Pauli sigma (I, X, Y, Z) on the target inside the controls, 0 elsewhere; bin s = the amplitudes with
# sub(i) = s inside the controls.  G maps every bin to itself (the select bits, the controls and the target are disjoint)
# and G^dagger = G.  The generator rules above, with one coefficient PER BIN instead of one per sample:
#     axpby(x; a, c)[i] = a[sub i] x[i] + c[sub i] (G x)[i] inside the controls     (elsewhere: x[i] 'gate', 0 'map')
#     cross(u, v)[b, s] = sum over bin s of conj(u[b, i]) (G v[b])[i]               complex128 (B, 2^k)
#     rot(x; theta)     = axpby(x; cos(theta/2), -i sin(theta/2)) in 'gate' mode    sigma in {X, Y, Z}, theta real
#     axpby:  gx = axpby(gy; conj a, conj c) in the same mode;  gc = cross_sigma(x, gy);  ga = cross_I(x, gy)
#     cross:  g_u = map(v; 0, conj gz);  g_v = map(u; 0, gz)
#     rot:    gx = rot(gy; -theta);  gtheta[b, s] = Im cross(gx, x)[b, s] / 2
# These are three nodes of their own and not a third family of `_Generator`: its nodes keep a, c and theta as (B,), hand
# them to `_vmap_states` as (B,) and reduce every cross to (B,); a parameter of shape (B, 2^k) changes each of those
# lines, for the families that exist too.  A parameter is kept as (Bp, 2^k) with Bp = 1 (shared by the batch: one table,
# one launch, and its gradient is the sum of the cross over the batch) or Bp = B (per sample: what the cotangents of
# `cross` are, so from the second order on; one launch per sample, tested and not tuned).  The spec is
# ``mux = (axis, target, bits, controls)``.
def _mux_fit(z: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """A cross (B, 2^k) as the gradient of a parameter ``like`` of shape (1 or B, 2^k)."""
    return z.sum(dim=0, keepdim=True) if like.shape[0] == 1 and z.shape[0] != 1 else z


def _vmap_mux(cls, info, in_dims, args: tuple, params: tuple, nstates: int = 1):
    """The ``vmap`` rule of the three nodes: the mapped dimension of the states goes into the batch dimension; a mapped
    parameter becomes per sample, a shared one that is not mapped stays shared."""
    v = info.batch_size
    args = list(args)
    same = nstates == 2 and args[0] is args[1] and in_dims[0] == in_dims[1]
    for i in range(nstates):
        args[i] = args[0] if (i == 1 and same) else _fold(args[i], in_dims[i], v)
    b = args[0].shape[0] // v
    for i in params:
        p, d = args[i], in_dims[i]
        if d is None and p.shape[0] == 1:
            continue
        p = p.movedim(d, 0) if d is not None else p.unsqueeze(0)
        args[i] = p.expand(v, b, p.shape[-1]).reshape(v * b, p.shape[-1])
    out = cls.apply(*args)
    return out.reshape(v, -1, out.shape[-1]), 0


class _MuxAxpby(torch.autograd.Function):
    """y = a[sub] x + c[sub] G x with a, c complex128 (1 or B, 2^k): see the rules above."""

    @staticmethod
    def forward(state: torch.Tensor, a: torch.Tensor, c: torch.Tensor, mux: tuple, mode: str) -> torch.Tensor:
        return backend.apply_mux_axpby(_kernel_arg(state), _plain(a), _plain(c), *mux, mode)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, a, c, ctx.mux, ctx.mode = inputs
        ctx.save_for_backward(state, a, c)
        ctx.save_for_forward(state, a, c)

    @staticmethod
    def jvp(ctx, state_t, a_t, c_t, *_):
        _single_forward_level()
        state, a, c = ctx.saved_tensors
        out = None
        if state_t is not None:
            out = _mux_axpby(ctx.mux, state_t, a, c, ctx.mode)
        if a_t is not None or c_t is not None:
            zero = torch.zeros_like(a)
            term = _mux_axpby(ctx.mux, state, zero if a_t is None else a_t, zero if c_t is None else c_t, 'map')
            out = term if out is None else out + term
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        mux = ctx.mux
        state, a, c = ctx.saved_tensors
        gstate = ga = gc = None
        if ctx.needs_input_grad[0]:
            gstate = _mux_axpby(mux, gy, a.conj(), c.conj(), ctx.mode)
        if ctx.needs_input_grad[1]:
            ga = _mux_fit(_mux_cross(('i', *mux[1:]), state, gy), a).to(a.dtype)
        if ctx.needs_input_grad[2]:
            gc = _mux_fit(_mux_cross(mux, state, gy), c).to(c.dtype)
        return gstate, ga, gc, None, None

    @staticmethod
    def vmap(info, in_dims, state, a, c, mux, mode):
        return _vmap_mux(_MuxAxpby, info, in_dims, (state, a, c, mux, mode), params=(1, 2))


class _MuxCross(torch.autograd.Function):
    """z[b, s] = sum over bin s of conj(u_i) (G v)_i, complex128 (B, 2^k): see the rules above."""

    @staticmethod
    def forward(bra: torch.Tensor, ket: torch.Tensor, mux: tuple) -> torch.Tensor:
        pk = _kernel_arg(ket)
        return backend.mux_cross(pk if bra is ket else _kernel_arg(bra), pk, *mux)

    @staticmethod
    def setup_context(ctx, inputs, output):
        bra, ket, ctx.mux = inputs
        ctx.save_for_backward(bra, ket)
        ctx.save_for_forward(bra, ket)

    @staticmethod
    def jvp(ctx, bra_t, ket_t, *_):
        _single_forward_level()
        bra, ket = ctx.saved_tensors
        return _jvp_two_slots(lambda u, v: _mux_cross(ctx.mux, u, v), bra, ket, bra_t, ket_t)

    @staticmethod
    def backward(ctx, gz: torch.Tensor):
        mux = ctx.mux
        bra, ket = ctx.saved_tensors
        gz = gz.to(torch.complex128)
        zero = torch.zeros_like(gz)
        gbra = gket = None
        if ctx.needs_input_grad[0]:
            gbra = _mux_axpby(mux, ket, zero, gz.conj(), 'map')
        if ctx.needs_input_grad[1]:
            gket = _mux_axpby(mux, bra, zero, gz, 'map')
        return gbra, gket, None

    @staticmethod
    def vmap(info, in_dims, bra, ket, mux):
        return _vmap_mux(_MuxCross, info, in_dims, (bra, ket, mux), params=(), nstates=2)


class _MuxRot(torch.autograd.Function):
    """y = R_sigma(theta[sub]) x, theta real (1 or B, 2^k): see the rules above -- one rotation and one cross per backward."""

    @staticmethod
    def forward(state: torch.Tensor, theta: torch.Tensor, mux: tuple) -> torch.Tensor:
        return backend.apply_mux_rot(_kernel_arg(state), _plain(theta), *mux)

    @staticmethod
    def setup_context(ctx, inputs, output):
        state, theta, ctx.mux = inputs
        ctx.save_for_backward(state, theta)
        ctx.save_for_forward(state, theta)

    @staticmethod
    def jvp(ctx, state_t, theta_t, *_):
        _single_forward_level()
        mux = ctx.mux
        state, theta = ctx.saved_tensors
        out = None
        if state_t is not None:
            out = _mux_rot(mux, state_t, theta)
        if theta_t is not None:
            y = _mux_rot(mux, state, theta)
            rate = -0.5j * theta_t.to(torch.complex128)
            term = _mux_axpby(mux, y, torch.zeros_like(rate), rate, 'map')
            out = term if out is None else out + term
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        mux = ctx.mux
        state, theta = ctx.saved_tensors
        gstate = _mux_rot(mux, gy, -theta)
        gtheta = None
        if ctx.needs_input_grad[1]:
            gtheta = _mux_fit(0.5 * _mux_cross(mux, gstate, state).imag, theta).to(theta.dtype)
        return (gstate if ctx.needs_input_grad[0] else None), gtheta, None

    @staticmethod
    def vmap(info, in_dims, state, theta, mux):
        return _vmap_mux(_MuxRot, info, in_dims, (state, theta, mux), params=(1,))


def _mux_spec(axis: str, target: int, bits: Sequence[int], controls: Sequence[int], axes: str, what: str) -> tuple:
    if axis not in tuple(axes):
        raise ValueError(f'{what}: axis must be one of {", ".join(repr(ch) for ch in axes)}; got {axis!r}')
    return (axis, int(target), *_bit_args(bits, controls))


def _mux_param(p, state: torch.Tensor, mux: tuple, dtype: torch.dtype, what: str) -> torch.Tensor:
    """(2^k,), (1, 2^k) or (B, 2^k) as (1 or B, 2^k) in ``dtype``, differentiably."""
    if not isinstance(p, torch.Tensor):
        p = torch.as_tensor(p, device=state.device)
    if p.is_complex() and not dtype.is_complex:
        raise ValueError(f'{what}: real angles expected, got {p.dtype}')
    p = p.to(dtype)
    if p.ndim == 1:
        p = p.unsqueeze(0)
    d = 1 << len(mux[2])
    if p.ndim != 2 or p.shape[-1] != d or p.shape[-2] not in (1, state.shape[-2]):
        raise ValueError(f'{what}: {len(mux[2])} select bits take ({d},) values, or ({state.shape[-2]}, {d}) for one row per '
                         f'sample; got {tuple(p.shape)}')
    return p


def _mux_axpby(mux: tuple, state: torch.Tensor, a, c, mode: str) -> torch.Tensor:
    _no_legacy(state)
    if mode not in ('gate', 'map'):
        raise ValueError(f"mux_axpby: mode must be 'gate' or 'map', got {mode!r}")
    a = _mux_param(a, state, mux, torch.complex128, 'mux_axpby')
    c = _mux_param(c, state, mux, torch.complex128, 'mux_axpby')
    return _MuxAxpby.apply(_flat_arg(state), a, c, mux, mode)


def _mux_cross(mux: tuple, bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    return _MuxCross.apply(*_cross_pair(bra, ket, 'mux_cross'), mux)


def _mux_rot(mux: tuple, state: torch.Tensor, theta) -> torch.Tensor:
    _no_legacy(state)
    return _MuxRot.apply(_flat_arg(state), _mux_param(theta, state, mux, torch.float64, 'mux_rot'), mux)


def mux_axpby(state: torch.Tensor, a, c, axis: str, target: int, bits: Sequence[int], controls: Sequence[int] = (),
              mode: str = 'gate') -> torch.Tensor:
    """Differentiable ``a[s] x + c[s] sigma x`` on a (B, 2**n) state: for every value s of the select bits ``bits``
    (``bits[0]`` = the most significant bit of s) its own complex pair (a[s], c[s]) and the Pauli ``axis`` ('i', 'x', 'y',
    'z') on index bit ``target``.  ``a``, ``c``: (2^k,) shared by the batch or (B, 2^k) per sample, differentiable to any
    order like the state.  Amplitudes outside the controls pass through (``mode='gate'``) or come out as 0
    (``mode='map'``, the cotangent of :func:`mux_cross`).  Shared coefficients are one read and one write of the state
    whatever k is; per-sample coefficients -- they arise from the second derivative on -- run one launch per sample: that
    route is tested, not tuned.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _mux_axpby(_mux_spec(axis, target, bits, controls, 'ixyz', 'mux_axpby'), state, a, c, mode)


def mux_cross(bra: torch.Tensor, ket: torch.Tensor, axis: str, target: int, bits: Sequence[int],
              controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable ``sum over sub(i) = s of conj(bra_i) (sigma ket)_i`` of two (B, 2**n) states inside the controls, one
    number per sample and per value s of the select bits: complex128 (B, 2^k), one read of each state whatever k is,
    bitwise reproducible.  Pass the same tensor twice for one read of the state.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _mux_cross(_mux_spec(axis, target, bits, controls, 'ixyz', 'mux_cross'), bra, ket)


def mux_rot(state: torch.Tensor, theta, axis: str, target: int, bits: Sequence[int],
            controls: Sequence[int] = ()) -> torch.Tensor:
    """Differentiable multiplexed rotation ``R_axis(theta[s])`` (``axis`` 'x', 'y' or 'z') on index bit ``target`` of a
    (B, 2**n) state for every value s of the select bits: ``theta`` real, (2^k,) shared by the batch or (B, 2^k) per
    sample (one launch per sample: tested, not tuned); cosine and sine of ``theta / 2`` are formed in double for both
    precisions.  One read and one write of the state forward; one rotation and one binned cross reduction backward,
    whatever k is.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    return _mux_rot(_mux_spec(axis, target, bits, controls, 'xyz', 'mux_rot'), state, theta)


# ---- every sample against every sample (csrc/dq_gram.hip) ----------------------------------------------------------------
# Two operations that close under differentiation -- every backward and every jvp below is written with the other one --
# so derivatives of any order exist by construction.  In PyTorch's conjugate convention, with Gbar / Ybar the cotangents:
#     G = gram(A, B)     = conj(A) B^T        Abar = combine(B, conj(Gbar))       Bbar = combine(A, Gbar^T)
#     Y = combine(S, C)  = C S                Sbar = combine(Ybar, C^H)           Cbar = gram(S, Ybar)^T
def _no_vmap(what: str):
    raise RuntimeError(f'deepquantum_amd: {what} under torch.vmap is not supported: the node already works on all rows of a '
                       'batch against all rows; call it on the whole batch instead of mapping over it')


class _Gram(torch.autograd.Function):
    """G[i, j] = sum_x conj(A[i, x]) B[j, x], complex128 (M, N): see the rules above."""

    @staticmethod
    def forward(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
        pk = _kernel_arg(ket)
        return backend.gram(pk if bra is ket else _kernel_arg(bra), pk)

    @staticmethod
    def setup_context(ctx, inputs, output):
        bra, ket = inputs
        ctx.save_for_backward(bra, ket)
        ctx.save_for_forward(bra, ket)

    @staticmethod
    def jvp(ctx, bra_t, ket_t):
        _single_forward_level()
        bra, ket = ctx.saved_tensors
        return _jvp_two_slots(gram, bra, ket, bra_t, ket_t)

    @staticmethod
    def backward(ctx, gg: torch.Tensor):
        bra, ket = ctx.saved_tensors
        gg = gg.to(torch.complex128)
        gbra = gket = None
        if ctx.needs_input_grad[0]:
            gbra = combine(ket, gg.conj())
        if ctx.needs_input_grad[1]:
            gket = combine(bra, gg.transpose(0, 1))
        return gbra, gket

    @staticmethod
    def vmap(info, in_dims, bra, ket):
        _no_vmap('gram')


class _Combine(torch.autograd.Function):
    """Y[m, x] = sum_j C[m, j] S[j, x] with C complex128 (M, N): see the rules above."""

    @staticmethod
    def forward(states: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
        return backend.combine(_kernel_arg(states), _plain(coef).detach())

    @staticmethod
    def setup_context(ctx, inputs, output):
        states, coef = inputs
        ctx.save_for_backward(states, coef)
        ctx.save_for_forward(states, coef)

    @staticmethod
    def jvp(ctx, states_t, coef_t):
        _single_forward_level()
        states, coef = ctx.saved_tensors
        return _jvp_two_slots(combine, states, coef, states_t, coef_t)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        states, coef = ctx.saved_tensors
        gstates = gcoef = None
        if ctx.needs_input_grad[0]:
            gstates = combine(gy, coef.conj().transpose(0, 1))
        if ctx.needs_input_grad[1]:
            gcoef = gram(states, gy).transpose(0, 1).to(coef.dtype)
        return gstates, gcoef

    @staticmethod
    def vmap(info, in_dims, states, coef):
        _no_vmap('combine')


def _rows_arg(x: torch.Tensor, what: str) -> torch.Tensor:
    if _is_batched(x):
        _no_vmap(what)
    if not isinstance(x, torch.Tensor) or x.ndim != 2 or not x.is_complex():
        raise ValueError(f'{what}: states must be complex (rows, 2**n) tensors')
    return x if x.is_contiguous() else x.contiguous()


def gram(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """Differentiable Gram matrix ``G[i, j] = <bra_i|ket_j>`` of (M, 2**n) and (N, 2**n) states, complex128 (M, N)
    (``backend.gram``); pass the same tensor twice for the self-Gram (half the reads, exactly Hermitian).  Not under vmap.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(bra, ket)
    same = bra is ket
    ket = _rows_arg(ket, 'gram')
    bra = ket if same else _rows_arg(bra, 'gram')
    if bra.dtype != ket.dtype:
        raise ValueError('gram: bra and ket must have one dtype')
    if bra.shape[1] != ket.shape[1]:
        raise ValueError(f'gram: bra and ket must have one number of qubits, got rows of {bra.shape[1]} and {ket.shape[1]}')
    return _Gram.apply(bra, ket)


def combine(states: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """Differentiable linear combinations ``Y[m] = sum_j coef[m, j] states[j]`` of (N, 2**n) states for a complex (M, N)
    ``coef``: (M, 2**n) in the states' dtype (``backend.combine``); gradients flow to both.  Not under vmap.
    A state that is not 16-byte aligned (a view at an odd complex64 offset) is copied, not refused (:func:`_kernel_arg`)."""
    _no_legacy(states, coef)
    states = _rows_arg(states, 'combine')
    if not isinstance(coef, torch.Tensor):
        raise ValueError(f'combine: coef must be a tensor, got {type(coef).__name__}')
    if _is_batched(coef):
        _no_vmap('combine')
    if coef.ndim != 2 or coef.shape[1] != states.shape[0]:
        raise ValueError(f'combine: coef must have shape (M, {states.shape[0]}) for {states.shape[0]} states, got {tuple(coef.shape)}')
    return _Combine.apply(states, coef.to(torch.complex128))
