"""Tensor-level entry points of the statevector kernels.

Every function takes PyTorch tensors (device memory owned by the caller), checks shapes on the host the
way the reference asserts them (operation.py:91-107, 285-288), and enqueues the matching libdqhip call
on ``torch.cuda.current_stream()``.  CUDA (= HIP on ROCm) tensors are required: a CPU tensor raises
``RuntimeError`` -- there is no CPU fallback in the product.  The unit tests that exercise host logic
without a GPU install an explicit test double with :func:`set_test_backend` (it lives under ``tests/``
and is built on the oracle); the package itself never imports ``oracle/``.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Any, NamedTuple, Sequence

import torch

from . import _lib

_test_backend: Any = None


class _NoGraph:
    """A test double must not be more capable than the product: the HIP entry points return tensors without an
    autograd graph, so every call into the double runs under ``no_grad`` as well (a double built from differentiable
    torch operations once hid a missing second derivative) -- and with forward-mode tangents switched off: a kernel
    that reads raw buffers carries none, the nodes' ``jvp`` rules do."""

    def __init__(self, obj: Any):
        self._obj = obj

    def __getattr__(self, name: str) -> Any:
        attr = getattr(self._obj, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            for a in list(args) + list(kwargs.values()):      # (what `_ptr` refuses, the double refuses)
                if isinstance(a, torch.Tensor) and (a.is_conj() or a.is_neg()):
                    raise ValueError('tensor with a pending conjugation / negation: resolve_conj() / resolve_neg() it first')
            was = torch._C._is_fwd_grad_enabled()
            torch._C._set_fwd_grad_enabled(False)
            try:
                with torch.no_grad():
                    return attr(*args, **kwargs)
            finally:
                torch._C._set_fwd_grad_enabled(was)

        return call


def set_test_backend(obj: Any) -> None:
    """Install (or clear with ``None``) a CPU test double.  For ``tests/`` only."""
    global _test_backend
    _test_backend = None if obj is None else _NoGraph(obj)


def get_test_backend() -> Any:
    return None if _test_backend is None else _test_backend._obj


def _suffix(t: torch.Tensor) -> str:
    if t.dtype == torch.complex64:
        return 'c64'
    if t.dtype == torch.complex128:
        return 'c128'
    raise TypeError(f'state must be complex64 or complex128, got {t.dtype}')


def _use_hip(t: torch.Tensor) -> bool:
    if t.is_cuda:
        return True
    if _test_backend is not None:
        return False
    raise RuntimeError(
        'deepquantum_amd: statevector kernels run on MI355X only; got a tensor on '
        f'{t.device}. Move the circuit/state to "cuda" (there is no CPU fallback).'
    )


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: torch.Tensor | None, row: int = 0) -> C.c_void_p:
    """The address of ``t[row:]`` (no view is made for it)."""
    # a lazily conjugated / negated view (x.mH of a column-major matrix is "contiguous" AND unconjugated in memory) must
    # never reach a kernel as a raw pointer
    if t is not None and (t.is_conj() or t.is_neg()):
        raise ValueError('tensor with a pending conjugation / negation: resolve_conj() / resolve_neg() it first')
    return C.c_void_p(0 if t is None else t.data_ptr() + (row and row * t.stride(0) * t.element_size()))


def _nqubit(state: torch.Tensor) -> int:
    dim = state.shape[-1]
    n = dim.bit_length() - 1
    if state.ndim != 2 or (1 << n) != dim:
        raise ValueError(f'state must have shape (batch, 2**n), got {tuple(state.shape)}')
    return n


def _check_mats(state: torch.Tensor, mats: torch.Tensor, k: int) -> tuple[torch.Tensor, int]:
    """Return contiguous (Bm, D, D) matrices in the state's dtype/device and the batch stride."""
    d = 1 << k
    if mats.ndim == 2:
        mats = mats.unsqueeze(0)
    if mats.ndim != 3 or mats.shape[-1] != d or mats.shape[-2] != d:
        raise ValueError(f'matrix must have shape (.., {d}, {d}), got {tuple(mats.shape)}')
    if mats.shape[0] not in (1, state.shape[0]):
        raise ValueError(f'matrix batch {mats.shape[0]} does not match state batch {state.shape[0]}')
    if mats.dtype != state.dtype or mats.device != state.device:
        mats = mats.to(device=state.device, dtype=state.dtype)
    mats = mats.resolve_conj().resolve_neg().contiguous()     # (.mH of a strided user matrix is contiguous with the conj bit set)
    stride = 0 if mats.shape[0] == 1 else d * d
    return mats, stride


MAX_BATCH = 32768     # slices of a batch wider than the 65535 a grid dimension can hold


def _slices(batch: int, step: int | None = None):
    """``(lo, hi)`` over a batch in slices of at most ``step`` samples: ``MAX_BATCH`` as it is when called, or the 65535 of
    an entry point whose batch is a grid axis of its own."""
    step = MAX_BATCH if step is None else step
    for lo in range(0, batch, step):
        yield lo, min(lo + step, batch)


def _call(entry: str, t: torch.Tensor, *args) -> None:
    """``<entry>_<c64 | c128>(*args, stream)`` for the dtype and the current stream of ``t``, checked."""
    _lib.check(getattr(_lib.load(), f'{entry}_{_suffix(t)}')(*args, _stream(t)), entry)


def _check_out(state: torch.Tensor, out: torch.Tensor | None, what: str, in_place: bool = True,
               shape: tuple[int, ...] | None = None) -> torch.Tensor:
    """``out`` checked (``None``: a new tensor): a contiguous tensor of the state's shape (or of ``shape``, where the
    primitive's result has another number of rows), dtype and device that shares no byte with the state or, where
    ``in_place`` says that a unit of work owns what it reads and writes, is the state's own buffer.  A shifted overlap is
    safe for nobody."""
    shape = tuple(state.shape) if shape is None else tuple(shape)
    if out is None:
        return torch.empty_like(state) if shape == tuple(state.shape) else torch.empty(shape, dtype=state.dtype, device=state.device)
    if tuple(out.shape) != shape or out.dtype != state.dtype or out.device != state.device or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous tensor of "
                         + ("the state's shape" if shape == tuple(state.shape) else f'shape {shape}') + ", the state's dtype and device")
    lo, hi = out.data_ptr(), state.data_ptr()
    apart = abs(lo - hi)
    if (lo < hi + state.nbytes and hi < lo + out.nbytes) and not (in_place and apart == 0 and out.nbytes == state.nbytes):
        raise ValueError(f'{what}: out overlaps the state '
                         + ('without being the same buffer' if in_place else '(out of place only)'))
    return out


def _finish_table(table: torch.Tensor, like: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
    """A constant table as the kernels read it: in ``dtype`` on the state's device, conjugation and negation resolved,
    contiguous and 16-byte aligned (a misaligned view is copied, not refused)."""
    if table.requires_grad:
        raise ValueError(f'{what}: the table is a constant -- gradients with respect to its entries are not supported; '
                         'detach() it')
    if table.dtype != dtype or table.device != like.device:
        table = table.to(device=like.device, dtype=dtype)
    table = table.resolve_conj().resolve_neg().contiguous()
    if table.is_cuda and table.data_ptr() % 16:
        table = table.clone()
    return table


# ---------------------------------------------------------------------------------------------------
def apply_gate(
    state: torch.Tensor,
    mats: torch.Tensor,
    targets: Sequence[int],
    controls: Sequence[int] = (),
    out: torch.Tensor | None = None,
) -> torch.Tensor:
    """psi' = (U on ``targets``, conditioned on all ``controls`` = 1) psi.

    ``state``: (B, 2**n) contiguous complex; ``targets``/``controls``: bit positions (LSB = 0),
    ``targets[0]`` is the matrix-index MSB.  ``out`` may be ``state`` itself (in place) for k <= 4.
    Replaces qmath.evolve_state / Gate.op_state_control of the reference.
    """
    n = _nqubit(state)
    targets, controls = [int(t) for t in targets], [int(c) for c in controls]
    k = len(targets)
    if not state.is_contiguous():
        raise ValueError('state must be contiguous')
    mats, stride = _check_mats(state, mats, k)
    if out is None:
        out = torch.empty_like(state)
    if not _use_hip(state):
        return _test_backend.apply_gate(state, mats, targets, controls, out)
    if state.shape[0] > MAX_BATCH:       # the batch is a grid dimension (<= 65535): very wide batches go in slices
        for lo, hi in _slices(state.shape[0]):
            apply_gate(state[lo:hi], mats[lo:hi] if stride else mats, targets, controls, out[lo:hi])
        return out
    _call('dq_apply_gate', state, _ptr(state), _ptr(out), _ptr(mats), stride, n, _lib.int_array(targets), k,
          _lib.int_array(controls), len(controls), state.shape[0])
    return out


#: records of a pass that travel in the kernel-argument segment (csrc/dq_wave.hip, WAVE_MAX_REC); a pass with more keeps them
#: in device memory (include/dq_hip.h, dq_wave_records / dq_apply_fused_grad_ext_*)
KERNARG_RECORDS = 112
#: Device tensors that launches of a HIP graph UNDER CAPTURE read and that a plan or a cache owns -- the kernel matrix buffer
#: of a circuit with fixed gates, the offsets of its deferred Rx blocks, the records of a long pass: the graph has their
#: addresses baked in, so they must outlive the plan cache's evictions.  Only tensors a cache OWNS are pinned (`own`):
#: what a capture allocates itself -- the matrix buffer of a trainable circuit, built anew inside the capture -- comes
#: from the graph's private pool and lives with the graph; pinning it would keep pool blocks from ever being reused.
#: Pins of a capture made by `utils.CapturedGraph` belong to that object (`_PIN_SINK`) and die with it; those of a raw
#: ``torch.cuda.graph`` capture stay here: a few KiB per captured circuit.
_CAPTURE_PINS: dict = {}
_PIN_SINK: list = []          # the innermost CapturedGraph under construction keeps its pins in _PIN_SINK[-1]


def own(t: torch.Tensor | None) -> torch.Tensor | None:
    """Mark a device tensor as owned by a plan / steady-state cache (what `pin_if_capturing` keeps alive)."""
    if t is not None:
        t._dq_owned = True
    return t


def pin_if_capturing(*tensors: torch.Tensor | None) -> None:
    first = next((t for t in tensors if t is not None), None)
    if first is None or not first.is_cuda or not torch.cuda.is_current_stream_capturing():
        return
    for t in tensors:
        if t is not None and getattr(t, '_dq_owned', False):
            if _PIN_SINK:
                _PIN_SINK[-1].setdefault(id(t), t)
            else:
                _CAPTURE_PINS.setdefault(id(t), t)


def _device_records(desc: _lib.DqFusedPass, n: int, device: torch.device) -> torch.Tensor | None:
    """The records of ``desc`` on ``device`` (a uint8 tensor, cached on the descriptor) when they do not fit the
    kernel-argument segment, else None.  Only passes with many gates can need them: up to 72 gates and reductions (the cap
    of every pass before ABI 24) the planner's bound on layout changes keeps a pass within the segment, and the count is not
    even asked for."""
    if desc.rounds[desc.nrounds - 1].gate_end <= 72:
        return None
    cache = desc.__dict__.setdefault('_dev_records', {})
    key = (n, device)
    hit = cache.get(key, False)
    if hit is False:
        lib = _lib.load()
        nbytes = lib.dq_wave_records(C.byref(desc), n, None, 0)
        if nbytes < 0:
            _lib.check(int(nbytes), 'dq_wave_records')
        if nbytes <= 32 * KERNARG_RECORDS:
            hit = None
        else:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('deepquantum_amd: the first run of a pass with more than 112 records copies them to the '
                                   'device; run the step once before capturing it (dq.CapturedGraph warms up by itself)')
            host = torch.empty(int(nbytes), dtype=torch.uint8)
            got = lib.dq_wave_records(C.byref(desc), n, host.data_ptr(), int(nbytes))
            assert got == nbytes
            hit = own(host.to(device))
        cache[key] = hit
    return hit


def apply_fused(
    state: torch.Tensor,
    mats: torch.Tensor,
    mat_batch_stride: int,
    desc: _lib.DqFusedPass,
    out: torch.Tensor | None = None,
    grads: torch.Tensor | None = None,
    known_zero: int = 0,
    slice_bits: tuple[int, int] | None = None,
) -> torch.Tensor:
    """Run one fused pass (see fusion.py).  ``mats``: flat complex buffer (Bm * stride or stride).
    ``state`` with ONE row and ``out`` with B rows: the single input state is shared by all outputs.
    ``grads`` (float64, (B, rows, 8), added to): a pass of the adjoint method's reverse sweep -- its DQ_FG_GRAD
    records reduce into it (include/dq_hip.h, dq_apply_fused_grad_c64 / _c128).
    ``known_zero``: index bits (read side) known to be |0> in ``state`` -- it is not read where one of them is 1, and
    ``out`` is not written where such a bit outside the tile is 1 (include/dq_hip.h, dq_apply_fused_zext_*).
    ``slice_bits = (mask, value)``: ONE SLICE of the pass -- only the tiles whose index bits ``mask`` (read side, outside the
    tile) equal ``value`` run (include/dq_hip.h, dq_apply_fused_slice_*)."""
    n = _nqubit(state)
    if out is None:
        out = state
    broadcast = state.shape[0] == 1 and out.shape[0] > 1
    if known_zero and grads is not None:
        raise ValueError('a reducing pass takes no known-zero bits')
    if slice_bits is not None and (grads is not None or out.shape[0] > MAX_BATCH):
        raise ValueError('a slice of a pass: no reducing pass, at most MAX_BATCH samples')
    if mats.dtype != state.dtype or mats.device != state.device or not mats.is_contiguous():
        raise ValueError('mats must be a contiguous buffer in the dtype/device of the state')
    if grads is not None:
        if (grads.dtype != torch.float64 or grads.ndim != 3 or grads.shape[0] != out.shape[0] or grads.shape[2] != 8
                or not grads.is_contiguous() or grads.device != state.device or broadcast):
            raise ValueError('grads must be a contiguous float64 (batch, rows, 8) accumulator on the device of the state')
    if not _use_hip(state):
        src = state.expand(out.shape[0], -1) if broadcast else state
        if grads is not None:
            return _test_backend.apply_fused(src, mats, mat_batch_stride, desc, out, grads=grads)
        if slice_bits is not None:
            return _test_backend.apply_fused(src, mats, mat_batch_stride, desc, out, known_zero=known_zero, slice_bits=slice_bits)
        if known_zero:
            return _test_backend.apply_fused(src, mats, mat_batch_stride, desc, out, known_zero=known_zero)
        return _test_backend.apply_fused(src, mats, mat_batch_stride, desc, out)
    if grads is not None:
        if out.shape[0] > MAX_BATCH:
            raise ValueError(f'reverse-sweep passes take at most {MAX_BATCH} samples')
        lib = _lib.load()
        rec = _device_records(desc, n, state.device)
        pin_if_capturing(mats, rec)
        if rec is not None:       # more records than the kernel-argument segment holds: the kernel reads them from device memory
            fn = lib.dq_apply_fused_grad_ext_c128 if state.dtype == torch.complex128 else lib.dq_apply_fused_grad_ext_c64
            rc = fn(_ptr(state), _ptr(out), _ptr(mats), int(mat_batch_stride), n, out.shape[0], C.byref(desc), _ptr(rec),
                    rec.numel(), _ptr(grads), grads.shape[1], _stream(state))
            _lib.check(rc, 'dq_apply_fused_grad_ext')
            return out
        fn = lib.dq_apply_fused_grad_c128 if state.dtype == torch.complex128 else lib.dq_apply_fused_grad_c64
        rc = fn(_ptr(state), _ptr(out), _ptr(mats), int(mat_batch_stride), n, out.shape[0], C.byref(desc), _ptr(grads),
                grads.shape[1], _stream(state))
        _lib.check(rc, 'dq_apply_fused_grad')
        return out
    if out.shape[0] > MAX_BATCH:
        rows = mats.reshape(-1, mat_batch_stride) if mat_batch_stride else None
        for lo, hi in _slices(out.shape[0]):
            apply_fused(state if broadcast else state[lo:hi], rows[lo:hi].reshape(-1) if rows is not None else mats,
                        mat_batch_stride, desc, out[lo:hi], known_zero=known_zero)
        return out
    lib = _lib.load()
    pin_if_capturing(mats)
    if slice_bits is not None:
        fn = lib.dq_apply_fused_slice_c128 if state.dtype == torch.complex128 else lib.dq_apply_fused_slice_c64
        rc = fn(_ptr(state), 0 if broadcast else 1 << n, _ptr(out), _ptr(mats), int(mat_batch_stride), n, out.shape[0],
                C.byref(desc), int(known_zero), int(slice_bits[0]), int(slice_bits[1]), _stream(state))
        _lib.check(rc, 'dq_apply_fused_slice')
        return out
    if known_zero:
        fn = lib.dq_apply_fused_zext_c128 if state.dtype == torch.complex128 else lib.dq_apply_fused_zext_c64
        rc = fn(_ptr(state), 0 if broadcast else 1 << n, _ptr(out), _ptr(mats), int(mat_batch_stride), n, out.shape[0],
                C.byref(desc), int(known_zero), _stream(state))
        _lib.check(rc, 'dq_apply_fused_zext')
        return out
    fn = getattr(lib, f'dq_apply_fused_{"bcast_" if broadcast else ""}{_suffix(state)}')
    rc = fn(_ptr(state), _ptr(out), _ptr(mats), int(mat_batch_stride), n, out.shape[0], C.byref(desc),
            _stream(state))
    _lib.check(rc, 'dq_apply_fused')
    return out


def fused_geometry(is_c128: bool, variant: int = 0) -> tuple[int, int, int]:
    """(m, slots, threads) of a compiled fused-kernel variant."""
    if _test_backend is not None and not torch.cuda.is_available():
        return _test_backend.fused_geometry(is_c128, variant)
    lib = _lib.load()
    m, s, t = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.dq_fused_geometry(int(is_c128), variant, C.byref(m), C.byref(s), C.byref(t)),
               'dq_fused_geometry')
    return m.value, s.value, t.value


_ws_cache: dict[tuple, torch.Tensor] = {}


def _workspace(state: torch.Tensor) -> torch.Tensor:
    # one workspace per (device, batch, stream): reductions enqueued on two streams must not share scratch
    stream = torch.cuda.current_stream(state.device).cuda_stream if state.is_cuda else 0
    key = (state.device, state.shape[0], stream)
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = _lib.load().dq_reduce_ws_bytes(state.shape[0])
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=state.device)
        _ws_cache[key] = ws
    return ws


def expect_pauli(state: torch.Tensor, xmask: int, zmask: int) -> torch.Tensor:
    """Re <psi_b|P|psi_b> for the Pauli string (xmask, zmask); a Y sets its bit in both masks.
    Returns float64 (B,)."""
    n = _nqubit(state)
    if not state.is_contiguous():
        raise ValueError('state must be contiguous')
    if not _use_hip(state):
        return _test_backend.expect_pauli(state, xmask, zmask)
    out = torch.empty(state.shape[0], dtype=torch.float64, device=state.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_expect_pauli_{_suffix(state)}')
    rc = fn(_ptr(state), xmask, zmask, n, state.shape[0], _ptr(out), _ptr(_workspace(state)), _stream(state))
    _lib.check(rc, 'dq_expect_pauli')
    return out


def _u64_array(values: Sequence[int]):
    return (C.c_uint64 * max(len(values), 1))(*[int(v) for v in values])


def expect_z_multi(state: torch.Tensor, zmasks: Sequence[int]) -> torch.Tensor:
    """<psi_b| Z-string_k |psi_b> for several Z-type strings in one read of the state per 32 strings:
    float64 (B, K)."""
    n = _nqubit(state)
    if not state.is_contiguous():
        raise ValueError('state must be contiguous')
    if not _use_hip(state):
        return torch.stack([_test_backend.expect_pauli(state, 0, z) for z in zmasks], dim=1)
    lib = _lib.load()
    fn = getattr(lib, f'dq_expect_zmulti_{_suffix(state)}')
    nblocks = max(1, min(2048, (1 << n) // 1024))
    parts = []
    for lo in range(0, len(zmasks), 32):
        grp = zmasks[lo:lo + 32]
        part = torch.empty(state.shape[0], nblocks, len(grp), dtype=torch.float64, device=state.device)
        rc = fn(_ptr(state), _u64_array(grp), len(grp), n, state.shape[0], _ptr(part), nblocks, _stream(state))
        _lib.check(rc, 'dq_expect_zmulti')
        parts.append(part.sum(dim=1))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def scale_z_signs(state: torch.Tensor, zmasks: Sequence[int], coef: torch.Tensor) -> torch.Tensor:
    """(sum_k coef[b, k] Z-string_k) |psi_b>: (B, 2**n) in the state's dtype; coef real (B, K)."""
    n = _nqubit(state)
    if not _use_hip(state):
        with torch.no_grad():
            return _scale_z_signs_double(state, zmasks, coef, n)
    if state.dtype == torch.complex64 and len(zmasks) > 32:
        return _scale_z_signs_wide(state, zmasks, coef, n)      # (several launches: their sum is formed in double)
    fn = getattr(_lib.load(), f'dq_scale_zsigns_{_suffix(state)}')
    out, coef = None, coef.to(torch.float64).contiguous()
    for lo in range(0, len(zmasks), 32):
        grp = zmasks[lo:lo + 32]
        part = torch.empty_like(state)
        rc = fn(_ptr(state), _ptr(part), _u64_array(grp), len(grp), _ptr(coef[:, lo:lo + 32].contiguous()), n,
                state.shape[0], _stream(state))
        _lib.check(rc, 'dq_scale_zsigns')
        out = part if out is None else out.add_(part)
    return out


def _scale_z_signs_double(state, zmasks, coef, n):
    """``scale_z_signs`` for the CPU test double (tests only)."""
    i = torch.arange(1 << n)
    w = torch.zeros(state.shape[0], 1 << n, dtype=torch.float64)
    for k, z in enumerate(zmasks):
        par = torch.zeros_like(i)
        for p in range(n):
            if (z >> p) & 1:
                par ^= (i >> p) & 1
        w += coef[:, k : k + 1].to(torch.float64) * (1 - 2 * par).to(torch.float64)
    return (state * w.to(state.real.dtype)).contiguous()


def inner(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """<bra_b|ket_b> as complex128 (B,).  Inputs (B, count) contiguous, same dtype."""
    if bra.shape != ket.shape or bra.dtype != ket.dtype or bra.ndim != 2:
        raise ValueError('bra/ket must be matching (B, count) tensors')
    if not (bra.is_contiguous() and ket.is_contiguous()):
        raise ValueError('bra/ket must be contiguous')
    if not _use_hip(bra):
        return _test_backend.inner(bra, ket)
    out = torch.empty(bra.shape[0], 2, dtype=torch.float64, device=bra.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_inner_{_suffix(bra)}')
    rc = fn(_ptr(bra), _ptr(ket), bra.shape[1], bra.shape[0], _ptr(out), _ptr(_workspace(bra)), _stream(bra))
    _lib.check(rc, 'dq_inner')
    return torch.view_as_complex(out)


def probs(state: torch.Tensor) -> torch.Tensor:
    """|psi|^2 elementwise in the state's real precision, same shape."""
    if not state.is_contiguous():
        raise ValueError('state must be contiguous')
    if not _use_hip(state):
        return _test_backend.probs(state)
    out = torch.empty(state.shape, dtype=state.real.dtype, device=state.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_probs_{_suffix(state)}')
    _lib.check(fn(_ptr(state), _ptr(out), state.numel(), _stream(state)), 'dq_probs')
    return out


def marginal(state: torch.Tensor, bits: Sequence[int]) -> torch.Tensor:
    """Marginal distribution over ``bits`` (bits[0] = MSB of the outcome index), float64 (B, 2**nw)."""
    n = _nqubit(state)
    bits = [int(b) for b in bits]
    if not _use_hip(state):
        return _test_backend.marginal(state, bits)
    nw = len(bits)
    b = state.shape[0]
    out = torch.zeros(b, 1 << nw, dtype=torch.float64, device=state.device)
    for lo, hi in _slices(b, 65535):                         # (the batch is a grid axis of its own)
        _call('dq_marginal', state, _ptr(state, lo), n, _lib.int_array(bits), nw, hi - lo, _ptr(out, lo))
    return out


def gate_grad(
    x: torch.Tensor, gy: torch.Tensor, targets: Sequence[int], controls: Sequence[int] = ()
) -> torch.Tensor:
    """gU[b] = sum over controlled amplitude groups of gy (outer) conj(x): complex128 (B, D, D)."""
    n = _nqubit(x)
    targets, controls = [int(t) for t in targets], [int(c) for c in controls]
    k = len(targets)
    if x.shape != gy.shape or x.dtype != gy.dtype:
        raise ValueError('x/gy mismatch')
    if not (x.is_contiguous() and gy.is_contiguous()):
        raise ValueError('x/gy must be contiguous')
    if not _use_hip(x):
        return _test_backend.gate_grad(x, gy, targets, controls)
    d = 1 << k
    if RDMK_MIN <= k <= RDMK_MAX:
        return rdmk_cross(x, gy, targets, controls)
    if k > RDMK_MAX:
        # beyond the matrix-core reduction: a plain GEMM (gy_mat @ x_mat^H) left to rocBLAS through torch
        return _gate_grad_gemm(x, gy, n, targets, controls)
    out = torch.zeros(x.shape[0], d, d, 2, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_gate_grad_{_suffix(x)}')
    rc = fn(_ptr(x), _ptr(gy), n, _lib.int_array(targets), k, _lib.int_array(controls), len(controls),
            x.shape[0], _ptr(out), _stream(x))
    _lib.check(rc, 'dq_gate_grad')
    return torch.view_as_complex(out)


def gate_grad_multi(x: torch.Tensor, gy: torch.Tensor, gates: Sequence[tuple[int, Sequence[int]]]) -> torch.Tensor:
    """``gate_grad`` for several single-target gates ``(target, controls)`` on the same pair of states:
    complex128 (B, G, 2, 2).  Gates are packed into as few launches as the kernel's tile allows (each launch reads
    both states once: 8 gates / 7 distinct high targets for complex64, 4 / 7 for complex128); states smaller than a
    tile go gate by gate."""
    n = _nqubit(x)
    if x.shape != gy.shape or x.dtype != gy.dtype or not (x.is_contiguous() and gy.is_contiguous()):
        raise ValueError('x/gy must be contiguous tensors of one shape and dtype')
    is128 = x.dtype == torch.complex128
    tile, per_call, low = (10, 4, 3) if is128 else (11, 8, 4)
    if not _use_hip(x) or n < tile:
        return torch.stack([gate_grad(x, gy, [t], list(c)) for t, c in gates], dim=1)
    nblocks = min(1 << (n - tile), 1536)          # ~6 workgroups per CU striding over the tiles
    parts = []
    lib = _lib.load()
    fn = getattr(lib, f'dq_gate_grad_multi_{_suffix(x)}')
    start = 0
    while start < len(gates):
        stop, high = start, set()
        while stop < len(gates) and stop - start < per_call:
            t = int(gates[stop][0])
            if t >= low and t not in high and len(high) == tile - low:
                break
            if t >= low:
                high.add(t)
            stop += 1
        grp = gates[start:stop]
        begin, bits = [0], []
        for _t, c in grp:
            bits += [int(q) for q in c]
            begin.append(len(bits))
        part = torch.empty(x.shape[0], nblocks, len(grp), 2, 2, 2, dtype=torch.float64, device=x.device)
        rc = fn(_ptr(x), _ptr(gy), n, len(grp), _lib.int_array([int(t) for t, _ in grp]), _lib.int_array(begin),
                _lib.int_array(bits), x.shape[0], _ptr(part), nblocks, _stream(x))
        _lib.check(rc, 'dq_gate_grad_multi')
        parts.append(part.sum(dim=1))
        start = stop
    out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    return torch.view_as_complex(out.contiguous())


RDMK_MIN, RDMK_MAX = 3, 10     # the k-wire cross reduction of dq_rdmk_cross_*


def rdmk_cross(
    x: torch.Tensor, gy: torch.Tensor, targets: Sequence[int], controls: Sequence[int] = ()
) -> torch.Tensor:
    """out[b, a, c] = sum over the controlled amplitude groups of gy[b, a] conj(x[b, c]) for 3 <= k <= 10 targets
    (matrix MSB = targets[0]): complex128 (B, 2^k, 2^k), on the matrix cores without copying the state
    (``dq_rdmk_cross_*``).  ``x is gy`` (the same buffer) is the reduced density matrix of the target wires: half the
    tiles, and the result is exactly Hermitian.  The workspace comes from PyTorch's allocator (legal under capture)."""
    n = _nqubit(x)
    targets, controls = [int(t) for t in targets], [int(c) for c in controls]
    k = len(targets)
    if x.shape != gy.shape or x.dtype != gy.dtype:
        raise ValueError('x/gy must be (batch, 2**n) tensors of one shape and dtype')
    if not (x.is_contiguous() and gy.is_contiguous()):
        raise ValueError('x/gy must be contiguous')
    if not RDMK_MIN <= k <= RDMK_MAX:
        raise ValueError(f'rdmk_cross: {k} targets, supported {RDMK_MIN}..{RDMK_MAX}')
    if not _use_hip(x):
        return _test_backend.gate_grad(x, gy, targets, controls)
    same = x.data_ptr() == gy.data_ptr()
    d = 1 << k
    lib = _lib.load()
    out = torch.empty(x.shape[0], d, d, 2, dtype=torch.float64, device=x.device)
    for lo, hi in _slices(x.shape[0]):
        nbytes = lib.dq_rdmk_ws_bytes(n, k, len(controls), hi - lo, int(x.dtype == torch.complex128), int(same))
        if nbytes < 0:
            raise ValueError(f'rdmk_cross: bad shape (n={n}, k={k}, controls={len(controls)})')
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        _call('dq_rdmk_cross', x, _ptr(x, lo), _ptr(gy, lo), n, _lib.int_array(targets), k, _lib.int_array(controls),
              len(controls), hi - lo, _ptr(out, lo), _ptr(ws), nbytes)
    return torch.view_as_complex(out)


def _gate_grad_gemm(x, gy, n, targets, controls):
    b = x.shape[0]
    wires_t = [n - 1 - t + 1 for t in targets]
    wires_c = [n - 1 - c + 1 for c in controls]
    rest = [i for i in range(1, n + 1) if i not in wires_t and i not in wires_c]
    perm = [0] + wires_t + rest + wires_c
    d = 1 << len(targets)

    def mat(t):
        t = t.reshape([b] + [2] * n).permute(perm).reshape(b, d, -1, 1 << len(controls))
        return t[..., -1]

    return (mat(gy) @ mat(x).mH).to(torch.complex128)


def pack(amps: torch.Tensor, mask: int, value: int) -> torch.Tensor:
    """Gather the sub-cube of each shard whose bits under ``mask`` equal ``value`` into a contiguous
    (B, 2**(nl - popcount(mask))) buffer."""
    nl = _nqubit(amps)
    if not _use_hip(amps):
        return _test_backend.pack(amps, mask, value)
    cnt = 1 << (nl - bin(mask).count('1'))
    out = torch.empty(amps.shape[0], cnt, dtype=amps.dtype, device=amps.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_pack_{_suffix(amps)}')
    _lib.check(fn(_ptr(amps), _ptr(out), nl, mask, value, amps.shape[0], _stream(amps)), 'dq_pack')
    return out


def unpack_axpby(
    amps: torch.Tensor,
    x: torch.Tensor,
    y: torch.Tensor | None,
    coef: torch.Tensor | None,
    mask: int,
    value: int,
) -> torch.Tensor:
    """amps[b, expand(c)] = coef[b,0] * x[b,c] + coef[b,1] * y[b,c] (or = x[b,c] when y is None), where
    expand() re-inserts ``value`` at the ``mask`` bit positions.  In place on ``amps``."""
    nl = _nqubit(amps)
    if not _use_hip(amps):
        return _test_backend.unpack_axpby(amps, x, y, coef, mask, value)
    stride = 0
    if y is not None:
        coef = coef.to(device=amps.device, dtype=amps.dtype).reshape(-1, 2).contiguous()
        if coef.shape[0] not in (1, amps.shape[0]):
            raise ValueError('coef batch mismatch')
        stride = 0 if coef.shape[0] == 1 else 2
    lib = _lib.load()
    fn = getattr(lib, f'dq_unpack_axpby_{_suffix(amps)}')
    rc = fn(_ptr(amps), _ptr(x), _ptr(y), _ptr(coef), stride, nl, mask, value, amps.shape[0], _stream(amps))
    _lib.check(rc, 'dq_unpack_axpby')
    return amps


def defer_rx(flat: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """The deferred form of the uncontrolled Rx-like gates of complex64 passes (include/dq_hip.h, DQ_MODE_RX), in place in
    the kernel matrix buffer ``flat`` (Bm, total): the blocks at the offsets ``index`` (LongTensor on the buffer's
    device; fusion.rx_defer_positions).  One launch (dq_defer_rx_c64); `fusion.defer_rx` is the same rewrite in tensor
    operations (tests and tools compare the two)."""
    if index is None or index.numel() == 0:
        return flat
    if not _use_hip(flat):
        return _test_backend.defer_rx(flat, index)
    assert flat.dtype == torch.complex64 and flat.ndim == 2 and flat.stride(1) == 1 and index.dtype == torch.long
    assert index.device == flat.device and index.is_contiguous()
    pin_if_capturing(index)
    for lo, hi in _slices(flat.shape[0]):                  # (the batch is a grid dimension)
        _call('dq_defer_rx', flat, _ptr(flat, lo), flat.stride(0), _ptr(index), index.numel(), hi - lo)
    return flat


def permute_bits(amps: torch.Tensor, src_of_dst: Sequence[int], out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b, i] = amps[b, sigma(i)], sigma(i) = sum_p bit_p(i) << src_of_dst[p]: re-label the local qubits
    (destination bit p takes the role of source bit src_of_dst[p]).  Out of place."""
    nl = _nqubit(amps)
    src_of_dst = [int(p) for p in src_of_dst]
    if sorted(src_of_dst) != list(range(nl)):
        raise ValueError('src_of_dst must be a permutation of the local bit positions')
    if out is None:
        out = torch.empty_like(amps)
    if not _use_hip(amps):
        return _test_backend.permute_bits(amps, src_of_dst, out)
    lib = _lib.load()
    fn = getattr(lib, f'dq_permute_bits_{_suffix(amps)}')
    _lib.check(fn(_ptr(amps), _ptr(out), nl, _lib.int_array(src_of_dst), amps.shape[0], _stream(amps)), 'dq_permute_bits')
    return out


def interleave(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(B, N), (B, N) -> (B, 2 N) with out[:, 2 i] = a[:, i], out[:, 2 i + 1] = b[:, i]: psi and the cotangent side by side
    along a new index bit 0, as a fused reverse sweep wants them (include/dq_hip.h, dq_interleave_*).  On the test double
    (CPU tensors): torch.stack."""
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device or a.ndim != 2:
        raise ValueError('interleave: two (batch, N) tensors of one dtype on one device')
    if not _use_hip(a) or (a.numel() & 1):
        return torch.stack([a, b], dim=-1).reshape(a.shape[0], -1)
    a, b = a.contiguous(), b.contiguous()
    if (a.data_ptr() | b.data_ptr()) & 15:      # a view at an odd complex64 offset: the kernels read 16-byte pieces
        return torch.stack([a, b], dim=-1).reshape(a.shape[0], -1)
    out = torch.empty(a.shape[0], 2 * a.shape[1], dtype=a.dtype, device=a.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_interleave_{_suffix(a)}')
    _lib.check(fn(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream(a)), 'dq_interleave')
    return out


def deinterleave(pair: torch.Tensor, which: int) -> torch.Tensor:
    """(B, 2 N) -> (B, N): out[:, i] = pair[:, 2 i + which] (dq_deinterleave_*)."""
    if pair.ndim != 2 or pair.shape[1] & 1 or which not in (0, 1):
        raise ValueError('deinterleave: a (batch, 2 N) tensor, which = 0 or 1')
    half = pair.shape[1] // 2
    if not _use_hip(pair) or not pair.is_contiguous() or ((pair.shape[0] * half) & 1) or (pair.data_ptr() & 15):
        return pair.reshape(pair.shape[0], -1, 2)[:, :, which].contiguous()
    out = torch.empty(pair.shape[0], half, dtype=pair.dtype, device=pair.device)
    lib = _lib.load()
    fn = getattr(lib, f'dq_deinterleave_{_suffix(pair)}')
    _lib.check(fn(_ptr(pair), _ptr(out), out.numel(), int(which), _stream(pair)), 'dq_deinterleave')
    return out


# ---------------------------------------------------------------------------------------------------
def rdm1_cross(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """T[b, k, a, c] = sum over the other wires of conj(bra[b, a on wire k, ..]) ket[b, c on wire k, ..] for every wire
    k at once: complex128 (B, n, 2, 2).  ``bra is ket`` reads the state once per pass (``dq_rdm1_cross_*``)."""
    n = _nqubit(ket)
    if bra.shape != ket.shape or bra.dtype != ket.dtype:
        raise ValueError('bra/ket must be (batch, 2**n) tensors of one shape and dtype')
    if not (bra.is_contiguous() and ket.is_contiguous()):
        raise ValueError('bra/ket must be contiguous')
    if not _use_hip(ket):
        return _test_backend.rdm1_cross(bra, ket)
    return _cross_reduce('dq_rdm1_cross', 'dq_rdm1_ws_bytes', bra, ket, (n,), (n, 2, 2))


def _cross_reduce(entry: str, sizer: str, bra: torch.Tensor, ket: torch.Tensor, mid: tuple, shape: tuple[int, ...] = (),
                  sizer_args: tuple = ()) -> torch.Tensor:
    """A cross reduction of the library, ``<entry>_<suffix>(bra, ket, *mid, batch, out, ws, ws_bytes, stream)``, over the
    batch in slices of at most MAX_BATCH samples: complex128 (B, *shape).  Each slice's float64 workspace is sized by
    ``<sizer>(n, batch, is_c128, bra is not ket, *sizer_args)`` and comes from PyTorch's allocator (legal under capture)."""
    n = _nqubit(ket)
    same = bra.data_ptr() == ket.data_ptr()
    out = torch.empty(ket.shape[0], *shape, 2, dtype=torch.float64, device=ket.device)
    for lo, hi in _slices(ket.shape[0]):
        nbytes = getattr(_lib.load(), sizer)(n, hi - lo, int(ket.dtype == torch.complex128), int(not same), *sizer_args)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=ket.device)
        _call(entry, ket, _ptr(bra, lo), _ptr(ket, lo), *mid, hi - lo, _ptr(out, lo), _ptr(ws), nbytes)
    return torch.view_as_complex(out)


def apply_wire_sum(state: torch.Tensor, mats: torch.Tensor) -> torch.Tensor:
    """sum_k (mats[b, k] on wire k) state[b]: the state's dtype, (B, 2**n); ``mats`` complex (B, n, 2, 2)
    (``dq_apply_wire_sum_*``)."""
    n = _nqubit(state)
    if not state.is_contiguous():
        raise ValueError('state must be contiguous')
    if mats.shape != (state.shape[0], n, 2, 2):
        raise ValueError(f'mats must have shape ({state.shape[0]}, {n}, 2, 2), got {tuple(mats.shape)}')
    if not _use_hip(state):
        return _test_backend.apply_wire_sum(state, mats)
    m = torch.view_as_real(mats.to(device=state.device, dtype=torch.complex128).resolve_conj().resolve_neg().contiguous())
    out = torch.empty_like(state)
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_wire_sum', state, _ptr(state, lo), _ptr(out, lo), _ptr(m, lo), n, hi - lo)
    return out


# ---------------------------------------------------------------------------------------------------
_sample_ws_cache: dict[tuple, torch.Tensor] = {}


def _sample_workspace(state: torch.Tensor, batch: int, n: int, nbytes: int) -> torch.Tensor:
    # A tree is cached per (device, batch, n, stream), like `_workspace`: two streams must not share it.  Unlike that
    # scratch a tree is 1.6 % of a complex64 state (34 MiB at n = 28, 545 MiB at batch 16), so a device and stream keep
    # ONE: a call with another (batch, n) drops the tree before it.  The allocator hands the block back to the stream
    # it was allocated on, and a captured graph holds the tree it used through `pin_if_capturing`.
    dev_stream = (state.device, torch.cuda.current_stream(state.device).cuda_stream)
    key = (dev_stream[0], batch, n, dev_stream[1])
    ws = _sample_ws_cache.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():      # (from the graph's pool: it lives with the graph, uncached)
            return torch.empty(nbytes // 8, dtype=torch.float64, device=state.device)
        for k in [k for k in _sample_ws_cache if (k[0], k[3]) == dev_stream]:
            del _sample_ws_cache[k]
        ws = own(torch.empty(nbytes // 8, dtype=torch.float64, device=state.device))
        _sample_ws_cache[key] = ws
    return ws


def clear_sample_workspace() -> None:
    """Drop the cached trees of ``sample_indices`` (one per device and stream, 2^n / 63 doubles per sample): the next
    call builds its own.  For a state that only just fits in memory next to what else is to be allocated."""
    _sample_ws_cache.clear()


def sample_indices(state: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Inverse-CDF samples of |psi|^2 for explicit uniforms: ``out[b, s]`` = the smallest i with
    ``C_b(i) > u[b, s] * T_b``, C_b the running sum of ``|state[b]|^2`` in double and T_b its total (the state need not
    be normalised).  ``state``: (B, 2**n) contiguous complex; ``u``: float64 (B, shots) in [0, 1) on the same device.
    Returns int64 (B, shots) flat indices; an index of probability zero is never returned.  No 2**n-element temporary
    (a tree of partial sums, 1.6 % of a complex64 state), no host synchronisation (``dq_sample_*``).

    The kernel reads the state with 16-byte loads: a state whose first amplitude is not 16-byte aligned (a complex64
    view at an odd storage offset) is refused with the kernel's argument error, not copied -- ``clone()`` it first.
    The tree stays cached for the next call with the same device, batch, n and stream, one per device and stream;
    ``clear_sample_workspace()`` drops it."""
    n = _nqubit(state)
    if not state.is_contiguous():
        raise ValueError('state must be contiguous')
    if u.ndim != 2 or u.shape[0] != state.shape[0] or u.shape[1] < 1 or u.dtype != torch.float64 or u.device != state.device:
        raise ValueError(f'u must be float64 ({state.shape[0]}, shots >= 1) on the device of the state, got '
                         f'{u.dtype} {tuple(u.shape)} on {u.device}')
    if not _use_hip(state):
        _suffix(state)
        with torch.no_grad():
            return _sample_indices_double(state, u)
    u = u.contiguous()
    out = torch.empty(u.shape, dtype=torch.int64, device=state.device)
    for lo, hi in _slices(state.shape[0], 65535):            # (dq_sample_*'s limit on the batch)
        nbytes = _lib.load().dq_sample_ws_bytes(n, hi - lo, int(state.dtype == torch.complex128))
        if nbytes < 0:
            raise ValueError(f'sample_indices: bad shape (n={n}, batch={hi - lo})')
        ws = _sample_workspace(state, hi - lo, n, nbytes)
        pin_if_capturing(ws)
        _call('dq_sample', state, _ptr(state, lo), n, hi - lo, _ptr(u, lo), u.shape[1], _ptr(out, lo), _ptr(ws), nbytes)
    return out


def _sample_indices_double(probs_or_state: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The contract of ``sample_indices`` in torch, for the CPU test double and for the (small) diagonal of a density
    matrix: float64 ``cumsum`` + ``searchsorted(right=True)``, then the clamp onto the last entry of non-zero
    probability.  A real input is taken as the probabilities, a complex one as amplitudes."""
    if probs_or_state.is_complex():
        p = probs_or_state.real.to(torch.float64) ** 2 + probs_or_state.imag.to(torch.float64) ** 2
    else:
        p = probs_or_state.to(torch.float64)
    c = torch.cumsum(p, dim=-1)
    idx = torch.searchsorted(c, (u * c[:, -1:]).contiguous(), right=True)
    # the last index of non-zero probability == the number of entries below the total: nothing beyond it is returned
    last = (c < c[:, -1:]).sum(-1, keepdim=True)
    return torch.minimum(idx, last)


_WIDE_BYTES = 256 << 20


def _scale_z_signs_wide(state: torch.Tensor, zmasks: Sequence[int], coef: torch.Tensor, n: int) -> torch.Tensor:
    """``scale_z_signs`` of a complex64 state with more than 32 strings.  A launch takes 32 strings; adding the launches'
    complex64 results would round three times or more where one launch rounds once.  So a slice at a time is widened,
    goes through the complex128 kernel once per 32 strings, is added up in complex128 and rounded to complex64 once: the
    error of a single launch, at about three times its traffic.

    A slice is about ``_WIDE_BYTES`` of complex128: whole samples, or, where one sample is larger, runs of 2^m amplitudes
    of it -- the sign of the index bits above m is constant over a run and goes into the run's coefficients, exactly.
    Three slices of complex128 (the widened input, the sum, one launch's result) are alive at a time, whatever n."""
    k = len(zmasks)
    m = min(n, max(8, (_WIDE_BYTES // 16).bit_length() - 1))
    coef = coef.to(torch.float64).reshape(state.shape[0], k)
    if m < n:
        h = torch.arange(1 << (n - m), device=state.device)
        par = torch.stack([h & (int(z) >> m) for z in zmasks], dim=1)
        for sh in (32, 16, 8, 4, 2, 1):
            par = par ^ (par >> sh)
        coef = (coef[:, None, :] * (1 - 2 * (par & 1)).to(torch.float64)[None]).reshape(-1, k)
        zmasks = [int(z) & ((1 << m) - 1) for z in zmasks]
    out = torch.empty_like(state)
    src, dst = state.reshape(-1, 1 << m), out.view(-1, 1 << m)
    rows = max(1, min(65535, _WIDE_BYTES // (16 << m)))
    for r0 in range(0, src.shape[0], rows):
        wide = scale_z_signs(src[r0:r0 + rows].to(torch.complex128), zmasks, coef[r0:r0 + rows])
        dst[r0:r0 + rows].copy_(wide)
    return out


# ---------------------------------------------------------------------------------------------------
# Diagonal operators on any number of wires (csrc/dq_diag.hip): table index sub(i) = sum_j bit_{bits[j]}(i) << (k-1-j)
def _distinct_positions(positions: Sequence[int], n: int) -> bool:
    return len(set(positions)) == len(positions) and not any(p < 0 or p >= n for p in positions)


def _check_bra(bra: torch.Tensor, ket: torch.Tensor, what: str) -> None:
    """The bra of a cross reduction of the streaming sections against its (checked) ket: one shape and dtype, contiguous
    (the ket itself: nothing left to check)."""
    if bra is ket:
        return
    if bra.shape != ket.shape or bra.dtype != ket.dtype:
        raise ValueError(f'{what}: bra/ket must be (batch, 2**n) tensors of one shape and dtype')
    if not bra.is_contiguous():
        raise ValueError(f'{what}: bra must be contiguous')


def _diag_args(state: torch.Tensor, bits: Sequence[int], controls: Sequence[int], what: str) -> tuple[int, list[int], list[int]]:
    n = _nqubit(state)
    bits, controls = [int(b) for b in bits], [int(c) for c in controls]
    if not state.is_contiguous():
        raise ValueError(f'{what}: state must be contiguous')
    if not bits:
        raise ValueError(f'{what}: at least one table bit is needed')
    if not _distinct_positions(bits + controls, n):
        raise ValueError(f'{what}: bits {bits} / controls {controls} must be distinct positions in [0, {n})')
    return n, bits, controls


def _diag_table(table: torch.Tensor, like: torch.Tensor, dtype: torch.dtype, k: int, what: str, batched: bool) -> torch.Tensor:
    """The table in ``dtype`` on the state's device, contiguous and 16-byte aligned: (2^k,), or (B, 2^k) when ``batched``
    admits one table per sample."""
    d = 1 << k
    ok = table.shape == (d,) or (batched and table.ndim == 2 and table.shape[1] == d and table.shape[0] in (1, like.shape[0]))
    if not ok:
        raise ValueError(f'{what}: a table over {k} bits has {d} entries' + (f', or ({like.shape[0]}, {d})' if batched else '')
                         + f'; got {tuple(table.shape)}')
    return _finish_table(table, like, dtype, what)


def _sub_index(n: int, bits: Sequence[int], controls: Sequence[int]) -> tuple[torch.Tensor, torch.Tensor]:
    """sub(i) and the control test for every i (CPU test double only)."""
    i = torch.arange(1 << n)
    k = len(bits)
    sub = torch.zeros_like(i)
    for j, p in enumerate(bits):
        sub |= ((i >> p) & 1) << (k - 1 - j)
    cmask = sum(1 << c for c in controls)
    return sub, (i & cmask) == cmask


def apply_diag(state: torch.Tensor, diag: torch.Tensor, bits: Sequence[int], controls: Sequence[int] = (),
               out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b, i] = diag[b, sub(i)] * state[b, i] on the amplitudes whose ``controls`` are all 1 (the others pass through):
    a diagonal operator on k = len(bits) index bits, ``bits[0]`` the most significant bit of the table index, in one read
    and one write of the state (``dq_apply_diag_*``).  ``diag``: complex (2^k,) or (B, 2^k); ``out`` may be ``state``."""
    n, bits, controls = _diag_args(state, bits, controls, 'apply_diag')
    k = len(bits)
    diag = _diag_table(diag, state, state.dtype, k, 'apply_diag', True)
    out = _check_out(state, out, 'apply_diag')
    if not _use_hip(state):
        return _diag_double(lambda: _apply_diag_double(state, diag, n, bits, controls, out))
    stride = (1 << k) if (diag.ndim == 2 and diag.shape[0] > 1) else 0
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_diag', state, _ptr(state, lo), _ptr(out, lo), _ptr(diag, lo if stride else 0), stride, n,
              _lib.int_array(bits), k, _lib.int_array(controls), len(controls), hi - lo)
    return out


def _diag_double(fn):
    """The plain-torch complex128 stand-ins below, for the CPU test double (tests only): like the double itself
    (``_NoGraph``) they build no graph and carry no forward-mode tangent."""
    was = torch._C._is_fwd_grad_enabled()
    torch._C._set_fwd_grad_enabled(False)
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch._C._set_fwd_grad_enabled(was)


def _apply_diag_double(state, diag, n, bits, controls, out):
    k = len(bits)
    sub, ok = _sub_index(n, bits, controls)
    f = diag.reshape(-1, 1 << k).to(torch.complex128)[:, sub]
    out.copy_(torch.where(ok, f * state.to(torch.complex128), state.to(torch.complex128)).to(state.dtype))
    return out


#: complex128 PHASE goes through a table of phases when the table has at most 2^16 entries, the state at least 2^8
#: amplitudes per entry and at least 2^24 amplitudes per sample: the table route is three launches for one, and up to
#: n = 22 it measured 1.2 to 1.6 times slower than forming the phase in flight, at n = 24 1.3 times faster (`apply_cost`;
#: the sweep over n is in DESIGN.md section 4.8)
PHASE_TABLE_MAX_BITS, PHASE_TABLE_MIN_REST, PHASE_TABLE_MIN_QUBITS = 16, 8, 24


def apply_cost(state: torch.Tensor, cost: torch.Tensor, par: torch.Tensor, bits: Sequence[int], controls: Sequence[int] = (),
               op: str = 'phase', out: torch.Tensor | None = None) -> torch.Tensor:
    """A real table ``cost`` (2^k,) over the index bits ``bits`` applied to the state (``dq_apply_cost_*``):

    * ``op='phase'``: out[b, i] = exp(-i par[b] cost[sub(i)]) state[b, i], ``par`` real (B,); amplitudes outside the
      controls pass through.  The angle is formed and reduced in double for both precisions.
    * ``op='scale'``: out[b, i] = par[b] cost[sub(i)] state[b, i], ``par`` complex (B,); amplitudes outside the controls
      come out as 0 (the cotangent of :func:`cost_cross`, which leaves them out)."""
    if op not in ('phase', 'scale'):
        raise ValueError(f"apply_cost: op must be 'phase' or 'scale', got {op!r}")
    n, bits, controls = _diag_args(state, bits, controls, 'apply_cost')
    k = len(bits)
    cost = _diag_table(cost, state, state.real.dtype, k, 'apply_cost', False)
    if par.shape != (state.shape[0],):
        raise ValueError(f'apply_cost: one parameter per sample, ({state.shape[0]},), expected; got {tuple(par.shape)}')
    if op == 'phase' and par.is_complex():
        raise ValueError('apply_cost: the phase parameter is real')
    out = _check_out(state, out, 'apply_cost')
    if not _use_hip(state):
        def double():
            sub, ok = _sub_index(n, bits, controls)
            c = cost.to(torch.float64)[sub]
            x = state.to(torch.complex128)
            if op == 'phase':
                y = torch.where(ok, torch.exp(-1j * par.to(torch.float64).reshape(-1, 1) * c) * x, x)
            else:
                y = torch.where(ok, par.to(torch.complex128).reshape(-1, 1) * c * x, torch.zeros_like(x))
            out.copy_(y.to(state.dtype))
            return out

        return _diag_double(double)
    if op == 'phase':
        p = par.to(device=state.device, dtype=torch.float64).contiguous()
    else:
        p = torch.view_as_real(par.to(device=state.device, dtype=torch.complex128).resolve_conj().resolve_neg().contiguous())
    code = _lib.COST_PHASE if op == 'phase' else _lib.COST_SCALE
    # complex128 phases of a small table: exp(-i t cost) once per table entry and sample -- the same kernel on a vector of
    # ones over the k table bits -- then the diagonal kernel, so that no double-precision sine and cosine is taken per
    # amplitude (measured: DESIGN.md section 4.8).  complex64 forms the phase in flight at every k: it is the faster there.
    via_table = (op == 'phase' and state.dtype == torch.complex128 and k <= PHASE_TABLE_MAX_BITS
                 and n >= max(k + PHASE_TABLE_MIN_REST, PHASE_TABLE_MIN_QUBITS))
    for lo, hi in _slices(state.shape[0]):
        if via_table:
            table = torch.ones(hi - lo, 1 << k, dtype=state.dtype, device=state.device)
            _call('dq_apply_cost', state, _ptr(table), _ptr(table), _ptr(cost), _ptr(p, lo), code, k,
                  _lib.int_array(range(k - 1, -1, -1)), k, _lib.int_array([]), 0, hi - lo)
            _call('dq_apply_diag', state, _ptr(state, lo), _ptr(out, lo), _ptr(table), 1 << k, n, _lib.int_array(bits), k,
                  _lib.int_array(controls), len(controls), hi - lo)
            continue
        _call('dq_apply_cost', state, _ptr(state, lo), _ptr(out, lo), _ptr(cost), _ptr(p, lo), code, n,
              _lib.int_array(bits), k, _lib.int_array(controls), len(controls), hi - lo)
    return out


def cost_cross(bra: torch.Tensor, ket: torch.Tensor, cost: torch.Tensor, bits: Sequence[int],
               controls: Sequence[int] = ()) -> torch.Tensor:
    """out[b] = sum over the amplitudes whose ``controls`` are all 1 of cost[sub(i)] conj(bra[b, i]) ket[b, i]: complex128
    (B,), accumulated in double, bitwise reproducible (``dq_cost_cross_*``).  ``bra`` and ``ket`` the same buffer: one read
    of the state, the expectation value <C>.  The workspace comes from PyTorch's allocator (legal under capture)."""
    n, bits, controls = _diag_args(ket, bits, controls, 'cost_cross')
    k = len(bits)
    _check_bra(bra, ket, 'cost_cross')
    cost = _diag_table(cost, ket, ket.real.dtype, k, 'cost_cross', False)
    if not _use_hip(ket):
        def double():
            sub, ok = _sub_index(n, bits, controls)
            w = cost.to(torch.float64)[sub] * ok
            return (w * bra.to(torch.complex128).conj() * ket.to(torch.complex128)).sum(dim=-1)

        return _diag_double(double)
    mid = (_ptr(cost), n, _lib.int_array(bits), k, _lib.int_array(controls), len(controls))
    return _cross_reduce('dq_cost_cross', 'dq_cost_cross_ws_bytes', bra, ket, mid)


# ---------------------------------------------------------------------------------------------------
# Pauli strings on any number of wires (csrc/dq_pauli.hip): (P psi)[i] = i^ny (-1)^popc((i ^ x) & z) psi[i ^ x]
def _support_args(state: torch.Tensor, controls: Sequence[int], support: int, named: str, what: str) -> tuple[int, list[int]]:
    """What the Pauli and the excitation entry points ask alike, before their own mask checks: a contiguous state and
    controls that are distinct positions of it outside the generator's mask ``support`` (``named``: what the message calls
    it, with a place for the mask)."""
    n = _nqubit(state)
    controls = [int(c) for c in controls]
    if not state.is_contiguous():
        raise ValueError(f'{what}: state must be contiguous')
    if controls:
        if len(set(controls)) != len(controls) or min(controls) < 0 or max(controls) >= n:
            raise ValueError(f'{what}: controls {controls} must be distinct positions in [0, {n})')
        cmask = 0
        for c in controls:
            cmask |= 1 << c
        if support & cmask:
            raise ValueError(f'{what}: controls {controls} must be disjoint from {named.format(support)}')
    return n, controls


def _pauli_args(state: torch.Tensor, xmask: int, zmask: int, controls: Sequence[int], what: str) -> tuple[int, int, int, list[int]]:
    xmask, zmask = int(xmask), int(zmask)
    n, controls = _support_args(state, controls, xmask | zmask, 'the Pauli string ({:#x})', what)
    if xmask < 0 or zmask < 0 or (xmask | zmask) >> n:
        raise ValueError(f'{what}: xmask={xmask:#x} / zmask={zmask:#x} must lie in [0, 2**{n})')
    return n, xmask, zmask, controls


def _pauli_coef(p, like: torch.Tensor, what: str) -> torch.Tensor:
    """One complex coefficient, or one per sample, as complex128 (B,) on the state's device."""
    p = torch.as_tensor(p, device=like.device).to(torch.complex128).reshape(-1)
    if p.shape[0] == 1 and like.shape[0] != 1:
        p = p.expand(like.shape[0])
    if p.shape[0] != like.shape[0]:
        raise ValueError(f'{what}: one coefficient, or one per sample ({like.shape[0]}), expected; got {p.shape[0]}')
    return p.resolve_conj().resolve_neg()


def _axpby_coef(a: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """(B, 4) float64 rows (Re a, Im a, Re c, Im c): what the axpby kernels read."""
    return torch.view_as_real(torch.stack([a, c], dim=1)).reshape(-1, 4).contiguous()


def _real_angles(theta: torch.Tensor, state: torch.Tensor, what: str) -> torch.Tensor:
    """One real angle per sample, as float64 on the state's device."""
    if theta.is_complex() or theta.shape != (state.shape[0],):
        raise ValueError(f'{what}: one real angle per sample, ({state.shape[0]},), expected; got '
                         f'{theta.dtype} {tuple(theta.shape)}')
    return theta.to(device=state.device, dtype=torch.float64)


def _pauli_gather(n: int, xmask: int, zmask: int, controls: Sequence[int]) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Source index i ^ x, factor i^ny (-1)^popc((i ^ x) & z) and the control test for every i (CPU test double only)."""
    i = torch.arange(1 << n)
    j = i ^ xmask
    par = j & zmask
    for sh in (32, 16, 8, 4, 2, 1):
        par = par ^ (par >> sh)
    factor = (1j ** (bin(xmask & zmask).count('1') % 4)) * (1 - 2 * (par & 1)).to(torch.complex128)
    cmask = sum(1 << c for c in controls)
    return j, factor, (i & cmask) == cmask


def apply_pauli_axpby(state: torch.Tensor, xmask: int, zmask: int, a, c, controls: Sequence[int] = (), mode: str = 'gate',
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b] = a[b] state[b] + c[b] P state[b] for the Pauli string P = (xmask, zmask) -- a Y sets its bit in both -- on
    the amplitudes whose ``controls`` are all 1, in one read and one write of the state whatever the weight of P
    (``dq_apply_pauli_axpby_*``).  ``a``, ``c``: complex, one value or one per sample.

    * ``mode='gate'``: amplitudes outside the controls pass through.
    * ``mode='map'``: they come out as 0 (the cotangent of :func:`pauli_cross`, which leaves them out).

    ``out`` may be ``state``."""
    if mode not in ('gate', 'map'):
        raise ValueError(f"apply_pauli_axpby: mode must be 'gate' or 'map', got {mode!r}")
    n, xmask, zmask, controls = _pauli_args(state, xmask, zmask, controls, 'apply_pauli_axpby')
    a, c = _pauli_coef(a, state, 'apply_pauli_axpby'), _pauli_coef(c, state, 'apply_pauli_axpby')
    out = _check_out(state, out, 'apply_pauli_axpby')
    if not _use_hip(state):
        def double():
            j, factor, ok = _pauli_gather(n, xmask, zmask, controls)
            x = state.to(torch.complex128)
            y = a.reshape(-1, 1) * x + c.reshape(-1, 1) * factor * x[:, j]
            out.copy_(torch.where(ok, y, x if mode == 'gate' else torch.zeros_like(x)).to(state.dtype))
            return out

        return _diag_double(double)
    return _pauli_launch(state, out, xmask, zmask, _axpby_coef(a, c), _lib.PAULI_GATE if mode == 'gate' else _lib.PAULI_MAP, n, controls)


def _pauli_launch(state, out, xmask, zmask, coef, code, n, controls):
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_pauli_axpby', state, _ptr(state, lo), _ptr(out, lo), xmask, zmask, _ptr(coef, lo), code, n,
              _lib.int_array(controls), len(controls), hi - lo)
    return out


def apply_pauli_rot(state: torch.Tensor, xmask: int, zmask: int, theta: torch.Tensor, controls: Sequence[int] = (),
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """exp(-i theta/2 P) state: :func:`apply_pauli_axpby` in 'gate' mode with a = cos(theta/2), c = -i sin(theta/2), the
    four real coefficients formed in double from the real ``theta`` (B,) without a detour through complex tensors."""
    n, xmask, zmask, controls = _pauli_args(state, xmask, zmask, controls, 'apply_pauli_rot')
    half = _real_angles(theta, state, 'apply_pauli_rot') * 0.5
    if not _use_hip(state):
        return apply_pauli_axpby(state, xmask, zmask, torch.cos(half), -1j * torch.sin(half), controls, 'gate', out)
    out = _check_out(state, out, 'apply_pauli_rot')
    zero = torch.zeros_like(half)
    coef = torch.stack([torch.cos(half), zero, zero, -torch.sin(half)], dim=1)
    return _pauli_launch(state, out, xmask, zmask, coef, _lib.PAULI_GATE, n, controls)


def pauli_cross(bra: torch.Tensor, ket: torch.Tensor, xmask: int, zmask: int, controls: Sequence[int] = ()) -> torch.Tensor:
    """out[b] = sum over the amplitudes whose ``controls`` are all 1 of conj(bra[b, i]) (P ket[b])[i]: complex128 (B,),
    accumulated in double, bitwise reproducible (``dq_pauli_cross_*``).  ``bra`` and ``ket`` the same buffer: one read of
    the state.  ``xmask = zmask = 0``: the inner product over the controlled amplitudes.  The workspace comes from
    PyTorch's allocator (legal under capture)."""
    n, xmask, zmask, controls = _pauli_args(ket, xmask, zmask, controls, 'pauli_cross')
    _check_bra(bra, ket, 'pauli_cross')
    if not _use_hip(ket):
        def double():
            j, factor, ok = _pauli_gather(n, xmask, zmask, controls)
            return (ok * bra.to(torch.complex128).conj() * factor * ket.to(torch.complex128)[:, j]).sum(dim=-1)

        return _diag_double(double)
    mid = (xmask, zmask, n, _lib.int_array(controls), len(controls))
    return _cross_reduce('dq_pauli_cross', 'dq_pauli_cross_ws_bytes', bra, ket, mid)


# ---------------------------------------------------------------------------------------------------
# Basis-state permutations on any number of wires (csrc/dq_perm.hip): out[b, j] = in[b, put(j, src[sub(j)])], where
# put(j, v) is j with the table bits replaced by the bits of v
PERM_PATHS = {'auto': _lib.PERM_AUTO, 'gather': _lib.PERM_GATHER, 'local': _lib.PERM_LOCAL}
PERM_MAX_BITS = 31


def permutation_local_bits(dtype: torch.dtype) -> int:
    """log2 of the amplitudes of a chunk of the 'local' path: every table bit must lie below it."""
    return _lib.load().dq_permutation_local_bits(int(dtype == torch.complex128))


def _perm_table(src: torch.Tensor, like: torch.Tensor, k: int, what: str) -> torch.Tensor:
    """The table as int32 on the state's device, contiguous and 16-byte aligned.  Its entries are not looked at here (no
    synchronisation): the kernels mask them to k bits, and whoever builds a table checks that it is a bijection
    (``PermutationGate``)."""
    if not isinstance(src, torch.Tensor) or src.is_floating_point() or src.is_complex() or src.dtype == torch.bool:
        raise ValueError(f'{what}: the table must be an integer tensor')
    if src.shape != (1 << k,):
        raise ValueError(f'{what}: a table over {k} bits has {1 << k} entries; got {tuple(src.shape)}')
    return _finish_table(src, like, torch.int32, what)


def apply_permutation(state: torch.Tensor, src: torch.Tensor, bits: Sequence[int], controls: Sequence[int] = (),
                      out: torch.Tensor | None = None, path: str = 'auto') -> torch.Tensor:
    """out[b, j] = state[b, put(j, src[sub(j)])] on the amplitudes whose ``controls`` are all 1 (the others are copied): the
    basis-state permutation |x> -> |perm(x)> on k = len(bits) index bits in gather form, ``src`` = perm^-1 an integer table
    of 2^k entries, ``bits[0]`` the most significant bit of its index -- one read and one write of the state, amplitudes
    copied bit for bit (``dq_apply_permutation_*``).  Out of place only: ``out`` must not overlap ``state``.  ``path``:
    'gather', 'local' (every table bit below :func:`permutation_local_bits`) or 'auto'."""
    n, bits, controls = _diag_args(state, bits, controls, 'apply_permutation')
    k = len(bits)
    if k > PERM_MAX_BITS:
        raise ValueError(f'apply_permutation: at most {PERM_MAX_BITS} table bits, got {k}')
    if path not in PERM_PATHS:
        raise ValueError(f"apply_permutation: path must be 'auto', 'gather' or 'local', got {path!r}")
    _suffix(state)
    src = _perm_table(src, state, k, 'apply_permutation')
    out = _check_out(state, out, 'apply_permutation', in_place=False)
    if path == 'local' and max(bits) >= permutation_local_bits(state.dtype):
        raise ValueError(f"apply_permutation: path='local' needs every table bit below "
                         f'{permutation_local_bits(state.dtype)}, got {bits}')
    if not _use_hip(state):
        return _diag_double(lambda: _apply_permutation_double(state, src, n, bits, controls, out))
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_permutation', state, _ptr(state, lo), _ptr(out, lo), _ptr(src), n, _lib.int_array(bits), k,
              _lib.int_array(controls), len(controls), hi - lo, PERM_PATHS[path])
    return out


def _apply_permutation_double(state, src, n, bits, controls, out):
    k = len(bits)
    sub, ok = _sub_index(n, bits, controls)
    v = src.to(torch.int64)[sub] & ((1 << k) - 1)
    i = torch.arange(1 << n)
    index = i & ~sum(1 << p for p in bits)
    for j, p in enumerate(bits):
        index = index | (((v >> (k - 1 - j)) & 1) << p)
    out.copy_(state[:, torch.where(ok, index, i)])
    return out


# ---------------------------------------------------------------------------------------------------
# SELECT over Pauli strings (csrc/dq_select.hip): out[b, i] = i^q (-1)^popc(j & z) in[b, j], j = i ^ x, with
# (x, z, q) = table[sub(i)] read from the select bits of i and x confined to the bits that are neither select nor control
SELECT_MAX_BITS = 31


def select_pauli_unit_bits(dtype: torch.dtype) -> int:
    """log2 of the amplitudes of a unit of the SELECT kernel: select bits at or above it are uniform over a workgroup."""
    return _lib.load().dq_select_pauli_unit_bits(int(dtype == torch.complex128))


class SelectTable:
    """The two tables of ``dq_apply_select_pauli_*`` for ``sum_s |s><s| (x) i^q_s P_s`` on a register of ``nqubit`` wires,
    from one ``(xmask, zmask, q)`` per value s of the select bits: masks over index bits as include/dq_hip.h section 14
    describes them, ``q`` the power of i in front of the string, 2^k entries.  The kernel's entry holds the power of i in
    front of ``X^x Z^z``: with ``ny = popc(x & z)`` Y factors that is ``q + ny`` for the operator and, P_s being Hermitian,
    ``ny - q`` for its adjoint -- both tables are built here, once, as int64 tensors (2^k, 2) = (x | q << 62, z), kept on
    the CPU and handed out per device by :meth:`on` (cached; the first use on a device copies them, which a graph capture
    does not allow: run once before capturing).  Pickles without the device copies."""

    def __init__(self, nqubit: int, entries: Sequence[tuple[int, int, int]]):
        n, size = int(nqubit), len(entries)
        if n < 1 or n > 40:
            raise ValueError(f'SelectTable: nqubit={nqubit} out of range [1, 40]')
        k = size.bit_length() - 1
        if size < 2 or (1 << k) != size or k > SELECT_MAX_BITS:
            raise ValueError(f'SelectTable: a table over k select bits has 2^k entries, 1 <= k <= {SELECT_MAX_BITS}; got {size}')
        forward, dagger = [], []
        for x, z, q in entries:
            x, z, q = int(x), int(z), int(q)
            if x < 0 or z < 0 or x >> n or z >> n:
                raise ValueError(f'SelectTable: every mask must lie in [0, 2**{n})')
            if q < 0 or q > 3:
                raise ValueError(f'SelectTable: a phase is a power of i in 0..3, got {q}')
            ny = bin(x & z).count('1')
            forward.append((x | ((q + ny) % 4) << 62, z))
            dagger.append((x | ((ny - q) % 4) << 62, z))
        self.nqubit, self.k = n, k
        signed = lambda rows: torch.tensor([[w - (1 << 64) if w >> 63 else w for w in row] for row in rows], dtype=torch.int64)
        self._host = (signed(forward), signed(dagger))
        self._devices: dict = {}

    def on(self, device, dagger: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
        """(table, table of the adjoint) on ``device``; ``dagger``: the other way round."""
        device = torch.device(device)
        hit = self._host if device.type == 'cpu' else self._devices.get(device)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('deepquantum_amd: the first use of a SELECT table on a device copies it there; run the '
                                   'step once before capturing it (dq.CapturedGraph warms up by itself)')
            hit = self._devices[device] = tuple(own(t.to(device)) for t in self._host)
        pin_if_capturing(*hit)
        return (hit[1], hit[0]) if dagger else hit

    def __getstate__(self):
        return {**self.__dict__, '_devices': {}}


def _select_words(words: torch.Tensor, like: torch.Tensor, k: int, what: str) -> torch.Tensor:
    """The table as int64 (2^k, 2) on the state's device, contiguous and 16-byte aligned.  Its entries are not looked at
    here (no synchronisation): the kernel confines every flip mask to the free bits."""
    if not isinstance(words, torch.Tensor) or words.dtype != torch.int64:
        raise ValueError(f'{what}: the table must be an int64 tensor (SelectTable.on)')
    if words.shape != (1 << k, 2):
        raise ValueError(f'{what}: a table over {k} select bits has shape ({1 << k}, 2); got {tuple(words.shape)}')
    return _finish_table(words, like, torch.int64, what)


def apply_select_pauli(state: torch.Tensor, table_words: torch.Tensor, bits: Sequence[int], controls: Sequence[int] = (),
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b, i] = i^q (-1)^popc(j & z) state[b, j], j = i ^ x, with (x, z, q) = table[sub(i)], on the amplitudes whose
    ``controls`` are all 1 (the others are copied): SELECT over the Pauli strings of ``table_words`` (one of
    :meth:`SelectTable.on`) for k = len(bits) select bits, ``bits[0]`` the most significant bit of s -- one read and one
    write of the state whatever the number of strings, exact (``dq_apply_select_pauli_*``).  Out of place only: ``out``
    must not overlap ``state``."""
    what = 'apply_select_pauli'
    n, bits, controls = _diag_args(state, bits, controls, what)
    k = len(bits)
    if k > SELECT_MAX_BITS:
        raise ValueError(f'{what}: at most {SELECT_MAX_BITS} select bits, got {k}')
    _suffix(state)
    words = _select_words(table_words, state, k, what)
    out = _check_out(state, out, what, in_place=False)
    if not _use_hip(state):
        return _diag_double(lambda: _apply_select_pauli_double(state, words, n, bits, controls, out))
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_select_pauli', state, _ptr(state, lo), _ptr(out, lo), _ptr(words), n, _lib.int_array(bits), k,
              _lib.int_array(controls), len(controls), hi - lo)
    return out


def _apply_select_pauli_double(state, words, n, bits, controls, out):
    sub, ok = _sub_index(n, bits, controls)
    i = torch.arange(1 << n)
    free = ((1 << n) - 1) & ~sum(1 << p for p in [*bits, *controls])
    w0, z = words[sub, 0], words[sub, 1]
    j = i ^ (w0 & free)
    par = torch.zeros_like(i)
    for p in range(n):
        par ^= ((j & z) >> p) & 1
    q = torch.where(ok, ((w0 >> 62) + 2 * par) & 3, 0)
    factor = torch.tensor([1, 1j, -1, -1j], dtype=state.dtype)[q]
    out.copy_(state[:, torch.where(ok, j, i)] * factor)
    return out


# ---------------------------------------------------------------------------------------------------
# Multiplexed one-qubit gates on any number of select wires (csrc/dq_mux.hip): for every pair i0 (target bit 0),
# i1 = i0 | 1 << target inside the controls, (out[i0], out[i1]) = M[sub(i0)] (in[i0], in[i1])
MUX_KINDS = {'u': _lib.MUX_U, 'ry': _lib.MUX_RY}


def _mux_table(table: torch.Tensor, like: torch.Tensor, kind: str, k: int, what: str) -> torch.Tensor:
    """The table in the state's precision on its device, contiguous and 16-byte aligned: complex (2^k, 2, 2) for 'u', real
    (2^k, 2) rows (c, s) for 'ry'.  Its entries are not looked at here (no synchronisation)."""
    if not isinstance(table, torch.Tensor):
        raise ValueError(f'{what}: the table must be a tensor, got {type(table).__name__}')
    d = 1 << k
    if kind == 'u':
        if table.shape != (d, 2, 2) or not table.is_complex():
            raise ValueError(f"{what}: a 'u' table over {k} select bits is complex ({d}, 2, 2); got {table.dtype} "
                             f'{tuple(table.shape)}')
        dtype = like.dtype
    else:
        if table.shape != (d, 2) or not table.is_floating_point():
            raise ValueError(f"{what}: an 'ry' table over {k} select bits is real ({d}, 2), rows (c, s); got {table.dtype} "
                             f'{tuple(table.shape)}')
        dtype = torch.float64 if like.dtype == torch.complex128 else torch.float32
    return _finish_table(table, like, dtype, what)


def apply_mux(state: torch.Tensor, table: torch.Tensor, kind: str, target: int, bits: Sequence[int], controls: Sequence[int] = (),
              dagger: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """A multiplexed (uniformly controlled) one-qubit gate: for every value s = sub(i) of the k = len(bits) select bits
    (``bits[0]`` the most significant bit of s) the 2x2 matrix M[s] on index bit ``target``, on the amplitudes whose
    ``controls`` are all 1 (the others pass through bitwise) -- one read and one write of the state whatever k is
    (``dq_apply_mux_*``).  ``kind='u'``: ``table`` complex (2^k, 2, 2); ``kind='ry'``: real (2^k, 2) rows (c, s) for
    M = [[c, -s], [s, c]].  One table for the whole batch.  ``dagger`` applies the conjugate transpose of every entry from
    the same table.  ``out`` may be ``state``."""
    what = 'apply_mux'
    if kind not in MUX_KINDS:
        raise ValueError(f"{what}: kind must be 'u' or 'ry', got {kind!r}")
    n, bits, controls = _diag_args(state, bits, controls, what)
    target = int(target)
    if not _distinct_positions(bits + controls + [target], n):
        raise ValueError(f'{what}: target {target} / bits {bits} / controls {controls} must be distinct positions in [0, {n})')
    k = len(bits)
    _suffix(state)
    table = _mux_table(table, state, kind, k, what)
    out = _check_out(state, out, what)
    if not _use_hip(state):
        return _diag_double(lambda: _apply_mux_double(state, table, kind, n, target, bits, controls, bool(dagger), out))
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_mux', state, _ptr(state, lo), _ptr(out, lo), _ptr(table), MUX_KINDS[kind], int(bool(dagger)), n,
              target, _lib.int_array(bits), k, _lib.int_array(controls), len(controls), hi - lo)
    return out


def _apply_mux_double(state, table, kind, n, target, bits, controls, dagger, out):
    sub, ok = _sub_index(n, bits, controls)
    if kind == 'ry':
        c, s = table[:, 0].to(torch.complex128), table[:, 1].to(torch.complex128)
        m = torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)
    else:
        m = table.to(torch.complex128)
    if dagger:
        m = m.mH.resolve_conj()
    m = m[sub]                                          # (2^n, 2, 2)
    i = torch.arange(1 << n)
    x = state.to(torch.complex128)
    x0, x1 = x[:, i & ~(1 << target)], x[:, i | (1 << target)]
    t = (i >> target) & 1
    row = m[i, t]                                       # (2^n, 2): the row of M that makes amplitude i
    out.copy_(torch.where(ok, row[:, 0] * x0 + row[:, 1] * x1, x).to(state.dtype))
    return out


def mux_cross(bra: torch.Tensor, ket: torch.Tensor, axis: str, target: int, bits: Sequence[int],
              controls: Sequence[int] = ()) -> torch.Tensor:
    """out[b, s] = sum over the amplitudes i with sub(i) = s whose ``controls`` are all 1 of conj(bra[b, i]) (G ket[b])[i],
    G the one-qubit Pauli ``axis`` ('i', 'x', 'y', 'z') on index bit ``target`` and sub() over the k = len(bits) select
    bits as in :func:`apply_mux`: complex128 (B, 2^k), accumulated in double, bitwise reproducible bin by bin, one read of
    each state whatever k is (``dq_mux_cross_*``).  ``bra`` and ``ket`` the same buffer: one read of the state.  The
    workspace comes from PyTorch's allocator (legal under capture)."""
    what = 'mux_cross'
    if axis not in _lib.MUX_AXES:
        raise ValueError(f"{what}: axis must be 'i', 'x', 'y' or 'z', got {axis!r}")
    n, bits, controls = _diag_args(ket, bits, controls, what)
    target = int(target)
    if not _distinct_positions(bits + controls + [target], n):
        raise ValueError(f'{what}: target {target} / bits {bits} / controls {controls} must be distinct positions in [0, {n})')
    k = len(bits)
    _suffix(ket)
    _check_bra(bra, ket, what)
    if not _use_hip(ket):
        return _diag_double(lambda: _mux_cross_double(bra, ket, axis, n, target, bits, controls))
    mid = (_lib.MUX_AXES[axis], n, target, _lib.int_array(bits), k, _lib.int_array(controls), len(controls))
    return _cross_reduce('dq_mux_cross', 'dq_mux_cross_ws_bytes', bra, ket, mid, (1 << k,), sizer_args=(k,))


def _mux_coef(p, state: torch.Tensor, k: int, dtype: torch.dtype, what: str) -> torch.Tensor:
    """One value per select value, shared by the batch (2^k,) / (1, 2^k) or per sample (B, 2^k): (1 or B, 2^k) in ``dtype``
    on the state's device."""
    p = torch.as_tensor(p, device=state.device)
    if p.is_complex() and not dtype.is_complex:
        raise ValueError(f'{what}: real angles expected, got {p.dtype}')
    p = p.to(dtype)
    if p.ndim == 1:
        p = p.unsqueeze(0)
    if p.ndim != 2 or p.shape[1] != 1 << k or p.shape[0] not in (1, state.shape[0]):
        raise ValueError(f'{what}: {k} select bits take ({1 << k},) values, or ({state.shape[0]}, {1 << k}) for one row per '
                         f'sample; got {tuple(p.shape)}')
    return p.resolve_conj().resolve_neg()


def _mux_launch(state: torch.Tensor, tables: torch.Tensor, kind: str, target: int, bits, controls) -> torch.Tensor:
    """``apply_mux`` with one table for the batch (``tables.shape[0] == 1``: one launch) or one per sample (one launch per
    sample: the route of second and higher derivatives, tested and not tuned)."""
    if tables.shape[0] == 1:
        return apply_mux(state, tables[0], kind, target, bits, controls)
    out = torch.empty_like(state)
    for b in range(state.shape[0]):
        apply_mux(state[b:b + 1], tables[b], kind, target, bits, controls, out=out[b:b + 1])
    return out


def apply_mux_axpby(state: torch.Tensor, a, c, axis: str, target: int, bits: Sequence[int], controls: Sequence[int] = (),
                    mode: str = 'gate') -> torch.Tensor:
    """out[b, i] = a[b, sub(i)] state[b, i] + c[b, sub(i)] (G state[b])[i] on the amplitudes whose ``controls`` are all 1, G
    the one-qubit Pauli ``axis`` ('i', 'x', 'y', 'z') on index bit ``target``; ``a``, ``c`` complex, (2^k,) for the batch or
    (B, 2^k) per sample.  Runs on ``dq_apply_mux_*`` with the table of the blocks a[s] I + c[s] sigma.

    * ``mode='gate'``: amplitudes outside the controls pass through.
    * ``mode='map'``: they come out as 0 (the cotangent of :func:`mux_cross`, which leaves them out): the controls become
      further select bits whose other entries are 0.

    Per-sample coefficients run one launch per sample."""
    what = 'apply_mux_axpby'
    if mode not in ('gate', 'map'):
        raise ValueError(f"{what}: mode must be 'gate' or 'map', got {mode!r}")
    if axis not in _lib.MUX_AXES:
        raise ValueError(f"{what}: axis must be 'i', 'x', 'y' or 'z', got {axis!r}")
    _n, bits, controls = _diag_args(state, bits, controls, what)
    k = len(bits)
    a, c = _mux_coef(a, state, k, torch.complex128, what), _mux_coef(c, state, k, torch.complex128, what)
    zero = torch.zeros_like(a + c)
    if axis == 'i':
        m = (a + c, zero, zero, a + c)
    elif axis == 'x':
        m = (a + zero, c + zero, c + zero, a + zero)
    elif axis == 'y':
        m = (a + zero, -1j * c + zero, 1j * c + zero, a + zero)
    else:
        m = (a + c, zero, zero, a - c)
    m = torch.stack(m, dim=-1)                          # (1 or B, 2^k, 4)
    if mode == 'map' and controls:
        full = m.new_zeros(m.shape[0], 1 << k, 1 << len(controls), 4)
        full[:, :, -1] = m
        m, bits, controls = full, bits + controls, []
    return _mux_launch(state, m.reshape(m.shape[0], -1, 2, 2).to(state.dtype), 'u', int(target), bits, controls)


def apply_mux_rot(state: torch.Tensor, theta, axis: str, target: int, bits: Sequence[int],
                  controls: Sequence[int] = ()) -> torch.Tensor:
    """R_axis(theta[b, sub(i)]) on index bit ``target``, ``axis`` one of 'x', 'y', 'z': :func:`apply_mux_axpby` in 'gate'
    mode with a = cos(theta/2), c = -i sin(theta/2), formed in double from the real ``theta`` -- (2^k,) or (B, 2^k); about
    y the real ``DQ_MUX_RY`` table of rows (cos, sin)."""
    what = 'apply_mux_rot'
    if axis not in ('x', 'y', 'z'):
        raise ValueError(f"{what}: axis must be 'x', 'y' or 'z', got {axis!r}")
    _n, bits, controls = _diag_args(state, bits, controls, what)
    half = _mux_coef(theta, state, len(bits), torch.float64, what) * 0.5
    if axis != 'y':
        return apply_mux_axpby(state, torch.cos(half), -1j * torch.sin(half), axis, target, bits, controls, 'gate')
    return _mux_launch(state, torch.stack([torch.cos(half), torch.sin(half)], dim=-1), 'ry', int(target), bits, controls)


def _mux_cross_double(bra, ket, axis, n, target, bits, controls):
    sub, ok = _sub_index(n, bits, controls)
    i = torch.arange(1 << n)
    v = ket.to(torch.complex128)
    t = (i >> target) & 1
    if axis in 'xy':
        v = v[:, i ^ (1 << target)]
    if axis == 'y':
        v = v * (1j * (2 * t - 1)).to(torch.complex128)             # (Y v)_0 = -i v_1, (Y v)_1 = i v_0
    elif axis == 'z':
        v = v * (1 - 2 * t).to(torch.complex128)
    terms = torch.where(ok, bra.to(torch.complex128).conj() * v, torch.zeros((), dtype=torch.complex128))
    out = torch.zeros(ket.shape[0], 1 << len(bits), dtype=torch.complex128)
    return out.index_add_(1, sub, terms)


# ---------------------------------------------------------------------------------------------------
# Excitation gates that touch only their subspace (csrc/dq_excite.hip).  A spec is (xmask, amask, zmask, negate) or
# (xmask, amask, zmask, negate, controls) over index bits: for every i0 with i0 & xmask == amask inside the controls,
# i1 = i0 ^ xmask and sigma = (-1)^(negate + popc(i0 & zmask)): (K x)[i1] = sigma x[i0], (K x)[i0] = -sigma x[i1], 0 elsewhere
def _excite_args(state: torch.Tensor, spec, what: str) -> tuple[int, int, int, int, int, list[int]]:
    if not isinstance(spec, (tuple, list)) or len(spec) not in (4, 5):
        raise ValueError(f'{what}: a spec is (xmask, amask, zmask, negate[, controls]), got {spec!r}')
    xmask, amask, zmask, negate = (int(v) for v in spec[:4])
    n, controls = _support_args(state, spec[4] if len(spec) == 5 else (), xmask | zmask,
                                'xmask | zmask ({:#x}): fold fixed bits into negate', what)
    _suffix(state)
    if xmask <= 0 or amask < 0 or zmask < 0 or (xmask | zmask) >> n:
        raise ValueError(f'{what}: xmask={xmask:#x} must lie in [1, 2**{n}), zmask={zmask:#x} in [0, 2**{n})')
    if amask & ~xmask:
        raise ValueError(f'{what}: amask={amask:#x} must be a subset of xmask={xmask:#x}')
    if zmask & xmask:
        raise ValueError(f'{what}: zmask={zmask:#x} and xmask={xmask:#x} share a bit: fold fixed bits into negate')
    if negate not in (0, 1):
        raise ValueError(f'{what}: negate must be 0 or 1, got {negate}')
    return n, xmask, amask, zmask, negate, controls


def _excite_pairs(n: int, xmask: int, amask: int, zmask: int, negate: int, controls: Sequence[int]):
    """i0, i1 and sigma of every pair (CPU test double only)."""
    i = torch.arange(1 << n)
    cmask = sum(1 << c for c in controls)
    i0 = i[(i & (xmask | cmask)) == (amask | cmask)]
    par = i0 & zmask
    for sh in (32, 16, 8, 4, 2, 1):
        par = par ^ (par >> sh)
    sigma = (1 - 2 * ((par & 1) ^ negate)).to(torch.complex128)
    return i0, i0 ^ xmask, sigma


def apply_excite_axpby(state: torch.Tensor, spec, a, c, mode: str = 'gate', out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b] = a[b] state[b] + c[b] K state[b] on the pairs of the excitation ``spec`` -- 2 / 2^(popc(xmask) + controls) of
    the state -- (``dq_apply_excite_axpby_*``).  ``a``, ``c``: complex, one value or one per sample.  Outside the pairs:

    * ``mode='gate'``: the amplitudes pass through bitwise (``a = cos t, c = sin t`` is ``exp(t K)``).
    * ``mode='map'``: they come out as 0 (the cotangent of :func:`excite_cross`, which leaves them out).

    What it costs.  ``out is state`` in ``'gate'`` mode is ONE sparse launch: a read and a write of the vectors that hold a
    pair, nothing else.  Any other ``out`` (``None``: a new tensor) is filled first -- ``copy_`` of the state for ``'gate'``,
    a full read and write; ``zero_()`` for ``'map'``, a full write -- and the sparse launch follows: out of place the gate
    is no cheaper than one full pass.  ``out is state`` in ``'map'`` mode goes through a zeroed temporary and a copy back."""
    what = 'apply_excite_axpby'
    if mode not in ('gate', 'map'):
        raise ValueError(f"{what}: mode must be 'gate' or 'map', got {mode!r}")
    n, xmask, amask, zmask, negate, controls = _excite_args(state, spec, what)
    a, c = _pauli_coef(a, state, what), _pauli_coef(c, state, what)
    if out is None:
        out = torch.empty_like(state)
    else:
        out = _check_out(state, out, what)
    if out.data_ptr() == state.data_ptr():
        if mode == 'map':
            return out.copy_(apply_excite_axpby(state, spec, a, c, 'map'))
    elif mode == 'gate':
        out.copy_(state)
    else:
        out.zero_()
    if not _use_hip(state):
        def double():
            i0, i1, sigma = _excite_pairs(n, xmask, amask, zmask, negate, controls)
            x0, x1 = state[:, i0].to(torch.complex128), state[:, i1].to(torch.complex128)
            out[:, i0] = (a.reshape(-1, 1) * x0 - c.reshape(-1, 1) * sigma * x1).to(state.dtype)
            out[:, i1] = (a.reshape(-1, 1) * x1 + c.reshape(-1, 1) * sigma * x0).to(state.dtype)
            return out

        return _diag_double(double)
    return _excite_launch(state, out, _axpby_coef(a, c), _lib.EXCITE_GATE if mode == 'gate' else _lib.EXCITE_MAP,
                          (xmask, amask, zmask, negate), n, controls)


def _excite_launch(state, out, coef, code, masks, n, controls):
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_excite_axpby', state, _ptr(state, lo), _ptr(out, lo), _ptr(coef, lo), code, *masks, n,
              _lib.int_array(controls), len(controls), hi - lo)
    return out


def apply_excite_rot(state: torch.Tensor, spec, theta: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """exp(theta K) state = (I + sin(theta) K + (1 - cos(theta)) K^2) state: :func:`apply_excite_axpby` in 'gate' mode with
    a = cos(theta), c = sin(theta), formed in double from the real ``theta`` (B,), per sample.  ``out=state`` is the
    sparse in-place gate; see :func:`apply_excite_axpby` for what any other ``out`` costs."""
    theta = _real_angles(theta, state, 'apply_excite_rot')
    return apply_excite_axpby(state, spec, torch.cos(theta), torch.sin(theta), 'gate', out)


def excite_cross(bra: torch.Tensor, ket: torch.Tensor, spec) -> torch.Tensor:
    """out[b] = sum_i conj(bra[b, i]) (K ket[b])[i]: complex128 (B,), accumulated in double, bitwise reproducible, reading
    only the pairs (``dq_excite_cross_*``).  ``bra`` and ``ket`` the same buffer: each pair is read once, and the real part
    is 0 up to rounding (K is anti-Hermitian).  The workspace comes from PyTorch's allocator (legal under capture)."""
    n, xmask, amask, zmask, negate, controls = _excite_args(ket, spec, 'excite_cross')
    _check_bra(bra, ket, 'excite_cross')
    if not _use_hip(ket):
        def double():
            i0, i1, sigma = _excite_pairs(n, xmask, amask, zmask, negate, controls)
            u, v = bra.to(torch.complex128).conj(), ket.to(torch.complex128)
            return (sigma * (u[:, i1] * v[:, i0] - u[:, i0] * v[:, i1])).sum(dim=-1)

        return _diag_double(double)
    mid = (xmask, amask, zmask, negate, n, _lib.int_array(controls), len(controls))
    return _cross_reduce('dq_excite_cross', 'dq_excite_cross_ws_bytes', bra, ket, mid)


# ---------------------------------------------------------------------------------------------------
# Sums of Pauli strings (csrc/dq_psum.hip): H = sum_t h_t P_t, grouped by flip mask, the whole sum in one launch
class PsumTable:
    """The table of ``dq_apply_psum_axpby_*`` / ``dq_psum_cross_*`` for a register of ``nqubit`` wires, from host lists:
    ``xmasks`` (G,), ``bounds`` (2G + 1,), ``zmasks`` (T,) and ``weights`` (T,) as include/dq_hip.h section 13 describes
    them.  Checked here, once -- the kernels cannot -- kept as CPU tensors, and handed out per device by :meth:`on`
    (cached; the first use on a device copies four small tensors, which a graph capture does not allow: run once before
    capturing).  Pickles without the device copies."""

    def __init__(self, nqubit: int, xmasks: Sequence[int], bounds: Sequence[int], zmasks: Sequence[int], weights: Sequence[float]):
        n, g, t = int(nqubit), len(xmasks), len(zmasks)
        if n < 1 or n > 40:
            raise ValueError(f'PsumTable: nqubit={nqubit} out of range [1, 40]')
        if g < 1 or t < 1 or len(bounds) != 2 * g + 1 or len(weights) != t:
            raise ValueError(f'PsumTable: {g} groups, {len(bounds)} bounds, {t} masks and {len(weights)} weights do not fit '
                             'together (at least one group and one term; 2G + 1 bounds)')
        if any(int(m) < 0 or int(m) >> n for m in (*xmasks, *zmasks)):
            raise ValueError(f'PsumTable: every mask must lie in [0, 2**{n})')
        bounds = [int(b) for b in bounds]
        if bounds[0] != 0 or bounds[-1] != t or any(lo > hi for lo, hi in zip(bounds, bounds[1:])):
            raise ValueError(f'PsumTable: bounds must rise from 0 to the number of terms ({t}), got {bounds}')
        self.nqubit, self.ngroups, self.nterms = n, g, t
        # what the evolution needs of H (:func:`apply_psum_evolve`): the coefficient b of the empty string, and the sum of
        # |h_t| over every other string -- each has norm 1, so the triangle inequality bounds ||H - b|| by it, rigorously
        # (the sum rounded up, not to the nearest)
        is_empty = [int(x) == 0 and int(zmasks[j]) == 0 for x, lo, hi in zip(xmasks, bounds[0::2], bounds[2::2]) for j in range(lo, hi)]
        self.constant = math.fsum(float(w) for w, e in zip(weights, is_empty) if e)
        rest = math.fsum(abs(float(w)) for w, e in zip(weights, is_empty) if not e)
        self.norm_bound = math.nextafter(rest, math.inf) if rest > 0.0 else 0.0
        self._host = (torch.tensor([int(m) for m in xmasks], dtype=torch.int64), torch.tensor(bounds, dtype=torch.int32),
                      torch.tensor([int(m) for m in zmasks], dtype=torch.int64), torch.tensor(weights, dtype=torch.float64))
        self._devices: dict = {}

    def on(self, device) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(xmasks, bounds, zmasks, weights) on ``device``."""
        device = torch.device(device)
        if device.type == 'cpu':
            return self._host
        hit = self._devices.get(device)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('deepquantum_amd: the first use of a Pauli sum on a device copies its table there; run '
                                   'the step once before capturing it (dq.CapturedGraph warms up by itself)')
            hit = self._devices[device] = tuple(own(t.to(device)) for t in self._host)
        pin_if_capturing(*hit)
        return hit

    def tail(self, device) -> tuple:
        """What every entry point that takes the table takes of it, in order: its four pointers on ``device``, G, T and n."""
        return (*(_ptr(t) for t in self.on(device)), self.ngroups, self.nterms, self.nqubit)

    def __getstate__(self):
        return {**self.__dict__, '_devices': {}}


def _capturing(t: torch.Tensor) -> bool:
    """Is the current stream capturing?  (Under the CPU test double there may be no device to ask: then it is not.)"""
    if t.is_cuda:
        return torch.cuda.is_current_stream_capturing()
    try:
        return bool(torch.cuda.is_current_stream_capturing())
    except RuntimeError:
        return False


def _psum_args(state: torch.Tensor, table: PsumTable, what: str) -> int:
    n = _nqubit(state)
    if not isinstance(table, PsumTable):
        raise ValueError(f'{what}: the table must be a backend.PsumTable, got {type(table).__name__}')
    if not state.is_contiguous():
        raise ValueError(f'{what}: state must be contiguous')
    if table.nqubit != n:
        raise ValueError(f'{what}: the table is for {table.nqubit} qubits, the state has {n}')
    return n


def _psum_apply_double(x: torch.Tensor, table: PsumTable) -> torch.Tensor:
    """H x in complex128, group by group (CPU test double only)."""
    xmasks, bounds, zmasks, weights = (t.tolist() for t in table.on('cpu'))
    j = torch.arange(x.shape[-1])
    y = torch.zeros_like(x)
    for g, xmask in enumerate(xmasks):
        w = torch.zeros(x.shape[-1], dtype=torch.complex128)
        for t in range(bounds[2 * g], bounds[2 * g + 2]):
            par = j & zmasks[t]
            for sh in (32, 16, 8, 4, 2, 1):
                par = par ^ (par >> sh)
            w += (weights[t] if t < bounds[2 * g + 1] else 1j * weights[t]) * (1 - 2 * (par & 1)).to(torch.complex128)
        y += (w * x)[:, j ^ xmask]
    return y


def apply_psum_axpby(state: torch.Tensor, table: PsumTable, a, c, mode: str = 'gate', out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b] = a[b] state[b] + c[b] H state[b] for the sum of Pauli strings H of ``table``, in one launch: G + 1 reads and
    one write of the state for G groups, whatever the number of strings (``dq_apply_psum_axpby_*``).  ``a``, ``c``:
    complex, one value or one per sample.  The support of H is the whole state, so ``mode`` -- 'gate' or 'map', as the
    generator nodes of ``ops`` pass it -- changes nothing.  Out of place only: ``out`` must not overlap ``state``."""
    what = 'apply_psum_axpby'
    if mode not in ('gate', 'map'):
        raise ValueError(f"{what}: mode must be 'gate' or 'map', got {mode!r}")
    _psum_args(state, table, what)
    a, c = _pauli_coef(a, state, what), _pauli_coef(c, state, what)
    out = _check_out(state, out, what, in_place=False)
    if not _use_hip(state):
        def double():
            x = state.to(torch.complex128)
            return out.copy_((a.reshape(-1, 1) * x + c.reshape(-1, 1) * _psum_apply_double(x, table)).to(state.dtype))

        return _diag_double(double)
    coef = _axpby_coef(a, c)
    tail = table.tail(state.device)
    for lo, hi in _slices(state.shape[0]):
        _call('dq_apply_psum_axpby', state, _ptr(state, lo), _ptr(out, lo), _ptr(coef, lo), *tail, hi - lo)
    return out


def psum_cross(bra: torch.Tensor, ket: torch.Tensor, table: PsumTable) -> torch.Tensor:
    """out[b] = sum_i conj(bra[b, i]) (H ket[b])[i] for the sum of Pauli strings H of ``table``, in one launch: complex128
    (B,), bitwise reproducible (``dq_psum_cross_*``).  ``bra`` and ``ket`` the same buffer: G reads of the state for G
    groups (one of them without a flip over 16-byte vectors), else G + 1.  The workspace comes from PyTorch's allocator
    (legal under capture)."""
    _psum_args(ket, table, 'psum_cross')
    _check_bra(bra, ket, 'psum_cross')
    if not _use_hip(ket):
        return _diag_double(lambda: (bra.to(torch.complex128).conj() * _psum_apply_double(ket.to(torch.complex128), table)).sum(dim=-1))
    return _cross_reduce('dq_psum_cross', 'dq_psum_cross_ws_bytes', bra, ket, table.tail(ket.device))


# ---- exp(-i t H) for a Pauli sum: a Chebyshev expansion, one launch per order --------------------------------------------
# With b the coefficient of the empty string, a >= ||H - b|| (`PsumTable.norm_bound`: the sum of |h_t| over the other
# strings -- every Pauli string has norm 1, so the triangle inequality makes it rigorous) and H' = (H - b) / a, whose
# spectrum lies in [-1, 1],
#     exp(-i t H) psi = e^{-i t b} [ J_0(z) phi_0 + 2 sum_{k >= 1} (-i)^k J_k(z) phi_k ],        z = a t,
#     phi_0 = psi,  phi_1 = H' psi,  phi_{k+1} = 2 H' phi_k - phi_{k-1}
# and |phi_k| <= |psi|, so the sum cut after order K is off by at most 2 sum_{k > K} |J_k(z)| |psi|: K is the smallest order
# whose tail is below the caller's tolerance.
def bessel_j(z: float, kmax: int | None = None) -> list[float]:
    """``J_0(z) .. J_kmax(z)`` for ``z >= 0`` in float64 (``kmax=None``: up to the order the expansion can need, about
    ``z + 10 z^(1/3) + 80``, beyond which every value is below 1e-40): Miller's backward recurrence
    ``J_{k-1} = (2k / z) J_k - J_{k+1}`` from an even order 30 above the last one wanted, rescaled where it grows past
    1e250, normalised by ``J_0 + 2 sum_k J_2k = 1``.  What it returns depends on ``z`` alone: ``kmax`` only cuts or pads."""
    z = float(z)
    if not (z >= 0.0 and math.isfinite(z)):
        raise ValueError(f'bessel_j: z must be finite and >= 0, got {z}')
    top = int(math.ceil(z + 10.0 * z ** (1.0 / 3.0))) + 80
    if z == 0.0:
        vals = [1.0] + [0.0] * top
    else:
        start = top + 30 + (top & 1)                    # (even)
        vals = [0.0] * (start + 1)
        hi, cur = 0.0, 1e-250                           # J_{k+1}, J_k up to the common factor
        vals[start] = cur
        for k in range(start, 0, -1):
            hi, cur = cur, (2.0 * k / z) * cur - hi
            vals[k - 1] = cur
            if abs(cur) > 1e250:                        # (what was set far above underflows to 0: it is that small)
                hi, cur = hi * 1e-250, cur * 1e-250
                for m in range(k - 1, start + 1):
                    vals[m] *= 1e-250
        norm = vals[0] + 2.0 * math.fsum(vals[2::2])
        vals = [v / norm for v in vals[:top + 1]]
    if kmax is None:
        return vals
    return vals[:kmax + 1] + [0.0] * max(0, kmax - top)


def _cheb_order(vals: list[float], tol: float) -> int:
    """The smallest K with ``2 sum_{k > K} |J_k| < tol`` for the values of :func:`bessel_j` (which end where the rest is 0)."""
    tail, k = 0.0, len(vals) - 1
    while k > 0 and 2.0 * (tail + abs(vals[k])) < tol:
        tail += abs(vals[k])
        k -= 1
    return k


def chebyshev_order(z: float, tol: float) -> int:
    """The order K at which the expansion of ``exp(-i z H')``, ``||H'|| <= 1``, is cut: the smallest with
    ``2 sum_{k > K} |J_k(|z|)| < tol``; about ``|z|`` plus a few dozen."""
    tol = float(tol)
    if not (tol > 0.0 and math.isfinite(tol)):
        raise ValueError(f'chebyshev_order: tol must be a positive number, got {tol}')
    return _cheb_order(bessel_j(abs(float(z))), tol)


def _evolve_window(table: PsumTable, bounds, what: str) -> tuple[float, float]:
    """(a, b) with the spectrum of H inside [b - a, b + a]: the rigorous ``(norm_bound, constant)`` of the table, or half the
    width and the centre of the caller's ``bounds = (lo, hi)``."""
    if bounds is None:
        return table.norm_bound, table.constant
    try:
        lo, hi = (float(v) for v in bounds)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: bounds must be (lo, hi), two real numbers, got {bounds!r}') from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f'{what}: bounds must be finite, got ({lo}, {hi})')
    if lo >= hi:
        raise ValueError(f'{what}: bounds must have lo < hi, got ({lo}, {hi})')
    return (hi - lo) / 2.0, (hi + lo) / 2.0


def _evolve_plan(table: PsumTable, ts: list[float], tol: float, window: tuple[float, float] | None = None):
    """Per sample: the phase e^{-i t b} c_k of every order, c_0 = J_0, c_k = 2 (-i sgn t)^k J_k(a |t|) up to the sample's OWN
    order K_b and exactly 0 above it -- a sample's result does not depend on who shares its batch -- and K = max K_b."""
    a, b = (table.norm_bound, table.constant) if window is None else window
    rows, memo = [], {}
    for t in ts:
        if t not in memo:
            vals = bessel_j(a * abs(t))
            kb = _cheb_order(vals, tol)
            phase = complex(math.cos(t * b), -math.sin(t * b))
            step = -1j if t >= 0 else 1j
            memo[t] = [phase * ((1.0 if k == 0 else 2.0) * vals[k]) * step ** k for k in range(kb + 1)]
        rows.append(memo[t])
    order = max(len(r) for r in rows) - 1
    return [r + [0j] * (order + 1 - len(r)) for r in rows], order


def apply_psum_evolve(state: torch.Tensor, table: PsumTable, t, tol: float, out: torch.Tensor | None = None,
                      bounds: tuple[float, float] | None = None) -> torch.Tensor:
    """out[b] = exp(-i t[b] H) state[b] for the sum of Pauli strings H of ``table``, to within ``tol`` |state[b]| in the
    2-norm plus rounding: the Chebyshev expansion above, cut at ``chebyshev_order(norm_bound * max |t|, tol)``.  ``t``: real,
    one value or one per sample; it is READ ON THE HOST (one device-to-host copy per call when it lives on a device),
    because the number of launches depends on it -- so the call is refused under stream capture.  The coefficients of all
    orders go to the device as one float64 tensor in one copy.

    Launches: ``dq_apply_psum_axpby_*`` for phi_1, two elementwise operations to start the sum, then exactly one
    ``dq_pauli_sum_cheb_step_*`` per order from 2 to K, each writing phi_{k+1} over phi_{k-1}.  Two state-sized work
    buffers besides ``state`` (never written) and ``out`` (which must not overlap it).  A sample with ``t = 0`` comes back bit
    for bit, and every sample comes out as it would alone.

    ``bounds=(lo, hi)``: an interval that holds the spectrum of H, used in place of the rigorous ``constant -+ norm_bound`` --
    half its width where ``norm_bound`` stands above and its centre in the phase -- so that the order follows the true width
    (``PauliSum.spectral_bounds``).  The CALLER answers for it: outside the interval the expansion grows instead of
    converging.  ``None``: today's path, the same launches and the same bits."""
    what = 'apply_psum_evolve'
    n = _psum_args(state, table, what)
    _suffix(state)
    tol = float(tol)
    if not (tol > 0.0 and math.isfinite(tol)):
        raise ValueError(f'{what}: tol must be a positive number, got {tol}')
    if _capturing(state):
        raise RuntimeError(f'deepquantum_amd: {what} under stream capture: the number of launches depends on t, which is read '
                           'on the host; capture the steps around it')
    if not isinstance(t, torch.Tensor):                 # (a Python float is a double: not through the default float32)
        t = torch.tensor(t, dtype=torch.complex128 if isinstance(t, complex) else torch.float64)
    if t.is_complex():
        raise ValueError(f'{what}: t must be real, got {t.dtype}')
    ts = [float(v) for v in t.detach().reshape(-1).tolist()]
    batch = state.shape[0]
    if len(ts) == 1 and batch != 1:
        ts = ts * batch
    if len(ts) != batch:
        raise ValueError(f'{what}: one t, or one per sample ({batch}), expected; got {len(ts)}')
    if not all(math.isfinite(v) for v in ts):
        raise ValueError(f'{what}: t is not finite')
    out = _check_out(state, out, what, in_place=False)
    window = None if bounds is None else _evolve_window(table, bounds, what)
    coefs, order = _evolve_plan(table, ts, tol, window)
    a, b = (table.norm_bound, table.constant) if window is None else window
    hip = _use_hip(state)
    if order == 0:                                      # (a t below the tolerance, or H a constant: a phase)
        c0 = torch.tensor([r[0] for r in coefs], dtype=torch.complex128).to(device=state.device, dtype=state.dtype)
        torch.mul(state, c0.reshape(-1, 1), out=out)
    elif not hip:
        def double():
            x = state.to(torch.complex128)
            c = torch.tensor(coefs, dtype=torch.complex128)             # (B, K + 1)
            prev, cur = x, (_psum_apply_double(x, table) - b * x) / a
            acc = c[:, 0:1] * prev + c[:, 1:2] * cur
            for k in range(2, order + 1):
                prev, cur = cur, (2.0 / a) * _psum_apply_double(cur, table) - (2.0 * b / a) * cur - prev
                acc = acc + c[:, k:k + 1] * cur
            return out.copy_(acc.to(state.dtype))

        _diag_double(double)
    else:
        # ONE host tensor, one copy: [B][4] for phi_1 = -b/a psi + 1/a H psi, [B][2] c_0, [B][2] c_1, then [K - 1][B][5]
        # rows (alpha, beta, gamma, Re c_k, Im c_k) = (2/a, -2b/a, -1, c_k) for the orders 2 .. K
        flat = [v for _ in range(batch) for v in (-b / a, 0.0, 1.0 / a, 0.0)]
        for k in (0, 1):
            flat += [v for r in coefs for v in (r[k].real, r[k].imag)]
        for k in range(2, order + 1):
            flat += [v for r in coefs for v in (2.0 / a, -2.0 * b / a, -1.0, r[k].real, r[k].imag)]
        dev = torch.tensor(flat, dtype=torch.float64).to(state.device)
        first = dev[:4 * batch].reshape(batch, 4)
        c01 = torch.view_as_complex(dev[4 * batch:8 * batch].reshape(2, batch, 2)).to(state.dtype)
        steps = dev[8 * batch:].reshape(order - 1, batch, 5)
        tail = table.tail(state.device)
        cur = torch.empty_like(state)
        for lo, hi in _slices(batch):
            _call('dq_apply_psum_axpby', state, _ptr(state, lo), _ptr(cur, lo), _ptr(first, lo), *tail, hi - lo)
        torch.mul(state, c01[0].reshape(-1, 1), out=out)
        out.addcmul_(cur, c01[1].reshape(-1, 1))
        prev, nxt = state, (torch.empty_like(state) if order >= 2 else None)    # (order 2 must leave the input alone)
        for k in range(2, order + 1):
            for lo, hi in _slices(batch):
                _call('dq_pauli_sum_cheb_step', state, _ptr(cur, lo), _ptr(prev, lo), _ptr(nxt, lo), _ptr(out, lo),
                      _ptr(steps[k - 2], lo), *tail, hi - lo)
            prev, cur = cur, nxt
            nxt = prev                                  # (from the third order on, phi_{k+1} goes over phi_{k-1})
    for s, v in enumerate(ts):
        if v == 0.0:
            out[s].copy_(state[s])
    return out


# ---- one extremal eigenpair of a Pauli sum: three-term Lanczos, two launches a step ----------------------------------------
# With v_j the unit Lanczos vectors, step j is
#     u = H v_j - beta_j v_{j-1}  (over v_{j-1}),    alpha_j = Re <v_j, u>                      dq_pauli_sum_lanczos_step_*
#     w = u - alpha_j v_j  (in place),               beta_{j+1} = |w|,  Re <v_j, w> (the monitor)         dq_lanczos_update_*
# and nothing is normalised in a pass of its own: the buffer of v_j holds x_j = s_j v_j with ONE known factor -- s_1 = |start|,
# s_j = beta_j after that, since x_{j+1} is the w of step j as it stands -- and the host folds 1 / s_j into the coefficients of
# the next launch: (1 / s_j, 0, -beta_j / s_{j-1}) for the first kernel, -alpha_j / s_j for the second.  The tridiagonal T_m of
# the alpha and beta lives on the host in float64; its wanted eigenpair (theta, y) gives the residual |beta_{m+1} y_m|.
class LanczosResult(NamedTuple):
    """What :func:`psum_lanczos` returns, one entry per sample: ``value`` float64 (B,), ``vector`` (B, 2**n) in the start's
    dtype and on its device or ``None``, ``residual`` float64 (B,) -- the estimate |beta_{m+1} y_m| --, ``steps`` int64 (B,),
    ``converged`` bool (B,), and the records ``alphas`` / ``betas`` (lists of B lists: alpha_1 .. alpha_m, beta_2 ..
    beta_{m+1}).  The small tensors live on the host."""
    value: torch.Tensor
    vector: torch.Tensor | None
    residual: torch.Tensor
    steps: torch.Tensor
    converged: torch.Tensor
    alphas: list
    betas: list


class _LanczosHip:
    """The launches of one pass over a batch on the device: ``start`` (never written), two work buffers that take turns and,
    for the pass that forms the Ritz vector, the sum."""

    def __init__(self, table: PsumTable, start: torch.Tensor, n: int, acc: torch.Tensor | None):
        self.start, self.n, self.acc, self.batch = start, n, acc, start.shape[0]
        self.tail = table.tail(start.device)
        self.out = torch.empty(self.batch, 2, dtype=torch.float64, device=start.device)
        lib, c128 = _lib.load(), int(start.dtype == torch.complex128)
        self.ws = []
        for lo, hi in _slices(self.batch):
            nbytes = lib.dq_psum_cross_ws_bytes(n, hi - lo, c128, 0)
            self.ws.append((torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=start.device), nbytes))
        # x_1 = start is copied into the first work buffer by the update kernel itself (0 + 1 * start), which leaves
        # |start|^2 in the same fixed order as every other sum of the run: a sample's record does not depend on its batch
        self.cur, self.prev, self.spare = start, torch.zeros_like(start), None
        self.norm2 = [r[0] for r in self.update(self.prev, [[1.0, 0.0]] * self.batch, None, read=True)]

    def coef(self, rows):
        return rows if isinstance(rows, torch.Tensor) else torch.tensor(rows, dtype=torch.float64).to(self.start.device)

    def step(self, rows, read=True):
        """u over x_{j-1} (into a buffer of its own where x_{j-1} is the start); (Re <x_j, u>, |u|^2) per sample."""
        if self.prev is self.start:
            self.spare = nxt = torch.empty_like(self.start)
        else:
            nxt = self.prev
        coef = self.coef(rows)
        for (lo, hi), (ws, nbytes) in zip(_slices(self.batch), self.ws):
            _call('dq_pauli_sum_lanczos_step', self.start, _ptr(self.cur, lo), _ptr(self.prev, lo), _ptr(nxt, lo), _ptr(coef, lo),
                  *self.tail, hi - lo, _ptr(self.out, lo), _ptr(ws), nbytes)
        self.w = nxt
        return self.out.tolist() if read else None

    def update(self, w, rows, acc, read=True):
        coef = self.coef(rows)
        for (lo, hi), (ws, nbytes) in zip(_slices(self.batch), self.ws):
            _call('dq_lanczos_update', self.start, _ptr(self.cur, lo), _ptr(w, lo), _ptr(acc, lo) if acc is not None else _ptr(None),
                  _ptr(coef, lo), self.n, hi - lo, _ptr(self.out, lo), _ptr(ws), nbytes)
        return self.out.tolist() if read else None

    def finish(self, rows, read=True):
        """w = u + e x_j in place, the sum += d x_j; (|w|^2, Re <x_j, w>) per sample.  Then w is x_{j+1}."""
        got = self.update(self.w, rows, self.acc, read)
        self.cur, self.prev = self.w, self.cur
        return got

    def last(self, rows):
        """The sum += d x_m for the samples whose last vector this is (e = 0: the other buffer stays as it is -- a scratch
        one where the other buffer is the caller's start, which is never written)."""
        self.update(torch.zeros_like(self.start) if self.prev is self.start else self.prev, rows, self.acc, read=False)


class _LanczosDouble:
    """The same recurrence in complex128 on the host, sample by sample (CPU test double only): every sum is taken over one
    sample's own 1-D tensors, so that a sample's record does not depend on its batch."""

    def __init__(self, table: PsumTable, start: torch.Tensor, n: int, acc: torch.Tensor | None):
        self.table, self.acc, self.batch = table, acc, start.shape[0]
        self.cur = [start[b].to(torch.complex128) for b in range(self.batch)]
        self.prev = [torch.zeros_like(x) for x in self.cur]
        self.norm2 = [float((x.real * x.real + x.imag * x.imag).sum()) for x in self.cur]

    @staticmethod
    def sums(x, y):
        return float((x.real * y.real + x.imag * y.imag).sum()), float((y.real * y.real + y.imag * y.imag).sum())

    def step(self, rows, read=True):
        if isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        self.w, out = [], []
        for b, (alpha, beta, gamma) in enumerate(rows):
            hx = _psum_apply_double(self.cur[b].reshape(1, -1), self.table)[0] if alpha != 0.0 else torch.zeros_like(self.cur[b])
            u = alpha * hx + beta * self.cur[b] + gamma * self.prev[b]
            self.w.append(u)
            out.append(list(self.sums(self.cur[b], u)))
        return out

    def finish(self, rows, read=True):
        if isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        out = []
        for b, (e, d) in enumerate(rows):
            self.w[b] = self.w[b] + e * self.cur[b]
            if self.acc is not None:
                self.acc[b] += d * self.cur[b]
            out.append(list(self.sums(self.cur[b], self.w[b]))[::-1])
        self.cur, self.prev = self.w, self.cur
        return out

    def last(self, rows):
        if isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        for b, (_e, d) in enumerate(rows):
            self.acc[b] += d * self.cur[b]


def _ritz_pair(alphas: list[float], betas: list[float], highest: bool):
    """The wanted eigenpair of T_m (alpha_1 .. alpha_m on the diagonal, beta_2 .. beta_m beside it), y_1 >= 0."""
    m = len(alphas)
    t = torch.diag(torch.tensor(alphas, dtype=torch.float64))
    if m > 1:
        off = torch.tensor(betas[:m - 1], dtype=torch.float64)
        t = t + torch.diag(off, 1) + torch.diag(off, -1)
    vals, vecs = torch.linalg.eigh(t)
    k = m - 1 if highest else 0
    y = vecs[:, k]
    return float(vals[k]), (-y if float(y[0]) < 0 else y).tolist()


def psum_lanczos(table: PsumTable, start: torch.Tensor, which: str = 'lowest', tol: float | None = None,
                 max_steps: int | None = None, vector: bool = True) -> LanczosResult:
    """ONE extremal eigenpair -- ``which='lowest'`` or ``'highest'`` -- of the sum of Pauli strings H of ``table``, per sample
    of ``start`` (B, 2**n), complex64 or complex128, which is never written and need not be normalised: plain three-term
    Lanczos, two launches a step (``dq_pauli_sum_lanczos_step_*``: G + 1 reads of the state for G groups and one write;
    ``dq_lanczos_update_*``: two reads and a write), each leaving its two sums in the same launch, bitwise reproducible.

    A sample stops at the first m with ``|beta_{m+1} y_m| <= tol * norm_bound`` (``tol``: 1e-6 for complex64, 1e-12 for
    complex128 by default), on breakdown (``beta_{m+1} <= eps * norm_bound``: the Krylov space is exhausted, the pair exact) or
    at ``max_steps`` (default ``min(1000, 4 * 2**n)``; then ``converged`` is False and the best pair so far comes back).  Every
    sample stops at its OWN step, with coefficients that are exactly 0 after it, and comes out bit for bit as it would alone.
    ``vector=True`` runs the recurrence a second time -- the same launches, the same bits -- and sums the unit Ritz vector
    ``sum_j (y_j / s_j) x_j`` on the way: twice the launches, three state-sized work buffers besides ``start`` whatever m is.

    The host reads one (B, 2) tensor of doubles per launch, so the call is refused under stream capture.

    What this is not.  Not several eigenpairs, and no re-orthogonalisation: ghost copies of converged Ritz values appear in
    T_m and do not disturb the extreme pair.  In a degenerate extremal eigenspace the value is right and the vector returned
    depends on the start.  complex64 vectors stall near a residual of 1e-7 * norm_bound: a ``tol`` below that only runs to
    ``max_steps``."""
    what = 'psum_lanczos'
    n = _psum_args(start, table, what)
    _suffix(start)
    if which not in ('lowest', 'highest'):
        raise ValueError(f"{what}: which must be 'lowest' or 'highest', got {which!r}")
    if tol is None:
        tol = 1e-6 if start.dtype == torch.complex64 else 1e-12
    tol = float(tol)
    if not (tol > 0.0 and math.isfinite(tol)):
        raise ValueError(f'{what}: tol must be a positive number, got {tol}')
    if max_steps is None:
        max_steps = min(1000, 4 << n)
    if int(max_steps) != max_steps or max_steps < 1:
        raise ValueError(f'{what}: max_steps must be a positive integer, got {max_steps!r}')
    max_steps = int(max_steps)
    if _capturing(start):
        raise RuntimeError(f'deepquantum_amd: {what} under stream capture: the host reads two sums after every launch and decides '
                           'when to stop; capture the steps around it')
    batch, highest = start.shape[0], which == 'highest'
    nb = table.norm_bound
    eps = float(torch.finfo(torch.float32 if start.dtype == torch.complex64 else torch.float64).eps)
    engine = _LanczosHip if _use_hip(start) else _LanczosDouble

    def run():
        first = engine(table, start, n, None)
        s1 = []
        for b, v in enumerate(first.norm2):
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError(f'{what}: the start vector of sample {b} is zero or not finite')
            s1.append(math.sqrt(v))
        if nb == 0.0:                                   # H is a constant: every vector is an eigenvector
            zeros = torch.zeros(batch, dtype=torch.float64)
            vec = None
            if vector:
                scale = torch.tensor([1.0 / s for s in s1], dtype=torch.float64).to(start.device).reshape(-1, 1)
                vec = (start * scale).to(start.dtype)
            return LanczosResult(torch.full((batch,), table.constant, dtype=torch.float64), vec, zeros, zeros.long(),
                                 torch.ones(batch, dtype=torch.bool), [[] for _ in range(batch)], [[] for _ in range(batch)])
        alphas, betas = [[] for _ in range(batch)], [[] for _ in range(batch)]
        scales = [[s] for s in s1]                      # s_1 .. s_m of each sample
        done: list = [None] * batch                     # (theta, y, residual, converged) once a sample has stopped
        recs = []                                       # the coefficient rows of every launch, for the second pass
        j = 0
        while any(d is None for d in done):
            j += 1
            rows = [[0.0, 0.0, 0.0] if done[b] is not None else
                    [1.0 / scales[b][-1], 0.0, -betas[b][-1] / scales[b][-2] if j > 1 else 0.0] for b in range(batch)]
            got = first.step(rows)
            for b in range(batch):
                if done[b] is None:
                    alphas[b].append(got[b][0] / scales[b][-1])
            erows = [[0.0, 0.0] if done[b] is not None else [-alphas[b][-1] / scales[b][-1], 0.0] for b in range(batch)]
            got = first.finish(erows)
            recs.append((rows, erows))
            for b in range(batch):
                if done[b] is not None:
                    continue
                beta = math.sqrt(max(got[b][0], 0.0))
                betas[b].append(beta)
                theta, y = _ritz_pair(alphas[b], betas[b], highest)
                res = abs(beta * y[-1])
                if not math.isfinite(res):
                    raise RuntimeError(f'{what}: the recurrence of sample {b} left the finite numbers at step {j}')
                if res <= tol * nb or beta <= eps * nb or j >= max_steps:
                    done[b] = (theta, y, res, res <= tol * nb or beta <= eps * nb)
                else:
                    scales[b].append(beta)
        steps = [len(a) for a in alphas]
        vec = None
        if vector:
            vec = torch.zeros_like(start) if engine is _LanczosHip else [torch.zeros(start.shape[-1], dtype=torch.complex128)
                                                                         for _ in range(batch)]
            again, top = engine(table, start, n, vec), max(steps)
            weight = lambda b, k: float(done[b][1][k - 1]) / scales[b][k - 1] if k <= steps[b] else 0.0  # noqa: E731
            # ONE host tensor, one copy: [top - 1][B][3] rows of the first kernel, then [top][B][2] rows of the second
            flat = [v for k in range(1, top) for b in range(batch) for v in (recs[k - 1][0][b] if k < steps[b] else [0.0, 0.0, 0.0])]
            flat += [v for k in range(1, top + 1) for b in range(batch)
                     for v in (recs[k - 1][1][b][0] if k < steps[b] else 0.0, weight(b, k))]
            dev = torch.tensor(flat, dtype=torch.float64).to(start.device)
            arows = dev[:3 * batch * (top - 1)].reshape(top - 1, batch, 3)
            erows = dev[3 * batch * (top - 1):].reshape(top, batch, 2)
            for k in range(1, top):
                again.step(arows[k - 1], read=False)
                again.finish(erows[k - 1], read=False)
            again.last(erows[top - 1])
            if engine is _LanczosDouble:
                vec = torch.stack(vec).to(start.dtype)
        return LanczosResult(torch.tensor([d[0] for d in done], dtype=torch.float64), vec,
                             torch.tensor([d[2] for d in done], dtype=torch.float64), torch.tensor(steps, dtype=torch.int64),
                             torch.tensor([bool(d[3]) for d in done], dtype=torch.bool), alphas, betas)

    return run() if engine is _LanczosHip else _diag_double(run)


# ---- every sample against every sample (csrc/dq_gram.hip) ----------------------------------------------------------------
#: rows of either operand per launch of `gram` (the workspace holds 32 x 32 partial sums per workgroup: 64 MiB at this size)
#: and of the output of `combine`; the wrappers slice wider batches
GRAM_MAX_ROWS = 2048


class GramGeometry(NamedTuple):
    """``dq_gram_geometry``: the rows of a tile; the real terms a float32 accumulator chains before it is added into a double
    (0 for complex128: float64 throughout); the columns of a lane's segment, of a wave's share of a step and of a
    workgroup's unit per iteration; the most workgroups a tile pair is spread over."""

    tile_rows: int
    chain: int
    lane_cols: int
    wave_cols: int
    unit_cols: int
    max_blocks: int


def gram_geometry(dtype: torch.dtype) -> GramGeometry:
    vals = [C.c_int() for _ in range(6)]
    _lib.check(_lib.load().dq_gram_geometry(int(dtype == torch.complex128), *[C.byref(v) for v in vals]), 'dq_gram_geometry')
    return GramGeometry(*[v.value for v in vals])


def _gram_rows(t: torch.Tensor, name: str, what: str) -> int:
    n = _nqubit(t)
    _suffix(t)
    if t.is_conj() or t.is_neg():                       # (what `_ptr` refuses, on the stand-in's route as well)
        raise ValueError(f'{what}: {name} is a tensor with a pending conjugation / negation: resolve_conj() / resolve_neg() it first')
    if not t.is_contiguous():
        raise ValueError(f'{what}: {name} must be contiguous')
    if t.shape[0] < 1:
        raise ValueError(f'{what}: {name} has no rows')
    if n == 0 and t.dtype == torch.complex64:
        raise ValueError(f'{what}: a complex64 row needs at least two amplitudes (one 16-byte vector)')
    return n


def gram(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """G[i, j] = sum_x conj(bra[i, x]) ket[j, x] for (M, 2^n) and (N, 2^n) states of one dtype: complex128 (M, N), on the
    matrix cores (``dq_gram_*``).  Up to 32 x 32 rows every row is read once; beyond that rows are tiled and a row of
    ``bra`` is read ceil(N / 32) times, a row of ``ket`` ceil(M / 32) times.  ``bra`` and ``ket`` the same buffer is the
    self-Gram: half the tiles, exactly Hermitian, a real diagonal.  complex64 sums at most ``gram_geometry().chain`` real
    terms in float32 before it continues in double.  Bitwise reproducible; an entry's bits depend on its two rows, n and the
    number of tile pairs of the launch alone (one pair up to 32 x 32 rows: entry (i, j) of a 5 x 7 Gram is the 1 x 1 Gram
    of those rows, bit for bit).  Batches beyond ``GRAM_MAX_ROWS`` rows are sliced here, so the self-Gram of a wider batch
    is Hermitian within rounding only.  The workspace comes from PyTorch's allocator (legal under capture)."""
    what = 'gram'
    n = _gram_rows(ket, 'ket', what)
    if bra is not ket:
        if bra.ndim != 2 or bra.shape[1] != ket.shape[1] or bra.dtype != ket.dtype or bra.device != ket.device:
            raise ValueError(f'{what}: bra/ket must be (rows, 2**n) tensors of one n, dtype and device, got {tuple(bra.shape)} '
                             f'{bra.dtype} and {tuple(ket.shape)} {ket.dtype}')
        _gram_rows(bra, 'bra', what)
    if not _use_hip(ket):
        def double():
            g = bra.to(torch.complex128).conj() @ ket.to(torch.complex128).T
            if bra.data_ptr() == ket.data_ptr() and bra.shape == ket.shape:      # the self-Gram, as the kernel leaves it
                up = torch.triu(g, 1)
                g = up + up.mH + torch.diag(g.diagonal().real).to(torch.complex128)
            return g.resolve_conj()

        return _diag_double(double)
    M, N = bra.shape[0], ket.shape[0]
    out = torch.empty(M, N, 2, dtype=torch.float64, device=ket.device)
    whole = M <= GRAM_MAX_ROWS and N <= GRAM_MAX_ROWS
    c128 = int(ket.dtype == torch.complex128)
    for alo, ahi in _slices(M, GRAM_MAX_ROWS):
        for blo, bhi in _slices(N, GRAM_MAX_ROWS):
            nbytes = _lib.load().dq_gram_ws_bytes(n, ahi - alo, bhi - blo, c128)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=ket.device)
            part = out if whole else torch.empty(ahi - alo, bhi - blo, 2, dtype=torch.float64, device=ket.device)
            _call('dq_gram', ket, _ptr(bra, alo), _ptr(ket, blo), n, ahi - alo, bhi - blo, _ptr(part), _ptr(ws), nbytes)
            if not whole:
                out[alo:ahi, blo:bhi] = part
    return torch.view_as_complex(out)


def combine(states: torch.Tensor, coef: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[m, x] = sum_j coef[m, j] states[j, x] for (N, 2^n) states and a complex (M, N) ``coef``: (M, 2^n) in the states'
    dtype, on the matrix cores (``dq_combine_*``).  ``coef`` is rounded once to the states' precision, the chain of an
    output element is 2 N real terms in that precision.  Up to 32 output rows the states are read once and ``out`` written
    once; beyond that output rows are tiled and the states read ceil(M / 32) times.  Out of place only: ``out`` must not
    overlap ``states``."""
    what = 'combine'
    n = _gram_rows(states, 'states', what)
    N = states.shape[0]
    if not isinstance(coef, torch.Tensor) or coef.ndim != 2 or coef.shape[1] != N or coef.shape[0] < 1:
        raise ValueError(f'{what}: coef must have shape (M, {N}) for {N} states, got '
                         f'{tuple(coef.shape) if isinstance(coef, torch.Tensor) else type(coef).__name__}')
    coef = _finish_table(coef, states, torch.complex128, what)
    M = coef.shape[0]
    out = _check_out(states, out, what, in_place=False, shape=(M, states.shape[1]))
    if not _use_hip(states):
        return _diag_double(lambda: out.copy_((coef @ states.to(torch.complex128)).to(states.dtype)))
    for lo, hi in _slices(M, GRAM_MAX_ROWS):
        _call('dq_combine', states, _ptr(states), _ptr(coef, lo), _ptr(out, lo), n, hi - lo, N)
    return out
