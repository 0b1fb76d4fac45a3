"""Gate library, API-compatible with the reference's gate.py for the statevector path.

Matrices are built with exactly the arithmetic of the reference (file:line cited per class) because
parity to 1e-10 in complex128 requires bit-identical matrices: fixed gates are float32-rounded
complex64 buffers that ``.to(torch.double)`` merely widens (SURVEY summary item 3), parametric gates
evaluate cos/sin/exp in the precision of their parameter.  A parameter may carry a leading batch
dimension (one value per data sample): the matrix builders then return (B, D, D), which replaces the
``torch.vmap`` over the whole circuit that the reference uses for batched data (circuit.py:232-240).
"""

from __future__ import annotations

from copy import copy
from typing import Any

import torch
from torch import nn
from torch.autograd.functional import jacobian

from .executor import Prim
from .operation import Gate, tensor_version
from .qmath import multi_kron  # noqa: F401  (re-exported for API parity)


def _is_batched(t: torch.Tensor) -> bool:
    return t.ndim >= 1 and t.numel() > 1


def _prep(theta: torch.Tensor) -> torch.Tensor:
    """Parameter -> shape () (single) or (B,) (one value per sample)."""
    return theta.reshape(-1) if _is_batched(theta) else theta.reshape(())


def _mat(entries: list[torch.Tensor], d: int) -> torch.Tensor:
    """Row-major entries, each () or (B,), -> (d, d) or (B, d, d)."""
    m = torch.stack(entries, dim=-1)
    return m.reshape(*m.shape[:-1], d, d)


def _diag(entries: list[torch.Tensor]) -> torch.Tensor:
    return torch.stack(entries, dim=-1).diag_embed()


def _as_param_tensor(x: Any) -> torch.Tensor:
    if isinstance(x, (torch.Tensor, nn.Parameter)):
        return x
    return torch.tensor(x, dtype=torch.float)


# ======================================================================================================
# structural base classes
# ======================================================================================================
class SingleGate(Gate):
    """Single-qubit gate (reference: gate.py:20-85)."""

    def __init__(self, name=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False, tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)
        assert len(self.wires) == 1
        self.nancilla = 2


class DoubleGate(Gate):
    """Two-qubit gate (reference: gate.py:88-185)."""

    def __init__(self, name=None, nqubit=2, wires=None, controls=None, condition=False, den_mat=False, tsr_mode=False):
        if wires is None:
            wires = [0, 1]
        assert len(wires) == 2
        super().__init__(name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)


class DoubleControlGate(DoubleGate):
    """Two-qubit gate of the form |0><0| (x) I + |1><1| (x) U with wires[0] the control
    (reference: gate.py:188-226).  The kernels see it as U on wires[1] controlled by wires[0]."""

    def __init__(self, name=None, nqubit=2, wires=None, den_mat=False, tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, controls=None, condition=False,
                         den_mat=den_mat, tsr_mode=tsr_mode)

    def prims(self, decompose: bool = True) -> list[Prim]:
        full = self.update_matrix()
        d = self.__dict__
        c = d.get('_prims_cache')          # as in Gate.prims: same matrix object, version and wires -> same primitives
        ver = tensor_version(full)
        if c is not None and ver is not None and c[0] is full and c[3] == ver and c[1] == self.wires:
            return c[2]
        m = full[..., 2:4, 2:4]
        out = [Prim(self._sub_kind, m, self._bits([self.wires[1]]), self._bits([self.wires[0]]))]
        # (a matrix that carries an autograd graph is a new object every forward: keeping it would only keep that graph --
        # and the AccumulateGrad nodes of its parameters, with the stream they were made on -- alive until the next one)
        d['_prims_cache'] = None if full.requires_grad else (full, list(self.wires), out, ver)
        return out

    _sub_kind = 'gen'


class TripleGate(Gate):
    """Three-qubit gate (reference: gate.py:229-265)."""

    def __init__(self, name=None, nqubit=3, wires=None, controls=None, condition=False, den_mat=False, tsr_mode=False):
        if wires is None:
            wires = [0, 1, 2]
        assert len(wires) == 3
        super().__init__(name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)


class ArbitraryGate(Gate):
    """Gate on an arbitrary list of wires or a ``minmax`` range (reference: gate.py:268-338)."""

    def __init__(self, name=None, nqubit=1, wires=None, minmax=None, controls=None, condition=False,
                 den_mat=False, tsr_mode=False):
        self.nqubit = nqubit
        if wires is None:
            if minmax is None:
                minmax = [0, nqubit - 1]
            self._check_minmax(minmax)
            wires = list(range(minmax[0], minmax[1] + 1))
        super().__init__(name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)
        self.minmax = [min(self.wires), max(self.wires)]
        self.local = all(b - a == 1 for a, b in zip(self.wires[:-1], self.wires[1:]))
        self.inv_mode = False

    def inverse(self) -> 'ArbitraryGate':
        gate = copy(self)
        gate.inv_mode = not self.inv_mode
        if isinstance(self.name, str):
            gate.name = self.name[:-7] if self.name.endswith('_dagger') else self.name + '_dagger'
        return gate


class _Parametric:
    """Shared machinery of parametric gates: parameter storage, inverse, derivative."""

    _param_names = ('theta',)

    def _setup_params(self, inputs: Any, requires_grad: bool) -> None:
        self.npara = len(self._param_names)
        self.requires_grad = requires_grad
        self.inv_mode = False
        self.init_para(inputs)

    def inputs_to_tensor(self, inputs: Any = None) -> torch.Tensor:
        """Reference: gate.py:368-376 -- nested lists unwrap to their first element, ``None`` draws
        U(0, 4 pi), Python numbers become float32 tensors."""
        while isinstance(inputs, list):
            inputs = inputs[0]
        if inputs is None:
            # (= torch.rand(1)[0] * 4 * torch.pi to the last bit, same draw from the generator; two tiny ops instead of four)
            return torch.rand(()).mul_(4 * torch.pi)
        return _as_param_tensor(inputs)

    # ``matrix`` is evaluated lazily: the reference recomputes it inside every ``init_para`` /
    # ``update_matrix`` call (gate.py:395-415), i.e. a handful of tiny device kernels per gate per forward.
    # Here ``init_para`` only stores the parameter; the circuit driver evaluates all gates of one class in
    # a single vectorised call (``QubitCircuit._precompute_matrices``), and ``gate.matrix`` computes on
    # demand when somebody reads it.
    @property
    def matrix(self) -> torch.Tensor:
        m = self.__dict__.get('_matrix_cache')
        if m is None:
            self.update_matrix()
            m = self.__dict__['_matrix_cache']
        return m

    @matrix.setter
    def matrix(self, value: torch.Tensor) -> None:
        self.__dict__['_matrix_cache'] = value

    def _invalidate(self) -> None:
        self.__dict__['_matrix_cache'] = None
        self.__dict__['_precomputed'] = None
        self.__dict__['_matrix_key'] = None

    def _param_key(self) -> tuple:
        """Identity and version of every parameter tensor (+ the inverse flag): what the cached matrix belongs to."""
        return tuple((t, tensor_version(t)) for t in (getattr(self, n) for n in self._param_names)) + (self.inv_mode,)

    def _stamp(self) -> None:
        self.__dict__['_matrix_key'] = self._param_key()

    def _fixed_matrix(self) -> torch.Tensor | None:
        """The cached matrix, if it is still the matrix of the current parameters and no autograd graph has to be
        built: a gate with fixed angles is evaluated once, not once per forward."""
        m, key = self.__dict__.get('_matrix_cache'), self.__dict__.get('_matrix_key')
        if m is None or key is None or key[-1] != self.inv_mode:
            return None
        grad = torch.is_grad_enabled()
        for (t, version), name in zip(key[:-1], self._param_names):
            cur = getattr(self, name)
            if cur is not t or version is None or tensor_version(cur) != version or (grad and cur.requires_grad):
                return None
        return m

    def init_para(self, inputs: Any = None) -> None:
        theta = self.inputs_to_tensor(inputs)
        if self.requires_grad:
            self.theta = nn.Parameter(theta)
        else:
            self.register_buffer('theta', theta)
        self._invalidate()

    def update_matrix(self) -> torch.Tensor:
        pre = self.__dict__.get('_precomputed')
        if pre is not None:
            return pre
        fixed = self._fixed_matrix()
        if fixed is not None:
            return fixed
        theta = -self.theta if self.inv_mode else self.theta
        matrix = self.get_matrix(theta)
        self.matrix = matrix.detach()
        self._stamp()
        return matrix

    def _apply(self, fn: Any, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate()
        return out

    def get_derivative(self, theta: Any) -> torch.Tensor:
        """dU/dtheta by differentiating the matrix builder (reference: gate.py:402-406)."""
        theta = self.inputs_to_tensor(theta).squeeze()
        du = jacobian(self._real_wrapper, theta)
        return du[..., 0] + du[..., 1] * 1j

    def inverse(self):
        gate = copy(self)
        gate.inv_mode = not self.inv_mode
        gate._invalidate()
        return gate

    def extra_repr(self) -> str:
        theta = -self.theta if self.inv_mode else self.theta
        val = theta.item() if theta.numel() == 1 else f'<batch of {theta.numel()}>'
        s = f'wires={self.wires}, theta={val}'
        return s if self.controls == [] else s + f', controls={self.controls}'


class ParametricSingleGate(_Parametric, SingleGate):
    """Single-qubit gate with one parameter (reference: gate.py:341-429)."""

    def __init__(self, name=None, inputs=None, nqubit=1, wires=None, controls=None, condition=False,
                 den_mat=False, tsr_mode=False, requires_grad=False):
        SingleGate.__init__(self, name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                            den_mat=den_mat, tsr_mode=tsr_mode)
        self._setup_params(inputs, requires_grad)


class ParametricDoubleGate(_Parametric, DoubleGate):
    """Two-qubit gate with one parameter (reference: gate.py:432-520)."""

    def __init__(self, name=None, inputs=None, nqubit=2, wires=None, controls=None, condition=False,
                 den_mat=False, tsr_mode=False, requires_grad=False):
        DoubleGate.__init__(self, name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                            den_mat=den_mat, tsr_mode=tsr_mode)
        self._setup_params(inputs, requires_grad)


# ======================================================================================================
# fixed single-qubit gates
# ======================================================================================================
def _fixed_single(cls_name: str, gate_name: str, build, kind: str = 'gen', inverse_name: str | None = None,
                  nancilla: int | None = None, doc: str = '', mode: int = 0):
    def __init__(self, nqubit=1, wires=None, controls=None, condition=False, den_mat=False, tsr_mode=False):
        SingleGate.__init__(self, name=gate_name, nqubit=nqubit, wires=wires, controls=controls,
                            condition=condition, den_mat=den_mat, tsr_mode=tsr_mode)
        self.register_buffer('matrix', build())
        if nancilla is not None:
            self.nancilla = nancilla

    def inverse(self):
        if inverse_name is None:
            return self
        other = globals()[inverse_name]
        return other(nqubit=self.nqubit, wires=self.wires, controls=self.controls, condition=self.condition,
                     den_mat=self.den_mat, tsr_mode=self.tsr_mode).to(self.matrix.device, self.matrix.real.dtype)

    return type(cls_name, (SingleGate,), {'__init__': __init__, 'inverse': inverse, '_kernel_kind': kind,
                                          '_kernel_mode': mode, '__doc__': doc})


PauliX = _fixed_single('PauliX', 'PauliX', lambda: torch.tensor([[0, 1], [1, 0]], dtype=torch.cfloat), kind='x',
                       doc='Pauli-X (reference: gate.py:800-872, matrix :841).')
PauliY = _fixed_single('PauliY', 'PauliY', lambda: torch.tensor([[0, -1j], [1j, 0]]), nancilla=4,
                       doc='Pauli-Y (reference: gate.py:875-951, matrix :916).')
PauliZ = _fixed_single('PauliZ', 'PauliZ', lambda: torch.tensor([[1, 0], [0, -1]], dtype=torch.cfloat), kind='diag',
                       doc='Pauli-Z (reference: gate.py:954-1024, matrix :995).')
Hadamard = _fixed_single('Hadamard', 'Hadamard',
                         lambda: torch.tensor([[1, 1], [1, -1]], dtype=torch.cfloat) / 2**0.5, nancilla=1, mode=3,
                         doc='Hadamard; note the float32-rounded 1/sqrt(2) (reference: gate.py:1027-1099, :1069).')
SGate = _fixed_single('SGate', 'SGate', lambda: torch.tensor([[1, 0], [0, 1j]]), kind='diag',
                      inverse_name='SDaggerGate', doc='S (reference: gate.py:1102-1188, matrix :1143).')
SDaggerGate = _fixed_single('SDaggerGate', 'SDaggerGate', lambda: torch.tensor([[1, 0], [0, -1j]]), kind='diag',
                            inverse_name='SGate', doc='S^dagger (reference: gate.py:1191-1258, matrix :1233).')
TGate = _fixed_single('TGate', 'TGate', lambda: torch.tensor([[1, 0], [0, (1 + 1j) / 2**0.5]]), kind='diag',
                      inverse_name='TDaggerGate', doc='T (reference: gate.py:1261-1322, matrix :1303).')
TDaggerGate = _fixed_single('TDaggerGate', 'TDaggerGate', lambda: torch.tensor([[1, 0], [0, (1 - 1j) / 2**0.5]]),
                            kind='diag', inverse_name='TGate', doc='T^dagger (reference: gate.py:1325-1388, :1367).')


class Identity(Gate):
    """Identity on any number of wires (reference: gate.py:756-797)."""

    _kernel_kind = 'diag'

    def __init__(self, nqubit=1, wires=None, den_mat=False, tsr_mode=False):
        super().__init__(name='Identity', nqubit=nqubit, wires=wires, den_mat=den_mat, tsr_mode=tsr_mode)
        self.register_buffer('matrix', torch.eye(2**self.nqubit, dtype=torch.cfloat))

    def prims(self, decompose: bool = True) -> list[Prim]:
        return []

    def get_unitary(self) -> torch.Tensor:
        return self.matrix

    def forward(self, x: Any) -> Any:
        return x


# ======================================================================================================
# parametric single-qubit gates
# ======================================================================================================
class U3Gate(ParametricSingleGate):
    r"""U3(theta, phi, lambda) (reference: gate.py:523-674, matrix :594-602)."""

    _param_names = ('theta', 'phi', 'lambd')

    def __init__(self, inputs=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False, requires_grad=False):
        super().__init__(name='U3Gate', inputs=inputs, nqubit=nqubit, wires=wires, controls=controls,
                         condition=condition, den_mat=den_mat, tsr_mode=tsr_mode, requires_grad=requires_grad)
        self.npara = 3

    def inputs_to_tensor(self, inputs: Any = None):
        if inputs is None:
            theta = torch.rand(()).mul_(torch.pi)          # (the reference's torch.rand(1)[0] * .., bit for bit)
            phi = torch.rand(()).mul_(2 * torch.pi)
            lambd = torch.rand(()).mul_(2 * torch.pi)
        elif isinstance(inputs, torch.Tensor) and inputs.ndim == 2:  # (batch, 3): one triple per sample
            theta, phi, lambd = inputs.unbind(-1)
        else:
            theta, phi, lambd = inputs[0], inputs[1], inputs[2]
        return _as_param_tensor(theta), _as_param_tensor(phi), _as_param_tensor(lambd)

    def get_matrix(self, theta: Any, phi: Any, lambd: Any) -> torch.Tensor:
        theta, phi, lambd = self.inputs_to_tensor([theta, phi, lambd])
        theta, phi, lambd = _prep(theta), _prep(phi), _prep(lambd)
        cos_t = torch.cos(theta / 2) + 0j
        sin_t = torch.sin(theta / 2) + 0j
        e_il = torch.exp(1j * lambd)
        e_ip = torch.exp(1j * phi)
        e_ipl = torch.exp(1j * (phi + lambd))
        return _mat([cos_t, -e_il * sin_t, e_ip * sin_t, e_ipl * cos_t], 2)

    def update_matrix(self) -> torch.Tensor:
        pre = self.__dict__.get('_precomputed')
        if pre is not None:
            return pre
        fixed = self._fixed_matrix()
        if fixed is not None:
            return fixed
        if self.inv_mode:
            theta, phi, lambd = -self.theta, -self.lambd, -self.phi
        else:
            theta, phi, lambd = self.theta, self.phi, self.lambd
        matrix = self.get_matrix(theta, phi, lambd)
        self.matrix = matrix.detach()
        self._stamp()
        return matrix

    def _real_wrapper(self, x: torch.Tensor) -> torch.Tensor:
        return torch.view_as_real(self.get_matrix(x[0], x[1], x[2]))

    def get_derivative(self, inputs: Any) -> torch.Tensor:
        if not isinstance(inputs, torch.Tensor):
            inputs = torch.tensor(inputs, dtype=torch.float)
        du = jacobian(self._real_wrapper, inputs.reshape(self.npara)).permute(3, 0, 1, 2)
        return du[..., 0] + du[..., 1] * 1j

    def init_para(self, inputs: Any = None) -> None:
        theta, phi, lambd = self.inputs_to_tensor(inputs)
        for name, val in (('theta', theta), ('phi', phi), ('lambd', lambd)):
            if self.requires_grad:
                setattr(self, name, nn.Parameter(val))
            else:
                self.register_buffer(name, val)
        self._invalidate()

    def extra_repr(self) -> str:
        s = f'wires={self.wires}, npara=3'
        return s if self.controls == [] else s + f', controls={self.controls}'


class PhaseShift(ParametricSingleGate):
    r"""diag(1, e^{i theta}) (reference: gate.py:677-753, matrix :737-742)."""

    _kernel_kind = 'diag'

    def __init__(self, inputs=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False, requires_grad=False):
        super().__init__(name='PhaseShift', inputs=inputs, nqubit=nqubit, wires=wires, controls=controls,
                         condition=condition, den_mat=den_mat, tsr_mode=tsr_mode, requires_grad=requires_grad)

    def get_matrix(self, theta: Any) -> torch.Tensor:
        theta = _prep(self.inputs_to_tensor(theta))
        e_it = torch.exp(1j * theta)
        return _diag([torch.ones_like(e_it), e_it])


class Rx(ParametricSingleGate):
    r"""exp(-i theta X / 2) (reference: gate.py:1389-1480, matrix :1443-1448)."""

    _kernel_mode = 2  # cos + 0j on the diagonal, (0 -/+ i sin) off it: exact zeros by construction

    def __init__(self, inputs=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False, requires_grad=False):
        super().__init__(name='Rx', inputs=inputs, nqubit=nqubit, wires=wires, controls=controls,
                         condition=condition, den_mat=den_mat, tsr_mode=tsr_mode, requires_grad=requires_grad)

    def get_matrix(self, theta: Any) -> torch.Tensor:
        theta = _prep(self.inputs_to_tensor(theta))
        cos = torch.cos(theta / 2) + 0j
        isin = torch.sin(theta / 2) * 1j
        return _mat([cos, -isin, -isin, cos], 2)


class Ry(ParametricSingleGate):
    r"""exp(-i theta Y / 2) (reference: gate.py:1483-1579, matrix :1538-1543)."""

    _kernel_mode = 1  # real entries + 0j

    def __init__(self, inputs=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False, requires_grad=False):
        super().__init__(name='Ry', inputs=inputs, nqubit=nqubit, wires=wires, controls=controls,
                         condition=condition, den_mat=den_mat, tsr_mode=tsr_mode, requires_grad=requires_grad)

    def get_matrix(self, theta: Any) -> torch.Tensor:
        theta = _prep(self.inputs_to_tensor(theta))
        cos = torch.cos(theta / 2)
        sin = torch.sin(theta / 2)
        return _mat([cos, -sin, sin, cos], 2) + 0j


class Rz(ParametricSingleGate):
    r"""exp(-i theta Z / 2) (reference: gate.py:1582-1671, matrix :1634-1639)."""

    _kernel_kind = 'diag'

    def __init__(self, inputs=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False, requires_grad=False):
        super().__init__(name='Rz', inputs=inputs, nqubit=nqubit, wires=wires, controls=controls,
                         condition=condition, den_mat=den_mat, tsr_mode=tsr_mode, requires_grad=requires_grad)

    def get_matrix(self, theta: Any) -> torch.Tensor:
        theta = _prep(self.inputs_to_tensor(theta))
        return _diag([torch.exp(-1j * theta / 2), torch.exp(1j * theta / 2)])


class ProjectionJ(ParametricSingleGate):
    r"""Measurement-plane rotation J(theta) used by MBQC transpilation (reference: gate.py:1674-1787,
    matrix :1751-1767)."""

    def __init__(self, inputs=None, nqubit=1, wires=None, plane='xy', controls=None, condition=False,
                 den_mat=False, tsr_mode=False, requires_grad=False):
        self.plane = plane.lower()
        super().__init__(name='ProjectionJ', inputs=inputs, nqubit=nqubit, wires=wires, controls=controls,
                         condition=condition, den_mat=den_mat, tsr_mode=tsr_mode, requires_grad=requires_grad)

    def get_matrix(self, theta: Any) -> torch.Tensor:
        theta = _prep(self.inputs_to_tensor(theta))
        if self.plane in ('xy', 'yx'):
            one = torch.ones_like(theta) + 0j
            e_m = torch.exp(-1j * theta)
            return _mat([one, e_m, one, -e_m], 2) / 2**0.5
        if self.plane in ('yz', 'zy'):
            cps = torch.cos(theta / 2) + torch.sin(theta / 2) + 0j
            cms = torch.cos(theta / 2) - torch.sin(theta / 2) + 0j
            return _mat([cps, -1j * cms, cms, 1j * cps], 2) / 2**0.5
        if self.plane in ('zx', 'xz'):
            cos = torch.cos(theta / 2)
            sin = torch.sin(theta / 2)
            return _mat([cos, sin, sin, -cos], 2) + 0j
        raise ValueError(f'Unsupported measurement plane: {self.plane}')

    def extra_repr(self) -> str:
        return super().extra_repr() + f', plane={self.plane}'


class CombinedSingleGate(SingleGate):
    """Product of single-qubit gates on one wire, applied as one 2x2 matrix
    (reference: gate.py:1790-1903, matrix :1837-1848)."""

    def __init__(self, gates, name=None, nqubit=1, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)
        for g in gates:
            g.nqubit, g.wires, g.controls = self.nqubit, self.wires, self.controls
            g.condition, g.den_mat, g.tsr_mode = self.condition, self.den_mat, self.tsr_mode
        self.gates = nn.ModuleList(gates)
        self.update_npara()
        self.update_matrix()

    def get_matrix(self) -> torch.Tensor:
        matrix = None
        for g in self.gates:
            matrix = g.update_matrix() if matrix is None else g.update_matrix() @ matrix
        return matrix

    def update_matrix(self) -> torch.Tensor:
        matrix = self.get_matrix()
        self.matrix = matrix.detach()
        return matrix

    def get_derivative(self, inputs: Any) -> torch.Tensor:
        """d(matrix)/d(each parameter): product rule over the factors (reference: gate.py:1850-1863)."""
        if not isinstance(inputs, torch.Tensor):
            inputs = torch.tensor(inputs, dtype=torch.float)
        inputs = inputs.reshape(self.npara)
        mats = [g.update_matrix() for g in self.gates]
        out, count = [], 0
        for i, g in enumerate(self.gates):
            if g.npara == 0:
                continue
            du = g.get_derivative(inputs[count : count + g.npara])
            du = du.unsqueeze(0) if du.ndim == 2 else du
            for d in du:
                acc = None
                for j, m in enumerate(mats):
                    term = d if j == i else m
                    acc = term if acc is None else term @ acc
                out.append(acc)
            count += g.npara
        return torch.stack(out)

    def update_npara(self) -> None:
        self.npara = sum(g.npara for g in self.gates)

    def add(self, gate: SingleGate) -> None:
        gate.nqubit, gate.wires, gate.controls = self.nqubit, self.wires, self.controls
        gate.condition, gate.den_mat, gate.tsr_mode = self.condition, self.den_mat, self.tsr_mode
        self.gates.append(gate)
        self.matrix = gate.matrix @ self.matrix
        self.npara += gate.npara

    def init_para(self, inputs: Any = None) -> None:
        count = 0
        for g in self.gates:
            if g.npara == 0:
                continue
            g.init_para(None if inputs is None else inputs[..., count : count + g.npara])
            count += g.npara
        self.update_matrix()

    def inverse(self) -> 'CombinedSingleGate':
        # a NEW gate, as the reference builds one (gate.py:1883-1900): a shallow copy would share ``_modules`` with
        # ``self``, so assigning ``inv.gates`` would also replace the original's factors
        name = self.name + '_dagger' if isinstance(self.name, str) else self.name
        return CombinedSingleGate(gates=[g.inverse() for g in reversed(self.gates)], name=name, nqubit=self.nqubit,
                                  wires=self.wires, controls=self.controls, condition=self.condition,
                                  den_mat=self.den_mat, tsr_mode=self.tsr_mode)


# ======================================================================================================
# two-qubit gates
# ======================================================================================================
class CNOT(DoubleControlGate):
    """CNOT with wires = [control, target] (reference: gate.py:1906-1960, matrix :1934)."""

    _sub_kind = 'x'

    def __init__(self, nqubit=2, wires=None, den_mat=False, tsr_mode=False):
        super().__init__(name='CNOT', nqubit=nqubit, wires=wires, den_mat=den_mat, tsr_mode=tsr_mode)
        self.register_buffer('matrix', torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]]) + 0j)
        self.nancilla = 2


def _swap_prims(gate: Gate, a: int, b: int, extra_controls: list[int]) -> list[Prim]:
    """SWAP(a, b) = CNOT(a,b) CNOT(b,a) CNOT(a,b): three exact bit-flip permutations."""
    x = gate.matrix.new_tensor([[0, 1], [1, 0]])
    ca, cb = gate._bits([a])[0], gate._bits([b])[0]
    ec = gate._bits(extra_controls)
    return [Prim('x', x, (cb,), (ca,) + ec), Prim('x', x, (ca,), (cb,) + ec), Prim('x', x, (cb,), (ca,) + ec)]


class Swap(DoubleGate):
    """SWAP (reference: gate.py:1963-2023, matrix :2006)."""

    def __init__(self, nqubit=2, wires=None, controls=None, condition=False, den_mat=False, tsr_mode=False):
        super().__init__(name='Swap', nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)
        self.register_buffer('matrix', torch.tensor([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]]) + 0j)

    def prims(self, decompose: bool = True) -> list[Prim]:
        if decompose:
            return _swap_prims(self, self.wires[0], self.wires[1], self.controls)
        return super().prims(decompose)


class ImaginarySwap(DoubleGate):
    """iSWAP (reference: gate.py:2026-2082, matrix :2069)."""

    def __init__(self, nqubit=2, wires=None, controls=None, condition=False, den_mat=False, tsr_mode=False):
        super().__init__(name='ImaginarySwap', nqubit=nqubit, wires=wires, controls=controls, condition=condition,
                         den_mat=den_mat, tsr_mode=tsr_mode)
        self.register_buffer('matrix', torch.tensor([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]]))


def _param_double(cls_name: str, gate_name: str, builder, kind: str = 'gen', doc: str = '', mode2: int = 0):
    def __init__(self, inputs=None, nqubit=2, wires=None, controls=None, condition=False, den_mat=False,
                 tsr_mode=False, requires_grad=False):
        ParametricDoubleGate.__init__(self, name=gate_name, inputs=inputs, nqubit=nqubit, wires=wires,
                                      controls=controls, condition=condition, den_mat=den_mat, tsr_mode=tsr_mode,
                                      requires_grad=requires_grad)

    def get_matrix(self, theta):
        return builder(_prep(self.inputs_to_tensor(theta)))

    return type(cls_name, (ParametricDoubleGate,),
                {'__init__': __init__, 'get_matrix': get_matrix, '_kernel_kind': kind, '_kernel_mode2': mode2, '__doc__': doc})


def _antidiag(entries: list[torch.Tensor]) -> torch.Tensor:
    return torch.stack(entries, dim=-1).diag_embed().flip(-1)


def _rxx(theta):
    cos = torch.cos(theta / 2)
    isin = torch.sin(theta / 2) * 1j
    return _diag([cos, cos, cos, cos]) + _antidiag([-isin, -isin, -isin, -isin])


def _ryy(theta):
    cos = torch.cos(theta / 2)
    isin = torch.sin(theta / 2) * 1j
    return _diag([cos, cos, cos, cos]) + _antidiag([isin, -isin, -isin, isin])


def _rzz(theta):
    e_m = torch.exp(-1j * theta / 2)
    e_p = torch.exp(1j * theta / 2)
    return _diag([e_m, e_p, e_p, e_m])


def _embed_middle(block: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """block_diag(1, block(2x2), 1) with optional leading batch dim."""
    out = torch.zeros(*block.shape[:-2], 4, 4, dtype=block.dtype, device=block.device)
    out[..., 0, 0] = 1
    out[..., 3, 3] = 1
    out[..., 1:3, 1:3] = block
    return out


def _rxy(theta):
    cos = torch.cos(theta / 2) + 0j
    isin = torch.sin(theta / 2) * 1j
    return _embed_middle(_mat([cos, -isin, -isin, cos], 2), theta)


def _rbs(theta):
    cos = torch.cos(theta)
    sin = torch.sin(theta)
    return _embed_middle(_mat([cos, sin, -sin, cos], 2) + 0j, theta)


# (mode2: the structure of the 4x4 matrix the class promises -- include/dq_hip.h, DQ_MODE_XCPLX = 5: non-zero only on the
# blocks (00, 11) and (01, 10); DQ_MODE_XREAL = 4: and real)
Rxx = _param_double('Rxx', 'Rxx', _rxx, mode2=5, doc='exp(-i theta XX / 2) (reference: gate.py:2085-2155, matrix :2139-2146).')
Ryy = _param_double('Ryy', 'Ryy', _ryy, mode2=5, doc='exp(-i theta YY / 2) (reference: gate.py:2158-2238, matrix :2212-2219).')
Rzz = _param_double('Rzz', 'Rzz', _rzz, kind='diag',
                    doc='exp(-i theta ZZ / 2) (reference: gate.py:2241-2309, matrix :2295-2300).')
Rxy = _param_double('Rxy', 'Rxy', _rxy, mode2=5, doc='exp(-i theta (XX+YY) / 4) (reference: gate.py:2312-2390, :2366-2373).')
ReconfigurableBeamSplitter = _param_double(
    'ReconfigurableBeamSplitter', 'ReconfigurableBeamSplitter', _rbs, mode2=4,
    doc='RBS gate (reference: gate.py:2393-2479, matrix :2455-2462).')


# ======================================================================================================
# three-qubit gates
# ======================================================================================================
class Toffoli(TripleGate):
    """CCX with wires = [control1, control2, target] (reference: gate.py:2482-2649, matrix :2521-2536)."""

    def __init__(self, nqubit=3, wires=None, den_mat=False, tsr_mode=False):
        super().__init__(name='Toffoli', nqubit=nqubit, wires=wires, den_mat=den_mat, tsr_mode=tsr_mode)
        m = torch.eye(8) + 0j
        m[6:8, 6:8] = torch.tensor([[0, 1], [1, 0]]) + 0j
        self.register_buffer('matrix', m)

    def prims(self, decompose: bool = True) -> list[Prim]:
        return [Prim('x', self.matrix[6:8, 6:8], self._bits([self.wires[2]]), self._bits(self.wires[:2]))]


class Fredkin(TripleGate):
    """CSWAP with wires = [control, target1, target2] (reference: gate.py:2652-2742, matrix :2691-2706)."""

    def __init__(self, nqubit=3, wires=None, den_mat=False, tsr_mode=False):
        super().__init__(name='Fredkin', nqubit=nqubit, wires=wires, den_mat=den_mat, tsr_mode=tsr_mode)
        m = torch.eye(8) + 0j
        m[4:8, 4:8] = torch.tensor([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]]) + 0j
        self.register_buffer('matrix', m)

    def prims(self, decompose: bool = True) -> list[Prim]:
        if decompose:
            return _swap_prims(self, self.wires[1], self.wires[2], [self.wires[0]])
        return [Prim('gen', self.matrix[4:8, 4:8], self._bits(self.wires[1:]), self._bits([self.wires[0]]))]


# ======================================================================================================
# arbitrary gates
# ======================================================================================================
class UAnyGate(ArbitraryGate):
    """User-supplied unitary on ``wires`` / ``minmax`` (reference: gate.py:2745-2788)."""

    def __init__(self, unitary, nqubit=1, wires=None, minmax=None, controls=None, name='UAnyGate', den_mat=False,
                 tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        if not isinstance(unitary, torch.Tensor):
            unitary = torch.tensor(unitary, dtype=torch.cfloat).reshape(-1, 2 ** len(self.wires))
        assert unitary.dtype in (torch.cfloat, torch.cdouble)
        assert unitary.shape[-1] == unitary.shape[-2] == 2 ** len(self.wires)
        eye = torch.eye(unitary.shape[-1], dtype=unitary.dtype, device=unitary.device)
        assert torch.allclose(unitary @ unitary.mH, eye, rtol=1e-5, atol=1e-4), 'Please check the unitary matrix'
        # the reference accepts 1e-4; the adjoint method's reverse sweep must then tell U^-1 from U^dagger (executor)
        self._exact_unitary = bool(torch.allclose(unitary @ unitary.mH, eye, rtol=0.0, atol=2e-6))
        self.register_buffer('matrix', unitary)
        self._kind_cache: tuple | None = None

    @property
    def _kernel_kind(self) -> str:
        """'diag' when the CURRENT matrix is exactly diagonal (the diagonal kernels ignore off-diagonal entries),
        re-derived whenever the buffer is replaced or written in place (``load_state_dict``, ``.to``): the test
        reads the matrix values, so its result is cached on the buffer's identity and version counter."""
        m = self.matrix
        ver = tensor_version(m)
        key = (m.data_ptr(), ver, m.device, m.dtype)
        if ver is None or self._kind_cache is None or self._kind_cache[0] != key:
            diag_only = m.ndim == 2 and len(self.wires) <= 2 and bool(
                (m == torch.diag_embed(m.diagonal(dim1=-2, dim2=-1))).all())
            self._kind_cache = (key, 'diag' if diag_only else 'gen')
        return self._kind_cache[1]

    def update_matrix(self) -> torch.Tensor:
        return self.matrix.mH if self.inv_mode else self.matrix


class LatentGate(ArbitraryGate):
    """Unitary obtained from the polar factor (u @ vh of the SVD) of a trainable latent matrix
    (reference: gate.py:2791-2864, matrix :2836-2840)."""

    def __init__(self, inputs=None, nqubit=1, wires=None, minmax=None, controls=None, name='LatentGate',
                 den_mat=False, tsr_mode=False, requires_grad=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        self.requires_grad = requires_grad
        self.init_para(inputs)

    def inputs_to_tensor(self, inputs: Any = None) -> torch.Tensor:
        d = 2 ** len(self.wires)
        if inputs is None:
            return torch.randn(d, d)
        if not isinstance(inputs, (torch.Tensor, nn.Parameter)):
            inputs = torch.tensor(inputs, dtype=torch.float)
        return inputs.reshape(d, d)

    def get_matrix(self, inputs: Any) -> torch.Tensor:
        latent = self.inputs_to_tensor(inputs) + 0j
        u, _, vh = torch.linalg.svd(latent)
        return u @ vh

    def update_matrix(self) -> torch.Tensor:
        latent = self.latent.mH if self.inv_mode else self.latent
        matrix = self.get_matrix(latent)
        self.matrix = matrix.detach()
        return matrix

    def get_derivative(self, latent: Any) -> torch.Tensor:
        latent = self.inputs_to_tensor(latent)
        du = jacobian(self._real_wrapper, latent).permute(3, 4, 0, 1, 2)
        return du[..., 0] + du[..., 1] * 1j

    def init_para(self, inputs: Any = None) -> None:
        latent = self.inputs_to_tensor(inputs)
        if self.requires_grad:
            self.latent = nn.Parameter(latent)
        else:
            self.register_buffer('latent', latent)
        self.update_matrix()
        self.npara = self.latent.numel()


class HamiltonianGate(ArbitraryGate):
    """exp(-i H t).  ``hamiltonian`` is a list such as ``[[0.5, 'x0y1'], [-1, 'z3y1']]`` (coefficient,
    Pauli letters each followed by its wire) or a dense tensor on ``wires`` / ``minmax``
    (reference: gate.py:2867-3024, matrix :2990-2994)."""

    _complex_buffers = ('ham_tsr',)

    def __init__(self, hamiltonian, t=None, nqubit=1, wires=None, minmax=None, controls=None, name='HamiltonianGate',
                 den_mat=False, tsr_mode=False, requires_grad=False):
        self.nqubit = nqubit
        self.ham_lst = None
        if isinstance(hamiltonian, list):
            self.ham_lst = self._terms(hamiltonian)
            wires = None
            minmax = self.get_minmax(hamiltonian)
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        self.npara = 1
        self.requires_grad = requires_grad
        self.register_buffer('ham_tsr', self._ham_matrix(hamiltonian))
        self.init_para([None, t])

    @staticmethod
    def _terms(ham: list) -> list[tuple[float, list[tuple[str, int]]]]:
        import re

        if len(ham) == 2 and isinstance(ham[1], str):
            ham = [ham]
        out = []
        for pair in ham:
            assert isinstance(pair, list) and isinstance(pair[1], str), 'Invalid input type'
            factors = [(p.lower(), int(w)) for p, w in re.findall(r'([xyzXYZ])(\d+)', pair[1])]
            out.append((pair[0], factors))
        return out

    def get_minmax(self, hamiltonian: list) -> list[int]:
        wires = [w for _, fs in self._terms(hamiltonian) for _, w in fs]
        return [min(wires), max(wires)]

    def _ham_matrix(self, ham: Any) -> torch.Tensor:
        if not isinstance(ham, list):
            ham = ham if isinstance(ham, torch.Tensor) else torch.tensor(ham, dtype=torch.cfloat)
            return ham if ham.is_complex() else ham + 0j
        paulis = {
            'x': torch.tensor([[0, 1], [1, 0]], dtype=torch.cfloat),
            'y': torch.tensor([[0, -1j], [1j, 0]]),
            'z': torch.tensor([[1, 0], [0, -1]], dtype=torch.cfloat),
        }
        lo, hi = self.minmax
        total = None
        for coef, factors in self._terms(ham):
            lst = [torch.eye(2, dtype=torch.cfloat)] * (hi - lo + 1)
            for p, w in factors:
                lst[w - lo] = paulis[p]
            term = multi_kron(lst) * coef
            total = term if total is None else total + term
        return total

    def inputs_to_tensor(self, inputs: Any = None):
        if inputs is None:
            return self.ham_tsr, torch.rand(1)[0]
        if isinstance(inputs, (list, tuple)) and len(inputs) == 2 and not isinstance(inputs[0], (int, float)):
            ham, t = inputs
        else:
            ham, t = None, inputs
        ham_tsr = self.ham_tsr if ham is None else self._ham_matrix(ham).to(self.ham_tsr)
        while isinstance(t, list):
            t = t[0]
        if t is None:
            t = torch.rand(1)[0]
        return ham_tsr, _as_param_tensor(t)

    def get_matrix(self, hamiltonian: Any, t: Any) -> torch.Tensor:
        ham, t = self.inputs_to_tensor([hamiltonian, t])
        t = _prep(t)
        if _is_batched(t):
            return torch.linalg.matrix_exp(-1j * ham * t.reshape(-1, 1, 1))
        return torch.linalg.matrix_exp(-1j * ham * t)

    def update_matrix(self) -> torch.Tensor:
        t = -self.t if self.inv_mode else self.t
        matrix = self.get_matrix(self.ham_tsr, t)
        assert matrix.shape[-1] == matrix.shape[-2] == 2 ** len(self.wires)
        self.matrix = matrix.detach()
        return matrix

    def _real_wrapper(self, x: Any) -> torch.Tensor:
        return torch.view_as_real(self.get_matrix(self.ham_tsr, x))

    def get_derivative(self, t: Any) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            t = torch.tensor(t, dtype=torch.float)
        du = jacobian(self._real_wrapper, t.squeeze())
        return du[..., 0] + du[..., 1] * 1j

    def init_para(self, inputs: Any = None) -> None:
        ham, t = self.inputs_to_tensor(inputs)
        self.register_buffer('ham_tsr', ham)
        if self.requires_grad:
            self.t = nn.Parameter(t)
        else:
            self.register_buffer('t', t)
        self.update_matrix()


class _FlatGate:
    """Mixin of the gates that have no matrix primitive and run through ``apply_flat`` -- (B, 2**n) -> (B, 2**n) -- between
    two fused stretches of a circuit (``QubitCircuit._run_operators``; ``Reset`` uses the same seam under its older
    name ``_state_dependent``).  What has no route yet is refused by name."""

    _runs_flat = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if kwargs.get('den_mat'):
            self._refuse('den_mat=True (density matrices)')

    def _refuse(self, what: str):
        raise NotImplementedError(f'{type(self).__name__}: {what} is not supported (the gate runs as a stand-alone pass over '
                                  'a state vector on one device)')

    @staticmethod
    def _constant(t: torch.Tensor, name: str, noun: str, plural: bool = False) -> None:
        """The gate's table carries no gradient: one that asks for it is refused by name."""
        if t.requires_grad:
            raise ValueError(f'{name}: {noun} are constants -- gradients with respect to them are not supported; detach() them'
                             if plural else
                             f'{name}: {noun} is a constant -- gradients with respect to its entries are not supported; '
                             'detach() it')

    def _mark_precision(self, device: torch.device) -> None:
        """For a table that does not tell the circuit's precision -- integers, or angles that may be float64 in a complex64
        circuit: a marker that follows ``.to()`` / ``.double()`` of the circuit, which ``_state_like`` reads instead."""
        self.register_buffer('_like', torch.zeros((), device=device), persistent=False)

    def prims(self, decompose: bool = True) -> list[Prim]:
        self._refuse('a matrix primitive -- fused passes, DistributedQubitCircuit (sharded states) --')

    def dm_prims(self, decompose: bool = True) -> list[Prim]:
        self._refuse('den_mat=True (density matrices)')

    def op_den_mat(self, x: torch.Tensor) -> torch.Tensor:
        self._refuse('den_mat=True (density matrices)')

    def op_dist_state(self, x):
        self._refuse('DistributedQubitCircuit (a sharded state)')

    def qasm_refusal(self):
        self._refuse('qasm()')

    def op_state(self, x: torch.Tensor) -> torch.Tensor:
        shape = x.shape
        return self.apply_flat(x.reshape(shape[0], -1)).reshape(shape)

    def _state_like(self) -> tuple[torch.dtype, torch.device]:
        """Complex dtype and device of the states the gate's table (or its precision marker) belongs to."""
        t = getattr(self, '_like', None)
        if t is None:
            t = self._table()
        return (t.dtype if t.is_complex() else (torch.complex128 if t.dtype == torch.float64 else torch.complex64)), t.device

    def get_unitary(self) -> torch.Tensor:
        dtype, device = self._state_like()
        with torch.no_grad():
            cols = self.apply_flat(torch.eye(2**self.nqubit, dtype=dtype, device=device))
        return cols.T.contiguous()


class DiagonalGate(_FlatGate, ArbitraryGate):
    """A fixed diagonal unitary on ``wires`` / ``minmax`` given by its 2^k complex entries, ``wires[0]`` the most significant
    bit of the entry index (the matrix convention of ``UAnyGate``): one multiplication per amplitude, one read and one write
    of the state for any k up to n (``dq_apply_diag_*``) -- a phase oracle over all wires, where a dense matrix has no
    route beyond 10.  The entries' moduli are checked to the 1e-4 that ``UAnyGate`` applies to its matrix."""

    _complex_buffers = ('diag',)

    def __init__(self, diag, nqubit=1, wires=None, minmax=None, controls=None, name='DiagonalGate', den_mat=False,
                 tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        if not isinstance(diag, torch.Tensor):
            diag = torch.tensor(diag, dtype=torch.cfloat)
        self._constant(diag, 'DiagonalGate', 'the table')
        if not diag.is_complex():
            diag = diag.to(torch.cdouble if diag.dtype == torch.float64 else torch.cfloat)
        diag = diag.reshape(-1)
        assert diag.shape[0] == 2 ** len(self.wires), f'a diagonal on {len(self.wires)} wires has {2 ** len(self.wires)} entries'
        assert torch.allclose(diag.abs(), torch.ones_like(diag.real), rtol=1e-5, atol=1e-4), 'Please check the diagonal entries'
        self.register_buffer('diag', diag)

    def _table(self) -> torch.Tensor:
        return self.diag

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        diag = self.diag.conj().resolve_conj() if self.inv_mode else self.diag
        return ops.diag_mul(x, diag, self._bits(self.wires), self._bits(self.controls))


class PermutationGate(_FlatGate, ArbitraryGate):
    """A classical reversible map ``|x> -> |perm(x)>`` on ``wires`` / ``minmax`` given by its table of 2^k integers,
    ``wires[0]`` the most significant bit of ``x`` (the matrix convention of ``UAnyGate``: the gate is the 0/1 matrix
    ``M[perm[x], x] = 1``) -- a bit oracle, a modular multiplication, a shift: one read and one write of the state for any
    k up to 31, amplitudes copied bit for bit (``dq_apply_permutation_*``), where a dense matrix does 2^k multiply-adds per
    amplitude and has no route beyond 10 wires.  ``perm`` must be a bijection of ``range(2^k)``; it is checked here, once.
    The gate keeps ``perm`` and its inverse ``inv`` as int32 buffers."""

    def __init__(self, perm, nqubit=1, wires=None, minmax=None, controls=None, name='PermutationGate', den_mat=False,
                 tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        k = len(self.wires)
        if k > 31:
            raise ValueError(f'PermutationGate: at most 31 wires, got {k}')
        if isinstance(perm, torch.Tensor):
            if perm.is_floating_point() or perm.is_complex() or perm.dtype == torch.bool:
                raise ValueError(f'PermutationGate: the table must hold integers, got {perm.dtype}')
            table = perm.detach().reshape(-1).to(torch.int64)
        else:
            entries = list(perm)
            if any(int(v) != v for v in entries):
                raise ValueError('PermutationGate: the table must hold integers')
            table = torch.tensor([int(v) for v in entries], dtype=torch.int64)
        if table.shape[0] != 2**k:
            raise ValueError(f'PermutationGate: a permutation on {k} wires has {2**k} entries, got {table.shape[0]}')
        if int(table.min()) < 0 or int(table.max()) >= 2**k:
            raise ValueError(f'PermutationGate: the entries must lie in [0, {2**k}), got {int(table.min())} .. {int(table.max())}')
        inv = torch.full_like(table, -1)
        inv[table] = torch.arange(2**k, dtype=torch.int64, device=table.device)
        if int(inv.min()) < 0:
            raise ValueError(f'PermutationGate: the table is not a bijection: it repeats entries and never reaches '
                             f'{int((inv < 0).nonzero()[0])}')
        self.register_buffer('perm', table.to(torch.int32))
        self.register_buffer('inv', inv.to(torch.int32))
        self._mark_precision(table.device)              # (integer tables have no precision)

    def tables(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(perm, perm^-1) of the gate as it stands: ``inverse()`` swaps them."""
        return (self.inv, self.perm) if self.inv_mode else (self.perm, self.inv)

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        perm, inv = self.tables()
        return ops.permute_basis(x, perm, self._bits(self.wires), self._bits(self.controls), inv=inv)

    def extra_repr(self) -> str:
        s = f'wires={self.wires}, entries={self.perm.numel()}'
        return s if self.controls == [] else s + f', controls={self.controls}'


def _mux_wires(gate: 'ArbitraryGate', name: str) -> int:
    """k of a multiplexer on ``gate.wires`` = k select wires, most significant first, then the target."""
    k = len(gate.wires) - 1
    if k < 1:
        raise ValueError(f'{name}: wires lists at least one select wire and then the target, got {gate.wires}')
    return k


class MultiplexedGate(_FlatGate, ArbitraryGate):
    """A multiplexer (uniformly controlled gate): for every value s of the k select wires its own one-qubit unitary
    ``unitaries[s]`` on the target.  ``wires`` lists the select wires, the most significant bit of s first, and then the
    target as the LAST wire, so that the gate equals ``UAnyGate(block_diag(U_0, .., U_{2^k - 1}), wires=wires)`` -- but
    runs as one read and one write of the state for any k up to n - 1 (``dq_apply_mux_*``), where the dense matrix does
    2^(k+1) multiply-adds per amplitude and has no route beyond 10 wires.  Every block is checked for unitarity to the
    1e-4 that ``UAnyGate`` applies to its matrix.  The table is a constant: it carries no gradient."""

    _complex_buffers = ('unitaries',)

    def __init__(self, unitaries, nqubit=1, wires=None, minmax=None, controls=None, name='MultiplexedGate', den_mat=False,
                 tsr_mode=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        k = _mux_wires(self, 'MultiplexedGate')
        if not isinstance(unitaries, torch.Tensor):
            unitaries = torch.tensor(unitaries, dtype=torch.cfloat)
        self._constant(unitaries, 'MultiplexedGate', 'the table')
        if not unitaries.is_complex():
            unitaries = unitaries.to(torch.cdouble if unitaries.dtype == torch.float64 else torch.cfloat)
        if unitaries.shape != (2**k, 2, 2):
            raise ValueError(f'MultiplexedGate: {k} select wires take a table of shape ({2**k}, 2, 2), got '
                             f'{tuple(unitaries.shape)}')
        eye = torch.eye(2, dtype=unitaries.dtype, device=unitaries.device)
        if not torch.allclose(unitaries @ unitaries.mH, eye.expand_as(unitaries), rtol=1e-5, atol=1e-4):
            raise ValueError('MultiplexedGate: a block of the table is not unitary')
        self.register_buffer('unitaries', unitaries.resolve_conj().contiguous())

    def _table(self) -> torch.Tensor:
        return self.unitaries

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        (target,) = self._bits(self.wires[-1:])
        return ops.mux_apply(x, self.unitaries, 'u', target, self._bits(self.wires[:-1]), self._bits(self.controls),
                             dagger=self.inv_mode)

    def extra_repr(self) -> str:
        s = f'select={self.wires[:-1]}, target={self.wires[-1]}'
        return s if self.controls == [] else s + f', controls={self.controls}'


class MultiplexedRotation(_FlatGate, ArbitraryGate):
    """A multiplexed rotation (uniformly controlled Rx / Ry / Rz): ``R_axis(angles[s])`` on the target for every value s of
    the k select wires.  ``wires`` lists the select wires, the most significant bit of s first, and then the target as
    the LAST wire: the gate equals ``UAnyGate(block_diag(R(angles[0]), ..), wires=wires)``, and equals the 2^k
    multi-controlled rotations with X flips it replaces -- in one read and one write of the state.  Cosine and sine of
    ``angles / 2`` are taken in the dtype of the angle buffer, on the host side; the tables made of them -- rows (c, s) for
    'y' (``DQ_MUX_RY``), 2x2 blocks for 'x' (``DQ_MUX_U``), phases over ``wires`` for 'z' (a diagonal operator:
    ``ops.diag_mul``, no multiplexer kernel) -- are formed once per precision and direction and kept.  The angles are
    constants: they carry no gradient -- unless ``requires_grad=True``: the 2^k angles are then one ``nn.Parameter``
    (random when ``angles is None``), the gate runs ``ops.mux_rot`` -- the same kernels forward, one rotation and one binned
    cross reduction (``dq_mux_cross_*``) backward, whatever k is -- and is differentiable to any order in the state and in
    the angles."""

    def __init__(self, axis, angles=None, nqubit=1, wires=None, minmax=None, controls=None, name='MultiplexedRotation',
                 den_mat=False, tsr_mode=False, requires_grad=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        k = _mux_wires(self, 'MultiplexedRotation')
        if axis not in ('x', 'y', 'z'):
            raise ValueError(f"MultiplexedRotation: axis must be 'x', 'y' or 'z', got {axis!r}")
        self.axis = axis
        self.requires_grad = bool(requires_grad)
        if angles is None:
            if not self.requires_grad:
                raise ValueError('MultiplexedRotation: angles=None (random angles) needs requires_grad=True')
            angles = torch.rand(2**k) * (4 * torch.pi)
        angles = _as_param_tensor(angles)
        if not self.requires_grad:
            self._constant(angles, 'MultiplexedRotation', 'the angles', plural=True)
        if angles.is_complex() or not angles.is_floating_point():
            angles = angles.real.to(torch.float) if angles.is_complex() else angles.to(torch.float)
        angles = angles.detach().reshape(-1)
        if angles.shape[0] != 2**k:
            raise ValueError(f'MultiplexedRotation: {k} select wires take {2**k} angles, got {angles.shape[0]}')
        if self.requires_grad:
            self.npara = 2**k
            self.angles = nn.Parameter(angles.clone().contiguous())
        else:
            self.register_buffer('angles', angles.contiguous())
        self._mark_precision(angles.device)             # (the angles may be float64 in a complex64 circuit)

    def init_para(self, inputs: Any = None) -> None:
        """Trainable angles only (the pattern of ``_OneAngle``): new random angles, or ``inputs``, in the parameter's own
        precision and on its device.  Constant angles stay as they are."""
        if not self.requires_grad:
            return
        old = self.angles
        if inputs is None:
            value = torch.rand(old.shape[0]) * (4 * torch.pi)
        else:
            value = _as_param_tensor(inputs).detach().reshape(-1)
            if value.shape[0] != old.shape[0]:
                raise ValueError(f'MultiplexedRotation: {old.shape[0]} angles expected, got {value.shape[0]}')
        self.angles = nn.Parameter(value.to(device=old.device, dtype=old.dtype))

    def table(self, dtype: torch.dtype) -> torch.Tensor:
        """The table of the gate as it stands for states of complex ``dtype``: 'y' (2^k, 2) real rows (c, s), 'x' complex
        (2^k, 2, 2), 'z' complex (2^(k+1),) phases over ``wires`` (the only one that depends on the direction)."""
        a = self.angles
        key = (dtype, a.device, self.inv_mode and self.axis == 'z')
        cache = self.__dict__.get('_mux_tables')
        ver = tensor_version(a)
        if cache is None or cache[0] is not a or ver is None or cache[1] != ver:
            cache = self.__dict__['_mux_tables'] = (a, ver, {})
        t = cache[2].get(key)
        if t is None:
            real = torch.float64 if dtype == torch.complex128 else torch.float32
            if self.axis == 'z':
                half = (-a if self.inv_mode else a) / 2
                t = torch.stack([torch.exp(-1j * half), torch.exp(1j * half)], dim=-1).reshape(-1).to(dtype)
            else:
                c, s = torch.cos(a / 2), torch.sin(a / 2)
                if self.axis == 'y':
                    t = torch.stack([c, s], dim=-1).to(real)
                else:
                    t = torch.stack([c + 0j, -1j * s, -1j * s, c + 0j], dim=-1).reshape(-1, 2, 2).to(dtype)
            cache[2][key] = t = t.contiguous()
        return t

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        if self.requires_grad:                          # (the inverse shares the parameter and negates it here)
            (target,) = self._bits(self.wires[-1:])
            return ops.mux_rot(x, -self.angles if self.inv_mode else self.angles, self.axis, target,
                               self._bits(self.wires[:-1]), self._bits(self.controls))
        t = self.table(x.dtype)
        if self.axis == 'z':
            return ops.diag_mul(x, t, self._bits(self.wires), self._bits(self.controls))
        (target,) = self._bits(self.wires[-1:])
        return ops.mux_apply(x, t, 'ry' if self.axis == 'y' else 'u', target, self._bits(self.wires[:-1]),
                             self._bits(self.controls), dagger=self.inv_mode)

    def extra_repr(self) -> str:
        s = f"axis='{self.axis}', select={self.wires[:-1]}, target={self.wires[-1]}"
        return s if self.controls == [] else s + f', controls={self.controls}'


class _OneAngle:
    """One real parameter, trainable, fixed or encoded, of a flat gate.  Where the gate has no table, ``_state_like`` comes
    from the parameter's device and precision (``.to()`` of the circuit converts it along)."""

    def _one_angle(self, inputs: Any, requires_grad: bool) -> None:
        self.npara = 1
        self.requires_grad = requires_grad
        self.init_para(inputs)

    def inputs_to_tensor(self, inputs: Any = None) -> torch.Tensor:
        while isinstance(inputs, list):
            inputs = inputs[0]
        if inputs is None:
            return torch.rand(())
        return _as_param_tensor(inputs)

    def init_para(self, inputs: Any = None) -> None:
        name = self._param_names[0]
        value = self.inputs_to_tensor(inputs)
        old = getattr(self, name, None)
        if old is not None and not isinstance(value, nn.Parameter):
            # (the parameter stays in the precision `.to()` of the circuit gave it -- `_state_like` reads the circuit's
            # precision from it -- whatever the precision of fresh random values or of encoded data)
            value = value.to(device=old.device, dtype=old.dtype)
        if self.requires_grad:
            setattr(self, name, nn.Parameter(value))
        else:
            self.register_buffer(name, value)

    def _angle(self) -> torch.Tensor:
        value = getattr(self, self._param_names[0])
        return -value if self.inv_mode else value

    def _state_like(self) -> tuple[torch.dtype, torch.device]:
        value = getattr(self, self._param_names[0])
        return (torch.complex128 if value.dtype == torch.float64 else torch.complex64), value.device

    def inverse(self):
        return ArbitraryGate.inverse(self)          # (the copy shares the parameter; `inv_mode` negates it where it is used)

    def extra_repr(self) -> str:
        value = self._angle()
        val = value.item() if value.numel() == 1 else f'<batch of {value.numel()}>'
        s = f'wires={self.wires}, {self._param_names[0]}={val}'
        return s if self.controls == [] else s + f', controls={self.controls}'


class CostPhase(_OneAngle, _FlatGate, ArbitraryGate):
    """``exp(-i t diag(cost))`` with one parameter ``t`` and a classical cost table of 2^k real entries over ``wires`` /
    ``minmax`` (``wires[0]`` the most significant bit of the entry index): a whole QAOA cost layer -- any cost, not only a
    short Ising polynomial -- in one read and one write of the state (``dq_apply_cost_*``).  ``t`` is trainable
    (``requires_grad=True``), fixed (``inputs``), or fed from the circuit's data (``encode=True``; a batch of data gives one
    ``t`` per sample).  The table is a constant: it carries no gradient.  The kernels read it in the state's real
    precision, so keep it in that precision (``.to()`` of the circuit converts it along) to spare a conversion per
    forward."""

    _param_names = ('t',)

    def __init__(self, cost, nqubit=1, wires=None, minmax=None, inputs=None, controls=None, name='CostPhase',
                 den_mat=False, tsr_mode=False, requires_grad=False):
        super().__init__(name=name, nqubit=nqubit, wires=wires, minmax=minmax, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        if not isinstance(cost, torch.Tensor):
            cost = torch.tensor(cost, dtype=torch.float)
        self._constant(cost, 'CostPhase', 'the cost table')
        if cost.is_complex() or not cost.is_floating_point():
            raise ValueError(f'CostPhase: the cost table must be real floating point, got {cost.dtype}')
        cost = cost.reshape(-1)
        assert cost.shape[0] == 2 ** len(self.wires), f'a cost on {len(self.wires)} wires has {2 ** len(self.wires)} entries'
        self.register_buffer('cost', cost)
        self._one_angle(inputs, requires_grad)

    def _table(self) -> torch.Tensor:
        return self.cost

    _state_like = _FlatGate._state_like             # (the table tells the precision, not the parameter ...)

    def init_para(self, inputs: Any = None) -> None:
        # (... which, unlike `_OneAngle`'s, takes the precision of the values it is given: float64 data in a complex64
        # circuit stay float64)
        t = self.inputs_to_tensor(inputs)
        if t.device != self.cost.device and not isinstance(t, nn.Parameter):
            t = t.to(self.cost.device)
        if self.requires_grad:
            self.t = nn.Parameter(t)
        else:
            self.register_buffer('t', t)

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        return ops.cost_phase(x, self.cost, self._angle(), self._bits(self.wires), self._bits(self.controls))


def _pauli_letters(pauli: str, what: str) -> str:
    if not isinstance(pauli, str) or any(ch not in 'xyzi' for ch in pauli.lower()):
        raise ValueError(f'{what}: a Pauli string is written with the letters x, y, z, i; got {pauli!r}')
    return pauli.lower()


def _pauli_bit_masks(nqubit: int, letters: str, wires: list[int]) -> tuple[int, int]:
    """(xmask, zmask) over index bits -- wire 0 is the most significant bit, a Y sets its bit in both."""
    xmask = zmask = 0
    for ch, w in zip(letters, wires):
        bit = 1 << (nqubit - 1 - w)
        if ch in 'xy':
            xmask |= bit
        if ch in 'yz':
            zmask |= bit
    return xmask, zmask


class PauliRot(_OneAngle, _FlatGate, ArbitraryGate):
    """``exp(-i theta/2 P)`` for a Pauli string ``P``: ``pauli`` holds one letter of ``xyzi`` (either case) per wire of
    ``wires`` (all wires by default).  One read and one write of the state whatever the weight of P, on any wires of the
    register (``dq_apply_pauli_axpby_*``) -- where a dense matrix has no route beyond a span of 10.  ``theta`` is trainable
    (``requires_grad=True``), fixed (``inputs``), or fed from the circuit's data (``encode=True``; a batch of data gives one
    ``theta`` per sample).  The gate's ``wires`` are those with a letter other than ``i``."""

    _param_names = ('theta',)
    get_matrix = None                                   # (no matrix: not one of the circuit's vectorised one-angle gates)

    def __init__(self, pauli, nqubit=1, wires=None, inputs=None, controls=None, name='PauliRot', den_mat=False,
                 tsr_mode=False, requires_grad=False):
        letters = _pauli_letters(pauli, 'PauliRot')
        if wires is None:
            wires = list(range(nqubit))
        if isinstance(wires, int):
            wires = [wires]
        if len(letters) != len(wires):
            raise ValueError(f'PauliRot: {len(letters)} letters for {len(wires)} wires')
        if set(letters) <= {'i'}:
            raise ValueError('PauliRot: the string is the identity -- a global phase, not a gate')
        self.pauli = ''.join(ch for ch in letters if ch != 'i')
        super().__init__(name=name, nqubit=nqubit, wires=[w for ch, w in zip(letters, wires) if ch != 'i'], controls=controls,
                         den_mat=den_mat, tsr_mode=tsr_mode)
        self._one_angle(inputs, requires_grad)

    def masks(self) -> tuple[int, int]:
        return _pauli_bit_masks(self.nqubit, self.pauli, self.wires)

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        xmask, zmask = self.masks()
        return ops.pauli_rot(x, xmask, zmask, self._angle(), self._bits(self.controls))

    def extra_repr(self) -> str:
        return f'pauli={self.pauli!r}, ' + _OneAngle.extra_repr(self)


class PauliEvolution(_OneAngle, _FlatGate, ArbitraryGate):
    """A Trotter product for ``exp(-i H t)``, ``H = sum_j coef_j P_j`` given as ``HamiltonianGate`` takes it --
    ``[[0.5, 'x0y1'], [-1, 'z3y1']]``, real coefficients, wires anywhere in the register -- with one parameter ``t``:
    ``steps`` slices of Pauli rotations ``exp(-i coef_j (t / steps) P_j)`` (``order=1``: the terms in the order given;
    ``order=2``: the symmetric product, half angles out and back), each rotation one read and one write of the state
    (:class:`PauliRot`).  Exact when the terms commute; differentiable through ``t``."""

    _param_names = ('t',)

    def __init__(self, hamiltonian, t=None, nqubit=1, steps=1, order=1, name='PauliEvolution', den_mat=False, tsr_mode=False,
                 requires_grad=False):
        if not isinstance(hamiltonian, list) or not hamiltonian:
            raise ValueError("PauliEvolution: the Hamiltonian is a list such as [[0.5, 'x0y1'], [-1, 'z3y1']]")
        if order not in (1, 2):
            raise ValueError(f'PauliEvolution: order must be 1 or 2, got {order!r}')
        if not isinstance(steps, int) or steps < 1:
            raise ValueError(f'PauliEvolution: steps must be a positive integer, got {steps!r}')
        self.terms = []
        for coef, factors in HamiltonianGate._terms(hamiltonian):
            ws = [w for _, w in factors]
            if isinstance(coef, complex) or not factors:
                raise ValueError(f'PauliEvolution: a term is a real coefficient and a non-empty Pauli string, got {coef!r}')
            if len(set(ws)) != len(ws):
                raise ValueError(f'PauliEvolution: a wire is repeated within one string (wires {ws})')
            if any(w < 0 or w >= nqubit for w in ws):
                raise ValueError(f'PauliEvolution: wires {ws} outside the register of {nqubit} qubits')
            self.terms.append((float(coef), ''.join(p for p, _ in factors), ws))
        self.steps, self.order = steps, order
        super().__init__(name=name, nqubit=nqubit, wires=sorted({w for _, _, ws in self.terms for w in ws}), den_mat=den_mat,
                         tsr_mode=tsr_mode)
        self._one_angle([t], requires_grad)

    def slice_sequence(self) -> list[tuple[int, float]]:
        """(term, share of its angle) of one slice, in the order applied."""
        m = len(self.terms)
        if self.order == 1 or m == 1:
            seq = [(j, 1.0) for j in range(m)]
        else:                                           # (the last term's two halves meet: one rotation)
            seq = [(j, 0.5) for j in range(m - 1)] + [(m - 1, 1.0)] + [(j, 0.5) for j in range(m - 2, -1, -1)]
        return seq[::-1] if self.inv_mode else seq

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        t = self._angle()
        masks = [_pauli_bit_masks(self.nqubit, letters, ws) for _, letters, ws in self.terms]
        seq = self.slice_sequence()
        for _ in range(self.steps):
            for j, share in seq:
                x = ops.pauli_rot(x, masks[j][0], masks[j][1], t * (2.0 * self.terms[j][0] * share / self.steps))
        return x

    def extra_repr(self) -> str:
        return f'terms={len(self.terms)}, steps={self.steps}, order={self.order}, ' + _OneAngle.extra_repr(self)


def excitation_masks(nqubit: int, create, annihilate, fermionic: bool = True, controls=()) -> tuple[int, int, int, int]:
    """``(xmask, amask, zmask, negate)`` over index bits (wire w is bit ``nqubit - 1 - w``) of ``K = E - E^dagger`` for
    ``E = a^dagger_{create[0]} a^dagger_{create[1]} .. a_{annihilate[0]} a_{annihilate[1]} ..`` under the Jordan-Wigner
    map over wire numbers, ``a_j = (prod_{l<j} Z_l) |0><1|_j``: for every index i0 with the annihilated wires occupied, the
    created ones empty and the controls 1, ``i1 = i0 ^ xmask`` and ``<i1|E|i0> = (-1)^(negate + popc(i0 & zmask))``.
    ``zmask`` holds the wires outside both lists below an odd number of listed wires; the sign of the listed wires
    themselves is found by walking the operator product over one integer; a control inside the string is always 1 where
    the gate acts, so its bit is folded into ``negate``.  ``fermionic=False``: no string and no sign, the qubit excitation."""
    create, annihilate, controls = [int(w) for w in create], [int(w) for w in annihilate], [int(w) for w in controls]
    listed = create + annihilate
    if not create or not annihilate:
        raise ValueError('excitation: create and annihilate each name at least one wire')
    if len(set(listed + controls)) != len(listed + controls):
        raise ValueError(f'excitation: a wire is repeated (create {create}, annihilate {annihilate}, controls {controls})')
    if any(w < 0 or w >= nqubit for w in listed + controls):
        raise ValueError(f'excitation: wires {listed + controls} outside the register of {nqubit} qubits')
    bit = lambda w: 1 << (nqubit - 1 - w)  # noqa: E731
    xmask = sum(bit(w) for w in listed)
    amask = sum(bit(w) for w in annihilate)
    if not fermionic:
        return xmask, amask, 0, 0
    occupied, negate = set(annihilate), 0
    for j, w in enumerate(reversed(listed)):            # (the rightmost operator acts first)
        negate ^= sum(1 for l in occupied if l < w) & 1
        if j < len(annihilate):
            occupied.remove(w)
        else:
            occupied.add(w)
    zmask = 0
    for l in range(nqubit):
        if l not in listed and sum(1 for w in listed if w > l) & 1:
            if l in controls:
                negate ^= 1
            else:
                zmask |= bit(l)
    return xmask, amask, zmask, negate


class ExcitationGate(_OneAngle, _FlatGate, ArbitraryGate):
    """``exp(theta (E - E^dagger))`` for the excitation ``E = a^dagger_{create[0]} a^dagger_{create[1]} .. a_{annihilate[0]}
    a_{annihilate[1]} ..`` (Jordan-Wigner over wire numbers, ``|1>`` occupied): the gate of UCCSD and of every
    particle-number-conserving ansatz, for any number of wires in the two lists.  It is a Givens rotation by the FULL angle
    ``theta`` between the basis states with the annihilated wires occupied and the created ones empty and their partners
    with the two lists swapped, with the sign of the Jordan-Wigner string; every other amplitude is untouched, and the
    kernel reads and writes the rotated pairs only -- 1/2 of the state for a single, 1/8 for a double, half of that per
    control (``dq_apply_excite_axpby_*``).  ``fermionic=False`` drops the string: the qubit excitation.

    Conventions.  The qubit single ``create=[q], annihilate=[p]`` is exactly ``rbs(theta)`` on wires ``[p, q]``
    (``ReconfigurableBeamSplitter``).  PennyLane's ``SingleExcitation(phi, wires=[p, q])`` / ``DoubleExcitation`` rotate by
    HALF their parameter and carry no string: ``SingleExcitation(phi, [p, q])`` is the qubit excitation ``create=[p],
    annihilate=[q], fermionic=False`` at ``theta = phi / 2`` (equally ``create=[q], annihilate=[p]`` at ``theta = -phi / 2``).

    ``theta`` is trainable (``requires_grad=True``), fixed (``inputs``), or fed from the circuit's data (``encode=True``; a
    batch of data gives one ``theta`` per sample)."""

    _param_names = ('theta',)
    get_matrix = None                                   # (no matrix: not one of the circuit's vectorised one-angle gates)

    def __init__(self, create, annihilate, nqubit=1, inputs=None, controls=None, fermionic=True, requires_grad=False,
                 name='ExcitationGate', den_mat=False, tsr_mode=False):
        create = [create] if isinstance(create, int) else list(create)
        annihilate = [annihilate] if isinstance(annihilate, int) else list(annihilate)
        ctrl = [] if controls is None else [controls] if isinstance(controls, int) else list(controls)
        excitation_masks(nqubit, create, annihilate, fermionic, ctrl)           # (the lists are checked there)
        self.create, self.annihilate, self.fermionic = create, annihilate, bool(fermionic)
        super().__init__(name=name, nqubit=nqubit, wires=create + annihilate, controls=controls, den_mat=den_mat,
                         tsr_mode=tsr_mode)
        self._one_angle(inputs, requires_grad)

    def masks(self) -> tuple[int, int, int, int]:
        """``(xmask, amask, zmask, negate)`` over index bits: see :func:`excitation_masks`."""
        return excitation_masks(self.nqubit, self.create, self.annihilate, self.fermionic, self.controls)

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        return ops.excite_rot(x, (*self.masks(), self._bits(self.controls)), self._angle())

    def extra_repr(self) -> str:
        return (f'create={self.create}, annihilate={self.annihilate}, fermionic={self.fermionic}, '
                + _OneAngle.extra_repr(self))


class Reset(Gate):
    r"""Reset qubits to :math:`|0\rangle` (reference: gate.py:3027-3094).

    ``postselect`` in (0, 1): project every wire on that outcome (or on the other one if its probability
    is exactly zero), renormalise and move the amplitude to :math:`|0\rangle` -- per wire one marginal
    reduction and one (non-unitary, per-sample) 2x2 gate launch.  ``postselect=None``: sample the joint
    outcome of the wires, project, renormalise, relabel to :math:`|0..0\rangle`.  The matrices depend on the
    state, so a circuit containing a ``Reset`` runs as separate fused stretches around it."""

    _state_dependent = True

    def __init__(self, nqubit=1, wires=None, postselect=0, tsr_mode=False):
        if wires is None:
            wires = list(range(nqubit))
        super().__init__(name='Reset', nqubit=nqubit, wires=wires, tsr_mode=tsr_mode)
        self.postselect = postselect

    def prims(self, decompose: bool = True) -> list[Prim]:
        raise NotImplementedError('Reset depends on the state: it has no fixed matrix / unitary')

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        n = self.nqubit
        if len(self.wires) == n:
            out = torch.zeros_like(x)
            out[:, 0] = 1
            return out
        if self.postselect in (0, 1):
            ps = self.postselect
            for wire in self.wires:
                bit = n - 1 - wire
                probs = ops.marginal(x, [bit])                                  # (B, 2)
                mask = 1 - torch.sign(probs[:, ps])
                norm = torch.sqrt(probs[:, ps] + mask)
                keep, other = (1 - mask) / norm, mask / norm
                zero = torch.zeros_like(keep)
                row0 = torch.stack([keep, other] if ps == 0 else [other, keep], dim=-1)
                mats = torch.stack([row0, torch.stack([zero, zero], dim=-1)], dim=-2) + 0j   # (B, 2, 2)
                x = ops.apply_gate(x, mats, [bit], [])
            return x
        assert self.postselect is None, 'postselect must be 0, 1 or None'
        wires = sorted(self.wires)
        bits = [n - 1 - w for w in wires]
        probs = ops.marginal(x, bits)                                          # (B, 2**k)
        sample = torch.multinomial(probs.detach().clamp_min(0), 1)             # (B, 1)
        amp = torch.gather(probs, 1, sample) ** -0.5                           # (B, 1)
        d = probs.shape[-1]
        mats = torch.zeros(x.shape[0], d, d, dtype=probs.dtype, device=x.device)
        mats = mats.index_put((torch.arange(x.shape[0], device=x.device), torch.zeros_like(sample[:, 0]),
                               sample[:, 0]), amp[:, 0]) + 0j
        return ops.apply_gate(x, mats, bits, [])

    def op_state(self, x: torch.Tensor) -> torch.Tensor:
        shape = x.shape
        return self.apply_flat(x.reshape(shape[0], -1)).reshape(shape)

    def op_dist_state(self, x):
        raise NotImplementedError('Reset on a sharded state is not supported (nor is it in the reference)')

    def get_unitary(self) -> torch.Tensor:
        raise NotImplementedError('Reset is not unitary')


class Barrier(Gate):
    """No-op separator (reference: gate.py:3097-3126)."""

    def __init__(self, nqubit=1, wires=None, name='Barrier'):
        if wires is None:
            wires = list(range(nqubit))
        super().__init__(name=name, nqubit=nqubit, wires=wires)

    def prims(self, decompose: bool = True) -> list[Prim]:
        return []

    def forward(self, x: Any) -> Any:
        return x

    def get_unitary(self) -> torch.Tensor:
        return torch.eye(2**self.nqubit, dtype=torch.cfloat)
