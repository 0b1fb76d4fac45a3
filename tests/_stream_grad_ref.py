"""Closed-form derivatives of the streaming operations, in numpy complex128, built from the forward references alone
(tests/_diag_ref.py, _pauli_ref.py, _excite_ref.py, _perm_ref.py, _mux_ref.py, _muxgrad_ref.py): nothing here calls ``ops`` or
``backend``.

Convention (PyTorch's): for a real loss L, dL = Re sum conj(g) d(input).  A linear map y = M x therefore has gx = M^+ gy,
a complex parameter p of y = p w has gp = sum conj(w) gy, and a real one the real part of that.  Parameters are one value
per sample, (B,); the gradient of a parameter shared by the samples is the sum of the rows returned here.

A generator family (Pauli strings, excitations) is a linear map G that is 0 off its support S and has G^+ = s G:

    axpby(x; a, c) = a x + c G x on S; x ('gate') or 0 ('map') elsewhere
        gx = axpby(gy; conj a, s conj c), same mode;   ga = sum_S conj(x) gy;   gc = sum conj(G x) gy
    cross(u, v) = sum conj(u) (G v)
        g_u = conj(gz) G v;   g_v = s gz G u
    rot(x; theta) = exp(r theta G) x = y
        gx = rot(gy; -theta);   gtheta = Re sum conj(gy) (r G y)

The diagonal operations with a real table c over the controls' subspace `on`:

    phase(x; t) = exp(-i t c) x on `on`, x elsewhere:   gx = phase(gy; -t);   gt = Im sum_on c conj(gy) y
    scale(x; s) = s c x on `on`, 0 elsewhere:           gx = scale(gy; conj s);   gs = sum_on c conj(x) gy
    cross(a, b) = sum_on c conj(a) b:                   g_a = scale(b; conj gz);   g_b = scale(a; gz)

The binned multiplexer operations (`MuxBins`): G the Pauli ``axis`` on ``target`` inside the controls (Hermitian, and it
maps every bin -- the amplitudes with one select value inside the controls -- to itself); a parameter is a row of 2^k
values per sample, (B, 2^k), and a cross is one number per sample and bin:

    axpby(x; a, c)[i] = a[sub i] x[i] + c[sub i] (G x)[i] inside the controls; x ('gate') or 0 ('map') elsewhere
        gx = axpby(gy; conj a, conj c), same mode;   ga = cross_I(x, gy);   gc = cross_axis(x, gy)
    cross(u, v)[b, s] = sum over bin s of conj(u) (G v)
        g_u = axpby(v; 0, conj gz, 'map');   g_v = axpby(u; 0, gz, 'map')
    rot(x; theta) = axpby(x; cos(theta/2), -i sin(theta/2), 'gate')
        gx = rot(gy; -theta);   gtheta = Im cross(gx, x) / 2

A JVP is the sum of the same partials applied to the tangents; a parameter's tangent moves the support only (a 'map' /
scale term)."""

import numpy as np

import _diag_ref
import _excite_ref
import _mux_ref
import _muxgrad_ref
import _pauli_ref
import _perm_ref


def rows(p, batch):
    """A parameter -- one value, or one per sample -- as (B,)."""
    p = np.asarray(p).reshape(-1)
    return np.broadcast_to(p, (batch,)) if p.shape[0] == 1 else p


def col(p, batch):
    return rows(p, batch).reshape(-1, 1)


# ---- the two generator families ------------------------------------------------------------------------------------------
class PauliStrings:
    """G = P = (xmask, zmask) inside the controls: Hermitian, rot = exp(-i theta/2 P)."""
    sign, rate = +1, -0.5j

    def __init__(self, n, xmask, zmask, controls=()):
        self.n, self.xmask, self.zmask, self.controls = n, xmask, zmask, tuple(controls)

    def support(self):
        return _pauli_ref.inside(self.n, self.controls)

    def axpby(self, x, a, c, mode='gate'):
        return _pauli_ref.axpby_ref(x, self.xmask, self.zmask, rows(a, len(x)), rows(c, len(x)), self.controls, mode)

    def cross(self, u, v):
        return _pauli_ref.cross_ref(u, v, self.xmask, self.zmask, self.controls)

    def rot(self, x, theta):
        return _pauli_ref.rot_ref(x, self.xmask, self.zmask, col(theta, len(x)), self.controls)


class Excitations:
    """G = K = E - E^+ on the pairs of a spec: real and anti-symmetric, rot = exp(theta K)."""
    sign, rate = -1, 1.0

    def __init__(self, n, spec):
        self.n, self.spec = n, spec

    def support(self):
        on = np.ones(1 << self.n, dtype=bool)
        on[_excite_ref.outside(self.n, self.spec)] = False
        return on

    def axpby(self, x, a, c, mode='gate'):
        return _excite_ref.index_axpby(x, self.spec, rows(a, len(x)), rows(c, len(x)), mode)

    def cross(self, u, v):
        return _excite_ref.index_cross(u, v, self.spec)

    def rot(self, x, theta):
        return _excite_ref.index_rot(x, self.spec, col(theta, len(x)))


def gen(fam, x):
    """G x (0 off the support)."""
    return fam.axpby(x, 0.0, 1.0, 'map')


def axpby_vjp(fam, x, a, c, mode, gy):
    gx = fam.axpby(gy, np.conj(a), fam.sign * np.conj(c), mode)
    ga = (np.conj(x) * gy)[:, fam.support()].sum(-1)
    gc = (np.conj(gen(fam, x)) * gy).sum(-1)
    return gx, ga, gc


def axpby_jvp(fam, x, a, c, mode, dx, da, dc):
    return fam.axpby(dx, a, c, mode) + fam.axpby(x, da, dc, 'map')


def cross_vjp(fam, u, v, gz):
    gz = col(gz, len(u))
    return np.conj(gz) * gen(fam, v), fam.sign * gz * gen(fam, u)


def cross_jvp(fam, u, v, du, dv):
    return fam.cross(du, v) + fam.cross(u, dv)


def rot_vjp(fam, x, theta, gy):
    y = fam.rot(x, theta)
    return fam.rot(gy, -np.asarray(theta)), (np.conj(gy) * (fam.rate * gen(fam, y))).sum(-1).real


def rot_jvp(fam, x, theta, dx, dtheta):
    return fam.rot(dx, theta) + col(dtheta, len(x)) * fam.rate * gen(fam, fam.rot(x, theta))


# ---- diagonal operations: `where` = (n, bits, controls) -----------------------------------------------------------------
def phase_vjp(x, c, t, where, gy):
    t = rows(t, len(x))
    y = _diag_ref.phase_ref(x, c, t, *where)
    return _diag_ref.phase_ref(gy, c, -t, *where), _diag_ref.cross_ref(gy, y, c, *where).imag


def phase_jvp(x, c, t, where, dx, dt):
    t = rows(t, len(x))
    y = _diag_ref.phase_ref(x, c, t, *where)
    return _diag_ref.phase_ref(dx, c, t, *where) + _diag_ref.scale_ref(y, c, -1j * rows(dt, len(x)), *where)


def scale_vjp(x, c, s, where, gy):
    return _diag_ref.scale_ref(gy, c, np.conj(rows(s, len(x))), *where), _diag_ref.cross_ref(x, gy, c, *where)


def scale_jvp(x, c, s, where, dx, ds):
    return _diag_ref.scale_ref(dx, c, rows(s, len(x)), *where) + _diag_ref.scale_ref(x, c, rows(ds, len(x)), *where)


def cost_cross_vjp(a, b, c, where, gz):
    gz = rows(gz, len(a))
    return _diag_ref.scale_ref(b, c, np.conj(gz), *where), _diag_ref.scale_ref(a, c, gz, *where)


def cost_cross_jvp(a, b, c, where, da, db):
    return _diag_ref.cross_ref(da, b, c, *where) + _diag_ref.cross_ref(a, db, c, *where)


def diag_mul_vjp(d, where, gy):
    return _diag_ref.diag_ref(gy, np.conj(d), *where)


def diag_mul_jvp(d, where, dx):
    return _diag_ref.diag_ref(dx, d, *where)


# ---- permutations and multiplexers: the forward reference with the inverse table / the dagger ----------------------------
def permute_vjp(perm, bits, controls, gy):
    return _perm_ref.permute_ref(gy, _perm_ref.inverse_of(perm), bits, controls)


def permute_jvp(perm, bits, controls, dx):
    return _perm_ref.permute_ref(dx, perm, bits, controls)


def mux_vjp(blocks, target, bits, controls, dagger, gy):
    return _mux_ref.mux_ref(gy, blocks, target, bits, controls, not dagger)


def mux_jvp(blocks, target, bits, controls, dagger, dx):
    return _mux_ref.mux_ref(dx, blocks, target, bits, controls, dagger)


# ---- the binned multiplexer operations: a parameter is (B, 2^k), a cross (B, 2^k) --------------------------------------
class MuxBins:
    """G = the Pauli ``axis`` on bit ``target`` inside the controls; bin s = the amplitudes inside the controls whose select
    bits ``bits`` (``bits[0]`` the most significant) spell s."""

    def __init__(self, n, axis, target, bits, controls=()):
        self.n, self.axis, self.target, self.bits, self.controls = n, axis, target, tuple(bits), tuple(controls)
        self.count = 1 << len(self.bits)

    def support(self):
        return _muxgrad_ref.inside(self.n, self.controls)

    def axpby(self, x, a, c, mode='gate'):
        return _muxgrad_ref.mux_axpby_ref(x, a, c, self.axis, self.target, self.bits, self.controls, mode)

    def cross(self, u, v, axis=None):
        return _muxgrad_ref.mux_cross_ref(u, v, axis or self.axis, self.target, self.bits, self.controls)

    def rot(self, x, theta):
        return _muxgrad_ref.mux_rot_ref(x, theta, self.axis, self.target, self.bits, self.controls)

    def norms(self, a):
        """|a restricted to bin s| for every sample and bin: (B, 2^k)."""
        inside = np.where(self.support(), np.abs(np.asarray(a).astype(np.complex128)) ** 2, 0.0)
        return np.sqrt(_muxgrad_ref.binned(inside, self.n, self.bits))


def binned_axpby_vjp(fam, x, a, c, mode, gy):
    return fam.axpby(gy, np.conj(a), np.conj(c), mode), fam.cross(x, gy, 'i'), fam.cross(x, gy)


def binned_axpby_jvp(fam, x, a, c, mode, dx, da, dc):
    return fam.axpby(dx, a, c, mode) + fam.axpby(x, da, dc, 'map')


def binned_cross_vjp(fam, u, v, gz):
    zero = np.zeros_like(gz)
    return fam.axpby(v, zero, np.conj(gz), 'map'), fam.axpby(u, zero, gz, 'map')


def binned_cross_jvp(fam, u, v, du, dv):
    return fam.cross(du, v) + fam.cross(u, dv)


def binned_rot_vjp(fam, x, theta, gy):
    gx = fam.rot(gy, -np.asarray(theta))
    return gx, 0.5 * fam.cross(gx, x).imag


def binned_rot_jvp(fam, x, theta, dx, dtheta):
    dtheta = np.asarray(dtheta)
    return fam.rot(dx, theta) + fam.axpby(fam.rot(x, theta), np.zeros_like(dtheta), -0.5j * dtheta, 'map')
