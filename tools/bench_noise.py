"""Noise layers on state vectors on the MI355X (dq_apply_jump_*, dq_jump_cross_*), every group
timed in one process with its yardstick, taking turns.

1. Kernels, complex64 n = 28 and complex128 n = 27 at batch 4.  ``jump_apply`` against ``apply_diag`` with a full-width
   table on the same state -- equal bytes (the state read and written; the diagonal also streams its table, which is
   charged to it), so the ratio is what the factor path costs: a Pauli-only layer, a damping layer without zeros, a jump
   (an exact zero and a flip) on the top and on the bottom wire.  ``jump_cross`` against ``cost_cross`` (full width).
2. A depolarizing and an amplitude-damping layer on all n wires end to end, sampler included
   (``qmath.apply_noise_layer``), against a loop over the wires of ``backend.marginal`` plus a per-sample 2x2
   ``backend.apply_gate`` -- the route ``Reset`` takes -- with the Kraus operator drawn from the marginal.
3. One noisy QAOA step at n = 14 (cost phase, mixer, depolarizing layer) as 256 trajectories against the same circuit
   with ``den_mat=True``.

Every point: one warm-up call, then the median of ``reps`` calls between device events.  The box is recorded first.

usage: python tools/bench_noise.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend, channel, qmath  # noqa: E402
from bench_diag import row, timed_group  # noqa: E402


def records(n, batch):
    """name -> (factors, xmask, phase, scale) on the device."""
    g = torch.Generator().manual_seed(n)
    one = torch.ones(batch, n, 2, dtype=torch.float64)
    zero = torch.zeros(batch, dtype=torch.int64)
    s = torch.ones(batch, dtype=torch.float64)
    z = torch.randint(0, 1 << n, (batch,), generator=g)
    x = torch.randint(0, 1 << n, (batch,), generator=g)
    pauli = one.clone()
    for p in range(n):
        pauli[:, p, 1] = 1.0 - 2.0 * ((z >> p) & 1)
    damp = 0.5 + 0.5 * torch.rand(batch, n, 2, dtype=torch.float64, generator=g)
    out = {'pauli layer': (pauli, x, torch.tensor([bin(int(v)).count('1') % 4 for v in x & z]), s),
           'damping layer': (damp, zero, zero, s * 1.25)}
    for where, p in (('top', n - 1), ('bottom', 0)):
        jump = damp.clone()
        jump[:, p, 0] = 0.0
        out[f'jump on the {where} wire'] = (jump, zero + (1 << p), zero, s * 1.25)
    return {k: tuple(t.cuda() for t in v) for k, v in out.items()}


def kernels(rows, dtype, n, batch, reps):
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    esz = 8 if dtype == torch.complex64 else 16
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    out = torch.empty_like(psi)
    sbytes = psi.numel() * esz
    full = list(range(n - 1, -1, -1))
    diag = torch.exp(1j * torch.randn(1 << n, dtype=torch.float64, device='cuda')).to(dtype)
    cost = torch.randn(1 << n, dtype=real, device='cuda')
    recs = records(n, batch)
    yard = 'apply_diag full width (yardstick)'
    group = {yard: lambda: backend.apply_diag(psi, diag, full, out=out)}
    for name, (f, x, m, s) in recs.items():
        group[f'jump_apply {name}'] = (lambda f=f, x=x, m=m, s=s: backend.jump_apply(psi, f, x, m, s, out=out))
    with torch.no_grad():
        ts = timed_group(group, reps)
    base = row(rows, yard, dtype, n, batch, ts[yard], 2 * sbytes + diag.numel() * esz)
    for name in recs:
        row(rows, f'jump_apply {name}', dtype, n, batch, ts[f'jump_apply {name}'], 2 * sbytes, base)
    other = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    weights = recs['damping layer'][0] ** 2
    for tag, bra, reads in (('weight', psi, 1), ('cross', other, 2)):
        yard = f'cost_cross {tag} (yardstick)'
        ts = timed_group({yard: lambda bra=bra: backend.cost_cross(bra, psi, cost, full),
                          'new': lambda bra=bra: backend.jump_cross(bra, psi, weights)}, reps)
        base = row(rows, yard, dtype, n, batch, ts[yard], reads * sbytes + cost.numel() * (esz // 2))
        row(rows, f'jump_cross {tag}', dtype, n, batch, ts['new'], reads * sbytes, base)
    del psi, other, out, diag, cost
    torch.cuda.empty_cache()


def per_wire_route(psi, n, stacks, gen):
    """A trajectory step wire by wire: the marginal of the wire, the Kraus operator drawn per sample from
    sum_c |K_j|c>|^2 P(c), a per-sample 2x2 gate, renormalised by the next marginal."""
    for w, k in enumerate(stacks):
        bit = n - 1 - w
        pm = backend.marginal(psi, [bit])                                     # (B, 2)
        col = (k.abs() ** 2).sum(-2).to(torch.float64)                        # (J, 2): |K_j |c>|^2
        pj = pm @ col.T                                                       # (B, J)
        j = torch.multinomial(pj.clamp_min(0), 1, generator=gen)[:, 0]
        mats = k[j] / torch.gather(pj, 1, j[:, None]).sqrt()[:, :, None]
        psi = backend.apply_gate(psi, mats.to(psi.dtype), [bit])
    return psi


def end_to_end(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    gen = torch.Generator('cuda').manual_seed(1)
    theta = torch.tensor([0.3], dtype=torch.float64)
    for name, cls in (('depolarizing', channel.Depolarizing), ('amp_damp', channel.AmplitudeDamping)):
        k = cls(inputs=theta).get_matrix(theta).reshape(-1, 2, 2)
        tables = qmath.noise_tables(n, [(w, k) for w in range(n)], 'cuda')
        stacks = [k.cuda()] * n
        with torch.no_grad():
            ts = timed_group({'old': lambda: per_wire_route(psi, n, stacks, gen),
                              'new': lambda: qmath._noise_flat(psi, n, tables, None, gen)}, reps)
        base = row(rows, f'{name} on {n} wires, wire by wire', dtype, n, batch, ts['old'], 3 * n * psi.numel() * esz)
        row(rows, f'{name} on {n} wires, noise layer', dtype, n, batch, ts['new'], 4 * psi.numel() * esz, base)
    del psi
    torch.cuda.empty_cache()


def qaoa_step(rows, n, traj, reps):
    def build(den_mat):
        cir = dq.QubitCircuit(n, den_mat=den_mat)
        cir.hlayer()
        for w in range(n):
            cir.rzz([w, (w + 1) % n], 0.4)
        for w in range(n):
            cir.rx(w, 0.3)
        if den_mat:
            for w in range(n):
                cir.depolarizing(w, 0.2)
        else:
            cir.noise_layer('depolarizing', 0.2, generator=torch.Generator('cuda').manual_seed(2))
        return cir.to('cuda')

    dm, sv = build(True), build(False)
    state = sv.init_state.state.expand(traj, -1, -1)
    with torch.no_grad():
        ts = timed_group({'dm': lambda: dm(), 'sv': lambda: sv(state=state)}, reps)
    base = row(rows, f'QAOA step n={n}, den_mat=True', torch.complex64, n, 1, ts['dm'], 2 * 8 << (2 * n))
    row(rows, f'QAOA step n={n}, {traj} trajectories', torch.complex64, n, traj, ts['sv'], 2 * 8 * traj << n, base)


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_noise.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    rows = []
    reps = 5 if quick else 11
    points = ((torch.complex64, 22, 4), (torch.complex128, 21, 4)) if quick else ((torch.complex64, 28, 4), (torch.complex128, 27, 4))
    for dtype, n, batch in points:
        kernels(rows, dtype, n, batch, reps)
    for dtype, n, batch in points:
        end_to_end(rows, dtype, n, batch, 3 if quick else 5)
    qaoa_step(rows, 10 if quick else 14, 256, reps)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
