"""complex128 torch references of the binned cost reduction and its cotangent on the CPU, from the definitions

    sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j),      on(i) = all control bits of i are 1

shared by test_hist_gpu.py, test_hist_autograd_gpu.py and test_costdist_cpu.py."""

import torch


def sub_index(n, bits, controls=()):
    i = torch.arange(1 << n)
    sub = torch.zeros_like(i)
    for j, p in enumerate(bits):
        sub |= ((i >> p) & 1) << (len(bits) - 1 - j)
    cm = sum(1 << c for c in controls)
    return sub, (i & cm) == cm


def hist_ref(bra, ket, bins, nbins, n, bits, controls=()):
    """out[b, v] = sum over on(i), bins[sub(i)] = v of conj(bra) ket, and the same sum of the terms' magnitudes."""
    sub, on = sub_index(n, bits, controls)
    terms = on * bra.to(torch.complex128).conj() * ket.to(torch.complex128)
    index = bins.to(torch.int64)[sub]
    out = torch.zeros(ket.shape[0], nbins, dtype=torch.complex128).index_add_(1, index, terms)
    return out, torch.zeros(ket.shape[0], nbins, dtype=torch.float64).index_add_(1, index, terms.abs())


def binned_ref(x, g, bins, n, bits, controls=()):
    """g[b, bins[sub(i)]] x[b, i] inside the controls, 0 elsewhere."""
    sub, on = sub_index(n, bits, controls)
    return on * g.to(torch.complex128)[:, bins.to(torch.int64)[sub]] * x.to(torch.complex128)
