#!/usr/bin/env python3
"""Chebyshev coefficients of the exponentially scaled Bessel functions in amico_amd/csrc/amx_debias.hip.

    z in [0, 8]  :  I0e(z) = sum' a0_k T_k(z/4 - 1)              I1e(z) = z * sum' a1_k T_k(z/4 - 1)
    z in [8, oo) :  I0e(z) = sum' b0_k T_k(16/z - 1) / sqrt(z)   I1e(z) = sum' b1_k T_k(16/z - 1) / sqrt(z)

(sum': the k = 0 term is halved).  The coefficients are the Chebyshev interpolants at 96 nodes of the functions
evaluated by mpmath at 50 digits, cut where they fall below 2e-18 of the first one (kA1 gets a trailing 0.0 so that
both small-argument series share one loop).  Run it to print the four tables exactly as they stand in the kernel source
and the largest relative error of each fit on a dense grid (evaluated in float64 by the same Clenshaw recurrence the
kernel uses).  Needs mpmath (the tables are made on first use, ~6 s); tests/test_debias.py compares the kernel's tables
with them.
"""
import functools

import numpy as np

N = 96


def cheb(f):
    import mpmath as mp
    ys = [mp.cos(mp.pi * (2 * j + 1) / (2 * N)) for j in range(N)]
    fs = [f(y) for y in ys]
    c = [2 * mp.fsum(fs[j] * mp.cos(mp.pi * k * (2 * j + 1) / (2 * N)) for j in range(N)) / N for k in range(N)]
    n = max(k for k in range(N) if abs(c[k]) > mp.mpf('2e-18') * abs(c[0])) + 1
    return [float(v) for v in c[:n]]


def ive(n, z):
    import mpmath as mp
    return mp.besseli(n, z) * mp.exp(-z)


@functools.lru_cache(maxsize=None)
def _tables():
    import mpmath as mp
    mp.mp.dps = 50
    t = {
        'kA0': cheb(lambda y: ive(0, 4 * (y + 1))),
        'kA1': cheb(lambda y: ive(1, 4 * (y + 1)) / (4 * (y + 1))),
        'kB0': cheb(lambda y: mp.sqrt(16 / (y + 1)) * ive(0, 16 / (y + 1))),
        'kB1': cheb(lambda y: mp.sqrt(16 / (y + 1)) * ive(1, 16 / (y + 1))),
    }
    t['kA1'] += [0.0] * (len(t['kA0']) - len(t['kA1']))
    return t


def tables():
    """the four coefficient lists as the kernel holds them"""
    return {k: list(v) for k, v in _tables().items()}


def source_text(t=None):
    """the tables as they stand in amx_debias.hip"""
    out = []
    for name, c in (t or tables()).items():
        out.append(f'__constant__ double {name}[{len(c)}] = {{')
        for i in range(0, len(c), 3):
            out.append('    ' + ' '.join(f'{v!r},' for v in c[i:i + 3]))
        out.append('};')
    return '\n'.join(out) + '\n'


def clenshaw(c, y):
    b1 = np.zeros_like(y)
    b2 = np.zeros_like(y)
    for k in range(len(c) - 1, 0, -1):
        b1, b2 = c[k] + 2.0 * y * b1 - b2, b1
    return 0.5 * c[0] + y * b1 - b2


def ive_f64(z, t=None):
    """(I0e, I1e) the way the kernel evaluates them, from the tables `t` (default: the generated ones)"""
    TABLES = t or tables()
    z = np.asarray(z, dtype=np.float64)
    small = z <= 8.0
    ya = np.where(small, z / 4.0 - 1.0, 0.0)
    yb = np.where(small, 0.0, 16.0 / np.where(small, 8.0, z) - 1.0)
    rs = 1.0 / np.sqrt(np.where(small, 1.0, z))
    i0 = np.where(small, clenshaw(TABLES['kA0'], ya), clenshaw(TABLES['kB0'], yb) * rs)
    i1 = np.where(small, z * clenshaw(TABLES['kA1'], ya), clenshaw(TABLES['kB1'], yb) * rs)
    return i0, i1


if __name__ == '__main__':
    import mpmath as mp
    print(source_text(), end='')
    zs = np.concatenate([np.linspace(0.0, 8.0, 4001)[1:], np.geomspace(8.0, 1e9, 4000)])
    i0, i1 = ive_f64(zs)
    e0 = max(abs(mp.mpf(float(a)) / ive(0, mp.mpf(float(z))) - 1) for a, z in zip(i0, zs))
    e1 = max(abs(mp.mpf(float(a)) / ive(1, mp.mpf(float(z))) - 1) for a, z in zip(i1, zs))
    print(f'// largest relative error on {len(zs)} points of (0, 1e9]: I0e {float(e0):.2e}, I1e {float(e1):.2e}')
