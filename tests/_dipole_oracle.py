"""NumPy restatement of the point-dipole calculator (``CalculatorDipole``), written from its formulas; float64 throughout.

Real space, pair p = (i, j), r = neighbor vector:  T(r) = prefactor (B I - C r r^T), V_i += T mu_j / 2 (half list: also
V_j += T mu_i / 2), with B, C the bare, short-range (erfc) or exclusion-switched long-range (erf) coefficients.
Reciprocal space:  V_i = [ sum_k G(k) k (cos(k r_i) S_c(k) + sin(k r_i) S_s(k)) / V - self mu_i + bg sum_j mu_j ] / 2,
S_c(k) = sum_j (mu_j . k) cos(k r_j), G(k) = prefactor 4 pi exp(-sigma^2 k^2 / 2) / k^2, G(0) = 0.
"""

from __future__ import annotations

import math

import numpy as np
from scipy.special import erf, erfc


def _coefficients(r, smearing, exclusion_radius, exclusion_degree):
    if smearing is None:
        return 1.0 / r**3, 3.0 / r**5
    alpha = 0.5 / smearing**2
    y = math.sqrt(alpha) * r
    ke = 2.0 * math.sqrt(alpha / math.pi) * np.exp(-alpha * r * r)
    if exclusion_radius is None:
        w, k = erfc(y), ke
    else:
        w, k = erf(y), -ke
    B = w / r**3 + k / r**2
    C = 3.0 * w / r**5 + k * (2.0 * alpha + 3.0 / r**2) / r**2
    if exclusion_radius is not None:
        h = 0.5 * (1.0 - np.cos(math.pi * r / exclusion_radius))
        fc = np.where(r < exclusion_radius, 1.0 - h**exclusion_degree, 0.0)
        B, C = -fc * B, -fc * C
    return B, C


def rspace(mu, pairs, vectors, smearing=None, exclusion_radius=None, exclusion_degree=1, prefactor=1.0, full=False):
    mu = np.asarray(mu, dtype=np.float64)
    out = np.zeros_like(mu)
    if len(pairs) == 0:
        return out
    v = np.asarray(vectors, dtype=np.float64)
    i, j = pairs[:, 0], pairs[:, 1]
    r = np.linalg.norm(v, axis=1)
    B, C = _coefficients(r, smearing, exclusion_radius, exclusion_degree)

    def apply(m):
        return prefactor * (B[:, None] * m - (C * np.sum(v * m, axis=1))[:, None] * v)

    np.add.at(out, i, apply(mu[j]))
    if not full:
        np.add.at(out, j, apply(mu[i]))
    return out / 2


def kvectors(cell, lr_wavelength):
    cell = np.asarray(cell, dtype=np.float64)
    ns = np.ceil(np.linalg.norm(cell, axis=1) / lr_wavelength).astype(np.int64)
    f = [np.fft.fftfreq(int(n)) * int(n) for n in ns]
    F = np.stack(np.meshgrid(*f, indexing="ij"), axis=-1).reshape(-1, 3)
    return 2.0 * math.pi * F @ np.linalg.inv(cell).T


def _G(k, smearing, prefactor):
    k2 = np.sum(k * k, axis=1)
    safe = np.where(k2 == 0, 1.0, k2)
    return np.where(k2 == 0, 0.0, prefactor * 4.0 * math.pi * np.exp(-0.5 * smearing**2 * safe) / safe)


def _chunks(K, N, budget=4_000_000):
    step = max(1, budget // max(N, 1))
    return [slice(a, min(K, a + step)) for a in range(0, K, step)]


def kspace(mu, positions, cell, smearing, lr_wavelength, prefactor=1.0, epsilon=0.0, grad_out=None):
    """The reciprocal-space part (N,3); with ``grad_out`` also the gradients of <grad_out, V> w.r.t. dipoles and positions."""
    mu = np.asarray(mu, dtype=np.float64)
    pos = np.asarray(positions, dtype=np.float64)
    k = kvectors(cell, lr_wavelength)
    G = _G(k, smearing, prefactor)
    vol = abs(np.linalg.det(np.asarray(cell, dtype=np.float64)))
    N = len(pos)
    field = np.zeros((N, 3))
    gmu = np.zeros((N, 3))
    gpos = np.zeros((N, 3))
    g = None if grad_out is None else np.asarray(grad_out, dtype=np.float64)
    for sl in _chunks(len(k), N):
        kk, GG = k[sl], G[sl]
        ph = kk @ pos.T  # (k, N)
        c, s = np.cos(ph), np.sin(ph)
        q = kk @ mu.T
        Sc, Ss = np.sum(q * c, axis=1), np.sum(q * s, axis=1)
        field += (c * (GG * Sc)[:, None] + s * (GG * Ss)[:, None]).T @ kk
        if g is not None:
            qg = kk @ g.T
            Tc, Ts = np.sum(qg * c, axis=1), np.sum(qg * s, axis=1)
            gmu += (c * (GG * Tc)[:, None] + s * (GG * Ts)[:, None]).T @ kk
            b = qg * (c * Ss[:, None] - s * Sc[:, None]) + q * (c * Ts[:, None] - s * Tc[:, None])
            gpos += (b * GG[:, None]).T @ kk
    alpha = 0.5 / smearing**2
    self_c = prefactor * 4.0 * math.pi / 3.0 * (alpha / math.pi) ** 1.5
    V = field / vol - self_c * mu
    if epsilon != 0.0:
        V = V + prefactor * 4.0 * math.pi / (2.0 * epsilon + 1.0) / vol * mu.sum(axis=0)
    if g is None:
        return V / 2
    gmu = gmu / vol - self_c * g
    if epsilon != 0.0:
        gmu = gmu + prefactor * 4.0 * math.pi / (2.0 * epsilon + 1.0) / vol * g.sum(axis=0)
    return V / 2, gmu / 2, gpos / vol / 2


def potential(mu, positions, cell, pairs, vectors, smearing=None, lr_wavelength=None, exclusion_radius=None,
              exclusion_degree=1, epsilon=0.0, prefactor=1.0, full=False):
    V = rspace(mu, pairs, vectors, smearing, exclusion_radius, exclusion_degree, prefactor, full)
    if smearing is None:
        return V
    return V + kspace(mu, positions, cell, smearing, lr_wavelength, prefactor, epsilon)
