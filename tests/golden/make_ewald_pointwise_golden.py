"""Generate tests/golden/ewald_pointwise.npz: the reciprocal-space kernel function of the range-separated 1/r^p potentials,

    f_p(z) = Gamma(a, z) / z^a,   a = (3 - p)/2,   z = sigma^2 k^2 / 2,          G(k) = c0 f_p(z),   dG/dk^2 = c0 sigma^2/2 f_p'(z),
    c0 = pi^(3/2) / Gamma(p/2) (2 sigma^2)^a                                       (prefactor 1)

point by point from mpmath at 60 digits (the upper incomplete gamma function itself, ``mpmath.gammainc``; no closed form and nothing
of csrc/kpot.h is restated here).

    python tests/golden/make_ewald_pointwise_golden.py

Every reference value is taken at the number the kernel under test really receives.  The test passes k-vectors (kappa, 0, 0) with
kappa a float32 number, so both precisions read the same input and kappa^2 is exact in double; z is formed here with the double
operations of ``make_kpot`` / ``lr_kernel_dev``: z = ((0.5 sigma) sigma) (kappa kappa).

Contents
  sigmas                   the three smearings
  kappa_s<i>               float32 kappa for sigma i, ascending; kappa = 0 first
  z_s<i>                   float64 z at kappa_s<i>: 0; the decades 1e-12 .. 1e-1; 200 points spread over (0.1, 60) in log z; z = 1
                           bracketed (the float32 kappa nearest to z = 1 and two float32 neighbours on either side: exp1_dev leaves
                           its series for the continued fraction there); 80 .. 750, past the point where exp(-z) leaves the double
                           range (~745)
  f_p<p>_s<i>, df_*        f_p and f_p' = -(exp(-z) + a f_p)/z at z_s<i>, p = 1..6; at z = 0: f = -1/a for p > 3, else 0 (the value
                           the library defines at k = 0), and f' = 0
  G_p<p>_s<i>, dG_*        c0 f_p and c0 sigma^2/2 f_p' (c0 from mpmath as well)
  under32, under64         (6, 3, 2) integers: the number of points of G and of dG per (p, sigma) whose reference lies in the float32 /
                           float64 underflow class of ``check`` (tests/test_gpu_dipole_pointwise.py): |reference| < 2^-120 / 2^-1016
"""

import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 60

SIGMAS = (0.5, 1.0, 2.5)
EXPONENTS = range(1, 7)


def half_sigma_sq(sigma):
    return 0.5 * sigma * sigma  # make_kpot: 0.5 * smearing * smearing


def z_of(sigma, kappa32):
    k = np.asarray(kappa32, np.float32).astype(np.float64)
    return half_sigma_sq(sigma) * (k * k)


def kappa_grid(sigma):
    hs2 = half_sigma_sq(sigma)
    targets = [10.0**e for e in range(-12, 0)]
    targets += list(np.exp(np.linspace(np.log(0.1), np.log(60.0), 202))[1:-1])
    targets += [60.0, 80.0, 100.0, 200.0, 400.0, 700.0, 740.0, 744.0, 745.0, 746.0, 750.0]
    kappa = [np.float32(np.sqrt(t / hs2)) for t in targets]
    one = np.float32(np.sqrt(1.0 / hs2))
    lo1, hi1 = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(1e9))
    kappa += [np.nextafter(lo1, np.float32(0)), lo1, one, hi1, np.nextafter(hi1, np.float32(1e9)), np.float32(0)]
    kappa = np.unique(np.asarray(kappa, np.float32))
    z = z_of(sigma, kappa)
    near = z[np.abs(z - 1.0) < 1e-6]
    assert (near < 1.0).any() and (near > 1.0).any(), near
    return kappa, z


def f_and_derivative(p, z):
    """f_p and f_p' at the double z, read exactly."""
    a = mp.mpf(3 - p) / 2
    if z == 0.0:
        return (-1 / a if p > 3 else mp.mpf(0)), mp.mpf(0)
    z = mp.mpf(float(z))
    f = mp.gammainc(a, z) / z**a
    return f, -(mp.e ** (-z) + a * f) / z


def c0(p, sigma):
    s = mp.mpf(sigma)
    return mp.pi ** (mp.mpf(3) / 2) / mp.gamma(mp.mpf(p) / 2) * (2 * s * s) ** (mp.mpf(3 - p) / 2)


def main():
    out = {"sigmas": np.array(SIGMAS)}
    under32 = np.zeros((6, len(SIGMAS), 2), np.int64)
    under64 = np.zeros_like(under32)
    for i, sigma in enumerate(SIGMAS):
        kappa, z = kappa_grid(sigma)
        out[f"kappa_s{i}"], out[f"z_s{i}"] = kappa, z
        for p in EXPONENTS:
            ref = [f_and_derivative(p, t) for t in z]
            c, s = c0(p, sigma), mp.mpf(sigma)
            cols = {"f": [r[0] for r in ref], "df": [r[1] for r in ref], "G": [c * r[0] for r in ref],
                    "dG": [c * s * s / 2 * r[1] for r in ref]}
            for name, col in cols.items():
                out[f"{name}_p{p}_s{i}"] = np.array([float(v) for v in col])
            for j, name in enumerate(("G", "dG")):
                # the class of `check`: the scale |reference| below 2^-120 / 2^-1016; the points at k = 0 are asserted exactly instead
                mag = np.abs(out[f"{name}_p{p}_s{i}"])[z > 0]
                under32[p - 1, i, j] = int((mag < 2.0**-120).sum())
                under64[p - 1, i, j] = int((mag < 2.0**-1016).sum())
        print(f"sigma {sigma}: {len(z)} points, z = {z[1]:.3e} .. {z[-1]:.1f}; float32 underflow class per p (G, dG): "
              f"{under32[:, i].tolist()}, float64: {under64[:, i].tolist()}")
    out["under32"], out["under64"] = under32, under64
    path = os.path.join(HERE, "ewald_pointwise.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes")
    assert size < 300_000


if __name__ == "__main__":
    main()
