"""The goldens of the reciprocal-space kernel function, ``tests/golden/ewald_pointwise.npz`` (mpmath, written by
``tests/golden/make_ewald_pointwise_golden.py``), against themselves and against numpy float64.  No GPU.

    f_p(z) = Gamma(a, z) / z^a,  a = (3 - p)/2,  z = sigma^2 k^2 / 2;     G = c0 f_p,  dG/dk^2 = c0 sigma^2/2 f_p'

  * the two identities of the derivative, f_p' = -f_{p-2} (p = 3..6, between stored columns) and f_p' = -(exp(-z) + a f_p)/z;
  * ``closed_forms``: the closed forms of integer p with f_p' = -(exp(-z) + a f_p)/z, which is what csrc/kpot.h evaluated for every
    z until the pointwise test of the device function (tests/test_gpu_ewald_pointwise.py).  For p >= 4 they are differences:
        f_4 cancels to order 2z, f_6 to 4z^2 as z grows, each on top of the z eps by which the rounding of sqrt(z) moves erfc;
        the derivative's sum is a difference of order sqrt(pi z) (p = 4), z ln(1/z) (p = 5), 2z (p = 6) as z -> 0.
    ``closed_form_tolerance`` states that loss; the test holds the forms to it, and shows that they miss the pointwise bound of the
    project (2e-14 + 2^-51 z) by the factors its docstring gives, so that nobody takes them for good again;
  * ``kpot_emulation``: what csrc/kpot.h evaluates now -- the closed forms up to z = 1, Legendre's continued fraction beyond, and
    f_p' = -f_{p-2} for p >= 4 -- which holds the pointwise bound everywhere.
"""

import os

import numpy as np
import pytest
from scipy.special import erfc, exp1, gamma

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXPONENTS = range(1, 7)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "ewald_pointwise.npz"))


def pointwise_bound(z):
    """The fp64 pointwise bound of the project, relative: 2e-14 and the rounding of z itself (which moves exp(-z) by z eps)."""
    return 2e-14 + 2.0**-51 * np.asarray(z, np.float64)


def closed_forms(p, z):
    """(f_p, f_p') at z > 0: the closed forms of integer p, and the derivative from -(exp(-z) + a f_p)/z."""
    z = np.asarray(z, np.float64)
    ez, rz = np.exp(-z), np.sqrt(z)
    f = {1: lambda: ez / z,
         2: lambda: np.sqrt(np.pi / z) * erfc(rz),
         3: lambda: exp1(z),
         4: lambda: 2.0 * (ez - np.sqrt(np.pi * z) * erfc(rz)),
         5: lambda: ez - z * exp1(z),
         6: lambda: ((2.0 - 4.0 * z) * ez + 4.0 * np.sqrt(np.pi * z * z * z) * erfc(rz)) / 3.0}[p]()
    return f, -(ez + 0.5 * (3 - p) * f) / z


def closed_form_tolerance(p, z):
    """Relative tolerances (of f_p, of f_p') of ``closed_forms``: the pointwise bound plus what the differences lose (module
    docstring): the cancellation factor times 4 eps, eps = 2^-52, for the roundings it magnifies (sqrt(z) and its product, and an
    erfc or E1 that is itself good to an ulp or two)."""
    z = np.asarray(z, np.float64)
    b, eps = pointwise_bound(z), 2.0**-52
    tf = b + {4: 4 * eps * z**2, 6: 4 * eps * z**3}.get(p, 0.0)
    tdf = b + {4: 2 * eps / np.sqrt(z) + 4 * eps * z, 5: 2 * eps / z, 6: 4 * eps / z + 4 * eps * z**2}.get(p, 0.0)
    return tf, tdf


def _cf(a, z):
    """exp(-z) / (z + (1-a)/(1 + 1/(z + (2-a)/(1 + 2/(z + ...))))) by backward recurrence, 20 + 80/z levels (csrc/kpot.h)."""
    out = np.empty_like(z)
    for i, zz in enumerate(z):
        t = 0.0
        for k in range(20 + int(80.0 / zz), 0, -1):
            t = (k - a) / (1.0 + k / (zz + t))
        out[i] = np.exp(-zz) / (zz + t)
    return out


def kpot_emulation(p, z):
    """(f_p, f_p') as lr_kernel_dev of csrc/kpot.h forms them, in numpy float64 (scipy's erfc and E1 for the device's)."""
    z = np.asarray(z, np.float64)
    f, df = closed_forms(p, z)
    if p < 4:
        return f, df
    big = z > 1.0
    f = f.copy()
    f[big] = _cf(0.5 * (3 - p), z[big])
    return f, -kpot_emulation(p - 2, z)[0]


def _columns(g, p, i):
    """z > 0 of sigma i and the four stored columns there."""
    z = g[f"z_s{i}"]
    keep = z > 0
    return (z[keep],) + tuple(g[f"{k}_p{p}_s{i}"][keep] for k in ("f", "df", "G", "dG"))


def _normal(ref):
    return np.abs(ref) > 2.0**-1016  # the float64 underflow class of the GPU test is left to the GPU test


def test_grid(g):
    """The grid is the one the generator documents: kappa is float32 and ascending from 0, z is formed from it with the double
    operations of make_kpot, both sides of z = 1 are within one float32 step of kappa, the decades and the end of exp's range are
    there, and the stored underflow counts are those of the stored columns."""
    assert list(g["sigmas"]) == [0.5, 1.0, 2.5]
    for i, sigma in enumerate(g["sigmas"]):
        kappa, z = g[f"kappa_s{i}"], g[f"z_s{i}"]
        assert kappa.dtype == np.float32 and kappa[0] == 0 and np.all(np.diff(kappa) > 0)
        k = kappa.astype(np.float64)
        assert np.array_equal(z, (0.5 * sigma * sigma) * (k * k))
        near = z[np.abs(z - 1.0) < 1e-6]
        assert (near < 1).sum() >= 2 and (near > 1).sum() >= 2
        for e in range(-12, 0):
            assert np.abs(z / 10.0**e - 1).min() < 1e-6
        assert ((z > 0.1) & (z < 60)).sum() >= 200 and z.max() > 746 and ((z > 700) & (z < 745)).any()
        for p in EXPONENTS:
            for j, name in enumerate(("G", "dG")):
                mag = np.abs(g[f"{name}_p{p}_s{i}"][z > 0])
                assert g["under32"][p - 1, i, j] == (mag < 2.0**-120).sum()
                assert g["under64"][p - 1, i, j] == (mag < 2.0**-1016).sum()
            # k = 0: the value the library defines there, and no derivative
            a = 0.5 * (3 - p)
            assert g[f"f_p{p}_s{i}"][0] == (-1 / a if p > 3 else 0.0) and g[f"df_p{p}_s{i}"][0] == 0.0 == g[f"dG_p{p}_s{i}"][0]


def test_prefactor(g):
    """G = c0 f and dG = c0 sigma^2/2 f' with c0 = pi^1.5 / Gamma(p/2) (2 sigma^2)^a in numpy, to 1e-14."""
    for i, sigma in enumerate(g["sigmas"]):
        for p in EXPONENTS:
            z, f, df, G, dG = _columns(g, p, i)
            c0 = np.pi**1.5 / gamma(0.5 * p) * (2 * sigma * sigma) ** (0.5 * (3 - p))
            ok = _normal(G) & _normal(f) & _normal(dG) & _normal(df)
            assert ok.sum() >= len(z) - 8
            G, dG, f, df = G[ok], dG[ok], f[ok], df[ok]
            assert np.abs(G / (c0 * f) - 1).max() < 1e-14
            assert np.abs(dG / (c0 * 0.5 * sigma * sigma * df) - 1).max() < 1e-14


def test_derivative_identities(g):
    """f_p' = -f_{p-2} between the stored columns (p = 3..6), and f_p' = -(exp(-z) + a f_p)/z, both to 1e-13.  The second is a
    difference for p >= 4 that float64 columns cannot resolve at small z, so with mpmath it is evaluated at 50 digits from f_p
    recomputed there; without mpmath, from the stored columns against the size of its terms."""
    try:
        import mpmath as mp
    except ImportError:
        mp = None
    for i in range(3):
        for p in EXPONENTS:
            z, f, df, _, _ = _columns(g, p, i)
            ok = _normal(df)
            if p >= 3:
                lower = g[f"f_p{p - 2}_s{i}"][g[f"z_s{i}"] > 0]
                assert np.abs(df[ok] / -lower[ok] - 1).max() < 1e-13, (p, i)
            a = 0.5 * (3 - p)
            if mp is None:
                rhs, size = -(np.exp(-z) + a * f) / z, (np.exp(-z) + abs(a) * np.abs(f)) / z
                assert (np.abs(df - rhs)[ok] / size[ok]).max() < 1e-13, (p, i)
                continue
            mp.mp.dps = 50
            for zz, d in zip(z[ok][::4], df[ok][::4]):
                x = mp.mpf(float(zz))
                rhs = -(mp.e ** (-x) + a * mp.gammainc(a, x) / x**a) / x
                assert abs(mp.mpf(float(d)) / rhs - 1) < 1e-13, (p, i, zz)


def test_recomputed_sample(g):
    """Every seventh point again from mpmath, at 50 digits rather than the generator's 60: the file is the generator's output."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    for i, sigma in enumerate(g["sigmas"]):
        s = mp.mpf(float(sigma))
        for p in EXPONENTS:
            z, f, df, G, dG = _columns(g, p, i)
            a = mp.mpf(3 - p) / 2
            c0 = mp.pi ** (mp.mpf(3) / 2) / mp.gamma(mp.mpf(p) / 2) * (2 * s * s) ** a
            for j in range(p % 7, len(z), 7):
                x = mp.mpf(float(z[j]))
                fr = mp.gammainc(a, x) / x**a
                dfr = -mp.gammainc(a + 1, x) / x ** (a + 1)
                for got, ref in ((f[j], fr), (df[j], dfr), (G[j], c0 * fr), (dG[j], c0 * s * s / 2 * dfr)):
                    assert got == float(ref), (p, i, z[j], got, float(ref))


# what the closed forms miss the pointwise bound by, at least (measured: the test prints the figures), per (p, quantity)
_CLOSED_FORMS_MISS = {(4, "f"): 100.0, (6, "f"): 1e4, (4, "df"): 100.0, (5, "df"): 1e5, (6, "df"): 1e8}


@pytest.mark.parametrize("p", EXPONENTS)
def test_closed_forms(g, p):
    """``closed_forms`` within ``closed_form_tolerance`` of the goldens for z < 700; for p <= 3 and for f_5 that is the pointwise
    bound itself, for the rest the test also asserts that the pointwise bound is missed (``_CLOSED_FORMS_MISS``), largest at the ends
    of the grid: f_4 481 x and f_6 2e5 x at z = 700, f_4' 676 x, f_5' 6e6 x, f_6' 2e9 x at z = 1e-12."""
    worst = {"f": 0.0, "df": 0.0}
    for i in range(3):
        z, f, df, _, _ = _columns(g, p, i)
        keep = z < 700  # beyond, exp(-z) is about to leave the normal range
        z = z[keep]
        got_f, got_df = closed_forms(p, z)
        tf, tdf = closed_form_tolerance(p, z)
        for key, got, ref, tol in (("f", got_f, f[keep], tf), ("df", got_df, df[keep], tdf)):
            err = np.abs(got / ref - 1)
            j = (err / tol).argmax()
            print(f"[ewald-pointwise-host] closed form p={p} {key:2s} sigma {g['sigmas'][i]}: max err/tolerance {(err / tol)[j]:.3f} at "
                  f"z = {z[j]:.3g}; max err/pointwise bound {(err / pointwise_bound(z)).max():.3g}")
            assert (err <= tol).all(), (p, key, z[j], err[j], tol[j])
            worst[key] = max(worst[key], (err / pointwise_bound(z)).max())
    for key in ("f", "df"):
        if (p, key) in _CLOSED_FORMS_MISS:
            assert worst[key] > _CLOSED_FORMS_MISS[(p, key)], (p, key, worst[key])
        else:
            assert worst[key] <= 1.0


@pytest.mark.parametrize("p", EXPONENTS)
def test_kpot_emulation(g, p):
    """``kpot_emulation`` within the pointwise bound of the goldens, both quantities, every point of normal size."""
    for i in range(3):
        z, f, df, _, _ = _columns(g, p, i)
        keep = z < 700
        z = z[keep]
        for key, got, ref in zip(("f", "df"), kpot_emulation(p, z), (f[keep], df[keep])):
            ratio = np.abs(got / ref - 1) / pointwise_bound(z)
            print(f"[ewald-pointwise-host] kpot.h form p={p} {key:2s} sigma {g['sigmas'][i]}: max err/bound {ratio.max():.3f} at "
                  f"z = {z[ratio.argmax()]:.3g}")
            assert ratio.max() <= 1.0, (p, key, z[ratio.argmax()], ratio.max())
