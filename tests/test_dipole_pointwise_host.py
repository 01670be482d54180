"""The radial functions of the dipolar pair tensor in plain numpy float64 (``radial_closed_form``), against the mpmath goldens of
``tests/golden/dipole_pointwise.npz`` (written by ``tests/golden/make_dipole_pointwise_golden.py``).  No GPU.

``radial_closed_form`` is the reference of the GPU tests wherever they leave the golden points (random directions, stars, the
grid-stride case).  It is written to hold 1e-13 over the whole range of the goldens:

  * mode 1 (short range) as erfcx(y) exp(-x): the exponential's argument x = r^2 / 2 sigma^2 reaches 676, where a float64 rounding
    of x alone moves exp(-x) by 7e-14, so x and exp(-x) are formed in long double;
  * the long-range functions for x < 4 from the power series of P(a, x) (every term positive), beyond from the erf forms, which
    have lost their cancellation there (at y = 2 the terms differ by a factor of three at least);
  * the switch as f_c = 1 - h^n = cos^2(t) (1 + h + ... + h^(n-1)), h = sin^2(t), t = pi r / 2 r_x, with cos(t) =
    sin(pi (r_x - r) / 2 r_x): r_x - r is exact next to r_x, where 1 - h^n would be a difference of two numbers next to 1.

The switched functions and the switch itself are measured as the GPU tests measure them, relative to what the switch multiplies
(f_c to 1, f_c'/r to n pi / 2 r_x r, B to |B_lr|, dB to |dB_lr| + |B_lr| n pi / 2 r_x r, likewise C): one float32 step inside
r_x, f_c is 1e-14 and the rounding of r = sqrt(r^2) in float64 alone moves it by a millionth of itself.  Everything else is
measured relative to its own value.
"""

import importlib.util
import os

import numpy as np
import pytest
from scipy.special import erf, erfcx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SQRT_PI = np.sqrt(np.pi)
INV_GAMMA_92 = 16.0 / (105.0 * SQRT_PI)  # 1 / Gamma(9/2)
INV_GAMMA_72 = 8.0 / (15.0 * SQRT_PI)
INV_GAMMA_52 = 4.0 / (3.0 * SQRT_PI)


def long_range(sigma, r2):
    """(B_lr, C_lr, dB_lr, dC_lr) at r^2 = r2: P(3/2, x)/r^3, 3 P(5/2, x)/r^5, -C_lr, -15 P(7/2, x)/r^7."""
    r2 = np.asarray(r2, np.float64)
    alpha = 0.5 / sigma**2
    x = alpha * r2
    e = np.exp(-x)
    # x < 4: P(a, x) / r^2a = alpha^a e^-x S(a), S(a) = sum_k x^k / Gamma(a + k + 1), S(a) = 1 / Gamma(a + 1) + x S(a + 1)
    xs = np.minimum(x, 4.0)
    term, total = np.ones_like(xs), np.ones_like(xs)
    for k in range(1, 61):
        term = term * xs / (3.5 + k)
        total = total + term
    s72 = INV_GAMMA_92 * total
    s52 = INV_GAMMA_72 + xs * s72
    s32 = INV_GAMMA_52 + xs * s52
    a32e = alpha * np.sqrt(alpha) * e
    Bs, Cs, dCs = a32e * s32, 3 * alpha * a32e * s52, -15 * alpha**2 * a32e * s72
    # x >= 4: the erf forms
    r = np.sqrt(np.maximum(r2, 1e-300))
    y, ke = np.sqrt(x), 2.0 * np.sqrt(alpha / np.pi) * e
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = erf(y)
        Be = w / r**3 - ke / r2
        Ce = 3 * w / r**5 - ke * (2 * alpha / r2 + 3 / r2**2)
        dCe = -15 * w / r**7 + ke / r2 * (15 / r2**2 + 10 * alpha / r2 + 4 * alpha**2)
    small = x < 4.0
    B, C, dC = np.where(small, Bs, Be), np.where(small, Cs, Ce), np.where(small, dCs, dCe)
    return B, C, -C, dC


def switch(rx, n, r):
    """f_c and f_c'/r at r; zero from r_x on."""
    r = np.asarray(r, np.float64)
    inside = r < rx
    ri = np.where(inside, r, 0.5 * rx)
    sin_t, cos_t = np.sin(np.pi * ri / (2 * rx)), np.sin(np.pi * (rx - ri) / (2 * rx))
    h = sin_t**2
    fc = cos_t**2 * sum(h**k for k in range(n))
    dfc = -n * h ** (n - 1) * (np.pi / (2 * rx)) * (2 * sin_t * cos_t) / ri
    return np.where(inside, fc, 0.0), np.where(inside, dfc, 0.0)


def radial_closed_form(mode, sigma, r2, rx=None, degree=1):
    """(B, C, dB, dC) of csrc/dipole.hip's dipole_bc in float64, dB = B'/r and dC = C'/r; r2 = r^2.
    mode 0: direct (sigma unused); 1: short range; 2: exclusion, -f_c T_lr with radius rx and the given degree."""
    r2 = np.asarray(r2, np.float64)
    if mode == 0:
        r = np.sqrt(r2)
        return 1 / r**3, 3 / r**5, -3 / r**5, -15 / r**7
    if mode == 1:
        alpha = 0.5 / sigma**2
        xl = r2.astype(np.longdouble) / (2 * np.longdouble(sigma) ** 2)
        e = np.exp(-xl).astype(np.float64)
        r = np.sqrt(r2)
        w, ke = erfcx(np.sqrt(alpha) * r) * e, 2.0 * np.sqrt(alpha / np.pi) * e
        B = w / r**3 + ke / r2
        C = 3 * w / r**5 + ke * (2 * alpha / r2 + 3 / r2**2)
        dC = -15 * w / r**7 - ke / r2 * (15 / r2**2 + 10 * alpha / r2 + 4 * alpha**2)
        return B, C, -C, dC
    B, C, dB, dC = long_range(sigma, r2)
    fc, dfc = switch(rx, degree, np.sqrt(r2))
    return -fc * B, -fc * C, -(dfc * B + fc * dB), -(dfc * C + fc * dC)


# ---- tests ----------------------------------------------------------------------------------------------------------------------
CASES = [f"m{m}_s{i}" for m in (0, 1, 2) for i in (0, 1, 2)] + ["m2_wide"]
TOL = 1e-13


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "dipole_pointwise.npz"))


def case_parameters(g, case):
    mode = int(case[1])
    sigma = 1.0 if case == "m2_wide" else float(g["sigmas"][int(case[-1])])
    rx = float(g[case + "_rx"]) if mode == 2 else None
    return mode, sigma, rx


def _rel(what, got, ref, scale=None):
    scale = np.abs(ref) if scale is None else scale
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / scale
    err[(ref == 0) & (got == 0)] = 0.0
    print(f"[dipole-pointwise-host] {what:<28s} max rel err {err.max():.3e} over {ref.size} points")
    assert err.max() <= TOL, (what, int(err.argmax()), got[err.argmax()], ref[err.argmax()])


@pytest.mark.parametrize("case", CASES)
def test_closed_form_matches_golden(g, case):
    mode, sigma, rx = case_parameters(g, case)
    r2_2 = 2.0 * g[case + "_g2_s"].astype(np.float64) ** 2
    r2_3 = 3.0 * g[case + "_g3_s"].astype(np.float64) ** 2
    if mode < 2:
        B, C, dB, _ = radial_closed_form(mode, sigma, r2_2)
        dC = radial_closed_form(mode, sigma, r2_3)[3]
        for name, got in (("B", B), ("C", C), ("dB", dB), ("dC", dC)):
            _rel(f"{case} {name}", got, g[f"{case}_{name}"])
        return
    B, C, dB, _ = long_range(sigma, r2_2)
    _, C3, _, dC = long_range(sigma, r2_3)
    for name, got in (("Blr", B), ("Clr", C), ("dBlr", dB), ("Clr3", C3), ("dClr", dC)):
        _rel(f"{case} {name}", got, g[f"{case}_{name}"])
    for n in g["degrees"]:
        k = f"{case}_n{int(n)}"
        fc, dfc = switch(rx, int(n), np.sqrt(r2_2))
        fc3, dfc3 = switch(rx, int(n), np.sqrt(r2_3))
        B, C, dB, _ = radial_closed_form(2, sigma, r2_2, rx, int(n))
        dC = radial_closed_form(2, sigma, r2_3, rx, int(n))[3]
        # with the switch, relative to what it multiplies (see the module docstring)
        r_2, r_3 = np.sqrt(r2_2), np.sqrt(r2_3)
        w2, w3 = int(n) * np.pi / (2 * rx * r_2), int(n) * np.pi / (2 * rx * r_3)
        Blr, Clr, Clr3 = g[case + "_Blr"], g[case + "_Clr"], g[case + "_Clr3"]
        scales = {"fc": 1.0, "fc3": 1.0, "dfc": w2, "dfc3": w3, "B": Blr, "C": Clr, "dB": np.abs(g[case + "_dBlr"]) + Blr * w2,
                  "dC": np.abs(g[case + "_dClr"]) + Clr3 * w3}
        for name, got in (("fc", fc), ("dfc", dfc), ("fc3", fc3), ("dfc3", dfc3), ("B", B), ("C", C), ("dB", dB), ("dC", dC)):
            _rel(f"{k} {name}", got, g[f"{k}_{name}"], scales[name])
        outside = np.sqrt(r2_2) >= rx
        assert outside.sum() >= 3 and np.all(g[k + "_B"][outside] == 0) and np.all(g[k + "_dB"][outside] == 0)


@pytest.mark.parametrize("case", CASES)
def test_golden_derivatives(g, case):
    """B' = -r C, i.e. dB = B'/r = -C, and dC = C'/r: the stored derivatives against mpmath's numerical derivative (30 digits) of
    the generator's own B(r) and C(r), at every fourth point (and, with a switch, the points next to r_x)."""
    import mpmath as mp

    spec = importlib.util.spec_from_file_location("make_dipole_pointwise_golden", os.path.join(GOLDEN, "make_dipole_pointwise_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    mode, sigma, rx = case_parameters(g, case)
    degrees = [int(n) for n in g["degrees"]] if mode == 2 else [None]

    def fun(which, n):
        def f(r):
            val = gen.radial(mode, sigma, r * r)[which]
            return val if mode < 2 else -gen.switch(mp.mpf(rx), n, r)[0] * val
        return f

    with mp.workdps(30):
        for n in degrees:
            key = case if mode < 2 else f"{case}_n{n}"
            for which, name, geom in ((0, "dB", 2), (1, "dC", 3)):
                s = g[f"{case}_g{geom}_s"].astype(np.float64)
                ref = g[f"{key}_{name}"]
                idx = set(range(0, len(s), 4))
                if mode == 2:
                    idx |= set(np.flatnonzero(np.abs(s * np.sqrt(geom) / rx - 1) < 1e-6))
                worst = 0.0
                for i in sorted(idx):
                    r = mp.sqrt(geom * mp.mpf(float(s[i])) ** 2)
                    if mode == 2 and r >= rx:
                        assert ref[i] == 0.0
                        continue
                    d = mp.diff(fun(which, n), r, h=mp.mpf(10) ** -12 * r) / r
                    worst = max(worst, float(abs(d - mp.mpf(float(ref[i]))) / abs(d)))
                print(f"[dipole-pointwise-host] {key} {name} against the derivative of {'BC'[which]}: max rel err {worst:.3e}")
                assert worst <= TOL, (key, name)
            if mode < 2:  # B' = -r C at the same points
                assert np.array_equal(g[case + "_dB"], -g[case + "_C"])
            else:
                assert np.array_equal(g[case + "_dBlr"], -g[case + "_Clr"])
