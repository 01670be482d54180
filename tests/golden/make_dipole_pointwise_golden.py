"""Generate tests/golden/dipole_pointwise.npz: the radial functions of the dipolar pair tensor T = B I - C r r^T (csrc/dipole.hip,
dipole_bc) and their derivatives dB = B'/r, dC = C'/r, point by point, from mpmath at 40 digits.  The formulas are our own, written
with the regularised incomplete gamma functions (x = alpha r^2, alpha = 1 / 2 sigma^2), not with the erf / erfc differences the
kernel and the closed form of tests/test_dipole_pointwise_host.py evaluate:

    mode 0  direct        B = 1/r^3                C = 3/r^5                  dC = -15/r^7
    mode 1  short range   B = Q(3/2, x)/r^3        C = 3 Q(5/2, x)/r^5        dC = -15 Q(7/2, x)/r^7
            long range    B_lr = P(3/2, x)/r^3     C_lr = 3 P(5/2, x)/r^5     dC_lr = -15 P(7/2, x)/r^7        dB = -C in all three
    mode 2  exclusion     -f_c T_lr:  B = -f_c B_lr,  dB = -(f_c'/r B_lr + f_c dB_lr),  likewise C;  f_c = 1 - h^n,
                          h = (1 - cos(pi r / r_x)) / 2 inside r_x, f_c = 0 from r_x on

    python tests/golden/make_dipole_pointwise_golden.py

Inputs are float32 scalars s (float32 values are float64 values too: both precisions receive the same numbers).  The tests place
a pair at r = (s, s, 0) to read B, C and dB, and at r = (s, s, s) to read dC, so the references are taken at r^2 = 2 s^2 and
r^2 = 3 s^2 exactly, each geometry with a grid of its own ("g2", "g3") that covers the y range of the case.

Grids in y = sqrt(x) = r / (sigma sqrt 2): geometric from 1e-3 to 1, linear above; y = 1, 2, 6.5 and r = r_x (where they lie in
the range) with their two float32 neighbours in s.

Contents (case = m0_s<i>, m1_s<i>, m2_s<i> for sigma i of `sigmas`, and m2_wide: sigma = 1, r_x = 12 sigma)
  sigmas, degrees                the smearings and the exclusion degrees
  <case>_rx                      exclusion radius (mode 2): 2.5 sigma, 12 sigma for m2_wide
  <case>_g2_s, <case>_g3_s       float32 inputs of the two geometries
  <case>_B, _C, _dB              at r^2 = 2 s^2 (g2);  <case>_dC at r^2 = 3 s^2 (g3)        -- modes 0 and 1
  <case>_Blr, _Clr, _dBlr        long-range functions at g2;  <case>_Clr3, _dClr at g3       -- mode 2
  <case>_n<n>_fc, _dfc           f_c and f_c'/r at g2;  _fc3, _dfc3 at g3                    -- mode 2, degree n
  <case>_n<n>_B, _C, _dB, _dC    the switched functions (g2, g2, g2, g3)
  <case>_under32, _under64       four counts (B, C, dB, dC): the points whose reference OUTPUT ELEMENT with prefactor 1 --
                                 B/2, C s^2/2, |dB| s/2, |dC| s^3/2; for mode 2 the same with the long-range functions, which is
                                 what the switch multiplies -- lies below 2^-120 (float32; in mode 1 counted over the points with
                                 y <= 9, its float32 range) or 2^-1016 (float64).  Zero for modes 0 and 2 (asserted here).
"""

import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 40

SIGMAS = (0.5, 1.0, 2.5)
DEGREES = (1, 2, 4)
Y_LO = 1e-3
Y_F32_MAX = 9.0  # mode 1 in float32 (beyond it everything underflows); float64 goes to 26
N_MODE01, N_MODE2 = 400, 180  # points per grid (mode 2 stores 29 arrays per case and point: the file has to stay below 300 KB)


def grid(sigma, geom, y_hi, n, specials_r=()):
    """float32 s with y = s sqrt(geom) / (sigma sqrt 2) on [Y_LO, y_hi]."""
    n_geo = n * 3 // 8
    y = np.concatenate([np.geomspace(Y_LO, 1.0, n_geo, endpoint=False), np.linspace(1.0, y_hi, n - n_geo)])
    if y_hi > Y_F32_MAX:  # mode 1: two thirds of the linear part inside the float32 range
        n_in = (n - n_geo) * 2 // 3
        y = np.concatenate([y[:n_geo], np.linspace(1.0, Y_F32_MAX, n_in), np.linspace(Y_F32_MAX, y_hi, n - n_geo - n_in + 1)[1:]])
    to_s = sigma * np.sqrt(2.0) / np.sqrt(float(geom))
    s = list((y * to_s).astype(np.float32))
    for r in [yy * sigma * np.sqrt(2.0) for yy in (1.0, 2.0, 6.5) if yy <= y_hi] + list(specials_r):
        c = np.float32(r / np.sqrt(float(geom)))
        s += [np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(1e9))]
    return np.unique(np.asarray(s, np.float32))


def radial(mode, sigma, r2):
    """(B, C, dB, dC) at r^2 = r2 (mpf); mode 0 direct, 1 short range, 2 long range (unswitched)."""
    r = mp.sqrt(r2)
    if mode == 0:
        g32 = g52 = g72 = mp.mpf(1)
    else:
        x = r2 / (2 * mp.mpf(sigma) ** 2)
        lo, hi = (x, mp.inf) if mode == 1 else (0, x)
        g32, g52, g72 = (mp.gammainc(mp.mpf(a) / 2, lo, hi, regularized=True) for a in (3, 5, 7))
    C = 3 * g52 / r**5
    return g32 / r**3, C, -C, -15 * g72 / r**7


def switch(rx, n, r):
    """f_c and f_c'/r."""
    if r >= rx:
        return mp.mpf(0), mp.mpf(0)
    h = (1 - mp.cos(mp.pi * r / rx)) / 2
    return 1 - h**n, -n * h ** (n - 1) * (mp.pi / (2 * rx)) * mp.sin(mp.pi * r / rx) / r


def arr(v):
    return np.array([float(t) for t in v])


def under_counts(s2, s3, y2, y3, B, C, dB, dC, y32_max=np.inf):
    """Points whose output element (prefactor 1) is below the range: see the module docstring."""
    el = [(np.abs(B) / 2, y2), (np.abs(C) * s2**2 / 2, y2), (np.abs(dB) * s2 / 2, y2), (np.abs(dC) * s3**3 / 2, y3)]
    u32 = [int(((e < 2.0**-120) & (y <= y32_max)).sum()) for e, y in el]
    u64 = [int((e < 2.0**-1016).sum()) for e, _ in el]
    return np.array(u32), np.array(u64)


def main():
    out = {"sigmas": np.array(SIGMAS), "degrees": np.array(DEGREES)}
    cases = [(f"m0_s{i}", 0, s, None) for i, s in enumerate(SIGMAS)] + [(f"m1_s{i}", 1, s, None) for i, s in enumerate(SIGMAS)]
    cases += [(f"m2_s{i}", 2, s, 2.5 * s) for i, s in enumerate(SIGMAS)] + [("m2_wide", 2, 1.0, 12.0)]
    for name, mode, sigma, rx in cases:
        root2s = sigma * np.sqrt(2.0)
        if mode == 0:
            y_hi, n, sp = 7.0, N_MODE01, ()
        elif mode == 1:
            y_hi, n, sp = 26.0, N_MODE01, ()
        else:
            y_hi, n, sp = 1.25 * rx / root2s, N_MODE2, (rx,)  # m2_wide: y to 10.6; the others to 2.2
        s2, s3 = grid(sigma, 2, y_hi, n, sp), grid(sigma, 3, y_hi, n, sp)
        out[f"{name}_g2_s"], out[f"{name}_g3_s"] = s2, s3
        r2_2 = [2 * mp.mpf(float(t)) ** 2 for t in s2]
        r2_3 = [3 * mp.mpf(float(t)) ** 2 for t in s3]
        f2 = [radial(mode, sigma, t) for t in r2_2]
        f3 = [radial(mode, sigma, t) for t in r2_3]
        s2d, s3d = s2.astype(np.float64), s3.astype(np.float64)
        y2, y3 = s2d * np.sqrt(2.0) / root2s, s3d * np.sqrt(3.0) / root2s
        if mode < 2:
            B, C, dB, dC = arr(t[0] for t in f2), arr(t[1] for t in f2), arr(t[2] for t in f2), arr(t[3] for t in f3)
            out[f"{name}_B"], out[f"{name}_C"], out[f"{name}_dB"], out[f"{name}_dC"] = B, C, dB, dC
            u32, u64 = under_counts(s2d, s3d, y2, y3, B, C, dB, dC, Y_F32_MAX if mode == 1 else np.inf)
        else:
            out[f"{name}_rx"] = np.array(rx)
            Blr, Clr, dBlr = arr(t[0] for t in f2), arr(t[1] for t in f2), arr(t[2] for t in f2)
            Clr3, dClr = arr(t[1] for t in f3), arr(t[3] for t in f3)
            out[f"{name}_Blr"], out[f"{name}_Clr"], out[f"{name}_dBlr"] = Blr, Clr, dBlr
            out[f"{name}_Clr3"], out[f"{name}_dClr"] = Clr3, dClr
            u32, u64 = under_counts(s2d, s3d, y2, y3, Blr, Clr, dBlr, dClr)
            for n_deg in DEGREES:
                sw2 = [switch(mp.mpf(rx), n_deg, mp.sqrt(t)) for t in r2_2]
                sw3 = [switch(mp.mpf(rx), n_deg, mp.sqrt(t)) for t in r2_3]
                k = f"{name}_n{n_deg}"
                out[k + "_fc"], out[k + "_dfc"] = arr(t[0] for t in sw2), arr(t[1] for t in sw2)
                out[k + "_fc3"], out[k + "_dfc3"] = arr(t[0] for t in sw3), arr(t[1] for t in sw3)
                out[k + "_B"] = arr(-w[0] * f[0] for w, f in zip(sw2, f2))
                out[k + "_C"] = arr(-w[0] * f[1] for w, f in zip(sw2, f2))
                out[k + "_dB"] = arr(-(w[1] * f[0] + w[0] * f[2]) for w, f in zip(sw2, f2))
                out[k + "_dC"] = arr(-(w[1] * f[1] + w[0] * f[3]) for w, f in zip(sw3, f3))
        out[f"{name}_under32"], out[f"{name}_under64"] = u32, u64
        print(f"{name}: {len(s2)} + {len(s3)} points, y to {y2.max():.2f} / {y3.max():.2f}; underflow class float32 {u32}, float64 {u64}")
        if mode != 1:
            assert not u32.any() and not u64.any(), name
    path = os.path.join(HERE, "dipole_pointwise.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes")
    assert size < 300_000


if __name__ == "__main__":
    main()
