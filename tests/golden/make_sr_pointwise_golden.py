"""Generate tests/golden/sr_pointwise.npz: the short-range pair function v_SR(d), its derivative, erfc and erfcx, point by
point, from mpmath at 60 digits (our own formulas, the ones oracle/pme_numpy.py::sr_pair states; nothing else is imported).

    python tests/golden/make_sr_pointwise_golden.py

Every reference value is taken at the number the kernel under test really receives: the stored input, read exactly.

Contents
  y, erfcx, erfc           float64 grid in y = d / (sigma sqrt 2) and the two functions at it: ~2000 points on (0, 6.5), every
                           boundary k/8 of the erfcx table (k = 1..52) with its two float64 neighbours, ~100 points on
                           [6.5, 27] with 6.5, its predecessor and y = sqrt(700 -+ 1) (the end of exp's range reduction)
  exp_x, exp_ref           float64 x = fl(y^2) for every third y, x = 699 .. 1e6 in steps across the end of the double range, and
                           exp(-x) (correctly rounded, subnormal or zero where it must be)
  sigmas                   the three smearings of the mode-1 sets
  m1_d_s<i>                float32 distances for sigma i (the y grid thinned -- see N_INTERIOR -- and mapped to d; the boundaries
                           k/8 keep their two float32 neighbours): input of the functions that take d.  float32 values are
                           float64 values too, so one reference serves both precisions
  m1_v_p<p>_s<i>, m1_dv_*  v_SR and dv_SR/dd of mode 1 (range separated: pref Q(p/2, x) / d^p), p = 1..6, at m1_d_s<i>
  m1_d2_s<i>               float32 SQUARED distances: input of the functions that take d^2; the reference is taken at the exact
                           square root of the stored value
  f1_v_p<p>_s<i>, f1_dv_*  the same functions at sqrt(m1_d2_s<i>), p = 1 and 6 (the exponents with a d^2-driven fast form)
  ex_cases                 rows (mode, p, exclusion_degree) of the coarse sets: modes 0 (bare), 2 (-v_LR f_cut), 3 (v (1 - f_cut))
  ex_sigma, ex_rx          their smearing (mode 2) and exclusion radius (modes 2, 3)
  ex_d                     float32 distances, 0.01 sigma to beyond rx, with x = d^2 / 2 sigma^2 = 1 and d = rx bracketed by
                           -+ 1 float32 step and -+ 1e-3
  ex_v_<k>, ex_dv_<k>      v_SR, dv_SR/dd of case k at ex_d;  ex_big_<k>: |v_LR| (mode 2) or |v| bare (modes 0, 3) there
  lg_x, lg_P_p<p>          float32 x in [1e-5, 1] and the regularised lower incomplete gamma function P(p/2, x), p = 1..6
  rows_sigma, rows_off     the "star" of tests/test_gpu_sr_pointwise.py: 300 partner offsets from a centre, multiples of 2^-17
                           (so centre + offset is exact in float32 for centres on a 2^-10 lattice inside a 60 x 60 x 60 cell)
  rows_d, rows_v_p<p>, rows_dv_p<p>   their exact lengths (rounded once) and v_SR, dv_SR/dd there, p = 1 and 6
The script prints the share of the mode-1 points in each tolerance class of the test (y <= 6.5; y > 6.5; float32 underflow).
"""

import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 60

SIGMAS = (0.6, 1.0, 2.3)
N_INTERIOR = {0: 260, 1: 600, 2: 260}  # points of (0, 6.5) kept per sigma (the file has to stay below 500 KB)
EX_SIGMA, EX_RX = 1.0, 3.5


def f64(v):
    return float(v)


def y_grid():
    rng = np.random.default_rng(20240607)
    interior = np.sort(rng.uniform(0.004, 6.496, 2000))
    bnd = []
    for k in range(1, 53):
        b = k / 8.0
        bnd += [np.nextafter(b, 0.0), b, np.nextafter(b, 100.0)]
    tail = list(np.sort(rng.uniform(6.5, 27.0, 92)))
    tail += [6.5, np.nextafter(6.5, 0.0), 6.75, 9.0, float(mp.sqrt(699)), float(mp.sqrt(700)), float(mp.sqrt(701)), 27.0]
    return np.unique(np.concatenate([interior, bnd, tail]))


def Q_and_dens(p, x):
    """Q(p/2, x), the regularised upper incomplete gamma function, and x^(p/2-1) e^-x / Gamma(p/2)."""
    ex = mp.e ** (-x)
    if p % 2 == 0:
        a = p // 2
        Q = ex * sum(x**k / mp.factorial(k) for k in range(a))
    else:
        Q = mp.erfc(mp.sqrt(x)) + ex * sum(x ** (k - mp.mpf(1) / 2) / mp.gamma(k + mp.mpf(1) / 2) for k in range(1, (p - 1) // 2 + 1))
    dens = x ** (mp.mpf(p) / 2 - 1) * ex / mp.gamma(mp.mpf(p) / 2)
    return Q, dens


def mode1(p, sigma, d):
    """pref Q(p/2, x) / d^p and its derivative in d; sigma is the double the descriptor carries, read exactly."""
    s = mp.mpf(sigma)
    x = d * d / (2 * s * s)
    Q, dens = Q_and_dens(p, x)
    v = Q / d**p
    dv = -dens * (d / (s * s)) / d**p - p * Q / d ** (p + 1)
    return v, dv


def fcut(rx, n, d):
    if d >= rx:
        return mp.mpf(0), mp.mpf(0)
    base = (1 - mp.cos(mp.pi * d / rx)) / 2
    return 1 - base**n, -n * base ** (n - 1) * (mp.pi / (2 * rx)) * mp.sin(mp.pi * d / rx)


def excl(mode, p, n, d):
    """(v, dv, big): modes 0, 2, 3 of srpot.h; big = |v_LR| (mode 2) or the bare |v| (modes 0, 3)."""
    rx = mp.mpf(EX_RX)
    if mode == 0:
        v = 1 / d**p
        return v, -p * v / d, v
    f, df = fcut(rx, n, d)
    if mode == 3:
        v = 1 / d**p
        dv = -p * v / d
        return v * (1 - f), dv * (1 - f) - v * df, v
    s = mp.mpf(EX_SIGMA)
    x = d * d / (2 * s * s)
    Q, dens = Q_and_dens(p, x)
    P = 1 - Q
    vl = P / d**p
    dvl = dens * (d / (s * s)) / d**p - p * P / d ** (p + 1)
    return -vl * f, -(dvl * f + vl * df), vl


def thin(y, n_interior):
    """The y grid with its part inside (0, 6.5) thinned to n_interior points and its tail to a third (the named points stay);
    the table boundaries stay."""
    on_boundary = np.zeros(len(y), bool)
    for k in range(1, 53):
        on_boundary |= np.abs(y - k / 8.0) < 1e-12
    interior = np.flatnonzero((y < 6.5) & ~on_boundary)
    keep = interior[np.linspace(0, len(interior) - 1, n_interior).round().astype(int)]
    special = [6.75, 9.0, float(mp.sqrt(699)), float(mp.sqrt(700)), float(mp.sqrt(701)), 27.0]
    sel = on_boundary | np.isin(y, special)
    sel[keep] = True
    sel[np.flatnonzero((y > 6.5) & ~on_boundary)[::3]] = True  # (the tail classes may hold a tenth of the points at most)
    return y[sel], on_boundary[sel]


def f32_with_neighbours(vals, centre_mask):
    """float32 roundings of vals; the entries flagged in centre_mask that are the middle of a (pred, b, succ) triple get their
    two float32 neighbours in place of the roundings of the float64 neighbours (which would coincide with b)."""
    out = np.asarray(vals, np.float64).astype(np.float32)
    idx = np.flatnonzero(centre_mask)
    for t in range(0, len(idx) - 2, 3):
        lo, mid, hi = idx[t], idx[t + 1], idx[t + 2]
        out[lo] = np.nextafter(out[mid], np.float32(0))
        out[hi] = np.nextafter(out[mid], np.float32(1e9))
    return np.unique(out)


def main():
    out = {}
    y = y_grid()
    out["y"] = y
    out["erfc"] = np.array([f64(mp.erfc(mp.mpf(float(t)))) for t in y])
    out["erfcx"] = np.array([f64(mp.erfc(mp.mpf(float(t))) * mp.e ** (mp.mpf(float(t)) ** 2)) for t in y])
    out["sigmas"] = np.array(SIGMAS)
    # exp(-x) at x = fl(y^2) (what the row body forms from d^2) for every third y, and past the end of the double range
    exp_x = np.unique(np.concatenate([(y * y)[::3], [699.0, 700.0, 701.0, 708.0, 709.0, 730.0, 744.0, 745.0, 746.0, 800.0, 1e6]]))
    out["exp_x"] = exp_x
    out["exp_ref"] = np.array([f64(mp.e ** (-mp.mpf(float(t)))) for t in exp_x])

    n_tot = n_tail = n_under = 0
    for i, sigma in enumerate(SIGMAS):
        ys, bmask = thin(y, N_INTERIOR[i])
        d32 = f32_with_neighbours(ys * sigma * np.sqrt(2.0), bmask)
        out[f"m1_d_s{i}"] = d32
        d2_32 = f32_with_neighbours((ys * sigma * np.sqrt(2.0)) ** 2, bmask)
        out[f"m1_d2_s{i}"] = d2_32
        for p in range(1, 7):
            ref = [mode1(p, sigma, mp.mpf(float(d))) for d in d32]
            out[f"m1_v_p{p}_s{i}"] = np.array([f64(r[0]) for r in ref])
            out[f"m1_dv_p{p}_s{i}"] = np.array([f64(r[1]) for r in ref])
            yy = d32.astype(np.float64) / (sigma * np.sqrt(2.0))
            n_tot += len(d32)
            under = np.abs(out[f"m1_v_p{p}_s{i}"]) < 2.0**-120
            n_under += int(under.sum())
            n_tail += int(((yy > 6.5) & ~under).sum())
        for p in (1, 6):
            ref = [mode1(p, sigma, mp.sqrt(mp.mpf(float(d2)))) for d2 in d2_32]
            out[f"f1_v_p{p}_s{i}"] = np.array([f64(r[0]) for r in ref])
            out[f"f1_dv_p{p}_s{i}"] = np.array([f64(r[1]) for r in ref])
    print(f"mode 1: {n_tot} points; y <= 6.5: {1 - (n_tail + n_under) / n_tot:.3f}, y > 6.5: {n_tail / n_tot:.3f}, "
          f"float32 underflow: {n_under / n_tot:.3f}")
    assert (n_tail + n_under) / n_tot <= 0.1
    ny_tail = int((y > 6.5).sum())
    print(f"y grid: {len(y)} points, y > 6.5: {ny_tail / len(y):.3f}")
    assert ny_tail / len(y) <= 0.1

    # ---- modes 0, 2, 3 ----
    rng = np.random.default_rng(5)
    d = list(np.exp(rng.uniform(np.log(0.01 * EX_SIGMA), np.log(1.3 * EX_RX), 240)))
    for c in (np.sqrt(2.0) * EX_SIGMA, EX_RX):  # x = 1 and d = rx
        c32 = np.float32(c)
        d += [c32, np.nextafter(c32, np.float32(0)), np.nextafter(c32, np.float32(1e9)), c * (1 - 1e-3), c * (1 + 1e-3)]
    ex_d = np.unique(np.asarray(d, np.float64).astype(np.float32))
    out["ex_d"] = ex_d
    out["ex_sigma"], out["ex_rx"] = np.array(EX_SIGMA), np.array(EX_RX)
    cases = [(0, p, 1) for p in (1, 3, 5, 6)] + [(m, p, n) for m in (2, 3) for p in (1, 3, 5, 6) for n in (1, 2, 8)]
    out["ex_cases"] = np.array(cases, np.int32)
    for k, (m, p, n) in enumerate(cases):
        ref = [excl(m, p, n, mp.mpf(float(t))) for t in ex_d]
        out[f"ex_v_{k}"] = np.array([f64(r[0]) for r in ref])
        out[f"ex_dv_{k}"] = np.array([f64(r[1]) for r in ref])
        out[f"ex_big_{k}"] = np.array([f64(abs(r[2])) for r in ref])

    # ---- lower incomplete gamma P(p/2, x) on the range of its power series ----
    lg_x = np.unique(np.concatenate([np.exp(rng.uniform(np.log(1e-5), 0.0, 96)), [1e-5, 0.5, np.nextafter(1.0, 0.0), 1.0]])
                     .astype(np.float32))
    out["lg_x"] = lg_x
    for p in range(1, 7):
        out[f"lg_P_p{p}"] = np.array([f64(1 - Q_and_dens(p, mp.mpf(float(t)))[0]) for t in lg_x])

    # ---- the star of the row tests ----
    rows_sigma = 0.6
    rng = np.random.default_rng(11)
    cyc = np.concatenate([rng.uniform(0.3, 4.0, 40), rng.uniform(4.0, 6.5, 14), [6.5, 6.5625, 6.9, 7.4, 8.0],
                          [k / 8.0 for k in (9, 17, 33, 40, 47)]])
    rng.shuffle(cyc)
    u = rng.normal(size=(300, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    off = u * (cyc[np.arange(300) % len(cyc)] * rows_sigma * np.sqrt(2.0))[:, None]
    off = np.round(off * 2.0**17) / 2.0**17
    out["rows_sigma"], out["rows_off"] = np.array(rows_sigma), off
    dd = [mp.sqrt(sum(mp.mpf(float(c)) ** 2 for c in o)) for o in off]
    out["rows_d"] = np.array([f64(t) for t in dd])
    for p in (1, 6):
        ref = [mode1(p, rows_sigma, t) for t in dd]
        out[f"rows_v_p{p}"] = np.array([f64(r[0]) for r in ref])
        out[f"rows_dv_p{p}"] = np.array([f64(r[1]) for r in ref])

    path = os.path.join(HERE, "sr_pointwise.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes")
    assert size < 500_000


if __name__ == "__main__":
    main()
