"""GPU timing of the spline potential (csrc/spline.hip, SplinePotential) against its yardsticks, eager:

  1. P3M (5 nodes), energy + forces, with a reciprocal-axis spline of Coulomb's long-range part, on the 8 000-ion and the
     31 944-atom boxes of workloads.py, fp32 and fp64 -- against the same calculator with CoulombPotential and
     double_backward = "analytic": the same primitives plus a pair sum the spline does not have.
  2. mipme_spline_kfilter_build against analytic.filter_table (tensor operations) for the same potential, 64^3 and 128^3.
  3. mipme_spline_eval / mipme_spline_eval_reciprocal on 4.76 M distances against a device copy of the same bytes (the floor of a
     one-read-one-write kernel) and against the reciprocal-axis spline written as eager tensor operations
     (searchsorted, gathers, where -- how the reference evaluates it).

    python tools/time_spline.py [--quick]

--quick: fewer repetitions (for a run under rocprofv3 --kernel-trace --stats)."""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402
from torchpme_amd import analytic, splines, workloads  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
N_DIST = 4_760_000


def timed(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def coulomb_lr_spline(smearing, r_max, n_knots=128):
    r = torch.logspace(-2, math.log10(r_max), n_knots, dtype=torch.float64)
    y = torch.erf(r / (math.sqrt(2) * smearing)) / r
    return dict(r_grid=r, y_grid=y, reciprocal=True, y_at_zero=math.sqrt(2 / math.pi) / smearing, yhat_at_zero=0.0,
                smearing=smearing)


def calculators_section(reps):
    print(f"# 1. P3M, 5 nodes, energy + forces (backward w.r.t. positions through pair_distances), ms per call (mean of {reps})")
    for make in (workloads.ionic_box, workloads.water_box):
        w = make()
        spline_kw = coulomb_lr_spline(w.smearing, 2 * float(np.linalg.norm(w.cell[0])))
        for dtype in (torch.float32, torch.float64):
            t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
            q, cell, S = t(w.charges), t(w.cell), t(w.shifts)
            idx = torch.tensor(w.pairs, device=dev)
            pos = t(w.positions).requires_grad_(True)
            spline = tpa.P3MCalculator(tpa.SplinePotential(**spline_kw).to(dev), mesh_spacing=w.mesh_spacing, interpolation_nodes=5)
            coulomb = tpa.P3MCalculator(tpa.CoulombPotential(smearing=w.smearing).to(dev), mesh_spacing=w.mesh_spacing,
                                        interpolation_nodes=5)
            coulomb.double_backward = "analytic"

            def step(calc):
                pos.grad = None
                d = tpa.pair_distances(pos, idx, cell, S)
                E = (calc(q, cell, pos, idx, d) * q).sum()
                E.backward()
                return E.detach()

            e_s, e_c = float(step(spline)), float(step(coulomb))
            ms_s, ms_c = timed(lambda: step(spline), reps), timed(lambda: step(coulomb), reps)
            print(f"{w.name:12s} N={w.n_atoms:6d} P={w.n_pairs:8d} mesh={w.n_mesh}^3 {str(dtype)[6:]:8s} spline {ms_s:8.3f} | "
                  f"Coulomb, analytic route {ms_c:8.3f} | k-space energy: spline {e_s:.6f}, Coulomb incl. pair sum {e_c:.6f}",
                  flush=True)


def filter_section(reps):
    print(f"# 2. G(k) of a reciprocal-axis spline, P3M 5 nodes, float64, ms per table (mean of {reps})")
    pot = tpa.SplinePotential(**coulomb_lr_spline(1.8, 140.0)).to(dev)
    for n in (64, 128):
        L = 0.55 * (n - 2)
        cell = torch.eye(3, dtype=torch.float64, device=dev) * L
        calc = tpa.P3MCalculator(pot, mesh_spacing=2 * L / (n - 2), interpolation_nodes=5)
        geom = analytic._geometry(calc, cell)
        assert tuple(geom.ns) == (n, n, n), geom.ns
        krn, pref = pot._splines()[1], pot._prefactor_float()
        a = splines.build_filter(geom, krn, pref, torch.float64, dev)
        b = analytic.filter_table(calc.potential, geom.scheme, geom.order, cell, geom.ns, geom)
        err = float((a - b).abs().max() / b.abs().max())
        ms_k = timed(lambda: splines.build_filter(geom, krn, pref, torch.float64, dev), reps)
        ms_t = timed(lambda: analytic.filter_table(calc.potential, geom.scheme, geom.order, cell, geom.ns, geom), reps)
        print(f"{n}^3: mipme_spline_kfilter_build {ms_k:8.3f} | analytic.filter_table (tensor ops) {ms_t:8.3f} | rel. difference {err:.1e}",
              flush=True)


def eager_reciprocal(x, X, Y, D2, ZX, ZY, ZD2, split):
    """The reciprocal-axis spline as tensor operations: searchsorted, gathers, where."""

    def cubic(v, X, Y, D2):
        i = torch.clamp(torch.searchsorted(X, v, right=True) - 1, 0, len(X) - 2)
        h = X[i + 1] - X[i]
        a, b = (X[i + 1] - v) / h, (v - X[i]) / h
        h26 = h * h / 6
        return a * (Y[i] + (a * a - 1) * D2[i] * h26) + b * (Y[i + 1] + (b * b - 1) * D2[i + 1] * h26)

    below = x < split
    safe = torch.where(below, split, x)
    return torch.where(below, cubic(x, ZX, ZY, ZD2), cubic(torch.reciprocal(safe), X, Y, D2))


def pointwise_section(reps):
    print(f"# 3. {N_DIST} distances, ms per launch (mean of {reps}); GB/s = bytes read + written / time")
    kw = coulomb_lr_spline(1.8, 140.0)
    recip = tpa.lib.CubicSplineReciprocal(kw["r_grid"], kw["y_grid"], y_at_zero=kw["y_at_zero"])
    plain = tpa.lib.CubicSpline(kw["r_grid"], kw["y_grid"])
    big = tpa.lib.CubicSpline(torch.linspace(0.01, 140.0, 5000, dtype=torch.float64), torch.sin(torch.linspace(0, 50, 5000, dtype=torch.float64)))
    rng = np.random.default_rng(0)
    for dtype in (torch.float32, torch.float64):
        x = torch.tensor(rng.uniform(0.8, 9.0, N_DIST), device=dev, dtype=dtype)
        out = torch.empty_like(x)
        xg = x.clone().requires_grad_(True)
        item = x.element_size()
        tabs = [t.to(dev, dtype) for t in recip._rev.cpu()] + [t.to(dev, dtype) for t in recip._zero.cpu()]
        split = torch.tensor(recip._split, device=dev, dtype=dtype)

        def value_and_derivative():
            xg.grad = None
            recip(xg).backward(out)

        rows = [("device copy (floor, 1 read + 1 write)", lambda: out.copy_(x), 2),
                ("spline_eval order 0, 128 knots (LDS)", lambda: plain(x), 2),
                ("spline_eval order 0, 5000 knots (global)", lambda: big(x), 2),
                ("spline_eval_reciprocal, value", lambda: recip(x), 2),
                ("spline_eval_reciprocal, value + derivative, then g * d", value_and_derivative, 3),
                ("reciprocal-axis spline, eager tensor ops", lambda: eager_reciprocal(x, *tabs, split), 2)]
        for label, fn, words in rows:
            ms = timed(fn, reps)
            print(f"{str(dtype)[6:]:8s} {label:56s} {ms:8.3f} ms  {words * N_DIST * item / ms / 1e6:8.1f} GB/s", flush=True)


def main():
    reps = 3 if QUICK else 20
    print(f"# {torch.cuda.get_device_name(0)}; eager (2 warm-up calls before each timing)")
    pointwise_section(reps)
    filter_section(reps)
    calculators_section(reps)


if __name__ == "__main__":
    main()
