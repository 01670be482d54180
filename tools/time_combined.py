"""GPU timing of the combined potential (csrc/combined.hip, CombinedPotential) against its yardsticks, eager:

  1. P3M (5 nodes), energy + forces + weight gradient, Coulomb + 1/r^6 with learnable weights, on the 8 000-ion and the
     31 944-atom boxes of workloads.py, fp32 and fp64 -- against what a user does without the class: two calculators with
     double_backward = "analytic", one per member, summed with the weights (two mesh passes, two pair sums).
  2. mipme_combined_kfilter_build against analytic.filter_table (tensor operations) per term, 64^3 and 128^3.
  3. The pair node on 4.76 M distances, orders 0 and 1, two and three terms, per-term and weighted, against a device copy of the
     same bytes (the floor of a one-read-one-write kernel) and against the members' tensor sr_from_dist; the two ways of
     contracting the per-term values with learnable weights.

    python tools/time_combined.py [--quick]

--quick: fewer repetitions (for a run under rocprofv3 --kernel-trace --stats)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402
from torchpme_amd import analytic, combined, workloads  # noqa: E402

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


def members(smearing, n_terms=2):
    pots = [tpa.CoulombPotential(smearing=smearing), tpa.InversePowerLawPotential(exponent=6, smearing=smearing),
            tpa.InversePowerLawPotential(exponent=3, smearing=smearing)]
    return pots[:n_terms]


def calculators_section(reps):
    print(f"# 1. P3M, 5 nodes, energy + forces + dE/dw (backward w.r.t. positions through pair_distances and w.r.t. the "
          f"weights), ms per call (mean of {reps})")
    for make in (workloads.ionic_box, workloads.water_box):
        w = make()
        for dtype in (torch.float32, torch.float64):
            t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
            q, cell, S = t(w.charges), t(w.cell), t(w.shifts)
            idx = torch.tensor(w.pairs, device=dev)
            pos = t(w.positions).requires_grad_(True)
            kw = dict(mesh_spacing=w.mesh_spacing, interpolation_nodes=5)
            pot = tpa.CombinedPotential(members(w.smearing), initial_weights=torch.tensor([1.0, -0.3], dtype=dtype),
                                        smearing=w.smearing).to(dev)
            one = tpa.P3MCalculator(pot, **kw)
            singles = [tpa.P3MCalculator(m.to(dev), **kw) for m in members(w.smearing)]
            for c in singles:
                c.double_backward = "analytic"
            weights = torch.tensor([1.0, -0.3], dtype=dtype, device=dev, requires_grad=True)

            def step_combined():
                pos.grad = pot.weights.grad = None
                d = tpa.pair_distances(pos, idx, cell, S)
                E = (one(q, cell, pos, idx, d) * q).sum()
                E.backward()
                return E.detach()

            def step_two_calculators():
                pos.grad = weights.grad = None
                d = tpa.pair_distances(pos, idx, cell, S)
                V = sum(wt * c(q, cell, pos, idx, d) for wt, c in zip(weights, singles))
                E = (V * q).sum()
                E.backward()
                return E.detach()

            e_c, e_t = float(step_combined()), float(step_two_calculators())
            gw_c, gw_t = pot.weights.grad.tolist(), weights.grad.tolist()
            ms_c, ms_t = timed(step_combined, reps), timed(step_two_calculators, reps)
            print(f"{w.name:12s} N={w.n_atoms:6d} P={w.n_pairs:8d} mesh={w.n_mesh}^3 {str(dtype)[6:]:8s} combined {ms_c:8.3f} | "
                  f"two calculators, analytic route {ms_t:8.3f} | ratio {ms_t / ms_c:5.2f} | E {e_c:.6f} / {e_t:.6f} | "
                  f"dE/dw {gw_c[0]:.5f} {gw_c[1]:.5f} / {gw_t[0]:.5f} {gw_t[1]:.5f}", flush=True)


def filter_section(reps):
    print(f"# 2. G_t(k) of Coulomb + 1/r^6 + 1/r^3, P3M 5 nodes, float64, ms for all three tables (mean of {reps})")
    pots = [m.to(dev) for m in members(1.8, 3)]
    pot = tpa.CombinedPotential(pots, smearing=1.8).to(dev)
    plan = combined.plan(pot)
    for n in (64, 128):
        L = 0.55 * (n - 2)
        cell = torch.eye(3, dtype=torch.float64, device=dev) * L
        kw = dict(mesh_spacing=2 * L / (n - 2), interpolation_nodes=5)
        calcs = [tpa.P3MCalculator(m, **kw) for m in pots]
        geom = analytic._geometry(calcs[0], cell)
        assert tuple(geom.ns) == (n, n, n), geom.ns
        a = combined.build_tables(geom, plan, torch.float64, dev)
        b = torch.stack([analytic.filter_table(c.potential, geom.scheme, geom.order, cell, geom.ns, geom) for c in calcs])
        err = float(((a - b).abs().amax(dim=(1, 2, 3)) / b.abs().amax(dim=(1, 2, 3))).max())
        ms_k = timed(lambda: combined.build_tables(geom, plan, torch.float64, dev), reps)
        ms_t = timed(lambda: [analytic.filter_table(c.potential, geom.scheme, geom.order, cell, geom.ns, geom) for c in calcs], reps)
        print(f"{n}^3: mipme_combined_kfilter_build {ms_k:8.3f} | analytic.filter_table per term (tensor ops) {ms_t:8.3f} | "
              f"rel. difference {err:.1e}", flush=True)


def pointwise_section(reps):
    print(f"# 3. {N_DIST} distances, ms per call (mean of {reps}); GB/s = bytes read + written / time")
    rng = np.random.default_rng(0)
    for dtype in (torch.float32, torch.float64):
        x = torch.tensor(rng.uniform(0.8, 9.0, N_DIST), device=dev, dtype=dtype)
        out = torch.empty_like(x)
        item = x.element_size()
        rows = [("device copy (floor, 1 read + 1 write)", lambda: out.copy_(x), 2)]
        for T in (2, 3):
            pots = [m.to(dev) for m in members(1.8, T)]
            pot = tpa.CombinedPotential(pots, initial_weights=torch.tensor([1.0, -0.3, 0.5][:T], dtype=dtype), smearing=1.8).to(dev)
            plan = combined.plan(pot)
            w = pot.weights.detach()
            for order in (0, 1):
                rows.append((f"T={T} order {order}, per term (1 read + {T} writes)",
                             lambda plan=plan, order=order: combined._launch(plan, order, x, None), 1 + T))
                rows.append((f"T={T} order {order}, weighted (1 read + 1 write)",
                             lambda plan=plan, order=order, w=w: combined._launch(plan, order, x, w), 2))
            rows.append((f"T={T} members' tensor sr_from_dist, weighted sum", lambda pot=pot: pot.sr_from_dist(x), 2))
            terms = combined._launch(plan, 0, x, None)
            rows.append((f"T={T} contraction of the terms: einsum('t,tp->p')",
                         lambda w=w, terms=terms: torch.einsum("t,tp->p", w, terms), 1 + T))
            rows.append((f"T={T} contraction of the terms: (w[:, None] * terms).sum(0)",
                         lambda w=w, terms=terms: (w[:, None] * terms).sum(dim=0), 1 + T))
        with torch.no_grad():
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
