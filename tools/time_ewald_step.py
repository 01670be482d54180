"""GPU timing of GraphedEwaldStep against what the package offered for an Ewald MD step before it, at three sizes an Ewald user
runs, with the cell gradient, in both dtypes:

  (a)  step:        ``step(positions)`` at a fixed cell -- one small copy and one graph replay
  (a') step, cell:  ``step(positions, cell=new)`` with ANOTHER cell in every call -- the point of the class: the same replay
  (b)  graphed:     ``GraphedEnergyForces(ewald_calc, ..., cell_gradient=True, charge_gradient=True)`` -- a replay of the captured
                    eager call (k-vector generation with tensor ops, four Ewald kernels, the general autograd nodes); fixed cell
  (c)  eager:       ``pair_distances``, the calculator, ``backward`` with a new cell tensor per call -- the only way to follow
                    the cell before this class

The four are timed alternately in the same process, in a new (seeded) order every round, each call ending in a synchronise; the
whole table is printed twice so that the run-to-run spread is visible.

    python tools/time_ewald_step.py [--quick]

--quick: fewer repetitions and one pass."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
LAM, CUTOFF, SMEARING = 1.25, 4.0, 1.0

# (label, atoms, box edge): lr_wavelength 1.25 gives 10^3, 16^3 and 32^3 k-vectors
SIZES = [("N=64", 64, 12.5), ("N=512", 512, 20.0), ("N=4096", 4096, 40.0)]


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    reps, passes = (3, 1) if QUICK else (20, 2)
    print(f"# {torch.cuda.get_device_name(0)}; ms per call ending in a synchronise (mean of {reps}, the four alternating in a shuffled order, after "
          "3 warm-up calls of each)")
    for run in range(passes):
        print(f"# run {run + 1}")
        for label, n, L in SIZES:
            rng = np.random.default_rng(n)
            pos, cell = rng.uniform(0, L, (n, 3)), np.eye(3) * L
            q = rng.normal(size=(n, 1))
            q -= q.mean()
            pairs, S, _ = tpa.neighbor_list(pos, cell, CUTOFF)
            for dtype in (torch.float32, torch.float64):
                t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
                tq, tc, tS, tp = t(q), t(cell), t(S), t(pos)
                ti = torch.tensor(pairs, device=dev)
                calc = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=SMEARING), lr_wavelength=LAM)
                K = int(np.prod(np.ceil(np.linalg.norm(cell, axis=1) / LAM)))
                step = tpa.GraphedEwaldStep(calc, tq, tc, tp, ti, tS, cell_gradient=True)
                parent = tpa.GraphedEnergyForces(calc, tq, tc, tp, ti, tS, cell_gradient=True, charge_gradient=True)
                # cells of the (a') and (c) calls: the box breathing by up to 0.1 %, all on the device before the clock starts
                cells = [t(cell * (1.0 + 1e-3 * np.sin(0.7 * i))) for i in range(reps + 4)]
                turn = [0]

                def fixed():
                    return step(tp)

                def moving():
                    turn[0] += 1
                    return step(tp, cell=cells[turn[0] % len(cells)])

                def graphed():
                    return parent(tp)

                def eager():
                    turn[0] += 1
                    p, c, qq = tp.clone().requires_grad_(True), cells[turn[0] % len(cells)].clone().requires_grad_(True), \
                        tq.clone().requires_grad_(True)
                    E = (calc(qq, c, p, ti, tpa.pair_distances(p, ti, c, tS)) * qq).sum()
                    E.backward()
                    return E

                fns = (fixed, moving, graphed, eager)
                for _ in range(3):
                    for fn in fns:
                        fn()
                torch.cuda.synchronize()
                ms = [0.0] * 4
                order = np.random.default_rng(run)
                for _ in range(reps):  # (a new order every round: the call that follows the slow eager one finds the queue cold)
                    for j in order.permutation(4):
                        ms[j] += one_call(fns[j]) / reps
                step(tp, cell=tc)
                E_a, E_b = float(fixed()[0]), float(graphed()[0])
                print(f"{label:7s} K={K:6d} n_k={step.n_k:6d} P={len(pairs):6d} {str(dtype)[6:]:8s} (a) step {ms[0]:7.3f}  (a') step, "
                      f"new cell {ms[1]:7.3f}  (b) graphed eager {ms[2]:7.3f}  (c) eager, new cell {ms[3]:7.3f}   b/a {ms[2] / ms[0]:5.2f}  "
                      f"a'/a {ms[1] / ms[0]:5.2f}  c/a' {ms[3] / ms[1]:5.2f}   E {E_a:.6f} / {E_b:.6f}", flush=True)


if __name__ == "__main__":
    main()
