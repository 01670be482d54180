"""GPU timing of GraphedDipoleStep(follow_cell=True) against the object without the keyword and against the eager sequence, at
the three (N, K) sizes of tools/time_dipole_step.py, with the cell gradient, in both dtypes:

  (a)  follow:        ``step(positions)`` of a ``follow_cell=True`` object at a fixed cell -- one small copy and one graph replay
                      that rebuilds the k table, 1/V and the inverse cell on the device
  (a') follow, cell:  ``step(positions, cell=new)`` with ANOTHER cell in every call -- the point of the keyword: the same replay
  (b)  fixed:         ``step(positions)`` of the object without the keyword (tables built once on the host); fixed cell
  (c)  eager:         pair vectors with tensor ops, ``calc(...)``, ``(V * mu).sum().backward()`` with a new cell tensor per call --
                      the only way to follow the cell before the keyword

The four are timed alternately in the same process, in a new (seeded) order every round, each call ending in a synchronise; the
whole table is printed twice so that the run-to-run spread is visible.

    python tools/time_dipole_cell_step.py [--quick] [--only-b]

--quick: fewer repetitions and one pass.  --only-b: (b) alone, one pass, with nothing the commits before the keyword lack: the
same file times the parent commit from a built checkout of it named by the environment variable TORCHPME_AMD_ROOT (an A/B of the
object without the keyword)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get("TORCHPME_AMD_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
ONLY_B = "--only-b" in sys.argv


def frame0():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dipole.npz"))
    return gold["frame0_positions"], gold["frame0_cell"], gold["frame0_dipoles"], float(gold["frame0_smearing"]), 0.1, 4.0


def random_box(n, L, lam, sm, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, L, (n, 3)), np.eye(3) * L, rng.normal(size=(n, 3)), sm, lam, 4.0


SIZES = [("N=8 (ESPResSo frame)", frame0), ("N=1000", lambda: random_box(1000, 27.0, 0.87, 1.5, 1)),
         ("N=8000", lambda: random_box(8000, 54.0, 2.0, 2.0, 2))]


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    reps, passes = (3, 1) if QUICK else (20, 1 if ONLY_B else 2)
    what = "(b) alone" if ONLY_B else "the four alternating in a shuffled order"
    print(f"# {torch.cuda.get_device_name(0)}; ms per call ending in a synchronise (mean of {reps}, {what}, after 3 warm-up calls "
          "of each)")
    for run in range(passes):
        print(f"# run {run + 1}")
        for label, make in SIZES:
            pos, cell, mu, sm, lam, rc = make()
            pairs, S, _ = tpa.neighbor_list(pos, cell, rc)
            for dtype in (torch.float32, torch.float64):
                t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
                tc, tS, tp, tm = t(cell), t(S), t(pos), t(mu)
                ti = torch.tensor(pairs, device=dev)
                calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=sm), lr_wavelength=lam)
                K = int(np.prod(np.ceil(np.linalg.norm(cell, axis=1) / lam)))
                plain = tpa.GraphedDipoleStep(calc, tm, tc, tp, ti, tS, cell_gradient=True)
                head = f"{label:22s} K={K:7d} n_k={plain.n_k:7d} P={len(pairs):7d} {str(dtype)[6:]:8s}"

                def fixed():
                    return plain(tp)

                if ONLY_B:
                    for _ in range(3):
                        fixed()
                    torch.cuda.synchronize()
                    ms_b = sum(one_call(fixed) for _ in range(reps)) / reps
                    print(f"{head} (b) fixed cell {ms_b:7.3f}   E {float(fixed()[0]):.6f}", flush=True)
                    continue
                step = tpa.GraphedDipoleStep(calc, tm, tc, tp, ti, tS, cell_gradient=True, follow_cell=True)
                # cells of the (a') and (c) calls: the box shrinking by up to 0.1 % (the N = 8 000 box is exactly 27 wavelengths
                # wide: a larger one has another grid), all on the device before the clock starts
                cells = [t(cell * (1.0 - 5e-4 * (1.0 + np.sin(0.7 * i)))) for i in range(reps + 4)]
                assert all(step.kgrid_matches(c) for c in cells)
                turn = [0]

                def follow():
                    return step(tp)

                def moving():
                    turn[0] += 1
                    return step(tp, cell=cells[turn[0] % len(cells)])

                def eager():
                    turn[0] += 1
                    p, m = tp.clone().requires_grad_(True), tm.clone().requires_grad_(True)
                    c = cells[turn[0] % len(cells)].clone().requires_grad_(True)
                    vec = p[ti[:, 1]] - p[ti[:, 0]] + tS @ c
                    E = (calc(m, c, p, ti, vec) * m).sum()
                    E.backward()
                    return E

                fns = (follow, moving, fixed, eager)
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
                E_a, E_b = float(follow()[0]), float(fixed()[0])
                print(f"{head} (a) follow {ms[0]:7.3f}  (a') follow, new cell {ms[1]:7.3f}  (b) fixed cell {ms[2]:7.3f}  (c) eager, "
                      f"new cell {ms[3]:7.3f}   a-b {1e3 * (ms[0] - ms[2]):+6.1f} us  a'-a {1e3 * (ms[1] - ms[0]):+6.1f} us  "
                      f"c/a' {ms[3] / ms[1]:5.2f}   E {E_a:.6f} / {E_b:.6f}  status {int(step.status.cpu()[0])}", flush=True)


if __name__ == "__main__":
    main()
