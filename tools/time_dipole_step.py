"""GPU timing of GraphedDipoleStep against the eager sequence it replaces, at the three (N, K) sizes of tools/time_dipole.py and
in both dtypes:

  (a) eager:  pair vectors from positions and shifts with tensor ops, ``calc(...)``, ``(V * mu).sum().backward()`` with gradients
              to positions and dipoles
  (b) step:   ``step(positions, dipoles)`` -- two small copies and one graph replay

(a) and (b) are timed alternately in the same process, each call ending in a synchronise; the whole table is printed twice so
that the run-to-run spread is visible.

    python tools/time_dipole_step.py [--quick]

--quick: fewer repetitions and one pass (for a run under rocprofv3 --kernel-trace --stats)."""
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
    reps, passes = (3, 1) if QUICK else (20, 2)
    print(f"# {torch.cuda.get_device_name(0)}; ms per call ending in a synchronise (mean of {reps}, (a) and (b) alternating, after "
          "3 warm-up calls of each)")
    for run in range(passes):
        print(f"# run {run + 1}")
        for label, make in SIZES:
            pos, cell, mu, sm, lam, rc = make()
            pairs, S, _ = tpa.neighbor_list(pos, cell, rc)
            for dtype in (torch.float32, torch.float64):
                t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
                tc, tS = t(cell), t(S)
                ti = torch.tensor(pairs, device=dev)
                tp, tm = t(pos).requires_grad_(True), t(mu).requires_grad_(True)
                calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=sm), lr_wavelength=lam)
                K = int(np.prod(np.ceil(np.linalg.norm(cell, axis=1) / lam)))
                step = tpa.GraphedDipoleStep(calc, tm.detach(), tc, tp.detach(), ti, tS)
                pos_in, mu_in = tp.detach().clone(), tm.detach().clone()

                def eager():
                    tp.grad = tm.grad = None
                    vec = tp[ti[:, 1]] - tp[ti[:, 0]] + tS @ tc
                    E = (calc(tm, tc, tp, ti, vec) * tm).sum()
                    E.backward()
                    return E

                def graphed():
                    return step(pos_in, mu_in)

                for _ in range(3):
                    eager()
                    graphed()
                torch.cuda.synchronize()
                ms_a = ms_b = 0.0
                for _ in range(reps):
                    ms_a += one_call(eager) / reps
                    ms_b += one_call(graphed) / reps
                E_a, E_b = float(eager().detach()), float(graphed()[0])
                print(f"{label:22s} K={K:7d} n_k={step.n_k:7d} P={len(pairs):7d} {str(dtype)[6:]:8s} (a) eager fwd+bwd(pos, mu) "
                      f"{ms_a:8.3f}  (b) step {ms_b:8.3f}  a/b {ms_a / ms_b:5.2f}   E {E_a:.6f} / {E_b:.6f}", flush=True)


if __name__ == "__main__":
    main()
