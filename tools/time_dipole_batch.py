"""GPU timing of GraphedDipoleBatch against the way the package served many small dipole systems before it, with the cell gradient,
in both dtypes and with NEW CELLS in every call:

  (a)  batch:  one ``GraphedDipoleBatch`` of the F frames: ``batch(cells=new)`` -- one copy of the (F, 3, 3) cells and one replay
  (b)  steps:  F ``GraphedDipoleStep(follow_cell=True)`` objects, ``step_f(cell=new_f)`` one after the other (a 3 x 3 copy and a
               replay each) and ONE synchronise at the end -- the fair form of the old way

Rows: F = 1, 8, 64 and 512 frames of 64 dipoles (10^3 k-vectors each), F = 8 and 64 frames of 512 dipoles (16^3), and one mixed
batch of one 4 096-dipole frame (32^3) beside 256 frames of 20 dipoles (7^3).  Every frame has its own random positions, dipoles
and list.  The two are timed alternately in the same process, in a new (seeded) order every round, each call ending in a
synchronise; both passes run on the same objects and the whole table is printed twice so that the run-to-run spread is visible.

    python tools/time_dipole_batch.py [--quick]

--quick: fewer repetitions, one pass and no 512-frame row."""
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
SMALL, MID, BIG, TINY = (64, 12.5), (512, 20.0), (4096, 40.0), (20, 8.5)  # (dipoles, box edge): 10^3, 16^3, 32^3 and 7^3 k-vectors

# (label, [(dipoles, box edge) per frame])
ROWS = [("64 x 1", [SMALL]), ("64 x 8", [SMALL] * 8), ("64 x 64", [SMALL] * 64), ("64 x 512", [SMALL] * 512),
        ("512 x 8", [MID] * 8), ("512 x 64", [MID] * 64), ("4096 + 20 x 256", [BIG] + [TINY] * 256)]


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def system(n, L, seed):
    rng = np.random.default_rng(seed)
    pos, cell = rng.uniform(0, L, (n, 3)), np.eye(3) * L
    mu = rng.normal(size=(n, 3))
    pairs, S, _ = tpa.neighbor_list(pos, cell, CUTOFF)
    return mu, cell, pos, np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(S).reshape(-1, 3)


def main():
    reps, passes = (3, 1) if QUICK else (20, 2)
    rows = [r for r in ROWS if not (QUICK and len(r[1]) > 300)]
    print(f"# {torch.cuda.get_device_name(0)}; ms per call ending in a synchronise (mean of {reps}, the two alternating in a shuffled "
          "order, after 3 warm-up calls of each)")
    lines = [[] for _ in range(passes)]
    for label, sizes in rows:
        systems = [system(n, L, 1000 * n + f) for f, (n, L) in enumerate(sizes)]
        F = len(systems)
        for dtype in (torch.float32, torch.float64):
            t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
            calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=SMEARING), lr_wavelength=LAM)
            frames = [(t(mu), t(cell), t(pos), torch.tensor(pairs, device=dev), t(S)) for mu, cell, pos, pairs, S in systems]
            batch = tpa.GraphedDipoleBatch(calc, frames, cell_gradient=True)
            steps = [tpa.GraphedDipoleStep(calc, *fr, cell_gradient=True, follow_cell=True) for fr in frames]
            # the cells of the calls: every box breathing by up to 0.1 %, all on the device before the clock starts
            base = torch.stack([fr[1] for fr in frames])
            cells = [base * (1.0 + 1e-3 * float(np.sin(0.7 * i))) for i in range(reps + 4)]
            turn = [0]

            def batched():
                turn[0] += 1
                return batch(cells=cells[turn[0] % len(cells)])

            def one_by_one():
                turn[0] += 1
                c = cells[turn[0] % len(cells)]
                for f, step in enumerate(steps):
                    step(cell=c[f])

            fns = (batched, one_by_one)
            for _ in range(3):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            for run in range(passes):
                ms = [0.0, 0.0]
                order = np.random.default_rng(run)
                for _ in range(reps):
                    for j in order.permutation(2):
                        ms[j] += one_call(fns[j]) / reps
                # the same cells for both: the energies must agree
                batch(cells=cells[0])
                for f, step in enumerate(steps):
                    step(cell=cells[0][f])
                torch.cuda.synchronize()
                E_a = batch.energies.double().cpu().numpy()
                E_b = np.array([float(s.energy) for s in steps])
                dev_E = float(np.abs(E_a - E_b).max() / max(1e-30, np.abs(E_b).max()))
                lines[run].append(f"{label:16s} F={F:4d} dipoles={batch.atom_ptr[-1]:6d} n_k={sum(batch.n_k):7d} {str(dtype)[6:]:8s} "
                                  f"(a) batch {ms[0]:8.3f}  (b) {F:3d} steps {ms[1]:8.3f}   b/a {ms[1] / ms[0]:6.2f}   (a) per frame "
                                  f"{1e3 * ms[0] / F:8.2f} us   max |E_a - E_b| / max |E| {dev_E:.1e}")
                print(f"[pass {run + 1}] " + lines[run][-1], flush=True)
            del batch, steps
    for run in range(passes):
        print(f"# run {run + 1}")
        print("\n".join(lines[run]), flush=True)


if __name__ == "__main__":
    main()
