"""GPU timing of the multi-channel Ewald step and batch (``n_channels=C``) against the two ways the package served (N, C) charges
before them, with the cell gradient, in both dtypes and with NEW CELLS in every call:

  (a)  one multi-channel object: ``step(cell=new)`` / ``batch(cells=new)`` -- one copy of the cells and one replay
  (b)  C single-channel objects, one per channel, replayed one after the other with the same new cells and ONE synchronise at the
       end -- the fair form of the old way
  (c)  the eager sequence -- pair_distances, EwaldCalculator with (N, C) charges, backward to positions, charges and cell -- with
       new cell tensors; for a batch the frames one after the other

Rows: the step with C = 2, 4, 8 at 64 atoms / 10^3 k-vectors, 512 / 16^3 and 4 096 / 32^3; the batch with C = 2, 8 at 64 frames of
64 atoms, 64 frames of 512 atoms and 512 frames of 64 atoms.  The ways alternate in one process in a new (seeded) order every
round, every call ends in a synchronise; both passes run on the same objects and the whole table is printed twice, as run 1 and
run 2.  The last table gives per row b/a of both runs and the run-to-run spread of (a) and of (b): a row counts as won only where
(a) is below (b) by more than that spread.  (c) is slow and runs in the first rounds of a pass only (its count is in the table).

    python tools/time_ewald_channels.py [--quick] [--out FILE]

The table goes to FILE (default profiles/ewald_channels_times.txt) and to the standard output.  --quick: fewer repetitions, one
pass, no 4 096-atom and no 512-frame row."""
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
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ewald_channels_times.txt")
LAM, CUTOFF, SMEARING = 1.25, 4.0, 1.0
SMALL, MID, BIG = (64, 12.5), (512, 20.0), (4096, 40.0)  # (atoms, box edge): 10^3, 16^3 and 32^3 k-vectors
CMAX = 8

# (label, [(atoms, box edge) per frame], channel counts); one frame: the step
ROWS = [("step 64", [SMALL], (2, 4, 8)), ("step 512", [MID], (2, 4, 8)), ("step 4096", [BIG], (2, 4, 8)),
        ("batch 64 x 64", [SMALL] * 64, (2, 8)), ("batch 512 x 64", [MID] * 64, (2, 8)), ("batch 64 x 512", [SMALL] * 512, (2, 8))]

_lines = []


def say(text=""):
    print(text, flush=True)
    _lines.append(text)


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def system(n, L, seed):
    rng = np.random.default_rng(seed)
    pos, cell = rng.uniform(0, L, (n, 3)), np.eye(3) * L
    q = rng.normal(size=(n, CMAX))
    q -= q.mean(axis=0)
    pairs, S, _ = tpa.neighbor_list(pos, cell, CUTOFF)
    return q, cell, pos, np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(S).reshape(-1, 3)


def eager_frame(calc, q, cell, pos, idx, sh):
    tq, tp, tc = (x.detach().clone().requires_grad_(True) for x in (q, pos, cell))
    V = calc(tq, tc, tp, idx, tpa.pair_distances(tp, idx, tc, sh))
    (V * tq).sum().backward()
    return tp.grad, tq.grad, tc.grad


def main():
    reps, reps_c, passes = (3, 1, 1) if QUICK else (20, 3, 2)
    rows = [r for r in ROWS if not (QUICK and (len(r[1]) > 300 or r[1][0] == BIG))]
    say(f"# {torch.cuda.get_device_name(0)}; ms per call ending in a synchronise, cell_gradient=True, new cells in every call; mean of "
        f"{reps} calls of (a) and (b) and of {reps_c} of (c), the ways alternating in a shuffled order, after 3 warm-up calls of each")
    table = [[] for _ in range(passes)]
    summary = []
    for label, sizes, channels in rows:
        systems = [system(n, L, 1000 * n + f) for f, (n, L) in enumerate(sizes)]
        F = len(systems)
        is_step = F == 1
        for dtype in (torch.float32, torch.float64):
            t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
            calc = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=SMEARING), lr_wavelength=LAM)
            geo = [(t(cell), t(pos), torch.tensor(pairs, device=dev), t(S)) for _, cell, pos, pairs, S in systems]
            q_all = [t(s[0]) for s in systems]

            def build(cols):
                frames = [(q[:, cols].contiguous(), *g) for q, g in zip(q_all, geo)]
                nc = frames[0][0].shape[1]
                if is_step:
                    return tpa.GraphedEwaldStep(calc, *frames[0], cell_gradient=True, n_channels=nc)
                return tpa.GraphedEwaldBatch(calc, frames, cell_gradient=True, n_channels=nc)

            singles = [build(slice(c, c + 1)) for c in range(max(channels))]
            # the cells of the calls: every box breathing by up to 0.1 %, all on the device before the clock starts
            base = torch.stack([g[0] for g in geo])
            cells = [base * (1.0 + 1e-3 * float(np.sin(0.7 * i))) for i in range(reps + 4)]
            for C in channels:
                multi = build(slice(0, C))
                turn = [0]

                def next_cells():
                    turn[0] += 1
                    c = cells[turn[0] % len(cells)]
                    return c[0] if is_step else c

                def way_a():
                    c = next_cells()
                    return multi(cell=c) if is_step else multi(cells=c)

                def way_b():
                    c = next_cells()
                    for one in singles[:C]:
                        one(cell=c) if is_step else one(cells=c)

                def way_c():
                    c = next_cells()
                    for f in range(F):
                        eager_frame(calc, q_all[f][:, :C], c if is_step else c[f], geo[f][1], geo[f][2], geo[f][3])

                fns = (way_a, way_b, way_c)
                for _ in range(3):
                    way_a(), way_b()
                way_c()
                torch.cuda.synchronize()
                per_run = []
                for run in range(passes):
                    ms, n = [0.0, 0.0, 0.0], [0, 0, 0]
                    order = np.random.default_rng(run)
                    for r in range(reps):
                        for j in order.permutation(3 if r < reps_c else 2):
                            ms[j] += one_call(fns[j])
                            n[j] += 1
                    ms = [m / k for m, k in zip(ms, n)]
                    # the same cells for both: the energies must agree
                    c0 = cells[0][0] if is_step else cells[0]
                    E_a = (multi(cell=c0) if is_step else multi(cells=c0))[0].double().reshape(-1).cpu().numpy()
                    E_b = sum((one(cell=c0) if is_step else one(cells=c0))[0].double().reshape(-1).cpu().numpy() for one in singles[:C])
                    dev_E = float(np.abs(E_a - E_b).max() / max(1e-30, np.abs(E_b).max()))
                    n_atoms = sum(s[2].shape[0] for s in systems)
                    n_k = multi.n_k if is_step else sum(multi.n_k)
                    line = (f"{label:15s} C={C} atoms={n_atoms:6d} n_k={n_k:7d} {str(dtype)[6:]:8s} (a) {C} channels {ms[0]:8.3f}  (b) {C} "
                            f"single-channel {ms[1]:8.3f}  (c) eager x{n[2]} {ms[2]:9.3f}   b/a {ms[1] / ms[0]:5.2f}  c/a {ms[2] / ms[0]:7.2f}   "
                            f"max |E_a - E_b| / max |E| {dev_E:.1e}")
                    table[run].append(line)
                    print(f"[pass {run + 1}] " + line, flush=True)
                    per_run.append(ms)
                if passes == 2:
                    (a1, b1, _), (a2, b2, _) = per_run
                    spread_a, spread_b = abs(a1 - a2), abs(b1 - b2)
                    won = min(b1, b2) - max(a1, a2) > max(spread_a, spread_b)
                    summary.append(f"{label:15s} C={C} {str(dtype)[6:]:8s} b/a {b1 / a1:5.2f} / {b2 / a2:5.2f}   run-to-run spread (a) "
                                   f"{spread_a:6.3f} ms ({100 * spread_a / min(a1, a2):4.1f} %)  (b) {spread_b:6.3f} ms "
                                   f"({100 * spread_b / min(b1, b2):4.1f} %)   (a) below (b) outside the spread: {'yes' if won else 'NO'}")
                del multi
            del singles
    for run in range(passes):
        say(f"# run {run + 1}")
        say("\n".join(table[run]))
    if summary:
        say("# (a) against (b) of the same run, and the run-to-run spread of the row")
        say("\n".join(summary))
    with open(OUT, "w") as f:
        f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
