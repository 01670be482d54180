"""GPU timing of ``GraphedFrameBatch(follow_cells=True)``: what it costs a frame batch to follow its cells, with
``cell_gradient=True``, in fp32 and fp64.

  (a)   a ``follow_cells`` batch replayed at a fixed cell: ``batch()``
  (a')  the same batch with new cells in every call: ``batch(cells=new)`` -- one (F, 3, 3) copy, the cells launch, the replay
  (b)   the same batch built without ``follow_cells``: ``batch()``
  (c)   the only variable-cell way before: per frame the eager sequence ``pair_distances`` -> calculator -> ``backward`` with a new
        cell tensor in every call (a host read of the cell, a new geometry and new filter tables per frame and call)
  (s)   one-frame rows only: ``GraphedEnergyForces(cell_gradient=True)`` of the same system, the fixed-cell single-system step

Rows: 1 x and 8 x the benchmark's water box (31 944 atoms, 64^3), 8 x 8 000 ions (32^3; fp64 only), 64 x 216 atoms (32^3).  The
ways are timed in turns in one process, in a new (seeded) order every round, every call ending in a synchronise, after three
warm-up calls of each; the whole table is taken twice (run 1, run 2) on the same objects so that the run-to-run spread shows.
The cells of (a') and (c) breathe by up to 0.1 % (the mesh rule keeps the mesh) and are on the device before the clock starts.

    python tools/time_frames_cells.py [--out FILE] [--root CHECKOUT --only b,s] [--quick]

``--root``: import the package from another checkout (the parent commit, say, which has (b) and (s) only: ``--only b,s``)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"a": "(a)  follow_cells, fixed cell", "a'": "(a') follow_cells, new cells", "b": "(b)  no follow_cells",
         "c": "(c)  eager, new cells", "s": "(s)  GraphedEnergyForces"}


def one_call(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def small_box(seed, tpa):
    """216 atoms on a jittered 6^3 lattice, cubic cell of 13.8, cutoff 5.5, smearing 1.1, mesh spacing 1.1: 32^3"""
    rng = np.random.default_rng(seed)
    L = 6 * 2.3
    g = (np.arange(6) + 0.5) * 2.3
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.35, 0.35, (216, 3))
    q = rng.normal(size=(216, 1))
    q -= q.mean()
    cell = L * np.eye(3)
    pairs, S, _ = tpa.neighbor_list(pos, cell, 5.5)
    return dict(charges=q, cell=cell, positions=pos, pairs=np.asarray(pairs).reshape(-1, 2), shifts=np.asarray(S).reshape(-1, 3),
                smearing=1.1, mesh_spacing=1.1, order=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,a',b,c,s")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_cells_times.txt"))
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, one run, small rows only")
    args = ap.parse_args()
    which = args.only.split(",")
    sys.path.insert(0, os.path.abspath(args.root))
    import torchpme_amd as tpa
    from torchpme_amd import workloads

    dev = torch.device("cuda", 0)
    reps, runs = (3, 1) if args.quick else (15, 2)
    as_dict = lambda w: dict(charges=w.charges, cell=w.cell, positions=w.positions, pairs=w.pairs, shifts=w.shifts,  # noqa: E731
                             smearing=w.smearing, mesh_spacing=w.mesh_spacing, order=w.order)
    rows = [("64 x 216 atoms, 32^3", lambda k: small_box(k, tpa), 64, (torch.float32, torch.float64))]
    if not args.quick:
        rows = [("1 x water box (31 944 atoms), 64^3", lambda k: as_dict(workloads.water_box(seed=1234 + k)), 1, (torch.float32, torch.float64)),
                ("8 x water box (31 944 atoms), 64^3", lambda k: as_dict(workloads.water_box(seed=1234 + k)), 8, (torch.float32, torch.float64)),
                ("8 x 8 000 ions, 32^3", lambda k: as_dict(workloads.ionic_box(seed=12 + k)), 8, (torch.float64,))] + rows
    package = "this checkout" if os.path.abspath(args.root) == ROOT else f"the checkout given by --root ({os.path.basename(os.path.abspath(args.root))})"
    out = [f"# {torch.cuda.get_device_name(0)}; package: {package}",
           f"# ms per call ending in a synchronise: mean of {reps} (min .. max), the ways in turns in a shuffled order, after 3 warm-up "
           "calls of each; P3M, cell_gradient=True", "# " + ";  ".join(NAMES[k] for k in which)]
    tables = [[] for _ in range(runs)]
    for label, make, F, dtypes in rows:
        systems = [make(k) for k in range(F)]
        s0 = systems[0]
        for dtype in dtypes:
            t = lambda a, dt=dtype: torch.tensor(np.asarray(a), device=dev, dtype=dt)  # noqa: E731
            frames = [(t(s["charges"]), t(s["cell"]), t(s["positions"]), t(s["pairs"], torch.int64), t(s["shifts"])) for s in systems]
            # a calculator per captured graph: a graph holds raw pointers into its calculator's caches
            make_calc = lambda: tpa.P3MCalculator(tpa.CoulombPotential(smearing=s0["smearing"]), mesh_spacing=s0["mesh_spacing"],  # noqa: E731
                                                  interpolation_nodes=s0["order"]).to(dev)
            base = torch.stack([f[1] for f in frames])
            cells = [base * (1.0 + 1e-3 * float(np.sin(0.7 * i))) for i in range(reps + 4)]
            turn = [0]
            fns, keep = {}, []
            if "a" in which or "a'" in which:
                follow = tpa.GraphedFrameBatch(make_calc(), frames, cell_gradient=True, follow_cells=True)
                keep.append(follow)
                if "a" in which:
                    fns["a"] = follow

                def with_cells():
                    turn[0] += 1
                    follow(cells=cells[turn[0] % len(cells)])

                if "a'" in which:
                    fns["a'"] = with_cells
            if "b" in which:
                fixed = tpa.GraphedFrameBatch(make_calc(), frames, cell_gradient=True)
                keep.append(fixed)
                fns["b"] = fixed
            if "c" in which:
                eager_calc = make_calc()
                leaves = [f[2].clone().requires_grad_(True) for f in frames]

                def eager():
                    turn[0] += 1
                    c = cells[turn[0] % len(cells)]
                    for f, (q, _, _, pairs, shifts) in enumerate(frames):
                        cell = c[f].clone().requires_grad_(True)  # a new cell tensor: what a loop over structures or NPT hands over
                        leaves[f].grad = None
                        d = tpa.pair_distances(leaves[f], pairs, cell, shifts)
                        V = eager_calc(q, cell, leaves[f], pairs, d)
                        (V * q).sum().backward()

                fns["c"] = eager
            if "s" in which and F == 1:
                single = tpa.GraphedEnergyForces(make_calc(), *frames[0], cell_gradient=True)
                keep.append(single)
                fns["s"] = single
            keys = list(fns)
            for _ in range(3):
                for k in keys:
                    fns[k]()
            torch.cuda.synchronize()
            for run in range(runs):
                ms = {k: [] for k in keys}
                order = np.random.default_rng(run)
                for _ in range(reps):
                    for j in order.permutation(len(keys)):
                        ms[keys[j]].append(one_call(fns[keys[j]]))
                mean = {k: float(np.mean(v)) for k, v in ms.items()}
                head = f"## {label}, {str(dtype)[6:]}"
                if "a'" in fns and "b" in fns:  # the same numbers from both ways, compared AFTER the timed calls
                    follow(cells=base)
                    fixed()
                    torch.cuda.synchronize()
                    dE = float(((follow.energies - fixed.energies).abs() / fixed.energies.abs()).max())
                    dC = float((follow.cell_grads - fixed.cell_grads).abs().max() / fixed.cell_grads.abs().max())
                    head += f"   (E of (a') at the cells of (b): {dE:.1e} relative, dE/dcell {dC:.1e} of the largest; frames with a status other than 0: {int((follow.status != 0).sum())})"
                tables[run].append(head)
                for k in keys:
                    tables[run].append(f"{NAMES[k]:<32} {mean[k]:9.4f}   ({min(ms[k]):.4f} .. {max(ms[k]):.4f})")
                notes, new = [], "a'"
                if "a" in fns and "b" in fns:
                    spread = max(max(ms["b"]) - min(ms["b"]), max(ms["a"]) - min(ms["a"]))
                    inside = abs(mean["a"] - mean["b"]) <= spread
                    notes.append(f"(a) - (b) = {1e3 * (mean['a'] - mean['b']):+.1f} us ({'within' if inside else 'OUTSIDE'} the spread of "
                                 f"{1e3 * spread:.1f} us)")
                if "a" in fns and new in fns:
                    notes.append(f"(a') - (a) = {1e3 * (mean[new] - mean['a']):+.1f} us: the copy and the cells launch")
                if "c" in fns and new in fns:
                    notes.append(f"(c) / (a') = {mean['c'] / mean[new]:.1f}")
                if "s" in fns and "a" in fns:
                    notes.append(f"(a) - (s) = {1e3 * (mean['a'] - mean['s']):+.1f} us: the batch of one beside the single-system step")
                if notes:
                    tables[run].append("    " + ";   ".join(notes))
                print("\n".join(tables[run][-(len(keys) + 1 + bool(notes)):]), flush=True)
            del fns, keep
    for run in range(runs):
        out.append(f"# run {run + 1}")
        out += tables[run]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(f"written: {args.out}")


if __name__ == "__main__":
    main()
