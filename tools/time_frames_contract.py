"""GPU timing of the first-order contract of a frame batch: E, F, dE/dq and dE/dcell of eight frames from one replay.

Workloads (boxes of ``workloads.py``, different seeds per frame): 8 x the cfg3 water box in fp32 (31 944 atoms, 64^3 mesh, P3M 5
nodes) and cfg4's one-GPU share, 8 x 8000 ions in fp64 (32^3 mesh).  Per workload, ms per evaluation of all eight frames:

  (a) ``GraphedFrameBatch`` without flags (energies + forces: the step as it was);
  (b) ``GraphedFrameBatch(charge_gradient=True, cell_gradient=True)``;
  (c) eight ``GraphedEnergyForces(charge_gradient=True, cell_gradient=True)`` replayed back to back on one stream -- the only way to
      the same results without (b).

The three are timed in turns, ROUNDS rounds of REPLAYS evaluations each; the table gives the median over the rounds and their
spread (max - min), then (b) - (a), the price of the contract, and whether (b) is below (c) by more than twice (c)'s spread.

    python tools/time_frames_contract.py                     # writes profiles/frames_contract_times.txt
    python tools/time_frames_contract.py --only a,c --root DIR --out FILE
``--root``: the checkout to import ``torchpme_amd`` from (default: this one) -- an older build of the package in the same job, for
(a) and (c), which need nothing new; ``--only``: which of the three to build and time.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, REPLAYS, FRAMES = 3, 200, 8


def ms_per_eval(replay):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPLAYS):
        replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPLAYS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_contract_times.txt"))
    args = ap.parse_args()
    which = args.only.split(",")
    sys.path.insert(0, os.path.abspath(args.root))
    import torchpme_amd as tpa
    from torchpme_amd import workloads

    dev = torch.device("cuda", 0)
    lines = [f"# package: {os.path.dirname(tpa.__file__)}",
             f"# ms per evaluation of {FRAMES} frames; median of {ROUNDS} rounds of {REPLAYS} evaluations, the variants in turns (spread = max - min)"]
    for label, make in (("8 x cfg3 water (31 944 atoms, 64^3, P3M 5 nodes, fp32)", lambda k: workloads.water_box(seed=1234 + k)),
                        ("8 x cfg4 ions (8000 atoms, 32^3, fp64)", lambda k: workloads.ionic_box(seed=12 + k))):
        ws = [make(k) for k in range(FRAMES)]
        w = ws[0]
        dtype = torch.float32 if w.dtype == "f32" else torch.float64
        t = lambda a, dt=dtype: torch.tensor(np.asarray(a), device=dev, dtype=dt)  # noqa: E731
        frames = [(t(x.charges), t(x.cell), t(x.positions), t(x.pairs, torch.int64), t(x.shifts)) for x in ws]
        Calc = tpa.P3MCalculator if w.scheme == "P3M" else tpa.PMECalculator
        # a calculator per captured graph: a graph holds raw pointers into its calculator's caches
        make_calc = lambda: Calc(tpa.CoulombPotential(smearing=w.smearing), mesh_spacing=w.mesh_spacing,  # noqa: E731
                                 interpolation_nodes=w.order).to(dev)
        run = {}
        if "a" in which:
            plain = tpa.GraphedFrameBatch(make_calc(), frames)
            run["a"] = plain.graph.replay
        if "b" in which:
            full = tpa.GraphedFrameBatch(make_calc(), frames, charge_gradient=True, cell_gradient=True)
            run["b"] = full.graph.replay
        if "c" in which:
            singles = [tpa.GraphedEnergyForces(make_calc(), *f, charge_gradient=True, cell_gradient=True) for f in frames]
            assert all(s._fused_contract for s in singles)

            def run_c():
                for s in singles:
                    s.graph.replay()

            run["c"] = run_c
        ms = {k: [] for k in run}
        for _ in range(ROUNDS):
            for k, fn in run.items():
                ms[k].append(ms_per_eval(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        lines.append(f"## {label}")
        if "b" in run and "c" in run:  # the same numbers from both, compared AFTER the timed replays
            E, F, dq, dc = full()
            worst = 0.0
            for k, s in enumerate(singles):
                e1, f1, q1, c1 = s()
                torch.cuda.synchronize()
                for x, y in ((E[k], e1), (F[k], f1), (dq[k], q1), (dc[k], c1)):
                    worst = max(worst, float((x - y).abs().max() / y.abs().max()))
            lines.append(f"largest relative difference of E, F, dE/dq, dE/dcell between (b) and (c): {worst:.1e}")
        names = {"a": "(a) GraphedFrameBatch, no flags", "b": "(b) GraphedFrameBatch, charge_gradient + cell_gradient",
                 "c": "(c) 8 x GraphedEnergyForces, both flags, back to back"}
        for k in run:
            lines.append(f"{names[k]:<58} {med[k]:.4f}   spread {spread[k]:.4f}   ({'  '.join(f'{x:.4f}' for x in ms[k])})")
        if "a" in run and "b" in run:
            lines.append(f"(b) - (a) = {1e3 * (med['b'] - med['a']):.1f} us: the price of dE/dq and dE/dcell for {FRAMES} frames")
        if "b" in run and "c" in run:
            margin = 2 * spread["c"]
            lines.append(f"(c) - (b) = {1e3 * (med['c'] - med['b']):.1f} us, twice the spread of (c) = {1e3 * margin:.1f} us: "
                         f"(b) is {'below' if med['c'] - med['b'] > margin else 'NOT below'} (c) by the margin;  (c) / (b) = {med['c'] / med['b']:.2f}")
        del run
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
