"""GPU timing of 2-D periodic (slab) frames in a frame batch: eight frames of the benchmark's water box (31 944 atoms each) in a
cell doubled along z (a vacuum gap of one box height, as tools/time_slab.py), mesh 64 x 64 x 128, P3M with 5 nodes, fp32,
``periodic = (True, True, False)``.  The frames share one neighbour list and differ in their positions by 1e-3 (far below the
skin a list would carry; the times do not depend on it).

  (a) ``GraphedFrameBatch(..., periodic=, slab_correction=True)``: the slab batch;
  (b) the same batch without the two keywords (no slab term);
  (c) eight ``GraphedEnergyForces(..., slab_correction=True)``, one per frame, replayed one after the other,
each without and with ``charge_gradient=True, cell_gradient=True``.  The three are timed in turns, ROUNDS rounds of REPLAYS
replays each; the table gives the median over the rounds and their spread, (a) - (b) and (c) / (a).

    python tools/time_slab_frames.py [output file]         # default: profiles/slab_frames_times.txt
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402
from torchpme_amd import workloads  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPLAYS, FRAMES = 5, 60, 8
PERIODIC = (True, True, False)


def replay_ms(graphs):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPLAYS):
        for g in graphs:
            g.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPLAYS


def main():
    w = workloads.water_box()
    cell = w.cell.copy()
    cell[2, 2] *= 2.0
    pairs, shifts, _ = tpa.neighbor_list_device(torch.tensor(w.positions, device=dev), torch.tensor(cell, device=dev), w.cutoff,
                                                periodic=PERIODIC)
    dtype = torch.float32
    t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
    q, cl, sh = t(w.charges), t(cell), shifts.to(dtype)
    rng = np.random.default_rng(1)
    frames = [(q, cl, t(w.positions + 1e-3 * rng.uniform(-1, 1, w.positions.shape)), pairs, sh) for _ in range(FRAMES)]
    # a calculator per captured graph: a graph holds raw pointers into its calculator's caches (filter table, plan)
    make_calc = lambda: tpa.P3MCalculator(tpa.CoulombPotential(smearing=w.smearing), mesh_spacing=w.mesh_spacing,  # noqa: E731
                                          interpolation_nodes=w.order).to(dev)
    lines = [f"# {FRAMES} frames of {w.n_atoms} atoms, {len(pairs)} pairs each, cell {cell[0, 0]:.1f} x {cell[1, 1]:.1f} x "
             f"{cell[2, 2]:.1f}, fp32, P3M 5 nodes; ms per evaluation of all frames, median of {ROUNDS} rounds of {REPLAYS} replays "
             "(min .. max)"]
    for flags in (False, True):
        kw = dict(charge_gradient=flags, cell_gradient=flags)
        batch_a = tpa.GraphedFrameBatch(make_calc(), frames, periodic=PERIODIC, slab_correction=True, **kw)
        batch_b = tpa.GraphedFrameBatch(make_calc(), frames, **kw)
        steps_c = [tpa.GraphedEnergyForces(make_calc(), f[0], f[1], f[2], f[3], f[4], periodic=PERIODIC, slab_correction=True, **kw)
                   for f in frames]
        ms = {"a": [], "b": [], "c": []}
        for _ in range(ROUNDS):
            ms["a"].append(replay_ms([batch_a.graph]))
            ms["b"].append(replay_ms([batch_b.graph]))
            ms["c"].append(replay_ms([s.graph for s in steps_c]))
        med = {k: statistics.median(v) for k, v in ms.items()}
        # (a) and (c) evaluate the same systems: compared AFTER the timed replays
        Ea, Fa = batch_a()[:2]
        dE = dF = 0.0
        for k, s in enumerate(steps_c):
            Ec, Fc = s()[:2]
            dE = max(dE, abs(float(Ea[k]) - float(Ec)) / abs(float(Ec)))
            dF = max(dF, float((Fa[k] - Fc).abs().max() / Fc.abs().max()))
        valid = dE < 1e-5 and dF < 1e-4
        lines.append(f"## {'E, F, dE/dq, dE/dcell' if flags else 'E, F'}   (E of (a) against (c): {dE:.1e} relative, F: {dF:.1e} of the "
                     f"largest{'' if valid else ' -- (a) DISAGREES: its time is not a measurement'})")
        for key, label in (("a", "(a) GraphedFrameBatch(slab_correction=True)"), ("b", "(b) GraphedFrameBatch()"),
                           ("c", f"(c) {FRAMES} x GraphedEnergyForces(slab_correction=True)")):
            lines.append(f"{label:<52} {med[key]:.4f}   ({min(ms[key]):.4f} .. {max(ms[key]):.4f})")
        lines.append(f"(a) - (b) = {1e3 * (med['a'] - med['b']):.1f} us     (c) / (a) = {med['c'] / med['a']:.2f}")
        del batch_a, batch_b, steps_c
    text = "\n".join(lines) + "\n"
    print(text, end="")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "slab_frames_times.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
