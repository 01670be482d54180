"""GPU timing of a 2-D periodic (slab) energy + forces step: the benchmark's water box (31 944 atoms) in a cell doubled along z
(a vacuum gap of one box height), mesh 64 x 64 x 128, P3M with 5 nodes, fp32, ``periodic = (True, True, False)``.

  (a) the eager slab call -- calculator with ``periodic=``, ``weighted_sum``, ``backward()`` -- with the gather tail switched off
      (``ops.TAIL_FUSION = False``: the slab term in launches of its own behind the step, the general backward; the only way
      before the term entered the tail), captured by hand with ``torch.cuda.graph`` and replayed;
  (b) ``GraphedEnergyForces(..., slab_correction=True)``;
  (c) the same object with ``slab_correction=False`` (the same neighbour list, no slab term),
(b) and (c) in the explicit-list form and in the ``neighbors=`` form with live bins.  The three are timed in turns, ROUNDS rounds of
REPLAYS replays each; the table gives the median over the rounds and their spread, and (b) - (c), (a) / (b).

    python tools/time_slab.py          # writes profiles/slab_times.txt
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402
from torchpme_amd import ops, workloads  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPLAYS = 7, 300
PERIODIC = (True, True, False)


def replay_ms(graph):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPLAYS):
        graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPLAYS


def hand_captured(calc, q, cell, pos, pairs, shifts):
    """(a): what a user could do before -- returns the graph and the tensors it writes."""
    per = torch.tensor(PERIODIC, device=dev)
    pos = pos.clone().requires_grad_(True)
    out = {}

    def evaluate():
        pos.grad = None
        V = calc(q, cell, pos, pairs, tpa.pair_distances(pos, pairs, cell, shifts), periodic=per)
        E = tpa.weighted_sum(V, q)
        E.backward()
        out["E"], out["F"] = E.detach(), pos.grad

    tail_fusion, ops.TAIL_FUSION = ops.TAIL_FUSION, False
    try:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                evaluate()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            evaluate()
    finally:
        ops.TAIL_FUSION = tail_fusion
    # what the graph reads lives in caches (pair topology and its entry streams, the calculator's filter table): pin it, as
    # GraphedEnergyForces does for its own graph
    topo = ops.get_topology(pairs, pos.shape[0])
    out["keepalive"] = [topo, getattr(calc, "_cache", None)] + [getattr(topo, k, None) for k in
                                                               ("row_ptr", "entries", "_ent32", "_ent_sh", "_packed", "_pair_sh")]
    return graph, out


def main():
    w = workloads.water_box()
    cell = w.cell.copy()
    cell[2, 2] *= 2.0
    pairs, shifts, _ = tpa.neighbor_list_device(torch.tensor(w.positions, device=dev), torch.tensor(cell, device=dev), w.cutoff,
                                                periodic=PERIODIC)
    dtype = torch.float32
    t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
    q, cl, pos, sh = t(w.charges), t(cell), t(w.positions), shifts.to(dtype)
    # a calculator per captured graph: a graph holds raw pointers into its calculator's caches (filter table, plan)
    make_calc = lambda: tpa.P3MCalculator(tpa.CoulombPotential(smearing=w.smearing), mesh_spacing=w.mesh_spacing,  # noqa: E731
                                          interpolation_nodes=w.order).to(dev)
    lines = [f"# {w.n_atoms} atoms, {len(pairs)} pairs, cell {cell[0, 0]:.1f} x {cell[1, 1]:.1f} x {cell[2, 2]:.1f}, fp32, P3M 5 nodes; "
             f"ms per step, median of {ROUNDS} rounds of {REPLAYS} replays (min .. max)"]
    # every object is built first and (a) is captured last: its graph reads buffers that live in the package's caches, and
    # nothing is constructed -- so nothing is evicted -- between its capture and the last timed replay
    forms = {}
    for form in ("explicit lists", "neighbors= (live bins)"):
        kw = dict(neighbor_indices=pairs, neighbor_shifts=sh) if form == "explicit lists" else dict(neighbors=w.cutoff)
        step_b = tpa.GraphedEnergyForces(make_calc(), q, cl, pos, periodic=PERIODIC, slab_correction=True, **kw)
        step_c = tpa.GraphedEnergyForces(make_calc(), q, cl, pos, periodic=PERIODIC, slab_correction=False, **kw)
        if form != "explicit lists" and step_b._live is None:
            form += " -> binned step"
        forms[form] = (step_b, step_c)
    graph_a, out_a = hand_captured(make_calc(), q, cl, pos, pairs, sh)
    for form, (step_b, step_c) in forms.items():
        ms = {"a": [], "b": [], "c": []}
        for _ in range(ROUNDS):
            ms["a"].append(replay_ms(graph_a))
            ms["b"].append(replay_ms(step_b.graph))
            ms["c"].append(replay_ms(step_c.graph))
        med = {k: statistics.median(v) for k, v in ms.items()}
        # (a) and (b) evaluate the same system: compared AFTER the timed replays
        graph_a.replay()
        Eb, Fb = step_b()
        torch.cuda.synchronize()
        dE = abs(float(Eb) - float(out_a["E"])) / abs(float(out_a["E"]))
        dF = float((Fb + out_a["F"]).abs().max() / out_a["F"].abs().max())
        valid = dE < 1e-5 and dF < 1e-4
        lines.append(f"## {form}   (E of (b) against (a): {dE:.1e} relative, F: {dF:.1e} of the largest"
                     f"{'' if valid else ' -- (a) DISAGREES: its time is not a measurement'})")
        for key, label in (("a", "(a) eager slab call, hand-captured, tail off"), ("b", "(b) GraphedEnergyForces(slab_correction=True)"),
                           ("c", "(c) GraphedEnergyForces(slab_correction=False)")):
            lines.append(f"{label:<48} {med[key]:.4f}   ({min(ms[key]):.4f} .. {max(ms[key]):.4f})")
        lines.append(f"(b) - (c) = {1e3 * (med['b'] - med['c']):.1f} us     (a) / (b) = {med['a'] / med['b']:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "slab_times.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
