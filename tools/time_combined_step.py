"""GPU timing of GraphedCombinedStep (csrc/combined_step.hip) against what there was before and against the single-potential
steps, on the benchmark's water box (31 944 atoms, P3M 5 nodes, 64^3, fp32, the list of workloads.water_box), Coulomb + 1/r^6
with the smearings of tools/time_combined.py:

  (a) the eager combined call + backward (the differentiable primitives of analytic.py), captured by hand with torch.cuda.graph
      -- the only way before; if the capture is refused the uncaptured call is timed and the row says so
  (b) GraphedCombinedStep with and without weight_gradient
  (c) GraphedEnergyForces with Coulomb alone
  (d) GraphedEnergyForces with 1/r^6 alone

HIP events around blocks of replays; median and spread (min .. max) of the per-replay time over the blocks.

    python tools/time_combined_step.py [--quick]

--quick: few replays (for a run under rocprofv3 --kernel-trace --stats)."""
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
QUICK = "--quick" in sys.argv
BLOCKS, PER_BLOCK = (3, 5) if QUICK else (9, 100)


def blocks_ms(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PER_BLOCK):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / PER_BLOCK)
    return out


def row(label, ms):
    med = statistics.median(ms)
    print(f"{label:64s} {med:8.4f} ms  (min {min(ms):.4f} .. max {max(ms):.4f}, {len(ms)} blocks of {PER_BLOCK})", flush=True)
    return med, max(ms) - min(ms)


def main():
    w = workloads.water_box()
    dtype = torch.float32
    t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
    q, cell, S, pos = t(w.charges), t(w.cell), t(w.shifts), t(w.positions)
    idx = torch.tensor(w.pairs, device=dev)
    kw = dict(mesh_spacing=w.mesh_spacing, interpolation_nodes=5)
    members = lambda: [tpa.CoulombPotential(smearing=w.smearing), tpa.InversePowerLawPotential(exponent=6, smearing=w.smearing)]  # noqa: E731
    pot = tpa.CombinedPotential(members(), initial_weights=torch.tensor([1.0, -0.3], dtype=dtype), smearing=w.smearing).to(dev)
    calc = tpa.P3MCalculator(pot, **kw)
    print(f"# {torch.cuda.get_device_name(0)}; {w.name} N={w.n_atoms} P={w.n_pairs} mesh={w.n_mesh}^3 float32, P3M 5 nodes, "
          f"Coulomb + 1/r^6 (smearing {w.smearing}), weights (1.0, -0.3)")

    # (a) the eager route, captured by hand
    p = pos.clone().requires_grad_(True)

    def eager():
        p.grad = pot.weights.grad = None
        d = tpa.pair_distances(p, idx, cell, S)
        E = (calc(q, cell, p, idx, d) * q).sum()
        E.backward()
        return E.detach()

    e_a = float(eager())
    gw_a = pot.weights.grad.tolist()
    label = "(a) eager combined call + backward, captured by hand"
    try:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        p.grad = pot.weights.grad = None
        with torch.cuda.graph(g):
            eager()
        fn_a = g.replay
    except Exception as exc:  # the capture is not something the eager route promises
        torch.cuda.synchronize()
        print(f"# (a): capture refused ({type(exc).__name__}: {str(exc).splitlines()[0][:120]}); timing the uncaptured call")
        label, fn_a = "(a) eager combined call + backward, NOT captured", eager
    a_med, a_spread = row(label, blocks_ms(fn_a))

    # (b) the new step
    step = tpa.GraphedCombinedStep(calc, q, cell, pos, idx, S)
    E, F, gw = step()
    print(f"#   E {float(E):.6f} (eager {e_a:.6f})  dE/dw {gw.tolist()} (eager {gw_a})")
    b_med, b_spread = row("(b) GraphedCombinedStep, weight_gradient=True", blocks_ms(step))
    step_nw = tpa.GraphedCombinedStep(calc, q, cell, pos, idx, S, weight_gradient=False)
    b2_med, _ = row("(b) GraphedCombinedStep, weight_gradient=False", blocks_ms(step_nw))

    # (c), (d) the single-potential steps
    meds = []
    for tag, m in zip("cd", members()):
        single = tpa.GraphedEnergyForces(tpa.P3MCalculator(m.to(dev), **kw), q, cell, pos, idx, S)
        meds.append(row(f"({tag}) GraphedEnergyForces, {type(m).__name__} alone", blocks_ms(single))[0])
    c_med, d_med = meds
    print(f"# (a) / (b) = {a_med / b_med:.2f}   (difference {a_med - b_med:.4f} ms; spreads {a_spread:.4f} and {b_spread:.4f} ms)")
    print(f"# (b) / ((c) + (d)) = {b_med / (c_med + d_med):.2f}   (b) - (c) = {b_med - c_med:.4f} ms   "
          f"(b, no weight gradient) / ((c) + (d)) = {b2_med / (c_med + d_med):.2f}")


if __name__ == "__main__":
    main()
