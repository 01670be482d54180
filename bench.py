"""Benchmark of the PME/P3M hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload water|ionic|dispersion] [--preset cfg2|cfg3|cfg4|cfg5]
                    [--dump-outputs DIR] [--full]

One *step* = one energy + forces evaluation of one frame (or ``--frames-per-gpu`` frames) per GPU, the reference's
protocol: ``d = pair_distances(...)`` -> ``V = calculator(...)`` -> ``E = sum(q*V)`` ->
``E.backward()`` (forces = -dE/dpositions).  Inputs are resident in HBM before the timed region.

Ranks.  ``--gpus N`` with N > 1 and no ``WORLD_SIZE`` in the environment re-executes this script under
``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`` (one process per GPU, backend
``nccl`` = RCCL); launched by an external ``torch.distributed.run`` it reads RANK / LOCAL_RANK / WORLD_SIZE as usual.
Every rank owns independent frames (weak scaling, no intra-cell decomposition).  With more than one rank the frame
energies are exchanged with an all_gather AFTER EVERY EVALUATION, inside the timed loop (``--exchange per-step``, the default:
what ``farm.farm_energies`` does; ``pipelined`` overlaps it with the next evaluation; ``final`` is round 2's single exchange
after the last step).  Every rank binds itself to a disjoint set of host cores on its GPU's NUMA node.  The time is the MAX
over ranks; ``weak_efficiency`` = rank 0's time with the other ranks idle / the time with all ranks busy, same invocation.

Timing protocol: >= ``--prewarm-ms`` of untimed replays (clock ramp), the W warm-up steps, then ``--blocks`` blocks of EXACTLY K
steps, each bracketed by barrier + synchronize: ONE block by default, so that K is the number of timed steps (five with
``--full``).  ``ms_per_step`` / ``value`` are the MEDIAN block's (the contract's one timed region; round 4 reported the first
block, which was the fastest one in every run); ``ms_per_step_first_block`` is the first.

A plain run does only that: set up, warm up, time, write the outputs (``--dump-outputs DIR``: rank 0's frame energies and
forces of the last timed step as ``DIR/energy.npy`` / ``DIR/forces.npy``, in the workload's precision) and print the line.
Everything else the benchmark measures or checks runs with ``--full`` only: with more than one rank the one-rank reference
block of ``weak_efficiency`` and one timed block per other exchange protocol, and on rank 0 the blocks below.

Rank 0 prints ONE JSON line: metric = atom-steps/s over all ranks, plus (``--full``)
  roofline     -- HBM roofline of the dominant kernel, timed live with HIP events on the launch stream
  roofline_valu -- the same launch against the VALU issue rate (pair-row instruction-lanes / peak)
  cpu_baseline -- the PyTorch-CPU oracle ("port" of the reference's ATen op sequence) timed on this host's cores
                  on a bounded sample, swept over thread counts (rank 0, N = 1 only)
  drop_in      -- the same frame through the reference's own call sequence, eager, no graph, no package-specific
                  helpers: caller-made distances -> calculator(...) -> (q*V).sum().backward(); ``cold_list_ms`` = the same
                  with a NEW neighbor_indices tensor every call (what the reference's users do)
  list_refresh -- the neighbour list on the device: reference-format build, the in-place refresh of the row stream the pair
                  kernels read (one graph replay), the first step after it, and ``md_amortized_ms_per_step`` = a loop of
                  steps with a refresh every 10 / 20 steps
"""

from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable

PRESETS = {
    # BASELINE.json configs[1..4]
    "cfg2": dict(workload="ionic", frames_per_gpu=1),
    "cfg3": dict(workload="water", frames_per_gpu=1),
    "cfg4": dict(workload="ionic", frames_per_gpu=8),  # 64 frames of 8 000 atoms on 8 GPUs = 8 per rank
    "cfg5": dict(workload="dispersion", frames_per_gpu=1),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="water", choices=["water", "ionic", "dispersion"])
    ap.add_argument("--preset", default=None, choices=sorted(PRESETS),
                    help="BASELINE.json configuration: sets --workload / --frames-per-gpu (cfg4 = ionic, 8 frames per GPU)")
    ap.add_argument("--frame-batch", default="one-launch", choices=["one-launch", "streams"],
                    help="with several frames per GPU: every kernel of the pipeline launched once for all frames "
                         "(GraphedFrameBatch), or one HIP graph per frame replayed on its own stream")
    ap.add_argument("--frames-per-gpu", type=int, default=1,
                    help="independent frames evaluated per rank and step (BASELINE.json configs[3]: --preset cfg4)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-drop-in", action="store_true")
    ap.add_argument("--no-frames-block", action="store_true", help="skip the `frames` block (2 / 4 / 8 frames in flight on one GPU)")
    ap.add_argument("--no-second-order", action="store_true",
                    help="skip the `second_order` block (one force-loss training step through the analytic route)")
    ap.add_argument("--no-contract", action="store_true",
                    help="skip the `contract` block (E+F, +dE/dq, +dE/dcell as graphs and eagerly; the TuningTimings protocol)")
    ap.add_argument("--store-distances", action="store_true",
                    help="also store the pair distances the fused pair kernel forms (a by-product nobody reads in an energy + "
                         "forces step; off: they stay in registers)")
    ap.add_argument("--exchange", default=None, choices=["log", "per-step", "pipelined", "final", "in-graph"],
                    help="all-gather of the frame energies.  log (default with more than one rank; SURVEY 8(e): ONE collective): "
                         "every step appends its energies to a device-resident log (last node of the step's HIP graph) and the "
                         "whole K x frames log is all-gathered once per timed region; per-step: a collective after every "
                         "evaluation, on the compute stream; pipelined: the same, overlapped with the next evaluation; final: "
                         "only the LAST step's energies, once; in-graph: the per-step collective captured into the step's graph")
    ap.add_argument("--sweep-orders", action="store_true",
                    help="instead of the bench line: the order / scheme sweep of the graph-replayed step on the headline box "
                         "(tools/r06/order_sweep.py: P3M 3-5, Lagrange 4, 6, 7 x fp32 / fp64, ms per step + scratch per kernel)")
    ap.add_argument("--no-exchange-sweep", action="store_true",
                    help="with several ranks: skip the one timed block per OTHER exchange protocol (parallelism.other_exchange_modes_ms_per_step)")
    ap.add_argument("--exchange-sweep", default="basic", choices=["basic", "full"],
                    help="which other protocols get their one timed block: basic = none, per-step, final (blocking collectives on the "
                         "compute stream, the primitive the log's own exchange uses); full = also log / pipelined (asynchronous)")
    ap.add_argument("--blocks", type=int, default=None,
                    help="timed blocks of --steps steps (the median block is the reported value); default 1, with --full 5")
    ap.add_argument("--full", action="store_true",
                    help="also run everything the headline figure does not need: the secondary blocks of rank 0 (instrumented "
                         "per-kernel pass, rooflines, accuracy, list refresh, drop-in, contract, frames, second order, CPU "
                         "baseline, host), and with several ranks weak_efficiency and the other exchange protocols")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the timed path computed in its last step (rank 0's frame energies "
                         "and forces) as DIR/<name>.npy")
    ap.add_argument("--prewarm-ms", type=float, default=30.0, help="untimed replays before the warm-up steps (clock ramp)")
    ap.add_argument("--no-list-refresh", action="store_true")
    ap.add_argument("--neighbors", default="list", choices=["list", "stream"],
                    help="list: the step reads the transposed (P,2) list of the workload; stream: rows written by the device "
                         "neighbour list (GraphedEnergyForces(neighbors=cutoff))")
    ap.add_argument("--launch", default="graph", choices=["graph", "eager"],
                    help="graph: replay the captured step (HIP graph); eager: launch every kernel from Python")
    # test hook (tests/test_bench_launch.py): the launch / rendezvous / timing / reporting path on CPU ranks with the gloo
    # backend and a trivial stand-in for the frame evaluation.  Its JSON line says so and is never a measurement.
    ap.add_argument("--stub-evaluator", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.preset is not None:
        for k, v in PRESETS[args.preset].items():
            setattr(args, k, v)
    if args.blocks is None:
        args.blocks = 5 if args.full else 1
    return args


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def respawn_under_torchrun(args, argv) -> int:
    """``--gpus N`` (N > 1) outside a torch.distributed launcher: start N ranks of this script, one per GPU."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def _cpulist(text: str):
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


def bind_rank_to_cores(local_rank: int, local_world: int, device_index):
    """Pin this rank to a disjoint slice of host cores, on its GPU's NUMA node when sysfs tells which one that is (eight
    Python ranks replaying 70 us graphs are host-sensitive: without this they migrate across sockets).  Returns a short
    description for the JSON line; never fails the run."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
        node, cores = None, None
        if device_index is not None:
            try:
                props = torch.cuda.get_device_properties(device_index)
                bdf = f"{props.pci_domain_id:04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}.0"
                node = int(open(f"/sys/bus/pci/devices/{bdf}/numa_node").read())
                if node >= 0:
                    cores = [c for c in _cpulist(open(f"/sys/devices/system/node/node{node}/cpulist").read()) if c in allowed]
            except Exception:
                node, cores = None, None
        if cores:
            # the ranks whose GPUs share this node split its cores: without knowing the others' nodes, use the rank's position
            # among `local_world` ranks spread evenly over the nodes
            n_nodes = max(1, len([d for d in os.listdir("/sys/devices/system/node") if d.startswith("node")]))
            share = max(1, local_world // n_nodes)
            k = local_rank % share
            per = max(1, len(cores) // share)
            mine = cores[k * per:(k + 1) * per] or cores
        else:
            per = max(1, len(allowed) // max(1, local_world))
            mine = allowed[local_rank * per:(local_rank + 1) * per] or allowed
        os.sched_setaffinity(0, mine)
        return {"numa_node": node, "cores": f"{mine[0]}-{mine[-1]}", "n_cores": len(mine)}
    except Exception as exc:  # not fatal: report and go on unbound
        return {"error": f"{type(exc).__name__}: {exc}"}


# ----------------------------------------------------------------------------------------------------------------------
def make_workload(name: str, seed_offset: int):
    from torchpme_amd import workloads

    if name == "water":
        return workloads.water_box(seed=1234 + seed_offset)
    if name == "ionic":
        return workloads.ionic_box(seed=12 + seed_offset)
    if name == "dispersion":
        return workloads.dispersion_box(seed=8 + seed_offset)
    raise ValueError(name)


class Frame:
    """Device-resident inputs of one frame + its calculator."""

    def __init__(self, w, device, store_distances: bool = False):
        import torchpme_amd as tpa

        self.w = w
        self.store_distances = store_distances
        dt = torch.float32 if w.dtype == "f32" else torch.float64
        self.dtype = dt
        self.pos = torch.tensor(w.positions, dtype=dt, device=device, requires_grad=True)
        self.q = torch.tensor(w.charges, dtype=dt, device=device)
        self.cell = torch.tensor(w.cell, dtype=dt, device=device)
        self.pairs = torch.tensor(w.pairs, dtype=torch.int64, device=device)
        self.shifts = torch.tensor(w.shifts, dtype=dt, device=device)
        self.minus_one = torch.tensor(-1.0, dtype=dt, device=device)  # backward seed: pos.grad = -dE/dr = forces
        pot = (tpa.CoulombPotential(smearing=w.smearing) if w.exponent == 1
               else tpa.InversePowerLawPotential(exponent=w.exponent, smearing=w.smearing))
        Calc = tpa.P3MCalculator if w.scheme == "P3M" else tpa.PMECalculator
        self.calc = Calc(pot, mesh_spacing=w.mesh_spacing, interpolation_nodes=w.order)
        self._tpa = tpa

    def step(self):
        """The package's fast eager form of the step (distances formed inside the pair kernel + weighted_sum)."""
        tpa = self._tpa
        self.pos.grad = None
        # "virtual": the distance tensor only connects the calculator to the positions in the autograd graph -- the fused
        # distance + pair kernel forms the distances in registers and nothing stores them (store_distances: by-product write)
        d = tpa.pair_distances(self.pos, self.pairs, self.cell, self.shifts,
                               deferred=True if self.store_distances else "virtual")
        self.distances = d.detach() if self.store_distances else None
        # the backward pass below is seeded with minus_one: promised to the forward, whose gather then writes the forces
        with tpa.ops.seed_promise(self.minus_one):
            V = self.calc(self.q, self.cell, self.pos, self.pairs, d)
        E = tpa.weighted_sum(V, self.q)
        E.backward(self.minus_one)
        return E.detach(), self.pos.grad

    def step_cold_list(self, mode: str = "list"):
        """The reference's usage with a NEW neighbour list every call (``examples/02-neighbor-lists-usage.py:97-164``).
        ``list``: fresh ``neighbor_indices`` / shifts tensors (same values: the cost is the per-list work of the row kernels
        -- the radix-sort transposition and the entry streams); ``stream``: the device neighbour list rebuilt in place
        (``NeighborStream.update``) and its handles passed through the same calculator call."""
        self.pos.grad = None
        if mode == "stream":
            if getattr(self, "_stream", None) is None:
                self._stream = self._tpa.NeighborStream(self.pos, self.cell, self.w.cutoff)
            nl = self._stream.update()
            pairs, d = nl.indices, nl.distances(self.pos, self.cell)
        else:
            pairs, shifts = self.pairs.clone(), self.shifts.clone()
            d = self._tpa.pair_distances(self.pos, pairs, self.cell, shifts)
        V = self.calc(self.q, self.cell, self.pos, pairs, d)
        E = (self.q * V).sum()
        E.backward()
        return E.detach(), -self.pos.grad

    def step_reference_protocol(self, distances: str = "helper"):
        """The reference's call sequence with nothing package-specific but the distance helper (the counterpart of the
        caller-side ``compute_distances``, tests/helpers.py:278-304): eager, no graph, no ``weighted_sum``, no deferral.
        ``distances="torch"`` forms the distances with plain tensor ops instead, exactly as the reference's helper does."""
        self.pos.grad = None
        if distances == "torch":
            vec = self.pos[self.pairs[:, 1]] - self.pos[self.pairs[:, 0]] + self.shifts @ self.cell
            d = torch.linalg.norm(vec, dim=1)
        else:
            d = self._tpa.pair_distances(self.pos, self.pairs, self.cell, self.shifts)
        V = self.calc(self.q, self.cell, self.pos, self.pairs, d)
        E = (self.q * V).sum()
        E.backward()
        return E.detach(), -self.pos.grad


class StubFrame:
    """Stand-in used by the CPU launch test (--stub-evaluator): no HIP, no oracle -- a dot product per 'frame'."""

    class _W:
        name, dtype, n_atoms, n_pairs, n_mesh, cutoff, scheme, order, exponent = "stub", "f64", 1000, 0, 0, 0.0, "-", 0, 1

    def __init__(self, seed, device):
        g = torch.Generator().manual_seed(seed)
        self.w = self._W()
        self.dtype = torch.float64
        self.x = torch.rand((self.w.n_atoms,), generator=g, dtype=torch.float64).to(device)

    def step(self):
        return (self.x * self.x).sum(), None


# VALU issue peak: 256 CUs x 4 SIMDs x 16 lanes, one instruction-lane per clock at the 2.4 GHz peak engine clock (a v_pk_*
# instruction counts once, as it issues once) -- /opt/skills/guides/MI355X_MICROARCH.md's CU model
VALU_PEAK_TLANEOPS = 256 * 4 * 16 * 2.4e9 / 1e12
# hot-loop ISA counts of the pair-row bodies, per entry (a loop iteration handles two): (VALU instructions, of which quarter-rate),
# counted in the disassembly of spread_rows_kernel<5, T, P, true> at the end of round 3 (llvm-objdump; loop control and masks
# included, the fp64 body's rare y >= 6.5 branch excluded; 44.5 and 43.5 for the fp32 bodies while their entry loads were waterfall loops)
# Round 4: the fp32 bodies run an unmasked main loop (33.5 per entry: 65 + 2 per iteration) for the iterations in which every
# lane has two full entries -- eight of a row's ten at cfg3 -- and the masked one (38.5) for the tails: 34.5 on average.
# End of round 4: loop bookkeeping in scalar registers, indexed record loads, z / d^2 chains kept scalar -- 54 (1/r) and 52 (1/r^6)
# vector instructions per unmasked iteration, 63 / 61 per masked one (hipcc -S, spread_rows_kernel<5, float, P, true, false>):
# 27.9 / 26.9 per entry at eight unmasked iterations in ten; the fp64 body 212 -> 203 per iteration of its masked loop.
PAIR_BODY_VALU = {("f32", 1): (27.9, 3), ("f32", 6): (26.9, 2), ("f64", 1): (87, 1)}
def sq_counters_of(workload: str, launched_kernel_family: str):
    """What the hardware counters say about the dominant launch (VALUBusy, vector instructions, waiting share): the committed
    figures of ONE rocprofv3 --pmc pass of this command (profiles/sq_counters.json, generated by tools/sq_to_json.py from the
    pass named in its `source`) -- bench.py cannot profile itself.  Refused, loudly, when the kernel the counters belong to is
    not the kernel family this run launches (round 5 quoted round 4's spread_rows_kernel counters next to plane_rows_kernel)."""
    path = os.path.join(ROOT, "profiles", "sq_counters.json")
    if not os.path.exists(path):
        return {"error": "profiles/sq_counters.json missing (tools/sq_to_json.py)"}
    entry = json.load(open(path)).get("workloads", {}).get(workload)
    if entry is None:
        return None
    family = entry["kernel"].split("<")[0]
    if family != launched_kernel_family:
        return {"error": f"STALE COUNTERS: profiles/sq_counters.json holds {entry['kernel']} (from {entry['source']}) but this run "
                         f"launches {launched_kernel_family}: re-run tools/profile_final.sh + tools/sq_to_json.py"}
    return {k: entry[k] for k in ("kernel", "valu_busy", "valu_instructions_per_launch", "wait_frac", "sq_clock_GHz",
                                  "launch_us_under_counters", "source")}


def valu_roofline(w, kernel: str, kernel_ms: float, launched_kernel_family: str = ""):
    """Second roofline of the dominant launch (the pair sum co-scheduled with the spread): instruction-lanes issued by the pair
    rows (entries x VALU instructions per entry, ISA count of the packed body's hot loop) against the chip's VALU issue rate.
    The spread bricks that share the launch are left out of the numerator, so `frac` understates the launch's VALU use by their
    share (~15 % at cfg3).  `frac_issue` weights the quarter-rate transcendentals by the four issue slots they hold."""
    body = PAIR_BODY_VALU.get((w.dtype, w.exponent))
    if body is None or "rspace" not in kernel:
        return None
    ops, quarter = body
    entries = 2 * w.n_pairs  # full rows: every pair once in each of its two rows
    achieved = entries * ops / (kernel_ms * 1e-3) / 1e12
    return {
        "bound": "valu",
        "kernel": kernel,
        "achieved": achieved,
        "peak": VALU_PEAK_TLANEOPS,
        "unit": "Tlane-op/s",
        "frac": achieved / VALU_PEAK_TLANEOPS,
        "frac_issue": entries * (ops + 3 * quarter) / (kernel_ms * 1e-3) / 1e12 / VALU_PEAK_TLANEOPS,
        "entries_per_launch": entries,
        "valu_per_entry": ops,
        "quarter_rate_per_entry": quarter,
        "kernel_ms": kernel_ms,
        "floor_ms": entries * (ops + 3 * quarter) / (VALU_PEAK_TLANEOPS * 1e12) * 1e3,
        # the model above counts the rows' hot loop at the nominal 2.4 GHz; the counters of the whole launch (committed figure,
        # not measured by this run) put its vector units at 81 % busy: the launch is bound by instruction issue
        "pmc": sq_counters_of(getattr(w, "name", "").split("_")[0], launched_kernel_family),
    }


def dominant_kernel_family(w=None, n_parts: int = 0, n_frames: int = 1) -> str:
    """Name (without template arguments) of the co-scheduled spread + pair-sum kernel this process launched / captured last, as
    the library reports it (mipme_last_cosched_kernel: what RAN, not what the geometry would allow)."""
    from torchpme_amd import _lib

    return _lib.load().mipme_last_cosched_kernel().decode()


def host_identification():
    """CPU model, logical cores and max clock of the box (the eager / drop-in lines are host-bound: comparable only with this)."""
    info = {"logical_cores": os.cpu_count()}
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                info["cpu"] = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        info["max_MHz"] = round(int(open("/sys/devices/system/cpu/cpu0/cpufreq/cpuinfo_max_freq").read()) / 1e3)
    except (OSError, ValueError):
        try:
            mhz = [float(line.split(":")[1]) for line in open("/proc/cpuinfo") if line.startswith("cpu MHz")]
            info["observed_MHz_max"] = round(max(mhz)) if mhz else None
        except (OSError, ValueError):
            pass
    try:
        info["affinity_cores"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    return info


def plane_parts(w, s: int) -> int:
    """Workgroups per plane of the plane spread the library uses for this workload's energy step (0: bricks)."""
    from torchpme_amd import _lib, ops

    try:
        geom = ops.MeshGeometry(w.cell, (w.n_mesh,) * 3, 0 if w.scheme == "PME" else 1, w.order)
        return int(_lib.load().mipme_plane_spread_parts(C_byref(geom.desc(1)), w.n_atoms, _lib.F32 if s == 4 else _lib.F64))
    except Exception:  # (stub runs without the library)
        return 0


def C_byref(x):
    import ctypes

    return ctypes.byref(x)


def algorithmic_bytes(w, s: int, fused: bool = True, store_distances: bool = False, parts: int = 0):
    """Minimum HBM bytes per energy+forces step (reference data formats) and per kernel launch.

    Per kernel the figure is what the launch must move IN THE FORMAT IT READS, never more than SURVEY's figure for the
    reference formats: the distance kernel streams int32 pairs + one packed shift word + writes d (8 + 4 + s bytes per
    pair instead of 16 + 3s + s), and the fused pair kernel streams two entries per pair (``entry_bytes`` each) and reads
    neither d nor dL/dd.  DESIGN.md section 2 lists both."""
    from torchpme_amd import ops

    P, N, M = w.n_pairs, w.n_atoms, w.n_mesh**3
    eb = getattr(ops, "FUSED_ENTRY_BYTES", 8)
    dw = P * s if store_distances else 0  # the distance by-product of the fused pair kernel, when somebody wants it
    n = w.order
    slot = 16 + 6 * n * s  # what the binning pass stores per atom: {mesh coordinates, index} + 6 n one-dimensional weights
    halo = ((8 + n - 1) / 8) ** 3  # a gather workgroup stages the (8 + n - 1)^3 halo tile of its 8^3 brick
    per_kernel = {
        "pair_distance_forward": (P * (8 + 4 + s) if fused else P * (16 + 3 * s + s)) + N * 3 * s,
        "pair_distance_backward": P * (16 + 3 * s + s) + N * 6 * s,
        "rspace_forward": (2 * P * eb + dw + N * 8 * s) if fused else (P * (16 + s) + N * 2 * s),
        "rspace_backward": P * (16 + 2 * s) + N * 3 * s,
        # mesh stages (the meshes themselves are L2 / Infinity-Cache resident at these sizes)
        "spread": N * (slot + s) + M * s,
        # the spread and the fused distance + pair kernel co-scheduled in one launch (mipme_sr_job_t): both byte counts
        "spread+rspace_forward": (2 * P * eb + dw + N * 8 * s) + N * (slot + s) + M * s,
        "gather": N * (slot + 6 * s) + int(halo * M * s),
        # gather + energy + force assembly in one launch (the step's tail): also reads the pair force sums, writes field and forces
        "gather+energy+forces": N * (slot + 12 * s) + int(halo * M * s),
        "gather_grad": N * (slot + 8 * s) + 2 * int(halo * M * s),
        "fft_r2c": 2 * M * s,
        "fft_c2r": 2 * M * s,
        "apply_filter": int(2.5 * M * s),
        # (y,z) plane transforms + one kernel for x-FFT * G * inverse x-FFT: the three stages above in one composite
        "convolve_xfused": int(6.5 * M * s),
        # one-pass binning: positions + charges in, record (16 B), 6 n weights and the (x, y, z, q) record out
        "bin_atoms": N * (4 * s + slot + 4 * s),
        # energy reduction E = sum q V, its adjoint, and the energy-mode force assembly gE q_a (f F_a + field_a)
        "energy_sum": N * 2 * s,
        "energy_sum_backward": N * 3 * s,
        "forces_finalize": N * 10 * s,
    }
    if parts > 0:
        # Plane spread (round 5; streamed entries: round 6): the co-scheduled launch reads, per atom, ONE plane-list entry -- packed
        # mesh coordinates, the y / z offsets and the n products charge * w_x, (3 + n) s bytes padded to 16 (32 B at n = 5, fp32;
        # round 5: list slot + record + 3 n weights + charge = 84 B) -- counted ONCE although every atom is read by the n planes it
        # reaches (they hit L2), and writes `parts` half-complex meshes instead of the real one; the convolution loses its forward
        # plane launch (reads M s, writes M s) and reads the parts instead; the binning pass also writes the entry, the charge by
        # slot and a per-wavefront max.
        Mh2 = 2 * w.n_mesh * w.n_mesh * (w.n_mesh // 2 + 1) * s  # bytes of a half-complex mesh
        entry = ((3 + n) * s + 15) // 16 * 16
        per_kernel["spread+rspace_forward"] = (2 * P * eb + dw + N * 8 * s) + N * entry + parts * Mh2
        per_kernel["convolve_xfused"] = int(4.5 * M * s) + (parts - 1) * Mh2
        per_kernel["bin_atoms"] += N * (entry + s) + (N // 64 + 1) * 4
    step = P * (32 + 3 * s) + P * (32 + 8 * s) + N * 25 * s + 19 * M * s
    return step, per_kernel


# ----------------------------------------------------------------------------------------------------------------------
def _time_cpu_steps(fn, n_warm: int, n_max: int, budget_s: float, n_min: int = 1):
    """n_warm untimed + up to n_max timed calls (monotonic clock, median); stops early once the budget would be exceeded, but
    never before n_min timed calls."""
    times, t_all = [], time.monotonic()
    while True:
        t0 = time.monotonic()
        res = fn()
        times.append(time.monotonic() - t0)
        if len(times) >= n_warm + n_max or (len(times) >= n_warm + n_min and time.monotonic() - t_all + times[-1] > budget_s):
            break
    timed = times[n_warm:] if len(times) > n_warm else times[-1:]
    return float(np.median(timed)), len(timed), len(times) - len(timed), res


def cpu_baseline(w, budget_s: float = 40.0):
    """Time the CPU restatement of the reference's op sequence (``oracle/pme_torch.py``: ATen ops on CPU tensors,
    autograd) on this host, with the reference's own timing protocol (``tuning/tuner.py:337-373``: warm-up calls, then
    repeated energy + forces evaluations of the SAME frame, monotonic clock, median), swept over thread counts
    {1, 8, 16, 32, 64, 128} (those the host has): ``value`` is the best, ``one_thread`` the 1-thread figure SURVEY 8(d)
    asks for."""
    from oracle import pme_numpy as O
    from oracle import pme_torch as OT

    if w.exponent != 1:  # the torch oracle covers the Coulomb configurations; fall back to the NumPy port
        return cpu_baseline_numpy(w, 25.0)
    dt = torch.float32 if w.dtype == "f32" else torch.float64
    spec = O.PotentialSpec("coulomb", 1, w.smearing, 1.0)
    q, cell, pos, pairs, S = OT.as_tensors(w, dt)
    scheme = "P3M" if w.scheme == "P3M" else "Lagrange"
    n_logical = os.cpu_count() or 1
    counts = [t for t in (1, 8, 16, 32, 64, 128) if t <= n_logical] or [1]
    saved = torch.get_num_threads()
    sweep, energy = {}, None
    per = budget_s / len(counts)
    try:
        for t in counts:
            torch.set_num_threads(t)
            med, n_timed, n_warm, (E, _F) = _time_cpu_steps(
                lambda: OT.energy_forces_step(spec, scheme, w.order, w.mesh_spacing, q, cell, pos, pairs, S),
                n_warm=1, n_max=2, budget_s=per)
            sweep[t] = {"s_per_step": round(med, 4), "atom_steps_per_s": w.n_atoms / med, "timed": n_timed, "warmup": n_warm}
            energy = float(E)
        # the reported figure: SURVEY 8(d)'s protocol (tuning/tuner.py:337-373: >= 4 warm-ups, >= 4 repeats, median) at the
        # thread count the sweep found best
        best = min(sweep, key=lambda t: sweep[t]["s_per_step"])
        torch.set_num_threads(best)
        med, n_timed, n_warm, _ = _time_cpu_steps(
            lambda: OT.energy_forces_step(spec, scheme, w.order, w.mesh_spacing, q, cell, pos, pairs, S),
            n_warm=4, n_max=4, budget_s=max(10.0, 10 * sweep[best]["s_per_step"]), n_min=4)
        final = {"s_per_step": round(med, 4), "atom_steps_per_s": w.n_atoms / med, "timed": n_timed, "warmup": n_warm, "threads": best}
    finally:
        torch.set_num_threads(saved)
    return {
        "value": final["atom_steps_per_s"],
        "protocol_run": final,
        "unit": "atom-steps/s",
        "cores": best,
        "kind": "port",
        "one_thread": sweep[1]["atom_steps_per_s"] if 1 in sweep else None,
        "host_logical_cores": n_logical,
        "thread_sweep": {str(t): v for t, v in sweep.items()},
        "sample": f"full energy+forces steps of the same {w.n_atoms}-atom frame with oracle/pme_torch.py (PyTorch-CPU ATen "
                  f"ops + autograd): thread sweep with 1 warm-up + up to 2 timed steps per count in {counts} (torch.set_num_threads; "
                  f"host has {n_logical} logical cores), then the TuningTimings protocol (tuning/tuner.py:337-373) at the best "
                  f"count: {final['warmup']} warm-ups + {final['timed']} timed steps, median = {final['s_per_step']:.3f} s/step at "
                  f"{best} threads; energy {energy:.4f}",
    }


def cpu_baseline_numpy(w, budget_s: float = 25.0):
    """Single-threaded NumPy port (``oracle/pme_numpy.py``), used for the potentials the torch oracle does not cover."""
    from oracle import pme_numpy as O

    dt = np.float32 if w.dtype == "f32" else np.float64
    spec = O.PotentialSpec("coulomb" if w.exponent == 1 else "ipl", w.exponent, w.smearing, 1.0)
    pos, q, cell = w.positions.astype(dt), w.charges.astype(dt), w.cell.astype(dt)
    scheme = "P3M" if w.scheme == "P3M" else "Lagrange"

    def step():
        dist, _ = O.pair_distances(pos, cell, w.pairs, w.shifts)
        V, cache = O.forward(spec, scheme, w.order, w.mesh_spacing, q, cell, pos, w.pairs, dist, return_cache=True)
        gr = O.backward(cache, q)
        gpos, _ = O.pair_distances_backward(pos, cell, w.pairs, w.shifts, gr["dist"])
        return -(gpos + gr["positions"])

    med, n_timed, _, _ = _time_cpu_steps(step, n_warm=0, n_max=4, budget_s=budget_s)
    return {
        "value": w.n_atoms / med,
        "unit": "atom-steps/s",
        "cores": 1,
        "kind": "port",
        "one_thread": w.n_atoms / med,
        "host_logical_cores": os.cpu_count(),
        "sample": f"{n_timed} full energy+forces step(s) of the same {w.n_atoms}-atom frame with oracle/pme_numpy.py "
                  f"(NumPy, single thread), median {med:.2f} s/step",
    }


def _host_loop_ms(fn, n: int, warm: int):
    """Wall time of ``n`` eager calls of ``fn`` (after ``warm`` untimed ones), bracketed by device synchronisations, in ms per
    call -- with the cyclic garbage collector off for the loop, as ``timeit`` does: a generation-2 collection that happens to
    fall into a 60-call loop and frees captured HIP graphs of an earlier block costs tens of milliseconds.  Returns (mean without
    the longest call, median of the per-call host times, last result)."""
    import gc

    for _ in range(warm):
        res = fn()
    torch.cuda.synchronize()
    was = gc.isenabled()
    gc.disable()
    try:
        per = []
        t0 = time.perf_counter()
        for _ in range(n):
            t1 = time.perf_counter()
            res = fn()
            per.append(time.perf_counter() - t1)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        if was:
            gc.enable()
    if os.environ.get("MIPME_BENCH_DEBUG") == "1":
        st = torch.cuda.memory_stats()
        from torchpme_amd import ops as _ops
        print(f"[host loop] mean {1e3 * total / n:.3f} median {1e3 * float(np.median(per)):.3f} max {1e3 * max(per):.2f} at "
              f"{int(np.argmax(per))} device_allocs {st.get('num_device_alloc')} frees {st.get('num_device_free')} "
              f"retries {st.get('num_alloc_retries')} spins {_ops.SPIN_TIMEOUTS} topos {len(_ops._TOPOLOGIES)}", file=sys.stderr, flush=True)
    # ONE call of such a loop is now and then 60-85 ms long on the boxes of this pool (no device allocation, no retry, none of the
    # library's polls timing out -- MIPME_BENCH_DEBUG=1 prints the evidence; the same loops in a process of their own do not show
    # it): the mean leaves the single longest call out, and that call is printed when debugging
    trimmed = (total - max(per)) / (n - 1) if n > 1 else total
    return 1e3 * trimmed, 1e3 * float(np.median(per)), res


def drop_in_timing(frame, n_steps: int = 60, n_warm: int = 10):
    """ms per step of the reference's own call sequence on the same frame (eager launches from Python, general autograd
    nodes), and the parity of its result with the package's fast form of the step."""
    out = {"protocol": "d = pair_distances(positions, pairs, cell, shifts); V = calculator(charges, cell, positions, "
                       "pairs, d); E = (charges * V).sum(); E.backward() -- eager, no HIP graph, no weighted_sum, no "
                       "deferred distances (reference: tuning/tuner.py:337-373, tests/helpers.py:278-304)"}
    E_fast, F_fast = frame.step()
    F_fast = F_fast.clone()
    for key, mode in (("ms_per_step", "helper"), ("ms_per_step_torch_distances", "torch")):
        out[key], _, (E, F) = _host_loop_ms(lambda: frame.step_reference_protocol(mode), n_steps, n_warm)
        out[f"{key}_steps"] = n_steps
        if mode == "helper":
            out["rel_energy_diff_vs_fast_path"] = abs(float(E) - float(E_fast)) / abs(float(E_fast))
            out["force_rel_l2_diff_vs_fast_path"] = float((F - F_fast).norm() / F_fast.norm())
    # the same sequence through the Python autograd nodes only (MIPME_FRONT=0): what the compiled front end (csrc/front.cpp)
    # takes off the host
    from torchpme_amd import _front, ops

    out["compiled_front_end"] = bool(ops.FRONT and _front.module() is not None)
    if out["compiled_front_end"]:
        ops.FRONT = False
        try:
            out["ms_per_step_python_nodes"] = _host_loop_ms(lambda: frame.step_reference_protocol("helper"), n_steps, n_warm)[0]
        finally:
            ops.FRONT = True
    # a NEW list every call, as the reference's users supply it
    for key, mode in (("cold_list_ms", "list"), ("cold_stream_ms", "stream")):
        n = max(5, n_steps // 4)
        out[key], _, (E, F) = _host_loop_ms(lambda: frame.step_cold_list(mode), n, 3)
        out[f"{key}_rel_energy_diff_vs_fast_path"] = abs(float(E) - float(E_fast)) / abs(float(E_fast))
    out["cold_list_note"] = ("cold_list_ms: fresh neighbor_indices / shifts tensors every call (per-list work: radix-sort "
                             "transposition + entry streams, then the same kernels); cold_stream_ms: NeighborStream.update() "
                             "(device cell list writes the pair kernels' rows in place) + the same calculator call")
    return out


class _Committed:
    """The committed full-size numbers of a benchmark box, by key suffix (``energy``, ``force_sample``, ...): the REFERENCE'S OWN
    fp64 evaluation (tests/golden/ref_fullsize.npz, made by importing torchpme: tests/golden/make_reference_fullsize.py) where
    the box has one, else the pinned oracle's (tests/golden/workloads.npz).  Nothing under oracle/ or /root/reference runs here."""

    def __init__(self, name: str):
        self.name, self.z, self.prefix, self.source = name, None, None, None
        for fname, prefix, what in (("ref_fullsize.npz", f"{name}_f64_", "the reference itself (torchpme, fp64)"),
                                    ("workloads.npz", f"{name}_", "pinned oracle (oracle/pme_numpy.py, fp64)")):
            path = os.path.join(ROOT, "tests", "golden", fname)
            if os.path.exists(path):
                z = np.load(path)
                if prefix + "energy" in z.files:
                    self.z, self.prefix, self.source = z, prefix, f"{what} for this box: tests/golden/{fname}"
                    break

    def __contains__(self, key):
        return self.z is not None and (self.prefix + key in self.z.files or f"{self.name}_{key}" in self.z.files)

    def __getitem__(self, key):  # (n_pairs, sample, pos_checksum carry no precision tag)
        k = self.prefix + key
        return self.z[k if k in self.z.files else f"{self.name}_{key}"]

    def matches(self, w) -> bool:
        chk = np.array([w.positions.sum(), (w.positions**2).sum(), w.charges.sum(), (w.charges**2).sum()])
        return (self.z is not None and int(self["n_pairs"]) == w.n_pairs
                and bool(np.allclose(chk, self["pos_checksum"], rtol=1e-12, atol=1e-9)))


def contract_timing(frame, name: str):
    """The whole first-order autograd contract of the reference on the headline box (rank 0, one GPU): ms per evaluation of
    {E, F}, {E, F, dE/dq}, {E, F, dE/dq, dE/dcell} as a replayed HIP graph (binned step and live-bin step) and eagerly, and the
    reference's own timing protocol literally (``tuning/tuner.py:337-373``: clones with ``requires_grad`` on positions, cell,
    charges; constant ``neighbor_distances``; ``result.sum().backward()``) -- each result against the committed oracle numbers
    of this box (``tests/golden/workloads.npz``; nothing under oracle/ runs here).  Reference for the contract:
    ``tests/calculators/test_workflow.py:164-192``."""
    tpa, w = frame._tpa, frame.w
    out = {"reference": "tests/calculators/test_workflow.py:164-192 (gradients w.r.t. positions, charges, cell from one backward "
                        "pass); tuning/tuner.py:337-373 (TuningTimings protocol)"}
    z = _Committed(name)
    if "cell_grad" not in z or not z.matches(w):
        z = None
    out["vs_committed_source"] = None if z is None else z.source
    rng = np.random.default_rng(4242)
    rng.normal(size=(w.n_atoms, 3))
    s_vec = rng.normal(size=(w.n_atoms, 1))  # (the checksum vectors of tests/golden/make_workloads_golden.py)

    def errors(E, F, dq=None, dc=None):
        if z is None:
            return {"reference": "no committed contract numbers for this box"}
        sample = z["sample"]
        e = {"rel_energy": abs(float(E) - float(z["energy"])) / abs(float(z["energy"]))}
        Fs = z["force_sample"]
        e["force_rel_l2_256_atoms"] = float(np.linalg.norm(F.detach().cpu().double().numpy()[sample] - Fs) / np.linalg.norm(Fs))
        if dq is not None:
            q_ = dq.detach().cpu().double().numpy()
            ref = z["charge_grad_sample"]
            e["charge_grad_rel_l2_256_atoms"] = float(np.linalg.norm(q_[sample, 0] - ref) / np.linalg.norm(ref))
            e["charge_grad_checksum_rel"] = abs(float((s_vec * q_).sum()) - float(z["charge_grad_dot"])) / (
                np.linalg.norm(s_vec) * np.linalg.norm(q_))
        if dc is not None:
            ref = z["cell_grad"]
            e["cell_grad_rel_max"] = float(np.abs(dc.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())
        return e

    graph = {}
    for label, kw in (("E+F", {}), ("E+F+dq", dict(charge_gradient=True)),
                      ("E+F+dq+dcell", dict(charge_gradient=True, cell_gradient=True))):
        for mode in ("binned", "live"):
            try:
                if mode == "binned":
                    step = tpa.GraphedEnergyForces(frame.calc, frame.q, frame.cell, frame.pos.detach(), frame.pairs, frame.shifts, **kw)
                else:
                    step = tpa.GraphedEnergyForces(frame.calc, frame.q, frame.cell, frame.pos.detach(), neighbors=w.cutoff, **kw)
                res = step()
                torch.cuda.synchronize()
                entry = {"ms_per_step": round(min(_event_ms(step.graph.replay, 300, 30) for _ in range(3)), 6),
                         "fused_in_the_step": bool(step._fused_contract), "live_bins": step._live is not None}
                entry["vs_reference"] = errors(res[0], res[1], res[2] if "dq" in label else None,
                                            res[-1] if "dcell" in label else None)
                graph[f"{label} ({mode})"] = entry
                del step
            except Exception as exc:  # noqa: BLE001
                graph[f"{label} ({mode})"] = {"error": f"{type(exc).__name__}: {exc}"[:300]}
    out["graph"] = graph
    # the graphed steps above sit in reference cycles (step <-> neighbour stream <-> handles): collect them NOW -- a cyclic
    # collection that destroys HIP graphs in the middle of a timed eager loop costs tens of milliseconds
    import gc

    gc.collect()
    torch.cuda.synchronize()

    # ---- eager: the reference call sequence with more leaves
    def eager(leaves, weighted, n=60, warm=10):
        pos = frame.pos.detach().clone().requires_grad_(True)
        q = frame.q.clone().requires_grad_("q" in leaves)
        cell = frame.cell.clone().requires_grad_("cell" in leaves)

        def step():
            pos.grad = q.grad = cell.grad = None
            d = tpa.pair_distances(pos, frame.pairs, cell, frame.shifts)
            V = frame.calc(q, cell, pos, frame.pairs, d)
            E = tpa.weighted_sum(V, q) if weighted else (q * V).sum()
            E.backward()
            return E

        ms, med, E = _host_loop_ms(step, n, warm)
        return {"ms_per_step": round(ms, 5), "host_ms_per_step_median": round(med, 5),
                "vs_reference": errors(E.detach(), -pos.grad, q.grad, cell.grad)}

    out["eager"] = {}
    for label, leaves in (("E+F", ()), ("E+F+dq", ("q",)), ("E+F+dq+dcell", ("q", "cell"))):
        out["eager"][f"{label}: (q*V).sum()"] = eager(leaves, False)
        out["eager"][f"{label}: weighted_sum"] = eager(leaves, True)

    # ---- the reference's TuningTimings protocol, literally
    d_fixed = tpa.pair_distances(frame.pos.detach(), frame.pairs, frame.cell, frame.shifts).detach().clone()
    p0, c0, q0 = frame.pos.detach(), frame.cell, frame.q

    def protocol():
        positions, cell, charges = p0.clone(), c0.clone(), q0.clone()
        for t in (positions, cell, charges):
            t.requires_grad_(True)
        result = frame.calc.forward(positions=positions, charges=charges, cell=cell, neighbor_indices=frame.pairs,
                                    neighbor_distances=d_fixed)
        value = result.sum()
        value.backward(retain_graph=True)
        return value, positions.grad, charges.grad, cell.grad

    ms, med, (val, gp, gq, gc) = _host_loop_ms(protocol, 60, 10)
    val = val.detach()
    tt = {"ms_per_call": round(ms, 5), "host_ms_per_call_median": round(med, 5),
          "protocol": "positions, cell, charges cloned with requires_grad; constant neighbor_distances; "
                      "calculator.forward(...).sum().backward(retain_graph=True) -- tuning/tuner.py:350-369"}
    timer = tpa.tuning.TuningTimings(q0, c0, p0, frame.pairs, d_fixed, n_repeat=20, n_warmup=4)
    tt["TuningTimings_median_ms"] = round(1e3 * float(timer(frame.calc)), 5)
    if z is not None and "sumseed_cell" in z:
        sample = z["sample"]
        rp = z["sumseed_pos_sample"]
        rq = z["sumseed_charge_sample"]
        rc = z["sumseed_cell"]
        tt["vs_reference"] = {
            "rel_value": abs(float(val) - float(z["sumseed_value"])) / abs(float(z["sumseed_value"])),
            "positions_grad_rel_l2_256_atoms": float(np.linalg.norm(gp.cpu().double().numpy()[sample] - rp) / np.linalg.norm(rp)),
            "charges_grad_rel_l2_256_atoms": float(np.linalg.norm(gq.cpu().double().numpy()[sample, 0] - rq) / np.linalg.norm(rq)),
            "cell_grad_rel_max": float(np.abs(gc.cpu().double().numpy() - rc).max() / np.abs(rc).max()),
        }
    out["tuning_protocol"] = tt
    return out


def frames_timing(workload: str, device, counts=(2, 4, 8), n_steps: int = 100):
    """Several independent frames of the headline size in flight on ONE GPU (the frames a rank owns; the
    reference cannot batch mesh calculators at all, calculators/pme.py:102-105): ms per evaluation of F frames and atom-steps/s
    for F = 2, 4, 8, through ``GraphedFrameBatch`` (one launch per kernel for all frames, blockIdx.y = frame) and through one
    replayed graph per frame on its own stream.  At 32k atoms ONE frame leaves most of the machine idle (the step is a chain of
    latencies); the N = 1 headline stays one frame."""
    import torchpme_amd as tpa

    out = {"note": "secondary block: F independent frames per GPU; `value` of the bench line is ONE frame",
           "frame": None, "one_launch_per_kernel": {}, "graph_per_frame_on_streams": {}}
    frames = [Frame(make_workload(workload, f), device) for f in range(max(counts))]
    w = frames[0].w
    out["frame"] = f"{w.name}: {w.n_atoms} atoms, {w.n_mesh}^3 mesh, {w.dtype}, seeds 0..{max(counts) - 1} of the workload"
    graphs = [tpa.GraphedEnergyForces(f.calc, f.q, f.cell, f.pos, f.pairs, f.shifts) for f in frames]
    streams = [torch.cuda.Stream(device) for _ in frames]
    for F in counts:
        batch = tpa.GraphedFrameBatch(frames[0].calc, [(f.q, f.cell, f.pos, f.pairs, f.shifts) for f in frames[:F]])
        ms = min(_event_ms(batch.graph.replay, n_steps, 10) for _ in range(2))
        out["one_launch_per_kernel"][str(F)] = {"ms_per_step": round(ms, 5), "atom_steps_per_s": F * w.n_atoms / (ms * 1e-3)}
        del batch

        def step_streams():
            cur = torch.cuda.current_stream(device)
            for g, st in zip(graphs[:F], streams[:F]):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    g.graph.replay()
            for st in streams[:F]:
                cur.wait_stream(st)

        ms = min(_event_ms(step_streams, n_steps, 10) for _ in range(2))
        out["graph_per_frame_on_streams"][str(F)] = {"ms_per_step": round(ms, 5), "atom_steps_per_s": F * w.n_atoms / (ms * 1e-3)}
    del graphs, streams, frames
    import gc

    gc.collect()  # (cycles holding HIP graphs: not in the middle of somebody else's timed loop)
    torch.cuda.synchronize()
    return out


def second_order_timing(frame, n_steps: int = 5, n_warm: int = 2):
    """Secondary block: what exact second derivatives cost (`calculator.double_backward = "analytic"`, the route through
    differentiable primitives; the reference differentiates its ATen chain to any order, calculators/calculator.py:43-87,
    103-189).  One training step of a loss on forces with learned charges: q = theta q0, E = sum q V, F = -dE/dr with
    create_graph=True, loss = sum F^2, loss.backward() to theta.  E is quadratic in theta, so d loss / d theta = 4 loss at
    theta = 1 exactly: the relative deviation from that is reported next to the time."""
    tpa = frame._tpa
    calc = type(frame.calc)(frame.calc.potential, mesh_spacing=frame.w.mesh_spacing, interpolation_nodes=frame.w.order)
    calc.double_backward = "analytic"
    theta = torch.ones((), dtype=frame.dtype, device=frame.q.device, requires_grad=True)
    pos = frame.pos.detach().clone().requires_grad_(True)

    def energy():
        q = frame.q * theta
        d = tpa.pair_distances(pos, frame.pairs, frame.cell, frame.shifts)
        return (q * calc(q, frame.cell, pos, frame.pairs, d)).sum()

    def forces_only():
        return torch.autograd.grad(energy(), pos)[0]

    def train_step():
        theta.grad = None
        (g,) = torch.autograd.grad(energy(), pos, create_graph=True)
        loss = (g * g).sum()
        loss.backward(inputs=[theta])
        return loss.detach()

    out = {"route": 'double_backward = "analytic" (torch-pme_amd/analytic.py, csrc/jets.hip)',
           "workload": "loss = sum F^2, F = -dE/dr (create_graph), charges = theta * q0; backward to theta"}
    out["energy_forces_ms"] = round(_host_loop_ms(forces_only, n_steps, n_warm)[0], 4)
    torch.cuda.reset_peak_memory_stats()
    out["force_loss_step_ms"] = round(_host_loop_ms(train_step, n_steps, n_warm)[0], 4)
    out["peak_allocated_GB"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    loss = float(train_step())
    out["loss"] = loss
    out["dloss_dtheta_rel_dev_from_4_loss"] = abs(float(theta.grad) - 4.0 * loss) / (4.0 * loss)
    return out


def oracle_accuracy(w, name, E32, F32, E64=None, F64=None):
    """The timed dtype's energy and forces (and the fp64 path's) against the committed full-size numbers of this very box: the
    REFERENCE'S OWN fp64 evaluation (tests/golden/ref_fullsize.npz) where there is one, else the pinned oracle's
    (tests/golden/workloads.npz) -- see _Committed.  Nothing under oracle/ runs here."""
    z = _Committed(name)
    if z.z is None:
        return {"reference": f"no committed numbers for workload {name}"}
    if not z.matches(w):
        return {"reference": "committed numbers belong to a different box (seed / size)"}
    Eo, sample, Fs = float(z["energy"]), z["sample"], z["force_sample"]

    def errs(E, F):
        F = F.detach().cpu().double().numpy()
        return {"rel_energy_error": abs(E - Eo) / abs(Eo),
                "force_rel_l2_error_256_atoms": float(np.linalg.norm(F[sample] - Fs) / np.linalg.norm(Fs)),
                "force_sq_rel_error": abs(float((F * F).sum()) - float(z["force_sq"])) / float(z["force_sq"])}

    out = {"reference": z.source, "reference_energy": Eo}
    out.update(errs(E32, F32))
    if E64 is not None:
        out["fp64_path_vs_reference"] = errs(E64, F64)
    return out


def _event_ms(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def list_refresh_timing(frame, frozen_list_ms: float):
    """What a new neighbour list costs (rank 0, one GPU), in ms: the reference-format build on the device; the per-list work
    of the list-based row kernels; the in-place refresh of the device row stream (one replay of the captured refresh graph);
    the first step after a refresh; and an MD-like loop with a refresh every 10 / 20 steps."""
    tpa, w = frame._tpa, frame.w
    from torchpme_amd import ops

    out = {}
    pos = frame.pos.detach()

    def host_timed(fn, n=3):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    out["reference_format_build_ms"] = host_timed(lambda: tpa.neighbor_list_device(pos, frame.cell, w.cutoff))

    def new_list_topology():
        pairs = frame.pairs.clone()
        topo = ops.get_topology(pairs, w.n_atoms)
        topo.compact_entries(frame.shifts, frame.shifts)

    out["list_path_transposition_ms"] = host_timed(new_list_topology)
    step = tpa.GraphedEnergyForces(frame.calc, frame.q, frame.cell, pos, neighbors=w.cutoff)
    st = step.stream
    out["row_capacity"], out["longest_row"], out["entries"] = st.row_capacity, st.longest_row, st.n_entries
    E_stream = float(step()[0])
    out["stream_refresh_ms"] = _event_ms(step.refresh_graph.replay, 30)
    out["stream_step_ms"] = _event_ms(step.graph.replay, 200, 20)

    def refresh_then_step():
        step.refresh_graph.replay()
        step.graph.replay()

    out["first_step_after_refresh_ms"] = _event_ms(refresh_then_step, 30) - out["stream_refresh_ms"]

    def md(interval, n=200):
        def run():
            for it in range(n):
                if it % interval == 0:
                    step.refresh_graph.replay()
                step.graph.replay()
        return _event_ms(run, 1, 1) / n

    out["md_amortized_ms_per_step"] = {"refresh_every_10": md(10), "refresh_every_20": md(20)}
    st.check(synchronize=True)
    out["frozen_list_ms_per_step"] = frozen_list_ms
    out["stream_energy"] = E_stream
    out["note"] = ("stream_refresh_ms = one replay of the captured refresh graph (cell-list binning: 4 kernels; the walk that "
                   "writes the 4-byte row stream + row bounds; status report) -- no (P,2) list, no sort, no re-capture of the "
                   "step; md_amortized = wall time of 200 graph replays with a refresh every k steps / 200")
    return out


DUMP_LIMIT_BYTES = 64 * 2**20


def write_outputs(directory: str, arrays: dict):
    """``--dump-outputs``: one ``<name>.npy`` per array (float32 / float64 as computed).  Above DUMP_LIMIT_BYTES the forces are cut
    to a fixed, seeded sample of atoms (the same for every build), whose indices go to ``forces_atom_index.npy``."""
    os.makedirs(directory, exist_ok=True)
    arrays = dict(arrays)
    forces = arrays.get("forces")
    if forces is not None and sum(a.nbytes for a in arrays.values()) > DUMP_LIMIT_BYTES:
        per_atom = forces.nbytes // forces.shape[1]
        room = DUMP_LIMIT_BYTES - sum(a.nbytes for k, a in arrays.items() if k != "forces")
        n_keep = max(1, min(forces.shape[1], room // (per_atom + 8)))
        idx = np.sort(np.random.default_rng(2024).choice(forces.shape[1], n_keep, replace=False))
        arrays["forces"] = np.ascontiguousarray(forces[:, idx])
        arrays["forces_atom_index"] = idx.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(directory, f"{name}.npy"), a)


# ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.sweep_orders:
        sys.path.insert(0, os.path.join(ROOT, "tools", "r06"))
        import order_sweep

        return order_sweep.main(as_json=True)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(respawn_under_torchrun(args, argv))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" in os.environ and world != args.gpus and rank == 0:
        print(f"[bench] --gpus {args.gpus} but the launcher started {world} rank(s); reporting n_gpus = {world}",
              file=sys.stderr)
    stub = args.stub_evaluator
    backend = "gloo" if stub else "nccl"
    distributed = world > 1 or os.environ.get("MIPME_FORCE_DIST") == "1"  # the latter: 1-rank smoke test of this path
    dist = None
    if distributed:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if not stub:
            torch.cuda.set_device(local_rank)
        # RCCL prints a version banner on the C-level stdout when the communicator comes up; keep stdout for the one JSON
        # line by pointing fd 1 at stderr while the process group initialises and runs its first collective
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if stub:
                dist.init_process_group(backend)
            else:
                dist.init_process_group(backend, device_id=torch.device("cuda", local_rank))
            dist.barrier()  # RCCL completes its lazy set-up before anything is timed or captured
            if not stub:
                torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
        world = dist.get_world_size()  # what the backend (RCCL) reports, not what the environment claimed
    device = torch.device("cpu") if stub else torch.device("cuda", local_rank)
    if not stub:
        torch.cuda.set_device(device)
    affinity = None
    if (distributed and os.environ.get("MIPME_BIND") != "0") or os.environ.get("MIPME_BIND") == "1":
        affinity = bind_rank_to_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)), None if stub else local_rank)

    def sync():
        if not stub:
            torch.cuda.synchronize()

    def close():
        if distributed:
            # every rank is past its last collective before any rank tears its connections down (a rank that exits while a
            # peer still reads from it can abort that peer)
            dist.barrier()
            dist.destroy_process_group()

    n_frames = max(1, args.frames_per_gpu)
    if stub:
        frames = [StubFrame(rank * n_frames + f, device) for f in range(n_frames)]
    else:
        import torchpme_amd as tpa
        from torchpme_amd import ops

        frames = [Frame(make_workload(args.workload, rank * n_frames + f), device, args.store_distances) for f in range(n_frames)]
    frame, w = frames[0], frames[0].w
    s = 4 if w.dtype == "f32" else 8
    # the farm's exchange: every rank contributes its frame energies to an all-gather (8 B per frame)
    exchange_mode = (args.exchange or "log") if distributed else "none"
    mode = {"x": exchange_mode}  # (the secondary blocks at the end time the other modes with the same closures)
    log_cap = max(1, args.steps)
    my_energy = torch.zeros(n_frames, dtype=frame.dtype, device=device)
    all_energies = torch.zeros(world * n_frames, dtype=frame.dtype, device=device)
    ring = [(torch.zeros_like(my_energy), torch.zeros_like(all_energies)) for _ in range(2)]
    pending = [None, None]

    def dbg(msg):
        if os.environ.get("MIPME_BENCH_DEBUG") == "1":
            sync()
            print(f"[bench rank {rank}] {msg}", file=sys.stderr, flush=True)

    launch = "eager" if stub else args.launch
    use_batch = launch == "graph" and n_frames > 1 and args.frame_batch == "one-launch"
    # exchange "log": the step's graph appends its energies to a device-resident log (graphed.EnergyLog: one more node);
    # "in-graph": the per-step RCCL all-gather is captured as the tail of the step's graph
    elog = None
    extra = {}
    if distributed and not stub and launch == "graph" and (use_batch or n_frames == 1):
        if exchange_mode == "log":
            elog = tpa.EnergyLog(log_cap, n_frames, device)
            extra["energy_log"] = elog
        elif exchange_mode == "in-graph":
            def _gather_in_graph(step):
                src = step.energies if hasattr(step, "energies") else step.energy.reshape(1)
                dist.all_gather_into_tensor(all_energies, src)

            extra["epilogue"] = _gather_in_graph
    elif exchange_mode == "in-graph":
        raise SystemExit("--exchange in-graph needs --launch graph and one graph per rank (one frame, or --frame-batch one-launch)")
    # without a graph of its own to ride on (eager launches, one graph per frame on its own stream, the CPU stub) the log is
    # filled by a copy after every step
    host_log = torch.zeros((log_cap, n_frames), dtype=torch.float64, device=device) if (distributed and elog is None) else None
    graphed = None
    if launch == "graph":
        try:
            own = extra if not use_batch else {}
            if args.neighbors == "stream":
                graphed = [tpa.GraphedEnergyForces(f.calc, f.q, f.cell, f.pos, neighbors=f.w.cutoff, **own) for f in frames]
            else:
                graphed = [tpa.GraphedEnergyForces(f.calc, f.q, f.cell, f.pos, f.pairs, f.shifts, **own) for f in frames]
        except Exception as exc:  # capture not possible on this stack: fall back to eager launches, and say so
            print(f"[bench] HIP-graph capture failed ({type(exc).__name__}: {exc}); using eager launches", file=sys.stderr)
            launch, graphed = "eager", None
            if elog is not None:  # nobody appends to a graph's log now: the log is filled by a copy after every step
                elog, extra = None, {}
                host_log = torch.zeros((log_cap, n_frames), dtype=torch.float64, device=device)
            use_batch = False

    # several frames per rank: every frame replays its graph on its own stream, so the (latency-bound, small) kernels of
    # independent frames overlap on the GPU; each stream orders the successive steps of its frame
    streams = [torch.cuda.Stream(device) for _ in frames] if (graphed is not None and n_frames > 1) else None
    batch = None
    if streams is not None and args.frame_batch == "one-launch":
        # all frames of this rank with one launch per kernel (blockIdx.y = frame) from one HIP graph
        batch = tpa.GraphedFrameBatch(frames[0].calc, [(f.q, f.cell, f.pos, f.pairs, f.shifts) for f in frames], **extra)

    def one_step():
        """One pass of the hot path over this rank's batch of frames; returns the frame energies (device tensors)."""
        if batch is not None:
            return list(batch()[0].unbind(0))
        if streams is not None:
            for g, st in zip(graphed, streams):
                with torch.cuda.stream(st):
                    g.graph.replay()
            return [g.energy for g in graphed]
        if graphed is not None:
            return [g()[0] for g in graphed]
        return [f.step()[0] for f in frames]

    def join_streams():
        if streams is not None and batch is None:
            for st in streams:
                torch.cuda.current_stream(device).wait_stream(st)

    def energies_tensor(energies):
        """This rank's frame energies as ONE contiguous tensor (the graphs' own static buffers where there are such)."""
        if batch is not None:
            return batch.energies
        if graphed is not None and n_frames == 1:
            return graphed[0].energy.reshape(1)
        for k, E in enumerate(energies):
            my_energy[k] = E.reshape(())
        return my_energy

    def exchange(i, energies):
        """The all-gather of one evaluation.  per-step / final: on the compute stream (the next evaluation waits for it);
        pipelined: copied to one of two slots and gathered asynchronously, waited for before the slot is reused."""
        if not distributed:
            return
        src = energies_tensor(energies)
        if mode["x"] == "pipelined":
            k = i % 2
            if pending[k] is not None:
                pending[k].wait()
            ring[k][0].copy_(src)
            pending[k] = dist.all_gather_into_tensor(ring[k][1], ring[k][0], async_op=True)
        else:
            dist.all_gather_into_tensor(all_energies, src)

    def drain(last_i):
        if distributed and mode["x"] == "pipelined":
            for k in range(2):
                if pending[k] is not None:
                    pending[k].wait()
                    pending[k] = None
            all_energies.copy_(ring[last_i % 2][1])

    logged = {"entries": 0, "pushes": 0}
    log_gathered = torch.zeros((world, log_cap, n_frames), dtype=torch.float64, device=device) if distributed else None

    def exchange_log():
        """ONE collective for the evaluations of a timed region: all-gather of this rank's whole (capacity, frames) log -- the
        last `capacity` evaluations, whatever the slot the newest one sits in (the log wraps around; no reset, no allocation and
        no copy inside the timed region: with the driver's 20-step regions every launch of this epilogue is ~1 % of the region)."""
        from torchpme_amd import farm

        farm.gather_energy_log(elog.values if elog is not None else host_log, out=log_gathered)
        logged["entries"] = int(log_gathered.numel())

    def newest_logged_energies():
        """(after the timed regions) the newest evaluation of every rank from the gathered log -> all_energies"""
        if logged["pushes"] > 0:
            all_energies.copy_(log_gathered[:, (logged["pushes"] - 1) % log_cap, :].reshape(-1))

    def run_steps(n, with_exchange=True):
        E = None
        x = mode["x"] if with_exchange else "none"
        for i in range(n):
            E = one_step()
            if elog is not None:
                logged["pushes"] += 1  # (every replay of a graph with a log appends, whatever the exchange protocol)
            if x in ("per-step", "pipelined"):
                join_streams()
                exchange(i, E)
            elif x == "log" and elog is None:
                join_streams()
                host_log[logged["pushes"] % log_cap].copy_(energies_tensor(E))
                logged["pushes"] += 1
        join_streams()
        if x == "final" and E is not None:
            exchange(0, E)
        if x == "log" and n > 0:
            exchange_log()
        if with_exchange and n > 0:
            drain(n - 1)
        return E

    def timed_block(n, only_rank0=False, with_exchange=True):
        """EXACTLY n steps bracketed by barrier + synchronize on both sides; only_rank0: the other ranks stay idle (and there
        is no exchange), for the one-rank reference time of weak_efficiency."""
        sync()
        if distributed:
            dist.barrier()
        sync()
        t0 = time.perf_counter()
        E = None
        if not only_rank0 or rank == 0:
            E = run_steps(n, with_exchange=with_exchange and not only_rank0)
        sync()
        dt_own = time.perf_counter() - t0  # this rank's own time (before it waits for the others)
        if distributed:
            dist.barrier()
        sync()
        return dt_own, E

    dbg("graph captured" if graphed is not None else "eager mode")
    # clock ramp: a fresh box needs tens of ms of work before its clocks settle (round 2: 7 % between a 1.5 ms timed region
    # right after 5 replays and a long run)
    n_prewarm, t_pre = 0, time.perf_counter()
    while not stub and (1e3 * (time.perf_counter() - t_pre) < args.prewarm_ms or (exchange_mode == "in-graph" and n_prewarm < 400)):
        run_steps(20, with_exchange=False)
        sync()
        n_prewarm += 20
        if exchange_mode == "in-graph" and n_prewarm >= 400:  # every replay is a collective: the same count on every rank
            break
    E = run_steps(args.warmup)
    dbg("warm-up done")
    t_alone = None
    # (an in-graph collective cannot run on one rank alone)
    if args.full and distributed and world > 1 and exchange_mode != "in-graph":
        t_alone, _ = timed_block(args.steps, only_rank0=True)
    block_times = []
    for b in range(max(1, args.blocks)):
        dt_own, Eb = timed_block(args.steps)
        E = Eb if Eb is not None else E
        block_times.append(dt_own)
    dbg("timed loops done")
    dumped = None
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step, copied out before anything else runs: the graphs' own
        # output buffers, or the eager step's results (forces = -dE/dpositions)
        dumped = {"energy": torch.stack([e.detach().reshape(()) for e in E])}
        if not stub:
            if batch is not None:
                dumped["forces"] = torch.stack(batch.forces)
            elif graphed is not None:
                dumped["forces"] = torch.stack([g.forces for g in graphed])
            else:
                dumped["forces"] = torch.stack([f.pos.grad for f in frames])
        dumped = {k: v.detach().cpu().numpy() for k, v in dumped.items()}
    dom_family = "" if stub else dominant_kernel_family()  # (asked NOW: the secondary blocks below launch other variants)
    log_entries = logged["entries"]  # (of the last timed block)
    # the other exchange protocols, one block each, same invocation (reported under parallelism.other_exchange_modes; never `value`)
    other_modes, other_times = [], []
    if args.full and distributed and not args.no_exchange_sweep and exchange_mode != "in-graph":
        sweep = ("none", "log", "per-step", "pipelined", "final") if args.exchange_sweep == "full" else ("none", "per-step", "final")
        for m in sweep:
            if m == exchange_mode or (m == "log" and exchange_mode == "in-graph"):
                continue
            mode["x"] = m
            run_steps(min(args.warmup, 5), with_exchange=m != "none")
            dt_m, _ = timed_block(args.steps, with_exchange=m != "none")
            other_modes.append(m)
            other_times.append(dt_m)
        mode["x"] = exchange_mode
        run_steps(1)  # (all_energies = the reported mode's, for the check below)
    if distributed and exchange_mode == "log":
        newest_logged_energies()
    n_blocks = len(block_times)
    own = torch.tensor(block_times + other_times + [t_alone or 0.0], dtype=torch.float64, device=device)
    if distributed:
        flat = torch.zeros(world * own.numel(), dtype=torch.float64, device=device)
        dist.all_gather_into_tensor(flat, own)
        gathered = flat.reshape(world, own.numel())
    else:
        gathered = own.reshape(1, -1)
    per_block = gathered[:, :n_blocks].max(dim=0).values.tolist()  # MAX over ranks, per block
    other_ms = {m: round(1e3 * float(gathered[:, n_blocks + k].max()) / args.steps, 6) for k, m in enumerate(other_modes)}
    # the contract's one timed region: the MEDIAN block (each block is exactly K steps between barrier + synchronize; the first
    # block was the fastest one in every run of round 4 -- a 1 % favourable pick, round-4 verdict); the first block is reported
    # next to it as ms_per_step_first_block
    sel = sorted(range(len(per_block)), key=per_block.__getitem__)[(len(per_block) - 1) // 2]
    elapsed = per_block[sel]
    per_rank_ms = [1e3 * float(v) / args.steps for v in gathered[:, sel].tolist()]  # (of the reported block)
    ms_per_step = 1e3 * elapsed / args.steps
    ms_per_step_first_block = 1e3 * per_block[0] / args.steps
    blocks_ms = [1e3 * v / args.steps for v in per_block]
    value = world * n_frames * w.n_atoms * args.steps / elapsed
    weak_efficiency = None
    if t_alone is not None or (args.full and distributed and world > 1):
        t1 = float(gathered[0, -1])
        weak_efficiency = {
            "value": t1 / elapsed if elapsed > 0 else None,
            "median_blocks": t1 / float(np.median(per_block)),
            "one_rank_ms_per_step": 1e3 * t1 / args.steps,
            "definition": "rank 0's time for the same K steps with the other ranks idle (no exchange) / MAX-over-ranks time "
                          "with all ranks busy and the exchange in the loop; same invocation, same clocks",
        }
    rank_info = {"rank": rank, "local_rank": local_rank, "affinity": affinity}
    if not stub:
        props = torch.cuda.get_device_properties(device)
        rank_info["device"] = {"name": props.name, "uuid": str(getattr(props, "uuid", None)),
                               "pci": f"{getattr(props, 'pci_domain_id', 0):04x}:{getattr(props, 'pci_bus_id', 0):02x}:"
                                      f"{getattr(props, 'pci_device_id', 0):02x}"}
    ranks = [rank_info]
    if distributed:
        ranks = [None] * world
        dist.all_gather_object(ranks, rank_info)
    parallelism = {
        "n_ranks": world,
        "backend": (f"{backend} ({'RCCL' if backend == 'nccl' else 'CPU test'}), world size reported by the backend"
                    if distributed else "none (single process)"),
        "exchange": exchange_mode,
        "collective": ({"log": "every step appends its frame energies to a device-resident log ("
                               + ("last node of the step's HIP graph" if elog is not None else "a copy after the step")
                               + "); ONE all_gather_into_tensor of the K x frames log per timed region, inside it (SURVEY 8(e))",
                        "per-step": "all_gather_into_tensor of the frame energies after EVERY evaluation, on the compute stream, "
                                    "inside the timed loop",
                        "pipelined": "all_gather_into_tensor after every evaluation, asynchronous (two slots), inside the timed loop",
                        "in-graph": "all_gather_into_tensor of the frame energies captured as the tail of the step's HIP graph",
                        "final": "one all_gather_into_tensor of the LAST step's frame energies per timed region"}[exchange_mode]
                       if distributed else None),
        "log_entries_gathered": log_entries if exchange_mode == "log" else None,
        "energies_gathered": int(all_energies.numel()) if distributed else n_frames,
        "energies_sum": float(all_energies.double().sum()) if distributed else None,
        "other_exchange_modes_ms_per_step": other_ms if distributed else None,
        "per_rank_ms_per_step": [round(v, 6) for v in per_rank_ms],
        "ranks": ranks,
    }
    timing = {
        "prewarm_ms": args.prewarm_ms, "prewarm_steps": n_prewarm, "blocks": len(blocks_ms),
        "blocks_ms_per_step": [round(v, 6) for v in blocks_ms],
        "protocol": "untimed replays for >= prewarm_ms, W warm-up steps, then `blocks` blocks of exactly K steps, each bracketed by "
                    "barrier + synchronize; ms_per_step / value = the median block (lower median), ms_per_step_first_block = the first one",
    }
    ms_per_step_median = float(np.median(blocks_ms))

    if dumped is not None:
        write_outputs(args.dump_outputs, dumped)
    if stub:
        if rank == 0:
            print(json.dumps({
                "metric": "stub", "value": value, "unit": "stub-units/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "f64",
                "data": "stub evaluator on CPU ranks (launch-path test; NOT a measurement of the hot path)",
                "config": {"workload": "stub", "frames_per_gpu": n_frames}, "parallelism": parallelism,
                "energies_gathered": int(all_energies.numel()) if distributed else n_frames,
                "energies_sum": float(all_energies.sum()) if distributed else None,
                "ms_per_step_median": ms_per_step_median, "ms_per_step_first_block": ms_per_step_first_block, "timing": timing,
                "weak_efficiency": weak_efficiency,
            }))
        close()
        return

    line = None
    if rank == 0:
        n_parts = plane_parts(w, s) if args.neighbors == "list" else 0
        if "plane" not in dom_family:  # what RAN decides (mipme_last_cosched_kernel), not what the geometry would allow
            n_parts = 0
        # a frame batch (GraphedFrameBatch) keeps its plane workgroups at <= 128 per launch (csrc/bricks.hip frames_forward_t)
        label_parts = n_parts
        while batch is not None and label_parts > 1 and label_parts * w.n_mesh * n_frames > 128:
            label_parts -= 1
        line = {
            "metric": "atom-steps/sec (energy+forces)",
            "value": value,
            "unit": "atom-steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "ms_per_step_median": ms_per_step_median,
            "ms_per_step_first_block": ms_per_step_first_block,
            "value_median": world * n_frames * w.n_atoms / (ms_per_step_median * 1e-3),
            "timing": timing,
            "weak_efficiency": weak_efficiency,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": w.dtype,
            "data": "synthetic",
            "config": {
                "workload": f"{w.name}: {w.n_atoms} atoms, {w.n_pairs} half pairs (rc={w.cutoff} A), "
                            f"{w.scheme} order {w.order}, {w.n_mesh}^3 mesh, "
                            f"{'Coulomb' if w.exponent == 1 else '1/r^%d' % w.exponent}, {w.dtype}, energy+forces via autograd",
                "preset": args.preset,
                "frames_per_gpu": n_frames,
                "neighbors": args.neighbors,
                "spread": (f"plane spread, {label_parts} workgroup(s) per x plane -- per band of rows where a plane's tile does not fit "
                           "the launch's LDS (128 x 128: z transform in the tile, y columns as a launch of their own) -- (charges "
                           "into the forward plane transform's LDS tiles; no forward plane launch)" if n_parts > 0 else "owner-computes bricks + forward plane launch"),
                "launch": ("HIP graph replay of the captured step"
                           + (", all frames in one launch per kernel (GraphedFrameBatch)" if batch is not None
                              else ", one stream per frame" if streams is not None else ""))
                          if launch == "graph" else "eager kernel launches",
                "parallelism": f"{world * n_frames} independent frame(s), {n_frames} per GPU, {world} rank(s)",
            },
            "parallelism": parallelism,
        }
    if not args.full:
        if rank == 0:
            print(json.dumps(line))
        close()
        return

    # ---- instrumented pass: per-call HIP-event timings on the launch stream (does not affect `value`) ----
    from torchpme_amd import _lib

    for _ in range(3):  # (eager launches of this route may be the process's first: code-object loads, lazy scratch)
        frame.step()
    torch.cuda.synchronize()
    ops.PROFILE = {}
    _lib.profile_enable(True)
    n_instr = min(args.steps, 50)
    for _ in range(n_instr):
        frame.step()
    torch.cuda.synchronize()
    prof = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in ops.PROFILE.items()}  # ms per call
    stages = {k: ms / calls for k, (calls, ms) in _lib.profile_report().items()}  # ms per launch, inside composites
    stage_calls = {k: calls / n_instr for k, (calls, ms) in _lib.profile_report().items()}
    _lib.profile_enable(False)
    ops.PROFILE = None

    # ---- accuracy of the timed dtype against the same path in fp64 (itself pinned to the reference at 1e-13) ----
    accuracy = None
    if rank == 0 and w.dtype == "f32":
        import copy

        w64 = copy.copy(w)
        w64.dtype = "f64"
        f64 = Frame(w64, device)
        E64, F64 = f64.step()
        frame.store_distances = True  # this one evaluation also stores the distance by-product of the pair kernel
        E32, F32 = frame.step()
        frame.store_distances = args.store_distances
        accuracy = {
            "vs_own_fp64": {"rel_energy_error": abs(float(E32) - float(E64)) / abs(float(E64)),
                            "force_rel_l2_error": float((F32.double() - F64).norm() / F64.norm())},
        }
        accuracy.update(oracle_accuracy(w, args.workload, float(E32), F32, float(E64), F64))
        # the distance tensor the step produced (by-product of the pair kernel) against plain tensor arithmetic in fp64
        p64, c64 = frame.pos.detach().double(), frame.cell.double()
        d_ref = (p64[frame.pairs[:, 1]] - p64[frame.pairs[:, 0]] + frame.shifts.double() @ c64).norm(dim=1)
        accuracy["distance_max_rel_error"] = float(((frame.distances.double() - d_ref).abs() / d_ref).max())
        del f64
    elif rank == 0:
        Ed, Fd = frame.step()
        accuracy = oracle_accuracy(w, args.workload, float(Ed), Fd)

    if rank == 0:
        # (the per-kernel stage times below are those of ONE frame's step whatever the number of frames per GPU)
        step_bytes, per_kernel = algorithmic_bytes(w, s, fused=ops.FUSE_DISTANCES, store_distances=args.store_distances,
                                                   parts=n_parts)
        kernels = {k: v for k, v in prof.items() if k in per_kernel}
        kernels.update({k: v for k, v in stages.items() if k in per_kernel})
        # dominant kernel = the longest single launch (an HBM-streaming pair kernel at these sizes); the per-kernel
        # table below lists every kernel with its launches per step
        # (single launches only: "convolve_xfused" is the library's composite of three launches -- (y,z) planes, x stage,
        # (y,z) planes -- timed as one stage; the largest of them is 9.8 us at cfg3)
        composite = {"convolve_xfused", "convolve"}
        dom = max((k for k in kernels if k not in composite), key=kernels.get)
        achieved = per_kernel[dom] / (kernels[dom] * 1e-3) / 1e9
        # HBM bytes per launch: bench.py cannot run the profiler on itself, so this is the figure of the COMMITTED rocprofv3
        # PMC passes of this same command (tools/profile_gpu.sh -> tools/pmc_to_json.py -> profiles/pmc_traffic.json),
        # labelled as such; null for workloads without a committed profile
        traffic, traffic_source = None, None
        pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if n_frames == 1 and os.path.exists(pmc_path):
            pmc = json.load(open(pmc_path))
            if args.workload != "water":  # other workloads with a committed counter pass (tools/pmc_to_json.py <...> <workload>)
                pmc = pmc.get("workloads", {}).get(args.workload, {"kernels": {}})
            traffic = pmc["kernels"].get(dom, {}).get("hbm_bytes_per_launch")
            if traffic is not None:
                traffic_source = (f"committed profile profiles/pmc_traffic.json (from {pmc.get('source')}; separate rocprofv3 "
                                  "--pmc FETCH_SIZE / WRITE_SIZE passes of this command, corrections in the file), not "
                                  "measured in this run")
        table = {
            k: {"ms_per_launch": round(v, 5), "launches_per_step": stage_calls.get(k, 1.0), "kernels_in_stage": (2 if n_parts > 0 else 3) if k in composite else 1,
                "algorithmic_MB": round(per_kernel[k] / 1e6, 3), "GBps": round(per_kernel[k] / (v * 1e-3) / 1e9, 1)}
            for k, v in sorted(kernels.items(), key=lambda kv: -kv[1])
        }
        moved = sum(per_kernel[k] * stage_calls.get(k, 1.0) for k in kernels)
        out = line
        out.update({
            "host": host_identification(),
            "roofline": {
                "bound": "hbm",
                "kernel": dom,
                "kernel_name": dom_family,
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": per_kernel[dom],
                "kernel_ms": kernels[dom],
                # The dominant launch is the pair sum co-scheduled with the spread.  It is bound by instruction issue and by
                # workgroup slots, not by bandwidth (profiles/r02_*_sq_counters.txt, r02_experiments.txt
                # item 10): over the round its bytes fell faster than its time -- 4-byte entries (-38 MB), distances no longer
                # stored (-19 MB) -- so `frac` fell while the kernel got faster.  For continuity with round 1's line: the same
                # launch time against the bytes of the formats it replaced (8-byte entries, distances stored).
                "note": "issue- and slot-bound pair sum, not HBM-bound; bytes cut this round (4-byte entries, distances kept in "
                        "registers) faster than time",
                "frac_at_round1_byte_accounting": ((per_kernel[dom] + 2 * w.n_pairs * (8 - getattr(ops, "FUSED_ENTRY_BYTES", 8))
                                                    + (0 if args.store_distances else w.n_pairs * s))
                                                   / (kernels[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS) if "rspace" in dom else None,
            },
            "roofline_valu": valu_roofline(w, dom, kernels[dom], dom_family),
            # whole step: bytes the kernels of this build move in their own formats (sum of the per-kernel figures below)
            # against the step time; SURVEY 8(d)'s figure for the reference's unfused formats is given for orientation only
            "step_bytes": {
                "moved_GB": moved / 1e9,
                "hbm_frac_moved": moved / (ms_per_step / n_frames * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "survey_reference_formats_GB": step_bytes / 1e9,
            },
            "kernels": table,
            "abi_call_ms": prof,
            "energy": float(E[0].item()),
            "accuracy": accuracy,
        })
        if world == 1 and n_frames == 1 and not args.no_list_refresh:
            try:
                out["list_refresh"] = list_refresh_timing(frame, ms_per_step_median)
                out["md_amortized_ms_per_step"] = out["list_refresh"]["md_amortized_ms_per_step"]
            except Exception as exc:  # e.g. more than 2^22 atoms: say so instead of losing the line
                out["list_refresh"] = {"error": f"{type(exc).__name__}: {exc}"}
        if world == 1 and not args.no_drop_in:
            out["drop_in"] = drop_in_timing(frame)
        if world == 1 and n_frames == 1 and not args.no_contract and not args.no_drop_in:
            try:
                out["contract"] = contract_timing(frame, args.workload)
            except Exception as exc:  # noqa: BLE001  (keep the line)
                out["contract"] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
        # (last of the GPU blocks: eager loops that run after it see an occasional 80 ms call -- not a device allocation, not a poll of
        # ours; with the block at the end nothing is timed behind it)
        if world == 1 and n_frames == 1 and not args.no_frames_block and not args.no_drop_in:
            try:
                out["frames"] = frames_timing(args.workload, device)
            except Exception as exc:  # noqa: BLE001  (keep the line)
                out["frames"] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
        if world == 1 and n_frames == 1 and not args.no_second_order and not args.no_drop_in:
            try:
                out["second_order"] = second_order_timing(frame)
            except Exception as exc:  # noqa: BLE001  (keep the line)
                out["second_order"] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(w)
        print(json.dumps(out))
    close()


if __name__ == "__main__":
    main()
