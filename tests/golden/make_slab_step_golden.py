"""Generate tests/golden/slab_step.npz from the reference implementation on the CPU: 2-D periodic (slab) systems.

    python tests/golden/make_slab_step_golden.py /path/to/reference/checkout

Every case is one system that is periodic along two cell vectors only (``periodic`` with one False), evaluated by the
reference's mesh calculators with ``periodic=``: per-atom potentials V, E = sum q V, and the gradients of E w.r.t.
positions, charges and the cell (one cell tensor for the mesh part and for d = |r_j - r_i + S cell|), in float64 and in
float32, plus the reference's own fp32-against-fp64 spread (max |f32 - f64|) of every quantity.

Cases (``names``): mesh 32 x 32 x 64 with the 64 along the non-periodic axis, cutoff 5, a few hundred atoms
  ortho_ax{0,1,2}_{neutral,charged}   orthorhombic cell, atoms in the middle half of the non-periodic axis, P3M (5 nodes)
  ortho_ax2_charged_pme               the same system as ortho_ax2_charged with PME (4 nodes)
  tric_ax2_charged                    triclinic cell whose cell[2] is not along z: z is Cartesian, L = |cell[2]|; P3M (4 nodes)
  lumpy_ax2_charged                   400 atoms in an eighth of the axis, away from the origin: more atoms per mesh brick than a
                                      brick has slots (overflow region), bricks without atoms, brick 0 among them
Keys per case: <name>_{cell,positions,charges,pairs,shifts,axis,method,nodes} and <name>_{V,E,gpos,gq,gcell}_{f64,f32},
<name>_spread_{V,E,gpos,gq,gcell}; ``smearing``, ``mesh_spacing``, ``cutoff``.  The pair lists come from this package's
``neighbor_list`` with the case's ``periodic``.  Data only.
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TORCHPME_REFERENCE", "../torch-pme")

# ---- import the reference with the two stubs it needs in this checkout ----
_v = types.ModuleType("torchpme._version")
_v.__version__ = "0.0.0"
_v.__version_tuple__ = (0, 0, 0)
sys.modules["torchpme._version"] = _v
_ves = types.ModuleType("vesin")
_ves.NeighborList = object
sys.modules["vesin"] = _ves
sys.path.insert(0, os.path.join(REF, "src"))
import torchpme  # noqa: E402

_spec = importlib.util.spec_from_file_location("_nl", os.path.join(ROOT, "torch-pme_amd", "neighbors.py"))
_nl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_nl)
neighbor_list = _nl.neighbor_list

CUTOFF, SMEARING, SPACING = 5.0, 1.2, 1.5
LONG, SHORT = 36.0, (20.0, 22.0)  # 2 L / h + 1 = 49 -> 64 points; 27.7, 30.3 -> 32 points


def layer(rng, grid, lo, hi):
    """Fractional coordinates of a jittered lattice: ``grid`` = sites per axis, the last axis confined to [lo, hi)."""
    g = np.stack(np.meshgrid(*[(np.arange(n) + 0.5) / n for n in grid], indexing="ij"), -1).reshape(-1, 3)
    g += rng.uniform(-0.25, 0.25, g.shape) / np.array(grid)
    g[:, 2] = lo + (hi - lo) * g[:, 2]
    return g


def charges(rng, n, net):
    q = rng.normal(size=(n, 1))
    q -= q.mean()
    return q + net / n


def systems(rng):
    out = {}
    for axis in range(3):
        lengths = [0.0, 0.0, 0.0]
        others = [d for d in range(3) if d != axis]
        lengths[axis], lengths[others[0]], lengths[others[1]] = LONG, SHORT[0], SHORT[1]
        frac = layer(rng, (6, 6, 8), 0.25, 0.75)  # 288 atoms
        order = others + [axis]
        f = np.empty_like(frac)
        f[:, order] = frac
        cell = np.diag(lengths)
        for tag, net in (("neutral", 0.0), ("charged", 3.0)):
            out[f"ortho_ax{axis}_{tag}"] = dict(cell=cell, positions=f @ cell, charges=charges(rng, len(f), net), axis=axis,
                                                method="p3m", nodes=5)
    s = out["ortho_ax2_charged"]
    out["ortho_ax2_charged_pme"] = dict(s, method="pme", nodes=4)
    cell = np.array([[20.0, 0.0, 0.0], [3.0, 22.0, 0.0], [4.0, 5.0, 34.0]])
    f = layer(rng, (6, 6, 8), 0.25, 0.75)
    out["tric_ax2_charged"] = dict(cell=cell, positions=f @ cell, charges=charges(rng, len(f), -2.0), axis=2, method="p3m", nodes=4)
    cell = np.diag([SHORT[0], SHORT[1], LONG])
    f = layer(rng, (10, 10, 4), 0.5, 0.625)  # 400 atoms in ONE of the eight layers of bricks along z, 25 per brick
    out["lumpy_ax2_charged"] = dict(cell=cell, positions=f @ cell, charges=charges(rng, len(f), 1.5), axis=2, method="p3m", nodes=5)
    return out


def evaluate(s, dtype):
    q = torch.tensor(s["charges"], dtype=dtype, requires_grad=True)
    pos = torch.tensor(s["positions"], dtype=dtype, requires_grad=True)
    cell = torch.tensor(s["cell"], dtype=dtype, requires_grad=True)
    idx = torch.tensor(s["pairs"], dtype=torch.int64)
    S = torch.tensor(s["shifts"], dtype=dtype)
    periodic = torch.tensor([d != s["axis"] for d in range(3)])
    pot = torchpme.CoulombPotential(smearing=SMEARING)
    if s["method"] == "p3m":
        calc = torchpme.P3MCalculator(pot, mesh_spacing=SPACING, interpolation_nodes=s["nodes"])
    else:
        calc = torchpme.PMECalculator(pot, mesh_spacing=SPACING, interpolation_nodes=s["nodes"])
    calc = calc.to(dtype)
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + S @ cell, dim=1)
    V = calc(q, cell, pos, idx, d, periodic=periodic)
    E = (q * V).sum()
    E.backward()
    return dict(V=V.detach().numpy(), E=E.detach().numpy().reshape(1), gpos=pos.grad.numpy(), gq=q.grad.numpy(),
                gcell=cell.grad.numpy())


def main():
    rng = np.random.default_rng(20261018)
    out = dict(smearing=SMEARING, mesh_spacing=SPACING, cutoff=CUTOFF)
    names = []
    for name, s in systems(rng).items():
        periodic = tuple(d != s["axis"] for d in range(3))
        pairs, shifts, _ = neighbor_list(s["positions"], s["cell"], CUTOFF, periodic=periodic)
        assert np.all(shifts[:, s["axis"]] == 0)
        s["pairs"], s["shifts"] = pairs.astype(np.int32), shifts.astype(np.int8)
        ns = torchpme.lib.kvectors.get_ns_mesh(torch.tensor(s["cell"]), SPACING).tolist()
        assert sorted(ns) == [32, 32, 64] and ns[s["axis"]] == 64, ns
        names.append(name)
        for k in ("cell", "positions", "charges", "pairs", "shifts"):
            out[f"{name}_{k}"] = s[k]
        out[f"{name}_axis"], out[f"{name}_method"], out[f"{name}_nodes"] = s["axis"], s["method"], s["nodes"]
        r64, r32 = evaluate(s, torch.float64), evaluate(s, torch.float32)
        line = []
        for key in r64:
            out[f"{name}_{key}_f64"] = r64[key]
            out[f"{name}_{key}_f32"] = r32[key].astype(np.float32)
            spread = float(np.abs(r32[key].astype(np.float64) - r64[key]).max())
            # a spread of zero would make the bound of the fp32 test (5 x spread) vacuous
            assert spread > 0.0, (name, key)
            out[f"{name}_spread_{key}"] = spread
            line.append(f"{key} {spread:.2e}/{np.abs(r64[key]).max():.2e}")
        print(f"{name}: N={len(s['charges'])} P={len(pairs)} Q={s['charges'].sum():+.2f} mesh={ns} spread/scale: " + ", ".join(line))
    out["names"] = np.array(names)
    path = os.path.join(HERE, "slab_step.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"wrote {path}: {size} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
