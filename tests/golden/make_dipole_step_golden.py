"""Generate tests/golden/dipole_step.npz from the reference implementation (CalculatorDipole / PotentialDipole) on the CPU.

    python tests/golden/make_dipole_step_golden.py /path/to/reference/checkout

What GraphedDipoleStep returns, computed by the reference: E = sum mu . V and the gradients of E w.r.t. dipoles, positions and
cell -- totals, through vectors = pos[j] - pos[i] + S cell built inside the autograd graph -- in fp64 and fp32 (the fp32 arrays
are stored as float32), plus sum_i |mu_i . V_i| (the scale of the rounding error of the scalar E).

Contents (``<case>_<field>`` keys):
  tric_<variant>_*  24 atoms in the triclinic cell of dipole.npz with the potentials of its variants (half, full, direct, excl1,
                    excl3, eps, pref); lr_wavelength 0.5 gives meshes 15 x 14 x 16: odd and even counts, so there are -n/2
                    planes whose k-vectors have no mirror in the grid
  big_{half,full}_* 300 atoms in a cubic cell of 20 A: a dense block of 252 atoms and 48 atoms farther than the cutoff from
                    everything (rows without a pair next to rows of more than 32 entries; 300 is more than the 256-atom tile
                    of the structure kernel and no multiple of the 16 rows of a row block); lr_wavelength 1.25 gives
                    16^3 = 4096 k-vectors.  Only the half list is stored: the full list is the half list followed by its
                    mirror (j, i, -S), which is how the test builds it.
The three ESPResSo frames of dipole.npz were generated with g = mu already and are used from there.
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
from torchpme.prefactors import eV_A  # noqa: E402

_spec = importlib.util.spec_from_file_location("_nl", os.path.join(ROOT, "torch-pme_amd", "neighbors.py"))
_nl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_nl)
neighbor_list = _nl.neighbor_list


def evaluate(calc, dtype, mu, pos, cell, pairs, shifts):
    """E = sum mu . V and its gradients w.r.t. dipoles, positions and cell (totals)."""
    calc = calc.to(dtype=dtype)
    tm = torch.tensor(mu, dtype=dtype, requires_grad=True)
    tp = torch.tensor(pos, dtype=dtype, requires_grad=True)
    tc = torch.tensor(cell, dtype=dtype, requires_grad=True)
    ti = torch.tensor(pairs, dtype=torch.int64)
    vec = tp[ti[:, 1]] - tp[ti[:, 0]] + torch.tensor(shifts, dtype=dtype) @ tc
    V = calc(dipoles=tm, cell=tc, positions=tp, neighbor_indices=ti, neighbor_vectors=vec)
    per_atom = (V * tm).sum(dim=1)
    E = per_atom.sum()
    E.backward()
    out_dtype = np.float64 if dtype == torch.float64 else np.float32
    res = {"E": np.asarray(E.detach().numpy(), dtype=out_dtype), "gmu": tm.grad.numpy().astype(out_dtype),
           "gpos": tp.grad.numpy().astype(out_dtype), "gcell": tc.grad.numpy().astype(out_dtype)}
    if dtype == torch.float64:
        res["absE"] = float(per_atom.detach().abs().sum())
    return res


def store(out, prefix, res, tag):
    for k, v in res.items():
        out[f"{prefix}_{k}" if k == "absE" else f"{prefix}_{k}_{tag}"] = np.asarray(v)


def run_case(out, prefix, kw, full, lam, mu, pos, cell, pairs, shifts):
    calc = torchpme.CalculatorDipole(torchpme.PotentialDipole(**kw), full_neighbor_list=full, lr_wavelength=lam)
    out[f"{prefix}_full"], out[f"{prefix}_lr_wavelength"] = full, np.nan if lam is None else lam
    for key in ("smearing", "exclusion_radius", "epsilon", "prefactor"):
        out[f"{prefix}_{key}"] = np.nan if kw.get(key) is None else kw[key]
    out[f"{prefix}_exclusion_degree"] = kw.get("exclusion_degree", 1)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        store(out, prefix, evaluate(calc, dtype, mu, pos, cell, pairs, shifts), tag)
    print(f"{prefix}: P={len(pairs)} E={float(out[prefix + '_E_f64']):.10f} (fp32 {float(out[prefix + '_E_f32']):.7f})")


def main():
    out = {}
    # ---- case 1: the triclinic cell of dipole.npz, the energy (g = mu) this time
    rng = np.random.default_rng(11)
    cell = np.array([[7.1, 0.0, 0.0], [1.3, 6.6, 0.0], [-0.9, 1.1, 7.4]])
    n = 24
    pos = rng.uniform(0, 1, (n, 3)) @ cell
    mu = rng.normal(size=(n, 3))
    cutoff = 3.6
    out["tric_cell"], out["tric_positions"], out["tric_dipoles"], out["tric_cutoff"] = cell, pos, mu, cutoff
    variants = {  # name: (potential kwargs, full list, lr_wavelength)
        "half": (dict(smearing=1.0), False, 0.5),
        "full": (dict(smearing=1.0), True, 0.5),
        "direct": (dict(), False, None),
        "excl1": (dict(smearing=1.0, exclusion_radius=2.5, exclusion_degree=1), False, 0.5),
        "excl3": (dict(smearing=1.0, exclusion_radius=2.5, exclusion_degree=3), False, 0.5),
        "eps": (dict(smearing=0.9, epsilon=2.5), False, 0.5),
        "pref": (dict(smearing=1.1, prefactor=eV_A), True, 0.5),
    }
    assert list(np.ceil(np.linalg.norm(cell, axis=1) / 0.5).astype(int)) == [15, 14, 16]
    for name, (kw, full, lam) in variants.items():
        pairs, shifts, _ = neighbor_list(pos, cell, cutoff, full_list=full)
        assert np.abs(shifts).max() <= 3
        p = f"tric_{name}"
        out[f"{p}_pairs"], out[f"{p}_shifts"] = pairs.astype(np.int16), shifts.astype(np.int8)
        run_case(out, p, kw, full, lam, mu, pos, cell, pairs, shifts)
    out["tric_variants"] = np.array(list(variants))

    # ---- case 2: 300 atoms, a dense block and isolated atoms
    rng = np.random.default_rng(12)
    L, cutoff, lam = 20.0, 3.5, 1.25
    cell = L * np.eye(3)
    g = np.arange
    block = np.stack(np.meshgrid(1.0 + 1.6 * g(6), 1.0 + 1.6 * g(6), 1.0 + 1.6 * g(7), indexing="ij"), -1).reshape(-1, 3)
    lone = np.stack(np.meshgrid(np.array([13.0, 17.0]), 1.0 + 4.0 * g(5), 1.0 + 4.0 * g(5), indexing="ij"), -1).reshape(-1, 3)[:48]
    pos = np.concatenate([block, lone]) + rng.uniform(-0.2, 0.2, (300, 3))
    pos = pos[rng.permutation(300)]  # (the lone atoms anywhere in the index range)
    mu = rng.normal(size=(300, 3))
    pairs, shifts, _ = neighbor_list(pos, cell, cutoff, full_list=False)
    rows = np.bincount(pairs.reshape(-1), minlength=300)  # entries per row of the transposed half list
    assert (rows == 0).sum() >= 1 and rows.max() > 32, (int((rows == 0).sum()), int(rows.max()))
    assert np.abs(shifts).max() <= 3
    assert int(np.prod(np.ceil(np.linalg.norm(cell, axis=1) / lam))) >= 4096
    out["big_cell"], out["big_positions"], out["big_dipoles"], out["big_cutoff"] = cell, pos, mu, cutoff
    out["big_pairs"], out["big_shifts"] = pairs.astype(np.int16), shifts.astype(np.int8)
    print(f"big: P={len(pairs)} empty rows {int((rows == 0).sum())} longest row {int(rows.max())}")
    kw = dict(smearing=1.2, epsilon=1.5)
    run_case(out, "big_half", kw, False, lam, mu, pos, cell, pairs, shifts)
    run_case(out, "big_full", kw, True, lam, mu, pos, cell, np.concatenate([pairs, pairs[:, ::-1]]),
             np.concatenate([shifts, -shifts]))

    path = os.path.join(HERE, "dipole_step.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
