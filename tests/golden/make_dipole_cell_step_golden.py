"""Generate tests/golden/dipole_cell_step.npz from the reference implementation (CalculatorDipole / PotentialDipole) on the CPU.

    python tests/golden/make_dipole_cell_step_golden.py /path/to/reference/checkout

What GraphedDipoleStep(follow_cell=True) returns, computed by the reference: E = sum mu . V and the gradients of E w.r.t. dipoles,
positions and cell -- totals, through vectors = pos[j] - pos[i] + S cell built inside the autograd graph -- in fp64 and fp32 (the
fp32 arrays are stored as float32), plus sum_i |mu_i . V_i| (the scale of the rounding error of the scalar E).  Every case is
stored at its cell (``c0``) AND at the strained cell ``cell1 = cell0 (I + eps)`` (``c1``, eps the strain of
make_ewald_step_golden.py) with the same list and shifts and the positions scaled along with the cell: the step follows the cell
without a new capture, and both ends are checked against the reference.

Contents (``<case>_<field>`` keys, ``<case>_<field>_<c0|c1>_<f64|f32>`` for results):
  tric_<variant>_*  the 24 atoms, the triclinic cell, the lists and the seven potentials of dipole_step.npz (half, full, direct,
                    excl1, excl3, eps, pref; read from that file); lr_wavelength 0.5 gives ns = (15, 14, 16) at both cells
                    (asserted)
  big_{half,full}_* 300 atoms in a cubic cell of 19.4: a dense block of 252 atoms and 48 atoms farther than the cutoff from
                    everything (rows without a pair next to rows of more than 32 entries); lr_wavelength 1.25 gives ns = 16^3
                    at both cells (asserted; at 20.0 |a| / lambda is exactly 16 and the strained cell has (17, 16, 17)).  Only
                    the half list is stored: the full list is the half list followed by its mirror (j, i, -S).
  kept_*            tric_half at 1.2 cell with the positions x 1.2, evaluated by the reference with lr_wavelength 0.6: |a_d| /
                    lambda = 14.2, 13.45, 15.07, the grid (15, 14, 16) of the construction cell (asserted) -- what a step built
                    at `cell` returns at 1.2 cell, where the eager call with lr_wavelength 0.5 would sum (18, 17, 19).
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

EPS = np.array([[0.012, 0.004, -0.003], [0.004, -0.009, 0.005], [-0.003, 0.005, 0.007]])  # (make_ewald_step_golden.py)
PARAMS = ("smearing", "exclusion_radius", "epsilon", "prefactor")


def ns_of(cell, lam):
    return [int(n) for n in np.ceil(np.linalg.norm(cell, axis=1) / lam)]


def evaluate(kw, full, lam, dtype, mu, pos, cell, pairs, shifts):
    """E = sum mu . V and its gradients w.r.t. dipoles, positions and cell (totals)."""
    # (a calculator of its own per run: `.to(float32)` rounds the potential's buffers for good)
    calc = torchpme.CalculatorDipole(torchpme.PotentialDipole(**kw), full_neighbor_list=full, lr_wavelength=lam).to(dtype=dtype)
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


def run_at(out, prefix, ctag, kw, full, lam, mu, pos, cell, pairs, shifts):
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        for k, v in evaluate(kw, full, lam, dtype, mu, pos, cell, pairs, shifts).items():
            out[f"{prefix}_absE_{ctag}" if k == "absE" else f"{prefix}_{k}_{ctag}_{tag}"] = np.asarray(v)
    print(f"{prefix} {ctag}: P={len(pairs)} E={float(out[f'{prefix}_E_{ctag}_f64']):.10f} "
          f"(fp32 {float(out[f'{prefix}_E_{ctag}_f32']):.7f})")


def run_case(out, prefix, kw, full, lam, mu, pos, cell, pairs, shifts):
    out[f"{prefix}_full"], out[f"{prefix}_lr_wavelength"] = full, np.nan if lam is None else lam
    for key in PARAMS:
        out[f"{prefix}_{key}"] = np.nan if kw.get(key) is None else kw[key]
    out[f"{prefix}_exclusion_degree"] = kw.get("exclusion_degree", 1)
    strain = np.eye(3) + EPS
    for ctag, c, p in (("c0", cell, pos), ("c1", cell @ strain, pos @ strain)):
        run_at(out, prefix, ctag, kw, full, lam, mu, p, c, pairs, shifts)


def main():
    out = {"strain": EPS}
    strain = np.eye(3) + EPS
    # ---- case 1: the triclinic system of dipole_step.npz with its seven potentials
    src = np.load(os.path.join(HERE, "dipole_step.npz"))
    cell, pos, mu = src["tric_cell"], src["tric_positions"], src["tric_dipoles"]
    out["tric_cell"], out["tric_positions"], out["tric_dipoles"] = cell, pos, mu
    assert ns_of(cell, 0.5) == [15, 14, 16] and ns_of(cell @ strain, 0.5) == [15, 14, 16]
    out["tric_ns"] = np.array([15, 14, 16])
    variants = [str(n) for n in src["tric_variants"]]
    assert variants == ["half", "full", "direct", "excl1", "excl3", "eps", "pref"]
    for name in variants:
        p = f"tric_{name}"
        kw = {key: float(src[f"{p}_{key}"]) for key in PARAMS if not np.isnan(float(src[f"{p}_{key}"]))}
        kw["exclusion_degree"] = int(src[f"{p}_exclusion_degree"])
        lam = float(src[f"{p}_lr_wavelength"])
        lam = None if np.isnan(lam) else lam
        assert lam in (None, 0.5)
        pairs, shifts = src[f"{p}_pairs"].astype(np.int64), src[f"{p}_shifts"].astype(np.int64)
        out[f"{p}_pairs"], out[f"{p}_shifts"] = pairs.astype(np.int16), shifts.astype(np.int8)
        run_case(out, p, kw, bool(src[f"{p}_full"]), lam, mu, pos, cell, pairs, shifts)
    out["tric_variants"] = np.array(variants)

    # ---- the kept grid: tric_half at 1.2 cell, summed over the grid of the construction cell
    big_cell = 1.2 * cell
    assert ns_of(big_cell, 0.6) == [15, 14, 16] and ns_of(big_cell, 0.5) == [18, 17, 19]
    np.testing.assert_allclose(np.linalg.norm(big_cell, axis=1) / 0.6, [14.2, 13.45, 15.07], atol=0.01)
    out["kept_scale"], out["kept_lr_wavelength"], out["kept_ns"] = 1.2, 0.6, np.array([15, 14, 16])
    run_at(out, "kept", "c0", dict(smearing=1.0), False, 0.6, mu, 1.2 * pos, big_cell, src["tric_half_pairs"].astype(np.int64),
           src["tric_half_shifts"].astype(np.int64))

    # ---- case 2: 300 atoms, a dense block and isolated atoms (the geometry of make_ewald_step_golden.py)
    rng = np.random.default_rng(32)
    L, cutoff, lam = 19.4, 3.3, 1.25
    cell = L * np.eye(3)
    g = np.arange
    block = np.stack(np.meshgrid(1.0 + 1.5 * g(6), 1.0 + 1.5 * g(6), 1.0 + 1.5 * g(7), indexing="ij"), -1).reshape(-1, 3)
    lone = np.stack(np.meshgrid(np.array([12.9, 16.4]), 1.0 + 3.8 * g(5), 1.0 + 3.8 * g(5), indexing="ij"), -1).reshape(-1, 3)[:48]
    pos = np.concatenate([block + rng.uniform(-0.2, 0.2, (252, 3)), lone + rng.uniform(-0.05, 0.05, (48, 3))])
    pos = pos[rng.permutation(300)]  # (the lone atoms anywhere in the index range)
    mu = rng.normal(size=(300, 3))
    pairs, shifts, _ = neighbor_list(pos, cell, cutoff, full_list=False)
    rows = np.bincount(pairs.reshape(-1), minlength=300)  # entries per row of the transposed half list
    assert (rows == 0).sum() == 48 and rows.max() > 32, (int((rows == 0).sum()), int(rows.max()))
    assert np.abs(shifts).max() <= 3
    assert ns_of(cell, lam) == [16, 16, 16] and ns_of(cell @ strain, lam) == [16, 16, 16]
    out["big_ns"] = np.array([16, 16, 16])
    out["big_cell"], out["big_positions"], out["big_dipoles"], out["big_cutoff"] = cell, pos, mu, cutoff
    out["big_pairs"], out["big_shifts"] = pairs.astype(np.int16), shifts.astype(np.int8)
    print(f"big: P={len(pairs)} empty rows {int((rows == 0).sum())} longest row {int(rows.max())}")
    kw = dict(smearing=1.2, epsilon=1.5)
    run_case(out, "big_half", kw, False, lam, mu, pos, cell, pairs, shifts)
    run_case(out, "big_full", kw, True, lam, mu, pos, cell, np.concatenate([pairs, pairs[:, ::-1]]),
             np.concatenate([shifts, -shifts]))

    path = os.path.join(HERE, "dipole_cell_step.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
