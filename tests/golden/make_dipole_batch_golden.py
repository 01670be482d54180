"""Generate tests/golden/dipole_batch.npz from the reference implementation (CalculatorDipole / PotentialDipole) on the CPU.

    python tests/golden/make_dipole_batch_golden.py /path/to/reference/checkout

What GraphedDipoleBatch returns for six frames and three calculators, computed by the reference frame by frame with `evaluate`
of make_dipole_cell_step_golden.py (E = sum mu . V and its total gradients w.r.t. dipoles, positions and cell), in fp64 and fp32
(the fp32 arrays stored as float32), at the frame's cell (``c0``) and at the strained cell ``cell (I + EPS)`` with the positions
scaled along (``c1``), plus sum_i |mu_i . V_i| per case (``absE``).  lr_wavelength is 1.25 throughout.

Calculators:
  D1 = PotentialDipole(smearing=1.0), half lists
  D2 = PotentialDipole(smearing=1.2, exclusion_radius=2.5, exclusion_degree=3, epsilon=1.5, prefactor=14.399645478425667), full
       lists: the half list followed by its mirror (j, i, -S); f3 has a stored full list of its own
  D3 = PotentialDipole() (direct), lr_wavelength=None, half lists, frames f1..f4 only
Frames:
  f0  1 atom in a cubic cell of edge 1.2, empty list (the geometry of ewald_batch.npz f0): the grid is (1, 1, 1) at both cells
      (asserted), so n_k = 0
  f1  the 2-atom triclinic frame of ewald_batch.npz with its one shifted pair, grid (3, 3, 3)
  f2  the 17-atom orthorhombic frame of ewald_batch.npz, grid (4, 9, 6): no multiple of the 16 rows of a row block
  f3  the 24-atom triclinic system and dipoles of dipole_step.npz with its lists tric_half / tric_full, grid (6, 6, 7)
  f4  the 300-atom system and dipoles of dipole_cell_step.npz (big_*), grid 16^3: at least 2 048 compacted k-vectors, two slices
      of the atom launch; rows without a pair beside rows of more than 32 entries
  f5  3 atoms in a cubic cell of edge 40.6, two of them 2 apart, a half list of that one pair; grid 33^3 = 17 968 compacted
      k-vectors, 17 slices: the lanes of the finish launch walk more than 16 slices
Every grid is the same at c0 and c1 (asserted).  The systems of f0..f4 are READ from the files named and not stored again; only
the new dipoles (f0, f1, f2, f5), the geometry of f5 and the results are.  Keys: ``f<n>_dipoles``, ``f5_{cell,positions,
pairs_half,shifts_half}``; per calculator ``<D>_frames`` (the frames it serves) and, with those frames one behind the other,
``<D>_E_<c0|c1>_<f64|f32>`` (F,), ``<D>_gmu_...`` and ``<D>_gpos_...`` (sum N, 3), ``<D>_gcell_...`` (F, 3, 3) and
``<D>_absE_<c0|c1>`` (F,).
"""

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_cell_step_golden", os.path.join(HERE, "make_dipole_cell_step_golden.py"))
_step = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_step)  # (imports the reference named on the command line, with the stubs it needs)
run_at, ns_of, EPS = _step.run_at, _step.ns_of, _step.EPS
LAM = 1.25

CALCS = {  # name: (potential, full list, lr_wavelength, frames)
    "D1": (dict(smearing=1.0), False, LAM, range(6)),
    "D2": (dict(smearing=1.2, exclusion_radius=2.5, exclusion_degree=3, epsilon=1.5, prefactor=14.399645478425667), True, LAM,
           range(6)),
    "D3": (dict(), False, None, range(1, 5)),
}
GRIDS = [[1, 1, 1], [3, 3, 3], [4, 9, 6], [6, 6, 7], [16, 16, 16], [33, 33, 33]]


def mirrored(pairs, shifts):
    return np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])


def systems(out):
    """[(dipoles, positions, cell, half list, full list)] of the six frames; a list is (pairs, shifts).  New data goes to `out`."""
    eb = np.load(os.path.join(HERE, "ewald_batch.npz"))
    ds = np.load(os.path.join(HERE, "dipole_step.npz"))
    dcs = np.load(os.path.join(HERE, "dipole_cell_step.npz"))
    rng = np.random.default_rng(41)
    g = lambda a: a.astype(np.int64)  # noqa: E731
    frames = []
    for n in range(3):  # f0..f2: the geometry of ewald_batch.npz, new dipoles
        pos = eb[f"f{n}_positions"]
        mu = out[f"f{n}_dipoles"] = rng.normal(size=pos.shape)
        half = (g(eb[f"f{n}_pairs_half"]).reshape(-1, 2), g(eb[f"f{n}_shifts_half"]).reshape(-1, 3))
        frames.append((mu, pos, eb[f"f{n}_cell"], half, mirrored(*half)))
    frames.append((ds["tric_dipoles"], ds["tric_positions"], ds["tric_cell"], (g(ds["tric_half_pairs"]), g(ds["tric_half_shifts"])),
                   (g(ds["tric_full_pairs"]), g(ds["tric_full_shifts"]))))
    half = (g(dcs["big_pairs"]), g(dcs["big_shifts"]))
    frames.append((dcs["big_dipoles"], dcs["big_positions"], dcs["big_cell"], half, mirrored(*half)))
    # f5: three atoms in a large cell, one pair
    cell = 40.6 * np.eye(3)
    pos = np.array([[3.0, 4.0, 5.0], [3.0, 4.0, 7.0], [22.0, 30.5, 11.0]])
    mu = rng.normal(size=(3, 3))
    half = (np.array([[0, 1]]), np.array([[0, 0, 0]]))
    assert abs(np.linalg.norm(pos[1] - pos[0]) - 2.0) < 1e-12
    out["f5_cell"], out["f5_positions"], out["f5_dipoles"] = cell, pos, mu
    out["f5_pairs_half"], out["f5_shifts_half"] = half[0].astype(np.int16), half[1].astype(np.int8)
    frames.append((mu, pos, cell, half, mirrored(*half)))
    strain = np.eye(3) + EPS
    for n, fr in enumerate(frames):
        assert ns_of(fr[2], LAM) == GRIDS[n] and ns_of(fr[2] @ strain, LAM) == GRIDS[n], (n, ns_of(fr[2], LAM), ns_of(fr[2] @ strain, LAM))
    return frames


def main():
    out = {}
    strain = np.eye(3) + EPS
    frames = systems(out)
    for cname, (kw, is_full, lam, served) in CALCS.items():
        raw = {}
        for n in served:
            mu, pos, cell, half, full = frames[n]
            pairs, shifts = full if is_full else half
            for ctag, c, p in (("c0", cell, pos), ("c1", cell @ strain, pos @ strain)):
                run_at(raw, f"{cname}_f{n}", ctag, kw, is_full, lam, mu, p, c, pairs.reshape(-1, 2), shifts.reshape(-1, 3))
        # one array per result, the served frames one behind the other (a zip member per frame and result costs more than it holds)
        out[f"{cname}_frames"] = np.array(list(served))
        for ctag in ("c0", "c1"):
            out[f"{cname}_absE_{ctag}"] = np.array([raw[f"{cname}_f{n}_absE_{ctag}"] for n in served])
            for tag in ("f64", "f32"):
                key = lambda field, n: raw[f"{cname}_f{n}_{field}_{ctag}_{tag}"]  # noqa: E731
                out[f"{cname}_E_{ctag}_{tag}"] = np.array([key("E", n) for n in served])
                out[f"{cname}_gcell_{ctag}_{tag}"] = np.stack([key("gcell", n) for n in served])
                for field in ("gmu", "gpos"):
                    out[f"{cname}_{field}_{ctag}_{tag}"] = np.concatenate([key(field, n) for n in served])
                assert out[f"{cname}_E_{ctag}_{tag}"].dtype == (np.float64 if tag == "f64" else np.float32)
    path = os.path.join(HERE, "dipole_batch.npz")
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(HERE, "dipole_cell_step.npz"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes (dipole_cell_step.npz: {limit})")
    assert os.path.getsize(path) < limit


if __name__ == "__main__":
    main()
