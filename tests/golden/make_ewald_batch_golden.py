"""Generate tests/golden/ewald_batch.npz from the reference implementation (EwaldCalculator) on the CPU.

    python tests/golden/make_ewald_batch_golden.py /path/to/reference/checkout

What GraphedEwaldBatch returns for five frames and two calculators, computed by the reference frame by frame with `evaluate` of
make_ewald_step_golden.py (E = (q . V).sum() and its total gradients w.r.t. charges, positions and cell), in fp64 and fp32, at
the frame's cell (``c0``) and at the strained cell ``cell (I + EPS)`` with the positions scaled along (``c1``), plus
sum_a |q_a V_a| per case (``absE``).  lr_wavelength is 1.25 as there.

Calculators:  C1 = CoulombPotential(smearing=1.0), half lists;  C2 = InversePowerLawPotential(6, smearing=0.9), full lists.
Frames:
  f0  1 atom in a cubic cell of edge 1.2, empty list: the grid is (1, 1, 1) at both cells (asserted), so n_k = 0, N = 1, P = 0
  f1  2 atoms in a small triclinic cell, one pair with a non-zero shift (the full list: the pair and its mirror)
  f2  17 atoms in an orthorhombic cell, ns = (4, 9, 6) at both cells (asserted): no multiple of the 16 rows of a row block
  f3  the 24-atom triclinic system of ewald_step.npz with the charges of its `net` variant, ns = (8, 7, 9)
  f4  the 300-atom system of ewald_step.npz, 16^3 k-vectors
The systems of f3 and f4 are READ from ewald_step.npz and not stored again; only their results are.  Keys:
``f<n>_{cell,positions,charges,pairs_half,shifts_half,pairs_full,shifts_full}`` for f0..f2 and
``<C1|C2>_f<n>_<E|gq|gpos|gcell>_<c0|c1>_<f64|f32>``, ``<C1|C2>_f<n>_absE_<c0|c1>`` for all.
"""

import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_step_golden", os.path.join(HERE, "make_ewald_step_golden.py"))
_step = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_step)  # (imports the reference named on the command line, with the stubs it needs)
torchpme, evaluate, neighbor_list, ns_of, EPS, LAM = _step.torchpme, _step.evaluate, _step.neighbor_list, _step.ns_of, _step.EPS, _step.LAM

CALCS = {
    "C1": (lambda: torchpme.CoulombPotential(smearing=1.0), False),
    "C2": (lambda: torchpme.InversePowerLawPotential(exponent=6, smearing=0.9), True),
}


def mirrored(pairs, shifts):
    return np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])


def systems():
    """[(charges, positions, cell, half list, full list)] of the five frames; a list is (pairs, shifts)."""
    step = np.load(os.path.join(HERE, "ewald_step.npz"))
    strain = np.eye(3) + EPS
    out = []
    # f0: one atom, a cell shorter than the wavelength along every axis
    cell = 1.2 * np.eye(3)
    assert ns_of(cell, LAM) == [1, 1, 1] and ns_of(cell @ strain, LAM) == [1, 1, 1]
    empty = (np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3), dtype=np.int64))
    out.append((np.array([[0.7]]), np.array([[0.3, 0.5, 0.9]]), cell, empty, empty))
    # f1: two atoms, the pair across the a face
    cell = np.array([[2.6, 0.0, 0.0], [0.4, 2.9, 0.0], [-0.3, 0.5, 3.1]])
    pos = np.array([[0.12, 0.2, 0.3], [0.85, 0.25, 0.4]]) @ cell
    half = (np.array([[0, 1]]), np.array([[-1, 0, 0]]))
    assert np.linalg.norm(pos[1] - pos[0] + half[1][0] @ cell) < 1.5
    out.append((np.array([[0.9], [-0.4]]), pos, cell, half, mirrored(*half)))
    # f2: 17 atoms, three different grid counts
    rng = np.random.default_rng(31)
    cell = np.diag([4.9, 11.0, 7.4])
    assert ns_of(cell, LAM) == [4, 9, 6] and ns_of(cell @ strain, LAM) == [4, 9, 6]
    pos = rng.uniform(0, 1, (17, 3)) @ cell
    q = rng.normal(size=(17, 1))
    q += 0.2 - q.mean()
    lists = []
    for full in (False, True):
        pairs, shifts, _ = neighbor_list(pos, cell, 3.0, full_list=full)
        assert len(pairs) > 0 and np.abs(shifts).max() <= 3 and np.abs(shifts).max() >= 1
        lists.append((pairs.astype(np.int64), shifts.astype(np.int64)))
    out.append((q, pos, cell, lists[0], lists[1]))
    # f3, f4: from ewald_step.npz
    g = lambda k: step[k].astype(np.int64)  # noqa: E731
    assert ns_of(step["tric_cell"], LAM) == [8, 7, 9]
    out.append((step["tric_net_charges"], step["tric_positions"], step["tric_cell"], (g("tric_half_pairs"), g("tric_half_shifts")),
                (g("tric_ipl6_pairs"), g("tric_ipl6_shifts"))))
    half = (g("big_pairs"), g("big_shifts"))
    out.append((step["big_half_charges"], step["big_positions"], step["big_cell"], half, mirrored(*half)))
    return out


def main():
    out = {}
    strain = np.eye(3) + EPS
    frames = systems()
    assert sum(abs(float(fr[0].sum())) > 0.1 for fr in frames) >= 2  # a net charge in at least two frames
    for n, (q, pos, cell, half, full) in enumerate(frames):
        if n < 3:
            out[f"f{n}_cell"], out[f"f{n}_positions"], out[f"f{n}_charges"] = cell, pos, q
            out[f"f{n}_pairs_half"], out[f"f{n}_shifts_half"] = half[0].astype(np.int16), half[1].astype(np.int8)
            out[f"f{n}_pairs_full"], out[f"f{n}_shifts_full"] = full[0].astype(np.int16), full[1].astype(np.int8)
        for cname, (make, is_full) in CALCS.items():
            pairs, shifts = full if is_full else half
            for ctag, c, p in (("c0", cell, pos), ("c1", cell @ strain, pos @ strain)):
                for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                    calc = torchpme.EwaldCalculator(make(), lr_wavelength=LAM, full_neighbor_list=is_full)
                    for k, v in evaluate(calc, dtype, q, p, c, pairs.reshape(-1, 2), shifts.reshape(-1, 3)).items():
                        out[f"{cname}_f{n}_absE_{ctag}" if k == "absE" else f"{cname}_f{n}_{k}_{ctag}_{tag}"] = np.asarray(v)
                print(f"{cname} f{n} {ctag}: N={len(q)} P={len(pairs)} E={float(out[f'{cname}_f{n}_E_{ctag}_f64']):.10f} "
                      f"(fp32 {float(out[f'{cname}_f{n}_E_{ctag}_f32']):.7f})")
    path = os.path.join(HERE, "ewald_batch.npz")
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(HERE, "slab_step.npz"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes (slab_step.npz: {limit})")
    assert os.path.getsize(path) < limit


if __name__ == "__main__":
    main()
