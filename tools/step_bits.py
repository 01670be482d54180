"""The bits of the dipole step and of the combined step: one SHA-256 line per output tensor.

``GraphedDipoleStep`` runs on the systems of ``tests/test_gpu_dipole_step.py`` -- the triclinic variants, 300 atoms with a half
and a full list, 37 atoms with smearing, with exclusion and direct, the three 8-atom crystal frames against 85^3 k-vectors --
in fp64 and fp32, with and without the cell gradient.  ``GraphedCombinedStep`` runs on the systems of
``tests/test_gpu_combined_step.py`` -- the golden cases (three terms, PME and P3M, half and full lists) and the random 37 atoms
with one and with eight terms -- in fp64 and fp32, with and without the weight gradient; its lines are the outputs and the pair
forces of the row kernel, each replayed twice (the mesh part spreads with LDS atomics: a line whose two replays disagree says
so).  The pair part, the reciprocal sums of the dipole step and every block sum have a fixed order, so two runs of the same code
give the same text, and a change that only moves the device code must give the same text as its parent.  The text ends with
one ``##`` line per configuration -- the number of its lines and the SHA-256 of them -- and one for the whole: what
``profiles/step_skeleton_bits.txt`` keeps.  The systems are the tests' own, through helpers of the two test modules;
``tests/test_step_bits_host.py`` walks them without a GPU, so a rename there shows up in the suite.

    python tools/step_bits.py [output file]

``--cell-step``: ``GraphedDipoleStep(follow_cell=True)`` alone, on the same dipole systems in the same four configurations, each
system at its construction cell and, from the same graph, at cell (I + eps) with the eps of
``tests/golden/make_dipole_cell_step_golden.py``: E, F, dE/dmu, dE/dcell and the status word.  ``profiles/dipole_one_body_bits.txt``
keeps that text as the commit before the kernels of ``csrc/dipole_step.hip`` became wrappers of ``csrc/dipole_step_bodies.h`` gave it.

    python tools/step_bits.py --cell-step [output file]
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torchpme_amd as tpa  # noqa: E402
import test_gpu_combined_step as C  # noqa: E402
import test_gpu_dipole_step as D  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def dipole_systems():
    """(name, calculator, (dipoles, positions, cell, pairs, shifts)) of every system of the dipole step's tests"""
    G, F = D.GOLD, D.FRAMES
    for name in (str(n) for n in G["tric_variants"]):
        p = f"tric_{name}"
        yield p, D._calc(p), (G["tric_dipoles"], G["tric_positions"], G["tric_cell"], G[f"{p}_pairs"], G[f"{p}_shifts"])
    for full in (False, True):
        p = "big_full" if full else "big_half"
        yield p, D._calc(p), (G["big_dipoles"], G["big_positions"], G["big_cell"], *D._big_list(full))
    small = (dict(smearing=0.9, epsilon=2.0, prefactor=1.7), dict(smearing=0.9, exclusion_radius=2.4, exclusion_degree=2), dict())
    for tag, kw in zip(("smearing", "exclusion", "direct"), small):
        calc = tpa.CalculatorDipole(tpa.PotentialDipole(**kw), lr_wavelength=0.7 if kw else None)
        yield f"small37_{tag}", calc, D._small_system()
    for frame in (0, 1, 2):
        p = f"frame{frame}"
        calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=float(F[f"{p}_smearing"]), prefactor=tpa.prefactors.eV_A),
                                    lr_wavelength=0.1)
        yield p, calc, (F[f"{p}_dipoles"], F[f"{p}_positions"], F[f"{p}_cell"], F[f"{p}_pairs"], F[f"{p}_shifts"])


def strain():
    """I + eps of tests/golden/make_dipole_cell_step_golden.py: the second cell of the step that follows its cell"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dipole_cell_step.npz"))
    return np.eye(3) + gold["strain"]


def run_dipole(dtype, cell_gradient, follow_cell=False):
    """follow_cell: ``GraphedDipoleStep(follow_cell=True)`` of the same systems, each at its construction cell (c0) and then, from
    the same graph, at cell (I + eps) with the positions scaled along (c1); the status word is a line of its own"""
    head = f"dipole{'_cell' if follow_cell else ''} {str(dtype)[6:]} cg={int(cell_gradient)}"
    keys = ("E", "F", "dE/dmu", "dE/dcell")[:4 if cell_gradient else 3]
    lines = []
    for name, calc, system in dipole_systems():
        if not follow_cell:
            out = D._build(calc, dtype, *system, cell_gradient=cell_gradient)()
            torch.cuda.synchronize()
            lines += [f"{head} {name} {key} {sha(o)}" for key, o in zip(keys, out)]
            continue
        mu, pos, cell, pairs, shifts = system
        ti = torch.tensor(np.asarray(pairs, dtype=np.int64), device=D.DEV)
        step = tpa.GraphedDipoleStep(calc, D._t(mu, dtype), D._t(cell, dtype), D._t(pos, dtype), ti, D._t(shifts, dtype),
                                     cell_gradient=cell_gradient, follow_cell=True)
        for ctag, m in (("c0", np.eye(3)), ("c1", strain())):
            out = step(D._t(np.asarray(pos) @ m, dtype), cell=D._t(np.asarray(cell) @ m, dtype))
            torch.cuda.synchronize()
            lines += [f"{head} {name} {ctag} {key} {sha(o)}" for key, o in zip(keys + ("status",), (*out, step.status))]
    return lines


def combined_cases():
    """(name, system, (members, weights), calculator kind, full list)"""
    for system in ("tric", "ortho"):
        for kind in ("pme", "p3m"):
            for list_tag in ("half", "full"):
                yield f"{system}_{kind}_{list_tag}", C._golden_system(system, list_tag), C.RS, kind, list_tag == "full"
    for n_terms, terms, kind in ((1, C.ONE, "pme"), (8, C.EIGHT, "p3m")):
        for list_tag in ("half", "full"):
            yield f"random_{n_terms}_{kind}_{list_tag}", C._random_system(list_tag), terms, kind, list_tag == "full"


def run_combined(dtype, weight_gradient):
    head = f"combined {str(dtype)[6:]} wg={int(weight_gradient)}"
    lines = []
    for name, s, (members, weights), kind, full in combined_cases():
        calc = C._calculator(C._combination(members, weights, dtype), kind, full, s["spacing"])
        step = tpa.GraphedCombinedStep(calc, *C._tensors(s, dtype), weight_gradient=weight_gradient, charge_gradient=not full)
        first = [o.clone() for o in (*step(), step._pair_force)]
        again = (*step(), step._pair_force)
        torch.cuda.synchronize()
        keys = ["E", "F"] + ["dE/dw"] * weight_gradient + ["dE/dq"] * (not full) + ["pair_force"]
        # (the mesh part spreads with LDS atomics: an output that two replays of one graph disagree on says so itself)
        lines += [f"{head} {name} {key} {sha(a)}{'' if torch.equal(a, b) else ' (differs between two replays)'}"
                  for key, a, b in zip(keys, first, again)]
    return lines


def main(argv):
    lines, summary = [], []
    digest = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()  # noqa: E731
    cell_step = "--cell-step" in argv
    argv = [a for a in argv if a != "--cell-step"]
    for run in ((lambda dtype, grad: run_dipole(dtype, grad, follow_cell=True)),) if cell_step else (run_dipole, run_combined):
        for dtype in (torch.float64, torch.float32):
            for grad in (True, False):
                got = run(dtype, grad)
                lines += got
                summary.append(f"## {' '.join(got[0].split()[:3])}: {len(got)} lines, sha256 {digest(got)}")
    summary.append(f"## all: {len(lines)} lines, sha256 {digest(lines)}")
    text = "\n".join([f"# {torch.cuda.get_device_name(0)}; sha256 of the raw bytes of every output"] + lines + summary) + "\n"
    if argv:
        with open(argv[0], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
