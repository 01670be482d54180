"""Generate tests/golden/combined_step.npz from the reference implementation on the CPU: the quantities one call of
``GraphedCombinedStep`` returns, from the reference's autograd.

    python tests/golden/make_combined_step_golden.py /path/to/reference/checkout

Systems: the two 24-atom systems of ``combined.npz`` (``tric``, ``ortho``; read from there, not copied), channel 0 of their
charges as an (N, 1) tensor.  Potential: the ``rs`` combination of ``make_combined_golden.py`` -- Coulomb(sigma 0.8) +
1/r^6(sigma 1.1) + 1/r^3(sigma 0.6), weights (1.0, -0.3, 0.5), the combination's own smearing 1.0.  Calculators:
``PMECalculator(mesh_spacing=0.6, interpolation_nodes=4)`` (``pme``) and ``P3MCalculator(mesh_spacing=0.6,
interpolation_nodes=3)`` (``p3m``), each with the half and the full list.

Contents, ``<sys>_<pme|p3m>_<half|full>_<key>_<f64|f32>``:
  E      sum_a q_a V_a
  gpos   dE/dpositions (N, 3), the distances d = |r_j - r_i + S cell| included
  gq     dE/dcharges (N, 1); half lists only
  gw     dE/dweights (3,)
The float32 runs are the reference's own, on a potential (weights included) converted to float32 before the calculator is built.
Data only.
"""

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
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

SYSTEMS = np.load(os.path.join(HERE, "combined.npz"))
W_RS = (1.0, -0.3, 0.5)


def make_rs(dtype):
    pot = torchpme.CombinedPotential(
        [torchpme.CoulombPotential(smearing=0.8), torchpme.InversePowerLawPotential(exponent=6, smearing=1.1),
         torchpme.InversePowerLawPotential(exponent=3, smearing=0.6)], initial_weights=torch.tensor(W_RS, dtype=dtype), smearing=1.0)
    return pot.to(dtype)


def evaluate(calc, dtype, sname, list_tag):
    q = torch.tensor(SYSTEMS[f"{sname}_charges"][:, :1], dtype=dtype, requires_grad=True)
    pos = torch.tensor(SYSTEMS[f"{sname}_positions"], dtype=dtype, requires_grad=True)
    cell = torch.tensor(SYSTEMS[f"{sname}_cell"], dtype=dtype)
    idx = torch.tensor(SYSTEMS[f"{sname}_pairs_{list_tag}"], dtype=torch.int64)
    S = torch.tensor(SYSTEMS[f"{sname}_shifts_{list_tag}"], dtype=dtype)
    w = calc.potential.weights
    w.grad = None
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + S @ cell, dim=1)
    E = (calc(q, cell, pos, idx, d) * q).sum()
    E.backward()
    out = {"E": E.detach().numpy().reshape(()), "gpos": pos.grad.numpy(), "gw": w.grad.numpy().copy()}
    if list_tag == "half":
        out["gq"] = q.grad.numpy()
    return out


def main():
    out = {}
    for sname in ("tric", "ortho"):
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            for list_tag in ("half", "full"):
                full = list_tag == "full"
                calcs = {
                    "pme": torchpme.PMECalculator(make_rs(dtype), mesh_spacing=0.6, interpolation_nodes=4, full_neighbor_list=full),
                    "p3m": torchpme.P3MCalculator(make_rs(dtype), mesh_spacing=0.6, interpolation_nodes=3, full_neighbor_list=full),
                }
                for cname, calc in calcs.items():
                    for key, val in evaluate(calc, dtype, sname, list_tag).items():
                        out[f"{sname}_{cname}_{list_tag}_{key}_{tag}"] = val.astype(np.float64 if tag == "f64" else np.float32)
        print(sname, "done")
    path = os.path.join(HERE, "combined_step.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
