"""Generate tests/golden/combined.npz from the reference implementation (CombinedPotential, potentials/combined.py) on the CPU.

    python tests/golden/make_combined_golden.py /path/to/reference/checkout

The two 24-atom systems (triclinic, orthorhombic; 2 charge channels, cutoff 3.6, half and full lists, a pair mask for the half
list) and the reciprocal-axis spline of case 3 are those of ``spline.npz``; they are copied into this file.

Potentials (the combination's own ``smearing`` is 1.0 where its members are range separated):
  rs        Coulomb(sigma 0.8) + 1/r^6(sigma 1.1) + 1/r^3(sigma 0.6), weights (1.0, -0.3, 0.5)
  direct    1/r + 1/r^6 without smearing, weights (0.7, -1.2), the combination's own exclusion_radius 2.5, degree 2
  fallback  Coulomb(sigma 1.0) + the spline "recip" of spline.npz (smearing 1.0), weights (0.8, 0.4)
Contents:
  <sys>_*                        cell, positions, charges, g (the seed of L = <g, V>), pairs_/shifts_ half and full, mask_half
  <sys>_<case>_<key>_<f64|f32>   V and the gradients of L w.r.t. charges (gq), positions (gpos), cell (gcell, through
                                 d = |r_j - r_i + S cell|), the distances (gd) and the weights (gw); cases rs_<pme|p3m|ewald>,
                                 rs_pme_full, rs_pme_mask, direct_<half|full|mask>, fallback_pme.  The float32 runs are the
                                 reference's own, on potentials (weights included) converted to float32 before the calculator
                                 is built.
  <sys>_rs_pme_h{q,pos,w}_f64    second order: the gradient of |dL/dpositions|^2 w.r.t. charges, positions and the weights
  m_dist, m_ksq, m_rs_<method>, m_direct_from_dist, m_rs_self, m_rs_background
                                 the reference's method values at 40 distances / 40 squared wave numbers (k^2 = 0 among them)
  sd_keys, sd_<i>                the reference's state dict of "rs": the names and, in their order, the values
  recip_{r,y,k,yhat}             the spline of case 3
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

F64 = torch.float64
SPLINE = np.load(os.path.join(HERE, "spline.npz"))
SYSTEM_KEYS = ("cell", "positions", "charges", "g", "pairs_half", "shifts_half", "pairs_full", "shifts_full", "mask_half")
W_RS, W_DIRECT, W_FALLBACK = (1.0, -0.3, 0.5), (0.7, -1.2), (0.8, 0.4)


class _Spline(torchpme.SplinePotential):
    """The reference's spline with a background correction of shape () like its other potentials': CombinedPotential stacks
    the members' values, and the (1,) of the spline class does not stack with Coulomb's ()."""

    def background_correction(self):
        return super().background_correction().reshape(())

    def self_contribution(self):
        return super().self_contribution().reshape(())


def make(case, dtype):
    w = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    if case == "rs":
        pot = torchpme.CombinedPotential(
            [torchpme.CoulombPotential(smearing=0.8), torchpme.InversePowerLawPotential(exponent=6, smearing=1.1),
             torchpme.InversePowerLawPotential(exponent=3, smearing=0.6)], initial_weights=w(W_RS), smearing=1.0)
    elif case == "direct":
        pot = torchpme.CombinedPotential([torchpme.CoulombPotential(), torchpme.InversePowerLawPotential(exponent=6)],
                                         initial_weights=w(W_DIRECT), exclusion_radius=2.5, exclusion_degree=2)
    else:
        t = lambda key: torch.tensor(SPLINE[f"recip_{key}"], dtype=dtype)  # noqa: E731
        spline = _Spline(r_grid=t("r"), y_grid=t("y"), k_grid=t("k"), yhat_grid=t("yhat"), reciprocal=True,
                         y_at_zero=float(np.sqrt(2 / np.pi)), yhat_at_zero=0.0, smearing=1.0)
        pot = torchpme.CombinedPotential([torchpme.CoulombPotential(smearing=1.0), spline], initial_weights=w(W_FALLBACK),
                                         smearing=1.0)
    return pot.to(dtype)


def evaluate(calc, dtype, s, list_tag, mask=None, second=False):
    q = torch.tensor(s["charges"], dtype=dtype, requires_grad=True)
    pos = torch.tensor(s["positions"], dtype=dtype, requires_grad=True)
    cell = torch.tensor(s["cell"], dtype=dtype, requires_grad=True)
    idx = torch.tensor(s[f"pairs_{list_tag}"], dtype=torch.int64)
    S = torch.tensor(s[f"shifts_{list_tag}"], dtype=dtype)
    g = torch.tensor(s["g"], dtype=dtype)
    w = calc.potential.weights
    w.grad = None
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + S @ cell, dim=1)
    d.retain_grad()
    kw = {} if mask is None else {"pair_mask": torch.tensor(mask)}
    V = calc(q, cell, pos, idx, d, **kw)
    L = (V * g).sum()
    if second:
        (gp,) = torch.autograd.grad(L, pos, create_graph=True)
        hq, hpos, hw = torch.autograd.grad((gp * gp).sum(), (q, pos, w))
        return {"hq": hq.numpy(), "hpos": hpos.numpy(), "hw": hw.numpy()}
    L.backward()
    return {"V": V.detach().numpy(), "gq": q.grad.numpy(), "gpos": pos.grad.numpy(), "gcell": cell.grad.numpy(),
            "gd": d.grad.numpy(), "gw": w.grad.numpy().copy()}


def main():
    rng = np.random.default_rng(20261018)
    out = {f"recip_{k}": SPLINE[f"recip_{k}"] for k in ("r", "y", "k", "yhat")}
    # ---- method values and the state dict
    rs, direct = make("rs", F64), make("direct", F64)
    dist = np.exp(rng.uniform(np.log(0.05), np.log(8.0), 40))
    ksq = np.exp(rng.uniform(np.log(1e-3), np.log(60.0), 40))
    ksq[3] = 0.0
    td, tk = torch.tensor(dist), torch.tensor(ksq)
    out["m_dist"], out["m_ksq"] = dist, ksq
    with torch.no_grad():
        for method in ("from_dist", "sr_from_dist", "lr_from_dist"):
            out[f"m_rs_{method}"] = getattr(rs, method)(td).numpy()
        out["m_rs_lr_from_k_sq"] = rs.lr_from_k_sq(tk).numpy()
        out["m_rs_self"] = rs.self_contribution().numpy().reshape(-1)
        out["m_rs_background"] = rs.background_correction().numpy().reshape(-1)
        out["m_direct_from_dist"] = direct.from_dist(td).numpy()
    sd = rs.state_dict()
    out["sd_keys"] = np.array(list(sd.keys()))
    for i, v in enumerate(sd.values()):
        out[f"sd_{i}"] = v.detach().numpy()
    # ---- calculators
    for sname in ("tric", "ortho"):
        s = {k: SPLINE[f"{sname}_{k}"] for k in SYSTEM_KEYS}
        for k, v in s.items():
            out[f"{sname}_{k}"] = v
        for dtype, tag in ((F64, "f64"), (torch.float32, "f32")):
            store = (lambda a: a.astype(np.float64)) if tag == "f64" else (lambda a: a.astype(np.float32))
            runs = {
                "rs_pme": (torchpme.PMECalculator(make("rs", dtype), mesh_spacing=0.6, interpolation_nodes=4), "half", None),
                "rs_p3m": (torchpme.P3MCalculator(make("rs", dtype), mesh_spacing=0.6, interpolation_nodes=3), "half", None),
                "rs_ewald": (torchpme.EwaldCalculator(make("rs", dtype), lr_wavelength=0.8), "half", None),
                "rs_pme_full": (torchpme.PMECalculator(make("rs", dtype), mesh_spacing=0.6, interpolation_nodes=4,
                                                       full_neighbor_list=True), "full", None),
                "rs_pme_mask": (torchpme.PMECalculator(make("rs", dtype), mesh_spacing=0.6, interpolation_nodes=4), "half",
                                s["mask_half"]),
                "direct_half": (torchpme.Calculator(make("direct", dtype)), "half", None),
                "direct_full": (torchpme.Calculator(make("direct", dtype), full_neighbor_list=True), "full", None),
                "direct_mask": (torchpme.Calculator(make("direct", dtype)), "half", s["mask_half"]),
                "fallback_pme": (torchpme.PMECalculator(make("fallback", dtype), mesh_spacing=0.6, interpolation_nodes=4),
                                 "half", None),
            }
            for case, (calc, list_tag, mask) in runs.items():
                for key, val in evaluate(calc, dtype, s, list_tag, mask=mask).items():
                    out[f"{sname}_{case}_{key}_{tag}"] = store(val)
            if tag == "f64":
                for key, val in evaluate(runs["rs_pme"][0], dtype, s, "half", second=True).items():
                    out[f"{sname}_rs_pme_{key}_f64"] = val
        print(sname, "done")
    path = os.path.join(HERE, "combined.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
