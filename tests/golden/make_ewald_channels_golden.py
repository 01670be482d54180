"""Generate tests/golden/ewald_channels.npz from the reference implementation (EwaldCalculator) on the CPU.

    python tests/golden/make_ewald_channels_golden.py /path/to/reference/checkout

What GraphedEwaldStep and GraphedEwaldBatch return for SEVERAL charge channels, (N, C) charges, computed by the reference with
`evaluate` of make_ewald_step_golden.py -- E = (q . V).sum() over atoms and channels and its total gradients w.r.t. charges (N, C),
positions and cell, in fp64 and fp32 (stored as float32), plus absE = sum_a |sum_c q_ac V_ac| -- at the construction cell
(``c0``) and at the strained cell ``cell (I + EPS)`` with the positions scaled along (``c1``).  The systems, potentials and lists
are READ from ewald_step.npz and ewald_batch.npz and not stored again: only the seeded charges and the results are.

Step cases (``<case>_charges``, ``<case>_<E|gq|gpos|gcell>_<c0|c1>_<f64|f32>``, ``<case>_absE_<c0|c1>``):
  tric_c3_net   Coulomb, smearing 1.0, the half list of tric_half; channel 0 neutral, channels 1 and 2 with different net charges
  tric_c2_excl  the potential (exclusion radius) and list of tric_excl
  tric_c2_ipl6  the potential (1/r^6: the k = 0 term is not zero, so bg multiplies Q_c) and full list of tric_ipl6, net charges
  tric_c8_half  eight channels on the list of tric_half: channel 2 all zeros, channel 5 equal to tric_net_charges
  big_c3_half, big_c2_full   the 300-atom system with the potential of big_half / big_full
Batch cases (``<C1|C2>_f<n>_...`` as in ewald_batch.npz, ``f<n>_charges``): the five frames of ewald_batch.npz with C = 3 charges
under its two calculators, C1 (Coulomb, half lists) and C2 (1/r^6, full lists).

Asserted here, relied on by the tests: every case has the same ns at both cells; in every case with more than one net charge
sum_c Q_c^2 and (sum_c Q_c)^2 differ by more than 10 % of the larger (a background term that mixes the channels cannot pass);
the reference's own fp32 - fp64 spread is non-zero for every stored key -- but for a key whose fp64 value is exactly zero in
every component (the force on the single atom of f0, zero term by term in both precisions).
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

STEP = np.load(os.path.join(HERE, "ewald_step.npz"))
BATCH = np.load(os.path.join(HERE, "ewald_batch.npz"))
STRAIN = np.eye(3) + EPS
BATCH_CALCS = {
    "C1": (lambda: torchpme.CoulombPotential(smearing=1.0), False),
    "C2": (lambda: torchpme.InversePowerLawPotential(exponent=6, smearing=0.9), True),
}


def _opt(x):
    x = float(x)
    return None if np.isnan(x) else x


def step_potential(prefix):
    """The potential of case ``prefix`` of ewald_step.npz, from the settings stored there."""
    kw = dict(smearing=_opt(STEP[f"{prefix}_smearing"]), exclusion_radius=_opt(STEP[f"{prefix}_exclusion_radius"]),
              exclusion_degree=int(STEP[f"{prefix}_exclusion_degree"]), prefactor=_opt(STEP[f"{prefix}_prefactor"]) or 1.0)
    if str(STEP[f"{prefix}_kind"]) == "coulomb":
        return torchpme.CoulombPotential(**kw)
    return torchpme.InversePowerLawPotential(exponent=int(STEP[f"{prefix}_exponent"]), **kw)


def step_list(prefix):
    name = prefix.split("_")[0]
    if name == "big":
        pairs, shifts = STEP["big_pairs"].astype(np.int64), STEP["big_shifts"].astype(np.int64)
        if prefix == "big_full":
            pairs, shifts = np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])
        return pairs, shifts
    return STEP[f"{prefix}_pairs"].astype(np.int64), STEP[f"{prefix}_shifts"].astype(np.int64)


def batch_system(n, full):
    """(positions, cell, pairs, shifts) of frame n of ewald_batch.npz."""
    kind = "full" if full else "half"
    if n < 3:
        return (BATCH[f"f{n}_positions"], BATCH[f"f{n}_cell"], BATCH[f"f{n}_pairs_{kind}"].astype(np.int64).reshape(-1, 2),
                BATCH[f"f{n}_shifts_{kind}"].astype(np.int64).reshape(-1, 3))
    if n == 3:
        return (STEP["tric_positions"], STEP["tric_cell"], *step_list("tric_ipl6" if full else "tric_half"))
    return (STEP["big_positions"], STEP["big_cell"], *step_list("big_full" if full else "big_half"))


def with_nets(rng, n, nets):
    """(n, C) seeded charges whose channel c sums to n * nets[c]."""
    q = rng.normal(size=(n, len(nets)))
    return q - q.mean(axis=0) + np.asarray(nets)[None, :]


def check_nets(q, what):
    Q = q.sum(axis=0)
    a, b = float((Q * Q).sum()), float(Q.sum() ** 2)
    assert abs(a - b) > 0.1 * max(a, b), (what, a, b)


def run(out, prefix, make_pot, full, q, pos, cell, pairs, shifts):
    assert ns_of(cell, LAM) == ns_of(cell @ STRAIN, LAM), prefix
    for ctag, c, p in (("c0", cell, pos), ("c1", cell @ STRAIN, pos @ STRAIN)):
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            # (a calculator of its own per run: `.to(float32)` rounds the potential's buffers for good)
            calc = torchpme.EwaldCalculator(make_pot(), lr_wavelength=LAM, full_neighbor_list=full)
            for k, v in evaluate(calc, dtype, q, p, c, pairs, shifts).items():
                out[f"{prefix}_absE_{ctag}" if k == "absE" else f"{prefix}_{k}_{ctag}_{tag}"] = np.asarray(v)
        for k in ("E", "gq", "gpos", "gcell"):
            hi, lo = out[f"{prefix}_{k}_{ctag}_f64"], out[f"{prefix}_{k}_{ctag}_f32"].astype(np.float64)
            assert lo.shape == hi.shape and out[f"{prefix}_{k}_{ctag}_f32"].dtype == np.float32
            assert np.abs(lo - hi).max() > 0 or not hi.any(), (prefix, k, ctag)
        print(f"{prefix} {ctag}: N={len(q)} C={q.shape[1]} P={len(pairs)} E={float(out[f'{prefix}_E_{ctag}_f64']):.10f} "
              f"(fp32 {float(out[f'{prefix}_E_{ctag}_f32']):.7f})")


def main():
    out = {}
    rng = np.random.default_rng(41)
    tric_net = STEP["tric_net_charges"]
    c8 = with_nets(rng, 24, [0.0, 0.1, 0.0, -0.15, 0.05, 0.0, 0.2, 0.0])
    c8[:, 2] = 0.0
    c8[:, 5] = tric_net[:, 0]
    step_cases = {  # name: (potential and full flag of, list of, charges)
        "tric_c3_net": ("tric_half", "tric_half", with_nets(rng, 24, [0.0, 0.3, -0.2])),
        "tric_c2_excl": ("tric_excl", "tric_excl", with_nets(rng, 24, [0.0, 0.0])),
        "tric_c2_ipl6": ("tric_ipl6", "tric_ipl6", with_nets(rng, 24, [0.3, -0.2])),
        "tric_c8_half": ("tric_half", "tric_half", c8),
        "big_c3_half": ("big_half", "big_half", with_nets(rng, 300, [0.0, 0.02, -0.03])),
        "big_c2_full": ("big_full", "big_full", with_nets(rng, 300, [0.02, -0.03])),
    }
    for name, (pot_of, list_of, q) in step_cases.items():
        if name not in ("tric_c2_excl",):
            check_nets(q, name)
        sysname = name.split("_")[0]
        out[f"{name}_charges"] = q
        pairs, shifts = step_list(list_of)
        run(out, name, lambda p=pot_of: step_potential(p), bool(STEP[f"{pot_of}_full"]), q, STEP[f"{sysname}_positions"],
            STEP[f"{sysname}_cell"], pairs, shifts)
    assert np.array_equal(out["tric_c8_half_charges"][:, 5:6], tric_net) and not out["tric_c8_half_charges"][:, 2].any()
    assert abs(out["tric_c3_net_charges"][:, 0].sum()) < 1e-12

    counts = [1, 2, 17, 24, 300]
    frame_q = [np.array([[0.7, -0.5, 0.3]]), np.array([[0.9, 0.2, -0.6], [-0.4, 0.5, -0.1]])]
    frame_q += [with_nets(rng, n, [0.0, 0.2, -0.15]) for n in counts[2:]]
    for n, q in enumerate(frame_q):
        assert q.shape == (counts[n], 3)
        check_nets(q, f"f{n}")
        out[f"f{n}_charges"] = q
        for cname, (make, full) in BATCH_CALCS.items():
            pos, cell, pairs, shifts = batch_system(n, full)
            run(out, f"{cname}_f{n}", make, full, q, pos, cell, pairs, shifts)

    path = os.path.join(HERE, "ewald_channels.npz")
    np.savez_compressed(path, **out)
    # Size.  Four of the cases have 300 atoms with C + 3 results per atom, at two cells, in fp64 and fp32: 4 x 2 x ~1 800 values x 12
    # bytes = 170 KB of mantissas that no compression shortens, the fp64 ones alone 115 KB; with the other cases the file is
    # larger than ewald_step.npz (154 KB), the largest Ewald golden so far.  The cases are what the tests are about and stay.
    other = max(os.path.getsize(os.path.join(HERE, f)) for f in ("ewald_step.npz", "ewald_batch.npz"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes (the largest other Ewald golden: {other})")
    assert os.path.getsize(path) < 300_000


if __name__ == "__main__":
    main()
