"""Point dipoles without a GPU: constructor errors, the PotentialDipole methods and the NumPy oracle against the reference's
outputs (tests/golden/dipole.npz), and the calculator's refusal of CPU tensors."""

import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from tests import _dipole_oracle as O

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "dipole.npz"))


def _opt(x):
    x = float(x)
    return None if np.isnan(x) else x


def _variant(name):
    p = f"tric_{name}"
    kw = dict(smearing=_opt(GOLD[f"{p}_smearing"]), exclusion_radius=_opt(GOLD[f"{p}_exclusion_radius"]),
              exclusion_degree=int(GOLD[f"{p}_exclusion_degree"]), epsilon=_opt(GOLD[f"{p}_epsilon"]) or 0.0,
              prefactor=_opt(GOLD[f"{p}_prefactor"]) or 1.0)
    return kw, bool(GOLD[f"{p}_full"]), _opt(GOLD[f"{p}_lr_wavelength"])


def _vectors(pos, cell, pairs, shifts):
    return pos[pairs[:, 1]] - pos[pairs[:, 0]] + shifts @ cell


def test_exports():
    assert "CalculatorDipole" in tpa.__all__ and "PotentialDipole" in tpa.__all__


def test_constructor_errors_match_the_reference():
    with pytest.raises(TypeError, match="Potential must be an instance of PotentialDipole, got"):
        tpa.CalculatorDipole(tpa.CoulombPotential(smearing=1.0))
    msg = "Either both `lr_wavelength` and `smearing` must be set or both must be None"
    with pytest.raises(AssertionError, match=msg):
        tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0))
    with pytest.raises(AssertionError, match=msg):
        tpa.CalculatorDipole(tpa.PotentialDipole(), lr_wavelength=0.5)
    tpa.CalculatorDipole(tpa.PotentialDipole())
    tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=0.5)


def test_potential_errors_match_the_reference():
    pot = tpa.PotentialDipole()
    v = torch.ones(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="Cannot compute cutoff function when `exclusion_radius` is not set"):
        pot.f_cutoff(v)
    with pytest.raises(ValueError, match="Cannot compute range-separated potential when `smearing` is not specified."):
        pot.sr_from_dist(v)
    with pytest.raises(ValueError, match="Cannot compute long-range contribution without specifying `smearing`."):
        pot.lr_from_dist(v)
    with pytest.raises(ValueError, match="Cannot compute long-range kernel without specifying `smearing`."):
        pot.lr_from_k_sq(v[:, 0])
    with pytest.raises(ValueError, match="Cannot compute long-range contribution without specifying `smearing`."):
        pot.self_contribution()


def test_buffers_match_the_reference():
    pot = tpa.PotentialDipole(smearing=0.8, exclusion_radius=2.0, exclusion_degree=2, epsilon=3.0, prefactor=2.0)
    assert sorted(dict(pot.named_buffers())) == ["epsilon", "exclusion_radius", "prefactor", "smearing"]
    assert all(b.dtype == torch.float64 for b in pot.buffers())
    assert pot.exclusion_degree == 2
    assert pot._host_params() == (0.8, 2.0, 3.0, 2.0)


def test_potential_methods_match_the_reference():
    v, k2 = torch.tensor(GOLD["methods_vectors"]), torch.tensor(GOLD["methods_k_sq"])
    pot = tpa.PotentialDipole(smearing=0.8, prefactor=2.0, epsilon=3.0)
    potx = tpa.PotentialDipole(smearing=0.8, exclusion_radius=2.0, exclusion_degree=2, prefactor=2.0)
    got = {
        "from_dist": pot.from_dist(v), "sr_from_dist": pot.sr_from_dist(v), "lr_from_dist": pot.lr_from_dist(v),
        "lr_from_k_sq": pot.lr_from_k_sq(k2), "self_contribution": pot.self_contribution(),
        "background_correction": pot.background_correction(torch.tensor(123.0)),
        "sr_from_dist_excl": potx.sr_from_dist(v), "f_cutoff_excl": potx.f_cutoff(v),
    }
    for name, val in got.items():
        want = GOLD[f"methods_{name}"]
        assert val.shape == want.shape, name
        np.testing.assert_allclose(val.numpy(), want, rtol=1e-12, atol=1e-13 * np.abs(want).max(), err_msg=name)
    assert tpa.PotentialDipole(smearing=1.0).background_correction(torch.tensor(1.0)) == 0.0


@pytest.mark.parametrize("name", [str(n) for n in GOLD["tric_variants"]])
def test_oracle_matches_the_reference(name):
    kw, full, lam = _variant(name)
    pos, cell, mu, g = GOLD["tric_positions"], GOLD["tric_cell"], GOLD["tric_dipoles"], GOLD["tric_g"]
    pairs, shifts = GOLD[f"tric_{name}_pairs"], GOLD[f"tric_{name}_shifts"]
    vec = _vectors(pos, cell, pairs, shifts)
    V = O.potential(mu, pos, cell, pairs, vec, lr_wavelength=lam, full=full, **kw)
    np.testing.assert_allclose(V, GOLD[f"tric_{name}_V_f64"], rtol=0, atol=1e-11 * np.abs(V).max())
    # gradients of <g, V>: the real-space dipole gradient is the pair sum applied to g (symmetric tensor), the pair-vector
    # gradient reaches the positions as +gvec on j and -gvec on i
    rkw = {k: kw[k] for k in ("smearing", "exclusion_radius", "exclusion_degree", "prefactor")}
    gmu = O.rspace(g, pairs, vec, full=full, **rkw)
    gpos = np.zeros_like(pos)
    gvec = GOLD[f"tric_{name}_gvec_f64"]
    np.add.at(gpos, pairs[:, 1], gvec)
    np.add.at(gpos, pairs[:, 0], -gvec)
    if lam is not None:
        _, kmu, kpos = O.kspace(mu, pos, cell, kw["smearing"], lam, kw["prefactor"], kw["epsilon"], grad_out=g)
        gmu, gpos = gmu + kmu, gpos + kpos
    for got, key in ((gmu, "gmu"), (gpos, "gpos")):
        want = GOLD[f"tric_{name}_{key}_f64"]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10 * np.abs(want).max(), err_msg=key)


@pytest.mark.parametrize("frame", [0, 1, 2])
def test_oracle_reproduces_espresso_frames(frame):
    p = f"frame{frame}"
    pos, cell, mu = GOLD[f"{p}_positions"], GOLD[f"{p}_cell"], GOLD[f"{p}_dipoles"]
    pairs = GOLD[f"{p}_pairs"]
    vec = _vectors(pos, cell, pairs, GOLD[f"{p}_shifts"])
    V = O.potential(mu, pos, cell, pairs, vec, smearing=float(GOLD[f"{p}_smearing"]), lr_wavelength=0.1,
                    prefactor=tpa.prefactors.eV_A)
    np.testing.assert_allclose(V, GOLD[f"{p}_V_f64"], rtol=0, atol=1e-11 * np.abs(V).max())
    np.testing.assert_allclose((V * mu).sum(), float(GOLD[f"{p}_energy"]), atol=1e-5, rtol=1e-4)


def test_calculator_refuses_cpu_tensors():
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=1.0)
    pos = torch.tensor(GOLD["chain_positions"])
    args = (torch.tensor(GOLD["chain_dipoles"]), torch.tensor(GOLD["chain_cell"]), pos, torch.tensor(GOLD["chain_pairs"]),
            torch.tensor(GOLD["chain_vectors"]))
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        calc(*args)
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        calc._compute_rspace(args[0], args[3], args[4])


def test_validation_messages():
    calc = tpa.CalculatorDipole(tpa.PotentialDipole())
    mu, cell, pos = torch.ones(3, 3), torch.eye(3), torch.zeros(3, 3)
    idx = torch.tensor([[0, 1]])
    with pytest.raises(ValueError, match=r"`neighbor_vectors` must be a tensor with shape \[num_neighbors, 3\]"):
        calc(mu, cell, pos, idx, torch.ones(1, 2))
    with pytest.raises(ValueError, match=r"`charges` must be a tensor with shape \[n_atoms, n_channels\]"):
        calc(torch.ones(2, 3), cell, pos, idx, torch.ones(1, 3))
    with pytest.raises(TypeError, match=r"type of `cell` \(torch.float64\) must be same as that of the `positions`"):
        calc(mu, cell.double(), pos, idx, torch.ones(1, 3))
