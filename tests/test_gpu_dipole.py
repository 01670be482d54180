"""CalculatorDipole on the GPU (csrc/dipole.hip): analytic and ESPResSo values, the reference's own outputs
(tests/golden/dipole.npz), gradcheck, both grid regimes of the reciprocal-space kernels against the NumPy oracle, edge
cases and the first-order limit."""

import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from tests import _dipole_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "dipole.npz"))
DTYPES = [torch.float64, torch.float32]


def _opt(x):
    x = float(x)
    return None if np.isnan(x) else x


def _variant(name):
    p = f"tric_{name}"
    kw = dict(smearing=_opt(GOLD[f"{p}_smearing"]), exclusion_radius=_opt(GOLD[f"{p}_exclusion_radius"]),
              exclusion_degree=int(GOLD[f"{p}_exclusion_degree"]), epsilon=_opt(GOLD[f"{p}_epsilon"]) or 0.0,
              prefactor=_opt(GOLD[f"{p}_prefactor"]) or 1.0)
    return kw, bool(GOLD[f"{p}_full"]), _opt(GOLD[f"{p}_lr_wavelength"])


def _t(x, dtype, grad=False):
    return torch.tensor(np.asarray(x), dtype=dtype, device=DEV, requires_grad=grad)


def _evaluate(calc, dtype, mu, pos, cell, pairs, shifts, g=None):
    """V and the gradients of <g, V> (g = mu: the energy) w.r.t. dipoles, positions, cell and the pair vectors."""
    tm, tp, tc = _t(mu, dtype, True), _t(pos, dtype, True), _t(cell, dtype, True)
    ti = torch.tensor(np.asarray(pairs), dtype=torch.int64, device=DEV)
    vec = tp[ti[:, 1]] - tp[ti[:, 0]] + _t(shifts, dtype) @ tc
    vec.retain_grad()
    V = calc(tm, tc, tp, ti, vec)
    L = (V * (tm if g is None else _t(g, dtype))).sum()
    L.backward()
    res = {"V": V, "L": L, "gmu": tm.grad, "gpos": tp.grad, "gcell": tc.grad, "gvec": vec.grad}
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


def _check_against_reference(res, prefix, dtype):
    for key in ("V", "gmu", "gpos", "gcell", "gvec"):
        want = GOLD[f"{prefix}_{key}_f64"]
        scale = np.abs(want).max()
        err = np.abs(res[key] - want).max()
        if dtype == torch.float64:
            tol = 1e-10 * scale
        else:  # 5x the spread of the reference's own fp32 run, floored at a few fp32 ulps of the scale
            spread = np.abs(GOLD[f"{prefix}_{key}_f32"] - want).max()
            tol = 5 * spread + 4 * np.finfo(np.float32).eps * scale
        assert err <= tol, f"{prefix} {key} {dtype}: max error {err:.3e} > {tol:.3e} (scale {scale:.3e})"


def _chain(dtype):
    return (_t(GOLD["chain_dipoles"], dtype), _t(GOLD["chain_cell"], dtype), _t(GOLD["chain_positions"], dtype),
            torch.tensor(GOLD["chain_pairs"], device=DEV), _t(GOLD["chain_vectors"], dtype))


# ---- analytic and ESPResSo values ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_analytic_and_espresso(dtype):
    mu, cell, pos, idx, vec = _chain(dtype)
    e = (tpa.CalculatorDipole(tpa.PotentialDipole())(mu, cell, pos, idx, vec) * mu).sum()
    torch.testing.assert_close(e, torch.tensor(float(GOLD["chain_direct"]), dtype=dtype, device=DEV))
    for smearing, key in ((1e10, "chain_sr_1e10"), (1e-10, "chain_sr_1e-10")):
        calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=smearing), lr_wavelength=1.0)
        e = (calc._compute_rspace(dipoles=mu, neighbor_indices=idx, neighbor_vectors=vec) * mu).sum()
        torch.testing.assert_close(e, torch.tensor(float(GOLD[key]), dtype=dtype, device=DEV))
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.5**0.5), lr_wavelength=0.1)  # ESPResSo alpha = 1
    e = (calc(mu, cell, pos, idx, vec) * mu).sum()
    torch.testing.assert_close(e, torch.tensor(float(GOLD["chain_ewald_alpha1"]), dtype=dtype, device=DEV), atol=1e-6,
                               rtol=1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", [0, 1, 2])
def test_crystal_frames(frame, dtype):
    p = f"frame{frame}"
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=float(GOLD[f"{p}_smearing"]), prefactor=tpa.prefactors.eV_A),
                                lr_wavelength=0.1)
    res = _evaluate(calc, dtype, GOLD[f"{p}_dipoles"], GOLD[f"{p}_positions"], GOLD[f"{p}_cell"], GOLD[f"{p}_pairs"],
                    GOLD[f"{p}_shifts"])
    np.testing.assert_allclose(res["L"], float(GOLD[f"{p}_energy"]), atol=1e-5, rtol=1e-4)  # ESPResSo
    np.testing.assert_allclose(-res["gpos"], GOLD[f"{p}_forces"], atol=1e-5, rtol=1e-4)
    _check_against_reference(res, p, dtype)


# ---- the reference's own outputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [str(n) for n in GOLD["tric_variants"]])
def test_triclinic_variants_match_the_reference(name, dtype):
    kw, full, lam = _variant(name)
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(**kw), full_neighbor_list=full, lr_wavelength=lam)
    res = _evaluate(calc, dtype, GOLD["tric_dipoles"], GOLD["tric_positions"], GOLD["tric_cell"],
                    GOLD[f"tric_{name}_pairs"], GOLD[f"tric_{name}_shifts"], GOLD["tric_g"])
    _check_against_reference(res, f"tric_{name}", dtype)


# ---- gradcheck -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "kw",
    [dict(smearing=0.8), dict(smearing=0.8, exclusion_radius=2.2, exclusion_degree=2), dict(), dict(smearing=0.7, epsilon=1.5)],
    ids=["smearing", "exclusion", "direct", "epsilon"],
)
def test_gradcheck(kw):
    rng = np.random.default_rng(5)
    cell = np.array([[4.3, 0.0, 0.0], [0.7, 4.1, 0.0], [-0.4, 0.5, 4.6]])
    pos = rng.uniform(0, 1, (6, 3)) @ cell
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, 3.0)
    vec0 = pos[pairs[:, 1]] - pos[pairs[:, 0]] + shifts @ cell
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(**kw), lr_wavelength=1.1 if kw.get("smearing") else None)
    idx = torch.tensor(pairs, device=DEV)
    d = torch.float64
    inputs = (_t(rng.normal(size=(6, 3)), d, True), _t(pos, d, True), _t(cell, d, True), _t(vec0, d, True))

    def f(mu, p, c, v):
        return calc(mu, c, p, idx, v)

    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-7, rtol=1e-5)


# ---- both grid regimes of the reciprocal-space kernels ---------------------------------------------------------------
def _oracle_check(mu, pos, cell, pairs, shifts, smearing, lam, g):
    """V, dL/dmu and dL/dpos of L = <g, V> against the oracle (fp64)."""
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=smearing), lr_wavelength=lam)
    res = _evaluate(calc, torch.float64, mu, pos, cell, pairs, shifts, g)
    vec = pos[pairs[:, 1]] - pos[pairs[:, 0]] + shifts @ cell
    V = O.potential(mu, pos, cell, pairs, vec, smearing=smearing, lr_wavelength=lam)
    _, kmu, kpos = O.kspace(mu, pos, cell, smearing, lam, grad_out=g)
    gmu = O.rspace(g, pairs, vec, smearing=smearing) + kmu
    gpos = kpos.copy()
    np.add.at(gpos, pairs[:, 1], res["gvec"])
    np.add.at(gpos, pairs[:, 0], -res["gvec"])
    for got, want, key in ((res["V"], V, "V"), (res["gmu"], gmu, "gmu"), (res["gpos"], gpos, "gpos")):
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err < 1e-10, (key, err)


def test_few_atoms_many_kvectors():
    """8 atoms against K = 85^3 = 614 125 k-vectors: the per-atom kernels run in k slices."""
    rng = np.random.default_rng(2)
    cell, pos = GOLD["frame0_cell"], GOLD["frame0_positions"]
    _oracle_check(GOLD["frame0_dipoles"], pos, cell, GOLD["frame0_pairs"], GOLD["frame0_shifts"],
                  float(GOLD["frame0_smearing"]), 0.1, rng.normal(size=pos.shape))


def test_many_atoms_odd_sizes():
    """N = 2003 atoms, K = 23 x 21 x 20 = 9660 k-vectors: no size a multiple of a tile."""
    rng = np.random.default_rng(4)
    cell = np.array([[28.1, 0.0, 0.0], [2.0, 26.0, 0.0], [-1.5, 1.0, 24.4]])
    n = 2003
    pos = rng.uniform(0, 1, (n, 3)) @ cell
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, 3.5)
    assert list(np.ceil(np.linalg.norm(cell, axis=1) / 1.25).astype(int)) == [23, 21, 20]
    _oracle_check(rng.normal(size=(n, 3)), pos, cell, pairs, shifts, 2.0, 1.25, rng.normal(size=(n, 3)))


# ---- edge cases ------------------------------------------------------------------------------------------------------
def test_empty_pair_list():
    rng = np.random.default_rng(8)
    cell = 6.0 * np.eye(3)
    pos = rng.uniform(0, 6, (5, 3))
    mu = rng.normal(size=(5, 3))
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=0.7)
    d = torch.float64
    tp = _t(pos, d, True)
    V = calc(_t(mu, d), _t(cell, d), tp, torch.zeros((0, 2), dtype=torch.int64, device=DEV),
             torch.zeros((0, 3), dtype=d, device=DEV))
    want = O.kspace(mu, pos, cell, 1.0, 0.7)
    np.testing.assert_allclose(V.detach().cpu().numpy(), want, rtol=0, atol=1e-12 * np.abs(want).max())
    (V * _t(mu, d)).sum().backward()
    assert torch.isfinite(tp.grad).all()


def test_direct_launches_no_reciprocal_kernel(monkeypatch):
    def fail(*args):
        raise AssertionError("the reciprocal-space sum ran without a smearing")

    monkeypatch.setattr(tpa.dipoles._DipoleKSpace, "apply", fail)
    monkeypatch.setattr(tpa._lib.load(), "mipme_ewald_filter", fail)
    mu, cell, pos, idx, vec = _chain(torch.float64)
    e = (tpa.CalculatorDipole(tpa.PotentialDipole())(mu, cell, pos, idx, vec) * mu).sum()
    assert float(e) == pytest.approx(-0.265625, rel=1e-14)


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_list_equals_half_list(dtype):
    rng = np.random.default_rng(9)
    cell = np.array([[7.1, 0.0, 0.0], [1.3, 6.6, 0.0], [-0.9, 1.1, 7.4]])
    pos = rng.uniform(0, 1, (30, 3)) @ cell
    mu = rng.normal(size=(30, 3))
    out = []
    for full in (False, True):
        pairs, shifts, _ = tpa.neighbor_list(pos, cell, 3.8, full_list=full)
        calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), full_neighbor_list=full, lr_wavelength=0.6)
        out.append(_evaluate(calc, dtype, mu, pos, cell, pairs, shifts))
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    for key in ("V", "gmu", "gpos", "gcell"):
        a, b = out[0][key], out[1][key]
        assert np.abs(a - b).max() <= tol * np.abs(a).max(), key


def test_two_calls_agree():
    rng = np.random.default_rng(10)
    cell = np.array([[7.1, 0.0, 0.0], [1.3, 6.6, 0.0], [-0.9, 1.1, 7.4]])
    pos = rng.uniform(0, 1, (40, 3)) @ cell
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, 3.8)
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=0.4)
    mu = rng.normal(size=(40, 3))
    a = _evaluate(calc, torch.float64, mu, pos, cell, pairs, shifts)
    b = _evaluate(calc, torch.float64, mu, pos, cell, pairs, shifts)
    for key in a:  # the real-space atomics leave the order of the last bits open
        assert np.abs(a[key] - b[key]).max() <= 1e-14 * np.abs(a[key]).max(), key


def test_double_backward_raises():
    mu, cell, pos, idx, _ = _chain(torch.float64)
    pos.requires_grad_(True)
    vec = pos[idx[:, 1]] - pos[idx[:, 0]]
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=1.0)
    e = (calc(mu, cell, pos, idx, vec) * mu).sum()
    (f,) = torch.autograd.grad(e, pos, create_graph=True)
    with pytest.raises(RuntimeError, match="dipole calculators are first order in this build"):
        f.pow(2).sum().backward()
