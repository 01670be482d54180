"""GraphedDipoleStep on the GPU (csrc/dipole_step.hip): E, F, dE/dmu and dE/dcell against the reference's own outputs
(tests/golden/dipole_step.npz, and the ESPResSo frames of tests/golden/dipole.npz), against the eager CalculatorDipole, against
finite differences of its own energy; what a replay leaves behind, bit reproducibility, new dipoles, a new list; the compacted
k list."""

import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "dipole_step.npz"))
FRAMES = np.load(os.path.join(HERE, "golden", "dipole.npz"))
DTYPES = [torch.float64, torch.float32]
EPS32 = float(np.finfo(np.float32).eps)


def test_class_is_exported():
    assert hasattr(tpa, "GraphedDipoleStep")


def _opt(x):
    x = float(x)
    return None if np.isnan(x) else x


def _t(x, dtype):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=dtype, device=DEV)


def _build(calc, dtype, mu, pos, cell, pairs, shifts, cell_gradient=True):
    ti = torch.tensor(np.asarray(pairs, dtype=np.int64), device=DEV)
    return tpa.GraphedDipoleStep(calc, _t(mu, dtype), _t(cell, dtype), _t(pos, dtype), ti, _t(shifts, dtype),
                                 cell_gradient=cell_gradient)


def _results(step, *args):
    out = step(*args)
    torch.cuda.synchronize()
    res = {"E": out[0], "F": out[1], "gmu": out[2]}
    if len(out) > 3:
        res["gcell"] = out[3]
    return {k: v.detach().double().cpu().numpy().copy() for k, v in res.items()}


def _check(res, want, spread, abs_e, dtype, what):
    """fp64: 1e-10 of the largest wanted value.  fp32: 5x the spread of the reference's own fp32 run + 4 eps32 of the scale (the
    bounds of tests/test_gpu_dipole.py); the scale of the scalar E is sum_i |mu_i . V_i| -- the difference of two scalars can be
    accidentally tiny, and E itself small next to its terms."""
    for key in res:
        scale = np.abs(want[key]).max()
        err = np.abs(res[key] - want[key]).max()
        if dtype == torch.float64:
            tol = 1e-10 * scale
        else:
            tol = 5 * spread[key] + 4 * EPS32 * (abs_e if key == "E" else scale)
        print(f"{what} {key} {dtype}: max error {err:.3e}, bound {tol:.3e}, scale {scale:.3e}")
        assert err <= tol, f"{what} {key} {dtype}: max error {err:.3e} > {tol:.3e} (scale {scale:.3e})"


def _golden(gold, prefix, e_key="E"):
    want = {"E": np.float64(gold[f"{prefix}_{e_key}_f64"]), "F": -gold[f"{prefix}_gpos_f64"], "gmu": gold[f"{prefix}_gmu_f64"],
            "gcell": gold[f"{prefix}_gcell_f64"]}
    f32 = {"E": np.float64(gold[f"{prefix}_{e_key}_f32"]), "F": -gold[f"{prefix}_gpos_f32"].astype(np.float64),
           "gmu": gold[f"{prefix}_gmu_f32"].astype(np.float64), "gcell": gold[f"{prefix}_gcell_f32"].astype(np.float64)}
    return want, {k: np.abs(f32[k] - want[k]).max() for k in want}


def _calc(prefix):
    kw = dict(smearing=_opt(GOLD[f"{prefix}_smearing"]), exclusion_radius=_opt(GOLD[f"{prefix}_exclusion_radius"]),
              exclusion_degree=int(GOLD[f"{prefix}_exclusion_degree"]), epsilon=_opt(GOLD[f"{prefix}_epsilon"]) or 0.0,
              prefactor=_opt(GOLD[f"{prefix}_prefactor"]) or 1.0)
    full = bool(GOLD[f"{prefix}_full"])
    return tpa.CalculatorDipole(tpa.PotentialDipole(**kw), full_neighbor_list=full, lr_wavelength=_opt(GOLD[f"{prefix}_lr_wavelength"]))


def _big_list(full):
    pairs, shifts = GOLD["big_pairs"].astype(np.int64), GOLD["big_shifts"].astype(np.int64)
    if full:  # the half list followed by its mirror, as the golden script builds it
        pairs, shifts = np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])
    return pairs, shifts


# ---- against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [str(n) for n in GOLD["tric_variants"]])
def test_triclinic_variants_match_the_reference(name, dtype):
    p = f"tric_{name}"
    step = _build(_calc(p), dtype, GOLD["tric_dipoles"], GOLD["tric_positions"], GOLD["tric_cell"], GOLD[f"{p}_pairs"],
                  GOLD[f"{p}_shifts"])
    want, spread = _golden(GOLD, p)
    _check(_results(step), want, spread, float(GOLD[f"{p}_absE"]), dtype, p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_300_atoms_match_the_reference(full, dtype):
    """More atoms than the LDS tile of the structure kernel, no multiple of the rows of a row block, rows without a pair and rows
    of more than two chunks, several k slices per atom."""
    p = "big_full" if full else "big_half"
    pairs, shifts = _big_list(full)
    step = _build(_calc(p), dtype, GOLD["big_dipoles"], GOLD["big_positions"], GOLD["big_cell"], pairs, shifts)
    assert step.n_k >= 2048
    want, spread = _golden(GOLD, p)
    _check(_results(step), want, spread, float(GOLD[f"{p}_absE"]), dtype, p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", [0, 1, 2])
def test_crystal_frames(frame, dtype):
    """8 atoms against 85^3 k-vectors (hundreds of slices): the reference's outputs and the ESPResSo energies and forces."""
    p = f"frame{frame}"
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=float(FRAMES[f"{p}_smearing"]), prefactor=tpa.prefactors.eV_A),
                                lr_wavelength=0.1)
    mu = FRAMES[f"{p}_dipoles"]
    step = _build(calc, dtype, mu, FRAMES[f"{p}_positions"], FRAMES[f"{p}_cell"], FRAMES[f"{p}_pairs"], FRAMES[f"{p}_shifts"])
    res = _results(step)
    np.testing.assert_allclose(res["E"], float(FRAMES[f"{p}_energy"]), atol=1e-5, rtol=1e-4)  # ESPResSo
    np.testing.assert_allclose(res["F"], FRAMES[f"{p}_forces"], atol=1e-5, rtol=1e-4)
    want, spread = _golden(FRAMES, p, e_key="L")
    _check(res, want, spread, float(np.abs((FRAMES[f"{p}_V_f64"] * mu).sum(axis=1)).sum()), dtype, p)


# ---- against the eager call --------------------------------------------------------------------------------------------------
def _eager(calc, dtype, mu, pos, cell, pairs, shifts):
    """What the step returns, from the eager calculator and autograd (the code of the parent commit)."""
    tm, tp, tc = (_t(x, dtype).requires_grad_(True) for x in (mu, pos, cell))
    ti = torch.tensor(np.asarray(pairs, dtype=np.int64), device=DEV)
    vec = tp[ti[:, 1]] - tp[ti[:, 0]] + _t(shifts, dtype) @ tc
    V = calc(tm, tc, tp, ti, vec)
    per_atom = (V * tm).sum(dim=1)
    E = per_atom.sum()
    E.backward()
    res = {"E": E, "F": -tp.grad, "gmu": tm.grad, "gcell": tc.grad, "absE": per_atom.abs().sum()}
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


def _small_system(n=37, seed=21, cutoff=3.4):
    rng = np.random.default_rng(seed)
    cell = np.array([[7.9, 0.0, 0.0], [1.1, 7.2, 0.0], [-0.8, 0.9, 8.1]])
    pos = rng.uniform(0, 1, (n, 3)) @ cell
    mu = rng.normal(size=(n, 3))
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, cutoff)
    return mu, pos, cell, pairs, shifts


def _check_against_eager(calc, dtype, system, what):
    """fp64: 1e-10 of the scale.  fp32: the bound of `_check` with the eager fp64 result as `want` and the eager call's own
    fp32 - fp64 spread in the place of the reference's."""
    want = _eager(calc, torch.float64, *system)
    abs_e = float(want.pop("absE"))
    spread = None
    if dtype == torch.float32:
        low = _eager(calc, torch.float32, *system)
        spread = {k: np.abs(low[k] - want[k]).max() for k in want}
    _check(_results(_build(calc, dtype, *system)), want, spread, abs_e, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
def test_300_atoms_match_the_eager_call(full, dtype):
    p = "big_full" if full else "big_half"
    system = (GOLD["big_dipoles"], GOLD["big_positions"], GOLD["big_cell"], *_big_list(full))
    _check_against_eager(_calc(p), dtype, system, p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize(
    "kw",
    [dict(smearing=0.9, epsilon=2.0, prefactor=1.7), dict(smearing=0.9, exclusion_radius=2.4, exclusion_degree=2), dict()],
    ids=["smearing", "exclusion", "direct"],
)
def test_37_atoms_match_the_eager_call(kw, dtype):
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(**kw), lr_wavelength=0.7 if kw else None)
    _check_against_eager(calc, dtype, _small_system(), f"37 atoms {sorted(kw)}")


def test_asymmetric_full_list():
    """A full list that is not symmetric (some mirrors removed): dE/dmu is V plus the transposed half, not 2 V.  The eager
    backward applies the forward sum to the upstream gradient, which is the transposed sum only for a symmetric list, so what is
    wanted comes from two eager FORWARD calls, which are right for any list: V of the list plus V of the mirrored list (j, i, -S)
    (the reciprocal part is in both: 2 V_k).  E and F (the eager pair-vector gradient is per listed pair) compare as usual."""
    mu, pos, cell, pairs, shifts = _small_system()
    fp, fs, _ = tpa.neighbor_list(pos, cell, 3.4, full_list=True)
    keep = np.ones(len(fp), dtype=bool)
    keep[::5] = False
    fp, fs = fp[keep], fs[keep]
    d = torch.float64
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.9), full_neighbor_list=True, lr_wavelength=0.7)
    want = _eager(calc, d, mu, pos, cell, fp, fs)
    abs_e = float(want.pop("absE"))
    V = []
    for p, s in ((fp, fs), (fp[:, ::-1].copy(), -fs)):
        ti = torch.tensor(p, device=DEV)
        vec = _t(pos, d)[ti[:, 1]] - _t(pos, d)[ti[:, 0]] + _t(s, d) @ _t(cell, d)
        V.append(calc(_t(mu, d), _t(cell, d), _t(pos, d), ti, vec).cpu().numpy())
    assert np.abs(V[0] - V[1]).max() > 1e-3 * np.abs(V[0]).max()  # (the list is asymmetric indeed)
    want["gmu"] = V[0] + V[1]
    res = _results(_build(calc, d, mu, pos, cell, fp, fs))
    for key in ("E", "F", "gmu", "gcell"):
        _check({key: res[key]}, want, None, abs_e, d, "asymmetric full list")
    np.testing.assert_allclose(res["E"], 0.5 * (mu * res["gmu"]).sum(), rtol=1e-12)


# ---- finite differences of the step's own energy ---------------------------------------------------------------------------------
def test_finite_differences():
    mu, pos, cell, pairs, shifts = _small_system()
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.9, epsilon=2.0), lr_wavelength=0.7)
    step = _build(calc, torch.float64, mu, pos, cell, pairs, shifts, cell_gradient=False)
    base = _results(step)
    h = 1e-5
    for key, which in (("F", 0), ("gmu", 1)):
        a, c = np.unravel_index(np.abs(base[key]).argmax(), base[key].shape)
        e = []
        for sgn in (+1, -1):
            moved = [pos.copy(), mu.copy()]
            moved[which][a, c] += sgn * h
            e.append(float(_results(step, _t(moved[0], torch.float64), _t(moved[1], torch.float64))["E"]))
        fd = (e[0] - e[1]) / (2 * h)
        got = -base[key][a, c] if key == "F" else base[key][a, c]
        print(f"finite difference {key}[{a},{c}]: {fd:.12e} analytic {got:.12e}")
        assert abs(fd - got) <= 1e-6 * abs(got)


# ---- replays -----------------------------------------------------------------------------------------------------------------
def _bits(step, *args):
    out = step(*args)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_is_left_in_an_accumulator(dtype):
    mu, pos, cell, pairs, shifts = _small_system()
    rng = np.random.default_rng(3)
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.9, epsilon=2.0), lr_wavelength=0.7)
    step = _build(calc, dtype, mu, pos, cell, pairs, shifts)
    A = (_t(pos, dtype), _t(mu, dtype))
    B = (_t(pos + rng.normal(scale=0.05, size=pos.shape), dtype), _t(rng.normal(size=mu.shape), dtype))
    first, other, again = _bits(step, *A), _bits(step, *B), _bits(step, *A)
    assert _same(first, again)
    assert not torch.equal(first[1], other[1])


def test_two_objects_agree_bitwise_in_fp32():
    system = (GOLD["big_dipoles"], GOLD["big_positions"], GOLD["big_cell"], *_big_list(False))
    a = _build(_calc("big_half"), torch.float32, *system)
    b = _build(_calc("big_half"), torch.float32, *system)
    assert _same(_bits(a), _bits(b))


def test_new_dipoles_without_a_recapture():
    mu, pos, cell, pairs, shifts = _small_system()
    mu2 = np.random.default_rng(4).normal(size=mu.shape)
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.9), lr_wavelength=0.7)
    step = _build(calc, torch.float64, mu, pos, cell, pairs, shifts)
    fresh = _build(calc, torch.float64, mu2, pos, cell, pairs, shifts)
    before = _bits(step)
    after = _bits(step, _t(pos, torch.float64), _t(mu2, torch.float64))
    assert _same(after, _bits(fresh)) and not torch.equal(before[2], after[2])
    assert _same(_bits(step, None, _t(mu, torch.float64)), before)  # the dipoles alone, the positions stay


def test_recapture_with_another_list():
    mu, pos, cell, pairs, shifts = _small_system()
    p2, s2, _ = tpa.neighbor_list(pos, cell, 2.9)
    assert 0 < len(p2) < len(pairs)
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.9), lr_wavelength=0.7)
    step = _build(calc, torch.float32, mu, pos, cell, pairs, shifts)
    before = _bits(step)
    step.recapture(torch.tensor(p2, device=DEV), _t(s2, torch.float32))
    fresh = _build(calc, torch.float32, mu, pos, cell, p2, s2)
    after = _bits(step)
    assert _same(after, _bits(fresh)) and not torch.equal(before[1], after[1])


# ---- the compacted k list ------------------------------------------------------------------------------------------------------
def test_n_k_counts_the_classes_of_the_grid():
    cases = (("tric_half", GOLD["tric_cell"], (15, 14, 16)), ("big_half", GOLD["big_cell"], (16, 16, 16)))
    for prefix, cell, ns in cases:
        calc = _calc(prefix)
        assert tuple(np.ceil(np.linalg.norm(cell, axis=1) / calc.lr_wavelength).astype(int)) == ns
        f = [np.rint(np.fft.fftfreq(n) * n).astype(int) for n in ns]
        grid = {(a, b, c) for a in f[0] for b in f[1] for c in f[2]}
        classes = set()
        for v in grid - {(0, 0, 0)}:
            m = tuple(-x for x in v)
            classes.add(max(v, m) if m in grid else v)
        name = "tric" if prefix.startswith("tric") else "big"
        pairs, shifts = (GOLD["tric_half_pairs"], GOLD["tric_half_shifts"]) if name == "tric" else _big_list(False)
        step = _build(calc, torch.float64, GOLD[f"{name}_dipoles"], GOLD[f"{name}_positions"], cell, pairs, shifts,
                      cell_gradient=False)
        assert step.n_k == len(classes) < len(grid) - 1
    direct = tpa.CalculatorDipole(tpa.PotentialDipole())
    mu, pos, cell, pairs, shifts = _small_system()
    assert _build(direct, torch.float64, mu, pos, cell, pairs, shifts).n_k == 0
