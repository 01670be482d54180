"""GraphedDipoleStep(follow_cell=True) on the GPU (mipme_dipole_cell_step, csrc/dipole_step.hip): E, F, dE/dmu and dE/dcell at
the construction cell and at other cells from ONE graph, against the reference's own outputs
(tests/golden/dipole_cell_step.npz), against the eager CalculatorDipole and against central differences of its own energy; the
status word; bit reproducibility; a direct potential; edge sizes; a new list.  And the object without the keyword: the same
golden, and the bits of the parent commit (profiles/step_skeleton_bits.txt); the object with the keyword has recorded bits too
(profiles/dipole_one_body_bits.txt)."""

import hashlib
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import torchpme_amd as tpa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_gpu_dipole_step import EPS32, _check, _eager, _small_system, _t  # noqa: E402  (the `_check` rule of the fixed-cell step)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(HERE, "golden", "dipole_cell_step.npz"))
DTYPES = [torch.float64, torch.float32]
STRAIN = np.eye(3) + GOLD["strain"]  # c1 = c0 STRAIN
# a third cell: 1 % larger and sheared; every |a_d| / lr_wavelength of the systems below stays between the same two integers
THIRD = 1.01 * np.eye(3) + np.array([[0.0, 0.008, 0.0], [0.0, 0.0, -0.006], [0.004, 0.0, 0.0]])
CASES = [f"tric_{n}" for n in GOLD["tric_variants"]] + ["big_half", "big_full"]


def _opt(x):
    x = float(x)
    return None if np.isnan(x) else x


def _calc(prefix):
    kw = dict(smearing=_opt(GOLD[f"{prefix}_smearing"]), exclusion_radius=_opt(GOLD[f"{prefix}_exclusion_radius"]),
              exclusion_degree=int(GOLD[f"{prefix}_exclusion_degree"]), epsilon=_opt(GOLD[f"{prefix}_epsilon"]) or 0.0,
              prefactor=_opt(GOLD[f"{prefix}_prefactor"]) or 1.0)
    return tpa.CalculatorDipole(tpa.PotentialDipole(**kw), full_neighbor_list=bool(GOLD[f"{prefix}_full"]),
                                lr_wavelength=_opt(GOLD[f"{prefix}_lr_wavelength"]))


def _system(prefix):
    """(dipoles, positions, cell, pairs, shifts) of a golden case"""
    if prefix.startswith("tric"):
        return (GOLD["tric_dipoles"], GOLD["tric_positions"], GOLD["tric_cell"], GOLD[f"{prefix}_pairs"].astype(np.int64),
                GOLD[f"{prefix}_shifts"].astype(np.int64))
    pairs, shifts = GOLD["big_pairs"].astype(np.int64), GOLD["big_shifts"].astype(np.int64)
    if prefix == "big_full":  # the half list followed by its mirror, as the golden script builds it
        pairs, shifts = np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])
    return GOLD["big_dipoles"], GOLD["big_positions"], GOLD["big_cell"], pairs, shifts


def _build(calc, dtype, mu, pos, cell, pairs, shifts, cell_gradient=True, follow_cell=True):
    ti = torch.tensor(np.asarray(pairs, dtype=np.int64), device=DEV)
    return tpa.GraphedDipoleStep(calc, _t(mu, dtype), _t(cell, dtype), _t(pos, dtype), ti, _t(shifts, dtype),
                                 cell_gradient=cell_gradient, follow_cell=follow_cell)


def _results(step, pos=None, mu=None, cell=None):
    args = [None if x is None else _t(x, step.dtype) for x in (pos, mu)]
    out = step(*args) if cell is None else step(*args, cell=_t(cell, step.dtype))
    torch.cuda.synchronize()
    res = dict(zip(("E", "F", "gmu", "gcell"), out))
    return {k: v.detach().double().cpu().numpy().copy() for k, v in res.items()}


def _status(step):
    return int(step.status.cpu()[0])


def _golden(prefix, ctag):
    want = {"E": np.float64(GOLD[f"{prefix}_E_{ctag}_f64"]), "F": -GOLD[f"{prefix}_gpos_{ctag}_f64"],
            "gmu": GOLD[f"{prefix}_gmu_{ctag}_f64"], "gcell": GOLD[f"{prefix}_gcell_{ctag}_f64"]}
    f32 = {"E": np.float64(GOLD[f"{prefix}_E_{ctag}_f32"]), "F": -GOLD[f"{prefix}_gpos_{ctag}_f32"].astype(np.float64),
           "gmu": GOLD[f"{prefix}_gmu_{ctag}_f32"].astype(np.float64), "gcell": GOLD[f"{prefix}_gcell_{ctag}_f32"].astype(np.float64)}
    return want, {k: np.abs(f32[k] - want[k]).max() for k in want}, float(GOLD[f"{prefix}_absE_{ctag}"])


def _bits(step, pos=None, mu=None, cell=None):
    args = [None if x is None else _t(x, step.dtype) for x in (pos, mu)]
    out = step(*args) if cell is None else step(*args, cell=_t(cell, step.dtype))
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- both cells, one graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prefix", CASES)
def test_both_cells_from_one_graph_match_the_reference(prefix, dtype):
    mu, pos, cell, pairs, shifts = _system(prefix)
    step = _build(_calc(prefix), dtype, mu, pos, cell, pairs, shifts)
    graph = step.graph
    assert tuple(step.cell.shape) == (3, 3) and step.status.dtype == torch.int32 and tuple(step.status.shape) == (1,)
    if prefix != "tric_direct":
        assert step.ns == tuple(int(n) for n in GOLD[prefix[:4].rstrip("_") + "_ns"]) and step.n_k > 0
    want, spread, abs_e = _golden(prefix, "c0")
    _check(_results(step), want, spread, abs_e, dtype, f"{prefix} c0")
    assert _status(step) == 0
    want, spread, abs_e = _golden(prefix, "c1")
    assert step.kgrid_matches(_t(cell @ STRAIN, dtype))
    _check(_results(step, pos=pos @ STRAIN, cell=cell @ STRAIN), want, spread, abs_e, dtype, f"{prefix} c1")
    assert _status(step) == 0 and step.graph is graph


@pytest.mark.parametrize("dtype", DTYPES)
def test_cells_come_and_go_without_a_recapture(dtype):
    mu, pos, cell, pairs, shifts = _system("tric_eps")
    step = _build(_calc("tric_eps"), dtype, mu, pos, cell, pairs, shifts)
    graph = step.graph
    first = _bits(step)
    other = _bits(step, pos=pos @ STRAIN, cell=cell @ STRAIN)
    again = _bits(step, pos=pos, cell=cell)
    assert step.graph is graph
    assert _same(first, again) and not torch.equal(first[0], other[0]) and not torch.equal(first[3], other[3])


# ---- a third cell against the eager call ---------------------------------------------------------------------------------------
def _follow_against_eager(calc, dtype, system, strain, what, res_of=None):
    """A step built at the system's cell and replayed at cell . strain with the positions scaled along, against the eager call at
    that cell (which chooses the same grid: asserted).  fp64: 1e-10 of the scale.  fp32: the bound of `_check` with the eager
    fp64 result as `want` and the eager call's own fp32 - fp64 spread in the place of the reference's."""
    mu, pos, cell, pairs, shifts = system
    moved = (mu, pos @ strain, cell @ strain, pairs, shifts)
    want = _eager(calc, torch.float64, *moved)
    abs_e = float(want.pop("absE"))
    spread = None
    if dtype == torch.float32:
        low = _eager(calc, torch.float32, *moved)
        spread = {k: np.abs(low[k] - want[k]).max() for k in want}
    step = _build(calc, dtype, *system)
    assert step.kgrid_matches(_t(moved[2], dtype))
    res = _results(step, pos=moved[1], cell=moved[2])
    assert _status(step) == 0
    if res_of is not None:
        res_of(res, want)
    _check(res, want, spread, abs_e, dtype, what)
    return step


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prefix", ["tric_half", "tric_excl3", "tric_eps", "big_full"])
def test_a_third_cell_matches_the_eager_call(prefix, dtype):
    _follow_against_eager(_calc(prefix), dtype, _system(prefix), THIRD, f"{prefix} third cell")


# ---- the construction cell: with and without the keyword -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prefix", ["tric_pref", "big_half"])
def test_construction_cell_with_and_without_the_keyword(prefix, dtype):
    system = _system(prefix)
    want, spread, abs_e = _golden(prefix, "c0")
    for follow in (True, False):
        step = _build(_calc(prefix), dtype, *system, follow_cell=follow)
        assert step.follow_cell is follow and hasattr(step, "status") is follow
        _check(_results(step), want, spread, abs_e, dtype, f"{prefix} follow_cell={follow}")


def _step_bits():
    spec = importlib.util.spec_from_file_location("step_bits", os.path.join(ROOT, "tools", "step_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("cell_gradient", [True, False], ids=["cg1", "cg0"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_object_without_the_keyword_has_the_bits_of_the_parent(dtype, cell_gradient):
    """The dipole lines of tools/step_bits.py (every system of the fixed-cell step's tests) hash to what
    profiles/step_skeleton_bits.txt records for the commits before the keyword."""
    lines = _step_bits().run_dipole(dtype, cell_gradient)
    head = " ".join(lines[0].split()[:3])
    got = f"## {head}: {len(lines)} lines, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}"
    recorded = open(os.path.join(ROOT, "profiles", "step_skeleton_bits.txt")).read().splitlines()
    assert got in recorded, got


@pytest.mark.parametrize("cell_gradient", [True, False], ids=["cg1", "cg0"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_cell_step_has_the_bits_of_the_parent(dtype, cell_gradient):
    """The same systems through the object WITH the keyword, each at its construction cell and at the strained one from the same
    graph (tools/step_bits.py --cell-step): the lines hash to what profiles/dipole_one_body_bits.txt records for the commit whose
    kernels of csrc/dipole_step.hip were written out in full."""
    lines = _step_bits().run_dipole(dtype, cell_gradient, follow_cell=True)
    head = " ".join(lines[0].split()[:3])
    got = f"## {head}: {len(lines)} lines, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}"
    recorded = open(os.path.join(ROOT, "profiles", "dipole_one_body_bits.txt")).read().splitlines()
    assert got in recorded, got


# ---- central differences of the step's own energy through `cell=` ----------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["tric_eps", "tric_excl3", "tric_direct"])
def test_finite_differences_of_the_cell(prefix):
    """Central differences with h = 1e-5 at fixed Cartesian positions, each of the nine components held to 1e-6 of the largest
    component of dE/dcell (step and bound of the Ewald step's test_finite_differences)."""
    mu, pos, cell, pairs, shifts = _system(prefix)
    step = _build(_calc(prefix), torch.float64, mu, pos, cell, pairs, shifts)
    base = _results(step)
    h = 1e-5
    scale = np.abs(base["gcell"]).max()
    for a in range(3):
        for b in range(3):
            e = []
            for sgn in (+1, -1):
                moved = cell.copy()
                moved[a, b] += sgn * h
                e.append(float(_results(step, cell=moved)["E"]))
            fd, got = (e[0] - e[1]) / (2 * h), base["gcell"][a, b]
            print(f"finite difference dE/dcell[{a},{b}]: {fd:.12e} analytic {got:.12e}")
            assert abs(fd - got) <= 1e-6 * scale
    assert _status(step) == 0


# ---- the status word ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_status_bit_0_another_grid_and_the_energy_of_the_kept_one(dtype):
    """A cell scaled by 1.2: the eager call would choose another grid, the step keeps its own and says so.  What it returns is
    what the reference gives for the kept grid (lr_wavelength 0.6 at 1.2 cell: the frequencies of the construction cell)."""
    mu, pos, cell, pairs, shifts = _system("tric_half")
    step = _build(_calc("tric_half"), dtype, mu, pos, cell, pairs, shifts)
    scale = float(GOLD["kept_scale"])
    assert not step.kgrid_matches(_t(scale * cell, dtype))
    res = _results(step, pos=scale * pos, cell=scale * cell)
    assert _status(step) == 1
    want, spread, abs_e = _golden("kept", "c0")
    _check(res, want, spread, abs_e, dtype, "kept grid")
    other, _, _ = _golden("tric_half", "c0")
    assert abs(float(res["E"]) - float(other["E"])) > 1e-3 * abs_e


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_bit_1_singular_cell_and_recovery(dtype):
    mu, pos, cell, pairs, shifts = _system("tric_half")
    step = _build(_calc("tric_half"), dtype, mu, pos, cell, pairs, shifts)
    first = _bits(step)
    singular = cell.copy()
    singular[2] = singular[0]
    res = _results(step, cell=singular)
    assert _status(step) & 2 and np.isnan(res["E"])
    assert _same(_bits(step, cell=cell), first)  # the next valid cell: the bits of the construction cell again
    assert _status(step) == 0


# ---- equal inputs, equal bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell_gradient", [True, False], ids=["cell", "nocell"])
def test_two_objects_and_repeated_replays_agree_bitwise_in_fp32(cell_gradient):
    mu, pos, cell, pairs, shifts = _system("big_half")
    a = _build(_calc("big_half"), torch.float32, mu, pos, cell, pairs, shifts, cell_gradient=cell_gradient)
    b = _build(_calc("big_half"), torch.float32, mu, pos, cell, pairs, shifts, cell_gradient=cell_gradient)
    c1, p1 = cell @ STRAIN, pos @ STRAIN
    first = _bits(a, pos=p1, cell=c1)
    assert len(first) == (4 if cell_gradient else 3)
    assert _same(first, _bits(b, pos=p1, cell=c1)) and _same(first, _bits(a)) and _same(first, _bits(a))


# ---- a direct potential ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_direct_potential_follows_the_cell(dtype):
    """No reciprocal part: n_k == 0, bit 0 is never set -- not at 1.2 cell either --, bit 1 and the NaN energy as ever."""
    system = _system("tric_direct")
    step = _follow_against_eager(_calc("tric_direct"), dtype, system, THIRD, "direct third cell")
    assert step.n_k == 0
    _follow_against_eager(_calc("tric_direct"), dtype, system, 1.2 * np.eye(3), "direct 1.2 cell")  # (asserts status 0)
    cell = system[2]
    singular = cell.copy()
    singular[2] = singular[0]  # (a . (b x a) is an exact zero for this cell: the rule of es_invert_cell is det == 0 or not finite)
    assert np.isnan(_results(step, cell=singular)["E"]) and _status(step) == 2


# ---- edge sizes ----------------------------------------------------------------------------------------------------------------
def _one_atom_force_scale(calc, mu, pos, cell):
    """The force on one dipole among its own images is zero term by term, F = -(1 / V) sum_k G (mu.k)^2 k (c s - s c), so a result
    holds rounding residue only and there is no "largest wanted value".  What the residue is measured against is the sum of the
    terms' magnitudes, each with the weight of its phase error: cos and sin of k.r come from two launches, and a phase formed in
    the working precision carries an error of |k.r| ulps (csrc/dipole_device.h), hence (1 / V) sum_k |G| (mu.k)^2 |k| (1 + |k.r|)
    (the rule of the Ewald step's test for one charge)."""
    from torchpme_amd.calculators import _integer_frequencies, _reciprocal_and_det

    tc = torch.tensor(cell, dtype=torch.float64)
    kv = ((2 * math.pi) * _integer_frequencies(tc, calc.lr_wavelength, None)[0] @ _reciprocal_and_det(tc)[0]).numpy()[1:]
    k2 = (kv * kv).sum(axis=1)
    G = 4 * math.pi * np.exp(-0.5 * float(calc.potential.smearing) ** 2 * k2) / k2
    weight = (kv @ mu[0]) ** 2 * np.sqrt(k2) * (1 + np.abs(kv @ pos[0]))
    return float((G * weight).sum() / abs(np.linalg.det(cell)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 5])
def test_no_pairs(n, dtype):
    """One atom, and five atoms with an empty list, at a strained cell: the reciprocal part, the self and the background term alone."""
    rng = np.random.default_rng(7)
    cell = np.array([[5.8, 0.0, 0.0], [0.5, 6.5, 0.0], [0.0, -0.4, 7.0]])
    system = (rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 3)) @ cell, cell, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3)))
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0, epsilon=2.0), lr_wavelength=1.5)

    def one_atom(res, want):
        if n > 1:
            return
        scale = _one_atom_force_scale(calc, system[0], system[1] @ THIRD, cell @ THIRD)
        want.pop("F")
        err, tol = np.abs(res.pop("F")).max(), (1e-10 if dtype == torch.float64 else 4 * EPS32) * scale
        print(f"1 atom F {dtype}: residue {err:.3e}, bound {tol:.3e}, scale {scale:.3e}")
        assert err <= tol

    _follow_against_eager(calc, dtype, system, THIRD, f"{n} atoms, no pairs", res_of=one_atom)


@pytest.mark.parametrize("dtype", DTYPES)
def test_8_atoms_against_40_cubed_kvectors(dtype):
    """Few atoms, many k-vectors: more than 16 k slices per atom, summed by the 16 lanes of the finish launch."""
    rng = np.random.default_rng(8)
    cell = 9.85 * np.eye(3)
    pos = rng.uniform(0, 9.85, (8, 3))
    mu = rng.normal(size=(8, 3))
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, 4.5)
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.5), lr_wavelength=0.25)
    step = _follow_against_eager(calc, dtype, (mu, pos, cell, pairs, shifts), STRAIN, "8 atoms")
    assert step.ns == (40, 40, 40) and step.n_k >= 40**3 // 2 - 1
    assert min(2048 // 8, step.n_k // 1024) > 16  # (the slice rule of csrc/step_device.h)


@pytest.mark.parametrize("dtype", DTYPES)
def test_37_atoms_the_last_row_block_is_partial(dtype):
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=0.9, epsilon=2.0, prefactor=1.7), lr_wavelength=0.7)
    _follow_against_eager(calc, dtype, _small_system(), THIRD, "37 atoms")


# ---- a new list ------------------------------------------------------------------------------------------------------------------
def test_recapture_with_a_cell_and_a_refused_list():
    dtype = torch.float32
    mu, pos, cell, pairs, shifts = _system("tric_half")
    p2, s2, _ = tpa.neighbor_list(pos, cell, 3.0)
    assert 0 < len(p2) < len(pairs)
    calc = _calc("tric_half")
    step = _build(calc, dtype, mu, pos, cell, pairs, shifts)
    graph, before = step.graph, _bits(step)
    c1, p1 = cell @ STRAIN, pos @ STRAIN
    with pytest.raises(ValueError, match=r"integers in \[-3, 3\]"):
        step.recapture(torch.tensor(p2, device=DEV), _t(s2 * 4 + 4, dtype), cell=_t(c1, dtype))
    with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\]"):
        step.recapture(torch.tensor(p2, device=DEV), _t(s2, dtype), cell=_t(c1, torch.float64))
    with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\]"):
        step(cell=_t(c1, dtype).cpu())
    assert step.graph is graph and torch.equal(step.cell, _t(cell, dtype)) and _same(_bits(step), before)
    step.recapture(torch.tensor(p2, device=DEV), _t(s2, dtype), positions=_t(p1, dtype), cell=_t(c1, dtype))
    assert step.graph is not graph and torch.equal(step.cell, _t(c1, dtype))
    after = _bits(step)
    fresh = _build(calc, dtype, mu, pos, cell, p2, s2)  # the same frozen grid: built at c0, replayed at c1
    assert _same(after, _bits(fresh, pos=p1, cell=c1)) and not torch.equal(before[1], after[1])
    # an object without the keyword takes no cell
    plain = _build(calc, dtype, mu, pos, cell, pairs, shifts, follow_cell=False)
    with pytest.raises(ValueError, match="follow_cell=True"):
        plain(cell=_t(c1, dtype))
    with pytest.raises(ValueError, match="follow_cell=True"):
        plain.recapture(torch.tensor(p2, device=DEV), _t(s2, dtype), cell=_t(c1, dtype))
