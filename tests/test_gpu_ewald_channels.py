"""GraphedEwaldStep and GraphedEwaldBatch with SEVERAL charge channels on the GPU (csrc/ewald_channels_step.hip,
csrc/ewald_channels_batch.hip): (N, C) charges against the reference's own outputs at two cells from ONE captured graph
(tests/golden/ewald_channels.npz), against C single-channel objects (the channels are independent), against finite differences of
the step's own energy, bit reproducibility of the step and of the batch, ``n_channels=1`` against the objects built without the
keyword, edge sizes against the eager calculator, new lists and the refusals that need a device.

Every test that passes ``n_channels`` fails on the code before the keyword existed with a TypeError."""

import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

import torchpme_amd as tpa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_ewald_batch as B  # noqa: E402  (the five frames and the two calculators of the batch)
import test_gpu_ewald_step as S  # noqa: E402  (the `_check` rule, the eager call, the systems of the step)
from test_gpu_ewald_step import EPS32, LAM, STRAIN, _check, _eager, _same, _t  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(HERE, "golden", "ewald_channels.npz"))
DTYPES = [torch.float64, torch.float32]
F64, F32 = torch.float64, torch.float32
# case: the case of ewald_step.npz whose potential, list kind and list it uses
STEP_CASES = {"tric_c3_net": "tric_half", "tric_c2_excl": "tric_excl", "tric_c2_ipl6": "tric_ipl6", "tric_c8_half": "tric_half",
              "big_c3_half": "big_half", "big_c2_full": "big_full"}
ALL = (0, 1, 2, 3, 4)


def test_the_keyword_is_exported():
    for cls in (tpa.GraphedEwaldStep, tpa.GraphedEwaldBatch):
        assert "n_channels" in inspect.signature(cls.__init__).parameters


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _system(case):
    """(charges (N, C), positions, cell, pairs, shifts) of a step case at its construction cell."""
    _, pos, cell, pairs, shifts = S._system(STEP_CASES[case])
    return GOLD[f"{case}_charges"], pos, cell, pairs, shifts


def _build(calc, dtype, q, pos, cell, pairs, shifts, cell_gradient=True, n_channels=None):
    ti = torch.tensor(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), device=DEV)
    q = np.asarray(q)
    return tpa.GraphedEwaldStep(calc, _t(q, dtype), _t(cell, dtype), _t(pos, dtype), ti, _t(np.asarray(shifts).reshape(-1, 3), dtype),
                                cell_gradient=cell_gradient, n_channels=q.shape[1] if n_channels is None else n_channels)


def _golden(prefix, ctag):
    g = lambda k, tag: GOLD[f"{prefix}_{k}_{ctag}_{tag}"].astype(np.float64)  # noqa: E731
    want = {"E": np.float64(g("E", "f64")), "F": -g("gpos", "f64"), "gq": g("gq", "f64"), "gcell": g("gcell", "f64")}
    f32 = {"E": np.float64(g("E", "f32")), "F": -g("gpos", "f32"), "gq": g("gq", "f32"), "gcell": g("gcell", "f32")}
    return want, {k: np.abs(f32[k] - want[k]).max() for k in want}, float(GOLD[f"{prefix}_absE_{ctag}"])


def _frame(n, full, dtype, channel=None):
    """Frame n of the batch with its C = 3 charges, or with channel `channel` of them alone."""
    _, pos, cell, pairs, shifts = B._system(n, full)
    q = GOLD[f"f{n}_charges"]
    if channel is not None:
        q = q[:, channel:channel + 1]
    return (_t(q, dtype), _t(cell, dtype), _t(pos, dtype), torch.tensor(pairs, device=DEV), _t(shifts, dtype))


def _batch(cname, dtype, which=ALL, cell_gradient=True):
    full = B.CALCS[cname][1]
    return tpa.GraphedEwaldBatch(B._calc(cname), [_frame(n, full, dtype) for n in which], cell_gradient=cell_gradient, n_channels=3)


# ---- against the reference, at both cells, from one graph -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_cases_match_the_reference_at_both_cells(case, dtype):
    q, pos, cell, pairs, shifts = _system(case)
    step = _build(S._calc(STEP_CASES[case]), dtype, q, pos, cell, pairs, shifts)
    C = q.shape[1]
    assert step.n_channels == C and step.charge_grad.shape == (len(q), C) and step.forces.shape == (len(q), 3)
    assert step.ns == ((16, 16, 16) if case.startswith("big") else (8, 7, 9))
    graph = step.graph
    _check(S._results(step), *_golden(case, "c0"), dtype, f"{case} cell0")
    assert S._status(step) == 0
    res = S._results(step, _t(pos @ STRAIN, dtype), cell=_t(cell @ STRAIN, dtype))
    _check(res, *_golden(case, "c1"), dtype, f"{case} cell1")
    assert S._status(step) == 0 and step.graph is graph
    if case == "tric_c8_half":  # a channel without charges gets no gradient, exactly; the others do
        assert not res["gq"][:, 2].any() and res["gq"][:, 5].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
def test_five_frames_match_the_reference_and_follow_their_cells(cname, dtype):
    full = B.CALCS[cname][1]
    batch = _batch(cname, dtype)
    assert batch.n_channels == 3 and batch.charge_grads_flat.shape == (344, 3) and batch.atom_ptr == [0, 1, 3, 20, 44, 344]
    assert batch.n_k[0] == 0 and batch.n_k[4] >= 2048
    for f, (a, b) in enumerate(zip(batch.atom_ptr[:-1], batch.atom_ptr[1:])):
        assert batch.charge_grads[f].shape == (b - a, 3)
        assert batch.charge_grads[f].data_ptr() == batch.charge_grads_flat[a:b].data_ptr()
    graph = batch.graph
    res = B._results(batch)
    for n in ALL:
        _check(res[n], *_golden(f"{cname}_f{n}", "c0"), dtype, f"{cname} f{n} cell0")
    assert B._status(batch) == [0] * 5
    # ONE call: frames 0, 2 and 4 move to the strained cell (positions and cell), frames 1 and 3 stay
    moved = (0, 2, 4)
    pos, cells = [], []
    for n in ALL:
        _, p, c, _, _ = B._system(n, full)
        pos.append(_t(p @ STRAIN if n in moved else p, dtype))
        cells.append(_t(c @ STRAIN if n in moved else c, dtype))
    res = B._results(batch, positions=pos, cells=cells)
    for n in ALL:
        ctag = "c1" if n in moved else "c0"
        _check(res[n], *_golden(f"{cname}_f{n}", ctag), dtype, f"{cname} f{n} {ctag} (mixed call)")
    assert B._status(batch) == [0] * 5 and batch.graph is graph and batch.kgrid_matches(cells) == [True] * 5


# ---- the channels are independent ---------------------------------------------------------------------------------------------
def _sum_of_channels(per_channel):
    out = {k: sum(r[k] for r in per_channel) for k in ("E", "F", "gcell")}
    out["gq"] = np.concatenate([r["gq"] for r in per_channel], axis=1)
    return out


def _check_1e10(res, want, what):
    for key in want:
        scale, err = np.abs(want[key]).max(), np.abs(res[key] - want[key]).max()
        print(f"{what} {key}: max difference {err:.3e}, bound {1e-10 * scale:.3e}")
        assert res[key].shape == want[key].shape and err <= 1e-10 * scale, (what, key, err, scale)


def test_step_equals_the_sum_of_single_channel_steps():
    """big_c3_half in fp64 at the strained cell: E, F and dE/dcell of one n_channels=3 step are the sums over three single-channel
    GraphedEwaldStep objects (the single-channel kernels), dE/dq their concatenation, to 1e-10 of the largest value."""
    case = "big_c3_half"
    q, pos, cell, pairs, shifts = _system(case)
    calc = S._calc(STEP_CASES[case])
    p1, c1 = _t(pos @ STRAIN, F64), _t(cell @ STRAIN, F64)
    res = S._results(_build(calc, F64, q, pos, cell, pairs, shifts), p1, cell=c1)
    singles = [S._results(S._build(calc, F64, q[:, c:c + 1], pos, cell, pairs, shifts), p1, cell=c1) for c in range(3)]
    _check_1e10(res, _sum_of_channels(singles), case)


@pytest.mark.parametrize("cname", ["C1", "C2"])
def test_batch_equals_the_sum_of_single_channel_batches(cname):
    full = B.CALCS[cname][1]
    systems = [B._system(n, full) for n in ALL]
    pos = [_t(s[1] @ STRAIN, F64) for s in systems]
    cells = [_t(s[2] @ STRAIN, F64) for s in systems]
    res = B._results(_batch(cname, F64), positions=pos, cells=cells)
    singles = []
    for c in range(3):
        one = tpa.GraphedEwaldBatch(B._calc(cname), [_frame(n, full, F64, channel=c) for n in ALL], cell_gradient=True)
        singles.append(B._results(one, positions=pos, cells=cells))
    for n in ALL:
        want = _sum_of_channels([singles[c][n] for c in range(3)])
        if n == 0:  # one atom: no force to compare with, residue on both sides
            want.pop("F")
        _check_1e10(res[n], want, f"{cname} f{n}")


# ---- finite differences of the step's own energy -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tric_c3_net", "tric_c2_ipl6"])
def test_finite_differences(case):
    """Central differences with h = 1e-5, every component held to 1e-6 of the largest component of its array, as in
    tests/test_gpu_ewald_step.py::test_finite_differences: all nine components of dE/dcell, the three largest of F, and the three
    largest of dE/dq IN EACH CHANNEL."""
    d = F64
    q, pos, cell, pairs, shifts = _system(case)
    step = _build(S._calc(STEP_CASES[case]), d, q, pos, cell, pairs, shifts)
    base = S._results(step)
    h = 1e-5

    def energy(q_=q, pos_=pos, cell_=cell):
        return float(S._results(step, _t(pos_, d), _t(q_, d), _t(cell_, d))["E"])

    def central(which, idx):
        e = []
        for sgn in (+1, -1):
            moved = {"q_": q.copy(), "pos_": pos.copy(), "cell_": cell.copy()}
            moved[which][idx] += sgn * h
            e.append(energy(**moved))
        return (e[0] - e[1]) / (2 * h)

    scale = np.abs(base["gcell"]).max()
    for a in range(3):
        for b in range(3):
            fd, got = central("cell_", (a, b)), base["gcell"][a, b]
            print(f"finite difference dE/dcell[{a},{b}]: {fd:.12e} analytic {got:.12e}")
            assert abs(fd - got) <= 1e-6 * scale
    scale = np.abs(base["F"]).max()
    for flat in np.argsort(-np.abs(base["F"]).ravel())[:3]:
        idx = np.unravel_index(flat, base["F"].shape)
        fd, got = central("pos_", idx), -base["F"][idx]
        print(f"finite difference F{list(idx)}: {fd:.12e} analytic {got:.12e}")
        assert abs(fd - got) <= 1e-6 * scale
    scale = np.abs(base["gq"]).max()
    for c in range(q.shape[1]):
        for a in np.argsort(-np.abs(base["gq"][:, c]))[:3]:
            fd, got = central("q_", (a, c)), base["gq"][a, c]
            print(f"finite difference dE/dq[{a},{c}]: {fd:.12e} analytic {got:.12e}")
            assert abs(fd - got) <= 1e-6 * scale


# ---- equal inputs, equal bits: the step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell_gradient", [True, False], ids=["cell", "nocell"])
def test_two_objects_and_repeated_replays_agree_bitwise_in_fp32(cell_gradient):
    case = "big_c3_half"
    q, pos, cell, pairs, shifts = _system(case)
    calc = S._calc(STEP_CASES[case])
    a = _build(calc, F32, q, pos, cell, pairs, shifts, cell_gradient=cell_gradient)
    b = _build(calc, F32, q, pos, cell, pairs, shifts, cell_gradient=cell_gradient)
    first = S._bits(a)
    assert len(first) == (4 if cell_gradient else 3)
    assert _same(first, S._bits(b)) and _same(first, S._bits(a)) and _same(first, S._bits(a))
    c1 = _t(cell @ STRAIN, F32)
    assert _same(S._bits(a, cell=c1), S._bits(b, cell=c1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cells_come_and_go_without_a_recapture(dtype):
    case = "tric_c3_net"
    q, pos, cell, pairs, shifts = _system(case)
    step = _build(S._calc(STEP_CASES[case]), dtype, q, pos, cell, pairs, shifts)
    graph = step.graph
    p0, c0, p1, c1 = _t(pos, dtype), _t(cell, dtype), _t(pos @ STRAIN, dtype), _t(cell @ STRAIN, dtype)
    first = S._bits(step, p0, cell=c0)
    other = S._bits(step, p1, cell=c1)
    again = S._bits(step, p0, cell=c0)
    assert step.graph is graph and _same(first, again)
    assert not torch.equal(first[0], other[0]) and not torch.equal(first[3], other[3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_new_charges_equal_a_fresh_object_to_the_bit(dtype):
    case = "tric_c3_net"
    q, pos, cell, pairs, shifts = _system(case)
    q2 = np.random.default_rng(4).normal(size=q.shape) + np.array([0.1, 0.0, -0.2])
    calc = S._calc(STEP_CASES[case])
    step = _build(calc, dtype, q, pos, cell, pairs, shifts)
    fresh = _build(calc, dtype, q2, pos, cell, pairs, shifts)
    graph, before = step.graph, S._bits(step)
    after = S._bits(step, charges=_t(q2, dtype))
    assert step.graph is graph
    assert _same(after, S._bits(fresh)) and not torch.equal(before[2], after[2])
    assert _same(S._bits(step, charges=_t(q, dtype)), before)


# ---- equal inputs, equal bits: the batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
def test_a_frames_bits_do_not_depend_on_the_batch(cname, dtype):
    batch = _batch(cname, dtype)
    first = B._bits(batch)
    assert all(B._same(a, b) for a, b in zip(first, B._bits(batch)))  # equal inputs, equal bits
    backwards = B._bits(_batch(cname, dtype, which=ALL[::-1]))
    for n in ALL:
        assert B._same(first[n], backwards[4 - n]), f"frame {n} in the reversed batch"
        assert B._same(first[n], B._bits(_batch(cname, dtype, which=(n,)))[0]), f"frame {n} alone"
    pair, swapped = B._bits(_batch(cname, dtype, which=(2, 4))), B._bits(_batch(cname, dtype, which=(4, 2)))
    assert B._same(pair[0], swapped[1]) and B._same(pair[1], swapped[0]) and B._same(pair[0], first[2]) and B._same(pair[1], first[4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_singular_cell_is_its_own_frames_business(dtype):
    cname, full = "C1", False
    batch = _batch(cname, dtype)
    graph, first = batch.graph, B._bits(batch)
    systems = [B._system(n, full) for n in ALL]
    cells0 = [_t(s[2], dtype) for s in systems]
    singular = systems[1][2].copy()
    singular[2] = singular[0]
    cells = list(cells0)
    cells[1] = _t(singular, dtype)
    broken = B._bits(batch, cells=cells)
    assert bool(torch.isnan(broken[1][0])) and bool(torch.isnan(broken[1][3]).all()) and int(broken[1][4]) == 2
    for n in (0, 2, 3, 4):
        assert B._same(first[n], broken[n]) and int(broken[n][4]) == 0, f"frame {n} beside a singular cell"
    again = B._bits(batch, cells=cells0)
    assert all(B._same(a, b) for a, b in zip(first, again)) and batch.graph is graph and B._status(batch) == [0] * 5


@pytest.mark.parametrize("cname", ["C1", "C2"])
@pytest.mark.parametrize("n", ALL)
def test_a_batch_of_one_frame_equals_the_step(n, cname):
    """fp64: to the bit (both kernel families run the bodies of csrc/ewald_channels_bodies.h).  fp32: the number of equal outputs
    is reported and the rest is held to 4 eps32 of the scale (the largest value of the array; sum |q V| for the scalar E): the
    dipole batch found differences of a few ulps between its two kernel families."""
    full = B.CALCS[cname][1]
    _, p, c, _, _ = B._system(n, full)
    for dtype in DTYPES:
        q, cell, pos, idx, sh = _frame(n, full, dtype)
        step = tpa.GraphedEwaldStep(B._calc(cname), q, cell, pos, idx, sh, cell_gradient=True, n_channels=3)
        batch = _batch(cname, dtype, which=(n,))
        for ctag, m in (("c0", np.eye(3)), ("c1", STRAIN)):
            pos_m, cell_m = _t(p @ m, dtype), _t(c @ m, dtype)
            one = [o.clone() for o in step(positions=pos_m, cell=cell_m)] + [step.status[0].clone()]
            got = B._bits(batch, positions=[pos_m], cells=[cell_m])[0]
            torch.cuda.synchronize()
            abs_e = float(GOLD[f"{cname}_f{n}_absE_{ctag}"])
            equal = 0
            for key, a, b in zip(("E", "F", "gq", "gcell", "status"), one, got):
                assert a.shape == b.shape
                if torch.equal(a, b):
                    equal += 1
                    continue
                assert dtype == F32, f"{cname} f{n} {ctag} fp64: {key} of the step and of the batch differ"
                scale = abs_e if key == "E" else float(a.abs().max())
                err = float((a.double() - b.double()).abs().max())
                print(f"{cname} f{n} {ctag} fp32 {key}: step and batch differ by {err:.3e}, bound {4 * EPS32 * scale:.3e}")
                assert err <= 4 * EPS32 * scale
            print(f"{cname} f{n} {ctag} {dtype}: {equal} of 5 outputs equal to the bit")
            assert int(got[4]) == 0


# ---- n_channels=1 is the object built without the keyword ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_explicit_one_channel_step_is_the_step_without_the_keyword(dtype):
    for prefix in ("tric_net", "tric_ipl6"):
        q, pos, cell, pairs, shifts = S._system(prefix)
        calc = S._calc(prefix)
        plain = S._build(calc, dtype, q, pos, cell, pairs, shifts)
        one = _build(calc, dtype, q, pos, cell, pairs, shifts, n_channels=1)
        assert one.n_channels == 1 and plain.n_channels == 1
        assert _same(S._bits(plain), S._bits(one))
        p1, c1 = _t(pos @ STRAIN, dtype), _t(cell @ STRAIN, dtype)
        a, b = S._bits(plain, p1, cell=c1), S._bits(one, p1, cell=c1)
        assert len(a) == len(b) == 4 and _same(a, b) and torch.equal(plain.status, one.status)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
def test_explicit_one_channel_batch_is_the_batch_without_the_keyword(cname, dtype):
    full = B.CALCS[cname][1]
    frames = [B._frame(n, full, dtype) for n in ALL]
    plain = tpa.GraphedEwaldBatch(B._calc(cname), frames, cell_gradient=True)
    one = tpa.GraphedEwaldBatch(B._calc(cname), frames, cell_gradient=True, n_channels=1)
    assert one.n_channels == 1 and plain.n_channels == 1
    a, b = B._bits(plain), B._bits(one)
    assert all(len(x) == 5 and B._same(x, y) for x, y in zip(a, b))
    assert torch.equal(plain.forces_flat, one.forces_flat) and torch.equal(plain.charge_grads_flat, one.charge_grads_flat)


# ---- edge sizes, against the eager calculator -------------------------------------------------------------------------------
def _check_against_eager(calc, dtype, system, what):
    """The rule of tests/test_gpu_ewald_step.py::_check_against_eager.  One atom: the force is held to 1e-10 / 4 eps32 of
    `_one_atom_force_scale` with sum_c q_c^2 in the place of q^2."""
    want = _eager(calc, F64, *system)
    abs_e = float(want.pop("absE"))
    spread = None
    if dtype == F32:
        low = _eager(calc, F32, *system)
        low.pop("absE")
        spread = {k: np.abs(low[k] - want[k]).max() for k in want}
    step = _build(calc, dtype, *system)
    res = S._results(step)
    if len(system[0]) == 1:
        q_all = np.array([[math.sqrt(float((system[0] ** 2).sum()))]])
        scale = S._one_atom_force_scale(calc, q_all, *system[1:3])
        want.pop("F")
        err, tol = np.abs(res.pop("F")).max(), (1e-10 if dtype == F64 else 4 * EPS32) * scale
        print(f"{what} F {dtype}: residue {err:.3e}, bound {tol:.3e}, scale {scale:.3e}")
        assert err <= tol
    _check(res, want, spread, abs_e, dtype, what)
    return step


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, C", [(1, 2), (5, 3)])
def test_no_pairs(n, C, dtype):
    """One atom with two channels, and five atoms with three, each with an empty list: the reciprocal part, the self and the
    background term alone -- per channel."""
    rng = np.random.default_rng(7)
    cell = np.array([[6.0, 0.0, 0.0], [0.5, 6.5, 0.0], [0.0, -0.4, 7.0]])
    q = rng.normal(size=(n, C)) + np.linspace(0.2, -0.3, C)
    system = (q, rng.uniform(0, 1, (n, 3)) @ cell, cell, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3)))
    calc = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=1.0), lr_wavelength=1.5)
    _check_against_eager(calc, dtype, system, f"{n} atoms, {C} channels, no pairs")


@pytest.mark.parametrize("dtype", DTYPES)
def test_8_atoms_8_channels_against_40_cubed_kvectors(dtype):
    """Few atoms, many k-vectors: more than a hundred k slices per atom, C + 3 = 11 partials each, summed by the 16 lanes of the
    finish launch."""
    rng = np.random.default_rng(8)
    cell = 10.0 * np.eye(3)
    pos = rng.uniform(0, 10.0, (8, 3))
    q = rng.normal(size=(8, 8))
    q -= q.mean(axis=0)
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, 4.5)
    calc = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=0.5), lr_wavelength=0.25)
    step = _check_against_eager(calc, dtype, (q, pos, cell, pairs, shifts), "8 atoms, 8 channels")
    assert step.ns == (40, 40, 40) and step.n_k >= 40**3 // 2 - 1 and step.n_channels == 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
@pytest.mark.parametrize("copies", [1, 2])
def test_a_batch_whose_frames_all_have_no_kvectors(cname, copies, dtype):
    batch = _batch(cname, dtype, which=(0,) * copies)
    assert batch.n_k == [0] * copies and batch.ns == [(1, 1, 1)] * copies
    res = B._results(batch)
    for f in range(copies):
        _check(res[f], *_golden(f"{cname}_f0", "c0"), dtype, f"{cname} f0 (copy {f} of {copies})")
    _, p, c, _, _ = B._system(0, False)
    res = B._results(batch, positions=[_t(p @ STRAIN, dtype)] * copies, cells=[_t(c @ STRAIN, dtype)] * copies)
    for f in range(copies):
        _check(res[f], *_golden(f"{cname}_f0", "c1"), dtype, f"{cname} f0 strained (copy {f} of {copies})")
    assert B._status(batch) == [0] * copies


def test_status_bit_0_another_grid_and_the_energy_of_the_kept_one():
    """A cell scaled by 1.2: the eager call would choose another grid, the step keeps its own and says so.  What it returns is
    the eager result for the step's own frequencies, handed to the eager call as ``kvectors=``."""
    from torchpme_amd.calculators import _integer_frequencies, _reciprocal_and_det

    d = F64
    case = "tric_c3_net"
    q, pos, cell, pairs, shifts = _system(case)
    calc = S._calc(STEP_CASES[case])
    step = _build(calc, d, q, pos, cell, pairs, shifts)
    cell2, pos2 = 1.2 * cell, 1.2 * pos
    assert not step.kgrid_matches(_t(cell2, d))
    res = S._results(step, _t(pos2, d), cell=_t(cell2, d))
    assert S._status(step) == 1 and np.isfinite(res["E"])
    freq, _ = _integer_frequencies(_t(cell, d), LAM, None)
    kv = (2 * math.pi) * freq @ _reciprocal_and_det(_t(cell2, d))[0]
    want = _eager(calc, d, q, pos2, cell2, pairs, shifts, kvectors=kv)
    abs_e = float(want.pop("absE"))
    want.pop("gcell")  # (the k-vectors are a constant of that call)
    res.pop("gcell")
    _check(res, want, None, abs_e, d, "kept grid")
    own = _eager(calc, d, q, pos2, cell2, pairs, shifts)
    assert abs(float(own["E"]) - float(want["E"])) > 1e-8 * abs_e  # (the other grid is another energy indeed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_status_bit_1_singular_cell_and_recovery(dtype):
    case = "tric_c2_excl"
    q, pos, cell, pairs, shifts = _system(case)
    step = _build(S._calc(STEP_CASES[case]), dtype, q, pos, cell, pairs, shifts)
    singular = cell.copy()
    singular[2] = singular[0]
    res = S._results(step, cell=_t(singular, dtype))
    assert S._status(step) & 2 and np.isnan(res["E"])
    _check(S._results(step, cell=_t(cell, dtype)), *_golden(case, "c0"), dtype, "after a singular cell")
    assert S._status(step) == 0


# ---- new lists and refusals ------------------------------------------------------------------------------------------------------
def test_recapture_with_another_list_and_a_refused_one():
    dtype = F32
    case = "tric_c3_net"
    q, pos, cell, pairs, shifts = _system(case)
    p2, s2, _ = tpa.neighbor_list(pos, cell, 3.0)
    assert 0 < len(p2) < len(pairs)
    calc = S._calc(STEP_CASES[case])
    step = _build(calc, dtype, q, pos, cell, pairs, shifts)
    graph, before = step.graph, S._bits(step)
    with pytest.raises(ValueError, match=r"integers in \[-3, 3\]"):
        step.recapture(torch.tensor(p2, device=DEV), _t(s2 * 4 + 4, dtype))
    with pytest.raises(ValueError, match=r"\[n_atoms, n_channels\] = \[24, 3\].*\[24, 1\]"):
        step.recapture(torch.tensor(p2, device=DEV), _t(s2, dtype), charges=_t(q[:, :1], dtype))
    assert step.graph is graph and _same(S._bits(step), before)
    step.recapture(torch.tensor(p2, device=DEV), _t(s2, dtype))
    fresh = _build(calc, dtype, q, pos, cell, p2, s2)
    after = S._bits(step)
    assert step.graph is not graph
    assert _same(after, S._bits(fresh)) and not torch.equal(before[1], after[1])


def test_batch_recapture_with_new_lists_and_a_refused_one():
    dtype, cname = F32, "C1"
    batch = _batch(cname, dtype)
    systems = [B._system(n, False) for n in ALL]
    lists = [(torch.tensor(s[3], device=DEV), _t(s[4], dtype)) for s in systems]
    graph, pairs, before = batch.graph, batch.pairs, B._bits(batch)
    bad = list(lists)
    sh = systems[2][4].copy()
    sh[0, 1] = 4
    bad[2] = (lists[2][0], _t(sh, dtype))
    with pytest.raises(ValueError, match=r"frame 2.*integers in \[-3, 3\]"):
        batch.recapture(bad)
    assert batch.graph is graph and batch.pairs is pairs and all(B._same(a, b) for a, b in zip(before, B._bits(batch)))
    p4, s4, _ = tpa.neighbor_list(systems[4][1], systems[4][2], 3.0)
    assert 0 < len(p4) < len(systems[4][3])
    new = list(lists)
    new[4] = (torch.tensor(np.asarray(p4, dtype=np.int64), device=DEV), _t(s4, dtype))
    batch.recapture(new)
    assert batch.graph is not graph and batch.pairs[4] is new[4][0]
    after = B._bits(batch)
    for n in (0, 1, 2, 3):
        assert B._same(before[n], after[n])
    assert not torch.equal(before[4][1], after[4][1])
    q, cell, pos, _, _ = _frame(4, False, dtype)
    step = tpa.GraphedEwaldStep(B._calc(cname), q, cell, pos, new[4][0], new[4][1], cell_gradient=True, n_channels=3)
    one = [o.clone() for o in step()]
    torch.cuda.synchronize()
    for key, a, b in zip(("E", "F", "gq", "gcell"), one, after[4]):
        scale = float(GOLD["C1_f4_absE_c0"]) if key == "E" else float(a.abs().max())
        assert float((a.double() - b.double()).abs().max()) <= 4 * EPS32 * scale, key


def test_a_wrong_shaped_charges_in_a_call_changes_nothing():
    for dtype in DTYPES:
        case = "tric_c3_net"
        q, pos, cell, pairs, shifts = _system(case)
        step = _build(S._calc(STEP_CASES[case]), dtype, q, pos, cell, pairs, shifts)
        before, q_before, pos_before = S._bits(step), step.q.clone(), step.pos.clone()
        for bad in (q[:, :1], q[:, 0], q[:1], np.concatenate([q, q[:, :1]], axis=1)):
            with pytest.raises(ValueError, match=r"`charges` must be a tensor with shape \[n_atoms, n_channels\] = \[24, 3\]"):
                step(_t(pos @ STRAIN, dtype), _t(bad, dtype))
        assert torch.equal(step.q, q_before) and torch.equal(step.pos, pos_before) and _same(S._bits(step), before)
    batch = _batch("C1", F64)
    before, q_before, pos_before = B._bits(batch), batch.q.clone(), batch.pos.clone()
    systems = [B._system(n, False) for n in ALL]
    moved = [_t(s[1] @ STRAIN, F64) for s in systems]
    good = [_t(GOLD[f"f{n}_charges"], F64) for n in ALL]
    with pytest.raises(ValueError, match=r"\[344, 3\].*\[344, 1\]"):
        batch(positions=moved, charges=torch.cat(good)[:, :1])
    with pytest.raises(ValueError, match=r"frame 3.*\[24, 3\].*\[24, 1\]"):
        batch(positions=moved, charges=good[:3] + [good[3][:, :1]] + good[4:])
    assert torch.equal(batch.q, q_before) and torch.equal(batch.pos, pos_before)
    assert all(B._same(a, b) for a, b in zip(before, B._bits(batch)))
    # the two forms of `charges=`
    as_list = B._bits(batch, charges=[2 * g for g in good])
    flat = B._bits(batch, charges=2 * torch.cat(good))
    assert all(B._same(a, b) for a, b in zip(as_list, flat)) and not torch.equal(as_list[3][2], before[3][2])


def test_constructor_refusals_with_device_tensors():
    q, cell, pos, idx, sh = _frame(2, False, F64)
    calc = B._calc("C1")
    with pytest.raises(ValueError, match=r"`n_channels` must be an int in 1\.\.8.*got 9"):
        tpa.GraphedEwaldStep(calc, q, cell, pos, idx, sh, n_channels=9)
    with pytest.raises(ValueError, match=r"`n_channels` must be an int in 1\.\.8.*got 3\.0"):
        tpa.GraphedEwaldBatch(calc, [(q, cell, pos, idx, sh)], n_channels=3.0)
    with pytest.raises(ValueError, match=r"\[n_atoms, n_channels\] = \[n_atoms, 2\].*n_channels = 2.*\[17, 3\]"):
        tpa.GraphedEwaldStep(calc, q, cell, pos, idx, sh, n_channels=2)
    with pytest.raises(ValueError, match=r"frame 1: `charges`.*\[n_atoms, 3\].*\[17, 1\]"):
        tpa.GraphedEwaldBatch(calc, [(q, cell, pos, idx, sh), (q[:, :1], cell, pos, idx, sh)], n_channels=3)
    with pytest.raises(ValueError, match="single charge channel"):  # the keyword left out: the single-channel sentence
        tpa.GraphedEwaldStep(calc, q, cell, pos, idx, sh)
    with pytest.raises(ValueError, match="frame 0: a single charge channel"):
        tpa.GraphedEwaldBatch(calc, [(q, cell, pos, idx, sh)])
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        tpa.GraphedEwaldStep(calc, q.cpu(), cell.cpu(), pos.cpu(), idx.cpu(), sh.cpu(), n_channels=3)
