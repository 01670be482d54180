"""``GraphedCombinedStep`` (``-m gpu``): energy, forces, dE/dweights and dE/dcharges of a combined potential from one graph replay
-- against the reference's autograd (``tests/golden/combined_step.npz``, written by ``tests/golden/make_combined_step_golden.py``),
against the single-member steps of ``GraphedEnergyForces`` (linearity), against the eager calculator on a seeded random system
that exercises the row kernel's edges, and the behaviour of the object: weights and positions followed without a new capture,
the refusal of a shift beyond the entry format (which leaves a step that is recaptured as it was), the deferred NaN flag.

Bounds.  float64: ``1e-10 * max|want|`` (the rule of ``tests/test_gpu_combined.py::_check_against_reference``).  float32: the
larger of (a) that rule's float32 bound -- 5 x the spread of the reference's own float32 run + 4 eps32 x scale; on the random
system, which has no reference run, the spread is taken as zero -- and (b) a bound measured at run time on code that is not under
test: for each member t alone, the error of the existing ``GraphedEnergyForces`` in float32 against its own float64 run, and
``2 x sum_t |w_t| err_t`` per quantity (2: the contracted table and the merged pair sum add in another order).  dE/dw_t is the
energy of member t alone, so its measured bound is ``2 x err_t`` of that member's energy, component by component.
Every comparison prints its error and bound before it asserts (``pytest -s``; one run is kept in
``profiles/combined_step_accuracy.txt``).
"""

import functools
import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYS = np.load(os.path.join(ROOT, "tests", "golden", "combined.npz"))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "combined_step.npz"))
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
EPS32 = float(np.finfo(np.float32).eps)
TAG = {F64: "f64", F32: "f32"}

# (kind, exponent, smearing) and weight of every member
RS = (((("c", 1, 0.8), ("p", 6, 1.1), ("p", 3, 0.6))), (1.0, -0.3, 0.5))
ONE = ((("c", 1, 0.9),), (0.8,))
EIGHT = ((("c", 1, 1.0), ("p", 2, 0.9), ("p", 3, 0.8), ("p", 4, 1.0), ("p", 5, 0.9), ("p", 6, 1.1), ("p", 1, 1.3), ("p", 6, 0.7)),
         (1.0, -0.4, 0.5, 0.3, -0.6, -0.3, 0.25, 0.7))


def _member(spec):
    kind, p, sm = spec
    return tpa.CoulombPotential(smearing=sm) if kind == "c" else tpa.InversePowerLawPotential(exponent=p, smearing=sm)


def _combination(members, weights, dtype=F64):
    pot = tpa.CombinedPotential([_member(m) for m in members], initial_weights=torch.tensor(weights, dtype=dtype), smearing=1.0)
    return pot.to(device=DEV, dtype=dtype)


def _calculator(pot, kind, full, spacing=0.6):
    if kind == "pme":
        return tpa.PMECalculator(pot, mesh_spacing=spacing, interpolation_nodes=4, full_neighbor_list=full)
    return tpa.P3MCalculator(pot, mesh_spacing=spacing, interpolation_nodes=3, full_neighbor_list=full)


# ---- systems -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_system(name, list_tag):
    return dict(q=SYS[f"{name}_charges"][:, :1].copy(), pos=SYS[f"{name}_positions"], cell=SYS[f"{name}_cell"],
                pairs=SYS[f"{name}_pairs_{list_tag}"], shifts=SYS[f"{name}_shifts_{list_tag}"].astype(np.float64), spacing=0.6)


@functools.lru_cache(maxsize=None)
def _random_system(list_tag):
    """37 atoms (the last wavefront of the row kernel holds one row, the last workgroup is mostly empty) in a triclinic cell; one
    atom sits two cells away from its image in the cell, so that its pairs carry shift components up to +-3; every pair of one
    other atom is deleted, so that its row is empty; rows run from 0 to more than 32 entries."""
    rng = np.random.default_rng(20261019)
    cell = np.array([[9.4, 0.0, 0.0], [1.1, 9.0, 0.0], [-0.8, 1.3, 9.7]])
    n = 37
    frac = []
    while len(frac) < n:  # half of the atoms in a denser region (long rows); no two closer than 0.9
        f = rng.uniform(0, 1, 3) if len(frac) < 20 else 0.3 + 0.45 * rng.uniform(0, 1, 3)
        dist = [np.linalg.norm(((f - g + 0.5) % 1.0 - 0.5) @ cell) for g in frac]
        if not dist or min(dist) > 0.9:
            frac.append(f)
    pos = np.array(frac) @ cell
    q = rng.normal(size=(n, 1))
    q -= q.mean()
    pairs, S, _ = tpa.neighbor_list(pos, cell, 5.2)
    pairs, S = np.asarray(pairs), np.asarray(S, dtype=np.float64)
    moved = int(pairs[np.argmax(S[:, 0] == 1), 0])  # the first atom of a pair across the cell's x boundary: +1 becomes +3
    lonely = 11 if moved != 11 else 12
    pos = pos.copy()
    pos[moved] += 2 * cell[0]  # r_j - r_i + S cell is unchanged with S +/- (2, 0, 0) for the pairs of this atom
    S[pairs[:, 0] == moved, 0] += 2
    S[pairs[:, 1] == moved, 0] -= 2
    keep = (pairs[:, 0] != lonely) & (pairs[:, 1] != lonely)
    pairs, S = pairs[keep], S[keep]
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    pairs, S = pairs[order], S[order]
    if list_tag == "full":
        pairs, S = np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([S, -S])
        order = np.argsort(pairs[:, 0], kind="stable")
        pairs, S = pairs[order], S[order]
    assert np.abs(S).max() == 3
    rows = np.bincount(pairs.ravel(), minlength=n) if list_tag == "half" else 2 * np.bincount(pairs[:, 0], minlength=n)
    assert rows[lonely] == 0 and rows.max() > 32, (rows.min(), rows.max())
    d = np.linalg.norm(pos[pairs[:, 1]] - pos[pairs[:, 0]] + S @ cell, axis=1)
    assert d.max() < 5.2 and d.min() > 0.9
    return dict(q=q, pos=pos, cell=cell, pairs=np.ascontiguousarray(pairs), shifts=np.ascontiguousarray(S), spacing=0.7)


def _tensors(s, dtype):
    t = lambda key: torch.tensor(s[key], dtype=dtype, device=DEV)  # noqa: E731
    return t("q"), t("cell"), t("pos"), torch.tensor(s["pairs"], device=DEV), t("shifts")


def _np(x):
    return x.detach().double().cpu().numpy().copy()


def _run_step(s, members, weights, kind, full, dtype, **kw):
    pot = _combination(members, weights, dtype)
    calc = _calculator(pot, kind, full, s["spacing"])
    step = tpa.GraphedCombinedStep(calc, *_tensors(s, dtype), charge_gradient=not full, **kw)
    out = step()
    torch.cuda.synchronize()
    calc.check()
    res = {"E": _np(out[0]), "F": _np(out[1]), "gw": _np(out[2])}
    if not full:
        res["gq"] = _np(out[3])
    return res, step, pot


# ---- code that is not under test: the single-member steps ------------------------------------------------------------------------
_SINGLE = {}


def _single_member(sys_key, s, spec, kind, full, dtype):
    """E, F (+ dE/dq and sum |q V| for a half list) of ``GraphedEnergyForces`` with one member alone; computed once per case."""
    key = (sys_key, spec, kind, full, dtype)
    if key not in _SINGLE:
        calc = _calculator(_member(spec).to(device=DEV, dtype=dtype), kind, full, s["spacing"])
        q = _tensors(s, dtype)[0]
        out = tpa.GraphedEnergyForces(calc, *_tensors(s, dtype), warmup=1, charge_gradient=not full)()
        torch.cuda.synchronize()
        res = {"E": _np(out[0]), "F": _np(out[1])}
        if not full:
            res["gq"] = _np(out[2])
            res["abs"] = float((_np(q) * res["gq"] / 2).__abs__().sum())
        _SINGLE[key] = res
    return _SINGLE[key]


def _measured_bounds(sys_key, s, members, weights, kind, full):
    """2 x sum_t |w_t| err_t per quantity, err_t = float32 against float64 of member t's own step; dE/dw: 2 x err_t of E."""
    errs = []
    for spec in members:
        r32, r64 = (_single_member(sys_key, s, spec, kind, full, dt) for dt in (F32, F64))
        errs.append({k: np.abs(r32[k] - r64[k]).max() for k in r64 if k != "abs"})
    out = {k: 2 * sum(abs(w) * e[k] for w, e in zip(weights, errs)) for k in errs[0]}
    out["gw"] = 2 * np.array([e["E"] for e in errs])
    return out


def _check(what, res, want, dtype, spread=None, measured=None):
    """``want[key]``: float64 values; ``spread[key]``: the reference's float32 error (None: no such run); ``measured``: bound (b)."""
    for key, w in want.items():
        scale = np.abs(w).max()
        err = np.abs(res[key] - w)
        if dtype == F64:
            tol = 1e-10 * scale
        else:
            tol = np.maximum(5 * (spread[key] if spread is not None else 0.0) + 4 * EPS32 * scale, measured[key])
        print(f"accuracy {what} {TAG[dtype]} {key}: max error {err.max():.3e}  bound {np.max(tol):.3e}  scale {scale:.3e}")
        assert (err <= tol).all(), f"{what} {key} {dtype}: error {err.max():.3e} > {np.min(tol):.3e} (scale {scale:.3e})"


# ---- against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("list_tag", ["half", "full"])
@pytest.mark.parametrize("kind", ["pme", "p3m"])
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_step_matches_the_reference(system, kind, list_tag, dtype):
    """E, F = -dE/dpositions, dE/dweights and (half lists) dE/dcharges of the golden cases."""
    s, full = _golden_system(system, list_tag), list_tag == "full"
    res, _, _ = _run_step(s, *RS, kind, full, dtype)
    prefix = f"{system}_{kind}_{list_tag}"
    keys = {"E": "E", "F": "gpos", "gw": "gw"} | ({} if full else {"gq": "gq"})
    sign = {"F": -1.0}
    want = {k: sign.get(k, 1.0) * GOLD[f"{prefix}_{g}_f64"] for k, g in keys.items()}
    spread = measured = None
    if dtype == F32:
        spread = {k: np.abs(sign.get(k, 1.0) * GOLD[f"{prefix}_{g}_f32"].astype(np.float64) - want[k]).max() for k, g in keys.items()}
        measured = _measured_bounds((system, list_tag), s, *RS, kind, full)
    _check(prefix, res, want, dtype, spread, measured)


# ---- linearity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pme", "p3m"])
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_linearity_against_single_member_steps(system, kind):
    """float64: E and F are sum_t w_t x (E, F of ``GraphedEnergyForces`` with member t alone) to 1e-12 of sum_t |w_t| max|.|_t (the
    bound of ``test_linearity_against_single_member_calculators``), and dE/dw_t is the energy of member t's step to 1e-12 of
    sum_a |q_a V_t,a| -- the sum of the magnitudes of the terms it is made of, as there."""
    s = _golden_system(system, "half")
    members, weights = RS
    res, _, _ = _run_step(s, members, weights, kind, False, F64)
    runs = [_single_member((system, "half"), s, spec, kind, False, F64) for spec in members]
    for key in ("E", "F", "gq"):
        want = sum(w * r[key] for w, r in zip(weights, runs))
        scale = sum(abs(w) * np.abs(r[key]).max() for w, r in zip(weights, runs))
        err = np.abs(res[key] - want).max()
        print(f"linearity {system} {kind} {key}: error {err:.3e}, scale {scale:.3e}, ratio {err / scale:.2e}")
        assert err <= 1e-12 * scale, (key, err, scale)
    for t, r in enumerate(runs):
        err = abs(res["gw"][t] - r["E"])
        print(f"linearity {system} {kind} gw[{t}]: error {err:.3e}, scale {r['abs']:.3e}")
        assert err <= 1e-12 * r["abs"], (t, res["gw"][t], r["E"])


# ---- against the eager calculator: the row kernel's edges -------------------------------------------------------------------------
def _eager(s, members, weights, kind, full):
    pot = _combination(members, weights, F64)
    calc = _calculator(pot, kind, full, s["spacing"])
    q, cell, pos, idx, S = _tensors(s, F64)
    q.requires_grad_(True)
    pos.requires_grad_(True)
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + S @ cell, dim=1)
    E = (calc(q, cell, pos, idx, d) * q).sum()
    gq, gpos, gw = torch.autograd.grad(E, (q, pos, pot.weights))
    out = {"E": _np(E), "F": -_np(gpos), "gw": _np(gw)}
    if not full:
        out["gq"] = _np(gq)
    return out


@functools.lru_cache(maxsize=None)
def _eager_cached(n_terms, list_tag):
    members, weights = ONE if n_terms == 1 else EIGHT
    return _eager(_random_system(list_tag), members, weights, "pme" if n_terms == 1 else "p3m", list_tag == "full")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("list_tag", ["half", "full"])
@pytest.mark.parametrize("n_terms", [1, 8])
def test_step_matches_the_eager_calculator_on_a_random_system(n_terms, list_tag, dtype):
    """N = 37, triclinic, rows of 0 to more than 32 entries, an empty row, shifts up to +-3; one term (Coulomb, PME) and eight
    (every exponent, two of them twice with another smearing; P3M).  Oracle: the eager calculator in float64 on the same list."""
    s, full = _random_system(list_tag), list_tag == "full"
    members, weights = ONE if n_terms == 1 else EIGHT
    kind = "pme" if n_terms == 1 else "p3m"
    res, step, _ = _run_step(s, members, weights, kind, full, dtype)
    assert step._bins is not None  # the brick route
    measured = _measured_bounds(("random", list_tag), s, members, weights, kind, full) if dtype == F32 else None
    _check(f"random_{n_terms}_{kind}_{list_tag}", res, _eager_cached(n_terms, list_tag), dtype, None, measured)


# ---- the object ----------------------------------------------------------------------------------------------------------------
def test_weights_are_followed_without_recapture():
    """E is linear in w: after one in-place SGD step with dE_dw, E_1 - E_0 = -lr |dE/dw|^2 (1e-10 relative, float64); the graph
    object is the same one."""
    s = _golden_system("tric", "half")
    pot = _combination(*RS)
    step = tpa.GraphedCombinedStep(_calculator(pot, "p3m", False), *_tensors(s, F64))
    graph, lr = step.graph, 0.05
    opt = torch.optim.SGD([pot.weights], lr=lr)
    E0, _, gw = step()
    E0, g = float(E0), gw.clone()
    pot.weights.grad = g.clone()
    opt.step()
    E1 = float(step()[0])
    want = -lr * float((g * g).sum())
    print(f"weights: E1 - E0 = {E1 - E0:.15e}, -lr |g|^2 = {want:.15e}")
    assert step.graph is graph
    assert abs((E1 - E0) - want) <= 1e-10 * abs(want)
    assert torch.equal(step._w, pot.weights.detach())


def test_positions_are_followed():
    """``step(p2)`` equals a freshly built step at ``p2`` bit for bit in float64; two replays at the same positions are
    bit-identical in float32 (no atomics in the new kernels).  The mesh part's spread does add with LDS atomics, but at both
    sets of positions used here (seeded; 3-point stencils on a 32^3 mesh, counted once on the host) no mesh point lies in the
    stencils of more than two atoms, and a sum of two addends does not depend on their order: energy and forces are held to the
    same bits as the pair sums."""
    s = _random_system("half")
    members, weights = EIGHT
    for dtype in (F64, F32):
        q, cell, pos, idx, S = _tensors(s, dtype)
        gen = torch.Generator(device="cpu").manual_seed(7)
        p2 = pos + 0.05 * torch.randn(pos.shape, generator=gen, dtype=dtype).to(DEV)
        calc = _calculator(_combination(members, weights, dtype), "p3m", False, s["spacing"])
        step = tpa.GraphedCombinedStep(calc, q, cell, pos, idx, S, charge_gradient=True)
        first = [x.clone() for x in step()]
        moved = [x.clone() for x in step(p2)]
        pair_force = step._pair_force.clone()
        assert not torch.equal(first[1], moved[1])
        again = [x.clone() for x in step()]
        assert torch.equal(pair_force, step._pair_force)
        for a, b in zip(moved, again):
            assert torch.equal(a, b)
        if dtype == F64:
            fresh = tpa.GraphedCombinedStep(calc, q, cell, p2, idx, S, charge_gradient=True)
            for a, b in zip(moved, fresh()):
                assert torch.equal(a, b)
            step.recapture(idx, S, positions=pos)
            for a, b in zip(first, step()):
                assert torch.equal(a, b)


def test_shift_out_of_range_and_nan_flag():
    s = _random_system("half")
    q, cell, pos, idx, S = _tensors(s, F64)
    calc = _calculator(_combination(*ONE), "pme", False, s["spacing"])
    bad = S.clone()
    bad[3, 1] = 4.0
    with pytest.raises(ValueError, match=r"integers in \[-3, 3\]"):
        tpa.GraphedCombinedStep(calc, q, cell, pos, idx, bad)
    step = tpa.GraphedCombinedStep(calc, q, cell, pos, idx, S)
    E = float(step()[0])
    nan_pos = pos.clone()
    nan_pos[2, 1] = float("nan")
    step(nan_pos)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=r"NaNs detected in the k-space filter result.*shape: \[1, 32, 32, 32\]"):
        step(pos)
    assert float(step(pos)[0]) == E  # the flag is cleared, the step serves on


def test_a_refused_recapture_leaves_the_step_as_it_was():
    """``recapture`` with a shift of 4 raises before anything of the object changes: ``pairs`` is still the list the replayed graph
    was captured for, and a further call returns the bits of the first (float64, the 37-atom system, one term)."""
    s = _random_system("half")
    q, cell, pos, idx, S = _tensors(s, F64)
    step = tpa.GraphedCombinedStep(_calculator(_combination(*ONE), "pme", False, s["spacing"]), q, cell, pos, idx, S)
    first = [x.clone() for x in step()]
    bad = S.clone()
    bad[3, 1] = 4.0
    with pytest.raises(ValueError, match=r"GraphedCombinedStep: the cell shifts must be integers in \[-3, 3\]"):
        step.recapture(idx.clone(), bad)
    assert step.pairs is idx
    for a, b in zip(first, step()):
        assert torch.equal(a, b)
