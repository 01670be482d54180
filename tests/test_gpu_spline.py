"""GPU tests of the spline potential: the three kernels of ``csrc/spline.hip`` point by point against the CPU form of the
splines, the autograd nodes, the filter tables, and every calculator with a ``SplinePotential`` against the reference's
values (``tests/golden/spline.npz``, written by ``tests/golden/make_spline_golden.py``)."""

import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, analytic, splines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "spline.npz"))
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
EPS32 = float(np.finfo(np.float32).eps)
KW = {
    "recip": dict(reciprocal=True, y_at_zero=math.sqrt(2 / math.pi), yhat_at_zero=0.0, smearing=1.0),
    "plain": dict(reciprocal=False, smearing=1.0),
    "direct": dict(reciprocal=True, y_at_zero=math.sqrt(2 / math.pi), yhat_at_zero=0.0, smearing=None, prefactor=2.5,
                   exclusion_radius=2.5, exclusion_degree=2),
}


def make_potential(name, dtype=F64, cls=tpa.SplinePotential, device=DEV):
    t = lambda key: torch.tensor(GOLD[f"{name}_{key}"], dtype=dtype)  # noqa: E731
    return cls(t("r"), t("y"), k_grid=t("k"), yhat_grid=t("yhat"), **KW[name]).to(device)


# ---- the kernels, point by point -------------------------------------------------------------------------------------------
def _knots(n, rng):
    """n knots on [0.5, 10.5] (jittered, so no two intervals are alike) of a smooth function."""
    x = 0.5 + 10.0 * (np.arange(n) + 0.3 * rng.uniform(size=n)) / n
    return x, np.sin(1.3 * x) * np.exp(-0.1 * x) + 0.2 * x


def _arguments(x, n_points, rng):
    """Below, inside and beyond the grid, exactly on knots (the first and the last among them)."""
    lo, hi = x[0], x[-1]
    pts = np.concatenate([[lo - 1.7, lo, hi, hi + 2.3, x[len(x) // 2]], rng.choice(x, 8), rng.uniform(lo - 0.5, hi + 0.5, n_points)])
    return rng.permutation(pts)[:n_points] if n_points >= 13 else pts[:n_points]


def _cpu_derivatives(fn, x, orders):
    """fn(x) and its derivatives by autograd of the CPU expression, float64."""
    xv = torch.tensor(x, dtype=F64, requires_grad=True)
    out = [fn(xv)]
    for _ in range(orders):
        out.append(torch.autograd.grad(out[-1].sum(), xv, create_graph=True)[0])
    return [o.detach().numpy() for o in out]


def _launch_eval(table, order, x):
    out = torch.empty_like(x)
    desc = _lib.SplineDesc()
    keep = table.fill(desc, x.device)  # noqa: F841
    _lib.check(_lib.load().mipme_spline_eval(_lib.current_stream(x.device), _lib.dtype_code(x.dtype), C.byref(desc), order,
                                             x.numel(), x.data_ptr(), out.data_ptr()))
    return out


def _tolerance(dtype, scale):
    """fp64: 1e-12 x scale; fp32: 4 eps32 x scale (the result is rounded once, to the argument's type).  ``scale`` is the
    largest magnitude of the quantity over the arguments of the test -- of the whole sweep, not of the one or five points of
    its smallest launches: a derivative near one of its zeros is still a difference of terms of the size it has elsewhere."""
    return (1e-12 if dtype == F64 else 4 * EPS32) * scale


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_knots", [2, 3, 96, 5000])
def test_spline_eval_orders_0_to_3(n_knots, dtype):
    """``mipme_spline_eval`` against autograd of the reference expression on the CPU; 5000 knots are beyond the LDS bound
    (``splines.LDS_KNOTS``), so the table is read from global memory."""
    assert 96 <= splines.LDS_KNOTS < 5000
    rng = np.random.default_rng(n_knots)
    x, y = _knots(n_knots, rng)
    spline = tpa.lib.CubicSpline(torch.tensor(x), torch.tensor(y))
    scales = None
    for n_points in (4099, 1, 5, 63, 64, 65):
        args = _arguments(x, n_points, rng)
        if dtype == F32:
            args = args.astype(np.float32).astype(np.float64)  # the arguments the kernel sees
        want = _cpu_derivatives(spline, args, 3)
        if scales is None:
            scales = [np.abs(w).max() for w in want]
        xd = torch.tensor(args, dtype=dtype, device=DEV)
        for order in range(4):
            got = _launch_eval(spline._table, order, xd)
            assert got.dtype == dtype
            err = np.abs(got.double().cpu().numpy() - want[order]).max()
            assert err <= _tolerance(dtype, scales[order]), (n_knots, n_points, order, err, scales[order])
    # exact interpolation at the knots (float64 arguments)
    if dtype == F64:
        got = _launch_eval(spline._table, 0, torch.tensor(x, device=DEV))
        assert np.abs(got.cpu().numpy() - y).max() <= 4e-16 * np.abs(y).max()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_knots", [2, 3, 96, 5000])
def test_spline_eval_reciprocal(n_knots, dtype):
    """The reciprocal-axis composite and its first derivative in one pass against the CPU composite and its autograd:
    arguments below the first knot (zero included), inside, beyond the last knot, on knots.

    Tolerance of the derivative.  fp32: 4 eps32 x max|dS/dx| over the sweep.  fp64: 1e-12 x max|dS/dx| plus the rounding that
    the yardstick and the kernel both carry: the derivative of a cubic in this form is a difference of two terms of size
    T = (|y_i| + |y_i+1|) / h_i, so either side is off by a few eps64 x T whatever the size of the result, and above the first
    knot the exact factor u^2 (u = 1/x up to 100 here) of ``-R'(u) u^2`` multiplies that rounding: 8 eps64 x T u^2 is allowed
    for the two of them (below the first knot 8 eps64 x T_Z).  Measured against 1e-12 x max|dS/dx| = 2.1e-13 alone: 2.8e-13
    at 96 knots and 1.4e-11 at 5000, both at the smallest x, where T u^2 = 9e4 (allowance 1.6e-10)."""
    rng = np.random.default_rng(100 + n_knots)
    x = np.logspace(-2, 2, n_knots) * (1 + 0.2 * rng.uniform(size=n_knots) / n_knots)
    y = np.array([math.erf(v / math.sqrt(2)) / v for v in x])
    spline = tpa.lib.CubicSplineReciprocal(torch.tensor(x), torch.tensor(y), y_at_zero=math.sqrt(2 / math.pi))
    scales = None
    for n_points in (4099, 1, 5, 63, 64, 65):
        pts = np.concatenate([[0.0, 0.3 * x[0], x[0], x[-1], 7.0 * x[-1]], rng.choice(x, 8),
                              np.exp(rng.uniform(np.log(0.2 * x[0]), np.log(3 * x[-1]), n_points))])
        args = rng.permutation(pts)[:n_points] if n_points >= 13 else pts[:n_points]
        if dtype == F32:
            args = args.astype(np.float32).astype(np.float64)
        want, dwant = _cpu_derivatives(spline, args, 1)
        below = args < x[0]
        u2 = np.where(below, 1.0, 1.0 / np.where(below, 1.0, args) ** 2)
        if scales is None:  # of the value and of the derivative, over the whole sweep
            scales = (np.abs(want).max(), np.abs(dwant).max())
        dtol = _tolerance(dtype, scales[1]) * np.ones_like(args)
        if dtype == F64:
            X, Y = spline._rev.x, spline._rev.y
            j = np.clip(np.searchsorted(X, 1.0 / np.where(below, 1.0, args), side="right") - 1, 0, len(X) - 2)
            T = np.where(below, (abs(spline._zero.y[0]) + abs(spline._zero.y[1])) / x[0],
                         (np.abs(Y[j]) + np.abs(Y[j + 1])) / (X[j + 1] - X[j]) * u2)
            dtol = dtol + 8 * np.finfo(np.float64).eps * T
        xd = torch.tensor(args, dtype=dtype, device=DEV)
        out, dout = torch.empty_like(xd), torch.empty_like(xd)
        desc = spline._descriptor(DEV)
        for d in (dout, None):
            _lib.check(_lib.load().mipme_spline_eval_reciprocal(_lib.current_stream(DEV), _lib.dtype_code(dtype), C.byref(desc),
                                                                xd.numel(), xd.data_ptr(), out.data_ptr(), _lib.ptr(d)))
            assert np.abs(out.double().cpu().numpy() - want).max() <= _tolerance(dtype, scales[0]), (n_knots, n_points)
        derr = np.abs(dout.double().cpu().numpy() - dwant)
        assert (derr <= dtol).all(), (n_knots, n_points, (derr / dtol).max())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_nan_argument_gives_nan(dtype):
    rng = np.random.default_rng(7)
    x, y = _knots(96, rng)
    spline = tpa.lib.CubicSpline(torch.tensor(x), torch.tensor(y))
    recip = tpa.lib.CubicSplineReciprocal(torch.tensor(x), torch.tensor(y))
    xd = torch.tensor([1.0, float("nan"), 3.0, float("nan")], dtype=dtype, device=DEV)
    for order in range(4):
        got = _launch_eval(spline._table, order, xd).cpu()
        assert torch.isnan(got).tolist() == [False, True, False, True], order
    xg = xd.clone().requires_grad_(True)
    out = recip(xg)
    (g,) = torch.autograd.grad(out.sum(), xg)
    assert torch.isnan(out).tolist() == [False, True, False, True] and torch.isnan(g).tolist() == [False, True, False, True]


def test_device_nodes_gradcheck():
    """The plain node and the reciprocal composite: first and second order by finite differences, arguments off the knots;
    orders above 3 of the plain node are zeros from the Python side."""
    rng = np.random.default_rng(11)
    x, y = _knots(17, rng)
    plain = tpa.lib.CubicSpline(torch.tensor(x), torch.tensor(y))
    mid = 0.5 * (x[1:] + x[:-1]) + 0.1 * (x[1] - x[0])
    pts = torch.tensor(np.concatenate([[x[0] - 0.4], mid[:-1], [x[-1] + 0.6]]), device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(plain, (pts,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradgradcheck(plain, (pts,), eps=1e-6, atol=1e-6, rtol=1e-5)
    v = plain(pts)
    for _ in range(4):
        (v,) = torch.autograd.grad(v.sum(), pts, create_graph=True)
    assert torch.equal(v, torch.zeros_like(pts))  # fourth derivative of a cubic
    xr = np.logspace(-1, 1, 15)
    recip = tpa.lib.CubicSplineReciprocal(torch.tensor(xr), torch.tensor(np.exp(-xr) / xr + 1 / (1 + xr)), y_at_zero=7.0)
    midr = np.sqrt(xr[1:] * xr[:-1]) * 1.01
    ptsr = torch.tensor(np.concatenate([[0.02, 0.07], midr, [14.0, 40.0]]), device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(recip, (ptsr,), eps=1e-7, atol=1e-6, rtol=1e-6)
    assert torch.autograd.gradgradcheck(recip, (ptsr,), eps=1e-7, atol=1e-5, rtol=1e-5)
    # the one-pass derivative and the composed one are the same function
    (g1,) = torch.autograd.grad(recip(ptsr).sum(), ptsr)
    (g2,) = torch.autograd.grad(recip(ptsr).sum(), ptsr, create_graph=True)
    assert (g1 - g2.detach()).abs().max() <= 1e-13 * g1.abs().max()


# ---- potential methods on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["recip", "plain", "direct"])
def test_methods_on_device_tensors(name, dtype):
    pot = make_potential(name)
    cast = lambda a: torch.tensor(a, dtype=dtype)  # noqa: E731
    d, k2 = cast(GOLD[f"{name}_dist"]), cast(GOLD[f"{name}_ksq"])
    cpu = make_potential(name, device="cpu")
    for method, arg in (("lr_from_dist", d), ("from_dist", d), ("lr_from_k_sq", k2)):
        got = getattr(pot, method)(arg.to(DEV))
        want = getattr(cpu, method)(arg.double()).numpy()
        assert got.dtype == dtype and got.device.type == "cuda"
        assert np.abs(got.double().cpu().numpy() - want).max() <= _tolerance(dtype, np.abs(want).max()), method
    assert pot.self_contribution().device.type == "cuda" and pot.background_correction().device.type == "cuda"
    np.testing.assert_allclose(pot.self_contribution().cpu().numpy().reshape(-1), GOLD[f"{name}_self_contribution"], rtol=1e-15)


# ---- filter tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["tric", "ortho"])
@pytest.mark.parametrize("name", ["recip", "plain"])
@pytest.mark.parametrize("scheme", ["pme", "p3m"])
def test_filter_table_kernel_matches_the_tensor_expression(scheme, name, system):
    pot = make_potential(name)
    calc = (tpa.PMECalculator(pot, mesh_spacing=0.6, interpolation_nodes=4) if scheme == "pme" else
            tpa.P3MCalculator(pot, mesh_spacing=0.6, interpolation_nodes=3))
    cell = torch.tensor(GOLD[f"{system}_cell"], device=DEV)
    geom = analytic._geometry(calc, cell)
    if system == "ortho":
        assert tuple(geom.ns) == (16, 32, 32)
    want = analytic.filter_table(calc.potential, geom.scheme, geom.order, cell, geom.ns, geom)
    got = splines.build_filter(geom, pot._splines()[1], pot._prefactor_float(), F64, DEV)
    assert got.shape == want.shape == (geom.ns[0], geom.ns[1], geom.ns[2] // 2 + 1)
    scale = want.abs().max()
    assert (got - want).abs().max() <= 1e-12 * scale
    assert abs(float(got[0, 0, 0]) - float(pot.lr_from_k_sq(torch.zeros(1, dtype=F64, device=DEV)))) <= 1e-12 * float(scale)  # k = 0
    # lib.KSpaceFilter / P3MKSpaceFilter with a spline kernel use the same kernel
    filt = (tpa.lib.KSpaceFilter(cell, geom.ns, pot) if scheme == "pme" else tpa.lib.P3MKSpaceFilter(cell, geom.ns, 3, pot))
    assert torch.equal(filt._kfilter, got)
    g32 = splines.build_filter(geom, pot._splines()[1], pot._prefactor_float(), F32, DEV)
    assert g32.dtype == F32 and (g32.double() - want).abs().max() <= 4 * EPS32 * scale


# ---- calculators against the reference -------------------------------------------------------------------------------------
def _evaluate(calc, dtype, system, list_tag, mask=None, second=False, cell_grad=True):
    t = lambda key, **kw: torch.tensor(GOLD[f"{system}_{key}"], dtype=dtype, device=DEV, **kw)  # noqa: E731
    q, pos = t("charges", requires_grad=True), t("positions", requires_grad=True)
    cell = t("cell", requires_grad=cell_grad)
    idx = torch.tensor(GOLD[f"{system}_pairs_{list_tag}"], device=DEV)
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + t(f"shifts_{list_tag}") @ cell, dim=1)
    d.retain_grad()
    kw = {} if mask is None else {"pair_mask": torch.tensor(mask, device=DEV)}
    V = calc(q, cell, pos, idx, d, **kw)
    assert V.dtype == dtype
    L = (V * t("g")).sum()
    if second:
        (gp,) = torch.autograd.grad(L, pos, create_graph=True)
        hq, hpos = torch.autograd.grad((gp * gp).sum(), (q, pos))
        return {"hq": hq.cpu().numpy(), "hpos": hpos.cpu().numpy()}
    L.backward()
    n = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
    # (a spline potential with its own zero short-range part: the pair sum is skipped, the distances are not used and have no
    # gradient -- the reference's 0 * d gives zeros)
    pot = calc.potential
    if pot.smearing is not None and pot._own_sr():
        assert d.grad is None
        gd = torch.zeros_like(d)
    else:  # everywhere else the distances must have a gradient
        assert d.grad is not None
        gd = d.grad
    return {"V": n(V), "gq": n(q.grad), "gpos": n(pos.grad), "gcell": n(cell.grad), "gd": n(gd)}


def _check_against_reference(res, prefix, dtype):
    """The rule of ``test_gpu_dipole._check_against_reference``."""
    for key in ("V", "gq", "gpos", "gcell", "gd"):
        want = GOLD[f"{prefix}_{key}_f64"]
        scale = np.abs(want).max()
        err = np.abs(res[key] - want).max()
        if dtype == F64:
            tol = 1e-10 * scale
        else:  # 5x the spread of the reference's own fp32 run, floored at a few fp32 ulps of the scale
            spread = np.abs(GOLD[f"{prefix}_{key}_f32"].astype(np.float64) - want).max()
            tol = 5 * spread + 4 * EPS32 * scale
        assert err <= tol, f"{prefix} {key} {dtype}: max error {err:.3e} > {tol:.3e} (scale {scale:.3e})"


def _calculator(pot, kind, full=False):
    if kind == "pme":
        return tpa.PMECalculator(pot, mesh_spacing=0.6, interpolation_nodes=4, full_neighbor_list=full)
    if kind == "p3m":
        return tpa.P3MCalculator(pot, mesh_spacing=0.6, interpolation_nodes=3, full_neighbor_list=full)
    if kind == "ewald":
        return tpa.EwaldCalculator(pot, lr_wavelength=0.8, full_neighbor_list=full)
    return tpa.Calculator(pot, full_neighbor_list=full)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["pme", "p3m", "ewald"])
@pytest.mark.parametrize("name", ["recip", "plain"])
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_range_separated_calculators_match_the_reference(system, name, kind, dtype):
    calc = _calculator(make_potential(name, dtype), kind)
    calc.double_backward = None  # whatever it says: a spline potential takes the primitives route
    res = _evaluate(calc, dtype, system, "half")
    _check_against_reference(res, f"{system}_{name}_{kind}", dtype)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["half", "full", "mask"])
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_direct_calculator_matches_the_reference(system, case, dtype):
    calc = _calculator(make_potential("direct", dtype), "direct", full=case == "full")
    mask = GOLD[f"{system}_mask_half"] if case == "mask" else None
    res = _evaluate(calc, dtype, system, "full" if case == "full" else "half", mask=mask)
    _check_against_reference(res, f"{system}_direct_{case}", dtype)


@pytest.mark.parametrize("name", ["recip", "plain"])
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_second_order_matches_the_reference(system, name):
    calc = _calculator(make_potential(name), "pme")
    res = _evaluate(calc, F64, system, "half", second=True)
    for key in ("hq", "hpos"):
        want = GOLD[f"{system}_{name}_pme_{key}_f64"]
        err = np.abs(res[key] - want).max()
        assert err <= 1e-9 * np.abs(want).max(), (key, err, np.abs(want).max())


# ---- the cached filter and the differentiable one --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pme", "p3m"])
def test_cached_filter_equals_the_differentiable_one_and_follows_the_cell(kind):
    calc = _calculator(make_potential("recip"), kind)
    t = lambda key: torch.tensor(GOLD[f"tric_{key}"], device=DEV)  # noqa: E731
    q, pos, cell = t("charges"), t("positions"), t("cell")
    idx = t("pairs_half")
    S = t("shifts_half").double()
    dist = lambda c: torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + S @ c, dim=1)  # noqa: E731
    V_cached = calc(q, cell, pos, idx, dist(cell))
    entry = calc.__dict__["_spline_G"]
    assert entry is not None and entry[0]() is cell
    assert calc(q, cell, pos, idx, dist(cell)) is not None and calc.__dict__["_spline_G"][3] is entry[3]  # a hit: the same table
    cell_g = cell.clone().requires_grad_(True)
    V_diff = calc(q, cell_g, pos, idx, dist(cell_g))
    assert V_diff.requires_grad and (V_cached - V_diff.detach()).abs().max() <= 1e-12 * V_cached.abs().max()
    with torch.no_grad():
        cell.mul_(1.02)  # in place: the version counter moves, the cached table must not be used
    V_scaled = calc(q, cell, pos * 1.02, idx, dist(cell))
    assert calc.__dict__["_spline_G"][3] is not entry[3]
    fresh = _calculator(make_potential("recip"), kind)
    V_fresh = fresh(q, cell.clone(), pos * 1.02, idx, dist(cell))
    # (the spread accumulates with atomics: equal to rounding, not bit for bit)
    assert (V_scaled - V_fresh).abs().max() <= 1e-12 * V_fresh.abs().max() and (V_scaled - V_cached).abs().max() > 1e-4


# ---- a subclass with a short-range part ------------------------------------------------------------------------------------
class _CoulombSplit(tpa.SplinePotential):
    """The "recip" table (erf(r / sqrt 2) / r) with Coulomb's short-range part erfc(r / sqrt 2) / r in tensor operations."""

    def sr_from_dist(self, dist, pair_mask=None):
        out = torch.erfc(dist / math.sqrt(2)) / dist
        return out if pair_mask is None else out * pair_mask


def test_subclass_with_short_range_part_reproduces_coulomb():
    """``P3MCalculator(CoulombPotential(smearing=1))`` from the spline of its long-range part plus the short-range part of a
    subclass, on the triclinic case.  The agreement is limited by the spline's interpolation error, measured on the CPU for
    this case: |spline - erf/r| <= 9.7e-7 over the pair distances (not used by a mesh calculator), and for the kernel on the
    32^3 mesh |G_spline - G| <= 0.459 (max |G| 12.3; the 96 knots at 2 pi / r_grid are coarse where exp(-k^2/2)/k^2 falls, and
    1/U^2 magnifies the difference at large k), which bounds the error of a potential by
    (1/V) sum_k mu_k |dG(k)| sum_j |q_j| = 0.871 / 0.782 for the two channels.  The bound is recomputed here from the two
    tables; the tolerance is 5 x it, and the short-range parts must agree to rounding."""
    spline_pot = make_potential("recip", cls=_CoulombSplit)
    coulomb = tpa.CoulombPotential(smearing=1.0).to(DEV)
    t = lambda key: torch.tensor(GOLD[f"tric_{key}"], device=DEV)  # noqa: E731
    q, pos, cell, idx = t("charges"), t("positions"), t("cell"), t("pairs_half")
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + t("shifts_half").double() @ cell, dim=1)
    kw = dict(mesh_spacing=0.6, interpolation_nodes=3)
    calc_s, calc_c = tpa.P3MCalculator(spline_pot, **kw), tpa.P3MCalculator(coulomb, **kw)
    V_s, V_c = calc_s(q, cell, pos, idx, d), calc_c(q, cell, pos, idx, d)
    geom = analytic._geometry(calc_s, cell)
    dG = (analytic.filter_table(calc_s.potential, geom.scheme, geom.order, cell, geom.ns, geom)
          - analytic.filter_table(calc_c.potential, geom.scheme, geom.order, cell, geom.ns, geom)).abs()
    mu = analytic._multiplicity(geom, F64, DEV)
    bound = (dG * mu).sum() / torch.abs(torch.det(cell)) * q.abs().sum(dim=0)
    np.testing.assert_allclose(bound.cpu().numpy(), [0.871, 0.782], rtol=2e-3)  # the measured values of the docstring
    # lr / 2 enters V: half the bound per potential
    err = (V_s - V_c).abs().max(dim=0).values
    print("subclass: |dV| per channel", err.cpu().numpy(), "bound / 2", (bound / 2).cpu().numpy())
    assert (err <= 5 * bound / 2).all()
    assert (spline_pot.sr_from_dist(d) - coulomb.sr_from_dist(d)).abs().max() <= 1e-14
    # and the pair sum is really there: without it the potentials differ by the short-range part
    V_lr_only = tpa.P3MCalculator(make_potential("recip"), **kw)(q, cell, pos, idx, d)
    assert (V_lr_only - V_s).abs().max() > 1e-3
    # the tight check: what the subclass adds to the long-range-only potential is the pair sum of Coulomb's short-range part,
    # 1/2 sum_j q_j erfc(d / sqrt 2) / d over both directions of the half list, to rounding (the two mesh parts are the same
    # computation; their spread accumulates with atomics, so equal to ~1e-15 of the potentials, not bit for bit)
    sr = (torch.erfc(d / math.sqrt(2)) / d).unsqueeze(-1)
    V_sr = torch.zeros_like(q).index_add_(0, idx[:, 0], q[idx[:, 1]] * sr).index_add_(0, idx[:, 1], q[idx[:, 0]] * sr) / 2
    scale = max(float(V_s.abs().max()), float(V_sr.abs().max()))
    assert ((V_s - V_lr_only) - V_sr).abs().max() <= 1e-12 * scale
