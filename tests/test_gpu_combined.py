"""GPU tests of the combined potential: the two kernels of ``csrc/combined.hip`` point by point (against mpmath, against
``mipme_kfilter_build``), the autograd nodes, and every calculator with a ``CombinedPotential`` against the reference's values
(``tests/golden/combined.npz``, written by ``tests/golden/make_combined_golden.py``) and against the weighted sum of
single-member calculators."""

import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, analytic, combined, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "combined.npz"))
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
EPS32 = float(np.finfo(np.float32).eps)
W_RS, W_DIRECT, W_FALLBACK = (1.0, -0.3, 0.5), (0.7, -1.2), (0.8, 0.4)


# ---- the pair kernel, point by point ----------------------------------------------------------------------------------------
SIGMA = 0.9
N_GRID = 4096
ORDERS = (0, 1, 2, 3)


def _grid(dtype):
    """4 096 distances log-spaced in [0.05 sigma, 8 sigma], as the kernel sees them (rounded to ``dtype``)."""
    d = np.logspace(math.log10(0.05 * SIGMA), math.log10(8.0 * SIGMA), N_GRID)
    return d.astype(np.float32).astype(np.float64) if dtype == F32 else d


def _R_monomials(p, n, x):
    """The monomials of R_n(x) as written in the issue: R_0 = 0, R_1 = 1, R_2 = 2x + p + 1, R_3 = 4x^2 + 2x(p+1) + (p+1)(p+2)."""
    return {0: [], 1: [1], 2: [2 * x, p + 1], 3: [4 * x * x, 2 * x * (p + 1), (p + 1) * (p + 2)]}[n]


@functools.lru_cache(maxsize=None)
def _truth(dtype):
    """{(mode, p, n): (value, scale)} over the grid for unit prefactor:
    v^(n) = (-1)^n d^-(p+n) [R_n A + (p)_n Q], scale = d^-(p+n) [sum |monomials of R_n| A + (p)_n Q]; mode 0: A = 0, Q = 1.
    Q(p/2, x) and A = 2 x^(p/2) e^-x / Gamma(p/2) come from mpmath at 30 digits -- Q(1/2, x) = erfc(sqrt x), Q(1, x) = e^-x,
    Q(a+1, x) = Q(a, x) + x^a e^-x / Gamma(a+1): sums of positive terms -- and are rounded to float64; the bracket and the power
    of d are then assembled in float64 from x and d as exact float64 inputs: every term is positive, so those half a dozen
    roundings cost 1e-15 of the value, a thousandth of the float64 tolerance."""
    import mpmath as mp

    mp.mp.dps = 30
    d = _grid(dtype)
    Q, A = np.empty((7, N_GRID)), np.empty((7, N_GRID))
    gam = {p: mp.gamma(mp.mpf(p) / 2) for p in range(1, 7)}  # Gamma(p/2)
    two_s2 = 2 * mp.mpf(SIGMA) ** 2
    x64 = np.empty(N_GRID)
    for i, di in enumerate(d):
        dm = mp.mpf(float(di))
        x = dm * dm / two_s2
        x64[i] = x
        e, sx = mp.exp(-x), mp.sqrt(x)
        xh = [mp.mpf(1)]  # x^(p/2)
        for p in range(1, 7):
            xh.append(xh[-1] * sx)
        q = {1: mp.erfc(sx), 2: e}
        for p in (3, 4, 5, 6):
            q[p] = q[p - 2] + xh[p - 2] * e / gam[p]  # x^a e^-x / Gamma(a + 1), a = (p - 2) / 2
        for p in range(1, 7):
            Q[p, i] = q[p]
            A[p, i] = 2 * xh[p] * e / gam[p]
    out = {}
    for p in range(1, 7):
        for n in ORDERS:
            mono = _R_monomials(p, n, x64)
            rf = math.prod(range(p, p + n))  # (p)_n
            invp = d ** -float(p + n)
            sgn = -1.0 if n & 1 else 1.0
            R, Rabs = sum(mono) if mono else 0.0, sum(np.abs(t) for t in mono) if mono else 0.0
            out[(1, p, n)] = (sgn * invp * (R * A[p] + rf * Q[p]), invp * (Rabs * A[p] + rf * Q[p]))
            out[(0, p, n)] = (sgn * invp * rf, invp * rf)
    return out


def _desc(terms, smeared):
    d = _lib.CombinedDesc(n_terms=len(terms))
    for t, (p, pref) in enumerate(terms):
        kind = _lib.COULOMB if p == 1 and t == 0 else _lib.INVERSE_POWER_LAW  # (both spellings of 1/r)
        d.terms[t] = _lib.PotentialDesc(kind=kind, exponent=p, smearing=SIGMA if smeared else -1.0, prefactor=pref,
                                        exclusion_radius=-1.0, exclusion_degree=1)
    return d


def _sr_eval(desc, order, d, weights=None):
    shape = (d.numel(),) if weights is not None else (desc.n_terms, d.numel())
    out = torch.full(shape, float("nan"), dtype=d.dtype, device=d.device)
    _lib.check(_lib.load().mipme_combined_sr_eval(_lib.current_stream(d.device), _lib.dtype_code(d.dtype), C.byref(desc), order,
                                                  None, d.numel(), d.data_ptr(), _lib.ptr(weights), out.data_ptr()))
    return out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1], ids=["direct", "smeared"])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6])
def test_sr_eval_against_mpmath(p, mode, dtype):
    """``mipme_combined_sr_eval``: orders 0..3, one term and three, the per-term and the weighted form, 4 096 distances and the
    sizes 1, 255, 257 and 600 001 (more than one pass of 2 048 blocks of 256: the grid-stride loop runs).  Error against the sum
    of magnitudes, tolerances 1e-12 (float64) and 3e-6 (float32): the project's pointwise ones."""
    tol = 1e-12 if dtype == F64 else 3e-6
    truth = _truth(dtype)
    grid = _grid(dtype)
    rng = np.random.default_rng(p)
    worst = 0.0
    for terms in ([(p, 1.0)], [(p, 1.0), (p % 6 + 1, -2.5), ((p + 2) % 6 + 1, 0.75)]):
        desc = _desc(terms, mode == 1)
        w = torch.tensor([0.7, -1.3, 2.1][:len(terms)], dtype=dtype, device=DEV)
        for size in (N_GRID, 1, 255, 257, 600001):
            idx = np.arange(size) % N_GRID if size >= N_GRID else rng.integers(0, N_GRID, size)
            d = torch.tensor(grid[idx], dtype=dtype, device=DEV)
            for order in ORDERS:
                got = _sr_eval(desc, order, d)
                assert got.shape == (len(terms), size) and got.dtype == dtype
                got_np = got.double().cpu().numpy()
                for t, (pt, pref) in enumerate(terms):
                    val, scale = truth[(mode, pt, order)]
                    err = np.abs(got_np[t] - pref * val[idx]) / (abs(pref) * scale[idx])
                    worst = max(worst, float(err.max()))
                    assert err.max() <= tol, (terms, size, order, t, float(err.max()), float(grid[idx][err.argmax()]))
                # the weighted form is the contraction of the per-term one, to rounding
                summed = _sr_eval(desc, order, d, w)
                assert summed.shape == (size,)
                mag = torch.einsum("t,tp->p", w.abs(), got.abs())
                ref = torch.einsum("t,tp->p", w.double(), got.double())
                assert ((summed.double() - ref).abs() <= 4 * torch.finfo(dtype).eps * mag.double()).all(), (terms, size, order)
    print(f"p={p} mode={mode} {dtype}: worst relative error {worst:.3e} (tolerance {tol:.0e})")


def test_closed_form_against_numerical_derivatives():
    """The yardstick of the test above -- the closed form with the R_n of the issue -- against mpmath's numerical
    derivatives of Q(p/2, d^2 / 2 sigma^2) / d^p at 40 digits."""
    import mpmath as mp

    mp.mp.dps = 40
    for p in range(1, 7):
        v = lambda r: mp.gammainc(mp.mpf(p) / 2, r * r / (2 * mp.mpf(SIGMA) ** 2), mp.inf, regularized=True) / r**p  # noqa: E731
        for n in ORDERS:
            for d in (0.07, 0.9, 5.0):
                dm = mp.mpf(d)
                x = dm * dm / (2 * mp.mpf(SIGMA) ** 2)
                A = 2 * x ** (mp.mpf(p) / 2) * mp.exp(-x) / mp.gamma(mp.mpf(p) / 2)
                Q = mp.gammainc(mp.mpf(p) / 2, x, mp.inf, regularized=True)
                closed = (-1) ** n * dm ** (-(p + n)) * (sum(_R_monomials(p, n, x)) * A + mp.rf(p, n) * Q)
                assert abs(closed - mp.diff(v, dm, n)) <= mp.mpf(10) ** -25 * abs(closed), (p, n, d)
    mp.mp.dps = 30


HIGH_ORDERS = (4, 5, 6)
N_HIGH = 8


def _R_coefficients(p, n):
    """Integer coefficients of R_n (of x^0 .. x^(n-1)) and (p)_n by the recurrence R_m+1 = (m + 2x) R_m - 2x R_m' + (p)_m."""
    cur, rising = [0] * 8, 1
    for m in range(n):
        cur = [(m - 2 * k) * cur[k] + (2 * cur[k - 1] if k else 0) + (rising if k == 0 else 0) for k in range(8)]
        rising *= p + m
    return cur[:n], rising


@functools.lru_cache(maxsize=None)
def _truth_high_orders():
    """{(p, n): (value, scale)} of the smeared pair function at orders 4..6 on 8 distances log-spaced in [0.05 sigma, 8 sigma]
    that float32 represents exactly: the value is mpmath's numerical derivative of Q(p/2, d^2 / 2 sigma^2) / d^p at 30 digits
    (no closed form of ours enters), the scale the sum of magnitudes d^-(p+n) [sum_k |c_k| x^k A + (p)_n Q]."""
    import mpmath as mp

    d = np.logspace(math.log10(0.05 * SIGMA), math.log10(8.0 * SIGMA), N_HIGH).astype(np.float32).astype(np.float64)
    out = {}
    with mp.workdps(30):
        s2 = 2 * mp.mpf(SIGMA) ** 2
        for p in range(1, 7):
            v = lambda r: mp.gammainc(mp.mpf(p) / 2, r * r / s2, mp.inf, regularized=True) / r**p  # noqa: E731
            for n in HIGH_ORDERS:
                coeffs, rf = _R_coefficients(p, n)
                val, scale = np.empty(N_HIGH), np.empty(N_HIGH)
                for i, di in enumerate(d):
                    dm = mp.mpf(float(di))
                    x = dm * dm / s2
                    A = 2 * x ** (mp.mpf(p) / 2) * mp.exp(-x) / mp.gamma(mp.mpf(p) / 2)
                    Q = mp.gammainc(mp.mpf(p) / 2, x, mp.inf, regularized=True)
                    val[i] = mp.diff(v, dm, n)
                    scale[i] = dm ** (-(p + n)) * (sum(abs(c) * x**k for k, c in enumerate(coeffs)) * A + rf * Q)
                out[(p, n)] = (val, scale)
    return d, out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_sr_eval_orders_four_to_six_against_mpmath(dtype):
    """Orders 4..6 of ``mipme_combined_sr_eval`` (what a fourth to sixth derivative through the node runs), p = 1..6: the
    smeared form against mpmath's numerical derivatives, the direct form against (-1)^n (p)_n / d^(p+n).  From order 4 on R_n has
    negative coefficients, so the error is measured against the sum of magnitudes; tolerances as for the orders 0..3."""
    tol = 1e-12 if dtype == F64 else 3e-6
    grid, truth = _truth_high_orders()
    d = torch.tensor(grid, dtype=dtype, device=DEV)
    worst = 0.0
    for p in range(1, 7):
        for n in HIGH_ORDERS:
            val, scale = truth[(p, n)]
            got = _sr_eval(_desc([(p, 1.0)], True), n, d)[0].double().cpu().numpy()
            err = float((np.abs(got - val) / scale).max())
            direct = _sr_eval(_desc([(p, 1.0)], False), n, d)[0].double().cpu().numpy()
            want = (-1.0) ** n * _R_coefficients(p, n)[1] * grid ** -float(p + n)
            err0 = float((np.abs(direct - want) / np.abs(want)).max())
            print(f"p={p} order {n} {dtype}: smeared {err:.3e}, direct {err0:.3e} (tolerance {tol:.0e})")
            worst = max(worst, err, err0)
    assert worst <= tol, worst


def test_nan_and_zero_distances():
    desc = _desc([(1, 1.0), (6, 1.0)], True)
    d = torch.tensor([1.0, float("nan"), 0.0, 2.0], dtype=F64, device=DEV)
    for order in (0, 1):
        got = _sr_eval(desc, order, d).cpu()
        assert torch.isnan(got[:, 1]).all() and torch.isfinite(got[:, [0, 2, 3]]).all()  # d = 0: floored at 1e-15, finite in float64
    assert _sr_eval(desc, 0, d[:0]).shape == (2, 0)


# ---- the autograd nodes ----------------------------------------------------------------------------------------------------
def _rs_members(sig=(0.8, 1.1, 0.6)):
    return [tpa.CoulombPotential(smearing=sig[0]), tpa.InversePowerLawPotential(exponent=6, smearing=sig[1]),
            tpa.InversePowerLawPotential(exponent=3, smearing=sig[2])]


def make(case, dtype=F64, learnable=True):
    w = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    if case == "rs":
        pot = tpa.CombinedPotential(_rs_members(), initial_weights=w(W_RS), learnable_weights=learnable, smearing=1.0)
    elif case == "direct":
        pot = tpa.CombinedPotential([tpa.CoulombPotential(), tpa.InversePowerLawPotential(exponent=6)],
                                    initial_weights=w(W_DIRECT), learnable_weights=learnable, exclusion_radius=2.5,
                                    exclusion_degree=2)
    else:
        t = lambda key: torch.tensor(GOLD[f"recip_{key}"], dtype=dtype)  # noqa: E731
        spline = tpa.SplinePotential(t("r"), t("y"), k_grid=t("k"), yhat_grid=t("yhat"), reciprocal=True,
                                     y_at_zero=math.sqrt(2 / math.pi), yhat_at_zero=0.0, smearing=1.0)
        pot = tpa.CombinedPotential([tpa.CoulombPotential(smearing=1.0), spline], initial_weights=w(W_FALLBACK),
                                    learnable_weights=learnable, smearing=1.0)
    return pot.to(device=DEV, dtype=dtype)


@pytest.mark.parametrize("case", ["rs", "direct"])
def test_nodes_gradcheck(case):
    pot = make(case)
    plan = combined.plan(pot)
    assert plan is not None
    d = torch.tensor(np.linspace(0.6, 3.7, 11), device=DEV, requires_grad=True)
    w = torch.tensor([0.9, -0.4, 0.6][:plan.n_terms], dtype=F64, device=DEV, requires_grad=True)
    terms = lambda x: combined._TermValues.apply(x, plan, 0)  # noqa: E731
    both = lambda x, ww: torch.einsum("t,tp->p", ww, combined._TermValues.apply(x, plan, 0))  # noqa: E731
    fixed = lambda x: combined._WeightedValues.apply(x, w.detach(), plan, 0)  # noqa: E731
    assert torch.autograd.gradcheck(terms, (d,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradgradcheck(terms, (d,), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(both, (d, w), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradgradcheck(both, (d, w), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(fixed, (d,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradgradcheck(fixed, (d,), eps=1e-6, atol=1e-6, rtol=1e-5)
    # pair_values picks the weighted node for constant weights and the einsum for learnable ones: the same numbers
    a = combined.pair_values(pot, plan, d)
    pot.weights.requires_grad_(False)
    b = combined.pair_values(pot, plan, d)
    assert (a - b).abs().max() <= 1e-14 * a.abs().max()
    want = pot.sr_from_dist(d) if case == "rs" else pot.from_dist(d)
    assert (a - want).abs().max() <= 1e-12 * want.abs().max()
    # the seventh derivative is refused by name
    x = terms(d)
    for _ in range(6):
        (x,) = torch.autograd.grad(x.sum(), d, create_graph=True)
    with pytest.raises(ValueError, match="MIPME_COMBINED_MAX_ORDER"):
        torch.autograd.grad(x.sum(), d)


# ---- filter tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("ns", [(8, 8, 8), (16, 8, 12)])
@pytest.mark.parametrize("scheme", ["pme", "p3m"])
def test_tables_equal_the_single_potential_filter(scheme, ns, dtype):
    """Every slice of ``mipme_combined_kfilter_build`` against ``mipme_kfilter_build`` for that term alone: the same bits (both
    kernels take |k|^2 and 1 / U^2 from ``kgrid_point`` of ``csrc/kgrid.h`` and the term's value from ``lr_kernel_dev``)."""
    pots = [tpa.CoulombPotential(smearing=0.8)] + [tpa.InversePowerLawPotential(exponent=p, smearing=0.5 + 0.1 * p, prefactor=1.0 + p)
                                                   for p in range(1, 7)]
    plan = combined.plan(tpa.CombinedPotential(pots, smearing=1.0))
    geom = ops.MeshGeometry(GOLD["tric_cell"], ns, _lib.LAGRANGE if scheme == "pme" else _lib.P3M, 4 if scheme == "pme" else 3)
    tables = combined.build_tables(geom, plan, dtype, DEV)
    assert tables.shape == (7, ns[0], ns[1], ns[2] // 2 + 1) and tables.dtype == dtype
    for t, m in enumerate(pots):
        single = ops.build_filter(geom, m._descriptor(), dtype, DEV)
        a, b = tables[t].cpu().numpy(), single.cpu().numpy()
        assert np.isfinite(a).all()
        assert np.array_equal(a, b), (t, np.abs(a - b).max())
    # lib.KSpaceFilter / P3MKSpaceFilter with a combined kernel: the same tables contracted with the weights
    pot = tpa.CombinedPotential(pots, initial_weights=torch.linspace(-1, 1, 7, dtype=dtype), smearing=1.0).to(DEV)
    cell = torch.tensor(GOLD["tric_cell"], dtype=dtype, device=DEV)
    filt = tpa.lib.KSpaceFilter(cell, ns, pot) if scheme == "pme" else tpa.lib.P3MKSpaceFilter(cell, ns, 3, pot)
    want = torch.tensordot(pot.weights.detach().to(dtype), tables, dims=1)
    assert filt._kfilter.shape == want.shape and (filt._kfilter - want).abs().max() <= 4 * torch.finfo(dtype).eps * want.abs().max()


@pytest.mark.parametrize("scheme", ["pme", "p3m"])
def test_filters_serve_a_combination_the_kernels_do_not(scheme):
    """``lib.KSpaceFilter`` / ``P3MKSpaceFilter`` with nine terms (no plan): the table is tabulated from the members' tensor
    ``lr_from_k_sq`` and equals the weighted sum of the single-member filters' tables.  Both sides evaluate the same closed
    forms in float64, so they agree to rounding: 1e-12 of the sum of the magnitudes."""
    members = [tpa.InversePowerLawPotential(exponent=p, smearing=0.7 + 0.05 * p) for p in range(1, 7)]
    members += [tpa.CoulombPotential(smearing=1.2), tpa.InversePowerLawPotential(exponent=6, smearing=0.9),
                tpa.InversePowerLawPotential(exponent=4, smearing=1.3)]
    w = torch.linspace(-1, 1, 9, dtype=F64)
    pot = tpa.CombinedPotential(members, initial_weights=w, smearing=1.0).to(DEV)
    assert combined.plan(pot) is None
    cell = torch.tensor(GOLD["tric_cell"], dtype=F64, device=DEV)
    ns = (16, 8, 12)
    make_filter = (lambda k: tpa.lib.KSpaceFilter(cell, ns, k)) if scheme == "pme" else (lambda k: tpa.lib.P3MKSpaceFilter(cell, ns, 3, k))
    got = make_filter(pot)._kfilter
    singles = [make_filter(m.to(DEV))._kfilter for m in members]
    want = sum(float(wt) * g for wt, g in zip(w, singles))
    scale = sum(abs(float(wt)) * g.abs() for wt, g in zip(w, singles))
    ratio = float(((got - want).abs() / scale.clamp(min=1e-300)).max())
    print(f"filter fallback {scheme}: worst error / sum of magnitudes {ratio:.2e}")
    assert got.shape == want.shape and ratio <= 1e-12


# ---- calculators against the reference -------------------------------------------------------------------------------------
def _calculator(pot, kind, full=False):
    if kind == "pme":
        return tpa.PMECalculator(pot, mesh_spacing=0.6, interpolation_nodes=4, full_neighbor_list=full)
    if kind == "p3m":
        return tpa.P3MCalculator(pot, mesh_spacing=0.6, interpolation_nodes=3, full_neighbor_list=full)
    if kind == "ewald":
        return tpa.EwaldCalculator(pot, lr_wavelength=0.8, full_neighbor_list=full)
    return tpa.Calculator(pot, full_neighbor_list=full)


def _evaluate(calc, dtype, system, list_tag, mask=None, second=False, cell_grad=True, params=()):
    """V and the gradients of L = <g, V> w.r.t. charges, positions, cell, distances and ``params`` (the weights)."""
    t = lambda key, **kw: torch.tensor(GOLD[f"{system}_{key}"], dtype=dtype, device=DEV, **kw)  # noqa: E731
    q, pos = t("charges", requires_grad=True), t("positions", requires_grad=True)
    cell = t("cell", requires_grad=cell_grad)
    idx = torch.tensor(GOLD[f"{system}_pairs_{list_tag}"], device=DEV)
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + t(f"shifts_{list_tag}") @ cell, dim=1)
    kw = {} if mask is None else {"pair_mask": torch.tensor(mask, device=DEV)}
    V = calc(q, cell, pos, idx, d, **kw)
    assert V.dtype == dtype
    L = (V * t("g")).sum()
    n = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
    params = tuple(params)
    if second:
        (gp,) = torch.autograd.grad(L, pos, create_graph=True)
        hq, hpos, *hw = torch.autograd.grad((gp * gp).sum(), (q, pos) + params)
        return {"hq": n(hq), "hpos": n(hpos), **({"hw": n(hw[0])} if hw else {})}
    wrt = (q, pos, d) + ((cell,) if cell_grad else ()) + params
    grads = list(torch.autograd.grad(L, wrt))
    res = {"V": n(V), "gq": n(grads[0]), "gpos": n(grads[1]), "gd": n(grads[2])}
    if cell_grad:
        res["gcell"] = n(grads[3])
    if params:
        res["gw"] = n(grads[-1])
    return res


def _check_against_reference(res, prefix, dtype, keys=("V", "gq", "gpos", "gcell", "gd", "gw")):
    """The rule of ``test_gpu_spline._check_against_reference``."""
    for key in keys:
        want = GOLD[f"{prefix}_{key}_f64"]
        scale = np.abs(want).max()
        err = np.abs(res[key] - want).max()
        if dtype == F64:
            tol = 1e-10 * scale
        else:  # 5x the spread of the reference's own fp32 run, floored at a few fp32 ulps of the scale
            spread = np.abs(GOLD[f"{prefix}_{key}_f32"].astype(np.float64) - want).max()
            tol = 5 * spread + 4 * EPS32 * scale
        assert err <= tol, f"{prefix} {key} {dtype}: max error {err:.3e} > {tol:.3e} (scale {scale:.3e})"


CASES = {  # golden case -> (potential, calculator, list, mask)
    "rs_pme": ("rs", "pme", "half", False), "rs_p3m": ("rs", "p3m", "half", False), "rs_ewald": ("rs", "ewald", "half", False),
    "rs_pme_full": ("rs", "pme", "full", False), "rs_pme_mask": ("rs", "pme", "half", True),
    "direct_half": ("direct", "direct", "half", False), "direct_full": ("direct", "direct", "full", False),
    "direct_mask": ("direct", "direct", "half", True), "fallback_pme": ("fallback", "pme", "half", False),
}


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_calculators_match_the_reference(system, case, dtype):
    """V and dL/d(charges, positions, cell, distances, weights) of every golden case.  With a cell gradient the mesh filter is
    the differentiable tensor expression; the same call with a constant cell takes the cached tables of
    ``mipme_combined_kfilter_build`` and must give the same V and remaining gradients."""
    pname, kind, list_tag, masked = CASES[case]
    pot = make(pname, dtype)
    assert (combined.plan(pot) is None) == (pname == "fallback")
    calc = _calculator(pot, kind, full=list_tag == "full")
    calc.double_backward = None  # whatever it says: a combined potential takes the primitives route
    mask = GOLD[f"{system}_mask_half"] if masked else None
    res = _evaluate(calc, dtype, system, list_tag, mask=mask, params=(pot.weights,))
    _check_against_reference(res, f"{system}_{case}", dtype)
    res = _evaluate(calc, dtype, system, list_tag, mask=mask, cell_grad=False, params=(pot.weights,))
    _check_against_reference(res, f"{system}_{case}", dtype, keys=("V", "gq", "gpos", "gd", "gw"))
    if kind in ("pme", "p3m") and pname != "fallback":
        assert calc.__dict__.get("_combined_G") is not None


@pytest.mark.parametrize("cell_grad", [True, False], ids=["cellgrad", "tables"])
@pytest.mark.parametrize("system", ["tric", "ortho"])
def test_second_order_matches_the_reference(system, cell_grad):
    pot = make("rs")
    res = _evaluate(_calculator(pot, "pme"), F64, system, "half", second=True, cell_grad=cell_grad, params=(pot.weights,))
    for key in ("hq", "hpos", "hw"):
        want = GOLD[f"{system}_rs_pme_{key}_f64"]
        err = np.abs(res[key] - want).max()
        assert err <= 1e-9 * np.abs(want).max(), (key, err, np.abs(want).max())


# ---- linearity: the combined call against single-member calculators ---------------------------------------------------------
def _single_member_runs(members, kind, system, cell_grad):
    runs = []
    for m in members:
        calc = _calculator(m.to(DEV), kind)
        calc.double_backward = "analytic"
        runs.append(_evaluate(calc, F64, system, "half", cell_grad=cell_grad))
    return runs


def _assert_linear(res, runs, weights, keys, tol=1e-12):
    for key in keys:
        want = sum(w * r[key] for w, r in zip(weights, runs))
        scale = sum(abs(w) * np.abs(r[key]).max() for w, r in zip(weights, runs))
        err = np.abs(res[key] - want).max()
        print(f"linearity {key}: error {err:.3e}, scale {scale:.3e}, ratio {err / scale:.2e}")
        assert err <= tol * scale, (key, err, scale)


@pytest.mark.parametrize("cell_grad", [True, False], ids=["cellgrad", "tables"])
@pytest.mark.parametrize("kind", ["pme", "p3m", "ewald", "direct"])
def test_linearity_against_single_member_calculators(kind, cell_grad):
    """combined = sum_t w_t x (the same calculator with member t alone, ``double_backward = "analytic"``) to 1e-12 of the sum of
    the magnitudes, float64; and the weight gradient is <g, V_t> of those runs."""
    if kind == "direct":
        members, weights = [tpa.CoulombPotential(), tpa.InversePowerLawPotential(exponent=6)], W_DIRECT
        pot = tpa.CombinedPotential(members, initial_weights=torch.tensor(weights, dtype=F64)).to(DEV)
    else:
        members, weights = _rs_members(), W_RS
        pot = make("rs")
    res = _evaluate(_calculator(pot, kind), F64, "tric", "half", cell_grad=cell_grad, params=(pot.weights,))
    runs = _single_member_runs(members, kind, "tric", cell_grad)
    _assert_linear(res, runs, weights, ("V", "gq", "gpos", "gd") + (("gcell",) if cell_grad else ()))
    g = GOLD["tric_g"]
    want = np.array([(g * r["V"]).sum() for r in runs])
    scale = np.array([np.abs(g * r["V"]).sum() for r in runs])
    assert (np.abs(res["gw"] - want) <= 1e-12 * scale).all(), (res["gw"], want)


# ---- the weights -----------------------------------------------------------------------------------------------------------
def _inputs(system="tric", dtype=F64):
    t = lambda key: torch.tensor(GOLD[f"{system}_{key}"], dtype=dtype, device=DEV)  # noqa: E731
    q, pos, cell = t("charges"), t("positions"), t("cell")
    idx = torch.tensor(GOLD[f"{system}_pairs_half"], device=DEV)
    d = torch.linalg.norm(pos[idx[:, 1]] - pos[idx[:, 0]] + t("shifts_half") @ cell, dim=1)
    return q, cell, pos, idx, d


@pytest.mark.parametrize("kind", ["pme", "direct"])
def test_an_optimizer_step_on_the_weights_changes_the_next_result(kind):
    """Nothing that is cached (the plan, the filter tables) depends on the weights."""
    pot = make("rs" if kind == "pme" else "direct")
    calc = _calculator(pot, kind)
    args = _inputs()
    g = torch.tensor(GOLD["tric_g"], device=DEV)
    opt = torch.optim.SGD(pot.parameters(), lr=0.05)
    V0 = calc(*args)
    assert V0.requires_grad  # through the weights alone
    (V0 * g).sum().backward()
    grad = pot.weights.grad.clone()
    tables = calc.__dict__.get("_combined_G")
    opt.step()  # in place
    V1 = calc(*args)
    if kind == "pme":
        assert calc.__dict__["_combined_G"][3] is tables[3]  # the same tables: a hit
    # V is linear in w: V1 - V0 = sum_t (w1 - w0)_t V_t, and <g, V1 - V0> = -lr |grad|^2
    change = float(((V1 - V0).detach() * g).sum())
    want = -0.05 * float((grad * grad).sum())
    assert abs(change - want) <= 1e-10 * abs(want) and abs(want) > 1e-6
    # fixed weights: a buffer, nothing to train, nothing recorded
    fixed = make("rs" if kind == "pme" else "direct", learnable=False)
    assert list(fixed.parameters()) == [] and "weights" in fixed.state_dict()
    with torch.no_grad():
        fixed.weights.copy_(pot.weights)
    Vf = _calculator(fixed, kind)(*args)
    assert not Vf.requires_grad and (Vf - V1.detach()).abs().max() <= 1e-12 * V1.abs().max()


def test_cached_tables_follow_the_cell():
    calc = _calculator(make("rs", learnable=False), "pme")
    q, cell, pos, idx, d = _inputs()
    calc(q, cell, pos, idx, d)
    entry = calc.__dict__["_combined_G"]
    assert entry[0]() is cell and entry[3].shape[0] == 3
    calc(q, cell, pos, idx, d)
    assert calc.__dict__["_combined_G"][3] is entry[3]
    with torch.no_grad():
        cell.mul_(1.02)  # in place: the version counter moves
    V_scaled = calc(q, cell, pos * 1.02, idx, d * 1.02)
    assert calc.__dict__["_combined_G"][3] is not entry[3]
    V_fresh = _calculator(make("rs", learnable=False), "pme")(q, cell.clone(), pos * 1.02, idx, d * 1.02)
    assert (V_scaled - V_fresh).abs().max() <= 1e-12 * V_fresh.abs().max()


# ---- combinations the kernels do not serve ---------------------------------------------------------------------------------
def test_nine_terms_take_the_tensor_route_and_stay_linear():
    members = [tpa.InversePowerLawPotential(exponent=p, smearing=0.7 + 0.05 * p) for p in range(1, 7)]
    members += [tpa.CoulombPotential(smearing=1.2), tpa.InversePowerLawPotential(exponent=6, smearing=0.9),
                tpa.InversePowerLawPotential(exponent=4, smearing=1.3)]
    weights = [0.5, -0.2, 0.3, 0.1, -0.4, 0.25, 1.0, -0.15, 0.35]
    pot = tpa.CombinedPotential(members, initial_weights=torch.tensor(weights, dtype=F64), smearing=1.0).to(DEV)
    assert combined.plan(pot) is None
    calc = _calculator(pot, "pme")
    res = _evaluate(calc, F64, "tric", "half", params=(pot.weights,))
    assert calc.__dict__.get("_combined_G") is None
    runs = _single_member_runs(members, "pme", "tric", True)
    _assert_linear(res, runs, weights, ("V", "gq", "gpos", "gcell", "gd"))
    g = GOLD["tric_g"]
    want = np.array([(g * r["V"]).sum() for r in runs])
    scale = np.array([np.abs(g * r["V"]).sum() for r in runs])
    print("linearity gw: ratios", np.abs(res["gw"] - want) / scale)
    assert (np.abs(res["gw"] - want) <= 1e-12 * scale).all()
