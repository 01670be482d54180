"""CPU tests (no GPU) of the spline potential's host side: construction (second derivatives, Fourier transform, cosine
integral), the CPU form of the splines and of ``SplinePotential``'s methods against the reference's values
(``tests/golden/spline.npz``, written by ``tests/golden/make_spline_golden.py``), the C-ABI mirror, and the entry points
that refuse a spline potential."""

import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, splines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "spline.npz"))
POTS = ("recip", "plain", "direct")
KW = {
    "recip": dict(reciprocal=True, y_at_zero=float(np.sqrt(2 / np.pi)), yhat_at_zero=0.0, smearing=1.0),
    "plain": dict(reciprocal=False, smearing=1.0),
    "direct": dict(reciprocal=True, y_at_zero=float(np.sqrt(2 / np.pi)), yhat_at_zero=0.0, smearing=None, prefactor=2.5,
                   exclusion_radius=2.5, exclusion_degree=2),
}


def make_potential(name, dtype=torch.float64, yhat=True):
    t = lambda key: torch.tensor(GOLD[f"{name}_{key}"], dtype=dtype)  # noqa: E731
    return tpa.SplinePotential(t("r"), t("y"), k_grid=t("k"), yhat_grid=t("yhat") if yhat else None, **KW[name])


def _close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= rel * scale, f"{what}: max error {err:.3e} > {rel:.0e} x scale {scale:.3e}"


@pytest.mark.parametrize("name", POTS)
def test_second_derivatives_match_the_reference(name):
    r, y = torch.tensor(GOLD[f"{name}_r"]), torch.tensor(GOLD[f"{name}_y"])
    d2 = tpa.lib.compute_second_derivatives(r, y)
    assert d2.dtype == r.dtype and d2.shape == r.shape
    _close(d2, GOLD[f"{name}_d2y"], "d2y")
    k2, yhat = torch.tensor(GOLD[f"{name}_k"]) ** 2, torch.tensor(GOLD[f"{name}_yhat"])
    _close(tpa.lib.compute_second_derivatives(k2, yhat), GOLD[f"{name}_khat_d2y"], "d2y of the kernel spline")
    assert float(d2[0]) == 0.0 and float(d2[-1]) == 0.0  # natural
    two = tpa.lib.compute_second_derivatives(torch.tensor([1.0, 2.0]), torch.tensor([3.0, 5.0]))
    assert two.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("name", POTS)
def test_methods_on_cpu_tensors_match_the_reference(name):
    pot = make_potential(name)
    d, k2 = torch.tensor(GOLD[f"{name}_dist"]), torch.tensor(GOLD[f"{name}_ksq"])
    assert (k2 == 0).any() and (d < GOLD[f"{name}_r"][0]).any() and (d > GOLD[f"{name}_r"][-1]).any()
    _close(pot.lr_from_dist(d), GOLD[f"{name}_lr_from_dist"], "lr_from_dist")
    _close(pot.from_dist(d), GOLD[f"{name}_from_dist"], "from_dist")
    _close(pot.lr_from_k_sq(k2), GOLD[f"{name}_lr_from_k_sq"], "lr_from_k_sq")
    _close(pot.kernel_from_k_sq(k2), GOLD[f"{name}_lr_from_k_sq"], "kernel_from_k_sq")
    _close(pot.self_contribution().reshape(-1), GOLD[f"{name}_self_contribution"], "self_contribution")
    assert float(pot.background_correction().sum()) == 0.0
    assert torch.equal(pot.sr_from_dist(d), torch.zeros_like(d))
    assert torch.equal(pot.lr_from_dist(d, torch.ones_like(d, dtype=torch.bool)), pot.lr_from_dist(d))  # mask accepted
    # the prefactor enters from_dist twice, as in the reference
    pref = float(pot.prefactor)
    _close(pot.from_dist(d), pref * pref * pot._splines()[0](d), "prefactor twice", rel=1e-15)
    # the result has the dtype of the argument, whatever the tables are
    assert pot.lr_from_dist(d.float()).dtype == torch.float32 and pot.lr_from_k_sq(k2.float()).dtype == torch.float32


def test_splines_interpolate_their_knots_and_extrapolate_the_end_cubics():
    r, y = torch.tensor(GOLD["plain_r"]), torch.tensor(GOLD["plain_y"])
    s = tpa.lib.CubicSpline(r, y)
    assert torch.equal(s(r), y)
    _close(s.d2y_points, GOLD["plain_d2y"], "d2y_points")
    # beyond the last knot: the last cubic, continued (its value from the polynomial written out)
    h = float(r[-1] - r[-2])
    x = float(r[-1]) + 0.37
    a, b = (float(r[-1]) - x) / h, (x - float(r[-2])) / h
    want = a * float(y[-2]) + b * float(y[-1]) + ((a**3 - a) * float(s.d2y_points[-2]) + (b**3 - b) * float(s.d2y_points[-1])) * h * h / 6
    assert abs(float(s(torch.tensor([x]))) - want) <= 1e-14 * max(1.0, abs(want))
    rr, yr = torch.tensor(GOLD["recip_r"]), torch.tensor(GOLD["recip_y"])
    sr = tpa.lib.CubicSplineReciprocal(rr, yr, y_at_zero=0.25)
    _close(sr(rr), yr, "reciprocal spline at its knots", rel=4e-16)
    assert float(sr(torch.zeros(1, dtype=torch.float64))) == 0.25
    assert float(tpa.lib.CubicSplineReciprocal(rr, yr)(torch.zeros(1, dtype=torch.float64))) == float(yr[0])
    assert abs(float(sr(torch.tensor([1e9], dtype=torch.float64)))) < 1e-6  # -> 0 at infinity
    # differentiable by autograd on the CPU
    x = torch.tensor(GOLD["recip_dist"], requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: sr(v), (x,), eps=1e-7, atol=1e-6)


def test_spline_fourier_transform_against_the_integral():
    """``compute_spline_ft`` against the integral itself (mpmath, 30 digits; the golden script): per k value the error may be
    at most the larger of twice the reference's own and 1e-12 x scale.  Measured (k = 0, 0.01, 0.1, 1, 5, 20; scale 1.26e5):
    this package 2.8e-14, 5.8e-11, 0, 8.9e-16, 3.6e-16, 1.6e-17; the reference 2.8e-14, 3.5e-7, 2.6e-11, 0, 1.7e-16, 3.3e-17
    -- its k^-6 Horner form loses seven digits at k dr = 0.005, the quadrature used here for k dr < 2 does not."""
    t = lambda key: torch.tensor(GOLD[key])  # noqa: E731
    got = tpa.lib.compute_spline_ft(t("ft_k"), t("ft_r"), t("ft_y"), t("ft_d2y")).numpy()
    truth, ref_err = GOLD["ft_truth"], GOLD["ft_reference_error"]
    assert (GOLD["ft_k"] == 0).any()
    err = np.abs(got - truth)
    tol = np.maximum(2 * ref_err, 1e-12 * np.abs(truth).max())
    print("compute_spline_ft error", err, "reference", ref_err, "tolerance", tol)
    assert (err <= tol).all(), (err, tol)
    assert np.abs(GOLD["ft_reference"] - truth).max() == ref_err.max()


@pytest.mark.parametrize("name", ("recip", "plain"))
def test_default_kernel_grid_is_the_transform_of_the_spline(name):
    """Without ``yhat_grid`` the kernel is ``compute_spline_ft`` on the default ``k_grid``: the reference's values (its closed
    form, scipy's Ci) to 1e-9 of the scale -- the two differ by the reference's rounding at small k dr, see above."""
    pot = make_potential(name, yhat=False)
    _close(pot.yhat_grid, GOLD[f"{name}_yhat"], "yhat_grid", rel=1e-9)
    r = torch.tensor(GOLD[f"{name}_r"])
    auto = tpa.SplinePotential(r, torch.tensor(GOLD[f"{name}_y"]), **KW[name])
    want = 2 * np.pi / GOLD["recip_r"][::-1] if name == "recip" else GOLD["plain_r"]
    _close(auto.k_grid, want, "default k_grid", rel=1e-15)


def test_cosine_integral():
    """Ci in float64 at 31 arguments from 1e-3 to 1e3 (both branches, the switch at 3 included) against mpmath: a few ulps of
    the largest term of the sum, |ln x| + gamma <= 7.5."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 30
    x = np.concatenate([np.logspace(-3, 3, 29), [3.0, np.nextafter(3.0, 4.0)]])
    want = np.array([float(mp.ci(mp.mpf(float(v)))) for v in x])
    err = np.abs(splines.cosine_integral(x) - want)
    assert err.max() <= 4 * np.finfo(np.float64).eps * 7.5, err.max()


def test_constructor_errors():
    r = torch.linspace(0.1, 5, 10)
    with pytest.raises(ValueError, match="Length of radial grid and value array mismatch."):
        tpa.SplinePotential(r, torch.zeros(9))
    with pytest.raises(ValueError, match="Positive-valued radial grid is needed for reciprocal axis spline."):
        tpa.SplinePotential(torch.linspace(0, 5, 10), torch.zeros(10), reciprocal=True)


@pytest.mark.parametrize("name", POTS)
def test_state_dict_pickle_and_deepcopy(name):
    pot = make_potential(name)
    d, k2 = torch.tensor(GOLD[f"{name}_dist"]), torch.tensor(GOLD[f"{name}_ksq"])
    keys = {"r_grid", "y_grid", "k_grid", "yhat_grid", "prefactor"} | ({"smearing"} if KW[name]["smearing"] else set())
    assert set(pot.state_dict()) == keys
    for other in (pickle.loads(pickle.dumps(pot)), copy.deepcopy(pot)):
        assert torch.equal(other.lr_from_dist(d), pot.lr_from_dist(d)) and torch.equal(other.lr_from_k_sq(k2), pot.lr_from_k_sq(k2))
        assert torch.equal(other.self_contribution(), pot.self_contribution())
    # a state dict carries the tables over: a potential built on other values evaluates the loaded ones
    r = torch.tensor(GOLD[f"{name}_r"])
    blank = tpa.SplinePotential(r, torch.ones_like(r), k_grid=torch.tensor(GOLD[f"{name}_k"]),
                                yhat_grid=torch.ones(len(GOLD[f"{name}_k"]), dtype=torch.float64), **KW[name])
    assert not torch.equal(blank.lr_from_dist(d), pot.lr_from_dist(d))
    blank.load_state_dict(pot.state_dict())
    assert torch.equal(blank.lr_from_dist(d), pot.lr_from_dist(d)) and torch.equal(blank.lr_from_k_sq(k2), pot.lr_from_k_sq(k2))
    # ... also when the potential is moved or converted after the load (the tables are rebuilt before the buffers move)
    for move in (lambda p: p.to("cpu"), lambda p: p.double(), lambda p: p.to(torch.float32)):
        moved = tpa.SplinePotential(r, torch.ones_like(r), k_grid=torch.tensor(GOLD[f"{name}_k"]),
                                    yhat_grid=torch.ones(len(GOLD[f"{name}_k"]), dtype=torch.float64), **KW[name])
        moved.load_state_dict(pot.state_dict())
        moved = move(moved)
        assert torch.equal(moved.lr_from_dist(d), pot.lr_from_dist(d)) and torch.equal(moved.lr_from_k_sq(k2), pot.lr_from_k_sq(k2))
        # (after .to(float32) the prefactor buffer itself is single precision)
        _close(moved.self_contribution(), pot.self_contribution(), "self_contribution", rel=1e-7)
    # .to(dtype) converts the buffers; the float64 tables stay, results follow the argument
    half = copy.deepcopy(pot).to(torch.float32)
    assert half.r_grid.dtype == torch.float32
    assert torch.equal(half.lr_from_dist(d), pot.lr_from_dist(d))
    calc = pickle.loads(pickle.dumps(tpa.Calculator(pot) if name == "direct" else tpa.PMECalculator(pot, mesh_spacing=0.6)))
    assert torch.equal(calc.potential.lr_from_dist(d), pot.lr_from_dist(d))


def test_struct_mirrors_the_header_and_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mipme_spline_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"const double*": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double}
    want = []
    for decl in (x.strip() for x in body.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(const double\*|int32_t|double)\s+(\w+)(?:\[(\d+)\])?", decl)
        assert m, decl
        t = ctype[m.group(1)]
        want.append((m.group(2), t * int(m.group(3)) if m.group(3) else t))
    got = list(_lib.SplineDesc._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", None) == getattr(b, "_length_", None), name
    assert C.sizeof(_lib.SplineDesc) == 3 * 8 + 2 * 4 + 9 * 8 + 8
    assert _lib.SplineDesc.zero_x.offset == 32 and _lib.SplineDesc.prefactor.offset == 104
    lib = _lib.load()
    for name in ("mipme_spline_eval", "mipme_spline_eval_reciprocal", "mipme_spline_kfilter_build"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # the existing structs keep their layout
    assert C.sizeof(_lib.PotentialDesc) == 40 and C.sizeof(_lib.MeshDesc) == 176 and C.sizeof(_lib.DipoleDesc) == 32


def test_abi_argument_errors_without_gpu():
    """Refusals of the three entry points that come before any launch."""
    lib = _lib.load()
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    sd = _lib.SplineDesc(x=a, y=a, d2y=a, n=1)
    assert lib.mipme_spline_eval(None, _lib.F64, C.byref(sd), 0, 4, a, a) == -1
    assert b"at least 2 knots" in lib.mipme_last_error()
    sd.n = 4
    assert lib.mipme_spline_eval(None, _lib.F64, C.byref(sd), 4, 4, a, a) == -1
    assert b"outside 0..3" in lib.mipme_last_error()
    assert lib.mipme_spline_eval(None, _lib.F64, None, 0, 4, a, a) == -1
    assert lib.mipme_spline_eval(None, _lib.F64, C.byref(sd), 0, 0, None, None) == 0  # nothing to do
    assert lib.mipme_spline_eval_reciprocal(None, _lib.F64, C.byref(sd), 4, a, a, None) == -1
    assert b"not a reciprocal-axis spline" in lib.mipme_last_error()
    md = _lib.MeshDesc(scheme=_lib.P3M, order=9, nx=4, ny=4, nz=4, n_channels=1)
    assert lib.mipme_spline_kfilter_build(None, _lib.F64, C.byref(md), C.byref(sd), a) == -1
    assert b"from 1 to 5" in lib.mipme_last_error()
    md = _lib.MeshDesc(scheme=_lib.LAGRANGE, order=4, nx=0, ny=4, nz=4, n_channels=1)
    assert lib.mipme_spline_kfilter_build(None, _lib.F64, C.byref(md), C.byref(sd), a) == -1


def test_entry_points_that_cannot_serve_a_spline_say_so():
    pot = make_potential("recip")
    calcs = [tpa.PMECalculator(pot, mesh_spacing=0.6), tpa.P3MCalculator(pot, mesh_spacing=0.6, interpolation_nodes=3),
             tpa.EwaldCalculator(pot, lr_wavelength=0.8), tpa.Calculator(make_potential("direct"))]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    idx = torch.zeros((1, 2), dtype=torch.long)
    for calc in calcs:
        assert calc._spec_str is None and calc._spec() is None
        with pytest.raises(TypeError, match="SplinePotential.*eagerly"):
            calc.scriptable()
        with pytest.raises(TypeError, match="SplinePotential.*eagerly"):
            tpa.GraphedEnergyForces(calc, z(2, 1), torch.eye(3, dtype=torch.float64), z(2, 3), idx, z(1, 3))
        with pytest.raises(TypeError, match="SplinePotential.*eagerly"):
            tpa.GraphedEnergyForces(calc, z(2, 1), torch.eye(3, dtype=torch.float64), z(2, 3), neighbors=3.0)
        with pytest.raises(TypeError, match="SplinePotential.*eagerly"):
            tpa.GraphedFrameBatch(calc, [(z(2, 1), torch.eye(3, dtype=torch.float64), z(2, 3), idx, z(1, 3))])
        with pytest.raises(TypeError, match="SplinePotential.*eagerly"):
            calc.potential._descriptor()
        # the eager call is the supported one: on CPU tensors it stops where every calculator does
        with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
            calc(z(2, 1), torch.eye(3, dtype=torch.float64), z(2, 3), idx, z(1))
    # the handles of a NeighborStream are refused by name (a stand-in carrying the marker the calculators look for)
    handle = torch.zeros((1, 2), dtype=torch.long)
    handle._mipme_stream = object()
    with pytest.raises(TypeError, match="NeighborStream.*SplinePotential.*eagerly"):
        calcs[0](z(2, 1), torch.eye(3, dtype=torch.float64), z(2, 3), handle, z(1))

    # other potentials without a descriptor keep their error
    class Custom(tpa.Potential):
        pass

    with pytest.raises(TypeError, match="Custom has no HIP kernel"):
        Custom(smearing=1.0)._descriptor()
    # a subclass of SplinePotential is one
    class Sub(tpa.SplinePotential):
        def sr_from_dist(self, dist, pair_mask=None):
            return torch.exp(-dist)

    sub = Sub(torch.tensor(GOLD["recip_r"]), torch.tensor(GOLD["recip_y"]), reciprocal=True, smearing=1.0)
    assert not sub._own_sr() and pot._own_sr()
    assert tpa.PMECalculator(sub, mesh_spacing=0.6)._spec_str is None
    d = torch.tensor(GOLD["recip_dist"])
    _close(sub.from_dist(d), sub.lr_from_dist(d) + torch.exp(-d), "from_dist of a subclass", rel=1e-15)
