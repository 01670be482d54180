"""CPU tests (no GPU) of the combined potential's host side: the constructor's errors, state dicts (the reference's among
them), the tensor methods against the reference's values (``tests/golden/combined.npz``, written by
``tests/golden/make_combined_golden.py``), the R_n coefficients the library forms, the C-ABI mirror and its refusals, and the
entry points that refuse a combined potential."""

import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, combined

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "combined.npz"))
F64 = torch.float64


def make_rs(dtype=F64, learnable=True):
    return tpa.CombinedPotential(
        [tpa.CoulombPotential(smearing=0.8), tpa.InversePowerLawPotential(exponent=6, smearing=1.1),
         tpa.InversePowerLawPotential(exponent=3, smearing=0.6)], initial_weights=torch.tensor([1.0, -0.3, 0.5], dtype=dtype),
        learnable_weights=learnable, smearing=1.0)


def make_direct(dtype=F64):
    return tpa.CombinedPotential([tpa.CoulombPotential(), tpa.InversePowerLawPotential(exponent=6)],
                                 initial_weights=torch.tensor([0.7, -1.2], dtype=dtype), exclusion_radius=2.5, exclusion_degree=2)


def _close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= rel * scale, f"{what}: max error {err:.3e} > {rel:.0e} x scale {scale:.3e}"


def test_constructor_errors_are_the_references():
    rs, direct = tpa.CoulombPotential(smearing=1.0), tpa.CoulombPotential()
    with pytest.raises(ValueError, match=re.escape(
            "Cannot combine direct (`smearing=None`) and range-separated (`smearing=float`) potentials.")):
        tpa.CombinedPotential([rs, direct], smearing=1.0)
    with pytest.raises(ValueError, match=re.escape(
            "You should specify a `smearing` when combining range-separated (`smearing=float`) potentials.")):
        tpa.CombinedPotential([rs, tpa.InversePowerLawPotential(exponent=6, smearing=1.0)])
    with pytest.raises(ValueError, match=re.escape(
            "Cannot specify `smearing` when combining direct (`smearing=None`) potentials.")):
        tpa.CombinedPotential([direct, tpa.InversePowerLawPotential(exponent=6)], smearing=1.0)
    with pytest.raises(ValueError, match=re.escape(
            "The number of initial weights must match the number of potentials being combined")):
        tpa.CombinedPotential([rs, rs], initial_weights=torch.ones(3), smearing=1.0)
    assert "CombinedPotential" in tpa.__all__


def test_weights_are_a_parameter_or_a_buffer():
    pot = make_rs()
    assert isinstance(pot.potentials, torch.nn.ModuleList) and len(pot.potentials) == 3
    assert isinstance(pot.weights, torch.nn.Parameter) and [n for n, _ in pot.named_parameters()] == ["weights"]
    fixed = make_rs(learnable=False)
    assert list(fixed.parameters()) == [] and "weights" in dict(fixed.named_buffers())
    default = tpa.CombinedPotential([tpa.CoulombPotential(), tpa.InversePowerLawPotential(exponent=6)])
    assert isinstance(default.weights, torch.nn.Parameter) and default.weights.tolist() == [1.0, 1.0]
    assert default.smearing is None and default.exclusion_radius is None


def test_state_dict_round_trip_and_the_references_state_dict():
    pot = make_rs()
    keys = [str(k) for k in GOLD["sd_keys"]]
    assert sorted(pot.state_dict().keys()) == sorted(keys)
    assert {"weights", "potentials.0.smearing", "potentials.1.exponent", "smearing", "prefactor"} <= set(keys)
    # the reference's state dict, stored as plain arrays, loads strictly into ours
    ref_sd = {k: torch.tensor(GOLD[f"sd_{i}"]) for i, k in enumerate(keys)}
    other = tpa.CombinedPotential(
        [tpa.CoulombPotential(smearing=2.0), tpa.InversePowerLawPotential(exponent=6, smearing=2.0),
         tpa.InversePowerLawPotential(exponent=3, smearing=2.0)], initial_weights=torch.zeros(3, dtype=F64), smearing=3.0)
    res = other.load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    d = torch.tensor(GOLD["m_dist"])
    _close(other.sr_from_dist(d).detach(), GOLD["m_rs_sr_from_dist"], "sr_from_dist after loading the reference's state dict")
    # ... and the kernels' descriptor follows the loaded buffers
    assert [t[1] for t in combined.plan(other).key] == [0.8, 1.1, 0.6]
    # ours loads back, survives pickling and deep copies
    for clone in (copy.deepcopy(pot), pickle.loads(pickle.dumps(pot))):
        _close(clone.sr_from_dist(d).detach(), GOLD["m_rs_sr_from_dist"], "copy")
    again = make_rs()
    with torch.no_grad():
        again.weights.zero_()
    again.load_state_dict(pot.state_dict())
    assert torch.equal(again.weights, pot.weights)


def test_methods_on_cpu_tensors_match_the_reference():
    rs, direct = make_rs(), make_direct()
    d, k2 = torch.tensor(GOLD["m_dist"]), torch.tensor(GOLD["m_ksq"])
    with torch.no_grad():
        for method in ("from_dist", "sr_from_dist", "lr_from_dist"):
            # (sr = v - lr is a difference: held to 1e-12 of the larger of the two)
            want = GOLD[f"m_rs_{method}"]
            got = getattr(rs, method)(d).numpy()
            scale = np.abs(GOLD["m_rs_from_dist"]) + np.abs(want)
            assert (np.abs(got - want) <= 1e-12 * scale).all(), method
        _close(rs.lr_from_k_sq(k2), GOLD["m_rs_lr_from_k_sq"], "lr_from_k_sq")
        _close(rs.self_contribution().reshape(-1), GOLD["m_rs_self"], "self_contribution", rel=1e-14)
        _close(rs.background_correction().reshape(-1), GOLD["m_rs_background"], "background_correction", rel=1e-14)
        want = GOLD["m_direct_from_dist"]
        assert (np.abs(direct.from_dist(d).numpy() - want) <= 1e-13 * np.abs(want)).all()
        # a pair mask reaches every member
        mask = torch.arange(40) % 3 != 0
        assert torch.equal(rs.from_dist(d, mask), rs.from_dist(d) * mask)
    # pbc_correction is the base class's zero, also with a Coulomb member and a slab geometry
    q = torch.ones(4, 2, dtype=F64)
    out = rs.pbc_correction(torch.tensor([True, True, False]), torch.rand(4, 3, dtype=F64), torch.eye(3, dtype=F64) * 5, q)
    assert out.shape == q.shape and float(out.abs().max()) == 0.0
    # the weights are cast to the dtype of the argument (the reference requires them to match)
    out32 = rs.sr_from_dist(d.float())
    assert out32.dtype == torch.float32 and rs.weights.dtype == F64
    # gradients reach the weights
    (gw,) = torch.autograd.grad(rs.lr_from_dist(d).sum(), rs.weights)
    want = torch.stack([m.lr_from_dist(d).sum() for m in rs.potentials])
    _close(gw, want, "d/dw of lr_from_dist", rel=1e-14)


def test_R_n_coefficients_from_the_host_recurrence():
    """R_1 = 1, R_2 = 2x + p + 1, R_3 = 4x^2 + 2x(p+1) + (p+1)(p+2); R_0 = 0; zeros above the degree."""
    pots = [tpa.InversePowerLawPotential(exponent=p, smearing=1.0) for p in range(1, 7)]
    plan = combined.plan(tpa.CombinedPotential(pots, smearing=1.0))
    assert plan is not None and plan.n_terms == 6
    want = {0: lambda p: [0, 0, 0], 1: lambda p: [1, 0, 0], 2: lambda p: [p + 1, 2, 0],
            3: lambda p: [(p + 1) * (p + 2), 2 * (p + 1), 4]}
    for order, poly in want.items():
        rows = combined.coefficients(plan, order)
        for p, row in zip(range(1, 7), rows):
            assert len(row) == combined.MAX_ORDER == 6
            assert row == [float(c) for c in poly(p)] + [0.0, 0.0, 0.0], (order, p, row)
    # the highest order has degree 5 with leading coefficient 2^5
    for row in combined.coefficients(plan, 6):
        assert row[5] == 32.0
    with pytest.raises(ValueError, match="MIPME_COMBINED_MAX_ORDER"):
        combined.coefficients(plan, 7)


def test_plan_serves_exactly_the_documented_combinations():
    c = lambda **kw: tpa.CoulombPotential(**kw)  # noqa: E731
    assert combined.plan(make_rs()) is not None and combined.plan(make_direct()) is not None
    assert combined.plan(c(smearing=1.0)) is None  # not a combination
    assert combined.plan(tpa.CombinedPotential([c(smearing=1.0, exclusion_radius=2.0)], smearing=1.0)) is None
    assert combined.plan(tpa.CombinedPotential([make_rs(), c(smearing=1.0)], smearing=1.0)) is None  # nested
    assert combined.plan(tpa.CombinedPotential([c(smearing=1.0)] * 9, smearing=1.0)) is None
    assert combined.plan(tpa.CombinedPotential([c(smearing=1.0)] * 8, smearing=1.0)).n_terms == 8

    class Sub(tpa.CoulombPotential):
        pass

    assert combined.plan(tpa.CombinedPotential([Sub(smearing=1.0)], smearing=1.0)) is None
    # the plan is cached per parameter set and follows a member's buffers
    pot = make_rs()
    first = combined.plan(pot)
    assert combined.plan(pot) is first
    with torch.no_grad():
        pot.potentials[1].smearing.fill_(1.3)
    second = combined.plan(pot)
    assert second is not first and second.desc.terms[1].smearing == 1.3 and second.desc.terms[1].exponent == 6
    # a step on the weights changes nothing in it
    with torch.no_grad():
        pot.weights.add_(0.1)
    assert combined.plan(pot) is second


def test_struct_mirrors_the_header_and_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mipme_combined_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.fullmatch(r"(int32_t|mipme_potential_t)\s+(\w+)(?:\[(\d+)\])?", x.strip()).groups()
              for x in body.split(";") if x.strip()]
    assert fields == [("int32_t", "n_terms", None), ("int32_t", "reserved", None), ("mipme_potential_t", "terms", "8")]
    assert [n for n, _ in _lib.CombinedDesc._fields_] == ["n_terms", "reserved", "terms"]
    assert _lib.CombinedDesc.terms.offset == 8 and C.sizeof(_lib.CombinedDesc) == 8 + 8 * C.sizeof(_lib.PotentialDesc) == 328
    assert int(re.search(r"#define MIPME_COMBINED_MAX_TERMS (\d+)", hdr).group(1)) == _lib.COMBINED_MAX_TERMS == 8
    assert int(re.search(r"#define MIPME_COMBINED_MAX_ORDER (\d+)", hdr).group(1)) == _lib.COMBINED_MAX_ORDER == 6
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408
    lib = _lib.load()
    for name in ("mipme_combined_sr_eval", "mipme_combined_kfilter_build"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert C.sizeof(_lib.PotentialDesc) == 40 and C.sizeof(_lib.MeshDesc) == 176  # the existing structs keep their layout


def _desc(*terms):
    d = _lib.CombinedDesc(n_terms=len(terms))
    for t, (kind, p, sm) in enumerate(terms):
        d.terms[t] = _lib.PotentialDesc(kind=kind, exponent=p, smearing=sm, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)
    return d


def test_abi_refusals_without_gpu():
    """Both entry points: NULL descriptor, n_terms outside 1..8, exponent outside 1..6, a range-separated term with
    smearing <= 0 -- all before any launch."""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    md = _lib.MeshDesc(scheme=_lib.LAGRANGE, order=4, nx=4, ny=4, nz=4, n_channels=1)
    IPL, COU = _lib.INVERSE_POWER_LAW, _lib.COULOMB

    def both(desc, needle):
        ref = None if desc is None else C.byref(desc)
        assert lib.mipme_combined_sr_eval(None, _lib.F64, ref, 0, None, 4, a, None, a) == -1
        msg = lib.mipme_last_error()
        assert needle in msg and b"mipme_combined_sr_eval" in msg, msg
        assert lib.mipme_combined_kfilter_build(None, _lib.F64, C.byref(md), ref, a) == -1
        msg = lib.mipme_last_error()
        assert needle in msg and b"mipme_combined_kfilter_build" in msg, msg

    both(None, b"NULL")
    for n in (0, 9, -1):
        d = _desc((COU, 1, 1.0))
        d.n_terms = n
        both(d, b"1 to 8")
    for p in (0, 7):
        both(_desc((COU, 1, 1.0), (IPL, p, 1.0)), b"Unsupported exponent")
    for sm in (0.0, -1.0):
        both(_desc((COU, 1, 1.0), (IPL, 6, sm)), b"must be positive")
    # a direct combination is fine for the pair function and has no filter table; a smeared term among direct ones is refused
    direct = _desc((COU, 1, -1.0), (IPL, 6, -1.0))
    assert lib.mipme_combined_sr_eval(None, _lib.F64, C.byref(direct), 2, None, 0, None, None, None) == 0
    assert lib.mipme_combined_kfilter_build(None, _lib.F64, C.byref(md), C.byref(direct), a) == -1
    assert b"must be positive" in lib.mipme_last_error()
    assert lib.mipme_combined_sr_eval(None, _lib.F64, C.byref(_desc((COU, 1, -1.0), (IPL, 6, 1.0))), 0, None, 0, None, None, None) == -1
    assert b"direct" in lib.mipme_last_error()
    ok = _desc((COU, 1, 1.0), (IPL, 6, 1.0))
    assert lib.mipme_combined_sr_eval(None, _lib.F64, C.byref(ok), 7, None, 0, None, None, None) == -1
    assert b"MIPME_COMBINED_MAX_ORDER" in lib.mipme_last_error()
    assert lib.mipme_combined_sr_eval(None, _lib.F64, C.byref(ok), 0, None, 4, None, None, None) == -1  # NULL arrays
    assert lib.mipme_combined_sr_eval(None, 7, C.byref(ok), 0, None, 4, a, None, a) == -1
    assert b"dtype" in lib.mipme_last_error()
    bad_mesh = _lib.MeshDesc(scheme=_lib.P3M, order=9, nx=4, ny=4, nz=4, n_channels=1)
    assert lib.mipme_combined_kfilter_build(None, _lib.F64, C.byref(bad_mesh), C.byref(ok), a) == -1
    assert b"from 1 to 5" in lib.mipme_last_error()


def test_entry_points_that_cannot_serve_a_combination_say_so():
    rs = make_rs()
    calcs = [tpa.PMECalculator(rs, mesh_spacing=0.6), tpa.P3MCalculator(rs, mesh_spacing=0.6, interpolation_nodes=3),
             tpa.EwaldCalculator(rs, lr_wavelength=0.8), tpa.Calculator(make_direct())]
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    eye = torch.eye(3, dtype=F64)
    idx = torch.zeros((1, 2), dtype=torch.long)
    for calc in calcs:
        assert calc._spec_str is None and calc._spec() is None
        with pytest.raises(TypeError, match="CombinedPotential.*eagerly"):
            calc.scriptable()
        with pytest.raises(TypeError, match="CombinedPotential.*eagerly"):
            tpa.GraphedEnergyForces(calc, z(2, 1), eye, z(2, 3), idx, z(1, 3))
        with pytest.raises(TypeError, match="CombinedPotential.*eagerly"):
            tpa.GraphedEnergyForces(calc, z(2, 1), eye, z(2, 3), neighbors=3.0)
        with pytest.raises(TypeError, match="CombinedPotential.*eagerly"):
            tpa.GraphedFrameBatch(calc, [(z(2, 1), eye, z(2, 3), idx, z(1, 3))])
        with pytest.raises(TypeError, match="CombinedPotential.*eagerly"):
            calc.potential._descriptor()
        with pytest.raises(NotImplementedError, match="CombinedPotential.*torch.vmap.*eagerly"):
            torch.vmap(calc)(z(2, 2, 1), eye.expand(2, 3, 3), z(2, 2, 3), idx.expand(2, 1, 2), z(2, 1))
        # whatever double_backward says, the eager call is the supported one: on CPU tensors it stops where every calculator does
        for mode in (None, "analytic"):
            calc.double_backward = mode
            with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
                calc(z(2, 1), eye, z(2, 3), idx, z(1))
    handle = torch.zeros((1, 2), dtype=torch.long)
    handle._mipme_stream = object()
    with pytest.raises(TypeError, match="NeighborStream.*CombinedPotential.*eagerly"):
        calcs[0](z(2, 1), eye, z(2, 3), handle, z(1))
    # a spline potential keeps its own messages
    with pytest.raises(TypeError, match="SplinePotential.*eagerly"):
        r = torch.linspace(0.1, 5, 8, dtype=F64)
        tpa.PMECalculator(tpa.SplinePotential(r, 1 / r, reciprocal=True, smearing=1.0), mesh_spacing=0.6).scriptable()
