"""CPU tests (no GPU) of the graphed step of a combined potential: the C-ABI mirror of ``mipme_combined_step_args_t``, the exported
symbols, the refusals of the entry point (host pointers: it must return before any launch) and of ``GraphedCombinedStep``."""

import ctypes as C
import os
import re

import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, combined

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
IPL, COU = _lib.INVERSE_POWER_LAW, _lib.COULOMB


def make_rs(learnable=True):
    return tpa.CombinedPotential(
        [tpa.CoulombPotential(smearing=0.8), tpa.InversePowerLawPotential(exponent=6, smearing=1.1),
         tpa.InversePowerLawPotential(exponent=3, smearing=0.6)], initial_weights=torch.tensor([1.0, -0.3, 0.5], dtype=F64),
        learnable_weights=learnable, smearing=1.0)


def test_struct_mirrors_the_header_field_by_field():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mipme_combined_step_args \{(.*?)\} mipme_combined_step_args_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    assert names == [n for n, _ in _lib.CombinedStepArgs._fields_]
    assert names[:2] == ["size", "version"]
    # offsets: every field is 8 bytes wide except the int32 / uint32 ones, which come in pairs -- no padding anywhere
    offset = 0
    for d, name in zip(decls, names):
        width = 4 if re.match(r"(u?int32_t)\b", d) else 8
        assert getattr(_lib.CombinedStepArgs, name).offset == offset, name
        assert getattr(_lib.CombinedStepArgs, name).size == width, name
        offset += width
    assert C.sizeof(_lib.CombinedStepArgs) == offset == 264
    assert int(re.search(r"#define MIPME_COMBINED_STEP_VERSION (\d+)", hdr).group(1)) == _lib.COMBINED_STEP_VERSION == 1
    a = _lib.CombinedStepArgs(n_atoms=3)
    assert a.size == 264 and a.version == 1 and a.n_atoms == 3
    with pytest.raises(TypeError, match="unknown field"):
        _lib.CombinedStepArgs(no_such_field=1)
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    lib = _lib.load()
    for name in ("mipme_combined_step", "mipme_combined_step_work"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert lib.mipme_combined_step_work.restype is C.c_int64
    md = _lib.MeshDesc(scheme=_lib.P3M, order=3, nx=32, ny=32, nz=32, n_channels=1)
    few, many = (lib.mipme_combined_step_work(None, C.byref(md), n, 3) for n in (16, 4096))
    assert 0 < few < many  # (it grows with the atoms: a slot per atom and the partial sums of every row block)
    assert lib.mipme_combined_step_work(None, C.byref(md), 16, 0) == 0 == lib.mipme_combined_step_work(None, C.byref(md), 16, 9)
    assert lib.mipme_combined_step_work(None, None, 16, 3) == 0


def _desc(*terms):
    d = _lib.CombinedDesc(n_terms=len(terms))
    for t, (kind, p, sm) in enumerate(terms):
        d.terms[t] = _lib.PotentialDesc(kind=kind, exponent=p, smearing=sm, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)
    return d


def _unit_mesh(**kw):
    md = _lib.MeshDesc(scheme=_lib.P3M, order=3, nx=32, ny=32, nz=32, n_channels=1)
    for i in range(3):
        md.cell[4 * i] = md.inv_cell[4 * i] = 1.0
    md.volume = 1.0
    for k, v in kw.items():
        setattr(md, k, v)
    return md


def test_entry_point_refusals_without_gpu():
    """Every refusal of the header's list with host pointers: -1 and the message, before any launch (and before the plan is
    read: its pointer here is a host buffer)."""
    lib = _lib.load()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    ok_desc = _desc((COU, 1, 0.8), (IPL, 6, 1.1))
    md = _unit_mesh()

    def args(**over):
        f = dict(plan=p, stream=None, dtype=_lib.F64, full_list=0, mesh=C.pointer(md), comb=C.pointer(ok_desc), n_atoms=4,
                 positions=p, charges=p, cell=p, weights=p, G_terms=p, G=p, rho_mesh=p, hat_work=p, phi_mesh=p, dc=p, atom_bins=p,
                 records=p, rho_hat=p, row_ptr=p, entries=p, shift_format=2, potentials=p, pair_force=p, field=p, energy=p,
                 grad_positions=p, grad_seed=None, grad_weights=p, grad_charges=p, work=p, nan_flag=None)
        f.update(over)
        return _lib.CombinedStepArgs(**f)

    def refused(a, needle):
        assert lib.mipme_combined_step(None if a is None else C.byref(a)) == -1
        msg = lib.mipme_last_error()
        assert needle in msg, msg

    refused(None, b"NULL argument struct")
    bad = args()
    bad.version = 7
    refused(bad, b"version 7")
    refused(args(dtype=5), b"invalid dtype")
    refused(args(comb=None), b"combined descriptor is NULL")
    for n in (0, 9, -1):
        d = _desc((COU, 1, 1.0))
        d.n_terms = n
        refused(args(comb=C.pointer(d)), b"1 to 8")
    refused(args(comb=C.pointer(_desc((COU, 1, 1.0), (IPL, 7, 1.0)))), b"Unsupported exponent")
    refused(args(comb=C.pointer(_desc((COU, 1, -1.0), (IPL, 6, -1.0)))), b"direct potential")
    refused(args(comb=C.pointer(_desc((COU, 1, 1.0), (IPL, 6, -1.0)))), b"term 1 has no `smearing`")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    two = _unit_mesh(n_channels=2)
    refused(args(mesh=C.pointer(two)), b"one charge channel")
    odd = _unit_mesh(nx=24)
    refused(args(mesh=C.pointer(odd)), b"power-of-two nx")
    refused(args(mesh=None), b"mesh descriptor is NULL")
    refused(args(full_list=1), b"grad_charges = 2 V needs a half list")
    refused(args(rho_hat=None), b"grad_weights needs rho_hat")
    refused(args(n_atoms=0), b"n_atoms")
    for name in ("plan", "positions", "charges", "cell", "weights", "G_terms", "G", "rho_mesh", "hat_work", "phi_mesh", "dc",
                 "records", "row_ptr", "entries", "potentials", "pair_force", "field", "energy", "grad_positions", "work",
                 "atom_bins"):
        refused(args(**{name: None}), b"NULL required buffer")
    # the optional outputs may be NULL together with what only they need: the next refusal is then the plan's, which a host
    # test cannot pass -- so the list above is complete when a NULL plan is the only thing left to object to
    refused(args(plan=None, grad_weights=None, grad_charges=None, rho_hat=None, full_list=1), b"NULL required buffer")
    # a mesh too small for bricks needs no atom_bins: the refusal left is again the plan
    small = _unit_mesh(nx=16, ny=16, nz=16)
    refused(args(mesh=C.pointer(small), atom_bins=None, plan=None), b"NULL required buffer")


def test_python_refusals():
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    eye = torch.eye(3, dtype=F64) * 8
    idx = torch.zeros((1, 2), dtype=torch.long)
    step = lambda calc, q=None: tpa.GraphedCombinedStep(calc, z(2, 1) if q is None else q, eye, z(2, 3), idx, z(1, 3))  # noqa: E731
    pme = lambda pot, **kw: tpa.PMECalculator(pot, mesh_spacing=0.6, **kw)  # noqa: E731
    c = lambda **kw: tpa.CoulombPotential(**kw)  # noqa: E731
    assert "GraphedCombinedStep" in tpa.__all__
    # a single potential: the other class serves it
    with pytest.raises(TypeError, match="CoulombPotential.*GraphedEnergyForces"):
        step(pme(c(smearing=1.0)))
    # combinations the kernels do not serve, each with its reason
    r = torch.linspace(0.1, 5, 8, dtype=F64)
    spline = tpa.SplinePotential(r, 1 / r, reciprocal=True, smearing=1.0)
    unserved = [
        (tpa.CombinedPotential([c(smearing=1.0), spline], smearing=1.0), "member 1 is a SplinePotential"),
        (tpa.CombinedPotential([make_rs(), c(smearing=1.0)], smearing=1.0), "member 0 is itself a CombinedPotential"),
        (tpa.CombinedPotential([c(smearing=1.0, exclusion_radius=2.0)], smearing=1.0), "member 0 has an exclusion radius"),
        (tpa.CombinedPotential([c(smearing=1.0)] * 9, smearing=1.0), "9 members"),
    ]
    for pot, why in unserved:
        assert combined.plan(pot) is None
        with pytest.raises(TypeError, match=why):
            step(pme(pot))
    direct = tpa.CombinedPotential([c(), tpa.InversePowerLawPotential(exponent=6)])
    with pytest.raises(TypeError, match="direct potentials"):
        step(tpa.Calculator(direct))
    # calculators without a mesh
    with pytest.raises(TypeError, match="PMECalculator or a P3MCalculator.*EwaldCalculator"):
        step(tpa.EwaldCalculator(make_rs(), lr_wavelength=0.8))
    with pytest.raises(TypeError, match="PMECalculator or a P3MCalculator, got a Calculator"):
        step(tpa.Calculator(make_rs()))
    # two channels, CPU tensors
    for calc in (pme(make_rs()), tpa.P3MCalculator(make_rs(), mesh_spacing=0.6, interpolation_nodes=3)):
        with pytest.raises(ValueError, match=r"single charge channel.*\(2, 2\)"):
            step(calc, z(2, 2))
        with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
            step(calc)
    # the refusals of the existing classes stay as they are
    with pytest.raises(TypeError, match="CombinedPotential.*eagerly"):
        tpa.GraphedEnergyForces(pme(make_rs()), z(2, 1), eye, z(2, 3), idx, z(1, 3))
