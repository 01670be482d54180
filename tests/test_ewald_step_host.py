"""CPU tests (no GPU) of the graphed Ewald step: the C-ABI mirror of ``mipme_ewald_step_args_t``, the exported symbols, the size
of the scratch, the refusals of the entry point (host pointers: it must return before any launch) and of ``GraphedEwaldStep``,
and the host side of the k-grid comparison."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ewald_step.npz"))
F64 = torch.float64


def test_class_is_exported():
    assert hasattr(tpa, "GraphedEwaldStep")
    assert "GraphedEwaldStep" in tpa.__all__


def test_struct_mirrors_the_header_field_by_field():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mipme_ewald_step_args \{(.*?)\} mipme_ewald_step_args_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    parsed = [re.search(r"(\w+)(?:\[(\d+)\])?$", d) for d in decls]
    names = [m.group(1) for m in parsed]
    assert names == [n for n, _ in _lib.EwaldStepArgs._fields_]
    assert names[:2] == ["size", "version"]
    # offsets: every field is 8 bytes wide except the int32 / uint32 ones (ns: three of them), which fill whole 8-byte groups --
    # no padding anywhere
    offset = 0
    for d, m in zip(decls, parsed):
        name = m.group(1)
        width = (4 if re.match(r"(u?int32_t)\b", d) else 8) * int(m.group(2) or 1)
        assert getattr(_lib.EwaldStepArgs, name).offset == offset, name
        assert getattr(_lib.EwaldStepArgs, name).size == width, name
        offset += width
    assert C.sizeof(_lib.EwaldStepArgs) == offset == 232
    assert int(re.search(r"#define MIPME_EWALD_STEP_VERSION (\d+)", hdr).group(1)) == _lib.EWALD_STEP_VERSION == 1
    a = _lib.EwaldStepArgs(n_atoms=3, ns=(C.c_int32 * 3)(8, 7, 9))
    assert a.size == 232 and a.version == 1 and a.n_atoms == 3 and list(a.ns) == [8, 7, 9]
    with pytest.raises(TypeError, match="unknown field"):
        _lib.EwaldStepArgs(no_such_field=1)


def test_symbols_are_declared_and_exported_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    lib = _lib.load()
    for name in ("mipme_ewald_step", "mipme_ewald_step_work"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    # appended entry points do not move the version
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408
    assert lib.mipme_version() == 408


def test_work_size():
    lib = _lib.load()
    work = lib.mipme_ewald_step_work
    assert work.restype is C.c_int64
    for n, k, c in ((0, 10, 0), (-1, 10, 0), ((1 << 22) + 1, 10, 0), (16, -1, 0), (16, -1, 1)):
        assert work(n, k, c) == 0, (n, k, c)
    assert 0 < work(16, 0, 0) < work(4096, 0, 0)  # it grows with the atoms ...
    assert work(16, 0, 0) < work(16, 4096, 0) < work(16, 1 << 20, 0)  # ... and with the k-vectors: more slices per atom
    assert work(300, 2048, 0) < work(300, 2048, 1) < work(300, 8192, 1)  # the cell gradient: partials per row and per k block


def test_entry_point_refusals_without_gpu():
    """Every refusal the arguments alone decide, with host pointers: -1 and the message, before any launch."""
    lib = _lib.load()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    desc = lambda **kw: _lib.PotentialDesc(**{**dict(kind=_lib.COULOMB, exponent=1, smearing=1.0, prefactor=1.0,  # noqa: E731
                                                     exclusion_radius=-1.0, exclusion_degree=1), **kw})
    smeared = desc()

    def args(**over):
        f = dict(stream=None, dtype=_lib.F64, full_list=0, pot=C.pointer(smeared), n_atoms=4, n_k=8, lr_wavelength=1.25,
                 ns=(C.c_int32 * 3)(8, 7, 9), cell_gradient=1, positions=p, charges=p, cell=p, frequencies=p, multiplicities=p,
                 row_ptr=p, entries=p, shift_format=2, records=p, kvectors=p, G=p, dG=p, s_cos=p, s_sin=p, energy=p, forces=p,
                 grad_charges=p, grad_cell=p, status=p, work=p)
        f.update(over)
        return _lib.EwaldStepArgs(**f)

    def refused(a, needle):
        assert lib.mipme_ewald_step(None if a is None else C.byref(a)) == -1
        msg = lib.mipme_last_error()
        assert needle in msg, msg

    refused(None, b"NULL argument struct")
    bad = args()
    bad.version = 7
    refused(bad, b"version 7")
    bad = args()
    bad.size = 8
    refused(bad, b"implausible argument struct size 8")
    refused(args(dtype=5), b"invalid dtype")
    refused(args(pot=None), b"potential descriptor is NULL")
    refused(args(pot=C.pointer(desc(smearing=-1.0))), b"has no smearing")
    refused(args(pot=C.pointer(desc(exclusion_radius=2.0, exclusion_degree=0))), b"exclusion_degree must be >= 1")
    refused(args(pot=C.pointer(desc(kind=_lib.INVERSE_POWER_LAW, exponent=7))), b"Unsupported exponent: 7")
    refused(args(n_k=-1), b"n_k must be >= 0")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    for n in (0, -3, (1 << 22) + 1):
        refused(args(n_atoms=n), b"n_atoms must be in 1..2^22")
    refused(args(lr_wavelength=0.0), b"lr_wavelength must be positive")
    refused(args(ns=(C.c_int32 * 3)(8, 0, 9)), b"ns >= 1")
    refused(args(grad_cell=None), b"cell_gradient needs grad_cell")
    refused(args(dG=None), b"cell_gradient needs dG")
    for name in ("positions", "charges", "cell", "row_ptr", "entries", "records", "energy", "forces", "grad_charges", "status", "work",
                 "frequencies", "multiplicities", "kvectors", "G", "s_cos", "s_sin"):
        refused(args(**{name: None}), b"NULL required buffer")
    # without k-vectors none of the reciprocal buffers is needed: what is left to object to is a required one
    refused(args(n_k=0, frequencies=None, multiplicities=None, kvectors=None, G=None, dG=None, s_cos=None, s_sin=None, cell_gradient=0,
                 grad_cell=None, work=None), b"NULL required buffer")


def test_python_refusals():
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    eye = torch.eye(3, dtype=F64) * 8
    idx = torch.tensor([[0, 1]])
    calc = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=1.0), lr_wavelength=2.0)

    def step(calc=calc, q=None, cell=eye, pos=None, idx=idx, sh=None):
        return tpa.GraphedEwaldStep(calc, z(2, 1) if q is None else q, cell, z(2, 3) if pos is None else pos, idx,
                                    z(1, 3) if sh is None else sh)

    with pytest.raises(TypeError, match="EwaldCalculator, got a PMECalculator"):
        step(calc=tpa.PMECalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=0.6))
    with pytest.raises(TypeError, match="EwaldCalculator, got a CalculatorDipole"):
        step(calc=tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=2.0))

    class Mine(tpa.CoulombPotential):
        pass

    r = torch.linspace(0.1, 6.0, 64, dtype=F64)
    others = (Mine(smearing=1.0), tpa.SplinePotential(r, torch.exp(-r), smearing=1.0),
              tpa.CombinedPotential([tpa.CoulombPotential(smearing=1.0), tpa.InversePowerLawPotential(6, smearing=1.0)], smearing=1.0))
    for pot in others:
        with pytest.raises(TypeError, match=f"exactly CoulombPotential and InversePowerLawPotential, got a {type(pot).__name__}"):
            step(calc=tpa.EwaldCalculator(pot, lr_wavelength=2.0))
    with pytest.raises(ValueError, match=r"single charge channel.*\[2, 2\]"):
        step(q=z(2, 2))
    with pytest.raises(ValueError, match=r"single charge channel.*\[2\]"):
        step(q=z(2))
    with pytest.raises(ValueError, match=r"`positions` must be a tensor with shape \[n_atoms, 3\].*\[3, 3\]"):
        step(pos=z(3, 3))
    with pytest.raises(ValueError, match=r"`positions` must be a tensor with shape \[n_atoms, 3\].*\[2, 2\]"):
        step(pos=z(2, 2))
    with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\].*\[3\]"):
        step(cell=z(3))
    with pytest.raises(ValueError, match="share one dtype.*float32.*float64"):
        step(q=torch.zeros(2, 1, dtype=torch.float32))
    with pytest.raises(ValueError, match="share one dtype"):
        step(cell=eye.float())
    with pytest.raises(ValueError, match=r"integers in \[-3, 3\]"):
        step(sh=torch.tensor([[0.0, 4.0, 0.0]], dtype=F64))
    with pytest.raises(ValueError, match=r"integers in \[-3, 3\]"):
        step(sh=torch.tensor([[0.0, 0.5, 0.0]], dtype=F64))
    with pytest.raises(ValueError, match=r"`neighbor_shifts` must be a tensor with shape \[n_pairs, 3\]"):
        step(sh=z(2, 3))
    with pytest.raises(ValueError, match=r"`neighbor_indices` must be a tensor with shape \[n_pairs, 2\]"):
        step(idx=torch.zeros((1, 3), dtype=torch.long))
    singular = eye.clone()
    singular[2] = singular[0]
    with pytest.raises(ValueError, match="not a valid unit cell"):
        step(cell=singular)
    # everything in order but on the CPU
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        step()
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        step(calc=tpa.EwaldCalculator(tpa.InversePowerLawPotential(6, smearing=1.0, exclusion_radius=2.0), lr_wavelength=2.0,
                                      full_neighbor_list=True))


@pytest.mark.parametrize("case", ["tric", "big"])
def test_kgrid_matches_agrees_with_the_frequencies_of_the_eager_call(case):
    """``kgrid_matches`` is decided by ``ns`` alone, so it needs no object: the grid ``_integer_frequencies`` builds for a cell has
    the shape the comparison predicts, for the golden cells (same grid) and for the cell scaled by 1.2 (another one)."""
    from torchpme_amd.calculators import _integer_frequencies
    from torchpme_amd.graphed import GraphedEwaldStep

    lam = float(GOLD["lr_wavelength"])
    cell0 = torch.tensor(GOLD[f"{case}_cell"], dtype=F64)
    step = GraphedEwaldStep.__new__(GraphedEwaldStep)  # (the host side of the object: no buffers, nothing launched)
    step.lr_wavelength, step.ns = lam, GraphedEwaldStep._ns_of(cell0, lam)
    assert step.ns == ((8, 7, 9) if case == "tric" else (16, 16, 16))

    def grid_shape(cell):
        f = _integer_frequencies(cell, lam, None)[0].numpy()
        return tuple(len(np.unique(f[:, d])) for d in range(3))

    strained = cell0 @ (torch.eye(3, dtype=F64) + torch.tensor(GOLD["strain"], dtype=F64))
    for cell, same in ((cell0, True), (strained, True), (1.2 * cell0, False), (cell0.float(), True)):
        assert step.kgrid_matches(cell) is same
        assert (grid_shape(cell) == step.ns) is same
