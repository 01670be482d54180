"""CPU tests (no GPU) of the graphed dipole step: the C-ABI mirror of ``mipme_dipole_step_args_t``, the exported symbols, the size
of the scratch, the refusals of the entry point (host pointers: it must return before any launch) and of ``GraphedDipoleStep``,
and the compaction of the k-vectors."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def test_class_is_exported():
    assert hasattr(tpa, "GraphedDipoleStep")
    assert "GraphedDipoleStep" in tpa.__all__


def test_struct_mirrors_the_header_field_by_field():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mipme_dipole_step_args \{(.*?)\} mipme_dipole_step_args_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    assert names == [n for n, _ in _lib.DipoleStepArgs._fields_]
    assert names[:2] == ["size", "version"]
    # offsets: every field is 8 bytes wide except the int32 / uint32 ones, which come in pairs -- no padding anywhere
    offset = 0
    for d, name in zip(decls, names):
        width = 4 if re.match(r"(u?int32_t)\b", d) else 8
        assert getattr(_lib.DipoleStepArgs, name).offset == offset, name
        assert getattr(_lib.DipoleStepArgs, name).size == width, name
        offset += width
    assert C.sizeof(_lib.DipoleStepArgs) == offset == 216
    assert int(re.search(r"#define MIPME_DIPOLE_STEP_VERSION (\d+)", hdr).group(1)) == _lib.DIPOLE_STEP_VERSION == 1
    a = _lib.DipoleStepArgs(n_atoms=3)
    assert a.size == 216 and a.version == 1 and a.n_atoms == 3
    with pytest.raises(TypeError, match="unknown field"):
        _lib.DipoleStepArgs(no_such_field=1)


def test_symbols_are_declared_and_exported_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    lib = _lib.load()
    for name in ("mipme_dipole_step", "mipme_dipole_step_work"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    # appended entry points do not move the version
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408
    assert lib.mipme_version() == 408


def test_work_size():
    lib = _lib.load()
    work = lib.mipme_dipole_step_work
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
    smeared = _lib.DipoleDesc(smearing=1.0, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)
    direct = _lib.DipoleDesc(smearing=-1.0, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)

    def args(**over):
        f = dict(stream=None, dtype=_lib.F64, full_list=0, pot=C.pointer(smeared), n_atoms=4, n_k=8, inv_volume=1.0, self_term=0.1,
                 background=0.0, positions=p, dipoles=p, cell=p, inv_cell=p, kvectors=p, G=p, dG=p, row_ptr=p, entries=p,
                 shift_format=2, cell_gradient=1, records=p, s_cos=p, s_sin=p, energy=p, forces=p, grad_dipoles=p, grad_cell=p,
                 work=p)
        f.update(over)
        return _lib.DipoleStepArgs(**f)

    def refused(a, needle):
        assert lib.mipme_dipole_step(None if a is None else C.byref(a)) == -1
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
    refused(args(pot=None), b"dipole descriptor is NULL")
    refused(args(pot=C.pointer(direct)), b"has no smearing")
    refused(args(pot=C.pointer(_lib.DipoleDesc(smearing=1.0, prefactor=1.0, exclusion_radius=2.0, exclusion_degree=0))),
            b"exclusion_degree must be >= 1")
    refused(args(n_k=-1), b"n_k must be >= 0")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    for n in (0, -3, (1 << 22) + 1):
        refused(args(n_atoms=n), b"n_atoms must be in 1..2^22")
    refused(args(inv_volume=0.0), b"inv_volume must be positive")
    refused(args(grad_cell=None), b"cell_gradient needs grad_cell")
    refused(args(inv_cell=None), b"cell_gradient needs grad_cell and inv_cell")
    refused(args(dG=None), b"cell_gradient needs dG")
    for name in ("positions", "dipoles", "cell", "row_ptr", "entries", "records", "energy", "forces", "grad_dipoles", "work",
                 "kvectors", "G", "s_cos", "s_sin"):
        refused(args(**{name: None}), b"NULL required buffer")
    # a direct potential needs none of the reciprocal buffers: what is left to object to is a required one
    refused(args(pot=C.pointer(direct), n_k=0, kvectors=None, G=None, dG=None, s_cos=None, s_sin=None, cell_gradient=0, grad_cell=None,
                 inv_cell=None, work=None), b"NULL required buffer")


def test_python_refusals():
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    eye = torch.eye(3, dtype=F64) * 8
    idx = torch.tensor([[0, 1]])
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=2.0)

    def step(calc=calc, mu=None, cell=eye, pos=None, idx=idx, sh=None):
        return tpa.GraphedDipoleStep(calc, z(2, 3) if mu is None else mu, cell, z(2, 3) if pos is None else pos, idx,
                                     z(1, 3) if sh is None else sh)

    with pytest.raises(TypeError, match="CalculatorDipole, got a PMECalculator"):
        step(calc=tpa.PMECalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=0.6))
    with pytest.raises(TypeError, match="CalculatorDipole, got a Calculator"):
        step(calc=tpa.Calculator(tpa.CoulombPotential()))
    with pytest.raises(ValueError, match=r"`dipoles` must be a tensor with shape \[n_atoms, 3\].*\[2, 1\]"):
        step(mu=z(2, 1))
    with pytest.raises(ValueError, match=r"`positions` must be a tensor with shape \[n_atoms, 3\].*\[3, 3\]"):
        step(pos=z(3, 3))
    with pytest.raises(ValueError, match=r"`positions` must be a tensor with shape \[n_atoms, 3\].*\[2, 2\]"):
        step(pos=z(2, 2))
    with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\].*\[3\]"):
        step(cell=z(3))
    with pytest.raises(ValueError, match="share one dtype.*float32.*float64"):
        step(mu=torch.zeros(2, 3, dtype=torch.float32))
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
    # everything in order but on the CPU
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        step()
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        step(calc=tpa.CalculatorDipole(tpa.PotentialDipole()))


def _classes(ns):
    """Number of +-k classes of the non-zero vectors of the fftfreq grid, by brute force."""
    f = [np.rint(np.fft.fftfreq(n) * n).astype(int) for n in ns]
    grid = {(a, b, c) for a in f[0] for b in f[1] for c in f[2]}
    seen = set()
    for v in grid:
        if v == (0, 0, 0):
            continue
        m = tuple(-x for x in v)
        seen.add(max(v, m) if m in grid else v)
    return len(seen)


@pytest.mark.parametrize("ns", [(15, 14, 16), (16, 16, 16), (5, 7, 3), (1, 1, 1), (2, 1, 4)])
def test_compacted_kvectors(ns):
    from torchpme_amd.graphed import _compact_kvectors

    f = [np.fft.fftfreq(n) * n for n in ns]
    F = np.stack(np.meshgrid(*f, indexing="ij"), axis=-1).reshape(-1, 3)
    rows, w = _compact_kvectors(F, ns)
    assert len(rows) == _classes(ns) and len(set(rows.tolist())) == len(rows)
    kept = {tuple(int(x) for x in F[r]) for r in rows}
    grid = {tuple(int(x) for x in v) for v in F}
    assert (0, 0, 0) not in kept
    for r, wt in zip(rows, w):
        v = tuple(int(x) for x in F[r])
        m = tuple(-x for x in v)
        assert wt == (2.0 if m in grid else 1.0)
        assert m not in kept  # one of each pair
    assert w.sum() == len(F) - 1  # every non-zero vector of the grid is accounted for once
