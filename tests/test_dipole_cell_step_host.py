"""CPU tests (no GPU) of the dipole step that follows its cell (``GraphedDipoleStep(follow_cell=True)``): the C-ABI mirror of
``mipme_dipole_cell_step_args_t``, the exported symbols, the size of the scratch, the refusals of the entry point (host pointers:
it must return before any launch) and of the Python surface, ``kgrid_matches``, and the contents of the golden file."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dipole_cell_step.npz"))
F64 = torch.float64


def test_struct_mirrors_the_header_field_by_field():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mipme_dipole_cell_step_args \{(.*?)\} mipme_dipole_cell_step_args_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)(\[3\])?$", d).group(1) for d in decls]
    assert names == [n for n, _ in _lib.DipoleCellStepArgs._fields_]
    assert names[:2] == ["size", "version"]
    assert "inv_volume" not in names and "inv_cell" not in names  # nothing that depends on the cell's values goes in by value
    # offsets: every field is 8 bytes wide except the int32 / uint32 ones, which come in pairs (ns[3] + cell_gradient) -- no padding
    offset = 0
    for d, name in zip(decls, names):
        width = 12 if d.endswith("[3]") else 4 if re.match(r"(u?int32_t)\b", d) else 8
        assert getattr(_lib.DipoleCellStepArgs, name).offset == offset, name
        assert getattr(_lib.DipoleCellStepArgs, name).size == width, name
        if width == 8:
            assert offset % 8 == 0, name
        offset += width
    assert C.sizeof(_lib.DipoleCellStepArgs) == offset == 248
    assert int(re.search(r"#define MIPME_DIPOLE_CELL_STEP_VERSION (\d+)", hdr).group(1)) == _lib.DIPOLE_CELL_STEP_VERSION == 1
    a = _lib.DipoleCellStepArgs(n_atoms=3)
    assert a.size == 248 and a.version == 1 and a.n_atoms == 3
    with pytest.raises(TypeError, match="unknown field"):
        _lib.DipoleCellStepArgs(inv_volume=1.0)
    # the struct of the fixed-cell step is what it was
    assert C.sizeof(_lib.DipoleStepArgs) == 216 and _lib.DIPOLE_STEP_VERSION == 1


def test_symbols_are_declared_and_exported_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    lib = _lib.load()
    for name in ("mipme_dipole_cell_step", "mipme_dipole_cell_step_work"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    # appended entry points do not move the version
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408
    assert lib.mipme_version() == 408


def test_work_size():
    lib = _lib.load()
    work, plain = lib.mipme_dipole_cell_step_work, lib.mipme_dipole_step_work
    assert work.restype is C.c_int64
    for n, k, c in ((0, 10, 0), (-1, 10, 0), ((1 << 22) + 1, 10, 0), (16, -1, 0), (16, -1, 1)):
        assert work(n, k, c) == 0, (n, k, c)
    assert 0 < work(16, 0, 0) < work(4096, 0, 0)  # it grows with the atoms ...
    assert work(16, 0, 0) < work(16, 4096, 0) < work(16, 1 << 20, 0)  # ... and with the k-vectors: more slices per atom
    assert work(300, 2048, 0) < work(300, 2048, 1) < work(300, 8192, 1)  # the cell gradient: partials per row and per k block
    for n, k, c in ((1, 0, 0), (16, 0, 1), (300, 2048, 0), (300, 2048, 1), (8000, 9841, 1)):
        assert work(n, k, c) == plain(n, k, c) + 16, (n, k, c)  # the head: the geometry record


def test_entry_point_refusals_without_gpu():
    """Every refusal the arguments alone decide, with host pointers: -1 and the message, before any launch."""
    lib = _lib.load()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    smeared = _lib.DipoleDesc(smearing=1.0, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)
    direct = _lib.DipoleDesc(smearing=-1.0, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)

    def args(**over):
        f = dict(stream=None, dtype=_lib.F64, full_list=0, pot=C.pointer(smeared), self_term=0.1, background=0.0, n_atoms=4, n_k=8,
                 lr_wavelength=1.0, ns=(C.c_int32 * 3)(3, 3, 3), cell_gradient=1, positions=p, dipoles=p, cell=p, frequencies=p,
                 multiplicities=p, row_ptr=p, entries=p, shift_format=2, records=p, kvectors=p, G=p, dG=p, s_cos=p, s_sin=p,
                 energy=p, forces=p, grad_dipoles=p, grad_cell=p, status=p, work=p)
        f.update(over)
        return _lib.DipoleCellStepArgs(**f)

    def refused(a, needle):
        assert lib.mipme_dipole_cell_step(None if a is None else C.byref(a)) == -1
        msg = lib.mipme_last_error()
        assert needle in msg and b"mipme_dipole_cell_step" in msg, msg

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
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        refused(args(lr_wavelength=lam), b"lr_wavelength must be positive")
    refused(args(ns=(C.c_int32 * 3)(3, 0, 3)), b"ns >= 1")
    refused(args(pot=C.pointer(_lib.DipoleDesc(smearing=1.0, prefactor=1.0, exclusion_radius=2.0, exclusion_degree=0))),
            b"exclusion_degree must be >= 1")
    refused(args(n_k=-1), b"n_k must be >= 0")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    for n in (0, -3, (1 << 22) + 1):
        refused(args(n_atoms=n), b"n_atoms must be in 1..2^22")
    refused(args(grad_cell=None), b"cell_gradient needs grad_cell")
    refused(args(dG=None), b"cell_gradient needs dG")
    refused(args(status=None), b"status is NULL")
    for name in ("positions", "dipoles", "cell", "row_ptr", "entries", "records", "energy", "forces", "grad_dipoles", "work",
                 "frequencies", "multiplicities", "kvectors", "G", "s_cos", "s_sin"):
        refused(args(**{name: None}), b"NULL required buffer")
    # the order: what comes first in the list above wins
    refused(args(dtype=5, pot=None), b"invalid dtype")
    refused(args(pot=C.pointer(direct), lr_wavelength=0.0), b"has no smearing")
    refused(args(shift_format=0, n_atoms=0), b"shift_format 2")
    refused(args(grad_cell=None, status=None), b"cell_gradient needs grad_cell")
    refused(args(status=None, positions=None), b"status is NULL")
    # a direct potential needs no grid and none of the reciprocal buffers: what is left to object to is a required one
    refused(args(pot=C.pointer(direct), n_k=0, lr_wavelength=0.0, ns=(C.c_int32 * 3)(0, 0, 0), frequencies=None, multiplicities=None,
                 kvectors=None, G=None, dG=None, s_cos=None, s_sin=None, cell_gradient=0, grad_cell=None, work=None),
            b"NULL required buffer")


def _host_step(follow_cell, dtype=F64, lam=0.5, cell0=None):
    """The host side of an object (no buffers, nothing launched): what the refusals and ``kgrid_matches`` read."""
    from torchpme_amd.graphed import GraphedDipoleStep, GraphedEwaldStep

    step = GraphedDipoleStep.__new__(GraphedDipoleStep)
    step.follow_cell, step.dtype, step.device = follow_cell, dtype, torch.device("cpu")
    if follow_cell:
        step.lr_wavelength = lam
        step.ns = (1, 1, 1) if cell0 is None else GraphedEwaldStep._ns_of(cell0, lam)
    return step


def test_python_refusals():
    sig = inspect.signature(tpa.GraphedDipoleStep.__init__)
    assert list(sig.parameters)[1:] == ["calculator", "dipoles", "cell", "positions", "neighbor_indices", "neighbor_shifts",
                                        "cell_gradient", "warmup", "follow_cell"]
    assert sig.parameters["follow_cell"].default is False and sig.parameters["warmup"].default == 3
    eye = torch.eye(3, dtype=F64) * 8
    idx, sh = torch.tensor([[0, 1]]), torch.zeros(1, 3, dtype=F64)
    # `cell=` on an object built without the keyword, in a call and in recapture: the reason names the keyword
    plain = _host_step(False)
    with pytest.raises(ValueError, match="follow_cell=True"):
        plain(cell=eye)
    with pytest.raises(ValueError, match="follow_cell=True"):
        plain.recapture(idx, sh, cell=eye)
    with pytest.raises(ValueError, match="follow_cell=True"):
        plain.kgrid_matches(eye)
    # a cell that is not (3, 3) of the object's dtype and device, before anything of the object changes (there is nothing
    # else in this object: anything past the check would raise an AttributeError)
    step = _host_step(True)
    for bad in (torch.zeros(3, dtype=F64), torch.zeros(9, dtype=F64), torch.zeros(1, 3, 3, dtype=F64), eye[:2]):
        with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\]"):
            step(cell=bad)
        with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\]"):
            step.recapture(idx, sh, cell=bad)
    with pytest.raises(ValueError, match=r"torch.float64.*got.*torch.float32"):
        step(cell=eye.float())
    with pytest.raises(ValueError, match=r"torch.float32.*got.*torch.float64"):
        _host_step(True, torch.float32).recapture(idx, sh, cell=eye)
    with pytest.raises(ValueError, match=r"`cell` must be a tensor"):
        step(cell=eye.numpy())
    # the constructor: the checks of the fixed-cell object, then "no CPU fallback"
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=2.0)
    with pytest.raises(ValueError, match=r"`cell` must be a tensor with shape \[3, 3\].*\[3\]"):
        tpa.GraphedDipoleStep(calc, z(2, 3), z(3), z(2, 3), idx, sh, follow_cell=True)
    with pytest.raises(ValueError, match="share one dtype"):
        tpa.GraphedDipoleStep(calc, z(2, 3), eye.float(), z(2, 3), idx, sh, follow_cell=True)
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        tpa.GraphedDipoleStep(calc, z(2, 3), eye, z(2, 3), idx, sh, follow_cell=True)


@pytest.mark.parametrize("case", ["tric", "big"])
def test_kgrid_matches_is_the_rule_of_the_ewald_step(case):
    from torchpme_amd.calculators import _integer_frequencies
    from torchpme_amd.graphed import GraphedEwaldStep

    lam = 0.5 if case == "tric" else 1.25
    cell0 = torch.tensor(GOLD[f"{case}_cell"], dtype=F64)
    step = _host_step(True, lam=lam, cell0=cell0)
    assert step.ns == tuple(int(n) for n in GOLD[f"{case}_ns"])
    ewald = GraphedEwaldStep.__new__(GraphedEwaldStep)
    ewald.lr_wavelength, ewald.ns = lam, step.ns

    def grid_shape(cell):
        f = _integer_frequencies(cell, lam, None)[0].numpy()
        return tuple(len(np.unique(f[:, d])) for d in range(3))

    strained = cell0 @ (torch.eye(3, dtype=F64) + torch.tensor(GOLD["strain"], dtype=F64))
    for cell, same in ((cell0, True), (strained, True), (1.2 * cell0, False), (cell0.float(), True)):
        assert step.kgrid_matches(cell) is same is ewald.kgrid_matches(cell)
        assert (grid_shape(cell) == step.ns) is same
    # a direct potential sums no grid: no cell differs
    direct = _host_step(True, lam=0.0)
    assert direct.kgrid_matches(cell0) and direct.kgrid_matches(5.0 * cell0)


def test_golden_file_has_every_case():
    variants = [str(n) for n in GOLD["tric_variants"]]
    assert variants == ["half", "full", "direct", "excl1", "excl3", "eps", "pref"]
    cases = [f"tric_{v}" for v in variants] + ["big_half", "big_full"]
    for p in cases:
        for ctag in ("c0", "c1"):
            for key in ("E", "gmu", "gpos", "gcell"):
                assert GOLD[f"{p}_{key}_{ctag}_f64"].dtype == np.float64 and GOLD[f"{p}_{key}_{ctag}_f32"].dtype == np.float32
            assert float(GOLD[f"{p}_absE_{ctag}"]) > 0
        for key in ("full", "lr_wavelength", "smearing", "exclusion_radius", "epsilon", "prefactor", "exclusion_degree"):
            assert f"{p}_{key}" in GOLD.files
    for key in ("E", "gmu", "gpos", "gcell"):
        assert f"kept_{key}_c0_f64" in GOLD.files and f"kept_{key}_c0_f32" in GOLD.files
    assert float(GOLD["kept_absE_c0"]) > 0 and float(GOLD["kept_scale"]) == 1.2 and float(GOLD["kept_lr_wavelength"]) == 0.6
    for v in variants:
        assert GOLD[f"tric_{v}_pairs"].dtype == np.int16 and GOLD[f"tric_{v}_shifts"].dtype == np.int8
    assert GOLD["big_pairs"].dtype == np.int16 and GOLD["big_shifts"].dtype == np.int8 and GOLD["big_positions"].shape == (300, 3)
    # the grids the script asserts: the same at c0 and c1, and the kept grid at 1.2 cell with lr_wavelength 0.6
    strain = np.eye(3) + GOLD["strain"]
    ns = lambda cell, lam: [int(n) for n in np.ceil(np.linalg.norm(cell, axis=1) / lam)]  # noqa: E731
    assert ns(GOLD["tric_cell"], 0.5) == ns(GOLD["tric_cell"] @ strain, 0.5) == list(GOLD["tric_ns"]) == [15, 14, 16]
    assert ns(GOLD["big_cell"], 1.25) == ns(GOLD["big_cell"] @ strain, 1.25) == list(GOLD["big_ns"]) == [16, 16, 16]
    assert float(GOLD["big_cell"][0, 0]) == 19.4
    assert ns(1.2 * GOLD["tric_cell"], 0.6) == list(GOLD["kept_ns"]) == [15, 14, 16] != ns(1.2 * GOLD["tric_cell"], 0.5)
    # the construction-cell results are those of dipole_step.npz
    old = np.load(os.path.join(ROOT, "tests", "golden", "dipole_step.npz"))
    for v in variants:
        np.testing.assert_allclose(GOLD[f"tric_{v}_E_c0_f64"], old[f"tric_{v}_E_f64"], rtol=1e-13)
        np.testing.assert_allclose(GOLD[f"tric_{v}_gcell_c0_f64"], old[f"tric_{v}_gcell_f64"], rtol=1e-10, atol=1e-12)
