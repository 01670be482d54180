"""CPU tests (no GPU) of the slab term of a frame batch: ``mipme_frames_slab_work``, ``mipme_frames_table_slab`` and
``mipme_frames_slab_step`` (include/mipme.h) -- the argument struct's mirror in ``_lib.py``, its size / version check, every
refusal before the first launch (host buffers stand in for the device pointers, as in tests/test_frames_contract_host.py), and
the ``ValueError``s of ``GraphedFrameBatch(..., periodic=, slab_correction=)``, which need no device."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mipme_frames_slab_work", "mipme_frames_table_slab", "mipme_frames_slab_step")


def _header_struct(name):
    """Field names, in order, of `typedef struct { ... } name;` in include/mipme.h."""
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*" + name + r"\s*;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        for part in decl.strip().split(","):
            if part.strip():
                fields.append(re.search(r"(\w+)\s*(?:\[\d+\])?\s*$", part.strip()).group(1))
    return fields


def test_slab_step_args_mirror_the_header_field_by_field():
    assert [n for n, _ in _lib.FramesSlabStepArgs._fields_] == _header_struct("mipme_frames_slab_step_args_t")
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    assert int(re.search(r"#define\s+MIPME_FRAMES_SLAB_STEP_VERSION\s+(\d+)", hdr).group(1)) == _lib.FRAMES_SLAB_STEP_VERSION
    inner = _lib.FramesStepArgs(n_frames=3)
    a = _lib.FramesSlabStepArgs(step=inner, slab_work_stride=7)
    # size, version | the step's struct, unchanged | slab, slab_work, slab_work_stride
    step_size = C.sizeof(_lib.FramesStepArgs)
    assert step_size == 8 + 2 * 8 + 8 + 4 * 8 + 8 + 5 * 8 + 8  # (as tests/test_frames_contract_host.py pins it)
    assert a.size == C.sizeof(_lib.FramesSlabStepArgs) == 8 + step_size + 3 * 8
    assert a.version == _lib.FRAMES_SLAB_STEP_VERSION and a.slab_work_stride == 7
    assert a.step.n_frames == 3 and a.step.size == step_size and a.step.version == _lib.FRAMES_STEP_VERSION
    with pytest.raises(TypeError, match="unknown field"):
        _lib.FramesSlabStepArgs(no_such_field=1)
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().mipme_version() == 408  # appended entry points do not move the version


def test_slab_step_refuses_another_size_or_version():
    lib = _lib.load()
    a = _lib.FramesSlabStepArgs(step=_lib.FramesStepArgs())
    a.size -= 8
    assert lib.mipme_frames_slab_step(C.byref(a)) == -1 and b"size" in lib.mipme_last_error()
    a = _lib.FramesSlabStepArgs(step=_lib.FramesStepArgs())
    a.version = _lib.FRAMES_SLAB_STEP_VERSION + 1
    assert lib.mipme_frames_slab_step(C.byref(a)) == -1 and b"version" in lib.mipme_last_error()
    a = _lib.FramesSlabStepArgs()  # the step's struct inside has no size / version of its own
    assert lib.mipme_frames_slab_step(C.byref(a)) == -1 and b"mipme_frames_slab_step_args_t.step" in lib.mipme_last_error()
    assert lib.mipme_frames_slab_step(None) == -1 and b"NULL argument struct" in lib.mipme_last_error()


def test_size_query_is_positive():
    lib = _lib.load()
    assert lib.mipme_frames_slab_work() >= 3 + 1  # at least the three moments and a ticket word


def _mesh(n=32, L=14.0):
    cell = np.eye(3) * L
    md = _lib.MeshDesc(scheme=_lib.P3M, order=5, nx=n, ny=n, nz=n, n_channels=1)
    for i in range(9):
        md.cell[i] = cell.flat[i]
        md.inv_cell[i] = np.linalg.inv(cell).flat[i]
    md.volume = L**3
    return md


def _frames(n_frames, stand_in, n_atoms=(100, 140, 60)):
    """Frames whose every pointer is `stand_in` (a host buffer): nothing may be launched with them."""
    fr = (_lib.Frame * n_frames)()
    for k in range(n_frames):
        f = fr[k]
        f.n_atoms, f.mesh = n_atoms[k], _mesh()
        for name, _ in _lib.Frame._fields_:
            if name not in ("n_atoms", "mesh", "full_list", "shift_format", "use_tail", "counter_ints", "dist_out"):
                setattr(f, name, stand_in)
        f.shift_format, f.use_tail, f.counter_ints = 2, 1, 0
    return fr


def test_every_refusal_comes_before_the_first_launch():
    lib = _lib.load()
    coulomb = _lib.PotentialDesc(kind=_lib.COULOMB, exponent=1, smearing=1.0, prefactor=1.0, exclusion_radius=-1, exclusion_degree=1)
    r6 = _lib.PotentialDesc(kind=_lib.INVERSE_POWER_LAW, exponent=6, smearing=1.0, prefactor=1.0, exclusion_radius=-1,
                            exclusion_degree=1)
    r1 = _lib.PotentialDesc(kind=_lib.INVERSE_POWER_LAW, exponent=1, smearing=1.0, prefactor=1.0, exclusion_radius=-1,
                            exclusion_degree=1)
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    F, dt = 3, _lib.F32
    nbytes = lib.mipme_frames_table_bytes(dt, F)
    host = np.zeros((nbytes,), dtype=np.uint8)
    stride = lib.mipme_frames_slab_work()
    codes = (C.c_int32 * F)(3, 0, 1)
    ptrs = (C.c_void_p * F)(a, a, a)
    fr = _frames(F, a)
    assert lib.mipme_frames_table_build(dt, F, fr, C.byref(coulomb), host.ctypes.data, nbytes) == 0

    def table(frames=fr, pot=coulomb, tab=host.ctypes.data, slab=codes, work=a, work_stride=stride):
        return lib.mipme_frames_table_slab(dt, F, frames, C.byref(pot), tab, nbytes, slab, work, work_stride)

    def step(frames=fr, pot=coulomb, slab=codes, work=a, work_stride=stride, device_table=a, cell_gradient=0, cell_work=None):
        inner = _lib.FramesStepArgs(plan=a, stream=None, dtype=dt, n_frames=F, frames=frames, pot=C.pointer(pot),
                                    device_table=device_table, G=a, G_stride=0, rho_mesh_all=a, hat_work_all=a, phi_mesh_all=a,
                                    dc_all=a, cell_work=cell_work, cell_gradient=cell_gradient)
        args = _lib.FramesSlabStepArgs(step=inner, slab=slab, slab_work=work, slab_work_stride=work_stride)
        return lib.mipme_frames_slab_step(C.byref(args))

    def contract():
        return lib.mipme_frames_table_contract(dt, F, fr, C.byref(coulomb), host.ctypes.data, nbytes, ptrs, None, None, 0, None, 0, a)

    # the table patch alone is host code: it succeeds with everything in place, before and after the contract, for 1/r written
    # as an inverse power law, and NULL codes take the term off again
    assert table() == 0
    assert contract() == 0 and table() == 0 and contract() == 0
    assert table(pot=r1) == 0
    assert table(slab=None, work=None, work_stride=0) == 0
    # NULL pieces
    assert table(tab=None) == -1 and b"mipme_frames_table_slab" in lib.mipme_last_error()
    assert table(work=None) == -1 and b"NULL slab array or slab_work" in lib.mipme_last_error()
    assert step(work=None) == -1 and b"NULL slab array or slab_work" in lib.mipme_last_error()
    assert step(slab=None) == -1 and b"NULL slab array or slab_work" in lib.mipme_last_error()
    assert step(device_table=None) == -1 and b"NULL buffer passed to mipme_frames_slab_step" in lib.mipme_last_error()
    assert step(cell_gradient=1) == -1 and b"needs cell_work" in lib.mipme_last_error()
    # an axis code outside 0..3
    for bad in (4, -1):
        wrong = (C.c_int32 * F)(3, bad, 1)
        for rc in (table(slab=wrong), step(slab=wrong)):
            assert rc == -1 and b"frame 1: slab must be 0 (off) or the non-periodic axis + 1" in lib.mipme_last_error()
    # a frame without use_tail
    no_tail = _frames(F, a)
    no_tail[2].use_tail = 0
    for rc in (table(frames=no_tail), step(frames=no_tail)):
        assert rc == -1 and b"frame 2" in lib.mipme_last_error() and b"use_tail" in lib.mipme_last_error()
    # a potential that is not 1/r
    for rc in (table(pot=r6), step(pot=r6)):
        assert rc == -1 and b"the slab term exists for 1/r only" in lib.mipme_last_error()
    # a stride below the query
    for rc in (table(work_stride=stride - 1), step(work_stride=stride - 1)):
        assert rc == -1 and b"slab_work_stride" in lib.mipme_last_error() and b"mipme_frames_slab_work()" in lib.mipme_last_error()


def test_batch_keywords_are_checked_without_a_device():
    calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=1.0)
    z = torch.zeros
    frame = (z(4, 1), torch.eye(3) * 10, z(4, 3), z((2, 2), dtype=torch.int64), z(2, 3))
    slab = (True, True, False)
    with pytest.raises(ValueError, match="`slab_correction` needs `periodic`"):
        tpa.GraphedFrameBatch(calc, [frame, frame], slab_correction=True)
    with pytest.raises(ValueError, match="`periodic` only selects the frames and axes of `slab_correction=True`"):
        tpa.GraphedFrameBatch(calc, [frame, frame], periodic=slab)
    with pytest.raises(ValueError, match="frame 1: `slab_correction` needs exactly two periodic axes"):
        tpa.GraphedFrameBatch(calc, [frame, frame], periodic=[slab, (False, True, False)], slab_correction=True)
    with pytest.raises(ValueError, match="one triple or one triple per frame"):
        tpa.GraphedFrameBatch(calc, [frame, frame], periodic=[slab, slab, slab, slab], slab_correction=True)
    r6 = tpa.P3MCalculator(tpa.InversePowerLawPotential(exponent=6, smearing=1.0), mesh_spacing=1.0)
    with pytest.raises(ValueError, match="the slab term exists for 1/r only"):
        tpa.GraphedFrameBatch(r6, [frame, frame], periodic=slab, slab_correction=True)
    with pytest.raises(ValueError, match="the potential needs a smearing"):
        tpa.GraphedFrameBatch(tpa.Calculator(tpa.CoulombPotential()), [frame, frame], periodic=slab, slab_correction=True)
    codes = tpa.GraphedFrameBatch._slab_codes
    assert codes(calc, 3, [(True, True, False), (True, True, True), (False, True, True)], True) == [3, 0, 1]
    assert codes(calc, 2, torch.tensor([True, False, True]), True) == [2, 2]
    assert codes(calc, 2, (True, True, True), True) is None and codes(calc, 2, None, False) is None
