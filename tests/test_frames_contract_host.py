"""CPU tests (no GPU) of the first-order contract of a frame batch: ``mipme_frames_cell_work``, ``mipme_frames_table_contract``
and ``mipme_frames_step`` (include/mipme.h) -- the argument struct's mirror in ``_lib.py``, its size / version check, every
refusal before the first launch (host buffers stand in for the device pointers, as in tests/test_host.py:
test_abi_argument_errors_without_gpu -- a refusal that regressed is caught here by its return code), and the ``ValueError`` of
``GraphedFrameBatch`` that needs no device."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_step_args_mirror_the_header_field_by_field():
    assert [n for n, _ in _lib.FramesStepArgs._fields_] == _header_struct("mipme_frames_step_args_t")
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    assert int(re.search(r"#define\s+MIPME_FRAMES_STEP_VERSION\s+(\d+)", hdr).group(1)) == _lib.FRAMES_STEP_VERSION
    a = _lib.FramesStepArgs(n_frames=3)
    assert a.size == C.sizeof(_lib.FramesStepArgs) == 8 + 2 * 8 + 8 + 4 * 8 + 8 + 5 * 8 + 8
    assert a.version == _lib.FRAMES_STEP_VERSION and a.n_frames == 3
    for name in ("mipme_frames_cell_work", "mipme_frames_table_contract", "mipme_frames_step"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().mipme_version() == 408  # appended entry points do not move the version


def test_step_refuses_another_size_or_version():
    lib = _lib.load()
    a = _lib.FramesStepArgs()
    a.size -= 8
    assert lib.mipme_frames_step(C.byref(a)) == -1 and b"size" in lib.mipme_last_error()
    a = _lib.FramesStepArgs()
    a.version = _lib.FRAMES_STEP_VERSION + 1
    assert lib.mipme_frames_step(C.byref(a)) == -1 and b"version" in lib.mipme_last_error()
    assert lib.mipme_frames_step(None) == -1 and b"NULL argument struct" in lib.mipme_last_error()


def _mesh(n=32, L=14.0):
    cell = np.eye(3) * L
    md = _lib.MeshDesc(scheme=_lib.P3M, order=5, nx=n, ny=n, nz=n, n_channels=1)
    for i in range(9):
        md.cell[i] = cell.flat[i]
        md.inv_cell[i] = np.linalg.inv(cell).flat[i]
    md.volume = L**3
    return md


def _frames(n_frames, stand_in, shift_format=2, n_atoms=(100, 140, 60)):
    """Frames whose every pointer is `stand_in` (a host buffer): nothing may be launched with them."""
    fr = (_lib.Frame * n_frames)()
    for k in range(n_frames):
        f = fr[k]
        f.n_atoms, f.mesh = n_atoms[k], _mesh()
        for name, _ in _lib.Frame._fields_:
            if name not in ("n_atoms", "mesh", "full_list", "shift_format", "use_tail", "counter_ints", "dist_out"):
                setattr(f, name, stand_in)
        f.shift_format, f.use_tail, f.counter_ints = shift_format, 1, 0
    return fr


def test_size_query_is_positive_and_grows_with_the_mesh_and_the_atoms():
    lib = _lib.load()
    small, large = _mesh(32), _mesh(64)
    w32, w64 = lib.mipme_frames_cell_work(C.byref(small), 200), lib.mipme_frames_cell_work(C.byref(large), 200)
    assert 0 < w32 < w64
    assert w32 >= 32 * 32 * 17  # at least the x stage's one real per half-grid point
    assert lib.mipme_frames_cell_work(C.byref(small), 2000) > w32  # nine pair sums per wavefront of the row blocks
    assert lib.mipme_frames_cell_work(None, 200) == 0 and lib.mipme_frames_cell_work(C.byref(small), 0) == 0


def test_every_refusal_comes_before_the_first_launch():
    lib = _lib.load()
    pd = _lib.PotentialDesc(kind=_lib.COULOMB, exponent=1, smearing=1.0, prefactor=1.0, exclusion_radius=-1, exclusion_degree=1)
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    F, dt = 3, _lib.F32
    nbytes = lib.mipme_frames_table_bytes(dt, F)
    host = np.zeros((nbytes,), dtype=np.uint8)
    ptrs = (C.c_void_p * F)(a, a, a)
    stride = max(lib.mipme_frames_cell_work(C.byref(_mesh()), n) for n in (100, 140, 60))
    fr = _frames(F, a)
    assert lib.mipme_frames_table_build(dt, F, fr, C.byref(pd), host.ctypes.data, nbytes) == 0

    def contract(frames, table=host.ctypes.data, gq=ptrs, gc=ptrs, G_deriv=a, work=a, work_stride=stride):
        return lib.mipme_frames_table_contract(dt, F, frames, C.byref(pd), table, nbytes, gq, gc, G_deriv, 0, work, work_stride, a)

    def step(frames, cell_gradient=1, cell_work=a, table=a):
        args = _lib.FramesStepArgs(plan=a, stream=None, dtype=dt, n_frames=F, frames=frames, pot=C.pointer(pd), device_table=table,
                                   G=a, G_stride=0, rho_mesh_all=a, hat_work_all=a, phi_mesh_all=a, dc_all=a, cell_work=cell_work,
                                   cell_gradient=cell_gradient)
        return lib.mipme_frames_step(C.byref(args))

    # the table setter alone is host code: with everything in place it succeeds, with or without either output
    assert contract(fr) == 0
    assert contract(fr, gc=None, G_deriv=None, work=None, work_stride=0) == 0
    assert contract(fr, gq=None) == 0
    # NULL pieces
    assert contract(fr, table=None) == -1 and b"mipme_frames_table_contract" in lib.mipme_last_error()
    assert contract(fr, G_deriv=None) == -1 and b"derivative tables" in lib.mipme_last_error()
    assert contract(fr, work=None) == -1 and b"cell_work" in lib.mipme_last_error()
    assert contract(fr, work_stride=stride - 1) == -1 and b"cell_work_stride" in lib.mipme_last_error()
    assert contract(fr, gc=(C.c_void_p * F)(a, None, a)) == -1 and b"frame 1: NULL grad_cell" in lib.mipme_last_error()
    assert contract(fr, gq=(C.c_void_p * F)(a, a, None)) == -1 and b"frame 2: NULL grad_charges" in lib.mipme_last_error()
    assert step(fr, table=None) == -1 and b"NULL buffer passed to mipme_frames_step" in lib.mipme_last_error()
    assert step(fr, cell_work=None) == -1 and b"needs cell_work" in lib.mipme_last_error()
    # a frame without use_tail
    no_tail = _frames(F, a)
    no_tail[1].use_tail = 0
    for rc in (contract(no_tail), contract(no_tail, gc=None), step(no_tail), step(no_tail, cell_gradient=0)):
        assert rc == -1 and b"frame 1" in lib.mipme_last_error() and b"use_tail" in lib.mipme_last_error()
    # a shift format other than 2 with the cell gradient (format 1 is fine for the charges alone)
    fmt1 = _frames(F, a, shift_format=1)
    for rc in (contract(fmt1), step(fmt1)):
        assert rc == -1 and b"4-byte entries (shift format 2)" in lib.mipme_last_error()
    assert contract(fmt1, gc=None) == 0
    # dist_out together with the cell gradient
    dist = _frames(F, a)
    dist[2].dist_out = a
    for rc in (contract(dist), step(dist)):
        assert rc == -1 and b"frame 2" in lib.mipme_last_error() and b"dist_out" in lib.mipme_last_error()
    assert contract(dist, gc=None) == 0


def test_cell_gradient_with_stored_distances_is_refused_without_a_device():
    calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=1.0)
    z = torch.zeros
    frame = (z(4, 1), torch.eye(3) * 10, z(4, 3), z((2, 2), dtype=torch.int64), z(2, 3))
    with pytest.raises(ValueError, match="`cell_gradient` and `store_distances` exclude each other"):
        tpa.GraphedFrameBatch(calc, [frame], cell_gradient=True, store_distances=True)
