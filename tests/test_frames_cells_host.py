"""CPU tests (no GPU) of the cells of a frame batch as a replay input: the exported symbols, the C-ABI mirror of
``mipme_frames_cells_args_t``, the refusals of the two entry points that take frames (host pointers: they return before any launch),
and ``mipme_frames_cell_geometry`` -- the inversion, validity and mesh rule the launch runs, compiled for the host from the same
``__host__ __device__`` body."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import torchpme_amd as tpa
from torchpme_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = _lib.F32, _lib.F64
MESH_DIFFERS, BAD = 1, 2


def test_symbols_are_declared_and_exported_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    lib = _lib.load()
    for name in ("mipme_frames_table_cells", "mipme_frames_cells", "mipme_frames_cell_geometry"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408
    assert lib.mipme_version() == 408
    assert "follow_cells" in tpa.GraphedFrameBatch.__init__.__code__.co_varnames
    for method in ("update_cells", "mesh_matches"):
        assert callable(getattr(tpa.GraphedFrameBatch, method))


def test_struct_mirrors_the_header_field_by_field():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mipme_frames_cells_args \{(.*?)\} mipme_frames_cells_args_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    fields = []  # (`uint32_t size, version` and `int32_t dtype, n_frames` declare two fields each)
    for d in decls:
        first, *more = [part.strip() for part in d.split(",")]
        kind, name = first.rsplit(" ", 1)
        fields += [(kind, n) for n in (name, *more)]
    assert [n for _, n in fields] == [n for n, _ in _lib.FramesCellsArgs._fields_]
    offset = 0
    for kind, name in fields:
        width = 4 if re.match(r"u?int32_t$", kind) else 8
        assert getattr(_lib.FramesCellsArgs, name).offset == offset, name
        assert getattr(_lib.FramesCellsArgs, name).size == width, name
        offset += width
    assert C.sizeof(_lib.FramesCellsArgs) == offset == 112
    assert int(re.search(r"#define MIPME_FRAMES_CELLS_VERSION (\d+)", hdr).group(1)) == _lib.FRAMES_CELLS_VERSION == 1
    a = _lib.FramesCellsArgs(n_frames=3, mesh_spacing=1.25)
    assert a.size == 112 and a.version == 1 and a.n_frames == 3 and a.mesh_spacing == 1.25
    with pytest.raises(TypeError, match="unknown field"):
        _lib.FramesCellsArgs(no_such_field=1)


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    # a wrong size / version, no frames: refused by host code alone
    a = _lib.FramesCellsArgs(n_frames=0)
    assert lib.mipme_frames_cells(C.byref(a)) != 0
    assert "no frames" in lib.mipme_last_error().decode()
    a.size = 104
    assert lib.mipme_frames_cells(C.byref(a)) != 0 and "size 104" in lib.mipme_last_error().decode()
    a = _lib.FramesCellsArgs(n_frames=0)
    a.version = 7
    assert lib.mipme_frames_cells(C.byref(a)) != 0 and "version 7" in lib.mipme_last_error().decode()
    assert lib.mipme_frames_cells(None) != 0
    assert lib.mipme_frames_table_cells(F64, 0, None, None, 0, None) != 0


def _geometry(cell, dtype, ns, h):
    lib = _lib.load()
    c = np.ascontiguousarray(cell, dtype=np.float64).reshape(9)
    inv, inv_vol, status = np.full(9, np.nan), C.c_double(np.nan), C.c_int32(-1)
    n = (C.c_int32 * 3)(*ns)
    rc = lib.mipme_frames_cell_geometry(c.ctypes.data_as(C.POINTER(C.c_double)), dtype, n, h,
                                        inv.ctypes.data_as(C.POINTER(C.c_double)), C.byref(inv_vol), C.byref(status))
    assert rc == 0, lib.mipme_last_error()
    return inv.reshape(3, 3), inv_vol.value, status.value


def _triclinic(rng):
    """row norms 5 to 20, off-diagonals up to 1: condition number below 10"""
    A = np.diag(rng.uniform(5.0, 20.0, 3)) + np.where(np.eye(3) == 0, rng.uniform(-1.0, 1.0, (3, 3)), 0.0)
    return A


def test_inverse_agrees_with_numpy():
    rng = np.random.default_rng(20261020)
    for _ in range(200):
        A = _triclinic(rng)
        assert np.linalg.cond(A) < 10
        want = np.linalg.inv(A)
        for dtype in (F64, F32):
            Ad = A if dtype == F64 else A.astype(np.float32).astype(np.float64)
            want = np.linalg.inv(Ad)
            inv, inv_vol, status = _geometry(Ad, dtype, ops.ns_mesh_from_cell(Ad, 1.1), 1.1)
            assert status == 0
            assert np.abs(inv - want).max() <= 1e-13 * np.abs(want).max()
            assert abs(inv_vol * abs(np.linalg.det(Ad)) - 1.0) < 1e-13
    # nullable outputs
    lib = _lib.load()
    status = C.c_int32(-1)
    c = np.eye(3).reshape(9) * 10.0
    assert lib.mipme_frames_cell_geometry(c.ctypes.data_as(C.POINTER(C.c_double)), F64, (C.c_int32 * 3)(32, 32, 32), 1.1, None, None,
                                          C.byref(status)) == 0 and status.value == 0
    assert lib.mipme_frames_cell_geometry(c.ctypes.data_as(C.POINTER(C.c_double)), 7, (C.c_int32 * 3)(32, 32, 32), 1.1, None, None,
                                          C.byref(status)) != 0


def test_bad_cells():
    rng = np.random.default_rng(5)
    A = _triclinic(rng)
    ns = ops.ns_mesh_from_cell(A, 1.1)
    equal_rows = A.copy()
    equal_rows[2] = equal_rows[0]
    with_nan = A.copy()
    with_nan[1, 2] = np.nan
    with_inf = A.copy()
    with_inf[0, 0] = np.inf
    zero = np.zeros((3, 3))
    for dtype in (F64, F32):
        assert _geometry(A, dtype, ns, 1.1)[2] == 0
        for bad in (equal_rows, with_nan, with_inf, -with_inf, zero):
            assert _geometry(bad, dtype, ns, 1.1)[2] & BAD, bad
    # a tiny cell: 1 / V overflows float32 and not float64
    tiny = A * 1e-15
    ns_tiny = ops.ns_mesh_from_cell(tiny, 1.1)
    assert _geometry(tiny, F32, ns_tiny, 1.1)[2] & BAD
    inv, inv_vol, status = _geometry(tiny, F64, ns_tiny, 1.1)
    assert status == 0 and np.isfinite(inv).all() and np.isfinite(inv_vol)
    assert np.abs(inv - np.linalg.inv(tiny)).max() <= 1e-13 * np.abs(inv).max()
    # a huge one: the volume overflows float64
    assert _geometry(A * 1e103, F64, ns, 1.1)[2] & BAD
    # a bad cell with finite rows still reports the mesh rule (bit 0)
    ns_equal = ops.ns_mesh_from_cell(equal_rows, 1.1)
    assert _geometry(equal_rows, F64, ns_equal, 1.1)[2] == BAD
    assert _geometry(equal_rows * 4.0, F64, ns_equal, 1.1)[2] == BAD | MESH_DIFFERS


def test_mesh_rule_bit_equals_the_host_rule():
    rng = np.random.default_rng(11)
    h = 1.1
    n_cells, disagreements, flagged = 0, 0, 0
    while n_cells < 1000:
        A = np.diag(rng.uniform(3.0, 40.0, 3)) + np.where(np.eye(3) == 0, rng.uniform(-1.0, 1.0, (3, 3)), 0.0)
        x = 2.0 * np.linalg.norm(A, axis=1) / h + 1.0
        powers = 2.0 ** np.round(np.log2(x))
        if (np.abs(x - powers) <= 1e-9 * powers).any():  # (never drawn in practice; the inputs keep clear of the rule's steps)
            continue
        assert (np.abs(x - powers) > 1e-9 * powers).all()
        n_cells += 1
        frozen = ops.ns_mesh_from_cell(A, h)
        # the frozen mesh itself, and the meshes one step away per axis, a mesh of one point and one that is no power of two
        candidates = [frozen, (frozen[0] * 2, frozen[1], frozen[2]), (frozen[0], max(1, frozen[1] // 2), frozen[2]),
                      (frozen[0], frozen[1], 1), (frozen[0], 48, frozen[2])]
        # and the frozen mesh seen from a scaled cell: what a strain scan does
        s = rng.uniform(0.4, 2.5)
        for ns, cell in [(c, A) for c in candidates] + [(frozen, A * s)]:
            xs = 2.0 * np.linalg.norm(cell, axis=1) / h + 1.0
            ps = 2.0 ** np.round(np.log2(xs))
            if (np.abs(xs - ps) <= 1e-9 * ps).any():
                continue
            want = tuple(ops.ns_mesh_from_cell(cell, h)) != tuple(ns)
            got = _geometry(cell, F64, ns, h)[2]
            assert got & BAD == 0
            disagreements += bool(got & MESH_DIFFERS) != want
            flagged += want
    assert disagreements == 0
    assert flagged > 1000  # both answers occur


def test_python_side_refusals_need_no_device():
    # the class refuses `cells=` / update_cells() on a batch without follow_cells; built without a GPU through __new__
    batch = tpa.GraphedFrameBatch.__new__(tpa.GraphedFrameBatch)
    batch.follow_cells = False
    with pytest.raises(ValueError, match="follow_cells=True"):
        batch.update_cells()
    with pytest.raises(ValueError, match="follow_cells=True"):
        batch(cells=[])
    with pytest.raises(ValueError, match="follow_cells=True"):
        batch.mesh_matches()
