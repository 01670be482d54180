"""``GraphedFrameBatch(follow_cells=True)``: the cells of a frame batch as a replay input (``mipme_frames_table_cells`` /
``mipme_frames_cells``; csrc/frames_cells.hip).  One launch ahead of the unchanged step graph turns the cells on the device into
the geometry of the batch's table, its G(k) and derivative tables and the validated copy of the cells the pair rows read.

Shapes: those of tests/test_gpu_frames_contract.py (three frames of 216 / 343 / 125 atoms, 32^3 at h = 1.1; the two slabs at
64 x 64 x 128 for the brick route).  Strained cells: ``cell_f @ (I + (f + 1) EPS)`` with the EPS of the Ewald step's golden data,
positions scaled along, pair lists kept (the same pairs for the oracle and for the batch)."""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import torchpme_amd as tpa  # noqa: E402
from torchpme_amd import _lib, ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pme_numpy as O  # noqa: E402
from tests.test_gpu_frames_contract import (DEV, KINDS, SM, boxes, frames_of, make_calc, oracle_contract, rel,  # noqa: E402
                                            tol_of)

EPS = np.array([[0.012, 0.004, -0.003], [0.004, -0.009, 0.005], [-0.003, 0.005, 0.007]])  # tests/golden/make_ewald_step_golden.py
F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
FLAGS = dict(charge_gradient=True, cell_gradient=True, follow_cells=True)


def tight_of(dtype):
    return 1e-11 if dtype == F64 else 2e-5


def strain(bx, scale=1.0):
    """(cell, positions) of every frame under I + (f + 1) scale EPS"""
    return [(b["cell"] @ (np.eye(3) + (f + 1) * scale * EPS), b["pos"] @ (np.eye(3) + (f + 1) * scale * EPS)) for f, b in enumerate(bx)]


_STRAINED = {}


def strained_refs(kind, full, layout="cubes"):
    """Strained cells and positions of a case with the oracle's answers at them: computed once, shared, left unchanged."""
    key = (kind, full, layout)
    if key not in _STRAINED:
        scheme, order, expo = KINDS[kind]
        h, bx = boxes(kind, full, layout)
        spec = O.PotentialSpec("coulomb" if expo == 1 else "ipl", expo, SM, 1.0)
        out = []
        for b, (cell, pos) in zip(bx, strain(bx)):
            out.append(dict(cell=cell, pos=pos, ref=oracle_contract(spec, scheme, order, h, b["q"], cell, pos, b["pairs"], b["S"], full)))
        _STRAINED[key] = out
    return _STRAINED[key]


def t(a, dtype):
    return torch.tensor(a, device=DEV, dtype=dtype)


def snapshot(out):
    """host copies of what a call returned (the buffers are static)"""
    torch.cuda.synchronize()
    E, F, dq, dc = out
    return (E.cpu().double().numpy().copy(), [f.cpu().double().numpy().copy() for f in F],
            [g.cpu().double().numpy().copy() for g in dq], dc.cpu().double().numpy().copy())


def errors(got, want, k):
    """relative errors (E, F, dE/dq, dE/dcell) of frame k between two snapshots, each by the largest component of `want`"""
    r = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    return (abs(got[0][k] - want[0][k]) / abs(want[0][k]), r(got[1][k], want[1][k]), r(got[2][k], want[2][k]), r(got[3][k], want[3][k]))


def check_oracle(out, refs, tol, what):
    E, F, dq, dc = out
    torch.cuda.synchronize()
    for k, ref in enumerate(refs):
        Eo, gpo, dqo, dco = ref
        errs = (abs(float(E[k]) - Eo) / abs(Eo), rel(-F[k], gpo), rel(dq[k], dqo), rel(dc[k], dco))
        print(f"{what} frame {k}: rel. errors E {errs[0]:.2e}  F {errs[1]:.2e}  dE/dq {errs[2]:.2e}  dE/dcell {errs[3]:.2e}")
        assert max(errs) <= tol, (what, k, errs)


def check_same(got, want, frames, dtype, what):
    """E, F, dE/dq within `tight`, dE/dcell within the contract's tolerance"""
    for k in frames:
        errs = errors(got, want, k)
        print(f"{what} frame {k}: E {errs[0]:.2e}  F {errs[1]:.2e}  dE/dq {errs[2]:.2e}  dE/dcell {errs[3]:.2e}")
        assert max(errs[:3]) <= tight_of(dtype) and errs[3] <= tol_of(dtype), (what, k, errs)


def status_of(batch):
    torch.cuda.synchronize()
    return batch.status.cpu().tolist()


def test_the_frozen_mesh_holds_under_the_strains():
    h, bx = boxes("p3m5-coulomb", False)
    for scale in (1.0, -1.0, 0.5):
        assert all(tuple(O.get_ns_mesh(cell, h)) == (32, 32, 32) for cell, _ in strain(bx, scale))
    h, bx = boxes("p3m5-coulomb", False, "slabs")
    assert all(tuple(O.get_ns_mesh(cell, h)) == (64, 64, 128) for cell, _ in strain(bx))


@DTYPES
@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_both_cells_from_one_graph_against_the_oracle(kind, full, dtype):
    h, bx = boxes(kind, full)
    refs = strained_refs(kind, full)
    assert all(tuple(O.get_ns_mesh(r["cell"], h)) == (32, 32, 32) for r in refs)
    calc = make_calc(kind, h, full, dtype)
    batch = tpa.GraphedFrameBatch(calc, frames_of(bx, dtype), **FLAGS)
    graph = batch.graph
    assert batch.ns == (32, 32, 32) and batch.cells.shape == (3, 3, 3) and batch.cells.dtype == dtype
    check_oracle(batch(), [b["ref"][0] for b in bx], tol_of(dtype), "cell0")
    assert status_of(batch) == [0, 0, 0]
    out = batch([t(r["pos"], dtype) for r in refs], cells=[t(r["cell"], dtype) for r in refs])
    check_oracle(out, [r["ref"] for r in refs], tol_of(dtype), "strained")
    assert status_of(batch) == [0, 0, 0] and batch.mesh_matches() == [True, True, True]
    assert batch.graph is graph
    assert _lib.load().mipme_last_cosched_kernel() == b"frames_plane_rows_kernel"
    # the (F, 3, 3) tensor form, back at cell0
    out = batch([t(b["pos"], dtype) for b in bx], cells=t(np.stack([b["cell"] for b in bx]), dtype))
    check_oracle(out, [b["ref"][0] for b in bx], tol_of(dtype), "cell0 again")
    assert batch.graph is graph


@DTYPES
@pytest.mark.parametrize("kind", list(KINDS))
def test_against_a_fresh_batch_at_the_strained_cells(kind, dtype):
    h, bx = boxes(kind, False)
    st = strain(bx)
    calc = make_calc(kind, h, False, dtype)
    batch = tpa.GraphedFrameBatch(calc, frames_of(bx, dtype), **FLAGS)
    got = snapshot(batch([t(p, dtype) for _, p in st], cells=[t(c, dtype) for c, _ in st]))
    at = [dict(b, cell=c, pos=p) for b, (c, p) in zip(bx, st)]
    fresh = tpa.GraphedFrameBatch(make_calc(kind, h, False, dtype), frames_of(at, dtype), charge_gradient=True, cell_gradient=True)
    assert fresh.ns == batch.ns and fresh.cells is None and fresh.status is None
    want = snapshot(fresh())
    check_same(got, want, range(3), dtype, "follow_cells vs fresh")
    if dtype == F64:  # the same kernels' tables: only the inversion differs (cofactors on the device, LAPACK on the host)
        for name in ("_G", "_G_deriv"):
            a, b = getattr(batch, name).cpu().numpy(), getattr(fresh, name).cpu().numpy()
            assert a.shape == b.shape
            err = np.abs(a - b).max() / min(np.abs(a).max(), np.abs(b).max())
            print(f"{name}: largest difference / largest entry = {err:.2e}")
            assert err <= 1e-11


@DTYPES
def test_cells_come_and_go(dtype):
    kind = "p3m5-coulomb"
    h, bx = boxes(kind, False)
    st = strain(bx)
    batch = tpa.GraphedFrameBatch(make_calc(kind, h, False, dtype), frames_of(bx, dtype), **FLAGS)
    pos0, cells0 = [t(b["pos"], dtype) for b in bx], [t(b["cell"], dtype) for b in bx]
    tables = lambda: (batch._G.clone(), batch._G_deriv.clone(), batch._table.clone(), batch._cells_valid.clone())  # noqa: E731
    first, tab1 = snapshot(batch(pos0, cells=cells0)), tables()
    second, tab2 = snapshot(batch([t(p, dtype) for _, p in st], cells=[t(c, dtype) for c, _ in st])), tables()
    third, tab3 = snapshot(batch(pos0, cells=cells0)), tables()
    for a, b in zip(tab1, tab3):  # a function of the buffer alone
        assert torch.equal(a, b)
    assert not torch.equal(tab1[0], tab2[0]) and not torch.equal(tab1[2], tab2[2]) and not torch.equal(tab1[3], tab2[3])
    check_same(third, first, range(3), dtype, "cell0 after strained")
    for k in range(3):
        assert abs(second[0][k] - first[0][k]) > 1e-4 * abs(first[0][k])
        assert np.abs(second[3][k] - first[3][k]).max() > 1e-4 * np.abs(first[3][k]).max()


@pytest.mark.parametrize("kind", ["p3m5-coulomb", "p3m5-r6"])
def test_finite_differences(kind):
    """All nine components of dE/dcell of frame 0, at fixed Cartesian positions and at the frozen mesh, from central differences of
    energies[0] through ``cells=``: h = 1e-5, bound 1e-6 of the largest component (tests/test_gpu_ewald_step.py, same rule).
    Frame 2 rides along with its cell untouched: its tables stay bit-equal and its results within `tight`."""
    h, bx = boxes(kind, False)
    two = [bx[0], bx[2]]
    batch = tpa.GraphedFrameBatch(make_calc(kind, h, False, F64), frames_of(two, F64), **FLAGS)
    base = snapshot(batch())
    Mh = batch._G.shape[1]
    G2, D2 = batch._G[1].clone(), batch._G_deriv[1].clone()
    step = 1e-5
    scale = np.abs(base[3][0]).max()
    cell2 = t(two[1]["cell"], F64)
    for a in range(3):
        for b in range(3):
            e = []
            for sgn in (+1.0, -1.0):
                c = two[0]["cell"].copy()
                c[a, b] += sgn * step
                out = snapshot(batch(cells=[t(c, F64), cell2]))
                e.append(out[0][0])
                errs = errors(out, base, 1)
                assert max(errs[:3]) <= tight_of(F64) and errs[3] <= tol_of(F64), (a, b, errs)
            fd, got = (e[0] - e[1]) / (2 * step), base[3][0][a, b]
            print(f"finite difference dE/dcell[{a},{b}]: {fd:.12e} analytic {got:.12e}")
            assert abs(fd - got) <= 1e-6 * scale
    assert batch._G.shape[1] == Mh and torch.equal(batch._G[1], G2) and torch.equal(batch._G_deriv[1], D2)
    assert status_of(batch) == [0, 0]


@DTYPES
def test_brick_route_and_the_slab_term(dtype):
    kind = "p3m5-coulomb"
    h, bx = boxes(kind, False, "slabs")
    st = strain(bx)
    assert all(tuple(O.get_ns_mesh(c, h)) == (64, 64, 128) for c, _ in st)
    periodic = [(True, True, False), (True, True, True)]
    batch = tpa.GraphedFrameBatch(make_calc(kind, h, False, dtype), frames_of(bx, dtype), periodic=periodic, slab_correction=True, **FLAGS)
    assert _lib.load().mipme_last_cosched_kernel() == b"frames_spread_rows_kernel"
    before = snapshot(batch())
    got = snapshot(batch([t(p, dtype) for _, p in st], cells=[t(c, dtype) for c, _ in st]))
    assert _lib.load().mipme_last_cosched_kernel() == b"frames_spread_rows_kernel" and status_of(batch) == [0, 0]
    at = [dict(b, cell=c, pos=p) for b, (c, p) in zip(bx, st)]
    fresh = tpa.GraphedFrameBatch(make_calc(kind, h, False, dtype), frames_of(at, dtype), periodic=periodic, slab_correction=True,
                                  charge_gradient=True, cell_gradient=True)
    check_same(got, snapshot(fresh()), range(2), dtype, "slab batch vs fresh")
    assert abs(got[0][0] - before[0][0]) > 1e-4 * abs(before[0][0])


@DTYPES
def test_a_half_grid_that_is_no_multiple_of_the_block(dtype):
    """The launch alone, through the C interface, on a 20 x 20 x 20 mesh: 4 400 half-grid points, 17.2 blocks of 256.

    The frames path refuses the 8 x 16 x 16 mesh (it needs more than 16 points per axis), and every mesh the mesh rule can give it is
    a power of two per axis with nx ny >= 1024, so its half grid is always a multiple of 256.  20^3 is the smallest mesh the entry
    point's checks admit whose half grid is not; the step itself needs a power-of-two nx, so here the cells launch runs on its
    own and its tables are compared with the host-built ones of the same mesh.  The words behind every slice must stay untouched."""
    lib = _lib.load()
    dt = _lib.dtype_code(dtype)
    F, ns, h = 2, (20, 20, 20), 1.1
    Mh = 20 * 20 * 11
    assert Mh % 256 != 0
    rng = np.random.default_rng(3)
    cells = np.stack([np.diag([9.0, 10.0, 11.0]) + 0.4 * rng.uniform(-1, 1, (3, 3)) for _ in range(F)])
    pot = tpa.CoulombPotential(smearing=SM)._descriptor()
    geoms = [ops.MeshGeometry(c if dtype == F64 else c.astype(np.float32).astype(np.float64), ns, _lib.P3M, 5) for c in cells]
    dummy = torch.zeros((4096,), dtype=torch.float64, device=DEV)  # stands in for every buffer the launch never touches
    cells_in, valid = t(cells, dtype), torch.zeros((F, 3, 3), dtype=dtype, device=DEV)
    frames = (_lib.Frame * F)()
    for k, f in enumerate(frames):
        for name, kind in _lib.Frame._fields_:
            if kind is C.c_void_p:
                setattr(f, name, dummy.data_ptr())
        f.n_atoms, f.mesh, f.cell, f.dist_out = 8, geoms[k].desc(1), valid[k].data_ptr(), None
        f.full_list, f.shift_format, f.use_tail, f.counter_ints = 0, 2, 1, 0
    nbytes = lib.mipme_frames_table_bytes(dt, F)
    host = np.zeros((nbytes,), dtype=np.uint8)
    _lib.check(lib.mipme_frames_table_build(dt, F, frames, C.byref(pot), host.ctypes.data, nbytes))
    status = torch.full((F,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.mipme_frames_table_cells(dt, F, frames, host.ctypes.data, nbytes, status.data_ptr()))
    table = torch.from_numpy(host).to(DEV)
    pad, mark = 64, -7.0
    G = torch.full((F, Mh + pad), mark, dtype=dtype, device=DEV)
    D = torch.full((F, 4 * Mh + pad), mark, dtype=dtype, device=DEV)
    a = _lib.FramesCellsArgs(stream=_lib.current_stream(torch.device(DEV, 0)), dtype=dt, n_frames=F, frames=frames, pot=C.pointer(pot),
                             device_table=table.data_ptr(), cells=cells_in.data_ptr(), cells_valid=valid.data_ptr(), G=G.data_ptr(),
                             G_stride=G.shape[1], G_deriv=D.data_ptr(), G_deriv_stride=D.shape[1], mesh_spacing=h,
                             status=status.data_ptr())
    # refusals first: a shared table, a cell pointer outside the validated copy
    a.G_stride = 0
    assert lib.mipme_frames_cells(C.byref(a)) != 0 and b"G_stride" in lib.mipme_last_error()
    a.G_stride = G.shape[1]
    frames[1].cell = dummy.data_ptr()
    assert lib.mipme_frames_cells(C.byref(a)) != 0 and b"cells_valid" in lib.mipme_last_error()
    frames[1].cell = valid[1].data_ptr()
    with _lib.on_device(torch.device(DEV, 0)):
        _lib.check(lib.mipme_frames_cells(C.byref(a)))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [1, 1]  # valid cells; 20 is not what the mesh rule gives
    assert torch.equal(valid, cells_in)
    assert bool((G[:, Mh:] == mark).all()) and bool((D[:, 4 * Mh:] == mark).all())
    tol = 1e-11 if dtype == F64 else 4 * float(np.finfo(np.float32).eps)  # (fp32: the float64 values differ by ~1e-15, rounded once)
    for k in range(F):
        Gh = ops.build_filter(geoms[k], pot, dtype, torch.device(DEV, 0)).reshape(-1)
        Dh = ops.filter_derivative(geoms[k], pot, dtype, torch.device(DEV, 0)).reshape(-1)
        for got, want in ((G[k, :Mh], Gh), (D[k, :4 * Mh], Dh)):
            assert float((got - want).abs().max()) <= tol * float(want.abs().max())


def test_status_bit_0_a_cell_the_frozen_mesh_no_longer_fits():
    kind = "p3m5-coulomb"
    h, bx = boxes(kind, False)
    scheme, order, expo = KINDS[kind]
    cells = [1.3 * bx[0]["cell"], bx[1]["cell"], bx[2]["cell"]]
    pos = [1.3 * bx[0]["pos"], bx[1]["pos"], bx[2]["pos"]]
    assert tuple(O.get_ns_mesh(cells[0], h)) == (64, 64, 64) and tuple(O.get_ns_mesh(cells[2], h)) == (32, 32, 32)
    assert tuple(O.get_ns_mesh(cells[0], 1.3 * h)) == (32, 32, 32)
    for dtype in (F64, F32):
        batch = tpa.GraphedFrameBatch(make_calc(kind, h, False, dtype), frames_of(bx, dtype), **FLAGS)
        out = batch([t(p, dtype) for p in pos], cells=[t(c, dtype) for c in cells])
        assert status_of(batch) == [1, 0, 0]
        assert bool(torch.isfinite(out[0]).all())
        assert batch.mesh_matches() == [False, True, True] and batch.mesh_matches(cells) == [False, True, True]
        assert batch.ns == (32, 32, 32)
        if dtype == F64:  # the frozen 32^3 mesh on the scaled cell is what the oracle builds for a spacing of 1.3 h
            spec = O.PotentialSpec("coulomb", 1, SM, 1.0)
            b = bx[0]
            ref = oracle_contract(spec, scheme, order, 1.3 * h, b["q"], cells[0], pos[0], b["pairs"], b["S"], False)
            check_oracle(tuple(x[:1] for x in out), [ref], 1e-9, "scaled by 1.3")


@DTYPES
def test_status_bit_1_a_singular_cell_and_recovery(dtype):
    kind = "p3m5-coulomb"
    h, bx = boxes(kind, False)
    batch = tpa.GraphedFrameBatch(make_calc(kind, h, False, dtype), frames_of(bx, dtype), **FLAGS)
    good = [t(b["cell"], dtype) for b in bx]
    before = snapshot(batch())
    tables = (batch._G.clone(), batch._G_deriv.clone(), batch._table.clone(), batch._cells_valid.clone())
    singular = bx[1]["cell"].copy()
    singular[2] = singular[0]  # two equal rows
    out = snapshot(batch(cells=[good[0], t(singular, dtype), good[2]]))
    assert status_of(batch) == [0, 2, 0]
    assert np.isnan(out[0][1]) and np.isfinite(out[0][[0, 2]]).all()
    check_same(out, before, (0, 2), dtype, "beside a singular cell")
    # nothing of the batch's geometry changed: the bad cell stays in the input buffer alone
    for a, b in zip(tables, (batch._G, batch._G_deriv, batch._table, batch._cells_valid)):
        assert torch.equal(a, b)
    assert all(np.isfinite(x).all() for x in out[1] + out[2]) and np.isfinite(out[3]).all()
    out = batch(cells=good)
    assert status_of(batch) == [0, 0, 0]
    check_oracle(out, [b["ref"][0] for b in bx], tol_of(dtype), "recovered")


def test_refusals_and_the_fixed_cell_path():
    kind, dtype = "p3m5-coulomb", F64
    h, bx = boxes(kind, False)
    frames = frames_of(bx, dtype)
    calc = make_calc(kind, h, False, dtype)
    good = [f[1] for f in frames]
    fixed = tpa.GraphedFrameBatch(calc, frames, charge_gradient=True, cell_gradient=True)
    with pytest.raises(ValueError, match="follow_cells=True"):
        fixed(cells=good)
    with pytest.raises(ValueError, match="follow_cells=True"):
        fixed.update_cells()
    assert fixed.mesh_matches(good) == [True, True, True]
    want = snapshot(fixed())
    batch = tpa.GraphedFrameBatch(calc, frames, energy_log=4, **FLAGS)
    first = snapshot(batch())
    check_same(first, want, range(3), dtype, "follow_cells at a fixed cell vs a batch without the keyword")
    kept = batch.cells.clone()
    wrong = [torch.stack(good)[:2], torch.stack(good).float(), torch.stack(good).cpu(), torch.stack(good).reshape(3, 9), good[:2],
             good + good[:1], [good[0], good[1].float(), good[2]], [good[0], good[1].cpu(), good[2]], [good[0], good[1][:2], good[2]],
             [good[0], None, good[2]]]
    moved = [f[2] + 0.5 for f in frames]
    for cells in wrong:
        with pytest.raises(ValueError, match="`cells` must"):
            batch(moved, cells=cells)  # (refused before the positions are copied)
    assert torch.equal(batch.cells, kept)
    again = snapshot(batch())
    check_same(again, first, range(3), dtype, "after refused calls")
    torch.cuda.synchronize()
    assert batch.energy_log.count() == 2  # one entry per call that replayed; calls with `cells=` count too
    st = strain(bx)
    new = [t(c, dtype) for c, _ in st]
    by_keyword = snapshot(batch([t(p, dtype) for _, p in st], cells=new))
    assert batch.energy_log.count() == 3
    batch(cells=good)
    batch.cells.copy_(torch.stack(new))
    batch.update_cells()
    by_update = snapshot(batch())
    assert batch.energy_log.count() == 5
    for k in range(3):
        assert max(errors(by_update, by_keyword, k)[:3]) <= tight_of(dtype)
    E = batch.energies.double().cpu().numpy()
    assert np.array_equal(batch.energy_log.values[0].cpu().numpy(), E)  # (capacity 4: the fifth entry wrapped to slot 0)
