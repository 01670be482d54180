"""``GraphedFrameBatch(charge_gradient=True, cell_gradient=True)``: E, F, dE/dq and dE/dcell of every frame of a batch from one
replay (``mipme_frames_table_contract`` / ``mipme_frames_step``: the CELL instantiations of the batched pair sum, the x stage's
store of w per frame, one launch of cell riders (riders x frames), the gather tail's grad_q / rpart, one finalize launch).

Against the oracle (oracle/pme_numpy.py) with the project's contract tolerances -- fp64 <= 1e-9, fp32 <= 2e-4 of the largest
component -- and against one ``GraphedEnergyForces`` per frame.  Shapes: three frames of 216 / 343 / 125 jittered-lattice atoms in
different triclinic cells, a cutoff of 5.5 (pairs cross the cell boundary: the pair part of dE/dcell comes from those alone), one
calculator whose mesh spacing gives every frame a 32^3 mesh -- more than one row block per frame (32 rows each), frames that end
inside a block, and a grid sized by the largest frame."""

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

DEV = "cuda"
RC, SM = 5.5, 1.1
KINDS = {"p3m5-coulomb": ("P3M", 5, 1), "pme4-coulomb": ("PME", 4, 1), "p3m5-r6": ("P3M", 5, 6)}


def lattice_box(seed, sides, tilt, a=2.3):
    """Jittered lattice of sides[0] x sides[1] x sides[2] atoms (spacing a) in a triclinic cell; neutral normal charges."""
    rng = np.random.default_rng(seed)
    sides = np.asarray(sides)
    g = [(np.arange(n) + 0.5) / n for n in sides]
    frac = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    cell = np.diag(sides * a).astype(float) + tilt * np.array([[0.0, 0.0, 0.0], [0.8, 0.0, 0.0], [-0.5, 0.7, 0.0]])
    pos = frac @ cell + rng.uniform(-0.35, 0.35, frac.shape)
    q = rng.normal(size=(len(pos), 1))
    q -= q.mean()
    return pos, cell, q


def oracle_contract(spec, scheme, order, h, q, cell, pos, pairs, S, full):
    """E, dE/dr, dE/dq, dE/dcell of E = sum q V."""
    dist, _ = O.pair_distances(pos, cell, pairs, S)
    V, cache = O.forward(spec, "P3M" if scheme == "P3M" else "Lagrange", order, h, q, cell, pos, pairs, dist, full_list=full,
                         return_cache=True)
    gr = O.backward(cache, q)
    gpos, gcell_pair = O.pair_distances_backward(pos, cell, pairs, S, gr["dist"])
    return float((q * V).sum()), gpos + gr["positions"], gr["charges"] + V, gr["cell"] + gcell_pair


def make_calc(kind, h, full, dtype):
    scheme, order, expo = KINDS[kind]
    pot = tpa.CoulombPotential(smearing=SM) if expo == 1 else tpa.InversePowerLawPotential(exponent=6, smearing=SM)
    Calc = tpa.P3MCalculator if scheme == "P3M" else tpa.PMECalculator
    return Calc(pot, mesh_spacing=h, interpolation_nodes=order, full_neighbor_list=full).to(dtype)


_BOXES = {}


def boxes(kind, full, layout="cubes"):
    """The frames of a case as numpy arrays, with the oracle's answers for them and for the positions moved by +0.02: computed
    once per (kind, list) and shared by the dtypes and the tests."""
    key = (kind, full, layout)
    if key not in _BOXES:
        scheme, order, expo = KINDS[kind]
        # "cubes": 216, 343, 125 atoms, 32^3 at h = 1.1;  "slabs": 250 and 324 atoms, 64 x 64 x 128 at h = 0.55
        shapes = [((6, 6, 6), 1.0), ((7, 7, 7), 0.6), ((5, 5, 5), -0.8)] if layout == "cubes" else [((5, 5, 10), 1.0), ((6, 6, 9), -0.7)]
        h = 1.1 if layout == "cubes" else 0.55
        spec = O.PotentialSpec("coulomb" if expo == 1 else "ipl", expo, SM, 1.0)
        out = []
        for k, (sides, tilt) in enumerate(shapes):
            pos, cell, q = lattice_box(100 + 7 * k + order, sides, tilt)
            if expo == 6:
                q = np.abs(q) + 0.5
            pairs, S, _ = tpa.neighbor_list(pos, cell, RC, full_list=full)
            ref = [oracle_contract(spec, scheme, order, h, q, cell, pos + d, pairs, S, full) for d in (0.0, 0.02)]
            out.append(dict(pos=pos, cell=cell, q=q, pairs=pairs, S=S, ref=ref, ns=tuple(int(n) for n in O.get_ns_mesh(cell, h))))
        _BOXES[key] = (h, out)
    return _BOXES[key]


def frames_of(bx, dtype):
    t = lambda a: torch.tensor(a, device=DEV, dtype=dtype)  # noqa: E731
    return [(t(b["q"]), t(b["cell"]), t(b["pos"]), torch.tensor(b["pairs"], device=DEV), t(b["S"])) for b in bx]


def rel(a, b):
    a = a.detach().cpu().double().numpy()
    return float(np.abs(a - b).max() / np.abs(b).max())


def tol_of(dtype):
    return 1e-9 if dtype == torch.float64 else 2e-4


def check_against_oracle(out, bx, which, tol):
    E, F, dq, dc = out
    torch.cuda.synchronize()
    for k, b in enumerate(bx):
        Eo, gpo, dqo, dco = b["ref"][which]
        errs = (abs(float(E[k]) - Eo) / abs(Eo), rel(-F[k], gpo), rel(dq[k], dqo), rel(dc[k], dco))
        print(f"frame {k}: rel. errors E {errs[0]:.2e}  F {errs[1]:.2e}  dE/dq {errs[2]:.2e}  dE/dcell {errs[3]:.2e}")
        assert max(errs) <= tol, (k, errs)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("full", [False, True], ids=["half", "full"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_batch_contract_against_oracle_and_single_frame_steps(kind, full, dtype):
    """Two replays, a third after every position moved by +0.02 in place: each frame's E, -F, dE/dq, dE/dcell against the oracle;
    then against one GraphedEnergyForces(charge_gradient=True, cell_gradient=True) per frame; the plane route of the spread."""
    h, bx = boxes(kind, full)
    assert all(b["ns"] == (32, 32, 32) for b in bx), [b["ns"] for b in bx]
    calc = make_calc(kind, h, full, dtype)
    frames = frames_of(bx, dtype)
    batch = tpa.GraphedFrameBatch(calc, frames, charge_gradient=True, cell_gradient=True)
    assert batch.ns == (32, 32, 32)
    assert _lib.load().mipme_last_cosched_kernel() == b"frames_plane_rows_kernel"
    tol = tol_of(dtype)
    for _ in range(2):
        out = batch()
        assert len(out) == 4 and out[2] is batch.charge_grads and out[3] is batch.cell_grads
        assert out[3].shape == (3, 3, 3) and [tuple(g.shape) for g in out[2]] == [(216, 1), (343, 1), (125, 1)]
        check_against_oracle(out, bx, 0, tol)
    moved = [f[2] + 0.02 for f in frames]
    check_against_oracle(batch(moved), bx, 1, tol)
    # ... and the single-frame step of every frame (E, F, dE/dq within test_frames_in_one_launch's bound, dE/dcell within the
    # contract's)
    tight = 1e-11 if dtype == torch.float64 else 2e-5
    E, F, dq, dc = batch()
    torch.cuda.synchronize()
    for k, f in enumerate(frames):
        single = tpa.GraphedEnergyForces(calc, *f, charge_gradient=True, cell_gradient=True)
        e1, f1, q1, c1 = single(moved[k])
        torch.cuda.synchronize()
        errs = (abs(float(E[k]) - float(e1)) / abs(float(e1)), rel(F[k], f1.cpu().double().numpy()),
                rel(dq[k], q1.cpu().double().numpy()), rel(dc[k], c1.cpu().double().numpy()))
        print(f"frame {k} vs single-frame step: E {errs[0]:.2e}  F {errs[1]:.2e}  dE/dq {errs[2]:.2e}  dE/dcell {errs[3]:.2e}")
        assert max(errs[:3]) <= tight and errs[3] <= tol, (k, errs)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_batch_of_one_frame(dtype):
    h, bx = boxes("p3m5-coulomb", False)
    calc = make_calc("p3m5-coulomb", h, False, dtype)
    frames = frames_of(bx[1:2], dtype)
    batch = tpa.GraphedFrameBatch(calc, frames, charge_gradient=True, cell_gradient=True)
    out = batch()
    assert out[3].shape == (1, 3, 3)
    check_against_oracle(out, bx[1:2], 0, tol_of(dtype))
    single = tpa.GraphedEnergyForces(calc, *frames[0], charge_gradient=True, cell_gradient=True)
    e1, f1, q1, c1 = single()
    torch.cuda.synchronize()
    tight = 1e-11 if dtype == torch.float64 else 2e-5
    assert abs(float(out[0][0]) - float(e1)) <= tight * abs(float(e1))
    assert rel(out[1][0], f1.cpu().double().numpy()) <= tight and rel(out[2][0], q1.cpu().double().numpy()) <= tight
    assert rel(out[3][0], c1.cpu().double().numpy()) <= tol_of(dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["p3m5-coulomb", "p3m5-r6"])
def test_brick_route(kind, dtype):
    """The brick route of the batched spread (frames_spread_rows_kernel).  The frames were chosen by their mesh: at h = 0.55 the
    two slabs of 5 x 5 x 10 and 6 x 6 x 9 lattice sites give 64 x 64 x 128, whose (y,z) planes -- 64 x 128 points -- exceed the LDS
    a plane workgroup of the co-scheduled launch may use in either precision, so that the batch keeps the bricks (1024 of them,
    the most the frames path takes); which route ran is asked of the library after the evaluation."""
    h, bx = boxes(kind, False, "slabs")
    assert all(b["ns"] == (64, 64, 128) for b in bx), [b["ns"] for b in bx]
    calc = make_calc(kind, h, False, dtype)
    batch = tpa.GraphedFrameBatch(calc, frames_of(bx, dtype), charge_gradient=True, cell_gradient=True)
    assert _lib.load().mipme_last_cosched_kernel() == b"frames_spread_rows_kernel"
    check_against_oracle(batch(), bx, 0, tol_of(dtype))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_flag_combinations_and_the_energy_log(dtype):
    h, bx = boxes("p3m5-coulomb", False)
    calc = make_calc("p3m5-coulomb", h, False, dtype)
    frames = frames_of(bx, dtype)
    tol = tol_of(dtype)
    lib = _lib.load()
    # flags off: a 2-tuple from the kernels of before
    plain = tpa.GraphedFrameBatch(calc, frames)
    assert lib.mipme_last_cosched_kernel() == b"frames_plane_rows_kernel"
    out = plain()
    assert len(out) == 2 and plain.charge_grads is None and plain.cell_grads is None
    torch.cuda.synchronize()
    E0 = out[0].cpu().double().numpy().copy()
    for k, b in enumerate(bx):
        assert abs(E0[k] - b["ref"][0][0]) <= tol * abs(b["ref"][0][0]) and rel(-out[1][k], b["ref"][0][1]) <= tol
    # single flags: the order of the returned tuple
    only_q = tpa.GraphedFrameBatch(calc, frames, charge_gradient=True)
    out = only_q()
    torch.cuda.synchronize()
    assert len(out) == 3 and isinstance(out[2], list) and only_q.cell_grads is None
    assert all(rel(out[2][k], b["ref"][0][2]) <= tol for k, b in enumerate(bx))
    only_c = tpa.GraphedFrameBatch(calc, frames, cell_gradient=True)
    out = only_c()
    torch.cuda.synchronize()
    assert len(out) == 3 and out[2].shape == (3, 3, 3) and only_c.charge_grads is None
    assert all(rel(out[2][k], b["ref"][0][3]) <= tol for k, b in enumerate(bx))
    # the energy log rides on the same gather tail
    logged = tpa.GraphedFrameBatch(calc, frames, charge_gradient=True, cell_gradient=True, energy_log=4)
    for _ in range(3):
        out = logged()
    torch.cuda.synchronize()
    assert logged.energy_log.count() == 3
    check_against_oracle(out, bx, 0, tol)
    E = logged.energies.double().cpu().numpy()
    for row in logged.energy_log.values[:3].cpu().numpy():
        assert np.array_equal(row, E)


def test_refusals_on_gpu_tensors(monkeypatch):
    h, bx = boxes("p3m5-coulomb", False)
    calc = make_calc("p3m5-coulomb", h, False, torch.float32)
    frames = frames_of(bx, torch.float32)
    with pytest.raises(ValueError, match="`cell_gradient` and `store_distances` exclude each other"):
        tpa.GraphedFrameBatch(calc, frames, cell_gradient=True, store_distances=True)
    # frames whose pair entries have no 4-byte form (here: the format switched off, as for shifts beyond its range)
    monkeypatch.setattr(ops, "COMPACT_ENTRIES", False)
    fresh = [(f[0], f[1], f[2], f[3].clone(), f[4].clone()) for f in frames]  # (new list tensors: no cached 4-byte entries)
    with pytest.raises(ValueError, match="`cell_gradient` needs 4-byte pair entries in every frame"):
        tpa.GraphedFrameBatch(calc, fresh, cell_gradient=True)
    # the charges alone ride on the gather tail, whatever the entry format
    out = tpa.GraphedFrameBatch(calc, fresh, charge_gradient=True)()
    torch.cuda.synchronize()
    assert len(out) == 3 and all(rel(out[2][k], b["ref"][0][2]) <= 2e-4 for k, b in enumerate(bx))
