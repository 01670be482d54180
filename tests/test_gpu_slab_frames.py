"""GPU tests of 2-D periodic (slab) frames in ``GraphedFrameBatch(..., periodic=, slab_correction=True)``, against the reference's
values: ``tests/golden/slab_step.npz`` (the single-frame cases of ``tests/test_gpu_slab_step.py``, here side by side in batches)
and ``tests/golden/slab_frames.npz`` (``make_slab_frames_golden.py``: three slab frames of axes 0, 1, 2 -- one triclinic -- and a
fully periodic frame on one 32^3 mesh).

Sizes: 32 x 32 x 64 or 32^3 meshes (128 / 64 bricks) and 216-400 atoms per frame, the smallest with bricks and power-of-two
planes.  Tolerances, both the project's own (``tests/test_gpu_slab_step.py``): fp64 1e-9 relative L2; fp32 max error <= 5 x the
reference's own fp32-against-fp64 spread of that quantity (stored in the goldens, checked there to be non-zero) + 4 eps32 x scale.
"""

import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = np.load(os.path.join(ROOT, "tests", "golden", "slab_step.npz"))
MIXED = np.load(os.path.join(ROOT, "tests", "golden", "slab_frames.npz"))
MIXED_NAMES = [str(n) for n in MIXED["names"]]
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
EPS32 = float(np.finfo(np.float32).eps)

#: frames of slab_step.npz that share a mesh and a calculator
BATCHES = {
    "ax2": ["ortho_ax2_neutral", "ortho_ax2_charged", "lumpy_ax2_charged"],  # (lumpy: overflow atoms, empty bricks, brick 0 too)
    "ax0": ["ortho_ax0_neutral", "ortho_ax0_charged"],
    "ax1": ["ortho_ax1_neutral", "ortho_ax1_charged"],
    "tric": ["tric_ax2_charged"],
    "pme": ["ortho_ax2_charged_pme"],
}


def frame(gold, name, dtype):
    """(charges, cell, positions, pairs, shifts) of a golden's case and its ``periodic`` triple."""
    t = lambda key, dt=dtype: torch.tensor(gold[f"{name}_{key}"], dtype=dt, device=DEV)  # noqa: E731
    axis = int(gold[f"{name}_axis"])
    return (t("charges"), t("cell"), t("positions"), t("pairs", torch.int64), t("shifts")), tuple(d != axis for d in range(3))


def calculator(gold, name):
    pot = tpa.CoulombPotential(smearing=float(gold["smearing"]))
    if f"{name}_method" in gold.files and str(gold[f"{name}_method"]) == "pme":
        cls = tpa.PMECalculator
    else:
        cls = tpa.P3MCalculator
    nodes = int(gold[f"{name}_nodes"]) if f"{name}_nodes" in gold.files else int(gold["nodes"])
    return cls(pot, mesh_spacing=float(gold["mesh_spacing"]), interpolation_nodes=nodes).to(DEV)


def make_batch(gold, names, dtype, slab=True, **kw):
    frames, periodic = zip(*(frame(gold, n, dtype) for n in names))
    if slab:
        kw = dict(dict(periodic=list(periodic), slab_correction=True), **kw)
    return tpa.GraphedFrameBatch(calculator(gold, names[0]), list(frames), **kw), frames


def rell2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def results(out, k):
    """Frame k of what a batch call returns, named as in the goldens (gpos = -forces); copies."""
    res = dict(E=out[0][k].reshape(1), gpos=-out[1][k])
    if len(out) == 4:
        res.update(gq=out[2][k], gcell=out[3][k])
    return {key: v.detach().double().cpu().numpy() for key, v in res.items()}


def check(got, want, spread, dtype, what):
    """got / want: {key: array}; spread(key): the reference's fp32 spread of that quantity."""
    for key, g in got.items():
        w = np.asarray(want[key], dtype=np.float64).reshape(g.shape)
        if dtype == F64:
            err, tol = rell2(g, w), 1e-9
        else:
            err, tol = np.abs(g - w).max(), 5 * spread(key) + 4 * EPS32 * np.abs(w).max()
        print(f"{what} {key} {dtype}: error {err:.3e} (bound {tol:.3e})")
        assert err <= tol, f"{what} {key} {dtype}: error {err:.3e} > {tol:.3e}"


def check_golden(out, gold, names, dtype, what=""):
    for k, name in enumerate(names):
        got = results(out, k)
        check(got, {key: gold[f"{name}_{key}_f64"] for key in got}, lambda key, n=name: float(gold[f"{n}_spread_{key}"]), dtype,
              f"{what}frame {k} {name}")


# ---- 1, 2: the single-frame goldens side by side ----------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("group", list(BATCHES))
def test_batches_against_the_reference_with_all_gradients(group, dtype):
    names = BATCHES[group]
    batch, _ = make_batch(STEP, names, dtype, charge_gradient=True, cell_gradient=True)
    assert batch.slab_axes == [int(STEP[f"{n}_axis"]) for n in names]
    check_golden(batch(), STEP, names, dtype)


@DTYPES
@pytest.mark.parametrize("group", list(BATCHES))
def test_batches_against_the_reference_energy_and_forces_only(group, dtype):
    """The plain gather (no cell sums) and no finalize launch; one batch also stores the distances."""
    names = BATCHES[group]
    store = group == "ax0"
    batch, frames = make_batch(STEP, names, dtype, store_distances=store)
    out = batch()
    assert len(out) == 2
    check_golden(out, STEP, names, dtype)
    if store:
        for k, (_, cell, pos, pairs, shifts) in enumerate(frames):
            assert batch.distances[k] is not None
            want = torch.linalg.norm(pos[pairs[:, 1]] - pos[pairs[:, 0]] + shifts @ cell, dim=1)
            # (a distance is a difference of coordinates: its rounding is that of the coordinates, a few eps x their size)
            scale = max(float(pos.abs().max()), float(cell.abs().max()))
            assert float((batch.distances[k] - want).abs().max()) <= 16 * torch.finfo(dtype).eps * scale


# ---- 3: mixed axes and a fully periodic frame in one batch, in both frame orders -------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("order", ["golden_order", "reversed"])
def test_mixed_axes_and_a_fully_periodic_frame(order, dtype):
    names = MIXED_NAMES if order == "golden_order" else MIXED_NAMES[::-1]
    axes = [int(MIXED[f"{n}_axis"]) for n in names]
    assert sorted(axes) == [-1, 0, 1, 2]
    batch, _ = make_batch(MIXED, names, dtype, charge_gradient=True, cell_gradient=True)
    assert batch.slab_axes == [None if a < 0 else a for a in axes]
    check_golden(batch(), MIXED, names, dtype, what=f"{order} ")


# ---- 4: replays ---------------------------------------------------------------------------------------------------------------------
def eager(calc, fr, periodic, pos):
    """One eager evaluation of a frame with all gradients (the slab term by launches of its own when ops.TAIL_FUSION is off)."""
    q, cell, _, pairs, shifts = fr
    q = q.detach().clone().requires_grad_(True)
    cell = cell.detach().clone().requires_grad_(True)
    p = pos.detach().clone().requires_grad_(True)
    per = None if all(periodic) else torch.tensor(periodic, device=DEV)
    V = calc(q, cell, p, pairs, tpa.pair_distances(p, pairs, cell, shifts, deferred="virtual"), periodic=per)
    E = tpa.weighted_sum(V, q)
    E.backward()
    return dict(E=E.detach().reshape(1), gpos=p.grad, gq=q.grad, gcell=cell.grad), V.grad_fn


@DTYPES
def test_replay_after_the_atoms_moved(dtype, monkeypatch):
    names = MIXED_NAMES
    batch, frames = make_batch(MIXED, names, dtype, charge_gradient=True, cell_gradient=True)
    first = [results(batch(), k) for k in range(len(names))]
    rng = np.random.default_rng(11)
    moved = [f[2] + torch.tensor(1e-4 * rng.uniform(-1, 1, f[2].shape), dtype=dtype, device=DEV) for f in frames]
    out = batch(moved)
    got = [results(out, k) for k in range(len(names))]
    monkeypatch.setattr(ops, "TAIL_FUSION", False)
    calc = calculator(MIXED, names[0])
    for k, name in enumerate(names):
        periodic = tuple(d != int(MIXED[f"{name}_axis"]) for d in range(3))
        want, node = eager(calc, frames[k], periodic, moved[k])
        assert node.tail is None and not node.slab_in_tail
        want = {key: v.detach().double().cpu().numpy() for key, v in want.items()}
        check(got[k], want, lambda key, n=name: float(MIXED[f"{n}_spread_{key}"]), dtype, f"moved frame {k} {name}")
        if dtype == F64:  # (the replay did see the new positions)
            assert np.abs(got[k]["gpos"] - first[k]["gpos"]).max() > 1e-6
    # back to the first positions: the moments' work words and tickets were left clean by the replays before
    out = batch([f[2] for f in frames])
    for k, name in enumerate(names):
        again = results(out, k)
        if dtype == F64:
            for key in again:
                err = rell2(again[key], first[k][key])
                print(f"replay with the first positions, frame {k} {key}: {err:.3e}")
                assert err <= 1e-12
        else:
            check(again, first[k], lambda key, n=name: float(MIXED[f"{n}_spread_{key}"]), dtype, f"first positions again, frame {k}")


# ---- 5: fully periodic frames ---------------------------------------------------------------------------------------------------------
@DTYPES
def test_fully_periodic_frames_are_what_they_were(dtype):
    lib = _lib.load()
    name = "full_charged"
    spread = lambda key: float(MIXED[f"{name}_spread_{key}"])  # noqa: E731
    kw = dict(charge_gradient=True, cell_gradient=True)
    plain, _ = make_batch(MIXED, [name, name], dtype, slab=False, **kw)
    kernel_plain = lib.mipme_last_cosched_kernel().decode()
    want = [results(plain(), k) for k in range(2)]
    # every frame fully periodic: nothing of the slab term is built or launched
    batch, _ = make_batch(MIXED, [name, name], dtype, periodic=(True, True, True), slab_correction=True, **kw)
    assert lib.mipme_last_cosched_kernel().decode() == kernel_plain
    assert batch.slab_axes is None and batch._slab is None and batch._slab_work is None
    out = batch()
    for k in range(2):
        check(results(out, k), want[k], spread, dtype, f"all periodic, frame {k}")
    # a fully periodic frame next to slab frames: the launches compiled with the term add nothing to it
    mixed, _ = make_batch(MIXED, MIXED_NAMES, dtype, **kw)
    check(results(mixed(), MIXED_NAMES.index(name)), want[0], spread, dtype, "the fully periodic frame of the mixed batch")


# ---- 6: the energy log ----------------------------------------------------------------------------------------------------------------
def test_energy_log_holds_the_energies_of_the_replays():
    names = BATCHES["ax1"]
    batch, frames = make_batch(STEP, names, F32, energy_log=4)
    rng = np.random.default_rng(5)
    seen = []
    for it in range(3):
        pos = [f[2] + torch.tensor(1e-3 * it * rng.uniform(-1, 1, f[2].shape), dtype=F32, device=DEV) for f in frames]
        seen.append(batch(pos)[0].double().cpu().numpy().copy())
    torch.cuda.synchronize()
    assert batch.energy_log.count() == 3
    assert np.array_equal(batch.energy_log.values[:3].cpu().numpy(), np.stack(seen))
    assert not np.array_equal(seen[0], seen[2])
    check_golden(batch([f[2] for f in frames]), STEP, names, F32, what="logged batch ")


# ---- 7: the stored field carries the term ----------------------------------------------------------------------------------------------
def test_backward_with_another_seed_uses_the_stored_field():
    names = MIXED_NAMES
    batch, _ = make_batch(MIXED, names, F64)
    forces = [f.clone() for f in batch()[1]]
    batch._launch_backward(torch.full((len(names),), -2.0, dtype=F64, device=DEV))
    torch.cuda.synchronize()
    for k, name in enumerate(names):
        err = rell2(batch._grad_pos[k].cpu().numpy(), 2.0 * forces[k].cpu().numpy())
        print(f"frame {k} {name}: seed -2 against twice the forces {err:.3e}")
        assert err <= 1e-12
    # (and the forces are the reference's, slab term included: the field of the term is not small against them)
    check_golden((batch.energies, forces), MIXED, names, F64)


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    names = BATCHES["ax0"]
    frames, periodic = zip(*(frame(STEP, n, F64) for n in names))
    frames = list(frames)
    calc = calculator(STEP, names[0])
    with pytest.raises(ValueError, match="`slab_correction` needs `periodic`"):
        tpa.GraphedFrameBatch(calc, frames, slab_correction=True)
    with pytest.raises(ValueError, match="`periodic` only selects the frames and axes of `slab_correction=True`"):
        tpa.GraphedFrameBatch(calc, frames, periodic=periodic[0])
    with pytest.raises(ValueError, match=r"frame 1: `slab_correction` needs exactly two periodic axes \(or three"):
        tpa.GraphedFrameBatch(calc, frames, periodic=[periodic[0], (True, False, False)], slab_correction=True)
    with pytest.raises(ValueError, match="one triple or one triple per frame"):
        tpa.GraphedFrameBatch(calc, frames, periodic=[periodic[0]], slab_correction=True)
    smearing = float(STEP["smearing"])
    r6 = tpa.P3MCalculator(tpa.InversePowerLawPotential(exponent=6, smearing=smearing), mesh_spacing=float(STEP["mesh_spacing"]),
                           interpolation_nodes=5).to(DEV)
    with pytest.raises(ValueError, match="`slab_correction`: the slab term exists for 1/r only"):
        tpa.GraphedFrameBatch(r6, frames, periodic=periodic[0], slab_correction=True)
    with pytest.raises(ValueError, match="`slab_correction` belongs to the mesh part: the potential needs a smearing"):
        tpa.GraphedFrameBatch(tpa.Calculator(tpa.CoulombPotential()), frames, periodic=periodic[0], slab_correction=True)
    # exponent 1 written as an inverse power law is 1/r
    r1 = tpa.P3MCalculator(tpa.InversePowerLawPotential(exponent=1, smearing=smearing), mesh_spacing=float(STEP["mesh_spacing"]),
                           interpolation_nodes=5).to(DEV)
    batch = tpa.GraphedFrameBatch(r1, frames, periodic=list(periodic), slab_correction=True)
    check_golden(batch(), STEP, names, F64, what="exponent 1 ")
