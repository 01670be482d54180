"""GraphedEwaldBatch on the GPU (csrc/ewald_batch.hip): five frames of 1 to 300 atoms, each with its own cell and k grid, served
by ONE captured graph -- against the reference's own outputs at two cells per frame (tests/golden/ewald_batch.npz), to the bit
against the same frames in another order, alone and replayed; isolation of a frame from what happens to another one; the status
words; the input forms; new lists; the refusals that need a device."""

import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "ewald_batch.npz"))
STEP = np.load(os.path.join(HERE, "golden", "ewald_step.npz"))
DTYPES = [torch.float64, torch.float32]
EPS32 = float(np.finfo(np.float32).eps)
LAM = float(STEP["lr_wavelength"])
STRAIN = np.eye(3) + STEP["strain"]
CALCS = {"C1": (lambda: tpa.CoulombPotential(smearing=1.0), False),
         "C2": (lambda: tpa.InversePowerLawPotential(6, smearing=0.9), True)}
ALL = (0, 1, 2, 3, 4)


def test_class_is_exported():
    assert hasattr(tpa, "GraphedEwaldBatch")
    assert "GraphedEwaldBatch" in tpa.__all__


def _t(x, dtype):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=dtype, device=DEV)


def _check(res, want, spread, abs_e, dtype, what):
    """The rule of tests/test_gpu_ewald_step.py::_check.  fp64: 1e-10 of the largest wanted value.  fp32: 5x the spread of the
    reference's own fp32 run + 4 eps32 of the scale; the scale of the scalar E is sum_a |q_a V_a| -- the difference of two scalars
    can be accidentally tiny, and E itself small next to its terms."""
    for key in res:
        scale = np.abs(want[key]).max()
        err = np.abs(res[key] - want[key]).max()
        if dtype == torch.float64:
            tol = 1e-10 * scale
        else:
            tol = 5 * spread[key] + 4 * EPS32 * (abs_e if key == "E" else scale)
        print(f"{what} {key} {dtype}: max error {err:.3e}, bound {tol:.3e}, scale {scale:.3e}")
        assert err <= tol, f"{what} {key} {dtype}: max error {err:.3e} > {tol:.3e} (scale {scale:.3e})"


def _calc(cname):
    make, full = CALCS[cname]
    return tpa.EwaldCalculator(make(), lr_wavelength=LAM, full_neighbor_list=full)


def _system(n, full):
    """(charges, positions, cell, pairs, shifts) of frame n at its construction cell, as the golden script builds them."""
    kind = "full" if full else "half"
    if n < 3:
        return (GOLD[f"f{n}_charges"], GOLD[f"f{n}_positions"], GOLD[f"f{n}_cell"],
                GOLD[f"f{n}_pairs_{kind}"].astype(np.int64).reshape(-1, 2), GOLD[f"f{n}_shifts_{kind}"].astype(np.int64).reshape(-1, 3))
    if n == 3:
        v = "ipl6" if full else "half"
        return (STEP["tric_net_charges"], STEP["tric_positions"], STEP["tric_cell"], STEP[f"tric_{v}_pairs"].astype(np.int64),
                STEP[f"tric_{v}_shifts"].astype(np.int64))
    pairs, shifts = STEP["big_pairs"].astype(np.int64), STEP["big_shifts"].astype(np.int64)
    if full:
        pairs, shifts = np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])
    return STEP["big_half_charges"], STEP["big_positions"], STEP["big_cell"], pairs, shifts


def _frame(n, full, dtype):
    q, pos, cell, pairs, shifts = _system(n, full)
    return (_t(q, dtype), _t(cell, dtype), _t(pos, dtype), torch.tensor(pairs, device=DEV), _t(shifts, dtype))


def _batch(cname, dtype, which=ALL, cell_gradient=True):
    full = CALCS[cname][1]
    return tpa.GraphedEwaldBatch(_calc(cname), [_frame(n, full, dtype) for n in which], cell_gradient=cell_gradient)


def _single(cname, dtype, n, lists=None):
    q, cell, pos, idx, sh = _frame(n, CALCS[cname][1], dtype)
    if lists is not None:
        idx, sh = lists
    return tpa.GraphedEwaldStep(_calc(cname), q, cell, pos, idx, sh, cell_gradient=True)


def _results(batch, *args, **kw):
    """Per frame {"E", "F", "gq", "gcell"} as float64 arrays."""
    out = batch(*args, **kw)
    torch.cuda.synchronize()
    host = lambda t: t.detach().double().cpu().numpy().copy()  # noqa: E731
    res = []
    for f in range(batch.n_frames):
        r = {"E": host(out[0][f]), "F": host(out[1][f]), "gq": host(out[2][f])}
        if len(out) > 3:
            r["gcell"] = host(out[3][f])
        res.append(r)
    return res


def _step_results(step, *args, **kw):
    out = step(*args, **kw)
    torch.cuda.synchronize()
    return {k: v.detach().double().cpu().numpy().copy() for k, v in zip(("E", "F", "gq", "gcell"), out)}


def _golden(cname, n, ctag):
    g = lambda k, tag: GOLD[f"{cname}_f{n}_{k}_{ctag}_{tag}"].astype(np.float64)  # noqa: E731
    want = {"E": np.float64(g("E", "f64")), "F": -g("gpos", "f64"), "gq": g("gq", "f64"), "gcell": g("gcell", "f64")}
    f32 = {"E": np.float64(g("E", "f32")), "F": -g("gpos", "f32"), "gq": g("gq", "f32"), "gcell": g("gcell", "f32")}
    return want, {k: np.abs(f32[k] - want[k]).max() for k in want}, float(GOLD[f"{cname}_f{n}_absE_{ctag}"])


def _bits(batch, *args, **kw):
    """The outputs of a call, per frame, as clones: [[E_f, F_f, gq_f, gcell_f, status_f]]."""
    out = batch(*args, **kw)
    torch.cuda.synchronize()
    return [[o[f].clone() for o in out] + [batch.status[f].clone()] for f in range(batch.n_frames)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _status(batch):
    return [int(s) for s in batch.status.cpu()]


# ---- against the reference: all five frames, both cells, one graph ----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
def test_five_frames_match_the_reference_and_follow_their_cells(cname, dtype):
    full = CALCS[cname][1]
    batch = _batch(cname, dtype)
    assert batch.ns == [(1, 1, 1), tuple(batch.ns[1]), (4, 9, 6), (8, 7, 9), (16, 16, 16)]
    assert batch.n_k[0] == 0 and batch.n_k[4] >= 2048 and batch.atom_ptr == [0, 1, 3, 20, 44, 344]
    graph = batch.graph
    res = _results(batch)
    for n in ALL:
        _check(res[n], *_golden(cname, n, "c0"), dtype, f"{cname} f{n} cell0")
    assert _status(batch) == [0] * 5
    # ONE call: frames 0, 2 and 4 move to the strained cell (positions and cell), frames 1 and 3 stay
    moved = (0, 2, 4)
    pos, cells = [], []
    for n in ALL:
        _, p, c, _, _ = _system(n, full)
        pos.append(_t(p @ STRAIN if n in moved else p, dtype))
        cells.append(_t(c @ STRAIN if n in moved else c, dtype))
    res = _results(batch, positions=pos, cells=cells)
    for n in ALL:
        ctag = "c1" if n in moved else "c0"
        _check(res[n], *_golden(cname, n, ctag), dtype, f"{cname} f{n} {ctag} (mixed call)")
    assert _status(batch) == [0] * 5 and batch.graph is graph
    assert batch.kgrid_matches(cells) == [True] * 5
    # without the cell gradient: three outputs, the same bounds
    plain = _batch(cname, dtype, cell_gradient=False)
    out = plain()
    assert len(out) == 3 and out[0].shape == (5,) and plain.cell_grads is None
    res = _results(plain)
    for n in ALL:
        want, spread, abs_e = _golden(cname, n, "c0")
        want.pop("gcell")
        _check(res[n], want, spread, abs_e, dtype, f"{cname} f{n} without the cell gradient")


def test_output_layout():
    batch = _batch("C1", torch.float32)
    E, F, gq, gcell = batch()
    assert E.shape == (5,) and gcell.shape == (5, 3, 3) and batch.status.shape == (5,) and batch.status.dtype == torch.int32
    assert batch.forces_flat.shape == (344, 3) and batch.charge_grads_flat.shape == (344, 1)
    for f, (a, b) in enumerate(zip(batch.atom_ptr[:-1], batch.atom_ptr[1:])):
        assert F[f].shape == (b - a, 3) and gq[f].shape == (b - a, 1)
        assert F[f].data_ptr() == batch.forces_flat[a:b].data_ptr() and gq[f].data_ptr() == batch.charge_grads_flat[a:b].data_ptr()


# ---- a frame's bits depend on its own inputs only -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
def test_independence_to_the_bit(cname, dtype):
    batch = _batch(cname, dtype)
    first = _bits(batch)
    assert all(_same(a, b) for a, b in zip(first, _bits(batch)))  # equal inputs, equal bits
    backwards = _bits(_batch(cname, dtype, which=ALL[::-1]))
    for n in ALL:
        assert _same(first[n], backwards[4 - n]), f"frame {n} in the reversed batch"
        alone = _bits(_batch(cname, dtype, which=(n,)))
        assert _same(first[n], alone[0]), f"frame {n} alone"


# ---- the batch of one frame and the single step of that frame run the same bodies (csrc/ewald_step_bodies.h) --------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
@pytest.mark.parametrize("n", ALL)
def test_a_batch_of_one_frame_equals_the_single_step_to_the_bit(n, cname, dtype):
    """E, F, dE/dq, dE/dcell and status, at the construction cell and -- from the same two graphs -- at the strained cell with
    the strained positions."""
    step, batch = _single(cname, dtype, n), _batch(cname, dtype, which=(n,))
    graphs = (step.graph, batch.graph)
    _, p, c, _, _ = _system(n, CALCS[cname][1])
    for ctag, m in (("c0", np.eye(3)), ("c1", STRAIN)):
        pos, cell = _t(p @ m, dtype), _t(c @ m, dtype)
        one = [o.clone() for o in step(positions=pos, cell=cell)] + [step.status[0].clone()]
        got = _bits(batch, positions=[pos], cells=[cell])[0]
        torch.cuda.synchronize()
        for key, a, b in zip(("E", "F", "gq", "gcell", "status"), one, got):
            assert a.shape == b.shape and torch.equal(a, b), f"{cname} f{n} {ctag} {dtype}: {key} of the step and of the batch differ"
        assert int(got[4]) == 0
    assert (step.graph, batch.graph) == graphs


# ---- what happens to one frame happens to that frame alone ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_isolation(dtype):
    cname, full = "C1", False
    batch = _batch(cname, dtype)
    graph, first = batch.graph, _bits(batch)
    systems = [_system(n, full) for n in ALL]
    pos0, cells0 = [_t(s[1], dtype) for s in systems], [_t(s[2], dtype) for s in systems]
    # new positions and a new cell for frame 2 only
    pos, cells = list(pos0), list(cells0)
    pos[2], cells[2] = _t(systems[2][1] @ STRAIN, dtype), _t(systems[2][2] @ STRAIN, dtype)
    other = _bits(batch, positions=pos, cells=cells)
    for n in (0, 1, 3, 4):
        assert _same(first[n], other[n]), f"frame {n} while frame 2 moved"
    assert not torch.equal(first[2][0], other[2][0])
    # a singular cell (two equal rows) for frame 1 only
    singular = systems[1][2].copy()
    singular[2] = singular[0]
    cells = list(cells0)
    cells[1] = _t(singular, dtype)
    broken = _bits(batch, positions=pos0, cells=cells)
    assert bool(torch.isnan(broken[1][0])) and bool(torch.isnan(broken[1][3]).all()) and int(broken[1][4]) == 2
    for n in (0, 2, 3, 4):
        assert _same(first[n], broken[n]) and int(broken[n][4]) == 0, f"frame {n} beside a singular cell"
    # the correct cell restores the first results bit for bit
    again = _bits(batch, cells=cells0)
    assert all(_same(a, b) for a, b in zip(first, again)) and batch.graph is graph and _status(batch) == [0] * 5


# ---- status bit 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_status_bit_0_of_one_frame_and_the_energy_of_the_kept_grid(dtype):
    """|a_0| of frame 3 is 9.0, so ceil(|a_0| / 1.25) = 8; stretched by 1.15 it is 9.  The batch keeps the frame's grid and says
    so in status[3] alone.  (The single step's test has no monotonic check of the energy: what the frame returns is what a
    GraphedEwaldStep of the same frame, built at the same cell and fed the stretched one, returns -- the fp64 step is the wanted
    value, the fp32 spread that of the frame's golden cell.)"""
    cname = "C1"
    batch = _batch(cname, dtype)
    systems = [_system(n, False) for n in ALL]
    stretched = systems[3][2].copy()
    stretched[0] *= 1.15
    assert int(np.ceil(np.linalg.norm(stretched[0]) / LAM)) == 9 != batch.ns[3][0]
    cells = [_t(s[2], dtype) for s in systems]
    cells[3] = _t(stretched, dtype)
    assert batch.kgrid_matches(cells) == [True, True, True, False, True]
    res = _results(batch, cells=cells)
    assert _status(batch) == [0, 0, 0, 1, 0] and np.isfinite(res[3]["E"])
    step = _single(cname, torch.float64, 3)
    want = _step_results(step, cell=_t(stretched, torch.float64))
    assert int(step.status.cpu()[0]) == 1
    _, spread, abs_e = _golden(cname, 3, "c0")
    _check(res[3], want, spread, abs_e, dtype, "frame 3 on its kept grid")
    for n in (0, 1, 2, 4):
        _check(res[n], *_golden(cname, n, "c0"), dtype, f"f{n} beside the stretched frame")


# ---- frames without k-vectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["C1", "C2"])
@pytest.mark.parametrize("copies", [1, 2])
def test_a_batch_whose_frames_all_have_no_kvectors(cname, copies, dtype):
    batch = _batch(cname, dtype, which=(0,) * copies)
    assert batch.n_k == [0] * copies and batch.ns == [(1, 1, 1)] * copies
    res = _results(batch)
    for f in range(copies):
        _check(res[f], *_golden(cname, 0, "c0"), dtype, f"{cname} f0 (copy {f} of {copies})")
    _, p, c, _, _ = _system(0, False)
    res = _results(batch, positions=[_t(p @ STRAIN, dtype)] * copies, cells=[_t(c @ STRAIN, dtype)] * copies)
    for f in range(copies):
        _check(res[f], *_golden(cname, 0, "c1"), dtype, f"{cname} f0 strained (copy {f} of {copies})")
    assert _status(batch) == [0] * copies


# ---- input forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_forms_and_new_charges(dtype):
    cname = "C1"
    batch = _batch(cname, dtype)
    graph = batch.graph
    systems = [_system(n, False) for n in ALL]
    pos = [_t(s[1] @ STRAIN, dtype) for s in systems]
    cells = [_t(s[2] @ STRAIN, dtype) for s in systems]
    q = [_t(s[0], dtype) for s in systems]
    as_lists = _bits(batch, positions=pos, charges=q, cells=cells)
    batch(positions=[_t(s[1], dtype) for s in systems], cells=[_t(s[2], dtype) for s in systems])
    flat = _bits(batch, positions=torch.cat(pos), charges=torch.cat(q), cells=torch.stack(cells))
    assert all(_same(a, b) for a, b in zip(as_lists, flat))
    with pytest.raises(ValueError, match="5 per-frame tensors"):
        batch(positions=pos[:4])
    # charges= alone: no second charge set is stored, so frame 3 is held against a GraphedEwaldStep of the same frame
    q2 = [_t(np.random.default_rng(40 + n).normal(size=s[0].shape) + 0.1, dtype) for n, s in enumerate(systems)]
    batch(positions=[_t(s[1], dtype) for s in systems], cells=[_t(s[2], dtype) for s in systems])
    before = _bits(batch)
    res = _results(batch, charges=q2)
    assert batch.graph is graph and not torch.equal(before[3][2], batch.charge_grads[3])
    step = _single(cname, torch.float64, 3)
    want = _step_results(step, charges=q2[3].double())
    _, spread, _ = _golden(cname, 3, "c0")
    abs_e = float(np.abs(0.5 * q2[3].double().cpu().numpy() * want["gq"]).sum())
    _check(res[3], want, spread, abs_e, dtype, "frame 3 with new charges")
    assert all(_same(a, b) for a, b in zip(before, _bits(batch, charges=torch.cat(q))))


# ---- new lists -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_recapture_with_new_lists_and_a_refused_one(dtype):
    cname = "C1"
    batch = _batch(cname, dtype)
    systems = [_system(n, False) for n in ALL]
    lists = [(torch.tensor(s[3], device=DEV), _t(s[4], dtype)) for s in systems]
    graph, pairs, before = batch.graph, batch.pairs, _bits(batch)
    # refused: a shift of 4 in frame 2 -- nothing of the object changes
    bad = list(lists)
    sh = systems[2][4].copy()
    sh[0, 1] = 4
    bad[2] = (lists[2][0], _t(sh, dtype))
    with pytest.raises(ValueError, match=r"frame 2.*integers in \[-3, 3\]"):
        batch.recapture(bad)
    assert batch.graph is graph and batch.pairs is pairs and all(_same(a, b) for a, b in zip(before, _bits(batch)))
    # taken: the half list of f4 at a shorter cutoff
    p4, s4, _ = tpa.neighbor_list(systems[4][1], systems[4][2], 3.0)
    assert 0 < len(p4) < len(systems[4][3])
    new = list(lists)
    new[4] = (torch.tensor(np.asarray(p4, dtype=np.int64), device=DEV), _t(s4, dtype))
    batch.recapture(new)
    assert batch.graph is not graph and batch.pairs[4] is new[4][0]
    after = _bits(batch)
    for n in (0, 1, 2, 3):
        assert _same(before[n], after[n])
    assert not torch.equal(before[4][1], after[4][1])
    res = _results(batch)
    step = _single(cname, torch.float64, 4, lists=(new[4][0], _t(s4, torch.float64)))
    want = _step_results(step)
    _, spread, abs_e = _golden(cname, 4, "c0")
    _check(res[4], want, spread, abs_e, dtype, "frame 4 with the shorter list")


# ---- refusals that need a device -------------------------------------------------------------------------------------------------
def test_constructor_refusals_with_a_device():
    calc = _calc("C1")
    with pytest.raises(ValueError, match="frame 1.*share one dtype.*float32"):
        tpa.GraphedEwaldBatch(calc, [_frame(1, False, torch.float64), _frame(2, False, torch.float32)])
    q, cell, pos, idx, sh = _frame(1, False, torch.float64)
    with pytest.raises(ValueError, match="frame 0.*share one dtype"):
        tpa.GraphedEwaldBatch(calc, [(q, cell.float(), pos, idx, sh)])
    with pytest.raises(ValueError, match="frame 1.*one device"):
        tpa.GraphedEwaldBatch(calc, [(q, cell, pos, idx, sh), (q, cell, pos.cpu(), idx, sh)])
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        tpa.GraphedEwaldBatch(calc, [tuple(t.cpu() for t in (q, cell, pos, idx, sh))])
    ok = tpa.GraphedEwaldBatch(calc, [(q, cell, pos, idx, sh)])
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        ok.recapture([(idx.cpu(), sh.cpu())])
