"""GraphedDipoleBatch on the GPU (csrc/dipole_batch.hip): six frames of 1 to 300 point dipoles, each with its own cell and k grid,
served by ONE captured graph -- against the reference's own outputs at two cells per frame (tests/golden/dipole_batch.npz), a
direct potential, to the bit against the same frames in another order, alone and replayed; isolation of a frame from what happens
to another one; the batch of one frame against GraphedDipoleStep(follow_cell=True); the status words; the input forms; new lists;
the refusals that need a device."""

import os
import sys

import numpy as np
import pytest
import torch

import torchpme_amd as tpa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_dipole_step import EPS32, _check, _t  # noqa: E402, F401  (the `_check` rule of the single step)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(HERE, "golden", "dipole_batch.npz"))
EB = np.load(os.path.join(HERE, "golden", "ewald_batch.npz"))
DS = np.load(os.path.join(HERE, "golden", "dipole_step.npz"))
DCS = np.load(os.path.join(HERE, "golden", "dipole_cell_step.npz"))
DTYPES = [torch.float64, torch.float32]
LAM = 1.25
STRAIN = np.eye(3) + DCS["strain"]
CALCS = {  # name: (potential, full lists, lr_wavelength)
    "D1": (dict(smearing=1.0), False, LAM),
    "D2": (dict(smearing=1.2, exclusion_radius=2.5, exclusion_degree=3, epsilon=1.5, prefactor=14.399645478425667), True, LAM),
    "D3": (dict(), False, None),
}
ALL = (0, 1, 2, 3, 4, 5)
ATOMS = [1, 2, 17, 24, 300, 3]
GRIDS = [(1, 1, 1), (3, 3, 3), (4, 9, 6), (6, 6, 7), (16, 16, 16), (33, 33, 33)]


def _calc(cname):
    kw, full, lam = CALCS[cname]
    return tpa.CalculatorDipole(tpa.PotentialDipole(**kw), full_neighbor_list=full, lr_wavelength=lam)


def _mirrored(pairs, shifts):
    return np.concatenate([pairs, pairs[:, ::-1]]), np.concatenate([shifts, -shifts])


_SYSTEMS = {}


def _system(n, full):
    """(dipoles, positions, cell, pairs, shifts) of frame n at its construction cell, as the golden script builds them."""
    if (n, full) in _SYSTEMS:
        return _SYSTEMS[n, full]
    i64 = lambda a: a.astype(np.int64)  # noqa: E731
    if n < 3:
        mu, pos, cell = GOLD[f"f{n}_dipoles"], EB[f"f{n}_positions"], EB[f"f{n}_cell"]
        half = (i64(EB[f"f{n}_pairs_half"]).reshape(-1, 2), i64(EB[f"f{n}_shifts_half"]).reshape(-1, 3))
        lst = _mirrored(*half) if full else half
    elif n == 3:
        v = "full" if full else "half"
        mu, pos, cell, lst = DS["tric_dipoles"], DS["tric_positions"], DS["tric_cell"], (i64(DS[f"tric_{v}_pairs"]), i64(DS[f"tric_{v}_shifts"]))
    elif n == 4:
        mu, pos, cell = DCS["big_dipoles"], DCS["big_positions"], DCS["big_cell"]
        half = (i64(DCS["big_pairs"]), i64(DCS["big_shifts"]))
        lst = _mirrored(*half) if full else half
    else:
        mu, pos, cell = GOLD["f5_dipoles"], GOLD["f5_positions"], GOLD["f5_cell"]
        half = (i64(GOLD["f5_pairs_half"]), i64(GOLD["f5_shifts_half"]))
        lst = _mirrored(*half) if full else half
    _SYSTEMS[n, full] = (mu, pos, cell, lst[0], lst[1])
    return _SYSTEMS[n, full]


def _frame(n, full, dtype):
    mu, pos, cell, pairs, shifts = _system(n, full)
    return (_t(mu, dtype), _t(cell, dtype), _t(pos, dtype), torch.tensor(pairs, device=DEV), _t(shifts, dtype))


def _batch(cname, dtype, which=ALL, cell_gradient=True):
    full = CALCS[cname][1]
    return tpa.GraphedDipoleBatch(_calc(cname), [_frame(n, full, dtype) for n in which], cell_gradient=cell_gradient)


def _single(cname, dtype, n, lists=None):
    mu, cell, pos, idx, sh = _frame(n, CALCS[cname][1], dtype)
    if lists is not None:
        idx, sh = lists
    return tpa.GraphedDipoleStep(_calc(cname), mu, cell, pos, idx, sh, cell_gradient=True, follow_cell=True)


def _results(batch, *args, **kw):
    """Per frame {"E", "F", "gmu", "gcell"} as float64 arrays."""
    out = batch(*args, **kw)
    torch.cuda.synchronize()
    host = lambda t: t.detach().double().cpu().numpy().copy()  # noqa: E731
    res = []
    for f in range(batch.n_frames):
        r = {"E": host(out[0][f]), "F": host(out[1][f]), "gmu": host(out[2][f])}
        if len(out) > 3:
            r["gcell"] = host(out[3][f])
        res.append(r)
    return res


def _step_results(step, *args, **kw):
    out = step(*args, **kw)
    torch.cuda.synchronize()
    return {k: v.detach().double().cpu().numpy().copy() for k, v in zip(("E", "F", "gmu", "gcell"), out)}


def _golden(cname, n, ctag):
    """(wanted fp64 values, the reference's own fp32 - fp64 spread, absE) of frame n: its slices of the calculator's arrays."""
    served = [int(f) for f in GOLD[f"{cname}_frames"]]
    i = served.index(n)
    a = sum(ATOMS[f] for f in served[:i])
    b = a + ATOMS[n]

    def get(tag):
        g = lambda k: GOLD[f"{cname}_{k}_{ctag}_{tag}"].astype(np.float64)  # noqa: E731
        return {"E": np.float64(g("E")[i]), "F": -g("gpos")[a:b], "gmu": g("gmu")[a:b], "gcell": g("gcell")[i]}

    want, f32 = get("f64"), get("f32")
    return want, {k: np.abs(f32[k] - want[k]).max() for k in want}, float(GOLD[f"{cname}_absE_{ctag}"][i])


def _bits(batch, *args, **kw):
    """The outputs of a call, per frame, as clones: [[E_f, F_f, gmu_f, gcell_f, status_f]]."""
    out = batch(*args, **kw)
    torch.cuda.synchronize()
    return [[o[f].clone() for o in out] + [batch.status[f].clone()] for f in range(batch.n_frames)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _status(batch):
    return [int(s) for s in batch.status.cpu()]


# ---- 1. against the reference: all six frames, both cells, one graph --------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["D1", "D2"])
def test_six_frames_match_the_reference_and_follow_their_cells(cname, dtype):
    full = CALCS[cname][1]
    batch = _batch(cname, dtype)
    assert batch.ns == GRIDS and batch.n_frames == 6 and batch.lr_wavelength == LAM
    assert batch.n_k[0] == 0 and batch.n_k[4] >= 2048 and batch.n_k[5] == 17968
    assert batch.atom_ptr == [0, 1, 3, 20, 44, 344, 347]
    graph = batch.graph
    res = _results(batch)
    for n in ALL:
        _check(res[n], *_golden(cname, n, "c0"), dtype, f"{cname} f{n} cell0")
    assert _status(batch) == [0] * 6
    # ONE call: frames 0, 2 and 4 move to the strained cell (positions and cell, given as lists), frames 1, 3 and 5 stay
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
    assert _status(batch) == [0] * 6 and batch.graph is graph
    assert batch.kgrid_matches(cells) == [True] * 6
    # without the cell gradient: three outputs, the same bounds
    plain = _batch(cname, dtype, cell_gradient=False)
    out = plain()
    assert len(out) == 3 and out[0].shape == (6,) and plain.cell_grads is None
    res = _results(plain)
    for n in ALL:
        want, spread, abs_e = _golden(cname, n, "c0")
        want.pop("gcell")
        _check(res[n], want, spread, abs_e, dtype, f"{cname} f{n} without the cell gradient")


# ---- 2. a direct potential: pair rows only ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_direct_potential(dtype):
    which = (1, 2, 3, 4)
    batch = _batch("D3", dtype, which=which)
    assert batch.n_k == [0] * 4 and batch.ns == [(1, 1, 1)] * 4 and batch.lr_wavelength == 0.0
    res = _results(batch)
    for f, n in enumerate(which):
        _check(res[f], *_golden("D3", n, "c0"), dtype, f"D3 f{n} cell0")
    assert _status(batch) == [0] * 4
    systems = [_system(n, False) for n in which]
    res = _results(batch, positions=[_t(s[1] @ STRAIN, dtype) for s in systems], cells=[_t(s[2] @ STRAIN, dtype) for s in systems])
    for f, n in enumerate(which):
        _check(res[f], *_golden("D3", n, "c1"), dtype, f"D3 f{n} cell1")
    assert _status(batch) == [0] * 4
    assert batch.kgrid_matches([_t(1.5 * s[2], dtype) for s in systems]) == [True] * 4
    # bit 0 is never set, whatever the cell: 1.5 x every cell, positions along
    batch(positions=[_t(1.5 * s[1], dtype) for s in systems], cells=[_t(1.5 * s[2], dtype) for s in systems])
    assert _status(batch) == [0] * 4


# ---- 3. output layout -------------------------------------------------------------------------------------------------------
def test_output_layout():
    batch = _batch("D1", torch.float32)
    E, F, gmu, gcell = batch()
    assert E.shape == (6,) and gcell.shape == (6, 3, 3) and batch.status.shape == (6,) and batch.status.dtype == torch.int32
    assert batch.forces_flat.shape == (347, 3) and batch.dipole_grads_flat.shape == (347, 3) and batch.cells.shape == (6, 3, 3)
    assert gcell is batch.cell_grads and gmu is batch.dipole_grads and F is batch.forces and E is batch.energies
    for f, (a, b) in enumerate(zip(batch.atom_ptr[:-1], batch.atom_ptr[1:])):
        assert F[f].shape == (b - a, 3) and gmu[f].shape == (b - a, 3)
        assert F[f].data_ptr() == batch.forces_flat[a:b].data_ptr() and gmu[f].data_ptr() == batch.dipole_grads_flat[a:b].data_ptr()


# ---- 4. a frame's bits depend on its own inputs only ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["D1", "D2"])
def test_independence_to_the_bit(cname, dtype):
    batch = _batch(cname, dtype)
    first = _bits(batch)
    assert all(_same(a, b) for a, b in zip(first, _bits(batch)))  # equal inputs, equal bits
    backwards = _bits(_batch(cname, dtype, which=ALL[::-1]))
    for n in ALL:
        assert _same(first[n], backwards[5 - n]), f"frame {n} in the reversed batch"
        alone = _bits(_batch(cname, dtype, which=(n,)))
        assert _same(first[n], alone[0]), f"frame {n} alone"


# ---- 5. what happens to one frame happens to that frame alone ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_isolation(dtype):
    cname, full = "D1", False
    batch = _batch(cname, dtype)
    graph, first = batch.graph, _bits(batch)
    systems = [_system(n, full) for n in ALL]
    pos0, cells0 = [_t(s[1], dtype) for s in systems], [_t(s[2], dtype) for s in systems]
    # new positions and a new cell for frame 2 only
    pos, cells = list(pos0), list(cells0)
    pos[2], cells[2] = _t(systems[2][1] @ STRAIN, dtype), _t(systems[2][2] @ STRAIN, dtype)
    other = _bits(batch, positions=pos, cells=cells)
    for n in (0, 1, 3, 4, 5):
        assert _same(first[n], other[n]), f"frame {n} while frame 2 moved"
    assert not torch.equal(first[2][0], other[2][0])
    # a singular cell (two equal rows) for frame 1 only
    singular = systems[1][2].copy()
    singular[2] = singular[0]
    cells = list(cells0)
    cells[1] = _t(singular, dtype)
    broken = _bits(batch, positions=pos0, cells=cells)
    assert bool(torch.isnan(broken[1][0])) and bool(torch.isnan(broken[1][3]).all()) and int(broken[1][4]) == 2
    for n in (0, 2, 3, 4, 5):
        assert _same(first[n], broken[n]) and int(broken[n][4]) == 0, f"frame {n} beside a singular cell"
    # the correct cells restore the first results bit for bit
    again = _bits(batch, cells=cells0)
    assert all(_same(a, b) for a, b in zip(first, again)) and batch.graph is graph and _status(batch) == [0] * 6


# ---- 6. the batch of one frame against the single step that follows its cell ----------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cname", ["D1", "D2"])
@pytest.mark.parametrize("n", ALL)
def test_a_batch_of_one_frame_against_the_single_step(n, cname, dtype):
    """E, F, dE/dmu and dE/dcell at the construction cell and -- from the same graphs -- at the strained cell with the strained
    positions, within the project's rule with the fp64 GraphedDipoleStep(follow_cell=True) as the wanted value.  The kernels of
    the batch are new text beside those of the single step: equality to the bit is not required here.
    profiles/dipole_batch_bits.txt records where it holds: in all 120 fp64 outputs of these cases and in 53 of the 120 fp32 ones
    (the others differ by a few ulp), so equality is not asserted."""
    want_step, batch = _single(cname, torch.float64, n), _batch(cname, dtype, which=(n,))
    graphs = (want_step.graph, batch.graph)
    assert batch.ns[0] == tuple(want_step.ns) and batch.n_k[0] == want_step.n_k
    _, p, c, _, _ = _system(n, CALCS[cname][1])
    for ctag, m in (("c0", np.eye(3)), ("c1", STRAIN)):
        want = _step_results(want_step, positions=_t(p @ m, torch.float64), cell=_t(c @ m, torch.float64))
        res = _results(batch, positions=[_t(p @ m, dtype)], cells=[_t(c @ m, dtype)])[0]
        _, spread, abs_e = _golden(cname, n, ctag)
        _check(res, want, spread, abs_e, dtype, f"{cname} f{n} {ctag}: batch of one against the single step")
        assert _status(batch) == [0] and int(want_step.status.cpu()[0]) == 0
    assert (want_step.graph, batch.graph) == graphs


# ---- 7. status bit 0 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_status_bit_0_of_one_frame_and_the_energy_of_the_kept_grid(dtype):
    """Frame 3's first axis stretched by 1.15: ceil(|a_0| / 1.25) goes from 6 to 7.  The batch keeps the frame's grid and says so
    in status[3] alone; what the frame returns is what a fp64 GraphedDipoleStep(follow_cell=True) of the same frame, built at the
    same cell and fed the stretched one, returns (the fp32 spread is that of the frame's golden cell)."""
    cname = "D1"
    batch = _batch(cname, dtype)
    systems = [_system(n, False) for n in ALL]
    stretched = systems[3][2].copy()
    stretched[0] *= 1.15
    assert int(np.ceil(np.linalg.norm(systems[3][2][0]) / LAM)) == 6 == batch.ns[3][0]
    assert int(np.ceil(np.linalg.norm(stretched[0]) / LAM)) == 7
    cells = [_t(s[2], dtype) for s in systems]
    cells[3] = _t(stretched, dtype)
    assert batch.kgrid_matches(cells) == [True, True, True, False, True, True]
    res = _results(batch, cells=cells)
    assert _status(batch) == [0, 0, 0, 1, 0, 0] and np.isfinite(res[3]["E"])
    step = _single(cname, torch.float64, 3)
    want = _step_results(step, cell=_t(stretched, torch.float64))
    assert int(step.status.cpu()[0]) == 1
    _, spread, abs_e = _golden(cname, 3, "c0")
    _check(res[3], want, spread, abs_e, dtype, "frame 3 on its kept grid")
    for n in (0, 1, 2, 4, 5):
        _check(res[n], *_golden(cname, n, "c0"), dtype, f"f{n} beside the stretched frame")


# ---- 8. input forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_forms_and_new_dipoles(dtype):
    cname = "D1"
    batch = _batch(cname, dtype)
    graph = batch.graph
    systems = [_system(n, False) for n in ALL]
    pos = [_t(s[1] @ STRAIN, dtype) for s in systems]
    cells = [_t(s[2] @ STRAIN, dtype) for s in systems]
    mu = [_t(s[0], dtype) for s in systems]
    as_lists = _bits(batch, positions=pos, dipoles=mu, cells=cells)
    batch(positions=[_t(s[1], dtype) for s in systems], cells=[_t(s[2], dtype) for s in systems])
    flat = _bits(batch, positions=torch.cat(pos), dipoles=torch.cat(mu), cells=torch.stack(cells))
    assert all(_same(a, b) for a, b in zip(as_lists, flat))
    with pytest.raises(ValueError, match="6 per-frame tensors"):
        batch(positions=pos[:5])
    # dipoles= alone: no second dipole set is stored, so frame 3 is held against a GraphedDipoleStep of the same frame
    mu2 = [_t(np.random.default_rng(50 + n).normal(size=s[0].shape), dtype) for n, s in enumerate(systems)]
    batch(positions=[_t(s[1], dtype) for s in systems], cells=[_t(s[2], dtype) for s in systems])
    before = _bits(batch)
    res = _results(batch, dipoles=mu2)
    assert batch.graph is graph and not torch.equal(before[3][2], batch.dipole_grads[3])
    step = _single(cname, torch.float64, 3)
    want = _step_results(step, dipoles=mu2[3].double())
    _, spread, _ = _golden(cname, 3, "c0")
    abs_e = float(np.abs(0.5 * (mu2[3].double().cpu().numpy() * want["gmu"]).sum(axis=1)).sum())
    _check(res[3], want, spread, abs_e, dtype, "frame 3 with new dipoles")
    assert all(_same(a, b) for a, b in zip(before, _bits(batch, dipoles=torch.cat(mu))))


# ---- 9. new lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_recapture_with_new_lists_and_a_refused_one(dtype):
    cname = "D1"
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
    for n in (0, 1, 2, 3, 5):
        assert _same(before[n], after[n])
    assert not torch.equal(before[4][1], after[4][1])
    res = _results(batch)
    step = _single(cname, torch.float64, 4, lists=(new[4][0], _t(s4, torch.float64)))
    want = _step_results(step)
    _, spread, abs_e = _golden(cname, 4, "c0")
    _check(res[4], want, spread, abs_e, dtype, "frame 4 with the shorter list")


# ---- 10. refusals that need a device ----------------------------------------------------------------------------------------
def test_constructor_refusals_with_a_device():
    calc = _calc("D1")
    with pytest.raises(ValueError, match="frame 1.*share one dtype.*float32"):
        tpa.GraphedDipoleBatch(calc, [_frame(1, False, torch.float64), _frame(2, False, torch.float32)])
    mu, cell, pos, idx, sh = _frame(1, False, torch.float64)
    with pytest.raises(ValueError, match="frame 0.*share one dtype"):
        tpa.GraphedDipoleBatch(calc, [(mu, cell.float(), pos, idx, sh)])
    with pytest.raises(ValueError, match="frame 1.*one device"):
        tpa.GraphedDipoleBatch(calc, [(mu, cell, pos, idx, sh), (mu, cell, pos.cpu(), idx, sh)])
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        tpa.GraphedDipoleBatch(calc, [tuple(t.cpu() for t in (mu, cell, pos, idx, sh))])
    ewald = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=1.0), lr_wavelength=LAM)
    with pytest.raises(TypeError, match="GraphedDipoleBatch serves a CalculatorDipole, got a EwaldCalculator"):
        tpa.GraphedDipoleBatch(ewald, [(mu, cell, pos, idx, sh)])
    ok = tpa.GraphedDipoleBatch(calc, [(mu, cell, pos, idx, sh)])
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        ok.recapture([(idx.cpu(), sh.cpu())])
