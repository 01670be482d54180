"""GPU tests of 2-D periodic (slab) systems in the fused and graphed MD steps, against the reference's values
(``tests/golden/slab_step.npz``, written by ``tests/golden/make_slab_step_golden.py``).

Sizes: every case has a 32 x 32 x 64 mesh (128 bricks) and 288 or 400 atoms, the smallest with bricks and power-of-two planes.
Routes these sizes reach (``mipme_last_cosched_kernel``): the PLANE spread (``plane_rows*``) whenever the charge mesh is not read
again -- every eager call here and the graphed steps without ``cell_gradient`` -- and the BRICK spread (``spread_rows*``) in the
graphed binned step with ``cell_gradient=True``, which keeps the charge mesh; the live-bin step has its own kernel
(``live_spread_rows_kernel``).  The sparse spread needs 4 096 bricks and is not reached.

Tolerances.  fp64: 1e-9 relative L2, the package's standing bound for the HIP path against the reference in double.  fp32: the
rule of ``tests/test_gpu_spline.py`` -- max error <= 5 x the reference's own fp32-against-fp64 spread of that quantity (stored in
the golden, checked there to be non-zero) + 4 eps32 x scale.  Replays after the atoms moved are compared with the eager call
with the gather tail switched off (``ops.TAIL_FUSION = False``), i.e. with the separate slab launches that serve every call
outside the tail, at the same two bounds (fp32: with the spread of the case the moved system was made from).
"""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "slab_step.npz"))
NAMES = [str(n) for n in GOLD["names"]]
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
EPS32 = float(np.finfo(np.float32).eps)
CUTOFF = float(GOLD["cutoff"])
DEFAULT_ROUTES = (os.environ.get("MIPME_PLANE_SPREAD", "1") != "0" and os.environ.get("MIPME_PLANE_BANDS", "1") != "0"
                  and os.environ.get("MIPME_DETERMINISTIC", "0") == "0")
#: stages of the library (``mipme_profile_report``) in ONE eager evaluation -- forward + backward -- with ``periodic=None`` of
#: the systems below, all four gradients asked: binning, spread + pair sum, convolution, gather + energy + forces, cell sums.
#: The count of the code before the slab term entered the tail; the slab call may have one more (the moments).
STAGES_FULLY_PERIODIC = 5


def system(name, dtype, grad=False):
    t = lambda key, dt=dtype: torch.tensor(GOLD[f"{name}_{key}"], dtype=dt, device=DEV)  # noqa: E731
    axis = int(GOLD[f"{name}_axis"])
    s = dict(q=t("charges"), cell=t("cell"), pos=t("positions"), pairs=t("pairs", torch.int64), shifts=t("shifts"), axis=axis,
             periodic=tuple(d != axis for d in range(3)))
    if grad:
        for k in ("q", "cell", "pos"):
            s[k].requires_grad_(True)
    return s


def calculator(name, potential=None):
    pot = tpa.CoulombPotential(smearing=float(GOLD["smearing"])) if potential is None else potential
    cls = tpa.P3MCalculator if str(GOLD[f"{name}_method"]) == "p3m" else tpa.PMECalculator
    return cls(pot, mesh_spacing=float(GOLD["mesh_spacing"]), interpolation_nodes=int(GOLD[f"{name}_nodes"])).to(DEV)


def rell2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def check_golden(got, name, dtype, what=""):
    """got: {V, E, gpos, gq, gcell} (any subset) as arrays."""
    for key, val in got.items():
        want = GOLD[f"{name}_{key}_f64"]
        val = np.asarray(val, dtype=np.float64).reshape(want.shape)
        if dtype == F64:
            err, tol = rell2(val, want), 1e-9
        else:
            scale = np.abs(want).max()
            err, tol = np.abs(val - want).max(), 5 * float(GOLD[f"{name}_spread_{key}"]) + 4 * EPS32 * scale
        print(f"{what}{name} {key} {dtype}: error {err:.3e} (bound {tol:.3e})")
        assert err <= tol, f"{what}{name} {key} {dtype}: error {err:.3e} > {tol:.3e}"


def check_same(got, want, dtype, what, name):
    """got against another evaluation of the same system by this package.  fp32: the bound of ``check_golden`` for the case the
    system was made from (the atoms are 1e-4 from the golden's): 5 x the reference's own fp32 spread + 4 eps32 x scale.  Not a
    multiple of eps32 x the size of the RESULT: dE/dcell is a sum of mesh, pair and atom terms of the size of E that cancel to a
    hundredth of it, and an fp32 evaluation carries the rounding of the terms -- which is what the reference's spread measures."""
    for key in got:
        g, w = got[key].detach().double().cpu().numpy(), want[key].detach().double().cpu().numpy().reshape(got[key].shape)
        if dtype == F64:
            err, tol = rell2(g, w), 1e-9
        else:
            err, tol = np.abs(g - w).max(), 5 * float(GOLD[f"{name}_spread_{key}"]) + 4 * EPS32 * np.abs(w).max()
        print(f"{what} {key} {dtype}: error {err:.3e} (bound {tol:.3e})")
        assert err <= tol, f"{what} {key} {dtype}: error {err:.3e} > {tol:.3e}"


def eager(calc, s, periodic=True, pos=None, pairs=None, shifts=None):
    """One eager evaluation with all four gradients: V, E, dE/dpos, dE/dq, dE/dcell and the potentials' autograd node."""
    q = s["q"].detach().clone().requires_grad_(True)
    cell = s["cell"].detach().clone().requires_grad_(True)
    p = (s["pos"] if pos is None else pos).detach().clone().requires_grad_(True)
    pairs = s["pairs"] if pairs is None else pairs
    shifts = s["shifts"] if shifts is None else shifts
    per = torch.tensor(s["periodic"], device=DEV) if periodic else None
    # (distances that live in the pair kernel's registers only, their gradient sent straight to positions and cell -- the
    # conditions under which a fully periodic call has its gather tail with the cell sums, too)
    V = calc(q, cell, p, pairs, tpa.pair_distances(p, pairs, cell, shifts, deferred="virtual"), periodic=per)
    node = V.grad_fn
    E = tpa.weighted_sum(V, q)
    E.backward()
    return dict(V=V.detach(), E=E.detach(), gpos=p.grad, gq=q.grad, gcell=cell.grad), node


def as_numpy(res):
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


# ---- the eager call: the slab term rides in the gather tail ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_eager_call_keeps_the_gather_tail(name, dtype):
    s = system(name, dtype)
    res, node = eager(calculator(name), s)
    tail = node.tail
    assert tail is not None, "a slab call with one channel and 1/r must keep the gather tail"
    assert tail["grad_q"] is not None and tail["grad_cell"] is not None
    assert node.slab_in_tail and node.slab_axis == s["axis"]
    check_golden(as_numpy(res), name, dtype)


def test_other_slab_calls_take_the_separate_launches():
    """Two channels: outside the tail, served by ``mipme_slab_forward`` / ``mipme_slab_backward`` as before -- and equal, channel
    by channel, to the single-channel call that rides in the tail."""
    name = "ortho_ax1_charged"
    s = system(name, F64)
    calc = calculator(name)
    q2 = torch.cat([s["q"], -2.0 * s["q"]], dim=1).requires_grad_(True)
    p = s["pos"].clone().requires_grad_(True)
    V2 = calc(q2, s["cell"], p, s["pairs"], tpa.pair_distances(p, s["pairs"], s["cell"], s["shifts"]),
              periodic=torch.tensor(s["periodic"], device=DEV))
    assert V2.grad_fn.tail is None and not V2.grad_fn.slab_in_tail
    want = GOLD[f"{name}_V_f64"]
    assert rell2(V2[:, :1].detach().cpu().numpy(), want) < 1e-9 and rell2(V2[:, 1:].detach().cpu().numpy(), -2.0 * want) < 1e-9


# ---- the graphed steps -----------------------------------------------------------------------------------------------------------
def graphed(calc, s, form, **kw):
    kw = dict(dict(charge_gradient=True, cell_gradient=True, slab_correction=True, periodic=s["periodic"]), **kw)
    if form == "explicit":
        return tpa.GraphedEnergyForces(calc, s["q"], s["cell"], s["pos"], s["pairs"], s["shifts"], **kw)
    return tpa.GraphedEnergyForces(calc, s["q"], s["cell"], s["pos"], neighbors=CUTOFF, live_bins={"binned": False, "live": True}[form],
                                   **kw)


def step_results(out):
    E, F, gq, gcell = out
    return dict(E=E.clone(), gpos=-F, gq=gq.clone(), gcell=gcell.clone())


def moved_positions(s, name):
    """The positions a little further on (1e-4: far more than any bound here, far less than a mesh point) -- such that no pair
    crosses the cutoff, so that a list rebuilt from them holds the pairs of the golden's list."""
    rng = np.random.default_rng(7)
    pos = s["pos"].double().cpu().numpy() + 1e-4 * rng.uniform(-1, 1, s["pos"].shape)
    cell = s["cell"].double().cpu().numpy()
    pairs, shifts, _ = tpa.neighbor_list(pos, cell, CUTOFF, periodic=s["periodic"])
    assert len(pairs) == len(GOLD[f"{name}_pairs"])
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)  # noqa: E731
    return t(pos, s["pos"].dtype), t(pairs, torch.int64), t(shifts, s["pos"].dtype)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["explicit", "binned", "live"])
@pytest.mark.parametrize("name", ["ortho_ax0_charged", "tric_ax2_charged", "ortho_ax2_charged_pme"])
def test_graphed_step(name, form, dtype, monkeypatch):
    s = system(name, dtype)
    calc = calculator(name)
    step = graphed(calc, s, form)
    assert (step._live is not None) == (form == "live")
    check_golden(as_numpy(step_results(step())), name, dtype, what=f"{form} ")
    # the atoms move: a replay with the old list, then the list rebuilt (refresh / recapture) -- against the eager call that
    # adds the term with launches of its own
    pos2, pairs2, shifts2 = moved_positions(s, name)
    got_stale = step_results(step(pos2))
    if form == "explicit":
        step.recapture(pairs2, shifts2, positions=pos2)
    else:
        step.refresh(pos2, check=True)
    got_fresh = step_results(step())
    monkeypatch.setattr(ops, "TAIL_FUSION", False)
    want, node = eager(calc, s, pos=pos2, pairs=pairs2, shifts=shifts2)
    assert node.tail is None and not node.slab_in_tail
    want.pop("V")
    check_same(got_stale, want, dtype, f"{form} {name} replay after the move", name)
    check_same(got_fresh, want, dtype, f"{form} {name} replay after the rebuild", name)
    if dtype == F64:  # (the replays did see the new positions)
        assert np.abs(as_numpy(got_fresh)["gpos"] - GOLD[f"{name}_gpos_f64"]).max() > 1e-6


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_graphed_step_without_the_extra_gradients_and_set_charges(dtype):
    """Energy + forces only (no charge / cell gradient in the tail), the energy log, and new charges."""
    name = "ortho_ax1_neutral"
    s = system(name, dtype)
    for form in ("explicit", "live"):
        step = graphed(calculator(name), s, form, charge_gradient=False, cell_gradient=False, energy_log=4)
        E, F = step()
        check_golden(dict(E=E.cpu().numpy(), gpos=-F.cpu().numpy()), name, dtype, what=f"{form} ")
        torch.cuda.synchronize()
        assert step.energy_log.count() == 1 and float(step.energy_log.values[0, 0]) == float(E)
        other = "ortho_ax1_charged"  # the same positions and list, other charges
        assert np.array_equal(GOLD[f"{other}_positions"], GOLD[f"{name}_positions"])
        step.set_charges(torch.tensor(GOLD[f"{other}_charges"], dtype=dtype, device=DEV))
        E, F = step()
        check_golden(dict(E=E.cpu().numpy(), gpos=-F.cpu().numpy()), other, dtype, what=f"{form} set_charges ")
        step.set_charges(torch.tensor(GOLD[f"{name}_charges"], dtype=dtype, device=DEV))  # (the binned step shares s["q"])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("live_bins", [False, None], ids=["binned", "live_or_fallback"])
def test_overflow_atoms_and_empty_bricks(live_bins, dtype):
    """400 atoms in one of the eight layers of bricks along z: 25 per brick where a brick has 4 x ceil(400 / 128) + 8 = 24 slots,
    every other brick -- brick 0 among them, whose workgroup assembles the energy -- empty."""
    name = "lumpy_ax2_charged"
    s = system(name, dtype)
    z = GOLD[f"{name}_positions"][:, 2] / GOLD[f"{name}_cell"][2, 2] * 64
    assert z.min() > 24 and z.max() < 48 and len(z) / 16 > 4 * -(-len(z) // 128) + 8
    step = tpa.GraphedEnergyForces(calculator(name), s["q"], s["cell"], s["pos"], neighbors=CUTOFF, periodic=s["periodic"],
                                   live_bins=live_bins, charge_gradient=True, cell_gradient=True, slab_correction=True)
    print("live step:", step._live is not None)
    check_golden(as_numpy(step_results(step())), name, dtype)


# ---- routes and launches ---------------------------------------------------------------------------------------------------------
def test_same_kernel_family_with_and_without_the_term():
    lib = _lib.load()
    name = "ortho_ax2_charged"
    s = system(name, F32)
    calc = calculator(name)
    seen = {}
    for periodic in (False, True):
        eager(calc, s, periodic=periodic)
        seen["eager", periodic] = lib.mipme_last_cosched_kernel().decode()
        for form in ("explicit", "live"):
            for cell_gradient in (False, True):
                kw = dict(slab_correction=periodic, cell_gradient=cell_gradient)
                if not periodic:
                    kw["periodic"] = (True, True, True) if form == "explicit" else s["periodic"]
                graphed(calc, s, form, **kw)
                seen[form, cell_gradient, periodic] = lib.mipme_last_cosched_kernel().decode()
    print(seen)
    for key, kernel in seen.items():
        if key[-1]:
            assert kernel == seen[key[:-1] + (False,)], key
    if DEFAULT_ROUTES:
        assert seen["eager", True].startswith("plane_rows")
        assert seen["explicit", False, True].startswith("plane_rows")
        assert seen["explicit", True, True].startswith("spread_rows")
        assert seen["live", True, True] == "live_spread_rows_kernel"


def test_one_stage_more_than_the_fully_periodic_call():
    name = "ortho_ax2_charged"
    s = system(name, F32)
    calc = calculator(name)
    counts = {}
    for periodic in (False, True):
        eager(calc, s, periodic=periodic)  # (plans, filter tables, topology)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        try:
            eager(calc, s, periodic=periodic)
            torch.cuda.synchronize()
            report = _lib.profile_report()
        finally:
            _lib.profile_enable(False)
        print(periodic, report)
        counts[periodic] = sum(calls for calls, _ in report.values())
        if periodic:
            assert report["slab_moments"][0] == 1 and "slab_forward" not in report
    assert counts[False] == STAGES_FULLY_PERIODIC
    assert counts[True] <= counts[False] + 1


# ---- finite differences ----------------------------------------------------------------------------------------------------------
def test_forces_against_central_differences():
    """fp64 central differences of E along six coordinates (the non-periodic one, Cartesian z of the triclinic case, among them)
    against the step's forces, at the 1e-6 relative the package states for its finite-difference route."""
    name = "tric_ax2_charged"
    s = system(name, F64)
    calc = calculator(name)
    step = graphed(calc, s, "explicit")
    F = step()[1].clone()
    per = torch.tensor(s["periodic"], device=DEV)

    def energy(pos):
        with torch.no_grad():
            V = calc(s["q"], s["cell"], pos, s["pairs"], tpa.pair_distances(pos, s["pairs"], s["cell"], s["shifts"]), periodic=per)
            return float((V * s["q"]).sum())

    h, scale = 1e-4, float(F.abs().max())
    for atom, d in ((0, 2), (17, 2), (101, 0), (200, 1), (287, 2), (143, 0)):
        plus, minus = s["pos"].clone(), s["pos"].clone()
        plus[atom, d] += h
        minus[atom, d] -= h
        fd = -(energy(plus) - energy(minus)) / (2 * h)
        err = abs(fd - float(F[atom, d])) / scale
        print(f"atom {atom} axis {d}: F {float(F[atom, d]):+.8e} fd {fd:+.8e} rel {err:.2e}")
        assert err <= 1e-6


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    name = "ortho_ax2_charged"
    s = system(name, F64)
    calc = calculator(name)
    with pytest.raises(ValueError, match="exactly two periodic axes"):
        tpa.GraphedEnergyForces(calc, s["q"], s["cell"], s["pos"], s["pairs"], s["shifts"], periodic=(True, False, False),
                                slab_correction=True)
    r6 = calculator(name, tpa.InversePowerLawPotential(exponent=6, smearing=float(GOLD["smearing"])))
    with pytest.raises(ValueError, match="exists for 1/r only"):
        tpa.GraphedEnergyForces(r6, s["q"], s["cell"], s["pos"], s["pairs"], s["shifts"], periodic=s["periodic"], slab_correction=True)
    # the C-ABI, two channels: a real plan, mesh and tail outputs, refused before anything is launched
    lib = _lib.load()
    geom, _ = calc._kspace_setup(s["cell"], F64, DEV, speculate=False)
    md, pot = geom.desc(2), calc.potential._descriptor()
    plan = _lib.FFTPlan(DEV, F64, geom.ns, 2)
    out = torch.zeros(8, dtype=F64, device=DEV)
    args = _lib.KspaceForwardArgs(plan=plan.handle, dtype=_lib.F64, mesh=C.pointer(md), pot=C.pointer(pot), n_atoms=len(s["q"]),
                                  out_energy=out.data_ptr(), out_grad_positions=out.data_ptr(), slab=3)
    assert lib.mipme_kspace_forward(C.byref(args)) == -1
    assert b"the slab term of the gather tail serves one channel" in lib.mipme_last_error()
    with pytest.raises(ValueError, match="one channel"):
        _lib.check(-1)
