"""Deferred slot fill (``MIPME_DEFER_SLOTS``, docs/SWITCHES.md): on the plane-spread route the binning pass runs lean -- counters,
overflow bookkeeping, atom records, plane-list entries and the destination slot of every atom -- and rider workgroups of the
convolution's inverse (y,z) plane launch write what only the gather (and a later backward pass) reads: slot record, 6n weights,
charge by slot, reach code.  What can go wrong is a slot the gather reads and no rider wrote (overflow slots, the last partial
rider block, fewer atoms than one block, a replayed graph whose atoms moved), coordinates that differ between the two launches,
a backward pass after another forward, cell riders and slot riders on one launch, a bricks-route call after a deferred one.

Every test asserts through ``mipme_last_slot_fill()`` which route RAN (0: one pass; B > 0: riders of B atoms each): a fallback
cannot hide a failure.  Boxes as tests/test_gpu_round6.py ``_box`` and tests/test_gpu_parity.py ``test_bin_overflow_region``
(64^3 mesh, cutoff 4); tolerances of the latter: potentials and energy / gradients 1e-11 / 1e-10 in fp64, 2e-5 / 2e-4 in fp32, the
energy relative to |E| as there."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from oracle import pme_numpy as O
from torchpme_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: the library's default routes (docs/SWITCHES.md): with any of these switched the one-pass kernel is what must have run
DEFERRED = (os.environ.get("MIPME_DEFER_SLOTS", "1") != "0" and os.environ.get("MIPME_PLANE_SPREAD", "1") != "0"
            and os.environ.get("MIPME_DETERMINISTIC", "0") == "0" and os.environ.get("MIPME_SPARSE_FORCE", "0") == "0")
L_BOX = 24.0
H = 2 * L_BOX / 62  # -> 64^3 mesh
SCHEMES = [("P3M", 5), ("P3M", 4), ("PME", 4)]
DTYPES = [torch.float64, torch.float32]


def rell2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def tols(dtype):
    return (1e-11, 1e-10) if dtype == torch.float64 else (2e-5, 2e-4)


def slot_fill():
    return _lib.load().mipme_last_slot_fill()


def assert_route(deferred=True):
    """The last forward call filled its slots by riders (or, deferred = False, in one pass)."""
    fill = slot_fill()
    assert (fill > 0) == (deferred and DEFERRED), fill
    return fill


def make_calc(scheme, order, dtype, sm=1.0):
    Calc = tpa.P3MCalculator if scheme == "P3M" else tpa.PMECalculator
    return Calc(tpa.CoulombPotential(smearing=sm), mesh_spacing=H, interpolation_nodes=order).to(dtype)


def lattice(rng, n_atoms=None, n_side=12, a=2.0):
    """tests/test_gpu_round6.py ``_box``: a jittered 12^3 lattice in a 24 A cube (1728 atoms); n_atoms: a random subset of it."""
    g = (np.arange(n_side) + 0.5) * a
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.3, 0.3, (n_side**3, 3))
    if n_atoms is not None:
        pos = pos[rng.permutation(len(pos))[:n_atoms]]
    return pos, n_side * a * np.eye(3)


class Ref:
    """Oracle results of one system: potentials, energy, forces; ``adjoint(g)``: the gradients of sum g V."""

    def __init__(self, scheme, order, q, cell, pos, pairs, S, sm=1.0):
        self.q, self.cell, self.pos, self.pairs, self.S = q, cell, pos, pairs, S
        dist, _ = O.pair_distances(pos, cell, pairs, S)
        spec = O.PotentialSpec("coulomb", 1, sm, 1.0)
        self.V, self.cache = O.forward(spec, "P3M" if scheme == "P3M" else "Lagrange", order, H, q, cell, pos, pairs, dist,
                                       return_cache=True)
        gr = self.adjoint(q)
        self.E = float((self.V * q).sum())
        self.E_scale = abs(self.E)
        self.F = -gr["positions"]
        self.dq = gr["charges"] + self.V
        self.dcell = gr["cell"]

    def adjoint(self, g):
        gr = O.backward(self.cache, g)
        gpos_d, gcell_d = O.pair_distances_backward(self.pos, self.cell, self.pairs, self.S, gr["dist"])
        return dict(positions=gr["positions"] + gpos_d, charges=gr["charges"], cell=gr["cell"] + gcell_d)


def system(pos, cell, q, scheme="P3M", order=5):
    pairs, S, _ = tpa.neighbor_list(pos, cell, 4.0)
    return Ref(scheme, order, q, cell, pos, pairs, S)


@functools.lru_cache(maxsize=None)
def box_ref(scheme, order):
    """The box every test without a shape of its own uses (computed once per scheme, never modified)."""
    rng = np.random.default_rng(101)
    pos, cell = lattice(rng)
    q = rng.normal(size=(len(pos), 1))
    q -= q.mean()
    return system(pos, cell, q, scheme, order)


def tensors(ref, dtype, grad=False):
    t = lambda a, g=False: torch.tensor(a, device=DEV, dtype=dtype, requires_grad=g)  # noqa: E731
    return t(ref.q), t(ref.cell, grad), t(ref.pos, grad), torch.tensor(ref.pairs, device=DEV), t(ref.S)


def force_error(F, ref, floor):
    """|F - F_ref| over |F_ref|, or (floor: the single atom in fp32, nothing else) over the larger of |F_ref| and |q V| / h.  A lone
    atom's force is the mesh's self-force, a discretisation residual between four and five orders below the scale its terms are
    rounded at (a potential energy per mesh spacing: the fp64 result, which needs no floor, is 3e-11 of its own norm where every
    other case is 2e-15): fp32 rounding of 1e-7 of that scale is 1e-3 .. 1e-2 of the residual itself, on either route."""
    F = np.asarray(F, dtype=np.float64)
    scale = np.linalg.norm(ref.F)
    if floor:
        scale = max(scale, float(np.linalg.norm(ref.q * ref.V)) / H)
    return float(np.linalg.norm(F - ref.F) / scale)


def check_eager(calc, ref, dtype, floor=False):
    """Potentials, energy and forces of the eager calculator (energy mode of the backward pass) against the oracle."""
    tolV, tolG = tols(dtype)
    tq, tc, tp, ti, tS = tensors(ref, dtype, grad=True)
    V = calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    assert_route()
    E = tpa.weighted_sum(V, tq)
    E.backward()
    eV, eE, eF = rell2(V.detach().cpu(), ref.V), abs(float(E.detach()) - ref.E) / ref.E_scale, force_error(-tp.grad.cpu(), ref, floor)
    print(f"eager {dtype} N={len(ref.pos)}: relV={eV:.2e} relE={eE:.2e} relF={eF:.2e}")
    assert eV < tolV and eE < tolV and eF < tolG, (eV, eE, eF)


def check_graphed(calc, ref, dtype, floor=False):
    tolV, tolG = tols(dtype)
    tq, tc, tp, ti, tS = tensors(ref, dtype)
    step = tpa.GraphedEnergyForces(calc, tq, tc, tp, ti, tS)
    E, F = step()
    assert_route()
    eE, eF = abs(float(E) - ref.E) / ref.E_scale, force_error(F.cpu(), ref, floor)
    print(f"graphed {dtype} N={len(ref.pos)}: relE={eE:.2e} relF={eF:.2e}")
    assert eE < tolV and eF < tolG, (eE, eF)
    return step


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("scheme,order", SCHEMES)
def test_parity_with_the_oracle(scheme, order, dtype):
    """Potentials, energy and forces on the box, through the eager calculator and through the graph-replayed step."""
    ref = box_ref(scheme, order)
    calc = make_calc(scheme, order, dtype)
    check_eager(calc, ref, dtype)
    check_graphed(calc, ref, dtype)


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import torchpme_amd as tpa
from torchpme_amd import _lib
d = np.load(sys.argv[2])
out = {}
for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
    t = lambda a: torch.tensor(a, device="cuda:0", dtype=dtype)
    calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=float(d["h"]), interpolation_nodes=5).to(dtype)
    ti, tS = torch.tensor(d["pairs"], device="cuda:0"), t(d["S"])
    V = calc(t(d["q"]), t(d["cell"]), t(d["pos"]), ti, tpa.pair_distances(t(d["pos"]), ti, t(d["cell"]), tS))
    out["fill_eager_" + name] = _lib.load().mipme_last_slot_fill()
    E, F = tpa.GraphedEnergyForces(calc, t(d["q"]), t(d["cell"]), t(d["pos"]), ti, tS)()
    out["fill_graph_" + name] = _lib.load().mipme_last_slot_fill()
    out["V_" + name], out["E_" + name], out["F_" + name] = V.cpu().numpy(), E.cpu().numpy(), F.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def test_deferred_against_one_pass_bit_for_bit(tmp_path):
    """``MIPME_PLANE_PARTS=1``: the fp32 mesh is bit-reproducible (fixed-point sums do not depend on arrival order) and a gather's
    result does not depend on which slot an atom sits in, so potentials, energy and forces with ``MIPME_DEFER_SLOTS=1`` and ``=0``
    are identical bit for bit; the fp64 sums (``ds_add_f64``) depend on order: 1e-12 relative.  The library reads its switches
    once per process: one fresh child process per setting."""
    ref = box_ref("P3M", 5)
    np.savez(tmp_path / "in.npz", q=ref.q, cell=ref.cell, pos=ref.pos, pairs=ref.pairs, S=ref.S, h=H)
    res = {}
    for defer in ("1", "0"):
        env = dict(os.environ, MIPME_PLANE_PARTS="1", MIPME_DEFER_SLOTS=defer)
        out = tmp_path / f"out{defer}.npz"
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(out)], env=env, capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        res[defer] = np.load(out)
    for name in ("f32", "f64"):
        for how in ("eager", "graph"):
            assert (res["1"][f"fill_{how}_{name}"] > 0) == DEFERRED and res["0"][f"fill_{how}_{name}"] == 0
    for k in ("V", "E", "F"):
        assert np.array_equal(res["1"][k + "_f32"], res["0"][k + "_f32"]), (k, np.abs(res["1"][k + "_f32"] - res["0"][k + "_f32"]).max())
        assert relmax(res["1"][k + "_f64"], res["0"][k + "_f64"]) <= 1e-12, k
    assert rell2(res["1"]["V_f64"], ref.V) < 1e-11  # (and both are the oracle's)


@functools.lru_cache(maxsize=None)
def rider_block():
    """Atoms per rider workgroup on the 64^3 mesh, as the launcher reports it after a deferred call."""
    ref = edge_ref(64)
    tq, tc, tp, ti, tS = tensors(ref, torch.float32)
    make_calc("P3M", 5, torch.float32)(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    return slot_fill()


@functools.lru_cache(maxsize=None)
def edge_ref(n_atoms):
    rng = np.random.default_rng(200 + n_atoms)
    pos, cell = lattice(rng, n_atoms)
    return system(pos, cell, rng.normal(size=(n_atoms, 1)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", ["1", "63", "64", "65", "B-1", "B", "B+1"])
def test_atom_counts_at_the_edges(n, dtype):
    """Fewer atoms than a wavefront, one more and one fewer than a wavefront and than a rider's share B of the atoms (what the
    launcher actually uses): the last partial rider, and no rider short of an atom.  (N = 1 in fp32: see force_error.)"""
    if n.startswith("B"):
        B = rider_block()
        if not DEFERRED:
            B = 1024
        assert 64 <= B <= 1024
        n_atoms = B + {"B-1": -1, "B": 0, "B+1": 1}[n]
    else:
        n_atoms = int(n)
    ref = edge_ref(n_atoms)
    calc = make_calc("P3M", 5, dtype)
    floor = n_atoms == 1 and dtype == torch.float32
    check_eager(calc, ref, dtype, floor=floor)
    check_graphed(calc, ref, dtype, floor=floor)


def blob(kind):
    """The "corner" and "slab" blobs of tests/test_gpu_parity.py ``test_bin_overflow_region``."""
    rng = np.random.default_rng(17)
    cell = np.eye(3) * L_BOX
    if kind == "corner":  # 260 atoms in a 2.6 A cube: nearly every destination slot lies in the brick overflow region
        N = 260
        pos = rng.uniform(0.2, 2.8, (N, 3))
    else:  # a sheet perpendicular to x: ~300 atoms for each of two plane lists of 128 -- the plane overflow list
        N = 600
        gy, gz = np.meshgrid((np.arange(25) + 0.5) * L_BOX / 25, (np.arange(24) + 0.5) * L_BOX / 24, indexing="ij")
        pos = np.stack([rng.uniform(3.0, 3.35, N), gy.ravel() + rng.uniform(-0.2, 0.2, N), gz.ravel() + rng.uniform(-0.2, 0.2, N)], 1)
    q = rng.normal(size=(N, 1))
    q -= q.mean()
    return system(pos, cell, q), rng.normal(size=(N, 1))


@functools.lru_cache(maxsize=None)
def blob_ref(kind):
    return blob(kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["corner", "slab"])
def test_brick_and_plane_list_overflow(kind, dtype):
    """Brick overflow (corner: dst >= over_base for nearly every atom) and plane-list overflow (slab): potentials, energy, forces
    and the general adjoint -- a random upstream gradient, whose second spread reads the riders' weights and reach codes."""
    ref, g = blob_ref(kind)
    tolV, tolG = tols(dtype)
    calc = make_calc("P3M", 5, dtype)
    check_eager(calc, ref, dtype)
    check_graphed(calc, ref, dtype)
    tq, tc, tp, ti, tS = tensors(ref, dtype, grad=True)
    tq.requires_grad_(True)
    V = calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    assert_route()
    (V * torch.tensor(g, device=DEV, dtype=dtype)).sum().backward()
    gr = ref.adjoint(g)
    errs = (rell2(V.detach().cpu(), ref.V), rell2(tp.grad.cpu(), gr["positions"]), rell2(tq.grad.cpu(), gr["charges"]),
            relmax(tc.grad.cpu(), gr["cell"]))
    print(f"adjoint {kind} {dtype}: relV={errs[0]:.2e} relGpos={errs[1]:.2e} relGq={errs[2]:.2e} relGcell={errs[3]:.2e}")
    assert errs[0] < tolV and errs[1] < tolG and errs[2] < 10 * tolV and errs[3] < 10 * tolG, errs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_replay_with_moving_atoms(dtype):
    """One captured step, three replays; before each the atoms move by a few mesh spacings (plus a jitter of their own), so they
    change bricks and the per-brick counts change: a slot that still holds the last replay's atom while the count covers it shows
    here and nowhere else."""
    ref0 = box_ref("P3M", 5)
    tolV, tolG = tols(dtype)
    calc = make_calc("P3M", 5, dtype)
    step = check_graphed(calc, ref0, dtype)
    rng = np.random.default_rng(303)
    pos = ref0.pos
    for shift in ([2.3, -3.7, 5.1], [-4.4, 1.9, 2.6], [7.2, 6.3, -8.5]):
        pos = pos + np.array(shift) * H + rng.uniform(-0.1, 0.1, pos.shape)
        ref = Ref("P3M", 5, ref0.q, ref0.cell, pos, ref0.pairs, ref0.S)
        E, F = step(torch.tensor(pos, device=DEV, dtype=dtype))
        assert_route()
        eE, eF = abs(float(E) - ref.E) / ref.E_scale, rell2(F.cpu(), ref.F)
        print(f"replay {dtype} shift={shift}: relE={eE:.2e} relF={eF:.2e}")
        assert eE < tolV and eF < tolG, (shift, eE, eF)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_contract_step_and_both_rider_kinds(dtype):
    """The whole contract -- E, F, dE/dq, dE/dcell against the oracle at the tolerances of tests/test_gpu_contract.py (largest
    component: 1e-9 / 2e-4) -- two ways.  ``GraphedEnergyForces(charge_gradient=True, cell_gradient=True)``: this step keeps the
    real charge mesh (no ``MIPME_FWD_RHO_MESH_UNUSED``), so its spread is the owner-computes brick spread and the binning pass
    must be the one-pass kernel: asserted.  The eager calculator with a differentiable cell and ``weighted_sum``: the plane spread
    runs, the gather tail forms dE/dcell, and the cell riders and the slot riders share the inverse plane launch."""
    ref = box_ref("P3M", 5)
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    tq, tc, tp, ti, tS = tensors(ref, dtype)
    calc = make_calc("P3M", 5, dtype)
    step = tpa.GraphedEnergyForces(calc, tq, tc, tp, ti, tS, charge_gradient=True, cell_gradient=True)
    assert step._fused_contract
    for _ in range(2):
        E, F, dq, dc = step()
        assert_route(deferred=False)
        errs = (abs(float(E) - ref.E) / abs(ref.E), relmax(F.cpu(), ref.F), relmax(dq.cpu(), ref.dq), relmax(dc.cpu(), ref.dcell))
        print(f"contract graph {dtype}: relE={errs[0]:.2e} relF={errs[1]:.2e} rel_dq={errs[2]:.2e} rel_dcell={errs[3]:.2e}")
        assert max(errs) <= tol, errs
    tq, tc, tp, ti, tS = tensors(ref, dtype, grad=True)
    tq.requires_grad_(True)
    E = tpa.weighted_sum(calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS, deferred="virtual")), tq)
    assert_route()
    assert (_lib.load().mipme_last_cell_riders() > 0) == DEFERRED  # (the gather tail forms dE/dcell: cell riders on that launch)
    E.backward()
    errs = (abs(float(E.detach()) - ref.E) / abs(ref.E), relmax(-tp.grad.cpu(), ref.F), relmax(tq.grad.cpu(), ref.dq),
            relmax(tc.grad.cpu(), ref.dcell))
    print(f"contract eager {dtype}: relE={errs[0]:.2e} relF={errs[1]:.2e} rel_dq={errs[2]:.2e} rel_dcell={errs[3]:.2e}")
    assert max(errs) <= tol, errs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_forward_forward_backward_then_bricks_route(dtype):
    """Two forward calls of one calculator at different positions, then ``backward()`` on the FIRST result with a random upstream
    gradient (its second spread reads weights, reach codes and the counter snapshot of the first call's bins); then a two-channel
    call of the same calculator on the same mesh -- the owner-computes brick route, which must find everything as the one-pass
    kernel leaves it."""
    ref = box_ref("P3M", 5)
    tolV, tolG = tols(dtype)
    calc = make_calc("P3M", 5, dtype)
    rng = np.random.default_rng(404)
    g = rng.normal(size=ref.q.shape)
    tq, tc, tp, ti, tS = tensors(ref, dtype, grad=True)
    tq.requires_grad_(True)
    V1 = calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    assert_route()
    pos2 = ref.pos + np.array([3.3, -2.1, 4.7]) * H
    tp2 = torch.tensor(pos2, device=DEV, dtype=dtype)
    V2 = calc(tq.detach(), tc.detach(), tp2, ti, tpa.pair_distances(tp2, ti, tc.detach(), tS))
    assert_route()
    (V1 * torch.tensor(g, device=DEV, dtype=dtype)).sum().backward()
    gr = ref.adjoint(g)
    ref2 = Ref("P3M", 5, ref.q, ref.cell, pos2, ref.pairs, ref.S)
    errs = (rell2(V1.detach().cpu(), ref.V), rell2(V2.cpu(), ref2.V), rell2(tp.grad.cpu(), gr["positions"]),
            rell2(tq.grad.cpu(), gr["charges"]), relmax(tc.grad.cpu(), gr["cell"]))
    print(f"fwd fwd bwd {dtype}: " + " ".join(f"{e:.2e}" for e in errs))
    assert errs[0] < tolV and errs[1] < tolV and errs[2] < tolG and errs[3] < 10 * tolV and errs[4] < 10 * tolG, errs
    # two channels: the bricks route (no plane spread), one pass
    q2 = np.concatenate([ref.q, rng.normal(size=ref.q.shape)], 1)
    dist, _ = O.pair_distances(ref.pos, ref.cell, ref.pairs, ref.S)
    Vo2 = O.forward(O.PotentialSpec("coulomb", 1, 1.0, 1.0), "P3M", 5, H, q2, ref.cell, ref.pos, ref.pairs, dist)
    tpd = tp.detach()
    Vc = calc(torch.tensor(q2, device=DEV, dtype=dtype), tc.detach(), tpd, ti, tpa.pair_distances(tpd, ti, tc.detach(), tS))
    assert_route(deferred=False)
    assert rell2(Vc.cpu(), Vo2) < tolV
    # ... and a deferred call again behind it
    V3 = calc(tq.detach(), tc.detach(), tpd, ti, tpa.pair_distances(tpd, ti, tc.detach(), tS))
    assert_route()
    assert rell2(V3.cpu(), ref.V) < tolV
