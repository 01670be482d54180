"""Inverse (y,z) planes split over S workgroups per plane (``MIPME_INV_PLANE_SPLIT`` = 1, 2, 4; docs/SWITCHES.md, docs/KERNELS.md):
workgroup (plane, h) takes one radix-S decimation-in-frequency stage of the y transform, keeps residue h, and finishes the rows
y = S m + h on its own.  What can go wrong is the decimation itself (twiddle, sign and order of the S inputs), the row map of the
store, the shortest transforms (ny = 4 S, nz = 4), ny != nz, the riders that share the launch (slot riders, cell riders), the
default's rule, and a route that quietly falls back.

Every case asserts through ``mipme_last_inverse_split()`` what RAN.  The library reads this switch at every launch, so one
process serves all three settings; ``MIPME_DEFER_SLOTS`` and ``MIPME_PLANE_PARTS`` are read once per process: child processes.

Tolerances.  The transform alone: the relative L2 bound of ``tests/test_gpu_parity.py::test_fused_convolution`` (1e-11 in fp64,
2e-4 in fp32), against ``numpy.fft`` in float64, for every S on its own.  The step: those of tests/test_gpu_deferred_slots.py
(energy 1e-11 / 2e-5, forces 1e-10 / 2e-4, the contract's largest component 1e-9 / 2e-4)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from oracle import pme_numpy as O
from torchpme_amd import _lib, ops, workloads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = (1, 2, 4)
DTYPES = [torch.float64, torch.float32]
DEFERRED = (os.environ.get("MIPME_DEFER_SLOTS", "1") != "0" and os.environ.get("MIPME_PLANE_SPREAD", "1") != "0"
            and os.environ.get("MIPME_DETERMINISTIC", "0") == "0" and os.environ.get("MIPME_SPARSE_FORCE", "0") == "0")


def rell2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(autouse=True)
def _restore_switch():
    old = os.environ.get("MIPME_INV_PLANE_SPLIT")
    yield
    if old is None:
        os.environ.pop("MIPME_INV_PLANE_SPLIT", None)
    else:
        os.environ["MIPME_INV_PLANE_SPLIT"] = old


def set_split(s):
    os.environ["MIPME_INV_PLANE_SPLIT"] = str(s)


def last_split():
    return _lib.load().mipme_last_inverse_split()


def expected_split(s, ny):
    return s if s > 1 and ny >= 4 * s else 1


# ---- 1. the transform alone -------------------------------------------------------------------------------------------------
def even_filter(ns):
    """A filter table that differs at every k and is even in every frequency (a real, Hermitian-consistent product)."""
    fx, fy = np.fft.fftfreq(ns[0], 1 / ns[0]), np.fft.fftfreq(ns[1], 1 / ns[1])
    fz = np.arange(ns[2] // 2 + 1, dtype=np.float64)
    return 0.9 + 0.4 * np.cos(0.9 * fx)[:, None, None] * np.cos(1.7 * fy)[None, :, None] * np.cos(0.6 * fz)[None, None, :]


def convolve(ns, dtype, G, seed=0):
    """``mipme_kspace_forward`` without bins and without ``rho_hat``: scatter spread -> fused convolution (forward planes, x stage,
    INVERSE PLANES) -> gather.  Returns the charge mesh the convolution read and the mesh it wrote."""
    rng = np.random.default_rng(seed)
    cell = np.diag([float(n) for n in ns])
    geom = ops.MeshGeometry(cell, ns, _lib.P3M, 3)
    md = geom.desc(1)
    n_atoms = int(min(20000, 2 * np.prod(ns)))
    t = lambda a: torch.tensor(a, dtype=dtype, device=DEV)  # noqa: E731
    pos, q = t(rng.uniform(0, 1, (n_atoms, 3)) * np.array(ns)), t(rng.normal(size=(n_atoms, 1)))
    Gt = t(G)
    plan = _lib.get_plan(DEV, dtype, ns, 1)
    assert plan.xfused
    pot = _lib.PotentialDesc(kind=_lib.COULOMB, exponent=1, smearing=1.0, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1)
    empty = lambda shape, dt=dtype: torch.empty(shape, dtype=dt, device=DEV)  # noqa: E731
    rho, phi = empty((1,) + tuple(ns)), empty((1,) + tuple(ns))
    hat_work, dc, out = empty((1, geom.n_half), _lib.complex_dtype(dtype)), empty((1,)), empty((n_atoms, 1))
    args = _lib.KspaceForwardArgs(plan=plan.handle, stream=_lib.current_stream(DEV), dtype=_lib.dtype_code(dtype), accumulate_out=0,
                                  mesh=C.pointer(md), pot=C.pointer(pot), n_atoms=n_atoms, positions=pos.data_ptr(),
                                  charges=q.data_ptr(), G=Gt.data_ptr(), rho_mesh=rho.data_ptr(), hat_work=hat_work.data_ptr(),
                                  phi_mesh=phi.data_ptr(), dc=dc.data_ptr(), out_lr=out.data_ptr(), flags=0)
    _lib.check(_lib.load().mipme_kspace_forward(C.byref(args)))
    torch.cuda.synchronize()
    return rho[0].cpu().numpy(), phi[0].cpu().numpy()


def convolution_error(ns, dtype, G):
    rho, phi = convolve(ns, dtype, G)
    want = np.fft.irfftn(np.fft.rfftn(rho.astype(np.float64)) * G, s=ns) * np.prod(ns)  # (both transforms un-normalised)
    return rell2(phi, want)


MESHES = [(16, 8, 8), (16, 16, 4), (16, 32, 64), (32, 64, 16), (64, 64, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ns", MESHES, ids=lambda ns: "x".join(map(str, ns)))
def test_transform_against_numpy(ns, dtype):
    """ny = 4 S (the smallest routed: 8 at S = 2, 16 at S = 4), ny = 2 S (8 at S = 4: must fall back, and says so), nz = 4 (the
    shortest z row), ny != nz in both orders, and the benchmark's 64^3; G = 1 and a table that differs at every k."""
    tol = 1e-11 if dtype == torch.float64 else 2e-4
    errs = {}
    for s in SPLITS:
        set_split(s)
        for name, G in (("ones", np.ones((ns[0], ns[1], ns[2] // 2 + 1))), ("even", even_filter(ns))):
            errs[s, name] = convolution_error(ns, dtype, G)
            assert last_split() == expected_split(s, ns[1]), (s, ns, last_split())
    print(f"inverse split {ns} {dtype}: " + "  ".join(f"S={s} {name} {e:.2e}" for (s, name), e in errs.items()))
    assert max(errs.values()) < tol, errs


# ---- 2. the step ----------------------------------------------------------------------------------------------------------------
class Sys:
    """A system, its calculator arguments and what the step must return."""

    def __init__(self, scheme, order, h, smearing, pos, cell, q, pairs, S, E, F, dq, dcell, sample=None):
        self.scheme, self.order, self.h, self.smearing = scheme, order, h, smearing
        self.pos, self.cell, self.q, self.pairs, self.S = pos, cell, q, pairs, S
        self.E, self.F, self.dq, self.dcell, self.sample = E, F, dq, dcell, sample

    def calc(self, dtype):
        Calc = tpa.P3MCalculator if self.scheme == "P3M" else tpa.PMECalculator
        return Calc(tpa.CoulombPotential(smearing=self.smearing), mesh_spacing=self.h, interpolation_nodes=self.order).to(dtype)

    def tensors(self, dtype, grad=False):
        t = lambda a, g=False: torch.tensor(a, device=DEV, dtype=dtype, requires_grad=g)  # noqa: E731
        return t(self.q, grad), t(self.cell, grad), t(self.pos, grad), torch.tensor(self.pairs, device=DEV), t(self.S)

    def pick(self, a):
        a = np.asarray(a.detach().cpu(), dtype=np.float64)
        return a if self.sample is None else a[self.sample]


@functools.lru_cache(maxsize=None)
def golden_system(name):
    """The water (31 944 atoms, P3M 5, 64^3) and ionic (8 000 ions, P3M 4, 32^3) boxes of tests/golden/workloads.npz: energy,
    dE/dcell and 256 sampled rows of the forces and of dE/dq."""
    w = {"water": workloads.water_box, "ionic": workloads.ionic_box}[name]()
    z = np.load(os.path.join(ROOT, "tests", "golden", "workloads.npz"))
    return Sys(w.scheme, w.order, w.mesh_spacing, w.smearing, w.positions, w.cell, w.charges, w.pairs, w.shifts,
               float(z[f"{name}_energy"]), z[f"{name}_force_sample"], z[f"{name}_charge_grad_sample"][:, None], z[f"{name}_cell_grad"],
               z[f"{name}_sample"])


@functools.lru_cache(maxsize=None)
def lattice_system():
    """No committed golden uses Lagrange interpolation on a mesh the plane route takes: the 1 728-atom lattice of
    tests/test_gpu_deferred_slots.py (24 A cube, 64^3 mesh), PME with 4 nodes, against the oracle (computed once)."""
    rng = np.random.default_rng(101)
    g = (np.arange(12) + 0.5) * 2.0
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.3, 0.3, (1728, 3))
    cell = 24.0 * np.eye(3)
    q = rng.normal(size=(1728, 1))
    q -= q.mean()
    h = 2 * 24.0 / 62
    pairs, S, _ = tpa.neighbor_list(pos, cell, 4.0)
    dist, _ = O.pair_distances(pos, cell, pairs, S)
    V, cache = O.forward(O.PotentialSpec("coulomb", 1, 1.0, 1.0), "Lagrange", 4, h, q, cell, pos, pairs, dist, return_cache=True)
    gr = O.backward(cache, q)
    gpos_d, gcell_d = O.pair_distances_backward(pos, cell, pairs, S, gr["dist"])
    return Sys("PME", 4, h, 1.0, pos, cell, q, pairs, S, float((V * q).sum()), -(gr["positions"] + gpos_d), gr["charges"] + V,
               gr["cell"] + gcell_d)


def system(name):
    return lattice_system() if name == "lattice" else golden_system(name)


def check_step(sy, dtype, s, contract, riders):
    """One captured step, two replays, each against the goldens.  (Bytes are compared in the child processes below, where the
    launches in front of the inverse planes are reproducible themselves.)"""
    tolE, tolF = (1e-11, 1e-10) if dtype == torch.float64 else (2e-5, 2e-4)
    tolC = 1e-9 if dtype == torch.float64 else 2e-4
    tq, tc, tp, ti, tS = sy.tensors(dtype)
    set_split(s)
    step = tpa.GraphedEnergyForces(sy.calc(dtype), tq, tc, tp, ti, tS, charge_gradient=contract, cell_gradient=contract)
    for _ in range(2):
        out = step()
        torch.cuda.synchronize()
        assert last_split() == s, (last_split(), s)  # (32^3 and 64^3 meshes: ny >= 16)
        eE = abs(float(out[0]) - sy.E) / abs(sy.E)
        eF = rell2(sy.pick(out[1]), sy.F)
        print(f"step {dtype} S={s} contract={contract}: relE={eE:.2e} relF={eF:.2e}", end="")
        assert eE < tolE and eF < tolF, (eE, eF)
        if contract:
            errs = (relmax(sy.pick(out[1]), sy.F), relmax(sy.pick(out[2]), sy.dq), relmax(out[3].cpu(), sy.dcell))
            print(f" relmaxF={errs[0]:.2e} rel_dq={errs[1]:.2e} rel_dcell={errs[2]:.2e}", end="")
            assert max(errs) <= tolC, errs
        print()
    if riders and not contract:  # (the plain step leaves its slots to riders of the inverse plane launch)
        assert (_lib.load().mipme_last_slot_fill() > 0) == DEFERRED


@pytest.mark.parametrize("contract", [False, True], ids=["EF", "EFqc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["water", "ionic", "lattice"])
def test_step_against_the_goldens(name, dtype, contract):
    """``GraphedEnergyForces`` with P3M 5 (water), P3M 4 (ionic) and Lagrange 4 (lattice), without and with ``charge_gradient`` /
    ``cell_gradient`` (the cell riders share the split launch), S = 1, 2, 4."""
    sy = system(name)
    for s in SPLITS:
        check_step(sy, dtype, s, contract, riders=name == "lattice")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_eager_contract_with_both_rider_kinds(dtype):
    """The eager calculator with a differentiable cell and ``weighted_sum``: cell riders AND slot riders behind the split planes."""
    sy = lattice_system()
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    for s in SPLITS:
        set_split(s)
        tq, tc, tp, ti, tS = sy.tensors(dtype, grad=True)
        E = tpa.weighted_sum(sy.calc(dtype)(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS, deferred="virtual")), tq)
        assert last_split() == s
        assert (_lib.load().mipme_last_slot_fill() > 0) == DEFERRED and (_lib.load().mipme_last_cell_riders() > 0) == DEFERRED
        E.backward()
        errs = (abs(float(E.detach()) - sy.E) / abs(sy.E), relmax(-tp.grad.cpu(), sy.F), relmax(tq.grad.cpu(), sy.dq),
                relmax(tc.grad.cpu(), sy.dcell))
        print(f"eager contract {dtype} S={s}: relE={errs[0]:.2e} relF={errs[1]:.2e} rel_dq={errs[2]:.2e} rel_dcell={errs[3]:.2e}")
        assert max(errs) <= tol, errs


_CHILD = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import torchpme_amd as tpa
from torchpme_amd import _lib
d = np.load(sys.argv[2])
out = {}
for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
    t = lambda a: torch.tensor(a, device="cuda:0", dtype=dtype)
    for s in (1, 2, 4):
        os.environ["MIPME_INV_PLANE_SPLIT"] = str(s)
        calc = tpa.PMECalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=float(d["h"]), interpolation_nodes=4).to(dtype)
        step = tpa.GraphedEnergyForces(calc, t(d["q"]), t(d["cell"]), t(d["pos"]), torch.tensor(d["pairs"], device="cuda:0"), t(d["S"]))
        E, F = step()
        E1, F1 = E.cpu().numpy().copy(), F.cpu().numpy().copy()
        E, F = step()
        k = f"{name}_{s}"
        out["split_" + k], out["fill_" + k] = _lib.load().mipme_last_inverse_split(), _lib.load().mipme_last_slot_fill()
        out["replay_" + k] = bool(np.array_equal(E1, E.cpu().numpy()) and np.array_equal(F1, F.cpu().numpy()))
        out["E_" + k], out["F_" + k] = E1, F1
        # the whole contract: the graphed step (cell riders behind the planes, one-pass binning) and the eager calculator with a
        # differentiable cell (cell riders, and slot riders unless MIPME_DEFER_SLOTS=0)
        step = tpa.GraphedEnergyForces(calc, t(d["q"]), t(d["cell"]), t(d["pos"]), torch.tensor(d["pairs"], device="cuda:0"), t(d["S"]),
                                       charge_gradient=True, cell_gradient=True)
        E, F, dq, dc = step()
        out["csplit_" + k] = _lib.load().mipme_last_inverse_split()
        out["cE_" + k], out["cF_" + k], out["cdq_" + k], out["cdc_" + k] = (x.cpu().numpy().copy() for x in (E, F, dq, dc))
        tq, tc, tp = (t(d[n]).requires_grad_(True) for n in ("q", "cell", "pos"))
        ti = torch.tensor(d["pairs"], device="cuda:0")
        E = tpa.weighted_sum(calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, t(d["S"]), deferred="virtual")), tq)
        out["esplit_" + k], out["efill_" + k] = _lib.load().mipme_last_inverse_split(), _lib.load().mipme_last_slot_fill()
        E.backward()
        out["eE_" + k], out["eF_" + k], out["edq_" + k], out["edc_" + k] = (x.detach().cpu().numpy().copy()
                                                                            for x in (E, -tp.grad, tq.grad, tc.grad))
np.savez(sys.argv[3], **out)
"""


def test_bytes_across_replays_and_processes_and_the_one_pass_binning(tmp_path):
    """Three fresh processes with ``MIPME_PLANE_PARTS=1`` (the launches in front of the inverse planes are then reproducible in
    fp32: tests/test_gpu_deferred_slots.py), all S in each: two with the deferred slot fill -- the fp32 energy and forces of two
    replays and of the two processes are the same bytes for a fixed S -- and one with ``MIPME_DEFER_SLOTS=0`` (the split planes
    without slot riders), which must give the goldens' figures like the others.  Every process also returns the whole contract
    (E, F, dE/dq, dE/dcell) from the graphed step and from the eager calculator: with ``MIPME_DEFER_SLOTS=0`` these are the cell
    riders behind split planes that carry no slot riders."""
    sy = lattice_system()
    np.savez(tmp_path / "in.npz", q=sy.q, cell=sy.cell, pos=sy.pos, pairs=sy.pairs, S=sy.S, h=sy.h)
    runs = [("a", "1"), ("b", "1"), ("c", "0")]
    procs = [subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / f"{tag}.npz")],
                              env=dict(os.environ, MIPME_PLANE_PARTS="1", MIPME_DEFER_SLOTS=defer), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for tag, defer in runs]
    for p in procs:
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
    res = {tag: np.load(tmp_path / f"{tag}.npz") for tag, _ in runs}
    for name, tolE, tolF in (("f32", 2e-5, 2e-4), ("f64", 1e-11, 1e-10)):
        for s in SPLITS:
            k = f"{name}_{s}"
            for tag, defer in runs:
                r = res[tag]
                assert int(r["split_" + k]) == s and (int(r["fill_" + k]) > 0) == (defer == "1" and DEFERRED), (tag, k)
                eE, eF = abs(float(r["E_" + k]) - sy.E) / abs(sy.E), rell2(r["F_" + k], sy.F)
                assert eE < tolE and eF < tolF, (tag, k, eE, eF)
                tolC = 1e-9 if name == "f64" else 2e-4
                for pre in ("c", "e"):
                    assert int(r[pre + "split_" + k]) == s, (tag, pre, k)
                    errs = (abs(float(r[pre + "E_" + k]) - sy.E) / abs(sy.E), relmax(r[pre + "F_" + k], sy.F),
                            relmax(r[pre + "dq_" + k], sy.dq), relmax(r[pre + "dc_" + k], sy.dcell))
                    assert max(errs) <= tolC, (tag, pre, k, errs)
                assert (int(r["efill_" + k]) > 0) == (defer == "1" and DEFERRED), (tag, k)
            if name == "f32":
                assert all(bool(res[tag]["replay_" + k]) for tag, _ in runs), k
                assert np.array_equal(res["a"]["E_" + k], res["b"]["E_" + k]) and np.array_equal(res["a"]["F_" + k], res["b"]["F_" + k]), k


def test_the_default_follows_the_number_of_planes():
    """Without the switch: the largest S of 4, 2 with at most 128 plane workgroups (S nx <= 128) and ny >= 4 S."""
    os.environ.pop("MIPME_INV_PLANE_SPLIT", None)
    for ns, want in (((64, 64, 64), 2), ((32, 64, 16), 4), ((32, 8, 8), 2), ((128, 16, 16), 1), ((16, 4, 8), 1)):
        assert convolution_error(ns, torch.float32, even_filter(ns)) < 2e-4
        assert last_split() == want, (ns, last_split())
    os.environ["MIPME_INV_PLANE_SPLIT"] = "3"  # (not a value: the default)
    convolve((64, 64, 64), torch.float32, even_filter((64, 64, 64)))
    assert last_split() == 2


# ---- 3. fall-backs --------------------------------------------------------------------------------------------------------------
def test_a_frame_batch_keeps_one_workgroup_per_plane():
    """Two frames of the lattice box (64^3 meshes) in one ``GraphedFrameBatch``: split 1, although a single mesh of that size splits."""
    sy = lattice_system()
    set_split(4)
    tq, tc, tp, ti, tS = sy.tensors(torch.float32)
    calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=sy.h, interpolation_nodes=5).to(torch.float32)
    tpa.GraphedEnergyForces(calc, tq, tc, tp, ti, tS)()
    assert last_split() == 4
    batch = tpa.GraphedFrameBatch(calc, [(tq, tc, tp, ti, tS), (tq, tc, tp.clone(), ti, tS)])
    assert batch.ns == (64, 64, 64)
    E, _ = batch()
    torch.cuda.synchronize()
    assert last_split() == 1
    assert abs(float(E[0]) - float(E[1])) <= 1e-5 * abs(float(E[0]))


@pytest.mark.parametrize("ns", [(4, 256, 256), (4, 128, 128), (16, 12, 16)], ids=["256-wide", "128-wide", "ny=12"])
def test_large_planes_and_hipfft_planes_keep_their_kernels(ns):
    """Planes beyond one workgroup's LDS (z rows + y columns as two launches), planes beyond 64 KB of LDS (the ones the plane spread
    takes in bands) and a ny that is no power of two (hipFFT planes): split 1 whatever the switch says, and the right numbers."""
    for s in (2, 4):
        set_split(s)
        assert convolution_error(ns, torch.float32, even_filter(ns)) < 2e-4
        assert last_split() == 1
