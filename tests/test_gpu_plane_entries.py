"""Plane-list entries that carry the y / z weights, and the list lookup of the plane workgroups without a scan
(csrc/bricks_device.h ``plane_entry_words``, ``plane_spread_yz_body``; docs/KERNELS.md "Plane-list entries").

The binning pass writes, per atom, the packed stencil reference point, ``charge * w_x[0..n)``, ``w_y[0..n)`` and ``w_z[0..n)``
(fp32, n <= 5; every other (n, dtype) keeps the entry with the two offsets and evaluates the weights in the plane workgroup).
A plane workgroup takes its lists as one sequence of entries; the list a lane's entry belongs to is the wavefront's first list
plus the list boundaries inside the wavefront's 64 entries.  What can go wrong: spans that cross many (empty) lists, lists at
capacity with the rest in the plane overflow list, totals that are no multiple of the workgroup, slices of several parts per
plane that begin inside a list, the banded body, the frame batches' kernel, both entry formats, non-finite input.

Every case asserts through ``mipme_last_cosched_kernel()`` (and ``mipme_plane_spread_parts``) that a plane kernel ran, compares
with oracle/pme_numpy.py at the tolerances of tests/test_gpu_parity.py ``test_bin_overflow_region`` (potentials and energy /
gradients 1e-11 / 1e-10 in fp64, 2e-5 / 2e-4 in fp32, the energy relative to |E|) and, in child processes (the library reads its
switches once), the deferred against the one-pass binning route at one part per plane: bit for bit in fp32 (fixed-point plane
sums do not depend on the order of arrival), 1e-12 relative in fp64 -- as tests/test_gpu_deferred_slots.py does.

Meshes are 32^3 unless said: the smallest the plane route accepts.  (The plane lists want nx >= 16, but the bins they live in
want more than two bricks of 8 along every axis -- ``bricks_supported`` -- and the transforms a power of two: on a 16^3 mesh no
plane kernel runs at all, and every case has to see one run.)"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from oracle import pme_numpy as O
from torchpme_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: the library's default routes (docs/SWITCHES.md): with one of these switched no plane kernel is expected
PLANES = (os.environ.get("MIPME_PLANE_SPREAD", "1") != "0" and os.environ.get("MIPME_DETERMINISTIC", "0") == "0"
          and os.environ.get("MIPME_SPARSE_FORCE", "0") == "0")
BANDS = PLANES and os.environ.get("MIPME_PLANE_BANDS", "1") != "0"
L_BOX = 24.0
H32 = 2 * L_BOX / 30  # 2 L / h + 1 = 31 -> 32^3 mesh
DTYPES = [torch.float64, torch.float32]
PLANE_KERNELS = ("plane_rows_capped_kernel", "plane_rows_kernel")


def rell2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def tols(dtype):
    return (1e-11, 1e-10) if dtype == torch.float64 else (2e-5, 2e-4)


class Case:
    """One system and its oracle results (computed once, never modified)."""

    def __init__(self, name, pos, cell, q, scheme="P3M", order=5, h=H32, sm=1.0, cutoff=4.0, ns=(32, 32, 32)):
        self.name, self.pos, self.cell, self.q = name, pos, cell, q
        self.scheme, self.order, self.h, self.sm, self.ns = scheme, order, h, sm, ns
        self.pairs, self.S, _ = tpa.neighbor_list(pos, cell, cutoff)
        dist, _ = O.pair_distances(pos, cell, self.pairs, self.S)
        spec = O.PotentialSpec("coulomb", 1, sm, 1.0)
        self.V, cache = O.forward(spec, "P3M" if scheme == "P3M" else "Lagrange", order, h, q, cell, pos, self.pairs, dist,
                                  return_cache=True)
        gr = O.backward(cache, q)
        gpos_d, _ = O.pair_distances_backward(pos, cell, self.pairs, self.S, gr["dist"])
        self.E = float((self.V * q).sum())
        self.F = -(gr["positions"] + gpos_d)

    def calc(self, dtype):
        Calc = tpa.P3MCalculator if self.scheme == "P3M" else tpa.PMECalculator
        return Calc(tpa.CoulombPotential(smearing=self.sm), mesh_spacing=self.h, interpolation_nodes=self.order).to(dtype)

    def tensors(self, dtype, grad=False):
        t = lambda a, g=False: torch.tensor(a, device=DEV, dtype=dtype, requires_grad=g)  # noqa: E731
        return t(self.q), t(self.cell), t(self.pos, grad), torch.tensor(self.pairs, device=DEV), t(self.S)


def neutral(rng, n):
    q = rng.normal(size=(n, 1))
    return q - q.mean()


def uniform_box(rng, n):
    """n atoms on distinct sites of a jittered 12^3 lattice (spacing 2 A: no two atoms closer than 1.4 A), in random order."""
    g = (np.arange(12) + 0.5) * 2.0
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return sites[rng.permutation(len(sites))[:n]] + rng.uniform(-0.3, 0.3, (n, 3))


@functools.lru_cache(maxsize=None)
def case(name):
    cell = np.eye(3) * L_BOX
    if name == "sparse40":  # 40 atoms on 32 x 8 sub-lists: a wavefront's 64 entries cross up to 40 list boundaries
        rng = np.random.default_rng(401)
        return Case(name, uniform_box(rng, 40), cell, neutral(rng, 40))
    if name == "sheet3000":
        # 3 000 atoms whose x lies inside ONE mesh cell (0.75 A wide; the cell of node 8 is [5.625, 6.375)), a jittered 50 x 60
        # lattice in (y, z): one x plane's sub-lists (4 x mean + 32 = 80 entries each) take 8 x 80 of them, the plane overflow
        # list the other ~2 400; neither is a multiple of the workgroup's 512
        rng = np.random.default_rng(402)
        gy, gz = np.meshgrid((np.arange(50) + 0.5) * L_BOX / 50, (np.arange(60) + 0.5) * L_BOX / 60, indexing="ij")
        pos = np.stack([rng.uniform(5.7, 6.3, 3000), gy.ravel() + rng.uniform(-0.1, 0.1, 3000),
                        gz.ravel() + rng.uniform(-0.08, 0.08, 3000)], 1)
        return Case(name, pos[rng.permutation(3000)], cell, neutral(rng, 3000), cutoff=2.5)
    if name == "uniform1500":
        rng = np.random.default_rng(403)
        return Case(name, uniform_box(rng, 1500), cell, neutral(rng, 1500))
    if name.startswith("triclinic"):  # triclinic-P3M5, -P3M4, -PME4
        scheme, order = name.split("-")[1][:3], int(name[-1])
        rng = np.random.default_rng(404)
        tri = cell + np.array([[0, 0, 0], [1.9, 0, 0], [-1.2, 2.6, 0]])
        pos = (uniform_box(rng, 700) / L_BOX) @ tri
        return Case(name, pos, tri, neutral(rng, 700), scheme=scheme, order=order)
    if name == "banded3000":  # a 32 x 128 x 128 mesh: planes of 128 x 128 are spread in bands of rows (tests/test_gpu_round6.py)
        rng = np.random.default_rng(405)
        diag = np.array([10.0, 40.0, 40.0])
        frac = rng.uniform(0, 1, (3000, 3))
        frac[:8, 1] = [0.0, 0.001, 0.999, 0.2499, 0.2501, 0.5, 0.7499, 0.7501]  # stencils that straddle band boundaries
        return Case(name, frac @ np.diag(diag), np.diag(diag), neutral(rng, 3000), h=0.7, sm=1.2, cutoff=3.0, ns=(32, 128, 128))
    raise KeyError(name)


ROUTE_CASES = ["sparse40", "sheet3000", "uniform1500", "triclinic-P3M5", "triclinic-P3M4", "triclinic-PME4", "banded3000"]


def assert_plane_kernel(c, calc, dtype, n_atoms, banded=False):
    """A plane kernel ran (not the bricks), on the mesh the case is meant for; returns the parts per plane."""
    geom = calc._cache[6]
    assert geom.ns == c.ns, geom.ns
    if not (BANDS if banded else PLANES):
        return 0
    lib = _lib.load()
    assert lib.mipme_last_cosched_kernel().decode() in PLANE_KERNELS, lib.mipme_last_cosched_kernel()
    parts = lib.mipme_plane_spread_parts(C.byref(geom.desc(1)), n_atoms, _lib.dtype_code(dtype))
    assert parts >= 1, parts
    return parts


def check_against_oracle(c, dtype):
    tolV, tolG = tols(dtype)
    banded = c.ns != (32, 32, 32)
    calc = c.calc(dtype)
    tq, tc, tp, ti, tS = c.tensors(dtype, grad=True)
    V = calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    parts = assert_plane_kernel(c, calc, dtype, len(c.pos), banded)
    assert not banded or parts <= 1
    E = tpa.weighted_sum(V, tq)
    E.backward()
    eV, eE, eF = rell2(V.detach().cpu(), c.V), abs(float(E.detach()) - c.E) / abs(c.E), rell2(-tp.grad.cpu(), c.F)
    print(f"{c.name} eager {dtype} parts={parts}: relV={eV:.2e} relE={eE:.2e} relF={eF:.2e}")
    assert eV < tolV and eE < tolV and eF < tolG, (eV, eE, eF)
    tq, tc, tp, ti, tS = c.tensors(dtype)
    E, F = tpa.GraphedEnergyForces(calc, tq, tc, tp, ti, tS)()
    assert_plane_kernel(c, calc, dtype, len(c.pos), banded)
    eE, eF = abs(float(E) - c.E) / abs(c.E), rell2(F.cpu(), c.F)
    print(f"{c.name} graphed {dtype}: relE={eE:.2e} relF={eF:.2e}")
    assert eE < tolV and eF < tolG, (eE, eF)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["sparse40", "sheet3000", "uniform1500"])
def test_lists_empty_full_and_sliced(name, dtype):
    """Cases 1-3 at the library's default parts per plane (2: the second part's slice begins inside a list): nearly empty lists,
    lists at capacity + the plane overflow list + a ragged last batch, uniformly filled lists."""
    check_against_oracle(case(name), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["triclinic-P3M5", "triclinic-P3M4", "triclinic-PME4"])
def test_orders_schemes_and_precisions(name, dtype):
    """P3M 5 and 4 and Lagrange 4 nodes in a triclinic cell, fp32 and fp64: every entry size, and both entry formats."""
    check_against_oracle(case(name), dtype)


def test_banded_body():
    """A 32 x 128 x 128 mesh, fp32: the lists of a band are the y slices of its rows and one more on either side."""
    check_against_oracle(case("banded3000"), torch.float32)


_CHILD = r"""
import ctypes
import json
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import torchpme_amd as tpa
from torchpme_amd import _lib
d = np.load(sys.argv[2])
meta = json.loads(str(d["meta"]))
lib = _lib.load()
out = {}
for i, m in enumerate(meta):
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        t = lambda a: torch.tensor(a, device="cuda:0", dtype=dtype)
        Calc = tpa.P3MCalculator if m["scheme"] == "P3M" else tpa.PMECalculator
        calc = Calc(tpa.CoulombPotential(smearing=m["sm"]), mesh_spacing=m["h"], interpolation_nodes=m["order"]).to(dtype)
        q, cell, pos, ti, tS = t(d[f"{i}_q"]), t(d[f"{i}_cell"]), t(d[f"{i}_pos"]), torch.tensor(d[f"{i}_pairs"], device="cuda:0"), t(d[f"{i}_S"])
        pg = pos.clone().requires_grad_(True)  # (force sums wanted: the pair sum is co-scheduled with the spread)
        V = calc(q, cell, pg, ti, tpa.pair_distances(pg, ti, cell, tS)).detach()
        k = f"{i}_{name}_"
        out[k + "fill_eager"], out[k + "kernel_eager"] = lib.mipme_last_slot_fill(), lib.mipme_last_cosched_kernel().decode()
        E, F = tpa.GraphedEnergyForces(calc, q, cell, pos, ti, tS)()
        out[k + "fill_graph"], out[k + "kernel_graph"] = lib.mipme_last_slot_fill(), lib.mipme_last_cosched_kernel().decode()
        out[k + "parts"] = lib.mipme_plane_spread_parts(ctypes.byref(calc._cache[6].desc(1)), len(d[f"{i}_pos"]), _lib.dtype_code(dtype))
        out[k + "V"], out[k + "E"], out[k + "F"] = V.cpu().numpy(), E.cpu().numpy(), F.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


@functools.lru_cache(maxsize=None)
def route_results():
    """ROUTE_CASES in three fresh processes, started together: (parts per plane, MIPME_DEFER_SLOTS) = (1, 1), (1, 0), (2, 1)."""
    tmp = tempfile.mkdtemp(prefix="plane_entries_")
    data = {"meta": json.dumps([dict(scheme=case(n).scheme, order=case(n).order, h=case(n).h, sm=case(n).sm) for n in ROUTE_CASES])}
    for i, n in enumerate(ROUTE_CASES):
        c = case(n)
        data.update({f"{i}_q": c.q, f"{i}_cell": c.cell, f"{i}_pos": c.pos, f"{i}_pairs": c.pairs, f"{i}_S": c.S})
    np.savez(os.path.join(tmp, "in.npz"), **data)
    procs = {}
    for parts, defer in (("1", "1"), ("1", "0"), ("2", "1")):
        env = dict(os.environ, MIPME_PLANE_PARTS=parts, MIPME_DEFER_SLOTS=defer)
        out = os.path.join(tmp, f"out_{parts}_{defer}.npz")
        procs[parts, defer] = (subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, os.path.join(tmp, "in.npz"), out], env=env,
                                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out)
    res = {}
    for key, (p, out) in procs.items():
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
        res[key] = np.load(out)
    return res


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_deferred_against_one_pass_bit_for_bit(name):
    """One part per plane: the lean binning pass (two more ``weights_1d`` calls for the entry) against the one-pass pass (which
    holds the three weight vectors already, as staged rows above 100 000 atoms): the same entries, so the same fp32 results bit for
    bit; the fp64 plane sums (``ds_add_f64``) depend on the order of arrival: 1e-12.  Both are the oracle's at the tolerances above."""
    res, i, c = route_results(), ROUTE_CASES.index(name), case(name)
    a, b = res["1", "1"], res["1", "0"]
    for prec in ("f32", "f64"):
        for how in ("eager", "graph"):
            if PLANES and (BANDS or c.ns == (32, 32, 32)):
                assert str(a[f"{i}_{prec}_kernel_{how}"]) in PLANE_KERNELS and str(b[f"{i}_{prec}_kernel_{how}"]) in PLANE_KERNELS
                assert int(a[f"{i}_{prec}_fill_{how}"]) > 0 and int(b[f"{i}_{prec}_fill_{how}"]) == 0
                assert int(a[f"{i}_{prec}_parts"]) == 1
    for k in ("V", "E", "F"):
        x, y = a[f"{i}_f32_{k}"], b[f"{i}_f32_{k}"]
        assert np.array_equal(x, y), (name, k, np.abs(x - y).max())
        assert relmax(a[f"{i}_f64_{k}"], b[f"{i}_f64_{k}"]) <= 1e-12, (name, k)
    for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        tolV, tolG = tols(dtype)
        errs = (rell2(a[f"{i}_{prec}_V"], c.V), abs(float(a[f"{i}_{prec}_E"]) - c.E) / abs(c.E), rell2(a[f"{i}_{prec}_F"], c.F))
        print(f"{name} {prec} one part per plane: relV={errs[0]:.2e} relE={errs[1]:.2e} relF={errs[2]:.2e}")
        assert errs[0] < tolV and errs[1] < tolV and errs[2] < tolG, errs


@pytest.mark.parametrize("prec,dtype", [("f64", torch.float64), ("f32", torch.float32)])
def test_one_and_two_parts_per_plane(prec, dtype):
    """Case 3 with 1 and with 2 workgroups per plane: the second part's slice [lo, hi) of the plane's entries begins inside a list
    (1 500 atoms, 40 lists per plane: ~235 entries, cut at ~117).  Each against the oracle; and against each other the fp32
    potentials differ only by the rounding of two partial plane sums instead of one."""
    res, i, c = route_results(), ROUTE_CASES.index("uniform1500"), case("uniform1500")
    tolV, tolG = tols(dtype)
    for parts in ("1", "2"):
        r = res[parts, "1"]
        if PLANES:
            assert int(r[f"{i}_{prec}_parts"]) == int(parts)
            assert str(r[f"{i}_{prec}_kernel_eager"]) in PLANE_KERNELS and str(r[f"{i}_{prec}_kernel_graph"]) in PLANE_KERNELS
        errs = (rell2(r[f"{i}_{prec}_V"], c.V), abs(float(r[f"{i}_{prec}_E"]) - c.E) / abs(c.E), rell2(r[f"{i}_{prec}_F"], c.F))
        print(f"uniform1500 {prec} parts={parts}: relV={errs[0]:.2e} relE={errs[1]:.2e} relF={errs[2]:.2e}")
        assert errs[0] < tolV and errs[1] < tolV and errs[2] < tolG, errs
    assert rell2(res["1", "1"][f"{i}_{prec}_V"], res["2", "1"][f"{i}_{prec}_V"]) < tolV


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_frame_batch(dtype):
    """Two frames (case 3 and the same atoms displaced) through ``GraphedFrameBatch``: ``frames_plane_rows_kernel`` reads the
    entries its own binning launch wrote."""
    c = case("uniform1500")
    tolV, tolG = tols(dtype)
    rng = np.random.default_rng(406)
    pos2 = c.pos + np.array([1.3, -2.2, 0.7]) * H32 + rng.uniform(-0.1, 0.1, c.pos.shape)
    dist2, _ = O.pair_distances(pos2, c.cell, c.pairs, c.S)
    V2, cache2 = O.forward(O.PotentialSpec("coulomb", 1, c.sm, 1.0), "P3M", 5, c.h, c.q, c.cell, pos2, c.pairs, dist2, return_cache=True)
    gr2 = O.backward(cache2, c.q)
    gpos_d2, _ = O.pair_distances_backward(pos2, c.cell, c.pairs, c.S, gr2["dist"])
    refs = [(c.E, c.F), (float((V2 * c.q).sum()), -(gr2["positions"] + gpos_d2))]
    tq, tc, tp, ti, tS = c.tensors(dtype)
    frames = [(tq, tc, tp, ti, tS), (tq, tc, torch.tensor(pos2, device=DEV, dtype=dtype), ti, tS)]
    batch = tpa.GraphedFrameBatch(c.calc(dtype), frames)
    assert batch.ns == (32, 32, 32)
    E, F = batch()
    if PLANES:
        assert _lib.load().mipme_last_cosched_kernel().decode() == "frames_plane_rows_kernel"
    for k, (Eo, Fo) in enumerate(refs):
        eE, eF = abs(float(E[k]) - Eo) / abs(Eo), rell2(F[k].cpu(), Fo)
        print(f"frame {k} {dtype}: relE={eE:.2e} relF={eF:.2e}")
        assert eE < tolV and eF < tolG, (k, eE, eF)


@pytest.mark.parametrize("what", ["nan-charge", "nan-x", "inf-y", "nan-z"])
def test_nonfinite_input_gives_nan_planes(what):
    """fp32, case 3: a NaN charge makes the bound of the fixed-point scale NaN (the per-wavefront maxima of the binning pass), a
    position that is not finite gives weights that are not finite, which the binning pass now stores in the entry and the lane
    that unpacks them meets (``guard_item``): it poisons the inverse scale of its plane.  Either way NaN reaches the mesh, the x
    stage spreads it over every plane, and the guard of the k-space filter raises; the next clean call is clean."""
    c = case("uniform1500")
    calc = c.calc(torch.float32)
    tq, tc, tp, ti, tS = c.tensors(torch.float32, grad=True)  # (force sums wanted: the pair sum is co-scheduled with the spread)
    assert torch.isfinite(calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))).all()
    assert_plane_kernel(c, calc, torch.float32, len(c.pos))
    q, pos = c.q.copy(), c.pos.copy()
    if what == "nan-charge":
        q[733] = float("nan")
    else:
        pos[733, "xyz".index(what[-1])] = float(what[:3])
    t = lambda a: torch.tensor(a, device=DEV, dtype=torch.float32)  # noqa: E731
    tb = t(pos).requires_grad_(True)
    V = calc(t(q), tc, tb, ti, tpa.pair_distances(tb, ti, tc, tS))
    assert_plane_kernel(c, calc, torch.float32, len(c.pos))
    assert torch.isnan(V).all()
    calc.check_nan = True
    with pytest.raises(ValueError, match="NaNs detected in the k-space filter result"):
        calc(t(q), tc, tb, ti, tpa.pair_distances(tb, ti, tc, tS))
    calc.check_nan = False
    V = calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    assert rell2(V.detach().cpu(), c.V) < 2e-5
