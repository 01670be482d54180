"""Rounds of two atoms per lane group in the gather + energy + forces launch (``MIPME_GATHER_PAIRS``, docs/SWITCHES.md;
docs/KERNELS.md section 10). A lane group of ``gather_tail_kernel`` takes the atoms ``idx`` and ``idx + 64`` of its brick's sequence
(own slots, then the overflow candidates) in one round and issues both atoms' loads together.  What can go wrong is the round
logic: a second atom that does not exist (count <= 64, an odd number of passes), the step from the brick's own slots to the
overflow walk inside a round, a third pass (more than 128 atoms), a slot no pass wrote, the order of the fp64 cell sums, a
captured graph whose bricks change between one and two passes.

Shapes: a 16 A cube on a 32^3 mesh -- 64 bricks, the smallest mesh on the plane-spread route -- with 2 100 atoms, so that a brick
has 4 * 33 + 8 -> 144 slots of its own and can hold every count up to 129 without overflowing.  The atoms are PLACED: jittered
sites of a 6^3 sub-lattice of each brick, at least a quarter of a mesh spacing inside every brick face and 0.6 mesh spacings (0.3 A)
apart; the per-brick counts are recomputed in NumPy with the binning rule from the float32 positions and asserted before a case
touches the GPU.

Every test asserts through ``mipme_last_gather_pairs()`` which form RAN.  Tolerances: those of
tests/test_gpu_deferred_slots.py ``test_parity_with_the_oracle`` (potentials and energy / gradients 1e-11 / 1e-10 in fp64,
2e-5 / 2e-4 in fp32), the contract at those of ``test_contract_step_and_both_rider_kinds`` (1e-9 / 2e-4 of the largest component).

The field of an atom is not returned by any call of the package; the forces -- s q (c F_pair + field), with pair sums that are
bit-reproducible -- carry it, and the bit-for-bit test compares them, the potentials, the energy and dE/dq = 2 V."""
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
#: the library's default (docs/SWITCHES.md): with any of these switched the loop of one atom is what must have run
PAIRS = os.environ.get("MIPME_GATHER_PAIRS", "1") != "0" and os.environ.get("MIPME_SPARSE_FORCE", "0") == "0"
L_BOX = 16.0
N_MESH = 32
H = 2 * L_BOX / 30  # -> 32^3 mesh, 0.5 A between points
BRICK = 8
N_ATOMS = 2100
CUTOFF = 3.0
#: (scheme, order, dtype, paired): the benchmark's fp32 P3M-5, the ionic presets' fp64 at order 4, and an order that keeps the loop
SETUPS = {"p3m5-f32": ("P3M", 5, torch.float32, True), "p3m4-f64": ("P3M", 4, torch.float64, True),
          "pme6-f32": ("PME", 6, torch.float32, False)}
#: atoms in the target brick; "over": more than its slots hold by more than one pass of 64, so that the overflow walk has rounds
CASES = ["1", "63", "64", "65", "127", "128", "129", "over"]
TARGET, EMPTY = 21, (0, 7, 22, 42, 63)  # bricks (bx * 4 + by) * 4 + bz


def rell2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def tols(dtype):
    return (1e-11, 1e-10) if dtype == torch.float64 else (2e-5, 2e-4)


def gather_pairs():
    return _lib.load().mipme_last_gather_pairs()


def assert_form(paired):
    """The last gather launch took its atoms in rounds of two (or, paired = False, one by one)."""
    got = gather_pairs()
    assert got == int(paired and PAIRS), got


def bin_capacity(nb, n):
    """csrc/bricks_device.h ``bin_capacity``: slots of a brick."""
    mean = (n + nb - 1) // nb
    return max(8, min((4 * mean + 8 + 7) // 8 * 8, (n + 7) // 8 * 8))


def brick_counts(pos, order, dtype):
    """Atoms per brick by the binning pass's rule (``atom_mesh_coords``: the mesh point of an atom is the nearest one for an odd
    order and the one below for an even order, from the positions as the kernel reads them) and how close any atom comes to a brick face."""
    p = torch.tensor(pos, dtype=dtype).to(torch.float64).numpy()
    u = N_MESH * (p @ np.linalg.inv(L_BOX * np.eye(3)))
    m = (np.rint(u) if order % 2 else np.floor(u)).astype(np.int64) % N_MESH
    b = ((m[:, 0] // BRICK) * 4 + m[:, 1] // BRICK) * 4 + m[:, 2] // BRICK
    face = u + (0.5 if order % 2 else 0.0)  # faces at multiples of 8 in this coordinate
    d = np.abs(face - BRICK * np.rint(face / BRICK)).min()
    return np.bincount(b, minlength=64), float(d)


def place(counts, order, rng):
    """``counts[b]`` atoms in brick b on distinct jittered sites of its 6^3 sub-lattice (brick-local mesh coordinates 0.5 + 1.4 k
    +- 0.1: in [0.4, 7.6] of a brick 8 wide, 1.2 apart at the least)."""
    out = []
    for b, n in enumerate(counts):
        if n == 0:
            continue
        assert n <= 216
        sites = rng.permutation(216)[:n]
        k = np.stack([sites // 36, (sites // 6) % 6, sites % 6], 1)
        local = 0.5 + 1.4 * k + rng.uniform(-0.1, 0.1, k.shape)
        origin = BRICK * np.array([b // 16, (b // 4) % 4, b % 4]) - (0.5 if order % 2 else 0.0)
        out.append((origin + local) * (L_BOX / N_MESH))
    pos = np.concatenate(out) % L_BOX
    return pos[rng.permutation(len(pos))]


def intended_counts(case, rng):
    cap = bin_capacity(64, N_ATOMS)
    assert cap >= 129
    k = cap + 70 if case == "over" else int(case)
    counts = np.zeros(64, dtype=np.int64)
    counts[TARGET] = k
    fill = [b for b in range(64) if b != TARGET and b not in EMPTY]
    counts[fill] = rng.multinomial(N_ATOMS - k, np.full(len(fill), 1.0 / len(fill)))
    assert counts[fill].max() <= 64 < cap and counts.sum() == N_ATOMS
    return counts, cap


class Ref:
    """Oracle results of one system (tests/test_gpu_deferred_slots.py ``Ref``)."""

    def __init__(self, scheme, order, q, cell, pos, pairs, S, sm=1.0):
        self.q, self.cell, self.pos, self.pairs, self.S = q, cell, pos, pairs, S
        dist, _ = O.pair_distances(pos, cell, pairs, S)
        spec = O.PotentialSpec("coulomb", 1, sm, 1.0)
        self.V, self.cache = O.forward(spec, "P3M" if scheme == "P3M" else "Lagrange", order, H, q, cell, pos, pairs, dist,
                                       return_cache=True)
        gr = O.backward(self.cache, q)
        gpos_d, gcell_d = O.pair_distances_backward(pos, cell, pairs, S, gr["dist"])
        self.E = float((self.V * q).sum())
        self.F = -(gr["positions"] + gpos_d)
        self.dq = gr["charges"] + self.V
        self.dcell = gr["cell"] + gcell_d


@functools.lru_cache(maxsize=None)
def case_ref(case, setup):
    """Positions with the case's counts (asserted with the kernel's rule), neighbour list, oracle: once per (case, setup)."""
    scheme, order, dtype, _ = SETUPS[setup]
    rng = np.random.default_rng(7000 + 31 * CASES.index(case) + order)
    counts, cap = intended_counts(case, rng)
    pos = place(counts, order, rng)
    got, face = brick_counts(pos, order, dtype)
    assert np.array_equal(got, counts), (case, setup, got[TARGET], counts[TARGET])
    assert got[TARGET] == (cap + 70 if case == "over" else int(case)) and all(got[b] == 0 for b in EMPTY)
    assert face >= 0.25, face
    q = rng.normal(size=(N_ATOMS, 1))
    q -= q.mean()
    cell = L_BOX * np.eye(3)
    pairs, S, _ = tpa.neighbor_list(pos, cell, CUTOFF)
    return Ref(scheme, order, q, cell, pos, pairs, S)


def make_calc(setup):
    scheme, order, dtype, _ = SETUPS[setup]
    Calc = tpa.P3MCalculator if scheme == "P3M" else tpa.PMECalculator
    return Calc(tpa.CoulombPotential(smearing=1.0), mesh_spacing=H, interpolation_nodes=order).to(dtype)


def tensors(ref, dtype, grad=False):
    t = lambda a, g=False: torch.tensor(a, device=DEV, dtype=dtype, requires_grad=g)  # noqa: E731
    return t(ref.q), t(ref.cell, grad), t(ref.pos, grad), torch.tensor(ref.pairs, device=DEV), t(ref.S)


def check_eager(calc, ref, dtype, paired, what=""):
    tolV, tolG = tols(dtype)
    tq, tc, tp, ti, tS = tensors(ref, dtype, grad=True)
    V = calc(tq, tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
    assert_form(paired)
    E = tpa.weighted_sum(V, tq)
    E.backward()
    eV, eE, eF = rell2(V.detach().cpu(), ref.V), abs(float(E.detach()) - ref.E) / abs(ref.E), rell2(-tp.grad.cpu(), ref.F)
    print(f"eager {what} {dtype}: relV={eV:.2e} relE={eE:.2e} relF={eF:.2e}")
    assert eV < tolV and eE < tolV and eF < tolG, (eV, eE, eF)


def check_graphed(calc, ref, dtype, paired, what=""):
    tolV, tolG = tols(dtype)
    tq, tc, tp, ti, tS = tensors(ref, dtype)
    step = tpa.GraphedEnergyForces(calc, tq, tc, tp, ti, tS)
    E, F = step()
    assert_form(paired)
    eE, eF = abs(float(E) - ref.E) / abs(ref.E), rell2(F.cpu(), ref.F)
    print(f"graphed {what} {dtype}: relE={eE:.2e} relF={eF:.2e}")
    assert eE < tolV and eF < tolG, (eE, eF)
    return step


@pytest.mark.parametrize("setup", list(SETUPS))
@pytest.mark.parametrize("case", CASES)
def test_counts_at_the_round_edges(case, setup):
    """k = 1 .. 129 atoms in one brick, and a brick beyond its slots: potentials, energy and forces against the oracle, eagerly
    and from the replayed graph, in the form the instantiation is meant to run in."""
    _, _, dtype, paired = SETUPS[setup]
    ref = case_ref(case, setup)
    calc = make_calc(setup)
    check_eager(calc, ref, dtype, paired, f"{case} {setup}")
    check_graphed(calc, ref, dtype, paired, f"{case} {setup}")


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import torchpme_amd as tpa
from torchpme_amd import _lib
d = np.load(sys.argv[2])
names = sorted({k.split("/")[0] for k in d.files})
out = {}
for name in names:
    for tag, dtype, order in (("f32", torch.float32, 5), ("f64", torch.float64, 4)):
        g = lambda k: d[name + "/" + tag + "/" + k]
        t = lambda a: torch.tensor(a, device="cuda:0", dtype=dtype)
        calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=float(d[name + "/h"]), interpolation_nodes=order).to(dtype)
        ti, tS = torch.tensor(g("pairs"), device="cuda:0"), t(g("S"))
        # (with gradients to form, as in check_eager, the eager call's gather is the tail kernel too)
        tp, tc = t(g("pos")).requires_grad_(True), t(g("cell")).requires_grad_(True)
        V = calc(t(g("q")), tc, tp, ti, tpa.pair_distances(tp, ti, tc, tS))
        k = name + "_" + tag
        out["pairs_eager_" + k] = _lib.load().mipme_last_gather_pairs()
        V = V.detach()
        E, F, dq = tpa.GraphedEnergyForces(calc, t(g("q")), t(g("cell")), t(g("pos")), ti, tS, charge_gradient=True)()
        out["pairs_graph_" + k] = _lib.load().mipme_last_gather_pairs()
        out["fill_" + k] = _lib.load().mipme_last_slot_fill()
        out["V_" + k], out["E_" + k], out["F_" + k], out["dq_" + k] = V.cpu().numpy(), E.cpu().numpy(), F.cpu().numpy(), dq.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def run_children(tmp_path, cases, settings):
    """The cases' systems (fp32 P3M-5 and fp64 P3M-4) in one fresh process per environment of ``settings``, started together: the
    library reads its switches once per process."""
    data = {}
    for case in cases:
        data[case + "/h"] = H
        for tag, setup in (("f32", "p3m5-f32"), ("f64", "p3m4-f64")):
            ref = case_ref(case, setup)
            for k in ("q", "cell", "pos", "pairs", "S"):
                data[f"{case}/{tag}/{k}"] = getattr(ref, k)
    np.savez(tmp_path / "in.npz", **data)
    procs = {}
    for name, env in settings.items():
        out = tmp_path / f"out_{name}.npz"
        procs[name] = (subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(out)],
                                        env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out)
    res = {}
    for name, (p, out) in procs.items():
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
        res[name] = np.load(out)
    return res


def test_pairs_against_the_loop_bit_for_bit(tmp_path):
    """``MIPME_GATHER_PAIRS=1`` against ``=0`` with ``MIPME_PLANE_PARTS=1`` (the fp32 mesh is then bit-reproducible: the protocol
    of ``test_deferred_against_one_pass_bit_for_bit``): the two forms run one function per atom, so potentials, energy, forces
    and dE/dq are identical bit for bit in fp32; in fp64 the mesh sums depend on arrival order: 1e-12 relative, as there."""
    cases = ("65", "129", "over")
    res = run_children(tmp_path, cases, {"1": dict(MIPME_PLANE_PARTS="1", MIPME_GATHER_PAIRS="1"),
                                         "0": dict(MIPME_PLANE_PARTS="1", MIPME_GATHER_PAIRS="0")})
    for case in cases:
        for tag in ("f32", "f64"):
            k = f"{case}_{tag}"
            for how in ("eager", "graph"):
                assert res["1"][f"pairs_{how}_{k}"] == int(PAIRS) and res["0"][f"pairs_{how}_{k}"] == 0, (k, how)
        for name in ("V", "E", "F", "dq"):
            a, b = res["1"][f"{name}_{case}_f32"], res["0"][f"{name}_{case}_f32"]
            assert np.array_equal(a, b), (case, name, np.abs(a - b).max())
            assert relmax(res["1"][f"{name}_{case}_f64"], res["0"][f"{name}_{case}_f64"]) <= 1e-12, (case, name)
        assert rell2(res["1"][f"V_{case}_f64"], case_ref(case, "p3m4-f64").V) < 1e-11  # (and both are the oracle's)


def test_one_pass_slot_fill(tmp_path):
    """``MIPME_DEFER_SLOTS=0``: the binning pass fills the slots itself (asserted) and the paired gather reads them."""
    res = run_children(tmp_path, ("129",), {"d0": dict(MIPME_DEFER_SLOTS="0")})["d0"]
    for tag, setup in (("f32", "p3m5-f32"), ("f64", "p3m4-f64")):
        ref = case_ref("129", setup)
        tolV, tolG = tols(SETUPS[setup][2])
        k = f"129_{tag}"
        assert res["fill_" + k] == 0 and res["pairs_eager_" + k] == int(PAIRS) and res["pairs_graph_" + k] == int(PAIRS)
        errs = (rell2(res["V_" + k], ref.V), abs(float(res["E_" + k]) - ref.E) / abs(ref.E), rell2(res["F_" + k], ref.F),
                rell2(res["dq_" + k], ref.dq))
        print(f"one-pass fill {tag}: relV={errs[0]:.2e} relE={errs[1]:.2e} relF={errs[2]:.2e} rel_dq={errs[3]:.2e}")
        assert errs[0] < tolV and errs[1] < tolV and errs[2] < tolG and errs[3] < 10 * tolV, errs


@pytest.mark.parametrize("setup", ["p3m5-f32", "p3m4-f64"])
def test_replay_across_the_pass_boundary(setup):
    """One graph captured with 64 atoms in the target brick; then one atom of a neighbouring brick is moved into it and out again:
    64 -> 65 -> 64 between replays.  The second atom of a lane group appears and disappears without a new capture."""
    scheme, order, dtype, paired = SETUPS[setup]
    ref0 = case_ref("64", setup)
    tolV, tolG = tols(dtype)
    step = check_graphed(make_calc(setup), ref0, dtype, paired, "64")
    counts0, _ = brick_counts(ref0.pos, order, dtype)
    # the mover: an atom of the brick below the target along z (TARGET - 1), shifted up by one brick (its site in the target brick
    # may be taken: the sub-lattice sites are 0.7 A apart and the jitter 0.05 A, so the nearest atom is still >= 0.6 A away ...
    # unless it sits on the same site: pick a mover whose site is free)
    p = torch.tensor(ref0.pos, dtype=dtype).to(torch.float64).numpy()
    u = N_MESH * p / L_BOX
    m = (np.rint(u) if order % 2 else np.floor(u)).astype(np.int64) % N_MESH
    b = ((m[:, 0] // BRICK) * 4 + m[:, 1] // BRICK) * 4 + m[:, 2] // BRICK
    shift = np.array([0.0, 0.0, BRICK * L_BOX / N_MESH])
    inside = ref0.pos[b == TARGET]
    mover = next(i for i in np.nonzero(b == TARGET - 1)[0] if np.linalg.norm(inside - (ref0.pos[i] + shift), axis=1).min() > 0.5)
    pos1 = ref0.pos.copy()
    pos1[mover] += shift
    counts1, face = brick_counts(pos1, order, dtype)
    assert counts0[TARGET] == 64 and counts1[TARGET] == 65 and counts1[TARGET - 1] == counts0[TARGET - 1] - 1 and face >= 0.25
    ref1 = Ref(scheme, order, ref0.q, ref0.cell, pos1, ref0.pairs, ref0.S)
    for name, pos, ref in (("65", pos1, ref1), ("64", ref0.pos, ref0), ("65", pos1, ref1)):
        E, F = step(torch.tensor(pos, device=DEV, dtype=dtype))
        assert_form(paired)
        eE, eF = abs(float(E) - ref.E) / abs(ref.E), rell2(F.cpu(), ref.F)
        print(f"replay -> {name} {dtype}: relE={eE:.2e} relF={eF:.2e}")
        assert eE < tolV and eF < tolG, (name, eE, eF)


@pytest.mark.parametrize("setup", ["p3m5-f32", "p3m4-f64"])
@pytest.mark.parametrize("case", ["65", "129", "over"])
def test_contract_step(case, setup):
    """``GraphedEnergyForces(charge_gradient=True, cell_gradient=True)``: E, F, dE/dq (``grad_q``) and dE/dcell (the gather's
    ``rpart`` sums, accumulated atom A before atom B, round by round) against the oracle."""
    _, _, dtype, paired = SETUPS[setup]
    ref = case_ref(case, setup)
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    tq, tc, tp, ti, tS = tensors(ref, dtype)
    step = tpa.GraphedEnergyForces(make_calc(setup), tq, tc, tp, ti, tS, charge_gradient=True, cell_gradient=True)
    assert step._fused_contract
    for _ in range(2):
        E, F, dq, dc = step()
        assert_form(paired)
        errs = (abs(float(E) - ref.E) / abs(ref.E), relmax(F.cpu(), ref.F), relmax(dq.cpu(), ref.dq), relmax(dc.cpu(), ref.dcell))
        print(f"contract {case} {dtype}: relE={errs[0]:.2e} relF={errs[1]:.2e} rel_dq={errs[2]:.2e} rel_dcell={errs[3]:.2e}")
        assert max(errs) <= tol, errs
