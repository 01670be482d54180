"""The route decisions of the calculator's autograd node (``ops._mesh_route``, ``ops._backward_plan``) are pure functions of
facts: run them over the product of their boolean inputs on the CPU and hold every outcome against the rules that
``include/mipme.h`` and INTEGRATION.md section 3b state for the C-ABI -- what a launch needs, never a second copy of the
expressions.

The product of the forward's route leaves out combinations the callers cannot produce (a force buffer without a fused pair
plan, ...; see ``pair_facts``) and asks about the 4-byte entries as the forward does: without them first, with them only where
the route wants them.  The full product of the booleans (2 x 8 192 x ~150 calls, a few seconds) runs at the base of the
remaining inputs (one channel, 1/r with a smearing -- a mesh calculator always has one --, 343 atoms, table shift codes, rows of
a pair list) and again with each of those changed alone (two channels, 1/r^6, 1/r^4, no atoms, 3 x int8 shifts, rows of a
NeighborStream, no smearing); every one of these passes also says which outcomes it must have met and which it must never
meet, so that no rule holds for want of a case.  The product of the integers (Cn x p_eff x N, with every shift format and
with and without a smearing) runs over every 101st combination of the booleans -- an odd stride, under which each of them
takes both values.  Direct cases show each of the four inputs switching its output off in an otherwise tail-capable call."""

import itertools

import pytest

from torchpme_amd import ops

B = (False, True)
#: (Cn, p_eff, N, shift_fmt, fmt_flags, smeared): the base, then one changed at a time; with each, outcomes that the full
#: product must meet at least once and outcomes it must never meet
BASE = (1, 1, 343, 1, 0, True)
FULL = {
    "base": (BASE, ("field", "records_out", "cosched", "ent32", "tail_ok", "tail_q", "tail_cell", "slab_in_tail",
                    "pair_partials", "rho_keep", "rho_hat", "keep_rho_mesh"), ("cell_partials",)),
    "two_channels": ((2, 1, 343, 1, 0, True), ("cell_partials", "keep_rho_mesh", "rho_hat"),
                     ("field", "records_out", "cosched", "want_ent32", "tail_ok", "rho_keep", "slab_in_tail")),
    "r6": ((1, 6, 343, 1, 0, True), ("cosched", "ent32", "tail_ok", "tail_q", "tail_cell", "field"), ("slab_in_tail",)),
    "r4": ((1, 4, 343, 1, 0, True), ("cosched", "field", "records_out"), ("want_ent32", "ent32", "tail_ok", "slab_in_tail")),
    "no_atoms": ((1, 1, 0, 1, 0, True), ("records_out", "field"), ("cosched", "want_ent32", "tail_ok")),
    "int8_shifts": ((1, 1, 343, 0, 0, True), ("records_out", "field", "pair_partials"), ("cosched", "want_ent32", "tail_ok")),
    "stream_rows": ((1, 1, 343, 0x101, 0x100, True), ("cosched", "ent32", "tail_ok", "tail_q", "tail_cell"), ()),
    "no_smearing": ((1, 1, 343, 1, 0, False), ("cosched", "field", "records_out"), ("want_ent32", "ent32", "tail_cell")),
}
PAIR_NAMES = ("fused", "force", "same_positions", "src_cell", "write_dist", "masked", "want_src_cell", "lazy")
OTHER_NAMES = ("coschedule", "tail_fusion", "xfused", "request_q", "request_cell", "want_q", "want_cell", "want_pos",
               "want_dist", "no_exclusion", "full_list", "slab", "bins")


def pair_facts(energy_fast_path):
    """What the pair plan can hand to the route: without the fused kernel none of its buffers; speculative force sums only
    with the energy fast path; stored distances only without a mask; a gradient for the distances' cell only if there is one."""
    for fused, force, same, src_cell, write_dist, masked, want_src_cell, lazy in itertools.product(B, repeat=8):
        if not fused and (force or same or src_cell or write_dist or want_src_cell):
            continue
        if (force and not energy_fast_path) or (write_dist and masked) or (want_src_cell and not src_cell):
            continue
        yield fused, force, same, src_cell, write_dist, masked, want_src_cell, lazy


def check_route(f, r):
    if r.tail_q or r.tail_cell:
        assert r.tail_ok
    if r.tail_ok:
        assert r.cosched and r.field and f["force"] and not r.rho_hat and f["p_eff"] in (1, 6) and f["no_exclusion"]
        assert not f["want_dist"]
    if r.tail_cell:
        assert r.ent32 and not f["write_dist"] and f["src_cell"]
    if r.ent32:
        assert r.want_ent32 and f["has_ent32"]
        assert r.cosched and f["force"] and f["p_eff"] in (1, 6) and f["smeared"] and f["no_exclusion"]
    if r.cosched:
        assert r.records_out and not f["masked"] and (f["shift_fmt"] & 0xFF) == 1 and f["N"] > 0
    if r.records_out:
        assert f["fused"] and f["bins"] and f["Cn"] == 1 and f["same_positions"]
    assert r.slab_in_tail == (f["slab"] and r.tail_ok)
    if f["slab"] and not r.tail_ok:
        assert not r.field
    if r.pair_partials:
        assert not r.cosched and not r.tail_cell
    if r.rho_keep:
        assert f["want_cell"] and f["Cn"] == 1 and not r.rho_hat
    if r.cell_partials:
        assert f["Cn"] > 1 and not r.tail_cell
    assert r.keep_rho_mesh == ((r.cell_partials or r.tail_cell) and not r.rho_keep and not r.rho_hat)
    # what a wanted gradient needs from the tail, if there is one: dE/dq only of a symmetric form
    if r.tail_q:
        assert r.symmetric
    if r.tail_ok and f["want_q"]:
        assert r.tail_q
    if r.tail_ok and (f["want_cell"] or f["want_src_cell"]):
        assert r.tail_cell


def run_product(energy_fast_path, ints, others, seen=None):
    Cn, p_eff, N, shift_fmt, fmt_flags, smeared = ints
    pairs = list(pair_facts(energy_fast_path))
    n = 0
    seen = set() if seen is None else seen
    for other in others:
        f = dict(zip(OTHER_NAMES, other), energy_fast_path=energy_fast_path, Cn=Cn, p_eff=p_eff, N=N, fmt_flags=fmt_flags,
                 smeared=smeared)
        for pair in pairs:
            f.update(zip(PAIR_NAMES, pair))
            f["shift_fmt"] = shift_fmt if f["fused"] else 0
            f["has_ent32"] = False
            r = ops._mesh_route(**f)
            check_route(f, r)
            seen.update(k for k, v in zip(r._fields, r) if v)
            if r.want_ent32:
                f["has_ent32"] = True
                r = ops._mesh_route(**f)
                check_route(f, r)
                seen.update(k for k, v in zip(r._fields, r) if v)
            n += 1
    return n


@pytest.mark.parametrize("name", list(FULL))
def test_mesh_route_over_the_product_of_its_booleans(name):
    ints, met, never_met = FULL[name]
    seen = set()
    for energy_fast_path in B:
        n = run_product(energy_fast_path, ints, itertools.product(B, repeat=len(OTHER_NAMES)), seen)
        assert n == 2 ** len(OTHER_NAMES) * len(list(pair_facts(energy_fast_path)))
    assert set(met) <= seen, sorted(set(met) - seen)
    assert not (set(never_met) & seen), sorted(set(never_met) & seen)


@pytest.mark.parametrize("Cn,p_eff,N", list(itertools.product((1, 2), (1, 6, 4), (0, 343))))
def test_mesh_route_over_the_product_of_its_integers(Cn, p_eff, N):
    formats = ((1, 0), (0, 0), (0x101, 0x100))
    for k, ((shift_fmt, fmt_flags), smeared, energy_fast_path) in enumerate(itertools.product(formats, B, B)):
        others = itertools.islice(itertools.product(B, repeat=len(OTHER_NAMES)), k, None, 101)
        assert run_product(energy_fast_path, (Cn, p_eff, N, shift_fmt, fmt_flags, smeared), others) > 0


def test_with_every_route_flag_off_nothing_speculative_is_requested():
    for other in itertools.product(B, repeat=len(OTHER_NAMES) - 3):
        f = dict(zip(OTHER_NAMES[3:], other), energy_fast_path=False, coschedule=False, tail_fusion=False, xfused=False,
                 Cn=1, p_eff=1, N=343, fmt_flags=0, smeared=True)
        for pair in pair_facts(False):
            f.update(zip(PAIR_NAMES, pair))
            f["shift_fmt"] = 1 if f["fused"] else 0
            for has_ent32 in B:
                r = ops._mesh_route(has_ent32=has_ent32, **f)
                assert not (r.field or r.cosched or r.want_ent32 or r.ent32 or r.tail_ok or r.tail_q or r.tail_cell
                            or r.slab_in_tail or r.pair_partials)


def base_facts(**changes):
    """The eager energy step of tests/test_gpu_contract.py: P3M, 1/r, fp32, half list, deferred distances, ``weighted_sum``."""
    f = dict(energy_fast_path=True, coschedule=True, tail_fusion=True, xfused=True, request_q=False, request_cell=False,
             want_q=False, want_cell=False, want_pos=True, want_dist=False, want_src_cell=False, Cn=1, N=343, p_eff=1,
             smeared=True, no_exclusion=True, full_list=False, lazy=False, slab=False, masked=False, fused=True, force=True,
             shift_fmt=1, fmt_flags=0, bins=True, same_positions=True, src_cell=True, write_dist=False, has_ent32=True)
    f.update(changes)
    return f


def test_named_case_tail_of_the_deferred_contract():
    """tests/test_gpu_contract.py::test_tail_is_used_for_the_deferred_contract: charges, cell and positions as leaves."""
    r = ops._mesh_route(**base_facts(want_q=True, want_cell=True, want_src_cell=True))
    assert r.tail_ok and r.tail_q and r.tail_cell and r.cosched and r.ent32 and not r.pair_partials and not r.slab_in_tail


def test_named_case_slab_without_tail_fusion():
    """tests/test_gpu_slab_step.py::test_graphed_step, the eager comparison with ``ops.TAIL_FUSION = False``."""
    r = ops._mesh_route(**base_facts(want_q=True, want_cell=True, want_src_cell=True, slab=True, tail_fusion=False))
    assert not r.tail_ok and not r.slab_in_tail and not r.field and not r.tail_q and not r.tail_cell


def test_named_case_slab_in_the_tail():
    """tests/test_gpu_slab_step.py::test_eager_call_keeps_the_gather_tail."""
    r = ops._mesh_route(**base_facts(want_q=True, want_cell=True, want_src_cell=True, slab=True))
    assert r.tail_ok and r.tail_q and r.tail_cell and r.slab_in_tail and r.field


CONTRACT = dict(want_q=True, want_cell=True, want_src_cell=True)  # the tail with everything it can carry


FORCES = {}  # positions only: the tail with energy and forces
#: (wanted gradients, the one input changed, outputs that go off, outputs that stay -- or come -- on).  With the whole contract
#: wanted, losing the tail's cell gradient sends the pair part's cell sums to the generic pair body: no co-scheduled launch.
SWITCHES = [
    (FORCES, dict(p_eff=4), ("want_ent32", "ent32", "tail_ok"), ("cosched", "records_out", "field")),
    (FORCES, dict(smeared=False), ("want_ent32", "ent32"), ("cosched", "tail_ok", "field")),
    (FORCES, dict(no_exclusion=False), ("want_ent32", "ent32", "tail_ok"), ("cosched", "field")),
    (FORCES, dict(has_ent32=False), ("ent32",), ("want_ent32", "cosched", "tail_ok")),
    (FORCES, dict(shift_fmt=0), ("cosched", "want_ent32", "ent32", "tail_ok"), ("records_out", "field")),
    (FORCES, dict(Cn=2), ("records_out", "cosched", "want_ent32", "field", "tail_ok"), ()),
    (FORCES, dict(N=0), ("cosched", "want_ent32", "tail_ok"), ("records_out", "field")),
    (FORCES, dict(masked=True), ("cosched", "want_ent32", "tail_ok"), ("records_out", "field")),
    (CONTRACT, dict(p_eff=4), ("want_ent32", "ent32", "tail_ok", "tail_q", "tail_cell", "cosched"),
     ("records_out", "field", "pair_partials", "rho_keep")),
    (CONTRACT, dict(smeared=False), ("want_ent32", "ent32", "tail_ok", "tail_q", "tail_cell", "cosched"),
     ("records_out", "field", "pair_partials")),
    (CONTRACT, dict(has_ent32=False), ("ent32", "tail_ok", "tail_q", "tail_cell", "cosched"), ("want_ent32", "pair_partials")),
    (CONTRACT, dict(shift_fmt=0), ("cosched", "want_ent32", "ent32", "tail_ok"), ("records_out", "field", "pair_partials")),
    (CONTRACT, dict(Cn=2), ("records_out", "cosched", "want_ent32", "field", "tail_ok", "rho_keep"),
     ("cell_partials", "pair_partials", "keep_rho_mesh")),
    (CONTRACT, dict(write_dist=True), ("tail_cell", "tail_ok", "cosched"), ("want_ent32", "pair_partials")),
]


@pytest.mark.parametrize("wants,change,off,still_on", SWITCHES)
def test_one_input_switches_its_outputs_off_in_a_tail_capable_call(wants, change, off, still_on):
    r = ops._mesh_route(**base_facts(**wants))
    assert r.records_out and r.cosched and r.want_ent32 and r.ent32 and r.tail_ok and r.field and not r.pair_partials
    if wants:
        assert r.tail_q and r.tail_cell and r.rho_keep and not r.cell_partials
    r = ops._mesh_route(**base_facts(**wants, **change))
    for name in off:
        assert not getattr(r, name), (change, name)
    for name in still_on:
        assert getattr(r, name), (change, name)


PLAN_NAMES = ("has_geom", "scaled", "energy", "need_q", "need_cell", "need_pos", "need_dist", "need_src_pos", "need_src_cell",
              "full_list", "has_rho_hat", "has_field", "rho_kept", "xfused", "has_topo", "has_fused", "has_force",
              "has_partials", "has_tab", "same_positions", "lazy")


def plan_facts():
    """Left out: the mesh's leftovers without a mesh, the fused plan's without one (and the gradients only it can ask for), a
    table next to the fused kernel or without rows, the mesh's energy mode without a scaled upstream gradient."""
    for v in itertools.product(B, repeat=len(PLAN_NAMES)):
        f = dict(zip(PLAN_NAMES, v))
        if not f["has_geom"] and (f["has_rho_hat"] or f["has_field"] or f["rho_kept"] or f["xfused"]):
            continue
        if not f["has_fused"] and (f["has_force"] or f["has_partials"] or f["need_src_pos"] or f["need_src_cell"] or f["lazy"]
                                   or f["same_positions"]):
            continue
        if (f["has_partials"] and not f["has_force"]) or (f["has_tab"] and (f["has_fused"] or not f["has_topo"])):
            continue
        if (f["energy"] and not f["scaled"]) or (f["has_fused"] and not f["has_topo"]) or (f["rho_kept"] and not f["has_rho_hat"]):
            continue
        yield f


@pytest.mark.parametrize("Cn", [1, 2])
def test_backward_plan_over_the_product_of_its_inputs(Cn):
    for f in plan_facts():
        p = ops._backward_plan(Cn=Cn, **f)
        mesh_wanted = f["has_geom"] and (f["need_q"] or f["need_cell"] or f["need_pos"])
        assert p.do_kspace == mesh_wanted
        if p.mesh is not None:
            assert mesh_wanted and (p.mesh == "energy") == f["energy"]
        if mesh_wanted and not f["energy"]:
            assert p.mesh == "general"
        # mipme_kspace_backward: grad_scale mode reads the forward's meshes; mesh_field only replaces the gradient gather
        if p.from_field:
            assert f["energy"] and f["has_field"] and not p.kb_pos and not p.kb_q
        if p.kb_pos or p.kb_q:
            assert p.mesh == "energy"
        # G_deriv: the kept rfftn(rho) of ONE channel inside the fused convolution; psi_hat otherwise, and for the 3-D plans
        if p.fused_cell:
            assert p.mesh == "general" and f["need_cell"] and f["rho_kept"] and f["xfused"] and Cn == 1 and not p.psi_hat
        if p.mesh == "general" and (not f["xfused"] or (f["need_cell"] and not p.fused_cell)):
            assert p.psi_hat
        if p.r2c:
            assert f["need_cell"] and not f["has_rho_hat"] and not f["energy"] and p.mesh == "general"
        if p.mesh == "general" and f["need_cell"]:
            assert f["has_rho_hat"] or p.r2c
        # dL/dq: gE V only for the symmetric form in energy mode; else exactly one pair kernel adds to what the mesh left
        assert p.energy_q == (p.pair_q == "energy")
        if p.energy_q:
            assert f["need_q"] and f["energy"] and not f["full_list"] and not p.kb_q and not p.zero_q and not p.atomic_q
        if f["need_q"]:
            assert (p.pair_q is not None) != p.atomic_q
            if not p.energy_q:
                assert (p.mesh is not None) != p.zero_q
                if p.mesh == "energy":
                    assert p.kb_q
        else:
            assert p.pair_q is None and not p.atomic_q and not p.zero_q and not p.kb_q
        if p.atomic_q:
            assert not f["has_topo"]
        if p.pair_q == "tabulated":
            assert f["has_tab"]
        if p.pair_q == "fused":
            assert f["has_fused"]
        assert p.pair_stream == (f["need_dist"] or p.atomic_q)
        # positions / cell of the pair part: finalize from the forward's sums, or the general adjoint -- one of them, if wanted
        sr_wanted = f["need_src_pos"] or f["need_src_cell"]
        assert (p.sr_done or p.sr_adjoint) == sr_wanted and not (p.sr_done and p.sr_adjoint)
        if p.sr_done:
            assert f["scaled"] and f["has_force"] and (f["has_partials"] or not f["need_src_cell"])
        if p.mesh_done:
            assert f["need_pos"] and f["has_field"] and f["energy"] and p.field_left
        if f["need_pos"] and f["has_geom"]:  # (somebody forms the mesh part's position gradient)
            assert p.mesh_done or (p.mesh is not None and (p.kb_pos or p.mesh == "general"))
        if p.one_finalize:
            assert p.sr_done and p.mesh_done and f["same_positions"] and f["need_src_pos"] and not f["lazy"]
