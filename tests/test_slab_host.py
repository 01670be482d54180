"""CPU tests (no GPU) of the slab term of the gather tail: the appended ``slab`` field of the two argument structs
(``include/mipme.h`` against the ctypes mirrors, old callers, the refusals that come before any device work), the argument
checks of ``GraphedEnergyForces(slab_correction=True)`` and the host-side cache of the slab axis."""

import ctypes as C
import itertools
import os
import re

import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"mipme_kspace_forward_args_t": _lib.KspaceForwardArgs, "mipme_md_args_t": _lib.MdArgs}
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64}


def _header_fields(name):
    """[(C type, field name)] of ``typedef struct ... { ... } name;`` in include/mipme.h, in order."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mipme.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*" + name + r"\s*;", hdr, flags=re.S).group(1)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        first, *more = decl.split(",")
        ctype, field = re.match(r"(.*?)(\w+)$", first.strip(), flags=re.S).groups()
        ctype = " ".join(ctype.split())
        out.append((ctype, field))
        out += [(ctype, m.strip()) for m in more]
    return out


@pytest.mark.parametrize("cname", sorted(ARGS))
def test_argument_struct_mirrors_the_header_field_by_field(cname):
    fields, mirror = _header_fields(cname), ARGS[cname]._fields_
    assert [f for _, f in fields] == [n for n, _ in mirror]
    for (ctype, field), (_, mtype) in zip(fields, mirror):
        if "*" in ctype:  # every pointer is 8 bytes, whatever it points to
            assert C.sizeof(mtype) == C.sizeof(C.c_void_p), field
        else:
            assert mtype is CTYPE[ctype], (field, ctype)
    # the appended fields come last, behind everything an older caller knows, and zero means off
    assert [n for n, _ in mirror[-2:]] == ["slab", "_pad_slab"]
    cls = ARGS[cname]
    assert cls.slab.offset == cls.energy_log_capacity.offset + 8 and C.sizeof(cls) == cls.slab.offset + 8
    assert cls().slab == 0


def _mesh(channels=1):
    md = _lib.MeshDesc(scheme=_lib.P3M, order=5, nx=32, ny=32, nz=64, n_channels=channels, volume=20.0 * 22.0 * 36.0)
    for d, length in enumerate((20.0, 22.0, 36.0)):
        md.cell[4 * d], md.inv_cell[4 * d] = length, 1.0 / length
    return md


def _pot(exponent=1):
    kind = _lib.COULOMB if exponent == 1 else _lib.INVERSE_POWER_LAW
    return _lib.PotentialDesc(kind=kind, exponent=exponent, smearing=1.2, prefactor=1.0, exclusion_radius=-1, exclusion_degree=1)


def test_slab_refusals_and_old_callers_of_kspace_forward():
    """The refusals of ``slab`` come before the library looks at the plan, so they are reached without a device; a struct
    with the size of a caller compiled before the field existed is read as ``slab = 0`` and gets past them."""
    lib = _lib.load()
    one = (C.c_double * 4)()
    out = C.addressof(one)

    def call(md, pot, size=None, **kw):
        a = _lib.KspaceForwardArgs(mesh=C.pointer(md), pot=C.pointer(pot), dtype=_lib.F64, **kw)
        if size is not None:
            a.size = size
        rc = lib.mipme_kspace_forward(C.byref(a))
        return rc, lib.mipme_last_error()

    tail = dict(out_energy=out, out_grad_positions=out)
    rc, msg = call(_mesh(), _pot(), slab=4, **tail)
    assert rc == -1 and b"slab must be 0 (off) or the non-periodic axis + 1" in msg
    rc, msg = call(_mesh(2), _pot(), slab=1, **tail)
    assert rc == -1 and b"the slab term of the gather tail serves one channel" in msg
    rc, msg = call(_mesh(), _pot(), slab=3)
    assert rc == -1 and b"slab rides on the gather tail" in msg
    rc, msg = call(_mesh(), _pot(6), slab=3, **tail)
    assert rc == -1 and b"the slab term exists for 1/r only" in msg
    # accepted as far as the arguments alone decide: the next check wants the plan
    rc, msg = call(_mesh(), _pot(), slab=3, **tail)
    assert rc == -1 and b"FFT plan is NULL" in msg
    # an old caller: the same bytes, but `size` ends before the field -- the two-channel refusal above is not reached
    old = _lib.KspaceForwardArgs.slab.offset
    rc, msg = call(_mesh(2), _pot(), size=old, slab=1, **tail)
    assert rc == -1 and b"FFT plan is NULL" in msg


def test_md_args_old_size_is_accepted():
    lib = _lib.load()
    md, pot = _mesh(), _pot()
    for size in (None, _lib.MdArgs.slab.offset):
        a = _lib.MdArgs(mesh=C.pointer(md), pot=C.pointer(pot), dtype=_lib.F64, n_atoms=0)
        if size is not None:
            a.size = size
        # (no atoms: refused by the range check of the live-bin kernels, which comes after the struct has been read)
        assert lib.mipme_md_step(C.byref(a)) == -1
        assert b"outside the live-bin kernels' range" in lib.mipme_last_error()


def _inputs(n=4):
    return (torch.ones(n, 1, dtype=torch.float64), 10.0 * torch.eye(3, dtype=torch.float64),
            torch.zeros(n, 3, dtype=torch.float64))


def test_graphed_slab_argument_checks():
    q, cell, pos = _inputs()
    coulomb = tpa.P3MCalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=1.0)
    for periodic in ((True, True, True), (True, False, False), (False, False, False)):
        with pytest.raises(ValueError, match="exactly two periodic axes"):
            tpa.GraphedEnergyForces(coulomb, q, cell, pos, neighbors=5.0, periodic=periodic, slab_correction=True)
    r6 = tpa.P3MCalculator(tpa.InversePowerLawPotential(exponent=6, smearing=1.0), mesh_spacing=1.0)
    with pytest.raises(ValueError, match="exists for 1/r only"):
        tpa.GraphedEnergyForces(r6, q, cell, pos, neighbors=5.0, periodic=(True, True, False), slab_correction=True)
    direct = tpa.Calculator(tpa.CoulombPotential(smearing=None))
    with pytest.raises(ValueError, match="needs a smearing"):
        tpa.GraphedEnergyForces(direct, q, cell, pos, neighbors=5.0, periodic=(True, True, False), slab_correction=True)


def test_slab_axis_cache_follows_the_tensor(monkeypatch):
    for flags in itertools.product((False, True), repeat=3):
        t = torch.tensor(flags)
        want = ops._slab_axis(list(flags))
        assert ops.slab_axis_of(t) == want
        assert ops.slab_axis_of(t) == want  # (from the cache)
        assert ops._SLAB_AXES[id(t)][1] == t._version
    assert ops.slab_axis_of(None) is None
    t = torch.tensor([True, True, False])
    assert ops.slab_axis_of(t) == 2
    t[2], t[0] = True, False  # in place: the version moves and the cache looks again
    assert ops.slab_axis_of(t) == 0
    t[1] = False
    assert ops.slab_axis_of(t) is None
    # a repeated call copies nothing: the cached entry answers even when the values cannot be read
    t = torch.tensor([True, False, True])
    assert ops.slab_axis_of(t) == 1
    def no_copy(_flags):
        raise AssertionError("the flags of an unchanged tensor were copied to the host again")

    monkeypatch.setattr(ops, "_slab_axis", no_copy)
    assert ops.slab_axis_of(t) == 1
