"""CPU tests (no GPU) of the multi-channel Ewald step and batch: the C-ABI mirrors of ``mipme_ewald_channels_step_args_t`` and
``mipme_ewald_channels_batch_args_t``, the exported symbols, how the scratch and the frame table grow with the channels, the
refusals of the entry points (host pointers: they must return before any launch), the refusals of ``GraphedEwaldStep`` and
``GraphedEwaldBatch`` with ``n_channels``, and that without the keyword -- or with ``n_channels=1`` -- the refusals are the
single-channel sentences, word for word."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib
from torchpme_amd import graphed as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
FRAME_BYTES, BLOCK_BYTES = 152, 8  # include/mipme.h: per frame, per workgroup
STEP_SYMBOLS = ("mipme_ewald_channels_step", "mipme_ewald_channels_step_work")
BATCH_SYMBOLS = ("mipme_ewald_channels_batch", "mipme_ewald_channels_batch_work", "mipme_ewald_channels_batch_table_bytes",
                 "mipme_ewald_channels_batch_table_build")


def _header():
    return open(os.path.join(ROOT, "include", "mipme.h")).read()


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, mirror, single, size", [
    ("mipme_ewald_channels_step_args", "EwaldChannelsStepArgs", "EwaldStepArgs", 232),
    ("mipme_ewald_channels_batch_args", "EwaldChannelsBatchArgs", "EwaldBatchArgs", 240),
])
def test_structs_mirror_the_header_field_by_field(name, mirror, single, size):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + r"_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    parsed = [re.search(r"(\w+)(?:\[(\d+)\])?$", d) for d in decls]
    names = [m.group(1) for m in parsed]
    cls = getattr(_lib, mirror)
    assert names == [n for n, _ in cls._fields_]
    assert names[:2] == ["size", "version"]
    # the fields of the single-channel struct plus n_channels, which takes the place of its padding word
    assert [n for n in names if n != "n_channels"] == [n for n, _ in getattr(_lib, single)._fields_ if n != "_pad"]
    offset = 0
    for d, m in zip(decls, parsed):
        field = m.group(1)
        width = (4 if re.match(r"(u?int32_t)\b", d) else 8) * int(m.group(2) or 1)
        assert getattr(cls, field).offset == offset, field
        assert getattr(cls, field).size == width, field
        offset += width
    assert C.sizeof(cls) == offset == size == C.sizeof(getattr(_lib, single))
    a = cls(n_channels=3)
    assert a.size == size and a.version == 1 and a.n_channels == 3
    with pytest.raises(TypeError, match="unknown field"):
        cls(no_such_field=1)


def test_versions_and_limits_of_the_header():
    hdr = _header()
    assert int(re.search(r"#define MIPME_EWALD_CHANNELS_STEP_VERSION (\d+)", hdr).group(1)) == _lib.EWALD_CHANNELS_STEP_VERSION == 1
    assert int(re.search(r"#define MIPME_EWALD_CHANNELS_BATCH_VERSION (\d+)", hdr).group(1)) == _lib.EWALD_CHANNELS_BATCH_VERSION == 1
    assert int(re.search(r"#define MIPME_EWALD_MAX_CHANNELS (\d+)", hdr).group(1)) == _lib.EWALD_MAX_CHANNELS == G.MAX_EWALD_CHANNELS == 8
    # the single-channel structs and their versions stay
    assert int(re.search(r"#define MIPME_EWALD_STEP_VERSION (\d+)", hdr).group(1)) == _lib.EWALD_STEP_VERSION == 1
    assert int(re.search(r"#define MIPME_EWALD_BATCH_VERSION (\d+)", hdr).group(1)) == _lib.EWALD_BATCH_VERSION == 1


def test_symbols_are_declared_and_exported_and_the_version_stays():
    hdr = _header()
    lib = _lib.load()
    for name in STEP_SYMBOLS + BATCH_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("mipme_ewald_step", "mipme_ewald_step_work", "mipme_ewald_batch", "mipme_ewald_batch_work",
                 "mipme_ewald_batch_table_bytes", "mipme_ewald_batch_table_build"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.mipme_version() == int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
def _slices(n, k):
    return 0 if k == 0 else max(1, min(-(-2048 // n), max(1, k // 256), 65535))


def _work_formula(n, k, c, cell):
    """include/mipme.h: geometry 16, C partials per 256 atoms, energy partials per 16 atoms, with the cell gradient 9 per row
    block and 10 per k block, C + 3 row results per atom and C + 3 slice partials per (slice, atom)."""
    rows = -(-n // 16)
    return 16 + c * -(-n // 256) + rows + (9 * rows + 10 * -(-k // 8) if cell else 0) + (c + 3) * n * (1 + _slices(n, k))


def test_step_work_size_grows_as_the_channels_say():
    lib = _lib.load()
    work = lib.mipme_ewald_channels_step_work
    assert work.restype is C.c_int64
    for n, k, c, cell in ((0, 10, 2, 0), (-1, 10, 2, 0), ((1 << 22) + 1, 10, 2, 0), (16, -1, 2, 0), (16, -1, 2, 1),
                          (16, 10, 1, 0), (16, 10, 0, 1), (16, 10, 9, 0), (16, 10, -2, 1)):
        assert work(n, k, c, cell) == 0, (n, k, c, cell)
    for n, k in ((1, 0), (16, 0), (300, 4096), (24, 250), (4096, 16384), (8, 32000)):
        for cell in (0, 1):
            sizes = [int(work(n, k, c, cell)) for c in range(2, 9)]
            assert sizes == [_work_formula(n, k, c, cell) for c in range(2, 9)], (n, k, cell)
            # one more channel: one partial per atom block, one result per atom and per (slice, atom)
            step = -(-n // 256) + n * (1 + _slices(n, k))
            assert all(b - a == step for a, b in zip(sizes, sizes[1:]))
            # one channel in this layout would be the single-channel step's area
            assert sizes[0] - step == int(lib.mipme_ewald_step_work(n, k, cell))


def _ptrs(n_atoms, n_k):
    return (np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int64), np.concatenate([[0], np.cumsum(n_k)]).astype(np.int64))


def test_batch_sizes_grow_as_the_channels_say():
    lib = _lib.load()
    wf, tf = lib.mipme_ewald_channels_batch_work, lib.mipme_ewald_channels_batch_table_bytes
    assert wf.restype is C.c_int64 and tf.restype is C.c_int64
    n_atoms, n_k = [1, 2, 17, 24, 300], [0, 9, 107, 251, 2047]
    ap, kp = _ptrs(n_atoms, n_k)
    F = len(n_atoms)
    for c in (1, 0, 9, -1):
        assert wf(F, ap.ctypes.data, kp.ctypes.data, c, 1) == 0 and tf(F, ap.ctypes.data, kp.ctypes.data, c, 1) == 0
    one = np.zeros(2, dtype=np.int64)
    for n_frames, a, k in ((0, ap, kp), ((1 << 20) + 1, ap, kp), (1, one, kp), (1, None, kp), (1, ap, None)):
        a_, k_ = (None if x is None else x.ctypes.data for x in (a, k))
        assert wf(n_frames, a_, k_, 3, 0) == 0 and tf(n_frames, a_, k_, 3, 0) == 0
    for cell in (0, 1):
        single_table = int(lib.mipme_ewald_batch_table_bytes(F, ap.ctypes.data, kp.ctypes.data, cell))
        for c in range(2, 9):
            assert int(wf(F, ap.ctypes.data, kp.ctypes.data, c, cell)) == sum(
                int(lib.mipme_ewald_channels_step_work(n, k, c, cell)) for n, k in zip(n_atoms, n_k))
            # the table: the same workgroups as the single-channel batch, whatever C
            assert int(tf(F, ap.ctypes.data, kp.ctypes.data, c, cell)) == single_table
    blocks = sum(max(1, -(-k // 256)) + -(-n // 256) + -(-k // 8) + n * _slices(n, k) + -(-n // 16) for n, k in zip(n_atoms, n_k))
    assert single_table == FRAME_BYTES * F + BLOCK_BYTES * blocks


def test_table_build_places_the_work_areas_of_the_channels():
    """The frame record of the table: the work areas one behind the other, each with C partials per atom block and C + 3 results
    per atom; a frame's slices begin at the same atoms and k-vectors whatever C."""
    lib = _lib.load()
    n_atoms, n_k = [17, 300, 1], [107, 2047, 0]
    ap, kp = _ptrs(n_atoms, n_k)
    ep = np.array([0, 65, 7000, 7001], dtype=np.int64)
    ns = np.array([[4, 9, 6], [16, 16, 16], [1, 1, 1]], dtype=np.int32)
    F, c, cell = 3, 5, 1
    n_bytes = int(lib.mipme_ewald_channels_batch_table_bytes(F, ap.ctypes.data, kp.ctypes.data, c, cell))
    host = np.zeros(n_bytes, dtype=np.uint8)
    build = lib.mipme_ewald_channels_batch_table_build
    assert build(F, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, ns.ctypes.data, c, cell, host.ctypes.data, n_bytes) == 0
    rec = host[:FRAME_BYTES * F].view(np.int64).reshape(F, FRAME_BYTES // 8)
    # int64 fields: atom0, n_atoms, k0, n_k, rp0, ent0, chunk, geom, atom_part, e_part, row_cell, k_cell, row_out, slice_part
    work0 = 0
    for f in range(F):
        n, k = n_atoms[f], n_k[f]
        assert list(rec[f, :4]) == [ap[f], n, kp[f], k]
        rows = -(-n // 16)
        geom, atom_part, e_part, row_cell, k_cell, row_out, slice_part = rec[f, 7:14]
        assert geom == work0 and atom_part == geom + 16 and e_part == atom_part + c * -(-n // 256)
        assert row_cell == e_part + rows and k_cell == row_cell + 9 * rows and row_out == k_cell + 10 * -(-k // 8)
        assert slice_part == row_out + (c + 3) * n
        work0 += int(lib.mipme_ewald_channels_step_work(n, k, c, cell))
    assert work0 == int(lib.mipme_ewald_channels_batch_work(F, ap.ctypes.data, kp.ctypes.data, c, cell))
    # refusals of the builder
    for bad_c in (1, 9):
        assert build(F, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, ns.ctypes.data, bad_c, cell, host.ctypes.data, n_bytes) == -1
        msg = lib.mipme_last_error()
        assert b"n_channels must be in 2..8" in msg and b"got %d" % bad_c in msg and b"mipme_ewald_batch_table_build" in msg, msg
    assert build(F, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, ns.ctypes.data, c, cell, host.ctypes.data, n_bytes - 8) == -1
    assert b"mipme_ewald_channels_batch_table_bytes says" in lib.mipme_last_error()
    assert build(F, ap.ctypes.data, kp.ctypes.data, None, ns.ctypes.data, c, cell, host.ctypes.data, n_bytes) == -1
    assert b"NULL array" in lib.mipme_last_error()


# ---- refusals of the entry points, with host pointers --------------------------------------------------------------------------
def _desc(**kw):
    return _lib.PotentialDesc(**{**dict(kind=_lib.COULOMB, exponent=1, smearing=1.0, prefactor=1.0, exclusion_radius=-1.0,
                                        exclusion_degree=1), **kw})


def test_step_entry_point_refusals_without_gpu():
    """Every refusal the arguments alone decide, with host pointers: -1 and the message, before any launch."""
    lib = _lib.load()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    smeared = _desc()

    def args(**over):
        f = dict(stream=None, dtype=_lib.F64, full_list=0, pot=C.pointer(smeared), n_atoms=4, n_k=8, lr_wavelength=1.25,
                 ns=(C.c_int32 * 3)(8, 7, 9), cell_gradient=1, positions=p, charges=p, cell=p, frequencies=p, multiplicities=p,
                 row_ptr=p, entries=p, shift_format=2, n_channels=3, records=p, kvectors=p, G=p, dG=p, s_cos=p, s_sin=p, energy=p,
                 forces=p, grad_charges=p, grad_cell=p, status=p, work=p)
        f.update(over)
        return _lib.EwaldChannelsStepArgs(**f)

    def refused(a, *needles):
        assert lib.mipme_ewald_channels_step(None if a is None else C.byref(a)) == -1
        msg = lib.mipme_last_error()
        for needle in needles:
            assert needle in msg, msg

    refused(None, b"NULL argument struct")
    bad = args()
    bad.version = 7
    refused(bad, b"version 7")
    bad = args()
    bad.size = 8
    refused(bad, b"implausible argument struct size 8")
    for c in (1, 9, 0, -1):
        refused(args(n_channels=c), b"mipme_ewald_channels_step: n_channels must be in 2..8", b"got %d" % c, b"mipme_ewald_step)")
    refused(args(dtype=5), b"invalid dtype")
    refused(args(pot=None), b"potential descriptor is NULL")
    refused(args(pot=C.pointer(_desc(smearing=-1.0))), b"has no smearing")
    refused(args(pot=C.pointer(_desc(exclusion_radius=2.0, exclusion_degree=0))), b"exclusion_degree must be >= 1")
    refused(args(pot=C.pointer(_desc(kind=_lib.INVERSE_POWER_LAW, exponent=7))), b"Unsupported exponent: 7")
    refused(args(n_k=-1), b"n_k must be >= 0")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    for n in (0, -3, (1 << 22) + 1):
        refused(args(n_atoms=n), b"n_atoms must be in 1..2^22")
    refused(args(lr_wavelength=0.0), b"lr_wavelength must be positive")
    refused(args(ns=(C.c_int32 * 3)(8, 0, 9)), b"ns >= 1")
    refused(args(grad_cell=None), b"cell_gradient needs grad_cell")
    refused(args(dG=None), b"cell_gradient needs dG")
    for name in ("positions", "charges", "cell", "row_ptr", "entries", "records", "energy", "forces", "grad_charges", "status", "work",
                 "frequencies", "multiplicities", "kvectors", "G", "s_cos", "s_sin"):
        refused(args(**{name: None}), b"NULL required buffer")
    refused(args(n_k=0, frequencies=None, multiplicities=None, kvectors=None, G=None, dG=None, s_cos=None, s_sin=None, cell_gradient=0,
                 grad_cell=None, work=None), b"NULL required buffer")


def test_batch_entry_point_refusals_without_gpu():
    lib = _lib.load()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    smeared = _desc()
    ap, kp = _ptrs([4, 2], [8, 0])
    ep = np.array([0, 7, 10], dtype=np.int64)

    def args(**over):
        f = dict(stream=None, dtype=_lib.F64, full_list=0, pot=C.pointer(smeared), n_frames=2, cell_gradient=1, lr_wavelength=1.25,
                 atom_ptr=ap.ctypes.data, k_ptr=kp.ctypes.data, entry_ptr=ep.ctypes.data, device_table=p, positions=p, charges=p,
                 cells=p, frequencies=p, multiplicities=p, row_ptr=p, entries=p, shift_format=2, n_channels=2, records=p, kvectors=p,
                 G=p, dG=p, s_cos=p, s_sin=p, energies=p, forces=p, grad_charges=p, grad_cells=p, status=p, work=p)
        f.update(over)
        return _lib.EwaldChannelsBatchArgs(**f)

    def refused(a, *needles):
        assert lib.mipme_ewald_channels_batch(None if a is None else C.byref(a)) == -1
        msg = lib.mipme_last_error()
        for needle in needles:
            assert needle in msg, msg

    refused(None, b"NULL argument struct")
    bad = args()
    bad.version = 7
    refused(bad, b"version 7")
    bad = args()
    bad.size = 8
    refused(bad, b"implausible argument struct size 8")
    for c in (1, 9, 0, -1):
        refused(args(n_channels=c), b"mipme_ewald_channels_batch: n_channels must be in 2..8", b"got %d" % c, b"mipme_ewald_batch)")
    refused(args(dtype=5), b"invalid dtype")
    refused(args(pot=None), b"potential descriptor is NULL")
    refused(args(pot=C.pointer(_desc(smearing=-1.0))), b"has no smearing")
    refused(args(pot=C.pointer(_desc(kind=_lib.INVERSE_POWER_LAW, exponent=7))), b"Unsupported exponent: 7")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    for n in (0, (1 << 20) + 1):
        refused(args(n_frames=n), b"n_frames must be in 1..2^20")
    refused(args(lr_wavelength=0.0), b"lr_wavelength must be positive")
    for name in ("atom_ptr", "k_ptr", "entry_ptr", "device_table"):
        refused(args(**{name: None}), b"NULL required buffer (atom_ptr, k_ptr, entry_ptr, device_table)")
    too_many = np.array([0, (1 << 22) + 1, (1 << 22) + 3], dtype=np.int64)
    refused(args(atom_ptr=too_many.ctypes.data), b"sizes the batch does not serve")
    refused(args(grad_cells=None), b"cell_gradient needs grad_cells")
    refused(args(dG=None), b"cell_gradient needs dG")
    for name in ("positions", "charges", "cells", "row_ptr", "entries", "records", "energies", "forces", "grad_charges", "status",
                 "work", "frequencies", "multiplicities", "kvectors", "G", "s_cos", "s_sin"):
        refused(args(**{name: None}), b"NULL required buffer")


# ---- refusals of the Python classes, on CPU tensors ---------------------------------------------------------------------------
Z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
EYE = torch.eye(3, dtype=F64) * 8
IDX = torch.tensor([[0, 1]])
CALC = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=1.0), lr_wavelength=2.0)


def _step(q=None, cell=EYE, pos=None, **kw):
    return tpa.GraphedEwaldStep(CALC, Z(2, 1) if q is None else q, cell, Z(2, 3) if pos is None else pos, IDX, Z(1, 3), **kw)


def _batch(qs, **kw):
    return tpa.GraphedEwaldBatch(CALC, [(q, EYE, Z(q.shape[0], 3) if q.dim() == 2 else Z(2, 3), IDX, Z(1, 3)) for q in qs], **kw)


def _message(fn, *args, **kw):
    with pytest.raises(ValueError) as err:
        fn(*args, **kw)
    return str(err.value)


def test_the_keyword_is_the_last_one_and_defaults_to_one():
    import inspect

    for cls in (tpa.GraphedEwaldStep, tpa.GraphedEwaldBatch):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "n_channels" and params[-1].default == 1 and params[-2].name == "warmup"
    last = list(inspect.signature(G._check_ewald_system).parameters.values())[-1]
    assert last.name == "n_channels" and last.default == 1


@pytest.mark.parametrize("bad", [0, 9, -1, 2.0, "2", None, True, np.int64(2)])
def test_n_channels_must_be_an_int_in_1_to_8(bad):
    for make in (lambda: _step(q=Z(2, 2), n_channels=bad), lambda: _batch([Z(2, 2)], n_channels=bad)):
        msg = _message(make)
        assert "`n_channels` must be an int in 1..8" in msg and repr(bad) in msg


def test_charges_must_be_n_atoms_by_n_channels():
    for q, shape in ((Z(2, 1), "[2, 1]"), (Z(2, 2), "[2, 2]"), (Z(2), "[2]"), (Z(2, 3, 1), "[2, 3, 1]")):
        msg = _message(_step, q=q, n_channels=3)
        assert msg.startswith("GraphedEwaldStep: `charges` must be a tensor with shape [n_atoms, n_channels] = [n_atoms, 3]")
        assert "n_channels = 3" in msg and msg.endswith(f"got tensor with shape {shape}")
    # the atoms of the charges are those of the positions
    assert "`positions` must be a tensor with shape [n_atoms, 3] with n_atoms = 3" in _message(_step, q=Z(3, 2), n_channels=2)
    # the batch names the frame; the same C for all frames
    msg = _message(_batch, [Z(2, 3), Z(2, 2)], n_channels=3)
    assert msg.startswith("GraphedEwaldBatch: frame 1: `charges` must be a tensor with shape [n_atoms, n_channels] = [n_atoms, 3]")
    assert msg.endswith("got tensor with shape [2, 2]")
    msg = _message(_batch, [Z(2, 1), Z(2, 3)], n_channels=3)
    assert msg.startswith("GraphedEwaldBatch: frame 0: ") and msg.endswith("got tensor with shape [2, 1]")
    # every other rule is the single-channel one
    assert "`cell` must be a tensor with shape [3, 3]" in _message(_step, q=Z(2, 2), cell=Z(3), n_channels=2)
    assert "share one dtype" in _message(_step, q=torch.zeros(2, 2), n_channels=2)


def test_without_the_keyword_the_refusals_are_the_single_channel_sentences():
    """(N, 2) charges without the keyword, or with n_channels=1: today's sentences, compared as strings with what the helper
    produces for one channel and with the sentences themselves."""
    step_sentence = ("GraphedEwaldStep handles a single charge channel, `charges` of shape [n_atoms, 1], got tensor with shape "
                     "[2, 2]")
    batch_sentence = ("GraphedEwaldBatch: frame 1: a single charge channel, `charges` of shape [n_atoms, 1], got tensor with shape "
                      "[2, 2]")
    helper_step = _message(G._check_ewald_system, "GraphedEwaldStep", Z(2, 2), EYE, Z(2, 3))
    helper_batch = _message(G._check_ewald_system, "GraphedEwaldBatch", Z(2, 2), EYE, Z(2, 3), frame=1, first=EYE)
    assert helper_step == step_sentence and helper_batch == batch_sentence
    assert _message(G._check_ewald_system, "GraphedEwaldStep", Z(2, 2), EYE, Z(2, 3), n_channels=1) == step_sentence
    for kw in ({}, {"n_channels": 1}):
        assert _message(_step, q=Z(2, 2), **kw) == step_sentence
        assert _message(_batch, [Z(2, 1), Z(2, 2)], **kw) == batch_sentence
        assert _message(_step, q=Z(2), **kw) == step_sentence.replace("[2, 2]", "[2]")
        # the rules behind the charges, too
        for other in (dict(pos=Z(3, 3)), dict(cell=Z(3)), dict(q=torch.zeros(2, 1))):
            want = _message(G._check_ewald_system, "GraphedEwaldStep", other.get("q", Z(2, 1)), other.get("cell", EYE),
                            other.get("pos", Z(2, 3)))
            assert _message(_step, **other, **kw) == want


def test_valid_input_on_the_cpu_has_no_fallback():
    for c in (2, 3, 8):
        with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
            _step(q=Z(2, c), n_channels=c)
        with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
            _batch([Z(2, c), Z(2, c)], n_channels=c, cell_gradient=True)
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        _step(n_channels=1)


def test_charges_of_a_call_must_have_the_exact_shape():
    """The shape check of ``charges=`` in a call, on the host side of the objects (no buffers, nothing launched)."""
    step = tpa.GraphedEwaldStep.__new__(tpa.GraphedEwaldStep)
    step.n_atoms, step.n_channels = 5, 3
    for bad in (Z(5, 1), Z(5), Z(1, 3), Z(5, 4), Z(15)):
        msg = _message(step, charges=bad)
        assert "`charges` must be a tensor with shape [n_atoms, n_channels] = [5, 3]" in msg and str(list(bad.shape)) in msg
    batch = tpa.GraphedEwaldBatch.__new__(tpa.GraphedEwaldBatch)
    batch.n_frames, batch.n_channels, batch.atom_ptr = 2, 3, [0, 2, 7]
    for bad in (Z(7, 1), Z(7), Z(21), Z(6, 3)):
        assert "= [7, 3]" in _message(batch, charges=bad)
    assert "frame 1: `charges` must be a tensor with shape [n_atoms, n_channels] = [5, 3]" in _message(batch, charges=[Z(2, 3), Z(5, 1)])
    assert "a list of 2 per-frame tensors wanted, got 1" in _message(batch, charges=[Z(7, 3)])
