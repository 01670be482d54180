"""CPU tests (no GPU) of the batched dipole step: the C-ABI mirror of ``mipme_dipole_batch_args_t``, the exported symbols, the
sizes of the scratch and of the frame table, the table itself for a heterogeneous set of frames, the refusals of the entry point
(host pointers: it must return before any launch) and of ``GraphedDipoleBatch``."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
FRAME_BYTES, BLOCK_BYTES = 152, 8  # include/mipme.h: per frame, per workgroup


def test_class_is_exported():
    assert hasattr(tpa, "GraphedDipoleBatch")
    assert "GraphedDipoleBatch" in tpa.__all__


def test_struct_mirrors_the_header_field_by_field():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mipme_dipole_batch_args \{(.*?)\} mipme_dipole_batch_args_t;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    parsed = [re.search(r"(\w+)(?:\[(\d+)\])?$", d) for d in decls]
    names = [m.group(1) for m in parsed]
    assert names == [n for n, _ in _lib.DipoleBatchArgs._fields_]
    assert names[:2] == ["size", "version"]
    # the fields of the Ewald batch, with self_term and background behind pot, dipoles for charges, grad_dipoles for grad_charges
    ewald = [n for n, _ in _lib.EwaldBatchArgs._fields_]
    at = ewald.index("pot") + 1
    swap = {"charges": "dipoles", "grad_charges": "grad_dipoles"}
    assert names == [swap.get(n, n) for n in ewald[:at]] + ["self_term", "background"] + [swap.get(n, n) for n in ewald[at:]]
    # offsets: every field is 8 bytes wide except the int32 / uint32 ones, which come in pairs -- no padding anywhere
    offset = 0
    for d, m in zip(decls, parsed):
        name = m.group(1)
        width = (4 if re.match(r"(u?int32_t)\b", d) else 8) * int(m.group(2) or 1)
        assert getattr(_lib.DipoleBatchArgs, name).offset == offset, name
        assert getattr(_lib.DipoleBatchArgs, name).size == width, name
        offset += width
    assert C.sizeof(_lib.DipoleBatchArgs) == offset == 256
    assert int(re.search(r"#define MIPME_DIPOLE_BATCH_VERSION (\d+)", hdr).group(1)) == _lib.DIPOLE_BATCH_VERSION == 1
    a = _lib.DipoleBatchArgs(n_frames=3, lr_wavelength=1.25, self_term=0.5)
    assert a.size == 256 and a.version == 1 and a.n_frames == 3 and a.lr_wavelength == 1.25 and a.self_term == 0.5
    with pytest.raises(TypeError, match="unknown field"):
        _lib.DipoleBatchArgs(no_such_field=1)


def test_symbols_are_declared_and_exported_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "mipme.h")).read()
    lib = _lib.load()
    for name in ("mipme_dipole_batch", "mipme_dipole_batch_work", "mipme_dipole_batch_table_bytes", "mipme_dipole_batch_table_build"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    # appended entry points do not move the version
    assert int(re.search(r"#define MIPME_VERSION (\d+)", hdr).group(1)) == 408
    assert lib.mipme_version() == 408


def _ptrs(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _sizes(n_atoms, n_k, cell):
    lib = _lib.load()
    ap, kp = _ptrs(n_atoms), _ptrs(n_k)
    return (int(lib.mipme_dipole_batch_work(len(n_atoms), ap.ctypes.data, kp.ctypes.data, cell)),
            int(lib.mipme_dipole_batch_table_bytes(len(n_atoms), ap.ctypes.data, kp.ctypes.data, cell)))


def _slices(n, k):
    """the dipole step's rule: slices of at least 1 024 k-vectors"""
    return 0 if k == 0 else max(1, min(-(-2048 // n), max(1, k // 1024)))


def _frame_work(n, k, cell):
    """include/mipme.h: geometry 16, 3 dipole partials per 256 atoms, energy partials per 16 atoms, with the cell gradient 9 per row
    block and 10 per block of 8 k-vectors, row results 6 N, slice partials 6 N S."""
    fin = -(-n // 16)
    return 16 + 3 * -(-n // 256) + fin + (9 * fin + 10 * -(-k // 8) if cell else 0) + 6 * n + 6 * n * _slices(n, k)


def _frame_blocks(n, k):
    """workgroups of the prep, k, atom and row launches of one frame"""
    return max(1, -(-k // 256)) + -(-n // 256), -(-k // 8), n * _slices(n, k), -(-n // 16)


def test_work_and_table_sizes():
    lib = _lib.load()
    assert lib.mipme_dipole_batch_work.restype is C.c_int64 and lib.mipme_dipole_batch_table_bytes.restype is C.c_int64
    # invalid: no frames, too many, an empty frame, a frame beyond 2^22 atoms, a negative k count, arrays that do not start at 0
    one = np.array([0, 4], dtype=np.int64)
    for n_frames, ap, kp in ((0, one, one), (-1, one, one), ((1 << 20) + 1, one, one), (1, np.array([0, 0], dtype=np.int64), one),
                             (1, np.array([0, (1 << 22) + 1], dtype=np.int64), one), (1, one, np.array([0, -1], dtype=np.int64)),
                             (1, np.array([1, 4], dtype=np.int64), one), (1, one, np.array([2, 4], dtype=np.int64)),
                             (2, np.array([0, 1 << 22, 1 << 23], dtype=np.int64), np.array([0, 1 << 30, 1 << 31], dtype=np.int64))):
        for cell in (0, 1):
            assert lib.mipme_dipole_batch_work(n_frames, ap.ctypes.data, kp.ctypes.data, cell) == 0
            assert lib.mipme_dipole_batch_table_bytes(n_frames, ap.ctypes.data, kp.ctypes.data, cell) == 0
    assert lib.mipme_dipole_batch_work(1, None, one.ctypes.data, 0) == 0 and lib.mipme_dipole_batch_table_bytes(1, one.ctypes.data, None, 0) == 0
    # three cases by hand
    # (a) one atom without k-vectors, no cell gradient: 16 + 3 + 1 + 6; prep 1 + 1, k 0, atoms 0, rows 1
    assert _sizes([1], [0], 0) == (26, FRAME_BYTES + BLOCK_BYTES * 3)
    # (b) 17 atoms, 110 k-vectors, cell gradient: 16 + 3 + 2 + 9 * 2 + 10 * 14 + 102 + 102 (one slice); prep 2, k 14, atoms 17, rows 2
    assert _sizes([17], [110], 1) == (383, FRAME_BYTES + BLOCK_BYTES * 35)
    # (c) 300 atoms with 2 048 k-vectors (2 slices: 2048 // 1024) beside (a), cell gradient: the sum of the frames' parts
    big = 16 + 6 + 19 + 9 * 19 + 10 * 256 + 1800 + 1800 * 2
    assert _frame_work(300, 2048, 1) == big and _frame_blocks(300, 2048) == (8 + 2, 256, 600, 19)
    assert _sizes([1, 300], [0, 2048], 1) == (26 + 9 + big, 2 * FRAME_BYTES + BLOCK_BYTES * (3 + 10 + 256 + 600 + 19))
    # the batch is the sum of the single steps
    for cell in (0, 1):
        n_atoms, n_k = [1, 2, 17, 24, 300, 4096], [0, 5, 110, 250, 2048, 16384]
        want = sum(int(lib.mipme_dipole_cell_step_work(n, k, cell)) for n, k in zip(n_atoms, n_k))
        assert _sizes(n_atoms, n_k, cell)[0] == want == sum(_frame_work(n, k, cell) for n, k in zip(n_atoms, n_k))


def _build(n_atoms, n_k, n_pairs, cell, ns=None):
    lib = _lib.load()
    F = len(n_atoms)
    ap, kp, ep = _ptrs(n_atoms), _ptrs(n_k), _ptrs([2 * p + 1 for p in n_pairs])
    ns = np.ascontiguousarray(np.arange(1, 3 * F + 1, dtype=np.int32).reshape(F, 3) if ns is None else ns)
    n_bytes = int(lib.mipme_dipole_batch_table_bytes(F, ap.ctypes.data, kp.ctypes.data, cell))
    host = np.full(n_bytes, 0xAB, dtype=np.uint8)
    rc = lib.mipme_dipole_batch_table_build(F, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, ns.ctypes.data, cell, host.ctypes.data, n_bytes)
    return rc, host, (ap, kp, ep, ns)


@pytest.mark.parametrize("cell", [0, 1])
def test_block_table_of_a_heterogeneous_batch(cell):
    """One 4 096-atom frame among small ones (one of them without k-vectors, one with a single atom, one with 17 slices): every
    (frame, local block) of every launch exactly once and in frame order, no block outside its frame, and the frames' slices and
    work areas where the prefix sums put them."""
    n_atoms, n_k, n_pairs = [20, 4096, 1, 3, 300, 17], [62, 16384, 0, 17968, 2048, 110], [30, 40000, 0, 1, 3457, 32]
    rc, host, (ap, kp, ep, ns) = _build(n_atoms, n_k, n_pairs, cell)
    assert rc == 0
    F = len(n_atoms)
    frames = host[: F * FRAME_BYTES].reshape(F, FRAME_BYTES)
    i64 = frames[:, :112].copy().view(np.int64)  # atom0, N, k0, K, rp0, ent0, chunk | geom, mu, e, row_cell, k_cell, row_out, slices
    i32 = frames[:, 112:].copy().view(np.int32)  # table, atom, fin, row, k blocks, slices | ns[3], pad
    assert [_slices(n, k) for n, k in zip(n_atoms, n_k)] == [1, 1, 0, 17, 2, 1]
    work0 = 0
    for f in range(F):
        n, k = n_atoms[f], n_k[f]
        s = _slices(n, k)
        assert list(i64[f, :6]) == [ap[f], n, kp[f], k, 2 * ap[f] + f, ep[f]]
        assert i64[f, 6] == (0 if s == 0 else -(-k // s))
        fin, kb = -(-n // 16), -(-k // 8) if cell else 0
        parts = [16, 3 * -(-n // 256), fin, 9 * fin if cell else 0, 10 * kb, 6 * n]
        assert list(i64[f, 7:14]) == [work0 + sum(parts[:j]) for j in range(7)]
        assert list(i32[f, :6]) == [max(1, -(-k // 256)), -(-n // 256), fin, fin if cell else 0, kb, s]
        assert list(i32[f, 6:9]) == list(ns[f]) and i32[f, 9] == 0
        work0 += _frame_work(n, k, cell)
    assert work0 == _sizes(n_atoms, n_k, cell)[0]
    blocks = host[F * FRAME_BYTES:].copy().view(np.int32).reshape(-1, 2)
    start = 0
    for which in range(4):  # prep, k, atoms, rows
        per_frame = [_frame_blocks(n, k)[which] for n, k in zip(n_atoms, n_k)]
        want = np.array([(f, b) for f, count in enumerate(per_frame) for b in range(count)], dtype=np.int32).reshape(-1, 2)
        got = blocks[start : start + len(want)]
        assert np.array_equal(got, want), which
        start += len(want)
    assert start == len(blocks)
    # the small frames do not pay for the large one: 20 atoms cost 20 atom blocks, not 4 096
    assert _frame_blocks(20, 62)[2] == 20 and _frame_blocks(3, 17968)[2] == 51


def test_table_build_refusals():
    lib = _lib.load()

    def refused(rc, needle):
        assert rc == -1
        msg = lib.mipme_last_error()
        assert needle in msg, msg

    rc, host, (ap, kp, ep, ns) = _build([4, 5], [8, 0], [3, 0], 1)
    assert rc == 0
    n = len(host)
    build = lib.mipme_dipole_batch_table_build
    refused(build(0, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, ns.ctypes.data, 1, host.ctypes.data, n), b"n_frames must be in 1..2^20")
    refused(build(2, ap.ctypes.data, kp.ctypes.data, None, ns.ctypes.data, 1, host.ctypes.data, n), b"NULL array")
    refused(build(2, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, ns.ctypes.data, 1, host.ctypes.data, n - 8), b"host_table_bytes")
    bad_ns = ns.copy()
    bad_ns[1, 2] = 0
    refused(build(2, ap.ctypes.data, kp.ctypes.data, ep.ctypes.data, bad_ns.ctypes.data, 1, host.ctypes.data, n), b"frame 1: ns must be >= 1")
    bad_ep = ep.copy()
    bad_ep[2] = bad_ep[1]  # (a frame without its one entry word)
    refused(build(2, ap.ctypes.data, kp.ctypes.data, bad_ep.ctypes.data, ns.ctypes.data, 1, host.ctypes.data, n), b"sizes the batch does not serve")


def test_entry_point_refusals_without_gpu():
    """Every refusal the arguments alone decide, with host pointers: -1 and the message, before any launch."""
    lib = _lib.load()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    desc = lambda **kw: _lib.DipoleDesc(**{**dict(smearing=1.0, prefactor=1.0, exclusion_radius=-1.0, exclusion_degree=1), **kw})  # noqa: E731
    smeared, direct = desc(), desc(smearing=-1.0)
    ap, kp, ep = _ptrs([4, 5]), _ptrs([8, 0]), _ptrs([7, 1])
    none = _ptrs([0, 0])

    def args(**over):
        f = dict(stream=None, dtype=_lib.F64, full_list=0, pot=C.pointer(smeared), self_term=0.1, background=0.0, n_frames=2,
                 cell_gradient=1, lr_wavelength=1.25, atom_ptr=ap.ctypes.data, k_ptr=kp.ctypes.data, entry_ptr=ep.ctypes.data,
                 device_table=p, positions=p, dipoles=p, cells=p, frequencies=p, multiplicities=p, row_ptr=p, entries=p, shift_format=2,
                 records=p, kvectors=p, G=p, dG=p, s_cos=p, s_sin=p, energies=p, forces=p, grad_dipoles=p, grad_cells=p, status=p, work=p)
        f.update(over)
        return _lib.DipoleBatchArgs(**f)

    def refused(a, needle):
        assert lib.mipme_dipole_batch(None if a is None else C.byref(a)) == -1
        msg = lib.mipme_last_error()
        assert needle in msg, msg

    refused(None, b"NULL argument struct")
    bad = args()
    bad.version = 7
    refused(bad, b"version 7")
    bad = args()
    bad.size = 8
    refused(bad, b"implausible argument struct size 8")
    refused(args(dtype=5), b"invalid dtype")
    refused(args(pot=None), b"dipole descriptor is NULL")
    refused(args(pot=C.pointer(desc(exclusion_radius=2.0, exclusion_degree=0))), b"exclusion_degree must be >= 1")
    for fmt in (0, 1, 2 | _lib.ROWS_PADDED):
        refused(args(shift_format=fmt), b"shift_format 2")
    for n in (0, -3, (1 << 20) + 1):
        refused(args(n_frames=n), b"n_frames must be in 1..2^20")
    for name in ("atom_ptr", "k_ptr", "entry_ptr", "device_table"):
        refused(args(**{name: None}), b"NULL required buffer")
    empty = _ptrs([4, 0])
    refused(args(atom_ptr=empty.ctypes.data), b"sizes the batch does not serve")
    # k-vectors need smearing; lr_wavelength <= 0 only without k-vectors AND without smearing
    refused(args(pot=C.pointer(direct)), b"has no smearing")
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        refused(args(lr_wavelength=lam), b"lr_wavelength must be positive")
    refused(args(lr_wavelength=0.0, k_ptr=none.ctypes.data), b"lr_wavelength must be positive")  # (smearing, no k-vectors)
    refused(args(grad_cells=None), b"cell_gradient needs grad_cells")
    refused(args(dG=None), b"cell_gradient needs dG")
    for name in ("positions", "dipoles", "cells", "row_ptr", "entries", "records", "energies", "forces", "grad_dipoles", "status", "work",
                 "frequencies", "multiplicities", "kvectors", "G", "s_cos", "s_sin"):
        refused(args(**{name: None}), b"NULL required buffer")
    # a direct potential without k-vectors and lr_wavelength 0 passes every check of the sizes: what is left to object to is a
    # required buffer (none of the reciprocal ones)
    refused(args(pot=C.pointer(direct), lr_wavelength=0.0, k_ptr=none.ctypes.data, frequencies=None, multiplicities=None,
                 kvectors=None, G=None, dG=None, s_cos=None, s_sin=None, cell_gradient=0, grad_cells=None, work=None),
            b"NULL required buffer")


def test_python_refusals():
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    eye = torch.eye(3, dtype=F64) * 8
    idx = torch.tensor([[0, 1]])
    calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0), lr_wavelength=2.0)
    good = (z(2, 3), eye, z(2, 3), idx, z(1, 3))

    def frame(mu=None, cell=eye, pos=None, idx=idx, sh=None):
        return (z(2, 3) if mu is None else mu, cell, z(2, 3) if pos is None else pos, idx, z(1, 3) if sh is None else sh)

    def batch(frames, calc=calc):
        return tpa.GraphedDipoleBatch(calc, frames)

    with pytest.raises(TypeError, match="GraphedDipoleBatch serves a CalculatorDipole, got a EwaldCalculator: use GraphedEwaldBatch or "
                                        "GraphedFrameBatch for charges"):
        batch([good], calc=tpa.EwaldCalculator(tpa.CoulombPotential(smearing=1.0), lr_wavelength=2.0))
    with pytest.raises(TypeError, match="CalculatorDipole, got a PMECalculator"):
        batch([good], calc=tpa.PMECalculator(tpa.CoulombPotential(smearing=1.0), mesh_spacing=0.6))
    with pytest.raises(ValueError, match="GraphedDipoleBatch: `frames` is empty"):
        batch([])
    with pytest.raises(ValueError, match="frame 1 must be .* got 4 items"):
        batch([good, good[:4]])
    with pytest.raises(ValueError, match=r"GraphedDipoleBatch: frame 1: `dipoles` must be a tensor with shape \[n_atoms, 3\].*\[2, 1\]"):
        batch([good, frame(mu=z(2, 1))])
    with pytest.raises(ValueError, match=r"frame 0: `dipoles` must be a tensor with shape \[n_atoms, 3\].*\[2\]"):
        batch([frame(mu=z(2))])
    with pytest.raises(ValueError, match=r"frame 2: `positions` must be a tensor with shape \[n_atoms, 3\] with n_atoms = 2 \(the "
                                         r"dipoles\).*\[3, 3\]"):
        batch([good, good, frame(pos=z(3, 3))])
    with pytest.raises(ValueError, match=r"frame 0: `cell` must be a tensor with shape \[3, 3\].*\[3\]"):
        batch([frame(cell=z(3))])
    with pytest.raises(ValueError, match="frame 1: .*share one dtype.*float32"):
        batch([good, frame(mu=torch.zeros(2, 3, dtype=torch.float32))])
    with pytest.raises(ValueError, match=r"frame 1: .*share one dtype.*\(frame 0: torch.float64\)"):
        batch([good, tuple(t.float() if t.is_floating_point() else t for t in good)])
    with pytest.raises(ValueError, match=r"frame 1: the cell shifts must be integers in \[-3, 3\]"):
        batch([good, frame(sh=torch.tensor([[0.0, 4.0, 0.0]], dtype=F64))])
    with pytest.raises(ValueError, match=r"frame 0: the cell shifts must be integers in \[-3, 3\]"):
        batch([frame(sh=torch.tensor([[0.0, 0.5, 0.0]], dtype=F64))])
    with pytest.raises(ValueError, match=r"frame 1: `neighbor_shifts` must be a tensor with shape \[n_pairs, 3\]"):
        batch([good, frame(sh=z(2, 3))])
    with pytest.raises(ValueError, match=r"frame 1: `neighbor_indices` must be a tensor with shape \[n_pairs, 2\]"):
        batch([good, frame(idx=torch.zeros((1, 3), dtype=torch.long))])
    with pytest.raises(ValueError, match=r"frame 1: a frame holds 1 to 2\^22 atoms"):
        batch([good, (z(0, 3), eye, z(0, 3), torch.zeros((0, 2), dtype=torch.long), z(0, 3))])
    singular = eye.clone()
    singular[2] = singular[0]
    direct = tpa.CalculatorDipole(tpa.PotentialDipole(), lr_wavelength=None)
    for c in (calc, direct):
        with pytest.raises(ValueError, match="frame 1: provided `cell` has a determinant of .*not a valid unit cell"):
            batch([good, frame(cell=singular)], calc=c)
    # everything in order but on the CPU
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        batch([good, good])
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        batch([good], calc=direct)
    with pytest.raises(tpa.MipmeError, match="no CPU fallback"):
        batch([good], calc=tpa.CalculatorDipole(tpa.PotentialDipole(smearing=1.0, exclusion_radius=2.0, exclusion_degree=3, epsilon=1.5),
                                                lr_wavelength=2.0, full_neighbor_list=True))


def test_the_batches_share_their_packing():
    """GraphedEwaldBatch and GraphedDipoleBatch pack, install, warm up and load through one private base."""
    from torchpme_amd import graphed

    for name in ("_pack", "_install", "_warm_up", "_load", "_recapture"):
        assert getattr(tpa.GraphedDipoleBatch, name) is getattr(tpa.GraphedEwaldBatch, name) is getattr(graphed._FrameTableBatch, name)
    assert tpa.GraphedDipoleBatch._who == "GraphedDipoleBatch" and tpa.GraphedEwaldBatch._who == "GraphedEwaldBatch"
    assert tpa.GraphedDipoleBatch._table_build == "mipme_dipole_batch_table_build"


def test_kgrid_matches_is_decided_per_frame_on_the_host():
    from torchpme_amd.graphed import GraphedDipoleBatch

    batch = GraphedDipoleBatch.__new__(GraphedDipoleBatch)  # (the host side of the object: no buffers, nothing launched)
    c0, c1 = torch.eye(3, dtype=F64) * 1.2, torch.tensor([[9.0, 0.0, 0.0], [1.2, 8.4, 0.0], [-0.7, 0.9, 10.3]], dtype=F64)
    batch.n_frames, batch.lr_wavelength, batch.ns = 2, 1.25, [(1, 1, 1), (8, 7, 9)]
    assert batch.kgrid_matches([c0, c1]) == [True, True]
    assert batch.kgrid_matches(torch.stack([c0, 1.2 * c1])) == [True, False]
    assert batch.kgrid_matches([1.1 * c0, c1.float()]) == [False, True]
    with pytest.raises(ValueError, match="2 cells wanted"):
        batch.kgrid_matches([c0])
    # a direct potential sums no grid
    batch.lr_wavelength, batch.ns = 0.0, [(1, 1, 1), (1, 1, 1)]
    assert batch.kgrid_matches([1.5 * c0, 1.5 * c1]) == [True, True]
