"""The kernels of csrc/ewald.hip -- what ``EwaldCalculator`` runs -- and the reciprocal-space kernel function ``lr_kernel_dev`` of
csrc/kpot.h point by point, through the C entry points (ctypes, no probe library).

``test_filter_pointwise``: ``mipme_ewald_filter`` at k-vectors (kappa, 0, 0) against the mpmath values of
``tests/golden/ewald_pointwise.npz``, which are taken at the z = sigma^2 kappa^2 / 2 the kernel forms.  Every G(k) table of the
project -- mesh filters, combined filters, frame tables, the steps that follow their cell -- is built from this one function.

    float64   |got - ref| <= (2e-14 + 2^-51 z) |ref|      (the z term: the rounding of z itself moves exp(-z) by z eps)
    float32   2^-24 more: the value is computed in double and rounded once
    underflow the rule of ``check`` (tests/test_gpu_dipole_pointwise.py), and the number of points in that class is the one the
              golden file records; no point is dropped
    k = 0     dG is exactly 0; G is exactly 0 for p <= 3 and k0 = -c0/a for p > 3, which carries the host's rounding of c0 (pow,
              tgamma) and nothing else: held to the bound above

``test_reciprocal_edges`` and its companions: ``mipme_ewald_structure`` / ``_potential`` / ``_backward`` against numpy float64 sums
of the same (rounded) inputs, at the edges of their tiling, chunking and batching.
"""

import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_dipole_pointwise import DEV, DTYPES, Checks, _eps, _np, _t
from torchpme_amd import _lib

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 4, 5, 9)  # kEwaldCMax = 4 channels per pass: one pass, a ragged one, a full one, two and three passes


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "ewald_pointwise.npz"))


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- the kernel function ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("si", [0, 1, 2], ids=["s0.5", "s1.0", "s2.5"])
@pytest.mark.parametrize("p", range(1, 7))
def test_filter_pointwise(g, p, si, dtype):
    """G and dG/dk^2 of 1/r^p at the ~230 points of one smearing (module docstring), with and without the dG output.

    With the closed forms that kpot.h evaluated for every z before this test (f_p as a difference for p >= 4, f_p' from
    -(exp(-z) + a f_p)/z) the float64 cases missed the bound by: p = 4 G 5e2 (z = 700), dG 7e2 (z = 1e-12); p = 5 dG 6e6
    (z = 1e-11); p = 6 G 2e5 (z = 700), dG 2e9 (z = 1e-12) -- the CPU emulation of tests/test_ewald_pointwise_host.py; the device
    figures are in docs/KERNELS.md."""
    sigma = float(g["sigmas"][si])
    kappa, z = g[f"kappa_s{si}"], g[f"z_s{si}"]
    K = len(kappa)
    kvec = torch.zeros((K, 3), dtype=dtype, device=DEV)
    kvec[:, 0] = torch.tensor(kappa, device=DEV).to(dtype)
    assert np.array_equal(_np(kvec)[:, 0], kappa.astype(np.float64))  # float32 numbers: both precisions read the same input
    pot = _lib.PotentialDesc(kind=0 if p == 1 else 1, exponent=p, smearing=sigma, prefactor=1.0, exclusion_radius=-1.0,
                             exclusion_degree=1)
    lib, st, dt = _lib.load(), _lib.current_stream(DEV), _lib.dtype_code(dtype)
    G, dG, G_only = _nan((K,), dtype), _nan((K,), dtype), _nan((K,), dtype)
    _lib.check(lib.mipme_ewald_filter(st, dt, C.byref(pot), K, kvec.data_ptr(), G.data_ptr(), dG.data_ptr()))
    _lib.check(lib.mipme_ewald_filter(st, dt, C.byref(pot), K, kvec.data_ptr(), G_only.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(_bits(G), _bits(G_only))
    G, dG = _np(G), _np(dG)
    ref_G, ref_dG = g[f"G_p{p}_s{si}"], g[f"dG_p{p}_s{si}"]
    tol = 2e-14 + 2.0**-51 * z + (2.0**-24 if dtype == torch.float32 else 0.0)
    # k = 0
    assert z[0] == 0.0 and dG[0] == 0.0
    if p <= 3:
        assert G[0] == 0.0
    else:
        assert abs(G[0] - ref_G[0]) <= tol[0] * abs(ref_G[0]), (G[0], ref_G[0])
    checks = Checks()
    what = f"filter p={p} sigma={sigma}"
    counts = [checks(f"{what} G", dtype, G[1:], ref_G[1:], np.abs(ref_G[1:]), tol[1:])[1],
              checks(f"{what} dG/dk^2", dtype, dG[1:], ref_dG[1:], np.abs(ref_dG[1:]), tol[1:])[1]]
    checks.done()
    want = g["under32" if dtype == torch.float32 else "under64"][p - 1, si]
    assert counts == [int(c) for c in want], (counts, want)


# ---- the sums -----------------------------------------------------------------------------------------------------------------------
def _inputs(rng, N, K, C, lo=0.0, hi=8.0):
    """float64 inputs of one structure: positions in [lo, hi)^3, |k| in [0.3, 6], charges and upstream gradient (N, C), G in
    [0.1, 1] with exact zeros (every fourth k-vector or so, never the first), dG in [-1, -0.1]."""
    kdir = rng.normal(size=(K, 3))
    G = rng.uniform(0.1, 1.0, K)
    G[1:][rng.uniform(size=K - 1) < 0.25] = 0.0
    if K > 1:
        G[K // 2] = 0.0
    return dict(pos=rng.uniform(lo, hi, (N, 3)), kv=kdir / np.linalg.norm(kdir, axis=1)[:, None] * rng.uniform(0.3, 6.0, (K, 1)),
                q=rng.normal(size=(N, C)), g=rng.normal(size=(N, C)), G=G, dG=rng.uniform(-1.0, -0.1, K))


class _Device:
    """The inputs of B structures, stacked as the padded batch the entry points take, rounded to ``dtype`` on the device."""

    def __init__(self, dtype, structures):
        self.dtype, self.B = dtype, len(structures)
        for key in ("pos", "kv", "q", "g", "G", "dG"):
            setattr(self, key, _t(np.stack([s[key] for s in structures]), dtype))
        self.N, self.K, self.C = self.pos.shape[1], self.kv.shape[1], self.q.shape[2]

    def rounded(self, b):
        return {key: _np(getattr(self, key)[b]) for key in ("pos", "kv", "q", "g", "G", "dG")}

    def _head(self):
        return _lib.current_stream(DEV), _lib.dtype_code(self.dtype), self.N, self.C, self.K

    def structure(self, w):
        oc, os_ = _nan((self.B, self.K, self.C), self.dtype), _nan((self.B, self.K, self.C), self.dtype)
        _lib.check(_lib.load().mipme_ewald_structure(*self._head(), _ptr(self.pos), _ptr(w), _ptr(self.kv), oc.data_ptr(),
                                                     os_.data_ptr(), self.B))
        return oc, os_

    def potential(self, Sc, Ss):
        out = _nan((self.B, self.N, self.C), self.dtype)
        _lib.check(_lib.load().mipme_ewald_potential(*self._head(), _ptr(self.pos), _ptr(self.kv), _ptr(self.G), _ptr(Sc), _ptr(Ss),
                                                     out.data_ptr(), self.B))
        return out

    def backward(self, Sc, Ss, Tc, Ts, want_pos=True, want_k=True, with_dG=True):
        """Both gradient buffers are NaN-filled and returned; only those asked for are passed."""
        gpos, gk = _nan((self.B, self.N, 3), self.dtype), _nan((self.B, self.K, 3), self.dtype)
        _lib.check(_lib.load().mipme_ewald_backward(
            *self._head(), _ptr(self.pos), _ptr(self.q), _ptr(self.g), _ptr(self.kv), _ptr(self.G), _ptr(self.dG) if with_dG else None,
            _ptr(Sc), _ptr(Ss), _ptr(Tc), _ptr(Ts), gpos.data_ptr() if want_pos else None, gk.data_ptr() if want_k else None, self.B))
        return gpos, gk


def _fma(a, b, c):
    """fl(a b + c) in float64 with one rounding, from the error-free product (Veltkamp / Dekker) and sum (Knuth); the last
    addition rounds a second time only where the exact sum lies within 2^-106 of a rounding boundary."""
    p = a * b
    ah, bh = a * 134217729.0, b * 134217729.0  # 2^27 + 1
    ah, bh = ah - (ah - a), bh - (bh - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl  # a b = p + e exactly
    s = p + c
    v = s - p
    t = (p - (s - v)) + (c - v)  # p + c = s + t exactly
    return s + (t + e)


def _kernel_phase(kv, pos):
    """k.r (K, N) with the roundings of the float64 kernels, which the compiler contracts to fma(k_z, z, fma(k_x, x, k_y y)) (read
    from their code objects).  The one-term float64 cases hold the bound only against a reference whose phase is rounded as the
    kernel's is (see ``test_reciprocal_edges`` of the dipole file); a matrix product leaves that to the BLAS at hand, which adds
    in another order for some shapes.  For the float32 kernels, whose phase is exact products of floats added in double, the order
    is immaterial."""
    k, r = kv[:, None, :], pos[None, :, :]
    return _fma(k[..., 2], r[..., 2], _fma(k[..., 0], r[..., 0], k[..., 1] * r[..., 1]))


def _trig(x):
    phase = _kernel_phase(x["kv"], x["pos"])  # (K, N)
    return np.cos(phase), np.sin(phase), (float(np.abs(phase).max()) if phase.size else 0.0)


def _structure_reference(w, c, s):
    """S_c, S_s (K, C) and the sums of the absolute values of their terms."""
    return c @ w, s @ w, np.abs(c) @ np.abs(w), np.abs(s) @ np.abs(w)


def _potential_reference(x, c, s, Sc, Ss):
    Gc, Gs = x["G"][:, None] * c, x["G"][:, None] * s
    return Gc.T @ Sc + Gs.T @ Ss, np.abs(Gc).T @ np.abs(Sc) + np.abs(Gs).T @ np.abs(Ss)


def _backward_reference(x, c, s, Sc, Ss, Tc, Ts):
    """(dL/dr, its absolute sum, dL/dk, its absolute sum) with B[k,i] = sum_ch g (c S_s - s S_c) + q (c T_s - s T_c)."""
    q, gr, kv, pos, G, dG = x["q"], x["g"], x["kv"], x["pos"], x["G"], x["dG"]
    Bm = c * (Ss @ gr.T + Ts @ q.T) - s * (Sc @ gr.T + Tc @ q.T)
    aq, ag = np.abs(q), np.abs(gr)
    Ba = np.abs(c) * (np.abs(Ss) @ ag.T + np.abs(Ts) @ aq.T) + np.abs(s) * (np.abs(Sc) @ ag.T + np.abs(Tc) @ aq.T)
    dot, dot_abs = (Tc * Sc + Ts * Ss).sum(1), (np.abs(Tc * Sc) + np.abs(Ts * Ss)).sum(1)
    gpos, gpos_abs = (G[:, None] * Bm).T @ kv, (np.abs(G)[:, None] * Ba).T @ np.abs(kv)
    gk = G[:, None] * (Bm @ pos) + (2 * dG * dot)[:, None] * kv
    gk_abs = np.abs(G)[:, None] * (Ba @ np.abs(pos)) + (2 * np.abs(dG) * dot_abs)[:, None] * np.abs(kv)
    return gpos, gpos_abs, gk, gk_abs


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _run_and_check(checks, what, dev, nullable=False):
    """All four kernels on the structures of ``dev``, each structure against its own reference.  The structure factors handed to
    the later kernels are the references, rounded: every kernel is measured on its own."""
    N, K, C, dtype = dev.N, dev.K, dev.C, dev.dtype
    eps = _eps(dtype)
    Sc_d, Ss_d = dev.structure(dev.q)
    Tc_d, Ts_d = dev.structure(dev.g)
    xs = [dev.rounded(b) for b in range(dev.B)]
    trig = [_trig(x) for x in xs]
    refS = [_structure_reference(x["q"], c, s) for x, (c, s, _) in zip(xs, trig)]
    refT = [_structure_reference(x["g"], c, s) for x, (c, s, _) in zip(xs, trig)]
    Sc, Ss, Tc, Ts = (_t(np.stack([r[j] for r in ref]), dtype) for ref in (refS, refT) for j in (0, 1))
    out_d = dev.potential(Sc, Ss)
    gpos_d, gk_d = dev.backward(Sc, Ss, Tc, Ts)
    torch.cuda.synchronize()
    chunks = -(-C // 4)
    d_lane, d_lane_k, d_atom = -(-N // 32) + 5, chunks * -(-N // 32) + 5, -(-K // 256) + 6 + 3
    for b, (x, (c, s, phi)) in enumerate(zip(xs, trig)):
        tag = f"{what} C={C}" + (f" structure {b}" if dev.B > 1 else "")
        base = 8 + 2 * C + 4 * phi
        for name, got, ref in (("S", (Sc_d, Ss_d), refS[b]), ("T", (Tc_d, Ts_d), refT[b])):
            checks(f"{tag} structure {name} cos", dtype, _np(got[0][b]).ravel(), ref[0].ravel(), ref[2].ravel(), (d_lane + base) * eps)
            checks(f"{tag} structure {name} sin", dtype, _np(got[1][b]).ravel(), ref[1].ravel(), ref[3].ravel(), (d_lane + base) * eps)
        rSc, rSs, rTc, rTs = (_np(t[b]) for t in (Sc, Ss, Tc, Ts))
        ref, ref_abs = _potential_reference(x, c, s, rSc, rSs)
        checks(f"{tag} potential", dtype, _np(out_d[b]).ravel(), ref.ravel(), ref_abs.ravel(), (d_atom + base) * eps)
        gpos, gpos_abs, gk, gk_abs = _backward_reference(x, c, s, rSc, rSs, rTc, rTs)
        checks(f"{tag} dL/dr", dtype, _np(gpos_d[b]).ravel(), gpos.ravel(), gpos_abs.ravel(), (d_atom + base) * eps)
        checks(f"{tag} dL/dk", dtype, _np(gk_d[b]).ravel(), gk.ravel(), gk_abs.ravel(), (d_lane_k + base) * eps)
    if nullable:
        only_pos, untouched_k = dev.backward(Sc, Ss, Tc, Ts, want_k=False, with_dG=False)
        untouched_pos, only_k = dev.backward(Sc, Ss, Tc, Ts, want_pos=False)
        torch.cuda.synchronize()
        assert torch.equal(_bits(only_pos), _bits(gpos_d)) and torch.equal(_bits(only_k), _bits(gk_d)), what
        assert bool(torch.isnan(untouched_k).all()) and bool(torch.isnan(untouched_pos).all()), what
        with pytest.raises(ValueError, match="grad_kvectors needs dG"):
            dev.backward(Sc, Ss, Tc, Ts, with_dG=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K", [1, 7, 9, 255, 257, 1023])
@pytest.mark.parametrize("N", [1, 31, 33, 255, 257])
def test_reciprocal_edges(N, K, dtype):
    """Structure factors, potential, dL/dr and dL/dk for C = 1, 3, 4, 5, 9 channels: positions in a box of edge 8, |k| in [0.3, 6];
    N one off the 32 atom lanes and the 256-atom LDS tile; K one off the 8 k-vectors of a block and the stride of 256 with which the
    per-atom kernels walk the k-vectors; C across the passes of kEwaldCMax = 4 channels.  Every output is NaN-filled before the call.
    With every C also: ``grad_positions`` alone (and without dG) and ``grad_kvectors`` alone give the bits of the joint call and
    leave the other buffer's NaN fill alone, and ``grad_kvectors`` without dG is refused.

    Bound per output element: (d + 8 + 2C + 4 phi_max) eps S_abs, eps = 2^-24 / 2^-53 -- the bound of ``test_reciprocal_edges`` of
    tests/test_gpu_dipole_pointwise.py (which explains phi_max and the 8) with 2C more for the sum over the channels inside one
    term (two products and two additions per channel in ``ewald_bracket``), and d the depth of the kernel's own summation:
      structure factors      ceil(N/32) + 5        a lane adds every 32nd atom, then 5 shuffle steps
      dL/dk                  ceil(C/4) ceil(N/32) + 5    the same, but one accumulator runs through all passes over the channels
      potential, dL/dr       ceil(K/256) + 6 + 3   a thread adds every 256th k-vector, 6 shuffle steps, 3 additions of the wave sums

    One-term sums (N = 1) are where the bound asks most: next to a zero of cos or sin the phase has to be good to a few eps of its
    distance from that zero.  With the phase formed in float32 the N = 1 structure factors missed it by up to 1e3 in the CPU emulation;
    the kernels now take ``dipole_phase3``, which forms and reduces a float phase in double.  The device figures before and after
    are in docs/KERNELS.md.  In float64 the numpy reference rounds the phase the way the kernel does (see the dipole test)."""
    checks = Checks()
    for C in CHANNELS:
        rng = np.random.default_rng(100000 * C + 1000 * N + K)
        _run_and_check(checks, f"N={N} K={K}", _Device(dtype, [_inputs(rng, N, K, C)]), nullable=True)
    checks.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_far_atoms(dtype):
    """N = 33, K = 257 with positions in [-100, 100)^3, far outside any cell that would go with these k-vectors: |k.r| reaches 1e3.
    The bound of ``test_reciprocal_edges``."""
    checks = Checks()
    for C in (1, 5):
        rng = np.random.default_rng(77 + C)
        _run_and_check(checks, "far atoms N=33 K=257", _Device(dtype, [_inputs(rng, 33, 257, C, -100.0, 100.0)]))
    checks.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,K", [(33, 9), (257, 257)])
def test_reciprocal_batches(N, K, dtype):
    """Padded batches (blockIdx.y): B = 3 structures with positions, k-vectors, charges, G and dG of their own, each against its
    own reference with the bound of ``test_reciprocal_edges``.  A wrong offset shows as another structure's numbers."""
    checks = Checks()
    for C in (1, 5):
        rng = np.random.default_rng(31 * N + K + C)
        dev = _Device(dtype, [_inputs(rng, N, K, C) for _ in range(3)])
        assert not torch.equal(dev.pos[0], dev.pos[1]) and not torch.equal(dev.kv[1], dev.kv[2])
        _run_and_check(checks, f"batch N={N} K={K}", dev, nullable=True)
    checks.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_empty_sizes(dtype):
    """What the entry points do at K = 0 and N = 0, pinned: without k-vectors the potential and dL/dr are exact zeros and the
    structure call writes nothing; without atoms the structure factors are exact zeros, and so is dL/dk (S = T = 0)."""
    lib, st, dt = _lib.load(), _lib.current_stream(DEV), _lib.dtype_code(dtype)
    rng = np.random.default_rng(5)
    for C in (1, 5):
        N, K = 33, 0
        x = _inputs(rng, N, 1, C)
        pos, q, gr = _t(x["pos"], dtype), _t(x["q"], dtype), _t(x["g"], dtype)
        out, gpos, gk = _nan((N, C), dtype), _nan((N, 3), dtype), _nan((4, 3), dtype)
        oc, os_ = _nan((4, C), dtype), _nan((4, C), dtype)
        _lib.check(lib.mipme_ewald_structure(st, dt, N, C, K, pos.data_ptr(), q.data_ptr(), None, oc.data_ptr(), os_.data_ptr(), 1))
        _lib.check(lib.mipme_ewald_potential(st, dt, N, C, K, pos.data_ptr(), None, None, None, None, out.data_ptr(), 1))
        _lib.check(lib.mipme_ewald_backward(st, dt, N, C, K, pos.data_ptr(), q.data_ptr(), gr.data_ptr(), None, None, None, None, None,
                                            None, None, gpos.data_ptr(), gk.data_ptr(), 1))
        torch.cuda.synchronize()
        assert bool((out == 0).all()) and bool((gpos == 0).all())
        assert bool(torch.isnan(oc).all()) and bool(torch.isnan(os_).all()) and bool(torch.isnan(gk).all())

        N, K = 0, 9
        x = _inputs(rng, 1, K, C)
        kv, G, dG = _t(x["kv"], dtype), _t(x["G"], dtype), _t(x["dG"], dtype)
        zero = torch.zeros((K, C), dtype=dtype, device=DEV)
        oc, os_, gk, gpos = _nan((K, C), dtype), _nan((K, C), dtype), _nan((K, 3), dtype), _nan((4, 3), dtype)
        _lib.check(lib.mipme_ewald_structure(st, dt, N, C, K, None, None, kv.data_ptr(), oc.data_ptr(), os_.data_ptr(), 1))
        _lib.check(lib.mipme_ewald_backward(st, dt, N, C, K, None, None, None, kv.data_ptr(), G.data_ptr(), dG.data_ptr(), zero.data_ptr(),
                                            zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), gpos.data_ptr(), gk.data_ptr(), 1))
        torch.cuda.synchronize()
        assert bool((oc == 0).all()) and bool((os_ == 0).all()) and bool((gk == 0).all())
        assert bool(torch.isnan(gpos).all())
