"""The dipole kernels of csrc/dipole.hip point by point, through the C entry points (ctypes, no probe library).

Real space -- ``mipme_dipole_rspace_forward`` / ``_backward`` on P isolated pairs (atoms 2p, 2p+1; N = 2P), so that every output
element is one term and the order of the atomics does not matter.  With a = g_i, b = mu_j and the partner's terms switched off
(mu_i = 0 and g_j = 0 on a half list, or ``full = 1``, where they are set and must not be read):

    out_i    = 1/2 pref (B b - C (b.r) r)
    grad_vec = 1/2 pref [ (dB (a.b) - dC (a.r)(b.r)) r - C ((b.r) a + (a.r) b) ]           dB = B'/r, dC = C'/r

    r = (s, s, 0), b = (0, 1, 1):        out_i,z = 1/2 pref B,   out_i,x = -1/2 pref C s^2
    r = (s, s, 0), a = b = e_z:          grad_vec = 1/2 pref dB r
    r = (s, s, s), a = e_x, b = e_y:     grad_vec,z = -1/2 pref dC s^3

against the mpmath values of ``tests/golden/dipole_pointwise.npz`` (taken at r^2 = 2 s^2, 3 s^2 exactly) -- and, away from the
golden points (random directions, stars, the grid-stride case), against ``radial_closed_form`` of
``tests/test_dipole_pointwise_host.py``, which the host test holds to 1e-13 of the goldens.

Bounds: the project's pointwise ones, ``bound`` of tests/test_gpu_sr_pointwise.py (x = alpha r^2 = y^2):

    modes 0 and 1, relative to |value|    float32 3e-6 + 2^-23 x (2e-5 + 2^-23 x beyond y = 6.5)      float64 2e-14 + 2^-51 x
    mode 2                                float32 3e-6                                                 float64 1e-12
        relative to what the switch multiplies: |B_lr| for B, |C_lr| for C, |dB_lr| + |B_lr| n pi / (2 r_x r) for dB (the second
        term inside r_x only), likewise dC: f_c = 1 - h^n is a difference of O(1) terms in any precision.

In mode 1 each of B, C, dB, dC is a sum of same-signed terms, so |value| is the size of the terms as well.  Underflow: the rule of
``check`` there (reference element below 2^-120 / 2^-1016: 0 <= |got| <= 2 |ref| + 2^-126 / 2^-1022), and the number of points in
that class must be the one the golden file records.  No point is dropped.  Vector outputs with several terms (random directions,
stars) are measured against the sum of the absolute values of their terms, each with its own radial scale.

Mode 2 from r_x on: exactly zero.  r is not an input here -- the kernel forms it from r^2 with three roundings -- so "from r_x on"
is asserted for r >= r_x (1 + 4 eps); the two points of each grid that sit within one float32 step of r_x fall under the general
bound instead, which at f_c <= 1e-13 they can only meet with an output that is all but zero.

Reciprocal space -- ``mipme_dipole_structure`` / ``_field`` / ``_backward`` against numpy float64 sums of the same inputs, at the
edges of their tiling (see ``test_reciprocal_edges``).
"""

import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests.test_dipole_pointwise_host import case_parameters, long_range, radial_closed_form
from tests.test_gpu_sr_pointwise import bound
from torchpme_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.float64]
ITYPES = [torch.int32, torch.int64]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "dipole_pointwise.npz"))


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _np(t):
    return t.double().cpu().numpy()


def _eps(dtype):
    return 2.0**-24 if dtype == torch.float32 else 2.0**-53


def _desc(sigma=None, rx=None, degree=1, pref=1.0):
    return _lib.DipoleDesc(smearing=-1.0 if sigma is None else sigma, prefactor=pref,
                           exclusion_radius=-1.0 if rx is None else rx, exclusion_degree=degree)


def rspace_forward(dtype, pairs, vec, mu, pot, full, n_atoms):
    out = torch.full((n_atoms, 3), float("nan"), dtype=dtype, device=DEV)
    _lib.check(_lib.load().mipme_dipole_rspace_forward(
        _lib.current_stream(DEV), _lib.dtype_code(dtype), _lib.index_code(pairs.dtype), n_atoms, pairs.shape[0], int(full),
        pairs.data_ptr(), vec.data_ptr(), mu.data_ptr(), C.byref(pot), out.data_ptr()))
    return out


def rspace_backward(dtype, pairs, vec, mu, grad_out, pot, full, n_atoms):
    gmu = torch.full((n_atoms, 3), float("nan"), dtype=dtype, device=DEV)
    gvec = torch.full_like(vec, float("nan"))
    _lib.check(_lib.load().mipme_dipole_rspace_backward(
        _lib.current_stream(DEV), _lib.dtype_code(dtype), _lib.index_code(pairs.dtype), n_atoms, pairs.shape[0], int(full),
        pairs.data_ptr(), vec.data_ptr(), mu.data_ptr(), grad_out.data_ptr(), C.byref(pot), gmu.data_ptr(), gvec.data_ptr()))
    return gmu, gvec


def check(what, dtype, got, ref, scale, tol):
    """|got - ref| <= tol * scale, or the underflow rule where scale is below the format's range (``check`` of
    test_gpu_sr_pointwise.py); prints the maxima; returns (max rel err, number of points in the underflow class)."""
    got, ref, scale = (np.asarray(a, np.float64) for a in (got, ref, scale))
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    tiny, floor = (2.0**-120, 2.0**-126) if dtype == torch.float32 else (2.0**-1016, 2.0**-1022)
    assert np.all(np.isfinite(got)), (what, np.flatnonzero(~np.isfinite(got))[:8])
    under = scale < tiny
    err = np.abs(got - ref)[~under] / scale[~under]
    worst = float((err / tol[~under]).max()) if err.size else 0.0
    print(f"[dipole-pointwise] {what:<52s} {str(dtype)[6:]:8s} max rel err {err.max() if err.size else 0.0:.3e}  "
          f"max err/bound {worst:.3f}  ({int(under.sum())} of {ref.size} in the underflow class)")
    bad = np.flatnonzero(~under)[err > tol[~under]]
    assert bad.size == 0, (what, dtype, bad[:8], got[bad[:8]], ref[bad[:8]], (err / tol[~under]).max())
    bad = np.flatnonzero(under & ~(np.abs(got) <= 2.0 * scale + floor))
    assert bad.size == 0, (what, dtype, "underflow class", bad[:8], got[bad[:8]], ref[bad[:8]])
    return (float(err.max()) if err.size else 0.0), int(under.sum())


class Checks:
    """``check`` for several quantities of one case: every one is measured and printed before the first failure is raised."""

    def __init__(self):
        self.failures = []

    def __call__(self, *args):
        try:
            return check(*args)
        except AssertionError as e:
            self.failures.append(e)
            return float("nan"), -1

    def done(self):
        assert not self.failures, self.failures


# ---- real space: the golden points --------------------------------------------------------------------------------------------
def _isolated_pairs(n, itype):
    return torch.arange(2 * n, device=DEV, dtype=itype).reshape(n, 2).contiguous()


def _atoms(n, dtype, at_i, at_j):
    a = np.empty((2 * n, 3))
    a[0::2], a[1::2] = at_i, at_j
    return _t(a, dtype)


def _pointwise_params():
    out = []
    for mode in (0, 1, 2):
        for si in (0, 1, 2):
            degrees = (1, 2, 4) if mode == 2 else (0,)
            combos = [(it, full) for it in ITYPES for full in (0, 1)] if si == 1 else [(torch.int64, 0)]
            for n in degrees:
                for it, full in combos:
                    out.append((f"m{mode}_s{si}", n, it, full))
    out += [("m2_wide", n, torch.int64, 0) for n in (1, 2, 4)]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case,degree,itype,full", _pointwise_params(),
                         ids=[f"{c}-n{n}-{str(it)[6:]}-full{f}" for c, n, it, f in _pointwise_params()])
def test_radial_pointwise(g, case, degree, itype, full, dtype):
    mode, sigma, rx = case_parameters(g, case)
    pot = _desc(None if mode == 0 else sigma, rx, max(degree, 1))
    s2, s3 = g[case + "_g2_s"].astype(np.float64), g[case + "_g3_s"].astype(np.float64)
    root = sigma * math.sqrt(2.0)
    y2, y3 = s2 * math.sqrt(2.0) / root, s3 * math.sqrt(3.0) / root
    if mode == 1 and dtype == torch.float32:  # y in [1e-3, 9] in float32, [1e-3, 26] in float64
        s2, y2, keep2 = s2[y2 <= 9.0], y2[y2 <= 9.0], y2 <= 9.0
        s3, y3, keep3 = s3[y3 <= 9.0], y3[y3 <= 9.0], y3 <= 9.0
    else:
        keep2, keep3 = np.ones(len(s2), bool), np.ones(len(s3), bool)
    n2, n3 = len(s2), len(s3)
    r_2, r_3 = s2 * math.sqrt(2.0), s3 * math.sqrt(3.0)
    # the partner's dipole and gradient: zero on the half list; with full = 1 set, and not read by out and grad_vectors
    other = (0.3, -0.7, 1.1) if full else (0.0, 0.0, 0.0)
    zero2, zero3 = np.zeros(n2), np.zeros(n3)

    # B and C: r = (s, s, 0), b = (0, 1, 1)
    vec2 = _t(np.stack([s2, s2, zero2], 1), dtype)
    pairs2 = _isolated_pairs(n2, itype)
    out = _np(rspace_forward(dtype, pairs2, vec2, _atoms(n2, dtype, other, (0.0, 1.0, 1.0)), pot, full, 2 * n2))
    # dB: a = b = e_z
    mu = _atoms(n2, dtype, other, (0.0, 0.0, 1.0))
    gout = _atoms(n2, dtype, (0.0, 0.0, 1.0), other)
    gmu2, gvec2 = rspace_backward(dtype, pairs2, vec2, mu, gout, pot, full, 2 * n2)
    gmu2, gvec2 = _np(gmu2), _np(gvec2)
    # dC: r = (s, s, s), a = e_x, b = e_y
    vec3 = _t(np.stack([s3, s3, s3], 1), dtype)
    pairs3 = _isolated_pairs(n3, itype)
    _, gvec3 = rspace_backward(dtype, pairs3, vec3, _atoms(n3, dtype, other, (0.0, 1.0, 0.0)),
                               _atoms(n3, dtype, (1.0, 0.0, 0.0), other), pot, full, 2 * n3)
    gvec3 = _np(gvec3)
    torch.cuda.synchronize()

    if mode < 2:
        B, Cc, dB, dC = (g[f"{case}_{k}"][kp] for k, kp in (("B", keep2), ("C", keep2), ("dB", keep2), ("dC", keep3)))
        sB, sC, sdB, sdC = np.abs(B), np.abs(Cc), np.abs(dB), np.abs(dC)
        x2, x3 = (y2 * y2, y3 * y3) if mode == 1 else (zero2, zero3)
        tol2, tol3 = bound(dtype, x2, np.sqrt(x2)), bound(dtype, x3, np.sqrt(x3))
    else:
        k = f"{case}_n{degree}"
        B, Cc, dB, dC = g[k + "_B"], g[k + "_C"], g[k + "_dB"], g[k + "_dC"]
        w2 = np.where(r_2 < rx, degree * np.pi / (2 * rx * r_2), 0.0)
        w3 = np.where(r_3 < rx, degree * np.pi / (2 * rx * r_3), 0.0)
        sB, sC = g[case + "_Blr"], g[case + "_Clr"]
        sdB, sdC = np.abs(g[case + "_dBlr"]) + sB * w2, np.abs(g[case + "_dClr"]) + g[case + "_Clr3"] * w3
        tol2, tol3 = bound(dtype, zero2, zero2, switched=True), bound(dtype, zero3, zero3, switched=True)
    name = f"{case} n={degree} {str(itype)[6:]} full={full}"
    checks = Checks()
    counts = [
        checks(f"{name} B", dtype, out[0::2, 2], 0.5 * B, 0.5 * sB, tol2)[1],
        checks(f"{name} C", dtype, out[0::2, 0], -0.5 * Cc * s2**2, 0.5 * sC * s2**2, tol2)[1],
        checks(f"{name} dB", dtype, gvec2[:, 0], 0.5 * dB * s2, 0.5 * sdB * s2, tol2)[1],
        checks(f"{name} dC", dtype, gvec3[:, 2], -0.5 * dC * s3**3, 0.5 * sdC * s3**3, tol3)[1],
    ]
    checks.done()
    want = g[case + ("_under32" if dtype == torch.float32 else "_under64")]
    assert counts == [int(c) for c in want], (counts, want)
    # the other components: out_y = out_z + out_x up to one rounding of the sum; grad_vec y = x; the rest is exactly zero
    check(f"{name} B + C (out_y)", dtype, out[0::2, 1], 0.5 * B - 0.5 * Cc * s2**2, 0.5 * sB + 0.5 * sC * s2**2, tol2)
    assert np.array_equal(gvec2[:, 1], gvec2[:, 0]) and np.all(gvec2[:, 2] == 0.0)
    # grad_dipoles of the run for dB is the forward sum applied to g: 1/2 B e_z at atom j (half list), nothing at i from mu_i = 0
    if not full:
        check(f"{name} grad_dipoles (B)", dtype, gmu2[1::2, 2], 0.5 * B, 0.5 * sB, tol2)
        assert np.all(out[1::2] == 0.0) and np.all(gmu2[0::2] == 0.0)
    else:  # full = 1 writes row i only: out_i from mu_j (mu_i is not read), grad_dipoles_i from g_j = (0.3, -0.7, 1.1)
        assert np.all(out[1::2] == 0.0) and np.all(gmu2[1::2] == 0.0)
        check(f"{name} grad_dipoles (B)", dtype, gmu2[0::2, 2], 0.5 * B * 1.1, 0.5 * sB * 1.1, tol2)
    if mode == 2:
        eps4 = 1.0 + 4 * (2.0**-23 if dtype == torch.float32 else 2.0**-52)
        beyond2, beyond3 = r_2 >= rx * eps4, r_3 >= rx * eps4
        assert beyond2.sum() >= 3 and beyond3.sum() >= 3
        assert np.all(out[0::2][beyond2] == 0.0) and np.all(gvec2[beyond2] == 0.0) and np.all(gvec3[beyond3] == 0.0)


# ---- real space: whole vectors --------------------------------------------------------------------------------------------------
def radial_with_scales(mode, sigma, rx, degree, r2, dtype):
    """(B, C, dB, dC), their error scales and the pointwise tolerance at r^2 = r2 (see the module docstring)."""
    r2 = np.asarray(r2, np.float64)
    val = radial_closed_form(mode, sigma, r2, rx, degree)
    if mode < 2:
        x = r2 * (0.5 / sigma**2 if mode == 1 else 0.0)
        return val, tuple(np.abs(v) for v in val), bound(dtype, x, np.sqrt(x))
    Bl, Cl, dBl, dCl = long_range(sigma, r2)
    r = np.sqrt(r2)
    w = np.where(r < rx, degree * np.pi / (2 * rx * r), 0.0)
    return val, (Bl, Cl, np.abs(dBl) + Bl * w, np.abs(dCl) + Cl * w), bound(dtype, 0 * r2, 0 * r2, switched=True)


def tensor_apply(val, sc, r, b):
    """T b = B b - C (b.r) r per pair, and the sum of the absolute values of its terms with the radial scales."""
    B, Cc, Bs, Cs = val[0], val[1], sc[0], sc[1]
    br, br_abs = (b * r).sum(1), (np.abs(b) * np.abs(r)).sum(1)
    return B[:, None] * b - (Cc * br)[:, None] * r, Bs[:, None] * np.abs(b) + (Cs * br_abs)[:, None] * np.abs(r)


def tensor_grad(val, sc, r, a, b):
    """d(a^T T b)/dr per pair and the sum of the absolute values of its terms."""
    (_, Cc, dB, dC), (_, Cs, dBs, dCs) = val, sc
    ar, br, ab = (a * r).sum(1), (b * r).sum(1), (a * b).sum(1)
    ar_, br_, ab_ = (np.abs(a) * np.abs(r)).sum(1), (np.abs(b) * np.abs(r)).sum(1), (np.abs(a) * np.abs(b)).sum(1)
    value = (dB * ab - dC * ar * br)[:, None] * r - Cc[:, None] * (br[:, None] * a + ar[:, None] * b)
    scale = (dBs * ab_ + dCs * ar_ * br_)[:, None] * np.abs(r) + Cs[:, None] * (br_[:, None] * np.abs(a) + ar_[:, None] * np.abs(b))
    return value, scale


def half_list_reference(mode, sigma, rx, degree, pref, dtype, vec, mu, gout):
    """Isolated pairs (2p, 2p+1) on a half list with everything set: out, grad_dipoles (N, 3) and grad_vectors (P, 3), each with
    its scale, and the tolerance per pair.  vec, mu, gout: the float64 images of what the kernel receives."""
    val, sc, tol = radial_with_scales(mode, sigma, rx, degree, (vec * vec).sum(1), dtype)
    h = 0.5 * pref
    res = {}
    for key, w in (("out", mu), ("grad_dipoles", gout)):
        v = np.empty_like(w)
        s = np.empty_like(w)
        v[0::2], s[0::2] = tensor_apply(val, sc, vec, w[1::2])
        v[1::2], s[1::2] = tensor_apply(val, sc, vec, w[0::2])
        res[key] = (h * v, abs(h) * s)
    v1, s1 = tensor_grad(val, sc, vec, gout[0::2], mu[1::2])
    v2, s2 = tensor_grad(val, sc, vec, gout[1::2], mu[0::2])
    res["grad_vectors"] = (h * (v1 + v2), abs(h) * (s1 + s2))
    return res, tol


def _random_directions(rng, n, r_lo, r_hi):
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u * rng.uniform(r_lo, r_hi, n)[:, None]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_general_directions(mode, dtype):
    """200 random directions, a, b, mu_i, g_j all set, half list, prefactor 1.7: the whole 3-vectors against the closed form."""
    rng = np.random.default_rng(100 + mode)
    n, sigma, degree, pref = 200, 1.0, 2, 1.7
    rx = 2.5 if mode == 2 else None
    vec = _t(_random_directions(rng, n, 0.07, 3.2), dtype)
    mu, gout = _t(rng.normal(size=(2 * n, 3)), dtype), _t(rng.normal(size=(2 * n, 3)), dtype)
    pot = _desc(None if mode == 0 else sigma, rx, degree, pref)
    pairs = _isolated_pairs(n, torch.int64)
    out = rspace_forward(dtype, pairs, vec, mu, pot, 0, 2 * n)
    gmu, gvec = rspace_backward(dtype, pairs, vec, mu, gout, pot, 0, 2 * n)
    torch.cuda.synchronize()
    ref, tol = half_list_reference(mode, sigma, rx, degree, pref, dtype, _np(vec), _np(mu), _np(gout))
    tol_atoms, tol_pairs = np.repeat(np.repeat(tol, 2), 3), np.repeat(tol, 3)
    for key, got, t in (("out", out, tol_atoms), ("grad_dipoles", gmu, tol_atoms), ("grad_vectors", gvec, tol_pairs)):
        check(f"random directions mode {mode} {key}", dtype, _np(got).ravel(), ref[key][0].ravel(), ref[key][1].ravel(), t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 1000])
def test_stars(L, mode, dtype):
    """One centre with L partners as a full list (both directions of every pair, full = 1): the centre's out and grad_dipoles are
    sums of L terms through the atomics.  Bound per component: sum_j tol_j |term_j| + (L + 2) eps sum_j |term_j| -- the pointwise
    bound of every term plus the L - 1 roundings of the sum in any order (and three spare)."""
    rng = np.random.default_rng(7 * L + mode)
    sigma, degree, pref = 1.0, 2, 1.0
    rx = 2.5 if mode == 2 else None
    off = _random_directions(rng, L, 0.3, 2.4 if mode == 2 else 3.5)
    tvec = _t(np.concatenate([off, -off]), dtype)
    idx = np.arange(1, L + 1)
    pairs = torch.tensor(np.concatenate([np.stack([0 * idx, idx], 1), np.stack([idx, 0 * idx], 1)]), device=DEV)
    mu, gout = _t(rng.normal(size=(L + 1, 3)), dtype), _t(rng.normal(size=(L + 1, 3)), dtype)
    pot = _desc(sigma, rx, degree, pref)
    out = rspace_forward(dtype, pairs, tvec, mu, pot, 1, L + 1)
    gmu, gvec = rspace_backward(dtype, pairs, tvec, mu, gout, pot, 1, L + 1)
    torch.cuda.synchronize()
    vec, m, go = _np(tvec)[:L], _np(mu), _np(gout)
    val, sc, tol = radial_with_scales(mode, sigma, rx, degree, (vec * vec).sum(1), dtype)
    extra = (L + 2) * _eps(dtype)
    for key, got, w in (("out", out, m), ("grad_dipoles", gmu, go)):
        got = _np(got)
        v, s = tensor_apply(val, sc, vec, w[1:])  # the centre's terms
        ref_c, scale_c, bound_c = 0.5 * v.sum(0), 0.5 * s.sum(0), 0.5 * ((tol[:, None] + extra) * s).sum(0)
        check(f"star L={L} mode {mode} centre {key}", dtype, got[0], ref_c, scale_c, bound_c / scale_c)
        v, s = tensor_apply(val, sc, vec, np.broadcast_to(w[0], (L, 3)))  # the partners: one term each (T is even in r)
        check(f"star L={L} mode {mode} partners {key}", dtype, got[1:].ravel(), 0.5 * v.ravel(), 0.5 * s.ravel(), np.repeat(tol, 3))
    # grad_vectors: entry (0, j) holds d(g_0^T T mu_j)/dr, entry (j, 0) d(g_j^T T mu_0)/dr at -r
    v1, s1 = tensor_grad(val, sc, vec, np.broadcast_to(go[0], (L, 3)), m[1:])
    v2, s2 = tensor_grad(val, sc, -vec, go[1:], np.broadcast_to(m[0], (L, 3)))
    ref, scale = 0.5 * np.concatenate([v1, v2]), 0.5 * np.concatenate([s1, s2])
    check(f"star L={L} mode {mode} grad_vectors", dtype, _np(gvec).ravel(), ref.ravel(), scale.ravel(), np.repeat(np.tile(tol, 2), 3))


def test_grid_stride():
    """P = 2^20 + 257 isolated pairs: the pair kernels launch 4096 blocks of 256 threads at most, so this is the smallest list at
    which a thread takes a second pair -- the last 257 pairs sit in the second trip of the loop and are checked on their own.
    Mode 1, sigma = 1, r in [0.8, 4] in random directions, float32 with int32 indices, forward and backward."""
    dtype, mode, sigma, pref = torch.float32, 1, 1.0, 1.0
    n = (1 << 20) + 257
    rng = np.random.default_rng(20)
    vec = torch.tensor(_random_directions(rng, n, 0.8, 4.0), dtype=dtype).to(DEV)
    mu = torch.tensor(rng.standard_normal((2 * n, 3), dtype=np.float32)).to(DEV)
    gout = torch.tensor(rng.standard_normal((2 * n, 3), dtype=np.float32)).to(DEV)
    pairs = _isolated_pairs(n, torch.int32)
    pot = _desc(sigma, None, 1, pref)
    out = rspace_forward(dtype, pairs, vec, mu, pot, 0, 2 * n)
    gmu, gvec = rspace_backward(dtype, pairs, vec, mu, gout, pot, 0, 2 * n)
    torch.cuda.synchronize()
    ref, tol = half_list_reference(mode, sigma, None, 1, pref, dtype, _np(vec), _np(mu), _np(gout))
    tol_atoms, tol_pairs = np.repeat(np.repeat(tol, 2), 3), np.repeat(tol, 3)
    for key, got, t, tail in (("out", out, tol_atoms, 6 * 257), ("grad_dipoles", gmu, tol_atoms, 6 * 257),
                              ("grad_vectors", gvec, tol_pairs, 3 * 257)):
        got, (r, s) = _np(got).ravel(), (a.ravel() for a in ref[key])
        check(f"grid stride {key}: all {n} pairs", dtype, got, r, s, t)
        check(f"grid stride {key}: the last 257 pairs", dtype, got[-tail:], r[-tail:], s[-tail:], t[-tail:])
        assert np.all(got[-tail:] != 0.0)


# ---- reciprocal space -----------------------------------------------------------------------------------------------------------
def _first_sliced_k():
    """The smallest K at which the per-atom kernels of one atom split K into slices (bisection on the library's own answer)."""
    size = _lib.load().mipme_dipole_partials_size
    lo, hi = 1, 2
    while size(1, hi) == 0:
        lo, hi = hi, 2 * hi
        assert hi < 1 << 30
    while hi - lo > 1:  # size(lo) == 0 < size(hi)
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if size(1, mid) > 0 else (mid, hi)
    return hi


def _filters(rng, K, pattern):
    """G and dG: 0 all non-zero; 1 a whole aligned block of 8 zeros (the first, and the ragged last one beyond K = 16);
    2 an aligned block with exactly one live entry; 3 entries with G = 0 and dG != 0."""
    G, dG = rng.uniform(0.1, 1.0, K), rng.uniform(-1.0, -0.1, K)
    if pattern == 1:
        G[:8] = dG[:8] = 0.0
        if K > 16:
            G[8 * ((K - 1) // 8):] = dG[8 * ((K - 1) // 8):] = 0.0
    elif pattern == 2:
        keep = min(5, K - 1)
        G[:keep] = dG[:keep] = 0.0
        G[keep + 1:8] = dG[keep + 1:8] = 0.0
    elif pattern == 3:
        G[rng.uniform(size=K) < 0.4] = 0.0
        G[0] = 0.0
    return G, dG


_RECIP_K = [1, 7, 9, 1023, "first sliced", "first sliced + 1"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K", _RECIP_K)
@pytest.mark.parametrize("N", [1, 31, 33, 255, 257])
def test_reciprocal_edges(N, K, dtype):
    """Structure factors, field, dL/dr and dL/dk from the C entry points against numpy float64 sums of the same (rounded) inputs:
    positions in a box of edge 8, |k| <= 6; N one off the 32 atom lanes and the 256-atom LDS tile; K one off the 8 k-vectors of a
    block, and the smallest K that the per-atom kernels slice (two slices, the last one ragged) and one more; four patterns of
    G / dG (``_filters``).  A k-vector with G = dG = 0 is pruned: its structure factors and gradient are exact zeros.

    Bound per output element: (d + 8 + 4 phi_max) eps S_abs, eps = 2^-24 / 2^-53, with
      S_abs    the same sum with every product term replaced by its absolute value, in float64;
      phi_max  max |k.r| over the case: the phase k.r is a dot product of three, in error by up to 3 eps sum_c |k_c r_c|, and
               sincos reduces an argument of that size; cos and sin move by as much as the phase does, so 4 phi_max eps per term
               (phi_max stands for sum_c |k_c r_c| <= |k| |r|; where a case has few (k, atom) pairs the 8 carries the rest);
      d        the depth of the kernel's own summation: 32-lane kernels add ceil(N/32) terms per lane, then 5 shuffle steps;
               per-atom kernels add ceil(chunk/256) terms per thread, then 6 shuffle steps, 3 additions of the wave sums (8 with
               one spare) and the slices in order;
      8        the roundings inside one term (dot products of three, the products with G, S and k) and of sincos itself.

    One-term sums (N = 1; the field at K = 1 has two) are where this bound asks most: an error dphi of the phase moves
    q cos(phi) by |q sin(phi)| dphi, which is set against S_abs = |q cos(phi)|, so next to a zero of cos or sin the phase has to be
    good to a few eps of its distance from that zero.  With the phase formed in float32 (absolute error |k.r| 2^-24) the N = 1
    structure factors missed the bound by up to 483 times (K = 2048; 325 at K = 1023, 267 at K = 2049, 1.3 at K = 9) and the
    field at N = 255, K = 1 by 1.33; the float32 kernels now form and reduce the phase in double (``dipole_phase3``): 0.05 of
    the bound at most, over all cases.  In
    float64 the numpy reference rounds the phase the way the kernel does, which is all that keeps its one-term cases inside."""
    lib, checks = _lib.load(), Checks()
    if isinstance(K, str):
        K = _first_sliced_k() + (1 if K.endswith("1") else 0)
        assert lib.mipme_dipole_partials_size(1, K) == 2 * 3 and lib.mipme_dipole_partials_size(1, K - 1 - (K % 2)) == 0
    rng = np.random.default_rng(1000 * N + K)
    eps, dt, st = _eps(dtype), _lib.dtype_code(dtype), _lib.current_stream(DEV)
    tpos, tmu, tg = _t(rng.uniform(0, 8, (N, 3)), dtype), _t(rng.normal(size=(N, 3)), dtype), _t(rng.normal(size=(N, 3)), dtype)
    kdir = rng.normal(size=(K, 3))
    tk = _t(kdir / np.linalg.norm(kdir, axis=1)[:, None] * rng.uniform(0.3, 6.0, (K, 1)), dtype)
    pos, mu, gr, kv = _np(tpos), _np(tmu), _np(tg), _np(tk)
    phase = kv @ pos.T  # (K, N)
    c, s = np.cos(phase), np.sin(phase)
    phi = 4 * np.abs(phase).max()
    n_part = lib.mipme_dipole_partials_size(N, K)
    slices = max(1, n_part // (3 * N))
    chunk = -(-K // slices)
    d_lane, d_atom = -(-N // 32) + 5, -(-chunk // 256) + 8 + slices
    partials = torch.empty(max(1, n_part), dtype=dtype, device=DEV)
    absk = np.abs(kv)

    def structure(w):
        q, q_abs = kv @ w.T, absk @ np.abs(w).T
        return (q * c).sum(1), (q * s).sum(1), (q_abs * np.abs(c)).sum(1), (q_abs * np.abs(s)).sum(1)

    for pattern in range(4):
        G64, dG64 = _filters(rng, K, pattern)
        tG, tdG = _t(G64, dtype), _t(dG64, dtype)
        G, dG = _np(tG), _np(tdG)
        live = (G != 0) | (dG != 0)
        assert pattern != 3 or ((G == 0) & live).any()
        what = f"N={N} K={K} pattern {pattern}"
        # structure factors (of the dipoles, and of g for the backward pass)
        S = {}
        for name, tw, w in (("S", tmu, mu), ("T", tg, gr)):
            oc, os_ = (torch.full((K,), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
            _lib.check(lib.mipme_dipole_structure(st, dt, N, K, tpos.data_ptr(), tw.data_ptr(), tk.data_ptr(), tG.data_ptr(),
                                                  tdG.data_ptr(), oc.data_ptr(), os_.data_ptr()))
            rc, rs, ac, as_ = structure(w)
            tol = (d_lane + 8 + phi) * eps
            checks(f"{what} structure {name} cos", dtype, _np(oc)[live], rc[live], ac[live], tol)
            checks(f"{what} structure {name} sin", dtype, _np(os_)[live], rs[live], as_[live], tol)
            assert np.all(_np(oc)[~live] == 0.0) and np.all(_np(os_)[~live] == 0.0)
            S[name] = (_t(np.where(live, rc, 0.0), dtype), _t(np.where(live, rs, 0.0), dtype))
        (tSc, tSs), (tTc, tTs) = S["S"], S["T"]
        Sc, Ss, Tc, Ts = _np(tSc), _np(tSs), _np(tTc), _np(tTs)
        # field: E_i = sum_k G k [cos S_c + sin S_s]
        out = torch.full((N, 3), float("nan"), dtype=dtype, device=DEV)
        _lib.check(lib.mipme_dipole_field(st, dt, N, K, tpos.data_ptr(), tk.data_ptr(), tG.data_ptr(), tSc.data_ptr(), tSs.data_ptr(),
                                          out.data_ptr(), partials.data_ptr()))
        b = G[:, None] * (c * Sc[:, None] + s * Ss[:, None])
        b_abs = np.abs(G)[:, None] * (np.abs(c * Sc[:, None]) + np.abs(s * Ss[:, None]))
        tol_atom = (d_atom + 8 + phi) * eps
        checks(f"{what} field", dtype, _np(out).ravel(), (b.T @ kv).ravel(), (b_abs.T @ absk).ravel() + 1e-300, tol_atom)
        # backward
        gpos = torch.full((N, 3), float("nan"), dtype=dtype, device=DEV)
        gk = torch.full((K, 3), float("nan"), dtype=dtype, device=DEV)
        _lib.check(lib.mipme_dipole_backward(st, dt, N, K, tpos.data_ptr(), tmu.data_ptr(), tg.data_ptr(), tk.data_ptr(), tG.data_ptr(),
                                             tdG.data_ptr(), tSc.data_ptr(), tSs.data_ptr(), tTc.data_ptr(), tTs.data_ptr(),
                                             gpos.data_ptr(), gk.data_ptr(), partials.data_ptr()))
        torch.cuda.synchronize()
        gdk, mdk = kv @ gr.T, kv @ mu.T  # (K, N): g_i.k, mu_i.k
        gdk_abs, mdk_abs = absk @ np.abs(gr).T, absk @ np.abs(mu).T
        u1, u2 = c * Ss[:, None] - s * Sc[:, None], c * Ts[:, None] - s * Tc[:, None]
        u1_abs = np.abs(c * Ss[:, None]) + np.abs(s * Sc[:, None])
        u2_abs = np.abs(c * Ts[:, None]) + np.abs(s * Tc[:, None])
        b = gdk * u1 + mdk * u2
        b_abs = gdk_abs * u1_abs + mdk_abs * u2_abs
        ref = (G[:, None] * b).T @ kv
        ref_abs = (np.abs(G)[:, None] * b_abs).T @ absk
        checks(f"{what} grad positions", dtype, _np(gpos).ravel(), ref.ravel(), ref_abs.ravel() + 1e-300, tol_atom)
        a1, a2 = c * Sc[:, None] + s * Ss[:, None], c * Tc[:, None] + s * Ts[:, None]
        a1_abs = np.abs(c * Sc[:, None]) + np.abs(s * Ss[:, None])
        a2_abs = np.abs(c * Tc[:, None]) + np.abs(s * Ts[:, None])
        ref = G[:, None] * (a1 @ gr + a2 @ mu + b @ pos) + (2 * dG * (Tc * Sc + Ts * Ss))[:, None] * kv
        ref_abs = np.abs(G)[:, None] * (a1_abs @ np.abs(gr) + a2_abs @ np.abs(mu) + b_abs @ np.abs(pos)) \
            + (2 * np.abs(dG) * (np.abs(Tc * Sc) + np.abs(Ts * Ss)))[:, None] * absk
        got = _np(gk)
        checks(f"{what} grad kvectors", dtype, got[live].ravel(), ref[live].ravel(), ref_abs[live].ravel(), (d_lane + 8 + phi) * eps)
        assert np.all(got[~live] == 0.0)
        if pattern == 3:  # G = 0, dG != 0 stays live: the k-gradient there is the dG term alone, and it is not zero
            only = (G == 0) & live
            assert np.all(np.abs(got[only]).sum(1) > 0)
    checks.done()
