"""The short-range pair functions and the row bodies that evaluate them, point by point against mpmath
(``tests/golden/sr_pointwise.npz``, written by ``tests/golden/make_sr_pointwise_golden.py``).

(a) Every variant of v_SR(d) and of the pieces it is made of runs as a kernel of its own, one input per thread, in the test-only
    probe ``tests/probe/sr_probe.hip`` (built by ``make -C torch-pme_amd/csrc probe``), which includes ``rows_body.h`` as it stands.
(b) A system of "stars" -- a centre and L partners that neighbour only the centre -- runs through ``mipme_sr_rows_fused`` with
    every entry format and through the probe's wrappers of the fp64 table body and the packed fp32 body; every row sum has one
    non-zero term, so potentials and force sums are pointwise too.
(c) The same system through the co-scheduled launch and the frames launch, against the separate launches.

Bounds (relative error; x = d^2 / 2 sigma^2, y = sqrt x; classes by x and y alone, no point is dropped):

    y <= 6.5, modes 0 and 1    float32 3e-6 + 2^-23 x      float64 2e-14 + 2^-51 x
    y <= 6.5, modes 2 and 3    float32 3e-6                float64 1e-12
    y >  6.5                   float32 2e-5 + 2^-23 x      float64 as for y <= 6.5

3e-6 / 1e-12 are the project's pointwise tolerances (test_exclusion_small_distances_fp32); the x term is the rounding of the
exponential's argument (a relative rounding of x moves exp(-x) by x eps; two of them); 2e-14 is three times the budgets of the
pieces of the fp64 body (table 2.22e-15, exp 4e-16, one-step rsq 2.4e-15, eight roundings); 2e-5 is what srpot.h documents for
the fp32 erfc polynomial beyond y = 6.5 -- the erfc part only, so the x term stays.
Potentials are measured relative to |v|.  In modes 2 and 3 the switch f_cut = 1 - base^n is a difference of O(1) terms whatever
the precision (at d = rx - 1 ulp it is 1e-14 in exact arithmetic), so the error is measured relative to what it multiplies:
|v_LR| (mode 2) or the bare |v| (mode 3).  Derivatives are measured relative to |v'| + p |v| / d, the size of the terms they are
a difference of, with |v_LR| / bare |v| for |v| in modes 2 / 3 and there, inside rx, the term of the switch's own derivative,
|v| n pi / (2 rx), added.
Underflow: where the reference is below 2^-120 (float32) or 2^-1016 (float64; the same six binades above the smallest normal
number) the assertion is 0 <= |got| <= 2 |ref| + 2^-126 (2^-1022) instead.
The stand-alone pieces take the figures of their own comments in srpot.h: exp_neg_table2 4e-16 and exp_neg_fast ("the 13-term
form") 3e-16, rcp_newton / rsqrt_newton "an ulp or two" = 2 x 2^-52; lower_gamma_series, which exists for mode 2, its tolerances.
"""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import torchpme_amd as tpa
from torchpme_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe", "_sr_probe.so")
DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.float64]
SQRT2 = np.sqrt(2.0)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "sr_pointwise.npz"))


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "torch-pme_amd", "csrc"), "probe"], check=True)
    lib = C.CDLL(PROBE)
    vp, i64, ci, PP = C.c_void_p, C.c_int64, C.c_int, C.POINTER(_lib.PotentialDesc)
    lib.sr_probe_last_error.restype = C.c_char_p
    lib.sr_probe_sr_eval.argtypes = [vp, ci, PP, i64, vp, vp, vp]
    lib.sr_probe_fast_rs.argtypes = [vp, ci, PP, i64, vp, vp, vp]
    lib.sr_probe_fast_rs_pk.argtypes = [vp, PP, i64, ci, vp, vp, vp]
    lib.sr_probe_scalar_f64.argtypes = [vp, ci, i64, vp, vp]
    lib.sr_probe_lower_gamma.argtypes = [vp, ci, ci, i64, vp, vp]
    rows = [vp, ci, i64, vp, vp, vp, vp, vp, vp, PP, ci, vp, vp]
    lib.sr_probe_rows_f64.argtypes = rows
    lib.sr_probe_rows_pk.argtypes = rows
    return lib


def _ok(lib, rc):
    assert rc == 0, (rc, lib.sr_probe_last_error())


def _desc(p, sigma=None, rx=None, degree=1):
    return _lib.PotentialDesc(kind=_lib.COULOMB if p == 1 else _lib.INVERSE_POWER_LAW, exponent=p,
                              smearing=-1.0 if sigma is None else sigma, prefactor=1.0,
                              exclusion_radius=-1.0 if rx is None else rx, exclusion_degree=degree)


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _np(t):
    return t.double().cpu().numpy()


def _stream():
    return _lib.current_stream(DEV)


def bound(dtype, x, y, switched=False):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if dtype == torch.float32:
        return np.full_like(x, 3e-6) if switched else np.where(y <= 6.5, 3e-6, 2e-5) + 2.0**-23 * x
    return np.full_like(x, 1e-12) if switched else 2e-14 + 2.0**-51 * x


def check(what, dtype, got, ref, scale, tol):
    """|got - ref| <= tol * scale, or the underflow rule where scale is below the format's range; prints the maximum."""
    got, ref, scale = (np.asarray(a, np.float64) for a in (got, ref, scale))
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    tiny, floor = (2.0**-120, 2.0**-126) if dtype == torch.float32 else (2.0**-1016, 2.0**-1022)
    assert np.all(np.isfinite(got)), (what, np.flatnonzero(~np.isfinite(got))[:8])
    under = scale < tiny
    err = np.abs(got - ref)[~under] / scale[~under]
    worst = float((err / tol[~under]).max()) if err.size else 0.0
    print(f"[sr-pointwise] {what:<44s} {str(dtype)[6:]:8s} max rel err {err.max() if err.size else 0.0:.3e}  "
          f"max err/bound {worst:.3f}  ({int(under.sum())} of {ref.size} in the underflow class)")
    bad = np.flatnonzero(~under)[err > tol[~under]]
    assert bad.size == 0, (what, dtype, bad[:8], got[bad[:8]], ref[bad[:8]])
    bad = np.flatnonzero(under & ~(np.abs(got) <= 2.0 * scale + floor))
    assert bad.size == 0, (what, dtype, "underflow class", bad[:8], got[bad[:8]], ref[bad[:8]])
    return float(err.max()) if err.size else 0.0


# ---- (a) functions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("si", [0, 1, 2])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6])
def test_sr_eval_range_separated(probe, g, dtype, si, p):
    sigma = float(g["sigmas"][si])
    d64 = g[f"m1_d_s{si}"].astype(np.float64)
    d = _t(d64, dtype)
    v, dv = torch.empty_like(d), torch.empty_like(d)
    pot = _desc(p, sigma)
    _ok(probe, probe.sr_probe_sr_eval(_stream(), _lib.dtype_code(dtype), C.byref(pot), d.numel(), d.data_ptr(), v.data_ptr(), dv.data_ptr()))
    rv, rdv = g[f"m1_v_p{p}_s{si}"], g[f"m1_dv_p{p}_s{si}"]
    y = d64 / (sigma * SQRT2)
    tol = bound(dtype, y * y, y)
    check(f"sr_eval mode 1 p={p} sigma={sigma} v", dtype, _np(v), rv, np.abs(rv), tol)
    check(f"sr_eval mode 1 p={p} sigma={sigma} dv", dtype, _np(dv), rdv, np.abs(rdv) + p * np.abs(rv) / d64, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(28))
def test_sr_eval_bare_and_exclusion(probe, g, dtype, case):
    mode, p, n = (int(t) for t in g["ex_cases"][case])
    sigma, rx = float(g["ex_sigma"]), float(g["ex_rx"])
    d64 = g["ex_d"].astype(np.float64)
    d = _t(d64, dtype)
    v, dv = torch.empty_like(d), torch.empty_like(d)
    pot = _desc(p, sigma if mode == 2 else None, rx if mode >= 2 else None, n)
    _ok(probe, probe.sr_probe_sr_eval(_stream(), _lib.dtype_code(dtype), C.byref(pot), d.numel(), d.data_ptr(), v.data_ptr(), dv.data_ptr()))
    rv, rdv, big = g[f"ex_v_{case}"], g[f"ex_dv_{case}"], g[f"ex_big_{case}"]
    tol = bound(dtype, np.zeros_like(d64), np.zeros_like(d64), switched=mode >= 2)
    dscale = np.abs(rdv) + p * big / d64
    if mode >= 2:
        dscale = dscale + np.where(d64 < rx, big * n * np.pi / (2 * rx), 0.0)
    check(f"sr_eval mode {mode} p={p} degree={n} v", dtype, _np(v), rv, big, tol)
    check(f"sr_eval mode {mode} p={p} degree={n} dv", dtype, _np(dv), rdv, dscale, tol)
    if mode == 2:  # beyond the exclusion radius the pair contributes exactly nothing
        assert np.all(_np(v)[d64 >= rx] == 0.0) and np.all(_np(dv)[d64 >= rx] == 0.0)


def _fast_reference(g, si, p):
    sigma = float(g["sigmas"][si])
    d2 = g[f"m1_d2_s{si}"].astype(np.float64)
    d = np.sqrt(d2)
    rv, rdv = g[f"f1_v_p{p}_s{si}"], g[f"f1_dv_p{p}_s{si}"]
    x = d2 / (2 * sigma * sigma)
    return sigma, d2, d, rv, rdv, x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("si", [0, 1, 2])
@pytest.mark.parametrize("p", [1, 6])
def test_fast_rs_eval(probe, g, dtype, si, p):
    sigma, d2, d, rv, rdv, x = _fast_reference(g, si, p)
    t = _t(d2, dtype)
    v, dvd = torch.empty_like(t), torch.empty_like(t)
    pot = _desc(p, sigma)
    _ok(probe, probe.sr_probe_fast_rs(_stream(), _lib.dtype_code(dtype), C.byref(pot), t.numel(), t.data_ptr(), v.data_ptr(), dvd.data_ptr()))
    tol = bound(dtype, x, np.sqrt(x))
    check(f"fast_rs_eval<{p}> sigma={sigma} v", dtype, _np(v), rv, np.abs(rv), tol)
    check(f"fast_rs_eval<{p}> sigma={sigma} dv", dtype, _np(dvd) * d, rdv, np.abs(rdv) + p * np.abs(rv) / d, tol)


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("si", [0, 1, 2])
@pytest.mark.parametrize("p", [1, 6])
def test_fast_rs_eval_packed(probe, g, si, p, swap):
    """Two distances per thread; each value also passes through the other slot of the 2-vector (swap)."""
    dtype = torch.float32
    sigma, d2, d, rv, rdv, x = _fast_reference(g, si, p)
    t = _t(d2, dtype)
    v, dvd = torch.full_like(t, float("nan")), torch.full_like(t, float("nan"))
    pot = _desc(p, sigma)
    _ok(probe, probe.sr_probe_fast_rs_pk(_stream(), C.byref(pot), t.numel(), swap, t.data_ptr(), v.data_ptr(), dvd.data_ptr()))
    tol = bound(dtype, x, np.sqrt(x))
    check(f"fast_rs_eval_pk<{p}> sigma={sigma} swap={swap} v", dtype, _np(v), rv, np.abs(rv), tol)
    check(f"fast_rs_eval_pk<{p}> sigma={sigma} swap={swap} dv", dtype, _np(dvd) * d, rdv, np.abs(rdv) + p * np.abs(rv) / d, tol)


def _scalar(probe, which, x):
    t = _t(x, torch.float64)
    out = torch.full_like(t, float("nan"))
    _ok(probe, probe.sr_probe_scalar_f64(_stream(), which, t.numel(), t.data_ptr(), out.data_ptr()))
    return _np(out)


@pytest.mark.parametrize("which,name,tol", [(0, "exp_neg_fast", 3e-16), (4, "exp_neg_table2", 4e-16)])
def test_exp_forms(probe, g, which, name, tol):
    x, ref = g["exp_x"], g["exp_ref"]
    got = _scalar(probe, which, x)
    check(name, torch.float64, got, ref, ref, tol)
    assert np.all(got[x >= 746.0] == 0.0)


@pytest.mark.parametrize("which,name", [(1, "rcp_newton"), (2, "rsqrt_newton")])
def test_newton_reciprocals(probe, g, which, name):
    x = np.unique(np.concatenate([g["exp_x"][(g["exp_x"] > 0) & (g["exp_x"] < 1e3)], 1.0 + 0.4 * g["y"], [1e-30, 1e-12, 1e12]]
                                 + [g[f"m1_d2_s{i}"].astype(np.float64) for i in range(3)]))
    xl = x.astype(np.longdouble)
    ref = (1 / xl if which == 1 else 1 / np.sqrt(xl))
    got = _scalar(probe, which, x)
    err = np.abs((got.astype(np.longdouble) - ref) / ref).astype(np.float64)
    print(f"[sr-pointwise] {name:<44s} float64  max rel err {err.max():.3e}")
    assert err.max() <= 2 * 2.0**-52


@pytest.mark.parametrize("which,name", [(3, "erfc_from_exp(double) with exp_neg_fast"), (5, "erfc_from_table with exp_neg_table2")])
def test_erfc_forms(probe, g, which, name):
    y, ref = g["y"], g["erfc"]
    got = _scalar(probe, which, y)
    check(name, torch.float64, got, ref, ref, bound(torch.float64, y * y, y))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6])
def test_lower_gamma_series(probe, g, dtype, p):
    x = _t(g["lg_x"], dtype)
    out = torch.empty_like(x)
    _ok(probe, probe.sr_probe_lower_gamma(_stream(), _lib.dtype_code(dtype), p, x.numel(), x.data_ptr(), out.data_ptr()))
    ref = g[f"lg_P_p{p}"]
    check(f"lower_gamma_series p={p}", dtype, _np(out), ref, ref, 3e-6 if dtype == torch.float32 else 1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_atoms(probe, dtype):
    """d = 0 in the forms that document a floor (sr_eval: d >= 1e-15; fast_rs_eval: d^2 >= 1e-30, 1e-24 in float): a finite
    potential, and a force contribution -- v'/d times the zero pair vector -- of exactly zero.  1/r^6 cannot be finite in
    float32 at any floor that leaves real distances alone (1e-12^-6 = 1e72), so there it is the Coulomb form only."""
    z = torch.zeros(4, dtype=dtype, device=DEV)
    for p in ([1, 6] if dtype == torch.float64 else [1]):
        pot = _desc(p, 1.0)
        v, dv = torch.empty_like(z), torch.empty_like(z)
        _ok(probe, probe.sr_probe_sr_eval(_stream(), _lib.dtype_code(dtype), C.byref(pot), 4, z.data_ptr(), v.data_ptr(), dv.data_ptr()))
        assert torch.isfinite(v).all() and torch.isfinite(dv).all() and (v > 0).all(), (p, v, dv)
        _ok(probe, probe.sr_probe_fast_rs(_stream(), _lib.dtype_code(dtype), C.byref(pot), 4, z.data_ptr(), v.data_ptr(), dv.data_ptr()))
        assert torch.isfinite(v).all() and torch.isfinite(dv).all() and (v > 0).all(), (p, v, dv)
        assert ((dv * z) == 0).all()


# ---- (b) rows -----------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)
CELL = 60.0


class Stars:
    """Stars in a 60 x 60 x 60 cell: centres on a lattice of spacing 12 (and one at a corner of the cell, whose partners leave
    through three faces), the partners of a star of length L at the first L golden offsets.  Every star of length L has one copy
    per charged slot in {0, 1, 15, 16, 31, 32, L - 2, L - 1}: the centre and that partner carry charges, the other partners
    none.  Atoms are numbered star by star, centre first, so a wavefront's four rows hold a long row next to rows of length 1
    (partners) and 0 (the centres without partners that follow every star of length 300).  Two groups of four stars (QUADS) have
    their four centres numbered first, at a multiple of 4: one wavefront holds four long rows of unequal length, so the unmasked
    iteration of the packed / fp64 bodies (taken while every lane of the wave has both its entries inside its row: once for
    lengths 300, 129, 65, 33, twice for 300, 129, 128, 65) runs and hands over to the masked one, with the charged slots inside
    the unmasked part, at its last entry, and behind it.  All coordinates are multiples of
    2^-17 below 64: exact in float32, as are their differences and the +-60 of a cell shift -- the pair vector a kernel forms is
    the golden offset itself."""

    # two wavefronts of four long rows each (centres numbered first, at a multiple of 4, partners afterwards): (L, charged slot)
    QUADS = (((300, 5), (129, 20), (65, 31), (33, 32)), ((300, 63), (129, 64), (128, 127), (65, 40)))

    def __init__(self, g, full):
        off = g["rows_off"]
        groups = []
        for L in LENGTHS:
            for s in sorted({s for s in (0, 1, 15, 16, 31, 32, L - 2, L - 1) if 0 <= s < L}):
                groups.append([(L, s)])
                if L == 300:
                    groups.append([(0, -1)])
        groups.insert(7, [(0, -1)])
        groups += [list(quad) for quad in self.QUADS]
        groups.append([(129, 77)])  # the corner star
        lattice = iter([(6.0 + 12 * i, 6.0 + 12 * j, 6.0 + 12 * k) for i in range(5) for j in range(5) for k in range(5)])
        pos, q, pairs, shifts, self.partner, self.centre, self.quad_rows = [], [], [], [], [], [], []
        k = 0

        def filler():
            pos.append((3.0, 3.0, 3.0 + len(pos) % 7))
            q.append(0.25)
            self.centre.append((len(pos) - 1, -1, 0.0))

        for gi, group in enumerate(groups):
            if len(group) > 1:
                while len(pos) % 4:
                    filler()
                self.quad_rows.append(len(pos))
            heads = []
            for L, s in group:
                c = (59.5, 59.25, 0.5) if gi == len(groups) - 1 else next(lattice)
                qc = (1 if k % 2 else -1) * (512 + (37 * k) % 400) / 1024.0
                k += 1
                qs = 1.0 + s / 64.0 if s >= 0 else 0.0
                heads.append((len(pos), L, s, c, qc, qs))
                self.centre.append((len(pos), s, qs))  # (atom, charged slot, its charge)
                pos.append(c)
                q.append(qc)
            for ic, L, s, c, qc, qs in heads:
                for j in range(L):
                    r = np.asarray(c) + off[j]
                    w = np.floor(r / CELL)
                    self.partner.append((len(pos), j, qc))  # (atom, slot, charge of its centre)
                    pairs.append((ic, len(pos)))
                    shifts.append(w)
                    pos.append(r - CELL * w)
                    q.append(qs if j == s else 0.0)
        while len(pos) % 16 == 0 or len(pos) % 16 > 11:  # the last block partly invalid: 1..11 of its 16 rows in use
            filler()
        assert len(self.quad_rows) == 2 and all(a % 4 == 0 for a in self.quad_rows)
        self.pos, self.q = np.asarray(pos, np.float64), np.asarray(q, np.float64)
        pairs, shifts = np.asarray(pairs, np.int64), np.asarray(shifts, np.float64)
        assert np.all(self.pos * 2.0**17 == np.round(self.pos * 2.0**17)) and self.pos.min() >= 0 and self.pos.max() < 64
        assert np.abs(shifts).max() == 1 and len({tuple(t) for t in shifts}) >= 7
        if full:
            pairs = np.concatenate([pairs, pairs[:, ::-1]])
            shifts = np.concatenate([shifts, -shifts])
        self.pairs, self.shifts, self.full = pairs, shifts, full
        self.N = len(self.pos)
        self.off, self.d = off, g["rows_d"]
        self.x = self.d**2 / (2 * float(g["rows_sigma"]) ** 2)

    def expected(self, g, p):
        """(V, F, scale_V, scale_F, tol-x) per atom: V = 1/2 q v(d), F = -q v'(d) u with u the unit vector to the partner."""
        v, dv = g[f"rows_v_p{p}"], g[f"rows_dv_p{p}"]
        V, F = np.zeros(self.N), np.zeros((self.N, 3))
        sV, sF, x = np.zeros(self.N), np.zeros(self.N), np.zeros(self.N)
        f = 2.0 if self.full else 1.0  # a full list holds every pair in both roles: the force SUMS count it twice
        for a, j, qc in self.partner:
            V[a], F[a] = 0.5 * qc * v[j], f * qc * dv[j] * self.off[j] / self.d[j]
            sV[a], sF[a], x[a] = 0.5 * abs(qc * v[j]), f * abs(qc) * (abs(dv[j]) + p * abs(v[j]) / self.d[j]), self.x[j]
        for a, s, qs in self.centre:
            if s >= 0:
                V[a], F[a] = 0.5 * qs * v[s], -f * qs * dv[s] * self.off[s] / self.d[s]
                sV[a], sF[a], x[a] = 0.5 * abs(qs * v[s]), f * abs(qs) * (abs(dv[s]) + p * abs(v[s]) / self.d[s]), self.x[s]
        return V, F, sV, sF, x


def _check_rows(what, dtype, V, F, exp, tol_scale=1.0):
    rV, rF, sV, sF, x = exp
    tol = tol_scale * bound(dtype, x, np.sqrt(x))
    has = sV > 0
    check(what + " V", dtype, V[has], rV[has], sV[has], tol[has])
    check(what + " F", dtype, F[has].ravel(), rF[has].ravel(), np.repeat(sF[has], 3), np.repeat(tol[has], 3))
    # rows without a charged partner: zero-charge entries contribute exact zeros, never a NaN
    assert np.all(V[~has] == 0.0) and np.all(F[~has] == 0.0), (what, V[~has][:4], F[~has][:4])


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("p", [1, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_star_rows(probe, g, dtype, p, full):
    st = Stars(g, full)
    assert st.N % 16 != 0
    sigma = float(g["rows_sigma"])
    pos, q = _t(st.pos, dtype), _t(st.q, dtype)
    cell = _t(np.eye(3) * CELL, dtype)
    pairs, S = torch.tensor(st.pairs, device=DEV), _t(st.shifts, dtype)
    N = st.N
    topo = ops.get_topology(pairs, N)
    pot = _desc(p, sigma)
    lib = _lib.load()
    exp = st.expected(g, p)
    dt = _lib.dtype_code(dtype)
    results = {}

    def fused(ent, fmt):
        rec = torch.empty((N, 4), dtype=dtype, device=DEV)
        out, force = torch.full((N,), float("nan"), dtype=dtype, device=DEV), torch.full((N, 3), float("nan"), dtype=dtype, device=DEV)
        _lib.check(lib.mipme_sr_rows_fused(_stream(), dt, N, topo.row_ptr.data_ptr(), ent.data_ptr(), topo.entries.data_ptr(), None,
                                           pos.data_ptr(), cell.data_ptr(), q.data_ptr(), q.data_ptr(), None, 0, full, C.byref(pot),
                                           0, fmt, rec.data_ptr(), 0, out.data_ptr(), force.data_ptr(), None, None, None))
        return _np(out), _np(force)

    ent0, fmt0 = topo.entries_with_shifts(S, table=False)
    ent1, fmt1 = topo.entries_with_shifts(S, table=True)
    ent2 = topo.compact_entries(S)
    assert (fmt0, fmt1) == (0, 1) and ent2 is not None
    results["fused format 0"] = fused(ent0, 0)
    results["fused format 1"] = fused(ent1, 1)
    results["fused format 2"] = fused(ent2, 2)
    rec = torch.cat([pos, q[:, None]], 1).contiguous()
    out, force = torch.full((N,), float("nan"), dtype=dtype, device=DEV), torch.full((N, 3), float("nan"), dtype=dtype, device=DEV)
    body = probe.sr_probe_rows_pk if dtype == torch.float32 else probe.sr_probe_rows_f64
    _ok(probe, body(_stream(), p, N, topo.row_ptr.data_ptr(), ent2.data_ptr(), pos.data_ptr(), cell.data_ptr(), q.data_ptr(),
                    rec.data_ptr(), C.byref(pot), full, out.data_ptr(), force.data_ptr()))
    results["packed fp32 body" if dtype == torch.float32 else "fp64 table body"] = (_np(out), _np(force))
    torch.cuda.synchronize()
    for name, (V, F) in results.items():
        _check_rows(f"rows p={p} full={full} {name}", dtype, V, F, exp)
    # ... and with each other, within the sum of their bounds
    names = list(results)
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            (Va, Fa), (Vb, Fb) = results[names[i]], results[names[j]]
            _check_rows(f"rows p={p} full={full} {names[i]} / {names[j]}", dtype, Va, Fa, (Vb, Fb) + exp[2:], tol_scale=2.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_atoms_rows(probe, dtype):
    """Three charged atoms at one position, all paired, through the bodies that document a floor on d^2: the fp64 table body
    (rows_body.h: d^2 >= 1e-30) and the generic body with fast_rs_eval (fp64 format 2: 1e-30; fp32 format 1, Coulomb: 1e-24).
    Potentials: 1/2 sum q_o pref Q(p/2, ~0) / d_min^p = 1/2 sum q_o d_min^-p to the accuracy of rsq (fp64: one Newton step,
    2.4e-15 per power of 1/d: 1e-13 for p = 6; fp32: 1 ulp and the rounding of 1e-24: 1e-6); forces exactly zero."""
    pos = _t([[7.25, 8.5, 9.75]] * 3, dtype)
    qn = np.array([0.75, -1.25, 2.0])
    q, cell = _t(qn, dtype), _t(np.eye(3) * CELL, dtype)
    pairs, S = torch.tensor([[0, 1], [0, 2], [1, 2]], device=DEV), torch.zeros((3, 3), dtype=dtype, device=DEV)
    N = 3
    topo = ops.get_topology(pairs, N)
    lib = _lib.load()
    cases = [("fp64 table body", 1), ("fp64 table body", 6), ("fused format 2", 1), ("fused format 2", 6)] if dtype == torch.float64 \
        else [("fused format 1", 1)]
    for name, p in cases:
        pot = _desc(p, 1.0)
        rec = torch.cat([pos, q[:, None]], 1).contiguous()
        out, force = torch.full((N,), float("nan"), dtype=dtype, device=DEV), torch.full((N, 3), float("nan"), dtype=dtype, device=DEV)
        if name == "fp64 table body":
            ent = topo.compact_entries(S)
            _ok(probe, probe.sr_probe_rows_f64(_stream(), p, N, topo.row_ptr.data_ptr(), ent.data_ptr(), pos.data_ptr(), cell.data_ptr(),
                                               q.data_ptr(), rec.data_ptr(), C.byref(pot), 0, out.data_ptr(), force.data_ptr()))
        else:
            fmt = int(name[-1])
            ent = topo.compact_entries(S) if fmt == 2 else topo.entries_with_shifts(S, table=True)[0]
            _lib.check(lib.mipme_sr_rows_fused(_stream(), _lib.dtype_code(dtype), N, topo.row_ptr.data_ptr(), ent.data_ptr(),
                                               topo.entries.data_ptr(), None, pos.data_ptr(), cell.data_ptr(), q.data_ptr(), q.data_ptr(),
                                               None, 0, 0, C.byref(pot), 0, fmt, rec.data_ptr(), 1, out.data_ptr(), force.data_ptr(),
                                               None, None, None))
        V, F = _np(out), _np(force)
        dmin = 1e-15 if dtype == torch.float64 else 1e-12
        want = 0.5 * (qn.sum() - qn) * dmin**-p
        err = np.abs(V - want) / np.abs(want)
        print(f"[sr-pointwise] coincident atoms {name} p={p} {str(dtype)[6:]}: V {V}, max rel err {err.max():.3e}, F {F.ravel()}")
        assert np.all(np.isfinite(V)) and err.max() <= (1e-13 if dtype == torch.float64 else 1e-6), (name, p, V, want)
        assert np.all(F == 0.0), (name, p, F)


# ---- (c) the co-scheduled and the frames launch ---------------------------------------------------------------------------------
def _rell2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / (np.linalg.norm(np.asarray(b)) + 1e-300))


def test_star_system_coscheduled(g, monkeypatch):
    """The stars through P3MCalculator in fp64 with the pair sum co-scheduled into the spread launch (the fp64 table body) and as
    a launch of its own, and through GraphedFrameBatch (one frame): all to the 1e-12 of test_coscheduled_pair_sum."""
    dtype = torch.float64
    st = Stars(g, 0)
    calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=float(g["rows_sigma"])), mesh_spacing=2.0, interpolation_nodes=5).to(dtype)
    tq, tc = _t(st.q[:, None], dtype), _t(np.eye(3) * CELL, dtype)
    ti, tS = torch.tensor(st.pairs, device=DEV), _t(st.shifts, dtype)
    res = {}
    for co in (True, False):
        monkeypatch.setattr(ops, "COSCHEDULE", co)
        tp = _t(st.pos, dtype).requires_grad_(True)
        _lib.profile_enable(True)
        d = tpa.pair_distances(tp, ti, tc, tS, deferred=True)
        V = calc(tq, tc, tp, ti, d)
        L = -0.7 * tpa.weighted_sum(V, tq)
        L.backward()
        stages = _lib.profile_report()
        _lib.profile_enable(False)
        assert ("spread+rspace_forward" in stages) == co, stages.keys()
        res[co] = (_np(d.detach()), _np(V.detach()), _np(tp.grad), float(L.detach()) / -0.7)
    want_d = st.d[[j for _, j, _ in st.partner]]
    assert np.abs(res[True][0] - want_d).max() / want_d.max() < 1e-14
    for a, b in zip(res[True][:3], res[False][:3]):
        assert _rell2(a, b) < 1e-12
    monkeypatch.setattr(ops, "COSCHEDULE", True)
    batch = tpa.GraphedFrameBatch(calc, [(tq, tc, _t(st.pos, dtype), ti, tS)])
    E, F = batch()
    V, grad, Eref = res[False][1], res[False][2] / -0.7, res[False][3]
    scale = float(np.abs(st.q[:, None] * V).sum())
    eE, eF = abs(float(E[0]) - Eref) / scale, _rell2(_np(F[0]), -grad)
    print(f"[sr-pointwise] frames launch against the separate launches: energy {eE:.3e} of sum |q V|, forces rel-L2 {eF:.3e}")
    assert eE < 1e-12
    assert eF < 1e-12
