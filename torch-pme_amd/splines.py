"""Cubic splines of a radial function and of its Fourier-space kernel (reference ``lib/splines.py``): what
:class:`~potentials.SplinePotential` is made of.

Construction runs once, on the host, in float64 (NumPy): the second derivatives of the natural spline from one Thomas sweep
(:func:`compute_second_derivatives`), the radial Fourier transform of the spline and of its 1/r tail (:func:`compute_spline_ft`,
with a cosine integral of its own: the package does not need scipy).  Evaluation is

* on CPU tensors the reference's expression in plain tensor operations (float64 tables, differentiable by autograd), and
* on device tensors ``csrc/spline.hip``: :class:`_SplineEval` is ``S^(m)(x)`` for m = 0..3 (``mipme_spline_eval``), its
  backward the same node one order up, so a spline is differentiable to any order in its argument (orders above 3 are zero);
  :class:`_SplineReciprocal` is the composite of a reciprocal-axis spline with its first derivative from the same pass
  (``mipme_spline_eval_reciprocal``) and, when its backward pass is itself recorded, the plain nodes glued with tensor
  operations.

The knot tables are float64 on the device and the spline is evaluated in double precision whatever the argument's type; the
result has the dtype of the argument.  (The reference evaluates in the dtype of the grids and promotes the result to it.)
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

_EULER_GAMMA = 0.5772156649015329


# ---- host side: construction -----------------------------------------------------------------------------------------------
def _second_derivatives(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Second derivatives of the natural cubic spline through (x, y): the tridiagonal system
    ``h[i-1]/6 m[i-1] + (h[i-1]+h[i])/3 m[i] + h[i]/6 m[i+1] = dy[i] - dy[i-1]``, ``m[0] = m[n-1] = 0``, by one Thomas sweep
    over Python floats (float64)."""
    n = len(x)
    out = np.zeros(n, dtype=np.float64)
    if n < 3:
        return out
    h = np.diff(x)
    dy = np.diff(y) / h
    sub, diag, sup, rhs = (h[:-1] / 6).tolist(), ((h[:-1] + h[1:]) / 3).tolist(), (h[1:] / 6).tolist(), np.diff(dy).tolist()
    m = n - 2  # interior unknowns
    cp, dp = [0.0] * m, [0.0] * m
    cp[0], dp[0] = sup[0] / diag[0], rhs[0] / diag[0]
    for i in range(1, m):
        den = diag[i] - sub[i] * cp[i - 1]
        cp[i] = sup[i] / den
        dp[i] = (rhs[i] - sub[i] * dp[i - 1]) / den
    sol = [0.0] * m
    sol[-1] = dp[-1]
    for i in range(m - 2, -1, -1):
        sol[i] = dp[i] - cp[i] * sol[i + 1]
    out[1:-1] = sol
    return out


def _as_f64(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        return t.detach().to("cpu", torch.float64).numpy().reshape(-1)
    return np.asarray(t, dtype=np.float64).reshape(-1)


def compute_second_derivatives(x_points: torch.Tensor, y_points: torch.Tensor) -> torch.Tensor:
    """Second derivatives at the knots of the natural cubic spline through ``(x_points, y_points)`` (reference
    ``lib/splines.py:159-197``).  Computed on the host in float64, returned in the dtype and on the device of ``x_points``."""
    d2 = _second_derivatives(_as_f64(x_points), _as_f64(y_points))
    return torch.tensor(d2, dtype=x_points.dtype, device=x_points.device)


def cosine_integral(x) -> np.ndarray:
    """Ci(x) = gamma + ln x + int_0^x (cos t - 1)/t dt for x > 0 in float64: the power series
    ``gamma + ln x + sum_n (-1)^n x^2n / (2n (2n)!)`` up to x = 3, above that the continued fraction of E1(ix) by the modified
    Lentz recurrence (``Ci = -Re E1(ix)``), 120 terms (converged to rounding from x = 3 on)."""
    x = np.asarray(x, dtype=np.float64)
    small = x <= 3.0
    xs = np.where(small, x, 1.0)
    x2 = xs * xs
    term = np.ones_like(xs)
    total = np.zeros_like(xs)
    for n in range(1, 26):
        term = term * (-x2) / ((2 * n - 1) * (2 * n))
        total = total + term / (2 * n)
    with np.errstate(divide="ignore", invalid="ignore"):
        series = _EULER_GAMMA + np.log(xs) + total
    xl = np.where(small, 3.0, x)
    b = 1.0 + 1j * xl
    c = np.full_like(b, 1e300)
    d = 1.0 / b
    h = d.copy()
    for i in range(1, 121):
        a = -float(i * i)
        b = b + 2.0
        d = 1.0 / (a * d + b)
        c = b + a / c
        h = h * (c * d)
    h = h * (np.cos(xl) - 1j * np.sin(xl))
    return np.where(small, series, -h.real)


_GL_NODES, _GL_WEIGHTS = np.polynomial.legendre.leggauss(16)


def _spline_ft(k: np.ndarray, x: np.ndarray, y: np.ndarray, d2: np.ndarray) -> np.ndarray:
    """``4 pi int_0^inf sin(kr)/k r f(r) dr`` for the spline f and its 1/r tail, float64.

    Interval [r_i, r_i+1], P(r) = r S_i(r) (a quartic).  Where ``k dr >= 2``, by four integrations by parts,

        int P sin(kr) dr = [ -P cos/k + P' sin/k^2 + P'' cos/k^3 - P''' sin/k^4 - P'''' cos/k^5 ]

    whose successive terms fall like ``1/(k dr)``: no large cancellation there.  Where ``k dr < 2`` -- where that expression, like
    the reference's k^-6 Horner form, is a difference of large terms -- by 16-point Gauss-Legendre quadrature of
    ``P(r) r sinc(kr)``: the phase changes by less than 2 across the interval, so the rule is exact to rounding, and at k = 0
    the integrand is the quintic ``r P(r)``: the finite limit comes out of the same line.
    Tail beyond r_N: ``r f(r) = A + B / r^2`` with ``A = y_N r_N - d2/(6 r_N)``, ``B = d2 r_N / 6`` and, in the Abel-regularised
    sense, ``int_rN^inf sin(kr) dr = cos(k r_N)/k``, ``int_rN^inf sin(kr)/r^2 dr = sin(k r_N)/r_N - k Ci(k r_N)``; none at k = 0."""
    n = len(x)
    r0, r1 = x[:-1], x[1:]
    h = r1 - r0
    y0, y1, m0, m1 = y[:-1], y[1:], d2[:-1], d2[1:]
    # S(r) = c0 + c1 t + c2 t^2 + c3 t^3, t = r - r0
    c0 = y0
    c1 = (y1 - y0) / h - h * (2 * m0 + m1) / 6
    c2 = m0 / 2
    c3 = (m1 - m0) / (6 * h)

    def poly_derivs(t):  # P = (r0 + t) S and its four derivatives at offset t (broadcast over intervals)
        r = r0 + t
        S = c0 + t * (c1 + t * (c2 + t * c3))
        S1 = c1 + t * (2 * c2 + 3 * t * c3)
        S2 = 2 * c2 + 6 * t * c3
        S3 = 6 * c3
        return r * S, S + r * S1, 2 * S1 + r * S2, 3 * S2 + r * S3, 4 * S3

    Pa, Pb = poly_derivs(np.zeros_like(h)), poly_derivs(h)
    out = np.zeros(len(k), dtype=np.float64)
    tn = 0.5 * (_GL_NODES + 1.0)  # nodes on [0, 1]
    tq = h[:, None] * tn[None, :]  # (N-1, Q)
    rq = r0[:, None] + tq
    Sq = c0[:, None] + tq * (c1[:, None] + tq * (c2[:, None] + tq * c3[:, None]))
    wq = 0.5 * h[:, None] * _GL_WEIGHTS[None, :] * rq * rq * Sq  # weights x r P(r)
    for a, kk in enumerate(k):
        if kk == 0.0:
            out[a] = wq.sum()
            continue
        closed = kk * h >= 2.0

        def bracket(P, r):
            cs, sn = np.cos(kk * r), np.sin(kk * r)
            return -P[0] * cs / kk + P[1] * sn / kk**2 + P[2] * cs / kk**3 - P[3] * sn / kk**4 - P[4] * cs / kk**5

        by_parts = (bracket(Pb, r1) - bracket(Pa, r0)) / kk
        quad = (wq * np.sinc(kk * rq / np.pi)).sum(axis=1)
        out[a] = np.where(closed, by_parts, quad).sum()
    # ---- tail: the natural spline in u = 1/r through (0, 0), (1/r_N, y_N), (1/r_N-1, y_N-1), continued to u -> 0
    rN, yN = x[-1], y[-1]
    tail_d2 = _second_derivatives(np.array([0.0, 1.0 / x[-1], 1.0 / x[-2]]), np.array([0.0, y[-1], y[-2]]))[1]
    A, B = yN * rN - tail_d2 / (6 * rN), tail_d2 * rN / 6
    nz = k != 0.0
    ks = np.where(nz, k, 1.0)
    tail = (A * np.cos(ks * rN) / ks + B * (np.sin(ks * rN) / rN - ks * cosine_integral(ks * rN))) / ks
    return 4 * math.pi * (out + np.where(nz, tail, 0.0))


def compute_spline_ft(k_points: torch.Tensor, x_points: torch.Tensor, y_points: torch.Tensor,
                      d2y_points: torch.Tensor) -> torch.Tensor:
    r"""Radial Fourier transform :math:`\hat f(k) = 4\pi\int \mathrm{d}r\, \frac{\sin kr}{k}\, r f(r)` of a splined function,
    including the tail beyond the last knot (reference ``lib/splines.py:200-379``; see :func:`_spline_ft` for how the
    integrals are taken -- the values are those of the integral itself, to rounding, also where the reference's closed form
    loses digits).  Host, float64; returned in the dtype and on the device of ``k_points``."""
    ft = _spline_ft(_as_f64(k_points), _as_f64(x_points), _as_f64(y_points), _as_f64(d2y_points))
    return torch.tensor(ft, dtype=k_points.dtype, device=k_points.device).reshape(k_points.shape)


# ---- device side -----------------------------------------------------------------------------------------------------------
#: knots up to which ``csrc/spline.hip`` stages a table in LDS (3 arrays of doubles: 48 KB, three workgroups per CU)
LDS_KNOTS = 2048


class _Table:
    """One plain spline: float64 knots on the host and, per device, a (3, n) float64 tensor ``x | y | d2y`` with the
    ``mipme_spline_t`` that points at it."""

    def __init__(self, x: np.ndarray, y: np.ndarray, d2: np.ndarray | None = None):
        self.x, self.y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
        self.d2 = _second_derivatives(self.x, self.y) if d2 is None else np.ascontiguousarray(d2, dtype=np.float64)
        self.n = len(self.x)
        self._dev = {}
        self._cpu = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_dev"], state["_cpu"] = {}, None
        return state

    def cpu(self):
        if self._cpu is None:
            self._cpu = tuple(torch.from_numpy(a) for a in (self.x, self.y, self.d2))
        return self._cpu

    def tensor(self, device) -> torch.Tensor:
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = torch.from_numpy(np.stack([self.x, self.y, self.d2])).to(device)
        return t

    def fill(self, desc, device):
        t = self.tensor(device)
        desc.x, desc.y, desc.d2y, desc.n = t.data_ptr(), t.data_ptr() + 8 * self.n, t.data_ptr() + 16 * self.n, self.n
        return t


def _eval_torch(x: torch.Tensor, table: _Table) -> torch.Tensor:
    """The reference's expression (``lib/splines.py:25-42``) on float64 tables; differentiable w.r.t. ``x`` by autograd."""
    X, Y, D2 = table.cpu()
    xd = x.to(torch.float64)
    i = torch.clamp(torch.searchsorted(X, xd.detach(), right=True) - 1, 0, table.n - 2)
    h = X[i + 1] - X[i]
    a = (X[i + 1] - xd) / h
    b = (xd - X[i]) / h
    h2over6 = h * h / 6
    out = a * (Y[i] + (a * a - 1) * D2[i] * h2over6) + b * (Y[i + 1] + (b * b - 1) * D2[i + 1] * h2over6)
    return out.to(x.dtype)


def _check_arg(x: torch.Tensor):
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"splines are evaluated on float32 and float64 tensors, got {x.dtype}")


class _SplineEval(torch.autograd.Function):
    """``S^(order)(x)`` of a plain spline on the device; the backward is the same node at ``order + 1``."""

    @staticmethod
    def forward(ctx, x, table, order):
        ctx.save_for_backward(x)
        ctx.table, ctx.order = table, order
        xc = x.detach().contiguous()
        if order > 3:  # (a cubic: never asked of the kernel)
            return torch.zeros_like(xc)
        out = torch.empty_like(xc)
        if xc.numel() == 0:
            return out
        desc = _lib.SplineDesc()
        keep = table.fill(desc, xc.device)  # noqa: F841  (the table outlives the launch: cached on `table`)
        with _lib.on_device(xc.device):
            _lib.check(_lib.load().mipme_spline_eval(_lib.current_stream(xc.device), _lib.dtype_code(xc.dtype), C.byref(desc),
                                                     order, xc.numel(), xc.data_ptr(), out.data_ptr()))
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * _SplineEval.apply(x, ctx.table, ctx.order + 1), None, None


class _SplineReciprocal(torch.autograd.Function):
    """``x < x0 ? Z(x) : R(1/x)`` with its first derivative from the same pass; a recorded backward (``create_graph=True``)
    differentiates the composition of plain nodes instead (the split of ``ops.fused_first_analytic_higher``)."""

    @staticmethod
    def forward(ctx, x, spline):
        xc = x.detach().contiguous()
        out = torch.empty_like(xc)
        want = ctx.needs_input_grad[0]
        dout = torch.empty_like(xc) if want else None
        if xc.numel():
            desc = spline._descriptor(xc.device)
            with _lib.on_device(xc.device):
                _lib.check(_lib.load().mipme_spline_eval_reciprocal(
                    _lib.current_stream(xc.device), _lib.dtype_code(xc.dtype), C.byref(desc), xc.numel(), xc.data_ptr(),
                    out.data_ptr(), _lib.ptr(dout)))
        ctx.spline = spline
        ctx.save_for_backward(x, dout)
        return out

    @staticmethod
    def backward(ctx, g):
        x, dout = ctx.saved_tensors
        if torch.is_grad_enabled():  # the backward pass is being recorded: a derivative that can be differentiated again
            return g * ctx.spline._composed_derivative(x), None
        return g * dout, None


class CubicSpline(torch.nn.Module):
    """Natural cubic spline of a real-valued function (reference ``lib/splines.py:4-42``).  The interval of an argument is
    ``searchsorted(x_points, x, right=True) - 1`` clamped to ``[0, n - 2]``: the end cubics extrapolate on both sides.

    :param x_points: abscissas of the knots (increasing)
    :param y_points: ordinates of the knots
    """

    def __init__(self, x_points: torch.Tensor, y_points: torch.Tensor):
        super().__init__()
        self.x_points = x_points
        self.y_points = y_points
        self._table = _Table(_as_f64(x_points), _as_f64(y_points))
        self.d2y_points = torch.tensor(self._table.d2, dtype=x_points.dtype, device=x_points.device)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            return _eval_torch(x, self._table)
        _check_arg(x)
        return _SplineEval.apply(x, self._table, 0)


class CubicSplineReciprocal(torch.nn.Module):
    r"""Spline on a :math:`1/x` axis that goes smoothly to zero as :math:`x\rightarrow\infty` (reference
    ``lib/splines.py:45-121``): the natural spline in ``1/x`` through ``(0, 0)`` and the flipped points; below ``x_points[0]``
    the 3-knot spline through ``(0, y_at_zero)``, ``(x0, y0)``, ``(x1, y1)``.

    :param x_points: abscissas of the knots, strictly positive
    :param y_points: ordinates of the knots
    :param y_at_zero: value at zero; defaults to ``y_points[0]``
    """

    def __init__(self, x_points: torch.Tensor, y_points: torch.Tensor, y_at_zero=None):
        super().__init__()
        x, y = _as_f64(x_points), _as_f64(y_points)
        self._rev = _Table(np.concatenate([[0.0], 1.0 / x[::-1]]), np.concatenate([[0.0], y[::-1]]))
        y0 = float(y[0]) if y_at_zero is None else float(y_at_zero)
        self._y_at_zero = y0
        self._zero = _Table(np.array([0.0, x[0], x[1]]), np.array([y0, y[0], y[1]]))
        self._split = float(x[0])
        self._desc = {}

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_desc"] = {}
        return state

    def _descriptor(self, device, prefactor: float = 1.0):
        """``mipme_spline_t`` of the composite on ``device`` (one struct per device and prefactor)."""
        d = self._desc.get((device, prefactor))
        if d is None:
            d = _lib.SplineDesc(reciprocal=1, prefactor=prefactor)
            self._rev.fill(d, device)
            for c in range(3):
                d.zero_x[c], d.zero_y[c], d.zero_d2y[c] = self._zero.x[c], self._zero.y[c], self._zero.d2[c]
            self._desc[(device, prefactor)] = d
        return d

    def _composed_derivative(self, x):
        """The first derivative of the composite from the plain nodes and tensor operations (differentiable again)."""
        below = x < self._split
        safe = torch.where(below, torch.full_like(x, self._split), x)
        u = torch.reciprocal(safe)
        return torch.where(below, _SplineEval.apply(x, self._zero, 1), -_SplineEval.apply(u, self._rev, 1) * u * u)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            below = x < self._split
            safe = torch.where(below, torch.full_like(x, self._split), x)
            return torch.where(below, _eval_torch(x, self._zero), _eval_torch(torch.reciprocal(safe), self._rev))
        _check_arg(x)
        return _SplineReciprocal.apply(x, self)


def spline_descriptor(spline, device, prefactor: float):
    """``mipme_spline_t`` of a :class:`CubicSpline` / :class:`CubicSplineReciprocal` with a prefactor (``mipme_spline_kfilter_build``)."""
    if isinstance(spline, CubicSplineReciprocal):
        return spline._descriptor(device, prefactor)
    d = _lib.SplineDesc(reciprocal=0, prefactor=prefactor)
    spline._table.fill(d, device)
    return d


def build_filter(geom, spline, prefactor: float, dtype, device) -> torch.Tensor:
    """G(k) = prefactor * spline(|k|^2) (/ U^2 for P3M) on the rfft half grid of ``geom``, by ``mipme_spline_kfilter_build``."""
    G = torch.empty((geom.ns[0], geom.ns[1], geom.ns[2] // 2 + 1), dtype=dtype, device=device)
    desc = spline_descriptor(spline, device, prefactor)
    md = geom.desc(1)
    with _lib.on_device(device):
        _lib.check(_lib.load().mipme_spline_kfilter_build(_lib.current_stream(device), _lib.dtype_code(dtype), C.byref(md),
                                                          C.byref(desc), G.data_ptr()))
    return G
