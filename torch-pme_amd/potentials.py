"""Pair potentials 1/r^p with Gaussian range separation (reference ``potentials/potential.py``,
``potentials/coulomb.py``, ``potentials/inversepowerlaw.py``).

Same constructor signatures, buffer names (``smearing``, ``prefactor``, ``exponent`` as float64
buffers; ``exclusion_radius``, ``exclusion_degree`` attributes) and method names as the reference,
so user code and ``state_dict`` round-trips carry over.  On the hot path the calculators do NOT call
these Python methods: they hand :meth:`Potential._descriptor` to the fused HIP kernels
(``csrc/rspace.hip`` evaluates v_SR and its derivative per pair, ``csrc/kfilter.hip`` evaluates the
Fourier-space kernel per mesh point).  The elementwise methods below exist for inspection and plotting,
as small closed-form tensor expressions.
"""

from __future__ import annotations

import math

import torch

from . import _lib

_SQRT_PI = math.sqrt(math.pi)


def _reg_upper_gamma(p: int, x: torch.Tensor) -> torch.Tensor:
    """Q(p/2, x) for integer p: finite sums (integer p/2) or erfc plus a finite sum (half-integer)."""
    ex = torch.exp(-x)
    if p % 2 == 0:
        term = torch.ones_like(x)
        total = torch.ones_like(x)
        for k in range(1, p // 2):
            term = term * x / k
            total = total + term
        return ex * total
    sx = torch.sqrt(x)
    q = torch.erfc(sx)
    term = ex / (_SQRT_PI * sx.clamp(min=1e-300))
    for k in range(1, (p - 1) // 2 + 1):
        term = term * x / (k - 0.5)
        q = q + term
    return q


def _exp1(z: torch.Tensor) -> torch.Tensor:
    """E1(z) = Gamma(0, z) for z > 0 (what the reference gets from ``lib/math.py:5-83``): power series
    -gamma - ln z - sum_k (-z)^k / (k k!) below z = 1, modified-Lentz continued fraction 1/(z+1-1/(z+3-4/(z+5-...))) above;
    both to double-precision rounding, as plain tensor expressions (differentiable)."""
    zs = z.clamp(max=1.0)
    term = torch.ones_like(z)
    ssum = torch.zeros_like(z)
    for k in range(1, 26):
        term = term * (-zs) / k
        ssum = ssum - term / k
    series = -0.5772156649015329 - torch.log(zs) + ssum
    zl = z.clamp(min=1.0)
    b = zl + 1.0
    c = torch.full_like(z, 1e300)
    d = 1.0 / b
    h = d
    for i in range(1, 61):
        an = -float(i * i)
        b = b + 2.0
        d = 1.0 / (an * d + b)
        c = b + an / c
        h = h * (c * d)
    return torch.where(z < 1.0, series, h * torch.exp(-zl))


_INV_GAMMA_HALF = {p: 1.0 / math.gamma(0.5 * p + 1.0) for p in range(1, 7)}


def _reg_lower_gamma(p: int, x: torch.Tensor) -> torch.Tensor:
    """P(p/2, x) = 1 - Q without the cancellation at small x: power series x^a e^-x sum_k x^k / Gamma(a+k+1) below x = 1
    (the reference calls ``torch.special.gammainc``, ``inversepowerlaw.py:98-103``), 1 - Q above."""
    a = 0.5 * p
    xs = x.clamp(max=1.0)
    term = torch.full_like(x, _INV_GAMMA_HALF[p])
    total = term.clone()
    for k in range(1, 25):
        term = term * xs / (a + k)
        total = total + term
    series = xs**a * torch.exp(-xs) * total
    return torch.where(x < 1.0, series, 1 - _reg_upper_gamma(p, x))


class Potential(torch.nn.Module):
    """Base interface of a pair potential (reference ``potentials/potential.py:4-212``).

    :param smearing: length scale of the SR/LR split (``None``: no split, real-space only)
    :param exclusion_radius: radius inside which the potential is smoothly switched off
    :param exclusion_degree: exponent of the raised-cosine switch
    :param prefactor: multiplicative prefactor (see :mod:`prefactors`)
    """

    _kind = None  # set by subclasses the HIP kernels know

    def __init__(
        self,
        smearing: float | None = None,
        exclusion_radius: float | None = None,
        exclusion_degree: int = 1,
        prefactor: float = 1.0,
    ):
        super().__init__()
        if smearing is not None:
            self.register_buffer("smearing", torch.tensor(smearing, dtype=torch.float64))
        else:
            self.smearing = None
        self.exclusion_radius = exclusion_radius
        self.exclusion_degree = exclusion_degree
        self.register_buffer("prefactor", torch.tensor(prefactor, dtype=torch.float64))
        self._host_cache = None

    # ---- host-side view of the parameters (buffers may live on the device) -------------------
    def _host_params(self):
        """(smearing|None, prefactor, exponent) as Python floats; one D2H copy, then cached."""
        key = (
            None if self.smearing is None else (self.smearing.data_ptr(), self.smearing._version),
            (self.prefactor.data_ptr(), self.prefactor._version),
        )
        if self._host_cache is None or self._host_cache[0] != key:
            sm = None if self.smearing is None else float(self.smearing)
            self._host_cache = (key, sm, float(self.prefactor), self._exponent_int())
        return self._host_cache[1:]

    def _exponent_int(self) -> int:
        raise NotImplementedError

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_host_cache"] = None  # host copies of the buffers / the C descriptor: rebuilt on first use
        state.pop("_desc_cache", None)
        return state

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._host_cache = None
        return out

    def _descriptor(self) -> _lib.PotentialDesc:
        """The plain-C description consumed by libmipme (``mipme_potential_t``)."""
        if self._kind is None:
            raise TypeError(
                f"{self.__class__.__name__} has no HIP kernel: the MI355X-native calculators support "
                "CoulombPotential and InversePowerLawPotential"
            )
        sm, pref, p = self._host_params()
        key = (sm, pref, p, self.exclusion_radius, self.exclusion_degree)
        cached = self.__dict__.get("_desc_cache")
        if cached is not None and cached[0] == key:
            return cached[1]  # read-only for the library: one struct per parameter set instead of one per call
        desc = _lib.PotentialDesc(
            kind=self._kind,
            exponent=p,
            smearing=-1.0 if sm is None else sm,
            prefactor=pref,
            exclusion_radius=-1.0 if self.exclusion_radius is None else float(self.exclusion_radius),
            exclusion_degree=int(self.exclusion_degree),
        )
        self.__dict__["_desc_cache"] = (key, desc)
        return desc

    # ---- reference method surface ------------------------------------------------------------
    def f_cutoff(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        """1 - ((1 - cos(pi r / r_excl)) / 2)^n inside the exclusion radius, 0 outside."""
        if self.exclusion_radius is None:
            raise ValueError("Cannot compute cutoff function when `exclusion_radius` is not set")
        rx = self.exclusion_radius
        inside = dist < rx
        base = 0.5 * (1 - torch.cos(torch.pi * dist / rx))
        out = torch.where(inside, 1 - base**self.exclusion_degree, torch.zeros_like(dist))
        return out if pair_mask is None else out * pair_mask

    def from_dist(self, dist, pair_mask=None):
        raise NotImplementedError(f"from_dist is not implemented for {self.__class__.__name__}")

    def lr_from_dist(self, dist, pair_mask=None):
        raise NotImplementedError(f"lr_from_dist is not implemented for {self.__class__.__name__}")

    def sr_from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        """V_SR = V - V_LR, or -V_LR * f_cut when an exclusion radius is set."""
        if self.smearing is None:
            raise ValueError("Cannot compute range-separated potential when `smearing` is not specified.")
        if self.exclusion_radius is None:
            return self.from_dist(dist, pair_mask=pair_mask) - self.lr_from_dist(dist, pair_mask=pair_mask)
        return -self.lr_from_dist(dist, pair_mask=pair_mask) * self.f_cutoff(dist, pair_mask=pair_mask)

    def lr_from_k_sq(self, k_sq):
        raise NotImplementedError(f"lr_from_k_sq is not implemented for {self.__class__.__name__}")

    def kernel_from_k_sq(self, k_sq: torch.Tensor) -> torch.Tensor:
        return self.lr_from_k_sq(k_sq)

    def self_contribution(self):
        raise NotImplementedError(f"self_contribution is not implemented for {self.__class__.__name__}")

    def background_correction(self):
        raise NotImplementedError(f"background_correction is not implemented for {self.__class__.__name__}")

    def pbc_correction(self, periodic, positions, cell, charges):
        """Correction for systems that are not periodic in all three directions; zero unless a subclass has one."""
        return self.prefactor * torch.zeros_like(charges)


class _PowerLawPotential(Potential):
    """Shared closed forms for 1/r^p, integer p in 1..6."""

    _p = 1

    def _exponent_int(self) -> int:
        return self._p

    def from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        out = dist.clamp(min=1e-15) ** (-self._p)
        if pair_mask is not None:
            out = out * pair_mask
        return self.prefactor * out

    def lr_from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        if self.smearing is None:
            raise ValueError("Cannot compute long-range contribution without specifying `smearing`.")
        d = dist.clamp(min=1e-12)
        x = 0.5 * d * d / self.smearing**2
        out = _reg_lower_gamma(self._p, x) / d**self._p
        if pair_mask is not None:
            out = out * pair_mask
        return self.prefactor * out

    def lr_from_k_sq(self, k_sq: torch.Tensor) -> torch.Tensor:
        if self.smearing is None:
            raise ValueError("Cannot compute long-range kernel without specifying `smearing`.")
        p = self._p
        a = 0.5 * (3 - p)
        c0 = math.pi**1.5 / math.gamma(0.5 * p) * (2 * self.smearing**2) ** a
        zero = k_sq == 0
        z = 0.5 * self.smearing**2 * torch.where(zero, torch.ones_like(k_sq), k_sq)
        ez = torch.exp(-z)
        if p == 1:
            f = ez / z
        elif p == 2:
            f = torch.sqrt(torch.pi / z) * torch.erfc(torch.sqrt(z))
        elif p == 4:
            f = 2 * (ez - torch.sqrt(torch.pi * z) * torch.erfc(torch.sqrt(z)))
        elif p == 6:
            f = ((2 - 4 * z) * ez + 4 * torch.sqrt(torch.pi * z**3) * torch.erfc(torch.sqrt(z))) / 3
        elif p == 3:  # Gamma(0, z) = E1(z)
            f = _exp1(z)
        else:  # p == 5: Gamma(-1, z) / z^-1 = e^-z - z E1(z)
            f = ez - z * _exp1(z)
        k0 = -c0 / a if p > 3 else 0.0
        return self.prefactor * torch.where(zero, k0 * torch.ones_like(k_sq), c0 * f)

    def self_contribution(self) -> torch.Tensor:
        if self.smearing is None:
            raise ValueError("Cannot compute self contribution without specifying `smearing`.")
        ph = 0.5 * self._p
        return self.prefactor / math.gamma(ph + 1) / (2 * self.smearing**2) ** ph

    def background_correction(self) -> torch.Tensor:
        if self.smearing is None:
            raise ValueError("Cannot compute background correction without specifying `smearing`.")
        p = self._p
        if p >= 3:
            return torch.zeros_like(self.smearing)
        return self.prefactor * math.pi**1.5 * (2 * self.smearing**2) ** (0.5 * (3 - p)) / ((3 - p) * math.gamma(0.5 * p))


    def pbc_correction(self, periodic, positions, cell, charges):
        """2-D slab term (reference ``potentials/coulomb.py:6-40,160-167``), non-zero when exactly two of ``periodic`` are
        True: ``(4 pi / V) (z_i M - (M2 + Q z_i^2) / 2 - Q L_z^2 / 12)`` with z along the non-periodic axis, Q, M, M2 the
        zeroth / first / second moments of the charges along it and L_z the length of that cell vector.  (The calculators
        evaluate the same expression in ``mipme_slab_forward``; this method is the inspectable tensor form.)"""
        if self._p != 1:  # the slab term exists for 1/r only (`potentials/inversepowerlaw.py:166-169`)
            return self.prefactor * torch.zeros_like(charges)
        if periodic is None:  # fully periodic: no term (and no device round trip to find that out)
            return self.prefactor * torch.zeros_like(charges)
        flags = [bool(v) for v in periodic.tolist()]
        if sum(flags) != 2:
            return self.prefactor * torch.zeros_like(charges)
        axis = flags.index(False)
        z = positions[:, axis : axis + 1]
        volume = torch.abs(torch.det(cell))
        Lz = torch.linalg.norm(cell[axis])
        Q, M, M2 = charges.sum(dim=0), (charges * z).sum(dim=0), (charges * z * z).sum(dim=0)
        return self.prefactor * (4 * math.pi / volume) * (z * M - 0.5 * (M2 + Q * z * z) - Q / 12.0 * Lz * Lz)


class InversePowerLawPotential(_PowerLawPotential):
    """1/r^p potential, p in 1..6 (reference ``potentials/inversepowerlaw.py:9-173``)."""

    _kind = _lib.INVERSE_POWER_LAW

    def __init__(
        self,
        exponent: int,
        smearing: float | None = None,
        exclusion_radius: float | None = None,
        exclusion_degree: int = 1,
        prefactor: float = 1.0,
    ):
        super().__init__(smearing, exclusion_radius, exclusion_degree, prefactor)
        if exponent not in (1, 2, 3, 4, 5, 6):
            raise ValueError(f"Unsupported exponent: {exponent}")
        self.register_buffer("exponent", torch.tensor(exponent, dtype=torch.float64))
        self._p = int(exponent)


class CoulombPotential(_PowerLawPotential):
    """Smoothed electrostatic 1/r potential (reference ``potentials/coulomb.py:43-171``)."""

    _kind = _lib.COULOMB
    _p = 1

    def __init__(
        self,
        smearing: float | None = None,
        exclusion_radius: float | None = None,
        exclusion_degree: int = 1,
        prefactor: float = 1.0,
    ):
        super().__init__(smearing, exclusion_radius, exclusion_degree, prefactor)


class SplinePotential(Potential):
    r"""Potential given as tables: a cubic spline of the real-space function and one of its Fourier-space kernel (reference
    ``potentials/spline.py:12-191``).  It is assumed to have a long-range part only -- ``sr_from_dist`` is zero; a subclass that
    redefines it with tensor operations adds a short-range part -- and to vanish at infinite separation.

    A calculator with a spline potential is evaluated through the differentiable primitives of :mod:`analytic` (spread,
    convolution, gather, pair sum), with the spline itself from ``csrc/spline.hip``: differentiable to any order w.r.t. charges,
    positions, cell and distances, at the cost of that route (a dozen launches, atomics in the spread) rather than that of the
    fused kernels, which do not know splines (:meth:`_descriptor` raises; no graph capture, no dispatcher op).

    Differences from the reference: the knot tables are float64 and the spline is evaluated in double precision, the result
    having the dtype of the argument (the reference evaluates in the dtype of the grids and promotes to it); with the
    ``sr_from_dist`` of this class the calculators skip the real-space pair sum instead of adding ``0 * d`` per pair, which
    differs only for non-finite distances.  The knot tables (grids, second derivatives) are detached float64 host copies of
    the buffers, made at construction and again after a buffer was written to: the spline is differentiable in its ARGUMENT
    to any order, but no gradient flows to ``y_grid`` / ``yhat_grid`` (the reference builds its second derivatives with
    tensor operations, so its tables can be learned in place; here a learned table is a new potential, or a
    ``load_state_dict``, per update).  As in the reference, ``from_dist`` applies the prefactor twice
    (``prefactor * (lr_from_dist + sr_from_dist)`` with ``lr_from_dist = prefactor * spline``).

    :param r_grid: radial grid of the real-space function
    :param y_grid: its values
    :param k_grid: radial grid of the k-space kernel; by default ``2 pi / r_grid`` (flipped) for a reciprocal-axis spline and
        ``r_grid`` otherwise
    :param yhat_grid: values of the k-space kernel; by default the Fourier transform of the spline
        (:func:`~splines.compute_spline_ft`)
    :param reciprocal: spline on a 1/r axis, for long-range functions; ``r_grid`` must be strictly positive
    :param y_at_zero: value for r -> 0 of a reciprocal-axis spline
    :param yhat_at_zero: value of the kernel for k -> 0
    :param smearing, exclusion_radius, exclusion_degree, prefactor: see :class:`Potential`
    """

    def __init__(
        self,
        r_grid: torch.Tensor,
        y_grid: torch.Tensor,
        k_grid: torch.Tensor | None = None,
        yhat_grid: torch.Tensor | None = None,
        reciprocal: bool | None = False,
        y_at_zero: float | None = None,
        yhat_at_zero: float | None = None,
        smearing: float | None = None,
        exclusion_radius: float | None = None,
        exclusion_degree: int = 1,
        prefactor: float = 1.0,
    ):
        super().__init__(smearing=smearing, exclusion_radius=exclusion_radius, exclusion_degree=exclusion_degree,
                         prefactor=prefactor)
        from . import splines

        if len(y_grid) != len(r_grid):
            raise ValueError("Length of radial grid and value array mismatch.")
        self.register_buffer("r_grid", r_grid)
        self.register_buffer("y_grid", y_grid)
        self._reciprocal = bool(reciprocal)
        if reciprocal and torch.min(r_grid) <= 0.0:
            raise ValueError("Positive-valued radial grid is needed for reciprocal axis spline.")
        if k_grid is None:
            if reciprocal:
                k_grid = torch.pi * 2 * torch.reciprocal(r_grid).flip(dims=[0])
            else:
                k_grid = r_grid.clone().detach()
        self.register_buffer("k_grid", k_grid)
        if yhat_grid is None:
            yhat_grid = splines.compute_spline_ft(k_grid, r_grid, y_grid, splines.compute_second_derivatives(r_grid, y_grid))
        self.register_buffer("yhat_grid", yhat_grid)
        self._y_at_zero_arg = None if y_at_zero is None else float(y_at_zero)
        self._yhat_at_zero_arg = None if yhat_at_zero is None else float(yhat_at_zero)
        self._tables_version = 0
        self._build_tables()

    # ---- the splines: host tables from the buffers, device copies made on first use (splines._Table) --------------------------
    def _buffers_key(self):
        return tuple((b.data_ptr(), b._version) for b in (self.r_grid, self.y_grid, self.k_grid, self.yhat_grid))

    def _build_tables(self):
        from . import splines

        d = self.__dict__
        if self._reciprocal:
            spline = splines.CubicSplineReciprocal(self.r_grid, self.y_grid, y_at_zero=self._y_at_zero_arg)
            krn = splines.CubicSplineReciprocal(self.k_grid**2, self.yhat_grid, y_at_zero=self._yhat_at_zero_arg)
        else:
            spline = splines.CubicSpline(self.r_grid, self.y_grid)
            krn = splines.CubicSpline(self.k_grid**2, self.yhat_grid)
        # (plain attributes: the splines hold no parameters or buffers, and state dicts stay those of the reference)
        d["_spline"], d["_krn_spline"] = spline, krn
        zero = torch.zeros(1, dtype=torch.float64)
        d["_y_at_zero"] = float(spline(zero)) if self._y_at_zero_arg is None else self._y_at_zero_arg
        d["_yhat_at_zero"] = float(krn(zero)) if self._yhat_at_zero_arg is None else self._yhat_at_zero_arg
        d["_tables_key"] = self._buffers_key()
        d["_tables_version"] = self._tables_version + 1
        d["_prefactor_cache"] = None

    def _splines(self):
        """(real-space spline, kernel spline), rebuilt when a buffer was written to (``load_state_dict``)."""
        if self._tables_key != self._buffers_key():
            self._build_tables()
        return self._spline, self._krn_spline

    def _apply(self, fn, *args, **kwargs):
        # buffers written to since the tables were built (load_state_dict, then .to(device)): rebuild from them first, while
        # they still have the dtype they were loaded in
        if self.__dict__.get("_tables_key") is not None and self._tables_key != self._buffers_key():
            self._build_tables()
        out = super()._apply(fn, *args, **kwargs)
        # the buffers moved (or changed dtype): the float64 host tables stay what they were built from, device copies of them
        # are made on the device of the arguments (splines._Table.tensor)
        self.__dict__["_tables_key"] = self._buffers_key()
        self.__dict__["_prefactor_cache"] = None
        return out

    def _prefactor_float(self) -> float:
        key = (self.prefactor.data_ptr(), self.prefactor._version)
        c = self.__dict__.get("_prefactor_cache")
        if c is None or c[0] != key:
            c = self.__dict__["_prefactor_cache"] = (key, float(self.prefactor))
        return c[1]

    def _descriptor(self):
        raise TypeError(
            f"{self.__class__.__name__} (a SplinePotential) has no fused HIP kernel: the descriptor-based entry points "
            "(graph capture, frame batches, live neighbour lists, the dispatcher op) do not serve it; call the calculator "
            "eagerly -- `calculator(charges, cell, positions, neighbor_indices, neighbor_distances)` -- which evaluates it "
            "through the differentiable primitives and `csrc/spline.hip`")

    def _own_sr(self) -> bool:
        """Whether ``sr_from_dist`` is this class's zero (the calculators then skip the pair sum)."""
        return type(self).sr_from_dist is SplinePotential.sr_from_dist

    # ---- reference method surface --------------------------------------------------------------------------------------------
    def from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        """``prefactor * (lr_from_dist + sr_from_dist)``: the prefactor enters twice, as in the reference."""
        return self.prefactor * (self.lr_from_dist(dist, pair_mask) + self.sr_from_dist(dist, pair_mask))

    def sr_from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        return 0.0 * dist

    def lr_from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        return self.prefactor.to(dist.device) * self._splines()[0](dist)

    def lr_from_k_sq(self, k_sq: torch.Tensor) -> torch.Tensor:
        return self.prefactor.to(k_sq.device) * self._splines()[1](k_sq)

    def self_contribution(self) -> torch.Tensor:
        self._splines()
        return self.prefactor * self._y_at_zero

    def background_correction(self) -> torch.Tensor:
        return self.prefactor * torch.zeros(1, device=self.prefactor.device)


class CombinedPotential(Potential):
    r"""Weighted sum :math:`\sum_t w_t v_t` of potentials, the weights fixed or learnable (reference
    ``potentials/combined.py:6-124``): every method is the weighted sum of the members' methods; ``pbc_correction`` is the base
    class's zero, as in the reference -- a combination has no slab term even with a Coulomb member.

    A calculator with a combined potential is evaluated through the differentiable primitives of :mod:`analytic`, whatever its
    ``double_backward`` says: differentiable to any order w.r.t. charges, positions, cell, distances and the weights, in ONE
    mesh pass and ONE pair sum for all members.  Where every member is exactly a :class:`CoulombPotential` or an
    :class:`InversePowerLawPotential` without an exclusion radius, and there are at most 8 of them, the members' pair functions
    (to any derivative order up to 6) and filter tables come from ``csrc/combined.hip`` (see :mod:`combined`).  Any other
    combination -- a :class:`SplinePotential` member, a nested combination, a member with an exclusion radius, a subclass,
    more than 8 terms -- goes through the members' tensor methods, as any unknown :class:`Potential` does: correct, and slower.
    The fused kernels take one potential and do not serve a combination (:meth:`_descriptor` raises; no graph capture, no
    frame batches, no live neighbour lists, no dispatcher op).

    Difference from the reference: the weights are cast to the dtype of the argument (the reference requires
    ``weights.dtype`` to be the dtype of the computation: ``torch.inner`` raises otherwise).

    :param potentials: the members; all range separated (``smearing`` set) or all direct
    :param initial_weights: one weight per member; ones by default
    :param learnable_weights: ``True``: ``weights`` is a ``Parameter``; ``False``: a buffer
    :param smearing: must be given exactly when the members are range separated (its value only tells the calculators that
        there is a long-range part)
    :param exclusion_radius, exclusion_degree: see :class:`Potential`
    """

    def __init__(
        self,
        potentials: list[Potential],
        initial_weights: torch.Tensor | None = None,
        learnable_weights: bool | None = True,
        smearing: float | None = None,
        exclusion_radius: float | None = None,
        exclusion_degree: int = 1,
    ):
        super().__init__(smearing=smearing, exclusion_radius=exclusion_radius, exclusion_degree=exclusion_degree)
        smearings = [pot.smearing for pot in potentials]
        if not all(smearings) and any(smearings):
            raise ValueError(
                r"Cannot combine direct (`smearing=None`) and range-separated (`smearing=float`) potentials."
            )
        if all(smearings) and not self.smearing:
            raise ValueError(
                r"You should specify a `smearing` when combining range-separated (`smearing=float`) potentials."
            )
        if not any(smearings) and self.smearing:
            raise ValueError(
                r"Cannot specify `smearing` when combining direct (`smearing=None`) potentials."
            )
        if initial_weights is not None:
            if len(initial_weights) != len(potentials):
                raise ValueError(
                    "The number of initial weights must match the number of potentials being combined"
                )
        else:
            initial_weights = torch.ones(len(potentials))
        self.potentials = torch.nn.ModuleList(potentials)
        if learnable_weights:
            self.weights = torch.nn.Parameter(initial_weights)
        else:
            self.register_buffer("weights", initial_weights)

    def _descriptor(self):
        raise TypeError(
            f"{self.__class__.__name__} (a CombinedPotential) has no fused HIP kernel: the descriptor-based entry points "
            "(graph capture, frame batches, live neighbour lists, the dispatcher op) take one potential and do not serve a "
            "combination; call the calculator eagerly -- `calculator(charges, cell, positions, neighbor_indices, "
            "neighbor_distances)` -- which evaluates it through the differentiable primitives and `csrc/combined.hip`")

    def _weighted(self, values: list) -> torch.Tensor:
        stacked = torch.stack(values, dim=-1)
        return torch.inner(self.weights.to(dtype=stacked.dtype, device=stacked.device), stacked)

    # ---- reference method surface --------------------------------------------------------------------------------------------
    def from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        return self._weighted([pot.from_dist(dist, pair_mask) for pot in self.potentials])

    def sr_from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        return self._weighted([pot.sr_from_dist(dist, pair_mask) for pot in self.potentials])

    def lr_from_dist(self, dist: torch.Tensor, pair_mask: torch.Tensor | None = None) -> torch.Tensor:
        return self._weighted([pot.lr_from_dist(dist, pair_mask) for pot in self.potentials])

    def lr_from_k_sq(self, k_sq: torch.Tensor) -> torch.Tensor:
        return self._weighted([pot.lr_from_k_sq(k_sq) for pot in self.potentials])

    def self_contribution(self) -> torch.Tensor:
        # (scalars of shape () or (1,), depending on the member's class: stacked as scalars)
        return self._weighted([pot.self_contribution().reshape(()) for pot in self.potentials])

    def background_correction(self) -> torch.Tensor:
        return self._weighted([pot.background_correction().reshape(()) for pot in self.potentials])
