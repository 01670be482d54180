"""Device side of :class:`~potentials.CombinedPotential`: the members' pair functions and filter tables from
``csrc/combined.hip``, for the combinations its kernels serve.

A combination is served (:func:`plan`) when every member is exactly a :class:`~potentials.CoulombPotential` or an
:class:`~potentials.InversePowerLawPotential` (no subclass) without an exclusion radius, the members are all range separated or
all direct, and there are at most 8 of them.  Anything else -- a spline member, a nested combination, a member with an exclusion
radius, a subclass, more terms -- is evaluated by the callers through the members' tensor methods.

* :class:`_TermValues` is the ``order``-th derivative w.r.t. the distance of every member's short-range pair function,
  ``(n_terms, n_pairs)``, in one pass over the distances (``mipme_combined_sr_eval``); its backward is the same node one order
  up, so the pair part is differentiable to order 6 in the distances (the library's ``MIPME_COMBINED_MAX_ORDER``).
* :class:`_WeightedValues` is the weighted sum ``(n_pairs,)`` from the same kernel with the weights read on the device: used
  when the weights need no gradient, so that no ``(n_terms, n_pairs)`` tensor is kept alive without need.
* :func:`pair_values` picks between them: weights that need a gradient take ``einsum('t,tp->p', w, terms)`` (written as a
  broadcast product and a sum) and autograd supplies dL/dw.
* :func:`build_tables` fills the members' filter tables G_t(k), ``(n_terms, nx, ny, nz/2+1)``, in one launch
  (``mipme_combined_kfilter_build``).  The callers cache them per cell and contract them with the weights per call, so a step
  of an optimizer on the weights invalidates nothing.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MAX_TERMS = _lib.COMBINED_MAX_TERMS
MAX_ORDER = _lib.COMBINED_MAX_ORDER


class Plan:
    """``mipme_combined_t`` of a served combination and the key of its members' parameters."""

    def __init__(self, key, desc):
        self.key, self.desc = key, desc
        self.n_terms = desc.n_terms


def plan(pot) -> Plan | None:
    """The :class:`Plan` of a combination the kernels serve, ``None`` for every other potential (cached on the potential per
    parameter set: the members' parameters are read through their own host caches, one device copy per parameter set)."""
    from .potentials import CombinedPotential, CoulombPotential, InversePowerLawPotential

    if not isinstance(pot, CombinedPotential):
        return None
    members = list(pot.potentials)
    if not 1 <= len(members) <= MAX_TERMS:
        return None
    if any(type(m) not in (CoulombPotential, InversePowerLawPotential) or m.exclusion_radius is not None for m in members):
        return None
    smeared = [m.smearing is not None for m in members]
    if any(smeared) != all(smeared):  # (the constructor refuses this; a member replaced afterwards)
        return None
    key = tuple((type(m)._kind,) + tuple(m._host_params()) for m in members)
    cached = pot.__dict__.get("_plan_cache")
    if cached is not None and cached.key == key:
        return cached
    desc = _lib.CombinedDesc(n_terms=len(members))
    for t, (kind, sm, pref, p) in enumerate(key):
        desc.terms[t] = _lib.PotentialDesc(kind=kind, exponent=p, smearing=-1.0 if sm is None else sm, prefactor=pref,
                                           exclusion_radius=-1.0, exclusion_degree=1)
    cached = pot.__dict__["_plan_cache"] = Plan(key, desc)
    return cached


def _launch(plan_, order, d, weights):
    dc = d.detach().contiguous()
    if dc.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"combined potentials are evaluated on float32 and float64 tensors, got {dc.dtype}")
    shape = dc.shape if weights is not None else (plan_.n_terms,) + tuple(dc.shape)
    out = torch.empty(shape, dtype=dc.dtype, device=dc.device)
    wc = None if weights is None else weights.detach().to(device=dc.device, dtype=dc.dtype).contiguous()
    with _lib.on_device(dc.device):
        _lib.check(_lib.load().mipme_combined_sr_eval(_lib.current_stream(dc.device), _lib.dtype_code(dc.dtype),
                                                      C.byref(plan_.desc), order, None, dc.numel(), dc.data_ptr(), _lib.ptr(wc),
                                                      out.data_ptr()))
    return out


class _TermValues(torch.autograd.Function):
    """``v_t^(order)(d)`` of every term, ``(n_terms, ...)``; the backward is the same node at ``order + 1``."""

    @staticmethod
    def forward(ctx, d, plan_, order):
        ctx.save_for_backward(d)
        ctx.plan, ctx.order = plan_, order
        return _launch(plan_, order, d, None)

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return (g * _TermValues.apply(d, ctx.plan, ctx.order + 1)).sum(dim=0), None, None


class _WeightedValues(torch.autograd.Function):
    """``sum_t w_t v_t^(order)(d)`` with constant weights; the backward is the same node at ``order + 1``."""

    @staticmethod
    def forward(ctx, d, weights, plan_, order):
        ctx.save_for_backward(d, weights)
        ctx.plan, ctx.order = plan_, order
        return _launch(plan_, order, d, weights)

    @staticmethod
    def backward(ctx, g):
        d, weights = ctx.saved_tensors
        return g * _WeightedValues.apply(d, weights, ctx.plan, ctx.order + 1), None, None, None


def pair_values(pot, plan_: Plan, dist: torch.Tensor) -> torch.Tensor:
    """``sum_t w_t v_t(dist)``: ``sr_from_dist`` of a range-separated combination, ``from_dist`` of a direct one (without pair
    mask and exclusion: the callers multiply)."""
    w = pot.weights
    if w.requires_grad and torch.is_grad_enabled():
        # einsum('t,tp->p', w, terms) as a broadcast product and a sum: einsum hands this shape (T x P, T a handful) to a
        # matrix-vector routine; both forms are timed in tools/time_combined.py, section 3
        terms = _TermValues.apply(dist, plan_, 0)
        wd = w.to(dtype=dist.dtype, device=dist.device)
        return (wd.reshape((-1,) + (1,) * dist.dim()) * terms).sum(dim=0)
    return _WeightedValues.apply(dist, w.detach(), plan_, 0)


def build_tables(geom, plan_: Plan, dtype, device) -> torch.Tensor:
    """G_t(k) of every member (/ U^2 for P3M) on the rfft half grid of ``geom``: ``(n_terms, nx, ny, nz/2+1)``."""
    out = torch.empty((plan_.n_terms, geom.ns[0], geom.ns[1], geom.ns[2] // 2 + 1), dtype=dtype, device=device)
    md = geom.desc(1)
    with _lib.on_device(device):
        _lib.check(_lib.load().mipme_combined_kfilter_build(_lib.current_stream(device), _lib.dtype_code(dtype), C.byref(md),
                                                            C.byref(plan_.desc), out.data_ptr()))
    return out


def coefficients(plan_: Plan, order: int):
    """The coefficients of R_order per member, lowest power first, as the library forms them (no device needed)."""
    buf = (C.c_double * (plan_.n_terms * MAX_ORDER))()
    _lib.check(_lib.load().mipme_combined_sr_eval(None, _lib.F64, C.byref(plan_.desc), order, buf, 0, None, None, None))
    return [list(buf[t * MAX_ORDER:(t + 1) * MAX_ORDER]) for t in range(plan_.n_terms)]
