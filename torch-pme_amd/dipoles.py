"""Point dipoles: :class:`PotentialDipole` and :class:`CalculatorDipole` (reference ``potentials/potential_dipole.py``,
``calculators/calculator_dipole.py``).

Same constructor signatures, buffer names, method names, exceptions and ``_compute_rspace`` / ``_compute_kspace`` as the
reference.  The calculator runs on HIP kernels (``csrc/dipole.hip``): the real-space pair sum of the dipolar tensor with a
thread per pair, and the explicit reciprocal-space sum without the reference's (2, K, N) phase tables.  The 1/V factor,
the self and background terms and the k-vector generation are small tensor ops here, so the cell gradient is autograd's.
Gradients are first order (dipoles, positions, cell, neighbor vectors); only CUDA tensors are accepted.

The elementwise :class:`PotentialDipole` methods are plain tensor expressions for inspection; they run on any device.
"""

from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._utils import _validate_parameters
from .calculators import _integer_frequencies, _reciprocal_and_det
from .ops import _call, first_order

DIPOLE_SECOND_ORDER_HINT = (
    "torchpme_amd: dipole calculators are first order in this build: CalculatorDipole gives gradients with respect to "
    "dipoles, positions, cell and neighbor_vectors, but a gradient computed with create_graph=True cannot be "
    "differentiated again."
)


def _first_order(fn):
    return first_order(fn, DIPOLE_SECOND_ORDER_HINT)


class PotentialDipole(torch.nn.Module):
    r"""Pair interaction of point dipoles, :math:`V = \mu_i^T T(\mathbf r) \mu_j` with
    :math:`T = (I / r^3 - 3 \mathbf r \mathbf r^T / r^5)` times ``prefactor`` (reference ``potential_dipole.py``).

    :param smearing: width ``sigma`` of the Gaussian that splits the interaction into short- and long-range parts
        (``None``: no split, real space only)
    :param exclusion_radius: radius inside which the long-range part is smoothly switched off
    :param exclusion_degree: exponent of the raised-cosine switch
    :param epsilon: dielectric constant of the surrounding medium (background term; 0: none)
    :param prefactor: multiplicative prefactor (see :mod:`prefactors`)
    """

    def __init__(
        self,
        smearing: float | None = None,
        exclusion_radius: float | None = None,
        exclusion_degree: int = 1,
        epsilon: float = 0.0,
        prefactor: float = 1.0,
    ):
        super().__init__()
        self.exclusion_degree = exclusion_degree
        if smearing is not None:
            self.register_buffer("smearing", torch.tensor(smearing, dtype=torch.float64))
        else:
            self.smearing = None
        if exclusion_radius is not None:
            self.register_buffer("exclusion_radius", torch.tensor(exclusion_radius, dtype=torch.float64))
        else:
            self.exclusion_radius = None
        self.register_buffer("epsilon", torch.tensor(epsilon, dtype=torch.float64))
        self.register_buffer("prefactor", torch.tensor(prefactor, dtype=torch.float64))
        self._host_cache = None

    # ---- host-side view of the parameters (buffers may live on the device) -------------------
    def _host_params(self):
        """(smearing|None, exclusion_radius|None, epsilon, prefactor) as Python floats; one D2H copy each, then cached."""

        def key(t):
            return None if t is None else (t.data_ptr(), t._version)

        k = (key(self.smearing), key(self.exclusion_radius), key(self.epsilon), key(self.prefactor), self.exclusion_degree)
        if self._host_cache is None or self._host_cache[0] != k:
            sm = None if self.smearing is None else float(self.smearing)
            rx = None if self.exclusion_radius is None else float(self.exclusion_radius)
            self._host_cache = (k, sm, rx, float(self.epsilon), float(self.prefactor))
        return self._host_cache[1:]

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_host_cache"] = None
        return state

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._host_cache = None
        return out

    def _descriptor(self) -> _lib.DipoleDesc:
        """``mipme_dipole_t`` of the real-space pair kernels."""
        sm, rx, _, pref = self._host_params()
        return _lib.DipoleDesc(
            smearing=-1.0 if sm is None else sm,
            prefactor=pref,
            exclusion_radius=-1.0 if rx is None else rx,
            exclusion_degree=int(self.exclusion_degree),
        )

    def _coulomb_descriptor(self) -> _lib.PotentialDesc:
        """The reciprocal-space kernel 4 pi prefactor exp(-sigma^2 k^2 / 2) / k^2 is Coulomb's: ``mipme_ewald_filter``."""
        sm, _, _, pref = self._host_params()
        return _lib.PotentialDesc(kind=_lib.COULOMB, exponent=1, smearing=sm, prefactor=pref, exclusion_radius=-1.0,
                                  exclusion_degree=1)

    # ---- reference method surface ------------------------------------------------------------
    def f_cutoff(self, vector: torch.Tensor) -> torch.Tensor:
        r"""Raised-cosine switch :math:`1 - ((1 - \cos \pi r / r_\mathrm{ex}) / 2)^n` inside ``exclusion_radius``, 0
        beyond; shape (P, 1).

        :param vector: (P, 3) pair vectors
        """
        r = torch.norm(vector, dim=1, keepdim=True)
        if self.exclusion_radius is None:
            raise ValueError("Cannot compute cutoff function when `exclusion_radius` is not set")
        h = 0.5 * (1 - torch.cos(torch.pi * (r / self.exclusion_radius)))
        return torch.where(r < self.exclusion_radius, 1 - h**self.exclusion_degree, 0.0)

    @staticmethod
    def _tensor(vector: torch.Tensor, B: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
        """(P, 3, 3) ``B I - C r r^T`` from (P, 1) coefficients."""
        eye = torch.eye(3, dtype=vector.dtype, device=vector.device)
        outer = vector.unsqueeze(2) * vector.unsqueeze(1)
        return B.unsqueeze(-1) * eye - C.unsqueeze(-1) * outer

    def _split_terms(self, vector: torch.Tensor):
        """(r, alpha, erf(sqrt(alpha) r), erfc(...), 2 sqrt(alpha/pi) exp(-alpha r^2)) of the range-separated forms."""
        alpha = 1 / (2 * self.smearing**2)
        r = torch.norm(vector, dim=1, keepdim=True)
        y = torch.sqrt(alpha) * r
        ke = 2 * torch.sqrt(alpha / torch.pi) * torch.exp(-alpha * r**2)
        return r, alpha, torch.erf(y), torch.erfc(y), ke

    def from_dist(self, vector: torch.Tensor) -> torch.Tensor:
        """Bare dipolar tensor ``prefactor (I / r^3 - 3 r r^T / r^5)``, shape (P, 3, 3).

        :param vector: (P, 3) pair vectors
        """
        r = torch.norm(vector, dim=1, keepdim=True)
        return self.prefactor * self._tensor(vector, 1.0 / r**3, 3.0 / r**5)

    def sr_from_dist(self, dist: torch.Tensor) -> torch.Tensor:
        """Short-range part, shape (P, 3, 3): ``from_dist - lr_from_dist`` (evaluated in its erfc form), or
        ``-lr_from_dist * f_cutoff`` when an exclusion radius is set.

        :param dist: (P, 3) pair vectors
        """
        if self.smearing is None:
            raise ValueError("Cannot compute range-separated potential when `smearing` is not specified.")
        if self.exclusion_radius is not None:
            return -self.lr_from_dist(dist) * self.f_cutoff(dist).unsqueeze(-1)
        r, alpha, _, erfc, ke = self._split_terms(dist)
        B = erfc / r**3 + ke / r**2
        C = 3.0 * erfc / r**5 + ke * (2 * alpha + 3 / r**2) / r**2
        return self.prefactor * self._tensor(dist, B, C)

    def lr_from_dist(self, dist: torch.Tensor) -> torch.Tensor:
        """Long-range part of the range-separated tensor, shape (P, 3, 3).

        :param dist: (P, 3) pair vectors
        """
        if self.smearing is None:
            raise ValueError("Cannot compute long-range contribution without specifying `smearing`.")
        r, alpha, erf, _, ke = self._split_terms(dist)
        B = erf / r**3 - ke / r**2
        C = 3.0 * erf / r**5 - ke * (2 * alpha + 3 / r**2) / r**2
        return self.prefactor * self._tensor(dist, B, C)

    def lr_from_k_sq(self, k_sq: torch.Tensor) -> torch.Tensor:
        """Fourier transform of the long-range part, ``prefactor 4 pi exp(-sigma^2 k^2 / 2) / k^2``, 0 at k = 0.

        :param k_sq: squared norms of the wave vectors
        """
        if self.smearing is None:
            raise ValueError("Cannot compute long-range kernel without specifying `smearing`.")
        masked = torch.where(k_sq == 0, 1.0, k_sq)  # no NaN in the backward pass through the k = 0 branch
        return self.prefactor * torch.where(
            k_sq == 0, 0.0, 4 * torch.pi * torch.exp(-0.5 * self.smearing**2 * masked) / masked
        )

    def self_contribution(self) -> torch.Tensor:
        """Self-interaction ``prefactor 4 pi / 3 (alpha / pi)^(3/2)`` that the reciprocal-space sum includes."""
        if self.smearing is None:
            raise ValueError("Cannot compute long-range contribution without specifying `smearing`.")
        alpha = 1 / (2 * self.smearing**2)
        return self.prefactor * 4 * torch.pi / 3 * torch.sqrt((alpha / torch.pi) ** 3)

    def background_correction(self, volume) -> torch.Tensor:
        """Surface term of a dielectric background, ``prefactor 4 pi / (2 epsilon + 1) / volume`` (0 when epsilon = 0)."""
        if self.epsilon == 0.0:
            return self.epsilon
        return self.prefactor * 4 * torch.pi / (2 * self.epsilon + 1) / volume


class _DipoleRSpace(torch.autograd.Function):
    """``V_i = 1/2 sum_j T(r_ij) mu_j`` over the pair list (``mipme_dipole_rspace_forward``); differentiable w.r.t. the
    dipoles and the pair vectors."""

    @staticmethod
    def forward(ctx, dipoles, vectors, indices, desc, full):
        lib = _lib.load()
        device, dtype = dipoles.device, dipoles.dtype
        mu, vec, idx = dipoles.detach().contiguous(), vectors.detach().contiguous(), indices.contiguous()
        out = torch.empty_like(mu)
        with _lib.on_device(device):
            _call("dipole_rspace", lib.mipme_dipole_rspace_forward, _lib.current_stream(device), _lib.dtype_code(dtype),
                  _lib.index_code(idx.dtype), mu.shape[0], idx.shape[0], int(full), idx.data_ptr(), vec.data_ptr(),
                  mu.data_ptr(), C.byref(desc), out.data_ptr())
        ctx.save_for_backward(mu, vec, idx)
        ctx.desc, ctx.full = desc, full
        return out

    @staticmethod
    @_first_order
    def backward(ctx, grad_out):
        lib = _lib.load()
        mu, vec, idx = ctx.saved_tensors
        need_mu, need_vec = ctx.needs_input_grad[:2]
        if not (need_mu or need_vec):
            return None, None, None, None, None
        device = mu.device
        g = grad_out.contiguous()
        grad_mu = torch.empty_like(mu) if need_mu else None
        grad_vec = torch.empty_like(vec) if need_vec else None
        with _lib.on_device(device):
            _call("dipole_rspace_backward", lib.mipme_dipole_rspace_backward, _lib.current_stream(device),
                  _lib.dtype_code(mu.dtype), _lib.index_code(idx.dtype), mu.shape[0], idx.shape[0], int(ctx.full),
                  idx.data_ptr(), vec.data_ptr(), mu.data_ptr(), g.data_ptr(), C.byref(ctx.desc), _lib.ptr(grad_mu),
                  _lib.ptr(grad_vec))
        return grad_mu, grad_vec, None, None, None


class _DipoleKSpace(torch.autograd.Function):
    """``E_i = sum_k G(k) k [cos(k r_i) S_c(k) + sin(k r_i) S_s(k)]``, ``S_c(k) = sum_j (mu_j . k) cos(k r_j)`` (and
    ``S_s`` with sin): the reciprocal-space sum of ``CalculatorDipole._compute_kspace`` without the 1/V factor.
    Differentiable w.r.t. dipoles, positions and the k-vectors (through which the cell gradient flows)."""

    @staticmethod
    def forward(ctx, dipoles, positions, kvectors, coulomb_desc):
        lib = _lib.load()
        device, dtype = positions.device, positions.dtype
        dt = _lib.dtype_code(dtype)
        mu, pos, kv = dipoles.detach().contiguous(), positions.detach().contiguous(), kvectors.detach().contiguous()
        N, K = pos.shape[0], kv.shape[0]
        G = torch.empty(K, dtype=dtype, device=device)
        dG = torch.empty(K, dtype=dtype, device=device)
        Sc = torch.empty(K, dtype=dtype, device=device)
        Ss = torch.empty(K, dtype=dtype, device=device)
        out = torch.empty((N, 3), dtype=dtype, device=device)
        partials = _partials(N, K, dtype, device)
        with _lib.on_device(device):
            st = _lib.current_stream(device)
            _call("ewald_filter", lib.mipme_ewald_filter, st, dt, C.byref(coulomb_desc), K, kv.data_ptr(), G.data_ptr(),
                  dG.data_ptr())
            _call("dipole_structure", lib.mipme_dipole_structure, st, dt, N, K, pos.data_ptr(), mu.data_ptr(),
                  kv.data_ptr(), G.data_ptr(), dG.data_ptr(), Sc.data_ptr(), Ss.data_ptr())
            _call("dipole_field", lib.mipme_dipole_field, st, dt, N, K, pos.data_ptr(), kv.data_ptr(), G.data_ptr(),
                  Sc.data_ptr(), Ss.data_ptr(), out.data_ptr(), _lib.ptr(partials))
        ctx.save_for_backward(mu, pos, kv, G, dG, Sc, Ss)
        return out

    @staticmethod
    @_first_order
    def backward(ctx, grad_out):
        lib = _lib.load()
        mu, pos, kv, G, dG, Sc, Ss = ctx.saved_tensors
        need_mu, need_pos, need_k = ctx.needs_input_grad[:3]
        if not (need_mu or need_pos or need_k):
            return None, None, None, None
        device, dtype = pos.device, pos.dtype
        dt = _lib.dtype_code(dtype)
        N, K = pos.shape[0], kv.shape[0]
        g = grad_out.contiguous()
        Tc, Ts = torch.empty_like(Sc), torch.empty_like(Ss)
        grad_mu = torch.empty_like(mu) if need_mu else None
        grad_pos = torch.empty_like(pos) if need_pos else None
        grad_k = torch.empty_like(kv) if need_k else None
        partials = _partials(N, K, dtype, device) if (need_mu or need_pos) else None
        with _lib.on_device(device):
            st = _lib.current_stream(device)
            _call("dipole_structure", lib.mipme_dipole_structure, st, dt, N, K, pos.data_ptr(), g.data_ptr(),
                  kv.data_ptr(), G.data_ptr(), dG.data_ptr(), Tc.data_ptr(), Ts.data_ptr())
            if need_mu:  # the sum is symmetric in (mu, g): the field of the structure factors of g
                _call("dipole_field", lib.mipme_dipole_field, st, dt, N, K, pos.data_ptr(), kv.data_ptr(), G.data_ptr(),
                      Tc.data_ptr(), Ts.data_ptr(), grad_mu.data_ptr(), _lib.ptr(partials))
            if need_pos or need_k:
                _call("dipole_backward", lib.mipme_dipole_backward, st, dt, N, K, pos.data_ptr(), mu.data_ptr(),
                      g.data_ptr(), kv.data_ptr(), G.data_ptr(), dG.data_ptr(), Sc.data_ptr(), Ss.data_ptr(),
                      Tc.data_ptr(), Ts.data_ptr(), _lib.ptr(grad_pos), _lib.ptr(grad_k), _lib.ptr(partials))
        return grad_mu, grad_pos, grad_k, None


def _partials(N: int, K: int, dtype, device):
    """Scratch of the k-sliced per-atom kernels (None when they need none)."""
    n = int(_lib.load().mipme_dipole_partials_size(N, K))
    return torch.empty(n, dtype=dtype, device=device) if n > 0 else None


class CalculatorDipole(torch.nn.Module):
    r"""Interacting point dipoles: ``V_i = 1/2 sum_j T(r_ij) mu_j`` in real space, plus the explicit reciprocal-space
    (Ewald) sum when the potential has a ``smearing`` (reference ``calculators/calculator_dipole.py``).  Returns the (N, 3)
    "potential" V; the energy is ``(V * dipoles).sum()``.

    :param potential: a :class:`PotentialDipole`
    :param full_neighbor_list: whether the pairs come from a full (True) or half (False) neighbor list
    :param lr_wavelength: spatial resolution of the reciprocal-space sum (set exactly when ``smearing`` is)
    """

    def __init__(self, potential: PotentialDipole, full_neighbor_list: bool = False, lr_wavelength: float | None = None):
        super().__init__()
        if not isinstance(potential, PotentialDipole):
            raise TypeError(f"Potential must be an instance of PotentialDipole, got {type(potential)}")
        self.potential = potential
        self.lr_wavelength = lr_wavelength
        assert (self.lr_wavelength is not None and self.potential.smearing is not None) or (
            self.lr_wavelength is None and self.potential.smearing is None
        ), "Either both `lr_wavelength` and `smearing` must be set or both must be None"
        self.full_neighbor_list = full_neighbor_list
        self._freq_cache = None  # see calculators._integer_frequencies

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_freq_cache"] = None  # holds a weak reference
        return state

    def _compute_rspace(self, dipoles: torch.Tensor, neighbor_indices: torch.Tensor,
                        neighbor_vectors: torch.Tensor) -> torch.Tensor:
        """Real-space pair sum, (N, 3): the bare tensor without ``smearing``, its short-range part with it."""
        _lib.require_device(dipoles, "dipoles")
        return _DipoleRSpace.apply(dipoles, neighbor_vectors, neighbor_indices, self.potential._descriptor(),
                                   bool(self.full_neighbor_list))

    def _compute_kspace(self, dipoles: torch.Tensor, cell: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """Reciprocal-space sum, (N, 3), with the self and background terms."""
        _lib.require_device(positions, "positions")
        sm, _, eps, pref = self.potential._host_params()
        recip, det = _reciprocal_and_det(cell)
        freq, self._freq_cache = _integer_frequencies(cell, self.lr_wavelength, self._freq_cache)
        kvectors = (2 * math.pi) * freq @ recip  # k = 2 pi F A^-T, differentiable w.r.t. the cell
        volume = torch.abs(det)
        field = _DipoleKSpace.apply(dipoles, positions, kvectors, self.potential._coulomb_descriptor()) / volume
        alpha = 0.5 / sm**2
        field = field - dipoles * (pref * 4 * math.pi / 3 * (alpha / math.pi) ** 1.5)
        if eps != 0.0:
            field = field + (pref * 4 * math.pi / (2 * eps + 1)) / volume * dipoles.sum(dim=0)
        return field / 2

    def forward(self, dipoles: torch.Tensor, cell: torch.Tensor, positions: torch.Tensor,
                neighbor_indices: torch.Tensor, neighbor_vectors: torch.Tensor) -> torch.Tensor:
        """The (N, 3) dipolar "potential" V of every atom.

        :param dipoles: (N, 3) atomic dipoles
        :param cell: (3, 3) cell, rows are the lattice vectors
        :param positions: (N, 3) Cartesian positions
        :param neighbor_indices: (P, 2) atom pairs (i, j)
        :param neighbor_vectors: (P, 3) pair vectors ``r_j - r_i`` (plus the periodic shift)
        """
        _validate_parameters(
            charges=dipoles,
            cell=cell,
            positions=positions,
            neighbor_indices=neighbor_indices,
            neighbor_distances=neighbor_vectors.norm(dim=-1),
        )
        if neighbor_vectors.dim() != 2 or neighbor_vectors.shape[1] != 3:
            raise ValueError(
                f"`neighbor_vectors` must be a tensor with shape [num_neighbors, 3], got tensor with shape "
                f"{list(neighbor_vectors.shape)}"
            )
        if dipoles.shape[1] != 3:
            raise ValueError(f"`dipoles` must be a tensor with shape [n_atoms, 3], got tensor with shape {list(dipoles.shape)}")
        _lib.require_device(positions, "positions")
        potential = self._compute_rspace(dipoles, neighbor_indices, neighbor_vectors)
        if self.potential.smearing is None:
            return potential
        return potential + self._compute_kspace(dipoles, cell, positions)
