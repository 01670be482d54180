"""ctypes binding of ``libmipme.so`` (C-ABI declared in ``include/mipme.h``).

There is deliberately NO fallback: if the HIP library is missing or a call fails, the product
path raises.  ``import torch`` happens before the ``dlopen`` so that ``libamdhip64.so.7`` /
``libhipfft.so.0`` resolve to the copies PyTorch already loaded (one HIP runtime per process, so
``torch.cuda.current_stream().cuda_stream`` is a valid ``hipStream_t`` for the library).
"""

from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIPME_LIB", os.path.join(_HERE, "libmipme.so"))  # MIPME_LIB: alternative build (experiments)

F32, F64 = 0, 1
I64, I32 = 0, 1
LAGRANGE, P3M = 0, 1
COULOMB, INVERSE_POWER_LAW = 0, 1

EXPORTS = (
    "mipme_last_error", "mipme_version", "mipme_fft_plan_create", "mipme_fft_plan_destroy", "mipme_kfilter_build",
    "mipme_convolve", "mipme_spread", "mipme_gather", "mipme_kspace_forward", "mipme_kspace_backward",
    "mipme_cellgrad_partials_size", "mipme_slab_forward", "mipme_slab_backward", "mipme_rspace_forward",
    "mipme_rspace_backward", "mipme_pair_distance_forward", "mipme_pair_distance_backward",
    "mipme_pair_partials_size", "mipme_topology_workspace_bytes", "mipme_topology_build", "mipme_topology_pack_shifts",
    "mipme_rspace_rows", "mipme_rspace_rows_value_bytes", "mipme_rspace_rows_tabulate", "mipme_rspace_rows_tabulated", "mipme_pair_distance_backward_rows", "mipme_rows_partials_size", "mipme_atom_bins_bytes", "mipme_plane_spread_parts", "mipme_last_cosched_kernel", "mipme_last_slot_fill", "mipme_last_cell_riders", "mipme_last_gather_pairs", "mipme_last_inverse_split", "mipme_frames_counter_ints",
    "mipme_profile_enable", "mipme_profile_report", "mipme_dot_forward", "mipme_dot_backward", "mipme_energy_log_push", "mipme_frames_table_energy_log",
    "mipme_nl_workspace_bytes", "mipme_nl_bin", "mipme_nl_count", "mipme_nl_fill", "mipme_nl_stream",
    "mipme_topology_pack_entries", "mipme_sr_rows_fused", "mipme_sr_rows_finalize",
    "mipme_pack_pair_shifts", "mipme_pair_distance_forward_packed", "mipme_fft_plan_xfused", "mipme_fft_plan_kgrid_blocks", "mipme_fft_r2c",
    "mipme_ewald_filter", "mipme_ewald_structure", "mipme_ewald_potential", "mipme_ewald_backward",
    "mipme_frames_table_bytes", "mipme_frames_table_build", "mipme_frames_forward", "mipme_frames_backward",
    "mipme_frames_cell_work", "mipme_frames_table_contract", "mipme_frames_step",
    "mipme_frames_slab_work", "mipme_frames_table_slab", "mipme_frames_slab_step",
    "mipme_frames_table_cells", "mipme_frames_cells", "mipme_frames_cell_geometry",
    "mipme_scaled_match", "mipme_scaled_match_work", "mipme_scaled_match_wide", "mipme_md_supported", "mipme_md_lists_ints", "mipme_md_rebin", "mipme_md_step", "mipme_set_skip_flag", "mipme_energy_select", "mipme_energy_select_sum", "mipme_energy_select_contract",
    "mipme_kfilter_build_deriv", "mipme_cell_tail_work", "mipme_values_equal", "mipme_checksum", "mipme_checksum_words",
    "mipme_spread_jet", "mipme_gather_jet", "mipme_gather_jet3", "mipme_pair_sum", "mipme_pair_sum_rows", "mipme_pair_dot", "mipme_pair_diff", "mipme_pair_scatter",
    "mipme_dipole_rspace_forward", "mipme_dipole_rspace_backward", "mipme_dipole_partials_size", "mipme_dipole_structure",
    "mipme_dipole_field", "mipme_dipole_backward",
    "mipme_spline_eval", "mipme_spline_eval_reciprocal", "mipme_spline_kfilter_build",
    "mipme_combined_sr_eval", "mipme_combined_kfilter_build",
    "mipme_combined_step", "mipme_combined_step_work",
    "mipme_dipole_step", "mipme_dipole_step_work",
    "mipme_ewald_step", "mipme_ewald_step_work",
    "mipme_ewald_batch", "mipme_ewald_batch_work", "mipme_ewald_batch_table_bytes", "mipme_ewald_batch_table_build",
    "mipme_dipole_cell_step", "mipme_dipole_cell_step_work",
    "mipme_dipole_batch", "mipme_dipole_batch_work", "mipme_dipole_batch_table_bytes", "mipme_dipole_batch_table_build",
    "mipme_ewald_channels_step", "mipme_ewald_channels_step_work",
    "mipme_ewald_channels_batch", "mipme_ewald_channels_batch_work", "mipme_ewald_channels_batch_table_bytes",
    "mipme_ewald_channels_batch_table_build",
)


class PotentialDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("exponent", C.c_int32),
        ("smearing", C.c_double),
        ("prefactor", C.c_double),
        ("exclusion_radius", C.c_double),
        ("exclusion_degree", C.c_int32),
        ("_pad", C.c_int32),
    ]


class DipoleDesc(C.Structure):
    """``mipme_dipole_t``: the dipolar pair tensor (its own descriptor, not a kind of ``mipme_potential_t``)."""

    _fields_ = [
        ("smearing", C.c_double),
        ("prefactor", C.c_double),
        ("exclusion_radius", C.c_double),
        ("exclusion_degree", C.c_int32),
        ("_pad", C.c_int32),
    ]


class SplineDesc(C.Structure):
    """``mipme_spline_t``: float64 knot tables on the device (plain or reciprocal-axis spline) and the 3-knot spline below the
    first knot of a reciprocal-axis one."""

    _fields_ = [
        ("x", C.c_void_p),
        ("y", C.c_void_p),
        ("d2y", C.c_void_p),
        ("n", C.c_int32),
        ("reciprocal", C.c_int32),
        ("zero_x", C.c_double * 3),
        ("zero_y", C.c_double * 3),
        ("zero_d2y", C.c_double * 3),
        ("prefactor", C.c_double),
    ]


#: ``MIPME_COMBINED_MAX_TERMS`` / ``MIPME_COMBINED_MAX_ORDER`` of the header
COMBINED_MAX_TERMS, COMBINED_MAX_ORDER = 8, 6


class CombinedDesc(C.Structure):
    """``mipme_combined_t``: the terms of a weighted sum of 1/r^p potentials (the weights stay on the device)."""

    _fields_ = [
        ("n_terms", C.c_int32),
        ("reserved", C.c_int32),
        ("terms", PotentialDesc * 8),
    ]


class MeshDesc(C.Structure):
    _fields_ = [
        ("scheme", C.c_int32),
        ("order", C.c_int32),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("nz", C.c_int32),
        ("n_channels", C.c_int32),
        ("cell", C.c_double * 9),
        ("inv_cell", C.c_double * 9),
        ("volume", C.c_double),
    ]


class SrJob(C.Structure):
    """``mipme_sr_job_t``: the short-range pair sum co-scheduled with the spread by ``mipme_kspace_forward``."""

    _fields_ = [
        ("n_atoms", C.c_int64),
        ("row_ptr", C.c_void_p),
        ("entries_shift", C.c_void_p),
        ("entries", C.c_void_p),
        ("positions", C.c_void_p),
        ("cell", C.c_void_p),
        ("charges", C.c_void_p),
        ("pot", C.POINTER(PotentialDesc)),
        ("full_list", C.c_int32),
        ("shift_format", C.c_int32),
        ("records", C.c_void_p),
        ("out", C.c_void_p),
        ("force", C.c_void_p),
        ("dist_out", C.c_void_p),
    ]


class Frame(C.Structure):
    """``mipme_frame_t``: one frame of ``mipme_frames_forward / backward`` (independent frames in one launch)."""

    _fields_ = [
        ("n_atoms", C.c_int64),
        ("positions", C.c_void_p),
        ("charges", C.c_void_p),
        ("cell", C.c_void_p),
        ("mesh", MeshDesc),
        ("atom_bins", C.c_void_p),
        ("brick_counters", C.c_void_p),
        ("row_ptr", C.c_void_p),
        ("entries_shift", C.c_void_p),
        ("entries", C.c_void_p),
        ("full_list", C.c_int32),
        ("shift_format", C.c_int32),
        ("records", C.c_void_p),
        ("rho_mesh", C.c_void_p),
        ("phi_mesh", C.c_void_p),
        ("dc", C.c_void_p),
        ("out", C.c_void_p),
        ("force", C.c_void_p),
        ("field", C.c_void_p),
        ("dist_out", C.c_void_p),
        ("energy", C.c_void_p),
        ("grad_positions", C.c_void_p),
        ("use_tail", C.c_int32),
        ("counter_ints", C.c_int32),
        ("grad_seed", C.c_void_p),
    ]


ARGS_VERSION = 2


class _VersionedArgs(C.Structure):
    """Base of the versioned argument structs (``include/mipme.h``): ``size`` / ``version`` are filled in here, every other
    field is passed by NAME -- a binding that forgets a field passes NULL for it instead of shifting the rest."""

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        super().__init__(size=C.sizeof(type(self)), version=ARGS_VERSION, **fields)


class KspaceForwardArgs(_VersionedArgs):
    """``mipme_kspace_forward_args_t``"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("plan", C.c_void_p), ("stream", C.c_void_p), ("dtype", C.c_int32), ("accumulate_out", C.c_int32),
        ("mesh", C.POINTER(MeshDesc)), ("pot", C.POINTER(PotentialDesc)), ("n_atoms", C.c_int64),
        ("positions", C.c_void_p), ("charges", C.c_void_p), ("G", C.c_void_p),
        ("rho_mesh", C.c_void_p), ("rho_hat", C.c_void_p), ("hat_work", C.c_void_p), ("phi_mesh", C.c_void_p),
        ("dc", C.c_void_p), ("out_lr", C.c_void_p), ("out_phi", C.c_void_p), ("atom_bins", C.c_void_p),
        ("gather_wait_event", C.c_void_p), ("out_field", C.c_void_p), ("out_records", C.c_void_p),
        ("sr_job", C.POINTER(SrJob)), ("out_cell_partials", C.c_void_p),
        ("out_energy", C.c_void_p), ("out_grad_positions", C.c_void_p), ("grad_seed", C.c_void_p),
        ("nan_flag", C.c_void_p),
        ("out_grad_charges", C.c_void_p), ("out_grad_cell", C.c_void_p), ("G_deriv", C.c_void_p), ("cell_work", C.c_void_p),
        ("aux_seed", C.c_void_p), ("out_rho_hat", C.c_void_p), ("flags", C.c_int64),
        ("energy_log", C.c_void_p), ("energy_log_cursor", C.c_void_p), ("energy_log_capacity", C.c_int64),
        ("slab", C.c_int32), ("_pad_slab", C.c_int32),
    ]


class KspaceBackwardArgs(_VersionedArgs):
    """``mipme_kspace_backward_args_t``"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("plan", C.c_void_p), ("stream", C.c_void_p), ("dtype", C.c_int32), ("_pad", C.c_int32),
        ("mesh", C.POINTER(MeshDesc)), ("pot", C.POINTER(PotentialDesc)), ("n_atoms", C.c_int64),
        ("positions", C.c_void_p), ("charges", C.c_void_p), ("grad_out", C.c_void_p), ("G", C.c_void_p),
        ("phi_mesh", C.c_void_p), ("rho_hat", C.c_void_p), ("rho_dc", C.c_void_p), ("phi_atoms", C.c_void_p),
        ("psi_mesh", C.c_void_p), ("psi_hat", C.c_void_p), ("hat_work", C.c_void_p), ("chi_mesh", C.c_void_p),
        ("dc", C.c_void_p), ("partials", C.c_void_p), ("grad_positions", C.c_void_p), ("grad_charges", C.c_void_p),
        ("grad_cell", C.c_void_p), ("atom_bins", C.c_void_p), ("grad_scale", C.c_void_p), ("mesh_field", C.c_void_p),
        ("kgrid_blocks_ready", C.c_int64), ("G_deriv", C.c_void_p),
    ]


class NlDesc(C.Structure):
    _fields_ = [
        ("cell", C.c_double * 9),
        ("inv_cell", C.c_double * 9),
        ("n_cells", C.c_int32 * 3),
        ("periodic", C.c_int32 * 3),
        ("cutoff", C.c_double),
        ("full_list", C.c_int32),
        ("_pad", C.c_int32),
        ("frac_offset", C.c_double * 3),
        ("frac_scale", C.c_double * 3),
        ("reach", C.c_int32 * 3),
        ("position_stride", C.c_int32),
    ]


class MdArgs(_VersionedArgs):
    """``mipme_md_args_t`` (version 1)"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("plan", C.c_void_p), ("stream", C.c_void_p), ("dtype", C.c_int32), ("shift_format", C.c_int32),
        ("mesh", C.POINTER(MeshDesc)), ("pot", C.POINTER(PotentialDesc)), ("n_atoms", C.c_int64),
        ("records", C.c_void_p), ("cell", C.c_void_p), ("G", C.c_void_p),
        ("rho_mesh", C.c_void_p), ("hat_work", C.c_void_p), ("phi_mesh", C.c_void_p), ("dc", C.c_void_p),
        ("atom_bins", C.c_void_p), ("live_lists", C.c_void_p), ("row_ptr", C.c_void_p), ("words", C.c_void_p),
        ("potentials", C.c_void_p), ("pair_force", C.c_void_p), ("energy", C.c_void_p), ("grad_positions", C.c_void_p),
        ("grad_seed", C.c_void_p), ("nan_flag", C.c_void_p), ("host_flags", C.c_void_p),
        ("grad_charges", C.c_void_p), ("grad_cell", C.c_void_p), ("G_deriv", C.c_void_p), ("cell_work", C.c_void_p),
        ("aux_seed", C.c_void_p),
        ("energy_log", C.c_void_p), ("energy_log_cursor", C.c_void_p), ("energy_log_capacity", C.c_int64),
        ("slab", C.c_int32), ("_pad_slab", C.c_int32),
    ]

    def __init__(self, **fields):
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=1, **fields)


FRAMES_STEP_VERSION = 1


class FramesStepArgs(_VersionedArgs):
    """``mipme_frames_step_args_t`` (version ``MIPME_FRAMES_STEP_VERSION``)"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("plan", C.c_void_p), ("stream", C.c_void_p), ("dtype", C.c_int32), ("n_frames", C.c_int32),
        ("frames", C.POINTER(Frame)), ("pot", C.POINTER(PotentialDesc)), ("device_table", C.c_void_p),
        ("G", C.c_void_p), ("G_stride", C.c_int64),
        ("rho_mesh_all", C.c_void_p), ("hat_work_all", C.c_void_p), ("phi_mesh_all", C.c_void_p), ("dc_all", C.c_void_p),
        ("cell_work", C.c_void_p), ("cell_gradient", C.c_int32), ("_pad", C.c_int32),
    ]

    def __init__(self, **fields):
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=FRAMES_STEP_VERSION, **fields)


FRAMES_CELLS_VERSION = 1


class FramesCellsArgs(_VersionedArgs):
    """``mipme_frames_cells_args_t`` (version ``MIPME_FRAMES_CELLS_VERSION``): the launch that turns the cells of a frame batch, as
    they stand on the device, into the geometry of its table, its filter tables and the validated copy of the cells"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("stream", C.c_void_p), ("dtype", C.c_int32), ("n_frames", C.c_int32),
        ("frames", C.POINTER(Frame)), ("pot", C.POINTER(PotentialDesc)), ("device_table", C.c_void_p),
        ("cells", C.c_void_p), ("cells_valid", C.c_void_p), ("G", C.c_void_p), ("G_stride", C.c_int64),
        ("G_deriv", C.c_void_p), ("G_deriv_stride", C.c_int64), ("mesh_spacing", C.c_double), ("status", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=FRAMES_CELLS_VERSION, **fields)


FRAMES_SLAB_STEP_VERSION = 1


class FramesSlabStepArgs(_VersionedArgs):
    """``mipme_frames_slab_step_args_t`` (version ``MIPME_FRAMES_SLAB_STEP_VERSION``): a ``mipme_frames_step_args_t`` plus the
    per-frame slab codes (host ``int32`` array: 0 = off, else the non-periodic axis + 1) and the moments' work buffer"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("step", FramesStepArgs), ("slab", C.POINTER(C.c_int32)), ("slab_work", C.c_void_p), ("slab_work_stride", C.c_int64),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=FRAMES_SLAB_STEP_VERSION, **fields)


COMBINED_STEP_VERSION = 1


class CombinedStepArgs(_VersionedArgs):
    """``mipme_combined_step_args_t`` (version ``MIPME_COMBINED_STEP_VERSION``)"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("plan", C.c_void_p), ("stream", C.c_void_p), ("dtype", C.c_int32), ("full_list", C.c_int32),
        ("mesh", C.POINTER(MeshDesc)), ("comb", C.POINTER(CombinedDesc)), ("n_atoms", C.c_int64),
        ("positions", C.c_void_p), ("charges", C.c_void_p), ("cell", C.c_void_p), ("weights", C.c_void_p),
        ("G_terms", C.c_void_p), ("G", C.c_void_p),
        ("rho_mesh", C.c_void_p), ("hat_work", C.c_void_p), ("phi_mesh", C.c_void_p), ("dc", C.c_void_p),
        ("atom_bins", C.c_void_p), ("records", C.c_void_p), ("rho_hat", C.c_void_p),
        ("row_ptr", C.c_void_p), ("entries", C.c_void_p), ("shift_format", C.c_int32), ("_pad", C.c_int32),
        ("potentials", C.c_void_p), ("pair_force", C.c_void_p), ("field", C.c_void_p), ("energy", C.c_void_p),
        ("grad_positions", C.c_void_p), ("grad_seed", C.c_void_p), ("grad_weights", C.c_void_p), ("grad_charges", C.c_void_p),
        ("work", C.c_void_p), ("nan_flag", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=COMBINED_STEP_VERSION, **fields)


DIPOLE_STEP_VERSION = 1


class DipoleStepArgs(_VersionedArgs):
    """``mipme_dipole_step_args_t`` (version ``MIPME_DIPOLE_STEP_VERSION``)"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("stream", C.c_void_p), ("dtype", C.c_int32), ("full_list", C.c_int32),
        ("pot", C.POINTER(DipoleDesc)), ("n_atoms", C.c_int64), ("n_k", C.c_int64),
        ("inv_volume", C.c_double), ("self_term", C.c_double), ("background", C.c_double),
        ("positions", C.c_void_p), ("dipoles", C.c_void_p), ("cell", C.c_void_p), ("inv_cell", C.c_void_p),
        ("kvectors", C.c_void_p), ("G", C.c_void_p), ("dG", C.c_void_p),
        ("row_ptr", C.c_void_p), ("entries", C.c_void_p), ("shift_format", C.c_int32), ("cell_gradient", C.c_int32),
        ("records", C.c_void_p), ("s_cos", C.c_void_p), ("s_sin", C.c_void_p),
        ("energy", C.c_void_p), ("forces", C.c_void_p), ("grad_dipoles", C.c_void_p), ("grad_cell", C.c_void_p),
        ("work", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=DIPOLE_STEP_VERSION, **fields)


DIPOLE_CELL_STEP_VERSION = 1


class DipoleCellStepArgs(_VersionedArgs):
    """``mipme_dipole_cell_step_args_t`` (version ``MIPME_DIPOLE_CELL_STEP_VERSION``)"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("stream", C.c_void_p), ("dtype", C.c_int32), ("full_list", C.c_int32),
        ("pot", C.POINTER(DipoleDesc)), ("self_term", C.c_double), ("background", C.c_double),
        ("n_atoms", C.c_int64), ("n_k", C.c_int64),
        ("lr_wavelength", C.c_double), ("ns", C.c_int32 * 3), ("cell_gradient", C.c_int32),
        ("positions", C.c_void_p), ("dipoles", C.c_void_p), ("cell", C.c_void_p),
        ("frequencies", C.c_void_p), ("multiplicities", C.c_void_p),
        ("row_ptr", C.c_void_p), ("entries", C.c_void_p), ("shift_format", C.c_int32), ("_pad", C.c_int32),
        ("records", C.c_void_p), ("kvectors", C.c_void_p), ("G", C.c_void_p), ("dG", C.c_void_p),
        ("s_cos", C.c_void_p), ("s_sin", C.c_void_p),
        ("energy", C.c_void_p), ("forces", C.c_void_p), ("grad_dipoles", C.c_void_p), ("grad_cell", C.c_void_p),
        ("status", C.c_void_p), ("work", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=DIPOLE_CELL_STEP_VERSION, **fields)


EWALD_STEP_VERSION = 1
EWALD_BATCH_VERSION = 1


class EwaldStepArgs(_VersionedArgs):
    """``mipme_ewald_step_args_t`` (version ``MIPME_EWALD_STEP_VERSION``)"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("stream", C.c_void_p), ("dtype", C.c_int32), ("full_list", C.c_int32),
        ("pot", C.POINTER(PotentialDesc)), ("n_atoms", C.c_int64), ("n_k", C.c_int64),
        ("lr_wavelength", C.c_double), ("ns", C.c_int32 * 3), ("cell_gradient", C.c_int32),
        ("positions", C.c_void_p), ("charges", C.c_void_p), ("cell", C.c_void_p),
        ("frequencies", C.c_void_p), ("multiplicities", C.c_void_p),
        ("row_ptr", C.c_void_p), ("entries", C.c_void_p), ("shift_format", C.c_int32), ("_pad", C.c_int32),
        ("records", C.c_void_p), ("kvectors", C.c_void_p), ("G", C.c_void_p), ("dG", C.c_void_p),
        ("s_cos", C.c_void_p), ("s_sin", C.c_void_p),
        ("energy", C.c_void_p), ("forces", C.c_void_p), ("grad_charges", C.c_void_p), ("grad_cell", C.c_void_p),
        ("status", C.c_void_p), ("work", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=EWALD_STEP_VERSION, **fields)


class EwaldBatchArgs(_VersionedArgs):
    """``mipme_ewald_batch_args_t`` (version ``MIPME_EWALD_BATCH_VERSION``); ``atom_ptr``, ``k_ptr`` and ``entry_ptr`` are HOST
    arrays of int64"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("stream", C.c_void_p), ("dtype", C.c_int32), ("full_list", C.c_int32),
        ("pot", C.POINTER(PotentialDesc)), ("n_frames", C.c_int32), ("cell_gradient", C.c_int32),
        ("lr_wavelength", C.c_double),
        ("atom_ptr", C.c_void_p), ("k_ptr", C.c_void_p), ("entry_ptr", C.c_void_p), ("device_table", C.c_void_p),
        ("positions", C.c_void_p), ("charges", C.c_void_p), ("cells", C.c_void_p),
        ("frequencies", C.c_void_p), ("multiplicities", C.c_void_p),
        ("row_ptr", C.c_void_p), ("entries", C.c_void_p), ("shift_format", C.c_int32), ("_pad", C.c_int32),
        ("records", C.c_void_p), ("kvectors", C.c_void_p), ("G", C.c_void_p), ("dG", C.c_void_p),
        ("s_cos", C.c_void_p), ("s_sin", C.c_void_p),
        ("energies", C.c_void_p), ("forces", C.c_void_p), ("grad_charges", C.c_void_p), ("grad_cells", C.c_void_p),
        ("status", C.c_void_p), ("work", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=EWALD_BATCH_VERSION, **fields)


EWALD_CHANNELS_STEP_VERSION = 1
EWALD_CHANNELS_BATCH_VERSION = 1
EWALD_MAX_CHANNELS = 8  # MIPME_EWALD_MAX_CHANNELS


class EwaldChannelsStepArgs(_VersionedArgs):
    """``mipme_ewald_channels_step_args_t`` (version ``MIPME_EWALD_CHANNELS_STEP_VERSION``): the fields of
    :class:`EwaldStepArgs` with ``n_channels`` where that struct pads"""

    _fields_ = [(name, tp) if name != "_pad" else ("n_channels", tp) for name, tp in EwaldStepArgs._fields_]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=EWALD_CHANNELS_STEP_VERSION, **fields)


class EwaldChannelsBatchArgs(_VersionedArgs):
    """``mipme_ewald_channels_batch_args_t`` (version ``MIPME_EWALD_CHANNELS_BATCH_VERSION``): the fields of
    :class:`EwaldBatchArgs` with ``n_channels`` where that struct pads"""

    _fields_ = [(name, tp) if name != "_pad" else ("n_channels", tp) for name, tp in EwaldBatchArgs._fields_]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=EWALD_CHANNELS_BATCH_VERSION, **fields)


DIPOLE_BATCH_VERSION = 1


class DipoleBatchArgs(_VersionedArgs):
    """``mipme_dipole_batch_args_t`` (version ``MIPME_DIPOLE_BATCH_VERSION``); ``atom_ptr``, ``k_ptr`` and ``entry_ptr`` are HOST
    arrays of int64"""

    _fields_ = [
        ("size", C.c_uint32), ("version", C.c_uint32),
        ("stream", C.c_void_p), ("dtype", C.c_int32), ("full_list", C.c_int32),
        ("pot", C.POINTER(DipoleDesc)), ("self_term", C.c_double), ("background", C.c_double),
        ("n_frames", C.c_int32), ("cell_gradient", C.c_int32),
        ("lr_wavelength", C.c_double),
        ("atom_ptr", C.c_void_p), ("k_ptr", C.c_void_p), ("entry_ptr", C.c_void_p), ("device_table", C.c_void_p),
        ("positions", C.c_void_p), ("dipoles", C.c_void_p), ("cells", C.c_void_p),
        ("frequencies", C.c_void_p), ("multiplicities", C.c_void_p),
        ("row_ptr", C.c_void_p), ("entries", C.c_void_p), ("shift_format", C.c_int32), ("_pad", C.c_int32),
        ("records", C.c_void_p), ("kvectors", C.c_void_p), ("G", C.c_void_p), ("dG", C.c_void_p),
        ("s_cos", C.c_void_p), ("s_sin", C.c_void_p),
        ("energies", C.c_void_p), ("forces", C.c_void_p), ("grad_dipoles", C.c_void_p), ("grad_cells", C.c_void_p),
        ("status", C.c_void_p), ("work", C.c_void_p),
    ]

    def __init__(self, **fields):
        unknown = set(fields) - {name for name, _ in self._fields_}
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(unknown)}")
        C.Structure.__init__(self, size=C.sizeof(type(self)), version=DIPOLE_BATCH_VERSION, **fields)


#: OR-ed into a shift format: rows written by ``mipme_nl_stream`` (``row_ptr`` int32[3N+1], every neighbour once per row)
ROWS_PADDED = 0x100
FWD_RHO_MESH_UNUSED = 1  # mipme_kspace_forward_args_t.flags: the caller never reads rho_mesh after the call


class MipmeError(RuntimeError):
    pass


_lib = None


def _declare(lib):
    vp, i64, ci, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    MP, PP = C.POINTER(MeshDesc), C.POINTER(PotentialDesc)
    lib.mipme_last_error.restype = C.c_char_p
    lib.mipme_last_error.argtypes = []
    lib.mipme_version.restype = ci
    lib.mipme_version.argtypes = []
    sig = {
        "mipme_fft_plan_create": [ci, ci, ci, ci, ci, C.POINTER(vp)],
        "mipme_fft_plan_destroy": [vp],
        "mipme_kfilter_build": [vp, ci, MP, PP, vp],
        "mipme_kfilter_build_deriv": [vp, ci, MP, PP, vp],
        "mipme_convolve": [vp, vp, vp, vp, vp, vp, vp, vp],
        "mipme_spread": [vp, ci, MP, i64, vp, vp, vp],
        "mipme_gather": [vp, ci, MP, i64, vp, vp, vp],
        "mipme_spread_jet": [vp, ci, MP, i64, vp, vp, ci, ci, ci, vp],
        "mipme_gather_jet": [vp, ci, MP, i64, vp, vp, ci, ci, ci, vp],
        "mipme_gather_jet3": [vp, ci, MP, i64, vp, vp, ci, ci, ci, vp],
        "mipme_pair_sum": [vp, ci, ci, i64, i64, ci, vp, vp, vp, ci, vp],
        "mipme_pair_sum_rows": [vp, ci, i64, ci, vp, vp, vp, vp, ci, vp],
        "mipme_pair_dot": [vp, ci, ci, i64, ci, vp, vp, vp, ci, vp],
        "mipme_pair_diff": [vp, ci, ci, i64, ci, vp, vp, vp],
        "mipme_pair_scatter": [vp, ci, ci, i64, i64, ci, vp, vp, vp, vp, vp],
        "mipme_kspace_forward": [C.POINTER(KspaceForwardArgs)],
        "mipme_kspace_backward": [C.POINTER(KspaceBackwardArgs)],
        "mipme_slab_forward": [vp, ci, ci, MP, dbl, i64, vp, vp, vp, vp],
        "mipme_slab_backward": [vp, ci, ci, MP, dbl, i64, vp, vp, vp, vp, vp, vp, vp],
        "mipme_rspace_forward": [vp, ci, ci, i64, i64, ci, vp, vp, vp, vp, ci, PP, ci, vp],
        "mipme_rspace_backward": [vp, ci, ci, i64, i64, ci, vp, vp, vp, vp, ci, PP, vp, vp, vp, vp],
        "mipme_pair_distance_forward": [vp, ci, ci, i64, vp, vp, vp, vp, vp],
        "mipme_pair_distance_backward": [vp, ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp],
        "mipme_topology_build": [vp, ci, i64, i64, vp, vp, i64, vp, vp],
        "mipme_topology_pack_shifts": [vp, ci, i64, vp, vp, vp, vp],
        "mipme_rspace_rows": [vp, ci, i64, ci, vp, vp, vp, vp, vp, ci, ci, PP, ci, vp],
        "mipme_rspace_rows_tabulate": [vp, ci, i64, vp, vp, vp, vp, ci, PP, vp, vp],
        "mipme_rspace_rows_tabulated": [vp, ci, i64, vp, vp, vp, ci, ci, ci, vp],
        "mipme_pair_distance_backward_rows": [vp, ci, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "mipme_topology_pack_entries": [vp, ci, i64, i64, vp, vp, vp, ci, vp, vp],
        "mipme_pack_pair_shifts": [vp, ci, i64, vp, vp, vp],
        "mipme_pair_distance_forward_packed": [vp, ci, i64, vp, vp, vp, vp, vp],
        "mipme_sr_rows_fused": [vp, ci, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, PP, ci, ci, vp, ci, vp, vp, vp, vp, vp],
        "mipme_sr_rows_finalize": [vp, ci, i64, vp, vp, vp, vp, ci, vp, vp, vp],
        "mipme_fft_r2c": [vp, vp, ci, MP, vp, vp],
        "mipme_frames_table_build": [ci, ci, C.POINTER(Frame), PP, vp, i64],
        "mipme_frames_forward": [vp, vp, ci, ci, C.POINTER(Frame), PP, vp, vp, i64, vp, vp, vp, vp],
        "mipme_frames_backward": [vp, ci, ci, C.POINTER(Frame), vp, vp],
        "mipme_ewald_filter": [vp, ci, PP, i64, vp, vp, vp],
        "mipme_ewald_structure": [vp, ci, i64, ci, i64, vp, vp, vp, vp, vp, i64],
        "mipme_ewald_potential": [vp, ci, i64, ci, i64, vp, vp, vp, vp, vp, vp, i64],
        "mipme_ewald_backward": [vp, ci, i64, ci, i64] + [vp] * 12 + [i64],
        "mipme_dipole_rspace_forward": [vp, ci, ci, i64, i64, ci, vp, vp, vp, C.POINTER(DipoleDesc), vp],
        "mipme_dipole_rspace_backward": [vp, ci, ci, i64, i64, ci, vp, vp, vp, vp, C.POINTER(DipoleDesc), vp, vp],
        "mipme_dipole_structure": [vp, ci, i64, i64] + [vp] * 7,
        "mipme_dipole_field": [vp, ci, i64, i64] + [vp] * 7,
        "mipme_dipole_backward": [vp, ci, i64, i64] + [vp] * 13,
        "mipme_spline_eval": [vp, ci, C.POINTER(SplineDesc), ci, i64, vp, vp],
        "mipme_spline_eval_reciprocal": [vp, ci, C.POINTER(SplineDesc), i64, vp, vp, vp],
        "mipme_spline_kfilter_build": [vp, ci, MP, C.POINTER(SplineDesc), vp],
        "mipme_combined_sr_eval": [vp, ci, C.POINTER(CombinedDesc), ci, C.POINTER(dbl), i64, vp, vp, vp],
        "mipme_combined_kfilter_build": [vp, ci, MP, C.POINTER(CombinedDesc), vp],
        "mipme_combined_step": [C.POINTER(CombinedStepArgs)],
        "mipme_dipole_step": [C.POINTER(DipoleStepArgs)],
        "mipme_dipole_cell_step": [C.POINTER(DipoleCellStepArgs)],
        "mipme_ewald_step": [C.POINTER(EwaldStepArgs)],
        "mipme_ewald_batch": [C.POINTER(EwaldBatchArgs)],
        "mipme_ewald_batch_table_build": [ci, vp, vp, vp, vp, ci, vp, i64],
        "mipme_ewald_channels_step": [C.POINTER(EwaldChannelsStepArgs)],
        "mipme_ewald_channels_batch": [C.POINTER(EwaldChannelsBatchArgs)],
        "mipme_ewald_channels_batch_table_build": [ci, vp, vp, vp, vp, ci, ci, vp, i64],
        "mipme_dipole_batch": [C.POINTER(DipoleBatchArgs)],
        "mipme_dipole_batch_table_build": [ci, vp, vp, vp, vp, ci, vp, i64],
        "mipme_dot_forward": [vp, ci, i64, vp, vp, vp, vp],
        "mipme_dot_backward": [vp, ci, i64, vp, vp, vp, vp, vp],
        "mipme_energy_log_push": [vp, ci, ci, vp, vp, vp, ci],
        "mipme_frames_table_energy_log": [ci, ci, vp, i64, vp, vp, ci],
        "mipme_frames_table_contract": [ci, ci, C.POINTER(Frame), PP, vp, i64, C.POINTER(vp), C.POINTER(vp), vp, i64, vp, i64, vp],
        "mipme_frames_step": [C.POINTER(FramesStepArgs)],
        "mipme_frames_table_slab": [ci, ci, C.POINTER(Frame), PP, vp, i64, C.POINTER(C.c_int32), vp, i64],
        "mipme_frames_slab_step": [C.POINTER(FramesSlabStepArgs)],
        "mipme_frames_table_cells": [ci, ci, C.POINTER(Frame), vp, i64, vp],
        "mipme_frames_cells": [C.POINTER(FramesCellsArgs)],
        "mipme_frames_cell_geometry": [C.POINTER(dbl), ci, C.POINTER(C.c_int32), dbl, C.POINTER(dbl), C.POINTER(dbl),
                                       C.POINTER(C.c_int32)],
        "mipme_scaled_match": [vp, ci, i64, vp, vp, vp, vp],
        "mipme_scaled_match_work": [i64],
        "mipme_scaled_match_wide": [vp, ci, i64, vp, vp, vp, vp, vp],
        "mipme_nl_bin": [vp, ci, C.POINTER(NlDesc), i64, vp, vp],
        "mipme_nl_count": [vp, ci, C.POINTER(NlDesc), i64, vp, vp],
        "mipme_nl_fill": [vp, ci, C.POINTER(NlDesc), i64, vp, vp, vp, vp, vp],
        "mipme_nl_stream": [vp, ci, C.POINTER(NlDesc), i64, vp, i64, vp, vp, vp],
        "mipme_set_skip_flag": [vp],
        "mipme_values_equal": [vp, ci, i64, vp, vp, vp],
        "mipme_checksum": [vp, vp, i64, vp, vp, vp],
        "mipme_energy_select": [vp, ci, i64, vp, vp, vp, vp, ci, vp, vp],
        "mipme_energy_select_sum": [vp, ci, i64, vp, vp, vp, vp, ci, vp, vp, vp],
        "mipme_energy_select_contract": [vp, ci, i64, vp, vp, vp, vp, ci, vp, vp, vp],
        "mipme_md_rebin": [C.POINTER(MdArgs)],
        "mipme_md_step": [C.POINTER(MdArgs)],
    }
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.restype = ci
        fn.argtypes = argtypes
    lib.mipme_cellgrad_partials_size.restype = i64
    lib.mipme_cellgrad_partials_size.argtypes = [MP, i64]
    lib.mipme_dipole_partials_size.restype = i64
    lib.mipme_dipole_partials_size.argtypes = [i64, i64]
    lib.mipme_pair_partials_size.restype = i64
    lib.mipme_pair_partials_size.argtypes = [i64]
    lib.mipme_topology_workspace_bytes.restype = i64
    lib.mipme_topology_workspace_bytes.argtypes = [i64]
    lib.mipme_rows_partials_size.restype = i64
    lib.mipme_rows_partials_size.argtypes = [i64]
    lib.mipme_atom_bins_bytes.restype = i64
    lib.mipme_atom_bins_bytes.argtypes = [MP, i64, ci]
    lib.mipme_last_cosched_kernel.restype = C.c_char_p
    lib.mipme_last_cosched_kernel.argtypes = []
    if hasattr(lib, "mipme_last_slot_fill"):  # (an older build named by MIPME_LIB for an A/B run lacks the query)
        lib.mipme_last_slot_fill.restype = ci
        lib.mipme_last_slot_fill.argtypes = []
        lib.mipme_last_cell_riders.restype = ci
        lib.mipme_last_cell_riders.argtypes = []
    if hasattr(lib, "mipme_last_gather_pairs"):
        lib.mipme_last_gather_pairs.restype = ci
        lib.mipme_last_gather_pairs.argtypes = []
    if hasattr(lib, "mipme_last_inverse_split"):
        lib.mipme_last_inverse_split.restype = ci
        lib.mipme_last_inverse_split.argtypes = []
    lib.mipme_plane_spread_parts.restype = ci
    lib.mipme_plane_spread_parts.argtypes = [MP, i64, ci]
    lib.mipme_frames_counter_ints.restype = i64
    lib.mipme_frames_counter_ints.argtypes = [MP, i64, ci]
    lib.mipme_md_supported.restype = ci
    lib.mipme_md_supported.argtypes = [MP, PP, i64, ci]
    lib.mipme_md_lists_ints.restype = i64
    lib.mipme_md_lists_ints.argtypes = [MP, i64]
    lib.mipme_nl_workspace_bytes.restype = i64
    lib.mipme_nl_workspace_bytes.argtypes = [C.POINTER(NlDesc), i64]
    lib.mipme_rspace_rows_value_bytes.restype = i64
    lib.mipme_rspace_rows_value_bytes.argtypes = [ci, i64]
    lib.mipme_checksum_words.restype = i64
    lib.mipme_checksum_words.argtypes = []
    lib.mipme_cell_tail_work.restype = i64
    lib.mipme_cell_tail_work.argtypes = [vp, MP, i64]
    lib.mipme_fft_plan_xfused.restype = ci
    lib.mipme_fft_plan_xfused.argtypes = [vp]
    lib.mipme_fft_plan_kgrid_blocks.restype = i64
    lib.mipme_fft_plan_kgrid_blocks.argtypes = [vp]
    lib.mipme_frames_cell_work.restype = i64
    lib.mipme_frames_cell_work.argtypes = [MP, i64]
    lib.mipme_combined_step_work.restype = i64
    lib.mipme_combined_step_work.argtypes = [vp, MP, i64, ci]
    lib.mipme_dipole_step_work.restype = i64
    lib.mipme_dipole_step_work.argtypes = [i64, i64, ci]
    lib.mipme_dipole_cell_step_work.restype = i64
    lib.mipme_dipole_cell_step_work.argtypes = [i64, i64, ci]
    lib.mipme_ewald_step_work.restype = i64
    lib.mipme_ewald_step_work.argtypes = [i64, i64, ci]
    lib.mipme_ewald_batch_work.restype = i64
    lib.mipme_ewald_batch_work.argtypes = [ci, vp, vp, ci]
    lib.mipme_ewald_batch_table_bytes.restype = i64
    lib.mipme_ewald_batch_table_bytes.argtypes = [ci, vp, vp, ci]
    lib.mipme_ewald_channels_step_work.restype = i64
    lib.mipme_ewald_channels_step_work.argtypes = [i64, i64, ci, ci]
    lib.mipme_ewald_channels_batch_work.restype = i64
    lib.mipme_ewald_channels_batch_work.argtypes = [ci, vp, vp, ci, ci]
    lib.mipme_ewald_channels_batch_table_bytes.restype = i64
    lib.mipme_ewald_channels_batch_table_bytes.argtypes = [ci, vp, vp, ci, ci]
    lib.mipme_dipole_batch_work.restype = i64
    lib.mipme_dipole_batch_work.argtypes = [ci, vp, vp, ci]
    lib.mipme_dipole_batch_table_bytes.restype = i64
    lib.mipme_dipole_batch_table_bytes.argtypes = [ci, vp, vp, ci]
    lib.mipme_frames_slab_work.restype = i64
    lib.mipme_frames_slab_work.argtypes = []
    lib.mipme_frames_table_bytes.restype = i64
    lib.mipme_frames_table_bytes.argtypes = [ci, ci]
    lib.mipme_profile_enable.restype = ci
    lib.mipme_profile_enable.argtypes = [ci]
    lib.mipme_profile_report.restype = i64
    lib.mipme_profile_report.argtypes = [C.c_char_p, i64]


def load():
    """Load (once) and return the ctypes handle of libmipme.so; raise if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MipmeError(
                f"HIP extension {LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C torch-pme_amd/csrc`). There is no CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        _declare(lib)
        _lib = lib
    return _lib


def check(rc: int):
    """Translate a C-ABI status into a Python exception (ValueError for MIPME_EINVAL)."""
    if rc == 0:
        return
    msg = load().mipme_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg)
    raise MipmeError(f"libmipme error {rc}: {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def dtype_code(dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.float64:
        return F64
    raise TypeError(f"libmipme supports float32 and float64 tensors, got {dtype}")


def complex_dtype(dtype):
    """The complex dtype of the half-grid arrays that go with a real ``dtype``."""
    return torch.complex64 if dtype == torch.float32 else torch.complex128


def index_code(dtype) -> int:
    if dtype == torch.int64:
        return I64
    if dtype == torch.int32:
        return I32
    raise TypeError(f"neighbor indices must be int64 or int32, got {dtype}")


def current_stream(device) -> int:
    """``hipStream_t`` of PyTorch's current stream on ``device`` (raw handle: no Stream object per call)."""
    idx = device.index
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_CTX = _NoCtx()


def on_device(device):
    """Context that makes ``device`` the current HIP device for the launches inside -- a no-op object when it already is
    (``torch.cuda.device`` costs ~4 us per enter / exit, several times per call)."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_CTX
    return torch.cuda.device(device)


def require_device(t, name: str):
    if not t.is_cuda:
        raise MipmeError(
            f"`{name}` lives on {t.device}: the MI355X-native path only runs on HIP devices "
            "(tensors on 'cuda'); there is no CPU fallback."
        )


class FFTPlan:
    """Owning wrapper of a ``mipme_fft_plan`` (own (y,z) plane kernels + x stage; hipFFT R2C / C2R for the general paths)."""

    def __init__(self, device, dtype, ns, batch):
        self.key = (torch.device(device).index, dtype, tuple(int(n) for n in ns), int(batch))
        handle = C.c_void_p()
        with torch.cuda.device(device):
            check(load().mipme_fft_plan_create(dtype_code(dtype), int(ns[0]), int(ns[1]), int(ns[2]), int(batch), C.byref(handle)))
        self.handle = handle
        #: the plan can run the convolution as (y,z) plane transforms + one fused x kernel (power-of-two nx)
        self.xfused = bool(load().mipme_fft_plan_xfused(handle))
        #: number of k-grid partial sums the fused convolution writes when asked for the cell sums (out_cell_partials)
        self.kgrid_blocks = int(load().mipme_fft_plan_kgrid_blocks(handle))

    def __del__(self):
        try:
            if self.handle and _lib is not None:
                _lib.mipme_fft_plan_destroy(self.handle)
        except Exception:
            pass


_PLANS: dict = {}


def get_plan(device, dtype, ns, batch, store: dict | None = None) -> FFTPlan:
    """Plan of (device, dtype, mesh, batch).  A plan owns device state that is live between its kernels (the brick counters
    of the binning pass), so evaluations that may run concurrently on different streams must not share one, and a plan must
    outlive every captured HIP graph that launches its kernels: the calculators therefore pass their own ``store`` dict
    (one plan per calculator and mesh, freed with the calculator).  Without a store a small global cache is used."""
    key = (torch.device(device).index, dtype, tuple(int(n) for n in ns), int(batch))
    cache = _PLANS if store is None else store
    plan = cache.get(key)
    if plan is None:
        if store is None and len(_PLANS) >= 32:
            _PLANS.pop(next(iter(_PLANS)))
        plan = FFTPlan(device, dtype, ns, batch)
        cache[key] = plan
    return plan


def profile_enable(on: bool):
    check(load().mipme_profile_enable(1 if on else 0))


def profile_report() -> dict:
    """{stage: (calls, total_ms)} recorded by the library since ``profile_enable(True)``."""
    lib = load()
    n = lib.mipme_profile_report(None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    lib.mipme_profile_report(buf, n + 1)
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.split()
        out[name] = (int(calls), float(ms))
    return out
