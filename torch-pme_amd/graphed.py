"""HIP-graph replay of one energy + forces evaluation.

At 32k atoms a step is a dozen short kernels behind ~0.3 ms of Python / autograd / launch overhead when run eagerly.  For a fixed topology (same neighbour list, cell, charges; positions change) the whole
``pair_distances -> calculator.forward -> (q*V).sum().backward()`` chain is captured once into a HIP graph
(``torch.cuda.CUDAGraph``: PyTorch is the capture front end, every captured node is a libmipme kernel
or a tiny reduction) and replayed per step.  This is the MD-loop form of the hot path; the calculators themselves
stay eager and reference-compatible.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, analytic, ops


def _capture_graph(device, warm_up, body, between=None):
    """The capture protocol of every graphed step: ``warm_up()`` on a side stream (plans, caches and lazy module loads get built
    off the default stream), join, device synchronisation, ``between()`` -- host-side work that must follow the warm-up and
    precede the capture --, then ``body()`` captured into a new graph, which is returned."""
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        warm_up()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    if between is not None:
        between()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


def _check_slab_potential(potential):
    """``slab_correction``: the 2-D periodic term exists for 1/r and rides on the mesh part."""
    desc = potential._descriptor()
    if not (desc.kind == _lib.COULOMB or desc.exponent == 1):
        raise ValueError("`slab_correction`: the slab term exists for 1/r only (CoulombPotential, or "
                         "InversePowerLawPotential(exponent=1))")
    if potential.smearing is None:
        raise ValueError("`slab_correction` belongs to the mesh part: the potential needs a smearing")


def _refuse_spline(calculator, what: str):
    """The captured steps run the fused kernels, which know neither a spline potential nor a combined one: say so before
    anything is launched."""
    from .potentials import CombinedPotential, SplinePotential

    for cls in (SplinePotential, CombinedPotential):
        if isinstance(getattr(calculator, "potential", None), cls):
            raise TypeError(f"{what} runs the fused kernels, which do not serve a {cls.__name__}: call the calculator eagerly "
                            "-- `calculator(charges, cell, positions, neighbor_indices, neighbor_distances)`")


class _LiveStep:
    """Buffers and argument struct of ``mipme_md_rebin`` / ``mipme_md_step`` (include/mipme.h): the energy + forces step of an
    MD-like loop on device-resident neighbour structures.  The atoms live in ONE (N, 4) array of records (x, y, z, charge) that
    every kernel of the step reads; the atom -> mesh-brick bookkeeping (bins, per-brick atom lists) is rebuilt only when the
    neighbour list is (``rebin``), while every weight is evaluated from the current positions in every step."""

    def __init__(self, calculator, charges, cell, positions, charge_gradient=False, cell_gradient=False, slab_axis=None):
        lib = self.lib = _lib.load()
        self.slab = 0 if slab_axis is None else int(slab_axis) + 1  # mipme_md_args_t.slab
        device, dtype = positions.device, positions.dtype
        N = positions.shape[0]
        self.device, self.dtype, self.n_atoms = device, dtype, N
        geom, G = calculator._kspace_setup(cell, dtype, device, speculate=False)
        self.geom, self.G = geom, G
        self.md = geom.desc(1)
        self.pot = calculator.potential._descriptor()
        self.dt = _lib.dtype_code(dtype)
        if charges.shape[1] != 1 or not lib.mipme_md_supported(C.byref(self.md), C.byref(self.pot), N, self.dt):
            raise NotImplementedError("outside the range of the live-bin step")
        self.plan = _lib.get_plan(device, dtype, geom.ns, 1, geom.plan_store)
        if not self.plan.xfused:
            raise NotImplementedError("the live-bin step needs a power-of-two mesh along x")
        self.rec = torch.empty((N, 4), dtype=dtype, device=device)
        self.rec[:, :3] = positions.detach()
        self.rec[:, 3] = charges.detach()[:, 0]
        cdtype = _lib.complex_dtype(dtype)
        self.cell = cell.detach().to(dtype).contiguous()
        self.rho = torch.empty(geom.ns, dtype=dtype, device=device)
        self.phi = torch.empty(geom.ns, dtype=dtype, device=device)
        self.hat = torch.empty((geom.n_half,), dtype=cdtype, device=device)
        self.dc = torch.empty((1,), dtype=dtype, device=device)
        self.bins = torch.empty((lib.mipme_atom_bins_bytes(C.byref(self.md), N, self.dt),), dtype=torch.uint8, device=device)
        self.lists = torch.zeros((lib.mipme_md_lists_ints(C.byref(self.md), N),), dtype=torch.int32, device=device)
        self.potentials = torch.empty((N,), dtype=dtype, device=device)
        self.pair_force = torch.empty((N, 3), dtype=dtype, device=device)
        self.energy = torch.empty((), dtype=dtype, device=device)
        self.grad = torch.empty((N, 3), dtype=dtype, device=device)
        self.minus_one = torch.tensor(-1.0, dtype=dtype, device=device)
        self.one = torch.tensor(1.0, dtype=dtype, device=device)
        # the rest of the autograd contract from the same five launches (+ one single-workgroup launch for the cell)
        self.grad_q = torch.empty((N, 1), dtype=dtype, device=device) if charge_gradient else None
        self.grad_cell = self.G_deriv = self.cell_work = None
        if cell_gradient:
            self.grad_cell = torch.empty((27,), dtype=dtype, device=device)
            self.G_deriv = ops.filter_derivative(geom, self.pot, dtype, device)
            self.cell_work = torch.empty((lib.mipme_cell_tail_work(self.plan.handle, C.byref(self.md), N),),
                                         dtype=torch.float64, device=device)
        self.flags = torch.zeros((1,), dtype=torch.int32).pin_memory()
        self.flags_np = self.flags.numpy()
        self.nan_flag = calculator._nan_flag_ptr()
        calculator._nan_shape = [1, *geom.ns]
        self.rows = None  # (row_ptr, words, shift_format)
        self.log = None  # an EnergyLog the step's gather appends the energy to (set by GraphedEnergyForces before its capture)

    def _args(self):
        row_ptr, words, fmt = self.rows if self.rows is not None else (self.lists, self.lists, 2)  # (rebin reads no rows)
        return _lib.MdArgs(
            plan=self.plan.handle, stream=_lib.current_stream(self.device), dtype=self.dt, shift_format=fmt,
            mesh=C.pointer(self.md), pot=C.pointer(self.pot), n_atoms=self.n_atoms, records=self.rec.data_ptr(),
            cell=self.cell.data_ptr(), G=self.G.data_ptr(), rho_mesh=self.rho.data_ptr(), hat_work=self.hat.data_ptr(),
            phi_mesh=self.phi.data_ptr(), dc=self.dc.data_ptr(), atom_bins=self.bins.data_ptr(),
            live_lists=self.lists.data_ptr(), row_ptr=row_ptr.data_ptr(), words=words.data_ptr(),
            potentials=self.potentials.data_ptr(), pair_force=self.pair_force.data_ptr(), energy=self.energy.data_ptr(),
            grad_positions=self.grad.data_ptr(), grad_seed=self.minus_one.data_ptr(), nan_flag=self.nan_flag,
            host_flags=self.flags.data_ptr(), grad_charges=_lib.ptr(self.grad_q), grad_cell=_lib.ptr(self.grad_cell),
            G_deriv=_lib.ptr(self.G_deriv), cell_work=_lib.ptr(self.cell_work), aux_seed=self.one.data_ptr(),
            energy_log=None if self.log is None else self.log.values.data_ptr(),
            energy_log_cursor=None if self.log is None else self.log.cursor.data_ptr(),
            energy_log_capacity=0 if self.log is None else self.log.capacity, slab=self.slab)

    def rebin(self):
        with _lib.on_device(self.device):
            a = self._args()
            _lib.check(self.lib.mipme_md_rebin(C.byref(a)))

    def step(self):
        with _lib.on_device(self.device):
            a = self._args()
            _lib.check(self.lib.mipme_md_step(C.byref(a)))

    @property
    def max_displacement(self) -> float:
        """A displacement (same units as the cell) every atom may make since the last rebin without leaving the margin of ONE mesh
        point: ``min_d 1 / (n_d |column d of inv(cell)|)`` (u_d = n_d r . inv(cell)[:, d] changes by at most n_d |dr| |column d|)."""
        inv = np.asarray(self.geom.inv_cell)
        return float(min(1.0 / (self.geom.ns[d] * np.linalg.norm(inv[:, d])) for d in range(3)))

    def moved(self) -> bool:
        """True if a step since the last look flagged an atom beyond the margin (clears the bit)."""
        f = int(self.flags_np[0])
        if f & 2:
            self.flags_np[0] = f & ~2
            return True
        return False

    def check(self):
        f = int(self.flags_np[0])
        if f:
            self.flags_np[0] = 0
            if f & 2:
                raise RuntimeError("GraphedEnergyForces: an atom has moved more than one mesh point since the last refresh(); "
                                   "the results of that step are invalid (its energy was returned as NaN) -- refresh the "
                                   "neighbour structures sooner, or call the object with check=True")
            raise RuntimeError("GraphedEnergyForces: a brick's atom list overflowed at the last refresh (very non-uniform "
                               "system); construct with live_bins=False")


class EnergyLog:
    """Device-resident log of the frame energies of successive evaluations (the frames a rank owns).

    A rank of the frame farm evaluates batch after batch of independent frames; with a log the energies of every batch stay
    on the device -- ``values[k]`` (``n_frames`` float64) = the energies of the k-th evaluation since :meth:`reset` -- and are
    exchanged ONCE (``farm.gather_energy_log``: one all-gather of the whole log) instead of once per evaluation.  The graphed
    steps append inside their gather launch -- the thread that writes a frame's energy also writes its log slot
    (``mipme_kspace_forward_args_t.energy_log``, ``mipme_md_args_t.energy_log``, ``mipme_frames_table_energy_log``): no extra
    launch, a replay costs neither the host nor the GPU anything (a separate push node measured +2.0 us on a 58 us step).
    Evaluations that do not end in the gather tail use :meth:`push` (``mipme_energy_log_push``, one small launch).  Slots wrap
    around: the log holds the last ``capacity`` evaluations; ``cursor`` (int32 per frame on the device, all equal) counts them."""

    def __init__(self, capacity: int, n_frames: int, device):
        if capacity < 1 or n_frames < 1:
            raise ValueError("an energy log needs capacity >= 1 and n_frames >= 1")
        self.capacity, self.n_frames = int(capacity), int(n_frames)
        self.values = torch.zeros((self.capacity, self.n_frames), dtype=torch.float64, device=device)
        self.cursor = torch.zeros((self.n_frames,), dtype=torch.int32, device=device)

    def push(self, energies: torch.Tensor) -> None:
        """Append ``energies`` (``n_frames`` reals on the log's device) -- one launch on the current stream, capturable."""
        if energies.numel() != self.n_frames or not energies.is_contiguous():
            raise ValueError(f"the log holds {self.n_frames} energies per evaluation, got a tensor of {tuple(energies.shape)}")
        _lib.require_device(energies, "energies")
        with _lib.on_device(energies.device):
            _lib.check(_lib.load().mipme_energy_log_push(
                _lib.current_stream(energies.device), _lib.dtype_code(energies.dtype), self.n_frames, energies.data_ptr(),
                self.values.data_ptr(), self.cursor.data_ptr(), self.capacity))

    def reset(self) -> None:
        """Start a new log (asynchronous, on the current stream)."""
        self.cursor.zero_()

    def count(self) -> int:
        """Evaluations pushed since :meth:`reset` (synchronises)."""
        return int(self.cursor[0].item())


def _as_energy_log(energy_log, n_frames, device):
    if energy_log is None or isinstance(energy_log, EnergyLog):
        if energy_log is not None and energy_log.n_frames != n_frames:
            raise ValueError(f"the energy log holds {energy_log.n_frames} energies per evaluation, the step produces {n_frames}")
        return energy_log
    return EnergyLog(int(energy_log), n_frames, device)


class GraphedEnergyForces:
    """``E, F = step(positions)`` with ``E = sum_i q_i V_i`` and ``F = -dE/dpositions``, replayed from a HIP graph.

    :param calculator: a :class:`PMECalculator` / :class:`P3MCalculator`
    :param charges, cell, positions, neighbor_indices, neighbor_shifts: tensors on the GPU; ``positions`` only
        provides the shape/dtype and the values for the warm-up.
    :param cell_gradient: also return ``dE/dcell`` (3,3) from every call (the virial is ``-cell.T @ dE/dcell``): the co-scheduled
        pair sum, the x stage of the convolution and the gather leave partial sums behind and ONE more single-workgroup launch
        assembles them (``mipme_kspace_forward_args_t.out_grad_cell``); cases those kernels do not cover (stored
        distances, non-integer shifts) go through the calculator's general autograd nodes instead -- same numbers
    :param charge_gradient: also return ``dE/dcharges`` (N,1) from every call (``= 2 V``, written by the gather launch).  With
        both flags a call returns ``E, F, dE/dq, dE/dcell`` -- the whole first-order autograd contract of the reference
        (``tests/calculators/test_workflow.py:164-192``) from one graph replay
    :param store_distances: keep the pair distances of the last evaluation in ``self.distances`` (P,) -- written by the pair
        kernel as a by-product; off by default: the kernel then forms them in registers only (19 MB less per step at 4.76 M
        pairs, and the packed fp32 body of the pair sum applies)
    :param neighbors: instead of ``neighbor_indices`` / ``neighbor_shifts``: a cutoff (float, skin included) or a
        :class:`~torchpme_amd.neighbors.NeighborStream`.  The object then owns a device neighbour list in the pair kernels' own
        format, built from ITS positions buffer, and :meth:`refresh` rebuilds it in place by replaying a second captured graph
        (cell-list binning + the walk that writes the rows): no list tensors, no sort, no re-capture of the step -- the MD form
        of the reference's "new list every call" (``examples/02-neighbor-lists-usage.py:97-164``).
    :param periodic: per-axis periodicity of the neighbour list made for ``neighbors=<cutoff>``
    :param slab_correction: add the 2-D periodic (slab) term of the reference (``potentials/coulomb.py:6-40``) for the one axis
        that ``periodic`` marks as not periodic: potentials, energy, forces, ``dE/dcharges`` and ``dE/dcell`` then describe a
        system that repeats in the other two directions only.  The term rides in the gather launch of the step (one small
        launch ahead of the spread forms the moments ``sum q z`` and ``sum q z^2``); the axis is fixed here, so a replay has no
        host round trip.  ``periodic`` must have exactly two true entries and the potential must be 1/r.  The mesh part stays
        periodic along that axis too: leaving a vacuum gap in the cell is the caller's business, as in the reference.  Off by
        default -- ``periodic`` alone only shapes the neighbour list
    :param live_bins: (``neighbors=`` form) also keep the atom -> mesh-brick bookkeeping across steps and rebuild it in
        :meth:`refresh`, evaluating every mesh weight on the fly from the current positions (``mipme_md_step``: five launches
        per step instead of six, no per-step binning pass, no per-brick candidate scan).  Valid while no atom has moved more
        than ONE MESH POINT since the last refresh -- :attr:`max_displacement` is that distance in the units of the cell;
        compare it with the skin in ``neighbors`` (a refresh criterion of skin / 2 can exceed it on a fine mesh).  Every step
        checks the margin on the device.  A step that violates it returns ``NaN`` as its energy (its other results are
        invalid too) and the next use of the object raises; ``step(positions, check=True)`` looks at the flag before it
        returns -- one stream synchronisation -- and, on a violation, refreshes the neighbour structures and evaluates again,
        so that what it returns is always valid.  In this mode the charges live in the object's records: change them with
        :meth:`set_charges`.  Default: on where the kernels cover the case (mesh calculators with 1/r or 1/r^6).
    :param energy_log: an :class:`EnergyLog` (or a capacity, for a new one: ``self.energy_log``) that every replay appends its
        energy to -- one more node at the end of the captured graph (frame farm: one exchange for many evaluations)
    :param epilogue: ``epilogue(step)`` is called once, INSIDE the capture, after everything else: whatever it launches on the
        current stream (e.g. an RCCL collective on ``step.energy``) becomes the tail of the replayed graph
    """

    def __init__(self, calculator, charges, cell, positions, neighbor_indices=None, neighbor_shifts=None, warmup: int = 3,
                 cell_gradient: bool = False, store_distances: bool = False, neighbors=None,
                 periodic=(True, True, True), live_bins: bool | None = None, charge_gradient: bool = False,
                 energy_log=None, epilogue=None, slab_correction: bool = False):
        _refuse_spline(calculator, "GraphedEnergyForces" + (" (`neighbors=` included)" if neighbors is not None else ""))
        self.calc = calculator
        self._slab_axis = self._periodic = None
        if slab_correction:
            flags = [bool(p) for p in periodic]
            if len(flags) != 3 or sum(flags) != 2:
                raise ValueError(f"`slab_correction` needs exactly two periodic axes, got periodic={tuple(flags)}")
            _check_slab_potential(calculator.potential)
            self._slab_axis = flags.index(False)
            # the calculator looks the axis up per (tensor, version): the warm-up pays the one host copy, the capture none
            self._periodic = torch.tensor(flags, dtype=torch.bool, device=positions.device)
        self.energy_log = _as_energy_log(energy_log, 1, positions.device)
        self._epilogue = epilogue
        self.store_distances = bool(store_distances)
        self.charge_gradient = bool(charge_gradient)
        self.stream = None
        if neighbors is not None:
            if neighbor_indices is not None or neighbor_shifts is not None:
                raise ValueError("give either `neighbors` or `neighbor_indices` / `neighbor_shifts`")
            if store_distances:
                raise ValueError("a device neighbour stream has no pair order to store distances in")
        elif neighbor_indices is None or neighbor_shifts is None:
            raise ValueError("`neighbor_indices` and `neighbor_shifts` (or `neighbors`) are required")
        self.q = charges.detach()
        #: with ``cell_gradient=True`` every call also returns dE/dcell (3,3) -- the virial is ``-cell.T @ dE/dcell``
        self.cell_gradient = bool(cell_gradient)
        self.cell = cell.detach().clone() if cell_gradient else cell.detach()
        self.pos = positions.detach().clone().requires_grad_(True)
        device = positions.device
        # seeding the backward pass with -1 makes ``pos.grad`` the forces directly (no fill and no negation kernel); the
        # derivatives w.r.t. charges and cell are asked of the same gather tail with a seed of their own (+1)
        self._minus_one = torch.tensor(-1.0, dtype=positions.dtype, device=device)
        self._one = torch.tensor(1.0, dtype=positions.dtype, device=device)
        self._fused_contract = True  # False: charges / cell gradients through the general autograd nodes (see _capture)
        self.charge_grad = self.cell_grad = None
        self._warmup = max(1, warmup)
        self.refresh_graph = None
        self._live = None
        if neighbors is not None and live_bins is not False and hasattr(calculator, "_kspace_setup") \
                and calculator.potential.smearing is not None:
            try:
                live = _LiveStep(calculator, self.q, self.cell, self.pos, self.charge_gradient, self.cell_gradient,
                                 slab_axis=self._slab_axis)
                live.rebin()  # trial: a very non-uniform system overflows the per-brick lists -> keep the binned step
                torch.cuda.current_stream(device).synchronize()
                live.check()
                self._live = live
                # the records are the atoms' storage from here on: `pos` is their (N, 3) view
                self.pos = live.rec[:, :3]
            except (NotImplementedError, RuntimeError):
                if live_bins:
                    raise
                self._live = None
        if neighbors is not None:
            from .neighbors import NeighborStream

            if isinstance(neighbors, NeighborStream) and self._live is not None:
                raise ValueError("with live bins the neighbour stream is built on the object's own records: pass the cutoff")
            if isinstance(neighbors, NeighborStream):
                if neighbors.n_atoms != self.pos.shape[0] or neighbors.dtype != self.pos.dtype:
                    raise ValueError("`neighbors` was built for other positions")
                self.stream = neighbors
                self.stream.positions = self.pos  # from now on the list is rebuilt from the graph's own buffer
                self.stream.update()
            else:
                self.stream = NeighborStream(self.pos, self.cell, float(neighbors), periodic=periodic)
            self.stream.check(synchronize=True)
            self._capture_refresh()
            self._capture(self.stream.indices, None)
        else:
            self._capture(neighbor_indices, neighbor_shifts)

    # ---- device neighbour list --------------------------------------------------------------------------------------------
    def _capture_refresh(self):
        if self._live is not None:
            self._live.rows = (self.stream.row_ptr, self.stream.words, 2 | _lib.ROWS_PADDED)
        self.refresh_graph = _capture_graph(self.pos.device, self._refresh_eager, self._refresh_eager)

    def _refresh_eager(self):
        self.stream.update()
        if self._live is not None:
            self._live.rebin()

    def refresh(self, positions: torch.Tensor | None = None, check: bool = False) -> None:
        """Rebuild the neighbour list from the current positions, in place (``neighbors=`` form only): one graph replay --
        binning, the walk that writes the rows, the status report --, after which the step graph reads the new list at the
        same addresses.  ``check=True`` waits for it and handles a row that outgrew its capacity (larger buffers, both
        graphs captured again); otherwise the status word is looked at when the object is next used."""
        if self.stream is None:
            raise RuntimeError("refresh() needs the `neighbors=` form; use recapture() with a new list otherwise")
        self._deferred_check()
        if positions is not None:
            with torch.no_grad():
                self.pos.copy_(positions)
        self.refresh_graph.replay()
        if check:
            torch.cuda.current_stream(self.pos.device).synchronize()
            self._deferred_check(recover=True)

    def _deferred_check(self, recover: bool = False):
        if self._live is not None:
            self._live.check()
        st = self.stream
        if st is None or not int(st._host_np[1]):
            return
        if recover and int(st._host_np[1]) == 1:  # only a row overflow: grow, capture again, rebuild
            st.grow()
            st.check(synchronize=True)
            self._capture_refresh()
            self._capture(st.indices, None)
            return
        st.check()

    def recapture(self, neighbor_indices, neighbor_shifts, positions: torch.Tensor | None = None) -> None:
        """New neighbour list (e.g. after the atoms moved by more than the skin): rebuild the pair topology and capture the
        step again; positions, cell and charges buffers are kept."""
        if positions is not None:
            with torch.no_grad():
                self.pos.copy_(positions)
        self._capture(neighbor_indices, neighbor_shifts)

    def _capture_live(self):
        self._live.log = None  # (a re-capture after an overflow warms up again: those evaluations are not the caller's)

        def warm_up():  # (the plan allocates its scratch on first use)
            for _ in range(self._warmup):
                self._live.step()

        def between():
            self._keepalive = [self._live, self.stream, getattr(self.calc, "_cache", None)]
            self._live.log = self.energy_log  # (from here on: the gather of the step appends its energy to the log)

        def body():
            self._live.step()
            self.energy = self._live.energy
            if self._epilogue is not None:
                self._epilogue(self)

        self.graph = _capture_graph(self.pos.device, warm_up, body, between)
        self.energy, self.forces, self.distances = self._live.energy, self._live.grad, None
        self.charge_grad = self._live.grad_q
        self.cell_grad = None if self._live.grad_cell is None else self._live.grad_cell[18:27].view(3, 3)
        self.pairs, self.shifts = self.stream.indices, None

    def _capture(self, neighbor_indices, neighbor_shifts):
        if self._live is not None:
            return self._capture_live()
        calculator, device, warmup = self.calc, self.pos.device, self._warmup
        self.pairs = neighbor_indices
        self.shifts = None if neighbor_shifts is None else neighbor_shifts.to(self.pos.dtype).contiguous()

        def warm_up():  # plans, topology, filter caches get built
            for it in range(max(1, warmup) + 1):
                self.pos.grad = self.cell.grad = self.q.grad = None
                self._eval()
                if it == 0 and (self.charge_gradient or self.cell_gradient) and self._fused_contract:
                    # did the gather tail take the request (seed_promise(charges=, cell=))?  Otherwise the general nodes:
                    # charges / cell become leaves and autograd differentiates w.r.t. them
                    t = self._tail
                    ok = t is not None and (t["grad_q"] is not None or not self.charge_gradient) and (
                        t["grad_cell"] is not None or not self.cell_gradient)
                    if not ok:
                        self._fused_contract = False
                        if self.charge_gradient:
                            self.q = self.q.clone().requires_grad_(True)
                        if self.cell_gradient:
                            self.cell.requires_grad_(True)

        def between():
            self.pos.grad = self.cell.grad = self.q.grad = None
            # The captured graph holds raw pointers into buffers that were built during the warm-up and live in caches: the
            # transposed pair list (+ packed shifts), the calculator's filter table, the reduction scratch.  Keep them alive
            # for the lifetime of the graph, whatever the caches evict later.
            topo = ops.get_topology(self.pairs, self.pos.shape[0]) if ops.PAIR_MODE == "rows" else None
            self._keepalive = [
                topo,
                getattr(calculator, "_cache", None),
                ops._dot_scratch(device, self.q.data_ptr()),
            ]
            if isinstance(topo, ops.PairTopology):
                # the entry streams are single-slot caches keyed by the shifts tensor: an eager call with the same pairs and other
                # shifts would replace the slot and free the buffer the graph reads -- pin the concrete tensors
                self._keepalive += [topo.row_ptr, topo.entries, topo._ent32, topo._ent_sh, topo._packed, topo._pair_sh]
            elif topo is not None:
                self._keepalive += [self.stream.row_ptr, self.stream.words]

        def body():
            self.energy = self._eval(log=self.energy_log)
            self.forces = self.pos.grad
            if self.energy_log is not None and not (self._tail is not None and self._tail["logged"]):
                self.energy_log.push(self.energy.reshape(1))  # (no gather tail in this step: one more node)
            if self._epilogue is not None:
                self._epilogue(self)
            if self._fused_contract:
                t = self._tail
                self._keepalive.append(t)  # (G_deriv, cell_work, the output buffers)
                self.charge_grad = t["grad_q"] if self.charge_gradient else None
                self.cell_grad = t["grad_cell"][18:27].view(3, 3) if self.cell_gradient else None
            else:
                # the backward pass is seeded with -1 (so that pos.grad is the force): undo the sign for charges and cell
                self.charge_grad = -self.q.grad if self.charge_gradient else None
                self.cell_grad = -self.cell.grad if self.cell_gradient else None

        self.graph = _capture_graph(device, warm_up, body, between)

    def _eval(self, log=None):
        # the pair kernel of the calculator forms the distances itself (no separate pass over the list); "virtual": in
        # registers only, True: stored as a by-product
        if self.stream is not None:
            d = self.stream.distances(self.pos, self.cell)
        else:
            d = ops.pair_distances(self.pos, self.pairs, self.cell, self.shifts,
                                   deferred=True if self.store_distances else "virtual")
        #: the pair distances of the last evaluation (P,) with ``store_distances=True``, else None
        self.distances = d.detach() if self.store_distances else None
        # the backward pass below is seeded with self._minus_one: promise that to the forward, whose gather then writes the
        # forces themselves (energy reduction and force assembly ride in the gather launch, see ops.SEED_PROMISE) -- and, on
        # request, dE/dcharges and dE/dcell with a seed of +1
        fused = self._fused_contract
        with ops.seed_promise(self._minus_one, charges=fused and self.charge_gradient, cell=fused and self.cell_gradient,
                              aux_seed=self._one, energy_log=log):
            if self._periodic is None:
                V = self.calc(self.q, self.cell, self.pos, self.pairs, d)
            else:
                V = self.calc(self.q, self.cell, self.pos, self.pairs, d, periodic=self._periodic)
        self._tail = getattr(V.grad_fn, "tail", None)
        E = ops.weighted_sum(V, self.q)
        E.backward(self._minus_one)
        return E.detach()

    @property
    def max_displacement(self):
        """How far an atom may move between two :meth:`refresh` calls of the live-bin step (one mesh point, in the units of the
        cell); ``None`` for the binned step, which re-bins every call."""
        return None if self._live is None else self._live.max_displacement

    def set_charges(self, charges: torch.Tensor) -> None:
        """New charge values (same shape) for the following steps.  The binned step reads the tensor given at construction, so
        writing into that tensor has the same effect there; the live-bin step keeps the charges in its atom records."""
        with torch.no_grad():
            if self._live is not None:
                self._live.rec[:, 3] = charges.detach()[:, 0]
            self.q.copy_(charges.detach())

    def __call__(self, positions: torch.Tensor | None = None, check: bool = False):
        """``E, F`` (+ ``dE/dcharges`` with ``charge_gradient``, + ``dE/dcell`` with ``cell_gradient``, in that order) of the
        current -- or the given -- positions: one graph replay.  The returned tensors are the graph's own buffers.

        ``check=True`` (live-bin step): wait for the step and look at its margin flag; if an atom had moved more than one mesh
        point since the last refresh, :meth:`refresh` (neighbour list and bins from the current positions) and evaluate again
        before returning -- the results are then valid whatever the atoms did, at the price of one synchronisation per call."""
        self._deferred_check()
        self.calc.check()  # a NaN a previous replay met (pinned word, no synchronisation)
        if positions is not None:
            with torch.no_grad():
                self.pos.copy_(positions)
        self.graph.replay()
        if check and self._live is not None:
            torch.cuda.current_stream(self.pos.device).synchronize()
            if self._live.moved():
                self.refresh(check=True)
                self.graph.replay()
                torch.cuda.current_stream(self.pos.device).synchronize()
                self._deferred_check()
        out = (self.energy, self.forces)
        if self.charge_gradient:
            out += (self.charge_grad,)
        if self.cell_gradient:
            out += (self.cell_grad,)
        return out


class _FramesFunction(torch.autograd.Function):
    """Energies of all frames of a :class:`GraphedFrameBatch` as one autograd node: forward = the batched pipeline
    (``mipme_frames_forward``), backward = the batched force assembly (``mipme_frames_backward``)."""

    @staticmethod
    def forward(ctx, batch, *positions):
        batch._launch_forward()
        ctx.batch = batch
        return batch.energies.detach()  # a fresh tensor object per call (the buffer itself is persistent)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        batch = ctx.batch
        # seeded with the batch's own -1 vector the gradients are already there (written by the gather's tail of the forward
        # pass); fresh aliases, so that the accumulation into positions.grad takes the buffers instead of copying them
        if g.data_ptr() != batch._minus_one.data_ptr():
            batch._launch_backward(g.contiguous())
        return (None, *(b.detach() for b in batch._grad_pos))


class GraphedFrameBatch:
    """Energy + forces of several independent frames (the frames a rank owns) with ONE launch per kernel of the
    pipeline -- ``blockIdx.y`` = frame (``mipme_frames_forward / backward``, csrc/bricks.hip) -- replayed from one HIP graph.

    The frames may differ in atoms, cell and neighbour list; they must give the same mesh dimensions and share the
    calculator (P3M / PME with 1/r or 1/r^6), dtype and device.  ``energies, forces = batch(positions_list=None)``:
    ``energies`` (F,), ``forces`` a list of (N_f, 3) tensors (static buffers of the graph: read them before the next call).
    ``charge_gradient`` / ``cell_gradient`` add ``dE/dcharges`` and ``dE/dcell`` of every frame to what a call returns, from the
    same replay -- the first-order contract of :class:`GraphedEnergyForces` for a whole batch.

    :param calculator: a :class:`PMECalculator` / :class:`P3MCalculator`
    :param frames: sequence of ``(charges, cell, positions, neighbor_indices, neighbor_shifts)``
    :param store_distances: keep every frame's pair distances in ``self.distances[f]`` (by-product of the pair kernel; needs a
        list ordered by its first index); off by default, see :class:`GraphedEnergyForces`
    :param energy_log: an :class:`EnergyLog` (or a capacity) that every replay appends its F energies to, see there
    :param epilogue: ``epilogue(batch)``, called once inside the capture after everything else (see :class:`GraphedEnergyForces`)
    :param charge_gradient: also return ``dE/dcharges`` of every frame -- a list of (N_f, 1) static buffers, ``= 2 V``, written
        by the gather launch (``self.charge_grads``)
    :param cell_gradient: also return ``dE/dcell`` at fixed Cartesian positions of every frame as ONE (F, 3, 3) tensor
        (``self.cell_grads``; the virial of frame f is ``-cell_f.T @ cell_grads[f]``): the pair sum, the x stage and the gather of
        the batch leave partial sums behind, one launch of cell riders (riders x frames) and one single-workgroup-per-frame launch
        assemble them (``mipme_frames_table_contract`` / ``mipme_frames_step``).  Needs cell shifts that fit the 4-byte entries
        in every frame and excludes ``store_distances``: both are refused here, by ``ValueError``.  With both flags a call
        returns ``energies, forces, charge_grads, cell_grads`` -- the order of :class:`GraphedEnergyForces`
    :param periodic: with ``slab_correction=True``: which cell vectors the frames repeat along -- one triple of booleans for
        every frame, or a sequence of F triples, one per frame.  A triple has exactly two true entries (a 2-D periodic frame; the
        third axis is its own, frames of one batch may differ in it) or three (a fully periodic frame, which gets no term)
    :param slab_correction: add the 2-D periodic (slab) term of the reference (``potentials/coulomb.py:6-40``) to every frame that
        ``periodic`` marks as a slab: its energy, forces, ``charge_grads``, ``cell_grads`` and ``energy_log`` entries then describe
        a system that repeats in two directions only, as with :class:`GraphedEnergyForces`.  One launch ahead of the binning
        forms the moments ``sum q``, ``sum q z``, ``sum q z^2`` of all frames (blocks x frames), and the gather and the cell
        finalize launch run compiled with the term (``mipme_frames_table_slab`` / ``mipme_frames_slab_step``).  The potential
        must be 1/r with a smearing.  The batch takes explicit pair lists, so ``periodic`` has no list to shape: it is refused
        without ``slab_correction=True``.  A batch whose frames are all fully periodic is built and launched as without the
        keywords
    :param follow_cells: the cells become a replay input (NPT, cell relaxation, strain scans, finite-difference stress): the batch
        owns ``self.cells`` (F, 3, 3) -- the input buffer --, a private validated copy that the pair rows read, and ``self.status``
        (F,) int32.  ``batch(positions, cells=...)`` copies the cells in, makes ONE launch (``mipme_frames_cells``: it inverts
        every cell in float64, patches the geometry of the device-resident table and rebuilds every frame's G(k) and derivative
        table) and replays the unchanged graph: no host read, nothing captured again.  ``update_cells()`` makes the launch alone,
        for callers whose own kernel (a barostat) wrote into ``self.cells``.  The mesh dimensions stay those of the construction
        (``self.ns``): ``dE/dcell`` is "at fixed Cartesian positions, at the frozen mesh", which is what makes E a smooth function
        of the cell.  ``status[f]`` bit 0: the mesh rule would give frame f another mesh at its present cell (results are still
        those of the frozen mesh; build a new batch when the accuracy matters; :meth:`mesh_matches` decides the same on the host).
        Bit 1: the cell is singular or not finite -- the frame keeps the geometry of its last valid cell, its energy comes out as
        NaN and its other outputs are invalid; the next valid cell recovers it.  The neighbour lists stay the caller's business
        (their skin has to cover the strain).  A batch of one frame is the variable-cell form of :class:`GraphedEnergyForces`
    """

    def __init__(self, calculator, frames, warmup: int = 2, store_distances: bool = False, energy_log=None, epilogue=None,
                 charge_gradient: bool = False, cell_gradient: bool = False, periodic=None, slab_correction: bool = False,
                 follow_cells: bool = False):
        _refuse_spline(calculator, "GraphedFrameBatch")
        frames = list(frames)
        slab = self._slab_codes(calculator, len(frames), periodic, slab_correction)
        lib = _lib.load()
        self.calc = calculator
        self.store_distances = bool(store_distances)
        self.charge_gradient, self.cell_gradient = bool(charge_gradient), bool(cell_gradient)
        if self.cell_gradient and self.store_distances:
            raise ValueError("GraphedFrameBatch: `cell_gradient` and `store_distances` exclude each other (the pair kernels "
                             "that form the cell sums keep the distances in registers)")
        F = self.n_frames = len(frames)
        if F == 0:
            raise ValueError("no frames")
        q0, _, p0, _, _ = frames[0]
        device, dtype = p0.device, p0.dtype
        _lib.require_device(p0, "positions")
        self.device, self.dtype = device, dtype
        dt = self._dt = _lib.dtype_code(dtype)
        self._pot = calculator.potential._descriptor()
        full = bool(calculator.full_neighbor_list)
        self.pos, self._keep, geoms, Gs = [], [], [], []
        for q, cell, pos, pairs, shifts in frames:
            if q.shape[1] != 1:
                raise ValueError("the frames path handles a single charge channel")
            geom, G = calculator._kspace_setup(cell, dtype, device, speculate=False)
            geoms.append(geom)
            Gs.append(G.reshape(-1))
        ns = geoms[0].ns
        if any(g.ns != ns for g in geoms):
            raise ValueError(f"all frames must give the same mesh, got {[g.ns for g in geoms]}")
        self.ns = ns
        M, Mh = geoms[0].n_mesh, geoms[0].n_half
        cdtype = _lib.complex_dtype(dtype)
        self._G = torch.stack(Gs).contiguous()
        self._rho = torch.empty((F,) + ns, dtype=dtype, device=device)
        self._phi = torch.empty((F,) + ns, dtype=dtype, device=device)
        self._hat = torch.empty((F, Mh), dtype=cdtype, device=device)
        self._dc = torch.empty((F,), dtype=dtype, device=device)
        self.energies = torch.empty((F,), dtype=dtype, device=device)
        self._plan = _lib.FFTPlan(device, dtype, ns, F)
        self._frames = (_lib.Frame * F)()
        self._minus_one = torch.full((F,), -1.0, dtype=dtype, device=device)
        self._grad_pos, self.distances = [], []
        self.follow_cells = bool(follow_cells)
        self.cells = self.status = self._cells_valid = None
        if self.follow_cells:
            #: (F, 3, 3): the cells the next ``update_cells()`` / ``batch(cells=...)`` evaluates; ``status``: (F,) int32, see the class
            self.cells = torch.stack([cell.detach().to(dtype).reshape(3, 3) for _, cell, _, _, _ in frames]).contiguous()
            self._cells_valid = self.cells.clone()  # what the pair rows read: written by the cells launch, for valid cells only
            self.status = torch.zeros((F,), dtype=torch.int32, device=device)
        compact_ok, ent_streams = True, []
        for k, (q, cell, pos, pairs, shifts) in enumerate(frames):
            N, P = pos.shape[0], pairs.shape[0]
            p = pos.detach().clone().contiguous().requires_grad_(True)
            qc = q.detach().reshape(-1).contiguous()
            cl = self._cells_valid[k] if self.follow_cells else cell.detach().to(dtype).contiguous()
            sh = shifts.to(dtype).contiguous()
            topo = ops.get_topology(pairs, N)
            ent_sh, fmt = topo.entries_with_shifts(sh, shifts, table=True)
            if ent_sh is None or fmt != 1:
                raise ValueError(f"frame {k}: cell shifts must be integers in [-3, 3] for the frames path")
            ent32 = topo.compact_entries(sh, shifts)  # 4-byte entries when every frame has them
            compact_ok = compact_ok and ent32 is not None
            ent_streams.append((ent_sh, ent32))
            md = geoms[k].desc(1)
            nbytes = lib.mipme_atom_bins_bytes(C.byref(md), N, dt)
            if nbytes <= 0:
                raise ValueError(f"frame {k}: mesh {ns} is outside the brick kernels' range")
            nb = ((ns[0] + 7) // 8) * ((ns[1] + 7) // 8) * ((ns[2] + 7) // 8)
            buf = dict(
                bins=torch.empty((nbytes,), dtype=torch.uint8, device=device),
                # (brick counters + the plane lists' counters where the plane spread applies: mipme_frame_t.counter_ints)
                counters=torch.zeros((max(nb + 1, int(lib.mipme_frames_counter_ints(C.byref(md), N, dt))),), dtype=torch.int32,
                                     device=device),
                records=torch.empty((N, 4), dtype=dtype, device=device),
                out=torch.empty((N,), dtype=dtype, device=device),
                force=torch.empty((N, 3), dtype=dtype, device=device),
                field=torch.empty((N, 3), dtype=dtype, device=device),
                grad=torch.empty((N, 3), dtype=dtype, device=device),
                dist=(torch.empty((P,), dtype=dtype, device=device)
                      if self.store_distances and topo.sorted_by_first and P > 0 else None),
            )
            f = self._frames[k]
            f.n_atoms, f.positions, f.charges, f.cell, f.mesh = N, p.data_ptr(), qc.data_ptr(), cl.data_ptr(), md
            f.atom_bins, f.brick_counters = buf["bins"].data_ptr(), buf["counters"].data_ptr()
            f.counter_ints = int(buf["counters"].numel())
            f.row_ptr, f.entries_shift, f.entries = topo.row_ptr.data_ptr(), ent_sh.data_ptr(), topo.entries.data_ptr()
            f.full_list, f.shift_format = int(full), int(fmt)
            f.records = buf["records"].data_ptr()
            f.rho_mesh, f.phi_mesh, f.dc = self._rho[k].data_ptr(), self._phi[k].data_ptr(), self._dc[k:].data_ptr()
            f.out, f.force, f.field = buf["out"].data_ptr(), buf["force"].data_ptr(), buf["field"].data_ptr()
            f.dist_out = _lib.ptr(buf["dist"])
            f.energy, f.grad_positions = self.energies[k:].data_ptr(), buf["grad"].data_ptr()
            # energy + forces of the frame in the gather launch, seeded with the -1 the backward pass of _eval() uses
            f.use_tail, f.grad_seed = 1, self._minus_one[k:].data_ptr()
            self.pos.append(p)
            self._grad_pos.append(buf["grad"])
            self.distances.append(buf["dist"])
            self._keep.append((qc, cl, sh, topo, ent_sh, ent32, buf, pairs))
        if compact_ok:  # the same (compact) entry format for every frame
            for k, (_, ent32) in enumerate(ent_streams):
                self._frames[k].entries_shift, self._frames[k].shift_format = ent32.data_ptr(), 2
        elif self.cell_gradient:
            bad = [k for k, (_, ent32) in enumerate(ent_streams) if ent32 is None]
            raise ValueError(f"GraphedFrameBatch: `cell_gradient` needs 4-byte pair entries in every frame; the cell shifts or "
                             f"the atom count of frame(s) {bad} do not fit them")
        nbytes = lib.mipme_frames_table_bytes(dt, F)
        host = np.zeros((nbytes,), dtype=np.uint8)
        _lib.check(lib.mipme_frames_table_build(dt, F, self._frames, C.byref(self._pot), host.ctypes.data, nbytes))
        self.charge_grads = self.cell_grads = self._cell_work = None
        if self.charge_gradient or self.cell_gradient:
            # the rest of the first-order contract from the same launches: seeded with +1 while the positions' seed is -1
            self._one = torch.ones((1,), dtype=dtype, device=device)
            ptrs = lambda tensors: (C.c_void_p * F)(*(t.data_ptr() for t in tensors))  # noqa: E731
            gq = gc = None
            G_deriv, G_deriv_stride, work_stride = None, 0, 0
            if self.charge_gradient:
                self.charge_grads = [torch.empty((f.n_atoms, 1), dtype=dtype, device=device) for f in self._frames]
                gq = ptrs(self.charge_grads)
            if self.cell_gradient:
                self._grad_cell = torch.empty((F, 27), dtype=dtype, device=device)  # mesh part, pair part, sum per frame
                self.cell_grads = self._grad_cell[:, 18:27].view(F, 3, 3)
                self._G_deriv = torch.stack([ops.filter_derivative(g, self._pot, dtype, device).reshape(-1) for g in geoms]).contiguous()
                G_deriv, G_deriv_stride = self._G_deriv.data_ptr(), self._G_deriv.shape[1]
                work_stride = max(int(lib.mipme_frames_cell_work(C.byref(f.mesh), f.n_atoms)) for f in self._frames)
                self._cell_work = torch.empty((F * work_stride,), dtype=torch.float64, device=device)
                gc = ptrs(self._grad_cell)
            _lib.check(lib.mipme_frames_table_contract(
                dt, F, self._frames, C.byref(self._pot), host.ctypes.data, nbytes, gq, gc, G_deriv, G_deriv_stride,
                _lib.ptr(self._cell_work), work_stride, self._one.data_ptr()))
        #: per frame: the non-periodic axis of a slab frame, ``None`` for a fully periodic one (``None`` as a whole: no slab term)
        self.slab_axes = None if slab is None else [c - 1 if c else None for c in slab]
        self._slab = self._slab_work = None
        if slab is not None:
            self._slab = (C.c_int32 * F)(*slab)
            self._slab_stride = int(lib.mipme_frames_slab_work())
            self._slab_work = torch.zeros((F * self._slab_stride,), dtype=torch.float64, device=device)
            _lib.check(lib.mipme_frames_table_slab(dt, F, self._frames, C.byref(self._pot), host.ctypes.data, nbytes, self._slab,
                                                   self._slab_work.data_ptr(), self._slab_stride))
        self.energy_log = _as_energy_log(energy_log, F, device)
        if self.energy_log is not None:  # every frame's gather tail also writes its slot of the log (no extra launch)
            _lib.check(lib.mipme_frames_table_energy_log(dt, F, host.ctypes.data, nbytes, self.energy_log.values.data_ptr(),
                                                         self.energy_log.cursor.data_ptr(), self.energy_log.capacity))
        if self.follow_cells:  # the status word of every frame on its gather tail (bit 1: the energy becomes NaN)
            _lib.check(lib.mipme_frames_table_cells(dt, F, self._frames, host.ctypes.data, nbytes, self.status.data_ptr()))
        self._table = torch.from_numpy(host).to(device)
        if self.follow_cells:  # from the first replay on the tables are a function of `self.cells` alone
            self.update_cells()

        def warm_up():  # (plans, lazy module loads)
            for _ in range(max(1, warmup)):
                self._eval()

        def body():
            self._eval()
            if epilogue is not None:
                epilogue(self)

        # (the warm-up evaluations appended to the log too: reset it before the capture)
        self.graph = _capture_graph(device, warm_up, body, None if self.energy_log is None else self.energy_log.reset)
        self.forces = [p.grad for p in self.pos]

    @staticmethod
    def _slab_codes(calculator, n_frames, periodic, slab_correction):
        """``mipme_frames_table_slab``'s code per frame (0 = fully periodic, else the non-periodic axis + 1) from the two keywords;
        ``None``: no slab term anywhere in the batch -- the calls and kernels of a batch without the keywords."""
        if not slab_correction:
            if periodic is not None:
                raise ValueError("GraphedFrameBatch: `periodic` only selects the frames and axes of `slab_correction=True` (the batch "
                                 "takes explicit pair lists, there is no neighbour list for it to shape)")
            return None
        if periodic is None:
            raise ValueError("GraphedFrameBatch: `slab_correction` needs `periodic`: one triple of booleans for every frame, or one "
                             "per frame")
        per = list(periodic)
        if len(per) == 3 and all(isinstance(p, (bool, int, np.bool_)) or (torch.is_tensor(p) and p.ndim == 0) for p in per):
            per = [per] * n_frames
        if len(per) != n_frames:
            raise ValueError(f"GraphedFrameBatch: `periodic` must be one triple or one triple per frame ({n_frames}), got {len(per)}")
        codes = []
        for k, triple in enumerate(per):
            flags = [bool(p) for p in triple]
            if len(flags) != 3 or sum(flags) < 2:
                raise ValueError(f"frame {k}: `slab_correction` needs exactly two periodic axes (or three: a fully periodic frame), "
                                 f"got periodic={tuple(flags)}")
            codes.append(0 if all(flags) else flags.index(False) + 1)
        _check_slab_potential(calculator.potential)
        return codes if any(codes) else None

    def _launch_forward(self):
        if self._slab is not None or self.charge_gradient or self.cell_gradient:  # (without flags: the call, and so the kernels, of before)
            with _lib.on_device(self.device):
                a = _lib.FramesStepArgs(
                    plan=self._plan.handle, stream=_lib.current_stream(self.device), dtype=self._dt, n_frames=self.n_frames,
                    frames=self._frames, pot=C.pointer(self._pot), device_table=self._table.data_ptr(), G=self._G.data_ptr(),
                    G_stride=self._G.shape[1], rho_mesh_all=self._rho.data_ptr(), hat_work_all=self._hat.data_ptr(),
                    phi_mesh_all=self._phi.data_ptr(), dc_all=self._dc.data_ptr(), cell_work=_lib.ptr(self._cell_work),
                    cell_gradient=int(self.cell_gradient))
                if self._slab is not None:
                    s = _lib.FramesSlabStepArgs(step=a, slab=self._slab, slab_work=self._slab_work.data_ptr(),
                                                slab_work_stride=self._slab_stride)
                    _lib.check(_lib.load().mipme_frames_slab_step(C.byref(s)))
                else:
                    _lib.check(_lib.load().mipme_frames_step(C.byref(a)))
            return
        with _lib.on_device(self.device):
            _lib.check(_lib.load().mipme_frames_forward(
                self._plan.handle, _lib.current_stream(self.device), self._dt, self.n_frames, self._frames,
                C.byref(self._pot), self._table.data_ptr(), self._G.data_ptr(), self._G.shape[1], self._rho.data_ptr(),
                self._hat.data_ptr(), self._phi.data_ptr(), self._dc.data_ptr()))

    def _launch_backward(self, g):
        with _lib.on_device(self.device):
            _lib.check(_lib.load().mipme_frames_backward(
                _lib.current_stream(self.device), self._dt, self.n_frames, self._frames, self._table.data_ptr(),
                g.data_ptr()))

    def _eval(self):
        for p in self.pos:
            p.grad = None
        E = _FramesFunction.apply(self, *self.pos)
        E.backward(self._minus_one)  # seeded with -1: positions.grad are the forces
        return E

    def _need_follow_cells(self, what):
        if not self.follow_cells:
            raise ValueError(f"GraphedFrameBatch: {what} needs a batch built with follow_cells=True (this one keeps the cells it was "
                             f"built with)")

    def _checked_cells(self, cells):
        """``cells`` as the (F, 3, 3) tensor or the list of F (3, 3) tensors ``torch.stack(..., out=self.cells)`` takes; refused by
        ``ValueError`` before anything changes."""
        F = self.n_frames
        seq = [cells] if torch.is_tensor(cells) else list(cells)
        if not torch.is_tensor(cells) and len(seq) != F:
            raise ValueError(f"GraphedFrameBatch: `cells` must hold one (3, 3) tensor per frame ({F}), got {len(seq)}")
        want = (F, 3, 3) if torch.is_tensor(cells) else (3, 3)
        for c in seq:
            if not torch.is_tensor(c) or tuple(c.shape) != want or c.dtype != self.dtype or c.device != self.cells.device:
                got = (tuple(c.shape), c.dtype, str(c.device)) if torch.is_tensor(c) else type(c).__name__
                raise ValueError(f"GraphedFrameBatch: `cells` must be a {(F, 3, 3)} tensor or {F} tensors of shape (3, 3), dtype "
                                 f"{self.dtype} on {self.cells.device}; got {got}")
        return cells if torch.is_tensor(cells) else seq

    def update_cells(self) -> None:
        """Make the tables of the batch those of ``self.cells`` as it stands on the device (one launch on the current stream; no
        host read).  ``batch(cells=...)`` calls it; call it yourself after writing into ``self.cells`` in place."""
        self._need_follow_cells("update_cells()")
        a = self.__dict__.get("_cells_args")
        if a is None:  # (every pointer in it is a buffer of the object: built once, only the stream is per call)
            G_deriv = self._G_deriv if self.cell_gradient else None
            a = self._cells_args = _lib.FramesCellsArgs(
                dtype=self._dt, n_frames=self.n_frames, frames=self._frames, pot=C.pointer(self._pot),
                device_table=self._table.data_ptr(), cells=self.cells.data_ptr(), cells_valid=self._cells_valid.data_ptr(),
                G=self._G.data_ptr(), G_stride=self._G.shape[1], G_deriv=_lib.ptr(G_deriv),
                G_deriv_stride=0 if G_deriv is None else G_deriv.shape[1], mesh_spacing=float(self.calc.mesh_spacing),
                status=self.status.data_ptr())
        with _lib.on_device(self.device):
            a.stream = _lib.current_stream(self.device)
            _lib.check(_lib.load().mipme_frames_cells(C.byref(a)))

    def mesh_matches(self, cells=None) -> list:
        """Per frame: would the mesh rule give the frozen mesh ``self.ns`` at these cells (default: ``self.cells``)?  Decided on
        the host (this reads the cells back); ``status`` bit 0 says the same on the device."""
        if cells is None:
            self._need_follow_cells("mesh_matches() without `cells`")
            cells = self.cells
        host = [torch.as_tensor(c).detach().to("cpu", torch.float64).numpy() for c in cells]
        if len(host) != self.n_frames:
            raise ValueError(f"GraphedFrameBatch: `cells` must hold one cell per frame ({self.n_frames}), got {len(host)}")
        return [tuple(ops.ns_mesh_from_cell(c, self.calc.mesh_spacing)) == tuple(self.ns) for c in host]

    def __call__(self, positions=None, cells=None):
        if cells is not None:
            self._need_follow_cells("`cells=`")
            cells = self._checked_cells(cells)
        if positions is not None:
            with torch.no_grad():
                for buf, new in zip(self.pos, positions):
                    buf.copy_(new)
        if cells is not None:
            if torch.is_tensor(cells):
                self.cells.copy_(cells)
            else:
                torch.stack(cells, out=self.cells)
            self.update_cells()
        self.calc.check()  # a NaN a previous replay met (pinned word, no synchronisation)
        self.graph.replay()
        out = (self.energies, self.forces)
        if self.charge_gradient:
            out += (self.charge_grads,)
        if self.cell_gradient:
            out += (self.cell_grads,)
        return out


class _ExplicitListStep:
    """What :class:`GraphedCombinedStep` and :class:`GraphedDipoleStep` share: a step (``self._launch()``, every launch on the
    current stream) whose row kernel walks an explicit pair list, captured for that list.  The subclass sets ``device``,
    ``dtype``, ``n_atoms`` and ``_warmup`` before it calls :meth:`_capture`."""

    _pinned = ()  # what else the captured graph holds raw pointers into (the subclass sets it before the first capture)

    def _capture(self, neighbor_indices, neighbor_shifts, copies=()):
        """Pack the list into ``row_ptr`` + 4-byte entries (other | code << 22), copy ``copies`` -- (buffer, new values or
        ``None``) pairs -- and capture the step.  A list the entries do not hold is refused before anything of the object changes:
        the graph it replays, ``pairs`` and the buffers stay as they were."""
        sh = neighbor_shifts.to(self.dtype).contiguous()
        topo = ops.get_topology(neighbor_indices, self.n_atoms)
        ent32 = topo.compact_entries(sh, neighbor_shifts)
        if ent32 is None:
            raise ValueError(f"{type(self).__name__}: the cell shifts must be integers in [-3, 3] (the 4-byte pair entries of the "
                             "row kernel) and the system at most 2^22 atoms")
        with torch.no_grad():
            for buf, new in copies:
                if new is not None:
                    buf.copy_(new)
        self.pairs, self._row_ptr, self._ent32 = neighbor_indices, topo.row_ptr, ent32
        # the captured graph holds raw pointers into cached buffers (the transposed list, the entry stream)
        self._keepalive = [topo, topo.row_ptr, ent32, sh, *self._pinned]
        self.graph = _capture_graph(self.device, self._warm_up, self._launch)

    def _warm_up(self):  # (the plan allocates its scratch on first use)
        for _ in range(self._warmup):
            self._launch()


def _combined_refusal(pot) -> str | None:
    """Why ``combined.plan`` does not serve this combination in the graphed step (``None``: it does)."""
    from .potentials import CombinedPotential, CoulombPotential, InversePowerLawPotential, SplinePotential

    members = list(pot.potentials)
    if len(members) > _lib.COMBINED_MAX_TERMS:
        return f"it has {len(members)} members, the kernels take at most {_lib.COMBINED_MAX_TERMS}"
    for k, m in enumerate(members):
        if isinstance(m, CombinedPotential):
            return f"member {k} is itself a CombinedPotential (nested combinations are not served)"
        if isinstance(m, SplinePotential):
            return f"member {k} is a SplinePotential; the kernels know CoulombPotential and InversePowerLawPotential members"
        if type(m) not in (CoulombPotential, InversePowerLawPotential):
            return (f"member {k} is a {type(m).__name__}; the kernels know exactly CoulombPotential and "
                    "InversePowerLawPotential members")
        if m.exclusion_radius is not None:
            return f"member {k} has an exclusion radius"
    if any(m.smearing is None for m in members):
        return "its members are direct potentials (`smearing=None`): the step is the range-separated mesh calculation"
    return None


class GraphedCombinedStep(_ExplicitListStep):
    """``E, F, dE_dw = step(positions)`` for a calculator with a :class:`~torchpme_amd.CombinedPotential` -- Coulomb +
    dispersion, or any weighted sum of range-separated 1/r^p terms -- replayed from one HIP graph: the MD form of the eager call.

    With ``V`` the potentials the eager calculator returns for the same arguments and ``w`` the potential's ``weights``:
    ``E = sum_a q_a V_a`` (0-dim), ``F = -dE/dpositions`` (N, 3), ``dE_dw = dE/dweights`` (n_terms,) with ``weight_gradient``, and
    behind it ``dE_dq = 2 V`` (N, 1) with ``charge_gradient`` (half lists only).  All of them are buffers of the object,
    overwritten by every call.  Everything is linear in the potential: the mesh part is one pass with the contracted table
    ``sum_t w_t G_t``, the pair part one walk over the rows with ``sum_t w_t v_t(d)``, and ``dE/dw_t`` is the energy of member t
    alone (``mipme_combined_step``, csrc/combined_step.hip).

    The weights are followed without a new capture: every call copies ``calculator.potential.weights`` into a device buffer of the
    object on the current stream just before the replay -- one small device copy, no host read -- so a step of an optimizer on
    the weights is seen by the next call.

    :param calculator: a :class:`PMECalculator` / :class:`P3MCalculator` whose potential is a combination ``combined.plan``
        serves with range-separated members: exactly ``CoulombPotential`` / ``InversePowerLawPotential`` members without an
        exclusion radius, at most 8 of them
    :param charges: (N, 1); the step reads this tensor in every call
    :param neighbor_indices, neighbor_shifts: an explicit half or full list (``calculator.full_neighbor_list``) whose cell shifts
        are integers in [-3, 3]
    :param weight_gradient: also return ``dE/dweights`` (one pass over the transformed charge mesh more per call)
    :param charge_gradient: also return ``dE/dcharges``; refused for a full list, which need not be symmetric
    """

    def __init__(self, calculator, charges, cell, positions, neighbor_indices, neighbor_shifts, weight_gradient: bool = True,
                 charge_gradient: bool = False, warmup: int = 3):
        from . import combined
        from .potentials import CombinedPotential

        pot = getattr(calculator, "potential", None)
        if not isinstance(pot, CombinedPotential):
            raise TypeError(f"GraphedCombinedStep serves a calculator with a CombinedPotential, got a {type(pot).__name__}: "
                            "use GraphedEnergyForces for a single potential")
        why = _combined_refusal(pot)
        self._plan_c = combined.plan(pot) if why is None else None
        if why is None and self._plan_c is None:
            why = "its members are not all range separated or all direct"
        if why is not None:
            raise TypeError(f"GraphedCombinedStep does not serve this CombinedPotential: {why}; call the calculator eagerly")
        if not hasattr(calculator, "mesh_spacing"):
            raise TypeError(f"GraphedCombinedStep needs a PMECalculator or a P3MCalculator, got a {type(calculator).__name__}")
        if charges.dim() != 2 or charges.shape[1] != 1:
            raise ValueError(f"GraphedCombinedStep handles a single charge channel, got charges of shape {tuple(charges.shape)}")
        for t, name in ((positions, "positions"), (charges, "charges"), (cell, "cell"), (neighbor_indices, "neighbor_indices"),
                        (neighbor_shifts, "neighbor_shifts")):
            _lib.require_device(t, name)
        self.calc = calculator
        self.weight_gradient, self.charge_gradient = bool(weight_gradient), bool(charge_gradient)
        self.full = bool(calculator.full_neighbor_list)
        if self.charge_gradient and self.full:
            raise ValueError("GraphedCombinedStep: `charge_gradient` (dE/dq = 2 V) needs a half list: a full list need not be "
                             "symmetric")
        lib = self._lib = _lib.load()
        device, dtype = positions.device, positions.dtype
        self.device, self.dtype, self._dt = device, dtype, _lib.dtype_code(dtype)
        N = self.n_atoms = positions.shape[0]
        T = self.n_terms = self._plan_c.n_terms
        geom = self._geom = analytic._geometry(calculator, cell)
        geom.plan_store = calculator._plan_store
        self._tables = analytic._combined_tables(calculator, self._plan_c, cell, geom, dtype)
        self._md = geom.desc(1)
        self._plan = _lib.get_plan(device, dtype, geom.ns, 1, geom.plan_store)
        if not self._plan.xfused:
            raise ValueError(f"GraphedCombinedStep needs a power-of-two mesh along x, the cell gives {geom.ns}")
        new = lambda *shape, dt=dtype: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
        cdtype = _lib.complex_dtype(dtype)
        self.q = charges.detach().contiguous()
        self.cell = cell.detach().to(dtype).contiguous()
        self.pos = positions.detach().clone().contiguous()
        self._w = new(T)
        self._G = new(*self._tables.shape[1:])
        self._rho, self._phi = new(*geom.ns), new(*geom.ns)
        self._hat = new(geom.n_half, dt=cdtype)
        self._rho_hat = new(geom.n_half, dt=cdtype) if self.weight_gradient else None
        self._dc = new(1)
        nbytes = int(lib.mipme_atom_bins_bytes(C.byref(self._md), N, self._dt))
        self._bins = new(nbytes, dt=torch.uint8) if nbytes > 0 else None  # (None: a mesh too small for bricks)
        self._rec = new(N, 4)
        self.potentials, self._pair_force, self._field = new(N), new(N, 3), new(N, 3)
        self.energy, self.forces = new(), new(N, 3)
        self.weight_grad = new(T) if self.weight_gradient else None
        self.charge_grad = new(N, 1) if self.charge_gradient else None
        self._minus_one = torch.tensor(-1.0, dtype=dtype, device=device)
        self._work = new(int(lib.mipme_combined_step_work(self._plan.handle, C.byref(self._md), N, T)), dt=torch.float64)
        self._nan_flag = calculator._nan_flag_ptr()
        calculator._nan_shape = [1, *geom.ns]
        self._warmup = max(1, int(warmup))
        self._pinned = (self._tables, self._plan, self._geom, getattr(self.calc, "_plan_store", None))  # members' tables, plan
        self._capture(neighbor_indices, neighbor_shifts)

    def _warm_up(self):
        self._w.copy_(self.calc.potential.weights.detach())
        super()._warm_up()

    def _launch(self):
        with _lib.on_device(self.device):
            a = _lib.CombinedStepArgs(
                plan=self._plan.handle, stream=_lib.current_stream(self.device), dtype=self._dt, full_list=int(self.full),
                mesh=C.pointer(self._md), comb=C.pointer(self._plan_c.desc), n_atoms=self.n_atoms, positions=self.pos.data_ptr(),
                charges=self.q.data_ptr(), cell=self.cell.data_ptr(), weights=self._w.data_ptr(),
                G_terms=self._tables.data_ptr(), G=self._G.data_ptr(), rho_mesh=self._rho.data_ptr(),
                hat_work=self._hat.data_ptr(), phi_mesh=self._phi.data_ptr(), dc=self._dc.data_ptr(),
                atom_bins=_lib.ptr(self._bins), records=self._rec.data_ptr(), rho_hat=_lib.ptr(self._rho_hat),
                row_ptr=self._row_ptr.data_ptr(), entries=self._ent32.data_ptr(), shift_format=2,
                potentials=self.potentials.data_ptr(), pair_force=self._pair_force.data_ptr(), field=self._field.data_ptr(),
                energy=self.energy.data_ptr(), grad_positions=self.forces.data_ptr(), grad_seed=self._minus_one.data_ptr(),
                grad_weights=_lib.ptr(self.weight_grad), grad_charges=_lib.ptr(self.charge_grad), work=self._work.data_ptr(),
                nan_flag=self._nan_flag)
            _lib.check(self._lib.mipme_combined_step(C.byref(a)))

    def recapture(self, neighbor_indices, neighbor_shifts, positions: torch.Tensor | None = None) -> None:
        """New neighbour list: rebuild the pair topology and capture the step again; every other buffer is kept."""
        self._capture(neighbor_indices, neighbor_shifts, [(self.pos, positions)])

    def __call__(self, positions: torch.Tensor | None = None):
        """``E, F`` (+ ``dE/dweights`` with ``weight_gradient``, + ``dE/dcharges`` with ``charge_gradient``, in that order) of the
        current -- or the given -- positions with the weights as they are now: one small copy and one graph replay."""
        self.calc.check()  # a NaN a previous replay met (pinned word, no synchronisation)
        with torch.no_grad():
            if positions is not None:
                self.pos.copy_(positions)
            self._w.copy_(self.calc.potential.weights.detach())
        self.graph.replay()
        out = (self.energy, self.forces)
        if self.weight_gradient:
            out += (self.weight_grad,)
        if self.charge_gradient:
            out += (self.charge_grad,)
        return out


def _compact_kvectors(freq: np.ndarray, ns):
    """Rows of the integer frequencies ``freq`` (K, 3) of a grid with ``ns`` points per axis that the dipole step sums, and their
    multiplicities: k = 0 is dropped, of every pair +-k whose two members are in the grid the one whose first non-zero component is
    positive is kept with weight 2, and a vector whose mirror is not in the grid (a component on the -n/2 plane of an even n) is
    kept with weight 1."""
    f = np.rint(np.asarray(freq, dtype=np.float64)).astype(np.int64)
    ns = np.asarray(ns, dtype=np.int64)
    unpaired = ((ns % 2 == 0)[None, :] & (f == -(ns // 2)[None, :])).any(axis=1)
    sign = np.sign(f)
    first = np.where(sign[:, 0] != 0, sign[:, 0], np.where(sign[:, 1] != 0, sign[:, 1], sign[:, 2]))
    keep = unpaired | (first > 0)
    rows = np.nonzero(keep)[0]
    return rows, np.where(unpaired[rows], 1.0, 2.0)


def _check_explicit_list(who, neighbor_indices, neighbor_shifts, frame=None):
    """The list rules of the steps that walk 4-byte pair entries.  ``frame``: the index the messages of a batch carry."""
    pre = "" if frame is None else f"{who}: frame {frame}: "
    if neighbor_indices.dim() != 2 or neighbor_indices.shape[1] != 2:
        raise ValueError(f"{pre}`neighbor_indices` must be a tensor with shape [n_pairs, 2], got tensor with shape "
                         f"{list(neighbor_indices.shape)}")
    if neighbor_shifts.dim() != 2 or tuple(neighbor_shifts.shape) != (neighbor_indices.shape[0], 3):
        raise ValueError(f"{pre}`neighbor_shifts` must be a tensor with shape [n_pairs, 3] with n_pairs = "
                         f"{neighbor_indices.shape[0]}, got tensor with shape {list(neighbor_shifts.shape)}")
    if neighbor_shifts.numel() > 0:
        s = neighbor_shifts.detach()
        if bool((s != s.round()).any()) or float(s.abs().max()) > 3:
            raise ValueError(f"{pre or who + ': '}the cell shifts must be integers in [-3, 3] (the 4-byte pair entries of the row "
                             "kernel); wrap the positions into the cell or use a shorter cutoff")


def _check_ewald_calculator(who, calculator, instead):
    """The calculator and potential the Ewald step kernels serve; ``instead``: the class for the mesh calculators."""
    from .calculators import EwaldCalculator
    from .potentials import CoulombPotential, InversePowerLawPotential

    if not isinstance(calculator, EwaldCalculator):
        raise TypeError(f"{who} serves an EwaldCalculator, got a {type(calculator).__name__}: use {instead} for the mesh "
                        "calculators")
    pot = calculator.potential
    if type(pot) not in (CoulombPotential, InversePowerLawPotential):
        raise TypeError(f"{who}: the kernels know exactly CoulombPotential and InversePowerLawPotential, got a "
                        f"{type(pot).__name__}; call the calculator eagerly")


MAX_EWALD_CHANNELS = _lib.EWALD_MAX_CHANNELS


def _check_n_channels(who, n_channels):
    """``n_channels`` of an Ewald step: an ``int`` in 1..8."""
    if isinstance(n_channels, bool) or not isinstance(n_channels, int) or not 1 <= n_channels <= MAX_EWALD_CHANNELS:
        raise ValueError(f"{who}: `n_channels` must be an int in 1..{MAX_EWALD_CHANNELS} (the charge channels the step kernels keep "
                         f"in registers), got {n_channels!r}")


def _check_channel_charges(who, charges, n_atoms, n_channels, frame=None):
    """``charges`` handed to a multi-channel object after construction: exactly ``(n_atoms, n_channels)`` -- ``copy_`` would
    broadcast an (N, 1) tensor into every channel without a word."""
    if tuple(charges.shape) != (n_atoms, n_channels):
        pre = f"{who}: " if frame is None else f"{who}: frame {frame}: "
        raise ValueError(f"{pre}`charges` must be a tensor with shape [n_atoms, n_channels] = [{n_atoms}, {n_channels}] "
                         f"(n_channels = {n_channels}), got tensor with shape {list(charges.shape)}")


def _check_ewald_system(who, charges, cell, positions, frame=None, first=None, n_channels=1):
    """Shapes, dtype and atom count of one system of an Ewald step.  In a batch, ``frame`` is its index and ``first`` the tensor
    whose dtype all frames share.  ``n_channels``: the charge channels of the object (1: the single-channel rules, word for
    word)."""
    batch = frame is not None
    pre = f"{who}: frame {frame}: " if batch else ""
    if n_channels == 1:
        if charges.dim() != 2 or charges.shape[1] != 1:
            raise ValueError(f"{pre or who + ' handles '}a single charge channel, `charges` of shape [n_atoms, 1], got tensor with "
                             f"shape {list(charges.shape)}")
    elif charges.dim() != 2 or charges.shape[1] != n_channels:
        raise ValueError(f"{pre or who + ': '}`charges` must be a tensor with shape [n_atoms, n_channels] = [n_atoms, {n_channels}] "
                         f"(n_channels = {n_channels}), got tensor with shape {list(charges.shape)}")
    if positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] != charges.shape[0]:
        raise ValueError(f"{pre}`positions` must be a tensor with shape [n_atoms, 3] with n_atoms = {charges.shape[0]} (the "
                         f"charges), got tensor with shape {list(positions.shape)}")
    if tuple(cell.shape) != (3, 3):
        raise ValueError(f"{pre}`cell` must be a tensor with shape [3, 3], got tensor with shape {list(cell.shape)}")
    shared = positions.dtype == charges.dtype == cell.dtype and (not batch or cell.dtype == first.dtype)
    if not shared or positions.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{pre}`positions`, `charges` and `cell`{' of all frames' if batch else ''} must share one dtype, float32 "
                         f"or float64, got {positions.dtype}, {charges.dtype} and {cell.dtype}"
                         + (f" (frame 0: {first.dtype})" if batch else ""))
    if positions.shape[0] < 1 or positions.shape[0] > (1 << 22):
        raise ValueError(f"{pre + 'a frame holds ' if batch else who + ' handles '}1 to 2^22 atoms (the 4-byte pair entries of the "
                         f"row kernel), got {positions.shape[0]}")


def _ewald_kgrid(cell, lr_wavelength):
    """``(ns, frequencies (K, 3) int32, multiplicities (K,) int32)`` of the k grid an Ewald step freezes for ``cell``: the integer
    frequencies as the eager call forms them (ValueError for a singular cell), one of every pair +-k."""
    from .calculators import _integer_frequencies

    freq, _ = _integer_frequencies(cell.detach(), lr_wavelength, None)
    ns = GraphedEwaldStep._ns_of(cell, lr_wavelength)
    f = freq.cpu().numpy()
    rows, weight = _compact_kvectors(f, ns)
    return ns, np.rint(f[rows]).astype(np.int32).reshape(-1, 3), weight.astype(np.int32)


class GraphedDipoleStep(_ExplicitListStep):
    """``E, F, dE_dmu = step(positions, dipoles)`` for a :class:`~torchpme_amd.CalculatorDipole`, replayed from one HIP graph: the
    MD form of the eager call for a fixed neighbour list and a cell that is fixed or, with ``follow_cell=True``, an input of
    every call (dipolar fluids, polarisable models).

    With ``V`` what the eager calculator returns for the same arguments and ``neighbor_vectors = r_j - r_i + S cell`` -- the step
    forms the pair vectors itself from the list and its cell shifts -- ``E = sum_i mu_i . V_i`` (0-dim), ``F = -dE/dpositions``
    (N, 3; the total derivative, through the pair vectors and the reciprocal part), ``dE_dmu = dE/ddipoles`` (N, 3; the total
    derivative: ``2 V`` for a half list, ``V`` plus the transposed half for a full one) and, with ``cell_gradient``, ``dE_dcell``
    (3, 3) at fixed Cartesian positions (the convention of ``GraphedEnergyForces(cell_gradient=True)``).  The field at dipole i is
    ``-dE_dmu[i]``, so the torque on it is ``mu_i x (-dE_dmu_i)``: ``torch.linalg.cross(dipoles, -dE_dmu)``.

    All outputs are buffers of the object, overwritten by every call.  A call copies the given positions and dipoles into the
    object's buffers and replays the graph: no host reads, and -- as on the eager dipole path -- no check for non-finite input.
    Every sum of the step has a fixed order (no floating-point atomics), so equal inputs give equal bits.  A new list needs
    :meth:`recapture`.

    Without ``follow_cell`` the cell is fixed for the life of the object: everything that depends on it is built once on the host.
    With ``follow_cell=True`` the cell is an input of the replay like the positions (NPT runs, cell relaxations, strain scans):
    ``step(positions, dipoles, cell)`` copies whichever of the three are given into the object's buffers (:attr:`cell` is the
    (3, 3) input buffer) and replays the one graph -- no host reads, nothing re-captured.  The k-vectors, G(k), dG/dk^2, the
    inverse cell, 1/V and the Cartesian shift vectors of the pair rows are rebuilt on the device inside the replay from the nine
    values of the cell buffer (``mipme_dipole_cell_step``; as many launches as the fixed-cell step).  The outputs mean what they
    mean above, at the current cell.  The SET of k-vectors is frozen at construction, as in :class:`GraphedEwaldStep`: the
    integer frequencies the eager call chooses for the construction cell, ``ns_d = ceil(|a_d| / lr_wavelength)`` (:attr:`ns`),
    one of every pair +-k (:attr:`n_k`).  :attr:`status` is a device ``int32`` (1,) tensor every replay writes -- bit 0: the
    eager call would sum another grid for this cell (never set for a direct potential); bit 1: ``det(cell)`` is zero or not
    finite (then E is NaN and the k table zeros) -- and :meth:`kgrid_matches` decides bit 0 on the host.  The skin of the list
    under a changing cell is the caller's business.

    E is quadratic in the dipoles, so the structure factors are formed once, one kernel evaluates the field and the position
    gradient from one phase per (atom, k), and only one of every pair +-k of the reciprocal grid is summed (:attr:`n_k` vectors);
    the pair part is one walk over the transposed list without atomics (``mipme_dipole_step``, csrc/dipole_step.hip).

    :param calculator: a :class:`CalculatorDipole` with any :class:`PotentialDipole` the eager call accepts (direct or range
        separated, with or without exclusion radius, ``epsilon``, ``prefactor``; half or full list from
        ``calculator.full_neighbor_list``)
    :param dipoles: (N, 3)
    :param cell: (3, 3), rows are the lattice vectors
    :param positions: (N, 3)
    :param neighbor_indices, neighbor_shifts: an explicit list (P, 2) with integer cell shifts (P, 3) in [-3, 3]; at most 2^22 atoms
    :param cell_gradient: also return ``dE/dcell``
    :param warmup: eager runs before the capture
    :param follow_cell: the cell is an input of every replay (``cell=`` of a call and of :meth:`recapture`)
    """

    def __init__(self, calculator, dipoles, cell, positions, neighbor_indices, neighbor_shifts, cell_gradient: bool = False,
                 warmup: int = 3, follow_cell: bool = False):
        from .calculators import _integer_frequencies, _reciprocal_and_det
        from .dipoles import CalculatorDipole

        if not isinstance(calculator, CalculatorDipole):
            raise TypeError(f"GraphedDipoleStep serves a CalculatorDipole, got a {type(calculator).__name__}: use GraphedEnergyForces "
                            "or GraphedCombinedStep for charges")
        if dipoles.dim() != 2 or dipoles.shape[1] != 3:
            raise ValueError(f"`dipoles` must be a tensor with shape [n_atoms, 3], got tensor with shape {list(dipoles.shape)}")
        if positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] != dipoles.shape[0]:
            raise ValueError(f"`positions` must be a tensor with shape [n_atoms, 3] with n_atoms = {dipoles.shape[0]} (the dipoles), "
                             f"got tensor with shape {list(positions.shape)}")
        if tuple(cell.shape) != (3, 3):
            raise ValueError(f"`cell` must be a tensor with shape [3, 3], got tensor with shape {list(cell.shape)}")
        if not (positions.dtype == dipoles.dtype == cell.dtype) or positions.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"`positions`, `dipoles` and `cell` must share one dtype, float32 or float64, got {positions.dtype}, "
                             f"{dipoles.dtype} and {cell.dtype}")
        if positions.shape[0] < 1 or positions.shape[0] > (1 << 22):
            raise ValueError(f"GraphedDipoleStep handles 1 to 2^22 atoms (the 4-byte pair entries of the row kernel), got "
                             f"{positions.shape[0]}")
        _check_explicit_list("GraphedDipoleStep", neighbor_indices, neighbor_shifts)
        for t, name in ((positions, "positions"), (dipoles, "dipoles"), (cell, "cell"), (neighbor_indices, "neighbor_indices"),
                        (neighbor_shifts, "neighbor_shifts")):
            _lib.require_device(t, name)
        self.calc = calculator
        self.cell_gradient = bool(cell_gradient)
        self.follow_cell = bool(follow_cell)
        self.full = bool(calculator.full_neighbor_list)
        lib = self._lib = _lib.load()
        device, dtype = positions.device, positions.dtype
        self.device, self.dtype, self._dt = device, dtype, _lib.dtype_code(dtype)
        N = self.n_atoms = positions.shape[0]
        pot = calculator.potential
        sm, _, eps, pref = pot._host_params()
        self._desc = pot._descriptor()
        new = lambda *shape, dt=dtype: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
        self.cell = cell.detach().clone().contiguous()
        cell_host = self.cell.to("cpu", torch.float64).numpy()
        det = float(np.linalg.det(cell_host))
        if det == 0.0 or not np.isfinite(det):
            raise ValueError(f"provided `cell` has a determinant of {det}, i.e. it is not a valid unit cell")
        if self.follow_cell:
            self._init_follow_cell(sm, eps, pref, new)
            self._finish_init(positions, dipoles, neighbor_indices, neighbor_shifts, warmup, new,
                              lib.mipme_dipole_cell_step_work)
            return
        self._inv_volume = 1.0 / abs(det)
        self._inv_cell = torch.tensor(np.linalg.inv(cell_host), dtype=dtype, device=device).contiguous()
        self._self_term, self._background = 0.0, 0.0
        self._kvec = self._G = self._dG = self._Sc = self._Ss = None
        self.n_k = 0
        if sm is not None:
            # the k-vectors exactly as CalculatorDipole._compute_kspace forms them, then one of every +-k pair
            recip, _ = _reciprocal_and_det(self.cell)
            freq, _ = _integer_frequencies(self.cell, calculator.lr_wavelength, None)
            ns = np.ceil(np.linalg.norm(cell_host, axis=1) / calculator.lr_wavelength).astype(np.int64)
            rows, weight = _compact_kvectors(freq.cpu().numpy(), ns)
            kvec = ((2 * math.pi) * freq @ recip)[torch.as_tensor(rows, device=device)].contiguous()
            K = self.n_k = int(kvec.shape[0])
            alpha = 0.5 / sm**2
            self._self_term = pref * 4 * math.pi / 3 * (alpha / math.pi) ** 1.5
            self._background = pref * 4 * math.pi / (2 * eps + 1) if eps != 0.0 else 0.0
            if K > 0:
                G, dG = new(K), new(K)
                with _lib.on_device(device):
                    _lib.check(lib.mipme_ewald_filter(_lib.current_stream(device), self._dt, C.byref(pot._coulomb_descriptor()), K,
                                                      kvec.data_ptr(), G.data_ptr(), dG.data_ptr()))
                w = torch.as_tensor(weight, dtype=dtype, device=device)
                self._kvec, self._G = kvec, G * w  # the multiplicity folded into the filter
                self._dG = dG * w if self.cell_gradient else None
                self._Sc, self._Ss = new(K), new(K)
        self._finish_init(positions, dipoles, neighbor_indices, neighbor_shifts, warmup, new, lib.mipme_dipole_step_work)

    def _init_follow_cell(self, sm, eps, pref, new):
        """What ``follow_cell=True`` freezes: the integer k grid of the construction cell (the rule and the helper of
        :class:`GraphedEwaldStep`) and the constants of the potential that do not depend on the cell.  The k-vectors, G, dG, 1/V
        and the inverse cell are buffers every replay writes."""
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._self_term, self._background = 0.0, 0.0
        self._freq = self._mult = self._kvec = self._G = self._dG = self._Sc = self._Ss = None
        self.n_k, self.ns, self.lr_wavelength = 0, (1, 1, 1), 0.0  # (a direct potential: no grid to compare with)
        if sm is None:
            return
        self.lr_wavelength = float(self.calc.lr_wavelength)
        self.ns, freq, mult = _ewald_kgrid(self.cell, self.lr_wavelength)
        K = self.n_k = int(len(mult))
        alpha = 0.5 / sm**2
        self._self_term = pref * 4 * math.pi / 3 * (alpha / math.pi) ** 1.5
        self._background = pref * 4 * math.pi / (2 * eps + 1) if eps != 0.0 else 0.0
        if K > 0:
            self._freq, self._mult = torch.tensor(freq, device=self.device), torch.tensor(mult, device=self.device)
            self._kvec, self._G, self._Sc, self._Ss = new(K, 3), new(K), new(K), new(K)
            self._dG = new(K) if self.cell_gradient else None

    def _finish_init(self, positions, dipoles, neighbor_indices, neighbor_shifts, warmup, new, work_size):
        N = self.n_atoms
        self.pos = positions.detach().clone().contiguous()
        self.mu = dipoles.detach().clone().contiguous()
        self._rec = new(2 * N, 4)
        self.energy, self.forces, self.dipole_grad = new(), new(N, 3), new(N, 3)
        self.cell_grad = new(3, 3) if self.cell_gradient else None
        self._work = new(max(1, int(work_size(N, self.n_k, int(self.cell_gradient)))), dt=torch.float64)
        self._warmup = max(1, int(warmup))
        self._capture(neighbor_indices, neighbor_shifts)

    def kgrid_matches(self, cell) -> bool:
        """Whether the eager calculator would sum the step's k grid for ``cell``: every ``ceil(|a_d| / lr_wavelength)`` equals
        the one of the construction cell (bit 0 of :attr:`status` clear), decided on the host with the rule of
        :meth:`GraphedEwaldStep.kgrid_matches`.  A direct potential sums no grid: always ``True``."""
        self._need_follow_cell("kgrid_matches")
        if self.lr_wavelength <= 0.0:
            return True
        return GraphedEwaldStep._ns_of(cell, self.lr_wavelength) == self.ns

    def _need_follow_cell(self, what):
        if not self.follow_cell:
            raise ValueError(f"GraphedDipoleStep: {what} needs an object built with follow_cell=True: the cell of this one is "
                             "fixed for the life of the object")

    def _checked_cell(self, cell):
        """The ``cell=`` argument of a call or of :meth:`recapture`, refused before anything of the object changes."""
        if cell is None:
            return None
        self._need_follow_cell("`cell=`")
        if not isinstance(cell, torch.Tensor) or tuple(cell.shape) != (3, 3) or cell.dtype != self.dtype or cell.device != self.device:
            got = (f"a {type(cell).__name__}" if not isinstance(cell, torch.Tensor) else
                   f"shape {list(cell.shape)}, {cell.dtype} on {cell.device}")
            raise ValueError(f"GraphedDipoleStep: `cell` must be a tensor with shape [3, 3], {self.dtype} on {self.device}, got {got}")
        return cell

    def _launch_follow_cell(self):
        with _lib.on_device(self.device):
            a = _lib.DipoleCellStepArgs(
                stream=_lib.current_stream(self.device), dtype=self._dt, full_list=int(self.full), pot=C.pointer(self._desc),
                self_term=self._self_term, background=self._background, n_atoms=self.n_atoms, n_k=self.n_k,
                lr_wavelength=self.lr_wavelength, ns=(C.c_int32 * 3)(*self.ns), cell_gradient=int(self.cell_gradient),
                positions=self.pos.data_ptr(), dipoles=self.mu.data_ptr(), cell=self.cell.data_ptr(),
                frequencies=_lib.ptr(self._freq), multiplicities=_lib.ptr(self._mult), row_ptr=self._row_ptr.data_ptr(),
                entries=self._ent32.data_ptr(), shift_format=2, records=self._rec.data_ptr(), kvectors=_lib.ptr(self._kvec),
                G=_lib.ptr(self._G), dG=_lib.ptr(self._dG), s_cos=_lib.ptr(self._Sc), s_sin=_lib.ptr(self._Ss),
                energy=self.energy.data_ptr(), forces=self.forces.data_ptr(), grad_dipoles=self.dipole_grad.data_ptr(),
                grad_cell=_lib.ptr(self.cell_grad), status=self.status.data_ptr(), work=self._work.data_ptr())
            _lib.check(self._lib.mipme_dipole_cell_step(C.byref(a)))

    def _launch(self):
        if self.follow_cell:
            return self._launch_follow_cell()
        with _lib.on_device(self.device):
            a = _lib.DipoleStepArgs(
                stream=_lib.current_stream(self.device), dtype=self._dt, full_list=int(self.full), pot=C.pointer(self._desc),
                n_atoms=self.n_atoms, n_k=self.n_k, inv_volume=self._inv_volume, self_term=self._self_term,
                background=self._background, positions=self.pos.data_ptr(), dipoles=self.mu.data_ptr(), cell=self.cell.data_ptr(),
                inv_cell=self._inv_cell.data_ptr(), kvectors=_lib.ptr(self._kvec), G=_lib.ptr(self._G), dG=_lib.ptr(self._dG),
                row_ptr=self._row_ptr.data_ptr(), entries=self._ent32.data_ptr(), shift_format=2,
                cell_gradient=int(self.cell_gradient), records=self._rec.data_ptr(), s_cos=_lib.ptr(self._Sc), s_sin=_lib.ptr(self._Ss),
                energy=self.energy.data_ptr(), forces=self.forces.data_ptr(), grad_dipoles=self.dipole_grad.data_ptr(),
                grad_cell=_lib.ptr(self.cell_grad), work=self._work.data_ptr())
            _lib.check(self._lib.mipme_dipole_step(C.byref(a)))

    def recapture(self, neighbor_indices, neighbor_shifts, positions: torch.Tensor | None = None,
                  dipoles: torch.Tensor | None = None, cell: torch.Tensor | None = None) -> None:
        """New neighbour list: rebuild the pair topology and capture the step again; every other buffer (and, with
        ``follow_cell``, the k grid) is kept.  ``cell`` needs ``follow_cell=True``.  The list and the cell are validated before
        anything of the object changes."""
        cell = self._checked_cell(cell)
        _check_explicit_list("GraphedDipoleStep", neighbor_indices, neighbor_shifts)
        self._capture(neighbor_indices, neighbor_shifts, [(self.pos, positions), (self.mu, dipoles), (self.cell, cell)])

    def __call__(self, positions: torch.Tensor | None = None, dipoles: torch.Tensor | None = None,
                 cell: torch.Tensor | None = None):
        """``E, F, dE_dmu`` (+ ``dE_dcell`` with ``cell_gradient``) of the current -- or the given -- positions, dipoles and, with
        ``follow_cell=True``, cell: up to three small copies and one graph replay."""
        cell = self._checked_cell(cell)
        with torch.no_grad():
            if positions is not None:
                self.pos.copy_(positions)
            if dipoles is not None:
                self.mu.copy_(dipoles)
            if cell is not None:
                self.cell.copy_(cell)
        self.graph.replay()
        out = (self.energy, self.forces, self.dipole_grad)
        if self.cell_gradient:
            out += (self.cell_grad,)
        return out


class GraphedEwaldStep(_ExplicitListStep):
    """``E, F, dE_dq = step(positions, charges, cell)`` for an :class:`~torchpme_amd.EwaldCalculator`, replayed from one HIP
    graph: the MD form of the eager call for a fixed neighbour list -- and a cell that may change from call to call (NPT runs,
    cell relaxations, strain scans).

    With ``V`` what the eager calculator returns for ``pair_distances(positions, pairs, cell, shifts)`` and the current cell,
    ``E = sum_a q_a V_a`` (0-dim), ``F = -dE/dpositions`` (N, 3), ``dE_dq = dE/dcharges`` (N, 1; the total derivative: ``2 V`` for
    a half list, ``V`` plus the transposed pair half for a full one) and, with ``cell_gradient``, ``dE_dcell`` (3, 3) at fixed
    Cartesian positions (the convention of the other steps).  All outputs are buffers of the object, overwritten by every call.

    A call copies whichever of ``positions``, ``charges`` and ``cell`` are given into the object's buffers and replays one graph:
    no host reads, nothing re-captured.  Everything that depends on the cell's values -- k-vectors, G(k), dG/dk^2, the inverse
    cell, 1/V, the Cartesian shift vectors of the pair rows -- is rebuilt on the device inside the replay from the nine values of
    the cell buffer (``mipme_ewald_step``, csrc/ewald_step.hip).  Every sum has a fixed order (no floating-point atomics), so
    equal inputs give equal bits.

    The SET of k-vectors is fixed when the object is built: the integer frequencies the eager call chooses for the construction
    cell, ``ns_d = ceil(|a_d| / lr_wavelength)`` per axis (:attr:`ns`), one of every pair +-k (:attr:`n_k` vectors).  The eager
    call would choose another grid as soon as some ``ns_d`` changes; the step keeps its grid, so the energy stays a smooth
    function of the cell, and says so: :attr:`status` is a device ``int32`` tensor every replay writes -- bit 0: the eager call
    would use another k grid for this cell; bit 1: ``det(cell)`` is zero or not finite (the energy is NaN then) -- and
    :meth:`kgrid_matches` is the same comparison on the host.  The skin of the list under a changing cell is the caller's
    business; a new list needs :meth:`recapture`.

    :param calculator: an :class:`EwaldCalculator` whose potential is exactly a :class:`CoulombPotential` or an
        :class:`InversePowerLawPotential` (exponent 1..6), with or without exclusion radius, any ``prefactor``; half or full list
        from ``calculator.full_neighbor_list``
    :param charges: (N, 1)
    :param cell: (3, 3), rows are the lattice vectors
    :param positions: (N, 3)
    :param neighbor_indices, neighbor_shifts: an explicit list (P, 2) with integer cell shifts (P, 3) in [-3, 3]; at most 2^22 atoms
    :param cell_gradient: also return ``dE/dcell``
    :param warmup: eager runs before the capture
    :param n_channels: the charge channels C, an ``int`` in 1..8 (:attr:`n_channels`).  With ``C >= 2`` ``charges`` is (N, C) --
        latent or learned charges, several per atom, each channel an independent system of charges on the same atoms -- and the
        object runs ``mipme_ewald_channels_step`` (csrc/ewald_channels_step.hip): with ``V`` the (N, C) potential of the eager
        call, ``E = sum_a sum_c q_ac V_ac``, ``F`` and ``dE_dcell`` are those of this energy and ``dE_dq`` is (N, C), the total
        derivative per channel.  The phase of every (atom, k) and the pair function of every list entry are computed once for
        all channels, so one replay costs far less than C single-channel replays.  A ``charges=`` of a later call must be
        exactly (N, C).  With the default 1 the object is the single-channel step, entry point and bits.
    """

    def __init__(self, calculator, charges, cell, positions, neighbor_indices, neighbor_shifts, cell_gradient: bool = False,
                 warmup: int = 3, n_channels: int = 1):
        who = "GraphedEwaldStep"
        _check_ewald_calculator(who, calculator, "GraphedEnergyForces")
        _check_n_channels(who, n_channels)
        _check_ewald_system(who, charges, cell, positions, n_channels=n_channels)
        _check_explicit_list(who, neighbor_indices, neighbor_shifts)
        self.lr_wavelength = float(calculator.lr_wavelength)
        self.ns, freq, mult = _ewald_kgrid(cell, self.lr_wavelength)
        for t, name in ((positions, "positions"), (charges, "charges"), (cell, "cell"), (neighbor_indices, "neighbor_indices"),
                        (neighbor_shifts, "neighbor_shifts")):
            _lib.require_device(t, name)
        self.calc = calculator
        self.cell_gradient = bool(cell_gradient)
        self.full = bool(calculator.full_neighbor_list)
        lib = self._lib = _lib.load()
        device, dtype = positions.device, positions.dtype
        self.device, self.dtype, self._dt = device, dtype, _lib.dtype_code(dtype)
        N = self.n_atoms = positions.shape[0]
        nc = self.n_channels = n_channels
        self._desc = calculator.potential._descriptor()
        new = lambda *shape, dt=dtype: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
        self.cell = cell.detach().clone().contiguous()
        K = self.n_k = int(len(mult))
        self._freq, self._mult = torch.tensor(freq, device=device), torch.tensor(mult, device=device)
        self._kvec, self._G, self._Sc, self._Ss = new(max(K, 1), 3), new(max(K, 1)), new(nc * max(K, 1)), new(nc * max(K, 1))
        self._dG = new(max(K, 1)) if self.cell_gradient else None
        self.pos = positions.detach().clone().contiguous()
        self.q = charges.detach().clone().contiguous()
        self._rec = new(N, 4)
        self.energy, self.forces, self.charge_grad = new(), new(N, 3), new(N, nc)
        self.cell_grad = new(3, 3) if self.cell_gradient else None
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        n_work = (lib.mipme_ewald_step_work(N, K, int(self.cell_gradient)) if nc == 1 else
                  lib.mipme_ewald_channels_step_work(N, K, nc, int(self.cell_gradient)))
        self._work = new(max(1, int(n_work)), dt=torch.float64)
        self._warmup = max(1, int(warmup))
        self._capture(neighbor_indices, neighbor_shifts)

    @staticmethod
    def _ns_of(cell, lr_wavelength):
        cell_host = cell.detach().to("cpu", torch.float64).numpy()
        return tuple(int(n) for n in np.ceil(np.linalg.norm(cell_host, axis=1) / lr_wavelength))

    def kgrid_matches(self, cell) -> bool:
        """Whether the eager calculator would sum the step's k grid for ``cell``: every ``ceil(|a_d| / lr_wavelength)`` equals
        the one of the construction cell (bit 0 of :attr:`status` clear), decided on the host."""
        return self._ns_of(cell, self.lr_wavelength) == self.ns

    def _launch(self):
        with _lib.on_device(self.device):
            fields = dict(
                stream=_lib.current_stream(self.device), dtype=self._dt, full_list=int(self.full), pot=C.pointer(self._desc),
                n_atoms=self.n_atoms, n_k=self.n_k, lr_wavelength=self.lr_wavelength, ns=(C.c_int32 * 3)(*self.ns),
                cell_gradient=int(self.cell_gradient), positions=self.pos.data_ptr(), charges=self.q.data_ptr(),
                cell=self.cell.data_ptr(), frequencies=self._freq.data_ptr(), multiplicities=self._mult.data_ptr(),
                row_ptr=self._row_ptr.data_ptr(), entries=self._ent32.data_ptr(), shift_format=2, records=self._rec.data_ptr(),
                kvectors=self._kvec.data_ptr(), G=self._G.data_ptr(), dG=_lib.ptr(self._dG), s_cos=self._Sc.data_ptr(),
                s_sin=self._Ss.data_ptr(), energy=self.energy.data_ptr(), forces=self.forces.data_ptr(),
                grad_charges=self.charge_grad.data_ptr(), grad_cell=_lib.ptr(self.cell_grad), status=self.status.data_ptr(),
                work=self._work.data_ptr())
            if self.n_channels == 1:
                a = _lib.EwaldStepArgs(**fields)
                _lib.check(self._lib.mipme_ewald_step(C.byref(a)))
            else:
                a = _lib.EwaldChannelsStepArgs(n_channels=self.n_channels, **fields)
                _lib.check(self._lib.mipme_ewald_channels_step(C.byref(a)))

    def recapture(self, neighbor_indices, neighbor_shifts, positions: torch.Tensor | None = None,
                  charges: torch.Tensor | None = None, cell: torch.Tensor | None = None) -> None:
        """New neighbour list: rebuild the pair topology and capture the step again; the k grid and every buffer are kept.  The
        list is validated before anything of the object changes."""
        _check_explicit_list("GraphedEwaldStep", neighbor_indices, neighbor_shifts)
        if charges is not None and self.n_channels > 1:
            _check_channel_charges("GraphedEwaldStep", charges, self.n_atoms, self.n_channels)
        self._capture(neighbor_indices, neighbor_shifts, [(self.pos, positions), (self.q, charges), (self.cell, cell)])

    def __call__(self, positions: torch.Tensor | None = None, charges: torch.Tensor | None = None,
                 cell: torch.Tensor | None = None):
        """``E, F, dE_dq`` (+ ``dE_dcell`` with ``cell_gradient``) of the current -- or the given -- positions, charges and cell:
        up to three small copies and one graph replay."""
        if charges is not None and self.n_channels > 1:  # (before anything of the object changes)
            _check_channel_charges("GraphedEwaldStep", charges, self.n_atoms, self.n_channels)
        with torch.no_grad():
            if positions is not None:
                self.pos.copy_(positions)
            if charges is not None:
                self.q.copy_(charges)
            if cell is not None:
                self.cell.copy_(cell)
        self.graph.replay()
        out = (self.energy, self.forces, self.charge_grad)
        if self.cell_gradient:
            out += (self.cell_grad,)
        return out


class _FrameTableBatch:
    """What the batches of explicit-list steps share (:class:`GraphedEwaldBatch`, :class:`GraphedDipoleBatch`): packing F lists
    into concatenated row pointers and 4-byte entries, the frame table, the capture, and the copies of a call.  A subclass names
    itself (``_who``) and the two table functions of its entry point, keeps the per-atom values beside the positions (charges or
    dipoles) in ``self._values`` and supplies ``_launch``."""

    MAX_FRAMES = 1 << 20
    _who = _table_bytes = _table_build = None
    _table_args = ()  # what the two table functions take between the host arrays and `cell_gradient`

    def _pack(self, lists):
        """Validate and pack F ``(neighbor_indices, neighbor_shifts)`` into the concatenated row pointers and 4-byte entries and
        build the frame table for them.  Nothing of the object changes: what is returned goes to :meth:`_install`."""
        who = self._who
        lists = [tuple(ls) for ls in lists]
        if len(lists) != self.n_frames:
            raise ValueError(f"{who}: {self.n_frames} lists wanted, one (neighbor_indices, neighbor_shifts) per frame, got {len(lists)}")
        for f, ls in enumerate(lists):
            if len(ls) != 2:
                raise ValueError(f"{who}: frame {f}: a list is (neighbor_indices, neighbor_shifts), got {len(ls)} items")
            _check_explicit_list(who, *ls, frame=f)
            for t, name in zip(ls, ("neighbor_indices", "neighbor_shifts")):
                _lib.require_device(t, f"{name} of frame {f}")
        rows, ents, keep = [], [], []
        for f, (idx, shifts) in enumerate(lists):
            sh = shifts.to(self.dtype).contiguous()
            topo = ops.get_topology(idx, self.atom_ptr[f + 1] - self.atom_ptr[f])
            ent32 = topo.compact_entries(sh, shifts)
            if ent32 is None:
                raise ValueError(f"{who}: frame {f}: the cell shifts must be integers in [-3, 3] (the 4-byte pair entries of the row "
                                 "kernel) and the frame at most 2^22 atoms")
            rows.append(topo.row_ptr)
            ents.append(ent32)
            keep.append(topo)
        entry_ptr = np.concatenate([[0], np.cumsum([e.shape[0] for e in ents])]).astype(np.int64)
        if int(entry_ptr[-1]) >= (1 << 31):
            raise ValueError(f"{who}: the lists hold {int(entry_ptr[-1])} entry words, the frame table 2^31 - 1 at most")
        lib, F, cg = self._lib, self.n_frames, int(self.cell_gradient)
        n_bytes = int(getattr(lib, self._table_bytes)(F, self._atom_ptr.ctypes.data, self._k_ptr.ctypes.data, *self._table_args, cg))
        host = np.zeros(n_bytes, dtype=np.uint8)
        _lib.check(getattr(lib, self._table_build)(F, self._atom_ptr.ctypes.data, self._k_ptr.ctypes.data, entry_ptr.ctypes.data,
                                                   self._ns.ctypes.data, *self._table_args, cg, host.ctypes.data, n_bytes))
        with torch.no_grad():
            row_ptr = torch.cat(rows).to(torch.int32).contiguous()
            ent32 = torch.cat(ents).contiguous()
        table = torch.from_numpy(host).to(self.device)  # one upload per capture
        return [ls[0] for ls in lists], row_ptr, ent32, entry_ptr, table

    def _install(self, packed):
        self.pairs, self._row_ptr, self._ent32, self._entry_ptr, self._table = packed
        self.graph = _capture_graph(self.device, self._warm_up, self._launch)

    def _warm_up(self):
        for _ in range(self._warmup):
            self._launch()

    def _load(self, positions=None, values=None, cells=None):
        """Each input given, a flat tensor or a list of F per-frame tensors, into the object's buffer: one copy each."""
        with torch.no_grad():
            for buf, new in ((self.pos, positions), (self._values, values), (self.cells.view(-1, 3), cells)):
                if new is None:
                    continue
                if isinstance(new, (list, tuple)):
                    if len(new) != self.n_frames:
                        raise ValueError(f"{self._who}: a list of {self.n_frames} per-frame tensors wanted, got {len(new)}")
                    if sum(int(t.shape[0]) for t in new) != buf.shape[0]:
                        raise ValueError(f"{self._who}: the per-frame tensors hold {sum(int(t.shape[0]) for t in new)} rows, the "
                                         f"buffer {buf.shape[0]}")
                    torch.cat([t.detach() for t in new], out=buf)
                else:
                    buf.copy_(new.detach().reshape(buf.shape))

    def _recapture(self, lists, positions, values, cells):
        packed = self._pack(lists)
        self._load(positions, values, cells)
        self._install(packed)


class GraphedEwaldBatch(_FrameTableBatch):
    """``energies, forces, dE_dq = batch(positions, charges, cells)`` for MANY small systems and one
    :class:`~torchpme_amd.EwaldCalculator`, replayed from one HIP graph: the data-set form of :class:`GraphedEwaldStep` --
    hundreds to thousands of structures of 10 to 500 atoms, each with its own cell, its own atom count and its own k grid, whose
    energies, forces, charge gradients and stress labels are wanted together.  A :class:`GraphedEwaldStep` replay at these sizes
    is seven launches of a few dozen workgroups: latency, not work.  The batch runs the same seven launches ONCE for all frames
    (``mipme_ewald_batch``, csrc/ewald_batch.hip; a table maps every workgroup to its frame, no workgroup straddles two).

    For frame f, ``energies[f]``, ``forces[f]``, ``dE_dq[f]`` and -- with ``cell_gradient`` -- ``dE_dcell[f]`` mean word for word
    what ``E``, ``F``, ``dE_dq`` and ``dE_dcell`` of a :class:`GraphedEwaldStep` of that frame mean: total derivatives, the cell
    gradient at fixed Cartesian positions.  ``energies`` is (F,); ``forces`` and ``dE_dq`` are lists of per-frame views into one
    flat buffer each, (sum N, 3) and (sum N, 1), also exposed as :attr:`forces_flat` and :attr:`charge_grads_flat`; ``dE_dcell``
    is one (F, 3, 3) tensor.  All outputs are buffers of the object, overwritten by every call.

    A call copies whichever of ``positions``, ``charges`` and ``cells`` are given into the object's buffers -- each either one
    flat tensor in frame order or a list of F per-frame tensors, which goes in through ONE ``torch.cat(..., out=buffer)`` -- and
    replays one graph: no host reads, nothing re-captured, and nothing launched depends on any cell having the values it had at
    construction.  Every sum has a fixed order, and a frame is computed from its own inputs alone: the bits it gets do not depend
    on its index, on F or on the other frames of the batch.

    The k grid of every frame is frozen at construction, as in the single step: :attr:`ns` ``[f]``, :attr:`n_k` ``[f]`` (one of
    every pair +-k).  :attr:`status` is a device ``int32`` (F,) tensor every replay writes, with the single step's two bits per
    frame -- bit 0: the eager call would use another k grid for this cell; bit 1: ``det(cell)`` is zero or not finite (that
    frame's energy is NaN, no other frame is touched) -- and :meth:`kgrid_matches` is the comparison of bit 0 on the host.
    :attr:`atom_ptr` holds the F + 1 host offsets of the frames in the flat buffers.  Frames whose cell is shorter than
    ``lr_wavelength`` along every axis have the grid (1, 1, 1) and ``n_k == 0``; they are served, as are frames with an empty list
    or a single atom.

    Several charge channels: with ``n_channels=C``, 2 <= C <= 8, every frame's ``charges`` is (N_f, C) -- the training set of a
    model with latent charges -- and the batch runs ``mipme_ewald_channels_batch`` (csrc/ewald_channels_batch.hip): per frame
    what a :class:`GraphedEwaldStep` with ``n_channels=C`` computes, ``dE_dq`` (N_f, C) per frame, :attr:`charge_grads_flat`
    (sum N, C).  ``charges=`` of a call is one flat (sum N, C) tensor or a list of F (N_f, C) tensors, exactly these shapes.

    Not served: the slab term, ``neighbors=`` streams, frames with different potentials or channel counts.

    :param calculator: one :class:`EwaldCalculator` for all frames, under the rules of :class:`GraphedEwaldStep`: the potential
        exactly a :class:`CoulombPotential` or an :class:`InversePowerLawPotential` (exponent 1..6), with or without exclusion
        radius, any ``prefactor``; half or full lists from ``calculator.full_neighbor_list``
    :param frames: sequence of ``(charges (N_f, 1), cell (3, 3), positions (N_f, 3), neighbor_indices (P_f, 2), neighbor_shifts
        (P_f, 3))``, one dtype (float32 or float64) and one device throughout; integer cell shifts in [-3, 3]
    :param cell_gradient: also return ``dE/dcell`` of every frame
    :param warmup: eager runs before the capture
    :param n_channels: the charge channels C of every frame, an ``int`` in 1..8 (:attr:`n_channels`); with the default 1 the
        object is the single-channel batch, entry point and bits
    """

    _who = "GraphedEwaldBatch"
    _table_bytes, _table_build = "mipme_ewald_batch_table_bytes", "mipme_ewald_batch_table_build"
    _values = property(lambda self: self.q)

    def __init__(self, calculator, frames, cell_gradient: bool = False, warmup: int = 3, n_channels: int = 1):
        who = "GraphedEwaldBatch"
        _check_ewald_calculator(who, calculator, "GraphedFrameBatch")
        _check_n_channels(who, n_channels)
        nc = self.n_channels = n_channels
        if nc > 1:
            self._table_bytes, self._table_build = "mipme_ewald_channels_batch_table_bytes", "mipme_ewald_channels_batch_table_build"
            self._table_args = (nc,)
        frames = [tuple(fr) for fr in frames]
        F = self.n_frames = len(frames)
        if F == 0:
            raise ValueError(f"{who}: `frames` is empty")
        if F > self.MAX_FRAMES:
            raise ValueError(f"{who} handles at most 2^20 frames, got {F}")
        self.lr_wavelength = float(calculator.lr_wavelength)
        first = frames[0][2] if len(frames[0]) == 5 else None
        grids = []
        for f, fr in enumerate(frames):
            if len(fr) != 5:
                raise ValueError(f"{who}: frame {f} must be (charges, cell, positions, neighbor_indices, neighbor_shifts), got "
                                 f"{len(fr)} items")
            charges, cell, positions, idx, shifts = fr
            _check_ewald_system(who, charges, cell, positions, frame=f, first=first, n_channels=nc)
            _check_explicit_list(who, idx, shifts, frame=f)
            for t in (charges, cell, idx, shifts, positions):
                if t.device != first.device:
                    raise ValueError(f"{who}: frame {f}: all tensors of all frames must be on one device, got {t.device} and "
                                     f"{first.device}")
            try:  # (raises ValueError for a singular cell)
                grids.append(_ewald_kgrid(cell, self.lr_wavelength))
            except ValueError as e:
                raise ValueError(f"{who}: frame {f}: {e}") from None
        for f, fr in enumerate(frames):
            for t, name in zip(fr, ("charges", "cell", "positions", "neighbor_indices", "neighbor_shifts")):
                _lib.require_device(t, f"{name} of frame {f}")
        self.calc = calculator
        self.cell_gradient = bool(cell_gradient)
        self.full = bool(calculator.full_neighbor_list)
        lib = self._lib = _lib.load()
        device, dtype = first.device, first.dtype
        self.device, self.dtype, self._dt = device, dtype, _lib.dtype_code(dtype)
        self._desc = calculator.potential._descriptor()
        counts = [fr[2].shape[0] for fr in frames]
        self._atom_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.atom_ptr = [int(v) for v in self._atom_ptr]
        self.ns, f_all, m_all = (list(x) for x in zip(*grids))
        self.n_k = [int(len(m)) for m in m_all]
        self._k_ptr = np.concatenate([[0], np.cumsum(self.n_k)]).astype(np.int64)
        self._ns = np.ascontiguousarray(np.asarray(self.ns, dtype=np.int32).reshape(F, 3))
        if nc == 1:
            n_work = int(lib.mipme_ewald_batch_work(F, self._atom_ptr.ctypes.data, self._k_ptr.ctypes.data, int(self.cell_gradient)))
        else:
            n_work = int(lib.mipme_ewald_channels_batch_work(F, self._atom_ptr.ctypes.data, self._k_ptr.ctypes.data, nc,
                                                             int(self.cell_gradient)))
        if n_work == 0:
            raise ValueError(f"{who}: the batch is beyond the limits of the frame table: the sums of the atoms ({self.atom_ptr[-1]}) "
                             f"and of the k-vectors ({int(self._k_ptr[-1])}) must stay below 2^31 and every launch below 2^24 "
                             "workgroups (the atom launch has sum_f N_f x slices_f)")
        SN, SK = self.atom_ptr[-1], int(self._k_ptr[-1])
        new = lambda *shape, dt=dtype: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
        self._freq = self._mult = self._kvec = self._G = self._Sc = self._Ss = self._dG = None
        if SK > 0:
            self._freq = torch.tensor(np.concatenate(f_all), device=device)
            self._mult = torch.tensor(np.concatenate(m_all), device=device)
            self._kvec, self._G, self._Sc, self._Ss = new(SK, 3), new(SK), new(nc * SK), new(nc * SK)
            self._dG = new(SK) if self.cell_gradient else None
        with torch.no_grad():
            self.pos = torch.cat([fr[2].detach() for fr in frames]).contiguous()
            self.q = torch.cat([fr[0].detach() for fr in frames]).contiguous()
            self.cells = torch.stack([fr[1].detach() for fr in frames]).contiguous()
        self._rec = new(SN, 4)
        self.energies, self.forces_flat, self.charge_grads_flat = new(F), new(SN, 3), new(SN, nc)
        self.cell_grads = new(F, 3, 3) if self.cell_gradient else None
        self.status = torch.zeros(F, dtype=torch.int32, device=device)
        self._work = new(max(1, n_work), dt=torch.float64)
        cut = lambda t: [t[a:b] for a, b in zip(self.atom_ptr[:-1], self.atom_ptr[1:])]  # noqa: E731
        self.forces, self.charge_grads = cut(self.forces_flat), cut(self.charge_grads_flat)
        self._warmup = max(1, int(warmup))
        self._install(self._pack([(fr[3], fr[4]) for fr in frames]))

    def _launch(self):
        with _lib.on_device(self.device):
            fields = dict(
                stream=_lib.current_stream(self.device), dtype=self._dt, full_list=int(self.full), pot=C.pointer(self._desc),
                n_frames=self.n_frames, cell_gradient=int(self.cell_gradient), lr_wavelength=self.lr_wavelength,
                atom_ptr=self._atom_ptr.ctypes.data, k_ptr=self._k_ptr.ctypes.data, entry_ptr=self._entry_ptr.ctypes.data,
                device_table=self._table.data_ptr(), positions=self.pos.data_ptr(), charges=self.q.data_ptr(),
                cells=self.cells.data_ptr(), frequencies=_lib.ptr(self._freq), multiplicities=_lib.ptr(self._mult),
                row_ptr=self._row_ptr.data_ptr(), entries=self._ent32.data_ptr(), shift_format=2, records=self._rec.data_ptr(),
                kvectors=_lib.ptr(self._kvec), G=_lib.ptr(self._G), dG=_lib.ptr(self._dG), s_cos=_lib.ptr(self._Sc),
                s_sin=_lib.ptr(self._Ss), energies=self.energies.data_ptr(), forces=self.forces_flat.data_ptr(),
                grad_charges=self.charge_grads_flat.data_ptr(), grad_cells=_lib.ptr(self.cell_grads), status=self.status.data_ptr(),
                work=self._work.data_ptr())
            if self.n_channels == 1:
                a = _lib.EwaldBatchArgs(**fields)
                _lib.check(self._lib.mipme_ewald_batch(C.byref(a)))
            else:
                a = _lib.EwaldChannelsBatchArgs(n_channels=self.n_channels, **fields)
                _lib.check(self._lib.mipme_ewald_channels_batch(C.byref(a)))

    def _check_charges(self, charges):
        """``charges=`` of a call on a multi-channel batch: exactly (sum N, C) or F tensors (N_f, C), checked before anything of
        the object changes (the single-channel batch keeps its own rules)."""
        if charges is None or self.n_channels == 1:
            return
        who = "GraphedEwaldBatch"
        if isinstance(charges, (list, tuple)):
            if len(charges) != self.n_frames:
                raise ValueError(f"{who}: a list of {self.n_frames} per-frame tensors wanted, got {len(charges)}")
            for f, t in enumerate(charges):
                _check_channel_charges(who, t, self.atom_ptr[f + 1] - self.atom_ptr[f], self.n_channels, frame=f)
        else:
            _check_channel_charges(who, charges, self.atom_ptr[-1], self.n_channels)

    def kgrid_matches(self, cells) -> list:
        """Per frame, whether the eager calculator would sum the frame's k grid for its cell in ``cells`` ((F, 3, 3) or a list):
        bit 0 of :attr:`status` clear, decided on the host."""
        if len(cells) != self.n_frames:
            raise ValueError(f"GraphedEwaldBatch: {self.n_frames} cells wanted, got {len(cells)}")
        return [GraphedEwaldStep._ns_of(c, self.lr_wavelength) == ns for c, ns in zip(cells, self.ns)]

    def recapture(self, lists, positions=None, charges=None, cells=None) -> None:
        """New neighbour lists, a sequence of F ``(neighbor_indices, neighbor_shifts)``: pack them, build the frame table again
        and capture the step again; the k grids and every buffer are kept.  Every list is validated and packed before anything of
        the object changes: a refused call leaves the object replaying what it replayed."""
        self._check_charges(charges)
        self._recapture(lists, positions, charges, cells)

    def __call__(self, positions=None, charges=None, cells=None):
        """``energies, forces, dE_dq`` (+ ``dE_dcell`` with ``cell_gradient``) of the current -- or the given -- positions, charges
        and cells of all frames: up to three copies and one graph replay."""
        self._check_charges(charges)
        self._load(positions, charges, cells)
        self.graph.replay()
        out = (self.energies, self.forces, self.charge_grads)
        if self.cell_gradient:
            out += (self.cell_grads,)
        return out


class GraphedDipoleBatch(_FrameTableBatch):
    """``energies, forces, dE_dmu = batch(positions, dipoles, cells)`` for MANY small systems of point dipoles and one
    :class:`~torchpme_amd.CalculatorDipole`, replayed from one HIP graph: the data-set form of
    ``GraphedDipoleStep(follow_cell=True)``, as :class:`GraphedEwaldBatch` is the data-set form of :class:`GraphedEwaldStep` --
    hundreds to thousands of polarisable or dipolar structures of 10 to 500 atoms, each with its own cell, its own atom count
    and its own k grid, whose energies, forces, fields (``-dE/dmu``) and stress labels are wanted together.  A
    :class:`GraphedDipoleStep` replay at these sizes is six or seven launches of a few dozen workgroups: latency, not work.  The
    batch runs the same seven launches ONCE for all frames (``mipme_dipole_batch``, csrc/dipole_batch.hip; a table maps every
    workgroup to its frame, no workgroup straddles two).

    For frame f, ``energies[f]``, ``forces[f]``, ``dE_dmu[f]`` and -- with ``cell_gradient`` -- ``dE_dcell[f]`` mean word for word
    what ``E``, ``F``, ``dE_dmu`` and ``dE_dcell`` of a ``GraphedDipoleStep(follow_cell=True)`` of that frame mean: total
    derivatives, the cell gradient at fixed Cartesian positions.  ``energies`` is (F,); ``forces`` and ``dE_dmu`` are lists of
    per-frame views into one flat buffer each, (sum N, 3), also exposed as :attr:`forces_flat` and :attr:`dipole_grads_flat`
    (the list of views as :attr:`dipole_grads`); ``dE_dcell`` is :attr:`cell_grads`, one (F, 3, 3) tensor.  All outputs are
    buffers of the object, overwritten by every call.

    A call copies whichever of ``positions``, ``dipoles`` and ``cells`` are given into the object's buffers -- each either one
    flat tensor in frame order or a list of F per-frame tensors, which goes in through ONE ``torch.cat(..., out=buffer)``
    (:attr:`cells` is the (F, 3, 3) input buffer) -- and replays one graph: no host reads, nothing re-captured, and nothing
    launched depends on any cell having the values it had at construction.  Every sum has a fixed order (no floating-point
    atomics), and a frame is computed from its own inputs alone: the bits it gets do not depend on its index, on F or on the
    other frames of the batch.

    The k grid of every frame is frozen at construction, as in the single step: :attr:`ns` ``[f]``, :attr:`n_k` ``[f]`` (one of
    every pair +-k).  :attr:`status` is a device ``int32`` (F,) tensor every replay writes, with the single step's two bits per
    frame -- bit 0: the eager call would use another k grid for this cell; bit 1: ``det(cell)`` is zero or not finite (that
    frame's energy and cell gradient are NaN, no other frame is touched) -- and :meth:`kgrid_matches` is the comparison of bit 0
    on the host.  :attr:`atom_ptr` holds the F + 1 host offsets of the frames in the flat buffers.  A direct potential (no
    smearing) sums no grid: ``lr_wavelength == 0.0``, every ``ns[f] == (1, 1, 1)`` and ``n_k[f] == 0``, bit 0 is never set.
    Frames with ``n_k == 0``, frames of one atom and frames with an empty list are served, mixed with others or alone.

    Not served: ``neighbors=`` streams, frames with different potentials, a double backward (the outputs are plain buffers, not
    part of an autograd graph).

    :param calculator: one :class:`CalculatorDipole` for all frames, with any :class:`PotentialDipole` the eager call accepts
        (direct or range separated, with or without exclusion radius, ``epsilon``, ``prefactor``); half or full lists from
        ``calculator.full_neighbor_list``
    :param frames: sequence of ``(dipoles (N_f, 3), cell (3, 3), positions (N_f, 3), neighbor_indices (P_f, 2), neighbor_shifts
        (P_f, 3))``, one dtype (float32 or float64) and one device throughout; integer cell shifts in [-3, 3]
    :param cell_gradient: also return ``dE/dcell`` of every frame
    :param warmup: eager runs before the capture
    """

    _who = "GraphedDipoleBatch"
    _table_bytes, _table_build = "mipme_dipole_batch_table_bytes", "mipme_dipole_batch_table_build"
    _values = property(lambda self: self.mu)

    @staticmethod
    def _check_system(who, f, dipoles, cell, positions, first):
        """Shapes, dtype and atom count of frame ``f``: the refusals of :class:`GraphedDipoleStep` with the frame's index."""
        pre = f"{who}: frame {f}: "
        if dipoles.dim() != 2 or dipoles.shape[1] != 3:
            raise ValueError(f"{pre}`dipoles` must be a tensor with shape [n_atoms, 3], got tensor with shape {list(dipoles.shape)}")
        if positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] != dipoles.shape[0]:
            raise ValueError(f"{pre}`positions` must be a tensor with shape [n_atoms, 3] with n_atoms = {dipoles.shape[0]} (the "
                             f"dipoles), got tensor with shape {list(positions.shape)}")
        if tuple(cell.shape) != (3, 3):
            raise ValueError(f"{pre}`cell` must be a tensor with shape [3, 3], got tensor with shape {list(cell.shape)}")
        shared = positions.dtype == dipoles.dtype == cell.dtype == first.dtype
        if not shared or positions.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{pre}`positions`, `dipoles` and `cell` of all frames must share one dtype, float32 or float64, got "
                             f"{positions.dtype}, {dipoles.dtype} and {cell.dtype} (frame 0: {first.dtype})")
        if positions.shape[0] < 1 or positions.shape[0] > (1 << 22):
            raise ValueError(f"{pre}a frame holds 1 to 2^22 atoms (the 4-byte pair entries of the row kernel), got "
                             f"{positions.shape[0]}")

    def __init__(self, calculator, frames, cell_gradient: bool = False, warmup: int = 3):
        from .dipoles import CalculatorDipole

        who = self._who
        if not isinstance(calculator, CalculatorDipole):
            raise TypeError(f"{who} serves a CalculatorDipole, got a {type(calculator).__name__}: use GraphedEwaldBatch or "
                            "GraphedFrameBatch for charges")
        frames = [tuple(fr) for fr in frames]
        F = self.n_frames = len(frames)
        if F == 0:
            raise ValueError(f"{who}: `frames` is empty")
        if F > self.MAX_FRAMES:
            raise ValueError(f"{who} handles at most 2^20 frames, got {F}")
        pot = calculator.potential
        sm, _, eps, pref = pot._host_params()
        self.lr_wavelength = float(calculator.lr_wavelength) if sm is not None else 0.0
        first = frames[0][2] if len(frames[0]) == 5 else None
        grids = []
        for f, fr in enumerate(frames):
            if len(fr) != 5:
                raise ValueError(f"{who}: frame {f} must be (dipoles, cell, positions, neighbor_indices, neighbor_shifts), got "
                                 f"{len(fr)} items")
            dipoles, cell, positions, idx, shifts = fr
            self._check_system(who, f, dipoles, cell, positions, first)
            _check_explicit_list(who, idx, shifts, frame=f)
            for t in (dipoles, cell, idx, shifts, positions):
                if t.device != first.device:
                    raise ValueError(f"{who}: frame {f}: all tensors of all frames must be on one device, got {t.device} and "
                                     f"{first.device}")
            det = float(np.linalg.det(cell.detach().to("cpu", torch.float64).numpy()))
            if det == 0.0 or not np.isfinite(det):
                raise ValueError(f"{who}: frame {f}: provided `cell` has a determinant of {det}, i.e. it is not a valid unit cell")
            if sm is None:  # (a direct potential: no grid to compare with)
                grids.append(((1, 1, 1), np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32)))
                continue
            try:
                grids.append(_ewald_kgrid(cell, self.lr_wavelength))
            except ValueError as e:
                raise ValueError(f"{who}: frame {f}: {e}") from None
        for f, fr in enumerate(frames):
            for t, name in zip(fr, ("dipoles", "cell", "positions", "neighbor_indices", "neighbor_shifts")):
                _lib.require_device(t, f"{name} of frame {f}")
        self.calc = calculator
        self.cell_gradient = bool(cell_gradient)
        self.full = bool(calculator.full_neighbor_list)
        lib = self._lib = _lib.load()
        device, dtype = first.device, first.dtype
        self.device, self.dtype, self._dt = device, dtype, _lib.dtype_code(dtype)
        self._desc = pot._descriptor()
        self._self_term, self._background = 0.0, 0.0
        if sm is not None:
            alpha = 0.5 / sm**2
            self._self_term = pref * 4 * math.pi / 3 * (alpha / math.pi) ** 1.5
            self._background = pref * 4 * math.pi / (2 * eps + 1) if eps != 0.0 else 0.0
        counts = [fr[2].shape[0] for fr in frames]
        self._atom_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.atom_ptr = [int(v) for v in self._atom_ptr]
        self.ns, f_all, m_all = (list(x) for x in zip(*grids))
        self.n_k = [int(len(m)) for m in m_all]
        self._k_ptr = np.concatenate([[0], np.cumsum(self.n_k)]).astype(np.int64)
        self._ns = np.ascontiguousarray(np.asarray(self.ns, dtype=np.int32).reshape(F, 3))
        n_work = int(lib.mipme_dipole_batch_work(F, self._atom_ptr.ctypes.data, self._k_ptr.ctypes.data, int(self.cell_gradient)))
        if n_work == 0:
            raise ValueError(f"{who}: the batch is beyond the limits of the frame table: the sums of the atoms ({self.atom_ptr[-1]}) "
                             f"and of the k-vectors ({int(self._k_ptr[-1])}) must stay below 2^31 and every launch below 2^24 "
                             "workgroups (the atom launch has sum_f N_f x slices_f)")
        SN, SK = self.atom_ptr[-1], int(self._k_ptr[-1])
        new = lambda *shape, dt=dtype: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
        self._freq = self._mult = self._kvec = self._G = self._Sc = self._Ss = self._dG = None
        if SK > 0:
            self._freq = torch.tensor(np.concatenate(f_all), device=device)
            self._mult = torch.tensor(np.concatenate(m_all), device=device)
            self._kvec, self._G, self._Sc, self._Ss = new(SK, 3), new(SK), new(SK), new(SK)
            self._dG = new(SK) if self.cell_gradient else None
        with torch.no_grad():
            self.pos = torch.cat([fr[2].detach() for fr in frames]).contiguous()
            self.mu = torch.cat([fr[0].detach() for fr in frames]).contiguous()
            self.cells = torch.stack([fr[1].detach() for fr in frames]).contiguous()
        self._rec = new(2 * SN, 4)
        self.energies, self.forces_flat, self.dipole_grads_flat = new(F), new(SN, 3), new(SN, 3)
        self.cell_grads = new(F, 3, 3) if self.cell_gradient else None
        self.status = torch.zeros(F, dtype=torch.int32, device=device)
        self._work = new(max(1, n_work), dt=torch.float64)
        cut = lambda t: [t[a:b] for a, b in zip(self.atom_ptr[:-1], self.atom_ptr[1:])]  # noqa: E731
        self.forces, self.dipole_grads = cut(self.forces_flat), cut(self.dipole_grads_flat)
        self._warmup = max(1, int(warmup))
        self._install(self._pack([(fr[3], fr[4]) for fr in frames]))

    def _launch(self):
        with _lib.on_device(self.device):
            a = _lib.DipoleBatchArgs(
                stream=_lib.current_stream(self.device), dtype=self._dt, full_list=int(self.full), pot=C.pointer(self._desc),
                self_term=self._self_term, background=self._background, n_frames=self.n_frames,
                cell_gradient=int(self.cell_gradient), lr_wavelength=self.lr_wavelength, atom_ptr=self._atom_ptr.ctypes.data,
                k_ptr=self._k_ptr.ctypes.data, entry_ptr=self._entry_ptr.ctypes.data, device_table=self._table.data_ptr(),
                positions=self.pos.data_ptr(), dipoles=self.mu.data_ptr(), cells=self.cells.data_ptr(),
                frequencies=_lib.ptr(self._freq), multiplicities=_lib.ptr(self._mult), row_ptr=self._row_ptr.data_ptr(),
                entries=self._ent32.data_ptr(), shift_format=2, records=self._rec.data_ptr(), kvectors=_lib.ptr(self._kvec),
                G=_lib.ptr(self._G), dG=_lib.ptr(self._dG), s_cos=_lib.ptr(self._Sc), s_sin=_lib.ptr(self._Ss),
                energies=self.energies.data_ptr(), forces=self.forces_flat.data_ptr(),
                grad_dipoles=self.dipole_grads_flat.data_ptr(), grad_cells=_lib.ptr(self.cell_grads),
                status=self.status.data_ptr(), work=self._work.data_ptr())
            _lib.check(self._lib.mipme_dipole_batch(C.byref(a)))

    def kgrid_matches(self, cells) -> list:
        """Per frame, whether the eager calculator would sum the frame's k grid for its cell in ``cells`` ((F, 3, 3) or a list):
        bit 0 of :attr:`status` clear, decided on the host.  A direct potential sums no grid: all ``True``."""
        if len(cells) != self.n_frames:
            raise ValueError(f"GraphedDipoleBatch: {self.n_frames} cells wanted, got {len(cells)}")
        if self.lr_wavelength <= 0.0:
            return [True] * self.n_frames
        return [GraphedEwaldStep._ns_of(c, self.lr_wavelength) == ns for c, ns in zip(cells, self.ns)]

    def recapture(self, lists, positions=None, dipoles=None, cells=None) -> None:
        """New neighbour lists, a sequence of F ``(neighbor_indices, neighbor_shifts)``: pack them, build the frame table again
        and capture the step again; the k grids and every buffer are kept.  Every list is validated and packed before anything of
        the object changes: a refused call leaves the object replaying what it replayed."""
        self._recapture(lists, positions, dipoles, cells)

    def __call__(self, positions=None, dipoles=None, cells=None):
        """``energies, forces, dE_dmu`` (+ ``dE_dcell`` with ``cell_gradient``) of the current -- or the given -- positions,
        dipoles and cells of all frames: up to three copies and one graph replay."""
        self._load(positions, dipoles, cells)
        self.graph.replay()
        out = (self.energies, self.forces, self.dipole_grads)
        if self.cell_gradient:
            out += (self.cell_grads,)
        return out
