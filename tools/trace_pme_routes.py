"""Launch-for-launch trace of the calculator's autograd node (``ops._PMEFunction``) over its routes.

Every C-ABI call that passes through ``ops._call`` / ``ops._scaled_match`` / ``mipme_set_skip_flag`` is written down with its
label, its C symbol and every argument as the function's ``argtypes`` describe it: pointers as ``null`` / ``set``, integers and
doubles by value, structs behind a ``byref`` field by field (``mipme_sr_job_t`` behind its pointer included).  Two runs of the
same code give the same text; a refactoring of the node's host code must give the same text as its parent.

    python tools/trace_pme_routes.py [output file] [case ...]

The system is the 343-atom box of ``tests/test_gpu_contract.py::setup`` (bricks, planes and the gather tail are all reached);
every case is evaluated twice (the second call meets the caches and the tabulated pair sum).  ``CASES`` is also what
``tests/test_gpu_pme_routes.py`` pins: ``run_case(name)`` returns the trace lines, the ``ops.PROFILE``-style label sequence and
the facts of the node of each evaluation."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torchpme_amd as tpa  # noqa: E402
from torchpme_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BASE = dict(dtype=torch.float32, scheme="P3M", order=5, expo=1, tri=False, mesh=True, channels=1, full_list=False, mask=False,
            slab=False, distances="virtual", reduce="weighted_sum", grads=("pos",), stream=False, graphed=None, flags={})

#: one base case and one case per axis varied alone
CASES = {
    "base": {},
    "fp64": dict(dtype=torch.float64),
    "pme4_triclinic": dict(scheme="PME", order=4, tri=True),
    "r6": dict(expo=6),
    "no_mesh": dict(mesh=False),
    "two_channels": dict(channels=2),
    "full_list": dict(full_list=True),
    "mask": dict(mask=True),
    "slab": dict(slab=True),
    "slab_tensor_ops": dict(slab=True, reduce="tensor_ops"),
    "slab_two_channels": dict(slab=True, channels=2),
    "dist_plain": dict(distances="plain"),
    "dist_default": dict(distances="default"),
    "dist_deferred": dict(distances=True),
    "reduce_tensor_ops": dict(reduce="tensor_ops"),
    "reduce_sum": dict(reduce="sum"),
    "reduce_random": dict(reduce="random"),
    "grads_all": dict(grads=("q", "cell", "pos")),
    "grads_charges": dict(grads=("q",)),
    "grads_cell": dict(grads=("cell",)),
    "stream": dict(stream=True),
    "graphed": dict(graphed={}),
    "graphed_contract": dict(graphed=dict(charge_gradient=True, cell_gradient=True)),
    "graphed_log": dict(graphed=dict(energy_log=4)),
    "pair_atomic": dict(flags=dict(PAIR_MODE="atomic")),
    "mesh_atomic": dict(flags=dict(MESH_MODE="atomic")),
    "no_xfused": dict(flags=dict(XFUSED=False)),
    "no_coschedule": dict(flags=dict(COSCHEDULE=False)),
    "no_compact_entries": dict(flags=dict(COMPACT_ENTRIES=False)),
    "no_tail_fusion": dict(flags=dict(TAIL_FUSION=False)),
    "no_energy_fast_path": dict(flags=dict(ENERGY_FAST_PATH=False)),
    "no_energy_detect": dict(flags=dict(ENERGY_DETECT=False), reduce="tensor_ops"),
    "no_fuse_distances": dict(flags=dict(FUSE_DISTANCES=False)),
    "no_tabulate": dict(flags=dict(TABULATE=False), distances="plain"),
    "device_select": dict(flags=dict(DEVICE_SELECT_MIN_ATOMS=0), distances="default", reduce="tensor_ops"),
}

_SCALARS = (C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_double)


def _value(ctype, v):
    """One argument or struct field as text."""
    if ctype is C.c_void_p:
        v = v.value if isinstance(v, C.c_void_p) else v
        return "set" if v else "null"
    if ctype in _SCALARS:
        return repr(v.value if isinstance(v, C._SimpleCData) else v)
    if isinstance(ctype, type) and issubclass(ctype, C.Array):
        return "[" + " ".join(repr(x) for x in v) + "]"
    if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
        if v is None:
            return "null"
        obj = getattr(v, "_obj", None)  # the struct behind a byref()
        if obj is None:
            if not v:
                return "null"
            obj = v.contents
        if isinstance(obj, C.Structure):
            return _struct(obj)
        return "set"
    if isinstance(ctype, type) and issubclass(ctype, C.Structure):
        return _struct(v)
    return f"<{ctype.__name__}>"


def _struct(s):
    return type(s).__name__ + "{" + ", ".join(f"{n}={_value(t, getattr(s, n))}" for n, t in s._fields_) + "}"


class Recorder:
    """Wraps ``ops._call``, ``ops._scaled_match`` and ``mipme_set_skip_flag`` while active."""

    def __init__(self):
        self.lines, self.labels = [], []

    def __enter__(self):
        lib = _lib.load()
        self._saved = (ops._call, ops._scaled_match, lib.mipme_set_skip_flag)
        call, match, skip = self._saved

        def traced_call(name, fn, *args):
            types = fn.argtypes
            assert len(types) == len(args), (fn.__name__, len(types), len(args))
            self.labels.append(name)
            self.lines.append(f"{name} {fn.__name__}(" + ", ".join(_value(t, a) for t, a in zip(types, args)) + ")")
            call(name, fn, *args)

        def traced_match(lib_, st, dt, n, g, q, res, flag_ptr):
            self.lines.append(f"_scaled_match(dtype={dt}, n={n}, flag={'set' if flag_ptr else 'null'})")
            match(lib_, st, dt, n, g, q, res, flag_ptr)

        def traced_skip(p):
            self.lines.append(f"mipme_set_skip_flag({'set' if p else 'null'})")
            return skip(p)

        ops._call, ops._scaled_match, lib.mipme_set_skip_flag = traced_call, traced_match, traced_skip
        return self

    def __exit__(self, *exc):
        ops._call, ops._scaled_match, _lib.load().mipme_set_skip_flag = self._saved
        return False


def _node_facts(node, rec):
    if node is None or not hasattr(node, "tail"):
        rec.lines.append(f"node: {None if node is None else node.name()}")
        return None
    tail = node.tail
    set_keys = None if tail is None else tuple(sorted(k for k, v in tail.items() if v is not None and v is not False))
    facts = dict(tail=set_keys, field=node.field is not None, fused=node.fused is not None,
                 force=node.fused is not None and node.fused["force"] is not None, slab_in_tail=bool(node.slab_in_tail),
                 energy_direct=bool(node.energy_direct), full_list=bool(node.full_list))
    rec.lines.append("node: " + ", ".join(f"{k}={v}" for k, v in facts.items()))
    return facts


def _evaluate(o, c, calc, rec, extra):
    """One forward + backward of the case; returns the facts of the node."""
    leaves = {k: c[k].clone().requires_grad_(k in o["grads"]) for k in ("q", "cell", "pos")}
    q, cell, pos = leaves["q"], leaves["cell"], leaves["pos"]
    pairs, shifts = extra["pairs"], extra["shifts"]
    if o["stream"]:
        nl = tpa.NeighborStream(pos, cell, c["rc"])
        pairs, d = nl.indices, nl.distances(pos, cell)
    elif o["distances"] == "plain":
        d = extra["plain"]
    else:
        d = tpa.pair_distances(pos, pairs, cell, shifts, deferred={"default": False}.get(o["distances"], o["distances"]))
    kw = {}
    if o["mask"]:
        kw["pair_mask"] = extra["mask"]
    if o["slab"]:
        kw["periodic"] = extra["periodic"]
    V = calc(q, cell, pos, pairs, d, **kw)
    facts = _node_facts(V.grad_fn, rec)
    if o["reduce"] == "weighted_sum":
        E = tpa.weighted_sum(V, q)
    elif o["reduce"] == "tensor_ops":
        E = (q * V).sum()
    elif o["reduce"] == "sum":
        E = V.sum()
    else:
        E = (extra["upstream"] * V).sum()
    E.backward()
    torch.cuda.synchronize()
    return facts


def run_case(name):
    """``(trace lines, [labels of evaluation 1, of evaluation 2], [node facts of each])`` of one case of ``CASES``."""
    from test_gpu_contract import setup

    o = dict(BASE, **CASES[name])
    torch.manual_seed(0)
    saved = {k: getattr(ops, k) for k in o["flags"]}
    saved["FRONT"] = ops.FRONT
    ops._TOPOLOGIES.clear()
    ops._BET_PAUSE[0] = 0
    rec = Recorder()
    labels, facts = [], []
    try:
        ops.FRONT = False
        for k, v in o["flags"].items():
            setattr(ops, k, v)
        c = setup(o["dtype"], o["scheme"], o["order"], o["expo"], o["tri"])
        dtype = o["dtype"]
        extra = dict(pairs=c["pairs"], shifts=c["shifts"])
        if o["full_list"]:
            extra["pairs"] = torch.cat([c["pairs"], c["pairs"].flip(1)]).contiguous()
            extra["shifts"] = torch.cat([c["shifts"], -c["shifts"]]).contiguous()
        if o["channels"] == 2:
            c["q"] = torch.cat([c["q"], -2.0 * c["q"]], dim=1).contiguous()
        rng = np.random.default_rng(17)
        extra["upstream"] = torch.tensor(rng.normal(size=tuple(c["q"].shape)), dtype=dtype, device=DEV)
        extra["mask"] = torch.tensor(rng.random(extra["pairs"].shape[0]) < 0.9, device=DEV)
        extra["periodic"] = torch.tensor([True, True, False], device=DEV)
        if o["distances"] == "plain":
            extra["plain"] = tpa.pair_distances(c["pos"], extra["pairs"], c["cell"], extra["shifts"]).detach().clone()
        calc = c["calc"]
        if not o["mesh"]:
            calc = tpa.Calculator(tpa.CoulombPotential(), full_neighbor_list=o["full_list"])
        elif o["full_list"]:
            calc.full_neighbor_list = True
        torch.cuda.synchronize()
        with rec:
            for rep in (1, 2):
                rec.lines.append(f"== {name}, evaluation {rep}")
                first = len(rec.labels)
                if o["graphed"] is not None:
                    step = tpa.GraphedEnergyForces(calc, c["q"], c["cell"], c["pos"], c["pairs"], c["shifts"], **o["graphed"])
                    facts.append(dict(tail=None if step._tail is None else tuple(sorted(
                        k for k, v in step._tail.items() if v is not None and v is not False))))
                    rec.lines.append(f"node: tail={facts[-1]['tail']}, fused_contract={step._fused_contract}")
                    step()
                    torch.cuda.synchronize()
                    del step
                else:
                    facts.append(_evaluate(o, c, calc, rec, extra))
                labels.append(rec.labels[first:])
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    return rec.lines, labels, facts


def main(argv):
    out = argv[0] if argv else None
    names = argv[1:] or list(CASES)
    lines = []
    for name in names:
        lines += run_case(name)[0]
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
