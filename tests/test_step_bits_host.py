"""``tools/step_bits.py`` takes its systems from helpers of ``tests/test_gpu_dipole_step.py`` and ``tests/test_gpu_combined_step.py``
and reads one buffer of ``GraphedCombinedStep``; nothing in the suite runs the tool.  This walks, without a GPU, everything the
tool does before it builds a step, and checks the names it uses afterwards: a rename in the tests or in the class fails here."""

import importlib.util
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("step_bits", os.path.join(ROOT, "tools", "step_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_systems_of_the_tool_exist():
    tool = _tool()
    dipole = list(tool.dipole_systems())
    assert len(dipole) == len(tool.D.GOLD["tric_variants"]) + 2 + 3 + 3
    for name, calc, system in dipole:
        assert len(system) == 5 and len(system[0]) == len(system[1]), name
    combined = list(tool.combined_cases())
    assert len(combined) == 8 + 4
    for name, s, (members, weights), kind, full in combined:
        assert {"q", "pos", "cell", "pairs", "shifts", "spacing"} <= set(s) and len(members) == len(weights), name


def test_the_cell_step_variant_of_the_tool():
    """``run_dipole(..., follow_cell=True)``: the strain is the golden script's, the names it builds the step from exist, and the
    class takes the two keywords and has the status word."""
    import numpy as np

    tool = _tool()
    assert "follow_cell" in inspect.signature(tool.run_dipole).parameters
    m = tool.strain()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dipole_cell_step.npz"))
    assert m.shape == (3, 3) and np.array_equal(m, np.eye(3) + gold["strain"]) and np.abs(gold["strain"]).max() > 0
    assert callable(tool.D._t) and hasattr(tool.D, "DEV")
    params = inspect.signature(tool.tpa.GraphedDipoleStep.__init__).parameters
    assert "follow_cell" in params and "cell_gradient" in params
    assert "cell" in inspect.signature(tool.tpa.GraphedDipoleStep.__call__).parameters
    assert "self.status" in inspect.getsource(tool.tpa.GraphedDipoleStep)


def test_the_names_the_tool_uses_behind_them():
    tool = _tool()
    assert callable(tool.D._build) and "cell_gradient" in inspect.signature(tool.D._build).parameters
    for name in ("_calculator", "_combination", "_tensors"):
        assert callable(getattr(tool.C, name)), name
    import torchpme_amd as tpa

    params = inspect.signature(tpa.GraphedCombinedStep.__init__).parameters
    assert "weight_gradient" in params and "charge_gradient" in params
    assert "self._pair_force" in inspect.getsource(tpa.GraphedCombinedStep.__init__)
