"""Where a GraphedDipoleBatch of ONE frame and the GraphedDipoleStep(follow_cell=True) of that frame agree to the bit.

The kernels of csrc/dipole_batch.hip are new text beside those of csrc/dipole_step.hip (the same arithmetic in the same order,
through the bodies of csrc/dipole_step_bodies.h), so equality is not promised; this prints where it holds: one line per frame of
``tests/test_gpu_dipole_batch.py``, calculator (D1, D2), dtype, cell (c0, the strained c1) and output -- ``equal`` or the largest
difference relative to the largest value -- and a ``##`` summary.  ``profiles/dipole_batch_bits.txt`` keeps the text.

    python tools/dipole_batch_bits.py [output file]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_dipole_batch as B  # noqa: E402


def main(argv):
    lines, n_equal, n_all = [], 0, 0
    for cname in ("D1", "D2"):
        for dtype in B.DTYPES:
            for n in B.ALL:
                step, batch = B._single(cname, dtype, n), B._batch(cname, dtype, which=(n,))
                _, p, c, _, _ = B._system(n, B.CALCS[cname][1])
                for ctag, m in (("c0", np.eye(3)), ("c1", B.STRAIN)):
                    pos, cell = B._t(p @ m, dtype), B._t(c @ m, dtype)
                    one = [o.clone() for o in step(positions=pos, cell=cell)] + [step.status[0].clone()]
                    got = B._bits(batch, positions=[pos], cells=[cell])[0]
                    for key, a, b in zip(("E", "F", "dE/dmu", "dE/dcell", "status"), one, got):
                        same = a.shape == b.shape and torch.equal(a, b)
                        n_equal, n_all = n_equal + same, n_all + 1
                        diff = float((a.double() - b.double()).abs().max() / max(1e-300, float(a.double().abs().max())))
                        lines.append(f"{cname} {str(dtype)[6:]} f{n} {ctag} {key}: " + ("equal" if same else f"differs, {diff:.2e} relative"))
    lines.append(f"## {n_equal} of {n_all} outputs equal to the bit")
    text = "\n".join([f"# {torch.cuda.get_device_name(0)}; batch of one frame against the single step that follows its cell"] + lines) + "\n"
    if argv:
        with open(argv[0], "w") as f:
            f.write(text)
    sys.stdout.write(text if not argv else lines[-1] + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
