"""The bits of the Ewald step and of its batched form: one SHA-256 line per output tensor.

The five frames of ``tests/test_gpu_ewald_batch.py`` (1, 2, 17, 24 and 300 atoms, from the goldens) go through
``GraphedEwaldStep`` (each frame) and through ``GraphedEwaldBatch`` (all five, and each alone): C1 (Coulomb) and C2 (1/r^6),
half and full lists, fp32 and fp64, with and without the cell gradient, at the construction cell and -- from the same graph --
at the strained cell with the strained positions, and once with a singular cell for frame 1.  Every sum of these steps has a
fixed order, so two runs of the same code give the same text, and a change that only moves the device code must give the same
text as its parent.  The text ends with one ``##`` line per configuration -- the number of its lines and the SHA-256 of
them -- and one for the whole: enough to compare two runs, and what ``profiles/ewald_one_body_bits.txt`` keeps.

    python tools/ewald_bits.py [output file]
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torchpme_amd as tpa  # noqa: E402
from test_gpu_ewald_batch import ALL, CALCS, LAM, STRAIN, _system, _t  # noqa: E402

KEYS = ("E", "F", "dE/dq", "dE/dcell")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def lines_of(tag, out, status):
    return [f"{tag} {key} {sha(o)}" for key, o in zip(KEYS, out)] + [f"{tag} status {sha(status)}"]


def run(cname, full, dtype, cell_gradient):
    calc = tpa.EwaldCalculator(CALCS[cname][0](), lr_wavelength=LAM, full_neighbor_list=full)
    systems = [_system(n, full) for n in ALL]
    frames = [(_t(q, dtype), _t(c, dtype), _t(p, dtype), torch.tensor(pairs, device="cuda"), _t(sh, dtype))
              for q, p, c, pairs, sh in systems]
    singular = systems[1][2].copy()
    singular[2] = singular[0]
    # (tag, per frame (positions, cell)): the construction cell, the strained one, frame 1 with two equal cell vectors
    calls = [("c0", [(_t(s[1], dtype), _t(s[2], dtype)) for s in systems]),
             ("c1", [(_t(s[1] @ STRAIN, dtype), _t(s[2] @ STRAIN, dtype)) for s in systems]),
             ("singular", [(_t(s[1], dtype), _t(singular if n == 1 else s[2], dtype)) for n, s in enumerate(systems)])]
    head = f"{cname} {'full' if full else 'half'} {str(dtype)[6:]} cg={int(cell_gradient)}"
    lines = []
    steps = [tpa.GraphedEwaldStep(calc, *fr, cell_gradient=cell_gradient) for fr in frames]
    batches = [(ALL, tpa.GraphedEwaldBatch(calc, frames, cell_gradient=cell_gradient))]
    batches += [((n,), tpa.GraphedEwaldBatch(calc, [frames[n]], cell_gradient=cell_gradient)) for n in ALL]
    for ctag, inputs in calls:
        for n, step in enumerate(steps):
            if ctag == "singular" and n != 1:
                continue
            out = step(positions=inputs[n][0], cell=inputs[n][1])
            torch.cuda.synchronize()
            lines += lines_of(f"{head} {ctag} step f{n}", out, step.status)
        for which, batch in batches:
            if ctag == "singular" and 1 not in which:
                continue
            out = batch(positions=[inputs[n][0] for n in which], cells=[inputs[n][1] for n in which])
            torch.cuda.synchronize()
            for f, n in enumerate(which):
                tag = f"{head} {ctag} batch of {len(which)} f{n}"
                lines += lines_of(tag, [o[f] for o in out], batch.status[f])
    return lines


def main(argv):
    lines, summary = [], []
    digest = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()  # noqa: E731
    for cname in CALCS:
        for full in (False, True):
            for dtype in (torch.float64, torch.float32):
                for cell_gradient in (True, False):
                    got = run(cname, full, dtype, cell_gradient)
                    lines += got
                    summary.append(f"## {' '.join(got[0].split()[:4])}: {len(got)} lines, sha256 {digest(got)}")
    summary.append(f"## all: {len(lines)} lines, sha256 {digest(lines)}")
    text = "\n".join([f"# {torch.cuda.get_device_name(0)}; sha256 of the raw bytes of every output"] + lines + summary) + "\n"
    if argv:
        with open(argv[0], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
