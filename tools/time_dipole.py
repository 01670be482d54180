"""GPU timing of CalculatorDipole -- forward, and forward + backward w.r.t. positions, eager -- at three (N, K) sizes, against
the charge Ewald sum of EwaldCalculator at the same N and K (the in-repo yardstick, tools/time_ewald.py) and an eager-torch
restatement of the table algorithm (the (K, N) cos / sin tables, then two contractions) where its tables fit in memory.

    python tools/time_dipole.py [--quick]

--quick: fewer repetitions (for a run under rocprofv3 --kernel-trace --stats)."""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchpme_amd as tpa  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
TABLE_BYTES_MAX = 24 << 30  # the table restatement's (K, N) tables and their autograd copies, at most


def frame0():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dipole.npz"))
    return gold["frame0_positions"], gold["frame0_cell"], gold["frame0_dipoles"], float(gold["frame0_smearing"]), 0.1, 4.0


def random_box(n, L, lam, sm, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, L, (n, 3)), np.eye(3) * L, rng.normal(size=(n, 3)), sm, lam, 4.0


SIZES = [("N=8 (ESPResSo frame)", frame0), ("N=1000", lambda: random_box(1000, 27.0, 0.87, 1.5, 1)),
         ("N=8000", lambda: random_box(8000, 54.0, 2.0, 2.0, 2))]


def table_kspace(mu, pos, kv, G):
    """The table algorithm in eager torch: (K, N) phases, cos / sin tables, contractions (no 1/V, self or background)."""
    ph = kv @ pos.T
    c, s = torch.cos(ph), torch.sin(ph)
    q = kv @ mu.T
    Sc, Ss = (q * c).sum(dim=1), (q * s).sum(dim=1)
    return (c * (G * Sc)[:, None] + s * (G * Ss)[:, None]).T @ kv


def timed(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    reps = 3 if QUICK else 20
    print(f"# {torch.cuda.get_device_name(0)}; eager, ms per call (mean of {reps} after 2 warm-up calls)")
    for label, make in SIZES:
        pos, cell, mu, sm, lam, rc = make()
        pairs, S, _ = tpa.neighbor_list(pos, cell, rc)
        for dtype in (torch.float32, torch.float64):
            t = lambda a: torch.tensor(np.asarray(a), device=dev, dtype=dtype)  # noqa: E731
            tc, tm, tS = t(cell), t(mu), t(S)
            ti = torch.tensor(pairs, device=dev)
            tp = t(pos).requires_grad_(True)
            calc = tpa.CalculatorDipole(tpa.PotentialDipole(smearing=sm), lr_wavelength=lam)
            K = int(np.prod(np.ceil(np.linalg.norm(cell, axis=1) / lam)))

            def vectors():
                return tp[ti[:, 1]] - tp[ti[:, 0]] + tS @ tc

            def fwd():
                with torch.no_grad():
                    return calc(tm, tc, tp, ti, vectors())

            def fwd_bwd():
                tp.grad = None
                E = (calc(tm, tc, tp, ti, vectors()) * tm).sum()
                E.backward()

            # the charge Ewald sum at the same N and K: EwaldCalculator with one charge channel
            q = t(np.random.default_rng(0).normal(size=(len(pos), 1)))
            ew = tpa.EwaldCalculator(tpa.CoulombPotential(smearing=sm), lr_wavelength=lam).to(dtype)

            def ew_fwd_bwd():
                tp.grad = None
                d = tpa.pair_distances(tp, ti, tc, tS)
                E = tpa.weighted_sum(ew(q, tc, tp, ti, d), q)
                E.backward()

            ms_f, ms_fb, ms_ew = timed(fwd, reps), timed(fwd_bwd, reps), timed(ew_fwd_bwd, reps)
            line = (f"{label:22s} K={K:7d} P={len(pairs):7d} {str(dtype)[6:]:8s} dipole fwd {ms_f:9.3f}  fwd+bwd(pos) "
                    f"{ms_fb:9.3f} | charge Ewald fwd+bwd(pos) {ms_ew:9.3f}")
            itemsize = torch.finfo(dtype).bits // 8
            if 6 * K * len(pos) * itemsize <= TABLE_BYTES_MAX:
                kv = (2 * math.pi) * tpa.calculators._integer_frequencies(tc, lam)[0] @ torch.linalg.inv(tc).T
                G = calc.potential.to(dtype).lr_from_k_sq((kv * kv).sum(dim=1))
                tpd = tp.detach().requires_grad_(True)

                def table_fwd():
                    with torch.no_grad():
                        return table_kspace(tm, tpd, kv, G)

                def table_fwd_bwd():
                    tpd.grad = None
                    (table_kspace(tm, tpd, kv, G) * tm).sum().backward()

                line += f" | tables (k-space only) fwd {timed(table_fwd, reps):9.3f}  fwd+bwd(pos) {timed(table_fwd_bwd, reps):9.3f}"
            else:
                line += " | tables: do not fit"
            print(line, flush=True)


if __name__ == "__main__":
    main()
