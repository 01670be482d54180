"""Workgroup timeline of the binned step's gather launch at cfg3 (tools/gather_timeline.py), the workgroups' lifetimes split by
the atom count of their brick: <= 64 (one pass of the gather's loop) against > 64 (two).  The counts are recomputed on the host
with the binning pass's rule.  Library built with -DMIPME_WG_TIMELINE=2 and named by MIPME_LIB
(profiles/gather_pairs.txt items 1 and 2):
    MIPME_LIB=torch-pme_amd/libmipme_gtimeline.so python tools/gather_timeline_split.py"""
import ctypes as C, os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchpme_amd as tpa
from torchpme_amd import workloads, _lib

w = workloads.water_box()
dev = torch.device("cuda"); dt = torch.float32
pos = torch.tensor(w.positions, device=dev, dtype=dt); cell = torch.tensor(w.cell, device=dev, dtype=dt); q = torch.tensor(w.charges, device=dev, dtype=dt)
calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=w.smearing), mesh_spacing=w.mesh_spacing, interpolation_nodes=w.order)
pairs = torch.tensor(w.pairs, device=dev); shifts = torch.tensor(w.shifts, device=dev, dtype=dt)
step = tpa.GraphedEnergyForces(calc, q, cell, pos, pairs, shifts)
lib = _lib.load()
lib.mipme_debug_wg_timeline.argtypes = [C.c_void_p, C.c_int]

# per-brick counts with the binning rule (odd order: nearest mesh point), from the float32 positions
n = 64
p32 = np.asarray(w.positions, dtype=np.float32).astype(np.float64)
inv = np.linalg.inv(np.asarray(w.cell, dtype=np.float32).astype(np.float64))
u = n * (p32 @ inv)
m = (np.rint(u) if w.order % 2 else np.floor(u)).astype(np.int64) % n
b = ((m[:, 0] // 8) * 8 + m[:, 1] // 8) * 8 + m[:, 2] // 8
counts = np.bincount(b, minlength=512)
print("order", w.order, "atoms", len(p32), "bricks > 64:", int((counts > 64).sum()), "max", counts.max(), "min", counts.min(), "mean %.1f" % counts.mean())
wg = np.arange(512)
brick = (wg & 7) * 64 + (wg >> 3)  # xcd_contiguous(wg, 512)
cw = counts[brick]

for rep in range(4):
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    buf = np.zeros(512 * 4, dtype=np.int64)
    assert lib.mipme_debug_wg_timeline(buf.ctypes.data, 512 * 4) == 0
    t = buf.reshape(512, 4)
    start, end = t[:, 0] * 0.01, t[:, 1] * 0.01
    t0 = start.min(); start = start - t0; end = end - t0
    d = end - start
    print("rep %d: launch span %.2f us; starts %.2f..%.2f" % (rep, end.max(), start.min(), start.max()))
    for nm, msk in (("<=64", cw <= 64), (">64", cw > 64)):
        print("   %-5s n=%3d  lifetime mean %.2f median %.2f max %.2f | end mean %.2f median %.2f p90 %.2f max %.2f | start mean %.2f" % (
            nm, int(msk.sum()), d[msk].mean(), np.median(d[msk]), d[msk].max(), end[msk].mean(), np.median(end[msk]),
            np.quantile(end[msk], 0.9), end[msk].max(), start[msk].mean()))
    last = np.argsort(end)[::-1][:16]
    print("   last 16 to end: counts", cw[last].tolist(), "ends", np.round(end[last], 2).tolist())
    print("   corr(count, lifetime) = %.3f" % np.corrcoef(cw, d)[0, 1])
