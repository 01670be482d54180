"""Phase timeline of the inverse (y,z) plane workgroups of the headline step (water box, 64^3, fp32): library built with
``bash tools/build_variant.sh ytimeline -DMIPME_WG_TIMELINE=2``, run with MIPME_LIB=<that .so> and, for the split kernels,
MIPME_INV_PLANE_SPLIT=2 / 4.  Every plane workgroup stamps entry, tile loaded, y done, z done, stored (fft_lds.h MIPME_YZ_PHASE);
this prints how its lifetime divides into these phases and when the workgroups start and end (profiles/inverse_planes_split.txt).
A stamped build is read for its SHARES, not for its length."""
import ctypes as C, os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchpme_amd as tpa
from torchpme_amd import workloads, _lib
w = workloads.water_box()
dev = torch.device("cuda"); dt = torch.float32
pos = torch.tensor(w.positions, device=dev, dtype=dt); cell = torch.tensor(w.cell, device=dev, dtype=dt); q = torch.tensor(w.charges, device=dev, dtype=dt)
pairs = torch.tensor(w.pairs, device=dev); shifts = torch.tensor(w.shifts, device=dev, dtype=dt)
calc = tpa.P3MCalculator(tpa.CoulombPotential(smearing=w.smearing), mesh_spacing=w.mesh_spacing, interpolation_nodes=w.order)
step = tpa.GraphedEnergyForces(calc, q, cell, pos, pairs, shifts)
lib = _lib.load()
split = lib.mipme_last_inverse_split()
n_wg = 64 * split
lib.mipme_debug_yz_phase.argtypes = [C.c_void_p, C.c_int]
names = ("load", "y", "merge+z", "store")
for reading in range(4):
    for _ in range(20): step()
    torch.cuda.synchronize()
    ph = np.zeros(1024 * 8, dtype=np.int64)
    assert lib.mipme_debug_yz_phase(ph.ctypes.data, 1024 * 8) == 0
    t = ph.reshape(1024, 8)[:n_wg, :5] * 0.01  # us
    t0 = t[:, 0].min()
    d = np.diff(t, axis=1)
    life = t[:, 4] - t[:, 0]
    print(f"reading {reading}: split {split}, {n_wg} plane workgroups; start {t[:, 0].min() - t0:.2f}..{t[:, 0].max() - t0:.2f}  "
          f"end {t[:, 4].min() - t0:.2f}..{t[:, 4].max() - t0:.2f}  lifetime mean {life.mean():.2f} median {np.median(life):.2f} max {life.max():.2f}")
    print("   phase mean us:  " + "  ".join(f"{n} {d[:, i].mean():.2f}" for i, n in enumerate(names))
          + "   share of lifetime:  " + "  ".join(f"{n} {100 * d[:, i].sum() / life.sum():.0f}%" for i, n in enumerate(names)))
