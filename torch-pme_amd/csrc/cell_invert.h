// The float64 cell inversion of the steps whose cell is a replay input (ewald_step.hip, ewald_batch.hip, frames_cells.hip), and
// what the frame batches derive from a cell that arrives on the device (frames_cells.hip; on the host: mipme_frames_cell_geometry).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

namespace mipme {

using std::isfinite;  // (the host side of the __host__ __device__ bodies below: unqualified, the name finds device overloads only)

// A^-T (rows b x c / det, c x a / det, a x b / det), 1 / |det| and "det is zero or not finite" of the cell, in float64
struct EsCell {
  double recip[9], inv_vol;
  bool bad;
};
template <typename T>
__host__ __device__ __forceinline__ EsCell es_invert_cell(const T* __restrict__ cell, double (&A)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) A[k] = double(cell[k]);
  EsCell g;
  const double* a = A;
  const double* b = A + 3;
  const double* c = A + 6;
  g.recip[0] = b[1] * c[2] - b[2] * c[1], g.recip[1] = b[2] * c[0] - b[0] * c[2], g.recip[2] = b[0] * c[1] - b[1] * c[0];
  g.recip[3] = c[1] * a[2] - c[2] * a[1], g.recip[4] = c[2] * a[0] - c[0] * a[2], g.recip[5] = c[0] * a[1] - c[1] * a[0];
  g.recip[6] = a[1] * b[2] - a[2] * b[1], g.recip[7] = a[2] * b[0] - a[0] * b[2], g.recip[8] = a[0] * b[1] - a[1] * b[0];
  const double det = a[0] * g.recip[0] + a[1] * g.recip[1] + a[2] * g.recip[2];
  g.bad = !(det != 0.0) || !isfinite(det);
  const double inv_det = 1.0 / det;
#pragma unroll
  for (int k = 0; k < 9; ++k) g.recip[k] *= inv_det;
  g.inv_vol = fabs(inv_det);
  return g;
}

// ---- the geometry of one frame of a batch that follows its cell (GraphedFrameBatch(follow_cells=True)) -------------------------
// status bits of a frame
constexpr int kCellMeshDiffers = 1;  // the mesh rule of the reference would give another mesh than the frozen one
constexpr int kCellBad = 2;          // the cell is singular or not finite (in float64, or in a value as the batch's dtype stores it)

struct FrameCellGeom {
  double A[9];     // the cell, float64 copies of the values of T
  double inv[9];   // A^-1, row-major (mipme_mesh_t.inv_cell, Geom::inv, KGeom::inv)
  double vol, inv_vol;
  double norm[3];  // |a_d|
  int status;      // kCellMeshDiffers | kCellBad
};

// is n_d what 2^ceil(log2(x)) gives, x = 2 |a_d| / h + 1 (ops.ns_mesh_from_cell; reference lib/kvectors.py:5-21)?  Without a
// logarithm: n / 2 < x <= n for a power of two n >= 2, x <= 1 for n = 1; a mesh size that is no power of two never is.
__host__ __device__ inline bool mesh_rule_gives(int n, double x) {
  if (n <= 0 || (n & (n - 1)) != 0) return false;
  if (n == 1) return x <= 1.0;
  return 0.5 * double(n) < x && x <= double(n);
}

template <typename T>
__host__ __device__ inline bool finite_as(double v) {
  return isfinite(v) && fabs(v) <= double(std::numeric_limits<T>::max());
}

// Inversion, validity and the mesh rule: one body for the kernel and for the host entry point.  A bad cell: det is zero (to within
// its rounding error, below) or not finite, or one of the values the launch would store -- the cell, its inverse, 1 / |det| as T, the volume, the row norms -- is
// not finite in the type it is stored in.  Bit 0 is evaluated whenever the row norms are finite.
template <typename T>
__host__ __device__ inline FrameCellGeom frame_cell_geometry(const T* __restrict__ cell, int nx, int ny, int nz, double mesh_spacing) {
  FrameCellGeom g;
  const EsCell e = es_invert_cell<T>(cell, g.A);
  bool bad = e.bad;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) g.inv[3 * c + d] = e.recip[3 * d + c];
  g.inv_vol = e.inv_vol;
  g.vol = 1.0 / e.inv_vol;
#pragma unroll
  for (int k = 0; k < 9; ++k) bad = bad || !isfinite(g.A[k]) || !isfinite(g.inv[k]);
  bad = bad || !finite_as<T>(g.inv_vol) || !isfinite(g.vol);
  const int ns[3] = {nx, ny, nz};
  bool differs = false, norms_ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double* a = g.A + 3 * d;
    g.norm[d] = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    norms_ok = norms_ok && finite_as<T>(g.norm[d]);
  }
  if (norms_ok && mesh_spacing > 0.0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) differs = differs || !mesh_rule_gives(ns[d], 2.0 * g.norm[d] / mesh_spacing + 1.0);
  }
  bad = bad || !norms_ok;
  // "det is zero" means zero to within the rounding error of its own evaluation: six triple products of magnitude up to
  // |a| |b| |c|, each a few units in the last place off.  Two equal rows give a det of that size, not an exact zero, and an inverse
  // formed from it would be finite noise.  (A cell as skewed as 1e-3 of its Hadamard bound is fourteen orders away from this.)
  bad = bad || !(g.vol > 32.0 * 2.220446049250313e-16 * ((g.norm[0] * g.norm[1]) * g.norm[2]));
  g.status = (differs ? kCellMeshDiffers : 0) | (bad ? kCellBad : 0);
  return g;
}

}  // namespace mipme
