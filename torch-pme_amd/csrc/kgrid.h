// The k-points of the rfft half grid: flat index -> integer frequencies -> k, |k|^2 and the P3M factor 1 / U^2.  Every kernel that
// tabulates a filter G(k) (kfilter.hip, spline.hip, combined.hip) takes these from here, so their tables are the same function
// of the mesh bit for bit; what differs between them is the kernel v(|k|^2) they multiply in.
// Reference: generate_kvectors_for_mesh (lib/kvectors.py:24-74), P3MKSpaceFilter._compute_influence / _charge_assignment
// (lib/kspace_filter.py:293-329,349-361).
#pragma once

#include <cmath>

#include "kpot.h"  // kPi

namespace mipme {

struct KGeom {
  double inv[9];  // inverse cell
  double h[3];    // |a_c| / n_c (P3M charge-assignment spacing, kspace_filter.py:308-311)
  int nx, ny, nz, nzh;
  int scheme, order;
};


static inline KGeom make_kgeom(const mipme_mesh_t* m) {
  KGeom g;
  for (int i = 0; i < 9; ++i) g.inv[i] = m->inv_cell[i];
  const int ns[3] = {m->nx, m->ny, m->nz};
  for (int c = 0; c < 3; ++c) {
    const double* a = m->cell + 3 * c;
    g.h[c] = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) / double(ns[c]);
  }
  g.nx = m->nx;
  g.ny = m->ny;
  g.nz = m->nz;
  g.nzh = m->nz / 2 + 1;
  g.scheme = m->scheme;
  g.order = m->order;
  return g;
}

__device__ inline int fft_freq(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }

// flat index p of the (nx, ny, nz/2 + 1) half grid -> (ix, iy, iz)
__device__ inline void half_grid_index(const KGeom& g, int64_t p, int& ix, int& iy, int& iz) {
  iz = int(p % g.nzh);
  const int64_t r = p / g.nzh;
  iy = int(r % g.ny);
  ix = int(r / g.ny);
}

// k = 2 pi A^-T f for the integer frequencies f (inv: the inverse cell, row major) into k[3]; returns |k|^2.  The multiply-adds
// are written out, not left to the compiler's contraction: every kernel that tabulates a filter calls this, so their tables
// agree bit for bit whatever gets fused around the call.
__device__ __forceinline__ double kvector_dev(const double* inv, const int* f, double* k) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
    k[c] = 2.0 * kPi * __builtin_fma(double(f[2]), inv[3 * c + 2],
                                     __builtin_fma(double(f[1]), inv[3 * c + 1], double(f[0]) * inv[3 * c + 0]));
  return __builtin_fma(k[2], k[2], __builtin_fma(k[0], k[0], k[1] * k[1]));
}

// 1 / U^2(k), U^2 = prod_c sinc(k_c h_c / 2)^(2 order), of the P3M filter G = v / U^2; 1 for Lagrange.  dead: U^2 = 0, where
// G = 0 -- callers store `dead ? 0 : v * inv`.
__device__ inline double p3m_inv_u2(const KGeom& g, const double* k, bool& dead) {
  dead = false;
  if (g.scheme == MIPME_LAGRANGE) return 1.0;
  double s = 1.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t = 0.5 * k[c] * g.h[c];
    s *= (t == 0.0) ? 1.0 : sin(t) / t;
  }
  double U2 = 1.0;
  const double s2 = s * s;
  for (int i = 0; i < g.order; ++i) U2 *= s2;
  dead = U2 == 0.0;
  return dead ? 0.0 : 1.0 / U2;
}

// point p of the half grid for a table builder: returns |k|^2, the factor 1 / U^2 and its dead flag
__device__ inline double kgrid_point(const KGeom& g, int64_t p, double& inv_u2, bool& dead) {
  int ix, iy, iz;
  half_grid_index(g, p, ix, iy, iz);
  const int f[3] = {fft_freq(ix, g.nx), fft_freq(iy, g.ny), iz};
  double k[3];
  const double k2 = kvector_dev(g.inv, f, k);
  inv_u2 = p3m_inv_u2(g, k, dead);
  return k2;
}

struct KPoint {
  double k[3];
  int f[3];
  double G, dGdk[3], dGdh[3];
  // dG/dk_c = alpha k_c - beta_c h_c,  dG/dh_c = -beta_c k_c: the four values per k-point the derivative table keeps
  double alpha, beta[3];
};

// Filter value and derivatives at the k-point (ix, iy, iz): the cell gradient's k-grid sums and the derivative table.  (The
// table G itself needs none of the derivatives: kfilter_kernel, from kgrid_point of kgrid.h.)
__device__ inline void eval_point(const KGeom& g, const KPot& kp, int ix, int iy, int iz, KPoint& o) {
  o.f[0] = fft_freq(ix, g.nx);
  o.f[1] = fft_freq(iy, g.ny);
  o.f[2] = iz;
  const double k2 = kvector_dev(g.inv, o.f, o.k);
  double v, dv;
  lr_kernel_dev(kp, k2, v, dv);
  if (g.scheme == MIPME_LAGRANGE) {
    o.G = v;
    o.alpha = 2.0 * dv;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o.dGdk[c] = 2.0 * o.k[c] * dv;
      o.dGdh[c] = 0.0;
      o.beta[c] = 0.0;
    }
    return;
  }
  // the sinc product of p3m_inv_u2 (kgrid.h) with ONE sincos per axis, the cosine being wanted too: the double-precision sin / cos
  // of libm are ~250 instructions each, and the cell-gradient sums of the x stage evaluate this for every k-point of the half
  // grid -- most of that kernel's extra 19 us
  double s = 1.0, t[3], sn[3], cs[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    t[c] = 0.5 * o.k[c] * g.h[c];
    sincos(t[c], &sn[c], &cs[c]);
    s *= (t[c] == 0.0) ? 1.0 : sn[c] / t[c];
  }
  double U2 = 1.0;
  const double s2 = s * s;
  for (int i = 0; i < g.order; ++i) U2 *= s2;
  if (U2 == 0.0) {
    o.G = 0.0;
    o.alpha = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) o.dGdk[c] = o.dGdh[c] = o.beta[c] = 0.0;
    return;
  }
  const double inv = 1.0 / U2;
  o.G = v * inv;
  o.alpha = 2.0 * dv * inv;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double tc = t[c];
    // d/dt ln(sin t / t) = cot t - 1/t
    const double L = fabs(tc) < 1e-4 ? (-tc / 3.0 - tc * tc * tc / 45.0) : (cs[c] / sn[c] - 1.0 / tc);
    const double w = o.G * double(2 * g.order) * L;
    o.dGdk[c] = 2.0 * o.k[c] * dv * inv - w * 0.5 * g.h[c];
    o.dGdh[c] = -w * 0.5 * o.k[c];
    o.beta[c] = 0.5 * w;
  }
}

}  // namespace mipme
