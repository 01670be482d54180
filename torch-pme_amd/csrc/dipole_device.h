// Device functions of the point-dipole kernels, shared by dipole.hip (the eager entry points) and dipole_step.hip (the
// graphed step): the phase k.r, the radial functions B, C, B'/r, C'/r of the pair tensor T = prefactor (B I - C r r^T) and the
// gradient of a^T T b.  See the head of dipole.hip for the formulas.
#pragma once

#include <cmath>

#include "common.h"
#include "srpot.h"

namespace mipme {

__device__ __forceinline__ void dipole_phase(float a, float& s, float& c) { sincosf(a, &s, &c); }
__device__ __forceinline__ void dipole_phase(double a, double& s, double& c) { sincos(a, &s, &c); }
// sin and cos of the phase k.r.  double: the phase in working precision.  float: the phase is formed and reduced in double --
// phi = k.r, n = rint(phi 2/pi) (by adding 1.5 2^52, whose low word then holds n), rho = phi - n pi/2 in [-pi/4, pi/4] -- and
// only rho is rounded to float; then sin(rho), cos(rho) from their degree-7 / degree-8 polynomials (the Cephes sinf / cosf
// coefficients: 1.3e-7 relative on that interval) and the quadrant swap.  A float phase carries an absolute error of
// |k.r| 2^-24 (4e-6 at |k.r| = 70): that was the accuracy limit of every float sum over k here, and next to a zero of cos or
// sin it left them no relative accuracy at all; this way both are good to 1.3e-7 of themselves.  (pi/2 as one double: n times
// its 6e-17 is below 2^-24 |rho| unless |rho| < 4e-9 n.)
__device__ __forceinline__ void dipole_phase3(double kx, double ky, double kz, double x, double y, double z, double& s,
                                              double& c) {
  sincos(kx * x + ky * y + kz * z, &s, &c);
}
__device__ __forceinline__ void dipole_phase3(float kx, float ky, float kz, float x, float y, float z, float& s, float& c) {
  constexpr double magic = 6755399441055744.0;  // 1.5 * 2^52
  const double phi = __builtin_fma(double(kx), double(x), __builtin_fma(double(ky), double(y), double(kz) * double(z)));
  const double t = __builtin_fma(phi, 0.63661977236758134308, magic);
  const int q = __double2loint(t);
  const float r = float(__builtin_fma(t - magic, -1.5707963267948966, phi)), z2 = r * r;
  const float sn = r + r * z2 * ((-1.9515295891e-4f * z2 + 8.3321608736e-3f) * z2 - 1.6666654611e-1f);
  const float cs = 1.0f - 0.5f * z2 + z2 * z2 * ((2.443315711809948e-5f * z2 - 1.388731625493765e-3f) * z2 + 4.166664568298827e-2f);
  const float a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;  // sin, cos up to sign
  s = __uint_as_float(__float_as_uint(a) ^ ((unsigned(q) & 2u) << 30));
  c = __uint_as_float(__float_as_uint(b) ^ ((unsigned(q + 1) & 2u) << 30));
}
__device__ __forceinline__ float dipole_erf(float y) { return erff(y); }
__device__ __forceinline__ double dipole_erf(double y) { return erf(y); }
__device__ __forceinline__ float dipole_exp(float x) { return expf(x); }
__device__ __forceinline__ double dipole_exp(double x) { return exp(x); }

static constexpr double kDipPi = 3.14159265358979323846;

template <typename T>
struct DipPot {
  int mode;  // 0: direct, 1: short range (erfc form), 2: exclusion -f_c T_lr (erf form)
  int deg;   // exclusion degree
  T pref, alpha, sqrt_alpha, kap, rx;
};

template <typename T>
static int make_dippot(const mipme_dipole_t* pot, DipPot<T>& d) {
  MIPME_REQUIRE(pot != nullptr, "dipole descriptor is NULL");
  const bool smeared = pot->smearing > 0, excl = pot->exclusion_radius > 0;
  MIPME_REQUIRE(!excl || pot->exclusion_degree >= 1, "exclusion_degree must be >= 1, got %d", pot->exclusion_degree);
  d.mode = smeared ? (excl ? 2 : 1) : 0;
  d.deg = pot->exclusion_degree;
  const double alpha = smeared ? 0.5 / (pot->smearing * pot->smearing) : 0.0;
  d.pref = T(pot->prefactor);
  d.alpha = T(alpha);
  d.sqrt_alpha = T(std::sqrt(alpha));
  d.kap = T(2.0 * std::sqrt(alpha / kDipPi));
  d.rx = T(excl ? pot->exclusion_radius : 0.0);
  return MIPME_OK;
}

// The long-range functions for x = alpha r^2 < 4 from the power series of the regularised lower incomplete gamma function,
//   P(a, x) = x^a e^-x S(a),  S(a) = sum_{k>=0} x^k / Gamma(a + k + 1),  S(a) = 1 / Gamma(a + 1) + x S(a + 1):
//   B_lr = P(3/2, x)/r^3 = alpha^(3/2) e^-x S(3/2),  C_lr = 3 P(5/2, x)/r^5 = 3 alpha^(5/2) e^-x S(5/2),
//   C_lr'/r = -15 P(7/2, x)/r^7 = -15 alpha^(7/2) e^-x S(7/2)
// (x^a / r^(2a) = alpha^a: no negative power of r, every term positive).  The erf forms below are differences whose leading
// terms cancel to order y^2, y^4, y^6: at y = 0.1 they left C with 5e-3 and C' with no correct digit in fp32, 4e-12 and 9e-10 in
// fp64.  One series, S(7/2), with the two others from the recurrence; term ratio x / (7/2 + k) < 8/9: 18 (float) / 32 (double)
// terms reach the rounding level at x = 4.  Below y = 2 the erf forms are also the less accurate ones for C' in fp32 (5e-6 on
// 1 <= y < 2), which is why the switch is not at x = 1 as in lower_gamma_series.
template <typename T>
__device__ __forceinline__ void dipole_lr_series(const DipPot<T>& P, T x, T e, T& B, T& C, T& dC) {
  constexpr int K = sizeof(T) == 4 ? 18 : 32;
  constexpr double ig52 = 0.75225277806367505, ig72 = 0.30090111122547002, ig92 = 0.085971746064420005;  // 1 / Gamma(a)
  T term = T(1), sum = T(1);
#pragma unroll
  for (int k = 1; k <= K; ++k) {
    term *= x * T(1.0 / (3.5 + k));
    sum += term;
  }
  const T s72 = T(ig92) * sum, s52 = T(ig72) + x * s72, s32 = T(ig52) + x * s52;
  const T a = P.alpha, a32e = a * P.sqrt_alpha * e;
  B = a32e * s32;
  C = T(3) * a * a32e * s52;
  dC = T(-15) * a * a * a32e * s72;
}

// B, C of the pair tensor at distance r (r2 = r^2, ri = 1/r); with GRAD also dB = B'/r and dC = C'/r.  EXCL: the exclusion
// variant (mode 2) -- an instantiation of its own, so that the series and the switch stay out of the instruction stream of
// the direct and the short-range form.
template <typename T, bool GRAD, bool EXCL>
__device__ __forceinline__ void dipole_bc(const DipPot<T>& P, T r2, T ri, T& B, T& C, T& dB, T& dC) {
  const T ri2 = ri * ri, ri3 = ri2 * ri, ri5 = ri3 * ri2;
  if (!EXCL && P.mode == 0) {
    B = ri3;
    C = T(3) * ri5;
    if (GRAD) {
      dB = T(-3) * ri5;
      dC = T(-15) * ri5 * ri2;
    }
    return;
  }
  const T r = r2 * ri, x = P.alpha * r2, y = P.sqrt_alpha * r, e = dipole_exp(-x);
  if (EXCL && x < T(4)) {
    dipole_lr_series<T>(P, x, e, B, C, dC);
    dB = -C;
  } else {
    // w = erfc(y) with kap as it is (short range), or w = erf(y) with kap negated (long range, exclusion variant)
    T w, kap;
    if (!EXCL) {
      w = erfc_from_exp(y, e);
      kap = P.kap;
    } else {
      w = dipole_erf(y);
      kap = -P.kap;
    }
    const T ke = kap * e, a = P.alpha;
    B = w * ri3 + ke * ri2;
    C = T(3) * w * ri5 + ke * (T(2) * a * ri2 + T(3) * ri2 * ri2);
    if (GRAD) {
      // B' = -r C;  C' = -15 w/r^6 - kap e (15/r^5 + 10 alpha/r^3 + 4 alpha^2/r)
      dB = -C;
      dC = T(-15) * w * ri5 * ri2 - ke * ri2 * (T(15) * ri2 * ri2 + T(10) * a * ri2 + T(4) * a * a);
    }
  }
  if (EXCL) {
    T fc = T(0), dfc = T(0);  // f_c and f_c'/r
    if (r < P.rx) {
      const T arg = T(kDipPi) * r / P.rx;
      T sn, cs;
      dipole_phase(arg, sn, cs);
      const T h = T(0.5) * (T(1) - cs);
      T hn1 = T(1);  // h^(n-1)
      for (int k = 1; k < P.deg; ++k) hn1 *= h;
      fc = T(1) - hn1 * h;
      if (GRAD) dfc = -T(P.deg) * hn1 * (T(0.5) * T(kDipPi) / P.rx) * sn * ri;
    }
    if (GRAD) {
      dB = -(dfc * B + fc * dB);
      dC = -(dfc * C + fc * dC);
    }
    B = -fc * B;
    C = -fc * C;
  }
}

// d(a^T T b)/dr without the prefactor, added to (gx, gy, gz)
template <typename T>
__device__ __forceinline__ void dipole_pair_grad(T rx, T ry, T rz, T C, T dB, T dC, T ax, T ay, T az, T bx, T by, T bz,
                                                 T& gx, T& gy, T& gz) {
  const T ar = ax * rx + ay * ry + az * rz, br = bx * rx + by * ry + bz * rz, ab = ax * bx + ay * by + az * bz;
  const T f = dB * ab - dC * ar * br;
  gx += f * rx - C * (br * ax + ar * bx);
  gy += f * ry - C * (br * ay + ar * by);
  gz += f * rz - C * (br * az + ar * bz);
}

}  // namespace mipme
