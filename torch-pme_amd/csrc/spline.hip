// Tabulated potentials: natural cubic splines on float64 knot tables (SplinePotential, reference potentials/spline.py;
// CubicSpline / CubicSplineReciprocal, lib/splines.py:4-121).
//
//   spline_eval_kernel        out[i] = S^(m)(x[i]), m = 0..3, of the plain spline (CubicSpline.forward and its derivatives:
//                             what the backward passes of the autograd node in splines.py are made of)
//   spline_recip_kernel       x < x0 ? Z(x) : R(1/x) and its first derivative in one pass (CubicSplineReciprocal.forward:
//                             a searchsorted, ten gathers and two where() over the list in the reference)
//   spline_kfilter_kernel     G(k) = prefactor * spline(|k|^2) [/ U^2(k)] on the rfft half grid; |k|^2 and 1 / U^2 from the index by
//                             kgrid_point of kgrid.h, as in kfilter.hip and combined.hip (KSpaceFilter.update /
//                             P3MKSpaceFilter.update with a spline kernel)
//
// One thread per argument, grid-stride.  The spline is evaluated in double precision whatever the argument's type; the result
// is stored in the argument's type.  A table of up to kLdsKnots knots is staged in LDS (3 arrays of doubles; 2048 knots are
// 48 KB, so three workgroups still share a CU's 160 KB); a longer one is read from global memory, where the binary search's
// first levels hit the same few cache lines in every lane.  The search runs ceil(log2 n) iterations for every lane -- no
// divergent exit -- and only ever reads knots 0..n-2; a NaN argument fails every comparison, lands in interval 0 and comes out as NaN.
#include <cmath>

#include "host.h"
#include "kgrid.h"

namespace mipme {

constexpr int kLdsKnots = 2048;
constexpr int kSplineBlock = 256;

struct SplineTab {
  const double* x;
  const double* y;
  const double* d2;
  int n;
  int iters;  // ceil(log2 n)
};

// the first interval of the 3-knot spline below the first knot of a reciprocal-axis spline (arguments below x0 only ever fall
// into it, or extrapolate it below zero)
struct ZeroCubic {
  double x0, x1, y0, y1, d0, d1;
};

// interval of v: searchsorted(x, v, right=True) - 1 clamped to [0, n-2], i.e. the last knot <= v among knots 0..n-2, else 0
__device__ __forceinline__ int spline_interval(const double* __restrict__ xk, int n, int iters, double v) {
  int lo = 0, len = n - 1;
  for (int it = 0; it < iters; ++it) {
    const int half = len >> 1;
    const bool up = xk[lo + half] <= v;  // (lo + half <= n - 2 throughout; false for NaN)
    lo = up ? lo + half : lo;
    len = up ? len - half : half;
  }
  return lo;
}

// m-th derivative of the cubic on [x0, x1] with values y0, y1 and second derivatives d0, d1 (one division: 1/h is shared; the
// double-precision divisions, not the table reads, are most of what a point costs)
template <int M>
__device__ __forceinline__ double cubic(double v, double x0, double x1, double y0, double y1, double d0, double d1) {
  const double h = x1 - x0;
  const double ih = 1.0 / h;
  const double a = (x1 - v) * ih, b = (v - x0) * ih;
  if constexpr (M == 0) {
    const double h26 = h * h / 6.0;
    return a * (y0 + (a * a - 1.0) * d0 * h26) + b * (y1 + (b * b - 1.0) * d1 * h26);
  } else if constexpr (M == 1) {
    return (y1 - y0) * ih + ((3.0 * b * b - 1.0) * d1 - (3.0 * a * a - 1.0) * d0) * (h / 6.0);
  } else if constexpr (M == 2) {
    return a * d0 + b * d1;
  } else {
    return (d1 - d0) * ih;
  }
}

// value and first derivative of the same cubic from one set of coefficients
__device__ __forceinline__ void cubic01(double v, double x0, double x1, double y0, double y1, double d0, double d1, double& val,
                                        double& der) {
  const double h = x1 - x0;
  const double ih = 1.0 / h;
  const double a = (x1 - v) * ih, b = (v - x0) * ih;
  const double h6 = h * (1.0 / 6.0);
  val = a * (y0 + (a * a - 1.0) * d0 * (h * h6)) + b * (y1 + (b * b - 1.0) * d1 * (h * h6));
  der = (y1 - y0) * ih + ((3.0 * b * b - 1.0) * d1 - (3.0 * a * a - 1.0) * d0) * h6;
}

template <int M>
__device__ __forceinline__ double spline_at(const SplineTab& t, const double* xk, const double* yk, const double* dk, double v) {
  const int i = spline_interval(xk, t.n, t.iters, v);
  const double r = cubic<M>(v, xk[i], xk[i + 1], yk[i], yk[i + 1], dk[i], dk[i + 1]);
  return v != v ? v : r;  // (the third derivative does not depend on v: a NaN argument still gives NaN)
}

// the knots in LDS (LDS = true: every thread of the block takes part, then a barrier) or where they are
template <bool LDS>
__device__ __forceinline__ void stage_table(const SplineTab& t, double* lds, const double*& xk, const double*& yk, const double*& dk) {
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < t.n; i += blockDim.x) {
      lds[i] = t.x[i];
      lds[t.n + i] = t.y[i];
      lds[2 * t.n + i] = t.d2[i];
    }
    __syncthreads();
    xk = lds;
    yk = lds + t.n;
    dk = lds + 2 * t.n;
  } else {
    xk = t.x;
    yk = t.y;
    dk = t.d2;
  }
}

template <typename T, int M, bool LDS>
__global__ __launch_bounds__(kSplineBlock) void spline_eval_kernel(SplineTab t, int64_t n_points, const T* __restrict__ x,
                                                                  T* __restrict__ out) {
  extern __shared__ double spline_lds[];
  const double *xk, *yk, *dk;
  stage_table<LDS>(t, spline_lds, xk, yk, dk);
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_points; i += stride)
    out[i] = T(spline_at<M>(t, xk, yk, dk, double(x[i])));
}

// value and first derivative of the reciprocal-axis composite at v
template <bool DERIV>
__device__ __forceinline__ void recip_at(const SplineTab& t, const ZeroCubic& z, const double* xk, const double* yk, const double* dk,
                                         double v, double& val, double& der) {
  if (v < z.x1) {
    if constexpr (DERIV)
      cubic01(v, z.x0, z.x1, z.y0, z.y1, z.d0, z.d1, val, der);
    else
      val = cubic<0>(v, z.x0, z.x1, z.y0, z.y1, z.d0, z.d1);
    return;
  }
  const double u = 1.0 / v;  // (NaN comes here: every value below is NaN then)
  const int i = spline_interval(xk, t.n, t.iters, u);
  const double x0 = xk[i], x1 = xk[i + 1], y0 = yk[i], y1 = yk[i + 1], d0 = dk[i], d1 = dk[i + 1];
  if constexpr (DERIV) {
    cubic01(u, x0, x1, y0, y1, d0, d1, val, der);
    der = -der * u * u;
  } else {
    val = cubic<0>(u, x0, x1, y0, y1, d0, d1);
  }
}

template <typename T, bool DERIV, bool LDS>
__global__ __launch_bounds__(kSplineBlock) void spline_recip_kernel(SplineTab t, ZeroCubic z, int64_t n_points,
                                                                   const T* __restrict__ x, T* __restrict__ out,
                                                                   T* __restrict__ dout) {
  extern __shared__ double spline_lds[];
  const double *xk, *yk, *dk;
  stage_table<LDS>(t, spline_lds, xk, yk, dk);
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_points; i += stride) {
    double val, der = 0.0;
    recip_at<DERIV>(t, z, xk, yk, dk, double(x[i]), val, der);
    out[i] = T(val);
    if constexpr (DERIV) dout[i] = T(der);
  }
}

// ---- G(k) from a spline in k^2
template <typename T, bool RECIP, bool LDS>
__global__ __launch_bounds__(kSplineBlock) void spline_kfilter_kernel(KGeom g, SplineTab t, ZeroCubic z, double prefactor,
                                                                     T* __restrict__ G) {
  extern __shared__ double spline_lds[];
  const double *xk, *yk, *dk;
  stage_table<LDS>(t, spline_lds, xk, yk, dk);
  const int64_t Mh = int64_t(g.nx) * g.ny * g.nzh;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < Mh; p += stride) {
    double inv;
    bool dead;
    const double k2 = kgrid_point(g, p, inv, dead);
    double v, unused = 0.0;
    if constexpr (RECIP)
      recip_at<false>(t, z, xk, yk, dk, k2, v, unused);
    else
      v = spline_at<0>(t, xk, yk, dk, k2);
    v *= prefactor;
    G[p] = T(dead ? 0.0 : v * inv);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int make_tab(const mipme_spline_t* sp, const char* who, SplineTab& t, ZeroCubic& z) {
  MIPME_REQUIRE(sp != nullptr, "%s: spline descriptor is NULL", who);
  MIPME_REQUIRE(sp->n >= 2, "%s: a spline needs at least 2 knots, got %d", who, int(sp->n));
  MIPME_REQUIRE(sp->x && sp->y && sp->d2y, "%s: NULL knot table", who);
  t.x = sp->x;
  t.y = sp->y;
  t.d2 = sp->d2y;
  t.n = sp->n;
  t.iters = 0;
  while ((int64_t(1) << t.iters) < int64_t(sp->n)) ++t.iters;
  z = ZeroCubic{sp->zero_x[0], sp->zero_x[1], sp->zero_y[0], sp->zero_y[1], sp->zero_d2y[0], sp->zero_d2y[1]};
  if (sp->reciprocal)
    MIPME_REQUIRE(sp->zero_x[1] > sp->zero_x[0], "%s: the spline below the first knot needs zero_x[1] > zero_x[0]", who);
  return MIPME_OK;
}

template <typename T>
static int spline_eval_impl(hipStream_t st, const SplineTab& t, int order, int64_t n, const void* x, void* out) {
  const T* xp = (const T*)x;
  T* op = (T*)out;
#define SPLINE_EVAL_CASE(M)                                                                                            \
  case M:                                                                                                              \
    if (t.n <= kLdsKnots)                                                                                              \
      spline_eval_kernel<T, M, true><<<stride_grid(n, kSplineBlock), kSplineBlock, size_t(3) * sizeof(double) * size_t(t.n), st>>>(t, n, xp, op); \
    else                                                                                                               \
      spline_eval_kernel<T, M, false><<<stride_grid(n, kSplineBlock), kSplineBlock, 0, st>>>(t, n, xp, op);                           \
    break;
  switch (order) {
    SPLINE_EVAL_CASE(0)
    SPLINE_EVAL_CASE(1)
    SPLINE_EVAL_CASE(2)
    SPLINE_EVAL_CASE(3)
  }
#undef SPLINE_EVAL_CASE
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int spline_recip_impl(hipStream_t st, const SplineTab& t, const ZeroCubic& z, int64_t n, const void* x, void* out, void* dout) {
  const T* xp = (const T*)x;
  T *op = (T*)out, *dp = (T*)dout;
  const size_t lds = size_t(3) * sizeof(double) * size_t(t.n);
  const unsigned grid = stride_grid(n, kSplineBlock);
  if (t.n <= kLdsKnots) {
    if (dp)
      spline_recip_kernel<T, true, true><<<grid, kSplineBlock, lds, st>>>(t, z, n, xp, op, dp);
    else
      spline_recip_kernel<T, false, true><<<grid, kSplineBlock, lds, st>>>(t, z, n, xp, op, dp);
  } else {
    if (dp)
      spline_recip_kernel<T, true, false><<<grid, kSplineBlock, 0, st>>>(t, z, n, xp, op, dp);
    else
      spline_recip_kernel<T, false, false><<<grid, kSplineBlock, 0, st>>>(t, z, n, xp, op, dp);
  }
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int spline_kfilter_impl(hipStream_t st, const mipme_mesh_t* m, const SplineTab& t, const ZeroCubic& z, bool recip,
                               double prefactor, void* G) {
  const KGeom g = make_kgeom(m);
  const int64_t Mh = int64_t(g.nx) * g.ny * g.nzh;
  const size_t lds = size_t(3) * sizeof(double) * size_t(t.n);
  const unsigned grid = stride_grid(Mh, kSplineBlock);
  T* Gp = (T*)G;
  if (t.n <= kLdsKnots) {
    if (recip)
      spline_kfilter_kernel<T, true, true><<<grid, kSplineBlock, lds, st>>>(g, t, z, prefactor, Gp);
    else
      spline_kfilter_kernel<T, false, true><<<grid, kSplineBlock, lds, st>>>(g, t, z, prefactor, Gp);
  } else {
    if (recip)
      spline_kfilter_kernel<T, true, false><<<grid, kSplineBlock, 0, st>>>(g, t, z, prefactor, Gp);
    else
      spline_kfilter_kernel<T, false, false><<<grid, kSplineBlock, 0, st>>>(g, t, z, prefactor, Gp);
  }
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int mipme_spline_eval(void* stream, int dtype, const mipme_spline_t* spline, int order, int64_t n_points, const void* x,
                      void* out) {
  SplineTab t;
  ZeroCubic z;
  const int rc = make_tab(spline, "mipme_spline_eval", t, z);
  if (rc) return rc;
  MIPME_REQUIRE(order >= 0 && order <= 3, "mipme_spline_eval: derivative order %d is outside 0..3 (higher ones are zero)", order);
  MIPME_REQUIRE(n_points >= 0, "mipme_spline_eval: invalid number of points");
  if (n_points == 0) return MIPME_OK;
  MIPME_REQUIRE(x && out, "mipme_spline_eval: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  DT_SWITCH(dtype, spline_eval_impl<float>(st, t, order, n_points, x, out), spline_eval_impl<double>(st, t, order, n_points, x, out));
}

int mipme_spline_eval_reciprocal(void* stream, int dtype, const mipme_spline_t* spline, int64_t n_points, const void* x,
                                 void* out, void* dout) {
  SplineTab t;
  ZeroCubic z;
  const int rc = make_tab(spline, "mipme_spline_eval_reciprocal", t, z);
  if (rc) return rc;
  MIPME_REQUIRE(spline->reciprocal, "mipme_spline_eval_reciprocal: the descriptor is not a reciprocal-axis spline");
  MIPME_REQUIRE(n_points >= 0, "mipme_spline_eval_reciprocal: invalid number of points");
  if (n_points == 0) return MIPME_OK;
  MIPME_REQUIRE(x && out, "mipme_spline_eval_reciprocal: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  DT_SWITCH(dtype, spline_recip_impl<float>(st, t, z, n_points, x, out, dout), spline_recip_impl<double>(st, t, z, n_points, x, out, dout));
}

int mipme_spline_kfilter_build(void* stream, int dtype, const mipme_mesh_t* mesh, const mipme_spline_t* spline, void* G) {
  SplineTab t;
  ZeroCubic z;
  const int rc = make_tab(spline, "mipme_spline_kfilter_build", t, z);
  if (rc) return rc;
  if (const int mrc = validate_mesh(mesh)) return mrc;
  MIPME_REQUIRE(G != nullptr, "mipme_spline_kfilter_build: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  DT_SWITCH(dtype, spline_kfilter_impl<float>(st, mesh, t, z, spline->reciprocal != 0, spline->prefactor, G),
            spline_kfilter_impl<double>(st, mesh, t, z, spline->reciprocal != 0, spline->prefactor, G));
}

}  // extern "C"
