// Weighted sums of 1/r^p potentials (CombinedPotential, reference potentials/combined.py) where the fused kernels do not apply:
//
//   combined_sr_kernel        the n-th derivative w.r.t. d of every term's pair function in ONE pass over the distances, written
//                             per term (n_terms, n_points) or contracted with device-resident weights (n_points,).  What the
//                             autograd node of combined.py is made of: its backward is the same kernel one order up
//   combined_kfilter_kernel   G_t(k) of every term on the rfft half grid, (n_terms, nx, ny, nz/2+1): |k|^2 and the P3M factor
//                             1 / U^2 once per point (kgrid_point of kgrid.h, as in kfilter.hip and spline.hip),
//                             lr_kernel_dev of kpot.h once per term
//
// Pair function of a term, x = d^2 / 2 sigma^2:   v = pref Q(p/2, x) / d^p  (range separated)   or   v = pref / d^p  (direct).
// With A = 2 x^(p/2) e^-x / Gamma(p/2) = 2 x dens(x)  (dQ/dx = -dens, dA/dx = A (p / 2x - 1))  and  (p)_n = p (p+1) ... (p+n-1):
//
//   v^(n) = (-1)^n pref d^-(p+n) [ R_n(x) A + (p)_n Q ],      R_0 = 0,   R_n+1 = (n + 2x) R_n - 2x R_n' + (p)_n
//
// so R_1 = 1, R_2 = 2x + p + 1, R_3 = 4x^2 + 2x(p+1) + (p+1)(p+2): a polynomial of degree n-1 whose coefficients depend on p
// alone.  The host forms them (combined_coefficients), the kernel evaluates them by Horner's rule.  The direct form is the same
// line with A = 0, Q = 1.  Q and dens come from upper_gamma<T> of srpot.h (erfc and a finite sum for odd p, e^-x times a finite
// sum for even p: one piece, no cancellation at short distances); the floor on d is that header's.
//
// One thread per distance, grid-stride; the terms travel in the kernel arguments (scalar registers).  No atomics, no scratch.
#include <cmath>

#include "host.h"
#include "kgrid.h"
#include "kpot.h"
#include "srpot.h"

namespace mipme {

constexpr int kCombBlock = 256;

struct CombTerm {
  int p;
  double inv_2s2;                          // 1 / (2 sigma^2); unused by a direct term
  double ca;                               // (-1)^n pref: multiplies R_n(x) A
  double cq;                               // (-1)^n pref (p)_n: multiplies Q
  double r[MIPME_COMBINED_MAX_ORDER];      // R_n = sum_k r[k] x^k, k < n
};

struct CombTerms {
  int n_terms;
  int order;
  CombTerm t[MIPME_COMBINED_MAX_TERMS];
};

// coefficients of R_order for exponent p (r[k] of x^k; the entries from `order` on are zero)
static void combined_coefficients(int p, int order, double* r) {
  double cur[MIPME_COMBINED_MAX_ORDER + 1] = {0.0};
  double rising = 1.0;  // (p)_n
  for (int n = 0; n < order; ++n) {
    // R_n+1 = (n + 2x) R_n - 2x R_n' + (p)_n: coefficient of x^k is (n - 2k) c_k + 2 c_k-1
    double next[MIPME_COMBINED_MAX_ORDER + 1] = {0.0};
    for (int k = 0; k <= n; ++k) next[k] = double(n - 2 * k) * cur[k] + (k > 0 ? 2.0 * cur[k - 1] : 0.0);
    next[0] += rising;
    for (int k = 0; k <= n; ++k) cur[k] = next[k];
    rising *= double(p + n);
  }
  for (int k = 0; k < MIPME_COMBINED_MAX_ORDER; ++k) r[k] = cur[k];
}

static double rising_factorial(int p, int n) {
  double v = 1.0;
  for (int i = 0; i < n; ++i) v *= double(p + i);
  return v;
}

// x, Q(p/2, x) and A = 2 x dens for d (floored) of type T.  float: x is formed in double and split into the float the finite sums
// see and a remainder dx, and both results -- each proportional to e^-x -- are scaled by 1 - dx: the rounding of x, relative
// 2^-24, would otherwise appear x-fold in e^-x (2e-6 at d = 8 sigma).
template <typename T>
__device__ __forceinline__ void comb_gamma(int p, double inv_2s2, T dc, T& x, T& Q, T& A) {
  T dens;
  if constexpr (sizeof(T) == 4) {
    const double xd = double(dc) * double(dc) * inv_2s2;
    x = float(xd);
    const float corr = 1.0f - float(xd - double(x));
    upper_gamma<T>(p, x, Q, dens);
    Q *= corr;
    dens *= corr;
  } else {
    x = dc * dc * inv_2s2;
    upper_gamma<T>(p, x, Q, dens);
  }
  A = T(2) * x * dens;
}

// v_t^(order)(d) of term t
template <typename T, bool SMEARED>
__device__ __forceinline__ T comb_term(const CombTerm& t, int order, T dc, T inv) {
  const T invp = powi(inv, t.p + order);
  if constexpr (!SMEARED) {
    return T(t.cq) * invp;
  } else {
    T x, Q, A;
    comb_gamma<T>(t.p, t.inv_2s2, dc, x, Q, A);
    T R = T(0);
    for (int k = order - 1; k >= 0; --k) R = R * x + T(t.r[k]);
    return invp * (T(t.ca) * R * A + T(t.cq) * Q);
  }
}

template <typename T, bool SMEARED, bool WEIGHTED>
__global__ __launch_bounds__(kCombBlock) void combined_sr_kernel(CombTerms c, int64_t n_points, const T* __restrict__ d,
                                                                const T* __restrict__ weights, T* __restrict__ out) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_points; i += stride) {
    const T di = d[i];
    const T dc = di < T(1e-15) ? T(1e-15) : di;  // (this way round a NaN distance stays NaN)
    const T inv = T(1) / dc;
    T sum = T(0);
    for (int t = 0; t < c.n_terms; ++t) {
      const T v = comb_term<T, SMEARED>(c.t[t], c.order, dc, inv);
      if constexpr (WEIGHTED)
        sum += weights[t] * v;
      else
        out[int64_t(t) * n_points + i] = v;
    }
    if constexpr (WEIGHTED) out[i] = sum;
  }
}

// ---- G_t(k): one lr_kernel_dev per term at every point of the half grid
struct CombKPots {
  int n_terms;
  KPot kp[MIPME_COMBINED_MAX_TERMS];
};

template <typename T>
__global__ __launch_bounds__(kCombBlock) void combined_kfilter_kernel(KGeom g, CombKPots c, T* __restrict__ G) {
  const int64_t Mh = int64_t(g.nx) * g.ny * g.nzh;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t pt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; pt < Mh; pt += stride) {
    double inv;
    bool dead;
    const double k2 = kgrid_point(g, pt, inv, dead);
    for (int t = 0; t < c.n_terms; ++t) {
      double v, dv;
      lr_kernel_dev(c.kp[t], k2, v, dv);
      G[int64_t(t) * Mh + pt] = T(dead ? 0.0 : v * inv);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int exponent_of(const mipme_potential_t& t) { return t.kind == MIPME_COULOMB ? 1 : t.exponent; }

// what both entry points refuse; *smeared: whether the combination is range separated (set by its first term)
static int check_combined(const mipme_combined_t* comb, const char* who, bool need_smearing, bool* smeared) {
  MIPME_REQUIRE(comb != nullptr, "%s: combined descriptor is NULL", who);
  MIPME_REQUIRE(comb->n_terms >= 1 && comb->n_terms <= MIPME_COMBINED_MAX_TERMS,
                "%s: n_terms is %d but a combination holds 1 to %d terms (MIPME_COMBINED_MAX_TERMS)", who, int(comb->n_terms),
                MIPME_COMBINED_MAX_TERMS);
  *smeared = need_smearing || comb->terms[0].smearing > 0;
  for (int t = 0; t < comb->n_terms; ++t) {
    const int p = exponent_of(comb->terms[t]);
    MIPME_REQUIRE(p >= 1 && p <= 6, "%s: term %d: Unsupported exponent: %d", who, t, p);
    if (*smeared)
      MIPME_REQUIRE(comb->terms[t].smearing > 0,
                    "%s: term %d of a range-separated combination: `smearing` is %g but must be positive", who, t,
                    comb->terms[t].smearing);
    else
      MIPME_REQUIRE(!(comb->terms[t].smearing > 0),
                    "%s: term %d has a `smearing` in a combination of direct potentials (term 0 has none)", who, t);
  }
  return MIPME_OK;
}

template <typename T>
static int combined_sr_impl(hipStream_t st, const CombTerms& c, bool smeared, int64_t n, const void* d, const void* w, void* out) {
  const T *dp = (const T*)d, *wp = (const T*)w;
  T* op = (T*)out;
  const unsigned grid = stride_grid(n, kCombBlock);
  if (smeared) {
    if (wp)
      combined_sr_kernel<T, true, true><<<grid, kCombBlock, 0, st>>>(c, n, dp, wp, op);
    else
      combined_sr_kernel<T, true, false><<<grid, kCombBlock, 0, st>>>(c, n, dp, wp, op);
  } else {
    if (wp)
      combined_sr_kernel<T, false, true><<<grid, kCombBlock, 0, st>>>(c, n, dp, wp, op);
    else
      combined_sr_kernel<T, false, false><<<grid, kCombBlock, 0, st>>>(c, n, dp, wp, op);
  }
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int combined_kfilter_impl(hipStream_t st, const mipme_mesh_t* m, const CombKPots& c, void* G) {
  const KGeom g = make_kgeom(m);
  const int64_t Mh = int64_t(g.nx) * g.ny * g.nzh;
  combined_kfilter_kernel<T><<<stride_grid(Mh, kCombBlock), kCombBlock, 0, st>>>(g, c, (T*)G);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int mipme_combined_sr_eval(void* stream, int dtype, const mipme_combined_t* comb, int order, double* coeff, int64_t n_points,
                           const void* d, const void* weights, void* out) {
  bool smeared = false;
  const int rc = check_combined(comb, "mipme_combined_sr_eval", false, &smeared);
  if (rc) return rc;
  MIPME_REQUIRE(order >= 0 && order <= MIPME_COMBINED_MAX_ORDER,
                "mipme_combined_sr_eval: derivative order %d is outside 0..%d (MIPME_COMBINED_MAX_ORDER)", order,
                MIPME_COMBINED_MAX_ORDER);
  MIPME_REQUIRE(n_points >= 0, "mipme_combined_sr_eval: invalid number of points");
  CombTerms c;
  c.n_terms = comb->n_terms;
  c.order = order;
  const double sign = (order & 1) ? -1.0 : 1.0;
  for (int t = 0; t < comb->n_terms; ++t) {
    const mipme_potential_t& pt = comb->terms[t];
    CombTerm& ct = c.t[t];
    ct.p = exponent_of(pt);
    ct.inv_2s2 = smeared ? 0.5 / (pt.smearing * pt.smearing) : 0.0;
    ct.ca = sign * pt.prefactor;
    ct.cq = sign * pt.prefactor * rising_factorial(ct.p, order);
    combined_coefficients(ct.p, order, ct.r);
    if (coeff)
      for (int k = 0; k < MIPME_COMBINED_MAX_ORDER; ++k) coeff[t * MIPME_COMBINED_MAX_ORDER + k] = ct.r[k];
  }
  if (n_points == 0) return MIPME_OK;
  MIPME_REQUIRE(d && out, "mipme_combined_sr_eval: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  DT_SWITCH(dtype, combined_sr_impl<float>(st, c, smeared, n_points, d, weights, out),
            combined_sr_impl<double>(st, c, smeared, n_points, d, weights, out));
}

int mipme_combined_kfilter_build(void* stream, int dtype, const mipme_mesh_t* mesh, const mipme_combined_t* comb, void* out) {
  bool smeared = true;
  int rc = check_combined(comb, "mipme_combined_kfilter_build", true, &smeared);
  if (rc) return rc;
  if ((rc = validate_mesh(mesh))) return rc;
  MIPME_REQUIRE(out != nullptr, "mipme_combined_kfilter_build: NULL pointer");
  CombKPots c;
  c.n_terms = comb->n_terms;
  for (int t = 0; t < comb->n_terms; ++t) {
    rc = make_kpot(&comb->terms[t], c.kp[t]);
    if (rc) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  DT_SWITCH(dtype, combined_kfilter_impl<float>(st, mesh, c, out), combined_kfilter_impl<double>(st, mesh, c, out));
}

}  // extern "C"
