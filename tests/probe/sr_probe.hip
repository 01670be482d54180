// Test-only probe (tests/test_gpu_sr_pointwise.py): the device functions of srpot.h / rows_body.h one input per thread, and the
// fp64 / packed fp32 row bodies as kernels of their own.  Nothing here is part of libmipme.so; the functions under test are the
// library's headers, included as they stand.  Every export returns 0 or a HIP error code (sr_probe_last_error: argument errors).
#include <cstdarg>
#include <cstdio>

#include "rows_body.h"

namespace mipme {
static thread_local char g_probe_error[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_probe_error, sizeof(g_probe_error), fmt, ap);
  va_end(ap);
}
void note_cosched_kernel(const char*) {}
}  // namespace mipme

using namespace mipme;

namespace {

constexpr int kThreads = 256;
inline unsigned blocks_for(int64_t n) { return unsigned((n + kThreads - 1) / kThreads); }
__device__ __forceinline__ int64_t global_index() { return int64_t(blockIdx.x) * kThreads + threadIdx.x; }

template <typename T>
__global__ __launch_bounds__(kThreads) void sr_eval_kernel(SRPot s, int64_t n, const T* __restrict__ d, T* __restrict__ v,
                                                           T* __restrict__ dv) {
  const int64_t i = global_index();
  if (i >= n) return;
  T a, b;
  sr_eval<T, true>(s, d[i], a, b);
  v[i] = a;
  dv[i] = b;
}

// the constants reach the function as the row bodies hand them on: FastRS by value, cast to T
template <int P, typename T>
__global__ __launch_bounds__(kThreads) void fast_rs_kernel(FastRS cf, int64_t n, const T* __restrict__ d2, T* __restrict__ v,
                                                           T* __restrict__ dvd) {
  const int64_t i = global_index();
  if (i >= n) return;
  T a, b;
  fast_rs_eval<P, true, T>(T(cf.inv_2s2), T(cf.c1), T(cf.pref), d2[i], a, b, cf.cheb);
  v[i] = a;
  dvd[i] = b;
}

// two inputs per thread: elements 2 i and 2 i + 1 in slots (x, y), or (y, x) with swap
template <int P>
__global__ __launch_bounds__(kThreads) void fast_rs_pk_kernel(FastRS cf, int64_t n, int swap, const float* __restrict__ d2,
                                                              float* __restrict__ v, float* __restrict__ dvd) {
  const int64_t i = global_index();
  if (2 * i >= n) return;
  const int64_t ia = 2 * i, ib = 2 * i + 1 < n ? 2 * i + 1 : 2 * i;
  const f2v in = swap ? f2v{d2[ib], d2[ia]} : f2v{d2[ia], d2[ib]};
  f2v a, b;
  fast_rs_eval_pk<P>(float(cf.inv_2s2), float(cf.c1), float(cf.pref), in, a, b);
  v[ia] = swap ? a.y : a.x;
  dvd[ia] = swap ? b.y : b.x;
  if (ib != ia) {
    v[ib] = swap ? a.x : a.y;
    dvd[ib] = swap ? b.x : b.y;
  }
}

// which: 0 exp_neg_fast(x), 1 rcp_newton(x), 2 rsqrt_newton(x), 3 erfc_from_exp(y, exp_neg_fast(y y)) with the coefficients of FastRS
__global__ __launch_bounds__(kThreads) void scalar_f64_kernel(int which, FastRS cf, int64_t n, const double* __restrict__ x,
                                                              double* __restrict__ out) {
  const int64_t i = global_index();
  if (i >= n) return;
  const double t = x[i];
  double r;
  if (which == 0)
    r = exp_neg_fast(t);
  else if (which == 1)
    r = rcp_newton(t);
  else if (which == 2)
    r = rsqrt_newton(t);
  else
    r = erfc_from_exp(t, exp_neg_fast(t * t), cf.cheb);
  out[i] = r;
}

// the tables staged in LDS exactly as sr_rows_f64_body does; two inputs per thread (exp_neg_table2 works on pairs)
// which: 0 exp_neg_table2(x), 1 erfc_from_table(y, exp_neg_table2(y y))
__global__ __launch_bounds__(kThreads) void table_f64_kernel(int which, int64_t n, const double* __restrict__ x,
                                                             double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double etab[kErfcxLdsDoubles + kExp2Tab];
  erfcx_table_to_lds(etab, threadIdx.x, kThreads);
  exp2_table_to_lds(etab + kErfcxLdsDoubles, threadIdx.x, kThreads);
  __syncthreads();
  const int64_t i = global_index();
  if (2 * i >= n) return;
  const int64_t ia = 2 * i, ib = 2 * i + 1 < n ? 2 * i + 1 : 2 * i;
  const double in[2] = {x[ia], x[ib]};
  const double arg[2] = {which == 0 ? in[0] : in[0] * in[0], which == 0 ? in[1] : in[1] * in[1]};
  double e[2];
  exp_neg_table2(arg, e, etab + kErfcxLdsDoubles);
  if (which == 1) {
    e[0] = erfc_from_table(in[0], e[0], etab);
    e[1] = erfc_from_table(in[1], e[1], etab);
  }
  out[ia] = e[0];
  if (ib != ia) out[ib] = e[1];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void lower_gamma_kernel(int p, int64_t n, const T* __restrict__ x, T* __restrict__ out) {
  const int64_t i = global_index();
  if (i >= n) return;
  out[i] = lower_gamma_series<T>(p, x[i]);
}

template <int PFAST>
__global__ __launch_bounds__(256) void rows_f64_kernel(FusedRowsArgs<double> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_rows[];
  sr_rows_f64_body<256, false, PFAST>(a, blockIdx.x, smem_rows);
}
template <int PFAST>
__global__ __launch_bounds__(256) void rows_pk_kernel(FusedRowsArgs<float> a) {
  __shared__ AtomRecord<float> shift_tab[kShiftTableSize];
  sr_rows_pk_body<PFAST, 256>(a, blockIdx.x, shift_tab);
}

int finish() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) set_error("launch failed: %s", hipGetErrorString(e));
  return int(e);
}

template <typename T>
int rows_args(FusedRowsArgs<T>& args, int64_t N, const void* row_ptr, const void* ent32, const void* pos, const void* cell,
              const void* q, const void* rec, const mipme_potential_t* pot, int full_list, void* out, void* force, int want_p) {
  SRPot s;
  if (make_srpot(pot, s)) return -1;
  MIPME_REQUIRE(fast_rs_exponent(s) == want_p, "the potential is not the range-separated 1/r^%d", want_p);
  MIPME_REQUIRE(N > 0 && N <= kCompactMaxAtoms && row_ptr && ent32 && pos && cell && q && rec && out && force,
                "invalid arguments to the row probe");
  const int lo = 0, hi = full_list ? 0 : 1;  // as mipme_sr_rows_fused, transpose = 0
  args = make_fused_rows_args<T>(s, make_fast_rs(s), N, row_ptr, ent32, nullptr, nullptr, pos, rec, cell, q, nullptr, lo, hi,
                                 full_list, 0, out, force, nullptr, nullptr, kShiftTable32);
  return 0;
}

}  // namespace

extern "C" {

const char* sr_probe_last_error() { return g_probe_error; }

int sr_probe_sr_eval(void* stream, int dtype, const mipme_potential_t* pot, int64_t n, const void* d, void* v, void* dv) {
  SRPot s;
  if (make_srpot(pot, s)) return -1;
  MIPME_REQUIRE(n > 0 && d && v && dv, "invalid arguments to sr_probe_sr_eval");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIPME_F32)
    sr_eval_kernel<float><<<blocks_for(n), kThreads, 0, st>>>(s, n, (const float*)d, (float*)v, (float*)dv);
  else
    sr_eval_kernel<double><<<blocks_for(n), kThreads, 0, st>>>(s, n, (const double*)d, (double*)v, (double*)dv);
  return finish();
}

int sr_probe_fast_rs(void* stream, int dtype, const mipme_potential_t* pot, int64_t n, const void* d2, void* v, void* dvd) {
  SRPot s;
  if (make_srpot(pot, s)) return -1;
  const int P = fast_rs_exponent(s);
  MIPME_REQUIRE(P == 1 || P == 6, "no fast form for this potential");
  MIPME_REQUIRE(n > 0 && d2 && v && dvd, "invalid arguments to sr_probe_fast_rs");
  const FastRS cf = make_fast_rs(s);
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = blocks_for(n);
  if (dtype == MIPME_F32) {
    if (P == 1)
      fast_rs_kernel<1, float><<<g, kThreads, 0, st>>>(cf, n, (const float*)d2, (float*)v, (float*)dvd);
    else
      fast_rs_kernel<6, float><<<g, kThreads, 0, st>>>(cf, n, (const float*)d2, (float*)v, (float*)dvd);
  } else {
    if (P == 1)
      fast_rs_kernel<1, double><<<g, kThreads, 0, st>>>(cf, n, (const double*)d2, (double*)v, (double*)dvd);
    else
      fast_rs_kernel<6, double><<<g, kThreads, 0, st>>>(cf, n, (const double*)d2, (double*)v, (double*)dvd);
  }
  return finish();
}

int sr_probe_fast_rs_pk(void* stream, const mipme_potential_t* pot, int64_t n, int swap, const void* d2, void* v, void* dvd) {
  SRPot s;
  if (make_srpot(pot, s)) return -1;
  const int P = fast_rs_exponent(s);
  MIPME_REQUIRE(P == 1 || P == 6, "no fast form for this potential");
  MIPME_REQUIRE(n > 0 && d2 && v && dvd, "invalid arguments to sr_probe_fast_rs_pk");
  const FastRS cf = make_fast_rs(s);
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = blocks_for((n + 1) / 2);
  if (P == 1)
    fast_rs_pk_kernel<1><<<g, kThreads, 0, st>>>(cf, n, swap, (const float*)d2, (float*)v, (float*)dvd);
  else
    fast_rs_pk_kernel<6><<<g, kThreads, 0, st>>>(cf, n, swap, (const float*)d2, (float*)v, (float*)dvd);
  return finish();
}

// which: 0 exp_neg_fast, 1 rcp_newton, 2 rsqrt_newton, 3 erfc_from_exp (double), 4 exp_neg_table2, 5 erfc_from_table
int sr_probe_scalar_f64(void* stream, int which, int64_t n, const void* x, void* out) {
  MIPME_REQUIRE(which >= 0 && which <= 5 && n > 0 && x && out, "invalid arguments to sr_probe_scalar_f64");
  hipStream_t st = (hipStream_t)stream;
  if (which <= 3) {
    SRPot s{1, 1, 1.0, 0.5, 0.0, 1};
    scalar_f64_kernel<<<blocks_for(n), kThreads, 0, st>>>(which, make_fast_rs(s), n, (const double*)x, (double*)out);
  } else {
    table_f64_kernel<<<blocks_for((n + 1) / 2), kThreads, 0, st>>>(which - 4, n, (const double*)x, (double*)out);
  }
  return finish();
}

int sr_probe_lower_gamma(void* stream, int dtype, int p, int64_t n, const void* x, void* out) {
  MIPME_REQUIRE(p >= 1 && p <= 6 && n > 0 && x && out, "invalid arguments to sr_probe_lower_gamma");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIPME_F32)
    lower_gamma_kernel<float><<<blocks_for(n), kThreads, 0, st>>>(p, n, (const float*)x, (float*)out);
  else
    lower_gamma_kernel<double><<<blocks_for(n), kThreads, 0, st>>>(p, n, (const double*)x, (double*)out);
  return finish();
}

// sr_rows_f64_body<256, false, P> / sr_rows_pk_body<P, 256> on their own: 4-byte entries (format 2), potential + force sums,
// arguments built from the inputs of mipme_sr_rows_fused.  rec: the (N, 4) records (x, y, z, q), packed by the caller.
int sr_probe_rows_f64(void* stream, int P, int64_t N, const void* row_ptr, const void* ent32, const void* pos, const void* cell,
                      const void* q, const void* rec, const mipme_potential_t* pot, int full_list, void* out, void* force) {
  MIPME_REQUIRE(P == 1 || P == 6, "P must be 1 or 6");
  FusedRowsArgs<double> args;
  if (rows_args<double>(args, N, row_ptr, ent32, pos, cell, q, rec, pot, full_list, out, force, P)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = unsigned((N + kRowsPerBlock - 1) / kRowsPerBlock);
  if (P == 1)
    rows_f64_kernel<1><<<g, 256, kRowsF64LdsBytes, st>>>(args);
  else
    rows_f64_kernel<6><<<g, 256, kRowsF64LdsBytes, st>>>(args);
  return finish();
}

int sr_probe_rows_pk(void* stream, int P, int64_t N, const void* row_ptr, const void* ent32, const void* pos, const void* cell,
                     const void* q, const void* rec, const mipme_potential_t* pot, int full_list, void* out, void* force) {
  MIPME_REQUIRE(P == 1 || P == 6, "P must be 1 or 6");
  FusedRowsArgs<float> args;
  if (rows_args<float>(args, N, row_ptr, ent32, pos, cell, q, rec, pot, full_list, out, force, P)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = unsigned((N + kRowsPerBlock - 1) / kRowsPerBlock);
  if (P == 1)
    rows_pk_kernel<1><<<g, 256, 0, st>>>(args);
  else
    rows_pk_kernel<6><<<g, 256, 0, st>>>(args);
  return finish();
}

}  // extern "C"
