// Point dipoles: CalculatorDipole / PotentialDipole (reference calculators/calculator_dipole.py,
// potentials/potential_dipole.py).  Dipoles mu (N,3); the output "potential" V (N,3), energy sum_i mu_i . V_i.
//
// Real space, thread per pair p = (i, j) with r = neighbor_vectors[p], device-scope atomics into (N,3) (the reference hands a
// fresh list to every call, so a row-sorted list would not pay -- the reasoning of EwaldCalculator's atomic pair path):
//   T(r) = prefactor (B(r) I - C(r) r r^T),   V_i += T mu_j / 2  (half list: also V_j += T mu_i / 2)
//   direct        B = 1/r^3,                              C = 3/r^5
//   short range   B = erfc(y)/r^3 + kap e/r^2,            C = 3 erfc(y)/r^5 + kap (2 alpha + 3/r^2) e/r^2
//   long range    B = erf(y)/r^3 - kap e/r^2,             C = 3 erf(y)/r^5 - kap (2 alpha + 3/r^2) e/r^2
//   exclusion     -f_c(r) T_lr(r)                         (T_lr from a power series for alpha r^2 < 4: dipole_lr_series)
// with alpha = 1/(2 sigma^2), y = sqrt(alpha) r, e = exp(-alpha r^2), kap = 2 sqrt(alpha/pi).  The short-range form is
// evaluated directly (the reference's from_dist - lr_from_dist cancels in fp32).  B' = -r C for every radial form.
//   dL/dr_p = prefactor/2 [ (B'/r)(a.b) r - (C'/r)(a.r)(b.r) r - C ((b.r) a + (a.r) b) ]  for a = g_i, b = mu_j (+ g_j, mu_i)
//
// Reciprocal space (the 1/V factor, self / background terms and the cell dependence of k stay with the caller):
//   structure      S_c(k) = sum_j (mu_j.k) cos(k r_j),  S_s likewise with sin                32 lanes per k
//   field          E_i = sum_k G(k) k [cos(k r_i) S_c + sin(k r_i) S_s]                    block per (atom, k slice)
//   grad positions dL/dr_i = sum_k G k [ (g_i.k)(-s S_c + c S_s) + (mu_i.k)(-s T_c + c T_s) ]   block per (atom, k slice)
//   grad kvectors  dL/dk = 2 dG k (T_c S_c + T_s S_s)
//                         + G sum_i [ g_i (c S_c + s S_s) + mu_i (c T_c + s T_s) + r_i ((g_i.k)(-s S_c + c S_s)
//                                                                                    + (mu_i.k)(-s T_c + c T_s)) ]   32 lanes per k
// with T the structure factors of the upstream gradient g.  With few atoms (the reference's own cases: N = 3..8 against
// K ~ 10^6) a block per atom would put a handful of workgroups on the device, so the per-atom kernels also split K into
// slices, write partial sums and reduce them in a second pass in a fixed order (deterministic).  k-vectors whose G and
// dG/dk^2 are exactly zero in the working dtype contribute nothing and are skipped (most of them in fp32).
#include "common.h"
#include "dipole_device.h"
#include "srpot.h"

namespace mipme {

template <typename I>
__device__ __forceinline__ void dipole_pair(const I* __restrict__ pairs, int64_t p, int64_t& i, int64_t& j) {
  i = int64_t(pairs[2 * p]);
  j = int64_t(pairs[2 * p + 1]);
}

// V_i += T mu_j / 2 (and V_j += T mu_i / 2 for a half list).  Also the dipole gradient: the same sum applied to g.
template <typename T, typename I, bool EXCL>
__global__ __launch_bounds__(256) void dipole_rspace_kernel(DipPot<T> P, int64_t n_pairs, bool full,
                                                           const I* __restrict__ pairs, const T* __restrict__ vec,
                                                           const T* __restrict__ mu, T* __restrict__ out) {
  for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < n_pairs; p += int64_t(gridDim.x) * blockDim.x) {
    int64_t i, j;
    dipole_pair<I>(pairs, p, i, j);
    const T rx = vec[3 * p], ry = vec[3 * p + 1], rz = vec[3 * p + 2];
    const T r2 = rx * rx + ry * ry + rz * rz;
    const T ri = T(1) / fsqrt(r2);
    T B, C, dB, dC;
    dipole_bc<T, false, EXCL>(P, r2, ri, B, C, dB, dC);
    const T hb = T(0.5) * P.pref * B, hc = T(0.5) * P.pref * C;
    {
      const T mx = mu[3 * j], my = mu[3 * j + 1], mz = mu[3 * j + 2];
      const T cr = hc * (mx * rx + my * ry + mz * rz);
      atomic_add(out + 3 * i, hb * mx - cr * rx);
      atomic_add(out + 3 * i + 1, hb * my - cr * ry);
      atomic_add(out + 3 * i + 2, hb * mz - cr * rz);
    }
    if (!full) {
      const T mx = mu[3 * i], my = mu[3 * i + 1], mz = mu[3 * i + 2];
      const T cr = hc * (mx * rx + my * ry + mz * rz);
      atomic_add(out + 3 * j, hb * mx - cr * rx);
      atomic_add(out + 3 * j + 1, hb * my - cr * ry);
      atomic_add(out + 3 * j + 2, hb * mz - cr * rz);
    }
  }
}

// dL/d neighbor_vectors for L = sum_i g_i . V_i
template <typename T, typename I, bool EXCL>
__global__ __launch_bounds__(256) void dipole_rspace_grad_vectors_kernel(DipPot<T> P, int64_t n_pairs, bool full,
                                                                        const I* __restrict__ pairs,
                                                                        const T* __restrict__ vec,
                                                                        const T* __restrict__ mu,
                                                                        const T* __restrict__ g,
                                                                        T* __restrict__ grad_vec) {
  for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < n_pairs; p += int64_t(gridDim.x) * blockDim.x) {
    int64_t i, j;
    dipole_pair<I>(pairs, p, i, j);
    const T rx = vec[3 * p], ry = vec[3 * p + 1], rz = vec[3 * p + 2];
    const T r2 = rx * rx + ry * ry + rz * rz;
    const T ri = T(1) / fsqrt(r2);
    T B, C, dB, dC;
    dipole_bc<T, true, EXCL>(P, r2, ri, B, C, dB, dC);
    T gx = T(0), gy = T(0), gz = T(0);
    dipole_pair_grad<T>(rx, ry, rz, C, dB, dC, g[3 * i], g[3 * i + 1], g[3 * i + 2], mu[3 * j], mu[3 * j + 1],
                        mu[3 * j + 2], gx, gy, gz);
    if (!full)
      dipole_pair_grad<T>(rx, ry, rz, C, dB, dC, g[3 * j], g[3 * j + 1], g[3 * j + 2], mu[3 * i], mu[3 * i + 1],
                          mu[3 * i + 2], gx, gy, gz);
    const T h = T(0.5) * P.pref;
    grad_vec[3 * p] = h * gx;
    grad_vec[3 * p + 1] = h * gy;
    grad_vec[3 * p + 2] = h * gz;
  }
}

// ---- reciprocal space ------------------------------------------------------------------------------------------------
static constexpr int kDipTile = 256;     // atoms staged per LDS tile
static constexpr int kDipKPerBlock = 8;  // k-vectors per block of the per-k kernels, 32 lanes each
static constexpr int kDipLanes = 256 / kDipKPerBlock;
static_assert(kDipLanes == 32, "the per-k reductions add 32 lanes");

template <typename T>
__device__ __forceinline__ bool dipole_k_live(const T* __restrict__ G, const T* __restrict__ dG, int64_t k) {
  return G == nullptr || G[k] != T(0) || (dG != nullptr && dG[k] != T(0));
}

template <typename T>
__device__ __forceinline__ T dipole_sum32(T v) {
#pragma unroll
  for (int off = kDipLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kDipLanes);
  return v;
}

// S_c(k) = sum_j (w_j . k) cos(k r_j), S_s(k) likewise; w = dipoles or the upstream gradient.  The atom lanes of a k-vector
// walk every 32nd atom of the LDS tile, the 32 partial sums are added with a shuffle tree (fixed order).
template <typename T>
__global__ __launch_bounds__(256) void dipole_structure_kernel(int64_t N, int64_t K, const T* __restrict__ pos,
                                                              const T* __restrict__ w, const T* __restrict__ kvec,
                                                              const T* __restrict__ G, const T* __restrict__ dG,
                                                              T* __restrict__ out_c, T* __restrict__ out_s) {
  __shared__ T sp[kDipTile * 3];
  __shared__ T sw[kDipTile * 3];
  const int al = threadIdx.x % kDipLanes;
  const int64_t k = int64_t(blockIdx.x) * kDipKPerBlock + threadIdx.x / kDipLanes;
  const bool live = k < K && dipole_k_live(G, dG, k);
  if (!__syncthreads_or(live)) {  // the whole block is pruned (uniform branch)
    if (k < K && al == 0) out_c[k] = out_s[k] = T(0);
    return;
  }
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  T ac = T(0), as = T(0);
  for (int64_t base = 0; base < N; base += kDipTile) {
    const int n = int(min<int64_t>(kDipTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * n; t += 256) {
      sp[t] = pos[3 * base + t];
      sw[t] = w[3 * base + t];
    }
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kDipLanes) {
        T s, c;
        dipole_phase3(kx, ky, kz, sp[3 * i], sp[3 * i + 1], sp[3 * i + 2], s, c);
        const T q = kx * sw[3 * i] + ky * sw[3 * i + 1] + kz * sw[3 * i + 2];
        ac += q * c;
        as += q * s;
      }
  }
  ac = dipole_sum32(ac);
  as = dipole_sum32(as);
  if (k < K && al == 0) {
    out_c[k] = live ? ac : T(0);
    out_s[k] = live ? as : T(0);
  }
}

template <typename T>
__device__ __forceinline__ void dipole_block_sum3(T& x, T& y, T& z, T* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    x += __shfl_xor(x, off, 64);
    y += __shfl_xor(y, off, 64);
    z += __shfl_xor(z, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[3 * wave] = x;
    red[3 * wave + 1] = y;
    red[3 * wave + 2] = z;
  }
  __syncthreads();
  x = red[0] + red[3] + red[6] + red[9];
  y = red[1] + red[4] + red[7] + red[10];
  z = red[2] + red[5] + red[8] + red[11];
}

// Block (i, slice): atom i against the k-vectors [slice * chunk, (slice + 1) * chunk), threads strided over them.
//   GRAD = false: the field E_i (S = structure of the weights)
//   GRAD = true:  dL/dr_i (S = structure of the dipoles mu, Tf = structure of g)
// out (N,3) when there is one slice, otherwise partial sums (n_slices, N, 3) for dipole_reduce_kernel.
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void dipole_atom_kernel(int64_t K, int64_t chunk, const T* __restrict__ pos,
                                                         const T* __restrict__ mu, const T* __restrict__ g,
                                                         const T* __restrict__ kvec, const T* __restrict__ G,
                                                         const T* __restrict__ Sc, const T* __restrict__ Ss,
                                                         const T* __restrict__ Tc, const T* __restrict__ Ts,
                                                         T* __restrict__ out) {
  __shared__ T red[12];
  const int64_t i = blockIdx.x, N = gridDim.x;
  const int64_t k0 = int64_t(blockIdx.y) * chunk, k1 = min<int64_t>(K, k0 + chunk);
  const T x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
  T gx = T(0), gy = T(0), gz = T(0), mx = T(0), my = T(0), mz = T(0);
  if (GRAD) {
    gx = g[3 * i], gy = g[3 * i + 1], gz = g[3 * i + 2];
    mx = mu[3 * i], my = mu[3 * i + 1], mz = mu[3 * i + 2];
  }
  T ax = T(0), ay = T(0), az = T(0);
  for (int64_t k = k0 + threadIdx.x; k < k1; k += 256) {
    const T gk = G[k];
    if (gk == T(0)) continue;  // exact: the term is G(k) times a finite sum
    const T kx = kvec[3 * k], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
    T s, c;
    dipole_phase3(kx, ky, kz, x, y, z, s, c);
    T b;
    if (GRAD)
      b = gk * ((gx * kx + gy * ky + gz * kz) * (c * Ss[k] - s * Sc[k]) +
                (mx * kx + my * ky + mz * kz) * (c * Ts[k] - s * Tc[k]));
    else
      b = gk * (c * Sc[k] + s * Ss[k]);
    ax += b * kx;
    ay += b * ky;
    az += b * kz;
  }
  dipole_block_sum3(ax, ay, az, red);
  if (threadIdx.x == 0) {
    T* o = out + 3 * (int64_t(blockIdx.y) * N + i);
    o[0] = ax;
    o[1] = ay;
    o[2] = az;
  }
}

// out[i, d] = sum over the slices in order of partial[slice, i, d]
template <typename T>
__global__ __launch_bounds__(256) void dipole_reduce_kernel(int64_t n3, int n_slices, const T* __restrict__ partial,
                                                           T* __restrict__ out) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n3) return;
  T acc = T(0);
  for (int s = 0; s < n_slices; ++s) acc += partial[int64_t(s) * n3 + t];
  out[t] = acc;
}

// dL/dk, 32 lanes per k-vector; positions, dipoles and g streamed through LDS
template <typename T>
__global__ __launch_bounds__(256) void dipole_grad_kvectors_kernel(int64_t N, int64_t K, const T* __restrict__ pos,
                                                                  const T* __restrict__ mu, const T* __restrict__ g,
                                                                  const T* __restrict__ kvec, const T* __restrict__ G,
                                                                  const T* __restrict__ dG, const T* __restrict__ Sc,
                                                                  const T* __restrict__ Ss, const T* __restrict__ Tc,
                                                                  const T* __restrict__ Ts, T* __restrict__ grad_k) {
  __shared__ T sp[kDipTile * 3];
  __shared__ T sm[kDipTile * 3];
  __shared__ T sg[kDipTile * 3];
  const int al = threadIdx.x % kDipLanes;
  const int64_t k = int64_t(blockIdx.x) * kDipKPerBlock + threadIdx.x / kDipLanes;
  const bool live = k < K && dipole_k_live(G, dG, k);
  if (!__syncthreads_or(live)) {
    if (k < K && al == 0) grad_k[3 * k] = grad_k[3 * k + 1] = grad_k[3 * k + 2] = T(0);
    return;
  }
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  const T lSc = Sc[kc], lSs = Ss[kc], lTc = Tc[kc], lTs = Ts[kc];
  T ax = T(0), ay = T(0), az = T(0);
  for (int64_t base = 0; base < N; base += kDipTile) {
    const int n = int(min<int64_t>(kDipTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * n; t += 256) {
      sp[t] = pos[3 * base + t];
      sm[t] = mu[3 * base + t];
      sg[t] = g[3 * base + t];
    }
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kDipLanes) {
        const T x = sp[3 * i], y = sp[3 * i + 1], z = sp[3 * i + 2];
        const T mx = sm[3 * i], my = sm[3 * i + 1], mz = sm[3 * i + 2];
        const T gx = sg[3 * i], gy = sg[3 * i + 1], gz = sg[3 * i + 2];
        T s, c;
        dipole_phase3(kx, ky, kz, x, y, z, s, c);
        const T a1 = c * lSc + s * lSs, a2 = c * lTc + s * lTs;
        const T b = (gx * kx + gy * ky + gz * kz) * (c * lSs - s * lSc) + (mx * kx + my * ky + mz * kz) * (c * lTs - s * lTc);
        ax += gx * a1 + mx * a2 + b * x;
        ay += gy * a1 + my * a2 + b * y;
        az += gz * a1 + mz * a2 + b * z;
      }
  }
  ax = dipole_sum32(ax);
  ay = dipole_sum32(ay);
  az = dipole_sum32(az);
  if (k < K && al == 0) {
    if (!live) {
      grad_k[3 * k] = grad_k[3 * k + 1] = grad_k[3 * k + 2] = T(0);
    } else {
      const T gk = G[k], two_dg = T(2) * dG[k] * (lTc * lSc + lTs * lSs);
      grad_k[3 * k] = gk * ax + two_dg * kx;
      grad_k[3 * k + 1] = gk * ay + two_dg * ky;
      grad_k[3 * k + 2] = gk * az + two_dg * kz;
    }
  }
}

// ---- launch helpers --------------------------------------------------------------------------------------------------
static constexpr int64_t kDipTargetBlocks = 2048;  // 256 CUs x 8 workgroups
static constexpr int64_t kDipMinSlice = 1024;      // k-vectors per slice at least (4 per thread)

static int64_t dipole_slices(int64_t N, int64_t K) {
  if (N <= 0 || K <= 0) return 1;
  int64_t s = (kDipTargetBlocks + N - 1) / N;
  s = std::min<int64_t>(s, std::max<int64_t>(1, K / kDipMinSlice));
  return std::max<int64_t>(1, std::min<int64_t>(s, 65535));
}

static inline unsigned dipole_pair_grid(int64_t P) {
  const int64_t b = (P + 255) / 256;
  return unsigned(std::max<int64_t>(1, std::min<int64_t>(b, 256 * 16)));
}

// the pair sum with the instantiation of the descriptor's mode (see dipole_bc)
template <typename T, typename I>
static void dipole_rspace_launch(hipStream_t st, const DipPot<T>& dp, int64_t P, bool full, const void* pairs,
                                 const void* vec, const void* mu, void* out) {
  if (dp.mode == 2)
    dipole_rspace_kernel<T, I, true><<<dipole_pair_grid(P), 256, 0, st>>>(dp, P, full, (const I*)pairs, (const T*)vec,
                                                                          (const T*)mu, (T*)out);
  else
    dipole_rspace_kernel<T, I, false><<<dipole_pair_grid(P), 256, 0, st>>>(dp, P, full, (const I*)pairs, (const T*)vec,
                                                                           (const T*)mu, (T*)out);
}

template <typename T, typename I>
static int dipole_rspace_forward_t(hipStream_t st, int64_t N, int64_t P, int full, const void* pairs, const void* vec,
                                   const void* mu, const mipme_dipole_t* pot, void* out) {
  DipPot<T> dp;
  int rc = make_dippot<T>(pot, dp);
  if (rc) return rc;
  MIPME_CHECK_HIP(zero_async(out, sizeof(T) * size_t(N) * 3, st));
  if (P == 0) return MIPME_OK;
  dipole_rspace_launch<T, I>(st, dp, P, full != 0, pairs, vec, mu, out);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T, typename I>
static int dipole_rspace_backward_t(hipStream_t st, int64_t N, int64_t P, int full, const void* pairs, const void* vec,
                                    const void* mu, const void* g, const mipme_dipole_t* pot, void* grad_mu,
                                    void* grad_vec) {
  DipPot<T> dp;
  int rc = make_dippot<T>(pot, dp);
  if (rc) return rc;
  if (grad_mu) {  // T is symmetric and even in r: the dipole gradient is the forward sum applied to g
    MIPME_CHECK_HIP(zero_async(grad_mu, sizeof(T) * size_t(N) * 3, st));
    if (P > 0) {
      dipole_rspace_launch<T, I>(st, dp, P, full != 0, pairs, vec, g, grad_mu);
      MIPME_LAUNCH_CHECK();
    }
  }
  if (grad_vec && P > 0) {
    if (dp.mode == 2)
      dipole_rspace_grad_vectors_kernel<T, I, true><<<dipole_pair_grid(P), 256, 0, st>>>(
          dp, P, full != 0, (const I*)pairs, (const T*)vec, (const T*)mu, (const T*)g, (T*)grad_vec);
    else
      dipole_rspace_grad_vectors_kernel<T, I, false><<<dipole_pair_grid(P), 256, 0, st>>>(
          dp, P, full != 0, (const I*)pairs, (const T*)vec, (const T*)mu, (const T*)g, (T*)grad_vec);
    MIPME_LAUNCH_CHECK();
  }
  return MIPME_OK;
}

template <typename T>
static int dipole_structure_t(hipStream_t st, int64_t N, int64_t K, const void* pos, const void* w, const void* kvec,
                              const void* G, const void* dG, void* out_c, void* out_s) {
  if (K == 0) return MIPME_OK;
  dipole_structure_kernel<T><<<unsigned((K + kDipKPerBlock - 1) / kDipKPerBlock), 256, 0, st>>>(
      N, K, (const T*)pos, (const T*)w, (const T*)kvec, (const T*)G, (const T*)dG, (T*)out_c, (T*)out_s);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T, bool GRAD>
static int dipole_atoms_t(hipStream_t st, int64_t N, int64_t K, const void* pos, const void* mu, const void* g,
                          const void* kvec, const void* G, const void* Sc, const void* Ss, const void* Tc,
                          const void* Ts, void* out, void* partials) {
  if (N == 0) return MIPME_OK;
  if (K == 0) {
    MIPME_CHECK_HIP(zero_async(out, sizeof(T) * size_t(N) * 3, st));
    return MIPME_OK;
  }
  const int64_t S = dipole_slices(N, K), chunk = (K + S - 1) / S;
  MIPME_REQUIRE(S == 1 || partials != nullptr, "partials scratch of mipme_dipole_partials_size() reals required");
  T* dst = S == 1 ? (T*)out : (T*)partials;
  dipole_atom_kernel<T, GRAD><<<dim3(unsigned(N), unsigned(S)), 256, 0, st>>>(
      K, chunk, (const T*)pos, (const T*)mu, (const T*)g, (const T*)kvec, (const T*)G, (const T*)Sc, (const T*)Ss,
      (const T*)Tc, (const T*)Ts, dst);
  MIPME_LAUNCH_CHECK();
  if (S > 1) {
    dipole_reduce_kernel<T><<<unsigned((3 * N + 255) / 256), 256, 0, st>>>(3 * N, int(S), (const T*)partials, (T*)out);
    MIPME_LAUNCH_CHECK();
  }
  return MIPME_OK;
}

template <typename T>
static int dipole_grad_kvectors_t(hipStream_t st, int64_t N, int64_t K, const void* pos, const void* mu, const void* g,
                                  const void* kvec, const void* G, const void* dG, const void* Sc, const void* Ss,
                                  const void* Tc, const void* Ts, void* grad_k) {
  if (K == 0) return MIPME_OK;
  dipole_grad_kvectors_kernel<T><<<unsigned((K + kDipKPerBlock - 1) / kDipKPerBlock), 256, 0, st>>>(
      N, K, (const T*)pos, (const T*)mu, (const T*)g, (const T*)kvec, (const T*)G, (const T*)dG, (const T*)Sc,
      (const T*)Ss, (const T*)Tc, (const T*)Ts, (T*)grad_k);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int dipole_backward_t(hipStream_t st, int64_t N, int64_t K, const void* pos, const void* mu, const void* g,
                             const void* kvec, const void* G, const void* dG, const void* Sc, const void* Ss,
                             const void* Tc, const void* Ts, void* grad_pos, void* grad_k, void* partials) {
  if (grad_pos) {
    int rc = dipole_atoms_t<T, true>(st, N, K, pos, mu, g, kvec, G, Sc, Ss, Tc, Ts, grad_pos, partials);
    if (rc) return rc;
  }
  if (grad_k && N == 0) {
    MIPME_CHECK_HIP(zero_async(grad_k, sizeof(T) * size_t(K) * 3, st));
    return MIPME_OK;
  }
  if (grad_k) return dipole_grad_kvectors_t<T>(st, N, K, pos, mu, g, kvec, G, dG, Sc, Ss, Tc, Ts, grad_k);
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

#define DIP_DT(dtype, F32CALL, F64CALL)       \
  do {                                        \
    if ((dtype) == MIPME_F32) return F32CALL; \
    if ((dtype) == MIPME_F64) return F64CALL; \
    set_error("invalid dtype %d", dtype);     \
    return MIPME_EINVAL;                      \
  } while (0)

#define DIP_DT_IDX(dtype, itype, CALL)                                                \
  do {                                                                                \
    if ((itype) != MIPME_I64 && (itype) != MIPME_I32) {                               \
      set_error("invalid index dtype %d", itype);                                     \
      return MIPME_EINVAL;                                                            \
    }                                                                                 \
    const bool i64 = (itype) == MIPME_I64;                                            \
    if ((dtype) == MIPME_F32) return i64 ? CALL(float, int64_t) : CALL(float, int32_t); \
    if ((dtype) == MIPME_F64) return i64 ? CALL(double, int64_t) : CALL(double, int32_t); \
    set_error("invalid dtype %d", dtype);                                             \
    return MIPME_EINVAL;                                                              \
  } while (0)

extern "C" {

int mipme_dipole_rspace_forward(void* stream, int dtype, int index_dtype, int64_t n_atoms, int64_t n_pairs,
                                int full_list, const void* neighbor_indices, const void* neighbor_vectors,
                                const void* dipoles, const mipme_dipole_t* pot, void* out) {
  MIPME_REQUIRE(n_atoms >= 0 && n_pairs >= 0, "invalid sizes passed to mipme_dipole_rspace_forward");
  MIPME_REQUIRE((n_atoms == 0 || out) && (n_pairs == 0 || (neighbor_indices && neighbor_vectors && dipoles)),
                "NULL buffer passed to mipme_dipole_rspace_forward");
  hipStream_t st = (hipStream_t)stream;
#define DIP_FWD(T, I) dipole_rspace_forward_t<T, I>(st, n_atoms, n_pairs, full_list, neighbor_indices, neighbor_vectors, dipoles, pot, out)
  DIP_DT_IDX(dtype, index_dtype, DIP_FWD);
#undef DIP_FWD
}

int mipme_dipole_rspace_backward(void* stream, int dtype, int index_dtype, int64_t n_atoms, int64_t n_pairs,
                                 int full_list, const void* neighbor_indices, const void* neighbor_vectors,
                                 const void* dipoles, const void* grad_out, const mipme_dipole_t* pot,
                                 void* grad_dipoles, void* grad_vectors) {
  MIPME_REQUIRE(n_atoms >= 0 && n_pairs >= 0, "invalid sizes passed to mipme_dipole_rspace_backward");
  MIPME_REQUIRE(n_pairs == 0 || (neighbor_indices && neighbor_vectors && dipoles && grad_out),
                "NULL buffer passed to mipme_dipole_rspace_backward");
  hipStream_t st = (hipStream_t)stream;
#define DIP_BWD(T, I)                                                                                                  \
  dipole_rspace_backward_t<T, I>(st, n_atoms, n_pairs, full_list, neighbor_indices, neighbor_vectors, dipoles, grad_out, \
                                 pot, n_atoms > 0 ? grad_dipoles : nullptr, grad_vectors)
  DIP_DT_IDX(dtype, index_dtype, DIP_BWD);
#undef DIP_BWD
}

int64_t mipme_dipole_partials_size(int64_t n_atoms, int64_t n_k) {
  const int64_t S = dipole_slices(n_atoms, n_k);
  return S > 1 ? S * n_atoms * 3 : 0;
}

int mipme_dipole_structure(void* stream, int dtype, int64_t n_atoms, int64_t n_k, const void* positions,
                           const void* weights, const void* kvectors, const void* G, const void* dG, void* out_cos,
                           void* out_sin) {
  MIPME_REQUIRE(n_atoms >= 0 && n_k >= 0 && n_k <= int64_t(kDipKPerBlock) * 0x7fffffff,
                "invalid sizes passed to mipme_dipole_structure");
  MIPME_REQUIRE(n_k == 0 || (kvectors && out_cos && out_sin && (n_atoms == 0 || (positions && weights))),
                "NULL buffer passed to mipme_dipole_structure");
  hipStream_t st = (hipStream_t)stream;
  DIP_DT(dtype, dipole_structure_t<float>(st, n_atoms, n_k, positions, weights, kvectors, G, dG, out_cos, out_sin),
         dipole_structure_t<double>(st, n_atoms, n_k, positions, weights, kvectors, G, dG, out_cos, out_sin));
}

int mipme_dipole_field(void* stream, int dtype, int64_t n_atoms, int64_t n_k, const void* positions,
                       const void* kvectors, const void* G, const void* s_cos, const void* s_sin, void* out,
                       void* partials) {
  MIPME_REQUIRE(n_atoms >= 0 && n_atoms <= 0x7fffffff && n_k >= 0, "invalid sizes passed to mipme_dipole_field");
  MIPME_REQUIRE(n_atoms == 0 || (positions && out && (n_k == 0 || (kvectors && G && s_cos && s_sin))),
                "NULL buffer passed to mipme_dipole_field");
  hipStream_t st = (hipStream_t)stream;
  DIP_DT(dtype,
         (dipole_atoms_t<float, false>(st, n_atoms, n_k, positions, nullptr, nullptr, kvectors, G, s_cos, s_sin, nullptr,
                                       nullptr, out, partials)),
         (dipole_atoms_t<double, false>(st, n_atoms, n_k, positions, nullptr, nullptr, kvectors, G, s_cos, s_sin,
                                        nullptr, nullptr, out, partials)));
}

int mipme_dipole_backward(void* stream, int dtype, int64_t n_atoms, int64_t n_k, const void* positions,
                          const void* dipoles, const void* grad_out, const void* kvectors, const void* G, const void* dG,
                          const void* s_cos, const void* s_sin, const void* t_cos, const void* t_sin,
                          void* grad_positions, void* grad_kvectors, void* partials) {
  MIPME_REQUIRE(n_atoms >= 0 && n_atoms <= 0x7fffffff && n_k >= 0 && n_k <= int64_t(kDipKPerBlock) * 0x7fffffff,
                "invalid sizes passed to mipme_dipole_backward");
  MIPME_REQUIRE(n_atoms == 0 || n_k == 0 ||
                    (positions && dipoles && grad_out && kvectors && G && s_cos && s_sin && t_cos && t_sin),
                "NULL buffer passed to mipme_dipole_backward");
  MIPME_REQUIRE(!grad_kvectors || dG || n_k == 0, "grad_kvectors needs dG");
  hipStream_t st = (hipStream_t)stream;
  DIP_DT(dtype,
         dipole_backward_t<float>(st, n_atoms, n_k, positions, dipoles, grad_out, kvectors, G, dG, s_cos, s_sin, t_cos,
                                  t_sin, grad_positions, grad_kvectors, partials),
         dipole_backward_t<double>(st, n_atoms, n_k, positions, dipoles, grad_out, kvectors, G, dG, s_cos, s_sin, t_cos,
                                   t_sin, grad_positions, grad_kvectors, partials));
}

}  // extern "C"
