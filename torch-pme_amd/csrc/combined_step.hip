// Energy + forces (+ weight and charge gradients) of a weighted sum of range-separated 1/r^p potentials in ONE step
// (mipme_combined_step, include/mipme.h): everything is linear in the potential, so
//
//   mesh part    one pass with the contracted table G = sum_t w_t G_t          (combined_contract_kernel + the existing launches)
//   pair part    one walk over the row stream with sum_t w_t v_t(d)            (combined_rows_kernel)
//   dE/dw_t      the energy of term t alone: pair sums per term from the same walk, (1/2V) sum_k mu_k G_t |rho^|^2 from one
//                pass over rho^ (combined_kenergy_kernel), the self / background constants of the term
//
// and one launch (combined_finish_kernel) assembles V_a, the forces and the sums.  The weights are read from device memory by
// every kernel: an optimizer step on them is seen by the next call of a captured graph.
//
// Launch order on the one stream: contract -> mesh part (binning, spread, convolution, gather: mipme_kspace_forward as it is) ->
// pair rows -> per-term mesh energies -> finish.  The rows read the (x, y, z, q) records the binning pass leaves, so they follow
// the mesh part; nothing runs beside anything else.
//
// No atomics in the kernels of this file; every sum is formed in a fixed order (the same bits run after run for the pair part).
#include <cmath>
#include <cstring>

#include "host.h"
#include "rows_body.h"
#include "srpot.h"
#include "step_device.h"

namespace mipme {

constexpr int kCsBlock = kStepBlock, kCsRowsPerBlock = kStepRowsPerBlock;  // (the block shapes of step_device.h)
constexpr int kCsMaxTerms = MIPME_COMBINED_MAX_TERMS;
constexpr int kCsRowPart = 4 + kCsMaxTerms;     // per row block: sum q V_sr, sum q^2, sum q phi, -, sum q u_t
constexpr int kCsKBlocksMax = 256;              // blocks of the per-term mesh energies

// what the kernels need of the terms, in the kernel arguments
struct CsTerms {
  int n_terms;
  int p[kCsMaxTerms];
  double inv_2s2[kCsMaxTerms], c1[kCsMaxTerms], pref[kCsMaxTerms];
  double self_t[kCsMaxTerms], bg_t[kCsMaxTerms];  // correction_terms() of every term
  double cheb[kErfcChebTerms];                    // erfc coefficients of the fp64 pair function
};

// work (float64): [row partials kCsRowPart per row block][k partials kCsMaxTerms per k block][consts: self_c, bg_c, one (as T), -]
//                 [phi: N slots (values of T)]
struct CsWork {
  int64_t n_row_blocks, n_k_blocks;
  double *row_part, *k_part, *consts;
  void* phi;
  int64_t total;
};
static int64_t cs_k_blocks(const mipme_mesh_t* m) {
  const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
  return std::max<int64_t>(1, std::min<int64_t>((Mh + kCsBlock - 1) / kCsBlock, kCsKBlocksMax));
}
static CsWork cs_work_layout(const mipme_mesh_t* m, int64_t N, void* base) {
  CsWork w;
  w.n_row_blocks = (N + kCsRowsPerBlock - 1) / kCsRowsPerBlock;
  w.n_k_blocks = cs_k_blocks(m);
  double* b = (double*)base;
  w.row_part = b;
  w.k_part = w.row_part + kCsRowPart * w.n_row_blocks;
  w.consts = w.k_part + kCsMaxTerms * w.n_k_blocks;
  w.phi = w.consts + 4;
  w.total = kCsRowPart * w.n_row_blocks + kCsMaxTerms * w.n_k_blocks + 4 + N;
  return w;
}

// ---- 1. contract: G = sum_t w_t G_t over the half grid; self_c = sum_t w_t self_t, bg_c = sum_t w_t bg_t ------------------------
// VEC reals per thread and step (16-byte loads) when the half grid allows it (Mh a multiple of VEC: every table is then aligned)
template <typename T>
__global__ __launch_bounds__(kCsBlock) void combined_contract_kernel(CsTerms ct, int64_t Mh, const T* __restrict__ weights,
                                                                    const T* __restrict__ G_terms, T* __restrict__ G,
                                                                    double* __restrict__ consts) {
  constexpr int VEC = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  __shared__ T w_s[kCsMaxTerms];
  if (threadIdx.x < kCsMaxTerms) w_s[threadIdx.x] = int(threadIdx.x) < ct.n_terms ? weights[threadIdx.x] : T(0);
  __syncthreads();
  const int nt = ct.n_terms;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double sc = 0.0, bc = 0.0;
#pragma unroll
    for (int t = 0; t < kCsMaxTerms; ++t) {
      if (t < nt) {
        sc += double(w_s[t]) * ct.self_t[t];
        bc += double(w_s[t]) * ct.bg_t[t];
      }
    }
    consts[0] = sc;
    consts[1] = bc;
    *reinterpret_cast<T*>(consts + 2) = T(1);  // the unit seed of the field gather on meshes without bricks
  }
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (Mh % VEC == 0) {
    const int64_t nv = Mh / VEC;
    for (int64_t i = tid; i < nv; i += stride) {
      vec_t acc = vec_t(T(0));
      for (int t = 0; t < nt; ++t) acc += w_s[t] * reinterpret_cast<const vec_t*>(G_terms + int64_t(t) * Mh)[i];
      reinterpret_cast<vec_t*>(G)[i] = acc;
    }
  } else {
    for (int64_t i = tid; i < Mh; i += stride) {
      T acc = T(0);
      for (int t = 0; t < nt; ++t) acc += w_s[t] * G_terms[int64_t(t) * Mh + i];
      G[i] = acc;
    }
  }
}

// ---- records of a mesh without bricks (the binning pass writes them otherwise) -----------------------------------------------
template <typename T>
__global__ __launch_bounds__(kCsBlock) void combined_records_kernel(int64_t N, const T* __restrict__ pos, const T* __restrict__ q,
                                                                   AtomRecord<T>* __restrict__ rec) {
  const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a < N) rec[a] = AtomRecord<T>{pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], q[a]};
}

// ---- 2. combined pair rows ---------------------------------------------------------------------------------------------------
// 16 lanes per atom row, 4 rows per wavefront, 256 threads; the 7^3 table of Cartesian shift vectors in LDS; one 16-byte record
// gather per entry (entries: other | code << 22); d^2 once per entry, then a loop over the terms that is uniform across the
// wavefront with a switch on the exponent into fast_rs_eval<P, true>.  Term parameters and weights are read with a uniform index
// from LDS; with WGRAD the per-term sums of every lane live in LDS too (no dynamically indexed registers, no scratch).
//   out[a]   = 1/2 sum_{potential entries} q_o sum_t w_t v_t          (roles as mipme_sr_rows_fused, potential + force sums)
//   force[a] = -sum_e q_o (sum_t w_t v_t'/d) vec_e
//   part[b]  = {sum q_a out_a, sum q_a^2, sum q_a phi_a, -, sum q_a u_t[a] (t < n_terms)} over the rows of workgroup b, float64
template <typename T>
struct CsRowTerm {
  T inv_2s2, c1, pref, w;
};

template <typename T, int P>
__device__ __forceinline__ void cs_eval2(const CsRowTerm<T>& tp, const T (&d2)[2], T (&v)[2], T (&dvd)[2], const double* cheb) {
#pragma unroll
  for (int u = 0; u < 2; ++u) fast_rs_eval<P, true, T>(tp.inv_2s2, tp.c1, tp.pref, d2[u], v[u], dvd[u], cheb);
}

template <typename T, bool WGRAD>
__global__ __launch_bounds__(kCsBlock) void combined_rows_kernel(CsTerms ct, int64_t N, const int* __restrict__ row_ptr,
                                                                const int* __restrict__ ent32,
                                                                const AtomRecord<T>* __restrict__ rec, const T* __restrict__ cell,
                                                                const T* __restrict__ weights, const T* __restrict__ phi,
                                                                int full, T* __restrict__ out, T* __restrict__ force,
                                                                double* __restrict__ part) {
  constexpr int U = 2;  // entries in flight per lane
  __shared__ AtomRecord<T> shift_tab[kShiftTableSize];
  __shared__ CsRowTerm<T> term_s[kCsMaxTerms];
  __shared__ int p_s[kCsMaxTerms];
  __shared__ T acc_s[WGRAD ? kCsMaxTerms : 1][kCsBlock];
  __shared__ double red[kCsBlock / 64][kCsRowPart];
  const int tid = threadIdx.x;
  const int nt = ct.n_terms;
  if (tid < kCsMaxTerms) {
    const bool live = tid < nt;
    term_s[tid] = CsRowTerm<T>{T(ct.inv_2s2[tid]), T(ct.c1[tid]), T(ct.pref[tid]), live ? weights[tid] : T(0)};
    p_s[tid] = live ? ct.p[tid] : 1;
  }
  step_fill_shift_table(shift_tab, cell);
  if constexpr (WGRAD) {
    for (int t = 0; t < kCsMaxTerms; ++t) acc_s[t][tid] = T(0);
  }
  __syncthreads();
  const int sub = tid % 16;
  int64_t a = int64_t(blockIdx.x) * kCsRowsPerBlock + tid / 16;
  const bool valid = a < N;
  if (!valid) a = N - 1;
  const int* __restrict__ rp = row_ptr + 2 * a;
  const int r0 = rp[0], mid = rp[1], r2 = rp[2];
  // a full list feeds the potential from role i only; the force sums walk both roles
  const int pot_end = full ? mid : r2;
  const int beg = r0, end = valid ? r2 : r0;
  const AtomRecord<T> own = rec[a];
  const T ax = own.x, ay = own.y, az = own.z, qa = own.w;
  T pot = T(0), fx = T(0), fy = T(0), fz = T(0);
  for (int base = beg; base < end; base += 16 * U) {
    T vx[U], vy[U], vz[U], d2[U], wf[U], wp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = base + u * 16 + sub;
      const bool ok = e < end;
      const int word = ent32[ok ? e : beg];  // (beg < end here: a real entry, given zero weight)
      const AtomRecord<T> o = rec[word & int(kCompactMaxAtoms - 1)];
      const AtomRecord<T> sh = shift_tab[unsigned(word) >> kCompactAtomBits];
      vx[u] = (o.x - ax) + sh.x;
      vy[u] = (o.y - ay) + sh.y;
      vz[u] = (o.z - az) + sh.z;
      d2[u] = vx[u] * vx[u] + vy[u] * vy[u] + vz[u] * vz[u];
      wf[u] = ok ? o.w : T(0);
      wp[u] = (ok && e < pot_end) ? o.w : T(0);
    }
    T sv[U], sd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) sv[u] = sd[u] = T(0);
    for (int t = 0; t < nt; ++t) {  // uniform across the workgroup
      const CsRowTerm<T> tp = term_s[t];
      T v[U], dvd[U];
      switch (p_s[t]) {
        case 1: cs_eval2<T, 1>(tp, d2, v, dvd, ct.cheb); break;
        case 2: cs_eval2<T, 2>(tp, d2, v, dvd, ct.cheb); break;
        case 3: cs_eval2<T, 3>(tp, d2, v, dvd, ct.cheb); break;
        case 4: cs_eval2<T, 4>(tp, d2, v, dvd, ct.cheb); break;
        case 5: cs_eval2<T, 5>(tp, d2, v, dvd, ct.cheb); break;
        default: cs_eval2<T, 6>(tp, d2, v, dvd, ct.cheb); break;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sv[u] += tp.w * v[u];
        sd[u] += tp.w * dvd[u];
      }
      if constexpr (WGRAD) {
        T add = T(0);
#pragma unroll
        for (int u = 0; u < U; ++u) add += wp[u] * v[u];
        acc_s[t][tid] += add;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pot += wp[u] * sv[u];
      const T sc = wf[u] * sd[u];
      fx -= sc * vx[u];
      fy -= sc * vy[u];
      fz -= sc * vz[u];
    }
  }
  pot = T(0.5) * row_sum(pot);
  fx = row_sum(fx);
  fy = row_sum(fy);
  fz = row_sum(fz);
  const bool mine = sub == 0 && valid;
  if (mine) {
    out[a] = pot;
    force[3 * a] = fx;
    force[3 * a + 1] = fy;
    force[3 * a + 2] = fz;
  }
  // block sums in float64: per wave by shuffles, then the waves in index order
  const int lane = tid & 63, wave = tid >> 6;
  const double qd = mine ? double(qa) : 0.0;
  const double e0 = wave_sum(qd * double(pot));
  const double e1 = wave_sum(qd * qd);
  const double e2 = wave_sum(mine ? qd * double(phi[a]) : 0.0);
  if (lane == 0) {
    red[wave][0] = e0;
    red[wave][1] = e1;
    red[wave][2] = e2;
    red[wave][3] = 0.0;
  }
  if constexpr (WGRAD) {
    const double ql = valid ? 0.5 * double(qa) : 0.0;  // every lane's share of q_a u_t[a]
    for (int t = 0; t < nt; ++t) {
      const double s = wave_sum(ql * double(acc_s[t][tid]));
      if (lane == 0) red[wave][4 + t] = s;
    }
  }
  __syncthreads();
  const int n_out = WGRAD ? 4 + nt : 4;
  if (tid < n_out) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kCsBlock / 64; ++w) s += red[w][tid];
    part[int64_t(blockIdx.x) * kCsRowPart + tid] = s;
  }
}

// ---- 4. per-term mesh energies: sum_k mu_k G_t(k) |rho^(k)|^2 over the half grid, all terms in one pass over rho^ --------------
// mu = 2 except on the kz = 0 and kz = nz/2 planes (the convention of the x stage's energy partials); the 1/2V is the finish's
template <typename T>
__global__ __launch_bounds__(kCsBlock) void combined_kenergy_kernel(int n_terms, int64_t Mh, int nzh, int nz,
                                                                   const T* __restrict__ G_terms, const T* __restrict__ rho_hat,
                                                                   double* __restrict__ k_part) {
  __shared__ double red[kCsBlock / 64][kCsMaxTerms];
  double acc[kCsMaxTerms];
#pragma unroll
  for (int t = 0; t < kCsMaxTerms; ++t) acc[t] = 0.0;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < Mh; k += stride) {
    const int iz = int(k % nzh);
    const double re = double(rho_hat[2 * k]), im = double(rho_hat[2 * k + 1]);
    const double w = ((iz == 0 || 2 * iz == nz) ? 1.0 : 2.0) * (re * re + im * im);
#pragma unroll
    for (int t = 0; t < kCsMaxTerms; ++t)
      if (t < n_terms) acc[t] += w * double(G_terms[int64_t(t) * Mh + k]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < kCsMaxTerms; ++t) {
    const double s = wave_sum(acc[t]);
    if (lane == 0) red[wave][t] = s;
  }
  __syncthreads();
  if (threadIdx.x < kCsMaxTerms) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kCsBlock / 64; ++w) s += red[w][threadIdx.x];
    k_part[int64_t(blockIdx.x) * kCsMaxTerms + threadIdx.x] = s;
  }
}

// ---- 5. finish ---------------------------------------------------------------------------------------------------------------
// per atom:  V_a = V_sr[a] + 1/2 (phi_a - q_a self_c - 2 bg_c Q / V);  grad_positions[a] = s q_a (c' pair_force[a] + field[a]);
// grad_charges[a] = 2 V_a.  Workgroup 0 then adds up the block partials, every sum in a fixed order:
//   energy = sum q V_sr + 1/2 sum q phi - 1/2 self_c sum q^2 - bg_c Q^2 / V                       (= sum_a q_a V_a)
//   grad_weights[t] = sum q u_t + (1/2V) sum_k mu G_t |rho^|^2 - 1/2 self_t sum q^2 - bg_t Q^2 / V
// field_has_q: `field` holds q_a field[a] already (meshes without bricks)
template <typename T>
__global__ __launch_bounds__(kCsBlock) void combined_finish_kernel(CsTerms ct, int64_t N, double inv_vol, const T* __restrict__ q,
                                                                  const T* __restrict__ phi, const T* __restrict__ dc,
                                                                  const double* __restrict__ consts, T* __restrict__ pot,
                                                                  const T* __restrict__ pair_force, const T* __restrict__ field,
                                                                  int field_has_q, T force_scale, const T* __restrict__ seed,
                                                                  T* __restrict__ grad_pos, T* __restrict__ grad_q,
                                                                  const double* __restrict__ row_part, int64_t n_row_blocks,
                                                                  const double* __restrict__ k_part, int64_t n_k_blocks,
                                                                  T* __restrict__ energy, T* __restrict__ grad_w) {
  __shared__ double red[kCsBlock / 64];
  const double self_c = consts[0], bg_c = consts[1];
  const double Q = double(dc[0]);
  const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (a < N) {
    const T qa = q[a];
    const T v = pot[a] + T(0.5) * (phi[a] - qa * T(self_c) - T(2.0 * bg_c * Q * inv_vol));
    pot[a] = v;
    if (grad_q) grad_q[a] = T(2) * v;
    const T s = seed ? seed[0] : T(1);
    const T mq = field_has_q ? T(1) : qa;
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_pos[3 * a + c] = s * (qa * force_scale * pair_force[3 * a + c] + mq * field[3 * a + c]);
  }
  if (blockIdx.x != 0) return;
  const int nt = ct.n_terms;
  // thread i adds the blocks i, i + 256, ... in that order; the threads are then added up in a fixed order too
  double s_sr = 0.0, s_q2 = 0.0, s_phi = 0.0;
  for (int64_t b = threadIdx.x; b < n_row_blocks; b += kCsBlock) {
    s_sr += row_part[b * kCsRowPart];
    s_q2 += row_part[b * kCsRowPart + 1];
    s_phi += row_part[b * kCsRowPart + 2];
  }
  s_sr = block_sum<kCsBlock / 64>(s_sr, red);
  s_q2 = block_sum<kCsBlock / 64>(s_q2, red);
  s_phi = block_sum<kCsBlock / 64>(s_phi, red);
  if (threadIdx.x == 0) energy[0] = T(s_sr + 0.5 * s_phi - 0.5 * self_c * s_q2 - bg_c * Q * Q * inv_vol);
  if (grad_w) {
    for (int t = 0; t < nt; ++t) {
      double u = 0.0, ek = 0.0;
      for (int64_t b = threadIdx.x; b < n_row_blocks; b += kCsBlock) u += row_part[b * kCsRowPart + 4 + t];
      for (int64_t b = threadIdx.x; b < n_k_blocks; b += kCsBlock) ek += k_part[b * kCsMaxTerms + t];
      u = block_sum<kCsBlock / 64>(u, red);
      ek = block_sum<kCsBlock / 64>(ek, red);
      if (threadIdx.x == 0)
        grad_w[t] = T(u + 0.5 * inv_vol * ek - 0.5 * ct.self_t[t] * s_q2 - ct.bg_t[t] * Q * Q * inv_vol);
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T>
static int combined_step_t(const mipme_combined_step_args_t& a, const CsTerms& ct, bool binned) {
  hipStream_t st = (hipStream_t)a.stream;
  const mipme_mesh_t* m = a.mesh;
  const int64_t N = a.n_atoms;
  const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
  const CsWork w = cs_work_layout(m, N, a.work);
  const bool wgrad = a.grad_weights != nullptr;
  int rc;
  combined_contract_kernel<T><<<stride_grid(Mh / (16 / sizeof(T)) + 1, kCsBlock), kCsBlock, 0, st>>>(
      ct, Mh, (const T*)a.weights, (const T*)a.G_terms, (T*)a.G, w.consts);
  MIPME_LAUNCH_CHECK();
  // the mesh part: the existing launches, unchanged.  out_lr (with the corrections of term 0 alone) lands in `potentials` and is
  // overwritten by the rows; what is kept is the raw gather / V (phi), the field and rho^
  mipme_kspace_forward_args_t f;
  std::memset(&f, 0, sizeof(f));
  f.size = sizeof(f);
  f.version = MIPME_ARGS_VERSION;
  f.plan = a.plan;
  f.stream = a.stream;
  f.dtype = a.dtype;
  f.mesh = m;
  f.pot = &a.comb->terms[0];
  f.n_atoms = N;
  f.positions = a.positions;
  f.charges = a.charges;
  f.G = a.G;
  f.rho_mesh = a.rho_mesh;
  f.hat_work = a.hat_work;
  f.phi_mesh = a.phi_mesh;
  f.dc = a.dc;
  f.out_lr = a.potentials;
  f.out_phi = w.phi;
  f.nan_flag = a.nan_flag;
  f.out_rho_hat = wgrad ? a.rho_hat : nullptr;
  if (binned) {
    f.atom_bins = a.atom_bins;
    f.out_field = a.field;
    f.out_records = a.records;
    f.flags = MIPME_FWD_RHO_MESH_UNUSED;
  } else {
    combined_records_kernel<T><<<unsigned((N + kCsBlock - 1) / kCsBlock), kCsBlock, 0, st>>>(
        N, (const T*)a.positions, (const T*)a.charges, (AtomRecord<T>*)a.records);
    MIPME_LAUNCH_CHECK();
  }
  if ((rc = mipme_kspace_forward(&f))) return rc;
  if (!binned) {
    // field <- q_a (1/V) sum_g phi(g) grad W_a(g): the gradient gather in its energy mode with a unit seed and g = q
    double self0, bg0;
    correction_terms(&a.comb->terms[0], self0, bg0);
    if ((rc = gather_grad_impl<T>(st, m, N, a.positions, a.charges, a.charges, a.phi_mesh, a.phi_mesh, a.dc, w.consts + 2, self0, bg0,
                                  a.field, nullptr)))
      return rc;
  }
  const unsigned row_blocks = unsigned(w.n_row_blocks);
  if (wgrad)
    combined_rows_kernel<T, true><<<row_blocks, kCsBlock, 0, st>>>(ct, N, (const int*)a.row_ptr, (const int*)a.entries,
                                                                   (const AtomRecord<T>*)a.records, (const T*)a.cell,
                                                                   (const T*)a.weights, (const T*)w.phi, a.full_list,
                                                                   (T*)a.potentials, (T*)a.pair_force, w.row_part);
  else
    combined_rows_kernel<T, false><<<row_blocks, kCsBlock, 0, st>>>(ct, N, (const int*)a.row_ptr, (const int*)a.entries,
                                                                    (const AtomRecord<T>*)a.records, (const T*)a.cell,
                                                                    (const T*)a.weights, (const T*)w.phi, a.full_list,
                                                                    (T*)a.potentials, (T*)a.pair_force, w.row_part);
  MIPME_LAUNCH_CHECK();
  if (wgrad) {
    combined_kenergy_kernel<T><<<unsigned(w.n_k_blocks), kCsBlock, 0, st>>>(ct.n_terms, Mh, m->nz / 2 + 1, m->nz,
                                                                            (const T*)a.G_terms, (const T*)a.rho_hat, w.k_part);
    MIPME_LAUNCH_CHECK();
  }
  combined_finish_kernel<T><<<unsigned((N + kCsBlock - 1) / kCsBlock), kCsBlock, 0, st>>>(
      ct, N, 1.0 / m->volume, (const T*)a.charges, (const T*)w.phi, (const T*)a.dc, w.consts, (T*)a.potentials,
      (const T*)a.pair_force, (const T*)a.field, binned ? 0 : 1, T(a.full_list ? 0.5 : 1.0), (const T*)a.grad_seed,
      (T*)a.grad_positions, (T*)a.grad_charges, w.row_part, w.n_row_blocks, w.k_part, w.n_k_blocks, (T*)a.energy,
      (T*)a.grad_weights);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_combined_step_work(const mipme_fft_plan* plan, const mipme_mesh_t* mesh, int64_t n_atoms, int n_terms) {
  (void)plan;
  if (!mesh || n_atoms < 0 || n_terms < 1 || n_terms > kCsMaxTerms) return 0;
  return cs_work_layout(mesh, n_atoms, nullptr).total;
}

int mipme_combined_step(const mipme_combined_step_args_t* in) {
  const char* who = "mipme_combined_step";
  mipme_combined_step_args_t a;
  int rc = load_args(in, a, MIPME_COMBINED_STEP_VERSION, who);
  if (rc) return rc;
  // (what the arguments alone decide comes before anything that needs a device or reads the plan)
  MIPME_REQUIRE(a.dtype == MIPME_F32 || a.dtype == MIPME_F64, "%s: invalid dtype %d", who, int(a.dtype));
  MIPME_REQUIRE(a.comb != nullptr, "%s: combined descriptor is NULL", who);
  const int nt = a.comb->n_terms;
  MIPME_REQUIRE(nt >= 1 && nt <= kCsMaxTerms, "%s: n_terms is %d but a combination holds 1 to %d terms (MIPME_COMBINED_MAX_TERMS)",
                who, nt, kCsMaxTerms);
  CsTerms ct;
  std::memset(&ct, 0, sizeof(ct));
  ct.n_terms = nt;
  for (int t = 0; t < nt; ++t) {
    const mipme_potential_t& pt = a.comb->terms[t];
    const int p = pt.kind == MIPME_COULOMB ? 1 : pt.exponent;
    MIPME_REQUIRE(p >= 1 && p <= 6, "%s: term %d: Unsupported exponent: %d", who, t, p);
    if (t == 0)
      MIPME_REQUIRE(pt.smearing > 0, "%s: term 0 is a direct potential (`smearing` is %g): the step serves range-separated "
                    "combinations only", who, pt.smearing);
    else
      MIPME_REQUIRE(pt.smearing > 0, "%s: term %d has no `smearing` in a range-separated combination (term 0 has one)", who, t);
    ct.p[t] = p;
    ct.inv_2s2[t] = 0.5 / (pt.smearing * pt.smearing);
    ct.c1[t] = std::sqrt(ct.inv_2s2[t]);
    ct.pref[t] = pt.prefactor;
    correction_terms(&pt, ct.self_t[t], ct.bg_t[t]);
  }
  for (int t = nt; t < kCsMaxTerms; ++t) ct.p[t] = 1;
  {
    const double cheb[kErfcChebTerms] = MIPME_ERFC_CHEB;
    for (int k = 0; k < kErfcChebTerms; ++k) ct.cheb[k] = cheb[k];
  }
  if ((rc = validate_mesh(a.mesh))) return rc;
  const mipme_mesh_t* m = a.mesh;
  MIPME_REQUIRE(m->n_channels == 1, "%s: the step serves one charge channel, the mesh has %d", who, int(m->n_channels));
  MIPME_REQUIRE(m->nx > 0 && (m->nx & (m->nx - 1)) == 0,
                "%s: the step runs the fused convolution, which needs a power-of-two nx (the mesh has nx = %d)", who, int(m->nx));
  if ((rc = check_step_rows(a.shift_format, a.n_atoms, who))) return rc;
  MIPME_REQUIRE(!a.grad_charges || !a.full_list,
                "%s: grad_charges = 2 V needs a half list (a full list need not be symmetric)", who);
  MIPME_REQUIRE(!a.grad_weights || a.rho_hat, "%s: grad_weights needs rho_hat (the per-term mesh energies are sums over rho^)", who);
  MIPME_REQUIRE(a.plan && a.positions && a.charges && a.cell && a.weights && a.G_terms && a.G && a.rho_mesh && a.hat_work &&
                    a.phi_mesh && a.dc && a.records && a.row_ptr && a.entries && a.potentials && a.pair_force && a.field &&
                    a.energy && a.grad_positions && a.work,
                "%s: NULL required buffer", who);
  const bool binned = bricks_supported(m, a.dtype);
  MIPME_REQUIRE(!binned || a.atom_bins, "%s: NULL required buffer (atom_bins: mipme_atom_bins_bytes() > 0 for this mesh)", who);
  // ---- from here on the plan is read
  const FftDims d = fft_plan_dims(a.plan);
  MIPME_REQUIRE(d.dtype == a.dtype && d.nx == m->nx && d.ny == m->ny && d.nz == m->nz && d.batch == 1,
                "The real-space mesh is inconsistent with the k-space grid.");
  MIPME_REQUIRE(fft_plan_xfused(a.plan), "%s: the plan has no fused convolution (power-of-two nx)", who);
  DT_SWITCH(a.dtype, combined_step_t<float>(a, ct, binned), combined_step_t<double>(a, ct, binned));
}

}  // extern "C"
