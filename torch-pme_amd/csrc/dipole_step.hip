// Energy, forces and dE/dmu (+ dE/dcell) of point dipoles in ONE step (mipme_dipole_step, include/mipme.h): the MD form of
// CalculatorDipole, every launch on one stream so that the whole step is one captured graph.
//
// E = sum_i mu_i . V_i is quadratic in the dipoles, so with the upstream gradient g = mu the structure factors of g are those of
// mu (T = S) and everything the eager forward + backward computes in five passes over the (k, atom) phases comes from two:
//
//   records    (x, y, z, -) / (mu_x, mu_y, mu_z, -) per atom, float64 block partials of sum_j mu_j        dipole_step_records_kernel
//   structure  S_c(k) = sum_j (mu_j.k) cos(k r_j), S_s likewise, over the COMPACTED k list                dipole_structure_kernel (dipole.hip)
//   atoms      per (atom, k) one phase: field_i += G k (c S_c + s S_s), bracket_i += G (mu_i.k)(c S_s - s S_c) k
//                                                                                                          dipole_step_atom_kernel
//   rows       per atom a over both roles of its row: c sum_e T(vec_e) mu_o and c sum_e grad_vec (mu_a.T(vec_e).mu_o),
//              vec_e = r_o - r_a + S'_e cell (role-adjusted shift); with CELL sum_p S_p (x) dE/dvec_p over role i
//                                                                                                          dipole_step_rows_kernel
//   cell k     per k: d/dk of 1/2 G |S|^2, contracted with k to 3 x 3, and 1/2 G |S|^2 itself              dipole_step_cellk_kernel
//   finish     16 lanes per atom over the slices: dE/dmu_i = field_i / V - self mu_i + bg/V sum_j mu_j + rows;
//              F_i = -bracket_i / V + rows; float64 block partials of 1/2 mu_i . dE/dmu_i                  dipole_step_finish_kernel
//   final      one block: E, and dE/dcell = rows - A^-T W / V - (E_k + E_bg) A^-T  with W = sum_k (dE_raw/dk) (x) k
//              (k = 2 pi f A^-T, so sum_k dE/dk . dk/dA = -A^-T W; 1/V gives the second term)              dipole_step_final_kernel
//
// The compacted list holds one of every +-k pair (the two terms of every sum above are equal) with the multiplicity folded into
// G and dG by the caller.  No atomics: every sum has a fixed order, results are the same bits run after run.
//
// mipme_dipole_cell_step is the same step with the CELL as an input of every call: dipole_cell_step_prep_kernel in the place of
// records (and of the caller's tables: k, G, dG, A^-1, 1/V from the nine values of the device cell), dipole_cell_step_finish_kernel
// and dipole_cell_step_final_kernel in the place of finish and final; see the section behind the final kernel.
//
// The kernels of this file are wrappers: each passes its arguments and blockIdx to the body of dipole_step_bodies.h that
// dipole_batch.hip calls for the same launch (the form of ewald_step.hip), so every formula of the step is written once for the
// three entry points.  The two finish kernels are the exception and keep their own text; the comment above each says why.
#include <cmath>

#include "dipole_device.h"
#include "dipole_step_bodies.h"
#include "ewald_step_device.h"  // kEsGeom: the geometry record the step that follows its cell shares with the Ewald step
#include "host.h"
#include "step_device.h"

namespace mipme {

constexpr int kDsBlock = kStepBlock;   // (the name the kernels and launches of this file use)
constexpr int64_t kDsMinSlice = 1024;  // k-vectors per slice at least (4 per thread)

// work: the layout of step_device.h without a head: [mu partials 3 per atom block] ... [row results 6 N][slice partials 6 N S]
static StepWork ds_work_layout(int64_t N, int64_t K, bool cell, void* base) {
  return step_work_layout(N, K, cell, base, 0, 3, 6, kDsMinSlice);
}

// ---- 1. records ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kDsBlock) void dipole_step_records_kernel(int64_t N, const T* __restrict__ pos, const T* __restrict__ mu,
                                                                      AtomRecord<T>* __restrict__ recp,
                                                                      AtomRecord<T>* __restrict__ recm, double* __restrict__ mu_part) {
  ds_records_body<T>(N, blockIdx.x, pos, mu, recp, recm, mu_part);
}

// ---- 2. fused atom kernel: block (i, slice), atom i against the k-vectors [slice * chunk, (slice + 1) * chunk) ---------------
// part[(slice N + i) 6 + c]: c < 3 the field sum_k G k (c S_c + s S_s), c >= 3 the bracket sum_k G (mu_i.k)(c S_s - s S_c) k
template <typename T>
__global__ __launch_bounds__(kDsBlock) void dipole_step_atom_kernel(int64_t K, int64_t chunk, const AtomRecord<T>* __restrict__ recp,
                                                                   const AtomRecord<T>* __restrict__ recm,
                                                                   const T* __restrict__ kvec, const T* __restrict__ G,
                                                                   const T* __restrict__ Sc, const T* __restrict__ Ss,
                                                                   T* __restrict__ part) {
  ds_atom_body<T>(blockIdx.x, blockIdx.y, gridDim.x, K, chunk, recp, recm, kvec, G, Sc, Ss, part);
}

// ---- 3. dipole pair rows -------------------------------------------------------------------------------------------------
// 16 lanes per atom row, 4 rows per wavefront; the 7^3 table of Cartesian shift vectors in LDS; per entry one word
// (other | code << 22) and two 16-byte record gathers (position, dipole of the partner).
//   row_out[6 a + c]     = scale sum_e (T(vec_e) mu_o)_c                      c < 3    (scale = prefactor, or prefactor / 2 for a
//   row_out[6 a + 3 + c] = scale sum_e (grad_vec (mu_a.T(vec_e).mu_o))_c                full list; both roles)
//   cell_part[9 b + 3 m + n] = scale sum over the role-i entries of the rows of block b of S_m (grad_vec ...)_n    (CELL, float64)
template <typename T, bool EXCL, bool CELL>
__global__ __launch_bounds__(kDsBlock) void dipole_step_rows_kernel(DipPot<T> P, int64_t N, const int* __restrict__ row_ptr,
                                                                   const int* __restrict__ ent32,
                                                                   const AtomRecord<T>* __restrict__ recp,
                                                                   const AtomRecord<T>* __restrict__ recm, const T* __restrict__ cell,
                                                                   T scale, T* __restrict__ row_out, double* __restrict__ cell_part) {
  ds_rows_body<T, EXCL, CELL>(P, N, blockIdx.x, row_ptr, ent32, recp, recm, cell, scale, row_out, cell_part);
}

// ---- 4. per-k cell gradient: 32 lanes per k-vector, positions and dipoles streamed through LDS ------------------------------
// With g = mu, T = S:  gk = dE_raw/dk = dG |S|^2 k + G sum_i [ mu_i (c S_c + s S_s) + r_i (mu_i.k)(c S_s - s S_c) ],  E_raw = 1/2 sum G |S|^2.
//   k_part[10 b + 3 a + n] = sum over the k-vectors of block b of gk_a k_n;   k_part[10 b + 9] = sum 1/2 G |S|^2        (float64)
template <typename T>
__global__ __launch_bounds__(kDsBlock) void dipole_step_cellk_kernel(int64_t N, int64_t K, const T* __restrict__ pos,
                                                                    const T* __restrict__ mu, const T* __restrict__ kvec,
                                                                    const T* __restrict__ G, const T* __restrict__ dG,
                                                                    const T* __restrict__ Sc, const T* __restrict__ Ss,
                                                                    double* __restrict__ k_part) {
  ds_cellk_body<T>(N, K, blockIdx.x, pos, mu, kvec, G, dG, Sc, Ss, k_part);
}

// ---- 5. finish -----------------------------------------------------------------------------------------------------------
// 16 lanes per atom: lane l adds the slices l, l + 16, ... in that order, then the 16 lanes are added by the shuffle tree of the
// rows (with few atoms there are hundreds of slices: one thread per atom would walk them one dependent load after the other)
// Own text, not a body: as a wrapper of one shared finish body its fp32 instance failed the BITS condition.  The compiler fuses
// other products of inv_vol f - self mu + bg/V M into multiply-adds in the inlined body (502 instructions for 499), and 38 of the
// 105 fp32 lines of tools/step_bits.py (12 E, 26 dE/dmu) were no longer the parent's; fp64 was equal (docs/HISTORY.md).
template <typename T>
__global__ __launch_bounds__(kDsBlock) void dipole_step_finish_kernel(int64_t N, int n_slices, T inv_vol, T self_term, T bg_over_v,
                                                                     const AtomRecord<T>* __restrict__ recm,
                                                                     const T* __restrict__ part, const T* __restrict__ row_out,
                                                                     const double* __restrict__ mu_part, int64_t n_mu_blocks,
                                                                     T* __restrict__ forces, T* __restrict__ grad_mu,
                                                                     double* __restrict__ e_part) {
  __shared__ double red[kStepWaves];
  double M[3] = {0.0, 0.0, 0.0};
  if (bg_over_v != T(0)) {  // (uniform) sum_j mu_j, the same fixed order in every block
#pragma unroll
    for (int c = 0; c < 3; ++c) M[c] = step_strided_sum(mu_part, n_mu_blocks, 3, c, red);
  }
  const int sub = threadIdx.x % 16;
  const int64_t a = int64_t(blockIdx.x) * kStepRowsPerBlock + threadIdx.x / 16;
  const bool valid = a < N;
  T f0 = T(0), f1 = T(0), f2 = T(0), b0 = T(0), b1 = T(0), b2 = T(0);
  if (valid)
    for (int s = sub; s < n_slices; s += 16) {
      const T* __restrict__ p = part + (int64_t(s) * N + a) * 6;
      f0 += p[0], f1 += p[1], f2 += p[2];
      b0 += p[3], b1 += p[4], b2 += p[5];
    }
  f0 = row_sum(f0), f1 = row_sum(f1), f2 = row_sum(f2);
  b0 = row_sum(b0), b1 = row_sum(b1), b2 = row_sum(b2);
  double e = 0.0;
  if (valid && sub == 0) {
    const T f[3] = {f0, f1, f2}, b[3] = {b0, b1, b2};
    const AtomRecord<T> m = recm[a];
    const T mv[3] = {m.x, m.y, m.z};
    const T* __restrict__ r = row_out + 6 * a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T d = (inv_vol * f[c] - self_term * mv[c] + bg_over_v * T(M[c])) + r[c];
      grad_mu[3 * a + c] = d;
      forces[3 * a + c] = r[3 + c] - inv_vol * b[c];
      e += 0.5 * double(mv[c]) * double(d);
    }
  }
  e = block_sum<kStepWaves>(e, red);
  if (threadIdx.x == 0) e_part[blockIdx.x] = e;
}

// ---- 6. final: one block ----------------------------------------------------------------------------------------------------
template <typename T, bool CELL>
__global__ __launch_bounds__(kDsBlock) void dipole_step_final_kernel(int64_t n_e_blocks, const double* __restrict__ e_part,
                                                                    T* __restrict__ energy, int64_t n_row_blocks,
                                                                    const double* __restrict__ row_cell, int64_t n_k_blocks,
                                                                    const double* __restrict__ k_cell, int64_t n_mu_blocks,
                                                                    const double* __restrict__ mu_part, double inv_vol, double bg,
                                                                    const T* __restrict__ inv_cell, T* __restrict__ grad_cell) {
  ds_final_core<T, CELL, T>(n_e_blocks, e_part, energy, n_row_blocks, row_cell, n_k_blocks, k_cell, n_mu_blocks, mu_part, &inv_vol, bg,
                            inv_cell, false, grad_cell);
}

// ---- the step that follows its cell (mipme_dipole_cell_step) ------------------------------------------------------------------
// Everything that depends on the cell's values comes from the nine values of the device cell in every call: prep takes the place
// of the records launch and also writes the k table, the geometry record (the head of the work area: the record of the Ewald
// step, kEsGeom doubles) and the status word; finish and final read 1/V and A^-1 from that record.  Structure, atoms, rows and
// cell k are the kernels above.  Prep and final are wrappers of ds_prep_body and ds_final_body (the latter shares ds_final_core
// with the final kernel above); finish keeps its own text.

// work: ds_work_layout behind the geometry record
static StepWork dcs_work_layout(int64_t N, int64_t K, bool cell, void* base) {
  return step_work_layout(N, K, cell, base, kEsGeom, 3, 6, kDsMinSlice);
}
static int64_t dcs_table_blocks(int64_t K) {
  return std::max<int64_t>(1, (K + kDsBlock - 1) / kDsBlock);  // (block 0 writes the geometry: at least one)
}

// ---- 1'. prep: k table and geometry (blocks blockIdx.x < n_table_blocks), records and dipole partials (the blocks behind them) ---
// lr_wavelength <= 0 (a potential without smearing): bit 0 of the status word is never set
template <typename T>
__global__ __launch_bounds__(kDsBlock) void dipole_cell_step_prep_kernel(KPot kp, int64_t N, int64_t K, int n_table_blocks,
                                                                        const T* __restrict__ cell, const int* __restrict__ freq,
                                                                        const int* __restrict__ mult, int ns0, int ns1, int ns2,
                                                                        double lr_wavelength, const T* __restrict__ pos,
                                                                        const T* __restrict__ mu, T* __restrict__ kvec,
                                                                        T* __restrict__ G, T* __restrict__ dG,
                                                                        AtomRecord<T>* __restrict__ recp,
                                                                        AtomRecord<T>* __restrict__ recm, double* __restrict__ mu_part,
                                                                        double* __restrict__ geom, int* __restrict__ status) {
  ds_prep_body<T>(kp, N, K, n_table_blocks, int(blockIdx.x), cell, freq, mult, ns0, ns1, ns2, lr_wavelength, pos, mu, kvec, G, dG, recp,
                  recm, mu_part, geom, status);
}

// ---- 5'. finish: dipole_step_finish_kernel with 1/V and bg/V from the geometry record ----------------------------------------------
// Own text, not a wrapper of ds_finish_body (which holds the same text for the batch): inlined, its fp32 instance failed the BITS
// condition for the reason given above dipole_step_finish_kernel (508 instructions for 501): 74 of the 270 fp32 lines of
// tools/step_bits.py --cell-step (22 E, 52 dE/dmu) were no longer the parent's; fp64 was equal.
template <typename T>
__global__ __launch_bounds__(kDsBlock) void dipole_cell_step_finish_kernel(int64_t N, int n_slices, T self_term, double background,
                                                                          const double* __restrict__ geom,
                                                                          const AtomRecord<T>* __restrict__ recm,
                                                                          const T* __restrict__ part, const T* __restrict__ row_out,
                                                                          const double* __restrict__ mu_part, int64_t n_mu_blocks,
                                                                          T* __restrict__ forces, T* __restrict__ grad_mu,
                                                                          double* __restrict__ e_part) {
  __shared__ double red[kStepWaves];
  const double inv_vol_d = geom[9];
  const T inv_vol = T(inv_vol_d), bg_over_v = T(background * inv_vol_d);
  double M[3] = {0.0, 0.0, 0.0};
  if (background != 0.0) {  // (uniform, and the same for every cell) sum_j mu_j, the same fixed order in every block
#pragma unroll
    for (int c = 0; c < 3; ++c) M[c] = step_strided_sum(mu_part, n_mu_blocks, 3, c, red);
  }
  const int sub = threadIdx.x % 16;
  const int64_t a = int64_t(blockIdx.x) * kStepRowsPerBlock + threadIdx.x / 16;
  const bool valid = a < N;
  T f0 = T(0), f1 = T(0), f2 = T(0), b0 = T(0), b1 = T(0), b2 = T(0);
  if (valid)
    for (int s = sub; s < n_slices; s += 16) {
      const T* __restrict__ p = part + (int64_t(s) * N + a) * 6;
      f0 += p[0], f1 += p[1], f2 += p[2];
      b0 += p[3], b1 += p[4], b2 += p[5];
    }
  f0 = row_sum(f0), f1 = row_sum(f1), f2 = row_sum(f2);
  b0 = row_sum(b0), b1 = row_sum(b1), b2 = row_sum(b2);
  double e = 0.0;
  if (valid && sub == 0) {
    const T f[3] = {f0, f1, f2}, b[3] = {b0, b1, b2};
    const AtomRecord<T> m = recm[a];
    const T mv[3] = {m.x, m.y, m.z};
    const T* __restrict__ r = row_out + 6 * a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T d = (inv_vol * f[c] - self_term * mv[c] + bg_over_v * T(M[c])) + r[c];
      grad_mu[3 * a + c] = d;
      forces[3 * a + c] = r[3 + c] - inv_vol * b[c];
      e += 0.5 * double(mv[c]) * double(d);
    }
  }
  e = block_sum<kStepWaves>(e, red);
  if (threadIdx.x == 0) e_part[blockIdx.x] = e;
}

// ---- 6'. final: dipole_step_final_kernel with 1/V and A^-1 from the geometry record; NaN for a bad cell ---------------------------
template <typename T, bool CELL>
__global__ __launch_bounds__(kDsBlock) void dipole_cell_step_final_kernel(int64_t n_e_blocks, const double* __restrict__ e_part,
                                                                         T* __restrict__ energy, int64_t n_row_blocks,
                                                                         const double* __restrict__ row_cell, int64_t n_k_blocks,
                                                                         const double* __restrict__ k_cell, int64_t n_mu_blocks,
                                                                         const double* __restrict__ mu_part, double bg,
                                                                         const double* __restrict__ geom, T* __restrict__ grad_cell) {
  ds_final_body<T, CELL>(n_e_blocks, e_part, energy, n_row_blocks, row_cell, n_k_blocks, k_cell, n_mu_blocks, mu_part, bg, geom,
                         grad_cell);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// Args: mipme_dipole_step_args_t or mipme_dipole_cell_step_args_t (the fields read here have the same names in both)
template <typename T, bool EXCL, typename Args>
static void dipole_step_rows_launch(hipStream_t st, const Args& a, const DipPot<T>& dp, const StepWork& w,
                                    const AtomRecord<T>* recp, const AtomRecord<T>* recm) {
  const unsigned blocks = unsigned((a.n_atoms + kStepRowsPerBlock - 1) / kStepRowsPerBlock);
  const T scale = T(a.full_list ? 0.5 : 1.0) * dp.pref;
  if (a.cell_gradient)
    dipole_step_rows_kernel<T, EXCL, true><<<blocks, kDsBlock, 0, st>>>(dp, a.n_atoms, (const int*)a.row_ptr, (const int*)a.entries,
                                                                       recp, recm, (const T*)a.cell, scale, (T*)w.row_out, w.row_cell);
  else
    dipole_step_rows_kernel<T, EXCL, false><<<blocks, kDsBlock, 0, st>>>(dp, a.n_atoms, (const int*)a.row_ptr, (const int*)a.entries,
                                                                        recp, recm, (const T*)a.cell, scale, (T*)w.row_out, nullptr);
}

template <typename T>
static int dipole_step_t(const mipme_dipole_step_args_t& a, const DipPot<T>& dp) {
  hipStream_t st = (hipStream_t)a.stream;
  const int64_t N = a.n_atoms, K = a.n_k;
  const bool cell = a.cell_gradient != 0;
  const StepWork w = ds_work_layout(N, K, cell, a.work);
  AtomRecord<T>* recp = (AtomRecord<T>*)a.records;
  AtomRecord<T>* recm = recp + N;
  int rc;
  dipole_step_records_kernel<T><<<unsigned(w.n_atom_blocks), kDsBlock, 0, st>>>(N, (const T*)a.positions, (const T*)a.dipoles, recp,
                                                                               recm, w.atom_part);
  MIPME_LAUNCH_CHECK();
  if (K > 0) {
    if ((rc = mipme_dipole_structure(a.stream, a.dtype, N, K, a.positions, a.dipoles, a.kvectors, a.G, cell ? a.dG : nullptr, a.s_cos,
                                     a.s_sin)))
      return rc;
    const int64_t chunk = (K + w.n_slices - 1) / w.n_slices;
    dipole_step_atom_kernel<T><<<dim3(unsigned(N), unsigned(w.n_slices)), kDsBlock, 0, st>>>(
        K, chunk, recp, recm, (const T*)a.kvectors, (const T*)a.G, (const T*)a.s_cos, (const T*)a.s_sin, (T*)w.slice_part);
    MIPME_LAUNCH_CHECK();
  }
  if (dp.mode == 2)
    dipole_step_rows_launch<T, true>(st, a, dp, w, recp, recm);
  else
    dipole_step_rows_launch<T, false>(st, a, dp, w, recp, recm);
  MIPME_LAUNCH_CHECK();
  if (cell && K > 0) {
    dipole_step_cellk_kernel<T><<<unsigned(w.n_k_blocks), kDsBlock, 0, st>>>(N, K, (const T*)a.positions, (const T*)a.dipoles,
                                                                            (const T*)a.kvectors, (const T*)a.G, (const T*)a.dG,
                                                                            (const T*)a.s_cos, (const T*)a.s_sin, w.k_cell);
    MIPME_LAUNCH_CHECK();
  }
  dipole_step_finish_kernel<T><<<unsigned(w.n_fin_blocks), kDsBlock, 0, st>>>(
      N, int(w.n_slices), T(a.inv_volume), T(a.self_term), T(a.background * a.inv_volume), recm, (const T*)w.slice_part,
      (const T*)w.row_out, w.atom_part, w.n_atom_blocks, (T*)a.forces, (T*)a.grad_dipoles, w.e_part);
  MIPME_LAUNCH_CHECK();
  if (cell)
    dipole_step_final_kernel<T, true><<<1, kDsBlock, 0, st>>>(w.n_fin_blocks, w.e_part, (T*)a.energy, w.n_row_blocks, w.row_cell,
                                                             w.n_k_blocks, w.k_cell, w.n_atom_blocks, w.atom_part, a.inv_volume,
                                                             a.background, (const T*)a.inv_cell, (T*)a.grad_cell);
  else
    dipole_step_final_kernel<T, false><<<1, kDsBlock, 0, st>>>(w.n_fin_blocks, w.e_part, (T*)a.energy, 0, nullptr, 0, nullptr, 0,
                                                              nullptr, a.inv_volume, a.background, nullptr, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int dipole_step_run(const mipme_dipole_step_args_t& a) {
  DipPot<T> dp;
  int rc = make_dippot<T>(a.pot, dp);
  if (rc) return rc;
  return dipole_step_t<T>(a, dp);
}

template <typename T>
static int dipole_cell_step_t(const mipme_dipole_cell_step_args_t& a, const DipPot<T>& dp, const KPot& kp) {
  hipStream_t st = (hipStream_t)a.stream;
  const int64_t N = a.n_atoms, K = a.n_k;
  const bool cell = a.cell_gradient != 0;
  const StepWork w = dcs_work_layout(N, K, cell, a.work);
  const int64_t n_table_blocks = dcs_table_blocks(K);
  AtomRecord<T>* recp = (AtomRecord<T>*)a.records;
  AtomRecord<T>* recm = recp + N;
  int rc;
  dipole_cell_step_prep_kernel<T><<<unsigned(n_table_blocks + w.n_atom_blocks), kDsBlock, 0, st>>>(
      kp, N, K, int(n_table_blocks), (const T*)a.cell, (const int*)a.frequencies, (const int*)a.multiplicities, a.ns[0], a.ns[1],
      a.ns[2], a.pot->smearing > 0 ? a.lr_wavelength : 0.0, (const T*)a.positions, (const T*)a.dipoles, (T*)a.kvectors, (T*)a.G,
      cell ? (T*)a.dG : nullptr, recp, recm, w.atom_part, w.head, (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (K > 0) {
    if ((rc = mipme_dipole_structure(a.stream, a.dtype, N, K, a.positions, a.dipoles, a.kvectors, a.G, cell ? a.dG : nullptr, a.s_cos,
                                     a.s_sin)))
      return rc;
    const int64_t chunk = (K + w.n_slices - 1) / w.n_slices;
    dipole_step_atom_kernel<T><<<dim3(unsigned(N), unsigned(w.n_slices)), kDsBlock, 0, st>>>(
        K, chunk, recp, recm, (const T*)a.kvectors, (const T*)a.G, (const T*)a.s_cos, (const T*)a.s_sin, (T*)w.slice_part);
    MIPME_LAUNCH_CHECK();
  }
  if (dp.mode == 2)
    dipole_step_rows_launch<T, true>(st, a, dp, w, recp, recm);
  else
    dipole_step_rows_launch<T, false>(st, a, dp, w, recp, recm);
  MIPME_LAUNCH_CHECK();
  if (cell && K > 0) {
    dipole_step_cellk_kernel<T><<<unsigned(w.n_k_blocks), kDsBlock, 0, st>>>(N, K, (const T*)a.positions, (const T*)a.dipoles,
                                                                            (const T*)a.kvectors, (const T*)a.G, (const T*)a.dG,
                                                                            (const T*)a.s_cos, (const T*)a.s_sin, w.k_cell);
    MIPME_LAUNCH_CHECK();
  }
  dipole_cell_step_finish_kernel<T><<<unsigned(w.n_fin_blocks), kDsBlock, 0, st>>>(
      N, int(w.n_slices), T(a.self_term), a.background, w.head, recm, (const T*)w.slice_part, (const T*)w.row_out, w.atom_part,
      w.n_atom_blocks, (T*)a.forces, (T*)a.grad_dipoles, w.e_part);
  MIPME_LAUNCH_CHECK();
  if (cell)
    dipole_cell_step_final_kernel<T, true><<<1, kDsBlock, 0, st>>>(w.n_fin_blocks, w.e_part, (T*)a.energy, w.n_row_blocks, w.row_cell,
                                                                  w.n_k_blocks, w.k_cell, w.n_atom_blocks, w.atom_part, a.background,
                                                                  w.head, (T*)a.grad_cell);
  else
    dipole_cell_step_final_kernel<T, false><<<1, kDsBlock, 0, st>>>(w.n_fin_blocks, w.e_part, (T*)a.energy, 0, nullptr, 0, nullptr, 0,
                                                                   nullptr, a.background, w.head, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int dipole_cell_step_run(const mipme_dipole_cell_step_args_t& a) {
  DipPot<T> dp;
  int rc = make_dippot<T>(a.pot, dp);
  if (rc) return rc;
  KPot kp{};
  if (a.n_k > 0) {  // the reciprocal-space kernel 4 pi prefactor exp(-sigma^2 k^2 / 2) / k^2 is Coulomb's
    mipme_potential_t coulomb{};
    coulomb.kind = MIPME_COULOMB, coulomb.exponent = 1, coulomb.smearing = a.pot->smearing, coulomb.prefactor = a.pot->prefactor;
    coulomb.exclusion_radius = -1.0, coulomb.exclusion_degree = 1;
    if ((rc = make_kpot(&coulomb, kp))) return rc;
  }
  return dipole_cell_step_t<T>(a, dp, kp);
}

}  // namespace mipme

using namespace mipme;

extern "C" {

// (the entry points of the step that follows its cell come first: templates are instantiated in the order of their first use, and
// with this order the kernels of mipme_dipole_step stay where they were at the end of the code object, byte for byte)
int64_t mipme_dipole_cell_step_work(int64_t n_atoms, int64_t n_k, int cell_gradient) {
  if (n_atoms < 1 || n_atoms > kCompactMaxAtoms || n_k < 0 || n_k > int64_t(kStepKPerBlock) * 0x7fffffff) return 0;
  return dcs_work_layout(n_atoms, n_k, cell_gradient != 0, nullptr).total;
}

int mipme_dipole_cell_step(const mipme_dipole_cell_step_args_t* in) {
  const char* who = "mipme_dipole_cell_step";
  mipme_dipole_cell_step_args_t a;
  int rc = load_args(in, a, MIPME_DIPOLE_CELL_STEP_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  MIPME_REQUIRE(a.dtype == MIPME_F32 || a.dtype == MIPME_F64, "%s: invalid dtype %d", who, int(a.dtype));
  MIPME_REQUIRE(a.pot != nullptr, "%s: dipole descriptor is NULL", who);
  MIPME_REQUIRE(a.n_k >= 0 && a.n_k <= int64_t(kStepKPerBlock) * 0x7fffffff, "%s: n_k must be >= 0, got %lld", who, (long long)a.n_k);
  MIPME_REQUIRE(a.n_k == 0 || a.pot->smearing > 0,
                "%s: n_k is %lld but the potential has no smearing (`smearing` is %g): a direct potential has no reciprocal part",
                who, (long long)a.n_k, a.pot->smearing);
  MIPME_REQUIRE(a.n_k == 0 || (std::isfinite(a.lr_wavelength) && a.lr_wavelength > 0 && a.ns[0] >= 1 && a.ns[1] >= 1 && a.ns[2] >= 1),
                "%s: lr_wavelength must be positive and ns >= 1 (the grid `status` compares with), got %g and (%d, %d, %d)", who,
                a.lr_wavelength, int(a.ns[0]), int(a.ns[1]), int(a.ns[2]));
  MIPME_REQUIRE(!(a.pot->exclusion_radius > 0) || a.pot->exclusion_degree >= 1, "%s: exclusion_degree must be >= 1, got %d", who,
                int(a.pot->exclusion_degree));
  if ((rc = check_step_rows(a.shift_format, a.n_atoms, who))) return rc;
  MIPME_REQUIRE(!a.cell_gradient || a.grad_cell, "%s: cell_gradient needs grad_cell", who);
  MIPME_REQUIRE(!a.cell_gradient || a.n_k == 0 || a.dG, "%s: cell_gradient needs dG (n_k reals of scratch)", who);
  MIPME_REQUIRE(a.status != nullptr, "%s: status is NULL (one int32 on the device, written by every call)", who);
  MIPME_REQUIRE(a.positions && a.dipoles && a.cell && a.row_ptr && a.entries && a.records && a.energy && a.forces && a.grad_dipoles &&
                    a.work && (a.n_k == 0 || (a.frequencies && a.multiplicities && a.kvectors && a.G && a.s_cos && a.s_sin)),
                "%s: NULL required buffer", who);
  DT_SWITCH(a.dtype, dipole_cell_step_run<float>(a), dipole_cell_step_run<double>(a));
}

int64_t mipme_dipole_step_work(int64_t n_atoms, int64_t n_k, int cell_gradient) {
  if (n_atoms < 1 || n_atoms > kCompactMaxAtoms || n_k < 0 || n_k > int64_t(kStepKPerBlock) * 0x7fffffff) return 0;
  return ds_work_layout(n_atoms, n_k, cell_gradient != 0, nullptr).total;
}

int mipme_dipole_step(const mipme_dipole_step_args_t* in) {
  const char* who = "mipme_dipole_step";
  mipme_dipole_step_args_t a;
  int rc = load_args(in, a, MIPME_DIPOLE_STEP_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  MIPME_REQUIRE(a.dtype == MIPME_F32 || a.dtype == MIPME_F64, "%s: invalid dtype %d", who, int(a.dtype));
  MIPME_REQUIRE(a.pot != nullptr, "%s: dipole descriptor is NULL", who);
  MIPME_REQUIRE(!(a.pot->exclusion_radius > 0) || a.pot->exclusion_degree >= 1, "%s: exclusion_degree must be >= 1, got %d", who,
                int(a.pot->exclusion_degree));
  MIPME_REQUIRE(a.n_k >= 0 && a.n_k <= int64_t(kStepKPerBlock) * 0x7fffffff, "%s: n_k must be >= 0, got %lld", who, (long long)a.n_k);
  MIPME_REQUIRE(a.n_k == 0 || a.pot->smearing > 0,
                "%s: n_k is %lld but the potential has no smearing (`smearing` is %g): a direct potential has no reciprocal part",
                who, (long long)a.n_k, a.pot->smearing);
  if ((rc = check_step_rows(a.shift_format, a.n_atoms, who))) return rc;
  MIPME_REQUIRE(std::isfinite(a.inv_volume) && a.inv_volume > 0, "%s: inv_volume must be positive, got %g", who, a.inv_volume);
  MIPME_REQUIRE(!a.cell_gradient || (a.grad_cell && a.inv_cell), "%s: cell_gradient needs grad_cell and inv_cell", who);
  MIPME_REQUIRE(!a.cell_gradient || a.n_k == 0 || a.dG, "%s: cell_gradient needs dG (dG/dk^2 of the compacted k-vectors)", who);
  MIPME_REQUIRE(a.positions && a.dipoles && a.cell && a.row_ptr && a.entries && a.records && a.energy && a.forces && a.grad_dipoles &&
                    a.work && (a.n_k == 0 || (a.kvectors && a.G && a.s_cos && a.s_sin)),
                "%s: NULL required buffer", who);
  DT_SWITCH(a.dtype, dipole_step_run<float>(a), dipole_step_run<double>(a));
}

}  // extern "C"
