// Energy, forces and dE/dq (+ dE/dcell) of point charges by the explicit Ewald sum in ONE step (mipme_ewald_step,
// include/mipme.h): the MD form of EwaldCalculator, every launch on one stream so that the whole step is one captured graph --
// and the first step whose CELL is an input of the replay: everything that depends on the cell's values (k-vectors, G, dG/dk^2,
// A^-1, 1/V, the Cartesian shift vectors) is rebuilt on the device from the nine values of the cell buffer in every call.
//
// E = sum_a q_a V_a is quadratic in the charges, so dE/dq_a = lr_a + c sum_e q_o v_SR(d_e) over both roles of the row of a
// (c = 1, or 1/2 for a full list: V plus the transposed pair half) and E = 1/2 sum_a q_a dE/dq_a.  With S the structure factors
// of the charges and the COMPACTED k list (one of every +-k pair, the multiplicity folded into G and dG; k = 0 left out):
//
//   prep       k blocks: A^-T, det from the device cell (every thread inverts the 3 x 3 itself), k = 2 pi F A^-T,
//              G = mult v_LR(k^2), dG = mult dv_LR/dk^2 per compacted frequency; the geometry record and the status word.
//              atom blocks: records (x, y, z, q), float64 block partials of Q = sum q                     ewald_step_prep_kernel
//   structure  S_c(k) = sum_j q_j cos(k r_j), S_s likewise, with the phase function of the launches below  ewald_step_structure_kernel
//   atoms      per (atom, k slice), one phase per (atom, k): phi_a += G (c S_c + s S_s), bracket_a += G k (c S_s - s S_c)
//                                                                                                          ewald_step_atom_kernel
//   rows       per atom a over both roles of its row: c sum_e q_o v_SR(d_e) and c q_a sum_e q_o v_SR'(d_e)/d_e u_e,
//              u_e = r_o - r_a + S'_e cell (role-adjusted shift, table built from the DEVICE cell); with CELL
//              sum_p S_p (x) dE/du_p over role i                                                            ewald_step_rows_kernel
//   cell k     per k: gk = dG |S|^2 k + G sum_j q_j r_j (c S_s - s S_c), contracted with k to 3 x 3, and 1/2 G |S|^2
//                                                                                                          ewald_step_cellk_kernel
//   finish     16 lanes per atom over the slices: dE/dq_a = phi_a / V - self q_a - 2 bg Q / V + rows;
//              F_a = rows - q_a bracket_a / V; float64 block partials of 1/2 q_a dE/dq_a                  ewald_step_finish_kernel
//   final      one block: E, and dE/dcell = rows - A^-T W / V - (E_k + E_bg) A^-T  with W = sum_k gk (x) k
//              (k = 2 pi F A^-T, so sum_k dE/dk . dk/dA = -A^-T W; the 1/V factors give the last term)     ewald_step_final_kernel
//
// bg = background term minus half the k = 0 limit of v_LR (non-zero for p > 3, where the eager sum keeps its k = 0 term): both
// are a constant times Q / V per atom.  No atomics and no workgroup that waits for another: every cross-block sum is float64
// block partials added in index order by a later launch, so equal inputs give equal bits, in fp32 too.
//
// Each of the seven computations is written once, as a body in ewald_step_bodies.h (es_prep_body ... es_final_body); the kernels
// below hand their body the arguments of the one system and the block index of the grid, those of ewald_batch.hip the slices of
// a frame and its local block index.
#include <cmath>

#include "ewald_step_bodies.h"
#include "ewald_step_device.h"
#include "host.h"

namespace mipme {

// ---- the kernels: the bodies of ewald_step_bodies.h with the arguments of one system and the block index of the grid -------
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_step_prep_kernel(KPot kp, int64_t N, int64_t K, int n_table_blocks,
                                                                  const T* __restrict__ cell, const int* __restrict__ freq,
                                                                  const int* __restrict__ mult, int ns0, int ns1, int ns2,
                                                                  double lr_wavelength, const T* __restrict__ pos,
                                                                  const T* __restrict__ q, T* __restrict__ kvec, T* __restrict__ G,
                                                                  T* __restrict__ dG, AtomRecord<T>* __restrict__ rec,
                                                                  double* __restrict__ q_part, double* __restrict__ geom,
                                                                  int* __restrict__ status) {
  es_prep_body<T>(kp, N, K, n_table_blocks, int(blockIdx.x), cell, freq, mult, ns0, ns1, ns2, lr_wavelength, pos, q, kvec, G, dG, rec,
                  q_part, geom, status);
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_step_structure_kernel(int64_t N, int64_t K, const AtomRecord<T>* __restrict__ rec,
                                                                       const T* __restrict__ kvec, T* __restrict__ Sc,
                                                                       T* __restrict__ Ss) {
  es_structure_body<T>(N, K, int64_t(blockIdx.x), rec, kvec, Sc, Ss);
}

// block (i, slice) of an N x n_slices grid
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_step_atom_kernel(int64_t K, int64_t chunk, const AtomRecord<T>* __restrict__ rec,
                                                                  const T* __restrict__ kvec, const T* __restrict__ G,
                                                                  const T* __restrict__ Sc, const T* __restrict__ Ss,
                                                                  T* __restrict__ part) {
  es_atom_body<T>(int64_t(blockIdx.x), int64_t(blockIdx.y), int64_t(gridDim.x), K, chunk, rec, kvec, G, Sc, Ss, part);
}

template <typename T, int PFAST, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_step_rows_kernel(SRPot sp, FastRS cf, int64_t N, const int* __restrict__ row_ptr,
                                                                  const int* __restrict__ ent32,
                                                                  const AtomRecord<T>* __restrict__ rec, const T* __restrict__ cell,
                                                                  T scale, T* __restrict__ row_out, double* __restrict__ cell_part) {
  es_rows_body<T, PFAST, CELL>(sp, cf, N, int64_t(blockIdx.x), row_ptr, ent32, rec, cell, scale, row_out, cell_part);
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_step_cellk_kernel(int64_t N, int64_t K, const AtomRecord<T>* __restrict__ rec,
                                                                   const T* __restrict__ kvec, const T* __restrict__ G,
                                                                   const T* __restrict__ dG, const T* __restrict__ Sc,
                                                                   const T* __restrict__ Ss, double* __restrict__ k_part) {
  es_cellk_body<T>(N, K, int64_t(blockIdx.x), rec, kvec, G, dG, Sc, Ss, k_part);
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_step_finish_kernel(int64_t N, int n_slices, T self_c, double two_bg,
                                                                    const double* __restrict__ geom,
                                                                    const AtomRecord<T>* __restrict__ rec, const T* __restrict__ part,
                                                                    const T* __restrict__ row_out, const double* __restrict__ q_part,
                                                                    int64_t n_q_blocks, T* __restrict__ forces,
                                                                    T* __restrict__ grad_q, double* __restrict__ e_part) {
  es_finish_body<T>(N, n_slices, int64_t(blockIdx.x), self_c, two_bg, geom, rec, part, row_out, q_part, n_q_blocks, forces, grad_q,
                    e_part);
}

// one block
template <typename T, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_step_final_kernel(int64_t n_e_blocks, const double* __restrict__ e_part,
                                                                   T* __restrict__ energy, int64_t n_row_blocks,
                                                                   const double* __restrict__ row_cell, int64_t n_k_blocks,
                                                                   const double* __restrict__ k_cell, int64_t n_q_blocks,
                                                                   const double* __restrict__ q_part, double bg,
                                                                   const double* __restrict__ geom, T* __restrict__ grad_cell) {
  es_final_body<T, CELL>(n_e_blocks, e_part, energy, n_row_blocks, row_cell, n_k_blocks, k_cell, n_q_blocks, q_part, bg, geom,
                         grad_cell);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T>
static int ewald_step_t(const mipme_ewald_step_args_t& a, const KPot& kp, const SRPot& sp) {
  hipStream_t st = (hipStream_t)a.stream;
  const int64_t N = a.n_atoms, K = a.n_k;
  const bool cell = a.cell_gradient != 0;
  const EsWork w = es_work_layout(N, K, cell, a.work);
  AtomRecord<T>* rec = (AtomRecord<T>*)a.records;
  const EsTerms t = es_terms(a.pot, kp, sp);
  ewald_step_prep_kernel<T><<<unsigned(w.n_table_blocks + w.n_atom_blocks), kEsBlock, 0, st>>>(
      kp, N, K, int(w.n_table_blocks), (const T*)a.cell, (const int*)a.frequencies, (const int*)a.multiplicities, a.ns[0], a.ns[1],
      a.ns[2], a.lr_wavelength, (const T*)a.positions, (const T*)a.charges, (T*)a.kvectors, (T*)a.G, cell ? (T*)a.dG : nullptr, rec,
      w.q_part, w.geom, (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (K > 0) {
    ewald_step_structure_kernel<T><<<unsigned((K + kEsKPerBlock - 1) / kEsKPerBlock), kEsBlock, 0, st>>>(
        N, K, rec, (const T*)a.kvectors, (T*)a.s_cos, (T*)a.s_sin);
    MIPME_LAUNCH_CHECK();
    const int64_t chunk = (K + w.n_slices - 1) / w.n_slices;
    ewald_step_atom_kernel<T><<<dim3(unsigned(N), unsigned(w.n_slices)), kEsBlock, 0, st>>>(
        K, chunk, rec, (const T*)a.kvectors, (const T*)a.G, (const T*)a.s_cos, (const T*)a.s_sin, (T*)w.slice_part);
    MIPME_LAUNCH_CHECK();
  }
  es_rows_dispatch(sp, cell, [&](auto pfast, auto with_cell) {
    ewald_step_rows_kernel<T, pfast(), with_cell()><<<unsigned(w.n_fin_blocks), kEsBlock, 0, st>>>(
        sp, t.cf, N, (const int*)a.row_ptr, (const int*)a.entries, rec, (const T*)a.cell, T(a.full_list ? 0.5 : 1.0), (T*)w.row_out,
        with_cell() ? w.row_cell : nullptr);
  });
  MIPME_LAUNCH_CHECK();
  if (cell && K > 0) {
    ewald_step_cellk_kernel<T><<<unsigned(w.n_k_blocks), kEsBlock, 0, st>>>(N, K, rec, (const T*)a.kvectors, (const T*)a.G,
                                                                           (const T*)a.dG, (const T*)a.s_cos, (const T*)a.s_sin,
                                                                           w.k_cell);
    MIPME_LAUNCH_CHECK();
  }
  ewald_step_finish_kernel<T><<<unsigned(w.n_fin_blocks), kEsBlock, 0, st>>>(N, int(w.n_slices), T(t.self_c), 2.0 * t.bg, w.geom, rec,
                                                                            (const T*)w.slice_part, (const T*)w.row_out, w.q_part,
                                                                            w.n_atom_blocks, (T*)a.forces, (T*)a.grad_charges,
                                                                            w.e_part);
  MIPME_LAUNCH_CHECK();
  if (cell)
    ewald_step_final_kernel<T, true><<<1, kEsBlock, 0, st>>>(w.n_fin_blocks, w.e_part, (T*)a.energy, w.n_row_blocks, w.row_cell,
                                                            w.n_k_blocks, w.k_cell, w.n_atom_blocks, w.q_part, t.bg, w.geom,
                                                            (T*)a.grad_cell);
  else
    ewald_step_final_kernel<T, false><<<1, kEsBlock, 0, st>>>(w.n_fin_blocks, w.e_part, (T*)a.energy, 0, nullptr, 0, nullptr, 0, nullptr,
                                                             t.bg, w.geom, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_ewald_step_work(int64_t n_atoms, int64_t n_k, int cell_gradient) {
  if (n_atoms < 1 || n_atoms > kCompactMaxAtoms || n_k < 0 || n_k > kEsMaxK) return 0;
  return es_work_layout(n_atoms, n_k, cell_gradient != 0, nullptr).total;
}

int mipme_ewald_step(const mipme_ewald_step_args_t* in) {
  const char* who = "mipme_ewald_step";
  mipme_ewald_step_args_t a;
  int rc = load_args(in, a, MIPME_EWALD_STEP_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  if ((rc = check_ewald_pot(a.dtype, a.pot, who))) return rc;
  MIPME_REQUIRE(a.n_k >= 0 && a.n_k <= kEsMaxK, "%s: n_k must be >= 0, got %lld", who, (long long)a.n_k);
  if ((rc = check_step_rows(a.shift_format, a.n_atoms, who))) return rc;
  MIPME_REQUIRE(std::isfinite(a.lr_wavelength) && a.lr_wavelength > 0 && a.ns[0] >= 1 && a.ns[1] >= 1 && a.ns[2] >= 1,
                "%s: lr_wavelength must be positive and ns >= 1 (the grid `status` compares with), got %g and (%d, %d, %d)", who,
                a.lr_wavelength, int(a.ns[0]), int(a.ns[1]), int(a.ns[2]));
  MIPME_REQUIRE(!a.cell_gradient || a.grad_cell, "%s: cell_gradient needs grad_cell", who);
  MIPME_REQUIRE(!a.cell_gradient || a.n_k == 0 || a.dG, "%s: cell_gradient needs dG (n_k reals of scratch)", who);
  MIPME_REQUIRE(a.positions && a.charges && a.cell && a.row_ptr && a.entries && a.records && a.energy && a.forces && a.grad_charges &&
                    a.status && a.work &&
                    (a.n_k == 0 || (a.frequencies && a.multiplicities && a.kvectors && a.G && a.s_cos && a.s_sin)),
                "%s: NULL required buffer", who);
  KPot kp;
  SRPot sp;
  if ((rc = make_kpot(a.pot, kp)) || (rc = make_srpot(a.pot, sp))) return rc;
  DT_SWITCH(a.dtype, ewald_step_t<float>(a, kp, sp), ewald_step_t<double>(a, kp, sp));
}

}  // extern "C"
