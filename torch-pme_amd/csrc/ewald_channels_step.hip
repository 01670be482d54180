// The Ewald step of ewald_step.hip for SEVERAL charge channels in ONE step (mipme_ewald_channels_step, include/mipme.h): (N, C)
// charges, 2 <= C <= 8, the channels independent systems of charges on the same atoms, cell, k grid and pair list -- the latent
// or learned charges of a model, several per atom.  E = sum_a sum_c q_ac V_ac, F = -dE/dr, dE/dq (N, C) and dE/dcell, from the
// same seven launches on one stream as the single-channel step, the cell an input of every replay.
//
// The expensive work of the step does not depend on the channel: per (atom, k) the phase, formed and reduced in double in float
// too, and its sincos; per pair entry the shift lookup, the distance and the pair function.  C single-channel steps repeat all
// of it C times; here it is done once and a channel adds a few FMAs.  With S^c the structure factor of channel c:
//
//   prep       the k table, geometry record and status of ewald_step.hip (its body); records (x, y, z, 0); float64 block
//              partials of Q_c = sum_a q_ac per channel                                              ewald_channels_step_prep_kernel
//   structure  S_c^c(k), S_s^c(k) for every channel from one phase per (k, atom), positions and charges of a tile in LDS
//                                                                                                ewald_channels_step_structure_kernel
//   atoms      per (atom, k slice), one phase per (atom, k): phi_c += G (c S_c^c + s S_s^c) per channel and THREE bracket sums
//              G k (c A_s - s A_c) with A_s = sum_c q_ac S_s^c, A_c likewise                        ewald_channels_step_atom_kernel
//   rows       per entry one shift, distance and pair function; pot_c += q_oc v per channel and ONE force weight
//              (sum_c q_ac q_oc) v'/d for the pair force and the role-i cell partial                 ewald_channels_step_rows_kernel
//   cell k     per k: gk = dG |S|^2 k + G sum_j r_j (c A_s - s A_c) with |S|^2 = sum_c |S^c|^2      ewald_channels_step_cellk_kernel
//   finish     dE/dq_ac = phi_c / V - self q_ac - 2 bg Q_c / V + pot_c; F_a = rows - bracket_a / V; float64 block partials of
//              1/2 sum_c q_ac dE/dq_ac                                                             ewald_channels_step_finish_kernel
//   final      E and dE/dcell; the 1/V term is (E_k - bg sum_c Q_c^2) / V: a channel sees its own background only
//                                                                                                  ewald_channels_step_final_kernel
//
// No atomics and no workgroup that waits for another: every cross-block sum is float64 block partials added in index order by a
// later launch, so equal inputs give equal bits.  Nothing launched depends on the cell's values.  Each computation is written
// once, as a body in ewald_channels_bodies.h; how the channels stay in registers (capacities 2, 4 and 8) is described there.
#include <cmath>

#include "ewald_channels_bodies.h"
#include "ewald_step_device.h"
#include "host.h"

namespace mipme {

// ---- the kernels: the bodies of ewald_channels_bodies.h with the arguments of one system and the block index of the grid ----
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_prep_kernel(KPot kp, int C, int64_t N, int64_t K, int n_table_blocks,
                                                                           const T* __restrict__ cell, const int* __restrict__ freq,
                                                                           const int* __restrict__ mult, int ns0, int ns1, int ns2,
                                                                           double lr_wavelength, const T* __restrict__ pos,
                                                                           const T* __restrict__ q, T* __restrict__ kvec,
                                                                           T* __restrict__ G, T* __restrict__ dG,
                                                                           AtomRecord<T>* __restrict__ rec, double* __restrict__ q_part,
                                                                           double* __restrict__ geom, int* __restrict__ status) {
  ec_prep_body<T>(kp, C, N, K, n_table_blocks, int(blockIdx.x), cell, freq, mult, ns0, ns1, ns2, lr_wavelength, pos, q, kvec, G, dG,
                  rec, q_part, geom, status);
}

template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_structure_kernel(int C, int64_t N, int64_t K,
                                                                                const AtomRecord<T>* __restrict__ rec,
                                                                                const T* __restrict__ q, const T* __restrict__ kvec,
                                                                                T* __restrict__ Sc, T* __restrict__ Ss) {
  ec_structure_body<T, CAP>(C, N, K, int64_t(blockIdx.x), rec, q, kvec, Sc, Ss);
}

// block (i, slice) of an N x n_slices grid
template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_atom_kernel(int C, int64_t K, int64_t chunk,
                                                                           const AtomRecord<T>* __restrict__ rec,
                                                                           const T* __restrict__ q, const T* __restrict__ kvec,
                                                                           const T* __restrict__ G, const T* __restrict__ Sc,
                                                                           const T* __restrict__ Ss, T* __restrict__ part) {
  ec_atom_body<T, CAP>(C, int64_t(blockIdx.x), int64_t(blockIdx.y), int64_t(gridDim.x), K, chunk, rec, q, kvec, G, Sc, Ss, part);
}

template <typename T, int CAP, int PFAST, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_rows_kernel(SRPot sp, FastRS cf, int C, int64_t N,
                                                                           const int* __restrict__ row_ptr,
                                                                           const int* __restrict__ ent32,
                                                                           const AtomRecord<T>* __restrict__ rec,
                                                                           const T* __restrict__ q, const T* __restrict__ cell, T scale,
                                                                           T* __restrict__ row_out, double* __restrict__ cell_part) {
  ec_rows_body<T, CAP, PFAST, CELL>(sp, cf, C, N, int64_t(blockIdx.x), row_ptr, ent32, rec, q, cell, scale, row_out, cell_part);
}

template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_cellk_kernel(int C, int64_t N, int64_t K,
                                                                            const AtomRecord<T>* __restrict__ rec,
                                                                            const T* __restrict__ q, const T* __restrict__ kvec,
                                                                            const T* __restrict__ G, const T* __restrict__ dG,
                                                                            const T* __restrict__ Sc, const T* __restrict__ Ss,
                                                                            double* __restrict__ k_part) {
  ec_cellk_body<T, CAP>(C, N, K, int64_t(blockIdx.x), rec, q, kvec, G, dG, Sc, Ss, k_part);
}

template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_finish_kernel(int C, int64_t N, int n_slices, T self_c, double two_bg,
                                                                             const double* __restrict__ geom, const T* __restrict__ q,
                                                                             const T* __restrict__ part, const T* __restrict__ row_out,
                                                                             const double* __restrict__ q_part, int64_t n_q_blocks,
                                                                             T* __restrict__ forces, T* __restrict__ grad_q,
                                                                             double* __restrict__ e_part) {
  ec_finish_body<T, CAP>(C, N, n_slices, int64_t(blockIdx.x), self_c, two_bg, geom, q, part, row_out, q_part, n_q_blocks, forces,
                         grad_q, e_part);
}

// one block
template <typename T, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_step_final_kernel(int C, int64_t n_e_blocks, const double* __restrict__ e_part,
                                                                            T* __restrict__ energy, int64_t n_row_blocks,
                                                                            const double* __restrict__ row_cell, int64_t n_k_blocks,
                                                                            const double* __restrict__ k_cell, int64_t n_q_blocks,
                                                                            const double* __restrict__ q_part, double bg,
                                                                            const double* __restrict__ geom, T* __restrict__ grad_cell) {
  ec_final_body<T, CELL>(C, n_e_blocks, e_part, energy, n_row_blocks, row_cell, n_k_blocks, k_cell, n_q_blocks, q_part, bg, geom,
                         grad_cell);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T, int CAP>
static int ewald_channels_step_t(const mipme_ewald_channels_step_args_t& a, const KPot& kp, const SRPot& sp) {
  hipStream_t st = (hipStream_t)a.stream;
  const int64_t N = a.n_atoms, K = a.n_k;
  const int C = a.n_channels;
  const bool cell = a.cell_gradient != 0;
  const EsWork w = ec_work_layout(N, K, C, cell, a.work);
  AtomRecord<T>* rec = (AtomRecord<T>*)a.records;
  const T* q = (const T*)a.charges;
  const EsTerms t = es_terms(a.pot, kp, sp);
  ewald_channels_step_prep_kernel<T><<<unsigned(w.n_table_blocks + w.n_atom_blocks), kEsBlock, 0, st>>>(
      kp, C, N, K, int(w.n_table_blocks), (const T*)a.cell, (const int*)a.frequencies, (const int*)a.multiplicities, a.ns[0], a.ns[1],
      a.ns[2], a.lr_wavelength, (const T*)a.positions, q, (T*)a.kvectors, (T*)a.G, cell ? (T*)a.dG : nullptr, rec, w.q_part, w.geom,
      (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (K > 0) {
    ewald_channels_step_structure_kernel<T, CAP><<<unsigned((K + kEsKPerBlock - 1) / kEsKPerBlock), kEsBlock, 0, st>>>(
        C, N, K, rec, q, (const T*)a.kvectors, (T*)a.s_cos, (T*)a.s_sin);
    MIPME_LAUNCH_CHECK();
    const int64_t chunk = (K + w.n_slices - 1) / w.n_slices;
    ewald_channels_step_atom_kernel<T, CAP><<<dim3(unsigned(N), unsigned(w.n_slices)), kEsBlock, 0, st>>>(
        C, K, chunk, rec, q, (const T*)a.kvectors, (const T*)a.G, (const T*)a.s_cos, (const T*)a.s_sin, (T*)w.slice_part);
    MIPME_LAUNCH_CHECK();
  }
  es_rows_dispatch(sp, cell, [&](auto pfast, auto with_cell) {
    ewald_channels_step_rows_kernel<T, CAP, pfast(), with_cell()><<<unsigned(w.n_fin_blocks), kEsBlock, 0, st>>>(
        sp, t.cf, C, N, (const int*)a.row_ptr, (const int*)a.entries, rec, q, (const T*)a.cell, T(a.full_list ? 0.5 : 1.0),
        (T*)w.row_out, with_cell() ? w.row_cell : nullptr);
  });
  MIPME_LAUNCH_CHECK();
  if (cell && K > 0) {
    ewald_channels_step_cellk_kernel<T, CAP><<<unsigned(w.n_k_blocks), kEsBlock, 0, st>>>(
        C, N, K, rec, q, (const T*)a.kvectors, (const T*)a.G, (const T*)a.dG, (const T*)a.s_cos, (const T*)a.s_sin, w.k_cell);
    MIPME_LAUNCH_CHECK();
  }
  ewald_channels_step_finish_kernel<T, CAP><<<unsigned(w.n_fin_blocks), kEsBlock, 0, st>>>(
      C, N, int(w.n_slices), T(t.self_c), 2.0 * t.bg, w.geom, q, (const T*)w.slice_part, (const T*)w.row_out, w.q_part, w.n_atom_blocks,
      (T*)a.forces, (T*)a.grad_charges, w.e_part);
  MIPME_LAUNCH_CHECK();
  if (cell)
    ewald_channels_step_final_kernel<T, true><<<1, kEsBlock, 0, st>>>(C, w.n_fin_blocks, w.e_part, (T*)a.energy, w.n_row_blocks,
                                                                     w.row_cell, w.n_k_blocks, w.k_cell, w.n_atom_blocks, w.q_part, t.bg,
                                                                     w.geom, (T*)a.grad_cell);
  else
    ewald_channels_step_final_kernel<T, false><<<1, kEsBlock, 0, st>>>(C, w.n_fin_blocks, w.e_part, (T*)a.energy, 0, nullptr, 0, nullptr,
                                                                      0, nullptr, t.bg, w.geom, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int ewald_channels_step_c(const mipme_ewald_channels_step_args_t& a, const KPot& kp, const SRPot& sp) {
  int rc = MIPME_OK;
  ec_capacity_dispatch(a.n_channels, [&](auto cap) { rc = ewald_channels_step_t<T, cap()>(a, kp, sp); });
  return rc;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_ewald_channels_step_work(int64_t n_atoms, int64_t n_k, int n_channels, int cell_gradient) {
  if (n_atoms < 1 || n_atoms > kCompactMaxAtoms || n_k < 0 || n_k > kEsMaxK) return 0;
  if (n_channels < kEcMinChannels || n_channels > kEcMaxChannels) return 0;
  return ec_work_layout(n_atoms, n_k, n_channels, cell_gradient != 0, nullptr).total;
}

int mipme_ewald_channels_step(const mipme_ewald_channels_step_args_t* in) {
  const char* who = "mipme_ewald_channels_step";
  mipme_ewald_channels_step_args_t a;
  int rc = load_args(in, a, MIPME_EWALD_CHANNELS_STEP_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  if ((rc = check_ewald_pot(a.dtype, a.pot, who))) return rc;
  MIPME_REQUIRE(a.n_channels >= kEcMinChannels && a.n_channels <= kEcMaxChannels,
                "%s: n_channels must be in 2..8, got %d (one channel: mipme_ewald_step)", who, int(a.n_channels));
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
  DT_SWITCH(a.dtype, ewald_channels_step_c<float>(a, kp, sp), ewald_channels_step_c<double>(a, kp, sp));
}

}  // extern "C"
