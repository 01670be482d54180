// The dipole step that follows its cell (mipme_dipole_cell_step, dipole_step.hip) for MANY small systems in one call
// (mipme_dipole_batch, include/mipme.h): F frames of point dipoles, each with its own cell, atom count, k grid and pair list,
// served by the same launches as one system -- prep, structure, atoms, rows, cell k (with the cell gradient), finish, final --
// each launched ONCE for the whole batch, on one stream, one after the other.  At the sizes the explicit dipolar Ewald sum is
// chosen for a step is six or seven launches of a few dozen workgroups each: latency, not work.  The batch puts the workgroups of
// all frames into the same seven launches.
//
// It is to the dipole step what ewald_batch.hip is to the Ewald step, with the same frame table (batch_table.h): a launch is a
// FLAT grid, the table maps every workgroup to (frame, local block), no workgroup is launched to find that it has nothing to do
// and none straddles two frames: one shift table per row block, one frame's positions and dipoles per LDS tile.  The table is
// built on the host from sizes alone (mipme_dipole_batch_table_build) -- nothing in it depends on any cell's values -- and
// uploaded once per capture.  A frame's work area is laid out exactly as the single step lays out its own (dcs_work_layout: the
// geometry record, 3 dipole partials per atom block, 6 results per atom, slices of at least 1024 k-vectors), the areas one behind
// the other in frame order; its two record arrays lie as the single step's, positions then dipoles, from record 2 * atom0.
//
// Inside its blocks a frame is computed as the single step computes it -- the bodies of dipole_step_bodies.h, which see one
// system and nothing of the table -- with LOCAL indices (partner atoms, row pointers and k-vectors count from the start of the
// frame): the slice count of the atom kernel is that of the single step for (N_f, K_f), every cross-block sum is float64 block
// partials of that frame added in index order by a later launch, and nothing a block reads belongs to another frame.  So the bits
// a frame gets depend on its own inputs alone -- not on its index, on F or on its neighbours in the batch.  No atomics, no
// workgroup waits for another.  A singular cell gives ITS frame a zero k table, E = NaN, dE/dcell = NaN and status bit 1, and
// no other frame anything.
#include <cmath>

#include "batch_table.h"
#include "dipole_device.h"
#include "dipole_step_bodies.h"
#include "ewald_step_device.h"
#include "host.h"

namespace mipme {

constexpr int kDbBlock = kStepBlock;
// the constants of dcs_work_layout (dipole_step.hip): the table lays out a frame's work area as the single step does
constexpr EbShape kDbShape = {kEsGeom, 3, 6, 1024};

// ---- the kernels: the bodies of dipole_step_bodies.h with the sizes, the slices and the local block index of the block's frame --
// blk and everything read from the frame's record is uniform per block.
template <typename T>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_prep_kernel(KPot kp, const EbFrame* __restrict__ frames,
                                                                    const EbBlock* __restrict__ blocks, const T* __restrict__ cells,
                                                                    const int* __restrict__ freq_all, const int* __restrict__ mult_all,
                                                                    double lr_wavelength, const T* __restrict__ pos_all,
                                                                    const T* __restrict__ mu_all, T* __restrict__ kvec_all,
                                                                    T* __restrict__ G_all, T* __restrict__ dG_all,
                                                                    AtomRecord<T>* __restrict__ rec_all, double* __restrict__ work,
                                                                    int* __restrict__ status) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  AtomRecord<T>* recp = rec_all + 2 * fr.atom0;
  ds_prep_body<T>(kp, fr.n_atoms, fr.n_k, fr.n_table_blocks, blk.local, cells + 9 * int64_t(blk.frame), freq_all + 3 * fr.k0,
                  mult_all + fr.k0, fr.ns[0], fr.ns[1], fr.ns[2], lr_wavelength, pos_all + 3 * fr.atom0, mu_all + 3 * fr.atom0,
                  kvec_all + 3 * fr.k0, G_all + fr.k0, dG_all ? dG_all + fr.k0 : nullptr, recp, recp + fr.n_atoms,
                  work + fr.atom_part, work + fr.geom, status + blk.frame);
}

template <typename T>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_structure_kernel(const EbFrame* __restrict__ frames,
                                                                         const EbBlock* __restrict__ blocks,
                                                                         const T* __restrict__ pos_all, const T* __restrict__ mu_all,
                                                                         const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                         const T* __restrict__ dG_all, T* __restrict__ Sc_all,
                                                                         T* __restrict__ Ss_all) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ds_structure_body<T>(fr.n_atoms, fr.n_k, int64_t(blk.local), pos_all + 3 * fr.atom0, mu_all + 3 * fr.atom0, kvec_all + 3 * fr.k0,
                       G_all + fr.k0, dG_all ? dG_all + fr.k0 : nullptr, Sc_all + fr.k0, Ss_all + fr.k0);
}

// local block = slice * N + i
template <typename T>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_atom_kernel(const EbFrame* __restrict__ frames,
                                                                    const EbBlock* __restrict__ blocks,
                                                                    const AtomRecord<T>* __restrict__ rec_all,
                                                                    const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                    const T* __restrict__ Sc_all, const T* __restrict__ Ss_all,
                                                                    double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms;
  const AtomRecord<T>* recp = rec_all + 2 * fr.atom0;
  ds_atom_body<T>(blk.local % N, blk.local / N, N, fr.n_k, fr.chunk, recp, recp + N, kvec_all + 3 * fr.k0, G_all + fr.k0,
                  Sc_all + fr.k0, Ss_all + fr.k0, (T*)(work + fr.slice_part));
}

// one shift table per row block: the table of the block's frame
template <typename T, bool EXCL, bool CELL>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_rows_kernel(DipPot<T> P, const EbFrame* __restrict__ frames,
                                                                    const EbBlock* __restrict__ blocks,
                                                                    const int* __restrict__ row_ptr_all,
                                                                    const int* __restrict__ ent32_all,
                                                                    const AtomRecord<T>* __restrict__ rec_all,
                                                                    const T* __restrict__ cells, T scale, double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const AtomRecord<T>* recp = rec_all + 2 * fr.atom0;
  ds_rows_body<T, EXCL, CELL>(P, fr.n_atoms, int64_t(blk.local), row_ptr_all + fr.rp0, ent32_all + fr.ent0, recp, recp + fr.n_atoms,
                              cells + 9 * int64_t(blk.frame), scale, (T*)(work + fr.row_out), work + fr.row_cell);
}

template <typename T>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_cellk_kernel(const EbFrame* __restrict__ frames,
                                                                     const EbBlock* __restrict__ blocks,
                                                                     const T* __restrict__ pos_all, const T* __restrict__ mu_all,
                                                                     const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                     const T* __restrict__ dG_all, const T* __restrict__ Sc_all,
                                                                     const T* __restrict__ Ss_all, double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ds_cellk_body<T>(fr.n_atoms, fr.n_k, int64_t(blk.local), pos_all + 3 * fr.atom0, mu_all + 3 * fr.atom0, kvec_all + 3 * fr.k0,
                   G_all + fr.k0, dG_all + fr.k0, Sc_all + fr.k0, Ss_all + fr.k0, work + fr.k_cell);
}

template <typename T>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_finish_kernel(const EbFrame* __restrict__ frames,
                                                                      const EbBlock* __restrict__ blocks, T self_term,
                                                                      double background, const AtomRecord<T>* __restrict__ rec_all,
                                                                      T* __restrict__ forces_all, T* __restrict__ grad_mu_all,
                                                                      double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ds_finish_body<T>(fr.n_atoms, fr.n_slices, int64_t(blk.local), self_term, background, work + fr.geom,
                    rec_all + 2 * fr.atom0 + fr.n_atoms, (const T*)(work + fr.slice_part), (const T*)(work + fr.row_out),
                    work + fr.atom_part, fr.n_atom_blocks, forces_all + 3 * fr.atom0, grad_mu_all + 3 * fr.atom0, work + fr.e_part);
}

// one block per frame: no block table
template <typename T, bool CELL>
__global__ __launch_bounds__(kDbBlock) void dipole_batch_final_kernel(const EbFrame* __restrict__ frames, double background,
                                                                     const double* __restrict__ work, T* __restrict__ energies,
                                                                     T* __restrict__ grad_cells) {
  const int64_t f = blockIdx.x;
  const EbFrame& fr = frames[f];
  ds_final_body<T, CELL>(fr.n_fin_blocks, work + fr.e_part, energies + f, fr.n_row_blocks, work + fr.row_cell, fr.n_k_blocks,
                         work + fr.k_cell, fr.n_atom_blocks, work + fr.atom_part, background, work + fr.geom,
                         CELL ? grad_cells + 9 * f : nullptr);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T, bool EXCL>
static void dipole_batch_rows_launch(hipStream_t st, const mipme_dipole_batch_args_t& a, const EbLayout& L, const DipPot<T>& dp,
                                     const EbFrame* frames, const EbBlock* b_row, const AtomRecord<T>* rec, double* work) {
  const T scale = T(a.full_list ? 0.5 : 1.0) * dp.pref;
  if (a.cell_gradient)
    dipole_batch_rows_kernel<T, EXCL, true><<<unsigned(L.n_rowblk), kDbBlock, 0, st>>>(
        dp, frames, b_row, (const int*)a.row_ptr, (const int*)a.entries, rec, (const T*)a.cells, scale, work);
  else
    dipole_batch_rows_kernel<T, EXCL, false><<<unsigned(L.n_rowblk), kDbBlock, 0, st>>>(
        dp, frames, b_row, (const int*)a.row_ptr, (const int*)a.entries, rec, (const T*)a.cells, scale, work);
}

template <typename T>
static int dipole_batch_t(const mipme_dipole_batch_args_t& a, const EbLayout& L, const DipPot<T>& dp, const KPot& kp) {
  hipStream_t st = (hipStream_t)a.stream;
  const bool cell = a.cell_gradient != 0;
  const EbFrame* frames = (const EbFrame*)a.device_table;
  const EbBlock* b_prep = (const EbBlock*)(frames + a.n_frames);
  const EbBlock* b_k = b_prep + L.n_prep;
  const EbBlock* b_atom = b_k + L.n_kblk;
  const EbBlock* b_row = b_atom + L.n_atomblk;
  AtomRecord<T>* rec = (AtomRecord<T>*)a.records;
  double* work = (double*)a.work;
  const T* pos = (const T*)a.positions;
  const T* mu = (const T*)a.dipoles;
  dipole_batch_prep_kernel<T><<<unsigned(L.n_prep), kDbBlock, 0, st>>>(
      kp, frames, b_prep, (const T*)a.cells, (const int*)a.frequencies, (const int*)a.multiplicities,
      a.pot->smearing > 0 ? a.lr_wavelength : 0.0, pos, mu, (T*)a.kvectors, (T*)a.G, cell ? (T*)a.dG : nullptr, rec, work,
      (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (L.n_kblk > 0) {
    dipole_batch_structure_kernel<T><<<unsigned(L.n_kblk), kDbBlock, 0, st>>>(frames, b_k, pos, mu, (const T*)a.kvectors,
                                                                             (const T*)a.G, cell ? (const T*)a.dG : nullptr,
                                                                             (T*)a.s_cos, (T*)a.s_sin);
    MIPME_LAUNCH_CHECK();
    dipole_batch_atom_kernel<T><<<unsigned(L.n_atomblk), kDbBlock, 0, st>>>(frames, b_atom, rec, (const T*)a.kvectors, (const T*)a.G,
                                                                           (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  if (dp.mode == 2)
    dipole_batch_rows_launch<T, true>(st, a, L, dp, frames, b_row, rec, work);
  else
    dipole_batch_rows_launch<T, false>(st, a, L, dp, frames, b_row, rec, work);
  MIPME_LAUNCH_CHECK();
  if (cell && L.n_kblk > 0) {
    dipole_batch_cellk_kernel<T><<<unsigned(L.n_kblk), kDbBlock, 0, st>>>(frames, b_k, pos, mu, (const T*)a.kvectors, (const T*)a.G,
                                                                         (const T*)a.dG, (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  dipole_batch_finish_kernel<T><<<unsigned(L.n_rowblk), kDbBlock, 0, st>>>(frames, b_row, T(a.self_term), a.background, rec,
                                                                          (T*)a.forces, (T*)a.grad_dipoles, work);
  MIPME_LAUNCH_CHECK();
  if (cell)
    dipole_batch_final_kernel<T, true><<<unsigned(a.n_frames), kDbBlock, 0, st>>>(frames, a.background, work, (T*)a.energies,
                                                                                 (T*)a.grad_cells);
  else
    dipole_batch_final_kernel<T, false><<<unsigned(a.n_frames), kDbBlock, 0, st>>>(frames, a.background, work, (T*)a.energies, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int dipole_batch_run(const mipme_dipole_batch_args_t& a, const EbLayout& L) {
  DipPot<T> dp;
  int rc = make_dippot<T>(a.pot, dp);
  if (rc) return rc;
  KPot kp{};
  if (L.sum_k > 0) {  // the reciprocal-space kernel 4 pi prefactor exp(-sigma^2 k^2 / 2) / k^2 is Coulomb's
    mipme_potential_t coulomb{};
    coulomb.kind = MIPME_COULOMB, coulomb.exponent = 1, coulomb.smearing = a.pot->smearing, coulomb.prefactor = a.pot->prefactor;
    coulomb.exclusion_radius = -1.0, coulomb.exclusion_degree = 1;
    if ((rc = make_kpot(&coulomb, kp))) return rc;
  }
  return dipole_batch_t<T>(a, L, dp, kp);
}

static const char* const kDbSizes =
    "sizes the batch does not serve (each frame 1..2^22 atoms, n_k >= 0, at least one entry word; the sums of the atoms, k-vectors "
    "and entries below 2^31; at most 2^24 - 1 workgroups per launch)";

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_dipole_batch_work(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int cell_gradient) {
  EbLayout L;
  if (!eb_layout(kDbShape, n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr)) return 0;
  return L.work_total;
}

int64_t mipme_dipole_batch_table_bytes(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int cell_gradient) {
  EbLayout L;
  if (!eb_layout(kDbShape, n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr)) return 0;
  return L.table_bytes;
}

int mipme_dipole_batch_table_build(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, const int64_t* entry_ptr,
                                   const int32_t* ns, int cell_gradient, void* host_table, int64_t host_table_bytes) {
  const char* who = "mipme_dipole_batch_table_build";
  MIPME_REQUIRE(n_frames >= 1 && n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, n_frames);
  MIPME_REQUIRE(atom_ptr && k_ptr && entry_ptr && ns && host_table, "%s: NULL array", who);
  for (int f = 0; f < n_frames; ++f)
    MIPME_REQUIRE(ns[3 * f] >= 1 && ns[3 * f + 1] >= 1 && ns[3 * f + 2] >= 1, "%s: frame %d: ns must be >= 1, got (%d, %d, %d)", who, f,
                  int(ns[3 * f]), int(ns[3 * f + 1]), int(ns[3 * f + 2]));
  EbLayout L;
  MIPME_REQUIRE(eb_layout(kDbShape, n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, nullptr, nullptr), "%s: %s", who,
                kDbSizes);
  MIPME_REQUIRE(host_table_bytes == L.table_bytes, "%s: host_table_bytes is %lld, mipme_dipole_batch_table_bytes says %lld", who,
                (long long)host_table_bytes, (long long)L.table_bytes);
  EbFrame* frames = (EbFrame*)host_table;
  eb_layout(kDbShape, n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, frames, (EbBlock*)(frames + n_frames));
  return MIPME_OK;
}

int mipme_dipole_batch(const mipme_dipole_batch_args_t* in) {
  const char* who = "mipme_dipole_batch";
  mipme_dipole_batch_args_t a;
  int rc = load_args(in, a, MIPME_DIPOLE_BATCH_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  MIPME_REQUIRE(a.dtype == MIPME_F32 || a.dtype == MIPME_F64, "%s: invalid dtype %d", who, int(a.dtype));
  MIPME_REQUIRE(a.pot != nullptr, "%s: dipole descriptor is NULL", who);
  MIPME_REQUIRE(!(a.pot->exclusion_radius > 0) || a.pot->exclusion_degree >= 1, "%s: exclusion_degree must be >= 1, got %d", who,
                int(a.pot->exclusion_degree));
  MIPME_REQUIRE((a.shift_format & 0xff) == 2 && !(a.shift_format & MIPME_ROWS_PADDED),
                "%s: the rows are read as 4-byte entries, other | code << 22 (shift_format 2), got shift_format %d", who,
                int(a.shift_format));
  MIPME_REQUIRE(a.n_frames >= 1 && a.n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, int(a.n_frames));
  MIPME_REQUIRE(a.atom_ptr && a.k_ptr && a.entry_ptr && a.device_table, "%s: NULL required buffer (atom_ptr, k_ptr, entry_ptr, device_table)",
                who);
  EbLayout L;
  MIPME_REQUIRE(eb_layout(kDbShape, a.n_frames, a.atom_ptr, a.k_ptr, a.entry_ptr, nullptr, a.cell_gradient != 0, L, nullptr, nullptr),
                "%s: %s", who, kDbSizes);
  MIPME_REQUIRE(L.sum_k == 0 || a.pot->smearing > 0,
                "%s: the frames hold %lld k-vectors but the potential has no smearing (`smearing` is %g): a direct potential has no "
                "reciprocal part", who, (long long)L.sum_k, a.pot->smearing);
  MIPME_REQUIRE(std::isfinite(a.lr_wavelength) && (a.lr_wavelength > 0 || (L.sum_k == 0 && !(a.pot->smearing > 0))),
                "%s: lr_wavelength must be positive (the grid `status` compares with; 0 only for a potential without smearing), got %g",
                who, a.lr_wavelength);
  MIPME_REQUIRE(!a.cell_gradient || a.grad_cells, "%s: cell_gradient needs grad_cells", who);
  MIPME_REQUIRE(!a.cell_gradient || L.sum_k == 0 || a.dG, "%s: cell_gradient needs dG (sum of n_k reals of scratch)", who);
  MIPME_REQUIRE(a.positions && a.dipoles && a.cells && a.row_ptr && a.entries && a.records && a.energies && a.forces && a.grad_dipoles &&
                    a.status && a.work &&
                    (L.sum_k == 0 || (a.frequencies && a.multiplicities && a.kvectors && a.G && a.s_cos && a.s_sin)),
                "%s: NULL required buffer", who);
  DT_SWITCH(a.dtype, dipole_batch_run<float>(a, L), dipole_batch_run<double>(a, L));
}

}  // extern "C"
