// The Ewald step of ewald_step.hip for MANY small systems in one call (mipme_ewald_batch, include/mipme.h): F frames, each with
// its own cell, atom count, k grid and pair list, served by the same launches as one system -- prep, structure, atoms, rows,
// cell k (with the cell gradient), finish, final -- each launched ONCE for the whole batch, on one stream, one after the other.
// At the sizes the explicit Ewald sum is chosen for a step is seven launches of a few dozen workgroups each: latency, not work.
// The batch puts the workgroups of all frames into the same seven launches.
//
// Frames differ in size, so a launch is a FLAT grid and a table maps every workgroup to (frame, local block): no workgroup is
// launched to find that it has nothing to do (one 4 096-atom frame beside 500 frames of 20 atoms costs the sum of their blocks,
// not 501 times the largest), and no workgroup straddles two frames: one shift table per row block, one frame's records per LDS
// tile.  The table (mipme_ewald_batch_table_build) is built on the host from sizes alone -- nothing in it depends on any cell's
// values -- and uploaded once per capture:
//   [EbFrame x F][prep blocks][k blocks (structure, cell k)][atom blocks][row blocks (rows, finish)]     (EbBlock = frame, local)
// A frame's record holds where its slices of the concatenated buffers begin and where its work area lies; the work area of a frame
// is laid out exactly as the single step lays out its own (es_work_layout), the areas one behind the other in frame order.
//
// Inside its blocks a frame is computed as the single step computes it -- by the same bodies (ewald_step_bodies.h), which see
// one system and nothing of the table -- with LOCAL indices (partner atoms, row pointers and k-vectors count from the start of
// the frame): the slice count of the atom kernel is that of the single step for (N_f, K_f), every cross-block sum is float64
// block partials of that frame added in index order by a later launch, and nothing a block reads belongs to another frame.  So
// the bits a frame gets depend on its own inputs alone -- not on its index, on F or on its neighbours in the batch.
// No atomics, no workgroup waits for another.  A singular cell gives ITS frame a zero k table, E = NaN, dE/dcell = NaN and
// status bit 1, and no other frame anything.
#include <cmath>

#include "batch_table.h"  // EbFrame, EbBlock, EbLayout, eb_layout: the frame table, shared with dipole_batch.hip
#include "ewald_step_bodies.h"
#include "ewald_step_device.h"
#include "host.h"

namespace mipme {

// the constants of es_work_layout: the table lays out a frame's work area as the single step does
constexpr EbShape kEbEwaldShape = {kEsGeom, 1, 4, kEsMinSlice};

// ---- the kernels: the bodies of ewald_step_bodies.h with the sizes, the slices and the local block index of the block's frame ----
// blk and everything read from the frame's record is uniform per block.  Partner atoms, row pointers and k-vectors are local to
// the frame: a body that gets the frame's slices computes what the single step computes.
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_prep_kernel(KPot kp, const EbFrame* __restrict__ frames,
                                                                   const EbBlock* __restrict__ blocks, const T* __restrict__ cells,
                                                                   const int* __restrict__ freq_all, const int* __restrict__ mult_all,
                                                                   double lr_wavelength, const T* __restrict__ pos_all,
                                                                   const T* __restrict__ q_all, T* __restrict__ kvec_all,
                                                                   T* __restrict__ G_all, T* __restrict__ dG_all,
                                                                   AtomRecord<T>* __restrict__ rec_all, double* __restrict__ work,
                                                                   int* __restrict__ status) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  es_prep_body<T>(kp, fr.n_atoms, fr.n_k, fr.n_table_blocks, blk.local, cells + 9 * int64_t(blk.frame), freq_all + 3 * fr.k0,
                  mult_all + fr.k0, fr.ns[0], fr.ns[1], fr.ns[2], lr_wavelength, pos_all + 3 * fr.atom0, q_all + fr.atom0,
                  kvec_all + 3 * fr.k0, G_all + fr.k0, dG_all ? dG_all + fr.k0 : nullptr, rec_all + fr.atom0, work + fr.atom_part,
                  work + fr.geom, status + blk.frame);
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_structure_kernel(const EbFrame* __restrict__ frames,
                                                                        const EbBlock* __restrict__ blocks,
                                                                        const AtomRecord<T>* __restrict__ rec_all,
                                                                        const T* __restrict__ kvec_all, T* __restrict__ Sc_all,
                                                                        T* __restrict__ Ss_all) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  es_structure_body<T>(fr.n_atoms, fr.n_k, int64_t(blk.local), rec_all + fr.atom0, kvec_all + 3 * fr.k0, Sc_all + fr.k0,
                       Ss_all + fr.k0);
}

// local block = slice * N + i
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_atom_kernel(const EbFrame* __restrict__ frames, const EbBlock* __restrict__ blocks,
                                                                   const AtomRecord<T>* __restrict__ rec_all,
                                                                   const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                   const T* __restrict__ Sc_all, const T* __restrict__ Ss_all,
                                                                   double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms;
  es_atom_body<T>(blk.local % N, blk.local / N, N, fr.n_k, fr.chunk, rec_all + fr.atom0, kvec_all + 3 * fr.k0, G_all + fr.k0,
                  Sc_all + fr.k0, Ss_all + fr.k0, (T*)(work + fr.slice_part));
}

// one shift table per row block: the table of the block's frame
template <typename T, int PFAST, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_rows_kernel(SRPot sp, FastRS cf, const EbFrame* __restrict__ frames,
                                                                   const EbBlock* __restrict__ blocks,
                                                                   const int* __restrict__ row_ptr_all,
                                                                   const int* __restrict__ ent32_all,
                                                                   const AtomRecord<T>* __restrict__ rec_all,
                                                                   const T* __restrict__ cells, T scale, double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  es_rows_body<T, PFAST, CELL>(sp, cf, fr.n_atoms, int64_t(blk.local), row_ptr_all + fr.rp0, ent32_all + fr.ent0, rec_all + fr.atom0,
                               cells + 9 * int64_t(blk.frame), scale, (T*)(work + fr.row_out), work + fr.row_cell);
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_cellk_kernel(const EbFrame* __restrict__ frames, const EbBlock* __restrict__ blocks,
                                                                    const AtomRecord<T>* __restrict__ rec_all,
                                                                    const T* __restrict__ kvec_all, const T* __restrict__ G_all,
                                                                    const T* __restrict__ dG_all, const T* __restrict__ Sc_all,
                                                                    const T* __restrict__ Ss_all, double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  es_cellk_body<T>(fr.n_atoms, fr.n_k, int64_t(blk.local), rec_all + fr.atom0, kvec_all + 3 * fr.k0, G_all + fr.k0, dG_all + fr.k0,
                   Sc_all + fr.k0, Ss_all + fr.k0, work + fr.k_cell);
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_finish_kernel(const EbFrame* __restrict__ frames, const EbBlock* __restrict__ blocks,
                                                                     T self_c, double two_bg, const AtomRecord<T>* __restrict__ rec_all,
                                                                     T* __restrict__ forces_all, T* __restrict__ grad_q_all,
                                                                     double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  es_finish_body<T>(fr.n_atoms, fr.n_slices, int64_t(blk.local), self_c, two_bg, work + fr.geom, rec_all + fr.atom0,
                    (const T*)(work + fr.slice_part), (const T*)(work + fr.row_out), work + fr.atom_part, fr.n_atom_blocks,
                    forces_all + 3 * fr.atom0, grad_q_all + fr.atom0, work + fr.e_part);
}

// one block per frame: no block table
template <typename T, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_batch_final_kernel(const EbFrame* __restrict__ frames, double bg,
                                                                    const double* __restrict__ work, T* __restrict__ energies,
                                                                    T* __restrict__ grad_cells) {
  const int64_t f = blockIdx.x;
  const EbFrame& fr = frames[f];
  es_final_body<T, CELL>(fr.n_fin_blocks, work + fr.e_part, energies + f, fr.n_row_blocks, work + fr.row_cell, fr.n_k_blocks,
                         work + fr.k_cell, fr.n_atom_blocks, work + fr.atom_part, bg, work + fr.geom, CELL ? grad_cells + 9 * f : nullptr);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T>
static int ewald_batch_t(const mipme_ewald_batch_args_t& a, const EbLayout& L, const KPot& kp, const SRPot& sp) {
  hipStream_t st = (hipStream_t)a.stream;
  const bool cell = a.cell_gradient != 0;
  const EbFrame* frames = (const EbFrame*)a.device_table;
  const EbBlock* b_prep = (const EbBlock*)(frames + a.n_frames);
  const EbBlock* b_k = b_prep + L.n_prep;
  const EbBlock* b_atom = b_k + L.n_kblk;
  const EbBlock* b_row = b_atom + L.n_atomblk;
  AtomRecord<T>* rec = (AtomRecord<T>*)a.records;
  double* work = (double*)a.work;
  const EsTerms t = es_terms(a.pot, kp, sp);
  ewald_batch_prep_kernel<T><<<unsigned(L.n_prep), kEsBlock, 0, st>>>(
      kp, frames, b_prep, (const T*)a.cells, (const int*)a.frequencies, (const int*)a.multiplicities, a.lr_wavelength,
      (const T*)a.positions, (const T*)a.charges, (T*)a.kvectors, (T*)a.G, cell ? (T*)a.dG : nullptr, rec, work, (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (L.n_kblk > 0) {
    ewald_batch_structure_kernel<T><<<unsigned(L.n_kblk), kEsBlock, 0, st>>>(frames, b_k, rec, (const T*)a.kvectors, (T*)a.s_cos,
                                                                            (T*)a.s_sin);
    MIPME_LAUNCH_CHECK();
    ewald_batch_atom_kernel<T><<<unsigned(L.n_atomblk), kEsBlock, 0, st>>>(frames, b_atom, rec, (const T*)a.kvectors, (const T*)a.G,
                                                                          (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  es_rows_dispatch(sp, cell, [&](auto pfast, auto with_cell) {
    ewald_batch_rows_kernel<T, pfast(), with_cell()><<<unsigned(L.n_rowblk), kEsBlock, 0, st>>>(
        sp, t.cf, frames, b_row, (const int*)a.row_ptr, (const int*)a.entries, rec, (const T*)a.cells, T(a.full_list ? 0.5 : 1.0), work);
  });
  MIPME_LAUNCH_CHECK();
  if (cell && L.n_kblk > 0) {
    ewald_batch_cellk_kernel<T><<<unsigned(L.n_kblk), kEsBlock, 0, st>>>(frames, b_k, rec, (const T*)a.kvectors, (const T*)a.G,
                                                                        (const T*)a.dG, (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  ewald_batch_finish_kernel<T><<<unsigned(L.n_rowblk), kEsBlock, 0, st>>>(frames, b_row, T(t.self_c), 2.0 * t.bg, rec, (T*)a.forces,
                                                                         (T*)a.grad_charges, work);
  MIPME_LAUNCH_CHECK();
  if (cell)
    ewald_batch_final_kernel<T, true><<<unsigned(a.n_frames), kEsBlock, 0, st>>>(frames, t.bg, work, (T*)a.energies, (T*)a.grad_cells);
  else
    ewald_batch_final_kernel<T, false><<<unsigned(a.n_frames), kEsBlock, 0, st>>>(frames, t.bg, work, (T*)a.energies, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_ewald_batch_work(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int cell_gradient) {
  EbLayout L;
  if (!eb_layout(kEbEwaldShape, n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr)) return 0;
  return L.work_total;
}

int64_t mipme_ewald_batch_table_bytes(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int cell_gradient) {
  EbLayout L;
  if (!eb_layout(kEbEwaldShape, n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr)) return 0;
  return L.table_bytes;
}

int mipme_ewald_batch_table_build(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, const int64_t* entry_ptr,
                                  const int32_t* ns, int cell_gradient, void* host_table, int64_t host_table_bytes) {
  const char* who = "mipme_ewald_batch_table_build";
  MIPME_REQUIRE(n_frames >= 1 && n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, n_frames);
  MIPME_REQUIRE(atom_ptr && k_ptr && entry_ptr && ns && host_table, "%s: NULL array", who);
  for (int f = 0; f < n_frames; ++f)
    MIPME_REQUIRE(ns[3 * f] >= 1 && ns[3 * f + 1] >= 1 && ns[3 * f + 2] >= 1, "%s: frame %d: ns must be >= 1, got (%d, %d, %d)", who, f,
                  int(ns[3 * f]), int(ns[3 * f + 1]), int(ns[3 * f + 2]));
  EbLayout L;
  MIPME_REQUIRE(eb_layout(kEbEwaldShape, n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, nullptr, nullptr),
                "%s: sizes the batch does not serve (each frame 1..2^22 atoms, n_k >= 0, at least one entry word; the sums of the atoms, "
                "k-vectors and entries below 2^31; at most 2^24 - 1 workgroups per launch)", who);
  MIPME_REQUIRE(host_table_bytes == L.table_bytes, "%s: host_table_bytes is %lld, mipme_ewald_batch_table_bytes says %lld", who,
                (long long)host_table_bytes, (long long)L.table_bytes);
  EbFrame* frames = (EbFrame*)host_table;
  eb_layout(kEbEwaldShape, n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, frames, (EbBlock*)(frames + n_frames));
  return MIPME_OK;
}

int mipme_ewald_batch(const mipme_ewald_batch_args_t* in) {
  const char* who = "mipme_ewald_batch";
  mipme_ewald_batch_args_t a;
  int rc = load_args(in, a, MIPME_EWALD_BATCH_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  if ((rc = check_ewald_pot(a.dtype, a.pot, who))) return rc;
  MIPME_REQUIRE((a.shift_format & 0xff) == 2 && !(a.shift_format & MIPME_ROWS_PADDED),
                "%s: the rows are read as 4-byte entries, other | code << 22 (shift_format 2), got shift_format %d", who,
                int(a.shift_format));
  MIPME_REQUIRE(a.n_frames >= 1 && a.n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, int(a.n_frames));
  MIPME_REQUIRE(std::isfinite(a.lr_wavelength) && a.lr_wavelength > 0, "%s: lr_wavelength must be positive, got %g", who, a.lr_wavelength);
  MIPME_REQUIRE(a.atom_ptr && a.k_ptr && a.entry_ptr && a.device_table, "%s: NULL required buffer (atom_ptr, k_ptr, entry_ptr, device_table)",
                who);
  EbLayout L;
  MIPME_REQUIRE(eb_layout(kEbEwaldShape, a.n_frames, a.atom_ptr, a.k_ptr, a.entry_ptr, nullptr, a.cell_gradient != 0, L, nullptr, nullptr),
                "%s: sizes the batch does not serve (each frame 1..2^22 atoms, n_k >= 0, at least one entry word; the sums of the atoms, "
                "k-vectors and entries below 2^31; at most 2^24 - 1 workgroups per launch)", who);
  MIPME_REQUIRE(!a.cell_gradient || a.grad_cells, "%s: cell_gradient needs grad_cells", who);
  MIPME_REQUIRE(!a.cell_gradient || L.sum_k == 0 || a.dG, "%s: cell_gradient needs dG (sum of n_k reals of scratch)", who);
  MIPME_REQUIRE(a.positions && a.charges && a.cells && a.row_ptr && a.entries && a.records && a.energies && a.forces && a.grad_charges &&
                    a.status && a.work &&
                    (L.sum_k == 0 || (a.frequencies && a.multiplicities && a.kvectors && a.G && a.s_cos && a.s_sin)),
                "%s: NULL required buffer", who);
  KPot kp;
  SRPot sp;
  if ((rc = make_kpot(a.pot, kp)) || (rc = make_srpot(a.pot, sp))) return rc;
  DT_SWITCH(a.dtype, ewald_batch_t<float>(a, L, kp, sp), ewald_batch_t<double>(a, L, kp, sp));
}

}  // extern "C"
