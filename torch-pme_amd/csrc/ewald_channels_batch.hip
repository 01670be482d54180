// The multi-channel Ewald step of ewald_channels_step.hip for MANY small systems in one call (mipme_ewald_channels_batch,
// include/mipme.h): F frames, each with its own cell, atom count, k grid and pair list, all with the same C charge channels --
// the training set of a model with latent charges, dE/dq of every channel of every frame back from one replay.  It is to
// ewald_channels_step.hip what ewald_batch.hip is to ewald_step.hip: the same seven launches, each ONCE for the whole batch as a
// flat grid, the frame table of batch_table.h mapping every workgroup to (frame, local block), the bodies of
// ewald_channels_bodies.h seeing one system and nothing of the table.
//
// The table is eb_layout's with a shape of its own: C partials per atom block, C + 3 results per atom.  EbFrame has no field for
// the channels: a frame's slice of the (sum N, C) charges and charge gradients begins at atom0 C, its slice of the S^c(k) at
// k0 C (channel-major inside the frame), and C is a kernel argument.  The bits a frame gets depend on its own inputs alone.
// No atomics, no workgroup waits for another.
#include <cmath>

#include "batch_table.h"
#include "ewald_channels_bodies.h"
#include "ewald_step_device.h"
#include "host.h"

namespace mipme {

// the constants of ec_work_layout: the table lays out a frame's work area as the single multi-channel step does
static EbShape ecb_shape(int C) { return EbShape{kEsGeom, C, C + 3, kEsMinSlice}; }
static bool ecb_channels_ok(int C) { return C >= kEcMinChannels && C <= kEcMaxChannels; }

// ---- the kernels: the bodies with the sizes, the slices and the local block index of the block's frame -------------------------
template <typename T>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_prep_kernel(KPot kp, int C, const EbFrame* __restrict__ frames,
                                                                            const EbBlock* __restrict__ blocks,
                                                                            const T* __restrict__ cells, const int* __restrict__ freq_all,
                                                                            const int* __restrict__ mult_all, double lr_wavelength,
                                                                            const T* __restrict__ pos_all, const T* __restrict__ q_all,
                                                                            T* __restrict__ kvec_all, T* __restrict__ G_all,
                                                                            T* __restrict__ dG_all, AtomRecord<T>* __restrict__ rec_all,
                                                                            double* __restrict__ work, int* __restrict__ status) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ec_prep_body<T>(kp, C, fr.n_atoms, fr.n_k, fr.n_table_blocks, blk.local, cells + 9 * int64_t(blk.frame), freq_all + 3 * fr.k0,
                  mult_all + fr.k0, fr.ns[0], fr.ns[1], fr.ns[2], lr_wavelength, pos_all + 3 * fr.atom0, q_all + fr.atom0 * C,
                  kvec_all + 3 * fr.k0, G_all + fr.k0, dG_all ? dG_all + fr.k0 : nullptr, rec_all + fr.atom0, work + fr.atom_part,
                  work + fr.geom, status + blk.frame);
}

template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_structure_kernel(int C, const EbFrame* __restrict__ frames,
                                                                                 const EbBlock* __restrict__ blocks,
                                                                                 const AtomRecord<T>* __restrict__ rec_all,
                                                                                 const T* __restrict__ q_all,
                                                                                 const T* __restrict__ kvec_all, T* __restrict__ Sc_all,
                                                                                 T* __restrict__ Ss_all) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ec_structure_body<T, CAP>(C, fr.n_atoms, fr.n_k, int64_t(blk.local), rec_all + fr.atom0, q_all + fr.atom0 * C, kvec_all + 3 * fr.k0,
                            Sc_all + fr.k0 * C, Ss_all + fr.k0 * C);
}

// local block = slice * N + i
template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_atom_kernel(int C, const EbFrame* __restrict__ frames,
                                                                            const EbBlock* __restrict__ blocks,
                                                                            const AtomRecord<T>* __restrict__ rec_all,
                                                                            const T* __restrict__ q_all, const T* __restrict__ kvec_all,
                                                                            const T* __restrict__ G_all, const T* __restrict__ Sc_all,
                                                                            const T* __restrict__ Ss_all, double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  const int64_t N = fr.n_atoms;
  ec_atom_body<T, CAP>(C, blk.local % N, blk.local / N, N, fr.n_k, fr.chunk, rec_all + fr.atom0, q_all + fr.atom0 * C,
                       kvec_all + 3 * fr.k0, G_all + fr.k0, Sc_all + fr.k0 * C, Ss_all + fr.k0 * C, (T*)(work + fr.slice_part));
}

// one shift table per row block: the table of the block's frame
template <typename T, int CAP, int PFAST, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_rows_kernel(SRPot sp, FastRS cf, int C, const EbFrame* __restrict__ frames,
                                                                            const EbBlock* __restrict__ blocks,
                                                                            const int* __restrict__ row_ptr_all,
                                                                            const int* __restrict__ ent32_all,
                                                                            const AtomRecord<T>* __restrict__ rec_all,
                                                                            const T* __restrict__ q_all, const T* __restrict__ cells,
                                                                            T scale, double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ec_rows_body<T, CAP, PFAST, CELL>(sp, cf, C, fr.n_atoms, int64_t(blk.local), row_ptr_all + fr.rp0, ent32_all + fr.ent0,
                                    rec_all + fr.atom0, q_all + fr.atom0 * C, cells + 9 * int64_t(blk.frame), scale,
                                    (T*)(work + fr.row_out), work + fr.row_cell);
}

template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_cellk_kernel(int C, const EbFrame* __restrict__ frames,
                                                                             const EbBlock* __restrict__ blocks,
                                                                             const AtomRecord<T>* __restrict__ rec_all,
                                                                             const T* __restrict__ q_all, const T* __restrict__ kvec_all,
                                                                             const T* __restrict__ G_all, const T* __restrict__ dG_all,
                                                                             const T* __restrict__ Sc_all, const T* __restrict__ Ss_all,
                                                                             double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ec_cellk_body<T, CAP>(C, fr.n_atoms, fr.n_k, int64_t(blk.local), rec_all + fr.atom0, q_all + fr.atom0 * C, kvec_all + 3 * fr.k0,
                        G_all + fr.k0, dG_all + fr.k0, Sc_all + fr.k0 * C, Ss_all + fr.k0 * C, work + fr.k_cell);
}

template <typename T, int CAP>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_finish_kernel(int C, const EbFrame* __restrict__ frames,
                                                                              const EbBlock* __restrict__ blocks, T self_c,
                                                                              double two_bg, const T* __restrict__ q_all,
                                                                              T* __restrict__ forces_all, T* __restrict__ grad_q_all,
                                                                              double* __restrict__ work) {
  const EbBlock blk = blocks[blockIdx.x];
  const EbFrame& fr = frames[blk.frame];
  ec_finish_body<T, CAP>(C, fr.n_atoms, fr.n_slices, int64_t(blk.local), self_c, two_bg, work + fr.geom, q_all + fr.atom0 * C,
                         (const T*)(work + fr.slice_part), (const T*)(work + fr.row_out), work + fr.atom_part, fr.n_atom_blocks,
                         forces_all + 3 * fr.atom0, grad_q_all + fr.atom0 * C, work + fr.e_part);
}

// one block per frame: no block table
template <typename T, bool CELL>
__global__ __launch_bounds__(kEsBlock) void ewald_channels_batch_final_kernel(int C, const EbFrame* __restrict__ frames, double bg,
                                                                             const double* __restrict__ work, T* __restrict__ energies,
                                                                             T* __restrict__ grad_cells) {
  const int64_t f = blockIdx.x;
  const EbFrame& fr = frames[f];
  ec_final_body<T, CELL>(C, fr.n_fin_blocks, work + fr.e_part, energies + f, fr.n_row_blocks, work + fr.row_cell, fr.n_k_blocks,
                         work + fr.k_cell, fr.n_atom_blocks, work + fr.atom_part, bg, work + fr.geom,
                         CELL ? grad_cells + 9 * f : nullptr);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T, int CAP>
static int ewald_channels_batch_t(const mipme_ewald_channels_batch_args_t& a, const EbLayout& L, const KPot& kp, const SRPot& sp) {
  hipStream_t st = (hipStream_t)a.stream;
  const bool cell = a.cell_gradient != 0;
  const int C = a.n_channels;
  const EbFrame* frames = (const EbFrame*)a.device_table;
  const EbBlock* b_prep = (const EbBlock*)(frames + a.n_frames);
  const EbBlock* b_k = b_prep + L.n_prep;
  const EbBlock* b_atom = b_k + L.n_kblk;
  const EbBlock* b_row = b_atom + L.n_atomblk;
  AtomRecord<T>* rec = (AtomRecord<T>*)a.records;
  const T* q = (const T*)a.charges;
  double* work = (double*)a.work;
  const EsTerms t = es_terms(a.pot, kp, sp);
  ewald_channels_batch_prep_kernel<T><<<unsigned(L.n_prep), kEsBlock, 0, st>>>(
      kp, C, frames, b_prep, (const T*)a.cells, (const int*)a.frequencies, (const int*)a.multiplicities, a.lr_wavelength,
      (const T*)a.positions, q, (T*)a.kvectors, (T*)a.G, cell ? (T*)a.dG : nullptr, rec, work, (int*)a.status);
  MIPME_LAUNCH_CHECK();
  if (L.n_kblk > 0) {
    ewald_channels_batch_structure_kernel<T, CAP><<<unsigned(L.n_kblk), kEsBlock, 0, st>>>(C, frames, b_k, rec, q, (const T*)a.kvectors,
                                                                                          (T*)a.s_cos, (T*)a.s_sin);
    MIPME_LAUNCH_CHECK();
    ewald_channels_batch_atom_kernel<T, CAP><<<unsigned(L.n_atomblk), kEsBlock, 0, st>>>(
        C, frames, b_atom, rec, q, (const T*)a.kvectors, (const T*)a.G, (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  es_rows_dispatch(sp, cell, [&](auto pfast, auto with_cell) {
    ewald_channels_batch_rows_kernel<T, CAP, pfast(), with_cell()><<<unsigned(L.n_rowblk), kEsBlock, 0, st>>>(
        sp, t.cf, C, frames, b_row, (const int*)a.row_ptr, (const int*)a.entries, rec, q, (const T*)a.cells,
        T(a.full_list ? 0.5 : 1.0), work);
  });
  MIPME_LAUNCH_CHECK();
  if (cell && L.n_kblk > 0) {
    ewald_channels_batch_cellk_kernel<T, CAP><<<unsigned(L.n_kblk), kEsBlock, 0, st>>>(
        C, frames, b_k, rec, q, (const T*)a.kvectors, (const T*)a.G, (const T*)a.dG, (const T*)a.s_cos, (const T*)a.s_sin, work);
    MIPME_LAUNCH_CHECK();
  }
  ewald_channels_batch_finish_kernel<T, CAP><<<unsigned(L.n_rowblk), kEsBlock, 0, st>>>(C, frames, b_row, T(t.self_c), 2.0 * t.bg, q,
                                                                                       (T*)a.forces, (T*)a.grad_charges, work);
  MIPME_LAUNCH_CHECK();
  if (cell)
    ewald_channels_batch_final_kernel<T, true><<<unsigned(a.n_frames), kEsBlock, 0, st>>>(C, frames, t.bg, work, (T*)a.energies,
                                                                                         (T*)a.grad_cells);
  else
    ewald_channels_batch_final_kernel<T, false><<<unsigned(a.n_frames), kEsBlock, 0, st>>>(C, frames, t.bg, work, (T*)a.energies, nullptr);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
static int ewald_channels_batch_c(const mipme_ewald_channels_batch_args_t& a, const EbLayout& L, const KPot& kp, const SRPot& sp) {
  int rc = MIPME_OK;
  ec_capacity_dispatch(a.n_channels, [&](auto cap) { rc = ewald_channels_batch_t<T, cap()>(a, L, kp, sp); });
  return rc;
}

}  // namespace mipme

using namespace mipme;

extern "C" {

int64_t mipme_ewald_channels_batch_work(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int n_channels, int cell_gradient) {
  EbLayout L;
  if (!ecb_channels_ok(n_channels) ||
      !eb_layout(ecb_shape(n_channels), n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr))
    return 0;
  return L.work_total;
}

int64_t mipme_ewald_channels_batch_table_bytes(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, int n_channels,
                                               int cell_gradient) {
  EbLayout L;
  if (!ecb_channels_ok(n_channels) ||
      !eb_layout(ecb_shape(n_channels), n_frames, atom_ptr, k_ptr, nullptr, nullptr, cell_gradient != 0, L, nullptr, nullptr))
    return 0;
  return L.table_bytes;
}

int mipme_ewald_channels_batch_table_build(int n_frames, const int64_t* atom_ptr, const int64_t* k_ptr, const int64_t* entry_ptr,
                                           const int32_t* ns, int n_channels, int cell_gradient, void* host_table,
                                           int64_t host_table_bytes) {
  const char* who = "mipme_ewald_channels_batch_table_build";
  MIPME_REQUIRE(ecb_channels_ok(n_channels), "%s: n_channels must be in 2..8, got %d (one channel: mipme_ewald_batch_table_build)", who,
                n_channels);
  MIPME_REQUIRE(n_frames >= 1 && n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, n_frames);
  MIPME_REQUIRE(atom_ptr && k_ptr && entry_ptr && ns && host_table, "%s: NULL array", who);
  for (int f = 0; f < n_frames; ++f)
    MIPME_REQUIRE(ns[3 * f] >= 1 && ns[3 * f + 1] >= 1 && ns[3 * f + 2] >= 1, "%s: frame %d: ns must be >= 1, got (%d, %d, %d)", who, f,
                  int(ns[3 * f]), int(ns[3 * f + 1]), int(ns[3 * f + 2]));
  const EbShape shape = ecb_shape(n_channels);
  EbLayout L;
  MIPME_REQUIRE(eb_layout(shape, n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, nullptr, nullptr),
                "%s: sizes the batch does not serve (each frame 1..2^22 atoms, n_k >= 0, at least one entry word; the sums of the atoms, "
                "k-vectors and entries below 2^31; at most 2^24 - 1 workgroups per launch)", who);
  MIPME_REQUIRE(host_table_bytes == L.table_bytes, "%s: host_table_bytes is %lld, mipme_ewald_channels_batch_table_bytes says %lld", who,
                (long long)host_table_bytes, (long long)L.table_bytes);
  EbFrame* frames = (EbFrame*)host_table;
  eb_layout(shape, n_frames, atom_ptr, k_ptr, entry_ptr, ns, cell_gradient != 0, L, frames, (EbBlock*)(frames + n_frames));
  return MIPME_OK;
}

int mipme_ewald_channels_batch(const mipme_ewald_channels_batch_args_t* in) {
  const char* who = "mipme_ewald_channels_batch";
  mipme_ewald_channels_batch_args_t a;
  int rc = load_args(in, a, MIPME_EWALD_CHANNELS_BATCH_VERSION, who);
  if (rc) return rc;
  // everything the arguments alone decide, before anything touches a device
  if ((rc = check_ewald_pot(a.dtype, a.pot, who))) return rc;
  MIPME_REQUIRE(ecb_channels_ok(a.n_channels), "%s: n_channels must be in 2..8, got %d (one channel: mipme_ewald_batch)", who,
                int(a.n_channels));
  MIPME_REQUIRE((a.shift_format & 0xff) == 2 && !(a.shift_format & MIPME_ROWS_PADDED),
                "%s: the rows are read as 4-byte entries, other | code << 22 (shift_format 2), got shift_format %d", who,
                int(a.shift_format));
  MIPME_REQUIRE(a.n_frames >= 1 && a.n_frames <= kEbMaxFrames, "%s: n_frames must be in 1..2^20, got %d", who, int(a.n_frames));
  MIPME_REQUIRE(std::isfinite(a.lr_wavelength) && a.lr_wavelength > 0, "%s: lr_wavelength must be positive, got %g", who, a.lr_wavelength);
  MIPME_REQUIRE(a.atom_ptr && a.k_ptr && a.entry_ptr && a.device_table, "%s: NULL required buffer (atom_ptr, k_ptr, entry_ptr, device_table)",
                who);
  EbLayout L;
  MIPME_REQUIRE(eb_layout(ecb_shape(a.n_channels), a.n_frames, a.atom_ptr, a.k_ptr, a.entry_ptr, nullptr, a.cell_gradient != 0, L, nullptr,
                          nullptr),
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
  DT_SWITCH(a.dtype, ewald_channels_batch_c<float>(a, L, kp, sp), ewald_channels_batch_c<double>(a, L, kp, sp));
}

}  // extern "C"
