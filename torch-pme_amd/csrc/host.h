// Host-side interfaces between the libmipme translation units: the one declaration of every host function that is defined in
// one .hip file and called from another, the few structs they exchange, and the helpers every entry point shares.  Each file
// that defines or calls one of these includes this header, so a definition that drifts from its declaration does not compile.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"

namespace mipme {

template <typename T>
constexpr int dtype_of() {
  return sizeof(T) == 4 ? MIPME_F32 : MIPME_F64;
}

#define DT_SWITCH(dtype, CALL_F32, CALL_F64)                    \
  do {                                                          \
    if ((dtype) == MIPME_F32) return CALL_F32;                  \
    if ((dtype) == MIPME_F64) return CALL_F64;                  \
    mipme::set_error("invalid dtype %d", int(dtype));           \
    return MIPME_EINVAL;                                        \
  } while (0)

// grid of a grid-stride kernel over n items: one pass of `block`-thread blocks up to 8 per CU of a 256-CU device (block = 256)
inline unsigned stride_grid(int64_t n, int block) {
  return unsigned(std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, 2048)));
}

// Copy a caller's versioned argument struct into the library's own layout: only the first `size` bytes the caller
// compiled are read, everything after them stays zero (fields are only ever appended).
template <typename A>
int load_args(const A* in, A& out, unsigned version, const char* what) {
  MIPME_REQUIRE(in != nullptr, "%s: NULL argument struct", what);
  MIPME_REQUIRE(in->version == version, "%s: argument struct version %u, library expects %u", what, in->version, version);
  MIPME_REQUIRE(in->size >= 16 && in->size <= 4096, "%s: implausible argument struct size %u", what, in->size);
  memset(&out, 0, sizeof(A));
  memcpy(&out, in, in->size < sizeof(A) ? in->size : sizeof(A));
  return MIPME_OK;
}

// The rows a step entry point walks itself (mipme_combined_step, mipme_dipole_step): unpadded, 4-byte entries whose low
// kStepRowsAtomBits bits hold the partner (kCompactAtomBits of rows_body.h, which this header does not include)
static constexpr int kStepRowsAtomBits = 22;
inline int check_step_rows(int shift_format, int64_t n_atoms, const char* who) {
  MIPME_REQUIRE((shift_format & 0xff) == 2 && !(shift_format & MIPME_ROWS_PADDED),
                "%s: the rows are read as 4-byte entries, other | code << 22 (shift_format 2), got shift_format %d", who, shift_format);
  MIPME_REQUIRE(n_atoms > 0 && n_atoms <= (int64_t(1) << kStepRowsAtomBits), "%s: n_atoms must be in 1..2^22, got %lld", who,
                (long long)n_atoms);
  return MIPME_OK;
}

// ---- mesh.hip: particle <-> mesh without bins -------------------------------------------------------------------------------
template <typename T> int spread_impl(hipStream_t st, const mipme_mesh_t* m, int64_t n_atoms, const void* pos, const void* val, double scale,
                                      void* mesh);
template <typename T> int gather_impl(hipStream_t st, const mipme_mesh_t* m, int64_t n_atoms, const void* pos, const void* mesh, void* out);
template <typename T> int gather_epilogue_impl(hipStream_t st, const mipme_mesh_t* m, int64_t n_atoms, const void* pos, const void* mesh,
                                               const void* q, const void* qsum, double self_c, double bg_c, void* out, void* raw,
                                               int accumulate, void* nan_flag);
template <typename T> int gather_grad_impl(hipStream_t st, const mipme_mesh_t* m, int64_t n_atoms, const void* pos, const void* q,
                                           const void* gout, const void* phi, const void* chi, const void* gsum_dc, const void* gscale,
                                           double self_c, double bg_c, void* grad_pos, void* grad_q);

// ---- kfilter.hip: the FFT plan, the k-space filter and the fused convolution -------------------------------------------------
struct FftDims { int dtype, nx, ny, nz, batch; };
int fft_plan_create(int dtype, int nx, int ny, int nz, int batch, mipme_fft_plan** out);
int fft_plan_destroy(mipme_fft_plan* p);
FftDims fft_plan_dims(const mipme_fft_plan* p);
int fft_plan_batch(const mipme_fft_plan* p);
bool fft_plan_xfused(const mipme_fft_plan* p);
int* fft_plan_brick_count(const mipme_fft_plan* p);
int fft_forward(mipme_fft_plan* p, hipStream_t st, const void* in, void* out);
int fft_inverse(mipme_fft_plan* p, hipStream_t st, void* in, void* out);
int64_t xconv_blocks(const mipme_fft_plan* p);
int convolve_xfused(mipme_fft_plan* p, hipStream_t st, const void* mesh_in, const void* G, void* hat, void* mesh_out,
                    void* dc, int64_t G_stride, const mipme_mesh_t* cell_mesh, const mipme_potential_t* cell_pot,
                    void* cell_partials, void* epart, const void* sr_part, int64_t n_sr_part, const RowRideHost* rh,
                    void* err_flag, const ConvCell* cc);
// Every entry point that runs a convolution on the plan calls this first: it clears what a plane spread tells the convolution
// ("forward planes done", their parts, "y columns pending"), so that a call that failed half-way cannot make the next one skip
// its forward planes.
void fft_plan_begin_step(mipme_fft_plan* p);
bool fft_plan_plane_forward_ok(const mipme_fft_plan* p);
bool fft_plan_plane_forward_ok_batched(const mipme_fft_plan* p);
void fft_plan_set_forward_done(mipme_fft_plan* p, bool done, int parts);
void fft_plan_set_forward_ycols(mipme_fft_plan* p, bool pending);
void* fft_plan_hat_parts(mipme_fft_plan* p, hipStream_t st, int n_more);
// MIPME_INV_PLANE_SPLIT (docs/SWITCHES.md): workgroups per x plane of the single-launch inverse (y,z) planes -- 1, 2 or 4; unset
// or anything else: 0 = chosen from the mesh (inverse_plane_split_auto).  Read at every launch (a captured graph keeps what it was
// captured with).
inline int inverse_plane_split_setting() {
  const char* e = getenv("MIPME_INV_PLANE_SPLIT");
  const int s = e ? atoi(e) : 0;
  return (s == 1 || s == 2 || s == 4) ? s : 0;
}
// The default: the largest S of 4, 2 whose S x nx plane workgroups are at most 128, half the CUs -- 256 workgroups of 16 waves
// take every CU and the slot riders queue behind them (64^3 fp32: the launch 7.69 us unsplit, 7.04 at S = 2, 9.15 at S = 4; 32^3
// fp64: the step 44.68 / 44.86 / 44.00 us; profiles/inverse_planes_split.txt) -- and whose transform is long enough (ny >= 4 S).
static constexpr int kInvPlaneSplitMaxWorkgroups = 128;
inline int inverse_plane_split_auto(int nx, int ny) {
  for (int s = 4; s > 1; s >>= 1)
    if (s * nx <= kInvPlaneSplitMaxWorkgroups && ny >= 4 * s) return s;
  return 1;
}
// (mipme_last_inverse_split: workgroups per plane of the last inverse (y,z) transform of a fused convolution; 1: the unsplit kernels)
void note_inverse_split(int split);
// *out = the plan's scratch for the energy partial sums of a gather tail (`bytes` of it, zeroed when first allocated), or
// MIPME_EINVAL with the advice to warm up before a stream capture
int fft_plan_tail_scratch(mipme_fft_plan* p, int64_t bytes, void** out);
template <typename T> int kfilter_build_impl(hipStream_t st, const mipme_mesh_t* m, const mipme_potential_t* pot, void* G);
template <typename T> int kfilter_deriv_impl(hipStream_t st, const mipme_mesh_t* m, const mipme_potential_t* pot, void* D);
template <typename T> int apply_filter_impl(hipStream_t st, int64_t Mh, int C, const void* hat, const void* G, void* out, void* dc);
template <typename T> int apply_filter_cellgrad_impl(hipStream_t st, const mipme_mesh_t* m, const mipme_potential_t* pot, const void* psi_hat,
                                                     const void* rho_hat, const void* G, void* out, void* dc, void* partials);
int64_t cellgrad_blocks(const mipme_mesh_t* m);
int64_t cellgrad_scratch_doubles();
template <typename T> int cellgrad_finalize_impl(hipStream_t st, const mipme_mesh_t* m, double bg, int64_t n_atoms, void* partials,
                                                 const void* pos, const void* grad_pos, const void* gout, const void* phi_atoms,
                                                 const void* rho_dc, const void* psi_dc, const void* energy_scale, void* grad_cell,
                                                 int64_t kgrid_blocks, const void* field, const void* q);
template <typename T> int cell_tail_finalize_impl(hipStream_t st, const mipme_mesh_t* m, double bg, double pair_scale, int64_t n_rows,
                                                  int64_t n_bricks, const void* rows, const void* rpart, const void* dc, const void* seed, void* out,
                                                  const GatherTailHost* slab = nullptr);

// ---- rspace.hip: pair-list kernels -------------------------------------------------------------------------------------------
template <typename T, typename I> int rspace_forward_impl(hipStream_t st, int64_t P, int64_t N, int C, const void* pairs, const void* dist, const void* q,
                                                          const void* mask, int full, const mipme_potential_t* pot, int accumulate, void* out);
template <typename T, typename I> int rspace_backward_impl(hipStream_t st, int64_t P, int64_t N, int C, const void* pairs, const void* dist,
                                                           const void* q, const void* mask, int full, const mipme_potential_t* pot, const void* g,
                                                           const void* gscale, void* grad_d, void* grad_q);
template <typename T, typename I> int distance_forward_impl(hipStream_t st, int64_t P, const void* pairs, const void* pos, const void* cell,
                                                            const void* shifts, void* out);
template <typename T, typename I> int distance_backward_impl(hipStream_t st, int64_t P, int64_t N, const void* pairs, const void* pos, const void* cell,
                                                             const void* shifts, const void* grad_d, void* partials, void* grad_pos, void* grad_cell);
template <typename T> int pack_pair_shifts_impl(hipStream_t st, int64_t P, const void* shifts, void* packed, void* flag);
template <typename T> int distance_forward_packed_impl(hipStream_t st, int64_t P, const void* pairs, const void* packed, const void* pos,
                                                       const void* cell, void* out);
int64_t pair_partials_blocks(int64_t P);

// ---- bricks.hip: the brick-binned single-frame path --------------------------------------------------------------------------
bool bricks_supported(const mipme_mesh_t* m, int dtype);
int64_t bins_bytes(const mipme_mesh_t* m, int64_t N, int dtype);
int plane_bins_capacity(const mipme_mesh_t* m, int64_t N, int dtype);
int plane_bands(const mipme_mesh_t* m, int dtype);
const void* bins_epart(const mipme_mesh_t* m, int64_t N, int dtype, void* bins, int64_t* n);
bool sr_job_fusable(const mipme_sr_job_t* job);
template <typename T> int bins_build(hipStream_t st, const mipme_mesh_t* m, int64_t n_atoms, const void* pos, void* bins, int* live,
                                     const void* q, void* atom_rec, bool plane_lists = false, bool defer_slots = false);
bool plane_spread_runs(const mipme_mesh_t* m, int64_t N, int dtype, const mipme_sr_job_t* job, const PlaneHost* ph, bool forward);
bool bins_defer_slots(const mipme_mesh_t* m, int64_t N, int dtype, const mipme_sr_job_t* job, const PlaneHost* ph);
SlotRider bins_slot_rider(const mipme_mesh_t* m, int64_t N, int dtype, void* bins, const void* pos, const void* q);
template <typename T> int spread_bricks(hipStream_t st, const mipme_mesh_t* m, int64_t N, void* bins, const void* val, double scale, void* mesh,
                                        int* clear_count, const mipme_sr_job_t* job, bool want_epart, double* cpart, const PlaneHost* ph = nullptr,
                                        bool* used_planes = nullptr);
template <typename T> int gather_bricks(hipStream_t st, const mipme_mesh_t* m, int64_t N, void* bins, const void* mesh, const void* q,
                                        const void* qsum, double self_c, double bg_c, void* out, void* raw, int accumulate, void* field,
                                        const GatherTailHost* th, void* nan_flag, int* live);
template <typename T> int gather_grad_bricks(hipStream_t st, const mipme_mesh_t* m, int64_t N, void* bins, const void* q, const void* gout,
                                             const void* phi, const void* chi, const void* psi_dc, const void* gscale, double self_c,
                                             double bg_c, void* grad_pos, void* grad_q);

// ---- live.hip: the MD step on live bins --------------------------------------------------------------------------------------
bool live_supported(const mipme_mesh_t* m, int64_t N, int dtype);
int64_t live_lists_ints(const mipme_mesh_t* m, int64_t N);
template <typename T> int live_rebin(hipStream_t st, const mipme_mesh_t* m, int64_t N, const void* rec4, void* bins, void* lists, void* host_flags);
template <typename T> int live_spread(hipStream_t st, const mipme_mesh_t* m, int64_t N, const void* rec4, void* bins, void* lists, void* mesh,
                                      const mipme_sr_job_t* job, void* host_flags, double* cpart);
template <typename T> int live_gather(hipStream_t st, const mipme_mesh_t* m, int64_t N, const void* rec4, void* bins, void* lists, const void* mesh,
                                      const void* qsum, double self_c, double bg_c, void* out, void* field, const GatherTailHost* th, void* nan_flag);

// ---- shared by the entry points of a step (api.hip, frames.hip) --------------------------------------------------------------
// self / background corrections: potentials/coulomb.py:144-158, potentials/inversepowerlaw.py:143-166
inline void correction_terms(const mipme_potential_t* pot, double& self_c, double& bg_c) {
  const int p = pot->kind == MIPME_COULOMB ? 1 : pot->exponent;
  const double two_s2 = 2.0 * pot->smearing * pot->smearing;
  self_c = pot->prefactor / std::tgamma(0.5 * p + 1.0) / std::pow(two_s2, 0.5 * p);
  if (p >= 3)
    bg_c = 0.0;
  else
    bg_c = pot->prefactor * std::pow(3.14159265358979323846, 1.5) * std::pow(two_s2, 0.5 * (3 - p)) /
           ((3 - p) * std::tgamma(0.5 * p));
}

// MIPME_PLANE_PARTS: workgroups per plane of the plane spread (default 2, at most kPlanePartsMax; read once per process)
static constexpr int kPlanePartsMax = 8;
inline int plane_spread_parts_setting() {
  static const int parts_env = [] { const char* e = getenv("MIPME_PLANE_PARTS"); return e ? atoi(e) : 2; }();
  return parts_env < 1 ? 1 : (parts_env > kPlanePartsMax ? kPlanePartsMax : parts_env);
}

// The plan's scratch behind a gather tail: the energy partial sums of the convolution's x stage, one per block, and behind them
// the pair kernel's sums, which that stage reduces to two more per block
inline int tail_attach_plan_scratch(GatherTailHost& tail, mipme_fft_plan* plan) {
  void* scratch = nullptr;
  tail.n_k = xconv_blocks(plan);
  tail.sr_reduced = 1;
  // (+ the moments of a slab term and the scratch of their launch: the size of the plan's buffer cannot change later)
  const int rc = fft_plan_tail_scratch(plan, int64_t(sizeof(double)) * (3 * tail.n_k + kSlabWork), &scratch);
  tail.epart_k = scratch;
  tail.slab_mom = scratch ? (double*)scratch + 3 * tail.n_k : nullptr;
  return rc;
}

// The slab term of a gather tail (mipme.h, slab = axis + 1; the caller has checked the range, one channel and 1/r)
inline void tail_attach_slab(GatherTailHost& tail, const mipme_mesh_t* m, const mipme_potential_t* pot, int slab) {
  const double* a = m->cell + 3 * (slab - 1);
  tail.slab = slab;
  tail.slab_c0 = pot->prefactor * 4.0 * 3.14159265358979323846 / m->volume;
  tail.slab_L = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
}

// The energy of a gather tail also goes to a log (mipme.h, energy_log): needs the log's cursor and a capacity the device's int
// holds.  `needs`: the start of the refusal, up to and including "energy_log_cursor".
inline int tail_attach_energy_log(GatherTailHost& tail, void* log, void* cursor, int64_t capacity, const char* needs) {
  MIPME_REQUIRE(cursor && capacity > 0 && capacity <= INT_MAX, "%s and a capacity > 0 (at most %d)", needs, INT_MAX);
  tail.elog = (double*)log;
  tail.elog_cursor = (int*)cursor;
  tail.elog_cap = int(capacity);
  return MIPME_OK;
}

// cell_work of an energy step's cell gradient (mipme_cell_tail_work), in doubles:
// [rows 25 per rider][rpart 9 per brick][cwave 9 per wavefront of the pair kernel][wbuf: one real per half-grid point]
struct CellWork {
  int64_t n_riders, n_bricks, n_waves;
  double *rows, *rpart, *cwave;
  void* wbuf;
  int64_t total;
};
inline CellWork cell_work_layout(const mipme_mesh_t* m, int64_t N, void* base) {
  CellWork w;
  const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
  w.n_riders = std::min<int64_t>(256, std::max<int64_t>(8, Mh / 2048));  // ~2 k-points per rider thread (1024 threads)
  w.n_bricks = int64_t((m->nx + 7) / 8) * ((m->ny + 7) / 8) * ((m->nz + 7) / 8);
  w.n_waves = (N + 3) / 4;  // 16 lanes per row: 4 rows per wavefront (rows_body.h)
  double* b = (double*)base;
  w.rows = b;
  w.rpart = w.rows + 25 * w.n_riders;
  w.cwave = w.rpart + 9 * w.n_bricks;
  w.wbuf = w.cwave + 9 * w.n_waves;
  w.total = 25 * w.n_riders + 9 * w.n_bricks + 9 * w.n_waves + Mh;  // (wbuf: Mh reals of <= 8 bytes)
  return w;
}

// ---- the cell gradient of a frame batch (mipme_frames_table_contract / mipme_frames_step) ---------------------------------------
// What the batch's cell riders and its finalize launch read of one frame: a record per frame behind the FrameDev array of the
// frames table (host and device copy alike).  n_riders == 0: the frame's batch carries no cell gradient.
struct FrameCellRec {
  mipme_mesh_t mesh;
  double bg, pair_scale;   // background term; 0.5 x the force scale of the pair list
  const void* wbuf;        // (nx, ny, nzh) reals: the x stage's w = mu |rho^|^2 of this frame
  const void* dG4;         // (nx, ny, nzh, 4) reals: the frame's derivative table
  const double* cwave;     // [9 * n_waves]
  double* rows;            // [n_riders][25]
  const double* rpart;     // [9 * n_bricks]
  const void* dc;          // 1 real
  const void* seed;        // device scalar, nullable (= 1)
  void* out;               // 27 reals: mesh part, pair part, sum
  int n_waves, n_riders, n_bricks, _pad;
  // the slab term of the frame (mipme_frames_table_slab; read by the SLAB finalize launch alone): as GatherTail's fields.
  // A fully periodic frame of a slab batch has c0 = 0 and moments of zero: every term it adds is an exact zero
  const double* slab_mom;
  double slab_c0, slab_L;
  int slab_axis, _pad_slab;
};
template <typename T> int frames_cell_riders(hipStream_t st, const FrameCellRec* recs, int n_frames, int n_riders, int nx, int ny,
                                             int nzh, const double* epart_k, int n_k);
template <typename T> int frames_cell_finalize(hipStream_t st, const FrameCellRec* recs, int n_frames);
// frames_slab.hip: the same launch with the slab term of every frame (FrameCellRec::slab_*)
template <typename T> int frames_slab_cell_finalize(hipStream_t st, const FrameCellRec* recs, int n_frames);

// cell_work of a frame batch, in doubles: `stride` per frame (frames_cell_stride of the largest frame, or more), laid out as
// [wbuf: n_frames x Mh reals, contiguous -- the batched x stage writes entry c at c * Mh -- in the first n_frames * Mh doubles]
// [per frame, stride - Mh doubles apart: rows 25 per rider | rpart 9 per brick | cwave 9 per wavefront of the row blocks]
// The row blocks of the co-scheduled launch write a slot for EVERY wavefront they hold (kRowsPerSpreadBlock rows, a wavefront per
// four of them), so cwave is sized by whole blocks; the riders read the (N + 3) / 4 wavefronts that hold a row.
inline int64_t frames_cell_stride(const mipme_mesh_t* m, int64_t N) {
  const CellWork w = cell_work_layout(m, N, nullptr);
  const int64_t rows_per_block = 32, waves_per_block = 8;  // (frames.hip: static_assert against SPREAD_THREADS / kRowLanes)
  const int64_t waves = (N + rows_per_block - 1) / rows_per_block * waves_per_block;
  return 25 * w.n_riders + 9 * w.n_bricks + 9 * waves + int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
}
inline CellWork frames_cell_layout(const mipme_mesh_t* m, int64_t N, int n_frames, int frame, void* base, int64_t stride,
                                   size_t real_bytes) {
  CellWork w = cell_work_layout(m, N, nullptr);
  const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
  w.wbuf = (char*)base + size_t(frame) * size_t(Mh) * real_bytes;
  w.rows = (double*)base + int64_t(n_frames) * Mh + int64_t(frame) * (stride - Mh);
  w.rpart = w.rows + 25 * w.n_riders;
  w.cwave = w.rpart + 9 * w.n_bricks;
  w.total = stride;
  return w;
}

}  // namespace mipme
