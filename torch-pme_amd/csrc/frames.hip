// Independent frames in one launch (include/mipme.h: mipme_frames_*; SURVEY 8(e): the frames a rank owns).
// Device bodies: bricks_device.h (the single-frame kernels' bodies, blockIdx.y = frame); the per-frame record: frames_device.h.
// The instantiations of the pair sum that also form the cell sums live in frames_cell.hip, a translation unit of their own, so that
// the kernels of this file -- all the flags-off step launches -- compile to what they were (tools/device_digest.py --kernels).
// The launches of a batch with the 2-D periodic (slab) term live in frames_slab.hip for the same reason; their entry points --
// host code -- are here (mipme_frames_table_slab, mipme_frames_slab_step).
#include "frames_device.h"

namespace mipme {
// ---- independent frames in one launch (include/mipme.h: mipme_frames_*) -----------------------------------------
// blockIdx.y = frame; every kernel reads its frame's arguments from a device-resident table (built once per batch), so a
// step of F frames is as many launches as a step of one frame.  The bodies are the single-frame kernels' bodies.
template <int SCHEME, int N, typename T>
__global__ __launch_bounds__(256) void frames_bin_atoms_kernel(const FrameDev<T>* __restrict__ table) {
  const FrameDev<T>& f = table[blockIdx.y];
  if (int64_t(blockIdx.x) * 256 >= f.N) return;
  bin_atoms_body<SCHEME, N, T>(f.g, f.bg, f.bins, f.N, f.pos, f.over_brick, f.rec, f.wts, f.q, f.atom_rec, blockIdx.x, nullptr,
                               const_cast<T*>(f.spread.qs));
}

template <int N, typename T, int PFAST, bool COMPACT>
__global__ __launch_bounds__(SPREAD_THREADS, (sizeof(T) == 4 && COMPACT) ? 6 : 1) void frames_spread_rows_kernel(const FrameDev<T>* __restrict__ table) {
  const FrameDev<T>& f = table[blockIdx.y];
  const unsigned n_spread = unsigned(f.bg.nb);
  if (blockIdx.x < n_spread)
    spread_brick_body<N, T>(f.spread, blockIdx.x);
  else if (blockIdx.x - n_spread < f.n_row_blocks) {
    extern __shared__ __attribute__((aligned(16))) char smem_rows[];  // see spread_rows_kernel
    AtomRecord<T>* tab = reinterpret_cast<AtomRecord<T>*>(smem_rows);
    if constexpr (COMPACT && std::is_same<T, float>::value) {
      if (!f.rows.dist_out) {
        sr_rows_pk_body<PFAST, SPREAD_THREADS>(f.rows, blockIdx.x - n_spread, tab);
        return;
      }
    }
#if MIPME_ROW_LANES == 16
    if constexpr (COMPACT && std::is_same<T, double>::value && (PFAST == 1 || PFAST == 6)) {
      if (!f.rows.dist_out) {
        sr_rows_f64_body<SPREAD_THREADS, false, PFAST>(f.rows, blockIdx.x - n_spread, smem_rows);
        return;
      }
    }
#endif
    sr_fused_rows_body<T, kPotForce, false, PFAST, false, true, SPREAD_THREADS, 2, COMPACT>(f.rows, blockIdx.x - n_spread, tab);
  }
}

// Plane spread for frame batches (round 5): blockIdx.y = frame; the first nx * parts workgroups of a frame are plane workgroups
// (plane_spread_yz_body: part 0 of frame f into its block of the batched half-complex mesh, the other parts into the plan's part
// buffers), the rest its row blocks.  `pa` holds the frame-independent fields; frame_stride = complex values per frame.
template <int SCHEME, int N, typename T, int PFAST, bool COMPACT>
__global__ __launch_bounds__(SPREAD_THREADS, (sizeof(T) == 4 && COMPACT) ? 6 : 1) void frames_plane_rows_kernel(const FrameDev<T>* __restrict__ table,
                                                                                                        PlaneArgs<T> pa, int64_t frame_stride) {
  const FrameDev<T>& f = table[blockIdx.y];
  const unsigned n_items = unsigned(f.g.nx) * unsigned(pa.parts);
  extern __shared__ __attribute__((aligned(16))) char smem_fp[];
  if (blockIdx.x < n_items) {
    pa.hat += int64_t(blockIdx.y) * frame_stride;
    if (pa.hat_more) pa.hat_more += int64_t(blockIdx.y) * frame_stride;
    plane_spread_yz_body<SCHEME, N, T>(f.spread, pa, blockIdx.x, smem_fp);
  } else if (blockIdx.x - n_items < f.n_row_blocks) {
    cosched_row_block<T, PFAST, COMPACT, false>(f.rows, blockIdx.x - n_items, smem_fp);
  }
}
template <int N, typename T>
__global__ __launch_bounds__(GATHER_THREADS) void frames_gather_kernel(const FrameDev<T>* __restrict__ table) {
  const FrameDev<T>& f = table[blockIdx.y];
  gather_brick_body<N, true, T>(f.g, f.bg, 1, f.bins, f.rec, f.wts, f.phi_mesh, f.q, f.dc, f.inv_vol, f.self_c, f.bg_c, true,
                                f.out, nullptr, f.field, blockIdx.x);
}

// the same with the tail: every frame of the batch carries tail scratch
template <int N, typename T>
__global__ __launch_bounds__(GATHER_THREADS) void frames_gather_tail_kernel(const FrameDev<T>* __restrict__ table,
                                                                           const double* __restrict__ epart_k, int n_k) {
  const FrameDev<T>& f = table[blockIdx.y];
  GatherTail<T> tail = f.tail;
  tail.epart_k = epart_k + int64_t(blockIdx.y) * n_k;  // the x stage writes one block of partial sums per batch entry
  tail.n_k = n_k;
  gather_brick_body<N, true, T, true>(f.g, f.bg, 1, f.bins, f.rec, f.wts, f.phi_mesh, f.q, f.dc, f.inv_vol, f.self_c, f.bg_c,
                                      true, f.out, nullptr, f.field, blockIdx.x, &tail);
}

// energy[f] = sum_a q_a V_a: one workgroup per frame, fixed summation order
template <typename T>
__global__ __launch_bounds__(1024) void frames_energy_kernel(const FrameDev<T>* __restrict__ table) {
  const FrameDev<T>& f = table[blockIdx.x];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < f.N; i += 1024) acc += double(f.q[i]) * double(f.out[i]);
  __shared__ double red[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < 16; ++w) tot += red[w];
    f.energy[0] = T(tot);
  }
}

// grad_positions[f][a] = gscale[f] q_a (c force_a + field_a)
template <typename T>
__global__ __launch_bounds__(256) void frames_finalize_kernel(const FrameDev<T>* __restrict__ table,
                                                             const T* __restrict__ gscale) {
  const FrameDev<T>& f = table[blockIdx.y];
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= 3 * f.N) return;
  f.grad_pos[t] = gscale[blockIdx.y] * f.q[t / 3] * (f.force_scale * f.force[t] + f.field[t]);
}

// int32 words of a frame's counter buffer: brick counters + overflow counter, and -- when the plane spread applies to the frame
// (plane_list_capacity) -- the plane lists' counters + their overflow counter
static int64_t frame_counter_ints(const mipme_mesh_t* m, int64_t n_atoms, int dtype) {
  const BrickGeom bg = make_brick_geom(m);
  int64_t n = int64_t(bg.nb) + 1;
  if (plane_list_capacity(m, n_atoms, dtype) > 0 && plane_fits_cosched(m, dtype)) n += int64_t(m->nx) * kPlaneSub + 1;
  return n;
}
static bool frame_plane_lists(const mipme_frame_t& f, int dtype) {
  // (whole planes only: the frame batches have no band variant; larger planes keep the bricks there)
  return plane_list_capacity(&f.mesh, f.n_atoms, dtype) > 0 && plane_fits_cosched(&f.mesh, dtype) &&
         int64_t(f.counter_ints) == frame_counter_ints(&f.mesh, f.n_atoms, dtype);
}
int64_t frames_counter_ints(const mipme_mesh_t* m, int64_t n_atoms, int dtype) { return frame_counter_ints(m, n_atoms, dtype); }

int frames_check(int dtype, int n_frames, const mipme_frame_t* fr) {  // (frames_device.h: frames_cells.hip's entry point calls it too)
  MIPME_REQUIRE(n_frames > 0 && fr, "no frames");
  MIPME_REQUIRE(dtype == MIPME_F32 || dtype == MIPME_F64, "invalid dtype %d", dtype);
  const mipme_mesh_t& m0 = fr[0].mesh;
  for (int k = 0; k < n_frames; ++k) {
    const mipme_frame_t& f = fr[k];
    int rc = validate_mesh(&f.mesh);
    if (rc) return rc;
    MIPME_REQUIRE(f.mesh.nx == m0.nx && f.mesh.ny == m0.ny && f.mesh.nz == m0.nz && f.mesh.scheme == m0.scheme &&
                      f.mesh.order == m0.order && f.mesh.n_channels == 1,
                  "frame %d: all frames need the same mesh, scheme and order and a single channel", k);
    MIPME_REQUIRE(bricks_supported(&f.mesh, dtype) && make_brick_geom(&f.mesh).nb <= 1024,
                  "frame %d: mesh %d x %d x %d is outside the brick kernels' range", k, f.mesh.nx, f.mesh.ny, f.mesh.nz);
    MIPME_REQUIRE(f.n_atoms > 0 && f.positions && f.charges && f.cell && f.atom_bins && f.brick_counters && f.row_ptr &&
                      f.entries_shift && f.entries && f.records && f.rho_mesh && f.phi_mesh && f.dc && f.out && f.force &&
                      f.field && f.energy && f.grad_positions,
                  "frame %d: NULL buffer or no atoms", k);
    // counter_ints was padding before round 5: a caller built against the old header may pass garbage.  Only the three
    // legal values are accepted, so that garbage cannot switch the plane lists on (they write behind the brick counters)
    MIPME_REQUIRE(f.counter_ints == 0 || int64_t(f.counter_ints) == int64_t(make_brick_geom(&f.mesh).nb) + 1 ||
                      int64_t(f.counter_ints) == frame_counter_ints(&f.mesh, f.n_atoms, dtype),
                  "frame %d: counter_ints = %d is neither 0, bricks + 1 = %d nor mipme_frames_counter_ints() = %lld (zero-initialise "
                  "mipme_frame_t)", k, f.counter_ints, make_brick_geom(&f.mesh).nb + 1,
                  (long long)frame_counter_ints(&f.mesh, f.n_atoms, dtype));
    MIPME_REQUIRE((f.shift_format == kShiftTable || f.shift_format == kShiftTable32) && f.shift_format == fr[0].shift_format,
                  "frame %d: the frames path needs the table shift format (1 or 2), the same for every frame", k);
  }
  return MIPME_OK;
}

template <typename T>
static int frames_table_build_t(int n_frames, const mipme_frame_t* fr, const mipme_potential_t* pot, void* host_table) {
  SRPot s;
  int rc = make_srpot(pot, s);
  if (rc) return rc;
  const int pfast = fast_rs_exponent(s);
  MIPME_REQUIRE(pot->smearing > 0 && (pfast == 1 || pfast == 6), "the frames path covers 1/r and 1/r^6 with a smearing");
  const FastRS cf = make_fast_rs(s);
  double self_c, bg_c;
  correction_terms(pot, self_c, bg_c);
  const int dtype = dtype_of<T>();
  FrameDev<T>* out = (FrameDev<T>*)host_table;
  for (int k = 0; k < n_frames; ++k) {
    const mipme_frame_t& f = fr[k];
    const mipme_mesh_t* m = &f.mesh;
    const BinsView v = bins_view(m, f.n_atoms, dtype, f.atom_bins);
    FrameDev<T> d;
    d.g = make_geom(m);
    d.bg = make_brick_geom(m);
    d.N = f.n_atoms;
    d.pos = (const T*)f.positions;
    d.q = (const T*)f.charges;
    d.bins = v.idx;
    d.bins.live = (int*)f.brick_counters;
    d.over_brick = v.over_brick;
    d.rec = v.rec;
    d.wts = (T*)v.wts;
    d.atom_rec = (AtomRecord<T>*)f.records;
    d.even = (m->order % 2) == 0;
    d.spread.g = d.g;
    d.spread.bg = d.bg;
    d.spread.C = 1;
    d.spread.bins = d.bins;
    d.spread.from_live = true;
    d.spread.rec = v.rec;
    d.spread.wts = (const T*)v.wts;
    d.spread.val = (const T*)f.charges;
    d.spread.scale = T(1);
    d.spread.mesh = (T*)f.rho_mesh;
    d.spread.stage_rows = spread_stage_rows(m->order, sizeof(T));
    d.spread.skip = nullptr;
    d.spread.det = false;  // (the frames path keeps the one-pass binning: MIPME_DETERMINISTIC covers single-frame evaluations)
    d.spread.qs = (const T*)v.qs;  // the charge by bin slot (written by the binning pass: bricks' staging and the plane spread)
    if (frame_plane_lists(f, dtype)) {  // plane lists: counters behind the brick counters (mipme_frames_counter_ints)
      d.bins.plive = d.bins.live + d.bg.nb + 1;
    } else {
      d.bins.pcap = 0;
      d.bins.wmax = nullptr;
    }
    d.spread.bins = d.bins;
    d.rows = make_fused_rows_args<T>(s, cf, f.n_atoms, f.row_ptr, f.entries_shift, f.entries, nullptr, f.positions, f.records,
                                     f.cell, f.charges, nullptr, 0, f.full_list ? 0 : 1, f.full_list, 0, f.out, f.force, nullptr,
                                     f.dist_out);
    const int64_t rpb = SPREAD_THREADS / kRowLanes;
    d.n_row_blocks = unsigned((f.n_atoms + rpb - 1) / rpb);
    d.phi_mesh = (const T*)f.phi_mesh;
    d.dc = (const T*)f.dc;
    d.inv_vol = T(1.0 / m->volume);
    d.self_c = T(self_c);
    d.bg_c = T(bg_c);
    d.out = (T*)f.out;
    d.field = (T*)f.field;
    d.energy = (T*)f.energy;
    d.force = (const T*)f.force;
    d.grad_pos = (T*)f.grad_positions;
    d.force_scale = f.full_list ? T(0.5) : T(1);
    // energy + forces; grad_q and the cell sums: mipme_frames_table_contract.  epart_k / n_k per batch entry: set by the gather
    // kernel (plan scratch)
    GatherTailHost th{};
    th.force = f.force;
    th.force_scale = f.full_list ? 0.5 : 1.0;
    th.seed = f.grad_seed;
    th.grad_pos = f.grad_positions;
    th.energy = f.energy;
    d.tail = make_gather_tail<T>(th, v.epart, int((f.n_atoms + 64 / kRowLanes - 1) / (64 / kRowLanes)), nullptr, nullptr);
    d.use_tail = f.use_tail != 0;
    d.rows.epart = f.use_tail ? v.epart : nullptr;
    out[k] = d;
  }
  return MIPME_OK;
}

// cell_work (nullable): the batch's cell gradient -- the CELL instantiations of the pair sum, the x stage's store of w, and behind
// the convolution the riders of every frame in one launch and the finalize launch (the contract is in the table already)
// slab: the table carries the slab term (mipme_frames_table_slab) -- the moments of every frame in one launch ahead of everything
// else, then the gather and the finalize launch compiled with the term (frames_slab.hip); every frame has its tail
template <typename T>
static int frames_forward_t(mipme_fft_plan* plan, hipStream_t st, int n_frames, const mipme_frame_t* fr, const void* table,
                            const void* G, int64_t G_stride, void* rho_all, void* hat_all, void* phi_all, void* dc_all,
                            int pfast, void* cell_work = nullptr, bool slab = false) {
  const FrameDev<T>* tb = (const FrameDev<T>*)table;
  const mipme_mesh_t* m = &fr[0].mesh;
  const BrickGeom bg = make_brick_geom(m);
  int64_t max_atoms = 0;
  for (int k = 0; k < n_frames; ++k) max_atoms = std::max<int64_t>(max_atoms, fr[k].n_atoms);
  const unsigned atom_blocks = unsigned((max_atoms + 255) / 256);
  const unsigned F = unsigned(n_frames);
  if (slab) {
    const int rcs = frames_slab_moments<T>(st, tb, n_frames, max_atoms);
    if (rcs) return rcs;
  }
  MIPME_DISPATCH_STENCIL_B(m->scheme, m->order, (frames_bin_atoms_kernel<S, N, T><<<dim3(atom_blocks, F), 256, 0, st>>>(tb)));
  MIPME_LAUNCH_CHECK();
  const int stage_rows = spread_stage_rows(m->order, sizeof(T));
  const size_t lds = spread_lds_bytes(m->order, sizeof(T), stage_rows);
  const int64_t rpb = SPREAD_THREADS / kRowLanes;
  const unsigned grid_x = unsigned(bg.nb) + unsigned((max_atoms + rpb - 1) / rpb);
  const bool compact = fr[0].shift_format == kShiftTable32;  // frames_check: the same format for every frame
  // plane spread (every frame of the batch has its plane lists: frame_plane_lists, decided when the table was built)
  bool planes = fft_plan_plane_forward_ok_batched(plan);
  for (int k = 0; k < n_frames && planes; ++k) planes = frame_plane_lists(fr[k], dtype_of<T>());
  fft_plan_begin_step(plan);
  int rc0 = MIPME_OK;
  if (!planes) note_cosched_kernel("frames_spread_rows_kernel");
  if (planes) {
    PlaneArgs<T> pa;
    size_t need = 0;
    plane_lds_layout<T>(m->ny, m->nz, pa, need);
    const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
    pa.hat = (Cplx<T>*)hat_all;
    // a batch has its frames for parallelism: as many parts as keep the plane workgroups of the launch at or below 128 (the
    // single-frame optimum at 64^3: 2 x 64); measured on 8 x 8000 ions / 32^3 fp64: 1 part 0.1243, 2 parts 0.1291, 3 parts
    // 0.1322 ms (bricks 0.1336); 16 x 1000 atoms / 32^3 fp32: 0.0569 / 0.0633 / 0.0691 (bricks 0.0600)
    pa.parts = plane_spread_parts_setting();
    while (pa.parts > 1 && int64_t(pa.parts) * m->nx * n_frames > 128) --pa.parts;
    if (pa.parts > 1) {
      pa.hat_more = (Cplx<T>*)fft_plan_hat_parts(plan, st, kPlanePartsMax - 1);
      pa.more_stride = Mh * n_frames;
      if (!pa.hat_more) pa.parts = 1;
    }
    while ((1 << pa.logny) < m->ny) ++pa.logny;
    while ((1 << pa.loglz) < m->nz / 2) ++pa.loglz;
    const size_t rows_lds = sizeof(T) * size_t(SPREAD_WAVES) * BRICK_PTS;
    const size_t plds = need > rows_lds ? need : rows_lds;
    const unsigned pgrid_x = unsigned(m->nx) * unsigned(pa.parts) + unsigned((max_atoms + rpb - 1) / rpb);
#define MIPME_FRAMES_PLANES(PF, CO) \
  MIPME_DISPATCH_STENCIL_B(m->scheme, m->order, (frames_plane_rows_kernel<S, N, T, PF, CO><<<dim3(pgrid_x, F), SPREAD_THREADS, plds, st>>>(tb, pa, Mh)))
    note_cosched_kernel("frames_plane_rows_kernel");
    if (cell_work) {  // (4-byte entries: mipme_frames_step has checked them for every frame; frames_cell.hip)
      if ((rc0 = frames_cell_plane_rows<T>(st, m->scheme, m->order, pfast, dim3(pgrid_x, F), plds, tb, pa, Mh))) return rc0;
    } else if (pfast == 1 && compact)
      MIPME_FRAMES_PLANES(1, true);
    else if (pfast == 1)
      MIPME_FRAMES_PLANES(1, false);
    else if (compact)
      MIPME_FRAMES_PLANES(6, true);
    else
      MIPME_FRAMES_PLANES(6, false);
#undef MIPME_FRAMES_PLANES
    fft_plan_set_forward_done(plan, true, pa.parts);
  } else if (cell_work) {
    if ((rc0 = frames_cell_spread_rows<T>(st, m->scheme, m->order, pfast, dim3(grid_x, F), lds, tb))) return rc0;
  } else if (pfast == 1 && compact)
    MIPME_DISPATCH_STENCIL_B(m->scheme, m->order,
                             ((void)S, frames_spread_rows_kernel<N, T, 1, true><<<dim3(grid_x, F), SPREAD_THREADS, lds, st>>>(tb)));
  else if (pfast == 1)
    MIPME_DISPATCH_STENCIL_B(m->scheme, m->order,
                             ((void)S, frames_spread_rows_kernel<N, T, 1, false><<<dim3(grid_x, F), SPREAD_THREADS, lds, st>>>(tb)));
  else if (compact)
    MIPME_DISPATCH_STENCIL_B(m->scheme, m->order,
                             ((void)S, frames_spread_rows_kernel<N, T, 6, true><<<dim3(grid_x, F), SPREAD_THREADS, lds, st>>>(tb)));
  else
    MIPME_DISPATCH_STENCIL_B(m->scheme, m->order,
                             ((void)S, frames_spread_rows_kernel<N, T, 6, false><<<dim3(grid_x, F), SPREAD_THREADS, lds, st>>>(tb)));
  MIPME_LAUNCH_CHECK();
  note_gather_pairs(0);  // (the batches' gathers take one atom per lane group and pass)
  bool all_tail = true;
  for (int k = 0; k < n_frames; ++k) all_tail = all_tail && fr[k].use_tail != 0;
  const int64_t n_k = xconv_blocks(plan) / n_frames;  // blocks of the x stage per batch entry
  void* epart_k = nullptr;
  int rc;
  if (all_tail && (rc = fft_plan_tail_scratch(plan, int64_t(sizeof(double)) * n_k * n_frames, &epart_k))) return rc;
  // the cell gradient takes one store per k-point from the x stage: w = mu |rho^|^2 of batch entry c at wbuf + c * Mh, the head of
  // the batch's cell_work (frames_cell_layout)
  ConvCell cc{};
  cc.wbuf = cell_work;
  rc = convolve_xfused(plan, st, rho_all, G, hat_all, phi_all, dc_all, G_stride, nullptr, nullptr, nullptr, epart_k, nullptr, 0, nullptr, nullptr,
                       cell_work ? &cc : nullptr);
  if (rc) return rc;
  const FrameCellRec* recs = frames_cell_recs<T>(table, n_frames);
  if (cell_work) {
    // the riders of all frames in a launch of their own, grid (riders, frames): the batched inverse planes before them fill the
    // device already (profiles/frames_contract_times.txt)
    MIPME_REQUIRE(all_tail, "the cell gradient of a frame batch rides on the gather tail of every frame");
    const int n_riders = int(cell_work_layout(m, 1, nullptr).n_riders);
    if ((rc = frames_cell_riders<T>(st, recs, n_frames, n_riders, m->nx, m->ny, m->nz / 2 + 1, (const double*)epart_k, int(n_k)))) return rc;
  }
  if (slab) {  // the same two launches with the term
    MIPME_REQUIRE(all_tail, "the slab term of a frame batch rides on the gather tail of every frame");
    if ((rc = frames_slab_gather_tail<T>(st, m->scheme, m->order, dim3(unsigned(bg.nb), F), tb, (const double*)epart_k, int(n_k)))) return rc;
    return cell_work ? frames_slab_cell_finalize<T>(st, recs, n_frames) : MIPME_OK;
  }
  if (all_tail) {  // energy + forces of every frame in the gather launch
    MIPME_DISPATCH_STENCIL_B(m->scheme, m->order,
                             ((void)S, frames_gather_tail_kernel<N, T><<<dim3(unsigned(bg.nb), F), GATHER_THREADS, 0, st>>>(
                                 tb, (const double*)epart_k, int(n_k))));
    MIPME_LAUNCH_CHECK();
    if (cell_work) return frames_cell_finalize<T>(st, recs, n_frames);
    return MIPME_OK;
  }
  MIPME_DISPATCH_STENCIL_B(m->scheme, m->order,
                           ((void)S, frames_gather_kernel<N, T><<<dim3(unsigned(bg.nb), F), GATHER_THREADS, 0, st>>>(tb)));
  MIPME_LAUNCH_CHECK();
  frames_energy_kernel<T><<<F, 1024, 0, st>>>(tb);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // namespace mipme

using namespace mipme;

template <typename T>
static int frames_table_energy_log_t(int n_frames, void* host_table, void* log, void* cursors, int capacity) {
  FrameDev<T>* d = (FrameDev<T>*)host_table;
  for (int f = 0; f < n_frames; ++f) {
    MIPME_REQUIRE(!log || d[f].use_tail, "the energy log rides on the gather tail (mipme_frame_t.use_tail) of every frame");
    d[f].tail.elog = log ? (double*)log + f : nullptr;
    d[f].tail.elog_cursor = log ? (int*)cursors + f : nullptr;
    d[f].tail.elog_cap = capacity;
    d[f].tail.elog_stride = n_frames;
  }
  return MIPME_OK;
}

// What every entry point of the contract refuses, per frame, before anything is launched
static int frames_contract_check(int n_frames, const mipme_frame_t* fr, bool cell) {
  for (int k = 0; k < n_frames; ++k) {
    MIPME_REQUIRE(fr[k].use_tail, "frame %d: dE/dcharges and dE/dcell ride on the gather tail (mipme_frame_t.use_tail)", k);
    if (!cell) continue;
    MIPME_REQUIRE(fr[k].shift_format == kShiftTable32,
                  "frame %d: the cell gradient needs 4-byte entries (shift format 2), got format %d", k, fr[k].shift_format);
    MIPME_REQUIRE(!fr[k].dist_out, "frame %d: the cell gradient and the distance by-product (dist_out) exclude each other", k);
  }
  return MIPME_OK;
}

template <typename T>
static int frames_table_contract_t(int n_frames, const mipme_frame_t* fr, const mipme_potential_t* pot, void* host_table,
                                   void* const* grad_charges, void* const* grad_cell, const void* G_deriv, int64_t G_deriv_stride,
                                   void* cell_work, int64_t cell_work_stride, const void* aux_seed) {
  static_assert(kRowsPerSpreadBlock == 32 && SPREAD_THREADS / 64 == 8, "frames_cell_stride (host.h) sizes cwave by these");
  SRPot s;
  int rc = make_srpot(pot, s);
  if (rc) return rc;
  MIPME_REQUIRE(!grad_cell || rows_cell_supported<T>(fast_rs_exponent(s), fr[0].shift_format, nullptr),
                "the cell gradient of a frame batch covers 1/r and 1/r^6 with 4-byte entries");
  double self_c, bg_c;
  correction_terms(pot, self_c, bg_c);
  FrameDev<T>* d = (FrameDev<T>*)host_table;
  FrameCellRec* recs = frames_cell_recs<T>(host_table, n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const mipme_frame_t& f = fr[k];
    GatherTail<T>& tail = d[k].tail;
    tail.grad_q = grad_charges ? (T*)grad_charges[k] : nullptr;
    tail.aux_seed = (const T*)aux_seed;
    tail.rpart = nullptr;
    // (the slab term, attached before or after this call by mipme_frames_table_slab, keeps its own: the records for z, and
    // its fields of the cell record)
    tail.rec4 = tail.slab_mom ? (const AtomRecord<T>*)f.records : nullptr;
    d[k].rows.cpart = nullptr;
    const FrameCellRec before = recs[k];
    recs[k] = FrameCellRec{};
    recs[k].slab_mom = before.slab_mom;
    recs[k].slab_c0 = before.slab_c0;
    recs[k].slab_L = before.slab_L;
    recs[k].slab_axis = before.slab_axis;
    if (!grad_cell) continue;
    const CellWork cw = frames_cell_layout(&f.mesh, f.n_atoms, n_frames, k, cell_work, cell_work_stride, sizeof(T));
    tail.rpart = cw.rpart;
    tail.rec4 = (const AtomRecord<T>*)f.records;  // (x, y, z, q) of every atom, written by the binning pass of the step
    d[k].rows.cpart = cw.cwave;
    FrameCellRec& r = recs[k];
    r.mesh = f.mesh;
    r.bg = bg_c;
    r.pair_scale = f.full_list ? 0.25 : 0.5;  // 0.5 x the force scale
    r.wbuf = cw.wbuf;
    r.dG4 = (const T*)G_deriv + int64_t(k) * G_deriv_stride;
    r.cwave = cw.cwave;
    r.rows = cw.rows;
    r.rpart = cw.rpart;
    r.dc = f.dc;
    r.seed = aux_seed ? aux_seed : f.grad_seed;
    r.out = grad_cell[k];
    r.n_waves = int(cw.n_waves);
    r.n_riders = int(cw.n_riders);
    r.n_bricks = int(cw.n_bricks);
  }
  return MIPME_OK;
}

// ---- the 2-D periodic (slab) term of a frame batch ---------------------------------------------------------------------------
// What both entry points refuse, before anything is launched.  slab[k]: 0 = frame k is fully periodic, else its non-periodic
// axis + 1
static int frames_slab_check(int n_frames, const mipme_frame_t* fr, const mipme_potential_t* pot, const int32_t* slab,
                             const void* work, int64_t stride, const char* who) {
  MIPME_REQUIRE(slab && work, "%s: NULL slab array or slab_work", who);
  MIPME_REQUIRE(pot->kind == MIPME_COULOMB || pot->exponent == 1, "%s: the slab term exists for 1/r only", who);
  MIPME_REQUIRE(stride >= kSlabWork, "%s: slab_work_stride = %lld is below mipme_frames_slab_work() = %d", who, (long long)stride,
                kSlabWork);
  for (int k = 0; k < n_frames; ++k) {
    MIPME_REQUIRE(slab[k] >= 0 && slab[k] <= 3, "%s: frame %d: slab must be 0 (off) or the non-periodic axis + 1, got %d", who, k,
                  int(slab[k]));
    MIPME_REQUIRE(fr[k].use_tail, "%s: frame %d: the slab term rides on the gather tail (mipme_frame_t.use_tail)", who, k);
  }
  return MIPME_OK;
}

template <typename T>
static int frames_table_slab_t(int n_frames, const mipme_frame_t* fr, const mipme_potential_t* pot, void* host_table,
                               const int32_t* slab, void* work, int64_t stride) {
  FrameDev<T>* d = (FrameDev<T>*)host_table;
  FrameCellRec* recs = frames_cell_recs<T>(host_table, n_frames);
  for (int k = 0; k < n_frames; ++k) {
    GatherTail<T>& tail = d[k].tail;
    GatherTailHost th{};
    if (slab && slab[k]) tail_attach_slab(th, &fr[k].mesh, pot, slab[k]);
    // every frame of a slab batch has its work slice: a fully periodic one keeps the zeros there and c0 = L = 0, so that the
    // launches compiled with the term add exact zeros to it
    tail.slab_mom = slab ? (const double*)work + int64_t(k) * stride : nullptr;
    tail.slab_c0 = th.slab_c0;
    tail.slab_L = th.slab_L;
    tail.slab_axis = th.slab ? th.slab - 1 : 0;
    // z of an atom comes from its record (x, y, z, q), written by the binning pass of the step; the cell sums read it too
    tail.rec4 = (slab || tail.rpart) ? (const AtomRecord<T>*)fr[k].records : nullptr;
    recs[k].slab_mom = tail.slab_mom;
    recs[k].slab_c0 = tail.slab_c0;
    recs[k].slab_L = tail.slab_L;
    recs[k].slab_axis = tail.slab_axis;
  }
  return MIPME_OK;
}

// What mipme_frames_forward, mipme_frames_step and mipme_frames_slab_step share, in the order their refusals have always had: the
// frames and the required buffers, then the entry point's own checks (`own_checks`, a callable returning a status), the plan, the
// potential -- 1/r or 1/r^6, with the slab term 1/r alone -- and the launches.  cell_work: NULL without the cell gradient
template <typename OwnChecks>
static int frames_launch(const char* who, const mipme_frames_step_args_t& a, void* cell_work, bool slab, OwnChecks&& own_checks) {
  int rc = frames_check(a.dtype, a.n_frames, a.frames);
  if (rc) return rc;
  MIPME_REQUIRE(a.plan && a.pot && a.device_table && a.G && a.rho_mesh_all && a.hat_work_all && a.phi_mesh_all && a.dc_all &&
                    a.G_stride >= 0,
                "NULL buffer passed to %s", who);
  if ((rc = own_checks())) return rc;
  MIPME_REQUIRE(fft_plan_xfused(a.plan) && fft_plan_batch(a.plan) == a.n_frames,
                "%s needs a plan with batch = n_frames and a power-of-two nx", who);
  SRPot s;
  if ((rc = make_srpot(a.pot, s))) return rc;
  const int pfast = fast_rs_exponent(s);
  if (slab)
    MIPME_REQUIRE(pfast == 1, "%s: the slab term exists for 1/r with a smearing", who);
  else
    MIPME_REQUIRE(pfast == 1 || pfast == 6, "the frames path covers 1/r and 1/r^6 with a smearing");
  hipStream_t st = (hipStream_t)a.stream;
  DT_SWITCH(a.dtype,
            frames_forward_t<float>(a.plan, st, a.n_frames, a.frames, a.device_table, a.G, a.G_stride, a.rho_mesh_all, a.hat_work_all,
                                    a.phi_mesh_all, a.dc_all, pfast, cell_work, slab),
            frames_forward_t<double>(a.plan, st, a.n_frames, a.frames, a.device_table, a.G, a.G_stride, a.rho_mesh_all, a.hat_work_all,
                                     a.phi_mesh_all, a.dc_all, pfast, cell_work, slab));
}

extern "C" {

int64_t mipme_frames_slab_work(void) { return kSlabWork; }

int mipme_frames_table_slab(int dtype, int n_frames, const mipme_frame_t* frames, const mipme_potential_t* pot, void* host_table,
                            int64_t host_table_bytes, const int32_t* slab, void* slab_work, int64_t slab_work_stride) {
  int rc = frames_check(dtype, n_frames, frames);
  if (rc) return rc;
  MIPME_REQUIRE(pot && host_table && host_table_bytes >= mipme_frames_table_bytes(dtype, n_frames),
                "invalid arguments to mipme_frames_table_slab");
  if (slab && (rc = frames_slab_check(n_frames, frames, pot, slab, slab_work, slab_work_stride, "mipme_frames_table_slab"))) return rc;
  DT_SWITCH(dtype, frames_table_slab_t<float>(n_frames, frames, pot, host_table, slab, slab_work, slab_work_stride),
            frames_table_slab_t<double>(n_frames, frames, pot, host_table, slab, slab_work, slab_work_stride));
}

int mipme_frames_slab_step(const mipme_frames_slab_step_args_t* s) {
  MIPME_REQUIRE(s, "NULL argument struct passed to mipme_frames_slab_step");
  MIPME_REQUIRE(s->size == sizeof(mipme_frames_slab_step_args_t), "mipme_frames_slab_step_args_t: size %u, this library expects %zu",
                s->size, sizeof(mipme_frames_slab_step_args_t));
  MIPME_REQUIRE(s->version == MIPME_FRAMES_SLAB_STEP_VERSION, "mipme_frames_slab_step_args_t: version %u, this library expects %d",
                s->version, MIPME_FRAMES_SLAB_STEP_VERSION);
  const mipme_frames_step_args_t* a = &s->step;
  MIPME_REQUIRE(a->size == sizeof(mipme_frames_step_args_t) && a->version == MIPME_FRAMES_STEP_VERSION,
                "mipme_frames_slab_step_args_t.step: size %u / version %u, this library expects %zu / %d", a->size, a->version,
                sizeof(mipme_frames_step_args_t), MIPME_FRAMES_STEP_VERSION);
  const char* who = "mipme_frames_slab_step";
  return frames_launch(who, *a, a->cell_gradient ? a->cell_work : nullptr, true, [&]() -> int {
    MIPME_REQUIRE(!a->cell_gradient || a->cell_work, "%s: the cell gradient needs cell_work", who);
    const int rc = frames_slab_check(a->n_frames, a->frames, a->pot, s->slab, s->slab_work, s->slab_work_stride, who);
    return rc ? rc : frames_contract_check(a->n_frames, a->frames, a->cell_gradient != 0);
  });
}

int64_t mipme_frames_table_bytes(int dtype, int n_frames) {
  if (n_frames <= 0) return 0;
  return int64_t(n_frames) * int64_t((dtype == MIPME_F32 ? sizeof(FrameDev<float>) : sizeof(FrameDev<double>)) + sizeof(FrameCellRec));
}

int64_t mipme_frames_cell_work(const mipme_mesh_t* mesh, int64_t n_atoms) {
  if (!mesh || validate_mesh(mesh) || n_atoms <= 0) return 0;
  return frames_cell_stride(mesh, n_atoms);
}

int mipme_frames_table_contract(int dtype, int n_frames, const mipme_frame_t* frames, const mipme_potential_t* pot, void* host_table,
                                int64_t host_table_bytes, void* const* grad_charges, void* const* grad_cell, const void* G_deriv,
                                int64_t G_deriv_stride, void* cell_work, int64_t cell_work_stride, const void* aux_seed) {
  int rc = frames_check(dtype, n_frames, frames);
  if (rc) return rc;
  MIPME_REQUIRE(pot && host_table && host_table_bytes >= mipme_frames_table_bytes(dtype, n_frames),
                "invalid arguments to mipme_frames_table_contract");
  if ((rc = frames_contract_check(n_frames, frames, grad_cell != nullptr))) return rc;
  for (int k = 0; k < n_frames; ++k) {
    MIPME_REQUIRE(!grad_charges || grad_charges[k], "frame %d: NULL grad_charges", k);
    MIPME_REQUIRE(!grad_cell || grad_cell[k], "frame %d: NULL grad_cell", k);
  }
  if (grad_cell) {
    MIPME_REQUIRE(G_deriv && cell_work && G_deriv_stride >= 0, "the cell gradient needs the frames' derivative tables (G_deriv) and cell_work");
    for (int k = 0; k < n_frames; ++k)
      MIPME_REQUIRE(cell_work_stride >= frames_cell_stride(&frames[k].mesh, frames[k].n_atoms),
                    "frame %d: cell_work_stride = %lld is below mipme_frames_cell_work() = %lld", k, (long long)cell_work_stride,
                    (long long)frames_cell_stride(&frames[k].mesh, frames[k].n_atoms));
  }
  DT_SWITCH(dtype,
            frames_table_contract_t<float>(n_frames, frames, pot, host_table, grad_charges, grad_cell, G_deriv, G_deriv_stride,
                                           cell_work, cell_work_stride, aux_seed),
            frames_table_contract_t<double>(n_frames, frames, pot, host_table, grad_charges, grad_cell, G_deriv, G_deriv_stride,
                                            cell_work, cell_work_stride, aux_seed));
}

int mipme_frames_step(const mipme_frames_step_args_t* a) {
  MIPME_REQUIRE(a, "NULL argument struct passed to mipme_frames_step");
  MIPME_REQUIRE(a->size == sizeof(mipme_frames_step_args_t), "mipme_frames_step_args_t: size %u, this library expects %zu", a->size,
                sizeof(mipme_frames_step_args_t));
  MIPME_REQUIRE(a->version == MIPME_FRAMES_STEP_VERSION, "mipme_frames_step_args_t: version %u, this library expects %d", a->version,
                MIPME_FRAMES_STEP_VERSION);
  return frames_launch("mipme_frames_step", *a, a->cell_gradient ? a->cell_work : nullptr, false, [&]() -> int {
    MIPME_REQUIRE(!a->cell_gradient || a->cell_work, "mipme_frames_step: the cell gradient needs cell_work");
    return frames_contract_check(a->n_frames, a->frames, a->cell_gradient != 0);
  });
}

int mipme_frames_table_build(int dtype, int n_frames, const mipme_frame_t* frames, const mipme_potential_t* pot,
                             void* host_table, int64_t host_table_bytes) {
  int rc = frames_check(dtype, n_frames, frames);
  if (rc) return rc;
  MIPME_REQUIRE(pot && host_table && host_table_bytes >= mipme_frames_table_bytes(dtype, n_frames),
                "invalid arguments to mipme_frames_table_build");
  DT_SWITCH(dtype, frames_table_build_t<float>(n_frames, frames, pot, host_table),
            frames_table_build_t<double>(n_frames, frames, pot, host_table));
}

int mipme_frames_table_energy_log(int dtype, int n_frames, void* host_table, int64_t host_table_bytes, void* log, void* cursors,
                                  int capacity) {
  MIPME_REQUIRE((dtype == MIPME_F32 || dtype == MIPME_F64) && n_frames > 0 && host_table &&
                    host_table_bytes >= mipme_frames_table_bytes(dtype, n_frames) && (!log || (cursors && capacity > 0)),
                "invalid arguments to mipme_frames_table_energy_log");
  DT_SWITCH(dtype, frames_table_energy_log_t<float>(n_frames, host_table, log, cursors, capacity),
            frames_table_energy_log_t<double>(n_frames, host_table, log, cursors, capacity));
}

int mipme_frames_forward(mipme_fft_plan* plan, void* stream, int dtype, int n_frames, const mipme_frame_t* frames,
                         const mipme_potential_t* pot, const void* device_table, const void* G, int64_t G_stride,
                         void* rho_mesh_all, void* hat_work_all, void* phi_mesh_all, void* dc_all) {
  mipme_frames_step_args_t a{};  // (the step's arguments without its flags; neither size nor version is looked at)
  a.plan = plan, a.stream = stream, a.dtype = dtype, a.n_frames = n_frames, a.frames = frames, a.pot = pot;
  a.device_table = device_table, a.G = G, a.G_stride = G_stride;
  a.rho_mesh_all = rho_mesh_all, a.hat_work_all = hat_work_all, a.phi_mesh_all = phi_mesh_all, a.dc_all = dc_all;
  return frames_launch("mipme_frames_forward", a, nullptr, false, [] { return int(MIPME_OK); });
}

int mipme_frames_table_cells(int dtype, int n_frames, const mipme_frame_t* frames, void* host_table, int64_t host_table_bytes,
                             void* status) {
  int rc = frames_check(dtype, n_frames, frames);
  if (rc) return rc;
  MIPME_REQUIRE(host_table && host_table_bytes >= mipme_frames_table_bytes(dtype, n_frames),
                "invalid arguments to mipme_frames_table_cells");
  for (int k = 0; k < n_frames && status; ++k)
    MIPME_REQUIRE(frames[k].use_tail, "frame %d: the status of a cell rides on the gather tail (mipme_frame_t.use_tail)", k);
  DT_SWITCH(dtype, frames_table_cells_t<float>(n_frames, host_table, status), frames_table_cells_t<double>(n_frames, host_table, status));
}

int mipme_frames_cells(const mipme_frames_cells_args_t* a) {
  MIPME_REQUIRE(a, "NULL argument struct passed to mipme_frames_cells");
  MIPME_REQUIRE(a->size == sizeof(mipme_frames_cells_args_t), "mipme_frames_cells_args_t: size %u, this library expects %zu", a->size,
                sizeof(mipme_frames_cells_args_t));
  MIPME_REQUIRE(a->version == MIPME_FRAMES_CELLS_VERSION, "mipme_frames_cells_args_t: version %u, this library expects %d", a->version,
                MIPME_FRAMES_CELLS_VERSION);
  int rc = frames_check(a->dtype, a->n_frames, a->frames);
  if (rc) return rc;
  MIPME_REQUIRE(a->pot && a->device_table && a->cells && a->cells_valid && a->G && a->status, "NULL buffer passed to mipme_frames_cells");
  MIPME_REQUIRE(a->mesh_spacing > 0 && std::isfinite(a->mesh_spacing), "mipme_frames_cells: mesh_spacing must be positive, got %g",
                a->mesh_spacing);
  const mipme_mesh_t* m = &a->frames[0].mesh;
  const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
  // every frame writes its own slice of the tables: a shared table (stride 0) cannot follow several cells
  MIPME_REQUIRE(a->G_stride >= Mh, "mipme_frames_cells: G_stride = %lld is below the half grid's %lld points", (long long)a->G_stride,
                (long long)Mh);
  MIPME_REQUIRE(!a->G_deriv || a->G_deriv_stride >= 4 * Mh, "mipme_frames_cells: G_deriv_stride = %lld is below 4 x %lld",
                (long long)a->G_deriv_stride, (long long)Mh);
  const size_t real = a->dtype == MIPME_F32 ? 4 : 8;
  for (int k = 0; k < a->n_frames; ++k) {
    MIPME_REQUIRE(a->frames[k].use_tail, "frame %d: the status of a cell rides on the gather tail (mipme_frame_t.use_tail)", k);
    // the pair rows read the validated copy, never the input buffer
    MIPME_REQUIRE(a->frames[k].cell == (const char*)a->cells_valid + size_t(k) * 9 * real,
                  "frame %d: mipme_frame_t.cell must point at the frame's slice of cells_valid", k);
  }
  hipStream_t st = (hipStream_t)a->stream;
  DT_SWITCH(a->dtype,
            frames_cells_launch<float>(st, a->n_frames, m, a->pot, a->device_table, a->cells, a->cells_valid, a->G, a->G_stride, a->G_deriv,
                                       a->G_deriv_stride, a->mesh_spacing, a->status),
            frames_cells_launch<double>(st, a->n_frames, m, a->pot, a->device_table, a->cells, a->cells_valid, a->G, a->G_stride, a->G_deriv,
                                        a->G_deriv_stride, a->mesh_spacing, a->status));
}

int64_t mipme_frames_counter_ints(const mipme_mesh_t* mesh, int64_t n_atoms, int dtype) {
  if (!mesh || validate_mesh(mesh) || !bricks_supported(mesh, dtype)) return 0;
  return frames_counter_ints(mesh, n_atoms, dtype);
}

int mipme_frames_backward(void* stream, int dtype, int n_frames, const mipme_frame_t* frames, const void* device_table,
                          const void* grad_scale) {
  int rc = frames_check(dtype, n_frames, frames);
  if (rc) return rc;
  MIPME_REQUIRE(device_table && grad_scale, "NULL buffer passed to mipme_frames_backward");
  int64_t max_atoms = 0;
  for (int k = 0; k < n_frames; ++k) max_atoms = std::max<int64_t>(max_atoms, frames[k].n_atoms);
  const dim3 grid(unsigned((3 * max_atoms + 255) / 256), unsigned(n_frames));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIPME_F32)
    frames_finalize_kernel<float><<<grid, 256, 0, st>>>((const FrameDev<float>*)device_table, (const float*)grad_scale);
  else
    frames_finalize_kernel<double><<<grid, 256, 0, st>>>((const FrameDev<double>*)device_table, (const double*)grad_scale);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

}  // extern "C"
