// The cells of a frame batch as a replay input (include/mipme.h: mipme_frames_table_cells / mipme_frames_cells /
// mipme_frames_cell_geometry; GraphedFrameBatch(follow_cells=True)).  ONE launch ahead of the step turns the (F, 3, 3) cells the
// caller wrote on the device into everything the step's kernels read of a cell: the geometry fields of the frame's records in the
// device-resident table, the frame's G(k) and derivative tables, and a validated copy of the cell for the pair rows.  No kernel of
// the step changes: they read the table as before (frames.hip, frames_cell.hip, frames_slab.hip).
//
// The safety property: a cell that is singular or not finite changes NOTHING but the frame's status word.  Table, validated copy
// and filter tables keep the values of the last valid cell, so no kernel of the step ever sees geometry that is not finite (a NaN
// never becomes a mesh index); the gather tail turns the frame's energy into NaN through GatherTail::live_flags (bit 1).
#include "cell_invert.h"
#include "frames_device.h"
#include "kgrid.h"

namespace mipme {

template <typename T>
struct FramesCellsArgs {
  FrameDev<T>* table;     // the uploaded table: n_frames FrameDev<T>, then n_frames FrameCellRec
  FrameCellRec* recs;
  const T* cells_in;      // (F, 3, 3): read by this launch alone
  T* cells_valid;         // (F, 3, 3): mipme_frame_t.cell of frame f points at slice f
  T* G;                   // frame f's table at G + f * G_stride
  T* D;                   // nullable: frame f's derivative table at D + f * D_stride (4 reals per point)
  int64_t G_stride, D_stride;
  int* status;            // (F)
  KPot kp;
  double mesh_spacing;
  double slab_pref;       // 4 pi prefactor: slab_c0 = slab_pref / V (tail_attach_slab of host.h)
  int nx, ny, nz, scheme, order;
};

// grid (ceil(Mh / 256), F) x 256 threads.  Every thread inverts its frame's cell itself (a few dozen float64 operations from nine
// wave-uniform loads, beside ~1000 for its k-point): the verdict is uniform per block without a word exchanged between blocks.
// Block x == 0 of a frame (its thread 0) is the only one that reads or writes the table, the validated copy and the status word;
// the others take everything from the kernel arguments.  All stores are plain global stores; the stream orders the launch against the step.
template <typename T, bool DERIV>
__global__ __launch_bounds__(256) void frames_cells_kernel(FramesCellsArgs<T> a) {
  const int f = blockIdx.y;
  const T* __restrict__ cell = a.cells_in + 9 * int64_t(f);
  const FrameCellGeom geo = frame_cell_geometry<T>(cell, a.nx, a.ny, a.nz, a.mesh_spacing);
  const bool bad = (geo.status & kCellBad) != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.status[f] = geo.status;
  if (bad) return;  // (uniform per block: every thread has formed the same verdict from the same nine values)
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (one thread, constant indices: a lane-indexed copy would send `geo` to scratch)
    FrameDev<T>& d = a.table[f];
    FrameCellRec& r = a.recs[f];
    const bool cell_rec = r.n_riders != 0;  // the record of the cell gradient (zero without it)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      d.g.inv[k] = geo.inv[k];
      d.spread.g.inv[k] = geo.inv[k];
      a.cells_valid[9 * int64_t(f) + k] = cell[k];
      if (cell_rec) {
        r.mesh.cell[k] = geo.A[k];
        r.mesh.inv_cell[k] = geo.inv[k];
      }
    }
    d.inv_vol = T(geo.inv_vol);
    if (cell_rec) r.mesh.volume = geo.vol;
    // the slab term of the frame: c0 != 0 marks a slab frame (a fully periodic frame of a slab batch keeps c0 = L = 0)
    if (d.tail.slab_c0 != 0.0) {
      const int axis = d.tail.slab_axis;
      const double c0 = a.slab_pref / geo.vol, L = axis == 0 ? geo.norm[0] : (axis == 1 ? geo.norm[1] : geo.norm[2]);
      d.tail.slab_c0 = c0;
      d.tail.slab_L = L;
      r.slab_c0 = c0;
      r.slab_L = L;
    }
  }
  const int nzh = a.nz / 2 + 1;
  const int64_t Mh = int64_t(a.nx) * a.ny * nzh;
  const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (p >= Mh) return;
  KGeom g;  // make_kgeom of kgrid.h for this cell
#pragma unroll
  for (int k = 0; k < 9; ++k) g.inv[k] = geo.inv[k];
  g.h[0] = geo.norm[0] / double(a.nx);
  g.h[1] = geo.norm[1] / double(a.ny);
  g.h[2] = geo.norm[2] / double(a.nz);
  g.nx = a.nx, g.ny = a.ny, g.nz = a.nz, g.nzh = nzh;
  g.scheme = a.scheme, g.order = a.order;
  {  // kfilter_kernel
    double inv, v, dv;
    bool dead;
    const double k2 = kgrid_point(g, p, inv, dead);
    lr_kernel_dev(a.kp, k2, v, dv);
    a.G[int64_t(f) * a.G_stride + p] = T(dead ? 0.0 : v * inv);
  }
  if constexpr (DERIV) {  // kfilter_deriv_kernel
    int ix, iy, iz;
    half_grid_index(g, p, ix, iy, iz);
    KPoint o;
    eval_point(g, a.kp, ix, iy, iz, o);
    T* __restrict__ D = a.D + int64_t(f) * a.D_stride + 4 * p;
    D[0] = T(o.alpha);
    D[1] = T(o.beta[0]);
    D[2] = T(o.beta[1]);
    D[3] = T(o.beta[2]);
  }
}

template <typename T>
int frames_cells_launch(hipStream_t st, int n_frames, const mipme_mesh_t* m, const mipme_potential_t* pot, void* device_table,
                        const void* cells_in, void* cells_valid, void* G, int64_t G_stride, void* G_deriv, int64_t G_deriv_stride,
                        double mesh_spacing, void* status) {
  FramesCellsArgs<T> a;
  int rc = make_kpot(pot, a.kp);
  if (rc) return rc;
  a.table = (FrameDev<T>*)device_table;
  a.recs = frames_cell_recs<T>(device_table, n_frames);
  a.cells_in = (const T*)cells_in;
  a.cells_valid = (T*)cells_valid;
  a.G = (T*)G;
  a.D = (T*)G_deriv;
  a.G_stride = G_stride;
  a.D_stride = G_deriv_stride;
  a.status = (int*)status;
  a.mesh_spacing = mesh_spacing;
  a.slab_pref = pot->prefactor * 4.0 * 3.14159265358979323846;
  a.nx = m->nx, a.ny = m->ny, a.nz = m->nz, a.scheme = m->scheme, a.order = m->order;
  const int64_t Mh = int64_t(m->nx) * m->ny * (m->nz / 2 + 1);
  const dim3 grid(unsigned((Mh + 255) / 256), unsigned(n_frames));
  if (G_deriv)
    frames_cells_kernel<T, true><<<grid, 256, 0, st>>>(a);
  else
    frames_cells_kernel<T, false><<<grid, 256, 0, st>>>(a);
  MIPME_LAUNCH_CHECK();
  return MIPME_OK;
}

template <typename T>
int frames_table_cells_t(int n_frames, void* host_table, void* status) {
  FrameDev<T>* d = (FrameDev<T>*)host_table;
  for (int f = 0; f < n_frames; ++f) {
    MIPME_REQUIRE(!status || d[f].use_tail, "frame %d: the status of a cell rides on the gather tail (mipme_frame_t.use_tail)", f);
    d[f].tail.live_flags = status ? (const int*)status + f : nullptr;
  }
  return MIPME_OK;
}

template int frames_cells_launch<float>(hipStream_t, int, const mipme_mesh_t*, const mipme_potential_t*, void*, const void*, void*, void*,
                                        int64_t, void*, int64_t, double, void*);
template int frames_cells_launch<double>(hipStream_t, int, const mipme_mesh_t*, const mipme_potential_t*, void*, const void*, void*, void*,
                                         int64_t, void*, int64_t, double, void*);
template int frames_table_cells_t<float>(int, void*, void*);
template int frames_table_cells_t<double>(int, void*, void*);

}  // namespace mipme

using namespace mipme;

extern "C" int mipme_frames_cell_geometry(const double cell[9], int dtype, const int32_t ns[3], double mesh_spacing, double inv_out[9],
                                          double* inv_vol_out, int32_t* status_out) {
  MIPME_REQUIRE(cell && ns && status_out, "NULL argument passed to mipme_frames_cell_geometry");
  MIPME_REQUIRE(dtype == MIPME_F32 || dtype == MIPME_F64, "invalid dtype %d", dtype);
  FrameCellGeom g;
  if (dtype == MIPME_F32) {
    float c32[9];  // the values the batch's buffer would hold
    for (int k = 0; k < 9; ++k) c32[k] = float(cell[k]);
    g = frame_cell_geometry<float>(c32, ns[0], ns[1], ns[2], mesh_spacing);
  } else {
    g = frame_cell_geometry<double>(cell, ns[0], ns[1], ns[2], mesh_spacing);
  }
  if (inv_out)
    for (int k = 0; k < 9; ++k) inv_out[k] = g.inv[k];
  if (inv_vol_out) *inv_vol_out = g.inv_vol;
  *status_out = g.status;
  return MIPME_OK;
}
