// The computations of the dipole step (dipole_step.hip), each ONCE, as a body that sees ONE system: its sizes, ITS slices of the
// buffers and the index of the block inside that system's launch -- the form of ewald_step_bodies.h.  The kernels of
// dipole_step.hip call them with their arguments and blockIdx (mipme_dipole_step and mipme_dipole_cell_step), the kernels of
// dipole_batch.hip with the sizes, the slices and the local block index of the frame table; the bodies see nothing of the table.
// What is computed is described at the head of dipole_step.hip.  The final launch of the step with a fixed cell and of the step that
// follows its cell differ in where 1/V and A^-1 come from and in nothing else: ds_final_core takes them as pointers,
// ds_final_body reads them from the geometry record.  Three kernels do NOT call a body and keep their own text
// (docs/HISTORY.md, "one body for each dipole step kernel"): dipole_step_finish_kernel and dipole_cell_step_finish_kernel of
// dipole_step.hip -- called through a body, the fp32 instances contract other products of dE/dmu into fused multiply-adds and give
// other bits -- so ds_finish_body serves the batch alone; and dipole_structure_kernel of dipole.hip, whose G is nullable.  The
// LDS arrays are declared in the bodies: every body is inlined into the one kernel that calls it.
#pragma once

#include <cmath>

#include "dipole_device.h"
#include "ewald_step_device.h"  // kEsGeom, es_invert_cell, lr_kernel_dev
#include "kpot.h"
#include "rows_body.h"
#include "step_device.h"

namespace mipme {

// ---- 0. records (dipole_step_records_kernel, and the atom blocks of prep): (x, y, z, -) / (mu_x, mu_y, mu_z, -) of every atom and
// the float64 block partials of sum_j mu_j
template <typename T>
__device__ __forceinline__ void ds_records_body(int64_t N, int64_t blk, const T* __restrict__ pos, const T* __restrict__ mu,
                                                AtomRecord<T>* __restrict__ recp, AtomRecord<T>* __restrict__ recm,
                                                double* __restrict__ mu_part) {
  __shared__ double red[kStepWaves];
  const int64_t a = blk * kStepBlock + threadIdx.x;
  double m[3] = {0.0, 0.0, 0.0};
  if (a < N) {
    const T mx = mu[3 * a], my = mu[3 * a + 1], mz = mu[3 * a + 2];
    recp[a] = AtomRecord<T>{pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], T(0)};
    recm[a] = AtomRecord<T>{mx, my, mz, T(0)};
    m[0] = double(mx), m[1] = double(my), m[2] = double(mz);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = block_sum<kStepWaves>(m[c], red);
    if (threadIdx.x == 0) mu_part[3 * blk + c] = s;
  }
}

// ---- 1. prep (dipole_cell_step_prep_kernel): k table and geometry (blocks blk < n_table_blocks), the two records of every atom
// and the dipole partials (the blocks behind them).  status: the ONE word of this system.  lr_wavelength <= 0 (a potential
// without smearing): bit 0 is never set
template <typename T>
__device__ __forceinline__ void ds_prep_body(const KPot& kp, int64_t N, int64_t K, int n_table_blocks, int blk,
                                             const T* __restrict__ cell, const int* __restrict__ freq, const int* __restrict__ mult,
                                             int ns0, int ns1, int ns2, double lr_wavelength, const T* __restrict__ pos,
                                             const T* __restrict__ mu, T* __restrict__ kvec, T* __restrict__ G, T* __restrict__ dG,
                                             AtomRecord<T>* __restrict__ recp, AtomRecord<T>* __restrict__ recm,
                                             double* __restrict__ mu_part, double* __restrict__ geom, int* __restrict__ status) {
  if (blk >= n_table_blocks) {  // (uniform per block)
    ds_records_body<T>(N, int64_t(blk - n_table_blocks), pos, mu, recp, recm, mu_part);
    return;
  }
  double A[9];
  const EsCell g = es_invert_cell(cell, A);
  if (blk == 0 && threadIdx.x == 0) {
    // A^-1 = (A^-T)^T, row-major
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) geom[3 * r + c] = g.recip[3 * c + r];
    geom[9] = g.inv_vol;
    geom[10] = g.bad ? 1.0 : 0.0;
    // bit 0: the eager call would choose another k grid for this cell, ns_d = ceil(|a_d| / lr_wavelength)
    const int ns[3] = {ns0, ns1, ns2};
    int st = g.bad ? 2 : 0;
    if (lr_wavelength > 0.0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double norm = sqrt(A[3 * d] * A[3 * d] + A[3 * d + 1] * A[3 * d + 1] + A[3 * d + 2] * A[3 * d + 2]);
        if (!(ceil(norm / lr_wavelength) == double(ns[d]))) st |= 1;
      }
    }
    status[0] = st;
  }
  const int64_t k = int64_t(blk) * kStepBlock + threadIdx.x;
  if (k >= K) return;
  double kv[3] = {0.0, 0.0, 0.0}, v = 0.0, dv = 0.0;
  if (!g.bad) {  // (a singular cell: a table of zeros, and the final launch writes NaN as the energy)
    const double f0 = double(freq[3 * k]), f1 = double(freq[3 * k + 1]), f2 = double(freq[3 * k + 2]);
#pragma unroll
    for (int n = 0; n < 3; ++n) kv[n] = (2.0 * kPi) * (f0 * g.recip[n] + f1 * g.recip[3 + n] + f2 * g.recip[6 + n]);
    lr_kernel_dev(kp, kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2], v, dv);
    const double m = double(mult[k]);
    v *= m;
    dv *= m;
  }
  kvec[3 * k] = T(kv[0]), kvec[3 * k + 1] = T(kv[1]), kvec[3 * k + 2] = T(kv[2]);
  G[k] = T(v);
  if (dG) dG[k] = T(dv);
}

// ---- 2. structure factors (dipole_structure_kernel of dipole.hip): S_c(k) = sum_j (mu_j . k) cos(k r_j), S_s likewise; 32 lanes
// per k-vector, positions and dipoles streamed through LDS; a block whose eight k-vectors all have G = dG = 0 is pruned whole
template <typename T>
__device__ __forceinline__ void ds_structure_body(int64_t N, int64_t K, int64_t blk, const T* __restrict__ pos,
                                                  const T* __restrict__ mu, const T* __restrict__ kvec, const T* __restrict__ G,
                                                  const T* __restrict__ dG, T* __restrict__ Sc, T* __restrict__ Ss) {
  __shared__ T sp[kStepTile * 3];
  __shared__ T sw[kStepTile * 3];
  const int al = threadIdx.x % kStepKLanes;
  const int64_t k = blk * kStepKPerBlock + threadIdx.x / kStepKLanes;
  const bool live = k < K && (G[k] != T(0) || (dG != nullptr && dG[k] != T(0)));
  if (!__syncthreads_or(live)) {  // the whole block is pruned (uniform branch)
    if (k < K && al == 0) Sc[k] = Ss[k] = T(0);
    return;
  }
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  T ac = T(0), as = T(0);
  for (int64_t base = 0; base < N; base += kStepTile) {
    const int n = int(min<int64_t>(kStepTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * n; t += kStepBlock) {
      sp[t] = pos[3 * base + t];
      sw[t] = mu[3 * base + t];
    }
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kStepKLanes) {
        T s, c;
        dipole_phase3(kx, ky, kz, sp[3 * i], sp[3 * i + 1], sp[3 * i + 2], s, c);
        const T q = kx * sw[3 * i] + ky * sw[3 * i + 1] + kz * sw[3 * i + 2];
        ac += q * c;
        as += q * s;
      }
  }
#pragma unroll
  for (int off = kStepKLanes / 2; off > 0; off >>= 1) ac += __shfl_xor(ac, off, kStepKLanes);
#pragma unroll
  for (int off = kStepKLanes / 2; off > 0; off >>= 1) as += __shfl_xor(as, off, kStepKLanes);
  if (k < K && al == 0) {
    Sc[k] = live ? ac : T(0);
    Ss[k] = live ? as : T(0);
  }
}

// ---- 3. fused atom body (dipole_step_atom_kernel): atom i of N against the k-vectors [slice * chunk, (slice + 1) * chunk) -------
// part[(slice N + i) 6 + c]: c < 3 the field sum_k G k (c S_c + s S_s), c >= 3 the bracket sum_k G (mu_i.k)(c S_s - s S_c) k
template <typename T>
__device__ __forceinline__ void ds_atom_body(int64_t i, int64_t slice, int64_t N, int64_t K, int64_t chunk,
                                             const AtomRecord<T>* __restrict__ recp, const AtomRecord<T>* __restrict__ recm,
                                             const T* __restrict__ kvec, const T* __restrict__ G, const T* __restrict__ Sc,
                                             const T* __restrict__ Ss, T* __restrict__ part) {
  __shared__ T red[kStepWaves][6];
  const int64_t k0 = slice * chunk, k1 = min<int64_t>(K, k0 + chunk);
  const AtomRecord<T> p = recp[i], m = recm[i];
  T fx = T(0), fy = T(0), fz = T(0), bx = T(0), by = T(0), bz = T(0);
  for (int64_t k = k0 + threadIdx.x; k < k1; k += kStepBlock) {
    const T gk = G[k];
    if (gk == T(0)) continue;  // exact: the term is G(k) times a finite sum
    const T kx = kvec[3 * k], ky = kvec[3 * k + 1], kz = kvec[3 * k + 2];
    const T sc = Sc[k], ss = Ss[k];
    T s, c;
    dipole_phase3(kx, ky, kz, p.x, p.y, p.z, s, c);
    const T f = gk * (c * sc + s * ss);
    const T b = gk * (m.x * kx + m.y * ky + m.z * kz) * (c * ss - s * sc);
    fx += f * kx;
    fy += f * ky;
    fz += f * kz;
    bx += b * kx;
    by += b * ky;
    bz += b * kz;
  }
  fx = wave_sum(fx), fy = wave_sum(fy), fz = wave_sum(fz);
  bx = wave_sum(bx), by = wave_sum(by), bz = wave_sum(bz);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = fx, red[wave][1] = fy, red[wave][2] = fz;
    red[wave][3] = bx, red[wave][4] = by, red[wave][5] = bz;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    T s = T(0);
#pragma unroll
    for (int w = 0; w < kStepWaves; ++w) s += red[w][threadIdx.x];
    part[(slice * N + i) * 6 + threadIdx.x] = s;
  }
}

// ---- 4. dipole pair rows (dipole_step_rows_kernel): 16 lanes per atom row, the 7^3 table of Cartesian shift vectors of the
// system's cell in LDS; per entry one word (other | code << 22) and two record gathers (position, dipole of the partner)
//   row_out[6 a + c]     = scale sum_e (T(vec_e) mu_o)_c                      c < 3
//   row_out[6 a + 3 + c] = scale sum_e (grad_vec (mu_a.T(vec_e).mu_o))_c
//   cell_part[9 blk + 3 m + n] = scale sum over the role-i entries of the rows of block blk of S_m (grad_vec ...)_n   (CELL, float64)
template <typename T, bool EXCL, bool CELL>
__device__ __forceinline__ void ds_rows_body(const DipPot<T>& P, int64_t N, int64_t blk, const int* __restrict__ row_ptr,
                                             const int* __restrict__ ent32, const AtomRecord<T>* __restrict__ recp,
                                             const AtomRecord<T>* __restrict__ recm, const T* __restrict__ cell, T scale,
                                             T* __restrict__ row_out, double* __restrict__ cell_part) {
  __shared__ AtomRecord<T> shift_tab[kShiftTableSize];
  __shared__ double red[kStepWaves][9];
  step_fill_shift_table(shift_tab, cell);
  __syncthreads();
  const StepRow row = step_row(N, blk, row_ptr);
  const AtomRecord<T> pa = recp[row.a], ma = recm[row.a];
  T fx = T(0), fy = T(0), fz = T(0), gx = T(0), gy = T(0), gz = T(0);
  T w00 = T(0), w01 = T(0), w02 = T(0), w10 = T(0), w11 = T(0), w12 = T(0), w20 = T(0), w21 = T(0), w22 = T(0);
  for (int base = row.beg; base < row.end; base += 16) {
    const int e = base + row.sub;
    const StepEntry en = step_entry(ent32, e, row);
    const AtomRecord<T> po = recp[en.o], mo = recm[en.o];
    const AtomRecord<T> sh = shift_tab[en.code];
    const T vx = (po.x - pa.x) + sh.x, vy = (po.y - pa.y) + sh.y, vz = (po.z - pa.z) + sh.z;
    const T r2 = vx * vx + vy * vy + vz * vz;
    const T ri = T(1) / fsqrt(r2);
    T B, C, dB, dC;
    dipole_bc<T, true, EXCL>(P, r2, ri, B, C, dB, dC);
    const T cr = C * (mo.x * vx + mo.y * vy + mo.z * vz);
    T ex = T(0), ey = T(0), ez = T(0);
    dipole_pair_grad<T>(vx, vy, vz, C, dB, dC, ma.x, ma.y, ma.z, mo.x, mo.y, mo.z, ex, ey, ez);
    if (en.ok) {
      fx += B * mo.x - cr * vx;
      fy += B * mo.y - cr * vy;
      fz += B * mo.z - cr * vz;
      gx += ex;
      gy += ey;
      gz += ez;
      if (CELL && e < row.mid) {  // role i: the listed pair, its own shift
        T sx, sy, sz;
        step_shift_of_code(en.code, sx, sy, sz);
        w00 += sx * ex, w01 += sx * ey, w02 += sx * ez;
        w10 += sy * ex, w11 += sy * ey, w12 += sy * ez;
        w20 += sz * ex, w21 += sz * ey, w22 += sz * ez;
      }
    }
  }
  fx = row_sum(fx), fy = row_sum(fy), fz = row_sum(fz);
  gx = row_sum(gx), gy = row_sum(gy), gz = row_sum(gz);
  if (row.sub == 0 && row.valid) {
    T* o = row_out + 6 * row.a;
    o[0] = scale * fx, o[1] = scale * fy, o[2] = scale * fz;
    o[3] = scale * gx, o[4] = scale * gy, o[5] = scale * gz;
  }
  if (CELL) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double s0 = wave_sum(double(w00)), s1 = wave_sum(double(w01)), s2 = wave_sum(double(w02));
    const double s3 = wave_sum(double(w10)), s4 = wave_sum(double(w11)), s5 = wave_sum(double(w12));
    const double s6 = wave_sum(double(w20)), s7 = wave_sum(double(w21)), s8 = wave_sum(double(w22));
    if (lane == 0) {
      red[wave][0] = s0, red[wave][1] = s1, red[wave][2] = s2;
      red[wave][3] = s3, red[wave][4] = s4, red[wave][5] = s5;
      red[wave][6] = s6, red[wave][7] = s7, red[wave][8] = s8;
    }
    __syncthreads();
    if (tid < 9) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < kStepWaves; ++w) s += red[w][tid];
      cell_part[9 * blk + tid] = double(scale) * s;
    }
  }
}

// ---- 5. per-k cell gradient (dipole_step_cellk_kernel): 32 lanes per k-vector, positions and dipoles streamed through LDS -------
//   k_part[10 blk + 3 a + n] = sum over the k-vectors of block blk of gk_a k_n;   k_part[10 blk + 9] = sum 1/2 G |S|^2     (float64)
template <typename T>
__device__ __forceinline__ void ds_cellk_body(int64_t N, int64_t K, int64_t blk, const T* __restrict__ pos, const T* __restrict__ mu,
                                              const T* __restrict__ kvec, const T* __restrict__ G, const T* __restrict__ dG,
                                              const T* __restrict__ Sc, const T* __restrict__ Ss, double* __restrict__ k_part) {
  __shared__ T sp[kStepTile * 3];
  __shared__ T sm[kStepTile * 3];
  __shared__ double red[kStepKPerBlock][kStepCellK];
  const int al = threadIdx.x % kStepKLanes, kl = threadIdx.x / kStepKLanes;
  const int64_t k = blk * kStepKPerBlock + kl;
  const bool live = k < K && (G[k] != T(0) || dG[k] != T(0));
  const int64_t kc = k < K ? k : 0;
  const T kx = kvec[3 * kc], ky = kvec[3 * kc + 1], kz = kvec[3 * kc + 2];
  const T lSc = Sc[kc], lSs = Ss[kc];
  T ax = T(0), ay = T(0), az = T(0);
  for (int64_t base = 0; base < N; base += kStepTile) {
    const int n = int(min<int64_t>(kStepTile, N - base));
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * n; t += kStepBlock) {
      sp[t] = pos[3 * base + t];
      sm[t] = mu[3 * base + t];
    }
    __syncthreads();
    if (live)
      for (int i = al; i < n; i += kStepKLanes) {
        const T x = sp[3 * i], y = sp[3 * i + 1], z = sp[3 * i + 2];
        const T mx = sm[3 * i], my = sm[3 * i + 1], mz = sm[3 * i + 2];
        T s, c;
        dipole_phase3(kx, ky, kz, x, y, z, s, c);
        const T a1 = c * lSc + s * lSs;
        const T b = (mx * kx + my * ky + mz * kz) * (c * lSs - s * lSc);
        ax += mx * a1 + b * x;
        ay += my * a1 + b * y;
        az += mz * a1 + b * z;
      }
  }
#pragma unroll
  for (int off = kStepKLanes / 2; off > 0; off >>= 1) {
    ax += __shfl_xor(ax, off, kStepKLanes);
    ay += __shfl_xor(ay, off, kStepKLanes);
    az += __shfl_xor(az, off, kStepKLanes);
  }
  if (al == 0) {
    double g[3] = {0.0, 0.0, 0.0}, e = 0.0;
    const double kd[3] = {double(kx), double(ky), double(kz)};
    if (live) {
      const double gk = double(G[kc]), s2 = double(lSc) * double(lSc) + double(lSs) * double(lSs), d = double(dG[kc]) * s2;
      g[0] = gk * double(ax) + d * kd[0];
      g[1] = gk * double(ay) + d * kd[1];
      g[2] = gk * double(az) + d * kd[2];
      e = 0.5 * gk * s2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int n = 0; n < 3; ++n) red[kl][3 * a + n] = g[a] * kd[n];
    red[kl][9] = e;
  }
  __syncthreads();
  if (threadIdx.x < kStepCellK) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kStepKPerBlock; ++q) s += red[q][threadIdx.x];
    k_part[kStepCellK * blk + threadIdx.x] = s;
  }
}

// ---- 6. finish (the text of dipole_cell_step_finish_kernel, for the batch alone: see the head): 16 lanes per atom, lane l adds the
// slices l, l + 16, ... in that order, then the 16 lanes are added by the shuffle tree of the rows; 1/V and bg/V from the geometry
// record
template <typename T>
__device__ __forceinline__ void ds_finish_body(int64_t N, int n_slices, int64_t blk, T self_term, double background,
                                               const double* __restrict__ geom, const AtomRecord<T>* __restrict__ recm,
                                               const T* __restrict__ part, const T* __restrict__ row_out,
                                               const double* __restrict__ mu_part, int64_t n_mu_blocks, T* __restrict__ forces,
                                               T* __restrict__ grad_mu, double* __restrict__ e_part) {
  __shared__ double red[kStepWaves];
  const double inv_vol_d = geom[9];
  const T inv_vol = T(inv_vol_d), bg_over_v = T(background * inv_vol_d);
  double M[3] = {0.0, 0.0, 0.0};
  if (background != 0.0) {  // (uniform, and the same for every cell) sum_j mu_j, the same fixed order in every block
#pragma unroll
    for (int c = 0; c < 3; ++c) M[c] = step_strided_sum(mu_part, n_mu_blocks, 3, c, red);
  }
  const int sub = threadIdx.x % 16;
  const int64_t a = blk * kStepRowsPerBlock + threadIdx.x / 16;
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
  if (threadIdx.x == 0) e_part[blk] = e;
}

// ---- 7. final (dipole_step_final_kernel, dipole_cell_step_final_kernel): one block per system: E, and
// dE/dcell = rows - A^-T W / V - (E_k + E_bg) A^-T with W = sum_k (dE_raw/dk) (x) k.  inv_cell: A^-1 row-major, in T (the caller's
// table) or in double (the geometry record); inv_vol is read with the cell gradient only; bad (uniform): NaN for a singular cell
template <typename T, bool CELL, typename Inv>
__device__ __forceinline__ void ds_final_core(int64_t n_e_blocks, const double* __restrict__ e_part, T* __restrict__ energy,
                                              int64_t n_row_blocks, const double* __restrict__ row_cell, int64_t n_k_blocks,
                                              const double* __restrict__ k_cell, int64_t n_mu_blocks,
                                              const double* __restrict__ mu_part, const double* __restrict__ inv_vol_p, double bg,
                                              const Inv* __restrict__ inv_cell, bool bad, T* __restrict__ grad_cell) {
  __shared__ double red[kStepWaves];
  __shared__ double tot[9 + kStepCellK + 3];
  const double E = step_strided_sum(e_part, n_e_blocks, 1, 0, red);
  if (threadIdx.x == 0) energy[0] = bad ? T(NAN) : T(E);
  if (CELL) {
    step_cell_totals(row_cell, n_row_blocks, k_cell, n_k_blocks, tot, red);
    for (int j = 0; j < 3; ++j) {
      const double s = step_strided_sum(mu_part, n_mu_blocks, 3, j, red);
      if (threadIdx.x == 0) tot[9 + kStepCellK + j] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
      const int m = threadIdx.x / 3, n = threadIdx.x % 3;
      const double* Wr = tot;
      const double* Wk = tot + 9;
      const double Ek = tot[9 + 9], inv_vol = inv_vol_p[0];
      const double* M = tot + 9 + kStepCellK;
      const double e_v = inv_vol * (Ek + 0.5 * bg * (M[0] * M[0] + M[1] * M[1] + M[2] * M[2]));  // what scales with 1/V
      double chain = 0.0;
      for (int a = 0; a < 3; ++a) chain += double(inv_cell[3 * a + m]) * Wk[3 * a + n];
      grad_cell[3 * m + n] = bad ? T(NAN) : T(Wr[3 * m + n] - inv_vol * chain - e_v * double(inv_cell[3 * n + m]));
    }
  }
}

// the step that follows its cell: A^-1, 1/V and the bad-cell flag from the geometry record
template <typename T, bool CELL>
__device__ __forceinline__ void ds_final_body(int64_t n_e_blocks, const double* __restrict__ e_part, T* __restrict__ energy,
                                              int64_t n_row_blocks, const double* __restrict__ row_cell, int64_t n_k_blocks,
                                              const double* __restrict__ k_cell, int64_t n_mu_blocks,
                                              const double* __restrict__ mu_part, double bg, const double* __restrict__ geom,
                                              T* __restrict__ grad_cell) {
  ds_final_core<T, CELL, double>(n_e_blocks, e_part, energy, n_row_blocks, row_cell, n_k_blocks, k_cell, n_mu_blocks, mu_part,
                                 geom + 9, bg, geom, geom[10] != 0.0, grad_cell);
}

}  // namespace mipme
