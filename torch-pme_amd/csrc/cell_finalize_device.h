// The finalize launch of an energy step's cell gradient: one workgroup assembles dE/dcell from the partial sums the step's kernels
// left behind.  A header of its own, for the single-frame kernel and the frame batch's (kfilter.hip) and for the batch's kernel
// with the slab term (frames_slab.hip).
#pragma once
#include "kpot.h"  // kPi

namespace mipme {

// doubles per cell rider row (cell_rider_body, kfilter.hip): 15 moments, 9 pair sums, E_k
static constexpr int kCellRow = 25;

// ---- dE/dcell of an energy step (E = sum q V, seed s), assembled by ONE workgroup from partial sums the step's kernels left
// behind (SURVEY.md Appendix A.5 with g = s q, i.e. psi = (s / 2V) rho):
//   rows[r][25]    cell riders (cell_rider_body): 15 moments of mu |rho^|^2 against the filter's derivative table
//                    M1[e][d] = sum w alpha f_e f_d (00 01 02 11 12 22),  M2[c][d] = sum w beta_c f_d
//                  => K[c][d] = 2 pi sum_k w dG/dk_c f_d = 2 pi (2 pi sum_e Ai[c][e] M1[e][d] - h_c M2[c][d]),
//                     H[c]    = sum_k w dG/dh_c = -2 pi sum_e Ai[c][e] M2[c][e],           h_c = |a_c| / n_c
//                  then 9 sums of the pair kernel  C[i][c] = sum_rows q_a sum_e w_e v'/d sh_i u_c,
//                  then E_k = sum_k mu G |rho^|^2  (= V sum_a q_a Phi_a: the gather is the adjoint of the spread)
//   rpart[b][9]    gather:   R[c][e] = sum_a r_{a,c} (s q_a field_{a,e})                                           (per brick)
// mesh part  gA[a][b] = -sum_c Ai[c][a] R[c][b] - (s/2V) sum_cd Ai[c][a] K[c][d] Ai[b][d] + dLdV V Ai[b][a]
//                       + (s/2V) H[a] / (|a_a| n_a) A[a][b],      dLdV = -s E_k / (2 V^2) + s bg Q^2 / V^2
// pair part  gP[m][c] = s f/2 sum_i Ai[i][m] C[i][c]   (every pair sits in two rows; f = 1/2 for a full list)
// out: 27 reals: mesh part, pair part, their sum.  Column sums: 25 groups of 16 lanes (rider rows) and 9 groups of 32 lanes
// (brick rows), sixteen loads in flight per lane -- a plain accumulation loop is a chain of dependent cold loads (the inputs
// were written by other XCDs a moment ago): 6.7 us for this kernel --, then 18 threads for the 3x3 algebra.
// SLAB: + the slab term of the step (GatherTail), which depends on the cell through V and L = |a_axis| alone (z is Cartesian):
//   gA[a][b] += -s E_slab Ai[b][a] - [a == axis] s c0 Q^2 L / 12 * A[a][b] / L,   E_slab = c0/2 (M^2 - Q M2 - Q^2 L^2 / 12)
struct SlabCell {
  const double* mom;  // {Q, M, M2}
  double c0, L;
  int axis;
};
template <typename T, bool SLAB>
__device__ __forceinline__ void cell_tail_finalize_body(mipme_mesh_t m, double bg, double pair_scale, int n_rows,
                                                        int n_bricks, const double* __restrict__ rows,
                                                        const double* __restrict__ rpart, const T* __restrict__ dc,
                                                        const T* __restrict__ seed, T* __restrict__ out, SlabCell sc) {
  __shared__ double gs[34], geo[18], s[31], res[18];
  {
    const int t = threadIdx.x;
    const double* base = nullptr;
    int n = 0, stride = 1, lanes = 16, l = 0, g = -1;
    if (t < 16 * kCellRow) {
      g = t >> 4, l = t & 15, lanes = 16;
      base = rows + g, n = n_rows, stride = kCellRow;
    } else if (t < 16 * kCellRow + 32 * 9) {
      const int u = t - 16 * kCellRow;
      g = kCellRow + (u >> 5), l = u & 31, lanes = 32;
      base = rpart + (u >> 5), n = n_bricks, stride = 9;
    }
    double v = 0.0;
    constexpr int B = 16;
    for (int i0 = l; i0 < n; i0 += lanes * B) {
      double tmp[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int i = i0 + lanes * u;
        tmp[u] = i < n ? base[int64_t(i) * stride] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) v += tmp[u];
    }
    // (16-lane groups are aligned to 16, 32-lane groups to 32 -- 16 * 25 = 400 is a multiple of 16 but not of 32: reduce both
    // with xor steps inside aligned 16-lane halves and combine the halves of a 32-lane group through LDS atomics-free adds)
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
    if (g >= 0 && g < kCellRow && l == 0) gs[g] = v;
    __shared__ double half[9][2];
    if (g >= kCellRow && (l & 15) == 0) half[g - kCellRow][l >> 4] = v;
    if (threadIdx.x == 1023) {  // cell and inverse cell to LDS with static indices (scalar loads of the by-value argument; the
                                // threads below index them by thread)
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        geo[i] = m.cell[i];
        geo[9 + i] = m.inv_cell[i];
      }
    }
    __syncthreads();
    if (threadIdx.x < 9) gs[kCellRow + threadIdx.x] = half[threadIdx.x][0] + half[threadIdx.x][1];
  }
  __syncthreads();
  const double* A = geo;
  const double* Ai = geo + 9;
  // s[0..8] = K, s[9..11] = H, s[12..20] = C, s[21..29] = R, s[30] = E_k
  if (threadIdx.x < 31) {
    const int t = threadIdx.x;
    double v;
    if (t < 9) {
      const int cc = t / 3, d = t % 3;
      double a = 0.0;
      for (int e = 0; e < 3; ++e) {
        const int lo = e < d ? e : d, hi = e < d ? d : e;
        a += Ai[3 * cc + e] * gs[lo * 3 - lo * (lo - 1) / 2 + (hi - lo)];
      }
      const double hc = sqrt(A[3 * cc] * A[3 * cc] + A[3 * cc + 1] * A[3 * cc + 1] + A[3 * cc + 2] * A[3 * cc + 2]) /
                        double(cc == 0 ? m.nx : (cc == 1 ? m.ny : m.nz));
      v = 2.0 * kPi * (2.0 * kPi * a - hc * gs[6 + 3 * cc + d]);
    } else if (t < 12) {
      const int cc = t - 9;
      double a = 0.0;
      for (int e = 0; e < 3; ++e) a += Ai[3 * cc + e] * gs[6 + 3 * cc + e];
      v = -2.0 * kPi * a;
    } else if (t < 21) {
      v = gs[15 + (t - 12)];
    } else if (t < 30) {
      v = gs[kCellRow + (t - 21)];
    } else {
      v = gs[24];
    }
    s[t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 18) {
    const double sd = seed ? double(seed[0]) : 1.0;
    const double V = m.volume, es = 0.5 * sd / V;
    if (threadIdx.x < 9) {
      const int a = threadIdx.x / 3, b = threadIdx.x % 3;
      const int nsa = a == 0 ? m.nx : (a == 1 ? m.ny : m.nz);
      const double Q = double(dc[0]);
      const double dLdV = -sd * s[30] / (2.0 * V * V) + sd * bg * Q * Q / (V * V);
      double v = 0.0;
      for (int c = 0; c < 3; ++c) {
        v -= Ai[3 * c + a] * s[21 + 3 * c + b];
        for (int d = 0; d < 3; ++d) v -= es * Ai[3 * c + a] * s[3 * c + d] * Ai[3 * b + d];
      }
      const double norm = sqrt(A[3 * a] * A[3 * a] + A[3 * a + 1] * A[3 * a + 1] + A[3 * a + 2] * A[3 * a + 2]);
      v += dLdV * V * Ai[3 * b + a] + es * s[9 + a] / (norm * double(nsa)) * A[3 * a + b];
      if constexpr (SLAB) {
        const double sQ = sc.mom[0], sM = sc.mom[1], sM2 = sc.mom[2];
        const double e_slab = 0.5 * sc.c0 * (sM * sM - sQ * sM2 - sQ * sQ * sc.L * sc.L / 12.0);
        v -= sd * e_slab * Ai[3 * b + a];
        if (a == sc.axis) v -= sd * sc.c0 * sQ * sQ / 12.0 * A[3 * a + b];
      }
      out[threadIdx.x] = T(v);
      res[threadIdx.x] = v;
    } else {
      const int mm = (threadIdx.x - 9) / 3, c = (threadIdx.x - 9) % 3;
      double v = 0.0;
      for (int i = 0; i < 3; ++i) v += Ai[3 * i + mm] * s[12 + 3 * i + c];
      v *= sd * pair_scale;
      out[threadIdx.x] = T(v);
      res[threadIdx.x] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 9) out[18 + threadIdx.x] = T(res[threadIdx.x] + res[9 + threadIdx.x]);  // the sum, for callers with ONE cell tensor
}

}  // namespace mipme
