// gfx950 kernels of the beam trace's FORWARD-mode pass: the tangents of the beam moments at EVERY point of a lattice
// along D directions in parameter space (lynx_track_moments_along_forward, lynx_track_particles_along_forward).
// Included only by lynx_hip.hip, behind lynx_trace_grad.hpp.
//
// The reverse pass (lynx_trace_grad.hpp) answers one scalar loss and gives its gradient with respect to every parameter;
// this is the other shape: few parameters, every output -- the orbit response matrix (d centroid at every BPM / d angle of
// every corrector), the Jacobian of residuals of a least-squares matching, "how does beta_x at every point move when Q3 is
// turned".  The trace's program has every leaf element as a step of its own (LYNX_STEP_FLAG_RAW: S = E, P = E + 1), and
// without a cavity step every element is an affine map of the 7-vector, so for a direction d
//
//   mu_dot[0] = 0, C_dot[0] = 0
//   for k = 1 .. S:
//     Mdot = sum over the direction's entries at element k - 1 of weight . dM_{k-1}/d(parameter or energy)   (none for most k)
//     mu_dot[k] = M mu_dot[k-1] + Mdot mu[k-1]
//     C_dot[k]  = M C_dot[k-1] M^T + X + X^T,   X = Mdot C[k-1] M^T
//
// with mu[k], C[k] READ from the forward trace, as k_trace_moments_bwd reads them, and M the step's row of the trace's
// table.  The mean and the biased covariance of a ParticleBeam obey the same recursion exactly (the head of
// lynx_trace_grad.hpp), so its tangents come from the moment records and no pass over the particles is made.
//
// A direction is a short list of entries (leaf, parameter row 0 .. 7 or kGradParams for the step energy, weight), the
// whole set in CSR form -- dir_start [D + 1], dir_leaf [n], dir_row [n], dir_weight [n] float64 -- with the entries of one
// direction ordered by leaf (the host orders them).  That covers an element object that occurs several times, RBend's
// `angle` (which feeds e1 and e2 with weight 1/2), the two rows of a vector parameter and the incoming energy (one
// kGradParams entry per leaf, weight 1).
//
// The sweep's own arithmetic is float64 for every lattice dtype, for the reason the head of lynx_trace_grad.hpp gives: the
// tangent of a Twiss value is the contraction of C_dot with -(beta / 2 eps) C^-1 and its like, which cancels (1 +
// alpha^2)-fold.  The maps and dM are the lattice's dtype (the builders'); the states are read as the trace left them.
//
//   k_trace_tangent_maps      one thread per (sample, entry): weight . dM of that entry's element along that entry's row by
//                             dual evaluation (step 3 of build_bwd_sample), 49 float64 to [B][n][49]
//   k_trace_records_to_moments   ParticleBeam: moment records [B][P][36] float64 -> mu, C of the sweep
//                             (k_trace_records_to_states without its cotangent half)
//   k_trace_moments_jvp       the sweep, one wave per (sample, direction)
#pragma once

#include "lynx_device.hpp"
#include "lynx_grad.hpp"
#include "lynx_trace.hpp"

namespace lynx {

// The directions on the device, one block: int32 dir_start [D + 1] | dir_leaf [n] | dir_row [n], then (8-aligned) float64
// dir_weight [n].
struct TraceDirections {
  const int32_t* start;
  const int32_t* leaf;
  const int32_t* row;
  const double* weight;
  int32_t count;    // D
  int32_t entries;  // n
};

// ---------------------------------------------------------------------------------------
// k_trace_tangent_maps: grid = ceil(B n / 64), 64 threads, thread = (sample, entry).  What step 3 of build_bwd_sample does
// per (element, parameter): the element's builder on dual numbers with the tangent seed on the entry's row (row ==
// kGradParams: on the step energy), through the 16 entries of class U in registers where the kind has that structure
// (build_entries_u: an entry outside the pattern has derivative zero) and through build_element otherwise.  The program
// has no cavity step (refused by the host), so the energy at every step is the incoming one -- what the trace's energy
// record holds at every point.  A kind without parameters (identity, custom map) has no derivative: zeros.  The
// derivative conventions are the builders' (lynx_dual.hpp).  Every thread writes its 49 cells.
// (Compiled for k_build_bwd's waves per SIMD, not for speed of its own: the dual-number builders are out-of-line functions
// that the two kernels SHARE, and the register budget they are compiled for is the loosest of their callers' -- without the
// attribute here k_build_bwd<float> went from 72 registers and six waves to 132 and three, and BASELINE config 5's reverse
// pass from 2.00 to 2.08 ms.)
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 7 : 1))) void k_trace_tangent_maps(LatticeDev lat, const T* __restrict__ energy_in, TraceDirections dirs,
                                                           double* __restrict__ mdot /* [B][n][49] */) {
  const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t n = dirs.entries;
  if (t >= lat.batch * n) return;
  const int64_t b = t / n;
  const int q = (int)(t - b * n);
  const int e = dirs.leaf[q], pidx = dirs.row[q];
  const double w = dirs.weight[q];
  double* out = mdot + t * 49;
  const lynx_elem el = lat.elems[e];
  const int np = bwd_kind_params_dev(el.kind);
  const bool energy_task = pidx == kGradParams;
  if (np == 0) {
    for (int c = 0; c < 49; ++c) out[c] = 0.0;
    return;
  }
  const T* p = static_cast<const T*>(lat.pool) + el.param_offset + b * (int64_t)el.batch_stride;
  Dual<T> dp[8];
  for (int k = 0; k < 8; ++k) dp[k] = Dual<T>(k < np ? p[k] : T(0), (k == pidx) ? T(1) : T(0));
  const Dual<T> de(energy_in[b], energy_task ? T(1) : T(0));
  Dual<T> m16[16];
  if (build_entries_u<Dual<T>>(el.kind, el.flags, dp, de, m16, nullptr)) {
    for (int c = 0; c < 49; ++c) out[c] = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) out[unit_entry_u(k)] = w * (double)m16[k].d;
  } else {
    Dual<T> dM[49];
    build_element<Dual<T>>(el.kind, el.flags, dp, de, dM, nullptr);
    for (int c = 0; c < 49; ++c) out[c] = w * (double)dM[c].d;
  }
}

// ---------------------------------------------------------------------------------------
// k_trace_records_to_moments: grid = B * P, 64 threads.  Record layout of LYNX_MOMENT_STRIDE: [0..6] mean, [7..27] the
// upper triangle of the biased covariance; the 7th row and column of C are zero (the 7th coordinate is 1 for every
// particle).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_trace_records_to_moments(const double* __restrict__ trace_fwd, double* __restrict__ mu,
                                                                 double* __restrict__ cov) {
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const double* rec = trace_fwd + p * LYNX_MOMENT_STRIDE;
  if (lane < 7) mu[p * 7 + lane] = lane < 6 ? rec[lane] : 1.0;
  if (lane < 49) {
    const int i = lane / 7, j = lane - i * 7;
    double c = 0.0;
    if (i < 6 && j < 6) {
      const int r = i < j ? i : j, q = i < j ? j : i;
      c = rec[7 + r * 6 - (r * (r - 1)) / 2 + (q - r)];
    }
    cov[p * 49 + lane] = c;
  }
}

// ---------------------------------------------------------------------------------------
// k_trace_moments_jvp: grid = B * D, one wave per (sample, direction), 49 lanes busy (lane = entry i * 7 + j; lanes 0 .. 6
// also own mu_dot).  Per step, with the state that ENTERS it (point s of the forward trace), its row M and -- if the
// direction has an entry at this leaf -- Mdot, the sum of the direction's entries there in entry order:
//   row, state and Mdot from registers to LDS                                 | barrier
//   Y = C_dot M^T,  Z = C M^T (with Mdot only)                                | barrier
//   mu_dot' = M mu_dot (+ Mdot mu),   C_dot' = M Y (+ X + X^T, X = Mdot Z: a lane forms its own X_ij and X_ji)
//   every read of mu_dot, C_dot                                              | barrier
//   mu_dot', C_dot' over them and out to point s + 1                         (the next step's first barrier follows)
// A step WITHOUT an entry of the direction skips the Mdot terms altogether -- it does not multiply by a zero matrix, so a
// NaN map or state elsewhere does not reach it.  The 7th coordinate is the constant 1: entry 6 of mu_dot and row and
// column 6 of C_dot are written as the exact zeros they are, at every point.  What step s + 1 needs from memory (row,
// state, the entries' Mdot: independent of the sweep) is fetched while step s is worked on -- the sweep is a chain of small
// dependent products, and a wave would otherwise wait for memory once per step.  One lane owns every cell it writes, the
// sums run in a fixed order, no atomics: the same call returns the same bits.
// ---------------------------------------------------------------------------------------
template <typename T, typename ST>
__global__ __launch_bounds__(64) void k_trace_moments_jvp(int S, TraceDirections dirs, const T* __restrict__ steps,
                                                          const ST* __restrict__ mu_trace, const ST* __restrict__ cov_trace,
                                                          const double* __restrict__ mdot /* [B][n][49] */,
                                                          double* __restrict__ mu_dot /* [B][D][P][7] */,
                                                          double* __restrict__ cov_dot /* [B][D][P][49] */) {
  using A = double;  // the sweep's own arithmetic, whatever the lattice's dtype (see the head of this file)
  __shared__ A s_m[64], s_mu[8], s_c[49], s_d[49], s_md[8], s_cd[49], s_y[49], s_z[49];
  const int D = dirs.count;
  const int64_t b = blockIdx.x / D;
  const int d = (int)(blockIdx.x - b * D);
  const int lane = threadIdx.x;
  const int cl = lane < 49 ? lane : 48, l7 = lane < 7 ? lane : 6;
  const int i = cl / 7, j = cl % 7;
  const int P = S + 1;
  const bool constant = i == 6 || j == 6;  // the 7th coordinate: no tangent
  const T* g_steps = steps + b * (int64_t)S * LYNX_STEP_STRIDE;
  const ST* g_mu = mu_trace + b * (int64_t)P * 7;
  const ST* g_c = cov_trace + b * (int64_t)P * 49;
  const double* g_d = mdot + b * (int64_t)dirs.entries * 49;
  double* o_mu = mu_dot + (b * D + d) * (int64_t)P * 7;
  double* o_c = cov_dot + (b * D + d) * (int64_t)P * 49;
  int q = dirs.start[d];
  const int q_end = dirs.start[d + 1];

  // point 0: no parameter reaches the incoming beam
  if (lane < 7) {
    s_md[lane] = A(0);
    o_mu[lane] = A(0);
  }
  if (lane < 49) {
    s_cd[lane] = A(0);
    o_c[lane] = A(0);
  }
  // (clamped lanes read a valid cell twice and use nothing of it)
  A n_m = A(0), n_mu = A(0), n_c = A(0), n_d = A(0);
  bool n_has = false;
  int at = q < q_end ? dirs.leaf[q] : -1;  // the leaf of the direction's next entry (uniform)
  const auto fetch = [&](int s) {
    n_m = (A)g_steps[(int64_t)s * LYNX_STEP_STRIDE + lane];
    n_mu = (A)g_mu[(int64_t)s * 7 + l7];
    n_c = (A)g_c[(int64_t)s * 49 + cl];
    n_d = A(0);
    n_has = false;
    while (at == s) {  // (uniform)
      n_d += g_d[(int64_t)q * 49 + cl];
      n_has = true;
      ++q;
      at = q < q_end ? dirs.leaf[q] : -1;
    }
  };
  if (S > 0) fetch(0);
  for (int s = 0; s < S; ++s) {
    s_m[lane] = n_m;
    if (lane < 7) s_mu[lane] = n_mu;
    if (lane < 49) {
      s_c[lane] = n_c;
      s_d[lane] = n_d;
    }
    const bool has = n_has;
    if (s + 1 < S) fetch(s + 1);
    __syncthreads();
    A y = s_cd[i * 7] * s_m[j * 7], z = A(0);  // Y = C_dot M^T
#pragma unroll
    for (int k = 1; k < 7; ++k) y = fma(s_cd[i * 7 + k], s_m[j * 7 + k], y);
    if (has) {
      z = s_c[i * 7] * s_m[j * 7];  // Z = C M^T
#pragma unroll
      for (int k = 1; k < 7; ++k) z = fma(s_c[i * 7 + k], s_m[j * 7 + k], z);
    }
    if (lane < 49) {
      s_y[lane] = y;
      s_z[lane] = z;
    }
    __syncthreads();
    A cd = s_m[i * 7] * s_y[j];  // M Y
#pragma unroll
    for (int k = 1; k < 7; ++k) cd = fma(s_m[i * 7 + k], s_y[k * 7 + j], cd);
    A md = s_m[l7 * 7] * s_md[0];  // M mu_dot
#pragma unroll
    for (int k = 1; k < 7; ++k) md = fma(s_m[l7 * 7 + k], s_md[k], md);
    if (has) {
      A x = s_d[i * 7] * s_z[j], xt = s_d[j * 7] * s_z[i];  // X_ij, X_ji of X = Mdot Z
#pragma unroll
      for (int k = 1; k < 7; ++k) {
        x = fma(s_d[i * 7 + k], s_z[k * 7 + j], x);
        xt = fma(s_d[j * 7 + k], s_z[k * 7 + i], xt);
      }
      cd += x + xt;
      A dm = s_d[l7 * 7] * s_mu[0];  // Mdot mu
#pragma unroll
      for (int k = 1; k < 7; ++k) dm = fma(s_d[l7 * 7 + k], s_mu[k], dm);
      md += dm;
    }
    if (constant) cd = A(0);
    if (l7 == 6) md = A(0);
    __syncthreads();
    if (lane < 7) {
      s_md[lane] = md;
      o_mu[(int64_t)(s + 1) * 7 + lane] = md;
    }
    if (lane < 49) {
      s_cd[lane] = cd;
      o_c[(int64_t)(s + 1) * 49 + lane] = cd;
    }
    // (no barrier here: what the next step writes first -- row, state, Mdot -- was last read in front of the barrier above,
    // and its own first barrier stands between these writes of mu_dot, C_dot and their reads)
  }
}

}  // namespace lynx
