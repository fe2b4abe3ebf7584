// gfx950 kernels of the moment loss along a beam trace (lynx_moments_along_loss, lynx_moments_along_loss_backward): the
// weighted sum of squared distances of named beam properties at chosen points of a trace to target values, and its
// cotangents, formed from the states that the trace left on the device.  Included only by lynx_hip.hip, behind
// lynx_trace_grad.hpp.
//
// A target point is (point, mask): bit k of the mask names property k of
//   0..5 mu_x .. mu_p, 6..11 sigma_x .. sigma_p, 12 sigma_xxp, 13 sigma_yyp, 14|15 emittance_x|y,
//   16|17 normalized_emittance_x|y, 18|19 beta_x|y, 20|21 alpha_x|y, 22 energy,
// and the terms of a sample are ordered by (point, bit).  A term's row is (target, weight) float64.  The value of a term
// is the float64 expression whose derivative grad.trace_property_cotangents forms on the host:
//   records form   n = rec[35], scale = n / (n - ddof), s2_c = rec[tri(c, c)] scale, cross_a = rec[tri(a, a + 1)]
//   moments form   s2_c = max(cov_cc, floor), floor = T(1e-20), derivative 0 where clamped, cross_a = cov[a][a + 1]
//   both           q = s2 p2 - cross^2, eps = sqrt(max(q, tiny)), tiny = the smallest normal T, derivative 0 where q <= tiny;
//                  sigma = sqrt(s2), beta = s2 / eps, alpha = -cross / eps, normalized emittance = eps gamma sqrt(1 - 1 /
//                  gamma^2), gamma = energy / m_e (0 with derivative 0 at gamma == 0)
// All arithmetic is float64 for both dtypes (a float32 state is widened on load), nothing is contracted to an FMA, and the
// reverse kernel recomputes the values by the forward kernel's function: the same bits.
//
//   k_moment_loss_fwd      one thread per (sample, target point): the point's state read once, every value of its mask to
//                          values[b][t], the point's partial loss (added in bit order) to point_loss[b][q]
//   k_moment_loss_finish   one thread per sample: loss[b] = the Q partial losses added in point order
//   k_moment_loss_bwd      one thread per (sample, target point): per term loss_bar[b] 2 w (value - target) through the host
//                          rule, accumulated per plane in registers, then one read-add-write per touched entry
// Target points are distinct, so no two threads touch one entry: no atomics, the same call returns the same bits.  The
// target points come by value, kMomentLossPoints of them per launch.
#pragma once

#include <limits>

#include "lynx_device.hpp"

namespace lynx {

constexpr int kMomentLossThreads = 64;
constexpr int kMomentLossPoints = 64;
constexpr int kMomentLossProperties = 23;
// the properties that read eps of plane x (bit 14, 16, 18, 20) and y, and those that read the energy
constexpr int kMomentLossEpsX = (1 << 14) | (1 << 16) | (1 << 18) | (1 << 20);
constexpr int kMomentLossEpsY = kMomentLossEpsX << 1;
constexpr int kMomentLossNormalized = (1 << 16) | (1 << 17);
constexpr int kMomentLossEnergy = kMomentLossNormalized | (1 << 22);

struct MomentLossPoints {
  int point[kMomentLossPoints];
  int mask[kMomentLossPoints];
  int term[kMomentLossPoints];  // the ordinal of the point's first term among a sample's T
};

__host__ __device__ constexpr int moment_loss_tri(int i, int j) { return 7 + i * 6 - (i * (i - 1)) / 2 + (j - i); }

// What a point's properties are written in.  s2[c] = sigma_c^2 and ds2[c] its derivative by the variance read.
struct MomentPointState {
  double mu[6], s2[6], ds2[6], cross[2], eps[2], energy, bg, dbg;
  bool free_[2];  // q > tiny: eps has a derivative
};

template <typename T, bool kRecords>
__device__ __forceinline__ MomentPointState moment_point_state(const double* __restrict__ rec, const T* __restrict__ mu,
                                                               const T* __restrict__ cov, const T* __restrict__ energy,
                                                               int ddof, int mask) {
  MomentPointState p;
  if constexpr (kRecords) {
    const double n = rec[35];
    const double scale = n / (n - (double)ddof);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      p.mu[c] = rec[c];
      p.s2[c] = rec[moment_loss_tri(c, c)] * scale;
      p.ds2[c] = scale;
    }
    p.cross[0] = rec[moment_loss_tri(0, 1)];
    p.cross[1] = rec[moment_loss_tri(2, 3)];
  } else {
    const double floor_ = (double)(T)1e-20;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      p.mu[c] = (double)mu[c];
      const double v = (double)cov[c * 7 + c];
      p.s2[c] = v <= floor_ ? floor_ : v;  // (a NaN stays one)
      p.ds2[c] = v > floor_ ? 1.0 : 0.0;
    }
    p.cross[0] = (double)cov[0 * 7 + 1];
    p.cross[1] = (double)cov[2 * 7 + 3];
  }
  const double tiny = (double)std::numeric_limits<T>::min();
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double q = p.s2[2 * a] * p.s2[2 * a + 1] - p.cross[a] * p.cross[a];
    p.eps[a] = sqrt(q <= tiny ? tiny : q);
    p.free_[a] = q > tiny;
  }
  p.energy = (double)*energy;
  p.bg = p.dbg = 0.0;
  if (mask & kMomentLossNormalized) {
    const double gamma = p.energy / LYNX_ELECTRON_MASS_EV;
    if (fabs(gamma) > 0) {
      p.bg = sqrt(1 - 1 / (gamma * gamma)) * gamma;  // relativistic beta . gamma
      p.dbg = gamma / sqrt(gamma * gamma - 1) / LYNX_ELECTRON_MASS_EV;
    }
  }
  return p;
}

// (k is a constant wherever this is called: the loops over the properties are unrolled)
__device__ __forceinline__ double moment_value(const MomentPointState& p, int k) {
  if (k < 6) return p.mu[k];
  if (k < 12) return sqrt(p.s2[k - 6]);
  if (k < 14) return p.cross[k - 12];
  if (k < 16) return p.eps[k - 14];
  if (k < 18) return p.eps[k - 16] * p.bg;
  if (k < 20) return p.s2[2 * (k - 18)] / p.eps[k - 18];
  if (k < 22) return -p.cross[k - 20] / p.eps[k - 20];
  return p.energy;
}

template <typename T, bool kRecords>
__global__ __launch_bounds__(kMomentLossThreads) void k_moment_loss_fwd(
    const double* __restrict__ records, const T* __restrict__ mu_trace, const T* __restrict__ cov_trace,
    const T* __restrict__ energy_trace, int64_t B, int P, int ddof, MomentLossPoints points, int first, int count, int Q,
    int n_terms, const double* __restrict__ rows, int64_t row_stride, double* __restrict__ values,
    double* __restrict__ point_loss) {
  const int64_t pair = (int64_t)blockIdx.x * kMomentLossThreads + threadIdx.x;
  if (pair >= B * count) return;
  const int64_t b = pair / count;
  const int j = (int)(pair - b * count);
  const int mask = points.mask[j];
  const int64_t at = b * P + points.point[j];
  const MomentPointState p = moment_point_state<T, kRecords>(kRecords ? records + at * LYNX_MOMENT_STRIDE : nullptr,
                                                             kRecords ? nullptr : mu_trace + at * 7,
                                                             kRecords ? nullptr : cov_trace + at * 49, energy_trace + at, ddof, mask);
  int t = points.term[j];
  double loss = 0.0;
#pragma unroll
  for (int k = 0; k < kMomentLossProperties; ++k) {
    if ((mask >> k) & 1) {
      const double* row = rows + b * row_stride + 2 * (int64_t)t;
      const double value = moment_value(p, k);
      const double d = value - row[0];
      values[b * n_terms + t] = value;
      loss += row[1] * (d * d);
      ++t;
    }
  }
  point_loss[b * Q + first + j] = loss;
}

__global__ __launch_bounds__(kMomentLossThreads) void k_moment_loss_finish(const double* __restrict__ point_loss, int64_t B, int Q,
                                                                           double* __restrict__ loss) {
  const int64_t b = (int64_t)blockIdx.x * kMomentLossThreads + threadIdx.x;
  if (b >= B) return;
  double sum = 0.0;
  for (int q = 0; q < Q; ++q) sum += point_loss[b * Q + q];
  loss[b] = sum;
}

// d eps: `bar` through eps = sqrt(max(q, tiny)) into the plane's three accumulators (0 where clamped)
__device__ __forceinline__ void moment_eps_bar(const MomentPointState& p, int a, double bar, double& s2b, double& p2b, double& crb) {
  const double w = p.free_[a] ? bar / (2.0 * p.eps[a]) : 0.0;
  s2b += w * p.s2[2 * a + 1];
  p2b += w * p.s2[2 * a];
  crb += -2.0 * w * p.cross[a];
}

template <typename T>
__device__ __forceinline__ void moment_add(T* entry, double bar) {  // one read-add-write, rounded once
  *entry = (T)((double)*entry + bar);
}

template <typename T, bool kRecords>
__global__ __launch_bounds__(kMomentLossThreads) void k_moment_loss_bwd(
    const double* __restrict__ records, const T* __restrict__ mu_trace, const T* __restrict__ cov_trace,
    const T* __restrict__ energy_trace, int64_t B, int P, int ddof, MomentLossPoints points, int count,
    const double* __restrict__ rows, int64_t row_stride, const double* __restrict__ loss_bar, double* __restrict__ grad_trace,
    T* __restrict__ mu_bar, T* __restrict__ cov_bar, T* __restrict__ energy_bar /* or null */) {
  const int64_t pair = (int64_t)blockIdx.x * kMomentLossThreads + threadIdx.x;
  if (pair >= B * count) return;
  const int64_t b = pair / count;
  const int j = (int)(pair - b * count);
  const int mask = points.mask[j];
  const int64_t at = b * P + points.point[j];
  const MomentPointState p = moment_point_state<T, kRecords>(kRecords ? records + at * LYNX_MOMENT_STRIDE : nullptr,
                                                             kRecords ? nullptr : mu_trace + at * 7,
                                                             kRecords ? nullptr : cov_trace + at * 49, energy_trace + at, ddof, mask);
  const double lb = loss_bar[b];
  double mub[6] = {0, 0, 0, 0, 0, 0}, varb[6] = {0, 0, 0, 0, 0, 0};
  double s2b[2] = {0, 0}, p2b[2] = {0, 0}, crb[2] = {0, 0}, eb = 0.0;
  int t = points.term[j];
#pragma unroll
  for (int k = 0; k < kMomentLossProperties; ++k) {
    if ((mask >> k) & 1) {
      const double* row = rows + b * row_stride + 2 * (int64_t)t;
      const double bar = lb * (2.0 * row[1] * (moment_value(p, k) - row[0]));
      ++t;
      if (k < 6) {
        mub[k] += bar;
      } else if (k < 12) {
        const int c = k - 6;
        varb[c] += p.ds2[c] != 0 ? bar * p.ds2[c] / (2.0 * sqrt(p.s2[c])) : 0.0;
      } else if (k < 14) {
        crb[k - 12] += bar;
      } else if (k < 16) {
        const int a = k - 14;
        moment_eps_bar(p, a, bar, s2b[a], p2b[a], crb[a]);
      } else if (k < 18) {
        const int a = k - 16;
        moment_eps_bar(p, a, bar * p.bg, s2b[a], p2b[a], crb[a]);
        eb += bar * p.eps[a] * p.dbg;
      } else if (k < 20) {
        const int a = k - 18;
        s2b[a] += bar / p.eps[a];
        moment_eps_bar(p, a, -bar * p.s2[2 * a] / (p.eps[a] * p.eps[a]), s2b[a], p2b[a], crb[a]);
      } else if (k < 22) {
        const int a = k - 20;
        crb[a] += -bar / p.eps[a];
        moment_eps_bar(p, a, bar * p.cross[a] / (p.eps[a] * p.eps[a]), s2b[a], p2b[a], crb[a]);
      } else {
        eb += bar;
      }
    }
  }
  double* g = kRecords ? grad_trace + at * LYNX_MOMENT_STRIDE : nullptr;
  T* mb = kRecords ? nullptr : mu_bar + at * 7;
  T* cb = kRecords ? nullptr : cov_bar + at * 49;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if ((mask >> c) & 1) {
      if constexpr (kRecords) moment_add(g + c, mub[c]);
      else moment_add(mb + c, mub[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const bool plane = c < 4 && (mask & (c < 2 ? kMomentLossEpsX : kMomentLossEpsY));
    if (!(((mask >> (6 + c)) & 1) || plane)) continue;
    double bar = varb[c];
    if (plane) bar += (c & 1 ? p2b[c / 2] : s2b[c / 2]) * p.ds2[c];
    if constexpr (kRecords) moment_add(g + moment_loss_tri(c, c), bar);
    else moment_add(cb + c * 7 + c, bar);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    if (!(mask & ((a ? kMomentLossEpsY : kMomentLossEpsX) | (1 << (12 + a))))) continue;
    if constexpr (kRecords) moment_add(g + moment_loss_tri(2 * a, 2 * a + 1), crb[a]);  // (an off-diagonal entry counted once)
    else moment_add(cb + 2 * a * 7 + 2 * a + 1, crb[a]);
  }
  if (mask & kMomentLossEnergy) moment_add(energy_bar + at, eb);
}

}  // namespace lynx
