// Forward-mode dual numbers for the map builders.
//
// The reverse pass of the gradient (k_build_bwd) needs dM/dtheta for every element
// parameter.  Instead of hand-deriving the partials of base_rmatrix / dipole edges / the
// cavity's T566..T555 terms, the builders of lynx_maps.hpp are instantiated a second time
// with T = Dual<float|double>: one seeded evaluation per (element, parameter) yields the
// derivative of all 49 map entries and of the 8 cavity coefficients.
// Comparisons act on the value part, so the builders take the same branches as the forward
// pass.  The derivative is that of the continuous map, not of the formulas as written where
// those cancel:
//  - `k1 == 0 -> 1e-12` (track_methods.py:67-68) keeps the derivative part, so a quadrupole at
//    k1 = 0 gets the limit of dM/dk1 (an autograd trace of the reference gives 0 there only
//    because the substitution is an in-place write);
//  - cos(sqrt(k2) L) and sin(sqrt(k2) L)/sqrt(k2) keep their values and take their derivative
//    from the power series in x = k2 L^2 while |x| < 1 (dual_series below): the closed form
//    differentiates to (L C - S)/(2 k2), which loses all digits as k2 -> 0;
//  - the bend's (1 - C)/k2 and (L - S)/k2 are that series, value and derivative (base_dx_dual):
//    their values, as the reference writes them, cancel in the same way;
//  - so does the solenoid's sin(kL)/k (solenoid_s_k_dual);
//  - the cavity's r55 bracket does not cancel (cavity_r55_bracket_dual).
#pragma once

#include "lynx_maps.hpp"

namespace lynx {

template <typename T> struct Dual {
  T v, d;
  LYNX_HD Dual() {}
  template <typename U> LYNX_HD Dual(U x) : v(T(x)), d(T(0)) {}
  LYNX_HD Dual(T v_, T d_) : v(v_), d(d_) {}
};

template <typename T> LYNX_HD Dual<T> operator+(Dual<T> a, Dual<T> b) { return Dual<T>(a.v + b.v, a.d + b.d); }
template <typename T> LYNX_HD Dual<T> operator-(Dual<T> a, Dual<T> b) { return Dual<T>(a.v - b.v, a.d - b.d); }
template <typename T> LYNX_HD Dual<T> operator-(Dual<T> a) { return Dual<T>(-a.v, -a.d); }
template <typename T> LYNX_HD Dual<T> operator*(Dual<T> a, Dual<T> b) {
  return Dual<T>(a.v * b.v, a.d * b.v + a.v * b.d);
}
template <typename T> LYNX_HD Dual<T> operator/(Dual<T> a, Dual<T> b) {
  const T q = a.v / b.v;
  return Dual<T>(q, (a.d - q * b.d) / b.v);
}
template <typename T> LYNX_HD bool operator==(Dual<T> a, Dual<T> b) { return a.v == b.v; }
template <typename T> LYNX_HD bool operator!=(Dual<T> a, Dual<T> b) { return a.v != b.v; }
template <typename T> LYNX_HD bool operator>(Dual<T> a, Dual<T> b) { return a.v > b.v; }
template <typename T> LYNX_HD bool operator<(Dual<T> a, Dual<T> b) { return a.v < b.v; }

// d/dx: sqrt -> 1/(2 sqrt x); sin -> cos; cos -> -sin; tan -> 1 + tan^2; sinh -> cosh; cosh -> sinh; log -> 1/x.
// INLINE, on the library functions themselves: the plain t_sin / t_cos / ... of lynx_maps.hpp are out-of-line on purpose
// (the forward builders' code size), but a dual-number builder makes dozens of such calls, and every call on this
// target saves and restores the caller's live registers through scratch memory -- that, not the arithmetic, was what
// k_build_bwd's parameter-gradient phase spent its time on.
LYNX_HD float dual_sin(float x) { return sinf(x); }
LYNX_HD double dual_sin(double x) { return sin(x); }
LYNX_HD float dual_cos(float x) { return cosf(x); }
LYNX_HD double dual_cos(double x) { return cos(x); }
LYNX_HD float dual_tan(float x) { return tanf(x); }
LYNX_HD double dual_tan(double x) { return tan(x); }
LYNX_HD float dual_sinh(float x) { return sinhf(x); }
LYNX_HD double dual_sinh(double x) { return sinh(x); }
LYNX_HD float dual_cosh(float x) { return coshf(x); }
LYNX_HD double dual_cosh(double x) { return cosh(x); }
LYNX_HD float dual_log(float x) { return logf(x); }
LYNX_HD double dual_log(double x) { return log(x); }
#define LYNX_DUAL_ALL(R)                                                                                                   \
  template <> LYNX_HD Dual<R> t_sqrt<Dual<R>>(Dual<R> x) { const R f = t_sqrt<R>(x.v); return Dual<R>(f, (R(0.5) / f) * x.d); } \
  template <> LYNX_HD Dual<R> t_sin<Dual<R>>(Dual<R> x) { return Dual<R>(dual_sin(x.v), dual_cos(x.v) * x.d); }             \
  template <> LYNX_HD Dual<R> t_cos<Dual<R>>(Dual<R> x) { return Dual<R>(dual_cos(x.v), -dual_sin(x.v) * x.d); }            \
  template <> LYNX_HD Dual<R> t_tan<Dual<R>>(Dual<R> x) { const R f = dual_tan(x.v); return Dual<R>(f, (R(1) + f * f) * x.d); } \
  template <> LYNX_HD Dual<R> t_sinh<Dual<R>>(Dual<R> x) { return Dual<R>(dual_sinh(x.v), dual_cosh(x.v) * x.d); }          \
  template <> LYNX_HD Dual<R> t_cosh<Dual<R>>(Dual<R> x) { return Dual<R>(dual_cosh(x.v), dual_sinh(x.v) * x.d); }          \
  template <> LYNX_HD Dual<R> t_log<Dual<R>>(Dual<R> x) { return Dual<R>(dual_log(x.v), (R(1) / x.v) * x.d); }
LYNX_DUAL_ALL(float)
LYNX_DUAL_ALL(double)
#undef LYNX_DUAL_ALL

// sum_{m >= 0} (-x)^m j! / (2m + j)!  =  1 - x / ((j+1)(j+2)) (1 - x / ((j+3)(j+4)) (1 - ...)), nested from the inside.
// With x = k2 L^2:  C = P_0(x),  S = L P_1(x),  (1 - C)/k2 = L^2 P_2(x) / 2,  (L - S)/k2 = L^3 P_3(x) / 6 -- entire
// functions of k2 whose derivatives (through the dual arithmetic, in k2 and L alike) do not cancel.  For |x| < 1 the
// first left-out term is below 1/12! (float, 6 terms) and 1/20! (double, 10 terms): under the type's epsilon.
template <typename R> LYNX_HD Dual<R> dual_series(Dual<R> x, int j) {
  constexpr int N = sizeof(R) == 4 ? 6 : 10;
  const Dual<R> one(R(1));
  Dual<R> t = one;
#pragma unroll
  for (int m = N - 1; m >= 1; --m) t = one - x * t / Dual<R>(R((j + 2 * m - 1) * (j + 2 * m)));
  return t;
}
template <typename R> LYNX_HD bool dual_series_converges(Dual<R> x) { return x.v > R(-1) && x.v < R(1); }

// cs_of (lynx_maps.hpp) for dual numbers, inline for the same reason; values as the plain builder's, derivatives from the
// series near k2 = 0 (dS/dk2 written out is (L C - S) / (2 k2))
template <typename R> LYNX_HD void cs_of(Dual<R> k2, Dual<R> L, Dual<R> s_at_zero, Dual<R>& c, Dual<R>& s) {
  if (k2.v > R(0)) {
    const Dual<R> a = t_sqrt(k2), x = a * L;
    c = t_cos(x);
    s = t_sin(x) / a;
  } else if (k2.v < R(0)) {
    const Dual<R> a = t_sqrt(-k2), x = a * L;
    c = t_cosh(x);
    s = t_sinh(x) / a;
  } else {
    c = Dual<R>(R(1));
    s = s_at_zero;
  }
  const Dual<R> x = k2 * (L * L);
  if (dual_series_converges(x)) {
    c.d = dual_series(x, 0).d;
    s.d = (L * dual_series(x, 1)).d;
  }
}

// nonzero_k1, base_dx, base_r56_bend (lynx_maps.hpp) for dual numbers: the substitution keeps the derivative part; the
// bend's (1 - cx)/kx2 and (L - sx)/kx2 are the series while it converges, value and derivative.  The values matter too:
// the edges and the tilt multiply M[0][5], M[4][1], M[4][5] into other entries, so the derivative of those entries is
// as good as these values (the plain form's (1 - cx) is 0 in float32 below |x| ~ 1e-8, where dx is hx L^2 / 2)
template <typename R> LYNX_HD Dual<R> nonzero_k1_dual(Dual<R> k1) { return k1.v == R(0) ? Dual<R>(R(1e-12), k1.d) : k1; }
template <typename R> LYNX_HD Dual<R> base_dx_dual(Dual<R> hx, Dual<R> kx2, Dual<R> L, Dual<R> cx) {
  const Dual<R> x = kx2 * (L * L);
  if (dual_series_converges(x)) return hx * (L * L) * dual_series(x, 2) / Dual<R>(R(2));
  return hx / kx2 * (Dual<R>(R(1)) - cx);
}
template <typename R> LYNX_HD Dual<R> base_r56_bend_dual(Dual<R> hx, Dual<R> kx2, Dual<R> L, Dual<R> sx, Dual<R> beta) {
  const Dual<R> x = kx2 * (L * L);
  if (dual_series_converges(x)) return hx * hx * (L * L * L) * dual_series(x, 3) / Dual<R>(R(6)) / (beta * beta);
  return hx * hx * (L - sx) / kx2 / (beta * beta);
}
// solenoid_s_k: sin(kL)/k is S of k2 = k^2; its value as the plain builder's, its derivative from the series
template <typename R> LYNX_HD Dual<R> solenoid_s_k_dual(Dual<R> s, Dual<R> k, Dual<R> L) {
  Dual<R> s_k = k.v != R(0) ? s / k : L;
  const Dual<R> kl = k * L, x = kl * kl;
  if (dual_series_converges(x)) s_k.d = (L * dual_series(x, 1)).d;
  return s_k;
}
#define LYNX_DUAL_BASE(R)                                                                                                  \
  template <> LYNX_HD Dual<R> nonzero_k1<Dual<R>>(Dual<R> k1) { return nonzero_k1_dual<R>(k1); }                            \
  template <> LYNX_HD Dual<R> base_dx<Dual<R>>(Dual<R> hx, Dual<R> kx2, Dual<R> L, Dual<R> cx) {                            \
    return base_dx_dual<R>(hx, kx2, L, cx);                                                                                  \
  }                                                                                                                          \
  template <> LYNX_HD Dual<R> base_r56_bend<Dual<R>>(Dual<R> hx, Dual<R> kx2, Dual<R> L, Dual<R> sx, Dual<R> beta) {        \
    return base_r56_bend_dual<R>(hx, kx2, L, sx, beta);                                                                      \
  }                                                                                                                          \
  template <> LYNX_HD Dual<R> solenoid_s_k<Dual<R>>(Dual<R> s, Dual<R> k, Dual<R> L) { return solenoid_s_k_dual<R>(s, k, L); }
LYNX_DUAL_BASE(float)
LYNX_DUAL_BASE(double)
#undef LYNX_DUAL_BASE

// cavity_r55_bracket (lynx_maps.hpp) without its cancellations: with a = 1/g0^2, b = 1/g1^2,
//   beta0 beta1 - 1 = ((1 - a)(1 - b) - 1) / (beta0 beta1 + 1) = -(a + b - a b) / (1 + beta0 beta1)          =: -eps
//   g0 g1 (a + b - a b) = g1/g0 + g0/g1 - 1/(g0 g1) = 2 + ((g0 - g1)^2 - 1) / (g0 g1)                          =: 2 + u
//   bracket = 1 - (2 + u) / (1 + beta0 beta1) = ((2 - eps) - (2 + u)) / (2 - eps) = -(eps + u) / (1 + beta0 beta1)
// eps and u are small and (for an energy change of more than one rest mass) of one sign.
template <typename R> LYNX_HD Dual<R> cavity_r55_bracket_dual(Dual<R> g0, Dual<R> g1, Dual<R> beta0, Dual<R> beta1) {
  const Dual<R> one(R(1));
  const Dual<R> a = one / (g0 * g0), b = one / (g1 * g1), sum = one + beta0 * beta1;
  const Dual<R> eps = (a + b - a * b) / sum, dg = g0 - g1, u = (dg * dg - one) / (g0 * g1);
  return -(eps + u) / sum;
}
template <> LYNX_HD Dual<float> cavity_r55_bracket<Dual<float>>(Dual<float> g0, Dual<float> g1, Dual<float> b0, Dual<float> b1) {
  return cavity_r55_bracket_dual<float>(g0, g1, b0, b1);
}
template <> LYNX_HD Dual<double> cavity_r55_bracket<Dual<double>>(Dual<double> g0, Dual<double> g1, Dual<double> b0, Dual<double> b1) {
  return cavity_r55_bracket_dual<double>(g0, g1, b0, b1);
}

template <> LYNX_HD Dual<float> t_fma<Dual<float>>(Dual<float> a, Dual<float> b, Dual<float> c) { return a * b + c; }
template <> LYNX_HD Dual<double> t_fma<Dual<double>>(Dual<double> a, Dual<double> b, Dual<double> c) { return a * b + c; }

}  // namespace lynx
