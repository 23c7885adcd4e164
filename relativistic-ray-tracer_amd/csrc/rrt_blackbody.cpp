// rrt_blackbody.cpp -- the host's share of the blackbody disk (RRT_DISK_BLACKBODY):
// the constants the device rule takes from the host (§15: the Page-Thorne profile's too), and
// rrt_blackbody_tint.  Plain C++ (no GPU code),
// so rrt_glibm.h's restatement of exp compiles as a host function here: host and device evaluate the
// same function on the same quotient, which is what makes ratio == 1 at T_obs == temperature.
#include <cmath>

#include "../../include/rrt.h"
#include "rrt_blackbody.h"
#include "rrt_glibm.h"

static const double LAMBDA[3] = {RRT_BB_LAMBDA_R, RRT_BB_LAMBDA_G, RRT_BB_LAMBDA_B};

void rrt_bb_constants(double temperature, double k[3], double n[3]) {
  for (int c = 0; c < 3; ++c) {
    k[c] = RRT_BB_HC_K / LAMBDA[c];
    n[c] = rrt_glibm_exp(k[c] / temperature) - 1.0;
  }
}

// The Page-Thorne profile.  S(x) without the norm, in the order of rrt_device.h
// disk_rgb<true, true>: the host finds the peak of the function the device evaluates.
static double pt_shape(double xx, double x0, double ca, double a2, const double x[3], const double d[3], const double c[3]) {
  double B = (xx - x0) - ca * rrt_glibm_log(xx / x0);
  for (int i = 0; i < 3; ++i) B = B - c[i] * rrt_glibm_log((xx - x[i]) / d[i]);
  const double x2 = xx * xx;
  const double den = (x2 * x2) * (((x2 * xx) - 3.0 * xx) + a2);
  return B / den;
}

void rrt_pt_constants(double s, double x0, double* ca, double* a2, double x[3], double d[3], double c[3], double* norm) {
  *ca = 1.5 * s;
  *a2 = 2.0 * s;
  const double t = rrt_glibm_acos(s) / 3.0;
  const double p3 = 3.14159265358979323 / 3.0;
  x[0] = 2.0 * rrt_glibm_cos(t - p3);
  x[1] = 2.0 * rrt_glibm_cos(t + p3);
  x[2] = -(2.0 * rrt_glibm_cos(t));
  for (int i = 0; i < 3; ++i) {
    const double xi = x[i], xj = x[(i + 1) % 3], xk = x[(i + 2) % 3];
    const double e = xi - s;
    d[i] = x0 - xi;
    c[i] = (3.0 * (e * e)) / (xi * ((xi - xj) * (xi - xk)));
    if (!std::isfinite(c[i])) c[i] = 0.0;
  }
  double lo = x0, hi = 2.0 * x0;
  for (int k = 0; k < RRT_PT_ROUNDS; ++k) {
    const double m1 = lo + (hi - lo) / 3.0;
    const double m2 = hi - (hi - lo) / 3.0;
    if (pt_shape(m1, x0, *ca, *a2, x, d, c) < pt_shape(m2, x0, *ca, *a2, x, d, c)) lo = m1; else hi = m2;
  }
  const double xp = 0.5 * (lo + hi);
  *norm = 1.0 / pt_shape(xp, x0, *ca, *a2, x, d, c);
}

// The three-wavelength Planck colour of T normalised to G = 1: B_lambda(T) is proportional to
// lambda^-5 / (exp(K / T) - 1), so rgb[c] = W_c (exp(K_G / T) - 1) / (exp(K_c / T) - 1) with
// W_c = (550 / lambda_c)^5; G is (1 x n_G) / n_G = 1 exactly.
extern "C" int rrt_blackbody_tint(double T, float rgb[3]) {
  if (!rgb || !(std::isfinite(T) && T >= RRT_BB_T_MIN && T <= RRT_BB_T_MAX)) return RRT_E_INVALID;
  double k[3], n[3];
  rrt_bb_constants(T, k, n);
  for (int c = 0; c < 3; ++c) {
    const double p = RRT_BB_LAMBDA_G / LAMBDA[c];
    const double w = ((p * p) * (p * p)) * p;
    rgb[c] = (float)((w * n[1]) / n[c]);
  }
  return RRT_OK;
}
