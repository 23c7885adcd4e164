// rrt_blackbody.cpp -- the host's share of the blackbody disk (RRT_DISK_BLACKBODY):
// the constants the device rule takes from the host, and rrt_blackbody_tint.  Plain C++ (no GPU code),
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
