// rrt_blackbody.h -- the constants of the blackbody disk (RRT_DISK_BLACKBODY), shared by
// the kernels (rrt_device.h disk_rgb), the host runtime (rrt_host.cpp fill_disk_params) and the host's
// own arithmetic (rrt_blackbody.cpp, plain C++: rrt_glibm.h's functions are host functions there).
#pragma once

#define RRT_BB_HC_K 14387768.77             // hc / k in nm K
#define RRT_BB_LAMBDA_R 610.0               // the channels' wavelengths in nm
#define RRT_BB_LAMBDA_G 550.0
#define RRT_BB_LAMBDA_B 465.0
#define RRT_BB_F_NORM (823543.0 / 46656.0)  // 1 / max of c^3 (1 - sqrt c), reached at c = 36 / 49
#define RRT_BB_T_MIN 1000.0                 // the temperatures rrt_set_disk and rrt_blackbody_tint take
#define RRT_BB_T_MAX 1e6

// K_c = RRT_BB_HC_K / lambda_c (one division) and N_c = rrt_glibm_exp(K_c / temperature) - 1, the
// function the device evaluates (rrt_glibm.h), not the C library's
void rrt_bb_constants(double temperature, double k[3], double n[3]);

// The constants of the Page-Thorne profile (RRT_DISK_PROFILE_PAGE_THORNE) for spin
// s = a / M and x0 = sqrt(r_in / M) as the device forms it: ca = 1.5 s, a2 = 2 s, the roots x[3] of
// x^3 - 3 x + 2 s, d[i] = x0 - x[i], the coefficients c[3] (not finite: 0) and norm = 1 / S(x_peak), the
// peak found by the fixed 200-round ternary search from [x0, 2 x0].  acos, cos and log are
// rrt_glibm.h's; S is evaluated in the device's operation order.
#define RRT_PT_ROUNDS 200
void rrt_pt_constants(double s, double x0, double* ca, double* a2, double x[3], double d[3], double c[3], double* norm);
