// tile_consts.hpp -- the constants and the one rounding routine that the kernels share with the host-only headers
// (dag_plan.hpp, sky_rules.hpp, plan_abi.hpp).  No HIP header: a plain C++17 compiler reads it as it is.
#pragma once

// a routine both sides run: __host__ __device__ under hipcc, a plain function for a host compiler
#ifdef __HIPCC__
#define PSOAP_HD __host__ __device__
#else
#define PSOAP_HD
#endif

namespace psoap {

// psoap/matrix_functions.pyx:16-17 (reference tree): c_kms and c_kms**2
constexpr double C_KMS = 2.99792458e5;

constexpr int NB = 128;       // panel width == tile edge of every blocked kernel
constexpr int KB = 16;        // k-rows staged per LDS buffer in the MFMA tile loop

PSOAP_HD inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

}  // namespace psoap
