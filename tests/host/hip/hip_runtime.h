// Stand-in for <hip/hip_runtime.h> when csrc/pcr_solve6.h and csrc/pcr_umeyama.h are compiled for the host alone (tests/test_pose_solvers_host.py):
// the function qualifiers vanish, the math functions are those of <cmath>.
#pragma once
#include <cmath>
#define __host__
#define __device__
using std::isfinite;
