// Unit of libivs.so: the row-pass surface kernels and their launcher.
#include <hip/hip_runtime.h>

#include "ivs_surface_pass_launch.hpp"
