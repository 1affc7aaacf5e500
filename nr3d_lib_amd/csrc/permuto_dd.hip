// nr3d_lib_amd/csrc/permuto_dd.hip -- permutohedral-encoder kernels for input dimensions 36 and 40 (permuto_device.h)
#include "permuto_device.h"
NR3D_PERMUTO_GROUP(d, NR3D_PERMUTO_CASE(36) NR3D_PERMUTO_CASE(40))
