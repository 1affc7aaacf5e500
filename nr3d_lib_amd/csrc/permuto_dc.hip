// nr3d_lib_amd/csrc/permuto_dc.hip -- permutohedral-encoder kernels for input dimensions 17-32 (permuto_device.h)
#include "permuto_device.h"
NR3D_PERMUTO_GROUP(c, NR3D_PERMUTO_CASE(17) NR3D_PERMUTO_CASE(18) NR3D_PERMUTO_CASE(19) NR3D_PERMUTO_CASE(20) NR3D_PERMUTO_CASE(24)
                      NR3D_PERMUTO_CASE(28) NR3D_PERMUTO_CASE(32))
