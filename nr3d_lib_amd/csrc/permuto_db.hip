// nr3d_lib_amd/csrc/permuto_db.hip -- permutohedral-encoder kernels for input dimensions 9-16 (permuto_device.h)
#include "permuto_device.h"
NR3D_PERMUTO_GROUP(b, NR3D_PERMUTO_CASE(9) NR3D_PERMUTO_CASE(10) NR3D_PERMUTO_CASE(11) NR3D_PERMUTO_CASE(12) NR3D_PERMUTO_CASE(13)
                      NR3D_PERMUTO_CASE(14) NR3D_PERMUTO_CASE(15) NR3D_PERMUTO_CASE(16))
