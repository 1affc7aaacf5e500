// nr3d_lib_amd/csrc/permuto_da.hip -- permutohedral-encoder kernels for input dimensions 2-8 (permuto_device.h; the reference splits
// its instantiations the same way, csrc/permuto/src/compile_split_*.cu)
#include "permuto_device.h"
NR3D_PERMUTO_GROUP(a, NR3D_PERMUTO_CASE(2) NR3D_PERMUTO_CASE(3) NR3D_PERMUTO_CASE(4) NR3D_PERMUTO_CASE(5) NR3D_PERMUTO_CASE(6)
                      NR3D_PERMUTO_CASE(7) NR3D_PERMUTO_CASE(8))
