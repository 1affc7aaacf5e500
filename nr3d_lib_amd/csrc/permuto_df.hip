// nr3d_lib_amd/csrc/permuto_df.hip -- permutohedral-encoder kernels for input dimension 56 (permuto_device.h; the high dimensions
// compile longest -- O(D^2) unrolled rank selects -- so each has a file of its own and the build runs them in parallel)
#include "permuto_device.h"
NR3D_PERMUTO_GROUP(f, NR3D_PERMUTO_CASE(56))
