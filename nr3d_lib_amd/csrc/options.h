// nr3d_lib_amd/csrc/options.h -- the library's run-time options, ONE table.
//
// The selectable code paths that the parity tests A/B against each other are entries of `g_val[]`, set through the C ABI
// (`nr3d_set_option`, include/nr3d_hip.h) -- a launch reads a plain int, never the environment.  There is nothing else: the
// library has no build-time variants.
#pragma once
#include <stdint.h>
#include <atomic>
#include "../../include/nr3d_hip.h"

namespace nr3d {
namespace opt {

// process-wide on purpose (autograd launches from its own thread), relaxed atomics: a concurrent set / launch is not a data race
// (include/nr3d_hip.h: test / measurement only)
extern std::atomic<int64_t> g_val[NR3D_OPT_COUNT];            // host_api.hip (defaults there)

static inline int64_t get(int id) { return g_val[id].load(std::memory_order_relaxed); }
static inline bool on(int id) { return get(id) != 0; }

}  // namespace opt
}  // namespace nr3d
