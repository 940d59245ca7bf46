// TEST INFRASTRUCTURE -- CPU shim of the map-rows launch (isaacgymloco_amd/csrc/ls_odometry.h): the same per-element function the HIP kernel
// lsim_k_map_rows calls, over the same flattened index, the lanes looped.  The entry point carries the signature of include/lsim.h (the
// stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_odometry.h"

extern "C" int emu_map_rows(const lsim_map_rows_t* mrp, void* /*stream*/) {
    const int rv = ls_mr_validate(mrp);
    if (rv != LSIM_OK) return rv;
    const long long elements = ls_mr_elements(*mrp);
    for (long long i = 0; i < elements; ++i) ls_mr_element(*mrp, i);
    return LSIM_OK;
}
