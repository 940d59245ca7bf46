// TEST INFRASTRUCTURE -- CPU shim of the odometry launch (isaacgymloco_amd/csrc/ls_odometry.h): the same per-env function the HIP kernel
// lsim_k_odometry_step calls, over the same lane -> env map, the lanes looped.  The entry point carries the signature of include/lsim.h
// (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_odometry.h"

extern "C" int emu_odometry_step(const lsim_odometry_t* odp, void* /*stream*/) {
    const int rv = ls_odo_validate(odp);
    if (rv != LSIM_OK) return rv;
    const lsim_odometry_t& od = *odp;
    const int slots = ls_odo_env_slots(od);
    for (int slot = 0; slot < slots; ++slot) ls_odo_env(od, slot * od.env_stride);
    return LSIM_OK;
}
