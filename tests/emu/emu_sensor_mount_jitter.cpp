// TEST INFRASTRUCTURE -- CPU shim of the mount-jitter launch (isaacgymloco_amd/csrc/ls_sensor_mount_jitter.h): the same per-env functions the
// HIP kernel lsim_k_sensor_mount_jitter calls, over the same lane -> env map, the lanes looped.  The entry point carries the signature of
// include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_sensor_mount_jitter.h"

extern "C" int emu_sensor_mount_jitter(const lsim_sensor_mount_jitter_t* mjp, void* /*stream*/) {
    const int rv = ls_smj_validate(mjp);
    if (rv != LSIM_OK) return rv;
    const lsim_sensor_mount_jitter_t& mj = *mjp;
    const int slots = ls_smj_env_slots(mj);
    for (int slot = 0; slot < slots; ++slot) {
        const int env = slot * mj.env_stride;
        if (ls_smj_fresh(mj, env)) ls_smj_env(mj, env);
    }
    return LSIM_OK;
}
