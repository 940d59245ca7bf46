// TEST INFRASTRUCTURE -- CPU shim of the stereo-artefact launch (isaacgymloco_amd/csrc/ls_sensor_stereo.h): the same per-lane functions the HIP
// kernel lsim_k_sensor_stereo calls, over the same block -> env map, the lanes looped, each __syncthreads() a loop boundary and the LDS a
// plain array.  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_sensor_stereo.h"
#include <string.h>

extern "C" int emu_sensor_stereo_sizes(int32_t width, int32_t height, size_t* lds_bytes) { return ls_st_sizes(width, height, lds_bytes); }

extern "C" int emu_sensor_stereo(const lsim_sensor_stereo_t* stp, void* /*stream*/) {
    const int rv = ls_st_validate(stp);
    if (rv != LSIM_OK) return rv;
    const lsim_sensor_stereo_t& st = *stp;
    const uint32_t tick_mod = ls_st_tick_mod(st);
    static uint32_t lds[LSIM_STEREO_MAX_LDS_BYTES / 4];
    for (int slot = 0; slot < ls_st_env_slots(st); ++slot) {
        const int env = slot * st.env_stride;
        bool fill;
        if (!ls_sensor_due(st.flags, st.episode_length, st.period, st.stagger, env, tick_mod, fill)) continue;
        memset(lds, 0xA5, sizeof lds);          // LDS is not initialised
        const LsStLds l = ls_st_carve(lds, st.width * st.height);
        const float fbe = ls_st_fbe(st, env);
        for (int lane = 0; lane < 2; ++lane) l.cnt[lane] = 0u;
        for (int lane = 0; lane < LS_ST_BLOCK; ++lane) ls_st_stage(st, env, lane, fbe, l);
        for (int lane = 0; lane < LS_ST_BLOCK; ++lane) ls_st_decide(st, env, lane, l);
        for (int lane = 0; lane < LS_ST_BLOCK; ++lane) ls_st_store(st, env, lane, ls_st_first_slot(st, env, fill), l);
        for (int lane = 0; lane < 2; ++lane)
            if (l.cnt[lane] != 0u) ls_rc_count((long long*)st.state + lane, (long long)l.cnt[lane]);
    }
    return LSIM_OK;
}
