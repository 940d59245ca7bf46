// TEST INFRASTRUCTURE -- CPU shim of the two entry points of isaacgymloco_amd/csrc/ls_frames_log.h: the same validation and the same per-env,
// per-row and per-column functions the HIP kernels call, the blocks and lanes looped.  The entry points carry the signatures of
// include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_frames_log.h"

extern "C" int emu_sensor_frames_log(const lsim_frames_log_t* flp, void* /*stream*/) {
    const int rv = ls_fl_validate(flp);
    if (rv != LSIM_OK) return rv;
    const lsim_frames_log_t& fl = *flp;
    const uint32_t tick_mod = ls_fl_tick_mod(fl);
    // launch 1: the ranks in ascending env order, which is what the blocks' counts add up to
    const int before = ls_fl_count_before(fl);
    long long logged = 0;
    for (int env = 0; env < fl.num_envs; ++env) {
        const int kind = ls_fl_kind(fl, env, tick_mod);
        ls_fl_assign(fl, env, kind, (long long)before + logged);
        if (kind == 2) ++logged;
    }
    ls_fl_finish_rank(fl, before, logged);
    // launch 2
    int lo, hi;
    ls_fl_copy_range(fl, lo, hi);
    const int groups = fl.row_stride >> 2;
    for (int row = lo; row < hi; ++row) {
        const int env = ls_fl_row_env(fl, row);
        if (env < 0) continue;
        for (int f = 0; f < fl.frames; ++f)
            for (int q = 0; q < groups; ++q) ls_fl_copy_group(fl, row, env, f, q);
    }
    fl.state[LSIM_FRAMES_LOG_COUNT] = fl.state[LSIM_FRAMES_LOG_NEXT];
    return LSIM_OK;
}

extern "C" int emu_latent_rows_grad(const lsim_latent_rows_grad_t* lgp, void* /*stream*/) {
    const int rv = ls_lg_validate(lgp);
    if (rv != LSIM_OK) return rv;
    const lsim_latent_rows_grad_t& lg = *lgp;
    for (int r = 0; r < lg.rows; ++r) {
        int t0 = 0, env = 0;
        const bool have = ls_lg_source(lg, r, t0, env);
        for (int j = 0; j < lg.latent_dim; ++j) lg.G[(size_t)r * (size_t)lg.G_stride + (size_t)j] = have ? ls_lg_column(lg, r, t0, env, j) : 0.0f;
    }
    return LSIM_OK;
}
