// TEST INFRASTRUCTURE -- CPU shim of the entry point of isaacgymloco_amd/csrc/ls_distill.h: the same validation, the same choice between the
// two paths and the same per-lane function the HIP kernel calls, the workgroups, waves and lanes looped and the sums met in the launch's
// order (the butterfly over 64 lanes, then the waves in ascending order).  The entry point carries the signature of include/lsim.h (the
// stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_distill.h"

template <bool VEC>
static void emu_dl_workgroups(const lsim_distill_loss_t& dl) {
    for (int p = 0; p < LSIM_DISTILL_PARTIALS; ++p) {
        float part[LS_DL_WAVES];
        for (int w = 0; w < LS_DL_WAVES; ++w) {
            float acc[64], next[64];
            for (int l = 0; l < 64; ++l) acc[l] = ls_dl_lane<VEC>(dl, p, 64 * w + l);
            for (int m = 32; m >= 1; m >>= 1) {
                for (int l = 0; l < 64; ++l) next[l] = acc[l] + acc[l ^ m];
                for (int l = 0; l < 64; ++l) acc[l] = next[l];
            }
            part[w] = acc[0];
        }
        float sum = part[0];
        for (int w = 1; w < LS_DL_WAVES; ++w) sum = sum + part[w];
        dl.partial[p] = sum;
    }
}

extern "C" int emu_distill_loss(const lsim_distill_loss_t* dlp, void* /*stream*/) {
    const int rv = ls_dl_validate(dlp);
    if (rv != LSIM_OK) return rv;
    if (ls_dl_vector(*dlp)) emu_dl_workgroups<true>(*dlp);
    else emu_dl_workgroups<false>(*dlp);
    return LSIM_OK;
}

// which path a call with these arguments takes (1: the 128-bit one), for the tests to assert that both are exercised
extern "C" int emu_distill_loss_path(const lsim_distill_loss_t* dlp) { return dlp && ls_dl_vector(*dlp) ? 1 : 0; }
