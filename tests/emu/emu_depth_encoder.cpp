// TEST INFRASTRUCTURE -- CPU shim of the depth-encoder launch (isaacgymloco_amd/csrc/ls_depth_encoder.h): the validation, the plan, the due rule
// (ls_sensor_due) and the index arithmetic (ls_de_slot, ls_de_tap, ls_de_base, the tap tables, ls_de_elu) are the kernel's own; a block of an
// env that is not due is skipped where the kernel's block returns; the sums the kernel forms on MFMA tiles and wave butterflies are plain
// fp32 loops here, tap after tap.  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_depth_encoder.h"
#include <vector>

static void emu_de_conv(const float* in, float* out, const int* tap, const float* w, const float* b, int K, int cout, int P, int wout, int s, int win) {
    for (int c = 0; c < cout; ++c)
        for (int pos = 0; pos < P; ++pos) {
            const int base = ls_de_base(pos, wout, s, win);
            float acc = 0.0f;
            for (int kk = 0; kk < K; ++kk) acc += w[(size_t)c * K + kk] * in[tap[kk] + base];
            out[c * P + pos] = ls_de_elu(acc + b[c]);
        }
}

extern "C" int emu_depth_encode_sizes(const lsim_depth_encoder_t* de, size_t* lds_bytes) { return ls_de_sizes(de, lds_bytes); }

extern "C" int emu_depth_encode(const lsim_depth_encoder_t* dep, void* /*stream*/) {
    LsDePlan p;
    const int rv = ls_de_validate(dep, p);
    if (rv != LSIM_OK) return rv;
    const lsim_depth_encoder_t& de = *dep;
    const uint32_t tick_mod = ls_de_tick_mod(de);
    const int slots = ls_de_env_slots(de);
    std::vector<float> lds((size_t)p.words);
    for (int b = 0; b < slots; ++b) {
        const int env = b * de.env_stride;
        if (env >= de.num_envs) continue;
        bool fill;
        if (!ls_sensor_due(de.flags, de.episode_length, de.period, de.stagger, env, tick_mod, fill)) continue;
        for (size_t k = 0; k < lds.size(); ++k) lds[k] = -1.0e30f;          // LDS is not initialised
        float* X = lds.data();
        float* A1 = X + p.oA1;
        int* T1 = (int*)(X + p.oT1);
        int* T2 = (int*)(X + p.oT2);
        const int R = de.height * de.width;
        for (int f = 0; f < de.frames; ++f)
            for (int r = 0; r < R; ++r) X[f * R + r] = de.hist[ls_de_slot(de, env, f) + (size_t)r];
        for (int kk = 0; kk < p.K1; ++kk) T1[kk] = ls_de_tap(kk, de.k1, de.height, de.width);
        for (int kk = 0; kk < p.K2; ++kk) T2[kk] = ls_de_tap(kk, de.k2, p.h1, p.w1);
        emu_de_conv(X, A1, T1, de.w1, de.b1, p.K1, de.c1, p.h1 * p.w1, p.w1, de.s1, de.width);
        emu_de_conv(A1, X, T2, de.w2, de.b2, p.K2, de.c2, p.h2 * p.w2, p.w2, de.s2, p.w1);
        float* row = de.latent + (size_t)env * (size_t)de.latent_stride;
        for (int o = 0; o < de.latent_dim; ++o) {
            float acc = 0.0f;
            for (int j = 0; j < p.K3; ++j) acc += de.w3[(size_t)o * p.K3 + j] * X[j];
            const float z = acc + de.b3[o];
            row[o] = de.final_act ? ls_de_elu(z) : z;
        }
    }
    return LSIM_OK;
}
