// TEST INFRASTRUCTURE -- CPU shim of the depth-memory launches (isaacgymloco_amd/csrc/ls_depth_memory.h): the validation, the plan, the tile split
// (16 envs per workgroup, hidden tiles of 16 units dealt to four waves, unit = ls_gru_unit(ht, q, r)), the freshness rule, the row arithmetic
// (ls_gru_at) and the cell's scalar math (ls_gru_cell, ls_gru_cell_bwd) are the kernels' own; a tile without a fresh env under RESETS_ONLY is
// skipped where the kernel's block returns; the sums the kernels form on MFMA tiles are plain fp32 loops here, term after term, through LDS
// images of the planned pitches.  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_depth_memory.h"
#include <vector>

static float emu_dot(const float* w, const float* x, int K) {
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc += w[k] * x[k];
    return acc;
}

extern "C" int emu_depth_memory_sizes(int32_t hidden, int32_t input_dim, size_t* a, size_t* b, size_t* c) { return ls_gru_sizes(hidden, input_dim, a, b, c); }

extern "C" int emu_depth_memory_step(const lsim_depth_memory_t* dmp, void* /*stream*/) {
    LsGruPlan p;
    const int rv = ls_dm_validate(dmp, p);
    if (rv != LSIM_OK) return rv;
    const lsim_depth_memory_t& dm = *dmp;
    const int N = dm.num_envs, L = dm.latent_dim, H = p.H, I = p.I;
    std::vector<float> lds((size_t)p.step_words);
    for (int tile = 0; tile < ls_gru_tiles(N); ++tile) {
        const int env0 = tile * LS_GRU_TILE;
        if (dm.flags & LSIM_SENSOR_RESETS_ONLY) {
            bool any = false;
            for (int e = 0; e < LS_GRU_TILE; ++e) any = any || (env0 + e < N && dm.episode_length[env0 + e] == 0);
            if (!any) continue;
        }
        for (size_t k = 0; k < lds.size(); ++k) lds[k] = -1.0e30f;          // LDS is not initialised
        float* xt = lds.data();
        float* hb = xt + LS_GRU_TILE * p.ldx;
        for (int e = 0; e < LS_GRU_TILE; ++e) {
            const int env = env0 + e;
            for (int c = 0; c < I; ++c)
                xt[e * p.ldx + c] = env < N ? (c < L ? dm.z[(size_t)env * dm.z_ld + c] : dm.p[(size_t)env * dm.p_ld + (c - L)]) : 0.0f;
            for (int j = 0; j < H; ++j)
                hb[e * p.ldh + j] = (env < N && !ls_gru_fresh(dm.flags, dm.episode_length, env)) ? dm.h[(size_t)env * dm.h_ld + j] : 0.0f;
        }
        for (int i = 0; i < LS_GRU_TILE; ++i) {
            const int env = env0 + i;
            const bool write = env < N && ls_gru_stepped(dm.flags, ls_gru_fresh(dm.flags, dm.episode_length, env));
            if (!write) continue;
            for (int wave = 0; wave < LS_GRU_WAVES; ++wave)
                for (int ht = wave; ht < p.HT; ht += LS_GRU_WAVES)
                    for (int q = 0; q < 4; ++q)
                        for (int r = 0; r < 4; ++r) {
                            const int j = ls_gru_unit(ht, q, r);
                            float pre[3], ghn = 0.0f;
                            for (int g = 0; g < 3; ++g) {
                                const float a = emu_dot(dm.weight_ih + (size_t)(g * H + j) * I, xt + i * p.ldx, I);
                                const float b = emu_dot(dm.weight_hh + (size_t)(g * H + j) * H, hb + i * p.ldh, H);
                                if (g < 2) pre[g] = (a + b) + dm.bias_ih[g * H + j] + dm.bias_hh[g * H + j];
                                else { pre[2] = a + dm.bias_ih[2 * H + j]; ghn = b + dm.bias_hh[2 * H + j]; }
                            }
                            float gr, gu, gn;
                            const float hn = ls_gru_cell(pre[0], pre[1], pre[2], ghn, hb[i * p.ldh + j], gr, gu, gn);
                            dm.h[(size_t)env * dm.h_ld + j] = hn;
                            if (dm.rows) dm.rows[(size_t)env * dm.rows_ld + L + j] = hn;
                        }
            if (dm.rows)
                for (int c = 0; c < L; ++c) dm.rows[(size_t)env * dm.rows_ld + c] = xt[i * p.ldx + c];
        }
    }
    return LSIM_OK;
}

extern "C" int emu_gru_sequence_forward(const lsim_gru_sequence_t* gsp, void* /*stream*/) {
    LsGruPlan p;
    const int rv = ls_gs_validate(gsp, false, p);
    if (rv != LSIM_OK) return rv;
    const lsim_gru_sequence_t& gs = *gsp;
    const int n = gs.num_envs, H = p.H, T = gs.steps, ld = p.ldh;
    std::vector<float> lds((size_t)p.fwd_words);
    for (int tile = 0; tile < ls_gru_tiles(n); ++tile) {
        const int env0 = tile * LS_GRU_TILE;
        for (size_t k = 0; k < lds.size(); ++k) lds[k] = -1.0e30f;
        float* W = lds.data();
        float* hb = W + 3 * H * ld;
        for (int idx = 0; idx < 3 * H * H; ++idx) W[(idx / H) * ld + idx % H] = gs.weight_hh[idx];
        for (int e = 0; e < LS_GRU_TILE; ++e)
            for (int j = 0; j < H; ++j) hb[e * ld + j] = env0 + e < n ? gs.h0[(size_t)(env0 + e) * H + j] : 0.0f;
        for (int t = 0; t < T; ++t) {
            const float* cur = hb + (t & 1) * LS_GRU_TILE * ld;
            float* nxt = hb + ((t + 1) & 1) * LS_GRU_TILE * ld;
            for (int i = 0; i < LS_GRU_TILE; ++i) {
                const int env = env0 + i, envc = env < n ? env : n - 1;
                const bool rs = gs.reset[(size_t)t * n + envc] != 0;
                std::vector<float> col((size_t)H);
                for (int k = 0; k < H; ++k) col[k] = rs ? 0.0f : cur[i * ld + k];
                for (int ht = 0; ht < p.HT; ++ht)
                    for (int q = 0; q < 4; ++q)
                        for (int r = 0; r < 4; ++r) {
                            const int j = ls_gru_unit(ht, q, r);
                            const float* gi = gs.gi + ls_gru_at(t, n, envc, 3 * H);
                            const float ar = emu_dot(W + j * ld, col.data(), H), au = emu_dot(W + (H + j) * ld, col.data(), H);
                            const float ghn = emu_dot(W + (2 * H + j) * ld, col.data(), H) + gs.bias_hh[2 * H + j];
                            float gr, gu, gn;
                            const float hn = ls_gru_cell(gi[j] + (ar + gs.bias_hh[j]), gi[H + j] + (au + gs.bias_hh[H + j]), gi[2 * H + j], ghn, col[j], gr, gu, gn);
                            nxt[i * ld + j] = hn;
                            if (env < n) {
                                gs.hs[ls_gru_at(t, n, env, H) + j] = hn;
                                if (gs.save) {
                                    float* sv = gs.save + ls_gru_at(t, n, env, 4 * H);
                                    sv[j] = gr; sv[H + j] = gu; sv[2 * H + j] = gn; sv[3 * H + j] = ghn;
                                }
                            }
                        }
            }
        }
    }
    return LSIM_OK;
}

extern "C" int emu_gru_sequence_backward(const lsim_gru_sequence_t* gsp, void* /*stream*/) {
    LsGruPlan p;
    const int rv = ls_gs_validate(gsp, true, p);
    if (rv != LSIM_OK) return rv;
    const lsim_gru_sequence_t& gs = *gsp;
    const int n = gs.num_envs, H = p.H, T = gs.steps, ld = p.ldg;
    std::vector<float> lds((size_t)p.bwd_words);
    for (int tile = 0; tile < ls_gru_tiles(n); ++tile) {
        const int env0 = tile * LS_GRU_TILE;
        for (size_t k = 0; k < lds.size(); ++k) lds[k] = -1.0e30f;
        float* WT = lds.data();
        float* db = WT + H * ld;
        for (int idx = 0; idx < 3 * H * H; ++idx) WT[(idx % H) * ld + idx / H] = gs.weight_hh[idx];
        for (int i = 0; i < LS_GRU_TILE; ++i) {
            const int env = env0 + i;
            if (env >= n) continue;                     // a column past n stores nothing, and no other column reads it
            std::vector<float> dh((size_t)H), carry((size_t)H);
            for (int j = 0; j < H; ++j) dh[j] = gs.dhs[ls_gru_at(T - 1, n, env, H) + j];
            for (int t = T - 1; t >= 0; --t) {
                float* buf = db + (t & 1) * LS_GRU_TILE * ld + i * ld;
                const bool rs = gs.reset[(size_t)t * n + env] != 0;
                const float* sv = gs.save + ls_gru_at(t, n, env, 4 * H);
                for (int j = 0; j < H; ++j) {
                    const float hp = rs ? 0.0f : (t > 0 ? gs.hs[ls_gru_at(t - 1, n, env, H) + j] : gs.h0[(size_t)env * H + j]);
                    float d[4];
                    carry[j] = ls_gru_cell_bwd(dh[j], sv[j], sv[H + j], sv[2 * H + j], sv[3 * H + j], hp, d);
                    buf[j] = d[0]; buf[H + j] = d[1]; buf[2 * H + j] = d[3];
                    float* o = gs.dgi + ls_gru_at(t, n, env, 3 * H);
                    o[j] = d[0]; o[H + j] = d[1]; o[2 * H + j] = d[2];
                    gs.dghn[ls_gru_at(t, n, env, H) + j] = d[3];
                }
                for (int k = 0; k < H; ++k) {
                    const float v = rs ? 0.0f : carry[k] + emu_dot(WT + k * ld, buf, 3 * H);
                    if (t > 0) dh[k] = v + gs.dhs[ls_gru_at(t - 1, n, env, H) + k];
                    else if (gs.dh0) gs.dh0[(size_t)env * H + k] = v;
                }
            }
        }
    }
    return LSIM_OK;
}
