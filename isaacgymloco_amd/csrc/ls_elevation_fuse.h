// ls_elevation_fuse.h -- the elevation map with a variance per cell (include/lsim.h, lsim_elevation_map_fused) and the map rows with a
// confidence block (lsim_map_rows_fused).  lsim.h states every formula; this file is that text in code.
//
// It stands on ls_elevation_map.h and restates nothing of it: the pose, the fill, the cell / slot / key helpers, the point of a ray
// (ls_em_point, behind both passes here), the window's cell of a slot (ls_em_window_cell), the scan's lookup (ls_em_lookup) and the
// argument check are that file's own functions, so a change to how a depth sample becomes a map point, or to how a scan point finds its cell,
// is made in that file alone (where the point's text stands twice, side by side: ls_em_insert says why).  What is here is what the variance
// adds: the two passes around the point, the fusion, and the variance next to the scan.  Compared against the commit that still had a text per launch:
// profiles/elevation_refactor_ab.json.  It stands on ls_odometry.h for the first block of the rows.
// tests/emu/emu_elevation_fuse.cpp compiles this file with g++ under LS_EMU and runs the same per-lane functions, the lanes looped and the LDS
// arrays plain arrays.
//
// Shape of the launch (lsim_k_elevation_map_fused): lsim_k_elevation_map's -- ONE workgroup of 256 lanes per visited env -- with
// 3 * G * G * 4 bytes of dynamic LDS (3, 12 or 48 KB): the keys, an int32 sum and an int32 count per slot.
//   0. the pose and ls_sensor_due;   1. fill: the stamps to -1;
//   2. due: the three LDS arrays to 0, barrier; pass 1 over the rays (r = lane, lane + 256, ...), each kept point one ds_max_u32
//      on its slot's key; barrier; pass 2 over the same rays, the point formed again by ls_em_point (nothing is cached: 16 K rays would need
//      scratch), each point within the band one ds_add_u32 on the slot's sum and one on its count; barrier; the lanes sweep the slots, and a
//      touched one reads its three words and var, fuses, and writes four dwords;
//   3. barrier; lane j < P looks its scan point up with ls_em_lookup, as lsim_k_elevation_map does, and reads var too: one more load and one more store.
// Only 32-bit integer LDS atomics, no float atomic: integer sums do not depend on the order of the rays.  Every branch around a barrier is on
// values the whole workgroup shares (env, fill, due, the pose).
#pragma once
#include "ls_elevation_map.h"
#include "ls_odometry.h"

#if defined(LS_EMU) || !defined(__HIPCC__)
LS_RC_FN void ls_ef_add(int32_t* p, int32_t v) { *p += v; }
#else
LS_RC_FN void ls_ef_add(int32_t* p, int32_t v) { (void)atomicAdd(p, v); }
#endif

LS_RC_FN void ls_ef_lds_clear(const lsim_elevation_map_t& em, uint32_t* keys, int32_t* sum, int32_t* cnt, int lane) {
    const int G2 = em.size * em.size;
    for (int s = lane; s < G2; s += LS_EM_BLOCK) { keys[s] = 0u; sum[s] = 0; cnt[s] = 0; }
}

// pass 1: this lane's rays into the keys.  Both passes form the point with ls_em_point, so pass 2 never meets a slot or a height that pass 1
// did not: ls_em_insert's own text (ls_elevation_map.h says why it has one) is kept out of this kernel
LS_RC_FN void ls_ef_pass_max(const lsim_elevation_map_t& em, const LsEmPose& s, int env, int lane, float rinv, uint32_t* keys) {
    const float* row = em.depth + (size_t)env * (size_t)em.depth_stride;
    const uint8_t* lab = em.labels ? em.labels + (size_t)env * (size_t)em.label_stride : (const uint8_t*)0;
    for (int r = lane; r < em.num_rays; r += LS_EM_BLOCK) {
        int slot; float z;
        if (ls_em_point(em, s, row, lab, r, rinv, slot, z)) ls_em_max(keys + slot, ls_em_key(z));
    }
}

// pass 2: the same rays again, each point formed by ls_em_point as pass 1 formed it; a point within `band` of its
// slot's maximum joins the slot's sum and count
LS_RC_FN void ls_ef_pass_sum(const lsim_elevation_map_fused_t& ef, const LsEmPose& s, int env, int lane, float rinv, const uint32_t* keys, int32_t* sum, int32_t* cnt) {
    const lsim_elevation_map_t& em = ef.em;
    const float* row = em.depth + (size_t)env * (size_t)em.depth_stride;
    const uint8_t* lab = em.labels ? em.labels + (size_t)env * (size_t)em.label_stride : (const uint8_t*)0;
    for (int r = lane; r < em.num_rays; r += LS_EM_BLOCK) {
        int slot; float z;
        if (!ls_em_point(em, s, row, lab, r, rinv, slot, z)) continue;
        const float df = ls_em_unkey(keys[slot]) - z;
        if (!(df <= ef.band)) continue;
        ls_ef_add(sum + slot, (int32_t)(df * 65536.0f + 0.5f));
        ls_ef_add(cnt + slot, 1);
    }
}

LS_RC_FN float ls_ef_age(int64_t tick, int32_t stamp) { return (float)(((uint32_t)tick - (uint32_t)stamp) & 0x7FFFFFFFu); }

// the touched slots: the measurement, then the fusion with what the slot held
LS_RC_FN void ls_ef_commit(const lsim_elevation_map_fused_t& ef, const LsEmPose& s, int env, int lane, const uint32_t* keys, const int32_t* sum, const int32_t* cnt) {
    const lsim_elevation_map_t& em = ef.em;
    const int G = em.size, G2 = G * G;
    const size_t base = (size_t)env * (size_t)G2;
    for (int k = lane; k < G2; k += LS_EM_BLOCK) {
        const uint32_t key = keys[k];
        if (key == 0u) continue;
        int ix, iy;
        ls_em_window_cell(s, G, k, ix, iy);
        const uint32_t word = ls_em_pack(ix, iy);
        const float zmax = ls_em_unkey(key);
        const int32_t n = cnt[k];
        // n >= 1 whenever both passes form the same z for the same ray, which the same code on the same inputs does; n == 0 reads as a sum of 0
        const float mean = n > 0 ? ls_div_exact((float)sum[k], (float)n) : 0.0f;
        const float zm = zmax - mean * 1.52587890625e-05f;
        const float ex = ((float)ix + 0.5f) * em.res - s.px, ey = ((float)iy + 0.5f) * em.res - s.py;
        const float rho2 = ex * ex + ey * ey;
        const float sigma = ef.sigma0 + ef.sigma2 * (rho2 + ef.range_z2);
        const int32_t nc = n < ef.count_cap ? (n > 0 ? n : 1) : ef.count_cap;
        const float vm = ls_div_exact(sigma * sigma, (float)nc) + ef.var_floor;
        const int32_t stamp = em.stamp[base + (size_t)k];
        float h = zm, var = vm;
        if (stamp >= 0 && em.cell[base + (size_t)k] == word) {
            const float h0 = em.height[base + (size_t)k];
            const float vp = ef.var[base + (size_t)k] + ef.var_growth * ls_ef_age(em.tick, stamp);
            const float d = zm - h0, S = vp + vm;
            if (ls_rc_finite(S) && d * d < ef.gate2 * S) {
                const float K = ls_div_exact(vp, S);
                h = h0 + K * d;
                var = K * vm;
            }
        }
        var = fminf(fmaxf(var, ef.var_floor), ef.var_max);
        em.height[base + (size_t)k] = h;
        ef.var[base + (size_t)k] = var;
        em.stamp[base + (size_t)k] = (int32_t)(em.tick & 0x7FFFFFFF);
        em.cell[base + (size_t)k] = word;
    }
}

// this lane's scan points: ls_em_scan with the aged variance next to the height
LS_RC_FN void ls_ef_scan(const lsim_elevation_map_fused_t& ef, const LsEmPose& s, int env, int lane, float rinv) {
    const lsim_elevation_map_t& em = ef.em;
    const size_t base = (size_t)env * (size_t)(em.size * em.size);
    float* scan = em.scan + (size_t)env * (size_t)em.scan_stride;
    float* svar = ef.scan_var + (size_t)env * (size_t)ef.var_stride;
    uint8_t* known = em.known + (size_t)env * (size_t)em.known_stride;
    for (int j = lane; j < em.num_points; j += LS_EM_BLOCK) {
        if (!s.ok) {
            scan[j] = 0.0f;
            svar[j] = ef.var_max;
            known[j] = (uint8_t)0;
            continue;
        }
        int32_t stamp;
        const int k = ls_em_lookup(em, s, j, base, rinv, stamp);
        float h = s.pz - em.unknown_drop, v = ef.var_max;
        uint8_t kn = (uint8_t)0;
        if (k >= 0) {
            kn = (uint8_t)1;
            h = em.height[base + (size_t)k];
            v = fminf(ef.var[base + (size_t)k] + ef.var_growth * ls_ef_age(em.tick, stamp), ef.var_max);       // fminf: a NaN operand yields the other
        }
        scan[j] = h;
        svar[j] = v;
        known[j] = kn;
    }
}

// ---- host side: the argument check shared by the library and the CPU shim (no launch happens before it passes)
static inline int ls_ef_validate(const lsim_elevation_map_fused_t* ef) {
    if (!ef) return LSIM_E_INVALID;
    const int rv = ls_em_validate(&ef->em);
    if (rv != LSIM_OK) return rv;
    if (!ls_rc_aligned(ef->var, 4) || !ls_rc_aligned(ef->scan_var, 4) || ef->var_stride < ef->em.num_points) return LSIM_E_INVALID;
    const float v[8] = {ef->sigma0, ef->sigma2, ef->range_z2, ef->band, ef->var_floor, ef->var_growth, ef->var_max, ef->gate2};
    for (int k = 0; k < 8; ++k) if (!ls_rc_host_finite(v[k]) || !(v[k] >= 0.0f)) return LSIM_E_INVALID;
    if (ef->band > 0.5f || ef->var_floor > ef->var_max || ef->count_cap < 1) return LSIM_E_INVALID;
    return LSIM_OK;
}

// ------------------------------------------------------------------------------------------------ map rows with a confidence
LS_RC_FN void ls_mf_element(const lsim_map_rows_fused_t& mf, long long i) {
    const lsim_map_rows_t& mr = mf.mr;
    const int P = mr.num_points, cols = mr.channels * P;
    const int slot = (int)(i / (long long)cols), col = (int)(i - (long long)slot * (long long)cols);
    if (col < P) { ls_mr_element(mr, i); return; }
    const size_t env = (size_t)slot * (size_t)mr.env_stride;          // < num_envs: slot <= (num_envs - 1) / env_stride
    const float sv = mf.scan_var[env * (size_t)mf.var_stride + (size_t)(col - P)];
    const bool kn = mr.known[env * (size_t)mr.known_stride + (size_t)(col - P)] != (uint8_t)0;
    mr.rows[env * (size_t)mr.ld + (size_t)col] = (kn && ls_rc_finite(sv) && sv >= 0.0f) ? ls_div_exact(mf.var_ref, mf.var_ref + sv) : 0.0f;
}

static inline int ls_mf_validate(const lsim_map_rows_fused_t* mf) {
    if (!mf) return LSIM_E_INVALID;
    const int rv = ls_mr_validate(&mf->mr);
    if (rv != LSIM_OK) return rv;
    if (!ls_rc_host_finite(mf->var_ref) || !(mf->var_ref > 0.0f)) return LSIM_E_INVALID;
    if (mf->mr.channels == 2 && (!ls_rc_aligned(mf->scan_var, 4) || mf->var_stride < mf->mr.num_points)) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
// What only the commit and the scan read, loaded from the argument block WHERE THEY RUN.  The compiler loads a by-value argument at the
// kernel's entry and keeps all 256 bytes in scalar registers through the ray loops; beside the pose that is more than the file holds, and
// it parked 17 of them in lanes of a vector register.  `ef` is the kernel's first argument, so it lies at the start of the argument block
// (the HSA kernarg segment: explicit arguments in order from offset 0); the empty asm hides where the pointer comes from, so these loads
// can neither be merged with the entry's nor moved ahead of it.  Fields the ray passes read are not copied: they come from `ef` itself.
LS_RC_FN lsim_elevation_map_fused_t ls_ef_late_fields() {
    uintptr_t p = (uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    const __attribute__((address_space(4))) lsim_elevation_map_fused_t* a = (const __attribute__((address_space(4))) lsim_elevation_map_fused_t*)p;
    lsim_elevation_map_fused_t l;
    l.em.pts = a->em.pts; l.em.height = a->em.height; l.em.stamp = a->em.stamp; l.em.cell = a->em.cell; l.em.scan = a->em.scan; l.em.known = a->em.known;
    l.em.tick = a->em.tick; l.em.num_points = a->em.num_points; l.em.scan_stride = a->em.scan_stride; l.em.known_stride = a->em.known_stride;
    l.em.size = a->em.size; l.em.res = a->em.res; l.em.unknown_drop = a->em.unknown_drop;
    l.var = a->var; l.scan_var = a->scan_var; l.sigma0 = a->sigma0; l.sigma2 = a->sigma2; l.range_z2 = a->range_z2; l.band = a->band;
    l.var_floor = a->var_floor; l.var_growth = a->var_growth; l.var_max = a->var_max; l.gate2 = a->gate2; l.count_cap = a->count_cap;
    l.var_stride = a->var_stride;
    return l;
}

__global__ __launch_bounds__(LS_EM_BLOCK) void lsim_k_elevation_map_fused(const lsim_elevation_map_fused_t ef, uint32_t tick_mod, float rinv) {
    extern __shared__ uint32_t ls_ef_lds[];
    const lsim_elevation_map_t& em = ef.em;
    const int G2 = em.size * em.size;
    uint32_t* keys = ls_ef_lds;
    int32_t* sum = (int32_t*)(ls_ef_lds + G2);
    int32_t* cnt = (int32_t*)(ls_ef_lds + 2 * G2);
    const int env = (int)blockIdx.x * em.env_stride, lane = (int)threadIdx.x;      // < num_envs: blockIdx.x <= (num_envs - 1) / env_stride
    bool fill;
    const bool due = ls_sensor_due(em.flags, em.episode_length, em.period, em.stagger, env, tick_mod, fill);
    const LsEmPose s = ls_em_pose(em, env, rinv);
    if (fill) ls_em_clear(em, env, lane);
    if (due && s.ok) {
        ls_ef_lds_clear(em, keys, sum, cnt, lane);
        __syncthreads();
        ls_ef_pass_max(em, s, env, lane, rinv, keys);
        __syncthreads();
        ls_ef_pass_sum(ef, s, env, lane, rinv, keys, sum, cnt);
        __syncthreads();
        ls_ef_commit(ls_ef_late_fields(), s, env, lane, keys, sum, cnt);
    }
    __syncthreads();
    if (!s.ok && lane == 0) ls_rc_count((long long*)em.state, 1);
    ls_ef_scan(ls_ef_late_fields(), s, env, lane, rinv);
}

extern "C" int lsim_elevation_map_fused(const lsim_elevation_map_fused_t* ef, void* stream) {
    const int rv = ls_ef_validate(ef);
    if (rv != LSIM_OK) return rv;
    const size_t lds = (size_t)3 * (size_t)ef->em.size * (size_t)ef->em.size * sizeof(uint32_t);      // at most 48 KB
    hipLaunchKernelGGL(lsim_k_elevation_map_fused, dim3((unsigned)ls_em_env_slots(ef->em)), dim3(LS_EM_BLOCK), lds, (hipStream_t)stream, *ef,
                       ls_em_tick_mod(ef->em), ls_em_rinv(ef->em));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}

__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_map_rows_fused(const lsim_map_rows_fused_t mf, long long elements) {
    const long long i = (long long)blockIdx.x * LS_RC_BLOCK + (long long)threadIdx.x;
    if (i >= elements) return;
    ls_mf_element(mf, i);
}

extern "C" int lsim_map_rows_fused(const lsim_map_rows_fused_t* mf, void* stream) {
    const int rv = ls_mf_validate(mf);
    if (rv != LSIM_OK) return rv;
    const long long elements = ls_mr_elements(mf->mr);
    const long long blocks = (elements + LS_RC_BLOCK - 1) / LS_RC_BLOCK;
    if (blocks > 0x7FFFFFFFLL) return LSIM_E_INVALID;       // more than a grid holds: only above 10^9 envs
    hipLaunchKernelGGL(lsim_k_map_rows_fused, dim3((unsigned)blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *mf, elements);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
