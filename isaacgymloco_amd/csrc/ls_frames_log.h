// ls_frames_log.h -- the two launches that carry a PPO gradient into the depth encoder (include/lsim.h): lsim_sensor_frames_log, a
// de-duplicated log of the images a rollout's captures produced, written behind the capture, and lsim_latent_rows_grad, the gradients of a
// minibatch's latent rows summed per logged image.  lsim.h states every rule; this file is that text in code.
//
// Self-contained like ls_depth_encoder.h (lsim.h, ls_sensor_model.h for the due rule, the C library): tests/emu/emu_frames_log.cpp compiles
// this file with g++ under LS_EMU and runs the same validation, per-env decision, row arithmetic, copy and sum over plain arrays.
//
// lsim_sensor_frames_log is TWO launches on the caller's stream.
//   1. lsim_k_frames_log_rank: one lane per env, blocks of LS_FL_BLOCK = 256.  A lane decides with ls_sensor_due whether its env is logged.
//      The rank of a logged env is the number of logged envs with a smaller index: block b counts those of the envs below its own first one
//      itself (its lanes stride over them, one 8-byte load each, then one sum over the block), and ranks its own 256 by ballot and popcount.
//      Block b therefore reads b * 256 episode lengths that other blocks read too -- N^2 / 512 loads in all, 32 K at N = 4096, from L2 --
//      and in exchange no block waits for another and no counter is shared: the row of an env is a function of the inputs alone.  The lane
//      then writes its env's entry of row_of[step] and, for a row below capacity, row_src[row].  The last block, which has counted every
//      logged env, writes the launch's range of rows and the overflow to `state`.  Nobody writes state[COUNT] here: every block reads it.
//   2. lsim_k_frames_log_copy: the rows [state[BASE], state[NEXT]) are the images to copy, and row_src says whose they are.  The blocks
//      grid-stride over them -- the grid is what the host can know, every visited env under FILL_ALL and one env in `period` otherwise, so
//      no block starts to find that its env is not due -- 256 lanes moving 16 bytes each per access, both sides
//      coalesced; the words between `pixels` and `row_stride` are written as 0.  Block 0 then publishes state[COUNT] = state[NEXT]: it is
//      the only writer of that word and no block of this launch reads it.
//
// lsim_latent_rows_grad is one launch: one wave per row r, four rows per block.  The wave walks t = t0, t0 + 1, ... while row_of[t][e] == r
// -- two dword loads per step that every lane makes alike, so they are broadcasts -- and its lanes own the columns j = lane, lane + 64, ...:
// each adds g[mb_of[t * N + e]][j] to its own fp32 sum in ascending t, so the order of every sum is the rule's and two calls agree bit for
// bit.  Rows of g are read coalesced, G is written coalesced, nothing is shared between lanes.
#pragma once
#include "ls_sensor_model.h"

#define LS_FL_BLOCK 256
#define LS_FL_MAX_COPY_BLOCKS 2048      // the copy's grid is capped here and strides over the rest

// ------------------------------------------------------------------------------------------------ frame log
// what the rank launch decides for env e: 0 not visited, 1 visited and not logged, 2 logged
LS_RC_FN int ls_fl_kind(const lsim_frames_log_t& fl, int env, uint32_t tick_mod) {
    if (env % fl.env_stride != 0) return 0;
    bool fill;
    return ls_sensor_due(fl.flags, fl.episode_length, fl.period, fl.stagger, env, tick_mod, fill) ? 2 : 1;
}
// rows in the log before this launch; a word outside 0 .. capacity (a state nobody zeroed) is read as the nearer end, so no row leaves the arrays
LS_RC_FN int ls_fl_count_before(const lsim_frames_log_t& fl) {
    if (fl.flags & LSIM_SENSOR_FILL_ALL) return 0;
    const int32_t c = fl.state[LSIM_FRAMES_LOG_COUNT];
    return c < 0 ? 0 : (c > fl.capacity ? fl.capacity : c);
}

// env e's entry of row_of[step], given its kind and (for a logged env) its row = count_before + rank
LS_RC_FN void ls_fl_assign(const lsim_frames_log_t& fl, int env, int kind, long long row) {
    int32_t* now = fl.row_of + (size_t)fl.step * (size_t)fl.num_envs;
    if (kind == 0) {
        now[env] = -1;
    } else if (kind == 2) {
        if (row < (long long)fl.capacity) {
            now[env] = (int32_t)row;
            fl.row_src[row] = fl.step * fl.num_envs + env;          // < num_steps * num_envs <= 2^31 - 1 (ls_fl_validate)
        } else {
            now[env] = -1;
        }
    } else if (!(fl.flags & LSIM_SENSOR_RESETS_ONLY)) {
        now[env] = (now - fl.num_envs)[env];                        // step >= 1: a launch with step 0 is FILL_ALL and logs every visited env
    }
}
// what the launch leaves in `state`, from the number of logged envs
LS_RC_FN void ls_fl_finish_rank(const lsim_frames_log_t& fl, int before, long long logged) {
    const long long room = (long long)fl.capacity - (long long)before;      // >= 0: count never exceeds capacity
    const long long written = logged < room ? logged : room;
    fl.state[LSIM_FRAMES_LOG_BASE] = before;
    fl.state[LSIM_FRAMES_LOG_NEXT] = before + (int32_t)written;
    fl.state[LSIM_FRAMES_LOG_OVERFLOW] = fl.state[LSIM_FRAMES_LOG_OVERFLOW] + (int32_t)(logged - written);      // never reset here: the caller's
}
// the range of rows the copy moves, clamped to what the arrays hold whatever `state` says
LS_RC_FN void ls_fl_copy_range(const lsim_frames_log_t& fl, int& lo, int& hi) {
    lo = fl.state[LSIM_FRAMES_LOG_BASE];
    hi = fl.state[LSIM_FRAMES_LOG_NEXT];
    if (lo < 0) lo = 0;
    if (hi > fl.capacity) hi = fl.capacity;
}
// the env whose image row `row` takes, or -1 when row_src does not name an env of this step (nothing is copied then)
LS_RC_FN int ls_fl_row_env(const lsim_frames_log_t& fl, int row) {
    const long long e = (long long)fl.row_src[row] - (long long)fl.step * (long long)fl.num_envs;
    return e >= 0 && e < (long long)fl.num_envs ? (int)e : -1;
}
// 16-byte group q (of row_stride / 4) of frame f of `env`'s image into row `row`
LS_RC_FN void ls_fl_copy_group(const lsim_frames_log_t& fl, int row, int env, int f, int q) {
    const float* src = fl.hist + ((size_t)env * (size_t)fl.hist_slots + (size_t)f) * (size_t)fl.hist_stride + (size_t)4 * (size_t)q;
    float* dst = fl.log + ((size_t)row * (size_t)fl.frames + (size_t)f) * (size_t)fl.row_stride + (size_t)4 * (size_t)q;
    const int left = fl.pixels - 4 * q;         // pixels of this group that exist
#if defined(__HIPCC__) && !defined(LS_EMU)
    if (left >= 4) {                            // hist and log are 16-byte aligned and both strides multiples of 4
        *(float4*)dst = *(const float4*)src;
        return;
    }
    *(float4*)dst = make_float4(left > 0 ? src[0] : 0.0f, left > 1 ? src[1] : 0.0f, left > 2 ? src[2] : 0.0f, 0.0f);
#else
    for (int k = 0; k < 4; ++k) dst[k] = k < left ? src[k] : 0.0f;
#endif
}

static inline int ls_fl_validate(const lsim_frames_log_t* fl) {
    if (!fl) return LSIM_E_INVALID;
    if (!ls_rc_aligned(fl->hist, 16) || !ls_rc_aligned(fl->log, 16) || !ls_rc_aligned(fl->episode_length, 8)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(fl->row_of, 4) || !ls_rc_aligned(fl->row_src, 4) || !ls_rc_aligned(fl->state, 4)) return LSIM_E_INVALID;
    if (fl->num_envs < 1 || fl->env_stride < 1) return LSIM_E_INVALID;
    if (fl->frames < 1 || fl->pixels < 1 || fl->hist_slots > LSIM_SENSOR_MAX_HISTORY || fl->frames > fl->hist_slots) return LSIM_E_INVALID;
    if (fl->pixels > fl->hist_stride || (fl->hist_stride & 3) != 0) return LSIM_E_INVALID;
    if (fl->row_stride < fl->pixels || (fl->row_stride & 3) != 0) return LSIM_E_INVALID;
    if (fl->num_steps < 1 || fl->step < 0 || fl->step >= fl->num_steps || fl->capacity < 1) return LSIM_E_INVALID;
    if ((long long)fl->num_steps * (long long)fl->num_envs > 0x7FFFFFFFLL) return LSIM_E_INVALID;
    if (fl->tick < 0 || fl->period < 1 || fl->stagger < 0 || fl->stagger > 1) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(fl->flags)) return LSIM_E_INVALID;
    if (fl->step == 0 && !(fl->flags & LSIM_SENSOR_FILL_ALL)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline uint32_t ls_fl_tick_mod(const lsim_frames_log_t& fl) { return ls_sensor_tick_mod(fl.tick, fl.period); }
// blocks of the copy: the envs the host knows to be logged -- every visited one under FILL_ALL, one in `period` otherwise -- capped
static inline unsigned ls_fl_copy_blocks(const lsim_frames_log_t& fl) {
    const long long slots = ls_sensor_env_slots(fl.num_envs, fl.env_stride);
    long long blocks = (fl.flags & LSIM_SENSOR_FILL_ALL) ? slots : (slots + fl.period - 1) / fl.period;
    if (blocks > (long long)fl.capacity) blocks = fl.capacity;
    if (blocks > LS_FL_MAX_COPY_BLOCKS) blocks = LS_FL_MAX_COPY_BLOCKS;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// ------------------------------------------------------------------------------------------------ gradient rows
// (t0, e) of row r, or false when row_src[r] names no transition (the row is written as zeros)
LS_RC_FN bool ls_lg_source(const lsim_latent_rows_grad_t& lg, int r, int& t0, int& env) {
    const int32_t s = lg.row_src[r];
    if (s < 0 || (long long)s >= (long long)lg.num_steps * (long long)lg.num_envs) return false;
    t0 = s / lg.num_envs;
    env = s - t0 * lg.num_envs;
    return true;
}
// column j of G[r]: the sum over the transitions that read row r, in ascending t
LS_RC_FN float ls_lg_column(const lsim_latent_rows_grad_t& lg, int r, int t0, int env, int j) {
    float acc = 0.0f;
    for (int t = t0; t < lg.num_steps; ++t) {
        const size_t at = (size_t)t * (size_t)lg.num_envs + (size_t)env;
        if (lg.row_of[at] != r) break;
        const int32_t m = lg.mb_of[at];
        if (m >= 0 && m < lg.batch) acc = acc + lg.g[(size_t)m * (size_t)lg.g_stride + (size_t)j];
    }
    return acc;
}
static inline int ls_lg_validate(const lsim_latent_rows_grad_t* lg) {
    if (!lg) return LSIM_E_INVALID;
    if (!ls_rc_aligned(lg->g, 4) || !ls_rc_aligned(lg->G, 4)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(lg->mb_of, 4) || !ls_rc_aligned(lg->row_of, 4) || !ls_rc_aligned(lg->row_src, 4)) return LSIM_E_INVALID;
    if (lg->batch < 1 || lg->rows < 0 || lg->latent_dim < 1 || lg->g_stride < lg->latent_dim || lg->G_stride < lg->latent_dim) return LSIM_E_INVALID;
    if (lg->num_steps < 1 || lg->num_envs < 1 || (long long)lg->num_steps * (long long)lg->num_envs > 0x7FFFFFFFLL) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_FL_BLOCK) void lsim_k_frames_log_rank(const lsim_frames_log_t fl, uint32_t tick_mod) {
    __shared__ int part[LS_FL_BLOCK / 64];
    __shared__ int own[LS_FL_BLOCK / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = (int)blockIdx.x * LS_FL_BLOCK;             // < num_envs by the grid
    // the logged envs below this block's first one
    int mine = 0;
    for (int e = tid; e < first; e += LS_FL_BLOCK) mine += ls_fl_kind(fl, e, tick_mod) == 2 ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    // this block's own envs
    const int env = first + tid;
    const int kind = env < fl.num_envs ? ls_fl_kind(fl, env, tick_mod) : 0;
    const unsigned long long logged = __ballot(kind == 2);
    if (lane == 0) {
        part[wave] = mine;
        own[wave] = __popcll(logged);
    }
    __syncthreads();
    long long below = 0;
    int block_total = 0;
#pragma unroll
    for (int w = 0; w < LS_FL_BLOCK / 64; ++w) {
        below += part[w];
        if (w < wave) below += own[w];
        block_total += own[w];
    }
    const int before = ls_fl_count_before(fl);
    if (env < fl.num_envs) {
        const long long rank = below + (long long)__popcll(logged & ((1ull << lane) - 1ull));
        ls_fl_assign(fl, env, kind, (long long)before + rank);
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        long long all = block_total;
#pragma unroll
        for (int w = 0; w < LS_FL_BLOCK / 64; ++w) all += part[w];
        ls_fl_finish_rank(fl, before, all);
    }
}

__global__ __launch_bounds__(LS_FL_BLOCK) void lsim_k_frames_log_copy(const lsim_frames_log_t fl) {
    int lo, hi;
    ls_fl_copy_range(fl, lo, hi);
    const int groups = fl.row_stride >> 2, per_image = fl.frames * groups;
    for (long long at = (long long)lo + (long long)blockIdx.x; at < (long long)hi; at += (long long)gridDim.x) {
        const int row = (int)at, env = ls_fl_row_env(fl, row);
        if (env < 0) continue;                  // the whole block: row is the block's
        for (int i = (int)threadIdx.x; i < per_image; i += LS_FL_BLOCK) {
            const int f = i / groups;
            ls_fl_copy_group(fl, row, env, f, i - f * groups);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) fl.state[LSIM_FRAMES_LOG_COUNT] = fl.state[LSIM_FRAMES_LOG_NEXT];
}

extern "C" int lsim_sensor_frames_log(const lsim_frames_log_t* fl, void* stream) {
    const int rv = ls_fl_validate(fl);
    if (rv != LSIM_OK) return rv;
    const unsigned blocks = (unsigned)(((long long)fl->num_envs + LS_FL_BLOCK - 1) / LS_FL_BLOCK);
    hipLaunchKernelGGL(lsim_k_frames_log_rank, dim3(blocks), dim3(LS_FL_BLOCK), 0, (hipStream_t)stream, *fl, ls_fl_tick_mod(*fl));
    if (hipGetLastError() != hipSuccess) return LSIM_E_HIP;
    hipLaunchKernelGGL(lsim_k_frames_log_copy, dim3(ls_fl_copy_blocks(*fl)), dim3(LS_FL_BLOCK), 0, (hipStream_t)stream, *fl);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}

__global__ __launch_bounds__(LS_FL_BLOCK) void lsim_k_latent_rows_grad(const lsim_latent_rows_grad_t lg) {
    const int lane = (int)threadIdx.x & 63;
    const long long r64 = (long long)blockIdx.x * (LS_FL_BLOCK / 64) + ((long long)threadIdx.x >> 6);
    if (r64 >= (long long)lg.rows) return;      // the whole wave: r is the wave's
    const int r = (int)r64;
    int t0 = 0, env = 0;
    const bool have = ls_lg_source(lg, r, t0, env);
    float* out = lg.G + (size_t)r * (size_t)lg.G_stride;
    for (int j = lane; j < lg.latent_dim; j += 64) out[j] = have ? ls_lg_column(lg, r, t0, env, j) : 0.0f;
}

extern "C" int lsim_latent_rows_grad(const lsim_latent_rows_grad_t* lg, void* stream) {
    const int rv = ls_lg_validate(lg);
    if (rv != LSIM_OK) return rv;
    if (lg->rows == 0) return LSIM_OK;
    const unsigned blocks = (unsigned)(((long long)lg->rows + LS_FL_BLOCK / 64 - 1) / (LS_FL_BLOCK / 64));
    hipLaunchKernelGGL(lsim_k_latent_rows_grad, dim3(blocks), dim3(LS_FL_BLOCK), 0, (hipStream_t)stream, *lg);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
