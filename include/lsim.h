/*
 * lsim.h -- C-ABI of the MI355X-native vectorised legged-robot simulator ("leggedsim").
 *
 * Drop-in boundary for the hot path of xyyandhtl/IsaacgymLoco: everything that
 * LeggedRobot.step() (legged_gym/envs/base/legged_robot.py:122-176) does between
 * receiving `actions` and returning the observation tuple, i.e. the Isaac Gym tensor
 * API calls listed in SURVEY.md 2.3 plus the torch post-physics stack.
 *
 * The reference has no FFI of its own on this path (it calls the closed-source
 * `isaacgym.gymapi` pybind module); each entry point below names the reference
 * call(s) it replaces.  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative LSIM_E_* code; the text of the
 *     last error of a handle is available from lsim_last_error().  No exceptions cross
 *     the ABI.  One caller thread per handle.
 *   - all device work is enqueued on the caller-supplied HIP stream (pass
 *     torch.cuda.current_stream().cuda_stream); no call synchronises the host unless
 *     documented.
 *   - device memory: the caller may pass one pre-allocated arena (lsim_query_arena gives
 *     the size) so that a PyTorch host can alias every buffer zero-copy the way the
 *     reference aliases simulator state with gymtorch.wrap_tensor (LR:930-944); with
 *     arena == NULL the library allocates (hipMalloc) and owns it.
 *   - quaternions are xyzw; root/body velocities are world-frame (LR:929-941).
 */
#ifndef LSIM_H
#define LSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSIM_ABI_VERSION 7   /* 2: LSIM_BUF_CONTACT_COUNT, fixed-point words in LSIM_BUF_STATS (round 2); 3: LSIM_BUF_SUBSTEP_TORQUES (round 3);
                                 4: lsim_config.solver_type / num_position_iterations out of the reserved words (round 4);
                                 5: lsim_config.lin_vel_at_com (centre-of-mass linear velocities, the PhysX convention) and tgs_limit_passes, lsim_get / set_reset_calls (round 5);
                                 6: LSIM_BUF_NONFINITE + LSIM_STATS_NONFINITE (robots whose simulated state is not finite), lsim_amp_step and the discriminator-update kernels (round 6);
                                 7: lsim_eval + lsim_eval_sizes / lsim_eval_clear / lsim_eval_accumulate (device-side policy evaluation: grouped metrics and state traces); no earlier struct or entry changed;
                                    also under 7, as pure additions (no earlier struct or entry changed, so a caller built against the first
                                    version-7 header runs unchanged): lsim_raycast + lsim_raycast_sizes (range sensors: rays against the terrain mesh);
                                    lsim_raycast_bodies + lsim_raycast_bodies_sizes (the same sensors also see the env's own robot);
                                    lsim_sensor_capture + LSIM_RNG_SENSOR (the sensor model: update period, latency, frame history, noise);
                                    lsim_depth_encode + lsim_depth_encode_sizes (a small CNN over a sensor's frame history, forward only);
                                    lsim_depth_encode_backward + lsim_depth_encode_backward_sizes (the gradients of that CNN's parameters);
                                    lsim_eval_columns + lsim_eval_columns_sizes / _clear / _accumulate (caller-supplied columns into the evaluator's groups);
                                    lsim_depth_memory_step + lsim_depth_memory_sizes, lsim_gru_sequence_forward / _backward (a GRU cell over the depth latent);
                                    lsim_sensor_mount_jitter + LSIM_RNG_SENSOR_MOUNT (a sensor's mount pose redrawn per episode, on the device);
                                    lsim_sensor_instrument + lsim_sensor_capture_inst + LSIM_RNG_SENSOR_INSTRUMENT (a sensor's latency, noise level,
                                    depth-scale error and field of view redrawn per episode, and the capture that reads them);
                                    lsim_elevation_map (a robot-centred height grid per env, fused from a sensor's depth rows and the robot's pose);
                                    lsim_odometry_step + LSIM_RNG_ODOMETRY (an estimated base pose that drifts with the distance travelled) and
                                    lsim_map_rows (the map's scan as the rows an actor reads, one launch);
                                    lsim_sensor_frames_log (the images a rollout's captures produced, logged once each, behind the capture) and
                                    lsim_latent_rows_grad (a minibatch's latent gradients summed per logged image);
                                    lsim_distill_loss (a minibatch's action means against a teacher's, gathered through the shuffle's permutation);
                                    lsim_elevation_map_fused (the elevation map with a banded mean per capture and a variance per cell, fused over the
                                    captures by a scalar Kalman filter) and lsim_map_rows_fused (the map's rows with a confidence block);
                                    lsim_sensor_stereo + lsim_sensor_stereo_sizes + LSIM_RNG_SENSOR_STEREO (a stereo camera's occlusion shadows, minimum
                                    range and depth-edge artefacts, written into the frame history behind a capture);
                                    lsim_sensor_shade + lsim_sensor_shade_sizes (a shaded colour frame behind lsim_raycast_bodies: the surface normal at
                                    every hit, whether the sun reaches it, a colour per pixel);
                                    lsim_elevation_map_cleanup (cells of the elevation map that a capture's rays pass over, well below the height
                                    the map holds, are forgotten: one launch between the capture and the map's) */

/* ---- fixed sizes of the robot family on this path (12-DoF quadrupeds) ---- */
#define LSIM_NUM_DOF 12
#define LSIM_NUM_BODIES 17      /* base + 4 x (hip, thigh, calf, foot); LR:1143 */
#define LSIM_NUM_LEGS 4
#define LSIM_NUM_ACTIONS 12
#define LSIM_ONE_STEP_OBS 45    /* LRC:51 */
#define LSIM_OBS_HISTORY 6      /* LRC:52 */
#define LSIM_NUM_OBS 270
#define LSIM_MAX_HEIGHT_PTS_X 32
#define LSIM_MAX_HEIGHT_PTS_Y 32
#define LSIM_NUM_HEIGHT_PTS 187 /* 17 x 11, AGC:79-80; the obs layout hard-codes 187 (LR:895) */
#define LSIM_NUM_PRIV_OBS 238   /* 45 + 3 + 3 + 187, LRC:53 */
#define LSIM_NUM_AMP_OBS 30     /* LR:416 */
#define LSIM_NUM_BASE_HEIGHT_PTS 63 /* 7 x 9, LR:1308-1312 */
#ifndef LSIM_MAX_COLLISION_POINTS /* the CPU oracle can be compiled with a larger table: densely sampled TRUE collision shapes (tests/test_shape_variants.py) */
#define LSIM_MAX_COLLISION_POINTS 64
#endif
#ifndef LSIM_MAX_CONTACTS      /* the CPU oracle can be compiled with a larger cap to measure what the cap costs (tests/test_contact_cap.py) */
#define LSIM_MAX_CONTACTS 8
#endif
#define LSIM_MAX_POSITION_ITERATIONS 12   /* solver_type 1: sub-iterations per sim_dt (the reference sets 4, LRC:246) */
#define LSIM_MAX_ROBOTS 4                 /* robot descriptions of one lsim_create_mixed instance */
#define LSIM_SOLVER_PGS 0
#define LSIM_SOLVER_TGS 1
#define LSIM_TERRAIN_LEVELS_MAX 32
#define LSIM_TERRAIN_TYPES_MAX 32

/* error codes */
#define LSIM_OK 0
#define LSIM_E_INVALID (-1)
#define LSIM_E_NOMEM (-2)
#define LSIM_E_HIP (-3)
#define LSIM_E_UNSUPPORTED (-4)
#define LSIM_E_ABI (-5)

/* ---- reward terms: every `_reward_<name>` defined in LR:1444-1770, in the
 * alphabetical order in which the reference evaluates and accumulates them
 * (class_to_dict iterates dir(), HLP:49 -> LR:1050-1055 -> LR:369-373). ---- */
enum lsim_reward_id {
    LSIM_R_ACTION_RATE = 0,
    LSIM_R_ANG_VEL_XY,
    LSIM_R_ANG_VEL_XY_UP,
    LSIM_R_BASE_HEIGHT,
    LSIM_R_BASE_HEIGHT_UP,
    LSIM_R_CALF_POSE,
    LSIM_R_CALF_POSE_UP,
    LSIM_R_COLLISION,
    LSIM_R_COLLISION_UP,
    LSIM_R_DOF_ACC,
    LSIM_R_DOF_POS_DIF,
    LSIM_R_DOF_POS_LIMITS,
    LSIM_R_DOF_VEL,
    LSIM_R_DOF_VEL_LIMITS,
    LSIM_R_FEET_AIR_TIME,
    LSIM_R_FEET_CONTACT_FORCES,
    LSIM_R_FEET_MIRROR,
    LSIM_R_FEET_MIRROR_UP,
    LSIM_R_FEET_SLIDE,
    LSIM_R_FEET_SLIDE_UP,
    LSIM_R_FEET_STUMBLE,
    LSIM_R_FEET_STUMBLE_UP,
    LSIM_R_FOOT_CLEARANCE_BASE,
    LSIM_R_FOOT_CLEARANCE_BASE_UP,
    LSIM_R_FOOT_CLEARANCE_TERRAIN,
    LSIM_R_FOOT_CLEARANCE_TERRAIN_UP,
    LSIM_R_HAS_CONTACT,
    LSIM_R_HIP_ACTION_MAGNITUDE,
    LSIM_R_HIP_POS,
    LSIM_R_HIP_POS_UP,
    LSIM_R_JOINT_POWER,
    LSIM_R_LIN_VEL_Z,
    LSIM_R_LIN_VEL_Z_UP,
    LSIM_R_ORIENTATION,
    LSIM_R_ORIENTATION_UP,
    LSIM_R_POWER,
    LSIM_R_POWER_DISTRIBUTION,
    LSIM_R_SMOOTHNESS,
    LSIM_R_STAND_NICE,
    LSIM_R_STAND_STILL,
    LSIM_R_STUCK,
    LSIM_R_TERMINATION,
    LSIM_R_THIGH_POSE,
    LSIM_R_THIGH_POSE_UP,
    LSIM_R_TORQUE_LIMITS,
    LSIM_R_TORQUES,
    LSIM_R_TORQUES_DIF,
    LSIM_R_TORQUES_DISTRIBUTION,
    LSIM_R_TRACKING_ANG_VEL,
    LSIM_R_TRACKING_LIN_VEL,
    LSIM_R_UPWARD,
    LSIM_NUM_REWARD_TERMS
};

/* ---- counter-based RNG draw sites (Philox4x32-10, key = (seed, rank)) ----
 * counter = (env, common_step_counter, tag, idx >> 2), lane = idx & 3,
 * u = (x >> 8) * 2^-24 in [0,1).  One tag per torch draw site of the reference
 * (stream order listed in SURVEY.md 8a quirk 12). */
enum lsim_rng_tag {
    LSIM_RNG_DELAY = 1,        /* LR:134            idx 0                                  */
    LSIM_RNG_CMD = 2,          /* LR:641-651        idx 0 vx, 1 vy, 2 heading|yaw, 3 vx_hi */
    LSIM_RNG_PUSH = 3,         /* LR:827            idx 0..1                               */
    LSIM_RNG_DISTURB = 4,      /* LR:842            idx 0..2                               */
    LSIM_RNG_TERM_NOISE = 5,   /* LR:451, LR:457    idx 0..44 obs, 45..231 heights         */
    LSIM_RNG_RESET_LEVEL = 6,  /* LR:864            idx 0                                  */
    LSIM_RNG_RESET_DOF = 7,    /* LR:699, LR:709    idx 0..11 pos ratio, 12..23 vel        */
    LSIM_RNG_RESET_ROOT = 8,   /* LR:730-812        idx 0..2 xyz, 3..5 rpy, 6..11 vel      */
    LSIM_RNG_RESET_CMD = 9,    /* LR:320 -> 641-651 same idx as LSIM_RNG_CMD               */
    LSIM_RNG_RESET_DR = 10,    /* LR:337-341, 535   idx 0 kp, 1 kd, 2 motor factor, 3 friction, 4 restitution */
    LSIM_RNG_OBS_NOISE = 11,   /* LR:394, LR:400    idx 0..44 obs, 45..231 heights         */
    LSIM_RNG_INIT = 12,        /* LR:999-1028, 1232 idx 0..11 motor_strength, 12 kp, 13 kd, 14 motor factor,
                                  15 payload, 16..18 com, 19 friction bucket id, 20 terrain level;
                                  step word = 0xFFFFFFFF                                    */
    LSIM_RNG_INIT_BUCKET = 13, /* LR:511            env word = bucket index, idx 0         */
    LSIM_RNG_POLICY = 14,      /* HIMP:94 (actor_critic.act sample), lsim_rollout_act: step word = draw counter,
                                  block p gives the two Box-Muller pairs of actions 2p, 2p+1       */
    LSIM_RNG_SENSOR = 15,      /* lsim_sensor_capture (no reference site): step word = (uint32) tick, the fourth counter word =
                                  (stream_id << 16) | ray -- one whole block per ray, all four words used      */
    LSIM_RNG_SENSOR_MOUNT = 16, /* lsim_sensor_mount_jitter (no reference site): step word = (uint32) tick, the fourth counter word =
                                  (stream_id << 16) | b, b = 0, 1 -- block 0: position x y z and rotation x, block 1: rotation y z, two words unused */
    LSIM_RNG_SENSOR_INSTRUMENT = 17, /* lsim_sensor_instrument (no reference site): step word = (uint32) tick, the fourth counter word =
                                  (stream_id << 16) | b, b = 0, 1 -- block 0: latency, noise gain, depth scale, depth quad, block 1: tan scale, three words unused */
    LSIM_RNG_ODOMETRY = 18,    /* lsim_odometry_step (no reference site): step word = (uint32) tick, the fourth counter word =
                                  (stream_id << 16) | b, b = 0, 1 -- block 0: the step's yaw, position and height noise, one word unused,
                                  block 1: the episode's scale, yaw and height bias, one word unused */
    LSIM_RNG_SENSOR_STEREO = 19 /* lsim_sensor_stereo (no reference site): step word = (uint32) tick, the fourth counter word =
                                  (stream_id << 16) | pixel -- one block per pixel, the first word used */
};

/* ---- robot model: the URDF after Isaac Gym's fixed-joint collapse ----
 * body order: 0 base, then for leg l in (FL, FR, RL, RR): 1+4l hip, 2+4l thigh, 3+4l calf, 4+4l foot.
 * dof order : 3l + (0 hip, 1 thigh, 2 calf)  (LR:1145). */
typedef struct lsim_body {
    float mass;
    float com[3];        /* in the body (link) frame */
    float inertia[6];    /* about the com, body axes: xx, xy, xz, yy, yz, zz */
    float joint_pos[3];  /* origin of this body's frame in the parent frame (rpy is 0 for all joints) */
    float joint_axis[3]; /* revolute axis (unit), zero vector for base / fixed feet */
    int32_t parent;      /* -1 for base */
    int32_t dof;         /* -1 for base and for the fixed foot */
} lsim_body;

typedef struct lsim_collision_point {
    float pos[3];   /* sphere centre in the body frame */
    float radius;   /* 0 for box corners */
    int32_t body;   /* body index the contact force is reported on */
    int32_t pad;
} lsim_collision_point;

typedef struct lsim_robot_model {
    lsim_body bodies[LSIM_NUM_BODIES];
    float dof_pos_lower[LSIM_NUM_DOF];  /* hard URDF limits (rad) */
    float dof_pos_upper[LSIM_NUM_DOF];
    float dof_vel_limit[LSIM_NUM_DOF];
    float dof_effort_limit[LSIM_NUM_DOF];
    int32_t num_collision_points;       /* ordered by priority: overflow beyond LSIM_MAX_CONTACTS is dropped from the end */
    int32_t pad;
    lsim_collision_point points[LSIM_MAX_COLLISION_POINTS];
    int32_t feet_bodies[LSIM_NUM_LEGS];   /* LR:1209-1211 */
    uint32_t penalised_body_mask;         /* LR:1213-1215 */
    uint32_t termination_body_mask;       /* LR:1217-1219 */
} lsim_robot_model;

/* ---- flat configuration: the values of the reference's nested config classes that the
 * path reads (LeggedRobotCfg LRC:48 and the Aliengo subclasses AGC/AGS/AGA). ---- */
typedef struct lsim_config {
    int32_t abi_version;      /* LSIM_ABI_VERSION */
    int32_t num_envs;         /* LRC:50 */
    uint32_t seed;            /* LRC:258 */
    uint32_t rank;            /* second Philox key word: one stream per data-parallel rank */

    /* control (LRC:117-127, AGC:94-100) */
    float sim_dt;             /* 0.005, LRC:239; > 0 (a divisor in the 'V' law), else LSIM_E_INVALID */
    int32_t decimation;       /* 4 */
    int32_t control_type;     /* 0 'P', 1 'V', 2 'T' (LR:676-687); anything else: LSIM_E_INVALID (the reference raises, LR:687) */
    float action_scale;
    float hip_reduction;
    float p_gains[LSIM_NUM_DOF];
    float d_gains[LSIM_NUM_DOF];
    float torque_limits[LSIM_NUM_DOF];   /* LR:571 */
    float default_dof_pos[LSIM_NUM_DOF]; /* LR:980-996 */
    float clip_actions;       /* LRC:216 */
    float clip_observations;

    /* domain randomisation (AGC:148-214) */
    int32_t delay;
    int32_t randomize_kp;  float kp_range[2];
    int32_t randomize_kd;  float kd_range[2];
    int32_t randomize_motor_strength; float motor_strength_range[2];
    int32_t randomize_friction; float friction_range[2];
    int32_t randomize_restitution; float restitution_range[2];
    int32_t randomize_payload_mass; float payload_mass_range[2];
    int32_t randomize_com_displacement; float com_displacement_range[2];
    int32_t push_robots; int32_t push_interval; float max_push_vel_xy;        /* LR:627, LR:1263; interval > 0 when push_robots, else LSIM_E_INVALID */
    int32_t disturbance; int32_t disturbance_interval; float disturbance_range[2]; /* LR:631; interval > 0 when disturbance, else LSIM_E_INVALID */

    /* reset (LR:690-820) */
    int32_t has_dof_init_pos_ratio; float dof_init_pos_ratio_range[2];
    int32_t randomize_dof_vel; float dof_init_vel_range[2];  /* effective range read at LR:708 */
    int32_t has_base_init_pos_range; float base_init_pos_range[3][2];
    int32_t has_base_init_rot_range; float base_init_rot_range[3][2];
    float base_init_vel_range[6][2];
    float base_init_state[13];      /* LR:1160-1161 */

    /* commands (AGC:102-115) */
    float command_ranges[4][2];     /* lin_vel_x, lin_vel_y, ang_vel_yaw, heading */
    int32_t heading_command;
    int32_t resampling_steps;       /* int(resampling_time / dt), LR:612 */
    int32_t commands_curriculum;
    float max_forward_curriculum, max_backward_curriculum, max_lat_curriculum;

    /* terrain (AGC:67-91) */
    int32_t mesh_type;              /* 0 plane, 1 heightfield, 2 trimesh; anything else: LSIM_E_INVALID.  Plane: LSIM_BUF_ENV_ORIGINS starts at zero,
                                       the grid of robots (LR:1243-1250) is left to the host (the product binding keeps every robot at the origin) */
    float horizontal_scale, vertical_scale, border_size;
    int32_t grid_rows, grid_cols;   /* tot_rows, tot_cols, TER:59-60 */
    int32_t terrain_num_rows, terrain_num_cols;  /* levels, types */
    float terrain_length, terrain_width;         /* env_length, env_width */
    int32_t terrain_curriculum;
    int32_t max_init_terrain_level;
    int32_t measure_heights;
    int32_t num_points_x, num_points_y;          /* 17, 11 */
    float measured_points_x[LSIM_MAX_HEIGHT_PTS_X];
    float measured_points_y[LSIM_MAX_HEIGHT_PTS_Y];
    float slope_threshold;          /* trimesh vertical-wall correction, TER:72-75 */
    float terrain_friction, terrain_restitution;

    /* termination (AGC:141-146, LR:249-286) */
    int32_t term_base_vel_violate_commands, term_out_of_border, term_fall_down;
    int32_t max_episode_length;     /* ceil(episode_length_s / dt), LR:1261 */
    int32_t send_timeouts;

    /* rewards (AGC:216-270) */
    float reward_scales[LSIM_NUM_REWARD_TERMS];  /* already multiplied by dt (LR:1046); 0 = inactive */
    int32_t only_positive_rewards;
    float tracking_sigma, soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit;
    float base_height_target, max_contact_force, foot_height_target_base, foot_height_target_terrain;
    int32_t stairsup_start_idx, stairsup_end_idx, pit_start_idx, gap_end_idx;   /* LR:79-90 */
    float episode_length_s;

    /* observations (AGC:272-291) */
    float obs_scale_lin_vel, obs_scale_ang_vel, obs_scale_dof_pos, obs_scale_dof_vel, obs_scale_height;
    int32_t add_noise;
    /* entries of noise_scale_vec (LR:883-910) as the host computed them in double precision:
       ang_vel (obs 3:6), gravity (6:9), dof_pos (9:21), dof_vel (21:33), heights (45+6 .. +187); commands/actions are 0 */
    float noise_vec_ang_vel, noise_vec_gravity, noise_vec_dof_pos, noise_vec_dof_vel, noise_vec_height;

    /* simulator (LRC:238-255); the solver is the build's own (DESIGN.md "Physics") */
    float gravity[3];
    int32_t solver_iterations;      /* sweeps of the velocity-level Gauss-Seidel solver (solver_type 0) */
    float contact_offset, max_depenetration_velocity, erp, contact_slop;
    int32_t using_amp;              /* LRC:36: step() also produces terminal AMP states */
    float max_linear_velocity, max_angular_velocity;   /* asset options LRC:229-230 (1000 / 1000): PhysX clamps body velocities there */
    /* cfg.sim.physx.solver_type (LRC:245): 0 = PGS -- `solver_iterations` velocity-level sweeps over the whole sim_dt;
       1 = TGS (Temporal Gauss-Seidel, what every reference config sets) -- the sim_dt is split into `num_position_iterations`
       sub-iterations (LRC:246; 1..LSIM_MAX_POSITION_ITERATIONS), each relaxes every row once against the positional error reached
       so far.  num_velocity_iterations (LRC:247) is 0 in the reference and not modelled. */
    int32_t solver_type;
    int32_t num_position_iterations;
    /* what the LINEAR velocity columns of the state tensors mean (root_states[:, 7:10], rigid_body_states[:, :, 7:10]; LR:929-941):
       1 = the velocity of the body's CENTRE OF MASS, which is what PhysX's getLinearVelocity() / setLinearVelocity() read and write and
       therefore what the reference's base_lin_vel (LR:198-199), feet velocities (LR:941), pushes (LR:822-828) and reset velocities
       (LR:816) are -- with the per-env payload COM displacement of the base included (LR:1025-1028); 0 = the velocity of the link origin
       (rounds 1-4 of this build).  Positions are the link origin's in both.  Injected tensors (LSIM_STEP_SKIP_PHYSICS) are taken as they
       are.  make_lsim_config sets 1. */
    int32_t lin_vel_at_com;
    /* solver_type 1 only: velocity-level Gauss-Seidel passes over the joint-limit rows ALONE after the last position iteration (contact
       impulses frozen, bounds of the configuration reached).  One relaxation per position iteration leaves the limit rows of a stiffly
       coupled leg short of their bounds; one such pass brings the share of joint speeds beyond the URDF limit to that of 8 PGS sweeps
       (DESIGN.md section 4).  0 = none (round 4); make_lsim_config sets 1; at most LSIM_MAX_POSITION_ITERATIONS. */
    int32_t tgs_limit_passes;
    int32_t reserved[2];
} lsim_config;

/* ---- device buffers.  Shapes are per handle (N = num_envs); dtype codes below. ---- */
#define LSIM_DT_F32 0
#define LSIM_DT_I64 1
#define LSIM_DT_U8 2   /* torch.bool compatible */
#define LSIM_DT_I32 3
#define LSIM_DT_I16 4

enum lsim_buffer_id {
    LSIM_BUF_OBS = 0,            /* f32 [N,270]   obs_buf, newest frame first (LR:403) */
    LSIM_BUF_PRIV_OBS,           /* f32 [N,238]   privileged_obs_buf (LR:404) */
    LSIM_BUF_REW,                /* f32 [N]       rew_buf (LR:368-380) */
    LSIM_BUF_RESET,              /* u8  [N]       reset_buf (LR:255, LR:329) */
    LSIM_BUF_TIME_OUT,           /* u8  [N]       time_out_buf (LR:260) */
    LSIM_BUF_EXTRAS_TIME_OUTS,   /* u8  [N]       extras["time_outs"]: only refreshed on steps with >=1 reset (LR:358-359) */
    LSIM_BUF_EPISODE_LENGTH,     /* i64 [N]       episode_length_buf (BT:73), caller-writable (HIMR:90-91) */
    LSIM_BUF_ROOT_STATES,        /* f32 [N,13]    gym root state tensor (LR:930) */
    LSIM_BUF_DOF_STATE,          /* f32 [N,12,2]  gym dof state tensor (LR:932) */
    LSIM_BUF_RIGID_BODY_STATES,  /* f32 [N,17,13] (LR:938) */
    LSIM_BUF_CONTACT_FORCES,     /* f32 [N,17,3]  net contact force per body, last sub-step (LR:944) */
    LSIM_BUF_TORQUES,            /* f32 [N,12]    last sub-step torques (LR:146) */
    LSIM_BUF_ACTIONS,            /* f32 [N,12]    clipped actions (LR:130) */
    LSIM_BUF_LAST_ACTIONS,       /* f32 [N,12] */
    LSIM_BUF_LAST_LAST_ACTIONS,  /* f32 [N,12] */
    LSIM_BUF_LAST_DOF_POS,       /* f32 [N,12] */
    LSIM_BUF_LAST_DOF_VEL,       /* f32 [N,12] */
    LSIM_BUF_LAST_TORQUES,       /* f32 [N,12] */
    LSIM_BUF_LAST_ROOT_VEL,      /* f32 [N,6] */
    LSIM_BUF_COMMANDS,           /* f32 [N,4]     (LR:967) */
    LSIM_BUF_BASE_LIN_VEL,       /* f32 [N,3]     (LR:198) */
    LSIM_BUF_BASE_ANG_VEL,       /* f32 [N,3] */
    LSIM_BUF_PROJECTED_GRAVITY,  /* f32 [N,3] */
    LSIM_BUF_FEET_AIR_TIME,      /* f32 [N,4] */
    LSIM_BUF_LAST_CONTACTS,      /* u8  [N,4] */
    LSIM_BUF_CONTACT_FILT,       /* u8  [N,4] */
    LSIM_BUF_MEASURED_HEIGHTS,   /* f32 [N,187]   (LR:624) */
    LSIM_BUF_PENDING_FORCE,      /* f32 [N,3]     body-local force on the base drawn at LR:842-844, consumed (and cleared) by the
                                                  first sub-step of the next step; the reference's self.disturbance is zero
                                                  again after every step (LR:235), its value survives only inside priv obs */
    LSIM_BUF_TERRAIN_LEVELS,     /* i64 [N] */
    LSIM_BUF_TERRAIN_TYPES,      /* i64 [N] */
    LSIM_BUF_ENV_ORIGINS,        /* f32 [N,3] */
    LSIM_BUF_KP_FACTORS,         /* f32 [N] */
    LSIM_BUF_KD_FACTORS,         /* f32 [N] */
    LSIM_BUF_MOTOR_STRENGTH,     /* f32 [N,12]    drawn once (LR:999-1007) */
    LSIM_BUF_MOTOR_STRENGTH_FACTORS, /* f32 [N]   redrawn at reset, never used (quirk 8) */
    LSIM_BUF_FRICTION,           /* f32 [N] */
    LSIM_BUF_RESTITUTION,        /* f32 [N] */
    LSIM_BUF_PAYLOAD,            /* f32 [N] */
    LSIM_BUF_COM_DISPLACEMENT,   /* f32 [N,3] */
    LSIM_BUF_EPISODE_SUMS,       /* f32 [N,LSIM_NUM_REWARD_TERMS] */
    LSIM_BUF_TERM_PRIV_OBS,      /* f32 [N,238]   rows valid where reset_buf (LR:227) */
    LSIM_BUF_TERM_AMP_OBS,       /* f32 [N,30]    rows valid where reset_buf (LR:228) */
    LSIM_BUF_AMP_OBS,            /* f32 [N,30]    get_amp_observations() of the post-step state (LR:406-416) */
    LSIM_BUF_DELAY_STEPS,        /* i32 [N]       action delay applied in the last step: the draw of LR:134, 0 with lsim_config.delay off (LR:135) */
    LSIM_BUF_CONTACT_COUNT,      /* i32 [N,2]     diagnostic: collision points within contact_offset of the terrain BEFORE the cap of
                                                  LSIM_MAX_CONTACTS -- [0] maximum over the sub-steps of this step, [1] last sub-step */
    LSIM_BUF_SUBSTEP_TORQUES,    /* f32 [N,decimation,12] diagnostic, written only under LSIM_STEP_RECORD_SUBSTEPS: the torques of EVERY sub-step
                                                  (LR:146 keeps only the last), i.e. _compute_torques(delayed_actions[:, i]) of LR:138-146 -- what
                                                  makes the action-delay model observable from outside */
    LSIM_BUF_STATS,              /* f32 [2,LSIM_STATS_SIZE] device-side per-step reductions, see below */
    LSIM_BUF_NONFINITE,          /* i64 [2]       [0] env-steps since lsim_create in which a robot's simulated state (root 13, joint angles 12, joint velocities 12, after the
                                                  last sub-step) held a NaN or an infinity -- CUMULATIVE, never cleared by the library (the caller may zero it); [1] the
                                                  step counter of the latest such step.  A robot that went non-finite stays so until its episode times out: it is
                                                  counted in every step.  Must stay 0: anything else is a solver blow-up, and until round 6 it was only visible as a slow kernel A */
    LSIM_BUF_HEIGHT_GRID,        /* i16 [rows,cols] */
    LSIM_BUF_TERRAIN_ORIGINS,    /* f32 [levels,types,3] */
    LSIM_BUF_TERRAIN_MESH,       /* i32 [rows,cols] per grid vertex of the reference's triangle mesh: bits 0-15 = height sample (int16);
                                    bits 16-17 = dx+1, bits 18-19 = dy+1 (horizontal displacement of the vertex, in cells: the
                                    slope_treshold vertical-wall correction, TER:72-75); bit 20 = some vertex of the 4x4 block around
                                    cell (i,j) is displaced (contacts there use the exact triangle query) */
    LSIM_NUM_BUFFERS
};

/* layout of one row of LSIM_BUF_STATS.  Two rows ping-pong: every lsim_step / lsim_reset_all call fills the row
 * lsim_get_stats_row() reports after the call and clears the other row for the next call, so a row stays valid
 * until the next call has run (read it, or copy it on the stream, before stepping again).
 *   [0]                      number of envs reset this step
 *   [1 .. 1+T)               sum over reset envs of episode_sums[k] / clip(ep_len,1)   (LR:349; divide by [0] and dt)
 *   [1+T]                    reserved (the host forms mean(terrain_levels), LR:353, from LSIM_BUF_TERRAIN_LEVELS)
 *   [2+T .. 10+T)            command_ranges[4][2] live values (LR:877-880)
 *   [10+T]                   reserved (the tracking sum of LR:875 is kept in fixed point, below)
 *   [11+T]                   reserved
 *   [12+T]                   number of envs whose simulated state was not finite in THIS step (see LSIM_BUF_NONFINITE for the running total)
 *   [LSIM_STATS_FIX ..)      internal, not for the host: int64 fixed-point (2^-32, each addend clamped to +-2^20) accumulators of [1 .. 1+T) and of the sum over reset envs of
 *                            episode_sums[tracking_lin_vel] (LR:875), and a ticket counter.  Waves add to them with integer atomics, so the sums
 *                            -- extras["episode"] and the command-curriculum decision -- do not depend on the order the waves arrive in; the last
 *                            resetting wave of a step converts [1 .. 1+T) to fp32.
 */
#define LSIM_STATS_RESET_COUNT 0
#define LSIM_STATS_EPISODE_SUMS 1
#define LSIM_STATS_LEVEL_SUM (1 + LSIM_NUM_REWARD_TERMS)
#define LSIM_STATS_CMD_RANGES (2 + LSIM_NUM_REWARD_TERMS)
#define LSIM_STATS_TRACK_SUM (10 + LSIM_NUM_REWARD_TERMS)
#define LSIM_STATS_RESET_STEPS (11 + LSIM_NUM_REWARD_TERMS)
#define LSIM_STATS_NONFINITE (12 + LSIM_NUM_REWARD_TERMS)
#define LSIM_STATS_FIX ((17 + LSIM_NUM_REWARD_TERMS) & ~1)      /* even float index: the int64 words are 8-byte aligned (rows are too) */
#define LSIM_STATS_FIX_TRACK LSIM_NUM_REWARD_TERMS             /* word index of the tracking sum */
#define LSIM_STATS_FIX_TICKET (LSIM_NUM_REWARD_TERMS + 1)      /* word index of the ticket counter */
#define LSIM_STATS_FIX_WORDS (LSIM_NUM_REWARD_TERMS + 2)
#define LSIM_STATS_SIZE (LSIM_STATS_FIX + 2 * LSIM_STATS_FIX_WORDS)

/* flags of lsim_step_ex */
#define LSIM_STEP_DEFAULT 0u
#define LSIM_STEP_SKIP_PHYSICS 1u   /* test hook: use ROOT/DOF/RIGID_BODY/CONTACT buffers as injected by the caller
                                       instead of simulating; still computes torques (E3) for the 4 sub-steps */
#define LSIM_STEP_NO_RESET 2u       /* test hook: compute reset_buf but do not reset_idx */
#define LSIM_STEP_RECORD_SUBSTEPS 4u /* test hook: also write LSIM_BUF_SUBSTEP_TORQUES (one 48-byte store per sub-step and robot) */
#define LSIM_STEP_TWO_KERNELS 8u    /* test / measurement hook: run reset_idx + observations as the separate kernel B on every step (the form the
                                       command-curriculum steps always take) instead of inside kernel A.  Same results, bit for bit */
#define LSIM_STEP_FLAT_PRIORITY 16u /* measurement hook: every wave of kernel A at the default issue priority (by default a robot's wave is raised with
                                       its number of contacts, so that the launch's slowest waves are not also waiting for their turn).  Same results */

typedef struct lsim_sim* lsim_handle;

/* sizeof() of the two structs as compiled into the library -- lets a foreign binding verify its mirror. */
int lsim_sizeof_config(void);
int lsim_sizeof_model(void);
int lsim_abi_version(void);

/* bytes of device memory one simulator instance needs (all buffers, 256-B aligned). */
int lsim_query_arena(const lsim_config* cfg, size_t* bytes_out);

/* replaces gym.create_sim + add_triangle_mesh/add_heightfield/add_ground + load_asset + create_env/create_actor
 * + acquire_*_tensor + prepare_sim (LR:467, LR:1069-1104, LR:1135, LR:1184-1205, LR:917-920, BT:85) and the
 * buffer allocation of BaseTask.__init__/LeggedRobot._init_buffers (BT:70-79, LR:913-1032).
 * height_grid: host int16 [grid_rows*grid_cols] (may be NULL for mesh_type plane);
 * terrain_origins: host float [terrain_num_rows*terrain_num_cols*3] (may be NULL for plane). */
int lsim_create(const lsim_config* cfg, const lsim_robot_model* model,
                const int16_t* height_grid, const float* terrain_origins,
                void* arena_dev, int device_id, lsim_handle* out);

/* several quadrupeds in one instance: env e simulates robot env_robot[e] (host uint8 [num_envs], each < num_robots) for its whole life.
 * cfgs[k] / models[k] describe robot k; cfgs[k] is a complete config for it (as for lsim_create), and the configs may differ ONLY in the
 * robot-specific set:
 *     action_scale, hip_reduction, p_gains, d_gains, torque_limits, default_dof_pos, base_init_state,
 *     base_height_target, foot_height_target_base, foot_height_target_terrain
 * (and the whole lsim_robot_model).  Everything else -- task, terrain, rewards, commands, domain randomisation, noise, solver -- is shared.
 * LSIM_E_INVALID if two configs differ outside that set, num_robots is not in 1..LSIM_MAX_ROBOTS, an env_robot entry is out of range, or a
 * robot is given no env.  The arena is sized by lsim_query_arena(&cfgs[0]).  Random draws are keyed by env as in lsim_create, so env e of
 * a mixed instance evolves exactly as env e of the single-robot instance of its robot (same config, seed and terrain).  lsim_create is the
 * num_robots = 1 case of this call. */
int lsim_create_mixed(const lsim_config* cfgs, const lsim_robot_model* models, int32_t num_robots,
                      const uint8_t* env_robot, const int16_t* height_grid, const float* terrain_origins,
                      void* arena_dev, int device_id, lsim_handle* out);

/* replaces gymtorch.wrap_tensor(acquire_*) (LR:930-944): device pointer + shape of one buffer. */
int lsim_get_buffer(lsim_handle h, int buffer_id, void** dev_ptr, int64_t shape[4], int* ndim, int* dtype);

/* LeggedRobot.reset_idx(all envs) as called by BaseTask.reset (BT:113); the caller follows it with one
 * zero-action lsim_step to complete reset() (BT:114). */
int lsim_reset_all(lsim_handle h, void* hip_stream);

/* LeggedRobot.reset_idx(env_ids) (LR:290-361) called from outside a step (a play / evaluation script resetting some robots by hand):
 * terrain curriculum per env, command curriculum over the reset set, dof / root / command / domain-randomisation redraws, buffer
 * clears, extras["episode"] sums into the stats row, episode_length_buf = 0.  reset_mask_dev: device uint8 [N], nonzero = reset this env
 * (the boolean form of env_ids; it is read by the kernels of this call only).  An all-zero mask is the reference's early return
 * (LR:298): only the stats rows swap, with a reset count of 0.  As after lsim_reset_all, observations are not recomputed (the reference
 * does not either): they are those of the next lsim_step.  Random draws are keyed by (env, common_step_counter, number of lsim_reset_envs
 * calls on this handle so far): every call draws fresh values, as every reset_idx of the reference does -- resetting an env that already
 * reset in the adjacent step, or the same env twice between two steps, gives it a new state each time.  Asynchronous on hip_stream. */
int lsim_reset_envs(lsim_handle h, const uint8_t* reset_mask_dev, void* hip_stream);

/* LeggedRobot.step(actions) (LR:122-176): replaces set_dof_actuation_force_tensor/simulate/fetch_results/
 * refresh_* x4 (LR:146-152), refresh_* (LR:187-190), set_*_indexed (LR:714, LR:818), set_actor_root_state_tensor
 * (LR:828), apply_rigid_body_force_tensors (LR:844) and the whole post_physics_step (LR:178-247).
 * actions_dev: device float [N,12].  Asynchronous on hip_stream. */
int lsim_step(lsim_handle h, const float* actions_dev, void* hip_stream);
int lsim_step_ex(lsim_handle h, const float* actions_dev, uint32_t flags, void* hip_stream);

/* host-side scalars (no device sync): common_step_counter (LR:194). */
int lsim_get_step_counter(lsim_handle h, int64_t* counter_out);
int lsim_set_step_counter(lsim_handle h, int64_t counter);
/* number of lsim_reset_envs calls on this handle so far (the salt of their random draws): a resumed run that restores it together with the
 * step counter redraws the same by-hand reset states as an uninterrupted one. */
int lsim_get_reset_calls(lsim_handle h, uint32_t* calls_out);
int lsim_set_reset_calls(lsim_handle h, uint32_t calls);
/* which row (0/1) of LSIM_BUF_STATS the most recent lsim_step / lsim_reset_all filled. */
int lsim_get_stats_row(lsim_handle h, int* row_out);

/* measurement aid (replaces the reference's time.time() bracketing, HIMR:106-147): with capacity > 0 every following
 * lsim_step records HIP events around its kernels on the caller's stream (no host sync); lsim_read_profile waits for
 * the last recorded step and returns per-step durations in milliseconds of kernel A (physics + post-physics) and
 * kernel B (reset + observations) for the most recent min(n_steps, capacity) steps; *n_inout: in = array length,
 * out = number of entries written.  capacity == 0 disables and frees the events. */
int lsim_set_profiling(lsim_handle h, int capacity);
int lsim_read_profile(lsim_handle h, float* ms_kernel_a, float* ms_kernel_b, int* n_inout);

/* name of a reward term / buffer (for bindings and logs); NULL if out of range. */
const char* lsim_reward_name(int reward_id);
const char* lsim_buffer_name(int buffer_id);

const char* lsim_last_error(lsim_handle h);
void lsim_destroy(lsim_handle h);

/* ---- rollout-side fused kernels (SURVEY.md 8f "fused storage"): the elementwise / storage half of the on-policy rollout
 * step.  The networks' GEMMs stay with the caller (PyTorch); these two calls replace the ~35 small torch kernels of
 *   HIMPPO.act                (HIMP:90-103: sample a ~ N(mean, std), log-prob, keep mean/std/values/observations),
 *   HIMPPO.process_env_step   (HIMP:105-118: next critic obs with the termination rows patched in, HIMR:119-121;
 *                              time-out bootstrap  r += gamma * V * time_out),
 *   HIMRolloutStorage.add_transitions (HST:92-106: eleven copies into the [T, N, .] storage at the step index).
 * Stateless: every argument is a device pointer (or scalar) of the caller; `step_idx_dev` and `draw_counter_dev` live
 * in device memory so that both calls can be captured in a HIP graph and replayed.  All pointers are fp32 unless noted. */
typedef struct lsim_rollout_storage {
    float* observations;                 /* [T, N, num_obs]       HST:60 */
    float* privileged_observations;      /* [T, N, num_priv_obs]  HST:62 */
    float* next_privileged_observations; /* [T, N, num_priv_obs]  HST:63 */
    float* actions;                      /* [T, N, num_actions] */
    float* values;                       /* [T, N, 1] */
    float* actions_log_prob;             /* [T, N, 1] */
    float* mu;                           /* [T, N, num_actions] */
    float* sigma;                        /* [T, N, num_actions] */
    float* rewards;                      /* [T, N, 1] */
    uint8_t* dones;                      /* [T, N, 1] u8 */
    int32_t num_steps, num_envs, num_obs, num_priv_obs, num_actions;   /* num_actions <= 32; row sizes even */
} lsim_rollout_storage;

/* actions_out[N, A] = mean + std * z with z ~ N(0,1) from Philox4x32-10 keyed (seed, rank), counter
 * (env, *draw_counter_dev, LSIM_RNG_POLICY, pair index), Box-Muller; log-prob summed over the action dimension;
 * writes storage row *step_idx_dev of observations, privileged_observations, actions, values, actions_log_prob, mu, sigma.
 * mean [N, A], std [A] (the policy's std parameter), values [N, 1], obs [N, num_obs], priv_obs [N, num_priv_obs]. */
int lsim_rollout_act(const lsim_rollout_storage* st, const int64_t* step_idx_dev, const int64_t* draw_counter_dev,
                     const float* mean, const float* std, const float* values, const float* obs, const float* priv_obs,
                     uint32_t seed, uint32_t rank, float* actions_out, void* stream);
/* after lsim_step: writes storage row *step_idx_dev of next_privileged_observations (term_priv_obs rows where dones, else
 * priv_obs), rewards (+ gamma * values * time_outs when time_outs != NULL), dones; then a second tiny kernel advances
 * *step_idx_dev and *draw_counter_dev by one.  dones / time_outs are u8 [N]; values is the [N, 1] critic output kept
 * from lsim_rollout_act's inputs. */
int lsim_rollout_post(const lsim_rollout_storage* st, int64_t* step_idx_dev, int64_t* draw_counter_dev,
                      const uint8_t* dones, const uint8_t* time_outs, const float* rewards, const float* values,
                      const float* priv_obs, const float* term_priv_obs, float gamma, void* stream);
/* lsim_rollout_act / lsim_rollout_post with the storage row and the sampler's counter passed BY VALUE (a host-driven rollout loop knows
 * both): same kernels, same results, and no second launch to advance device-side counters -- the caller advances its own.
 * LSIM_E_INVALID when step_idx is outside [0, num_steps). */
int lsim_rollout_act_at(const lsim_rollout_storage* st, int64_t step_idx, int64_t draw_counter,
                        const float* mean, const float* std, const float* values, const float* obs, const float* priv_obs,
                        uint32_t seed, uint32_t rank, float* actions_out, void* stream);
int lsim_rollout_post_at(const lsim_rollout_storage* st, int64_t step_idx, const uint8_t* dones, const uint8_t* time_outs,
                         const float* rewards, const float* values, const float* priv_obs, const float* term_priv_obs, float gamma,
                         void* stream);
/* GAE(lambda) reverse sweep of HIMRolloutStorage.compute_returns (HST:113-123), one thread per env over the T stored steps:
 *   delta = r_t + (1 - done_t) * gamma * V_{t+1} - V_t;   A_t = delta + (1 - done_t) * gamma * lam * A_{t+1};   returns_t = A_t + V_t
 * with V_T = last_values [N, 1].  Writes returns [T, N, 1] and the raw advantages returns - values [T, N, 1]; the batch
 * normalisation of HST:126-127 (a global mean / std, reduced over ranks when data parallel) stays with the caller. */
int lsim_rollout_gae(const lsim_rollout_storage* st, const float* last_values, float gamma, float lam,
                     float* returns, float* advantages, void* stream);

/* ---- fused rollout-time forward of the HIM policy (HAC:136-163, HES:64-68, HIMP:90-96): estimator encoder
 * (observation history -> 3 velocity + latent), L2-normalised latent, actor on [one-step obs, velocity, latent], critic on the
 * privileged observation -- 11 Linear layers with ELU between them -- in one launch, MFMA fp32, activations in LDS.
 * Weights are passed PADDED and TILED: both dimensions rounded up to multiples of 16 (zero filled beyond [n_out][k_in]) and stored as
 * 16 x 16 blocks, weight[(n / 16) * (k_pad / 16) + k / 16][n % 16][k % 16] -- the 1 KB block of output tile n / 16 and k chunk k / 16 is
 * contiguous, so the wave that owns an output tile reads whole cache lines, each once (ABI v5; v4 took [n_pad][k_pad] row-major: half a
 * line per row and chunk, with the second half evicted from the CU's 32 KB vector cache before its turn when a wave owned two tiles) --
 * bias [n_pad]; 16-byte aligned (the caller packs torch's nn.Linear parameters once per policy update).
 * mean_out [num_envs, num_actions], values_out [num_envs, 1].  LSIM_E_UNSUPPORTED for other topologies / sizes (hidden widths > 512,
 * inputs > 272, a first actor layer padded beyond 272, a layer whose k_pad exceeds its predecessor's n_pad -- it would read activation
 * columns nobody wrote): run the networks in the host framework then. */
typedef struct lsim_mlp_layer {
    const float* weight;      /* [n_pad / 16][k_pad / 16][16][16]: see above */
    const float* bias;        /* [n_pad] */
    int32_t k_pad, n_pad, k_in, n_out;
} lsim_mlp_layer;
typedef struct lsim_him_policy {
    lsim_mlp_layer encoder[3];   /* HES:36-45  history -> ... -> 3 + latent (no activation after the last layer) */
    lsim_mlp_layer actor[4];     /* HAC:66-80  one_step_obs + 3 + latent -> ... -> num_actions */
    lsim_mlp_layer critic[4];    /* HAC:82-95  privileged obs -> ... -> 1 */
    int32_t num_obs, num_priv_obs, num_one_step_obs, num_actions;
} lsim_him_policy;
int lsim_policy_forward(const lsim_him_policy* p, const float* obs, const float* priv_obs, int64_t num_envs, float* mean_out,
                        float* values_out, void* stream);

/* lsim_policy_forward and lsim_rollout_act_at in ONE launch: the blocks that evaluate the networks also copy the observation rows into
 * storage row step_idx, sample the actions (same Philox draws, same log-probability sums as lsim_rollout_act) and store actions, values,
 * log-prob, mu, sigma.  num_envs = st->num_envs; the storage's observation widths and action count must equal the policy's. */
int lsim_policy_act_at(const lsim_him_policy* p, const lsim_rollout_storage* st, int64_t step_idx, int64_t draw_counter,
                       const float* obs, const float* priv_obs, const float* std, uint32_t seed, uint32_t rank,
                       float* mean_out, float* values_out, float* actions_out, void* stream);

/* lsim_policy_act_at that also performs the PREVIOUS step's lsim_rollout_post_at (prev_step < 0: none): the privileged observation the critic
 * blocks stage for this step is the previous step's next critic observation (termination rows patched in from prev_term_priv_obs where
 * prev_dones), and values_out still holds the previous step's values when they form  r + gamma * V * time_out.  The caller stores the last
 * step of a rollout with lsim_rollout_post_at.  Same results as the separate calls. */
int lsim_policy_act_post_at(const lsim_him_policy* p, const lsim_rollout_storage* st, int64_t step_idx, int64_t draw_counter,
                            const float* obs, const float* priv_obs, const float* std, uint32_t seed, uint32_t rank,
                            float* mean_out, float* values_out, float* actions_out,
                            int64_t prev_step, const uint8_t* prev_dones, const uint8_t* prev_time_outs, const float* prev_rewards,
                            const float* prev_term_priv_obs, float gamma, void* stream);

/* The two launches above with ONE MORE SEGMENT of the actor input (a vision policy's depth latent, learn/vision.py).  The actor's first layer
 * then reads, in this column order,
 *   [ one-step observation (num_one_step_obs) | velocity estimate (3) | normalised latent (encoder[2].n_out - 3) | rows[env, 0 .. dim) ]
 * i.e. the extra columns come LAST: a policy whose first actor layer holds zeros there computes what the plain launch computes, bit for bit.
 * Rows past num_envs and the columns up to k_pad read zero.  Nothing else of the launch differs (same blocks, sampling, stores).
 * `store`: NULL, or a dense [num_steps, num_envs, dim] tensor whose row step_idx receives the rows the actor read (lsim_policy_act_post_at_ext
 * only; lsim_policy_forward_ext ignores it).
 * Checked on the host before anything is launched or written: LSIM_E_INVALID for a NULL struct or rows, dim < 1 or ld < dim;
 * LSIM_E_UNSUPPORTED unless actor[0].k_in == num_one_step_obs + encoder[2].n_out + dim and actor[0].k_pad <= 272; and whatever
 * lsim_policy_forward / lsim_policy_act_post_at refuse.  (Those go on refusing a policy whose first actor layer is wider than theirs.) */
typedef struct lsim_policy_extra {
    const float* rows;   /* [num_envs, ld] fp32: row e is appended to env e's actor input */
    int32_t dim, ld;     /* 1 <= dim <= ld */
    float* store;        /* NULL, or dense [T, N, dim]: row step_idx receives the rows (act entry only) */
} lsim_policy_extra;
int lsim_policy_forward_ext(const lsim_him_policy* p, const lsim_policy_extra* extra, const float* obs, const float* priv_obs, int64_t num_envs,
                            float* mean_out, float* values_out, void* stream);
int lsim_policy_act_post_at_ext(const lsim_him_policy* p, const lsim_policy_extra* extra, const lsim_rollout_storage* st, int64_t step_idx,
                                int64_t draw_counter, const float* obs, const float* priv_obs, const float* std, uint32_t seed, uint32_t rank,
                                float* mean_out, float* values_out, float* actions_out,
                                int64_t prev_step, const uint8_t* prev_dones, const uint8_t* prev_time_outs, const float* prev_rewards,
                                const float* prev_term_priv_obs, float gamma, void* stream);

/* ---- the AMP rollout step in one launch (SURVEY.md 8f rank 4 "discriminator reward fused after the step"): what HybridPolicyRunner does between
 * env.step() and process_env_step() (rsl_rl/runners/hybrid_runner.py:183-200) --
 *   next' = where(dones, terminal_amp_states, next_amp_obs)                                  HYBR:191-192
 *   d = head(relu(W2 relu(W1 [norm(amp_obs) | norm(next')] + b1) + b2))                      amp_discriminator.py:55-62, utils/utils.py:124-130
 *   reward = reward_coef * max(1 - (d - 1)^2 / 4, 0);  lerp > 0: (1 - lerp) * reward + lerp * task_reward     amp_discriminator.py:63-72
 *   replay ring rows (cursor + env) % capacity <- (amp_obs, next')                            storage/replay_buffer.py:52-68
 *   amp_obs_carry <- next_amp_obs (the NEXT step's amp_obs, un-patched)                       HYBR:196
 * The two trunk layers use lsim_mlp_layer's padded 16 x 16-block layout (see lsim_him_policy); head_weight [hidden[1].n_pad] zero padded, head_bias [1];
 * norm_mean / norm_var: the running moments as the reference keeps them (float64 [amp_dim]; both NULL = no normaliser).
 * amp_dim <= 32, hidden[0].n_pad <= 1024, hidden[1].n_pad <= 1024; fp32 MFMA, activations in LDS, nothing but the outputs written. */
typedef struct lsim_amp_disc {
    lsim_mlp_layer hidden[2];    /* DISC:18-25: Linear + ReLU, Linear + ReLU */
    const float* head_weight;    /* DISC:27 amp_linear.weight */
    const float* head_bias;      /* amp_linear.bias [1], device */
    const double* norm_mean;     /* UT:78-106 */
    const double* norm_var;
    double norm_eps, norm_clip;  /* UT:114-116: 1e-4, 10 */
    double reward_coef, task_reward_lerp;   /* DISC:14-15 (python floats) */
    int32_t amp_dim, reserved;
} lsim_amp_disc;
/* workspace: lsim_amp_step_workspace() bytes, 16-byte aligned, ZERO-FILLED by the caller before its first use (every call leaves it ready for the next).
 * amp_obs, next_amp_obs, terminal_amp_states [num_envs, amp_dim]; dones u8 [num_envs] or NULL (no patching); task_rewards [num_envs] (may be NULL when
 * lerp == 0); rewards_out [num_envs]; disc_out [num_envs] or NULL (the discriminator's raw output d); amp_obs_carry [num_envs, amp_dim] or NULL, must not
 * alias amp_obs; replay_states / replay_next_states [replay_capacity, amp_dim] or both NULL, replay_capacity >= num_envs, 0 <= replay_cursor < capacity
 * (the caller advances its cursor by num_envs modulo capacity, RB:66-68). */
int lsim_amp_step_workspace(int64_t num_envs, size_t* bytes);
int lsim_amp_step(const lsim_amp_disc* d, const float* amp_obs, const float* next_amp_obs, const uint8_t* dones, const float* terminal_amp_states,
                  const float* task_rewards, int64_t num_envs, float* rewards_out, float* disc_out, float* amp_obs_carry,
                  float* replay_states, float* replay_next_states, int64_t replay_capacity, int64_t replay_cursor,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- learner-side kernel: weight / bias gradient of a small Linear layer over a tall minibatch,
 *   dw[n, k] = sum_b g[b, n] * x[b, k],   db[n] = sum_b g[b, n]      (torch.nn.Linear backward: grad_weight = g^T x, grad_bias = g.sum(0))
 * for any batch >= 1 and any layer of k_in * n_out <= 140 000 weights.  Two forms: layers with ceil(n_out / 16) * ceil(k_in / 16) <= 32 (each
 * <= 8) and k_in * n_out <= 4096 -- the heads and narrow layers of HAC:66-95 / HES:36-54 / DISC:18-25, whose K = 102 400 reductions BLAS runs at
 * a few percent of peak -- keep the whole result in one wave's accumulators (the single-wave form); every other layer runs as 64 x 64 / 64 x 128
 * output tiles (the tiled form).  x [batch, k_in] with row stride ldx >= k_in, g [batch, n_out] with row stride ldg >= n_out (floats), dw
 * [n_out, k_in] and db [n_out] (db may be NULL) contiguous, 4-byte aligned (a slice of a gradient arena).
 * What the tiled form relies on:
 *   - a row pitch ld % 4 == 0 on a 16-byte aligned pointer (ld % 2 == 0 on an 8-byte aligned one, for x) is read in whole 16-byte (8-byte)
 *     vectors up to the pitch: the floats between a row's width and its pitch must be readable, their values (NaN included) never reach a
 *     result.  Any other pitch or alignment is read float by float, inside the width;
 *   - `workspace` is 16-byte aligned when k_in % 4 == 0 (LSIM_E_INVALID otherwise).
 * `workspace` is a caller-allocated device buffer of at least lsim_linear_wgrad_workspace() bytes holding the partial results, one per
 * `num_waves` batch slices (summed in a fixed order: deterministic); every byte of it may be overwritten, none needs initialising.
 * Returns LSIM_E_UNSUPPORTED for batch <= 0 and for larger layers (use BLAS), LSIM_E_INVALID for a NULL x, g, dw or workspace, a pitch below
 * the width or a workspace that is too small. */
int lsim_linear_wgrad_workspace(long batch, int k_in, int n_out, size_t* bytes, int* num_waves);
int lsim_linear_wgrad(const float* x, int64_t ldx, const float* g, int64_t ldg, int64_t batch, int k_in, int n_out,
                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* Forward of a Linear layer followed by ELU (alpha = 1): out[b, :] = elu(x[b, :] W^T + bias), the hidden layers of the actor, critic and
 * estimator MLPs (rsl_rl/modules/him_actor_critic.py:52-76, him_estimator.py:40-62 build them as nn.Linear + nn.ELU pairs; HIMPPO.update
 * runs them on minibatches of 102 400 rows, him_ppo.py:136-150).  fp32 MFMA with the activation applied to the accumulators: the layer's
 * output is written once instead of BLAS output + elementwise read + write.  x [batch, k_in] with leading dimension ldx, weight
 * [n_out, k_in] contiguous (nn.Linear.weight), bias [n_out] or NULL, out [batch, n_out] with leading dimension ldo.
 * LSIM_E_UNSUPPORTED unless n_out % 4 == 0, ldo % 4 == 0 and out is 16-byte aligned (use BLAS + ELU).  x and weight are read at ANY 4-byte
 * alignment, pitch and k_in: the loads are 16 bytes wide where both operands allow it (k_in % 4 == 0, ldx % 4 == 0, both pointers 16-byte aligned),
 * 8 bytes where both allow that, single floats otherwise; only out (and mask_src below) must be 16-byte aligned.  Rows >= batch and the columns
 * between k_in and ldx are never read, the columns between n_out and ldo never written.  The ELU's negative side is exp(x) - 1 with the hardware
 * exponential: for a given pre-activation x <= 0 its absolute error is at most 1.2e-7 (2^-24 for the exponential, (2^-24 + 1.4e-8) / e for the
 * rounding of x log2(e), 2^-25 for the subtraction); elu(0) is +0.0 and elu(x) is exactly -1 for x <= -18; positive x pass unchanged. */
int lsim_linear_elu_forward(const float* x, int64_t ldx, const float* weight, const float* bias, int64_t batch, int k_in, int n_out,
                            float* out, int64_t ldo, void* stream);

/* Backward of a Linear layer followed by ELU (y = x W^T + b, z = elu(y), alpha = 1) given the gradient of z: the gradient of the
 * pre-activation  grad_pre = grad_out * (z > 0 ? 1 : z + 1)  (torch's elu_backward on the saved OUTPUT) is formed on the fly as the MFMA
 * operand of the weight-gradient kernel and written once -- [batch, n_out] contiguous -- for the caller's input-gradient GEMM
 * (grad_pre @ W); dw / db as lsim_linear_wgrad.  One pass over grad_out and z instead of elu_backward + column sum + wgrad.
 * grad_pre may be NULL when no input gradient will be formed (the first layer of a network): the gradient of the pre-activation is then
 * only used inside the kernel and never written.  grad_pre has no pitch argument: row b starts at grad_pre + b * n_out; it is written in
 * 16-byte vectors when n_out % 4 == 0 and must then be 16-byte aligned (LSIM_E_INVALID otherwise).  elu_out [batch, n_out] with row stride
 * ldz >= n_out is read like g; g is read in 16-byte vectors only when g and elu_out both allow it.
 * Same workspace as lsim_linear_wgrad; LSIM_E_UNSUPPORTED for shapes lsim_linear_wgrad handles in its single-wave form (k_in * n_out <= 4096). */
int lsim_linear_elu_wgrad(const float* x, int64_t ldx, const float* grad_out, int64_t ldg, const float* elu_out, int64_t ldz, int64_t batch,
                          int k_in, int n_out, float* dw, float* db, float* grad_pre, void* workspace, size_t workspace_bytes, void* stream);

/* The same for a Linear layer followed by ReLU (the AMP discriminator's trunk, amp_discriminator.py:18-25), given the saved ReLU OUTPUT:
 * grad_pre = grad_out * [relu_out > 0] (torch's threshold_backward). */
int lsim_linear_relu_wgrad(const float* x, int64_t ldx, const float* grad_out, int64_t ldg, const float* relu_out, int64_t ldz, int64_t batch,
                           int k_in, int n_out, float* dw, float* db, float* grad_pre, void* workspace, size_t workspace_bytes, void* stream);

/* out[b, n] = mask_src[b, n] > 0 ? sum_k x[b, k] weight[n, k] : 0: a product consumed by a ReLU's backward, mask applied to the accumulators (no
 * separate threshold_backward pass).  Limits as lsim_linear_elu_forward; mask_src [batch, n_out] with leading dimension ldm % 4 == 0, 16-byte aligned. */
int lsim_linear_masked_forward(const float* x, int64_t ldx, const float* weight, const float* mask_src, int64_t ldm, int64_t batch, int k_in, int n_out,
                               float* out, int64_t ldo, void* stream);

/* ---- discriminator update (HybridPPO.update, hybrid_ppo.py:236-281): the elementwise passes between the GEMMs of the LSGAN loss / gradient penalty.
 * lsim_relu_head_backward: for the head d = relu_out . head_weight + b on relu_out [batch, n] (leading dimension ld) and grad_d [batch] = d loss / d d:
 *   grad_pre[b, j] = relu_out[b, j] > 0 ? grad_d[b] * head_weight[j] : 0  (one fp32 product; rows DENSE: grad_pre has no pitch argument, row b starts
 *   at grad_pre + b * n, 16-byte aligned; +0.0 and -0.0 in relu_out count as masked),  grad_bias[j] = sum_b grad_pre[b, j],
 *   grad_head [n + 4]: [j < n] = sum_b relu_out[b, j] * grad_d[b],  [n] = sum_b grad_d[b], three zeros  -- one pass, sums in a fixed order.
 * lsim_masked_colsum: out[j] = sum_b (mask_src[b, j] > 0 ? v[b, j] : 0) -- a select, not a product: v may hold anything where the mask is not positive.
 * n % 4 == 0, n <= 1024, n / 4 a divisor of 256; 16-byte aligned rows; workspace lsim_relu_cols_workspace() bytes.  LSIM_E_UNSUPPORTED otherwise. */
int lsim_relu_cols_workspace(int64_t batch, int n, size_t* bytes);
int lsim_relu_head_backward(const float* relu_out, int64_t ld, const float* grad_d, const float* head_weight, int64_t batch, int n,
                            float* grad_pre, float* grad_bias, float* grad_head, void* workspace, size_t workspace_bytes, void* stream);
int lsim_masked_colsum(const float* v, int64_t ldv, const float* mask_src, int64_t ldm, int64_t batch, int n, float* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Normalizer.update (utils/utils.py:86-106; twice per minibatch at hybrid_ppo.py:279-281): the batch moments of x [batch, dim <= 64] merged into the
 * float64 running mean / var / count (device arrays [dim], [dim], [1], updated in place) with the parallel-variance formula; batch sums in float64.
 * Two launches, no host round trip.  workspace: lsim_running_moments_workspace() bytes, 8-byte aligned.
 * The batch variance is the one-pass form sum x^2 / n - mean^2 in float64: its absolute error is bounded by about 3 D 2^-53 times the column's
 * mean square, D = rows per thread + slices / 4 + 6 (below 200 up to 10^5 rows).  On a (nearly) constant column the batch variance IS that rounding
 * noise, of either sign -- negligible next to the Normalizer's epsilon of 1e-4 for |x| up to a few thousand, not beyond: the MERGED variance is
 * therefore clamped at 0 (it is never negative; a NaN stays a NaN).  count becomes count + batch exactly (one float64 addition). */
int lsim_running_moments_workspace(size_t* bytes);
int lsim_running_moments_update(const float* x, int64_t ldx, int64_t batch, int dim, double* mean, double* var, double* count,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The discriminator's input rows of one sampled block in HybridPPO.update (hybrid_ppo.py:247-251 normalize_torch on state and next state, then
 * amp_discriminator.py:57 / :37 torch.cat([state, next_state], dim=-1)):  out[b, 0:dim] = f(states[b]), out[b, dim:2 dim] = f(next_states[b]),
 * f(x) = clamp((x - float32(mean)) / sqrt(float32(var + eps)), +-clip) (utils/utils.py:124-130), or the identity when norm_mean == NULL (the gradient
 * penalty's un-normalised pair).  One launch; `out` may point into a larger stacked evaluation (row pitch ld_out >= 2 dim). */
int lsim_amp_pair_rows(const float* states, int64_t ld_states, const float* next_states, int64_t ld_next, const double* norm_mean,
                       const double* norm_var, double norm_eps, double norm_clip, int64_t batch, int dim, float* out, int64_t ld_out, void* stream);

/* lsim_linear_wgrad and lsim_linear_elu_wgrad with the final, fixed-order sum of the partial results left to the caller: `pending` receives
 * what that sum needs, the workspace must stay untouched until lsim_wgrad_reduce_batch has run for it, and dw / db hold nothing until then.  A backward pass
 * collects the records of all its layers and sums them in ONE launch behind the last weight-gradient kernel (15 launches of a few
 * microseconds per minibatch become one); same arithmetic, same results bit for bit.  items: host array; any n (the call splits it). */
typedef struct lsim_wgrad_pending {
    const float* part; const float* part2;      /* partial results of dw [num_partials, count] and of db [num_partials, count2] (NULL: no bias) */
    float* out; float* out2;                    /* dw, db */
    int32_t num_partials, count, count2, reserved;
} lsim_wgrad_pending;
int lsim_linear_wgrad_deferred(const float* x, int64_t ldx, const float* g, int64_t ldg, int64_t batch, int k_in, int n_out,
                               float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream, lsim_wgrad_pending* pending);
int lsim_linear_elu_wgrad_deferred(const float* x, int64_t ldx, const float* grad_out, int64_t ldg, const float* elu_out, int64_t ldz, int64_t batch,
                                   int k_in, int n_out, float* dw, float* db, float* grad_pre, void* workspace, size_t workspace_bytes, void* stream,
                                   lsim_wgrad_pending* pending);
int lsim_linear_relu_wgrad_deferred(const float* x, int64_t ldx, const float* grad_out, int64_t ldg, const float* relu_out, int64_t ldz, int64_t batch,
                                    int k_in, int n_out, float* dw, float* db, float* grad_pre, void* workspace, size_t workspace_bytes, void* stream,
                                    lsim_wgrad_pending* pending);
int lsim_wgrad_reduce_batch(const lsim_wgrad_pending* items, int n, void* stream);

/* dst[r, :] = src[index[r], :] for 4-byte elements (rows of `cols` elements, both contiguous; index: int64 [n] on the device): the once-per-update
 * shuffle of the rollout storage through the minibatch permutation (HST:140-164) at copy bandwidth -- torch's advanced indexing computes an
 * offset per element (2.6 TB/s on these row widths). */
int lsim_gather_rows(const void* src, int64_t cols, const int64_t* index, int64_t n, void* dst, void* stream);
/* the same with destination rows `dst_ld` elements apart (dst_ld >= cols; elements cols .. dst_ld - 1 of a row are left alone): HIMRolloutStorage keeps its
 * shuffled observation fields in rows padded to 16 bytes so that the first layers of the networks read aligned rows */
int lsim_gather_rows_ld(const void* src, int64_t cols, const int64_t* index, int64_t n, void* dst, int64_t dst_ld, void* stream);

/* w[r, :] /= max(||w[r, :]||_2, eps) in place for a small matrix (rows * cols <= 4096): torch.nn.functional.normalize(w, dim=-1, p=2, eps) written
 * back, as HIMEstimator.update does with its prototypes before every loss evaluation (HES:80-81) -- one launch instead of clone, norm, clamp,
 * divide and copy.  Sums in column order: may differ from torch's reduction in the last bit. */
int lsim_normalize_rows(float* w, int rows, int cols, float eps, void* stream);

/* Clipped-PPO loss of HIMPPO.update (HIMP:136-176), forward AND backward in one pass: per-sample Gaussian log-prob, ratio, clipped
 * surrogate, clipped value loss, entropy bonus, and the KL estimate of the adaptive learning-rate rule (HIMP:144-156).
 *   out5 = { mean surrogate, mean value loss, mean entropy, mean KL, total = surrogate + value_loss_coef * value - entropy_coef * entropy }
 *   grad_mu [B, A], grad_sigma [B, A], grad_value [B] = d total / d (mu, sigma, value), torch's sub-gradient conventions.
 * mu, sigma, actions, old_mu, old_sigma [B, A]; value, old_logp, advantages, returns, target_values [B], all contiguous fp32.
 * target_values may be NULL when use_clipped_value_loss == 0.  workspace: lsim_ppo_loss_workspace() bytes; deterministic.
 * The sub-gradients, as torch forms them: max(a, b) gives each side 1/2 where a == b, clamp passes the gradient on the CLOSED interval
 * (ratio == 1 +- clip_param and v - target == +-clip_param pass).  Rows with advantage 0 get grad_mu = 0 exactly and only the entropy
 * term in grad_sigma.  num_actions is unbounded here.  The operands are read only; every element of the outputs is written. */
int lsim_ppo_loss_workspace(long batch, size_t* bytes);
int lsim_ppo_loss(const float* mu, const float* sigma, const float* value, const float* actions, const float* old_logp, const float* advantages,
                  const float* returns, const float* target_values, const float* old_mu, const float* old_sigma, int64_t batch, int num_actions,
                  float clip_param, float value_loss_coef, float entropy_coef, int use_clipped_value_loss,
                  float* out5, float* grad_mu, float* grad_sigma, float* grad_value, void* workspace, size_t workspace_bytes, void* stream);
/* The same with the state-independent standard deviation of HIMActorCritic (HAC:93: `std`, one value per action) passed as what it is: `std`
 * [A] instead of its broadcast sigma [B, A] (the reference forms mean * 0 + std, HAC:147), and grad_std [A] = the column sums of what
 * grad_sigma would hold, added up in a fixed order -- the broadcast, its backward and the column sum (five launches and 10 MB per minibatch)
 * disappear.  workspace: lsim_ppo_loss_std_workspace() bytes.  num_actions <= 60 (LSIM_E_INVALID above).  grad_std must not be NULL and is
 * overwritten, not accumulated into; no grad_sigma [B, A] is formed or needed anywhere. */
int lsim_ppo_loss_std_workspace(long batch, int num_actions, size_t* bytes);
int lsim_ppo_loss_std(const float* mu, const float* std, const float* value, const float* actions, const float* old_logp, const float* advantages,
                      const float* returns, const float* target_values, const float* old_mu, const float* old_sigma, int64_t batch, int num_actions,
                      float clip_param, float value_loss_coef, float entropy_coef, int use_clipped_value_loss,
                      float* out5, float* grad_mu, float* grad_std, float* grad_value, void* workspace, size_t workspace_bytes, void* stream);


/* Adaptive learning rate of HIMPPO (HIMP:144-156) evaluated on the device: *lr_dev /= factor when *kl_mean_dev > 2 desired_kl,
 * *= factor when 0 < *kl_mean_dev < desired_kl / 2, clamped to [lr_min, lr_max].  Both scalars live in device memory (the optimisers read
 * the same lr tensor), so the reference's per-minibatch host read-back of the KL estimate is not needed. */
int lsim_adaptive_lr(const float* kl_mean_dev, float desired_kl, float lr_min, float lr_max, float factor, float* lr_dev, void* stream);

/* Sinkhorn-Knopp assignment of the estimator's prototype scores (HIMEstimator.sinkhorn, HES:119-133; no gradient flows through it):
 *   Q = exp(scores / eps)^T;  Q /= sum(Q);  iters x { Q /= rowsum; Q /= K; Q /= colsum; Q /= B };  out = (Q * B)^T
 * scores [batch, K] with row stride lds (floats), K <= 64, out [batch, K] contiguous.  Computed as E * u[k] * v[b] with 2 * iters + 1
 * small launches instead of ~26 passes over the matrix; `workspace` holds E and the per-block partial sums
 * (lsim_sinkhorn_workspace() bytes, 16-byte aligned like `out`); sums are formed in a fixed order (deterministic).
 * `workspace` and `out` must be 16-byte aligned whatever K is (LSIM_E_INVALID otherwise); `scores` needs 4-byte alignment only: rows are read
 * with 16-byte loads when K % 4 == 0, lds % 4 == 0 and the pointer is 16-byte aligned, one float at a time otherwise.  lds >= K, eps > 0,
 * iters >= 1, batch >= 1.  exp(scores / eps) must stay finite in fp32 (cosine scores and eps = 0.05 reach exp(20)). */
int lsim_sinkhorn_workspace(long batch, int K, size_t* bytes);
int lsim_sinkhorn(const float* scores, int64_t lds, int64_t batch, int K, float eps, int iters, float* out,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Loss head of HIMEstimator.update (HES:76-108) forward AND backward, everything between the two encoder outputs and the scalar loss:
 *   enc_out [batch, 3 + latent] (row stride ld_enc): predicted base velocity | student latent;  tgt_out [batch, latent]: target latent;
 *   proto [K, latent] contiguous, rows already L2-normalised (HES:92-93);  vel [batch, 3] (row stride ld_vel): the regression target.
 *   z = F.normalize(latent), scores = z proto^T, q = Sinkhorn(scores) (no gradient), swap = -0.5 mean(q_s log_softmax(S_t / T) +
 *   q_t log_softmax(S_s / T)), est = mse(pred_vel, vel).
 *   losses3 = { est, swap, est + swap };  grad_enc [batch, 3 + latent], grad_tgt [batch, latent], grad_proto [K, latent] contiguous =
 *   d (est + swap) / d (enc_out, tgt_out, proto).  latent <= 32, K <= 64.  10 launches; sums in a fixed order (deterministic).
 * workspace: lsim_estimator_loss_workspace() bytes, 16-byte aligned.  It is scratch: nothing in it survives the call or is read from an
 * earlier one, and the caller may hand the same bytes to any other entry afterwards.
 * The prototypes are used as given: nothing here normalises them or assumes unit rows, and grad_proto is the gradient with respect to the rows
 * as passed (the caller's normalisation, lsim_normalize_rows, is not differentiated).  A latent row with norm below 1e-12 takes F.normalize's
 * clamped branch: z = x * 1e12 and d x = d z * 1e12, without the projection.  enc_out, tgt_out and vel need 4-byte alignment only; the four
 * operands are read only; every element of the four outputs is written.  temperature > 0, sinkhorn_eps > 0, sinkhorn_iters >= 1. */
int lsim_estimator_loss_workspace(int64_t batch, int latent, int K, size_t* bytes);
int lsim_estimator_loss(const float* enc_out, int64_t ld_enc, const float* tgt_out, int64_t ld_tgt, const float* proto, const float* vel,
                        int64_t ld_vel, int64_t batch, int latent, int K, float temperature, float sinkhorn_eps, int sinkhorn_iters,
                        float* losses3, float* grad_enc, float* grad_tgt, float* grad_proto, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Gradient clipping + Adam of one optimiser step in two launches (HIMP:183-184, HES:113-114: clip_grad_norm_(params, max_grad_norm) then
 * torch.optim.Adam.step(), no amsgrad / weight decay / maximize), on the caller's tensors: `count` <= 48 parameters with numel[i] elements
 * each, their gradients (rescaled in place by min(max_grad_norm / (||g|| + 1e-6), 1), as clip_grad_norm_ does; max_grad_norm <= 0: no
 * clipping), first / second moment estimates and per-parameter step counters (float scalars, incremented).  The pointer tables are HOST
 * arrays of device pointers.  Learning rate: *lr_dev if lr_dev != NULL (device scalar, see lsim_adaptive_lr), else lr_host.
 * grad_norm_out (device, may be NULL) receives the total norm before clipping.  workspace: lsim_adam_clip_step_workspace(count) bytes.
 * Every tensor uses ITS OWN step counter for the bias corrections (counters may differ); the counters hold integers as floats.  0 <= beta < 1,
 * eps > 0, 1 <= numel[i] < 2^31; tensors need 4-byte alignment only and must not overlap. */
int lsim_adam_clip_step_workspace(int count, size_t* bytes);
int lsim_adam_clip_step(int count, const int64_t* numel, float* const* params, float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, float* const* steps, const float* lr_dev, float lr_host, float beta1, float beta2,
                        float eps, float max_grad_norm, float* grad_norm_out, void* workspace, size_t workspace_bytes, void* stream);

/* lsim_adam_clip_step for an optimiser with several parameter groups (HybridPPO, HYBP:86-92 + HYBP:270-273: one Adam over the actor-critic,
 * the discriminator trunk with weight decay 1e-3 and its head with weight decay 1e-1, gradient clipping over the actor-critic's parameters
 * only): weight_decay[i] >= 0 per tensor (torch.optim.Adam's L2 form, grad + weight_decay * param, applied after the clipping and not written
 * back to the gradient; NULL = none), and only tensors [0, clip_count) enter the clipped norm and are rescaled.  grad_norm_out = that norm
 * (0 for clip_count == 0, where nothing is rescaled).  0 <= clip_count <= count. */
int lsim_adam_clip_step_ex(int count, const int64_t* numel, float* const* params, float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, float* const* steps, const float* weight_decay, int clip_count,
                           const float* lr_dev, float lr_host, float beta1, float beta2, float eps, float max_grad_norm,
                           float* grad_norm_out, void* workspace, size_t workspace_bytes, void* stream);

/* Actor input of HIMActorCritic (HAC:136-141; HES:64-68 for the normalisation): out[b] = [ obs[b, :num_one_step_obs] | enc_out[b, :3] |
 * enc_out[b, 3:3+latent] / max(||.||, 1e-12) ], out [batch, num_one_step_obs + 3 + latent] contiguous; obs / enc_out with row strides
 * ld_obs / ld_enc (floats).  No gradient flows through this (the estimator's outputs are detached there). */
int lsim_actor_input(const float* obs, int64_t ld_obs, int num_one_step_obs, const float* enc_out, int64_t ld_enc, int latent,
                     int64_t batch, float* out, void* stream);

/* ---- policy evaluation on the device: grouped metrics and state traces (no reference FFI; the reference evaluates in
 * legged_gym/scripts/play.py:124-164 with .item() reads of one robot and the means of extras["episode"]).
 * ONE launch per env-step, after lsim_step, on the caller's stream, no host synchronisation, capturable in a single-stream graph.
 * The evaluator only READS the simulator's buffers; it works on raw device pointers (this struct, filled by the caller from
 * lsim_get_buffer and its own per-env constants), not on the lsim_handle.
 *
 * Group of an env = ((robot * num_types) + terrain_type) * num_levels + terrain_level, where a factor whose LSIM_EVAL_BY_* bit is NOT set in
 * `group_by` counts as 0 and its extent as 1 (num_groups = product of the kept extents).  robot = robot_ids[env] (0 when robot_ids == NULL);
 * each factor is clamped into [0, extent).  The group is LATCHED when an episode starts: on a reset step terrain_levels already holds the NEXT
 * episode's level.  After lsim_eval_clear the first lsim_eval_accumulate latches every env from the buffers as they are (group, start position),
 * so an episode in progress at that moment is counted from there on; clear right after env.reset() for whole episodes.
 *
 * Every step, per env, in this order (g = the latched group):
 *   return_so_far += fix(rew) (int64, exact), length_so_far += 1          -- rew / reset_buf / time_out_buf describe the step that just ended
 *   reset_buf == 0 -> STEP SAMPLE added to group g (the state buffers hold the state after the step):
 *       SAMPLES += 1
 *       e2 = (cmd_x - base_lin_vel_x)^2 + (cmd_y - base_lin_vel_y)^2;  LIN_ERR += sqrt(e2);  LIN_ERR_SQ += e2
 *       y = |cmd_yaw - base_ang_vel_z|;  YAW_ERR += y;  YAW_ERR_SQ += y * y
 *       POWER += sum_j |tau_j * qd_j|;  TORQUE_SQ += sum_j tau_j^2;  ACTION_RATE += sum_j (a_j - a_last_j)^2        (sums in joint order 0..11, fp32)
 *       FEET_CONTACT += number of nonzero contact_filt[env][0..3]
 *       TORQUE_SAT += number of joints with |tau_j| >= 0.98f * torque_limit_j
 *       PEAK_TORQUE_RATIO = max(PEAK_TORQUE_RATIO, fix(max_j |tau_j| / torque_limit_j))                                (integer atomicMax)
 *     then last_position = root_states[env][0..1]
 *   reset_buf != 0 -> EPISODE RECORD added to group g (the state buffers already hold the post-reset state and are NOT sampled):
 *       EPISODES += 1;  TIME_OUTS += (time_out_buf != 0);  FALLS += (time_out_buf == 0)
 *       RETURN += return_so_far (valid on the reset step too: it is the evaluator's own sum of rew);  LENGTH += length_so_far
 *       DISTANCE += |last_position - start_position| (horizontal; last_position is the last PRE-reset position, so the distance is one
 *                   step short of the episode's end by construction)
 *     then return_so_far = length_so_far = 0, g = group from the buffers now, start_position = last_position = root_states[env][0..1]
 * Accumulators: int64 words, value * 2^32 (fix(v) = llrint(clamp(v, -2^20, 2^20) * 2^32): every addend clamped as in LSIM_BUF_STATS), added with
 * integer atomics, so equal inputs give bitwise equal tables whatever the order of waves; COUNT words are plain integers.  A non-finite addend
 * (incl. a non-finite rew or peak candidate) is not added: it increments the group's NONFINITE word instead.  The host divides. */
#define LSIM_EVAL_BY_ROBOT 1u
#define LSIM_EVAL_BY_TYPE 2u
#define LSIM_EVAL_BY_LEVEL 4u
#define LSIM_EVAL_MAX_GROUPS 4096          /* LSIM_MAX_ROBOTS x LSIM_TERRAIN_TYPES_MAX x LSIM_TERRAIN_LEVELS_MAX */
#define LSIM_EVAL_MAX_TRACE_ENVS 64
#define LSIM_EVAL_SAT_PERMILLE 980         /* TORQUE_SAT threshold: |tau| >= 0.98 x limit */
enum lsim_eval_word {                      /* columns of the table [num_groups, LSIM_EVAL_WORDS] int64; "count" = plain integer, "fix" = value * 2^32 */
    LSIM_EVAL_W_SAMPLES = 0,               /* count */
    LSIM_EVAL_W_LIN_ERR,                   /* fix */
    LSIM_EVAL_W_LIN_ERR_SQ,                /* fix */
    LSIM_EVAL_W_YAW_ERR,                   /* fix */
    LSIM_EVAL_W_YAW_ERR_SQ,                /* fix */
    LSIM_EVAL_W_POWER,                     /* fix */
    LSIM_EVAL_W_TORQUE_SQ,                 /* fix */
    LSIM_EVAL_W_ACTION_RATE,               /* fix */
    LSIM_EVAL_W_FEET_CONTACT,              /* count */
    LSIM_EVAL_W_TORQUE_SAT,                /* count */
    LSIM_EVAL_W_PEAK_TORQUE_RATIO,         /* fix, maximum instead of sum */
    LSIM_EVAL_W_EPISODES,                  /* count */
    LSIM_EVAL_W_TIME_OUTS,                 /* count */
    LSIM_EVAL_W_FALLS,                     /* count */
    LSIM_EVAL_W_RETURN,                    /* fix */
    LSIM_EVAL_W_LENGTH,                    /* count (env-steps) */
    LSIM_EVAL_W_DISTANCE,                  /* fix */
    LSIM_EVAL_W_NONFINITE,                 /* count */
    LSIM_EVAL_WORDS
};
/* Trace ring: row (t mod trace_capacity) of trace [trace_capacity, num_trace_envs, LSIM_EVAL_TRACE_DIM] f32, t = the evaluator's device-side
 * launch counter (starts at 0 after lsim_eval_clear; the first 8 bytes of `state`, int64).  Columns, for env trace_envs[k] -- the fields of the
 * reference's Logger.log_states call (play.py:143-158) for ALL joints and feet, then root pose, reward and reset flag (on a reset step the
 * state columns hold the post-reset state, as the buffers do): */
#define LSIM_EVAL_TR_DOF_POS_TARGET 0      /* 12: actions * action_scale + default_dof_pos (fp32, product and sum rounded separately or fused) */
#define LSIM_EVAL_TR_DOF_POS 12            /* 12 */
#define LSIM_EVAL_TR_DOF_VEL 24            /* 12 */
#define LSIM_EVAL_TR_TORQUES 36            /* 12 */
#define LSIM_EVAL_TR_COMMANDS 48           /* 3: x, y, yaw */
#define LSIM_EVAL_TR_BASE_LIN_VEL 51       /* 3 */
#define LSIM_EVAL_TR_BASE_ANG_VEL 54       /* 3 */
#define LSIM_EVAL_TR_CONTACT_FORCES_Z 57   /* 4: contact_forces[env][feet_bodies[i]][2] */
#define LSIM_EVAL_TR_ROOT_POS 61           /* 3 */
#define LSIM_EVAL_TR_ROOT_QUAT 64          /* 4: xyzw */
#define LSIM_EVAL_TR_REW 68                /* 1 */
#define LSIM_EVAL_TR_RESET 69              /* 1: 0.0 / 1.0 */
#define LSIM_EVAL_TRACE_DIM 70
typedef struct lsim_eval {
    /* simulator buffers (lsim_get_buffer), read only */
    const float* rew;                 /* [N] */
    const uint8_t* reset_buf;         /* [N] */
    const uint8_t* time_out_buf;      /* [N] */
    const float* commands;            /* [N,4]     16-byte aligned */
    const float* base_lin_vel;        /* [N,3] */
    const float* base_ang_vel;        /* [N,3] */
    const float* root_states;         /* [N,13] */
    const float* dof_state;           /* [N,12,2]  16-byte aligned */
    const float* torques;             /* [N,12]    16-byte aligned */
    const float* actions;             /* [N,12]    16-byte aligned */
    const float* last_actions;        /* [N,12]    16-byte aligned */
    const uint8_t* contact_filt;      /* [N,4]     4-byte aligned */
    const float* contact_forces;      /* [N,17,3] */
    const int64_t* terrain_types;     /* [N] */
    const int64_t* terrain_levels;    /* [N] */
    /* per-env constants of the caller */
    const uint8_t* robot_ids;         /* [N] or NULL (one robot) */
    const float* torque_limits;       /* [N,12]    16-byte aligned */
    const float* default_dof_pos;     /* [N,12]    16-byte aligned */
    const float* action_scale;        /* [N,12]    16-byte aligned; per joint, hip reduction included */
    /* evaluator-owned device memory, sizes from lsim_eval_sizes, zeroed by lsim_eval_clear */
    void* state;                      /* 16-byte aligned */
    int64_t* table;                   /* [num_groups, LSIM_EVAL_WORDS] */
    float* trace;                     /* [trace_capacity, num_trace_envs, LSIM_EVAL_TRACE_DIM] or NULL when num_trace_envs == 0 */
    int32_t num_envs, num_robots, num_types, num_levels;
    uint32_t group_by;                /* LSIM_EVAL_BY_* bits */
    int32_t num_groups;               /* must equal the product of the kept extents */
    int32_t num_trace_envs, trace_capacity;
    int32_t feet_bodies[LSIM_NUM_LEGS];                 /* rows of contact_forces */
    int32_t trace_envs[LSIM_EVAL_MAX_TRACE_ENVS];       /* host-side list: checked (< num_envs) before any launch */
} lsim_eval;
/* bytes of state / table / trace.  LSIM_E_INVALID: num_envs < 1, num_groups < 1 or > LSIM_EVAL_MAX_GROUPS, num_trace_envs < 0 or
 * > LSIM_EVAL_MAX_TRACE_ENVS, trace_capacity < 1, a NULL output pointer. */
int lsim_eval_sizes(int64_t num_envs, int num_groups, int num_trace_envs, int trace_capacity, size_t* state_bytes, size_t* table_bytes,
                    size_t* trace_bytes);
/* zero state, table and trace (three memsets on the stream): no group latched, launch counter 0 */
int lsim_eval_clear(const lsim_eval* e, void* stream);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch: e == NULL, a NULL or misaligned pointer (robot_ids may be
 * NULL; trace may be NULL only when num_trace_envs == 0), num_envs < 1, num_robots outside 1..LSIM_MAX_ROBOTS, num_types outside
 * 1..LSIM_TERRAIN_TYPES_MAX, num_levels outside 1..LSIM_TERRAIN_LEVELS_MAX, group_by with unknown bits, num_groups != product of the kept
 * extents, num_trace_envs outside 0..LSIM_EVAL_MAX_TRACE_ENVS, trace_capacity < 1, a trace env or a feet body out of range. */
int lsim_eval_accumulate(const lsim_eval* e, void* stream);

/* ---- caller-supplied per-env columns into the evaluator's groups: what lsim_eval's fixed metric set does not hold (a vision policy's
 * depth influence, its encoder's scan error, ...), accumulated under the same guarantees -- 2^-32 fixed-point int64 words, integer atomics
 * only, bitwise reproducible, ONE launch, no host synchronisation, no floating-point atomic anywhere.
 *
 * One lsim_eval_columns_accumulate launch, per env e:
 *   e contributes only if reset_buf[e] == 0, its latched group g1 = group1[e] of `state` (group + 1; 0: none latched yet) is non-zero and
 *   g1 - 1 < num_groups; otherwise nothing is written for it.  A contributing env adds to row g1 - 1 of `table`:
 *     word 0 += 1
 *     for column k, v = values[e * ld + k]:   v finite     -> sum_k += fix(v), sq_k += fix(v * v)     (the product is ONE fp32 multiply; fix is
 *                                                             lsim_eval's, clamp to +-2^20 included, so an overflowing square adds the clamp)
 *                                             v not finite -> nonfinite_k += 1 and nothing else
 *   Row layout: [samples | sum_0, sq_0, nonfinite_0 | sum_1, sq_1, nonfinite_1 | ...], 1 + LSIM_EVAL_COL_WORDS * num_cols words.
 * Ordering: the launch goes AFTER lsim_eval_accumulate of the same env-step, on the same stream (that launch latches the groups).  Launched once
 * per lsim_eval_accumulate from the first one on, word 0 equals the main table's SAMPLES word group by group.  The launch reads `state` and
 * never writes it; the evaluator's launch counter stays lsim_eval_accumulate's.  Before the first lsim_eval_accumulate no group is latched and
 * the launch adds nothing. */
#define LSIM_EVAL_MAX_COLUMNS 6
#define LSIM_EVAL_COL_WORDS 3     /* per column: sum, sum of squares, non-finite count */
typedef struct lsim_eval_columns {
    const void* state;            /* the lsim_eval.state whose latched groups are used; READ ONLY here; 16-byte aligned */
    const uint8_t* reset_buf;     /* [N], the one the evaluator reads */
    const float* values;          /* [N, ld] fp32, 4-byte aligned */
    int64_t* table;               /* [num_groups, 1 + 3 * num_cols] int64, 8-byte aligned */
    int64_t num_envs;             /* the evaluator's */
    int32_t num_groups, num_cols, ld;   /* 1 <= num_cols <= LSIM_EVAL_MAX_COLUMNS, ld >= num_cols */
} lsim_eval_columns;
/* bytes of the table.  LSIM_E_INVALID: num_groups outside 1..LSIM_EVAL_MAX_GROUPS, num_cols outside 1..LSIM_EVAL_MAX_COLUMNS, a NULL output pointer. */
int lsim_eval_columns_sizes(int num_groups, int num_cols, size_t* table_bytes);
/* zero the table (one memset on the stream); the argument checks of lsim_eval_columns_accumulate */
int lsim_eval_columns_clear(const lsim_eval_columns* c, void* stream);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch: c == NULL, a NULL or misaligned pointer, num_envs outside
 * what lsim_eval_sizes accepts, num_groups outside 1..LSIM_EVAL_MAX_GROUPS, num_cols outside 1..LSIM_EVAL_MAX_COLUMNS, ld < num_cols. */
int lsim_eval_columns_accumulate(const lsim_eval_columns* c, void* stream);

/* ---- range sensors: rays against the terrain mesh (depth cameras, lidar; no reference FFI: the reference has no such sensor).
 * ONE launch, on the caller's stream, no host synchronisation, capturable in a graph.  The launch only READS the simulator's buffers,
 * through raw device pointers (this struct, filled by the caller from lsim_get_buffer and the terrain constants of its lsim_config).
 * lsim_raycast sees ONLY THE TERRAIN; lsim_raycast_bodies (below) adds the collision shapes of the env's OWN robot.  Other envs' robots are never seen.
 *
 * Geometry -- the mesh the contact code collides with (LSIM_BUF_TERRAIN_MESH, word[a][b] of grid vertex (a, b)):
 *   vertex (a, b) = ( (a + dx) * horizontal_scale - border_size, (b + dy) * horizontal_scale - border_size, (int16)(word & 0xFFFF) * vertical_scale ),
 *                   dx = ((word >> 16) & 3) - 1, dy = ((word >> 18) & 3) - 1
 *   cell (i, j), 0 <= i <= grid_rows - 2, 0 <= j <= grid_cols - 2, has the two triangles (p00, p11, p01) and (p00, p10, p11), pab = vertex (i + a, j + b).
 *   A triangle (a, b, c) with |(b - a) x (c - a)|^2 < 1e-16 does not exist.  mesh_type 1 (heightfield): the same words, dx = dy = 0 in all of them.
 *   mesh_type 0 (plane), or mesh == NULL: the single unbounded plane z = 0.
 *   Bits 20 and 24-31 of a word only speed the walk up and never change a result: bit 20 clear = no vertex of the 4 x 4 vertex block
 *   (i-1..i+2, j-1..j+2) is displaced; bits 24-31 = dz: no vertex of that block is higher than (height + dz * 4) height steps, 255 = unknown.
 * Ray r of env e:  o = p + R(q) * mount_pos[e],  d = R(q) * R(mount_quat[e]) * dirs[r],  (p, q) = root_states[e][0:3], [3:7] (quaternion xyzw, used as
 *   given: the caller keeps it and dirs[r] of unit length; R(q) v = v + 2 w (u x v) + 2 u x (u x v), u = q.xyz, w = q.w).
 * Result: the smallest t in [near, far] for which o + t d lies on a triangle, from EITHER side of it (the walls that displacement makes are seen
 *   from both sides); `far` when there is none -- also when the ray never meets the grid's footprint [0, (rows-1) hs] x [0, (cols-1) hs] - border.
 *   A ray (nearly) parallel to a triangle's plane, |n . d| < 1e-30 for the unnormalised n, does not hit that triangle.
 *   Edges are inclusive.  With U, V, W the three edge functions of the triangle (U = -e2 . (s x d), V = e1 . (s x d), W = n . d - U - V for
 *   e1 = b - a, e2 = c - a, s = o - a, n = e1 x e2, all three multiplied by sign(n . d)), the ray is inside when U >= -E2, V >= -E1 and
 *   W >= -(E1 + E2 + E3), Ek = 2^-18 * max|component of ek| * max|component of s|, E3 = 2^-20 * max|component of e1| * max|component of e2| (the
 *   rounding of n . d): Ek is 4-8 times the rounding error of the fp32 edge function (six products of three factors each), so two triangles
 *   that share an edge cannot both reject a ray that passes between them.  It admits a
 *   ray that passes OUTSIDE an edge by at most 2^-18 * sqrt(3) * |o - a| / sin(angle between ray and edge), 3.3e-5 m at 5 m: less than the position
 *   uncertainty of a world coordinate 190 m from the origin that the tests allow for (6e-5 m), so a ray reported as a hit is a hit for a ray within that.
 *   out[e][r] = t * scale[r] (scale == NULL: t); a miss is far * scale[r].  scale[r] = cos(angle of dirs[r] to the optical axis) turns range into
 *   the z-depth a depth camera reports.
 *   A non-finite component of o or d: out = far * scale[r], and the ray is counted in state[0] (int64, cumulative, the caller may zero it; it must
 *   stay 0, as LSIM_BUF_NONFINITE).  No NaN is ever written (a non-finite scale is the caller's).
 *   Envs: e = 0, env_stride, 2 env_stride, ...; the other rows of `out` are not touched.
 * NOT SUPPORTED: an origin below the surface.  The mesh is a displaced height grid without overhangs; a ray that starts under it reports the first
 *   face it meets from below, which means nothing. */
#define LSIM_RAYCAST_MAX_RAYS 16384        /* rays per env: a 128 x 128 image; 64 x 48 = 3072, a 16 x 360 lidar = 5760 */
#define LSIM_RAYCAST_STATE_WORDS 4         /* int64: [0] non-finite rays; [1] reserved; [2] cells walked, [3] triangles tested (only a build with LS_RAYCAST_COUNTERS writes [2], [3], and from lsim_raycast_bodies [1] = primitives that passed the bounding test) */
typedef struct lsim_raycast {
    const float* root_states;         /* [N,13] simulator buffer, read only */
    const int32_t* mesh;              /* LSIM_BUF_TERRAIN_MESH [grid_rows,grid_cols], or NULL (plane) */
    const float* mount;               /* [N,7] sensor pose in the base frame: position, quaternion xyzw */
    const float* dirs;                /* [R,3] unit vectors in the sensor frame, shared by all envs */
    const float* scale;               /* [R] or NULL */
    float* out;                       /* [N,out_stride], 16-byte aligned; row e holds R values */
    void* state;                      /* LSIM_RAYCAST_STATE_WORDS int64, 8-byte aligned, zeroed by the caller */
    int32_t num_envs, num_rays;       /* N >= 1, R in 1..LSIM_RAYCAST_MAX_RAYS */
    int32_t env_stride;               /* >= 1 */
    int32_t out_stride;               /* floats between rows of out: >= R, a multiple of 4 (16-byte aligned rows) */
    int32_t mesh_type, grid_rows, grid_cols;      /* lsim_config's; grid extents >= 2 unless plane */
    float horizontal_scale, vertical_scale, border_size;
    float near, far;                  /* 0 <= near < far, far finite */
} lsim_raycast_t;    /* the struct tag and the entry point share the name; C and C++ code names the type lsim_raycast_t */
/* bytes of `state`.  LSIM_E_INVALID: a NULL output pointer */
int lsim_raycast_sizes(size_t* state_bytes);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch: rc == NULL; root_states, mount, dirs, out or state NULL;
 * a pointer not aligned to its element (out: 16 bytes, state: 8); mesh NULL with mesh_type != 0; N < 1; R outside 1..LSIM_RAYCAST_MAX_RAYS;
 * env_stride < 1; out_stride < R or not a multiple of 4; mesh_type outside 0..2; grid_rows or grid_cols < 2 for a mesh; horizontal_scale or
 * vertical_scale not finite and > 0, border_size not finite (mesh only); near < 0, near >= far, far not finite. */
int lsim_raycast(const lsim_raycast_t* rc, void* stream);

/* ---- range sensors that also see the robot: the terrain of lsim_raycast plus the articulated collision primitives of the env's OWN robot.
 * ONE launch, same rules as lsim_raycast (caller's stream, no host synchronisation, capturable, read-only on the simulator's buffers).
 * NOT SUPPORTED: the robots of other envs (they share terrain tiles without colliding; a sensor never sees them).
 *
 * Everything lsim_raycast_t says holds for `rc` (terrain geometry, near / far / scale, misses, the non-finite rule and state[0], env_stride), with
 * these additions.
 * Sensor frame.  flags == 0: as lsim_raycast, o = p + R(q) mount_pos[e], d = R(q) R(mount_quat[e]) dirs[r].  LSIM_RAYCAST_FRAME_YAW: the same two
 *   formulas with q replaced by qy = (0, 0, q.z, q.w) / sqrt(q.z^2 + q.w^2) (the base's position and yaw only: a gimbal or chase camera; a base with
 *   q.z = q.w = 0 makes the pose non-finite).  Body poses below ALWAYS use the full q.
 * Robot.  k = env_robot[e] (NULL: 0) selects robots[k], 0 <= k < num_robots.  A robot is 17 bodies in the order and tree of lsim_robot_model
 *   (body 0 the base; leg l = 0..3 has hip 1 + 4l, thigh 2 + 4l, calf 3 + 4l, foot 4 + 4l, each the child of the one before, the hip of body 0)
 *   and num_prims primitives.  Forward kinematics, from root_states[e][0:7] and th_j = dof_state[e][j][0] ONLY (rigid_body_states is not read:
 *   after the post-step reset root and joint state are the consistent pair), in coordinates RELATIVE TO THE BASE POSITION p:
 *     body 0:  P_0 = 0, Q_0 = q.      body b > 0 with parent a:  P_b = P_a + R(Q_a) joint_pos_b,
 *     Q_b = Q_a * (joint_axis_b sin(th/2), cos(th/2)), th = th_dof_b, or 0 when dof_b < 0 (the fixed feet);  (a * b: R(a * b) = R(a) R(b), xyzw).
 *   Primitive i on body b:  centre C_i = P_b + R(Q_b) pos_i,  axes = the columns of R(Q_b * quat_i)  (pos, quat: the primitive's pose in the body frame).
 * Primitives are convex solids, in their own frame (centre at 0):
 *     LSIM_RAYCAST_PRIM_SPHERE    size[0] = r:               |x| <= r
 *     LSIM_RAYCAST_PRIM_BOX       size = half extents:       |x_k| <= size[k]
 *     LSIM_RAYCAST_PRIM_CAPSULE   size[0] = r, size[1] = h:  distance to the segment (0, 0, -h)..(0, 0, h) <= r
 *     LSIM_RAYCAST_PRIM_CYLINDER  size[0] = r, size[1] = h:  x^2 + y^2 <= r^2 and |z| <= h        (flat caps)
 * Body test, carried out in the base-relative coordinates: the ray is o' + t d with o' = o - p = R(q or qy) mount_pos[e] -- small, and exact to
 *   rounding wherever the env stands, so the accuracy of a body hit does not depend on the env's distance from the world origin (the test
 *   tolerances rest on this: a body hit is judged at the coordinate magnitude of this frame, under a metre).  The set of t with o' + t d inside
 *   primitive i is an interval [t_in, t_out] (the whole line counts, t may be negative) or empty.  The primitive contributes t_in -- its FRONT
 *   face -- if near <= t_in <= far, and nothing otherwise: a ray that starts inside a primitive, or enters it before `near`, passes out of it
 *   freely (a camera may sit inside the trunk box).  Only primitives whose body b has bit b of body_mask set are seen.
 * Result: t = min(terrain result of lsim_raycast, the contributed t_in of every seen primitive); out[e][r] = t * scale[r], far * scale[r] for a miss.
 *   A non-finite component of o, d or of any of the twelve th_j of the env: out = far * scale[r], label 0, the ray is counted in state[0].
 *   With num_prims == 0 for the env's robot, or body_mask == 0, and flags == 0, `out` is lsim_raycast's bit for bit.
 * labels (may be NULL): labels[e][r] (uint8, label_stride bytes between rows) = 0: the result is `far` and no body gave it; 1: terrain, t < far;
 *   2 + b: body b.  When a body's t_in equals the terrain's t the body wins; between bodies the primitive earlier in the table wins.  (Terrain met
 *   exactly at t == far is the value of a miss and is labelled 0.) */
#define LSIM_RAYCAST_MAX_PRIMS 48          /* primitives per robot (Aliengo: 29) */
#define LSIM_RAYCAST_PRIM_SPHERE 0
#define LSIM_RAYCAST_PRIM_BOX 1
#define LSIM_RAYCAST_PRIM_CAPSULE 2
#define LSIM_RAYCAST_PRIM_CYLINDER 3
#define LSIM_RAYCAST_FRAME_YAW 1u          /* flags: the sensor frame follows the base's position and yaw only */
typedef struct lsim_raycast_prim {
    int32_t kind, body;               /* LSIM_RAYCAST_PRIM_*, 0..LSIM_NUM_BODIES-1 */
    float pos[3];                     /* centre in the body frame */
    float quat[4];                    /* orientation in the body frame, xyzw, unit */
    float size[3];                    /* per kind, above; unused entries 0 */
} lsim_raycast_prim;
typedef struct lsim_raycast_body {    /* the four kinematic fields of lsim_body */
    float joint_pos[3];
    float joint_axis[3];
    int32_t parent, dof;
} lsim_raycast_body;
typedef struct lsim_raycast_robot {
    lsim_raycast_body bodies[LSIM_NUM_BODIES];
    int32_t num_prims;                /* 0..LSIM_RAYCAST_MAX_PRIMS */
    int32_t pad[3];
    lsim_raycast_prim prims[LSIM_RAYCAST_MAX_PRIMS];
} lsim_raycast_robot;
typedef struct lsim_raycast_bodies {
    lsim_raycast_t rc;                /* as for lsim_raycast */
    const float* dof_state;           /* [N,12,2] simulator buffer, read only */
    const uint8_t* env_robot;         /* [N] robot index per env, or NULL: robot 0 */
    const lsim_raycast_robot* robots; /* [num_robots] DEVICE memory: what the launch reads */
    const lsim_raycast_robot* robots_host;  /* the same bytes in HOST memory: what the argument check reads (a launch replayed from a graph checks nothing) */
    uint8_t* labels;                  /* [N,label_stride] or NULL */
    int32_t num_robots;               /* 1..LSIM_MAX_ROBOTS; 1 when env_robot == NULL */
    int32_t label_stride;             /* bytes between rows of labels: >= R (ignored when labels == NULL) */
    uint32_t body_mask;               /* bit b: body b is seen */
    uint32_t flags;                   /* LSIM_RAYCAST_FRAME_YAW or 0 */
} lsim_raycast_bodies_t;
/* bytes of `state` (lsim_raycast's) and of one lsim_raycast_robot.  LSIM_E_INVALID: a NULL output pointer */
int lsim_raycast_bodies_sizes(size_t* state_bytes, size_t* robot_bytes);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch: rb == NULL; anything lsim_raycast refuses in rb->rc;
 * dof_state, robots or robots_host NULL or not 4-byte aligned; num_robots outside 1..LSIM_MAX_ROBOTS, or != 1 with env_robot == NULL (a table of
 * several robots without the table of which env runs which); labels != NULL with label_stride < R; a flag bit other than LSIM_RAYCAST_FRAME_YAW;
 * and in robots_host[0..num_robots): num_prims outside 0..LSIM_RAYCAST_MAX_PRIMS; a body whose parent / dof is not the tree's above (dof: -1 or
 * 0..11) or whose joint_pos / joint_axis is not finite; a primitive with kind outside 0..3, body outside 0..16, a non-finite pos or quat, or a
 * size entry it uses (sphere 1, box 3, capsule / cylinder 2) that is not finite and > 0. */
int lsim_raycast_bodies(const lsim_raycast_bodies_t* rb, void* stream);

/* ---- shaded frames: what turns the range and the label of lsim_raycast_bodies into a picture -- the surface normal at every hit, whether
 * the sun reaches that point, and a colour.  ONE launch under the rules of lsim_raycast_bodies (caller's stream, no host synchronisation, raw
 * pointers only, capturable in a graph, read-only on the simulator's buffers), enqueued BEHIND an lsim_raycast_bodies of the same `rb` on
 * the same stream: it reads what that launch wrote, rb.rc.out and rb.labels (required), visits the same envs e = 0, env_stride, ... and
 * writes rgba, surface and state[0] only.  Other envs' robots are neither drawn nor do they cast shadows.  All arithmetic in fp32.
 *
 * Per pixel r of a visited env e:
 *   1. Ray.  o, o' = R(q or qy) mount_pos[e] and d exactly as lsim_raycast_bodies forms them (the yaw frame under LSIM_RAYCAST_FRAME_YAW).
 *      A non-finite component of o or d, or of any of the env's twelve joint positions: the pixel is SKY (step 6) and counted in
 *      rb.rc.state[0] (so a bad env counts once in the ray launch and once here).  L = labels[e][r]; L == 0 or L > 1 + LSIM_NUM_BODIES: SKY.
 *   2. Range.  t0 = out[e][r] / scale[r] (scale == NULL: out[e][r]).
 *   3. Terrain, L == 1.  mesh_type 0 or mesh == NULL: t = t0, m = (0, 0, 1).  Otherwise the cell (i, j) of P0 = o + t0 d,
 *        i = clamp(floor((P0.x + border_size) / horizontal_scale), 0, grid_rows - 2), j likewise from P0.y and grid_cols;
 *      over the cells (i - 1 + c / 3, j - 1 + c % 3), c = 0..8, that exist, and in each its two triangles in the order of lsim_raycast,
 *      the FIRST triangle whose own intersection value t_k with this ray (lsim_raycast's triangle rule with near = rc.near and no upper
 *      bound) minimises |t_k - t0| is the face of the hit: t = t_k, m = e1 x e2 of that triangle (the walk found its hit among these
 *      triangles from the same o and d, so t_k reproduces the walk's value; t0 differs from it by the rounding of the scale only).
 *      No triangle of the nine cells met: t = t0, m = (0, 0, 1).  n = m / |m|, negated when m . d > 0 (turned against the ray).
 *      P = o + t d.
 *   4. Body, L == 2 + b.  Among the SEEN primitives of body b, in table order, the first whose t_in for the ray o' + t d (the
 *      primitive's interval of lsim_raycast_bodies) minimises |t_in - t0|: t = t_in; none: SKY.  With x = the hit point in the
 *      primitive's frame (centre at 0), its OUTWARD normal there, n_l:
 *        sphere    x / |x|
 *        box       the axis k with the largest |x_k| - size[k] (the first on ties; the face of the entered slab): sign(x_k) e_k
 *        cylinder  rho = sqrt(x_0^2 + x_1^2);  rho - r >= |x_2| - h: the side, (x_0, x_1, 0) / rho;  else the cap, (0, 0, sign(x_2))
 *        capsule   c = (0, 0, clamp(x_2, -h, h)), the nearest point of its segment: (x - c) / |x - c|
 *      n = n_l in world orientation (sum of n_l[k] times local axis k); it is not turned: a front face has n . d <= 0 up to rounding.
 *      P = o + t d and P' = o' + t d.
 *   5. Light.  c = n . sun.  light = 0 when c <= 0;  1 without LSIM_SHADE_SHADOWS;  otherwise 0 exactly when the shadow ray is occluded.
 *      The shadow ray has direction `sun` and runs over [0, shadow_far] from P + shadow_bias n (P' + shadow_bias n for the bodies).  It is
 *      occluded when lsim_raycast_bodies' body test with near = 0, far = shadow_far finds a contributing primitive (a seen primitive of
 *      the env's own robot whose FRONT face is met at 0 <= t_in <= shadow_far; a primitive the point lies inside contributes nothing),
 *      or when lsim_raycast's terrain result with near = 0, far = shadow_far is < shadow_far.  A pixel with c <= 0 casts no shadow ray.
 *   6. Colour.  k = ambient + (1 - ambient) * light * c.  The albedo is palette[L] = r | g << 8 | b << 16, each channel a_c = byte * (1 / 255).
 *      Terrain with checker > 0: g = k * checker_gain when (int) floor(P.x / checker) + (int) floor(P.y / checker) is odd (the checker
 *      is anchored in the world), else g = k.  Each channel of the pixel is (uint) floor(255 * min(max(a_c * g, 0), 1) + 0.5);
 *      rgba[e][r] = r | g << 8 | b << 16 | 255 << 24 and surface[e][r] = (n.x, n.y, n.z, light).
 *      SKY: rgba[e][r] = (palette[0] & 0xFFFFFF) | 255 << 24, surface[e][r] = (0, 0, 0, 0).  No NaN is ever written.
 * Two launches on the same inputs write the same bits (no atomic but the int64 count of state[0]).
 * NOT BUILT: textures, anti-aliasing, soft shadows, specular terms, visual meshes (the collision primitives are what is drawn), frames
 * above LSIM_RAYCAST_MAX_RAYS pixels. */
#define LSIM_SHADE_SHADOWS 1u              /* shade_flags: cast a shadow ray from every lit pixel */
typedef struct lsim_sensor_shade {
    lsim_raycast_bodies_t rb;         /* the struct lsim_raycast_bodies was launched with; labels != NULL */
    uint32_t* rgba;                   /* [N,rgba_stride] one word per pixel, 16-byte aligned */
    float* surface;                   /* [N,R,4] normal xyz and light, 16-byte aligned, or NULL */
    const uint32_t* palette;          /* [2 + LSIM_NUM_BODIES] rgb words by label: 0 the sky, 1 the terrain, 2 + b body b; 4-byte aligned */
    float sun[3];                     /* unit vector TOWARDS the sun, world frame, sun[2] > 0 */
    float ambient;                    /* 0..1 */
    float checker;                    /* metres, >= 0 (0: none) */
    float checker_gain;               /* factor on the darker squares: finite, >= 0 */
    float shadow_bias, shadow_far;    /* metres, finite, >= 0 */
    int32_t rgba_stride;              /* words between rows of rgba: >= R, a multiple of 4 */
    uint32_t shade_flags;             /* LSIM_SHADE_SHADOWS or 0 */
} lsim_sensor_shade_t;
/* bytes of rb.rc.state (lsim_raycast's) and of `palette`.  LSIM_E_INVALID: a NULL output pointer */
int lsim_sensor_shade_sizes(size_t* state_bytes, size_t* palette_bytes);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: ss == NULL; anything
 * lsim_raycast_bodies refuses in ss->rb; rb.labels == NULL; rgba NULL or not 16-byte aligned; surface given and not 16-byte aligned;
 * palette NULL or not 4-byte aligned; rgba_stride < R or not a multiple of 4; a component of sun not finite, | |sun|^2 - 1 | > 1e-3 or
 * sun[2] <= 0; ambient outside [0, 1] (or NaN); checker, checker_gain, shadow_bias or shadow_far negative or not finite; a bit of
 * shade_flags other than LSIM_SHADE_SHADOWS. */
int lsim_sensor_shade(const lsim_sensor_shade_t* ss, void* stream);

/* ---- sensor model: a range sensor as a real instrument -- an update period, latency, a short history of frames, noise, dropout, clipping.
 * ONE launch, same rules as lsim_raycast_bodies (caller's stream, no host synchronisation, read-only on the simulator's buffers).  The launch
 * renders only the envs that are DUE, runs each of their rays through the model and maintains hist, a per-env ring of the last K captures.
 *
 * Rays.  `rb` is read exactly as lsim_raycast_bodies reads it, and `raw`, the value of ray r of env e, is the value lsim_raycast_bodies writes
 *   to out[e][r], bit for bit, with its label.  TERRAIN-ONLY FORM: rb.robots == NULL with rb.num_robots == 0 and rb.flags == 0 -- then dof_state,
 *   env_robot, robots_host and body_mask are not read, raw is the value lsim_raycast(&rb.rc) writes, bit for bit, and a label (labels may still
 *   be given) is 1 for t < far and 0 otherwise.
 * Which envs.  Env e is visited when e % rb.rc.env_stride == 0, as before.  For a visited env
 *     fill = (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0          (the env was reset since its last step: LSIM_BUF_EPISODE_LENGTH)
 *     due  = fill || ( !(flags & LSIM_SENSOR_RESETS_ONLY) && (tick + (stagger ? e : 0)) % period == 0 )
 *   For an env that is NOT due NOTHING is written: not its row of rb.rc.out, not its labels, not its rows of hist.  (state[0] counts only rays
 *   of due envs.)  stagger spreads the captures over the period, 1 env in `period` per launch; without it all envs capture on the same ticks.
 * Per ray r of a due env, all arithmetic in fp32 (a compiler may contract a product and a sum into one fused operation):
 *     rb.rc.out[e][r] = raw, the label as before: `out` stays the CLEAN value (a privileged target);
 *     hit = (t < far) for the unscaled t of the ray: a miss, and a non-finite ray (counted in state[0], as before), carries no noise and is never dropped;
 *     x0..x3 = Philox4x32-10, key (seed, rank), counter (e, (uint32_t)tick, LSIM_RNG_SENSOR, (stream_id << 16) | r);   u_k = (x_k >> 8) * 2^-24;
 *     g = 2 * ((u0 + u1 + u2) - 1.5f), summed left to right: a bounded three-uniform stand-in for a unit normal -- mean 0, variance exactly 1,
 *         |g| <= 3, no transcendental function, so the same bits on every host;
 *     v = hit ? raw + (sigma0 + sigma2 * raw * raw) * g : raw          (noise that grows with the square of the depth, as a stereo camera's)
 *     if (hit && u3 < p_drop) v = drop_value                            (a hole)
 *     v = min(max(v, clip_lo), clip_hi);      y = (v - offset) * gain
 *   and the history, K = latency + frames slots per env, oldest first:
 *     fill:       hist[e][k][r] = y for every k < K                    (an episode never starts with frames of the previous one)
 *     otherwise:  hist[e][k][r] = hist[e][k + 1][r] for k = 0 .. K - 2 in this order, then hist[e][K - 1][r] = y.
 *   hist[e][0 .. frames) is what a policy reads: `frames` consecutive captures, oldest first, the newest of them (slot frames - 1) `latency`
 *   captures old; slots frames .. K - 1 are the captures still on their way.  Age is counted in captures of the env, not in ticks.
 * tick is passed BY VALUE, as the simulator's step word is: a launch replayed from a captured graph repeats its due set and its draws.  A caller
 *   that captures the launch captures one graph per tick of a period, or launches the sensor outside the graph. */
#define LSIM_SENSOR_MAX_HISTORY 8
#define LSIM_SENSOR_FILL_ALL 1u            /* flags: every visited env is due and its whole history is filled */
#define LSIM_SENSOR_RESETS_ONLY 2u         /* flags: only envs with episode_length == 0 are due (a by-hand reset between two steps) */
typedef struct lsim_sensor_model {
    lsim_raycast_bodies_t rb;         /* as for lsim_raycast_bodies; rb.robots == NULL with num_robots == 0 and rb.flags == 0: terrain only */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    float* hist;                      /* [N, K, hist_stride], K = latency + frames, 16-byte aligned */
    int64_t tick;                     /* >= 0: the caller's step counter, by value */
    uint32_t seed, rank, stream_id;   /* Philox key; stream_id < 65536 separates the sensors of one env */
    int32_t period, stagger;          /* period >= 1; stagger 0 / 1 */
    int32_t latency, frames;          /* latency >= 0, frames >= 1, latency + frames <= LSIM_SENSOR_MAX_HISTORY */
    int32_t hist_stride;              /* floats between slots of hist: >= R, a multiple of 4 */
    float sigma0, sigma2;             /* finite, >= 0 */
    float p_drop, drop_value;         /* 0 <= p_drop <= 1; drop_value finite */
    float clip_lo, clip_hi;           /* finite, clip_lo <= clip_hi */
    float offset, gain;               /* finite */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
} lsim_sensor_model_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch: sm == NULL; anything lsim_raycast_bodies refuses in sm->rb
 * (terrain-only form: anything lsim_raycast refuses in sm->rb.rc, labels != NULL with label_stride < R; robots == NULL with num_robots != 0 or
 * rb.flags != 0 is not that form and is refused); episode_length NULL or not 8-byte aligned; hist NULL or not 16-byte aligned; tick < 0;
 * stream_id >= 65536; period < 1; stagger outside 0..1; latency < 0; frames < 1; latency + frames > LSIM_SENSOR_MAX_HISTORY; hist_stride < R or
 * not a multiple of 4; sigma0, sigma2 not finite or < 0; p_drop outside [0, 1]; drop_value, clip_lo, clip_hi, offset or gain not finite;
 * clip_lo > clip_hi; a flag bit other than the two above; both of them set. */
int lsim_sensor_capture(const lsim_sensor_model_t* sm, void* stream);

/* ---- sensor mount jitter: where the instrument sits, redrawn for every env that starts an episode.  ONE launch, the rules of
 * lsim_sensor_capture (caller's stream, no host synchronisation, raw pointers only).  It reads `nominal` and episode_length and writes rows of
 * `mount` -- the array a sensor's lsim_raycast_t.mount points at, so a capture enqueued BEHIND it on the same stream renders a reset env, whole
 * history included, from its new pose.  No capture kernel changes: they read the mount through the pointer they already have.
 *
 * Which envs.  Env e is visited when e % env_stride == 0.  A visited env is FRESH when
 *     (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0                  (lsim_sensor_capture's `fill`; the tick plays no part in it)
 *   LSIM_SENSOR_RESETS_ONLY is accepted and changes nothing here.  For an env that is not visited or not fresh NOTHING is written.
 * Draws.  Two Philox4x32-10 blocks, key (seed, rank), counters (e, (uint32_t)tick, LSIM_RNG_SENSOR_MOUNT, (stream_id << 16) | b), b = 0, 1:
 *     x0..x3 = block 0, x4..x7 = block 1;   u_k = (x_k >> 8) * 2^-24,   s_k = 2 u_k - 1   for k = 0..5 (exact in fp32); x6, x7 are not used.
 *   The draw depends on (e, tick, stream_id) and the key only: a second launch on the same tick writes the same bits (reset_idx() by hand, then
 *   the step that shares its tick).
 * Per fresh env, all arithmetic in fp32 (a compiler may contract a product and a sum into one fused operation), n = nominal[e], m = mount[e]:
 *     m[k] = n[k] + s_k * pos_range[k],  k = 0..2                              (metres along the base x, y, z)
 *     a_k = s_{3+k} * rot_range[k];   h_k = 0.5 * a_k;   c = 1 / sqrt(1 + (h_0^2 + h_1^2 + h_2^2))     (square root and division correctly rounded)
 *     d = (h_0 c, h_1 c, h_2 c, c)  xyzw: the Cayley map of a -- no transcendental function, so the same on every host.  Its rotation angle is
 *         2 atan(|a| / 2): |a| to third order, 0.25 % short at 10 degrees, and never more than 2 atan(|rot_range| / 2);
 *     m[3..6] = d (x) n[3..6],  the Hamilton product, R(m) = R(d) R(n):
 *         m3 = d.w n.x + n.w d.x + (d.y n.z - d.z n.y),   m4 = d.w n.y + n.w d.y + (d.z n.x - d.x n.z),
 *         m5 = d.w n.z + n.w d.z + (d.x n.y - d.y n.x),   m6 = d.w n.w - (d.x n.x + d.y n.y + d.z n.z)
 *   The error turns about the BASE axes (rot_range[1] is the pitch error of a forward camera) and is not renormalised: |m_quat| = |n_quat| up
 *   to rounding.  All-zero ranges give d = (0, 0, 0, 1) and m = n exactly (a component -0 may come out as +0).
 * tick is passed by value as lsim_sensor_capture's is, and replays from a captured graph in the same way. */
typedef struct lsim_sensor_mount_jitter {
    const float* nominal;             /* [N, 7] position + quaternion xyzw, as lsim_raycast_t.mount; read only, 4-byte aligned */
    float* mount;                     /* [N, 7] what the sensor's lsim_raycast_t.mount points at; 4-byte aligned; must not be `nominal` */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    int64_t tick;                     /* >= 0, by value: the tick of the capture that follows */
    uint32_t seed, rank, stream_id;   /* as lsim_sensor_model_t's; stream_id < 65536 */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
    int32_t num_envs, env_stride;     /* N >= 1; every env_stride-th env is visited (>= 1) */
    float pos_range[3];               /* metres, half-widths along the base x, y, z: finite, >= 0 */
    float rot_range[3];               /* radians, half-widths about the base x, y, z: finite, >= 0 */
} lsim_sensor_mount_jitter_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: mj == NULL; nominal or mount NULL or not
 * 4-byte aligned; episode_length NULL or not 8-byte aligned; mount == nominal; num_envs < 1; env_stride < 1; tick < 0; stream_id >= 65536; a
 * pos_range or rot_range entry that is negative or not finite; a flag bit other than the sensor model's two; both of them set. */
int lsim_sensor_mount_jitter(const lsim_sensor_mount_jitter_t* mj, void* stream);

/* ---- sensor instrument error: the instrument's own constants -- latency, noise level, depth-scale error, field of view -- redrawn for every
 * env that starts an episode, and the capture that reads them.  TWO entries, each ONE launch under the rules of lsim_sensor_capture (caller's
 * stream, no host synchronisation, raw pointers only): lsim_sensor_instrument writes rows of `inst`, and lsim_sensor_capture_inst, enqueued
 * BEHIND it on the same stream, is lsim_sensor_capture with the row of each env in place of the shared constants.  lsim_sensor_capture itself,
 * its kernel and lsim_sensor_model_t do not change: the rows come through the new entry's own argument.
 *
 * The row.  inst[e] is 8 floats, rows 32 bytes apart:   { lat, noise_gain, depth_scale, depth_quad, tan_scale, 0, 0, 0 }
 *   lat: the env's latency in captures, an integer held in a float; noise_gain: a factor on the model's noise; depth_scale (no unit) and
 *   depth_quad (1/m): the relative depth error depth_scale + depth_quad * d of a hit at reported depth d (a focal / baseline miscalibration
 *   gives an error proportional to d, a disparity offset one proportional to d^2); tan_scale: the factor on the tangent of every ray's angle
 *   to the optical axis (the sensor frame's +x), 1 / (relative focal-length error).  The three zeros are reserved and written as zeros.
 *   The NEUTRAL row { sm.latency, 1, 0, 0, 1, 0, 0, 0 } makes lsim_sensor_capture_inst write the bits lsim_sensor_capture writes.
 *
 * lsim_sensor_instrument.
 * Which envs.  Env e is visited when e % env_stride == 0.  A visited env is FRESH when
 *     (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0                  (lsim_sensor_capture's `fill`; the tick plays no part in it)
 *   LSIM_SENSOR_RESETS_ONLY is accepted and changes nothing here.  For an env that is not visited or not fresh NOTHING is written.
 * Draws.  Two Philox4x32-10 blocks, key (seed, rank), counters (e, (uint32_t)tick, LSIM_RNG_SENSOR_INSTRUMENT, (stream_id << 16) | b), b = 0, 1:
 *     x0..x3 = block 0, x4..x7 = block 1;   u_k = (x_k >> 8) * 2^-24  for k = 0..4 (exact in fp32); x5, x6, x7 are not used.
 *   The draw depends on (e, tick, stream_id) and the key only: a second launch on the same tick writes the same bits.
 * Per fresh env, all arithmetic in fp32 (a compiler may contract a product and a sum into one fused operation):
 *     span = lat_hi - lat_lo;   j = min(span, (int) floor(u_0 * (float)(span + 1)));   lat = (float)(lat_hi - j)
 *         (uniform on the integers lat_lo .. lat_hi: u_0 (span + 1) < span + 1 before rounding, and the min takes a product rounded up to span + 1)
 *     noise_gain  = gain_lo + u_1 * (gain_hi - gain_lo)
 *     depth_scale = (2 u_2 - 1) * scale_range                                   (2 u - 1 is exact)
 *     depth_quad  = (2 u_3 - 1) * quad_range
 *     tan_scale   = 1 + (2 u_4 - 1) * fov_range
 *   Zero ranges (lat_lo = lat_hi, gain_lo = gain_hi = 1, the other three 0) give the row { lat_hi, 1, 0, 0, 1, 0, 0, 0 } exactly (a 0 may
 *   carry either sign).  The row is written as two 16-byte stores.
 * tick is passed by value as lsim_sensor_capture's is, and replays from a captured graph in the same way. */
typedef struct lsim_sensor_instrument {
    float* inst;                      /* [N, 8] the rows, 32-byte aligned */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    int64_t tick;                     /* >= 0, by value: the tick of the capture that follows */
    uint32_t seed, rank, stream_id;   /* as lsim_sensor_model_t's; stream_id < 65536 */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
    int32_t num_envs, env_stride;     /* N >= 1; every env_stride-th env is visited (>= 1) */
    int32_t lat_lo, lat_hi;           /* captures: 0 <= lat_lo <= lat_hi < LSIM_SENSOR_MAX_HISTORY */
    float gain_lo, gain_hi;           /* finite, 0 <= gain_lo <= gain_hi */
    float scale_range, quad_range;    /* half-widths of depth_scale (no unit) and depth_quad (1/m): finite, >= 0 */
    float fov_range;                  /* half-width of tan_scale about 1: finite, 0 <= fov_range < 1 */
} lsim_sensor_instrument_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: si == NULL; inst NULL or not 32-byte
 * aligned; episode_length NULL or not 8-byte aligned; num_envs < 1; env_stride < 1; tick < 0; stream_id >= 65536; lat_lo < 0; lat_lo > lat_hi;
 * lat_hi >= LSIM_SENSOR_MAX_HISTORY; gain_lo, gain_hi, scale_range, quad_range or fov_range negative or not finite; gain_lo > gain_hi;
 * fov_range >= 1; a flag bit other than the sensor model's two; both of them set. */
int lsim_sensor_instrument(const lsim_sensor_instrument_t* si, void* stream);

/* lsim_sensor_capture with per-env instrument rows: everything said of lsim_sensor_capture holds -- which envs are due, the rays, `raw`, the
 * clean `out` and the labels, the Philox block per ray at LSIM_RNG_SENSOR, dropout, clip, offset and gain, the layout of hist with its
 * K = sm->latency + sm->frames slots -- except for the three things below.  `inst` is the [N, 8] array above (here 16-byte alignment
 * suffices); a due env reads its own row { lat, noise_gain, depth_scale, depth_quad, tan_scale, .. } and an env that is not due reads none.
 * Field of view.  s = dirs[r], in the sensor frame, sc = scale ? scale[r] : 1.  If tan_scale != 1.0f and s.x > 0, with T = tan_scale:
 *     y' = s.y * T;   z' = s.z * T;   n = sqrt(s.x * s.x + y' * y' + z' * z')   (fp32 sum, left to right, possibly fused; the root correctly rounded)
 *     q = 1 / n   (correctly rounded);      s' = (s.x * q, y' * q, z' * q);      sc' = sc * q      (q itself when scale is NULL)
 *   and the ray is cast along s' and reported with sc' wherever lsim_sensor_capture uses s and sc: every tangent to the +x axis is multiplied
 *   by T, and for a z-depth camera (scale = the cosine to the axis) sc' is the new cosine.  Otherwise (tan_scale == 1.0f, or a ray with
 *   s.x <= 0, which has no finite tangent) s and sc are used untouched.  `out` and the labels are the clean values of the rays actually cast.
 * Calibration and noise, on a hit only, in place of lsim_sensor_capture's line for v (g, u3 as there):
 *     m = raw * (1 + (depth_scale + depth_quad * raw))                      (no operation of this line is fused with another: m is a rounded product)
 *     v = m + (noise_gain * (sigma0 + sigma2 * raw * raw)) * g
 *   then dropout, clip, offset and gain as there.  A miss and a non-finite ray report raw, as there.
 * Latency.  L = min(max((int) lat, 0), sm->latency);   Ke = L + sm->frames  (<= K):
 *     fill:       hist[e][k][r] = y for every k < K                              (as there)
 *     otherwise:  hist[e][k][r] = hist[e][k + 1][r] for k = 0 .. Ke - 2 in this order, then hist[e][k][r] = y for k = Ke - 1 .. K - 1.
 *   Slots 0 .. frames - 1, what a policy reads, are then L captures old; slots Ke .. K - 1 only ever hold the newest capture.  L = sm->latency
 *   is lsim_sensor_capture's shift.
 * LSIM_E_INVALID, checked on the host before any launch: everything lsim_sensor_capture refuses; inst NULL or not 16-byte aligned. */
int lsim_sensor_capture_inst(const lsim_sensor_model_t* sm, const float* inst, void* stream);

/* ---- stereo artefacts: what a stereo pair does to the image lsim_sensor_capture reports -- no depth where only one imager sees (occlusion
 * shadows), none below a minimum range, and depth edges that lose pixels or smear the foreground over the background.  ONE launch under the
 * rules of lsim_sensor_capture (caller's stream, no host synchronisation, raw pointers only, capturable in a graph).  Enqueued BEHIND a
 * capture on the same stream, with its tick, period, stagger, flags, episode_length, seed, rank and stream_id, it visits the same envs and
 * rewrites pixels of the history slots that capture just wrote.  It reads the clean depth rows (rb.rc.out of a z-depth camera), the labels
 * when there are any, episode_length and optionally the instrument rows; it reads and writes hist, adds to state, and writes nothing else.
 *
 * The image.  R = width * height pixels, r = row * width + c, rows top to bottom, columns left to right.  The image belongs to the LEFT
 *   imager; the second one sits `baseline` metres to its RIGHT.  fb = (focal length in pixels) * baseline, formed once on the host.
 * Which envs.  Env e is visited when e % env_stride == 0; fill and due are lsim_sensor_capture's, on the same fields.  For an env that is
 *   not due NOTHING is written.
 * Per pixel r of a due env, all arithmetic in fp32, every quotient correctly rounded, no two operations fused; the result is a function of
 * the stored bits of depth:
 *   1. Z = depth[e * depth_stride + r];   t = inv_scale ? Z * inv_scale[r] : Z
 *      valid = |Z| <= FLT_MAX  and  t_lo < t  and  t < t_hi  and  (labels == NULL or labels[e * label_stride + r] != 0)
 *      (lsim_elevation_map's rule for a range, with any label but "nothing")
 *   2. fbe = (inst && inst[8 e + 4] != 1.0f) ? fb / inst[8 e + 4] : fb            (the instrument's tan_scale shortens the focal length)
 *      delta = fbe / Z;      u = (float)c - delta        (the column at which the second imager sees the point)
 *   3. shadowed:  valid, and some column c' with c < c' <= min(width - 1, c + window) of the same row is valid and has u(c') <= u(c)
 *      (the second imager's ray to this pixel passes behind a nearer surface; a surface both imagers see keeps u strictly increasing along
 *      a row and casts nothing; a foreground object shadows the background on its LEFT side only)
 *   4. too near:  valid and delta > max_disparity                                 (such a pixel still occludes others)
 *   5. edge:  valid, not shadowed, not too near, and some valid pixel r' of the image within Chebyshev distance edge_radius of r has
 *      Z(r') < Z(r) * (1 - edge_rel)   (1 - edge_rel rounded, then the product rounded).  The pixel's FOREGROUND is the r' of smallest Z
 *      among those, on ties the smallest index r'.
 *   6. x0..x3 = Philox4x32-10, key (seed, rank), counter (e, (uint32_t)tick, LSIM_RNG_SENSOR_STEREO, (stream_id << 16) | r);  u0 = (x0 >> 8) * 2^-24
 *   7. HOLE when shadowed, or too near, or (edge and u0 < p_edge_hole);  else FATTEN when edge and u0 < p_edge_cum  (p_edge_cum is the fp32
 *      sum p_edge_hole + p_edge_fatten, formed on the host);  else the pixel is kept.
 *   8. a hole writes y_hole = (min(max(drop_value, clip_lo), clip_hi) - offset) * gain, what the capture writes for a dropped pixel;
 *      a fattened pixel writes the value the CAPTURE wrote to slot K - 1 of its foreground pixel, K = latency + frames -- whether this
 *      launch rewrites that foreground pixel too plays no part; a kept pixel writes nothing.  The value goes to the slots the capture
 *      wrote its y to:  every k < K under fill;  otherwise k = Ke - 1 .. K - 1, Ke = K without inst and
 *      Ke = min(max((int) inst[8 e], 0), latency) + frames with it (lsim_sensor_capture_inst's rule).
 *   9. state[0] += the holes written, state[1] += the fattened pixels (int64, cumulative).
 * With fb = 0, max_disparity = FLT_MAX and both probabilities 0 the launch writes nothing.  Two launches on the same inputs write the same
 * bits (no floating-point atomic; the draw depends on (e, tick, stream_id, r) and the key only).  tick is by value, as the capture's.
 * NOT BUILT: a projector or texture model, holes correlated over regions, the firmware's filters, a vertical baseline. */
#define LSIM_STEREO_MAX_WINDOW 128
#define LSIM_STEREO_MAX_LDS_BYTES 163840
typedef struct lsim_sensor_stereo {
    const float* depth;               /* row e starts at depth + e * depth_stride and holds R clean z-depths; read only, 4-byte aligned */
    const uint8_t* labels;            /* [N,label_stride] the capture's labels, or NULL */
    const float* inv_scale;           /* [R] 1 / the sensor's scale, or NULL: 1; 4-byte aligned */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    const float* inst;                /* [N,8] lsim_sensor_instrument's rows, 16-byte aligned, or NULL */
    float* hist;                      /* [N, K, hist_stride] the capture's, K = latency + frames, 16-byte aligned */
    void* state;                      /* 2 int64, 8-byte aligned, zeroed by the caller: [0] holes written, [1] pixels fattened */
    int64_t tick;                     /* >= 0, by value: the capture's */
    int64_t depth_stride;             /* floats between rows of depth: >= R */
    int32_t label_stride;             /* bytes between rows of labels: >= R (ignored when labels == NULL) */
    int32_t hist_stride;              /* the capture's: >= R, a multiple of 4 */
    int32_t latency, frames;          /* the capture's: latency >= 0, frames >= 1, latency + frames <= LSIM_SENSOR_MAX_HISTORY */
    int32_t num_envs, env_stride;     /* N >= 1; every env_stride-th env is visited (>= 1) */
    int32_t width, height;            /* >= 1; R = width * height must be an image lsim_sensor_stereo_sizes accepts */
    int32_t period, stagger;          /* the capture's */
    uint32_t flags;                   /* the capture's: 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
    uint32_t seed, rank, stream_id;   /* the capture's; stream_id < 65536 */
    float fb;                         /* focal length in pixels * baseline in metres: finite, >= 0 */
    float max_disparity;              /* pixels: > 0 (FLT_MAX or infinity: no minimum range) */
    int32_t window;                   /* columns searched for an occluder: 1 .. LSIM_STEREO_MAX_WINDOW */
    float t_lo, t_hi;                 /* 0 <= t_lo < t_hi: the ranges that carry a depth */
    int32_t edge_radius;              /* 0 .. 3 (0: no edge artefacts) */
    float edge_rel;                   /* finite, 0 <= edge_rel < 1 */
    float p_edge_hole, p_edge_cum;    /* 0 <= p_edge_hole <= p_edge_cum <= 1 */
    float drop_value, clip_lo, clip_hi, offset, gain;   /* the capture's: finite, clip_lo <= clip_hi */
} lsim_sensor_stereo_t;
/* bytes of dynamic LDS the launch needs for a width x height image (Z, u and the value to write as floats, the outcome as a byte, per pixel,
 * and two counters).  LSIM_E_INVALID: lds_bytes NULL, width or height < 1, or a plan above LSIM_STEREO_MAX_LDS_BYTES (R > 12601). */
int lsim_sensor_stereo_sizes(int32_t width, int32_t height, size_t* lds_bytes);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: st == NULL; depth or hist NULL or
 * misaligned (4 and 16 bytes); inv_scale given and not 4-byte aligned; inst given and not 16-byte aligned; episode_length or state NULL or
 * not 8-byte aligned; width or height < 1 or an image lsim_sensor_stereo_sizes refuses; depth_stride < R; labels given with
 * label_stride < R; hist_stride < R or not a multiple of 4; latency < 0; frames < 1; latency + frames > LSIM_SENSOR_MAX_HISTORY;
 * num_envs < 1; env_stride < 1; tick < 0; stream_id >= 65536; period < 1; stagger outside 0..1; a flag bit other than the sensor model's
 * two, or both; window outside 1..LSIM_STEREO_MAX_WINDOW; edge_radius outside 0..3; fb, edge_rel, p_edge_hole or p_edge_cum negative or
 * not finite; edge_rel >= 1; p_edge_cum > 1 or < p_edge_hole; max_disparity <= 0 or NaN; t_lo < 0, t_lo >= t_hi (or either NaN);
 * drop_value, clip_lo, clip_hi, offset or gain not finite; clip_lo > clip_hi. */
int lsim_sensor_stereo(const lsim_sensor_stereo_t* st, void* stream);

/* ---- elevation map: a robot-centred 2.5-D height grid per env, filled from the depth rows of a sensor's captures and the robot's own pose,
 * and sampled at the points of the height scan.  ONE launch under the rules of lsim_sensor_capture (caller's stream, no host
 * synchronisation, raw pointers only).  Enqueued BEHIND a capture on the same stream, with its tick, period, stagger, flags and
 * episode_length, it visits the same envs, inserts for the same due set and reads the depth rows that capture just wrote.  It reads the
 * simulator's root_states and writes only its own arrays.  All arithmetic in fp32 (a compiler may contract a product and a sum).
 *
 * State, per env e.  G = size, one of 16, 32, 64; res the cell size in metres; rinv = 1.0f / res, formed ONCE on the host (correctly
 *   rounded) and multiplied with: the absolute cell of a world point (x, y) is (ix, iy) = (floor(x * rinv), floor(y * rinv)) -- a true floor,
 *   coordinates are negative inside the terrain border.  (For res a power of two x * rinv is x / res exactly.)
 *   The grid is WORLD-ALIGNED and TOROIDAL: absolute cell (ix, iy) lives in slot s = (ix & (G-1)) * G + (iy & (G-1)) (two's complement), and
 *   nothing is ever shifted or copied when the robot moves.
 *     height[e][s] f32;   stamp[e][s] i32: tick & 0x7FFFFFFF of the last write (never negative, whatever the tick), -1 never;   cell[e][s] u32: ((ix + 32768) << 16) | (iy + 32768)
 *   A slot KNOWS absolute cell (ix, iy) when stamp >= 0 and cell equals that cell's packed word; a slot left over from a cell that has
 *   scrolled out of the window no longer matches and reads as unknown, without a clearing pass.  A point whose floor(x * rinv) or
 *   floor(y * rinv) is not inside (-32768, 32768) is skipped, when inserting and when looking up.
 * Which envs.  Env e is visited when e % env_stride == 0; fill and due are lsim_sensor_capture's, on the same fields.
 *     bad pose: a non-finite component of root_states[e][0:7] or assumed_mount[e][0:7].  Such an env inserts nothing (its three arrays are
 *         still cleared by fill), its scan row is 0 with known 0, and it adds 1 to state[0] (int64, cumulative) per launch.
 *     fill: all G * G stamps of the env become -1 first (a new episode starts with an empty map).
 *     not due: height, stamp and cell of the env are not written.      Every visited env, due or not, has its scan row rewritten.
 * Insert (due, pose finite).  (p, q) = root_states[e][0:3], [3:7];  (mpos, mq) = assumed_mount[e][0:3], [3:7];  R as in lsim_raycast.  Ray r:
 *     d = a * depth[e * depth_stride + r] + b;      t = inv_scale ? d * inv_scale[r] : d
 *     valid:  |d| <= FLT_MAX  and  t_lo < t  and  t < t_hi  and  (labels == NULL or labels[e * label_stride + r] == 1, terrain)
 *     v = dirs[r] * t;   P = p + R(q) (mpos + R(mq) v);   P not finite: skipped
 *     (ix, iy) = the cell of (P.x, P.y);   (cx, cy) = the cell of (p.x, p.y), each first clamped to [-40000, 40000] as a float
 *     kept:  -G/2 <= ix - cx < G/2  and  -G/2 <= iy - cy < G/2                    (the window: G cells, so no two kept cells share a slot)
 *   Within one capture a cell takes the MAXIMUM P.z of its kept points (the upper surface, what a foot meets), built in LDS with an unsigned
 *   integer atomic max on key(z) = bits(z) ^ (bits(z) >> 31 ? 0xFFFFFFFF : 0x80000000), which orders as the floats do (-0 below +0); key 0 is
 *   no finite float's and marks an untouched slot.  The result does not depend on ray order: reproducible bit for bit.
 *   Behind a barrier every touched slot is overwritten -- the newest capture wins over older ones:
 *     height[e][s] = that maximum;   stamp[e][s] = (int32)(tick & 0x7FFFFFFF);   cell[e][s] = the packed word.
 * Scan (every visited env with a finite pose, behind a barrier after the insert).  Point j of pts [P, 2], in the base-yaw frame:
 *     n = 1 / sqrt(q.z^2 + q.w^2)  (root and quotient correctly rounded);   qy = (0, 0, q.z n, q.w n);   w = p.xy + (R(qy) (pts[j], 0)).xy
 *   -- LSIM_RAYCAST_FRAME_YAW's frame, the reference's quat_apply_yaw.  If the slot of w's cell knows that cell:
 *     scan[e][j] = height,  known[e][j] = 1;      otherwise  scan[e][j] = p.z - unknown_drop,  known[e][j] = 0
 *   (also when w is not finite, q.z = q.w = 0, or its cell is out of range).  No NaN is ever written.
 * `assumed_mount` is a pointer of its own: pointed at a sensor's NOMINAL mount while the capture reads a jittered one, the map is wrong in
 *   the way a robot's is.  Pointing `root_states` at lsim_odometry_step's `est` gives the map a drifting pose.  Averaging and a variance per cell:
 *   lsim_elevation_map_fused below.  NOT BUILT: overhangs, latency compensation of the pose. */
typedef struct lsim_elevation_map {
    const float* root_states;         /* [N,13] simulator buffer, read only */
    const float* assumed_mount;       /* [N,7] the mount pose the map believes in: position, quaternion xyzw */
    const float* dirs;                /* [R,3] the sensor's ray directions */
    const float* inv_scale;           /* [R] 1 / the sensor's scale, or NULL: 1 */
    const float* depth;               /* row e starts at depth + e * depth_stride and holds R values */
    const uint8_t* labels;            /* [N,label_stride] the capture's labels, or NULL */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    const float* pts;                 /* [P,2] scan points in the base-yaw frame */
    float* height;                    /* [N,G,G] */
    int32_t* stamp;                   /* [N,G,G], -1 from the caller at creation */
    uint32_t* cell;                   /* [N,G,G] */
    float* scan;                      /* [N,scan_stride] */
    uint8_t* known;                   /* [N,known_stride] */
    void* state;                      /* 1 int64, 8-byte aligned, zeroed by the caller: [0] visits of envs with a non-finite pose */
    int64_t tick;                     /* >= 0, by value: the capture's */
    int64_t depth_stride;             /* floats between rows of depth: >= R */
    int32_t num_envs, num_rays;       /* N >= 1, R in 1..LSIM_RAYCAST_MAX_RAYS */
    int32_t env_stride;               /* >= 1 */
    int32_t label_stride;             /* bytes between rows of labels: >= R (ignored when labels == NULL) */
    int32_t num_points;               /* P in 1..LSIM_ELEVATION_MAP_MAX_POINTS */
    int32_t scan_stride, known_stride;/* elements between rows: >= P */
    int32_t size;                     /* G: 16, 32 or 64 */
    int32_t period, stagger;          /* the capture's */
    uint32_t flags;                   /* the capture's: 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
    float res;                        /* metres per cell: finite, > 0 */
    float a, b;                       /* depth in metres = a * stored value + b: finite */
    float t_lo, t_hi;                 /* 0 <= t_lo < t_hi: the ranges that are inserted */
    float unknown_drop;               /* finite: an unknown scan point reads p.z - unknown_drop */
} lsim_elevation_map_t;
#define LSIM_ELEVATION_MAP_MAX_POINTS 256
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: em == NULL; root_states, assumed_mount,
 * dirs, depth, pts, height, stamp, cell or scan NULL or not 4-byte aligned; inv_scale given and not 4-byte aligned; known or episode_length
 * NULL, episode_length or state not 8-byte aligned (state NULL); size not 16, 32 or 64; res, a, b or unknown_drop not finite; res <= 0;
 * t_lo < 0, t_lo >= t_hi (or either NaN); P outside 1..LSIM_ELEVATION_MAP_MAX_POINTS; R outside 1..LSIM_RAYCAST_MAX_RAYS; depth_stride < R;
 * labels given with label_stride < R; scan_stride or known_stride < P; tick < 0; period < 1; stagger outside 0..1; env_stride < 1;
 * num_envs < 1; a flag bit other than the sensor model's two; both of them set. */
int lsim_elevation_map(const lsim_elevation_map_t* em, void* stream);

/* ---- odometry: an ESTIMATED base pose that drifts with the distance travelled, for whatever should see the world as a robot does (an
 * elevation map given `est` for its root_states is placed with dead-reckoning error in scale, yaw and height).  ONE launch, one lane per
 * visited env, under the rules of lsim_sensor_mount_jitter (caller's stream, no host synchronisation, raw pointers only, tick by value).  It
 * reads root_states and episode_length, and reads and writes its own state `odo`; it writes rows of `est`.
 *
 * Which envs.  Env e is visited when e % env_stride == 0.  A visited env is FRESH when
 *     (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0
 *   LSIM_SENSOR_RESETS_ONLY is accepted and changes nothing here.  For an env that is not visited NOTHING is written.
 * State.  odo[e] is 12 floats, 48 bytes: {dx, dy, dz, h, scale, yaw_bias, z_bias, 0, prev_x, prev_y, 0, 0} -- the position error in metres,
 *   h the Cayley half-tangent of the yaw error (the error angle is 2 atan h), the episode's three biases, and the true xy of the last launch.
 *   The three zeros are written at every launch.
 * Draws.  Two Philox4x32-10 blocks, key (seed, rank), counters (e, (uint32_t)tick, LSIM_RNG_ODOMETRY, (stream_id << 16) | b), b = 0, 1:
 *     x0..x3 = block 0, x4..x7 = block 1;   u_k = (x_k >> 8) * 2^-24,   s_k = 2 u_k - 1  (exact in fp32), k = 0, 1, 2 and 4, 5, 6;
 *     x3 and x7 are not used.  s0..s2 are the STEP's noise (used by an env that is not fresh), s4..s6 the EPISODE's biases (used by a fresh one).
 * (p, q) = root_states[e][0:3], [3:7].  All arithmetic in fp32 (a compiler may contract a product and a sum); square roots and quotients are
 * correctly rounded.
 *   Fresh env:      dx = dy = dz = h = 0;   scale = s4 * scale_range;   yaw_bias = s5 * yaw_range;   z_bias = s6 * z_range;   prev = p.xy
 *   Otherwise, with a finite root_states[e][0:7]:
 *     D = p.xy - prev                          (D = (0, 0) when a component of prev is not finite)
 *     L = sqrt(D.x^2 + D.y^2)
 *     h += 0.5 * L * (yaw_bias + yaw_noise * s0)
 *     c = 1 / sqrt(1 + h^2);   d = (0, 0, h c, c)  xyzw         (the Cayley map, as in the mount jitter: no transcendental function)
 *     r = R(d) (D.x, D.y, 0)                   (R as in lsim_raycast:  v + 2 w (u x v) + 2 u x (u x v))
 *     k = 1 + (scale + pos_noise * s1)
 *     dx += k r.x - D.x;   dy += k r.y - D.y
 *     dz += L * (z_bias + z_noise * s2)
 *     prev = p.xy
 *   Otherwise (a non-finite component of root_states[e][0:7]):   dx = dy = dz = h = 0;   prev = (NaN, NaN), both words 0x7FC00000 -- the next
 *     finite step integrates D = 0 and the drift starts again from there; the biases are kept.  (A fresh env with such a pose draws its biases
 *     and stores prev = p.xy as it is.)
 *   Every visited env, fresh or not, with c and d formed from the h just stored (h = 0: d = (0, 0, 0, 1)):
 *     est[e][0:3] = p + (dx, dy, dz)
 *     est[e][3:7] = d (x) q, the Hamilton product written out as in lsim_sensor_mount_jitter, not renormalised.  d turns about the WORLD z:
 *         the estimate is wrong in yaw only; roll and pitch against gravity are what an IMU observes.
 *     est[e][7:13] = root_states[e][7:13]
 *     -- except that a non-finite root_states[e][0:7] is copied to est[e][0:7] unchanged (whatever reads est goes on counting it as bad).
 * Consequences.  Every increment is proportional to L: a second launch on the same tick with unmoved robots changes nothing (a fresh env draws
 *   the same biases again; the others integrate D = 0).  All-zero ranges give est[e][0:7] == root_states[e][0:7] bit for bit, up to -0 -> +0,
 *   and dx = dy = dz = h = 0 for ever.  The yaw error bends the PATH: the increment is rotated by the error the estimate has accumulated, so a
 *   yaw bias of b rad/m displaces the estimate by about b s^2 / 2 after s metres straight ahead. */
typedef struct lsim_odometry {
    const float* root_states;         /* [N,13] simulator buffer, read only, 4-byte aligned */
    float* est;                       /* [N,13] the estimated root states; 4-byte aligned; must not be `root_states` */
    float* odo;                       /* [N,12] the state above; 16-byte aligned; zeroed by the caller at creation */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    int64_t tick;                     /* >= 0, by value */
    uint32_t seed, rank, stream_id;   /* as lsim_sensor_model_t's; stream_id < 65536 */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
    int32_t num_envs, env_stride;     /* N >= 1; every env_stride-th env is visited (>= 1) */
    float scale_range;                /* half-width of the episode's distance-scale error, no unit: finite, >= 0 */
    float yaw_range;                  /* half-width of the episode's yaw bias, rad per metre travelled: finite, >= 0 */
    float z_range;                    /* half-width of the episode's height bias, metres per metre travelled: finite, >= 0 */
    float pos_noise, yaw_noise, z_noise;  /* half-widths of the per-step noise on the same three, in the same units: finite, >= 0 */
} lsim_odometry_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: od == NULL; root_states or est NULL or
 * not 4-byte aligned; odo NULL or not 16-byte aligned; episode_length NULL or not 8-byte aligned; est == root_states; num_envs < 1;
 * env_stride < 1; tick < 0; stream_id >= 65536; one of the six ranges negative or not finite; a flag bit other than the sensor model's two;
 * both of them set. */
int lsim_odometry_step(const lsim_odometry_t* od, void* stream);

/* ---- map rows: the elevation map's scan as the rows an actor reads (lsim_policy_extra.rows), in the units of the privileged height scan.
 * ONE launch under the same rules, elementwise over every visited env (e % env_stride == 0) and every column:
 *     rows[e * ld + j]     = clamp(pose[e][2] - z_offset - scan[e * scan_stride + j], -1, 1) * scale       j < P
 *                            (two subtractions in this order, the clamp, then one product; nothing a compiler can contract)
 *     rows[e * ld + P + j] = known[e * known_stride + j] ? 1.0f : 0.0f                                    j < P, channels == 2 only
 *   A non-finite pose[e][2] or scan value writes 0 to the first block: no NaN is ever written.  Columns >= channels * P of a row, and rows
 *   of envs that are not visited, are not touched.  `pose` is the pose the map was given (lsim_elevation_map_t.root_states: the estimate
 *   with odometry, else the simulator's).  With z_offset = 0.5 and scale = obs_scales.height_measurements, fed LSIM_BUF_MEASURED_HEIGHTS and
 *   LSIM_BUF_ROOT_STATES, the first block is the noise-free privileged observation's scan block bit for bit. */
typedef struct lsim_map_rows {
    const float* scan;                /* [N,scan_stride] lsim_elevation_map_t.scan; 4-byte aligned */
    const uint8_t* known;             /* [N,known_stride] lsim_elevation_map_t.known; read only when channels == 2, NULL refused then */
    const float* pose;                /* [N,13] root states, only [e][2] is read; 4-byte aligned */
    float* rows;                      /* [N,ld]; 4-byte aligned */
    int32_t num_points;               /* P in 1..LSIM_ELEVATION_MAP_MAX_POINTS */
    int32_t channels;                 /* 1: heights; 2: heights, then known */
    int32_t scan_stride, known_stride;/* elements between rows: >= P (known_stride ignored when channels == 1) */
    int32_t ld;                       /* floats between rows of `rows`: >= channels * P */
    int32_t num_envs, env_stride;     /* N >= 1; every env_stride-th env is visited (>= 1) */
    float z_offset, scale;            /* finite */
} lsim_map_rows_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: mr == NULL; scan, pose or rows NULL or
 * not 4-byte aligned; channels == 2 and known NULL; P outside 1..LSIM_ELEVATION_MAP_MAX_POINTS; channels outside 1..2; scan_stride < P;
 * channels == 2 and known_stride < P; ld < channels * P; z_offset or scale not finite; num_envs < 1; env_stride < 1. */
int lsim_map_rows(const lsim_map_rows_t* mr, void* stream);

/* ---- elevation map with a variance per cell: lsim_elevation_map whose cells AVERAGE the points of a capture and are fused over the captures
 * by a scalar Kalman filter.  ONE launch under the rules of lsim_elevation_map, which it replaces in a sensor's chain (same position,
 * stream, tick and flags).  `em` is that launch's own struct and everything said there holds unchanged: which envs are visited, fill and
 * due, a bad pose, a ray's validity, its point P and its cell, the window, the words written to stamp and cell, the scan lookup, scan and
 * known.  Fill clears the stamps only: the var of a slot that knows no cell is never read.  All arithmetic in fp32 (a compiler may contract a
 * product and a sum); every quotient below is correctly rounded; int-to-float conversions round to nearest.
 *
 * State.  var[e][s] f32 next to height[e][s]: the variance of the stored height, in m^2; meaningful where the slot knows a cell.
 * Insert (due, pose finite), two passes over the rays and three words of LDS per slot (key, an int32 sum, an int32 count):
 *   Pass 1.  key(z) maximum per slot over the kept points, as lsim_elevation_map's:  zmax.
 *   Pass 2, behind a barrier, over the same rays, every point formed again by the same operations:
 *     df = zmax - P.z   (one fp32 subtraction, >= 0);     the point TAKES PART when df <= band:
 *     sum += q,  q = (int32)(df * 65536.0f + 0.5f)  (the product is exact);     count += 1              (32-bit integer LDS atomics)
 *   Integer sums are associative: the result does not depend on ray order and two launches write the same bits.  band <= 0.5 keeps
 *   q <= 32769 and R * 32769 < 2^31 for every legal R: no sum overflows.  The point that set zmax has df = 0, so count >= 1 -- by construction, not by arithmetic:
 *   both passes form P.z with the SAME code on the same inputs and so get the same bits.  An implementation guards the quotient all the same
 *   (count == 0 reads as zm = zmax), and a sum added to a slot whose key is 0 is never read.
 * Measurement of a touched slot (key != 0) that holds absolute cell (ix, iy), p = root_states[e][0:3] as given to the map:
 *     zm  = zmax - ((float) sum / (float) count) * 2^-16
 *     X = ((float) ix + 0.5f) * res,  Y = ((float) iy + 0.5f) * res;      rho2 = (X - p.x)^2 + (Y - p.y)^2
 *     sigma = sigma0 + sigma2 * (rho2 + range_z2)                  (the sensor's noise at the range of the CELL, not of the rays)
 *     vm  = sigma * sigma / (float) min(count, count_cap) + var_floor
 * Commit, behind a barrier.  With the slot's words as they were before this launch's write (after fill):
 *     age = (float) (((uint32) tick - (uint32) stamp) & 0x7FFFFFFF)             (ticks since the last write, across the stamp's 31-bit wrap)
 *     vp  = var + var_growth * age;      d = zm - height;      S = vp + vm
 *   fuse, when the slot knows this cell and S is finite and d * d < gate2 * S (strict):
 *     K = vp / S;      height = height + K * d;      var = K * vm
 *   otherwise (a new cell, a surface that changed, an estimate that ran away -- the newest capture wins, as it always did):
 *     height = zm;     var = vm
 *   then var = min(max(var, var_floor), var_max), and stamp and cell as lsim_elevation_map writes them.
 * Scan.  scan and known as lsim_elevation_map's.  A known point reports, with the age formed at THIS launch's tick from the slot's stamp,
 *     scan_var[e][j] = min(var + var_growth * age, var_max)
 *   and an unknown point or a bad pose var_max.  No NaN is ever written.
 * Consequences.  band = 0 and gate2 = 0: zmax - 0.0f is zmax and the gate never opens, so height, stamp, cell, scan and known are
 *   lsim_elevation_map's bit for bit.  A cell the camera has left ages: its scan_var grows by var_growth per tick up to var_max.
 * NOT BUILT: variance growth per metre travelled, latency compensation of the pose, overhangs.  (Clearing cells the camera looks through:
 *   lsim_elevation_map_cleanup below, a launch of its own ahead of this one.) */
typedef struct lsim_elevation_map_fused {
    lsim_elevation_map_t em;          /* everything lsim_elevation_map takes, with its meaning and its checks */
    float* var;                       /* [N,G,G] 4-byte aligned */
    float* scan_var;                  /* [N,var_stride] 4-byte aligned */
    float sigma0, sigma2;             /* the noise model: sigma = sigma0 + sigma2 * range^2, metres */
    float range_z2;                   /* the square of the camera's height above the ground, m^2 */
    float band;                       /* metres below the cell's highest point that are averaged: 0 .. 0.5 */
    float var_floor, var_growth;      /* m^2; m^2 per tick */
    float var_max;                    /* m^2: >= var_floor */
    float gate2;                      /* the square of the gate in standard deviations */
    int32_t count_cap;                /* >= 1: more points than this do not lower vm further (their errors are correlated) */
    int32_t var_stride;               /* elements between rows of scan_var: >= P */
} lsim_elevation_map_fused_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: ef == NULL; everything
 * lsim_elevation_map refuses of ef->em; var or scan_var NULL or not 4-byte aligned; var_stride < P; one of sigma0, sigma2, range_z2, band,
 * var_floor, var_growth, var_max, gate2 negative or not finite; band > 0.5; var_floor > var_max; count_cap < 1. */
int lsim_elevation_map_fused(const lsim_elevation_map_fused_t* ef, void* stream);

/* ---- map rows with a confidence: lsim_map_rows whose second block says how far each height can be trusted.  ONE launch, elementwise:
 *     rows[e * ld + j]     = lsim_map_rows's first block, from the same fields of `mr`                      j < P
 *     rows[e * ld + P + j] = known[e * known_stride + j] ? var_ref / (var_ref + scan_var[e * var_stride + j]) : 0.0f       j < P, channels == 2 only
 *   (one sum, one correctly rounded quotient): in (0, 1] for a known point -- 1/2 where the variance is var_ref -- and 0 for an unknown
 *   one.  A scan_var that is not finite or negative reads as 0 confidence: no NaN is ever written. */
typedef struct lsim_map_rows_fused {
    lsim_map_rows_t mr;               /* everything lsim_map_rows takes; channels == 2: heights, then the confidence */
    const float* scan_var;            /* [N,var_stride] lsim_elevation_map_fused_t.scan_var; read only when channels == 2, NULL refused then */
    int32_t var_stride;               /* elements between rows of scan_var: >= P (ignored when channels == 1) */
    float var_ref;                    /* m^2: finite, > 0 */
} lsim_map_rows_fused_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: mf == NULL; everything lsim_map_rows
 * refuses of mf->mr; var_ref not finite or <= 0; channels == 2 and scan_var NULL, not 4-byte aligned or var_stride < P. */
int lsim_map_rows_fused(const lsim_map_rows_fused_t* mf, void* stream);

/* ---- elevation map, visibility clean-up: a cell that the newest capture's rays pass over, well below the height the map holds for it, on
 * their way to ground further away is FORGOTTEN (its stamp becomes -1).  The map launches only ever add; a maximum lifted by noise, a
 * stereo-fattened depth edge or a stretch placed with a pose that has since drifted otherwise stays for the whole episode.  ONE launch
 * under the rules of lsim_elevation_map, enqueued BETWEEN the capture and the map's launch of the same tick, with the same stream, tick and
 * flags: the newest capture's rays are tested against the map of the EARLIER captures, and the map's launch then inserts the new points and
 * writes scan / known from the cleaned map.  `em` is the map's own struct and means what it means there (plain or fused); its scan, known,
 * pts and state are not touched, and neither are height, cell and var: only stamp and cleared are written.  All arithmetic in fp32 (a
 * compiler may contract a product and a sum); the square roots and the quotient below are correctly rounded.
 *
 * Which envs.  Visited, fill and due are lsim_elevation_map's, on em's fields.
 *     fill (a fresh env):  cleared[e] = 0 and nothing else -- the map's launch of this tick empties the env, so it is never cleaned.
 *     due, not fill, pose finite (lsim_elevation_map's "bad pose" on root_states and assumed_mount):  the env is cleaned, as below.
 *     otherwise (not visited; not due; a bad pose, which the map's launch counts and this one does not):  NOTHING is written.
 *   So a launch with LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY writes nothing but those zeros.
 * Stage.  One threshold and one int32 count (0) per slot s of the env, in LDS (2 * G * G * 4 bytes).  With (ix, iy) the one cell of the
 *   window centred on the pose that lives in slot s:
 *     the slot knows that cell (stamp >= 0 and cell == its packed word):
 *         thr[s] = (height[e][s] - clear_margin) - clear_sigma * sqrt(var[e][s])          (the last term only when var != NULL)
 *     otherwise (never written, forgotten, or a cell of an older window):   thr[s] = -infinity
 *   A var that is negative or NaN makes thr NaN, and a NaN thr is never undercut: such a cell stays.
 * Rays, behind a barrier.  Ray r with d and t as lsim_elevation_map forms them is USED when  |d| <= FLT_MAX,  t_lo < t < t_hi,  the label is
 *   terrain where labels are given  -- that launch's range and label tests; its end point does NOT have to lie inside the window --  and
 *   t > end_gap.  With P(t') = p + R(q) (mpos + R(mq) (dirs[r] * t')), the operations and their order those of lsim_elevation_map's P:
 *     O = p + R(q) mpos   (the camera);      E = P(t - end_gap)   (one subtraction);      the ray is skipped when a component of O or E is not finite
 *   In CELL units  o = O.xy * rinv,  e = E.xy * rinv  (skipped when a floor of the four is not inside (-32768, 32768)),  dxy = e - o,  and
 *     dz = E.z - O.z,      L = sqrt((E.x - O.x)^2 + (E.y - O.y)^2)   (metres),      z(u) = O.z + u * dz,   u in [0, 1]
 *   the segment's xy projection is walked cell by cell (Amanatides - Woo) from (ix, iy) = (floor o.x, floor o.y).  Per axis a, when
 *   |d_a| >= 2^-20 cells:  the next boundary b_a = i_a + 1 (d_a > 0) or i_a (d_a < 0),  k_a = 1 / d_a,  u_a = ((float) b_a - o_a) * k_a, formed
 *   anew from the integer boundary after every step (nothing accumulates); an axis that moves less never steps (u_a = +infinity).
 *   At most 2 G + 2 cells are visited, the first included.  With u_in = 0 for the first cell:
 *     u_out = min(u_x, u_y, 1)
 *     the cell COUNTS when it lies inside the window (-G/2 <= i - c < G/2 on both axes, lsim_elevation_map's) and u_out > u_in:
 *         hi = max(z(u_in), z(u_out));      rho = u_out * L;      count[slot] += 1   when   hi + clear_slope * rho < thr[slot]
 *     (a 32-bit integer LDS atomic).  Cells outside the window are stepped over (and once the walk has been inside the window and left it,
 *     it may stop: the window is convex and a segment does not come back).
 *     the walk ends when u_out >= 1;  otherwise the axis with the smaller u steps (x on a tie: the cell entered and left at the same u does not
 *     count), its u is formed anew, and u_in = u_out.
 *   A segment visits a cell at most once and no two window cells share a slot, so a ray adds at most 1 to a slot.  The counts are integers:
 *   they do not depend on ray order and two launches on the same inputs write the same bits (no floating-point atomic).
 *   What the three margins are for:  clear_margin absorbs the sensor's noise;  clear_slope * rho the error of the pose's pitch and roll, which
 *   grows with the distance from the camera;  clear_sigma * sqrt(var) what the fused map itself admits not to know.  hi is the HIGHER end of the
 *   ray's passage through the cell, so a ray that dives into a riser inside the cell does not clear it, and end_gap keeps the ray's own last
 *   cells -- where floor() may have put its point into the neighbour -- out of the test.  A true surface under a clean capture and the true
 *   pose is never forgotten when clear_margin exceeds the height a ray gains across one cell of its own end: sqrt(2) * res * (terrain slope).
 * Sweep, behind a barrier.  A slot with count >= min_rays:  stamp[e][s] = -1;  cleared[e] += the number of such slots (int32, since fill).
 *   height, cell and var keep their bits; a forgotten slot reads unknown and is simply overwritten by its next measurement (the fused map
 *   starts such a cell anew: "the slot knows this cell" is false).
 * NOT BUILT: misses and dropped pixels as free-space rays, overhangs, other envs' robots, lowering a cell instead of forgetting it. */
typedef struct lsim_elevation_map_cleanup {
    lsim_elevation_map_t em;          /* the map's own struct: same meaning, same checks (scan, known, pts and state are not touched) */
    const float* var;                 /* [N,G,G] the fused map's variance, 4-byte aligned, or NULL (plain map) */
    int32_t* cleared;                 /* [N] cells forgotten since the env's episode began; 4-byte aligned */
    float clear_margin;               /* metres: finite, >= 0 */
    float clear_slope;                /* metres per metre of horizontal distance from the camera: finite, >= 0 */
    float clear_sigma;                /* standard deviations of the cell's own variance: finite, >= 0 */
    float end_gap;                    /* metres cut off the ray's end: finite, >= 0 */
    int32_t min_rays;                 /* >= 1: rays that must pass below the threshold */
} lsim_elevation_map_cleanup_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: ec == NULL; everything
 * lsim_elevation_map refuses of ec->em; cleared NULL or not 4-byte aligned; var given and not 4-byte aligned; clear_margin, clear_slope,
 * clear_sigma or end_gap negative or not finite; min_rays < 1. */
int lsim_elevation_map_cleanup(const lsim_elevation_map_cleanup_t* ec, void* stream);

/* ---- foot scans: heights at a small pattern of points around each of the four feet, read from the true terrain or from an elevation map,
 * as the rows an actor reads.  ONE launch under the rules of lsim_map_rows (caller's stream, no host synchronisation, raw pointers only,
 * capturable).  It is STATELESS: no tick, no flags, no due rule -- every visited env (e % env_stride == 0) has its rows rewritten at every
 * launch; for an env that is not visited NOTHING is written.  It reads `pose`, dof_state, the robot tables, `pattern` and the arrays of its
 * source, and writes rows, heights, known and state only.  All arithmetic in fp32; a compiler may contract a product and a sum except where
 * this text says it may not.
 *
 * Per visited env e, with (p, q) = pose[e][0:3], [3:7]:
 * Foot centres, by forward kinematics from `pose` and th_j = dof_state[e][j][0] ONLY (rigid_body_states is not read: its rows are stale for an
 *   env that reset inside the step).  k = env_robot[e] (NULL: 0) selects robots[k] as in lsim_raycast_bodies; only its `bodies` are read.  The
 *   recursion is lsim_raycast_bodies', in coordinates relative to p:
 *     P_0 = 0, Q_0 = q;      body b > 0 with parent a:  P_b = P_a + R(Q_a) joint_pos_b,
 *     Q_b = Q_a * (joint_axis_b sin(th/2), cos(th/2)), th = th_dof_b, or 0 when dof_b < 0;      (a * b: R(a * b) = R(a) R(b), xyzw; R as in lsim_raycast)
 *   Foot l = 0..3 is body 4 + 4l:  F_l = P_{4+4l}  (base-relative, world orientation)  and its centre is c_l = p + F_l.  With `pose` pointed at
 *   lsim_odometry_step's `est` the feet are placed as the robot would place them: its estimated base pose plus its joint encoders.
 * Points.  pattern [K, 2] holds offsets in the yaw frame of q, 1 <= K <= LSIM_FOOT_SCAN_MAX_POINTS, the same for every foot:
 *     n = 1 / sqrt(q.z^2 + q.w^2)  (root and quotient correctly rounded);   qy = (0, 0, q.z n, q.w n)       -- lsim_elevation_map's scan frame
 *     o = R(qy) (pattern[j], 0);      w = ((p.x + F_l.x) + o.x,  (p.y + F_l.y) + o.y)                        point j of foot l
 * Source LSIM_FOOT_SCAN_TERRAIN: the reference's height sampler (LR:1342-1355), what LSIM_BUF_MEASURED_HEIGHTS is sampled with.
 *     fx = (w.x + border_size) / horizontal_scale,  fy likewise   (one sum, one correctly rounded IEEE quotient each, NOT contracted)
 *     (px, py) = (fx, fy) truncated toward zero (NaN: 0; saturating), then clipped to [0, grid_rows - 2] x [0, grid_cols - 2]
 *     h = vertical_scale * min(g[px][py], g[px + 1][py], g[px][py + 1])       g = height_grid [grid_rows, grid_cols] int16 (LSIM_BUF_HEIGHT_GRID)
 *     mesh_type == 0 (the plane): h = 0 and height_grid is not read.      known = 1 always.
 * Source LSIM_FOOT_SCAN_MAP: lsim_elevation_map's lookup, on that map's height / stamp / cell with its size G and res.
 *     rinv = 1.0f / res, formed ONCE on the host;   (ix, iy) = (floor(w.x * rinv), floor(w.y * rinv))  (a true floor);   the slot as there.
 *     the slot knows the cell (stamp >= 0 and cell == the packed word):  h = height[e][slot], known = 1
 *     otherwise -- also when a component of w is not finite or a floor is not inside (-32768, 32768):  h = p.z - unknown_drop, known = 0
 * Outputs, for i = l * K + j (foot-major, 4 K values per env):
 *     rows[e * ld + i]         = clamp(((p.z + F_l.z) - z_offset) - h, -1, 1) * scale
 *                                (one sum, two subtractions in this order, the clamp, one product: nothing a compiler can contract);
 *                                a difference that is not finite writes 0
 *     rows[e * ld + 4 K + i]   = known ? 1.0f : 0.0f                                       channels == 2 only
 *     heights[e * heights_stride + i] = h   and   known[e * known_stride + i] = known      each only when its pointer is given
 *   Columns >= channels * 4 K of a row are not touched.
 * Bad env: a non-finite component of pose[e][0:7], a non-finite th_j (any of the twelve), or q.z = q.w = 0.  Its row blocks, heights and known
 *   are all 0 and state[0] (int64, cumulative) gains 1 per launch.  No NaN is ever written to rows.
 * NOT BUILT: a confidence at foot points (lsim_map_rows_fused's second block), contact-dependent patterns, the foot's own radius. */
#define LSIM_FOOT_SCAN_MAX_POINTS 64       /* K: points per foot */
#define LSIM_FOOT_SCAN_TERRAIN 0           /* source */
#define LSIM_FOOT_SCAN_MAP 1
typedef struct lsim_foot_scan {
    const float* pose;                /* [N,13] root states (the simulator's, or lsim_odometry_step's est); only [e][0:7] is read; 4-byte aligned */
    const float* dof_state;           /* [N,12,2] simulator buffer, read only; 4-byte aligned */
    const uint8_t* env_robot;         /* [N] robot index per env, or NULL: robot 0 */
    const lsim_raycast_robot* robots; /* [num_robots] DEVICE memory: what the launch reads (its `bodies` only) */
    const lsim_raycast_robot* robots_host;  /* the same bytes in HOST memory: what the argument check reads */
    const float* pattern;             /* [K,2] offsets around a foot in the base-yaw frame, metres; 4-byte aligned */
    const int16_t* height_grid;       /* terrain source: [grid_rows,grid_cols] LSIM_BUF_HEIGHT_GRID, 2-byte aligned; may be NULL when mesh_type == 0 */
    const float* height;              /* map source: lsim_elevation_map_t.height [N,G,G] */
    const int32_t* stamp;             /* map source: lsim_elevation_map_t.stamp [N,G,G] */
    const uint32_t* cell;             /* map source: lsim_elevation_map_t.cell [N,G,G] */
    float* rows;                      /* [N,ld]; 4-byte aligned */
    float* heights;                   /* [N,heights_stride] or NULL; 4-byte aligned */
    uint8_t* known;                   /* [N,known_stride] or NULL */
    void* state;                      /* 1 int64, 8-byte aligned, zeroed by the caller: [0] visits of bad envs */
    int32_t source;                   /* LSIM_FOOT_SCAN_TERRAIN or LSIM_FOOT_SCAN_MAP */
    int32_t num_envs, env_stride;     /* N >= 1; every env_stride-th env is visited (>= 1) */
    int32_t num_robots;               /* 1..LSIM_MAX_ROBOTS; 1 when env_robot == NULL */
    int32_t num_points;               /* K in 1..LSIM_FOOT_SCAN_MAX_POINTS */
    int32_t channels;                 /* 1: heights; 2: heights, then known */
    int32_t ld;                       /* floats between rows of `rows`: >= channels * 4 K */
    int32_t heights_stride, known_stride;   /* elements between rows: >= 4 K (each ignored when its pointer is NULL) */
    int32_t mesh_type;                /* terrain source: 0 plane, otherwise the height grid is sampled */
    int32_t grid_rows, grid_cols;     /* terrain source, mesh_type != 0: >= 2, grid_rows * grid_cols < 2^31 */
    int32_t size;                     /* map source: G, 16, 32 or 64 */
    float horizontal_scale, vertical_scale, border_size;   /* terrain source, mesh_type != 0: the config's; the two scales finite and > 0, the border finite */
    float res;                        /* map source: metres per cell, finite and > 0 */
    float unknown_drop;               /* map source: finite */
    float z_offset, scale;            /* finite */
} lsim_foot_scan_t;
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch, nothing written: fs == NULL; pose, dof_state, robots,
 * robots_host, pattern or rows NULL or not 4-byte aligned; heights given and not 4-byte aligned; state NULL or not 8-byte aligned; source not
 * one of the two; num_envs < 1; env_stride < 1; num_robots outside 1..LSIM_MAX_ROBOTS, or != 1 with env_robot == NULL; K outside
 * 1..LSIM_FOOT_SCAN_MAX_POINTS; channels outside 1..2; ld < channels * 4 K; heights given with heights_stride < 4 K; known given with
 * known_stride < 4 K; z_offset or scale not finite; in robots_host[0..num_robots) a body whose parent / dof is not the tree's
 * lsim_raycast_bodies accepts or whose joint_pos / joint_axis is not finite (num_prims and prims are not looked at).
 * Terrain source with mesh_type != 0: height_grid NULL or not 2-byte aligned; grid_rows or grid_cols < 2 or their product >= 2^31;
 * horizontal_scale or vertical_scale not finite or <= 0; border_size not finite.
 * Map source: height, stamp or cell NULL or not 4-byte aligned; size not 16, 32 or 64; res not finite or <= 0; unknown_drop not finite. */
int lsim_foot_scan(const lsim_foot_scan_t* fs, void* stream);

/* ---- depth encoder: a small CNN over a modelled sensor's frame history -> one latent row per env.  FORWARD ONLY (lsim_depth_encode_backward
 * below is its backward pass; isaacgymloco_amd/learn/depth_encoder.py joins the two under autograd).  ONE launch, same rules as lsim_sensor_capture: the caller's stream, no
 * host synchronisation, raw pointers only, so it can be captured in a graph.  It reads `hist` (and episode_length for the due rule), the
 * parameters where the caller keeps them, and writes `latent`; nothing else.
 *
 * Input.  hist, hist_stride are those of the sensor's lsim_sensor_model_t, hist_slots its K = latency + frames.  The image of env e has `frames`
 *   channels, channel f = slot f (oldest first), pixel (y, x) = ray r = y * width + x:
 *     x[f][y][x] = hist[(e * hist_slots + f) * hist_stride + y * width + x],   f < frames, y < height, x < width.
 * Network.  Two square-kernel convolutions without padding or dilation, then a linear layer; ELU(v) = v > 0 ? v : expm1(v)  (alpha = 1):
 *     h1 = (height - k1) / s1 + 1,  w1 = (width - k1) / s1 + 1,  h2 = (h1 - k2) / s2 + 1,  w2 = (w1 - k2) / s2 + 1      (integer division)
 *     a1[c][y][x] = ELU( b1[c] + sum_{f < frames, i < k1, j < k1} w1[c][f][i][j] * x[f][y * s1 + i][x * s1 + j] ),      c < c1, y < h1, x < w1
 *     a2[c][y][x] = ELU( b2[c] + sum_{d < c1, i < k2, j < k2}     w2[c][d][i][j] * a1[d][y * s2 + i][x * s2 + j] ),     c < c2, y < h2, x < w2
 *     z[o]        = b3[o] + sum_{c < c2, y < h2, x < w2} w3[o][(c * h2 + y) * w2 + x] * a2[c][y][x],                    o < latent_dim
 *     latent[e * latent_stride + o] = final_act ? ELU(z[o]) : z[o]
 *   The parameters are in torch's own contiguous layout -- w1 [c1][frames][k1][k1], w2 [c2][c1][k2][k2] (Conv2d.weight), w3 [latent_dim][c2*h2*w2]
 *   (Linear.weight on torch.flatten of NCHW: (c, y, x)) -- and are read at every launch, so an optimiser step is seen by the next one.
 *   Every sum is fp32, in any order, and a product and a sum may be fused.  A non-finite value of hist propagates as it does through torch.
 * Which envs.  Env e is visited when e % env_stride == 0 and is due by the rule of lsim_sensor_capture, with the same episode_length, tick,
 *   period, stagger and flags:  fill = (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0;
 *     due = fill || ( !(flags & LSIM_SENSOR_RESETS_ONLY) && (tick + (stagger ? e : 0)) % period == 0 ).
 *   For an env that is not visited or not due NOTHING is written: its latent row keeps the encoding of its last capture.  Launched after the
 *   sensor's capture of the same tick, the due envs are exactly those whose history has just changed.  tick is passed by value (see above).
 * Limits: the kernel keeps the image, a1 and a2 of one env in the workgroup's LDS; lsim_depth_encode_sizes states the bytes. */
#define LSIM_DEPTH_ENC_MAX_CHANNELS 64     /* c1, c2 */
#define LSIM_DEPTH_ENC_MAX_KERNEL 8        /* k1, k2 */
#define LSIM_DEPTH_ENC_MAX_STRIDE 4        /* s1, s2 */
#define LSIM_DEPTH_ENC_MAX_LATENT 256      /* latent_dim */
#define LSIM_DEPTH_ENC_MAX_LDS_BYTES 163840 /* 4 * (max(frames*height*width, c2*h2*w2) + c1*h1*w1 + frames*k1*k1 + c1*k2*k2), the first two terms each
                                              rounded up to a multiple of 4: the image and a2 share one region, a1 has its own, then one tap table per convolution */
typedef struct lsim_depth_encoder {
    const float* hist;                /* [N, hist_slots, hist_stride]: lsim_sensor_model_t.hist, read only, 16-byte aligned */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    const float* w1;                  /* [c1][frames][k1][k1], 4-byte aligned like every parameter */
    const float* b1;                  /* [c1] */
    const float* w2;                  /* [c2][c1][k2][k2] */
    const float* b2;                  /* [c2] */
    const float* w3;                  /* [latent_dim][c2 * h2 * w2] */
    const float* b3;                  /* [latent_dim] */
    float* latent;                    /* [N, latent_stride], 16-byte aligned: row e, latent_dim floats */
    int64_t tick;                     /* >= 0, by value: the tick of the sensor's capture */
    int32_t hist_stride, hist_slots;  /* floats between slots (>= height * width, a multiple of 4); K: frames <= hist_slots <= LSIM_SENSOR_MAX_HISTORY */
    int32_t num_envs, env_stride;     /* >= 1 */
    int32_t height, width, frames;    /* >= 1 */
    int32_t c1, k1, s1;               /* 1..MAX_CHANNELS, 1..MAX_KERNEL (<= height, width), 1..MAX_STRIDE */
    int32_t c2, k2, s2;               /* likewise, k2 <= h1, w1 */
    int32_t latent_dim, final_act;    /* 1..MAX_LATENT; 0 / 1 */
    int32_t latent_stride;            /* floats between rows of latent: >= latent_dim, a multiple of 4 */
    int32_t period, stagger;          /* as lsim_sensor_model_t's */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
} lsim_depth_encoder_t;
/* bytes of dynamic LDS the configuration needs (only the extents are read: no pointer, no tick).  LSIM_E_INVALID: de or lds_bytes NULL, an extent
 * out of range as listed below, or more than LSIM_DEPTH_ENC_MAX_LDS_BYTES */
int lsim_depth_encode_sizes(const lsim_depth_encoder_t* de, size_t* lds_bytes);
/* the launch described above.  LSIM_E_INVALID, checked on the host before any launch (nothing is written): de == NULL; hist or latent NULL or
 * not 16-byte aligned; episode_length NULL or not 8-byte aligned; a parameter NULL or not 4-byte aligned; num_envs, env_stride, height, width
 * or frames < 1; frames > hist_slots; hist_slots > LSIM_SENSOR_MAX_HISTORY; height * width > hist_stride; hist_stride not a multiple of 4;
 * c1, c2 outside 1..64; k1, k2 outside 1..8; s1, s2 outside 1..4; k1 > height or width; k2 > h1 or w1; latent_dim outside 1..256; final_act
 * outside 0..1; latent_stride < latent_dim or not a multiple of 4; the LDS bytes above the limit; tick < 0; period < 1; stagger outside 0..1;
 * a flag bit other than the sensor model's two; both of them set. */
int lsim_depth_encode(const lsim_depth_encoder_t* de, void* stream);

/* ---- frame log: the images a rollout's captures produced, each logged ONCE, so that the update can encode them again under autograd (the PPO
 * gradient into the encoder, isaacgymloco_amd/learn/vision.py).  Launched behind the sensor's capture with its tick and flags; same rules as
 * lsim_depth_encode: the caller's stream, no host synchronisation, raw pointers only, capturable in a graph.  TWO launches per call (the rows
 * are assigned by the first and copied by the second).  It reads hist, episode_length, row_of[step - 1] and state, and writes log, row_of[step],
 * row_src and state; nothing else.
 *
 * Input.  hist, hist_stride, hist_slots, episode_length, tick, period, stagger, flags, num_envs, env_stride: exactly lsim_depth_encode's, and
 *   the due rule is that launch's:  fill = (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0;
 *     due = fill || ( !(flags & LSIM_SENSOR_RESETS_ONLY) && (tick + (stagger ? e : 0)) % period == 0 ).
 *   `pixels` = height * width floats of each of the first `frames` slots are an env's image.  `step` in 0 .. num_steps - 1 is the storage row
 *   whose latent this capture produces: the chain run behind env step s - 1 belongs to row s, the one that starts a rollout to row 0.
 * Output.  log [capacity, frames, row_stride]: row_stride a multiple of 4, >= pixels, so lsim_depth_encode and its backward read log in place
 *   as a batch with hist = log, hist_slots = frames, hist_stride = row_stride.  row_of [num_steps, N]: the row of log that holds the image env e
 *   showed the encoder for storage row t, or -1.  row_src [capacity]: the (t, e) that wrote a row, as t * N + e.  state: int32 words,
 *   [LSIM_FRAMES_LOG_COUNT] the rows in use, [LSIM_FRAMES_LOG_OVERFLOW] the images that found no room since the caller last zeroed it,
 *   [LSIM_FRAMES_LOG_BASE], [LSIM_FRAMES_LOG_NEXT] the range of rows the last call wrote (what its second launch reads).  The caller zeroes
 *   state once at creation.
 * Rules.  With LSIM_SENSOR_FILL_ALL -- the start of a rollout, step 0 -- count is first taken as 0 and every visited env (e % env_stride == 0)
 *   is LOGGED; otherwise the visited envs that are due are.  A logged env e gets
 *       row = count_before + (the number of logged envs of this call with an index < e):
 *   a function of the inputs alone, no atomic on a shared counter.  If row < capacity: log[row][f][0 .. pixels) = hist[(e * hist_slots + f) *
 *   hist_stride + 0 .. pixels) for f < frames, log[row][f][pixels .. row_stride) = 0, row_of[step][e] = row, row_src[row] = step * N + e.
 *   Otherwise row_of[step][e] = -1 and overflow grows by one.  count grows by the number of rows written.
 *   A visited env that is not logged gets row_of[step][e] = row_of[step - 1][e] -- except in a LSIM_SENSOR_RESETS_ONLY call (a reset by hand in
 *   the middle of a step), which leaves its entry as it is.  An env that is not visited gets row_of[step][e] = -1.
 *   Rows of log and row_src at or above count are never written. */
#define LSIM_FRAMES_LOG_COUNT 0
#define LSIM_FRAMES_LOG_OVERFLOW 1
#define LSIM_FRAMES_LOG_BASE 2
#define LSIM_FRAMES_LOG_NEXT 3
#define LSIM_FRAMES_LOG_STATE_WORDS 4
typedef struct lsim_frames_log {
    const float* hist;                /* [N, hist_slots, hist_stride]: lsim_sensor_model_t.hist, read only, 16-byte aligned */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    float* log;                       /* [capacity, frames, row_stride], 16-byte aligned */
    int32_t* row_of;                  /* [num_steps, N], 4-byte aligned like the next two */
    int32_t* row_src;                 /* [capacity] */
    int32_t* state;                   /* [LSIM_FRAMES_LOG_STATE_WORDS] */
    int64_t tick;                     /* >= 0, by value: the tick of the sensor's capture */
    int32_t hist_stride, hist_slots;  /* as in lsim_depth_encoder_t: >= pixels and a multiple of 4; frames <= hist_slots <= LSIM_SENSOR_MAX_HISTORY */
    int32_t num_envs, env_stride;     /* >= 1 */
    int32_t frames, pixels;           /* >= 1 */
    int32_t row_stride;               /* floats between the frames of log: >= pixels, a multiple of 4 */
    int32_t step, num_steps;          /* 0 <= step < num_steps, by value; num_steps * num_envs < 2^31 */
    int32_t capacity;                 /* rows of log and row_src: >= 1 */
    int32_t period, stagger;          /* as lsim_sensor_model_t's */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
} lsim_frames_log_t;
/* the call described above.  LSIM_E_INVALID, checked on the host before any launch (nothing is written): fl == NULL; hist or log NULL or not
 * 16-byte aligned; episode_length NULL or not 8-byte aligned; row_of, row_src or state NULL or not 4-byte aligned; num_envs, env_stride, frames
 * or pixels < 1; frames > hist_slots; hist_slots > LSIM_SENSOR_MAX_HISTORY; pixels > hist_stride; hist_stride not a multiple of 4;
 * row_stride < pixels or not a multiple of 4; num_steps < 1; step outside 0 .. num_steps - 1; step == 0 without LSIM_SENSOR_FILL_ALL;
 * capacity < 1; num_steps * num_envs >= 2^31; tick < 0; period < 1; stagger outside 0..1; a flag bit other than the sensor model's two; both
 * of them set. */
int lsim_sensor_frames_log(const lsim_frames_log_t* fl, void* stream);

/* ---- gradient rows: d loss / d latent of a minibatch's transitions summed per logged image, the input of lsim_depth_encode_backward over
 * log[0 .. R).  ONE launch under the same rules.  With row_of, row_src as the frame log wrote them and mb_of[t * N + e] the position of
 * transition (t, e) in the minibatch (its row of g), or -1: for r < rows, (t0, e) = (row_src[r] / N, row_src[r] % N),
 *     G[r * G_stride + j] = sum of g[mb_of[t * N + e] * g_stride + j]  over t = t0, t0 + 1, ...  while t < num_steps and row_of[t][e] == r,
 *   for j < latent_dim, terms with mb_of < 0 (or >= batch) skipped: an fp32 sum in ascending t from 0.0f, so two calls with the same inputs
 *   write the same bits.  G is WRITTEN, not accumulated; a row no transition of the minibatch reads is zeros, and so is one whose row_src lies
 *   outside 0 .. num_steps * N - 1.  Columns >= latent_dim and rows >= `rows` of G are not touched.  It reads g, mb_of, row_of and row_src. */
typedef struct lsim_latent_rows_grad {
    const float* g;                   /* [batch, g_stride], 4-byte aligned like every pointer here */
    const int32_t* mb_of;             /* [num_steps * N] */
    const int32_t* row_of;            /* [num_steps, N] */
    const int32_t* row_src;           /* [>= rows] */
    float* G;                         /* [rows, G_stride] */
    int32_t batch;                    /* B >= 1 */
    int32_t rows;                     /* R >= 0, by value (0: nothing is launched) */
    int32_t latent_dim;               /* >= 1 */
    int32_t g_stride, G_stride;       /* floats between rows: >= latent_dim */
    int32_t num_steps, num_envs;      /* >= 1; num_steps * num_envs < 2^31 */
} lsim_latent_rows_grad_t;
/* LSIM_E_INVALID, checked on the host before any launch (nothing is written): lg == NULL; a pointer NULL or not 4-byte aligned; batch < 1;
 * rows < 0; latent_dim < 1; g_stride or G_stride < latent_dim; num_steps or num_envs < 1; num_steps * num_envs >= 2^31. */
int lsim_latent_rows_grad(const lsim_latent_rows_grad_t* lg, void* stream);

/* ---- distillation loss: the squared error between a minibatch's action means and a teacher's means of the same transitions, its gradient
 * and its per-workgroup sums.  ONE launch under the same rules: the caller's stream, no host synchronisation, raw pointers only, capturable in
 * a graph.  `target` holds the teacher's means of EVERY transition of the rollout and index[i] names the transition minibatch row i holds (the
 * slice of the shuffle's permutation), so no gathered copy of the labels exists.  For i < batch, j < actions, with t = index[i]:
 *     0 <= t < target_rows:   d = mu[i * mu_stride + j] - target[t * target_stride + j];     g[i * g_stride + j] = d * scale
 *     otherwise (the row carries no loss):   g[i * g_stride + j] = +0.0f, the row adds nothing to any sum, and neither target nor the
 *                                            values of mu's row enter the result (they may be anything, NaN included)
 *   One subtraction and one product per element, both fp32 and correctly rounded: nothing can be fused, so g is the same bits on every
 *   implementation.  Columns >= actions of g, and the words between `actions` and a stride of mu and target, are neither read nor written.
 *   partial[p], p < LSIM_DISTILL_PARTIALS, is the fp32 sum of d * d over the rows workgroup p owns -- rows p * chunk .. min(batch, (p + 1) *
 *   chunk) - 1 with chunk = ceil(batch / LSIM_DISTILL_PARTIALS) --, UNSCALED; a workgroup that owns no row, or only rows without a loss,
 *   writes 0.  All LSIM_DISTILL_PARTIALS words are written by every call.  The caller forms the loss, 0.5 * scale * sum_p partial[p] (with
 *   scale = 2 / (batch * actions): the mean squared error, of which g is the gradient).  The grid is LSIM_DISTILL_PARTIALS workgroups whatever
 *   batch is; the order of every sum is a function of batch, actions and that constant only (and of which of the two paths below runs): no
 *   floating-point atomic, nothing passes between workgroups, and two calls with the same inputs write the same bits to g and partial.
 *   Paths.  With actions and the three strides multiples of 4 and mu, target and g 16-byte aligned the launch moves 128 bits per access;
 *   otherwise one element.  g is identical on both; partial may differ in rounding.
 *   It reads mu, target and index and writes g and partial; nothing else. */
#define LSIM_DISTILL_PARTIALS 256
#define LSIM_DISTILL_MAX_ACTIONS 16
typedef struct lsim_distill_loss {
    const float* mu;                  /* [batch, mu_stride]: the student's action means of a minibatch, 4-byte aligned like every pointer here */
    const float* target;              /* [target_rows, target_stride]: the teacher's means of every transition of the rollout */
    const int32_t* index;             /* [batch]: the row of target for minibatch row i; outside 0 .. target_rows - 1: the row carries no loss */
    float* g;                         /* [batch, g_stride], WRITTEN: d loss / d mu */
    float* partial;                   /* [LSIM_DISTILL_PARTIALS], WRITTEN, all of it: per-workgroup sums of d * d, unscaled */
    int32_t batch;                    /* >= 1 */
    int32_t actions;                  /* 1 .. LSIM_DISTILL_MAX_ACTIONS */
    int32_t target_rows;              /* >= 1 */
    int32_t mu_stride, target_stride, g_stride;   /* floats between rows: >= actions */
    float scale;                      /* finite, by value: 2 / (batch * actions) as the caller formed it in fp32 */
} lsim_distill_loss_t;
/* LSIM_E_INVALID, checked on the host before the launch (nothing is written): dl == NULL; mu, target, index, g or partial NULL or not 4-byte
 * aligned; batch < 1; actions < 1 or > LSIM_DISTILL_MAX_ACTIONS; target_rows < 1; mu_stride, target_stride or g_stride < actions; scale not
 * finite. */
int lsim_distill_loss(const lsim_distill_loss_t* dl, void* stream);

/* ---- depth encoder, BACKWARD: the gradients of the six parameters from the gradient of `latent`, for a batch of images.  Same rules as every
 * launch here: the caller's stream, no host synchronisation, raw pointers only, capturable in a graph.  THREE launches per call, whatever the
 * extents and the data.  It reads the frames, the parameters, `g` and `latent`, and writes the six gradient buffers and the workspace; nothing else.
 *
 * Input.  The frames are addressed as lsim_depth_encode's hist -- x[b][f][y][x] = hist[(b * hist_slots + f) * hist_stride + y * width + x] -- so a
 *   sensor's history and a contiguous [B, frames, H * W] batch (hist_slots = frames, hist_stride = H * W when that is a multiple of 4) both fit.
 *   `latent` [B, latent_stride] is lsim_depth_encode's output for the same rows and parameters; g [B, g_stride] is the gradient of the loss with
 *   respect to it.  a1, a2 are the forward's activations (recomputed; never stored in memory).  ELU'(a) = a > 0 ? 1 : a + 1 in terms of the
 *   OUTPUT a of ELU (it equals exp(pre): continuous and 1-Lipschitz in a).
 * Gradients.
 *     dz[b][o]   = final_act ? g[b][o] * ELU'(latent[b][o]) : g[b][o]
 *     gb3[o]     = sum_b dz[b][o]
 *     gw3[o][j]  = sum_b dz[b][o] * a2[b][j]                                   j = (c * h2 + y) * w2 + x
 *     da2[b][j]  = sum_o w3[o][j] * dz[b][o]
 *     d2         = da2 * ELU'(a2)
 *     gb2[c]     = sum_{b,y,x} d2[b][c][y][x]
 *     gw2[c][d][i][j] = sum_{b,y,x} d2[b][c][y][x] * a1[b][d][y*s2+i][x*s2+j]
 *     da1[b][d][Y][X] = sum_{c,i,j,y,x : y*s2+i = Y, x*s2+j = X} w2[c][d][i][j] * d2[b][c][y][x]
 *     d1         = da1 * ELU'(a1)
 *     gb1[c]     = sum_{b,y,x} d1[b][c][y][x]
 *     gw1[c][f][i][j] = sum_{b,y,x} d1[b][c][y][x] * x[b][f][y*s1+i][x*s1+j]
 *   Every sum is fp32 and a product and a sum may be fused; the ORDER of every sum is a function of the extents, `batch` and the number of
 *   workgroups (below) only, so two calls with the same inputs write the same bits.  There is no gradient with respect to the frames.
 *   The six outputs have the parameters' own contiguous layouts and are WRITTEN, not accumulated into.  A non-finite input: unspecified result.
 * Workgroups.  W = min(batch, the kernel's own choice -- a function of the extents, at most 256 --, and grid_limit when that is > 0) workgroups
 *   share the samples: workgroup k takes batch / W consecutive samples, the first batch % W workgroups one more, and keeps one partial sum of
 *   gw1 | gb1 | gw2 | gb2 in the workspace; the partial sums are added in the order of k.
 * Workspace.  lsim_depth_encode_backward_sizes states the bytes: 4 * batch * (c2*h2*w2 + latent_dim) -- a2 and dz of every row, for gw3 and gb3 --
 *   plus the partial sums of the largest W the extents and grid_limit allow, which does not grow with batch.  No buffer of the size of a1 exists. */
typedef struct lsim_depth_encoder_bwd {
    const float* hist;                /* [B, hist_slots, hist_stride], read only, 16-byte aligned */
    const float* w1;                  /* the parameters, as in lsim_depth_encoder_t, 4-byte aligned */
    const float* b1;
    const float* w2;
    const float* b2;
    const float* w3;
    const float* b3;
    const float* g;                   /* [B, g_stride]: d loss / d latent, 4-byte aligned */
    const float* latent;              /* [B, latent_stride]: the forward's output of the same rows, 4-byte aligned */
    float* gw1;                       /* [c1][frames][k1][k1], 4-byte aligned like every gradient */
    float* gb1;                       /* [c1] */
    float* gw2;                       /* [c2][c1][k2][k2] */
    float* gb2;                       /* [c2] */
    float* gw3;                       /* [latent_dim][c2 * h2 * w2] */
    float* gb3;                       /* [latent_dim] */
    void* workspace;                  /* 16-byte aligned, workspace_bytes >= what lsim_depth_encode_backward_sizes reports */
    uint64_t workspace_bytes;
    int32_t hist_stride, hist_slots;  /* as in lsim_depth_encoder_t */
    int32_t batch;                    /* B >= 1 */
    int32_t height, width, frames;
    int32_t c1, k1, s1;
    int32_t c2, k2, s2;
    int32_t latent_dim, final_act;
    int32_t g_stride, latent_stride;  /* floats between rows: >= latent_dim */
    int32_t grid_limit;               /* 0: the kernel's own choice; n >= 1: at most n workgroups share the samples */
} lsim_depth_encoder_bwd_t;
/* bytes of dynamic LDS of the per-sample launch and of the workspace (only batch, the extents and grid_limit are read).  LSIM_E_INVALID: a NULL
 * argument, batch < 1, grid_limit < 0, an extent out of range as for lsim_depth_encode_sizes, or more LDS than LSIM_DEPTH_ENC_MAX_LDS_BYTES:
 *   4 * (frames*height*width + c1*h1*w1 + c2*h2*w2 + latent_dim, each rounded up to a multiple of 4, + frames*k1*k1 + c1*k2*k2 + h1*w1 + h2*w2)
 *   plus a few hundred bytes for the launch's own arguments */
int lsim_depth_encode_backward_sizes(const lsim_depth_encoder_bwd_t* db, size_t* lds_bytes, size_t* workspace_bytes);
/* the launches described above.  LSIM_E_INVALID, checked on the host before anything is launched or written: db == NULL; hist NULL or not
 * 16-byte aligned; a parameter, a gradient, g or latent NULL or not 4-byte aligned; workspace NULL or not 16-byte aligned; workspace_bytes below
 * what _sizes reports; batch < 1; grid_limit < 0; height, width or frames < 1; frames > hist_slots; hist_slots > LSIM_SENSOR_MAX_HISTORY;
 * height * width > hist_stride; hist_stride not a multiple of 4; c1, c2 outside 1..64; k1, k2 outside 1..8; s1, s2 outside 1..4; k1 > height or
 * width; k2 > h1 or w1; latent_dim outside 1..256; final_act outside 0..1; g_stride or latent_stride < latent_dim; the LDS bytes above the limit. */
int lsim_depth_encode_backward(const lsim_depth_encoder_bwd_t* db, void* stream);

/* ---- depth memory: ONE GRU cell (torch's nn.GRUCell, gate order r, z, n) behind the depth encoder, so that what the camera saw a second ago is
 * still there when the hind feet reach it.  Three launches share the cell: lsim_depth_memory_step advances every env's hidden state by one
 * control step during the rollout; lsim_gru_sequence_forward / _backward run the recurrence over a stored rollout chunk and back (truncated
 * back-propagation through time; isaacgymloco_amd/learn/depth_memory.py joins them under autograd).  Same rules as every launch here: the
 * caller's stream, no host synchronisation, raw pointers only, capturable in a graph, ONE launch per call.
 *
 * The cell.  The parameters stay in torch's own contiguous layout and are read where torch keeps them at every launch, so an optimiser step is
 *   seen by the next one:  weight_ih [3H][I], weight_hh [3H][H], bias_ih [3H], bias_hh [3H];  rows 0..H-1 are gate r, H..2H-1 gate z (called u
 *   below: z is the latent), 2H..3H-1 gate n.
 *     x    = [ z_e (L columns of the encoder's latent row) | p_e (P columns of the env's one-step observation; P may be 0) ],   I = L + P
 *     gi   = W_ih x + b_ih                       gh = W_hh h_prev + b_hh
 *     r    = sigmoid(gi_r + gh_r)                u  = sigmoid(gi_z + gh_z)             n = tanh(gi_n + r * gh_n)
 *     h'   = (1 - u) * n + u * h_prev            sigmoid(v) = 1 / (1 + exp(-v))
 *   Note r * (W_hn h + b_hn), not W_hn (r * h).  Every sum is fp32, in any order, and a product and a sum may be fused.
 * Limits.  hidden is a multiple of 16, at most LSIM_GRU_MAX_HIDDEN; I <= LSIM_GRU_MAX_INPUT.  The two sequence kernels keep W_hh resident in the
 *   workgroup's LDS, so lsim_depth_memory_sizes -- and with it all three launches -- ACCEPTS hidden in {16, 32, 48, 64, 80, 96} and REFUSES 112
 *   and 128 (their plan is above LSIM_GRU_MAX_LDS_BYTES).
 *
 * lsim_depth_memory_step.  A workgroup owns 16 consecutive envs.  For env e
 *     fresh = (flags & LSIM_SENSOR_FILL_ALL) || episode_length[e] == 0      (the rule of lsim_sensor_capture for a reset: no tick argument)
 *     h_prev = fresh ? 0 : h[e]
 *   flags 0: every env steps; LSIM_SENSOR_FILL_ALL: every env steps from h_prev = 0; LSIM_SENSOR_RESETS_ONLY: only fresh envs are stepped and
 *   written, the others keep h and their row bit for bit (a by-hand reset between two steps).  For a stepped env h[e] = h' in place and, when
 *   rows != NULL, rows[e] = [ z_e | h'_e ] (L + H columns: what the actor reads).  Nothing else is written. */
#define LSIM_GRU_MAX_HIDDEN 128
#define LSIM_GRU_MAX_INPUT 512
#define LSIM_GRU_MAX_LDS_BYTES 163840
typedef struct lsim_depth_memory {
    const float* z;                   /* [N, z_ld]: the encoder's latent rows, L columns read, 4-byte aligned like every float pointer here */
    const float* p;                   /* [N, p_ld]: the one-step observation, P columns read; NULL with proprio_dim == 0 */
    const int64_t* episode_length;    /* [N] LSIM_BUF_EPISODE_LENGTH, read only, 8-byte aligned */
    const float* weight_ih;           /* [3H][I] */
    const float* weight_hh;           /* [3H][H] */
    const float* bias_ih;             /* [3H] */
    const float* bias_hh;             /* [3H] */
    float* h;                         /* [N, h_ld]: the hidden state, H columns, updated in place */
    float* rows;                      /* [N, rows_ld]: [z | h'], L + H columns; NULL: not written */
    int32_t num_envs;                 /* >= 1 */
    int32_t latent_dim, proprio_dim;  /* L >= 1, P >= 0, L + P <= LSIM_GRU_MAX_INPUT */
    int32_t hidden;                   /* H */
    int32_t z_ld, p_ld, h_ld, rows_ld;/* floats between rows: >= L, >= P, >= H, >= L + H (p_ld / rows_ld are not read without p / rows) */
    uint32_t flags;                   /* 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY */
} lsim_depth_memory_t;
/* bytes of dynamic LDS of the three launches for a cell of `hidden` units and `input_dim` = L + P inputs (any of the three outputs may be NULL):
 *   step      4 * 16 * ((I rounded up to 16) + 2 + H + 2)                       the tile's x and h
 *   forward   4 * (3H + 32) * (H + 2)                                            W_hh and two copies of the tile's h
 *   backward  4 * (H + 32) * (3H + 2)                                            W_hh transposed and two copies of the tile's gate gradients
 * LSIM_E_INVALID: hidden < 16, not a multiple of 16 or > LSIM_GRU_MAX_HIDDEN; input_dim outside 1..LSIM_GRU_MAX_INPUT; any of the three above
 * LSIM_GRU_MAX_LDS_BYTES (hidden 112 and 128). */
int lsim_depth_memory_sizes(int32_t hidden, int32_t input_dim, size_t* lds_step, size_t* lds_forward, size_t* lds_backward);
/* the rollout launch described above.  LSIM_E_INVALID, checked on the host before any HIP call (nothing is written): dm == NULL; z, h, a
 * parameter NULL or not 4-byte aligned; episode_length NULL or not 8-byte aligned; proprio_dim > 0 with p NULL or not 4-byte aligned; rows not
 * 4-byte aligned; num_envs < 1; latent_dim < 1; proprio_dim < 0; hidden or latent_dim + proprio_dim refused by lsim_depth_memory_sizes;
 * z_ld < L; p_ld < P with P > 0; h_ld < H; rows_ld < L + H with rows; a flag bit other than the sensor model's two; both of them set. */
int lsim_depth_memory_step(const lsim_depth_memory_t* dm, void* stream);

/* lsim_gru_sequence_forward / _backward: the same recurrence over T stored steps of n envs, contiguous [T, n, .] arrays.  A workgroup owns 16
 * consecutive envs for all T steps, so the time of a call is T times the latency of one step, whatever n up to one workgroup per CU.
 * Forward.  gi [T, n, 3H] is the input projection W_ih x + b_ih of every step, formed by the caller with one GEMM over all T * n rows (the
 *   serial kernel never reads W_ih).  reset [T, n]: nonzero means h_prev = 0 at that step.  For t = 0 .. T-1
 *     h_prev = reset[t] ? 0 : (t == 0 ? h0 : hs[t-1]);      hs[t] = h' of the cell above with gi = gi[t]
 *   and, when save != NULL, save[t] = [ r | u | n | gh_n ] (4H columns; gh_n = W_hn h_prev + b_hn): what the backward needs, stored rather than
 *   recomputed, because recomputing gh in the backward would double the matrix work of its serial chain.
 * Backward.  dhs [T, n, H] is d loss / d hs[t] from whatever reads the states.  With dh the total gradient at step t (dh = dhs[T-1] at t = T-1),
 *   for t = T-1 .. 0, h_prev as in the forward:
 *     dn~ = dh * (1 - u) * (1 - n*n)        du~ = dh * (h_prev - n) * u * (1 - u)        dr~ = dn~ * gh_n * r * (1 - r)
 *     dgi[t]  = [ dr~ | du~ | dn~ ]         dghn[t] = dn~ * r
 *     dh(t-1) = ( dh * u + [ dr~ | du~ | dn~ * r ] . W_hh ) * (reset[t] ? 0 : 1)  +  dhs[t-1]           (the last term for t >= 1)
 *   and dh0 (when not NULL) = the bracket times the reset factor at t = 0.  dgi and dghn are WRITTEN, not accumulated.  The parameter gradients
 *   are then GEMMs and column sums over the T * n rows that the caller issues: dW_ih = dgi^T x, dW_hh = [dgi_r | dgi_u | dghn]^T h_prev,
 *   db_ih = sum dgi, db_hh = sum [dgi_r | dgi_u | dghn].  There is no gradient with respect to x.
 *   The order of every sum is a function of the extents only: two calls with the same inputs write the same bits. */
typedef struct lsim_gru_sequence {
    const float* gi;                  /* [T, n, 3H], 16-byte aligned like every [T, n, .] and [n, .] array here; forward only */
    const float* h0;                  /* [n, H] */
    const uint8_t* reset;             /* [T, n] */
    const float* weight_hh;           /* [3H][H], 4-byte aligned */
    const float* bias_hh;             /* [3H], 4-byte aligned; forward only */
    float* hs;                        /* [T, n, H]: written by the forward, read by the backward */
    float* save;                      /* [T, n, 4H]: written by the forward (NULL: not kept), read by the backward */
    const float* dhs;                 /* [T, n, H]; backward only, like the next three */
    float* dgi;                       /* [T, n, 3H] */
    float* dghn;                      /* [T, n, H] */
    float* dh0;                       /* [n, H], or NULL */
    int32_t steps, num_envs, hidden;  /* T >= 1, n >= 1, H as above */
} lsim_gru_sequence_t;
/* LSIM_E_INVALID, checked on the host before any HIP call: gs == NULL; gi, h0 or hs NULL or not 16-byte aligned; save not 16-byte aligned;
 * reset NULL; weight_hh or bias_hh NULL or not 4-byte aligned; steps < 1; num_envs < 1; hidden refused by lsim_depth_memory_sizes */
int lsim_gru_sequence_forward(const lsim_gru_sequence_t* gs, void* stream);
/* LSIM_E_INVALID likewise: gs == NULL; h0, hs, save, dhs, dgi or dghn NULL or not 16-byte aligned; dh0 not 16-byte aligned; reset NULL;
 * weight_hh NULL or not 4-byte aligned; steps < 1; num_envs < 1; hidden refused by lsim_depth_memory_sizes */
int lsim_gru_sequence_backward(const lsim_gru_sequence_t* gs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSIM_H */
