/*
 * sag.h - C ABI of libsag.so: batched SafeAdaptationGym.step() on MI355X (gfx950).
 *
 * This is the drop-in boundary for the hot path.  The reference has no FFI; its
 * seam is the Python object MujocoBridge (reference safe_adaptation_gym/
 * mujoco_bridge.py:15-280) as consumed by SafeAdaptationGym.step/reset/observation
 * (safe_adaptation_gym.py:56-139), World (world.py:139-165,219-231) and the tasks'
 * compute_reward/reset/set_mocaps (tasks/<task>.py).  Each entry point below names the
 * reference calls it replaces.  Plain pointers and sizes only; no exceptions cross
 * the ABI; every function returns 0 on success and a negative sag_status on error,
 * with a message available from sag_last_error().
 *
 * Ownership: the caller owns every host buffer it passes; the library owns all
 * device memory.  One context per GPU, one HIP stream per context.  A context is
 * not thread-safe; distinct contexts are independent (one host thread each).
 *
 * Per-env physics failure (non-finite state, the reference's PhysicsError branch,
 * safe_adaptation_gym.py:73-75) is reported as DATA (done=1, reward=-10, cost=0),
 * not as an error code.
 */
#ifndef SAG_H_
#define SAG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAG_ABI_VERSION 5

/* ---- capacities (maxima over the reference's task set: Task.obstacles) ---- */
#define SAG_MAX_HAZARDS 9  /* tasks/go_to_goal.py:83-84  [9,10,0,1]          */
#define SAG_MAX_VASES 10   /* tasks/go_to_goal.py:83-84                     */
#define SAG_MAX_PILLARS 2  /* every task has <= 1; one spare                */
#define SAG_MAX_BUTTONS 6  /* tasks/collect.py:11 NUM_BUTTONS = 6           */
#define SAG_MAX_NU 12      /* doggo.xml:134-145                             */
#define SAG_LIDAR_BINS 16  /* safe_adaptation_gym.py:22                     */

/* ---- robots (safe_adaptation_gym.py:15-19 control substeps) ---- */
enum sag_robot { SAG_ROBOT_POINT = 0, SAG_ROBOT_CAR = 1, SAG_ROBOT_DOGGO = 2 };

/* ---- task ids = index into sorted benchmark.TASKS keys
 *      (benchmark/__init__.py:14-20; pinned by tests/golden/sampler.json) ---- */
enum sag_task {
  SAG_TASK_CATCH_GOAL = 0,
  SAG_TASK_COLLECT = 1,
  SAG_TASK_DRIBBLE_BALL = 2,
  SAG_TASK_GO_TO_GOAL = 3,
  SAG_TASK_GO_TO_GOAL_DAMPING = 4,
  SAG_TASK_GO_TO_GOAL_MOTOR = 5,
  SAG_TASK_GO_TO_GOAL_SCARCE = 6,
  SAG_TASK_HAUL_BOX = 7,
  SAG_TASK_PRESS_BUTTONS = 8,
  SAG_TASK_PRESS_BUTTONS_SCARCE = 9,
  SAG_TASK_PUSH_BOX = 10,
  SAG_TASK_PUSH_BOX_SCARCE = 11,
  SAG_TASK_ROLL_ROD = 12,
  SAG_TASK_UNSUPERVISED = 13,
  SAG_NUM_TASKS = 14
};

enum sag_box_kind { SAG_BOX_NONE = 0, SAG_BOX_BOX = 1, SAG_BOX_ROD = 2, SAG_BOX_BALL = 3 };

enum sag_status {
  SAG_OK = 0,
  SAG_ERR_ARG = -1,      /* bad argument                                  */
  SAG_ERR_HIP = -2,      /* HIP runtime error (message has the HIP text)  */
  SAG_ERR_NODEVICE = -3, /* no gfx950 device / device ordinal out of range */
  SAG_ERR_STATE = -4,    /* call out of order (step before set_layout)    */
  SAG_ERR_UNSUPPORTED = -5
};

/*
 * Per-env record: what rebuild() + World.reset() install in the reference
 * (world.py:108-137 world_config, mujoco_bridge.py:59-63,154-166, tasks' reset)
 * and, read back, the full simulator + task state (checkpoint / parity tests).
 * Host side it is an array-of-records [n_envs][SAG_REC_FLOATS] float32 plus
 * [n_envs][SAG_REC_INTS] int32; the library transposes to its SoA device layout.
 * World-frame planar coordinates; angles in radians; SI units.
 */
enum sag_rec_float {
  SAG_F_ROBOT = 0,        /* x, y, yaw, vx, vy, w  (world frame)                      */
  SAG_F_ROBOT0 = 6,       /* x0, y0, rot0: pose at rebuild (qpos frame, mujoco_bridge.py:59-63) */
  SAG_F_GEAR = 9,         /* point motor-x gear: 0.3, Motor variant 3.0 (go_to_goal_motor.py:12-16) */
  SAG_F_DAMP = 10,        /* slide damping: 0.01, Damping variant 0.001 (go_to_goal_damping.py:12-17) */
  SAG_F_ACTION_NOISE = 11, /* world.py:31                                             */
  SAG_F_CTRL_SCALE = 12,  /* [SAG_MAX_NU] ctrlrange scale (world.py:72-73)            */
  SAG_F_HAZARD_SIZE = 24, /* world.py:20                                              */
  SAG_F_VASE_SIZE = 25,   /* world.py:21  (half extent)                               */
  SAG_F_PILLAR_SIZE = 26, /* world.py:22  (radius)                                    */
  SAG_F_KEEPOUT = 27,     /* robot, hazards, vases, pillars, box  (world.py:60-70, push_box.py:13) */
  SAG_F_GOAL = 32,        /* x, y                                                     */
  SAG_F_CATCH = 34,       /* origin x, y, current_radius, next_radius (catch_goal.py:14-18) */
  SAG_F_LAST = 38,        /* last goal dist, last box dist, last box-goal dist        */
  SAG_F_BOX = 41,         /* x, y, yaw, vx, vy, w                                     */
  SAG_F_HAZARDS = 47,     /* (x, y) * SAG_MAX_HAZARDS                                 */
  SAG_F_PILLARS = 65,     /* (x, y) * SAG_MAX_PILLARS                                 */
  SAG_F_BUTTONS = 69,     /* (x, y) * SAG_MAX_BUTTONS                                 */
  SAG_F_VASES = 81,       /* (x, y, yaw, vx, vy, w) * SAG_MAX_VASES                   */
  SAG_F_BOUND = 141,      /* info['bound'] (world.py:75-78); carried, not used on the device */
  SAG_F_ROBOT_EXT = 144,  /* robot DoF beyond the planar base. car (car.xml:21-32): wheel rates left,
                           * right (rad/s about the axle); rear ball: angular velocity x,y,z
                           * (relative to the base, base frame); ball quaternion w,x,y,z.
                           * doggo (doggo.xml): [0] base z, [1..4] base quaternion w,x,y,z, [5] vz,
                           * [6..8] base angular velocity in the base frame (MuJoCo free-joint qvel),
                           * [9..21] the 13 hinge angles in qpos order (hip_1_z, hip_1_y, ankle_1,
                           * hip_4_z, hip_4_y, ankle_4, waist_x, hip_2_z, hip_2_y, ankle_2, hip_3_z,
                           * hip_3_y, ankle_3), [22..34] their rates.  ROBOT x, y, vx, vy are the base
                           * position / world velocity; ROBOT yaw and w are derived (heading, world
                           * yaw rate) and written back every step.  A zero quaternion at install
                           * time means "upright at ROBOT yaw, z = 0.22, joints at 0".            */
  SAG_ROBOT_EXT_FLOATS = 40,
  SAG_REC_FLOATS = 184
};

enum sag_rec_int {
  SAG_I_TASK = 0,
  SAG_I_NH = 1,
  SAG_I_NV = 2,
  SAG_I_NP = 3,
  SAG_I_NB = 4,
  SAG_I_BOX_KIND = 5,
  SAG_I_GOAL_BUTTON = 6,  /* press_buttons.py:72                                   */
  SAG_I_BTN_STATE = 7,    /* 0 = BUTTON_CHANGE, 1 = NORMAL (press_buttons.py:101-104) */
  SAG_I_BTN_TIMER = 8,    /* press_buttons.py:107-121                              */
  SAG_I_CATCH_TIMER = 9,  /* catch_goal.py:17                                      */
  SAG_I_ACTIVE_MASK = 10, /* collect.py:15-16: bit b = buttons{b} still active     */
  SAG_I_STEP = 11,        /* env steps since rebuild (time = step * nstep * dt)    */
  SAG_I_ENV_ID = 12,      /* global env index (counter-based RNG stream id)        */
  SAG_I_FLAGS = 13,       /* bit0: resample failed (ResamplingError), bit1: tape exhausted,
                           * bit2: a Doggo constraint did not fit the row budget and was dropped */
  SAG_I_EPISODE = 14,     /* episode nonce of the counter-based generator (24 bits): with SAG_I_ENV_ID
                           * and SAG_I_STEP it forms the counter, so that the device-side draws of
                           * throughput mode (action noise, goal resampling, CatchGoal radii, button
                           * choice) differ from episode to episode as the reference's reseeded
                           * RandomState does (safe_adaptation_gym.py:97-101).  sag_set_layout takes it
                           * from the record, sag_reset adds one */
  SAG_I_AWAKE = 15,       /* bit k: free body k (vases 0 .., the task object = bit SAG_MAX_VASES) takes part in the NEXT forward
                           * evaluation although it is at rest.  sag_set_layout sets it for bodies whose bounding circle
                           * overlaps another free body's, a pillar's or a button's (HaulBox spawns its box at robot + .6
                           * without a keep-out check, haul_box.py:17-18: MuJoCo separates such a pair in the first steps,
                           * and so does this); the first substep clears it (a body in motion is awake by its velocity);
                           * sag_set_state / sag_get_state carry it like any other field (ABI v5) */
  SAG_REC_INTS = 16
};

typedef struct sag_config {
  int32_t abi_version;  /* SAG_ABI_VERSION                                     */
  int32_t robot;        /* enum sag_robot                                      */
  int32_t n_envs;       /* envs owned by this context (one shard)              */
  int32_t device;       /* HIP device ordinal                                  */
  int32_t max_hazards;  /* SoA capacities, <= SAG_MAX_*; 0 drops the arrays    */
  int32_t max_vases;
  int32_t max_pillars;
  int32_t max_buttons;
  int32_t has_box;      /* allocate box state                                  */
  int32_t reserved0;
  uint64_t seed;        /* key of the counter-based generator (throughput mode); sag_set_seed changes it */
} sag_config;

typedef struct sag_ctx sag_ctx;

/* Static per-robot facts: replaces Robot (robot.py:11-59) + the substep table
 * (safe_adaptation_gym.py:15-19).  out[0]=nu out[1]=obs_dim out[2]=nstep
 * out[3]=nq out[4]=nv; dt in *dt. */
int sag_robot_info(int32_t robot, int32_t out[5], double* dt);

/* Replaces MujocoBridge.__init__ (mujoco_bridge.py:26-36): allocates the SoA
 * world for n_envs on one device and creates the context's stream. */
int sag_create(const sag_config* cfg, sag_ctx** out);
int sag_destroy(sag_ctx* ctx);
const char* sag_last_error(const sag_ctx* ctx); /* ctx may be NULL: last create error */

/* Replaces MujocoBridge.rebuild(world_config) + World.reset()
 * (mujoco_bridge.py:170-175, world.py:167-170, safe_adaptation_gym.py:170-172)
 * for the listed envs, without compiling anything.  env_ids == NULL means
 * 0..n-1.  Velocities in the record are honoured (normally 0). */
int sag_set_layout(sag_ctx* ctx, const int32_t* env_ids, int32_t n,
                   const float* rec_f, const int32_t* rec_i);

/* Re-install the records last given to sag_set_layout for these envs (start
 * of a fixed-layout episode); their episode nonce (SAG_I_EPISODE) advances by one. */
int sag_reset(sag_ctx* ctx, const int32_t* env_ids, int32_t n);

/* env.seed(s) (safe_adaptation_gym.py:113-118) for the device-side generator of throughput
 * mode: the key of the counter-based stream from the next step on. */
int sag_set_seed(sag_ctx* ctx, uint64_t seed);

/* Checkpoint / parity access to the complete per-env state (same records). */
int sag_get_state(sag_ctx* ctx, const int32_t* env_ids, int32_t n, float* rec_f,
                  int32_t* rec_i);
int sag_set_state(sag_ctx* ctx, const int32_t* env_ids, int32_t n,
                  const float* rec_f, const int32_t* rec_i);

/* Host-buffer step = SafeAdaptationGym.step (safe_adaptation_gym.py:56-83) for
 * every env of the context.
 *   actions  [n_envs][nu] f32, before noise/clip (:58-67)
 *   noise    [n_envs][nu] f32 standard normals (parity mode: the reference's
 *            rs.normal draws) or NULL: counter-based generator on device
 *   tape     [n_envs][tape_len] u32 raw generator words consumed by in-step
 *            draws in the reference's order (App. B.6: CatchGoal radius,
 *            goal resample uniforms, button choice) or NULL: counter-based
 *   nstep    physics substeps; <0 = the robot's table value (5/10/12);
 *            0 = no physics: evaluate reward/cost/observation at the current state
 *   obs      [n_envs][obs_dim] f32   reward [n_envs][2] f32 (col 1 only used by
 *            Unsupervised, tasks/unsupervised.py:66)   cost/done/goal_met
 *            [n_envs] u8   tape_used [n_envs] i32 (may be NULL)
 * Any output pointer may be NULL (skipped).  Synchronous. */
int sag_step(sag_ctx* ctx, const float* actions, const float* noise,
             const uint32_t* tape, int32_t tape_len, int32_t nstep, float* obs,
             float* reward, uint8_t* cost, uint8_t* done, uint8_t* goal_met,
             int32_t* tape_used);

/* External contact results for the NEXT step with nstep == 0 (one-shot; replay of recorded episodes: the caller sets
 * the poses with sag_set_state and supplies what the physics would have reported).  Replaces, per env, the outcome of
 * MujocoBridge.robot_contacts on the final state (mujoco_bridge.py:177-191): cost_contacts[i] = number of contacts
 * robot geom <-> obstacle geom (world.py:146; -1 = keep the device's own geometric result for this env),
 * btn_mask[i] = buttons the robot touches (tasks/press_buttons.py:51, tasks/collect.py:32).  Host arrays [n_envs];
 * NULL, NULL clears a pending set.  A step with nstep != 0 ignores and clears it. */
int sag_set_ext_contacts(sag_ctx* ctx, const int32_t* cost_contacts, const uint32_t* btn_mask);

/* Device-buffer step for learners that live on the GPU: same semantics, all
 * pointers are device pointers on ctx's device (or NULL as above), enqueued on
 * the context stream; returns without waiting.  sag_wait() joins. */
int sag_step_device(sag_ctx* ctx, const float* d_actions, const float* d_noise,
                    int32_t nstep, float* d_obs, float* d_reward, uint8_t* d_cost,
                    uint8_t* d_done, uint8_t* d_goal_met);
int sag_wait(sag_ctx* ctx);

/* First observation after reset: `self.observation` at safe_adaptation_gym.py:104,107
 * (mj_forward + sensors + 3 lidars, no reward/cost). */
int sag_observe(sag_ctx* ctx, float* obs);

/* The lidar + hazard-cost kernel on its own (BASELINE config 2), on explicit
 * poses; replaces lidar_observations/_lidar (safe_adaptation_gym.py:133-139,
 * 174-223) and the hazard loop of World.compute_cost (world.py:147-153).
 *   robot   [n][3] f32 x, y, yaw          points [n][K][2] f32
 *   group   [n][K] u8: 0 inactive, 1 obstacle, 2 goal, 3 object (consts.py:13-16),
 *           +128 flags a hazard (tested for cost with hazard_size)
 *   lidar   [n][48] f32 = [obstacles, objects, goal]    bins [n][K] i32 (-1 =
 *           inactive)      cost [n] u8
 * Host pointers; synchronous. */
int sag_lidar_cost(sag_ctx* ctx, int32_t n, int32_t K, const float* robot,
                   const float* points, const uint8_t* group, float hazard_size,
                   float* lidar, int32_t* bins, uint8_t* cost);

/* The same kernel on DEVICE buffers of the context's device, enqueued on the context stream
 * without host copies or synchronisation (sag_wait joins); bracketed by the HIP events of
 * sag_enable_timing / sag_kernel_time_ms like a step launch.  d_bins may be NULL. */
int sag_lidar_cost_device(sag_ctx* ctx, int32_t n, int32_t K, const float* d_robot,
                          const float* d_points, const uint8_t* d_group, float hazard_size,
                          float* d_lidar, int32_t* d_bins, uint8_t* d_cost);

/* Device allocation helpers so NumPy-only hosts can keep action/observation
 * buffers resident (bench harness, GPU learners without torch). */
int sag_dev_alloc(sag_ctx* ctx, uint64_t bytes, void** dptr);
int sag_dev_free(sag_ctx* ctx, void* dptr);
int sag_dev_upload(sag_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int sag_dev_download(sag_ctx* ctx, void* dst, const void* src, uint64_t bytes);
/* Fill d_actions [n_envs][nu] with U(-1,1) from the counter-based generator
 * (stream = step index): the synthetic policy of the bench. */
int sag_dev_fill_actions(sag_ctx* ctx, float* d_actions, uint32_t step_index);

/* Timing of the step kernel alone, measured with HIP events on the context
 * stream: mean milliseconds per launch over the launches since the last call
 * with reset != 0.  Feeds bench.py's roofline.achieved. */
int sag_kernel_time_ms(sag_ctx* ctx, int32_t reset, double* mean_ms, int64_t* launches);
/* Diagnostic (tests): Doggo mass matrix [19x19], bias [19], contact-free qacc [19] and M^-1 [19x19]
 * per env from the wave-cooperative routines; out[n_envs][760] doubles. */
int sag_debug_doggo_coop(sag_ctx* ctx, double* out);

/* rgb_observation (safe_adaptation_gym.py:122-126 `physics.render(height=64, width=64,
 * camera_id='vision')`): the first-person image of every env at its current state,
 * out[n_envs][64][64][3] uint8 (row 0 = top).  Host buffer / device buffer variants. */
int sag_render_rgb(sag_ctx* ctx, uint8_t* out);
int sag_render_rgb_device(sag_ctx* ctx, void* d_out);

/* Human / debugging view (safe_adaptation_gym.py:109-111 render() with render_options, render.py,
 * mujoco_bridge.py:126-153): the same device ray caster with any of the scene's cameras -
 *   camera 0 the robot's `vision` camera, 1 `fixednear` (pos 0 -2 2, zaxis 0 -1 1), 2 `fixedfar` (0 -5 5),
 *          3 `track` (fixednear's view, following the robot body)
 * any image size, and with flags & 1 the overlays of render_lidars_and_collision: three rings of 16 spheres above
 * the robot (obstacles red, goal green, objects blue; alpha = min(1, lidar value + .1), safe_adaptation_gym.py:239-257)
 * and the red cost sphere.  out[n_envs][height][width][3] uint8, row 0 = top.  sag_render shows the observation / cost
 * of the context's last host-buffer step; the device variant takes them as (device) pointers or NULL. */
int sag_render(sag_ctx* ctx, int32_t camera, int32_t width, int32_t height, int32_t flags, uint8_t* out);
int sag_render_device(sag_ctx* ctx, int32_t camera, int32_t width, int32_t height, int32_t flags,
                      const float* d_obs, const uint8_t* d_cost, void* d_out);
/* A chosen subset of the envs.
 * as sag_render_device, for the envs with a non-zero byte of d_mask ([n_envs] device bytes, complete before the call;
 * NULL: every env = sag_render_device).  Rows of other envs in d_out are not written.  Stream-ordered, no wait. */
int sag_render_rows_device(sag_ctx* ctx, int32_t camera, int32_t width, int32_t height, int32_t flags,
                           const float* d_obs, const uint8_t* d_cost, const uint8_t* d_mask, void* d_out);
/* as sag_render, for n listed envs: out [n][height][width][3] host, row j = env env_ids[j] (host int32, any order,
 * duplicates allowed).  Overlays show rows env_ids[j] of the context's own observation / cost buffers, as sag_render.
 * The staging buffer is sized for n images, not n_envs.  n == 0: SAG_OK, nothing launched.
 * SAG_ERR_ARG, nothing launched: NULL pointers with n > 0, n < 0, an index outside [0, n_envs), bad camera / size. */
int sag_render_envs(sag_ctx* ctx, int32_t camera, int32_t width, int32_t height, int32_t flags,
                    const int32_t* env_ids, int32_t n, uint8_t* out);

/* Depth and segmentation images (physics.render(depth=True) / (segmentation=True) behind the reference's render_options):
 * the same ray caster, cameras, sizes and flags as sag_render, stating per pixel the NEAREST surface of any alpha - a
 * translucent hazard disc or goal cylinder is a surface; of two geoms at exactly one distance the earlier in the scene's
 * build order (hazards, vases, pillars, goal, buttons, task object, robot geoms, lidar rings, cost sphere); then the floor.
 *   SAG_RENDER_DEPTH         [rows][height][width] float: the distance from the camera plane in metres, as dm_control
 *                            linearises the z-buffer (not the ray's length): t / sqrt(1 + u^2 + v^2) for the pixel's ray
 *                            u X + v Y - Z, computed in double and rounded once.  Sky pixels hold SAG_DEPTH_SKY (MuJoCo's
 *                            default zfar taken as metres: the model's extent is not known here - parity unpinned, as for
 *                            the colour image).
 *   SAG_RENDER_SEGMENTATION  [rows][height][width][2] int32: channel 0 the instance, channel 1 the class (enum
 *                            sag_seg_class), mirroring dm_control's (objid, objtype); the sky is (-1, -1).
 * Row 0 = top. */
enum sag_render_output { SAG_RENDER_DEPTH = 1, SAG_RENDER_SEGMENTATION = 2 };
#define SAG_DEPTH_SKY 50.0f
enum sag_seg_class {
  SAG_SEG_FLOOR = 0,  /* instance 0                                                                         */
  SAG_SEG_HAZARD = 1, /* instance = the index in the record; so for VASE, PILLAR and BUTTON                 */
  SAG_SEG_VASE = 2,
  SAG_SEG_PILLAR = 3,
  SAG_SEG_GOAL = 4,   /* instance 0                                                                         */
  SAG_SEG_BUTTON = 5,
  SAG_SEG_OBJECT = 6, /* PushBox box 0 and its corner columns 1..4 in build order; rod or ball 0            */
  SAG_SEG_ROBOT = 7,  /* geom index in build order: Point 0 sphere, 1 arrow; Car 0..4 boxes, 5..6 wheels,   */
                      /* 7 rear ball; Doggo 0..13 in geom-table order                                       */
  SAG_SEG_LIDAR = 8,  /* instance = ring * 16 + bin; only with flags & 1                                    */
  SAG_SEG_COST = 9    /* instance 0; only with flags & 1 and the cost flag up                               */
};
/* Device buffer, stream-ordered, no wait, no timing events.  d_mask as in sag_render_rows_device: [n_envs] device bytes,
 * NULL = every env; env b goes into row b and rows of other envs are not written.  d_out: [n_envs] rows, aligned to 4 B
 * (depth) or 8 B (segmentation).  d_obs / d_cost: what the overlays show (device pointers or NULL).
 * SAG_ERR_ARG, nothing launched: an unknown output, bad camera / size, NULL or misaligned d_out. */
int sag_render_aux_device(sag_ctx* ctx, int32_t output, int32_t camera, int32_t width, int32_t height, int32_t flags,
                          const float* d_obs, const uint8_t* d_cost, const uint8_t* d_mask, void* d_out);
/* Host buffer: row j = env env_ids[j] (host int32, any order, duplicates allowed); env_ids == NULL: envs 0 .. n_envs - 1,
 * n is ignored.  Overlays show the context's own observation / cost rows, as sag_render.  The staging is sized for the rows
 * asked for and shared with sag_render / sag_render_envs.  n == 0: SAG_OK, nothing launched.
 * SAG_ERR_ARG, nothing launched: an unknown output, bad camera / size, NULL out with rows to write, n < 0, an index outside
 * [0, n_envs). */
int sag_render_aux(sag_ctx* ctx, int32_t output, int32_t camera, int32_t width, int32_t height, int32_t flags,
                   const int32_t* env_ids, int32_t n, void* out);

/* Diagnostic: how many envs the last split step handed to the busy kernel (0 for the
 * single-kernel form).  Synchronises the context stream. */
int sag_busy_count(sag_ctx* ctx, int32_t* count);
/* Diagnostic, only in libraries built with -DSAG_CYCLES (SAG_ERR_UNSUPPORTED otherwise):
 * wavefront clock ticks per code section of the step kernel, [3 launch forms][16]. */
int sag_debug_cycles(sag_ctx* ctx, int32_t reset, uint64_t* out, int32_t n);
/* Per-launch HIP-event bracketing of the step kernel is off by default. */
int sag_enable_timing(sag_ctx* ctx, int32_t on);

int sag_device_count(void);

/* ---- native reset path ------------------------------------------------
 * World.DEFAULT (world.py:17-34), the keys that influence sampling or the installed record. */
typedef struct sag_world_config {
  double placements_margin, robot_keepout, hazards_size, vases_size, pillars_size;
  double hazards_keepout, vases_keepout, pillars_keepout;
  double robot_ctrl_range_scale, action_noise, max_bound;
  int32_t random_bound, reserved;
} sag_world_config;
void sag_world_config_default(sag_world_config* cfg);

/* What the sampler needs to know about a Task object (tasks/task.py:14-97): the host mirror builds one from the
 * Task's own `obstacles`, `placement_extents`, `setup_placements()` and attributes (safe_adaptation_gym_amd/tasks), so a
 * subclass that overrides them changes the layouts; `task_id` selects the device-side per-step logic (compute_reward /
 * set_mocaps / on-goal reset), which cannot be overridden from Python.  Rectangles are (xmin, ymin, xmax, ymax). */
typedef struct sag_task_desc {
  int32_t task_id;                       /* enum sag_task */
  int32_t n_hazards, n_vases, n_pillars; /* Task.obstacles = [hazards, vases, gremlins (always 0), pillars] */
  int32_t has_goal;                      /* a 'goal' placement, re-drawn by GoToGoal.reset (go_to_goal.py:50-80) */
  int32_t box_kind;                      /* enum sag_box_kind; SAG_BOX_NONE: no task object */
  int32_t box_yaw;                       /* build_world_config draws a yaw for it (push_box.py; not roll_rod / dribble_ball) */
  int32_t box_at_robot;                  /* haul_box.py:17-18: after sampling the object sits at robot + (box_offset, 0) */
  int32_t n_buttons;
  int32_t button_reset;                  /* task.reset: 0 none, 1 rs.choice(n_buttons) + timer (press_buttons.py:71-77), 2 all active (collect.py) */
  int32_t button_timer;                  /* BUTTON_TICKING_DELAY */
  int32_t reserved;
  double extents[4];                     /* Task.placement_extents */
  double goal_keepout, box_keepout, button_keepout, box_offset;
  double box_rect[4];                    /* all zero: the extents (placement None) */
  double button_rect[4];
  double gear, damping;                  /* point.xml variants (go_to_goal_motor.py, go_to_goal_damping.py) */
} sag_task_desc;
/* the descriptor of one of the reference's 14 tasks; returns SAG_ERR_ARG for an unknown id */
int sag_task_desc_default(int32_t task_id, sag_task_desc* out);
/* NULL if the descriptor is one the sampler and the device can serve, else a static string naming the offending field
 * and the rule (capacities, button_timer 0..5 and 5 with button_reset 1, finite non-negative keep-outs, rectangles with
 * xmin < xmax and ymin < ymax or all zero, no goal together with buttons).  sag_sample_layouts_desc returns SAG_ERR_ARG
 * when this is not NULL for one of its descriptors. */
const char* sag_task_desc_check(const sag_task_desc* desc);

/* Replaces World.__init__ + sample_layout + _build_world_config + World.reset's host draws
 * (world.py:36-137,172-217; tasks' setup_placements/build_world_config/reset) for n envs on the
 * host cores.  Env j owns np.random.RandomState(seeds[j]) (exact legacy MT19937 stream, the
 * reference's draw order) and yields record j of include/sag.h, env id env_id0 + j.
 * first_episode != 0: the Task object is new (Cauchy ctrl-scale draw, world.py:72-73), else the
 * World persists (safe_adaptation_gym.py:105-106).  mt_* (each may be NULL) return the generator
 * after the draws (key [n][624], pos, has_gauss, gauss) so a parity harness can continue the
 * same stream in numpy.  status[j] (may be NULL): 0 ok, <0 ResamplingError.  Returns the number
 * of envs that failed, or a negative sag_status.  No GPU involved. */
int sag_sample_layouts(int32_t robot, int32_t n, const uint32_t* seeds, const int32_t* task_ids,
                       const sag_world_config* cfg, int32_t first_episode, int32_t env_id0,
                       float* rec_f, int32_t* rec_i, uint32_t* mt_key, int32_t* mt_pos,
                       int32_t* mt_has_gauss, double* mt_gauss, int32_t* status, int32_t nthreads);
/* The same with explicit task descriptors: env j uses descs[desc_of_env[j]] (n_descs of them).  sag_sample_layouts is
 * this call with the 14 default descriptors and desc_of_env = task_ids.  SAG_ERR_ARG if sag_task_desc_check rejects a
 * descriptor. */
int sag_sample_layouts_desc(int32_t robot, int32_t n, const uint32_t* seeds, const sag_task_desc* descs, int32_t n_descs,
                            const int32_t* desc_of_env, const sag_world_config* cfg, int32_t first_episode, int32_t env_id0,
                            float* rec_f, int32_t* rec_i, uint32_t* mt_key, int32_t* mt_pos,
                            int32_t* mt_has_gauss, double* mt_gauss, int32_t* status, int32_t nthreads);

/* ---- device reset path (throughput mode) -----------------------------------------------------
 * The same steps as sag_sample_layouts_desc (placements in the reference's dict order, keep-outs max(keepout, size),
 * margin + 0.165 for the Doggo, <= 1000 candidates per placement and 10 000 layout attempts, the draws after the layout,
 * the goal resample, task.reset) sampled on the device, with the words of the counter-based generator (context key,
 * stream 3) instead of the reference's MT19937: the layouts follow the host sampler's distribution, not its stream.
 * Parity mode keeps sag_sample_layouts.
 *
 * sag_set_tasks: the descriptor table (each checked with sag_task_desc_check and against the context's capacities),
 * env i's descriptor desc_of_env[i] ([n_envs], host) and the world config, kept on the device.  env_id0 is the global id
 * of the context's env 0 (SAG_I_ENV_ID, the generator's env word).  Call it when the task set changes. */
int sag_set_tasks(sag_ctx* ctx, const sag_task_desc* descs, int32_t n_descs, const int32_t* desc_of_env,
                  const sag_world_config* cfg, int32_t env_id0);
/* sag_reset_device: samples and installs new layouts on the context stream, without host records.
 *   first_episode != 0: new Task objects (Cauchy ctrl scale, random bound, fresh button state, catch radii 1 / .2 and timer);
 *                 0: SAG_F_CTRL_SCALE, SAG_F_BOUND, SAG_I_BTN_STATE, SAG_I_CATCH_TIMER and SAG_F_CATCH + 2, + 3 are kept
 *                 from the env's current state (needs an installed layout)
 *   episode0      the episode nonce of envs of a context that has no layout yet; otherwise each reset env's nonce
 *                 advances by one (as sag_reset), so an env never draws the same layout twice under one key.  A later
 *                 episode draws under the SAG_I_ENV_ID the env carries: env_id0 + i, unless sag_fork_device with
 *                 SAG_FORK_SAME_STREAM gave it its source's
 *   d_mask        [n_envs] DEVICE bytes: only envs with a non-zero byte are reset; NULL: every env.  A mask written on
 *                 another stream must be complete before the call.
 *   status        [n_envs] host, may be NULL: 0, -1 (layout attempts exhausted), -2 (goal resample exhausted); 0 for envs
 *                 not reset
 *   bound         [n_envs] host, may be NULL: every env's SAG_F_BOUND after the call (info['bound'])
 * Installation is sag_set_layout's (task.reset's `last` distances, overlap flags, cleared cost flag), and the layout store
 * of sag_reset holds the device-drawn records.  Returns the number of envs whose sampling failed - then NOTHING is
 * installed - or a negative sag_status.  Synchronous. */
int sag_reset_device(sag_ctx* ctx, int32_t first_episode, int32_t episode0, const uint8_t* d_mask, int32_t* status,
                     float* bound);

/* ---- the rollout loop on the context stream (throughput mode) ----------------------------------
 * step -> episode bookkeeping -> masked reset of the envs that ended -> step, without a host wait or copy:
 *   sag_step_device(..., d_obs, d_reward, d_cost, d_done, d_goal_met);
 *   sag_episode_track_device(ctx, d_reward, d_cost, d_done, d_goal_met, max_steps, d_ended, d_episode);
 *   sag_copy_rows_device(ctx, d_ended, obs_dim * 4, d_obs, d_final);   (optional: the final observations, before the
 *                                                                        reset overwrites the rows of the envs that ended)
 *   sag_reset_device_async(ctx, d_ended, d_obs);
 *
 * sag_reset_device_async: stream-ordered form of sag_reset_device(first_episode = 0): needs sag_set_tasks and an installed
 * layout.  Enqueued on the context stream, returns without waiting, no host copy.  d_mask as in sag_reset_device (NULL:
 * every env).  d_obs: [n_envs][obs_dim] f32 device buffer (16-byte aligned for the Doggo) or NULL; the rows of the envs
 * that were reset receive the observation of their new state (what sag_observe returns for them), no other row is written.
 * Commit is per env: an env whose sampling fails keeps its state, nonce, layout-store row, observation row and episode
 * accumulators, and bit 0 of its SAG_I_FLAGS is set (the ResamplingError bit).  No timing events are recorded
 * (sag_kernel_time_ms stays the step's figure).  Pending external contacts (sag_set_ext_contacts) are always dropped: the
 * host cannot know whether the mask was empty. */
int sag_reset_device_async(sag_ctx* ctx, const uint8_t* d_mask, float* d_obs);
/* Envs reset / envs whose sampling failed by sag_reset_device_async since the last call with clear != 0.
 * Synchronises the stream. */
int sag_reset_device_counts(sag_ctx* ctx, int32_t clear, uint64_t* n_reset, uint64_t* n_failed);

/* Episode bookkeeping after a step, on the context stream, all pointers device pointers [n_envs]
 * (d_reward [n_envs][2], column 0 is accumulated; d_episode [n_envs][4], 16-byte aligned).  Per env: ret += reward (one
 * fp32 add), cost += cost != 0, length += 1, goals += goal_met != 0;
 * ended = done ? 1 : (max_steps > 0 && length >= max_steps ? 2 : 0); d_ended[i] = ended (usable as a reset mask as it is).
 * If ended, d_episode[i] = {ret, cost, length, goals} as four floats and the accumulators return to zero.  Rows of envs
 * that did not end are not written.  The accumulators (one float4 per env) are allocated and zeroed on first use;
 * sag_reset_device_async zeroes those of the envs it commits. */
int sag_episode_track_device(sag_ctx* ctx, const float* d_reward, const uint8_t* d_cost, const uint8_t* d_done,
                             const uint8_t* d_goal_met, int32_t max_steps, uint8_t* d_ended, float* d_episode);
/* Zero the accumulators of the masked envs (NULL: all), stream-ordered. */
int sag_episode_clear(sag_ctx* ctx, const uint8_t* d_mask);
/* For the envs with a non-zero byte of d_mask ([n_envs] device bytes; NULL: every env) copy row i
 * (row_bytes bytes) of d_src to row i of d_dst.  Stream-ordered, returns without waiting, no host copy,
 * no timing events.  SAG_ERR_ARG with nothing enqueued: NULL d_src / d_dst, row_bytes <= 0 or not a
 * multiple of 16, a pointer that is not 16-byte aligned, d_src == d_dst. */
int sag_copy_rows_device(sag_ctx* ctx, const uint8_t* d_mask, int32_t row_bytes, const void* d_src, void* d_dst);

/* ---- a time-major rollout buffer on the context stream (throughput mode) -------------------------
 * The step takes arbitrary device pointers, so T steps of experience need no copy: step t writes plane t of [T][pitch]...
 * arrays (pitch >= n_envs envs per plane), and per step
 *   sag_step_device(ctx, actions[t], NULL, -1, obs[t + 1], reward[t], cost[t], terminated[t], goal_met[t]);
 *   sag_episode_track_device(ctx, reward[t], cost[t], terminated[t], goal_met[t], max_steps, ended[t], episode[t]);
 *   sag_append_rows_device(ctx, ended[t], obs_dim * 4, obs[t + 1], d_store, capacity, d_count, t == 0, slot[t]);
 *   sag_reset_device_async(ctx, ended[t], obs[t + 1]);
 * keeps the final observations of the episodes that ended - the few rows a learner bootstraps from after a truncation -
 * compacted in d_store; after T steps sag_gae_device turns stored rewards, costs, `ended` bytes and the learner's values into
 * advantages and returns of both channels.  Both calls are enqueued on the context stream and return without waiting; they copy
 * nothing to the host, record no timing events and need no installed layout.
 *
 * sag_append_rows_device: the compacting sibling of sag_copy_rows_device.  For each env i with a non-zero byte of d_mask
 * ([n_envs] device bytes, required) row i of d_src (row_bytes bytes, a multiple of 16; both buffers 16-byte aligned) is
 * appended to d_store ([capacity][row_bytes]) at slot s, and d_slot[i] = s.  d_slot ([n_envs] int32) is written for EVERY env:
 * -1 where the mask byte is zero or the row did not fit.  d_count is one device int32, the number of slots claimed so far: it
 * may exceed capacity - a claim at or beyond capacity writes no row and gets slot -1 -, so min(count, capacity) rows of the
 * store are valid and max(0, count - capacity) rows were dropped.  restart != 0 sets the counter to zero on the stream before
 * the append.  Claiming costs one returning atomic add per wavefront (64 consecutive envs) that has any set lane: inside such
 * a group of 64 envs the slots ascend with the env index; the order BETWEEN groups is unspecified and may differ from run to
 * run - d_slot is the only map from envs to rows.  Rows of the store that no claim reached are not written.
 * SAG_ERR_ARG with nothing enqueued: a NULL pointer, row_bytes <= 0 or not a multiple of 16, d_src or d_store not 16-byte
 * aligned, d_src == d_store, capacity < 1, d_count or d_slot not 4-byte aligned. */
int sag_append_rows_device(sag_ctx* ctx, const uint8_t* d_mask, int32_t row_bytes, const void* d_src, void* d_store,
                           int32_t capacity, int32_t* d_count, int32_t restart, int32_t* d_slot);

/* sag_gae_device: generalised advantage estimation for the reward channel and, when d_cvalue is given, the cost channel.
 * Every array is a device array; time-major ones have `pitch` >= n_envs elements per step, of which the first n_envs are
 * read or written (the rest is never touched).
 *   d_reward [T][pitch][2] f32 (column 0 is used; 8-byte aligned)     d_cost [T][pitch] u8      d_ended [T][pitch] u8: 0, 1
 *   (terminated) or 2 (truncated), as sag_episode_track_device writes it      d_value, d_cvalue [T + 1][pitch] f32 (d_cvalue
 *   NULL: no cost channel)      d_slot [T][pitch] int32 or NULL: the slots of sag_append_rows_device      d_final_value,
 *   d_final_cvalue [capacity] f32 or NULL: the learner's values of the rows of that store
 *   outputs d_adv, d_ret, d_cadv, d_cret [T][pitch] f32; the cost outputs are required exactly when d_cvalue is given.
 * Per env, carry = 0 and t = T - 1 ... 0, in fp32 with every operation rounded on its own (no fused multiply-add), and
 * gl = gamma * lam rounded once:
 *   e = ended[t]
 *   e == 0:                                                            nv = value[t + 1]            (carry stays)
 *   e == 2, d_slot and d_final_value given, 0 <= slot[t] < capacity:   nv = final_value[slot[t]];   carry = 0
 *   otherwise (terminated, or truncated without a kept final row):     nv = 0;                      carry = 0
 *   q = gamma * nv;  s = r + q;  delta = s - value[t];  p = gl * carry;  A = delta + p;  ret = A + value[t]
 *   adv[t] = A;  ret[t] = ret;  carry = A
 * with r = reward[t][0].  The cost channel is the same recurrence with r = (cost[t] != 0 ? 1 : 0), d_cvalue, d_final_cvalue,
 * cost_gamma and cost_lam.  value[t + 1] of an env that ended at t belongs to the new episode and is not read for it.
 * SAG_ERR_ARG with nothing enqueued: a NULL desc or required array, T < 1, pitch < n_envs, one of the four gammas / lambdas
 * outside [0, 1] or not finite, d_reward not 8-byte or another array not 4-byte aligned, cost outputs without d_cvalue or
 * d_cvalue without both cost outputs, d_slot with capacity < 1. */
typedef struct sag_gae_desc {
  int32_t T, pitch, capacity, reserved;
  float gamma, lam, cost_gamma, cost_lam;
  const float* d_reward;
  const uint8_t* d_cost;
  const uint8_t* d_ended;
  const float* d_value;
  const float* d_cvalue;
  const int32_t* d_slot;
  const float* d_final_value;
  const float* d_final_cvalue;
  float* d_adv;
  float* d_ret;
  float* d_cadv;
  float* d_cret;
} sag_gae_desc;
int sag_gae_device(sag_ctx* ctx, const sag_gae_desc* desc);

/* ---- a Gaussian actor-critic MLP on the context stream (throughput mode) --------------------------
 * sag_policy_forward_device: one fused forward of a two-hidden-layer MLP with a shared trunk and three heads,
 *   obs [n_rows][obs_dim] -> hidden -> hidden -> nu + 2 outputs = action mean (nu), reward value, cost value,
 * with obs_dim and nu the context's robot's.  One launch reads each observation row once and writes only the outputs; enqueued
 * on the context stream, it returns without waiting, copies nothing to the host, records no timing events and needs no layout.
 * What with the rollout buffer above closes the model-free loop on the device: the policy writes actions[t], logp[t], value[t]
 * and cost_value[t] from obs[t], the step reads actions[t].
 *
 * d_params: contiguous fp32 in natural (row-major) layout, H = hidden:
 *   W1[obs_dim][H]  b1[H]  W2[H][H]  b2[H]  W3[H][nu + 2]  b3[nu + 2]  std[nu]
 * d_obs: n_rows rows of obs_pitch >= obs_dim floats (obs_pitch a multiple of 4, d_obs 16-byte aligned); rows at or beyond
 * n_rows and the pad columns are not read.  n_rows is arbitrary (a final-observation store is not n_envs rows).
 * Outputs, any of which may be NULL: d_actions [n_rows][nu], d_logp, d_value, d_cvalue [n_rows]; rows at or beyond n_rows are
 * not written.
 *
 * The defined arithmetic.  Every unit j of every layer, in fp32:
 *   acc = bias[j];   for k = 0 ... K - 1 in ascending order: acc = fmaf(x[k], W[k][j], acc);   y[j] = act(acc)
 * (one rounding per product - the fp32-input matrix instruction computes exactly this chain); the head has no activation.
 *   SAG_POLICY_RELU: act(x) = x > 0 ? x : 0
 *   SAG_POLICY_TANH: act(x) = 1 - 2 * rcp(exp2(c * x) + 1), c = 2 log2(e) rounded to fp32, with the hardware exp2 and
 *                    reciprocal (1 ulp-class) and every operation rounded on its own
 * Sampling: a[u] = mean[u] + std[u] * z[u], the product and the sum rounded separately, written UNCLAMPED (the step clips; a
 * learner needs the raw sample).  z[u] is a standard normal of the counter-based generator under the context key (sag_set_seed)
 * on stream 5: the Philox4x32-10 block of the counter
 *   word 0 = env_id0 (sag_set_tasks; 0 without tasks) + row0 + row    word 1 = draw    word 2 = u / 4    word 3 = 0x14000000
 * gives u % 4 = 0, 1 the two normals (cos, sin) of the Box-Muller transform of its words 0, 1 and u % 4 = 2, 3 those of its
 * words 2, 3, as sag_plan_sample_device maps them.  Word 3 is stream 5 placed above the 26 bits of streams 0 - 3.
 *   logp = -(0.5f * sum_u z[u]^2) - logp_const, the sum in ascending u in fp32, each square and each sum rounded;
 *   logp_const = sum_u log(std[u]) + nu * 0.5 * log(2 pi), rounded once by the caller.
 * With SAG_POLICY_MEAN in flags, or with d_actions == NULL (the value-only evaluation), nothing is sampled: z = 0, the actions
 * are the mean exactly and logp = -logp_const.
 * SAG_ERR_ARG with nothing enqueued: a NULL desc, d_params or d_obs; d_obs not 16-byte aligned, d_params or an output not
 * 4-byte aligned; hidden not a multiple of 32 in 32 ... 256; an unknown activation or flag bit; obs_pitch < obs_dim or not a
 * multiple of 4; n_rows < 1; a logp_const that is not finite. */
enum sag_policy_activation { SAG_POLICY_RELU = 0, SAG_POLICY_TANH = 1 };
enum sag_policy_flags { SAG_POLICY_MEAN = 1 };
typedef struct sag_policy_desc {
  int32_t n_rows, hidden, activation, flags;
  int32_t obs_pitch, reserved;
  uint32_t draw, row0;
  float logp_const;
  const float* d_params;
  const float* d_obs;
  float* d_actions;
  float* d_logp;
  float* d_value;
  float* d_cvalue;
} sag_policy_desc;
int sag_policy_forward_device(sag_ctx* ctx, const sag_policy_desc* desc);

/* ---- the PPO-Lagrangian update of that MLP on the context stream (throughput mode) ----------------
 * sag_policy_backward_device: the gradient of a clipped-surrogate actor loss, two critic losses and an entropy bonus through
 * the network of sag_policy_forward_device, over rows stored the way the rollout buffer stores them; sag_adam_device: the
 * optimiser step.  Both are enqueued on the context stream and return without waiting; they copy nothing to the host, record
 * no timing events and need no installed layout (the one exception: a call that has to grow the context's workspace - the
 * first one, or one with a larger grid or more parameters than any before - synchronises the stream once, as
 * sag_plan_shift_device does).
 *
 * Inputs: n_planes planes of `pitch` >= n_rows rows each; in every plane the first n_rows rows are read, the rest is never
 * touched.  Row g of the batch (0 <= g < n_planes * n_rows) is row g % n_rows of plane g / n_rows.
 *   d_obs [n_planes][pitch][obs_pitch] f32 (16-byte aligned, obs_pitch a multiple of 4 and >= obs_dim; pad columns not read)
 *   d_actions [n_planes][pitch][nu]     d_logp_old, d_adv, d_ret [n_planes][pitch]
 *   d_cadv, d_cret [n_planes][pitch], each may be NULL: then its term is absent (cadv counts as cadv_sub; no cost critic loss,
 *   statistic 2 is zero)                d_params as sag_policy_forward_device
 * Output: d_grad [n_params + 8] f32 - the gradient in the parameter layout (W1 b1 W2 b2 W3 b3 std), then 8 statistics.
 *
 * The defined function.  Per row, with mean, v, cv the forward's chain recomputed (no activation is read from memory):
 *   zeta[u] = (a[u] - mean[u]) / std[u]
 *   logp = -0.5 * sum_u zeta[u]^2 - sum_u log(std[u]) - nu / 2 * log(2 pi)      (the log sum is formed on the device)
 *   rho  = exp(logp - logp_old)
 *   A    = adv_mul * (adv - adv_sub) - cadv_mul * (cadv - cadv_sub)
 *   live = (A >= 0 && rho <= 1 + clip) || (A < 0 && rho >= 1 - clip)
 *   L    = -(live ? rho : clamp(rho, 1 - clip, 1 + clip)) * A + vf_coef * 0.5 * (v - ret)^2 + cvf_coef * 0.5 * (cv - cret)^2
 *          - ent_coef * sum_u log(std[u])
 *   grad = scale * sum over rows of dL / dtheta for every entry of W1 b1 W2 b2 W3 b3 std (for std: the derivative with respect
 *          to std itself, not its logarithm)
 * A row that is not live contributes nothing through logp.  The ReLU derivative is (z > 0) on the forward's own fp32
 * pre-activation, the tanh derivative 1 - h^2 on the forward's h.  `scale` is the caller's 1 / (rows of the whole batch), so
 * that calls over parts of a batch add up to the batch mean.  The statistics, each times scale:
 *   0 sum(-surrogate)   1 sum(0.5 (v - ret)^2)   2 sum(0.5 (cv - cret)^2)   3 sum(logp_old - logp)   4 rows not live
 *   5 rows              6, 7 zero
 * With SAG_POLICY_GRAD_ACCUMULATE all n_params + 8 words are added to what d_grad holds; without it they replace it.
 *
 * Determinism: the same inputs, library and device give the same bits in d_grad on every call; there are no floating-point
 * atomics.  grid = min(ceil(n_planes * n_rows / 32), max_blocks > 0 ? min(max_blocks, 1024) : 256) persistent blocks; block b
 * takes the tiles of 32 consecutive rows b, b + grid, ... in that order and writes one partial into a workspace owned by the
 * context (freed with it); a final pass computes d_grad[i] = old + scale * partial[0][i] + scale * partial[1][i] + ... in
 * ascending block order, `old` being d_grad[i] under ACCUMULATE and 0 otherwise.  The grid is a function of n_planes * n_rows
 * and max_blocks only; the order of the sums inside a block is not part of the ABI, and unlike the forward this function is
 * defined to a tolerance, not bit for bit (exp, log and the reciprocal are the hardware's 1 ulp-class ones).
 *
 * hidden: 32 ... 128 for every robot.  160 ... 256 return SAG_ERR_UNSUPPORTED (the weight-gradient accumulators of a block stay
 * in registers; beyond 128 they do not fit).
 * SAG_ERR_ARG with nothing enqueued: a NULL desc, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret or d_grad; d_obs not
 * 16-byte or another array not 4-byte aligned; hidden not a multiple of 32 in 32 ... 256; an unknown activation or flag bit;
 * obs_pitch < obs_dim or not a multiple of 4; n_rows < 1, n_planes < 1 or pitch < n_rows; max_blocks < 0; clip outside (0, 1);
 * a coefficient or scale that is not finite. */
enum sag_policy_grad_flags { SAG_POLICY_GRAD_ACCUMULATE = 1 };
typedef struct sag_policy_grad_desc {
  int32_t n_rows, n_planes, pitch, obs_pitch;
  int32_t hidden, activation, flags, max_blocks;
  float clip, vf_coef, cvf_coef, ent_coef;
  float adv_mul, adv_sub, cadv_mul, cadv_sub;
  float scale, reserved;
  const float* d_params;
  const float* d_obs;
  const float* d_actions;
  const float* d_logp_old;
  const float* d_adv;
  const float* d_ret;
  const float* d_cadv;
  const float* d_cret;
  float* d_grad;
} sag_policy_grad_desc;
int sag_policy_backward_device(sag_ctx* ctx, const sag_policy_grad_desc* desc);

/* sag_adam_device: one Adam step on n elements of d_param, d_grad, d_m and d_v, in fp32 with every operation rounded on its
 * own (no fused multiply-add) and correctly rounded sqrt and division:
 *   m   = fl(fl(beta1 * m) + fl(fl(1 - beta1) * g))
 *   v   = fl(fl(beta2 * v) + fl(fl(fl(1 - beta2) * g) * g))
 *   den = fl(sqrt(v) + eps)
 *   p   = fl(p - fl(fl(step * m) / den))
 *   for index >= clamp_first:  p = p > clamp_lo ? p : clamp_lo
 * step = lr * sqrt(1 - beta2^t) / (1 - beta1^t), rounded once by the caller; clamp_first == n clamps nothing (an MLP's std sits
 * at the end of its parameters: clamp_first = n_params - nu keeps it at or above clamp_lo).
 * SAG_ERR_ARG with nothing enqueued: a NULL desc or pointer, one not 4-byte aligned; n < 1; clamp_first outside [0, n]; beta1 or
 * beta2 outside [0, 1); eps <= 0; a step or clamp_lo that is not finite. */
typedef struct sag_adam_desc {
  int32_t n, clamp_first;
  float beta1, beta2, eps, step, clamp_lo, reserved;
  float* d_param;
  const float* d_grad;
  float* d_m;
  float* d_v;
} sag_adam_desc;
int sag_adam_device(sag_ctx* ctx, const sag_adam_desc* desc);

/* ---- what a learner needs around the backward pass: moments, the mixed advantage, the multiplier, the clip ----------
 * Four functions over device arrays whose results stay on the device for a later call on the same stream.  Each is enqueued on
 * the context stream and returns without waiting; none copies to the host, records timing events or needs an installed layout
 * (the one exception, as above: a call of sag_moments_device or sag_grad_clip_device that has to grow the context's workspace
 * - the first one, or one with a larger grid than any before - synchronises the stream once).  No floating-point atomics: the
 * same inputs, library and device give the same bits on every call.
 *
 * Pitched arrays: n_planes planes of `pitch` >= n_rows rows; logical element e (0 <= e < n_planes * n_rows) is row
 * r = e % n_rows of plane p = e / n_rows.  Pad rows (r >= n_rows) are never read or written.
 *
 * The reductions' grid rule (sag_moments_device, sag_grad_clip_device): a block's unit of work is a chunk of 4096 consecutive
 * logical elements; grid = min(ceil(elements / 4096), max_blocks > 0 ? min(max_blocks, 1024) : 256) blocks of 256 threads;
 * block b takes the chunks b, b + grid, ... in that order and writes one partial (an fp32 sum, and an integer count) into a
 * workspace owned by the context (freed with it); the partials are then added in ascending block order.  The grid is a
 * function of the element count and max_blocks only.  The order of the sums inside a block is not part of the ABI, so the two
 * reductions are defined to a tolerance, not bit for bit.
 *
 * sag_moments_device: count, mean, population variance and reciprocal deviation of one column of a pitched array.
 *   d_x     f32; element (p, r) is at float offset (p * pitch + r) * stride.  stride = 1 for a plain [n_planes][pitch] array
 *           (then it is streamed with 16-byte loads wherever four elements of one plane start at a 16-byte boundary);
 *           stride = 4 with d_x = episode + 1 reads the cost column of the rollout buffer's [T][pitch][4] episode rows.  The
 *           other columns of a strided row are never read.
 *   d_mask  [n_planes][pitch] u8 or NULL: element (p, r) counts where its byte is non-zero (with NULL: every element).  An
 *           element that does not count is never read into the arithmetic: a NaN there, in a pad row or in another column
 *           does not reach the output.
 *   d_out   [4] f32 = {count, mean, var, rstd}:
 *             count  the counting elements, accumulated as integers and converted to f32 once
 *             mean   sum(x) / count
 *             var    sum((x - mean)^2) / count, a second pass over the array that reads the fp32 mean the first one wrote
 *             rstd   1 / (sqrt(var) + eps), sqrt and the division correctly rounded
 *           count == 0 gives {0, 0, 0, 0}.
 * SAG_ERR_ARG with nothing enqueued: a NULL desc, d_x or d_out; d_x or d_out not 4-byte aligned; n_rows, n_planes or
 * stride < 1; pitch < n_rows; n_planes * n_rows >= 2^31; max_blocks < 0; eps negative or not finite. */
typedef struct sag_moments_desc {
  int32_t n_rows, n_planes, pitch, stride;
  int32_t max_blocks, reserved;
  float eps, reserved_f;
  const float* d_x;
  const uint8_t* d_mask;
  float* d_out;
} sag_moments_desc;
int sag_moments_device(sag_ctx* ctx, const sag_moments_desc* desc);

/* sag_advantage_mix_device: the advantage the backward pass is given, elementwise over [n_planes][pitch] f32 arrays and
 * defined bit for bit - every operation rounded on its own, no fused multiply-add:
 *   a = adv;   adv_mode 1: a = fl(a - m_a);   adv_mode 2: a = fl(fl(a - m_a) * s_a)
 *   c = cadv;  cadv_mode likewise with m_c, s_c
 *   out = d_cadv ? fl(a - fl(lam * c)) : a
 * m_a, s_a are words 1 and 3 (mean, rstd) of d_adv_mom, m_c, s_c those of d_cadv_mom: arrays as sag_moments_device writes
 * them, required where the mode is above 0 (d_cadv_mom only with d_cadv).  lam = d_lambda ? d_lambda[0] : cost_weight - word
 * 0 of sag_lagrange_device's state is such a d_lambda.  Modes: 0 raw, 1 centred, 2 standardised.  d_out may be d_adv or
 * d_cadv itself (an element is read before it is written) but may not overlap them otherwise.
 * SAG_ERR_ARG with nothing enqueued: a NULL desc, d_adv or d_out; a moments array missing for its mode; a pointer not 4-byte
 * aligned; n_rows or n_planes < 1; pitch < n_rows; n_planes * n_rows >= 2^31; a mode outside 0 ... 2; a cost_weight that is not
 * finite. */
enum sag_advantage_mode { SAG_ADV_RAW = 0, SAG_ADV_CENTER = 1, SAG_ADV_STANDARDIZE = 2 };
typedef struct sag_advantage_mix_desc {
  int32_t n_rows, n_planes, pitch, reserved;
  int32_t adv_mode, cadv_mode;
  float cost_weight, reserved_f;
  const float* d_adv;
  const float* d_cadv;      /* NULL: no cost term */
  const float* d_adv_mom;
  const float* d_cadv_mom;
  const float* d_lambda;    /* NULL: cost_weight */
  float* d_out;
} sag_advantage_mix_desc;
int sag_advantage_mix_device(sag_ctx* ctx, const sag_advantage_mix_desc* desc);

/* sag_lagrange_device: one projected ascent step of the Lagrange multiplier, bit for bit (one small launch).
 *   d_mom    [4] f32: the moments of the costs of the episodes that ended (sag_moments_device over the episode rows' cost
 *            column under the `done` mask); words 0 (count) and 1 (mean) are read
 *   d_state  [4] f32 = {lambda, last mean cost, last episode count, updates taken}
 * With count > 0:  t = fl(lambda + fl(lr * fl(mean - budget)));  t = t > 0 ? t : 0;  lambda = t < lambda_max ? t : lambda_max
 * (a NaN t becomes 0); word 1 = mean, word 2 = count, word 3 = fl(word 3 + 1).
 * With count == 0 only word 2 becomes 0: lambda, the last mean and the number of updates stay.
 * SAG_ERR_ARG with nothing enqueued: a NULL desc, d_mom or d_state, one not 4-byte aligned; lr or budget not finite; lr < 0;
 * lambda_max < 0 or NaN (+infinity is allowed: no upper clamp). */
typedef struct sag_lagrange_desc {
  float lr, budget, lambda_max, reserved;
  const float* d_mom;
  float* d_state;
} sag_lagrange_desc;
int sag_lagrange_device(sag_ctx* ctx, const sag_lagrange_desc* desc);

/* sag_grad_clip_device: global-norm clipping of d_grad[0 ... n) in place, the clip_grad_norm_ convention:
 *   norm   = sqrt(sum g^2)                        (the grid rule above over n elements; sqrt correctly rounded)
 *   factor = min(1, max_norm / (norm + 1e-6))     (fp32, the division correctly rounded)
 *   g      = fl(g * factor);  with factor == 1 nothing is written and every bit of d_grad stays
 *   d_out  [2] f32 = {norm, factor}; it must not overlap d_grad[0 ... n)
 * Words of d_grad at and behind n are not touched (the learner passes n_params: the 8 statistics behind the gradient stay).
 * A norm that is not finite is not special-cased, as in the convention: an infinite norm gives factor 0 (finite elements
 * become 0, infinite ones NaN), a NaN norm gives a NaN factor and with it NaN in every element.
 * Two launches: the partials; then every block adds them in ascending order and scales the chunks that are its own.
 * SAG_ERR_ARG with nothing enqueued: a NULL desc, d_grad or d_out, one not 4-byte aligned; n < 1; max_blocks < 0; max_norm
 * negative or not finite; d_out inside d_grad[0 ... n). */
typedef struct sag_grad_clip_desc {
  int32_t n, max_blocks;
  float max_norm, reserved;
  float* d_grad;
  float* d_out;
} sag_grad_clip_desc;
int sag_grad_clip_device(sag_ctx* ctx, const sag_grad_clip_desc* desc);

/* ---- observation normalisation on the context stream (throughput mode) ----------------------------
 * Running per-column moments of stored observation rows, the table made from them, and the forward and backward of the MLP
 * above with every observation element normalised where it is staged - no separate normalising pass writes or re-reads a row.
 * Each of the three functions is enqueued on the context stream and returns without waiting; none copies to the host, records
 * timing events or needs an installed layout (the one exception, as above: the first sag_obs_stats_device of a context
 * allocates its workspace; sag_policy_backward_norm_device shares sag_policy_backward_device's).  No floating-point atomics.
 *
 * sag_obs_stats_device: the moments of a batch of rows, merged into a running state, and the table of that state.
 *   d_obs    [n_planes][pitch][obs_pitch] f32, 16-byte aligned, obs_pitch >= obs_dim (the context's robot's) and a multiple
 *            of 4.  The first n_rows rows of every plane count; pad rows and pad columns are never read into a register that
 *            the arithmetic uses: a NaN there does not reach the output.
 *   d_state  [1 + 2 obs_dim] f64 = {count, mean[obs_dim], M2[obs_dim]}, 8-byte aligned, owned by the caller; all zeros is the
 *            empty state.
 *   d_table  [2][obs_dim] f32 = the mean row, then the rstd row; 16-byte aligned.
 * The defined function, per column k, with n_b = n_planes * n_rows:
 *   mean_b = sum(x) / n_b                                   s = (float)mean_b
 *   M2_b   = max(0, sum((x - s)^2) - n_b * (mean_b - s)^2)  a second pass over the array (the two-pass form of
 *            sag_moments_device; the shift s is what a block can subtract in fp32, the correction term restores mean_b)
 * Inside a block the sums are fp32 (x - s and its square each rounded); the per-block partials are added in ascending block
 * order in fp64, and everything from there on is fp64 with every operation rounded on its own:
 *   n = n_a + n_b    w = n_b / n    delta = mean_b - mean_a
 *   mean = mean_a + delta * w                               M2 = (M2_a + M2_b) + (delta * delta) * (n_a * w)
 * (Chan et al.; an empty state has w = 1 and takes the batch's moments exactly).  Then, given the state, bit for bit:
 *   table.mean[k] = (float)mean      table.rstd[k] = (float)(1.0 / sqrt(M2 / n + (double)eps))
 * the (x - mean) / sqrt(var + eps) convention with the population variance; the fp64 sqrt and division are correctly rounded.
 * A count that is not above 0 after the call writes mean 0 and rstd 1 (the identity).
 * With SAG_OBS_STATS_TABLE_ONLY in flags d_obs may be NULL and is not read, the state is not touched and the table is
 * rewritten from it (n_rows, n_planes, pitch, obs_pitch and max_blocks are ignored): what a checkpoint restore uses, so that
 * the table always comes from the same device arithmetic.
 * The grid rule: a block's unit of work is a chunk of 1024 consecutive logical rows (row e is row e % n_rows of plane
 * e / n_rows); grid = min(ceil(n_b / 1024), max_blocks > 0 ? min(max_blocks, 1024) : 1024) blocks of 256 threads; block b takes
 * the chunks b, b + grid, ... in that order and writes one [obs_dim] partial per pass into a workspace owned by the context
 * (freed with it).  The order of the sums inside a block is not part of the ABI, so the moments are defined to a tolerance;
 * the same inputs, library and device give the same bits on every call.
 * SAG_ERR_ARG with nothing enqueued and state and table untouched: a NULL desc, d_state or d_table; a NULL d_obs without
 * TABLE_ONLY; d_obs or d_table not 16-byte, d_state not 8-byte aligned; n_rows or n_planes < 1; pitch < n_rows;
 * n_planes * n_rows >= 2^31; obs_pitch < obs_dim or not a multiple of 4; max_blocks < 0; eps not finite or <= 0; an unknown
 * flag bit. */
enum sag_obs_stats_flags { SAG_OBS_STATS_TABLE_ONLY = 1 };
typedef struct sag_obs_stats_desc {
  int32_t n_rows, n_planes, pitch, obs_pitch;
  int32_t max_blocks, flags;
  float eps, reserved;
  const float* d_obs;
  double* d_state;
  float* d_table;
} sag_obs_stats_desc;
int sag_obs_stats_device(sag_ctx* ctx, const sag_obs_stats_desc* desc);

/* sag_policy_forward_norm_device, sag_policy_backward_norm_device: sag_policy_forward_device and sag_policy_backward_device
 * under the unchanged descriptors; everything those define holds - the chains, the sampling, the grid rule, the limits
 * (backward: hidden <= 128, SAG_ERR_UNSUPPORTED above), the determinism, the refusals - except that every observation element
 * x of column k is replaced, where the row is staged, by
 *   xh = fl(fl(x - mean[k]) * rstd[k]);   xh = xh < -clip ? -clip : xh;   xh = xh > clip ? clip : xh
 * with no contraction, bit for bit (a NaN passes through).  d_table is [2][obs_dim] f32 as sag_obs_stats_device writes it.
 * The zero-filled rows of a partial tile (at or beyond the last row) stay zero and are not normalised.  clip = +infinity
 * clamps nothing.
 * Additional refusals (SAG_ERR_ARG, nothing enqueued): d_table NULL or not 16-byte aligned; clip <= 0 or NaN. */
int sag_policy_forward_norm_device(sag_ctx* ctx, const sag_policy_desc* desc, const float* d_table, float clip);
int sag_policy_backward_norm_device(sag_ctx* ctx, const sag_policy_grad_desc* desc, const float* d_table, float clip);

/* ---- shuffled-row minibatches on the context stream (throughput mode) ------------------------------
 * A random permutation written on the device and the backward pass over a list of rows: what a learner needs to draw every
 * epoch's minibatches from a fresh shuffle of all T x N stored rows without an upload, a sort or a gathered copy of the batch.
 * Both are enqueued on the context stream and return without waiting; neither copies to the host, records timing events or
 * needs an installed layout (sag_policy_backward_rows_device shares sag_policy_backward_device's workspace and its one
 * exception).  No atomics.
 *
 * sag_permutation_device: d_index[i] = pi(i) for 0 <= i < n, one 4-byte store per element; nothing at or behind d_index + n is
 * touched.  pi is a bijection of [0, n) defined bit for bit - the same key (sag_set_seed), draw and n give the same array on
 * every call and device:
 *   b = max(2, bit length of (n - 1)); the walk domain is 2^b, so n <= 2^b and, for n > 2, 2^b < 2 n.
 *   F is an unbalanced Feistel network of 6 rounds on b-bit words: wl = b / 2 (floor), wr = b - wl, L = x >> wr,
 *   R = x & (2^wr - 1); round r = 0 ... 5:
 *     f = word 0 of Philox4x32-10(counter = {R, draw, r, 0x18000000}, the context key) & (2^wl - 1)
 *     (L, R) <- (R, L ^ f), then wl and wr change places
 *   F(x) = (L << wr) | R with the widths as they stand after the last round (six is even: the starting ones).  Counter word 3
 *   is stream 6, placed where streams 4 (0x10000000, the planner) and 5 (0x14000000, the policy) sit.
 *   Cycle walking: x = i; do x = F(x) while x >= n; pi(i) = x.  The walk ends because F permutes [0, 2^b).
 * pi is a keyed pseudo-random permutation, not a uniform draw from all n! orders.  Below about 16 elements the halves are 1 to
 * 2 bits wide and the distribution over the draws is visibly non-uniform (n = 5: chi^2 / dof of the position x value table
 * 7 to 9, where n = 130 gives 1.0 within its noise): at those sizes the function promises a bijection and nothing more.  The caller advances
 * `draw` from call to call.
 * SAG_ERR_ARG with nothing enqueued: a NULL ctx or d_index; d_index not 4-byte aligned; n < 1. */
int sag_permutation_device(sag_ctx* ctx, int32_t n, uint32_t draw, int32_t* d_index);

/* sag_policy_backward_rows_device: sag_policy_backward_device over a list of rows.  `desc` describes the planes exactly as
 * there; batch row j (0 <= j < n_index) is logical element e = d_rows[j] of those planes - row e % n_rows of plane
 * e / n_rows - read in place: no gathered copy is written.  With d_table == NULL the rows are read raw and obs_clip is ignored;
 * otherwise they are normalised where they are staged, as sag_policy_backward_norm_device does.
 *   d_rows  [n_index] DEVICE int32, 4-byte aligned, complete before the call in stream order (sag_permutation_device on the
 *           same stream writes such a list; a slice d_index + a of it is a minibatch).  An entry outside
 *           [0, n_planes * n_rows) is a row that is absent: nothing is read for it, it adds nothing to the gradient or the
 *           statistics, and statistic 5 (the rows that took part) does not count it - a wrong list cannot read outside the
 *           arrays.  Duplicates are allowed and count once each.
 * The grid and tiling rule is sag_policy_backward_device's with n_index in the place of n_planes * n_rows: tiles are 32
 * consecutive list entries, taken by the persistent blocks in the same order and followed by the same reduce.  Consequently
 * the list 0, 1, ..., n_planes * n_rows - 1 gives the bits of sag_policy_backward_device (with a table: of
 * sag_policy_backward_norm_device) under the same desc.  `scale` is the caller's - 1 / n_index for a minibatch's mean.
 * SAG_ERR_ARG with nothing enqueued: everything the contiguous calls refuse; a NULL d_rows or one not 4-byte aligned;
 * n_index < 1; with a table: d_table not 16-byte aligned, obs_clip not finite or not above 0.  SAG_ERR_UNSUPPORTED: hidden
 * 160 ... 256, as there. */
int sag_policy_backward_rows_device(sag_ctx* ctx, const sag_policy_grad_desc* desc, const int32_t* d_rows, int32_t n_index,
                                    const float* d_table, float obs_clip);

/* ---- fork on the device (throughput mode) -------------------------------------------------------
 * sag_fork_device: env i of `dst` takes the complete state of env d_src[i] of `src`, a context on the same device - `dst`
 * itself (a fork inside a batch) or another one, of any n_envs (a few real envs feeding many planner envs; a second context
 * of the same size is a snapshot: fork into it to save, fork back to restore).  Enqueued on dst's stream, returns without
 * waiting, no host copy.  Between two contexts dst's stream first waits for what is enqueued on src's (a step, say), and
 * src's stream then waits for the copy, so a following step of src cannot overtake it.
 *   d_src   [dst n_envs] DEVICE int32, complete before the call (as a reset mask).  d_src[i] < 0: env i is left alone.
 * Commit is per env.  Rejected - the env keeps everything - are an index >= src's n_envs and, in one context, a source that
 * this call overwrites: with j = d_src[i] != i, env i is rejected if d_src[j] >= 0 && d_src[j] != j (d_src[i] == i is a
 * harmless copy onto itself), so no read of the call meets one of its writes.
 * A committed env receives the record (every field of sag_get_state, its step, nonce and flags included) except
 * SAG_I_ENV_ID, the source's row of the layout store (sag_reset restarts the source's layout), its episode accumulators
 * (zero if only dst tracks episodes), its cost byte and, when both contexts have tasks, its task descriptor index.  Its next
 * step runs as after sag_set_state.  It keeps its own SAG_I_ENV_ID, in the state and in the layout store: its action noise
 * and in-step draws differ from the source's from the next step on.  With SAG_FORK_SAME_STREAM the env id is copied too:
 * source and copy draw the same numbers (common random numbers for a planner) and sample the same next layout.
 * Pending external contacts (sag_set_ext_contacts) of dst are dropped.  No timing events are recorded.
 * SAG_ERR_ARG, with nothing enqueued: NULL d_src, unknown flag bits, another robot, other capacities (max_*, has_box),
 * another device, or both contexts with tasks whose descriptor tables differ.  SAG_ERR_STATE: a context without a layout,
 * or dst with tasks and src without. */
enum sag_fork_flags { SAG_FORK_SAME_STREAM = 1 };
int sag_fork_device(sag_ctx* dst, sag_ctx* src, const int32_t* d_src, int32_t flags);
/* Envs copied / envs rejected by sag_fork_device into ctx since the last call with clear != 0.  Synchronises the stream. */
int sag_fork_counts(sag_ctx* ctx, int32_t clear, uint64_t* n_copied, uint64_t* n_rejected);
/* ctx's stream waits for everything enqueued so far on producer's (a context on the same device): what ctx enqueues next may
 * read what producer's stream writes - a planner's action buffer read by the env's step.  No host wait.  producer == ctx: SAG_OK,
 * nothing to do.  SAG_ERR_ARG: NULL, another device. */
int sag_wait_for(sag_ctx* ctx, sag_ctx* producer);

/* ---- shooting planner on the device (throughput mode) -------------------------------------------
 * The other half of a planner built on sag_fork_device: a context of n_envs = G * K envs holds K candidates for each of G real
 * envs (groups are consecutive: candidate k of group g is env g * K + k), and one planning iteration is
 *   sag_fork_device(plan ctx, real ctx, d_src = i / K)   every real env broadcast to its K candidates
 *   sag_plan_sample_device                               K action sequences per group from mean / sigma
 *   sag_plan_score_device                                H steps without observations; return and cost per candidate
 *   sag_plan_refit_device                                rank under the cost budget, refit mean / sigma to the elites
 * all enqueued on the context stream: no host wait, no host copy.  Every buffer is fp32 on the context's device, h-major:
 *   plans [H][n_envs][nu]    mean, sigma [H][G][nu]    (8-byte aligned; step t's actions and the mean's first action are contiguous)
 *   score [n_envs][4] = {discounted return, discounted cost, steps alive, goals met}, 16-byte aligned
 * Refused with SAG_ERR_ARG and nothing enqueued: a NULL or misaligned pointer, K < 1, n_envs % K != 0, H < 1, E < 1, E > K, gamma
 * outside (0, 1] or non-finite, a negative or non-finite sigma_min / sigma_init; SAG_ERR_STATE: a context without a layout.
 *
 * sag_plan_sample_device: plans[h][g*K+k][u] = clamp(mean[h][g][u] + sigma[h][g][u] * z, -1, 1), z = 0 for k = 0 (the current
 * mean is always a candidate).  z is a standard normal of the counter-based generator under the context key (sag_set_seed) on
 * stream 4: with e = h * nu + u, the Philox4x32-10 block of the counter
 *   word 0 = env_id0 (sag_set_tasks; 0 without tasks) + g*K + k    word 1 = draw    word 2 = e / 4    word 3 = 0x10000000
 * gives e % 4 = 0, 1 the two normals (cos, sin) of the Box-Muller transform of its words 0, 1 and e % 4 = 2, 3 those of its
 * words 2, 3 (the transform of the action noise: u = ((w >> 8) + 0.5) / 2^24 in fp32).  Word 3 is stream 4 placed above the 26 bits
 * (episode nonce << 2 | stream) of streams 0 - 3.  The caller advances `draw` from call to call. */
int sag_plan_sample_device(sag_ctx* ctx, int32_t K, int32_t H, const float* d_mean, const float* d_sigma, uint32_t draw,
                           float* d_plans);
/* Zeroes d_score, then H times: the step on actions d_plans + t * n_envs * nu (the device's own action noise and in-step draws,
 * the robot's substeps, no observation), then per env still alive ret += w_t * reward, cost += w_t * (cost != 0), steps += 1,
 * goals += goal_met != 0, with w_0 = 1, w_{t+1} = w_t * gamma in fp32 and the product and the sum rounded separately.  An env
 * stops being alive after a step that reports done; that step is counted.  The context's state advances by H steps: fork again
 * before the next scoring.  Pending external contacts are dropped, as by any step. */
int sag_plan_score_device(sag_ctx* ctx, const float* d_plans, int32_t H, float gamma, float* d_score);
/* Per group: the K candidates in a total order - feasible ones (score cost <= d_budget[g]; every one when d_budget is NULL)
 * first, by higher return; then the infeasible ones by lower cost, then higher return; ties by lower k; a candidate whose return
 * or cost is not finite after every finite one, by k.  The first E are the elites: mean[h][g][u] = (the sum of their plan
 * values in ascending k, in fp32) * (1 / E), sigma = max(sigma_min, sqrt(mean squared deviation from that mean)).
 * d_best[g] = the k of the first candidate, d_best_score[g] (or NULL) its score row.  d_budget: [G] floats or NULL. */
int sag_plan_refit_device(sag_ctx* ctx, int32_t K, int32_t H, int32_t E, const float* d_plans, const float* d_score,
                          const float* d_budget, float sigma_min, float* d_mean, float* d_sigma, int32_t* d_best,
                          float* d_best_score);
/* Receding-horizon warm start after the first action was taken: mean[h] = mean[h + 1], the last row 0, every sigma = sigma_init. */
int sag_plan_shift_device(sag_ctx* ctx, int32_t G, int32_t H, float* d_mean, float* d_sigma, float sigma_init);
/* mean = 0 and sigma = sigma_init for the groups with a non-zero byte of d_mask ([G] device bytes; NULL: every group): the
 * episodes of these envs restarted. */
int sag_plan_clear_device(sag_ctx* ctx, int32_t G, int32_t H, const uint8_t* d_mask, float* d_mean, float* d_sigma,
                          float sigma_init);

#ifdef __cplusplus
}
#endif
#endif /* SAG_H_ */
