/* include/memgym.h -- C ABI of libmemgym_hip.so (MI355X / gfx950 batched Memory Gym hot path).
 *
 * The reference (MarcoMeter/endless-memory-gym) has no FFI: the boundary trainers program against is
 * the Gymnasium Env protocol of its Python classes.  Each entry point below replaces the per-instance
 * Python method named next to it, batched over `num_envs` independent environment instances whose
 * state lives in HBM.  All `*_dev` pointers are device pointers owned by the caller (e.g. torch
 * tensors); `stream` is a hipStream_t (void* so that this header needs no HIP include); every call
 * only enqueues work on that stream (no host synchronisation) unless stated otherwise.
 *
 * Return value: 0 on success, negative on error (`mg_last_error()` holds the message).
 * A handle binds one device; it is not thread-safe, distinct handles are independent.
 *
 * Observation layout (identical to pygame.surfarray.array3d in the reference, e.g.
 * memory_gym/mortar_mayhem_grid.py:276,373): uint8 [num_envs][84 (x)][84 (y)][3 (rgb)].
 */
#ifndef MEMGYM_H
#define MEMGYM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_env mg_env;

#define MG_OBS_DIM 84
#define MG_OBS_BYTES (84 * 84 * 3) /* 21,168 */
#define MG_INFO_SLOTS 8

/* Per-env end-of-episode record, written by mg_step when an env reports done (the reference's
 * `info` dict returned on the terminal step, e.g. mortar_mayhem_grid.py:356-362).  Device SoA,
 * all arrays [num_envs]; any pointer may be NULL.  `aux[k]` meaning per env id: see mg_info_name(). */
typedef struct mg_info_buffers {
    /* Versioning: set to sizeof(mg_info_buffers) of the header the caller was built against.  The library reads that many
     * bytes (never more than it knows) and treats the fields a shorter, older struct lacks as NULL; 0, a size that is not a
     * multiple of the pointer size, or one larger than this build's struct plus 16 pointers (e.g. the device pointer a
     * caller built against the round-2 header -- which had no such member -- passes in this place) is refused (-1). */
    size_t struct_size;
    double* ep_reward_dev;         /* "reward": Python sum() of the step rewards, in double        */
    int32_t* ep_length_dev;        /* "length"                                                      */
    float* aux_dev[MG_INFO_SLOTS]; /* "success", "commands_completed", "num_fails", ... per env id */
    /* Optional (gymnasium 0.29 VectorEnv convention, info["final_observation"]): with autoreset != 0 and this pointer
     * set, mg_step also writes the TERMINAL observation of every instance that finished in this call to row i of this
     * buffer (same format and shape as obs_dev; rows of other instances are left untouched) while obs_dev row i holds
     * the first observation of the new episode.  One option set: the step's own launches draw both frames, for every env id in every
     * observation format (round 6 for MG_OBS_U8_XYC: 0-4 % of a step for eight env ids, 11-12 % for SearingSpotlights-v0 and
     * Endless-MysteryPath-v0) -- the mortar family's ONE launch per step, the finite Mystery Path ids' step + raster / path-service launches, the
     * spotlight family's fused raster / reset launch, and Endless-MysteryPath-v0's step + raster / service launches with one sparse raster
     * launch behind them that draws the terminal frames from the descriptors they leave.  Otherwise (per-instance option sets; agent sprites
     * too big for registers, the agent_scale option, on the Mystery Path family; under graph capture the mortar family and the spotlight
     * family's image-order formats): a step without auto-reset, the terminal rows copied, a masked reset whose frames a sparse raster
     * launch draws; mg_debug_counter "final_obs_generic_steps" counts those calls. */
    void* final_obs_dev;
    /* Optional: the step reward of every instance as the reference computes it -- a Python float, i.e. a double
     * (e.g. mortar_mayhem_grid.py:288-352) -- next to reward_dev's float32 rounding of it; [num_envs]. */
    double* reward64_dev;
    /* Optional (round 5): info["ground_truth"] as the reference returns it -- a float64 array (endless_mortar_mayhem.py:259,358,362,
     * endless_searing_spotlights.py:407,496, endless_mystery_path.py:92-97) -- [num_envs][mg_gt_dim]; gt_dev is its float32
     * rounding (0.6 -> 0.60000002).  Costs one small launch behind the step's; see also mg_ground_truth64. */
    double* gt64_dev;
    /* Optional (round 6): uint8 [num_envs], written by every mg_step: 1 where the instance's episode was ENDED IN THIS STEP BECAUSE IT
     * REACHED A CAPACITY OF THIS BUILD (done_dev is 1 for it as well), else 0.  The reference's lists grow without limit -- path
     * segments (pygame_assets.py:559, called from endless_mystery_path.py:333-335), fall-off cells (:385-393), the command list
     * (endless_mortar_mayhem.py:311-333), live spotlights (endless_searing_spotlights.py:191) -- here they hold 128 segments, 128
     * cells, 512 commands (mg_set_capacity raises the first and the third) and 16 spotlights per instance.  An instance that would need one more ends its episode like a truncation
     * (a reset follows under autoreset); the sticky error bit (mg_poll_errors: 4, 8, 32, 1) is raised as before, so a caller that
     * ignores this array still hears about it.  With it a trainer treats the instance as truncated and goes on with the batch. */
    uint8_t* capacity_dev;
    /* Optional: TERMINAL FRAME RECORDS -- the frame an episode ended on, kept as a frame record (FRAME RECORDS, below) instead of a frame:
     * [num_envs] records of mg_frame_record_bytes each, 16-byte aligned.  DEFINITION: where mg_step / mg_step_masked returns done_dev[i] == 1, row i
     * holds the frame descriptor of instance i as it was BEFORE ANY RESET OF THIS CALL: mg_draw_frames(env, final_frames_dev, num_envs, &i, 1, F, row,
     * stream) writes exactly the bytes row i of final_obs_dev gets from a drawn mg_step of a twin handle in format F with the same history.  Where
     * done_dev[i] == 0 -- instances outside active_dev included -- row i is NOT written.  autoreset 0 and 1; with 0 the row equals what mg_save_frames
     * stores after the call.  Everything else the call leaves -- state, PCG64 streams, the descriptors mg_render / mg_save_frames read, reward, done,
     * episode records, ground truth, error bits -- is bit for bit what the same call without this member leaves.  The rows have the validity of frame
     * records: keep mg_frame_layout next to them.
     * This is what lets a trainer in the gymnasium vector convention step HEADLESS: obs_dev == NULL with final_frames_dev is legal (with final_obs_dev
     * it stays refused: terminal observations are frames), masked or not, one option set or several, every observation format, in the SAME NUMBER OF
     * LAUNCHES as the headless step without the member -- the RECORDS form of the family's (masked) step kernel stores the row itself: the instance's
     * lane (one 16-byte store: Mortar Mayhem ids; four: Mystery Path ids; Endless-MysteryPath-v0 also from its queue server's lane) or its 16-lane
     * group (Searing Spotlights ids: the head from the first lane, a hole word from each).  With obs_dev != NULL the call is that headless arrangement
     * followed by the family's dense raster launch (the one mg_render uses; filtered by active_dev in mg_step_masked): the PLAIN arrangement, not the
     * fused one -- a drawn step that wants its terminal frames cheaply AND its frames fused passes final_obs_dev instead.  Nothing is allocated, no
     * state is added (MG_STATE_VERSION is unchanged), the call can be captured into a HIP graph.  mg_debug_counter "final_frame_steps" counts the
     * calls.  Refused (-1): final_frames_dev together with final_obs_dev (the caller picks one); a final_frames_dev that is not 16-byte aligned.
     * mg_advance, mg_play and their traced siblings do not take it. */
    void* final_frames_dev;
} mg_info_buffers;

/* gymnasium.make(id) + Env.__init__  (memory_gym/__init__.py:13-61; e.g. mortar_mayhem_grid.py:55-90).
 * env_id: one of the reference's registered ids.  Allocates the SoA state for num_envs instances on
 * `device` and builds the stamp atlases / background templates.  Synchronous. */
int mg_create(const char* env_id, int32_t num_envs, int device, mg_env** out);
void mg_destroy(mg_env* env);
const char* mg_last_error(void);

/* Static properties (action_space / observation_space / ground_truth_space of the reference classes):
 * mg_action_dim: 1 = Discrete(4) (mortar_mayhem_grid.py:82, endless_mystery_path.py:83),
 *                2 = MultiDiscrete([3,3]) (e.g. mortar_mayhem.py:83).
 * mg_gt_dim:     0, or the size of info["ground_truth"] (endless_mortar_mayhem.py:91-96 -> 2,
 *                endless_mystery_path.py:92-97 -> 3, endless_searing_spotlights.py:112-117 -> 4). */
int32_t mg_num_envs(const mg_env* env);
int32_t mg_action_dim(const mg_env* env);
int32_t mg_gt_dim(const mg_env* env);
/* MortarMayhemB-Grid-v0 / MortarMayhemB-v0 return a Dict observation (mortar_mayhem_b_grid.py:83-96):
 * "visual_observation" is the usual frame, "vector_observation" the one-hot command list float32[20 * 9]
 * (_encode_commands_one_hot :100-129).  mg_vec_dim: 180 for those ids, else 0.  mg_bind_vector_obs registers the
 * caller's device buffer float32 [num_envs][mg_vec_dim]; the library writes row i whenever instance i is reset
 * (mg_reset and same-step auto-reset) -- the vector is constant within an episode.  NULL unbinds. */
int32_t mg_vec_dim(const mg_env* env);
int mg_bind_vector_obs(mg_env* env, float* vec_dev);
/* name of aux slot k of mg_info_buffers for this env id, or NULL */
const char* mg_info_name(const mg_env* env, int k);

/* One key of the reference's reset `options` dict (process_reset_params, e.g.
 * mortar_mayhem_grid.py:36-53).  `values`/`n`: scalars are n == 1, "sample one per episode" lists
 * have n >= 1.  Unknown key -> error -2 (the Python layer turns it into the reference's
 * AssertionError text); unsupported value -> error -3.  Takes effect at the next reset (also
 * auto-resets), for every instance of the handle that runs under option set 0 (all of them unless
 * mg_bind_option_sets says otherwise, below). */
int mg_set_option(mg_env* env, const char* key, const double* values, int n);

/* Per-instance reset options.  In the reference reset(seed, options) belongs to ONE environment instance (e.g.
 * mortar_mayhem_grid.py:213-236): a pool of workers runs different curricula side by side.  Here a handle holds up to
 * MG_MAX_OPTION_SETS option sets; set 0 is the one mg_set_option writes.  mg_set_option_set writes one key of set
 * `set_id` (a set that has never been written starts from the reference's defaults); mg_bind_option_sets registers the
 * caller's device array int32 [num_envs]: instance i runs under set set_of_dev[i] -- for its resets, auto-resets AND its steps
 * (rewards, limits and display options are read at step time, like the reference's self.reset_params) -- read by every
 * following mg_reset / mg_step; the caller changes an instance's entry when that instance is reset with other options
 * (stream-ordered, e.g. a tensor assignment on the launch stream).  NULL unbinds (every instance under set 0).
 * Options that change the geometry shared by the handle's instances (the *_scale, agent_speed, arena_size, radius and dim /
 * interval options that rebuild atlases, templates or tables) can only be set in set 0, i.e. for all instances: -3 otherwise.
 * A geometry option is accepted in a set > 0 when it says what the handle's geometry already is.
 * Every family (all ten ids).  With more than one set in use the per-set kernels read their parameters from memory and a handle
 * steps in its plain arrangement: a mortar-family handle with two launches, a SearingSpotlights handle resets inside its step
 * kernel, an Endless-MysteryPath handle serves its queue in a launch of its own (and generates every segment when it is due). */
#define MG_MAX_OPTION_SETS 8
int mg_set_option_set(mg_env* env, int set_id, const char* key, const double* values, int n);
int mg_bind_option_sets(mg_env* env, const int32_t* set_of_dev);

/* Capacities of the per-instance lists that the reference grows without limit.  mg_set_capacity(env, what, value), before the handle's
 * first mg_reset (it re-allocates the list's array; mg_state_size changes with it and a checkpoint only loads into a handle of the same
 * capacity); mg_capacity returns the value in force, -1 for a name the env id does not have.
 *   "path_segments"  Endless-MysteryPath-v0: segments of an episode's path (EndlessMysteryPath.add_path_segment, pygame_assets.py:559,
 *                    called from endless_mystery_path.py:333-335 whenever the agent enters the last but one); default 128 = 1,024 tiles,
 *                    4 .. 32,767, 52 bytes per segment and instance.  (Not a ring: an agent that falls off is put back to the START of
 *                    its path, endless_mystery_path.py:316-322, and walks every segment again.)  The agent's x is kept in 32 bits and the
 *                    fall-off cells by column and row, exactly over the whole range (8 x 32,767 columns of 12 px; state version 8 --
 *                    versions <= 7 kept x in 16 bits, which wrapped after 32,767 px, about segment 341).
 *   "commands"       Endless-MortarMayhem-v0: entries of the command list (endless_mortar_mayhem.py:311-333); default 512, 4 .. 32,768,
 *                    one byte per entry and instance.
 *   "fall_off_cells" Endless-MysteryPath-v0 (read only): 128 distinct cells an episode may fall off at (:385-393).
 * An instance that would need one more entry than the capacity ends its episode in that step: done_dev, mg_info_buffers.capacity_dev and
 * the sticky error bit (mg_poll_errors) say so.  16 live spotlights per instance (the spotlight family) is fixed. */
int mg_set_capacity(mg_env* env, const char* what, int64_t value);
int64_t mg_capacity(mg_env* env, const char* what);

/* Observation format written to obs_dev by mg_reset / mg_step (default MG_OBS_U8_XYC).
 *   MG_OBS_U8_XYC   uint8   [num_envs][84 x][84 y][3]  -- the reference's observation: pygame.surfarray.array3d order
 *                                                         (e.g. mortar_mayhem_grid.py:277,372), 21,168 B per instance
 *   MG_OBS_F32_CYX  float32 [num_envs][3][84 y][84 x]  -- value / 255 in image (CHW) order, the tensor a trainer builds
 *                                                         from the observation before its CNN; 84,672 B per instance
 *   MG_OBS_F16_CYX  float16 [num_envs][3][84 y][84 x]  -- the float32 quotient rounded to nearest-even half
 *   MG_OBS_BF16_CYX bfloat16 [num_envs][3][84 y][84 x] -- the float32 quotient rounded to nearest-even bfloat16
 *   MG_OBS_U8_CYX   uint8   [num_envs][3][84 y][84 x]  -- the reference's bytes in image (CHW) order:
 *                                                         out[i][c][y][x] == xyc[i][x][y][c]; 21,168 B per instance, the uint8
 *                                                         rollout buffer a CNN trainer keeps (/ 255 goes into its first layer)
 * The conversion is fused into the raster kernel's stream-out (no second pass over HBM).  mg_obs_bytes returns the
 * bytes per instance of the current format.
 * Which arrangements a format takes: the mortar family's one-launch step and the finite Mystery Path ids' step + raster / path-service
 * launches (and the forms of both that keep terminal observations) run for all five formats, and so does the spotlight family's
 * fused raster / reset launch (deferred resets served inside the raster launch, terminal frames drawn there; which sizes take it
 * without kept terminal observations is a measured choice per format, csrc/mg_spot.hip fuse_resets()).  Endless-MysteryPath-v0's fused
 * raster / service launch (served queues, lazy initial segments, records ahead of time, the fast masked reset) runs for all five formats
 * as well: no format is excluded, a measured choice (csrc/mg_mystery.hip steps_fused(), profiles/emp_chw.md).  No id steps unfused because of its
 * format; what keeps the plain launches is per-instance option sets and, on the Mystery Path family, agent sprites too big for registers. */
#define MG_OBS_U8_XYC 0
#define MG_OBS_F32_CYX 1
#define MG_OBS_F16_CYX 2
#define MG_OBS_BF16_CYX 3
#define MG_OBS_U8_CYX 4
int mg_set_obs_format(mg_env* env, int format);
size_t mg_obs_bytes(const mg_env* env);

/* Env.reset(seed, options) (e.g. mortar_mayhem_grid.py:213-278) for all instances, or for those with
 * mask_dev[i] != 0.  seeds_dev: int64 [num_envs] -> instance i is re-seeded exactly like
 * gymnasium's reset(seed=s): Generator(PCG64(SeedSequence(s))); NULL -> keep each instance's stream
 * (reset(seed=None)).  Writes the first observation of every reset instance to obs_dev (others are
 * left untouched) and, if gt_dev != NULL and mg_gt_dim() > 0, info["ground_truth"] as float32
 * [num_envs][gt_dim]. */
int mg_reset(mg_env* env, const int64_t* seeds_dev, const uint8_t* mask_dev, void* obs_dev, float* gt_dev,
             void* stream);

/* Rasterise the CURRENT frame of every instance again into obs_dev (the frame the last mg_reset / mg_step produced; the
 * reference's _draw_surfaces + surfarray.array3d without stepping, e.g. mortar_mayhem_grid.py:92-102,373).  No state
 * changes; instances that the last call left untouched (a masked mg_reset) are skipped here as well.  Uses: observations into a second buffer, a changed observation format, and the placement probe of the
 * Python mirror (the store stream is 8-13 % faster into some allocations than into others: profiles/r01l_placement.md). */
int mg_render(mg_env* env, void* obs_dev, void* stream);

/* Env.render() with render_mode "debug_rgb_array" (e.g. mortar_mayhem_grid.py:403-405 -> _build_debug_surface :104-135)
 * for every instance: the ground-truth view (target tile ring / whole path and walls / everything the spotlight layer
 * hides drawn over it), stretched to 336 x 336 like pygame.transform.scale, in IMAGE order:
 * rgb_dev uint8 [num_envs][336 y][336 x][3].  Changes nothing the observations, rewards or RNG streams depend on; the
 * only state it touches is the mortar family's counter of entries popped from the reference's CLONE of the command
 * visualisation list (mortar_mayhem_grid.py:122: every debug render pops one), so that zero, one or several renders
 * between steps show what the reference shows.  After headless steps (obs_dev == NULL) or mg_advance it shows the state the last
 * of those steps left -- the view a drawn run of the same steps gives, episodes that ended inside included -- and right after
 * mg_set_state the view of the handle the blob was taken from (tests/test_gpu_debug_arrangements.py).  Synchronous (allocates and
 * frees a scratch buffer); not a hot path.  The view of a few instances, kept and drawn later without either: mg_save_debug_frames below. */
int mg_render_debug(mg_env* env, uint8_t* rgb_dev, void* stream);

/* Env.step(action) (e.g. mortar_mayhem_grid.py:280-375) for all instances.
 * actions_dev: int32 [num_envs] (Discrete) or [num_envs][2] (MultiDiscrete).
 * reward_dev: float32 [num_envs] (the reference's Python float, rounded once to float32);
 * done_dev: uint8 [num_envs] (`truncation` is always False in the reference).
 * autoreset != 0: an instance that reports done is reset in the same call with seed=None (its RNG
 * stream continues, exactly what `env.reset()` right after a terminal step does) and obs_dev/gt_dev
 * hold the first observation of the new episode; the finished episode's info is in `info`.
 *
 * HEADLESS STEP: obs_dev == NULL steps without drawing -- every env id, every observation format, one or several option sets,
 * autoreset 0 and 1, with or without any of the optional buffers.  State, every instance's PCG64 stream, reward, done, ground truth,
 * the episode records, the error bits and the frame descriptors the step leaves are bit for bit those of a drawn step of the same
 * handle; the frames are simply not written (the raster is 85-95 % of a drawn step).  mg_render after any number of headless steps
 * writes for every instance exactly the frame the last step would have drawn -- for an instance that step auto-reset, the first frame of
 * the new episode.  Headless and drawn steps alternate freely in one handle.  A headless step takes the family's plain arrangement
 * without its raster launch: the mortar family's step kernel alone; the spotlight family's and the finite Mystery Path ids' step
 * kernel with the resets / paths generated in it; Endless-MysteryPath-v0's step kernel and its queue server as a launch of its own
 * (whatever earlier fused steps left owed is generated first, and the next drawn step is fused again) -- a linear chain of launches,
 * capturable into a HIP graph.  Refused (-1): obs_dev == NULL together with info->final_obs_dev -- terminal observations are frames.
 * (The frame an episode ended on leaves a headless step as a RECORD: info->final_frames_dev, see mg_info_buffers.)
 * mg_reset and mg_single_step keep requiring their buffers.  mg_debug_counter "headless_steps" counts these calls. */
int mg_step(mg_env* env, const int32_t* actions_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev,
            float* gt_dev, const mg_info_buffers* info, int autoreset, void* stream);

/* Env.step(action) (e.g. mortar_mayhem_grid.py:280-375) of the SELECTED instances: those with active_dev[i] != 0 step, the others are left alone.
 * active_dev: uint8 [num_envs], read on `stream` by the step's launches; the host never looks at it (no synchronisation, no allocation).
 * active_dev == NULL is mg_step with the remaining arguments -- same launches, same fused arrangements -- and counts as an ordinary step.
 * DEFINITION: take the subsequence of calls in which instance i was active; its results are exactly what a handle stepped with plain mg_step
 * gives instance i for the same actions in the same order.
 *   active_dev[i] != 0  everything mg_step would do to the instance, bit for bit: state, PCG64 stream, frame descriptor, reward_dev[i], done_dev[i],
 *                       its gt_dev row, every mg_info_buffers row, obs_dev row i, final_obs_dev row i, same-call auto-reset, capacity ends, error bits.
 *   active_dev[i] == 0  nothing of the instance changes: state, stream and descriptor stay; row i of obs_dev, gt_dev, final_obs_dev, ep_reward_dev,
 *                       ep_length_dev, aux_dev[k], gt64_dev and the bound vector observation is NOT written.  Written are reward_dev[i] = 0 and done_dev[i] = 0, and where given reward64_dev[i] = 0 and capacity_dev[i] = 0, so
 *                       that the step's outputs serve as masks and sums without another look at active_dev.  Its action entry is not interpreted.
 * A mask of all zeros is legal.  Uses: one episode per seed (active = not yet finished, autoreset 0 or 1 -- the evaluation protocol of the Memory Gym
 * paper without stepping an instance past its end), instances stepped at different rates (action repeat, asynchronous samplers), pausing part of a batch.
 * Launches: the arrangement of a HEADLESS step with the MASKED form of its step kernel (mortar_step_masked_kernel; spot_step_masked_kernel, never deferred;
 * mystery_step_masked_kernel with the paths generated in it; Endless-MysteryPath-v0: whatever earlier fused steps left owed is generated first -- for every
 * instance, which changes no result -- then emp_step_masked_kernel and the queue server, which serves the active instances' entries alone; the next
 * unmasked drawn step is fused again), then, with obs_dev, ONE raster launch restricted to the active instances.  A linear chain, capturable into a HIP
 * graph: the mask is read from memory at replay.  obs_dev == NULL is a masked headless step (refused together with final_obs_dev, like mg_step).
 * With final_obs_dev and autoreset the generic path of mg_step is taken -- masked step without auto-reset, the finished rows copied, masked reset by
 * done_dev.  mg_render afterwards behaves as after mg_step: inactive instances keep the descriptor they had.  Per-instance option sets, every observation
 * format, mg_set_capacity, checkpoints between masked steps (MG_STATE_VERSION is unchanged: no state is added), mg_expert_actions / mg_advance before and
 * after work as documented.  An all-ones mask costs the plain arrangement, not the fused one (profiles/masked_step.md).
 * mg_debug_counter "masked_steps" counts the calls with active_dev != NULL (a masked headless step is counted there and in "headless_steps").
 * Errors (-1): a NULL actions_dev, reward_dev or done_dev; before the first mg_reset / mg_set_state; a geometry option set since the last reset. */
int mg_step_masked(mg_env* env, const int32_t* actions_dev, const uint8_t* active_dev, void* obs_dev, float* reward_dev,
                   uint8_t* done_dev, float* gt_dev, const mg_info_buffers* info, int autoreset, void* stream);

/* NEXT-STEP AUTO-RESET (gymnasium >= 1.0, AutoresetMode.NEXT_STEP): Env.step(action) (e.g. mortar_mayhem_grid.py:280-375) for the instances with
 * restart_dev[i] == 0, Env.reset() (seed=None, :213-278) for those with restart_dev[i] != 0 -- the caller feeds the previous call's done_dev back in, so
 * that the step that ends an episode returns the TERMINAL observation as its ordinary observation and the following call returns the first observation
 * of the new episode, with reward 0 and done 0.  restart_dev: uint8 [num_envs], read on `stream` by the call's launches; the host never looks at it.
 * DEFINITION: the pair  mg_step_masked(env, actions_dev, active = !restart, obs_dev, reward_dev, done_dev, gt_dev, info, autoreset = 0, stream);
 *                       mg_reset(env, NULL, restart, obs_dev, gt_dev, stream);   [+ mg_ground_truth64 into info->gt64_dev where that is set]
 *   restart_dev[i] != 0  the instance is reset instead of stepped: its PCG64 stream continues (seeds_dev == NULL), it keeps the option set it has, its action
 *                        entry is not interpreted; reward_dev[i] = 0, done_dev[i] = 0, and where given reward64_dev[i] = 0 and capacity_dev[i] = 0; its rows of
 *                        ep_reward_dev, ep_length_dev and aux_dev[k] keep their previous contents; its rows of obs_dev, gt_dev, gt64_dev and the bound vector
 *                        observation are the reset's.
 *   restart_dev[i] == 0  everything mg_step(..., autoreset = 0) would do to the instance, bit for bit; row i of obs_dev is the frame after the step, which is
 *                        the terminal frame where done_dev[i] is set, and the instance stays in its terminal state until a later call restarts it.
 * Every row of obs_dev is written.  The handle's memory afterwards is the pair's, bit for bit -- also the frame descriptor rows: those of the instances
 * that were not restarted are marked "leave the frame untouched" as after any masked mg_reset (mg_render / mg_save_frames right behind the call skip
 * them; obs_dev holds their frames, and their next step rewrites the rows).
 * ALIASING: restart_dev == done_dev is legal and the intended use.  Each instance's flag is read before its done is written.
 * Launches: the mortar and the spotlight family run the NEXT form of their two-launch step -- mortar_step_next_kernel / spot_step_next_kernel, in which a
 * flagged instance is reset by its own lane(s), the family's dense raster launch, and one small launch that settles the descriptor rows; their
 * one-launch / fused serve arrangements are not used.  The Mystery Path ids run the pair itself behind one small launch that writes the mask and a copy
 * of the flags into the handle's scratch.  A linear chain on `stream`, nothing synchronises; the handle's first call allocates that scratch (2 x
 * num_envs bytes) and therefore refuses a stream that is being captured, later calls can be captured into a HIP graph: restart_dev and actions_dev are
 * read at replay.  Per-instance option sets and every observation format work as documented; MG_STATE_VERSION is unchanged: no state is added.
 * mg_debug_counter "next_steps" counts the calls, "next_fused_steps" those that took a family's own kernel.
 * Refused (-1) before anything is stepped: before the first mg_reset / mg_set_state; a NULL actions_dev, restart_dev, obs_dev, reward_dev or done_dev
 * (there is no headless next-step call: mg_reset has no headless form); info->final_obs_dev or info->final_frames_dev set (there are no terminal rows
 * in this mode: the terminal frame is the observation); a geometry option set since the last reset.  An active mask together with restart flags does
 * not exist. */
int mg_step_next(mg_env* env, const int32_t* actions_dev, const uint8_t* restart_dev, void* obs_dev, float* reward_dev,
                 uint8_t* done_dev, float* gt_dev, const mg_info_buffers* info, void* stream);

/* The float64 ground truth of every instance from the CURRENT state (what the last mg_reset / mg_step left), [num_envs][mg_gt_dim]
 * on the device: the doubles the reference puts into info["ground_truth"] after reset() as well as after step().  Enqueued on
 * `stream`; a no-op for env ids without ground truth. */
int mg_ground_truth64(mg_env* env, double* gt64_dev, void* stream);

/* The scripted teacher: for every instance the action the CPU oracle's expert hook gives in the instance's CURRENT state -- what the last
 * mg_reset / mg_step left, i.e. the new episode's state where that step auto-reset the instance -- written to actions_dev in the layout
 * mg_step reads (int32 [num_envs] for Discrete ids, [num_envs][2] for MultiDiscrete ids).  The reference itself has no such method; the
 * DEFINITION is the oracle's hooks, restated on the records the step kernels keep:
 *   oracle/mgo_mortar.c  mm_expert (:546)                  the five Mortar Mayhem ids: wait while commands are shown and while the tiles
 *                                                          are on, else move to the target tile (Endless: the shorter way round the wrap)
 *   oracle/mgo_mystery.c mpf_expert / emp_expert (:713-745) follow the path: the node behind the agent's in the reference's path list
 *   oracle/mgo_spot.c    sp_expert (:770)                  the first remaining coin, then the exit
 * With probability eps instance i gets, instead, the uniformly random action of oracle/mgo_api.c mgo_batch_expert (:262-289): a
 * counter-based hash of (seed, step, i), the same numbers for any eps in [0, 1] -- so a caller that passes its step counter gets the
 * oracle's policy for "competent play" bit for bit (tests/test_gpu_expert.py, all ten ids).  Per-instance option sets are honoured.
 * ONE small launch, enqueued on `stream`: no synchronisation, no allocation, no state change, and nothing is drawn from any instance's PCG64
 * stream -- calling it, or not, changes no later observation, reward or random number.  It can be captured into a HIP graph; eps, seed and
 * step are kernel arguments, so a captured launch replays the values it was captured with (a trainer that wants fresh random actions per
 * replay updates the node's arguments or leaves the call outside the graph). */
int mg_expert_actions(mg_env* env, double eps, uint64_t seed, uint64_t step, int32_t* actions_dev, void* stream);

/* `steps` steps under the scripted teacher WITHOUT A FRAME: the warm-up behind reset(seed) that takes the instances' episodes out of
 * phase, the return of the teacher per curriculum setting, the check that an option set is solvable.  DEFINITION: state, streams, frame
 * descriptors and error bits afterwards equal bit for bit those after
 *     for t in 0 .. steps-1:
 *         mg_expert_actions(env, eps, seed, step0 + t, A, stream)
 *         mg_step(env, A, NULL, R, D, gt_dev, info, 1, stream)            (headless, auto-reset)
 * and the sums in `out` are the ones that loop produces; eps = 1 is therefore the uniformly random policy and eps = 0 the teacher.
 * gt_dev may be NULL, otherwise it holds the ground truth after the last step.  `out` may be NULL.  mg_render draws the frames the last
 * step left.  Nothing synchronises.  The scratch the loop needs (actions, reward, done, one row of episode records: about 50 bytes per
 * instance) is allocated AT THE HANDLE'S FIRST mg_advance; every later call allocates nothing and can be captured into a HIP graph --
 * steps, eps, seed and step0 are then the captured values, as with mg_expert_actions.
 * The five Mortar Mayhem ids run the loop INSIDE one launch (mortar_advance_kernel: a lane per instance plays teacher, step and sums by
 * itself; at most 1,024 steps per launch, a longer call is split); mg_debug_counter "advance_fused_steps" counts the steps taken this
 * way, which are no "headless_steps".  The other five ids take the loop above on the host -- expert launch, headless step, one small
 * accumulate launch per step; their resets are cooperative (A* paths, 16 lanes per spotlight instance), so there is no in-launch form
 * for them yet -- and count as "headless_steps".  Terminal observations do not exist here: episodes that end inside the call are
 * counted and summed, not shown.
 * Errors (-1): before the first mg_reset / mg_set_state; steps < 1; eps outside [0, 1]; a geometry option set since the last reset. */
typedef struct mg_advance_out {      /* all device arrays [num_envs], any may be NULL; OVERWRITTEN with this call's sums */
    size_t   struct_size;             /* in: sizeof(mg_advance_out) of the caller's header                                                 */
    double*  reward_sum_dev;          /* step rewards as the reference's doubles, added in step order                      */
    int32_t* episodes_dev;            /* episodes that ended in these steps (capacity ends included)                       */
    double*  ep_reward_sum_dev;       /* sum of info["reward"] over those episodes, in order of ending                     */
    int64_t* ep_length_sum_dev;       /* sum of info["length"]                                                             */
    double*  aux_sum_dev[MG_INFO_SLOTS]; /* sum of aux slot k (mg_info_name), e.g. "success"; slots without a name are not written */
} mg_advance_out;
int mg_advance(mg_env* env, int32_t steps, double eps, uint64_t seed, uint64_t step0,
               float* gt_dev, const mg_advance_out* out, void* stream);

/* `steps` steps of a CALLER-SUPPLIED action tape WITHOUT A FRAME: what mg_advance is for the library's teacher, for the caller's own action sequences --
 * planning by random shooting from a saved state (mg_save_instances / mg_load_instances), replaying recorded demonstrations, counterfactual probes,
 * evaluating stored tapes of one episode per seed.
 *   tape_dev          int32 [steps][num_envs] (Discrete ids) or [steps][num_envs][2] (MultiDiscrete ids): step-major, row t is what mg_step takes as actions_dev
 *   mode              MG_PLAY_THROUGH: auto-reset, an instance that ends an episode goes on into the next one, like mg_advance
 *                     MG_PLAY_EPISODE: every instance plays until ITS episode ends, is then left alone and is NOT reset
 *   active_dev        uint8 [num_envs] or NULL (= everybody): the instances that play at all; read by the launches, never by the host
 *   reward_trace_dev  float32 [steps][num_envs] or NULL      done_trace_dev  uint8 [steps][num_envs] or NULL
 *   steps_played_dev  int32 [num_envs] or NULL: the steps each instance took in this call
 *   sums              mg_advance_out, with the struct-size rules of mg_advance; OVERWRITTEN with this call's sums; or NULL
 *   gt_dev            as in mg_step_masked: rows of the instances that stepped hold the ground truth after their last step; or NULL
 * DEFINITION: state, PCG64 streams, frame descriptors, ground truth, error bits, traces and sums afterwards equal bit for bit those after
 *     alive[i] = active_dev ? active_dev[i] != 0 : 1;  played[i] = 0
 *     for t in 0 .. steps-1:
 *         mg_step_masked(env, tape_dev + t * row, M, NULL, R_t, D_t, gt_dev, info, mode == MG_PLAY_THROUGH, stream)
 *                 M = alive; M = NULL (the plain headless mg_step) when active_dev == NULL and mode == MG_PLAY_THROUGH
 *         sums += step t's rows: the additions of mg_advance, in the same order
 *         played[i] += alive[i]
 *         if mode == MG_PLAY_EPISODE: alive[i] &= !D_t[i]
 * where R_t / D_t are row t of the traces (scratch where a trace is NULL) and `info` the handle's scratch rows (reward64, the episode record, the named
 * aux slots).  What follows from mg_step_masked's own definition: an instance that is not alive keeps its state, its stream and its descriptor; its
 * trace entries are 0 and its tape entries are not interpreted; an instance that never was alive has sums and steps_played of 0.  In MG_PLAY_EPISODE a
 * finished instance stays in the terminal state mg_step with autoreset == 0 leaves: mg_render shows its terminal frame, and the caller resets it (a
 * masked mg_reset) or loads a record into it before it is stepped again.  mg_render draws, for every instance, the frame its last step left.
 * Nothing synchronises.  The scratch (an alive byte, one reward / done row and the episode-record rows: about 40 bytes per instance) is allocated AT THE
 * HANDLE'S FIRST mg_play, which therefore cannot be captured; every later call allocates nothing and can be captured into a HIP graph -- tape and mask are
 * read from memory at replay, steps and mode are the captured values.  MG_STATE_VERSION is unchanged: no state is added.  Per-instance option sets,
 * mg_set_capacity and every observation format work as they do for the calls of the definition.
 * The five Mortar Mayhem ids run the loop INSIDE one launch (mortar_play_kernel: a lane per instance reads its tape entry, steps, stores its trace
 * entries and keeps sums and step count in registers; a MG_PLAY_EPISODE lane leaves the loop at its own end; at most 1,024 steps per launch, a longer call
 * is split); mg_debug_counter "play_fused_steps" counts the steps of such calls, which are no "headless_steps".  The other five ids take the loop above on
 * the host -- the headless (masked) step and one small accumulate launch per step -- and count as "headless_steps" / "masked_steps".
 * Errors (-1): before the first mg_reset / mg_set_state; steps < 1; tape_dev NULL; a mode other than the two; a bad sums->struct_size; a geometry
 * option set since the last reset. */
#define MG_PLAY_THROUGH 0
#define MG_PLAY_EPISODE 1
int mg_play(mg_env* env, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev,
            float* reward_trace_dev, uint8_t* done_trace_dev, int32_t* steps_played_dev,
            float* gt_dev, const mg_advance_out* sums, void* stream);

/* ROLLOUT TRACES: mg_advance / mg_play that KEEP EVERY STEP -- the frame record, the action played, the teacher's label, reward and done -- so that K steps
 * under the teacher (or under the caller's tape) leave a complete rollout behind and mg_draw_frames later draws only the minibatch rows training asks for.
 * All trace arrays are step-major, row t belongs to step t of the call; every array may be NULL (not kept).
 * DEFINITION: state, PCG64 streams, frame descriptors, ground truth, error bits and sums after either call are exactly those of mg_advance / mg_play with the
 * same arguments, and row t of the traces is what the definition loop of that call produces at step t:
 *   mg_advance_traced   actions row t = what mg_expert_actions(env, eps, seed, step0 + t, ...) wrote before the step;
 *                       labels  row t = what mg_expert_actions(env, 0.0, seed, step0 + t, ...) gives in the same state (the teacher's answer: DAgger labels);
 *   both                reward / done row t = the R / D of step t;
 *                       frames row t = what mg_save_frames(env, NULL, num_envs, frames + t * num_envs * mg_frame_record_bytes, stream) stores right after step t:
 *                       the frame the step would have drawn -- the new episode's first frame where the step auto-reset the instance.
 * What follows for MG_PLAY_EPISODE and for instances outside active_dev: an instance that does not step keeps its descriptor, so its frames rows repeat the
 * descriptor it has -- the terminal one after its own done, the one from before the call if it never was alive -- and its reward / done entries are 0.
 * trace == NULL is legal and makes the call its untraced sibling (mg_play_traced then keeps no reward / done rows either).  Frame traces have the validity of
 * frame records: keep mg_frame_layout next to them.  The frame BEFORE the call's first step is not part of the trace: mg_save_frames it first (the Python
 * mirror does, into row 0 of a [steps + 1] store).
 * The scratch is the siblings' (allocated at the handle's first mg_advance / mg_advance_traced, respectively mg_play / mg_play_traced, which cannot be captured);
 * every later call allocates nothing and can be captured into a HIP graph: the trace pointers are then the captured values, their contents are written at
 * replay.  MG_STATE_VERSION is unchanged: no state is added.
 * The five Mortar Mayhem ids run the loop INSIDE one launch per 1,024 steps (mortar_advance_traced_kernel / mortar_play_traced_kernel: the lane stores its action
 * straight into the trace row, evaluates the teacher a second time for the label, and stores the 16-byte descriptor its step has just left as one vector store;
 * all trace offsets are 64-bit); the other five ids take the loop on the host with the trace rows as the loop's own A / R / D rows, one more teacher launch for
 * the labels and one mg_save_frames launch per step.  mg_debug_counter "traced_steps" counts the steps of calls with a trace, "traced_fused_steps" those taken
 * in-launch; they also count as the siblings' "advance_fused_steps" / "play_fused_steps" / "headless_steps" / "masked_steps".
 * STILL OUT OF SCOPE: the terminal frames of episodes that end inside a call (the reset frame replaces them, as in mg_advance); the MortarMayhemB ids' vector
 * observation per step; the debug view of the steps inside a call (between calls: mg_save_debug_frames).
 * Errors (-1): everything the sibling refuses; a mg_rollout_trace.struct_size that is no layout of this header; a frames_dev that is not 16-byte aligned;
 * actions_dev / labels_dev that are not 8-byte aligned; actions_dev or labels_dev set in mg_play_traced (the tape is the caller's, there is no teacher). */
typedef struct mg_rollout_trace {   /* every array may be NULL */
    size_t   struct_size;           /* in: sizeof(mg_rollout_trace) of the caller's header; checked like mg_advance_out's */
    void*    frames_dev;   /* [steps][num_envs] records of mg_frame_record_bytes each; 16-byte aligned */
    int32_t* actions_dev;  /* [steps][num_envs * action_dim]: the action played at step t  (mg_advance_traced only) */
    int32_t* labels_dev;   /* same shape: the teacher's answer at eps = 0 in the state before step t (mg_advance_traced only) */
    float*   reward_dev;   /* [steps][num_envs] */
    uint8_t* done_dev;     /* [steps][num_envs] */
} mg_rollout_trace;
int mg_advance_traced(mg_env* env, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev,
                      const mg_advance_out* out, const mg_rollout_trace* trace, void* stream);
int mg_play_traced(mg_env* env, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev,
                   int32_t* steps_played_dev, float* gt_dev, const mg_advance_out* sums,
                   const mg_rollout_trace* trace, void* stream);

/* The single-instance fast path (BASELINE config C1: gym.make(id), one instance, numpy in / numpy out -- the reference's own loop,
 * /root/reference/bench.py:12-30).  For a handle with num_envs == 1, mg_single_open allocates every per-call buffer in pinned,
 * device-mapped HOST memory and returns the host addresses: the kernels read the action from it and store observation, reward,
 * done, ground truth and the end-of-episode record straight into it (21 KB over PCIe), so that one call = store the action,
 * enqueue the step's launches, wait for the stream -- no copy operation, no allocation, no indexing kernel.
 *   mg_single_reset(env, seed, has_seed, stream)   Env.reset(seed) + wait; options through mg_set_option as ever
 *   mg_single_step(env, a0, a1, stream)            Env.step(action) WITHOUT auto-reset (the caller resets, like the reference's
 *                                                  loop) + wait; results are in the buffers of mg_single_io when it returns.
 *                                                  Returns 0, a negative error code, or -- POSITIVE -- the device error bits as they
 *                                                  stand (mg_peek_errors; sticky until mg_poll_errors).  The wait polls a word in the
 *                                                  pinned block that a stream memory operation writes behind the step's launches
 *                                                  (no hipStreamSynchronize; round 6)
 * `obs` has the handle's observation format; `gt` holds mg_gt_dim doubles; `vec` the MortarMayhemB vector observation or NULL.
 * The buffers live as long as the handle.  Same results as the batched path with one instance (tests/test_gpu_single_instance.py). */
typedef struct mg_single_io {
    size_t struct_size;   /* in: sizeof(mg_single_io) of the caller's header */
    void* obs;
    float* vec;
    double* reward;       /* the step reward as the reference's Python float */
    uint8_t* done;
    double* gt;
    double* ep_reward;    /* valid when *done: info["reward"], info["length"], aux[k] (mg_info_name) */
    int32_t* ep_length;
    float* aux[MG_INFO_SLOTS];
} mg_single_io;
int mg_single_open(mg_env* env, mg_single_io* io);
int mg_single_reset(mg_env* env, int64_t seed, int has_seed, void* stream);
int mg_single_step(mg_env* env, int32_t a0, int32_t a1, void* stream);

/* Checkpoint hooks (the reference cannot serialise an env; SoA state makes it free).  Synchronous.
 * mg_state_size: bytes needed.  The blob starts with a 64-byte header {magic "MGSTATE1", MG_STATE_VERSION, num_envs,
 * payload bytes, FNV-1a of the env id}; the layout behind it is private to one MG_STATE_VERSION.  mg_set_state refuses
 * (-1, message in mg_last_error) a blob whose magic, version, env id, num_envs or payload size differ from the handle's
 * instead of mis-assigning it.  (The finite Mystery Path ids' blobs carry the order of every instance's path since mg_expert_actions exists:
 * 64 bytes per instance more than before, so an earlier blob of those two ids is refused by its payload size; the other eight ids' layout
 * is what it was.  The spotlight family's blobs carry the frame descriptors as well, 128 bytes per instance more -- what mg_render,
 * mg_render_debug and a reset's stale holes read before the restored handle's first step; an earlier blob of those two ids is refused
 * by its payload size in the same way.) */
#define MG_STATE_VERSION 8u
size_t mg_state_size(const mg_env* env);
int mg_get_state(mg_env* env, void* host_buf, size_t size);
int mg_set_state(mg_env* env, const void* host_buf, size_t size);

/* INSTANCE RECORDS: single instances saved to and loaded from caller-owned DEVICE memory -- rewind an instance to a checkpoint of its own episode,
 * branch K action sequences from one state (counterfactual probes: same state, different memory content), search and archive-and-return exploration,
 * hand one hard state to many instances, move states around inside a batch.  (mg_get_state / mg_set_state cover the whole handle, are synchronous
 * and go through host memory.)
 *   mg_save_instances   record j <- instance idx_dev[j]                  (idx_dev == NULL: instance j), j = 0 .. count-1
 *   mg_load_instances   instance idx_dev[j] <- record rec_of_dev[j]      (rec_of_dev == NULL: record j; idx_dev == NULL: instance j)
 * DEFINITION: let record r be saved from instance s at some moment.  After a load of r into instance d, instance d gives from then on, for the same
 * actions in the same order, bit for bit what instance s gave from the moment of the save: state and PCG64 stream, frames, reward, done and ground
 * truth, episode records, same-call auto-resets, capacity ends, error bits, mg_expert_actions, mg_render_debug and the bound vector observation.  Every
 * instance the load does not name keeps everything; a save changes nothing observable on any instance.  A copy inside the handle is a save followed by a
 * load through the buffer, so overlapping source and destination sets are no special case.
 * count is a host integer (it sizes the grid), 0 <= count; count == 0 does nothing.  rec_dev: 16-byte aligned, count * mg_instance_bytes bytes; the
 * layout of a record is private.  idx_dev / rec_of_dev: int32 [count] on the device, read by the launches; the host never looks at them.  An entry
 * idx_dev[j] < 0 is skipped: a fixed-size index array padded with -1 serves any subset without a host look, and a captured graph replays with other
 * contents.  An entry idx_dev[j] >= num_envs, or rec_of_dev[j] outside 0 .. count-1, is skipped as well and raises error bit 512 (mg_poll_errors); it
 * never becomes an out-of-bounds access.  One record may be loaded into many instances.  The instance indices of ONE load must be distinct: with
 * duplicates it is unspecified which entry wins, but the instance ends up holding exactly one whole record (a claim launch in front of the copy decides).
 * WHAT TRAVELS: everything the checkpoint holds per instance, and the frame descriptor row -- so mg_render after a load draws the loaded instance's
 * frame as of the save.  The MortarMayhemB ids' bound vector observation row is carried in the record and written back by the load (bind before the
 * save; a new binding is a new layout).  Endless-MysteryPath-v0: path segments still owed are generated before a save reads, stream-ordered (the launch
 * a headless step uses); a record generated ahead of time belongs to the instance and travels with it.  WHAT DOES NOT: the words of a launch (hand-over,
 * claim and ticket words, queues, counters) and the caller's set_of_dev entry (mg_bind_option_sets) -- THE CALLER OWNS IT AND COPIES IT: an instance
 * loaded from a record runs under the option set its set_of_dev entry names, so copy the saved instance's entry along (the Python mirror does).
 * VALIDITY: a record is valid for the handle it was saved from, under the geometry it was saved under -- not for another handle (exit generations and
 * atlases are handle-local) and not across a rebuild of the geometry (a geometry option followed by a reset; mg_set_capacity; mg_set_state on the
 * spotlight family; a new mg_bind_vector_obs binding).  mg_instance_layout returns a 64-bit value that is unique to the handle within the process and
 * changes at every such rebuild: keep it next to the records and compare before loading.  mg_load_instances CANNOT check this -- the records carry no
 * header -- and loading a stale record is undefined for the named instances.  mg_instance_bytes is fixed once the handle has been reset.
 * obs_dev != NULL: the load draws the frames of the loaded instances, and only those, into their rows (the masked step's raster launch); other rows
 * are untouched.  obs_dev == NULL draws nothing; mg_render later shows the loaded frames.
 * LAUNCHES: both calls only enqueue on `stream`, nothing synchronises.  A save: (Endless-MysteryPath-v0: the owed-segment launch,) one row-copy launch
 * -- a wave per record, each row moved with the widest access its size allows, rows longer than 16 KiB shared by several waves.  A load: a small claim
 * launch, the row-copy launch, and with obs_dev a memset of the row mask and one raster launch.  The scratch a load needs (an int32 claim word and a
 * uint8 row-mask entry per instance) is allocated AT THE HANDLE'S FIRST mg_load_instances; every later call allocates nothing, and both calls can be
 * captured into a HIP graph (the index arrays are read at replay).  MG_STATE_VERSION is unchanged: no state is added.
 * mg_debug_counter "instance_saves" / "instance_loads" count the calls with count > 0, on the host.
 * Errors (-1): before the first mg_reset / mg_set_state; count < 0; a NULL or misaligned rec_dev; a geometry option set since the last reset. */
size_t   mg_instance_bytes(const mg_env* env);   /* bytes of one record; a multiple of 16 */
uint64_t mg_instance_layout(const mg_env* env);
int mg_save_instances(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream);
int mg_load_instances(mg_env* env, const int32_t* idx_dev, const int32_t* rec_of_dev, int32_t count, const void* rec_dev,
                      void* obs_dev, void* stream);

/* FRAME RECORDS: keep a frame as its descriptor and draw it later.  Every frame this library writes is a pure function of the instance's frame
 * descriptor -- the row the step kernels leave behind: 16 B (Mortar Mayhem ids), 64 B (Mystery Path ids), 128 B (Searing Spotlights ids) -- and the
 * handle's atlas; the frame itself is 21,168 to 84,672 B.  A trainer steps headless or drawn, keeps each step's descriptor rows in a store of its own and
 * at training time draws exactly the minibatch rows it wants, in the network's format, straight into its input tensor.
 *   mg_save_frames   record j <- the CURRENT frame descriptor of instance idx_dev[j]   (idx_dev == NULL: instance j), j = 0 .. count-1
 *   mg_draw_frames   row j of obs_dev <- the frame of record pick_dev[j]               (pick_dev == NULL: record j, and then count <= n_records)
 * DEFINITION: let a record be saved from instance i after some call, and let that call have written row i of its observation buffer in format F.  Then
 * mg_draw_frames(..., F, ...) writes that record's row with exactly those bytes; for any other format it writes the bytes a handle in that format would
 * have shown.  After a headless step (obs_dev == NULL) the record draws the frame the step would have drawn.  Nothing of the handle's state, streams or
 * descriptors changes in either call.
 * mg_save_frames: the index conventions of mg_save_instances -- an entry < 0 is skipped, an entry >= num_envs is skipped and raises error bit 512; a
 * skipped entry leaves its record untouched.  rec_dev: 16-byte aligned, count * mg_frame_record_bytes bytes; so a row block of a larger [T][N] store is
 * filled step by step.  One small row-gather launch.  (Endless-MysteryPath-v0: the descriptor rows are complete once the step's launches have run, owed
 * path segments are no part of them: nothing is flushed and nothing synchronises, exactly as for mg_render.)
 * mg_draw_frames: count is independent of num_envs -- one frame, or millions; format is any MG_OBS_*, independent of the handle's own (records carry no
 * format); obs_dev: 16-byte aligned, count rows of that format.  A pick outside 0 .. n_records-1 leaves its row untouched and raises bit 512.  A record
 * whose descriptor says "leave the frame untouched" -- what a masked mg_reset leaves for the instances it did not reset -- leaves its row untouched, as
 * mg_render does.  Duplicates in pick_dev are legal.  ONE launch: the gather form of the family's raster kernel (persistent workgroups walk the output
 * rows, read the pick workgroup-uniformly, compose from the record with the composer mg_render uses, stream the row out; 64-bit row offsets) with the
 * grid, LDS request and store flavour of a raster launch over `count` frames.
 * Both calls only enqueue on `stream`, allocate nothing and can be captured into a HIP graph; indices, picks and records are read at replay.
 * VALIDITY, as for instance records: a record belongs to the handle it was saved from and to the atlas it was saved under.  mg_frame_layout returns a
 * 64-bit value that is unique to the handle within the process and changes whenever something changes that a stored descriptor would draw differently:
 * everything that changes mg_instance_layout (a rebuild of the geometry -- this is also where the Mystery Path family chooses between its two composers
 * by sprite size --, mg_set_capacity, mg_set_state on the spotlight family, a new vector-observation binding) and the spotlight family's switch to its
 * border composer (black_background set for the first time, or a state loaded that has it).  The sticky hide_chessboard / black_background options
 * themselves need no new layout: the background template is a field of the descriptor and travels in the record.  The library CANNOT check this -- the
 * records carry no header: keep the value next to the records and compare before drawing (the Python mirror does); drawing a stale record is undefined
 * for its row.  mg_frame_record_bytes is sizeof the family's descriptor: 16 / 64 / 128.
 * OUT OF SCOPE: terminal-observation rows as FRAMES (final_obs_dev and the terminal descriptors the fused launches keep behind it: mg_save_frames never
 * sees them -- the frame an episode ended on is kept as a record by mg_step itself, mg_info_buffers.final_frames_dev, and drawn by mg_draw_frames like any
 * other); the MortarMayhemB ids' vector observation.  (Descriptor traces out of mg_play / mg_advance: mg_play_traced / mg_advance_traced, above.  The
 * debug view: records of its own, mg_save_debug_frames / mg_draw_debug_frames, below.)
 * mg_debug_counter "frame_saves" / "frame_draws" count the calls with count > 0, on the host.  MG_STATE_VERSION is unchanged: no state is added.
 * Errors (-1): before the first mg_reset / mg_set_state; a geometry option set since the last reset; a NULL or misaligned rec_dev / obs_dev; count < 0;
 * n_records < 1 with count > 0; an unknown format; pick_dev == NULL with count > n_records; n_records or count > INT32_MAX. */
size_t   mg_frame_record_bytes(const mg_env* env);   /* 16 / 64 / 128: sizeof the family's frame descriptor */
uint64_t mg_frame_layout(const mg_env* env);
int mg_save_frames(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream);
int mg_draw_frames(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int format, void* obs_dev,
                   void* stream);

/* EPISODE SEQUENCES: cut a rollout into episodes at `done`, chop the episodes into sequences of at most `length` steps, and draw minibatches of sequences
 * [m][length] with zero rows at the pads -- what every trainer of a recurrent or memory-based agent does with a rollout, here on the device, enqueue-only,
 * in a deterministic order.
 *   mg_split_episodes       done rows [steps][num_envs] -> a table of mg_sequence {instance, t0, len, flags}, ordered by (instance, t0)
 *   mg_sequence_picks       sequences (all, or a selection) -> pick[m][length] record indices, -1 at the pads, and an optional mask
 *   mg_draw_frames_padded   mg_draw_frames, but a pick below 0 writes its row as ZEROS and is no error
 * mg_split_episodes, DEFINITION.  done_dev is [steps][num_envs], one byte each, step-major: what a trace's done_dev holds.  For instance i let
 * n_i = steps_of_dev ? clamp(steps_of_dev[i], 0, steps) : steps; rows t >= n_i of that instance are ignored (steps_of_dev = mg_play's steps_played_dev:
 * a trace made with MG_PLAY_EPISODE or with a mask gives no sequences for steps the instance never took).  Walk t = 0 .. n_i - 1 with t0 = 0 and
 * first = start_dev ? start_dev[i] != 0 : 1:
 *   a sequence closes at t when done[t][i] is set, or t - t0 + 1 == length, or t == n_i - 1;
 *   the closing sequence is {i, t0, t - t0 + 1, (first ? MG_SEQ_FIRST : 0) | (done[t][i] ? MG_SEQ_LAST : 0)};
 *   after a sequence has closed, t0 = t + 1 and first = done[t][i].
 * The table holds all instances' sequences ordered by (instance, t0) ascending; the order is part of the definition, and no atomic decides where an entry
 * lands.  *count_dev receives the TRUE number of sequences S, also when S > capacity.  Entries 0 .. min(S, capacity) - 1 are written, nothing is written
 * at or beyond capacity, entries S .. capacity - 1 are left untouched.  capacity == 0 with seq_dev == NULL is legal and only counts.  A table is always
 * large enough at num_envs * ceil(steps / length) plus the number of set done bytes.
 * LAUNCHES: three small ones -- a lane per instance counts (lanes of a wave read 64 neighbouring bytes of a done row), one workgroup scans the
 * workgroups' sums and writes *count_dev, a lane per instance walks its column again and writes its entries, each as one 16-byte store.  The scratch (an
 * int32 per instance and one per 256 instances) is allocated AT THE HANDLE'S FIRST CALL, which therefore cannot be captured; every later call allocates
 * nothing and can be captured into a HIP graph: done_dev, steps_of_dev and start_dev are read at replay.  Nothing synchronises.
 * Errors (-1): before the first mg_reset / mg_set_state; a NULL done_dev or count_dev; steps < 1, length < 1 or capacity < 0; a NULL or not 16-byte
 * aligned seq_dev with capacity > 0; (steps + 1) * num_envs > INT32_MAX (a pick is an int32).
 * mg_sequence_picks: row j of pick_dev ([m][length] int32) is taken from sequence s = sel_dev ? sel_dev[j] : j.  With V = min(*count_dev, capacity), the
 * number of entries the table holds:
 *   0 <= s < V                  pick[j][l] = (t0 + l) * num_envs + instance for l < len, -1 for l >= len;
 *   s < 0                       a whole row of -1, no error: a minibatch padded to a fixed m;
 *   s >= V, sel_dev == NULL     a whole row of -1, no error: "all sequences" with m == capacity, capturable;
 *   s >= V, sel_dev set         a whole row of -1 and error bit 512 (mg_poll_errors).
 * mask_dev is optional, uint8 [m][length]: 1 where the pick is 0 or more.  The pick indexes the flattened [steps + 1][num_envs] frame store of a trace
 * whose row 0 is the frame before the call's first step (the Python mirror's RolloutTrace.frames) -- row t there is the observation action t was played
 * in -- and the same number indexes the flattened [steps][num_envs] action, label, reward and done rows.  ONE launch, a lane per element; count_dev is
 * read on the device, nothing synchronises, nothing is allocated; capturable.  num_envs is the handle's.
 * Errors (-1): a NULL count_dev or pick_dev; capacity < 0; a NULL or misaligned seq_dev with capacity > 0; m < 0; length < 1; m * length > INT32_MAX.
 * mg_draw_frames_padded: mg_draw_frames with ONE difference -- a pick below 0 writes its row as zeros, every byte, in every format, and raises no error.
 * Everything else is mg_draw_frames word for word: a pick at or above n_records leaves its row untouched and raises bit 512; a record the composer skips
 * leaves its row untouched; the refusals, the 64-bit row offsets, the single launch (the PAD form of the family's gather raster: the workgroup that meets
 * a padding row stores 21,168 / 42,336 / 84,672 bytes of zeros as 16-byte vectors straight from registers, without a compose) and capturability are the
 * same.  pick_dev == NULL is legal and then equals mg_draw_frames.
 * mg_debug_counter "sequence_splits" counts the mg_split_episodes calls, "padded_draws" the mg_draw_frames_padded calls with count > 0, on the host.
 * MG_STATE_VERSION is unchanged: no state is added.
 * OUT OF SCOPE: sliding memory windows for transformer agents (windows of their own: mg_window_picks, below, and there a window does reach into the
 * previous trace); sequences that continue across two traces (the start of a trace starts a sequence,
 * start_dev only sets the MG_SEQ_FIRST flag); terminal frames inside a traced call (still the trace's own open item); the MortarMayhemB ids' vector
 * observation per step. */
typedef struct mg_sequence { int32_t instance, t0, len, flags; } mg_sequence;   /* 16 bytes, stored as one vector */
#define MG_SEQ_FIRST 1   /* the sequence starts an episode */
#define MG_SEQ_LAST  2   /* the sequence ends with its episode's done */
int mg_split_episodes(mg_env* env, const uint8_t* done_dev, int32_t steps, const int32_t* steps_of_dev, const uint8_t* start_dev,
                      int32_t length, mg_sequence* seq_dev, int32_t capacity, int32_t* count_dev, void* stream);
int mg_sequence_picks(mg_env* env, const mg_sequence* seq_dev, const int32_t* count_dev, int32_t capacity, const int32_t* sel_dev,
                      int32_t m, int32_t length, int32_t* pick_dev, uint8_t* mask_dev, void* stream);
int mg_draw_frames_padded(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int format,
                          void* obs_dev, void* stream);

/* MEMORY WINDOWS: for every training sample (t, i) the window of instance i's previous `window` steps inside the same episode, with a mask and a length --
 * what a TransformerXL-style agent with a sliding episodic memory trains on -- and the gather of such windows from a trainer's own per-step store
 * (hidden states, values, log-probs) with zero rows at the pads.  A window reaches back over an episode's earlier steps INCLUDING INTO THE PREVIOUS TRACE.
 *   mg_episode_positions    done rows [steps][num_envs] -> pos [steps + 1][num_envs]: how many steps the episode of a store row had already taken
 *   mg_window_picks         positions, samples (all, or a selection) -> pick[m][window] row indices, -1 at the pads, an optional mask and length
 *   mg_gather_rows_padded   rows of ANY byte length gathered by pick; a pick below 0 writes its row as ZEROS and is no error
 * All three are enqueue-only on `stream`, synchronise nothing, keep no scratch in the handle and allocate nothing -- so even a handle's first call can be
 * captured into a HIP graph; the arrays are read at replay, the integers are the captured values.  MG_STATE_VERSION is unchanged: no state is added.
 * mg_episode_positions, DEFINITION.  done_dev is [steps][num_envs] bytes, step-major: a trace's done_dev.  pos_dev is int32 [steps + 1][num_envs]: row t
 * is the number of steps instance i's current episode had already taken when the observation of row t of the [steps + 1][num_envs] frame store was shown
 * (row 0 of that store is the frame before the call's first step, as in mg_sequence_picks).  With n_i as in mg_split_episodes (steps_of_dev clamped to
 * 0 .. steps, NULL: steps):
 *   pos[0][i]   = pos0_dev ? max(pos0_dev[i], 0) : 0
 *   pos[t+1][i] = done[t][i] ? 0 : pos[t][i] + 1     for t <  n_i     (a position stops counting at INT32_MAX)
 *   pos[t+1][i] = pos[t][i]                          for t >= n_i
 * Row `steps` is the carry-out: passed as pos0_dev of the next trace's call it makes positions continue across two traces.  Under MG_PLAY_EPISODE the
 * carry-out of a finished instance is 0, which is right once the caller has reset it.
 * LAUNCHES: one small one, a lane per instance walking its column; the lanes of a wave read 64 neighbouring bytes of a done row and store 64 neighbouring
 * int32, as the split's count kernel does.  No atomic, no scratch.
 * Errors (-1): before the first mg_reset / mg_set_state; a NULL done_dev or pos_dev; steps < 1; (steps + 1) * num_envs > INT32_MAX.
 * mg_window_picks, DEFINITION.  Row j of pick_dev ([m][window] int32) belongs to sample s = sel_dev ? sel_dev[j] : j, with s = t * num_envs + i and
 * 0 <= t <= steps (row `steps` is the bootstrap observation).  pos_dev is what mg_episode_positions wrote for this trace.  Let
 *   e   = t - pos[t][i]                   the episode's first row, which may be negative: the episode began in an earlier trace
 *   hi  = t - lag
 *   lo  = max(e, hi - window + 1, -back)
 *   len = max(0, hi - lo + 1)
 * then pick[j][l] = (back + lo + l) * num_envs + i for l < len, and -1 behind it: the valid picks first, oldest first, the pads after them -- the
 * sequences' convention.  A pick indexes a store of [back + steps + 1][num_envs] rows whose first `back` rows are the LAST `back` rows before row 0 of
 * this trace: rows K_prev - back .. K_prev - 1 of the previous trace's [K_prev + 1][num_envs] store (its row K_prev is this trace's row 0).  back = 0 keeps
 * a window inside the trace.  lag = 0: the window ends with the sample's own observation (windows of frames); lag = 1: it ends one step earlier
 * (TransformerXL memories of past hidden states); any lag >= 0 is legal.  mask_dev (uint8 [m][window], 1 where the pick is 0 or more) and len_dev
 * (int32 [m]) are optional.
 *   s < 0                                              a whole row of -1, len 0, no error: a minibatch padded to a fixed m;
 *   s >= (steps + 1) * num_envs, sel_dev set           a whole row of -1, len 0 and error bit 512 (mg_poll_errors);
 *   sel_dev == NULL                                    m <= (steps + 1) * num_envs is required.
 * ONE launch, a lane per element; pos_dev and sel_dev are read at replay.  num_envs is the handle's.
 * Errors (-1): a NULL pos_dev or pick_dev; steps < 1, m < 0, window < 1, lag < 0 or back < 0; m * window > INT32_MAX;
 * (back + steps + 1) * num_envs > INT32_MAX; sel_dev == NULL with m > (steps + 1) * num_envs.
 * mg_gather_rows_padded: row j of dst_dev receives row pick_dev[j] of src_dev ([n_rows] rows), row_bytes bytes each, for any row_bytes >= 1 and any
 * alignment of the two bases.  A pick below 0 writes the row as zeros, every byte, and is no error; a pick at or beyond n_rows leaves the row untouched and
 * raises bit 512; pick_dev == NULL means row j, and then count <= n_rows is required.  src and dst must not overlap: the call refuses it where the two
 * ranges (n_rows rows, count rows) share a byte.  Byte offsets are 64-bit.
 * ONE launch.  The host chooses the widest access of 16 / 8 / 4 / 2 / 1 bytes that divides row_bytes and both base addresses.  Rows of 32 accesses or more
 * take the ROW form: a wave walks four neighbouring output rows together, the picks read wave-uniformly, the four rows' loads of a round issued before
 * its first store, a zero row stored straight from registers.  Shorter rows (an action, a reward, a done byte) take the PACKED form: lanes over the
 * flattened count * row_bytes / width accesses, so that a wave is not spent on 4 bytes.  No LDS, no barrier, no atomic except the error word's.
 * Errors (-1): count, n_rows < 0 or > INT32_MAX; row_bytes < 1 or > INT32_MAX; pick_dev == NULL with count > n_rows; with count > 0: a NULL dst_dev, a
 * NULL src_dev with n_rows > 0, overlapping ranges.
 * mg_debug_counter "episode_positions", "window_picks" and "row_gathers" count the calls that were not refused, on the host.
 * OUT OF SCOPE: windows that reach back over more than one earlier trace in one store (assemble a longer prefix: the definition only needs `back` rows
 * in front of row 0); attention masks for segment-level recurrence with gradients across segments; terminal frames inside a traced call. */
int mg_episode_positions(mg_env* env, const uint8_t* done_dev, int32_t steps, const int32_t* steps_of_dev, const int32_t* pos0_dev,
                         int32_t* pos_dev, void* stream);
int mg_window_picks(mg_env* env, const int32_t* pos_dev, int32_t steps, const int32_t* sel_dev, int32_t m, int32_t window, int32_t lag,
                    int32_t back, int32_t* pick_dev, uint8_t* mask_dev, int32_t* len_dev, void* stream);
int mg_gather_rows_padded(mg_env* env, const void* src_dev, int64_t n_rows, int64_t row_bytes, const int32_t* pick_dev, int64_t count,
                          void* dst_dev, void* stream);

/* ROLLOUT TARGETS: what a PPO trainer computes between "rollout done" and "first minibatch" -- generalised advantage estimates, returns, a mask of the
 * rows that have a target, and the moments advantages are normalised with -- from a rollout's reward / done rows and the critic's values, on the device.
 *   mg_rollout_targets   reward, done [steps][num_envs], value [steps + 1][num_envs] -> adv, ret, valid [steps][num_envs], col [3][num_envs]
 *   mg_sum_columns       col [rows][num_envs] -> out [rows], summed in a fixed order
 * Both are enqueue-only on `stream`, synchronise nothing, keep no scratch in the handle and allocate nothing -- so even a handle's first call can be
 * captured into a HIP graph; the arrays are read at replay, gamma, lambda and steps are the captured values.  MG_STATE_VERSION is unchanged: no state
 * is added.
 * ARRAYS.  reward_dev (float32), done_dev, skip_dev, trunc_dev (one byte each) and final_value_dev (float32) are [steps][num_envs], step-major: what a
 * trace holds; skip_dev, trunc_dev and final_value_dev are optional.  value_dev is float32 [steps + 1][num_envs]: row t is the critic's value of row t of
 * the [steps + 1][num_envs] frame store (the convention of mg_sequence_picks: row 0 is the frame before the call's first step), row `steps` the bootstrap
 * value.  adv_dev, ret_dev (float32 [steps][num_envs]), valid_dev (uint8 [steps][num_envs]) and col_dev (double [3][num_envs]) are each optional, but at
 * least one of them must be given; a NULL output is not written.
 * mg_rollout_targets, DEFINITION.  n_i as in mg_split_episodes: steps_of_dev clamped to 0 .. steps, NULL: steps.  Every arithmetic step below is one
 * IEEE float32 operation, rounded to nearest and never fused.  gl = gamma * lambda, computed once on the host in float32.  For instance i start with
 * a = 0 and walk t = steps - 1 down to 0:
 *   t >= n_i, or skip_dev set and skip[t][i] != 0   the row has no target: adv = ret = 0, valid = 0, a = 0, and on to the next row;
 *   v = value[t][i], r = reward[t][i];
 *   done[t][i] != 0                                 carry = 0; nv = (trunc_dev set and trunc[t][i] != 0) ? (final_value_dev ? final_value[t][i]
 *                                                   : value[t+1][i]) : 0;
 *   otherwise                                       nv = value[t+1][i], carry = a;
 *   delta = (r + gamma * nv) - v;  a = delta + gl * carry;
 *   adv[t][i] = a, ret[t][i] = a + v, valid[t][i] = 1.
 * The multiply by nv = 0 and the add are part of the definition: a reward of -0.0 on a terminal row gives what the loop gives.  lambda = 1 gives
 * discounted returns-to-go in ret.  col_dev holds, for instance i, col[0][i] the count, col[1][i] the sum and col[2][i] the sum of squares of its valid
 * adv values, accumulated in the walk's own order (t descending), each a rounded double operation: (double)a * (double)a, then the add.
 * HOW THE CONVENTIONS MAP ON THE DEFINITION.
 *   same-step auto-reset                     nothing but done: the next value row belongs to the new episode and is not looked at;
 *   same-step auto-reset, truncated ends     additionally trunc_dev and final_value_dev, the critic's value of the terminal observation
 *                                            (mg_info_buffers.final_obs_dev / final_frames_dev rows);
 *   next-step auto-reset (mg_step_next)      skip[t] = the restart flags of call t -- the row after an episode's end is a reset row, not a transition:
 *                                            it gives no target and does not leak into its neighbours -- and trunc_dev WITHOUT final_value_dev: the
 *                                            terminal observation is frame row t + 1, so value[t+1] is its value.
 * mg_sum_columns writes out[r] = the sum of col[r][0 .. num_envs - 1] in this FIXED order, which is part of the definition: 256 partial sums, partial
 * l starting at 0.0 and adding instances l, l + 256, l + 512, ... ascending; then the halving tree part[l] += part[l + h] for l < h, h = 128, 64, ..., 1;
 * out[r] = part[0].  Every add is one rounded double operation; no atomic is used.  num_envs is the handle's.  With rows = 3 and mg_rollout_targets'
 * col_dev it gives the count, the sum and the sum of squares of all valid advantages.
 * LAUNCHES: mg_rollout_targets is ONE launch, a lane per instance walking its column backwards in blocks of 16 rows whose loads are all issued before
 * the first is used; the lanes of a wave read 256 neighbouring bytes of a float row and 64 of a flag row and store the same shapes; value[t+1] is the
 * row loaded one step earlier.  No LDS, no atomic, no scratch.  mg_sum_columns is one small launch, a 256-lane workgroup per row.
 * Errors (-1), mg_rollout_targets: before the first mg_reset / mg_set_state; a NULL reward_dev, done_dev or value_dev; all four outputs NULL;
 * steps < 1; (steps + 1) * num_envs > INT32_MAX; gamma or lambda outside [0, 1] or NaN; final_value_dev without trunc_dev; an output range that shares
 * a byte with an input range or with another output.  mg_sum_columns: rows < 1; a NULL col_dev or out_dev.
 * mg_debug_counter "rollout_targets" counts the mg_rollout_targets calls that were not refused, on the host.
 * OUT OF SCOPE: values in bf16 / f16; rows of a masked rollout in which an instance merely paused (those are not cuts: only steps_of_dev and skip_dev
 * are understood); V-trace and other off-policy corrections; normalising inside the kernel (the moments are there for the caller to do it). */
int mg_rollout_targets(mg_env* env, const float* reward_dev, const uint8_t* done_dev, const float* value_dev, int32_t steps,
                       const int32_t* steps_of_dev, const uint8_t* skip_dev, const uint8_t* trunc_dev, const float* final_value_dev,
                       float gamma, float lambda, float* adv_dev, float* ret_dev, uint8_t* valid_dev, double* col_dev, void* stream);
int mg_sum_columns(mg_env* env, const double* col_dev, int32_t rows, double* out_dev, void* stream);

/* DEBUG-VIEW RECORDS: keep the ground-truth view of a FEW instances and draw it later.  mg_render_debug draws every instance at once, from the current state,
 * synchronously: at 65,536 instances 22 GB of views and 1.4 GB of scratch to look at one of them.  But a debug view, like a frame, is a pure function of a
 * descriptor of the family's frame-descriptor type (16 / 64 / 128 B) and the handle's atlas -- the descriptor mg_render_debug fills for every instance before it
 * draws.  A trainer that logs a short video of what is hidden from the agent saves the descriptors of the instances it watches, one small launch per step,
 * and draws all of them with one launch at the end.
 *   mg_save_debug_frames   record j <- the debug-view descriptor of instance idx_dev[j]   (idx_dev == NULL: instance j, and then count <= num_envs)
 *   mg_draw_debug_frames   row j of rgb_dev <- the view of record pick_dev[j]              (pick_dev == NULL: record j, and then count <= n_records)
 * DEFINITION: take a handle and a twin with the same history; every time mg_render_debug is called on the twin, mg_save_debug_frames is called on the handle
 * for a set S of instances.  Then for every i in S the saved record, drawn at size 336, gives bit for bit row i of the twin's output at that moment; and an
 * instance outside S behaves like an instance of a handle on which no debug render was ever made.
 * mg_save_debug_frames computes the descriptor from the CURRENT state, exactly what mg_render_debug computes for that instance, and counts as ONE debug render
 * of the named instances and of no other: on the five Mortar Mayhem ids the named instance's count of entries popped from the CLONE of the command
 * visualisation list (see mg_render_debug) advances by one; nothing else in the handle changes, and an instance that is not named keeps its count.  Index
 * conventions of mg_save_frames: an entry < 0 is skipped, an entry >= num_envs is skipped and raises error bit 512; a skipped entry leaves its record
 * untouched and its instance is not popped.  Entries must be DISTINCT: a repeated index is not detected, and on the Mortar Mayhem ids it leaves that
 * instance's pop count and the records of its duplicate entries undefined (on the other ids the duplicates hold the same descriptor).  Records are
 * mg_frame_record_bytes each and valid under mg_frame_layout, by the rules of the frame records -- but they are NOT frame records: mg_draw_frames draws
 * something else from them.  One launch, one lane per entry.  Endless-MysteryPath-v0: the view reads the path segments, so segments the handle still owes
 * are generated first, by a launch on `stream` in front of the save (as for mg_save_instances); nothing synchronises.
 * mg_draw_debug_frames: ONE launch, the gather form of the family's raster kernel with the composer mg_render_debug uses for the handle.  size 336: rgb_dev
 * is uint8 [count][336 y][336 x][3], the reference's debug_rgb_array -- every pixel of the debug surface four times per axis, out[y][x][c] =
 * surface[x >> 2][y >> 2][c], written straight from the composed frame as 16-byte stores (no second pass over memory; 64-bit row offsets).  size 84: rgb_dev
 * is uint8 [count][84 x][84 y][3], the debug surface before its stretch, in the observation layout.  Any other size: -1.  These are no observation formats:
 * the MG_OBS_* values and mg_set_obs_format are untouched.  Picks as for mg_draw_frames: one outside 0 .. n_records-1 leaves its row untouched and raises bit
 * 512, duplicates are legal, count == 0 does nothing.
 * Both calls only enqueue on `stream`, allocate nothing and can be captured into a HIP graph; indices, picks and records are read at replay.  mg_render_debug
 * is unchanged.  mg_debug_counter "debug_frame_saves" / "debug_frame_draws" count the calls with count > 0, on the host.  MG_STATE_VERSION is unchanged: no
 * state is added.
 * Errors (-1): those of mg_save_frames / mg_draw_frames (rgb_dev in the place of obs_dev); idx_dev == NULL with count > num_envs; a size other than 84 / 336. */
int mg_save_debug_frames(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream);
int mg_draw_debug_frames(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int size, void* rgb_dev,
                         void* stream);

/* Measurement hooks (bench.py's roofline leg): mg_set_profiling(env, N) makes every N-th mg_step (N = 1: every step,
 * 0: off) bracket its kernels with hipEvents recorded on the launch stream (a bracketed step costs ~15 us of stream
 * time, hence the sampling).  mg_get_profile(kind) synchronises, returns the summed elapsed milliseconds and the
 * number of bracketed launches since the last call, and clears.  kind 0 = logic kernel (one lane per instance),
 * kind 1 = raster kernel (the HBM-write-bound one). */
int mg_set_profiling(mg_env* env, int on);
int mg_get_profile(mg_env* env, int kind, double* total_ms, int64_t* launches);

/* Device-side error bits raised by the kernels since the last call (the reference's only failure paths are Python
 * exceptions, e.g. pygame_assets.py:723-724 "No valid path found"); 0 = none.  Synchronous.
 *   1  spotlight slots exhausted (more than 16 live spotlights)      2  path generation found no valid path
 *   4  endless path longer than 128 segments                         8  more than 128 distinct fall-off cells
 *  16  past-path window wider than 16 columns
 *  32  Endless Mortar Mayhem: the command list reached its capacity of 512 entries (the reference's list is unbounded,
 *      endless_mortar_mayhem.py:316-318); the episode of that instance was ended
 *  64  a deferred-reset queue was found over-full (an earlier fused launch failed before draining it); the excess
 *      entries were dropped
 * 256  SearingSpotlights-v0: use_exit = False at the reset of an instance that has never had an exit (the reference raises
 *      AttributeError there, searing_spotlights.py:431-435; with an earlier exit it keeps drawing that one, and so does this
 *      library); no exit was drawn
 * 512  mg_save_instances / mg_load_instances / mg_save_frames / mg_draw_frames / mg_save_debug_frames / mg_draw_debug_frames: an instance index
 *      >= num_envs, or a record index outside the call's records; the entry was skipped, nothing else changed
 * 128  reserved (rounds <= 3: a frame workgroup of the mortar family's one-launch step gave up waiting for its descriptor.
 *      Since round 4 that launch cannot time out -- a frame wave that waits too long steps the instances itself,
 *      mg_mortar.hip mortar_step_raster_kernel -- and the bit is never raised) */
int mg_poll_errors(mg_env* env, int* flags);

/* The same bits as they stand right now: no synchronisation, nothing cleared.  The error word lives in pinned host
 * memory that the kernels update with system-scope atomics, so a trainer can look after every mg_step for free and
 * sees a bit at the latest one step after the kernel that raised it finished.  (SearingSpotlights option sets that
 * overflow the 16 slots in every long enough episode are refused by mg_reset up front; the bit covers the rest.) */
int mg_peek_errors(mg_env* env, int* flags);

/* Observation-buffer allocator (optional; any device-accessible obs_dev works with mg_reset / mg_step).  The reference
 * has no counterpart: its observation is a host numpy array returned by pygame.surfarray.array3d
 * (mortar_mayhem_grid.py:277,372); here the batch of observations is one device buffer that the raster kernel streams
 * into, and WHERE that buffer lies in HBM decides 12-15 % of the kernel's speed: the MI355X's memory falls into three
 * zones of ~96 GB, a store stream confined to one zone runs at 5.1-5.5 TB/s, one split over two zones at 6.2-6.4 TB/s
 * (profiles/r02_zones.md), and an ordinary allocation lies in one zone.  mg_obs_alloc builds the buffer with the HIP
 * virtual-memory API from 304-MiB physical pieces, each classified against the first one with a 0.1-ms two-window store
 * probe, half of them from the first piece's zone and half from elsewhere, mapped alternately into one contiguous
 * virtual range (rounded up to whole pieces).  Pieces it does not need and spacer allocations of 8 GiB that are never
 * mapped or written keep the driver's allocator moving during the search and are released before the call returns (at
 * most `search_budget_bytes` in total; MG_OBS_SEARCH_DEFAULT = half of the free memory, at most 128 GiB: that much
 * VRAM is transiently unavailable to other processes on the GPU; 0 = no search.  A pristine VRAM can hand out 100-130 GiB
 * of ONE zone in a row: with the default budget such a process gets the plain allocation, info.zones == 1).  Pieces are
 * classified by thresholds that start from the figures measured on the development boxes and turn RELATIVE (geometric
 * mean of the slowest and the fastest pair seen, -/+ 3 %) once both kinds of pair have been observed.  Buffers of 304 MiB or
 * less, and runtimes without hipMemCreate, get a plain hipMalloc.  The range is accessible from the owning device and from
 * every device that reports peer access to it.  Virtual address ranges are never returned to the runtime (a reused range can
 * keep stale translations on ROCm 7.2): a process that allocates and frees buffers for ever uses address space, not memory.
 * Synchronous; 2-10 ms typically.  The search is bounded in time (mg_obs_set_search_ms, default 1,500 ms): the clock is read
 * after every handle the walk creates and the walk ends when the time spent plus the projected cost of handing everything
 * back would pass the bound, so that the call as a whole stays within 1.5 x the bound plus the assembly of the buffer
 * (info.search_ms; a search that runs out of time ends with what it has: two zones if it found them, else the plain
 * allocation).  The library reads no environment variable for any of this (the Python mirror forwards MEMGYM_OBS_SEARCH_MS /
 * MEMGYM_OBS_SEARCH_GB as arguments).  mg_obs_free releases a buffer obtained here (after synchronising the device); the
 * pieces go to a pool of at most ten for the next buffer. */
typedef struct mg_obs_alloc_info {
    int zones;               /* 2, 3 = pieces from that many zones; 1 = no second zone within the budget (plain
                              * allocation); 0 = plain allocation without a search (small buffer, no room)          */
    int pieces;              /* physical pieces mapped                                                                */
    size_t piece_bytes;
    size_t searched_bytes;   /* bytes of unused pieces and spacers walked over (transient, released)                  */
    double probe_same_tbps;  /* store probe, first piece + a piece classified "same zone" (largest seen; ~5.1)        */
    double probe_cross_tbps; /* ... + a piece classified "other zone" (smallest seen; ~6.3); 0 = none seen            */
    double search_ms;
} mg_obs_alloc_info;
#define MG_OBS_SEARCH_DEFAULT ((size_t)-1)
int mg_obs_alloc(int device, size_t bytes, size_t search_budget_bytes, void** out_dev, mg_obs_alloc_info* info);
/* The same for a buffer whose observations are `frame_bytes` each (= mg_obs_bytes of the handle: 21,168 for MG_OBS_U8_XYC and MG_OBS_U8_CYX -- what
 * mg_obs_alloc assumes --, 42,336 for the 16-bit formats, 84,672 for MG_OBS_F32_CYX).  A raster launch writes at fronts that are one
 * WINDOW = 14,336 observations apart, and the split that is fast is the one of the concurrently written fronts: pieces are dealt to the
 * zones window by window (neighbouring windows start in different zones, a window's pieces alternate).  For windows of about one
 * piece that is mg_obs_alloc's alternating order; for the 16-bit formats (1.9 pieces per window) the alternating order leaves all
 * fronts in one zone at any time (round 6: bfloat16 observations at 65,536 instances 0.72 -> 0.83 of peak). */
int mg_obs_alloc_for(int device, size_t bytes, size_t frame_bytes, size_t search_budget_bytes, void** out_dev, mg_obs_alloc_info* info);
/* The order mg_obs_alloc_for would use, without allocating anything (no GPU needed): returns the number of pieces k of a buffer of
 * `bytes` and, for the first max_pieces of them, the zone (0 .. zones - 1; zones = 2 or 3) each is taken from; *lead_bytes = where in the
 * assembled range the buffer starts (it sits in the middle of the k pieces).  tests/test_obs_plan.py walks the fronts of a launch over it. */
int mg_obs_plan(size_t bytes, size_t frame_bytes, int zones, size_t* piece_bytes, size_t* lead_bytes, int* zone_of_piece, int max_pieces);
int mg_obs_free(void* obs_dev);
int mg_obs_set_search_ms(double ms);  /* process-wide; >= 0 */
/* Measurement hook (bench.py's per-box control: roofline.box_probe_GBps).  DESTROYS THE BUFFER'S CONTENTS: the n_frames x 21,168
 * bytes at obs_dev are overwritten with zeros -- a caller that probes a live observation buffer steps or renders (mg_render) afterwards.
 * ONE launch of a pure store stream on `stream`; the caller times it with events.  pattern 0 = linear fill, one 16-byte store per
 * thread (the memory system's ceiling for stores at this size and placement); pattern 1 = the raster's store shape without compose
 * work (persistent 256-lane workgroups writing whole frames; the raster's grid and residency): a CONTROL for the raster, not a ceiling
 * (a raster with compose work can beat it); patterns 2 / 3 = other frame-shaped streams measured in round 5 (pairs of adjacent
 * vectors per lane; pairs + each wave a contiguous quarter of the frame: tools/store_shapes.py, profiles/r05_store_shapes.md); patterns
 * 4 / 5 (round 6, profiles/r06_store_counters.md): the frame walk with line-aligned ownership (every 128-byte line written by one
 * workgroup); one frame per workgroup without the persistent loop; 6 / 7: the frame walk with neighbouring frames on the same XCD;
 * eight consecutive frames per workgroup as 64-byte-aligned spans. */
int mg_store_probe(void* obs_dev, size_t n_frames, int pattern, void* stream);
/* Test hook: live buffers, pooled spare pieces, bytes of virtual address space reserved so far. */
int mg_obs_debug_stats(size_t* live_buffers, size_t* pooled_pieces, size_t* reserved_va_bytes);

/* Multi-GPU helper for caller-owned observation memory on ANOTHER GPU of the node (BASELINE config 5: rank r's raster
 * kernels store their frames straight into rank 0's buffer over xGMI; memory_gym_amd/dist.py PeerObsBuffer): checks
 * hipDeviceCanAccessPeer(device, peer_device) and switches peer access on for `device`.  0 = the kernels of a handle on
 * `device` may be given pointers into `peer_device`'s memory; -1 = no peer access (fall back to a gather). */
int mg_enable_peer_access(int device, int peer_device);

/* Test / telemetry hook: named counters of a handle.  "one_launch_rescues" (mortar family): 64-instance slots of the one-launch
 * step that a frame wave stepped itself because the step workgroup's wave had not claimed them in time (0 on a GPU that
 * dispatches the step workgroups first; tests/test_gpu_one_launch.py forces the other order).  "path_gen_ticks" / "path_gen_paths"
 * (finite Mystery Path: wave-ticks and paths of the A* generation inside the step's launches; "path_lane_paths": those of them that the
 * lane-per-path generator made, which serves a raster launch's queue of more than 1,024 resets).  "emp_ahead_records"
 * (Endless-MysteryPath: first segments of NEXT episodes generated ahead of time, which a finishing instance's own step turns into its
 * reset -- EndlessMysteryPathEnv.reset, endless_mystery_path.py:195-280, without a queue entry); "emp_own_resets" (such resets; counted
 * by the lab build only).  "one_launch_steps" (mortar family): mg_step calls of this handle that went out as the one-launch kernel, counted
 * on the host.  "spot_fused_steps" (spotlight family): mg_step calls of this handle that went out as the fused raster / reset launch
 * (spot_raster_serve_kernel), counted on the host.  "emp_fused_steps" (Endless-MysteryPath): mg_step calls of this handle that went out as the
 * fused raster / service launch (emp_raster_serve_kernel), counted on the host.  "final_obs_generic_steps" (every id): mg_step calls of this handle that kept terminal observations
 * (mg_info_buffers.final_obs_dev, autoreset) on the generic path -- a step without auto-reset, a copy of the finished rows, a masked reset --
 * instead of inside the step's own launches, counted on the host.  "headless_steps" (every id): headless steps of this handle -- mg_step calls
 * with obs_dev == NULL and the steps mg_advance took through its loop form; "advance_fused_steps" (every id; only the mortar family has the
 * form): steps mg_advance took inside mortar_advance_kernel.  Both counted on the host.  "play_fused_steps" (every id; only the mortar family
 * has the form): steps mg_play took inside mortar_play_kernel; the steps of its loop form count as "headless_steps" and, where a mask applied,
 * "masked_steps".  "instance_saves" / "instance_loads" (every id):
 * mg_save_instances / mg_load_instances calls of this handle with count > 0, counted on the host.  "frame_saves" / "frame_draws" (every id): the same
 * for mg_save_frames / mg_draw_frames; "debug_frame_saves" / "debug_frame_draws" (every id): the same for mg_save_debug_frames / mg_draw_debug_frames.
 * "traced_steps" / "traced_fused_steps" (every id; only the mortar family has the in-launch form): steps of
 * mg_advance_traced / mg_play_traced calls that came with a trace, and those of them taken inside mortar_advance_traced_kernel / mortar_play_traced_kernel.
 * Unknown name: -1.  Synchronous. */
int mg_debug_counter(mg_env* env, const char* name, int64_t* value);

/* Test hook: copy the numpy-compatible PCG64 words of instance i to host:
 * out[6] = {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger}.  Synchronous. */
int mg_debug_rng(mg_env* env, int32_t i, uint64_t* out);
/* Test hook, the reverse: instance i continues with the PCG64 stream given in the same six words -- the reference's
 * `env.np_random = np.random.Generator(bit_generator with this state)` at this point of the episode.  Nothing else of the instance
 * changes, except that whatever a family had computed ahead of time from the old stream is dropped (Endless-MysteryPath: the next
 * episode's first segment).  in[3] (the increment's low word) must be odd.  Synchronous: work
 * in flight and work put off is finished first, the words are written with host copies -- no kernel of the library reads this hook.
 * tests/test_gpu_rng_edges.py uses it to put rejected and extreme draws where the device restates numpy's stream. */
int mg_debug_set_rng(mg_env* env, int32_t i, const uint64_t* in);

#ifdef __cplusplus
}
#endif
#endif
