/*
 * simpletetris.h -- C ABI of the MI355X batched SimpleTetris step engine.
 *
 * This is the drop-in boundary for gym-simpletetris' per-step hot path.  The
 * reference has no FFI: its interface is the Python class
 * TetrisEnv/TetrisEngine in /root/reference/gym_simpletetris/envs/tetris_env.py.
 * Each entry point below names the reference method it replaces; the Python
 * host package (gym-simpletetris_amd/gym_simpletetris_amd) binds these with
 * ctypes and re-exposes the reference's Gym surface.
 *
 * Conventions
 *  - All functions return ST_OK (0) or a negative st_status; the message of
 *    the last failure on the calling thread is st_last_error().
 *  - Pointers named d_* are DEVICE pointers on the context's device; the
 *    caller owns them.  Context state (boards, pieces, counters, MT19937
 *    states) is owned by the context and lives in HBM.
 *  - Every call that takes a stream is asynchronous on that stream
 *    (NULL = the device's null stream).  Calls on one context must be
 *    serialised by the caller (the reference env is not thread-safe either,
 *    tetris_env.py:187 uses the global `random`).
 *  - Env e's piece RNG is CPython's MT19937 seeded with random.seed(seed[e]):
 *    results equal the reference run under the per-env isolation protocol
 *    (random.setstate/getstate around every reset/step of env e).
 */
#ifndef SIMPLETETRIS_H
#define SIMPLETETRIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: st_step_wire carries the reward's 32 bits (st_wire_words grew by one
 * word for 10x20), st_unwire_shards.  3: st_gate_actions / st_gate_wait,
 * st_stream_wait (additions only).  4: st_step_n (addition only).
 * st_step_export: addition only, version unchanged (a build without it is
 * refused by the host package when it binds the symbol); so are
 * st_after_slots / st_afterstates / st_placement_actions,
 * st_policy_linear / st_play_linear, st_place / st_step_placements /
 * st_play_linear_placements, st_reachable / st_route_actions and
 * st_feature_rows / st_afterstates_set / st_policy_linear_set /
 * st_play_linear_set, st_next_piece / st_policy_lookahead /
 * st_play_lookahead, st_routes / st_policy_routed / st_play_routed,
 * st_fork, st_next_weights / st_policy_expect / st_play_expect, and
 * st_lock_set / st_afterstates_at / st_routes_at / st_policy_locks /
 * st_play_locks, and st_ntuple_set / st_ntuple_table_len / st_ntuple_eval /
 * st_policy_ntuple / st_play_ntuple.
 * Snapshots (st_save) keep their own format version, unchanged. */
#define ST_ABI_VERSION 4

typedef struct st_ctx st_ctx;
typedef void *st_stream; /* hipStream_t */

typedef enum st_status {
    ST_OK = 0,
    ST_EINVAL = -1,  /* bad argument (reference: ValueError/KeyError) */
    ST_ENOMEM = -2,  /* device allocation failed */
    ST_EHIP = -3,    /* HIP runtime error */
    ST_ESTATE = -4   /* call order violated (e.g. step before seed) */
} st_status;

/* Scoring / rule flags: TetrisEngine.__init__ kwargs, tetris_env.py:126-137. */
enum st_flags {
    ST_REWARD_STEP = 1u << 0,               /* reward_step              :256 */
    ST_PENALISE_HEIGHT = 1u << 1,           /* penalise_height          :286 */
    ST_PENALISE_HEIGHT_INCREASE = 1u << 2,  /* penalise_height_increase :288 */
    ST_ADVANCED_CLEARS = 1u << 3,           /* advanced_clears          :266 */
    ST_HIGH_SCORING = 1u << 4,              /* high_scoring             :270 */
    ST_PENALISE_HOLES = 1u << 5,            /* penalise_holes           :294 */
    ST_PENALISE_HOLES_INCREASE = 1u << 6,   /* penalise_holes_increase  :296 */
    ST_STEP_RESET = 1u << 7                 /* step_reset               :248 */
};

/* What st_step does when an env dies (reference: the caller decides). */
enum st_autoreset {
    ST_AUTORESET_NONE = 0,     /* exact single-env semantics: state stays as the
                                  reference leaves it after a death step (incl.
                                  the R8 erase at tetris_env.py:303); caller
                                  calls st_reset(mask) like `if done: reset()` */
    ST_AUTORESET_SAME_STEP = 1 /* TetrisEngine.clear() runs inside the same
                                  kernel; obs is the terminal obs, terminal
                                  counters go to the ST_STAT_EP_* rows */
};

typedef struct st_config {
    int32_t width;      /* 4..32   (TetrisEnv width=10,  tetris_env.py:344) */
    int32_t height;     /* 4..28   (TetrisEnv height=20, tetris_env.py:345) */
    int32_t lock_delay; /* <= 32766 (tetris_env.py:356; negative acts as 0, :175) */
    uint32_t flags;     /* st_flags */
    int32_t autoreset;  /* st_autoreset */
} st_config;

/* Per-env int32 counters, SoA rows of the stats block (TetrisEngine.get_info,
 * tetris_env.py:232-241). */
enum st_stat {
    ST_STAT_TIME = 0,
    ST_STAT_SCORE = 1,
    ST_STAT_LINES = 2,
    ST_STAT_HOLES = 3,
    ST_STAT_PIECE_HEIGHT = 4,
    ST_STAT_DEATHS = 5,
    ST_STAT_COUNT0 = 6,   /* shape_counts T,J,L,Z,S,I,O: rows 6..12 */
    ST_STAT_MT_INDEX = 13,/* MT19937 index (0..624); see st_mt_sync */
    ST_STAT_PIECE = 14,   /* the piece word (uint32, = st_state_views.piece) */
    ST_STAT_EP_TIME = 15, /* terminal counters of the last finished episode */
    ST_STAT_EP_SCORE = 16,/* (ST_AUTORESET_SAME_STEP only)                   */
    ST_STAT_EP_LINES = 17,
    ST_STAT_EP_HOLES = 18,
    ST_NSTAT = 19
};

/* Device views of the context-owned state.  `stride` (>= n_envs, multiple of
 * 64) separates SoA rows.
 *   board  : uint32 [width][stride]  bit y of word (x, e) = board[x, y]
 *            (the reference's board[x, y], tetris_env.py:140, one bit-packed
 *            uint32 per board row x of the (width, height) array)
 *   piece  : uint32 [stride]  id | rot<<3 | anchor_x<<5 | anchor_y<<11 | lock<<17
 *            (an alias of stats row ST_STAT_PIECE)
 *            id in shape_names order T,J,L,Z,S,I,O (tetris_env.py:19);
 *            rot = number of rotate_left (rotated(cclk=False)) mod 4
 *   stats  : int32 [ST_NSTAT][stride]
 *   mt     : uint32 [stride][mt_pitch]; words [0, 624) of each row are the
 *            env's MT19937 state (CPython random.getstate()) after st_mt_sync;
 *            the rest is engine-private (the next generation, see st_mt_sync) */
typedef struct st_state_views {
    uint32_t *board;
    uint32_t *piece;
    int32_t *stats;
    uint32_t *mt;
    int64_t n_envs;
    int64_t stride;
    int32_t width, height;
    int64_t mt_pitch; /* words between consecutive envs' rows of mt */
} st_state_views;

/* ---- lifecycle: TetrisEnv.__init__ (tetris_env.py:343-392) ---------------- */
int st_create(st_ctx **out, const st_config *cfg, int device, int64_t n_envs); /* n_envs <= 2^24 */
int st_destroy(st_ctx *ctx);                     /* TetrisEnv.close, :466 */

/* random.seed(seed[e]) for every env (host array of n_envs uint64 seeds).
 * Also initialises counters as TetrisEngine.__init__ does (time = score = -1,
 * :165-166).  Required before the first st_reset. */
int st_seed(st_ctx *ctx, const uint64_t *seeds_host, st_stream stream);

/* TetrisEngine.clear (tetris_env.py:306-315) on every env with d_mask[e] != 0
 * (d_mask == NULL: all envs).  The reference's reset observation is the empty
 * board (clear() returns the board before the piece is drawn), so no
 * observation is produced here. */
int st_reset(st_ctx *ctx, const uint8_t *d_mask, st_stream stream);

/* TetrisEnv.step (tetris_env.py:397-403) / TetrisEngine.step (:243-304) on
 * every env.  d_actions: uint8 [n_envs] in 0..6 (values >= 7 are rejected on
 * the host side by the wrapper; the kernel treats them as idle).
 * Outputs (any may be NULL):
 *   d_obs    : uint32 [width][n_envs]  packed observation (board + current
 *              piece overlay, :301-302), same bit layout as st_state_views.board
 *   d_reward : int32 [n_envs]   (every reference reward is integer-valued)
 *   d_done   : uint8 [n_envs]                                                 */
int st_step(st_ctx *ctx, const uint8_t *d_actions, uint32_t *d_obs, int32_t *d_reward,
            uint8_t *d_done, st_stream stream);

/* Same as st_step but also writes the float32 observation the reference
 * returns (np.array(state, float32), :400): d_obs_f32 float [n_envs][width][height],
 * fused into the step kernel. */
int st_step_f32(st_ctx *ctx, const uint8_t *d_actions, uint32_t *d_obs, float *d_obs_f32,
                int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* k consecutive steps (TetrisEngine.step k times, :243-304), one step
 * kernel launch each, enqueued by one host call: step i takes the actions at
 * device pointer d_actions[i] (d_actions: a HOST array of k device
 * pointers) and writes d_obs / d_obs_f32 (NULL: packed only) / d_reward /
 * d_done, so each holds step k-1's outputs when the stream reaches the end
 * -- st_step / st_step_f32 called k times, without the caller's per-call
 * host overhead between the launches (a native driver loop).  An armed
 * st_gate_actions gates the first of the k steps only.  k <= 0: nothing. */
int st_step_n(st_ctx *ctx, const uint8_t *const *d_actions, int64_t k, uint32_t *d_obs, float *d_obs_f32,
              int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* st_step for a vector env (gym's autoreset convention), one
 * launch.  d_obs_f32 may be NULL (packed only).
 *   d_final_obs (uint32 [width][n_envs], or NULL): when given, an env that
 *     died and was reset inside this step (ST_AUTORESET_SAME_STEP) returns
 *     the RESET observation in d_obs / d_obs_f32 -- the empty board that
 *     clear() returns (tetris_env.py:306-315, :405-411) -- and its terminal
 *     observation (what the reference's step returned, :301-302) is written
 *     to d_final_obs.  Only the columns of such envs are meaningful (the
 *     kernel writes 16-B groups holding one).  NULL: the terminal obs is
 *     returned in d_obs (st_step's convention).  d_final_obs requires d_obs
 *     (ST_EINVAL otherwise).
 *   d_info (int32 [ST_NSTAT][n_envs], or NULL): every counter row after the
 *     step (get_info, :232-241, from one snapshot written by the step
 *     kernel): rows ST_STAT_* as in st_state_views.stats except
 *     ST_STAT_MT_INDEX (not written); the ST_STAT_EP_* rows hold the
 *     finished episode's counters where the env was reset in this step and
 *     0 elsewhere.
 * The headline st_step kernel is a separate instantiation: these outputs
 * cost it nothing. */
int st_step_vec(st_ctx *ctx, const uint8_t *d_actions, uint32_t *d_obs, float *d_obs_f32,
                int32_t *d_reward, uint8_t *d_done, uint32_t *d_final_obs, int32_t *d_info,
                st_stream stream);

/* BASELINE C5's gather format.  st_step_wire is st_step writing, instead of
 * obs / reward / done, one bit stream per env: column x's `height` obs bits
 * (exactly st_step's packed obs word x) at bit x*height, then the reward's
 * 32 bits (two's complement: lossless for every int32 the step computes,
 * host-written counters included) and the done bit -- stored as
 * st_wire_words(width, height) = ceil((width*height + 33) / 32) uint32 rows
 * d_wire [words][n_envs] (10x20: 8 words, 32 B per env, against 48 B for
 * obs + reward + done as width + 2 rows), so a per-step gather of every
 * shard's outputs to rank 0 (tetris_env.py:397-403's return values, for all
 * envs) moves 1.5x fewer bytes over xGMI.  st_unwire turns wire rows back
 * into st_step's outputs (d_obs uint32 [width][n], d_reward int32 [n],
 * d_done uint8 [n]), bit-exact.  st_unwire_shards does the same straight from
 * a gather's receive buffer: d_wire [shards][words][n_cap], shard r's envs at
 * its columns 0 .. count_r - 1, where shard r holds the contiguous global
 * block of distributed.shard_range (counts n_global / shards, the first
 * n_global % shards shards one more; n_cap >= the largest count) -> d_obs
 * [width][n_global], d_reward [n_global], d_done [n_global] in global env
 * order.  st_wire_words returns ST_EINVAL for a board outside 1..32 x 1..28. */
int st_wire_words(int32_t width, int32_t height);
int st_step_wire(st_ctx *ctx, const uint8_t *d_actions, uint32_t *d_wire, st_stream stream);
int st_unwire(int32_t width, int32_t height, int64_t n, const uint32_t *d_wire, uint32_t *d_obs,
              int32_t *d_reward, uint8_t *d_done, st_stream stream);
int st_unwire_shards(int32_t width, int32_t height, int64_t n_global, int32_t shards, int64_t n_cap,
                     const uint32_t *d_wire, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                     st_stream stream);

/* k consecutive st_step calls in ONE launch: the driver loop of README.md:43-51
 * (`for t: obs, r, done, info = env.step(a[t])`) with all actions known up
 * front (synthetic / replayed rollouts).  Boards and counters stay on chip
 * between steps.  d_actions: uint8 [k][n_envs]; outputs per step at [t]
 * (any may be NULL): d_obs uint32 [k][width][n_envs], d_obs_f32 float
 * [k][n_envs][width][height], d_reward int32 [k][n_envs], d_done uint8
 * [k][n_envs].  Results are identical to k calls of st_step / st_step_f32. */
int st_rollout(st_ctx *ctx, int32_t k, const uint8_t *d_actions, uint32_t *d_obs,
               float *d_obs_f32, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Packed obs (uint32 [width][n_envs]) -> float32 [n_envs][width][height]
 * (TetrisEnv._observation 'ram' + the float32 cast, :400 / :421-424). */
int st_obs_to_f32(st_ctx *ctx, const uint32_t *d_obs, float *d_out, st_stream stream);

/* TetrisEngine.render() (tetris_env.py:317-321): board with the current
 * piece overlaid, packed like st_step's d_obs (uint32 [width][n_envs]), for
 * every env, without stepping. */
int st_render(st_ctx *ctx, uint32_t *d_obs, st_stream stream);

/* Grayscale / RGB image of packed observations: convert_grayscale(board, size)
 * (tetris_env.py:76-114) [+ convert_grayscale_rgb, :117-122], evaluated in
 * closed form per pixel.  d_out: [n_envs][size][size][channels]
 * (channels 1 or 3), float32 (as_u8 == 0: TetrisEnv obs, :426-433) or uint8
 * (as_u8 != 0: render('rgb_array'), :458-462).  Values 0 / 128 / 190. */
int st_grayscale(st_ctx *ctx, const uint32_t *d_obs, int32_t size, int32_t channels,
                 int32_t as_u8, void *d_out, st_stream stream);

/* One env's step outputs and state as one record of st_export_words(width,
 * height) uint32 words, for the single-env surface's per-step read-back in
 * ONE transfer (TetrisEnv.step's obs / reward / done and get_info's counters,
 * tetris_env.py:397-403, :232-241, and CPython's random state, :187):
 *   [0, width)              packed obs word x of `env` (from d_obs [width][n_envs])
 *   width                   reward (from d_reward)      width + 1   done (d_done)
 *   width + 2 + r           stats row r, r < ST_NSTAT (ST_STAT_PIECE: the piece word)
 *   M + i, i < 624          (parts & ST_EXPORT_MT) MT word i, M = width + 2 + ST_NSTAT
 *   M + 624 + x*height + y  (parts & ST_EXPORT_OBS_F32) cell (x, y) of the obs
 *                           as float32 0.0 / 1.0: np.array(state, float32), :400
 * Parts not requested are not written.  d_obs / d_reward / d_done may be
 * NULL (zeros written).  The MT words and the ST_STAT_MT_INDEX word are
 * CPython's form (random.getstate(), as st_mt_sync would leave them) without
 * changing the env's state.  d_out: device memory (or host memory the device
 * can write). */
#define ST_EXPORT_MT 1u
#define ST_EXPORT_OBS_F32 2u
int st_export_env(st_ctx *ctx, int64_t env, const uint32_t *d_obs, const int32_t *d_reward,
                  const uint8_t *d_done, uint32_t parts, uint32_t *d_out, st_stream stream);
int st_export_words(int32_t width, int32_t height);

/* st_step (d_obs, d_reward, d_done) followed by st_export_env(env, the same
 * three, parts, d_out), in ONE launch: every env steps (TetrisEngine.step,
 * tetris_env.py:243-304), env's record is written by the workgroup that
 * stepped it.  d_obs, d_reward, d_done and d_out are all required (the
 * record is read back from them; d_out may be mapped pinned host memory, as
 * for st_export_env).  ST_EINVAL for a NULL, env outside [0, n_envs) or
 * parts outside the two flags; ST_ESTATE before st_seed + st_reset; all
 * before any GPU call.  Like st_step_wire it is not gated and does not
 * consume an armed gate; it honours st_set_action_flag as st_step does. */
int st_step_export(st_ctx *ctx, const uint8_t *d_actions, int64_t env, uint32_t parts, uint32_t *d_out,
                   uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Device views of the state (valid until st_destroy). */
int st_state(st_ctx *ctx, st_state_views *out);

/* hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, stream) -- moves state
 * between the views above and caller buffers (crafted states). */
int st_copy(void *dst, const void *src, int64_t bytes, st_stream stream);

/* The step kernels keep each env's MT19937 generation double-buffered (the
 * next generation is computed a few words per draw into a second buffer and
 * becomes current at index 624) and draw every env's next piece ahead of its
 * spawn (the "preview", whose words the reference has not consumed yet: the
 * rollouts draw it right behind a lock, st_step at the start of the step
 * after one, so an env may also hold none between launches), so
 * between steps ST_STAT_MT_INDEX carries engine bits above bit 9 and the
 * current words may sit in the second buffer.  st_mt_sync (on `stream`)
 * brings every env back to CPython's form -- words [0, 624) of its mt row and
 * an index 0..624 equal random.getstate(), the preview's words given back.
 * Call it before reading stats or mt through st_state's views; st_save calls
 * it itself.  Writing a CPython state (words [0, 624), index 0..624) is always
 * valid. */
int st_mt_sync(st_ctx *ctx, st_stream stream);

/* State snapshot: the engine attributes of every env (board, piece, counters,
 * shape counts: TetrisEngine.__init__ / _new_piece, tetris_env.py:138-199)
 * and its MT19937 state (CPython random.getstate(), :187).
 * st_state_bytes: the size of one snapshot of this context.
 * st_save: writes it to host memory (a 64-byte header -- magic "STSNAP\0\1",
 *   snapshot format version (1), width, height, ST_NSTAT, n_envs -- then board uint32
 *   [width][n_envs], stats int32 [ST_NSTAT][n_envs], mt uint32 [n_envs][624]).
 * st_load: restores one into a context with the same width, height and
 *   n_envs (scoring flags and lock delay are configuration, not state, and
 *   may differ).  A loaded context needs no st_seed / st_reset.
 * Both synchronous; ST_EINVAL on a size or header mismatch. */
int64_t st_state_bytes(const st_ctx *ctx);
int st_save(st_ctx *ctx, void *host_out, int64_t bytes);
int st_load(st_ctx *ctx, const void *host_in, int64_t bytes);

/* Greedy placement policy (a benchmark / test workload generator, not part
 * of the reference env; SURVEY 8(d) "clear-heavy variant"): d_actions[e] =
 * the action a greedy player takes in env e's current state -- rotate_left
 * toward, then move toward, then hard-drop onto the placement maximizing
 * 80*lines - 12*holes - 3*height - 2000*(piece above the top) over all
 * (rotation, anchor x) hard-dropped from row 0 (first maximum in rotation,
 * then x order) -- or, with probability explore_permille/1000, the uniform
 * action splitmix64(seed ^ ((t << 32) ^ e)) >> 32 mod 7.  Reads the state
 * enqueued before it on `stream`. */
int st_policy_greedy(st_ctx *ctx, uint64_t seed, int64_t t, uint32_t explore_permille,
                     uint8_t *d_actions, st_stream stream);

/* Afterstates: what every placement of env e's current piece would lead to,
 * the input of afterstate value functions and feature players (Dellacherie /
 * BCTS, CEM over feature weights), evaluated on the device in one launch.
 *
 * Placement slots of a board of width W: slot = rot * (W + 6) + (x + 3), rot
 * 0..3 applications of rotated(cclk=False) (tetris_env.py:22-26, as in the
 * piece word), anchor x in -3..W+2; S = st_after_slots(W) = 4 * (W + 6) slots
 * in st_policy_greedy's (rot, x) order.
 *
 * The afterstate of a slot takes the env's current board and current piece
 * id only (the piece's present rot, anchor and lock counter play no part, nor
 * does lock_delay).  The slot is VALID iff not is_occupied(cells, (x, 0),
 * board) (:29-36; cells above row 0 do not count, so a placement hanging off
 * the board above the top is valid, as in the reference).  The piece is then
 * hard-dropped from row 0 (:54-59), set with _set_piece's clipping (:323-327)
 * and _clear_lines runs (:205-216).  This is the idealised placement
 * st_policy_greedy scores: NOT a promise that a sequence of moves, rotations
 * and gravity steps can bring the live piece there.
 *
 * Feature rows (int32; every row, and the board, of an invalid slot is 0): */
enum st_after_feat {
    ST_AFTER_VALID,      /* 1 / 0 */
    ST_AFTER_Y,          /* anchor row after the drop */
    ST_AFTER_LINES,      /* rows cleared */
    ST_AFTER_HOLES,      /* _count_holes (:218-220) of the board after the clear */
    ST_AFTER_HEIGHT,     /* height - topmost occupied row, 0 if empty (st_policy_greedy's height) */
    ST_AFTER_ROWS,       /* sum(np.any(board, axis=0)): the reference's height (:287, :289) */
    ST_AFTER_ABOVE,      /* 1 if a cell of the piece lay above row 0 (clipped at :326) */
    ST_AFTER_DEAD,       /* np.any(board[:, 0]) after the clear (:277) */
    ST_AFTER_REWARD,     /* the reward TetrisEngine.step returns for the step that locks the
                            piece there (:256-297): under the context's scoring flags, from the
                            env's current holes and piece_height counters, reward_step
                            included, -100 on death */
    ST_AFTER_AGG_HEIGHT, /* sum of column heights h[x] = height - topmost occupied row of column x (0 if empty) */
    ST_AFTER_BUMPINESS,  /* sum |h[x] - h[x + 1]| */
    ST_AFTER_NFEAT
};
/* 4 * (width + 6); ST_EINVAL for a width outside 4..32. */
int st_after_slots(int32_t width);
/* d_feat   : int32 [n_envs][ST_AFTER_NFEAT][S], required.
 * d_boards : uint32 [n_envs][width][S] or NULL; word (e, x, s) is column x of
 *            slot s's afterstate in the bit layout of st_state_views.board,
 *            before any death-step erase (:303).
 * Both have the slot innermost.  Reads the state enqueued before it on
 * `stream` and changes none of it (board, piece, counters, MT); needs no
 * st_mt_sync; is not gated and consumes no gate.  ST_EINVAL for a NULL ctx or
 * d_feat, ST_ESTATE before st_seed + st_reset, both before any GPU call. */
int st_afterstates(st_ctx *ctx, int32_t *d_feat, uint32_t *d_boards, st_stream stream);
/* d_actions[e] (uint8 [n_envs]) = the primitive action that moves env e's live
 * piece toward slot d_slots[e] (int32 [n_envs]): 4 (rotate_left) if its rot
 * differs from the slot's, else 1 / 0 if its anchor x is left / right of the
 * slot's, else 2 (hard drop); a slot outside [0, S) gives 2.  This is
 * st_policy_greedy's rule: afterstates -> score -> argmax ->
 * st_placement_actions -> st_step, repeated, plays the chosen placement out.
 * NULL checks and ST_ESTATE as for st_afterstates. */
int st_placement_actions(st_ctx *ctx, const int32_t *d_slots, uint8_t *d_actions, st_stream stream);

/* Reachability: which placement slots the live piece can really be locked in
 * under the reference's own step, in how many steps, and how to start.
 *
 * Let L = max(lock_delay, 0).  The live piece's state is (rot, x, y, l):
 * rotation, anchor and the lock counter _lock_delay, as in the piece word.
 * One TetrisEngine.step(a) (tetris_env.py:243-304) acts on it, with the board
 * fixed, as follows:
 *  1. the action (:245): left / right / hard_drop / soft_drop / rotate_left /
 *     rotate_right / idle (:39-73), each keeping the old position where
 *     is_occupied (:29-36) refuses the new one;
 *  2. gravity, soft_drop (:247); if it moved the piece and step_reset is on,
 *     l = 0 (:248);
 *  3. if _has_dropped() (:259): l = (l + 1) % (L + 1); if that is 0 the piece
 *     LOCKS at its (rot, x, y), else the step ends in state (rot, x, y, l).
 * The start state need not be collision-free (a spawn onto the stack, a
 * host-written piece): the rules only ever test the destination.
 *
 * Slot s = rot * (W + 6) + (x + 3) of st_afterstates is REACHABLE iff it is
 * valid and some action sequence from the env's present piece state locks the
 * piece at (rot, x, ST_AFTER_Y[s]).
 *   steps[s]: the length of the shortest such sequence, the locking step
 *             counted (so >= 1); 0 where the slot is not reachable.
 *   first[s]: the lowest-numbered action that begins a shortest sequence; 2
 *             where the slot is not reachable (as st_placement_actions gives
 *             for a slot it cannot serve).
 * It follows that after first[s] the target is steps[s] - 1 away, and that
 * locking there leaves exactly that slot's afterstate board and, in that step,
 * its ST_AFTER_REWARD.  Lock positions that are no slot's landing (a tuck under
 * an overhang) are outside the slot set and are not reported here: "Lock
 * positions" below reports, evaluates and routes them.
 *
 * Both calls follow st_afterstates: they read the state enqueued before them
 * on `stream` and change none of it (board, piece, counters, MT, preview), need
 * no st_mt_sync, are not gated and consume no gate; a host-written piece id 7
 * is read as 6.  ST_EINVAL for a NULL ctx or a NULL required pointer and for
 * max(lock_delay, 0) > ST_REACH_MAX_LOCK, ST_ESTATE before st_seed + st_reset,
 * all before any GPU call.  A host-written lock counter above L gives an
 * unspecified result, except that every steps stays >= 0, every first in 0..6
 * and nothing faults. */
#define ST_REACH_MAX_LOCK 3   /* the largest lock_delay the search takes */
/* d_steps int32 [n_envs][S], required; d_first uint8 [n_envs][S] or NULL (then
 * only the distances are searched, which is cheaper).  Slot innermost, like
 * d_feat. */
int st_reachable(st_ctx *ctx, int32_t *d_steps, uint8_t *d_first, st_stream stream);
/* d_actions[e] (uint8 [n_envs], required) = first[d_slots[e]] of env e: 2 for a
 * slot outside [0, S), invalid, or unreachable.  d_steps int32 [n_envs] or
 * NULL: steps[d_slots[e]] (0 likewise).  route_actions -> st_step, repeated,
 * locks the piece in a reachable slot after exactly steps[s] steps, d_steps
 * falling by one a step. */
int st_route_actions(st_ctx *ctx, const int32_t *d_slots, uint8_t *d_actions, int32_t *d_steps, st_stream stream);

/* Linear feature player (Dellacherie / BCTS players, CEM or ES over feature
 * weights): env e scores every placement slot of its current piece with
 * weight row e % n_w and picks one, in one launch.
 * d_weights: float32 [n_w][ST_AFTER_NFEAT] on the device, n_w >= 1 (one row
 * for every env, or one row per candidate of a population).
 *
 * Slots, validity and the eleven feature values of a slot are st_afterstates's,
 * word for word: the same board, the same piece id, the same scoring flags
 * and the same holes / piece_height counters.
 *
 * Score of a slot, in float32, every product and every sum rounded on its own
 * (no fused multiply-add):
 *   acc = 0.0f;
 *   for r = 0 .. ST_AFTER_NFEAT - 1, in enum order: acc = acc + w[r] * (float)feat[r];
 * Every feature is an integer far below 2^24, so its conversion is exact.  Row
 * VALID is 1 on every candidate: its weight is a bias.
 *
 * Choice: the valid slot with the largest score; ties go to the lowest slot
 * number (st_policy_greedy's "first maximum in rotation, then x order").  If
 * no slot is valid: slot -1, score 0.0f, and the d_best column all zero.
 * Weights must be finite; with others the result is unspecified, except that
 * the slot stays in [-1, S) and nothing faults.
 *
 * d_slots   int32 [n_envs] or NULL: the chosen slot.
 * d_actions uint8 [n_envs] or NULL: st_placement_actions's rule for the chosen
 *           slot and the live piece (4, else 1 or 0, else 2); 2 for slot -1.
 * d_scores  float [n_envs] or NULL: the chosen slot's score.
 * d_best    int32 [ST_AFTER_NFEAT][n_envs] or NULL: row r of the chosen slot at
 *           [r][e], the env innermost (what a TD learner on afterstate
 *           features stores).
 * Like st_afterstates it reads the state enqueued before it on `stream` and
 * changes none of it, needs no st_mt_sync, is not gated and consumes no gate.
 * ST_EINVAL for a NULL ctx, NULL d_weights, n_w < 1 or all four outputs NULL;
 * ST_ESTATE before st_seed + st_reset; both before any GPU call. */
int st_policy_linear(st_ctx *ctx, const float *d_weights, int64_t n_w,
                     int32_t *d_slots, uint8_t *d_actions, float *d_scores, int32_t *d_best,
                     st_stream stream);

/* k times (st_policy_linear -> st_step), enqueued by one host call: iteration
 * i writes the policy's actions into a buffer the context owns (allocated on
 * the first call, which also waits for the stream once -- see
 * st_step_placements; freed by st_destroy) and runs the ordinary step on them.
 * d_return   int64 [n_envs] or NULL: += the reward of every one of the k steps.
 * d_episodes int32 [n_envs] or NULL: += the done of every one of the k steps.
 *   Both add to what the caller left in them, so consecutive calls chain
 *   (zero them before the first).
 * d_obs / d_reward / d_done: the LAST step's outputs as st_step writes them
 *   (as with st_step_n), any of them NULL.
 * That buffer (the actions, and the rows of reward / done the sums are taken
 * from) is one per context: calls on the same context must be ordered on one
 * stream, or the later one enqueued only after the earlier has finished; two
 * calls in flight on different streams would overwrite each other's rows.
 * The steps are not gated and an armed st_gate_actions stays armed; the
 * st_set_action_flag word is honoured as in st_step.  k <= 0 does nothing.
 * Works under both autoreset modes: under ST_AUTORESET_SAME_STEP a finished
 * env starts its next episode in the step that ended it (what evaluating a
 * population wants); under ST_AUTORESET_NONE a dead env keeps being stepped
 * in the state the reference leaves behind, exactly as k calls of
 * st_policy_linear + st_step by hand would.
 * ST_EINVAL for a NULL ctx, NULL d_weights or n_w < 1, ST_ESTATE before
 * st_seed + st_reset, both before any GPU call. */
int st_play_linear(st_ctx *ctx, const float *d_weights, int64_t n_w, int64_t k,
                   int64_t *d_return, int32_t *d_episodes,
                   uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Placement step: the game the afterstate literature plays -- one decision is
 * one piece, the action is the placement, the transition is the afterstate
 * plus the next piece -- defined in the reference's own terms only.
 *
 * COMMITTING slot s of env e, s = rot * (W + 6) + (x + 3) as in st_afterstates:
 *  - VALID slot: s in [0, S) and not is_occupied(rotated^rot(shapes[id]),
 *    (x, 0), board) (tetris_env.py:29-36) -- the very validity rule of
 *    st_afterstates, on the env's current board and piece id.  The env's piece
 *    becomes: shape = rot applications of rotated(cclk=False) to the base shape
 *    (:22-26); anchor = (x, 0); _lock_delay = max(lock_delay, 0), so that
 *    _lock_delay_fn (:175) returns 0 on the next drop and the piece locks in
 *    that step whatever lock_delay is.  As a piece word:
 *    id | rot << 3 | x << 5 | 0 << 11 | max(lock_delay, 0) << 17.  Every shape
 *    holds cell (0, 0), so a valid slot has 0 <= x < W and fits the field.
 *  - INVALID slot (occupied at row 0, outside [0, S), e.g. -1): the piece is
 *    left exactly as it is, lock counter included.
 * Nothing else changes: board, counters, MT, preview.
 *
 * A PLACEMENT STEP is a commit followed by TetrisEngine.step(2) (hard_drop,
 * :243-304).  For a valid slot it follows from the reference that the piece
 * locks in this step (time + 1), the reward is that slot's ST_AFTER_REWARD,
 * the board after the step is that slot's st_afterstates board (before the
 * death erase, :303, or the same-step reset), the next piece is drawn, and
 * under ST_AUTORESET_SAME_STEP a death resets inside the step as usual.  For
 * an invalid slot the step is an ordinary hard drop of the live piece (as
 * st_placement_actions gives 2 for a slot outside [0, S) and st_policy_linear
 * for slot -1); with lock_delay > 0 it need not lock.
 *
 * st_place: the commit alone, one launch.  d_slots int32 [n_envs]; d_placed
 * uint8 [n_envs] or NULL: 1 where the slot was valid and committed, else 0.
 * It reads the board and writes the piece row only; a host-written piece id 7
 * is read as 6, as in st_afterstates.  ST_EINVAL for a NULL ctx or d_slots,
 * ST_ESTATE before st_seed + st_reset, both before any GPU call; not gated,
 * consumes no gate, needs no st_mt_sync. */
int st_place(st_ctx *ctx, const int32_t *d_slots, uint8_t *d_placed, st_stream stream);
/* st_place, then the ordinary step (st_step's kernel, unchanged) on a buffer
 * the context owns that holds action 2 for every env (part of st_play_linear's
 * allocation: made and filled on first use, freed by st_destroy): two
 * launches.  The context's FIRST call of st_play_linear, st_step_placements
 * or st_play_linear_placements allocates that buffer, fills it on `stream`
 * and waits for the stream (hipStreamSynchronize): it is not asynchronous
 * and must not be made while the stream is being captured; later calls only
 * enqueue.  d_placed as for st_place; d_obs / d_reward / d_done as st_step
 * writes them, any of them NULL.  The step is not gated and an armed
 * st_gate_actions stays armed; the st_set_action_flag word is honoured.
 * Errors as for st_place. */
int st_step_placements(st_ctx *ctx, const int32_t *d_slots, uint8_t *d_placed,
                       uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);
/* st_play_linear at placement level: k times (st_policy_linear's choice,
 * committed by the same launch -> the step on the constant hard drop), two
 * launches per piece, identical to k rounds of st_policy_linear +
 * st_step_placements(its d_slots) by hand; where no slot is valid (slot -1)
 * nothing is committed and the live piece hard-drops.  d_return, d_episodes,
 * the last step's d_obs / d_reward / d_done, the one-buffer-per-context
 * ordering rule, both autoreset modes, k <= 0 and the errors are
 * st_play_linear's, word for word. */
int st_play_linear_placements(st_ctx *ctx, const float *d_weights, int64_t n_w, int64_t k,
                              int64_t *d_return, int32_t *d_episodes,
                              uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Feature sets: the rows Dellacherie's and the BCTS (Thiery & Scherrer)
 * players are built from, behind the rows of st_after_feat.
 *
 * ST_FEATS_BASE is st_after_feat, ST_AFTER_NFEAT = 11 rows.  ST_FEATS_BCTS has
 * ST_AFTER_NFEAT + ST_AFTER_NEXT = 18 rows: rows 0..10 are st_after_feat's, word
 * for word; row ST_AFTER_NFEAT + v is st_after_ext's value v.
 *
 * B is the slot's afterstate board after _clear_lines and before any death
 * erase -- exactly the board st_afterstates returns in d_boards -- B[x][y] with
 * x in 0..W-1 and y = 0 the top row.  The piece's cells are
 * rotated^rot(shapes[id]) at (x + i, ST_AFTER_Y + j), unclipped.  A HOLE is an
 * empty cell with a filled cell above it in its column (_count_holes,
 * tetris_env.py:218-220).  All rows are int32 and 0 on an invalid slot. */
enum st_feature_set { ST_FEATS_BASE = 0, ST_FEATS_BCTS = 1 };
enum st_after_ext {            /* extended row index = ST_AFTER_NFEAT + value */
    ST_AFTER_EXT_LANDING2,   /* 2 * H - 1 - (ymin + ymax), ymin / ymax the smallest / largest row of the
                                piece's cells (unclipped: ymin may be negative): twice the height of the
                                piece's middle above the floor, a bottom-row cell spanning heights 0..1.
                                Dellacherie's landing height is LANDING2 / 2; doubled, the row is an integer */
    ST_AFTER_EXT_ERODED,     /* LINES * (the piece's cells that _set_piece wrote, i.e. inside the board,
                                and that lay in a row that was then cleared) */
    ST_AFTER_EXT_ROW_TRANS,  /* over all H rows of B, a filled wall left of column 0 and right of column
                                W - 1: the horizontally adjacent pairs that differ.  An empty row counts 2
                                (an empty 10x20 board: 40); the "occupied rows only" convention is this
                                row plus a multiple of ROWS and a constant */
    ST_AFTER_EXT_COL_TRANS,  /* over all W columns, cell (x, H) = the floor filled and nothing above row 0:
                                the pairs (y, y + 1), y in 0..H-1, that differ (an empty 10x20 board: 10) */
    ST_AFTER_EXT_WELLS,      /* a well cell is an empty cell whose left and right neighbours are filled
                                (walls count as filled); the sum over maximal vertical runs of well cells
                                in a column of d (d + 1) / 2, d the run's length.  Covered well cells
                                count like open ones */
    ST_AFTER_EXT_HOLE_DEPTH, /* sum over holes of the number of filled cells above the hole in its column */
    ST_AFTER_EXT_HOLE_ROWS,  /* the rows of B that hold at least one hole */
    ST_AFTER_NEXT
};
/* The number of rows of a feature set: 11 or 18; ST_EINVAL for any other set. */
int st_feature_rows(int32_t set);
/* st_afterstates with the rows of `set`: d_feat int32 [n_envs][rows][S],
 * rows = st_feature_rows(set); d_boards as for st_afterstates (the boards do
 * not depend on the set).  With ST_FEATS_BASE it is st_afterstates: the same
 * kernel, outputs equal bit for bit.  Reads and leaves the state, ordering and
 * gates as st_afterstates does.  ST_EINVAL for a NULL ctx or d_feat or a bad
 * set, ST_ESTATE before st_seed + st_reset, both before any GPU call. */
int st_afterstates_set(st_ctx *ctx, int32_t set, int32_t *d_feat, uint32_t *d_boards, st_stream stream);
/* st_policy_linear over the rows of `set`, with an optional slot mask.
 * d_weights: float32 [n_w][rows].  The score is st_policy_linear's chain over
 * the set's rows in index order, acc = acc + w[r] * (float)feat[r] from 0.0f,
 * every product and every sum rounded on its own; ties go to the lowest slot.
 * d_allowed: int32 [n_envs][S] or NULL.  A slot is a CANDIDATE iff it is valid
 *   and (d_allowed == NULL or d_allowed[e][s] != 0); an invalid slot is never
 *   one, whatever the mask says.  The layout is st_reachable's d_steps, so a
 *   player can be confined to the slots the live piece can really reach.
 * The choice is the candidate with the largest score; no candidate gives slot
 * -1, action 2, score 0.0f and a zero d_best column.
 * d_slots / d_actions / d_scores as for st_policy_linear; d_best int32
 * [rows][n_envs] or NULL.  With ST_FEATS_BASE and a NULL mask it is
 * st_policy_linear: the same kernel.  State, ordering and gates as there.
 * ST_EINVAL for a NULL ctx, NULL d_weights, a bad set, n_w < 1 or all four
 * outputs NULL; ST_ESTATE before st_seed + st_reset; both before any GPU call. */
int st_policy_linear_set(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w,
                         const int32_t *d_allowed, int32_t *d_slots, uint8_t *d_actions,
                         float *d_scores, int32_t *d_best, st_stream stream);
/* st_play_linear (placements == 0) or st_play_linear_placements (placements
 * != 0) with the rows of `set`: d_weights float32 [n_w][rows]; the same
 * loop, the same ring of reward / done rows and the same sums, the same
 * first-call rule (see st_step_placements), d_return / d_episodes / d_obs /
 * d_reward / d_done, k <= 0 and both autoreset modes as there.  It takes no
 * mask: one would be stale after the first step.  ST_EINVAL for a NULL ctx,
 * NULL d_weights, a bad set or n_w < 1, ST_ESTATE before st_seed + st_reset,
 * both before any GPU call. */
int st_play_linear_set(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, int64_t k,
                       int32_t placements, int64_t *d_return, int32_t *d_episodes,
                       uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Next piece.  d_next[e] (uint8 [n_envs]) is the id, in shape_names order
 * (tetris_env.py:19), of the shape _choose_shape() (tetris_env.py:183-191)
 * would return for env e in its present state.  _choose_shape reads
 * shape_counts and the env's MT19937 state and nothing else; shape_counts
 * changes only at a spawn (_new_piece, :193-200) and clear() (:306-315) keeps
 * it, so this is the piece the env's next _new_piece takes, whether that spawn
 * follows a lock or a reset (the reference itself has no preview attribute: it
 * draws only when it spawns).
 * The call changes nothing the reference can see: board, piece and counters
 * stay bit for bit the same, so does the MT19937 state in the form st_mt_sync /
 * st_save / st_export_env give it, and every later step gives the results it
 * would have given without the call.  (Engine-private: an env that holds no
 * drawn piece for its next spawn draws it here and keeps it, as st_step does
 * at its start.)  A host-written CPython state (index 0..624) is a valid input,
 * a draw that runs across index 624 included.
 * Not gated, consumes no gate, needs no st_mt_sync before or after; ordered by
 * `stream` like every other call.  ST_EINVAL for a NULL ctx or d_next,
 * ST_ESTATE before st_seed + st_reset, both before any GPU call. */
int st_next_piece(st_ctx *ctx, uint8_t *d_next, st_stream stream);

/* Two-ply player: st_policy_linear_set with the next piece known.
 * First ply: the slots s1, their validity and their rows f1 are
 *   st_afterstates_set(set)'s for the env's current piece, word for word;
 *   R = st_feature_rows(set).  s1 is a CANDIDATE iff it is valid and
 *   (d_allowed == NULL or d_allowed[e][s1] != 0): st_policy_linear_set's rule
 *   and its int32 [n_envs][S] layout.
 * Second ply: for a candidate s1 with f1[ST_AFTER_DEAD] = 0 let X(s1) be the
 *   state the placement step of s1 leaves (st_step_placements; in the
 *   reference: the piece set to the slot's rotation at (x, 0), then
 *   step(hard_drop), tetris_env.py:243-304): its board is the slot's afterstate
 *   board, its live piece is st_next_piece's, its holes / piece_height counters
 *   are as :283-297 leave them.  f2(s1, s2) and the validity of s2 are what
 *   st_afterstates_set(set) returns in state X(s1), word for word,
 *   ST_AFTER_REWARD included.  The mask does not apply to s2.
 * Scores, float32, every product and every sum rounded on its own:
 *   S1(s1) = st_policy_linear_set's chain over f1 with row e % n_w of
 *     d_weights1 (float [n_w][R]); 0.0f if d_weights1 is NULL.
 *   M2(s1) = the largest chain score over the valid s2 with row e % n_w of
 *     d_weights2 (float [n_w][R], required); ties go to the lowest s2.
 *   score(s1) = S1(s1) + T(s1), one float32 add; T = M2(s1) where a valid s2
 *     exists; T = dead_value where s1 is dead or no s2 is valid, and the slot's
 *     second-ply slot is then -1.
 * Choice: the candidate with the largest score, ties to the lowest s1.  No
 *   candidate: slot -1, second slot -1, action 2, score 0.0f.  Weights and
 *   dead_value must be finite; otherwise the result is unspecified, except
 *   that slots stay in [-1, S) and nothing faults.
 * Outputs, each may be NULL but not all six: d_slots int32 [n_envs]; d_slots2
 *   int32 [n_envs], the best s2 behind the chosen s1; d_actions uint8
 *   [n_envs], st_placement_actions's rule for the chosen s1; d_scores float
 *   [n_envs]; d_scores_all float [n_envs][S] and d_slots2_all int32
 *   [n_envs][S]: score(s1) and its best s2 for every candidate, 0.0f / -1 for
 *   every other slot.
 * State, ordering and gates as for st_next_piece: nothing the reference can see
 * changes.  ST_EINVAL for a NULL ctx, NULL d_weights2, a bad set, n_w < 1, all
 * six outputs NULL or a non-finite dead_value; ST_ESTATE before st_seed +
 * st_reset; both before any GPU call. */
int st_policy_lookahead(st_ctx *ctx, int32_t set, const float *d_weights1, const float *d_weights2,
                        int64_t n_w, float dead_value, const int32_t *d_allowed, int32_t *d_slots,
                        int32_t *d_slots2, uint8_t *d_actions, float *d_scores, float *d_scores_all,
                        int32_t *d_slots2_all, st_stream stream);
/* st_play_linear_placements with st_policy_lookahead's choice: k times
 * (st_policy_lookahead, d_allowed NULL, its chosen s1 committed by the same
 * launch -> the step on the constant hard drop), identical to k rounds of
 * st_policy_lookahead + st_step_placements(d_slots) by hand.  The ring of
 * reward / done rows and the sums, the first-call rule (see
 * st_step_placements), the one-buffer-per-context ordering rule, both
 * autoreset modes, k <= 0 and the last step's d_obs / d_reward / d_done are
 * st_play_linear_placements's.  It takes no mask (st_play_linear_set's reason).
 * ST_EINVAL for a NULL ctx, NULL d_weights2, a bad set, n_w < 1 or a non-finite
 * dead_value, ST_ESTATE before st_seed + st_reset, both before any GPU call. */
int st_play_lookahead(st_ctx *ctx, int32_t set, const float *d_weights1, const float *d_weights2,
                      int64_t n_w, float dead_value, int64_t k, int64_t *d_return, int32_t *d_episodes,
                      uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Next-piece odds.  d_m (int32 [7][n_envs], env innermost) row i is
 * 5 + max_j counts[j] - counts[i] over the ST_STAT_COUNT0 .. +6 rows of the
 * moment: exactly m of _choose_shape (tetris_env.py:186), every value >= 5.
 * _choose_shape picks shape i with probability m[i] / sum(m), and
 * shape_counts changes only at a spawn and is kept by clear() (st_next_piece's
 * argument), so these are the odds of the piece the env's next _new_piece
 * takes, behind a lock or behind a reset -- what an agent may know of it:
 * shape_counts is info['statistics'] of every step.
 * Reads the counter rows only and changes nothing, the engine-private preview
 * included.  Not gated, consumes no gate, needs no st_mt_sync.  ST_EINVAL for a
 * NULL ctx or d_m, ST_ESTATE before st_seed + st_reset, both before any GPU
 * call. */
int st_next_weights(st_ctx *ctx, int32_t *d_m, st_stream stream);

/* Expectimax player: st_policy_lookahead over the odds of the next piece in
 * place of the piece itself -- the two-ply player SimpleTetris-v0 allows (the
 * reference shows no preview; st_next_piece reads the env's MT19937 state).
 * First ply, word for word st_policy_lookahead's: the slots s1, their
 *   validity and rows f1, the CANDIDATE rule and d_allowed, R =
 *   st_feature_rows(set), the weight row e % n_w, S1(s1) (0.0f if d_weights1
 *   is NULL), X(s1) (its board and its holes / piece_height counters), the
 *   unfused float32 chain and ties to the lowest slot.
 * Per-piece tail: for a candidate s1 and every piece q = 0..6 (shape_names
 *   order), T_q(s1) = the largest chain score, with row e % n_w of d_weights2,
 *   over the valid s2 of the rows st_afterstates_set(set) would return in
 *   X(s1) with live piece q, ties to the lowest s2 -- if s1 is not dead and
 *   some s2 is valid for q; otherwise T_q(s1) = dead_value and that piece's
 *   best s2 is -1.
 * Expectation: with m = st_next_weights of env e and M = sum of m[q] (an exact
 *   integer sum), acc = 0.0f; for q = 0..6 in order acc = acc + (float)m[q] *
 *   T_q(s1); E(s1) = acc / (float)M.  Every product, every sum and the one
 *   division are rounded on their own (IEEE round-to-nearest-even; no fused
 *   multiply-add).  The conversions of m and M are exact below 2^24: counts
 *   that make a weight or the sum larger give an unspecified score, never a
 *   fault.
 * Score: score(s1) = S1(s1) + E(s1), one float32 add -- for a dead s1 too,
 *   whose T_q are all dead_value: E is then the chain's value, which need not
 *   be dead_value bit for bit.  Choice: the candidate with the largest score,
 *   ties to the lowest s1.  No candidate: slot -1, action 2, score 0.0f.
 *   Weights and dead_value must be finite (st_policy_lookahead's rule).
 * Outputs, each may be NULL but not all six: d_slots int32 [n_envs]; d_actions
 *   uint8 [n_envs], st_placement_actions's rule for the chosen s1; d_scores
 *   float [n_envs]; d_scores_all float [n_envs][S], score(s1) for candidates,
 *   0.0f elsewhere; d_tails float [n_envs][7][S], T_q(s1) for candidates, 0.0f
 *   elsewhere; d_slots2_all int32 [n_envs][7][S], the best s2 per piece, -1
 *   where there is none or the slot is no candidate.
 * State: reads the board, the piece word and the counter rows; changes
 *   nothing, the engine-private preview and both MT generation buffers
 *   included; unlike st_policy_lookahead it draws no preview and never reads
 *   the MT row: two contexts with the same boards, pieces and counters give
 *   the same outputs whatever their seeds.  One launch.  Not gated, needs no
 *   st_mt_sync.
 * ST_EINVAL for a NULL ctx, NULL d_weights2, a bad set, n_w < 1, all six
 * outputs NULL or a non-finite dead_value; ST_ESTATE before st_seed +
 * st_reset; both before any GPU call. */
int st_policy_expect(st_ctx *ctx, int32_t set, const float *d_weights1, const float *d_weights2,
                     int64_t n_w, float dead_value, const int32_t *d_allowed, int32_t *d_slots,
                     uint8_t *d_actions, float *d_scores, float *d_scores_all, float *d_tails,
                     int32_t *d_slots2_all, st_stream stream);
/* st_play_lookahead with st_policy_expect's choice: k times (st_policy_expect,
 * d_allowed NULL, its chosen s1 committed by the same launch -> the step on
 * the constant hard drop), identical to k rounds of st_policy_expect +
 * st_step_placements(d_slots) by hand.  Everything else -- the ring and the
 * sums, the first-call rule, the one-buffer-per-context rule, both autoreset
 * modes, k <= 0, the outputs and the errors -- is st_play_lookahead's. */
int st_play_expect(st_ctx *ctx, int32_t set, const float *d_weights1, const float *d_weights2,
                   int64_t n_w, float dead_value, int64_t k, int64_t *d_return, int32_t *d_episodes,
                   uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Routes: the whole shortest way of the live piece into a slot, and a player
 * that plans it once a piece and plays it out under the reference's own step.
 *
 * For env e and slot s, in piece state x0 (the present piece word) with the
 * board fixed: a0 = what st_route_actions answers for s in state x0, x1 = the
 * piece state after step(a0) ("Reachability", 1. to 3.), a1 = st_route_actions's
 * answer in x1, and so on -- well defined because after first[s] the target is
 * steps[s] - 1 away.  The ROUTE of a reachable slot is (a0 .. a(n-1)) with
 * n = steps[s]; its last action locks the piece in s.  Equivalently: with D(x)
 * the length of the shortest sequence from x that locks at the slot's landing,
 * a_i is the lowest-numbered action whose successor has D = D(x_i) - 1, for
 * D = 1 the lowest-numbered action that locks there.
 *
 * Encoding: d_route is uint64 [ST_ROUTE_WORDS][n_envs]; action i sits at bits
 * 3 * (i % 21) .. + 2 of word i / 21; bit 63 is 0.  Every field at or past the
 * route's end holds 7, which no step takes as an action, so reading past the
 * end is noticed.  A slot that cannot be served (outside [0, S), invalid or
 * unreachable) gives all fields 7 and steps 0.  A route longer than
 * ST_ROUTE_MAX keeps its first ST_ROUTE_MAX actions and reports its true length
 * in d_steps: the caller plans again when the fields run out.  (No 4..32-wide
 * board is known to produce one.)
 *
 * The three calls read and leave the state as st_reachable does, need no
 * st_mt_sync, and a host-written piece word is read as st_reachable reads it.
 * ST_EINVAL for a NULL ctx, a NULL required pointer, a bad set, n_w < 1 or
 * max(lock_delay, 0) > ST_REACH_MAX_LOCK, ST_ESTATE before st_seed + st_reset,
 * both before any GPU call. */
#define ST_ROUTE_MAX 42   /* actions a packed route holds */
#define ST_ROUTE_WORDS 2  /* its uint64 words: 21 actions each */
/* The route to d_slots[e] (int32 [n_envs]) for every env with d_need[e] != 0
 * (uint8 [n_envs]; NULL: every env); the words of the other envs in d_route /
 * d_steps are left untouched.  d_steps int32 [n_envs] or NULL. */
int st_routes(st_ctx *ctx, const int32_t *d_slots, const uint8_t *d_need, uint64_t *d_route, int32_t *d_steps,
              st_stream stream);
/* For the needed envs: d_slots[e] is what st_policy_linear_set(set, d_weights,
 * n_w, d_allowed = st_reachable's d_steps) chooses, d_scores[e] its score,
 * d_route / d_steps what st_routes gives for that slot -- one launch.  No
 * candidate: slot -1, steps 0, score 0.0f, an all-7 route.  d_slots and d_route
 * are required; d_steps and d_scores may be NULL. */
int st_policy_routed(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, const uint8_t *d_need,
                     int32_t *d_slots, uint64_t *d_route, int32_t *d_steps, float *d_scores, st_stream stream);
/* k primitive steps of the routed player from one host call, identical to
 * this by hand: rem[e] = 0 for every env at the start of the call (plans are
 * local to a call, so a state the host wrote between two calls never meets a
 * stale plan); then k times: the envs with rem == 0 take st_policy_routed's
 * slot and route and rem = min(steps, ST_ROUTE_MAX); a[e] = the env's next
 * route action, or 2 where it has no route (as st_route_actions gives);
 * rem = max(rem - 1, 0); the ordinary st_step on a.  d_return / d_episodes
 * accumulate as in st_play_linear; d_pieces[e] (int32 [n_envs] or NULL) += 1 in
 * every step that issues a route's last action.
 * A call with k = a followed by one with k = b equals one call with k = a + b:
 * planning again in the middle of a route finds the same slot, since the old
 * target stays reachable and keeps its score while the reachable set only
 * shrinks along a shortest route, and the rest of the route is the route from
 * the state reached.
 * The ring of reward / done rows and the sums, the first-call rule (see
 * st_step_placements), the one-buffer-per-context ordering rule, both autoreset
 * modes, k <= 0, the last step's d_obs / d_reward / d_done, not being gated and
 * honouring the st_set_action_flag word are st_play_linear's. */
int st_play_routed(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, int64_t k, int64_t *d_return,
                   int32_t *d_episodes, int32_t *d_pieces, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                   st_stream stream);

/* Lock positions: every place the live piece can be locked at, the tucks under
 * overhangs that are no slot's landing included -- their set, their afterstate
 * rows, the routes into them, a linear player over all of them and its play
 * loop.
 *
 * A LOCK POSITION of env e is a triple (rot, x, y) such that
 *  - some action sequence from the env's present piece state locks the piece at
 *    rotation rot, anchor (x, y), under the three rules of "Reachability"
 *    (action, gravity, lock counter), the board fixed and
 *    L = max(lock_delay, 0) <= ST_REACH_MAX_LOCK, and
 *  - the piece is collision-free there: not is_occupied(cells, (x, y), board)
 *    (tetris_env.py:29-36).
 * A start that collides and locks where it stands (a spawn onto the stack) is
 * therefore no lock position.  A lock position is always grounded (is_occupied
 * at (x, y + 1)) and has 0 <= x < W, 0 <= y < H.  Slot s of st_afterstates is
 * reachable (st_reachable: steps > 0) iff (rot_s, x_s, ST_AFTER_Y[s]) is a lock
 * position.
 *
 * Encoding: pos = slot * 32 + y (int32), slot = rot * (W + 6) + (x + 3) as
 * everywhere; -1: none.  The numeric order of pos is the order of choice:
 * lowest slot, then lowest row.
 *
 * A position is EVALUABLE iff pos decodes to a slot in [0, S) and a row y < H,
 * the piece is collision-free at (x, y) in rot and is occupied at (x, y + 1).
 * Evaluation does not depend on reachability.
 *
 * The five calls read and leave the state as st_reachable does (they read the
 * state enqueued before them on `stream` and change none of it -- st_play_locks
 * steps, as st_play_routed does), need no st_mt_sync, are not gated and consume
 * no gate, and a host-written piece word is read as st_reachable reads it.
 * ST_EINVAL for a NULL ctx, a NULL required pointer, a bad set, n_w < 1, a cap
 * < 1 where a list is passed, or max(lock_delay, 0) > ST_REACH_MAX_LOCK (all
 * five calls); ST_ESTATE before st_seed + st_reset; both before any GPU call. */
#define ST_LOCK_POS(slot, y) ((slot) * 32 + (y))
#define ST_LOCK_SLOT(pos) ((pos) >> 5)
#define ST_LOCK_Y(pos) ((pos) & 31)
/* d_rows uint32 [n_envs][S] or NULL: bit y of word (e, s) is set iff
 * (rot_s, x_s, y) is a lock position.  d_pos int32 [n_envs][cap] or NULL: the
 * env's lock positions in ascending pos order, padded with -1; a list longer
 * than cap is cut to its first cap entries (cap >= 1 with a non-NULL d_pos).
 * d_count int32 [n_envs] or NULL: the true count, cut or not.  Not all three
 * may be NULL.  A start outside the lane grid, which st_reachable answers with
 * "reaches no slot", gives an empty set. */
int st_lock_set(st_ctx *ctx, uint32_t *d_rows, int32_t *d_pos, int64_t cap, int32_t *d_count, st_stream stream);
/* d_pos int32 [n_envs][cap], any order, any values; d_feat int32
 * [n_envs][rows][cap], rows = st_feature_rows(set); d_boards uint32
 * [n_envs][W][cap] or NULL.  For an evaluable position the rows are those of
 * st_afterstates_set with the piece set at (x, y) in place of the hard drop
 * from row 0: ST_AFTER_Y = y, the piece set with _set_piece's clipping, then
 * _clear_lines, ST_AFTER_REWARD from the env's holes and piece_height counters
 * under the context's flags, the seven BCTS rows from the piece's cells at
 * (x + i, y + j); the board is the board after the clear, before any death
 * erase.  Every row and the board of a non-evaluable entry, -1 included, is 0
 * (ST_AFTER_VALID too).  At pos = ST_LOCK_POS(s, ST_AFTER_Y[s]) of a valid
 * slot the rows and board equal st_afterstates_set's for s bit for bit. */
int st_afterstates_at(st_ctx *ctx, int32_t set, const int32_t *d_pos, int64_t cap, int32_t *d_feat,
                      uint32_t *d_boards, st_stream stream);
/* st_routes with the target (rot, x, y) of d_pos[e] in place of a slot's
 * landing: D(x) is the length of the shortest sequence that locks exactly
 * there.  Encoding, ST_ROUTE_MAX, d_need and the all-7 / steps 0 answer for a
 * position that cannot be served (-1, undecodable, or no lock position) are
 * st_routes's. */
int st_routes_at(st_ctx *ctx, const int32_t *d_pos, const uint8_t *d_need, uint64_t *d_route, int32_t *d_steps,
                 st_stream stream);
/* For the needed envs, one launch: the lock set as st_lock_set gives it; every
 * lock position's rows as st_afterstates_at gives them; the unfused float32
 * chain of st_policy_linear_set with weight row e % n_w; d_pos[e] = the lock
 * position with the largest score, ties to the lowest pos; d_route / d_steps
 * what st_routes_at gives for it.  d_pos is required.  d_route may be NULL:
 * the backward search and the walk are then skipped, and d_steps is not
 * written.  d_steps, d_scores (float [n_envs]), d_best (int32 [rows][n_envs],
 * the chosen position's rows) and d_count (int32 [n_envs], the lock count) may
 * be NULL.  No lock position: pos -1, steps 0, score 0.0f, a zero d_best
 * column, an all-7 route.  Envs that are not needed keep their words. */
int st_policy_locks(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, const uint8_t *d_need,
                    int32_t *d_pos, uint64_t *d_route, int32_t *d_steps, float *d_scores, int32_t *d_best,
                    int32_t *d_count, st_stream stream);
/* st_play_routed word for word, with st_policy_locks as the planner: the rem
 * rule, plans local to a call, d_pieces, the ring and the sums, the first-call
 * rule, the one-buffer-per-context rule, both autoreset modes and k <= 0.
 * A call with k = a followed by one with k = b equals one call with k = a + b,
 * by st_play_routed's argument: the lock set only shrinks along a shortest
 * route, the old target stays in it and keeps its score (the board does not
 * move before the lock), ties go to the lowest pos, and the rest of the route
 * is the route from the state reached. */
int st_play_locks(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, int64_t k, int64_t *d_return,
                  int32_t *d_episodes, int32_t *d_pieces, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                  st_stream stream);

/* N-tuple network: a learned, non-linear afterstate value beside the linear
 * rows -- a set of small windows on the board, each window's bit pattern the
 * index into a lookup table (the systematic n-tuple networks of the SZ-Tetris
 * literature, trained by TD on afterstates or by CMA-ES), evaluated on every
 * placement slot in one launch.
 *
 * Network: T tuples, 1 <= T <= ST_NTUPLE_MAX_TUPLES, each six int32
 *   (x, y, w, h, flip, base): a w x h window whose top-left cell is column x,
 *   row y (row 0 is the top, as everywhere here), with 1 <= w, 1 <= h,
 *   w * h <= ST_NTUPLE_MAX_BITS, 0 <= x, x + w <= W, 0 <= y, y + h <= H, flip
 *   in {0, 1}, base >= 0.  table_len = max over t of base_t + 2^(w_t h_t) must
 *   be <= 2^31 - 1.  Bases may overlap: tuples then share weights.
 * Index: on a board B in the layout of st_state_views.board (word c = column c,
 *   bit r = row r), with i' = flip ? w - 1 - i : i,
 *     idx_t(B) = sum over i < w of (((B[x + i'] >> y) & (2^h - 1)) << (i * h)).
 *   A tuple and its mirror image (W - x - w, y, w, h, !flip, base) read mirrored
 *   boards identically.  Only bits below H are read (host-written garbage above
 *   row H - 1 plays no part), and every base_t + idx_t lies in [0, table_len).
 * Value: N(B): acc = 0.0f; for t = 0 .. T - 1 in order acc = acc +
 *   table[base_t + idx_t(B)] -- float32 adds, each rounded on its own, in this
 *   order.
 * Player: st_policy_linear_set with the network behind it.  The slots, their
 *   validity, the rows f and the CANDIDATE rule with d_allowed are
 *   st_policy_linear_set's, word for word.  S1(s) is its chain with weight row
 *   e % n_w; 0.0f if d_weights is NULL (n_w is then ignored).  B(s) is the
 *   slot's afterstate board -- st_afterstates's d_boards: after _clear_lines,
 *   before any death erase.  V(s) = N(B(s)) if f[ST_AFTER_DEAD] == 0, else
 *   dead_value.  score(s) = S1(s) + V(s), one float32 add.  Choice: the
 *   candidate with the largest score, ties to the lowest slot.  No candidate:
 *   slot -1, action 2, score 0.0f, value 0.0f, a zero d_best column and an
 *   all -1 index column.  Weights, dead_value and the table entries that are
 *   read must be finite; otherwise the result is unspecified, except that the
 *   slot stays in [-1, S) and nothing faults.  With the ST_AFTER_REWARD row's
 *   weight 1 and every other weight 0 this is the TD afterstate rule
 *   argmax r + V(s'). */
#define ST_NTUPLE_MAX_TUPLES 4096
#define ST_NTUPLE_MAX_BITS 16
/* Validates tuples_host (int32 [T][6]) against the context's W, H by the rules
 * above -- on failure ST_EINVAL with the offending tuple named in
 * st_last_error, and nothing changes -- and copies the descriptors to device
 * memory the context owns (freed by st_destroy, replaced by a later call).
 * T == 0 removes the network.  Synchronous, like st_seed's upload; needs only
 * st_create. */
int st_ntuple_set(st_ctx *ctx, const int32_t *tuples_host, int32_t T);
/* table_len of the context's network, 0 without one (or for a NULL ctx). */
int64_t st_ntuple_table_len(const st_ctx *ctx);
/* N of m caller boards d_boards uint32 [W][m]; d_boards NULL: the context's
 * own boards, m = n_envs (the argument is ignored), read at pitch `stride`.
 * d_values float [m] or NULL; d_index int32 [T][m] or NULL, base_t + idx_t; not
 * both NULL.  d_table: float [>= table_len].  One lane per board; reads nothing
 * else of the context and changes nothing.  ST_EINVAL for a NULL ctx or
 * d_table, both outputs NULL or m < 0; ST_ESTATE without a network, and with
 * d_boards NULL before st_seed + st_reset; all before any GPU call. */
int st_ntuple_eval(st_ctx *ctx, const float *d_table, const uint32_t *d_boards, int64_t m, float *d_values,
                   int32_t *d_index, st_stream stream);
/* The player above, one launch.  d_slots, d_actions, d_scores and d_best are
 * st_policy_linear_set's.  d_values float [n_envs]: V of the chosen slot.
 * d_index int32 [T][n_envs] (env innermost, like d_best): base_t + idx_t(B(s))
 * of the chosen slot; -1 in every row where no slot was chosen or the chosen
 * slot is dead (no table entry was read for it).  d_values_all float
 * [n_envs][S]: V(s) for every candidate, 0.0f elsewhere.  Each output may be
 * NULL, but not all seven.  Reads and leaves the state as st_policy_linear_set
 * does; not gated, needs no st_mt_sync.
 * Errors, before any GPU call, in this order: ST_EINVAL for a NULL ctx or
 * d_table, a bad set, n_w < 1 with non-NULL d_weights, all outputs NULL or a
 * non-finite dead_value; ST_ESTATE without a network; ST_ESTATE before
 * st_seed + st_reset. */
int st_policy_ntuple(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, const float *d_table,
                     float dead_value, const int32_t *d_allowed, int32_t *d_slots, uint8_t *d_actions,
                     float *d_scores, float *d_values, int32_t *d_best, int32_t *d_index, float *d_values_all,
                     st_stream stream);
/* st_play_lookahead with st_policy_ntuple's choice, at placement level: k times
 * (st_policy_ntuple, d_allowed NULL, its chosen slot committed by the same
 * launch -> the step on the constant hard drop), identical to k rounds of
 * st_policy_ntuple + st_step_placements(d_slots) by hand.  The ring of reward /
 * done rows and the sums, the first-call rule, the one-buffer-per-context
 * ordering rule, both autoreset modes, k <= 0 and the last step's d_obs /
 * d_reward / d_done are st_play_linear_placements's.  Errors as
 * st_policy_ntuple's (no output rule). */
int st_play_ntuple(st_ctx *ctx, int32_t set, const float *d_weights, int64_t n_w, const float *d_table,
                   float dead_value, int64_t k, int64_t *d_return, int32_t *d_episodes, uint32_t *d_obs,
                   int32_t *d_reward, uint8_t *d_done, st_stream stream);

/* Fork: env states copied on the device, between two contexts or inside one --
 * what a rollout player, a beam search or a population restart needs to put one
 * game into many envs and play on from there.
 *
 * For every env e of dst with d_mask[e] != 0 (uint8 [dst.n_envs]; NULL: every
 * env), env e takes the state of env d_index[e] of src (int32 [dst.n_envs];
 * NULL: d_index[e] = e).  An env whose index lies outside [0, src.n_envs) is
 * left exactly as it is: nothing faults and nothing is reported.  The envs of
 * dst that are not written keep every bit, src is only read, and padding envs
 * are neither read nor written.
 *
 * flags == 0, the deep copy: in the reference's terms copy.deepcopy of the
 *   TetrisEngine (tetris_env.py:125-335) together with random.getstate().
 *   Board, piece word, all ST_NSTAT counter rows (the ST_STAT_EP_* rows
 *   included) and the MT19937 state of dst env e are src env d_index[e]'s, in
 *   the form st_mt_sync / st_save / st_export_env give it, and every later call
 *   on dst env e (st_step*, st_rollout, st_next_piece, the policies) gives what
 *   the same call on src env d_index[e] would give.  The engine-private part
 *   travels too: the env's whole MT row -- both generation buffers, so the
 *   next generation's progress and a pending preview with its consumed-word
 *   count stay as they are in src.
 * ST_FORK_KEEP_RNG, the engine without the random state: board, piece word and
 *   every counter row except ST_STAT_MT_INDEX are copied as above (the shape
 *   counts are counter rows); dst env e keeps its own MT19937 state, exactly as
 *   st_mt_sync would show it before the call, so the copies of one game draw
 *   different futures from their own streams.  A preview dst env e held was
 *   drawn under its old shape counts (_choose_shape reads shape_counts,
 *   tetris_env.py:183-191): it is dropped and its words are given back, which
 *   leaves the written envs -- and only them -- in the form st_mt_sync gives.
 *
 * dst and src must have equal width and height and sit on the same device
 * (ST_EINVAL otherwise); lock_delay, the scoring flags and the autoreset mode are
 * configuration, not state, and may differ, as for st_load.  A copied lock
 * counter above dst's max(lock_delay, 0) is a host-written lock counter above L
 * ("Reachability") to the calls that read it.
 * dst == src is allowed.  The result is defined iff no env that is written with
 * the state of a DIFFERENT env is itself the source of another written env (a
 * broadcast of group roots that are not written satisfies this by
 * construction); otherwise the written envs' contents are unspecified, but
 * they stay valid states: every index in range, nothing faults.
 *
 * Asynchronous on `stream`; the caller orders the work of both contexts on it.
 * Not gated, consumes no gate, needs no st_mt_sync before or after, and leaves
 * both contexts' play buffers alone.  ST_EINVAL for a NULL context, an unknown
 * flag bit or mismatched contexts, ST_ESTATE unless both contexts are past
 * st_seed + st_reset (or st_load); all before any GPU call. */
enum st_fork_flags { ST_FORK_KEEP_RNG = 1u << 0 };
int st_fork(st_ctx *dst, st_ctx *src, const int32_t *d_index, const uint8_t *d_mask,
            uint32_t flags, st_stream stream);

/* Synthetic action source used by the benchmark and the parity tests:
 * d_out[e] = splitmix64(seed ^ ((t << 32) ^ (global_offset + e))) % 7. */
int st_gen_actions(uint8_t *d_out, int64_t n, int64_t t, uint64_t seed,
                   int64_t global_offset, st_stream stream);

/* Sticky check for actions outside 0..6 (the reference raises KeyError for
 * them, tetris_env.py:245; st_step treats them as idle) as its own launch,
 * for an action batch not (yet) passed to a step: sets *d_flag = 1 if
 * any of d_actions[0..n) is > 6, never clears it.  d_flag may be host memory
 * mapped for the device, so the caller can poll it without synchronising
 * (the batched surface's validate_actions='async'). */
int st_check_actions(const uint8_t *d_actions, int64_t n, uint32_t *d_flag, st_stream stream);

/* The same check fused into the step kernels: once a flag word is set,
 * every st_step / st_step_f32 / st_rollout on this context sets *d_flag = 1
 * when any of its actions is > 6 (never clears it), from the action loads the
 * step does anyway -- no extra launch, no sync.  d_flag: device memory or host
 * memory mapped for the device (st_host_device_ptr), owned by the caller and
 * valid until it is replaced; NULL turns the check off (the default). */
int st_set_action_flag(st_ctx *ctx, uint32_t *d_flag);

/* The reference's immediate KeyError (tetris_env.py:245: value_action_map
 * [action] fails before TetrisEngine.step changes any state) for actions
 * already on the device, without draining the stream:
 *   st_gate_actions checks d_actions[0..n_envs) on `stream` (one small
 *     launch) and records an event behind it; the NEXT st_step / st_step_f32 /
 *     st_step_vec on this context is gated: if any action was outside 0..6 it
 *     changes no env and writes no output (every env is skipped), else it is
 *     the ordinary step.  Enqueue that step right away.
 *   st_gate_wait then waits for the check only (the event; the gated step is
 *     already queued behind it and runs while the host waits) and returns 1 if
 *     an action was outside 0..6 (the step was skipped: raise KeyError), 0 if
 *     not, < 0 on error (ST_ESTATE without a pending st_gate_actions).
 * Other calls (st_step_wire, st_rollout, st_reset) are not gated and do not
 * consume the gate. */
int st_gate_actions(st_ctx *ctx, const uint8_t *d_actions, st_stream stream);
int st_gate_wait(st_ctx *ctx);

/* Runtime helpers for hosts that bind only this library (the Python package
 * uses them instead of opening the HIP runtime by name, which could load a
 * second runtime copy beside the one the kernels use):
 * st_stream_sync: hipStreamSynchronize(stream);
 * st_host_device_ptr: the device address of pinned, mapped host memory
 * (hipHostGetDevicePointer);
 * st_stream_wait: work enqueued on `waiter` after this call waits (on the
 * device, no host wait) for the work enqueued on `signaller` before it
 * (hipEventRecord + hipStreamWaitEvent; both streams on the current device).
 * The vector env orders its reuse of an output slot behind the consumer
 * streams a caller registered (TetrisVecEnv.record_stream). */
int st_stream_sync(st_stream stream);
int st_host_device_ptr(void *host, void **d_out);
int st_stream_wait(st_stream waiter, st_stream signaller);

/* Diagnostics: when the environment variable ST_STAMPS is set at st_create,
 * st_step runs an instrumented build of the step kernel that records
 * s_memtime at its phase boundaries per wave; this copies the last step's
 * stamps ([n_waves][16] uint64: 10 phase stamps, s_memrealtime at start and
 * end, HW_ID, XCC_ID) to host memory.  Timing study only. */
int st_debug_stamps(st_ctx *ctx, uint64_t *host_out, int64_t max_words);

/* Message for the last failed call on this thread ("" if none). */
const char *st_last_error(void);
int st_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLETETRIS_H */
