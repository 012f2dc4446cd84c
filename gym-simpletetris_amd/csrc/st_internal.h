// Internal declarations shared by the HIP kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simpletetris.h"

namespace st {

constexpr int kWave = 64;      // one env per lane, one wave per workgroup
constexpr int kPad = 4;        // wall columns on each side of the LDS board
constexpr int kMaxW = 32;
constexpr int kMaxH = 28;
constexpr int kMtN = 624;
constexpr int kNtMaxT = 4096;  // simpletetris.h's limit on the tuples of an n-tuple network (st_ntuple_set)
// Per-env MT storage (words): generation buffers A and B, then a 16-word pad
// (see st_kernels.hip, "Double-buffered twist"); 16-B aligned.
constexpr int64_t kMtPitch = 2 * kMtN + 16;
// after the last env: a draw window reads up to 16 words past index 623 of B
constexpr int64_t kMtPadBack = 64;
// diagnostic stamps per workgroup: st_step: logic wave 10 s_memtime phase
// stamps, s_memrealtime at start and end, HW_ID, XCC_ID, draw kind (words
// 0-15); draw wave 12 stamps + s_memrealtime at start and end (words 16-31);
// st_rollout: per-phase cycle totals of the logic / draw / output wave
// (words 0-15 / 16-31 / 32-47)
constexpr int kStampWords = 48;
constexpr int kPieceRow = ST_STAT_PIECE;     // rows 0..14 (counters + piece) move every step
constexpr int kHotRows = ST_STAT_PIECE + 1;
constexpr int kHotQ = (kHotRows * 16 + kWave - 1) / kWave;  // 16-B slots per lane

struct KParams {
    int32_t W, H;
    int32_t lock_mod;   // max(lock_delay, 0) + 1   (tetris_env.py:175)
    uint32_t flags;
    int32_t autoreset;
    uint32_t ablate;    // TIMING DIAGNOSTICS ONLY (env ST_ABLATE at st_create, read only by
                        // -DST_ABLATION=1 builds, tools/ablate.sh); 0 in
                        // every correct run: 1 = no lock path, 2 = no MT draw,
                        // 4 = no twist, 8 = no obs output; st_step: 1024 =
                        // counter rows read from the first workgroup's lines,
                        // 2048 = lock-path counter stores dropped, 4096 = board
                        // stores dropped, 8192 = late counter loads from the
                        // first workgroup's lines, 16384 / 32768 = the logic /
                        // draw wave's part of 2048 only; 65536 / 131072 = the
                        // draw wave's count / MT-word store only; 262144 = the draw
                        // wave's count rows T J L Z not loaded, 524288 = MT windows
                        // read as zeros, 1048576 = no next-generation chunks,
                        // 2097152 = the lock-path counter rows not loaded,
                        // 4194304 = the store phase's LDS transposition skipped
    uint64_t *stamps;   // DIAGNOSTIC build only (env ST_STAMPS at st_create): per-wave
                        // s_memtime at 8 phase boundaries of the step kernel
    int32_t k;          // st_rollout: number of steps
    int64_t n;          // real envs
    int64_t stride;     // padded env count (multiple of 64) = SoA row stride
    // state
    uint32_t *board;    // [W][stride]
    uint32_t *piece;    // [stride]
    int32_t *stats;     // [ST_NSTAT][stride]
    uint32_t *mt;       // [stride][kMtPitch]
    // io
    const uint8_t *actions;  // [n]
    const uint8_t *mask;     // [n] (reset) or null
    const uint64_t *seeds;   // [stride] (seed)
    uint32_t *obs;           // [W][n]
    float *obs_f32;          // [n][W][H]
    int32_t *reward;         // [n]
    uint8_t *done;           // [n]
    uint32_t *act_flag;      // st_set_action_flag: sticky "action outside 0..6" word, or null
    uint32_t *final_obs;     // st_step_vec: [W][n] terminal obs of envs reset in the step, or null
    uint32_t *wire;          // st_step_wire: [st_wire_words(W, H)][n] gather format, or null
    int32_t *info;           // st_step_vec: [ST_NSTAT][n] counters after the step, or null
    int32_t cus;             // compute units of the device (launch_rollout's kernel choice)
    // st_gate_actions: the step skips every env (no state change, no output)
    // when *gate == gate_epoch, i.e. the gate check before it saw an action
    // outside 0..6 (the reference's KeyError before any state change,
    // tetris_env.py:245); null: no gate (every launch but a gated one)
    const uint32_t *gate;
    uint32_t gate_epoch;
};

hipError_t launch_seed(const KParams &p, hipStream_t s);
hipError_t launch_reset(const KParams &p, hipStream_t s);
hipError_t launch_step(const KParams &p, hipStream_t s);
hipError_t launch_step_packed(const KParams &p, hipStream_t s);  // st_step_packed.hip: k_step<.., F32 = false, ..>
// st_step_export: p.obs / p.reward / p.done are the step's outputs and the record's sources
hipError_t launch_step_export(const KParams &p, int64_t env, uint32_t parts, uint32_t *out, hipStream_t s);
hipError_t launch_rollout(const KParams &p, hipStream_t s);
hipError_t launch_obs_f32(const KParams &p, const uint32_t *obs, float *out, hipStream_t s);
hipError_t launch_render(const KParams &p, hipStream_t s);
hipError_t launch_export(const KParams &p, int64_t env, const uint32_t *obs, const int32_t *rew,
                         const uint8_t *done, uint32_t parts, uint32_t *out, hipStream_t s);
hipError_t launch_mt_sync(const KParams &p, hipStream_t s);
hipError_t launch_policy_greedy(const KParams &p, uint64_t seed, int64_t t, uint32_t explore,
                                uint8_t *out, hipStream_t s);
// st_afterstates: feat int32 [n][ST_AFTER_NFEAT][S], boards uint32 [n][W][S] or null (S = 4 * (W + 6))
hipError_t launch_afterstates(const KParams &p, int32_t *feat, uint32_t *boards, hipStream_t s);
hipError_t launch_placement_actions(const KParams &p, const int32_t *slots, uint8_t *out, hipStream_t s);
// st_policy_linear: weights float [n_w][ST_AFTER_NFEAT]; slots int32 [n], actions uint8 [n], scores
// float [n], best int32 [ST_AFTER_NFEAT][n], any null
hipError_t launch_policy_linear(const KParams &p, const float *weights, int64_t n_w, int32_t *slots, uint8_t *actions,
                                float *scores, int32_t *best, hipStream_t s);
// st_place: commits slots int32 [n] (the piece row alone is written); placed uint8 [n] or null
hipError_t launch_place(const KParams &p, const int32_t *slots, uint8_t *placed, hipStream_t s);
// st_play_linear_placements: st_policy_linear's choice, committed like launch_place; no other output
hipError_t launch_policy_linear_commit(const KParams &p, const float *weights, int64_t n_w, hipStream_t s);
// st_afterstates_set, set = ST_FEATS_BCTS (the base set is launch_afterstates): feat int32 [n][18][S]
hipError_t launch_afterstates_set(const KParams &p, int set, int32_t *feat, uint32_t *boards, hipStream_t s);
// st_policy_linear_set / st_play_linear_set: launch_policy_linear (commit: and launch_policy_linear_commit) over the
// rows of `set` -- weights float [n_w][rows], best int32 [rows][n] -- and with allowed int32 [n][S] or null; the base
// set takes no commit here (launch_policy_linear_commit is that)
hipError_t launch_policy_linear_set(const KParams &p, int set, bool commit, const float *weights, int64_t n_w,
                                    const int32_t *allowed, int32_t *slots, uint8_t *actions, float *scores,
                                    int32_t *best, hipStream_t s);
// st_next_piece: next uint8 [n] or null (then only the missing previews are drawn)
hipError_t launch_next_piece(const KParams &p, uint8_t *next, hipStream_t s);
// st_policy_lookahead / st_play_lookahead (commit: the chosen first-ply slot is committed like launch_place):
// launch_next_piece, then the two-ply kernel over the rows of `set` -- weights1 float [n_w][rows] or null, weights2
// float [n_w][rows], allowed int32 [n][S] or null; slots / slots2 int32 [n], actions uint8 [n], scores float [n],
// scores_all float [n][S], slots2_all int32 [n][S], any null
hipError_t launch_policy_lookahead(const KParams &p, int set, bool commit, const float *weights1,
                                   const float *weights2, int64_t n_w, float dead_value, const int32_t *allowed,
                                   int32_t *slots, int32_t *slots2, uint8_t *actions, float *scores,
                                   float *scores_all, int32_t *slots2_all, hipStream_t s);
// st_next_weights: m int32 [7][n], row i = 5 + max(counts) - counts[i] (st_expect.hip)
hipError_t launch_next_weights(const KParams &p, int32_t *m, hipStream_t s);
// st_policy_expect / st_play_expect (commit: the chosen first-ply slot is committed like launch_place): the expectimax
// kernel over the rows of `set`, one launch, the MT row never read -- weights, allowed, slots, actions, scores and
// scores_all as launch_policy_lookahead's; tails float [n][7][S], slots2_all int32 [n][7][S], any output null
hipError_t launch_policy_expect(const KParams &p, int set, bool commit, const float *weights1, const float *weights2,
                                int64_t n_w, float dead_value, const int32_t *allowed, int32_t *slots,
                                uint8_t *actions, float *scores, float *scores_all, float *tails, int32_t *slots2_all,
                                hipStream_t s);
// st_play_linear: adds rows 0 .. rows - 1 of reward int32 [rows][n] / done uint8 [rows][n] to acc_return
// int64 [n] / acc_episodes int32 [n] (either null) and copies the last row to out_reward / out_done (either null)
hipError_t launch_play_sum(const KParams &p, const int32_t *reward, const uint8_t *done, int rows, int64_t *acc_return,
                           int32_t *acc_episodes, int32_t *out_reward, uint8_t *out_done, hipStream_t s);
// st_reachable: steps int32 [n][S]; first uint8 [n][S] or null (then the untagged search)
hipError_t launch_reachable(const KParams &p, int32_t *steps, uint8_t *first, hipStream_t s);
// st_route_actions: slots int32 [n], actions uint8 [n]; steps int32 [n] or null
hipError_t launch_route_actions(const KParams &p, const int32_t *slots, uint8_t *actions, int32_t *steps,
                                hipStream_t s);
// st_routes (set -1: the route to slots_in int32 [n]) / st_policy_routed / st_play_routed (set a feature set: the
// planner -- weights float [n_w][rows], the chosen slot to slots int32 [n], its score to scores float [n] or null).
// route uint64 [ST_ROUTE_WORDS][n]; steps int32 [n] or null.  An env is needed iff rem[e] == 0 (rem int32 [n], then
// set to min(steps, ST_ROUTE_MAX)), or without rem iff need[e] != 0 (need uint8 [n] or null: every env); nothing is
// written for the others
hipError_t launch_routes(const KParams &p, int set, const float *weights, int64_t n_w, const int32_t *slots_in,
                         const uint8_t *need, int32_t *rem, int32_t *slots, uint64_t *route, int32_t *steps,
                         float *scores, hipStream_t s);
// st_play_routed: act uint8 [n] = the next action of each env's route (2 where rem[e] == 0), rem falls by one,
// pieces int32 [n] or null += 1 with a route's last action
hipError_t launch_route_pop(const KParams &p, const uint64_t *route, const int32_t *steps, int32_t *rem, uint8_t *act,
                            int32_t *pieces, hipStream_t s);
// st_lock_set (st_locks.hip): rows uint32 [n][S], pos int32 [n][cap] (ascending, -1 behind the last), count int32 [n],
// any null
hipError_t launch_lock_set(const KParams &p, uint32_t *rows, int32_t *pos, int64_t cap, int32_t *count, hipStream_t s);
// st_afterstates_at: pos int32 [n][cap] -> feat int32 [n][rows of set][cap], boards uint32 [n][W][cap] or null
hipError_t launch_afterstates_at(const KParams &p, int set, const int32_t *pos, int64_t cap, int32_t *feat,
                                 uint32_t *boards, hipStream_t s);
// st_routes_at (set -1: the route to pos_in int32 [n]) / st_policy_locks / st_play_locks (set a feature set: the
// planner over every lock position -- the chosen position to pos int32 [n], its score to scores, its rows to best
// int32 [rows][n], the lock count to count int32 [n], each of the three or null; route null: the choice alone).
// need, rem, route and steps as launch_routes's
hipError_t launch_locks(const KParams &p, int set, const float *weights, int64_t n_w, const int32_t *pos_in,
                        const uint8_t *need, int32_t *rem, int32_t *pos, uint64_t *route, int32_t *steps,
                        float *scores, int32_t *best, int32_t *count, hipStream_t s);
// st_ntuple_eval (st_ntuple.hip): desc int32 [T][6] (validated by st_ntuple_set), table float [table_len], boards
// uint32 [W][pitch] with m boards in use -> values float [m], index int32 [T][m], either null; m <= 0: no launch
hipError_t launch_ntuple_eval(const int32_t *desc, int T, const float *table, const uint32_t *boards, int64_t pitch,
                              int64_t m, float *values, int32_t *index, hipStream_t s);
// st_policy_ntuple / st_play_ntuple (commit: the chosen slot is committed like launch_place): weights float
// [n_w][rows of set] or null, allowed int32 [n][S] or null; slots int32 [n], actions uint8 [n], scores / values float
// [n], best int32 [rows][n], index int32 [T][n], values_all float [n][S], any null
hipError_t launch_policy_ntuple(const KParams &p, int set, bool commit, const float *weights, int64_t n_w,
                                const int32_t *desc, int T, const float *table, float dead_value,
                                const int32_t *allowed, int32_t *slots, uint8_t *actions, float *scores, float *values,
                                int32_t *best, int32_t *index, float *values_all, hipStream_t s);
// st_fork: dst env e takes the state of src env index[e] (index int32 [dst.n] or null: e) where mask[e] != 0 (mask
// uint8 [dst.n] or null: every env) and the index lies in [0, src.n); keep_rng: the MT19937 state stays dst's own.
// waves: the deep copy's waves per 64 envs, 1 or 4
hipError_t launch_fork(const KParams &dst, const KParams &src, const int32_t *index, const uint8_t *mask, bool keep_rng,
                       int waves, hipStream_t s);
hipError_t launch_grayscale(const KParams &p, const uint32_t *obs, int size, int channels,
                            int as_u8, void *out, hipStream_t s);
hipError_t launch_unwire(int W, int H, int64_t n_global, int shards, int64_t n_cap, const uint32_t *wire,
                         uint32_t *obs, int32_t *reward, uint8_t *done, hipStream_t s);
hipError_t launch_check_actions(const uint8_t *a, int64_t n, uint32_t *flag, hipStream_t s);
hipError_t launch_gate_actions(const uint8_t *a, int64_t n, uint32_t *words, uint32_t *host, uint32_t epoch,
                               hipStream_t s);
hipError_t launch_gen_actions(uint8_t *out, int64_t n, int64_t t, uint64_t seed, int64_t off,
                              hipStream_t s);

}  // namespace st
