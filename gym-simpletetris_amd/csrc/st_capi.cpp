// st_capi.cpp -- extern "C" boundary of the batched SimpleTetris engine.
// Declared in include/simpletetris.h; each entry point cites the reference
// method it replaces there.  Owns the device state; launches the kernels of
// st_kernels.hip on the caller's stream.
#include <algorithm>
#include <cmath>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "st_internal.h"

struct st_ctx {
    st_config cfg;
    uint32_t ablate;
    uint64_t *stamps;
    int device;
    int64_t n;
    int64_t stride;
    bool seeded;
    bool reset_once;
    uint32_t *board;
    uint32_t *piece;
    int32_t *stats;
    uint32_t *mt;
    uint32_t *act_flag;  // st_set_action_flag (caller-owned), or null
    int cus;             // compute units of the device
    // st_gate_actions / st_gate_wait: the gate word (device), its host copy
    // (pinned, mapped), the event recorded behind the gate kernel, the last
    // epoch, and whether the next step launch is gated / a wait is pending
    uint32_t *gate;
    uint32_t *gate_host;
    uint32_t *gate_host_dev;
    hipEvent_t gate_ev;
    uint32_t gate_epoch;
    bool gate_armed;
    bool gate_pending;
    // st_play_linear / st_step_placements / st_play_linear_placements: one
    // allocation made on first use (play_parts) -- a ring of reward rows int32
    // [R][n], the policy's actions uint8 [n], a ring of done rows uint8 [R][n],
    // the constant action 2 (hard drop) uint8 [n], filled then; behind them
    // (8-byte aligned) st_play_routed's / st_play_locks's plans: route uint64
    // [ST_ROUTE_WORDS][n], slot (st_play_locks: lock position), steps and rem
    // int32 [n]
    int32_t *play_buf;
    // st_ntuple_set: the network's descriptors int32 [nt_T][6] (device), its tuple count (0: no network) and
    // table length
    int32_t *nt_desc;
    int32_t nt_T;
    int64_t nt_len;
};

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(ST_EHIP, "%s: %s", what, hipGetErrorString(e));
}

#define ST_HIP(call)                                   \
    do {                                               \
        hipError_t _e = (call);                        \
        if (_e != hipSuccess) return hip_fail(_e, #call); \
    } while (0)

// Make the context's device current for the duration of a call.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

st::KParams params(const st_ctx *c) {
    st::KParams p{};
    p.W = c->cfg.width;
    p.H = c->cfg.height;
    p.lock_mod = (c->cfg.lock_delay > 0 ? c->cfg.lock_delay : 0) + 1;
    p.flags = c->cfg.flags;
    p.autoreset = c->cfg.autoreset;
    p.ablate = c->ablate;
    p.stamps = c->stamps;
    p.n = c->n;
    p.stride = c->stride;
    p.board = c->board;
    p.piece = c->piece;
    p.stats = c->stats;
    p.mt = c->mt;
    p.act_flag = c->act_flag;
    p.cus = c->cus;
    return p;
}

void free_state(st_ctx *c) {
    if (c->board) (void)hipFree(c->board);
    if (c->stats) (void)hipFree(c->stats);
    if (c->mt) (void)hipFree(c->mt);
    if (c->stamps) (void)hipFree(c->stamps);
    if (c->gate) (void)hipFree(c->gate);
    if (c->gate_host) (void)hipHostFree(c->gate_host);
    if (c->gate_ev) (void)hipEventDestroy(c->gate_ev);
    if (c->play_buf) (void)hipFree(c->play_buf);
    c->play_buf = nullptr;
    if (c->nt_desc) (void)hipFree(c->nt_desc);
    c->nt_desc = nullptr;
    c->nt_T = 0;
    c->nt_len = 0;
    c->gate = c->gate_host = c->gate_host_dev = nullptr;
    c->gate_ev = nullptr;
    c->stamps = nullptr;
    c->board = c->piece = c->mt = nullptr;
    c->stats = nullptr;
}

// The parts of the context's play buffer, allocated (and its constant row
// filled, on `s`, waited for) on first use; freed by free_state.
struct PlayParts {
    int64_t R;           // ring rows: one step's reward + done each, as many as fit 20 MiB, at most 32, at least one
    int32_t *ring_rew;   // int32 [R][n]
    uint8_t *act;        // uint8 [n]
    uint8_t *ring_done;  // uint8 [R][n]
    uint8_t *twos;       // uint8 [n], every byte 2
    uint64_t *plan_route;  // st_play_routed: uint64 [ST_ROUTE_WORDS][n]
    int32_t *plan_slot;    // int32 [n]
    int32_t *plan_steps;   // int32 [n]
    int32_t *plan_rem;     // int32 [n]: actions left of the env's plan
};

int play_parts(st_ctx *c, const char *fn, hipStream_t s, PlayParts *out) {
    const int64_t n = c->n;
    const int64_t R = std::max<int64_t>(1, std::min<int64_t>(32, (int64_t(4) << 20) / n));
    PlayParts q;
    q.R = R;
    const size_t plan_off = ((size_t)n * (size_t)(R * (sizeof(int32_t) + 1) + 2) + 7) & ~(size_t)7;
    if (!c->play_buf) {
        int32_t *buf = nullptr;
        const size_t plan_bytes = (size_t)n * (ST_ROUTE_WORDS * sizeof(uint64_t) + 3 * sizeof(int32_t));
        hipError_t e = hipMalloc(&buf, plan_off + plan_bytes);
        if (e != hipSuccess) return fail(ST_ENOMEM, "%s: hipMalloc failed: %s", fn, hipGetErrorString(e));
        uint8_t *twos = reinterpret_cast<uint8_t *>(buf + R * n) + n + R * n;
        e = hipMemsetAsync(twos, 2, (size_t)n, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            return fail(ST_EHIP, "%s: filling the hard-drop actions: %s", fn, hipGetErrorString(e));
        }
        c->play_buf = buf;
    }
    q.ring_rew = c->play_buf;
    q.act = reinterpret_cast<uint8_t *>(q.ring_rew + R * n);
    q.ring_done = q.act + n;
    q.twos = q.ring_done + R * n;
    q.plan_route = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(c->play_buf) + plan_off);
    q.plan_slot = reinterpret_cast<int32_t *>(q.plan_route + ST_ROUTE_WORDS * n);
    q.plan_steps = q.plan_slot + n;
    q.plan_rem = q.plan_steps + n;
    *out = q;
    return ST_OK;
}

}  // namespace

extern "C" {

const char *st_last_error(void) { return g_err; }
int st_abi_version(void) { return ST_ABI_VERSION; }

int st_create(st_ctx **out, const st_config *cfg, int device, int64_t n_envs) {
    g_err[0] = 0;
    if (!out || !cfg) return fail(ST_EINVAL, "st_create: null argument");
    *out = nullptr;
    if (cfg->width < 4 || cfg->width > st::kMaxW)
        return fail(ST_EINVAL, "width %d outside [4, %d]", cfg->width, st::kMaxW);
    if (cfg->height < 4 || cfg->height > st::kMaxH)
        return fail(ST_EINVAL, "height %d outside [4, %d]", cfg->height, st::kMaxH);
    if (cfg->lock_delay > 32766) return fail(ST_EINVAL, "lock_delay %d > 32766", cfg->lock_delay);
    if (cfg->flags & ~0xFFu) return fail(ST_EINVAL, "unknown flag bits 0x%x", cfg->flags);
    if (cfg->autoreset != ST_AUTORESET_NONE && cfg->autoreset != ST_AUTORESET_SAME_STEP)
        return fail(ST_EINVAL, "autoreset %d unknown", cfg->autoreset);
    if (n_envs < 1 || n_envs > (int64_t(1) << 24))  // 32-bit element offsets in the kernels
        return fail(ST_EINVAL, "n_envs %lld outside [1, 2^24] per context", (long long)n_envs);
    int ndev = 0;
    ST_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ST_EINVAL, "device %d of %d", device, ndev);
    DeviceGuard g(device);
    if (!g.ok) return fail(ST_EHIP, "hipSetDevice(%d) failed", device);

    st_ctx *c = new st_ctx();
    c->cfg = *cfg;
    c->device = device;
    if (const char *ab = getenv("ST_ABLATE")) c->ablate = (uint32_t)strtoul(ab, nullptr, 0);
    c->n = n_envs;
    if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) c->cus = 0;
    c->stride = (n_envs + st::kWave - 1) / st::kWave * st::kWave;
    const size_t sd = (size_t)c->stride;
    hipError_t e = hipSuccess;
    // board rows padded to a multiple of 4: a wave's 16-B accesses cover 4 rows
    const size_t wpad = (size_t)((cfg->width + 3) & ~3);
    if (e == hipSuccess) e = hipMalloc(&c->board, sd * wpad * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&c->stats, sd * ST_NSTAT * sizeof(int32_t));
    if (e == hipSuccess) c->piece = reinterpret_cast<uint32_t *>(c->stats) + ST_STAT_PIECE * sd;
    // MT states: [stride][kMtPitch] (+ the back pad a draw window may reach)
    if (e == hipSuccess) e = hipMalloc(&c->mt, (sd * st::kMtPitch + st::kMtPadBack) * sizeof(uint32_t));
    // diagnostic phase stamps (ST_STAMPS set: the instrumented step kernel)
    if (e == hipSuccess && getenv("ST_STAMPS"))
        e = hipMalloc(&c->stamps, (sd / st::kWave) * st::kStampWords * sizeof(uint64_t));
    if (e != hipSuccess) {
        free_state(c);
        delete c;
        return fail(ST_ENOMEM, "st_create: hipMalloc failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return ST_OK;
}

int st_destroy(st_ctx *c) {
    if (!c) return ST_OK;
    DeviceGuard g(c->device);
    (void)hipDeviceSynchronize();
    free_state(c);
    delete c;
    return ST_OK;
}

int st_seed(st_ctx *c, const uint64_t *seeds_host, st_stream stream) {
    if (!c || !seeds_host) return fail(ST_EINVAL, "st_seed: null argument");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    // padding envs get seeds too (they run, unreported, in the last wave)
    uint64_t *d_seeds = nullptr;
    ST_HIP(hipMalloc(&d_seeds, (size_t)c->stride * sizeof(uint64_t)));
    hipError_t e = hipMemcpyAsync(d_seeds, seeds_host, (size_t)c->n * sizeof(uint64_t),
                                  hipMemcpyHostToDevice, s);
    if (e == hipSuccess && c->stride > c->n)
        e = hipMemsetAsync(d_seeds + c->n, 0, (size_t)(c->stride - c->n) * sizeof(uint64_t), s);
    st::KParams p = params(c);
    p.seeds = d_seeds;
    if (e == hipSuccess) e = st::launch_seed(p, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_seeds);
    if (e != hipSuccess) return hip_fail(e, "st_seed");
    c->seeded = true;
    return ST_OK;
}

int st_reset(st_ctx *c, const uint8_t *d_mask, st_stream stream) {
    if (!c) return fail(ST_EINVAL, "st_reset: null context");
    if (!c->seeded) return fail(ST_ESTATE, "st_reset before st_seed");
    DeviceGuard g(c->device);
    st::KParams p = params(c);
    p.mask = d_mask;
    ST_HIP(st::launch_reset(p, (hipStream_t)stream));
    if (!d_mask) c->reset_once = true;
    return ST_OK;
}

static int step_impl(st_ctx *c, const uint8_t *d_actions, uint32_t *d_obs, float *d_obs_f32,
                     int32_t *d_reward, uint8_t *d_done, st_stream stream, uint32_t *d_final_obs = nullptr,
                     int32_t *d_info = nullptr, bool gated = true) {
    if (!c || !d_actions) return fail(ST_EINVAL, "st_step: null argument");
    if (!c->seeded || !c->reset_once)
        return fail(ST_ESTATE, "st_step before st_seed + st_reset (tetris_env.py:244 needs an anchor)");
    DeviceGuard g(c->device);
    st::KParams p = params(c);
    p.actions = d_actions;
    p.obs = d_obs;
    p.obs_f32 = d_obs_f32;
    p.reward = d_reward;
    p.done = d_done;
    p.final_obs = d_final_obs;
    p.info = d_info;
    // st_gate_actions ran for this step: skip it all if it saw a bad action
    // (gated false: st_play_linear's steps, whose actions are not the gate's -- it stays armed)
    if (gated && c->gate_armed) {
        p.gate = c->gate;
        p.gate_epoch = c->gate_epoch;
        c->gate_armed = false;
    }
    ST_HIP(st::launch_step(p, (hipStream_t)stream));
    return ST_OK;
}

int st_step(st_ctx *c, const uint8_t *d_actions, uint32_t *d_obs, int32_t *d_reward,
            uint8_t *d_done, st_stream stream) {
    return step_impl(c, d_actions, d_obs, nullptr, d_reward, d_done, stream);
}

int st_step_f32(st_ctx *c, const uint8_t *d_actions, uint32_t *d_obs, float *d_obs_f32,
                int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    if (!d_obs_f32) return fail(ST_EINVAL, "st_step_f32: null d_obs_f32");
    return step_impl(c, d_actions, d_obs, d_obs_f32, d_reward, d_done, stream);
}

int st_step_n(st_ctx *c, const uint8_t *const *d_actions, int64_t k, uint32_t *d_obs, float *d_obs_f32,
              int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    if (!c) return fail(ST_EINVAL, "st_step_n: null context");
    if (k <= 0) return ST_OK;
    if (!d_actions) return fail(ST_EINVAL, "st_step_n: null action pointer array");
    for (int64_t i = 0; i < k; ++i)
        if (!d_actions[i]) return fail(ST_EINVAL, "st_step_n: null action pointer");
    // one device switch for the whole loop (step_impl's own guard then finds
    // the device current and sets nothing)
    DeviceGuard g(c->device);
    for (int64_t i = 0; i < k; ++i) {
        const int rc = step_impl(c, d_actions[i], d_obs, d_obs_f32, d_reward, d_done, stream);
        if (rc != ST_OK) return rc;
    }
    return ST_OK;
}

int st_step_vec(st_ctx *c, const uint8_t *d_actions, uint32_t *d_obs, float *d_obs_f32, int32_t *d_reward,
                uint8_t *d_done, uint32_t *d_final_obs, int32_t *d_info, st_stream stream) {
    // final_obs is part of the obs output: without d_obs the kernel's two store
    // paths would disagree on whether it is written
    if (d_final_obs && !d_obs) return fail(ST_EINVAL, "st_step_vec: d_final_obs needs d_obs");
    return step_impl(c, d_actions, d_obs, d_obs_f32, d_reward, d_done, stream, d_final_obs, d_info);
}

int st_wire_words(int32_t width, int32_t height) {
    if (width < 1 || height < 1 || width > st::kMaxW || height > st::kMaxH)
        return fail(ST_EINVAL, "st_wire_words: board %dx%d outside 1..%d x 1..%d", width, height, st::kMaxW,
                    st::kMaxH);
    return (width * height + 33 + 31) / 32;
}

int st_step_wire(st_ctx *c, const uint8_t *d_actions, uint32_t *d_wire, st_stream stream) {
    if (!c || !d_actions || !d_wire) return fail(ST_EINVAL, "st_step_wire: null argument");
    if (!c->seeded || !c->reset_once)
        return fail(ST_ESTATE, "st_step_wire before st_seed + st_reset (tetris_env.py:244 needs an anchor)");
    DeviceGuard g(c->device);
    st::KParams p = params(c);
    p.actions = d_actions;
    p.wire = d_wire;
    ST_HIP(st::launch_step(p, (hipStream_t)stream));
    return ST_OK;
}

int st_unwire(int32_t width, int32_t height, int64_t n, const uint32_t *d_wire, uint32_t *d_obs,
              int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    if (st_wire_words(width, height) < 0) return ST_EINVAL;
    if (n < 0) return fail(ST_EINVAL, "st_unwire: negative size");
    if (n > 0 && (!d_wire || !d_obs || !d_reward || !d_done)) return fail(ST_EINVAL, "st_unwire: null argument");
    ST_HIP(st::launch_unwire(width, height, n, 1, n, d_wire, d_obs, d_reward, d_done, (hipStream_t)stream));
    return ST_OK;
}

int st_unwire_shards(int32_t width, int32_t height, int64_t n_global, int32_t shards, int64_t n_cap,
                     const uint32_t *d_wire, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    if (st_wire_words(width, height) < 0) return ST_EINVAL;
    if (n_global < 0 || shards < 1) return fail(ST_EINVAL, "st_unwire_shards: n_global < 0 or shards < 1");
    if (n_cap < (n_global + shards - 1) / shards)
        return fail(ST_EINVAL, "st_unwire_shards: n_cap %lld below the largest shard (%lld)", (long long)n_cap,
                    (long long)((n_global + shards - 1) / shards));
    if (n_global > 0 && (!d_wire || !d_obs || !d_reward || !d_done))
        return fail(ST_EINVAL, "st_unwire_shards: null argument");
    ST_HIP(st::launch_unwire(width, height, n_global, shards, n_cap, d_wire, d_obs, d_reward, d_done,
                             (hipStream_t)stream));
    return ST_OK;
}

int st_rollout(st_ctx *c, int32_t k, const uint8_t *d_actions, uint32_t *d_obs, float *d_obs_f32,
               int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    if (!c || !d_actions) return fail(ST_EINVAL, "st_rollout: null argument");
    if (k < 1) return fail(ST_EINVAL, "st_rollout: k = %d < 1", k);
    if (!c->seeded || !c->reset_once)
        return fail(ST_ESTATE, "st_rollout before st_seed + st_reset (tetris_env.py:244 needs an anchor)");
    DeviceGuard g(c->device);
    st::KParams p = params(c);
    p.k = k;
    p.actions = d_actions;
    p.obs = d_obs;
    p.obs_f32 = d_obs_f32;
    p.reward = d_reward;
    p.done = d_done;
    ST_HIP(st::launch_rollout(p, (hipStream_t)stream));
    return ST_OK;
}

int st_mt_sync(st_ctx *c, st_stream stream) {
    if (!c) return fail(ST_EINVAL, "st_mt_sync: null context");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_mt_sync(params(c), (hipStream_t)stream));
    return ST_OK;
}

int st_obs_to_f32(st_ctx *c, const uint32_t *d_obs, float *d_out, st_stream stream) {
    if (!c || !d_obs || !d_out) return fail(ST_EINVAL, "st_obs_to_f32: null argument");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_obs_f32(params(c), d_obs, d_out, (hipStream_t)stream));
    return ST_OK;
}

int st_render(st_ctx *c, uint32_t *d_obs, st_stream stream) {
    if (!c || !d_obs) return fail(ST_EINVAL, "st_render: null argument");
    if (!c->seeded) return fail(ST_ESTATE, "st_render before st_seed");
    DeviceGuard g(c->device);
    st::KParams p = params(c);
    p.obs = d_obs;
    ST_HIP(st::launch_render(p, (hipStream_t)stream));
    return ST_OK;
}

int st_export_env(st_ctx *c, int64_t env, const uint32_t *d_obs, const int32_t *d_reward,
                  const uint8_t *d_done, uint32_t parts, uint32_t *d_out, st_stream stream) {
    if (!c || !d_out) return fail(ST_EINVAL, "st_export_env: null argument");
    if (env < 0 || env >= c->n) return fail(ST_EINVAL, "st_export_env: env %lld of %lld", (long long)env,
                                            (long long)c->n);
    if (parts & ~(ST_EXPORT_MT | ST_EXPORT_OBS_F32)) return fail(ST_EINVAL, "st_export_env: parts 0x%x", parts);
    if (!c->seeded) return fail(ST_ESTATE, "st_export_env before st_seed");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_export(params(c), env, d_obs, d_reward, d_done, parts, d_out, (hipStream_t)stream));
    return ST_OK;
}

int st_step_export(st_ctx *c, const uint8_t *d_actions, int64_t env, uint32_t parts, uint32_t *d_out,
                   uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    if (!c || !d_actions || !d_out || !d_obs || !d_reward || !d_done)
        return fail(ST_EINVAL, "st_step_export: null argument");
    if (env < 0 || env >= c->n) return fail(ST_EINVAL, "st_step_export: env %lld of %lld", (long long)env,
                                            (long long)c->n);
    if (parts & ~(ST_EXPORT_MT | ST_EXPORT_OBS_F32)) return fail(ST_EINVAL, "st_step_export: parts 0x%x", parts);
    if (!c->seeded || !c->reset_once)
        return fail(ST_ESTATE, "st_step_export before st_seed + st_reset (tetris_env.py:244 needs an anchor)");
    DeviceGuard g(c->device);
    st::KParams p = params(c);  // (not gated: an armed st_gate_actions stays armed)
    p.actions = d_actions;
    p.obs = d_obs;
    p.reward = d_reward;
    p.done = d_done;
    ST_HIP(st::launch_step_export(p, env, parts, d_out, (hipStream_t)stream));
    return ST_OK;
}

int st_export_words(int32_t width, int32_t height) {
    return width + 2 + ST_NSTAT + st::kMtN + width * height;
}

int st_grayscale(st_ctx *c, const uint32_t *d_obs, int32_t size, int32_t channels, int32_t as_u8,
                 void *d_out, st_stream stream) {
    if (!c || !d_obs || !d_out) return fail(ST_EINVAL, "st_grayscale: null argument");
    if (channels != 1 && channels != 3) return fail(ST_EINVAL, "channels %d not 1 or 3", channels);
    const int lim = c->cfg.width > c->cfg.height ? c->cfg.width : c->cfg.height;
    const int gap = size / 100 + 1;
    if (size < 8 || size > 4096 || (size - 2 * gap) / lim - gap < 1)
        return fail(ST_EINVAL, "st_grayscale: size %d too small for a %dx%d board", size,
                    c->cfg.width, c->cfg.height);
    DeviceGuard g(c->device);
    ST_HIP(st::launch_grayscale(params(c), d_obs, size, channels, as_u8, d_out, (hipStream_t)stream));
    return ST_OK;
}

int st_copy(void *dst, const void *src, int64_t bytes, st_stream stream) {
    if (bytes < 0 || ((!dst || !src) && bytes)) return fail(ST_EINVAL, "st_copy: bad argument");
    if (!bytes) return ST_OK;
    ST_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDefault, (hipStream_t)stream));
    return ST_OK;
}

int st_state(st_ctx *c, st_state_views *out) {
    if (!c || !out) return fail(ST_EINVAL, "st_state: null argument");
    out->board = c->board;
    out->piece = c->piece;
    out->stats = c->stats;
    out->mt = c->mt;
    out->mt_pitch = st::kMtPitch;
    out->n_envs = c->n;
    out->stride = c->stride;
    out->width = c->cfg.width;
    out->height = c->cfg.height;
    return ST_OK;
}

namespace {
struct SnapHeader {  // st_save / st_load, 64 bytes
    char magic[8];
    uint32_t abi;  // the snapshot format version (kSnapVersion)
    int32_t width, height, nstat;
    int64_t n;
    uint8_t pad[32];
};
static_assert(sizeof(SnapHeader) == 64, "snapshot header");
const char kSnapMagic[8] = {'S', 'T', 'S', 'N', 'A', 'P', 0, 1};
// the snapshot format's own version (written where ABI 1 wrote its ABI
// version, 1): independent of ST_ABI_VERSION, which changes with the calls
constexpr uint32_t kSnapVersion = 1;

int64_t snap_bytes(const st_ctx *c) {
    return (int64_t)sizeof(SnapHeader) +
           c->n * 4 * ((int64_t)c->cfg.width + ST_NSTAT + st::kMtN);
}
}  // namespace

int64_t st_state_bytes(const st_ctx *c) { return c ? snap_bytes(c) : -1; }

int st_save(st_ctx *c, void *host_out, int64_t bytes) {
    if (!c || !host_out) return fail(ST_EINVAL, "st_save: null argument");
    if (bytes != snap_bytes(c))
        return fail(ST_EINVAL, "st_save: buffer is %lld bytes, a snapshot is %lld", (long long)bytes,
                    (long long)snap_bytes(c));
    DeviceGuard g(c->device);
    SnapHeader h{};
    memcpy(h.magic, kSnapMagic, sizeof(h.magic));
    h.abi = kSnapVersion;
    h.width = c->cfg.width;
    h.height = c->cfg.height;
    h.nstat = ST_NSTAT;
    h.n = c->n;
    char *o = static_cast<char *>(host_out);
    memcpy(o, &h, sizeof(h));
    o += sizeof(h);
    const size_t row = (size_t)c->n * 4, pitch = (size_t)c->stride * 4;
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(st::launch_mt_sync(params(c), nullptr));  // CPython's MT state in the snapshot
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy2D(o, row, c->board, pitch, row, c->cfg.width, hipMemcpyDeviceToHost));
    o += row * c->cfg.width;
    ST_HIP(hipMemcpy2D(o, row, c->stats, pitch, row, ST_NSTAT, hipMemcpyDeviceToHost));
    o += row * ST_NSTAT;
    const size_t mrow = (size_t)st::kMtN * 4, mpitch = (size_t)st::kMtPitch * 4;
    ST_HIP(hipMemcpy2D(o, mrow, c->mt, mpitch, mrow, (size_t)c->n, hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_load(st_ctx *c, const void *host_in, int64_t bytes) {
    if (!c || !host_in) return fail(ST_EINVAL, "st_load: null argument");
    if (bytes != snap_bytes(c))
        return fail(ST_EINVAL, "st_load: %lld bytes, this context's snapshot is %lld", (long long)bytes,
                    (long long)snap_bytes(c));
    SnapHeader h;
    memcpy(&h, host_in, sizeof(h));
    if (memcmp(h.magic, kSnapMagic, sizeof(h.magic)) != 0) return fail(ST_EINVAL, "st_load: not a snapshot");
    if (h.abi != kSnapVersion || h.nstat != ST_NSTAT)
        return fail(ST_EINVAL, "st_load: snapshot format %u (%d counter rows), this is %u (%d)", h.abi,
                    h.nstat, kSnapVersion, ST_NSTAT);
    if (h.width != c->cfg.width || h.height != c->cfg.height || h.n != c->n)
        return fail(ST_EINVAL, "st_load: snapshot of %lld %dx%d envs, context has %lld %dx%d",
                    (long long)h.n, h.width, h.height, (long long)c->n, c->cfg.width, c->cfg.height);
    const char *in = static_cast<const char *>(host_in) + sizeof(h);
    const size_t row = (size_t)c->n * 4, pitch = (size_t)c->stride * 4;
    {  // MT indexes must be CPython's (0..624): st_save writes them synced
        const int32_t *mi = reinterpret_cast<const int32_t *>(in + row * c->cfg.width) + ST_STAT_MT_INDEX * c->n;
        for (int64_t e = 0; e < c->n; ++e)
            if (mi[e] < 0 || mi[e] > st::kMtN)
                return fail(ST_EINVAL, "st_load: env %lld has MT index %d outside [0, 624]", (long long)e, mi[e]);
    }
    DeviceGuard g(c->device);
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy2D(c->board, pitch, in, row, row, c->cfg.width, hipMemcpyHostToDevice));
    in += row * c->cfg.width;
    ST_HIP(hipMemcpy2D(c->stats, pitch, in, row, row, ST_NSTAT, hipMemcpyHostToDevice));
    in += row * ST_NSTAT;
    const size_t mrow = (size_t)st::kMtN * 4, mpitch = (size_t)st::kMtPitch * 4;
    ST_HIP(hipMemcpy2D(c->mt, mpitch, in, mrow, mrow, (size_t)c->n, hipMemcpyHostToDevice));
    ST_HIP(hipDeviceSynchronize());
    c->seeded = c->reset_once = true;
    return ST_OK;
}

int st_debug_stamps(st_ctx *c, uint64_t *host_out, int64_t max_words) {
    if (!c || !host_out) return fail(ST_EINVAL, "st_debug_stamps: null argument");
    if (!c->stamps) return fail(ST_ESTATE, "context was not created with ST_STAMPS set");
    DeviceGuard g(c->device);
    int64_t n = (c->stride / st::kWave) * st::kStampWords;
    if (max_words < n) n = max_words;
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(host_out, c->stamps, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_policy_greedy(st_ctx *c, uint64_t seed, int64_t t, uint32_t explore_permille, uint8_t *d_actions,
                     st_stream stream) {
    if (!c || !d_actions) return fail(ST_EINVAL, "st_policy_greedy: null argument");
    if (t < 0 || explore_permille > 1000) return fail(ST_EINVAL, "st_policy_greedy: t < 0 or explore > 1000");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_policy_greedy before st_seed + st_reset");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_policy_greedy(params(c), seed, t, explore_permille, d_actions, (hipStream_t)stream));
    return ST_OK;
}

int st_after_slots(int32_t width) {
    if (width < 4 || width > st::kMaxW)
        return fail(ST_EINVAL, "st_after_slots: width %d outside [4, %d]", width, st::kMaxW);
    return 4 * (width + 6);
}

int st_afterstates(st_ctx *c, int32_t *d_feat, uint32_t *d_boards, st_stream stream) {
    if (!c || !d_feat) return fail(ST_EINVAL, "st_afterstates: null argument");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_afterstates before st_seed + st_reset");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_afterstates(params(c), d_feat, d_boards, (hipStream_t)stream));
    return ST_OK;
}

int st_placement_actions(st_ctx *c, const int32_t *d_slots, uint8_t *d_actions, st_stream stream) {
    if (!c || !d_slots || !d_actions) return fail(ST_EINVAL, "st_placement_actions: null argument");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_placement_actions before st_seed + st_reset");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_placement_actions(params(c), d_slots, d_actions, (hipStream_t)stream));
    return ST_OK;
}

int st_reachable(st_ctx *c, int32_t *d_steps, uint8_t *d_first, st_stream stream) {
    if (!c || !d_steps) return fail(ST_EINVAL, "st_reachable: null argument");
    if (c->cfg.lock_delay > ST_REACH_MAX_LOCK)
        return fail(ST_EINVAL, "st_reachable: lock_delay %d > %d", c->cfg.lock_delay, ST_REACH_MAX_LOCK);
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_reachable before st_seed + st_reset");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_reachable(params(c), d_steps, d_first, (hipStream_t)stream));
    return ST_OK;
}

int st_route_actions(st_ctx *c, const int32_t *d_slots, uint8_t *d_actions, int32_t *d_steps, st_stream stream) {
    if (!c || !d_slots || !d_actions) return fail(ST_EINVAL, "st_route_actions: null argument");
    if (c->cfg.lock_delay > ST_REACH_MAX_LOCK)
        return fail(ST_EINVAL, "st_route_actions: lock_delay %d > %d", c->cfg.lock_delay, ST_REACH_MAX_LOCK);
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_route_actions before st_seed + st_reset");
    DeviceGuard g(c->device);
    ST_HIP(st::launch_route_actions(params(c), d_slots, d_actions, d_steps, (hipStream_t)stream));
    return ST_OK;
}

int st_policy_linear(st_ctx *c, const float *d_weights, int64_t n_w, int32_t *d_slots, uint8_t *d_actions,
                     float *d_scores, int32_t *d_best, st_stream stream) {
    if (!c || !d_weights) return fail(ST_EINVAL, "st_policy_linear: null argument");
    if (n_w < 1) return fail(ST_EINVAL, "st_policy_linear: n_w %lld < 1", (long long)n_w);
    if (!d_slots && !d_actions && !d_scores && !d_best) return fail(ST_EINVAL, "st_policy_linear: every output is null");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_policy_linear before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_linear: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_policy_linear(params(c), d_weights, n_w, d_slots, d_actions, d_scores, d_best,
                                    (hipStream_t)stream));
    return ST_OK;
}

// st_play_linear (commit false: the policy's primitive action, then the step
// on it) and st_play_linear_placements (commit true: the policy commits its
// slot, then the step on the constant hard drop)
// set: the rows the policy scores (st_play_linear_set; the base set runs the two older kernels)
// look: st_play_lookahead -- the policy is the two-ply kernel (d_weights its second-ply rows, look->weights1 its
// first-ply rows or null), committing its own choice
// look->expect: st_play_expect -- the same with the expectimax kernel (the odds of the next piece, not the piece)
struct PlayLookahead {
    const float *weights1;
    float dead_value;
    bool expect = false;
};
// routed: st_play_routed -- the planner for the envs whose plan has run out, then the pop of every env's next action
// locks: st_play_locks -- the planner over every lock position (plan_slot then holds the chosen position)
struct PlayRouted {
    int32_t *pieces;
    bool locks = false;
};
// ntuple: st_play_ntuple -- the policy is the n-tuple kernel (d_weights its first-ply rows or null), committing its
// own choice
struct PlayNtuple {
    const float *table;
    float dead_value;
};
static int play_impl(st_ctx *c, const char *fn, bool commit, const float *d_weights, int64_t n_w, int64_t k,
                     int64_t *d_return, int32_t *d_episodes, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                     st_stream stream, int32_t set = ST_FEATS_BASE, const PlayLookahead *look = nullptr,
                     const PlayRouted *routed = nullptr, const PlayNtuple *ntuple = nullptr) {
    if (!c || (ntuple ? !ntuple->table : !d_weights)) return fail(ST_EINVAL, "%s: null argument", fn);
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS) return fail(ST_EINVAL, "%s: unknown feature set %d", fn, set);
    if (n_w < 1 && d_weights) return fail(ST_EINVAL, "%s: n_w %lld < 1", fn, (long long)n_w);
    if (look && !std::isfinite(look->dead_value)) return fail(ST_EINVAL, "%s: dead_value is not finite", fn);
    if (ntuple && !std::isfinite(ntuple->dead_value)) return fail(ST_EINVAL, "%s: dead_value is not finite", fn);
    if (routed && c->cfg.lock_delay > ST_REACH_MAX_LOCK)
        return fail(ST_EINVAL, "%s: lock_delay %d > %d", fn, c->cfg.lock_delay, ST_REACH_MAX_LOCK);
    if (ntuple && c->nt_T < 1) return fail(ST_ESTATE, "%s without a network (st_ntuple_set)", fn);
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "%s before st_seed + st_reset", fn);
    if (k <= 0) return ST_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "%s: hipSetDevice(%d) failed", fn, c->device);
    hipStream_t s = (hipStream_t)stream;
    PlayParts q;
    if (const int rc = play_parts(c, fn, s, &q)) return rc;
    const int64_t n = c->n, R = q.R;
    const bool acc = d_return || d_episodes;
    // With accumulators, step i writes its reward / done into the ring's next
    // row, and one launch behind every R steps (and behind the last) adds the
    // rows; the last of them also copies the last row out to d_reward / d_done.
    // Without, the steps write d_reward / d_done themselves.  d_obs is the
    // last step's alone.
    int row = 0;
    if (routed) ST_HIP(hipMemsetAsync(q.plan_rem, 0, (size_t)n * sizeof(int32_t), s));  // plans are local to a call
    for (int64_t i = 0; i < k; ++i) {
        const bool last = i == k - 1;
        if (routed) {
            if (routed->locks)
                ST_HIP(st::launch_locks(params(c), set, d_weights, n_w, nullptr, nullptr, q.plan_rem, q.plan_slot,
                                        q.plan_route, q.plan_steps, nullptr, nullptr, nullptr, s));
            else
                ST_HIP(st::launch_routes(params(c), set, d_weights, n_w, nullptr, nullptr, q.plan_rem, q.plan_slot,
                                         q.plan_route, q.plan_steps, nullptr, s));
            ST_HIP(st::launch_route_pop(params(c), q.plan_route, q.plan_steps, q.plan_rem, q.act, routed->pieces, s));
        } else if (ntuple)
            ST_HIP(st::launch_policy_ntuple(params(c), set, true, d_weights, n_w, c->nt_desc, c->nt_T, ntuple->table,
                                            ntuple->dead_value, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, s));
        else if (look && look->expect)
            ST_HIP(st::launch_policy_expect(params(c), set, true, look->weights1, d_weights, n_w, look->dead_value,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s));
        else if (look)
            ST_HIP(st::launch_policy_lookahead(params(c), set, true, look->weights1, d_weights, n_w, look->dead_value,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s));
        else if (set != ST_FEATS_BASE)
            ST_HIP(st::launch_policy_linear_set(params(c), set, commit, d_weights, n_w, nullptr, nullptr,
                                                commit ? nullptr : q.act, nullptr, nullptr, s));
        else if (commit) ST_HIP(st::launch_policy_linear_commit(params(c), d_weights, n_w, s));
        else ST_HIP(st::launch_policy_linear(params(c), d_weights, n_w, nullptr, q.act, nullptr, nullptr, s));
        int32_t *rew = acc || !d_reward ? q.ring_rew + (int64_t)row * n : d_reward;
        uint8_t *done = acc || !d_done ? q.ring_done + (int64_t)row * n : d_done;
        const int rc = step_impl(c, commit ? q.twos : q.act, last ? d_obs : nullptr, nullptr, rew, done, stream,
                                 nullptr, nullptr, /*gated=*/false);
        if (rc != ST_OK) return rc;
        if (!acc) continue;
        if (++row == R || last) {
            ST_HIP(st::launch_play_sum(params(c), q.ring_rew, q.ring_done, row, d_return, d_episodes,
                                       last ? d_reward : nullptr, last ? d_done : nullptr, s));
            row = 0;
        }
    }
    return ST_OK;
}

int st_play_linear(st_ctx *c, const float *d_weights, int64_t n_w, int64_t k, int64_t *d_return, int32_t *d_episodes,
                   uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    return play_impl(c, "st_play_linear", false, d_weights, n_w, k, d_return, d_episodes, d_obs, d_reward, d_done,
                     stream);
}

int st_play_linear_placements(st_ctx *c, const float *d_weights, int64_t n_w, int64_t k, int64_t *d_return,
                              int32_t *d_episodes, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                              st_stream stream) {
    return play_impl(c, "st_play_linear_placements", true, d_weights, n_w, k, d_return, d_episodes, d_obs, d_reward,
                     d_done, stream);
}

int st_feature_rows(int32_t set) {
    if (set == ST_FEATS_BASE) return ST_AFTER_NFEAT;
    if (set == ST_FEATS_BCTS) return ST_AFTER_NFEAT + ST_AFTER_NEXT;
    return fail(ST_EINVAL, "st_feature_rows: unknown feature set %d", set);
}

int st_afterstates_set(st_ctx *c, int32_t set, int32_t *d_feat, uint32_t *d_boards, st_stream stream) {
    if (!c || !d_feat) return fail(ST_EINVAL, "st_afterstates_set: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_afterstates_set: unknown feature set %d", set);
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_afterstates_set before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_afterstates_set: hipSetDevice(%d) failed", c->device);
    if (set == ST_FEATS_BASE) ST_HIP(st::launch_afterstates(params(c), d_feat, d_boards, (hipStream_t)stream));
    else ST_HIP(st::launch_afterstates_set(params(c), set, d_feat, d_boards, (hipStream_t)stream));
    return ST_OK;
}

int st_policy_linear_set(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, const int32_t *d_allowed,
                         int32_t *d_slots, uint8_t *d_actions, float *d_scores, int32_t *d_best, st_stream stream) {
    if (!c || !d_weights) return fail(ST_EINVAL, "st_policy_linear_set: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_policy_linear_set: unknown feature set %d", set);
    if (n_w < 1) return fail(ST_EINVAL, "st_policy_linear_set: n_w %lld < 1", (long long)n_w);
    if (!d_slots && !d_actions && !d_scores && !d_best)
        return fail(ST_EINVAL, "st_policy_linear_set: every output is null");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_policy_linear_set before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_linear_set: hipSetDevice(%d) failed", c->device);
    if (set == ST_FEATS_BASE && !d_allowed)  // st_policy_linear's own kernel
        ST_HIP(st::launch_policy_linear(params(c), d_weights, n_w, d_slots, d_actions, d_scores, d_best,
                                        (hipStream_t)stream));
    else
        ST_HIP(st::launch_policy_linear_set(params(c), set, false, d_weights, n_w, d_allowed, d_slots, d_actions,
                                            d_scores, d_best, (hipStream_t)stream));
    return ST_OK;
}

int st_play_linear_set(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, int64_t k, int32_t placements,
                       int64_t *d_return, int32_t *d_episodes, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                       st_stream stream) {
    return play_impl(c, "st_play_linear_set", placements != 0, d_weights, n_w, k, d_return, d_episodes, d_obs,
                     d_reward, d_done, stream, set);
}

int st_next_piece(st_ctx *c, uint8_t *d_next, st_stream stream) {
    if (!c || !d_next) return fail(ST_EINVAL, "st_next_piece: null argument");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_next_piece before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_next_piece: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_next_piece(params(c), d_next, (hipStream_t)stream));
    return ST_OK;
}

int st_fork(st_ctx *dst, st_ctx *src, const int32_t *d_index, const uint8_t *d_mask, uint32_t flags,
            st_stream stream) {
    if (!dst || !src) return fail(ST_EINVAL, "st_fork: null context");
    if (flags & ~(uint32_t)ST_FORK_KEEP_RNG) return fail(ST_EINVAL, "st_fork: unknown flag bits 0x%x", flags);
    if (dst->cfg.width != src->cfg.width || dst->cfg.height != src->cfg.height)
        return fail(ST_EINVAL, "st_fork: a %dx%d context from a %dx%d one", dst->cfg.width, dst->cfg.height,
                    src->cfg.width, src->cfg.height);
    if (dst->device != src->device)
        return fail(ST_EINVAL, "st_fork: contexts on devices %d and %d", dst->device, src->device);
    if (!dst->seeded || !dst->reset_once || !src->seeded || !src->reset_once)
        return fail(ST_ESTATE, "st_fork before st_seed + st_reset of both contexts");
    // the deep copy's grid: one wave per 64 envs (measured no slower than four, DESIGN.md "Fork"); DIAGNOSTIC
    // (tools/fork_bench.py's A/B of the two): ST_FORK_WAVES=4 selects the other
    int waves = 1;
    if (const char *w = getenv("ST_FORK_WAVES")) waves = atoi(w) == 4 ? 4 : 1;
    DeviceGuard g(dst->device);
    if (!g.ok) return fail(ST_EHIP, "st_fork: hipSetDevice(%d) failed", dst->device);
    ST_HIP(st::launch_fork(params(dst), params(src), d_index, d_mask, (flags & ST_FORK_KEEP_RNG) != 0, waves,
                           (hipStream_t)stream));
    return ST_OK;
}

int st_policy_lookahead(st_ctx *c, int32_t set, const float *d_weights1, const float *d_weights2, int64_t n_w,
                        float dead_value, const int32_t *d_allowed, int32_t *d_slots, int32_t *d_slots2,
                        uint8_t *d_actions, float *d_scores, float *d_scores_all, int32_t *d_slots2_all,
                        st_stream stream) {
    if (!c || !d_weights2) return fail(ST_EINVAL, "st_policy_lookahead: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_policy_lookahead: unknown feature set %d", set);
    if (n_w < 1) return fail(ST_EINVAL, "st_policy_lookahead: n_w %lld < 1", (long long)n_w);
    if (!d_slots && !d_slots2 && !d_actions && !d_scores && !d_scores_all && !d_slots2_all)
        return fail(ST_EINVAL, "st_policy_lookahead: every output is null");
    if (!std::isfinite(dead_value)) return fail(ST_EINVAL, "st_policy_lookahead: dead_value is not finite");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_policy_lookahead before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_lookahead: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_policy_lookahead(params(c), set, false, d_weights1, d_weights2, n_w, dead_value, d_allowed,
                                       d_slots, d_slots2, d_actions, d_scores, d_scores_all, d_slots2_all,
                                       (hipStream_t)stream));
    return ST_OK;
}

int st_play_lookahead(st_ctx *c, int32_t set, const float *d_weights1, const float *d_weights2, int64_t n_w,
                      float dead_value, int64_t k, int64_t *d_return, int32_t *d_episodes, uint32_t *d_obs,
                      int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    const PlayLookahead look{d_weights1, dead_value};
    return play_impl(c, "st_play_lookahead", true, d_weights2, n_w, k, d_return, d_episodes, d_obs, d_reward, d_done,
                     stream, set, &look);
}

int st_next_weights(st_ctx *c, int32_t *d_m, st_stream stream) {
    if (!c || !d_m) return fail(ST_EINVAL, "st_next_weights: null argument");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_next_weights before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_next_weights: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_next_weights(params(c), d_m, (hipStream_t)stream));
    return ST_OK;
}

int st_policy_expect(st_ctx *c, int32_t set, const float *d_weights1, const float *d_weights2, int64_t n_w,
                     float dead_value, const int32_t *d_allowed, int32_t *d_slots, uint8_t *d_actions,
                     float *d_scores, float *d_scores_all, float *d_tails, int32_t *d_slots2_all, st_stream stream) {
    if (!c || !d_weights2) return fail(ST_EINVAL, "st_policy_expect: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_policy_expect: unknown feature set %d", set);
    if (n_w < 1) return fail(ST_EINVAL, "st_policy_expect: n_w %lld < 1", (long long)n_w);
    if (!d_slots && !d_actions && !d_scores && !d_scores_all && !d_tails && !d_slots2_all)
        return fail(ST_EINVAL, "st_policy_expect: every output is null");
    if (!std::isfinite(dead_value)) return fail(ST_EINVAL, "st_policy_expect: dead_value is not finite");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_policy_expect before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_expect: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_policy_expect(params(c), set, false, d_weights1, d_weights2, n_w, dead_value, d_allowed, d_slots,
                                    d_actions, d_scores, d_scores_all, d_tails, d_slots2_all, (hipStream_t)stream));
    return ST_OK;
}

int st_play_expect(st_ctx *c, int32_t set, const float *d_weights1, const float *d_weights2, int64_t n_w,
                   float dead_value, int64_t k, int64_t *d_return, int32_t *d_episodes, uint32_t *d_obs,
                   int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    const PlayLookahead look{d_weights1, dead_value, true};
    return play_impl(c, "st_play_expect", true, d_weights2, n_w, k, d_return, d_episodes, d_obs, d_reward, d_done,
                     stream, set, &look);
}

// what st_routes / st_policy_routed check before any GPU call
static int routes_check(st_ctx *c, const char *fn, bool ptrs_ok) {
    if (!c || !ptrs_ok) return fail(ST_EINVAL, "%s: null argument", fn);
    if (c->cfg.lock_delay > ST_REACH_MAX_LOCK)
        return fail(ST_EINVAL, "%s: lock_delay %d > %d", fn, c->cfg.lock_delay, ST_REACH_MAX_LOCK);
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "%s before st_seed + st_reset", fn);
    return ST_OK;
}

int st_routes(st_ctx *c, const int32_t *d_slots, const uint8_t *d_need, uint64_t *d_route, int32_t *d_steps,
              st_stream stream) {
    if (const int rc = routes_check(c, "st_routes", d_slots && d_route)) return rc;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_routes: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_routes(params(c), -1, nullptr, 0, d_slots, d_need, nullptr, nullptr, d_route, d_steps, nullptr,
                             (hipStream_t)stream));
    return ST_OK;
}

int st_policy_routed(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, const uint8_t *d_need,
                     int32_t *d_slots, uint64_t *d_route, int32_t *d_steps, float *d_scores, st_stream stream) {
    if (!c || !d_weights || !d_slots || !d_route) return fail(ST_EINVAL, "st_policy_routed: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_policy_routed: unknown feature set %d", set);
    if (n_w < 1) return fail(ST_EINVAL, "st_policy_routed: n_w %lld < 1", (long long)n_w);
    if (const int rc = routes_check(c, "st_policy_routed", true)) return rc;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_routed: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_routes(params(c), set, d_weights, n_w, nullptr, d_need, nullptr, d_slots, d_route, d_steps,
                             d_scores, (hipStream_t)stream));
    return ST_OK;
}

int st_play_routed(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, int64_t k, int64_t *d_return,
                   int32_t *d_episodes, int32_t *d_pieces, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                   st_stream stream) {
    const PlayRouted routed{d_pieces};
    return play_impl(c, "st_play_routed", false, d_weights, n_w, k, d_return, d_episodes, d_obs, d_reward, d_done,
                     stream, set, nullptr, &routed);
}

int st_lock_set(st_ctx *c, uint32_t *d_rows, int32_t *d_pos, int64_t cap, int32_t *d_count, st_stream stream) {
    if (const int rc = routes_check(c, "st_lock_set", d_rows || d_pos || d_count)) return rc;
    if (d_pos && cap < 1) return fail(ST_EINVAL, "st_lock_set: cap %lld < 1", (long long)cap);
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_lock_set: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_lock_set(params(c), d_rows, d_pos, d_pos ? cap : 0, d_count, (hipStream_t)stream));
    return ST_OK;
}

int st_afterstates_at(st_ctx *c, int32_t set, const int32_t *d_pos, int64_t cap, int32_t *d_feat, uint32_t *d_boards,
                      st_stream stream) {
    if (!c || !d_pos || !d_feat) return fail(ST_EINVAL, "st_afterstates_at: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_afterstates_at: unknown feature set %d", set);
    if (cap < 1) return fail(ST_EINVAL, "st_afterstates_at: cap %lld < 1", (long long)cap);
    if (const int rc = routes_check(c, "st_afterstates_at", true)) return rc;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_afterstates_at: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_afterstates_at(params(c), set, d_pos, cap, d_feat, d_boards, (hipStream_t)stream));
    return ST_OK;
}

int st_routes_at(st_ctx *c, const int32_t *d_pos, const uint8_t *d_need, uint64_t *d_route, int32_t *d_steps,
                 st_stream stream) {
    if (const int rc = routes_check(c, "st_routes_at", d_pos && d_route)) return rc;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_routes_at: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_locks(params(c), -1, nullptr, 0, d_pos, d_need, nullptr, nullptr, d_route, d_steps, nullptr,
                            nullptr, nullptr, (hipStream_t)stream));
    return ST_OK;
}

int st_policy_locks(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, const uint8_t *d_need, int32_t *d_pos,
                    uint64_t *d_route, int32_t *d_steps, float *d_scores, int32_t *d_best, int32_t *d_count,
                    st_stream stream) {
    if (!c || !d_weights || !d_pos) return fail(ST_EINVAL, "st_policy_locks: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_policy_locks: unknown feature set %d", set);
    if (n_w < 1) return fail(ST_EINVAL, "st_policy_locks: n_w %lld < 1", (long long)n_w);
    if (const int rc = routes_check(c, "st_policy_locks", true)) return rc;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_locks: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_locks(params(c), set, d_weights, n_w, nullptr, d_need, nullptr, d_pos, d_route, d_steps, d_scores,
                            d_best, d_count, (hipStream_t)stream));
    return ST_OK;
}

int st_play_locks(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, int64_t k, int64_t *d_return,
                  int32_t *d_episodes, int32_t *d_pieces, uint32_t *d_obs, int32_t *d_reward, uint8_t *d_done,
                  st_stream stream) {
    PlayRouted routed{d_pieces};
    routed.locks = true;
    return play_impl(c, "st_play_locks", false, d_weights, n_w, k, d_return, d_episodes, d_obs, d_reward, d_done,
                     stream, set, nullptr, &routed);
}

int st_ntuple_set(st_ctx *c, const int32_t *tuples_host, int32_t T) {
    if (!c) return fail(ST_EINVAL, "st_ntuple_set: null context");
    if (T < 0 || T > st::kNtMaxT)
        return fail(ST_EINVAL, "st_ntuple_set: T %d outside [0, %d]", T, st::kNtMaxT);
    if (T > 0 && !tuples_host) return fail(ST_EINVAL, "st_ntuple_set: null tuples");
    const int W = c->cfg.width, H = c->cfg.height;
    int64_t len = 0;
    for (int32_t t = 0; t < T; ++t) {
        const int32_t *d = tuples_host + 6 * (int64_t)t;
        const int64_t x = d[0], y = d[1], w = d[2], h = d[3], flip = d[4], base = d[5];
        const char *bad = w < 1 || h < 1                  ? "w or h < 1"
                          : w * h > ST_NTUPLE_MAX_BITS    ? "more than 16 cells"
                          : x < 0 || x + w > W            ? "columns off the board"
                          : y < 0 || y + h > H            ? "rows off the board"
                          : flip != 0 && flip != 1        ? "flip not 0 or 1"
                          : base < 0                      ? "negative base"
                          : base + (int64_t(1) << (w * h)) > INT32_MAX ? "table_len above 2^31 - 1"
                                                          : nullptr;
        if (bad)
            return fail(ST_EINVAL, "st_ntuple_set: tuple %d (x %d, y %d, w %d, h %d, flip %d, base %d) on a %dx%d board: %s",
                        t, d[0], d[1], d[2], d[3], d[4], d[5], W, H, bad);
        len = std::max(len, base + (int64_t(1) << (w * h)));
    }
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_ntuple_set: hipSetDevice(%d) failed", c->device);
    int32_t *desc = nullptr;
    if (T > 0) {
        const size_t bytes = (size_t)T * 6 * sizeof(int32_t);
        hipError_t e = hipMalloc(&desc, bytes);
        if (e != hipSuccess) return fail(ST_ENOMEM, "st_ntuple_set: hipMalloc failed: %s", hipGetErrorString(e));
        e = hipMemcpy(desc, tuples_host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(desc);
            return hip_fail(e, "st_ntuple_set: uploading the descriptors");
        }
    }
    if (c->nt_desc) {  // (launches that read the old descriptors may still be queued)
        (void)hipDeviceSynchronize();
        (void)hipFree(c->nt_desc);
    }
    c->nt_desc = desc;
    c->nt_T = T;
    c->nt_len = len;
    return ST_OK;
}

int64_t st_ntuple_table_len(const st_ctx *c) { return c ? c->nt_len : 0; }

int st_ntuple_eval(st_ctx *c, const float *d_table, const uint32_t *d_boards, int64_t m, float *d_values,
                   int32_t *d_index, st_stream stream) {
    if (!c || !d_table) return fail(ST_EINVAL, "st_ntuple_eval: null argument");
    if (!d_values && !d_index) return fail(ST_EINVAL, "st_ntuple_eval: every output is null");
    if (d_boards && m < 0) return fail(ST_EINVAL, "st_ntuple_eval: m %lld < 0", (long long)m);
    if (c->nt_T < 1) return fail(ST_ESTATE, "st_ntuple_eval without a network (st_ntuple_set)");
    if (!d_boards && (!c->seeded || !c->reset_once))
        return fail(ST_ESTATE, "st_ntuple_eval of the context's boards before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_ntuple_eval: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_ntuple_eval(c->nt_desc, c->nt_T, d_table, d_boards ? d_boards : c->board,
                                  d_boards ? m : c->stride, d_boards ? m : c->n, d_values, d_index,
                                  (hipStream_t)stream));
    return ST_OK;
}

int st_policy_ntuple(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, const float *d_table,
                     float dead_value, const int32_t *d_allowed, int32_t *d_slots, uint8_t *d_actions,
                     float *d_scores, float *d_values, int32_t *d_best, int32_t *d_index, float *d_values_all,
                     st_stream stream) {
    if (!c || !d_table) return fail(ST_EINVAL, "st_policy_ntuple: null argument");
    if (set != ST_FEATS_BASE && set != ST_FEATS_BCTS)
        return fail(ST_EINVAL, "st_policy_ntuple: unknown feature set %d", set);
    if (d_weights && n_w < 1) return fail(ST_EINVAL, "st_policy_ntuple: n_w %lld < 1", (long long)n_w);
    if (!d_slots && !d_actions && !d_scores && !d_values && !d_best && !d_index && !d_values_all)
        return fail(ST_EINVAL, "st_policy_ntuple: every output is null");
    if (!std::isfinite(dead_value)) return fail(ST_EINVAL, "st_policy_ntuple: dead_value is not finite");
    if (c->nt_T < 1) return fail(ST_ESTATE, "st_policy_ntuple without a network (st_ntuple_set)");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_policy_ntuple before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_policy_ntuple: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_policy_ntuple(params(c), set, false, d_weights, n_w, c->nt_desc, c->nt_T, d_table, dead_value,
                                    d_allowed, d_slots, d_actions, d_scores, d_values, d_best, d_index, d_values_all,
                                    (hipStream_t)stream));
    return ST_OK;
}

int st_play_ntuple(st_ctx *c, int32_t set, const float *d_weights, int64_t n_w, const float *d_table,
                   float dead_value, int64_t k, int64_t *d_return, int32_t *d_episodes, uint32_t *d_obs,
                   int32_t *d_reward, uint8_t *d_done, st_stream stream) {
    const PlayNtuple nt{d_table, dead_value};
    return play_impl(c, "st_play_ntuple", true, d_weights, n_w, k, d_return, d_episodes, d_obs, d_reward, d_done,
                     stream, set, nullptr, nullptr, &nt);
}

int st_place(st_ctx *c, const int32_t *d_slots, uint8_t *d_placed, st_stream stream) {
    if (!c || !d_slots) return fail(ST_EINVAL, "st_place: null argument");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_place before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_place: hipSetDevice(%d) failed", c->device);
    ST_HIP(st::launch_place(params(c), d_slots, d_placed, (hipStream_t)stream));
    return ST_OK;
}

int st_step_placements(st_ctx *c, const int32_t *d_slots, uint8_t *d_placed, uint32_t *d_obs, int32_t *d_reward,
                       uint8_t *d_done, st_stream stream) {
    if (!c || !d_slots) return fail(ST_EINVAL, "st_step_placements: null argument");
    if (!c->seeded || !c->reset_once) return fail(ST_ESTATE, "st_step_placements before st_seed + st_reset");
    DeviceGuard g(c->device);
    if (!g.ok) return fail(ST_EHIP, "st_step_placements: hipSetDevice(%d) failed", c->device);
    hipStream_t s = (hipStream_t)stream;
    PlayParts q;
    if (const int rc = play_parts(c, "st_step_placements", s, &q)) return rc;
    ST_HIP(st::launch_place(params(c), d_slots, d_placed, s));
    // (not gated: the actions are the context's own, an armed st_gate_actions stays armed)
    return step_impl(c, q.twos, d_obs, nullptr, d_reward, d_done, stream, nullptr, nullptr, /*gated=*/false);
}

int st_check_actions(const uint8_t *d_actions, int64_t n, uint32_t *d_flag, st_stream stream) {
    if (n < 0) return fail(ST_EINVAL, "st_check_actions: negative size");
    if (n > 0 && (!d_actions || !d_flag)) return fail(ST_EINVAL, "st_check_actions: null argument");
    ST_HIP(st::launch_check_actions(d_actions, n, d_flag, (hipStream_t)stream));
    return ST_OK;
}

int st_set_action_flag(st_ctx *c, uint32_t *d_flag) {
    if (!c) return fail(ST_EINVAL, "st_set_action_flag: null context");
    c->act_flag = d_flag;
    return ST_OK;
}

int st_gate_actions(st_ctx *c, const uint8_t *d_actions, st_stream stream) {
    if (!c || !d_actions) return fail(ST_EINVAL, "st_gate_actions: null argument");
    DeviceGuard g(c->device);
    if (!c->gate) {  // first use: the gate words (k_gate_actions), the mapped host word, the event
        // into locals first: the context takes them only when every one
        // succeeded (a later call never meets a half-built gate)
        uint32_t *gate = nullptr, *host = nullptr;
        void *host_dev = nullptr;
        hipEvent_t ev = nullptr;
        hipError_t e = hipMalloc(&gate, 4 * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(gate, 0, 4 * sizeof(uint32_t));
        if (e == hipSuccess) e = hipHostMalloc(&host, sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&host_dev, host, 0);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            if (ev) (void)hipEventDestroy(ev);
            if (host) (void)hipHostFree(host);
            if (gate) (void)hipFree(gate);
            return hip_fail(e, "st_gate_actions: allocating the gate");
        }
        *host = 0;
        c->gate = gate;
        c->gate_host = host;
        c->gate_host_dev = static_cast<uint32_t *>(host_dev);
        c->gate_ev = ev;
    }
    c->gate_epoch = (c->gate_epoch + 1u) & 0x7FFFFFFFu ? (c->gate_epoch + 1u) & 0x7FFFFFFFu : 1u;  // 31 bits, never 0
    hipStream_t s = (hipStream_t)stream;
    ST_HIP(st::launch_gate_actions(d_actions, c->n, c->gate, c->gate_host_dev, c->gate_epoch, s));  // gate = words[0]
    ST_HIP(hipEventRecord(c->gate_ev, s));
    c->gate_armed = true;
    c->gate_pending = true;
    return ST_OK;
}

int st_gate_wait(st_ctx *c) {
    if (!c) return fail(ST_EINVAL, "st_gate_wait: null context");
    if (!c->gate_pending) return fail(ST_ESTATE, "st_gate_wait without st_gate_actions");
    c->gate_pending = false;
    // the gate ends here: a step not launched by now (its launch failed, or
    // the caller never made it) is not gated by this check later
    c->gate_armed = false;
    // the gate kernel's last block writes epoch | bad << 31 to the mapped
    // host word (system scope): spin on it -- the wake-up of an event wait
    // costs more than the check itself -- and fall back to the event after
    // ~4 million polls (a few ms: the stream was busy with earlier work)
    const uint32_t ep = c->gate_epoch;
    for (int i = 0; i < (1 << 22); ++i) {
        const uint32_t v = __atomic_load_n(c->gate_host, __ATOMIC_ACQUIRE);
        if ((v & 0x7FFFFFFFu) == ep) return (int)(v >> 31);
        __builtin_ia32_pause();
    }
    DeviceGuard g(c->device);
    ST_HIP(hipEventSynchronize(c->gate_ev));
    const uint32_t v = __atomic_load_n(c->gate_host, __ATOMIC_ACQUIRE);
    if ((v & 0x7FFFFFFFu) != ep) return fail(ST_EHIP, "st_gate_wait: the gate kernel finished without its answer");
    return (int)(v >> 31);
}

int st_stream_wait(st_stream waiter, st_stream signaller) {
    if (waiter == signaller) return ST_OK;
    int dev = 0;
    ST_HIP(hipGetDevice(&dev));
    // one reusable event per (device, signalling stream) and thread: a wait
    // enqueued by hipStreamWaitEvent keeps the record it saw, so re-recording
    // the event for the next call is safe
    struct Ev {
        int dev;
        st_stream s;
        hipEvent_t ev;
    };
    thread_local Ev cache[16];
    thread_local int used = 0;
    hipEvent_t ev = nullptr;
    for (int i = 0; i < used; ++i)
        if (cache[i].dev == dev && cache[i].s == signaller) ev = cache[i].ev;
    if (!ev) {
        ST_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (used < 16) {
            cache[used++] = Ev{dev, signaller, ev};
        } else {  // evict the oldest entry
            (void)hipEventDestroy(cache[0].ev);
            for (int i = 1; i < 16; ++i) cache[i - 1] = cache[i];
            cache[15] = Ev{dev, signaller, ev};
        }
    }
    ST_HIP(hipEventRecord(ev, (hipStream_t)signaller));
    ST_HIP(hipStreamWaitEvent((hipStream_t)waiter, ev, 0));
    return ST_OK;
}

int st_stream_sync(st_stream stream) {
    ST_HIP(hipStreamSynchronize((hipStream_t)stream));
    return ST_OK;
}

int st_host_device_ptr(void *host, void **d_out) {
    if (!host || !d_out) return fail(ST_EINVAL, "st_host_device_ptr: null argument");
    *d_out = nullptr;
    ST_HIP(hipHostGetDevicePointer(d_out, host, 0));
    return ST_OK;
}

int st_gen_actions(uint8_t *d_out, int64_t n, int64_t t, uint64_t seed, int64_t global_offset,
                   st_stream stream) {
    if (!d_out && n > 0) return fail(ST_EINVAL, "st_gen_actions: null output");
    if (n < 0 || t < 0) return fail(ST_EINVAL, "st_gen_actions: negative size/time");
    ST_HIP(st::launch_gen_actions(d_out, n, t, seed, global_offset, (hipStream_t)stream));
    return ST_OK;
}

}  // extern "C"
