// nlsolver_amd/csrc/nlsg_de.hip — host side of the DE engine + its C-ABI
// (include/nlsg_c_api.h). Owns the device buffers and the HIP stream; enqueues
// the kernels of nlsg_de_kernels.h. No CPU fallback: every entry point either
// runs on a gfx950 device or returns an error.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "nlsg_comm.h"
#include "nlsg_de_kernels.h"
#include "nlsg_engine.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_de : EngineBase {
  nlsg_de_config cfg;
  DeParams p;
  double *x0_dev = nullptr;
  double *zero_dev = nullptr;
  double *rec = nullptr;  // local record (single-GPU finaliser input)
  int chunks = 0;
  int group = 0;  // lanes per agent when several agents share a wave (D <= 64), else 0
  bool long_rows = false;  // D > 1024: rows streamed in segments (de_*_long_kernel)
  bool initialised = false;
  uint64_t k = 0;            // generations launched so far (= index of the next head)
  // strategy random: the head of turn k (scan, stop tests) does not feed generation k+1
  // except through the stop flag, so it runs on a side stream beside that generation
  // (the generation is non-destructive: it writes the other population / score buffers).
  hipStream_t side = nullptr;
  hipEvent_t ev_gen[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_head[4] = {nullptr, nullptr, nullptr, nullptr};
  ShardComm *comm = nullptr;  // set by nlsg_de_comm_attach
  DeRtcKernels rtc;           // objective == NLSG_OBJ_CUSTOM: the kernels hiprtc built for it
  bool overlap = false;
  bool fused = false;   // head k and generation k+1 share one launch (strategy random, one GPU)
  // The screening wave pays where the screen decides nearly every agent and costs where it does not
  // (its undecided agents run one after the other in one wave). The waves that start at a multiple
  // of 128 agents count the decisions of their first two agents on the device; wherever the host reads the state anyway (status, best, download, the
  // polls of minimize) it compares the count with the generations launched since the last look and
  // drops bit kDeBoundScreen of DeParams.bound -- the parent's one-agent launches -- while the share
  // of decided agents is below kDeScreenKeep, then tries the screening wave again for one interval after
  // kDeScreenProbe generations. Switching changes the path only, never an output: the one-agent
  // path clears the miss counts it writes over. NLSG_DE_SCREEN_ADAPT=0: the screening wave stays on.
  bool screen_capable = false, screen_adapt = false;
  uint32_t stat_seen = 0;   // the device's count at the last look
  uint64_t k_seen = 0;      // generations launched at the last look
  uint64_t k_off = 0;       // generations launched when the screening wave was switched off
};

namespace {

// kernels of a run-time compiled objective take the same arguments through the module API
void launch_module(nlsg_de *e, hipFunction_t fn, unsigned grid, void **args) {
  launch_module_kernel(fn, grid, 256, 0, e->stream, args);
}

void launch_init(nlsg_de *e) {
  const dim3 grid(static_cast<unsigned>((e->p.shard_n + 3) / 4)), block(256);
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &e->x0_dev};
    launch_module(e, e->rtc.init, grid.x, args);
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    return with_bool(e->p.vec, [&](auto V) {
      if (e->long_rows) {  // D > 1024: the segment-streaming kernels, per objective and row alignment only
        hipLaunchKernelGGL((de_init_long_kernel<O, V>), grid, block, 0, e->stream, e->p, e->x0_dev);
        return true;
      }
      return with_chunks(e->chunks, [&](auto C) {
        hipLaunchKernelGGL((de_init_kernel<O, C, V>), grid, block, 0, e->stream, e->p, e->x0_dev);
      });
    });
  }));
}

// The instantiation <OBJ, C, V, B, S> of a one-agent-per-wave generation family (de_generation_kernel,
// de_turn_kernel) that this engine launches; launch(O, C, V, B, S) enqueues it. An engine that uses
// the bound launches the instantiation that has it (DeParams.bound, objectives with terms >= 0
// only), and one that screens, the instantiation with the screening wave (kDeBoundScreen, one
// chunk only).
template <typename Launch>
bool with_wave_kernel(const nlsg_de *e, Launch &&launch) {
  return with_objective(e->cfg.objective, [&](auto O) {
    return with_chunks(e->chunks, [&](auto C) {
      return with_bool(e->p.vec, [&](auto V) {
        using B = std::bool_constant<TermsNonNegative<O>::value>;
        using S = std::bool_constant<B::value && C == 1>;
        if (e->p.bound & kDeBoundScreen) launch(O, C, V, B{}, S{});
        else if (e->p.bound) launch(O, C, V, B{}, std::false_type{});
        else launch(O, C, V, std::false_type{}, std::false_type{});
      });
    });
  });
}

// waves of a generation: one per agent, one per 64 / group agents (D <= 64), or one per
// kDeScreenAgents = 4 agents (the screening wave, kDeBoundScreen)
uint64_t generation_waves(const nlsg_de *e) {
  const uint64_t per_wave = (e->p.bound & kDeBoundScreen) ? kDeScreenAgents : e->group ? 64 / e->group : 1;
  return (e->p.shard_n + per_wave - 1) / per_wave;
}

void launch_generation(nlsg_de *e, int par, uint64_t generation, int ignore_done = 0) {
  e->p.gen_key = ctr_key(e->p.seed, generation);
  const uint64_t waves = generation_waves(e);
  const dim3 grid(static_cast<unsigned>((waves + 3) / 4)), block(256);
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &par, &generation, &ignore_done};
    launch_module(e, e->rtc.generation, grid.x, args);
    return;
  }
  if (e->long_rows) {
    routed(with_objective(e->cfg.objective, [&](auto O) {
      return with_bool(e->p.vec, [&](auto V) {
        hipLaunchKernelGGL((de_generation_long_kernel<O, V>), grid, block, 0, e->stream, e->p, par, generation,
                           ignore_done);
      });
    }));
    return;
  }
  if (e->group) {
    routed(with_objective(e->cfg.objective, [&](auto O) {
      return with_groups(e->group, [&](auto G) {
        hipLaunchKernelGGL((de_generation_groups_kernel<O, G>), grid, block, 0, e->stream, e->p, par, generation,
                           ignore_done);
      });
    }));
    return;
  }
  routed(with_wave_kernel(e, [&](auto O, auto C, auto V, auto B, auto S) {
    hipLaunchKernelGGL((de_generation_kernel<O, C, V, B, S>), grid, block, 0, e->stream, e->p, par, generation,
                       ignore_done);
  }));
}

// head k and generation k+1 in one launch (de_turn_kernel)
void launch_fused_turn(nlsg_de *e, int par, uint64_t generation) {
  e->p.gen_key = ctr_key(e->p.seed, generation);
  const uint64_t waves = generation_waves(e);
  const dim3 grid(static_cast<unsigned>((waves + 3) / 4 + e->p.ntiles)), block(256);
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &par, &generation};
    launch_module(e, e->rtc.turn, grid.x, args);
    return;
  }
  if (e->group) {
    routed(with_objective(e->cfg.objective, [&](auto O) {
      return with_groups(e->group, [&](auto G) {
        hipLaunchKernelGGL((de_turn_groups_kernel<O, G>), grid, block, 0, e->stream, e->p, par, generation);
      });
    }));
    return;
  }
  routed(with_wave_kernel(e, [&](auto O, auto C, auto V, auto B, auto S) {
    hipLaunchKernelGGL((de_turn_kernel<O, C, V, B, S>), grid, block, 0, e->stream, e->p, par, generation);
  }));
}

// Head of turn k outside a fused turn, one launch. rec_dev == nullptr: one GPU, the head
// finishes the turn; else the shard's exchange record.
void launch_head(nlsg_de *e, double *rec_dev, hipStream_t st) {
  hipLaunchKernelGGL(de_scan_head_kernel, dim3(e->p.ntiles), dim3(256), 0, st, e->p, e->k, rec_dev);
}
void launch_local_summary(nlsg_de *e, double *rec_dev, hipStream_t st) { launch_head(e, rec_dev, st); }
void launch_head_single(nlsg_de *e, hipStream_t st) { launch_head(e, nullptr, st); }

// One turn on one GPU. Serial form: head k, then generation k+1. Overlapped form
// (strategy random): generation k+1 is launched on the main stream as soon as head k-1 is
// done, head k runs on the side stream next to it; if head k fires a stop test the
// generation's output (other buffers) is simply never adopted.
int launch_turn_single(nlsg_de *e) {
  const uint64_t k = e->k;
  if (e->fused) {
    launch_fused_turn(e, static_cast<int>(k & 1), k + 1);
  } else if (!e->overlap) {
    launch_head_single(e, e->stream);
    launch_generation(e, static_cast<int>(k & 1), k + 1);
  } else {
    NLSG_HIP(hipStreamWaitEvent(e->side, e->ev_gen[k & 3], 0));      // population k exists
    launch_head_single(e, e->side);
    NLSG_HIP(hipEventRecord(e->ev_head[k & 3], e->side));
    if (k > 0) NLSG_HIP(hipStreamWaitEvent(e->stream, e->ev_head[(k - 1) & 3], 0));
    launch_generation(e, static_cast<int>(k & 1), k + 1);
    NLSG_HIP(hipEventRecord(e->ev_gen[(k + 1) & 3], e->stream));
  }
  e->k = k + 1;
  return NLSG_OK;
}

// make the main stream wait for everything queued on the side stream
int join_side(nlsg_de *e) {
  if (e->overlap && e->k > 0) NLSG_HIP(hipStreamWaitEvent(e->stream, e->ev_head[(e->k - 1) & 3], 0));
  return NLSG_OK;
}

constexpr double kDeScreenKeep = 0.9;       // share of decided agents below which the screening wave is dropped
constexpr uint64_t kDeScreenProbe = 1024;   // generations after which it is tried again
constexpr uint64_t kDeScreenLook = 8;       // generations a look needs to judge

// the screening wave on or off by what the sampled waves decided since the last look (nlsg_de.screen_adapt)
void adapt_screen(nlsg_de *e, uint32_t stat) {
  if (!e->screen_adapt) return;
  const uint64_t gens = e->k - e->k_seen;
  if (e->p.bound & kDeBoundScreen) {
    if (gens < kDeScreenLook) return;  // (the counters keep running: judged at a later look)
    const uint64_t pairs = (e->p.shard_n + 1) / 2;
    const uint64_t sampled = std::min<uint64_t>(2 * ((pairs + 63) / 64), e->p.shard_n);  // agents of the counting waves
    const double share = static_cast<double>(stat - e->stat_seen) / (static_cast<double>(sampled) * static_cast<double>(gens));
    if (share < kDeScreenKeep) {
      e->p.bound &= ~kDeBoundScreen;
      e->k_off = e->k;
    }
  } else if (e->k - e->k_off >= kDeScreenProbe) {
    e->p.bound |= kDeBoundScreen;
  }
  e->stat_seen = stat;
  e->k_seen = e->k;
}

int read_state(nlsg_de *e, DeState *host) {
  int rc = join_side(e);
  if (rc) return rc;
  hipLaunchKernelGGL(de_settle_kernel, dim3(1), dim3(1), 0, e->stream, e->p, e->k);
  NLSG_HIP(hipMemcpyAsync(host, e->p.state, sizeof(DeState), hipMemcpyDeviceToHost, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  adapt_screen(e, static_cast<uint32_t>(host->pad[0]));
  return NLSG_OK;
}

}  // namespace

extern "C" {

const char *nlsg_last_error(void) { return err_buf(); }
int nlsg_abi_version(void) { return NLSG_ABI_VERSION; }
int nlsg_release_cached(void) {
  pool_release_all();
  return NLSG_OK;
}
uint64_t nlsg_cached_bytes(void) { return pool_idle_bytes(); }
int nlsg_pool_poison(void) { return pool_poison(); }
int nlsg_call_timing(double *ms_out6) {
  if (!ms_out6) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  const CallTiming &t = call_timing();
  ms_out6[0] = t.create_ms;
  ms_out6[1] = t.upload_ms;
  ms_out6[2] = t.init_ms;
  ms_out6[3] = t.iterate_ms;
  ms_out6[4] = t.readback_ms;
  ms_out6[5] = t.destroy_ms;
  return NLSG_OK;
}

int nlsg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int d = 0; d < n; d++) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) == hipSuccess &&
        std::strncmp(prop.gcnArchName, "gfx950", 6) == 0)
      ok++;
  }
  return ok;
}

static int de_create(const nlsg_de_config *cfg, const nlsg_custom_objective *custom, nlsg_de **out);

int nlsg_de_create(const nlsg_de_config *cfg, nlsg_de **out) {
  if (const int rc = builtin_door(cfg, "nlsg_de")) return rc;
  return timed_create([&] { return de_create(cfg, nullptr, out); });
}

int nlsg_de_create_custom(const nlsg_de_config *cfg, const nlsg_custom_objective *obj, nlsg_de **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return timed_create([&] { return de_create(cfg, obj, out); });
}

static int de_create(const nlsg_de_config *cfg, const nlsg_custom_objective *custom, nlsg_de **out) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_de_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_de_config size mismatch (%u vs %zu)",
                cfg->struct_size, sizeof(nlsg_de_config));
  if (cfg->dim < 1) return fail(NLSG_ERR_INVALID_ARG, "dim must be >= 1");
  if (cfg->dim > 1024 && custom && custom->chain == NLSG_CUSTOM_VECTOR)
    return fail(NLSG_ERR_UNSUPPORTED,
                "dim %llu > 1024: a whole-vector objective needs the point in the wave's registers",
                (unsigned long long)cfg->dim);
  if (cfg->dim > 0xffffffffull) return fail(NLSG_ERR_UNSUPPORTED, "dim beyond 2^32");
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->strategy != NLSG_DE_BEST && cfg->strategy != NLSG_DE_RANDOM)
    return fail(NLSG_ERR_INVALID_ARG, "unknown strategy %d", cfg->strategy);
  if (cfg->shard_n < 4 || cfg->shard_lo + cfg->shard_n > cfg->pop)
    return fail(NLSG_ERR_INVALID_ARG,
                "shard [%llu,+%llu) invalid for pop %llu (a shard needs >= 4 agents: three "
                "distinct donors besides the target, nlsolver.h:2331-2355)",
                (unsigned long long)cfg->shard_lo, (unsigned long long)cfg->shard_n,
                (unsigned long long)cfg->pop);
  if (cfg->shard_n > 0xffffffffull)  // donor indices are drawn as 32-bit values inside a shard
    return fail(NLSG_ERR_UNSUPPORTED, "shard_n >= 2^32 agents per engine");
  nlsg_de *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_de", &e)) return rc;
  CreateGuard<nlsg_de> guard(e, nlsg_de_destroy);
  e->cfg = *cfg;
  const uint64_t D = cfg->dim, n = cfg->shard_n;
  e->chunks = row_chunks(D);
  e->long_rows = D > 1024;  // the reference has no limit (nlsolver.h:2302-2477)
  e->group = lane_group_of(D, false);
  if (const char *g = std::getenv("NLSG_DE_GROUPS"))  // A/B switch: 0 = one agent per wave at any D
    if (g[0] == '0') e->group = 0;
  DeParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  DeviceOwner &own = e->own;
  auto alloc = [&](auto **ptr, size_t bytes) { own.alloc(ptr, bytes ? bytes : 8); };
  const size_t rows = n * D * sizeof(double);
  alloc(&p.buf[0], rows);
  alloc(&p.buf[1], rows);
  alloc(&p.scores[0], n * sizeof(double));
  alloc(&p.scores[1], n * sizeof(double));
  alloc(&p.home[0], n);
  alloc(&p.home[1], n);
  alloc(&p.best_x, D * sizeof(double));
  if (cfg->trace) alloc(&p.trace, n * kTraceWords * sizeof(uint64_t));
  if (cfg->trace) alloc(&p.counts, kDeCounts * sizeof(uint64_t));  // the bound's and the screen's path counters (cleared by init)
  alloc(&p.state, sizeof(DeState));
  p.ntiles = static_cast<uint32_t>((n + kTile - 1) / kTile);
  alloc(&p.part, p.ntiles * sizeof(TilePartial));
  own.zeroed(&p.ticket, (kDeScreenStat + 1) * sizeof(uint32_t));  // the head's ticket, and the screen's sampled count
  own.zeroed(&e->zero_dev, 16);
  p.zero = e->zero_dev;
  alloc(&e->x0_dev, D * sizeof(double));
  alloc(&e->rec, (kRecHeader + D) * sizeof(double));
  e->timing_events();
  // Overlapped turns (one GPU, strategy random) are opt-in (NLSG_DE_OVERLAP=1): on MI355X /
  // ROCm 7.2 the two cross-stream event waits per turn cost more (~+3 us) than the 10 us
  // head they hide, measured at pop = 65536 (61.7 vs 58.7 us per turn).
  const char *ov = std::getenv("NLSG_DE_OVERLAP");
  e->overlap = cfg->strategy == NLSG_DE_RANDOM && cfg->shard_n == cfg->pop && ov && ov[0] == '1';
  const char *fu = std::getenv("NLSG_DE_FUSED_TURN");
  e->fused = cfg->strategy == NLSG_DE_RANDOM && cfg->shard_n == cfg->pop && !e->long_rows &&
             !e->overlap && !cfg->trace && !(fu && fu[0] == '0');  // the trace buffer is not double-buffered
  if (e->overlap) {  // (the owner drains the side stream with the engine's own before any block goes back)
    own.stream(&e->side);
    for (int i = 0; i < 4; i++) {
      own.event(&e->ev_gen[i], hipEventDisableTiming);
      own.event(&e->ev_head[i], hipEventDisableTiming);
    }
  }
  if (const int rc = e->setup_status("device allocation failed: %s")) return rc;
  p.pop = cfg->pop;
  p.D = D;
  p.shard_lo = cfg->shard_lo;
  p.shard_n = n;
  p.CR = cfg->CR;
  set_crossover_test(p, cfg->CR);
  p.F = cfg->F;
  p.eps = cfg->eps;
  p.fmul = cfg->minimize ? 1.0 : -1.0;  // f_multiplier, nlsolver.h:2418
  p.max_iter = cfg->max_iter;
  p.best_val_no_change = cfg->best_val_no_change;
  p.seed = cfg->seed;
  p.strategy = cfg->strategy;
  p.vec = (D % 2 == 0) ? 1 : 0;
  // measured at pop 2^20 (1 GiB per buffer): generation 0.892 -> 0.805 ms; at pop 65 536 (both
  // buffers inside the Infinity Cache): 47.8 -> 46.6 us — the streamed stores win at both sizes
  p.stream = 1;
  if (const char *sv = std::getenv("NLSG_DE_STREAM")) p.stream = sv[0] == '1' ? 1 : 0;  // A/B switch
  // reject on the mutant-only terms (DeParams.bound). A/B switches, read here like NLSG_DE_STREAM:
  // NLSG_DE_BOUND=0 off; NLSG_DE_BOUND_CR / NLSG_DE_BOUND_RETRY another threshold / retry period
  // (the sweeps of DESIGN.md section 3)
  double min_cr = kDeBoundMinCR, max_cr = kDeBoundMaxCR;
  uint32_t retry = kDeBoundRetry;
  if (const char *bc = std::getenv("NLSG_DE_BOUND_CR")) {  // from this rate up, CR >= 1 included
    min_cr = std::atof(bc);
    max_cr = HUGE_VAL;
  }
  if (const char *br = std::getenv("NLSG_DE_BOUND_RETRY")) {
    const long r = std::atol(br);
    if (r >= 1 && r <= (1l << 30) && (r & (r - 1)) == 0) retry = static_cast<uint32_t>(r);
  }
  const char *bo = std::getenv("NLSG_DE_BOUND");
  p.bound = !custom && !e->group && !e->long_rows && !(bo && bo[0] == '0') &&
                    de_bound_gate(cfg->objective, cfg->strategy, cfg->minimize != 0, cfg->CR, D, min_cr, max_cr)
                ? 1
                : 0;
  p.retry_mask = retry - 1;
  // the half-row screen on top of the bound (kDeBoundScreen): NLSG_DE_SCREEN=0 off,
  // NLSG_DE_SCREEN_RETRY another retry period (the sweep of DESIGN.md section 3)
  bool screen_on = true;
  uint32_t screen_retry = kDeScreenRetry;
  de_screen_env(std::getenv("NLSG_DE_SCREEN"), std::getenv("NLSG_DE_SCREEN_RETRY"), &screen_on, &screen_retry);
  if (p.bound && screen_on && e->chunks == 1 &&
      de_screen_gate(cfg->objective, cfg->strategy, cfg->minimize != 0, cfg->CR, D, min_cr, max_cr))
    p.bound |= kDeBoundScreen;
  p.screen_retry_mask = screen_retry - 1;
  e->screen_capable = (p.bound & kDeBoundScreen) != 0;
  const char *ad = std::getenv("NLSG_DE_SCREEN_ADAPT");
  e->screen_adapt = e->screen_capable && !(ad && ad[0] == '0');
  if (custom)
    if (const int rc = rtc_build_de(custom, e->long_rows ? 0 : e->chunks, p.vec != 0, e->group, &e->rtc)) return rc;
  *out = guard.release();
  return NLSG_OK;
}

int nlsg_de_destroy(nlsg_de *e) {  // (drained: the engine's stream and the side stream)
  return timed_destroy(e, [&] { comm_detach(e->comm); });
}

int nlsg_de_init(nlsg_de *e, const double *x0_host) {
  if (!e || !x0_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipMemcpyAsync(e->x0_dev, x0_host, e->p.D * sizeof(double), hipMemcpyHostToDevice,
                          e->stream));
  // the host buffer is borrowed for this call only
  NLSG_HIP(hipStreamSynchronize(e->stream));
  int rcj = join_side(e);  // a previous run's last head may still be queued on the side stream
  if (rcj) return rcj;
  hipLaunchKernelGGL(de_reset_state_kernel, dim3(1), dim3(1), 0, e->stream, e->p);
  if (e->p.counts) NLSG_HIP(hipMemsetAsync(e->p.counts, 0, kDeCounts * sizeof(uint64_t), e->stream));
  launch_init(e);
  e->k = 0;
  if (e->screen_capable) {  // a new solve starts with the screening wave; the device's count keeps running
    e->p.bound |= kDeBoundScreen;
    e->k_seen = e->k_off = 0;
  }
  if (e->overlap) NLSG_HIP(hipEventRecord(e->ev_gen[0], e->stream));
  NLSG_HIP(launches_status());
  e->initialised = true;
  return NLSG_OK;
}

int nlsg_de_step(nlsg_de *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  if (e->cfg.shard_n != e->cfg.pop)
    return fail(NLSG_ERR_STATE,
                "sharded engine: use nlsg_de_turn_begin / nlsg_de_turn_end around the exchange");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  for (uint64_t t = 0; t < turns; t++) {
    int rc = launch_turn_single(e);
    if (rc) return rc;
  }
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_status(nlsg_de *e, nlsg_status *out) {
  if (!e || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  DeState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  fill_status(s, out);
  return NLSG_OK;
}

int nlsg_de_best(nlsg_de *e, double *x_host, double *f, uint64_t *index) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  DeState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  if (x_host)
    NLSG_HIP(hipMemcpy(x_host, e->p.best_x, e->p.D * sizeof(double), hipMemcpyDeviceToHost));
  if (f) *f = s.best_f;
  if (index) *index = s.best_id;
  return NLSG_OK;
}

int nlsg_de_download(nlsg_de *e, double *pop_host, double *scores_host, uint64_t *trace_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  DeState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  const uint64_t n = e->p.shard_n, D = e->p.D;
  if (pop_host) {  // rows are spread over both buffers (DeParams.home): gathered, then one copy
    DeviceOwner tmp(e->cfg.device);  // (drains the stream before the block goes back: a failed copy may still be queued)
    tmp.watch(e->stream);
    double *stage = nullptr;
    NLSG_HIP(tmp.take(&stage, n * D * sizeof(double)));
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(n, 65536));
    hipLaunchKernelGGL(de_gather_kernel, dim3(grid), dim3(256), 0, e->stream, e->p, s.parity, stage);
    hipError_t he = hipMemcpyAsync(pop_host, stage, n * D * sizeof(double), hipMemcpyDeviceToHost,
                                   e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = launches_status();
    if (he != hipSuccess) return fail(NLSG_ERR_HIP, "population download failed: %s", hipGetErrorString(he));
  }
  if (scores_host)
    NLSG_HIP(hipMemcpy(scores_host, e->p.scores[s.parity], n * sizeof(double),
                       hipMemcpyDeviceToHost));
  if (trace_host) {
    if (!e->p.trace) return fail(NLSG_ERR_STATE, "engine was created without cfg.trace");
    NLSG_HIP(hipMemcpy(trace_host, e->p.trace, n * kTraceWords * sizeof(uint64_t),
                       hipMemcpyDeviceToHost));
  }
  return NLSG_OK;
}

int nlsg_de_bound_counts(nlsg_de *e, uint64_t *out3) {
  if (!e || !out3) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  if (!e->p.counts) return fail(NLSG_ERR_STATE, "engine was created without cfg.trace");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rc = join_side(e);
  if (rc) return rc;
  NLSG_HIP(hipMemcpyAsync(out3, e->p.counts, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_bound_state(const nlsg_de *e, int32_t *enabled, uint32_t *retry_period) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (enabled) *enabled = e->p.bound != 0;
  if (retry_period) *retry_period = e->p.retry_mask + 1;
  return NLSG_OK;
}

int nlsg_de_bound_gate(int32_t objective, int32_t strategy, int32_t minimize, double CR, uint64_t dim) {
  return de_bound_gate(objective, strategy, minimize != 0, CR, dim) ? 1 : 0;
}

int nlsg_de_screen_counts(nlsg_de *e, uint64_t *out2) {
  if (!e || !out2) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  if (!e->p.counts) return fail(NLSG_ERR_STATE, "engine was created without cfg.trace");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rc = join_side(e);
  if (rc) return rc;
  NLSG_HIP(hipMemcpyAsync(out2, e->p.counts + kDeScreenDecided, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                          e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_screen_state(const nlsg_de *e, int32_t *enabled, uint32_t *retry_period) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (enabled) *enabled = (e->p.bound & kDeBoundScreen) != 0;
  if (retry_period) *retry_period = e->p.screen_retry_mask + 1;
  return NLSG_OK;
}

int nlsg_de_screen_gate(int32_t objective, int32_t strategy, int32_t minimize, double CR, uint64_t dim) {
  return de_screen_gate(objective, strategy, minimize != 0, CR, dim) ? 1 : 0;
}

int nlsg_de_screen_env(int32_t *enabled, uint32_t *retry_period) {
  bool on = true;
  uint32_t period = kDeScreenRetry;
  de_screen_env(std::getenv("NLSG_DE_SCREEN"), std::getenv("NLSG_DE_SCREEN_RETRY"), &on, &period);
  if (enabled) *enabled = on ? 1 : 0;
  if (retry_period) *retry_period = period;
  return NLSG_OK;
}

int nlsg_de_screen_rule(uint32_t selector, uint64_t generation, uint64_t agent, uint32_t bound_retry,
                        uint32_t screen_retry, int32_t outcome, uint32_t *count_after) {
  if (count_after) *count_after = de_screen_count_after((selector >> 2) & 3u, outcome);
  return de_screen_tries(selector, generation, static_cast<uint32_t>(agent), bound_retry - 1, screen_retry - 1) ? 1 : 0;
}

int nlsg_de_upload(nlsg_de *e, const double *pop_host, const double *scores_host) {
  if (!e || !pop_host || !scores_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  DeState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  const uint64_t n = e->p.shard_n, D = e->p.D;
  NLSG_HIP(hipMemcpy(e->p.buf[s.parity], pop_host, n * D * sizeof(double), hipMemcpyHostToDevice));
  NLSG_HIP(hipMemsetAsync(e->p.home[s.parity], s.parity, n, e->stream));  // every row in buf[parity]
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(hipMemcpy(e->p.scores[s.parity], scores_host, n * sizeof(double),
                     hipMemcpyHostToDevice));
  return NLSG_OK;
}

int nlsg_de_minimize(nlsg_de *e, double *x_inout_host, uint64_t poll_every, nlsg_status *out) {
  if (!e || !x_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  PhaseClock clk;
  int rc = nlsg_de_init(e, x_inout_host);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  if (poll_every == 0) poll_every = 32;
  DeState s;
  for (;;) {
    rc = nlsg_de_step(e, poll_every);
    if (rc) return rc;
    rc = read_state(e, &s);
    if (rc) return rc;
    if (s.done) break;
  }
  call_timing().iterate_ms = clk.lap();
  // x = agents[best_id] (nlsolver.h:2444)
  NLSG_HIP(hipMemcpy(x_inout_host, e->p.best_x, e->p.D * sizeof(double), hipMemcpyDeviceToHost));
  if (out) fill_status(s, out);
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_de_time_generation_kernel(nlsg_de *e, uint32_t launches, float *ms_total) {
  if (!e || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  DeState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  rc = time_repeats(e->stream, e->ev0, e->ev1, 1, ms_total, [&]() -> int {
    for (uint32_t k = 0; k < launches; k++)
      launch_generation(e, (s.parity + static_cast<int>(k)) & 1, s.iter + 1 + k, 1);
    return NLSG_OK;
  });
  if (rc) return rc;
  // The population advanced `launches` generations without best scans; the
  // engine must be re-initialised before it is used for a solve again.
  e->initialised = false;
  return NLSG_OK;
}

int nlsg_de_time_turns(nlsg_de *e, uint64_t turns, float *ms_total) {
  if (!e || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  if (e->cfg.shard_n != e->cfg.pop) return fail(NLSG_ERR_STATE, "sharded engine");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rcj = join_side(e);
  if (rcj) return rcj;
  return time_repeats(e->stream, e->ev0, e->ev1, 1, ms_total, [&]() -> int {
    for (uint64_t t = 0; t < turns; t++) {
      int rc = launch_turn_single(e);
      if (rc) return rc;
    }
    return join_side(e);
  });
}

uint64_t nlsg_de_record_doubles(const nlsg_de *e) {
  return e ? static_cast<uint64_t>(kRecHeader) + e->p.D : 0;
}

int nlsg_de_turn_begin(nlsg_de *e, double *send_dev) {
  if (!e || !send_dev) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  launch_local_summary(e, send_dev, e->stream);
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_turn_end(nlsg_de *e, const double *gathered_dev, int32_t world) {
  int rc = nlsg_de_turn_finalize(e, gathered_dev, world);
  if (rc) return rc;
  return nlsg_de_turn_generation(e);
}

int nlsg_de_turn_finalize(nlsg_de *e, const double *gathered_dev, int32_t world) {
  if (!e || !gathered_dev || world < 1) return fail(NLSG_ERR_INVALID_ARG, "bad argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  hipLaunchKernelGGL(de_finalize_kernel, dim3(1), dim3(256), 0, e->stream, e->p, gathered_dev,
                     world, static_cast<uint64_t>(kRecHeader) + e->p.D);
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_turn_generation(nlsg_de *e) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  launch_generation(e, static_cast<int>(e->k & 1), e->k + 1);
  e->k += 1;
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_can_speculate(const nlsg_de *e) {
  return (e && e->cfg.strategy == NLSG_DE_RANDOM) ? 1 : 0;
}

int nlsg_de_comm_attach(nlsg_de *e, const unsigned char *unique_id, int32_t world, int32_t rank) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (e->comm) return fail(NLSG_ERR_STATE, "a communicator is already attached");
  if (static_cast<uint64_t>(world) * e->p.shard_n != e->p.pop ||
      static_cast<uint64_t>(rank) * e->p.shard_n != e->p.shard_lo)
    return fail(NLSG_ERR_INVALID_ARG, "shard [%llu, +%llu) of %llu does not match rank %d of %d",
                (unsigned long long)e->p.shard_lo, (unsigned long long)e->p.shard_n,
                (unsigned long long)e->p.pop, rank, world);
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return comm_attach(&e->comm, unique_id, world, rank, static_cast<uint64_t>(kRecHeader) + e->p.D);
}

int nlsg_de_comm_ranks(nlsg_de *e, int32_t *world_out, int32_t *rank_out) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  return comm_query(e->comm, world_out, rank_out);
}

// `turns` sharded turns without a host round trip.
// Strategy best: head k -> all-gather -> finaliser -> generation k+1, all on the engine's
// stream (nothing can overlap, so no cross-stream dependency is paid for).
// Strategy random: the generation needs the exchange only for the stop flag and writes the
// other buffers, so the whole head of turn k (summary, all-gather, finaliser) runs on the
// collective's stream beside generation k+1; generation k+1 waits for finaliser k-1 only.
// If finaliser k fires a stop test, generation k+1 is never adopted and k+2 is a no-op.
int nlsg_de_step_sharded(nlsg_de *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_init has not been called");
  if (!e->comm) return fail(NLSG_ERR_STATE, "nlsg_de_comm_attach has not been called");
  if (turns == 0) return NLSG_OK;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  ShardComm *c = e->comm;
  const uint64_t stride = static_cast<uint64_t>(kRecHeader) + e->p.D;
  if (e->cfg.strategy != NLSG_DE_RANDOM) {
    for (uint64_t t = 0; t < turns; t++) {
      const uint64_t k = e->k;
      launch_local_summary(e, e->rec, e->stream);
      NLSG_RCCL(rccl_api().AllGather(e->rec, c->gathered, stride, ncclDouble, c->comm, e->stream));
      hipLaunchKernelGGL(de_finalize_kernel, dim3(1), dim3(256), 0, e->stream, e->p, c->gathered,
                         c->world, stride);
      launch_generation(e, static_cast<int>(k & 1), k + 1);
      e->k = k + 1;
    }
    NLSG_HIP(launches_status());
    return NLSG_OK;
  }
  hipStream_t S = e->stream, C = c->stream;  // S is never the hipStreamLegacy handle (borrowed_stream)
  NLSG_HIP(hipEventRecord(c->pop_ready[e->k & 1], S));  // population k exists
  for (uint64_t t = 0; t < turns; t++) {
    const uint64_t k = e->k;
    NLSG_HIP(hipStreamWaitEvent(C, c->pop_ready[k & 1], 0));
    launch_local_summary(e, e->rec, C);
    NLSG_RCCL(rccl_api().AllGather(e->rec, c->gathered, stride, ncclDouble, c->comm, C));
    hipLaunchKernelGGL(de_finalize_kernel, dim3(1), dim3(256), 0, C, e->p, c->gathered, c->world,
                       stride);
    NLSG_HIP(hipEventRecord(c->head_done[k & 1], C));
    if (t > 0) NLSG_HIP(hipStreamWaitEvent(S, c->head_done[(k - 1) & 1], 0));
    launch_generation(e, static_cast<int>(k & 1), k + 1);
    NLSG_HIP(hipEventRecord(c->pop_ready[(k + 1) & 1], S));
    e->k = k + 1;
  }
  // the engine's stream ends behind the last head (status / download / the next call)
  NLSG_HIP(hipStreamWaitEvent(S, c->head_done[(e->k - 1) & 1], 0));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

}  // extern "C"
