// nlsolver_amd/csrc/nlsg_pso.hip — host side of the PSO engine + its C-ABI
// (include/nlsg_c_api.h). Same structure as nlsg_de.hip. No CPU fallback.
#include <algorithm>
#include <cmath>
#include <vector>

#include "nlsg_comm.h"
#include "nlsg_engine.h"
#include "nlsg_pso_kernels.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_pso : EngineBase {
  nlsg_pso_config cfg;
  PsoParams p;
  double *lower_dev = nullptr, *upper_dev = nullptr, *zero_dev = nullptr, *tab_dev = nullptr;
  ShardLocal *loc = nullptr;
  ShardComm *comm = nullptr;  // set by nlsg_pso_comm_attach
  PsoRtcKernels rtc;          // objective == NLSG_OBJ_CUSTOM: the kernels hiprtc built for it
  double *rec = nullptr;
  int chunks = 0;
  int group = 0;  // lanes per particle when several particles share a wave (D <= 64), else 0
  bool long_rows = false;  // D > 1024: rows streamed in segments (pso_*_long_kernel)
  unsigned move_grid_cap = 2048;  // workgroups of the striding move kernel: 8 per CU (move_blocks_per_cu)
  bool initialised = false;
};

namespace {

// the two PSO types (nlsg_pso_create rejects every other value)
template <typename F>
bool with_type(int type, F &&f) {
  return with_value<NLSG_PSO_VANILLA, NLSG_PSO_ACCELERATED>(type, std::forward<F>(f));
}

void launch_init(nlsg_pso *e) {
  const dim3 grid(static_cast<unsigned>((e->p.shard_n + 3) / 4)), block(256);
  const bool vec = e->p.D % 2 == 0;
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p};
    launch_module_kernel(e->rtc.init, grid.x, 256, 0, e->stream, args);
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    return with_bool(vec, [&](auto V) {
      if (e->long_rows) {  // D > 1024: the segment-streaming kernels, per objective, row alignment and PSO type only
        hipLaunchKernelGGL((pso_init_long_kernel<O, V>), grid, block, 0, e->stream, e->p);
        return true;
      }
      return with_chunks(e->chunks, [&](auto C) {
        hipLaunchKernelGGL((pso_init_kernel<O, C, V>), grid, block, 0, e->stream, e->p);
      });
    });
  }));
}

void launch_move(nlsg_pso *e, int timing, uint64_t iter_ovr) {
  // waves: one per particle, or one per 64 / group particles
  const uint64_t per_wave = e->group ? 64 / e->group : 1;
  const uint64_t waves = (e->p.shard_n + per_wave - 1) / per_wave;
  dim3 grid(static_cast<unsigned>((waves + 3) / 4)), block(256);
  // the one-particle-per-wave kernel strides over the shard: enough workgroups to fill every CU
  // (eight four-wave workgroups each), each wave then keeps the shared rows for all its particles
  // (the Accelerated move, bound by the vector unit; the Vanilla move is bound by HBM and keeps
  // one particle per wave: more rows in flight — striding measured 0.79 -> 0.69 of the roofline)
  const bool vec = e->p.D % 2 == 0;
  const bool accel = e->cfg.type == NLSG_PSO_ACCELERATED;
  if (accel && !e->group && !e->long_rows && grid.x > e->move_grid_cap) grid.x = e->move_grid_cap;
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &timing, &iter_ovr};
    launch_module_kernel(e->rtc.move, grid.x, 256, 0, e->stream, args);
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    return with_type(e->cfg.type, [&](auto T) {
      if (e->group)  // (D <= 64, so never with long rows)
        return with_groups(e->group, [&](auto G) {
          hipLaunchKernelGGL((pso_move_groups_kernel<O, G, T>), grid, block, 0, e->stream, e->p, timing, iter_ovr);
        });
      return with_bool(vec, [&](auto V) {
        if (e->long_rows) {
          hipLaunchKernelGGL((pso_move_long_kernel<O, V, T>), grid, block, 0, e->stream, e->p, timing, iter_ovr);
          return true;
        }
        return with_chunks(e->chunks, [&](auto C) {
          hipLaunchKernelGGL((pso_move_kernel<O, C, V, T>), grid, block, 0, e->stream, e->p, timing, iter_ovr);
        });
      });
    });
  }));
}

// Workgroups per CU of the striding Accelerated move: eight (two more than the six a CU holds at
// once with this kernel's 77 registers). Round 4 tried one exactly resident round instead (4 .. 8
// per CU through this switch: 152 / 151 / 149 / 148 / 147 us per launch) — no tail effect to remove;
// the kernel sits at the vector unit's issue rate (rocprofv3: the unit 91 % busy at the 2.0 GHz the
// chip sustains under fp64 load), so only fewer instructions make it faster.
unsigned move_blocks_per_cu() {
  if (const char *b = std::getenv("NLSG_PSO_MOVE_BLOCKS_PER_CU"))  // A/B switch
    if (std::atoi(b) > 0) return static_cast<unsigned>(std::atoi(b));
  return 8;
}

void launch_local_summary(nlsg_pso *e, double *rec_dev) {
  hipLaunchKernelGGL(pso_scan_partial_kernel, dim3(e->p.ntiles), dim3(256), 0, e->stream, e->p);
  if (!(e->cfg.eps > 0)) {
    hipLaunchKernelGGL(pso_local_kernel, dim3(1), dim3(256), 0, e->stream, e->p, e->loc, rec_dev);
    return;
  }
  hipLaunchKernelGGL(pso_local_kernel, dim3(1), dim3(256), 0, e->stream, e->p, e->loc,
                     static_cast<double *>(nullptr));
  hipLaunchKernelGGL(pso_var_partial_kernel, dim3(e->p.ntiles), dim3(256), 0, e->stream, e->p,
                     &e->loc->mean);
  hipLaunchKernelGGL(pso_var_local_kernel, dim3(1), dim3(256), 0, e->stream, e->p, e->loc);
  hipLaunchKernelGGL(pso_pack_record_kernel, dim3(1), dim3(256), 0, e->stream, e->p, e->loc,
                     rec_dev);
}

void launch_turn_single(nlsg_pso *e) {
  if (e->cfg.eps > 0) {
    launch_local_summary(e, e->rec);
    hipLaunchKernelGGL(pso_finalize_kernel, dim3(1), dim3(256), 0, e->stream, e->p, e->rec, 1,
                       static_cast<uint64_t>(kRecHeader) + e->p.D);
  } else {
    hipLaunchKernelGGL(pso_scan_head_kernel, dim3(e->p.ntiles), dim3(256), 0, e->stream, e->p);
  }
  launch_move(e, 0, 0);
}

int read_state(nlsg_pso *e, PsoState *host) {
  hipLaunchKernelGGL(pso_settle_kernel, dim3(1), dim3(1), 0, e->stream, e->p);
  NLSG_HIP(hipMemcpyAsync(host, e->p.state, sizeof(PsoState), hipMemcpyDeviceToHost, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

}  // namespace

extern "C" {

static int pso_create(const nlsg_pso_config *cfg, const nlsg_custom_objective *custom, nlsg_pso **out);

int nlsg_pso_create(const nlsg_pso_config *cfg, nlsg_pso **out) {
  if (const int rc = builtin_door(cfg, "nlsg_pso")) return rc;
  return timed_create([&] { return pso_create(cfg, nullptr, out); });
}

int nlsg_pso_create_custom(const nlsg_pso_config *cfg, const nlsg_custom_objective *obj,
                           nlsg_pso **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return timed_create([&] { return pso_create(cfg, obj, out); });
}

static int pso_create(const nlsg_pso_config *cfg, const nlsg_custom_objective *custom, nlsg_pso **out) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_pso_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_pso_config size mismatch (%u vs %zu)",
                cfg->struct_size, sizeof(nlsg_pso_config));
  if (cfg->dim < 1) return fail(NLSG_ERR_INVALID_ARG, "dim must be >= 1");
  if (cfg->dim > 1024 && custom && custom->chain == NLSG_CUSTOM_VECTOR)
    return fail(NLSG_ERR_UNSUPPORTED,
                "dim %llu > 1024: a whole-vector objective needs the point in the wave's registers",
                (unsigned long long)cfg->dim);
  if (cfg->dim > 0xffffffffull) return fail(NLSG_ERR_UNSUPPORTED, "dim beyond 2^32");
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->type != NLSG_PSO_VANILLA && cfg->type != NLSG_PSO_ACCELERATED)
    return fail(NLSG_ERR_INVALID_ARG, "unknown PSO type %d", cfg->type);
  if (cfg->shard_n < 1 || cfg->shard_lo + cfg->shard_n > cfg->n_particles)
    return fail(NLSG_ERR_INVALID_ARG, "shard [%llu,+%llu) invalid for %llu particles",
                (unsigned long long)cfg->shard_lo, (unsigned long long)cfg->shard_n,
                (unsigned long long)cfg->n_particles);
  if (cfg->shard_n > (1ull << 32))
    return fail(NLSG_ERR_UNSUPPORTED, "shard_n > 2^32 particles per engine");
  nlsg_pso *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_pso", &e)) return rc;
  CreateGuard<nlsg_pso> guard(e, nlsg_pso_destroy);
  e->cfg = *cfg;
  const uint64_t D = cfg->dim, n = cfg->shard_n;
  e->chunks = row_chunks(D);
  e->long_rows = D > 1024;  // the reference has no limit (nlsolver.h:2498-2742)
  e->group = lane_group_of(D, false);
  if (const char *g = std::getenv("NLSG_PSO_GROUPS"))  // A/B switch: 0 = one particle per wave at any D
    if (g[0] == '0') e->group = 0;
  PsoParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  auto alloc = [&](auto **ptr, size_t bytes) { own.alloc(ptr, bytes ? bytes : 8); };
  const bool vanilla = cfg->type == NLSG_PSO_VANILLA;
  const size_t rows = n * D * sizeof(double);
  alloc(&p.pos, rows);
  if (vanilla) alloc(&p.vel, rows);
  if (vanilla) alloc(&p.pbest_pos, rows);
  alloc(&p.pbest_val, n * sizeof(double));
  alloc(&p.cur_val, n * sizeof(double));
  own.zeroed(&p.gbest_x, D * sizeof(double));
  alloc(&e->lower_dev, D * sizeof(double));
  alloc(&e->upper_dev, D * sizeof(double));
  own.zeroed(&e->zero_dev, 16);
  alloc(&p.state, sizeof(PsoState));
  p.ntiles = static_cast<uint32_t>((n + kTile - 1) / kTile);
  alloc(&p.part, p.ntiles * sizeof(TilePartial));
  own.zeroed(&p.ticket, 8);
  alloc(&e->loc, sizeof(ShardLocal));
  alloc(&e->rec, (kRecHeader + D) * sizeof(double));
  const std::vector<double> tab = pso_inertia_table(cfg->inertia, cfg->max_iter, &p.tab_fixed);
  p.tab_len = tab.size();
  alloc(&e->tab_dev, p.tab_len * sizeof(double));
  if (he == hipSuccess)
    he = hipMemcpy(e->tab_dev, tab.data(), p.tab_len * sizeof(double), hipMemcpyHostToDevice);
  e->timing_events();
  if (const int rc = e->setup_status("device allocation failed: %s")) return rc;
  p.lower = e->lower_dev;
  p.upper = e->upper_dev;
  p.zero = e->zero_dev;
  p.inertia_tab = e->tab_dev;
  p.n = cfg->n_particles;
  p.D = D;
  p.shard_lo = cfg->shard_lo;
  p.shard_n = n;
  p.inertia = cfg->inertia;
  p.cog = cfg->cognitive;
  p.soc = cfg->social;
  p.eps = cfg->eps;
  p.fmul = cfg->minimize ? 1.0 : -1.0;
  p.max_iter = cfg->max_iter;
  p.best_val_no_change = cfg->best_val_no_change;
  p.seed = cfg->seed;
  p.type = cfg->type;
  p.bounded = cfg->bounded ? 1 : 0;
  if (custom)
    if (const int rc = rtc_build_pso(custom, e->long_rows ? 0 : e->chunks, p.D % 2 == 0, cfg->type, e->group, &e->rtc))
      return rc;
  if (cfg->type == NLSG_PSO_ACCELERATED && !e->group && !e->long_rows) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0)
      e->move_grid_cap = move_blocks_per_cu() * static_cast<unsigned>(cus);
  }
  *out = guard.release();
  return NLSG_OK;
}

int nlsg_pso_destroy(nlsg_pso *e) {
  return timed_destroy(e, [&] { comm_detach(e->comm); });
}

int nlsg_pso_init(nlsg_pso *e, const double *lower_host, const double *upper_host) {
  if (!e || !lower_host || !upper_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const size_t bytes = e->p.D * sizeof(double);
  NLSG_HIP(hipMemcpyAsync(e->lower_dev, lower_host, bytes, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->upper_dev, upper_host, bytes, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));  // host buffers are borrowed for this call only
  hipLaunchKernelGGL(pso_reset_state_kernel, dim3(1), dim3(1), 0, e->stream, e->p);
  launch_init(e);
  NLSG_HIP(launches_status());
  e->initialised = true;
  return NLSG_OK;
}

int nlsg_pso_step(nlsg_pso *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  if (e->cfg.shard_n != e->cfg.n_particles)
    return fail(NLSG_ERR_STATE,
                "sharded engine: use nlsg_pso_turn_begin / nlsg_pso_turn_end around the exchange");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  for (uint64_t t = 0; t < turns; t++) launch_turn_single(e);
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_pso_status(nlsg_pso *e, nlsg_status *out) {
  if (!e || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PsoState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  fill_status(s, out);
  return NLSG_OK;
}

int nlsg_pso_best(nlsg_pso *e, double *x_host, double *f, uint64_t *index) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PsoState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  if (x_host)
    NLSG_HIP(hipMemcpy(x_host, e->p.gbest_x, e->p.D * sizeof(double), hipMemcpyDeviceToHost));
  if (f) *f = s.gbest_val;
  if (index) *index = s.gbest_idx;
  return NLSG_OK;
}

int nlsg_pso_download(nlsg_pso *e, double *pos_host, double *vel_host, double *pbest_val_host,
                      double *cur_val_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  const uint64_t n = e->p.shard_n, D = e->p.D;
  if (pos_host) NLSG_HIP(hipMemcpy(pos_host, e->p.pos, n * D * sizeof(double), hipMemcpyDeviceToHost));
  if (vel_host) {
    if (!e->p.vel) return fail(NLSG_ERR_STATE, "velocities exist only for Vanilla PSO");
    NLSG_HIP(hipMemcpy(vel_host, e->p.vel, n * D * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (pbest_val_host)
    NLSG_HIP(hipMemcpy(pbest_val_host, e->p.pbest_val, n * sizeof(double), hipMemcpyDeviceToHost));
  if (cur_val_host)
    NLSG_HIP(hipMemcpy(cur_val_host, e->p.cur_val, n * sizeof(double), hipMemcpyDeviceToHost));
  return NLSG_OK;
}

int nlsg_pso_minimize(nlsg_pso *e, double *x_out_host, const double *lower_host,
                      const double *upper_host, uint64_t poll_every, nlsg_status *out) {
  if (!e || !x_out_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  PhaseClock clk;
  int rc = nlsg_pso_init(e, lower_host, upper_host);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  if (poll_every == 0) poll_every = 32;
  PsoState s;
  for (;;) {
    rc = nlsg_pso_step(e, poll_every);
    if (rc) return rc;
    rc = read_state(e, &s);
    if (rc) return rc;
    if (s.done) break;
  }
  call_timing().iterate_ms = clk.lap();
  // x = swarm_best_position (nlsolver.h:2601)
  NLSG_HIP(hipMemcpy(x_out_host, e->p.gbest_x, e->p.D * sizeof(double), hipMemcpyDeviceToHost));
  if (out) fill_status(s, out);
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_pso_time_move_kernel(nlsg_pso *e, uint32_t launches, float *ms_total) {
  if (!e || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PsoState s;
  int rc = read_state(e, &s);
  if (rc) return rc;
  rc = time_repeats(e->stream, e->ev0, e->ev1, 1, ms_total, [&]() -> int {
    for (uint32_t k = 0; k < launches; k++) launch_move(e, 1, s.iter + k);
    return NLSG_OK;
  });
  if (rc) return rc;
  e->initialised = false;  // the swarm moved without best bookkeeping: re-init before solving
  return NLSG_OK;
}

uint64_t nlsg_pso_record_doubles(const nlsg_pso *e) {
  return e ? static_cast<uint64_t>(kRecHeader) + e->p.D : 0;
}

int nlsg_pso_turn_begin(nlsg_pso *e, double *send_dev) {
  if (!e || !send_dev) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  launch_local_summary(e, send_dev);
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_pso_turn_end(nlsg_pso *e, const double *gathered_dev, int32_t world) {
  if (!e || !gathered_dev || world < 1) return fail(NLSG_ERR_INVALID_ARG, "bad argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  hipLaunchKernelGGL(pso_finalize_kernel, dim3(1), dim3(256), 0, e->stream, e->p, gathered_dev,
                     world, static_cast<uint64_t>(kRecHeader) + e->p.D);
  launch_move(e, 0, 0);
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_pso_comm_attach(nlsg_pso *e, const unsigned char *unique_id, int32_t world, int32_t rank) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (e->comm) return fail(NLSG_ERR_STATE, "a communicator is already attached");
  if (static_cast<uint64_t>(world) * e->p.shard_n != e->p.n ||
      static_cast<uint64_t>(rank) * e->p.shard_n != e->p.shard_lo)
    return fail(NLSG_ERR_INVALID_ARG, "shard [%llu, +%llu) of %llu does not match rank %d of %d",
                (unsigned long long)e->p.shard_lo, (unsigned long long)e->p.shard_n,
                (unsigned long long)e->p.n, rank, world);
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return comm_attach(&e->comm, unique_id, world, rank, static_cast<uint64_t>(kRecHeader) + e->p.D);
}

int nlsg_pso_comm_ranks(nlsg_pso *e, int32_t *world_out, int32_t *rank_out) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  return comm_query(e->comm, world_out, rank_out);
}

// `turns` sharded turns without a host round trip. The move needs the exchanged swarm best, so
// nothing can run beside the collective: summary -> all-gather -> finaliser -> move, all on the
// engine's stream (no cross-stream dependency to pay for).
int nlsg_pso_step_sharded(nlsg_pso *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_init has not been called");
  if (!e->comm) return fail(NLSG_ERR_STATE, "nlsg_pso_comm_attach has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  ShardComm *c = e->comm;
  const uint64_t stride = static_cast<uint64_t>(kRecHeader) + e->p.D;
  for (uint64_t t = 0; t < turns; t++) {
    launch_local_summary(e, e->rec);
    NLSG_RCCL(rccl_api().AllGather(e->rec, c->gathered, stride, ncclDouble, c->comm, e->stream));
    hipLaunchKernelGGL(pso_finalize_kernel, dim3(1), dim3(256), 0, e->stream, e->p, c->gathered,
                       c->world, stride);
    launch_move(e, 0, 0);
  }
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

}  // extern "C"
