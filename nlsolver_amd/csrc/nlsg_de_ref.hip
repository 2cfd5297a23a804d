// nlsolver_amd/csrc/nlsg_de_ref.hip — host side of the reference-order DE engine + C-ABI.
// Batched solves of the reference's own DE (nlsolver.h:2414-2476) on the caller's xorshift states.
#include <vector>

#include "nlsg_de_ref_kernels.h"
#include "nlsg_engine.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_de_ref : EngineBase {
  DeRefRtcKernels rtc;  // objective == NLSG_OBJ_CUSTOM: the kernel hiprtc built for it
  nlsg_de_ref_config cfg;
  DeRefParams p;
  size_t lds = 0;
  uint64_t *jump_dev = nullptr;
};

namespace {
// Work of one launch: about 2^19 draws-and-terms per solve (the population's share of a generation
// is pop x (D + 8)), so that a launch stays in the low milliseconds at the largest tested size.
constexpr uint64_t kDeRefLaunchWork = 1ull << 19;

// M^64 of xorshift128+'s state transition, as a nibble table: entry (j, v) is M^64 applied to the
// state whose nibble j (bits 4j .. 4j+3 of the 128-bit state x0 | x1 << 64) is v and all else 0.
void build_jump_table(uint64_t *out) {
  uint64_t col[128][2];
  for (int k = 0; k < 128; k++) {
    uint64_t a = k < 64 ? 1ull << k : 0, b = k < 64 ? 0 : 1ull << (k - 64);
    for (int i = 0; i < 64; i++) xorshift_step(a, b);
    col[k][0] = a;
    col[k][1] = b;
  }
  for (int j = 0; j < 32; j++)
    for (int v = 0; v < 16; v++) {
      uint64_t r0 = 0, r1 = 0;
      for (int bit = 0; bit < 4; bit++)
        if ((v >> bit) & 1) {
          r0 ^= col[4 * j + bit][0];
          r1 ^= col[4 * j + bit][1];
        }
      out[2 * (16 * j + v)] = r0;
      out[2 * (16 * j + v) + 1] = r1;
    }
}

template <int OBJ>
hipError_t prepare(size_t lds) {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(de_ref_kernel<OBJ>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

void launch(nlsg_de_ref *e) {
  const unsigned grid = static_cast<unsigned>(e->p.batch), block = 64;
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p};
    launch_module_kernel(e->rtc.solve, grid, block, static_cast<unsigned>(e->lds), e->stream, args);
    return;
  }
  // (Rastrigin is rejected at creation)
  routed(with_value<NLSG_OBJ_ROSENBROCK, NLSG_OBJ_SPHERE, NLSG_OBJ_STYBLINSKI_TANG>(e->cfg.objective, [&](auto O) {
    hipLaunchKernelGGL(de_ref_kernel<O>, grid, block, e->lds, e->stream, e->p);
  }));
}

// x0 and the states in, then launches of at most p.gens generations until every solve is done:
// after 1, 2, 4, ... 16 launches the host reads the count of finished solves
int upload(nlsg_de_ref *e, const double *x0, const uint64_t *rng_state) {
  const uint64_t B = e->p.batch;
  std::vector<DeRefCtl> ctl(B);
  for (uint64_t b = 0; b < B; b++) {
    DeRefCtl &c = ctl[b];
    std::memset(&c, 0, sizeof c);
    c.s0 = rng_state[2 * b];
    c.s1 = rng_state[2 * b + 1];
    c.std_err = __builtin_nan("");
  }
  NLSG_HIP(hipMemcpyAsync(e->p.x, x0, B * e->p.D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->p.ctl, ctl.data(), B * sizeof(DeRefCtl), hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemsetAsync(e->p.n_done, 0, sizeof(uint32_t), e->stream));
  return NLSG_OK;
}
int run(nlsg_de_ref *e) {
  const uint64_t B = e->p.batch;
  // every solve is done after at most max_iter + 1 best scans: a bound that catches a stuck engine
  const uint64_t gens = e->p.gens;
  const uint64_t bound = e->cfg.max_iter / gens + 3;
  uint64_t launched = 0;
  for (uint32_t n = 1;; n = n < 16 ? 2 * n : 16) {
    for (uint32_t k = 0; k < n; k++) launch(e);
    launched += n;
    NLSG_HIP(launches_status());
    uint32_t done = 0;
    NLSG_HIP(hipMemcpyAsync(&done, e->p.n_done, sizeof done, hipMemcpyDeviceToHost, e->stream));
    NLSG_HIP(hipStreamSynchronize(e->stream));
    if (done >= B) return NLSG_OK;
    if (launched > bound)
      return fail(NLSG_ERR_STATE, "reference-order DE: %llu of %llu solves unfinished after %llu launches",
                  (unsigned long long)(B - done), (unsigned long long)B, (unsigned long long)launched);
  }
}
}  // namespace

extern "C" {

static int de_ref_create(const nlsg_de_ref_config *cfg, const nlsg_custom_objective *custom, nlsg_de_ref **out);

int nlsg_de_ref_create(const nlsg_de_ref_config *cfg, nlsg_de_ref **out) {
  if (const int rc = builtin_door(cfg, "nlsg_de_ref")) return rc;
  return de_ref_create(cfg, nullptr, out);
}

int nlsg_de_ref_create_custom(const nlsg_de_ref_config *cfg, const nlsg_custom_objective *obj,
                              nlsg_de_ref **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return de_ref_create(cfg, obj, out);
}

static int de_ref_create(const nlsg_de_ref_config *cfg, const nlsg_custom_objective *custom, nlsg_de_ref **out) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_de_ref_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_de_ref_config size mismatch (%u vs %zu)", cfg->struct_size,
                sizeof(nlsg_de_ref_config));
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->objective == NLSG_OBJ_RASTRIGIN || (custom && custom->chain == NLSG_CUSTOM_VECTOR))
    return fail(NLSG_ERR_UNSUPPORTED,
                "reference-order DE needs an objective given by its terms whose arithmetic the device "
                "shares with the reference (not Rastrigin: its cosine is the device's own; not a whole-vector body)");
  if (cfg->strategy != NLSG_DE_BEST && cfg->strategy != NLSG_DE_RANDOM)
    return fail(NLSG_ERR_INVALID_ARG, "unknown strategy %d", cfg->strategy);
  // generate_indices (nlsolver.h:2331-2355) needs three donors besides `fixed`: it never ends below 4
  if (cfg->pop < 4)
    return fail(NLSG_ERR_INVALID_ARG, "pop %llu < 4: the reference's donor pick never terminates",
                (unsigned long long)cfg->pop);
  if (cfg->dim < 1 || cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "dim and batch must be >= 1");
  if (cfg->batch > 0x7fffffffull || cfg->pop > 0x7fffffffull)
    return fail(NLSG_ERR_UNSUPPORTED, "batch and pop must be < 2^31");
  nlsg_de_ref *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_de_ref", &e)) return rc;
  CreateGuard<nlsg_de_ref> guard(e, nlsg_de_ref_destroy);
  e->cfg = *cfg;
  DeRefParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  const uint64_t B = cfg->batch, pop = cfg->pop, D = cfg->dim, L = cfg->log_capacity;
  p.lds_pop = de_ref_lds_bytes(pop, D, true, true) <= kDeRefLdsBudget;
  p.lds_scores = p.lds_pop || de_ref_lds_bytes(pop, D, false, true) <= kDeRefLdsBudget;
  e->lds = de_ref_lds_bytes(pop, D, p.lds_pop, p.lds_scores);
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  own.alloc(&p.x, B * D * 8);
  own.alloc(&p.ctl, B * sizeof(DeRefCtl));
  own.alloc(&p.agents, B * pop * D * 8);
  own.alloc(&p.scores, B * (pop + 8) * 8);
  if (!p.lds_pop) own.alloc(&p.trial, B * (D + 8) * 8);
  own.alloc(&p.n_done, sizeof(uint32_t));
  own.alloc(&e->jump_dev, kDeRefJumpEntries * 16);
  if (L) own.alloc(&p.log_x, B * L * D * 8);
  if (L) own.alloc(&p.log_f, B * L * 8);
  e->timing_events();
  if (he == hipSuccess) {
    std::vector<uint64_t> jt(2 * kDeRefJumpEntries);
    build_jump_table(jt.data());
    he = hipMemcpy(e->jump_dev, jt.data(), kDeRefJumpEntries * 16, hipMemcpyHostToDevice);
  }
  if (he == hipSuccess && !custom) he = prepare<NLSG_OBJ_ROSENBROCK>(e->lds);
  if (he == hipSuccess && !custom) he = prepare<NLSG_OBJ_SPHERE>(e->lds);
  if (he == hipSuccess && !custom) he = prepare<NLSG_OBJ_STYBLINSKI_TANG>(e->lds);
  if (he == hipSuccess && custom) {
    if (const int rc = rtc_build_de_ref(custom, &e->rtc)) return rc;
    if (const int rc = module_kernel_lds(e->rtc.solve, e->lds, "device setup failed: %s")) return rc;
  }
  if (const int rc = e->setup_status()) return rc;
  p.jump = e->jump_dev;
  p.batch = B;
  p.pop = pop;
  p.D = D;
  p.max_iter = cfg->max_iter;
  p.best_val_no_change = cfg->best_val_no_change;
  p.log_cap = L;
  const uint64_t per_gen = pop * (D + 8);
  p.gens = per_gen >= kDeRefLaunchWork ? 1 : kDeRefLaunchWork / per_gen;
  p.CR = cfg->CR;
  p.F = cfg->F;
  p.eps = cfg->eps;
  p.fmul = cfg->minimize ? 1.0 : -1.0;  // f_multiplier, nlsolver.h:2418
  p.strategy = cfg->strategy;
  *out = guard.release();
  return NLSG_OK;
}

int nlsg_de_ref_destroy(nlsg_de_ref *e) { return destroy_engine(e); }

int nlsg_de_ref_minimize(nlsg_de_ref *e, double *x_inout_host, uint64_t *rng_state_inout_host,
                         nlsg_status *status_host) {
  if (!e || !x_inout_host || !rng_state_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const uint64_t B = e->p.batch, D = e->p.D;
  int rc = upload(e, x_inout_host, rng_state_inout_host);
  if (rc) return rc;
  rc = run(e);
  if (rc) return rc;
  std::vector<DeRefCtl> ctl(B);
  NLSG_HIP(hipMemcpy(x_inout_host, e->p.x, B * D * 8, hipMemcpyDeviceToHost));
  NLSG_HIP(hipMemcpy(ctl.data(), e->p.ctl, B * sizeof(DeRefCtl), hipMemcpyDeviceToHost));
  uint64_t first_err = ~0ull;
  for (uint64_t b = 0; b < B; b++) {
    const DeRefCtl &c = ctl[b];
    rng_state_inout_host[2 * b] = c.s0;
    rng_state_inout_host[2 * b + 1] = c.s1;
    if (c.err != kDeRefErrNone && first_err == ~0ull) first_err = b;
    if (status_host) {
      nlsg_status &st = status_host[b] = status_row(c.f_value, c.iter, c.fcalls, c.best_id);
      st.val_no_change = c.val_no_change;
      st.std_err = c.std_err;
      st.done = c.err == kDeRefErrNone ? 1 : 0;
      st.reserved = c.err;
    }
  }
  if (first_err != ~0ull) {
    if (ctl[first_err].err == kDeRefErrCap)
      return fail(NLSG_ERR_UNSUPPORTED,
                  "reference-order DE: solve %llu: the donor pick drew %u times without three distinct donors "
                  "(the reference would not terminate)",
                  (unsigned long long)first_err, kDeRefMaxDonorDraws);
    return fail(NLSG_ERR_UNSUPPORTED,
                "reference-order DE: solve %llu: a draw of exactly 1.0 made generate_index return pop "
                "(the reference reads out of bounds; no result is defined)",
                (unsigned long long)first_err);
  }
  return NLSG_OK;
}

int nlsg_de_ref_log(nlsg_de_ref *e, uint64_t b, double *xs_host, double *fs_host, uint64_t *count) {
  if (!e || !count) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (b >= e->p.batch) return fail(NLSG_ERR_INVALID_ARG, "solve %llu out of range", (unsigned long long)b);
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  DeRefCtl c;
  NLSG_HIP(hipMemcpy(&c, e->p.ctl + b, sizeof c, hipMemcpyDeviceToHost));
  *count = c.log_count;
  const uint64_t L = e->p.log_cap, n = c.log_count < L ? c.log_count : L, D = e->p.D;
  if (n && xs_host) NLSG_HIP(hipMemcpy(xs_host, e->p.log_x + b * L * D, n * D * 8, hipMemcpyDeviceToHost));
  if (n && fs_host) NLSG_HIP(hipMemcpy(fs_host, e->p.log_f + b * L, n * 8, hipMemcpyDeviceToHost));
  return NLSG_OK;
}

int nlsg_de_ref_time_solve(nlsg_de_ref *e, const double *x0_host, const uint64_t *rng_state0_host,
                           uint32_t repeats, float *ms_total) {
  if (!e || !x0_host || !rng_state0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return time_repeats(
      e->stream, e->ev0, e->ev1, repeats, ms_total, [&]() -> int { return run(e); },
      [&]() -> int { return upload(e, x0_host, rng_state0_host); });  // outside the interval
}

int nlsg_de_ref_jump_table(uint64_t *table_host) {
  if (!table_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  build_jump_table(table_host);
  return NLSG_OK;
}

int nlsg_de_ref_pick_donors(const double *draws_host, uint64_t n, uint64_t fixed, uint64_t pop,
                            uint64_t *ids_host, uint64_t *used, int32_t *flag) {
  if (!draws_host || !ids_host || !used || !flag) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  uint64_t pos = 0;
  bool out_of_draws = false;
  *flag = de_ref_donors(fixed, pop,
                        [&]() {
                          if (pos < n) return draws_host[pos++];
                          out_of_draws = true;
                          pos++;
                          return 0.0;
                        },
                        ids_host);
  *used = pos;
  if (out_of_draws) return fail(NLSG_ERR_INVALID_ARG, "the pick needs more than %llu draws", (unsigned long long)n);
  return NLSG_OK;
}

}  // extern "C"
