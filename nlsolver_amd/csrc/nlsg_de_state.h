// nlsolver_amd/csrc/nlsg_de_state.h — what the keyed DE engines share: the turn engine
// (nlsg_de_kernels.h) and the resident batch engine (nlsg_de_batch_kernels.h) keep the same
// device-resident state per solve and close a turn's head with the same two functions, so a
// solve's counters and stop decisions cannot differ between them.
#pragma once

#ifndef __HIPCC_RTC__
#include <cstdlib>
#endif

#include "nlsg_common.h"

namespace nlsg {

constexpr int kDeMaxTries = 64;       // bounded donor rejection loop

// Device-resident solver state (one per engine).
struct DeState {
  uint64_t best_id;        // global index of the incumbent best
  double best_f;           // its score
  uint64_t iter;           // completed generations
  uint64_t val_no_change;  // nlsolver.h:2439
  uint64_t fcalls;
  double std_err;
  int32_t done;
  int32_t parity;          // population / score buffer holding the current generation
  int32_t pad[2];
};

// Head number k looks at the population after k generations: buffer k & 1. It records
// that position in the state; a head that fires a stop test freezes the state there.
// (P: DeParams, or the resident batch engine's DeBatchParams -- pop, eps and the two limits)
template <typename P>
__device__ inline void head_position(DeState *st, const P &p, uint64_t k) {
  st->iter = k;
  st->fcalls = p.pop * (k + 1);
  st->parity = static_cast<int32_t>(k & 1);
}

// Counters and stop tests shared by the two finalisers (thread 0 only).
template <typename P>
__device__ inline void finish_turn(DeState *st, const P &p, uint64_t bi, double bv,
                                   bool have_best, double se) {
  // not_updated <=> best_id did not move: the strict '<' scan (:2431-2437) can
  // never return to the incumbent once it has left it.
  const bool not_updated = (bi == st->best_id);
  st->val_no_change = not_updated ? st->val_no_change + 1 : 0;  // :2439
  st->best_id = bi;
  if (have_best) st->best_f = bv;
  st->std_err = se;
  if (st->iter >= p.max_iter || st->val_no_change >= p.best_val_no_change ||
      (p.eps > 0 && se < p.eps)) {  // :2441-2443
    st->done = 1;
  }
}

// Host side, at create: the crossover test u01(z) < CR on the draw itself. u01 is monotone in z,
// so there is a smallest z whose uniform reaches CR (none: every draw passes). Fills the
// cr_thresh / cr_all pair of DeParams or DeBatchParams; both engines' kernels read the same test.
template <typename P>
inline void set_crossover_test(P &p, double cr) {
  p.cr_all = 0;
  if (u01(~0ull) < cr) {
    p.cr_all = 1;
    p.cr_thresh = ~0ull;
  } else if (!(u01(0) < cr)) {  // CR <= 0 or NaN: no draw passes
    p.cr_thresh = 0;
  } else {
    uint64_t lo = 0, hi = ~0ull;  // u01(lo) < CR <= u01(hi)
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (u01(mid) < cr) lo = mid; else hi = mid;
    }
    p.cr_thresh = hi;
  }
}

#ifndef __HIPCC_RTC__
// Host side, at create: may the register-resident generation reject on the mutant-only terms
// (DeParams.bound)? Strategy random (the kept coordinates are the agent's own row), minimising
// (fmul == 1: the objective's value is the score), an objective whose terms are >= 0
// (TermsNonNegative), one agent per wave with the row in registers, and a crossover rate at which
// enough terms are known for the bound to decide: at CR 0.9 81 % of Rosenbrock's terms are, at
// CR 0.5 25 %. kDeBoundMinCR and kDeBoundRetry come from the sweeps in DESIGN.md section 3.
// From CR 1 up no coordinate is kept: the plain path reads no own row either, and the bound only
// adds its bookkeeping (measured slower), so the gate closes again there.
constexpr double kDeBoundMinCR = 0.8, kDeBoundMaxCR = 1.0;
constexpr uint32_t kDeBoundRetry = 256;  // a hinted agent tries the bound every R-th generation
inline bool de_bound_gate(int objective, int strategy, bool minimize, double cr, uint64_t dim,
                          double min_cr = kDeBoundMinCR, double max_cr = kDeBoundMaxCR) {
  return (objective == NLSG_OBJ_ROSENBROCK || objective == NLSG_OBJ_SPHERE) &&
         strategy == NLSG_DE_RANDOM && minimize && dim >= 65 && dim <= 1024 && cr >= min_cr &&
         cr < max_cr;
}

// Host side, at create: may the generation screen trials on half a row, two agents per wave
// (kDeBoundScreen)? Wherever the bound may and the row fills one chunk past its half: 65 <= D <=
// 128. Below 65 the packed kernels run; above 128 half a chunk is no longer half a wave's lanes.
// kDeScreenRetry comes from the sweep in DESIGN.md section 3.
constexpr uint32_t kDeScreenRetry = 16;  // an agent with >= 2 misses in a row tries every R-th generation
inline bool de_screen_gate(int objective, int strategy, bool minimize, double cr, uint64_t dim,
                           double min_cr = kDeBoundMinCR, double max_cr = kDeBoundMaxCR) {
  return de_bound_gate(objective, strategy, minimize, cr, dim, min_cr, max_cr) && dim >= 65 && dim <= 128;
}
// The screen's two A/B switches as nlsg_de_create reads them: NLSG_DE_SCREEN=0 off,
// NLSG_DE_SCREEN_RETRY another retry period (a power of two up to 2^30, else ignored).
inline void de_screen_env(const char *screen, const char *retry, bool *on, uint32_t *period) {
  *on = !(screen && screen[0] == '0');
  *period = kDeScreenRetry;
  if (retry) {
    const long r = std::atol(retry);
    if (r >= 1 && r <= (1l << 30) && (r & (r - 1)) == 0) *period = static_cast<uint32_t>(r);
  }
}

// Host side: what nlsg_de_status and nlsg_de_batch_status report of a solve's state
inline void fill_status(const DeState &s, nlsg_status *out) {
  *out = status_row(s.best_f, s.iter, s.fcalls, s.best_id);
  out->val_no_change = s.val_no_change;
  out->std_err = s.std_err;
  out->done = s.done;
}

#endif

// The miss count in bits 2-3 of a selector byte (kDeBoundScreen), as a pure function: does an
// agent with this byte try the screen in `generation`, and what the count becomes. The screening wave
// (de_generation_screen) calls these two, and nlsg_de_screen_rule hands them to the host's tests.
// Written without short-circuits: in the kernel the operands are per-lane values, and a branch on
// one costs more than the mask arithmetic.
//   outcome: 0 the screen decided, 1 it was tried and missed, 2 it was not tried or declined
__host__ __device__ inline bool de_screen_tries(uint32_t sel, uint64_t generation, uint32_t a,
                                                uint32_t bound_retry_mask, uint32_t screen_retry_mask) {
  const uint32_t ga = static_cast<uint32_t>(generation) + a;  // the masks fit 32 bits
  const bool bound_tries = ((sel & 2u) == 0) | ((ga & bound_retry_mask) == 0);
  const uint32_t cnt = (sel >> 2) & 3u;
  return bound_tries & ((cnt < 2) | ((ga & screen_retry_mask) == 0));
}
__host__ __device__ inline uint32_t de_screen_count_after(uint32_t cnt, int outcome) {
  return outcome == 0 ? 0u : outcome == 1 ? (cnt < 3 ? cnt + 1 : 3u) : cnt;
}

}  // namespace nlsg
