// nlsolver_amd/csrc/nlsg_de_state.h — what the keyed DE engines share: the turn engine
// (nlsg_de_kernels.h) and the resident batch engine (nlsg_de_batch_kernels.h) keep the same
// device-resident state per solve and close a turn's head with the same two functions, so a
// solve's counters and stop decisions cannot differ between them.
#pragma once

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
#endif

}  // namespace nlsg
