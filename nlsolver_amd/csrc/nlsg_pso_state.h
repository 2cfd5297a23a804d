// nlsolver_amd/csrc/nlsg_pso_state.h — what the keyed PSO engines share: the turn engine
// (nlsg_pso_kernels.h) and the resident batch engine (nlsg_pso_batch_kernels.h) keep the same
// device-resident state per solve, read the inertia schedule from the same table and close a
// turn's head with the same two functions, so a solve's counters and stop decisions cannot differ
// between them.
#pragma once

#ifndef __HIPCC_RTC__
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#endif

#include "nlsg_common.h"
#include "nlsg_math.h"

namespace nlsg {

struct PsoState {
  double gbest_val;        // swarm_best_value (+inf sentinel)
  uint64_t gbest_idx;      // global particle index of the swarm best
  uint64_t iter;           // completed position updates
  uint64_t val_no_change;
  uint64_t fevals;
  double std_err;
  int32_t done;
  int32_t pending;         // a move ran since the last head (iter++ due)
};

struct PsoParams {
  double *pos, *vel, *pbest_pos;  // [shard_n][D]; vel / pbest_pos only for Vanilla
  double *pbest_val, *cur_val;    // [shard_n]
  double *gbest_x;                // [D]
  const double *lower, *upper;    // [D]
  const double *inertia_tab;      // pow(inertia, k), k < tab_len (Accelerated, :2613)
  PsoState *state;
  TilePartial *part;
  uint32_t *ticket;               // arrival counter of pso_scan_head_kernel's blocks
  const double *zero;
  uint64_t tab_len;
  uint32_t ntiles;
  int32_t tab_fixed;              // the table ends at a fixed point of pow (0, 1, inf): later k repeat it
  uint64_t n, D, shard_lo, shard_n;
  double inertia, cog, soc, eps, fmul;
  uint64_t max_iter, best_val_no_change, seed;
  int32_t type, bounded;
};

// inertia = pow(init_inertia, iter) (:2613) as the host libm computes it: from the table, whose
// last entry repeats for ever when it is a fixed point of the sequence. Only a schedule that is
// still moving after the table's 2^22 entries (|inertia| within 2e-4 of 1, or negative) falls
// back to the device's pow, which is not bit-identical to glibc's.
__device__ inline double pso_inertia_at(const PsoParams &p, uint64_t iter) {
  if (iter < p.tab_len) return p.inertia_tab[iter];
  return p.tab_fixed ? p.inertia_tab[p.tab_len - 1] : pow(p.inertia, static_cast<double>(iter));
}

__device__ inline void pso_apply_pending(PsoState *st) {
  if (st->pending) {
    st->iter += 1;
    st->pending = 0;
  }
}

// update_best_positions' bookkeeping (2727-2740) + stop tests (2599-2600); thread 0
__device__ inline bool pso_finish_turn(PsoState *st, const PsoParams &p, bool have, double bv,
                                       uint64_t gi, double se) {
  const bool update_happened = have && bv < st->gbest_val;  // strict '<' (:2724)
  if (update_happened) {
    st->gbest_val = bv;
    st->gbest_idx = gi;
  }
  st->fevals += p.n;  // :2734
  st->val_no_change = update_happened ? 0 : st->val_no_change + 1;  // :2740, B9 repaired
  st->std_err = se;
  if (st->iter >= p.max_iter || st->val_no_change >= p.best_val_no_change ||
      (p.eps > 0 && se < p.eps)) {
    st->done = 1;
  } else {
    st->pending = 1;
  }
  return update_happened;
}

#ifndef __HIPCC_RTC__
// Host side, at create: the inertia schedule pow(inertia, iter) (:2613) computed with the host
// libm, as the reference does, so the device uses bit-identical values. max_iter + 1 entries
// (guarded against wrapping), or up to the first fixed point of the sequence (0 after underflow,
// 1, inf), which sets *tab_fixed; at most 2^22 entries. Both engines' kernels read it through
// pso_inertia_at.
inline std::vector<double> pso_inertia_table(double inertia, uint64_t max_iter, int32_t *tab_fixed) {
  const uint64_t want = max_iter == ~0ull ? ~0ull : max_iter + 1;
  const uint64_t cap = std::min<uint64_t>(want, 1u << 22);
  std::vector<double> tab;
  tab.reserve(std::min<uint64_t>(cap, 4096));
  *tab_fixed = 0;
  for (uint64_t k = 0; k < cap; k++) {
    tab.push_back(std::pow(inertia, static_cast<double>(k)));
    if (k >= 2 && std::memcmp(&tab[k], &tab[k - 1], 8) == 0 && std::memcmp(&tab[k], &tab[k - 2], 8) == 0 &&
        (tab[k] == 0.0 || tab[k] == 1.0 || std::isinf(tab[k]))) {
      *tab_fixed = 1;
      break;
    }
  }
  return tab;
}

// Host side: what nlsg_pso_status and nlsg_pso_batch_status report of a solve's state
inline void fill_status(const PsoState &s, nlsg_status *out) {
  *out = status_row(s.gbest_val, s.iter, s.fevals, s.gbest_idx);
  out->val_no_change = s.val_no_change;
  out->std_err = s.std_err;
  out->done = s.done;
}
#endif

}  // namespace nlsg
