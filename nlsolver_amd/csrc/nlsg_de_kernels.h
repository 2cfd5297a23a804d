// nlsolver_amd/csrc/nlsg_de_kernels.h — gfx950 kernels of the DE engine.
//
// Replaces the loops of DE::solve (nlsolver.h:2414-2476):
//   de_init_kernel        init_agents + initial scoring      (2315-2323, 2423-2425)
//   de_generation_kernel  generate_indices + propose_new_agent + f() + selection (2449-2472)
//   de_scan_head_kernel   best scan, std_err (2037-2052) when eps > 0 can decide, no-change
//                         counter, stop tests (2429-2447) -- or the shard's exchange record
//   de_turn_kernel        head k and generation k+1 in one launch (strategy random)
//   de_generation_groups_kernel / de_turn_groups_kernel   the same for D <= 64: several agents
//                         per wave, one per group of lanes
//   de_finalize_kernel    the head's decisions from the records of all shards
//
// Data layout in HBM: population row-major [shard_n][D] fp64, two buffers; a per-agent
// selector (DeParams.home) says which one holds the row of the generation being read, and
// only accepted trials are stored (into the other one). Scores [shard_n] fp64, double-buffered.
// Mapping (D > 64): one wave64 per agent; lane l holds elements c*128 + 2l, +1 of each
// 128-element chunk c, so every wave-level load/store is one contiguous 1 KiB
// burst (global_load_dwordx4 / global_store_dwordx4) when D is even. One agent
// per wave and 4 agents per 256-thread block, dispatched dynamically: measured
// 10-13 % faster at pop = 2^20 than persistent grid-stride waves (same device,
// same run), which lose to load imbalance between CUs (DESIGN.md §DE kernel).
#pragma once

#include "nlsg_common.h"
#include "nlsg_de_state.h"

namespace nlsg {

constexpr int kTraceWords = 5;        // r1, r2, r3, jrand, accept

// Where a row lives. A synchronous generation reads generation k and writes k + 1, but a row is
// only stored when its trial is accepted: home[par][j] (0 or 1) says which of buf[0] / buf[1]
// holds agent j's row in the generation read from parity par. A generation that reads parity
// par stores an accepted trial of agent a into buf[home[par][a] ^ 1] and sets
// home[par ^ 1][a] = home[par][a] ^ 1; a rejected one stores nothing and carries the selector
// over (home[par ^ 1][a] = home[par][a]). Like `scores`, the selectors are double-buffered by
// parity. Why the slot written is free: during generation k + 1 and head k, every reader
// (donor gathers, the own / non-crossed row, the head's best row) goes through home_k, so
// nobody reads buf[1 - home_k[a]] row a; and a speculative generation that a stop test
// discards leaves home_k, scores_k and the rows they point to untouched: it is never adopted,
// exactly as when every row was copied into the other buffer.
//
// Bit 1 of a selector byte is not part of the selector: the register-resident generation
// (de_fetch_agent / de_process_agent, 65 <= D <= 1024) keeps its per-agent bound hint there
// (DeParams.bound below). Every reader of a selector therefore takes `& 1`: de_row, the `row`
// lambdas of de_fetch_agent and of the packed generation, DeAgent.home, de_gather_kernel and the
// head's best row (both through de_row). Init stores 0 and upload's memset stores the parity
// (0 or 1), so both clear the hint. Bits 2-3 are the screen's miss count (kDeBoundScreen), kept by
// the screening wave alone and carried through select() as DeAgent.miss; the same readers ignore them.
struct DeParams {
  double *buf[2];      // population ping-pong, rows addressed through `home`
  double *scores[2];   // [shard_n] each, ping-pong with the population: a generation reads
                       // scores[src] and writes scores[src^1], so it never destroys the
                       // state it started from (it may run speculatively, see nlsg_de.hip)
  uint8_t *home[2];    // [shard_n] each: the buffer holding each agent's row (see above)
  double *best_x;      // [D] row of the incumbent best (valid after a scan)
  uint64_t *trace;     // [shard_n*5] or nullptr
  DeState *state;
  TilePartial *part;   // [ntiles] written by de_scan_partial_kernel
  uint32_t *ticket;    // arrival counter of de_scan_head_kernel's blocks (zero between launches)
  const double *zero;  // 16 bytes of zeros: source for lanes past the row end
  uint32_t ntiles;
  uint32_t stream;     // the new generation's rows are stored nontemporally: they are read again a
                       // whole generation later, the caches are better spent on the rows being
                       // gathered (NLSG_DE_STREAM=0 is the A/B switch)
  uint64_t pop, D, shard_lo, shard_n;
  double CR, F, eps, fmul;
  uint64_t max_iter, best_val_no_change, seed;
  int32_t strategy;
  int32_t vec;         // rows are 16-byte aligned (D even)
  // set by the host (nlsg_de.hip): wave-uniform values every wave of a launch would recompute
  uint64_t gen_key;    // ctr_key(seed, generation) of the generation being launched
  uint64_t cr_thresh;  // u01(z) < CR  <=>  z < cr_thresh (u01 is monotone in z): the crossover
  int32_t cr_all;      // test on the draw's bits; cr_all: CR > 1, every draw passes
  // Reject on the mutant-only terms (host-set, wave-uniform; de_bound_gate in nlsg_de_state.h).
  // For an objective whose computed terms are all >= 0 (TermsNonNegative), the lane tree over the
  // terms whose coordinates all come from the mutant, with +0.0 in place of every other term, is
  // a lower bound of the trial's computed score bit for bit: round-to-nearest addition is
  // monotone in each operand. bound >= old_score therefore implies !(score < old_score), and the
  // trial is rejected without the agent's own row ever being read (a rejected trial stores
  // old_score, not its own score: nothing observable changes). An agent whose bound did not
  // decide carries a hint (bit 1 of its selector byte, see above) and takes the plain path --
  // own row loaded with the donors, one evaluation -- except in the generations where
  // (generation + a) & retry_mask == 0, when it tries the bound again. The path taken never
  // changes an output.
  int32_t bound;
  uint64_t *counts;    // cfg.trace only, else nullptr: [kDeCounts] agents per path (kDeBound*, kDeScreen*), for tests
  uint32_t retry_mask; // R - 1, R a power of two
  // Half-row reject screen (host-set, wave-uniform; de_screen_gate in nlsg_de_state.h; 65 <= D <= 128
  // with `bound` set). The same lane tree with +0.0 in place of every term that touches a coordinate
  // >= 64 is <= the bound above, hence <= the score, by the same argument: screen >= old_score
  // rejects the trial on 512 B of each donor row and 64 crossover draws. Half a row is 32 lanes, so
  // a wave of the generation screens two agents at a time, one per half-wave (de_generation_screen); an agent the
  // screen does not decide goes through de_fetch_agent / de_process_agent unchanged. Bits 2-3 of an
  // agent's selector byte count its consecutive screen misses (saturating at 3; a decision clears
  // them): from two misses on the agent skips the screen except in the generations where
  // (generation + a) & screen_retry_mask == 0. The screen only ever rejects, and only in a
  // generation in which the agent tries the bound; no output depends on it.
  // The flag is bit 1 of `bound` (kDeBoundScreen; the kernels only test `bound` for non-zero): the
  // argument block keeps its size, and the engines that do not screen their exact launches.
  uint32_t screen_retry_mask;  // R - 1, R a power of two
};
constexpr int32_t kDeBoundScreen = 2;
constexpr int kDeScreenStat = 32;  // word of the `ticket` block, a cache line away from the head's ticket

// DeParams.counts: the bound decided / it did not and the trial was rejected / it did not (or every
// coordinate came from the mutant: the bound is the score) and the trial was accepted; then the
// screen's own two: it decided (counted under kDeBoundDecided as well: what the screen rejects the
// bound rejects) / it was tried and did not
constexpr int kDeBoundDecided = 0, kDeBoundRejected = 1, kDeBoundAccepted = 2;
constexpr int kDeScreenDecided = 3, kDeScreenMissed = 4, kDeCounts = 5;

// agent `local`'s row in buffer h (a home selector value; the select keeps DeParams out of
// scratch and any stray byte inside the two buffers)
__device__ inline double *de_row(const DeParams &p, uint32_t h, uint64_t local) {
  return ((h & 1u) ? p.buf[1] : p.buf[0]) + local * p.D;
}

// ---- generation 0 ----------------------------------------------------------
template <int OBJ, int CHUNKS, bool VEC>
__global__ __launch_bounds__(256) void de_init_kernel(DeParams p, const double *__restrict__ x0) {
  const uint64_t a = static_cast<uint64_t>(blockIdx.x) * 4 +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (a >= p.shard_n) return;
  const int lane = lane_id();
  const uint64_t ka = ctr_key(ctr_key(p.seed, 0), p.shard_lo + a);
  double xv[CHUNKS][2];
#pragma unroll
  for (int c = 0; c < CHUNKS; c++) {
    const uint64_t e0 = static_cast<uint64_t>(c) * 128 + 2 * static_cast<uint64_t>(lane);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint64_t e = e0 + k;
      // generate_sequence, nlsolver.h:2309: (u - 0.5) * offset[i]
      xv[c][k] = (e < p.D) ? (u01(ctr_key(ka, e)) - 0.5) * x0[e] : 0.0;
    }
  }
  store_row<CHUNKS, VEC>(p.buf[0] + a * p.D, p.D, xv);
  const double f = p.fmul * wave_objective<OBJ, CHUNKS>(xv, p.D);  // :2423-2425
  if (lane == 0) {
    p.scores[0][a] = f;
    p.home[0][a] = 0;
  }
}

__global__ void de_reset_state_kernel(DeParams p) {
  DeState *s = p.state;
  s->best_id = 0;  // "best_id = 0" (:2428), a GLOBAL index on every rank
  s->best_f = 0.0;
  s->iter = 0;
  s->val_no_change = 0;
  s->fcalls = p.pop;
  s->std_err = __builtin_nan("");
  s->done = 0;
  s->parity = 0;
}

// ---- one generation ----------------------------------------------------------
// Everything a wave needs about one agent before it can build the trial: donor indices
// (wave-uniform), the crossover mask, the rows and the old score. All row loads of a fetch are
// issued back to back.
template <int CHUNKS>
struct DeAgent {
  uint64_t a, ka, r0, r1, r2, jrand;
  uint32_t home;          // home[par][a] & 1: the buffer holding the agent's row
  uint32_t hint;          // home[par][a] & 2: the bound did not decide this agent's last try
  uint32_t miss;          // bits 2-3 of the selector byte to leave behind (the screening wave sets it, else 0)
  bool bound;            // wave-uniform: this generation tries the bound, `keep` is not loaded yet
  uint64_t cross[CHUNKS][2];  // lane masks (lane_bit): the trial takes the mutant here (crossover draw or jrand)
  double keep[CHUNKS][2], d1[CHUNKS][2], d2[CHUNKS][2], d3[CHUNKS][2];
  double old_score;
};

// load_row where the trial keeps the old coordinate only: a lane whose coordinates all take the
// mutant (`skip`, lane masks) reads the zero pad instead (at CR 0.9 about 4 lanes in 5); `none` (wave-uniform):
// every lane does
template <int CHUNKS, bool VEC>
__device__ inline void load_row_kept(const double *__restrict__ row, uint64_t D,
                                     const double *__restrict__ zero, const uint64_t (&skip)[CHUNKS][2],
                                     double (&v)[CHUNKS][2], bool none = false) {
  const int lane = lane_id();
  const uint32_t n = none ? 0u : limit32(D);  // `none` folded into the wave-uniform limit
#pragma unroll
  for (int c = 0; c < CHUNKS; c++) {
    const uint32_t e0 = static_cast<uint32_t>(c) * 128 + 2 * static_cast<uint32_t>(lane);
    if (VEC) {
      const double *src = (e0 < n && !lane_bit(skip[c][0] & skip[c][1])) ? row + e0 : zero;
      const double2 t = *reinterpret_cast<const double2 *>(src);
      v[c][0] = t.x;
      v[c][1] = t.y;
    } else {
      v[c][0] = *((e0 < n && !lane_bit(skip[c][0])) ? row + e0 : zero);
      v[c][1] = *((e0 + 1 < n && !lane_bit(skip[c][1])) ? row + e0 + 1 : zero);
    }
  }
}

template <bool BOUND, int CHUNKS, bool VEC>
__device__ inline void de_fetch_agent(const DeParams &p, int par, uint64_t kg, uint64_t generation,
                                      uint64_t best_id, uint64_t a, DeAgent<CHUNKS> &c) {
  const uint64_t D = p.D;
  const uint64_t ga = p.shard_lo + a;  // the global agent id keys the RNG
  // the agent's key and its wave-uniform draws are computed on the vector unit (see on_valu):
  // lane L takes draw D + L of the agent's stream — lane 0 the crossover's jrand (:2364), lane
  // 1 + k donor candidate k — so the donor loop below only picks lanes
  const uint64_t ka = ctr_key(kg, ga);  // wave-uniform: on the scalar unit (the vector unit is
                                         // the busier one here: 68 % against 35 % at pop = 65 536)
  const int lane = lane_id();
  // generate_index (:2325-2329), size_t(u * max): shard sizes and D fit 32 bits, so the
  // conversion is the one-instruction 32-bit one (same truncation)
  const uint32_t lim = static_cast<uint32_t>(lane == 0 ? p.D : p.shard_n);
  // (draw D + lane: its index + 1 fits 32 bits like D, golden_times)
  const uint32_t idx = static_cast<uint32_t>(
      u01(mix64(ka + golden_times(static_cast<uint32_t>(p.D) + static_cast<uint32_t>(lane) + 1u))) *
      static_cast<double>(lim));
  const uint64_t drawn = idx >= lim ? lim - 1 : idx;  // the u == 1.0 corner clamped (B10)
  // Home selectors, loaded here so that their latency hides behind the donor picks: lane 0 the
  // agent's own, lanes 1..7 those of donor candidates 0..6 (a pick past candidate 6 -- tiny
  // shards -- takes a scalar load below). The other lanes repeat lane 0's address: one load of
  // every candidate would touch 64 cache lines per wave, more than the rows themselves.
  const uint8_t *__restrict__ hp = p.home[par];
  const uint32_t hsel = hp[(lane >= 1 && lane < 8) ? drawn : a];
  c.jrand = readlane64(drawn, 0);  // :2364
  // the crossover mask of propose_new_agent (nlsolver.h:2357-2375), before any row load: the
  // non-crossed source is read only where the trial keeps it.
  // ctr_key(ka, e) = mix64(ka + G (e + 1)), e + 1 = (2 lane + 1) + (128 ch + k): one 64-bit
  // multiply per lane, the rest are compile-time constants; u01(z) < CR is decided on the
  // draw's bits (cr_thresh: the smallest z whose uniform is >= CR)
  const uint64_t ka_lane = ka + golden_times(2 * static_cast<uint32_t>(lane) + 1u);
  const uint32_t jrand32 = static_cast<uint32_t>(c.jrand);  // < D <= 1024
  const uint64_t cr_all = p.cr_all ? ~0ull : 0ull;
#pragma unroll
  for (int ch = 0; ch < CHUNKS; ch++) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint32_t e = static_cast<uint32_t>(ch) * 128 + 2 * static_cast<uint32_t>(lane) + k;
      const uint64_t z = mix64(ka_lane + kGolden * static_cast<uint64_t>(128 * ch + k));
      c.cross[ch][k] = __ballot(z < p.cr_thresh) | cr_all | __ballot(e == jrand32);
    }
  }
  // generate_indices (nlsolver.h:2331-2355): three distinct donors != fixed,
  // by rejection, drawn inside this engine's shard. Wave-uniform (scalar) code.
  const uint64_t fixed = (p.strategy == NLSG_DE_RANDOM) ? ga : best_id;  // :2451-2457
  // Candidate k is the draw of lane k + 1: the first three lanes (in order) whose candidate
  // differs from `fixed` and from the picks before it are found with three wave-wide compares
  // and find-first-set — the rejection loop as a handful of instructions instead of a scalar
  // loop of branches (this kernel was bound by the CU's scalar issue at pop = 65 536: ~400 scalar
  // instructions per wave against ~320 vector ones). Same candidates in the same order.
  const uint64_t cand_v = p.shard_lo + drawn;
  constexpr uint64_t top = 1ull << 63;
  const uint64_t m0 = __ballot(cand_v != fixed) & ~1ull;  // lane 0 holds jrand
  const int i0 = __builtin_ctzll(m0 | top);
  uint64_t r0 = readlane64(cand_v, i0);
  const uint64_t m1 = m0 & __ballot(cand_v != r0) & ((~0ull << i0) << 1);
  const int i1 = __builtin_ctzll(m1 | top);
  uint64_t r1 = readlane64(cand_v, i1);
  const uint64_t m2 = m1 & __ballot(cand_v != r1) & ((~0ull << i1) << 1);
  const int i2 = __builtin_ctzll(m2 | top);
  uint64_t r2 = readlane64(cand_v, i2);
  const bool slow = m0 == 0 || m1 == 0 || m2 == 0;
  if (slow) {  // fewer than three among 63 candidates (tiny shards): the literal loop, from the start
    r0 = r1 = r2 = ~0ull;
    int have = 0;
    for (int k = 0; k < kDeMaxTries && have < 3; k++) {
      // (candidate 63 has no lane: after 61 rejections it is drawn the slow way)
      const uint64_t cand =
          p.shard_lo + (k < 63 ? readlane64(drawn, k + 1)
                               : clamp_index(u01(ctr_key(ka, p.D + 1 + k)), p.shard_n));
      const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
      if (!used) {
        if (have == 0) r0 = cand;
        else if (have == 1) r1 = cand;
        else r2 = cand;
        have++;
      }
    }
    for (uint64_t cand = p.shard_lo; have < 3; cand++) {  // fallback: lowest unused
      const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
      if (!used) {
        if (have == 0) r0 = cand;
        else if (have == 1) r1 = cand;
        else r2 = cand;
        have++;
      }
    }
  }
  // candidate i - 1 sits in lane i: the selector is read from lane min(i, 7) without a branch, and
  // one wave-uniform branch for all three donors replaces it by a load where that lane is not the
  // candidate's (a pick past candidate 6, or the literal loop: tiny shards). Without the literal
  // loop i0 < i1 < i2, so i2 decides for the three. The loaded bytes go back to scalar registers:
  // the buffer select below then stays on the scalar unit.
  auto sel_lane = [&](int i) {
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hsel), i < 7 ? i : 7));
  };
  uint32_t h0 = sel_lane(i0), h1 = sel_lane(i1), h2 = sel_lane(i2);
  if (slow || i2 >= 8) {
    auto sel_load = [&](uint64_t r) {
      return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(hp[r - p.shard_lo])));
    };
    h0 = sel_load(r0);
    h1 = sel_load(r1);
    h2 = sel_load(r2);
  }
  c.a = a;
  c.ka = ka;
  c.r0 = r0;
  c.r1 = r1;
  c.r2 = r2;
  const uint32_t hraw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hsel), 0));
  c.home = hraw & 1u;
  c.hint = 0;
  c.miss = 0;
  c.bound = false;
  if constexpr (BOUND) {
    c.hint = hraw & 2u;
    c.bound = p.bound && (c.hint == 0 || ((generation + a) & p.retry_mask) == 0);
  }
  // rows: 3 donors and the non-crossed source -- the agent's own row for strategy random, the
  // row of best_id (L2-resident) for strategy best -- where the trial keeps it
  // (shard-local indices and D fit 32 bits: one scalar multiply pair per row offset)
  // Both buffer bases are taken out of the kernel arguments once and the selector -- in a scalar
  // register -- selects between the two values: left to itself the compiler loads the base from
  // the argument block at an offset made from the selector, a dependent scalar load per row behind
  // a detour through the vector unit.
  const uint32_t d32 = static_cast<uint32_t>(p.D);
  // (global address space spelled out: behind the asm the compiler no longer sees a kernel argument)
  typedef double __attribute__((address_space(1))) global_double;
  global_double *b0 = (global_double *)p.buf[0], *b1 = (global_double *)p.buf[1];
  asm("" : "+s"(b0), "+s"(b1));
  auto row = [&](uint32_t h, uint64_t local) {
    return (double *)((h & 1u) ? b1 : b0) + static_cast<uint64_t>(static_cast<uint32_t>(local)) * d32;
  };
  load_row<CHUNKS, VEC>(row(h0, r0 - p.shard_lo), D, p.zero, c.d1);
  load_row<CHUNKS, VEC>(row(h1, r1 - p.shard_lo), D, p.zero, c.d2);
  load_row<CHUNKS, VEC>(row(h2, r2 - p.shard_lo), D, p.zero, c.d3);
  // (a wave that tries the bound reads the own row only if the bound does not decide: here every
  // lane of it reads the zero pad, one line, and the code stays free of a branch)
  load_row_kept<CHUNKS, VEC>(p.strategy == NLSG_DE_RANDOM ? row(c.home, a) : p.best_x, D, p.zero,
                             c.cross, c.keep, BOUND && c.bound);
  c.old_score = p.scores[par][a];
}

template <int OBJ, int CHUNKS, bool VEC, bool BOUND>
__device__ inline void de_process_agent(const DeParams &p, int par, DeAgent<CHUNKS> &c) {
  static_assert(!BOUND || TermsNonNegative<OBJ>::value, "the bound needs terms >= 0");
  const int lane = lane_id();
  const uint64_t D = p.D;
  // selection (:2466) and what a generation leaves behind; `hint` is 0 or 2 (DeParams.bound)
  auto select = [&](bool accept, double score, const double (&trial)[CHUNKS][2], uint32_t hint) {
    if (accept) {  // a rejected trial stores nothing: the row stays where home says it is
      double *out = de_row(p, c.home ^ 1u, c.a);
      if (p.stream)  // wave-uniform
        store_row_stream<CHUNKS, VEC>(out, D, trial);
      else
        store_row<CHUNKS, VEC>(out, D, trial);
    }
    if (lane == 0) {
      p.scores[par ^ 1][c.a] = accept ? score : c.old_score;
      p.home[par ^ 1][c.a] = static_cast<uint8_t>((accept ? c.home ^ 1u : c.home) | hint | c.miss);
    }
    if (p.trace != nullptr && lane == 0) {
      uint64_t *t = p.trace + c.a * kTraceWords;
      t[0] = c.r0;
      t[1] = c.r1;
      t[2] = c.r2;
      t[3] = c.jrand;
      t[4] = accept ? 1u : 0u;
    }
  };
  auto count = [&](int which) {  // engines created with cfg.trace only
    if (p.counts != nullptr && lane == 0)
      atomicAdd(reinterpret_cast<unsigned long long *>(p.counts + which), 1ull);
  };
  // propose_new_agent (nlsolver.h:2357-2375)
  double trial[CHUNKS][2];
  if constexpr (BOUND) {
    if (c.bound) {  // wave-uniform; fmul == 1 here, so the objective's value is the score
      uint64_t kept = 0;  // lanes with a coordinate inside D that the trial takes from the old row
      const uint32_t d32 = static_cast<uint32_t>(D);
#pragma unroll
      for (int ch = 0; ch < CHUNKS; ch++) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
          const uint32_t e = static_cast<uint32_t>(ch) * 128 + 2 * static_cast<uint32_t>(lane) + k;
          trial[ch][k] = c.d1[ch][k] + p.F * (c.d2[ch][k] - c.d3[ch][k]);  // the mutant everywhere
          kept |= __ballot(e < d32) & ~c.cross[ch][k];
        }
      }
      const bool any_kept = kept != 0ull;
      const double bound = wave_objective_masked<OBJ, CHUNKS>(trial, c.cross, D);
      if (bound >= c.old_score) {  // (false for NaN) the score cannot be lower: rejected unread
        select(false, bound, trial, 0u);
        count(kDeBoundDecided);
        return;
      }
      if (!any_kept) {  // CR >= 1: the mutant is the trial and the bound its score
        const bool accept = bound < c.old_score;
        select(accept, bound, trial, 0u);
        count(accept ? kDeBoundAccepted : kDeBoundRejected);
        return;
      }
      // not decided: the own row now, a dependent load, and the full evaluation
      load_row_kept<CHUNKS, VEC>(de_row(p, c.home, c.a), D, p.zero, c.cross, c.keep);
#pragma unroll
      for (int ch = 0; ch < CHUNKS; ch++) {
#pragma unroll
        for (int k = 0; k < 2; k++) trial[ch][k] = lane_bit(c.cross[ch][k]) ? trial[ch][k] : c.keep[ch][k];
      }
      const double score = wave_objective<OBJ, CHUNKS>(trial, D);  // :2463
      const bool accept = score < c.old_score;                     // :2466 (NaN -> keep)
      select(accept, score, trial, 2u);
      count(accept ? kDeBoundAccepted : kDeBoundRejected);
      return;
    }
  }
#pragma unroll
  for (int ch = 0; ch < CHUNKS; ch++) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const double mut = c.d1[ch][k] + p.F * (c.d2[ch][k] - c.d3[ch][k]);
      trial[ch][k] = lane_bit(c.cross[ch][k]) ? mut : c.keep[ch][k];
    }
  }
  // (elements >= D are 0 in every loaded row, hence 0 in the trial as well)
  const double score = p.fmul * wave_objective<OBJ, CHUNKS>(trial, D);  // :2463
  select(score < c.old_score, score, trial, c.hint);                    // :2466 (NaN -> keep)
}

// ---- agents of at most 64 coordinates: 64 / G agents per wave, one per group of G lanes (G = 4, 8,
// 16, 32 for D <= 8, 16, 32, 64; lane g of a group holds coordinates 2g, 2g + 1). One agent per
// wave leaves 64 - D / 2 lanes idle and costs the same 38 us per generation at D = 16 as at
// D = 64. Everything that is wave-uniform above is group-uniform here and lives in vector
// registers: the agent's key, its draws (lane g of a group takes draw D + round * G + g of the
// agent's stream: draw D is jrand, draw D + 1 + k donor candidate k) and the donor picks, which
// walk the candidates in order with selects instead of branches. group_objective gives the trial
// the bits of the full-wave tree, so a population's history does not depend on the packing.
template <int OBJ, int G>
__device__ inline void de_generation_groups_block(const DeParams &p, int par, uint64_t generation,
                                                  int ignore_done, uint64_t block) {
  constexpr int P = 64 / G;
  const DeState *__restrict__ st = p.state;
  if (!ignore_done && st->done) return;
  const uint64_t wave = block * 4 + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (wave * P >= p.shard_n) return;
  const int lane = lane_id(), g = lane & (G - 1), gi = lane / G;
  const bool live = wave * P + gi < p.shard_n;
  const uint64_t a = live ? wave * P + gi : wave * P;  // idle groups shadow a live agent
  const uint64_t D = p.D;
  const uint8_t *__restrict__ hp = p.home[par];
  const uint32_t ha = hp[a];  // issued ahead of the donor picks
  const bool rnd = p.strategy == NLSG_DE_RANDOM;
  const uint64_t kg = first64(ctr_key(on_valu(p.seed), generation));
  const uint64_t ga = p.shard_lo + a;
  const uint64_t ka = ctr_key(kg, ga);
  const uint64_t fixed = rnd ? ga : st->best_id;  // :2451-2457
  // draws D + round * G + g; cross-lane reads stay inside the group
  const int base = gi * G;
  uint64_t drawn = ctr_key(ka, D + static_cast<uint64_t>(g));
  const uint64_t jrand = clamp_index(u01(__shfl(drawn, base, 64)), D);  // :2364
  // generate_indices (nlsolver.h:2331-2355): three distinct donors != fixed, by rejection
  uint64_t r0 = ~0ull, r1 = ~0ull, r2 = ~0ull;
  int have = 0;
  for (int k = 0; k < kDeMaxTries; k++) {
    if (__ballot(have < 3) == 0ull) break;
    const int pos = k + 1;  // candidate k is draw D + pos: round pos / G, lane pos % G
    if (pos >= G && (pos & (G - 1)) == 0)
      drawn = ctr_key(ka, D + static_cast<uint64_t>(pos + g));
    const uint64_t cand =
        p.shard_lo + clamp_index(u01(__shfl(drawn, base + (pos & (G - 1)), 64)), p.shard_n);
    const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
    const bool take = !used && have < 3;
    r0 = (take && have == 0) ? cand : r0;
    r1 = (take && have == 1) ? cand : r1;
    r2 = (take && have == 2) ? cand : r2;
    have += take ? 1 : 0;
  }
  for (uint64_t cand = p.shard_lo; __ballot(have < 3) != 0ull; cand++) {  // fallback: lowest unused
    const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
    const bool take = !used && have < 3;
    r0 = (take && have == 0) ? cand : r0;
    r1 = (take && have == 1) ? cand : r1;
    r2 = (take && have == 2) ? cand : r2;
    have += take ? 1 : 0;
  }
  // the crossover mask of propose_new_agent (nlsolver.h:2357-2375); u01(zc) < CR on the draw's
  // bits (DeParams.cr_thresh)
  const uint32_t j0 = 2 * g, j1 = 2 * g + 1;
  const bool in0 = j0 < D, in1 = j1 < D;
  const uint64_t ka_lane = ka + kGolden * (2 * static_cast<uint64_t>(g) + 1);
  bool cross[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint64_t zc = mix64(ka_lane + kGolden * static_cast<uint64_t>(k));
    cross[k] = zc < p.cr_thresh || p.cr_all || 2 * static_cast<uint64_t>(g) + k == jrand;
  }
  // rows through the home selectors: three donors, and where the trial keeps the old coordinate
  // the agent's own row (strategy random) or the row of best_id (strategy best)
  const uint32_t d32 = static_cast<uint32_t>(D);
  auto row = [&](uint32_t h, uint64_t local) {
    return ((h & 1u) ? p.buf[1] : p.buf[0]) + static_cast<uint64_t>(static_cast<uint32_t>(local)) * d32;
  };
  auto load2 = [&](const double *rp, double (&v)[2]) {
    v[0] = in0 ? rp[j0] : 0.0;
    v[1] = in1 ? rp[j1] : 0.0;
  };
  double d1[2], d2[2], d3[2], keep[2];
  load2(row(hp[r0 - p.shard_lo], r0 - p.shard_lo), d1);
  load2(row(hp[r1 - p.shard_lo], r1 - p.shard_lo), d2);
  load2(row(hp[r2 - p.shard_lo], r2 - p.shard_lo), d3);
  const double *ks = rnd ? row(ha, a) : p.best_x;
  keep[0] = (in0 && !cross[0]) ? ks[j0] : 0.0;
  keep[1] = (in1 && !cross[1]) ? ks[j1] : 0.0;
  const double old_score = p.scores[par][a];
  double trial[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const double mut = d1[k] + p.F * (d2[k] - d3[k]);
    const double t = cross[k] ? mut : keep[k];
    trial[k] = (k ? in1 : in0) ? t : 0.0;
  }
  const double score = p.fmul * group_objective<OBJ, G>(trial[0], trial[1], D);  // :2463
  const bool accept = score < old_score;                                         // :2466
  if (live) {
    if (accept) {  // a rejected trial stores nothing (DeParams.home)
      double *out = row(ha ^ 1u, a);
      if (in0) out[j0] = trial[0];
      if (in1) out[j1] = trial[1];
    }
    if (g == 0) {
      p.scores[par ^ 1][a] = accept ? score : old_score;
      p.home[par ^ 1][a] = static_cast<uint8_t>(accept ? ha ^ 1u : ha);
      if (p.trace != nullptr) {
        uint64_t *t = p.trace + a * kTraceWords;
        t[0] = r0;
        t[1] = r1;
        t[2] = r2;
        t[3] = jrand;
        t[4] = accept ? 1u : 0u;
      }
    }
  }
}

template <int OBJ, int G>
__global__ __launch_bounds__(256) void de_generation_groups_kernel(DeParams p, int par,
                                                                   uint64_t generation,
                                                                   int ignore_done) {
  de_generation_groups_block<OBJ, G>(p, par, generation, ignore_done, blockIdx.x);
}

// ---- the half-row reject screen: four agents per wave, planned side by side (kDeBoundScreen) -----
// Wave w of the generation takes agents 4w .. 4w + 3 (kDeScreenAgents) and runs in two phases.
//
// Phase 1, the plan, once per wave. Lane 8q + c works for agent 4w + q (the groups q >= 4, and
// those past the shard's end, shadow agent 4w and never run). Every lane of a group computes the
// agent's key; lane c takes draw D + c of its stream -- c = 0 jrand, c = 1..7 donor candidates
// 0..6, the values lanes 0..7 of the one-agent path hold -- and loads a selector byte: the agent's
// own (c = 0) or its candidate's (always in bounds), so every byte load of the wave is one round
// trip. The picks are made inside the group by first occurrences: candidate k is kept when it
// differs from the agent and from every candidate before it (six lane-shifted compares, masked to
// the group), the picks are the first three kept ones in order (a lane's rank is the population
// count of its group's kept bits below its own), and the agent runs the screen when there are
// three. That is de_fetch_agent's rule -- the first three candidates in order that differ from the
// agent and from each other -- wherever the third of them lies at candidate <= 6; every other agent
// declines (fewer than three donors among the rule's candidates, or a pick whose selector byte no
// lane loaded: both end in the one-agent path, and nothing the device writes tells them apart).
// Checked exhaustively on the host (tests/test_de_picks_cpu.py). No value goes through scalar
// registers. Each agent's plan -- the addresses of its three donor rows, key, old score, jrand,
// selector byte, `run` -- goes into 64 B of LDS private to the wave: no block-level barrier, a
// wave reads what it wrote.
//
// Phase 2, the rows, one pass per two agents: the lower half-wave works on agent 4w + 2i, the upper
// one on 4w + 2i + 1, half-lane j = lane & 31 holding coordinates 2j, 2j + 1. A half reads its
// agent's plan from LDS (one address per half: a broadcast), the first 512 B of the three donor
// rows, and does the per-coordinate work: 64 crossover draws, mutant, terms, the half's tree, the
// decision and the stores of the decided exit. The crossover masks of both passes are computed
// ahead of the first use of a row.
//
// Afterwards the agents the screen did not decide -- missed, declined, backed off, no bound try
// this generation -- go through de_fetch_agent / de_process_agent, run by the whole wave one after
// the other, with the miss count phase 2 left for them.
//
// The screen value. Lane j accumulates as wave_objective_masked does -- 0.0, then term 2j, then
// term 2j + 1, +0.0 in place of a term that reads a kept coordinate -- with term 63 always +0.0
// (its neighbour x64 is not loaded), and the butterfly levels 16 .. 1 run inside the half. Proof
// that this is wave_objective_masked's tree with every term >= 64 replaced by +0.0: there lanes
// 32..63 hold +0.0 before the butterfly, level 32 of wave_sum runs first and leaves
// acc_j + (+0.0) = acc_j in lanes j and 32 + j (acc_j is >= +0 or NaN), and levels 16 .. 1 never
// cross the half. Terms are >= +0 or NaN (TermsNonNegative) and round-to-nearest addition is
// monotone in each operand, so screen <= bound <= score bit for bit whenever the bound is not NaN,
// and screen >= old_score (false for NaN) implies bound >= old_score: the bound's "decided" exit,
// whose stores are the ones made here. (A NaN among the terms past 63 makes bound and score NaN:
// the trial is rejected all the same, every output equal; only the bound's hint and its counters,
// which no output depends on, would then say "not decided".)
//
// Why four agents and not eight: with eight (four passes) the wave issues 80 vector instructions
// per agent against 144 of the two-agent wave it replaces, but a population of 65 536 is then 8 192
// waves, all resident at once and in step, and the turn was no faster.
constexpr int kDeScreenPasses = 2;                      // passes of phase 2 (at most 4: a group per agent)
constexpr int kDeScreenAgents = 2 * kDeScreenPasses;    // agents of a screening wave (nlsg_de.hip: the grid)
constexpr int kDePlanWords = 16;  // 32-bit words of an agent's plan in LDS (de_generation_screen)

template <int OBJ, bool VEC, int NP = kDeScreenPasses>
__device__ inline void de_generation_screen(const DeParams &p, int par, uint64_t generation, uint64_t block) {
  static_assert(TermsNonNegative<OBJ>::value, "the screen needs terms >= 0");
  using O = Objective<OBJ>;
  typedef double __attribute__((address_space(1))) global_double;
  typedef double __attribute__((ext_vector_type(2))) double_x2;
  typedef double_x2 __attribute__((address_space(1))) global_double_x2;
  // plan of agent a0 + q, written in phase 1 and read in phase 2 by this wave alone:
  //   words 0-5 the addresses of the three donor rows, 6-7 the agent's key, 8-9 its old score,
  //   10 jrand, 11 the selector byte (bits 0-7) and `run` (bit 8), 12-14 the donors' indices
  __shared__ __attribute__((aligned(16))) uint32_t plans[4 * 8 * kDePlanWords];
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t per_wave = 2 * NP;
  const uint64_t a0 = per_wave * (block * 4 + __builtin_amdgcn_readfirstlane(static_cast<int>(tid >> 6)));
  if (a0 >= p.shard_n) return;
  const uint64_t rest = p.shard_n - a0;
  const uint32_t n_live = rest < per_wave ? static_cast<uint32_t>(rest) : per_wave;  // wave-uniform
  const uint32_t lane = tid & 63u;
  const uint32_t d32 = static_cast<uint32_t>(p.D);
  // both buffer bases out of the kernel arguments once (see de_fetch_agent)
  global_double *base0 = (global_double *)p.buf[0], *base1 = (global_double *)p.buf[1];
  asm("" : "+s"(base0), "+s"(base1));
  {  // ---- phase 1, the plan: lane 8q + c works for agent a0 + q
    const uint32_t c = lane & 7u, q = lane >> 3;
    const bool live = q < n_live;
    // (shard sizes fit 32 bits; a group past the shard's end shadows agent a0 and never runs)
    const uint32_t a = static_cast<uint32_t>(a0) + (live ? q : 0u);
    const uint8_t *__restrict__ hp = p.home[par];
    const uint64_t ka = ctr_key(p.gen_key, p.shard_lo + a);
    // draw D + c of the agent's stream: c = 0 jrand (:2364), c = 1..7 donor candidates 0..6
    const uint32_t lim = c == 0 ? d32 : static_cast<uint32_t>(p.shard_n);
    const uint32_t idx = static_cast<uint32_t>(u01(mix64(ka + golden_times(d32 + c + 1u))) * static_cast<double>(lim));
    const uint32_t drawn = idx >= lim ? lim - 1 : idx;  // the u == 1.0 corner clamped (B10)
    // every byte load of the wave in one round trip: c = 0 the agent's selector byte, c = 1..7 the
    // candidates' (always in bounds), and the old score beside them
    const uint32_t sel = hp[c == 0 ? a : drawn];
    const double old_score = p.scores[par][a];
    // generate_indices (nlsolver.h:2331-2355) on candidates 0..6: a candidate is kept when it differs
    // from the agent and from every candidate before it; the picks are the first three kept ones.
    // row_shr:s brings lane c - s's draw; the masks leave only compares of candidates of one group
    // (c - s >= 1). A lane whose source lies outside its row keeps its own value and is masked too.
    constexpr uint64_t each = 0x0101010101010101ull;
    uint64_t dup = __ballot(dpp_mov32<0x111, 0xF>(drawn, drawn) == drawn) & (0xFCull * each);
    dup |= __ballot(dpp_mov32<0x112, 0xF>(drawn, drawn) == drawn) & (0xF8ull * each);
    dup |= __ballot(dpp_mov32<0x113, 0xF>(drawn, drawn) == drawn) & (0xF0ull * each);
    dup |= __ballot(dpp_mov32<0x114, 0xF>(drawn, drawn) == drawn) & (0xE0ull * each);
    dup |= __ballot(dpp_mov32<0x115, 0xF>(drawn, drawn) == drawn) & (0xC0ull * each);
    dup |= __ballot(dpp_mov32<0x116, 0xF>(drawn, drawn) == drawn) & (0x80ull * each);
    const uint64_t keep = __ballot(drawn != a) & ~dup & (0xFEull * each);
    const uint32_t grp = static_cast<uint32_t>(keep >> (lane & 56u)) & 0xFFu;  // the group's byte
    const uint32_t rank = static_cast<uint32_t>(__builtin_popcount(grp & ((1u << c) - 1u)));
    const bool ok = __builtin_popcount(grp) >= 3;
    const bool mine = ((grp >> c) & 1u) != 0 && rank < 3;
    const bool run = live & ok & de_screen_tries(sel, generation, a, p.retry_mask, p.screen_retry_mask);
    uint32_t *rec = plans + (tid >> 3) * kDePlanWords;
    if (c == 0) {
      // (an agent that does not run has fewer than three picks: every address it leaves behind is
      // a row's all the same)
      const uint64_t b = reinterpret_cast<uint64_t>(base0);
      const uint64_t os = static_cast<uint64_t>(__double_as_longlong(old_score));
      const uint32_t bl = static_cast<uint32_t>(b), bh = static_cast<uint32_t>(b >> 32);
      *reinterpret_cast<uint4 *>(rec) = make_uint4(bl, bh, bl, bh);
      *reinterpret_cast<uint4 *>(rec + 4) =
          make_uint4(bl, bh, static_cast<uint32_t>(ka), static_cast<uint32_t>(ka >> 32));
      *reinterpret_cast<uint4 *>(rec + 8) = make_uint4(static_cast<uint32_t>(os), static_cast<uint32_t>(os >> 32),
                                                       drawn, (sel & 0xFFu) | (run ? 0x100u : 0u));
    }
    if (mine) {
      global_double *row = ((sel & 1u) ? base1 : base0) + static_cast<uint64_t>(drawn) * d32;
      *reinterpret_cast<uint64_t *>(rec + 2 * rank) = reinterpret_cast<uint64_t>(row);
      rec[12 + rank] = drawn;
    }
  }
  // the wave reads what its own lanes wrote: LDS operations of a wave complete in order, and the
  // compiler must not move the reads up
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // ---- phase 2, the rows: in pass i the lower half-wave works on agent a0 + 2i, the upper one on
  // a0 + 2i + 1; half-lane j holds coordinates 2j, 2j + 1
  const uint32_t j = lane & 31u;
  const bool upper = lane >= 32;
  const uint32_t *plan0 = plans + (tid >> 6) * (8 * kDePlanWords) + (upper ? kDePlanWords : 0);
  struct Pass {
    double old_score;
    uint32_t jrand, flags;
    double d1[2], d2[2], d3[2];
  };
  // the plan and the first 512 B of the three donor rows (coordinates 0..63 < D), never the own row
  auto fetch = [&](int i, Pass &R) {
    const uint32_t *rd = plan0 + i * (2 * kDePlanWords);
    const uint4 w0 = *reinterpret_cast<const uint4 *>(rd);
    const uint2 w1 = *reinterpret_cast<const uint2 *>(rd + 4);
    const uint4 w2 = *reinterpret_cast<const uint4 *>(rd + 8);
    auto u64 = [](uint32_t lo, uint32_t hi) { return (static_cast<uint64_t>(hi) << 32) | lo; };
    R.old_score = __longlong_as_double(static_cast<long long>(u64(w2.x, w2.y)));
    R.jrand = w2.z;
    R.flags = w2.w;
    auto load2 = [&](uint64_t row, double (&v)[2]) {
      const global_double *src = reinterpret_cast<const global_double *>(row) + 2 * j;
      if (VEC) {
        const double_x2 t = *reinterpret_cast<const global_double_x2 *>(src);
        v[0] = t.x;
        v[1] = t.y;
      } else {
        v[0] = src[0];
        v[1] = src[1];
      }
    };
    load2(u64(w0.x, w0.y), R.d1);
    load2(u64(w0.z, w0.w), R.d2);
    load2(u64(w1.x, w1.y), R.d3);
  };
  // Crossover masks of coordinates 2j, 2j + 1 (propose_new_agent, nlsolver.h:2357-2375) as lane masks,
  // for every pass and ahead of the first use of a row: this is the work a wave has while its rows
  // are on their way. known0 / known1: the terms 2j and 2j + 1 read mutant coordinates only (lane
  // j + 1's first flag is the next bit; half-lane 31's neighbour is x64: never known).
  const uint64_t golden_j = golden_times(2 * j + 1u);
  const uint64_t cr_all = p.cr_all ? ~0ull : 0ull;
  uint64_t known0[NP], known1[NP];
  auto masks = [&](int i) {
    const uint32_t *rd = plan0 + i * (2 * kDePlanWords);
    const uint64_t ka_lane = *reinterpret_cast<const uint64_t *>(rd + 6) + golden_j;
    const uint32_t jrand = rd[10];
    const uint64_t c0 = __ballot(mix64(ka_lane) < p.cr_thresh) | cr_all | __ballot(2 * j == jrand);
    const uint64_t c1 = __ballot(mix64(ka_lane + kGolden) < p.cr_thresh) | cr_all | __ballot(2 * j + 1 == jrand);
    constexpr uint64_t not31 = ~((1ull << 31) | (1ull << 63));
    known0[i] = O::kChain ? (c0 & c1) : c0;
    known1[i] = c1 & (O::kChain ? (c0 >> 1) : ~0ull) & not31;
  };
  uint32_t decided = 0;  // bit q: the screen rejected the trial of agent a0 + q
  uint32_t lefts = 0;    // byte i: bits 2-3 of the selector byte pass i's agent leaves behind
  auto rows = [&](int i, const Pass &R, double x0, double x1) {
    const uint32_t a = static_cast<uint32_t>(a0) + 2 * i + (upper ? 1u : 0u);
    const bool run = (R.flags & 0x100u) != 0;
    const uint32_t cnt = (R.flags >> 2) & 3u;
    const double xn = lane_down1(x0);  // lane j + 1's first coordinate
    double acc = 0.0;
    acc = acc + (lane_bit(known0[i]) ? O::term(x0, x1) : 0.0);
    acc = acc + (lane_bit(known1[i]) ? O::term(x1, xn) : 0.0);
    butterfly_levels<16>([&](auto off) { acc = xor_add<decltype(off)::value>(acc); });
    const bool dec = run && acc >= R.old_score;  // (false for NaN) the score cannot be lower: rejected
    lefts |= (de_screen_count_after(cnt, dec ? 0 : run ? 1 : 2) << 2) << (8 * i);
    if (j == 0 && dec) {  // what the bound's "decided" exit stores (select(false, ..., 0u))
      p.scores[par ^ 1][a] = R.old_score;
      p.home[par ^ 1][a] = static_cast<uint8_t>(R.flags & 1u);
      if (p.trace != nullptr) {
        const uint32_t *rd = plan0 + i * (2 * kDePlanWords);
        uint64_t *t = p.trace + static_cast<uint64_t>(a) * kTraceWords;
        t[0] = p.shard_lo + rd[12];
        t[1] = p.shard_lo + rd[13];
        t[2] = p.shard_lo + rd[14];
        t[3] = R.jrand;
        t[4] = 0u;
      }
    }
    if (p.counts != nullptr && j == 0 && run) {  // engines created with cfg.trace only
      if (dec) atomicAdd(reinterpret_cast<unsigned long long *>(p.counts + kDeBoundDecided), 1ull);
      atomicAdd(reinterpret_cast<unsigned long long *>(p.counts + (dec ? kDeScreenDecided : kDeScreenMissed)), 1ull);
    }
    const uint64_t d = __ballot(dec);
    decided |= ((static_cast<uint32_t>(d) & 1u) | ((static_cast<uint32_t>(d >> 32) & 1u) << 1)) << (2 * i);
    // pass 0 of the waves that start at a multiple of 128 (agents 128 m and 128 m + 1) adds its
    // decisions to a running count the host reads with the state (kDeScreenStat): what the engine
    // switches the screening wave off and on by, see nlsg_de.hip
    if (i == 0 && (a0 & 127u) == 0) {
      asm volatile("" ::: "memory");
      if (d != 0ull && lane == 0)
        atomicAdd(p.ticket + kDeScreenStat, static_cast<uint32_t>(__builtin_popcountll(d & 0x0000000100000001ull)));
    }
  };
  // the row loads of two passes are in flight at a time: those of pass i + 2 leave as soon as the
  // mutant of pass i has freed their registers
  Pass R[2];
  fetch(0, R[0]);
  if (NP > 1) fetch(1, R[1]);
#pragma unroll
  for (int i = 0; i < NP; i++) masks(i);
#pragma unroll
  for (int i = 0; i < NP; i++) {
    Pass &C = R[i & 1];
    const Pass S = C;
    const double x0 = C.d1[0] + p.F * (C.d2[0] - C.d3[0]);  // the mutant
    const double x1 = C.d1[1] + p.F * (C.d2[1] - C.d3[1]);
    if (i + 2 < NP) fetch(i + 2, C);
    rows(i, S, x0, x1);
  }
  // not decided here (missed, declined, backed off, no bound try): the trial goes through the
  // one-agent path, run by the whole wave, one agent after the other
  uint32_t undecided = ~decided & ((1u << n_live) - 1u);
  if (undecided == 0) return;
  const uint32_t lefts_l = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lefts), 0));
  const uint32_t lefts_h = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lefts), 32));
  const uint64_t best_id = p.state->best_id;
  do {
    const uint32_t q = static_cast<uint32_t>(__builtin_ctz(undecided));
    undecided &= undecided - 1u;
    DeAgent<1> A;
    de_fetch_agent<true, 1, VEC>(p, par, p.gen_key, generation, best_id, a0 + q, A);
    A.miss = (((q & 1u) ? lefts_h : lefts_l) >> (8 * (q >> 1))) & 0xCu;
    de_process_agent<OBJ, 1, VEC, true>(p, par, A);
  } while (undecided != 0);
}

// One agent per wave. (Two agents per wave — ten gathers in flight — measured -7 % kernel time at
// pop = 65536 but +9 % at pop = 2^20 and only -2 % per turn; not kept.)
// BOUND: the instantiation an engine with DeParams.bound set launches (TermsNonNegative objectives
// only); every other engine runs BOUND = false, the code without the bound. SCREEN: the instantiation
// an engine with kDeBoundScreen set launches (de_generation_screen); the others are the code without it.
template <int OBJ, int CHUNKS, bool VEC, bool BOUND = false, bool SCREEN = false>
__device__ inline void de_generation_block(const DeParams &p, int par, uint64_t generation,
                                           int ignore_done, uint64_t block) {
  // `generation` (k+1) and the source buffer `par` (k & 1) come from the host: the k-th
  // turn's head may still be running when this kernel starts (speculative launch for
  // strategy random); the device state is only consulted for the stop flag, which is
  // final for every head older than that one.
  const DeState *__restrict__ st = p.state;
  if (!ignore_done && st->done) return;  // a stop test fired: the turn is a no-op
  if constexpr (SCREEN) {  // kDeBoundScreen: the launch's grid has a block per 4 * kDeScreenAgents agents
    static_assert(BOUND && CHUNKS == 1, "the screen rides on the bound, rows of 65..128 coordinates");
    de_generation_screen<OBJ, VEC>(p, par, generation, block);
    return;
  }
  const uint64_t a0 = block * 4 + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (a0 >= p.shard_n) return;
  const uint64_t kg = p.gen_key;  // = ctr_key(p.seed, generation), from the host
  const uint64_t best_id = st->best_id;
  DeAgent<CHUNKS> A;
  de_fetch_agent<BOUND, CHUNKS, VEC>(p, par, kg, generation, best_id, a0, A);
  de_process_agent<OBJ, CHUNKS, VEC, BOUND>(p, par, A);
}

template <int OBJ, int CHUNKS, bool VEC, bool BOUND = false, bool SCREEN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SCREEN ? 8 : 1, 8))) void de_generation_kernel(DeParams p, int par, uint64_t generation,
                                                          int ignore_done) {
  de_generation_block<OBJ, CHUNKS, VEC, BOUND, SCREEN>(p, par, generation, ignore_done, blockIdx.x);
}

// Gather of the population `par` into one contiguous [shard_n][D] block (host download)
__global__ __launch_bounds__(256) void de_gather_kernel(DeParams p, int par, double *__restrict__ out) {
  for (uint64_t r = blockIdx.x; r < p.shard_n; r += gridDim.x) {
    const double *__restrict__ src = de_row(p, p.home[par][r], r);
    for (uint64_t d = threadIdx.x; d < p.D; d += 256) out[r * p.D + d] = src[d];
  }
}

// ---- best scan + stop tests -------------------------------------------------
// ---- the head of a turn ---------------------------------------------------------
// Separate scan / finisher launches cost a dependent dispatch each (~5 us; 10 us of a 59 us
// turn at pop 65536 for eps <= 0, five launches and ~25 us with a two-pass std_err), so a head
// is ONE launch: one block per tile of kTile scores reduces it -- minimum and first index and,
// when std_err can decide (eps > 0), the tile's sum and its M2 about the TILE mean, scores held
// in registers -- publishes that with write-through stores, drains them and takes a ticket;
// the block that takes the last ticket reads every partial with cache-bypassing loads and
// finishes: best with the incumbent rule, std_err, counters, stop tests, best_x -- or, on a
// shard, the exchange record
//   [minv, mini(bits), sum, M2 about the shard mean, valid, x_best[0..D)]   (kRecHeader + D)
// (`valid` is 0 only for a shard whose scores are all NaN and that does not own the incumbent).
// std_err (nlsolver.h:2037-2052) in one pass: tiles are merged the way shards are,
//   total = tree_t(sum_t), mean = total / n, M2 = tree_t(M2_t + n_t (sum_t / n_t - mean)^2)
// (a population of one tile is exactly the two-pass formula). min / first-index are order-
// independent and the sums keep their fixed trees (thread-sequential partials, wave butterfly,
// ((w0+w1)+w2)+w3 per tile, the same tree over tiles), so which block ends up last does not
// matter. No release / acquire fence: a release would write back every dirty line that
// generation blocks of the same launch hold in the XCD's L2.
// thread 0, after the block's partial stores: true in the block that arrived last
__device__ inline bool take_ticket(const DeParams &p) { return take_ticket(p.ticket, p.ntiles); }

// `rec` == nullptr: one GPU, the launch finishes the turn; else the shard's exchange record
__device__ inline void de_scan_head_block(const DeParams &p, uint64_t k, uint32_t tile, double *rec) {
  __shared__ double red[4];
  __shared__ double mv[4];
  __shared__ uint64_t mi[4];
  __shared__ uint64_t s_row;
  __shared__ int s_have;
  __shared__ int s_last;
  DeState *st = p.state;
  if (st->done) return;  // only written by a last block, after every block got here
  const int par = static_cast<int>(k & 1);
  const bool need_se = p.eps > 0;
  const double *__restrict__ sc = p.scores[par];
  const uint64_t base = static_cast<uint64_t>(tile) * kTile;
  const uint64_t tile_n = (p.shard_n - base) < kTile ? (p.shard_n - base) : kTile;
  double v[kTile / 256];
  double acc = 0.0;
  double bv = __builtin_inf();
  uint64_t bi = ~0ull;
#pragma unroll
  for (int q = 0; q < kTile / 256; q++) {
    const uint64_t i = threadIdx.x + 256u * q;
    v[q] = sc[base + (i < tile_n ? i : 0)];  // clamped, masked below
  }
#pragma unroll
  for (int q = 0; q < kTile / 256; q++) {
    const uint64_t i = threadIdx.x + 256u * q;
    if (i < tile_n) {
      acc = acc + v[q];
      argmin_combine(bv, bi, v[q], base + i);
    }
  }
  double tile_sum = 0.0, tile_m2 = 0.0;
  if (need_se) {
    tile_sum = block_tree_256(acc, red);
    const double tile_mean = tile_sum / static_cast<double>(tile_n);
    acc = 0.0;
#pragma unroll
    for (int q = 0; q < kTile / 256; q++) {
      const double d = v[q] - tile_mean;
      if (threadIdx.x + 256u * q < tile_n) acc = acc + d * d;  // :2046-2049
    }
    tile_m2 = block_tree_256(acc, red);
  }
  block_argmin_256(bv, bi, mv, mi);
  if (threadIdx.x == 0) {
    sc1_store(&p.part[tile].minv, bv);
    __hip_atomic_store(&p.part[tile].mini, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (need_se) {
      sc1_store(&p.part[tile].sum, tile_sum);
      sc1_store(&p.part[tile].m2, tile_m2);
    }
    s_last = take_ticket(p) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  if (threadIdx.x == 0) head_position(st, p, k);
  bv = __builtin_inf();
  bi = ~0ull;
  for (uint32_t j = threadIdx.x; j < p.ntiles; j += 256)
    argmin_combine(bv, bi, sc1_load(&p.part[j].minv),
                   __hip_atomic_load(&p.part[j].mini, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  block_argmin_256(bv, bi, mv, mi);
  double total = 0.0, m2 = 0.0;
  if (need_se) {
    acc = 0.0;
    for (uint32_t j = threadIdx.x; j < p.ntiles; j += 256) acc = acc + sc1_load(&p.part[j].sum);
    total = block_tree_256(acc, red);
    const double mean = total / static_cast<double>(p.shard_n);  // :2044
    acc = 0.0;
    for (uint32_t j = threadIdx.x; j < p.ntiles; j += 256) {
      const uint64_t jb = static_cast<uint64_t>(j) * kTile;
      const double nj = static_cast<double>((p.shard_n - jb) < kTile ? (p.shard_n - jb) : kTile);
      // equal means add no between-tile term: the subtraction's own result when they are
      // finite, and M2 = +inf (the literal formula's) instead of NaN when the sums overflowed
      const double mj = sc1_load(&p.part[j].sum) / nj;
      const double dm = mj == mean ? 0.0 : mj - mean;
      acc = acc + (sc1_load(&p.part[j].m2) + nj * (dm * dm));
    }
    m2 = block_tree_256(acc, red);
  }
  if (threadIdx.x == 0) {
    // Shard minimum with the reference's tie rule (strict '<' scan starting from the
    // incumbent, nlsolver.h:2432-2437): the incumbent survives when nobody in the shard is
    // strictly better.
    const uint64_t inc = st->best_id;
    uint64_t gi = (bi == ~0ull) ? inc : p.shard_lo + bi;
    if (inc >= p.shard_lo && inc < p.shard_lo + p.shard_n) {
      const double inc_score = sc[inc - p.shard_lo];
      if (!(bv < inc_score)) {
        gi = inc;
        bv = inc_score;
      }
    }
    const bool mine = gi >= p.shard_lo && gi < p.shard_lo + p.shard_n;
    if (rec == nullptr) {
      finish_turn(st, p, gi, bv, mine,
                  need_se ? sqrt(m2 / static_cast<double>(p.pop - 1))  // :2050-2051
                          : __builtin_nan(""));
    } else {
      rec[0] = bv;
      rec[1] = __longlong_as_double(static_cast<long long>(gi));
      rec[2] = total;
      rec[3] = m2;
      rec[4] = mine ? 1.0 : 0.0;
    }
    s_row = gi - p.shard_lo;
    s_have = mine ? 1 : 0;
  }
  __syncthreads();
  const bool have = s_have != 0;
  const uint64_t r = have ? s_row : 0;
  const double *row = de_row(p, p.home[par][r], r);  // x = agents[best_id], :2444
  if (rec != nullptr) {
    for (uint64_t d = threadIdx.x; d < p.D; d += 256) rec[kRecHeader + d] = have ? row[d] : 0.0;
  } else if (have) {
    for (uint64_t d = threadIdx.x; d < p.D; d += 256) p.best_x[d] = row[d];
  }
}

__global__ __launch_bounds__(256) void de_scan_head_kernel(DeParams p, uint64_t k, double *rec) {
  de_scan_head_block(p, k, blockIdx.x, rec);
}

// One launch per turn for strategy random (one GPU): the first ntiles blocks run
// head k (scan of population k, stop tests), the others build generation k+1 from population
// k at the same time. Random donors do not depend on the head's result; if head k fires a
// stop test, generation k+1 went to the other buffers and is never adopted (exactly the
// speculative turn of the sharded path), so results equal the serial order head -> generation.
template <int OBJ, int CHUNKS, bool VEC, bool BOUND = false, bool SCREEN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SCREEN ? 8 : 1, 8))) void de_turn_kernel(DeParams p, int par, uint64_t generation) {
  if (blockIdx.x < p.ntiles) {
    de_scan_head_block(p, generation - 1, blockIdx.x, nullptr);
    return;
  }
  de_generation_block<OBJ, CHUNKS, VEC, BOUND, SCREEN>(p, par, generation, 0, blockIdx.x - p.ntiles);
}

// the same turn with the packed generation (agents of at most 64 coordinates, several per wave)
template <int OBJ, int G>
__global__ __launch_bounds__(256) void de_turn_groups_kernel(DeParams p, int par, uint64_t generation) {
  if (blockIdx.x < p.ntiles) {
    de_scan_head_block(p, generation - 1, blockIdx.x, nullptr);
    return;
  }
  de_generation_groups_block<OBJ, G>(p, par, generation, 0, blockIdx.x - p.ntiles);
}

// ---- the sharded path ----------------------------------------------------------
// Finaliser over `world` records (world == 1: the local record): global best
// (lower value; on ties the incumbent, then the lower global index), counters,
// stop tests (nlsolver.h:2439-2447), best_x. Single block.
__global__ __launch_bounds__(256) void de_finalize_kernel(DeParams p, const double *recs,
                                                        int32_t world, uint64_t rec_stride) {
  __shared__ int s_win;
  DeState *st = p.state;
  if (st->done) return;
  if (threadIdx.x == 0) {
    const uint64_t inc = st->best_id;
    int win = -1;
    double bv = __builtin_inf();
    uint64_t bi = inc;
    for (int r = 0; r < world; r++) {
      const double *rec = recs + static_cast<uint64_t>(r) * rec_stride;
      if (rec[4] != 1.0) continue;
      const double v = rec[0];
      const uint64_t i = static_cast<uint64_t>(__double_as_longlong(rec[1]));
      // a NaN incumbent stays: nothing is '< NaN' in the scan of :2432-2437, whatever an
      // earlier rank's record holds
      if (i == inc && v != v) {
        bv = v;
        bi = i;
        win = r;
        break;
      }
      const bool better =
          win < 0 || v < bv || (v == bv && bi != inc && (i == inc || i < bi));
      if (better) {
        bv = v;
        bi = i;
        win = r;
      }
    }
    // std_err over the global scores (only when it can decide: eps > 0)
    double se = __builtin_nan("");
    if (p.eps > 0) {
      // merge per-shard (n, sum, M2) in rank order; one shard == the two-pass
      // formula of nlsolver.h:2037-2052
      const double n_r = static_cast<double>(p.shard_n);
      double tot = 0.0;
      for (int r = 0; r < world; r++) tot = tot + recs[static_cast<uint64_t>(r) * rec_stride + 2];
      const double gmean = tot / static_cast<double>(p.pop);
      double m2 = 0.0;
      for (int r = 0; r < world; r++) {
        const double *rec = recs + static_cast<uint64_t>(r) * rec_stride;
        double term = rec[3];
        if (world > 1) {
          const double mr = rec[2] / n_r;
          const double dm = mr == gmean ? 0.0 : mr - gmean;  // as in the tile merge
          term = term + n_r * (dm * dm);
        }
        m2 = m2 + term;
      }
      se = sqrt(m2 / static_cast<double>(p.pop - 1));  // :2050-2051
    }
    finish_turn(st, p, bi, bv, win >= 0, se);
    s_win = win;
  }
  __syncthreads();
  if (s_win < 0) return;  // no valid record: keep best_x
  const double *src = recs + static_cast<uint64_t>(s_win) * rec_stride + kRecHeader;
  for (uint64_t d = threadIdx.x; d < p.D; d += 256) p.best_x[d] = src[d];
}

// ---- rows longer than a wave's registers hold (D > 1024; the reference has no limit) -----------
// One wave per agent, the rows taken in segments of 1024 coordinates. A generation makes two
// pass: it builds the trial segment by segment, scores it (objective_accumulate: the whole-row
// summation order) and stores it into the buffer the agent's row is not in (DeParams.home: that
// slot is nobody's until the generation is adopted); the selector then says whether the trial
// or the old row is the survivor, so a rejected trial costs no copy. Same draws (the element's index keys them), same arithmetic, same bits
// as the register-resident kernels would give — the oracle restates neither layout.
template <int OBJ, bool VEC>
__global__ __launch_bounds__(256) void de_init_long_kernel(DeParams p, const double *__restrict__ x0) {
  const uint64_t a = static_cast<uint64_t>(blockIdx.x) * 4 +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (a >= p.shard_n) return;
  const int lane = lane_id();
  const uint64_t D = p.D;
  const uint64_t ka = ctr_key(ctr_key(p.seed, 0), p.shard_lo + a);
  auto element = [&](uint64_t e) {  // generate_sequence, nlsolver.h:2309
    return (e < D) ? (u01(ctr_key(ka, e)) - 0.5) * x0[e] : 0.0;
  };
  double acc = 0.0;
  for (uint64_t e_base = 0; e_base < D; e_base += 128 * kSeg) {
    double xv[kSeg][2];
#pragma unroll
    for (int c = 0; c < kSeg; c++)
#pragma unroll
      for (int k = 0; k < 2; k++)
        xv[c][k] = element(e_base + static_cast<uint64_t>(c) * 128 + 2 * static_cast<uint64_t>(lane) + k);
    store_segment<VEC>(p.buf[0] + a * D, e_base, D, xv);
    objective_accumulate<OBJ, kSeg>(acc, xv, e_base, D, element(e_base + 128 * kSeg));
  }
  const double f = p.fmul * objective_finish<OBJ>(acc, D);  // :2423-2425
  if (lane == 0) {
    p.scores[0][a] = f;
    p.home[0][a] = 0;
  }
}

template <int OBJ, bool VEC>
__global__ __launch_bounds__(256) void de_generation_long_kernel(DeParams p, int par, uint64_t generation,
                                                               int ignore_done) {
  const DeState *__restrict__ st = p.state;
  if (!ignore_done && st->done) return;
  const uint64_t a = static_cast<uint64_t>(blockIdx.x) * 4 +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (a >= p.shard_n) return;
  const int lane = lane_id();
  const uint64_t D = p.D;
  const uint8_t *__restrict__ hp = p.home[par];
  const uint64_t kg = first64(ctr_key(on_valu(p.seed), generation));
  // donors and the forced dimension exactly as de_fetch_agent draws them
  const uint64_t ga = p.shard_lo + a;
  const uint64_t ka = first64(ctr_key(kg, on_valu(ga)));
  const uint64_t drawn = clamp_index(u01(ctr_key(ka, D + static_cast<uint64_t>(lane))),
                                     lane == 0 ? D : p.shard_n);
  const uint64_t best_id = st->best_id;
  const bool rnd = p.strategy == NLSG_DE_RANDOM;
  const uint64_t fixed = rnd ? ga : best_id;
  uint64_t r0 = ~0ull, r1 = ~0ull, r2 = ~0ull;
  int have = 0;
  for (int k = 0; k < kDeMaxTries && have < 3; k++) {
    const uint64_t cand = p.shard_lo + (k < 63 ? readlane64(drawn, k + 1)
                                               : clamp_index(u01(ctr_key(ka, D + 1 + k)), p.shard_n));
    const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
    if (!used) {
      if (have == 0) r0 = cand;
      else if (have == 1) r1 = cand;
      else r2 = cand;
      have++;
    }
  }
  for (uint64_t cand = p.shard_lo; have < 3; cand++) {
    const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
    if (!used) {
      if (have == 0) r0 = cand;
      else if (have == 1) r1 = cand;
      else r2 = cand;
      have++;
    }
  }
  const uint64_t jrand = readlane64(drawn, 0);
  const uint32_t ha = hp[a];
  const double *own = de_row(p, ha, a), *d1 = de_row(p, hp[r0 - p.shard_lo], r0 - p.shard_lo),
               *d2 = de_row(p, hp[r1 - p.shard_lo], r1 - p.shard_lo),
               *d3 = de_row(p, hp[r2 - p.shard_lo], r2 - p.shard_lo);
  const double *keep = rnd ? own : p.best_x;  // non-crossed coordinates (:2369-2372)
  auto trial_at = [&](uint64_t e) {  // one coordinate of the trial, the same in every lane
    if (e >= D) return 0.0;
    const uint64_t zc = ctr_key(ka, e);
    const double mut = d1[e] + p.F * (d2[e] - d3[e]);
    return (zc < p.cr_thresh || p.cr_all || e == jrand) ? mut : keep[e];
  };
  double *out = de_row(p, ha ^ 1u, a);
  double acc = 0.0;
  const uint64_t ka_lane = ka + kGolden * (2 * static_cast<uint64_t>(lane) + 1);
  for (uint64_t e_base = 0; e_base < D; e_base += 128 * kSeg) {
    double v1[kSeg][2], v2[kSeg][2], v3[kSeg][2], vk[kSeg][2], trial[kSeg][2];
    load_segment<VEC>(d1, e_base, D, p.zero, v1);
    load_segment<VEC>(d2, e_base, D, p.zero, v2);
    load_segment<VEC>(d3, e_base, D, p.zero, v3);
    load_segment<VEC>(keep, e_base, D, p.zero, vk);
    const uint64_t kseg = ka_lane + kGolden * e_base;
#pragma unroll
    for (int ch = 0; ch < kSeg; ch++)
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const uint64_t e = e_base + static_cast<uint64_t>(ch) * 128 + 2 * static_cast<uint64_t>(lane) + k;
        const uint64_t zc = mix64(kseg + kGolden * static_cast<uint64_t>(128 * ch + k));
        const double mut = v1[ch][k] + p.F * (v2[ch][k] - v3[ch][k]);
        trial[ch][k] = (zc < p.cr_thresh || p.cr_all || e == jrand) ? mut : vk[ch][k];
      }
    store_segment<VEC, true>(out, e_base, D, trial);
    objective_accumulate<OBJ, kSeg>(acc, trial, e_base, D, trial_at(e_base + 128 * kSeg));
  }
  const double score = p.fmul * objective_finish<OBJ>(acc, D);  // :2463
  const double old_score = p.scores[par][a];
  const bool accept = score < old_score;  // :2466 (NaN -> keep)
  if (lane == 0) {
    p.scores[par ^ 1][a] = accept ? score : old_score;
    p.home[par ^ 1][a] = static_cast<uint8_t>(accept ? ha ^ 1u : ha);
  }
  if (p.trace != nullptr && lane == 0) {
    uint64_t *t = p.trace + a * kTraceWords;
    t[0] = r0;
    t[1] = r1;
    t[2] = r2;
    t[3] = jrand;
    t[4] = accept ? 1u : 0u;
  }
}

// Before the host reads the state: unless a stop test fired, the engine stands after the
// k generations it has launched (the last head only saw k-1 of them).
// (and the screen's running count of sampled decisions travels with the state: kDeScreenStat)
__global__ void de_settle_kernel(DeParams p, uint64_t k) {
  if (!p.state->done) head_position(p.state, p, k);
  p.state->pad[0] = static_cast<int32_t>(p.ticket[kDeScreenStat]);
}

}  // namespace nlsg
