// nlsolver_amd/csrc/nlsg_de_ref_kernels.h — reference-order Differential Evolution: the reference's
// own DE (nlsolver.h:2414-2476, helpers 2302-2375) on the caller's xorshift stream, bit for bit.
//
// The reference's generation is asynchronous and in place: agent i's donors may be rows that agents
// < i replaced moments earlier, and every draw comes from ONE serial xorshift128+ stream. What makes
// it run well on a wave anyway is that the draw schedule does not depend on the population:
// generate_indices (2331-2355) rejects on the draws and on `fixed` only, and every agent then takes
// one forced-dimension draw and exactly D crossover draws (2364-2373; the left operand of || is always
// evaluated). So the wave produces the stream 64 draws at a time — lane l holds the state l steps
// ahead, and all lanes jump 64 steps with a nibble table of M^64 (xorshift128+ is linear over GF(2))
// — into an LDS ring, and the agents read their draws from it: the donor picks wave-uniformly, the
// crossover draws one per lane. The agents themselves are committed in index order, each trial's
// objective summed in index order (the reference's functors are plain left-to-right loops).
//
// One workgroup of one wave per solve. The population and its scores live in LDS when they fit
// (de_ref_lds_plan), else in global memory; a launch runs at most `gens` generations and leaves its
// state behind for the next (the host enqueues launches until every solve is done).
#pragma once

#include "nlsg_common.h"

namespace nlsg {

constexpr int kDeRefRing = 256;                 // draws the ring holds (a power of two)
constexpr int kDeRefJumpEntries = 32 * 16;      // nibble table of M^64: 32 nibbles x 16 values
constexpr uint32_t kDeRefMaxDonorDraws = 1u << 20;  // hard cap of one agent's donor rejection loop

// per-solve error flags (nlsg_status.reserved of the solve)
constexpr int32_t kDeRefErrNone = 0;
constexpr int32_t kDeRefErrIndex = 1;  // a draw of exactly 1.0 made generate_index return `pop`
constexpr int32_t kDeRefErrCap = 2;    // the donor rejection loop hit kDeRefMaxDonorDraws

// rng::xorshift::yield (nlsolver.h:1350-1361) on a raw state; returns the 64-bit sum it scales
__host__ __device__ inline uint64_t xorshift_step(uint64_t &x0, uint64_t &x1) {
  uint64_t t = x0;
  const uint64_t s = x1;
  x0 = s;
  t ^= t << 23;
  t ^= t >> 18;
  t ^= s ^ (s >> 5);
  x1 = t;
  return t + s;
}

// generate_indices (nlsolver.h:2331-2355) on draws from `next`: ids = {fixed, three distinct donors
// != fixed}. Guard rails the reference does not have: an index >= pop (only a draw of exactly 1.0
// makes one; the reference would read that row out of bounds) ends the pick with kDeRefErrIndex, and
// more than kDeRefMaxDonorDraws draws (the reference would spin) with kDeRefErrCap.
template <typename Next>
__host__ __device__ inline int32_t de_ref_donors(uint64_t fixed, uint64_t pop, Next &&next, uint64_t ids[4]) {
  ids[0] = fixed;
  int samples = 1;
  for (uint32_t k = 0; k < kDeRefMaxDonorDraws; k++) {
    const uint64_t prop = static_cast<uint64_t>(next() * static_cast<double>(pop));  // :2328
    if (prop >= pop) return kDeRefErrIndex;
    bool used = false;
    for (int j = 0; j < samples; j++) used |= (ids[j] == prop);
    if (!used) {
      ids[samples++] = prop;
      if (samples == 4) return kDeRefErrNone;
    }
  }
  return kDeRefErrCap;
}

struct DeRefCtl {  // one solve's state between launches
  uint64_t s0, s1;   // xorshift state after the last consumed draw
  uint64_t iter, fcalls, best_id, val_no_change, log_count;
  double std_err, f_value;
  int32_t phase;  // 0 fresh, 1 running, 2 finished
  int32_t err;    // kDeRefErr*
};

struct DeRefParams {
  double *x;              // [batch][D]: x0 in, the best agent out
  DeRefCtl *ctl;          // [batch]
  double *agents;         // [batch][pop][D] (the LDS copy's home between launches)
  double *scores;         // [batch][pop + 8]
  double *trial;          // [batch][D + 8] (used when the population is not in LDS)
  const uint64_t *jump;   // [32][16][2]: M^64 applied to nibble j = v of the state
  double *log_x;          // [batch][log_cap][D] or null
  double *log_f;          // [batch][log_cap]
  uint32_t *n_done;       // solves finished so far
  uint64_t batch, pop, D, max_iter, best_val_no_change, log_cap, gens;
  double CR, F, eps, fmul;
  int32_t strategy;       // NLSG_DE_BEST / NLSG_DE_RANDOM
  int32_t lds_pop;        // agents, scores and trial in LDS
  int32_t lds_scores;     // scores in LDS (always when lds_pop)
  int32_t pad;
};

// LDS layout: jump table | ring of states | term buffer | scores (pop + 8) | agents pop x D | trial D + 8
constexpr size_t kDeRefFixedLds = kDeRefJumpEntries * 16 + kDeRefRing * 16 + 72 * 8;
__host__ __device__ inline size_t de_ref_lds_bytes(uint64_t pop, uint64_t D, bool lds_pop, bool lds_scores) {
  size_t b = kDeRefFixedLds;
  if (lds_pop || lds_scores) b += (pop + 8) * 8;
  if (lds_pop) b += (pop * D + D + 8) * 8;
  return b;
}
// at most this much per workgroup: two of them still fit a CU's 160 KiB
constexpr size_t kDeRefLdsBudget = 78 * 1024;

// The wave's view of the stream. Lane l holds the state S_{H+l} (before draw H + l); the ring holds
// the states after draws [H - 256, H); `P` draws have been consumed. Positions count from the
// launch's start. The draw k is the sum of the two words of the state after it (yield's t + s).
struct DeRefStream {
  uint64_t st0, st1;  // this lane's state
  uint64_t H, P;      // wave-uniform
  uint64_t *ring;     // [256][2] LDS
  const uint64_t *jump;  // [512][2] LDS

  __device__ inline void block() {  // draws [H, H + 64) into the ring, then every lane jumps 64
    uint64_t a = st0, b = st1;
    xorshift_step(a, b);
    const int lane = lane_id();
    const uint64_t slot = (H + static_cast<uint64_t>(lane)) & (kDeRefRing - 1);
    ring[2 * slot] = a;
    ring[2 * slot + 1] = b;
    uint64_t r0 = 0, r1 = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t *e = jump + 2 * (16 * j + ((st0 >> (4 * j)) & 15));
      r0 ^= e[0];
      r1 ^= e[1];
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t *e = jump + 2 * (16 * (16 + j) + ((st1 >> (4 * j)) & 15));
      r0 ^= e[0];
      r1 ^= e[1];
    }
    st0 = r0;
    st1 = r1;
    H += 64;
    __syncthreads();
  }
  __device__ inline void ensure(uint64_t n) {  // n <= 64: draws [P, P + n) are in the ring
    while (H < P + n) block();
  }
  __device__ inline double at(uint64_t k) const {  // draw k (in the ring)
    const uint64_t slot = k & (kDeRefRing - 1);
    return u01(ring[2 * slot] + ring[2 * slot + 1]);
  }
  __device__ inline double next() {  // the next draw, wave-uniform
    ensure(1);
    return at(P++);
  }
};

// f(row) with the objective's terms added in index order (orc_objective_seq): the terms of 64
// coordinates at a time go through the wave's buffer `tb` (72 doubles) and one serial chain.
template <int OBJ>
__device__ inline double de_ref_objective(const double *row, uint64_t D, double *tb) {
  using O = Objective<OBJ>;
  const int lane = lane_id();
  const uint64_t nt = O::n_terms(D);
  double acc = 0.0;
  for (uint64_t e0 = 0; e0 < nt; e0 += 64) {
    const uint64_t e = e0 + static_cast<uint64_t>(lane);
    double t = 0.0;
    if (e < nt) t = O::term(row[e], O::kChain ? row[e + 1] : 0.0);  // (chain: e + 1 < D)
    tb[lane] = t;
    __syncthreads();
    acc = serial_sum_lds(tb, static_cast<int>(nt - e0 < 64 ? nt - e0 : 64), acc);
    __syncthreads();
  }
  return O::finish(acc, D);
}

// std_err (nlsolver.h:2037-2052): mean and squared deviations in index order (pow(d, 2) == d * d)
__device__ inline double de_ref_std_err(const double *scores, uint64_t n) {
  const double mean = serial_sum_lds(scores, static_cast<int>(n)) / static_cast<double>(n);
  const double ss = serial_chain_lds(scores, static_cast<int>(n), 0.0, [mean](double v) {
    const double d = v - mean;
    return d * d;
  });
  return sqrt(ss / static_cast<double>(n - 1));
}

template <int OBJ>
__device__ inline void de_ref_log(const DeRefParams &p, DeRefCtl &c, uint64_t b, const double *row, double f) {
  if (c.log_count < p.log_cap) {
    double *dst = p.log_x + (b * p.log_cap + c.log_count) * p.D;
    for (uint64_t d = static_cast<uint64_t>(lane_id()); d < p.D; d += 64) dst[d] = row[d];
    if (lane_id() == 0) p.log_f[b * p.log_cap + c.log_count] = f;
  }
  c.log_count++;
}

template <int OBJ>
__global__ __launch_bounds__(64) void de_ref_kernel(DeRefParams p) {
  extern __shared__ __align__(16) unsigned char de_ref_smem[];
  const uint64_t b = blockIdx.x;
  const int lane = lane_id();
  DeRefCtl c = p.ctl[b];  // (every lane: wave-uniform copy)
  if (c.phase == 2) return;
  const uint64_t pop = p.pop, D = p.D;

  uint64_t *jump = reinterpret_cast<uint64_t *>(de_ref_smem);
  uint64_t *ring = jump + 2 * kDeRefJumpEntries;
  double *tb = reinterpret_cast<double *>(ring + 2 * kDeRefRing);
  double *lds_rest = tb + 72;
  for (int k = lane; k < kDeRefJumpEntries; k += 64) {
    jump[2 * k] = p.jump[2 * k];
    jump[2 * k + 1] = p.jump[2 * k + 1];
  }
  double *const g_agents = p.agents + b * pop * D;
  double *const g_scores = p.scores + b * (pop + 8);
  double *scores = p.lds_scores ? lds_rest : g_scores;
  double *agents = p.lds_pop ? lds_rest + pop + 8 : g_agents;
  double *trial = p.lds_pop ? agents + pop * D : p.trial + b * (D + 8);
  if (p.lds_pop && c.phase == 1)
    for (uint64_t k = lane; k < pop * D; k += 64) agents[k] = g_agents[k];
  if (p.lds_scores && c.phase == 1)
    for (uint64_t k = lane; k < pop; k += 64) scores[k] = g_scores[k];
  if (p.lds_scores)
    for (uint64_t k = pop + lane; k < pop + 8; k += 64) scores[k] = 0.0;  // (serial_chain_lds reads past)

  DeRefStream s;
  s.ring = ring;
  s.jump = jump;
  s.H = 0;
  s.P = 0;
  s.st0 = c.s0;
  s.st1 = c.s1;
  for (int k = 0; k < lane; k++) xorshift_step(s.st0, s.st1);  // lane l: S_l
  __syncthreads();

  auto finish = [&](int32_t err) {
    c.err = err;
    c.phase = 2;
    for (uint64_t d = lane; d < D; d += 64) p.x[b * D + d] = agents[c.best_id * D + d];  // :2444
    c.f_value = scores[c.best_id];
  };

  if (c.phase == 0) {
    // init_agents / generate_sequence (2302-2323): (u - 0.5) * x0[d], agent-major draw order
    const uint64_t n = pop * D;
    for (uint64_t k0 = 0; k0 < n; k0 += 64) {
      s.ensure(64);
      const uint64_t k = k0 + static_cast<uint64_t>(lane);
      if (k < n) agents[k] = (s.at(s.P + lane) - 0.5) * p.x[b * D + k % D];
      s.P += n - k0 < 64 ? n - k0 : 64;
    }
    __syncthreads();
    for (uint64_t a = 0; a < pop; a++) {  // :2423-2425
      const double f = de_ref_objective<OBJ>(agents + a * D, D, tb);
      if (p.log_cap) de_ref_log<OBJ>(p, c, b, agents + a * D, f);
      else c.log_count++;
      if (lane == 0) scores[a] = p.fmul * f;
    }
    __syncthreads();
    c.fcalls = pop;
    c.iter = 0;
    c.best_id = 0;
    c.val_no_change = 0;
    c.phase = 1;
  }

  for (uint64_t g = 0; c.phase == 1; g++) {
    if (g == p.gens) break;  // (between generations: the next launch starts with the best scan)
    // best scan (2432-2437): the running strict '<' against the incumbent ends on the first index
    // of the minimum if that minimum is strictly below the incumbent's score, else on the incumbent
    double mnv = __builtin_inf();
    uint64_t mni = ~0ull;
    for (uint64_t i = lane; i < pop; i += 64) argmin_combine(mnv, mni, scores[i], i);
    butterfly_levels<32>([&](auto off) {
      constexpr int o = decltype(off)::value;
      const double ov = lane_xor<o>(mnv);
      const uint64_t oi = lane_xor<o>(mni);
      argmin_combine(mnv, mni, ov, oi);
    });
    bool not_updated = true;
    if (mni != ~0ull && mnv < scores[c.best_id]) {
      c.best_id = mni;
      not_updated = false;
    }
    c.val_no_change = not_updated ? c.val_no_change + 1 : 0;  // :2439
    c.std_err = de_ref_std_err(scores, pop);
    if (c.iter >= p.max_iter || c.val_no_change >= p.best_val_no_change || c.std_err < p.eps) {  // :2441-2447
      finish(kDeRefErrNone);
      break;
    }
    int32_t err = kDeRefErrNone;
    for (uint64_t i = 0; i < pop; i++) {  // :2449
      uint64_t ids[4];
      err = de_ref_donors(p.strategy == NLSG_DE_RANDOM ? i : c.best_id, pop, [&]() { return s.next(); }, ids);
      if (err != kDeRefErrNone) break;
      // propose_new_agent (2357-2375): forced dimension, then one draw per coordinate
      const uint64_t dim = static_cast<uint64_t>(s.next() * static_cast<double>(D));  // (== D: none forced)
      const double *r0 = agents + ids[0] * D, *r1 = agents + ids[1] * D, *r2 = agents + ids[2] * D,
                   *r3 = agents + ids[3] * D;
      for (uint64_t d0 = 0; d0 < D; d0 += 64) {
        s.ensure(64);
        const uint64_t d = d0 + static_cast<uint64_t>(lane);
        if (d < D) {
          const double u = s.at(s.P + lane);
          trial[d] = (u < p.CR || d == dim) ? r1[d] + p.F * (r2[d] - r3[d]) : r0[d];
        }
        s.P += D - d0 < 64 ? D - d0 : 64;
      }
      __syncthreads();
      const double f = de_ref_objective<OBJ>(trial, D, tb);
      if (p.log_cap) de_ref_log<OBJ>(p, c, b, trial, f);
      else c.log_count++;
      const double score = p.fmul * f;  // :2463
      c.fcalls++;
      if (score < scores[i]) {  // :2466-2471
        for (uint64_t d = lane; d < D; d += 64) agents[i * D + d] = trial[d];
        __syncthreads();
        if (lane == 0) scores[i] = score;
      }
      __syncthreads();
    }
    if (err != kDeRefErrNone) {
      finish(err);
      break;
    }
    c.iter++;
  }

  // leave the state for the next launch (or the caller)
  if (s.P > 0) {
    const uint64_t slot = (s.P - 1) & (kDeRefRing - 1);
    c.s0 = ring[2 * slot];
    c.s1 = ring[2 * slot + 1];
  }
  if (c.phase == 1) {
    if (p.lds_pop)
      for (uint64_t k = lane; k < pop * D; k += 64) g_agents[k] = agents[k];
    if (p.lds_scores)
      for (uint64_t k = lane; k < pop; k += 64) g_scores[k] = scores[k];
  }
  __syncthreads();
  if (lane == 0) {
    p.ctl[b] = c;
    if (c.phase == 2) atomicAdd(p.n_done, 1u);
  }
}

}  // namespace nlsg
