// nlsolver_amd/csrc/nlsg_de_batch_kernels.h — gfx950 kernels of the resident batch DE engine
// (nlsg_de_batch_*): `batch` independent keyed solves of one shape, one 256-thread workgroup per
// solve, population and scores resident in LDS, the whole turn loop -- head k (best scan, std_err,
// no-change counter, stop tests), then generation k + 1 -- inside one kernel.
//
// Solve b is bit-identical to the turn engine (nlsg_de_kernels.h) with seed seeds[b]: the draw
// layout, donor picks, crossover test, trial arithmetic, objective trees, argmin, incumbent rule
// and std_err below are that engine's own code or restate it line by line; head_position and
// finish_turn ARE its functions.
//   de_batch_init_kernel   de_reset_state_kernel + de_init_kernel per solve (rows to HBM)
//   de_batch_kernel        at most `turns` turns of every solve that is not done
//
// LDS of a workgroup (doubles): [state 8][red 4][mv 4][mi 4][spare 4] best_x[D] scores[pop]
// rows[2][pop][S], S = D | 1: an odd row stride, so the rows a wave's donor gathers touch at the
// same columns start 2 S dwords apart and walk all 32 even bank offsets instead of hitting the
// same banks (S = D = 8: four offsets, 16 agents per wave on them). The generation is
// synchronous: it reads rows[cur] and writes every agent's survivor -- the accepted trial or the
// old row -- into rows[cur ^ 1]; an agent's score is read and rewritten by its own lanes only, so
// one score vector is enough. Nothing is speculative here: a head that fires a stop test ends
// the solve's loop before the generation, and the state freezes where the turn engine freezes it.
// Between launches the state waits in HBM: rows [batch][pop][D] (unpadded), scores, best_x,
// DeState per solve.
// A user objective with run-time parameters (NLSG_N_PARAMS, nlsg_common.h) adds its solve's row
// as static LDS in front of this block; both kernels stage it before the first evaluation.
#pragma once

#include "nlsg_de_state.h"

namespace nlsg {

constexpr uint64_t kDeBatchMaxPop = kTile;  // one reduction tile: std_err is the two-pass formula
constexpr uint64_t kDeBatchMaxDim = 128;    // one register chunk per lane, both mappings
constexpr uint64_t kDeBatchLdsBudget = 160 * 1024;  // what gfx950 gives one workgroup
constexpr uint64_t kDeBatchHeaderDoubles = 24;

__host__ __device__ inline uint64_t de_batch_stride(uint64_t D) { return D | 1ull; }
// dynamic LDS of one workgroup; 0: the shape is outside the engine's ranges
__host__ __device__ inline uint64_t de_batch_lds_bytes(uint64_t pop, uint64_t D) {
  if (pop < 4 || pop > kDeBatchMaxPop || D < 1 || D > kDeBatchMaxDim) return 0;
  return 8 * (kDeBatchHeaderDoubles + D + pop + 2 * pop * de_batch_stride(D));
}

struct DeBatchParams {
  double *rows;           // [batch][pop][D] current generation of every solve
  double *scores;         // [batch][pop]
  double *best_x;         // [batch][D] row of best_id as of the last head
  DeState *state;         // [batch]
  const uint64_t *seeds;  // [batch]
  const double *x0;       // [batch][D]
  uint32_t *n_done;       // solves whose stop test has fired since the last init
  uint64_t batch, pop, D;
  double CR, F, eps, fmul;
  uint64_t max_iter, best_val_no_change;
  uint64_t cr_thresh;     // as DeParams.cr_thresh / cr_all
  int32_t cr_all;
  int32_t strategy;
  const double *params;   // [batch][n_params] run-time objective parameters, or null (n_params == 0)
};

// ---- generation 0: de_reset_state_kernel + de_init_kernel of solve blockIdx.x / blocks_per ----
template <int OBJ>
__global__ __launch_bounds__(256) void de_batch_init_kernel(DeBatchParams p, uint32_t blocks_per) {
  const uint64_t b = blockIdx.x / blocks_per;
  const uint32_t blk = blockIdx.x - static_cast<uint32_t>(b) * blocks_per;
  if (blk == 0 && threadIdx.x == 0) {
    DeState *s = p.state + b;
    s->best_id = 0;  // "best_id = 0" (:2428)
    s->best_f = 0.0;
    s->iter = 0;
    s->val_no_change = 0;
    s->fcalls = p.pop;
    s->std_err = __builtin_nan("");
    s->done = 0;
    s->parity = 0;
    s->pad[0] = s->pad[1] = 0;
  }
  stage_custom_params(p.params, b, true);  // (a user objective with parameters; else nothing)
  const uint64_t a = static_cast<uint64_t>(blk) * 4 +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (a >= p.pop) return;
  const int lane = lane_id();
  const double *__restrict__ x0 = p.x0 + b * p.D;
  const uint64_t ka = ctr_key(ctr_key(p.seeds[b], 0), a);
  double xv[1][2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint64_t e = 2 * static_cast<uint64_t>(lane) + k;
    // generate_sequence, nlsolver.h:2309: (u - 0.5) * offset[i]
    xv[0][k] = (e < p.D) ? (u01(ctr_key(ka, e)) - 0.5) * x0[e] : 0.0;
  }
  double *row = p.rows + (b * p.pop + a) * p.D;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint64_t e = 2 * static_cast<uint64_t>(lane) + k;
    if (e < p.D) row[e] = xv[0][k];
  }
  const double f = p.fmul * wave_objective<OBJ, 1>(xv, p.D);  // :2423-2425
  if (lane == 0) p.scores[b * p.pop + a] = f;
}

// ---- head k: de_scan_head_block for a population of one tile on one device ----------------------
// (shard_lo = 0, shard_n = pop, ntiles = 1). The turn engine's last block then merges one
// partial: its argmin pass returns the tile's pair unchanged, and its std_err merge adds zeros
// and a between-tile term of exactly 0 (the tile mean IS the mean) to the tile's M2, which is a
// sum of squares (never -0): m2 == tile_m2 bit for bit, so the merge is not repeated here.
// All 256 threads call it; it ends with a barrier after which st and best_x are the head's.
__device__ inline void de_batch_head(const DeBatchParams &p, DeState *st, const double *sc,
                                     const double *rows, uint32_t S, double *best_x, uint64_t k,
                                     double *red, double *mv, uint64_t *mi) {
  const bool need_se = p.eps > 0;
  const uint64_t tile_n = p.pop;
  double v[kTile / 256];
  double acc = 0.0;
  double bv = __builtin_inf();
  uint64_t bi = ~0ull;
#pragma unroll
  for (int q = 0; q < kTile / 256; q++) {
    const uint64_t i = threadIdx.x + 256u * q;
    v[q] = sc[i < tile_n ? i : 0];  // clamped, masked below
  }
#pragma unroll
  for (int q = 0; q < kTile / 256; q++) {
    const uint64_t i = threadIdx.x + 256u * q;
    if (i < tile_n) {
      acc = acc + v[q];
      argmin_combine(bv, bi, v[q], i);
    }
  }
  double tile_m2 = 0.0;
  if (need_se) {
    const double tile_sum = block_tree_256(acc, red);
    const double tile_mean = tile_sum / static_cast<double>(tile_n);  // :2044
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
    head_position(st, p, k);
    // the reference's tie rule (strict '<' scan starting from the incumbent, nlsolver.h:2432-2437)
    const uint64_t inc = st->best_id;
    uint64_t gi = (bi == ~0ull) ? inc : bi;
    const double inc_score = sc[inc];
    if (!(bv < inc_score)) {
      gi = inc;
      bv = inc_score;
    }
    finish_turn(st, p, gi, bv, true,
                need_se ? sqrt(tile_m2 / static_cast<double>(p.pop - 1))  // :2050-2051
                        : __builtin_nan(""));
  }
  __syncthreads();
  const double *row = rows + st->best_id * S;  // x = agents[best_id], :2444
  for (uint32_t d = threadIdx.x; d < p.D; d += 256) best_x[d] = row[d];
  __syncthreads();
}

// ---- generation, D <= 64: de_generation_groups_block on LDS rows -------------------------------
// 64 / G agents per wave; the four waves walk the population in passes of 4 * 64 / G agents.
template <int OBJ, int G>
__device__ inline void de_batch_generation(const DeBatchParams &p, uint64_t seed, uint64_t generation,
                                           uint64_t best_id, const double *cur, double *nxt,
                                           uint32_t S, double *sc, const double *best_x) {
  constexpr int P = 64 / G;
  const uint64_t n = p.pop, D = p.D;
  const uint32_t wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int lane = lane_id(), g = lane & (G - 1), gi = lane / G;
  const bool rnd = p.strategy == NLSG_DE_RANDOM;
  const uint64_t kg = ctr_key(seed, generation);
  const uint32_t j0 = 2 * g, j1 = 2 * g + 1;
  const bool in0 = j0 < D, in1 = j1 < D;
  for (uint64_t wave = wid; wave * P < n; wave += 4) {
    const bool live = wave * P + gi < n;
    const uint64_t a = live ? wave * P + gi : wave * P;  // idle groups shadow a live agent
    const uint64_t ka = ctr_key(kg, a);
    const uint64_t fixed = rnd ? a : best_id;  // :2451-2457
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
      const uint64_t cand = clamp_index(u01(__shfl(drawn, base + (pos & (G - 1)), 64)), n);
      const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
      const bool take = !used && have < 3;
      r0 = (take && have == 0) ? cand : r0;
      r1 = (take && have == 1) ? cand : r1;
      r2 = (take && have == 2) ? cand : r2;
      have += take ? 1 : 0;
    }
    for (uint64_t cand = 0; __ballot(have < 3) != 0ull; cand++) {  // fallback: lowest unused
      const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
      const bool take = !used && have < 3;
      r0 = (take && have == 0) ? cand : r0;
      r1 = (take && have == 1) ? cand : r1;
      r2 = (take && have == 2) ? cand : r2;
      have += take ? 1 : 0;
    }
    // the crossover mask of propose_new_agent (nlsolver.h:2357-2375) on the draw's bits
    bool cross[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint64_t zc = ctr_key(ka, 2 * static_cast<uint64_t>(g) + k);
      cross[k] = zc < p.cr_thresh || p.cr_all || 2 * static_cast<uint64_t>(g) + k == jrand;
    }
    auto load2 = [&](const double *rp, double (&v)[2]) {
      v[0] = in0 ? rp[j0] : 0.0;
      v[1] = in1 ? rp[j1] : 0.0;
    };
    double d1[2], d2[2], d3[2], own[2];
    load2(cur + static_cast<uint32_t>(r0) * S, d1);
    load2(cur + static_cast<uint32_t>(r1) * S, d2);
    load2(cur + static_cast<uint32_t>(r2) * S, d3);
    load2(cur + static_cast<uint32_t>(a) * S, own);
    // where the trial keeps the old coordinate: the agent's own row (strategy random) or the row
    // of best_id as the head left it (strategy best)
    double keep[2];
    keep[0] = rnd ? own[0] : (in0 ? best_x[j0] : 0.0);
    keep[1] = rnd ? own[1] : (in1 ? best_x[j1] : 0.0);
    const double old_score = sc[a];
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
      double *out = nxt + static_cast<uint32_t>(a) * S;
      if (in0) out[j0] = accept ? trial[0] : own[0];
      if (in1) out[j1] = accept ? trial[1] : own[1];
      if (g == 0) sc[a] = accept ? score : old_score;
    }
  }
}

// ---- generation, 64 < D <= 128: one wave per agent (de_fetch_agent + de_process_agent, one chunk;
// the donor pick is the literal loop those restate with ballots: the same candidates in the same
// order). The four waves walk the population four agents at a time.
template <int OBJ>
__device__ inline void de_batch_generation_waves(const DeBatchParams &p, uint64_t seed,
                                                 uint64_t generation, uint64_t best_id,
                                                 const double *cur, double *nxt, uint32_t S,
                                                 double *sc, const double *best_x) {
  const uint64_t n = p.pop, D = p.D;
  const uint32_t wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int lane = lane_id();
  const bool rnd = p.strategy == NLSG_DE_RANDOM;
  const uint64_t kg = ctr_key(seed, generation);
  const uint32_t j0 = 2 * lane, j1 = 2 * lane + 1;
  const bool in0 = j0 < D, in1 = j1 < D;
  for (uint64_t a = wid; a < n; a += 4) {
    const uint64_t ka = ctr_key(kg, a);
    // lane L takes draw D + L of the agent's stream: lane 0 the crossover's jrand (:2364), lane
    // 1 + k donor candidate k
    const uint64_t drawn = clamp_index(u01(ctr_key(ka, D + static_cast<uint64_t>(lane))), lane == 0 ? D : n);
    const uint64_t jrand = readlane64(drawn, 0);
    const uint64_t fixed = rnd ? a : best_id;  // :2451-2457
    uint64_t r0 = ~0ull, r1 = ~0ull, r2 = ~0ull;
    int have = 0;
    for (int k = 0; k < kDeMaxTries && have < 3; k++) {
      // (candidate 63 has no lane: after 61 rejections it is drawn the slow way)
      const uint64_t cand = k < 63 ? readlane64(drawn, k + 1) : clamp_index(u01(ctr_key(ka, D + 1 + k)), n);
      const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
      if (!used) {
        if (have == 0) r0 = cand;
        else if (have == 1) r1 = cand;
        else r2 = cand;
        have++;
      }
    }
    for (uint64_t cand = 0; have < 3; cand++) {  // fallback: lowest unused
      const bool used = (cand == fixed) || (have > 0 && cand == r0) || (have > 1 && cand == r1);
      if (!used) {
        if (have == 0) r0 = cand;
        else if (have == 1) r1 = cand;
        else r2 = cand;
        have++;
      }
    }
    bool cross[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint64_t e = 2 * static_cast<uint64_t>(lane) + k;
      cross[k] = ctr_key(ka, e) < p.cr_thresh || p.cr_all || e == jrand;
    }
    auto load2 = [&](const double *rp, double (&v)[2]) {
      v[0] = in0 ? rp[j0] : 0.0;
      v[1] = in1 ? rp[j1] : 0.0;
    };
    double d1[2], d2[2], d3[2], own[2];
    load2(cur + static_cast<uint32_t>(r0) * S, d1);
    load2(cur + static_cast<uint32_t>(r1) * S, d2);
    load2(cur + static_cast<uint32_t>(r2) * S, d3);
    load2(cur + static_cast<uint32_t>(a) * S, own);
    double keep[2];
    keep[0] = rnd ? own[0] : (in0 ? best_x[j0] : 0.0);
    keep[1] = rnd ? own[1] : (in1 ? best_x[j1] : 0.0);
    const double old_score = sc[a];
    double trial[1][2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const double mut = d1[k] + p.F * (d2[k] - d3[k]);
      const double t = cross[k] ? mut : keep[k];
      trial[0][k] = (k ? in1 : in0) ? t : 0.0;
    }
    const double score = p.fmul * wave_objective<OBJ, 1>(trial, D);  // :2463
    const bool accept = score < old_score;                           // :2466 (NaN -> keep)
    double *out = nxt + static_cast<uint32_t>(a) * S;
    if (in0) out[j0] = accept ? trial[0][0] : own[0];
    if (in1) out[j1] = accept ? trial[0][1] : own[1];
    if (lane == 0) sc[a] = accept ? score : old_score;
  }
}

// G = 4 / 8 / 16 / 32: the packed mapping for D <= 8 / 16 / 32 / 64; G = 64: one wave per agent
// (64 < D <= 128) -- the turn engine's two mappings. Grid = batch, 256 threads, dynamic LDS
// de_batch_lds_bytes(pop, D). Every barrier is reached by all 256 threads: the loop's exits test
// st->done, which thread 0 writes before the barrier that ends de_batch_head.
template <int OBJ, int G>
__global__ __launch_bounds__(256) void de_batch_kernel(DeBatchParams p, uint64_t turns) {
  extern __shared__ double de_batch_lds[];
  const uint64_t b = blockIdx.x;
  const uint32_t n = static_cast<uint32_t>(p.pop), D = static_cast<uint32_t>(p.D);
  const uint32_t S = static_cast<uint32_t>(de_batch_stride(D));
  DeState *st = reinterpret_cast<DeState *>(de_batch_lds);  // 8 doubles
  double *red = de_batch_lds + 8, *mv = de_batch_lds + 12;
  uint64_t *mi = reinterpret_cast<uint64_t *>(de_batch_lds + 16);
  double *best_x = de_batch_lds + kDeBatchHeaderDoubles;
  double *sc = best_x + D;
  double *rows = sc + n;
  if (threadIdx.x == 0) *st = p.state[b];
  __syncthreads();
  if (st->done) return;  // a finished solve is a no-op (uniform: read after the barrier)
  {
    const double *__restrict__ src = p.rows + b * n * D;
    for (uint32_t r = threadIdx.x / D, c = threadIdx.x % D; r < n;) {
      rows[r * S + c] = src[r * D + c];
      c += 256 % D;
      r += 256 / D;
      if (c >= D) {
        c -= D;
        r++;
      }
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) sc[i] = p.scores[b * n + i];
    for (uint32_t i = threadIdx.x; i < D; i += 256) best_x[i] = p.best_x[b * D + i];
    stage_custom_params(p.params, b, false);  // once per launch, published by the barrier below
  }
  __syncthreads();
  const uint64_t seed = p.seeds[b];
  uint64_t k = st->iter;  // generations made so far = index of the next head (head_position)
  uint32_t cur = 0;
  const uint32_t buf = n * S;
  for (uint64_t t = 0; t < turns; t++) {
    de_batch_head(p, st, sc, rows + cur * buf, S, best_x, k, red, mv, mi);
    if (st->done) break;
    const uint64_t best_id = st->best_id;
    if constexpr (G == 64)
      de_batch_generation_waves<OBJ>(p, seed, k + 1, best_id, rows + cur * buf, rows + (cur ^ 1u) * buf,
                                     S, sc, best_x);
    else
      de_batch_generation<OBJ, G>(p, seed, k + 1, best_id, rows + cur * buf, rows + (cur ^ 1u) * buf, S,
                                  sc, best_x);
    __syncthreads();
    cur ^= 1u;
    k++;
  }
  // unless a stop test fired, the solve stands after the k generations it has made (de_settle_kernel)
  if (threadIdx.x == 0) {
    if (!st->done) head_position(st, p, k);
    p.state[b] = *st;
    if (st->done) __hip_atomic_fetch_add(p.n_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  {
    double *__restrict__ dst = p.rows + b * n * D;
    const double *from = rows + cur * buf;
    for (uint32_t r = threadIdx.x / D, c = threadIdx.x % D; r < n;) {
      dst[r * D + c] = from[r * S + c];
      c += 256 % D;
      r += 256 / D;
      if (c >= D) {
        c -= D;
        r++;
      }
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) p.scores[b * n + i] = sc[i];
    for (uint32_t i = threadIdx.x; i < D; i += 256) p.best_x[b * D + i] = best_x[i];
  }
}

}  // namespace nlsg
