// nlsolver_amd/csrc/nlsg_pso_batch_kernels.h — gfx950 kernels of the resident batch PSO engine
// (nlsg_pso_batch_*): `batch` independent keyed solves of one shape, one 256-thread workgroup per
// solve, the swarm resident in LDS, the whole turn loop -- head (best scan of the last evaluation,
// std_err of the personal bests, no-change counter, stop tests), then the move -- inside one kernel.
//
// Solve b is bit-identical to the turn engine (nlsg_pso_kernels.h) with seed seeds[b] and bounds
// lower[b] / upper[b]: the draw layout, det_rnorm, the update expressions, the objective trees, the
// argmin and std_err below restate that engine's kernels line by line; pso_apply_pending,
// pso_finish_turn and pso_inertia_at ARE its functions (nlsg_pso_state.h).
//   pso_batch_init_kernel   pso_reset_state_kernel + pso_init_kernel per solve (rows to HBM)
//   pso_batch_kernel        at most `turns` turns of every solve that is not done
//
// LDS of a workgroup (doubles, every array at an even offset = 16-byte aligned):
//   [state 8][red 4][mv 4][mi 4][row, copy 4] gbest_x[S] lower[S] upper[S] pbest_val[n'] cur_val[n']
//   (Accelerated) rn_tab[512]  pos[n][S]  (Vanilla) vel[n][S] pbest_pos[n][S]
// with S = D rounded up to even and n' = n rounded up to even. A lane holds coordinates 2g, 2g + 1
// of its particle: with an even stride the pair is one aligned 16-byte access (ds_read_b128 /
// ds_write_b128), and the lanes of a wave read consecutive 16-byte slots of a row, rows of one
// pass back to back -- no two lanes of a lane group meet on a bank unless they read the same row
// of different arrays, which are separate instructions. Nothing gathers across rows (a particle is
// read and written by its own lanes only and meets the others through gbest_x alone), so the odd
// stride of the DE engine would buy nothing and would cost the alignment. The move is in place.
// The pad column of an odd D holds 0.0 and is masked on every read.
// Between launches the state waits in HBM: rows [batch][n][D] (unpadded), values, gbest_x, bounds
// and PsoState per solve.
// A user objective with run-time parameters (NLSG_N_PARAMS, nlsg_common.h) adds its solve's row
// as static LDS in front of this block -- a multiple of 16 bytes, so the alignment above holds;
// both kernels stage it before the first evaluation.
#pragma once

#include "nlsg_pso_state.h"

namespace nlsg {

constexpr uint64_t kPsoBatchMaxN = kTile;    // one reduction tile: std_err is the two-pass formula
constexpr uint64_t kPsoBatchMaxDim = 128;    // one register chunk per lane, both mappings
constexpr uint64_t kPsoBatchLdsBudget = 160 * 1024;  // what gfx950 gives one workgroup
constexpr uint64_t kPsoBatchHeaderDoubles = 24;

__host__ __device__ inline uint64_t pso_batch_even(uint64_t v) { return (v + 1) & ~1ull; }
// dynamic LDS of one workgroup; 0: the shape is outside the engine's ranges
__host__ __device__ inline uint64_t pso_batch_lds_bytes(uint64_t n, uint64_t D, int type) {
  if (n < 1 || n > kPsoBatchMaxN || D < 1 || D > kPsoBatchMaxDim) return 0;
  if (type != NLSG_PSO_VANILLA && type != NLSG_PSO_ACCELERATED) return 0;
  const uint64_t S = pso_batch_even(D), np = pso_batch_even(n);
  const bool accel = type == NLSG_PSO_ACCELERATED;
  return 8 * (kPsoBatchHeaderDoubles + 3 * S + 2 * np + (accel ? static_cast<uint64_t>(kRnormTabDoubles) : 0) +
              (accel ? 1 : 3) * n * S);
}

// q holds the shape and the coefficients (n = shard_n, shard_lo = 0, seed unused) and the arrays of
// ALL solves: pos / vel / pbest_pos [batch][n][D], pbest_val / cur_val [batch][n], gbest_x / lower /
// upper [batch][D], state [batch]; inertia_tab is the engine's one table.
struct PsoBatchParams {
  PsoParams q;
  const uint64_t *seeds;  // [batch]
  uint32_t *n_done;       // solves whose stop test has fired since the last init
  uint64_t batch;
  const double *params;   // [batch][n_params] run-time objective parameters, or null (n_params == 0)
};

// ---- pso_reset_state_kernel + pso_init_kernel of solve blockIdx.x / blocks_per --------------------
template <int OBJ>
__global__ __launch_bounds__(256) void pso_batch_init_kernel(PsoBatchParams p, uint32_t blocks_per) {
  const uint64_t b = blockIdx.x / blocks_per;
  const uint32_t blk = blockIdx.x - static_cast<uint32_t>(b) * blocks_per;
  const uint64_t n = p.q.shard_n, D = p.q.D;
  if (blk == 0 && threadIdx.x == 0) {
    PsoState *s = p.q.state + b;
    s->gbest_val = __builtin_inf();
    s->gbest_idx = 0;
    s->iter = 0;
    s->val_no_change = 0;
    s->fevals = 0;
    s->std_err = __builtin_nan("");
    s->done = 0;
    s->pending = 0;
  }
  stage_custom_params(p.params, b, true);  // (a user objective with parameters; else nothing)
  const uint64_t i = static_cast<uint64_t>(blk) * 4 +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  if (i >= n) return;
  const int lane = lane_id();
  const double *__restrict__ lower = p.q.lower + b * D;
  const double *__restrict__ upper = p.q.upper + b * D;
  const uint64_t kp = ctr_key(ctr_key(p.seeds[b], 0), i);
  double xv[1][2], vv[1][2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint64_t e = 2 * static_cast<uint64_t>(lane) + k;
    const double lo = e < D ? lower[e] : 0.0, hi = e < D ? upper[e] : 0.0;
    const double temp = fabs(hi - lo);  // :2645
    xv[0][k] = lo + ((hi - lo) * u01(ctr_key(kp, 2 * e)));
    vv[0][k] = -temp + (u01(ctr_key(kp, 2 * e + 1)) * temp);
    if (e >= D) xv[0][k] = 0.0;
  }
  const uint64_t off = (b * n + i) * D;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint64_t e = 2 * static_cast<uint64_t>(lane) + k;
    if (e < D) {
      p.q.pos[off + e] = xv[0][k];
      if (p.q.type == NLSG_PSO_VANILLA) {
        p.q.vel[off + e] = vv[0][k];
        p.q.pbest_pos[off + e] = xv[0][k];  // :2652
      }
    }
  }
  const double f = p.q.fmul * wave_objective<OBJ, 1>(xv, D);
  if (lane == 0) {
    p.q.cur_val[b * n + i] = f;
    // +inf sentinel (B8), as pso_init_kernel: a NaN or +inf first value does not win
    p.q.pbest_val[b * n + i] = f < __builtin_inf() ? f : __builtin_inf();
  }
}

// ---- head of a turn: pso_scan_partial / pso_local / pso_var_partial / pso_var_local /
// pso_pack_record / pso_finalize (eps > 0) or pso_scan_head (eps <= 0) for a swarm of one tile on
// one device (shard_lo = 0, shard_n = n, ntiles = 1, world = 1). The turn engine's second level
// then reduces ONE partial: thread 0 adds it to +0.0, the other threads carry +0.0 through the
// same tree, and a sum that started from +0.0 is never -0, so 0.0 + total == total and
// 0.0 + m2 == m2 bit for bit (a NaN keeps its payload through the add); the finaliser's
// `0.0 + rec[2]`, `0.0 + rec[3]` are the same identity and with world == 1 it adds no
// between-shard term. Its mean total / n is pso_local_kernel's total / shard_n. So the second
// level is not repeated here. All 256 threads call it; it ends with a barrier after which st
// and gbest_x are the head's.
__device__ inline void pso_batch_head(const PsoParams &q, PsoState *st, const double *pbest_val,
                                      const double *cur_val, const double *pos, uint32_t S,
                                      double *gbest_x, double *red, double *mv, uint64_t *mi,
                                      uint64_t *row_copy) {
  const bool need_se = q.eps > 0;
  const uint64_t n = q.shard_n;
  if (threadIdx.x == 0) pso_apply_pending(st);
  double acc = 0.0;
  double bv = __builtin_inf();
  uint64_t bi = ~0ull;
  for (uint64_t i = threadIdx.x; i < n; i += 256) {
    acc = acc + pbest_val[i];
    argmin_combine(bv, bi, cur_val[i], i);
  }
  double m2 = 0.0;
  if (need_se) {
    const double total = block_tree_256(acc, red);
    const double mean = total / static_cast<double>(n);
    acc = 0.0;
    for (uint64_t i = threadIdx.x; i < n; i += 256) {
      const double d = pbest_val[i] - mean;
      acc = acc + d * d;
    }
    m2 = block_tree_256(acc, red);
  }
  block_argmin_256(bv, bi, mv, mi);
  if (threadIdx.x == 0) {
    // std_err(particle_best_values), :2601
    const double se = need_se ? sqrt(m2 / static_cast<double>(q.n - 1)) : __builtin_nan("");
    const bool have = bi != ~0ull;
    const bool upd = pso_finish_turn(st, q, have, bv, bi, se);
    row_copy[0] = bi;
    row_copy[1] = upd ? 1 : 0;
  }
  __syncthreads();
  if (row_copy[1]) {  // swarm_best_position = positions[best], :2737
    const double *row = pos + static_cast<uint32_t>(row_copy[0]) * S;
    for (uint32_t d = threadIdx.x; d < q.D; d += 256) gbest_x[d] = row[d];
  }
  __syncthreads();
}

// ---- the move: pso_move_groups_kernel (G = 4 / 8 / 16 / 32, D <= 2 G: 64 / G particles per wave)
// and pso_move_kernel<., 1, ., .> (G = 64: one wave per particle, 64 < D <= 128) on LDS rows. The
// four waves walk the swarm in passes of 4 * 64 / G particles. The lane's two coordinates 2g,
// 2g + 1 are one 16-byte access.
template <int OBJ, int G, int TYPE>
__device__ inline void pso_batch_move(const PsoParams &q, uint64_t seed, uint64_t iter, double *pos,
                                      double *vel, double *pbest_pos, uint32_t S, double *pbest_val,
                                      double *cur_val, const double *gbest_x, const double *lower,
                                      const double *upper, const double *rn_tab) {
  constexpr int P = 64 / G;
  const uint64_t n = q.shard_n, D = q.D;
  const uint32_t wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int lane = lane_id(), g = lane & (G - 1), gi = lane / G;
  const uint64_t kit = ctr_key(seed, iter + 1);
  const uint32_t j0 = 2 * g;
  const bool in[2] = {j0 < D, j0 + 1 < D};
  const bool slot = j0 < S;  // the lane's 16-byte slot lies inside the row
  auto load2 = [&](const double *rp, bool on, double (&v)[2]) {
    double2 t = make_double2(0.0, 0.0);
    if (on && slot) t = *reinterpret_cast<const double2 *>(rp + j0);
    v[0] = in[0] ? t.x : 0.0;
    v[1] = in[1] ? t.y : 0.0;
  };
  double gb[2], lo[2], hi[2];
  load2(gbest_x, true, gb);
  load2(lower, q.bounded != 0, lo);
  load2(upper, q.bounded != 0, hi);
  double inertia = q.inertia;
  if (TYPE == NLSG_PSO_ACCELERATED)  // :2613 inertia = pow(init_inertia, iter)
    inertia = pso_inertia_at(q, iter);
  for (uint64_t wave = wid; wave * P < n; wave += 4) {
    const bool live = wave * P + gi < n;
    const uint64_t i = live ? wave * P + gi : wave * P;  // idle groups shadow a live particle
    const uint64_t kp = ctr_key(kit, i);
    const uint32_t off = static_cast<uint32_t>(i) * S;
    double xv[2], vv[2], pb[2];
    load2(pos + off, true, xv);
    load2(vel + off, TYPE == NLSG_PSO_VANILLA, vv);
    load2(pbest_pos + off, TYPE == NLSG_PSO_VANILLA, pb);
    const double old_pbest = pbest_val[i];
    // draws 2e and 2e+1 of element e = 2g + k: mix64(kp + G64 (2e + 1 [+ 1])), 2e + 1 = 4g + 2k + 1
    const uint64_t kp_lane = kp + kGolden * (4 * static_cast<uint64_t>(g) + 1);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint64_t z1 = mix64(kp_lane + kGolden * static_cast<uint64_t>(2 * k));
      const double u1 = u01(z1);
      const double u2 = TYPE == NLSG_PSO_ACCELERATED
                            ? u01_low32(z1)
                            : u01(mix64(kp_lane + kGolden * static_cast<uint64_t>(2 * k + 1)));
      double pnew;
      if (TYPE == NLSG_PSO_ACCELERATED) {
        const double rn = det_rnorm(z1, rn_tab);  // rnorm, :2479-2485
        pnew = inertia * rn + (1 - q.cog) * xv[k] + q.soc * gb[k];  // :2693-2697
      } else {
        // intended Vanilla update (B7 repaired): pbest[j] - pos, gbest[j] - pos
        vv[k] = (inertia * vv[k]) + q.cog * u1 * (pb[k] - xv[k]) + q.soc * u2 * (gb[k] - xv[k]);
        pnew = xv[k] + vv[k];  // :2683
      }
      if (q.bounded) {  // :2701-2715
        pnew = pnew < lo[k] ? lo[k] : pnew;
        pnew = pnew > hi[k] ? hi[k] : pnew;
      }
      xv[k] = in[k] ? pnew : 0.0;
      vv[k] = in[k] ? vv[k] : 0.0;
    }
    double f;
    if constexpr (G == 64) {
      const double row[1][2] = {{xv[0], xv[1]}};
      f = q.fmul * wave_objective<OBJ, 1>(row, D);
    } else {
      f = q.fmul * group_objective<OBJ, G>(xv[0], xv[1], D);
    }
    const bool better = f < old_pbest;  // :2733-2735
    if (live) {
      if (slot) {
        *reinterpret_cast<double2 *>(pos + off + j0) = make_double2(xv[0], xv[1]);
        if (TYPE == NLSG_PSO_VANILLA) {
          *reinterpret_cast<double2 *>(vel + off + j0) = make_double2(vv[0], vv[1]);
          if (better) *reinterpret_cast<double2 *>(pbest_pos + off + j0) = make_double2(xv[0], xv[1]);
        }
      }
      if (g == 0) {
        cur_val[i] = f;
        if (better) pbest_val[i] = f;
      }
    }
  }
}

// rows [n][D] in HBM <-> [n][S] in LDS (the pad column of an odd D is written 0.0 on the way in)
__device__ inline void pso_batch_rows_in(double *dst, const double *__restrict__ src, uint32_t n,
                                         uint32_t D, uint32_t S) {
  for (uint32_t r = threadIdx.x / D, c = threadIdx.x % D; r < n;) {
    dst[r * S + c] = src[r * D + c];
    c += 256 % D;
    r += 256 / D;
    if (c >= D) {
      c -= D;
      r++;
    }
  }
  if (S != D)
    for (uint32_t r = threadIdx.x; r < n; r += 256) dst[r * S + D] = 0.0;
}
__device__ inline void pso_batch_rows_out(double *__restrict__ dst, const double *src, uint32_t n,
                                          uint32_t D, uint32_t S) {
  for (uint32_t r = threadIdx.x / D, c = threadIdx.x % D; r < n;) {
    dst[r * D + c] = src[r * S + c];
    c += 256 % D;
    r += 256 / D;
    if (c >= D) {
      c -= D;
      r++;
    }
  }
}

// G = 4 / 8 / 16 / 32: the packed mapping for D <= 8 / 16 / 32 / 64; G = 64: one wave per particle
// (64 < D <= 128) -- the turn engine's two mappings. Grid = batch, 256 threads, dynamic LDS
// pso_batch_lds_bytes(n, D, TYPE). Every barrier is reached by all 256 threads: the loop's exits
// test st->done, which thread 0 writes before the barrier that ends pso_batch_head.
template <int OBJ, int G, int TYPE>
__global__ __launch_bounds__(256) void pso_batch_kernel(PsoBatchParams p, uint64_t turns) {
  extern __shared__ __attribute__((aligned(16))) double pso_batch_lds[];
  constexpr bool kVanilla = TYPE == NLSG_PSO_VANILLA;
  const PsoParams &q = p.q;
  const uint64_t b = blockIdx.x;
  const uint32_t n = static_cast<uint32_t>(q.shard_n), D = static_cast<uint32_t>(q.D);
  const uint32_t S = static_cast<uint32_t>(pso_batch_even(D));
  const uint32_t np = static_cast<uint32_t>(pso_batch_even(n));
  PsoState *st = reinterpret_cast<PsoState *>(pso_batch_lds);  // 7 doubles
  double *red = pso_batch_lds + 8, *mv = pso_batch_lds + 12;
  uint64_t *mi = reinterpret_cast<uint64_t *>(pso_batch_lds + 16);
  uint64_t *row_copy = reinterpret_cast<uint64_t *>(pso_batch_lds + 20);
  double *gbest_x = pso_batch_lds + kPsoBatchHeaderDoubles;
  double *lower = gbest_x + S, *upper = lower + S;
  double *pbest_val = upper + S, *cur_val = pbest_val + np;
  double *rn_tab = cur_val + np;
  double *pos = rn_tab + (kVanilla ? 0 : kRnormTabDoubles);
  double *vel = kVanilla ? pos + n * S : pos;           // (Accelerated: never dereferenced)
  double *pbest_pos = kVanilla ? vel + n * S : pos;
  if (threadIdx.x == 0) *st = q.state[b];
  __syncthreads();
  if (st->done) return;  // a finished solve is a no-op (uniform: read after the barrier)
  if (!kVanilla) rnorm_table_to_lds(rn_tab);
  {
    const uint64_t rows = b * n * D;
    pso_batch_rows_in(pos, q.pos + rows, n, D, S);
    if (kVanilla) {
      pso_batch_rows_in(vel, q.vel + rows, n, D, S);
      pso_batch_rows_in(pbest_pos, q.pbest_pos + rows, n, D, S);
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
      pbest_val[i] = q.pbest_val[b * n + i];
      cur_val[i] = q.cur_val[b * n + i];
    }
    for (uint32_t i = threadIdx.x; i < S; i += 256) {
      gbest_x[i] = i < D ? q.gbest_x[b * D + i] : 0.0;
      lower[i] = i < D ? q.lower[b * D + i] : 0.0;
      upper[i] = i < D ? q.upper[b * D + i] : 0.0;
    }
    stage_custom_params(p.params, b, false);  // once per launch, published by the barrier below
  }
  __syncthreads();
  const uint64_t seed = p.seeds[b];
  for (uint64_t t = 0; t < turns; t++) {
    pso_batch_head(q, st, pbest_val, cur_val, pos, S, gbest_x, red, mv, mi, row_copy);
    if (st->done) break;
    pso_batch_move<OBJ, G, TYPE>(q, seed, st->iter, pos, vel, pbest_pos, S, pbest_val, cur_val,
                                 gbest_x, lower, upper, rn_tab);
    __syncthreads();
  }
  // between launches the solve stands settled, as pso_settle_kernel leaves it for the host
  if (threadIdx.x == 0) {
    pso_apply_pending(st);
    q.state[b] = *st;
    if (st->done) __hip_atomic_fetch_add(p.n_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  {
    const uint64_t rows = b * n * D;
    pso_batch_rows_out(q.pos + rows, pos, n, D, S);
    if (kVanilla) {
      pso_batch_rows_out(q.vel + rows, vel, n, D, S);
      pso_batch_rows_out(q.pbest_pos + rows, pbest_pos, n, D, S);
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
      q.pbest_val[b * n + i] = pbest_val[i];
      q.cur_val[b * n + i] = cur_val[i];
    }
    for (uint32_t i = threadIdx.x; i < D; i += 256) q.gbest_x[b * D + i] = gbest_x[i];
  }
}

}  // namespace nlsg
