// nlsolver_amd/csrc/nlsg_rtc.h — user objectives compiled for the device at engine creation
// (SURVEY.md §8f N3). The kernels are the SAME templates the built-in objectives use
// (nlsg_de_kernels.h, embedded as text at build time) instantiated by hiprtc around a
// user-written Objective<NLSG_OBJ_CUSTOM>; hiprtc is resolved at run time (nlsg_rtc_load).
#pragma once

#include "nlsg_common.h"

namespace nlsg {

// The loaded module of one engine. What an rtc_build_* fills is this plus the module's kernels under
// the names their launch sites use; a failed build leaves it as it was.
struct RtcModule {
  hipModule_t mod = nullptr;
};
// Unloads the module and resets the kernels with it. Every destroy calls it between drain() and
// close(): the module goes while the device is still the engine's and nothing of it is in flight.
template <typename K>
void rtc_release(K *k) {
  if (k && k->mod) hipModuleUnload(k->mod);
  if (k) *k = K();
}

struct DeRtcKernels : RtcModule {
  hipFunction_t init = nullptr, generation = nullptr, turn = nullptr;
};
// Compiles de_init / de_generation / de_turn kernels for the objective, CHUNKS = chunks, VEC = vec.
// group != 0: generation and fused turn are the packed kernels (`group` lanes per agent)
int rtc_build_de(const nlsg_custom_objective *obj, int chunks, bool vec, int group,
                 DeRtcKernels *out);
struct PsoRtcKernels : RtcModule {
  hipFunction_t init = nullptr, move = nullptr;
};
// pso_init / pso_move kernels; type = nlsg_pso_type.
// group != 0: the move is the packed kernel (`group` lanes per particle)
int rtc_build_pso(const nlsg_custom_objective *obj, int chunks, bool vec, int type, int group,
                  PsoRtcKernels *out);
struct BfgsRtcKernels : RtcModule {  // finite-difference model around the user's objective, or the one on its gradient body
  hipFunction_t init = nullptr, search = nullptr;
  hipFunction_t resident = nullptr;  // bfgs_resident_kernel, for an engine made with NLSG_BFGS_RESIDENT only
};
// wave_rows_offset: where the per-wave parameter rows (obj->n_params > 0) start in the kernels' dynamic
// LDS block, in doubles — the caller's own launch layout (behind bfgs_fd_seq_lds_bytes(chunks) in
// reference order, else 0); it becomes NLSG_PARAMS_PER_WAVE
// grad_body != nullptr (nlsg_bfgs_create_gradient): the kernels are instantiated on kBfgsCustomGrad, whose
// gradient is that body (Objective<NLSG_OBJ_CUSTOM>::grad) instead of finite differences
int rtc_build_bfgs(const nlsg_custom_objective *obj, int chunks, bool vec, long wave_rows_offset,
                   BfgsRtcKernels *out, const char *grad_body = nullptr, bool resident = false);
struct NmRtcKernels : RtcModule {
  hipFunction_t solve = nullptr;
};
int rtc_build_nm(const nlsg_custom_objective *obj, int chunks, bool reference_order, NmRtcKernels *out);
struct DeRefRtcKernels : RtcModule {  // reference-order DE (nlsg_de_ref_kernels.h)
  hipFunction_t solve = nullptr;
};
int rtc_build_de_ref(const nlsg_custom_objective *obj, DeRefRtcKernels *out);
// the resident batch engines (nlsg_de_batch_kernels.h, nlsg_pso_batch_kernels.h): the init kernel and the
// one that runs the turns
struct ResidentRtcKernels : RtcModule {
  hipFunction_t init = nullptr, turns = nullptr;
};
// group: lanes per agent (4 / 8 / 16 / 32), or 64 for one wave per agent
int rtc_build_de_batch(const nlsg_custom_objective *obj, int group, ResidentRtcKernels *out);
// group: lanes per particle (4 / 8 / 16 / 32), or 64 for one wave per particle; type = nlsg_pso_type
int rtc_build_pso_batch(const nlsg_custom_objective *obj, int group, int type, ResidentRtcKernels *out);
struct LmRtcKernels : RtcModule {  // finite-difference model (default functors) around the user's objective
  hipFunction_t iter = nullptr;
  hipFunction_t resident = nullptr;  // Gauss-Newton models of n <= 64: lm_resident_kernel / lm_curve_resident_kernel
};
// wide_chunks != 0: the evaluation kernel of the n > 64 path (a probe point of wide_chunks x 128
// coordinates per wave) instead of the one-wave iteration kernel
int rtc_build_lm(const nlsg_custom_objective *obj, int wide_chunks, bool reference_order, LmRtcKernels *out);
// the Gauss-Newton evaluation kernel of n parameters (lm_iter_kernel to 64, the one-pass kernels to 128
// and 256, the super-block kernel beyond) on the link `value_body` / `slope_body` describe; k->iter
// (n <= 64: k->resident beside it)
int rtc_build_lm_link(const nlsg_lm_link *link, uint64_t n, LmRtcKernels *out);
// lm_resident_kernel<LmTanhLink> for a TanhRegression engine; k->resident only
int rtc_build_lm_tanh_resident(LmRtcKernels *out);
// the curve model's iteration kernel (lm_curve_iter_kernel) of n <= 64 parameters and curve->k data per
// observation, around the residual-and-Jacobian body; k->iter, and lm_curve_resident_kernel as k->resident
int rtc_build_lm_curve(const nlsg_lm_curve *curve, uint64_t n, LmRtcKernels *out);
struct HybRtcKernels : RtcModule {
  hipFunction_t solve = nullptr;
};
// wide_chunks != 0: the n > 128 kernel with that many 128-coordinate chunks per lane
int rtc_build_nmpso(const nlsg_custom_objective *obj, int wide_chunks, HybRtcKernels *out);
struct SannRtcKernels : RtcModule {
  hipFunction_t anneal = nullptr;
};
// group != 0: the packed kernel (several chains per wave) with `group` lanes per chain
int rtc_build_sann(const nlsg_custom_objective *obj, int chunks, bool vec, int group,
                   SannRtcKernels *out);

}  // namespace nlsg
