// nlsolver_amd/csrc/nlsg_rtc.hip — run-time compilation of user objectives (see nlsg_rtc.h).
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "nlsg_rtc.h"

#include "build/nlsg_embedded_sources.inc"

namespace nlsg {
namespace {

struct RtcApi {
  void *lib = nullptr;
  decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
  decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
  decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
  decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
  decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
  decltype(&hiprtcGetCode) GetCode = nullptr;
  decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
  decltype(&hiprtcAddNameExpression) AddNameExpression = nullptr;
  decltype(&hiprtcGetLoweredName) GetLoweredName = nullptr;
};

RtcApi &rtc_api() {
  static RtcApi api;
  return api;
}

// engines may be created from several host threads at once: the table is filled under a lock
// and published whole (api.lib is set last, by the assignment of the finished copy)
std::mutex &rtc_mutex() {
  static std::mutex m;
  return m;
}

int rtc_load(const char *path_in) {
  std::lock_guard<std::mutex> hold(rtc_mutex());
  RtcApi &api = rtc_api();
  if (api.lib) return NLSG_OK;
  const char *path = (path_in && path_in[0]) ? path_in : "libhiprtc.so";
  void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!lib) return fail(NLSG_ERR_UNSUPPORTED, "cannot load hiprtc (%s): %s", path, dlerror());
  RtcApi a;
#define NLSG_RTC_SYM(field, name)                                            \
  a.field = reinterpret_cast<decltype(a.field)>(dlsym(lib, #name));          \
  if (!a.field) {                                                            \
    dlclose(lib);                                                            \
    return fail(NLSG_ERR_UNSUPPORTED, "%s does not export " #name, path);    \
  }
  NLSG_RTC_SYM(CreateProgram, hiprtcCreateProgram)
  NLSG_RTC_SYM(CompileProgram, hiprtcCompileProgram)
  NLSG_RTC_SYM(GetProgramLogSize, hiprtcGetProgramLogSize)
  NLSG_RTC_SYM(GetProgramLog, hiprtcGetProgramLog)
  NLSG_RTC_SYM(GetCodeSize, hiprtcGetCodeSize)
  NLSG_RTC_SYM(GetCode, hiprtcGetCode)
  NLSG_RTC_SYM(DestroyProgram, hiprtcDestroyProgram)
  NLSG_RTC_SYM(AddNameExpression, hiprtcAddNameExpression)
  NLSG_RTC_SYM(GetLoweredName, hiprtcGetLoweredName)
#undef NLSG_RTC_SYM
  a.lib = lib;
  api = a;
  return NLSG_OK;
}

}  // namespace

// What rtc_build compiles: the text, and what the user's part of it is called in the error of a failed
// compilation. rc != 0: the text could not be made of what the user gave, and the error is recorded.
struct RtcSource {
  int rc;
  std::string text;
  const char *what;
};

// `kernel_header` around the user's Objective<NLSG_OBJ_CUSTOM>.
// wave_rows_offset >= 0 (rtc_build_bfgs, with n_params > 0 only): the kernels own a wave per solve, so the
// rows live per wave in the dynamic LDS block, that many doubles from its start (NLSG_PARAMS_PER_WAVE).
// grad_body (rtc_build_bfgs for nlsg_bfgs_create_gradient only): one more member, Objective::grad, made of it;
// without one the source is byte for byte what it is without this argument.
// params_group > 0 (rtc_build_sann's packed kernel, with n_params > 0 only): a row per group of that many lanes
// (NLSG_PARAMS_PER_GROUP) instead of one per wave.
static RtcSource rtc_custom_source(const nlsg_custom_objective *obj, const char *kernel_header,
                                   long wave_rows_offset = -1, const char *grad_body = nullptr,
                                   int params_group = 0) {
  if (!obj || !obj->term_body || !obj->term_body[0])
    return {fail(NLSG_ERR_INVALID_ARG, "a custom objective needs a term body"), "", "custom objective"};
  // n_params > 0 (resident batch engines and nlsg_nm / nmpso / lm / bfgs_create_params; every
  // *_create_custom besides has rejected it): the macro
  // puts the solve's row into static LDS (nlsg_common.h) and the bodies read it as p(k); for BFGS a
  // second macro puts a row per wave into the dynamic block and p(k) indexes the wave's own. With
  // n_params == 0 the source is byte for byte what it was before parameters existed, for every engine.
  const int n_params = obj->n_params > 0 ? obj->n_params : 0;
  const bool per_wave = n_params && wave_rows_offset >= 0;
  std::string src;
  if (n_params) src += "#define NLSG_N_PARAMS " + std::to_string(n_params) + "\n";
  if (per_wave) src += "#define NLSG_PARAMS_PER_WAVE " + std::to_string(wave_rows_offset) + "\n";
  const bool per_group = per_wave && params_group > 0;
  if (per_group) src += "#define NLSG_PARAMS_PER_GROUP " + std::to_string(params_group) + "\n";
  src += std::string("#include \"") + kernel_header + "\"\n"
         "namespace nlsg {\n"
         "template <>\n"
         "struct Objective<NLSG_OBJ_CUSTOM> {\n";
  if (per_group)  // the row of lane group threadIdx.x / G
    src += "  __device__ static inline double p(uint64_t k) { return custom_params_group_row()[k]; }\n";
  else if (per_wave)  // the row of wave threadIdx.x >> 6
    src += "  __device__ static inline double p(uint64_t k) { return custom_params_wave_row()[k]; }\n";
  else if (n_params)
    src += "  __device__ static inline double p(uint64_t k) { return custom_params_lds[k]; }\n";
  if (obj->chain == NLSG_CUSTOM_VECTOR) {
    // whole-vector form: term_body is the body of  double f(const X &x, uint64_t D)
    src += "  static constexpr bool kChain = false;\n"
           "  static constexpr bool kWhole = true;\n"
           "  __device__ static inline double term(double, double) { return 0.0; }\n"
           "  __device__ static inline uint64_t n_terms(uint64_t) { return 0; }\n"
           "  __device__ static inline double finish(double s, uint64_t) { return s; }\n"
           "  template <typename X>\n"
           "  __device__ static inline double whole(const X &x, uint64_t D) {\n    (void)D;\n#line 1 "
           "\"vector_body\"\n";
    src += obj->term_body;
    src += "\n  }\n";
    if (grad_body) {  // the body of  double grad(const X &x, uint64_t i, uint64_t D)  = df/dx_i, i wave-uniform
      src += "  template <typename X>\n"
             "  __device__ static inline double grad(const X &x, uint64_t i, uint64_t D) {\n"
             "    (void)x;\n    (void)i;\n    (void)D;\n#line 1 \"grad_body\"\n";
      src += grad_body;
      src += "\n  }\n";
    }
    src += "};\n}  // namespace nlsg\n";
  } else {
    src += "  static constexpr bool kWhole = false;\n"
           "  static constexpr bool kChain = ";
    src += obj->chain ? "true" : "false";
    src += ";\n  __device__ static inline double term(double xi, double xn) {\n    (void)xn;\n#line 1 "
           "\"term_body\"\n";
    src += obj->term_body;
    src += "\n  }\n"
           "  __device__ static inline uint64_t n_terms(uint64_t D) { return kChain ? (D ? D - 1 : 0) : D; }\n"
           "  __device__ static inline double finish(double s, uint64_t D) {\n    (void)D;\n#line 1 "
           "\"finish_body\"\n";
    src += (obj->finish_body && obj->finish_body[0]) ? obj->finish_body : "return s;";
    src += "\n  }\n"
           "  template <typename X>\n"
           "  __device__ static inline double whole(const X &, uint64_t) { return 0.0; }\n";
    if (grad_body) {  // df/dx_i from x_{i-1}, x_i, x_{i+1} and the sum of terms s, per lane
      src += "  __device__ static inline double grad(double xm, double xi, double xn, uint64_t i, uint64_t D, "
             "double s) {\n"
             "    (void)xm;\n    (void)xi;\n    (void)xn;\n    (void)i;\n    (void)D;\n    (void)s;\n#line 1 "
             "\"grad_body\"\n";
      src += grad_body;
      src += "\n  }\n";
    }
    src += "};\n}  // namespace nlsg\n";
  }
  return {NLSG_OK, src, "custom objective"};
}

// A compiled code object and the lowered names of its kernels, kept by source text: a second engine
// of the same link and kernel (another max_iter, another solver, the drop-in class's engine per call)
// loads it instead of compiling for seconds. The oldest entries go once there are kRtcKeptMax.
struct RtcKept {
  std::vector<char> code;
  std::vector<std::string> lowered;
  uint64_t age = 0;
};
constexpr size_t kRtcKeptMax = 32;
static std::map<std::string, RtcKept> &rtc_kept() {
  static std::map<std::string, RtcKept> m;
  return m;
}
static std::mutex &rtc_kept_mutex() {
  static std::mutex m;
  return m;
}

static int rtc_load_code(const std::vector<char> &code, const std::vector<std::string> &lowered,
                         const char *what, hipModule_t *mod_out, std::vector<hipFunction_t> *fns_out) {
  hipModule_t mod = nullptr;
  hipError_t he = hipModuleLoadData(&mod, code.data());
  std::vector<hipFunction_t> fns(lowered.size(), nullptr);
  for (size_t i = 0; i < lowered.size() && he == hipSuccess; i++)
    he = hipModuleGetFunction(&fns[i], mod, lowered[i].c_str());
  if (he != hipSuccess) {
    if (mod) hipModuleUnload(mod);
    return fail(NLSG_ERR_HIP, "loading the compiled %s failed: %s", what, hipGetErrorString(he));
  }
  *mod_out = mod;
  *fns_out = fns;
  return NLSG_OK;
}

// `src` (which includes the embedded headers by name) to a loaded module, one function per name
// expression; `what` names the user's part of it in the error of a failed compilation.
// keep_code: look the source up among the kept code objects first, and keep this one
static int rtc_compile_source(const std::string &src, const char *what,
                              const std::vector<std::string> &name_exprs, hipModule_t *mod_out,
                              std::vector<hipFunction_t> *fns_out, bool keep_code) {
  const int rc = rtc_load(nullptr);
  if (rc) return rc;
  RtcApi &api = rtc_api();
  std::string key;
  if (keep_code) {
    key = src;
    for (const std::string &n : name_exprs) key += '\n' + n;
    RtcKept hit;
    bool found = false;
    {
      std::lock_guard<std::mutex> hold(rtc_kept_mutex());
      const auto it = rtc_kept().find(key);
      if (it != rtc_kept().end()) {
        hit = it->second;
        found = true;
      }
    }
    if (found) return rtc_load_code(hit.code, hit.lowered, what, mod_out, fns_out);
  }
  const int nh = static_cast<int>(sizeof(kEmbedded) / sizeof(kEmbedded[0]));
  std::vector<const char *> names(nh), texts(nh);
  for (int i = 0; i < nh; i++) {
    names[i] = kEmbedded[i].name;
    texts[i] = kEmbedded[i].text;
  }
  hiprtcProgram prog = nullptr;
  if (api.CreateProgram(&prog, src.c_str(), "nlsg_custom_objective.hip", nh, texts.data(),
                        names.data()) != HIPRTC_SUCCESS)
    return fail(NLSG_ERR_HIP, "hiprtcCreateProgram failed");
  for (const std::string &n : name_exprs)
    if (api.AddNameExpression(prog, n.c_str()) != HIPRTC_SUCCESS) {
      api.DestroyProgram(&prog);
      return fail(NLSG_ERR_HIP, "hiprtcAddNameExpression(%s) failed", n.c_str());
    }
  // the flags of csrc/Makefile: device arithmetic must stay bit-reproducible
  // ... and no spilling of vector registers to accumulation registers: for a kernel bounded to 1024
  // threads (128 registers per lane) the compiler has placed 9 spill AGPRs behind 124 VGPRs (a user term
  // body in nm_solve_driver_kernel), 133 in all -- the dispatch of a 1024-thread workgroup is then refused
  // ("out of VGPRs"). Spills go to scratch instead, and the count stays within the bound.
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-fno-fast-math", "-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"};
  const hiprtcResult cr = api.CompileProgram(prog, 7, opts);
  if (cr != HIPRTC_SUCCESS) {
    size_t ls = 0;
    api.GetProgramLogSize(prog, &ls);
    std::string log(ls ? ls : 1, '\0');
    if (ls) api.GetProgramLog(prog, &log[0]);
    api.DestroyProgram(&prog);
    if (log.size() > 400) log.resize(400);
    return fail(NLSG_ERR_INVALID_ARG, "%s does not compile: %s", what, log.c_str());
  }
  size_t cs = 0;
  if (api.GetCodeSize(prog, &cs) != HIPRTC_SUCCESS || cs == 0) {
    api.DestroyProgram(&prog);
    return fail(NLSG_ERR_HIP, "hiprtcGetCodeSize failed");
  }
  std::vector<char> code(cs);
  if (api.GetCode(prog, code.data()) != HIPRTC_SUCCESS) {
    api.DestroyProgram(&prog);
    return fail(NLSG_ERR_HIP, "hiprtcGetCode failed");
  }
  std::vector<std::string> lowered_names;
  for (const std::string &n : name_exprs) {
    const char *lowered = nullptr;  // lives in the program: copied before it is destroyed
    if (api.GetLoweredName(prog, n.c_str(), &lowered) != HIPRTC_SUCCESS || !lowered) {
      api.DestroyProgram(&prog);
      return fail(NLSG_ERR_HIP, "loading the compiled %s failed: %s", what, hipGetErrorString(hipErrorNotFound));
    }
    lowered_names.push_back(lowered);
  }
  api.DestroyProgram(&prog);
  const int lrc = rtc_load_code(code, lowered_names, what, mod_out, fns_out);
  if (!lrc && keep_code) {
    static uint64_t clock = 0;
    std::lock_guard<std::mutex> hold(rtc_kept_mutex());
    std::map<std::string, RtcKept> &kept = rtc_kept();
    if (kept.size() >= kRtcKeptMax) {
      auto oldest = kept.begin();
      for (auto it = kept.begin(); it != kept.end(); ++it)
        if (it->second.age < oldest->second.age) oldest = it;
      kept.erase(oldest);
    }
    RtcKept &slot = kept[key];
    slot.code = std::move(code);
    slot.lowered = std::move(lowered_names);
    slot.age = ++clock;
  }
  return lrc;
}

// a kernel's template-id (a name expression) and where its function goes
struct RtcBind {
  std::string name;
  hipFunction_t *fn;
};

// What every rtc_build_* ends in: the source to a module, the binds' functions out of it. `binds` point into
// *out, which is written on success only: then it holds the module, the bound kernels and nothing else.
template <typename K>
static int rtc_build(const RtcSource &source, bool keep_code, K *out, const std::vector<RtcBind> &binds) {
  if (source.rc) return source.rc;
  std::vector<std::string> names;
  for (const RtcBind &b : binds) names.push_back(b.name);
  hipModule_t mod = nullptr;
  std::vector<hipFunction_t> fns;
  if (const int rc = rtc_compile_source(source.text, source.what, names, &mod, &fns, keep_code)) return rc;
  *out = K();
  out->mod = mod;
  for (size_t i = 0; i < binds.size(); i++) *binds[i].fn = fns[i];
  return NLSG_OK;
}

// the objective id every kernel of a user objective is instantiated on
static std::string custom_id() { return std::to_string(static_cast<int>(NLSG_OBJ_CUSTOM)); }
static std::string targs(int chunks, bool vec) {
  return custom_id() + ", " + std::to_string(chunks) + ", " + (vec ? "true" : "false");
}

int rtc_build_de(const nlsg_custom_objective *obj, int chunks, bool vec, int group,
                 DeRtcKernels *out) {
  const RtcSource source = rtc_custom_source(obj, "nlsg_de_kernels.h");
  if (chunks == 0) {  // D > 1024: the segment-streaming kernels (no fused turn)
    const std::string t = custom_id() + ", " + (vec ? "true" : "false");
    return rtc_build(source, false, out,
                     {{"nlsg::de_init_long_kernel<" + t + ">", &out->init},
                      {"nlsg::de_generation_long_kernel<" + t + ">", &out->generation}});
  }
  const std::string t = targs(chunks, vec), g = custom_id() + ", " + std::to_string(group);
  return rtc_build(source, false, out,
                   {{"nlsg::de_init_kernel<" + t + ">", &out->init},
                    {group ? "nlsg::de_generation_groups_kernel<" + g + ">" : "nlsg::de_generation_kernel<" + t + ">",
                     &out->generation},
                    {group ? "nlsg::de_turn_groups_kernel<" + g + ">" : "nlsg::de_turn_kernel<" + t + ">",
                     &out->turn}});
}

// the resident batch engine's two kernels, next to the turn kernels they restate
int rtc_build_de_batch(const nlsg_custom_objective *obj, int group, ResidentRtcKernels *out) {
  return rtc_build(rtc_custom_source(obj, "nlsg_de_batch_kernels.h"), false, out,
                   {{"nlsg::de_batch_init_kernel<" + custom_id() + ">", &out->init},
                    {"nlsg::de_batch_kernel<" + custom_id() + ", " + std::to_string(group) + ">", &out->turns}});
}

// the resident batch PSO engine's two kernels, next to the turn kernels they restate
int rtc_build_pso_batch(const nlsg_custom_objective *obj, int group, int type, ResidentRtcKernels *out) {
  return rtc_build(rtc_custom_source(obj, "nlsg_pso_batch_kernels.h"), false, out,
                   {{"nlsg::pso_batch_init_kernel<" + custom_id() + ">", &out->init},
                    {"nlsg::pso_batch_kernel<" + custom_id() + ", " + std::to_string(group) + ", " +
                         std::to_string(type) + ">",
                     &out->turns}});
}

int rtc_build_pso(const nlsg_custom_objective *obj, int chunks, bool vec, int type, int group,
                  PsoRtcKernels *out) {
  const RtcSource source = rtc_custom_source(obj, "nlsg_pso_kernels.h");
  const std::string ty = ", " + std::to_string(type) + ">";
  if (chunks == 0) {  // D > 1024: the segment-streaming kernels
    const std::string t = custom_id() + ", " + (vec ? "true" : "false");
    return rtc_build(source, false, out,
                     {{"nlsg::pso_init_long_kernel<" + t + ">", &out->init},
                      {"nlsg::pso_move_long_kernel<" + t + ty, &out->move}});
  }
  const std::string t = targs(chunks, vec);
  return rtc_build(source, false, out,
                   {{"nlsg::pso_init_kernel<" + t + ">", &out->init},
                    {group ? "nlsg::pso_move_groups_kernel<" + custom_id() + ", " + std::to_string(group) + ty
                           : "nlsg::pso_move_kernel<" + t + ty,
                     &out->move}});
}

int rtc_build_bfgs(const nlsg_custom_objective *obj, int chunks, bool vec, long wave_rows_offset,
                   BfgsRtcKernels *out, const char *grad_body, bool resident) {
  // <CHUNKS, VEC, MODEL>: MODEL = the objective id selects the finite-difference BfgsModel, kBfgsCustomGrad
  // (-2, nlsg_bfgs_kernels.h) the one that evaluates the objective's own gradient body
  const std::string t = std::to_string(chunks) + ", " + (vec ? "true" : "false") + ", " +
                        (grad_body ? std::string("nlsg::kBfgsCustomGrad") : custom_id());
  // (the resident kernel is instantiated for an engine that asks for it only: a lock-step engine compiles
  // what it always did)
  std::vector<RtcBind> binds = {{"nlsg::bfgs_init_kernel<" + t + ">", &out->init},
                                {"nlsg::bfgs_search_kernel<" + t + ">", &out->search}};
  if (resident) binds.push_back({"nlsg::bfgs_resident_kernel<" + t + ">", &out->resident});
  // (a row per wave in the dynamic block.) The code object is kept by its source, as the annealer's: engines
  // that differ in alpha, max_iter or grad_eps only — a sweep of step lengths, the drop-in's engine per call —
  // load it instead of compiling.
  return rtc_build(rtc_custom_source(obj, "nlsg_bfgs_kernels.h", wave_rows_offset, grad_body), true, out, binds);
}

int rtc_build_nm(const nlsg_custom_objective *obj, int chunks, bool reference_order, NmRtcKernels *out) {
  // chunks == 0: the driver-wave kernel (n <= 128)
  return rtc_build(rtc_custom_source(obj, "nlsg_nm_kernels.h"), false, out,
                   {{chunks == 0 ? "nlsg::nm_solve_driver_kernel<" + custom_id() + (reference_order ? ", true>" : ">")
                                 : "nlsg::nm_solve_kernel<" + custom_id() + ", " + std::to_string(chunks) + ">",
                     &out->solve}});
}

int rtc_build_de_ref(const nlsg_custom_objective *obj, DeRefRtcKernels *out) {
  return rtc_build(rtc_custom_source(obj, "nlsg_de_ref_kernels.h"), false, out,
                   {{"nlsg::de_ref_kernel<" + custom_id() + ">", &out->solve}});
}

int rtc_build_nmpso(const nlsg_custom_objective *obj, int wide_chunks, HybRtcKernels *out) {
  return rtc_build(rtc_custom_source(obj, "nlsg_nmpso_kernels.h"), false, out,
                   {{wide_chunks ? "nlsg::nmpso_solve_wide_kernel<" + custom_id() + ", " +
                                       std::to_string(wide_chunks) + ">"
                                 : "nlsg::nmpso_solve_kernel<" + custom_id() + ">",
                     &out->solve}});
}

int rtc_build_sann(const nlsg_custom_objective *obj, int chunks, bool vec, int group,
                   SannRtcKernels *out) {
  const std::string name =
      chunks == 0 ? "nlsg::sann_anneal_long_kernel<" + custom_id() + ", " + (vec ? "true" : "false") + ">"
      : group     ? "nlsg::sann_anneal_groups_kernel<" + custom_id() + ", " + std::to_string(group) + ">"
                  : "nlsg::sann_anneal_kernel<" + targs(chunks, vec) + ">";
  // n_params > 0 (nlsg_sann_create_params): the rows start the dynamic block (offset 0), one per wave, or with
  // `group` one per lane group. The code object is kept by its source: the engines of a sweep, of the drop-in's
  // calls and of a sharded batch differ in their configuration only and load it instead of compiling.
  return rtc_build(rtc_custom_source(obj, "nlsg_sann_kernels.h", obj && obj->n_params > 0 ? 0 : -1, nullptr, group),
                   true, out, {{name, &out->anneal}});
}

// NLSG_LM_RESIDENT_NT=1 (A/B switch, read when a module is built): the resident kernels re-read their data
// with nontemporal loads, as the lock-step kernels stream theirs, instead of plain ones. Same bits.
static const char *lm_resident_nt() {
  const char *e = std::getenv("NLSG_LM_RESIDENT_NT");
  return e && e[0] == '1' ? "true" : "false";
}

int rtc_build_lm(const nlsg_custom_objective *obj, int wide_chunks, bool reference_order, LmRtcKernels *out) {
  const std::string id = custom_id();
  const std::string name =
      wide_chunks ? (reference_order ? "nlsg::lm_wide_fd_lanes_kernel<" + id + ">"
                                     : "nlsg::lm_wide_fd_eval_kernel<" + id + ", " + std::to_string(wide_chunks) + ">")
                  : "nlsg::lm_fd_iter_kernel<" + id + (reference_order ? ", true>" : ">");
  return rtc_build(rtc_custom_source(obj, "nlsg_lm_kernels.h"), false, out, {{name, &out->iter}});
}
// The Gauss-Newton evaluation kernel of the shape, instantiated on a link made of the two bodies
// (nlsg_lm_kernels.h LmTanhLink is the pattern). The same selection by n as the built-in engine's, the
// same flags as the offline build (rtc_compile_source): a body that restates tanh gives the built-in
// kernel's bits.
int rtc_build_lm_link(const nlsg_lm_link *link, uint64_t n, LmRtcKernels *out) {
  if (!link || !link->value_body || !link->value_body[0] || !link->slope_body || !link->slope_body[0])
    return fail(NLSG_ERR_INVALID_ARG, "a link needs a value body and a slope body");
  std::string src =
      "#include \"nlsg_lm_kernels.h\"\n"
      "namespace nlsg {\n"
      "struct LmUserLink {\n"
      "  static constexpr bool kZeroAtZero = false;\n"  // (not known of a body: the rows >= m are masked)
      "  __device__ static inline double value(double z) {\n#line 1 \"value_body\"\n";
  src += link->value_body;
  src += "\n  }\n"
         "  __device__ static inline double slope(double z, double v) {\n    (void)z;\n    (void)v;\n#line 1 "
         "\"slope_body\"\n";
  src += link->slope_body;
  src += "\n  }\n};\n}  // namespace nlsg\n";
  const char *kernel = n <= 64 ? "lm_iter_kernel" : n <= 128 ? "lm_wide128x8_tanh_eval_kernel"
                     : n <= 256 ? "lm_wide256x8_tanh_eval_kernel" : "lm_wide_mfma_tanh_eval_kernel";
  std::vector<RtcBind> binds = {{std::string("nlsg::") + kernel + "<nlsg::LmUserLink>", &out->iter}};
  // (one wave per problem: the resident driver's kernel rides in the same module)
  if (n <= 64)
    binds.push_back({std::string("nlsg::lm_resident_kernel<nlsg::LmUserLink, ") + lm_resident_nt() + ">",
                     &out->resident});
  return rtc_build({NLSG_OK, src, "link"}, true, out, binds);
}
// The resident driver's kernel on the built-in link. The library's own set of kernels holds the lock-step
// pair only, so a TanhRegression engine gets this one here, the first time the resident driver is chosen on
// it; the code object is kept by its source, and every further engine loads it.
int rtc_build_lm_tanh_resident(LmRtcKernels *out) {
  return rtc_build({NLSG_OK, "#include \"nlsg_lm_kernels.h\"\n", "resident kernel"}, true, out,
                   {{std::string("nlsg::lm_resident_kernel<nlsg::LmTanhLink, ") + lm_resident_nt() + ">",
                     &out->resident}});
}
// lm_curve_iter_kernel on a model made of the body (nlsg_lm_kernels.h): K data per observation, the
// padded column count chosen from n. The body sees th(j), t(k), y, n, r and J(j).
int rtc_build_lm_curve(const nlsg_lm_curve *curve, uint64_t n, LmRtcKernels *out) {
  if (!curve || !curve->body || !curve->body[0])
    return fail(NLSG_ERR_INVALID_ARG, "a curve model needs a body (nlsg_lm_curve)");
  std::string src =
      "#include \"nlsg_lm_kernels.h\"\n"
      "namespace nlsg {\n"
      "struct LmUserCurve {\n"
      "  static constexpr int kK = " + std::to_string(curve->k) + ";\n"
      "  template <typename Th, typename T, typename Jt>\n"
      "  __device__ static inline void eval(const Th &th, const T &t, const double y, const int n, double &r,\n"
      "                                     const Jt &J) {\n"
      "    (void)th;\n    (void)t;\n    (void)y;\n    (void)n;\n    (void)J;\n#line 1 \"curve_body\"\n";
  src += curve->body;
  src += "\n  }\n};\n}  // namespace nlsg\n";
  const int npad = n <= 16 ? 16 : n <= 32 ? 32 : 64;
  return rtc_build({NLSG_OK, src, "curve model"}, true, out,
                   {{"nlsg::lm_curve_iter_kernel<nlsg::LmUserCurve, " + std::to_string(npad) + ">", &out->iter},
                    {"nlsg::lm_curve_resident_kernel<nlsg::LmUserCurve, " + std::to_string(npad) + ", " +
                         lm_resident_nt() + ">",
                     &out->resident}});
}

}  // namespace nlsg

extern "C" int nlsg_rtc_load(const char *hiprtc_path) { return nlsg::rtc_load(hiprtc_path); }

extern "C" uint64_t nlsg_custom_params_lds_bytes(int32_t n_params) {
  return nlsg::custom_params_lds_bytes(n_params);
}
