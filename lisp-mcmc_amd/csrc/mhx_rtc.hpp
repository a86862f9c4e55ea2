// mhx_rtc.hpp -- user-expression models and prior bodies: the reference's
// :function is an arbitrary closure (M:1134-1137) and its priors arbitrary prior-bounds-let
// bodies (M:346-369, nv-specific.lisp:25-34).  A host shim hands their bodies over as
// C-syntax expressions; they are spliced into a model / prior struct next to the SAME kernel
// bodies (mhx_kernels.hpp, embedded in the library) and compiled for gfx950 with hiprtc.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "mhx_finalize.hpp"
#include "mhx_launch.hpp"
#include "mhx_types.hpp"

namespace mhx {

// (UserExpr, RecognisedModel and SPEC_USER: mhx_finalize.hpp, the HIP-free side)

struct UserProgram {
  hipModule_t module = nullptr;
  hipFunction_t f_logpost = nullptr, f_init = nullptr, f_step = nullptr, f_adaptive = nullptr;
  hipFunction_t f_model[MR__COUNT] = {};  // the model read-outs' twins (MHX_MODEL_READOUTS, mhx_launch.hpp)
  hipFunction_t f_split_sweep = nullptr, f_split_step = nullptr;  // only with has_split
  hipFunction_t f_split_tsweep = nullptr;                         // (the tile-sliced sweep)
  hipFunction_t f_persist = nullptr, f_persist_ts = nullptr;      // (the persistent split kernels)
  bool has_split = false;
  const Family* fam = nullptr;  // the kernel family (workgroup shape) the module was built for
  std::string source, log;
  ~UserProgram();
};

// Checks `expr` against the expression grammar of include/mhx.h and rewrites it for splicing:
// parameter identifiers -> p_<name>, integer literals -> doubles, abs/min/max -> device forms.
// extra: additional identifiers allowed as they are, separated by blanks ("x", "bounds_total",
// "y model error").
int rtc_prepare_expr(const std::string& expr, const std::vector<std::string>& names,
                     const char* extra, std::string* out, std::string* err);

// What an expression IS (mhx_expr.cpp; RecognisedModel: mhx_finalize.hpp).  `expr` is the text as
// the caller gave it, `names` its parameter names.
bool rtc_recognise(const std::string& expr, const std::vector<std::string>& names,
                   RecognisedModel* out);

// models[slot] / priors[slot] -> compiled module.  builtin_fallback: the problem also has
// functions with ahead-of-time models, so the generic dispatcher must be part of the kernels.
// Returns 0 or fills *err.
int rtc_build(const std::vector<UserExpr>& models, const std::vector<UserExpr>& priors,
              bool builtin_fallback, bool with_split, const Family& fam, UserProgram* prog,
              std::string* err);
// The same through a process-wide cache (keyed by device and generated source): engines that
// describe the same problem share one compiled module.  Returns nullptr and fills *err on error.
std::shared_ptr<UserProgram> rtc_get(const std::vector<UserExpr>& models,
                                     const std::vector<UserExpr>& priors, bool builtin_fallback,
                                     bool with_split, const Family& fam, std::string* err);

hipError_t rtc_launch_logpost(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                              const double* theta, int64_t n, double* out, double* parts);
// the twin of launch_model (mhx_launch.hpp): the program's model read-out kernel of A's type
template <class Args>
hipError_t rtc_launch_model(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                            const ChainState& S, const Args& A);
hipError_t rtc_launch_init(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                           const ChainState& S);
hipError_t rtc_launch_step_injected(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                                    const ChainState& S, const double* L, int per_chain_l,
                                    const double* z, const double* u, const double* T,
                                    unsigned char* accepted);
hipError_t rtc_launch_split_sweep(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                                  const ChainState& S, int slices);
hipError_t rtc_launch_split_tsweep(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                                   const FnDesc* slices, const ChainState& S, int n_slices);
hipError_t rtc_launch_split_step(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                                 const ChainState& S, const RunDesc& R, int mode, int plain);
hipError_t rtc_launch_adaptive(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                               const ChainState& S, const RunDesc& R, int64_t max_iters,
                               int plain);
hipError_t rtc_launch_persist(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                              const ChainState& S, const RunDesc& R, int slices, int64_t max_iters,
                              int plain);
int rtc_persist_per_cu(const UserProgram& p, int ts);
hipError_t rtc_launch_persist_ts(const UserProgram& p, hipStream_t st, const ProblemDesc* P,
                                 const FnDesc* slices, const ChainState& S, const RunDesc& R,
                                 int n_slices, int64_t max_iters, int plain);

// mhx_get_derived: the module of one set of prepared expression texts over `names` (p_<name> in
// the texts), kernel mhx_user_derived (mhx_derived.hpp), through the same process-wide and on-disk
// caches as the stepping programs but never part of them.  nullptr and *err on error.
struct DerivedProgram {
  hipModule_t module = nullptr;
  hipFunction_t f_derived = nullptr;
  std::string log;
  ~DerivedProgram();
};
std::shared_ptr<DerivedProgram> rtc_get_derived(const std::vector<std::string>& exprs,
                                                const std::vector<std::string>& names,
                                                std::string* err);
hipError_t rtc_launch_derived(const DerivedProgram& p, hipStream_t st, const ChainState& S,
                              const DerivedArgs& A);

}  // namespace mhx
