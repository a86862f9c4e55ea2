// mhx_engine.cpp -- host side of libmhx: the C ABI of include/mhx.h over the gfx950 kernels.
//
// No CPU fallback exists: every numeric entry point launches HIP kernels on the configured
// device and fails with MHX_EDEVICE when that is impossible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mhx.h"
#include <dlfcn.h>

#include <memory>

#include "mhx_ensemble.hpp"
#include "mhx_finalize.hpp"
#include "mhx_heldout.hpp"
#include "mhx_launch.hpp"
#include "mhx_plan.hpp"
#include "mhx_rtc.hpp"
#include "mhx_stage.hpp"
#include "mhx_types.hpp"

using namespace mhx;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return fail(MHX_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                  __FILE__, __LINE__);                                                  \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  hipError_t alloc(size_t count, bool zero = true) {
    release();
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = count;
    if (zero) e = hipMemset(p, 0, count * sizeof(T));
    return e;
  }
};

struct Dataset {
  DevBuf<double> x, y, w, c, txlo, txhi, tgh;
  std::vector<double> hx;  // host copy of the padded x: tile ranges are formed per kernel family
  size_t n = 0;            // data points (hx holds the pads too)
  // mhx_get_waic's per-point constants where the device's c array does not hold them (Poisson:
  // -log-factorial(y_i); a normal likelihood with a second column of x, which takes c's place)
  std::vector<double> hconst;
  bool no_rec = false;     // MHX_NO_RECURRENCE=1 when the dataset was set
  bool set = false;
  // a dataset per walker (mhx_set_dataset_planes): x (and a shared 1/sigma) above, the walkers'
  // own arrays here; pdesc = the device copy of pd, which finalize_problem completes
  bool planes = false;
  int sigma_kind = MHX_SIGMA_NONE;
  DevBuf<double> py, pw, pconst;
  PlaneDesc pd{};
  DevBuf<PlaneDesc> pdesc;
};

int64_t steps_to_settle_of(int d) { return 10 * (int64_t)std::max(50, d); }  // M:873

// ---- RCCL, loaded lazily (libmhx.so has no link-time dependency on it: a single-GPU host needs
// no collective library).  Only what the pooled-covariance tick uses; the types are restated
// from rccl.h (NCCL ABI: opaque communicator, 128-byte id, ncclDouble = 8, ncclSum = 0).
typedef struct mhxNcclComm* nccl_comm_t;
struct nccl_unique_id { char internal[128]; };
struct Rccl {
  void* h = nullptr;
  int (*GetUniqueId)(nccl_unique_id*) = nullptr;
  int (*CommInitRank)(nccl_comm_t*, int, nccl_unique_id, int) = nullptr;
  int (*CommInitAll)(nccl_comm_t*, int, const int*) = nullptr;
  int (*CommDestroy)(nccl_comm_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
// The library is opened RTLD_LOCAL, and that is load-bearing.  What is known (DESIGN.md
// section 6): four full-suite test processes of round 2 that had used RCCL and hiprtc ended in
// `double free or corruption (!prev)` / `free(): invalid pointer` AFTER their work was done,
// while this dlopen said RTLD_GLOBAL (later RTLD_GLOBAL | RTLD_NODELETE) - with the ROCm
// installation's librccl as well as with the one PyTorch bundles; none of the dozens of runs
// since it says RTLD_LOCAL has.  Both builds of librccl export, next to the nccl* entry points,
// several hundred C++ symbols of default visibility - weak std:: template instantiations and
// fmt::v7's STB_GNU_UNIQUE data objects (`nm -D`) - which RTLD_GLOBAL adds to the scope every
// LATER-loaded library's own weak symbols are resolved in; two libraries tearing down what each
// takes for its own object at exit is the mechanism - reproduced in round 4
// (tools/debug/rccl_exit_abort.py): old flags, RCCL through libmhx, a hiprtc model, THEN a torch
// operation, everything left to the interpreter's exit -> `double free or corruption (!prev)`,
// twice in two runs; RTLD_LOCAL, same process: exit status 0; LD_DEBUG=bindings shows 67 weak
// C++ symbols of libraries that do not depend on RCCL bound into it under the old flags, none
// under the new.  So the flag is kept local, nothing of RCCL's is
// ever visible to anybody but this file's dlsym calls, and one test keeps a process with RCCL,
// hiprtc and torch at exit status 0 (tests/test_gpu_rccl_stub.py).
// MHX_RCCL_DLOPEN_GLOBAL=1 restores the old flags - for that debug script only, and only in a
// library built with -DMHX_DEBUG_HOOKS (tests/hooks/libmhx_hooks.so; the release library has
// neither of the two test switches).
std::string g_rccl_why;  // why rccl().ok is false
Rccl& rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r;
  tried = true;
  // MHX_RCCL_LIBRARY: the copy that belongs to the HIP runtime this process uses (the Python
  // binding points it at PyTorch's bundled librccl.so when it shares PyTorch's libamdhip64; the
  // tests point it at their stub); then the soname: a host that already has RCCL loaded shares
  // that instance
  const char* names[] = {getenv("MHX_RCCL_LIBRARY"), "librccl.so.1", "librccl.so",
                         "/opt/rocm/lib/librccl.so"};
#ifdef MHX_DEBUG_HOOKS
  const char* dg = getenv("MHX_RCCL_DLOPEN_GLOBAL");
  const int flags = (dg && atoi(dg) != 0) ? (RTLD_NOW | RTLD_GLOBAL | RTLD_NODELETE)
                                           : (RTLD_NOW | RTLD_LOCAL);
#else
  const int flags = RTLD_NOW | RTLD_LOCAL;
#endif
  const char* opened = nullptr;
  for (const char* n : names) {
    if (!n || !*n) continue;
    r.h = dlopen(n, flags);
    if (r.h) {
      opened = n;
      break;
    }
    g_rccl_why = dlerror();
  }
  if (!r.h) {
    if (g_rccl_why.empty()) g_rccl_why = "librccl.so not found";
    return r;
  }
  // One HIP runtime per process: the collective is enqueued on OUR stream, so the library must be
  // bound to the very libamdhip64 libmhx uses.  (A librccl that needs another soname of the
  // runtime - a different ROCm major - would bring a second runtime into the process: its
  // hipStream_t handles are not ours.)  Compared by the address both sides resolve a HIP entry
  // point to.
  {
    void* theirs = dlsym(r.h, "hipStreamSynchronize");
    void* ours = reinterpret_cast<void*>(&hipStreamSynchronize);
    if (theirs && theirs != ours) {
      Dl_info a{}, b{};
      (void)dladdr(theirs, &a);
      (void)dladdr(ours, &b);
      char buf[768];
      snprintf(buf, sizeof buf, "%s is bound to HIP runtime %s, libmhx to %s: refused (one HIP "
               "runtime per process; set MHX_RCCL_LIBRARY to the librccl of the runtime in use)",
               opened, a.dli_fname ? a.dli_fname : "?", b.dli_fname ? b.dli_fname : "?");
      g_rccl_why = buf;
      dlclose(r.h);
      r.h = nullptr;
      return r;
    }
  }
#define SYM(field, name) *(void**)(&r.field) = dlsym(r.h, name)
  SYM(GetUniqueId, "ncclGetUniqueId");
  SYM(CommInitRank, "ncclCommInitRank");
  SYM(CommInitAll, "ncclCommInitAll");
  SYM(CommDestroy, "ncclCommDestroy");
  SYM(AllReduce, "ncclAllReduce");
  SYM(GroupStart, "ncclGroupStart");
  SYM(GroupEnd, "ncclGroupEnd");
  SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
  r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.AllReduce &&
         r.GroupStart && r.GroupEnd;
  if (!r.ok) g_rccl_why = std::string(opened) + " lacks one of the eight nccl* entry points libmhx binds";
  return r;
}
const char* rccl_err(int rc) {
  return rccl().GetErrorString ? rccl().GetErrorString(rc) : "error";
}
constexpr int kNcclDouble = 8, kNcclSum = 0;

int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace

struct mhx_engine {
  mhx_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stop_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  ProblemDesc P{};  // host copy; device pointers inside
  bool fn_set[MHX_MAX_FUNCTIONS] = {};
  Dataset data[MHX_MAX_FUNCTIONS];
  DevBuf<ProblemDesc> dP;
  bool problem_dirty = true;
  UserExpr fn_expr[MHX_MAX_FUNCTIONS];     // MHX_MODEL_EXPR bodies
  RecognisedModel fn_recog[MHX_MAX_FUNCTIONS];  // ... and what they are (mhx_expr.cpp)
  bool recognise = true;                   // mhx_set_expr_recognition
  UserExpr prior_expr[MHX_MAX_FUNCTIONS];  // prior-bounds-let bodies
  std::string lik_expr[MHX_MAX_FUNCTIONS]; // create-log-liklihood-function bodies (validated)
  std::shared_ptr<UserProgram> user_prog;  // run-time compiled kernels (shared, rtc_get)
  int spec = SPEC_GENERIC;
  std::string kernel_name;  // mhx_kernel_name
  std::string rtc_note;     // why run-time specialisation was not possible (first line)
  const Family* fam = &family_w8();  // kernel family (workgroup shape) of the current problem
  int cus = 256;                     // compute units of the device (mhx_create)
  // the environment switches (mhx_plan.hpp): read when the problem is finalised, and again at the
  // start of every run (the run-time ones: compaction, graphs, re-slicing)
  EngineKnobs knobs;
  ProblemShape shape;                // what the mode rules read of the finalised problem

  ChainState S{};
  DevBuf<double> theta, prob, best_theta, best_prob, hist_prob, hist_theta, L, temperature,
      mat_tmp, pool_stats, pool_vec, L_pool;
  DevBuf<int32_t> pool_valid;
  int64_t global_iter = 0;  // loop iterations launched since mhx_adaptive_begin (pooled cadence)
  uint64_t pool_refreshes = 0;
  DevBuf<int64_t> length, age, n_hist, loop_i, reset_index;
  DevBuf<uint64_t> draw;
  DevBuf<int32_t> shutting, status, fwd_idx, stop_flag;
  DevBuf<unsigned long long> step_counter;
  // split mode (few chains, long datasets): 0 = batch kernels, else workgroups per chain
  int split_slices = 0;
  int64_t split_portion = 512;  // iterations queued between two looks at the chain states
  // one portion of split-mode launches captured as a HIP graph (replayed; the kernel arguments -
  // chain state pointers, run description - are frozen in it, so it is dropped whenever the run or
  // the problem changes): fewer microseconds per launch than issuing 2 N + 1 kernels one by one
  hipGraphExec_t split_graph = nullptr;
  int64_t split_graph_iters = 0;
  int split_graph_plain = -1;
  DevBuf<double> split_prop, split_u, split_part;
  DevBuf<int32_t> split_pending;
  // tile-sliced split mode (k_split_tsweep): split_slices = slices of whole windows per function,
  // ts_table = their FnDescs [K][split_slices] on the device
  // persistent split mode (k_persist): the per-chain split mode's slots, ONE launch for many
  // iterations - when every workgroup of the launch is resident at once (finalize_problem)
  bool persist = false;
  DevBuf<unsigned long long> persist_msg;  // [C][64]: the chains' proposal blocks (mhx_types.hpp)
  DevBuf<unsigned char> persist_part;      // [C][K][slots][16]: {partial sum, generation} pairs
  DevBuf<int32_t> persist_error;           // [1]: a master gave up waiting (ChainState::persist_error)
  bool persist_launched = false;           // the open launch is a persistent one: look at the flag
  bool persist_off = false;                // a persistent launch failed on this engine: never again
  bool tsplit = false;
  int ts_initial = 0;  // slices a run starts with (compact_tsplit may cut finer as chains finish)
  // iterations the split modes have queued since the run began.  The tile-sliced mode repacks
  // only where this count is a multiple of the portion length: when and how the sums are
  // regrouped is then a function of the walk, not of how the host chunks its advance calls
  int64_t split_iter = 0;
  bool ts_repack_due = false;
  DevBuf<FnDesc> ts_table;
  bool chains_ready = false;

  RunDesc R{};
  DevBuf<double> temps;          // a window of the temperature schedule (ensure_temps)
  int64_t temps_count = 0;       // entries held on the device, from R.temps_first
  double run_temperature = 1.0;  // :temperature of the current run
  bool run_ready = false;
  int64_t chunk_iters = 64;

  mhx_allreduce_fn allreduce = nullptr;
  void* allreduce_ctx = nullptr;
  int allreduce_device = 0;
  // native collective of the pooled tick: an RCCL communicator of this engine's own
  // (mhx_comm_init_rank: one process per GPU) or its group's (mhx_group_create)
  nccl_comm_t comm = nullptr;
  bool comm_owned = false;
  // slot -> chain map of the stepping kernel (ChainState::slot_chain): rebuilt from the chain
  // states whenever a quarter of the slots in use have finished (compact_slots)
  DevBuf<int32_t> slot_map;
  int64_t slots_mapped = 0;  // chains dealt at the last compact_slots (0: identity map)
  bool launch_open = false;  // steps enqueued by launch_steps_enqueue(), not yet finished
  int64_t launch_iters = 0;

  // device staging of the host-facing calls (mhx_logpost, mhx_step_injected, read-backs): grown
  // on demand and kept, instead of a hipMalloc / hipFree pair per call
  DevBuf<unsigned char> stage;

  // accounting
  uint64_t launches = 0;
  double kernel_ms = 0.0;
  uint64_t timed_launches = 0;
  double summary_ms = 0.0;  // kernels of the last batched summary call (mhx_get_summary_timing)
};

namespace {

void drop_split_graph(mhx_engine* e);

int use_device(mhx_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  return MHX_OK;
}

// wait for whatever an engine has in its queue (error paths: nothing is reported from here)
void drain(mhx_engine* e) {
  if (hipSetDevice(e->device) == hipSuccess && e->stream) (void)hipStreamSynchronize(e->stream);
}

// The slice table of the tile-sliced split mode: function k, slice s = windows [s per_k,
// (s + 1) per_k) of its dataset, as a FnDesc of its own (what k_split_tsweep hands to sweep()).
int build_ts_table(mhx_engine* e, int ts) {
  std::vector<FnDesc> tab((size_t)e->P.K * ts);
  // one function, one window per slice, one persistent launch: a sweep workgroup's window stays
  // in its LDS from its first round on (sweep(): FnDesc::solo; no DMA, no tile barriers and no
  // layout vote in the rounds after it)
  bool resident = e->persist && e->P.K == 1 && kPadPoints <= 2 * e->fam->tile_points;
  for (int k = 0; k < e->P.K; ++k) {
    const FnDesc& f = e->P.fn[k];
    const int64_t nwin = (f.n + kPadPoints - 1) / kPadPoints;
    const int64_t per = (nwin + ts - 1) / ts;
    for (int sl = 0; sl < ts; ++sl) {
      FnDesc g = f;
      const int64_t off = (int64_t)sl * per * kPadPoints;
      g.lik_const = 0.0;
      g.solo = 0;
      resident = resident && per == 1;
      if (off >= f.n) {
        g.n = 0;
        g.n_tiles = 0;
      } else {
        g.n = std::min<int64_t>(per * kPadPoints, f.n - off);
        g.n_tiles = (g.n + e->fam->tile_points - 1) / e->fam->tile_points;
        g.x = f.x + off;
        g.y = f.y + off;
        if (f.w) g.w = f.w + off;
        if (f.c) g.c = f.c + off;
        if (f.txlo) g.txlo = f.txlo + off / kPadPoints;
        if (f.txhi) g.txhi = f.txhi + off / kPadPoints;
        if (f.tgh) g.tgh = f.tgh + off / kPadPoints;
      }
      tab[(size_t)k * ts + sl] = g;
    }
  }
  if (resident && !e->knobs.no_resident_slices)
    for (FnDesc& g : tab) g.solo = g.n_tiles > 0 ? 1 : 0;
  if (e->ts_table.n < tab.size() && e->ts_table.alloc(tab.size(), false) != hipSuccess)
    return fail(MHX_ENOMEM, "hipMalloc of the slice table failed");
  HIP_TRY(hipMemcpy(e->ts_table.p, tab.data(), tab.size() * sizeof(FnDesc), hipMemcpyHostToDevice));
  return MHX_OK;
}

// one of a dataset's per-window tables (mhx_finalize.hpp), on the device
int upload_table(DevBuf<double>& buf, const std::vector<double>& tab, int k, const char* what) {
  if (buf.alloc(tab.size(), false) != hipSuccess)
    return fail(MHX_ENOMEM, "hipMalloc of dataset %d's %s failed", k, what);
  HIP_TRY(hipMemcpy(buf.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  return MHX_OK;
}

// The split modes' partial sums and the persistent kernels' handshake blocks, for the launch form
// that was planned.
int alloc_split_buffers(mhx_engine* e) {
  e->S.split_slots = e->tsplit ? e->split_slices : e->split_slices * e->fam->waves_per_group;
  e->S.split_part = nullptr;
  if (e->tsplit) {
    const int rc = build_ts_table(e, e->split_slices);
    if (rc != MHX_OK) return rc;
  }
  HIP_TRY(hipMemset(e->split_pending.p, 0, (size_t)e->cfg.n_chains * sizeof(int32_t)));
  if (e->split_slices == 0) return MHX_OK;
  // (tile-sliced: room for the most slices a later re-slicing may take - compact_tsplit)
  const size_t slots_max = e->tsplit ? (size_t)std::max<int64_t>(e->S.split_slots, std::min<int64_t>(e->shape.nwin, 512))
                                     : (size_t)e->S.split_slots;
  const size_t np = (size_t)e->cfg.n_chains * e->P.K * slots_max;
  if (e->split_part.alloc(np) != hipSuccess)
    return fail(MHX_ENOMEM, "hipMalloc of the split-mode partial sums failed");
  e->S.split_part = e->split_part.p;
  if (e->persist) {  // (the handshake blocks of the persistent kernels: mhx_types.hpp)
    const size_t nm = 64 * (size_t)e->cfg.n_chains;
    const size_t npb = 16 * np;
    if ((e->persist_msg.n < nm && e->persist_msg.alloc(nm) != hipSuccess) ||
        (e->persist_part.n < npb && e->persist_part.alloc(npb) != hipSuccess))
      return fail(MHX_ENOMEM, "hipMalloc of the persistent kernel's handshake buffers failed");
    if (!e->persist_error.p && e->persist_error.alloc(1) != hipSuccess)
      return fail(MHX_ENOMEM, "hipMalloc of the persistent kernel's error word failed");
    e->S.persist_msg = e->persist_msg.p;
    e->S.persist_part = e->persist_part.p;
    e->S.persist_error = e->persist_error.p;
  }
  return MHX_OK;
}

// Every rule below is a function of mhx_finalize.hpp or mhx_plan.hpp; what is done here is the
// allocating, uploading and compiling between them.
int finalize_problem(mhx_engine* e) {
  if (!e->problem_dirty) return MHX_OK;
  e->knobs = read_knobs();
  const EngineKnobs& kn = e->knobs;
  ProblemDesc& P = e->P;
  drop_split_graph(e);
  // a new problem may run in another mode and family: slot s is chain s until the next deal
  e->S.slot_chain = nullptr;
  e->S.n_slots = e->cfg.n_chains;
  e->slots_mapped = 0;
  // 1. is everything there
  const bool pooled = e->cfg.adapt_mode == MHX_ADAPT_POOLED;
  FnInput in[MHX_MAX_FUNCTIONS];
  for (int k = 0; k < P.K; ++k) {
    in[k].fn_set = e->fn_set[k];
    in[k].data_set = e->data[k].set;
    in[k].planes = e->data[k].planes;
    in[k].expr = &e->fn_expr[k];
    in[k].recog = &e->fn_recog[k];
    in[k].prior_expr = !e->prior_expr[k].expr.empty();
    in[k].lik_expr = !e->lik_expr[k].empty();
  }
  if (Refusal r = validate_problem(P, in, pooled)) return fail(r.code, "%s", r.msg.c_str());
  // 2. the shape the mode rules read, and the kernel family: it fixes the tile size and with it
  // the tiles per dataset
  ProblemShape& sh = e->shape;
  sh = ProblemShape{};
  for (int k = 0; k < P.K; ++k) {
    sh.longest = std::max<int64_t>(sh.longest, P.fn[k].n);
    sh.planes = sh.planes || in[k].planes;
  }
  sh.nwin = ceil_div(sh.longest, kPadPoints);
  sh.K = P.K;
  sh.d = P.d;
  sh.chains = e->cfg.n_chains;
  sh.pooled = pooled;
  sh.persist_off = e->persist_off;
  sh.cus = e->cus;
  e->fam = choose_family(sh, kn) == 16 ? &family_w16() : &family_w8();
  sh.waves_per_group = e->fam->waves_per_group;
  sh.tile_points = e->fam->tile_points;
  // 3. the windows' x ranges and grids
  for (int k = 0; k < P.K; ++k) {
    FnDesc& f = P.fn[k];
    Dataset& D = e->data[k];
    std::vector<double> lo, hi, gh;
    window_ranges(D.hx.data(), D.n, &lo, &hi);
    int rc = upload_table(D.txlo, lo, k, "tile ranges");
    if (rc == MHX_OK) rc = upload_table(D.txhi, hi, k, "tile ranges");
    if (rc != MHX_OK) return rc;
    f.txlo = D.txlo.p;
    f.txhi = D.txhi.p;
    f.n_tiles = ceil_div(f.n, e->fam->tile_points);
    // (a dataset that is ONE grid needs no table; MHX_NO_WINDOW_GRIDS=1: round 3's rule, one
    // grid or none)
    f.tgh = nullptr;
    if (f.grid_H == 0.0 && !D.no_rec && !kn.no_window_grids && window_grids(D.hx.data(), D.n, &gh)) {
      rc = upload_table(D.tgh, gh, k, "window grids");
      if (rc != MHX_OK) return rc;
      f.tgh = D.tgh.p;
    }
    // the one tile stays in LDS (sweep).  Measured (tools/ab_tree.sh, test.lisp's shape): +9 %
    // with one chain, -5 % with 512 and -15 % with 2048 chains: only the single-walker case, the
    // reference's own way of working, gets it.  (A dataset per walker: no resident tile, a sweep
    // of its own, planes_loglik.)
    f.solo = D.planes ? 2 : (P.K == 1 && f.n_tiles == 1 && e->cfg.n_chains <= e->fam->waves_per_group) ? 1 : 0;
  }
  // 4. a dataset per walker: resident in the tile buffers or streamed, and where
  bool planes_res = false;
  if (sh.planes) {
    PlanesFn pf[MHX_MAX_FUNCTIONS];
    PlanesLayout pl[MHX_MAX_FUNCTIONS];
    for (int k = 0; k < P.K; ++k) pf[k] = PlanesFn{in[k].planes, P.fn[k].n, e->data[k].sigma_kind};
    planes_res = planes_layout(pf, P.K, e->fam->waves_per_group, kn, pl);
    for (int k = 0; k < P.K; ++k) {
      Dataset& D = e->data[k];
      if (!D.planes) continue;
      D.pd.resident = pl[k].resident;
      D.pd.bit = pl[k].bit;
      D.pd.off_x = pl[k].off_x;
      D.pd.off_w = pl[k].off_w;
      D.pd.off_rows = pl[k].off_rows;
      D.pd.row_stride = pl[k].row_stride;
      HIP_TRY(hipMemcpy(D.pdesc.p, &D.pd, sizeof(PlaneDesc), hipMemcpyHostToDevice));
      P.fn[k].c = reinterpret_cast<const double*>(D.pdesc.p);
    }
  }
  // 5. what the expressions run as; the switches the kernels read.  MHX_NO_TILE_SKIP=1: every
  // Gaussian peak at every point (the skipping is exact, so this only exists to show that the
  // results do not change); MHX_NO_YW=1: the shared-tile layout with x for every step;
  // MHX_NO_DEAL=1: every wave judges its own chain's proposal (A/B runs; same bits either way)
  for (int k = 0; k < P.K; ++k) {
    P.fn[k].tile_skip = kn.no_tile_skip ? 0 : 1;
    P.fn[k].no_yw = kn.no_yw ? 1 : 0;
  }
  P.no_deal = kn.no_deal ? 1 : 0;
  P.test_lose_sweepers = 0;
#ifdef MHX_DEBUG_HOOKS  // (tests/hooks/libmhx_hooks.so: a persistent launch whose sweepers never come)
  P.test_lose_sweepers = kn.test_lose_sweepers ? 1 : 0;
#endif
  if (Refusal r = resolve_functions(P, in, e->recognise && !kn.no_recognise)) return fail(r.code, "%s", r.msg.c_str());
  sh.heavy = heavy_problem(P);
  // 6. which kernels
  bool has_tgh[MHX_MAX_FUNCTIONS];
  for (int k = 0; k < P.K; ++k) has_tgh[k] = P.fn[k].tgh != nullptr;
  KernelChoice choice = choose_kernels(P, in, has_tgh, pooled, kn);
  // 7. the program compiled at run time, or - enumerated models only - the generic kernels
  // instead (no hiprtc on this machine?)
  e->rtc_note.clear();
  std::shared_ptr<UserProgram> prog;
  if (choice.rtc) {
    std::vector<UserExpr> priors;
    for (int k = 0; k < P.K; ++k)
      if (choice.fn[k].prior_slot >= 0) priors.push_back(e->prior_expr[k]);
    std::string err;
    prog = rtc_get(program_models(choice, e->fn_expr, e->lik_expr), priors, choice.builtin_fallback,
                   want_split(sh, kn, !choice.builtin_fallback), *e->fam, &err);
    if (!prog && choice.compile_required)
      return fail(MHX_EUNSUPPORTED, "%s%s", sh.planes ? "a dataset per walker needs kernels compiled at run time: " : "",
                  err.c_str());
    if (!prog) {
      e->rtc_note = err.substr(0, err.find('\n'));
      fall_back_to_generic(&choice);
    }
  }
  e->user_prog = prog;
  e->spec = choice.rtc ? SPEC_USER : choice.spec;
  // 8. the problem as the kernels read it
  apply_choice(choice, &P);
  HIP_TRY(hipMemcpy(e->dP.p, &P, sizeof(ProblemDesc), hipMemcpyHostToDevice));
  // 9. the launch form (mhx_plan.hpp) ...
  sh.capable = e->spec == SPEC_USER ? e->user_prog->has_split : e->fam->split_capable(e->spec);
  if (sh.capable) {
    for (int ts = 0; ts < 2; ++ts)
      (ts ? sh.per_cu_ts : sh.per_cu) = e->spec == SPEC_USER ? rtc_persist_per_cu(*e->user_prog, ts)
                                                             : e->fam->persist_per_cu(e->spec, ts);
  }
  const LaunchPlan plan = plan_modes(sh, kn);
  e->tsplit = plan.tsplit;
  e->split_slices = plan.split_slices;
  e->persist = plan.persist;
  e->ts_initial = plan.ts_initial;
  // 10. ... its tables and buffers
  const int rc = alloc_split_buffers(e);
  if (rc != MHX_OK) return rc;
  // 11. a name for what was chosen (mhx_kernel_name)
  e->kernel_name = kernel_name(choice, e->fam->waves_per_group, planes_res, plan, e->rtc_note);
  e->problem_dirty = false;
  return MHX_OK;
}

// launch through the ahead-of-time table or the run-time compiled module
hipError_t do_logpost(mhx_engine* e, const double* th, int64_t n, double* out, double* parts) {
  return e->spec == SPEC_USER
             ? rtc_launch_logpost(*e->user_prog, e->stream, e->dP.p, th, n, out, parts)
             : e->fam->logpost(e->spec, e->stream, e->dP.p, th, n, out, parts);
}
hipError_t do_init(mhx_engine* e) {
  return e->spec == SPEC_USER ? rtc_launch_init(*e->user_prog, e->stream, e->dP.p, e->S)
                              : e->fam->init(e->spec, e->stream, e->dP.p, e->S);
}
hipError_t do_step_injected(mhx_engine* e, const double* L, int pcl, const double* z,
                            const double* u, const double* T, unsigned char* acc) {
  return e->spec == SPEC_USER
             ? rtc_launch_step_injected(*e->user_prog, e->stream, e->dP.p, e->S, L, pcl, z, u, T, acc)
             : e->fam->step_injected(e->spec, e->stream, e->dP.p, e->S, L, pcl, z, u, T, acc);
}
hipError_t do_split_sweep(mhx_engine* e) {
  if (e->tsplit)
    return e->spec == SPEC_USER
               ? rtc_launch_split_tsweep(*e->user_prog, e->stream, e->dP.p, e->ts_table.p, e->S,
                                         e->split_slices)
               : e->fam->split_tsweep(e->spec, e->stream, e->dP.p, e->ts_table.p, e->S,
                                      e->split_slices);
  return e->spec == SPEC_USER
             ? rtc_launch_split_sweep(*e->user_prog, e->stream, e->dP.p, e->S, e->split_slices)
             : e->fam->split_sweep(e->spec, e->stream, e->dP.p, e->S, e->split_slices);
}
hipError_t do_split_step(mhx_engine* e, int mode, int plain) {
  return e->spec == SPEC_USER
             ? rtc_launch_split_step(*e->user_prog, e->stream, e->dP.p, e->S, e->R, mode, plain)
             : e->fam->split_step(e->spec, e->stream, e->dP.p, e->S, e->R, mode, plain);
}
hipError_t do_persist(mhx_engine* e, int64_t iters, int plain) {
  if (e->tsplit)
    return e->spec == SPEC_USER
               ? rtc_launch_persist_ts(*e->user_prog, e->stream, e->dP.p, e->ts_table.p, e->S, e->R,
                                       e->split_slices, iters, plain)
               : e->fam->persist_ts(e->spec, e->stream, e->dP.p, e->ts_table.p, e->S, e->R,
                                    e->split_slices, iters, plain);
  return e->spec == SPEC_USER
             ? rtc_launch_persist(*e->user_prog, e->stream, e->dP.p, e->S, e->R, e->split_slices, iters, plain)
             : e->fam->persist(e->spec, e->stream, e->dP.p, e->S, e->R, e->split_slices, iters, plain);
}
hipError_t do_adaptive(mhx_engine* e, int64_t iters, int plain) {
  return e->spec == SPEC_USER
             ? rtc_launch_adaptive(*e->user_prog, e->stream, e->dP.p, e->S, e->R, iters, plain)
             : e->fam->adaptive(e->spec, e->stream, e->dP.p, e->S, e->R, iters, plain);
}

int check_model(int model, const int32_t* shape, int n_shape, int n_index) {
  switch (model) {
    case MHX_MODEL_POLY:
      if (n_index < 1) return fail(MHX_EINVAL, "POLY needs >= 1 parameter");
      return MHX_OK;
    case MHX_MODEL_GAUSS_PEAKS:
    case MHX_MODEL_LORENTZ_PEAKS:
      if (n_shape < 2 || shape[0] < 0 || shape[1] < 0 || shape[0] + 3 * shape[1] != n_index)
        return fail(MHX_EINVAL, "peaks model: shape {nbg,npk} must satisfy nbg+3*npk == n_index");
      return MHX_OK;
    case MHX_MODEL_LORDER_MIXED:
      return n_index == 6 ? MHX_OK : fail(MHX_EINVAL, "LORDER_MIXED takes 6 parameters");
    case MHX_MODEL_EXP_DECAY:
      return n_index == 3 ? MHX_OK : fail(MHX_EINVAL, "EXP_DECAY takes 3 parameters");
    case MHX_MODEL_SINUSOID:
      return n_index == 4 ? MHX_OK : fail(MHX_EINVAL, "SINUSOID takes 4 parameters");
    case MHX_MODEL_PVOIGT2:
      return n_index == 11 ? MHX_OK : fail(MHX_EINVAL, "PVOIGT2 takes 11 parameters");
    default:
      return fail(MHX_EINVAL, "unknown model id %d", model);
  }
}

// (log_factorial_ref, the Poisson constant of M:379-380: mhx_heldout.hpp, which forms it for
// mhx_get_heldout too)

int alloc_state(mhx_engine* e) {
  const int64_t C = e->cfg.n_chains;
  const int d = e->cfg.n_params;
  const int64_t sts = steps_to_settle_of(d);
  int want = e->cfg.history_capacity > 0 ? e->cfg.history_capacity : 1024;
  want = std::max<int>(want, (int)std::max<int64_t>(1000, sts));
  const int Rcap = pow2_ceil(want);
  auto& S = e->S;
  S.n_chains = C;
  S.slot_chain = nullptr;
  S.n_slots = (int64_t)C;
  S.chain_offset = e->cfg.chain_offset;
  S.d = d;
  S.R = Rcap;
  S.seed = e->cfg.seed;
#define ALLOC(buf, count)                                             \
  if (e->buf.alloc((size_t)(count)) != hipSuccess)                    \
    return fail(MHX_ENOMEM, "hipMalloc of %s (%zu elements) failed", #buf, (size_t)(count));
  ALLOC(theta, C * d);
  ALLOC(prob, C);
  ALLOC(best_theta, C * d);
  ALLOC(best_prob, C);
  ALLOC(length, C);
  ALLOC(age, C);
  ALLOC(draw, C);
  ALLOC(n_hist, C);
  ALLOC(hist_prob, C * Rcap);
  ALLOC(hist_theta, C * Rcap * d);
  ALLOC(L, C * d * d);
  ALLOC(temperature, C);
  ALLOC(loop_i, C);
  ALLOC(reset_index, C);
  ALLOC(shutting, C);
  ALLOC(status, C);
  ALLOC(fwd_idx, C * sts);
  ALLOC(mat_tmp, C * 2 * d * d);
  ALLOC(pool_stats, C * (1 + d + d * d));
  ALLOC(stop_flag, 1);
  ALLOC(step_counter, 1);
  ALLOC(pool_vec, 1 + d + d * d);
  ALLOC(L_pool, d * d);
  ALLOC(pool_valid, 1);
  ALLOC(split_prop, C * d);
  ALLOC(split_u, C);
  ALLOC(split_pending, C);
#undef ALLOC
  S.theta = e->theta.p;
  S.prob = e->prob.p;
  S.best_theta = e->best_theta.p;
  S.best_prob = e->best_prob.p;
  S.length = e->length.p;
  S.age = e->age.p;
  S.draw = e->draw.p;
  S.n_hist = e->n_hist.p;
  S.hist_prob = e->hist_prob.p;
  S.hist_theta = e->hist_theta.p;
  S.L = e->L.p;
  S.temperature = e->temperature.p;
  S.loop_i = e->loop_i.p;
  S.reset_index = e->reset_index.p;
  S.shutting = e->shutting.p;
  S.status = e->status.p;
  S.fwd_idx = e->fwd_idx.p;
  S.mat_tmp = e->mat_tmp.p;
  S.pool_stats = e->pool_stats.p;
  S.step_counter = e->step_counter.p;
  S.pool_vec = e->pool_vec.p;
  S.L_pool = e->L_pool.p;
  S.pool_valid = e->pool_valid.p;
  S.split_prop = e->split_prop.p;
  S.split_u = e->split_u.p;
  S.split_pending = e->split_pending.p;
  S.split_part = nullptr;
  S.split_slots = 0;
  return MHX_OK;
}

void drop_split_graph(mhx_engine* e) {
  if (e->split_graph) (void)hipGraphExecDestroy(e->split_graph);
  e->split_graph = nullptr;
  e->split_graph_iters = 0;
  e->split_graph_plain = -1;
}

// `bytes` of staging memory, 256-byte aligned pieces carved by the caller
int ensure_stage(mhx_engine* e, size_t bytes) {
  if (e->stage.n >= bytes) return MHX_OK;
  const size_t want = std::max<size_t>(bytes, 2 * e->stage.n);
  if (e->stage.alloc(want, false) != hipSuccess)
    return fail(MHX_ENOMEM, "hipMalloc of %zu staging bytes failed", want);
  return MHX_OK;
}

// The slot -> chain map on the device (ChainState::slot_chain).  Grown whenever a deal needs more
// entries than it holds: which of compact_tsplit / compact_slots / deal_initial runs first depends
// on the problem the engine was finalised for, and the three need different lengths.
int put_slot_map(mhx_engine* e, const std::vector<int32_t>& map) {
  if (e->slot_map.n < map.size()) {
    HIP_TRY(hipStreamSynchronize(e->stream));  // (nobody reads the old map any more)
    drop_split_graph(e);                       // (its address is frozen into captured launches)
    e->S.slot_chain = nullptr;
    if (e->slot_map.alloc(map.size() + 64, false) != hipSuccess)
      return fail(MHX_ENOMEM, "hipMalloc of the slot map (%zu entries) failed", map.size());
  }
  HIP_TRY(hipMemcpy(e->slot_map.p, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  e->S.slot_chain = e->slot_map.p;
  e->S.n_slots = (int64_t)map.size();
  return MHX_OK;
}

// Chains that have finished give up their wave slots - where that pays.  In a long run of many
// chains the walks end at very different loop indices (:prob-settle), and a workgroup whose
// chains are mostly done carries idle waves through every tile of every sweep until its last
// chain ends.  But a wave that has its SIMD to itself runs at 39 % of the SIMD's issue rate where
// four sharing it get 25 % each, so as long as there is a CU for every workgroup the survivors
// are better left spread out (measured: packing 4096 chains' survivors made complete runs of
// config 2 8 % and of poly7 20 % SLOWER; dealing them evenly over the same 256 workgroups made
// them 20 % and 11 % faster).  So: the chains still walking are dealt round-robin over
// max(what they need, min(what the launch had, what the GPU holds)) workgroups, empty slots
// marked -1: every CU and SIMD gets its share of the waves that are left.  The chains' results do not depend on the slot they walk in (per-walker
// adaptation; Philox is keyed by the chain's global id; in the pooled mode the statistics kernels
// index chains, not slots, and the pooled factor is the same for every chain).  Batch kernels
// only (split mode has no idle waves).  MHX_NO_COMPACT=1: off.
// Tile-sliced split mode: the chains still walking are PACKED into as few groups as hold them
// (a group's workgroups walk their slices whether one of its chains is pending or all eight), and
// the functions are cut again so that the sweep launch keeps about 512 workgroups.  The partial
// sums are then grouped by other slices: results to rounding, like everything in the split modes.
int compact_tsplit(mhx_engine* e, const std::vector<int32_t>& st, int64_t running) {
  const int64_t W = e->fam->waves_per_group;
  const int64_t mapped = e->slots_mapped > 0 ? e->slots_mapped : e->cfg.n_chains;
  if (!repack_due(running, mapped)) return MHX_OK;
  const int64_t groups = ceil_div(running, W);
  std::vector<int32_t> map((size_t)(groups * W), -1);
  size_t j = 0;
  for (size_t c = 0; c < st.size(); ++c)
    if (st[c] == MHX_CHAIN_RUNNING) map[j++] = (int32_t)c;
  {
    const int rc = put_slot_map(e, map);
    if (rc != MHX_OK) return rc;
  }
  e->slots_mapped = running;
  const int64_t ts = reslice_tsplit(e->shape, e->knobs, e->split_slices, e->persist, groups);
  if (ts != e->split_slices) {
    const int rc = build_ts_table(e, (int)ts);
    if (rc != MHX_OK) return rc;
    e->split_slices = (int)ts;
    e->S.split_slots = (int)ts;
  }
  drop_split_graph(e);  // (the chain state is an argument frozen into the captured launches)
  return MHX_OK;
}

// a new run: every chain walks again, in the slices the problem was finalised with
int reset_tsplit(mhx_engine* e) {
  if (!e->tsplit || e->split_slices == e->ts_initial) return MHX_OK;
  const int rc = build_ts_table(e, e->ts_initial);
  if (rc != MHX_OK) return rc;
  e->split_slices = e->ts_initial;
  e->S.split_slots = e->ts_initial;
  return MHX_OK;
}

int compact_slots(mhx_engine* e, const std::vector<int32_t>& st, int64_t running) {
  if (e->knobs.no_compact || !e->fam) return MHX_OK;
  if (e->tsplit) {
    if (!e->ts_repack_due) return MHX_OK;
    e->ts_repack_due = false;
    return compact_tsplit(e, st, running);
  }
  if (e->split_slices > 0) return MHX_OK;
  const int64_t W = e->fam->waves_per_group;
  const int64_t in_use = e->S.slot_chain ? e->S.n_slots : e->cfg.n_chains;
  // chains mapped at the last deal (all of them before the first): a new deal when a quarter of
  // them has finished since.  With no more workgroups than the GPU holds their number stays, and
  // the deal only evens out how many waves each CU and SIMD still has to run.
  const int64_t mapped = e->slots_mapped > 0 ? e->slots_mapped : e->cfg.n_chains;
  if (!repack_due(running, mapped)) return MHX_OK;
  const int64_t target = deal_target(e->cus, W, in_use, running, e->knobs.compact_always);
  std::vector<int32_t> map((size_t)(target * W), -1);
  int64_t j = 0;
  for (size_t c = 0; c < st.size(); ++c)
    if (st[c] == MHX_CHAIN_RUNNING) {
      map[(size_t)((j % target) * W + j / target)] = (int32_t)c;
      ++j;
    }
  const int rc = put_slot_map(e, map);
  if (rc != MHX_OK) return rc;
  e->slots_mapped = running;
  return MHX_OK;
}

// ... and the same at the start of a run whose chains do not fill the GPU: 1024 chains are 128
// workgroups of 8 - two waves on every SIMD of half the CUs, the other half idle; dealt over 256
// workgroups of 4 every wave has a SIMD to itself.
int deal_initial(mhx_engine* e) {
  if (e->knobs.no_compact || e->split_slices > 0 || !e->fam) return MHX_OK;
  const int64_t W = e->fam->waves_per_group, C = e->cfg.n_chains;
  const int64_t target = deal_initial_target(e->cus, W, C);
  if (target == 0) return MHX_OK;
  std::vector<int32_t> map((size_t)(target * W), -1);
  for (int64_t c = 0; c < C; ++c) map[(size_t)((c % target) * W + c / target)] = (int32_t)c;
  const int rc = put_slot_map(e, map);
  if (rc != MHX_OK) return rc;
  e->slots_mapped = C;
  return MHX_OK;
}

// the start of a run (mhx_adaptive_begin, plain steps): the run-time switches read again, the
// problem finalised, every chain walking again in slot s = chain s and the slices the problem was
// finalised with; the run description is an argument frozen into the captured launches
int begin_run(mhx_engine* e) {
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  e->knobs = read_knobs();
  if ((rc = finalize_problem(e)) != MHX_OK) return rc;
  drop_split_graph(e);
  e->S.slot_chain = nullptr;
  e->S.n_slots = e->cfg.n_chains;
  e->slots_mapped = 0;
  e->split_iter = 0;
  e->ts_repack_due = false;
  return reset_tsplit(e);
}

int count_running(mhx_engine* e, int64_t* n_running) {
  std::vector<int32_t> st((size_t)e->cfg.n_chains);
  HIP_TRY(hipMemcpy(st.data(), e->status.p, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t r = 0;
  for (int32_t s : st) r += s == MHX_CHAIN_RUNNING;
  *n_running = r;
  return compact_slots(e, st, r);
}

// The temperature schedule of M:878, entries [lo, hi): (max 1 (* (cos (* x pi (+ 1 (* 2 (floor
// temp-steps 5000))) (/ (* 2 temp-steps)))) temperature)), products left to right, the rational
// factor converted to double.  The device holds a WINDOW of it over the loop indices the next
// launch can reach (every running chain that still anneals has loop index 1 + iterations since
// begin), so a run with n = 1e9 "until stopped" costs 32 MB, not 8 GB.
const int64_t kTempsWindow = [] {  // MHX_TEMPS_WINDOW: a small window for tests of the sliding
  const char* s = getenv("MHX_TEMPS_WINDOW");
  const long long v = s ? atoll(s) : 0;
  return (int64_t)(v >= 16 ? v : (1 << 22));
}();
int ensure_temps(mhx_engine* e, int64_t lo, int64_t hi) {
  RunDesc& R = e->R;
  hi = std::min(hi, R.temp_steps);
  if (lo >= hi) return MHX_OK;  // beyond the schedule: nothing is read
  if (lo >= R.temps_first && hi <= R.temps_first + e->temps_count) return MHX_OK;
  const int64_t top = std::min(R.temp_steps, lo + std::max<int64_t>(hi - lo, kTempsWindow));
  std::vector<double> temps((size_t)(top - lo));
  const double kfac = (double)(1 + 2 * (R.temp_steps / 5000));
  const double inv = 1.0 / (double)(2 * R.temp_steps);
  for (int64_t x = lo; x < top; ++x) {
    const double arg = (((double)x * M_PI) * kfac) * inv;
    const double v = std::cos(arg) * e->run_temperature;
    temps[(size_t)(x - lo)] = v > 1.0 ? v : 1.0;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));  // (a launch may still be reading the old window)
  if ((int64_t)e->temps.n < top - lo) {
    // the new buffer first, the old one released only once it exists: a failed allocation
    // leaves R.temps and the window it describes as they were
    DevBuf<double> fresh;
    if (fresh.alloc(temps.size(), false) != hipSuccess)
      return fail(MHX_ENOMEM, "hipMalloc(temperature schedule, %zu) failed", temps.size());
    std::swap(e->temps.p, fresh.p);
    std::swap(e->temps.n, fresh.n);
    R.temps = nullptr;  // (the old window went with `fresh`; set again below)
    e->temps_count = 0;
  }
  if (hipMemcpy(e->temps.p, temps.data(), temps.size() * sizeof(double), hipMemcpyHostToDevice) !=
      hipSuccess) {
    R.temps = nullptr;
    e->temps_count = 0;
    e->run_ready = false;  // no schedule on the device: the run cannot go on
    return fail(MHX_EDEVICE, "copying the temperature schedule to the device failed");
  }
  R.temps = e->temps.p;
  R.temps_first = lo;
  e->temps_count = top - lo;
  drop_split_graph(e);  // the run description is frozen into captured launches
  return MHX_OK;
}

// one timed launch of the fused step kernel: enqueue (returns without waiting, so that a group
// keeps every GPU busy at once) and finish (waits for it and does the accounting)
int launch_steps_finish(mhx_engine* e);
int launch_steps_enqueue(mhx_engine* e, int64_t iters, int plain) {
  if (e->launch_open) {
    const int rc = launch_steps_finish(e);
    if (rc != MHX_OK) return rc;
  }
  if (!plain) {
    const int rc = ensure_temps(e, e->global_iter + 1, e->global_iter + 1 + iters);
    if (rc != MHX_OK) return rc;
  }
  HIP_TRY(hipEventRecord(e->ev0, e->stream));
  if (e->split_slices > 0 && e->persist && !e->tsplit) {
    // persistent split mode: one launch, `iters` iterations (the kernel leaves its loop when no
    // chain is running any more); the sync words start every launch at zero
    // (launches of at most 2^22 iterations: what mhx_adaptive_advance asks for at most anyway)
    for (int64_t left = iters; left > 0; left -= (int64_t)1 << 22) {
      HIP_TRY(hipMemsetAsync(e->persist_msg.p, 0, e->persist_msg.n * sizeof(unsigned long long), e->stream));
      HIP_TRY(hipMemsetAsync(e->persist_part.p, 0, e->persist_part.n, e->stream));
      HIP_TRY(do_persist(e, std::min<int64_t>(left, (int64_t)1 << 22), plain));
      e->persist_launched = true;
      e->launches += 1;
    }
  } else if (e->split_slices > 0) {
    // split mode: prime (first half of iteration 1), then per iteration the sweep over all
    // slices and the chain's own launch (second half + first half of the next; the last one
    // leaves nothing outstanding).  2 * iters + 1 small launches, queued without waiting.
    // The batch kernel leaves its loop when no chain of the workgroup is running; here the HOST
    // drives the iterations, so they go out in portions with a look at the chain states between
    // them (the caller may ask for 2^40 iterations meaning "until done").
    int64_t left = iters;
    const int64_t portion = std::max<int64_t>(e->split_portion, 16);
    if (e->ts_repack_due) {  // the last launch ended on a portion boundary: look at the chains now
      int64_t running = 0;
      HIP_TRY(hipStreamSynchronize(e->stream));
      const int rc = count_running(e, &running);
      if (rc != MHX_OK) return rc;
      HIP_TRY(hipEventRecord(e->ev0, e->stream));
    }
    while (left > 0) {
      // (portions end where split_iter is a multiple of their length, whatever the caller asked for)
      const int64_t now = std::min<int64_t>(left, portion - e->split_iter % portion);
      // (round 4 tried ONE launch per iteration - the last workgroup of a chain group, by an
      // atomic ticket, running the group's step at the end of the sweep's launch: bit-identical,
      // and 27.7 us per iteration of 64 walkers where these two launches take 25.1: between two
      // nodes of a graph lie 0.3 us; what an iteration costs are the dependent memory round
      // trips inside both kernels, which the fusion only lines up behind a ticket)
      auto issue = [&](int64_t count) -> hipError_t {
        hipError_t he = do_split_step(e, 0, plain);
        for (int64_t it = 0; it < count && he == hipSuccess; ++it) {
          he = do_split_sweep(e);
          if (he == hipSuccess) he = do_split_step(e, it + 1 < count ? 1 : 2, plain);
        }
        return he;
      };
      // (only whole portions: a remainder of another length would mean capturing again)
      const bool use_graph = !e->knobs.no_graph && now == e->split_portion && !e->persist;
      bool done = false;
      if (e->persist) {  // tile-sliced, persistent: the portion is ONE launch (k_persist_ts)
        HIP_TRY(hipMemsetAsync(e->persist_msg.p, 0, e->persist_msg.n * sizeof(unsigned long long), e->stream));
        HIP_TRY(hipMemsetAsync(e->persist_part.p, 0, e->persist_part.n, e->stream));
        HIP_TRY(do_persist(e, now, plain));
        e->persist_launched = true;
        done = true;
      }
      if (use_graph) {
        if (!e->split_graph || e->split_graph_iters != now || e->split_graph_plain != plain) {
          drop_split_graph(e);
          hipGraph_t g = nullptr;
          if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const hipError_t he = issue(now);
            const hipError_t ce = hipStreamEndCapture(e->stream, &g);
            if (he == hipSuccess && ce == hipSuccess && g &&
                hipGraphInstantiate(&e->split_graph, g, nullptr, nullptr, 0) == hipSuccess) {
              e->split_graph_iters = now;
              e->split_graph_plain = plain;
            } else {
              e->split_graph = nullptr;
            }
            if (g) (void)hipGraphDestroy(g);
          }
          (void)hipGetLastError();
        }
        if (e->split_graph) {
          HIP_TRY(hipGraphLaunch(e->split_graph, e->stream));
          done = true;
        }
      }
      if (!done) HIP_TRY(issue(now));
      e->launches += e->persist ? 1 : 2 * (uint64_t)now + 1;
      left -= now;
      e->split_iter += now;
      e->ts_repack_due = e->tsplit && e->split_iter % portion == 0;
      if (left > 0) {
        int64_t running = 0;
        HIP_TRY(hipStreamSynchronize(e->stream));
        const int rc = count_running(e, &running);
        if (rc != MHX_OK) return rc;
        if (running == 0) break;
      }
    }
  } else {
    HIP_TRY(do_adaptive(e, iters, plain));
  }
  HIP_TRY(hipEventRecord(e->ev1, e->stream));
  e->launch_open = true;
  e->launch_iters = iters;
  // counted when the launch is in the queue, not when somebody has waited for it: the chains'
  // loop indices move with the kernel, and the schedule window and the pooled cadence of the
  // next launch are derived from this count whatever happens on the host in between
  if (!plain) e->global_iter += iters;
  return MHX_OK;
}
int launch_steps_finish(mhx_engine* e) {
  if (!e->launch_open) return MHX_OK;
  e->launch_open = false;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipEventSynchronize(e->ev1));
  if (e->persist_launched) {
    // a persistent launch counts on all its workgroups being on the GPU at once; when another
    // kernel held it, a master gave up waiting for its sweep workgroups: the iteration was taken
    // back (no chain was touched), this run is over, and the engine returns to two launches
    e->persist_launched = false;
    int32_t err = 0;
    HIP_TRY(hipMemcpy(&err, e->persist_error.p, sizeof err, hipMemcpyDeviceToHost));
    if (err != 0) {
      HIP_TRY(hipMemset(e->persist_error.p, 0, sizeof err));
      e->persist = false;
      e->persist_off = true;
      e->problem_dirty = true;  // (modes and kernel name are derived again, without persistence)
      e->run_ready = false;
      return fail(MHX_EDEVICE, "a persistent launch did not get all its workgroups onto the GPU at once "
                               "(another kernel held it); no chain was touched - begin again "
                               "(the engine now uses two launches per iteration)");
    }
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  e->kernel_ms += ms;
  e->timed_launches++;
  e->launches++;
  // keep a launch near 50 ms so the stop flag and the host stay responsive
  if (ms > 0.f) {
    double per_iter = ms / (double)std::max<int64_t>(e->launch_iters, 1);
    int64_t want = (int64_t)(50.0 / std::max(per_iter, 1e-6));
    e->chunk_iters = std::min<int64_t>(std::max<int64_t>(want, 8), 1 << 16);
  }
  return MHX_OK;
}
int launch_steps(mhx_engine* e, int64_t iters, int plain) {
  const int rc = launch_steps_enqueue(e, iters, plain);
  return rc != MHX_OK ? rc : launch_steps_finish(e);
}

// Pooled adaptation tick (MHX_ADAPT_POOLED): per-chain displacement statistics -> sum over the
// chains of this rank (fixed order) -> all-reduce over ranks (caller's hook: RCCL through
// torch.distributed, or any MPI-like sum) -> covariance, Cholesky, 2.38^2/d on every rank.
// (with an RCCL communicator everything stays on the engine's stream: no host synchronisation
// between the statistics kernels, the all-reduce and the factorisation)
int pool_enqueue_stats(mhx_engine* e) {
  HIP_TRY(e->fam->pool_stats(e->stream, e->S, e->R));
  HIP_TRY(e->fam->pool_reduce(e->stream, e->S));
  return MHX_OK;
}
int pool_enqueue_allreduce(mhx_engine* e) {  // inside ncclGroupStart/End when a group drives it
  const size_t E = 1 + (size_t)e->P.d + (size_t)e->P.d * e->P.d;
  const int rc = rccl().AllReduce(e->pool_vec.p, e->pool_vec.p, E, kNcclDouble, kNcclSum, e->comm,
                                  e->stream);
  if (rc != 0)
    return fail(MHX_ECOMM, "ncclAllReduce: %s", rccl_err(rc));
  return MHX_OK;
}
int pool_enqueue_factor(mhx_engine* e) {
  HIP_TRY(e->fam->pool_factor(e->stream, e->S));
  e->launches += 3;
  e->pool_refreshes++;
  return MHX_OK;
}
int pool_refresh(mhx_engine* e) {
  const size_t E = 1 + (size_t)e->P.d + (size_t)e->P.d * e->P.d;
  if (e->comm) {
    int rc = pool_enqueue_stats(e);
    if (rc == MHX_OK) rc = pool_enqueue_allreduce(e);
    if (rc == MHX_OK) rc = pool_enqueue_factor(e);
    return rc;  // stream-ordered before the next step launch
  }
  HIP_TRY(e->fam->pool_stats(e->stream, e->S, e->R));
  HIP_TRY(e->fam->pool_reduce(e->stream, e->S));
  if (e->allreduce) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    int rc;
    if (e->allreduce_device) {
      rc = e->allreduce(e->allreduce_ctx, e->pool_vec.p, E, 1);
    } else {
      std::vector<double> h(E);
      HIP_TRY(hipMemcpy(h.data(), e->pool_vec.p, E * sizeof(double), hipMemcpyDeviceToHost));
      rc = e->allreduce(e->allreduce_ctx, h.data(), E, 0);
      if (rc == 0)
        HIP_TRY(hipMemcpy(e->pool_vec.p, h.data(), E * sizeof(double), hipMemcpyHostToDevice));
    }
    if (rc != 0) return fail(MHX_ECOMM, "all-reduce hook returned %d", rc);
  }
  HIP_TRY(e->fam->pool_factor(e->stream, e->S));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->launches += 3;
  e->pool_refreshes++;
  return MHX_OK;
}

}  // namespace

extern "C" {

int mhx_version(void) { return MHX_VERSION; }
#ifndef MHX_SOURCE_ID
#define MHX_SOURCE_ID "unknown"
#endif
#ifdef MHX_DEBUG_HOOKS
const char* mhx_build_id(void) { return "csrc:" MHX_SOURCE_ID "+hooks"; }
#else
const char* mhx_build_id(void) { return "csrc:" MHX_SOURCE_ID; }
#endif
const char* mhx_last_error(void) { return g_err.c_str(); }

int mhx_device_count(int* count) {
  if (!count) return fail(MHX_EINVAL, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(MHX_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return MHX_OK;
}

int mhx_create(const mhx_config* cfg, mhx_engine** out) {
  if (!cfg || !out) return fail(MHX_EINVAL, "cfg/out is NULL");
  *out = nullptr;
  if (cfg->n_chains < 1) return fail(MHX_EINVAL, "n_chains must be >= 1");
  if (cfg->n_params < 1 || cfg->n_params > MHX_MAX_PARAMS)
    return fail(MHX_EINVAL, "n_params must be in [1,%d]", MHX_MAX_PARAMS);
  if (cfg->n_functions < 1 || cfg->n_functions > MHX_MAX_FUNCTIONS)
    return fail(MHX_EINVAL, "n_functions must be in [1,%d]", MHX_MAX_FUNCTIONS);
  if (cfg->adapt_mode != MHX_ADAPT_FAITHFUL && cfg->adapt_mode != MHX_ADAPT_POOLED)
    return fail(MHX_EINVAL, "adapt_mode");
  if ((uint64_t)(cfg->chain_offset + cfg->n_chains) > 0xFFFFFFFFull)
    return fail(MHX_EINVAL, "global chain ids must fit 32 bits (Philox counter word)");
  int ndev = 0;
  hipError_t he = hipGetDeviceCount(&ndev);
  if (he != hipSuccess || ndev <= 0)
    return fail(MHX_EDEVICE, "no HIP device available (%s): libmhx has no CPU path",
                he != hipSuccess ? hipGetErrorString(he) : "0 devices");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(MHX_EINVAL, "device %d out of range (have %d)", cfg->device, ndev);
  mhx_engine* e = new (std::nothrow) mhx_engine();
  if (!e) return fail(MHX_ENOMEM, "host allocation failed");
  e->cfg = *cfg;
  e->device = cfg->device;
  int rc = MHX_OK;
  do {
    if ((rc = use_device(e)) != MHX_OK) break;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) != hipSuccess) {
      rc = fail(MHX_EDEVICE, "hipGetDeviceProperties failed");
      break;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !getenv("MHX_ALLOW_ANY_ARCH")) {
      rc = fail(MHX_EDEVICE, "device %d is %s; libmhx is built for gfx950 (MI355X) only",
                e->device, prop.gcnArchName);
      break;
    }
    if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess ||
        e->cus <= 0)
      e->cus = 256;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&e->stop_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) {
      rc = fail(MHX_EDEVICE, "stream/event creation failed");
      break;
    }
    if (family_w8().configure() != hipSuccess || family_w16().configure() != hipSuccess ||
        summary_configure() != hipSuccess || model_readouts_configure() != hipSuccess) {
      rc = fail(MHX_EDEVICE, "hipFuncSetAttribute(max dynamic LDS = %zu / %zu) failed",
                family_w8().lds_bytes, family_w16().lds_bytes);
      break;
    }
    if (e->dP.alloc(1) != hipSuccess) {
      rc = fail(MHX_ENOMEM, "hipMalloc(ProblemDesc) failed");
      break;
    }
    e->P.d = cfg->n_params;
    e->P.K = cfg->n_functions;
    if ((rc = alloc_state(e)) != MHX_OK) break;
    e->R.stop_flag = e->stop_flag.p;
  } while (0);
  if (rc != MHX_OK) {
    std::string keep = g_err;
    mhx_destroy(e);
    g_err = keep;
    return rc;
  }
  *out = e;
  return MHX_OK;
}

void mhx_destroy(mhx_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->comm && e->comm_owned && rccl().ok) (void)rccl().CommDestroy(e->comm);
  e->comm = nullptr;
  drop_split_graph(e);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  if (e->stop_stream) (void)hipStreamDestroy(e->stop_stream);
  delete e;
}

int mhx_set_function(mhx_engine* e, int k, int model_id, const int32_t* shape, int n_shape,
                     const int32_t* param_index, int n_index) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "function index %d out of range", k);
  if (n_index < 0 || n_index > MHX_MAX_FN_PARAMS || (n_index > 0 && !param_index))
    return fail(MHX_EINVAL, "n_index must be in [0,%d]", MHX_MAX_FN_PARAMS);
  if (n_shape < 0 || n_shape > 4 || (n_shape > 0 && !shape)) return fail(MHX_EINVAL, "n_shape");
  int rc = check_model(model_id, shape, n_shape, n_index);
  if (rc != MHX_OK) return rc;
  FnDesc& f = e->P.fn[k];
  for (int j = 0; j < n_index; ++j) {
    if (param_index[j] < 0 || param_index[j] >= e->P.d)
      return fail(MHX_EINVAL, "param_index[%d] = %d outside [0,%d)", j, param_index[j], e->P.d);
    f.idx[j] = param_index[j];
  }
  f.model = model_id;
  e->fn_expr[k] = UserExpr();
  e->fn_recog[k] = RecognisedModel();
  f.n_idx = n_index;
  for (int i = 0; i < 4; ++i) f.shape[i] = i < n_shape ? shape[i] : 0;
  e->fn_set[k] = true;
  e->problem_dirty = true;
  return MHX_OK;
}

// x1: the second column of a vector-valued x (mhx_set_dataset_cols), or NULL
static int set_dataset_impl(mhx_engine* e, int k, const double* x, const double* x1, const double* y,
                            const double* sigma, size_t n, int likelihood) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "dataset index %d out of range", k);
  if (n > 0 && (!x || !y)) return fail(MHX_EINVAL, "x/y is NULL");
  if (likelihood < MHX_LIK_NORMAL || likelihood > MHX_LIK_EXPR)
    return fail(MHX_EINVAL, "unknown likelihood %d", likelihood);
  if (x1 && likelihood == MHX_LIK_NORMAL_CUTOFF)
    return fail(MHX_EUNSUPPORTED, "a second column of x with log-liklihood-normal-cutoff: the tiles' "
                                  "fourth array is taken by the clamp's per-point constants");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  // padded to a whole number of tiles of either kernel family
  const size_t np = std::max<size_t>((n + kPadPoints - 1) / kPadPoints, 1) * kPadPoints;
  std::vector<double> hx(np), hy(np), hw(np), hc(np);
  long double csum = 0.0L;
  const double half_log_2pi = -0.5 * std::log(2.0 * M_PI);  // (* -1/2 (log (* 2 pi))) M:377
  std::vector<float> lf_cache;
  std::vector<double> hconst(likelihood == MHX_LIK_POISSON || (x1 && likelihood == MHX_LIK_NORMAL) ? n : 0);
  for (size_t i = 0; i < n; ++i) {
    hx[i] = x[i];
    hy[i] = y[i];
    if (likelihood == MHX_LIK_POISSON) {
      if (!(y[i] >= 0.0) || y[i] != std::floor(y[i]) || y[i] > 1e9)
        return fail(MHX_EINVAL, "poisson count y[%zu] = %g is not a non-negative integer", i, y[i]);
      hw[i] = 0.0;
      hc[i] = 0.0;
      hconst[i] = -log_factorial_ref((long)y[i], e->cfg.poisson_logfact_double != 0, lf_cache);
      csum += (long double)hconst[i];
    } else if (likelihood == MHX_LIK_EXPR) {
      hw[i] = sigma ? sigma[i] : 1.0;  // handed to the expression as `error`, untouched
      hc[i] = 0.0;
    } else {
      const double s = sigma ? sigma[i] : 1.0;  // (if data-error data-error 1) M:1144
      if (!(s > 0.0) || !std::isfinite(s))
        return fail(MHX_EINVAL, "sigma[%zu] = %g must be finite and > 0 (M:376)", i, s);
      hw[i] = 1.0 / s;
      hy[i] = y[i] * hw[i];  // the kernel forms r = y/sigma - m/sigma with one fma
      hc[i] = half_log_2pi + (-1.0 * std::log(s));  // first two terms of M:377
      csum += (long double)hc[i];
    }
  }
  for (size_t i = n; i < np; ++i) {  // neutral pads: r = (0 - m) * 0 = 0
    hx[i] = n ? x[n - 1] : 0.0;
    hy[i] = 0.0;
    hw[i] = 0.0;
    hc[i] = 0.0;
  }
  if (x1 && likelihood == MHX_LIK_NORMAL) std::copy(hc.begin(), hc.begin() + n, hconst.begin());
  if (x1)  // (the c array is read by the cutoff likelihood only, which was refused above)
    for (size_t i = 0; i < np; ++i) hc[i] = n ? x1[i < n ? i : n - 1] : 0.0;
  Dataset& D = e->data[k];
  if (D.x.alloc(np, false) != hipSuccess || D.y.alloc(np, false) != hipSuccess ||
      D.w.alloc(np, false) != hipSuccess || D.c.alloc(np, false) != hipSuccess)
    return fail(MHX_ENOMEM, "hipMalloc of dataset %d (%zu points) failed", k, np);
  HIP_TRY(hipMemcpy(D.x.p, hx.data(), np * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.y.p, hy.data(), np * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.w.p, hw.data(), np * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.c.p, hc.data(), np * sizeof(double), hipMemcpyHostToDevice));
  FnDesc& f = e->P.fn[k];
  f.x = D.x.p;
  f.y = D.y.p;
  f.w = D.w.p;
  f.c = D.c.p;
  f.txlo = f.txhi = nullptr;  // per-tile x ranges and n_tiles: finalize_problem, per family
  f.n = (int64_t)n;
  f.n_tiles = 0;
  D.hx.swap(hx);
  D.hconst.swap(hconst);
  f.lik = likelihood;
  f.lik_const = (double)csum;
  f.xmin = f.xmax = n ? x[0] : 0.0;
  for (size_t i = 1; i < n; ++i) {
    f.xmin = std::min(f.xmin, x[i]);
    f.xmax = std::max(f.xmax, x[i]);
  }
  // A uniformly spaced x grid (spectra, histograms, time series: x_i = x_0 + i h) lets the
  // Gaussian peaks advance by a two-multiply recurrence instead of an exp per point
  // (PeaksModel, csrc/mhx_device.hpp).  Accepted when the n points are a grid of step
  // h = (x_(n-1) - x_0) / (n - 1) (mhx_finalize.hpp: grid_step); MHX_NO_RECURRENCE=1 keeps the
  // direct form.
  const char* nr = getenv("MHX_NO_RECURRENCE");
  D.no_rec = nr && atoi(nr) != 0;
  f.grid_H = D.no_rec ? 0.0 : 64.0 * grid_step(x, n);
  f.tgh = nullptr;  // (per-window grids: finalize_problem)
  f.n_xcols = x1 ? 2 : 1;
  D.n = n;
  D.set = true;
  if (D.planes) {  // (a shared dataset replaces a dataset per walker)
    D.planes = false;
    D.py.release();
    D.pw.release();
    D.pconst.release();
  }
  e->problem_dirty = true;
  return MHX_OK;
}

static int planes_refuse_lik(int likelihood) {
  static const char* kName[] = {"MHX_LIK_NORMAL", "MHX_LIK_NORMAL_CUTOFF", "MHX_LIK_POISSON", "MHX_LIK_EXPR"};
  if (likelihood < MHX_LIK_NORMAL || likelihood > MHX_LIK_EXPR)
    return fail(MHX_EINVAL, "unknown likelihood %d", likelihood);
  if (likelihood != MHX_LIK_NORMAL)
    return fail(MHX_EUNSUPPORTED, "a dataset per walker (mhx_set_dataset_planes) with %s: only "
                                  "MHX_LIK_NORMAL has a per-walker sweep", kName[likelihood]);
  return MHX_OK;
}

int mhx_set_dataset_planes(mhx_engine* e, int k, const double* x, const double* y,
                           const double* sigma, int sigma_kind, size_t n, int likelihood) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "dataset index %d out of range", k);
  if (n == 0 || !x || !y) return fail(MHX_EINVAL, "mhx_set_dataset_planes: n == 0 or x / y is NULL");
  if (sigma_kind < MHX_SIGMA_NONE || sigma_kind > MHX_SIGMA_PER_POINT ||
      (sigma_kind != MHX_SIGMA_NONE) != (sigma != nullptr))
    return fail(MHX_EINVAL, "mhx_set_dataset_planes: sigma_kind %d does not go with a%s sigma",
                sigma_kind, sigma ? "" : " NULL");
  int rc = planes_refuse_lik(likelihood);
  if (rc != MHX_OK) return rc;
  if (e->cfg.adapt_mode == MHX_ADAPT_POOLED)
    return fail(MHX_EUNSUPPORTED, "a dataset per walker (mhx_set_dataset_planes) with "
                                  "MHX_ADAPT_POOLED: one pooled covariance assumes one posterior");
  const size_t C = (size_t)e->cfg.n_chains;
  const size_t ns = sigma_kind == MHX_SIGMA_SHARED ? n : sigma_kind == MHX_SIGMA_PER_CHAIN ? C
                    : sigma_kind == MHX_SIGMA_PER_POINT ? C * n : 0;
  for (size_t i = 0; i < ns; ++i)
    if (!(sigma[i] > 0.0) || !std::isfinite(sigma[i]))
      return fail(MHX_EINVAL, "sigma[%zu] = %g must be finite and > 0 (M:376)", i, sigma[i]);
  // x, its ranges and grid, and the shared 1/sigma: as a shared dataset (row 0 stands in for y)
  rc = set_dataset_impl(e, k, x, nullptr, y, sigma_kind == MHX_SIGMA_SHARED ? sigma : nullptr, n,
                        MHX_LIK_NORMAL);
  if (rc != MHX_OK) return rc;
  Dataset& D = e->data[k];
  D.set = false;  // (until the planes are in place)
  const size_t pitch = ((n + kPlanePad - 1) / kPlanePad) * kPlanePad;
  const bool wplane = sigma_kind == MHX_SIGMA_PER_POINT;
  const bool wscalar = sigma_kind == MHX_SIGMA_PER_CHAIN || sigma_kind == MHX_SIGMA_NONE;
  std::vector<double> hy(C * pitch, 0.0), hw(wplane ? C * pitch : (wscalar ? C : 1), 0.0), hc(C);
  const double half_log_2pi = -0.5 * std::log(2.0 * M_PI);
  for (size_t c = 0; c < C; ++c) {
    long double csum = 0.0L;
    for (size_t i = 0; i < n; ++i) {  // (the arithmetic of set_dataset_impl, point by point)
      const double sg = sigma_kind == MHX_SIGMA_NONE ? 1.0
                        : sigma_kind == MHX_SIGMA_SHARED ? sigma[i]
                        : sigma_kind == MHX_SIGMA_PER_CHAIN ? sigma[c] : sigma[c * n + i];
      const double w = 1.0 / sg;
      hy[c * pitch + i] = y[c * n + i] * w;
      if (wplane) hw[c * pitch + i] = w;
      else if (wscalar) hw[c] = w;
      csum += (long double)(half_log_2pi + (-1.0 * std::log(sg)));
    }
    hc[c] = (double)csum;
  }
  if (D.py.alloc(hy.size(), false) != hipSuccess || D.pw.alloc(hw.size(), false) != hipSuccess ||
      D.pconst.alloc(C, false) != hipSuccess || (!D.pdesc.p && D.pdesc.alloc(1) != hipSuccess))
    return fail(MHX_ENOMEM, "hipMalloc of dataset %d (%zu walkers x %zu points) failed", k, C, pitch);
  HIP_TRY(hipMemcpy(D.py.p, hy.data(), hy.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.pw.p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.pconst.p, hc.data(), C * sizeof(double), hipMemcpyHostToDevice));
  D.pd = PlaneDesc{};
  D.pd.y = D.py.p;
  D.pd.w = D.pw.p;
  D.pd.lik_const = D.pconst.p;
  D.pd.n_rows = (int64_t)C;
  D.pd.pitch = (int64_t)pitch;
  D.pd.w_kind = wplane ? kPlaneWPlane : (wscalar ? kPlaneWScalar : kPlaneWShared);
  D.sigma_kind = sigma_kind;
  D.planes = true;
  D.set = true;
  e->problem_dirty = true;
  return MHX_OK;
}

int mhx_set_dataset(mhx_engine* e, int k, const double* x, const double* y, const double* sigma,
                    size_t n, int likelihood) {
  return set_dataset_impl(e, k, x, nullptr, y, sigma, n, likelihood);
}

int mhx_set_dataset_cols(mhx_engine* e, int k, const double* const* xcols, int n_cols,
                         const double* y, const double* sigma, size_t n, int likelihood) {
  if (!xcols || n_cols < 1 || n_cols > 2 || !xcols[0] || (n_cols == 2 && !xcols[1]))
    return fail(MHX_EINVAL, "x must come as 1 or 2 columns (%d given)", n_cols);
  return set_dataset_impl(e, k, xcols[0], n_cols == 2 ? xcols[1] : nullptr, y, sigma, n, likelihood);
}

int mhx_set_bounds(mhx_engine* e, int k, const int32_t* idx, const double* lo, const double* hi,
                   int n) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "function index %d out of range", k);
  if (n < 0 || n > MHX_MAX_BOUNDS || (n > 0 && (!idx || !lo || !hi)))
    return fail(MHX_EINVAL, "n bounds must be in [0,%d]", MHX_MAX_BOUNDS);
  FnDesc& f = e->P.fn[k];
  for (int i = 0; i < n; ++i) {
    if (idx[i] >= e->P.d) return fail(MHX_EINVAL, "bounds idx[%d] = %d outside the vector", i, idx[i]);
    f.bidx[i] = idx[i] < 0 ? -1 : idx[i];
    f.blo[i] = lo[i];
    f.bhi[i] = hi[i];
  }
  f.n_bounds = n;
  e->problem_dirty = true;
  return MHX_OK;
}

// does `expr` mention the identifier `id` (as a whole word)?
static bool expr_names(const char* expr, const char* id) {
  const size_t n = strlen(id);
  for (const char* p = expr; (p = strstr(p, id)) != nullptr; p += n) {
    const bool left = p == expr || !(isalnum((unsigned char)p[-1]) || p[-1] == '_');
    const bool right = !(isalnum((unsigned char)p[n]) || p[n] == '_');
    if (left && right) return true;
  }
  return false;
}
static bool valid_ident(const char* s) {
  if (!s || !(isalpha((unsigned char)s[0]) || s[0] == '_')) return false;
  for (const char* p = s; *p; ++p)
    if (!(isalnum((unsigned char)*p) || *p == '_')) return false;
  return strcmp(s, "x") != 0 && strcmp(s, "xcol0") != 0 && strcmp(s, "xcol1") != 0 &&
         strcmp(s, "bounds_total") != 0;
}

int mhx_set_function_expr(mhx_engine* e, int k, const char* expr, const char* const* param_names,
                          const int32_t* param_index, int n_index) {
  if (!e || !expr) return fail(MHX_EINVAL, "engine/expr is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "function index %d out of range", k);
  if (n_index < 0 || n_index > MHX_MAX_FN_PARAMS || (n_index > 0 && (!param_names || !param_index)))
    return fail(MHX_EINVAL, "n_index must be in [0,%d]", MHX_MAX_FN_PARAMS);
  UserExpr u;
  for (int j = 0; j < n_index; ++j) {
    if (!valid_ident(param_names[j]))
      return fail(MHX_EINVAL, "parameter name %d is not an identifier (or is x / bounds_total)", j);
    if (param_index[j] < 0 || param_index[j] >= e->P.d)
      return fail(MHX_EINVAL, "param_index[%d] = %d outside [0,%d)", j, param_index[j], e->P.d);
    u.names.push_back(param_names[j]);
    u.index.push_back(param_index[j]);
  }
  std::string err;
  if (rtc_prepare_expr(expr, u.names, "x xcol0 xcol1", &u.expr, &err) != 0)
    return fail(MHX_EINVAL, "%s", err.c_str());
  u.xcols = expr_names(expr, "xcol1") ? 2 : 1;
  FnDesc& f = e->P.fn[k];
  f.model = MHX_MODEL_EXPR;
  f.n_idx = n_index;
  for (int j = 0; j < n_index; ++j) f.idx[j] = param_index[j];
  for (int i = 0; i < 4; ++i) f.shape[i] = 0;
  e->fn_expr[k] = u;
  (void)rtc_recognise(expr, u.names, &e->fn_recog[k]);  // which kernels: finalize_problem
  e->fn_set[k] = true;
  e->problem_dirty = true;
  return MHX_OK;
}

int mhx_expr_classify(const char* expr, const char* const* param_names, int n_names,
                      int32_t* model, int32_t* shape, int32_t* order, int32_t* n_order) {
  if (!expr || !model) return fail(MHX_EINVAL, "expr/model is NULL");
  if (n_names < 0 || n_names > MHX_MAX_FN_PARAMS || (n_names > 0 && !param_names))
    return fail(MHX_EINVAL, "n_names must be in [0,%d]", MHX_MAX_FN_PARAMS);
  std::vector<std::string> names;
  for (int j = 0; j < n_names; ++j) {
    if (!valid_ident(param_names[j]))
      return fail(MHX_EINVAL, "parameter name %d is not an identifier (or is x / bounds_total)", j);
    names.push_back(param_names[j]);
  }
  std::string out, err;
  if (rtc_prepare_expr(expr, names, "x xcol0 xcol1", &out, &err) != 0) return fail(MHX_EINVAL, "%s", err.c_str());
  RecognisedModel r;
  (void)rtc_recognise(expr, names, &r);
  *model = r.model >= 0 ? r.model : MHX_MODEL_EXPR;
  if (shape) {
    shape[0] = r.shape[0];
    shape[1] = r.shape[1];
  }
  if (n_order) *n_order = (int32_t)r.order.size();
  if (order)
    for (size_t j = 0; j < r.order.size(); ++j) order[j] = r.order[j];
  return MHX_OK;
}

int mhx_set_expr_recognition(mhx_engine* e, int on) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  e->recognise = on != 0;
  e->problem_dirty = true;
  return MHX_OK;
}

int mhx_set_prior_expr(mhx_engine* e, int k, const char* expr, const char* const* names,
                       const int32_t* index, int n) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "function index %d out of range", k);
  if (!expr || !*expr) {  // back to the plain bounds-total body
    e->prior_expr[k] = UserExpr();
    e->problem_dirty = true;
    return MHX_OK;
  }
  if (n < 0 || n > MHX_MAX_PARAMS || (n > 0 && (!names || !index)))
    return fail(MHX_EINVAL, "n must be in [0,%d]", MHX_MAX_PARAMS);
  UserExpr u;
  for (int j = 0; j < n; ++j) {
    if (!valid_ident(names[j])) return fail(MHX_EINVAL, "name %d is not an identifier", j);
    if (index[j] < 0 || index[j] >= e->P.d)
      return fail(MHX_EINVAL, "index[%d] = %d outside [0,%d)", j, index[j], e->P.d);
    u.names.push_back(names[j]);
    u.index.push_back(index[j]);
  }
  // the macro also binds <key>-bound, the penalty of that one key (M:356-360, docstring M:348):
  // identifier <name>_bound, encoded as index -(g+1)
  for (int j = 0; j < n; ++j) {
    u.names.push_back(std::string(names[j]) + "_bound");
    u.index.push_back(-(index[j] + 1));
  }
  std::string err;
  if (rtc_prepare_expr(expr, u.names, "bounds_total", &u.expr, &err) != 0)
    return fail(MHX_EINVAL, "%s", err.c_str());
  e->prior_expr[k] = u;
  e->problem_dirty = true;
  return MHX_OK;
}

int mhx_set_likelihood_expr(mhx_engine* e, int k, const char* expr) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (k < 0 || k >= e->P.K) return fail(MHX_EINVAL, "function index %d out of range", k);
  if (!expr || !*expr) return fail(MHX_EINVAL, "likelihood expression is empty");
  std::string out, err;
  if (rtc_prepare_expr(expr, std::vector<std::string>(), "y model error", &out, &err) != 0)
    return fail(MHX_EINVAL, "%s", err.c_str());
  e->lik_expr[k] = out;
  e->problem_dirty = true;
  return MHX_OK;
}

// in two halves, so that a group has every device working before it waits for the first
static int init_chains_enqueue(mhx_engine* e, const double* theta0, int broadcast) {
  if (!e || !theta0) return fail(MHX_EINVAL, "engine/theta0 is NULL");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if ((rc = finalize_problem(e)) != MHX_OK) return rc;
  const int64_t C = e->cfg.n_chains;
  const int d = e->P.d;
  if (broadcast) {
    std::vector<double> full((size_t)C * d);
    for (int64_t c = 0; c < C; ++c) memcpy(&full[(size_t)c * d], theta0, sizeof(double) * d);
    HIP_TRY(hipMemcpy(e->theta.p, full.data(), full.size() * sizeof(double), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(e->theta.p, theta0, (size_t)C * d * sizeof(double), hipMemcpyHostToDevice));
  }
  e->chains_ready = false;
  e->run_ready = false;
  HIP_TRY(do_init(e));
  return MHX_OK;
}
static int init_chains_finish(mhx_engine* e) {
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->launches++;
  e->chains_ready = true;
  return MHX_OK;
}
int mhx_init_chains(mhx_engine* e, const double* theta0, int broadcast) {
  const int rc = init_chains_enqueue(e, theta0, broadcast);
  return rc != MHX_OK ? rc : init_chains_finish(e);
}

int mhx_logpost(mhx_engine* e, const double* theta, size_t n, double* out, double* parts) {
  if (!e || (n > 0 && (!theta || !out))) return fail(MHX_EINVAL, "NULL argument");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if ((rc = finalize_problem(e)) != MHX_OK) return rc;
  if (n == 0) return MHX_OK;
  if (e->shape.planes && n > (size_t)INT32_MAX)  // (a wave keeps its row in 32 bits: plane_walker_set)
    return fail(MHX_EINVAL, "mhx_logpost on a dataset per walker takes at most 2^31 - 1 rows");
  const int d = e->P.d;
  const size_t o_th = 0, o_out = align256(n * d * sizeof(double)),
               o_parts = o_out + align256(n * sizeof(double));
  if ((rc = ensure_stage(e, o_parts + 2 * n * sizeof(double))) != MHX_OK) return rc;
  double* dth = reinterpret_cast<double*>(e->stage.p + o_th);
  double* dout = reinterpret_cast<double*>(e->stage.p + o_out);
  double* dparts = reinterpret_cast<double*>(e->stage.p + o_parts);
  HIP_TRY(hipMemcpy(dth, theta, n * d * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(do_logpost(e, dth, (int64_t)n, dout, dparts));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->launches++;
  HIP_TRY(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
  if (parts) HIP_TRY(hipMemcpy(parts, dparts, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_step_injected(mhx_engine* e, const double* L, int per_chain_l, const double* z,
                      const double* u, const double* T, uint8_t* accepted_out) {
  if (!e || !L || !z || !u || !T) return fail(MHX_EINVAL, "NULL argument");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if ((rc = finalize_problem(e)) != MHX_OK) return rc;
  const size_t C = (size_t)e->cfg.n_chains, d = (size_t)e->P.d;
  const size_t nL = (per_chain_l ? C : 1) * d * d;
  const size_t o_z = align256(nL * sizeof(double)), o_u = o_z + align256(C * d * sizeof(double)),
               o_T = o_u + align256(C * sizeof(double)), o_acc = o_T + align256(C * sizeof(double));
  if ((rc = ensure_stage(e, o_acc + C)) != MHX_OK) return rc;
  double* dL = reinterpret_cast<double*>(e->stage.p);
  double* dz = reinterpret_cast<double*>(e->stage.p + o_z);
  double* du = reinterpret_cast<double*>(e->stage.p + o_u);
  double* dT = reinterpret_cast<double*>(e->stage.p + o_T);
  unsigned char* dacc = e->stage.p + o_acc;
  HIP_TRY(hipMemcpy(dL, L, nL * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dz, z, C * d * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(du, u, C * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dT, T, C * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(dacc, 0, C));
  HIP_TRY(do_step_injected(e, dL, per_chain_l, dz, du, dT, dacc));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->launches++;
  if (accepted_out) HIP_TRY(hipMemcpy(accepted_out, dacc, C, hipMemcpyDeviceToHost));
  return MHX_OK;
}

void mhx_run_opts_default(mhx_run_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->n = 100000;         // (n 100000)        M:862
  o->temperature = 1e3;  // (temperature 1d3) M:862
  o->auto_mode = 1;      // (auto (or :prob-settle :slope-settle nil)) evaluates to :prob-settle
}

static int adaptive_begin_enqueue(mhx_engine* e, const mhx_run_opts* o) {
  if (!e || !o) return fail(MHX_EINVAL, "NULL argument");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (o->n < 0) return fail(MHX_EINVAL, "n must be >= 0");
  if (o->auto_mode != 0 && o->auto_mode != 1)
    return fail(MHX_EUNSUPPORTED, ":slope-settle is outside the accelerated path");
  if (!(o->temperature > 0.0) || !std::isfinite(o->temperature))
    return fail(MHX_EINVAL, "temperature must be finite and > 0");
  int rc = begin_run(e);
  if (rc != MHX_OK) return rc;
  if ((rc = deal_initial(e)) != MHX_OK) return rc;
  const int d = e->P.d;
  RunDesc& R = e->R;
  R.n = o->n;                                       // (floor n) M:866
  R.sts = steps_to_settle_of(d);                    // M:873
  R.temp_steps = std::max<int64_t>(R.n, 10 * R.sts);  // M:875
  R.tail = std::max<int64_t>(2000, R.sts);          // (max 2000 steps-to-settle) M:906, M:917
  R.auto_mode = o->auto_mode;
  R.has_mwl = o->max_walker_length > 0;
  R.mwl = o->max_walker_length / 2;  // (floor max-walker-length 2) M:868
  R.adapt_mode = e->cfg.adapt_mode;
  R.stop_flag = e->stop_flag.p;
  if (R.has_mwl && R.mwl < 1) return fail(MHX_EINVAL, "max_walker_length must be >= 2");
  // temps M:878: the first window now, the rest as the loop gets there (ensure_temps)
  e->run_temperature = o->temperature;
  e->temps_count = 0;
  R.temps_first = 0;
  e->global_iter = 0;
  if ((rc = ensure_temps(e, 0, std::min<int64_t>(R.temp_steps, kTempsWindow))) != MHX_OK) return rc;
  HIP_TRY(hipMemset(e->stop_flag.p, 0, sizeof(int32_t)));  // (setf mfit-walker-estop nil) M:865
  const size_t C = (size_t)e->cfg.n_chains, dd = (size_t)d * d;
  if (o->l_matrix) {
    if (o->l_matrix_per_chain) {
      HIP_TRY(hipMemcpy(e->L.p, o->l_matrix, C * dd * sizeof(double), hipMemcpyHostToDevice));
    } else {
      std::vector<double> full(C * dd);
      for (size_t c = 0; c < C; ++c) memcpy(&full[c * dd], o->l_matrix, dd * sizeof(double));
      HIP_TRY(hipMemcpy(e->L.p, full.data(), full.size() * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  e->run_ready = false;
  HIP_TRY(hipMemsetAsync(e->pool_valid.p, 0, sizeof(int32_t), e->stream));
  HIP_TRY(e->fam->initial_l(e->stream, e->S, R, o->l_matrix ? 1 : 0, o->temperature));
  return MHX_OK;
}
static int adaptive_begin_finish(mhx_engine* e) {
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->launches++;
  e->run_ready = true;
  e->global_iter = 0;
  return MHX_OK;
}
int mhx_adaptive_begin(mhx_engine* e, const mhx_run_opts* o) {
  const int rc = adaptive_begin_enqueue(e, o);
  return rc != MHX_OK ? rc : adaptive_begin_finish(e);
}

// A failure between begin and the end of a run leaves host and device bookkeeping apart (some
// launches went out, others did not): the run is over, a new mhx_adaptive_begin starts the next.
static int run_failed(mhx_engine* e, int rc) {
  e->run_ready = false;
  return rc;
}

int mhx_adaptive_advance(mhx_engine* e, int64_t max_iters, int64_t* n_running) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->run_ready) return fail(MHX_ESTATE, "mhx_adaptive_begin has not been called");
  if (e->problem_dirty) {
    e->run_ready = false;
    return fail(MHX_ESTATE, "the problem was changed after mhx_adaptive_begin: begin again");
  }
  if (max_iters < 0) return fail(MHX_EINVAL, "max_iters < 0");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if (e->cfg.adapt_mode == MHX_ADAPT_POOLED) {
    // launches end on the pooled cadence (every 200 iterations since begin), where the
    // displacement statistics of all chains and ranks are combined
    int64_t left = max_iters;
    while (left > 0) {
      const int64_t to_tick = 200 - (e->global_iter % 200);
      const int64_t now = std::min(left, to_tick);
      if ((rc = launch_steps(e, now, 0)) != MHX_OK) return run_failed(e, rc);
      left -= now;
      if (e->global_iter % 200 == 0 && (rc = pool_refresh(e)) != MHX_OK) return run_failed(e, rc);
    }
  } else {
    // (one launch per call unless it would outrun the schedule window: then window by window,
    // looking at the chains in between - "until done" is asked for as 2^40 iterations)
    int64_t left = max_iters;
    while (left > 0) {
      const int64_t now = std::min(left, kTempsWindow);
      if ((rc = launch_steps(e, now, 0)) != MHX_OK) return run_failed(e, rc);
      left -= now;
      if (left > 0) {
        int64_t running = 0;
        if ((rc = count_running(e, &running)) != MHX_OK) return run_failed(e, rc);
        if (running == 0) break;
      }
    }
  }
  if (n_running && (rc = count_running(e, n_running)) != MHX_OK) return run_failed(e, rc);
  return MHX_OK;
}

int mhx_adaptive_steps_full(mhx_engine* e, const mhx_run_opts* o) {
  int rc = mhx_adaptive_begin(e, o);
  if (rc != MHX_OK) return rc;
  int64_t running = 1;
  while (running > 0) {
    if ((rc = mhx_adaptive_advance(e, e->chunk_iters, &running)) != MHX_OK) return rc;
  }
  return MHX_OK;
}

int mhx_adaptive_steps(mhx_engine* e, int64_t n) {
  mhx_run_opts o;
  mhx_run_opts_default(&o);
  o.n = n;               // (walker-adaptive-steps-full walker :n n :temperature 10
  o.temperature = 10.0;  //                              :auto :prob-settle) M:947
  o.auto_mode = 1;
  return mhx_adaptive_steps_full(e, &o);
}

static int plain_steps(mhx_engine* e, int64_t n, const double* L, int per_chain_l, double T);

int mhx_many_steps(mhx_engine* e, int64_t n, const double* L, int per_chain_l) {
  return plain_steps(e, n, L, per_chain_l, 1.0);
}

int mhx_take_step(mhx_engine* e, const double* L, int per_chain_l, double temperature) {
  if (!(temperature > 0.0) || !std::isfinite(temperature))
    return fail(MHX_EINVAL, "temperature must be finite and > 0");
  return plain_steps(e, 1, L, per_chain_l, temperature);
}

// (dotimes (i n) (walker-take-step w :l-matrix L :temperature T)) M:852-853, M:1072-1095
static int plain_steps(mhx_engine* e, int64_t n, const double* L, int per_chain_l, double T) {
  if (!e || !L)
    return fail(MHX_EINVAL, "NULL argument (the nil :l-matrix defaults of M:851 / M:1074 are "
                            "formed by the host shims from mhx_get_trace)");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (n < 0) return fail(MHX_EINVAL, "n < 0");
  int rc = begin_run(e);
  if (rc != MHX_OK) return rc;
  const size_t C = (size_t)e->cfg.n_chains, dd = (size_t)e->P.d * e->P.d;
  if (per_chain_l) {
    HIP_TRY(hipMemcpy(e->L.p, L, C * dd * sizeof(double), hipMemcpyHostToDevice));
  } else {
    std::vector<double> full(C * dd);
    for (size_t c = 0; c < C; ++c) memcpy(&full[c * dd], L, dd * sizeof(double));
    HIP_TRY(hipMemcpy(e->L.p, full.data(), full.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // (dotimes (i n) (walker-take-step w :l-matrix L)) M:852-853: loop index 0..n-1, T = 1
  RunDesc& R = e->R;
  R.n = n;
  R.sts = steps_to_settle_of(e->P.d);
  R.temp_steps = 0;
  R.tail = 0;
  R.auto_mode = 0;
  R.has_mwl = 0;
  R.temps = nullptr;
  R.stop_flag = e->stop_flag.p;
  HIP_TRY(hipMemset(e->stop_flag.p, 0, sizeof(int32_t)));
  {
    std::vector<int64_t> zero(C, 0);
    std::vector<int32_t> st(C), run(C, MHX_CHAIN_RUNNING);
    std::vector<double> one(C, T);
    HIP_TRY(hipMemcpy(st.data(), e->status.p, C * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c)
      if (st[c] == MHX_CHAIN_FP_TRAP) run[c] = MHX_CHAIN_FP_TRAP;
    HIP_TRY(hipMemcpy(e->loop_i.p, zero.data(), C * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->status.p, run.data(), C * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->temperature.p, one.data(), C * sizeof(double), hipMemcpyHostToDevice));
  }
  int64_t running = 1;
  while (running > 0) {
    if ((rc = launch_steps(e, e->chunk_iters, 1)) != MHX_OK) return rc;
    if ((rc = count_running(e, &running)) != MHX_OK) return rc;
  }
  e->run_ready = false;
  return MHX_OK;
}

int mhx_request_stop(mhx_engine* e) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  static const int32_t one = 1;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(e->stop_flag.p, &one, sizeof one, hipMemcpyHostToDevice, e->stop_stream));
  HIP_TRY(hipStreamSynchronize(e->stop_stream));
  return MHX_OK;
}

int mhx_set_allreduce(mhx_engine* e, mhx_allreduce_fn fn, void* ctx, int wants_device_buffer) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  // a hook set after mhx_comm_init_rank replaces the library's own communicator (which would
  // otherwise take precedence in pool_refresh): the caller has decided that every rank exchanges
  // through the hook
  if (fn && e->comm) {
    if (e->comm_owned && rccl().ok) (void)rccl().CommDestroy(e->comm);
    e->comm = nullptr;
    e->comm_owned = false;
  }
  e->allreduce = fn;
  e->allreduce_ctx = ctx;
  e->allreduce_device = wants_device_buffer;
  return MHX_OK;
}

int mhx_get_state(mhx_engine* e, double* theta, double* logpost, double* best_theta,
                  double* best_logpost, int64_t* length, int64_t* age) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t C = (size_t)e->cfg.n_chains, d = (size_t)e->P.d;
  if (theta) HIP_TRY(hipMemcpy(theta, e->theta.p, C * d * sizeof(double), hipMemcpyDeviceToHost));
  if (logpost) HIP_TRY(hipMemcpy(logpost, e->prob.p, C * sizeof(double), hipMemcpyDeviceToHost));
  if (best_theta)
    HIP_TRY(hipMemcpy(best_theta, e->best_theta.p, C * d * sizeof(double), hipMemcpyDeviceToHost));
  if (best_logpost)
    HIP_TRY(hipMemcpy(best_logpost, e->best_prob.p, C * sizeof(double), hipMemcpyDeviceToHost));
  if (length) HIP_TRY(hipMemcpy(length, e->length.p, C * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (age) HIP_TRY(hipMemcpy(age, e->age.p, C * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_get_chain(mhx_engine* e, int64_t chain, double* theta, double* logpost,
                  double* best_theta, double* best_logpost, int64_t* length, int64_t* age) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (chain < 0 || chain >= e->cfg.n_chains) return fail(MHX_EINVAL, "chain out of range");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t d = (size_t)e->P.d, c = (size_t)chain;
  if (theta) HIP_TRY(hipMemcpy(theta, e->theta.p + c * d, d * sizeof(double), hipMemcpyDeviceToHost));
  if (logpost) HIP_TRY(hipMemcpy(logpost, e->prob.p + c, sizeof(double), hipMemcpyDeviceToHost));
  if (best_theta)
    HIP_TRY(hipMemcpy(best_theta, e->best_theta.p + c * d, d * sizeof(double), hipMemcpyDeviceToHost));
  if (best_logpost)
    HIP_TRY(hipMemcpy(best_logpost, e->best_prob.p + c, sizeof(double), hipMemcpyDeviceToHost));
  if (length) HIP_TRY(hipMemcpy(length, e->length.p + c, sizeof(int64_t), hipMemcpyDeviceToHost));
  if (age) HIP_TRY(hipMemcpy(age, e->age.p + c, sizeof(int64_t), hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_get_chain_status(mhx_engine* e, int32_t* status, int64_t* loop_index) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t C = (size_t)e->cfg.n_chains;
  if (status) HIP_TRY(hipMemcpy(status, e->status.p, C * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (loop_index)
    HIP_TRY(hipMemcpy(loop_index, e->loop_i.p, C * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_get_lmatrix(mhx_engine* e, double* L) {
  if (!e || !L) return fail(MHX_EINVAL, "NULL argument");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t C = (size_t)e->cfg.n_chains, dd = (size_t)e->P.d * e->P.d;
  HIP_TRY(hipMemcpy(L, e->L.p, C * dd * sizeof(double), hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_get_temperature(mhx_engine* e, double* T) {
  if (!e || !T) return fail(MHX_EINVAL, "NULL argument");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  HIP_TRY(hipMemcpy(T, e->temperature.p, (size_t)e->cfg.n_chains * sizeof(double),
                    hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_get_acceptance(mhx_engine* e, int take, double* out) {
  if (!e || !out) return fail(MHX_EINVAL, "NULL argument");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (take < 1) return fail(MHX_EINVAL, "take must be >= 1");
  if (take > e->S.R) return fail(MHX_EINVAL, "take %d exceeds history_capacity %d", take, e->S.R);
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t C = (size_t)e->cfg.n_chains;
  if ((rc = ensure_stage(e, C * sizeof(double))) != MHX_OK) return rc;
  double* d = reinterpret_cast<double*>(e->stage.p);
  HIP_TRY(e->fam->acceptance(e->stream, e->S, take, d));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, d, C * sizeof(double), hipMemcpyDeviceToHost));
  return MHX_OK;
}

int mhx_get_trace(mhx_engine* e, int64_t chain, int take, double* prob, double* theta,
                  int* n_out) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (chain < 0 || chain >= e->cfg.n_chains) return fail(MHX_EINVAL, "chain out of range");
  if (take < 0) return fail(MHX_EINVAL, "take < 0");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const int Rcap = e->S.R, d = e->P.d;
  int64_t nh = 0, len = 0;
  HIP_TRY(hipMemcpy(&nh, e->n_hist.p + chain, sizeof nh, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&len, e->length.p + chain, sizeof len, hipMemcpyDeviceToHost));
  int64_t avail = std::min<int64_t>(std::min<int64_t>(len, nh), Rcap);
  int t = (int)std::min<int64_t>(avail, take);
  if (n_out) *n_out = t;
  if (t == 0) return MHX_OK;
  // the newest t entries are ring slots (nh - t) ... (nh - 1) modulo the capacity: one or two
  // contiguous runs - only those are copied, oldest first, and turned round on the host
  const int64_t lo = (nh - t) & (int64_t)(Rcap - 1);
  const int64_t run1 = std::min<int64_t>(t, Rcap - lo), run2 = t - run1;
  std::vector<double> hp((size_t)t), ht;
  const double* rp = e->hist_prob.p + chain * Rcap;
  HIP_TRY(hipMemcpy(hp.data(), rp + lo, (size_t)run1 * sizeof(double), hipMemcpyDeviceToHost));
  if (run2 > 0)
    HIP_TRY(hipMemcpy(hp.data() + run1, rp, (size_t)run2 * sizeof(double), hipMemcpyDeviceToHost));
  if (theta) {
    ht.resize((size_t)t * d);
    const double* rt = e->hist_theta.p + chain * Rcap * d;
    HIP_TRY(hipMemcpy(ht.data(), rt + lo * d, (size_t)run1 * d * sizeof(double), hipMemcpyDeviceToHost));
    if (run2 > 0)
      HIP_TRY(hipMemcpy(ht.data() + run1 * d, rt, (size_t)run2 * d * sizeof(double),
                        hipMemcpyDeviceToHost));
  }
  for (int s = 0; s < t; ++s) {  // s = 0 is the newest = the last one copied
    const size_t src = (size_t)(t - 1 - s);
    if (prob) prob[s] = hp[src];
    if (theta) memcpy(theta + (size_t)s * d, &ht[src * d], sizeof(double) * d);
  }
  return MHX_OK;
}

int mhx_get_proposal_factor(mhx_engine* e, int64_t chain, int take, double* L_out, int* status,
                            int* n_forward) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (chain < 0 || chain >= e->cfg.n_chains) return fail(MHX_EINVAL, "chain out of range");
  if (take < 1 || take > e->S.R)
    return fail(MHX_EINVAL, "take must be in [1, history_capacity = %d]", e->S.R);
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t dd = (size_t)e->P.d * e->P.d;
  const size_t o_out = align256(dd * sizeof(double)), o_fwd = o_out + align256(dd * sizeof(double)),
               o_info = o_fwd + align256((size_t)take * sizeof(int32_t));
  if ((rc = ensure_stage(e, o_info + 2 * sizeof(int32_t))) != MHX_OK) return rc;
  double* cov = reinterpret_cast<double*>(e->stage.p);
  double* out = reinterpret_cast<double*>(e->stage.p + o_out);
  int32_t* fwd = reinterpret_cast<int32_t*>(e->stage.p + o_fwd);
  int32_t* info = reinterpret_cast<int32_t*>(e->stage.p + o_info);
  HIP_TRY(hipMemsetAsync(e->stage.p, 0, o_info + 2 * sizeof(int32_t), e->stream));
  HIP_TRY(e->fam->l_matrix(e->stream, e->S, chain, take, fwd, cov, out, info));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int32_t hinfo[2];
  HIP_TRY(hipMemcpy(hinfo, info, sizeof hinfo, hipMemcpyDeviceToHost));
  if (status) *status = hinfo[0];
  if (n_forward) *n_forward = hinfo[1];
  if (L_out) HIP_TRY(hipMemcpy(L_out, out, dd * sizeof(double), hipMemcpyDeviceToHost));
  return MHX_OK;
}

extern "C++" {
// ---- the batched read-outs of the history ring: walker-set-get, fit curves and bands, derived
// quantities.  Each works through its items - chains, or parameter vectors - in portions whose
// pieces (mhx_stage.hpp) stay below kStageBudget of the engine's stage buffer whatever the call's
// size.  A read-out is a call struct with
//   check(e)           the arguments against engine e, before anything is launched
//   items(e), points() what there is to work through (points: 1 unless x goes in chunks)
//   carve(e, c, n, m)  the pieces of n items at m points, taken from carver c
//   upload(e, p)       the copies and clears ahead of portion p's kernels (not timed)
//   launch(e, p)       ... its kernels
//   collect(e, p)      ... and its results, copied to the caller's arrays
// and dst[], its host destinations; run_portions() does the rest.

// a host destination: the caller's array at the engine's item 0 (may be NULL), bytes per item
struct HostDst {
  void* p = nullptr;
  size_t item_bytes = 0;
  void* at(int64_t item) const { return static_cast<unsigned char*>(p) + (size_t)item * item_bytes; }
};
template <class T>
static T* stage_at(const mhx_engine* e, size_t offset) {
  return reinterpret_cast<T*>(e->stage.p + offset);
}
// n items from item i0 on: from the stage buffer to a destination
static int copy_back(const HostDst& h, int64_t i0, int64_t n, const void* dev) {
  if (h.p && h.item_bytes > 0)
    HIP_TRY(hipMemcpy(h.at(i0), dev, (size_t)n * h.item_bytes, hipMemcpyDeviceToHost));
  return MHX_OK;
}
// ... the pieces at off[k] of the stage to dst[k], k < N: portion p's results of one value per item
template <size_t N>
static int copy_back_each(const mhx_engine* e, const HostDst* dst, const Portion& p, const size_t (&off)[N]) {
  for (size_t k = 0; k < N; ++k) {
    const int rc = copy_back(dst[k], p.i0, p.n, e->stage.p + off[k]);
    if (rc != MHX_OK) return rc;
  }
  return MHX_OK;
}
// ... and a pointwise result that arrives a chunk of points at a time: `rows` rows per item of p.m
// points each, `per` bytes a point, to their places p.m0 .. in the caller's rows of m points
static int copy_back_points(const HostDst& h, const Portion& p, int64_t m, size_t per, size_t rows, const void* dev) {
  if (h.p && rows > 0)
    HIP_TRY(hipMemcpy2D(static_cast<unsigned char*>(h.at(p.i0)) + (size_t)p.m0 * per, (size_t)m * per, dev,
                        (size_t)p.m * per, (size_t)p.m * per, (size_t)p.n * rows, hipMemcpyDeviceToHost));
  return MHX_OK;
}
// the window of a read-out of the chains' histories
static int window_check(const mhx_engine* e, int take) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (take < 1 || take > e->S.R)
    return fail(MHX_EINVAL, "take must be in [1, history_capacity = %d]", e->S.R);
  return MHX_OK;
}
// function fn of a ready engine, for a read-out of its model over its data: the problem is made
// final.  sigma_of: the public call that divides a residual by sigma, which MHX_LIK_EXPR has none of.
static int fn_check(mhx_engine* e, int fn, const char* sigma_of = nullptr) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  int rc = use_device(e);
  if (rc != MHX_OK || (rc = finalize_problem(e)) != MHX_OK) return rc;
  if (fn < 0 || fn >= e->P.K) return fail(MHX_EINVAL, "function %d out of range", fn);
  if (sigma_of && e->P.fn[fn].lik == MHX_LIK_EXPR)
    return fail(MHX_EUNSUPPORTED, "%s with MHX_LIK_EXPR (function %d): an expression likelihood's `error` "
                                  "need not be a sigma to divide a residual by", sigma_of, fn);
  if (e->P.fn[fn].n < 1) return fail(MHX_EINVAL, "function %d has no data points", fn);
  return MHX_OK;
}
// the model read-out kernel of A's type: the ahead-of-time spec's, or the run-time compiled program's
template <class Args>
static hipError_t launch_model(mhx_engine* e, const Args& A) {
  return e->spec == SPEC_USER ? rtc_launch_model(*e->user_prog, e->stream, e->dP.p, e->S, A)
                              : launch_model(e->spec, e->stream, e->dP.p, e->S, A);
}
static int fill_pcts(PctList* pc, const int32_t* num, const int32_t* den, int n_pct) {
  if (n_pct < 0 || n_pct > MHX_MAX_PERCENTILES)
    return fail(MHX_EINVAL, "n_pct must be in [0,%d]", MHX_MAX_PERCENTILES);
  if (n_pct > 0 && (!num || !den)) return fail(MHX_EINVAL, "NULL percentile list");
  pc->n = n_pct;
  for (int k = 0; k < n_pct; ++k) {
    if (den[k] < 1 || num[k] < 0 || (int64_t)num[k] > (int64_t)100 * den[k])
      return fail(MHX_EINVAL, "percentile %d: %d/%d is outside [0, 100]", k, num[k], den[k]);
    pc->num[k] = num[k];
    pc->den[k] = den[k];
  }
  return MHX_OK;
}

// The cursor of call c on engine e: the call's own where it has one (c.cursor(e): a read-out whose
// chunk of points depends on its arguments), else portion_cursor's over c.items and c.points.
template <class Q>
static auto cursor_for(const Q& c, const mhx_engine* e, int) -> decltype(c.cursor(e)) {
  return c.cursor(e);
}
template <class Q>
static PortionCursor cursor_for(const Q& c, const mhx_engine* e, long) {
  return portion_cursor(c.items(e), c.points(),
                        [&](Carver& cv, int64_t n, int64_t m) { c.carve(e, cv, n, m); });
}

// Call q on every engine of engs, engine i's results landing at item first[i] of the caller's
// arrays (first NULL: one engine, item 0).  Round by round, every engine's portion is enqueued
// before any is waited for; summary_ms gathers the kernels' time over the portions.
template <class Q>
static int run_portions(const std::vector<mhx_engine*>& engs, const int64_t* first, const Q& q) {
  const size_t E = engs.size();
  std::vector<Q> calls(E, q);
  int rc = MHX_OK;
  for (size_t i = 0; i < E; ++i)
    if ((rc = calls[i].check(engs[i])) != MHX_OK) return rc;
  std::vector<PortionCursor> at(E);
  for (size_t i = 0; i < E; ++i) {
    mhx_engine* e = engs[i];
    Q& c = calls[i];
    for (HostDst& h : c.dst)
      if (h.p && first) h.p = h.at(first[i]);
    e->summary_ms = 0.0;
    at[i] = cursor_for(c, e, 0);
  }
  auto give_up = [&](int code) {
    for (mhx_engine* e : engs) drain(e);
    return code;
  };
  // The stage buffer is sized once per engine, for the call's largest portion - its first, in
  // items and in points - and before the first launch: no piece moves while the call runs, so
  // what one chunk of points leaves in the buffer (the fit's selection and status) is there for
  // the next, and every carve() below sees the final e->stage.p.
  for (size_t i = 0; i < E; ++i) {
    if (at[i].done()) continue;
    const Portion p = at[i].now();
    Carver cv;
    calls[i].carve(engs[i], cv, p.n, p.m);
    if ((rc = use_device(engs[i])) != MHX_OK || (rc = ensure_stage(engs[i], cv.bytes())) != MHX_OK)
      return give_up(rc);
  }
  auto enqueue = [&](mhx_engine* e, const Q& c, const Portion& p) {
    int r = use_device(e);
    if (r != MHX_OK || (r = c.upload(e, p)) != MHX_OK) return r;
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    if ((r = c.launch(e, p)) != MHX_OK) return r;
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    return (int)MHX_OK;
  };
  auto collect = [&](mhx_engine* e, const Q& c, const Portion& p) {
    const int r = use_device(e);
    if (r != MHX_OK) return r;
    HIP_TRY(hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->summary_ms += (double)ms;
    return c.collect(e, p);
  };
  for (;;) {
    bool any = false;
    for (size_t i = 0; i < E; ++i) {
      if (at[i].done()) continue;
      any = true;
      if ((rc = enqueue(engs[i], calls[i], at[i].now())) != MHX_OK) return give_up(rc);
    }
    if (!any) return MHX_OK;
    for (size_t i = 0; i < E; ++i) {
      if (at[i].done()) continue;
      if ((rc = collect(engs[i], calls[i], at[i].now())) != MHX_OK) return give_up(rc);
      at[i].advance();
    }
  }
}
template <class Q>
static int run_portions(mhx_engine* e, const Q& q) {
  return run_portions({e}, nullptr, q);
}
}  // extern "C++"

// ---- walker-set-get: every chain's summary in one launch (k_percentiles, k_covariances,
// k_l_matrices, k_window_best).  Results and scratch (an index list of `take` ints and up to two
// d x d matrices per chain) are a portion's pieces.
struct SummaryCall {
  int kind = 0, take = 0;
  PctList pc{};
  SummaryShape y{};
  HostDst dst[4];  // of the pieces dv[0], dv[1], iv[0], iv[1]; NULL where a piece is no result

  SummaryCall(int kind_, int take_, double* d0, double* d1, int32_t* i0, int32_t* i1)
      : kind(kind_), take(take_) {
    dst[0].p = d0, dst[1].p = d1, dst[2].p = i0, dst[3].p = i1;
  }
  int check(mhx_engine* e) {
    const int rc = window_check(e, take);
    if (rc != MHX_OK) return rc;
    y = summary_shape(kind, e->P.d, pc.n, take);
    for (int k = 0; k < 2; ++k) {
      dst[k].item_bytes = y.nd[k] * sizeof(double);
      dst[2 + k].item_bytes = sizeof(int32_t);
    }
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  SummaryPieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_summary(c, y, n);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    carve(e, c, p.n, p.m);
    // (the factor kernel leaves what it does not reach untouched, as k_l_matrix does: zeros)
    HIP_TRY(hipMemsetAsync(e->stage.p, 0, c.bytes(), e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const SummaryPieces s = carve(e, c, p.n, p.m);
    double* const dv[2] = {stage_at<double>(e, s.dv[0]), stage_at<double>(e, s.dv[1])};
    int32_t* const iv[2] = {stage_at<int32_t>(e, s.iv[0]), stage_at<int32_t>(e, s.iv[1])};
    int32_t* const scratch = stage_at<int32_t>(e, s.scratch);
    switch (kind) {
      case SUM_PERCENTILES: {
        const bool lds = !e->knobs.summary_no_lds && pct_lds_bytes(take, e->P.d) <= kPctLdsBudget;
        HIP_TRY(launch_percentiles(e->stream, e->S, p.i0, p.n, take, pc, lds, dv[0], iv[0]));
        break;
      }
      case SUM_COVARIANCES:
        HIP_TRY(launch_covariances(e->stream, e->S, p.i0, p.n, take, scratch, dv[0], iv[0], iv[1]));
        break;
      case SUM_FACTORS:
        HIP_TRY(launch_l_matrices(e->stream, e->S, p.i0, p.n, take, scratch, dv[1], dv[0], iv[0], iv[1]));
        break;
      default:
        HIP_TRY(launch_window_best(e->stream, e->S, p.i0, p.n, take, dv[0], dv[1]));
        break;
    }
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const SummaryPieces s = carve(e, c, p.n, p.m);
    return copy_back_each(e, dst, p, {s.dv[0], s.dv[1], s.iv[0], s.iv[1]});
  }
};

int mhx_percentile_rank(int64_t len, int32_t num, int32_t den, int64_t* pos, int32_t* between) {
  if (len < 1) return fail(MHX_EINVAL, "len must be >= 1");
  if (den < 1 || num < 0 || (int64_t)num > (int64_t)100 * den)
    return fail(MHX_EINVAL, "the percentile %d/%d is outside [0, 100]", num, den);
  int64_t p = 0;
  int32_t b = 0;
  percentile_rank_of(len, num, den, &p, &b);
  if (pos) *pos = p;
  if (between) *between = b;
  return MHX_OK;
}

int mhx_get_percentiles(mhx_engine* e, int take, const int32_t* pct_num, const int32_t* pct_den,
                        int n_pct, double* out, int32_t* n_used) {
  SummaryCall q(SUM_PERCENTILES, take, out, nullptr, n_used, nullptr);
  int rc = window_check(e, take);
  if (rc != MHX_OK || (rc = fill_pcts(&q.pc, pct_num, pct_den, n_pct)) != MHX_OK) return rc;
  if (n_pct == 0) return MHX_OK;
  return run_portions(e, q);
}
int mhx_get_covariances(mhx_engine* e, int take, double* cov, int32_t* n_unique, int32_t* status) {
  return run_portions(e, SummaryCall(SUM_COVARIANCES, take, cov, nullptr, n_unique, status));
}
int mhx_get_proposal_factors(mhx_engine* e, int take, double* L, int32_t* status,
                             int32_t* n_forward) {
  return run_portions(e, SummaryCall(SUM_FACTORS, take, L, nullptr, status, n_forward));
}
int mhx_get_window_best(mhx_engine* e, int take, double* prob, double* theta) {
  return run_portions(e, SummaryCall(SUM_BEST, take, prob, theta, nullptr, nullptr));
}
int mhx_get_history_capacity(mhx_engine* e, int32_t* capacity) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (capacity) *capacity = e->S.R;
  return MHX_OK;
}
int mhx_get_summary_timing(mhx_engine* e, double* kernel_ms) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (kernel_ms) *kernel_ms = e->summary_ms;
  return MHX_OK;
}

// ---- batched traces: every chain's steps, filtered and thinned on the device (k_traces).  A
// portion's pieces: the column list, the rows and their envelopes, the three counts, and the list
// of kept ring slots (`take` ints per chain).
extern "C++" {
// rows `thin` (M:149-157) leaves of a list of n_kept: the items start, start + stride, ...
static int64_t trace_rows_of(int64_t n_kept, int64_t stride, int64_t start) {
  return n_kept <= start ? 0 : (n_kept - start + stride - 1) / stride;
}
}  // extern "C++"
struct TraceCall {
  int take = 0, filter = 0, stride = 0, start = 0, n_cols = 0, max_out = 0;
  bool cols_null = false, envelope = false;
  std::vector<int32_t> cols;
  enum { VALUES, LO, HI, N_OUT, N_KEPT, N_USED };
  HostDst dst[6];

  TraceCall(int take_, int filter_, int stride_, int start_, const int32_t* cols_, int n_cols_, int max_out_,
            double* values, double* lo, double* hi, int32_t* n_out, int32_t* n_kept, int32_t* n_used)
      : take(take_), filter(filter_), stride(stride_), start(start_), n_cols(n_cols_), max_out(max_out_),
        cols_null(!cols_), envelope(lo || hi) {
    if (cols_ && n_cols >= 1) cols.assign(cols_, cols_ + n_cols);
    dst[VALUES].p = values, dst[LO].p = lo, dst[HI].p = hi;
    dst[N_OUT].p = n_out, dst[N_KEPT].p = n_kept, dst[N_USED].p = n_used;
  }
  int check(mhx_engine* e) {
    const int rc = window_check(e, take);
    if (rc != MHX_OK) return rc;
    const int R = e->S.R, d = e->P.d;
    if (filter != MHX_TRACE_STEPS && filter != MHX_TRACE_UNIQUE && filter != MHX_TRACE_FORWARD)
      return fail(MHX_EINVAL, "filter must be MHX_TRACE_STEPS, _UNIQUE or _FORWARD, not %d", filter);
    if (stride < 1 || stride > R) return fail(MHX_EINVAL, "stride must be in [1, history_capacity = %d]", R);
    if (start < 0 || start >= stride) return fail(MHX_EINVAL, "start must be in [0, stride = %d)", stride);
    if (n_cols < 1) return fail(MHX_EINVAL, "n_cols must be >= 1");
    if (cols_null) return fail(MHX_EINVAL, "cols is NULL");
    for (int j = 0; j < n_cols; ++j)
      if (cols[j] < MHX_TRACE_PROB || cols[j] >= d)
        return fail(MHX_EINVAL, "cols[%d] = %d outside [-1,%d)", j, cols[j], d);
    if (max_out < 1 || max_out > R) return fail(MHX_EINVAL, "max_out must be in [1, history_capacity = %d]", R);
    if (!one_item_fits([&](Carver& c, int64_t n) { carve(e, c, n, 1); }))
      return fail(MHX_EINVAL, "the pieces of ONE chain exceed the stage budget of %zu bytes", kStageBudget);
    const size_t row = (size_t)max_out * (size_t)n_cols * sizeof(double);
    dst[VALUES].item_bytes = dst[LO].item_bytes = dst[HI].item_bytes = row;
    dst[N_OUT].item_bytes = dst[N_KEPT].item_bytes = dst[N_USED].item_bytes = sizeof(int32_t);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  TracePieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_traces(c, n_cols, max_out, take, envelope ? 1 : 0, n);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const TracePieces s = carve(e, c, p.n, p.m);
    // the outputs, which lie together: rows from n_out on stay all-bits-zero
    HIP_TRY(hipMemsetAsync(e->stage.p + s.values, 0, s.kept - s.values, e->stream));
    HIP_TRY(hipMemcpyAsync(e->stage.p + s.cols, cols.data(), cols.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                           e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const TracePieces s = carve(e, c, p.n, p.m);
    HIP_TRY(launch_traces(e->stream, e->S, p.i0, p.n, take, filter, stride, start, n_cols, max_out,
                          stage_at<int32_t>(e, s.cols), stage_at<int32_t>(e, s.kept), stage_at<double>(e, s.values),
                          dst[LO].p ? stage_at<double>(e, s.lo) : nullptr,
                          dst[HI].p ? stage_at<double>(e, s.hi) : nullptr, stage_at<int32_t>(e, s.n_out),
                          stage_at<int32_t>(e, s.n_kept), stage_at<int32_t>(e, s.n_used)));
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const TracePieces s = carve(e, c, p.n, p.m);
    const size_t off[6] = {s.values, s.lo, s.hi, s.n_out, s.n_kept, s.n_used};
    for (int k = 0; k < 6; ++k) {
      const int rc = copy_back(dst[k], p.i0, p.n, e->stage.p + off[k]);
      if (rc != MHX_OK) return rc;
    }
    return MHX_OK;
  }
};

int mhx_trace_rows(int64_t n_kept, int32_t stride, int32_t start, int64_t* rows) {
  if (n_kept < 0) return fail(MHX_EINVAL, "n_kept must be >= 0");
  if (stride < 1) return fail(MHX_EINVAL, "stride must be >= 1");
  if (start < 0 || start >= stride) return fail(MHX_EINVAL, "start must be in [0, stride = %d)", stride);
  if (rows) *rows = trace_rows_of(n_kept, stride, start);
  return MHX_OK;
}
int mhx_get_traces(mhx_engine* e, int take, int filter, int stride, int start, const int32_t* cols, int n_cols,
                   int max_out, double* values, double* lo, double* hi, int32_t* n_out, int32_t* n_kept,
                   int32_t* n_used) {
  return run_portions(e, TraceCall(take, filter, stride, start, cols, n_cols, max_out, values, lo, hi, n_out,
                                   n_kept, n_used));
}

// ---- walker-get-data-and-fit (M:1230-1255): model values and credible bands on the device
// (k_band_select, k_fit).  An ITEM is a parameter vector (mhx_eval_function) or a chain
// (mhx_get_fit_bands).  Items and points are worked through in portions: at most
// kFitChunkPoints points of x at a time, and as many items as keep the pieces - x, the
// parameter vectors or the selected steps' slots, the results - below kStageBudget.
struct FitCall {
  int fn = 0, take = 0;  // take 0: parameter vectors, else bands of the engine's chains
  int64_t n = 0, m = 0;  // (n < 0: bands, whatever take is: check)
  const double* theta = nullptr;  // [n][d] on the host (parameter vectors)
  const double* xcols = nullptr;  // [n_cols][m] on the host, or NULL: the function's dataset
  int n_cols = 1;
  enum { YMAX, YMIN, N_SEL, STATUS };
  HostDst dst[4];

  FitCall(int fn_, int take_, int64_t n_, const double* theta_, const double* xcols_, int n_cols_,
          int64_t m_, double* ymax, double* ymin, int32_t* n_sel, int32_t* status)
      : fn(fn_), take(take_), n(n_), m(m_), theta(theta_), xcols(xcols_), n_cols(n_cols_) {
    const size_t row = (size_t)std::max<int64_t>(m, 0) * sizeof(double);
    dst[YMAX] = {ymax, row}, dst[YMIN] = {ymin, row};
    dst[N_SEL] = {n_sel, sizeof(int32_t)}, dst[STATUS] = {status, sizeof(int32_t)};
  }
  // x columns the model of function fn reads
  static int fn_cols(const mhx_engine* e, int fn) {
    return e->P.fn[fn].model == MHX_MODEL_EXPR ? std::max(1, e->fn_expr[fn].xcols) : 1;
  }
  int check(mhx_engine* e) {
    if (!e) return fail(MHX_EINVAL, "engine is NULL");
    int rc = take != 0 || n < 0 ? window_check(e, take) : MHX_OK;
    if (rc != MHX_OK || (rc = use_device(e)) != MHX_OK || (rc = finalize_problem(e)) != MHX_OK) return rc;
    if (fn < 0 || fn >= e->P.K) return fail(MHX_EINVAL, "function %d out of range", fn);
    if (n_cols != fn_cols(e, fn))
      return fail(MHX_EINVAL, "function %d reads %d column(s) of x, n_cols is %d", fn, fn_cols(e, fn), n_cols);
    if (!xcols && m != e->P.fn[fn].n)
      return fail(MHX_EINVAL, "xcols is NULL: m must be the dataset's %lld points", (long long)e->P.fn[fn].n);
    if (m < 1) return fail(MHX_EINVAL, "m must be >= 1");
    if (take == 0 && n > 0 && !theta) return fail(MHX_EINVAL, "theta is NULL");
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return take > 0 ? e->cfg.n_chains : n; }
  int64_t points() const { return m; }
  FitPieces carve(const mhx_engine* e, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_fit(c, e->P.d, take, n_items, m_points);
  }
  // items [i0, i0 + n) at points [m0, m0 + m).  What depends on the items alone is done on the
  // portion's first chunk of points: the status gathers over the chunks
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const FitPieces s = carve(e, c, p.n, p.m);
    const size_t mb = (size_t)p.m * sizeof(double);
    if (xcols) {
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.x0), xcols + p.m0, mb, hipMemcpyHostToDevice, e->stream));
      if (n_cols > 1)
        HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.x1), xcols + m + p.m0, mb, hipMemcpyHostToDevice, e->stream));
    }
    if (p.m0 != 0) return MHX_OK;
    if (take > 0)
      HIP_TRY(hipMemsetAsync(stage_at<int32_t>(e, s.status), 0, (size_t)p.n * sizeof(int32_t), e->stream));
    else
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.theta), theta + (size_t)p.i0 * e->P.d,
                             (size_t)p.n * e->P.d * sizeof(double), hipMemcpyHostToDevice, e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const FitPieces s = carve(e, c, p.n, p.m);
    const FnDesc& f = e->P.fn[fn];
    FitArgs A{};
    A.fn = fn;
    A.n = p.n;
    A.m = p.m;
    A.n_chunks = fit_chunks(p.m);
    if (xcols) {
      A.x0 = stage_at<double>(e, s.x0);
      A.x1 = n_cols > 1 ? stage_at<double>(e, s.x1) : nullptr;
    } else {
      A.x0 = f.x + p.m0;
      A.x1 = f.n_xcols > 1 ? f.c + p.m0 : nullptr;
    }
    A.ymax = stage_at<double>(e, s.ymax);
    if (take > 0) {
      int32_t *const sel = stage_at<int32_t>(e, s.sel), *const n_sel = stage_at<int32_t>(e, s.n_sel);
      A.theta = e->S.hist_theta;
      A.sel = sel;
      A.n_sel = n_sel;
      A.sel_pitch = take;
      A.rows_per_item = e->S.R;
      A.row0 = p.i0 * e->S.R;
      A.ymin = stage_at<double>(e, s.ymin);
      A.status = stage_at<int32_t>(e, s.status);
      if (p.m0 == 0) HIP_TRY(launch_band_select(e->stream, e->S, p.i0, p.n, take, sel, n_sel));
    } else {
      A.theta = stage_at<double>(e, s.theta);
      A.rows_per_item = 1;
    }
    HIP_TRY(launch_model(e, A));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const FitPieces s = carve(e, c, p.n, p.m);
    const size_t dv[2] = {s.ymax, s.ymin};
    for (int k = 0; k < (take > 0 ? 2 : 1); ++k) {
      const int rc = copy_back_points(dst[k], p, m, sizeof(double), 1, e->stage.p + dv[k]);
      if (rc != MHX_OK) return rc;
    }
    if (take == 0 || p.m0 + p.m < m) return MHX_OK;  // (the status gathers over the chunks of points)
    return copy_back_each(e, dst + N_SEL, p, {s.n_sel, s.status});
  }
};

int mhx_band_count(int64_t take, int64_t* k) {
  if (take < 1) return fail(MHX_EINVAL, "take must be >= 1");
  if (k) *k = band_count_of(take);
  return MHX_OK;
}
int mhx_eval_function(mhx_engine* e, int fn, const double* theta, int64_t n, const double* xcols,
                      int n_cols, int64_t m, double* out) {
  if (n < 0) return fail(MHX_EINVAL, "n < 0");
  return run_portions(e, FitCall(fn, 0, n, theta, xcols, n_cols, m, out, nullptr, nullptr, nullptr));
}
int mhx_get_fit_bands(mhx_engine* e, int fn, int take, const double* xcols, int n_cols, int64_t m,
                      double* ymax, double* ymin, int32_t* n_selected, int32_t* status) {
  return run_portions(e, FitCall(fn, take, -1, nullptr, xcols, n_cols, m, ymax, ymin, n_selected, status));
}

// ---- what mhx_get_waic and mhx_get_loo share: both read the ENGINE's own data of function fn,
// whose per-point constants are on the device (the normal forms' c array), on the host
// (Dataset::hconst, uploaded into the portion's stage piece `cst`) or none (MHX_LIK_EXPR).
static int refuse_planes(const mhx_engine* e, const char* who) {
  for (int k = 0; k < e->P.K; ++k)
    if (e->data[k].planes)
      return fail(MHX_EUNSUPPORTED, "%s on an engine with a dataset per walker "
                                    "(mhx_set_dataset_planes): the planes' per-point constants "
                                    "live per walker and are not on the device", who);
  return MHX_OK;
}
// the chunk's constants, where the host holds them; the status gathers over the chunks of points
static int upload_own_data(mhx_engine* e, int fn, const Portion& p, size_t cst, size_t status) {
  const Dataset& D = e->data[fn];
  if (!D.hconst.empty())
    HIP_TRY(hipMemcpyAsync(stage_at<double>(e, cst), D.hconst.data() + p.m0, (size_t)p.m * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
  if (p.m0 == 0)
    HIP_TRY(hipMemsetAsync(stage_at<int32_t>(e, status), 0, (size_t)p.n * sizeof(int32_t), e->stream));
  return MHX_OK;
}
extern "C++" {
template <class Args>  // WaicArgs, LooArgs: x0, x1, y, w, c of the chunk
static void set_own_data(const mhx_engine* e, int fn, const Portion& p, size_t cst, Args& A) {
  const FnDesc& f = e->P.fn[fn];
  const DataView v = data_view(f, nullptr, p.m0);
  A.x0 = v.x0, A.x1 = v.x1, A.y = v.y, A.w = v.w;
  A.c = !e->data[fn].hconst.empty() ? stage_at<double>(e, cst) : f.lik == MHX_LIK_EXPR ? nullptr : f.c + p.m0;
}
}  // extern "C++"

// ---- WAIC (include/mhx.h has the definition): every chain's pointwise log-sum-exp and Welford
// moments of the log-likelihood terms of function fn over its window (k_waic), and their totals
// (k_waic_totals).  An item is a chain; the function's points go in chunks of kFitChunkPoints, a
// whole number of MHX_WAIC_BLOCK blocks, so a block is the same points whatever the split.  The
// blocks' partial sums of all chunks stay in the stage; the totals are taken on the last chunk.
struct WaicCall {
  int fn = 0, take = 0, want = 0;
  int64_t m = 0, nb_total = 0;
  enum { ELPD, LPPD, P_WAIC, N_HIGH, N_USED, STATUS, PW_LPPD, PW_P, PW_ACC, N_DST };
  HostDst dst[N_DST];
  static_assert(kFitChunkPoints % MHX_WAIC_BLOCK == 0, "a chunk of points is whole blocks");

  WaicCall(int fn_, int take_, double* elpd, double* lppd, double* p_waic, int32_t* n_high,
           double* pw_lppd, double* pw_p, double* pw_acc, int32_t* n_used, int32_t* status)
      : fn(fn_), take(take_) {
    dst[ELPD] = {elpd, sizeof(double)}, dst[LPPD] = {lppd, sizeof(double)};
    dst[P_WAIC] = {p_waic, sizeof(double)}, dst[N_HIGH] = {n_high, sizeof(int32_t)};
    dst[N_USED] = {n_used, sizeof(int32_t)}, dst[STATUS] = {status, sizeof(int32_t)};
    dst[PW_LPPD].p = pw_lppd, dst[PW_P].p = pw_p, dst[PW_ACC].p = pw_acc;
    want = (pw_lppd ? WAIC_WANT_LPPD : 0) | (pw_p ? WAIC_WANT_P : 0) | (pw_acc ? WAIC_WANT_ACC : 0);
  }
  int check(mhx_engine* e) {
    int rc = window_check(e, take);
    if (rc != MHX_OK || (rc = fn_check(e, fn)) != MHX_OK) return rc;
    if ((rc = refuse_planes(e, "mhx_get_waic")) != MHX_OK) return rc;
    m = e->P.fn[fn].n;
    nb_total = waic_blocks(m);
    dst[PW_LPPD].item_bytes = dst[PW_P].item_bytes = (size_t)m * sizeof(double);
    dst[PW_ACC].item_bytes = (size_t)m * 4 * sizeof(double);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return m; }
  WaicPieces carve(const mhx_engine*, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_waic(c, nb_total, want, n_items, m_points);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const WaicPieces s = carve(e, c, p.n, p.m);
    return upload_own_data(e, fn, p, s.cst, s.status);
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const WaicPieces s = carve(e, c, p.n, p.m);
    WaicArgs A{};
    A.c0 = p.i0, A.n = p.n;
    A.take = take, A.fn = fn;
    A.n_blocks = (int32_t)waic_blocks(p.m);
    A.blk0 = p.m0 / MHX_WAIC_BLOCK, A.nb_total = nb_total, A.m = p.m;
    set_own_data(e, fn, p, s.cst, A);
    A.pw_lppd = (want & WAIC_WANT_LPPD) ? stage_at<double>(e, s.pw_lppd) : nullptr;
    A.pw_p = (want & WAIC_WANT_P) ? stage_at<double>(e, s.pw_p) : nullptr;
    A.pw_acc = (want & WAIC_WANT_ACC) ? stage_at<double>(e, s.pw_acc) : nullptr;
    A.part_lppd = stage_at<double>(e, s.part_lppd);
    A.part_p = stage_at<double>(e, s.part_p);
    A.part_high = stage_at<int32_t>(e, s.part_high);
    A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_model(e, A));
    if (p.m0 + p.m >= m)
      HIP_TRY(launch_waic_totals(e->stream, e->S, p.i0, p.n, take, nb_total, A.part_lppd, A.part_p, A.part_high,
                                 stage_at<double>(e, s.elpd), stage_at<double>(e, s.lppd),
                                 stage_at<double>(e, s.p_waic), stage_at<int32_t>(e, s.n_high),
                                 stage_at<int32_t>(e, s.n_used), A.status));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const WaicPieces s = carve(e, c, p.n, p.m);
    const size_t pw[3] = {s.pw_lppd, s.pw_p, s.pw_acc};
    for (int k = 0; k < 3; ++k) {  // (pw_acc: four doubles a point)
      const size_t per = (k == 2 ? 4 : 1) * sizeof(double);
      const int rc = copy_back_points(dst[PW_LPPD + k], p, m, per, 1, e->stage.p + pw[k]);
      if (rc != MHX_OK) return rc;
    }
    if (p.m0 + p.m < m) return MHX_OK;  // (the totals come with the last chunk of points)
    return copy_back_each(e, dst, p, {s.elpd, s.lppd, s.p_waic, s.n_high, s.n_used, s.status});
  }
};

int mhx_get_waic(mhx_engine* e, int fn, int take, double* elpd, double* lppd, double* p_waic,
                 int32_t* n_high, double* pw_lppd, double* pw_p, double* pw_acc, int32_t* n_used,
                 int32_t* status) {
  return run_portions(e, WaicCall(fn, take, elpd, lppd, p_waic, n_high, pw_lppd, pw_p, pw_acc, n_used, status));
}

// ---- held-out predictive density (include/mhx.h has the definition): WAIC's log-sum-exp over the
// window, of the terms of data the CALLER hands in, with the value moments beside it (k_heldout),
// and the totals (k_heldout_totals).  An item is a chain; the caller's points go in chunks of
// kFitChunkPoints, whole blocks, as WAIC's do, and the blocks' partial sums of all chunks stay in
// the stage.  The caller's arrays are turned into the kernel's ys, w, c and use bytes on the host
// (mhx_heldout.hpp) and uploaded per portion: what all chains share once per chunk of points, the
// rest [items][chunk].  Nothing of the engine's datasets is read, so a dataset per walker is served.
struct HeldoutCall {
  int fn = 0, take = 0, want = 0, n_cols = 1, lik = 0;
  bool logfact_double = false;
  int64_t m = 0, nb_total = 0;
  const double* xcols = nullptr;
  HeldoutLayout lay{};
  int y_per_chain = 0, sigma_kind = 0, use_per_chain = 0;
  // (Y, SIGMA, USE are read, not written: they lie here to move with a group's chains)
  enum { LPD, N_SCORED, N_USED, STATUS, PW_LPD, PW_ACC, Y, SIGMA, USE, N_DST };
  HostDst dst[N_DST];
  // a portion's prepared arrays: they must outlive its copies, which collect() has waited for
  // before the next upload() refills them
  mutable std::vector<double> h_ys, h_w, h_c;
  mutable std::vector<uint8_t> h_use;
  mutable std::vector<float> lf_cache;
  static_assert(kFitChunkPoints % MHX_HELDOUT_BLOCK == 0, "a chunk of points is whole blocks");

  HeldoutCall(int fn_, int take_, const double* xcols_, int n_cols_, int64_t m_, const double* y, int y_per_chain_,
              const double* sigma, int sigma_kind_, const uint8_t* use, int use_per_chain_, double* lpd,
              int32_t* n_scored, double* pw_lpd, double* pw_acc, int32_t* n_used, int32_t* status)
      : fn(fn_), take(take_), n_cols(n_cols_), m(m_), xcols(xcols_), y_per_chain(y_per_chain_ != 0),
        sigma_kind(sigma_kind_), use_per_chain(use_per_chain_ != 0) {
    const size_t row = (size_t)std::max<int64_t>(m, 0);
    dst[LPD] = {lpd, sizeof(double)}, dst[N_SCORED] = {n_scored, sizeof(int32_t)};
    dst[N_USED] = {n_used, sizeof(int32_t)}, dst[STATUS] = {status, sizeof(int32_t)};
    dst[PW_LPD] = {pw_lpd, row * sizeof(double)}, dst[PW_ACC] = {pw_acc, row * 4 * sizeof(double)};
    dst[Y] = {const_cast<double*>(y), y_per_chain ? row * sizeof(double) : 0};
    dst[SIGMA] = {const_cast<double*>(sigma), sigma_kind == MHX_SIGMA_PER_CHAIN   ? sizeof(double)
                                              : sigma_kind == MHX_SIGMA_PER_POINT ? row * sizeof(double)
                                                                                  : 0};
    dst[USE] = {const_cast<uint8_t*>(use), use_per_chain ? row : 0};
    want = (pw_lpd ? HELDOUT_WANT_LPD : 0) | (pw_acc ? HELDOUT_WANT_ACC : 0);
  }
  // What does not depend on which engine of a group serves a chain: the arguments, and the caller's
  // data over all n_total chains as mhx_set_dataset would check them.  e0: any engine of the call.
  int check_data(const mhx_engine* e0, int64_t n_total) {
    if (!e0) return fail(MHX_EINVAL, "engine is NULL");
    if (fn < 0 || fn >= e0->P.K) return fail(MHX_EINVAL, "function %d out of range", fn);
    if (m < 1) return fail(MHX_EINVAL, "m must be >= 1");
    if (!xcols || !dst[Y].p) return fail(MHX_EINVAL, "mhx_get_heldout: xcols / y is NULL");
    if (sigma_kind < MHX_SIGMA_NONE || sigma_kind > MHX_SIGMA_PER_POINT ||
        (sigma_kind != MHX_SIGMA_NONE) != (dst[SIGMA].p != nullptr))
      return fail(MHX_EINVAL, "mhx_get_heldout: sigma_kind %d does not go with a%s sigma", sigma_kind,
                  dst[SIGMA].p ? "" : " NULL");
    lik = e0->P.fn[fn].lik;
    logfact_double = e0->cfg.poisson_logfact_double != 0;
    char msg[160];
    if (heldout_validate(lik, static_cast<const double*>(dst[Y].p), y_per_chain,
                         static_cast<const double*>(dst[SIGMA].p), sigma_kind, n_total, m, msg, sizeof msg) != 0)
      return fail(MHX_EINVAL, "%s", msg);
    lay = heldout_layout(lik, y_per_chain, sigma_kind, dst[USE].p != nullptr, use_per_chain);
    nb_total = waic_blocks(m);
    return MHX_OK;
  }
  int check(mhx_engine* e) {
    int rc = window_check(e, take);
    if (rc != MHX_OK || (rc = fn_check(e, fn)) != MHX_OK) return rc;
    if (n_cols != FitCall::fn_cols(e, fn))
      return fail(MHX_EINVAL, "function %d reads %d column(s) of x, n_cols is %d", fn, FitCall::fn_cols(e, fn),
                  n_cols);
    if (e->P.fn[fn].lik != lik)
      return fail(MHX_EINVAL, "function %d: the engines of the group differ in its likelihood", fn);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return m; }
  HeldoutPieces carve(const mhx_engine*, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_heldout(c, nb_total, want, lay, n_items, m_points);
  }
  HeldoutData data() const {
    HeldoutData D;
    D.y = static_cast<const double*>(dst[Y].p), D.sigma = static_cast<const double*>(dst[SIGMA].p);
    D.use = static_cast<const uint8_t*>(dst[USE].p);
    D.y_per_chain = y_per_chain, D.sigma_kind = sigma_kind, D.use_per_chain = use_per_chain;
    D.m = m;
    return D;
  }
  // chains [i0, i0 + n) at points [m0, m0 + m): x and the prepared arrays of the chunk
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HeldoutPieces s = carve(e, c, p.n, p.m);
    const size_t mb = (size_t)p.m * sizeof(double);
    HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.x0), xcols + p.m0, mb, hipMemcpyHostToDevice, e->stream));
    if (n_cols > 1)
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.x1), xcols + m + p.m0, mb, hipMemcpyHostToDevice, e->stream));
    h_ys.resize(heldout_elems(lay.ys, p.n, p.m)), h_w.resize(heldout_elems(lay.w, p.n, p.m));
    h_c.resize(heldout_elems(lay.c, p.n, p.m)), h_use.resize(heldout_elems(lay.use, p.n, p.m));
    heldout_fill(lik, logfact_double, lay, data(), p.i0, p.n, p.m0, p.m, h_ys.data(), h_w.data(), h_c.data(),
                 h_use.data(), lf_cache);
    const struct { size_t at; const void* src; size_t bytes; } up[4] = {
        {s.ys, h_ys.data(), h_ys.size() * sizeof(double)}, {s.w, h_w.data(), h_w.size() * sizeof(double)},
        {s.c, h_c.data(), h_c.size() * sizeof(double)}, {s.use, h_use.data(), h_use.size()}};
    for (const auto& u : up)
      if (u.bytes > 0)
        HIP_TRY(hipMemcpyAsync(e->stage.p + u.at, u.src, u.bytes, hipMemcpyHostToDevice, e->stream));
    if (p.m0 == 0)
      HIP_TRY(hipMemsetAsync(stage_at<int32_t>(e, s.status), 0, (size_t)p.n * sizeof(int32_t), e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HeldoutPieces s = carve(e, c, p.n, p.m);
    HeldoutArgs A{};
    A.c0 = p.i0, A.n = p.n;
    A.take = take, A.fn = fn;
    A.n_blocks = (int32_t)waic_blocks(p.m);
    A.blk0 = p.m0 / MHX_HELDOUT_BLOCK, A.nb_total = nb_total, A.m = p.m;
    A.x0 = stage_at<double>(e, s.x0);
    A.x1 = n_cols > 1 ? stage_at<double>(e, s.x1) : nullptr;
    A.ys = stage_at<double>(e, s.ys), A.y_pitch = heldout_pitch(lay.ys, p.m);
    A.w = stage_at<double>(e, s.w), A.w_pitch = heldout_pitch(lay.w, p.m), A.w_step = heldout_step(lay.w);
    A.c = lay.c == kHoNone ? nullptr : stage_at<double>(e, s.c);
    A.c_pitch = heldout_pitch(lay.c, p.m), A.c_step = heldout_step(lay.c);
    A.use = lay.use == kHoNone ? nullptr : stage_at<unsigned char>(e, s.use);
    A.use_pitch = heldout_pitch(lay.use, p.m);
    A.pw_lpd = (want & HELDOUT_WANT_LPD) ? stage_at<double>(e, s.pw_lpd) : nullptr;
    A.pw_acc = (want & HELDOUT_WANT_ACC) ? stage_at<double>(e, s.pw_acc) : nullptr;
    A.part_lpd = stage_at<double>(e, s.part_lpd);
    A.part_scored = stage_at<int32_t>(e, s.part_scored);
    A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_model(e, A));
    if (p.m0 + p.m >= m)
      HIP_TRY(launch_heldout_totals(e->stream, e->S, p.i0, p.n, take, nb_total, A.part_lpd, A.part_scored,
                                    stage_at<double>(e, s.lpd), stage_at<int32_t>(e, s.n_scored),
                                    stage_at<int32_t>(e, s.n_used), A.status));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HeldoutPieces s = carve(e, c, p.n, p.m);
    int rc = copy_back_points(dst[PW_LPD], p, m, sizeof(double), 1, e->stage.p + s.pw_lpd);
    if (rc != MHX_OK || (rc = copy_back_points(dst[PW_ACC], p, m, 4 * sizeof(double), 1, e->stage.p + s.pw_acc)) != MHX_OK)
      return rc;
    if (p.m0 + p.m < m) return MHX_OK;  // (the totals come with the last chunk of points)
    return copy_back_each(e, dst, p, {s.lpd, s.n_scored, s.n_used, s.status});
  }
};

int mhx_get_heldout(mhx_engine* e, int fn, int take, const double* xcols, int n_cols, int64_t m,
                    const double* y, int y_per_chain, const double* sigma, int sigma_kind,
                    const uint8_t* use, int use_per_chain, double* lpd, int32_t* n_scored,
                    double* pw_lpd, double* pw_acc, int32_t* n_used, int32_t* status) {
  HeldoutCall q(fn, take, xcols, n_cols, m, y, y_per_chain, sigma, sigma_kind, use, use_per_chain, lpd, n_scored,
                pw_lpd, pw_acc, n_used, status);
  int rc = window_check(e, take);
  if (rc != MHX_OK || (rc = q.check_data(e, e->cfg.n_chains)) != MHX_OK) return rc;
  return run_portions(e, q);
}

// ---- PSIS-LOO (include/mhx.h has the definition): every chain's likelihood terms of function fn
// over its window, staged, and pw_lppd (k_loo_values), the Pareto-smoothed estimate of every (chain,
// point) column (the model-free k_loo_fit), the block sums of the chunk (k_loo_block_sums) and the
// totals (k_loo_totals).  An item is a chain.  The terms of a portion are staged, `take` doubles per
// chain and point, so the chunk of points is the call's own (loo_cursor, mhx_stage.hpp): whole
// MHX_LOO_BLOCK blocks, as many as let one chain fit the budget - a block is the same points
// whatever the split.  The blocks' partial sums of all chunks stay in the stage; the totals are
// taken on the last chunk.
struct LooCall {
  int fn = 0, take = 0, tail_len = 0, P = 0, want = 0;
  double k_limit = 0.7;
  int64_t m = 0, nb_total = 0;
  enum { ELPD, P_LOO, LPPD, N_HIGH, N_USED, STATUS, PW_ELPD, PW_KHAT, PW_LPPD, PW_ACC, TAIL, N_DST };
  HostDst dst[N_DST];
  static_assert(kLooBlock == MHX_LOO_BLOCK, "MHX_LOO_BLOCK (include/mhx.h)");

  LooCall(int fn_, int take_, int tail_len_, double k_limit_, double* elpd, double* p_loo, double* lppd,
          int32_t* n_high, int32_t* n_used, int32_t* status, double* pw_elpd, double* pw_khat, double* pw_lppd,
          double* pw_acc, double* tail)
      : fn(fn_), take(take_), tail_len(tail_len_), k_limit(k_limit_) {
    dst[ELPD] = {elpd, sizeof(double)}, dst[P_LOO] = {p_loo, sizeof(double)}, dst[LPPD] = {lppd, sizeof(double)};
    dst[N_HIGH] = {n_high, sizeof(int32_t)}, dst[N_USED] = {n_used, sizeof(int32_t)};
    dst[STATUS] = {status, sizeof(int32_t)};
    dst[PW_ELPD].p = pw_elpd, dst[PW_KHAT].p = pw_khat, dst[PW_LPPD].p = pw_lppd;
    dst[PW_ACC].p = pw_acc, dst[TAIL].p = tail;
    want = (pw_acc ? LOO_WANT_ACC : 0) | (tail ? LOO_WANT_TAIL : 0);
  }
  int check(mhx_engine* e) {
    int rc = window_check(e, take);
    if (rc != MHX_OK || (rc = fn_check(e, fn)) != MHX_OK) return rc;
    if (tail_len < 0 || tail_len > MHX_LOO_MAX_TAIL)
      return fail(MHX_EINVAL, "tail_len must be in [0, MHX_LOO_MAX_TAIL = %d]", MHX_LOO_MAX_TAIL);
    if (k_limit != k_limit) return fail(MHX_EINVAL, "k_limit is a NaN");
    if ((rc = refuse_planes(e, "mhx_get_loo")) != MHX_OK) return rc;
    m = e->P.fn[fn].n;
    nb_total = loo_blocks(m);
    P = loo_tail_length_of(take, tail_len);
    if (cursor(e).chunk < 1)
      return fail(MHX_EUNSUPPORTED, "mhx_get_loo: the %d staged terms of each of a chain's first %lld "
                                    "points do not fit the 64 MiB of a portion: the greatest take that fits is %d",
                  take, (long long)std::min<int64_t>(m, kLooBlock), loo_max_take(m, P, want));
    const size_t row = (size_t)m * sizeof(double);
    dst[PW_ELPD].item_bytes = dst[PW_KHAT].item_bytes = dst[PW_LPPD].item_bytes = row;
    dst[PW_ACC].item_bytes = 4 * row;
    dst[TAIL].item_bytes = (size_t)P * row;
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return m; }
  PortionCursor cursor(const mhx_engine* e) const { return loo_cursor(items(e), m, take, P, want); }
  LooPieces carve(const mhx_engine*, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_loo(c, nb_total, take, P, want, n_items, m_points);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const LooPieces s = carve(e, c, p.n, p.m);
    return upload_own_data(e, fn, p, s.cst, s.status);
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const LooPieces s = carve(e, c, p.n, p.m);
    LooArgs A{};
    A.c0 = p.i0, A.n = p.n;
    A.take = take, A.fn = fn;
    A.n_blocks = (int32_t)loo_value_blocks(p.m);
    A.m = p.m;
    set_own_data(e, fn, p, s.cst, A);
    A.terms = stage_at<double>(e, s.terms);
    A.pw_lppd = stage_at<double>(e, s.pw_lppd);
    A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_model(e, A));
    double* const pw_elpd = stage_at<double>(e, s.pw_elpd);
    double* const pw_khat = stage_at<double>(e, s.pw_khat);
    double* const part_elpd = stage_at<double>(e, s.part_elpd);
    double* const part_lppd = stage_at<double>(e, s.part_lppd);
    int32_t* const part_high = stage_at<int32_t>(e, s.part_high);
    HIP_TRY(launch_loo_fit(e->stream, e->S, p.i0, p.n, take, tail_len, p.m,
                           !e->knobs.loo_no_lds && loo_use_lds(take, P), A.terms, pw_elpd, pw_khat,
                           (want & LOO_WANT_ACC) ? stage_at<double>(e, s.pw_acc) : nullptr,
                           (want & LOO_WANT_TAIL) ? stage_at<double>(e, s.tail) : nullptr, A.status));
    HIP_TRY(launch_loo_block_sums(e->stream, p.n, p.m, p.m0 / MHX_LOO_BLOCK, nb_total, k_limit, pw_elpd,
                                  A.pw_lppd, pw_khat, part_elpd, part_lppd, part_high));
    if (p.m0 + p.m >= m)
      HIP_TRY(launch_loo_totals(e->stream, e->S, p.i0, p.n, take, nb_total, part_elpd, part_lppd, part_high,
                                stage_at<double>(e, s.elpd), stage_at<double>(e, s.p_loo),
                                stage_at<double>(e, s.lppd), stage_at<int32_t>(e, s.n_high),
                                stage_at<int32_t>(e, s.n_used), A.status));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const LooPieces s = carve(e, c, p.n, p.m);
    const size_t pw[5] = {s.pw_elpd, s.pw_khat, s.pw_lppd, s.pw_acc, s.tail};
    const size_t per[5] = {1, 1, 1, 4, (size_t)P};  // (doubles a point)
    for (int k = 0; k < 5; ++k) {
      if (per[k] == 0) continue;
      const int rc = copy_back_points(dst[PW_ELPD + k], p, m, per[k] * sizeof(double), 1, e->stage.p + pw[k]);
      if (rc != MHX_OK) return rc;
    }
    if (p.m0 + p.m < m) return MHX_OK;  // (the totals come with the last chunk of points)
    return copy_back_each(e, dst, p, {s.elpd, s.p_loo, s.lppd, s.n_high, s.n_used, s.status});
  }
};

int mhx_loo_tail_length(int64_t n, int32_t tail_len, int32_t* M) {
  if (n < 0) return fail(MHX_EINVAL, "n < 0");
  if (tail_len < 0 || tail_len > MHX_LOO_MAX_TAIL)
    return fail(MHX_EINVAL, "tail_len must be in [0, MHX_LOO_MAX_TAIL = %d]", MHX_LOO_MAX_TAIL);
  if (M) *M = loo_tail_length_of(n, tail_len);
  return MHX_OK;
}
int mhx_get_loo(mhx_engine* e, int fn, int take, int tail_len, double k_limit, double* elpd_loo, double* p_loo,
                double* lppd, int32_t* n_high, int32_t* n_used, int32_t* status, double* pw_elpd,
                double* pw_khat, double* pw_lppd, double* pw_acc, double* tail) {
  return run_portions(e, LooCall(fn, take, tail_len, k_limit, elpd_loo, p_loo, lppd, n_high, n_used, status,
                                 pw_elpd, pw_khat, pw_lppd, pw_acc, tail));
}

// ---- residuals (include/mhx.h has the definition): function fn at one parameter vector per chain
// over the chain's own data, and the block partials of the standardized residuals (k_resid), then
// their totals (k_resid_totals).  An item is a chain; the function's points go in chunks of
// kFitChunkPoints, a whole number of MHX_RESID_BLOCK blocks, so a block is the same points whatever
// the split.  The partials of all chunks stay in the stage; the totals are taken on the last chunk.
// The data are read where the engine holds them: the shared arrays, or the planes of a dataset per
// walker (PlaneDesc), through a DataView (data_view, mhx_stage.hpp).
struct ResidCall {
  int fn = 0, want = 0;
  double z_limit = 0.0;
  int64_t m = 0, nb_total = 0;
  enum { CHI2, SUM_Z, DW, MAX_ABS_Z, MAX_INDEX, N_POS, N_RUNS, N_OUT, STATUS, FIT, Z, THETA, N_DST };
  HostDst dst[N_DST];  // (THETA is read, not written: it lies here to move with a group's chains)
  static_assert(kFitChunkPoints % MHX_RESID_BLOCK == 0, "a chunk of points is whole blocks");

  ResidCall(int fn_, const double* theta, double z_limit_, double* fit, double* z, double* chi2,
            double* sum_z, double* dw, double* max_abs_z, int64_t* max_index, int32_t* n_pos,
            int32_t* n_runs, int32_t* n_out, int32_t* status)
      : fn(fn_), z_limit(z_limit_) {
    dst[CHI2] = {chi2, sizeof(double)}, dst[SUM_Z] = {sum_z, sizeof(double)};
    dst[DW] = {dw, sizeof(double)}, dst[MAX_ABS_Z] = {max_abs_z, sizeof(double)};
    dst[MAX_INDEX] = {max_index, sizeof(int64_t)}, dst[N_POS] = {n_pos, sizeof(int32_t)};
    dst[N_RUNS] = {n_runs, sizeof(int32_t)}, dst[N_OUT] = {n_out, sizeof(int32_t)};
    dst[STATUS] = {status, sizeof(int32_t)};
    dst[FIT].p = fit, dst[Z].p = z, dst[THETA].p = const_cast<double*>(theta);
    want = (fit ? RESID_WANT_FIT : 0) | (z ? RESID_WANT_Z : 0);
  }
  int check(mhx_engine* e) {
    const int rc = fn_check(e, fn, "mhx_get_residuals");
    if (rc != MHX_OK) return rc;
    if (z_limit != z_limit) return fail(MHX_EINVAL, "z_limit is not a number");
    m = e->P.fn[fn].n;
    nb_total = resid_blocks(m);
    dst[FIT].item_bytes = dst[Z].item_bytes = (size_t)m * sizeof(double);
    dst[THETA].item_bytes = (size_t)e->P.d * sizeof(double);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return m; }
  ResidPieces carve(const mhx_engine* e, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_resid(c, nb_total, e->P.d, dst[THETA].p ? 1 : 0, want, n_items, m_points);
  }
  // what depends on the chains alone is done on the portion's first chunk of points
  int upload(mhx_engine* e, const Portion& p) const {
    if (p.m0 != 0) return MHX_OK;
    Carver c;
    const ResidPieces s = carve(e, c, p.n, p.m);
    if (dst[THETA].p)
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.theta), dst[THETA].at(p.i0), (size_t)p.n * dst[THETA].item_bytes,
                             hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(stage_at<int32_t>(e, s.status), 0, (size_t)p.n * sizeof(int32_t), e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const ResidPieces s = carve(e, c, p.n, p.m);
    const Dataset& D = e->data[fn];
    ResidArgs A{};
    A.c0 = p.i0, A.n = p.n;
    A.fn = fn;
    A.n_blocks = (int32_t)resid_blocks(p.m);
    A.blk0 = p.m0 / MHX_RESID_BLOCK, A.nb_total = nb_total, A.m = p.m, A.p_first = p.m0;
    A.z_limit = z_limit;
    A.theta = dst[THETA].p ? stage_at<double>(e, s.theta) : nullptr;
    A.data = data_view(e->P.fn[fn], D.planes ? &D.pd : nullptr, p.m0);
    A.fit = (want & RESID_WANT_FIT) ? stage_at<double>(e, s.fit) : nullptr;
    A.z = (want & RESID_WANT_Z) ? stage_at<double>(e, s.z) : nullptr;
    A.part_chi2 = stage_at<double>(e, s.part_chi2);
    A.part_sumz = stage_at<double>(e, s.part_sumz);
    A.part_dw = stage_at<double>(e, s.part_dw);
    A.part_max = stage_at<double>(e, s.part_max);
    A.part_idx = stage_at<int64_t>(e, s.part_idx);
    A.part_cnt = stage_at<int32_t>(e, s.part_cnt);
    A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_model(e, A));
    if (p.m0 + p.m >= m)
      HIP_TRY(launch_resid_totals(e->stream, p.n, nb_total, A, stage_at<double>(e, s.chi2),
                                  stage_at<double>(e, s.sum_z), stage_at<double>(e, s.dw),
                                  stage_at<double>(e, s.max_abs_z), stage_at<int64_t>(e, s.max_index),
                                  stage_at<int32_t>(e, s.n_pos), stage_at<int32_t>(e, s.n_runs),
                                  stage_at<int32_t>(e, s.n_out)));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const ResidPieces s = carve(e, c, p.n, p.m);
    const size_t pw[2] = {s.fit, s.z};
    for (int k = 0; k < 2; ++k) {
      const int rc = copy_back_points(dst[FIT + k], p, m, sizeof(double), 1, e->stage.p + pw[k]);
      if (rc != MHX_OK) return rc;
    }
    if (p.m0 + p.m < m) return MHX_OK;  // (the totals come with the last chunk of points)
    return copy_back_each(e, dst, p,
                          {s.chi2, s.sum_z, s.dw, s.max_abs_z, s.max_index, s.n_pos, s.n_runs, s.n_out, s.status});
  }
};

int mhx_get_residuals(mhx_engine* e, int fn, const double* theta, double z_limit, double* fit,
                      double* z, double* chi2, double* sum_z, double* dw, double* max_abs_z,
                      int64_t* max_index, int32_t* n_pos, int32_t* n_runs, int32_t* n_out,
                      int32_t* status) {
  return run_portions(e, ResidCall(fn, theta, z_limit, fit, z, chi2, sum_z, dw, max_abs_z, max_index, n_pos,
                                   n_runs, n_out, status));
}

// ---- normal equations (include/mhx.h has the definition): function fn and its central differences
// at one parameter vector per chain over the chain's own data, the block partials of the products
// (k_normeq), then their totals, scattered through the function's gather map (k_normeq_totals).
// An item is a chain; the function's points go in chunks of kFitChunkPoints, a whole number of
// MHX_NORMEQ_BLOCK blocks, so a block is the same points whatever the split.  The partials of all
// chunks stay in the stage; the totals are taken on the last chunk.  g moves by copy_back_points.
struct NormEqCall {
  int fn = 0, per_chain = 0, p = 0, n_tasks = 0;
  int32_t col[MHX_MAX_FN_PARAMS] = {};
  int64_t m = 0, nb_total = 0;
  int64_t n_all = 0;  // the chains of the caller's arrays: the engine's, or the whole group's
  enum { JTJ, JTR, CHI2, STATUS, G, THETA, STEPS, N_DST };
  HostDst dst[N_DST];  // (THETA and STEPS are read, not written: they lie here to move with a group's chains)
  static_assert(kFitChunkPoints % MHX_NORMEQ_BLOCK == 0, "a chunk of points is whole blocks");

  NormEqCall(int64_t n_all_, int fn_, const double* theta, const double* steps, int per_chain_steps,
             double* jtj, double* jtr, double* chi2, double* g, int32_t* status)
      : fn(fn_), per_chain(per_chain_steps != 0), n_all(n_all_) {
    dst[JTJ].p = jtj, dst[JTR].p = jtr, dst[G].p = g;
    dst[CHI2] = {chi2, sizeof(double)}, dst[STATUS] = {status, sizeof(int32_t)};
    dst[THETA].p = const_cast<double*>(theta), dst[STEPS].p = const_cast<double*>(steps);
  }
  int check(mhx_engine* e) {
    const int rc = fn_check(e, fn, "mhx_get_normal_equations");
    if (rc != MHX_OK) return rc;
    const FnDesc& f = e->P.fn[fn];
    if (!dst[STEPS].p) return fail(MHX_EINVAL, "steps is NULL");
    const int d = e->P.d;
    // (checked before a group's calls move to their engines' chains: all of the caller's steps)
    const double* hs = static_cast<const double*>(dst[STEPS].p);
    const int64_t n_steps = per_chain ? n_all * (int64_t)d : d;
    for (int64_t k = 0; k < n_steps; ++k)
      if (!(hs[k] >= 0.0) || !std::isfinite(hs[k]))
        return fail(MHX_EINVAL, "step %lld is negative or not finite", (long long)k);
    m = f.n;
    // the columns: the distinct places of theta the function reads, ascending
    bool reads[MHX_MAX_PARAMS + 1] = {};
    for (int j = 0; j < f.n_idx; ++j) reads[f.idx[j]] = true;
    p = 0;
    for (int t = 0; t < d; ++t)
      if (reads[t]) col[p++] = t;
    n_tasks = normeq_tasks(p);
    nb_total = normeq_blocks(m);
    dst[JTJ].item_bytes = (size_t)d * d * sizeof(double);
    dst[JTR].item_bytes = dst[THETA].item_bytes = (size_t)d * sizeof(double);
    dst[STEPS].item_bytes = per_chain ? (size_t)d * sizeof(double) : 0;
    dst[G].item_bytes = (size_t)d * m * sizeof(double);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return m; }
  NormEqPieces carve(const mhx_engine* e, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_normeq(c, nb_total, n_tasks, e->P.d, per_chain, dst[THETA].p ? 1 : 0, dst[G].p ? 1 : 0,
                        n_items, m_points);
  }
  // what depends on the chains alone is done on the portion's first chunk of points
  int upload(mhx_engine* e, const Portion& pn) const {
    Carver c;
    const NormEqPieces s = carve(e, c, pn.n, pn.m);
    const size_t d = (size_t)e->P.d;
    if (dst[G].p)
      HIP_TRY(hipMemsetAsync(e->stage.p + s.g, 0, (size_t)pn.n * d * (size_t)pn.m * sizeof(double), e->stream));
    if (pn.m0 != 0) return MHX_OK;
    if (dst[THETA].p)
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.theta), dst[THETA].at(pn.i0), (size_t)pn.n * d * sizeof(double),
                             hipMemcpyHostToDevice, e->stream));
    if (per_chain)
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.chain_steps), dst[STEPS].at(pn.i0),
                             (size_t)pn.n * d * sizeof(double), hipMemcpyHostToDevice, e->stream));
    else
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.steps), dst[STEPS].p, d * sizeof(double),
                             hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(stage_at<int32_t>(e, s.status), 0, (size_t)pn.n * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(e->stage.p + s.jtr, 0, (size_t)pn.n * d * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->stage.p + s.jtj, 0, (size_t)pn.n * d * d * sizeof(double), e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& pn) const {
    Carver c;
    const NormEqPieces s = carve(e, c, pn.n, pn.m);
    const Dataset& D = e->data[fn];
    NormEqArgs A{};
    A.c0 = pn.i0, A.n = pn.n;
    A.fn = fn;
    A.n_blocks = (int32_t)normeq_blocks(pn.m);
    A.p = p, A.n_tasks = n_tasks, A.pitch = normeq_pitch(p);
    A.steps_pitch = per_chain ? e->P.d : 0;
    A.blk0 = pn.m0 / MHX_NORMEQ_BLOCK, A.nb_total = nb_total, A.m = pn.m;
    for (int a = 0; a < p; ++a) A.col[a] = col[a];
    A.theta = dst[THETA].p ? stage_at<double>(e, s.theta) : nullptr;
    A.steps = stage_at<double>(e, per_chain ? s.chain_steps : s.steps);
    A.data = data_view(e->P.fn[fn], D.planes ? &D.pd : nullptr, pn.m0);
    A.g = dst[G].p ? stage_at<double>(e, s.g) : nullptr;
    A.part = stage_at<double>(e, s.part);
    A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_model(e, A));  // (A.sub, A.lanes are the launcher's: they depend on the kernel's family)
    if (pn.m0 + pn.m >= m)
      HIP_TRY(launch_normeq_totals(e->stream, A, e->P.d, stage_at<double>(e, s.jtj), stage_at<double>(e, s.jtr),
                                   stage_at<double>(e, s.chi2)));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& pn) const {
    Carver c;
    const NormEqPieces s = carve(e, c, pn.n, pn.m);
    // (g: rows (chain, place) of pn.m points each, m apart at the caller's)
    const int rc = copy_back_points(dst[G], pn, m, sizeof(double), (size_t)e->P.d, e->stage.p + s.g);
    if (rc != MHX_OK || pn.m0 + pn.m < m) return rc;  // (the totals come with the last chunk of points)
    return copy_back_each(e, dst, pn, {s.jtj, s.jtr, s.chi2, s.status});
  }
};

int mhx_get_normal_equations(mhx_engine* e, int fn, const double* theta, const double* steps,
                             int per_chain_steps, double* jtj, double* jtr, double* chi2, double* g,
                             int32_t* status) {
  return run_portions(e, NormEqCall(e ? e->cfg.n_chains : 0, fn, theta, steps, per_chain_steps, jtj, jtr, chi2,
                                    g, status));
}

// ---- candidate scores (include/mhx.h has the definition): the chi-square of m_cand parameter
// vectors per chain over the chain's own data, function by function (k_cand: one launch a selected
// function, over all of its points - nothing pointwise comes back, so the points need no chunks and
// a block is the same points whatever the portions), then every candidate's total and the chain's
// `keep` best (k_cand_totals).  An item is a chain; its pieces are the m_cand scores and the
// m_cand x nb_pitch block sums, nb_pitch the blocks of all selected functions.  The data are read
// where the engine holds them, through a DataView.
struct CandCall {
  int fn = 0, per_chain = 0, keep = 0;
  int64_t m_cand = 0, nb_pitch = 0;
  enum { SCORE, BEST_INDEX, BEST_SCORE, N_BAD, CAND, N_DST };
  HostDst dst[N_DST];  // (CAND is read, not written: it lies here to move with a group's chains)

  CandCall(int fn_, const double* cand, int64_t m, int per_chain_, int keep_, double* score,
           int32_t* best_index, double* best_score, int32_t* n_bad)
      : fn(fn_), per_chain(per_chain_ != 0), keep(keep_), m_cand(m) {
    dst[SCORE].p = score, dst[BEST_INDEX].p = best_index, dst[BEST_SCORE].p = best_score;
    dst[N_BAD] = {n_bad, sizeof(int32_t)};
    dst[CAND].p = const_cast<double*>(cand);
  }
  int first_fn() const { return fn >= 0 ? fn : 0; }
  int end_fn(const mhx_engine* e) const { return fn >= 0 ? fn + 1 : e->P.K; }
  int check(mhx_engine* e) {
    if (!e) return fail(MHX_EINVAL, "engine is NULL");
    if (!dst[CAND].p) return fail(MHX_EINVAL, "cand is NULL");
    if (m_cand < 1 || m_cand > (int64_t)INT32_MAX - 1)
      return fail(MHX_EINVAL, "m must be in [1, 2^31 - 2]");
    if (keep < 1 || keep > MHX_CAND_KEEP_MAX)
      return fail(MHX_EINVAL, "keep must be in [1,%d]", MHX_CAND_KEEP_MAX);
    if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
    if (fn < -1 || fn >= e->P.K) return fail(MHX_EINVAL, "function %d out of range (-1: all)", fn);
    nb_pitch = 0;
    for (int k = first_fn(); k < end_fn(e); ++k) {
      const int rc = fn_check(e, k, "mhx_get_candidate_scores");
      if (rc != MHX_OK) return rc;
      nb_pitch += resid_blocks(e->P.fn[k].n);
    }
    const int d = e->P.d;
    if (!one_item_fits([&](Carver& c, int64_t n) { carve_cand(c, nb_pitch, d, per_chain, keep, m_cand, n); }))
      return fail(MHX_EINVAL, "%lld candidates over %lld blocks of points outgrow the stage: try fewer a call",
                  (long long)m_cand, (long long)nb_pitch);
    dst[SCORE].item_bytes = (size_t)m_cand * sizeof(double);
    dst[BEST_INDEX].item_bytes = (size_t)keep * sizeof(int32_t);
    dst[BEST_SCORE].item_bytes = (size_t)keep * sizeof(double);
    dst[CAND].item_bytes = per_chain ? (size_t)m_cand * (size_t)d * sizeof(double) : 0;
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  CandPieces carve(const mhx_engine* e, Carver& c, int64_t n_items, int64_t) const {
    return carve_cand(c, nb_pitch, e->P.d, per_chain, keep, m_cand, n_items);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const CandPieces s = carve(e, c, p.n, p.m);
    const size_t row = (size_t)m_cand * (size_t)e->P.d * sizeof(double);
    HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.cand), per_chain ? dst[CAND].at(p.i0) : dst[CAND].p,
                           per_chain ? (size_t)p.n * row : row, hipMemcpyHostToDevice, e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const CandPieces s = carve(e, c, p.n, p.m);
    int64_t blk0 = 0;
    for (int k = first_fn(); k < end_fn(e); ++k) {
      const FnDesc& f = e->P.fn[k];
      const Dataset& D = e->data[k];
      CandArgs A{};
      A.c0 = p.i0, A.n = p.n;
      A.fn = k;
      A.n_blocks = (int32_t)resid_blocks(f.n);
      A.m_cand = m_cand, A.cand_pitch = per_chain ? m_cand : 0;
      A.blk0 = blk0, A.nb_pitch = nb_pitch, A.m = f.n;
      A.cand = stage_at<double>(e, s.cand);
      A.data = data_view(f, D.planes ? &D.pd : nullptr, 0);  // (all of the function's points: no chunks)
      A.part = stage_at<double>(e, s.part);
      HIP_TRY(launch_model(e, A));
      blk0 += A.n_blocks;
    }
    HIP_TRY(launch_cand_totals(e->stream, e->dP.p, fn, p.n, m_cand, nb_pitch, keep, stage_at<double>(e, s.part),
                               stage_at<double>(e, s.score), stage_at<int32_t>(e, s.best_index),
                               stage_at<double>(e, s.best_score), stage_at<int32_t>(e, s.n_bad)));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const CandPieces s = carve(e, c, p.n, p.m);
    return copy_back_each(e, dst, p, {s.score, s.best_index, s.best_score, s.n_bad});
  }
};

int mhx_get_candidate_scores(mhx_engine* e, int fn, const double* cand, int64_t m, int per_chain,
                             int keep, double* score, int32_t* best_index, double* best_score,
                             int32_t* n_bad) {
  return run_portions(e, CandCall(fn, cand, m, per_chain, keep, score, best_index, best_score, n_bad));
}

// ---- credible bands (include/mhx.h has the definition): every chain's pointwise percentiles and
// moments of function fn over its window (k_fitpct_values, then the model-free k_fitpct_select).
// An item is a chain.  The window's values of a portion are staged, `take` doubles per chain and
// point, so the chunk of points is the call's own (fitpct_cursor, mhx_stage.hpp): whole blocks of
// the value kernel, as many as let one chain fit the budget.
struct FitPctCall {
  int fn = 0, take = 0, n_cols = 1;
  int64_t m = 0;
  const double* xcols = nullptr;  // [n_cols][m] on the host, or NULL: the function's dataset
  PctList pc{};
  enum { PCT, MEAN, STDDEV, N_USED, STATUS };
  HostDst dst[5];
  static_assert(kFitPctBlock == MHX_FITPCT_BLOCK, "MHX_FITPCT_BLOCK (include/mhx.h)");

  FitPctCall(int fn_, int take_, const double* xcols_, int n_cols_, int64_t m_, double* pct, double* mean,
             double* stddev, int32_t* n_used, int32_t* status)
      : fn(fn_), take(take_), n_cols(n_cols_), m(m_), xcols(xcols_) {
    const size_t row = (size_t)std::max<int64_t>(m, 0) * sizeof(double);
    dst[PCT].p = pct, dst[MEAN] = {mean, row}, dst[STDDEV] = {stddev, row};
    dst[N_USED] = {n_used, sizeof(int32_t)}, dst[STATUS] = {status, sizeof(int32_t)};
  }
  int check(mhx_engine* e) {
    int rc = window_check(e, take);
    if (rc != MHX_OK || (rc = fn_check(e, fn)) != MHX_OK) return rc;
    if (n_cols != FitCall::fn_cols(e, fn))
      return fail(MHX_EINVAL, "function %d reads %d column(s) of x, n_cols is %d", fn, FitCall::fn_cols(e, fn),
                  n_cols);
    if (!xcols && m != e->P.fn[fn].n)
      return fail(MHX_EINVAL, "xcols is NULL: m must be the dataset's %lld points", (long long)e->P.fn[fn].n);
    if (m < 1) return fail(MHX_EINVAL, "m must be >= 1");
    if (cursor(e).chunk < 1)
      return fail(MHX_EUNSUPPORTED, "mhx_get_fit_percentiles: the %d staged values of each of a chain's first %lld "
                                    "points do not fit the 64 MiB of a portion: the greatest take that fits is %d",
                  take, (long long)std::min<int64_t>(m, kFitPctBlock), fitpct_max_take(m, pc.n));
    dst[PCT].item_bytes = (size_t)pc.n * (size_t)m * sizeof(double);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return m; }
  PortionCursor cursor(const mhx_engine* e) const { return fitpct_cursor(items(e), m, take, pc.n); }
  FitPctPieces carve(const mhx_engine*, Carver& c, int64_t n_items, int64_t m_points) const {
    return carve_fitpct(c, take, pc.n, n_items, m_points);
  }
  // chains [i0, i0 + n) at points [m0, m0 + m): the status gathers over the chunks of points
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const FitPctPieces s = carve(e, c, p.n, p.m);
    const size_t mb = (size_t)p.m * sizeof(double);
    if (xcols) {
      HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.x0), xcols + p.m0, mb, hipMemcpyHostToDevice, e->stream));
      if (n_cols > 1)
        HIP_TRY(hipMemcpyAsync(stage_at<double>(e, s.x1), xcols + m + p.m0, mb, hipMemcpyHostToDevice, e->stream));
    }
    if (p.m0 == 0)
      HIP_TRY(hipMemsetAsync(stage_at<int32_t>(e, s.status), 0, (size_t)p.n * sizeof(int32_t), e->stream));
    return MHX_OK;
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const FitPctPieces s = carve(e, c, p.n, p.m);
    const FnDesc& f = e->P.fn[fn];
    const bool step_fastest = e->knobs.fitpct_step_fastest;
    FitPctArgs A{};
    A.c0 = p.i0, A.n = p.n;
    A.take = take, A.fn = fn;
    A.n_blocks = (int32_t)fitpct_blocks(p.m);
    A.m = p.m;
    A.vs_step = step_fastest ? 1 : p.m, A.vs_point = step_fastest ? take : 1;
    if (xcols) {
      A.x0 = stage_at<double>(e, s.x0);
      A.x1 = n_cols > 1 ? stage_at<double>(e, s.x1) : nullptr;
    } else {
      A.x0 = f.x + p.m0;
      A.x1 = f.n_xcols > 1 ? f.c + p.m0 : nullptr;
    }
    A.values = stage_at<double>(e, s.values);
    A.mean = stage_at<double>(e, s.mean);
    A.stddev = stage_at<double>(e, s.stddev);
    A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_model(e, A));
    // (no percentile asked for: the selection only completes n_used and the status - no column is laid down)
    const bool lds = pc.n > 0 && !e->knobs.fitpct_no_lds && fitpct_cols(take) > 0;
    HIP_TRY(launch_fitpct_select(e->stream, e->S, p.i0, p.n, take, p.m, A.vs_step, A.vs_point, pc, lds,
                                 !e->knobs.fitpct_select_singly, A.values,
                                 stage_at<double>(e, s.pct), stage_at<int32_t>(e, s.n_used), A.status));
    e->launches++;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const FitPctPieces s = carve(e, c, p.n, p.m);
    const size_t dv[3] = {s.pct, s.mean, s.stddev};
    for (int k = 0; k < 3; ++k) {  // (pct: a row per chain and percentile)
      const int rc = copy_back_points(dst[k], p, m, sizeof(double), k == PCT ? (size_t)pc.n : 1, e->stage.p + dv[k]);
      if (rc != MHX_OK) return rc;
    }
    if (p.m0 + p.m < m) return MHX_OK;  // (the status gathers over the chunks of points)
    return copy_back_each(e, dst + N_USED, p, {s.n_used, s.status});
  }
};

int mhx_get_fit_percentiles(mhx_engine* e, int fn, int take, const double* xcols, int n_cols, int64_t m,
                            const int32_t* pct_num, const int32_t* pct_den, int n_pct, double* pct,
                            double* mean, double* stddev, int32_t* n_used, int32_t* status) {
  FitPctCall q(fn, take, xcols, n_cols, m, pct, mean, stddev, n_used, status);
  int rc = window_check(e, take);
  if (rc != MHX_OK || (rc = fill_pcts(&q.pc, pct_num, pct_den, n_pct)) != MHX_OK) return rc;
  return run_portions(e, q);
}

// ---- walker-with-exp (M:1052-1064) and the posterior of the expression: derived quantities of
// every chain on the device (mhx_user_derived, run-time compiled: mhx_derived.hpp; then
// k_derived_summary).  A portion's pieces: the values [n][ne][take], the results, n_used.
struct DerivedCall {
  int ne = 0, take = 0, n_names = 0;
  std::vector<std::string> exprs, names;  // prepared texts; names as given
  int32_t idx[MHX_MAX_PARAMS + 1] = {0};
  PctList pc{};
  std::shared_ptr<DerivedProgram> prog;  // of this call's engine's device
  enum { AT_BEST, PCT, MEAN, STDDEV, VALUES, N_USED, STATUS };
  HostDst dst[7];

  // the part of the arguments that needs no engine: texts, names, destinations
  int prepare(const char* const* exprs_, int n_expr, const char* const* names_, const int32_t* index,
              int n_names_, int take_, const int32_t* pct_num, const int32_t* pct_den, int n_pct,
              double* at_most_likely, double* pct, double* mean, double* stddev, double* values,
              int32_t* n_used, int32_t* status) {
    if (n_expr < 1 || n_expr > MHX_MAX_DERIVED || !exprs_)
      return fail(MHX_EINVAL, "n_expr must be in [1,%d]", MHX_MAX_DERIVED);
    if (n_names_ < 0 || n_names_ > MHX_MAX_PARAMS || (n_names_ > 0 && (!names_ || !index)))
      return fail(MHX_EINVAL, "n_names must be in [0,%d]", MHX_MAX_PARAMS);
    ne = n_expr;
    take = take_;
    n_names = n_names_;
    for (int j = 0; j < n_names; ++j) {
      if (!valid_ident(names_[j]) || !strcmp(names_[j], "prob"))
        return fail(MHX_EINVAL, "name %d is not an identifier (or is x / bounds_total / prob)", j);
      names.push_back(names_[j]);
      idx[j] = index[j];
    }
    for (int k = 0; k < n_expr; ++k) {
      if (!exprs_[k] || !*exprs_[k]) return fail(MHX_EINVAL, "expression %d is empty", k);
      std::string out, err;
      if (rtc_prepare_expr(exprs_[k], names, "prob", &out, &err) != 0)
        return fail(MHX_EINVAL, "expression %d: %s", k, err.c_str());
      exprs.push_back(out);
    }
    const int rc = fill_pcts(&pc, pct_num, pct_den, n_pct);
    if (rc != MHX_OK) return rc;
    const size_t row = (size_t)ne * sizeof(double);
    dst[AT_BEST] = {at_most_likely, row}, dst[MEAN] = {mean, row}, dst[STDDEV] = {stddev, row};
    dst[PCT] = {pct, row * (size_t)pc.n};
    dst[VALUES] = {values, row * (size_t)std::max(take, 0)};
    dst[N_USED] = {n_used, sizeof(int32_t)};
    dst[STATUS] = {status, (size_t)ne * sizeof(int32_t)};
    return MHX_OK;
  }
  int check(mhx_engine* e) {
    int rc = window_check(e, take);
    if (rc != MHX_OK) return rc;
    for (int j = 0; j < n_names; ++j)
      if (idx[j] < 0 || idx[j] >= e->P.d)
        return fail(MHX_EINVAL, "index[%d] = %d outside [0,%d)", j, idx[j], e->P.d);
    if ((rc = use_device(e)) != MHX_OK) return rc;
    std::string err;
    prog = rtc_get_derived(exprs, names, &err);
    if (!prog) return fail(MHX_EINVAL, "%s", err.c_str());
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  DerivedPieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_derived(c, ne, take, pc.n, n);
  }
  int upload(mhx_engine*, const Portion&) const { return MHX_OK; }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const DerivedPieces s = carve(e, c, p.n, p.m);
    DerivedArgs A{};
    A.c0 = p.i0;
    A.n = p.n;
    A.take = take;
    A.pitch = take;
    for (int j = 0; j < n_names; ++j) A.idx[j] = idx[j];
    A.values = stage_at<double>(e, s.values);
    A.at_best = stage_at<double>(e, s.at_best);
    const bool lds = !e->knobs.summary_no_lds && pct_lds_bytes(take, ne) <= kPctLdsBudget;
    HIP_TRY(rtc_launch_derived(*prog, e->stream, e->S, A));
    HIP_TRY(launch_derived_summary(e->stream, e->S, p.i0, p.n, take, ne, pc, lds, A.values,
                                   stage_at<double>(e, s.pct), stage_at<double>(e, s.mean),
                                   stage_at<double>(e, s.stddev), stage_at<int32_t>(e, s.n_used),
                                   stage_at<int32_t>(e, s.status)));
    e->launches += 2;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const DerivedPieces s = carve(e, c, p.n, p.m);
    const int which[5] = {AT_BEST, PCT, MEAN, STDDEV, STATUS};
    const size_t off[5] = {s.at_best, s.pct, s.mean, s.stddev, s.status};
    for (int k = 0; k < 5; ++k) {
      const int rc = copy_back(dst[which[k]], p.i0, p.n, e->stage.p + off[k]);
      if (rc != MHX_OK) return rc;
    }
    const int64_t c0 = p.i0, n = p.n;
    std::vector<int32_t> used;
    if (dst[N_USED].p || dst[VALUES].p) {
      used.resize((size_t)n);
      HIP_TRY(hipMemcpy(used.data(), stage_at<int32_t>(e, s.n_used), (size_t)n * sizeof(int32_t),
                        hipMemcpyDeviceToHost));
      if (dst[N_USED].p) memcpy(dst[N_USED].at(c0), used.data(), (size_t)n * sizeof(int32_t));
    }
    if (dst[VALUES].p) {
      // entries at and beyond n_used are not the caller's to lose: whole runs of full windows in
      // one copy, a chain with a shorter window row by row
      double* const host = static_cast<double*>(dst[VALUES].p);
      const double* const dev = stage_at<double>(e, s.values);
      const size_t per = (size_t)ne * (size_t)take;
      int64_t a = 0;
      while (a < n) {
        int64_t b = a;
        while (b < n && used[(size_t)b] == take) ++b;
        if (b > a)
          HIP_TRY(hipMemcpy(host + (size_t)(c0 + a) * per, dev + (size_t)a * per,
                            (size_t)(b - a) * per * sizeof(double), hipMemcpyDeviceToHost));
        if (b < n) {
          if (used[(size_t)b] > 0)
            HIP_TRY(hipMemcpy2D(host + (size_t)(c0 + b) * per, (size_t)take * sizeof(double),
                                dev + (size_t)b * per, (size_t)take * sizeof(double),
                                (size_t)used[(size_t)b] * sizeof(double), (size_t)ne, hipMemcpyDeviceToHost));
          ++b;
        }
        a = b;
      }
    }
    return MHX_OK;
  }
};

int mhx_get_derived(mhx_engine* e, const char* const* exprs, int n_expr, const char* const* names,
                    const int32_t* index, int n_names, int take, const int32_t* pct_num,
                    const int32_t* pct_den, int n_pct, double* at_most_likely, double* pct,
                    double* mean, double* stddev, double* values, int32_t* n_used,
                    int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  DerivedCall q;
  const int rc = q.prepare(exprs, n_expr, names, index, n_names, take, pct_num, pct_den, n_pct,
                           at_most_likely, pct, mean, stddev, values, n_used, status);
  return rc != MHX_OK ? rc : run_portions(e, q);
}

// ---- walker-param-histo (M:1361-1369) and walker-plot-corner (M:1333-1359) as integer counts
// over the caller's edges, for every chain on the device (k_histograms, k_pair_grids).  A
// portion's pieces: the edges - one set, or the portion's chains' - the counts, what fell outside
// / inside, n_used, status; the grids' pair list besides.
extern "C++" {
// the distinct parameters cols[0 .. n_cols) of a vector of d, 1 <= n_cols <= d, as a kernel's ColList
static int fill_cols(ColList* cl, const int32_t* cols, int n_cols, int d) {
  cl->n = n_cols;
  for (int p = 0; p <= MHX_MAX_PARAMS; ++p) cl->of_param[p] = -1, cl->idx[p] = 0;
  for (int c = 0; c < n_cols; ++c) {
    if (cols[c] < 0 || cols[c] >= d) return fail(MHX_EINVAL, "cols[%d] = %d outside [0,%d)", c, cols[c], d);
    if (cl->of_param[cols[c]] >= 0)
      return fail(MHX_EINVAL, "cols[%d] = %d is cols[%d] again", c, cols[c], cl->of_param[cols[c]]);
    cl->of_param[cols[c]] = c;
    cl->idx[c] = cols[c];
  }
  return MHX_OK;
}
// what the two calls share: the window, the columns and the edges
struct BinSpec {
  int take = 0, n_cols = 0, n_bins = 0, per_chain = 0;
  ColList cl{};
  size_t row() const { return (size_t)n_cols * ((size_t)n_bins + 1); }  // doubles of one set of edge rows
  // the arguments against every engine of the call; the edges of ALL its chains are read here,
  // in the caller's (global) chain order, before anything is launched
  int prepare(const std::vector<mhx_engine*>& engs, int take_, const int32_t* cols, int n_cols_,
              int n_bins_, int max_bins, const double* edges, int edges_per_chain) {
    int rc = MHX_OK;
    int64_t chains = 0;
    for (const mhx_engine* e : engs) {
      if ((rc = window_check(e, take_)) != MHX_OK) return rc;
      chains += e->cfg.n_chains;
    }
    const int d = engs[0]->P.d;
    if (n_bins_ < 1 || n_bins_ > max_bins) return fail(MHX_EINVAL, "n_bins must be in [1,%d]", max_bins);
    if (n_cols_ < 1 || n_cols_ > d || !cols) return fail(MHX_EINVAL, "n_cols must be in [1, d = %d]", d);
    if (edges_per_chain != 0 && edges_per_chain != 1) return fail(MHX_EINVAL, "edges_per_chain must be 0 or 1");
    if (!edges) return fail(MHX_EINVAL, "edges is NULL");
    take = take_, n_cols = n_cols_, n_bins = n_bins_, per_chain = edges_per_chain;
    if ((rc = fill_cols(&cl, cols, n_cols, d)) != MHX_OK) return rc;
    const int64_t sets = per_chain ? chains : 1;
    for (int64_t s = 0; s < sets; ++s)
      for (int c = 0; c < n_cols; ++c) {
        const double* b = edges + (size_t)s * row() + (size_t)c * ((size_t)n_bins + 1);
        for (int k = 0; k <= n_bins; ++k)
          if (b[k] != b[k] || (k > 0 && b[k] < b[k - 1]))
            return fail(MHX_EINVAL, "edges of chain %lld, column %d: edge %d is %s", per_chain ? (long long)s : -1LL,
                        c, k, b[k] != b[k] ? "a NaN" : "below the edge before it");
      }
    return MHX_OK;
  }
  int check(const mhx_engine* e) const {
    const int rc = window_check(e, take);
    if (rc != MHX_OK) return rc;
    for (int c = 0; c < n_cols; ++c)
      if (cl.idx[c] >= e->P.d) return fail(MHX_EINVAL, "cols[%d] = %d outside [0,%d)", c, cl.idx[c], e->P.d);
    return MHX_OK;
  }
  HostDst edges_src(const double* edges) const {
    return {const_cast<double*>(edges), per_chain ? row() * sizeof(double) : 0};
  }
  // the portion's edges into their piece: the shared set, or the rows of the chains from i0 on
  int upload_edges(mhx_engine* e, const HostDst& src, size_t piece, const Portion& p) const {
    HIP_TRY(hipMemcpyAsync(e->stage.p + piece, src.at(p.i0), (per_chain ? (size_t)p.n : 1) * row() * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    return MHX_OK;
  }
};
}  // extern "C++"

struct HistoCall {
  BinSpec b;
  // EDGES is a source, not a destination: it stands among dst[] so that a group offsets the
  // per-chain edges by the engine's first chain as it offsets the results (0 bytes an item: shared)
  enum { COUNTS, OUTSIDE, N_USED, STATUS, EDGES };
  HostDst dst[5];

  int prepare(const std::vector<mhx_engine*>& engs, int take, const int32_t* cols, int n_cols, int n_bins,
              const double* edges, int edges_per_chain, int32_t* counts, int32_t* outside,
              int32_t* n_used, int32_t* status) {
    const int rc = b.prepare(engs, take, cols, n_cols, n_bins, MHX_MAX_HISTO_BINS, edges, edges_per_chain);
    if (rc != MHX_OK) return rc;
    const size_t nc = (size_t)n_cols * sizeof(int32_t);
    dst[COUNTS] = {counts, nc * (size_t)n_bins}, dst[OUTSIDE] = {outside, nc * 2};
    dst[N_USED] = {n_used, sizeof(int32_t)}, dst[STATUS] = {status, nc};
    dst[EDGES] = b.edges_src(edges);
    return MHX_OK;
  }
  int check(mhx_engine* e) {
    const int rc = b.check(e);
    if (rc != MHX_OK) return rc;
    if (!one_item_fits([&](Carver& c, int64_t n) { carve(e, c, n, 1); }))
      return fail(MHX_EINVAL, "the pieces of ONE chain exceed the stage budget of %zu bytes", kStageBudget);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  HistoPieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_histo(c, b.n_cols, b.n_bins, b.per_chain, n);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HistoPieces s = carve(e, c, p.n, p.m);
    HIP_TRY(hipMemsetAsync(e->stage.p, 0, c.bytes(), e->stream));
    return b.upload_edges(e, dst[EDGES], s.edges, p);
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HistoPieces s = carve(e, c, p.n, p.m);
    const bool lds = !e->knobs.histo_no_lds && histo_lds_bytes(b.n_cols, b.n_bins) <= kPctLdsBudget;
    HIP_TRY(launch_histograms(e->stream, e->S, p.i0, p.n, b.take, b.cl, b.n_bins, stage_at<double>(e, s.edges),
                              b.per_chain ? (int64_t)b.row() : 0, lds, stage_at<int32_t>(e, s.counts),
                              stage_at<int32_t>(e, s.outside), stage_at<int32_t>(e, s.n_used),
                              stage_at<int32_t>(e, s.status)));
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HistoPieces s = carve(e, c, p.n, p.m);
    const size_t off[4] = {s.counts, s.outside, s.n_used, s.status};
    for (int k = 0; k < 4; ++k) {
      const int rc = copy_back(dst[k], p.i0, p.n, e->stage.p + off[k]);
      if (rc != MHX_OK) return rc;
    }
    return MHX_OK;
  }
};

struct GridCall {
  BinSpec b;
  int n_pairs = 0;
  std::vector<int32_t> pairs;  // pair_a [n_pairs], then pair_b [n_pairs]
  enum { COUNTS, N_INSIDE, N_USED, STATUS, EDGES };  // (EDGES: as HistoCall's)
  HostDst dst[5];

  int prepare(const std::vector<mhx_engine*>& engs, int take, const int32_t* cols, int n_cols,
              const int32_t* pair_a, const int32_t* pair_b, int n_pairs_, int n_bins, const double* edges,
              int edges_per_chain, int32_t* counts, int32_t* n_inside, int32_t* n_used, int32_t* status) {
    const int rc = b.prepare(engs, take, cols, n_cols, n_bins, MHX_MAX_GRID_BINS, edges, edges_per_chain);
    if (rc != MHX_OK) return rc;
    if (n_pairs_ < 0 || n_pairs_ > MHX_MAX_GRID_PAIRS || (n_pairs_ > 0 && (!pair_a || !pair_b)))
      return fail(MHX_EINVAL, "n_pairs must be in [0,%d]", MHX_MAX_GRID_PAIRS);
    n_pairs = n_pairs_;
    pairs.assign((size_t)2 * n_pairs, 0);
    for (int q = 0; q < n_pairs; ++q) {
      if (pair_a[q] < 0 || pair_a[q] >= n_cols || pair_b[q] < 0 || pair_b[q] >= n_cols || pair_a[q] == pair_b[q])
        return fail(MHX_EINVAL, "pair %d: (%d, %d) are not two distinct places in cols[%d]", q, pair_a[q],
                    pair_b[q], n_cols);
      pairs[(size_t)q] = pair_a[q];
      pairs[(size_t)n_pairs + q] = pair_b[q];
    }
    const size_t np = (size_t)n_pairs * sizeof(int32_t);
    dst[COUNTS] = {counts, np * (size_t)n_bins * (size_t)n_bins}, dst[N_INSIDE] = {n_inside, np};
    dst[N_USED] = {n_used, sizeof(int32_t)}, dst[STATUS] = {status, np};
    dst[EDGES] = b.edges_src(edges);
    return MHX_OK;
  }
  int check(mhx_engine* e) {
    const int rc = b.check(e);
    if (rc != MHX_OK) return rc;
    if (!one_item_fits([&](Carver& c, int64_t n) { carve(e, c, n, 1); }))
      return fail(MHX_EINVAL, "the pieces of ONE chain (%d pairs of %d x %d cells) exceed the stage budget of %zu bytes",
                  n_pairs, b.n_bins, b.n_bins, kStageBudget);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  GridPieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_grid(c, b.n_cols, b.n_bins, n_pairs, b.per_chain, n);
  }
  int upload(mhx_engine* e, const Portion& p) const {
    Carver c;
    const GridPieces s = carve(e, c, p.n, p.m);
    HIP_TRY(hipMemsetAsync(e->stage.p, 0, c.bytes(), e->stream));
    if (n_pairs > 0)
      HIP_TRY(hipMemcpyAsync(e->stage.p + s.pairs, pairs.data(), pairs.size() * sizeof(int32_t),
                             hipMemcpyHostToDevice, e->stream));
    return b.upload_edges(e, dst[EDGES], s.edges, p);
  }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const GridPieces s = carve(e, c, p.n, p.m);
    const bool lds = !e->knobs.histo_no_lds && grid_lds_bytes(b.take, b.n_cols, b.n_bins, n_pairs) <= kPctLdsBudget;
    HIP_TRY(launch_pair_grids(e->stream, e->S, p.i0, p.n, b.take, b.cl, b.n_bins, n_pairs,
                              stage_at<double>(e, s.edges), b.per_chain ? (int64_t)b.row() : 0,
                              stage_at<int32_t>(e, s.pairs), lds, stage_at<int32_t>(e, s.counts),
                              stage_at<int32_t>(e, s.n_inside), stage_at<int32_t>(e, s.n_used),
                              stage_at<int32_t>(e, s.status)));
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const GridPieces s = carve(e, c, p.n, p.m);
    const size_t off[4] = {s.counts, s.n_inside, s.n_used, s.status};
    for (int k = 0; k < 4; ++k) {
      const int rc = copy_back(dst[k], p.i0, p.n, e->stage.p + off[k]);
      if (rc != MHX_OK) return rc;
    }
    return MHX_OK;
  }
};

int mhx_get_histograms(mhx_engine* e, int take, const int32_t* cols, int n_cols, int n_bins,
                       const double* edges, int edges_per_chain, int32_t* counts, int32_t* outside,
                       int32_t* n_used, int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  HistoCall q;
  const int rc = q.prepare({e}, take, cols, n_cols, n_bins, edges, edges_per_chain, counts, outside, n_used, status);
  return rc != MHX_OK ? rc : run_portions(e, q);
}
int mhx_get_pair_grids(mhx_engine* e, int take, const int32_t* cols, int n_cols, const int32_t* pair_a,
                       const int32_t* pair_b, int n_pairs, int n_bins, const double* edges,
                       int edges_per_chain, int32_t* counts, int32_t* n_inside, int32_t* n_used,
                       int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  GridCall q;
  const int rc = q.prepare({e}, take, cols, n_cols, pair_a, pair_b, n_pairs, n_bins, edges, edges_per_chain,
                           counts, n_inside, n_used, status);
  return rc != MHX_OK ? rc : run_portions(e, q);
}

// ---- autocorrelation time, effective sample size and the half moments of split R-hat of every
// chain on the device (k_autocorr; include/mhx.h has the definitions).  A portion's pieces: rho -
// which the kernel reads back, so it is carved whether or not the caller wants it - tau, ess, the
// half means and variances, n_lags, n_used, status.
extern "C++" {
struct AutocorrCall {
  int take = 0, max_lag = 0;
  ColList cl{};
  enum { ACF, TAU, ESS, HALF_MEAN, HALF_VAR, N_LAGS, N_USED, STATUS };
  HostDst dst[8];

  int prepare(const std::vector<mhx_engine*>& engs, int take_, const int32_t* cols, int n_cols, int max_lag_,
              double* tau, double* ess, double* acf, double* half_mean, double* half_var, int32_t* n_lags,
              int32_t* n_used, int32_t* status) {
    for (const mhx_engine* e : engs) {
      const int rc = window_check(e, take_);
      if (rc != MHX_OK) return rc;
    }
    const int d = engs[0]->P.d;
    if (max_lag_ < 1 || max_lag_ > MHX_MAX_AUTOCORR_LAG)
      return fail(MHX_EINVAL, "max_lag must be in [1,%d]", MHX_MAX_AUTOCORR_LAG);
    if (n_cols < 1 || n_cols > d || !cols) return fail(MHX_EINVAL, "n_cols must be in [1, d = %d]", d);
    take = take_, max_lag = max_lag_;
    const int rc = fill_cols(&cl, cols, n_cols, d);
    if (rc != MHX_OK) return rc;
    const size_t nc = (size_t)n_cols * sizeof(double);
    dst[ACF] = {acf, nc * ((size_t)max_lag + 1)};
    dst[TAU] = {tau, nc}, dst[ESS] = {ess, nc};
    dst[HALF_MEAN] = {half_mean, nc * 2}, dst[HALF_VAR] = {half_var, nc * 2};
    dst[N_LAGS] = {n_lags, sizeof(int32_t)}, dst[N_USED] = {n_used, sizeof(int32_t)};
    dst[STATUS] = {status, (size_t)n_cols * sizeof(int32_t)};
    return MHX_OK;
  }
  int check(mhx_engine* e) {
    const int rc = window_check(e, take);
    if (rc != MHX_OK) return rc;
    for (int c = 0; c < cl.n; ++c)
      if (cl.idx[c] >= e->P.d) return fail(MHX_EINVAL, "cols[%d] = %d outside [0,%d)", c, cl.idx[c], e->P.d);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  AutocorrPieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_autocorr(c, cl.n, max_lag, n);
  }
  // (the kernel writes every entry that collect() copies: nothing to clear)
  int upload(mhx_engine*, const Portion&) const { return MHX_OK; }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const AutocorrPieces s = carve(e, c, p.n, p.m);
    const bool lds = !e->knobs.autocorr_no_lds && autocorr_lds_bytes(take, cl.n, true) <= kPctLdsBudget;
    HIP_TRY(launch_autocorr(e->stream, e->S, p.i0, p.n, take, cl, max_lag, lds, stage_at<double>(e, s.acf),
                            stage_at<double>(e, s.tau), stage_at<double>(e, s.ess),
                            stage_at<double>(e, s.half_mean), stage_at<double>(e, s.half_var),
                            stage_at<int32_t>(e, s.n_lags), stage_at<int32_t>(e, s.n_used),
                            stage_at<int32_t>(e, s.status)));
    return MHX_OK;
  }
  // the items of [0, n) for which whole(item) holds, in runs of one copy each
  template <class Whole>
  static int copy_runs(const HostDst& h, int64_t i0, int64_t n, const unsigned char* dev, Whole whole) {
    for (int64_t a = 0; a < n;) {
      if (!whole(a)) {
        ++a;
        continue;
      }
      int64_t b = a;
      while (b < n && whole(b)) ++b;
      HIP_TRY(hipMemcpy(h.at(i0 + a), dev + (size_t)a * h.item_bytes, (size_t)(b - a) * h.item_bytes,
                        hipMemcpyDeviceToHost));
      a = b;
    }
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const AutocorrPieces s = carve(e, c, p.n, p.m);
    const int which[5] = {TAU, ESS, N_LAGS, N_USED, STATUS};
    const size_t off[5] = {s.tau, s.ess, s.n_lags, s.n_used, s.status};
    int rc = MHX_OK;
    for (int k = 0; k < 5; ++k)
      if ((rc = copy_back(dst[which[k]], p.i0, p.n, e->stage.p + off[k])) != MHX_OK) return rc;
    if (!dst[ACF].p && !dst[HALF_MEAN].p && !dst[HALF_VAR].p) return MHX_OK;
    // what the kernel did not write is not the caller's to lose: the half moments of a window of
    // fewer than two steps, rho beyond n_lags
    const size_t n = (size_t)p.n;
    std::vector<int32_t> used(n), lags(n);
    HIP_TRY(hipMemcpy(used.data(), stage_at<int32_t>(e, s.n_used), n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lags.data(), stage_at<int32_t>(e, s.n_lags), n * sizeof(int32_t), hipMemcpyDeviceToHost));
    const auto halves = [&](int64_t a) { return used[(size_t)a] >= 2; };
    if (dst[HALF_MEAN].p && (rc = copy_runs(dst[HALF_MEAN], p.i0, p.n, e->stage.p + s.half_mean, halves)) != MHX_OK)
      return rc;
    if (dst[HALF_VAR].p && (rc = copy_runs(dst[HALF_VAR], p.i0, p.n, e->stage.p + s.half_var, halves)) != MHX_OK)
      return rc;
    if (dst[ACF].p) {
      // whole runs of chains with every lag in one copy; neighbours that share a smaller n_lags in
      // one 2-D copy (the rows of a run lie at one pitch: its height is the run's columns)
      if ((rc = copy_runs(dst[ACF], p.i0, p.n, e->stage.p + s.acf,
                          [&](int64_t a) { return lags[(size_t)a] == max_lag; })) != MHX_OK)
        return rc;
      const size_t row = ((size_t)max_lag + 1) * sizeof(double);
      for (int64_t a = 0; a < p.n;) {
        const int32_t la = lags[(size_t)a];
        int64_t b = a + 1;
        while (b < p.n && lags[(size_t)b] == la) ++b;
        if (la >= 0 && la < max_lag)
          HIP_TRY(hipMemcpy2D(dst[ACF].at(p.i0 + a), row, e->stage.p + s.acf + (size_t)a * dst[ACF].item_bytes, row,
                              ((size_t)la + 1) * sizeof(double), (size_t)(b - a) * (size_t)cl.n,
                              hipMemcpyDeviceToHost));
        a = b;
      }
    }
    return MHX_OK;
  }
};
}  // extern "C++"

int mhx_get_autocorr(mhx_engine* e, int take, const int32_t* cols, int n_cols, int max_lag, double* tau,
                     double* ess, double* acf, double* half_mean, double* half_var, int32_t* n_lags,
                     int32_t* n_used, int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  AutocorrCall q;
  const int rc = q.prepare({e}, take, cols, n_cols, max_lag, tau, ess, acf, half_mean, half_var, n_lags, n_used, status);
  return rc != MHX_OK ? rc : run_portions(e, q);
}

// ---- highest-density intervals and quantile ladders of every chain on the device (k_hdi;
// include/mhx.h has the definition): the window's columns - the ring's, or the values of derived
// expressions staged by mhx_user_derived - sorted as keys.  A portion's pieces: the staged values
// (derived form), lo, hi, pos, the ladder, n_used, status and, on the memory path, the keys.
extern "C++" {
static int hdi_mass_check(int32_t num, int32_t den) {
  return den >= 1 && den <= 1000000 && num >= 1 && (int64_t)num <= (int64_t)100 * den;
}
struct HdiCall {
  int take = 0, n_cols = 0, n_mass = 0, n_ladder = 0;
  bool derived = false, lds = false;  // lds: the path on this call's engine (check)
  ColList cl{};
  int32_t num[MHX_MAX_HDI_MASSES] = {0}, den[MHX_MAX_HDI_MASSES] = {0};
  DerivedCall dq;  // the derived form's texts, names and compiled module
  enum { LO, HI, POS, LADDER, N_USED, STATUS };
  HostDst dst[6];

  // cols NULL: the derived form, n_cols_ expressions that dq has already taken
  int prepare(const std::vector<mhx_engine*>& engs, int take_, const int32_t* cols, int n_cols_,
              const int32_t* mass_num, const int32_t* mass_den, int n_mass_, int n_ladder_, double* lo, double* hi,
              int32_t* pos, double* ladder, int32_t* n_used, int32_t* status) {
    int rc = MHX_OK;
    for (const mhx_engine* e : engs)
      if ((rc = window_check(e, take_)) != MHX_OK) return rc;
    const int d = engs[0]->P.d;
    if (!derived) {
      if (n_cols_ < 1 || n_cols_ > d || !cols) return fail(MHX_EINVAL, "n_cols must be in [1, d = %d]", d);
      if ((rc = fill_cols(&cl, cols, n_cols_, d)) != MHX_OK) return rc;
    } else {
      cl = ColList{};
      cl.n = n_cols_;
    }
    if (n_mass_ < 0 || n_mass_ > MHX_MAX_HDI_MASSES || (n_mass_ > 0 && (!mass_num || !mass_den)))
      return fail(MHX_EINVAL, "n_mass must be in [0,%d]", MHX_MAX_HDI_MASSES);
    for (int q = 0; q < n_mass_; ++q) {
      if (!hdi_mass_check(mass_num[q], mass_den[q]))
        return fail(MHX_EINVAL, "mass %d: %d/%d is outside (0, 100] or its denominator outside [1, 1000000]", q,
                    mass_num[q], mass_den[q]);
      num[q] = mass_num[q], den[q] = mass_den[q];
    }
    if (n_ladder_ != 0 && (n_ladder_ < 2 || n_ladder_ > MHX_MAX_HDI_LADDER))
      return fail(MHX_EINVAL, "n_ladder must be 0 or in [2,%d]", MHX_MAX_HDI_LADDER);
    take = take_, n_cols = n_cols_, n_mass = n_mass_, n_ladder = n_ladder_;
    const size_t cell = (size_t)n_mass * (size_t)n_cols;
    dst[LO] = {lo, cell * sizeof(double)}, dst[HI] = {hi, cell * sizeof(double)};
    dst[POS] = {pos, cell * sizeof(int32_t)};
    dst[LADDER] = {ladder, (size_t)n_cols * (size_t)n_ladder * sizeof(double)};
    dst[N_USED] = {n_used, sizeof(int32_t)}, dst[STATUS] = {status, (size_t)n_cols * sizeof(int32_t)};
    return MHX_OK;
  }
  int check(mhx_engine* e) {
    int rc = window_check(e, take);
    if (rc != MHX_OK) return rc;
    if (derived) {
      if ((rc = dq.check(e)) != MHX_OK) return rc;
    } else {
      for (int c = 0; c < cl.n; ++c)
        if (cl.idx[c] >= e->P.d) return fail(MHX_EINVAL, "cols[%d] = %d outside [0,%d)", c, cl.idx[c], e->P.d);
    }
    lds = hdi_use_lds(take, n_cols, e->knobs);
    if (!one_item_fits([&](Carver& c, int64_t n) { carve(e, c, n, 1); }))
      return fail(MHX_EINVAL, "the pieces of ONE chain (the keys of %d columns of %lld slots among them) exceed the "
                              "stage budget of %zu bytes", n_cols, (long long)hdi_pad(take), kStageBudget);
    return MHX_OK;
  }
  int64_t items(const mhx_engine* e) const { return e->cfg.n_chains; }
  int64_t points() const { return 1; }
  HdiPieces carve(const mhx_engine*, Carver& c, int64_t n, int64_t) const {
    return carve_hdi(c, n_cols, n_mass, n_ladder, take, derived ? 1 : 0, lds ? 0 : hdi_pad(take), n);
  }
  // (the kernel writes every entry that collect() copies: nothing to clear)
  int upload(mhx_engine*, const Portion&) const { return MHX_OK; }
  int launch(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HdiPieces s = carve(e, c, p.n, p.m);
    HdiArgs A{};
    A.c0 = p.i0;
    A.take = take, A.n_mass = n_mass, A.n_ladder = n_ladder;
    A.use_lds = lds ? 1 : 0;
    A.tpad = (int32_t)hdi_pad(take);
    for (int q = 0; q < n_mass; ++q) A.mass_num[q] = num[q], A.mass_den[q] = den[q];
    A.cl = cl;
    if (derived) {
      DerivedArgs D{};
      D.c0 = p.i0;
      D.n = p.n;
      D.take = take;
      D.pitch = take;
      for (int j = 0; j < dq.n_names; ++j) D.idx[j] = dq.idx[j];
      D.values = stage_at<double>(e, s.values);
      D.at_best = nullptr;
      HIP_TRY(rtc_launch_derived(*dq.prog, e->stream, e->S, D));
      A.vals = D.values;
      A.vals_chain = (int64_t)n_cols * take, A.vals_col = take, A.vals_step = 1;
      ++e->launches;
    }
    A.keys = lds ? nullptr : stage_at<unsigned long long>(e, s.keys);
    A.lo = stage_at<double>(e, s.lo), A.hi = stage_at<double>(e, s.hi);
    A.pos = stage_at<int32_t>(e, s.pos);
    A.ladder = stage_at<double>(e, s.ladder);
    A.n_used = stage_at<int32_t>(e, s.n_used), A.status = stage_at<int32_t>(e, s.status);
    HIP_TRY(launch_hdi(e->stream, e->S, p.n, A));
    ++e->launches;
    return MHX_OK;
  }
  int collect(mhx_engine* e, const Portion& p) const {
    Carver c;
    const HdiPieces s = carve(e, c, p.n, p.m);
    return copy_back_each(e, dst, p, {s.lo, s.hi, s.pos, s.ladder, s.n_used, s.status});
  }
};
// the two forms over the engines of one call (first NULL: one engine)
static int hdi_run(const std::vector<mhx_engine*>& engs, const int64_t* first, int take, const int32_t* cols,
                   int n_cols, const int32_t* mass_num, const int32_t* mass_den, int n_mass, int n_ladder,
                   double* lo, double* hi, int32_t* pos, double* ladder, int32_t* n_used, int32_t* status) {
  HdiCall q;
  const int rc = q.prepare(engs, take, cols, n_cols, mass_num, mass_den, n_mass, n_ladder, lo, hi, pos, ladder,
                           n_used, status);
  return rc != MHX_OK ? rc : run_portions(engs, first, q);
}
static int derived_hdi_run(const std::vector<mhx_engine*>& engs, const int64_t* first, const char* const* exprs,
                           int n_expr, const char* const* names, const int32_t* index, int n_names, int take,
                           const int32_t* mass_num, const int32_t* mass_den, int n_mass, int n_ladder, double* lo,
                           double* hi, int32_t* pos, double* ladder, int32_t* n_used, int32_t* status) {
  HdiCall q;
  q.derived = true;
  int rc = q.dq.prepare(exprs, n_expr, names, index, n_names, take, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr);
  if (rc == MHX_OK)
    rc = q.prepare(engs, take, nullptr, n_expr, mass_num, mass_den, n_mass, n_ladder, lo, hi, pos, ladder, n_used,
                   status);
  return rc != MHX_OK ? rc : run_portions(engs, first, q);
}
}  // extern "C++"

int mhx_hdi_span(int64_t n, int32_t num, int32_t den, int64_t* g) {
  if (n < 1) return fail(MHX_EINVAL, "n must be >= 1");
  if (!hdi_mass_check(num, den))
    return fail(MHX_EINVAL, "the mass %d/%d is outside (0, 100] or its denominator outside [1, 1000000]", num, den);
  if (g) *g = hdi_span_of(n, num, den);
  return MHX_OK;
}
int mhx_get_hdi(mhx_engine* e, int take, const int32_t* cols, int n_cols, const int32_t* mass_num,
                const int32_t* mass_den, int n_mass, int n_ladder, double* lo, double* hi, int32_t* pos,
                double* ladder, int32_t* n_used, int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  return hdi_run({e}, nullptr, take, cols, n_cols, mass_num, mass_den, n_mass, n_ladder, lo, hi, pos, ladder, n_used,
                 status);
}
int mhx_get_derived_hdi(mhx_engine* e, const char* const* exprs, int n_expr, const char* const* names,
                        const int32_t* index, int n_names, int take, const int32_t* mass_num,
                        const int32_t* mass_den, int n_mass, int n_ladder, double* lo, double* hi, int32_t* pos,
                        double* ladder, int32_t* n_used, int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  return derived_hdi_run({e}, nullptr, exprs, n_expr, names, index, n_names, take, mass_num, mass_den, n_mass,
                         n_ladder, lo, hi, pos, ladder, n_used, status);
}

// ---- ensemble percentiles: ONE posterior from all chains of a walker set (k_ensemble_digits;
// include/mhx.h has the definitions, mhx_ensemble.hpp the bookkeeping).  Eight count passes and,
// where a `between` rank is the last of its run, one successor pass.  Per pass and engine: the
// task list goes up, the counters are cleared, one launch over all the engine's chains, tasks x
// 2 KiB of counters come back.  The host adds the engines' counters (exact integers), picks every
// target's digit once and hands every engine the same next tasks.  The scratch does not depend
// on `take` or grow with the pool: no portions.
extern "C++" {
static int ensemble_run(const std::vector<mhx_engine*>& engs, const int64_t* first, int take,
                        const int32_t* cols, int n_cols, const uint8_t* include, const int32_t* pct_num,
                        const int32_t* pct_den, int n_pct, double* out, int64_t* n_pooled, int32_t* n_used,
                        int32_t* status) {
  static_assert(kEnsMaxTasks == 1008, "63 columns x 16 percentiles");
  int rc = MHX_OK;
  for (const mhx_engine* e : engs)
    if ((rc = window_check(e, take)) != MHX_OK) return rc;
  const int d = engs[0]->P.d;
  if (n_cols < 1 || n_cols > d || !cols) return fail(MHX_EINVAL, "n_cols must be in [1, d = %d]", d);
  ColList cl{};
  PctList pc{};
  if ((rc = fill_cols(&cl, cols, n_cols, d)) != MHX_OK || (rc = fill_pcts(&pc, pct_num, pct_den, n_pct)) != MHX_OK)
    return rc;
  const size_t E = engs.size();
  int64_t total = 0;
  std::vector<int64_t> at(E);
  for (size_t i = 0; i < E; ++i) {
    if (engs[i]->P.d != d) return fail(MHX_EINVAL, "the engines' parameter counts differ");
    at[i] = first ? first[i] : 0;
    total += engs[i]->cfg.n_chains;
  }
  if (include) {
    bool any = false;
    for (int64_t c = 0; c < total && !any; ++c) any = include[c] != 0;
    if (!any) return fail(MHX_EINVAL, "include leaves no chain");
  }
  const int max_tasks = ensemble_max_tasks(n_cols, n_pct);
  std::vector<EnsemblePieces> pieces(E);
  auto give_up = [&](int code) {
    for (mhx_engine* e : engs) drain(e);
    return code;
  };
  // the scratch, cleared; the mask of the engine's own chains
  auto prepare = [&](size_t i) -> int {
    mhx_engine* e = engs[i];
    Carver cv;
    pieces[i] = carve_ensemble(cv, max_tasks, n_cols, e->cfg.n_chains);
    int r = use_device(e);
    if (r != MHX_OK || (r = ensure_stage(e, cv.bytes())) != MHX_OK) return r;
    e->summary_ms = 0.0;
    HIP_TRY(hipMemsetAsync(e->stage.p, 0, cv.bytes(), e->stream));
    if (include)
      HIP_TRY(hipMemcpyAsync(e->stage.p + pieces[i].include, include + at[i], (size_t)e->cfg.n_chains,
                             hipMemcpyHostToDevice, e->stream));
    return MHX_OK;
  };
  for (size_t i = 0; i < E; ++i)
    if ((rc = prepare(i)) != MHX_OK) return give_up(rc);

  std::vector<EnsTask> tasks((size_t)max_tasks);
  std::vector<uint64_t> sum, part;
  // One pass: `nt` tasks of `words` counters each, cleared to `fill` bytes; every engine's launch
  // is enqueued before any is waited for; sum[] gathers the engines' counters by `join`.
  auto enqueue = [&](size_t i, int mode, int nt, size_t words, int fill) -> int {
    mhx_engine* e = engs[i];
    const EnsemblePieces& s = pieces[i];
    const int r = use_device(e);
    if (r != MHX_OK) return r;
    HIP_TRY(hipMemcpyAsync(e->stage.p + s.tasks, tasks.data(), (size_t)nt * sizeof(EnsTask), hipMemcpyHostToDevice,
                           e->stream));
    HIP_TRY(hipMemsetAsync(e->stage.p + s.counters, fill, (size_t)nt * words * sizeof(uint64_t), e->stream));
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    const bool lds = !e->knobs.ensemble_no_lds && ensemble_lds_bytes(take, cl.n, true) <= kPctLdsBudget;
    HIP_TRY(launch_ensemble_digits(e->stream, e->S, e->cfg.n_chains, take, cl,
                                   include ? stage_at<uint8_t>(e, s.include) : nullptr,
                                   stage_at<EnsTask>(e, s.tasks), nt, mode, lds, stage_at<uint64_t>(e, s.counters),
                                   stage_at<int32_t>(e, s.n_used), stage_at<int32_t>(e, s.status)));
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    return MHX_OK;
  };
  auto collect = [&](size_t i, size_t n_words, bool least) -> int {
    mhx_engine* e = engs[i];
    const int r = use_device(e);
    if (r != MHX_OK) return r;
    HIP_TRY(hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->summary_ms += (double)ms;
    HIP_TRY(hipMemcpy(part.data(), e->stage.p + pieces[i].counters, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n_words; ++k) sum[k] = least ? std::min(sum[k], part[k]) : sum[k] + part[k];
    return MHX_OK;
  };
  auto pass = [&](int mode, int nt) -> int {
    const bool least = mode == ENS_SUCCESSOR;
    const size_t words = least ? 1 : (size_t)kEnsBins, n_words = (size_t)nt * words;
    sum.assign(n_words, least ? ~(uint64_t)0 : 0);
    part.resize(n_words);
    int r = MHX_OK;
    for (size_t i = 0; i < E; ++i)
      if ((r = enqueue(i, mode, nt, words, least ? 0xFF : 0)) != MHX_OK) return r;
    for (size_t i = 0; i < E; ++i)
      if ((r = collect(i, n_words, least)) != MHX_OK) return r;
    return MHX_OK;
  };

  // pass 0 counts every column whole: the pool's size comes with it
  const int n_targets = n_cols * n_pct;
  std::vector<EnsTarget> targets((size_t)n_targets);
  if ((rc = pass(ENS_COUNT_FIRST, ensemble_first_tasks(n_cols, tasks.data()))) != MHX_OK) return give_up(rc);
  int64_t pooled = 0;
  for (int b = 0; b < kEnsBins; ++b) pooled += (int64_t)sum[(size_t)b];
  if (pooled < 1) return fail(MHX_ESTATE, "the included chains hold no step");
  ensemble_targets(pooled, pc, n_cols, targets.data());
  for (int p = 0; p < kEnsPasses && n_targets > 0; ++p) {
    const int shift = ensemble_shift(p);
    if (p > 0 && (rc = pass(ENS_COUNT, ensemble_tasks(targets.data(), n_targets, shift, tasks.data()))) != MHX_OK)
      return give_up(rc);
    if (!ensemble_advance(targets.data(), n_targets, shift, sum.data()))
      return fail(MHX_EDEVICE, "ensemble percentiles: pass %d's counts do not hold a rank", p);
  }
  const int n_succ = ensemble_successor_tasks(targets.data(), n_targets, tasks.data());
  if (n_succ > 0) {
    if ((rc = pass(ENS_SUCCESSOR, n_succ)) != MHX_OK) return give_up(rc);
    ensemble_take_successors(targets.data(), n_targets, sum.data());
  }
  // the counts; then the outputs, which nothing can fail any more
  std::vector<int32_t> used((size_t)total), flags((size_t)n_cols, 0), flag_part((size_t)n_cols);
  auto counts_of = [&](size_t i) -> int {
    mhx_engine* e = engs[i];
    const int r = use_device(e);
    if (r != MHX_OK) return r;
    HIP_TRY(hipMemcpy(used.data() + at[i], e->stage.p + pieces[i].n_used, (size_t)e->cfg.n_chains * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flag_part.data(), e->stage.p + pieces[i].status, (size_t)n_cols * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
    for (int c = 0; c < n_cols; ++c) flags[(size_t)c] |= flag_part[(size_t)c] ? 1 : 0;
    return MHX_OK;
  };
  for (size_t i = 0; i < E; ++i)
    if ((rc = counts_of(i)) != MHX_OK) return give_up(rc);
  if (out)
    for (int k = 0; k < n_targets; ++k) out[k] = ensemble_value(targets[(size_t)k]);
  if (n_pooled) *n_pooled = pooled;
  if (n_used) std::copy(used.begin(), used.end(), n_used);
  if (status) std::copy(flags.begin(), flags.end(), status);
  return MHX_OK;
}
}  // extern "C++"

int mhx_get_ensemble_percentiles(mhx_engine* e, int take, const int32_t* cols, int n_cols, const uint8_t* include,
                                 const int32_t* pct_num, const int32_t* pct_den, int n_pct, double* out,
                                 int64_t* n_pooled, int32_t* n_used, int32_t* status) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  return ensemble_run({e}, nullptr, take, cols, n_cols, include, pct_num, pct_den, n_pct, out, n_pooled, n_used, status);
}
int mhx_ensemble_pick(const uint64_t* counts, int n_bins, int64_t rank, int32_t* digit, int64_t* rank_in_bin,
                      int64_t* bin_count) {
  if (!counts || n_bins < 1) return fail(MHX_EINVAL, "mhx_ensemble_pick: n_bins must be >= 1 and counts given");
  int32_t dg = 0;
  int64_t rb = 0, bc = 0;
  if (!ensemble_pick(counts, n_bins, rank, &dg, &rb, &bc))
    return fail(MHX_EINVAL, "mhx_ensemble_pick: rank %lld is outside [0, the sum of the counts)", (long long)rank);
  if (digit) *digit = dg;
  if (rank_in_bin) *rank_in_bin = rb;
  if (bin_count) *bin_count = bc;
  return MHX_OK;
}

// Split R-hat from the half moments of mhx_get_autocorr: host arithmetic only, every sum serial
// from its first term (include/mhx.h).
int mhx_split_rhat(const double* half_mean, const double* half_var, const int32_t* n_used, int64_t n_chains,
                   int n_cols, double* rhat) {
  if (!half_mean || !half_var || !n_used) return fail(MHX_EINVAL, "NULL argument");
  if (n_chains < 1) return fail(MHX_EINVAL, "n_chains must be >= 1");
  if (n_cols < 1) return fail(MHX_EINVAL, "n_cols must be >= 1");
  const int32_t h = n_used[0] / 2;
  if (n_used[0] < 0 || h < 2)
    return fail(MHX_EINVAL, "chain 0: a window of %d steps has halves of %d, fewer than 2", n_used[0], h);
  for (int64_t c = 1; c < n_chains; ++c)
    if (n_used[c] < 0 || n_used[c] / 2 != h)
      return fail(MHX_EINVAL, "chain %lld: a window of %d steps, halves of %d where chain 0 has %d",
                  (long long)c, n_used[c], n_used[c] / 2, h);
  if (!rhat) return MHX_OK;
  const int64_t M = 2 * n_chains;
  const size_t pitch = (size_t)n_cols * 2;
  const double shrink = (double)(h - 1) / (double)h;
  for (int k = 0; k < n_cols; ++k) {
    const double *mu = half_mean + (size_t)k * 2, *var = half_var + (size_t)k * 2;
    double sv = var[0], sm = mu[0];
    for (int64_t q = 1; q < M; ++q) {
      sv = sv + var[(size_t)(q / 2) * pitch + (size_t)(q % 2)];
      sm = sm + mu[(size_t)(q / 2) * pitch + (size_t)(q % 2)];
    }
    const double W = sv / (double)M, mean = sm / (double)M;
    double sb = (mu[0] - mean) * (mu[0] - mean);
    for (int64_t q = 1; q < M; ++q) {
      const double u = mu[(size_t)(q / 2) * pitch + (size_t)(q % 2)] - mean;
      sb = sb + u * u;
    }
    const double b_over_h = sb / (double)(M - 1);
    const double var_plus = shrink * W + b_over_h;
    rhat[k] = __builtin_sqrt(var_plus / W);
  }
  return MHX_OK;
}

int mhx_set_history(mhx_engine* e, int64_t chain, const double* prob, const double* theta, int n) {
  if (!e || !prob || !theta) return fail(MHX_EINVAL, "NULL argument");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (chain < 0 || chain >= e->cfg.n_chains) return fail(MHX_EINVAL, "chain out of range");
  if (n < 1) return fail(MHX_EINVAL, "a walk has at least one step");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const int Rcap = e->S.R, d = e->P.d;
  const int keep = std::min(n, Rcap);  // the ring holds the newest `keep` steps
  std::vector<double> hp((size_t)Rcap, 0.0), ht((size_t)Rcap * d, 0.0);
  // chronological order: step s (0 = newest) of the input is entry keep-1-s of the ring
  for (int s = 0; s < keep; ++s) {
    const int slot = keep - 1 - s;
    hp[(size_t)slot] = prob[s];
    memcpy(&ht[(size_t)slot * d], theta + (size_t)s * d, sizeof(double) * d);
  }
  // most-likely-step as :add-step would have left it (strictly greater wins, oldest first)
  int best = n - 1;
  for (int s = n - 2; s >= 0; --s)
    if (prob[s] > prob[best]) best = s;
  const int64_t nh = keep, len = keep, age = n;
  HIP_TRY(hipMemcpy(e->hist_prob.p + chain * Rcap, hp.data(), hp.size() * sizeof(double),
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->hist_theta.p + chain * Rcap * d, ht.data(), ht.size() * sizeof(double),
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->n_hist.p + chain, &nh, sizeof nh, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->length.p + chain, &len, sizeof len, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->age.p + chain, &age, sizeof age, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->theta.p + chain * d, theta, sizeof(double) * d, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->prob.p + chain, prob, sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->best_theta.p + chain * d, theta + (size_t)best * d, sizeof(double) * d,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->best_prob.p + chain, prob + best, sizeof(double), hipMemcpyHostToDevice));
  return MHX_OK;
}

int mhx_walker_modify(mhx_engine* e, int action, int64_t n) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (!e->chains_ready) return fail(MHX_ESTATE, "mhx_init_chains has not been called");
  if (action < MHX_MODIFY_BURN_WALKS || action > MHX_MODIFY_RESET_TO_MOST_LIKELY)
    return fail(MHX_EINVAL, "unknown walker-modify action %d", action);
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if (action <= MHX_MODIFY_KEEP_WALKS) {
    // (subseq walk 0 (- length burn-number)) / (subseq walk 0 keep-number), M:566-569: a bounding
    // index outside the list is an error in the reference; nothing is changed then
    std::vector<int64_t> len((size_t)e->cfg.n_chains);
    HIP_TRY(hipMemcpy(len.data(), e->length.p, len.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t v : len)
      if (n < 0 || n > v)
        return fail(MHX_EINVAL, "%s %lld is outside a walk of length %lld",
                    action == MHX_MODIFY_BURN_WALKS ? ":burn-number" : ":keep-number",
                    (long long)n, (long long)v);
  }
  HIP_TRY(e->fam->modify(e->stream, e->S, action, n));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->launches++;
  return MHX_OK;
}

int mhx_get_pooled(mhx_engine* e, double* stats, double* L_pool, int32_t* valid,
                   uint64_t* refreshes) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  const size_t d = (size_t)e->P.d, E = 1 + d + d * d;
  if (stats) HIP_TRY(hipMemcpy(stats, e->pool_vec.p, E * sizeof(double), hipMemcpyDeviceToHost));
  if (L_pool) HIP_TRY(hipMemcpy(L_pool, e->L_pool.p, d * d * sizeof(double), hipMemcpyDeviceToHost));
  if (valid) HIP_TRY(hipMemcpy(valid, e->pool_valid.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (refreshes) *refreshes = e->pool_refreshes;
  return MHX_OK;
}

int mhx_get_counters(mhx_engine* e, uint64_t* chain_steps, uint64_t* kernel_launches) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if (chain_steps) {
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, e->step_counter.p, sizeof v, hipMemcpyDeviceToHost));
    *chain_steps = v;
  }
  if (kernel_launches) *kernel_launches = e->launches;
  return MHX_OK;
}

const char* mhx_kernel_name(mhx_engine* e) {
  if (!e) {
    fail(MHX_EINVAL, "engine is NULL");
    return nullptr;
  }
  if (use_device(e) != MHX_OK || finalize_problem(e) != MHX_OK) return nullptr;
  return e->kernel_name.c_str();
}

// ---- native RCCL for one-process-per-GPU hosts -------------------------------------------------
int mhx_comm_get_unique_id(uint8_t id[128]) {
  if (!id) return fail(MHX_EINVAL, "id is NULL");
  Rccl& r = rccl();
  if (!r.ok) return fail(MHX_ECOMM, "RCCL unavailable: %s", g_rccl_why.c_str());
  nccl_unique_id u;
  const int rc = r.GetUniqueId(&u);
  if (rc != 0) return fail(MHX_ECOMM, "ncclGetUniqueId: %s", rccl_err(rc));
  memcpy(id, u.internal, 128);
  return MHX_OK;
}

int mhx_comm_init_rank(mhx_engine* e, const uint8_t id[128], int rank, int n_ranks) {
  if (!e || !id) return fail(MHX_EINVAL, "NULL argument");
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MHX_EINVAL, "rank %d of %d", rank, n_ranks);
  Rccl& r = rccl();
  if (!r.ok) return fail(MHX_ECOMM, "RCCL unavailable: %s", g_rccl_why.c_str());
  int rc = use_device(e);
  if (rc != MHX_OK) return rc;
  if (e->comm && e->comm_owned) (void)r.CommDestroy(e->comm);
  e->comm = nullptr;
  nccl_unique_id u;
  memcpy(u.internal, id, 128);
  const int nr = r.CommInitRank(&e->comm, n_ranks, u, rank);
  if (nr != 0) {
    e->comm = nullptr;
    return fail(MHX_ECOMM, "ncclCommInitRank: %s", rccl_err(nr));
  }
  e->comm_owned = true;
  return MHX_OK;
}

int mhx_kernel_timing(mhx_engine* e, int reset, double* avg_ms, uint64_t* launches,
                      double* total_ms) {
  if (!e) return fail(MHX_EINVAL, "engine is NULL");
  if (avg_ms) *avg_ms = e->timed_launches ? e->kernel_ms / (double)e->timed_launches : 0.0;
  if (launches) *launches = e->timed_launches;
  if (total_ms) *total_ms = e->kernel_ms;
  if (reset) {
    e->kernel_ms = 0.0;
    e->timed_launches = 0;
  }
  return MHX_OK;
}


// ---- several GPUs under ONE host process (the reference's own way of running many walkers is a
// list mapped in one image, M:1029-1033): one engine + stream per device, contiguous global chain
// ranges, launches enqueued on every device before any is waited for, and for the pooled
// covariance ONE ncclAllReduce per tick issued on the engines' streams inside ncclGroupStart/End.
struct mhx_group {
  std::vector<mhx_engine*> eng;
  std::vector<int64_t> first, count;
  bool rccl_comms = false;    // distinct devices: communicators from ncclCommInitAll
  DevBuf<double> local_sum;   // same-device groups (tests on one GPU): device-side sum buffer
  int64_t global_iter = 0;
};

namespace {
int group_fail_cleanup(mhx_group* g, int rc) {
  const std::string keep = g_err;
  mhx_group_destroy(g);
  g_err = keep;
  return rc;
}
// the engines of a group that share ONE device cannot use RCCL (a communicator wants distinct
// devices): their pool vectors are summed by the host through pinned copies.  Only the
// single-GPU rehearsal of the group code path runs through here.
int group_pool_sum_local(mhx_group* g) {
  const mhx_engine* e0 = g->eng[0];
  const size_t E = 1 + (size_t)e0->P.d + (size_t)e0->P.d * e0->P.d;
  std::vector<double> sum(E, 0.0), h(E);
  for (mhx_engine* e : g->eng) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(h.data(), e->pool_vec.p, E * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < E; ++i) sum[i] += h[i];  // rank order: reproducible
  }
  for (mhx_engine* e : g->eng) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(e->pool_vec.p, sum.data(), E * sizeof(double), hipMemcpyHostToDevice));
  }
  return MHX_OK;
}
int group_pool_tick(mhx_group* g) {
  int rc = MHX_OK;
  for (mhx_engine* e : g->eng) {
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = pool_enqueue_stats(e)) != MHX_OK) return rc;
  }
  if (g->eng.size() > 1 || g->rccl_comms) {
    if (g->rccl_comms) {
      // one collective per device, issued by this one thread: inside ncclGroupStart/End, each
      // call with ITS device current.  Whatever fails in between, the group is closed again
      // (an open group would swallow every later nccl call of the process).
      Rccl& r = rccl();
      int nr = r.GroupStart();
      if (nr != 0) return fail(MHX_ECOMM, "ncclGroupStart: %s", rccl_err(nr));
      for (mhx_engine* e : g->eng) {
        if (hipSetDevice(e->device) != hipSuccess) {
          rc = fail(MHX_EDEVICE, "hipSetDevice(%d) failed inside the collective group", e->device);
          break;
        }
        if ((rc = pool_enqueue_allreduce(e)) != MHX_OK) break;
      }
      const std::string keep = g_err;
      nr = r.GroupEnd();
      if (rc != MHX_OK) {
        g_err = keep;  // the first failure is the one reported
        return rc;
      }
      if (nr != 0) return fail(MHX_ECOMM, "ncclGroupEnd: %s", rccl_err(nr));
    } else if ((rc = group_pool_sum_local(g)) != MHX_OK) {
      return rc;
    }
  }
  for (mhx_engine* e : g->eng) {
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = pool_enqueue_factor(e)) != MHX_OK) return rc;
  }
  return MHX_OK;
}
// (see run_failed: after a failure inside a run no engine of the group may be advanced again)
int group_run_failed(mhx_group* g, int rc) {
  const std::string keep = g_err;
  for (mhx_engine* e : g->eng) {
    if (e->launch_open) (void)launch_steps_finish(e);
    drain(e);
    e->run_ready = false;
  }
  g_err = keep;
  return rc;
}
}  // namespace

int mhx_group_partition(int64_t n_chains, int n_parts, int part, int64_t* first, int64_t* count) {
  if (n_chains < 0 || n_parts < 1 || part < 0 || part >= n_parts || !first || !count)
    return fail(MHX_EINVAL, "mhx_group_partition: bad argument");
  const int64_t base = n_chains / n_parts, rem = n_chains % n_parts;
  *count = base + (part < rem ? 1 : 0);
  *first = base * part + std::min<int64_t>(part, rem);
  return MHX_OK;
}

int mhx_group_create(const mhx_config* cfg, const int32_t* devices, int n_devices,
                     mhx_group** out) {
  if (!cfg || !devices || !out) return fail(MHX_EINVAL, "NULL argument");
  *out = nullptr;
  if (n_devices < 1 || n_devices > 64) return fail(MHX_EINVAL, "n_devices must be in [1,64]");
  if (cfg->n_chains < n_devices) return fail(MHX_EINVAL, "fewer chains than devices");
  mhx_group* g = new (std::nothrow) mhx_group();
  if (!g) return fail(MHX_ENOMEM, "host allocation failed");
  bool distinct = true;
  for (int i = 0; i < n_devices; ++i)
    for (int j = 0; j < i; ++j) distinct = distinct && devices[i] != devices[j];
  for (int i = 0; i < n_devices; ++i) {
    mhx_config c = *cfg;
    int64_t first = 0, count = 0;
    (void)mhx_group_partition(cfg->n_chains, n_devices, i, &first, &count);
    c.n_chains = count;
    c.chain_offset = cfg->chain_offset + first;
    c.device = devices[i];
    mhx_engine* e = nullptr;
    const int rc = mhx_create(&c, &e);
    if (rc != MHX_OK) return group_fail_cleanup(g, rc);
    g->eng.push_back(e);
    g->first.push_back(first);
    g->count.push_back(count);
  }
  // MHX_GROUP_FORCE_RCCL=1 (tests, -DMHX_DEBUG_HOOKS builds only): engines that share a device
  // take the communicator branch too - only a stand-in librccl accepts that (tests/stub_rccl);
  // the real one wants one device per rank, which is why such groups otherwise sum through the
  // host (group_pool_sum_local) - and so does a group of ONE device, which the real librccl
  // does accept: ncclCommInitAll of one communicator, ncclGroupStart / ncclAllReduce /
  // ncclGroupEnd per tick, the calls a node with several GPUs makes, on the one GPU of a test box
#ifdef MHX_DEBUG_HOOKS
  const char* fr = getenv("MHX_GROUP_FORCE_RCCL");
  const bool force_rccl = fr && atoi(fr) != 0;
#else
  const bool force_rccl = false;
#endif
  if ((n_devices > 1 || force_rccl) && cfg->adapt_mode == MHX_ADAPT_POOLED &&
      (distinct || force_rccl)) {
    Rccl& r = rccl();
    if (!r.ok) return group_fail_cleanup(g, fail(MHX_ECOMM, "RCCL unavailable: %s", g_rccl_why.c_str()));
    std::vector<nccl_comm_t> comms((size_t)n_devices, nullptr);
    std::vector<int> devs(devices, devices + n_devices);
    const int nr = r.CommInitAll(comms.data(), n_devices, devs.data());
    if (nr != 0)
      return group_fail_cleanup(g, fail(MHX_ECOMM, "ncclCommInitAll: %s",
                                        rccl_err(nr)));
    for (int i = 0; i < n_devices; ++i) {
      g->eng[(size_t)i]->comm = comms[(size_t)i];
      g->eng[(size_t)i]->comm_owned = true;
    }
    g->rccl_comms = true;
  }
  *out = g;
  return MHX_OK;
}

void mhx_group_destroy(mhx_group* g) {
  if (!g) return;
  for (mhx_engine* e : g->eng) mhx_destroy(e);
  delete g;
}

int mhx_group_size(const mhx_group* g) { return g ? (int)g->eng.size() : 0; }

mhx_engine* mhx_group_engine(mhx_group* g, int i) {
  if (!g || i < 0 || i >= (int)g->eng.size()) {
    fail(MHX_EINVAL, "group / index");
    return nullptr;
  }
  return g->eng[(size_t)i];
}

int mhx_group_chain_range(const mhx_group* g, int i, int64_t* first, int64_t* count) {
  if (!g || i < 0 || i >= (int)g->eng.size()) return fail(MHX_EINVAL, "group / index");
  if (first) *first = g->first[(size_t)i];
  if (count) *count = g->count[(size_t)i];
  return MHX_OK;
}

#define MHX_GROUP_EACH(call)                       \
  do {                                             \
    if (!g) return fail(MHX_EINVAL, "group is NULL"); \
    for (mhx_engine* e : g->eng) {                 \
      const int rc_ = (call);                      \
      if (rc_ != MHX_OK) return rc_;               \
    }                                              \
    return MHX_OK;                                 \
  } while (0)

int mhx_group_set_function(mhx_group* g, int k, int model_id, const int32_t* shape, int n_shape,
                           const int32_t* param_index, int n_index) {
  MHX_GROUP_EACH(mhx_set_function(e, k, model_id, shape, n_shape, param_index, n_index));
}
int mhx_group_set_dataset(mhx_group* g, int k, const double* x, const double* y,
                          const double* sigma, size_t n, int likelihood) {
  MHX_GROUP_EACH(mhx_set_dataset(e, k, x, y, sigma, n, likelihood));  // replicated on every GPU
}
int mhx_group_set_dataset_planes(mhx_group* g, int k, const double* x, const double* y,
                                 const double* sigma, int sigma_kind, size_t n, int likelihood) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  if (n == 0 || !x || !y) return fail(MHX_EINVAL, "mhx_group_set_dataset_planes: n == 0 or x / y is NULL");
  for (size_t i = 0; i < g->eng.size(); ++i) {  // every member: the rows of its chain range
    const size_t first = (size_t)g->first[i];
    const double* sg = !sigma ? nullptr
                       : sigma_kind == MHX_SIGMA_PER_CHAIN ? sigma + first
                       : sigma_kind == MHX_SIGMA_PER_POINT ? sigma + first * n : sigma;
    const int rc = mhx_set_dataset_planes(g->eng[i], k, x, y + first * n, sg, sigma_kind, n, likelihood);
    if (rc != MHX_OK) return rc;
  }
  return MHX_OK;
}
int mhx_group_set_dataset_cols(mhx_group* g, int k, const double* const* xcols, int n_cols,
                               const double* y, const double* sigma, size_t n, int likelihood) {
  MHX_GROUP_EACH(mhx_set_dataset_cols(e, k, xcols, n_cols, y, sigma, n, likelihood));
}
int mhx_group_set_bounds(mhx_group* g, int k, const int32_t* idx, const double* lo,
                         const double* hi, int n) {
  MHX_GROUP_EACH(mhx_set_bounds(e, k, idx, lo, hi, n));
}
int mhx_group_set_function_expr(mhx_group* g, int k, const char* expr,
                                const char* const* param_names, const int32_t* param_index,
                                int n_index) {
  MHX_GROUP_EACH(mhx_set_function_expr(e, k, expr, param_names, param_index, n_index));
}
int mhx_group_set_expr_recognition(mhx_group* g, int on) {
  MHX_GROUP_EACH(mhx_set_expr_recognition(e, on));
}
int mhx_group_set_prior_expr(mhx_group* g, int k, const char* expr, const char* const* names,
                             const int32_t* index, int n) {
  MHX_GROUP_EACH(mhx_set_prior_expr(e, k, expr, names, index, n));
}
int mhx_group_set_likelihood_expr(mhx_group* g, int k, const char* expr) {
  MHX_GROUP_EACH(mhx_set_likelihood_expr(e, k, expr));
}
int mhx_group_request_stop(mhx_group* g) { MHX_GROUP_EACH(mhx_request_stop(e)); }

int mhx_group_init_chains(mhx_group* g, const double* theta0, int broadcast) {
  if (!g || !theta0) return fail(MHX_EINVAL, "NULL argument");
  // the first step of every chain (M:1148-1163) is a full log-posterior: enqueued on every
  // device before the first is waited for
  for (size_t i = 0; i < g->eng.size(); ++i) {
    mhx_engine* e = g->eng[i];
    const double* th = broadcast ? theta0 : theta0 + (size_t)g->first[i] * (size_t)e->P.d;
    const int rc = init_chains_enqueue(e, th, broadcast);
    if (rc != MHX_OK) {  // (what is already in the queues runs out; nobody is marked ready)
      for (size_t j = 0; j < i; ++j) drain(g->eng[j]);
      return rc;
    }
  }
  int rc = MHX_OK;
  for (mhx_engine* e : g->eng) {
    const int r = init_chains_finish(e);
    if (rc == MHX_OK) rc = r;
  }
  return rc;
}

int mhx_group_adaptive_begin(mhx_group* g, const mhx_run_opts* o) {
  if (!g || !o) return fail(MHX_EINVAL, "NULL argument");
  for (size_t i = 0; i < g->eng.size(); ++i) {
    mhx_run_opts oi = *o;
    if (o->l_matrix && o->l_matrix_per_chain)
      oi.l_matrix = o->l_matrix + (size_t)g->first[i] * (size_t)g->eng[i]->P.d * g->eng[i]->P.d;
    const int rc = adaptive_begin_enqueue(g->eng[i], &oi);
    if (rc != MHX_OK) {
      for (size_t j = 0; j < i; ++j) drain(g->eng[j]);
      return rc;
    }
  }
  int rc = MHX_OK;
  for (mhx_engine* e : g->eng) {
    const int r = adaptive_begin_finish(e);
    if (rc == MHX_OK) rc = r;
  }
  if (rc != MHX_OK)
    for (mhx_engine* e : g->eng) e->run_ready = false;
  g->global_iter = 0;
  return rc;
}

int mhx_group_adaptive_advance(mhx_group* g, int64_t max_iters, int64_t* n_running) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  if (max_iters < 0) return fail(MHX_EINVAL, "max_iters < 0");
  for (mhx_engine* e : g->eng)
    if (!e->run_ready) return fail(MHX_ESTATE, "mhx_group_adaptive_begin has not been called");
  const bool pooled = g->eng[0]->cfg.adapt_mode == MHX_ADAPT_POOLED;
  int rc = MHX_OK;
  auto count_all = [&](int64_t* total) -> int {
    *total = 0;
    for (mhx_engine* e : g->eng) {
      int64_t r = 0;
      int rc2 = use_device(e);
      if (rc2 == MHX_OK) rc2 = count_running(e, &r);
      if (rc2 != MHX_OK) return rc2;
      *total += r;
    }
    return MHX_OK;
  };
  int64_t left = max_iters;
  while (left > 0) {
    const int64_t now = pooled ? std::min<int64_t>(left, 200 - (g->global_iter % 200))
                               : std::min<int64_t>(left, kTempsWindow);
    for (mhx_engine* e : g->eng) {  // every GPU gets its launch before any is waited for
      if ((rc = use_device(e)) != MHX_OK) return group_run_failed(g, rc);
      if ((rc = launch_steps_enqueue(e, now, 0)) != MHX_OK) return group_run_failed(g, rc);
    }
    for (mhx_engine* e : g->eng)
      if ((rc = launch_steps_finish(e)) != MHX_OK) return group_run_failed(g, rc);
    g->global_iter += now;
    left -= now;
    if (pooled && g->global_iter % 200 == 0 && (rc = group_pool_tick(g)) != MHX_OK)
      return group_run_failed(g, rc);
    if (left > 0 && (!pooled || g->global_iter % 200 == 0)) {  // "until done": look at the chains
      int64_t total = 0;
      if ((rc = count_all(&total)) != MHX_OK) return group_run_failed(g, rc);
      if (total == 0) break;
    }
  }
  if (n_running && (rc = count_all(n_running)) != MHX_OK) return group_run_failed(g, rc);
  return MHX_OK;
}

int mhx_group_adaptive_steps_full(mhx_group* g, const mhx_run_opts* o) {
  int rc = mhx_group_adaptive_begin(g, o);
  if (rc != MHX_OK) return rc;
  int64_t running = 1;
  while (running > 0) {
    int64_t chunk = 1 << 16;
    for (mhx_engine* e : g->eng) chunk = std::min(chunk, e->chunk_iters);
    if ((rc = mhx_group_adaptive_advance(g, chunk, &running)) != MHX_OK) return rc;
  }
  return MHX_OK;
}

int mhx_group_get_state(mhx_group* g, double* theta, double* logpost, double* best_theta,
                        double* best_logpost, int64_t* length, int64_t* age) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  for (size_t i = 0; i < g->eng.size(); ++i) {
    mhx_engine* e = g->eng[i];
    const size_t f = (size_t)g->first[i], d = (size_t)e->P.d;
    const int rc = mhx_get_state(e, theta ? theta + f * d : nullptr, logpost ? logpost + f : nullptr,
                                 best_theta ? best_theta + f * d : nullptr,
                                 best_logpost ? best_logpost + f : nullptr,
                                 length ? length + f : nullptr, age ? age + f : nullptr);
    if (rc != MHX_OK) return rc;
  }
  return MHX_OK;
}

int mhx_group_get_counters(mhx_group* g, uint64_t* chain_steps, uint64_t* kernel_launches) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  uint64_t cs = 0, kl = 0;
  for (mhx_engine* e : g->eng) {
    uint64_t a = 0, b = 0;
    const int rc = mhx_get_counters(e, &a, &b);
    if (rc != MHX_OK) return rc;
    cs += a;
    kl += b;
  }
  if (chain_steps) *chain_steps = cs;
  if (kernel_launches) *kernel_launches = kl;
  return MHX_OK;
}

// the batched read-outs over a group: engine i's results land at its first global chain
extern "C++" {
template <class Q>
static int run_portions(mhx_group* g, const Q& q) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  return run_portions(g->eng, g->first.data(), q);
}
}
int mhx_group_get_percentiles(mhx_group* g, int take, const int32_t* pct_num,
                              const int32_t* pct_den, int n_pct, double* out, int32_t* n_used) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  SummaryCall q(SUM_PERCENTILES, take, out, nullptr, n_used, nullptr);
  int rc = MHX_OK;
  for (mhx_engine* e : g->eng)
    if ((rc = window_check(e, take)) != MHX_OK) return rc;
  if ((rc = fill_pcts(&q.pc, pct_num, pct_den, n_pct)) != MHX_OK) return rc;
  if (n_pct == 0) return MHX_OK;
  return run_portions(g, q);
}
int mhx_group_get_covariances(mhx_group* g, int take, double* cov, int32_t* n_unique,
                              int32_t* status) {
  return run_portions(g, SummaryCall(SUM_COVARIANCES, take, cov, nullptr, n_unique, status));
}
int mhx_group_get_proposal_factors(mhx_group* g, int take, double* L, int32_t* status,
                                   int32_t* n_forward) {
  return run_portions(g, SummaryCall(SUM_FACTORS, take, L, nullptr, status, n_forward));
}
int mhx_group_get_window_best(mhx_group* g, int take, double* prob, double* theta) {
  return run_portions(g, SummaryCall(SUM_BEST, take, prob, theta, nullptr, nullptr));
}

int mhx_group_get_fit_bands(mhx_group* g, int fn, int take, const double* xcols, int n_cols,
                            int64_t m, double* ymax, double* ymin, int32_t* n_selected,
                            int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  if (m < 1) return fail(MHX_EINVAL, "m must be >= 1");
  return run_portions(g, FitCall(fn, take, -1, nullptr, xcols, n_cols, m, ymax, ymin, n_selected, status));
}

int mhx_group_get_fit_percentiles(mhx_group* g, int fn, int take, const double* xcols, int n_cols, int64_t m,
                                  const int32_t* pct_num, const int32_t* pct_den, int n_pct, double* pct,
                                  double* mean, double* stddev, int32_t* n_used, int32_t* status) {
  FitPctCall q(fn, take, xcols, n_cols, m, pct, mean, stddev, n_used, status);
  if (!g || g->eng.empty()) return fail(MHX_EINVAL, "group is NULL");
  int rc = window_check(g->eng[0], take);
  if (rc != MHX_OK || (rc = fill_pcts(&q.pc, pct_num, pct_den, n_pct)) != MHX_OK) return rc;
  return run_portions(g, q);
}
int mhx_group_get_waic(mhx_group* g, int fn, int take, double* elpd, double* lppd, double* p_waic,
                       int32_t* n_high, double* pw_lppd, double* pw_p, double* pw_acc,
                       int32_t* n_used, int32_t* status) {
  return run_portions(g, WaicCall(fn, take, elpd, lppd, p_waic, n_high, pw_lppd, pw_p, pw_acc, n_used, status));
}
int mhx_group_get_heldout(mhx_group* g, int fn, int take, const double* xcols, int n_cols, int64_t m,
                          const double* y, int y_per_chain, const double* sigma, int sigma_kind,
                          const uint8_t* use, int use_per_chain, double* lpd, int32_t* n_scored,
                          double* pw_lpd, double* pw_acc, int32_t* n_used, int32_t* status) {
  if (!g || g->eng.empty()) return fail(MHX_EINVAL, "group is NULL");
  HeldoutCall q(fn, take, xcols, n_cols, m, y, y_per_chain, sigma, sigma_kind, use, use_per_chain, lpd, n_scored,
                pw_lpd, pw_acc, n_used, status);
  int64_t n_total = 0;
  for (const mhx_engine* e : g->eng) n_total += e->cfg.n_chains;
  int rc = window_check(g->eng[0], take);
  if (rc != MHX_OK || (rc = q.check_data(g->eng[0], n_total)) != MHX_OK) return rc;
  return run_portions(g, q);  // (the per-chain arrays move to each engine's first global chain with the outputs)
}
int mhx_group_get_loo(mhx_group* g, int fn, int take, int tail_len, double k_limit, double* elpd_loo,
                      double* p_loo, double* lppd, int32_t* n_high, int32_t* n_used, int32_t* status,
                      double* pw_elpd, double* pw_khat, double* pw_lppd, double* pw_acc, double* tail) {
  return run_portions(g, LooCall(fn, take, tail_len, k_limit, elpd_loo, p_loo, lppd, n_high, n_used, status,
                                 pw_elpd, pw_khat, pw_lppd, pw_acc, tail));
}

int mhx_group_get_residuals(mhx_group* g, int fn, const double* theta, double z_limit, double* fit,
                            double* z, double* chi2, double* sum_z, double* dw, double* max_abs_z,
                            int64_t* max_index, int32_t* n_pos, int32_t* n_runs, int32_t* n_out,
                            int32_t* status) {
  return run_portions(g, ResidCall(fn, theta, z_limit, fit, z, chi2, sum_z, dw, max_abs_z, max_index, n_pos,
                                   n_runs, n_out, status));
}

int mhx_group_get_normal_equations(mhx_group* g, int fn, const double* theta, const double* steps,
                                   int per_chain_steps, double* jtj, double* jtr, double* chi2,
                                   double* g_out, int32_t* status) {
  int64_t n_all = 0;
  if (g)
    for (int64_t c : g->count) n_all += c;
  return run_portions(g, NormEqCall(n_all, fn, theta, steps, per_chain_steps, jtj, jtr, chi2, g_out, status));
}

int mhx_group_get_candidate_scores(mhx_group* g, int fn, const double* cand, int64_t m, int per_chain,
                                   int keep, double* score, int32_t* best_index, double* best_score,
                                   int32_t* n_bad) {
  return run_portions(g, CandCall(fn, cand, m, per_chain, keep, score, best_index, best_score, n_bad));
}

int mhx_group_get_traces(mhx_group* g, int take, int filter, int stride, int start, const int32_t* cols,
                         int n_cols, int max_out, double* values, double* lo, double* hi, int32_t* n_out,
                         int32_t* n_kept, int32_t* n_used) {
  return run_portions(g, TraceCall(take, filter, stride, start, cols, n_cols, max_out, values, lo, hi, n_out,
                                   n_kept, n_used));
}

int mhx_group_get_derived(mhx_group* g, const char* const* exprs, int n_expr,
                          const char* const* names, const int32_t* index, int n_names, int take,
                          const int32_t* pct_num, const int32_t* pct_den, int n_pct,
                          double* at_most_likely, double* pct, double* mean, double* stddev,
                          double* values, int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  DerivedCall q;
  const int rc = q.prepare(exprs, n_expr, names, index, n_names, take, pct_num, pct_den, n_pct,
                           at_most_likely, pct, mean, stddev, values, n_used, status);
  return rc != MHX_OK ? rc : run_portions(g, q);
}

int mhx_group_get_histograms(mhx_group* g, int take, const int32_t* cols, int n_cols, int n_bins,
                             const double* edges, int edges_per_chain, int32_t* counts,
                             int32_t* outside, int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  HistoCall q;
  const int rc = q.prepare(g->eng, take, cols, n_cols, n_bins, edges, edges_per_chain, counts, outside, n_used, status);
  return rc != MHX_OK ? rc : run_portions(g, q);
}
int mhx_group_get_pair_grids(mhx_group* g, int take, const int32_t* cols, int n_cols,
                             const int32_t* pair_a, const int32_t* pair_b, int n_pairs, int n_bins,
                             const double* edges, int edges_per_chain, int32_t* counts,
                             int32_t* n_inside, int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  GridCall q;
  const int rc = q.prepare(g->eng, take, cols, n_cols, pair_a, pair_b, n_pairs, n_bins, edges, edges_per_chain,
                           counts, n_inside, n_used, status);
  return rc != MHX_OK ? rc : run_portions(g, q);
}

int mhx_group_get_autocorr(mhx_group* g, int take, const int32_t* cols, int n_cols, int max_lag, double* tau,
                           double* ess, double* acf, double* half_mean, double* half_var, int32_t* n_lags,
                           int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  AutocorrCall q;
  const int rc = q.prepare(g->eng, take, cols, n_cols, max_lag, tau, ess, acf, half_mean, half_var, n_lags, n_used, status);
  return rc != MHX_OK ? rc : run_portions(g, q);
}

int mhx_group_get_hdi(mhx_group* g, int take, const int32_t* cols, int n_cols, const int32_t* mass_num,
                      const int32_t* mass_den, int n_mass, int n_ladder, double* lo, double* hi, int32_t* pos,
                      double* ladder, int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  return hdi_run(g->eng, g->first.data(), take, cols, n_cols, mass_num, mass_den, n_mass, n_ladder, lo, hi, pos,
                 ladder, n_used, status);
}
int mhx_group_get_derived_hdi(mhx_group* g, const char* const* exprs, int n_expr, const char* const* names,
                              const int32_t* index, int n_names, int take, const int32_t* mass_num,
                              const int32_t* mass_den, int n_mass, int n_ladder, double* lo, double* hi,
                              int32_t* pos, double* ladder, int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  return derived_hdi_run(g->eng, g->first.data(), exprs, n_expr, names, index, n_names, take, mass_num, mass_den,
                         n_mass, n_ladder, lo, hi, pos, ladder, n_used, status);
}

int mhx_group_get_ensemble_percentiles(mhx_group* g, int take, const int32_t* cols, int n_cols,
                                       const uint8_t* include, const int32_t* pct_num, const int32_t* pct_den,
                                       int n_pct, double* out, int64_t* n_pooled, int32_t* n_used, int32_t* status) {
  if (!g) return fail(MHX_EINVAL, "group is NULL");
  return ensemble_run(g->eng, g->first.data(), take, cols, n_cols, include, pct_num, pct_den, n_pct, out, n_pooled,
                      n_used, status);
}

}  // extern "C"
