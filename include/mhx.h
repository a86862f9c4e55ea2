/*
 * mhx.h -- C ABI of libmhx, the MI355X-native batched Metropolis-Hastings engine.
 *
 * This is the drop-in boundary for ONE path of afranson/Lisp-MCMC: everything
 * `walker-adaptive-steps` does per step, batched over many independent walkers
 * ("chains").  The reference has no FFI of its own (it is 100 % Common Lisp); the
 * boundary is the exported Lisp surface listed below, and each entry point here
 * names the reference function(s) whose work it takes over.  Citations are
 * file:line under the reference checkout, `M:` = mcmc-fitting.lisp.
 *
 *   walker-create              M:1132-1163   -> mhx_create + mhx_set_function /
 *                                               mhx_set_dataset / mhx_set_bounds +
 *                                               mhx_init_chains
 *   walker-make-step           M:1067-1070   -> mhx_logpost
 *   walker-take-step           M:1072-1095   -> mhx_take_step (Philox z,u), mhx_step_injected
 *                                               (caller's z,u) and the body of
 *                                               mhx_adaptive_advance
 *   walker-adaptive-steps-full M:862-942     -> mhx_adaptive_begin / _advance / _steps_full
 *   walker-adaptive-steps      M:946-947     -> mhx_adaptive_steps
 *   walker-many-steps          M:849-853     -> mhx_many_steps
 *   walker-get                 M:487-543     -> mhx_get_state / _acceptance / _lmatrix /
 *                                               _trace / _proposal_factor
 *   walker-set-get             M:1029-1030   -> mhx_get_percentiles / _covariances /
 *                                               _proposal_factors / _window_best (every
 *                                               chain in one launch), mhx_group_get_*
 *   nth-percentile             M:1495-1506   -> mhx_percentile_rank (the position rule)
 *   walker-get-data-and-fit    M:1230-1255   -> mhx_eval_function, mhx_get_fit_bands,
 *                                               mhx_band_count, mhx_group_get_fit_bands
 *   walker-param-histo         M:1361-1369   -> mhx_get_histograms (make-histo M:1541-1564 as
 *   walker-plot-corner         M:1333-1359   -> mhx_get_pair_grids   counts over given edges)
 *   (no counterpart: the reference judges convergence by eye, walker-catepillar-plots
 *    M:1294-1310)                           -> mhx_get_autocorr, mhx_split_rhat
 *   walker-with-exp            M:1052-1064   -> mhx_get_derived, mhx_group_get_derived (the
 *                                               expression at every step, and its posterior)
 *   walker-modify              M:547-580     -> mhx_walker_modify (+ mhx_set_history)
 *   create-log-liklihood-function M:402-416  -> mhx_set_likelihood_expr
 *   prior-bounds-let           M:346-369     -> mhx_set_bounds (+ mhx_set_prior_expr)
 *   mfit-walker-estop          M:860-861     -> mhx_request_stop
 *   a list of walkers mapped in one image (M:1029-1033, nv-specific.lisp:58-66)
 *                                            -> mhx_group_* : one host process, several GPUs
 *
 * Conventions: every function returns MHX_OK (0) or a negative MHX_E* code and never
 * throws; the message of the last failure on the calling thread is available from
 * mhx_last_error().  All arrays are caller-allocated, caller-owned, dense row-major
 * IEEE binary64 / int32 HOST buffers; the engine owns its device memory and copies
 * in/out synchronously.  One handle is not thread-safe (the reference is single
 * threaded); distinct handles are independent.  No torch / C++ types appear here.
 */
#ifndef MHX_H
#define MHX_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#else /* hiprtc (run-time compiled expression kernels): no libc headers, built-in types */
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
using __hip_internal::uint8_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MHX_VERSION 200 /* 0.2.0 */

/* ---- limits ------------------------------------------------------------ */
#define MHX_MAX_PARAMS 63    /* d: length of the shared parameter vector (one lane of the
                                chain's wavefront per parameter, lane 63 draws the accept
                                uniform)                                              */
#define MHX_MAX_FUNCTIONS 16 /* K: functions / datasets of one (global) fit         */
#define MHX_MAX_FN_PARAMS 32 /* parameters one function gathers from the vector      */
#define MHX_MAX_BOUNDS 64    /* bounds in one prior-bounds-let block                */
#define MHX_MAX_PERCENTILES 16 /* percentiles one mhx_get_percentiles call may ask for */
#define MHX_MAX_DERIVED 16   /* expressions one mhx_get_derived call may evaluate        */
#define MHX_MAX_HISTO_BINS 1024 /* bins of one column of mhx_get_histograms               */
#define MHX_MAX_GRID_BINS 64 /* bins a side of one mhx_get_pair_grids grid               */
#define MHX_MAX_GRID_PAIRS 4096 /* pairs one mhx_get_pair_grids call may count            */
#define MHX_MAX_AUTOCORR_LAG 1023 /* greatest lag of one mhx_get_autocorr call              */
#define MHX_MAX_HDI_MASSES 8 /* masses one mhx_get_hdi call may ask for                   */
#define MHX_MAX_HDI_LADDER 4096 /* ranks of one column's quantile ladder (mhx_get_hdi)    */

/* ---- status codes ------------------------------------------------------ */
enum {
  MHX_OK = 0,
  MHX_EINVAL = -1,   /* bad argument (message says which)                          */
  MHX_ENOMEM = -2,   /* host or device allocation failed                           */
  MHX_EDEVICE = -3,  /* a HIP call failed / no usable gfx950 device                */
  MHX_ESTATE = -4,   /* call out of order (e.g. stepping before mhx_init_chains)   */
  MHX_EUNSUPPORTED = -5,
  MHX_ECOMM = -6     /* collective hook failed                                     */
};

/* ---- model designators ----------------------------------------------------
 * The reference's :function is a Lisp closure (lambda (x &key ... &allow-other-keys))
 * (M:1134-1137) that cannot cross to the GPU; the boundary takes an enumerated device
 * model plus an index map into the shared parameter vector (global fits share
 * parameters through one plist, README "Global Parameter Fitting").  Local parameter j
 * of function k is theta[param_index[j]].  `shape` carries the model's integer shape.
 *
 *  POLY          p = n_index;            f = c0 + c1 x + ... (Horner)
 *  GAUSS_PEAKS   shape = {nbg, npk};     f = bg(x) + sum_p A_p exp(-((x-mu_p)/w_p)^2)
 *                local order: bg_0..bg_{nbg-1}, then (A, mu, w) per peak
 *  LORENTZ_PEAKS shape = {nbg, npk};     f = bg(x) + sum_p A_p / (1 + ((x-mu_p)/w_p)^2)
 *  LORDER_MIXED  6 params scale, linewidth, x0, mix, bg0, bg1 (test.lisp:16-17 names)
 *                u=(x-x0)/linewidth; f = scale*(cos(mix)*(-2u) + sin(mix)*(1-u^2))/(1+u^2)^2
 *                                        + bg0 + bg1*x
 *  EXP_DECAY     3 params A, tau, c;     f = A exp(-x/tau) + c
 *  SINUSOID      4 params A, omega, phi, c;  f = A sin(omega x + phi) + c
 *  PVOIGT2       11 params A, b0, b1, mu1, w1, eta1, mu2, w2, eta2, rho, c2
 *                pv(x;mu,w,eta) = eta/(1+u^2) + (1-eta) exp(-u^2), u=(x-mu)/w
 *                f = b0 + b1 x + c2 x^2 + A (pv1 + rho pv2)
 */
enum {
  MHX_MODEL_POLY = 0,
  MHX_MODEL_GAUSS_PEAKS = 1,
  MHX_MODEL_LORENTZ_PEAKS = 2,
  MHX_MODEL_LORDER_MIXED = 3,
  MHX_MODEL_EXP_DECAY = 4,
  MHX_MODEL_SINUSOID = 5,
  MHX_MODEL_PVOIGT2 = 6,
  MHX_MODEL_EXPR = 7, /* set by mhx_set_function_expr, never passed to mhx_set_function */
  MHX_MODEL__COUNT = 8
};

/* ---- likelihood kinds (what the reference's :log-liklihood closure computes) */
enum {
  MHX_LIK_NORMAL = 0,        /* log-liklihood-normal (+ README weighted form) M:393-400 */
  MHX_LIK_NORMAL_CUTOFF = 1, /* log-liklihood-normal-cutoff, each term >= -5000 M:419-427 */
  MHX_LIK_POISSON = 2,       /* log-poisson over points, M:379-383 via M:402-416      */
  MHX_LIK_EXPR = 3           /* create-log-liklihood-function M:402-416: the per-point term
                                is the expression given to mhx_set_likelihood_expr       */
};

/* ---- adaptation modes --------------------------------------------------- */
enum {
  MHX_ADAPT_FAITHFUL = 0, /* per-walker rule of M:888-942, no collective              */
  MHX_ADAPT_POOLED = 1    /* extension: forward-step displacement statistics pooled
                             over all chains (and ranks) every 200 steps              */
};

/* ---- per-chain status (mhx_get_chain_status) ----------------------------- */
enum {
  MHX_CHAIN_RUNNING = 0,
  MHX_CHAIN_DONE = 1,          /* loop index reached n (M:904)                        */
  MHX_CHAIN_FP_TRAP = 2,       /* reference would have signalled an unhandled float
                                  trap (invalid/overflow outside the handler-case of
                                  M:891-894): the walker is frozen where it stood     */
  MHX_CHAIN_STOPPED = 3        /* mfit-walker-estop seen                              */
};

typedef struct mhx_engine mhx_engine;

/* Engine-wide configuration.  Zero-initialise, then set fields; 0 means "default". */
typedef struct mhx_config {
  int64_t n_chains;        /* walkers on THIS engine (one engine per GPU/rank)        */
  int32_t n_params;        /* d                                                        */
  int32_t n_functions;     /* K (1 for an ordinary fit)                                */
  int32_t device;          /* HIP device ordinal                                        */
  int32_t adapt_mode;      /* MHX_ADAPT_*                                               */
  uint64_t seed;           /* Philox key                                                */
  int64_t chain_offset;    /* global id of local chain 0 (multi-GPU sharding): the
                              Philox counter uses global ids, so results do not
                              depend on how chains are partitioned                      */
  int32_t history_capacity;/* steps of (prob, theta) kept per chain (ring).  0 ->
                              1024 = enough for every window the controller reads
                              (acceptance 1000, settle 10*max(50,d)); the reference
                              keeps everything (M:549) - set >= n to do the same       */
  int32_t poisson_logfact_double; /* 0: log-factorial summed in single floats as
                              M:379-380 does; 1: lgamma in binary64                    */
} mhx_config;

/* Options of one walker-adaptive-steps-full call (M:862).  Defaults of the Lisp
 * lambda list are applied by mhx_run_opts_default(). */
typedef struct mhx_run_opts {
  int64_t n;               /* :n, default 100000 (walker-adaptive-steps passes 30000)  */
  double temperature;      /* :temperature, default 1d3 (walker-adaptive-steps: 10)    */
  int32_t auto_mode;       /* :auto  0 = nil, 1 = :prob-settle (:slope-settle is
                              outside the path)                             */
  int64_t max_walker_length; /* :max-walker-length, 0 = nil                            */
  const double* l_matrix;  /* :l-matrix, d*d row-major, NULL = nil                     */
  int32_t l_matrix_per_chain; /* 1: l_matrix holds n_chains matrices                   */
} mhx_run_opts;

/* Collective hook for MHX_ADAPT_POOLED on several ranks: sum `n` doubles in place
 * over all ranks.  `buf` is a DEVICE pointer when device_buffer != 0 (RCCL path),
 * else a host pointer.  Return 0 on success. */
typedef int (*mhx_allreduce_fn)(void* ctx, double* buf, size_t n, int device_buffer);

/* ---- lifecycle ----------------------------------------------------------- */
int mhx_version(void);
/* Which sources this binary was built from: "csrc:<16 hex digits>", the leading digits of the
 * SHA-256 over the library's sources in a fixed order (csrc/Makefile: SRC_ID).  bench.py and
 * tools/profile_summary.py store it next to every measurement, so that an instruction count
 * taken from a committed rocprof summary is only ever combined with the binary that produced it. */
const char* mhx_build_id(void);
const char* mhx_last_error(void);
int mhx_device_count(int* count);
int mhx_create(const mhx_config* cfg, mhx_engine** out);
void mhx_destroy(mhx_engine* e);

/* ---- problem definition (walker-create, M:1132-1163) ---------------------- */
/* Function k: device model + gather map (param_index[j] in [0,d) ).               */
int mhx_set_function(mhx_engine* e, int k, int model_id, const int32_t* shape, int n_shape,
                     const int32_t* param_index, int n_index);
/* Dataset k in the layout clean-data/clean-data-error produce (M:774-825): x, y and a
 * per-point sigma (sigma == NULL -> 1.0 everywhere, the (or data-error 1) of M:1144).
 * The engine copies.  For MHX_LIK_POISSON y holds the counts k_i and sigma is ignored. */
int mhx_set_dataset(mhx_engine* e, int k, const double* x, const double* y,
                    const double* sigma, size_t n, int likelihood);
/* The same with a VECTOR-VALUED x: "multiple or linked independent variables" - the reference
 * hands each element of the x list to the function as it is (M:400), and a closure reads its
 * components with (elt x 0), (elt x 1) (M:1136-1137).  xcols[j][i] = component j of point i,
 * n_cols 1 or 2.  Component 0 is the x of every enumerated model and of the windows' ranges;
 * an expression function names the components xcol0 (= x) and xcol1.  Not with
 * MHX_LIK_NORMAL_CUTOFF (MHX_EUNSUPPORTED). */
int mhx_set_dataset_cols(mhx_engine* e, int k, const double* const* xcols, int n_cols,
                         const double* y, const double* sigma, size_t n, int likelihood);
/* A DATASET PER WALKER (nv-specific.lisp:5-10, 50-66: one walker per column of a file, all on the
 * same frequency sweep): walker c of the engine fits (x, y[c], sigma of c) with function k.
 * y is [n_chains][n] row-major; sigma_kind says what `sigma` holds (below).  The engine copies and
 * prepares each walker's values exactly as mhx_set_dataset prepares a shared dataset: y/sigma and
 * 1/sigma by the same host divisions, the constant sum_i(-1/2 log 2pi - log sigma_i) in the same
 * order - one constant per walker.
 *   THE SUM, stated once for every kernel, family, slot and form:  the walker's arrays are padded
 *   to a multiple of 128 points with (x_last, 0, 0).  Lane l of the walker's wave takes points
 *   l, l + 64, l + 128, ... in that order; the even blocks of 64 go into one accumulator, the odd
 *   ones into a second, each point as  r = fma(-f(x), 1/sigma, y/sigma), acc = fma(r, r, acc)
 *   (the (y/sigma - f(x)/sigma)^2 of mhx_set_dataset), f by the model's guarded direct form - what
 *   mhx_eval_function evaluates: no fast path, no uniform-grid recurrence, no peak skipping; the
 *   two accumulators are added, the 64 lanes by the engine's butterfly, and the result is
 *   fma(-1/2, sum, the walker's constant).  A walker's bits depend on its own data, parameters and
 *   draws only - not on the other walkers of the launch, nor on whether the planes sit in LDS
 *   (where a workgroup's share fits the tile buffers: csrc/mhx_plan.hpp, planes_resident) or are
 *   streamed from memory (MHX_PLANES_NO_LDS=1: always).
 * Randomness, controller and history are those of a shared dataset: walker c does what the
 * reference would do with walker c's data alone.
 * MHX_LIK_NORMAL and one column of x only: the other likelihoods are refused here, a problem that
 * also uses two columns of x (mhx_set_dataset_cols) and MHX_ADAPT_POOLED (one pooled covariance
 * assumes one posterior) here or when the problem is finalised, all with MHX_EUNSUPPORTED.  n == 0,
 * a NULL x or y, or an unknown sigma_kind: MHX_EINVAL.  Functions set this way and with
 * mhx_set_dataset may be mixed in one global fit; a later mhx_set_dataset* call for the same k
 * replaces this one.  Such a problem always runs in kernels compiled at run time (hiprtc; without
 * it: MHX_EUNSUPPORTED with hiprtc's message) and in the batch form.
 * mhx_logpost on such an engine: row i of theta is evaluated on the data of walker
 * i mod n_chains.  mhx_eval_function, mhx_get_fit_bands and the read-outs of the history are
 * unchanged: they read the model, the shared x and the ring only. */
enum {
  MHX_SIGMA_NONE = 0,      /* sigma == NULL: 1.0 everywhere (M:1144)                  */
  MHX_SIGMA_SHARED = 1,    /* sigma[n]: one per point, the same for every walker       */
  MHX_SIGMA_PER_CHAIN = 2, /* sigma[n_chains]: one scalar per walker (nv-data-std-dev) */
  MHX_SIGMA_PER_POINT = 3  /* sigma[n_chains][n]                                       */
};
int mhx_set_dataset_planes(mhx_engine* e, int k, const double* x, const double* y,
                           const double* sigma, int sigma_kind, size_t n, int likelihood);
/* prior-bounds-let block of function k (M:346-369): idx[i] < 0 means "key absent from
 * the plist" (getf default 0d0, M:353).  n == 0 -> log-prior-flat (M:340-343). */
int mhx_set_bounds(mhx_engine* e, int k, const int32_t* idx, const double* lo,
                   const double* hi, int n);
/* Function k given as an EXPRESSION: what a host shim makes of the body
 * of (lambda (x &key a b &allow-other-keys) <body>) (M:1134-1137).  `expr` is a C-syntax
 * arithmetic expression over `x` (with a vector-valued x, mhx_set_dataset_cols: `xcol0`, `xcol1`), the
 * identifiers in param_names (local parameter j =
 * theta[param_index[j]]), numeric literals, + - * / ?: < <= > >= == != && || !, and the
 * functions exp log sqrt sin cos tan atan tanh abs pow min max floor, and ipow(u, n) (n an
 * integer: SBCL's order of multiplications for (expt u n)).  It is compiled for gfx950
 * with hiprtc into the same fused kernels when the problem is finalised (first
 * mhx_init_chains / mhx_logpost), and evaluated without contraction.  Accuracy: exp and log
 * < 1 ulp (exp: inf above ln(DBL_MAX), 0 below the underflow, NaN for NaN and +-inf; log:
 * finite on positive subnormals, NaN for x <= 0, +inf and NaN); sqrt abs floor min max exact; a
 * quotient by a divisor that does not depend on x is a * (1/b), within 1.5 ulp - inf where 1/b
 * overflows (|b| < 2^-1024), fewer bits where 1/b is subnormal (|b| > 2^1022) - unless
 * MHX_EXPR_EXACT_DIV=1, which keeps IEEE divisions.
 * A body that IS one of the enumerated models - a polynomial background c0 + c1 x + ... plus
 * Gaussian peaks a * exp(-ipow((x - mu) / w, 2)) or Lorentzian peaks a / (1 + ipow((x - mu) / w,
 * 2)) over distinct parameters (pow(u, 2.0), u * u and -1 * S are understood; csrc/mhx_expr.cpp) -
 * is recognised here, below the ABI, and runs as MHX_MODEL_POLY / _GAUSS_PEAKS / _LORENTZ_PEAKS
 * with the gather map permuted into that model's order: the same function through the peak
 * kernels' fused arithmetic (a few ulp per point from the text's own rounding, inside the path's
 * tolerance), with their per-window peak skipping and uniform-grid recurrence - the lambda a
 * Lisp host hands to walker-create gets the kernels of BASELINE's config 2 without knowing
 * them.  A function whose likelihood is MHX_LIK_EXPR always stays an expression. */
int mhx_set_function_expr(mhx_engine* e, int k, const char* expr, const char* const* param_names,
                          const int32_t* param_index, int n_index);
/* on = 0: every expression of this engine is compiled exactly as written (default: on). */
int mhx_set_expr_recognition(mhx_engine* e, int on);
/* What mhx_set_function_expr makes of `expr` - needs no engine and no device (hosts' logs, tests):
 * *model = the MHX_MODEL_* that serves it (MHX_MODEL_EXPR: compiled as written), shape[2] its
 * {nbg, npk}, order[j] = which of param_names is local parameter j of that model (*n_order
 * entries, at most n_names; 0 for MHX_MODEL_EXPR).  shape, order, n_order may be NULL. */
int mhx_expr_classify(const char* expr, const char* const* param_names, int n_names,
                      int32_t* model, int32_t* shape, int32_t* order, int32_t* n_order);
/* Body of function k's prior-bounds-let prior (M:366-369) as an expression over
 * `bounds_total` (the sum of the block set by mhx_set_bounds) and the identifiers in `names`
 * (names[i] = theta[index[i]]), e.g. NV's "bounds_total + (mu1 > mu2 ? -1e9 : 0.0)". */
int mhx_set_prior_expr(mhx_engine* e, int k, const char* expr, const char* const* names,
                       const int32_t* index, int n);
/* Per-point log-likelihood of function k as an expression: the closure handed to
 * create-log-liklihood-function (M:402-416), (lambda (y model error) <body>), with `y` the
 * measured value, `model` the model's prediction at that x and `error` the point's sigma as
 * its docstring defines them (the reference's code passes the WHOLE stddev list as the third
 * argument, M:415, so only bodies that ignore `error` ever ran there).  The log-likelihood is
 * the plain sum of the terms over the points.  Dataset k must have been set with
 * MHX_LIK_EXPR (x, y, sigma are kept as given) and function k with mhx_set_function_expr. */
int mhx_set_likelihood_expr(mhx_engine* e, int k, const char* expr);
/* First step of every chain (M:1148-1150): theta0 is [n_chains][d], or [d] when
 * broadcast != 0.  Resets history, age, length, most-likely step. */
int mhx_init_chains(mhx_engine* e, const double* theta0, int broadcast);

/* ---- pure evaluation / injected-randomness parity hooks -------------------- */
/* walker-make-step's prob for n arbitrary parameter vectors theta[n][d] (M:1067-1070).
 * parts (optional, [n][2]) receives the likelihood sum and the prior sum. */
int mhx_logpost(mhx_engine* e, const double* theta, size_t n, double* out, double* parts);
/* One walker-take-step per chain (M:1072-1095) with the caller's randomness:
 * L  [d][d] (per_chain_l == 0) or [n_chains][d][d];  z [n_chains][d] standard normals
 * (what alexandria:gaussian-random would have returned, M:687);  u [n_chains] the
 * (random 1.0d0) of M:1092;  T [n_chains] temperatures.  accepted_out (optional)
 * receives 1 where the proposal was taken. */
int mhx_step_injected(mhx_engine* e, const double* L, int per_chain_l, const double* z,
                      const double* u, const double* T, uint8_t* accepted_out);

/* ---- the controller (walker-adaptive-steps-full, M:862-942) ---------------- */
void mhx_run_opts_default(mhx_run_opts* o);
/* Everything before the do loop: schedule, steps-to-settle, initial L (M:866-901). */
int mhx_adaptive_begin(mhx_engine* e, const mhx_run_opts* o);
/* Run up to max_iters iterations of the do loop (M:902-942) for every chain that is
 * still running; *n_running (optional) receives how many chains have not finished.
 * (Asking for n_running lets the engine look at the chain states: between launches it deals
 * the chains still walking evenly over the GPU's workgroups - a chain's results do not depend
 * on where it runs; MHX_NO_COMPACT=1 keeps every chain in its first place.) */
int mhx_adaptive_advance(mhx_engine* e, int64_t max_iters, int64_t* n_running);
/* begin + advance until every chain is done or mhx_request_stop was called. */
int mhx_adaptive_steps_full(mhx_engine* e, const mhx_run_opts* o);
/* (walker-adaptive-steps w n): n, :temperature 10, :auto :prob-settle (M:946-947). */
int mhx_adaptive_steps(mhx_engine* e, int64_t n);
/* walker-many-steps (M:849-853): n steps with a constant L, temperature 1.  The nil default
 * of M:851, diag(1e-2 * median-params), is formed by the host shims (mhx_get_trace); pass L. */
int mhx_many_steps(mhx_engine* e, int64_t n, const double* L, int per_chain_l);
/* (walker-take-step w :l-matrix L :temperature T) for every chain (M:1072-1095): ONE step with
 * the device's own randomness (Philox, the next draw of each chain).  The nil default of
 * M:1074, diag(1e-2 * most-likely-params of the newest 1000 steps), is the shims' to form. */
int mhx_take_step(mhx_engine* e, const double* L, int per_chain_l, double temperature);
int mhx_request_stop(mhx_engine* e);

/* Multi-rank pooled adaptation through a caller-supplied sum (MPI, a test stub ...): installs the
 * all-reduce used every adaptation tick.  The native path is RCCL: mhx_comm_init_rank (one
 * process per GPU) or mhx_group_create (one process, several GPUs) below.  A hook installed
 * AFTER mhx_comm_init_rank replaces that communicator (it is destroyed): every rank must then
 * exchange through its hook. */
int mhx_set_allreduce(mhx_engine* e, mhx_allreduce_fn fn, void* ctx, int wants_device_buffer);

/* ---- native RCCL (librccl.so is loaded on first use; MHX_ECOMM when it is absent) ----------
 * One process per GPU: rank 0 calls mhx_comm_get_unique_id and hands the 128 bytes to the other
 * ranks by whatever channel the host has (a file, MPI, torch.distributed ...); then EVERY rank
 * calls mhx_comm_init_rank on its engine (collective: ncclCommInitRank).  From then on the
 * pooled tick of MHX_ADAPT_POOLED is k_pool_stats -> k_pool_reduce -> ncclAllReduce(1+d+d*d
 * doubles, sum) -> k_pool_factor, all on the engine's stream with no host synchronisation. */
int mhx_comm_get_unique_id(uint8_t id[128]);
int mhx_comm_init_rank(mhx_engine* e, const uint8_t id[128], int rank, int n_ranks);

/* ---- one host process, several GPUs ---------------------------------------------------------
 * The reference runs many walkers as a list mapped in ONE Lisp image (M:1029-1033); a group is
 * that list spread over GPUs: cfg->n_chains walkers in all, contiguous global id ranges per
 * device (mhx_group_partition; Philox counters use global ids, so the walks do not depend on the
 * number of devices), one engine + one HIP stream per device, datasets replicated.  Every
 * group call enqueues its launches on ALL devices before it waits for any.  With
 * MHX_ADAPT_POOLED and more than one device the communicators come from ncclCommInitAll and the
 * tick's all-reduce is issued for all devices inside ncclGroupStart/End.  (Engines of a group
 * that name the SAME device - a rehearsal on one GPU - sum their statistics through the host.)
 * cfg->device is ignored; cfg->chain_offset is the global id of the group's first chain.
 * mhx_group_engine(g, i) exposes engine i to every per-engine entry point above (read-backs of
 * one walker, mhx_logpost ...); problem definition goes through the mhx_group_set_* twins. */
typedef struct mhx_group mhx_group;
int mhx_group_partition(int64_t n_chains, int n_parts, int part, int64_t* first, int64_t* count);
int mhx_group_create(const mhx_config* cfg, const int32_t* devices, int n_devices,
                     mhx_group** out);
void mhx_group_destroy(mhx_group* g);
int mhx_group_size(const mhx_group* g);
mhx_engine* mhx_group_engine(mhx_group* g, int i);
int mhx_group_chain_range(const mhx_group* g, int i, int64_t* first, int64_t* count);
int mhx_group_set_function(mhx_group* g, int k, int model_id, const int32_t* shape, int n_shape,
                           const int32_t* param_index, int n_index);
int mhx_group_set_dataset(mhx_group* g, int k, const double* x, const double* y,
                          const double* sigma, size_t n, int likelihood);
/* (y and a per-walker sigma cover ALL chains of the group: every member engine gets the rows of
 * its chain range, mhx_group_chain_range) */
int mhx_group_set_dataset_planes(mhx_group* g, int k, const double* x, const double* y,
                                 const double* sigma, int sigma_kind, size_t n, int likelihood);
int mhx_group_set_dataset_cols(mhx_group* g, int k, const double* const* xcols, int n_cols,
                               const double* y, const double* sigma, size_t n, int likelihood);
int mhx_group_set_bounds(mhx_group* g, int k, const int32_t* idx, const double* lo,
                         const double* hi, int n);
int mhx_group_set_function_expr(mhx_group* g, int k, const char* expr,
                                const char* const* param_names, const int32_t* param_index,
                                int n_index);
int mhx_group_set_expr_recognition(mhx_group* g, int on);
int mhx_group_set_prior_expr(mhx_group* g, int k, const char* expr, const char* const* names,
                             const int32_t* index, int n);
int mhx_group_set_likelihood_expr(mhx_group* g, int k, const char* expr);
/* theta0: [cfg->n_chains][d] in global chain order, or [d] when broadcast != 0 */
int mhx_group_init_chains(mhx_group* g, const double* theta0, int broadcast);
int mhx_group_adaptive_begin(mhx_group* g, const mhx_run_opts* o);
int mhx_group_adaptive_advance(mhx_group* g, int64_t max_iters, int64_t* n_running);
int mhx_group_adaptive_steps_full(mhx_group* g, const mhx_run_opts* o);
int mhx_group_request_stop(mhx_group* g);
/* gathered in global chain order; any pointer may be NULL */
int mhx_group_get_state(mhx_group* g, double* theta, double* logpost, double* best_theta,
                        double* best_logpost, int64_t* length, int64_t* age);
int mhx_group_get_counters(mhx_group* g, uint64_t* chain_steps, uint64_t* kernel_launches);

/* ---- read-back (walker-get, M:487-543) ------------------------------------ */
/* Any pointer may be NULL.  theta/best_theta [n_chains][d]; others [n_chains]. */
int mhx_get_state(mhx_engine* e, double* theta, double* logpost, double* best_theta,
                  double* best_logpost, int64_t* length, int64_t* age);
/* The same for ONE chain (what the accessors of one walker need: walker-last-step,
 * walker-most-likely-step, walker-length, walker-age): d doubles instead of n_chains * d. */
int mhx_get_chain(mhx_engine* e, int64_t chain, double* theta, double* logpost,
                  double* best_theta, double* best_logpost, int64_t* length, int64_t* age);
int mhx_get_chain_status(mhx_engine* e, int32_t* status, int64_t* loop_index);
int mhx_get_lmatrix(mhx_engine* e, double* L /* [n_chains][d][d] */);
int mhx_get_temperature(mhx_engine* e, double* T /* [n_chains] */);
/* (walker-get w :get :acceptance :take take) for every chain, as a double. */
int mhx_get_acceptance(mhx_engine* e, int take, double* out);
/* Newest-first steps of one chain, as (walker-get w :get :steps :take take):
 * prob[take], theta[take][d]; *n_out = steps actually available. */
int mhx_get_trace(mhx_engine* e, int64_t chain, int take, double* prob, double* theta,
                  int* n_out);
/* (walker-get w :get :l-matrix :take take) of one chain recomputed on the host from the
 * device trace: status 0 ok, 1 caught error (type-error/div0/overflow -> fallback in
 * M:891-894), 2 uncaught invalid-operation.  n_forward = (length :forward-steps). */
int mhx_get_proposal_factor(mhx_engine* e, int64_t chain, int take, double* L_out,
                            int* status, int* n_forward);

/* ---- walker-set-get (M:1029-1030): summaries of EVERY chain in one launch ----
 * What (mapcar (lambda (w) (walker-get w :get ... :take take)) walkers) computes, on the
 * device ring, without moving any history to the host.  n_chains = the engine's chains; take in
 * [1, history_capacity] as for mhx_get_proposal_factor; every chain's window is its newest
 * min(take, walker-length, steps the ring holds) steps; any output pointer may be NULL;
 * MHX_ESTATE before mhx_init_chains.  The chains are worked through in portions whose device
 * scratch stays below 64 MiB whatever n_chains and take are.  A chain in MHX_CHAIN_FP_TRAP is
 * summarised from the history it has. */

/* The position rule of nth-percentile (M:1495-1506) for the n = num/den per cent point of len
 * sorted values: q = num (len-1) / (100 den) as an exact rational, *pos = floor(q), *between =
 * 1 when q has a fractional part (the percentile is then the mean of elements pos and pos+1).
 * For integer n (the median's 50) this is the reference's own arithmetic; for 2.5 / 84.1 / 97.5
 * the reference multiplies single-floats, and the rational reading is this project's
 * definition.  Host only: needs no engine and no device.  MHX_EINVAL unless len >= 1,
 * den >= 1, 0 <= num <= 100 den. */
int mhx_percentile_rank(int64_t len, int32_t num, int32_t den, int64_t* pos, int32_t* between);
/* out[n_chains][n_pct][d]: for percentile q = pct_num[q]/pct_den[q] per cent and parameter p the
 * value nth-percentile gives on parameter p's column of the chain's window: the element at pos
 * of the ascending sort, or (e[pos] + e[pos+1]) / 2 (IEEE) when between.  :median-params is
 * 50/1, `95cr` 5/2 and 195/2, `iqr` 25/1 and 75/1, `standard-deviation-normal` 841/10.  Exact
 * for any take (selection on the device; no sort, no window size limit).  -0 sorts before +0
 * (they compare equal: either may be returned); a NaN sorts last, whatever its sign.
 * n_used[n_chains]: steps the window held (< min(take, walker-length): the ring had wrapped).
 * 0 <= n_pct <= MHX_MAX_PERCENTILES; n_pct = 0 writes nothing. */
int mhx_get_percentiles(mhx_engine* e, int take, const int32_t* pct_num, const int32_t* pct_den,
                        int n_pct, double* out, int32_t* n_used);
/* (walker-get w :get :covariance-matrix :take take) M:541 = lplist-covariance (M:614-643) of
 * :unique-steps (M:492-496): cov[n_chains][d][d].  Unique steps: those whose prob differs IN
 * BITS from the next older step's, the oldest of the window always kept (n_unique[n_chains]).
 * Averages (/ (reduce #'+ x) n), then every entry the serial sum over the unique steps, newest
 * first, of (x_i - avg_i)(x_j - avg_j) / n, the division inside the sum, no fused multiply-add.
 * status[n_chains]: 0 ok, 1 an average or an entry is not finite (a trapped overflow in the
 * reference). */
int mhx_get_covariances(mhx_engine* e, int take, double* cov, int32_t* n_unique, int32_t* status);
/* mhx_get_proposal_factor for every chain (:l-matrix M:543; :stddev-params M:525-539 is its
 * diagonal): L[n_chains][d][d], status[n_chains] (0 ok, 1 caught, 2 invalid operation, 3 a
 * single forward step: the reference's empty matrix), n_forward[n_chains] - the same device
 * code, the same bits. */
int mhx_get_proposal_factors(mhx_engine* e, int take, double* L, int32_t* status,
                             int32_t* n_forward);
/* (walker-get w :get :most-likely-step :take take) M:503-505: the step of greatest prob in the
 * window, among equal greatest probs the OLDEST (the reduce keeps the older unless the newer
 * is strictly greater): prob[n_chains], theta[n_chains][d]. */
int mhx_get_window_best(mhx_engine* e, int take, double* prob, double* theta);
/* Steps the device history ring of every chain holds: the greatest `take` (the power of two
 * not below mhx_config.history_capacity and the adaptation window). */
int mhx_get_history_capacity(mhx_engine* e, int32_t* capacity);
/* HIP-event milliseconds the kernels of the engine's last mhx_get_percentiles / _covariances /
 * _proposal_factors / _window_best / _fit_bands / _derived / _histograms / _pair_grids / _waic /
 * _loo / _heldout / _traces / _fit_percentiles / _residuals / _normal_equations / _candidate_scores or
 * mhx_eval_function call ran (all portions; copies excluded). */
int mhx_get_summary_timing(mhx_engine* e, double* kernel_ms);
/* The same for a group, gathered in global chain order like mhx_group_get_state; every
 * device's launch is enqueued before any is waited for. */
int mhx_group_get_percentiles(mhx_group* g, int take, const int32_t* pct_num,
                              const int32_t* pct_den, int n_pct, double* out, int32_t* n_used);
int mhx_group_get_covariances(mhx_group* g, int take, double* cov, int32_t* n_unique,
                              int32_t* status);
int mhx_group_get_proposal_factors(mhx_group* g, int take, double* L, int32_t* status,
                                   int32_t* n_forward);
int mhx_group_get_window_best(mhx_group* g, int take, double* prob, double* theta);

/* ---- walker-get-data-and-fit (M:1230-1255), its -no-stddev sibling (M:1208-1227) and
 * walker-plot-residuals (M:1271-1283) without the plotting: the model's VALUES and the envelope
 * of the model over the most probable two thirds of the walk, computed on the device. */

/* (ceiling (* 0.66 take)) M:1250, the steps the envelope is taken over.  0.66 is read as a
 * SINGLE float and the integer is coerced to single: the product is rounded to binary32 before
 * the ceiling (150 -> 100, 300 -> 199, 1000 -> 660).  Host only: needs no engine and no device.
 * MHX_EINVAL unless take >= 1. */
int mhx_band_count(int64_t take, int64_t* k);
/* out[n][m]: function fn of the finalised problem at the m points xcols[0 .. n_cols)[m] (column
 * after column) for each of the n FULL parameter vectors theta[n][d]; the function's gather map
 * is applied as in the sweep.  n_cols must be the columns of x the function reads (2 for an
 * expression model that names xcol1, else 1).  xcols == NULL: the function's own dataset x, which
 * is on the device already; m must then be its point count (pads are not included).  Every value
 * is the model's direct form at that x: no likelihood, no prior, no recurrence, no tile
 * skipping.  Accuracy, per value: within 1e-12 * sum |terms| of the reference's formula (the terms:
 * the background's monomials and the peaks, in absolute value) PLUS THE ARGUMENT TERM of the models
 * that form their argument otherwise than the reference does.  Peaks (Gaussian, Lorentzian,
 * pseudo-Voigt): t = fma(x, iw, c) with c = fl(-mu * iw) is the reference's (x - mu) / w at a centre
 * moved by at most delta = |mu| * 2^-53 - half an ulp of mu -, so a value differs by at most
 * 2 * sum_k |A_k| * |dg_k/dx| * delta_k more (|dg/dx| = 2 |u| / |w| * g for a Gaussian,
 * 2 |u| / |w| / (1 + u^2)^2 for a Lorentzian, u = (x - mu) / w; the factor 2 stands for iw's own
 * rounding and the final rounding of t).  Nothing near the origin; up to 8e-12 of a peak's height
 * at x ~ mu ~ 2000, w = 0.05 (1.72 * |mu| / |w| * 2^-53, on the flanks).  The sweep's uniform-grid recurrence adds the grid's tolerated departure,
 * 8 ulp of the window's max |x|, to delta.  Sinusoid: |A| * (|om x| + |ph|) * 2^-53 (also doubled);
 * exp-decay: |x / tau| * 2^-52 relative on the exponential.  Polynomials, MHX_MODEL_LORDER_MIXED and
 * expression models form their arguments as the reference does: 1e-12 * sum |terms| alone.  Centre x
 * (subtract a constant near the peaks from x and from the centres) when |mu| / w is beyond about 1e4.
 * Serves every model the engine can walk (ahead-of-time kernels, the generic one,
 * run-time compiled expression and specialised problems).  Worked through in portions whose
 * device scratch stays below 64 MiB whatever n and m are.  mhx_get_summary_timing covers it. */
int mhx_eval_function(mhx_engine* e, int fn, const double* theta, int64_t n, const double* xcols,
                      int n_cols, int64_t m, double* out);
/* For every chain c, ymax[n_chains][m] and ymin[n_chains][m]: M:1249-1253 on the device ring, no
 * history crossing to the host.  take_c = min(take, walker-length_c); the candidates are ALL the
 * steps the ring holds (the reference sorts the whole walk - only the COUNT comes from take);
 * k_c = min(mhx_band_count(take_c), steps held) of them are selected: those of greatest prob,
 * among equal probs (-0 = +0) the newer first, a NaN prob last.  ymax / ymin are the greatest /
 * smallest model value over the selected steps at each x: the very bits mhx_eval_function
 * returns for those parameter vectors.  n_selected[c] = k_c; status[c] = 1 when a selected value
 * is not finite (the reference would have trapped; that chain's band is unspecified), else 0.
 * xcols, n_cols, m as for mhx_eval_function.  take in [1, history_capacity]; any output may be
 * NULL; MHX_ESTATE before mhx_init_chains. */
int mhx_get_fit_bands(mhx_engine* e, int fn, int take, const double* xcols, int n_cols, int64_t m,
                      double* ymax, double* ymin, int32_t* n_selected, int32_t* status);
/* The same for a group, in global chain order; every device's launch is enqueued before any is
 * waited for. */
int mhx_group_get_fit_bands(mhx_group* g, int fn, int take, const double* xcols, int n_cols,
                            int64_t m, double* ymax, double* ymin, int32_t* n_selected,
                            int32_t* status);

/* ---- walker-with-exp (M:1052-1064) and the posterior of the expression -----------------------
 * The reference substitutes a walker's most-likely parameters into an expression and evaluates
 * it: a peak area, a width, a ratio.  Here the n_expr expressions g_q are evaluated at EVERY step
 * of every chain's window, on the device ring, and summarised there, so the quantity comes with
 * its error bar.  exprs[q]: C syntax, the grammar of mhx_set_prior_expr - the identifiers in
 * names (names[i] = theta[index[i]]), literals, the operators and functions listed at
 * mhx_set_function_expr - plus `prob`, the step's log-posterior.  x, xcol0, xcol1, bounds_total
 * and any unknown identifier: MHX_EINVAL, mhx_last_error names the identifier.  Evaluated without
 * contraction with the engine's exp / log (< 1 ulp; MHX_EXPR_OCML_MATH=1: ocml's); every division
 * is IEEE (a step is evaluated once: there is no reciprocal to hoist, MHX_EXPR_EXACT_DIV plays no
 * part).  The expressions are compiled with hiprtc into a module of their own, kept - per process
 * and on disk, as the expression models are - under the prepared texts and names: the same texts
 * a second time compile nothing.
 * The window is mhx_get_percentiles': the newest min(take, walker-length, steps held) steps,
 * n_used[n_chains] as there; take in [1, history_capacity]; n_expr in [1, MHX_MAX_DERIVED];
 * 0 <= n_pct <= MHX_MAX_PERCENTILES; any output may be NULL; MHX_ESTATE before mhx_init_chains; a
 * chain in MHX_CHAIN_FP_TRAP is summarised from the history it has.
 *   values[n_chains][n_expr][take]  values[c][q][s] = g_q at the step s-th from newest; entries
 *                                   with s >= n_used[c] are not written
 *   at_most_likely[n_chains][n_expr] g_q at the chain's most-likely step, the walker's own
 *                                   (:most-likely-params M:511-515; mhx_get_state's best_theta,
 *                                   `prob` = best_logpost) whatever take is: walker-with-exp
 *   pct[n_chains][n_pct][n_expr]    nth-percentile (M:1495-1506) of the window's values: the rank
 *                                   rule of mhx_percentile_rank, the order of mhx_get_percentiles
 *                                   (a NaN last, -0 / +0 interchangeable); an element of the
 *                                   ascending order or the IEEE mean of two neighbours
 *   mean[n_chains][n_expr]          M:1518-1519: the serial sum newest first, one division
 *   stddev[n_chains][n_expr]        standard-deviation M:1521-1527: the serial sum newest first of
 *                                   (v - mean) * (v - mean), / (n - 1), sqrt.  With ONE step this
 *                                   is the IEEE 0/0: a NaN (the reference divides by zero)
 *   status[n_chains][n_expr]        1: a value of the window is not finite (the reference would
 *                                   have trapped), else 0
 * Worked through in portions whose device scratch stays below 64 MiB; mhx_get_summary_timing
 * covers the call. */
int mhx_get_derived(mhx_engine* e, const char* const* exprs, int n_expr, const char* const* names,
                    const int32_t* index, int n_names, int take, const int32_t* pct_num,
                    const int32_t* pct_den, int n_pct, double* at_most_likely, double* pct,
                    double* mean, double* stddev, double* values, int32_t* n_used,
                    int32_t* status);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_derived(mhx_group* g, const char* const* exprs, int n_expr,
                          const char* const* names, const int32_t* index, int n_names, int take,
                          const int32_t* pct_num, const int32_t* pct_den, int n_pct,
                          double* at_most_likely, double* pct, double* mean, double* stddev,
                          double* values, int32_t* n_used, int32_t* status);

/* ---- walker-param-histo (M:1361-1369) and walker-plot-corner (M:1333-1359) as counts ---------
 * The reference bins one parameter of one walk (make-histo M:1541-1557) and scatters every step
 * of every parameter pair.  Here every chain's window is counted on the device ring over edges
 * the CALLER supplies, and only integers come back: 20 per parameter instead of the trace, a grid
 * of pair counts instead of the scatter.  The device forms no edge and adds no floating-point
 * number, so the counts are exact whatever the order of its threads.
 * The bin rule, make-histo's: with the edges b_0 <= b_1 <= ... <= b_B of a column, a value v
 * falls in bin n = the smallest n in 1..B with v <= b_n.  A value equal to b_0 lies in bin 1;
 * with all edges equal bin 1 holds every value equal to them; v < b_0 counts as `below`, v > b_B
 * as `above` (make-histo's own edges - (linspace bottom top :len B+1), exact rationals coerced to
 * double - can leave the greatest value above b_B: the reference drops it, here it is counted);
 * a NaN is counted nowhere and sets the column's status; +-inf follow the comparisons.
 * The window is mhx_get_percentiles': the newest min(take, walker-length, steps held) steps,
 * n_used[n_chains] as there; take in [1, history_capacity]; any output may be NULL; MHX_ESTATE
 * before mhx_init_chains; a chain in MHX_CHAIN_FP_TRAP is served from the history it has.
 *   cols[n_cols]   distinct parameter indices in [0, d), 1 <= n_cols <= d, in any order
 *   edges          [n_cols][n_bins + 1] when edges_per_chain == 0: one set for every chain (the
 *                  histograms of a walker set are then comparable), or
 *                  [n_chains][n_cols][n_bins + 1] when edges_per_chain == 1.  Every row free of
 *                  NaN and non-decreasing, else MHX_EINVAL (mhx_last_error names the chain and
 *                  the column) and nothing is launched
 *   n_bins         in [1, MHX_MAX_HISTO_BINS]
 *   counts[n_chains][n_cols][n_bins]   counts[c][k][n-1] = values of column k in bin n
 *   outside[n_chains][n_cols][2]       (below, above): the counts and these sum to n_used[c]
 *                                      unless the column held a NaN
 *   status[n_chains][n_cols]           1: the column held a NaN, else 0
 * Worked through in portions whose device scratch stays below 64 MiB whatever the call's size;
 * mhx_get_summary_timing covers the call. */
int mhx_get_histograms(mhx_engine* e, int take, const int32_t* cols, int n_cols, int n_bins,
                       const double* edges, int edges_per_chain, int32_t* counts,
                       int32_t* outside, int32_t* n_used, int32_t* status);
/* The joint counts of parameter pairs over the same edges, bin rule and window.  pair_a[q] and
 * pair_b[q] are two distinct places in cols; any list of 0 <= n_pairs <= MHX_MAX_GRID_PAIRS
 * pairs; n_bins in [1, MHX_MAX_GRID_BINS].
 *   counts[n_chains][n_pairs][n_bins][n_bins]  cell [i][j] of pair q: the steps whose
 *                                      cols[pair_a[q]] value lies in bin i+1 and whose
 *                                      cols[pair_b[q]] value lies in bin j+1
 *   n_inside[n_chains][n_pairs]        the steps with both values in a bin (the cells' sum)
 *   status[n_chains][n_pairs]          1: either column held a NaN, else 0
 * A call whose pieces for ONE chain (n_pairs n_bins^2 counts and the rest) exceed the 64 MiB of a
 * portion is refused with MHX_EINVAL; nothing is allocated for it. */
int mhx_get_pair_grids(mhx_engine* e, int take, const int32_t* cols, int n_cols,
                       const int32_t* pair_a, const int32_t* pair_b, int n_pairs, int n_bins,
                       const double* edges, int edges_per_chain, int32_t* counts,
                       int32_t* n_inside, int32_t* n_used, int32_t* status);
/* The same for a group, in global chain order (per-chain edges too); every device's work is
 * enqueued before any is waited for. */
int mhx_group_get_histograms(mhx_group* g, int take, const int32_t* cols, int n_cols, int n_bins,
                             const double* edges, int edges_per_chain, int32_t* counts,
                             int32_t* outside, int32_t* n_used, int32_t* status);
int mhx_group_get_pair_grids(mhx_group* g, int take, const int32_t* cols, int n_cols,
                             const int32_t* pair_a, const int32_t* pair_b, int n_pairs, int n_bins,
                             const double* edges, int edges_per_chain, int32_t* counts,
                             int32_t* n_inside, int32_t* n_used, int32_t* status);

/* ---- how much the windows are worth: autocorrelation time, effective sample size and the half
 * moments of split R-hat, of every chain and every requested parameter in ONE device launch.  The
 * reference has no such function (its convergence checks are plots): the definitions are this
 * library's own and fix the results to the last bit - plain IEEE binary64 operations in the order
 * stated, no fused multiply-add, nothing clamped.
 * The window is mhx_get_percentiles': the newest t = min(take, walker-length, steps held) steps
 * x_0 (newest) ... x_{t-1} of column p, n_used[c] = t.
 *   m      = (x_0 + x_1 + ... + x_{t-1}) / t       the serial sum newest first, one division
 *   dev_s  = x_s - m
 *   L      = min(max_lag, t - 1)                   n_lags[c]
 *   c_k    = (sum_{s = 0}^{t-1-k} dev_s dev_{s+k}) / t   for k = 0 .. L: every product rounded,
 *            added serially in ascending s to a sum that starts at 0.0, one division
 *   rho_k  = c_k / c_0                             acf[c][k][0 .. L]
 *   P_j    = rho_{2j} + rho_{2j+1}                 for every j with 2j + 1 <= L
 *   S      = P_0 + P_1 + ...  serially from 0.0, ending before the first P_j for which P_j > 0 is
 *            false (a NaN ends it too): Geyer's initial positive sequence
 *   tau    = 2 S - 1,  ess = t / tau               (a two-step window: tau = 0, ess = +inf)
 * status[c][k], a sum of
 *   MHX_AUTOCORR_NONFINITE  a value of the column's window is not finite: the column's numbers
 *                           and its other bits are unspecified (other columns and chains are not
 *                           touched by it)
 *   MHX_AUTOCORR_CONSTANT   c_0 == 0 - one step, or a chain that never moved in the window: the
 *                           rho are the IEEE 0/0, and tau is rho_0 (that NaN) in place of 2 S - 1,
 *                           so that tau and ess are NaN
 *   MHX_AUTOCORR_OPEN       the lags ran out before any P_j ended the sum: max_lag was too small
 *                           for this chain and tau is a lower bound.  (A one-step window has no
 *                           P_j at all: CONSTANT and OPEN.)
 * The halves of split R-hat: h = floor(t / 2); half 0 holds x_0 .. x_{h-1} (the newer steps),
 * half 1 x_{t-h} .. x_{t-1} (the older; for odd t the middle step belongs to neither).
 *   half_mean[c][k][2]  the serial sum newest first / h
 *   half_var[c][k][2]   the serial sum newest first of (x - half_mean) (x - half_mean), / (h - 1)
 *                       (h = 1: the IEEE 0/0, as mhx_get_derived's standard deviation of one
 *                       step); with h = 0 neither is written
 * Arguments: cols[n_cols] distinct parameter indices in [0, d), 1 <= n_cols <= d, in any order;
 * max_lag in [1, MHX_MAX_AUTOCORR_LAG]; take in [1, history_capacity].  tau, ess, status
 * [n_chains][n_cols]; acf [n_chains][n_cols][max_lag + 1], entries beyond n_lags[c] are not
 * written; n_lags, n_used [n_chains].  Any output may be NULL.  MHX_ESTATE before
 * mhx_init_chains; a chain in MHX_CHAIN_FP_TRAP is served from the history it has.  Worked
 * through in portions whose device scratch stays below 64 MiB; mhx_get_summary_timing covers the
 * call. */
enum {
  MHX_AUTOCORR_NONFINITE = 1,
  MHX_AUTOCORR_CONSTANT = 2,
  MHX_AUTOCORR_OPEN = 4
};
int mhx_get_autocorr(mhx_engine* e, int take, const int32_t* cols, int n_cols, int max_lag,
                     double* tau, double* ess, double* acf, double* half_mean,
                     double* half_var, int32_t* n_lags, int32_t* n_used, int32_t* status);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_autocorr(mhx_group* g, int take, const int32_t* cols, int n_cols, int max_lag,
                           double* tau, double* ess, double* acf, double* half_mean,
                           double* half_var, int32_t* n_lags, int32_t* n_used, int32_t* status);
/* Split R-hat of every column from the half moments exactly as mhx_get_autocorr fills them.  Host
 * only: needs no engine and no device.  For one column, over the M = 2 n_chains sequences in the
 * order chain 0 half 0, chain 0 half 1, chain 1 half 0, ...:
 *   W        = (the serial sum of the variances) / M
 *   mu       = (the serial sum of the means) / M
 *   B_over_h = (the serial sum of (mu_i - mu) (mu_i - mu)) / (M - 1)
 *   var_plus = ((h - 1) / h) W + B_over_h           (h - 1) / h one double division
 *   rhat[k]  = sqrt(var_plus / W)                   (W = 0 follows IEEE)
 * every sum from its first term.  MHX_EINVAL - mhx_last_error names the first offending chain -
 * unless n_chains >= 1, every chain has the same h = floor(n_used / 2), and h >= 2: chains of
 * unequal windows are not comparable by this statistic (pick a take no longer than the shortest
 * walk).  rhat [n_cols] may be NULL. */
int mhx_split_rhat(const double* half_mean, const double* half_var, const int32_t* n_used,
                   int64_t n_chains, int n_cols, double* rhat);

/* ---- ensemble percentiles: ONE posterior from all chains of a walker set.  On a set whose chains
 * sample the same posterior (one shared dataset) the user wants one median and one 95 % interval
 * drawn from every step of every chain, not one per chain.  The reference has no walker-set
 * reduction; the definition is this library's own and fixes every bit.
 *   window   chain c contributes its newest t_c = min(take, walker-length, steps held) steps: the
 *            window of mhx_get_percentiles.  n_used[c] = t_c, and 0 for an excluded chain
 *   pool     for column p the multiset of x[c][s][p] over all included chains c and s < t_c
 *   size     N = the sum of the t_c, an int64: *n_pooled
 *   rank     mhx_percentile_rank(N, num, den) gives pos and between
 *   value    the element at pos of the pool in ascending order by the order of
 *            mhx_get_percentiles: a NaN sorts last whatever its sign; -0 and +0 compare equal and
 *            either may stand for the other
 *   between  the IEEE (e[pos] + e[pos+1]) / 2
 * that is nth-percentile (M:1495-1506) on the concatenation of the chains' :param lists.  Exact
 * whatever n_chains and take are: a most-significant-digit-first radix selection over the whole
 * device - eight passes of 8-bit digits over the 64-bit order keys and, where a `between` rank is
 * the last of its run of equal values, one pass for the successor: at most nine launches, no
 * sort, no history moved; only integer counts cross to the host, so the result does not depend
 * on thread order, workgroup order or the split of the chains over devices.
 * Arguments: cols[n_cols] distinct parameter indices in [0, d), 1 <= n_cols <= d, in any order
 * (the outputs follow that order); include[n_chains] (NULL: every chain) leaves out the chains
 * whose byte is 0 - those that never converged, which show up as stuck in split R-hat or through
 * a poor most-likely step; 0 <= n_pct <= MHX_MAX_PERCENTILES (0 writes only the counts); take in
 * [1, history_capacity].  out [n_pct][n_cols]; status [n_cols]: 1 when the pool's column holds a
 * NaN.  Any output may be NULL.  MHX_ESTATE before mhx_init_chains; MHX_EINVAL for bad arguments
 * and for an include that leaves no chain; the outputs stay untouched on error.  A chain in
 * MHX_CHAIN_FP_TRAP is served from the history it has.  The device scratch (the counters of at
 * most 1008 tasks, 2 KiB each, the task list, the mask, n_used) does not depend on take;
 * mhx_get_summary_timing covers the kernels of all passes.  ("Ensemble" because mhx_get_pooled
 * already means the pooled adaptation.) */
int mhx_get_ensemble_percentiles(mhx_engine* e, int take, const int32_t* cols, int n_cols,
                                 const uint8_t* include, const int32_t* pct_num,
                                 const int32_t* pct_den, int n_pct, double* out, int64_t* n_pooled,
                                 int32_t* n_used, int32_t* status);
/* The same over a group: include and n_used in global chain order.  Every engine runs each pass
 * over its own chains, every device's launch enqueued before any is waited for; the host adds the
 * engines' counters (exact integers), picks once and hands every engine the same next tasks, and
 * takes the least of the engines' successors. */
int mhx_group_get_ensemble_percentiles(mhx_group* g, int take, const int32_t* cols, int n_cols,
                                       const uint8_t* include, const int32_t* pct_num,
                                       const int32_t* pct_den, int n_pct, double* out,
                                       int64_t* n_pooled, int32_t* n_used, int32_t* status);
/* One step of that selection on the host (needs no engine and no device): of counts[n_bins], the
 * smallest *digit whose cumulative count exceeds rank, the rank within that bin and the bin's
 * count.  MHX_EINVAL unless n_bins >= 1 and 0 <= rank < the sum of the counts.  Any output may
 * be NULL. */
int mhx_ensemble_pick(const uint64_t* counts, int n_bins, int64_t rank, int32_t* digit,
                      int64_t* rank_in_bin, int64_t* bin_count);

/* ---- which model to have fitted: WAIC (Watanabe; Gelman, Hwang and Vehtari 2014), the pointwise
 * predictive accuracy of every chain, on the device ring.  The reference has no such function
 * (walker-plot-residuals is what it offers): the definition is this library's own and fixes the
 * results operation by operation.  All arithmetic is plain IEEE binary64 multiply, add, subtract
 * and divide, never fused.  `fn` is one function of a global fit, N its point count, x_i the
 * dataset's own x.
 *   window   the newest n = min(take, walker-length, steps held) steps theta_0 (newest) ...
 *            theta_{n-1}: the window of mhx_get_percentiles.  n_used[c] = n
 *   value    v_is = function fn at x_i for theta_s, the very bits mhx_eval_function returns
 *   term     l_is, by the dataset's likelihood, from the numbers mhx_set_dataset forms:
 *            w_i = 1 / sigma_i, ys_i = y_i * w_i, c_i = -1/2 log(2 pi) + (-1 * log sigma_i) for the
 *            normal forms (sigma NULL: 1); c_i = -log-factorial(y_i) for Poisson, in the form
 *            mhx_config.poisson_logfact_double selects (the addends of the sweep's constant)
 *              MHX_LIK_NORMAL         a = v * w_i;  r = ys_i - a;  h = 0.5 * r;  q = h * r;
 *                                     l = c_i - q
 *              MHX_LIK_NORMAL_CUTOFF  the same, then l > -5000 ? l : -5000
 *              MHX_LIK_POISSON        l = ((y_i * tlog_rate(v)) - v) + c_i, tlog_rate the sweep's
 *                                     table logarithm (NaN unless v is a positive normal number)
 *              MHX_LIK_EXPR           l = the likelihood expression at (y_i, v, error_i); no constant
 *   over s   for s = 0 .. n-1 in that order, k = s + 1, q_k = 1.0 / k (one division):
 *              Welford      delta = l - mean;  mean = mean + delta * q_k;
 *                           M2 = M2 + delta * (l - mean)            from mean = 0, M2 = 0
 *              log-sum-exp  s = 0: M = l, S = 1.  Then with up = l > M,
 *                           g = exp(up ? M - l : l - M)  (the engine's exp, < 1 ulp),
 *                           S = up ? S * g + 1 : S + g,  M = up ? l : M
 *   point    pw_acc[c][i] = {M, S, mean, M2}
 *            pw_p[c][i]    = M2 / (n - 1)       (n = 1: the IEEE 0/0, as mhx_get_derived's
 *                                               standard deviation of one step)
 *            pw_lppd[c][i] = M + log(S / n)     (the engine's log, < 1 ulp; S / n one division)
 *   chain    the points go in blocks of MHX_WAIC_BLOCK: block b holds points b MHX_WAIC_BLOCK ..
 *            A block's sum of a pointwise quantity t: lane j = i mod 64 of the block adds its
 *            points serially in ascending i to a sum that starts at 0.0 (a point beyond N adds
 *            0.0), then the 64 lane sums are added pairwise, lanes 32 apart first, then 16, 8, 4,
 *            2, 1 (u_j = u_j + u_{j xor m}).  lppd[c] and p_waic[c] are the blocks' sums of
 *            pw_lppd and pw_p, added serially in ascending b to a sum that starts at 0.0.
 *            elpd[c] = lppd[c] - p_waic[c], one subtraction (waic = -2 elpd is the caller's).
 *            n_high[c] = the exact count of points with pw_p > 0.4 (where the variance
 *            approximation is known to be unreliable)
 *   status   a sum of
 *              MHX_WAIC_NONFINITE  a v_is or l_is of the chain is not finite (the reference would
 *                                  have trapped): the chain's numbers are unspecified; no other
 *                                  chain is touched by it
 *              MHX_WAIC_ONE_STEP   n = 1: pw_p and p_waic are NaN
 *            An empty window (n = 0: a walk that :burn-walks emptied) has no mean to take:
 *            n_used[c] = 0, status[c] = MHX_WAIC_NONFINITE, the chain's numbers are unspecified.
 * The results are the same bits from call to call, whatever portions the call is worked through
 * in and however a group's chains are split over its engines.
 * elpd, lppd, p_waic [n_chains]; n_high, n_used, status [n_chains]; pw_lppd, pw_p [n_chains][N];
 * pw_acc [n_chains][N][4].  Any output may be NULL.  take in [1, history_capacity], fn a function
 * of the problem, else MHX_EINVAL; MHX_ESTATE before mhx_init_chains; MHX_EUNSUPPORTED for an
 * engine with a dataset per walker (mhx_set_dataset_planes: its per-point constants are per
 * walker and not on the device).  The outputs stay untouched on error.  A chain in
 * MHX_CHAIN_FP_TRAP is served from the history it has.  Serves every model the engine can walk.
 * Worked through in portions whose device scratch stays below 64 MiB; mhx_get_summary_timing
 * covers the call. */
#define MHX_WAIC_BLOCK 256 /* points of one block of mhx_get_waic's sums */
enum {
  MHX_WAIC_NONFINITE = 1,
  MHX_WAIC_ONE_STEP = 2
};
int mhx_get_waic(mhx_engine* e, int fn, int take, double* elpd, double* lppd, double* p_waic,
                 int32_t* n_high, double* pw_lppd, double* pw_p, double* pw_acc, int32_t* n_used,
                 int32_t* status);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_waic(mhx_group* g, int fn, int take, double* elpd, double* lppd, double* p_waic,
                       int32_t* n_high, double* pw_lppd, double* pw_p, double* pw_acc,
                       int32_t* n_used, int32_t* status);

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman and Gabry 2017;
 * Vehtari, Simpson, Gelman, Yao and Gabry), the remedy for the points mhx_get_waic counts in n_high:
 * per data point the leave-one-out predictive accuracy elpd_loo_i and the Pareto shape khat_i that
 * says whether it can be trusted (khat above about 0.7: it cannot; the point is influential or an
 * outlier), from the same window of the same ring.  The reference has no such function: the
 * definition is this library's own and fixes the results operation by operation.  All arithmetic is
 * IEEE binary64 multiply, add, subtract, divide and square root, never fused; gexp and tlog are the
 * engine's exp and log (< 1 ulp each).  (double) of an integer is exact.  For chain c, function fn of
 * N points, point i:
 *   window, value, term   exactly mhx_get_waic's: n = min(take, walker-length, steps held) steps,
 *            newest first, with the terms l_0 ... l_{n-1} of point i, the same bits.  n_used[c] = n
 *   lppd     pw_lppd[c][i] by mhx_get_waic's running log-sum-exp, then M + tlog(S / n): the bits of
 *            mhx_get_waic's pw_lppd
 *   tail length   M = mhx_loo_tail_length(n, tail_len) (below)
 *   order    the steps are ordered by (key(l_s) ascending, s ascending), key the order of
 *            mhx_get_percentiles (-0 before +0).  The tail T_1 <= ... <= T_M is the first M of that
 *            order - the smallest terms, which are the largest importance ratios -, the body is the
 *            rest and l_cut is the body's first term.  With M = 0, T_1 = l_cut = the smallest term
 *            and every step is body.  Of steps with equal terms across the cut the newer ones
 *            (smaller s) are tail
 *   body sum S_b = the sum of gexp(T_1 - l_s) over the body's steps in ascending s, serially from 0.0
 *   ratios   for k = 1 .. M:  u_k = T_{M+1-k};  r_k = gexp(T_1 - u_k);  x_k = r_k - r_cut,
 *            r_cut = gexp(T_1 - l_cut)
 *   fit      (Zhang and Stephens 2009, with the prior of Vehtari et al.)  Md = (double)M,
 *            Mg = 30 + floor(sqrt M) as an integer (G = (double)Mg), x* = x_q, q = (M + 2) / 4 in
 *            integer division.  Unless x* > 0 and x_M > 0 the point is FLAT (below).  For j = 1 .. Mg:
 *              theta_j = 1.0 / x_M + ((1.0 - sqrt(G / (j - 0.5))) / 3.0) / x*
 *              k_j = (sum over k = 1 .. M, serially from 0.0, of tlog(1.0 - theta_j * x_k)) / Md
 *              L_j = Md * ((tlog((-theta_j) / k_j) - k_j) - 1.0)
 *            then w_j = 1.0 / (sum over i = 1 .. Mg, serially from 0.0, of gexp(L_i - L_j)),
 *            theta^ = the sum over j, serially from 0.0, of theta_j * w_j,
 *            k_raw = (sum over k, serially from 0.0, of tlog(1.0 - theta^ * x_k)) / Md,
 *            sigma = (-k_raw) / theta^,  khat = (Md * k_raw + 5.0) / (double)(M + 10).
 *            Any of theta^, k_raw, sigma, khat not finite, or sigma <= 0: the point is FLAT
 *   smoothing   for k = 1 .. M:  p_k = (k - 0.5) / Md;  t_k = tlog(1.0 - p_k);  y_k = (-khat) * t_k;
 *            q_k = (sigma * E(y_k)) / khat, where E(y) = gexp(y) - 1.0 unless |y| < 2^-5, where it is
 *            y * (1 + y * (c_2 + y * (c_3 + ... + y * c_8))) with c_m = 1.0 / m! (the quotients of
 *            1.0 by 2, 6, 24, 120, 720, 5040, 40320), every product and sum rounded;  khat = 0
 *            exactly: q_k = (-sigma) * t_k.  lw_k = min(tlog(q_k + r_cut), 0.0).
 *            A FLAT point, and every point where M = 0, takes the raw lw_k = T_1 - u_k and
 *            khat = +infinity (sigma is given as 0.0)
 *   estimate   W = the sum over k = 1 .. M, serially from 0.0, of gexp(lw_k + (u_k - T_1)),
 *            V = the same of gexp(lw_k);  A = (double)(n - M) + W;  D = S_b + V;
 *            pw_elpd[c][i] = T_1 + tlog(A / D);  pw_khat[c][i] = khat;
 *            pw_acc[c][i] = {T_1, l_cut, S_b, sigma};  tail[c][i][0 .. M-1] = T_1 .. T_M, NaN beyond
 *   chain    elpd_loo[c] and lppd[c] are the sums of pw_elpd and pw_lppd over blocks of MHX_LOO_BLOCK
 *            points by mhx_get_waic's rule (lane-serial, pairwise over the 64 lanes, serial over the
 *            blocks);  p_loo[c] = lppd[c] - elpd_loo[c], one subtraction (looic = -2 elpd_loo is the
 *            caller's);  n_high[c] = the exact count of points with khat > k_limit (+infinity, the
 *            khat of a point that was not fitted, exceeds every finite k_limit)
 *   status   a sum of
 *              MHX_LOO_NONFINITE  a value or a term of the chain is not finite (the reference would
 *                                 have trapped): the chain's numbers are unspecified; no other chain
 *                                 is touched by it
 *              MHX_LOO_SHORT      n < 25: M = 0, no point has a tail to fit
 *              MHX_LOO_FLAT       M > 0 and at least one point was FLAT (a chain that never moved is
 *                                 FLAT at every point: pw_elpd is the term itself)
 *              MHX_LOO_EMPTY      n = 0 (with MHX_LOO_SHORT): n_used[c] = 0, the pointwise results
 *                                 are NaN (pw_khat +infinity), the totals their sums
 * The results are the same bits from call to call, whatever portions the call is worked through in,
 * whether the fit reads its columns from LDS or from the staged terms (MHX_LOO_NO_LDS=1), and however
 * a group's chains are split over its engines.
 * elpd_loo, p_loo, lppd [n_chains]; n_high, n_used, status [n_chains]; pw_elpd, pw_khat, pw_lppd
 * [n_chains][N]; pw_acc [n_chains][N][4]; tail [n_chains][N][P] with P = mhx_loo_tail_length(take,
 * tail_len).  Any output may be NULL.  take in [1, history_capacity], tail_len in
 * [0, MHX_LOO_MAX_TAIL], fn a function of the problem, k_limit not a NaN, else MHX_EINVAL;
 * MHX_ESTATE before mhx_init_chains; MHX_EUNSUPPORTED for an engine with a dataset per walker
 * (mhx_set_dataset_planes: its per-point constants are per walker and not on the device), and where
 * the `take` staged terms of each of a chain's first MHX_LOO_BLOCK points do not fit the 64 MiB of a
 * portion (mhx_last_error names the greatest take that fits).  The outputs stay untouched on
 * error.  Serves every model the engine can walk.  Worked through in portions whose device scratch
 * stays below 64 MiB; mhx_get_summary_timing covers the call. */
#define MHX_LOO_BLOCK 256     /* points of one block of mhx_get_loo's sums */
#define MHX_LOO_MAX_TAIL 1024 /* the longest tail fitted */
enum {
  MHX_LOO_NONFINITE = 1,
  MHX_LOO_SHORT = 2,
  MHX_LOO_FLAT = 4,
  MHX_LOO_EMPTY = 8
};
/* The tail length of a window of n steps.  tail_len = 0: *M = min(floor(n / 5), R) with R the least
 * integer whose square is at least 9 n (ceil(3 sqrt n), in integer arithmetic).  tail_len > 0:
 * *M = min(tail_len, floor(n / 5)) - the caller's way to shorten the tail for an autocorrelated
 * chain.  Never above MHX_LOO_MAX_TAIL; a length below 5 (n < 25) is given as 0.  1000 -> 95,
 * 8192 -> 272, a full ring of 65536 -> 768.  Host only: needs no engine and no device.  MHX_EINVAL
 * unless n >= 0 and tail_len is in [0, MHX_LOO_MAX_TAIL].  M may be NULL. */
int mhx_loo_tail_length(int64_t n, int32_t tail_len, int32_t* M);
int mhx_get_loo(mhx_engine* e, int fn, int take, int tail_len, double k_limit, double* elpd_loo,
                double* p_loo, double* lppd, int32_t* n_high, int32_t* n_used, int32_t* status,
                double* pw_elpd, double* pw_khat, double* pw_lppd, double* pw_acc, double* tail);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_loo(mhx_group* g, int fn, int take, int tail_len, double k_limit, double* elpd_loo,
                      double* p_loo, double* lppd, int32_t* n_high, int32_t* n_used,
                      int32_t* status, double* pw_elpd, double* pw_khat, double* pw_lppd,
                      double* pw_acc, double* tail);

/* ---- held-out predictive density: the log pointwise predictive density, under every chain's
 * window, of data the CALLER hands in - a fold left out of the fit (K-fold cross-validation, the
 * remedy the PSIS-LOO authors prescribe for points whose khat is high), a repeated measurement, or
 * the walker's own spectrum of a set with a dataset per walker.  mhx_get_waic and mhx_get_loo score
 * a chain on the data it walked over; this call reads the model, the ring and the caller's arrays
 * only, so an engine with a dataset per walker (mhx_set_dataset_planes) is SERVED: its planes are
 * not read.  The reference has no such function: the definition is this library's own and fixes the
 * results operation by operation.  All arithmetic is plain IEEE binary64 multiply, add, subtract
 * and divide, never fused.  For chain c, function fn and the caller's point i < m:
 *   data     xcols [n_cols][m] as for mhx_get_fit_percentiles (never NULL here; n_cols the function's
 *            column count), shared by all chains.  y [m], or [n_chains][m] with y_per_chain.  sigma by
 *            sigma_kind with m in place of n: MHX_SIGMA_NONE (NULL), MHX_SIGMA_SHARED [m],
 *            MHX_SIGMA_PER_CHAIN [n_chains], MHX_SIGMA_PER_POINT [n_chains][m].  use NULL (every
 *            point), [m], or [n_chains][m] with use_per_chain: chain c USES point i where its byte is
 *            nonzero
 *   window   mhx_get_waic's: the newest n = min(take, walker-length, steps held) steps, newest
 *            first.  n_used[c] = n
 *   value    v_is = function fn at x_i for theta_s, the very bits mhx_eval_function returns
 *   term     l_is = mhx_get_waic's term for the function's own likelihood (MHX_LIK_NORMAL,
 *            _NORMAL_CUTOFF, _POISSON, _EXPR), from numbers formed of the caller's (y, sigma) exactly as
 *            mhx_set_dataset would form them: w = 1 / sigma, ys = y * w, c = -1/2 log(2 pi) +
 *            (-1 * log sigma) by libm's log for the normal forms (no sigma: 1); c = -log-factorial(y)
 *            in the form mhx_config.poisson_logfact_double selects for Poisson (sigma is not read);
 *            error = sigma (no sigma: 1) and no constant for an expression likelihood.  The caller's
 *            arrays are checked as mhx_set_dataset checks them for that likelihood, used or not: a
 *            sigma that is not finite and > 0, or a Poisson y that is no count, is refused by its
 *            index in the caller's array ("sigma[3]")
 *   over s   for s = 0 .. n-1 in that order, k = s + 1, q_k = 1.0 / k (one division):
 *              log-sum-exp (M, S) of the TERMS l_is: mhx_get_waic's, operation for operation
 *              Welford of the VALUES v_is:  delta = v - mean_v;  mean_v = mean_v + delta * q_k;
 *                           M2_v = M2_v + delta * (v - mean_v)           from mean_v = 0, M2_v = 0
 *            (mhx_get_fit_percentiles' mean is the same recurrence: the same bits at the same x)
 *   point    pw_acc[c][i] = {M, S, mean_v, M2_v};  pw_lpd[c][i] = M + log(S / n) (the engine's log,
 *            < 1 ulp; S / n one division).  A point chain c does not use: 0.0 in all five, and it
 *            adds 0.0 to every sum
 *   chain    lpd[c] = the sum of pw_lpd over blocks of MHX_HELDOUT_BLOCK points by mhx_get_waic's
 *            rule: lane j = i mod 64 of a block adds its points serially in ascending i to a sum that
 *            starts at 0.0 (a point beyond m or not used adds 0.0), the 64 lane sums are added
 *            pairwise, lanes 32 apart first, then 16, 8, 4, 2, 1, and the blocks' sums serially in
 *            ascending b to a sum that starts at 0.0.  n_scored[c] = the exact count of used points
 *   status   a sum of
 *              MHX_HELDOUT_NONFINITE  a v_is or l_is of a point the chain USES is not finite, or the
 *                                     window is empty (n = 0): the chain's numbers are unspecified;
 *                                     no other chain is touched by it.  What an unused point
 *                                     evaluates to sets nothing
 *              MHX_HELDOUT_NO_POINTS  the chain uses no point: lpd[c] = 0.0, n_scored[c] = 0
 * The results are the same bits from call to call, whatever portions the call is worked through in
 * and however a group's chains are split over its engines.  With the engine's own (x, y, sigma) and
 * use NULL, pw_lpd, lpd and pw_acc[..][0..1] are the bits of mhx_get_waic's pw_lppd, lppd and pw_acc.
 * lpd [n_chains]; n_scored, n_used, status [n_chains]; pw_lpd [n_chains][m]; pw_acc [n_chains][m][4].
 * Any output may be NULL.  take in [1, history_capacity], fn a function of the problem, m >= 1,
 * xcols and y not NULL, n_cols the function's, sigma_kind one of the four and NONE exactly where
 * sigma is NULL, the data valid (above), else MHX_EINVAL; MHX_ESTATE before mhx_init_chains;
 * MHX_EUNSUPPORTED where the problem cannot be made final, as for mhx_get_waic and
 * mhx_get_fit_percentiles (a dataset per walker is not such a case).  The outputs stay untouched on
 * error.  A chain in MHX_CHAIN_FP_TRAP is served from the history it has.  Serves every model the
 * engine can walk.
 * Worked through in portions whose device scratch stays below 64 MiB; mhx_get_summary_timing covers
 * the call. */
#define MHX_HELDOUT_BLOCK 256 /* points of one block of mhx_get_heldout's sums */
enum {
  MHX_HELDOUT_NONFINITE = 1,
  MHX_HELDOUT_NO_POINTS = 2
};
int mhx_get_heldout(mhx_engine* e, int fn, int take, const double* xcols, int n_cols, int64_t m,
                    const double* y, int y_per_chain, const double* sigma, int sigma_kind,
                    const uint8_t* use, int use_per_chain, double* lpd, int32_t* n_scored,
                    double* pw_lpd, double* pw_acc, int32_t* n_used, int32_t* status);
/* The same for a group: y, sigma, use and the outputs that go by chain are in global chain order;
 * every device's work is enqueued before any is waited for. */
int mhx_group_get_heldout(mhx_group* g, int fn, int take, const double* xcols, int n_cols,
                          int64_t m, const double* y, int y_per_chain, const double* sigma,
                          int sigma_kind, const uint8_t* use, int use_per_chain, double* lpd,
                          int32_t* n_scored, double* pw_lpd, double* pw_acc, int32_t* n_used,
                          int32_t* status);

/* ---- credible bands: the pointwise posterior of the fit curve, of every chain, on the device ring.
 * mhx_get_fit_bands is the reference's envelope - the extremes of the model over the most probable
 * steps, a plotting device whose width depends on take.  This is the posterior statement: at each
 * x the percentiles, the mean and the standard deviation of f(x; theta_s) over the window.  The
 * reference has no such function: the definition is this library's own and fixes the results
 * operation by operation.  All arithmetic is plain IEEE binary64, never fused.
 *   window      the newest n = min(take, walker-length, steps held) steps theta_0 (newest) ...
 *               theta_{n-1}: the window of mhx_get_percentiles and mhx_get_waic, NOT the candidate
 *               set of mhx_get_fit_bands.  n_used[c] = n
 *   value       v_js = function fn at point j for theta_s, the very bits mhx_eval_function returns.
 *               xcols, n_cols, m as for mhx_eval_function (NULL: the function's own x; two columns
 *               where the function reads two)
 *   percentile  pct[c][q][j] = nth-percentile (M:1495-1506) of the n values {v_js}_s at
 *               pct_num[q] / pct_den[q] per cent: mhx_percentile_rank(n, ...) gives pos and
 *               between; the result is the element at pos of the ascending order, or
 *               (e[pos] + e[pos+1]) / 2 - one IEEE add, one IEEE divide - when between.  The order
 *               is that of mhx_get_percentiles: -0 before +0 (they compare equal as numbers: either
 *               may be returned), a NaN last whatever its sign.  Exact for any take: a radix
 *               selection over the 64-bit order keys, nothing approximated
 *   moments     over s = 0 .. n-1 in that order, k = s + 1, q_k = 1.0 / k (one division):
 *                 delta = v - mean;  mean = mean + delta * q_k;  M2 = M2 + delta * (v - mean)
 *               from mean = 0, M2 = 0 (mhx_get_waic's Welford recurrence).  mean[c][j] = the final
 *               mean; stddev[c][j] = sqrt(M2 / (n - 1)): one IEEE divide, a correctly rounded
 *               square root (n = 1: the IEEE 0/0, as mhx_get_derived)
 *   status      a sum of
 *                 MHX_FITPCT_NONFINITE  some v_js of the chain is not finite: the percentiles still
 *                                       follow the order above, the moments are whatever IEEE
 *                                       gives; no other chain is touched by it
 *                 MHX_FITPCT_ONE_STEP   n = 1
 *                 MHX_FITPCT_EMPTY      n = 0: the chain's numbers are unspecified, n_used[c] = 0
 * pct [n_chains][n_pct][m]; mean, stddev [n_chains][m]; n_used, status [n_chains].  Any output
 * may be NULL.  take in [1, history_capacity], fn a function of the problem, m >= 1, n_cols the
 * function's, 0 <= n_pct <= MHX_MAX_PERCENTILES (0: the moments only), else MHX_EINVAL;
 * MHX_ESTATE before mhx_init_chains; the outputs stay untouched on error.  A chain in
 * MHX_CHAIN_FP_TRAP is served from the history it has.  Serves every model the engine can walk,
 * an engine with a dataset per walker (mhx_set_dataset_planes) included: the call reads the model,
 * the shared x and the ring only.  The results are the same bits from call to call, whatever
 * portions the call is worked through in, whether the selection reads its columns from LDS or
 * from memory (MHX_FITPCT_NO_LDS=1), and however a group's chains are split over its engines.
 * Device scratch: the window's values of a portion are staged, take doubles per chain and point,
 * and the points go in chunks of whole blocks of MHX_FITPCT_BLOCK so that a portion stays below
 * 64 MiB whatever n_chains and m are.  ONE chain's smallest chunk - p = min(m, MHX_FITPCT_BLOCK)
 * points - must fit: 8 p take bytes of values, 8 p (n_pct + 4) of x and results, 8 for the two
 * counts and 2 KiB of alignment within 64 MiB: take <= 65529 - n_pct at m >= 128, more at fewer
 * points (a ring of 65536 is served whole at m <= 127).  Beyond that the call is refused with
 * MHX_EUNSUPPORTED and mhx_last_error names the greatest take that fits.
 * mhx_get_summary_timing covers the call. */
#define MHX_FITPCT_BLOCK 128 /* points of one block of mhx_get_fit_percentiles' value kernel */
enum {
  MHX_FITPCT_NONFINITE = 1,
  MHX_FITPCT_ONE_STEP = 2,
  MHX_FITPCT_EMPTY = 4
};
int mhx_get_fit_percentiles(mhx_engine* e, int fn, int take, const double* xcols, int n_cols,
                            int64_t m, const int32_t* pct_num, const int32_t* pct_den, int n_pct,
                            double* pct, double* mean, double* stddev, int32_t* n_used,
                            int32_t* status);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_fit_percentiles(mhx_group* g, int fn, int take, const double* xcols, int n_cols,
                                  int64_t m, const int32_t* pct_num, const int32_t* pct_den,
                                  int n_pct, double* pct, double* mean, double* stddev,
                                  int32_t* n_used, int32_t* status);

/* ---- which walkers fit badly: walker-plot-residuals (M:1271-1292) without the plotting, for EVERY
 * walker of a set, with the goodness-of-fit statistics of the standardized residuals reduced on the
 * device.  For each chain c function `fn` is evaluated at ONE parameter vector over the chain's own
 * data; the fit values and the residuals themselves come back only when asked for.  The definition
 * fixes the results operation by operation; all arithmetic is plain IEEE binary64 multiply, add,
 * subtract, divide and square root, never fused.  N is the function's point count.
 *   theta    [n_chains][d], the caller's vectors (the medians mhx_get_percentiles returned, say);
 *            NULL: each chain's most-likely parameters, which are on the device
 *   data     the function's shared dataset, or chain c's own plane where the engine was given a
 *            dataset per walker (mhx_set_dataset_planes; all four sigma_kinds), in the numbers the
 *            engine formed when the dataset was set and holds on the device: w_i = 1 / sigma_i,
 *            ys_i = y_i * w_i (MHX_SIGMA_PER_CHAIN: the walker's one w; MHX_SIGMA_NONE and a NULL
 *            sigma: 1.0); for Poisson the raw counts y_i.  Nothing is uploaded per point.
 *   value    v_i = function fn at the dataset's own x_i for theta_c, the very bits
 *            mhx_eval_function returns.  fit[c][i] = v_i
 *   z        the standardized residual, fit minus data as the reference has it (M:1283):
 *              MHX_LIK_NORMAL, MHX_LIK_NORMAL_CUTOFF   a = v_i * w_i;  z_i = a - ys_i
 *              MHX_LIK_POISSON (Pearson)               dl = v_i - y_i;  rt = sqrt(v_i) (correctly
 *                                                      rounded);  z_i = dl / rt (one division)
 *              MHX_LIK_EXPR                            refused (MHX_EUNSUPPORTED): an expression
 *                                                      likelihood's `error` need not be a sigma
 *            z[c][i] = z_i
 *   point    in dataset order i = 0 .. N-1:  t_chi = z_i * z_i;  t_dw = 0.0 at i = 0, else
 *            dd = z_i - z_{i-1}, t_dw = dd * dd;  s_i = (z_i > 0.0) - zero, -0 and NaN are "not
 *            positive"
 *   sums     chi2[c], sum_z[c], dw[c] = the sums of t_chi, z_i, t_dw by mhx_get_waic's rule with
 *            blocks of MHX_RESID_BLOCK points: lane j = i mod 64 of a block adds its points serially
 *            in ascending i to a sum that starts at 0.0 (a point beyond N adds 0.0), the 64 lane
 *            sums are added pairwise, lanes 32 apart first, then 16, 8, 4, 2, 1
 *            (u_j = u_j + u_{j xor m}), and the blocks' sums are added serially in ascending block
 *            order to a sum that starts at 0.0.  (Durbin and Watson's statistic is dw / chi2, the
 *            caller's division.)
 *   counts   exact integers: n_pos[c] = #{i : s_i};  n_runs[c] = 1 + #{i >= 1 : s_i != s_{i-1}}, the
 *            runs of equal sign (Wald and Wolfowitz);  n_out[c] = #{i : |z_i| > z_limit}
 *   extreme  from m = -1.0, idx = -1: for ascending i, where |z_i| > m take (m, idx) = (|z_i|, i).
 *            A NaN never compares greater and is passed over; ties keep the earliest i.
 *            max_abs_z[c] = m, max_index[c] = idx
 *   status   MHX_RESID_NONFINITE where some v_i or z_i of the chain is not finite: the chain's three
 *            sums are then unspecified; its counts and extreme still follow the rules above, and
 *            no other chain is touched by it
 * The results are the same bits from call to call, whatever portions the call is worked through in,
 * however the points are split into chunks and however a group's chains are split over its engines.
 * fit, z [n_chains][N]; chi2, sum_z, dw, max_abs_z [n_chains]; max_index [n_chains]; n_pos, n_runs,
 * n_out, status [n_chains].  Any output may be NULL.  fn a function of the problem and z_limit not a
 * NaN, else MHX_EINVAL; MHX_ESTATE before mhx_init_chains; the outputs stay untouched on error.
 * Serves every model the engine can walk.  Worked through in portions whose device scratch stays
 * below 64 MiB; mhx_get_summary_timing covers the call. */
#define MHX_RESID_BLOCK 256 /* points of one block of mhx_get_residuals' sums */
enum {
  MHX_RESID_NONFINITE = 1
};
int mhx_get_residuals(mhx_engine* e, int fn, const double* theta, double z_limit, double* fit,
                      double* z, double* chi2, double* sum_z, double* dw, double* max_abs_z,
                      int64_t* max_index, int32_t* n_pos, int32_t* n_runs, int32_t* n_out,
                      int32_t* status);
/* The same for a group, in global chain order (theta too); every device's work is enqueued before
 * any is waited for. */
int mhx_group_get_residuals(mhx_group* g, int fn, const double* theta, double z_limit, double* fit,
                            double* z, double* chi2, double* sum_z, double* dw, double* max_abs_z,
                            int64_t* max_index, int32_t* n_pos, int32_t* n_runs, int32_t* n_out,
                            int32_t* status);

/* ---- before the walk: the normal equations of EVERY walker's least-squares problem ------------
 * What any least-squares tool forms from the Jacobian: the weighted residual vector u, the scaled
 * Jacobian g by central differences, and their products F = g^T g (the Gauss-Newton / Fisher
 * matrix, whose inverse is the classical covariance (J^T W J)^-1), b = g^T u (the step's right-hand
 * side: F delta = b is the Gauss-Newton step that RAISES the likelihood) and chi2 = u^T u, for
 * function `fn` at ONE parameter vector per chain over the chain's own data.  The definition fixes
 * the results operation by operation; every operation is one IEEE binary64 rounding (add, subtract,
 * multiply, divide, square root), nothing is fused, there is no fma.  N is the function's point
 * count, d the length of the parameter vector.
 *   theta    [n_chains][d], the caller's vectors; NULL: each chain's most-likely parameters, as
 *            mhx_get_residuals
 *   steps    the half-widths h of the central differences, one per place of theta: [d], or
 *            [n_chains][d] when per_chain_steps != 0.  Each >= 0 and finite, else MHX_EINVAL.
 *   data     as mhx_get_residuals: the numbers the engine formed when the dataset was set, w_i =
 *            1 / sigma_i, ys_i = y_i * w_i (chain c's own row of a dataset per walker, all four
 *            sigma_kinds); for Poisson the raw counts y_i
 *   centre   v_i = function fn at x_i for theta_c, the very bits mhx_eval_function returns
 *   column   for place t of theta (a GLOBAL index, 0 <= t < d) with h = steps[..][t]:
 *            if h == 0, or function fn does not read theta_t (t is not in its gather map), the
 *            column is exactly +0.0: g[c][t][.], jtr[c][t], and row and column t of jtj[c].  Else
 *              tp = theta_t + h;  tm = theta_t - h;  dh = tp - tm
 *              vp_i, vm_i = function fn at x_i for theta_c with theta_t replaced by tp, by tm - the
 *                           very bits mhx_eval_function returns for those vectors
 *              df = vp_i - vm_i;  J = df / dh
 *   scaling  by the function's likelihood:
 *              MHX_LIK_NORMAL, MHX_LIK_NORMAL_CUTOFF   g_it = J * w_i;  a = v_i * w_i;  u_i = ys_i - a
 *                    (the cutoff's clamp is NOT differentiated: these are the normal likelihood's
 *                    equations whatever the cutoff)
 *              MHX_LIK_POISSON (Fisher scoring)        rt = sqrt(v_i) (correctly rounded);
 *                    g_it = J / rt;  dl = y_i - v_i;  u_i = dl / rt
 *              MHX_LIK_EXPR                            refused (MHX_EUNSUPPORTED), for
 *                    mhx_get_residuals' reason: an expression likelihood's `error` need not be a sigma
 *            u_i is the exact negation of mhx_get_residuals' z_i.  g[c][t][i] = g_it
 *   sums     the points go in blocks of MHX_NORMEQ_BLOCK: block b holds points 1024 b ..
 *            min(1024 b + 1023, N - 1).  Within a block each of
 *              chi2 = sum u_i * u_i;  jtr[t] = sum g_it * u_i;  jtj[t][s] = sum g_it * g_is  (t <= s)
 *            is formed serially in ascending i from 0.0: pr = (the product); sum = sum + pr.  A
 *            point beyond N is skipped (not added as zero).  The blocks' sums are then added
 *            serially in ascending b to a sum that starts at 0.0.  jtj[s][t] is a copy of
 *            jtj[t][s]: both triangles are written.
 *   status   MHX_NORMEQ_NONFINITE where any v_i, vp_i, vm_i, g_it or u_i of the chain is not
 *            finite - dh == 0 with h != 0 among them, the IEEE 0/0 or x/0: the chain's numbers are
 *            then unspecified, and no other chain is touched by it
 * The results are the same bits from call to call, whatever portions the call is worked through in,
 * however the points are split into chunks and however a group's chains are split over its engines.
 * jtj [n_chains][d][d]; jtr [n_chains][d]; chi2, status [n_chains]; g [n_chains][d][N].  Any output
 * may be NULL.  fn a function of the problem, else MHX_EINVAL; MHX_ESTATE before mhx_init_chains;
 * the outputs stay untouched on error.  Serves every model the engine can walk.  Worked through in
 * portions whose device scratch stays below 64 MiB (one chain's, where that alone is more);
 * mhx_get_summary_timing covers the call.
 * Measured (tools/normeq_timing.py, 4096 chains, one MI355X, medians of 9 warm calls): 8
 * parameters on 1e5 shared points 44.5 ms wall, 43.9 ms of kernel (17 model values per point:
 * 1.6e11 values/s) against 79 s by 17 mhx_eval_function calls and numpy per chain (64 chains
 * timed, extrapolated); 4096 spectra of 334 points, a dataset per walker, 7 parameters: 0.38 ms
 * wall, 0.17 ms of kernel, against 2.4 s. */
#define MHX_NORMEQ_BLOCK 1024 /* points of one block of mhx_get_normal_equations' sums */
enum {
  MHX_NORMEQ_NONFINITE = 1
};
int mhx_get_normal_equations(mhx_engine* e, int fn, const double* theta, const double* steps,
                             int per_chain_steps, double* jtj, double* jtr, double* chi2,
                             double* g, int32_t* status);
/* The same for a group, in global chain order (theta and per-chain steps too); every device's work
 * is enqueued before any is waited for. */
int mhx_group_get_normal_equations(mhx_group* g, int fn, const double* theta, const double* steps,
                                   int per_chain_steps, double* jtj, double* jtr, double* chi2,
                                   double* g_out, int32_t* status);

/* ---- candidate search: the chi-square of MANY parameter vectors per walker, ranked on the device.
 * The brute-force stage of a least-squares toolkit (lmfit's brute, MINUIT's scan) for a walker set:
 * every chain tries m candidate vectors against its own data in one call, the points are read once,
 * and the `keep` best come back.  Levenberg-Marquardt and the walk's proposal are local; where a
 * line moves from spectrum to spectrum this finds the basin they start in.  It also gives the
 * chi-square maps drawn around a solution (per_chain candidates: each walker's own vector with one
 * or two places replaced).  The definition fixes the results operation by operation.
 *   cand      per_chain == 0: [m][d], tried by every chain; else [n_chains][m][d], chain c's own.
 *             Full parameter vectors.
 *   fn        >= 0: that function alone; -1: all K functions of the problem
 *   term      chi2_k(c, j), for function k, chain c and candidate j, is exactly the chi2 that
 *             mhx_get_residuals defines for theta = cand_j over chain c's data: the shared dataset
 *             or the chain's plane (all four sigma_kinds); v_i the bits of mhx_eval_function; z_i per
 *             likelihood as stated there; t_i = z_i * z_i summed by the MHX_RESID_BLOCK rule (lane
 *             j = i mod 64 of a block serially from 0.0, the lanes pairwise 32, 16, 8, 4, 2, 1 apart,
 *             the blocks serially in ascending order from 0.0).  Nothing is fused.
 *   score     score[c][j] = 0.0 + chi2_k0 + chi2_k1 + ..., added serially in ascending k over the
 *             selected functions
 *   not finite  where some v_i or z_i of a selected function is not finite, or the total is not
 *             finite, score[c][j] is exactly +infinity and the candidate counts in n_bad[c].  No
 *             other candidate or chain is touched by it.
 *   ranking   best_index[c][r], best_score[c][r], r = 0 .. keep-1: chain c's candidates in ascending
 *             (score, index) order - equal scores (those at +infinity too) go to the smaller index.
 *             Where m < keep the remaining entries are index -1, score +infinity.
 * The results are the same bits from call to call, whatever portions the call is worked through in
 * and however a group's chains are split over its engines.
 * score [n_chains][m]; best_index, best_score [n_chains][keep]; n_bad [n_chains].  Any output may be
 * NULL.  m in [1, 2^31 - 2], keep in [1, MHX_CAND_KEEP_MAX], fn -1 or a function of the problem and
 * cand not NULL, else MHX_EINVAL; MHX_EINVAL too where ONE chain's pieces - m scores and m block sums
 * for each of the selected functions' blocks, 8 bytes each, and the shared candidates - outgrow the
 * stage: try fewer candidates a call.  MHX_ESTATE before mhx_init_chains.  MHX_EUNSUPPORTED, by name,
 * where a selected function has an expression likelihood (MHX_LIK_EXPR), as mhx_get_residuals
 * refuses it.  The outputs stay untouched on error.  Serves every model the engine can walk.  Worked
 * through in portions of chains whose device scratch stays below 64 MiB; mhx_get_summary_timing
 * covers the call.
 * Measured (tools/cand_timing.py, 4096 chains, one MI355X, build csrc:2a3e91c16c6b7519 - the
 * kernels of this commit, before this comment was completed - medians of 9 warm calls): 4096
 * spectra of 334 points, a dataset per walker, 7 parameters, a shared 17 x 17 grid: 1.43 ms wall,
 * 1.03 ms of kernel, against 57.8 ms by 289 mhx_get_residuals calls; 64 shared candidates of 8
 * parameters on 1e5 shared points: 55.8 ms wall, 54.6 ms of kernel (4.8e11 model values/s), against
 * 288 ms by 64 mhx_get_residuals calls.  (One mhx_logpost of all 262144 rows - the walk's own sum,
 * other bits, shared data only - takes 9.7 ms there.) */
#define MHX_CAND_KEEP_MAX 16 /* the most candidates mhx_get_candidate_scores ranks per chain */
int mhx_get_candidate_scores(mhx_engine* e, int fn, const double* cand, int64_t m, int per_chain,
                             int keep, double* score, int32_t* best_index, double* best_score,
                             int32_t* n_bad);
/* The same for a group, in global chain order (per-chain candidates too); every device's work is
 * enqueued before any is waited for. */
int mhx_group_get_candidate_scores(mhx_group* g, int fn, const double* cand, int64_t m, int per_chain,
                                   int keep, double* score, int32_t* best_index, double* best_score,
                                   int32_t* n_bad);

/* ---- batched traces: the steps of EVERY chain, filtered and thinned on the device -------------
 * What (mapcar (lambda (w) (walker-get w :get :steps / :unique-steps / :forward-steps / :params /
 * :param / :log-liklihoods :take take)) walkers) reads (M:490-510, M:540) - the data behind
 * walker-catepillar-plots (M:1294-1309), walker-liklihood-plot (M:1313-1320) and
 * walker-plot-one-corner (M:1322-1331) - in one call: only the columns asked for, only every
 * stride-th kept step, optionally with the extremes of what lies between.  No arithmetic is done:
 * every number returned is a number of the ring, bit for bit.
 *   window    chain c's window is exactly what mhx_get_trace(e, c, take, ...) delivers, newest
 *             first: steps s = 0 .. t-1 with t = n_used[c] = min(take, walker-length, steps the
 *             ring holds).  take in [1, history_capacity].
 *   filter    gives the KEPT LIST, newest first; n_kept[c] is its length.
 *               MHX_TRACE_STEPS    every step
 *               MHX_TRACE_UNIQUE   (M:492-496) step s when s == t-1 or the bits of prob[s] differ
 *                                  from the bits of prob[s+1]: the oldest step is always kept, a
 *                                  NaN equals a NaN of the same bits, -0 differs from +0
 *               MHX_TRACE_FORWARD  (M:497-502) step s when s < t-1 and !(prob[s] <= prob[s+1]):
 *                                  the oldest step is never kept, a NaN on either side keeps s
 *             (the predicates of mhx_get_covariances and mhx_get_proposal_factors)
 *   thinning  `thin` (M:149-157) of the kept list: row r is kept item i = start + r stride;
 *             rows = mhx_trace_rows(n_kept[c], stride, start) = 0 when n_kept <= start, else
 *             ceil((n_kept - start) / stride); n_out[c] = min(rows, max_out).
 *             values[c][r][j] = column cols[j] of that step's parameter vector, or the step's prob
 *             where cols[j] == MHX_TRACE_PROB.  Rows n_out[c] .. max_out-1 of values, lo and hi
 *             are all-bits-zero.
 *   envelope  computed only when lo or hi is given.  Row r's bucket is the kept items i in
 *             [start + r stride, min(start + (r+1) stride, n_kept)), visited in that order.  lo
 *             and hi both start as the bucket's first value (= values[c][r][j]); for each later
 *             value v: if (v < lo) lo = v; if (v > hi) hi = v;  So a NaN that is not first is
 *             ignored, a first NaN stays, and of -0.0 / +0.0 the earlier one stays.  With stride 1
 *             lo == hi == values.
 * values, lo, hi [n_chains][max_out][n_cols]; n_out, n_kept, n_used [n_chains]; any output may be
 * NULL.  MHX_EINVAL unless filter is one of the three, 1 <= stride <= history_capacity,
 * 0 <= start < stride, 1 <= n_cols, cols is non-NULL and every cols[j] lies in [-1, d) (a column
 * may be named more than once), 1 <= max_out <= history_capacity; also when the pieces of ONE
 * chain (up to three arrays of max_out n_cols doubles) exceed the 64 MiB of a portion.  MHX_ESTATE
 * before mhx_init_chains; a chain in MHX_CHAIN_FP_TRAP is read from the history it has.  Worked
 * through in portions whose device scratch stays below 64 MiB; mhx_get_summary_timing covers the
 * call. */
enum {
  MHX_TRACE_STEPS = 0,
  MHX_TRACE_UNIQUE = 1,
  MHX_TRACE_FORWARD = 2
};
#define MHX_TRACE_PROB (-1) /* a "column" that is the step's prob */
int mhx_get_traces(mhx_engine* e, int take, int filter, int stride, int start,
                   const int32_t* cols, int n_cols, int max_out, double* values, double* lo,
                   double* hi, int32_t* n_out, int32_t* n_kept, int32_t* n_used);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_traces(mhx_group* g, int take, int filter, int stride, int start,
                         const int32_t* cols, int n_cols, int max_out, double* values, double* lo,
                         double* hi, int32_t* n_out, int32_t* n_kept, int32_t* n_used);
/* *rows = the rows `thin` (M:149-157) leaves of a list of n_kept items: those at start,
 * start + stride, ...  Host only: needs no engine and no device.  MHX_EINVAL unless n_kept >= 0,
 * stride >= 1, 0 <= start < stride. */
int mhx_trace_rows(int64_t n_kept, int32_t stride, int32_t start, int64_t* rows);

/* Highest-density intervals and quantile ladders of every chain, on the device: the narrowest
 * interval that holds a given mass of a column's window, and the window's quantile function at
 * evenly spaced ranks.  This library's own definition (the reference's intervals are equal-tailed:
 * mhx_get_percentiles); the one read-out that orders a window.  For chain c and column cols[j]:
 *   window    that of mhx_get_percentiles: the newest n = min(take, walker-length, steps held)
 *             steps; n_used[c] = n.
 *   order     s_0 .. s_{n-1}: the column's window values in ascending order of the key of
 *             mhx_get_percentiles - -0 before +0, every NaN last.
 *   span      of the mass mass_num[q] / mass_den[q] per cent: g = min(floor(n num / (100 den)),
 *             n - 1) in exact integers = mhx_hdi_span(n, num, den).
 *   interval  w_i = s_{i+g} - s_i for i = 0 .. n-1-g, each ONE IEEE subtraction of the two doubles;
 *             pos[c][q][j] = the least i whose w_i is not greater than any other (of equal least
 *             widths the lowest interval); lo[c][q][j] = s_pos and hi[c][q][j] = s_{pos+g}, numbers
 *             of the ring bit for bit (the subtraction itself is never returned).  A mass of 100
 *             gives the window's least and greatest value.
 *   ladder    n_ladder = L is 0 or in [2, MHX_MAX_HDI_LADDER]: ladder[c][j][i] = s_{r_i} with
 *             r_i = floor(i (n - 1) / (L - 1)) in exact integers, i = 0 .. L-1 (ranks repeat where
 *             n < L).  A NaN comes back as the NaN mhx_get_percentiles returns for it.
 *   status    status[c][j] = MHX_HDI_NONFINITE where the column's window holds a value that is not
 *             finite; lo, hi and pos of that column are then unspecified (hi and lo are still
 *             values of the window, pos a rank in range), its ladder stays defined, and the other
 *             columns of the chain are unaffected.
 * cols: distinct indices in [0, d), 1 <= n_cols <= d, as mhx_get_histograms; 0 <= n_mass <=
 * MHX_MAX_HDI_MASSES, each mass with 1 <= den <= 1000000 and 1 <= num <= 100 den.  lo, hi, pos
 * [n_chains][n_mass][n_cols] (the layout of mhx_get_percentiles' out), ladder
 * [n_chains][n_cols][n_ladder], status [n_chains][n_cols], n_used [n_chains]; any output may be
 * NULL.  MHX_EINVAL on any other argument and when the pieces of ONE chain exceed the 64 MiB of a
 * portion - which happens only where the keys of the padded windows (n_cols columns of the least
 * power of two >= take, 8 bytes each) lie in memory, not in a workgroup's LDS: 63 columns of a
 * window of 2^17 steps with ladders of 4096 ranks.
 * MHX_ESTATE before mhx_init_chains.  Worked through in portions whose device scratch stays below
 * 64 MiB; mhx_get_summary_timing covers the call. */
enum {
  MHX_HDI_NONFINITE = 1
};
int mhx_get_hdi(mhx_engine* e, int take, const int32_t* cols, int n_cols, const int32_t* mass_num,
                const int32_t* mass_den, int n_mass, int n_ladder, double* lo, double* hi,
                int32_t* pos, double* ladder, int32_t* n_used, int32_t* status);
/* The same of derived quantities: mhx_get_derived's expressions (its grammar, compile cache and
 * value kernel, `prob` included) evaluated at every step of the window take the ring columns'
 * place, expression k as column k (n_cols = n_expr).  status[c][k] = MHX_HDI_NONFINITE where a
 * value of expression k is not finite, as mhx_get_derived's status.  Refuses what mhx_get_derived
 * refuses of exprs, names, index and take. */
int mhx_get_derived_hdi(mhx_engine* e, const char* const* exprs, int n_expr,
                        const char* const* names, const int32_t* index, int n_names, int take,
                        const int32_t* mass_num, const int32_t* mass_den, int n_mass, int n_ladder,
                        double* lo, double* hi, int32_t* pos, double* ladder, int32_t* n_used,
                        int32_t* status);
/* The same for a group, in global chain order; every device's work is enqueued before any is
 * waited for. */
int mhx_group_get_hdi(mhx_group* g, int take, const int32_t* cols, int n_cols,
                      const int32_t* mass_num, const int32_t* mass_den, int n_mass, int n_ladder,
                      double* lo, double* hi, int32_t* pos, double* ladder, int32_t* n_used,
                      int32_t* status);
int mhx_group_get_derived_hdi(mhx_group* g, const char* const* exprs, int n_expr,
                              const char* const* names, const int32_t* index, int n_names, int take,
                              const int32_t* mass_num, const int32_t* mass_den, int n_mass,
                              int n_ladder, double* lo, double* hi, int32_t* pos, double* ladder,
                              int32_t* n_used, int32_t* status);
/* *g = the span of a mass of num/den per cent among n sorted values: min(floor(n num / (100 den)),
 * n - 1), in exact integers whatever n.  Host only: needs no engine and no device.  MHX_EINVAL
 * unless n >= 1, 1 <= den <= 1000000 and 1 <= num <= 100 den. */
int mhx_hdi_span(int64_t n, int32_t num, int32_t den, int64_t* g);

/* Restore a saved walk (walker-load, sketched in the comments M:987-1001): prob[n], theta[n][d]
 * NEWEST FIRST, as walker-save would have written them.  Sets the ring (newest
 * min(n, history_capacity) steps), last-step, length, age = n and the most-likely step. */
int mhx_set_history(mhx_engine* e, int64_t chain, const double* prob, const double* theta, int n);

/* walker-modify's list surgery (M:566-578) for every chain: :burn-walks n drops the n oldest
 * steps, :keep-walks n keeps the n newest, :reset makes the walk its oldest retained step,
 * :reset-to-most-likely the most likely step (both also move last-step); n is ignored by the
 * resets.  (:add-step happens inside walker-take-step on the device; :delete = mhx_destroy.) */
enum {
  MHX_MODIFY_BURN_WALKS = 0,
  MHX_MODIFY_KEEP_WALKS = 1,
  MHX_MODIFY_RESET = 2,
  MHX_MODIFY_RESET_TO_MOST_LIKELY = 3
};
int mhx_walker_modify(mhx_engine* e, int action, int64_t n);

/* MHX_ADAPT_POOLED read-back: stats [1+d+d*d] = (n, sum delta, sum delta delta^T) pooled over
 * chains (and ranks) at the last 200-iteration tick; L_pool [d][d] = (2.38^2/d) chol(cov);
 * valid = 1 when that factor is in use; refreshes = ticks performed. */
int mhx_get_pooled(mhx_engine* e, double* stats, double* L_pool, int32_t* valid,
                   uint64_t* refreshes);

/* Total chain-steps taken by this engine since creation (all chains). */
int mhx_get_counters(mhx_engine* e, uint64_t* chain_steps, uint64_t* kernel_launches);

/* Which kernels serve the current problem, for logs and benchmarks: "w16/gauss22_normal" (an
 * ahead-of-time specialisation of the 16-chains-per-workgroup family), "w8/generic", or
 * "w16/rtc[PeaksModel<2, 3, false>:normal]" (compiled at run time, one entry per function).
 * Finalises the problem like mhx_init_chains does; NULL (and mhx_last_error) if that fails.
 * The string lives until the problem is changed or the engine destroyed. */
const char* mhx_kernel_name(mhx_engine* e);

/* Timing of the step kernel on the engine's own stream (HIP events): average
 * milliseconds per launch and launches since the last reset. */
int mhx_kernel_timing(mhx_engine* e, int reset, double* avg_ms, uint64_t* launches,
                      double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* MHX_H */
