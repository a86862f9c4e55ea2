;;;; bindings.lisp -- CFFI declarations of include/mhx.h, one defcfun per entry point.
(in-package #:mcmc-fitting-amd)

(cffi:define-foreign-library libmhx
  (:unix (:or "libmhx.so" "./libmhx.so"))
  (t (:default "libmhx")))

(defun load-libmhx (&optional path)
  "Load libmhx.so (PATH overrides the search).  There is no pure-Lisp fallback: without the
library, or without a gfx950 device, walker-create signals MHX-ERROR."
  (if path
      (cffi:load-foreign-library path)
      (cffi:use-foreign-library libmhx)))

(define-condition mhx-error (error)
  ((code :initarg :code :reader mhx-error-code)
   (message :initarg :message :reader mhx-error-message))
  (:report (lambda (c s)
             (format s "libmhx error ~d: ~a" (mhx-error-code c) (mhx-error-message c)))))

;;; status codes / enums of mhx.h
(defconstant +mhx-ok+ 0)
(defconstant +lik-normal+ 0)
(defconstant +lik-normal-cutoff+ 1)
(defconstant +lik-poisson+ 2)
(defconstant +lik-expr+ 3)
(defconstant +sigma-none+ 0)
(defconstant +sigma-shared+ 1)
(defconstant +sigma-per-chain+ 2)
(defconstant +sigma-per-point+ 3)
(defconstant +chain-running+ 0)
(defconstant +chain-done+ 1)
(defconstant +chain-fp-trap+ 2)
(defconstant +chain-stopped+ 3)

(cffi:defcstruct mhx-config
  (n-chains :int64)
  (n-params :int32)
  (n-functions :int32)
  (device :int32)
  (adapt-mode :int32)
  (seed :uint64)
  (chain-offset :int64)
  (history-capacity :int32)
  (poisson-logfact-double :int32))

(cffi:defcstruct mhx-run-opts
  (n :int64)
  (temperature :double)
  (auto-mode :int32)
  (max-walker-length :int64)
  (l-matrix :pointer)
  (l-matrix-per-chain :int32))

(cffi:defcfun ("mhx_version" %mhx-version) :int)
(cffi:defcfun ("mhx_build_id" %mhx-build-id) :string)
(cffi:defcfun ("mhx_last_error" %mhx-last-error) :string)
(cffi:defcfun ("mhx_device_count" %mhx-device-count) :int (count :pointer))
(cffi:defcfun ("mhx_create" %mhx-create) :int (cfg :pointer) (out :pointer))
(cffi:defcfun ("mhx_destroy" %mhx-destroy) :void (e :pointer))
(cffi:defcfun ("mhx_set_function" %mhx-set-function) :int
  (e :pointer) (k :int) (model-id :int) (shape :pointer) (n-shape :int)
  (param-index :pointer) (n-index :int))
(cffi:defcfun ("mhx_set_dataset" %mhx-set-dataset) :int
  (e :pointer) (k :int) (x :pointer) (y :pointer) (sigma :pointer) (n :size) (likelihood :int))
(cffi:defcfun ("mhx_set_dataset_planes" %mhx-set-dataset-planes) :int
  (e :pointer) (k :int) (x :pointer) (y :pointer) (sigma :pointer) (sigma-kind :int) (n :size)
  (likelihood :int))
(cffi:defcfun ("mhx_set_dataset_cols" %mhx-set-dataset-cols) :int
  (e :pointer) (k :int) (xcols :pointer) (n-cols :int) (y :pointer) (sigma :pointer) (n :size)
  (likelihood :int))
(cffi:defcfun ("mhx_set_bounds" %mhx-set-bounds) :int
  (e :pointer) (k :int) (idx :pointer) (lo :pointer) (hi :pointer) (n :int))
(cffi:defcfun ("mhx_set_function_expr" %mhx-set-function-expr) :int
  (e :pointer) (k :int) (expr :string) (param-names :pointer) (param-index :pointer) (n-index :int))
(cffi:defcfun ("mhx_set_expr_recognition" %mhx-set-expr-recognition) :int (e :pointer) (on :int))
(cffi:defcfun ("mhx_expr_classify" %mhx-expr-classify) :int
  (expr :string) (param-names :pointer) (n-names :int) (model :pointer) (shape :pointer)
  (order :pointer) (n-order :pointer))
(cffi:defcfun ("mhx_set_prior_expr" %mhx-set-prior-expr) :int
  (e :pointer) (k :int) (expr :string) (names :pointer) (index :pointer) (n :int))
(cffi:defcfun ("mhx_set_likelihood_expr" %mhx-set-likelihood-expr) :int
  (e :pointer) (k :int) (expr :string))
(cffi:defcfun ("mhx_walker_modify" %mhx-walker-modify) :int (e :pointer) (action :int) (n :int64))
(cffi:defcfun ("mhx_set_history" %mhx-set-history) :int
  (e :pointer) (chain :int64) (prob :pointer) (theta :pointer) (n :int))
(cffi:defcfun ("mhx_get_pooled" %mhx-get-pooled) :int
  (e :pointer) (stats :pointer) (l-pool :pointer) (valid :pointer) (refreshes :pointer))
(cffi:defcfun ("mhx_init_chains" %mhx-init-chains) :int
  (e :pointer) (theta0 :pointer) (broadcast :int))
(cffi:defcfun ("mhx_logpost" %mhx-logpost) :int
  (e :pointer) (theta :pointer) (n :size) (out :pointer) (parts :pointer))
(cffi:defcfun ("mhx_step_injected" %mhx-step-injected) :int
  (e :pointer) (l :pointer) (per-chain-l :int) (z :pointer) (u :pointer) (temp :pointer)
  (accepted-out :pointer))
(cffi:defcfun ("mhx_run_opts_default" %mhx-run-opts-default) :void (o :pointer))
(cffi:defcfun ("mhx_adaptive_begin" %mhx-adaptive-begin) :int (e :pointer) (o :pointer))
(cffi:defcfun ("mhx_adaptive_advance" %mhx-adaptive-advance) :int
  (e :pointer) (max-iters :int64) (n-running :pointer))
(cffi:defcfun ("mhx_adaptive_steps_full" %mhx-adaptive-steps-full) :int (e :pointer) (o :pointer))
(cffi:defcfun ("mhx_adaptive_steps" %mhx-adaptive-steps) :int (e :pointer) (n :int64))
(cffi:defcfun ("mhx_many_steps" %mhx-many-steps) :int
  (e :pointer) (n :int64) (l :pointer) (per-chain-l :int))
(cffi:defcfun ("mhx_request_stop" %mhx-request-stop) :int (e :pointer))
(cffi:defcfun ("mhx_set_allreduce" %mhx-set-allreduce) :int
  (e :pointer) (fn :pointer) (ctx :pointer) (wants-device-buffer :int))
(cffi:defcfun ("mhx_get_state" %mhx-get-state) :int
  (e :pointer) (theta :pointer) (logpost :pointer) (best-theta :pointer) (best-logpost :pointer)
  (length :pointer) (age :pointer))
(cffi:defcfun ("mhx_get_chain_status" %mhx-get-chain-status) :int
  (e :pointer) (status :pointer) (loop-index :pointer))
(cffi:defcfun ("mhx_get_lmatrix" %mhx-get-lmatrix) :int (e :pointer) (l :pointer))
(cffi:defcfun ("mhx_get_temperature" %mhx-get-temperature) :int (e :pointer) (temp :pointer))
(cffi:defcfun ("mhx_get_acceptance" %mhx-get-acceptance) :int
  (e :pointer) (take :int) (out :pointer))
(cffi:defcfun ("mhx_get_trace" %mhx-get-trace) :int
  (e :pointer) (chain :int64) (take :int) (prob :pointer) (theta :pointer) (n-out :pointer))
(cffi:defcfun ("mhx_get_proposal_factor" %mhx-get-proposal-factor) :int
  (e :pointer) (chain :int64) (take :int) (l-out :pointer) (status :pointer) (n-forward :pointer))
(cffi:defcfun ("mhx_get_counters" %mhx-get-counters) :int
  (e :pointer) (chain-steps :pointer) (kernel-launches :pointer))
(cffi:defcfun ("mhx_kernel_name" %mhx-kernel-name) :string (e :pointer))
(cffi:defcfun ("mhx_kernel_timing" %mhx-kernel-timing) :int
  (e :pointer) (reset :int) (avg-ms :pointer) (launches :pointer) (total-ms :pointer))

(cffi:defcfun ("mhx_take_step" %mhx-take-step) :int
  (e :pointer) (l :pointer) (per-chain-l :int) (temperature :double))
(cffi:defcfun ("mhx_get_chain" %mhx-get-chain) :int
  (e :pointer) (chain :int64) (theta :pointer) (logpost :pointer) (best-theta :pointer)
  (best-logpost :pointer) (length :pointer) (age :pointer))
;;; native RCCL for one-process-per-GPU hosts (a Lisp image per GPU, e.g. under MPI)
(cffi:defcfun ("mhx_comm_get_unique_id" %mhx-comm-get-unique-id) :int (id :pointer))
(cffi:defcfun ("mhx_comm_init_rank" %mhx-comm-init-rank) :int
  (e :pointer) (id :pointer) (rank :int) (n-ranks :int))
;;; one Lisp image, several GPUs
(cffi:defcfun ("mhx_group_partition" %mhx-group-partition) :int
  (n-chains :int64) (n-parts :int) (part :int) (first :pointer) (count :pointer))
(cffi:defcfun ("mhx_group_create" %mhx-group-create) :int
  (cfg :pointer) (devices :pointer) (n-devices :int) (out :pointer))
(cffi:defcfun ("mhx_group_destroy" %mhx-group-destroy) :void (g :pointer))
(cffi:defcfun ("mhx_group_size" %mhx-group-size) :int (g :pointer))
(cffi:defcfun ("mhx_group_engine" %mhx-group-engine) :pointer (g :pointer) (i :int))
(cffi:defcfun ("mhx_group_chain_range" %mhx-group-chain-range) :int
  (g :pointer) (i :int) (first :pointer) (count :pointer))
(cffi:defcfun ("mhx_group_set_function" %mhx-group-set-function) :int
  (g :pointer) (k :int) (model-id :int) (shape :pointer) (n-shape :int)
  (param-index :pointer) (n-index :int))
(cffi:defcfun ("mhx_group_set_dataset" %mhx-group-set-dataset) :int
  (g :pointer) (k :int) (x :pointer) (y :pointer) (sigma :pointer) (n :size) (likelihood :int))
(cffi:defcfun ("mhx_group_set_dataset_planes" %mhx-group-set-dataset-planes) :int
  (g :pointer) (k :int) (x :pointer) (y :pointer) (sigma :pointer) (sigma-kind :int) (n :size)
  (likelihood :int))
(cffi:defcfun ("mhx_group_set_dataset_cols" %mhx-group-set-dataset-cols) :int
  (g :pointer) (k :int) (xcols :pointer) (n-cols :int) (y :pointer) (sigma :pointer) (n :size)
  (likelihood :int))
(cffi:defcfun ("mhx_group_set_bounds" %mhx-group-set-bounds) :int
  (g :pointer) (k :int) (idx :pointer) (lo :pointer) (hi :pointer) (n :int))
(cffi:defcfun ("mhx_group_set_function_expr" %mhx-group-set-function-expr) :int
  (g :pointer) (k :int) (expr :string) (param-names :pointer) (param-index :pointer) (n-index :int))
(cffi:defcfun ("mhx_group_set_expr_recognition" %mhx-group-set-expr-recognition) :int
  (g :pointer) (on :int))
(cffi:defcfun ("mhx_group_set_prior_expr" %mhx-group-set-prior-expr) :int
  (g :pointer) (k :int) (expr :string) (names :pointer) (index :pointer) (n :int))
(cffi:defcfun ("mhx_group_set_likelihood_expr" %mhx-group-set-likelihood-expr) :int
  (g :pointer) (k :int) (expr :string))
(cffi:defcfun ("mhx_group_init_chains" %mhx-group-init-chains) :int
  (g :pointer) (theta0 :pointer) (broadcast :int))
(cffi:defcfun ("mhx_group_adaptive_begin" %mhx-group-adaptive-begin) :int (g :pointer) (o :pointer))
(cffi:defcfun ("mhx_group_adaptive_advance" %mhx-group-adaptive-advance) :int
  (g :pointer) (max-iters :int64) (n-running :pointer))
(cffi:defcfun ("mhx_group_adaptive_steps_full" %mhx-group-adaptive-steps-full) :int
  (g :pointer) (o :pointer))
(cffi:defcfun ("mhx_group_request_stop" %mhx-group-request-stop) :int (g :pointer))
(cffi:defcfun ("mhx_group_get_state" %mhx-group-get-state) :int
  (g :pointer) (theta :pointer) (logpost :pointer) (best-theta :pointer) (best-logpost :pointer)
  (length :pointer) (age :pointer))
(cffi:defcfun ("mhx_group_get_counters" %mhx-group-get-counters) :int
  (g :pointer) (chain-steps :pointer) (kernel-launches :pointer))
;; walker-set-get: summaries of every chain in one launch
(cffi:defcfun ("mhx_percentile_rank" %mhx-percentile-rank) :int
  (len :int64) (num :int32) (den :int32) (pos :pointer) (between :pointer))
(cffi:defcfun ("mhx_get_percentiles" %mhx-get-percentiles) :int
  (e :pointer) (take :int) (pct-num :pointer) (pct-den :pointer) (n-pct :int) (out :pointer)
  (n-used :pointer))
(cffi:defcfun ("mhx_get_covariances" %mhx-get-covariances) :int
  (e :pointer) (take :int) (cov :pointer) (n-unique :pointer) (status :pointer))
(cffi:defcfun ("mhx_get_proposal_factors" %mhx-get-proposal-factors) :int
  (e :pointer) (take :int) (l-out :pointer) (status :pointer) (n-forward :pointer))
(cffi:defcfun ("mhx_get_window_best" %mhx-get-window-best) :int
  (e :pointer) (take :int) (prob :pointer) (theta :pointer))
(cffi:defcfun ("mhx_get_history_capacity" %mhx-get-history-capacity) :int
  (e :pointer) (capacity :pointer))
(cffi:defcfun ("mhx_get_summary_timing" %mhx-get-summary-timing) :int
  (e :pointer) (kernel-ms :pointer))
(cffi:defcfun ("mhx_group_get_percentiles" %mhx-group-get-percentiles) :int
  (g :pointer) (take :int) (pct-num :pointer) (pct-den :pointer) (n-pct :int) (out :pointer)
  (n-used :pointer))
(cffi:defcfun ("mhx_group_get_covariances" %mhx-group-get-covariances) :int
  (g :pointer) (take :int) (cov :pointer) (n-unique :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_proposal_factors" %mhx-group-get-proposal-factors) :int
  (g :pointer) (take :int) (l-out :pointer) (status :pointer) (n-forward :pointer))
(cffi:defcfun ("mhx_group_get_window_best" %mhx-group-get-window-best) :int
  (g :pointer) (take :int) (prob :pointer) (theta :pointer))
(cffi:defcfun ("mhx_band_count" %mhx-band-count) :int (take :int64) (k :pointer))
(cffi:defcfun ("mhx_eval_function" %mhx-eval-function) :int
  (e :pointer) (fn :int) (theta :pointer) (n :int64) (xcols :pointer) (n-cols :int) (m :int64)
  (out :pointer))
(cffi:defcfun ("mhx_get_fit_bands" %mhx-get-fit-bands) :int
  (e :pointer) (fn :int) (take :int) (xcols :pointer) (n-cols :int) (m :int64) (ymax :pointer)
  (ymin :pointer) (n-selected :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_fit_bands" %mhx-group-get-fit-bands) :int
  (g :pointer) (fn :int) (take :int) (xcols :pointer) (n-cols :int) (m :int64) (ymax :pointer)
  (ymin :pointer) (n-selected :pointer) (status :pointer))
(cffi:defcfun ("mhx_get_derived" %mhx-get-derived) :int
  (e :pointer) (exprs :pointer) (n-expr :int) (names :pointer) (index :pointer) (n-names :int)
  (take :int) (pct-num :pointer) (pct-den :pointer) (n-pct :int) (at-most-likely :pointer)
  (pct :pointer) (mean :pointer) (stddev :pointer) (values :pointer) (n-used :pointer)
  (status :pointer))
(cffi:defcfun ("mhx_group_get_derived" %mhx-group-get-derived) :int
  (g :pointer) (exprs :pointer) (n-expr :int) (names :pointer) (index :pointer) (n-names :int)
  (take :int) (pct-num :pointer) (pct-den :pointer) (n-pct :int) (at-most-likely :pointer)
  (pct :pointer) (mean :pointer) (stddev :pointer) (values :pointer) (n-used :pointer)
  (status :pointer))
;; walker-param-histo / walker-plot-corner as counts over the caller's edges
(cffi:defcfun ("mhx_get_histograms" %mhx-get-histograms) :int
  (e :pointer) (take :int) (cols :pointer) (n-cols :int) (n-bins :int) (edges :pointer)
  (edges-per-chain :int) (counts :pointer) (outside :pointer) (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_get_pair_grids" %mhx-get-pair-grids) :int
  (e :pointer) (take :int) (cols :pointer) (n-cols :int) (pair-a :pointer) (pair-b :pointer)
  (n-pairs :int) (n-bins :int) (edges :pointer) (edges-per-chain :int) (counts :pointer)
  (n-inside :pointer) (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_histograms" %mhx-group-get-histograms) :int
  (g :pointer) (take :int) (cols :pointer) (n-cols :int) (n-bins :int) (edges :pointer)
  (edges-per-chain :int) (counts :pointer) (outside :pointer) (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_pair_grids" %mhx-group-get-pair-grids) :int
  (g :pointer) (take :int) (cols :pointer) (n-cols :int) (pair-a :pointer) (pair-b :pointer)
  (n-pairs :int) (n-bins :int) (edges :pointer) (edges-per-chain :int) (counts :pointer)
  (n-inside :pointer) (n-used :pointer) (status :pointer))
;; autocorrelation time, effective sample size, the half moments of split R-hat; split R-hat
(cffi:defcfun ("mhx_get_autocorr" %mhx-get-autocorr) :int
  (e :pointer) (take :int) (cols :pointer) (n-cols :int) (max-lag :int) (tau :pointer)
  (ess :pointer) (acf :pointer) (half-mean :pointer) (half-var :pointer) (n-lags :pointer)
  (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_autocorr" %mhx-group-get-autocorr) :int
  (g :pointer) (take :int) (cols :pointer) (n-cols :int) (max-lag :int) (tau :pointer)
  (ess :pointer) (acf :pointer) (half-mean :pointer) (half-var :pointer) (n-lags :pointer)
  (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_split_rhat" %mhx-split-rhat) :int
  (half-mean :pointer) (half-var :pointer) (n-used :pointer) (n-chains :int64) (n-cols :int)
  (rhat :pointer))
;; ensemble percentiles: one posterior from all chains of a walker set; one step of its selection
(cffi:defcfun ("mhx_get_ensemble_percentiles" %mhx-get-ensemble-percentiles) :int
  (e :pointer) (take :int) (cols :pointer) (n-cols :int) (include :pointer) (pct-num :pointer)
  (pct-den :pointer) (n-pct :int) (out :pointer) (n-pooled :pointer) (n-used :pointer)
  (status :pointer))
(cffi:defcfun ("mhx_group_get_ensemble_percentiles" %mhx-group-get-ensemble-percentiles) :int
  (g :pointer) (take :int) (cols :pointer) (n-cols :int) (include :pointer) (pct-num :pointer)
  (pct-den :pointer) (n-pct :int) (out :pointer) (n-pooled :pointer) (n-used :pointer)
  (status :pointer))
(cffi:defcfun ("mhx_ensemble_pick" %mhx-ensemble-pick) :int
  (counts :pointer) (n-bins :int) (rank :int64) (digit :pointer) (rank-in-bin :pointer)
  (bin-count :pointer))
;; WAIC: the pointwise predictive accuracy of every chain (status: a sum of the two constants)
(defconstant +waic-nonfinite+ 1)
(defconstant +waic-one-step+ 2)
(cffi:defcfun ("mhx_get_waic" %mhx-get-waic) :int
  (e :pointer) (fn :int) (take :int) (elpd :pointer) (lppd :pointer) (p-waic :pointer)
  (n-high :pointer) (pw-lppd :pointer) (pw-p :pointer) (pw-acc :pointer) (n-used :pointer)
  (status :pointer))
(cffi:defcfun ("mhx_group_get_waic" %mhx-group-get-waic) :int
  (g :pointer) (fn :int) (take :int) (elpd :pointer) (lppd :pointer) (p-waic :pointer)
  (n-high :pointer) (pw-lppd :pointer) (pw-p :pointer) (pw-acc :pointer) (n-used :pointer)
  (status :pointer))
;; PSIS-LOO: leave-one-out accuracy and Pareto k of every chain (status: a sum of the four constants)
(defconstant +loo-nonfinite+ 1)
(defconstant +loo-short+ 2)
(defconstant +loo-flat+ 4)
(defconstant +loo-empty+ 8)
(defconstant +loo-max-tail+ 1024)
(cffi:defcfun ("mhx_loo_tail_length" %mhx-loo-tail-length) :int
  (n :int64) (tail-len :int32) (m :pointer))
(cffi:defcfun ("mhx_get_loo" %mhx-get-loo) :int
  (e :pointer) (fn :int) (take :int) (tail-len :int) (k-limit :double) (elpd-loo :pointer)
  (p-loo :pointer) (lppd :pointer) (n-high :pointer) (n-used :pointer) (status :pointer)
  (pw-elpd :pointer) (pw-khat :pointer) (pw-lppd :pointer) (pw-acc :pointer) (tail :pointer))
(cffi:defcfun ("mhx_group_get_loo" %mhx-group-get-loo) :int
  (g :pointer) (fn :int) (take :int) (tail-len :int) (k-limit :double) (elpd-loo :pointer)
  (p-loo :pointer) (lppd :pointer) (n-high :pointer) (n-used :pointer) (status :pointer)
  (pw-elpd :pointer) (pw-khat :pointer) (pw-lppd :pointer) (pw-acc :pointer) (tail :pointer))
;; held-out predictive density: data the caller hands in, scored under every chain's window
;; (status: a sum of the two constants)
(defconstant +heldout-nonfinite+ 1)
(defconstant +heldout-no-points+ 2)
(cffi:defcfun ("mhx_get_heldout" %mhx-get-heldout) :int
  (e :pointer) (fn :int) (take :int) (xcols :pointer) (n-cols :int) (m :int64) (y :pointer)
  (y-per-chain :int) (sigma :pointer) (sigma-kind :int) (use :pointer) (use-per-chain :int)
  (lpd :pointer) (n-scored :pointer) (pw-lpd :pointer) (pw-acc :pointer) (n-used :pointer)
  (status :pointer))
(cffi:defcfun ("mhx_group_get_heldout" %mhx-group-get-heldout) :int
  (g :pointer) (fn :int) (take :int) (xcols :pointer) (n-cols :int) (m :int64) (y :pointer)
  (y-per-chain :int) (sigma :pointer) (sigma-kind :int) (use :pointer) (use-per-chain :int)
  (lpd :pointer) (n-scored :pointer) (pw-lpd :pointer) (pw-acc :pointer) (n-used :pointer)
  (status :pointer))
;; credible bands: pointwise percentiles and moments of the fit (status: a sum of the three constants)
(defconstant +fitpct-nonfinite+ 1)
(defconstant +fitpct-one-step+ 2)
(defconstant +fitpct-empty+ 4)
(cffi:defcfun ("mhx_get_fit_percentiles" %mhx-get-fit-percentiles) :int
  (e :pointer) (fn :int) (take :int) (xcols :pointer) (n-cols :int) (m :int64) (pct-num :pointer)
  (pct-den :pointer) (n-pct :int) (pct :pointer) (mean :pointer) (stddev :pointer)
  (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_fit_percentiles" %mhx-group-get-fit-percentiles) :int
  (g :pointer) (fn :int) (take :int) (xcols :pointer) (n-cols :int) (m :int64) (pct-num :pointer)
  (pct-den :pointer) (n-pct :int) (pct :pointer) (mean :pointer) (stddev :pointer)
  (n-used :pointer) (status :pointer))
;; residuals: the goodness of fit of every walker at one parameter vector each (theta may be null)
(defconstant +resid-nonfinite+ 1)
(cffi:defcfun ("mhx_get_residuals" %mhx-get-residuals) :int
  (e :pointer) (fn :int) (theta :pointer) (z-limit :double) (fit :pointer) (z :pointer)
  (chi2 :pointer) (sum-z :pointer) (dw :pointer) (max-abs-z :pointer) (max-index :pointer)
  (n-pos :pointer) (n-runs :pointer) (n-out :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_residuals" %mhx-group-get-residuals) :int
  (g :pointer) (fn :int) (theta :pointer) (z-limit :double) (fit :pointer) (z :pointer)
  (chi2 :pointer) (sum-z :pointer) (dw :pointer) (max-abs-z :pointer) (max-index :pointer)
  (n-pos :pointer) (n-runs :pointer) (n-out :pointer) (status :pointer))
;; normal equations: g^T g, g^T u and u^T u of every walker's least-squares problem (theta may be null)
(defconstant +normeq-nonfinite+ 1)
(cffi:defcfun ("mhx_get_normal_equations" %mhx-get-normal-equations) :int
  (e :pointer) (fn :int) (theta :pointer) (steps :pointer) (per-chain-steps :int) (jtj :pointer)
  (jtr :pointer) (chi2 :pointer) (g :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_normal_equations" %mhx-group-get-normal-equations) :int
  (g :pointer) (fn :int) (theta :pointer) (steps :pointer) (per-chain-steps :int) (jtj :pointer)
  (jtr :pointer) (chi2 :pointer) (g-out :pointer) (status :pointer))
;; candidate search: the chi-square of m vectors per walker, ranked (any output may be null)
(defconstant +cand-keep-max+ 16)
(cffi:defcfun ("mhx_get_candidate_scores" %mhx-get-candidate-scores) :int
  (e :pointer) (fn :int) (cand :pointer) (m :int64) (per-chain :int) (keep :int) (score :pointer)
  (best-index :pointer) (best-score :pointer) (n-bad :pointer))
(cffi:defcfun ("mhx_group_get_candidate_scores" %mhx-group-get-candidate-scores) :int
  (g :pointer) (fn :int) (cand :pointer) (m :int64) (per-chain :int) (keep :int) (score :pointer)
  (best-index :pointer) (best-score :pointer) (n-bad :pointer))
(cffi:defcfun ("mhx_get_traces" %mhx-get-traces) :int
  (e :pointer) (take :int) (filter :int) (stride :int) (start :int) (cols :pointer) (n-cols :int)
  (max-out :int) (values :pointer) (lo :pointer) (hi :pointer) (n-out :pointer) (n-kept :pointer)
  (n-used :pointer))
(cffi:defcfun ("mhx_group_get_traces" %mhx-group-get-traces) :int
  (g :pointer) (take :int) (filter :int) (stride :int) (start :int) (cols :pointer) (n-cols :int)
  (max-out :int) (values :pointer) (lo :pointer) (hi :pointer) (n-out :pointer) (n-kept :pointer)
  (n-used :pointer))
(cffi:defcfun ("mhx_trace_rows" %mhx-trace-rows) :int
  (n-kept :int64) (stride :int32) (start :int32) (rows :pointer))
;; highest-density intervals and quantile ladders: the one read-out that orders a window
(cffi:defcfun ("mhx_hdi_span" %mhx-hdi-span) :int
  (n :int64) (num :int32) (den :int32) (g :pointer))
(cffi:defcfun ("mhx_get_hdi" %mhx-get-hdi) :int
  (e :pointer) (take :int) (cols :pointer) (n-cols :int) (mass-num :pointer) (mass-den :pointer)
  (n-mass :int) (n-ladder :int) (lo :pointer) (hi :pointer) (pos :pointer) (ladder :pointer)
  (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_hdi" %mhx-group-get-hdi) :int
  (g :pointer) (take :int) (cols :pointer) (n-cols :int) (mass-num :pointer) (mass-den :pointer)
  (n-mass :int) (n-ladder :int) (lo :pointer) (hi :pointer) (pos :pointer) (ladder :pointer)
  (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_get_derived_hdi" %mhx-get-derived-hdi) :int
  (e :pointer) (exprs :pointer) (n-expr :int) (names :pointer) (index :pointer) (n-names :int)
  (take :int) (mass-num :pointer) (mass-den :pointer) (n-mass :int) (n-ladder :int) (lo :pointer)
  (hi :pointer) (pos :pointer) (ladder :pointer) (n-used :pointer) (status :pointer))
(cffi:defcfun ("mhx_group_get_derived_hdi" %mhx-group-get-derived-hdi) :int
  (g :pointer) (exprs :pointer) (n-expr :int) (names :pointer) (index :pointer) (n-names :int)
  (take :int) (mass-num :pointer) (mass-den :pointer) (n-mass :int) (n-ladder :int) (lo :pointer)
  (hi :pointer) (pos :pointer) (ladder :pointer) (n-used :pointer) (status :pointer))

(defmacro with-c-call (&body body)
  "HIP/RCCL runtime code may raise inexact/invalid flags that SBCL turns into conditions;
mask the traps around every foreign call (SURVEY 8b)."
  #+sbcl `(sb-int:with-float-traps-masked (:invalid :divide-by-zero :overflow :inexact)
            ,@body)
  #-sbcl `(progn ,@body))

(defun check (rc)
  (unless (= rc +mhx-ok+)
    (error 'mhx-error :code rc :message (%mhx-last-error)))
  rc)

(defun fill-doubles (ptr seq)
  (let ((i 0))
    (map nil (lambda (v)
               (setf (cffi:mem-aref ptr :double i) (coerce v 'double-float))
               (incf i))
         seq)
    ptr))

(defun fill-int32s (ptr seq)
  (let ((i 0))
    (map nil (lambda (v) (setf (cffi:mem-aref ptr :int32 i) v) (incf i)) seq)
    ptr))

(defmacro with-c-strings ((var strings) &body body)
  "VAR: a foreign array of char* holding copies of STRINGS for the extent of BODY"
  (let ((n (gensym "N")) (ptrs (gensym "PTRS")) (i (gensym "I")))
    `(let* ((,n (length ,strings))
            (,ptrs (mapcar #'cffi:foreign-string-alloc ,strings)))
       (unwind-protect
            (cffi:with-foreign-object (,var :pointer (max 1 ,n))
              (loop for p in ,ptrs for ,i from 0
                    do (setf (cffi:mem-aref ,var :pointer ,i) p))
              ,@body)
         (mapc #'cffi:foreign-string-free ,ptrs)))))

(defun read-doubles (ptr n)
  (let ((out (make-array n :element-type 'double-float)))
    (dotimes (i n out)
      (setf (aref out i) (cffi:mem-aref ptr :double i)))))
