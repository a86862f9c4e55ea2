;;;; walker.lisp -- walker-create / walker-adaptive-steps / walker-get over libmhx.
;;; Mirrors the reference's surface for the walker-adaptive-steps path; every number is
;;; computed below the C ABI.  Citations M: = mcmc-fitting.lisp of the reference.
(in-package #:mcmc-fitting-amd)

(defvar mfit-walker-estop nil
  "As in the reference (M:860-861): walker-adaptive-steps-full clears it on entry (M:865) and
looks at it between launches of the stepping kernel (about every 50 ms of GPU work, where the
reference looks once per iteration, M:904).  Set it from an interrupt handler or another
thread and the walk stops where it is; (request-stop walker) does the same without the
variable.")

(defstruct walker-step
  (prob most-negative-double-float :type float)
  (params nil :type list))

(defstruct walker
  (engine (cffi:null-pointer))          ; mhx_engine* (single device)
  (group (cffi:null-pointer))           ; mhx_group*  (:devices with more than one entry)
  (ranges nil :type list)               ; group: ((first count engine-pointer) ...) per device
  (function nil :type list)
  (param-keys nil :type list)
  (param-style :multiple-kwargs :type symbol)
  (data nil :type list)
  (data-error nil :type list)
  (log-liklihood nil :type list)
  (log-prior nil :type list)
  (n-chains 1 :type integer)
  (n-params 0 :type integer)
  ;; walker-set-create: ((y stddev) ...) of function 0, one entry per walker, whose DATA and
  ;; DATA-ERROR hold walker 0's; nil: every walker fits DATA
  (planes nil :type list))

(defvar *walker-set-planes* nil
  "Bound by walker-set-create around its call of walker-create: (ys sigma sigma-kind thetas) - the
y column of every walker, the stddevs as mhx_set_dataset_planes takes them for SIGMA-KIND (nil:
none), and the starting vector of every walker.  walker-create then hands function 0 its dataset
through mhx_set_dataset_planes and every walker its own first step.")

(defun force-list (item) (if (consp item) item (list item))) ; M:755-759

(defun get-depth (tree)                 ; M:761-772
  (cond ((null tree) nil)
        ((numberp tree) 0)
        ((arrayp tree) (array-rank tree))
        (t (+ 1 (get-depth (elt tree 0))))))

(defun clean-data (data number-of-functions)
  "The layouts walker-create accepts for :data (M:807-825): one dataset (x-column y-column), or
a list of them, one per function; columns may be lists or vectors."
  (let ((depth (get-depth data)))
    (when (and depth (= depth 2))       ; a single dataset: wrap it
      (setf data (list data)
            depth 3))
    ;; one dataset whose x elements are vectors - "multiple or linked independent variables",
    ;; mcmc-fitting.lisp:1136-1137: ((#(a1 b1) #(a2 b2) ...) (y1 y2 ...)) for ONE function
    (when (and depth (= depth 3) (= number-of-functions 1) (= (length data) 2)
               (every #'realp (coerce (second data) 'list)))
      (setf data (list data)
            depth 4))
    (unless (and depth (>= depth 3))
      (error "walker-create: :data must be (x-column y-column) or a list of such datasets"))
    (unless (= (length data) number-of-functions)
      (error "walker-create: ~d dataset~:p for ~d function~:p"
             (length data) number-of-functions))
    (loop for dataset in data
          collect (loop for column in dataset collect (coerce column 'list)))))

(defun clean-data-error (stddev ys)
  "M:774-805 for the layouts the path uses: a number broadcasts; a structure equal to the y
structure is taken as is; anything else broadcasts its first element."
  (labels ((first-element (tree)
             (cond ((null tree) nil)
                   ((numberp tree) tree)
                   (t (first-element (elt tree 0))))))
    (cond ((numberp stddev)
           (mapcar (lambda (y) (make-list (length y) :initial-element stddev)) ys))
          ((and (= (length stddev) (length ys))
                (every (lambda (s y) (and (not (numberp s)) (= (length s) (length y))))
                       stddev ys))
           (mapcar (lambda (s) (coerce s 'list)) stddev))
          ((and (= (length ys) 1) (every #'numberp stddev)
                (= (length stddev) (length (first ys))))
           (list (coerce stddev 'list)))
          (t (let ((v (first-element stddev)))
               (mapcar (lambda (y) (make-list (length y) :initial-element v)) ys))))))

(defun plist-keys (plist)               ; M:190-193, first occurrence wins
  (let ((keys nil))
    (loop for (k nil) on plist by #'cddr
          do (unless (member k keys) (push k keys)))
    (nreverse keys)))

(defun %dataset-of (walker fn-number chain)
  "the dataset (x y) function FN-NUMBER of walker CHAIN fits"
  (let ((data (elt (walker-data walker) fn-number)))
    (if (and (walker-planes walker) (zerop fn-number))
        (list (first data) (first (elt (walker-planes walker) chain)))
        data)))

(defun %stddev-of (walker fn-number chain)
  (if (and (walker-planes walker) (zerop fn-number))
      (second (elt (walker-planes walker) chain))
      (elt (walker-data-error walker) fn-number)))

(defun grouped-p (walker)
  (not (cffi:null-pointer-p (walker-group walker))))

(defun engine-of (walker &optional (chain 0))
  "values: the mhx_engine* that owns global chain CHAIN, and the chain's index on that engine"
  (cond ((grouped-p walker)
         (loop for (first count engine) in (walker-ranges walker)
               when (< -1 (- chain first) count)
                 do (return (values engine (- chain first)))
               finally (error "chain ~d outside the walker's ~d chains" chain
                              (walker-n-chains walker))))
        ((cffi:null-pointer-p (walker-engine walker)) (error "walker has been destroyed"))
        (t (values (walker-engine walker) chain))))

(defun all-engines (walker)
  (if (grouped-p walker)
      (mapcar #'third (walker-ranges walker))
      (list (engine-of walker))))

(defun signal-if-trapped (walker)
  "A frozen chain is where the reference would have signalled an unhandled float trap."
  (loop for (first count engine) in (if (grouped-p walker)
                                         (walker-ranges walker)
                                         (list (list 0 (walker-n-chains walker) (engine-of walker))))
        do (cffi:with-foreign-object (st :int32 count)
             (with-c-call (check (%mhx-get-chain-status engine st (cffi:null-pointer))))
             (dotimes (c count)
               (when (= (cffi:mem-aref st :int32 c) +chain-fp-trap+)
                 (error 'floating-point-invalid-operation
                        :operation 'walker-take-step :operands (list :chain (+ first c))))))))

;;; ------------------------------------------------------------------ walker-create
(defun %set-planes (walker k cx n lik)
  "function K's dataset of a walker set (*walker-set-planes*): the shared x in CX, N points"
  (destructuring-bind (ys sigma sigma-kind thetas) *walker-set-planes*
    (declare (ignore thetas))
    (let ((c (length ys)))
      (cffi:with-foreign-objects ((cy :double (* c n)) (cs :double (max 1 (length sigma))))
        (fill-doubles cy (loop for y in ys append y))
        (fill-doubles cs sigma)
        (with-c-call
          (check (if (grouped-p walker)
                     (%mhx-group-set-dataset-planes (walker-group walker) k cx cy
                                                    (if sigma cs (cffi:null-pointer))
                                                    sigma-kind n lik)
                     (%mhx-set-dataset-planes (walker-engine walker) k cx cy
                                              (if sigma cs (cffi:null-pointer))
                                              sigma-kind n lik))))))))

(defun %define-problem (walker set-function set-function-expr set-dataset set-dataset-cols
                        set-bounds set-prior-expr set-likelihood-expr)
  "walker-create's per-function work (M:1138-1147), through the seven setters of one engine or of
a group (each takes the function index k first and applies CHECK itself)."
  (let* ((keys (walker-param-keys walker)) (d (length keys)))
    (loop for fn in (walker-function walker)
          for k from 0
          for ds in (walker-data walker)
          for sg in (walker-data-error walker)
          for lik in (walker-log-liklihood walker)
          for pri in (walker-log-prior walker)
          do (let* ((idx (mapcar (lambda (key)
                                   (or (position key keys)
                                       (error "function ~d reads key ~s that :params does not supply"
                                              k key)))
                                 (model-keys fn)))
                    (shape (model-shape fn))
                    (n (length (first ds))))
               (cffi:with-foreign-objects ((cidx :int32 (max 1 (length idx)))
                                           (cshape :int32 (max 1 (length shape))))
                 (fill-int32s cidx idx)
                 (fill-int32s cshape shape)
                 (if (model-expr fn)
                     ;; an arbitrary closure body: compiled for gfx950 at init (expr.lisp)
                     (with-c-strings (cnames (mapcar #'mangle-symbol (model-keys fn)))
                       (funcall set-function-expr k (model-expr fn) cnames cidx (length idx)))
                     (funcall set-function k (model-id fn) cshape (length shape) cidx
                              (length idx))))
               (cffi:with-foreign-objects ((cx :double (max 1 n)) (cy :double (max 1 n))
                                           (cs :double (max 1 n)) (cx1 :double (max 1 n))
                                           (cols :pointer 2))
                 (fill-doubles cy (second ds))
                 (fill-doubles cs sg)
                 (if (and (plusp n) (typep (elt (first ds) 0) 'sequence))
                     ;; a vector-valued x (mcmc-fitting.lisp:1136-1137): its two components as
                     ;; columns, (elt x 0) -> xcol0, (elt x 1) -> xcol1 (expr.lisp)
                     (progn
                       (fill-doubles cx (mapcar (lambda (v) (elt v 0)) (first ds)))
                       (fill-doubles cx1 (mapcar (lambda (v) (elt v 1)) (first ds)))
                       (setf (cffi:mem-aref cols :pointer 0) cx
                             (cffi:mem-aref cols :pointer 1) cx1)
                       (funcall set-dataset-cols k cols 2 cy cs n (likelihood-id lik)))
                     (progn
                       (fill-doubles cx (first ds))
                       (funcall set-dataset k cx cy cs n (likelihood-id lik)))))
               (when (likelihood-spec-p lik)
                 (funcall set-likelihood-expr k (likelihood-spec-expr lik)))
               (let ((bounds (cond ((null pri) nil)
                                   ((eq pri 'log-prior-flat) nil)
                                   ((eq pri #'log-prior-flat) nil)
                                   ((prior-bounds-spec-p pri) (prior-bounds-spec-bounds pri))
                                   (t (error 'mhx-error
                                             :code -5
                                             :message ":log-prior must be log-prior-flat or (prior-bounds ...)")))))
                 (cffi:with-foreign-objects ((bi :int32 (max 1 (length bounds)))
                                             (lo :double (max 1 (length bounds)))
                                             (hi :double (max 1 (length bounds))))
                   (fill-int32s bi (mapcar (lambda (b) (or (position (first b) keys) -1)) bounds))
                   (fill-doubles lo (mapcar #'second bounds))
                   (fill-doubles hi (mapcar #'third bounds))
                   (funcall set-bounds k bi lo hi (length bounds)))
                 (when (and (prior-bounds-spec-p pri) (prior-bounds-spec-body-expr pri))
                   (cffi:with-foreign-object (gi :int32 (max 1 d))
                     (fill-int32s gi (loop for i below d collect i))
                     (with-c-strings (cnames (mapcar #'mangle-symbol keys))
                       (funcall set-prior-expr k (prior-bounds-spec-body-expr pri)
                                cnames gi d)))))))))

(defun walker-create (&key function data params data-error log-liklihood log-prior param-bounds
                        (n-chains 1) (device 0) devices (seed 0) (chain-offset 0)
                        (history-capacity 0) (pooled nil))
  "(walker-create &key function data params data-error log-liklihood log-prior param-bounds)
M:1132-1163.  :function takes model designators (models.lisp); everything else as the
reference, single items or lists with one item per function.  N-CHAINS > 1 makes a walker
set that steps as one batch; :DEVICES '(0 1 ...) spreads the set over several GPUs from this
one Lisp image (mhx_group_*: contiguous chain ranges, every GPU busy at once); :POOLED t pools
the adaptive proposal covariance over all chains (one RCCL all-reduce per 200 steps)."
  (declare (ignorable param-bounds))
  (let* ((function (force-list function))
         (k-fns (length function))
         (data (clean-data data k-fns))
         (ys (mapcar #'second data))
         (data-error (clean-data-error (if data-error data-error 1) ys))
         (keys (plist-keys params))
         (d (length keys))
         (values (mapcar (lambda (k) (coerce (getf params k) 'double-float)) keys))
         (liks (if (consp log-liklihood) log-liklihood
                   (make-list k-fns :initial-element log-liklihood)))
         (pris (if (consp log-prior) log-prior (make-list k-fns :initial-element log-prior)))
         (devices (or devices (list device)))
         (grouped (> (length devices) 1))
         (walker (make-walker :function function :param-keys keys :data data
                              :data-error data-error :log-liklihood liks :log-prior pris
                              :n-chains n-chains :n-params d))
         (ok nil))
    (unless (every #'model-p function)
      (error 'mhx-error :code -5 :message ":function must be a model designator (see models.lisp)"))
    (cffi:with-foreign-objects ((cfg '(:struct mhx-config)) (out :pointer)
                                (devs :int32 (length devices)))
      (dotimes (i (cffi:foreign-type-size '(:struct mhx-config)))
        (setf (cffi:mem-aref cfg :uint8 i) 0))
      (setf (cffi:foreign-slot-value cfg '(:struct mhx-config) 'n-chains) n-chains
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'n-params) d
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'n-functions) k-fns
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'device) (first devices)
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'adapt-mode) (if pooled 1 0)
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'seed) seed
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'chain-offset) chain-offset
            (cffi:foreign-slot-value cfg '(:struct mhx-config) 'history-capacity) history-capacity)
      (fill-int32s devs devices)
      (cond (grouped
             (with-c-call (check (%mhx-group-create cfg devs (length devices) out)))
             (setf (walker-group walker) (cffi:mem-ref out :pointer))
             (setf (walker-ranges walker)
                   (loop for i below (%mhx-group-size (walker-group walker))
                         collect (cffi:with-foreign-objects ((first :int64) (count :int64))
                                   (check (%mhx-group-chain-range (walker-group walker) i
                                                                  first count))
                                   (list (cffi:mem-ref first :int64) (cffi:mem-ref count :int64)
                                         (%mhx-group-engine (walker-group walker) i))))))
            (t
             (with-c-call (check (%mhx-create cfg out)))
             (setf (walker-engine walker) (cffi:mem-ref out :pointer)))))
    (unwind-protect
         (let ((e (walker-engine walker)) (g (walker-group walker)))
           (if grouped
               (%define-problem
                walker
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-group-set-function g k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-group-set-function-expr g k a))))
                (lambda (k &rest a)
                  (if *walker-set-planes*
                      (%set-planes walker k (first a) (fourth a) (fifth a))
                      (with-c-call (check (apply #'%mhx-group-set-dataset g k a)))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-group-set-dataset-cols g k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-group-set-bounds g k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-group-set-prior-expr g k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-group-set-likelihood-expr g k a)))))
               (%define-problem
                walker
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-set-function e k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-set-function-expr e k a))))
                (lambda (k &rest a)
                  (if *walker-set-planes*
                      (%set-planes walker k (first a) (fourth a) (fifth a))
                      (with-c-call (check (apply #'%mhx-set-dataset e k a)))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-set-dataset-cols e k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-set-bounds e k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-set-prior-expr e k a))))
                (lambda (k &rest a) (with-c-call (check (apply #'%mhx-set-likelihood-expr e k a))))))
           (let ((thetas (fourth *walker-set-planes*)))  ; (a starting vector per walker)
             (cffi:with-foreign-object (th :double (if thetas (* n-chains d) d))
               (fill-doubles th (if thetas (loop for v in thetas append v) values))
               (with-c-call (check (if grouped
                                       (%mhx-group-init-chains g th (if thetas 0 1))
                                       (%mhx-init-chains e th (if thetas 0 1)))))))
           (setf ok t))
      (unless ok (walker-destroy walker)))
    (signal-if-trapped walker)
    walker))

(defun data-separated (data)
  "The columns of one file, x first, as one dataset (x y) per remaining column: what the
reference's NV tools make of a frequency sweep before they create one walker per dataset."
  (let ((x (elt data 0)))
    (map 'list (lambda (column) (list x column)) (subseq data 1))))

(defun walker-set-create (&key function datasets params data-error log-liklihood log-prior
                            (device 0) devices (seed 0) (chain-offset 0) (history-capacity 0))
  "A walker set in which every walker fits a dataset of its own over a shared x.  DATASETS: a list
of (x y), one per walker, every x the same numbers; PARAMS: one plist for all walkers or a list of
one plist per walker with the same keys in the same order; DATA-ERROR: nil, one number, one number
per walker, one list per point, or one list per point per walker.  One function, the normal
likelihood.  The result is an ordinary walker of (length DATASETS) chains that walk in one launch:
walker c does what a single walker on dataset c would do."
  (let* ((c (length datasets))
         (x (map 'list (lambda (v) (coerce v 'double-float)) (first (first datasets))))
         (n (length x))
         (ys (loop for ds in datasets
                   for i from 0
                   do (unless (and (= (length (first ds)) n)
                                   (every (lambda (a b) (eql (coerce a 'double-float) b))
                                          (first ds) x))
                        (error "walker-set-create: walker ~d: its x differs from walker 0's" i))
                      (unless (= (length (second ds)) n)
                        (error "walker-set-create: walker ~d: y must be as long as x" i))
                   collect (coerce (second ds) 'list)))
         (plists (if (keywordp (first params)) (make-list c :initial-element params) params))
         (keys (plist-keys (first plists)))
         (thetas (loop for pl in plists
                       for i from 0
                       do (unless (equal (plist-keys pl) keys)
                            (error "walker-set-create: walker ~d: its params have other keys, or another order, than walker 0's" i))
                       collect (mapcar (lambda (k) (coerce (getf pl k) 'double-float)) keys))))
    (unless (= (length plists) c)
      (error "walker-set-create: ~d parameter lists for ~d walkers" (length plists) c))
    (multiple-value-bind (sigma kind rows)
        (cond ((null data-error)
               (values nil +sigma-none+
                       (make-list c :initial-element (make-list n :initial-element 1))))
              ((numberp data-error)
               (values (make-list c :initial-element data-error) +sigma-per-chain+
                       (make-list c :initial-element (make-list n :initial-element data-error))))
              ((and (= (length data-error) c) (every #'numberp data-error))
               (values (coerce data-error 'list) +sigma-per-chain+
                       (map 'list (lambda (s) (make-list n :initial-element s)) data-error)))
              ((and (= (length data-error) n) (every #'numberp data-error))
               (values (coerce data-error 'list) +sigma-shared+
                       (make-list c :initial-element (coerce data-error 'list))))
              ((and (= (length data-error) c)
                    (every (lambda (s) (and (not (numberp s)) (= (length s) n))) data-error))
               (values (loop for s in (coerce data-error 'list) append (coerce s 'list))
                       +sigma-per-point+
                       (map 'list (lambda (s) (coerce s 'list)) data-error)))
              (t (error "walker-set-create: :data-error must be nil, a number, one number per walker, one list per point, or one list per point per walker")))
      (let* ((*walker-set-planes* (list ys sigma kind thetas))
             (walker (walker-create :function function :data (list x (first ys))
                                    :params (first plists) :data-error (first rows)
                                    :log-liklihood log-liklihood :log-prior log-prior
                                    :n-chains c :device device :devices devices :seed seed
                                    :chain-offset chain-offset
                                    :history-capacity history-capacity)))
        (setf (walker-planes walker) (mapcar #'list ys rows))
        walker))))

(defun walker-destroy (walker)
  (cond ((grouped-p walker)
         (with-c-call (%mhx-group-destroy (walker-group walker)))
         (setf (walker-group walker) (cffi:null-pointer)
               (walker-ranges walker) nil))
        ((not (cffi:null-pointer-p (walker-engine walker)))
         (with-c-call (%mhx-destroy (walker-engine walker)))
         (setf (walker-engine walker) (cffi:null-pointer))))
  nil)

(defun request-stop (walker)
  "What (setf mfit-walker-estop t) does in the reference (M:860-861, polled at M:904)."
  (if (grouped-p walker)
      (with-c-call (check (%mhx-group-request-stop (walker-group walker))))
      (with-c-call (check (%mhx-request-stop (engine-of walker))))))

;;; ------------------------------------------------------------------ state read-back
(defun %state (walker chain)
  "values: theta prob best-theta best-prob length age  of chain CHAIN (d doubles cross the ABI,
not the state of every chain)"
  (multiple-value-bind (e c) (engine-of walker chain)
    (let ((d (walker-n-params walker)))
      (cffi:with-foreign-objects ((th :double d) (lp :double) (bt :double d) (bl :double)
                                  (ln :int64) (ag :int64))
        (with-c-call (check (%mhx-get-chain e c th lp bt bl ln ag)))
        (values (read-doubles th d) (cffi:mem-ref lp :double)
                (read-doubles bt d) (cffi:mem-ref bl :double)
                (cffi:mem-ref ln :int64) (cffi:mem-ref ag :int64))))))

(defun %plist (walker vec)
  (loop for k in (walker-param-keys walker)
        for i from 0
        append (list k (aref vec i))))

(defun walker-last-step (walker &optional (chain 0))
  (multiple-value-bind (th lp) (%state walker chain)
    (make-walker-step :prob lp :params (%plist walker th))))

(defun walker-most-likely-step (walker &optional (chain 0))
  (multiple-value-bind (th lp bt bl) (%state walker chain)
    (declare (ignore th lp))
    (make-walker-step :prob bl :params (%plist walker bt))))

(defun walker-length (walker &optional (chain 0))
  (nth-value 4 (%state walker chain)))

(defun walker-age (walker &optional (chain 0))
  (nth-value 5 (%state walker chain)))

(defun walker-chain-status (walker)
  (loop for e in (all-engines walker)
        for n in (if (grouped-p walker)
                     (mapcar #'second (walker-ranges walker))
                     (list (walker-n-chains walker)))
        append (cffi:with-foreign-object (st :int32 n)
                 (with-c-call (check (%mhx-get-chain-status e st (cffi:null-pointer))))
                 (loop for c below n collect (cffi:mem-aref st :int32 c)))))

(defun walker-kernel-name (walker)
  "Which kernels serve this walker's problem, e.g. \"w8/lorder_normal\" or
\"w8/rtc[expr:normal] split x24\" (mhx_kernel_name)."
  (with-c-call (%mhx-kernel-name (engine-of walker))))

(defun %trace (walker chain take)
  "newest-first list of walker-steps, (walker-get :get :steps :take take)"
  (multiple-value-bind (e c) (engine-of walker chain)
    (let* ((d (walker-n-params walker))
           (take (max 1 take)))
      (cffi:with-foreign-objects ((pr :double take) (th :double (* take d)) (n-out :int))
        (with-c-call (check (%mhx-get-trace e c take pr th n-out)))
        ;; the reference keeps every step of a walk (M:549), the engine the newest
        ;; history-capacity in its device ring: a window that reaches past the ring is answered
        ;; with what is there, and says so
        (when (< (cffi:mem-ref n-out :int) take)
          (warn "walker-get :take ~d: the device history ring holds the newest ~d steps of this walk; create the walker with :history-capacity >= the walk's length to keep them all"
                take (cffi:mem-ref n-out :int)))
        (loop for s below (cffi:mem-ref n-out :int)
              collect (make-walker-step
                       :prob (cffi:mem-aref pr :double s)
                       :params (%plist walker (read-doubles (cffi:inc-pointer th (* 8 s d)) d))))))))

(defun walker-walk (walker &optional (chain 0))
  (%trace walker chain (walker-length walker chain)))

(defun walker-modify (walker &key modify burn-number keep-number &allow-other-keys)
  "M:547-580.  :add-step happens on the device inside walker-take-step; :add-walks is unused
by the reference itself (M:556 discards the nconc)."
  (flet ((each (action n)
           (dolist (e (all-engines walker))
             (with-c-call (check (%mhx-walker-modify e action n))))))
    (ecase modify
      (:burn-walks (each 0 burn-number))
      (:keep-walks (each 1 keep-number))
      (:reset (each 2 0) walker)
      (:reset-to-most-likely (each 3 0) walker)
      (:delete (walker-destroy walker)))))

;;; ------------------------------------------------------------------ stepping
(defun %fill-matrix (lm l-matrix d)
  (dotimes (i d lm)
    (dotimes (j d)
      (setf (cffi:mem-aref lm :double (+ (* i d) j)) (coerce (aref l-matrix i j) 'double-float)))))

(defun %with-matrix (l-matrix d fn)
  (cffi:with-foreign-object (lm :double (* d d))
    (funcall fn (%fill-matrix lm l-matrix d))))

(defun diagonal-covariance (values)
  "a d x d matrix with VALUES on its diagonal (M:605-611)"
  (let* ((d (length values))
         (a (make-array (list d d) :element-type 'double-float :initial-element 0d0)))
    (loop for v in values
          for i from 0
          do (setf (aref a i i) (coerce v 'double-float)))
    a))

(defun walker-adaptive-steps-full (walker &key (n 100000) (temperature 1d3)
                                            (auto :prob-settle)
                                            (sampling-optimization :covariance)
                                            max-walker-length l-matrix)
  "M:862-942.  The do loop runs on the GPU in launches of about 50 ms; between launches this
function looks at MFIT-WALKER-ESTOP, as the reference does at the top of every iteration
(M:904), and raises the device's stop flag when it is set.  :auto :slope-settle and
:sampling-optimization :best-value are outside the accelerated path and signal MHX-ERROR."
  (unless (eq sampling-optimization :covariance)
    (error 'mhx-error :code -5 :message ":best-value is outside the accelerated path"))
  (when (eq auto :slope-settle)
    (error 'mhx-error :code -5 :message ":slope-settle is outside the accelerated path"))
  (setf mfit-walker-estop nil)          ; M:865
  (let* ((d (walker-n-params walker))
         (grouped (grouped-p walker))
         (g (walker-group walker))
         (e (engine-of walker)))
    (cffi:with-foreign-objects ((o '(:struct mhx-run-opts)) (lm :double (* d d))
                                (running :int64) (avg :double) (launches :uint64)
                                (total :double))
      (%mhx-run-opts-default o)
      (setf (cffi:foreign-slot-value o '(:struct mhx-run-opts) 'n) (floor n)
            (cffi:foreign-slot-value o '(:struct mhx-run-opts) 'temperature)
            (coerce temperature 'double-float)
            (cffi:foreign-slot-value o '(:struct mhx-run-opts) 'auto-mode) (if auto 1 0)
            (cffi:foreign-slot-value o '(:struct mhx-run-opts) 'max-walker-length)
            (if max-walker-length (floor max-walker-length) 0)
            (cffi:foreign-slot-value o '(:struct mhx-run-opts) 'l-matrix-per-chain) 0
            (cffi:foreign-slot-value o '(:struct mhx-run-opts) 'l-matrix)
            (if l-matrix (%fill-matrix lm l-matrix d) (cffi:null-pointer)))
      (with-c-call (check (if grouped
                              (%mhx-group-adaptive-begin g o)
                              (%mhx-adaptive-begin e o))))
      ;; M:902-942 in launches; the launch length follows the measured time per iteration
      (let ((chunk 16) (stop-sent nil))
        (loop
          (when (and mfit-walker-estop (not stop-sent))
            (request-stop walker)
            (setf stop-sent t))
          (with-c-call (check (%mhx-kernel-timing e 1 avg launches total)))
          (with-c-call (check (if grouped
                                  (%mhx-group-adaptive-advance g chunk running)
                                  (%mhx-adaptive-advance e chunk running))))
          (when (zerop (cffi:mem-ref running :int64)) (return))
          (with-c-call (check (%mhx-kernel-timing e 0 avg launches total)))
          (let ((ms (cffi:mem-ref total :double)))
            (when (> ms 0d0)
              (setf chunk (max 8 (min 65536 (floor (* chunk 50d0) ms))))))))))
  (signal-if-trapped walker)
  nil)

(defun walker-adaptive-steps (walker &optional (n 30000))
  "M:946-947"
  (walker-adaptive-steps-full walker :n n :temperature 10 :auto :prob-settle))

(defun mcmc-fit (&rest args &key function data params data-error log-liklihood log-prior
                              param-bounds &allow-other-keys)
  "M:1165-1175"
  (declare (ignore function data params data-error log-liklihood log-prior param-bounds))
  (let ((walker (apply #'walker-create args)))
    (walker-adaptive-steps walker)
    walker))

(defun %scaled-diagonal (plist)
  "(diagonal-covariance (plist-values (scale-plist 1e-2 plist))) of M:851 / M:1074.  The 1e-2 is
a SINGLE float there, so every entry is (* 1e-2 value) with the single widened to a double."
  (diagonal-covariance (loop for (nil v) on plist by #'cddr collect (* 1e-2 v))))

(defun walker-many-steps (walker n &optional l-matrix)
  "(walker-many-steps the-walker n &optional l-matrix) M:849-853: N steps with a constant
l-matrix, temperature 1; without one, 1e-2 of the median parameters on the diagonal (M:851)."
  (let ((l-matrix (or l-matrix
                      (%scaled-diagonal (walker-get walker :get :median-params)))))
    (%with-matrix l-matrix (walker-n-params walker)
                  (lambda (lm)
                    (dolist (e (all-engines walker))
                      (with-c-call (check (%mhx-many-steps e n lm 0)))))))
  (signal-if-trapped walker)
  nil)

(defun walker-take-step (walker &key l-matrix (temperature 1))
  "(walker-take-step walker &key l-matrix (temperature 1)) M:1072-1095: one step of every chain
with the device's own randomness (the reference draws its own too, M:687 / M:1092); without an
l-matrix, 1e-2 of the most likely parameters on the diagonal (M:1074)."
  (let ((l-matrix (or l-matrix
                      (%scaled-diagonal (walker-get walker :get :most-likely-params :take 1000)))))
    (%with-matrix l-matrix (walker-n-params walker)
                  (lambda (lm)
                    (dolist (e (all-engines walker))
                      (with-c-call
                        (check (%mhx-take-step e lm 0 (coerce temperature 'double-float))))))))
  (signal-if-trapped walker)
  walker)

(defun walker-take-step-injected (walker &key l-matrix (temperature 1) z u)
  "The parity hook: M:1072-1095 for a single-chain walker with the CALLER's randomness, Z = the d
numbers alexandria:gaussian-random would return (M:687), U = (random 1.0d0) (M:1092).
Returns true when the proposal was taken."
  (let* ((e (engine-of walker)) (d (walker-n-params walker)))
    (unless (= (walker-n-chains walker) 1)
      (error "walker-take-step-injected: single-chain walkers only"))
    (%with-matrix
     l-matrix d
     (lambda (lm)
       (cffi:with-foreign-objects ((cz :double d) (cu :double) (ct :double) (acc :uint8))
         (fill-doubles cz z)
         (setf (cffi:mem-ref cu :double) (coerce u 'double-float)
               (cffi:mem-ref ct :double) (coerce temperature 'double-float))
         (with-c-call (check (%mhx-step-injected e lm 0 cz cu ct acc)))
         (signal-if-trapped walker)
         (= 1 (cffi:mem-ref acc :uint8)))))))

;;; ------------------------------------------------------------------ walker-get M:487-543
(defun median (sequence)                ; nth-percentile 50, M:1493-1517
  (let* ((copy (sort (copy-seq sequence) #'<))
         (n (* 50 (- (length copy) 1) 1/100)))
    (multiple-value-bind (pos rem) (floor n)
      (if (= rem 0)
          (elt copy pos)
          (/ (+ (elt copy pos) (elt copy (+ pos 1))) 2)))))

(defun %covariance-of-plists (plists keys)
  "Population covariance of the parameter vectors in PLISTS (what lplist-covariance, M:614-643,
gives for :covariance-matrix): averages first, then for every matrix entry the sum over the
vectors of (x_i - mean_i)(x_j - mean_j) / n, the division inside the sum."
  (let* ((n (length plists))
         (d (length keys))
         (rows (mapcar (lambda (pl) (mapcar (lambda (k) (getf pl k)) keys)) plists))
         (means (loop for i below d
                      collect (/ (loop for row in rows sum (nth i row)) n)))
         (cov (make-array (list d d) :element-type 'double-float :initial-element 0d0)))
    (dotimes (i d cov)
      (dotimes (j d)
        (let ((mi (nth i means)) (mj (nth j means)) (acc 0d0))
          (dolist (row rows)
            (incf acc (/ (* (- (nth i row) mi) (- (nth j row) mj)) n)))
          (setf (aref cov i j) acc))))))

(defun walker-get (walker &key (get :steps) take param (chain 0))
  (let* ((len (walker-length walker chain))
         (take (if take (min len take) len))
         (d (walker-n-params walker))
         (keys (walker-param-keys walker)))
    (flet ((steps () (%trace walker chain take)))
      (case get
        (:steps (steps))
        (:log-liklihoods (mapcar #'walker-step-prob (steps)))
        (:params (mapcar #'walker-step-params (steps)))
        (:param (mapcar (lambda (s) (getf (walker-step-params s) param)) (steps)))
        (:unique-steps
         ;; the parameters of every step whose prob differs from that of the step before it in
         ;; time (the walk is newest first; the oldest step always counts), M:492-496
         (loop for (newer older) on (steps)
               unless (and older (equal (walker-step-prob newer) (walker-step-prob older)))
                 collect (walker-step-params newer)))
        (:forward-steps
         ;; the parameters of every step that improved on the one before it, M:497-502
         (loop for (newer older) on (steps)
               when (and older (> (walker-step-prob newer) (walker-step-prob older)))
                 collect (walker-step-params newer)))
        (:most-likely-step
         (reduce (lambda (x y) (if (> (walker-step-prob x) (walker-step-prob y)) x y)) (steps)))
        (:most-likely-params (walker-step-params (walker-most-likely-step walker chain)))
        (:median-params
         (let ((s (steps)))
           (loop for k in keys
                 append (list k (median (mapcar (lambda (st) (getf (walker-step-params st) k)) s))))))
        (:acceptance
         (multiple-value-bind (e c) (engine-of walker chain)
           (let ((n (if (grouped-p walker)
                        (second (find e (walker-ranges walker) :key #'third :test #'cffi:pointer-eq))
                        (walker-n-chains walker))))
             (cffi:with-foreign-object (out :double n)
               (with-c-call (check (%mhx-get-acceptance e (max 1 take) out)))
               (/ (round (* (cffi:mem-aref out :double c) take)) take)))))
        (:l-matrix
         (multiple-value-bind (e c) (engine-of walker chain)
           (cffi:with-foreign-objects ((lm :double (* d d)) (st :int) (nf :int))
             (with-c-call (check (%mhx-get-proposal-factor e c (max 1 take) lm st nf)))
             (case (cffi:mem-ref st :int)
               (0 (let ((a (make-array (list d d) :element-type 'double-float)))
                    (dotimes (i d a)
                      (dotimes (j d)
                        (setf (aref a i j) (cffi:mem-aref lm :double (+ (* i d) j)))))))
               (1 (error 'division-by-zero :operation 'cholesky-decomp :operands nil))
               (2 (error 'floating-point-invalid-operation :operation 'cholesky-decomp
                                                            :operands nil))
               (t (make-array '(0 0) :element-type 'double-float))))))
        (:stddev-params
         ;; M:525-539: the diagonal of the l-matrix (0d0 while the walk is shorter than 10);
         ;; the l-matrix itself is the second value
         (if (< len 10)
             (loop for k in keys append (list k 0d0))
             (let ((l (walker-get walker :get :l-matrix :take take :chain chain)))
               (values (loop for k in keys
                             for i from 0
                             append (list k (aref l i i)))
                       l))))
        (:covariance-matrix             ; M:541
         (%covariance-of-plists (walker-get walker :get :unique-steps :take take :chain chain)
                                keys))
        (t (error "walker-get: unknown :get ~s" get))))))

;;; ------------------------------------------------------------------ walker-set-get M:1029-1030
;;; walker-get mapped over the set.  The summarising selectors are ONE batched device call for all
;;; chains (mhx_get_percentiles / _covariances / _proposal_factors / _window_best, or their
;;; mhx_group_get_* forms): no history crosses to the host.  The list-valued selectors are ONE
;;; mhx_get_traces call: the device filters, and only the columns the selector reads come back.
(defun %set-call (walker engine-fn group-fn &rest args)
  "ENGINE-FN on the walker's engine or GROUP-FN on its group, ARGS after the handle"
  (with-c-call
    (check (if (grouped-p walker)
               (apply group-fn (walker-group walker) args)
               (apply engine-fn (engine-of walker) args)))))

(defun %set-lengths (walker)
  "(walker-length w) of every chain, read once"
  (let ((n (walker-n-chains walker))
        (none (cffi:null-pointer)))
    (cffi:with-foreign-object (ln :int64 n)
      (%set-call walker #'%mhx-get-state #'%mhx-group-get-state none none none none ln none)
      (loop for c below n collect (cffi:mem-aref ln :int64 c)))))

(defun %l-matrix-value (status matrix)
  "what (walker-get :get :l-matrix) makes of the device's status"
  (case status
    (0 matrix)
    (1 (error 'division-by-zero :operation 'cholesky-decomp :operands nil))
    (2 (error 'floating-point-invalid-operation :operation 'cholesky-decomp :operands nil))
    (t (make-array '(0 0) :element-type 'double-float))))

(defun %set-traces (walker window filter stride start cols envelope)
  "mhx_get_traces for every chain of the set: the columns COLS (places in the parameter vector, -1
the step's prob) of every STRIDE-th step FILTER (0 every step, 1 :unique-steps, 2 :forward-steps)
keeps of the newest WINDOW, from the START-th on.  Values: the rows ROWS carved per chain, the
vectors VALUES, LO and HI [n][rows][n-cols] (LO and HI nil without ENVELOPE) and the lists n-out,
n-kept, n-used."
  (let* ((n (walker-n-chains walker))
         (nc (length cols))
         (rows (max 1 (cffi:with-foreign-object (r :int64)
                        (with-c-call (check (%mhx-trace-rows window stride start r)))
                        (cffi:mem-ref r :int64))))
         (count (* n rows nc))
         (vals (cffi:foreign-alloc :double :count count))
         (lo (if envelope (cffi:foreign-alloc :double :count count) (cffi:null-pointer)))
         (hi (if envelope (cffi:foreign-alloc :double :count count) (cffi:null-pointer))))
    (unwind-protect
         (cffi:with-foreign-objects ((colp :int32 nc) (n-out :int32 n) (n-kept :int32 n)
                                     (n-used :int32 n))
           (fill-int32s colp cols)
           (%set-call walker #'%mhx-get-traces #'%mhx-group-get-traces
                      window filter stride start colp nc rows vals lo hi n-out n-kept n-used)
           (flet ((doubles (ptr)
                    (if (cffi:null-pointer-p ptr) nil (read-doubles ptr count)))
                  (ints (ptr)
                    (loop for c below n collect (cffi:mem-aref ptr :int32 c))))
             (values rows (doubles vals) (doubles lo) (doubles hi)
                     (ints n-out) (ints n-kept) (ints n-used))))
      (cffi:foreign-free vals)
      (unless (cffi:null-pointer-p lo) (cffi:foreign-free lo))
      (unless (cffi:null-pointer-p hi) (cffi:foreign-free hi)))))

(defun walker-set-get (walker &key (get :steps) take param)
  "(walker-set-get the-walker-set &key get take param) M:1029-1030 over a batched walker: a list
with one entry per chain, each what (walker-get walker :get get :take take :chain c) returns.  A
condition is signalled for the first chain walker-get would signal it for, as mapcar would."
  (let* ((n (walker-n-chains walker))
         (d (walker-n-params walker))
         (keys (walker-param-keys walker))
         (lengths (%set-lengths walker))
         (longest (reduce #'max lengths))
         (wanted (max 1 (if take (min take longest) longest)))
         (ring (cffi:with-foreign-object (cap :int32)
                 (with-c-call
                   (check (%mhx-get-history-capacity (first (all-engines walker)) cap)))
                 (cffi:mem-ref cap :int32)))
         (window (min wanted ring))
         (none (cffi:null-pointer)))
    (flet ((per-chain ()
             (loop for c below n
                   collect (walker-get walker :get get :take take :param param :chain c)))
           (note-truncation ()
             (when (> wanted ring)
               (warn "walker-set-get ~s :take ~d: the device history ring holds the newest ~d steps of a walk; create the walker with :history-capacity >= the walks' length to keep them all"
                     get wanted ring)))
           (plist-at (ptr offset)
             (%plist walker (read-doubles (cffi:inc-pointer ptr (* 8 offset)) d)))
           (matrix-at (ptr offset)
             (let ((a (make-array (list d d) :element-type 'double-float)))
               (dotimes (i d a)
                 (dotimes (j d)
                   (setf (aref a i j) (cffi:mem-aref ptr :double (+ offset (* i d) j)))))))
           (listed ()
             ;; M:490-502, M:509-510, M:540: the steps themselves, filtered on the device
             (let* ((every (loop for j below d collect j))
                    (column (and (eq get :param) (position param keys)))
                    (cols (case get
                            (:steps (cons -1 every))
                            (:log-liklihoods (list -1))
                            (:param (list (or column -1)))
                            (t every)))
                    (nc (length cols)))
               (multiple-value-bind (rows v lo hi n-out n-kept n-used)
                   (%set-traces walker window
                                (case get (:unique-steps 1) (:forward-steps 2) (t 0))
                                1 0 cols nil)
                 (declare (ignore lo hi n-kept))
                 (when (some (lambda (used len) (< used (if take (min take len) len)))
                             n-used lengths)
                   (warn "walker-set-get ~s :take ~d: the device history ring holds the newest ~d steps of a walk; create the walker with :history-capacity >= the walks' length to keep them all"
                         get wanted ring))
                 (flet ((plist-from (at)
                          (loop for k in keys
                                for j from at
                                append (list k (aref v j)))))
                   (loop for c below n
                         for held in n-out
                         collect (loop for r below held
                                       collect (let ((at (* nc (+ (* c rows) r))))
                                                 (case get
                                                   (:steps (make-walker-step
                                                            :prob (aref v at)
                                                            :params (plist-from (1+ at))))
                                                   (:log-liklihoods (aref v at))
                                                   (:param (and column (aref v at)))
                                                   (t (plist-from at)))))))))))
      (case get
        (:median-params                 ; nth-percentile 50 of every parameter, M:516-523
         (cffi:with-foreign-objects ((num :int32) (den :int32) (out :double (* n d)))
           (setf (cffi:mem-ref num :int32) 50
                 (cffi:mem-ref den :int32) 1)
           (%set-call walker #'%mhx-get-percentiles #'%mhx-group-get-percentiles
                      window num den 1 out none)
           (note-truncation)
           (loop for c below n collect (plist-at out (* c d)))))
        (:covariance-matrix             ; M:541
         (cffi:with-foreign-object (cov :double (* n d d))
           (%set-call walker #'%mhx-get-covariances #'%mhx-group-get-covariances
                      window cov none none)
           (note-truncation)
           (loop for c below n collect (matrix-at cov (* c d d)))))
        (:most-likely-step              ; M:503-505 over the window
         (cffi:with-foreign-objects ((pr :double n) (th :double (* n d)))
           (%set-call walker #'%mhx-get-window-best #'%mhx-group-get-window-best window pr th)
           (note-truncation)
           (loop for c below n
                 collect (make-walker-step :prob (cffi:mem-aref pr :double c)
                                           :params (plist-at th (* c d))))))
        ((:l-matrix :stddev-params)     ; M:543, M:525-539
         (if (> wanted ring)
             (per-chain)        ; walker-get signals what the device says of such a window
             (cffi:with-foreign-objects ((lm :double (* n d d)) (st :int32 n))
               (%set-call walker #'%mhx-get-proposal-factors #'%mhx-group-get-proposal-factors
                          window lm st none)
               (loop for c below n
                     for len in lengths
                     collect (if (and (eq get :stddev-params) (< len 10))
                                 (loop for k in keys append (list k 0d0))
                                 (let ((l (%l-matrix-value (cffi:mem-aref st :int32 c)
                                                           (matrix-at lm (* c d d)))))
                                   (if (eq get :l-matrix)
                                       l
                                       (loop for k in keys
                                             for i from 0
                                             append (list k (aref l i i))))))))))
        ((:steps :params :param :log-liklihoods :unique-steps :forward-steps)
         (if (and take (< take 1))
             (per-chain)                ; no window the device could be asked for
             (listed)))
        (t (per-chain))))))

;;; ------------------------------------------------------------------ histograms M:1361-1369, M:1541-1564
;;; walker-param-histo without the plot, and for a whole walker set the same counts - and the
;;; corner plot as grids of pair counts - from the device (mhx_get_histograms, mhx_get_pair_grids):
;;; the boundaries are make-histo's own, formed here with rationals; no history crosses to the host.
(defun %histo-x (bottom top num-bins)
  "make-histo-x's list M:1563-1564 from the extremes (one bin: the reference divides by zero in a
linspace of one element; the bin's centre is returned)"
  (let ((start (+ bottom (/ (/ (- top bottom) num-bins) 2))))
    (if (= num-bins 1)
        (list (coerce start 'double-float))
        (%even-grid start top num-bins))))

(defun make-histo (sequence num-bins)
  "(make-histo sequence num-bins) M:1542-1557 on an ascending SEQUENCE: count n is the number of
elements not yet counted that are <= boundary n of (linspace bottom top :len (1+ num-bins)).
NUM-BINS is required: the reference's automatic count is not mirrored."
  (let* ((bottom (reduce #'min sequence))
         (top (reduce #'max sequence))
         (boundaries (%even-grid bottom top (1+ num-bins)))
         (left (coerce sequence 'list)))
    (loop for boundary in (cdr boundaries)
          collect (let ((pos (or (position-if (lambda (v) (> v boundary)) left)
                                 (length left))))
                    (setf left (nthcdr pos left))
                    pos))))

(defun make-histo-x (sequence num-bins)
  "(make-histo-x sequence num-bins) M:1559-1564"
  (%histo-x (reduce #'min sequence) (reduce #'max sequence) num-bins))

(defun walker-param-histo (walker key &key (take 10000) (bins 20) (chain 0))
  "(walker-param-histo walker key &key take bins) M:1361-1369 without the plot: the list
(histo-x histo) the reference hands to gnuplot"
  (let ((ascending (sort (copy-seq (walker-get walker :get :param :param key :take take :chain chain))
                         #'<)))
    (list (make-histo-x ascending bins) (make-histo ascending bins))))

(defun %bin-window (walker take who)
  "the window the device serves for :take TAKE (nil: every walk whole), warning when a walk's
window reaches past the ring"
  (let* ((longest (reduce #'max (%set-lengths walker)))
         (wanted (max 1 (if take (min take longest) longest)))
         (ring (cffi:with-foreign-object (cap :int32)
                 (with-c-call
                   (check (%mhx-get-history-capacity (first (all-engines walker)) cap)))
                 (cffi:mem-ref cap :int32))))
    (when (> wanted ring)
      (warn "~a :take ~d: the device history ring holds the newest ~d steps of a walk; create the walker with :history-capacity >= the walks' length to keep them all"
            who wanted ring))
    (min wanted ring)))

(defun %key-columns (walker keys)
  "the places of KEYS (nil: all) among the walker's parameter keys"
  (let ((all (walker-param-keys walker)))
    (loop for k in (or keys all)
          collect (or (position k all)
                      (error "~s is no parameter key of the walker" k)))))

(defun %fill-reference-edges (walker window cols bins edges)
  "make-histo's boundaries of every chain and column into EDGES [n][nc][bins + 1], from the 0 and
100 per cent points of the window (mhx_get_percentiles); returns the extremes ((lo hi) ...) per
chain and column"
  (let ((n (walker-n-chains walker))
        (d (walker-n-params walker))
        (nc (length cols))
        (none (cffi:null-pointer)))
    (cffi:with-foreign-objects ((num :int32 2) (den :int32 2) (out :double (* n 2 d)))
      (fill-int32s num '(0 100))
      (fill-int32s den '(1 1))
      (%set-call walker #'%mhx-get-percentiles #'%mhx-group-get-percentiles window num den 2 out none)
      (loop for c below n
            collect (loop for p in cols
                          for j from 0
                          collect (let ((lo (cffi:mem-aref out :double (+ (* c 2 d) p)))
                                        (hi (cffi:mem-aref out :double (+ (* c 2 d) d p))))
                                    (fill-doubles (cffi:inc-pointer edges (* 8 (1+ bins) (+ (* c nc) j)))
                                                  (%even-grid lo hi (1+ bins)))
                                    (list lo hi)))))))

(defun walker-set-param-histo (walker &key keys (take 10000) (bins 20))
  "walker-param-histo for every chain of the set and every key of KEYS (nil: all) from three
device calls: a list with, chain by chain, the plist (key (histo-x histo) ...)"
  (let* ((n (walker-n-chains walker))
         (cols (%key-columns walker keys))
         (names (or keys (walker-param-keys walker)))
         (nc (length cols))
         (window (%bin-window walker take "walker-set-param-histo"))
         (none (cffi:null-pointer)))
    (cffi:with-foreign-objects ((edges :double (* n nc (1+ bins))) (colp :int32 nc)
                                (counts :int32 (* n nc bins)))
      (fill-int32s colp cols)
      (let ((extremes (%fill-reference-edges walker window cols bins edges)))
        (%set-call walker #'%mhx-get-histograms #'%mhx-group-get-histograms
                   window colp nc bins edges 1 counts none none none)
        (loop for c below n
              for chain-extremes in extremes
              collect (loop for k in names
                            for j from 0
                            for (lo hi) in chain-extremes
                            append (list k (list (%histo-x lo hi bins)
                                                 (loop for b below bins
                                                       collect (cffi:mem-aref counts :int32
                                                                              (+ (* bins (+ (* c nc) j)) b)))))))))))

(defun %permute-params (params)
  "walker-plot-corner's pair list M:1334-1340"
  (loop for (head . others) on params
        append (loop for other in others collect (list head other))))

(defun walker-set-corner-grid (walker &key take (bins 20) keys)
  "walker-plot-corner M:1333-1359 as counts: for every chain of the set a list of ((key1 key2) grid)
in the reference's pair order, GRID a BINS x BINS array whose cell (i j) counts the steps with key1
in bin i+1 and key2 in bin j+1 of make-histo's boundaries for that chain and key.  TAKE nil: the
whole walk."
  (let* ((n (walker-n-chains walker))
         (cols (%key-columns walker keys))
         (names (or keys (walker-param-keys walker)))
         (nc (length cols))
         (places (%permute-params (loop for j below nc collect j)))
         (np (length places))
         (window (%bin-window walker take "walker-set-corner-grid"))
         (none (cffi:null-pointer)))
    (cffi:with-foreign-objects ((edges :double (* n nc (1+ bins))) (colp :int32 nc)
                                (pa :int32 (max 1 np)) (pb :int32 (max 1 np))
                                (counts :int32 (max 1 (* n np bins bins))))
      (fill-int32s colp cols)
      (fill-int32s pa (mapcar #'first places))
      (fill-int32s pb (mapcar #'second places))
      (%fill-reference-edges walker window cols bins edges)
      (%set-call walker #'%mhx-get-pair-grids #'%mhx-group-get-pair-grids
                 window colp nc pa pb np bins edges 1 counts none none none)
      (loop for c below n
            collect (loop for (a b) in places
                          for q from 0
                          collect (let ((grid (make-array (list bins bins) :element-type 'fixnum)))
                                    (dotimes (i bins)
                                      (dotimes (j bins)
                                        (setf (aref grid i j)
                                              (cffi:mem-aref counts :int32
                                                             (+ (* bins bins (+ (* c np) q)) (* i bins) j)))))
                                    (list (list (elt names a) (elt names b)) grid)))))))

;;; ------------------------------------------------------------------ traces as arrays
;;; What walker-catepillar-plots M:1294-1309, walker-liklihood-plot M:1313-1320 and
;;; walker-plot-one-corner M:1322-1331 draw, for every walker of a set, as arrays: one
;;; mhx_get_traces call, thinned on the device with the reference's `thin` M:149-157.
(defun walker-set-trace (walker &key keys take (thin 1) (start 0) (which :steps) envelope (prob t))
  "The steps of every chain of the set as arrays [n-chains][rows], newest first: a plist of
:values (key array ...) for KEYS (nil: all), :prob (the steps' log-posteriors, nil unless PROB),
:n-out, :n-kept and :n-used (lists: rows written, steps WHICH kept, steps the window held; the
rows of chain c beyond its n-out are zero) and, with ENVELOPE, :lo and :hi (key array ...),
:prob-lo and :prob-hi: the smallest and greatest value among the THIN kept steps a row stands
for.  WHICH: :steps, :unique-steps or :forward-steps; THIN, START: (thin list thin start) of what
WHICH keeps; TAKE nil: every walk whole."
  (let* ((n (walker-n-chains walker))
         (names (or keys (walker-param-keys walker)))
         (cols (append (if prob (list -1) nil) (%key-columns walker keys)))
         (nc (length cols))
         (lead (if prob 1 0))
         (window (%bin-window walker take "walker-set-trace")))
    (multiple-value-bind (rows v lo hi n-out n-kept n-used)
        (%set-traces walker window
                     (ecase which (:steps 0) (:unique-steps 1) (:forward-steps 2))
                     thin start cols envelope)
      (labels ((column (vec j)
                 (let ((a (make-array (list n rows) :element-type 'double-float)))
                   (dotimes (c n a)
                     (dotimes (r rows)
                       (setf (aref a c r) (aref vec (+ (* nc (+ (* c rows) r)) j)))))))
               (per-key (vec)
                 (loop for k in names
                       for j from lead
                       append (list k (column vec j)))))
        (append (list :values (per-key v)
                      :prob (and prob (column v 0))
                      :n-out n-out :n-kept n-kept :n-used n-used)
                (and envelope
                     (list :lo (per-key lo) :hi (per-key hi)
                           :prob-lo (and prob (column lo 0))
                           :prob-hi (and prob (column hi 0)))))))))

(defun walker-set-catepillar (walker &key take points)
  "The numbers behind walker-catepillar-plots and walker-liklihood-plot for every walker of the
set.  POINTS nil: every step of the newest TAKE (nil: the whole walks).  POINTS p: buckets of
stride = (ceiling window p) steps, and of each bucket its first value and its extremes, so that no
excursion is lost to the thinning.  A plist of :stride, :n-out (rows of each chain, newest first),
:params (key (:first array [:lo array :hi array]) ...) and :log-liklihoods (:first array ...);
the arrays are [n-chains][rows]."
  (let* ((window (%bin-window walker take "walker-set-catepillar"))
         (stride (if points (max 1 (ceiling window points)) 1))
         (r (walker-set-trace walker :take window :thin stride :envelope (and points t))))
    (flet ((sides (first lo hi)
             (append (list :first first) (and points (list :lo lo :hi hi)))))
      (list :stride stride
            :n-out (getf r :n-out)
            :params (loop for k in (walker-param-keys walker)
                          append (list k (sides (getf (getf r :values) k)
                                                (getf (getf r :lo) k)
                                                (getf (getf r :hi) k))))
            :log-liklihoods (sides (getf r :prob) (getf r :prob-lo) (getf r :prob-hi))))))

;;; ------------------------------------------------------------------ what a window is worth
;;; The reference judges convergence by eye (walker-catepillar-plots M:1294-1310); these are the
;;; numbers one asks of a walker set first, every chain from one device call (mhx_get_autocorr,
;;; whose comment in include/mhx.h has the definitions).
(defun walker-set-autocorr (walker &key keys (take 1000) (max-lag 255))
  "For every chain of the set the plist (key (:tau tau :ess ess :status status) ...) over KEYS
(nil: all): the integrated autocorrelation time of the newest TAKE steps by Geyer's initial
positive sequence over lags up to MAX-LAG, steps / tau, and 0 or a sum of 1 (a value that is not
finite), 2 (the chain did not move: tau is a NaN) and 4 (MAX-LAG too small: tau is a lower bound)."
  (let* ((n (walker-n-chains walker))
         (cols (%key-columns walker keys))
         (names (or keys (walker-param-keys walker)))
         (nc (length cols))
         (window (%bin-window walker take "walker-set-autocorr"))
         (none (cffi:null-pointer)))
    (cffi:with-foreign-objects ((colp :int32 nc) (tau :double (* n nc)) (ess :double (* n nc))
                                (status :int32 (* n nc)))
      (fill-int32s colp cols)
      (%set-call walker #'%mhx-get-autocorr #'%mhx-group-get-autocorr
                 window colp nc max-lag tau ess none none none none none status)
      (loop for c below n
            collect (loop for k in names
                          for j from 0
                          append (list k (list :tau (cffi:mem-aref tau :double (+ (* c nc) j))
                                               :ess (cffi:mem-aref ess :double (+ (* c nc) j))
                                               :status (cffi:mem-aref status :int32 (+ (* c nc) j)))))))))

(defun walker-set-rhat (walker &key keys (take 1000))
  "Split R-hat over the set's chains, the plist (key rhat ...) over KEYS (nil: all): each chain's
newest TAKE steps cut in two halves (mhx_get_autocorr's half moments, mhx_split_rhat).  MHX-ERROR
when the chains' windows differ in length or hold fewer than four steps."
  (let* ((n (walker-n-chains walker))
         (cols (%key-columns walker keys))
         (names (or keys (walker-param-keys walker)))
         (nc (length cols))
         (window (%bin-window walker take "walker-set-rhat"))
         (none (cffi:null-pointer)))
    (cffi:with-foreign-objects ((colp :int32 nc) (hm :double (* n nc 2)) (hv :double (* n nc 2))
                                (used :int32 n) (rhat :double nc))
      (fill-int32s colp cols)
      (%set-call walker #'%mhx-get-autocorr #'%mhx-group-get-autocorr
                 window colp nc 1 none none none hm hv none used none)
      (with-c-call
        (check (%mhx-split-rhat hm hv used n nc rhat)))
      (loop for k in names
            for j from 0
            append (list k (cffi:mem-aref rhat :double j))))))

;;; ------------------------------------------------------------------ the narrowest interval
;;; :95cr and its kin are equal-tailed (nth-percentile M:1495-1506): for a width pressed against its
;;; bound or a skewed derived area they can leave out the most probable value.  The highest-density
;;; interval needs the window in order; the device sorts it (mhx_get_hdi, whose comment in
;;; include/mhx.h has the definition), and the sorted window at evenly spaced ranks comes with it.
(defun %hdi-mass (mass)
  "MASS per cent as the (num . den) mhx_get_hdi takes: a rational as it is, a float to the
thousandth of a per cent"
  (let ((r (if (rationalp mass) mass (/ (round (* 1000 mass)) 1000))))
    (cons (numerator r) (denominator r))))

(defun %hdi-call (walker take keys masses n-ladder who)
  "mhx_get_hdi over KEYS: (values lo hi ladder names n-cols), lo and hi [n][n-mass][n-cols] and
ladder [n][n-cols][n-ladder] as lisp arrays"
  (let* ((n (walker-n-chains walker))
         (cols (%key-columns walker keys))
         (names (or keys (walker-param-keys walker)))
         (nc (length cols))
         (nm (length masses))
         (window (%bin-window walker take who))
         (none (cffi:null-pointer))
         (lo (make-array (* n nm nc) :element-type 'double-float))
         (hi (make-array (* n nm nc) :element-type 'double-float))
         (ladder (make-array (* n nc n-ladder) :element-type 'double-float)))
    (cffi:with-foreign-objects ((colp :int32 nc) (num :int32 (max nm 1)) (den :int32 (max nm 1))
                                (lop :double (max 1 (* n nm nc))) (hip :double (max 1 (* n nm nc)))
                                (ladp :double (max 1 (* n nc n-ladder))))
      (fill-int32s colp cols)
      (fill-int32s num (mapcar #'car masses))
      (fill-int32s den (mapcar #'cdr masses))
      (%set-call walker #'%mhx-get-hdi #'%mhx-group-get-hdi
                 window colp nc num den nm n-ladder lop hip none ladp none none)
      (dotimes (i (* n nm nc))
        (setf (aref lo i) (cffi:mem-aref lop :double i)
              (aref hi i) (cffi:mem-aref hip :double i)))
      (dotimes (i (* n nc n-ladder))
        (setf (aref ladder i) (cffi:mem-aref ladp :double i))))
    (values lo hi ladder names nc)))

(defun walker-set-hdi (walker &key (mass 95) keys (take 1000))
  "For every chain of the set the plist (key (low high) ...) over KEYS (nil: all): the narrowest
interval between two of the chain's newest TAKE steps that holds MASS per cent of them, from one
device call.  Of equally narrow intervals the lowest."
  (multiple-value-bind (lo hi ladder names nc)
      (%hdi-call walker take keys (list (%hdi-mass mass)) 0 "walker-set-hdi")
    (declare (ignore ladder))
    (loop for c below (walker-n-chains walker)
          collect (loop for k in names
                        for j from 0
                        append (list k (list (aref lo (+ (* c nc) j)) (aref hi (+ (* c nc) j))))))))

(defun walker-hdi (walker &key (chain 0) (mass 95) keys (take 1000))
  "One chain's entry of walker-set-hdi.  The device call is the whole set's."
  (elt (walker-set-hdi walker :mass mass :keys keys :take take) chain))

(defun walker-set-quantiles (walker &key (points 101) keys (take 1000))
  "For every chain of the set the plist (key vector ...) over KEYS (nil: all): the chain's newest
TAKE steps in ascending order at POINTS (2 to 4096) evenly spaced ranks - entry i has rank
(floor (* i (1- n)) (1- points)) - for an ECDF, a violin or a Q-Q plot, from one device call."
  (multiple-value-bind (lo hi ladder names nc)
      (%hdi-call walker take keys nil points "walker-set-quantiles")
    (declare (ignore lo hi))
    (loop for c below (walker-n-chains walker)
          collect (loop for k in names
                        for j from 0
                        append (list k (subseq ladder (* (+ (* c nc) j) points)
                                               (* (+ (* c nc) j 1) points)))))))

;;; ------------------------------------------------------------------ one posterior for the set
;;; On a set whose chains sample the same posterior the steps of all chains make ONE sample.  The
;;; reference has no walker-set reduction (walker-set-get answers per chain); this is an exact
;;; selection over the pool on the device (mhx_get_ensemble_percentiles, whose comment in
;;; include/mhx.h has the definitions).
(defun walker-set-ensemble-get (walker &key (get :median-params) (take 1000) keys include)
  "GET of the pool of every chain's newest TAKE steps, the plist (key value ...) over KEYS (nil:
all), from one device call.  GET: :median-params, :95cr (a list low high), :iqr, :stddev-normal
(the 84.1 point minus the median) or (:percentile n).  INCLUDE: a sequence with one generalised
boolean per chain that leaves out the chains marked nil (those that never converged); nil: all."
  (let* ((n (walker-n-chains walker))
         (cols (%key-columns walker keys))
         (names (or keys (walker-param-keys walker)))
         (nc (length cols))
         (selector (if (consp get) (first get) get))
         (points (%exp-percentiles (if (eq get :median-params) :median get)))
         (n-pct (length points))
         (window (%bin-window walker take "walker-set-ensemble-get"))
         (none (cffi:null-pointer)))
    (unless (and points (member selector '(:median-params :95cr :iqr :stddev-normal :percentile)))
      (error "unknown :get ~s" get))
    (when (and include (/= (length include) n))
      (error ":include must hold one entry per chain (~d), not ~d" n (length include)))
    (cffi:with-foreign-objects ((colp :int32 nc) (num :int32 n-pct) (den :int32 n-pct)
                                (mask :uint8 n) (out :double (* n-pct nc)))
      (fill-int32s colp cols)
      (fill-int32s num (mapcar #'car points))
      (fill-int32s den (mapcar #'cdr points))
      (let ((i 0))
        (map nil (lambda (v) (setf (cffi:mem-aref mask :uint8 i) (if v 1 0)) (incf i)) include))
      (%set-call walker #'%mhx-get-ensemble-percentiles #'%mhx-group-get-ensemble-percentiles
                 window colp nc (if include mask none) num den n-pct out none none none)
      (loop for k in names
            for j from 0
            append (list k (flet ((point (q) (cffi:mem-aref out :double (+ (* q nc) j))))
                             (ecase selector
                               ((:median-params :percentile) (point 0))
                               (:95cr (list (point 0) (point 1)))
                               ((:iqr :stddev-normal) (- (point 1) (point 0))))))))))

;;; ------------------------------------------------------------------ which model to have fitted
;;; The reference compares models by eye (walker-plot-residuals).  WAIC (Watanabe; Gelman, Hwang and
;;; Vehtari 2014) from the device ring, every chain in one call per function of a global fit
;;; (mhx_get_waic, whose comment in include/mhx.h has the definition).
(defun walker-set-waic (walker &key (take 1000))
  "For every chain of the set the plist (:elpd :lppd :p-waic :waic :n-high :n-used :status) over its
newest TAKE steps, summed over the functions of a global fit: lppd - p-waic, the log pointwise
predictive density, the effective number of parameters, -2 elpd, the points whose variance term
exceeds 0.4, the window, and 0 or +waic-one-step+.  FLOATING-POINT-INVALID-OPERATION where a model
value or a likelihood term of a window is not finite: the reference would have trapped there."
  (let* ((n (walker-n-chains walker))
         (k-fns (length (walker-function walker)))
         (window (%bin-window walker take "walker-set-waic"))
         (none (cffi:null-pointer))
         (lppd-sum (make-array n :element-type 'double-float :initial-element 0d0))
         (p-sum (make-array n :element-type 'double-float :initial-element 0d0))
         (high (make-array n :element-type 'fixnum :initial-element 0))
         (used (make-array n :element-type 'fixnum :initial-element 0))
         (flags (make-array n :element-type 'fixnum :initial-element 0)))
    (cffi:with-foreign-objects ((lppd :double n) (p :double n) (nh :int32 n) (nu :int32 n)
                                (st :int32 n))
      (dotimes (fn k-fns)
        (%set-call walker #'%mhx-get-waic #'%mhx-group-get-waic
                   fn window none lppd p nh none none none nu st)
        (dotimes (c n)
          (incf (aref lppd-sum c) (cffi:mem-aref lppd :double c))
          (incf (aref p-sum c) (cffi:mem-aref p :double c))
          (incf (aref high c) (cffi:mem-aref nh :int32 c))
          (setf (aref used c) (cffi:mem-aref nu :int32 c))
          ;; (the two status bits, function after function: a bit set once stays set)
          (let ((now (cffi:mem-aref st :int32 c))
                (before (aref flags c)))
            (setf (aref flags c)
                  (+ (if (or (oddp now) (oddp before)) +waic-nonfinite+ 0)
                     (if (or (>= now +waic-one-step+) (>= before +waic-one-step+))
                         +waic-one-step+
                         0)))))))
    (loop for c below n
          do (when (oddp (aref flags c))
               (error 'floating-point-invalid-operation
                      :operation 'walker-set-waic :operands (list :chain c)))
          collect (let ((elpd (- (aref lppd-sum c) (aref p-sum c))))
                    (list :elpd elpd :lppd (aref lppd-sum c) :p-waic (aref p-sum c)
                          :waic (* -2d0 elpd) :n-high (aref high c) :n-used (aref used c)
                          :status (aref flags c))))))

(defun walker-waic (walker &key (chain 0) (take 1000))
  "One chain's entry of walker-set-waic.  The device call is the whole set's: for more than a few
chains call walker-set-waic once and take its elements."
  (elt (walker-set-waic walker :take take) chain))

;;; PSIS-LOO (Vehtari, Gelman and Gabry 2017) where walker-set-waic's :n-high says WAIC cannot tell:
;;; the leave-one-out accuracy and the count of points whose Pareto khat exceeds K-LIMIT, every
;;; chain in one call per function of a global fit (mhx_get_loo, whose comment in include/mhx.h has
;;; the definition).  The totals only: the pointwise elpd and khat are the Python mirror's.
(defun walker-set-loo (walker &key (take 1000) (tail 0) (k-limit 0.7d0))
  "For every chain of the set the plist (:elpd-loo :p-loo :looic :lppd :n-high :n-used :status) over
its newest TAKE steps, summed over the functions of a global fit: the leave-one-out expected log
pointwise predictive density, lppd - elpd-loo, -2 elpd-loo, the log pointwise predictive density,
the points whose Pareto khat exceeds K-LIMIT, the window, and a sum of +loo-short+, +loo-flat+ and
+loo-empty+.  TAIL: the tail length, 0 for the rule.  FLOATING-POINT-INVALID-OPERATION where a
model value or a likelihood term of a window is not finite: the reference would have trapped there."
  (let* ((n (walker-n-chains walker))
         (k-fns (length (walker-function walker)))
         (window (%bin-window walker take "walker-set-loo"))
         (none (cffi:null-pointer))
         (elpd-sum (make-array n :element-type 'double-float :initial-element 0d0))
         (lppd-sum (make-array n :element-type 'double-float :initial-element 0d0))
         (high (make-array n :element-type 'fixnum :initial-element 0))
         (used (make-array n :element-type 'fixnum :initial-element 0))
         (flags (make-array n :element-type 'fixnum :initial-element 0)))
    (cffi:with-foreign-objects ((elpd :double n) (lppd :double n) (nh :int32 n) (nu :int32 n)
                                (st :int32 n))
      (dotimes (fn k-fns)
        (%set-call walker #'%mhx-get-loo #'%mhx-group-get-loo
                   fn window tail (coerce k-limit 'double-float)
                   elpd none lppd nh nu st none none none none none)
        (dotimes (c n)
          (incf (aref elpd-sum c) (cffi:mem-aref elpd :double c))
          (incf (aref lppd-sum c) (cffi:mem-aref lppd :double c))
          (incf (aref high c) (cffi:mem-aref nh :int32 c))
          (setf (aref used c) (cffi:mem-aref nu :int32 c))
          ;; (the four status bits, function after function: a bit set once stays set)
          (let ((now (cffi:mem-aref st :int32 c))
                (before (aref flags c)))
            (setf (aref flags c)
                  (loop for b in (list +loo-nonfinite+ +loo-short+ +loo-flat+ +loo-empty+)
                        sum (if (or (oddp (floor now b)) (oddp (floor before b))) b 0)))))))
    (loop for c below n
          do (when (oddp (aref flags c))
               (error 'floating-point-invalid-operation
                      :operation 'walker-set-loo :operands (list :chain c)))
          collect (let ((elpd-loo (aref elpd-sum c)))
                    (list :elpd-loo elpd-loo :p-loo (- (aref lppd-sum c) elpd-loo)
                          :looic (* -2d0 elpd-loo) :lppd (aref lppd-sum c) :n-high (aref high c)
                          :n-used (aref used c) :status (aref flags c))))))

(defun walker-loo (walker &key (chain 0) (take 1000) (tail 0) (k-limit 0.7d0))
  "One chain's entry of walker-set-loo.  The device call is the whole set's: for more than a few
chains call walker-set-loo once and take its elements."
  (elt (walker-set-loo walker :take take :tail tail :k-limit k-limit) chain))

;;; Data the walk did not see - a repeated measurement, a fold left out of the fit, or each walker's
;;; own spectrum of a set with a dataset per walker, which walker-set-waic refuses - scored under
;;; every walker's window in one call (mhx_get_heldout, whose comment in include/mhx.h has the
;;; definition).  The totals only: the pointwise densities, the fit moments and the K-fold layer
;;; are the Python mirror's.
(defun walker-set-score-data (walker data &key data-error (take 1000) (fn-number 0))
  "For every walker of the set the plist (:lpd :n-scored :n-used :status): the log pointwise
predictive density of DATA = (x y) under its newest TAKE steps by function FN-NUMBER's own
likelihood, the points scored, the window, and 0 or +heldout-no-points+.  y is one sequence of
numbers for every walker, or a sequence of one such sequence per walker.  DATA-ERROR: nil, one
number, or one number per point.  FLOATING-POINT-INVALID-OPERATION where a model value or a
likelihood term of a window is not finite: the reference would have trapped there."
  (let* ((n (walker-n-chains walker))
         (x (coerce (first data) 'list))
         (y (second data))
         (m (length x))
         (per-chain (not (realp (elt y 0))))
         (rows (if per-chain (coerce y 'list) (list y)))
         (window (%bin-window walker take "walker-set-score-data"))
         (none (cffi:null-pointer))
         (sigma (cond ((null data-error) nil)
                      ((realp data-error) (make-list m :initial-element data-error))
                      (t (coerce data-error 'list))))
         (yp (cffi:foreign-alloc :double :count (* (length rows) m)))
         (sp (if sigma (cffi:foreign-alloc :double :count m) none)))
    (unless (and (if per-chain (= (length rows) n) t)
                 (every (lambda (row) (= (length row) m)) rows)
                 (or (null sigma) (= (length sigma) m)))
      (cffi:foreign-free yp)
      (when sigma (cffi:foreign-free sp))
      (error "walker-set-score-data: y must be ~d numbers, or ~d rows of them, and :data-error nil, ~
              a number or ~d numbers" m n m))
    (unwind-protect
         (cffi:with-foreign-objects ((xp :double m) (lpd :double n) (ns :int32 n) (nu :int32 n)
                                     (st :int32 n))
           (fill-doubles xp x)
           (fill-doubles yp (loop for row in rows append (coerce row 'list)))
           (when sigma (fill-doubles sp sigma))
           (%set-call walker #'%mhx-get-heldout #'%mhx-group-get-heldout
                      fn-number window xp 1 m yp (if per-chain 1 0) sp (if sigma 1 0) none 0
                      lpd ns none none nu st)
           (loop for c below n
                 do (when (oddp (cffi:mem-aref st :int32 c))
                      (error 'floating-point-invalid-operation
                             :operation 'walker-set-score-data :operands (list :chain c)))
                 collect (list :lpd (cffi:mem-aref lpd :double c)
                               :n-scored (cffi:mem-aref ns :int32 c)
                               :n-used (cffi:mem-aref nu :int32 c)
                               :status (cffi:mem-aref st :int32 c))))
      (cffi:foreign-free yp)
      (when sigma (cffi:foreign-free sp)))))

;;; ------------------------------------------------------------------ data and fit M:1208-1283
;;; The numbers behind the reference's plots.  The :function lives on the device, so the fit
;;; curve is mhx_eval_function and the envelope of the model over the most probable two thirds of
;;; the walk is mhx_get_fit_bands: no history crosses to the host.  :chain selects a member of a
;;; batched walker.
(defun %even-grid (low high count)
  "COUNT doubles from LOW to HIGH inclusive: exact rationals, made doubles at the end"
  (let ((step (/ (cl:rational (- high low)) (1- count)))
        (origin (cl:rational low)))
    (loop for i below count
          collect (coerce (+ origin (* i step)) 'double-float))))

(defun %parameter-vector (walker plist)
  (loop for k in (walker-param-keys walker) collect (getf plist k)))

(defun %model-values (walker fn-number plist xs)
  "function FN-NUMBER at the parameters PLIST: at the list XS, or at its own dataset's x (XS nil)"
  (let* ((d (walker-n-params walker))
         (m (if xs
                (length xs)
                (length (first (elt (walker-data walker) fn-number))))))
    (cffi:with-foreign-objects ((th :double d) (xp :double m) (out :double m))
      (fill-doubles th (%parameter-vector walker plist))
      (when xs (fill-doubles xp xs))
      (with-c-call
        (check (%mhx-eval-function (first (all-engines walker)) fn-number th 1
                                   (if xs xp (cffi:null-pointer)) 1 m out)))
      (coerce (read-doubles out m) 'list))))

(defun %clamped-take (walker take chain)
  (let ((len (walker-length walker chain)))
    (if (or (null take) (> take len)) len take)))

(defun %solution (walker which-solution take chain)
  (case which-solution
    (:most-likely (walker-step-params
                   (walker-get walker :get :most-likely-step :take take :chain chain)))
    (t (walker-get walker :get :median-params :take take :chain chain))))

(defun %shifted (values shift)
  (if shift (mapcar (lambda (v) (+ shift v)) values) values))

(defun walker-get-data-and-fit-no-stddev (walker &key (take 1000) (x-column 0) (y-column 1)
                                                   (fn-number 0)
                                                   (which-solution (or :most-likely :median))
                                                   x-shift y-shift (chain 0))
  "-> (x-fit y-fit x-data y-data params): the fit on 1000 points between the data's least and
greatest x at the chosen solution"
  (let* ((take (%clamped-take walker take chain))
         (data (%dataset-of walker fn-number chain))
         (x-data (elt data x-column))
         (y-data (elt data y-column))
         (x-fit (%even-grid (reduce #'min x-data) (reduce #'max x-data) 1000))
         (params (%solution walker which-solution take chain))
         (y-fit (%model-values walker fn-number params x-fit)))
    (list (%shifted x-fit x-shift) (%shifted y-fit y-shift)
          (%shifted x-data x-shift) (%shifted y-data y-shift) params)))

(defun walker-get-data-and-fit (walker &key (take 1000) (x-column 0) (y-column 1) (fn-number 0)
                                         (which-solution (or :most-likely :median))
                                         x-shift y-shift (chain 0))
  "-> (x-fit max-ys min-ys y-fit x-data y-data params): as above, with the greatest and smallest
model value at every x-fit over the (ceiling (* 0.66 take)) most probable steps of the walk"
  (destructuring-bind (x-fit-shifted y-fit-shifted x-data-shifted y-data-shifted params)
      (walker-get-data-and-fit-no-stddev walker :take take :x-column x-column :y-column y-column
                                                :fn-number fn-number
                                                :which-solution which-solution
                                                :x-shift x-shift :y-shift y-shift :chain chain)
    (let* ((n (walker-n-chains walker))
           (m 1000)
           (x-data (elt (elt (walker-data walker) fn-number) x-column))
           (x-fit (%even-grid (reduce #'min x-data) (reduce #'max x-data) m))
           (ring (cffi:with-foreign-object (cap :int32)
                   (with-c-call
                     (check (%mhx-get-history-capacity (first (all-engines walker)) cap)))
                   (cffi:mem-ref cap :int32)))
           (take (%clamped-take walker take chain))
           (ymax (cffi:foreign-alloc :double :count (* n m)))
           (ymin (cffi:foreign-alloc :double :count (* n m))))
      (when (> (walker-length walker chain) ring)
        (warn "walker-get-data-and-fit :take ~d: the device history ring holds the newest ~d steps of a walk; create the walker with :history-capacity >= the walk's length to keep them all"
              take ring))
      (unwind-protect
           (cffi:with-foreign-objects ((xp :double m) (st :int32 n))
             (fill-doubles xp x-fit)
             (%set-call walker #'%mhx-get-fit-bands #'%mhx-group-get-fit-bands
                        fn-number (max 1 (min take ring)) xp 1 m ymax ymin (cffi:null-pointer) st)
             (unless (zerop (cffi:mem-aref st :int32 chain))
               (error 'floating-point-invalid-operation
                      :operation 'walker-get-data-and-fit :operands (list :chain chain)))
             (flet ((row (ptr)
                      (loop for i below m
                            collect (+ (if y-shift y-shift 0)
                                       (cffi:mem-aref ptr :double (+ (* chain m) i))))))
               (list x-fit-shifted (row ymax) (row ymin) y-fit-shifted x-data-shifted
                     y-data-shifted params)))
        (cffi:foreign-free ymax)
        (cffi:foreign-free ymin)))))

;;; ------------------------------------------------------------------ credible bands of the fit
;;; walker-get-data-and-fit's max-ys / min-ys are the reference's envelope, whose width depends on
;;; :take.  The pointwise posterior of the curve - percentiles, mean and standard deviation of the
;;; model at each x over the window - is mhx_get_fit_percentiles (include/mhx.h has the
;;; definition): every walker of a set in one device call, no history moved.
(defun %credible-points (band who)
  "the (num . den) per cent points (low median high) of BAND: :95cr, :iqr or (:percentile low high)"
  (flet ((ratio (n) (cons (round (* 1000 n)) 1000)))
    (cond ((and (consp band) (eq (first band) :percentile) (= 3 (length band))
                (<= 0 (second band) (third band) 100))
           (list (ratio (second band)) '(50 . 1) (ratio (third band))))
          ((eq band :95cr) '((5 . 2) (50 . 1) (195 . 2)))
          ((eq band :iqr) '((25 . 1) (50 . 1) (75 . 1)))
          (t (error 'mhx-error :code -1
                               :message (format nil "~a: a band is :95cr, :iqr or (:percentile low high), not ~s"
                                                who band))))))

(defun %fit-credible (walker take points band x-column fn-number chains who)
  "the entries (x-fit hi lo median mean stddev) of the walkers CHAINS from one device call"
  (let* ((n (walker-n-chains walker))
         (m points)
         (x-data (elt (elt (walker-data walker) fn-number) x-column))
         (x-fit (%even-grid (reduce #'min x-data) (reduce #'max x-data) m))
         (window (%bin-window walker take who))
         (per-cent (%credible-points band who))
         (pct (cffi:foreign-alloc :double :count (* n 3 m)))
         (mean (cffi:foreign-alloc :double :count (* n m)))
         (sd (cffi:foreign-alloc :double :count (* n m))))
    (unwind-protect
         (cffi:with-foreign-objects ((xp :double m) (num :int32 3) (den :int32 3) (st :int32 n))
           (fill-doubles xp x-fit)
           (fill-int32s num (mapcar #'car per-cent))
           (fill-int32s den (mapcar #'cdr per-cent))
           (%set-call walker #'%mhx-get-fit-percentiles #'%mhx-group-get-fit-percentiles
                      fn-number window xp 1 m num den 3 pct mean sd (cffi:null-pointer) st)
           (loop for c in chains
                 do (when (oddp (cffi:mem-aref st :int32 c))
                      (error 'floating-point-invalid-operation
                             :operation who :operands (list :chain c)))
                 collect (flet ((row (ptr offset)
                                  (loop for i below m
                                        collect (cffi:mem-aref ptr :double (+ offset i)))))
                           (list x-fit
                                 (row pct (* (+ (* c 3) 2) m))
                                 (row pct (* (* c 3) m))
                                 (row pct (* (+ (* c 3) 1) m))
                                 (row mean (* c m))
                                 (row sd (* c m))))))
      (cffi:foreign-free pct)
      (cffi:foreign-free mean)
      (cffi:foreign-free sd))))

(defun walker-get-fit-credible (walker &key (take 1000) (points 1000) (band :95cr) (x-column 0)
                                         (fn-number 0) (chain 0))
  "-> (x-fit hi lo median mean stddev): at POINTS points between the data's least and greatest x
the BAND - :95cr, :iqr or (:percentile low high) - the median, the mean and the standard deviation
of function FN-NUMBER over the walk's newest TAKE steps, computed on the device.
FLOATING-POINT-INVALID-OPERATION where a model value of the window is not finite.  The device call
is the whole set's: for more than a few walkers call walker-set-get-fit-credible once."
  (first (%fit-credible walker take points band x-column fn-number (list chain)
                        'walker-get-fit-credible)))

(defun walker-set-get-fit-credible (walker &key (take 1000) (points 1000) (band :95cr) (x-column 0)
                                             (fn-number 0))
  "walker-get-fit-credible for every walker of the set, from ONE device call: a list with one entry
per chain"
  (%fit-credible walker take points band x-column fn-number
                 (loop for c below (walker-n-chains walker) collect c)
                 'walker-set-get-fit-credible))

(defun walker-get-residuals (walker &key (take 1000) (x-column 0) (y-column 1) (fn-number 0)
                                      (chain 0))
  "-> (x-data residuals stddev): the model at the median parameters minus the data, at the
data's own x - what walker-plot-residuals draws"
  (let* ((take (%clamped-take walker take chain))
         (data (%dataset-of walker fn-number chain))
         (x-data (elt data x-column))
         (y-data (elt data y-column))
         (stddev (%stddev-of walker fn-number chain))
         (stddev (if (= 1 (length stddev))
                     (make-list (length x-data) :initial-element (elt stddev 0))
                     stddev))
         (params (walker-get walker :get :median-params :take take :chain chain))
         (y-fit (%model-values walker fn-number params nil)))
    (list x-data (mapcar #'- y-fit y-data) stddev)))

;;; ------------------------------------------------------------------ which walkers fit badly
;;; walker-get-residuals for every walker of a set, and the goodness-of-fit statistics of the
;;; standardized residuals, from ONE device call (mhx_get_residuals, whose comment in
;;; include/mhx.h has the definition) at the medians - one mhx_get_percentiles call - or at the
;;; most-likely parameters, which the device holds.
(defun runs-z (n-pos n-neg runs)
  "Wald and Wolfowitz's score of RUNS runs of equal sign among N-POS positive and N-NEG other
residuals; nil where it is undefined"
  (let ((total (+ n-pos n-neg)))
    (when (>= total 2)
      (let* ((mu (+ 1 (/ (* 2 n-pos n-neg) total)))
             (var (/ (* (- mu 1) (- mu 2)) (- total 1))))
        (when (plusp var)
          (/ (- runs mu) (sqrt (coerce var 'double-float))))))))

(defun %with-residuals (walker take fn-number which-solution z-limit pointwise consumer)
  "CONSUMER on the foreign arrays (fit chi2 sum-z dw max-z max-index n-pos n-runs n-out status) of one
mhx_get_residuals call for the set; fit is null unless POINTWISE"
  (let* ((n (walker-n-chains walker))
         (d (length (walker-param-keys walker)))
         (m (length (first (elt (walker-data walker) fn-number))))
         (none (cffi:null-pointer))
         (fit (if pointwise (cffi:foreign-alloc :double :count (* n m)) none)))
    (unwind-protect
         (cffi:with-foreign-objects ((th :double (* n d)) (chi2 :double n) (sum-z :double n)
                                     (dw :double n) (max-z :double n) (max-index :int64 n)
                                     (n-pos :int32 n) (n-runs :int32 n) (n-out :int32 n)
                                     (status :int32 n))
           (unless (eq which-solution :most-likely)
             (fill-doubles th (loop for plist in (walker-set-get walker :get :median-params
                                                                        :take take)
                                    append (%parameter-vector walker plist))))
           (%set-call walker #'%mhx-get-residuals #'%mhx-group-get-residuals
                      fn-number (if (eq which-solution :most-likely) none th)
                      (coerce z-limit 'double-float) fit none chi2 sum-z dw max-z max-index
                      n-pos n-runs n-out status)
           (funcall consumer fit chi2 sum-z dw max-z max-index n-pos n-runs n-out status))
      (when pointwise (cffi:foreign-free fit)))))

(defun walker-set-get-residuals (walker &key (take 1000) (fn-number 0) (which-solution :median))
  "walker-get-residuals for every walker of the set: a list with, walker by walker, (x-data
residuals stddev) of the walker's own data, from one device call.  WHICH-SOLUTION: :median or
:most-likely (the walker's most-likely parameters)."
  (let ((n (walker-n-chains walker))
        (m (length (first (elt (walker-data walker) fn-number)))))
    (%with-residuals
     walker take fn-number which-solution 3d0 t
     (lambda (fit chi2 sum-z dw max-z max-index n-pos n-runs n-out status)
       (declare (ignore chi2 sum-z dw max-z max-index n-pos n-runs n-out status))
       (loop for c below n
             collect (let* ((data (%dataset-of walker fn-number c))
                            (x-data (elt data 0))
                            (y-data (elt data 1))
                            (stddev (%stddev-of walker fn-number c))
                            (stddev (if (= 1 (length stddev))
                                        (make-list (length x-data) :initial-element (elt stddev 0))
                                        stddev))
                            (y-fit (loop for i below m
                                         collect (cffi:mem-aref fit :double (+ (* c m) i)))))
                       (list x-data (mapcar #'- y-fit y-data) stddev)))))))

(defun walker-set-goodness-of-fit (walker &key (take 1000) (fn-number 0) (which-solution :median)
                                            (z-limit 3d0))
  "For every walker of the set the plist (:chi2 :dof :reduced-chi2 :mean-z :durbin-watson :runs
:n-pos :runs-z :max-z :max-z-index :n-out :status) of its standardized residuals (fit minus data over
the point's error) at the medians over TAKE, or at the most-likely parameters: the sum of their
squares, the points minus the distinct parameters the function reads, their quotient, the mean
residual, sum (z_i - z_{i-1})^2 / chi2, the runs of equal sign, the positive residuals, runs-z of
them, the greatest |z| and its point, the points with |z| > Z-LIMIT, and 0 or +resid-nonfinite+
(the sums of such a walker mean nothing).  One device call; no fit values cross to the host."
  (let* ((n (walker-n-chains walker))
         (m (length (first (elt (walker-data walker) fn-number))))
         (fn (elt (force-list (walker-function walker)) fn-number))
         (dof (- m (length (remove-duplicates (model-keys fn))))))
    (%with-residuals
     walker take fn-number which-solution z-limit nil
     (lambda (fit chi2 sum-z dw max-z max-index n-pos n-runs n-out status)
       (declare (ignore fit))
       (loop for c below n
             collect (let ((chi (cffi:mem-aref chi2 :double c))
                           (pos (cffi:mem-aref n-pos :int32 c))
                           (runs (cffi:mem-aref n-runs :int32 c))
                           (flag (cffi:mem-aref status :int32 c)))
                       (list :chi2 chi :dof dof
                             :reduced-chi2 (if (and (zerop flag) (plusp dof)) (/ chi dof) nil)
                             :mean-z (if (zerop flag) (/ (cffi:mem-aref sum-z :double c) m) nil)
                             :durbin-watson (if (and (zerop flag) (plusp chi))
                                                (/ (cffi:mem-aref dw :double c) chi)
                                                nil)
                             :runs runs :n-pos pos :runs-z (runs-z pos (- m pos) runs)
                             :max-z (cffi:mem-aref max-z :double c)
                             :max-z-index (cffi:mem-aref max-index :int64 c)
                             :n-out (cffi:mem-aref n-out :int32 c)
                             :status flag)))))))

(defun walker-goodness-of-fit (walker &key (chain 0) (take 1000) (fn-number 0)
                                        (which-solution :median) (z-limit 3d0))
  "One walker's entry of walker-set-goodness-of-fit.  FLOATING-POINT-INVALID-OPERATION where a model
value or a residual of that walker is not finite.  The device call is the whole set's: for more
than a few walkers call walker-set-goodness-of-fit once and take its elements."
  (let ((entry (elt (walker-set-goodness-of-fit walker :take take :fn-number fn-number
                                                       :which-solution which-solution
                                                       :z-limit z-limit)
                    chain)))
    (unless (zerop (getf entry :status))
      (error 'floating-point-invalid-operation
             :operation 'walker-goodness-of-fit :operands (list :chain chain)))
    entry))

;;; ------------------------------------------------------------------ before the walk: Laplace
;;; The normal equations of every walker's least-squares problem from ONE device call per function
;;; (mhx_get_normal_equations, whose comment in include/mhx.h has the definition): the sums F =
;;; g^T g, b = g^T u and chi2 = u^T u, added over the functions of a global fit in ascending order.
;;; The shim returns the device's sums; the inverse of F, the proposal factor and the
;;; Levenberg-Marquardt polish are host linear algebra and stay in the Python mirror
;;; (walker_set_laplace, least_squares), as waic_compare does.
(defun normeq-steps (values)
  "the default half-widths of the central differences: cbrt(2^-52) |v|, with 1 in place of |v|
where v is 0"
  (mapcar (lambda (v)
            (let ((a (abs (coerce v 'double-float))))
              (* 6.0554544523933395d-6 (if (zerop a) 1d0 a))))
          values))

(defun walker-set-laplace (walker &key (which-solution :most-likely) (take 1000) steps fixed)
  "For every walker of the set the plist (:params :chi2 :dof :reduced-chi2 :gradient :fisher-matrix
:status) of its least-squares problem at its most-likely parameters (WHICH-SOLUTION :median: at
the medians over TAKE): the sum of the squared weighted residuals, the points minus the varied
keys, their quotient, the plist key -> b = g^T u, F = g^T g as a list of rows in the order of the
walker's keys, and 0 or +normeq-nonfinite+ (the sums of such a walker mean nothing).  STEPS: a plist
key -> half-width of the central difference (default: normeq-steps of the parameters); the keys in
FIXED are held: their rows and columns are zero.  The covariance is the inverse of F over the
varied keys."
  (let* ((n (walker-n-chains walker))
         (keys (walker-param-keys walker))
         (d (length keys))
         (k-fns (length (force-list (walker-function walker))))
         (points (loop for fn below k-fns
                       sum (length (first (elt (walker-data walker) fn)))))
         (dof (- points (- d (length fixed))))
         (plists (if (eq which-solution :most-likely)
                     (loop for c below n
                           collect (walker-step-params (walker-most-likely-step walker c)))
                     (walker-set-get walker :get :median-params :take take)))
         (f-sum (make-array (* n d d) :element-type 'double-float :initial-element 0d0))
         (b-sum (make-array (* n d) :element-type 'double-float :initial-element 0d0))
         (chi-sum (make-array n :element-type 'double-float :initial-element 0d0))
         (flags (make-array n :element-type 'fixnum :initial-element 0))
         (none (cffi:null-pointer)))
    (cffi:with-foreign-objects ((th :double (* n d)) (hs :double (* n d)) (jtj :double (* n d d))
                                (jtr :double (* n d)) (chi2 :double n) (status :int32 n))
      (fill-doubles th (loop for plist in plists append (%parameter-vector walker plist)))
      (fill-doubles hs (loop for plist in plists
                             append (loop for k in keys
                                          for h in (normeq-steps (%parameter-vector walker plist))
                                          collect (cond ((member k fixed) 0d0)
                                                        ((getf steps k)
                                                         (coerce (getf steps k) 'double-float))
                                                        (t h)))))
      (dotimes (fn k-fns)
        (%set-call walker #'%mhx-get-normal-equations #'%mhx-group-get-normal-equations
                   fn th hs 1 jtj jtr chi2 none status)
        (dotimes (i (* n d d))
          (incf (aref f-sum i) (cffi:mem-aref jtj :double i)))
        (dotimes (i (* n d))
          (incf (aref b-sum i) (cffi:mem-aref jtr :double i)))
        (dotimes (c n)
          (incf (aref chi-sum c) (cffi:mem-aref chi2 :double c))
          (unless (zerop (cffi:mem-aref status :int32 c))
            (setf (aref flags c) +normeq-nonfinite+)))))
    (loop for c below n
          for plist in plists
          collect (let ((chi (aref chi-sum c))
                        (flag (aref flags c)))
                    (list :params plist :chi2 chi :dof dof
                          :reduced-chi2 (if (and (zerop flag) (plusp dof)) (/ chi dof) nil)
                          :gradient (loop for k in keys
                                          for j from 0
                                          append (list k (aref b-sum (+ (* c d) j))))
                          :fisher-matrix (loop for i below d
                                               collect (loop for j below d
                                                             collect (aref f-sum (+ (* c d d) (* i d) j))))
                          :status flag)))))

(defun walker-laplace (walker &key (chain 0) (which-solution :most-likely) (take 1000) steps fixed)
  "One walker's entry of walker-set-laplace.  FLOATING-POINT-INVALID-OPERATION where a value of
that walker is not finite.  The device call is the whole set's: for more than a few walkers call
walker-set-laplace once and take its elements."
  (let ((entry (elt (walker-set-laplace walker :which-solution which-solution :take take
                                               :steps steps :fixed fixed)
                    chain)))
    (unless (zerop (getf entry :status))
      (error 'floating-point-invalid-operation
             :operation 'walker-laplace :operands (list :chain chain)))
    entry))

;;; ------------------------------------------------------------------ before the polish: search
;;; The brute-force stage of a least-squares toolkit for a walker set: every walker tries the same
;;; candidate vectors against its own data in ONE device call (mhx_get_candidate_scores, whose
;;; comment in include/mhx.h has the definition) and the device ranks them.  Ranking the kept ones
;;; again under the prior, candidates per walker and the chi-square maps stay in the Python mirror
;;; (walker_set_search, walker_set_chi2_map).
(defun candidate-grid (params axes)
  "The starts of a search: the plist PARAMS with the keys of the plist AXES (key -> list of values)
replaced by the Cartesian product of the axes' values.  Two values: the list of plists in row-major
order, the first axis slowest, and the list of the axes' lengths."
  (let ((rows (list (copy-list params))))
    (loop for (key vals) on axes by #'cddr
          do (setf rows (loop for row in rows
                              append (loop for v in vals
                                           collect (let ((new (copy-list row)))
                                                     (setf (getf new key) v)
                                                     new)))))
    (values rows (loop for (key vals) on axes by #'cddr
                       collect (progn key (length vals))))))

(defun walker-set-search (walker candidates &key (keep 4))
  "For every walker of the set the plist (:params :index :chi2 :kept :n-bad) of a search over
CANDIDATES, a list of parameter plists every walker tries against its own data, summed over the
functions of a global fit: the candidate of least chi-square (among equals the first), its place in
CANDIDATES and its chi-square; :kept the KEEP best as (index chi2) lists in ascending (chi2, index)
order, at most +cand-keep-max+; :n-bad the candidates with a value or residual that is not finite
(they rank last).  A walker without a finite candidate gets :index -1 and :params nil.  One device
call."
  (let* ((n (walker-n-chains walker))
         (d (length (walker-param-keys walker)))
         (m (length candidates))
         (none (cffi:null-pointer))
         (cand (cffi:foreign-alloc :double :count (max 1 (* m d)))))
    (unwind-protect
         (cffi:with-foreign-objects ((best-index :int32 (* n keep)) (best-score :double (* n keep))
                                     (n-bad :int32 n))
           (fill-doubles cand (loop for plist in candidates
                                    append (%parameter-vector walker plist)))
           (%set-call walker #'%mhx-get-candidate-scores #'%mhx-group-get-candidate-scores
                      -1 cand m 0 keep none best-index best-score n-bad)
           (loop for c below n
                 collect (let* ((kept (loop for r below keep
                                            for j = (cffi:mem-aref best-index :int32 (+ (* c keep) r))
                                            when (>= j 0)
                                              collect (list j (cffi:mem-aref best-score :double
                                                                             (+ (* c keep) r)))))
                                (best (first kept))
                                (found (and best (<= (second best) most-positive-double-float))))
                           (list :params (if found (copy-list (elt candidates (first best))) nil)
                                 :index (if found (first best) -1)
                                 :chi2 (if best (second best) nil)
                                 :kept kept
                                 :n-bad (cffi:mem-aref n-bad :int32 c)))))
      (cffi:foreign-free cand))))

;;; ------------------------------------------------------------------ save / load M:971-1001
;;; The plist the reference's (commented) walker-construct-print-list builds, written and read
;;; under with-standard-io-syntax; functions are only NAMED in the file, so walker-load wants
;;; the :function / :log-liklihood / :log-prior designators again, exactly as there.
;;; ------------------------------------------------------------ derived quantities M:1052-1064
;;; walker-with-exp is host work in a Lisp host: the most-likely parameters go into the form and
;;; the form is evaluated, whatever it is.  Its posterior - the form at every step of the window,
;;; then percentiles, mean and standard deviation - is mhx_get_derived: the form crosses as a
;;; device expression (form->c) and no history crosses back.
(defun %with-parameters (form plist)
  "FORM with every keyword replaced by its value in PLIST"
  (cond ((keywordp form) (getf plist form))
        ((consp form) (cons (%with-parameters (car form) plist)
                            (%with-parameters (cdr form) plist)))
        (t form)))

(defun walker-with-exp (walker exp &key (take 1000))
  "EXP, a form whose keywords name parameters of WALKER - (* :a1 :w1 (sqrt pi)) - evaluated with
the walker's most-likely parameters in their place"
  (eval (%with-parameters exp (walker-get walker :get :most-likely-params :take take))))

(defun %keywords-of (form)
  "the keywords of FORM, each once, in the order they first appear"
  (let ((seen nil))
    (labels ((walk (f)
               (cond ((keywordp f) (pushnew f seen))
                     ((consp f) (walk (car f)) (walk (cdr f))))))
      (walk form))
    (nreverse seen)))

(defun %exp-percentiles (get)
  "the (num . den) per cent points mhx_get_derived is asked for to answer GET"
  (cond ((consp get)
         ;; n to the thousandth of a per cent, as an exact ratio (84.1 -> 84100 / 1000)
         (list (cons (round (* 1000 (second get))) 1000)))
        (t (case get
             (:median '((50 . 1)))
             (:95cr '((5 . 2) (195 . 2)))
             (:iqr '((25 . 1) (75 . 1)))
             (:stddev-normal '((50 . 1) (841 . 10)))
             (t nil)))))

(defun walker-set-exp-get (walker exp &key (get :median) (take 1000))
  "For every chain of WALKER, GET of the values EXP takes over the chain's newest TAKE steps: one
device call (mhx_get_derived), a list with one entry per chain.  GET: :most-likely (EXP at the
most-likely step), :median, :95cr (a list low high), :iqr, :mean, :stddev (a NaN for a one-step
window), :stddev-normal (the 84.1 point minus the median), :values (newest first) or
(:percentile n).  Besides keywords EXP may name PROB, the step's log-posterior."
  (let* ((n (walker-n-chains walker))
         (keys (walker-param-keys walker))
         (used (%keywords-of exp))
         (index (loop for k in used
                      collect (or (position k keys)
                                  (error 'mhx-error :code -1
                                                    :message (format nil "~s is no parameter of the walker" k)))))
         (names (mapcar #'mangle-symbol used))
         (text (form->c exp))
         (points (%exp-percentiles get))
         (n-pct (length points))
         (selector (if (consp get) (first get) get))
         (ring (cffi:with-foreign-object (cap :int32)
                 (with-c-call
                   (check (%mhx-get-history-capacity (first (all-engines walker)) cap)))
                 (cffi:mem-ref cap :int32)))
         (window (max 1 (min take ring)))
         (none (cffi:null-pointer))
         (vals (if (eq selector :values)
                   (cffi:foreign-alloc :double :count (* n window))
                   none)))
    (unless (member selector '(:most-likely :median :95cr :iqr :mean :stddev :stddev-normal
                               :values :percentile))
      (error 'mhx-error :code -1 :message (format nil "unknown :get ~s" get)))
    (unwind-protect
         (with-c-strings (exprs (list text))
           (with-c-strings (name-ptrs names)
             (cffi:with-foreign-objects ((idx :int32 (max 1 (length index)))
                                         (num :int32 (max 1 n-pct)) (den :int32 (max 1 n-pct))
                                         (best :double n) (pct :double (* n (max 1 n-pct)))
                                         (mean :double n) (sd :double n) (held :int32 n))
               (fill-int32s idx index)
               (fill-int32s num (mapcar #'car points))
               (fill-int32s den (mapcar #'cdr points))
               (%set-call walker #'%mhx-get-derived #'%mhx-group-get-derived
                          exprs 1 name-ptrs idx (length index) window num den n-pct
                          best pct mean sd vals held none)
               (flet ((point (c q) (cffi:mem-aref pct :double (+ (* c n-pct) q))))
                 (loop for c below n
                       collect (ecase selector
                                 (:most-likely (cffi:mem-aref best :double c))
                                 ((:median :percentile) (point c 0))
                                 (:95cr (list (point c 0) (point c 1)))
                                 ((:iqr :stddev-normal) (- (point c 1) (point c 0)))
                                 (:mean (cffi:mem-aref mean :double c))
                                 (:stddev (cffi:mem-aref sd :double c))
                                 (:values
                                  (loop for s below (cffi:mem-aref held :int32 c)
                                        collect (cffi:mem-aref vals :double (+ (* c window) s))))))))))
      (unless (cffi:null-pointer-p vals)
        (cffi:foreign-free vals)))))

(defun walker-exp-get (walker exp &key (get :median) (take 1000) (chain 0))
  "walker-set-exp-get's answer for one chain of WALKER"
  (elt (walker-set-exp-get walker exp :get get :take take) chain))

(defun %designator-name (x)
  (cond ((null x) nil)
        ((symbolp x) x)
        ((model-p x) (or (model-expr x) (list :model (model-id x) (model-shape x))))
        ((likelihood-spec-p x) (likelihood-spec-expr x))
        ((prior-bounds-spec-p x) (list :prior-bounds (prior-bounds-spec-bounds x)))
        (t (princ-to-string x))))

(defun walker-save (walker filename &optional take (chain 0))
  "(walker-save walker filename &optional take): the newest TAKE steps (all of them by default)
of chain CHAIN with the data they were walked on."
  (when (walker-planes walker)
    (error 'mhx-error :code -5
                      :message "walker-save of a walker set with a dataset per walker (walker-set-create): the file holds one dataset per function"))
  (let ((form (list :fn (mapcar #'%designator-name (walker-function walker))
                    :data (walker-data walker)
                    :param-keys (walker-param-keys walker)
                    :stddev (walker-data-error walker)
                    :log-liklihood (mapcar #'%designator-name (walker-log-liklihood walker))
                    :log-prior (mapcar #'%designator-name (walker-log-prior walker))
                    :walker (mapcar (lambda (s)
                                      (list :prob (walker-step-prob s)
                                            :params (walker-step-params s)))
                                    (walker-get walker :get :steps :take take :chain chain)))))
    (with-open-file (out filename :direction :output :if-exists :supersede)
      (with-standard-io-syntax
        (let ((*package* (find-package :keyword)))
          (write form :stream out)
          (terpri out))))
    nil))

(defun walker-load (filename &key function log-liklihood log-prior quiet (device 0) (seed 0))
  "(walker-load filename &key function log-liklihood log-prior quiet): without the designators,
print what the file recommends and return nil; with :function (and optionally the others),
rebuild the walker on the GPU and restore the saved walk (mhx_set_history)."
  (let* ((full (with-open-file (in filename :direction :input)
                 (with-standard-io-syntax
                   (let ((*package* (find-package :keyword)) (*read-eval* nil))
                     (read in)))))
         (data (getf full :data))
         (stddev (getf full :stddev))
         (keys (getf full :param-keys))
         (walks (getf full :walker)))
    (unless quiet
      (format t "*Recommendations*~%function: ~s~%log-liklihood: ~s~%log-prior: ~s~%"
              (getf full :fn) (getf full :log-liklihood) (getf full :log-prior)))
    (when function
      (let* ((newest (first walks))
             (walker (walker-create :function function :data data
                                    :params (getf newest :params) :data-error stddev
                                    :log-liklihood log-liklihood :log-prior log-prior
                                    :device device :seed seed))
             (n (length walks))
             (d (length keys)))
        (cffi:with-foreign-objects ((pr :double n) (th :double (* n d)))
          (loop for w in walks
                for s from 0
                do (setf (cffi:mem-aref pr :double s) (coerce (getf w :prob) 'double-float))
                   (loop for k in keys
                         for j from 0
                         do (setf (cffi:mem-aref th :double (+ (* s d) j))
                                  (coerce (getf (getf w :params) k) 'double-float))))
          (with-c-call (check (%mhx-set-history (engine-of walker) 0 pr th n))))
        walker))))
