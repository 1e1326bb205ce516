;;;; mi355x-simplex.lisp -- CFFI glue: linear-programming:*solver*  ->  libmi355x_simplex.so
;;;;
;;;; Usage (nothing in the reference library changes):
;;;;
;;;;   (asdf:load-system "mi355x-simplex")
;;;;   (let ((linear-programming:*solver* 'mi355x-simplex:mi355x-simplex-solver))
;;;;     (linear-programming:solve-problem problem))          ; src/solver.lisp:53-56
;;;;
;;;; or (setf linear-programming:*solver* 'mi355x-simplex:mi355x-simplex-solver), after which
;;;; solve-problem / with-solved-problem / with-solution-variables work unchanged.
;;;;
;;;; Two routes from a `problem` to a solution object:
;;;;  * NATIVE (the default for problems whose numbers are double-floats / integers): the parsed
;;;;    problem (src/problem.lisp:45-53) is marshalled straight into the library (mi355x_problem_*),
;;;;    which assembles the tableau in C++ (= build-tableau, src/simplex.lisp:142-328, in double-float;
;;;;    single-phase problems never exist as a dense tableau on either side), solves it on the GPU and
;;;;    keeps a light solution (objective row, RHS column, basis, var-mapping: all that
;;;;    src/simplex.lisp:74-120 read).  The Lisp side holds a MI355X-SOLUTION with methods on the
;;;;    four solution-* generics (src/solver.lisp:59-80).  No boxed R x C matrix, no per-element
;;;;    coerce.
;;;;  * BUILD-TABLEAU route (:full-tableau t, :devices > 1, :native nil, or numbers the double-float
;;;;    assembly would not reproduce bit for bit -- ratios, single-floats): the reference's exported
;;;;    build-tableau, the tableau coerced and uploaded, the solved values written back into the
;;;;    same `tableau`, which the reference's own methods (src/solver.lisp:61-80) serve.
;;;; What stays in Lisp either way: the DSL parser, the hook, the generics.  What moves to the GPU:
;;;; n-solve-tableau (src/simplex.lisp:399-461) -- pricing, ratio test, rank-1 update and the
;;;; two-phase hand-over -- in double-float arithmetic.
;;;;
;;;; Scope: LP, double-float.  Problems with integer / binary variables are declined with
;;;; unsupported-constraint-error (src/conditions.lisp:69-77) as the hook's contract expects of
;;;; a backend (src/solver.lisp:40-45); rational problems are solved in double-float (every
;;;; entry is coerced), which is the documented behaviour of this backend -- unless :exact t asks
;;;; for the reference's rational semantics: a problem whose numbers are all rational is then
;;;; solved on exact fraction-free integer tableaux (mi355x_xtab_*) and the tableau's matrix holds
;;;; the exact ratios afterwards.  Entries beyond (signed-byte 64), or values that outgrow 128 bits
;;;; (256 bits with :exact-max-bits 256) during the solve, are declined with unsupported-constraint-error.
;;;;
;;;; NOTE: could not be executed in the build image (no Lisp there); reviewed against
;;;; include/mi355x_simplex.h and the reference sources cited inline.

(defpackage :mi355x-simplex
  (:use :cl)
  (:import-from :linear-programming/simplex
                #:build-tableau #:tableau-matrix #:tableau-basis-columns
                #:tableau-var-count #:tableau-constraint-count #:tableau-instance-problem
                #:tableau-variable #:tableau-objective-value)
  (:import-from :linear-programming/problem
                #:problem-type #:problem-vars #:problem-objective-var #:problem-objective-func
                #:problem-integer-vars #:problem-var-bounds #:problem-constraints)
  (:import-from :linear-programming/solver
                #:solution-problem #:solution-objective-value #:solution-variable
                #:solution-reduced-cost)
  (:import-from :linear-programming/conditions
                #:solver-error #:unbounded-problem-error #:infeasible-problem-error
                #:unsupported-constraint-error)
  (:export #:mi355x-simplex-solver
           #:mi355x-solve-problems
           #:mi355x-solution
           #:solution-pivots
           #:free-solution
           #:native-var-mapping
           #:device-count
           #:mi355x-error))

(in-package :mi355x-simplex)

;;; ------------------------------------------------------------------ the shared library
(cffi:define-foreign-library libmi355x-simplex
  (:unix (:or "libmi355x_simplex.so" "./libmi355x_simplex.so"))
  (t (:default "libmi355x_simplex")))

(cffi:use-foreign-library libmi355x-simplex)

;; status codes, include/mi355x_simplex.h
(defconstant +mi-optimal+ 0)
(defconstant +mi-unbounded+ 1)
(defconstant +mi-infeasible+ 2)
(defconstant +mi-max-pivots+ 3)
(defconstant +mi-art-nonzero+ 4)
(defconstant +mi-art-stuck+ 5)
(defconstant +mi-nonfinite+ 6)   ; column shards only: the tableau overflowed (see solve-column-partitioned)
(defconstant +mi-cancelled+ 7)   ; mi355x_*_cancel from another thread (never from this single-threaded glue)
(defconstant +mi-running+ 100)
(defconstant +mi-unsupported+ -6)      ; a member of an exact batch whose start is not unit basis columns; a shape the batch declines
(defconstant +mi-exact-overflow+ -7)   ; an exact tableau outgrew 128 bits   ; per-LP status of a batch member a capped / cancelled solve left unfinished

(cffi:defcfun ("mi355x_device_count" device-count) :int)
(cffi:defcfun ("mi355x_last_error" %last-error) :string)
(cffi:defcfun ("mi355x_tab_create" %tab-create) :int
  (out :pointer) (rows :int64) (cols :int64) (host-matrix :pointer) (host-basis :pointer)
  (device :int))
(cffi:defcfun ("mi355x_tab_create_compact" %tab-create-compact) :int
  (out :pointer) (rows :int64) (var-count :int64) (n-stored :int64) (host-stored :pointer)
  (stored-cols :pointer) (host-basis :pointer) (device :int))
(cffi:defcfun ("mi355x_tab_destroy" %tab-destroy) :void (tab :pointer))
(cffi:defcfun ("mi355x_tab_solve" %tab-solve) :int
  (tab :pointer) (is-max :int) (fp-factor :double) (max-pivots :int64) (n-pivots :pointer))
(cffi:defcfun ("mi355x_solve_two_phase" %solve-two-phase) :int
  (art :pointer) (main :pointer) (main-is-max :int) (fp-factor :double) (n-pivots :pointer))
(cffi:defcfun ("mi355x_two_phase_handover" %two-phase-handover) :int
  (art :pointer) (main :pointer) (fp-factor :double) (n-driveout :pointer))
(cffi:defcfun ("mi355x_tab_download" %tab-download) :int
  (tab :pointer) (host-matrix :pointer) (host-basis :pointer) (last-row :pointer)
  (last-col :pointer))
;; one tableau column-partitioned over several GPUs (include/mi355x_simplex.h, mi355x_colpart_*)
(cffi:defcfun ("mi355x_colpart_create_on" %colpart-create-on) :int
  (out :pointer) (rows :int64) (cols :int64) (host-matrix :pointer) (host-basis :pointer)
  (n-devices :int) (device-ids :pointer))
(cffi:defcfun ("mi355x_colpart_solve_two_phase" %colpart-solve-two-phase) :int
  (art :pointer) (main-cols :int64) (main-objective-row :pointer) (main-is-max :int)
  (fp-factor :double) (n-pivots :pointer) (main-out :pointer))
(cffi:defcfun ("mi355x_colpart_solve" %colpart-solve) :int
  (handle :pointer) (is-max :int) (fp-factor :double) (max-pivots :int64) (n-pivots :pointer))
(cffi:defcfun ("mi355x_colpart_download" %colpart-download) :int
  (handle :pointer) (host-matrix :pointer) (host-basis :pointer) (last-row :pointer)
  (last-col :pointer))
(cffi:defcfun ("mi355x_colpart_destroy" %colpart-destroy) :void (handle :pointer))
;; a batch of same-shape tableaux over one or several GPUs (include/mi355x_simplex.h, mi355x_multibatch_*)
(cffi:defcfun ("mi355x_multibatch_create" %multibatch-create) :int
  (out :pointer) (n-lps :int64) (rows :int64) (cols :int64) (host-matrices :pointer)
  (host-bases :pointer) (n-devices :int) (device-ids :pointer))
(cffi:defcfun ("mi355x_multibatch_solve" %multibatch-solve) :int
  (handle :pointer) (is-max :int) (fp-factor :double) (max-pivots :int64) (status :pointer)
  (n-pivots :pointer))
(cffi:defcfun ("mi355x_multibatch_solve_two_phase" %multibatch-solve-two-phase) :int
  (art :pointer) (main :pointer) (main-is-max :int) (fp-factor :double) (status :pointer)
  (n-pivots :pointer))
(cffi:defcfun ("mi355x_multibatch_two_phase_handover" %multibatch-two-phase-handover) :int
  (art :pointer) (main :pointer) (fp-factor :double) (phase1-status :pointer) (status :pointer)
  (n-driveout :pointer))
(cffi:defcfun ("mi355x_multibatch_download" %multibatch-download) :int
  (handle :pointer) (lp-index :int64) (host-matrix :pointer) (host-basis :pointer)
  (last-row :pointer) (last-col :pointer))
(cffi:defcfun ("mi355x_multibatch_destroy" %multibatch-destroy) :void (handle :pointer))

;; the native route: problem -> (C++ build-tableau, GPU solve) -> light solution
;; (include/mi355x_simplex.h, "native host side of the hook")
(cffi:defcfun ("mi355x_problem_create" %problem-create) :int
  (out :pointer) (is-max :int) (n-vars :int64))
(cffi:defcfun ("mi355x_problem_set_objective" %problem-set-objective) :int
  (problem :pointer) (vars :pointer) (coefs :pointer) (nnz :int64))
(cffi:defcfun ("mi355x_problem_set_bounds" %problem-set-bounds) :int
  (problem :pointer) (var :int64) (has-lb :int) (lb :double) (has-ub :int) (ub :double))
(cffi:defcfun ("mi355x_problem_set_integer" %problem-set-integer) :int
  (problem :pointer) (var :int64))
(cffi:defcfun ("mi355x_problem_add_constraint" %problem-add-constraint) :int
  (problem :pointer) (op :int) (vars :pointer) (coefs :pointer) (nnz :int64) (rhs :double))
(cffi:defcfun ("mi355x_problem_destroy" %problem-destroy) :void (problem :pointer))
(cffi:defcfun ("mi355x_var_mapping" %var-mapping) :int
  (problem :pointer) (var :int64) (kind :pointer) (col :pointer) (offset :pointer))
(cffi:defcfun ("mi355x_simplex_solver" %simplex-solver) :int
  (problem :pointer) (fp-tolerance :double) (device :int) (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_begin" %solver-begin) :int
  (problem :pointer) (fp-tolerance :double) (device :int) (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_step" %solver-step) :int
  (job :pointer) (max-pivots :int64) (n-pivots :pointer))
(cffi:defcfun ("mi355x_simplex_solver_finish" %solver-finish) :int
  (job :pointer) (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_abandon" %solver-abandon) :void (job :pointer))
(cffi:defcfun ("mi355x_simplex_solver_many_begin" %solver-many-begin) :int
  (problems :pointer) (n :int64) (fp-tolerance :double) (n-devices :int) (device-ids :pointer)
  (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_many_step" %solver-many-step) :int
  (job :pointer) (max-pivots :int64) (status :pointer))
(cffi:defcfun ("mi355x_simplex_solver_many_finish" %solver-many-finish) :int
  (job :pointer) (status :pointer) (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_many_abandon" %solver-many-abandon) :void (job :pointer))
(cffi:defcfun ("mi355x_simplex_solver_bb_begin" %bb-begin) :int
  (problem :pointer) (int-order :pointer) (n-int :int64) (fp-tolerance :double) (int-tolerance :double)
  (width :int64) (n-devices :int) (device-ids :pointer) (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_bb_step" %bb-step) :int
  (job :pointer) (max-nodes :int64) (n-nodes :pointer))
(cffi:defcfun ("mi355x_simplex_solver_bb_finish" %bb-finish) :int
  (job :pointer) (out :pointer))
(cffi:defcfun ("mi355x_simplex_solver_bb_abandon" %bb-abandon) :void (job :pointer))
(cffi:defcfun ("mi355x_solution_objective_value" %solution-objective-value) :int
  (solution :pointer) (out :pointer))
(cffi:defcfun ("mi355x_solution_variable" %solution-variable) :int
  (solution :pointer) (var :int64) (out :pointer))
(cffi:defcfun ("mi355x_solution_reduced_cost" %solution-reduced-cost) :int
  (solution :pointer) (var :int64) (out :pointer))
(cffi:defcfun ("mi355x_solution_pivots" %solution-pivots) :int
  (solution :pointer) (phase1 :pointer) (phase2 :pointer))
(cffi:defcfun ("mi355x_solution_destroy" %solution-destroy) :void (solution :pointer))
(cffi:defcfun ("mi355x_xtab_create" %xtab-create) :int
  (out :pointer) (rows :int64) (cols :int64) (num :pointer) (den :pointer) (basis :pointer)
  (device :int) (min-bits :int))
(cffi:defcfun ("mi355x_xtab_create_wide" %xtab-create-wide) :int
  (out :pointer) (rows :int64) (cols :int64) (num :pointer) (den :pointer) (basis :pointer)
  (device :int) (min-bits :int) (max-bits :int))
(cffi:defcfun ("mi355x_xtab_solve" %xtab-solve) :int
  (tab :pointer) (is-max :int) (max-pivots :int64) (n-pivots :pointer))
(cffi:defcfun ("mi355x_xtab_solve_two_phase" %xtab-solve-two-phase) :int
  (art :pointer) (main :pointer) (main-is-max :int) (max-pivots :int64) (n-pivots :pointer))
(cffi:defcfun ("mi355x_xtab_download" %xtab-download) :int
  (tab :pointer) (num-lo-hi :pointer) (den-lo-hi :pointer) (basis :pointer))
(cffi:defcfun ("mi355x_xtab_download_limbs" %xtab-download-limbs) :int
  (tab :pointer) (limbs :int) (num-limbs :pointer) (den-limbs :pointer) (basis :pointer))
(cffi:defcfun ("mi355x_xtab_destroy" %xtab-destroy) :void (tab :pointer))
(cffi:defcfun ("mi355x_xtab_set_pivot_rule" %xtab-set-pivot-rule) :int (tab :pointer) (rule :int))
(cffi:defcfun ("mi355x_xbatch_create" %xbatch-create) :int
  (out :pointer) (n-lps :int64) (rows :int64) (cols :int64) (num :pointer) (den :pointer) (basis :pointer)
  (device :int) (min-bits :int))
(cffi:defcfun ("mi355x_xbatch_solve" %xbatch-solve) :int
  (batch :pointer) (is-max :int) (max-pivots :int64) (status :pointer) (n-pivots :pointer))
(cffi:defcfun ("mi355x_xbatch_solve_two_phase" %xbatch-solve-two-phase) :int
  (art :pointer) (main :pointer) (main-is-max :int) (max-pivots :int64) (status :pointer) (n-pivots :pointer))
(cffi:defcfun ("mi355x_xbatch_download" %xbatch-download) :int
  (batch :pointer) (lp-index :int64) (num-lo-hi :pointer) (den-lo-hi :pointer) (basis :pointer))
(cffi:defcfun ("mi355x_xbatch_destroy" %xbatch-destroy) :void (batch :pointer))
(cffi:defcfun ("mi355x_xbatch_set_pivot_rule" %xbatch-set-pivot-rule) :int (batch :pointer) (rule :int))
(cffi:defcfun ("mi355x_xbb_base_create" %xbb-base-create) :int
  (out :pointer) (rows :int64) (cols :int64) (num :pointer) (den :pointer) (basis :pointer) (ncv :int64)
  (nb :int64) (n-vars :int64) (kind :pointer) (col :pointer) (off-num :pointer) (off-den :pointer) (device :int))
(cffi:defcfun ("mi355x_xbb_base_destroy" %xbb-base-destroy) :void (base :pointer))
(cffi:defcfun ("mi355x_xbatch_create_nodes" %xbatch-create-nodes) :int
  (out-main :pointer) (out-art :pointer) (base :pointer) (n-nodes :int64) (depth :int64) (var :pointer)
  (sense :pointer) (bound :pointer) (min-bits :int))
(cffi:defcfun ("mi355x_xbatch_readback" %xbatch-readback) :int
  (batch :pointer) (values-lo-hi :pointer) (basis :pointer) (status :pointer))
;; single-float tableaux (include/mi355x_simplex.h, mi355x_stab_*): the reference's single-float path
(cffi:defcfun ("mi355x_stab_create" %stab-create) :int
  (out :pointer) (rows :int64) (cols :int64) (matrix :pointer) (basis :pointer) (device :int))
(cffi:defcfun ("mi355x_stab_solve" %stab-solve) :int
  (tab :pointer) (is-max :int) (fp-factor :double) (max-pivots :int64) (n-pivots :pointer))
(cffi:defcfun ("mi355x_stab_solve_two_phase" %stab-solve-two-phase) :int
  (art :pointer) (main :pointer) (main-is-max :int) (fp-factor :double) (max-pivots :int64)
  (pivots-out :pointer))
(cffi:defcfun ("mi355x_stab_download" %stab-download) :int
  (tab :pointer) (matrix :pointer) (basis :pointer) (last-row :pointer) (last-col :pointer))
(cffi:defcfun ("mi355x_stab_destroy" %stab-destroy) :void (tab :pointer))
;; batches of single-float LPs (mi355x_sbatch_*): one workgroup per member, the member's tableau in LDS
(cffi:defcfun ("mi355x_sbatch_create" %sbatch-create) :int
  (out :pointer) (n-lps :int64) (rows :int64) (cols :int64) (matrices :pointer) (basis :pointer)
  (device :int))
(cffi:defcfun ("mi355x_sbatch_solve" %sbatch-solve) :int
  (batch :pointer) (is-max :int) (fp-factor :double) (max-pivots :int64) (status :pointer)
  (n-pivots :pointer))
(cffi:defcfun ("mi355x_sbatch_solve_two_phase" %sbatch-solve-two-phase) :int
  (art :pointer) (main :pointer) (main-is-max :int) (fp-factor :double) (max-pivots :int64)
  (status :pointer) (n-pivots :pointer))
(cffi:defcfun ("mi355x_sbatch_download" %sbatch-download) :int
  (batch :pointer) (lp-index :int64) (matrix :pointer) (basis :pointer) (last-row :pointer)
  (last-col :pointer))
(cffi:defcfun ("mi355x_sbatch_destroy" %sbatch-destroy) :void (batch :pointer))

(define-condition mi355x-error (solver-error)
  ((code :initarg :code :reader mi355x-error-code)
   (message :initarg :message :reader mi355x-error-message))
  (:report (lambda (err stream)
             (format stream "libmi355x_simplex failed with status ~D: ~A"
                     (mi355x-error-code err) (mi355x-error-message err)))))

(defun check (code)
  "Negative statuses are library errors (MI_BAD_ARG, MI_HIP_ERROR, MI_NO_DEVICE ...)."
  (when (minusp code)
    (error 'mi355x-error :code code :message (%last-error)))
  code)

(defmacro with-foreign-fp-mode (&body body)
  "SBCL enables floating point traps; foreign code that produces an inf/nan must not raise
SIGFPE in the Lisp thread."
  #+sbcl `(sb-int:with-float-traps-masked (:overflow :invalid :divide-by-zero :inexact)
            ,@body)
  #-sbcl `(progn ,@body))

;;; ------------------------------------------------------------------ tableau <-> raw doubles
(defun tableau->vectors (tableau)
  "Flatten the boxed (simple-array real 2) of src/simplex.lisp:53 into a row-major
(simple-array double-float (*)) and the fixnum basis (tagged words: never hand their storage
to C) into a (signed-byte 64) vector."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (flat (make-array (* rows cols) :element-type 'double-float))
         (basis-src (tableau-basis-columns tableau))
         (basis (make-array (max 1 (length basis-src)) :element-type '(signed-byte 64)
                                                       :initial-element 0)))
    (dotimes (r rows)
      (dotimes (c cols)
        (setf (aref flat (+ (* r cols) c))
              (coerce (aref matrix r c) 'double-float))))
    (dotimes (i (length basis-src))
      (setf (aref basis i) (aref basis-src i)))
    (values flat basis rows cols)))

(defun vectors->tableau (tableau flat basis)
  "Write the solved values back into the tableau's own arrays (the struct slots are read-only,
the arrays are not), so tableau-variable & co. (src/simplex.lisp:74-120) read GPU results."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (basis-dst (tableau-basis-columns tableau)))
    (dotimes (r rows)
      (dotimes (c cols)
        (setf (aref matrix r c) (aref flat (+ (* r cols) c)))))
    (dotimes (i (length basis-dst))
      (setf (aref basis-dst i) (aref basis i)))
    tableau))

(defun upload-tableau (tableau device)
  "Returns (values handle flat basis): a device handle plus the host staging vectors."
  (multiple-value-bind (flat basis rows cols) (tableau->vectors tableau)
    (cffi:with-foreign-object (out :pointer)
      (cffi:with-pointer-to-vector-data (pm flat)
        (cffi:with-pointer-to-vector-data (pb basis)
          (check (with-foreign-fp-mode
                   (%tab-create out rows cols pm pb device)))))
      (values (cffi:mem-ref out :pointer) flat basis))))

(defun exact-unit-entry-p (x one)
  "X is exactly 1 (ONE true) / exactly +0 (ONE false): the integers build-tableau stores
(src/simplex.lisp:217-219, 255-259) or their float forms, never -0.0."
  (if one
      (= x 1)
      (and (zerop x) (not (and (floatp x) (minusp (float-sign x)))))))

(defun unit-basis-p (tableau)
  "True when every basis column is exactly the unit vector of its row (objective row included):
what build-tableau produces for the slack columns of a single-phase problem."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (var-count (1- (array-dimension matrix 1)))
         (basis (tableau-basis-columns tableau))
         (seen (make-array var-count :element-type 'bit :initial-element 0)))
    (dotimes (i (length basis) t)
      (let ((b (aref basis i)))
        (unless (and (integerp b) (<= 0 b) (< b var-count) (zerop (aref seen b)))
          (return nil))
        (setf (aref seen b) 1)
        (dotimes (r rows)
          (unless (exact-unit-entry-p (aref matrix r b) (= r i))
            (return-from unit-basis-p nil)))))))

(defun upload-tableau-compact (tableau device)
  "Single-phase problems: only [non-basic columns | RHS] is coerced and crosses PCIe
(mi355x_tab_create_compact); the slack identity block -- a third of the boxed matrix at n = 2m --
is neither converted nor uploaded, and no dense device buffer exists for a plain solve with the
light read-back.  Returns (values handle basis), or NIL when the basis columns are not exact unit
vectors (the caller then uploads the dense tableau)."
  (when (and (plusp (length (tableau-basis-columns tableau))) (unit-basis-p tableau))
    (let* ((matrix (tableau-matrix tableau))
           (rows (array-dimension matrix 0))
           (var-count (1- (array-dimension matrix 1)))
           (basis-src (tableau-basis-columns tableau))
           (m (length basis-src))
           (n-stored (- var-count m))
           (basic (make-array var-count :element-type 'bit :initial-element 0)))
      (when (plusp n-stored)
        (dotimes (i m) (setf (aref basic (aref basis-src i)) 1))
        (let ((stored-cols (make-array n-stored :element-type '(signed-byte 64)))
              (stored (make-array (* rows (1+ n-stored)) :element-type 'double-float))
              (basis (make-array m :element-type '(signed-byte 64)))
              (j 0))
          (dotimes (c var-count)
            (when (zerop (aref basic c))
              (setf (aref stored-cols j) c)
              (incf j)))
          (dotimes (r rows)
            (let ((base (* r (1+ n-stored))))
              (dotimes (k n-stored)
                (setf (aref stored (+ base k))
                      (coerce (aref matrix r (aref stored-cols k)) 'double-float)))
              (setf (aref stored (+ base n-stored))
                    (coerce (aref matrix r var-count) 'double-float))))
          (dotimes (i m) (setf (aref basis i) (aref basis-src i)))
          (cffi:with-foreign-object (out :pointer)
            (cffi:with-pointer-to-vector-data (ps stored)
              (cffi:with-pointer-to-vector-data (pc stored-cols)
                (cffi:with-pointer-to-vector-data (pb basis)
                  (check (with-foreign-fp-mode
                           (%tab-create-compact out rows var-count n-stored ps pc pb device))))))
            (values (cffi:mem-ref out :pointer) basis)))))))

(defun download-tableau (handle tableau flat basis)
  "Full write-back: every entry of the solved tableau (400 MB and 5e7 boxed doubles at
8192 x 4096 -- only worth it when the caller wants to look inside the tableau)."
  (cffi:with-pointer-to-vector-data (pm flat)
    (cffi:with-pointer-to-vector-data (pb basis)
      (check (%tab-download handle pm pb (cffi:null-pointer) (cffi:null-pointer)))))
  (vectors->tableau tableau flat basis))

(defun download-solution (handle tableau basis)
  "Light write-back (the default): the objective row, the RHS column and the basis are all
that tableau-objective-value, tableau-variable and tableau-reduced-cost read
(src/simplex.lisp:74-120), so only those are fetched and stored into the tableau's arrays;
the interior of the matrix keeps its pre-solve contents."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (last-row (make-array cols :element-type 'double-float))
         (last-col (make-array rows :element-type 'double-float))
         (basis-dst (tableau-basis-columns tableau)))
    (cffi:with-pointer-to-vector-data (pr last-row)
      (cffi:with-pointer-to-vector-data (pc last-col)
        (cffi:with-pointer-to-vector-data (pb basis)
          (check (%tab-download handle (cffi:null-pointer) pb pr pc)))))
    (dotimes (r rows)
      (setf (aref matrix r (1- cols)) (aref last-col r)))
    (dotimes (c cols)
      (setf (aref matrix (1- rows) c) (aref last-row c)))
    (dotimes (i (length basis-dst))
      (setf (aref basis-dst i) (aref basis i)))
    tableau))

;;; ------------------------------------------------------------------ several GPUs
(defun device-count-of (devices)
  "DEVICES is a count (devices 0 .. n-1) or a list of device ids."
  (if (listp devices) (length devices) devices))

(defun colpart-create (flat basis rows cols devices)
  "mi355x_colpart_create_on: one shard per device of DEVICES (a count, or a list of distinct ids)."
  (let ((n (device-count-of devices)))
    (cffi:with-foreign-object (out :pointer)
      (cffi:with-foreign-object (ids :int (max n 1))
        (when (listp devices)
          (loop for d in devices for i from 0 do (setf (cffi:mem-aref ids :int i) d)))
        (cffi:with-pointer-to-vector-data (pm flat)
          (cffi:with-pointer-to-vector-data (pb basis)
            (check (with-foreign-fp-mode
                     (%colpart-create-on out rows cols pm pb n
                                         (if (listp devices) ids (cffi:null-pointer))))))))
      (cffi:mem-ref out :pointer))))

(defun colpart-read-back (handle tableau flat basis rows cols full-tableau)
  "Full or light write-back from a column-partitioned handle into TABLEAU's arrays."
  (let* ((matrix (tableau-matrix tableau))
         (last-row (make-array cols :element-type 'double-float))
         (last-col (make-array rows :element-type 'double-float))
         (basis-dst (tableau-basis-columns tableau)))
    (cffi:with-pointer-to-vector-data (pr last-row)
      (cffi:with-pointer-to-vector-data (pc last-col)
        (cffi:with-pointer-to-vector-data (pb basis)
          (if full-tableau
              (cffi:with-pointer-to-vector-data (pm flat)
                (check (%colpart-download handle pm pb pr pc)))
              (check (%colpart-download handle (cffi:null-pointer) pb pr pc))))))
    (if full-tableau
        (vectors->tableau tableau flat basis)
        (progn
          (dotimes (r rows) (setf (aref matrix r (1- cols)) (aref last-col r)))
          (dotimes (c cols) (setf (aref matrix (1- rows) c) (aref last-row c)))
          (dotimes (i (length basis-dst)) (setf (aref basis-dst i) (aref basis i)))
          tableau))))

(defun solve-two-phase-column-partitioned (art-tab main-tab devices factor full-tableau n-pivots)
  "Two-phase n-solve-tableau (src/simplex.lisp:402-452) with the ARTIFICIAL tableau
column-partitioned over DEVICES: phase 1, the drive-out pivots, the hand-over and phase 2 all stay
on the partition (mi355x_colpart_solve_two_phase).  The main tableau is not uploaded -- the library
takes its objective row only; its constraint rows are the artificial tableau's.  Returns
:unsupported / :overflowed when the partitioned path does not apply (the caller's tableaux are
untouched and it solves them on one device)."
  (multiple-value-bind (art-flat art-basis rows art-cols) (tableau->vectors art-tab)
    (let* ((main-matrix (tableau-matrix main-tab))
           (main-cols (array-dimension main-matrix 1))
           (objective (make-array main-cols :element-type 'double-float))
           (art-handle (colpart-create art-flat art-basis rows art-cols devices))
           (main-handle (cffi:null-pointer)))
      (dotimes (c main-cols)
        (setf (aref objective c) (coerce (aref main-matrix (1- rows) c) 'double-float)))
      (unwind-protect
           (let ((status
                   (cffi:with-foreign-object (out :pointer)
                     (setf (cffi:mem-ref out :pointer) (cffi:null-pointer))
                     (prog1
                         (cffi:with-pointer-to-vector-data (po objective)
                           (with-foreign-fp-mode
                             (%colpart-solve-two-phase art-handle main-cols po
                                                       (max-problem-p main-tab) factor n-pivots
                                                       out)))
                       (setf main-handle (cffi:mem-ref out :pointer))))))
             (cond
               ((= status -6) :unsupported)                 ; MI_UNSUPPORTED: artificial basis not unit columns
               ((= status +mi-nonfinite+) :overflowed)
               (t
                (check status)
                (signal-outcome status)
                (let ((main-flat (make-array (* rows main-cols) :element-type 'double-float))
                      (main-basis (make-array (max 1 (1- rows)) :element-type '(signed-byte 64)
                                                                :initial-element 0)))
                  (colpart-read-back main-handle main-tab main-flat main-basis rows main-cols
                                     full-tableau)))))
        (unless (cffi:null-pointer-p main-handle) (%colpart-destroy main-handle))
        (%colpart-destroy art-handle)))))

(defun solve-column-partitioned (tableau devices factor max-pivots full-tableau n-pivots)
  "Single-phase n-solve-tableau (src/simplex.lisp:453-461) with the tableau's non-basic columns
distributed over DEVICES GPUs of this node (RCCL over xGMI inside the library; logical shards on
one GPU when fewer are visible).  Same pivots, same bits as on one device."
  (multiple-value-bind (flat basis rows cols) (tableau->vectors tableau)
    (let ((handle (colpart-create flat basis rows cols devices)))
      (unwind-protect
           (let ((status (solve-in-chunks
                          (lambda (cap) (%colpart-solve handle (max-problem-p tableau) factor cap n-pivots))
                          rows cols max-pivots n-pivots)))
             ;; A compact column shard cannot do what the reference does with an entering column
             ;; that holds an infinity or a NaN (it would turn basic columns, which a shard does not
             ;; store, into NaNs): the library stops with MI_NONFINITE and the caller, whose tableau
             ;; has not been written to, solves it on one device, where that case is reproduced.
             (when (= status +mi-nonfinite+)
               (return-from solve-column-partitioned :overflowed))
             (signal-outcome status)
             (colpart-read-back handle tableau flat basis rows cols full-tableau))
        (%colpart-destroy handle)))))

(defun signal-outcome (status)
  "C outcome -> the reference's conditions (src/conditions.lisp:43-60)."
  (cond
    ((= status +mi-optimal+) nil)
    ((= status +mi-unbounded+) (error 'unbounded-problem-error))     ; src/simplex.lisp:458-459
    ((= status +mi-infeasible+) (error 'infeasible-problem-error))   ; src/simplex.lisp:405-407
    ((= status +mi-art-nonzero+) (error "Artificial variable still non-zero"))
    ((= status +mi-art-stuck+)
     (error "Artificial variable still in basis and cannot be replaced"))
    ((= status +mi-max-pivots+) (error 'mi355x-error :code status :message "pivot cap reached"))
    (t (error 'mi355x-error :code status :message "unknown status"))))

(defun max-problem-p (tableau)
  (if (eq 'max (problem-type (tableau-instance-problem tableau))) 1 0))

;;; ------------------------------------------------------------------ a way out of a solve
;;; The reference's loop has no iteration cap and no anti-cycling rule (src/simplex.lisp:453-461):
;;; an LP that cycles under Dantzig's rule with lowest-index ties runs for ever.  In Lisp that
;;; loop can be interrupted (C-c, sb-ext:with-timeout, bt:interrupt-thread); one blocking foreign
;;; call cannot.  So the glue never makes an unbounded foreign call for a single-phase solve: it
;;; asks for CHUNK pivots at a time (MI_MAX_PIVOTS = "chunk used up, still running") and is back
;;; in Lisp -- where pending interrupts are served -- a few times per second.  A solve continued
;;; call by call takes exactly the pivots of one long call (the cap is a test in the select step;
;;; pinned by the test-suite through the Python mirror's identical loop).  Other threads can
;;; also end a blocking call with mi355x_tab_cancel / mi355x_colpart_cancel (MI_CANCELLED).
(defun chunk-pivots (rows cols)
  "Pivots per foreign call: about a tenth to half a second of GPU time at every size (one pivot
moves 16 rows x cols bytes through HBM per 16 pivots; small tableaux cost ~4 us per pivot)."
  (max 1024 (min 65536 (floor (expt 2 36) (max 1 (* rows cols))))))

(defun solve-in-chunks (solve-fn rows cols max-pivots n-pivots)
  "Calls (funcall SOLVE-FN cap) -- cap pivots of n-solve-tableau, *N-PIVOTS = pivots of that call
-- until the status is something else than MI_MAX_PIVOTS or MAX-PIVOTS (0 = no cap) are used up.
Leaves the total in N-PIVOTS[0] and returns the last status."
  (let ((chunk (chunk-pivots rows cols))
        (total 0))
    (loop
      (let* ((cap (if (plusp max-pivots) (min chunk (- max-pivots total)) chunk))
             (status (check (with-foreign-fp-mode (funcall solve-fn cap)))))
        (incf total (cffi:mem-aref n-pivots :int64 0))
        (when (or (/= status +mi-max-pivots+)
                  (and (plusp max-pivots) (>= total max-pivots)))
          (setf (cffi:mem-aref n-pivots :int64 0) total)
          (return status))))))

;;; ------------------------------------------------------------------ single-float solves
;;; :precision :single.  The Lisp reader makes 0.5 a SINGLE-FLOAT, and the reference then solves in
;;; single-float arithmetic with single-float thresholds (src/utils.lisp:84-124).  The reference's own
;;; build-tableau produces the tableau; every entry must be a single-float or an integer of at most 2^24
;;; in magnitude (anything else -- a double-float, a ratio, a larger integer -- is declined, never rounded
;;; silently); the entries cross the boundary as single-floats, the library solves in IEEE binary32
;;; (include/mi355x_simplex.h, mi355x_stab_*) in bounded chunks, and the solved single-floats are written
;;; back into the same `tableau`, which the reference's own methods then serve (src/solver.lisp:61-80).
(defun single-entry-p (x)
  (or (typep x 'single-float) (and (integerp x) (<= (abs x) 16777216))))

(defun single-tableau->vectors (tableau)
  "tableau->vectors in single-float; an entry that is neither a single-float nor an integer a
single-float holds exactly is declined: unsupported-constraint-error (single ENTRY)."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (flat (make-array (* rows cols) :element-type 'single-float))
         (basis-src (tableau-basis-columns tableau))
         (basis (make-array (max 1 (length basis-src)) :element-type '(signed-byte 64)
                                                       :initial-element 0)))
    (dotimes (r rows)
      (dotimes (c cols)
        (let ((x (aref matrix r c)))
          (unless (single-entry-p x)
            (error 'unsupported-constraint-error :constraint (list 'single x)
                                                 :solver-name "mi355x-simplex"))
          (setf (aref flat (+ (* r cols) c)) (coerce x 'single-float)))))
    (dotimes (i (length basis-src))
      (setf (aref basis i) (aref basis-src i)))
    (values flat basis rows cols)))

(defun upload-single-tableau (tableau device)
  "Returns (values handle flat basis): a mi355x_stab handle plus the host staging vectors."
  (multiple-value-bind (flat basis rows cols) (single-tableau->vectors tableau)
    (cffi:with-foreign-object (out :pointer)
      (cffi:with-pointer-to-vector-data (pm flat)
        (cffi:with-pointer-to-vector-data (pb basis)
          (check (with-foreign-fp-mode
                   (%stab-create out rows cols pm pb device)))))
      (values (cffi:mem-ref out :pointer) flat basis))))

(defun download-single-tableau (handle tableau flat basis)
  "Every entry of the solved tableau, as single-floats, into the tableau's own arrays."
  (cffi:with-pointer-to-vector-data (pm flat)
    (cffi:with-pointer-to-vector-data (pb basis)
      (check (%stab-download handle pm pb (cffi:null-pointer) (cffi:null-pointer)))))
  (vectors->tableau tableau flat basis))

(defun single-solve-two-phase-in-chunks (art-handle main-handle rows cols main-is-max factor max-pivots
                                         n-pivots)
  "mi355x_stab_solve_two_phase is resumable: CHUNK pivots per call (both phases and the drive-out
pivots together) until the status is something else than MI_MAX_PIVOTS or MAX-PIVOTS (0 = no cap) are
used up.  Returns the last status."
  (let ((chunk (chunk-pivots rows cols))
        (total 0))
    (loop
      (let* ((cap (if (plusp max-pivots) (min chunk (- max-pivots total)) chunk))
             (status (check (with-foreign-fp-mode
                              (%stab-solve-two-phase art-handle main-handle main-is-max factor cap
                                                     n-pivots)))))
        (incf total (+ (cffi:mem-aref n-pivots :int64 0) (cffi:mem-aref n-pivots :int64 1)))
        (when (or (/= status +mi-max-pivots+)
                  (and (plusp max-pivots) (>= total max-pivots)))
          (return status))))))

(defun check-precision (precision exact branch-and-bound devices native full-tableau pivot-rule)
  "The argument errors of :PRECISION: an unknown value, and :SINGLE together with a keyword that asks for
another path."
  (unless (member precision '(:double :single))
    (error "MI355X-SIMPLEX-SOLVER: :precision must be :double or :single, not ~S" precision))
  (when (eq precision :single)
    (let ((clash (cond (exact :exact)
                       (branch-and-bound :branch-and-bound)
                       ((> (device-count-of devices) 1) :devices)
                       ((eq native t) :native)
                       (full-tableau :full-tableau)
                       ((not (eq pivot-rule :dantzig)) :pivot-rule))))
      (when clash
        (error "MI355X-SIMPLEX-SOLVER: :precision :single does not go with ~S" clash)))))

(defun solve-in-single-precision (problem fp-tolerance device max-pivots)
  "The :precision :single route of mi355x-simplex-solver: returns the solved `tableau`, every entry a
single-float."
  (when (problem-integer-vars problem)
    (error 'unsupported-constraint-error
           :constraint (cons 'integer (problem-integer-vars problem))
           :solver-name "mi355x-simplex"))
  (let ((tableaus (build-tableau problem problem :fp-tolerance-factor fp-tolerance))
        (factor (coerce fp-tolerance 'double-float)))
    (cffi:with-foreign-object (n-pivots :int64 2)
      (if (listp tableaus)
          (destructuring-bind (art-tab main-tab) tableaus
            (multiple-value-bind (art-handle art-flat art-basis) (upload-single-tableau art-tab device)
              (declare (ignorable art-flat art-basis))
              (unwind-protect
                   (multiple-value-bind (main-handle main-flat main-basis)
                       (upload-single-tableau main-tab device)
                     (unwind-protect
                          (let ((status (single-solve-two-phase-in-chunks
                                         art-handle main-handle
                                         (array-dimension (tableau-matrix art-tab) 0)
                                         (array-dimension (tableau-matrix art-tab) 1)
                                         (max-problem-p main-tab) factor max-pivots n-pivots)))
                            (signal-outcome status)
                            (download-single-tableau main-handle main-tab main-flat main-basis))
                       (%stab-destroy main-handle)))
                (%stab-destroy art-handle))))
          (multiple-value-bind (handle flat basis) (upload-single-tableau tableaus device)
            (unwind-protect
                 (let ((status (solve-in-chunks
                                (lambda (cap) (%stab-solve handle (max-problem-p tableaus) factor cap
                                                           n-pivots))
                                (1+ (tableau-constraint-count tableaus))
                                (1+ (tableau-var-count tableaus)) max-pivots n-pivots)))
                   (signal-outcome status)
                   (download-single-tableau handle tableaus flat basis))
              (%stab-destroy handle)))))))

;;; Lists of problems under :precision :single (mi355x-solve-problems): the members of one shape and sense
;;; side by side as ONE batch of single-float tableaux (mi355x_sbatch_*: one workgroup per member for its
;;; whole solve, both phases and everything between them on the device), member by member what
;;; solve-in-single-precision gives the member alone.  A member is a list (tableau flat basis): the
;;; reference's build-tableau result and its single-float staging vectors.
(defun single-member (tableau)
  "(tableau flat basis); declines as single-tableau->vectors does."
  (multiple-value-bind (flat basis) (single-tableau->vectors tableau)
    (list tableau flat basis)))

(defun sbatch-create (members device)
  "MEMBERS of ONE shape, back to back behind one mi355x_sbatch handle.  Returns the handle, or NIL when the
library declines the shape (MI_UNSUPPORTED: a member does not fit the LDS budget)."
  (let* ((n (length members))
         (matrix (tableau-matrix (first (first members))))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (m (1- rows))
         (flat (make-array (* n rows cols) :element-type 'single-float))
         (bases (make-array (max 1 (* n m)) :element-type '(signed-byte 64) :initial-element 0)))
    (loop for (nil member-flat member-basis) in members for k from 0
          do (dotimes (i (* rows cols))
               (setf (aref flat (+ (* k rows cols) i)) (aref member-flat i)))
             (dotimes (i m)
               (setf (aref bases (+ (* k m) i)) (aref member-basis i))))
    (cffi:with-foreign-object (out :pointer)
      (let ((code (cffi:with-pointer-to-vector-data (pm flat)
                    (cffi:with-pointer-to-vector-data (pb bases)
                      (with-foreign-fp-mode
                        (%sbatch-create out n rows cols pm pb device))))))
        (if (= code +mi-unsupported+)
            nil
            (progn (check code) (cffi:mem-ref out :pointer)))))))

(defun sbatch-solve-in-chunks (solve-fn rows cols max-pivots n status)
  "Calls (funcall SOLVE-FN cap) -- one bounded foreign call on a batch, CAP pivots per member -- until no
member is left at MI_MAX_PIVOTS or MAX-PIVOTS (0 = no cap) are used up: a further call carries every
unfinished member on and does not touch a finished one.  STATUS (int32 x N) holds the members' statuses."
  (let ((chunk (chunk-pivots rows cols))
        (done 0))
    (loop
      (let ((cap (if (plusp max-pivots) (min chunk (- max-pivots done)) chunk)))
        (check (with-foreign-fp-mode (funcall solve-fn cap)))
        (incf done cap)
        (when (or (and (plusp max-pivots) (>= done max-pivots))
                  (loop for k below n
                        never (= (cffi:mem-aref status :int32 k) +mi-max-pivots+)))
          (return done))))))

(defun sbatch-read-back (handle k member)
  "Member K of a batch: every solved single-float into the member's own tableau."
  (destructuring-bind (tableau flat basis) member
    (cffi:with-pointer-to-vector-data (pm flat)
      (cffi:with-pointer-to-vector-data (pb basis)
        (check (%sbatch-download handle k pm pb (cffi:null-pointer) (cffi:null-pointer)))))
    (vectors->tableau tableau flat basis)))

(defun solve-single-batch (members device factor max-pivots)
  "MEMBERS: single-phase members of ONE shape and ONE sense.  Returns a list parallel to MEMBERS -- the
solved tableau, or a condition object -- or :DECLINED when the library declines the shape."
  (let ((handle (sbatch-create members device)))
    (if (null handle)
        :declined
        (unwind-protect
             (let* ((n (length members))
                    (tableau (first (first members)))
                    (matrix (tableau-matrix tableau)))
               (cffi:with-foreign-objects ((status :int32 n) (pivots :int64 n))
                 (sbatch-solve-in-chunks
                  (lambda (cap) (%sbatch-solve handle (max-problem-p tableau) factor cap status pivots))
                  (array-dimension matrix 0) (array-dimension matrix 1) max-pivots n status)
                 (loop for member in members for k from 0
                       collect (or (outcome-condition (cffi:mem-aref status :int32 k))
                                   (sbatch-read-back handle k member)))))
          (%sbatch-destroy handle)))))

(defun solve-single-two-phase-batch (pairs device factor max-pivots)
  "PAIRS: lists (art-member main-member) of ONE shape each and one sense.  One pair of batches, both phases
and the step between them per member on the device (mi355x_sbatch_solve_two_phase in bounded calls;
MAX-PIVOTS caps both phases and the drive-outs together, as for a member alone).  Returns a list parallel
to PAIRS, or :DECLINED."
  (let ((art-handle (sbatch-create (mapcar #'first pairs) device))
        (main-handle nil))
    (if (null art-handle)
        :declined
        (unwind-protect
             (progn
               (setf main-handle (sbatch-create (mapcar #'second pairs) device))
               (if (null main-handle)
                   :declined
                   (let* ((n (length pairs))
                          (main-tableau (first (second (first pairs))))
                          (art-matrix (tableau-matrix (first (first (first pairs))))))
                     (cffi:with-foreign-objects ((status :int32 n) (pivots :int64 (* 2 n)))
                       (sbatch-solve-in-chunks
                        (lambda (cap) (%sbatch-solve-two-phase art-handle main-handle
                                                               (max-problem-p main-tableau) factor cap
                                                               status pivots))
                        (array-dimension art-matrix 0) (array-dimension art-matrix 1) max-pivots n status)
                       (loop for (nil main-member) in pairs for k from 0
                             collect (or (outcome-condition (cffi:mem-aref status :int32 k))
                                         (sbatch-read-back main-handle k main-member)))))))
          (when main-handle (%sbatch-destroy main-handle))
          (%sbatch-destroy art-handle)))))

(defun check-list-precision (precision exact native devices pivot-rule)
  "The argument errors of mi355x-solve-problems' :PRECISION: an unknown value, and :SINGLE together with a
keyword that asks for another path (the single-float batch is one device and the reference's rule)."
  (unless (member precision '(:double :single))
    (error "MI355X-SOLVE-PROBLEMS: :precision must be :double or :single, not ~S" precision))
  (when (eq precision :single)
    (let ((clash (cond (exact :exact)
                       ((eq native :many) :native)
                       ((> (device-count-of devices) 1) :devices)
                       ((not (eq pivot-rule :dantzig)) :pivot-rule))))
      (when clash
        (error "MI355X-SOLVE-PROBLEMS: :precision :single does not go with ~S" clash)))))

(defun solve-problems-in-single-precision (problems fp-tolerance device max-pivots)
  "The :precision :single route of mi355x-solve-problems: the reference's build-tableau and the
single-entry-p check per member (a declined member's condition takes its place), single-phase members
grouped by (rows cols sense), two-phase members by (rows art-cols main-cols sense), a group of two or more
as one batch; members alone in their group, shapes the batch declines and integer problems go through
(mi355x-simplex-solver p :precision :single) one by one.  Returns the list of results."
  (let* ((n (length problems))
         (results (make-array n :initial-element nil))
         (groups (make-hash-table :test #'equal))
         (groups2 (make-hash-table :test #'equal))
         (factor (coerce fp-tolerance 'double-float)))
    (flet ((solve-alone (k)
             (setf (aref results k)
                   (handler-case (mi355x-simplex-solver (nth k problems) :fp-tolerance fp-tolerance
                                                                         :device device
                                                                         :max-pivots max-pivots
                                                                         :precision :single)
                     (error (c) c)))))
      (loop for problem in problems for k from 0
            do (if (problem-integer-vars problem)
                   (solve-alone k)                     ; -> unsupported-constraint-error
                   (let ((built (handler-case
                                    (let ((tableaus (build-tableau problem problem
                                                                   :fp-tolerance-factor fp-tolerance)))
                                      (if (listp tableaus)
                                          (mapcar #'single-member tableaus)
                                          (single-member tableaus)))
                                  (error (c) c))))
                     (cond
                       ((typep built 'condition) (setf (aref results k) built))
                       ((listp (first built))          ; two-phase: (art-member main-member)
                        (let ((art (tableau-matrix (first (first built))))
                              (main (tableau-matrix (first (second built)))))
                          (push (cons k built)
                                (gethash (list (array-dimension art 0) (array-dimension art 1)
                                               (array-dimension main 1)
                                               (max-problem-p (first (second built))))
                                         groups2))))
                       (t
                        (let ((matrix (tableau-matrix (first built))))
                          (push (cons k built)
                                (gethash (list (array-dimension matrix 0) (array-dimension matrix 1)
                                               (max-problem-p (first built)))
                                         groups))))))))
      (flet ((solve-groups (table solve-fn)
               (maphash
                (lambda (shape members)
                  (declare (ignore shape))
                  (setf members (reverse members))
                  (let ((outcomes (if (rest members)
                                      (funcall solve-fn (mapcar #'cdr members) device factor max-pivots)
                                      :declined)))
                    (if (eq outcomes :declined)
                        (loop for (k . nil) in members do (solve-alone k))
                        (loop for (k . nil) in members
                              for outcome in outcomes
                              do (setf (aref results k) outcome)))))
                table)))
        (solve-groups groups #'solve-single-batch)
        (solve-groups groups2 #'solve-single-two-phase-batch)))
    (coerce results 'list)))

;;; ------------------------------------------------------------------ exact rational solves
;;; :exact t.  The reference's build-tableau already yields the rational matrix; its numerators and
;;; denominators cross the boundary, the library solves on a fraction-free integer tableau T with one
;;; denominator D (include/mi355x_simplex.h, mi355x_xtab_*), and (/ T D) is written back into the
;;; same `tableau`, which the reference's own methods then serve (src/solver.lisp:61-80).
(defun rational-numbers-p (problem)
  (flet ((expression-ok (alist) (every (lambda (term) (rationalp (cdr term))) alist)))
    (and (expression-ok (problem-objective-func problem))
         (every (lambda (entry)
                  (destructuring-bind (lb . ub) (cdr entry)
                    (and (or (null lb) (rationalp lb)) (or (null ub) (rationalp ub)))))
                (problem-var-bounds problem))
         (every (lambda (constraint)
                  (and (expression-ok (second constraint)) (rationalp (third constraint))))
                (problem-constraints problem)))))

(defun exact-declined (what)
  (error 'unsupported-constraint-error :constraint (cons 'exact what) :solver-name "mi355x-simplex"))

(defun pivot-rule-code (pivot-rule)
  "MI_RULE_* of :PIVOT-RULE's value (include/mi355x_simplex.h); any other value is an error."
  (case pivot-rule
    (:dantzig 0)
    (:bland 1)
    (:dantzig-bland 2)
    (t (error "MI355X-SIMPLEX: :pivot-rule must be :dantzig, :bland or :dantzig-bland, not ~S" pivot-rule))))

(defun check-pivot-rule (pivot-rule exact)
  "The argument errors of :PIVOT-RULE: an unknown rule, and a rule other than :DANTZIG without :EXACT T (the
double-float routes keep the reference's rule: in floating point neither of the other two is a theorem)."
  (when (and (plusp (pivot-rule-code pivot-rule)) (not exact))
    (error "MI355X-SIMPLEX: :pivot-rule ~S needs :exact t" pivot-rule)))

(defun upload-exact-tableau (tableau device &optional (max-bits 128) (rule 0))
  "mi355x_xtab_create (MAX-BITS 256: mi355x_xtab_create_wide, a handle whose solves may go on to 256
bits) from the tableau's rational matrix; declines entries beyond (signed-byte 64).  RULE: the handle's
pivot rule (mi355x_xtab_set_pivot_rule), 0 for the reference's."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1)))
    (cffi:with-foreign-objects ((num :int64 (* rows cols)) (den :int64 (* rows cols))
                                (basis :int64 (max 1 (1- rows))) (out :pointer))
      (dotimes (r rows)
        (dotimes (c cols)
          (let ((x (aref matrix r c)))
            (unless (and (typep (numerator x) '(signed-byte 64)) (typep (denominator x) '(signed-byte 64)))
              (exact-declined (list 'coefficient x)))
            (setf (cffi:mem-aref num :int64 (+ (* r cols) c)) (numerator x)
                  (cffi:mem-aref den :int64 (+ (* r cols) c)) (denominator x)))))
      (dotimes (r (1- rows))
        (setf (cffi:mem-aref basis :int64 r) (aref (tableau-basis-columns tableau) r)))
      (let ((status (if (= max-bits 128)
                        (%xtab-create out rows cols num den basis device 0)
                        (%xtab-create-wide out rows cols num den basis device 0 max-bits))))
        (when (= status +mi-exact-overflow+) (exact-declined (list 'overflow max-bits)))
        (check status)
        (let ((handle (cffi:mem-ref out :pointer))
              (done nil))
          (unwind-protect
               (progn (unless (zerop rule) (check (%xtab-set-pivot-rule handle rule)))
                      (setf done t)
                      handle)
            (unless done (%xtab-destroy handle))))))))

(defun download-exact-tableau (handle tableau &optional member (max-bits 128))
  "(/ T D) into the tableau's matrix, T and D rebuilt from their 64-bit limbs (two, or four from a handle
that may be at 256 bits: MAX-BITS 256); the basis.
MEMBER: HANDLE is a batch (mi355x_xbatch_*) and the tableau its member of that index."
  (let* ((matrix (tableau-matrix tableau))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (n-limbs (if (and (null member) (> max-bits 128)) 4 2)))
    (flet ((limbs (ptr k)
             ;; little-endian, two's complement: the top limb carries the sign
             (let ((value (cffi:mem-aref ptr :int64 (+ (* n-limbs k) (1- n-limbs)))))
               (loop for i from (- n-limbs 2) downto 0
                     do (setf value (+ (ash value 64)
                                       (logand (cffi:mem-aref ptr :int64 (+ (* n-limbs k) i)) (1- (ash 1 64))))))
               value)))
      (cffi:with-foreign-objects ((num :int64 (* n-limbs rows cols)) (den :int64 n-limbs)
                                  (basis :int64 (max 1 (1- rows))))
        (check (cond (member (%xbatch-download handle member num den basis))
                     ((= n-limbs 4) (%xtab-download-limbs handle 4 num den basis))
                     (t (%xtab-download handle num den basis))))
        (let ((d (limbs den 0)))
          (dotimes (r rows)
            (dotimes (c cols)
              (setf (aref matrix r c) (/ (limbs num (+ (* r cols) c)) d)))))
        (dotimes (r (1- rows))
          (setf (aref (tableau-basis-columns tableau) r) (cffi:mem-aref basis :int64 r)))
        tableau))))

(defun exact-status (status &optional (max-bits 128))
  "STATUS, or the declined condition that carries the width that was the limit."
  (when (= status +mi-exact-overflow+) (exact-declined (list 'overflow max-bits)))
  status)

(defun solve-exactly (problem device max-pivots &optional (instance-problem problem) (max-bits 128) (rule 0))
  "build-tableau, then n-solve-tableau on exact tableaux in bounded calls; returns the tableau.
INSTANCE-PROBLEM: a branch-and-bound node of PROBLEM (src/simplex.lisp:488-501).  MAX-BITS: 128, or 256
to let the solve start again at 256 bits where 128 overflow.  RULE: the pivot rule of every tableau."
  (let ((tableaus (build-tableau problem instance-problem)))
    (cffi:with-foreign-object (n-pivots :int64 2)
      (if (listp tableaus)
          (destructuring-bind (art-tab main-tab) tableaus
            (let ((art (upload-exact-tableau art-tab device max-bits rule)))
              (unwind-protect
                   (let ((main (upload-exact-tableau main-tab device max-bits rule)))
                     (unwind-protect
                          (let* ((matrix (tableau-matrix art-tab))
                                 (status (solve-in-chunks
                                          (lambda (cap)
                                            (prog1 (exact-status (%xtab-solve-two-phase art main (max-problem-p main-tab)
                                                                                        cap n-pivots)
                                                                 max-bits)
                                              (incf (cffi:mem-aref n-pivots :int64 0) (cffi:mem-aref n-pivots :int64 1))))
                                          (array-dimension matrix 0) (array-dimension matrix 1)
                                          max-pivots n-pivots)))
                            (signal-outcome status)
                            (download-exact-tableau main main-tab nil max-bits))
                       (%xtab-destroy main)))
                (%xtab-destroy art))))
          (let ((handle (upload-exact-tableau tableaus device max-bits rule)))
            (unwind-protect
                 (let ((status (solve-in-chunks
                                (lambda (cap) (exact-status (%xtab-solve handle (max-problem-p tableaus) cap n-pivots)
                                                            max-bits))
                                (1+ (tableau-constraint-count tableaus)) (1+ (tableau-var-count tableaus))
                                max-pivots n-pivots)))
                   (signal-outcome status)
                   (download-exact-tableau handle tableaus nil max-bits))
              (%xtab-destroy handle)))))))

;;; Many exact problems of one shape: one batch of exact tableaux (mi355x_xbatch_*), one workgroup per
;;; member, everything between the phases on the device.  Statuses are per member; a member that needs
;;; more than 128 bits or whose start the library declines gets its condition object, the others
;;; their solved tableau.
(defun upload-exact-batch (tableaus device &optional (rule 0))
  "mi355x_xbatch_create from same-shape tableaus' rational matrices, member after member.  NIL when
the batch cannot take them (an entry beyond (signed-byte 64), a shape whose snapshots do not fit a
workgroup's LDS): the caller then solves the members one by one.  RULE: the batch's pivot rule
(mi355x_xbatch_set_pivot_rule), 0 for the reference's."
  (let* ((n (length tableaus))
         (matrix (tableau-matrix (first tableaus)))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (m (1- rows))
         (size (* n rows cols)))
    (when (notevery (lambda (tab)
                      (let ((mat (tableau-matrix tab)))
                        (dotimes (k (array-total-size mat) t)
                          (let ((x (row-major-aref mat k)))
                            (unless (and (typep (numerator x) '(signed-byte 64))
                                         (typep (denominator x) '(signed-byte 64)))
                              (return nil))))))
                    tableaus)
      (return-from upload-exact-batch nil))
    (let ((num (cffi:foreign-alloc :int64 :count size))
          (den (cffi:foreign-alloc :int64 :count size))
          (basis (cffi:foreign-alloc :int64 :count (max 1 (* n m)))))
      (unwind-protect
           (cffi:with-foreign-object (out :pointer)
             (loop for tab in tableaus for k from 0
                   do (let ((mat (tableau-matrix tab))
                            (base (* k rows cols)))
                        (dotimes (e (* rows cols))
                          (let ((x (row-major-aref mat e)))
                            (setf (cffi:mem-aref num :int64 (+ base e)) (numerator x)
                                  (cffi:mem-aref den :int64 (+ base e)) (denominator x))))
                        (dotimes (r m)
                          (setf (cffi:mem-aref basis :int64 (+ (* k m) r))
                                (aref (tableau-basis-columns tab) r)))))
             (let ((status (%xbatch-create out n rows cols num den basis device 0)))
               (unless (= status +mi-unsupported+)
                 (check status)
                 (let ((handle (cffi:mem-ref out :pointer))
                       (done nil))
                   (unwind-protect
                        (progn (unless (zerop rule) (check (%xbatch-set-pivot-rule handle rule)))
                               (setf done t)
                               handle)
                     (unless done (%xbatch-destroy handle)))))))
        (cffi:foreign-free num)
        (cffi:foreign-free den)
        (cffi:foreign-free basis)))))

(defun exact-member-condition (status)
  "The condition object of a batch member's final status (NIL: it has a solution)."
  (cond
    ((= status +mi-exact-overflow+)
     (make-condition 'unsupported-constraint-error :constraint '(exact overflow 128) :solver-name "mi355x-simplex"))
    ((= status +mi-unsupported+)
     (make-condition 'unsupported-constraint-error :constraint '(exact start) :solver-name "mi355x-simplex"))
    (t (outcome-condition status))))

(defun solve-exact-batch (members device max-pivots &optional solve-wider (rule 0))
  "MEMBERS: build-tableau's results for all-rational problems of ONE shape and sense -- tableaus, or
lists (art main).  One batch (or a pair) of exact tableaux solved side by side in bounded foreign
calls; MAX-PIVOTS (0 = none) caps each member, both phases together.  Returns a list parallel to
MEMBERS: the solved (main) tableau or a condition object, or :DECLINED when the batch cannot take
the group.  SOLVE-WIDER (a function of the member's index, or NIL): what a member that outgrew the
batch's 128 bits gets instead of its condition.  RULE: the pivot rule of both batches."
  (let* ((two-phase (listp (first members)))
         (n (length members))
         (firsts (if two-phase (mapcar #'first members) members))
         (mains (if two-phase (mapcar #'second members) members))
         (matrix (tableau-matrix (first firsts)))
         (is-max (max-problem-p (first mains)))
         (first-handle (upload-exact-batch firsts device rule))
         (main-handle nil))
    (unless first-handle (return-from solve-exact-batch :declined))
    (unwind-protect
         (progn
           (when two-phase
             (setf main-handle (upload-exact-batch mains device rule))
             (unless main-handle (return-from solve-exact-batch :declined)))
           (cffi:with-foreign-objects ((status :int32 n) (pivots :int64 (* 2 n)) (budget :int64 1))
             ;; a call's status for solve-in-chunks: MI_MAX_PIVOTS while some member is left at its cap
             (solve-in-chunks
              (lambda (cap)
                (check (if two-phase
                           (%xbatch-solve-two-phase first-handle main-handle is-max cap status pivots)
                           (%xbatch-solve first-handle is-max cap status pivots)))
                (setf (cffi:mem-aref budget :int64 0) cap)
                (if (loop for k below n thereis (= (cffi:mem-aref status :int32 k) +mi-max-pivots+))
                    +mi-max-pivots+
                    +mi-optimal+))
              (array-dimension matrix 0) (array-dimension matrix 1) max-pivots budget)
             (loop for tab in mains for k from 0
                   collect (cond ((and solve-wider (= (cffi:mem-aref status :int32 k) +mi-exact-overflow+))
                                  (funcall solve-wider k))
                                 ((exact-member-condition (cffi:mem-aref status :int32 k)))
                                 (t (download-exact-tableau (or main-handle first-handle) tab k))))))
      (when main-handle (%xbatch-destroy main-handle))
      (%xbatch-destroy first-handle))))

(defun solve-problems-exactly (problems device max-pivots solve-alone &optional (max-bits 128) (rule 0))
  "The :exact t route of MI355X-SOLVE-PROBLEMS: a vector of results.  (funcall SOLVE-ALONE k problem)
returns member K's result through MI355X-SIMPLEX-SOLVER.  MAX-BITS 256: the batches stay at their 64 / 128
bits, and a member that outgrows them is solved again through SOLVE-ALONE (which allows 256 bits).  RULE: the
pivot rule of every batch (SOLVE-ALONE carries its own)."
  (let ((results (make-array (length problems) :initial-element nil))
        (groups (make-hash-table :test #'equal)))
    (loop for problem in problems for k from 0
          do (if (or (problem-integer-vars problem) (not (rational-numbers-p problem)))
                 (setf (aref results k) (funcall solve-alone k problem))
                 (let ((tableaus (handler-case (build-tableau problem problem)
                                   (error (c) c))))
                   (if (typep tableaus 'condition)
                       (setf (aref results k) tableaus)
                       (let* ((two-phase (listp tableaus))
                              (art (tableau-matrix (if two-phase (first tableaus) tableaus)))
                              (main (if two-phase (second tableaus) tableaus)))
                         (push (cons k tableaus)
                               (gethash (list two-phase (array-dimension art 0) (array-dimension art 1)
                                              (array-dimension (tableau-matrix main) 1) (max-problem-p main))
                                        groups)))))))
    (maphash
     (lambda (shape members)
       (declare (ignore shape))
       (setf members (reverse members))
       (let ((outcomes (if (rest members)
                           (solve-exact-batch (mapcar #'cdr members) device max-pivots
                                              (when (> max-bits 128)
                                                (lambda (q)
                                                  (let ((k (car (nth q members))))
                                                    (funcall solve-alone k (nth k problems)))))
                                              rule)
                           :declined)))
         (if (eq outcomes :declined)
             (loop for (k . nil) in members
                   do (setf (aref results k) (funcall solve-alone k (nth k problems))))
             (loop for (k . nil) in members
                   for outcome in outcomes
                   do (setf (aref results k) outcome)))))
     groups)
    results))

;;; :exact t with :branch-and-bound t: simplex-solver with integer variables (src/simplex.lisp:462-542) on
;;; rationals, where violated-integer-constraint's INTEGERP (:475-480) is meaningful.  The loop below is
;;; the reference's, entry for entry; only WHEN a node LP is solved differs: the top :bb-width unsolved
;;; entries of the stack are solved in one round, grouped by (depth, artificial rows) into batches of
;;; exact tableaux that the library assembles on the device from the base problem's general form and the
;;; entries' rows (mi355x_xbatch_create_nodes), and read back light (mi355x_xbatch_readback).  Every
;;; stack entry is popped sooner or later and a node's result depends on its own rows only, so the
;;; results do not depend on :bb-width.  An entry here is a list of rows (var sense bound), newest
;;; first, sense 0 for <= and 1 for >=.
(defun exact-node-problem (problem entry)
  "PROBLEM with the entry's rows in front of its constraints (src/simplex.lisp:489-500)."
  (let ((node (copy-structure problem)))
    (setf (slot-value node 'linear-programming/problem::constraints)
          (append (mapcar (lambda (row)
                            (destructuring-bind (var sense bound) row
                              (list (if (zerop sense) '<= '>=) (list (cons var 1)) bound)))
                          entry)
                  (problem-constraints problem)))
    node))

(defun exact-mapping-offset (mapping)
  (if (eq (first mapping) 'linear-programming/simplex::signed) 0 (third mapping)))

(defun exact-row-artificial-p (mapping sense bound)
  "Does the node row need an artificial variable?  (a negative bound - offset flips its sense, :243-252)"
  (= 1 (if (minusp (- bound (exact-mapping-offset mapping))) (- 1 sense) sense)))

(defun upload-exact-bb-base (problem main-tab device)
  "mi355x_xbb_base_create from the general form MAIN-TAB (build-tableau's main tableau) of PROBLEM."
  (let* ((matrix (tableau-matrix main-tab))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (vars (coerce (problem-vars problem) 'list))
         (n-vars (length vars))
         (mappings (mapcar (lambda (var) (gethash var (linear-programming/simplex::tableau-var-mapping main-tab))) vars))
         (ncv (loop for mapping in mappings
                    sum (if (eq (first mapping) 'linear-programming/simplex::signed) 2 1)))
         (nb (count-if (lambda (entry) (and (cadr entry) (cddr entry))) (problem-var-bounds problem))))
    (cffi:with-foreign-objects ((num :int64 (* rows cols)) (den :int64 (* rows cols))
                                (basis :int64 (max 1 (1- rows))) (kind :int32 n-vars) (col :int64 n-vars)
                                (off-num :int64 n-vars) (off-den :int64 n-vars) (out :pointer))
      (flet ((int64 (x)
               (unless (typep x '(signed-byte 64)) (exact-declined (list 'coefficient x)))
               x))
        (dotimes (e (* rows cols))
          (let ((x (row-major-aref matrix e)))
            (setf (cffi:mem-aref num :int64 e) (int64 (numerator x))
                  (cffi:mem-aref den :int64 e) (int64 (denominator x)))))
        (dotimes (r (1- rows))
          (setf (cffi:mem-aref basis :int64 r) (aref (tableau-basis-columns main-tab) r)))
        (loop for mapping in mappings for v from 0
              do (let ((offset (exact-mapping-offset mapping)))
                   (setf (cffi:mem-aref kind :int32 v)
                         (position (first mapping) '(linear-programming/simplex::positive
                                                     linear-programming/simplex::negative
                                                     linear-programming/simplex::signed))
                         (cffi:mem-aref col :int64 v) (second mapping)
                         (cffi:mem-aref off-num :int64 v) (int64 (numerator offset))
                         (cffi:mem-aref off-den :int64 v) (int64 (denominator offset))))))
      (let ((status (%xbb-base-create out rows cols num den basis ncv nb n-vars kind col off-num off-den device)))
        (when (= status +mi-exact-overflow+) (exact-declined '(overflow 128)))
        (check status)
        (cffi:mem-ref out :pointer)))))

(defun exact-light-values (problem main-tab ptr basis rows cols)
  "(objective . alist of (var . value)) of one member from mi355x_xbatch_readback's values at PTR -- D, the
right-hand sides, the objective row as limb pairs -- and its basis: tableau-objective-value and
tableau-variable (src/simplex.lisp:74-107) on ratios."
  (flet ((limbs (k)
           (+ (logand (cffi:mem-aref ptr :int64 (* 2 k)) (1- (ash 1 64)))
              (ash (cffi:mem-aref ptr :int64 (1+ (* 2 k))) 64))))
    (let ((d (limbs 0)))
      (flet ((basic (column)
               (let ((idx (loop for r below (1- rows)
                                when (= column (cffi:mem-aref basis :int64 r)) return r)))
                 (if idx (/ (limbs (+ 1 idx)) d) 0))))
        (cons (/ (limbs (+ 1 rows (1- cols))) d)
              (loop for var across (problem-vars problem)
                    collect (let ((mapping (gethash var (linear-programming/simplex::tableau-var-mapping main-tab))))
                              (cons var
                                    (ecase (first mapping)
                                      (linear-programming/simplex::positive
                                       (+ (third mapping) (basic (second mapping))))
                                      (linear-programming/simplex::negative
                                       (- (third mapping) (basic (second mapping))))
                                      (linear-programming/simplex::signed
                                       (- (basic (second mapping)) (basic (1+ (second mapping))))))))))))))

(defun solve-exact-bb-group (problem main-tab base entries n-art max-pivots &optional (rule 0))
  "ENTRIES: nodes of one depth and one number of artificial rows (N-ART, the base's included).  One batch (or
pair) assembled by the library, solved in bounded calls, read back light.  A list parallel to ENTRIES:
(objective . values), :INFEASIBLE, or the condition object of the node's outcome.  RULE: the pivot rule, set on
both batches."
  (let* ((n (length entries))
         (depth (length (first entries)))
         (rows (+ depth (array-dimension (tableau-matrix main-tab) 0)))
         (cols (+ depth (array-dimension (tableau-matrix main-tab) 1)))
         (per (+ 1 rows cols))
         (vars (problem-vars problem))
         (is-max (max-problem-p main-tab))
         (main-handle nil)
         (art-handle nil)
         (values-lo-hi (cffi:foreign-alloc :int64 :count (* 2 n per)))
         (basis (cffi:foreign-alloc :int64 :count (max 1 (* n (1- rows))))))
    (unwind-protect
         (cffi:with-foreign-objects ((var :int64 (* n depth)) (sense :int32 (* n depth)) (bound :int64 (* n depth))
                                     (out-main :pointer) (out-art :pointer) (status :int32 n)
                                     (member-status :int32 n) (pivots :int64 (* 2 n)) (budget :int64 1))
           (loop for entry in entries for q from 0
                 do (loop for (name row-sense row-bound) in entry for k from 0
                          do (unless (typep row-bound '(signed-byte 64)) (exact-declined (list 'bound row-bound)))
                             (setf (cffi:mem-aref var :int64 (+ (* q depth) k)) (position name vars)
                                   (cffi:mem-aref sense :int32 (+ (* q depth) k)) row-sense
                                   (cffi:mem-aref bound :int64 (+ (* q depth) k)) row-bound)))
           (let ((created (%xbatch-create-nodes out-main out-art base n depth var sense bound 0)))
             (when (= created +mi-unsupported+) (exact-declined (list 'batch 'shape rows cols)))
             (check created))
           (setf main-handle (cffi:mem-ref out-main :pointer)
                 art-handle (if (zerop n-art) nil (cffi:mem-ref out-art :pointer)))
           (unless (zerop rule)
             (check (%xbatch-set-pivot-rule main-handle rule))
             (when art-handle (check (%xbatch-set-pivot-rule art-handle rule))))
           (solve-in-chunks
            (lambda (cap)
              (check (if art-handle
                         (%xbatch-solve-two-phase art-handle main-handle is-max cap status pivots)
                         (%xbatch-solve main-handle is-max cap status pivots)))
              (setf (cffi:mem-aref budget :int64 0) cap)
              (if (loop for k below n thereis (= (cffi:mem-aref status :int32 k) +mi-max-pivots+))
                  +mi-max-pivots+
                  +mi-optimal+))
            rows (+ cols n-art) max-pivots budget)
           (check (%xbatch-readback main-handle values-lo-hi basis member-status))
           (loop for q below n
                 collect (let ((st (cffi:mem-aref status :int32 q)))
                           (cond
                             ((= st +mi-infeasible+) :infeasible)
                             ((or (/= st +mi-optimal+) (/= 0 (cffi:mem-aref member-status :int32 q)))
                              (exact-member-condition (if (= st +mi-optimal+) +mi-exact-overflow+ st)))
                             (t (exact-light-values problem main-tab
                                                    (cffi:inc-pointer values-lo-hi (* 16 q per))
                                                    (cffi:inc-pointer basis (* 8 q (1- rows)))
                                                    rows cols))))))
      (when art-handle (%xbatch-destroy art-handle))
      (when main-handle (%xbatch-destroy main-handle))
      (cffi:foreign-free values-lo-hi)
      (cffi:foreign-free basis))))

(defun solve-exact-branch-and-bound (problem device max-pivots bb-width max-nodes &optional (rule 0))
  "simplex-solver (src/simplex.lisp:506-542) on an integer problem whose numbers are all rational.  Returns
the incumbent's solved `tableau` (its node solved once more on its own, so that the reference's methods
serve it), or signals as the reference does.  RULE: the pivot rule of the root, of every node batch and of
that last solve."
  (when (null (problem-constraints problem))
    (exact-declined '(branch-and-bound no-constraints)))       ; (build-tableau's special case has no general form)
  (let* ((tableaus (build-tableau problem problem))
         (main-tab (if (listp tableaus) (second tableaus) tableaus))
         (base-art (count (array-dimension (tableau-matrix main-tab) 1) (tableau-basis-columns main-tab)))
         (base (upload-exact-bb-base problem main-tab device))
         (results (make-hash-table :test #'equal))
         (comparator (if (eq (problem-type problem) 'max) #'< #'>))
         (stack (list '()))
         (processed 0)
         (current-best nil)
         (current-entry nil))
    (flet ((solve-round ()
             ;; the top BB-WIDTH unsolved entries of the stack, in one round
             (let ((groups (make-hash-table :test #'equal)))
               (loop for entry in stack
                     with taken = 0
                     while (< taken bb-width)
                     unless (nth-value 1 (gethash entry results))
                       do (incf taken)
                          (if (null entry)
                              (setf (gethash entry results)
                                    (handler-case
                                        (let ((tab (solve-exactly problem device max-pivots problem 128 rule)))
                                          (cons (tableau-objective-value tab)
                                                (loop for var across (problem-vars problem)
                                                      collect (cons var (tableau-variable tab var)))))
                                      (infeasible-problem-error () :infeasible)))
                              (push entry
                                    (gethash (list (length entry)
                                                   (+ base-art
                                                      (loop for (var sense bound) in entry
                                                            count (exact-row-artificial-p
                                                                   (gethash var (linear-programming/simplex::tableau-var-mapping main-tab))
                                                                   sense bound))))
                                             groups))))
               (maphash (lambda (shape entries)
                          (loop for entry in entries
                                for result in (solve-exact-bb-group problem main-tab base entries (second shape)
                                                                    max-pivots rule)
                                do (setf (gethash entry results) result)))
                        groups)))
           (violated (values-alist)                               ; violated-integer-constraint, :475-480
             (find-if (lambda (var) (not (integerp (cdr (assoc var values-alist)))))
                      (problem-integer-vars problem))))
      (unwind-protect
           (loop while stack
                 do (when (and (plusp max-nodes) (>= processed max-nodes))
                      (error 'mi355x-error :code +mi-max-pivots+ :message "node cap reached"))
                    (unless (nth-value 1 (gethash (first stack) results))
                      (solve-round))
                    (let* ((entry (pop stack))
                           (result (gethash entry results)))
                      (incf processed)
                      (remhash entry results)
                      (cond
                        ((eq result :infeasible))
                        ((typep result 'condition) (error result))
                        (t
                         (destructuring-bind (objective . values-alist) result
                           (let ((split-var (violated values-alist)))
                             (cond
                               ((and split-var current-best (not (funcall comparator current-best objective))))
                               (split-var                          ; gen-entries, :466-473
                                (let ((value (cdr (assoc split-var values-alist))))
                                  (setf stack (list* (cons (list split-var 0 (floor value)) entry)
                                                     (cons (list split-var 1 (ceiling value)) entry)
                                                     stack))))
                               ((or (not current-best) (funcall comparator current-best objective))
                                (setf current-best objective
                                      current-entry entry)))))))))
        (%xbb-base-destroy base))
      (if current-best
          (solve-exactly problem device max-pivots (exact-node-problem problem current-entry) 128 rule)
          (error 'infeasible-problem-error)))))

;;; ------------------------------------------------------------------ the native route
;;; SURVEY 8(f) rows 2-3: at 8192 x 4096 the reference's build-tableau conses a boxed 4097 x 12289
;;; (simple-array real 2) -- 5e7 boxed entries -- and the build-tableau route then coerces every one
;;; of them.  Here the parsed problem itself crosses the C ABI: one foreign call per constraint with
;;; its coefficients in two specialised vectors, the tableau is assembled by the library's host
;;; threads straight into pinned staging buffers (csrc/host_problem.cpp), and what comes back is a
;;; handle to (objective row, RHS column, basis, var-mapping).
(defclass mi355x-solution ()
  ((problem :initarg :problem :reader mi355x-solution-problem
            :documentation "The problem instance the solution answers (solution-problem).")
   (handle :initarg :handle :accessor mi355x-solution-handle
           :documentation "mi355x_solution*; a null pointer once FREE-SOLUTION has run.")
   (var-index :initarg :var-index :reader mi355x-solution-var-index
              :documentation "eq hash table: variable symbol -> its index in problem-vars, the
name the C ABI knows the variable by."))
  (:documentation "What MI355X-SIMPLEX-SOLVER returns on the native route: the light solution
object of the library behind the four solution-* generics (src/solver.lisp:59-80).  Holds
O(rows + cols) doubles on the C side; released by the garbage collector's finalizer (SBCL) or
explicitly by FREE-SOLUTION."))

(defun make-solution (problem handle var-index)
  (let ((solution (make-instance 'mi355x-solution :problem problem :handle handle
                                                  :var-index var-index)))
    ;; the finalizer must not close over SOLUTION itself (it would never become garbage)
    #+sbcl (sb-ext:finalize solution (lambda () (%solution-destroy handle)) :dont-save t)
    solution))

(defun free-solution (solution)
  "Releases the C side of SOLUTION now instead of at some later garbage collection.  Idempotent;
the solution answers no generic afterwards."
  (let ((handle (mi355x-solution-handle solution)))
    (unless (cffi:null-pointer-p handle)
      #+sbcl (sb-ext:cancel-finalization solution)
      (setf (mi355x-solution-handle solution) (cffi:null-pointer))
      (%solution-destroy handle)))
  nil)

(defun live-handle (solution)
  (let ((handle (mi355x-solution-handle solution)))
    (when (cffi:null-pointer-p handle)
      (error "~S has been released with free-solution" solution))
    handle))

(defun solution-var-index (solution variable)
  "Index of VARIABLE in problem-vars, or the reference's error for a stranger
(src/simplex.lisp:85-86, 115-116)."
  (or (gethash variable (mi355x-solution-var-index solution))
      (error "~S is not a variable in the tableau" variable)))

(defmethod solution-problem ((solution mi355x-solution))          ; src/solver.lisp:59-62
  (mi355x-solution-problem solution))

(defmethod solution-objective-value ((solution mi355x-solution))  ; src/solver.lisp:64-67, simplex.lisp:74-78
  (cffi:with-foreign-object (out :double)
    (check (%solution-objective-value (live-handle solution) out))
    (cffi:mem-ref out :double)))

(defmethod solution-variable ((solution mi355x-solution) variable) ; src/solver.lisp:69-72, simplex.lisp:81-107
  (if (eq variable (problem-objective-var (mi355x-solution-problem solution)))
      (solution-objective-value solution)
      (let ((index (solution-var-index solution variable)))
        (cffi:with-foreign-object (out :double)
          (check (%solution-variable (live-handle solution) index out))
          (cffi:mem-ref out :double)))))

(defmethod solution-reduced-cost ((solution mi355x-solution) variable) ; src/solver.lisp:74-80, simplex.lisp:111-120
  (let ((index (solution-var-index solution variable)))
    (cffi:with-foreign-object (out :double)
      (let ((status (%solution-reduced-cost (live-handle solution) index out)))
        ;; MI_BAD_ARG with a valid index: the variable's mapping is not `positive`
        (when (= status -1)
          (error "~S has no lower bound" variable))                 ; src/simplex.lisp:117-118
        (check status)
        (cffi:mem-ref out :double)))))

(defun solution-pivots (solution)
  "(values phase-1-pivots phase-2-pivots) the solve took (drive-out pivots count as phase 1)."
  (cffi:with-foreign-objects ((p1 :int64) (p2 :int64))
    (check (%solution-pivots (live-handle solution) p1 p2))
    (values (cffi:mem-ref p1 :int64) (cffi:mem-ref p2 :int64))))

(defun call-with-linear-expression (alist var-index fn)
  "ALIST: a linear expression ((var . coef) ...) as the parser leaves it (src/problem.lisp:45-53).
Calls FN with pointers to its variable indices (int64) and coefficients (double) and their count;
the vectors are pinned for the length of the call only (the library copies)."
  (let* ((nnz (length alist))
         (vars (make-array (max nnz 1) :element-type '(signed-byte 64) :initial-element 0))
         (coefs (make-array (max nnz 1) :element-type 'double-float :initial-element 0d0)))
    (loop for (var . coef) in alist for k from 0
          do (setf (aref vars k) (or (gethash var var-index)
                                     (error "~S is not a variable of the problem" var))
                   (aref coefs k) (coerce coef 'double-float)))
    (cffi:with-pointer-to-vector-data (pv vars)
      (cffi:with-pointer-to-vector-data (pc coefs)
        (funcall fn pv pc nnz)))))

(defun marshal-problem (problem)
  "PROBLEM (src/problem.lisp:45-53) -> (values mi355x_problem* var-index): variables named by
their index in problem-vars, every number coerced to double-float.  The caller destroys the
handle (mi355x_problem_destroy)."
  (let* ((vars (problem-vars problem))
         (var-index (make-hash-table :test #'eq :size (max 1 (length vars)))))
    (loop for var across vars for i from 0 do (setf (gethash var var-index) i))
    (cffi:with-foreign-object (out :pointer)
      (check (%problem-create out (if (eq 'max (problem-type problem)) 1 0) (length vars)))
      (let ((handle (cffi:mem-ref out :pointer))
            (complete nil))
        (unwind-protect
             (progn
               (call-with-linear-expression
                (problem-objective-func problem) var-index
                (lambda (pv pc nnz) (check (%problem-set-objective handle pv pc nnz))))
               ;; (var . (lb . ub)), NIL = unbounded on that side; a variable without an entry
               ;; is >= 0 (src/simplex.lisp:189-212)
               (loop for (var . (lb . ub)) in (problem-var-bounds problem)
                     do (check (%problem-set-bounds
                                handle (or (gethash var var-index)
                                           (error "~S is not a variable of the problem" var))
                                (if lb 1 0) (if lb (coerce lb 'double-float) 0d0)
                                (if ub 1 0) (if ub (coerce ub 'double-float) 0d0))))
               (dolist (var (problem-integer-vars problem))
                 (check (%problem-set-integer handle (gethash var var-index))))
               ;; (op alist rhs), op one of <= >= = (src/problem.lisp:45-53)
               (loop for (op expression rhs) in (problem-constraints problem)
                     do (call-with-linear-expression
                         expression var-index
                         (lambda (pv pc nnz)
                           (check (%problem-add-constraint handle (ecase op (<= 0) (>= 1) (= 2))
                                                           pv pc nnz (coerce rhs 'double-float))))))
               (setf complete t)
               (values handle var-index))
          (unless complete (%problem-destroy handle)))))))

(defun native-var-mapping (problem variable)
  "The var-mapping entry the library's build-tableau gives VARIABLE, in the reference's form
(src/simplex.lisp:44-46): (positive col offset), (negative col offset) or (signed col) -- with the
reference's OWN symbols (internal to linear-programming/simplex, src/simplex.lisp:197-210), so that an
entry compares EQUAL with what (gethash variable (tableau-var-mapping tableau)) holds there."
  (multiple-value-bind (handle var-index) (marshal-problem problem)
    (unwind-protect
         (cffi:with-foreign-objects ((kind :int) (col :int64) (offset :double))
           (check (%var-mapping handle (or (gethash variable var-index)
                                           (error "~S is not a variable of the problem" variable))
                                kind col offset))
           (ecase (cffi:mem-ref kind :int)
             (0 (list 'linear-programming/simplex::positive (cffi:mem-ref col :int64) (cffi:mem-ref offset :double)))
             (1 (list 'linear-programming/simplex::negative (cffi:mem-ref col :int64) (cffi:mem-ref offset :double)))
             (2 (list 'linear-programming/simplex::signed (cffi:mem-ref col :int64)))))
      (%problem-destroy handle))))

(defun native-number-p (x)
  "Numbers the library's double-float build-tableau treats exactly as the reference's generic
arithmetic followed by the glue's coerce would: double-floats, and integers a double holds
exactly.  (A ratio or a single-float is combined in its own type first by the reference --
rhs - coef * lb at src/simplex.lisp:235-238 -- and rounded to double afterwards.)"
  (or (typep x 'double-float)
      (and (integerp x) (<= (abs x) (expt 2 53)))))

(defun native-numbers-p (problem)
  (flet ((expression-ok (alist) (every (lambda (term) (native-number-p (cdr term))) alist)))
    (and (expression-ok (problem-objective-func problem))
         (every (lambda (entry)
                  (destructuring-bind (lb . ub) (cdr entry)
                    (and (or (null lb) (native-number-p lb)) (or (null ub) (native-number-p ub)))))
                (problem-var-bounds problem))
         (every (lambda (constraint)
                  (and (expression-ok (second constraint)) (native-number-p (third constraint))))
                (problem-constraints problem)))))

(defun solve-natively (problem factor device max-pivots)
  "simplex-solver for an LP (src/simplex.lisp:506-542 without branch-and-bound) entirely behind
the C ABI: marshal, mi355x_simplex_solver_begin (build-tableau + upload), ..._step in bounded
chunks (never an unbounded foreign call; the phases of a two-phase problem included), ..._finish.
Returns a MI355X-SOLUTION or signals the reference's conditions."
  (multiple-value-bind (problem-handle var-index) (marshal-problem problem)
    (unwind-protect
         (cffi:with-foreign-objects ((out :pointer) (n-pivots :int64))
           (let ((status (with-foreign-fp-mode (%solver-begin problem-handle factor device out))))
             ;; the no-constraint special case decides unboundedness while building
             ;; (src/simplex.lisp:170, 174)
             (when (= status +mi-unbounded+) (error 'unbounded-problem-error))
             (check status))
           (let ((job (cffi:mem-ref out :pointer))
                 (consumed nil)
                 (rows (1+ (length (problem-constraints problem)))))
             (unwind-protect
                  (let ((status (solve-in-chunks
                                 (lambda (cap) (%solver-step job cap n-pivots))
                                 rows (+ rows (length (problem-vars problem))) max-pivots n-pivots)))
                    (signal-outcome status)
                    (setf consumed t)                ; finish consumes the job whatever it returns
                    (check (%solver-finish job out))
                    (make-solution problem (cffi:mem-ref out :pointer) var-index))
               (unless consumed (%solver-abandon job)))))
      (%problem-destroy problem-handle))))

(defun solve-branch-and-bound (problem factor int-tolerance width devices max-nodes)
  "simplex-solver with integer variables (src/simplex.lisp:462-542) behind the C ABI: marshal,
mi355x_simplex_solver_bb_begin with problem-integer-vars IN ORDER (the order decides which variable
is branched on), ..._bb_step in bounded chunks of nodes (never an unbounded foreign call),
..._bb_finish (the incumbent).  The search is the reference's node for node; up to WIDTH node LPs
are solved side by side.  Returns a MI355X-SOLUTION or signals the reference's conditions."
  (multiple-value-bind (problem-handle var-index) (marshal-problem problem)
    (unwind-protect
         (let* ((int-vars (problem-integer-vars problem))
                (n-int (length int-vars))
                (n-dev (device-count-of devices)))
           (cffi:with-foreign-objects ((order :int64 (max n-int 1)) (ids :int (max n-dev 1))
                                       (out :pointer) (n-nodes :int64))
             (loop for var in int-vars for k from 0
                   do (setf (cffi:mem-aref order :int64 k) (gethash var var-index)))
             (when (listp devices)
               (loop for d in devices for i from 0 do (setf (cffi:mem-aref ids :int i) d)))
             (check (with-foreign-fp-mode
                      (%bb-begin problem-handle order n-int factor (coerce int-tolerance 'double-float)
                                 width n-dev (if (listp devices) ids (cffi:null-pointer)) out)))
             (let ((job (cffi:mem-ref out :pointer))
                   (consumed nil)
                   (done 0))
               (unwind-protect
                    (let ((status
                            (loop
                              (let* ((cap (if (plusp max-nodes) (min 256 (- max-nodes done)) 256))
                                     (rc (check (with-foreign-fp-mode (%bb-step job cap n-nodes)))))
                                (incf done (cffi:mem-ref n-nodes :int64))
                                (when (or (/= rc +mi-max-pivots+)
                                          (and (plusp max-nodes) (>= done max-nodes)))
                                  (return rc))))))
                      (when (= status +mi-max-pivots+)
                        (error 'mi355x-error :code status :message "node cap reached"))
                      (signal-outcome status)
                      (setf consumed t)              ; finish consumes the job whatever it returns
                      (check (%bb-finish job out))
                      (make-solution problem (cffi:mem-ref out :pointer) var-index))
                 (unless consumed (%bb-abandon job))))))
      (%problem-destroy problem-handle))))

(defun solve-problems-natively (problems factor devices max-pivots)
  "A LIST of problems entirely behind the C ABI: every problem marshalled (mi355x_problem_*), ONE job of
the library for the list (mi355x_simplex_solver_many_begin groups the members by tableau shape and
sense into multi-device batches; two-phase members as pairs of batches with the step between the
phases on the devices), stepped in bounded foreign calls, the light solutions read back.  Returns a
list parallel to PROBLEMS: a MI355X-SOLUTION, or the condition object the one-problem hook would
signal for that member.  No boxed tableau exists for any member (BASELINE config 4 from Lisp: 1 024
build-tableau results would be 2e8 boxed entries)."
  (let* ((n (length problems))
         (marshalled '())                ; (handle var-index) per problem, filled INSIDE the unwind-protect: a
         (n-dev (device-count-of devices))   ; marshalling error midway must not leak the handles made so far
         (rows (1+ (reduce #'max problems :key (lambda (p) (length (problem-constraints p))))))
         (cols (+ rows (reduce #'max problems :key (lambda (p) (length (problem-vars p))))))
         (chunk (chunk-pivots rows cols)))
    (unwind-protect
         (cffi:with-foreign-objects ((handles :pointer n) (ids :int (max n-dev 1)) (out :pointer)
                                     (status :int32 n) (solutions :pointer n))
           (dolist (problem problems)
             (push (multiple-value-list (marshal-problem problem)) marshalled))
           (setf marshalled (nreverse marshalled))
           (loop for (handle nil) in marshalled for k from 0
                 do (setf (cffi:mem-aref handles :pointer k) handle))
           (when (listp devices)
             (loop for d in devices for i from 0 do (setf (cffi:mem-aref ids :int i) d)))
           (check (with-foreign-fp-mode
                    (%solver-many-begin handles n factor n-dev
                                        (if (listp devices) ids (cffi:null-pointer)) out)))
           (let ((job (cffi:mem-ref out :pointer))
                 (consumed nil)
                 (done 0))
             (unwind-protect
                  (progn
                    (loop
                      (let* ((cap (if (plusp max-pivots) (min chunk (- max-pivots done)) chunk))
                             (rc (check (with-foreign-fp-mode (%solver-many-step job cap status)))))
                        (incf done cap)
                        (when (or (/= rc +mi-max-pivots+)
                                  (and (plusp max-pivots) (>= done max-pivots)))
                          (return))))
                    (setf consumed t)                ; finish consumes the job whatever it returns
                    (check (%solver-many-finish job status solutions))
                    (loop for problem in problems
                          for (nil var-index) in marshalled
                          for k from 0
                          collect (let ((st (cffi:mem-aref status :int32 k)))
                                    (cond
                                      ((= st +mi-optimal+)
                                       (make-solution problem (cffi:mem-aref solutions :pointer k) var-index))
                                      ((= st -6)                         ; MI_UNSUPPORTED: integer variables
                                       (make-condition 'unsupported-constraint-error
                                                       :constraint (cons 'integer (problem-integer-vars problem))
                                                       :solver-name "mi355x-simplex"))
                                      ((= st +mi-running+) (outcome-condition +mi-max-pivots+))
                                      ;; a member whose unit FAILED (device error, out of memory ...: the
                                      ;; other units went on) carries that negative code
                                      ((minusp st)
                                       (make-condition 'mi355x-error :code st
                                                                     :message (format nil "member ~D failed" k)))
                                      (t (outcome-condition st))))))
               (unless consumed (%solver-many-abandon job)))))
      (loop for (handle nil) in marshalled do (%problem-destroy handle)))))

;;; ------------------------------------------------------------------ the *solver* value
(defun solve-two-phase-in-chunks (art-handle main-handle rows cols main-is-max factor max-pivots
                                  n-pivots)
  "n-solve-tableau's two-phase branch (src/simplex.lisp:402-452) without an unbounded foreign call:
phase 1 in chunks on the artificial tableau, the step between the phases
(mi355x_two_phase_handover: feasibility test, drive-out pivots, hand-over -- bounded by the row
count), phase 2 in chunks on the main tableau.  Same pivots, same bits as mi355x_solve_two_phase.
ROWS x COLS: the artificial tableau's shape (chunk size).  MAX-PIVOTS (0 = none) caps the two
phases together.  Returns the final status."
  (let* ((used 0)
         (status (solve-in-chunks (lambda (cap) (%tab-solve art-handle 0 factor cap n-pivots))
                                  rows cols max-pivots n-pivots)))
    (incf used (cffi:mem-aref n-pivots :int64 0))
    (cond
      ((/= status +mi-optimal+) status)
      (t
       (setf status (check (with-foreign-fp-mode
                             (%two-phase-handover art-handle main-handle factor n-pivots))))
       (incf used (cffi:mem-aref n-pivots :int64 0))
       (cond
         ((/= status +mi-optimal+) status)         ; MI_INFEASIBLE / MI_ART_NONZERO / MI_ART_STUCK
         ((and (plusp max-pivots) (>= used max-pivots)) +mi-max-pivots+)
         (t (solve-in-chunks (lambda (cap) (%tab-solve main-handle main-is-max factor cap n-pivots))
                             rows cols (if (plusp max-pivots) (- max-pivots used) 0)
                             n-pivots)))))))

(defun mi355x-simplex-solver (problem &rest args
                              &key (fp-tolerance 1024) (device 0) (devices 1) (max-pivots 0)
                                full-tableau (native :auto) branch-and-bound (bb-width 1)
                                (int-tolerance 0) (max-nodes 0) exact (exact-max-bits 128)
                                (pivot-rule :dantzig) (precision :double)
                              &allow-other-keys)
  "Solver interface function for the MI355X backend (the value of
linear-programming:*solver*, src/solver.lisp:39-49).  Takes a problem and backend keyword
arguments -- :fp-tolerance (as the built-in solver, src/simplex.lisp:506-511), :device,
:devices (a count > 1 or a list of device ids: the tableau -- for a two-phase problem the
artificial tableau, with phase 1, the hand-over and phase 2 all on the partition -- is
column-partitioned over those GPUs of the node), :max-pivots, :full-tableau (return a `tableau`
with every entry of the solved tableau written back), :native (:auto, the default: the native
route whenever the problem's numbers are double-floats / integers and neither :full-tableau nor
:devices asks for the tableau itself; T: the native route also for ratios and single-floats, which
are then rounded to double BEFORE build-tableau's arithmetic instead of after; NIL: always the
build-tableau route) -- and returns a solution object answering solution-problem,
solution-objective-value, solution-variable and solution-reduced-cost (src/solver.lisp:40-45): a
MI355X-SOLUTION on the native route, a solved `tableau` otherwise.  solve-problem forwards these
keywords (src/solver.lisp:53-56):
  (solve-problem problem :devices 8)        (solve-problem problem :devices '(4 5 6 7))
:branch-and-bound T (opt-in; without it integer problems are declined as before) solves an integer
problem with the reference's branch-and-bound (src/simplex.lisp:462-542), node for node, in the
library: :bb-width node LPs side by side (default 1; results do not depend on it), :int-tolerance
(0, the default: a value is integral iff it is an integer-valued double; > 0: within that many
double-float-epsilons of an integer), :max-nodes (0 = no cap).
:exact T (opt-in) solves a problem whose numbers are all rational with the reference's rational
semantics (src/utils.lisp:84-124) on exact integer tableaux and returns the solved `tableau`, its
matrix holding the exact ratios; any float in the problem means the double-float routes above,
unchanged.  :exact-max-bits (128, the default, or 256; opt-in) is the widest integer the exact tableaux
may grow to: with 256 a solve that outgrows 128 bits starts again at 256 bits instead of being declined,
and the declined condition past those is (exact overflow 256).
:exact T together with :branch-and-bound T, on a problem with integer variables whose numbers are all
rational: the reference's branch-and-bound in rational arithmetic, where its integrality test is INTEGERP
of a ratio (src/simplex.lisp:475-480); :bb-width node LPs per round as batches of exact tableaux assembled
on the device, :max-nodes as above; returns the incumbent's solved `tableau`.  (Without integer variables
the combination is declined; with a float anywhere it is the double-float branch-and-bound above.  Exact
branch-and-bound rides on batches, which stop at 128 bits: with :exact-max-bits 256 it is an error.)
:pivot-rule (opt-in, with :exact T only) is how the exact solves choose a pivot.  :dantzig, the default, is
find-entering-column and find-pivoting-row (src/simplex.lisp:362-389) as they stand: no anti-cycling rule, and
on rationals a cycle never ends.  :bland takes the lowest eligible column and, among the rows of the minimum
ratio, the one whose basis column is lowest; :dantzig-bland does so only after a degenerate pivot and until
the next one that is not.  Both end on every input; they reach the exact branch-and-bound's root and node
batches too.  An unknown rule, and a rule other than :dantzig without :exact T, are errors; with :exact T on a
problem that holds a float such a rule is declined: unsupported-constraint-error (exact pivot-rule RULE).
:precision :single (opt-in; :double, the default, is everything above, unchanged) is the reference's
single-float path: what the reader makes of 0.5 is a SINGLE-FLOAT, and the reference then solves in single-float
arithmetic with single-float-epsilon thresholds (src/utils.lisp:84-124).  The reference's build-tableau builds
the tableau, whose entries must all be single-floats or integers of at most 2^24 in magnitude -- anything else is
declined, never rounded: unsupported-constraint-error (single ENTRY) --, the library solves it in IEEE binary32,
and the solved `tableau` comes back with every entry a single-float.  Together with :exact, :branch-and-bound,
more than one of :devices, :native T, :full-tableau or a :pivot-rule other than :dantzig it is an error, as is
an unknown value."
  (declare (ignore args))
  (check-pivot-rule pivot-rule exact)
  (check-precision precision exact branch-and-bound devices native full-tableau pivot-rule)
  (when (eq precision :single)
    (return-from mi355x-simplex-solver
      (solve-in-single-precision problem fp-tolerance device max-pivots)))
  (when (and (plusp (pivot-rule-code pivot-rule)) (not (rational-numbers-p problem)))
    (exact-declined (list 'pivot-rule pivot-rule)))
  (unless (member exact-max-bits '(128 256))
    (error "MI355X-SIMPLEX-SOLVER: :exact-max-bits must be 128 or 256, not ~S" exact-max-bits))
  (when (and exact branch-and-bound (/= exact-max-bits 128))
    (error "MI355X-SIMPLEX-SOLVER: :exact t :branch-and-bound t does not take :exact-max-bits ~S" exact-max-bits))
  (when (and exact branch-and-bound)
    (unless (problem-integer-vars problem)
      (exact-declined '(branch-and-bound)))
    (when (rational-numbers-p problem)
      (return-from mi355x-simplex-solver
        (solve-exact-branch-and-bound problem device max-pivots bb-width max-nodes
                                      (pivot-rule-code pivot-rule)))))
  ;; :branch-and-bound T (opt-in): integer problems through the library's branch-and-bound job
  ;; (:bb-width node LPs side by side, :int-tolerance 0 = exact integrality, :max-nodes 0 = no cap)
  (when (and branch-and-bound (problem-integer-vars problem))
    (return-from mi355x-simplex-solver
      (solve-branch-and-bound problem (coerce fp-tolerance 'double-float) int-tolerance bb-width devices
                              max-nodes)))
  ;; :exact T (opt-in): all-rational problems on exact tableaux (integer problems are declined below)
  (when (and exact (null (problem-integer-vars problem)) (rational-numbers-p problem))
    (return-from mi355x-simplex-solver
      (solve-exactly problem device max-pivots problem exact-max-bits (pivot-rule-code pivot-rule))))
  (when (problem-integer-vars problem)
    (error 'unsupported-constraint-error
           :constraint (cons 'integer (problem-integer-vars problem))
           :solver-name "mi355x-simplex"))
  (when (and native (not full-tableau) (<= (device-count-of devices) 1)
             (plusp (length (problem-vars problem)))
             (or (eq native t) (native-numbers-p problem)))
    (return-from mi355x-simplex-solver
      (solve-natively problem (coerce fp-tolerance 'double-float) device max-pivots)))
  (let ((tableaus (build-tableau problem problem :fp-tolerance-factor fp-tolerance))
        (factor (coerce fp-tolerance 'double-float)))
    (cffi:with-foreign-object (n-pivots :int64 2)
      (if (listp tableaus)
          ;; two-phase: (art-tableau main-tableau), src/simplex.lisp:326-328, 402-452
          (destructuring-bind (art-tab main-tab) tableaus
           (if (and (> (device-count-of devices) 1)
                    (not (member (solve-two-phase-column-partitioned art-tab main-tab devices factor
                                                                     full-tableau n-pivots)
                                 '(:unsupported :overflowed))))
               main-tab
            (multiple-value-bind (art-handle art-flat art-basis) (upload-tableau art-tab device)
              (declare (ignorable art-flat art-basis))
              (unwind-protect
                   (multiple-value-bind (main-handle main-flat main-basis)
                       (upload-tableau main-tab device)
                     (unwind-protect
                          (let ((status (solve-two-phase-in-chunks
                                         art-handle main-handle
                                         (array-dimension (tableau-matrix art-tab) 0)
                                         (array-dimension (tableau-matrix art-tab) 1)
                                         (max-problem-p main-tab) factor max-pivots n-pivots)))
                            (signal-outcome status)
                            (if full-tableau
                                (download-tableau main-handle main-tab main-flat main-basis)
                                (download-solution main-handle main-tab main-basis)))
                       (%tab-destroy main-handle)))
                (%tab-destroy art-handle)))))
          ;; single phase, src/simplex.lisp:453-461
          (if (and (> (device-count-of devices) 1)
                   (not (eq :overflowed
                            (solve-column-partitioned tableaus devices factor max-pivots
                                                      full-tableau n-pivots))))
              tableaus
              ;; one device.  With the light read-back (the default) only [non-basic columns | RHS]
              ;; is coerced and uploaded (mi355x_tab_create_compact); :full-tableau, or a basis that
              ;; is not a set of exact unit columns, takes the dense upload.
              (multiple-value-bind (compact-handle compact-basis)
                  (if full-tableau (values nil nil) (upload-tableau-compact tableaus device))
                (if compact-handle
                    (unwind-protect
                         (let ((status (solve-in-chunks
                                        (lambda (cap) (%tab-solve compact-handle (max-problem-p tableaus)
                                                                  factor cap n-pivots))
                                        (1+ (tableau-constraint-count tableaus))
                                        (1+ (tableau-var-count tableaus)) max-pivots n-pivots)))
                           (signal-outcome status)
                           (download-solution compact-handle tableaus compact-basis))
                      (%tab-destroy compact-handle))
                    (multiple-value-bind (handle flat basis) (upload-tableau tableaus device)
                      (unwind-protect
                           (let ((status (solve-in-chunks
                                          (lambda (cap) (%tab-solve handle (max-problem-p tableaus) factor
                                                                    cap n-pivots))
                                          (1+ (tableau-constraint-count tableaus))
                                          (1+ (tableau-var-count tableaus)) max-pivots n-pivots)))
                             (signal-outcome status)
                             (if full-tableau
                                 (download-tableau handle tableaus flat basis)
                                 (download-solution handle tableaus basis)))
                        (%tab-destroy handle))))))))))

;;; ------------------------------------------------------------------ many problems at once
;;; The hook takes ONE problem per call (src/solver.lisp:53-56), so N calls of solve-problem solve
;;; N small LPs one after the other -- each alone cannot fill the GPU (a 512 x 256 LP occupies 8 of
;;; 256 CUs).  BASELINE config 4 is exactly that workload; the library solves such LPs side by
;;; side (mi355x_multibatch_*: every LP resident in the register files of a few CUs, all LPs of a
;;; sub-batch in one launch, one sub-batch per GPU, no communication).  This is its Lisp entry:
;;; a LIST of problems in, a list of solved tableaus out, each answering the four solution-*
;;; generics exactly as the tableau (solve-problem p) returns.
(defun outcome-condition (status)
  "The condition SIGNAL-OUTCOME would signal for STATUS, as an object (NIL for MI_OPTIMAL)."
  (handler-case (progn (signal-outcome status) nil)
    (error (c) c)))

(defun pack-tableaus (tableaus)
  "Same-shape tableaus -> (values flat bases rows cols): the matrices coerced to double-float one
after the other, the bases as (signed-byte 64)."
  (let* ((n (length tableaus))
         (first-matrix (tableau-matrix (first tableaus)))
         (rows (array-dimension first-matrix 0))
         (cols (array-dimension first-matrix 1))
         (m (1- rows))
         (flat (make-array (* n rows cols) :element-type 'double-float))
         (bases (make-array (max 1 (* n m)) :element-type '(signed-byte 64) :initial-element 0)))
    (loop for tab in tableaus for k from 0
          do (let ((matrix (tableau-matrix tab))
                   (basis (tableau-basis-columns tab))
                   (base (* k rows cols)))
               (dotimes (r rows)
                 (dotimes (c cols)
                   (setf (aref flat (+ base (* r cols) c))
                         (coerce (aref matrix r c) 'double-float))))
               (dotimes (i m)
                 (setf (aref bases (+ (* k m) i)) (aref basis i)))))
    (values flat bases rows cols)))

(defun multibatch-create (tableaus devices)
  "mi355x_multibatch_create over DEVICES (a count or a list of ids): LP k lives in sub-batch
k / ceil(n / devices)."
  (multiple-value-bind (flat bases rows cols) (pack-tableaus tableaus)
    (let ((n-dev (device-count-of devices)))
      (cffi:with-foreign-objects ((out :pointer) (ids :int (max n-dev 1)))
        (when (listp devices)
          (loop for d in devices for i from 0 do (setf (cffi:mem-aref ids :int i) d)))
        (cffi:with-pointer-to-vector-data (pm flat)
          (cffi:with-pointer-to-vector-data (pb bases)
            (check (with-foreign-fp-mode
                     (%multibatch-create out (length tableaus) rows cols pm pb n-dev
                                         (if (listp devices) ids (cffi:null-pointer)))))))
        (cffi:mem-ref out :pointer)))))

(defun multibatch-read-back (handle k tab full-tableau)
  "Member K of a batch into TAB's own arrays: every entry, or (default) the objective row, the RHS
column and the basis -- all that tableau-variable & co. read (src/simplex.lisp:74-120)."
  (let* ((matrix (tableau-matrix tab))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (last-row (make-array cols :element-type 'double-float))
         (last-col (make-array rows :element-type 'double-float))
         (flat (when full-tableau (make-array (* rows cols) :element-type 'double-float)))
         (basis (make-array (max 1 (1- rows)) :element-type '(signed-byte 64) :initial-element 0))
         (basis-dst (tableau-basis-columns tab)))
    (cffi:with-pointer-to-vector-data (pr last-row)
      (cffi:with-pointer-to-vector-data (pc last-col)
        (cffi:with-pointer-to-vector-data (pb basis)
          (if full-tableau
              (cffi:with-pointer-to-vector-data (pm flat)
                (check (%multibatch-download handle k pm pb pr pc)))
              (check (%multibatch-download handle k (cffi:null-pointer) pb pr pc))))))
    (if full-tableau
        (vectors->tableau tab flat basis)
        (progn
          (dotimes (r rows) (setf (aref matrix r (1- cols)) (aref last-col r)))
          (dotimes (c cols) (setf (aref matrix (1- rows) c) (aref last-row c)))
          (dotimes (i (length basis-dst)) (setf (aref basis-dst i) (aref basis i)))
          tab))))

(defun multibatch-solve-in-chunks (handle is-max factor rows cols max-pivots n status pivots)
  "mi355x_multibatch_solve in bounded foreign calls, as for a single tableau: members a chunk left
at MI_MAX_PIVOTS carry on in the next call (finished ones re-price as optimal at once).  STATUS
(int32 x N) holds the members' statuses afterwards.  Returns the pivot budget used (chunk caps)."
  (let ((chunk (chunk-pivots rows cols))
        (done 0))
    (loop
      (let ((cap (if (plusp max-pivots) (min chunk (- max-pivots done)) chunk)))
        (check (with-foreign-fp-mode
                 (%multibatch-solve handle is-max factor cap status pivots)))
        (incf done cap)
        (when (or (and (plusp max-pivots) (>= done max-pivots))
                  (loop for k below n
                        never (= (cffi:mem-aref status :int32 k) +mi-max-pivots+)))
          (return done))))))

(defun solve-two-phase-batch (pairs devices factor max-pivots full-tableau)
  "PAIRS: lists (art-tableau main-tableau) of ONE shape each and one sense (build-tableau's results
for two-phase problems, src/simplex.lisp:326-328).  Phase 1 on the batch of artificial tableaux in
bounded calls, the step between the phases per member on the devices
(mi355x_multibatch_two_phase_handover: feasibility test, drive-out pivots, hand-over;
src/simplex.lisp:405-451), phase 2 on the batch of main tableaux in bounded calls.  MAX-PIVOTS (0 =
none) caps each phase.  Returns a list parallel to PAIRS: the solved main tableau or a condition
object."
  (let* ((n (length pairs))
         (art-matrix (tableau-matrix (first (first pairs))))
         (rows (array-dimension art-matrix 0))
         (cols (array-dimension art-matrix 1))
         (art-handle (multibatch-create (mapcar #'first pairs) devices))
         (main-handle nil))
    (unwind-protect
         (progn
           (setf main-handle (multibatch-create (mapcar #'second pairs) devices))
           (cffi:with-foreign-objects ((status1 :int32 n) (between :int32 n) (status2 :int32 n)
                                       (pivots :int64 n))
             (multibatch-solve-in-chunks art-handle 0 factor rows cols max-pivots n status1 pivots)
             (check (with-foreign-fp-mode
                      (%multibatch-two-phase-handover art-handle main-handle factor status1 between
                                                      (cffi:null-pointer))))
             (multibatch-solve-in-chunks main-handle (max-problem-p (second (first pairs))) factor
                                         rows cols max-pivots n status2 pivots)
             (loop for (nil main-tab) in pairs for k from 0
                   collect (let ((st (if (= (cffi:mem-aref between :int32 k) +mi-optimal+)
                                         (cffi:mem-aref status2 :int32 k)
                                         (cffi:mem-aref between :int32 k))))
                             (or (outcome-condition st)
                                 (multibatch-read-back main-handle k main-tab full-tableau))))))
      (when main-handle (%multibatch-destroy main-handle))
      (%multibatch-destroy art-handle))))

(defun solve-same-shape-batch (tableaus devices factor max-pivots full-tableau)
  "TABLEAUS: single-phase tableaus of ONE shape and ONE sense.  Packs them into one multi-device
batch, solves them side by side and writes every member's results back into its own arrays.
Returns a list parallel to TABLEAUS: the tableau, or a condition object for a member without a
solution (unbounded-problem-error ...)."
  (let* ((n (length tableaus))
         (matrix (tableau-matrix (first tableaus)))
         (rows (array-dimension matrix 0))
         (cols (array-dimension matrix 1))
         (handle (multibatch-create tableaus devices)))
    (unwind-protect
         (cffi:with-foreign-objects ((status :int32 n) (pivots :int64 n))
           (multibatch-solve-in-chunks handle (max-problem-p (first tableaus)) factor rows cols
                                       max-pivots n status pivots)
           (loop for tab in tableaus for k from 0
                 collect (or (outcome-condition (cffi:mem-aref status :int32 k))
                             (multibatch-read-back handle k tab full-tableau))))
      (%multibatch-destroy handle))))

(defun mi355x-solve-problems (problems &rest args
                              &key (fp-tolerance 1024) (device 0) (devices 1) (max-pivots 0)
                                full-tableau (errorp t) native exact (exact-max-bits 128)
                                (pivot-rule :dantzig) (precision :double)
                              &allow-other-keys)
  "Solves a LIST of problems and returns the list of their solved tableaus, in order -- what
  (mapcar #'solve-problem problems) returns, with the independent LPs running side by side on
the GPU(s) instead of one after the other.
  * Single-phase problems (every row a <= row after build-tableau's sign normalisation,
    src/simplex.lisp:243-263) are grouped by tableau shape and sense; a group of two or more is one
    multi-device batch (mi355x_multibatch_*: DEVICES sub-batches, one per GPU, no communication).
  * Two-phase problems (build-tableau returned (art main), src/simplex.lisp:326-328) are grouped by
    the shapes of their two tableaux; a group of two or more is a pair of batches -- phase 1, the
    per-member feasibility test, drive-out pivots and hand-over (src/simplex.lisp:402-452) and phase 2
    on the devices, each phase in bounded foreign calls (mi355x_multibatch_solve with a cap,
    mi355x_multibatch_two_phase_handover between them).  Problems alone in their group go through
    MI355X-SIMPLEX-SOLVER one by one.
  * A member without a solution does not abort the others: with :ERRORP NIL its place in the
    result holds the condition object (unbounded-problem-error, infeasible-problem-error,
    unsupported-constraint-error ...); with :ERRORP T (default, what mapcar of solve-problem
    would do) the first such condition is signalled after every member has been attempted.
  * :NATIVE :MANY hands the whole list to the library instead (mi355x_simplex_solver_many_*: the
    problems marshalled as they are, tableaux assembled, grouped and batched in C++): the result list
    then holds MI355X-SOLUTION objects -- the way to solve BASELINE config 4's 1 024 LPs from Lisp
    without 1 024 boxed tableaux.  (:NATIVE NIL, the default, keeps every member a `tableau`.)
  * :EXACT T (opt-in) solves the members whose numbers are all rational (and that have no integer
    variables) with the reference's rational semantics (src/utils.lisp:84-124): they are grouped by
    tableau shape and sense in the same way, and a group of two or more is ONE batch of exact
    tableaux (mi355x_xbatch_*: one workgroup per member, both phases and everything between them on
    the device, in bounded foreign calls) -- every member comes back as the solved `tableau` that
    (mi355x-simplex-solver p :exact t) returns, its matrix holding the exact ratios.  Members alone
    in their group, shapes the batch declines and members with a float anywhere go through
    (mi355x-simplex-solver p :exact t) one by one; :MAX-PIVOTS caps each member, both phases
    together.  :EXACT-MAX-BITS 256 (default 128): the batches stay at 64 / 128 bits, and a member a
    batch declines for outgrowing them is solved again, alone, with 256 bits allowed; its result (or its
    condition) takes its place, the other members are untouched.  :EXACT NIL (default): nothing changes.
  * :PIVOT-RULE (:DANTZIG, the default, :BLAND or :DANTZIG-BLAND; with :EXACT T only): MI355X-SIMPLEX-SOLVER's,
    for every batch and every member solved alone, the 256-bit re-solve included.  An unknown rule and a rule
    other than :DANTZIG without :EXACT T are errors; a member that holds a float declines such a rule, and its
    condition takes its place.
  * The other keywords are MI355X-SIMPLEX-SOLVER's, applied to every member: :FP-TOLERANCE (the
    tolerance factor, src/simplex.lisp:506-511), :DEVICE (the GPU of members solved alone), :DEVICES
    (a count or a list of device ids: the sub-batches' GPUs), :MAX-PIVOTS (a cap per member; 0 = none,
    as the reference), :FULL-TABLEAU (every entry of every solved tableau written back).
  * :PRECISION :SINGLE (opt-in; :DOUBLE, the default, is everything above, unchanged): every member takes the
    reference's single-float path, what (mi355x-simplex-solver p :precision :single) returns for it -- the
    reference's build-tableau, every entry a single-float or an integer of at most 2^24 in magnitude (a member
    with anything else is declined, its unsupported-constraint-error (single ENTRY) takes its place),
    single-float arithmetic and single-float-epsilon thresholds.  Single-phase members are grouped by shape
    and sense, two-phase members by the shapes of their two tableaux (no unit-basis restriction), and a
    group of two or more is ONE batch of single-float tableaux (mi355x_sbatch_*: one workgroup per member with
    the member's tableau in LDS, both phases and everything between them on the device, in bounded foreign
    calls); the solved single-floats are written back into each member's `tableau`.  Members alone in their
    group, shapes beyond the batch's LDS budget and integer problems go one by one.  Together with :EXACT,
    :NATIVE :MANY, more than one of :DEVICES or a :PIVOT-RULE other than :DANTZIG it is an error that names
    the keyword; so is an unknown precision.
Every returned solution object's results are bit-identical to the single-problem path's."
  (declare (ignore args))
  (check-list-precision precision exact native devices pivot-rule)
  (when (eq precision :single)
    (let ((results (solve-problems-in-single-precision problems fp-tolerance device max-pivots)))
      (when errorp
        (let ((failed (find-if (lambda (r) (typep r 'condition)) results)))
          (when failed (error failed))))
      (return-from mi355x-solve-problems results)))
  (check-pivot-rule pivot-rule exact)
  (when (and (eq native :many) (not full-tableau) problems)
    ;; the whole list behind ONE job of the library: no build-tableau, no boxed matrices; the members
    ;; come back as MI355X-SOLUTION objects
    (let ((results (solve-problems-natively problems (coerce fp-tolerance 'double-float)
                                            (if (and (integerp devices) (<= devices 1)) (list device) devices)
                                            max-pivots)))
      (when errorp
        (let ((failed (find-if (lambda (r) (typep r 'condition)) results)))
          (when failed (error failed))))
      (return-from mi355x-solve-problems results)))
  (when exact
    (let ((results (solve-problems-exactly
                    problems device max-pivots
                    (lambda (k problem)
                      (declare (ignore k))
                      (handler-case (mi355x-simplex-solver problem :fp-tolerance fp-tolerance
                                                                   :device device :max-pivots max-pivots
                                                                   :full-tableau full-tableau
                                                                   :native native :exact t
                                                                   :exact-max-bits exact-max-bits
                                                                   :pivot-rule pivot-rule)
                        (error (c) c)))
                    exact-max-bits (pivot-rule-code pivot-rule))))
      (when errorp
        (let ((failed (find-if (lambda (r) (typep r 'condition)) results)))
          (when failed (error failed))))
      (return-from mi355x-solve-problems (coerce results 'list))))
  (let* ((n (length problems))
         (results (make-array n :initial-element nil))
         (groups (make-hash-table :test #'equal))
         (groups2 (make-hash-table :test #'equal))          ; two-phase members, by the shapes of (art main)
         (factor (coerce fp-tolerance 'double-float)))
    (flet ((solve-alone (k problem)
             (setf (aref results k)
                   ;; (:native NIL, the default here, keeps the result list homogeneous -- every member
                   ;; a `tableau`; :native :auto lets a member solved alone take the native route)
                   (handler-case (mi355x-simplex-solver problem :fp-tolerance fp-tolerance
                                                                :device device :max-pivots max-pivots
                                                                :full-tableau full-tableau
                                                                :native native)
                     (error (c) c)))))
      ;; build-tableau for every member; two-phase members and integer problems leave the batch
      (loop for problem in problems for k from 0
            do (if (problem-integer-vars problem)
                   (solve-alone k problem)             ; -> unsupported-constraint-error
                   (let ((tableaus (handler-case
                                       (build-tableau problem problem :fp-tolerance-factor fp-tolerance)
                                     (error (c) c))))
                     (cond
                       ((typep tableaus 'condition) (setf (aref results k) tableaus))
                       ((listp tableaus)
                        (let ((art (tableau-matrix (first tableaus)))
                              (main (tableau-matrix (second tableaus))))
                          (push (cons k tableaus)
                                (gethash (list (array-dimension art 0) (array-dimension art 1)
                                               (array-dimension main 1) (max-problem-p (second tableaus)))
                                         groups2))))
                       ((not (unit-basis-p tableaus)) (solve-alone k problem))
                       (t
                        (let ((matrix (tableau-matrix tableaus)))
                          (push (cons k tableaus)
                                (gethash (list (array-dimension matrix 0) (array-dimension matrix 1)
                                               (max-problem-p tableaus))
                                         groups))))))))
      (maphash
       (lambda (shape members)
         (declare (ignore shape))
         (setf members (reverse members))
         (if (rest members)
             (loop for (k . nil) in members
                   for outcome in (solve-same-shape-batch (mapcar #'cdr members) devices factor
                                                          max-pivots full-tableau)
                   do (setf (aref results k) outcome))
             (solve-alone (car (first members)) (nth (car (first members)) problems))))
       groups)
      (maphash
       (lambda (shape members)
         (declare (ignore shape))
         (setf members (reverse members))
         (if (rest members)
             (loop for (k . nil) in members
                   for outcome in (solve-two-phase-batch (mapcar #'cdr members) devices factor
                                                         max-pivots full-tableau)
                   do (setf (aref results k) outcome))
             (solve-alone (car (first members)) (nth (car (first members)) problems))))
       groups2))
    (when errorp
      (let ((failed (find-if (lambda (r) (typep r 'condition)) results)))
        (when failed (error failed))))
    (coerce results 'list)))
