/* lsfm.h -- C ABI of the MI355X-native LinearSFM hot path (liblsfm_hip.so).
 *
 * Every entry point replaces one public method of the reference's CLinearSFMImp
 * (/root/reference/linux/src/LinearSFMImp/LinearSFMImp.h, "Imp.h"; bodies in LinearSFMImp.cpp, "Imp.cpp").
 * Plain pointers and sizes only; all arrays are HOST arrays in the reference's own layout unless the name
 * says "dev".  Every function returns an int status: 0 ok, <0 invalid input / runtime failure, >0 numerical
 * (PCG not converged / not positive definite).  The reference's methods are void and ignore CHOLMOD's
 * status (Imp.cpp:2356, 7006).  There is NO CPU fallback: without a usable HIP device every call fails with
 * LSFM_ERR_NO_DEVICE.
 *
 * Map layout (= LocalMapInfoStereo / LocalMapInfo, Imp.h:75-178):
 *   stno[6m+3n]   labels: <=0 pose id (-stno, x6), >0 feature id (x3)
 *   stVal[6m+3n]  poses (tx ty tz alpha beta gamma) then features (x y z)
 *   U[nU*36]      6x6 row-major pose-pose information blocks, (Ui,Uj) block coordinates, Ui<=Uj, diagonal
 *                 blocks stored full; several entries with the same coordinates add up
 *   W[nW*18]      6x3 row-major pose-feature blocks, (photo, feature), sorted by feature, >=1 per feature
 *   V[n*9]        3x3 feature blocks;  FBlock[n] first W index of each feature
 *   Mono only:    ScaP (id of the scale pose), Fix (0..2 fixed translation axis of ScaP), Sign (+-1),
 *                 FScaP / FFix (those of the map's first frame)
 */
#ifndef LSFM_H
#define LSFM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSFM_OK 0
#define LSFM_ERR_ARG (-1)
#define LSFM_ERR_NO_DEVICE (-2)
#define LSFM_ERR_HIP (-3)
#define LSFM_ERR_OOM (-4)
#define LSFM_ERR_INTERNAL (-5)
#define LSFM_ERR_IO (-6)
#define LSFM_ERR_NOT_SPD (-7) /* a camera system whose factorisation met a pivot far below zero: the information matrices are not positive definite */
#define LSFM_NOT_CONVERGED 1

typedef struct lsfm_context lsfm_context; /* one per GPU / stream; thread-compatible, not thread-safe */

/* mirrors LocalMapInfoStereo / LocalMapInfo (Imp.h:75-178); arrays owned by whoever filled the struct */
typedef struct lsfm_map {
	int Ref, FRef, m, n, nU, nW;
	int ScaP, Fix, Sign, FScaP, FFix; /* Mono only */
	int* stno;
	double* stVal;
	double* U;
	int *Ui, *Uj;
	double* W;
	int *photo, *feature;
	double* V;
	int* FBlock;
	/* optional extension (NULL = absent): per pose, the index of the LOCAL MAP that brought it into the tree.  Only
	 * used to order the Cholesky preconditioner along the join tree; filled on outputs, honoured on inputs, so that a
	 * map produced by one lsfm_tree_run can seed another (multi-GPU subtree sharding). */
	int* pose_origin;
} lsfm_map;

typedef struct lsfm_stats {
	/* whole run */
	double t_total_ms;      /* region the reference times: Imp.cpp:1929 -> 2068 (all transforms + joins) */
	double t_transform_ms, t_join_ms, t_schur_ms, t_pcg_ms, t_backsub_ms;
	long pcg_iterations;    /* sum over levels of the iterations run (batched systems iterate together) */
	long spmv_launches;
	double spmv_ms;         /* HIP-event time of all SpMV launches, measured on the context's stream */
	double spmv_bytes;      /* algorithmic bytes of all SpMV launches ("K10a") */
	long spmv_nnzb_upper_last, spmv_rows_last; /* upper blocks / block rows of the last (top) system */
	double max_rel_residual;/* max over systems of ||E - S x|| / ||E|| at exit */
	int levels, joins, transforms;
	int not_converged;      /* number of systems that hit the iteration cap */
	/* the two instrumented kernels, each bracketed by HIP events on the context's stream (one bracket per tree level):
	 * K9 k_schur_panel (Schur assembly, all panel variants of a level + k_schur_w for the tiles none of them takes) and
	 * K3/K4 k_tr_entries (information transform, one lane per W block).  bytes = algorithmic bytes of those launches
	 *  */
	long schur_launches, trf_launches;
	double schur_ms, schur_bytes, trf_ms, trf_bytes;
	/* algorithmic flops of the K9 launches: per feature with k W blocks, k (108 + 36) for W V^-1 and the right-hand side and
	 * k (k + 1) / 2 * 216 for the pose pairs (Imp.cpp:2260-2328) -- at the top levels K9 is bound by the fp64 matrix rate */
	double schur_flops;
	/* wall ms lsfm_tree_upload took to bring the tree's N local maps into HBM (PCIe; never part of t_total_ms) */
	double upload_ms;
	/* how many times the tree was joined by this call: 1, or more when a run was repeated (a plan or step count of an earlier run
	 * that did not fit the values, a system left above its bound by an unlucky rounding of its factorisation) */
	int attempts;
	/* LSFM_FACTOR_DIGEST=1 in the environment (a debug / test aid, off by default: two more passes over every factor): sums
	 * modulo 2^64 of the mixed bit patterns of every camera system as assembled (s_digest) and of every Cholesky factor the run
	 * computed (factor_digest), over all levels.  The factorisation accumulates its updates in fixed point (integer atomics), so two
	 * runs with equal s_digest have equal factor_digest, whatever order the work-groups ran in. */
	unsigned long long s_digest, factor_digest;
	/* feature-sharded runs: tree levels whose camera systems were factored distributed over the ranks (lsfm_tree_set_comm_blocks) */
	int dist_solves;
	/* ... and, over those levels, the block products (6x6x6 multiply-adds) of the numeric factorisations: all of them / those of the
	 * shared separator columns, which every rank repeats (the replicated share: an Amdahl bound of the distributed solve) */
	double dist_work_total, dist_work_shared;
	/* LSFM_FACTOR_DIGEST=1: every camera system of the run is factored TWICE (the work-groups of the two factorisations are scheduled
	 * differently, their atomics land in another order); the number of systems whose two factors were not the same bits.  Must be 0:
	 * the accumulation is in fixed point. */
	int refactor_mismatch;
	/* LSFM_FACTOR_DIGEST=1: the camera systems of every level (S and the right-hand side E) are ASSEMBLED twice from the same joint
	 * maps (K9's work-groups land their sums in another order); the number of levels whose two assemblies were not the same bits.
	 * Must be 0 since round 5: K9 adds in fixed point (include: the per-feature fallback kernel). */
	int s_rebuild_mismatch;
	/* tree levels (or stage-level calls) whose camera systems -- at most 16 poses each -- were assembled, factored and solved by the
	 * one-launch dense path (one work-group per join, the system in LDS: lsfm_small.hip), and the HIP-event time of those launches */
	int small_levels;
	double t_small_ms;
} lsfm_stats;

/* ---- context ------------------------------------------------------------------------------------ */
/* device: HIP device ordinal.  arena_bytes: device memory reserved for maps and work space (0 = size on
 * demand from the inputs of the first call).  Fails with LSFM_ERR_NO_DEVICE when no GPU is usable. */
int lsfm_context_create(int device, size_t arena_bytes, lsfm_context** out);
void lsfm_context_destroy(lsfm_context* ctx);
/* Solver controls.  rel_tol: the refinement of a system stops when ||E - S x|| <= rel_tol * ||E|| (default 1e-12: the
 * residual level of a direct fp64 solve, which is what the reference computes) or when the true residual stops
 * shrinking.  max_steps: most refinement steps a system may take, 1 .. 50 (<= 0: the default, 50); a system that is
 * still above 1e-9 relative when the cap is reached counts as not converged. */
int lsfm_set_pcg(lsfm_context* ctx, double rel_tol, int max_steps);
/* Precision of the preconditioner.  mode 0 (default): fp64 throughout, the reference's arithmetic.  mode 1, "mixed": the
 * Cholesky factor of every camera system is kept and applied in fp32 (half the bytes of the triangular solves; the
 * factorisation itself runs in fp64 and is rounded once -- an fp32 elimination breaks down on these matrices), while S,
 * the right-hand side, the iterate and the residual r = E - S x stay fp64: every refinement step corrects against the
 * fp64 residual, and the stopping rule is the same relative residual as in mode 0, reached in more steps (2-3 instead
 * of 1).  BASELINE.json configs[4]. */
int lsfm_set_precision(lsfm_context* ctx, int mode);
/* Camera systems of a few poses (the lowest levels of a tree: thousands of independent joins a level) are assembled, factored (dense
 * Cholesky in LDS, one refinement step) and solved, features included, by ONE launch with one work-group per join instead of the level
 * pipeline's ~55 (Imp.cpp:2119-2378, run per join by the reference).  max_poses: the largest system that takes this path -- 0: none,
 * every level takes the sparse pipeline; at most 16 (what the kernel holds); default 5 (Stereo: the two lowest levels; where the path
 * beats the pipeline).  The tests compare the two paths at every size.  Feature-sharded runs and the fp32 preconditioner
 * always take the pipeline. */
int lsfm_set_small_solve(lsfm_context* ctx, int max_poses);
/* Which kernel multiplies by the Schur matrix in the CG.  0 (default): by size -- a matrix that stays in L2 / Infinity
 * Cache (every level of the named configurations) is multiplied from a row-sorted list of both orientations of its
 * blocks, a larger one streams its upper blocks from HBM once.  1: always the streaming kernel.  2: always the list.
 * A measurement / test knob; it applies to the systems analysed after the call (a recorded plan keeps its choice). */
int lsfm_set_spmv_variant(lsfm_context* ctx, int variant);
/* Which kernel of lsfm_map_covariance_columns multiplies a supernode group's dense panel with the solved columns.  0 (default): the
 * faster one where measured.  1: lane per column, inside the group's own launch.  2: 16x16 tiles on
 * v_mfma_f64_16x16x4_f64 in a launch of their own.  A measurement / test knob: the results agree to rounding. */
int lsfm_set_covcols_panel(lsfm_context* ctx, int variant);
const char* lsfm_last_error(lsfm_context* ctx);
void* lsfm_stream(lsfm_context* ctx); /* hipStream_t the library launches on */

/* frees the arrays of a map that the LIBRARY allocated (outputs of the functions below) */
void lsfm_map_release(lsfm_map* g);

/* ---- the three methods the reference's scheduler calls ------------------------------------------ */
/* replaces CLinearSFMImp::lmj_Transform_PF3DStereo (Imp.h:206, Imp.cpp:349-1924): `in` expressed in the frame
 * of its pose `Ref`.  out: library-allocated. */
int lsfm_transform_stereo(lsfm_context* ctx, const lsfm_map* in, int Ref, lsfm_map* out);
/* replaces lmj_Transform_PF3DMono (Imp.h:218, Imp.cpp:3173-6509) */
int lsfm_transform_mono(lsfm_context* ctx, const lsfm_map* in, int Ref, int ScaP, int Fix, lsfm_map* out);

/* replaces lmj_LinearLS_PF3DStereo (Imp.h:207, Imp.cpp:2551-2978): joins End (already in Cur's frame) with Cur
 * and solves.  Unlike the reference (which frees both inputs, Imp.cpp:2937-2958, and publishes the result in
 * the member m_GMapS) inputs are left untouched and the joint map is returned in `joint`.
 * eP_out[6m] / eF_out[3n] (optional, may be NULL) receive the assembled right-hand sides. */
int lsfm_join_stereo(lsfm_context* ctx, const lsfm_map* End, const lsfm_map* Cur, lsfm_map* joint,
                     double* eP_out, double* eF_out);
/* replaces lmj_LinearLS_PF3DMono (Imp.h:221, Imp.cpp:7282-7874).  The reference unwraps the scale-pose angles of
 * both inputs in place (Imp.cpp:7427-7465); here the inputs stay const and the unwrapped values are used inside. */
int lsfm_join_mono(lsfm_context* ctx, const lsfm_map* End, const lsfm_map* Cur, lsfm_map* joint,
                   double* eP_out, double* eF_out);

/* replaces lmj_solveLinearSFMStereo (Imp.h:209, Imp.cpp:2119-2378), same argument list + context.
 * Schur complement on the features, preconditioned CG on the camera system (instead of CHOLMOD),
 * back-substitution.  Writes stVal[0..6m+3n).  x0 (optional, may be NULL): initial guess for the 6m pose
 * scalars.  V is read only (the reference inverts it in place and restores it).
 * LSFM_ERR_ARG for W not sorted by feature, a feature without a W block, a photo index outside [0, m) and a U block that does not
 * satisfy 0 <= Ui <= Uj < m (lsfm_solve_mono alike). */
int lsfm_solve_stereo(lsfm_context* ctx, double* stVal, const double* eb, const double* ea, const double* U,
                      const double* W, const double* V, const int* Ui, const int* Uj, const int* photo,
                      const int* feature, int m, int n, int nU, int nW, const double* x0);
/* replaces lmj_solveLinearSFMMono (Imp.h:223, Imp.cpp:6756-7041); Ref/ScaP/Fix/Sign/FixBlk as at the reference's
 * call site Imp.cpp:7860-7864 (Ref = block index of the reference pose, ScaP = its scalar offset, Fix = scalar
 * index of the gauge-fixed translation). */
int lsfm_solve_mono(lsfm_context* ctx, double* stVal, const double* eb, const double* ea, const double* U,
                    const double* W, const double* V, const int* Ui, const int* Uj, const int* photo,
                    const int* feature, int m, int n, int nU, int nW, int Ref, int ScaP, int Fix, int Sign,
                    int FixBlk, const double* x0);

/* ---- Gauss-Newton polish of the map-joining objective (BASELINE.json north_star "plus the Gauss-Newton BA refinement") ----
 * NO reference counterpart: the reference joins once and has no iterative step (no loop and no residual anywhere in LinearSFMImp.cpp) --
 * PARITY UNPINNED; the tests hold it against the CPU checker's statement of the same steps and against properties (the objective never rises, its gradient falls, a minimiser is
 * a fixed point).  Minimises, over the global state x and ALL N local maps at once,
 *     F(x) = sum_k || x^_k - f_k(x) ||^2_{I_k}
 * x^_k / I_k: estimate / information matrix of local map k, f_k: the reference's own change of frame into map k's frame
 * (Imp.cpp:421-455, Mono 3268-3306) with the Jacobian the reference's transform forms (Imp.cpp:485-683, Mono 3383-3688) -- the objective
 * every join of the tree linearises once.  A step solves H d = b (H = sum J^T I J, b = sum J^T I r) through the same Schur + factorisation
 * as a tree level and takes x += a d, a = 1 halved (at most 8 times) while F does not fall; a step without decrease ends the run.
 * maps[N]: the local maps the tree was built from.  x: the global state to start from -- m, n, stno, stVal (updated in place; arrays of
 * the caller), Ref = the pose its frame is anchored at (Stereo: not in the state; a local map with that Ref is in the global frame),
 * Mono: ScaP / Fix (the gauge: the 6 scalars of pose Ref and scalar Fix of pose ScaP stay where they are), optional pose_origin --
 * e.g. the result of lsfm_tree_download / lsfm_divide_conquer.  type: 0 Stereo, 1 Monocular.  obj[iters + 1], gnorm[iters + 1]: F and
 * max |b_i| over the free scalars at the start and after every step; halvings[iters] (may be NULL; 9: no decrease found).
 * Returns LSFM_OK, LSFM_NOT_CONVERGED (a step's camera system stayed above its residual bound), < 0 errors (LSFM_ERR_ARG: a local
 * variable that is not in the global state, a global variable no map holds, a Stereo map that holds the global reference pose). */
int lsfm_gn_polish(lsfm_context* ctx, const lsfm_map* maps, int N, int type, lsfm_map* x, int iters, double* obj, double* gnorm, int* halvings);

/* ---- per-map consistency of a joined map and the robust polish (NO reference counterpart: the reference has no objective to evaluate
 * and no step -- PARITY UNPINNED; the tests hold both against the CPU checker's F with the local maps' information matrices scaled) ----
 * chi2[N]: chi^2_k = r_k^T I_k r_k with r_k = x^_k - f_k(x) (angles wrapped) at the global state x, the terms of lsfm_gn_polish's F;
 * dof[N] (optional, may be NULL): the length of map k's state vector, 6 m_k + 3 n_k.  Same arguments and errors as lsfm_gn_polish; x is
 * read only.  One work-group per map sums its U, W and V terms in a fixed order (no atomics): the same input gives the same bits. */
int lsfm_map_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, double* chi2, int* dof);
/* Gauss-Newton polish with whole local maps as the M-estimator's residuals (IRLS).  kind: 0 none (exactly lsfm_gn_polish), 1 Huber,
 * 2 Cauchy; c > 0 (finite, checked for every kind) the threshold on s_k = chi2_k / dof_k.  Minimises G(x) = sum_k dof_k rho(chi2_k(x) / dof_k):
 *   Huber  rho(s) = s (s <= c^2),  2 c sqrt(s) - c^2 otherwise;   w = rho'(s) = min(1, c / sqrt(s))
 *   Cauchy rho(s) = c^2 ln(1 + s / c^2);                          w = rho'(s) = 1 / (1 + s / c^2)
 * A step solves the Gauss-Newton system with I_k replaced by w_k I_k (w_k at the current state) and takes x += a d, a halved while G
 * does not fall, exactly as lsfm_gn_polish does with F; the gauge (Mono) is lsfm_gn_polish's.  obj[iters + 1] = G per iterate (kind 0:
 * F); gnorm[iters + 1] as lsfm_gn_polish, of the weighted gradient; halvings[iters] (may be NULL); chi2[N], weight[N] (each may be
 * NULL): at the returned state (chi2 bit for bit what lsfm_map_chi2 gives there; kind 0: every weight 1).  Returns as lsfm_gn_polish;
 * LSFM_ERR_ARG also for an unknown kind or c <= 0 / not finite. */
int lsfm_gn_polish_robust(lsfm_context* ctx, const lsfm_map* maps, int N, int type, lsfm_map* x, int iters, int kind, double c,
                          double* obj, double* gnorm, int* halvings, double* chi2, double* weight);

/* ---- per-feature consistency and the polish that down-weights single features (NO reference counterpart: PARITY UNPINNED; the tests
 * hold both against the CPU checker's F on re-weighted map dicts) ----
 * For local map k with I_k = [U W; W^T V] and residual r = (r_p, r_f) at the global state x,
 *     chi2_k = r_p^T (U - sum_f W_f V_f^-1 W_f^T) r_p + sum_f c_kf,   c_kf = g_f^T V_f^-1 g_f >= 0,   g_f = V_f r_f + sum_a W_af^T r_a:
 * c_kf is the chi^2 (3 degrees of freedom) of feature f of map k given the map's poses.
 * fchi2[sum_k n_k]: c_kf in map order, within a map in the map's feature order.  pose_chi2[N] (may be NULL): chi2_k - sum_f c_kf, the pose
 * part under the map's own Schur complement.  Arguments and errors: lsfm_map_chi2's; x is read only.  LSFM_ERR_NOT_SPD: a V_f is not
 * positive definite (lsfm_last_error names the map and the feature).  One work-group per map, V_f^-1 by a 3x3 Cholesky in registers,
 * every sum in a fixed order and no atomics: the same input gives the same bits. */
int lsfm_map_feature_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, double* fchi2, double* pose_chi2);
/* Gauss-Newton polish with single features of single local maps as the M-estimator's residuals (IRLS).  kind: 0 none (exactly
 * lsfm_gn_polish), 1 Huber, 2 Cauchy with rho and rho' as stated for lsfm_gn_polish_robust, on s_kf = c_kf / 3; c > 0 finite.  Minimises
 *     G(x) = sum_k (chi2_k - sum_f c_kf) + 3 sum_kf rho(c_kf / 3).
 * Scaling the conditional term of feature f by w_f is again an information matrix,
 *     I_k(w) = [U - sum_f (1 - w_f) W_f V_f^-1 W_f^T,  w_f W_f;  w_f W_f^T,  w_f V_f]     (w = 1: I_k;  w_f = 0: f marginalised out),
 * so a step solves the Gauss-Newton system of the maps I_k(w_k), w_kf = rho'(s_kf) at the current state, and takes x += a d, a halved
 * while G does not fall, as the other polishes do (G summed in a fixed order).  No map-level weight is applied (w_k = 1): the two
 * estimators are not combined.  A redescending weight (Cauchy) on Monocular sets can choose the wrong instance of a pulled feature
 * (DESIGN.md 16): prefer Huber there.  obj / gnorm / halvings as lsfm_gn_polish_robust; fchi2[sum_k n_k], fweight[sum_k n_k] (each may be
 * NULL): at the returned state, fchi2 bit for bit what lsfm_map_feature_chi2 gives there; kind 0: every weight 1.  Returns and argument
 * errors: lsfm_gn_polish_robust's; LSFM_ERR_NOT_SPD as lsfm_map_feature_chi2. */
int lsfm_gn_polish_robust_features(lsfm_context* ctx, const lsfm_map* maps, int N, int type, lsfm_map* x, int iters, int kind, double c,
                                   double* obj, double* gnorm, int* halvings, double* fchi2, double* fweight);

/* ---- the information matrix at a state: the joint map of the N local maps linearised at x ----
 * H = sum_k w_k J_k^T I_k J_k and the state x as an lsfm_map (library-allocated: lsfm_map_release), the matrix a step of
 * lsfm_gn_polish[_robust] solves with at x.  maps / N / type / x and every argument check: lsfm_gn_polish's; x is read only.
 * weight[N] (may be NULL: all 1): finite, >= 0 (else LSFM_ERR_ARG) -- e.g. what lsfm_gn_polish_robust returned.
 * obj (may be NULL): sum_k w_k chi2_k.  b[6m + 3n] (may be NULL): sum_k w_k J_k^T I_k r_k, poses then features, x's order.
 * No reference counterpart: PARITY UNPINNED, as for lsfm_gn_polish.
 * The map is canonical and its structure depends on the labels alone, never on values: m, n, stno, stVal, Ref, FRef, ScaP, Fix, Sign,
 * FScaP, FFix are x's; pose_origin is x's if given, else the first local map holding the pose; U has exactly one block per pose pair
 * (Ui <= Uj) that a local map or a hub role (a map's Ref / ScaP pose against its poses) produces, sorted by (Ui, Uj), diagonal blocks
 * full; W is sorted by feature and within a feature by ascending pose, exactly one block per (pose, feature) -- a block whose value
 * happens to be zero stays --, feature[] / FBlock[] to match; V one block per feature.  Mono: the rows and columns of the gauge
 * scalars are kept (the gauge is applied by whoever inverts: lsfm_map_covariance(mono = 1) reads it from Ref / ScaP / Fix).  The
 * result is an input like any other map to lsfm_map_covariance[_columns], lsfm_schur_pattern, lsfm_write_localmap / _mapset and
 * lsfm_tree_upload.
 * One assembly of the polish at x, then two kernels that sum the repeated blocks of its working form (one lane per output block, its
 * sources in map order, no atomics).  The assembly in front of them adds with atomics: two calls agree to rounding, NOT bit for bit.
 * Lifetime: works in the context's arenas like lsfm_gn_polish. */
int lsfm_gn_linearise(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight,
                      lsfm_map* out, double* obj, double* b);
/* measurement entry: the same, and times[3] (may be NULL) = HIP-event ms of the assembly, of the W and of the U coalescing launch;
 * counts[4] (may be NULL) = blocks of the working form's W, of out's W, of the working form's U, of out's U */
int lsfm_gn_linearise_timed(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight,
                            lsfm_map* out, double* obj, double* b, double* times, int* counts);
/* The same at given feature weights: the matrix, the quadratic value and the gradient of one step of lsfm_gn_polish_robust_features
 * at fixed weights,
 *     H = sum_k w_k J_k^T I_k(w_k.) J_k,   obj = sum_k w_k (pose_chi2_k + sum_f w_kf c_kf),   b = sum_k w_k J_k^T I_k(w_k.) r_k
 * with I_k(w) as stated for lsfm_gn_polish_robust_features.  fweight[sum_k n_k] (not NULL): w_kf in map order and within a map in the
 * map's feature order -- the order lsfm_gn_polish_robust_features returns.  Every entry must be finite and in [0, 1], else LSFM_ERR_ARG
 * (lsfm_last_error names the map and the feature; the context stays usable): a weight above 1 would SUBTRACT a positive semi-definite
 * term from the map's Schur complement U - sum_f W_f V_f^-1 W_f^T, and I_k(w) is positive semi-definite for every w in [0, 1] only.
 * weight[N] (may be NULL) as for lsfm_gn_linearise; the two multiply.  Every other argument check is lsfm_gn_linearise's;
 * LSFM_ERR_NOT_SPD: a V_f is not positive definite (the map and the feature are named, as by lsfm_map_feature_chi2).
 * `out` is canonical exactly as lsfm_gn_linearise's, with one difference: U also holds a block for every pair of poses of a local map
 * that see a common feature (the places the correction of U falls into), whether or not the map holds a U block there.  The structure
 * depends on the labels alone, never on fweight: a block that exists only for the correction is exactly 0.0 when every weight of its
 * features is 1, and a V block whose instances all have weight 0 is a zero block and stays.  W and V follow lsfm_gn_linearise's rules.
 * The chi^2 pass of lsfm_map_feature_chi2 (reading the weights), the fill of the correction slots, the feature-robust step's assembly,
 * then the two coalescing kernels; obj is summed in a fixed order. */
int lsfm_gn_linearise_features(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight,
                               const double* fweight, lsfm_map* out, double* obj, double* b);
/* measurement entry: times[4] (may be NULL) = HIP-event ms of the chi^2 pass + slot fill, of the rest of the assembly, of the W and of
 * the U coalescing launch; counts[4] as lsfm_gn_linearise_timed */
int lsfm_gn_linearise_features_timed(lsfm_context* ctx, const lsfm_map* maps, int N, int type, const lsfm_map* x, const double* weight,
                                     const double* fweight, lsfm_map* out, double* obj, double* b, double* times, int* counts);

/* ---- marginal covariances of a map (NO reference counterpart: the reference keeps the information matrix and never inverts it) ----
 * Sigma = I^-1 with I = [U W; W^T V] of `map` (any lsfm_map: a downloaded tree result, a checkpoint node, a local map).
 * mono = 0: Stereo, I is used as it is (the map's Ref pose is not in its state).  mono = 1: the gauge of lsfm_solve_mono /
 * lsfm_gn_polish -- the 6 scalars of the pose labelled map->Ref and scalar map->Fix (0..2) of the pose labelled map->ScaP are held
 * fixed: Sigma is the inverse with those rows / columns removed, and it is reported as 0 there.
 * Outputs (each optional, NULL = not wanted; all in the map's own order of poses / features, unscaled, unpermuted):
 *   pose_cov[36 m]   Sigma_pp, row-major 6x6 per pose
 *   feat_cov[9 n]    Sigma_ff, row-major 3x3 per feature
 *   pair_cov[36 cap_blocks]  Sigma_pq for every block (p <= q) of the camera system's pattern, in the order lsfm_schur_pattern returns
 *                    for the same map (row by row, diagonal block first); *nnzb receives the count (LSFM_ERR_ARG when cap_blocks is
 *                    too small, *nnzb still set)
 * Always fp64 and always the sparse factorisation (lsfm_set_precision / lsfm_set_small_solve do not apply); deterministic: the same
 * input gives the same bits.  The camera system is factored as a tree level's is, then inverted on the factor's own pattern (selected
 * inversion); the features follow from Sigma_ff = V^-1 + V^-1 (sum W^T Sigma W) V^-1.
 * Returns LSFM_OK; LSFM_ERR_NOT_SPD when the factorisation met a non-positive pivot; > 0 (the number of floored pivots) when a pivot
 * had to be floored (the result is then not the inverse of I and nothing is written); < 0 errors as elsewhere (LSFM_ERR_ARG: W not
 * sorted by feature, a Mono map whose Ref / ScaP is not in its state).
 * Lifetime: works in the context's arenas like lsfm_solve_* -- a tree's result must be downloaded first. */
int lsfm_map_covariance(lsfm_context* ctx, const lsfm_map* map, int mono, double* pose_cov, double* feat_cov, double* pair_cov, int cap_blocks, int* nnzb);
/* measurement entry: the same, and times[4] (may be NULL) = HIP-event ms of the Schur reduction + symbolic analysis, the numeric
 * factorisation, the selected inversion (with the gather onto the pattern), the feature part */
int lsfm_map_covariance_timed(lsfm_context* ctx, const lsfm_map* map, int mono, double* pose_cov, double* feat_cov, double* pair_cov, int cap_blocks, int* nnzb,
                              double* times);

/* ---- whole columns of Sigma for chosen poses (NO reference counterpart) ----
 * Sigma_{.,Q} for the k distinct poses Q = poses[0..k) (indices into the map's own pose order, 0 <= poses[a] < m, k >= 1): every block
 * Sigma_{p,q} and Sigma_{f,q}, on AND off the camera system's pattern -- what gating a loop closure between two poses that share no
 * feature, the uncertainty of a relative pose or the joint marginal of a few key frames need.  map, mono, the gauge, the argument
 * checks and the lifetime in the context's arenas are lsfm_map_covariance's.  The camera system is factored as there; the 6 k unit
 * right-hand sides are solved side by side against the factor (in chunks of 32 poses) and refined in fp64 against S itself:
 * always one step, then while some column's correction |delta|_inf / |x|_inf is above the context's rel_tol (lsfm_set_pcg; default
 * 1e-12) and fell by at least half in the last step, at most max_steps steps.  On the 200-map Mono chain, where the unrefined
 * lsfm_map_covariance is 1e-6 of the variances off, three steps leave 2e-10.
 * Outputs (each optional, at least one non-NULL; unscaled, unpermuted):
 *   pose_cols[36 k m]  block Sigma_{p, poses[a]} at pose_cols + 36 (a m + p), row-major 6x6: rows = scalars of p, columns = scalars of poses[a]
 *   feat_cols[18 k n]  block Sigma_{f, poses[a]} at feat_cols + 18 (a n + f), row-major 3x6
 *   joint[6k * 6k]     Sigma_QQ, row-major, EXACTLY symmetric: block (a, b), a < b, is taken from column b and mirrored, a diagonal
 *                      block is (X + X^T) / 2
 *   steps              refinement steps taken (the most over the chunks)
 *   last_corr[k]       per requested pose the largest |delta_c|_inf / |x_c|_inf of the last correction over its six columns
 * Fixed scalars (Mono gauge) have zero rows and columns: asking for the Ref pose gives zeros.
 * Always fp64 and always the sparse factorisation (lsfm_set_precision / lsfm_set_small_solve do not apply).  NOT bit-reproducible
 * from call to call (the sweeps add into the rows of a column's ancestors by atomics); the refinement leaves the difference at
 * rounding level of the result.  lsfm_set_spmv_variant does not apply either: the residual is always taken from the row-sorted
 * list of S's blocks, built for this call.
 * Returns LSFM_OK; LSFM_NOT_CONVERGED when max_steps steps were taken and the last correction was still above rel_tol (the results are
 * written; a refinement that stops because its corrections no longer halve has reached what fp64 gives and is LSFM_OK -- last_corr
 * says where it ended); LSFM_ERR_NOT_SPD, and > 0 = the number of floored pivots (nothing written, *steps = 0), exactly as
 * lsfm_map_covariance -- LSFM_NOT_CONVERGED is 1 too, so pass `steps` to tell one floored pivot from a refinement that ran out of
 * steps; LSFM_ERR_OOM when the columns of a chunk do not fit the device (24 + 18 n / m doubles per pose scalar and
 * column); LSFM_ERR_ARG for all outputs NULL, k < 1, an index out of range or given twice, and whatever lsfm_map_covariance refuses. */
int lsfm_map_covariance_columns(lsfm_context* ctx, const lsfm_map* map, int mono, const int* poses, int k, double* pose_cols, double* feat_cols,
                                double* joint, int* steps, double* last_corr);
/* measurement entry: the same, and times[4] (may be NULL) = HIP-event ms of the Schur reduction + symbolic analysis, the numeric
 * factorisation, all sweeps and products of the solve and its refinement, the feature part */
int lsfm_map_covariance_columns_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* poses, int k, double* pose_cols, double* feat_cols,
                                      double* joint, int* steps, double* last_corr, double* times);

/* ---- whole columns of Sigma for chosen features, and an exact gate for feature pairs (NO reference counterpart) ----
 * The question "are feature f and feature g the same point?" needs Sigma_d = Var(x_f - x_g) = Sigma_ff + Sigma_gg - Sigma_fg - Sigma_gf
 * and d^2 = (x_f - x_g)^T Sigma_d^-1 (x_f - x_g).  Sigma_fg is off every pattern the library keeps.  Both entries solve three
 * right-hand sides per item against the factor of the camera system S, side by side in chunks of 64 items, by
 * lsfm_map_covariance_columns' sweeps and refinement:
 *     B_a = -sum_(h,s) s W_h V_h^-1 over the item's signed features (f, +1)[, (g, -1)];   X_a = S^-1 B_a
 *     Sigma_{p,a} = X_a rows;   Sigma_{h,a} = s_h V_h^-1 [h in a] - V_h^-1 sum_b W_bh^T X_a[p_b]
 *     a pair:  Sigma_d = V_f^-1 + V_g^-1 + B_a^T X_a -- a sum of positive semi-definite terms, no cancellation of marginals
 * map, mono, the gauge, the argument checks, the lifetime in the context's arenas, the refinement rule and the statuses
 * (LSFM_ERR_NOT_SPD, > 0 floored pivots with nothing written and *steps = 0, LSFM_NOT_CONVERGED with the results written,
 * LSFM_ERR_OOM) are lsfm_map_covariance_columns'; always fp64, always the sparse factorisation.
 *
 * lsfm_map_covariance_feature_columns: Sigma_{.,F} for the k distinct features F = feats[0..k) (indices into the map's feature order).
 *   pose_cols[18 k m]  block Sigma_{p, feats[a]} at pose_cols + 18 (a m + p), row-major 6x3 (Mono: zero rows for the fixed scalars)
 *   feat_cols[9 k n]   block Sigma_{g, feats[a]} at feat_cols + 9 (a n + g), row-major 3x3, the feature's own diagonal block included
 *   joint[3k * 3k]     Sigma_FF, row-major, exactly symmetric by the rule of lsfm_map_covariance_columns' joint
 *   last_corr[k]       per requested feature the largest |delta_c|_inf / |x_c|_inf of the last correction over its three columns
 * LSFM_ERR_ARG for all outputs NULL, k < 1, an index out of range or given twice.
 *
 * lsfm_map_feature_pair_gate: for the K pairs (f, g) = (pairs[2 a], pairs[2 a + 1]), f != g; a feature may occur in several pairs.
 *   d2[K]              d^2 of the pair, x_f - x_g from map->stVal; NaN where Sigma_d has a non-positive Cholesky pivot (the call goes on)
 *   cov_diff[9 K]      Sigma_d, row-major 3x3, exactly symmetric (may be NULL; at least one of d2, cov_diff is not)
 *   last_corr[K]       as above, per pair
 * LSFM_ERR_ARG for all outputs NULL, K < 1, an index out of range or f == g. */
int lsfm_map_covariance_feature_columns(lsfm_context* ctx, const lsfm_map* map, int mono, const int* feats, int k, double* pose_cols, double* feat_cols,
                                        double* joint, int* steps, double* last_corr);
int lsfm_map_feature_pair_gate(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, double* d2, double* cov_diff, int* steps,
                               double* last_corr);
/* measurement entries: the same, and times[4] (may be NULL) = HIP-event ms of the Schur reduction + symbolic analysis, the numeric
 * factorisation, all sweeps and products of the solve and its refinement, the feature part / the gate kernel */
int lsfm_map_covariance_feature_columns_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* feats, int k, double* pose_cols,
                                              double* feat_cols, double* joint, int* steps, double* last_corr, double* times);
int lsfm_map_feature_pair_gate_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, double* d2, double* cov_diff, int* steps,
                                     double* last_corr, double* times);

/* ---- merging feature pairs of a map, with their joint compatibility D^2 (NO reference counterpart) ----
 * out = `map` with x_f = x_g declared for the K pairs (f, g) = (pairs[2 a], pairs[2 a + 1]), indices into the map's feature order, f != g.
 * The pairs partition the features into classes, the connected components of the pair graph (a pair given twice, in either order,
 * or a pair that closes a cycle is fine); a class's representative is its member with the smallest index; output feature c is the
 * c-th representative in ascending order (an untouched feature is a class of one).  With T the expansion x = T y the constrained
 * Gaussian is exact and again a map, because V is block diagonal:
 *     U' = U;   V'_c = sum_{h in c} V_h, members ascending;   W'_{p,c} = sum_{h in c} sum_{blocks (p,h)} W, one block per (pose, class),
 *     ascending pose, its sources added by (member, position in the input);   y^ = argmin_y (x^ - T y)^T I (x^ - T y)
 * (Mono: the gauge scalars of lsfm_solve_mono held at x^'s values).  y^ = y0 + I'^-1 T^T I (x^ - T y0), y0 = x^ with every class at its
 * representative's estimate, through the camera system of the MERGED map: one right-hand side for lsfm_map_covariance_columns' sweeps
 * and refinement, then a back-substitution.  The same solve gives the joint compatibility of all pairs
 *     D^2 = sum_g r_g^T V_g r_g - eta^T delta        (r_g = x^_g - x^_rep over the merged-away features, eta = T^T I r, delta = y^ - y0)
 * = d^T (A Sigma A^T)^-1 d with *dof = 3 (n - n') degrees of freedom; for one pair it is lsfm_map_feature_pair_gate's d^2.
 * out (library-allocated, lsfm_map_release): m, the poses' labels, pose_origin, Ref, FRef, ScaP, Fix, Sign, FScaP, FFix and U / Ui / Uj are
 * the input's, bit for bit; stVal = y^ (a gauge scalar: bit for bit the input's); an output feature has its representative's label;
 * a class of one keeps V and its W run bit for bit (repeated (pose, feature) blocks stay, as in lsfm_map_marginalise), a larger class has
 * one W block per pose.  rep[n] (may be NULL): the output feature of every input feature.  d2, dof, steps, last_corr[1] may be NULL.
 * Bit-reproducible from call to call: the structure, U' V' W', the right-hand side, and D^2 GIVEN the solved delta.  NOT: delta itself
 * (the sweeps add with atomics), and so y^ and the last bits of D^2; the refinement leaves the difference at rounding level.
 * Always fp64 and always the sparse factorisation (lsfm_set_precision / lsfm_set_small_solve do not apply).  The merged map goes
 * through the host between the merging passes and the factorisation in this version.
 * Returns exactly as lsfm_map_covariance_columns: LSFM_OK; LSFM_NOT_CONVERGED (results written); LSFM_ERR_NOT_SPD, and > 0 = floored
 * pivots (out untouched, *steps = 0); LSFM_ERR_OOM; LSFM_ERR_ARG for K < 1, an index out of range, f == g, out == NULL, and whatever
 * lsfm_map_covariance refuses.  Lifetime: works in the context's arenas like lsfm_map_covariance. */
int lsfm_map_merge_features(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, lsfm_map* out, double* d2, int* dof, int* rep,
                            int* steps, double* last_corr);
/* measurement entry: the same, and times[5] (may be NULL) = HIP-event ms of upload + W' / V' passes + the merged map's download | its
 * upload + reduction + analysis + factorisation | right-hand side + sweeps + refinement | back-substitution + D^2 | download */
int lsfm_map_merge_features_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, lsfm_map* out, double* d2, int* dof,
                                  int* rep, int* steps, double* last_corr, double* times);
/* Test entry, NO device needed: the structure of lsfm_map_merge_features from the map's index arrays and the pairs alone (no value is
 * read).  Outputs, each optional:
 *   rep[n]          the output feature of every input feature
 *   photo, feature[cap_w], FBlock[n']   the output's W index arrays
 *   sptr[cap_w + 1], sidx[cap_w]        per output W block its sources (input W blocks) as a CSR, by (member feature, position in the input)
 *   info[8]         { n', nW', classes of more than one, features removed, output blocks with more than one source, 0, 0, 0 }
 *   why[why_cap]    what is wrong, when LSFM_ERR_ARG is returned
 * Call it once with info alone for the sizes (cap_w >= nW' for photo / feature / sptr, >= the input's nW for sidx).  LSFM_ERR_ARG for
 * K < 1, an index out of range, f == g, W not sorted by feature, a cap that is too small. */
int lsfm_merge_structure(const lsfm_map* map, const int* pairs, int K, int* rep, int* photo, int* feature, int* FBlock, int* sptr, int* sidx, int cap_w,
                         int* info, char* why, int why_cap);

/* ---- candidate feature pairs for the gate: a cell search with a sure bound (NO reference counterpart) ----
 * The first stage in front of lsfm_map_feature_pair_gate / lsfm_map_merge_features: from the map alone, every pair f < g of indices into
 * the map's feature order with, d = x_f - x_g from map->stVal,
 *   1. dx^2 + dy^2 + dz^2 <= radius^2 in fp64 (the products and sums rounded one by one, left to right); radius finite and > 0: a
 *      metric cap the caller always gives;
 *   2. only when feat_cov != NULL:  q_fg = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d <= tau, tau finite and > 0.  feat_cov[9 n] is what
 *      lsfm_map_covariance writes (the upper triangle is read); the sum is factored by a 3x3 LDL^T in registers; a pair whose sum has a
 *      pivot that is not > 0 (NaN included) is KEPT, with q = NaN: the call never drops what it cannot bound.
 * For any joint covariance Var(x_f - x_g) + Var(x_f + x_g) = 2 (Sigma_ff + Sigma_gg), hence Var(x_f - x_g) <= 2 (Sigma_ff + Sigma_gg) and
 * q_fg <= d^2_fg, the gate's distance: a pair dropped by 2. is one the gate rejects at tau (under the Mono gauge too: a conditioned
 * covariance is a covariance).  Pairs within 4 ulp of radius^2 or 1e-12 relative of tau may fall on either side.
 * Outputs: pairs[2 cap] sorted by (f, g) ascending; dist2[cap] and q[cap] (each may be NULL; q without feat_cov: LSFM_ERR_ARG); *count =
 * the number found, set even when cap is too small -- the call then returns LSFM_ERR_ARG and writes nothing else (lsfm_map_covariance's
 * nnzb convention); pairs == NULL with cap == 0 is the sizing call (LSFM_OK, *count alone).  n < 2: *count = 0.
 * Bit-reproducible: the same input gives the same pairs in the same order and the same bits of dist2 and q; no value is summed by
 * atomics and a final sort on the unique key (f << 32) | g fixes the order.
 * A uniform grid of cells of edge radius (1 + 2^-20) (21 bits of cell index per axis), a stable radix sort of the features by cell, then
 * one wave per (cell, 64 of its records) against the half neighbourhood, counting and then filling.  The call does no
 * factorisation and reads neither U, W nor V, and needs no `mono`.
 * Returns LSFM_OK; LSFM_ERR_ARG (lsfm_last_error says which; the context stays usable) for radius or tau out of range, a feature
 * coordinate that is not finite (the feature is named), more than 2^21 cells along an axis ("radius too small for the map's extent"),
 * more than 2^31 - 1 candidates ("reduce the radius"), more than 2^25 features, a cap that is too small; LSFM_ERR_OOM when the output does not fit the arenas.
 * Lifetime: works in the context's arenas like lsfm_map_covariance -- a tree's result must be downloaded first. */
int lsfm_map_feature_pair_candidates(lsfm_context* ctx, const lsfm_map* map, const double* feat_cov, double radius, double tau, int* pairs, double* dist2,
                                     double* q, long long cap, long long* count);
/* measurement entry: the same, and times[4] (may be NULL) = HIP-event ms of upload + cell keys | the sort, the records in cell order and
 * the cell table | the counting pass and its scan | the fill pass, the final sort and the download; info[4] (may be NULL) = { occupied
 * cells, features in the fullest cell, pair tests made, candidates } */
int lsfm_map_feature_pair_candidates_timed(lsfm_context* ctx, const lsfm_map* map, const double* feat_cov, double radius, double tau, int* pairs,
                                           double* dist2, double* q, long long cap, long long* count, double* times, long long* info);

/* ---- joint compatibility of gated feature pairs: sequential selection (NO reference counterpart) ----
 * Between lsfm_map_feature_pair_gate, which judges each pair alone, and lsfm_map_merge_features, which reports the joint D^2 of all the
 * pairs it is given: which of the K pairs (f_b, g_b) = (pairs[2 b], pairs[2 b + 1]) are compatible TOGETHER.  With A the 3K x (6m + 3n)
 * matrix of rows e_f - e_g, C = A Sigma A^T and d = A x^ (map->stVal): block C_ba = Sigma_{f_b,a} - Sigma_{g_b,a} from the feature rows of
 * the gate's column group a -- the 3 K columns the gate solves, no others (chunks of 64 groups, lsfm_map_covariance_columns' sweeps and
 * refinement); a diagonal block is the gate's Sigma_d, d2[K] the gate's individual d^2 (NaN as there); C is made exactly symmetric by the
 * rule of `joint` above.  joint_C[(3K)^2] (may be NULL): C, row-major, pairs in input order.
 * order[K] (may be NULL): the processing order, a permutation of 0..K-1.  NULL: ascending d2, ties by input index, NaN last -- a function
 * of the bits of d2 alone.
 * Selection, for b in that order, with Acc the list of the pairs accepted so far:
 *   - f_b and g_b already connected in the graph whose edges are the accepted pairs (a pair given twice, in either order; the side that
 *     closes a cycle): status 2 (implied), delta = 0, nothing is factored.  The test is structural and exact: C_AccAcc is singular exactly
 *     when the rows of A are dependent, i.e. when a pair closes a cycle, so no pivot threshold exists.
 *   - otherwise S = C_bb - C_bAcc C_AccAcc^-1 C_Accb, e = d_b - C_bAcc C_AccAcc^-1 d_Acc, delta = e^T S^-1 e by a 3x3 Cholesky; a pivot that is
 *     not > 0 (NaN included) or a NaN d2: status 0, delta = NaN; status 1 (accepted) iff delta <= tau, else status 0.
 *   *D2 = the sum of delta over the accepted pairs in processing order = d_Acc^T C_AccAcc^-1 d_Acc, with 3 *accepted degrees of freedom:
 *   what lsfm_map_merge_features reports for exactly those pairs.  tau > 0, +inf allowed (every independent pair is accepted).
 * A delta within 1e-6 relative of tau may fall on either side (the sweeps behind C are not bit-reproducible); what follows is then the
 * selection after that decision.  GIVEN the bits of C, d, the order and tau the selection is bit-reproducible: a right-looking blocked
 * Cholesky with rejection on the device, panels of 16 pairs, the trailing update on v_mfma_f64_16x16x4_f64 with one wave per output tile,
 * no floating-point atomics.
 * Outputs: status[K], delta[K] in input order; *accepted, *implied the counts; *steps, last_corr[K] as the gate's; d2, joint_C, last_corr
 * may be NULL.  1 <= K <= LSFM_JOINT_GATE_MAX.
 * Returns as lsfm_map_feature_pair_gate: LSFM_OK; LSFM_NOT_CONVERGED (results written); LSFM_ERR_NOT_SPD, and > 0 = floored pivots (nothing
 * written, *steps = 0); LSFM_ERR_OOM; LSFM_ERR_ARG for K out of range, an index out of range, f == g, an order that is no permutation, tau
 * NaN or <= 0, a required output NULL, and whatever lsfm_map_covariance refuses.  Lifetime: the context's arenas, as the gate. */
#define LSFM_JOINT_GATE_MAX 2048
int lsfm_map_feature_pair_joint_gate(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, const int* order, double tau, int* status,
                                     double* delta, double* d2, double* joint_C, int* accepted, int* implied, double* D2, int* steps, double* last_corr);
/* measurement entry: the same, and times[6] (may be NULL) = HIP-event ms of reduction + analysis | factorisation | sweeps + refinement | the
 * blocks of C | the selection: its kernels, k_jc_permute to the last panel, and nothing else | the downloads (d2, status, delta, joint_C) together
 * with what the host does between them: the order, the endpoint numbering, the selection's device allocations and uploads */
int lsfm_map_feature_pair_joint_gate_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const int* pairs, int K, const int* order, double tau,
                                           int* status, double* delta, double* d2, double* joint_C, int* accepted, int* implied, double* D2, int* steps,
                                           double* last_corr, double* times);
/* Test entry: the selection alone on the caller's matrix.  C[(3K)^2] row-major and symmetric (either triangle of a block pair may be the one read), d[3K], ends[2K] the two
 * endpoints of every pair (any int labels; equal labels are one vertex; ends[2 b] != ends[2 b + 1]), order[K] or NULL (then the individual
 * d^2 = d_b^T C_bb^-1 d_b is taken on the host, NaN where C_bb has a pivot that is not > 0), tau as above.  status[K], delta[K], *D2,
 * *accepted, *implied as above.  Host plumbing around the kernels of the call above; nothing is solved. */
int lsfm_selftest_pair_select(lsfm_context* ctx, int K, const double* C, const double* d, const int* ends, const int* order, double tau, int* status,
                              double* delta, double* D2, int* accepted, int* implied);

/* ---- marginalising features out of a map (NO reference counterpart: the reference keeps every feature to the end) ----
 * out = `map` with every feature f that has drop[f] != 0 (drop[n], one flag per feature in the map's order) marginalised out:
 *     U' = U - sum_{f dropped} W_f V_f^-1 W_f^T
 * exact for a Gaussian, and again a map: V stays block diagonal, the fill lands in U.  The sum is taken by the pieces a tree level
 * reduces its camera system with (V^-1, the pattern of S, K9: fixed-point sums), over the dropped features alone; a kept feature's V
 * is never inverted.  Mono: the rows and columns of the gauge scalars (zero in the map) stay exactly zero; no gauge is applied.
 * The result is canonical and its structure depends on the labels and the flags alone, never on values: poses, their estimates, Ref,
 * FRef, ScaP, Fix, Sign, FScaP, FFix and pose_origin are the input's; the kept features stay in their order with V, W, photo and their
 * estimates bit for bit the input's (repeated (pose, feature) blocks stay as they are), feature[] and FBlock[] renumbered; U' has
 * exactly one block per pose pair (Ui <= Uj), sorted by (Ui, Uj), the diagonal block first and full -- the pairs of U's pattern, the
 * pairs that observe a common dropped feature and every diagonal; a block whose value happens to be zero stays.
 * Dropping nothing gives the canonical form of the same matrix; dropping everything gives n = 0, nW = 0: the pose graph.
 * Entries of U with the same coordinates are summed by atomics: two calls agree to rounding where the input has such duplicates and
 * bit for bit where it has none (the sums over the features are in fixed point and do not depend on their order).
 * Returns LSFM_OK; LSFM_ERR_NOT_SPD when the V block of a dropped feature is not positive definite (out is not touched);
 * LSFM_ERR_ARG for drop == NULL and for what lsfm_map_covariance refuses (W not sorted by feature, a feature without a W block, an
 * index out of range).  out: library-allocated (lsfm_map_release).
 * Lifetime: works in the context's arenas like lsfm_map_covariance -- a tree's result must be downloaded first. */
int lsfm_map_marginalise(lsfm_context* ctx, const lsfm_map* map, const unsigned char* drop, lsfm_map* out);
/* measurement entry: the same, and times[3] (may be NULL) = HIP-event ms of flags + partition of W + V^-1 + pattern, of K9's values,
 * of the emission of U' with the download */
int lsfm_map_marginalise_timed(lsfm_context* ctx, const lsfm_map* map, const unsigned char* drop, lsfm_map* out, double* times);

/* ---- marginalising poses out of a map: key-frame maps (NO reference counterpart) ----
 * out = `map` with every pose p that has keep_pose[p] == 0 (keep_pose[m], one flag per pose in the map's order) marginalised out,
 * together with the features that go with them.  Rules:
 *   gauge     the Ref pose, where it is in the state, must be kept; for a Mono map (mono = 1) the ScaP pose too
 *   features  a feature seen by a dropped pose must be dropped, or the marginal would not be a map (its fill would join a feature
 *             to poses that never saw it).  drop_feat == NULL: exactly those features are dropped.  drop_feat[n] given: the flags
 *             of lsfm_map_marginalise; a kept feature that a dropped pose sees is refused (lsfm_last_error names it), features
 *             beyond those may be dropped as well.
 * Stage A is lsfm_map_marginalise over the dropped features (U1; this version goes through the host between the stages).  Stage B,
 * with D the dropped and K the kept poses:
 *     U'_KK = U1_KK - U1_KD U1_DD^-1 U1_DK
 * exact for a Gaussian.  U1_DD is factored by lsfm_map_covariance's own front end, in the order its symbolic analysis likes; the
 * correction is formed as Y^T Y, Y = L^-1 D^-1/2 P U1_DK from a forward sweep alone (side by side, 32 boundary poses per chunk), on
 * v_mfma_f64_16x16x4_f64 in a fixed order: it inherits the Cauchy-Schwarz bound element by element, which a solve followed by a product
 * does not, and the diagonal blocks come out EXACTLY symmetric.  (The sweeps add with atomics: two calls agree to rounding.)
 * The result is lsfm_map_marginalise's canonical form with the kept poses renumbered in their order, its structure from labels and
 * flags alone: stno / stVal / pose_origin of the kept variables and Ref .. FFix are the input's; the kept features are bit for bit as
 * stage A leaves them, photo[] renumbered; U' has exactly one block per pair (Ui <= Uj), sorted by (Ui, Uj), the diagonal first and
 * full -- the pairs of U1_KK's pattern, every pair of kept poses that border the same connected component of the graph on D, every
 * diagonal; a block that happens to be zero stays.  A Mono map's gauge rows and columns stay exactly zero.  Keeping every pose is
 * lsfm_map_marginalise.
 * Returns LSFM_OK; LSFM_ERR_NOT_SPD (a dropped V, or U1_DD) and > 0 = the number of floored pivots of U1_DD's factor, exactly as
 * lsfm_map_covariance: nothing is written, out is untouched; LSFM_ERR_OOM when the swept columns (36 |D| |Bd| doubles, Bd the kept
 * poses with a block into D) do not fit the device, the message has the size; LSFM_ERR_ARG for keep_pose == NULL, a rule above, and
 * what lsfm_map_marginalise refuses.  out: library-allocated (lsfm_map_release).
 * Lifetime: works in the context's arenas like lsfm_map_covariance -- a tree's result must be downloaded first. */
int lsfm_map_marginalise_poses(lsfm_context* ctx, const lsfm_map* map, int mono, const unsigned char* keep_pose, const unsigned char* drop_feat,
                               lsfm_map* out);
/* measurement entry: the same, and times[5] (may be NULL) = HIP-event ms of stage A with its way through the host, of the structure +
 * the uploads of stage B, of the factorisation (reduction, analysis, numbers), of the right-hand sides + forward sweeps, of the SYRK +
 * the emission of U' with its download; info[8] (may be NULL) = { |D|, |Bd|, connected components of D, blocks of U', chunks, leaf
 * tasks, supernode groups, group levels } (the last three: the factor of U1_DD; 0 when nothing is dropped) */
int lsfm_map_marginalise_poses_timed(lsfm_context* ctx, const lsfm_map* map, int mono, const unsigned char* keep_pose, const unsigned char* drop_feat,
                                     lsfm_map* out, double* times, int* info);
/* Test entry, NO device needed: the structure of lsfm_map_marginalise_poses from the map's labels and the flags alone (the values of
 * `map` are not read; the pattern of U1 is formed on the host: the pairs of U, the pairs of poses that see a common dropped feature,
 * every diagonal).  Outputs, each optional; pose indices are the INPUT map's except in Ui / Uj:
 *   drop[n]     the feature flags stage A runs with
 *   comp[m]     connected component of a dropped pose in the graph of U1_DD, numbered by their smallest pose; -1: kept
 *   nptr[components + 1 <= m + 1], nidx[cap_n]   N(c) as a CSR: the kept poses with a block of U1 into component c, ascending
 *   bd[<= m]    Bd, the union of all N(c), ascending
 *   Ui, Uj[cap_u]   the pattern of U' in the OUTPUT's numbering, sorted
 *   info[8]     { |D|, |Bd|, components, blocks of U', entries of nidx, dropped features, blocks of U1, fill pairs }
 *   why[why_cap]    what is wrong, when LSFM_ERR_ARG is returned
 * Call it once without nidx / Ui / Uj for the sizes.  LSFM_ERR_ARG as lsfm_map_marginalise_poses, and when a cap is too small. */
int lsfm_marg_pose_structure(const lsfm_map* map, int mono, const unsigned char* keep_pose, const unsigned char* drop_feat, unsigned char* drop,
                             int* comp, int* nptr, int* nidx, int cap_n, int* bd, int* Ui, int* Uj, int cap_u, int* info, char* why, int why_cap);

/* Test entry, NO device needed: the structure of the joint system that lsfm_gn_polish[_robust[_features]], lsfm_map[_feature]_chi2 and
 * lsfm_gn_linearise build from the labels and index arrays of the N local maps and the global state x alone (no value is read).
 * want_slots: every map's U range is extended by the correction slots of lsfm_gn_polish_robust_features; want_coalesce: the coalesced
 * form of lsfm_gn_linearise as well.  Outputs, each optional; poses and features are indices into x unless said otherwise:
 *   info[10]      { M, NFG, local poses P, local feature instances FI, NUJ, NWJ, nU', nW', slots, contributors } (NUJ / NWJ: blocks of the
 *                 working form, every map writes its own; nU' / nW': coalesced, 0 without want_coalesce)
 *   map_hubs[3 N] per map { hub columns nh (0: the map's frame is the global one), pose of Ref_k, pose of ScaP_k (-1: none) }
 *   wdst[FI]      first block of a feature instance in the joint W: its nh hub blocks, then its own run
 *   fptrJ[NFG + 1], photoJ[cap_wj]   the joint W: the run of every global feature and the pose of every block
 *   UiJ, UjJ[cap_uj]   the joint U's coordinates
 *   photo, feature[cap_w], FBlock[NFG], Ui, Uj[cap_u]   the coalesced W (sorted by feature, then pose) and U (sorted by (Ui, Uj))
 *   slot_map, slot_a, slot_b, slot_count[cap_s]   per correction slot its map, its LOCAL poses a <= b and the number of its contributors
 *   why[why_cap]  what is wrong, when LSFM_ERR_ARG is returned
 * Call it once with info alone for the sizes.  LSFM_ERR_ARG for what the calls above cannot place, and when a cap is too small. */
int lsfm_gn_structure(const lsfm_map* maps, int N, int type, const lsfm_map* x, int want_slots, int want_coalesce, int* info, int* map_hubs,
                      int* wdst, int* fptrJ, int* photoJ, int cap_wj, int* UiJ, int* UjJ, int cap_uj, int* photo, int* feature, int* FBlock,
                      int cap_w, int* Ui, int* Uj, int cap_u, int* slot_map, int* slot_a, int* slot_b, int* slot_count, int cap_s, char* why,
                      int why_cap);

/* replaces pba_inverseV (Imp.h:213, Imp.cpp:3022-3042): V^-1 of the n 3x3 feature blocks, IN PLACE like the reference's (which
 * inverts V in place and restores it afterwards, Imp.cpp:2210-2212, 2365): the upper triangle of the computed inverse, mirrored.
 * m is unused, as in the reference. */
int lsfm_inverse_v(lsfm_context* ctx, double* V, int m, int n);
/* replaces pba_solveFeatures (Imp.h:214, Imp.cpp:2980-3020), same argument list + context: the features' back-substitution
 * dpb_f = IV_f (eb_f - sum_p W_pf^T dpa_p) for given pose values dpa[6m]; IV[9n] as lsfm_inverse_v leaves it, W[18 nW] sorted by
 * feature with mapCor[f] blocks for feature f (the reference's mapPhoto), photo[nW] their poses.  ea is unused, as in the reference. */
int lsfm_solve_features(lsfm_context* ctx, const double* W, const double* IV, const double* ea, const double* eb, const double* dpa, double* dpb,
                        int m, int n, const int* mapCor, const int* photo);

/* Test / debug entry: the BLOCK PATTERN of the camera system S = U - W V^-1 W^T as the device builds it for a joint map
 * given by its index arrays alone (hash set of the pose pairs that share a feature, plus U's pattern; sorted into block
 * CSR).  It stands where the reference marks a dense m x m byte mask and scans it (Imp.cpp:2131-2205, sba_crsm_* 30-76)
 * and where pba_constructAuxCSS{LM,GN} (Imp.cpp:2529-2549 / 7248-7280) lists the same pattern for cholmod_amd.
 * Upper triangle, row by row, columns ascending, the diagonal block first: rowptr[m + 1], colidx[cap]; *nnzb receives the
 * number of blocks (LSFM_ERR_ARG when cap is too small). */
int lsfm_schur_pattern(lsfm_context* ctx, const int* Ui, const int* Uj, const int* photo, const int* feature, int m, int n, int nU, int nW,
                       int* rowptr, int* colidx, int cap, int* nnzb);

/* Test / measurement entry, NO device needed: the host half of the solver that stands where the reference calls cholmod_amd /
 * cholmod_analyze_p (Imp.cpp:2413, 2440 / 7081, 7112) -- nested-dissection ordering along the join tree + symbolic block
 * Cholesky factorisation of a camera system given by its upper block pattern (rowptr[m + 1], colidx: as lsfm_schur_pattern
 * returns it; every diagonal block present) and, per pose, the index of the local map that brought it (origin[m]; NULL: its
 * position).  Outputs (each optional): perm[m] (new -> old), colptr[m + 1] and rowidx[cap] = block CSC of L in the new
 * numbering (rows ascending, diagonal first); info[8] = { blocks of L, height of the elimination tree, supernode groups, group
 * levels, leaf tasks, poses in separators, 0, 0 }; *avg_ms = wall ms of one analysis, averaged over reps.  Returns LSFM_ERR_ARG
 * when cap is too small (info[0] still holds the size needed). */
int lsfm_symbolic_analyse(int m, const int* rowptr, const int* colidx, const int* origin, int reps, int* perm, int* colptr, int* rowidx,
                          int cap, int* info, double* avg_ms);

/* ---- the scheduler itself ------------------------------------------------------------------------ */
/* replaces lmj_PF3D_Divide_Conquer{Stereo,Mono} (Imp.h:205/220, Imp.cpp:1926-2063 / 6511-6630): hierarchical
 * join of maps[0..N) with the reference's binary-tree order; all joins of one tree level run as ONE batch on
 * the device.  maps are read only.  mono: 0 Stereo, 1 Monocular.  out: library-allocated final map.
 * Two phases so that a caller (bench) can time the device part with inputs resident in HBM:
 *   lsfm_tree_upload   copies the N maps to the device (PCIe), returns a handle
 *   lsfm_tree_run      runs the whole tree on the device (this is the region the reference times)
 *   lsfm_tree_download copies the final map back;  lsfm_tree_free releases the handle.
 * Lifetime rule: the result of lsfm_tree_run lives in the CONTEXT's arenas, which every other compute call on the same
 * context (another tree's upload or run, lsfm_transform_*, lsfm_join_*, lsfm_solve_*) reuses.  Download (or export) a
 * tree before the context does anything else; a download after such a call fails with LSFM_ERR_ARG instead of
 * returning overwritten memory.  The resident INPUT maps of a tree are its own: a tree can be run again at any time. */
typedef struct lsfm_tree lsfm_tree;
int lsfm_tree_upload(lsfm_context* ctx, const lsfm_map* maps, int N, int mono, lsfm_tree** out);
int lsfm_tree_run(lsfm_context* ctx, lsfm_tree* tree, lsfm_stats* stats);
/* on = 1 (default): the final map is re-expressed in its first frame (Imp.cpp:2039-2063).  on = 0: it is left in the
 * frame of its last join -- what the reference's loop holds for an intermediate tree node; used when the tree is a
 * SUBTREE whose root is joined further by another call (multi-GPU sharding). */
int lsfm_tree_set_final_reanchor(lsfm_tree* tree, int on);
/* on = 1 (default): the first lsfm_tree_run of a tree records what depends on its STRUCTURE only (container sizes, block
 * pattern of every Schur system, ordering / elimination tree / supernodes of its factorisation -- the reference repeats
 * that analysis in every join, cholmod_analyze_p, Imp.cpp:2440) and later runs of the same resident tree reuse it: they are
 * enqueued without a host <-> device round trip.  The numeric work of a run is the same either way.  on = 0: every run
 * analyses from scratch (what a first run costs; lsfm_stats.t_total_ms of the first run reports it too). */
int lsfm_tree_set_plans(lsfm_tree* tree, int on);
int lsfm_tree_download(lsfm_context* ctx, lsfm_tree* tree, lsfm_map* out);
/* Level checkpoint / resume (the reference keeps every node of the tree in RAM, m_LMsetS[i] = m_GMapS, Imp.cpp:2032, and
 * writes none).  lsfm_tree_set_stop_level(tree, L > 0): a run ends after L tree levels, leaving the ceil(N / 2^L) nodes of that level
 * -- each with its state, its information matrix, its first frame (FRef / FScaP / FFix) and the origins of its poses, odd-indexed ones
 * not yet taken back to their first frame: exactly what the reference's loop holds at that point (Imp.cpp:1997-2025 re-anchors while it
 * builds the NEXT level).  lsfm_tree_node_count: nodes of the level the last run ended at (1 after a whole tree; 0: not run /
 * overwritten).  lsfm_tree_download_node: node k of it (library-allocated, lsfm_map_release).  The nodes uploaded as the maps of a new
 * tree (lsfm_tree_upload: FRef, FScaP, FFix and pose_origin are honoured) and run to the end give the map the uninterrupted tree
 * gives; lsfm_write_localmap stores a node with a trailer the reference's reader never reaches, lsfm_read_localmap restores it.
 * L = 0 (default): the whole tree. */
int lsfm_tree_set_stop_level(lsfm_tree* tree, int levels);
int lsfm_tree_node_count(lsfm_context* ctx, lsfm_tree* tree);
int lsfm_tree_download_node(lsfm_context* ctx, lsfm_tree* tree, int k, lsfm_map* out);
/* the state vector of the final map alone (no information blocks): *m poses, *n features; stno / stVal (each optional, caller's
 * arrays of cap >= 6 m + 3 n entries) in the layout of lsfm_map -- both NULL: sizes only */
int lsfm_tree_download_state(lsfm_context* ctx, lsfm_tree* tree, int* m, int* n, int* stno, double* stVal, size_t cap);
void lsfm_tree_free(lsfm_context* ctx, lsfm_tree* tree);
/* ---- device-resident hand-off of a tree node (multi-GPU sub-tree sharding; no counterpart in the reference, whose
 * scheduler keeps every node in one process: m_LMsetS[i] = m_GMapS, Imp.cpp:2032) ---------------------------------
 * A finished tree's final map is PACKED into one contiguous device buffer (a 256-byte header, then the arrays
 * with map-local indices, each 256-byte aligned) that the caller owns and may move to another GPU by any means that
 * moves device bytes (RCCL send/recv, hipMemcpyPeer).  lsfm_tree_upload_dev builds the resident inputs of a new tree
 * from N such buffers on this context's device -- no host copy of the arrays, only the N headers are read back.
 *   lsfm_tree_export_size  bytes lsfm_tree_export_dev will write (0: tree not run / overwritten)
 *   lsfm_tree_export_dev   dst: device memory of >= cap bytes, accessible from the context's device
 *   lsfm_packed_size       total bytes of a packed map, from its first LSFM_PACK_HEADER_BYTES (256) bytes copied to the
 *                          host (0: not a pack -- magic, version, sizes or the array offsets stored in it do not fit)
 *   lsfm_tree_upload_dev   packed[k]: device pointer of packed map k (pose origins travel inside the pack) */
size_t lsfm_tree_export_size(lsfm_context* ctx, lsfm_tree* tree);
int lsfm_tree_export_dev(lsfm_context* ctx, lsfm_tree* tree, void* dst, size_t cap);
#define LSFM_PACK_HEADER_BYTES 256
size_t lsfm_packed_size(const void* host_header256);
int lsfm_tree_upload_dev(lsfm_context* ctx, const void* const* packed, int N, int mono, lsfm_tree** out);
/* A REDUCED pack of a finished tree's final map: every feature whose label is not in keep_ids[0..nkeep) marginalised out
 * (lsfm_map_marginalise has the arithmetic and the canonical form), in the format of lsfm_tree_export_dev -- lsfm_packed_size and
 * lsfm_tree_upload_dev take it unchanged.  A node handed on this way no longer carries the features that nothing above it will
 * meet again.  keep_ids: host array, any order, may repeat; ids the map does not hold are ignored; nkeep = 0 (keep_ids may then be
 * NULL) drops every feature.  Device to device: the keep list goes up, the counts come back (one synchronisation for the features
 * and W blocks, one for the pattern of U'), nothing else crosses.  Works in the arenas the result does not occupy and in the scratch
 * arena: the result stays intact -- an lsfm_tree_export_dev or lsfm_tree_download afterwards still gives the full map.
 *   lsfm_tree_export_reduced_size  *bytes = what lsfm_tree_export_reduced_dev will write for the same keep list
 *   lsfm_tree_export_reduced_dev   dst: device memory of >= cap bytes; cap too small: LSFM_ERR_ARG, lsfm_last_error names the size
 * LSFM_ERR_ARG also for a tree that has not been run or whose result was overwritten; LSFM_ERR_NOT_SPD as lsfm_map_marginalise
 * (dst then holds no pack). */
int lsfm_tree_export_reduced_size(lsfm_context* ctx, lsfm_tree* tree, const int* keep_ids, int nkeep, size_t* bytes);
int lsfm_tree_export_reduced_dev(lsfm_context* ctx, lsfm_tree* tree, const int* keep_ids, int nkeep, void* dst, size_t cap);
/* measurement entry: the same, and times[5] (may be NULL) = HIP-event ms of flags + scans + the pattern of U' (with its two read-backs),
 * of the partition pass over W alone, of the per-feature gather + V^-1, of K9's values, of the emission of U' */
int lsfm_tree_export_reduced_dev_timed(lsfm_context* ctx, lsfm_tree* tree, const int* keep_ids, int nkeep, void* dst, size_t cap, double* times);
/* new VALUES for the resident inputs of a tree made by lsfm_tree_upload_dev: N packed maps with the same sizes as the ones
 * it was built from -- the next step of a scheduler that joins the same sub-tree roots again.  Keeps the tree's
 * allocations; its plans (lsfm_tree_set_plans) are kept when the labels and index arrays are the same too (a digest of
 * them is taken on the device at upload and at reload) and dropped otherwise, so that a reload with another structure
 * costs an analysing run instead of a wrong result. */
int lsfm_tree_reload_dev(lsfm_context* ctx, lsfm_tree* tree, const void* const* packed, int N);

/* ---- feature-sharded joins: the top of the tree over several GPUs (no counterpart in the reference; SURVEY 8e "P2") --------
 * The Schur loop (Imp.cpp:2244-2332), the back-substitution (2980-3020) and the feature part of the information transform
 * (1270-1917) are sums over features.  G processes (one per GPU) each hold a SLICE of every map -- all poses and U blocks,
 * the features f with feat_id % G == slice together with their V and W blocks (the same feature of two maps lands in the
 * same slice, so common features still meet in a join) -- and run the SAME tree; three sums per level cross the GPUs:
 *   transform   the pose rows of I C and the hub-hub block (sum over the features of W C_f, C_f^T (I C)_f)
 *   join        S = U - sum_f W V^-1 W^T and E = eP - sum_f W V^-1 eF (U's part is taken by rank 0 alone); in a run that
 *               analyses also the union of the ranks' pose-pair patterns
 *   solve       the pose solution of rank 0 replaces everyone's (the replicated factorisations may differ in the last bit)
 * The library does not link a collective library: the caller hands over device memory `dev_buf` that the reduced arrays
 * live in and a function that sums `count` elements at `offset_bytes` of that buffer over all ranks, in place, ordered after
 * the work already enqueued on `hip_stream` and before the work enqueued on it afterwards (RCCL: ncclAllReduce on that stream;
 * torch.distributed: all_reduce under torch.cuda.ExternalStream(hip_stream)).  Returns 0 on success.  Every rank must call
 * lsfm_tree_run on its slice tree at the same time; the number and sizes of the calls are the same on every rank.
 * Every sum is announced by a sum of 4 int64 at offset 0 of the buffer (the first 256 bytes are the library's): {ranks that have
 * failed, ranks that have not, count, dtype}.  A rank whose run fails between two sums (out of memory, a HIP error, a buffer too
 * small) does not leave its peers waiting: it follows their headers, adds zeros to every sum they make and reaches the exchange of
 * the run's flags with them, where every rank learns of the failure -- lsfm_tree_run then returns an error on EVERY rank
 * (the failed rank its own, the others LSFM_ERR_INTERNAL "another rank ... failed").  Only a failure of `fn` itself (non-zero
 * return: the communicator is gone) cannot be matched; the caller must then tear the job down. */
#define LSFM_DTYPE_F64 0
#define LSFM_DTYPE_I64 1
typedef int (*lsfm_allreduce_fn)(void* user, size_t offset_bytes, size_t count, int dtype, void* hip_stream);
/* fn == NULL: off (the default).  world == 1 is allowed (every sum is then this rank's own: a way to exercise the caller's function) */
int lsfm_tree_set_comm(lsfm_tree* tree, int rank, int world, lsfm_allreduce_fn fn, void* user, void* dev_buf, size_t dev_bytes);
/* Distributes the POSE-side solve of such a tree as well (SURVEY 8e "P2"; the reference factors every camera system in one
 * CHOLMOD call, Imp.cpp:2444-2445).  block_maps = 2^k: rank r joined block r of block_maps consecutive local maps of the whole
 * tree before this tree took over (the pose origins inside the packs say which local map brought a pose).  The nested dissection
 * of every camera system follows the join tree, so a pose whose separator level lies inside one block is only ever coupled to
 * poses of that block and to the separators between blocks: rank r factors the columns of block r's poses and collects their
 * updates of the inter-block separator columns (64-bit fixed-point accumulators); those are summed over the ranks with ONE integer
 * all-reduce -- exact, so every rank holds the same bits -- and every rank factors the separators.  The triangular solves go the
 * same way (own columns, sum of the shared rows, shared columns | shared columns, own columns, sum of the solution).  0 (default):
 * every rank factors everything.  Set on every rank alike, before the first run. */
int lsfm_tree_set_comm_blocks(lsfm_tree* tree, int block_maps);
/* The final map of a finished tree cut into `nslices` packs (same format as lsfm_tree_export_dev: every pack holds ALL poses
 * and U blocks, and the features with feat_id % nslices == slice in their order, with their V and W blocks).
 *   lsfm_tree_export_slice_sizes  bytes of every slice pack, sizes[nslices]
 *   lsfm_tree_export_slice_dev    writes pack `slice` to dst (device memory of >= cap bytes) */
int lsfm_tree_export_slice_sizes(lsfm_context* ctx, lsfm_tree* tree, int nslices, size_t* sizes);
int lsfm_tree_export_slice_dev(lsfm_context* ctx, lsfm_tree* tree, int nslices, int slice, void* dst, size_t cap);

/* convenience: upload + run + download */
int lsfm_divide_conquer(lsfm_context* ctx, const lsfm_map* maps, int N, int mono, lsfm_map* out, lsfm_stats* stats);

/* ---- file formats (Imp.cpp:3044-3132, 6660-6754, 2102-2117, 7876-7967) ---------------------------- */
int lsfm_read_localmap(const char* path, int mono, lsfm_map* out); /* out: library-allocated */
/* dir/localmap_<first>.txt ... localmap_<first+count-1>.txt (the loop around lmj_readInformation*, Imp.cpp:125 naming)
 * on `threads` host threads (<= 0: one per core, at most 32); out[count] library-allocated, filled in order.  On a
 * failure nothing is kept and *failed (optional) is the number of the first file that could not be read. */
int lsfm_read_localmaps(const char* dir, int first, int count, int mono, int threads, lsfm_map* out, int* failed);
/* one map in the local-map text format at %.17g (write -> lsfm_read_localmap is the identity): stores a tree node with its
 * information matrix, which the reference computes (DOC.pdf p.1) but never writes */
int lsfm_write_localmap(const char* path, int mono, const lsfm_map* map);
/* Binary cache of a set of local maps ("optional binary cache with identical semantics" beside the parallel parser of
 * lmj_readInformation*'s files, Imp.cpp:3044-3132 / 6660-6754): one file, the arrays the text reader produced, bit for bit (layout:
 * lsfm_io.cpp).  lsfm_write_mapset writes maps[N] (atomically: a temporary file renamed); lsfm_mapset_info gives N and the type
 * (LSFM_ERR_IO: missing / not a cache); lsfm_read_mapset reads maps first .. first+count-1 (0-based) on `threads` host threads into
 * out[count] (library-allocated; LSFM_ERR_IO and nothing kept when the file is truncated, foreign or of the other map type). */
int lsfm_write_mapset(const char* path, const lsfm_map* maps, int N, int mono);
int lsfm_mapset_info(const char* path, int* N, int* mono);
/* Eight bytes of the cache's header are the writer's: a stamp of what the cache was made from (0: none).  set_to != NULL writes it, stamp
 * (optional) receives what the file holds afterwards.  The command line stamps a cache with a hash of the resolved -path and of the size and
 * modification time of every localmap_k.txt it parsed, and parses again when the files no longer match (advisor, round 4: a cache was trusted
 * whenever it held enough maps of the right type). */
int lsfm_mapset_stamp(const char* path, unsigned long long* stamp, const unsigned long long* set_to);
int lsfm_read_mapset(const char* path, int mono, int first, int count, int threads, lsfm_map* out);
/* -cov / -covf files of the command line: one line per pose (feature) in the order of the pose (feature) file -- ascending id --, the
 * id followed by the 21 (6) upper-triangle entries of its covariance block, row by row, at %.17g.  pose_cov[36 m] / feat_cov[9 n] as
 * lsfm_map_covariance writes them, stno[6m + 3n] the map's labels; a NULL path: that file is not written */
int lsfm_save_covariances(const char* pose_path, const char* feat_path, const int* stno, int m, int n, const double* pose_cov, const double* feat_cov);
/* reads such a file back (k = 6: poses, 3: features): ids[cap], the full symmetric blocks cov[cap k k]; *count = lines read */
int lsfm_read_covariances(const char* path, int k, int* ids, double* cov, int cap, int* count);
/* The -covcols file (lsfm_map_covariance_columns): one line per (requested pose, pose) -- "id_q id_p" and the 36 entries of
 * Sigma_{p,q} row by row at %.17g.  Requested poses in the order given (poses[k]: indices into the map's pose order), within one the
 * poses in the pose file's order (ascending id, the last state entry of an id).  pose_cols[36 k m] as lsfm_map_covariance_columns
 * writes it, stno the map's labels.  Written through a temporary file that is renamed into place. */
int lsfm_save_cov_columns(const char* path, const int* stno, int m, const int* poses, int k, const double* pose_cols);
/* ... and back: ids_q[cap], ids_p[cap], blocks[36 cap]; *count = lines read.  LSFM_ERR_IO for a line cut short, LSFM_ERR_ARG when
 * cap is too small */
int lsfm_read_cov_columns(const char* path, int* ids_q, int* ids_p, double* blocks, int cap, int* count);
/* The -gateout file (lsfm_map_feature_pair_gate): one line per pair in the order given -- "id_f id_g d2" and the six upper entries
 * of Sigma_d row by row at %.17g.  ids[2 K] the labels of the pairs' features, d2[K] and cov_diff[9 K] as the gate writes them.
 * Written through a temporary file that is renamed into place. */
int lsfm_save_pair_gate(const char* path, const int* ids, int K, const double* d2, const double* cov_diff);
/* ... and back: ids_f[cap], ids_g[cap], d2[cap], the full symmetric blocks cov_diff[9 cap]; *count = lines read.  LSFM_ERR_IO for a
 * line cut short, LSFM_ERR_ARG when cap is too small */
int lsfm_read_pair_gate(const char* path, int* ids_f, int* ids_g, double* d2, double* cov_diff, int cap, int* count);
/* The -mergeout file (lsfm_map_merge_features): line 1 "K features_removed dof D2" (D2 at %.17g), then one line per pair in the order
 * given, "id_f id_g id_kept" = ids[3 a .. 3 a + 3): the labels of the pair's features and of the feature both became.  Written through
 * a temporary file that is renamed into place. */
int lsfm_save_merge_report(const char* path, int K, int removed, int dof, double d2, const int* ids);
/* ... and back: the head and ids[3 cap].  LSFM_ERR_IO for a line cut short and for a file with fewer or more lines than its head
 * says, LSFM_ERR_ARG when cap < K */
int lsfm_read_merge_report(const char* path, int* K, int* removed, int* dof, double* d2, int* ids, int cap);
/* The -jgateout file (lsfm_map_feature_pair_joint_gate): line 1 "K accepted implied dof D2" with dof = 3 accepted; then per pair, in the
 * order given, "id_f id_g status d2 delta" at %.17g (NaN is written "nan"); ids[2 K] the labels of the pairs' features.  Written through a
 * temporary file that is renamed into place. */
int lsfm_save_joint_gate(const char* path, const int* ids, int K, const int* status, const double* d2, const double* delta, int accepted, int implied,
                         double D2);
/* ... and back: head[4] = { K, accepted, implied, dof }, *D2, ids[2 cap], status / d2 / delta [cap].  LSFM_ERR_IO for a line cut short, fewer
 * or more lines than the head says, a status outside 0..2, counts in the head that are not those of the lines, dof != 3 accepted;
 * LSFM_ERR_ARG when cap < K (the head is set: call with cap = 0 for the size) */
int lsfm_read_joint_gate(const char* path, int* ids, int* status, double* d2, double* delta, int cap, int* head, double* D2);
/* A pair list, the input format of -gate and -merge and the output of -cand: one line "id_f id_g" per pair, ids[2 K] the labels of the
 * pairs' features, K >= 0.  Written through a temporary file that is renamed into place. */
int lsfm_save_pair_list(const char* path, const int* ids, long long K);
/* ... and back: ids[2 cap]; *count = pairs in the file, set also when cap is too small (LSFM_ERR_ARG; call with cap = 0 for the size).
 * Read as -gate and -merge read it: whitespace-separated ids, two per pair.  LSFM_ERR_IO for an odd number of ids (a line cut short)
 * and for anything that is not an id */
int lsfm_read_pair_list(const char* path, int* ids, long long cap, long long* count);
int lsfm_save_state(const char* path, const double* st, const int* stno, int n);
/* the same state vector as raw doubles (parity tooling): int32 n, int32 0, stno[n] (+ 4 bytes of padding when n is odd),
 * st[n] float64 */
int lsfm_save_state_bin(const char* path, const double* st, const int* stno, int n);
int lsfm_save_poses(const char* pose_path, const char* feat_path, const int* stno, const double* st, int n);

/* ---- stand-alone kernel entry for measurement: y = S x on a symmetric 6x6-block matrix given as upper block
 * CSR (rowptr[m+1], colidx[nnzb], val[nnzb*36], diagonal blocks full); runs `reps` launches and returns the
 * average launch time in ms measured with HIP events on the context's stream. */
int lsfm_spmv_bench(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val,
                    const double* x, double* y, int reps, double* avg_ms, double* algorithmic_bytes);

/* Measurement only: how fast this chip moves nblocks 6x3 blocks of W (144 bytes each) from one array to another with the
 * access pattern of the W kernels -- mode 0: one lane per block, the block as 18 doubles (lane stride 144 bytes, what
 * k_tr_entries / k_join_rhs_w / k_backsub do); mode 1: one lane per block, nine 16-byte loads; mode 2: consecutive lanes
 * on consecutive 16 bytes (the stream copy).  avg_ms over reps launches (HIP events); bytes moved = 2 * 144 * nblocks. */
int lsfm_wstream_bench(lsfm_context* ctx, long long nblocks, int mode, int reps, double* avg_ms);

/* Self-test of the library's own fill and small-copy kernels (they stand where hipMemsetAsync / hipMemcpyAsync stood until round 5:
 * every accumulator of the path is cleared and every index table arrives through them): fills of `cases` pseudo-random (offset, length,
 * byte) triples -- unaligned heads and tails included -- into a guarded buffer, host -> device copies of random lengths through the
 * pinned ring (one by one and as batches), each read back and compared.  Returns LSFM_OK, or LSFM_ERR_INTERNAL with the first
 * mismatch in lsfm_last_error. */
int lsfm_selftest_prims(lsfm_context* ctx, int cases, unsigned seed);

/* Test entry: the per-feature kernel of the level solve (K7) alone, with everything it leaves per feature.  V[9n], eb[3n] in;
 * IV[9n] = V^-1 as lsfm_inverse_v returns it, LY[9n] = (l00 l10 l11 l20 l21 l22 | L^T eb) with V^-1 = L L^T, the record the Schur
 * kernels read (l00 is NaN where V^-1 has no Cholesky factor).  skip: the feature range starts that many doubles into the device
 * arrays (0 or 1: an odd value puts every array 8 bytes off a 16-byte boundary). */
int lsfm_selftest_vinv(lsfm_context* ctx, const double* V, const double* eb, int n, int skip, double* IV, double* LY);

/* Test entry: the device Cholesky factorisation of a camera system (the preconditioner of every level solve, the factor the
 * covariance calls invert; it stands for cholmod_analyze / factorize / solve, Imp.cpp:2380-2449 / 7043-7121) on a matrix of the
 * caller's, and UNREFINED applications of it.  Inside a level solve the refinement tests the true residual and goes on until it
 * passes, so a factor or a triangular sweep that is slightly wrong only costs steps there; here nothing corrects it.  The call runs
 * the solver's own host steps and nothing else: ordering + symbolic analysis, scatter with the power-of-four scaling, numeric
 * factorisation, one application z = (L L^T)^-1 r per right-hand side in the order given; no product with S, no refinement.
 *   m, rowptr[m + 1], colidx, val[36 nnzb]   symmetric positive definite matrix, upper block CSR, every block row starting with its
 *                   diagonal block, stored full (as lsfm_spmv_bench; LSFM_ERR_ARG otherwise)
 *   origin[m]       local map that brought each pose, as lsfm_symbolic_analyse (NULL: its position)
 *   fixed[6 m]      != 0: a scalar held at zero -- its row and column leave the system, z is 0 there (NULL: none)
 *   pose_seg[m], nseg   independent system each pose belongs to, 0 .. nseg - 1
 *   r[nrhs][6 m]    right-hand sides
 *   mode            bit 0: the first right-hand side takes the level solve's route -- its forward substitution rides on the
 *                   factorisation, the application starts behind it; bit 1: the factor is rounded to fp32 before the applications
 *                   (lsfm_set_precision(ctx, 1)'s sweeps)
 * Outputs: z[nrhs][6 m]; dot[nrhs][nseg] = r . z per system; the whole factor in the new numbering (each optional) -- perm[m]
 * (new -> old), colptr[m + 1], rowidx[cap_blocks] (block CSC, rows ascending, diagonal first), L[36 cap_blocks] (row-major 6x6
 * blocks of the factor of the SCALED matrix D P S P^T D), Dinv[36 m] (inverses of the diagonal blocks of L), dscale[6 m] (the
 * diagonal of D, powers of two) --; info[LSFM_SELFTEST_CHOL_INFO] = { blocks of L, leaf tasks, columns in leaf tasks, most deferred
 * update pairs of a leaf column, supernode groups, group levels, group levels launched as the fused panel kernel, group levels
 * launched as panel + rank-update kernels, most rows below a group, the factorisation's error word (1 + block column of a
 * non-positive pivot), pivots held at their lower bound, 0 ... }.
 * Returns LSFM_ERR_ARG when cap_blocks is too small (info[0] still holds the size needed), LSFM_ERR_NOT_SPD for a non-positive
 * pivot (info is complete, the other outputs are what the device left). */
#define LSFM_SELFTEST_CHOL_INFO 16
int lsfm_selftest_chol(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                       const int* pose_seg, int nseg, const double* r, int nrhs, int mode, double* z, double* dot, int* perm, int* colptr, int* rowidx,
                       double* L, double* Dinv, double* dscale, int cap_blocks, int* info);

/* Test entry: the side-by-side triangular sweeps of the columns calls (lsfm_map_covariance_columns, lsfm_map_covariance_feature_columns,
 * lsfm_map_feature_pair_gate, lsfm_map_feature_pair_joint_gate, the first step of lsfm_map_merge_features; the forward half alone:
 * lsfm_map_marginalise_poses) on a matrix of the caller's, UNREFINED, and one launch of their residual product.  In those calls the
 * sweeps are the preconditioner of a refinement against S itself, so a wrong block of a sweep only costs steps there; here nothing
 * corrects it.  The call runs the library's own steps and nothing else: ordering + symbolic analysis, scatter, fp64 factorisation
 * (no fused forward substitution), the group columns merged into the one array of the factor -- as the columns calls' front does --,
 * then  B -> elimination order, scaled -> forward sweep -> [fwd] -> backward sweep -> caller's numbering, scaled -> x.
 *   m, rowptr, colidx, val, origin, fixed   as lsfm_selftest_chol, with the same checks (LSFM_ERR_ARG)
 *   B[6 m][R]       right-hand sides in the caller's numbering, unscaled, the R values of a scalar row contiguous; 1 <= R <= 192,
 *                   need not be a multiple of 6 or 3
 *   X[6 m][R]       (may be NULL) input of the residual product; zero in fixed rows.  Needs y (LSFM_ERR_ARG), and y needs X
 * Outputs, each optional: x[6 m][R] = P^T D (L L^T)^-1 D P B (0 in fixed rows); fwd[6 m][R] = L^-1 D P B, the slab after the forward
 * sweep alone, in elimination order and scaled (what lsfm_map_marginalise_poses consumes); perm[m] (new -> old), dscale[6 m] (the
 * diagonal of D, new numbering, powers of two); y[6 m][R] = B - S X by one launch of the columns calls' residual kernel on the
 * row-sorted list of S's blocks (built whatever lsfm_set_spmv_variant says; the setting is put back); a fixed row of y is B's.
 * The panel version is the context's (lsfm_set_covcols_panel).
 * info[LSFM_SELFTEST_CC_SWEEPS_INFO] = { leaf tasks, supernode groups, group levels, most rows below a group, mask of the run widths
 * that occur among the groups (bit s - 1: a group of s block columns), launches of the leaf-task forward kernel, of the group forward
 * kernel, of the forward panel kernel, of the backward panel kernel, the panel version that ran (1 plain, 2 MFMA), the
 * factorisation's error word, pivots held at their lower bound, 0 ... }.
 * Returns LSFM_ERR_NOT_SPD for a non-positive pivot (info is complete, nothing else is written). */
#define LSFM_SELFTEST_CC_SWEEPS_INFO 16
int lsfm_selftest_cc_sweeps(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin,
                            const unsigned char* fixed, const double* B, int R, const double* X, double* x, double* fwd, int* perm, double* dscale,
                            double* y, int* info);

/* Test entry: the batched coordinate transform (lsfm_transform.hip) on a batch of the caller's, as a tree level calls it -- several
 * maps in one set of launches, each with a target of its own -- where lsfm_transform_stereo / lsfm_transform_mono hand it one map.  The
 * N maps are uploaded as one batch, transformed once, and every map of the result is downloaded; no plans, no hook, no communicator.
 *   tref[N]         id of each map's new reference pose; < 0: the map is passed through (so is one that is in that frame already)
 *   tscap[N], tfix[N]   Mono: id of the new scale pose and the fixed component (ignored for Stereo; may be NULL then)
 *   alias_passthrough   != 0: the transform leaves the W blocks of passed-through maps in its input and records where (as for a
 *                   join that reads them from there); out[b].W of such a map is then filled from the input batch at the recorded
 *                   offset, its photo / feature / FBlock are the transform's
 *   out[N]          library-allocated, each released with lsfm_map_release */
int lsfm_selftest_transform(lsfm_context* ctx, const lsfm_map* maps, int N, int mono, const int* tref, const int* tscap, const int* tfix,
                            int alias_passthrough, lsfm_map* out);

/* Test entry: the one-launch dense path for camera systems of at most 16 poses (lsfm_small.hip, lsfm_set_small_solve) on a batch of
 * the caller's, as a tree level hands it one -- G independent systems back to back in ONE launch, where lsfm_solve_stereo /
 * lsfm_solve_mono hand it a single system.  Host plumbing only: the arrays are uploaded, x_pose / x_feat are filled with the
 * caller's values, the kernel is launched once, the outputs are downloaded; no plans, no run record, no refusal of a bad system
 * (what the kernel reports is returned in status).
 *   pose_off[G + 1], feat_off[G + 1], u_off[G + 1]   first pose / feature / U block of every system; from 0 to M / NF / NU.  Every
 *                   system has at least one pose; one without features or without U blocks is allowed
 *   active[G]       0: a carried system -- its x_pose becomes x0 (0 where x0 is NULL), its x_feat is not touched (NULL: all active)
 *   U, Ui, Uj       [36 NU], [NU]: blocks in the batch's pose numbering, Ui <= Uj, both inside the system the block is listed under
 *   W, photo, feature, nW   [18 nW], [nW]: sorted by feature (the batch's numbering), every feature with at least one block, every
 *                   block's pose inside its feature's system
 *   V [9 NF], ea [6 M], eb [3 NF], x0 [6 M] (may be NULL), fixed [6 M] (may be NULL; != 0: a scalar held at zero, the Mono gauge)
 *   strips          16-row strips of the kernel instance to launch: 1, 2, 3 or 6 (systems of at most 2, 5, 8, 16 poses); 0: the
 *                   instance of the largest system, as a level chooses it
 *   x_pose [6 M], x_feat [3 NF]   in: the prefill; out: the solution where the kernel wrote one
 *   status[2]       systems left above the residual bound or with a V that has no factor; 1 + a system with a non-positive pivot
 *                   (0: none) -- that system's x_pose and x_feat are not written
 *   max_rel         the largest relative residual of the launch
 * LSFM_ERR_ARG, before anything is enqueued, for strips outside { 0, 1, 2, 3, 6 }, a system with more poses than the instance's panel
 * has rows for (6 m > 16 strips), more than 16 poses, offsets that do not tile the batch, or a block of another system's pose. */
int lsfm_selftest_small(lsfm_context* ctx, int G, const int* pose_off, const int* feat_off, const int* u_off, const unsigned char* active,
                        const double* U, const int* Ui, const int* Uj, const double* W, const int* photo, const int* feature, int nW, const double* V,
                        const double* ea, const double* eb, const double* x0, const unsigned char* fixed, int strips, double* x_pose, double* x_feat,
                        int* status, double* max_rel);

#ifdef __cplusplus
}
#endif
#endif
