// The sparse block Cholesky factorisation of a camera system (K10's preconditioner, lsfm_chol.hip): the device layout of the factor and
// the host steps that make and apply it -- shared by the level solve (lsfm_level.hip), the refinement (lsfm_pcg.hip) and the marginal
// covariances (lsfm_cov.hip).
#pragma once
#include <vector>

#include "lsfm_internal.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

// ---------------------------------------------------------------------------------------------------------------
// sparse block Cholesky: device side
// ---------------------------------------------------------------------------------------------------------------
struct CholDev {
	int M = 0, nnzL = 0, nlevels = 0, tail_begin = 0; // columns [tail_begin, M) (in level order) run in one launch
	int* colptr = nullptr;  // [M+1]
	int* rowidx = nullptr;  // [nnzL] ascending inside a column, diagonal first
	int* perm = nullptr;    // [M] new -> old
	int* pinv = nullptr;    // [M] old -> new
	int* order = nullptr;   // [M] columns sorted by elimination-tree level
	std::vector<int> level_ptr; // host: order[level_ptr[l] .. level_ptr[l+1]) = columns of level l (before the tail)
	// tasks: connected pieces of the elimination tree that one work-group walks serially (lsfm_symbolic.cpp).  Only the leaf tasks
	// (task level 0, sub-trees of at most task_x blocks: tasks [0, ntask0), columns task_cols[0 .. ncol0)) are walked as tasks,
	// each whole in LDS (chol_upload_index checks it); the columns above them go by supernode group
	int* task_cols = nullptr;          // [M] columns grouped by task, ascending inside a task
	int* task_ptr = nullptr;           // [ntasks+1] tasks ordered by task level
	int* col_task = nullptr;           // [M] task (position in task_ptr) of a column
	int* col_lpos = nullptr;           // [M] position of a column inside its task
	int* col_nin = nullptr;            // [M] leading rows of a column (below the diagonal) that belong to its own task
	int ntask0 = 0, ncol0 = 0;
	int task0_maxsize = 0; // most columns in a leaf task (LDS of the solve launches)
	int task0_lds = 0;     // dynamic LDS of the factorisation launch (k_chol_factor_level)
	int task0_outer = 0;   // largest number of deferred update pairs of a leaf column (k_chol_update_outer)
	// supernode groups: the columns above the leaf tasks, cut into runs of <= CHOL_GS consecutive columns of one
	// fundamental supernode (same rows below the run), ordered by group level (children before parents)
	int ngroups = 0;
	int *grp_c0 = nullptr, *grp_s = nullptr, *grp_nr = nullptr; // [ngroups] first column, columns, rows below the run
	std::vector<int> glevel_ptr;    // host: groups of level l = [glevel_ptr[l], glevel_ptr[l+1])
	std::vector<int> glevel_maxnr;  // host: most rows below a run of the level
	std::vector<int> glevel_maxs;   // host: most block columns of a run of the level (LDS of k_sn_panel)
	int sn_fused_levels = 0, sn_split_levels = 0; // what the last chol_factor launched: group levels as k_sn_panel<true> / as k_sn_panel<false> + k_sn_syrk
	// distributed factorisation (lsfm_symbolic.hpp): owner of every column (-1: shared), null when off; the shared columns are the
	// last ones, from first_shared on (their blocks: from block shared_blk0 of L on)
	int* col_owner = nullptr;
	int first_shared = 0, shared_blk0 = 0;
	double work_total = 0, work_shared = 0;
	std::vector<char> glevel_owned, glevel_shared;
	int* blob = nullptr;    // all index arrays above are slices of this one allocation
	size_t blob_ints = 0;
	float *Lf = nullptr, *Dinvf = nullptr; // mixed precision: the factor rounded to fp32 for the triangular solves (null: fp64)
	double* wv = nullptr;   // [M*6] forward-solve results of the group columns (lsfm_chol.hip k_sn_fwd / k_sn_bwd)
	double* Lg = nullptr;   // [nnzL*36] the factor of the supernode-group columns (same indexing as L; L keeps their unfactored blocks)
	float* Lgf = nullptr;   // mixed precision: its fp32 copy
	double* L = nullptr;    // [nnzL*36] block values, column major by blocks, each block row-major 6x6
	double* Dinv = nullptr; // [M*36] inverse of the diagonal Cholesky factors (lower triangular)
	double* diag0 = nullptr; // [M*6] diagonal of the scaled S as it was scattered (new numbering): what a pivot of the separators is held against
	double* dscale = nullptr; // [M*6] the scaling D^-1/2 (powers of two; new numbering): right-hand sides enter and solutions leave through it
	int* d_err = nullptr;
};

// Distributed factorisation (feature-sharded tree runs, lsfm_symbolic.hpp col_owner): which of a launch's work-groups take
// part -- the ones whose first column belongs to `want` (a rank's block, or -1: the shared separator columns).  col_owner == null: all.
struct OwnFilter {
	const int* col_owner = nullptr;
	int want = 0;
	__device__ __forceinline__ bool skip(int col) const { return col_owner && col_owner[col] != want; }
};
__device__ __forceinline__ int find_row(const int* __restrict__ rowidx, int lo, int hi, int target)
{
	while (lo < hi) { int mid = (lo + hi) >> 1; if (rowidx[mid] < target) lo = mid + 1; else hi = mid; }
	return lo;
}


struct CholSymbolic; // lsfm_symbolic.hpp
struct CholHostIn {
	std::vector<unsigned long long> keys; // sorted upper pattern of S
	std::vector<int> origin;              // local map that brought each pose
};

// the two small device -> host copies of the analysis (a synchronisation)
void chol_fetch(lsfm_context* ctx, const SchurSystem& sy, const int* d_origin, CholHostIn& in);
// symbolic analysis on the host (lsfm_symbolic.cpp), index arrays to the device, value arrays allocated in ctx->scratch
void chol_analyse(lsfm_context* ctx, const SchurSystem& sy, const CholHostIn& in, CholDev& ch);
// the two halves of chol_analyse's device part, for callers that hold a symbolic factorisation already (a level prepared ahead):
// its index arrays to the device (what a plan keeps); the same + chol_alloc_values
void chol_upload_index(lsfm_context* ctx, const CholSymbolic& sym, CholDev& ch);
void chol_upload_symbolic(lsfm_context* ctx, const CholSymbolic& sym, CholDev& ch);
// the value arrays of a run (ctx->scratch) for index arrays that are in place, ch.L and the error flag ch.d_err zeroed
void chol_alloc_values(lsfm_context* ctx, CholDev& ch);
// the scaled, permuted S into the factor's storage (fixed scalars: identity rows / columns), the scaling to ch.dscale
void chol_scatter(lsfm_context* ctx, const SchurSystem& sy, const unsigned char* fixed, CholDev& ch);
// numeric factorisation: the leaf columns' factor in ch.L, the supernode-group columns' in ch.Lg, every L_jj^-1 in ch.Dinv
void chol_factor(lsfm_context* ctx, const SchurSystem& sy, const unsigned char* fixed, CholDev& ch, double* fwd_v = nullptr);
// the group columns' factor copied into ch.L (a no-op when chol_factor already did it): afterwards ch.L + ch.Dinv hold the whole factor
void chol_merge_groups(lsfm_context* ctx, const CholDev& ch);
// mixed precision: the factor rounded to fp32 (ch.Lf, ch.Lgf, ch.Dinvf, in ctx->scratch), which chol_apply then applies
void chol_round_to_float(lsfm_context* ctx, CholDev& ch);
// v = D^-1/2 P r: a right-hand side into elimination order (what chol_factor's fwd_v and chol_apply's fwd_done expect)
void chol_perm_in(lsfm_context* ctx, const CholDev& ch, const double* r, const unsigned char* fixed, double* v);
// z = (L L^T)^-1 r in the original numbering (v: work vector in elimination order), dot[seg * dot_stride] += r . z per system
void chol_apply(lsfm_context* ctx, const CholDev& ch, const double* r, double* v, double* z, const unsigned char* fixed, const int* pose_seg, double* dot, int dot_stride, bool fwd_done = false);
// the factorisation of this system is distributed over the ranks of a feature-sharded run (CholDev::col_owner)
bool chol_distributed(const lsfm_context* ctx, const CholDev& ch);
// feature-sharded run: one or two host numbers summed over the ranks, in place (a synchronisation)
void comm_sum_host(lsfm_context* ctx, long long* h, int n);
// chol_selftest (test entry lsfm_selftest_chol: the factor of a caller's matrix and unrefined applications of it): lsfm_internal.hpp

// The front the test entries on a caller's matrix share (lsfm_selftest_chol, lsfm_selftest_cc_sweeps): the upper block CSR as a
// SchurSystem on the device and its factor, by chol_analyse -> chol_scatter -> chol_factor with a RunStatsDev of the call's own.
// Resets the scratch arena; what the caller allocates there afterwards follows the factor.
struct SelftestFront {
	SchurSystem sy;                  // M, nnzb, S, rowptr, upper_keys (rowsorted: + the SpMV index with gent / goth)
	CholDev ch;                      // factored; the group columns not merged into ch.L yet
	unsigned char* d_fixed = nullptr; // the caller's fixed[6 m] on the device (null: none)
	RunStatsDev* d_run = nullptr;    // floored pivots
	double* fwd_v = nullptr;         // ride_r given: its forward substitution, as chol_apply's fwd_done expects it
};
// extra_bytes: what the caller will allocate in the scratch arena behind the factor.  *nnzL_out (may be null) = blocks of the factor,
// written before cap_blocks (< 0: no bound) refuses a caller whose arrays are too small.  rowsorted: the row-sorted list of both
// orientations of S's blocks is built whatever lsfm_set_spmv_variant says, as cov_front_rowsorted forces it; the context's setting
// is put back.  ride_r[6 m] (host, may be null): a right-hand side whose forward substitution rides on the factorisation.
void chol_selftest_front(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                         size_t extra_bytes, int cap_blocks, int* nnzL_out, bool rowsorted, const double* ride_r, SelftestFront& fr);

} // namespace lsfm
