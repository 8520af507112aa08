// What the single-map calls on a factored camera system share: the front end that checks a map, uploads it, reduces it to the camera
// system and factors that (lsfm_cov.hip: lsfm_map_covariance, lsfm_map_marginalise_poses and, with the row-sorted block list, the
// columns calls and the merge), the device memory of one call, the refined side-by-side solve of a chunk of columns and the one
// driver that walks a list of requested items chunk by chunk (lsfm_covcols.hip: lsfm_map_covariance_columns; lsfm_featcols.hip:
// lsfm_map_covariance_feature_columns, lsfm_map_feature_pair_gate).  lsfm_map_merge_features (lsfm_merge.hip) has one column and a
// body of its own.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "lsfm_chol.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

// device memory of one call beyond the context's arenas (as large as the factor, or as the columns asked for); a refused
// allocation is LSFM_ERR_OOM, and the device's error state is left clean for the calls that follow
struct DevBuf {
	void* p = nullptr;
	~DevBuf() { if (p) (void)hipFree(p); }
	template <class T> T* get(size_t n)
	{
		const hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
		if (e == hipErrorOutOfMemory)
		{
			(void)hipGetLastError();
			p = nullptr;
			throw Error{ LSFM_ERR_OOM, "out of device memory: " + std::to_string(std::max<size_t>(n, 1) * sizeof(T)) + " bytes for the columns of one call" };
		}
		LSFM_CHECK_HIP(e);
		return static_cast<T*>(p);
	}
};

// The factored camera system of a map, in the context's arenas: A = D^-1/2 P S P^T D^-1/2 = L L^T, whole in ch.L / ch.Dinv.
struct CovFront {
	SolveIO io;              // the uploaded map (io.W / io.photo / io.fptr / io.d_fixed: device)
	SchurSystem sy;
	CholDev ch;
	RunStatsDev* d_run = nullptr; // this call's own record (floored pivots)
	hipEvent_t ev[3] = { nullptr, nullptr, nullptr }; // start | reduced + analysed | factored
};
// checks the map's arguments (throws LSFM_ERR_ARG), uploads it (system_fptr / system_upload, lsfm_system.hpp) and runs a tree level's own
// pieces on it, fp64, sparse path: schur_vinv -> build_schur_pattern -> chol_fetch -> build_schur_values -> chol_analyse -> chol_scatter -> chol_factor ->
// chol_merge_groups.  Resets arena 0 and the scratch arena.
void cov_front(lsfm_context* ctx, const lsfm_map* map, bool mono, CovFront& fr);
// the numerical status of the factorisation, read once: throws LSFM_ERR_NOT_SPD, returns the number of floored pivots
int cov_front_status(lsfm_context* ctx, const CovFront& fr);
// the front of a columns call: cov_front with the row-sorted list of S's blocks (fr.sy.gent / goth, which cc_solve_refine's residual
// reads) whatever lsfm_set_spmv_variant says -- the context's setting is put back --, then cov_front_status.  Returns the number of
// floored pivots: 0 = the factor is usable, > 0 = it is of a perturbed S and the caller writes nothing.
int cov_front_rowsorted(lsfm_context* ctx, const lsfm_map* map, bool mono, CovFront& fr);

// The side-by-side triangular sweeps of lsfm_covcols.hip against the factor `ch` (whole in ch.L / ch.Dinv), in place on a slab
// V[6 ch.M][R] in elimination order, R <= 6 CC_KC = 192: V <- L^-1 V, and V <- L^-T V.  lsfm_map_covariance_columns runs one after the
// other; lsfm_map_marginalise_poses the forward one alone.
#define CC_KC 32 /* poses per chunk of columns (lsfm_covcols.hip) */
// count (may be null): the launches of each kernel are added to it (what lsfm_selftest_cc_sweeps reports).
struct CcLaunches { int fwd_tasks = 0, fwd_groups = 0, fwd_panel = 0, bwd_panel = 0, panel = 0; }; // panel: the version that ran, 1 plain, 2 MFMA
void cc_sweep_forward(lsfm_context* ctx, const CholDev& ch, int R, double* V, CcLaunches* count = nullptr);
void cc_sweep_backward(lsfm_context* ctx, const CholDev& ch, int R, double* V, CcLaunches* count = nullptr);

// ---- what lsfm_covcols.hip shares with lsfm_featcols.hip: a chunk of R <= 192 columns X = S^-1 B, solved side by side and refined ----
// the device memory of a columns call, whatever its right-hand sides are: three slabs [6 M][Rmax] and the norms of a refinement step
struct CcWork {
	DevBuf bV, bX, bY, bN;
	double* V = nullptr;  // elimination order, scaled: right-hand side in, solution out
	double* Xo = nullptr; // the solved columns of the chunk in the map's numbering, [6 m][R]
	double* Y = nullptr;  // B, then the residual [6 m][R]; free for the caller's layouts once the chunk is solved
	unsigned long long* norm = nullptr;
	std::vector<double> hn;
	std::vector<double> ratio; // [R] per column the |delta|_inf / |x|_inf of the last correction
	void alloc(int M, int Rmax);
};
struct CcOutcome { int steps = 0; bool undone = false; }; // undone: max_steps steps were taken and the last correction was above rel_tol
// enqueues B, unscaled and in the map's numbering (fixed scalars zero), into B[6 M][R] on the context's stream
using CcRhs = std::function<void(double* B)>;
// wk.Xo = S^-1 B by the sweeps against fr's factor and lsfm_map_covariance_columns' refinement rule (lsfm.h); wk.ratio is filled
CcOutcome cc_solve_refine(lsfm_context* ctx, const CovFront& fr, int R, CcWork& wk, const CcRhs& rhs);
// width = the columns of one requested item, 6 (a pose) or 3 (a feature, or a pair of features):
// out[a][6 m][width] = Xo[row][width a + c], the pose rows of the chunk in the caller's layout
void cc_pose_out(lsfm_context* ctx, int width, int M, int R, const double* Xo, double* out);
// out[a][nrows][3][width]: the feature rows -V^-1 W^T Xo of the features rows[nrows] (rows null: all nrows = n features); grp (width 3,
// may be null): [2 per column group] the features (f, +1), (g, -1 or none: g < 0) the group's columns belong to, whose own rows
// receive +- V^-1 as well
void cc_feat(lsfm_context* ctx, int width, const CovFront& fr, int R, const int* rows, int nrows, const int* grp, const double* Xo, double* out);

// ---- the driver of a columns call: the factored front, then the k requested items in chunks of `chunk`, each R = width kcur columns ----
struct CcCall {
	int k;                // requested items
	int width;            // columns of one item: 6 (a pose) or 3 (a feature, or a pair of features)
	int chunk;            // most items of a chunk: CC_KC poses, 2 CC_KC features or pairs -- 192 columns either way
	size_t extra_doubles; // the caller's own device outputs, for the refusal of a call that does not fit the free device memory
	const char* noun;     // what the items are called in that refusal
};
// The callables, c0 = the chunk's first item, kcur its items:
//   prep    once the factor stands: allocates (and uploads) what the caller's own kernels need on the device
//   rhs     the chunk's right-hand sides, as CcRhs
//   layout  (may be empty) the solved chunk into the caller's layouts, counted with the solve: times[2]
//   emit    the caller's kernels behind the solve: times[3]
//   fetch   downloads what layout and emit wrote; the stream is synchronised after it
// steps_out / last_corr / times as the C ABI's entries have them (lsfm.h; all may be null).  Returns as lsfm_map_covariance_columns: > 0
// floored pivots (nothing was run, *steps_out = 0), LSFM_NOT_CONVERGED, LSFM_OK.
using CcPrep = std::function<void(const CovFront& fr)>;
using CcChunkRhs = std::function<void(int c0, int kcur, int R, const CovFront& fr, double* B)>;
using CcStep = std::function<void(int c0, int kcur, int R, const CovFront& fr, CcWork& wk)>;
using CcFetch = std::function<void(int c0, int kcur, int R, CcWork& wk)>;
int cc_run(lsfm_context* ctx, const lsfm_map* map, bool mono, const CcCall& call, int* steps_out, double* last_corr, double* times, const CcPrep& prep,
           const CcChunkRhs& rhs, const CcStep& layout, const CcStep& emit, const CcFetch& fetch);
// ---- what lsfm_featcols.hip shares with lsfm_jointgate.hip: the column groups of signed features and the gate of a chunk ----
// The column groups of a call on the device, [2 k]: group a = the signed features (f, +1)[, (g, -1); g < 0: none]; rhs() is what the group
// calls hand cc_run as the right-hand sides of a chunk (B = -sum s W V^-1, k_fc_rhs).
struct FcGroups {
	DevBuf buf;
	int* d = nullptr; // [2 k]
	void upload(lsfm_context* ctx, const std::vector<int>& grp);
	const int* of(int c0) const { return d + 2 * (size_t)c0; }
	CcChunkRhs rhs(lsfm_context* ctx) const;
};
// the gate of the chunk's kcur pairs grp[2 kcur] from the solved columns Xo[6 m][R] (k_fc_gate, a wave per pair): d2[kcur] (may be null) =
// dx^T Sigma_d^-1 dx, NaN at a pivot that is not > 0; cov[9 kcur] (may be null) = Sigma_d, exactly symmetric
void fc_gate(lsfm_context* ctx, const CovFront& fr, int R, int kcur, const int* grp, const double* Xo, const double* dx, double* d2, double* cov);

// joint[k width][k width], its chunks' columns in place, made exactly symmetric: block (a, b), a < b, from column b and mirrored; a
// diagonal block (X + X^T) / 2
void symmetrise_joint(double* joint, int k, int width);

} // namespace lsfm
