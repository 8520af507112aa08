// Whole columns of Sigma = I^-1 for a chosen set Q of poses (C ABI: lsfm_map_covariance_columns): every block Sigma_{p,q} and
// Sigma_{f,q}, q in Q, on and off the camera system's pattern.  No reference counterpart.
//
// The camera system is reduced and factored by lsfm_map_covariance's own front end (cov_front, lsfm_cov.hip): A = D^-1/2 P S P^T D^-1/2
// = L L^T, fp64, sparse path.  The 6 |Q| unit right-hand sides are then solved SIDE BY SIDE against that factor and refined in fp64
// against S itself:
//     X = (L L^T)^-1 B,  B = D^-1/2 P E_Q;     Sigma_{.,Q} = P^T D^-1/2 X
//     repeat:  Sigma_{.,Q} += P^T D^-1/2 (L L^T)^-1 D^-1/2 P (E_Q - S Sigma_{.,Q})
// until the correction of every column is below the context's rel_tol relative to the column (or stops falling by half, or max_steps).
// The stopping rule looks at the correction, not at the residual: the entries of S are 1e6..1e8, so the residual of a unit
// right-hand side stalls around 1e-10 while the solution is already two orders better.
//
// Layout: a chunk of R = 6 k_c columns is one array X[6 M][R], the R values of one scalar row contiguous.  A lane owns a COLUMN: the
// lanes of a wave load and store 512 contiguous bytes, the block of L (or S, or W) they multiply with is the same for all of them
// -- its address is uniform -- and every such block is read once per
// sweep for all R columns, where the single-vector kernels (k_chol_fwd/bwd_tasks, k_sn_fwd/bwd, k_spmv_gather) read the whole factor
// per vector.  The sweeps run on CholDev's own schedule: the leaf tasks in one launch, then the supernode-group levels one after the
// other.  A group's dense trapezoid below its run is a matrix product with N = R, in two versions (lsfm_set_covcols_panel): on
// v_mfma_f64_16x16x4_f64 in a launch of its own (k_cc_fwd_panel / k_cc_bwd_panel), or lane per column inside the run's launch.
//
// k_c = CC_KC = 32: one work-group must hold all columns of the chunk (a block of L is then fetched by one work-group only), the
// panel kernels run one wave per 16 columns, twelve waves = CC_MAXT lanes (the plain version: CC_MAXT / 192 = 4 row slices beside
// each other), and the three arrays of a chunk ([6 M][192] doubles: 9 KB per pose each, 97 MB on a 3500-pose map) are what a call
// allocates whatever k is.  Measured: the time of a chunk hardly grows with its columns, so a full chunk is
// the cheapest way through a long list.  More poses go through in chunks.
//
// Not bit-reproducible: the rows of a column's ancestors collect their updates by fp64 atomics from whichever work-group comes
// first.  The refinement takes the difference (a few ulps of the unrefined solve) far below what is asked of the result.
//
// The host side is one driver for every columns call (cc_run, lsfm_cov.hpp): the factored front, the chunks, the refined solve of
// each, the two event brackets and the read-backs; lsfm_map_covariance_columns at the end of this file and the two entries of
// lsfm_featcols.hip are its callers, each a right-hand side, a layout / emit step and the downloads.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lsfm_chol.hpp"
#include "lsfm_cov.hpp"
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_solve.hpp"
#include "lsfm_symbolic.hpp"

namespace lsfm {

namespace {

/* CC_KC = 32 poses per chunk (see above): lsfm_cov.hpp */
#define CC_MAXT 768  /* lanes of a supernode-group work-group: columns x row slices */
#define CC_GK (6 * CHOL_GS) /* most scalar columns of a group's run */
#define CC_PANEL_DEFAULT 2 /* a group's panel product when the context does not say (lsfm_set_covcols_panel): 1 plain, 2 MFMA */
#define CC_GY 32     /* most work-groups that share one group's panel (k_cc_fwd_panel / k_cc_bwd_panel) */
#define CC_EPW 16    /* entries of S's gather list per work-group of the product */
#define CC_FB 8      /* features per work-group of the feature kernel */
#define CC_ROWS 48   /* scalar rows per work-group of k_cc_perm_out */

// a value another wave of the work-group has just added to by atomics (they are performed in L2): read it there
__device__ __forceinline__ double ld_l2(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The unit columns E_Q of the requested poses in the map's numbering, column 6 a + c = scalar c of pose qpose[a] (a fixed scalar's
// column is zero).
__global__ void k_cc_unit(int M, int R, const unsigned char* __restrict__ fixed, const int* __restrict__ qpose, double* __restrict__ out)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)M * 6 * R) return;
	const int r = (int)(idx % R);
	const size_t row = idx / R;
	const int p = (int)(row / 6), q = (int)(row % 6);
	const bool one = p == qpose[r / 6] && q == r % 6 && !(fixed && fixed[row]);
	out[idx] = one ? 1.0 : 0.0;
}

// V = D^-1/2 P Y (a residual into elimination order, scaled like the factor; fixed scalars zero)
__global__ void k_cc_perm_in(int M, int R, const int* __restrict__ perm, const double* __restrict__ dscale, const unsigned char* __restrict__ fixed,
                             const double* __restrict__ Y, double* __restrict__ V)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)M * 6 * R) return;
	const int r = (int)(idx % R);
	const size_t row = idx / R;
	const size_t src = (size_t)perm[row / 6] * 6 + row % 6;
	V[idx] = (fixed && fixed[src]) ? 0.0 : Y[src * R + r] * dscale[row];
}

// Xo (+)= P^T D^-1/2 V in the map's numbering (fixed scalars zero); ADD: the correction of a refinement step, with the largest
// |delta| (norm[r]) and the largest |x| after it (norm[R + r]) of every column (non-negative doubles order like their bit patterns)
template <bool ADD>
__device__ __forceinline__ void cc_perm_out(int M, int R, const int* __restrict__ pinv, const double* __restrict__ dscale, const unsigned char* __restrict__ fixed,
                                            const double* __restrict__ V, double* __restrict__ Xo, unsigned long long* __restrict__ norm)
{
	const int r = threadIdx.x;
	if (r >= R) return;
	const int row0 = blockIdx.x * CC_ROWS, row1 = min(row0 + CC_ROWS, 6 * M);
	double md = 0.0, mx = 0.0;
	for (int row = row0; row < row1; row++)
	{
		const size_t src = (size_t)pinv[row / 6] * 6 + row % 6;
		const double d = (fixed && fixed[row]) ? 0.0 : V[src * R + r] * dscale[src];
		double* o = Xo + (size_t)row * R + r;
		if (ADD)
		{
			const double x = *o + d;
			*o = x;
			md = fmax(md, fabs(d)); mx = fmax(mx, fabs(x));
		}
		else *o = d;
	}
	if (ADD)
	{
		atomicMax(norm + r, (unsigned long long)__double_as_longlong(md));
		atomicMax(norm + R + r, (unsigned long long)__double_as_longlong(mx));
	}
}
__global__ void k_cc_perm_out(int M, int R, const int* __restrict__ pinv, const double* __restrict__ dscale, const unsigned char* __restrict__ fixed,
                              const double* __restrict__ V, double* __restrict__ Xo)
{
	cc_perm_out<false>(M, R, pinv, dscale, fixed, V, Xo, nullptr);
}
__global__ void k_cc_perm_add(int M, int R, const int* __restrict__ pinv, const double* __restrict__ dscale, const unsigned char* __restrict__ fixed,
                              const double* __restrict__ V, double* __restrict__ Xo, unsigned long long* __restrict__ norm)
{
	cc_perm_out<true>(M, R, pinv, dscale, fixed, V, Xo, norm);
}

// ---- the sweeps ---------------------------------------------------------------------------------------------------------------
// One work-group walks a run of columns in elimination order: the columns of a leaf task (GROUP = false: a0 = task_ptr, a1 = task_cols)
// (a2 = col_task) or of a supernode group (GROUP = true: a0 = grp_c0, a1 = grp_s, a2 = grp_nr of the level).  Lane x owns column x of X.
// Forward, column j:   y_j = L_jj^-1 v_j;   v_i -= L_ij y_j for every block below the diagonal.
// Rows inside the run are touched by this work-group alone (a leaf task is a whole sub-tree; the columns of a group's run follow each
// other), and a lane only ever reads what it wrote itself: plain loads and stores, no barrier.  Rows outside (ancestors) collect the
// sums of several work-groups: atomics.  A group's common rows -- the dense 6 nr x 6 s trapezoid below its run -- are a matrix
// product X_rows -= Panel X_run.  own_panel (the plain version): once the run is solved, the row slices (threadIdx.y) take every
// blockDim.y-th block row of the panel, sum over the run's columns in registers and add once per row.  Otherwise the launch has the
// run's lanes only and k_cc_fwd_panel follows it.
template <bool GROUP>
__global__ void __launch_bounds__(CC_MAXT) k_cc_fwd(const int* __restrict__ a0, const int* __restrict__ a1, const int* __restrict__ a2, bool own_panel,
                                                    int R, const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ L,
                                                    const double* __restrict__ Dinv, double* X)
{
	const int r = threadIdx.x;
	const bool on = r < R;
	const int slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y), ns = blockDim.y;
	const int me = blockIdx.x;
	const int b = a0[me]; // first column (group) / first slot of task_cols (task)
	const int nc = GROUP ? a1[me] : a0[me + 1] - b;
	if (slice == 0 && on)
		for (int k = 0; k < nc; k++)
		{
			const int j = GROUP ? b + k : a1[b + k];
			double v[6], y[6];
#pragma unroll
			for (int q = 0; q < 6; q++) v[q] = X[((size_t)j * 6 + q) * R + r];
			const double* D = Dinv + (size_t)j * 36;
#pragma unroll
			for (int c = 0; c < 6; c++)
			{
				double s = 0.0;
#pragma unroll
				for (int q = 0; q <= c; q++) s = fma(D[c * 6 + q], v[q], s);
				y[c] = s;
			}
#pragma unroll
			for (int q = 0; q < 6; q++) X[((size_t)j * 6 + q) * R + r] = y[q];
			const int e0 = colptr[j] + 1, e1 = GROUP ? colptr[j] + (nc - k) : colptr[j + 1]; // (a group: the rows of its own run only)
			for (int en = e0; en < e1; en++)
			{
				const int i = rowidx[en];
				const double* blk = L + (size_t)en * 36;
				double o[6];
#pragma unroll
				for (int rr = 0; rr < 6; rr++)
				{
					double s = 0.0;
#pragma unroll
					for (int q = 0; q < 6; q++) s = fma(blk[rr * 6 + q], y[q], s);
					o[rr] = s;
				}
				double* dst = X + (size_t)i * 6 * R + r;
				if (GROUP || a2[i] == me)
				{
#pragma unroll
					for (int rr = 0; rr < 6; rr++) dst[(size_t)rr * R] -= o[rr];
				}
				else
				{
#pragma unroll
					for (int rr = 0; rr < 6; rr++) atomic_add_f64(dst + (size_t)rr * R, -o[rr]);
				}
			}
		}
	if (!GROUP || !own_panel) return;
	__syncthreads(); // y of the whole run is in X
	if (!on) return;
	const int nr = a2[me], rows0 = colptr[b + nc - 1] + 1;
	for (int i = slice; i < nr; i += ns)
	{
		double o[6] = { 0, 0, 0, 0, 0, 0 };
		for (int t = 0; t < nc; t++)
		{
			const double* blk = L + ((size_t)colptr[b + t] + (nc - t) + i) * 36;
			double y[6];
#pragma unroll
			for (int q = 0; q < 6; q++) y[q] = X[((size_t)(b + t) * 6 + q) * R + r];
#pragma unroll
			for (int rr = 0; rr < 6; rr++)
#pragma unroll
				for (int q = 0; q < 6; q++) o[rr] = fma(blk[rr * 6 + q], y[q], o[rr]);
		}
		double* dst = X + (size_t)rowidx[rows0 + i] * 6 * R + r;
#pragma unroll
		for (int rr = 0; rr < 6; rr++) atomic_add_f64(dst + (size_t)rr * R, -o[rr]);
	}
}

// Backward, column j from the last to the first:   z = y_j - sum_i L_ij^T x_i;   x_j = L_jj^-T z.
// A group first takes the common rows off its whole run, z_run -= Panel^T X_rows: k_cc_bwd_panel in the launch before, or (own_panel)
// the row slices split the panel's block rows and add their parts into the run's rows of X, which nobody else touches in this
// launch; then one slice solves the run.  Every x_i read
// is final: an ancestor's from an earlier launch, a row of the run from this lane itself.
template <bool GROUP>
__global__ void __launch_bounds__(CC_MAXT) k_cc_bwd(const int* __restrict__ a0, const int* __restrict__ a1, const int* __restrict__ a2, bool own_panel,
                                                    int R, const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ L,
                                                    const double* __restrict__ Dinv, double* X)
{
	const int r = threadIdx.x;
	const bool on = r < R;
	const int slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y), ns = blockDim.y;
	const int me = blockIdx.x;
	const int b = a0[me];
	const int nc = GROUP ? a1[me] : a0[me + 1] - b;
	if (GROUP && own_panel)
	{
		const int nr = a2[me], rows0 = colptr[b + nc - 1] + 1;
		if (on && slice < nr)
			for (int t = 0; t < nc; t++)
			{
				double acc[6] = { 0, 0, 0, 0, 0, 0 };
				for (int i = slice; i < nr; i += ns)
				{
					const double* blk = L + ((size_t)colptr[b + t] + (nc - t) + i) * 36;
					const double* src = X + (size_t)rowidx[rows0 + i] * 6 * R + r;
					double x[6];
#pragma unroll
					for (int rr = 0; rr < 6; rr++) x[rr] = src[(size_t)rr * R];
#pragma unroll
					for (int c = 0; c < 6; c++)
#pragma unroll
						for (int rr = 0; rr < 6; rr++) acc[c] = fma(blk[rr * 6 + c], x[rr], acc[c]);
				}
				double* dst = X + (size_t)(b + t) * 6 * R + r;
#pragma unroll
				for (int c = 0; c < 6; c++) atomic_add_f64(dst + (size_t)c * R, -acc[c]);
			}
		__syncthreads();
	}
	if (slice != 0 || !on) return;
	for (int k = nc - 1; k >= 0; k--)
	{
		const int j = GROUP ? b + k : a1[b + k];
		double z[6];
#pragma unroll
		for (int c = 0; c < 6; c++) z[c] = GROUP ? ld_l2(X + ((size_t)j * 6 + c) * R + r) : X[((size_t)j * 6 + c) * R + r];
		const int e0 = colptr[j] + 1, e1 = GROUP ? colptr[j] + (nc - k) : colptr[j + 1];
		for (int en = e0; en < e1; en++)
		{
			const double* blk = L + (size_t)en * 36;
			const double* src = X + (size_t)rowidx[en] * 6 * R + r;
			double x[6];
#pragma unroll
			for (int rr = 0; rr < 6; rr++) x[rr] = src[(size_t)rr * R];
#pragma unroll
			for (int c = 0; c < 6; c++)
#pragma unroll
				for (int rr = 0; rr < 6; rr++) z[c] = fma(-blk[rr * 6 + c], x[rr], z[c]);
		}
		const double* D = Dinv + (size_t)j * 36;
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			double s = 0.0;
#pragma unroll
			for (int q = c; q < 6; q++) s = fma(D[q * 6 + c], z[q], s);
			X[((size_t)j * 6 + c) * R + r] = s;
		}
	}
}

// ---- a group's trapezoid on the matrix cores ------------------------------------------------------------------------------------
// X_rows -= Panel X_run as 16 x 16 tiles of v_mfma_f64_16x16x4_f64 (lane l feeds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]
// and holds C[row (l >> 4) + 4 reg][col l & 15]).  The contraction is over the run's 6 s <= CC_GK scalars: a wave owns 16 columns of
// X and keeps its slice of X_run -- the B operand -- in registers for the whole launch; the work-groups of a group (blockIdx.y) deal
// the panel's 16-row tiles among themselves, and a tile goes through LDS once for all waves.  The tile is full except in the last
// rows of the panel and, for an odd s, the last k step.  Rows of X outside the run: atomics, as in the plain version.
typedef double cc_v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(CC_MAXT) k_cc_fwd_panel(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ grp_nr, int R,
                                                          const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ L, double* X)
{
	__shared__ double As[16][CC_GK + 1];
	const int me = blockIdx.x, b = grp_c0[me], nc = grp_s[me];
	const int K = 6 * nc, NR = 6 * grp_nr[me], ntile = (NR + 15) / 16;
	if ((int)blockIdx.y >= ntile) return;
	const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
	const int col = (tid >> 6) * 16 + (lane & 15);
	const bool cin = col < R;
	double bq[CC_GK / 4];
#pragma unroll
	for (int ks = 0; ks < CC_GK / 4; ks++)
	{
		const int k = 4 * ks + kq;
		bq[ks] = (k < K && cin) ? X[((size_t)b * 6 + k) * R + col] : 0.0;
	}
	const int rows0 = colptr[b + nc - 1] + 1;
	for (int rt = blockIdx.y; rt < ntile; rt += gridDim.y)
	{
		__syncthreads(); // the tile of the round before has been read
		for (int e = tid; e < 16 * CC_GK; e += blockDim.x)
		{
			const int rl = e / CC_GK, k = e - rl * CC_GK, rho = rt * 16 + rl;
			double v = 0.0;
			if (rho < NR && k < K)
			{
				const int i = rho / 6, t = k / 6;
				v = L[((size_t)colptr[b + t] + (nc - t) + i) * 36 + (rho - 6 * i) * 6 + (k - 6 * t)];
			}
			As[rl][k] = v;
		}
		__syncthreads();
		cc_v4d acc = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
		for (int ks = 0; ks < CC_GK / 4; ks++)
			if (4 * ks < K) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[lane & 15][4 * ks + kq], bq[ks], acc, 0, 0, 0);
#pragma unroll
		for (int reg = 0; reg < 4; reg++)
		{
			const int rho = rt * 16 + kq + 4 * reg;
			if (rho < NR && cin) atomic_add_f64(X + ((size_t)rowidx[rows0 + rho / 6] * 6 + rho % 6) * R + col, -acc[reg]);
		}
	}
}

// z_run -= Panel^T X_rows: the contraction is over the panel's 6 nr rows, dealt among the work-groups of a group in chunks of CC_GK; the
// chunk of the panel goes through LDS, the gathered rows of X (final: their groups ran in earlier launches) are the B operand, and
// the up to three 16-row tiles of the run collect over all chunks in registers before they are added to the run's rows of X.
__global__ void __launch_bounds__(CC_MAXT) k_cc_bwd_panel(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ grp_nr, int R,
                                                          const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ L, double* X)
{
	__shared__ double Ps[CC_GK][CC_GK + 1]; // [row of the chunk][scalar of the run]
	const int me = blockIdx.x, b = grp_c0[me], nc = grp_s[me];
	const int K = 6 * nc, NR = 6 * grp_nr[me], nchunk = (NR + CC_GK - 1) / CC_GK;
	if ((int)blockIdx.y >= nchunk) return;
	const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
	const int col = (tid >> 6) * 16 + (lane & 15);
	const bool cin = col < R;
	const int rows0 = colptr[b + nc - 1] + 1;
	cc_v4d acc[CC_GK / 16];
#pragma unroll
	for (int mt = 0; mt < CC_GK / 16; mt++) acc[mt] = (cc_v4d){ 0.0, 0.0, 0.0, 0.0 };
	for (int c = blockIdx.y; c < nchunk; c += gridDim.y)
	{
		const int rho0 = c * CC_GK;
		__syncthreads();
		for (int e = tid; e < CC_GK * CC_GK; e += blockDim.x)
		{
			const int rl = e / CC_GK, k = e - rl * CC_GK, rho = rho0 + rl;
			double v = 0.0;
			if (rho < NR && k < K)
			{
				const int i = rho / 6, t = k / 6;
				v = L[((size_t)colptr[b + t] + (nc - t) + i) * 36 + (rho - 6 * i) * 6 + (k - 6 * t)];
			}
			Ps[rl][k] = v;
		}
		double bq[CC_GK / 4];
#pragma unroll
		for (int ks = 0; ks < CC_GK / 4; ks++)
		{
			const int rho = rho0 + 4 * ks + kq;
			bq[ks] = (rho < NR && cin) ? X[((size_t)rowidx[rows0 + rho / 6] * 6 + rho % 6) * R + col] : 0.0;
		}
		__syncthreads();
#pragma unroll
		for (int ks = 0; ks < CC_GK / 4; ks++)
			if (rho0 + 4 * ks < NR)
			{
#pragma unroll
				for (int mt = 0; mt < CC_GK / 16; mt++)
					if (16 * mt < K) acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ps[4 * ks + kq][16 * mt + (lane & 15)], bq[ks], acc[mt], 0, 0, 0);
			}
	}
#pragma unroll
	for (int mt = 0; mt < CC_GK / 16; mt++)
#pragma unroll
		for (int reg = 0; reg < 4; reg++)
		{
			const int k = 16 * mt + kq + 4 * reg;
			if (k < K && cin) atomic_add_f64(X + ((size_t)b * 6 + k) * R + col, -acc[mt][reg]);
		}
}

// ---- Y -= S Xo for all columns in one pass over S -------------------------------------------------------------------------------
// The multi-column sibling of k_spmv_gather on the same list (both orientations of every block, sorted by the row they add to; the
// holes of the diagonal blocks last): a work-group takes CC_EPW consecutive entries, a lane sums its column over the entries of one
// target row in registers and adds once per row and work-group.  Fixed scalars as there: their rows receive nothing (and Xo is zero
// in them, so their columns give nothing).
__global__ void __launch_bounds__(CC_KC * 6) k_cc_resid(int nent, const unsigned long long* __restrict__ ent, const int* __restrict__ oth,
                                                        const double* __restrict__ S, const unsigned char* __restrict__ fixed, int R,
                                                        const double* __restrict__ Xo, double* __restrict__ Y)
{
	const int r = threadIdx.x;
	if (r >= R) return;
	const int e0 = blockIdx.x * CC_EPW, e1 = min(e0 + CC_EPW, nent);
	int cur = -1;
	double acc[6] = { 0, 0, 0, 0, 0, 0 };
	auto flush = [&]() {
		if (cur < 0) return;
#pragma unroll
		for (int rr = 0; rr < 6; rr++)
			if (!(fixed && fixed[(size_t)cur * 6 + rr])) atomic_add_f64(Y + ((size_t)cur * 6 + rr) * R + r, -acc[rr]);
	};
	for (int e = e0; e < e1; e++)
	{
		const unsigned long long key = ent[e];
		if (key == ~0ull) break; // (the holes are the tail of the list)
		const int row = (int)(key >> 32);
		const unsigned kk = (unsigned)(key & 0xffffffffull);
		if (row != cur)
		{
			flush();
			cur = row;
#pragma unroll
			for (int rr = 0; rr < 6; rr++) acc[rr] = 0.0;
		}
		const double* blk = S + (size_t)(kk >> 1) * 36;
		const double* src = Xo + (size_t)oth[e] * 6 * R + r;
		double x[6];
#pragma unroll
		for (int q = 0; q < 6; q++) x[q] = src[(size_t)q * R];
		if (kk & 1u)
		{
#pragma unroll
			for (int rr = 0; rr < 6; rr++)
#pragma unroll
				for (int q = 0; q < 6; q++) acc[rr] = fma(blk[q * 6 + rr], x[q], acc[rr]);
		}
		else
		{
#pragma unroll
			for (int rr = 0; rr < 6; rr++)
#pragma unroll
				for (int q = 0; q < 6; q++) acc[rr] = fma(blk[rr * 6 + q], x[q], acc[rr]);
		}
	}
	flush();
}

// ---- back to the caller's layouts -----------------------------------------------------------------------------------------------
// CW = the columns of one requested item: 6 (a pose, lsfm_map_covariance_columns) or 3 (a feature or a pair of features,
// lsfm_featcols.hip).  pose_cols of the chunk: out[a][6 m rows][CW] = Xo[row][CW a + c]
template <int CW>
__global__ void k_cc_pose_out(int M, int R, const double* __restrict__ Xo, double* __restrict__ out)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t per = (size_t)M * 6 * CW;
	if (idx >= per * (R / CW)) return;
	const int a = (int)(idx / per);
	const size_t rem = idx - (size_t)a * per;
	out[idx] = Xo[(rem / CW) * R + CW * a + rem % CW];
}
// the rows of all k requested poses (for `joint`): out[6 b + q][R] = Xo[6 qall[b] + q][R]
__global__ void k_cc_rows(int k, int R, const int* __restrict__ qall, const double* __restrict__ Xo, double* __restrict__ out)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)k * 6 * R) return;
	const size_t row = idx / R;
	out[idx] = Xo[((size_t)qall[row / 6] * 6 + row % 6) * R + idx % R];
}

// Sigma_{f,Q} = -V_f^-1 sum_a W_af^T Sigma_{p_a,Q}: one pass over W for all columns.  A work-group takes CC_FB features in turn; the
// feature's run of W blocks and its V^-1 are uniform (broadcast), a lane sums its column.  out[a][NR][3][CW] (feat_cols of the chunk):
// the 3 CW values of one (feature, requested item) are contiguous and consecutive features follow each other.
// rows (may be null: every feature, NR = the map's n): the NR features whose rows are wanted, row i of the output is feature rows[i].
// grp (CW == 3 only, may be null): the signed features (f, +1), (g, -1; g < 0: none) of column group a at grp[2 a], grp[2 a + 1] --
// the columns are then those of I^-1 (e_f - e_g), and the rows of f and g themselves receive the diagonal term +- V^-1.
template <int CW>
__global__ void __launch_bounds__(CC_KC * 6) k_cc_feat(int NR, const int* __restrict__ rows, const int* __restrict__ grp, const int* __restrict__ fptr,
                                                       const int* __restrict__ photo, const double* __restrict__ W, const double* __restrict__ IV, int R,
                                                       const double* __restrict__ Xo, double* __restrict__ out)
{
	const int r = threadIdx.x;
	if (r >= R) return;
	const int i0 = blockIdx.x * CC_FB, i1 = min(i0 + CC_FB, NR);
	const int a = r / CW, c = r - CW * a;
	for (int fi = i0; fi < i1; fi++)
	{
		const int f = rows ? rows[fi] : fi;
		const int w0 = fptr[f], w1 = fptr[f + 1];
		double t[3] = { 0, 0, 0 };
		for (int w = w0; w < w1; w++)
		{
			const double* wb = W + (size_t)w * 18;
			const double* src = Xo + (size_t)photo[w] * 6 * R + r;
#pragma unroll
			for (int q = 0; q < 6; q++)
			{
				const double x = src[(size_t)q * R];
#pragma unroll
				for (int j = 0; j < 3; j++) t[j] = fma(wb[q * 3 + j], x, t[j]);
			}
		}
		const double* iv = IV + (size_t)f * 9;
		double* o = out + ((size_t)a * NR + fi) * (3 * CW) + c;
		double sgn = 0.0;
		if (CW == 3 && grp) sgn = f == grp[2 * a] ? 1.0 : (f == grp[2 * a + 1] ? -1.0 : 0.0);
#pragma unroll
		for (int i = 0; i < 3; i++)
		{
			const double v = -(iv[i * 3] * t[0] + iv[i * 3 + 1] * t[1] + iv[i * 3 + 2] * t[2]);
			o[i * CW] = (CW == 3 && sgn != 0.0) ? sgn * iv[i * 3 + c] + v : v;
		}
	}
}

inline unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

} // namespace

// The two halves of (L L^T)^-1 on a slab V[6 M][R], in place, on CholDev's own schedule (shared with lsfm_marg_poses.hip, which needs
// the forward half alone): the leaf tasks in one launch, then the supernode-group levels one after the other -- backward the other
// way round.
namespace {
struct SweepShape {
	unsigned rp, nsl, pt;
	bool plain;
	SweepShape(const lsfm_context* ctx, int R)
	{
		plain = (ctx->covcols_panel ? ctx->covcols_panel : CC_PANEL_DEFAULT) == 1;
		rp = (unsigned)((R + LSFM_WAVE - 1) / LSFM_WAVE * LSFM_WAVE);
		nsl = plain ? std::min(8u, CC_MAXT / rp) : 1u;
		pt = (unsigned)((R + 15) / 16) * LSFM_WAVE; // a wave per 16 columns (<= CC_MAXT: R <= 6 CC_KC)
	}
};
} // namespace

void cc_sweep_forward(lsfm_context* ctx, const CholDev& ch, int R, double* V, CcLaunches* count)
{
	hipStream_t s = ctx->stream;
	const SweepShape sh(ctx, R);
	const unsigned rp = sh.rp, nsl = sh.nsl, pt = sh.pt;
	const bool plain = sh.plain;
	const int ngl = (int)ch.glevel_ptr.size() - 1;
	if (count) count->panel = plain ? 1 : 2;
	if (ch.ntask0)
	{
		hipLaunchKernelGGL(k_cc_fwd<false>, dim3(ch.ntask0), dim3(rp, 1), 0, s, ch.task_ptr, ch.task_cols, ch.col_task, false, R, ch.colptr, ch.rowidx, ch.L, ch.Dinv, V);
		if (count) count->fwd_tasks++;
	}
	for (int l = 0; l < ngl; l++)
	{
		const int g0 = ch.glevel_ptr[l], ng = ch.glevel_ptr[l + 1] - g0, mnr = ch.glevel_maxnr[l];
		if (!ng) continue;
		hipLaunchKernelGGL(k_cc_fwd<true>, dim3(ng), dim3(rp, nsl), 0, s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, plain, R, ch.colptr, ch.rowidx, ch.L, ch.Dinv, V);
		if (count) count->fwd_groups++;
		if (!plain && mnr > 0)
		{
			hipLaunchKernelGGL(k_cc_fwd_panel, dim3(ng, std::min(CC_GY, (6 * mnr + 15) / 16)), dim3(pt), 0, s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, R, ch.colptr, ch.rowidx, ch.L, V);
			if (count) count->fwd_panel++;
		}
	}
}

void cc_sweep_backward(lsfm_context* ctx, const CholDev& ch, int R, double* V, CcLaunches* count)
{
	hipStream_t s = ctx->stream;
	const SweepShape sh(ctx, R);
	const unsigned rp = sh.rp, nsl = sh.nsl, pt = sh.pt;
	const bool plain = sh.plain;
	const int ngl = (int)ch.glevel_ptr.size() - 1;
	for (int l = ngl - 1; l >= 0; l--)
	{
		const int g0 = ch.glevel_ptr[l], ng = ch.glevel_ptr[l + 1] - g0, mnr = ch.glevel_maxnr[l];
		if (!ng) continue;
		if (!plain && mnr > 0)
		{
			hipLaunchKernelGGL(k_cc_bwd_panel, dim3(ng, std::min(CC_GY, (6 * mnr + CC_GK - 1) / CC_GK)), dim3(pt), 0, s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, R, ch.colptr, ch.rowidx, ch.L, V);
			if (count) count->bwd_panel++;
		}
		hipLaunchKernelGGL(k_cc_bwd<true>, dim3(ng), dim3(rp, nsl), 0, s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, plain, R, ch.colptr, ch.rowidx, ch.L, ch.Dinv, V);
	}
	if (ch.ntask0) hipLaunchKernelGGL(k_cc_bwd<false>, dim3(ch.ntask0), dim3(rp, 1), 0, s, ch.task_ptr, ch.task_cols, (const int*)nullptr, false, R, ch.colptr, ch.rowidx, ch.L, ch.Dinv, V);
}

void CcWork::alloc(int M, int Rmax)
{
	const size_t slab = (size_t)M * 6 * Rmax;
	V = bV.get<double>(slab);
	Xo = bX.get<double>(slab);
	Y = bY.get<double>(slab);
	norm = bN.get<unsigned long long>(2 * (size_t)Rmax);
	hn.assign(2 * (size_t)Rmax, 0.0);
}

// Xo = S^-1 B for the R columns of a chunk: the unrefined solve against the factor, then refinement in fp64 against S itself --
// always one step, then while the corrections are above the tolerance and still halving.  rhs(dst) enqueues B, unscaled and in the
// map's numbering, into dst[6 M][R]: once for the first solve and once per step as the start of Y = B - S Xo.
CcOutcome cc_solve_refine(lsfm_context* ctx, const CovFront& fr, int R, CcWork& wk, const CcRhs& rhs)
{
	const SolveIO& io = fr.io;
	const SchurSystem& sy = fr.sy;
	const CholDev& ch = fr.ch;
	hipStream_t s = ctx->stream;
	const int M = ch.M;
	const unsigned rp = (unsigned)((R + LSFM_WAVE - 1) / LSFM_WAVE * LSFM_WAVE);
	const size_t cells = (size_t)M * 6 * R;
	double *V = wk.V, *Xo = wk.Xo, *Y = wk.Y;
	// (L L^T)^-1 applied to V in place
	auto sweep = [&]() {
		cc_sweep_forward(ctx, ch, R, V);
		cc_sweep_backward(ctx, ch, R, V);
	};
	const double tol = ctx->pcg.rel_tol;
	const int max_steps = std::max(1, ctx->pcg.max_steps);
	// ---- the unrefined solve ----
	rhs(Y);
	hipLaunchKernelGGL(k_cc_perm_in, dim3(blocks_of(cells, 256)), dim3(256), 0, s, M, R, ch.perm, ch.dscale, io.d_fixed, Y, V);
	sweep();
	hipLaunchKernelGGL(k_cc_perm_out, dim3(blocks_of((size_t)M * 6, CC_ROWS)), dim3(rp), 0, s, M, R, ch.pinv, ch.dscale, io.d_fixed, V, Xo);
	// ---- refinement ----
	CcOutcome oc;
	double prev = 0.0;
	std::vector<double>& hn = wk.hn;
	std::vector<double>& ratio = wk.ratio;
	ratio.assign(R, 0.0);
	for (;;)
	{
		rhs(Y);
		hipLaunchKernelGGL(k_cc_resid, dim3(blocks_of((size_t)2 * sy.nnzb, CC_EPW)), dim3(rp), 0, s, 2 * sy.nnzb, sy.gent, sy.goth, sy.S, io.d_fixed, R, Xo, Y);
		hipLaunchKernelGGL(k_cc_perm_in, dim3(blocks_of(cells, 256)), dim3(256), 0, s, M, R, ch.perm, ch.dscale, io.d_fixed, Y, V);
		sweep();
		dev_zero(ctx, wk.norm, 2 * (size_t)R * sizeof(unsigned long long));
		hipLaunchKernelGGL(k_cc_perm_add, dim3(blocks_of((size_t)M * 6, CC_ROWS)), dim3(rp), 0, s, M, R, ch.pinv, ch.dscale, io.d_fixed, V, Xo, wk.norm);
		LSFM_CHECK_HIP(hipGetLastError());
		d2h(ctx, hn.data(), wk.norm, 2 * (size_t)R * sizeof(double)); // (the bit patterns of non-negative doubles)
		oc.steps++;
		double worst = 0.0;
		for (int r = 0; r < R; r++)
		{
			ratio[r] = hn[R + r] > 0.0 ? hn[r] / hn[R + r] : (hn[r] > 0.0 ? INFINITY : 0.0);
			if (!(ratio[r] <= worst)) worst = ratio[r]; // (a NaN counts as the worst)
		}
		if (worst <= tol) break;
		if (oc.steps >= max_steps) { oc.undone = true; break; }
		if (oc.steps > 1 && !(worst <= 0.5 * prev)) break; // as far as fp64 refinement against this factor goes
		prev = worst;
	}
	return oc;
}

// Test entry of the C ABI (lsfm_selftest_cc_sweeps, include/lsfm.h has the arguments): the sweeps above on a caller's matrix with
// nothing behind them -- the front of the Cholesky's own test entry (no fused forward substitution, fp64), chol_merge_groups as in
// cov_front, then cc_solve_refine's unrefined solve with the slab copied out between its halves -- and k_cc_resid once, on the list
// cov_front_rowsorted would have built.  The caller has checked the arguments.
int cc_sweeps_selftest(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                       const double* B, int R, const double* X, double* x, double* fwd, int* perm, double* dscale, double* y, int* info)
{
	if (R < 1 || R > 6 * CC_KC) LSFM_FAIL(LSFM_ERR_ARG, "a chunk has 1 .. " + std::to_string(6 * CC_KC) + " columns");
	const size_t ns = (size_t)m * 6, cells = ns * R;
	SelftestFront fr;
	chol_selftest_front(ctx, m, rowptr, colidx, val, origin, fixed, 3 * cells * sizeof(double) + 4096, -1, nullptr, X != nullptr, nullptr, fr);
	const CholDev& ch = fr.ch;
	const SchurSystem& sy = fr.sy;
	chol_merge_groups(ctx, ch);
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	double *Y = sc.alloc<double>(cells), *V = sc.alloc<double>(cells), *Xo = sc.alloc<double>(cells);
	const unsigned rp = (unsigned)((R + LSFM_WAVE - 1) / LSFM_WAVE * LSFM_WAVE);
	h2d(ctx, Y, B, cells * sizeof(double));
	CcLaunches count;
	hipLaunchKernelGGL(k_cc_perm_in, dim3(blocks_of(cells, 256)), dim3(256), 0, s, m, R, ch.perm, ch.dscale, fr.d_fixed, Y, V);
	cc_sweep_forward(ctx, ch, R, V, &count);
	LSFM_CHECK_HIP(hipGetLastError());
	// the factorisation's status before anything is handed out: the sweeps of a factor that does not exist mean nothing
	RunStatsDev rs;
	d2h(ctx, &rs, fr.d_run, sizeof rs);
	const int chol_err = d2h_int(ctx, ch.d_err);
	if (fwd && !chol_err) d2h(ctx, fwd, V, cells * sizeof(double));
	cc_sweep_backward(ctx, ch, R, V, &count);
	hipLaunchKernelGGL(k_cc_perm_out, dim3(blocks_of(ns, CC_ROWS)), dim3(rp), 0, s, m, R, ch.pinv, ch.dscale, fr.d_fixed, V, Xo);
	LSFM_CHECK_HIP(hipGetLastError());
	std::vector<int> gs(ch.ngroups);
	if (ch.ngroups) d2h_ints(ctx, ch.grp_s, gs.data(), gs.size());
	int widths = 0;
	for (int w : gs) widths |= 1 << (w - 1);
	const int ngl = (int)ch.glevel_ptr.size() - 1;
	info[0] = ch.ntask0; info[1] = ch.ngroups; info[2] = std::max(ngl, 0);
	info[3] = ch.glevel_maxnr.empty() ? 0 : *std::max_element(ch.glevel_maxnr.begin(), ch.glevel_maxnr.end());
	info[4] = widths;
	info[5] = count.fwd_tasks; info[6] = count.fwd_groups; info[7] = count.fwd_panel; info[8] = count.bwd_panel; info[9] = count.panel;
	info[10] = chol_err; info[11] = rs.floored;
	if (chol_err) LSFM_FAIL(LSFM_ERR_NOT_SPD, "the matrix is not positive definite (block column " + std::to_string(chol_err - 1) + " of the factor)");
	if (x) d2h(ctx, x, Xo, cells * sizeof(double));
	if (perm) d2h(ctx, perm, ch.perm, (size_t)m * sizeof(int));
	if (dscale) d2h(ctx, dscale, ch.dscale, ns * sizeof(double));
	if (X)
	{
		// Y = B - S X as a refinement step forms it: Y holds B still (k_cc_perm_in only read it)
		if (!sy.gent) LSFM_FAIL(LSFM_ERR_INTERNAL, "the matrix has no row-sorted block list");
		h2d(ctx, Xo, X, cells * sizeof(double));
		hipLaunchKernelGGL(k_cc_resid, dim3(blocks_of((size_t)2 * sy.nnzb, CC_EPW)), dim3(rp), 0, s, 2 * sy.nnzb, sy.gent, sy.goth, sy.S, fr.d_fixed, R, Xo, Y);
		LSFM_CHECK_HIP(hipGetLastError());
		d2h(ctx, y, Y, cells * sizeof(double));
	}
	return LSFM_OK;
}

void cc_pose_out(lsfm_context* ctx, int width, int M, int R, const double* Xo, double* out)
{
	const dim3 grid(blocks_of((size_t)M * 6 * R, 256)), block(256);
	if (width == 6) hipLaunchKernelGGL(k_cc_pose_out<6>, grid, block, 0, ctx->stream, M, R, Xo, out);
	else hipLaunchKernelGGL(k_cc_pose_out<3>, grid, block, 0, ctx->stream, M, R, Xo, out);
}

void cc_feat(lsfm_context* ctx, int width, const CovFront& fr, int R, const int* rows, int nrows, const int* grp, const double* Xo, double* out)
{
	if (nrows <= 0) return;
	const SolveIO& io = fr.io;
	const dim3 grid(blocks_of(nrows, CC_FB)), block((unsigned)((R + LSFM_WAVE - 1) / LSFM_WAVE * LSFM_WAVE));
	if (width == 6) hipLaunchKernelGGL(k_cc_feat<6>, grid, block, 0, ctx->stream, nrows, rows, (const int*)nullptr, io.fptr, io.photo, io.W, fr.sy.IV, R, Xo, out);
	else hipLaunchKernelGGL(k_cc_feat<3>, grid, block, 0, ctx->stream, nrows, rows, grp, io.fptr, io.photo, io.W, fr.sy.IV, R, Xo, out);
}

int cc_run(lsfm_context* ctx, const lsfm_map* map, bool mono, const CcCall& call, int* steps_out, double* last_corr, double* times, const CcPrep& prep,
           const CcChunkRhs& rhs, const CcStep& layout, const CcStep& emit, const CcFetch& fetch)
{
	const int k = call.k, w = call.width;
	if (steps_out) *steps_out = 0;
	CovFront fr;
	const int floored = cov_front_rowsorted(ctx, map, mono, fr);
	if (floored > 0) return floored; // the factor is of a perturbed S: nothing is written
	hipStream_t s = ctx->stream;
	const int M = fr.ch.M;
	const int kc = std::min(k, call.chunk), Rmax = w * kc;
	{
		const size_t need = (3 * (size_t)M * 6 * Rmax + call.extra_doubles) * sizeof(double);
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b)
			throw Error{ LSFM_ERR_OOM, "out of device memory: the columns of " + std::to_string(kc) + " " + call.noun + " need " + std::to_string(need) + " bytes, " + std::to_string(free_b) + " are free" };
	}
	CcWork wk;
	wk.alloc(M, Rmax);
	prep(fr);
	hipEvent_t ev[3] = { ctx->pool_event(), ctx->pool_event(), ctx->pool_event() };
	int most_steps = 0;
	bool undone = false;
	double t_solve = 0.0, t_emit = 0.0;
	for (int c0 = 0; c0 < k; c0 += kc)
	{
		const int kcur = std::min(kc, k - c0), R = w * kcur;
		LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
		const CcOutcome oc = cc_solve_refine(ctx, fr, R, wk, [&](double* B) { rhs(c0, kcur, R, fr, B); });
		most_steps = std::max(most_steps, oc.steps);
		undone = undone || oc.undone;
		if (last_corr)
			for (int a = 0; a < kcur; a++) last_corr[c0 + a] = *std::max_element(wk.ratio.begin() + w * a, wk.ratio.begin() + w * a + w);
		if (layout) layout(c0, kcur, R, fr, wk);
		LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
		emit(c0, kcur, R, fr, wk);
		LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
		LSFM_CHECK_HIP(hipGetLastError());
		fetch(c0, kcur, R, wk);
		LSFM_CHECK_HIP(hipStreamSynchronize(s));
		t_solve += event_ms(ev[0], ev[1]);
		t_emit += event_ms(ev[1], ev[2]);
	}
	if (steps_out) *steps_out = most_steps;
	if (times)
	{
		times[0] = event_ms(fr.ev[0], fr.ev[1]);
		times[1] = event_ms(fr.ev[1], fr.ev[2]);
		times[2] = t_solve; times[3] = t_emit;
	}
	return undone ? LSFM_NOT_CONVERGED : LSFM_OK;
}

void symmetrise_joint(double* joint, int k, int width)
{
	const size_t w = (size_t)width, N = (size_t)k * w;
	for (size_t i = 0; i < N; i++)
		for (size_t j = i; j < N; j++)
		{
			const double v = i / w == j / w ? 0.5 * (joint[i * N + j] + joint[j * N + i]) : joint[i * N + j];
			joint[i * N + j] = joint[j * N + i] = v;
		}
}

int map_covariance_columns(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* poses, int k, double* pose_cols, double* feat_cols, double* joint,
                           int* steps_out, double* last_corr, double* times)
{
	const int m = map->m, n = map->n;
	{
		std::vector<char> seen(m, 0);
		for (int a = 0; a < k; a++)
		{
			if (poses[a] < 0 || poses[a] >= m) LSFM_FAIL(LSFM_ERR_ARG, "requested pose " + std::to_string(poses[a]) + " is not one of the map's " + std::to_string(m));
			if (seen[poses[a]]) LSFM_FAIL(LSFM_ERR_ARG, "pose " + std::to_string(poses[a]) + " is requested twice");
			seen[poses[a]] = 1;
		}
	}
	hipStream_t s = ctx->stream;
	const int kc = std::min(k, CC_KC);
	const bool want_feat = feat_cols && n;
	const size_t nF = want_feat ? (size_t)n * 18 * kc : 0, nJ = joint ? (size_t)k * 36 * kc : 0;
	DevBuf bF, bJ, bQ;
	double *F = nullptr, *Jd = nullptr; // feat_cols of a chunk | the rows of the k requested poses in a chunk's columns
	int* dq = nullptr;
	std::vector<double> hj(nJ);
	int own_steps = 0;
	int& steps = steps_out ? *steps_out : own_steps; // (> 0: the results were written)
	const int rc = cc_run(ctx, map, mono, CcCall{ k, 6, CC_KC, nF + nJ, "poses" }, &steps, last_corr, times,
		[&](const CovFront&) {
			if (want_feat) F = bF.get<double>(nF);
			if (joint) Jd = bJ.get<double>(nJ);
			dq = bQ.get<int>(k);
			h2d(ctx, dq, poses, (size_t)k * sizeof(int));
		},
		[&](int c0, int, int R, const CovFront& fr, double* B) {
			hipLaunchKernelGGL(k_cc_unit, dim3(blocks_of((size_t)m * 6 * R, 256)), dim3(256), 0, s, m, R, fr.io.d_fixed, dq + c0, B);
		},
		[&](int, int, int R, const CovFront&, CcWork& wk) { // (wk.Y is free once the chunk is solved: the chunk of pose_cols)
			if (pose_cols) cc_pose_out(ctx, 6, m, R, wk.Xo, wk.Y);
			if (joint) hipLaunchKernelGGL(k_cc_rows, dim3(blocks_of((size_t)k * 6 * R, 256)), dim3(256), 0, s, k, R, dq, wk.Xo, Jd);
		},
		[&](int, int, int R, const CovFront& fr, CcWork& wk) {
			if (want_feat) cc_feat(ctx, 6, fr, R, nullptr, n, nullptr, wk.Xo, F);
		},
		[&](int c0, int kcur, int R, CcWork& wk) {
			if (pose_cols) d2h(ctx, pose_cols + (size_t)c0 * m * 36, wk.Y, (size_t)m * 6 * R * sizeof(double));
			if (want_feat) d2h(ctx, feat_cols + (size_t)c0 * n * 18, F, (size_t)kcur * n * 18 * sizeof(double));
			if (!joint) return;
			d2h(ctx, hj.data(), Jd, (size_t)k * 6 * R * sizeof(double));
			for (int row = 0; row < 6 * k; row++) memcpy(&joint[(size_t)row * 6 * k + 6 * c0], &hj[(size_t)row * R], (size_t)R * sizeof(double));
		});
	if (joint && steps > 0) symmetrise_joint(joint, k, 6);
	return rc;
}

} // namespace lsfm
