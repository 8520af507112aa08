// The sparse 6x6-block Cholesky factorisation of a camera system S (lsfm_chol.hpp): kernels and host steps.  It stands for
// cholmod_analyze / factorize / solve (pba_solveCholmod{LM,GN}, Imp.cpp:2380-2449 / 7043-7121) and is used as the preconditioner
// of the refinement (lsfm_pcg.hip, driven by lsfm_level.hip) and as the factor the marginal covariances invert (lsfm_cov.hip).
//
// Block-Jacobi needs O(10 m) iterations on these matrices (a pose chain of length m plus one dense "hub" row per join of the tree;
// measured 84k iterations without convergence at m = 3499), so the preconditioner is a factorisation of S itself, made cheap by the
// structure of the join tree:
//   * ordering and symbolic analysis on the host (lsfm_symbolic.cpp: nested dissection along the tree, elimination tree, column
//     patterns, leaf tasks, supernode groups) from the block pattern, while the numeric Schur assembly runs on the device;
//   * numeric factorisation on the device in two parts.  Leaf tasks -- sub-trees of the elimination tree small enough for LDS -- are
//     walked whole by one work-group each, all in ONE launch (k_chol_factor_level), their updates into the columns above them in
//     a second (k_chol_update_outer).  The columns above go by supernode group -- a run of <= CHOL_GS columns of one fundamental
//     supernode, a dense trapezoid -- one launch per group level (k_sn_panel<true>; k_sn_panel<false> + k_sn_syrk on tall panels);
//   * triangular solves by the same schedule: k_chol_fwd/bwd_tasks for the leaf tasks, k_sn_fwd/bwd per group level; the first
//     forward substitution of a level rides on the factorisation (chol_factor's fwd_v).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "lsfm_device.hpp"
#include "lsfm_symbolic.hpp"
#include "lsfm_chol.hpp"

namespace lsfm {

// ---------------------------------------------------------------------------------------------------------------
// Scaled matrix, fixed-point accumulators.  The factorisation works on  D^-1/2 (P S P^T) D^-1/2  with D the diagonal of S rounded
// to powers of four: an exact scaling (no rounding: Cholesky commutes with it), after which every diagonal entry lies in
// [1/8, 1) and -- the matrix and all its Schur complements being positive definite -- every entry, and every partial sum of
// the updates  sum_k l_ik l_jk  an entry ever receives (Cauchy-Schwarz over any subset of the columns), lies in (-1, 1).
// The blocks of the supernode-group columns, the ones several work-groups of a launch add to, are therefore kept as 64-bit
// FIXED-POINT numbers in units of 2^-61 while they accumulate: integer atomics are associative, so the sum no longer depends
// on the order the atomics land in (two runs on the same S give the same factor bit for bit; round 3's fp64 atomics made the
// root system of a 16 384-map monocular tree come out indefinite in one run out of fifteen), and it is more accurate than
// the fp64 sum it replaces: every addend is rounded once to 2^-62 of the diagonal, instead of every partial sum to 2^-53 of
// its own size.  The panel kernel converts a block back when it loads it.  Leaf columns (one work-group owns each: no
// atomics) stay doubles.  Right-hand sides enter scaled (k_perm_in) and leave unscaled (k_perm_out_dot).
// ---------------------------------------------------------------------------------------------------------------
#define FX_ONE 0x1p61
#define FX_INV 0x1p-61
__device__ __forceinline__ long long fx_from(double v) { return __double2ll_rn(fmin(fmax(v, -2.0), 2.0) * FX_ONE); }
__device__ __forceinline__ double fx_to(long long a) { return (double)a * FX_INV; }
__device__ __forceinline__ void fx_atomic_sub(double* slot, double t)
{
	// (no return value used: global_atomic_add_u64 without a round trip)
	__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)fx_from(-t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// power of two s with s^2 d in [1/8, 1): the scale of a scalar row / column whose diagonal entry is d
__device__ __forceinline__ int scale_exp(double d)
{
	if (!(d > 0) || !(d < 1e300)) return 0; // (not positive definite: reported by the pivot test)
	return (__builtin_amdgcn_frexp_exp(d) + 1) >> 1;
}

// A (upper blocks of S, old numbering) -> lower blocks of the scaled P S P^T in L's storage (fixed point in the group columns:
// col_task[j] >= ntask0), its diagonal to diag0, the scale factors to dscale
__global__ void k_chol_scatter(int nnzb, const unsigned long long* __restrict__ keys, const double* __restrict__ S, const int* __restrict__ srow,
                               const int* __restrict__ pinv, const int* __restrict__ colptr, const int* __restrict__ rowidx,
                               const unsigned char* __restrict__ fixed, const int* __restrict__ col_task, int ntask0, double* __restrict__ L,
                               double* __restrict__ diag0, double* __restrict__ dscale, const int* __restrict__ col_owner, int rank)
{
	int e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= nnzb) return;
	const unsigned long long key = keys[e];
	const int p = (int)(key >> 32), q = (int)(key & 0xffffffffull);
	int i = pinv[p], j = pinv[q];
	bool tr = false; // stored block is S(p,q); the lower block L(i,j), i >= j, is S(perm i, perm j)
	if (i < j) { int t = i; i = j; j = t; tr = true; }
	const int pos = find_row(rowidx, colptr[j], colptr[j + 1], i);
	const double* s = S + (size_t)e * 36;
	double* d = L + (size_t)pos * 36;
	const int rowp = tr ? q : p, colp = tr ? p : q; // old indices of the block's rows / columns
	// scales from the diagonal blocks of S (the first block of every block row)
	const double* dr = S + (size_t)srow[rowp] * 36;
	const double* dc = S + (size_t)srow[colp] * 36;
	int kr[6], kc[6];
	for (int r = 0; r < 6; r++)
	{
		kr[r] = scale_exp((fixed && fixed[(size_t)rowp * 6 + r]) ? 1.0 : dr[r * 7]);
		kc[r] = scale_exp((fixed && fixed[(size_t)colp * 6 + r]) ? 1.0 : dc[r * 7]);
	}
	const bool fx = col_task[j] >= ntask0;
	// (distributed: a rank starts the columns of its own block from S, rank 0 the shared ones too; everybody else's stay zero --
	// the scaling and the diagonal are everybody's)
	const bool put = !col_owner || col_owner[j] == rank || (col_owner[j] < 0 && rank == 0);
	for (int r = 0; r < 6; r++)
		for (int c = 0; c < 6; c++)
		{
			double v = tr ? s[c * 6 + r] : s[r * 6 + c];
			if (fixed && (fixed[(size_t)rowp * 6 + r] || fixed[(size_t)colp * 6 + c])) v = (rowp == colp && r == c) ? 1.0 : 0.0;
			v = ldexp(v, -(kr[r] + kc[c]));
			if (put)
			{
				if (fx) reinterpret_cast<long long*>(d)[r * 6 + c] = fx_from(v);
				else d[r * 6 + c] = v;
			}
			if (i == j && r == c) { diag0[(size_t)j * 6 + r] = v; dscale[(size_t)j * 6 + r] = ldexp(1.0, -kr[r]); }
		}
}

// pivot block of column j (block c0 of Lb, memory or LDS): L_jj = chol(A_jj) in place, its inverse to Dinv and to sLi
// (LDS, 36 doubles); ends with a barrier
__device__ void chol_pivot(int j, int c0, double* L, double* __restrict__ Dinv, int* err, double* sLi)
{
	const int tid = threadIdx.x;
	if (tid < LSFM_WAVE)
	{
		// 6x6 Cholesky and its inverse by the first wave: lane 6 r + c holds element (r,c), pivots and columns travel
		// by shuffles (one thread doing it alone took ~3 us of the ~5 us column step on the critical path)
		const bool in = tid < 36;
		const int r = in ? tid / 6 : 0, c = in ? tid % 6 : 0;
		double a = in ? L[(size_t)c0 * 36 + tid] : 0.0;
		bool ok = true;
#pragma unroll
		for (int k = 0; k < 6; k++)
		{
			double d = __shfl(a, k * 6 + k, LSFM_WAVE);
			if (!(d > 0)) { ok = false; d = 1.0; }
			const double piv = sqrt(d);
			if (in && c == k) a = (r == k) ? piv : (r > k ? a / piv : a);
			const double lrk = __shfl(a, r * 6 + k, LSFM_WAVE), lck = __shfl(a, c * 6 + k, LSFM_WAVE);
			if (in && r > k && c > k) a -= lrk * lck;
		}
		if (c > r) a = 0.0;
		if (!ok && tid == 0) atomicExch(err, 1 + j);
		if (in) L[(size_t)c0 * 36 + tid] = a;
		// inverse, column `tid` per lane (lanes 0..5): L x = e_tid by forward substitution, L's entries broadcast
		double x[6];
#pragma unroll
		for (int i = 0; i < 6; i++)
		{
			double sacc = (i == tid) ? 1.0 : 0.0;
#pragma unroll
			for (int k = 0; k < i; k++) sacc -= __shfl(a, i * 6 + k, LSFM_WAVE) * x[k];
			x[i] = sacc / __shfl(a, i * 6 + i, LSFM_WAVE);
		}
		if (tid < 6)
		{
#pragma unroll
			for (int i = 0; i < 6; i++)
			{
				const double v = i >= tid ? x[i] : 0.0;
				sLi[i * 6 + tid] = v;
				Dinv[(size_t)j * 36 + i * 6 + tid] = v;
			}
		}
	}
	__syncthreads();
}
// L_ij = A_ij * Li^T for the n blocks below the pivot block c0: one thread per (block, row)
__device__ void chol_scale_column(int c0, int n, double* L, const double* sLi)
{
	for (int w = threadIdx.x; w < n * 6; w += blockDim.x)
	{
		double* blk = L + (size_t)(c0 + 1 + w / 6) * 36 + (w % 6) * 6;
		double a[6], o[6];
		for (int k = 0; k < 6; k++) a[k] = blk[k];
		for (int c = 0; c < 6; c++)
		{
			double s = 0;
			for (int k = 0; k <= c; k++) s = fma(a[k], sLi[c * 6 + k], s);
			o[c] = s;
		}
		for (int k = 0; k < 6; k++) blk[k] = o[k];
	}
}
// the deferred updates of leaf column j: the pairs of its blocks a >= b >= m (m: its rows inside its own task, which the LDS walk
// updated) -- targets in columns outside the task, nobody inside the task waits for them.  Other columns
// update the same blocks, so these are atomics -- made contiguous: every lane parks its 6x6 product in LDS and the
// work-group adds block after block with consecutive lanes on consecutive doubles (one lane per block scatters 64
// rows per wave instruction: ~0.1 TB/s)
#define CHOL_OUT_THREADS 128
__device__ void chol_column_update_outer(int j, int m, const int* __restrict__ colptr, const int* __restrict__ rowidx, double* __restrict__ L, int first, int stride)
{
	__shared__ double sT[CHOL_OUT_THREADS * 37];
	__shared__ int spos[CHOL_OUT_THREADS];
	const int c0 = colptr[j], n = colptr[j + 1] - c0 - 1 - m;
	const int npairs = n * (n + 1) / 2;
	const int tid = threadIdx.x;
	for (int base = first; base < npairs; base += stride)
	{
		const int pr = base + tid;
		int pos = -1;
		if (pr < npairs)
		{
			int a = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
			while (a * (a + 1) / 2 > pr) a--;
			while ((a + 1) * (a + 2) / 2 <= pr) a++;
			const int b = pr - a * (a + 1) / 2 + m;
			a += m;
			const int ra = rowidx[c0 + 1 + a], rb = rowidx[c0 + 1 + b];
			double La[36], Lb[36], T[36];
			ld<36>(La, L + (size_t)(c0 + 1 + a) * 36);
			ld<36>(Lb, L + (size_t)(c0 + 1 + b) * 36);
			mmt<6, 6, 6, false>(La, Lb, T);
			const int cb = colptr[rb], nb = colptr[rb + 1] - cb;
			pos = cb + (a - b);
			if (!(a - b < nb && rowidx[pos] == ra)) pos = find_row(rowidx, cb, cb + nb, ra);
			for (int q = 0; q < 36; q++) sT[tid * 37 + q] = T[q];
		}
		spos[tid] = pos;
		__syncthreads();
		for (int idx = tid; idx < CHOL_OUT_THREADS * 36; idx += CHOL_OUT_THREADS)
		{
			const int p = idx / 36, q = idx - p * 36;
			const int ps = spos[p];
			if (ps >= 0) fx_atomic_sub(L + (size_t)ps * 36 + q, sT[p * 37 + q]); // (targets are supernode-group columns: fixed point)
		}
		__syncthreads();
	}
}

// the deferred updates of the leaf tasks, into the columns above them: one column per blockIdx.x, pairs split over blockIdx.y
__global__ void __launch_bounds__(CHOL_OUT_THREADS) k_chol_update_outer(const int* __restrict__ cols, const int* __restrict__ col_nin,
                                                                         const int* __restrict__ colptr, const int* __restrict__ rowidx,
                                                                         double* __restrict__ L, OwnFilter of)
{
	const int j = cols[blockIdx.x];
	if (of.skip(j)) return;
	chol_column_update_outer(j, col_nin[j], colptr, rowidx, L, blockIdx.y * CHOL_OUT_THREADS, gridDim.y * CHOL_OUT_THREADS);
}
// Triangular solves by task.  The entries of v that belong to the task's own columns live in LDS while the work-group
// walks the task: a column step inside a task then costs LDS latency instead of a global atomic + fence round trip
// (measured 2.7 us per step, the critical path of the whole solve).  Rows outside the task (ancestors) are updated /
// read in global memory; nobody inside the task reads them.
// LDS per task column (CHOL_TASK_LDS_PER_COL, lsfm_symbolic.hpp): its slice of v (6), the inverse pivot block (36) and three
// ints (column, first block, count): everything a column step needs except the sub-diagonal blocks themselves is fetched side
// by side before the walk
template <class FT>
__device__ __forceinline__ void chol_task_stage(int b, int e, const int* __restrict__ task_cols, const int* __restrict__ colptr,
                                                const FT* __restrict__ Dinv, const double* __restrict__ v, double* lv, double* sD, int* sj,
                                                int* sc0, int* sn)
{
	const int tid = threadIdx.x, nt = blockDim.x, nc = e - b;
	for (int q = tid; q < nc; q += nt)
	{
		const int j = task_cols[b + q];
		sj[q] = j;
		const int c0 = colptr[j];
		sc0[q] = c0; sn[q] = colptr[j + 1] - c0 - 1;
	}
	for (int q = tid; q < nc * 6; q += nt) lv[q] = v[(size_t)task_cols[b + q / 6] * 6 + q % 6];
	for (int q = tid; q < nc * 36; q += nt) sD[q] = (double)Dinv[(size_t)task_cols[b + q / 36] * 36 + q % 36];
	__syncthreads();
}
template <class FT>
__global__ void __launch_bounds__(256) k_chol_fwd_tasks(const int* __restrict__ task_ptr, const int* __restrict__ task_cols,
                                                         const int* __restrict__ col_task, const int* __restrict__ col_lpos, int task0,
                                                         const int* __restrict__ colptr, const int* __restrict__ rowidx, const FT* __restrict__ L,
                                                         const FT* __restrict__ Dinv, double* __restrict__ v, OwnFilter of)
{
	extern __shared__ double lds[];
	__shared__ double sy[6];
	const int b = task_ptr[blockIdx.x], e = task_ptr[blockIdx.x + 1], me = task0 + blockIdx.x, nc = e - b;
	if (of.skip(task_cols[b])) return;
	const int tid = threadIdx.x, nt = blockDim.x;
	double* lv = lds;
	double* sD = lds + 6 * nc;
	int* sj = reinterpret_cast<int*>(sD + 36 * nc);
	int *sc0 = sj + nc, *sn = sc0 + nc;
	chol_task_stage(b, e, task_cols, colptr, Dinv, v, lv, sD, sj, sc0, sn);
	for (int k = 0; k < nc; k++)
	{
		const int c0 = sc0[k], n = sn[k];
		if (tid < 6)
		{
			const double* Li = sD + k * 36;
			double s = 0;
			for (int q = 0; q <= tid; q++) s = fma(Li[tid * 6 + q], lv[k * 6 + q], s);
			sy[tid] = s;
		}
		__syncthreads();
		if (tid < 6) lv[k * 6 + tid] = sy[tid];
		for (int w = tid; w < n * 6; w += nt)
		{
			const int en = c0 + 1 + w / 6, r = w % 6;
			const FT* blk = L + (size_t)en * 36 + r * 6;
			double s = 0;
			for (int q = 0; q < 6; q++) s = fma((double)blk[q], sy[q], s);
			const int i = rowidx[en];
			if (col_task[i] == me) lds_add_f64(&lv[col_lpos[i] * 6 + r], -s);
			else atomic_add_f64(v + (size_t)i * 6 + r, -s);
		}
		__syncthreads();
	}
	for (int q = tid; q < nc * 6; q += nt) v[(size_t)sj[q / 6] * 6 + q % 6] = lv[q];
}
template <class FT>
__global__ void __launch_bounds__(256) k_chol_bwd_tasks(const int* __restrict__ task_ptr, const int* __restrict__ task_cols,
                                                         const int* __restrict__ col_task, const int* __restrict__ col_lpos, int task0,
                                                         const int* __restrict__ colptr, const int* __restrict__ rowidx, const FT* __restrict__ L,
                                                         const FT* __restrict__ Dinv, double* __restrict__ v, OwnFilter of)
{
	extern __shared__ double lds[];
	__shared__ double red[256];
	__shared__ double ss[6];
	const int b = task_ptr[blockIdx.x], e = task_ptr[blockIdx.x + 1], me = task0 + blockIdx.x, nc = e - b;
	if (of.skip(task_cols[b])) return;
	const int tid = threadIdx.x, nt = blockDim.x;
	const int c = tid % 6, g = tid / 6, ng = nt / 6;
	double* lv = lds;
	double* sD = lds + 6 * nc;
	int* sj = reinterpret_cast<int*>(sD + 36 * nc);
	int *sc0 = sj + nc, *sn = sc0 + nc;
	chol_task_stage(b, e, task_cols, colptr, Dinv, v, lv, sD, sj, sc0, sn);
	for (int k = nc - 1; k >= 0; k--)
	{
		const int c0 = sc0[k], n = sn[k];
		double s = 0;
		if (g < ng)
			for (int en = g; en < n; en += ng)
			{
				const FT* blk = L + (size_t)(c0 + 1 + en) * 36;
				const int i = rowidx[c0 + 1 + en];
				if (col_task[i] == me)
				{
					const double* xi = &lv[col_lpos[i] * 6];
					for (int r = 0; r < 6; r++) s = fma((double)blk[r * 6 + c], xi[r], s);
				}
				else
				{
					const double* xi = v + (size_t)i * 6;
					for (int r = 0; r < 6; r++) s = fma((double)blk[r * 6 + c], xi[r], s);
				}
			}
		red[tid] = (g < ng) ? s : 0.0;
		__syncthreads();
		if (tid < 6)
		{
			double t = lv[k * 6 + tid];
			for (int q = 0; q < ng; q++) t -= red[q * 6 + tid];
			ss[tid] = t;
		}
		__syncthreads();
		if (tid < 6)
		{
			const double* Li = sD + k * 36;
			double t = 0;
			for (int q = tid; q < 6; q++) t = fma(Li[q * 6 + tid], ss[q], t);
			lv[k * 6 + tid] = t;
		}
		__syncthreads();
	}
	for (int q = tid; q < nc * 6; q += nt) v[(size_t)sj[q / 6] * 6 + q % 6] = lv[q];
}

// ---------------------------------------------------------------------------------------------------------------
// Leaf tasks: everything the walk touches fits LDS.  The column steps of a task are a chain of dependent global
// round trips (pivot block, scaled column, updated targets: ~6 per column, 10-14 us measured); all blocks of the
// task's columns (288 B each + row index) fit CHOL_FACTOR_LDS (lsfm_symbolic.hpp: LSFM_TASK_X is capped so that they
// do), so they are fetched side by side once, the walk runs at LDS latency and the result is written back once.
// ---------------------------------------------------------------------------------------------------------------
struct SmallTask {
	int nc, nb;          // columns, blocks (pivot blocks included)
	double* sB;          // [nb * 36] blocks, column after column
	int* sR;             // [nb] row index of every block
	int *sj, *sc0, *sn, *sm, *sbo; // per column: global column, first global block, blocks below the pivot, in-task rows, first LDS block
};
__device__ __forceinline__ size_t small_task_bytes(int nc, int nb) { return (size_t)nb * (288 + 4) + (size_t)(5 * nc + 1) * 4 + 8; }
// lays the task out in LDS (base must be 8-byte aligned) and copies blocks and row indices in; ends with a barrier
__device__ void small_task_stage(SmallTask& t, char* base, int b0, int nc, const int* __restrict__ task_cols, const int* __restrict__ col_nin,
                                 const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ L)
{
	const int tid = threadIdx.x, nt = blockDim.x;
	__shared__ int s_nb;
	t.nc = nc;
	int* meta = reinterpret_cast<int*>(base);
	t.sj = meta; t.sc0 = meta + nc; t.sn = meta + 2 * nc; t.sm = meta + 3 * nc; t.sbo = meta + 4 * nc; // sbo has nc + 1 entries
	for (int q = tid; q < nc; q += nt)
	{
		const int j = task_cols[b0 + q];
		t.sj[q] = j;
		const int c0 = colptr[j];
		t.sc0[q] = c0; t.sn[q] = colptr[j + 1] - c0 - 1; t.sm[q] = col_nin ? col_nin[j] : 0;
	}
	__syncthreads();
	if (tid == 0)
	{
		int acc = 0;
		for (int q = 0; q < nc; q++) { t.sbo[q] = acc; acc += 1 + t.sn[q]; }
		t.sbo[nc] = acc;
		s_nb = acc;
	}
	__syncthreads();
	t.nb = s_nb;
	size_t off = ((size_t)(5 * nc + 1) * 4 + 7) & ~(size_t)7;
	t.sB = reinterpret_cast<double*>(base + off);
	t.sR = reinterpret_cast<int*>(base + off + (size_t)t.nb * 288);
	for (int e = tid; e < t.nb; e += nt)
	{
		int lo = 0, hi = nc - 1; // column of LDS block e
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.sbo[mid] <= e) lo = mid; else hi = mid - 1; }
		t.sR[e] = rowidx[t.sc0[lo] + (e - t.sbo[lo])];
	}
	for (int i = tid; i < t.nb * 36; i += nt)
	{
		const int e = i / 36;
		int lo = 0, hi = nc - 1;
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.sbo[mid] <= e) lo = mid; else hi = mid - 1; }
		t.sB[i] = L[(size_t)(t.sc0[lo] + (e - t.sbo[lo])) * 36 + (i - e * 36)];
	}
	__syncthreads();
}
// LDS column of a global column index that belongs to the task (columns are ascending)
__device__ __forceinline__ int small_task_col(const SmallTask& t, int col)
{
	int lo = 0, hi = t.nc - 1;
	while (lo < hi) { const int mid = (lo + hi) >> 1; if (t.sj[mid] < col) lo = mid + 1; else hi = mid; }
	return lo;
}
__device__ void chol_factor_task_lds(int task, const int* __restrict__ task_ptr, const int* __restrict__ task_cols,
                                     const int* __restrict__ col_nin, const int* __restrict__ colptr,
                                     const int* __restrict__ rowidx, double* __restrict__ L, double* __restrict__ Dinv, int* err)
{
	extern __shared__ double lds_d[];
	__shared__ double sLi[36];
	const int b0 = task_ptr[task], nc = task_ptr[task + 1] - b0;
	const int tid = threadIdx.x, nt = blockDim.x;
	SmallTask t;
	small_task_stage(t, reinterpret_cast<char*>(lds_d), b0, nc, task_cols, col_nin, colptr, rowidx, L);
	for (int k = 0; k < nc; k++)
	{
		const int cl = t.sbo[k], n = t.sn[k], m = t.sm[k];
		chol_pivot(t.sj[k], cl, t.sB, Dinv, err, sLi); // pivot block in LDS; Dinv to memory; ends with a barrier
		chol_scale_column(cl, n, t.sB, sLi);
		__syncthreads();
		// updates into the task's own columns (b < m), all in LDS; one pair per target block
		for (int idx = tid; idx < m * n; idx += nt)
		{
			const int b = idx / n, a = idx - b * n;
			if (a < b) continue;
			double La[36], Lb[36], T[36];
			ld<36>(La, t.sB + (size_t)(cl + 1 + a) * 36);
			ld<36>(Lb, t.sB + (size_t)(cl + 1 + b) * 36);
			mmt<6, 6, 6, false>(La, Lb, T);
			const int ra = t.sR[cl + 1 + a], rb = t.sR[cl + 1 + b];
			const int lq = small_task_col(t, rb);
			const int cb = t.sbo[lq], nbk = 1 + t.sn[lq];
			int pos = cb + (a - b);
			if (!(a - b < nbk && t.sR[pos] == ra)) pos = find_row(t.sR, cb, cb + nbk, ra);
			double* d = t.sB + (size_t)pos * 36;
			for (int q = 0; q < 36; q++) d[q] -= T[q];
		}
		__syncthreads();
	}
	// the factor goes back to memory once (the deferred updates into ancestor columns read it there)
	for (int i = tid; i < t.nb * 36; i += nt)
	{
		const int e = i / 36;
		int lo = 0, hi = nc - 1;
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.sbo[mid] <= e) lo = mid; else hi = mid - 1; }
		L[(size_t)(t.sc0[lo] + (e - t.sbo[lo])) * 36 + (i - e * 36)] = t.sB[i];
	}
}

// the leaf tasks of the factorisation in one launch, one work-group per task
__global__ void __launch_bounds__(256) k_chol_factor_level(const int* __restrict__ task_ptr, const int* __restrict__ task_cols,
                                                            const int* __restrict__ col_nin, const int* __restrict__ colptr,
                                                            const int* __restrict__ rowidx, double* __restrict__ L, double* __restrict__ Dinv, int* err, OwnFilter of)
{
	if (of.skip(task_cols[task_ptr[blockIdx.x]])) return;
	chol_factor_task_lds(blockIdx.x, task_ptr, task_cols, col_nin, colptr, rowidx, L, Dinv, err);
}


// ---------------------------------------------------------------------------------------------------------------
// Supernode groups: the factorisation above the leaf tasks.  With a path that revisits, the separators of the
// dissection are 20-70 poses wide and every separator column has 100-300 blocks below it: walking such a chain
// column by column in one work-group (the round-1 scheme) left the chip idle -- 27 ms for the top join of the
// NC3500-like set.  A group is a run of s <= CHOL_GS consecutive columns of one fundamental supernode: column c0+t
// holds [its diagonal block, the s-1-t later columns of the run, the nr common rows below the run], so block
// (row i of the common rows, column t) sits at colptr[c0+t] + (s-t) + i: the run is a dense trapezoid in the block
// storage as it is.  Per group level (children before parents) two launches (one while the panels are short: k_sn_panel<true>
// does both):
//   k_sn_panel   every work-group factors the s x s diagonal blocks in LDS (redundantly: the other CUs would idle)
//                and solves its 16 block rows of the panel against them:  X = A L_dd^-T
//   k_sn_syrk    the rank update: block (r_a, r_b) -= sum_t X[a,t] X[b,t]^T for the pairs (a >= b) of common rows, on the
//                matrix cores, left as contiguous atomics (groups of one level share ancestors)
// ---------------------------------------------------------------------------------------------------------------
/* CHOL_GS (most block columns of a group, 8): lsfm_symbolic.hpp */
#define SN_RB 16                    /* block rows of the panel per work-group */
#define SN_XS (6 * CHOL_GS + 1)     /* odd row stride of the panel rows in LDS */
#define SN_THREADS 256               /* 96 lanes own rows; the rest is there to keep more loads in flight */
#define SN_LD 8                      /* loads in flight per lane in the copy loops (a dependent load costs ~1.5 us) */
#define SN_PT (SN_THREADS + 64)      /* k_sn_panel: one more wave, the pivot wave (look-ahead factorisation of the diagonal blocks) */
// 1 / sqrt(x) without the ~300-cycle IEEE sqrt + divide chains (they sat on the critical path of every column step):
// hardware estimate + three Newton steps (full double precision up to an ulp or two -- the factor is a preconditioner
// under iterative refinement)
__device__ __forceinline__ double fast_rsqrt(double x)
{
	double r = __builtin_amdgcn_rsq(x);
	const double h = 0.5 * x;
	r = r * fma(-h * r, r, 1.5);
	r = r * fma(-h * r, r, 1.5);
	r = r * fma(-h * r, r, 1.5);
	return r;
}
// the double that lane `lane` (a compile-time constant) of the wave holds in v, as a wave-uniform value in scalar registers:
// two v_readlane_b32.  LDS reads in which every lane asks for the same address were measured at ~28 clocks per wave instruction
// on this chip (four waves on a CU share the LDS pipe): the 36 pivot-row entries of a block of dot products cost 18 of them per
// wave, 2 400 clocks per block and CU; one lane each loading one entry and 72 v_readlane_b32 cost the wave ~300 clocks of its own SIMD
__device__ __forceinline__ double wave_bcast(double v, int lane)
{
	const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
	return __hiloint2double(hi, lo);
}
// the same to full double precision with a shorter dependent chain, for the pivot wave (the chain of six of them per diagonal
// block is what a block column costs when its dot products are short): one Halley step, cubic -- the hardware estimate is good to
// ~2^-23, the step leaves ~2^-66 -- five dependent operations instead of nine
__device__ __forceinline__ double fast_rsqrt_h(double x)
{
	const double y = __builtin_amdgcn_rsq(x);
	const double e = fma(-x, y * y, 1.0);
	return fma(y, e * fma(0.375, e, 0.5), y);
}
__device__ __forceinline__ int sn_idx(int s, int u, int t) { return t * s - t * (t - 1) / 2 + (u - t); }

// Dense s x s (blocks) Cholesky of the run's diagonal part, one lane per scalar row, left-looking by block columns: for
// block column t every lane i >= 6t forms  a[c] = A[i][6t+c] - sum_{j<6t} L[i][j] L[6t+c][j]  (own row from LDS with an
// odd stride, the six pivot rows broadcast); the six lanes of the block's own rows publish theirs as the 6x6 diagonal block
// D, everybody factors D in registers (56 flops: cheaper than a second barrier-separated phase) and finishes its row.
// Two barriers per block column instead of the ~6 of the block-by-block walk, no idle lanes: ~15 us for 96 x 96 instead
// of ~65.  The panel rows X = A L_dd^-T are the same recurrence on rows below the diagonal part: other waves of the work-group
// carry them along, block column by block column, on their own SIMDs.
// fv != null: the forward substitution of ONE right-hand side rides along (the first preconditioner application of a
// level, known before the factorisation starts): fv_g^T is one more panel row, so the recurrence leaves y_g = L_dd^-1 fv_g
// in it, and every work-group takes X y_g off fv at its common rows -- what k_sn_fwd does in a launch of its own per
// group level (25 of them at the top join).  y_g goes to fw for the backward substitution.
// FUSED = false: grid (groups, chunks of SN_RB block rows of the panel); k_sn_syrk follows with the rank update.
// FUSED = true:  grid (groups, pairs (ca >= cb) of chunks of SN_RB / 2 block rows): the work-group solves the panel rows of
//                BOTH chunks and subtracts their product X_ca X_cb^T from the ancestors itself -- T = X X^T is a dense
//                (48 x 6s) x (6s x 48) contraction on v_mfma_f64_16x16x4_f64, leaving as 36 contiguous atomics per block --
//                so a group level is ONE launch.  The unfactored blocks are only read from L and the factor goes to a
//                second array Lg (same indexing): no work-group overwrites what another one of the level still reads,
//                nothing is parked.  (The solves of chunks shared by several pairs are redundant, like the diagonal part:
//                latency, not work, is what a level costs.)  Used while a level's panels have few enough rows
//                (chol_factor); beyond that the pairs would take more rounds of work-groups than the two launches.
typedef double sn_v4d __attribute__((ext_vector_type(4)));
// Profiling aid (make K9_TIMING=1): lane 0 of the first chunk's work-group of every group adds up the shader clocks of the phases
// of k_sn_panel: [0] index set-up, [1] blocks -> LDS, [2] the column loop, [3] right-hand side + inverse diagonal + stores, [4] rank
// update (fused), [5] work-groups counted, [6] sum of s.  Compiled out otherwise.
#ifdef LSFM_K9_TIMING
__device__ unsigned long long g_sn_t[32];
#define SNT_DECL unsigned long long snt_prev = __builtin_readcyclecounter()
#define SNT(i) do { if (threadIdx.x == 0 && blockIdx.y == 0) { const unsigned long long n_ = __builtin_readcyclecounter(); atomicAdd(&g_sn_t[(FUSED ? 16 : 0) + (i)], n_ - snt_prev); snt_prev = n_; } } while (0)
// inside the column loop: summed in registers, flushed once after the loop (an atomic per mark would be waited for at the next barrier)
#define SNL_DECL unsigned long long snl_[2] = { 0, 0 }
#define SNL(i) do { if (threadIdx.x == 0 && blockIdx.y == 0) { const unsigned long long n_ = __builtin_readcyclecounter(); snl_[i] += n_ - snt_prev; snt_prev = n_; } } while (0)
#define SNL_FLUSH do { if (threadIdx.x == 0 && blockIdx.y == 0) { atomicAdd(&g_sn_t[(FUSED ? 16 : 0) + 8], snl_[0]); atomicAdd(&g_sn_t[(FUSED ? 16 : 0) + 9], snl_[1]); } \
	if (threadIdx.x == 128 && blockIdx.y == 0) for (int q_ = 0; q_ < 6; q_++) atomicAdd(&g_sn_t[(FUSED ? 16 : 0) + 10 + q_], snp_[q_]); } while (0)
// the same for the first panel lane (tid 128, a lane that works in every phase): [0] slot reads [1] finish arithmetic [2] writes [3] wait at the barrier after B
// [4] dot products [5] wait at the barrier after A
#define SNP_DECL unsigned long long snp_[6] = { 0, 0, 0, 0, 0, 0 }, snp_prev = __builtin_readcyclecounter()
#define SNP(i) do { if (threadIdx.x == 128 && blockIdx.y == 0) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); const unsigned long long n_ = __builtin_readcyclecounter(); snp_[i] += n_ - snp_prev; snp_prev = n_; } } while (0)
extern "C" void lsfm_debug_sn(unsigned long long* out, int reset)
{
	(void)hipDeviceSynchronize();
	if (out) (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sn_t), sizeof(unsigned long long) * 32);
	if (reset) { unsigned long long z[32] = { 0 }; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sn_t), z, sizeof(z)); }
}
#else
#define SNT_DECL do { } while (0)
#define SNT(i) do { } while (0)
#define SNL_DECL do { } while (0)
#define SNL(i) do { } while (0)
#define SNL_FLUSH do { } while (0)
#define SNP_DECL do { } while (0)
#define SNP(i) do { } while (0)
#endif
template <bool FUSED>
__global__ void __launch_bounds__(SN_PT) k_sn_panel(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ grp_nr,
                                                          const int* __restrict__ colptr, double* __restrict__ L, double* __restrict__ Lg,
                                                          double* __restrict__ Dinv, int* err, const int* __restrict__ rowidx, double* __restrict__ fv,
                                                          double* __restrict__ fw, int smax, const double* __restrict__ diag0, double piv_floor, int* nfloor, OwnFilter of)
{
	// LDS by the widest run of the LEVEL (smax block columns), not by CHOL_GS: most levels of most systems hold runs of 1-6
	// columns, and at 150 KB a work-group had a CU to itself -- a level of 2 000 small work-groups took 8 rounds
	extern __shared__ double Ms[];
	const int LD = 6 * smax;                       // dense scalar rows of the diagonal part
	const int xs = ((LD + 3) & ~3) + 1;            // odd row stride, with room for the zero padding of the MFMA k step
	// rows 0 .. 6 GS - 1: L_dd (dense scalar rows); rows 6 GS ..: the panel rows of this work-group.  Lanes 0..95 own the
	// diagonal rows, lanes 128..223 (two other waves, other SIMDs) the panel rows: the same recurrence, in step
	__shared__ double sD[36];
	__shared__ double sLp[2 * 28];        // the pivot wave's L_tt (lower triangle, 21) and 1 / diag (6), two slots in turn
	__shared__ double sInvD[6 * CHOL_GS]; // 1 / L_kk of the run
	__shared__ double sFl[6 * CHOL_GS];   // diagonal of the (scaled) S at the run's columns: what a pivot is held against
	__shared__ int sSrc[CHOL_GS * (CHOL_GS + 1) / 2], sDst[CHOL_GS * (CHOL_GS + 1) / 2], sCol[CHOL_GS];
	__shared__ int sRow[SN_RB];  // common row (position below the run) of every panel slot, -1: empty slot
	__shared__ int spos[(SN_RB / 2) * (SN_RB / 2)]; // FUSED: block of L every (a, b) product goes to, -1: none
	double* const Ls = Ms;
	double* const Xs = Ms + LD * xs;
	const int g = blockIdx.x, c0 = grp_c0[g], s = grp_s[g], nr = grp_nr[g];
	if (of.skip(c0)) return;
	constexpr int HB = SN_RB / 2;
	int ca = 0, cb = 0;
	if constexpr (FUSED)
	{
		const int nch = (nr + HB - 1) / HB, p = blockIdx.y;
		if (p > 0 && p >= nch * (nch + 1) / 2) return;
		ca = (int)((sqrtf(8.0f * p + 1.0f) - 1.0f) * 0.5f);
		while (ca * (ca + 1) / 2 > p) ca--;
		while ((ca + 1) * (ca + 2) / 2 <= p) ca++;
		cb = p - ca * (ca + 1) / 2;
	}
	else if (blockIdx.y > 0 && (int)blockIdx.y * SN_RB >= nr) return;
	const bool diag_pair = !FUSED || ca == cb; // this work-group writes its (first) chunk's rows of the factor
	const int tid = threadIdx.x, nt = blockDim.x;
	SNT_DECL;
	const int nb = s * (s + 1) / 2, n6 = 6 * s;
	// where every block of the run's diagonal part sits in the block storage / in the dense rows (one lane per block)
	for (int t = tid; t < s; t += nt) sCol[t] = colptr[c0 + t];
	// (fetched here, once: in the column loop this load sat between the two barriers of every block column -- a memory round trip per column)
	for (int t = tid; t < 6 * s; t += nt) sFl[t] = diag0[(size_t)c0 * 6 + t];
	if (tid < SN_RB)
	{
		int row;
		if constexpr (FUSED) row = tid < HB ? ca * HB + tid : (ca == cb ? nr : cb * HB + (tid - HB));
		else row = blockIdx.y * SN_RB + tid;
		sRow[tid] = row < nr ? row : -1;
	}
	__syncthreads();
	for (int e = tid; e < nb; e += nt)
	{
		int t = 0;
		while (sn_idx(s, s - 1, t) < e) t++; // column of packed block e (s <= 16: a short scan)
		const int u = t + (e - sn_idx(s, t, t));
		sSrc[e] = (sCol[t] + (u - t)) * 36;
		sDst[e] = 6 * u * xs + 6 * t;
	}
	const int rows0 = sCol[s - 1] + 1; // the common rows: what the last column of the run holds below its diagonal
	int upd_pos = -1;
	if constexpr (FUSED)
	{
		// targets of the rank update, fetched now: the loads fly while the blocks arrive (the position is parked in LDS after them)
		if (tid < HB * HB)
		{
			const int a = tid / HB, b = tid - a * HB;
			const int ia = sRow[a], ib = ca == cb ? sRow[b] : sRow[HB + b];
			if (ia >= 0 && ib >= 0 && ia >= ib)
			{
				const int ra = rowidx[rows0 + ia], rb = rowidx[rows0 + ib];
				// the rows of the run from rb on are a subset of column rb's rows; nested patterns put the target at the same offset
				const int cbk = colptr[rb], nbk = colptr[rb + 1] - cbk;
				upd_pos = cbk + (ia - ib);
				if (!(ia - ib < nbk && rowidx[upd_pos] == ra)) upd_pos = find_row(rowidx, cbk, cbk + nbk, ra);
			}
		}
	}
	__syncthreads();
	SNT(0);
	// blocks -> dense rows, two numbers per load, SN_LD loads in flight per lane (a dependent load costs ~1.5 us).  The blocks are
	// the fixed-point accumulators of the group columns: converted as they are stored to LDS
	const int nd2 = nb * 18, np2 = SN_RB * s * 18; // pairs of numbers: diagonal part, panel slots
	const bool pivot_wave = tid >= SN_THREADS;
	if (pivot_wave && tid - SN_THREADS < 36) sD[tid - SN_THREADS] = fx_to(reinterpret_cast<const long long*>(L)[(size_t)sCol[0] * 36 + (tid - SN_THREADS)]);
	for (int base = 0; base < (pivot_wave ? 0 : nd2 + np2); base += SN_THREADS * SN_LD)
	{
		longlong2 v[SN_LD];
#pragma unroll
		for (int i = 0; i < SN_LD; i++)
		{
			const int q = base + i * SN_THREADS + tid;
			if (q < nd2) { const int e = q / 18; v[i] = *reinterpret_cast<const longlong2*>(L + (size_t)sSrc[e] + 2 * (q - e * 18)); }
			else if (q < nd2 + np2)
			{
				const int qq = q - nd2, blk = qq / 18, il = blk / s, t = blk - il * s, row = sRow[il];
				if (row >= 0) v[i] = *reinterpret_cast<const longlong2*>(L + (size_t)(sCol[t] + (s - t) + row) * 36 + 2 * (qq - blk * 18));
			}
		}
#pragma unroll
		for (int i = 0; i < SN_LD; i++)
		{
			const int q = base + i * SN_THREADS + tid;
			if (q < nd2) { const int e = q / 18, w = 2 * (q - e * 18); double* d = &Ls[sDst[e] + (w / 6) * xs + w % 6]; d[0] = fx_to(v[i].x); d[1] = fx_to(v[i].y); }
			else if (q < nd2 + np2)
			{
				const int qq = q - nd2, blk = qq / 18, w = 2 * (qq - blk * 18), il = blk / s, t = blk - il * s;
				if (sRow[il] >= 0)
				{
					double* d = &Xs[(6 * il + w / 6) * xs + 6 * t + w % 6];
					d[0] = fx_to(v[i].x); d[1] = fx_to(v[i].y);
				}
			}
		}
	}
	const int XR = LD + 6 * SN_RB; // row of the right-hand side, owned by lane 128 + 6 SN_RB
	const bool with_fv = fv && diag_pair;
	if (with_fv && tid < n6) Ms[XR * xs + tid] = fv[(size_t)c0 * 6 + tid];
	if constexpr (FUSED) { if (tid < HB * HB) spos[tid] = upd_pos; }
	bool bad = false;
	// the 6x6 Cholesky of the block in sD by every lane of the pivot wave alike, published in slot (t & 1): L_tt (lower triangle) and 1 / diag
	auto pivot_chol = [&](int t) {
		const int k0 = 6 * t, pl = tid - SN_THREADS;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier(); // (one wave: its LDS accesses are served in order; the compiler must keep them so)
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		double d[21], di[6];
#pragma unroll
		for (int r = 0; r < 6; r++)
#pragma unroll
			for (int c = 0; c <= r; c++) d[r * (r + 1) / 2 + c] = sD[r * 6 + c];
#pragma unroll
		for (int k = 0; k < 6; k++)
		{
			double pv = d[k * (k + 1) / 2 + k];
			// Modified Cholesky for the separators.  What is left of the last diagonal blocks of a top separator after everything
			// below them has been eliminated is, for the weakly observable directions of a long monocular chain (scale drift),
			// the difference of numbers a thousand to 1e13 times larger.  A pivot is taken by its magnitude, bounded below by
			// piv_floor x the entry the (scaled) S had: the factor is the exact factor of S plus a small perturbation in those one
			// or two directions, which the CG around it removes in a few steps.  Only a pivot that is negative on the scale of S
			// itself (or not a number) means the system is not positive definite.
			const double flr = sFl[k0 + k];
			const double fl = piv_floor * flr, neg = piv_floor > 0 ? -0.01 * flr : 0.0; // (piv_floor = 0: any non-positive pivot is an error)
			if (!(pv > fl))
			{
				if (!(pv == pv) || !(pv > neg) || !(fl > 0)) { bad = true; pv = 1.0; }
				else { pv = fmax(fabs(pv), fl); if (nfloor && pl == 0 && blockIdx.y == 0) atomicAdd(nfloor, 1); }
			}
#ifdef LSFM_DEBUG_PIVOT
			if (pl == 0 && blockIdx.y == 0 && c0 + t >= 16380)
				printf("[piv] col %d k %d pv %.6e fl %.3e raw %.6e\n", c0 + t, k, pv, fl, d[k * (k + 1) / 2 + k]);
#endif
			di[k] = fast_rsqrt_h(pv);
			d[k * (k + 1) / 2 + k] = pv * di[k];
#pragma unroll
			for (int r = k + 1; r < 6; r++) d[r * (r + 1) / 2 + k] *= di[k];
#pragma unroll
			for (int r = k + 1; r < 6; r++)
#pragma unroll
				for (int c = k + 1; c <= r; c++) d[r * (r + 1) / 2 + c] -= d[r * (r + 1) / 2 + k] * d[c * (c + 1) / 2 + k];
		}
		if (pl == 0)
		{
			double* slot = sLp + (t & 1) * 28;
#pragma unroll
			for (int q = 0; q < 21; q++) slot[q] = d[q];
#pragma unroll
			for (int k = 0; k < 6; k++) slot[21 + k] = di[k];
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	};
	// ... and its rows into the dense rows (nobody reads the diagonal block's place before the end of the loop; the lanes that own
	// these rows have nothing to do for column t), 1 / diag with them
	auto pivot_rows = [&](int t) {
		const int k0 = 6 * t, pl = tid - SN_THREADS;
		const double* slot = sLp + (t & 1) * 28;
		if (pl < 36)
		{
			const int r = pl / 6, c = pl - 6 * r;
			Ls[(k0 + r) * xs + k0 + c] = c <= r ? slot[r * (r + 1) / 2 + c] : 0.0;
			if (pl < 6) sInvD[k0 + pl] = slot[21 + pl];
		}
	};
	// the first diagonal block: fetched by the pivot wave itself before the block loads (sD), factored while they arrive
	if (pivot_wave) pivot_chol(0);
	__syncthreads();
	SNT(1);
	// row of Ms this lane owns (-1: none).  The lanes of the last wave (tid >= SN_THREADS) own none: it is the pivot wave
	const int ri = tid < LD ? tid : ((tid >= 128 && tid < 128 + 6 * SN_RB) ? LD + (tid - 128) : ((with_fv && tid == 128 + 6 * SN_RB) ? XR : -1));
	const bool panel_lane = ri >= LD && (ri == XR || sRow[(ri - LD) / 6] >= 0);
	// The column loop, with the factorisation of the 6x6 diagonal blocks taken off everybody's path (look-ahead).  Per block
	// column t a lane that owns a row below block t does  A(t): a = its six entries of the column minus the dot products with the
	// columns before;  B(t): finish them against L_tt.  L_tt = chol(D_tt) is a chain of six dependent reciprocal square roots:
	// round 3 had every lane run it between the two barriers of every column.  Now the PIVOT WAVE does: while the others are in
	// A(t) it forms D_tt itself from the finished rows of block t (36 lanes, one entry each, dot products of length 6t), factors
	// it, publishes L_tt and 1 / diag(L_tt) in one of two slots and puts the block's rows in place; B(t) is 27 numbers through
	// scalar registers and 27 multiply-adds.  Two barriers per column, as before.
	auto pivot_step = [&](int t) {
		const int k0 = 6 * t, pl = tid - SN_THREADS;
		if (pl < 36)
		{
			const int r = pl / 6, c = pl - 6 * r;
			const double* xr = &Ls[(k0 + r) * xs];
			const double* xc = &Ls[(k0 + c) * xs];
			double d0 = c <= r ? xr[k0 + c] : xc[k0 + r], d1 = 0.0, d2 = 0.0; // (the lower triangle of the symmetric block)
			for (int j = 0; j < k0; j += 6) // (twelve reads in flight per step: a dependent LDS read costs ~150 clocks)
			{
				double p[6], q[6];
#pragma unroll
				for (int k = 0; k < 6; k++) { p[k] = xr[j + k]; q[k] = xc[j + k]; }
				d0 = fma(-p[0], q[0], d0); d1 = fma(-p[1], q[1], d1); d2 = fma(-p[2], q[2], d2);
				d0 = fma(-p[3], q[3], d0); d1 = fma(-p[4], q[4], d1); d2 = fma(-p[5], q[5], d2);
			}
			sD[pl] = d0 + (d1 + d2);
		}
		pivot_chol(t);
		pivot_rows(t);
	};
	double a[6];
	// A(0): nothing before the first column
	if (!pivot_wave && (panel_lane || (ri >= 6 && ri < n6)))
	{
		const double* xi = &Ms[ri * xs];
#pragma unroll
		for (int c = 0; c < 6; c++) a[c] = xi[c];
	}
	if (pivot_wave) pivot_rows(0);
	__syncthreads();
	SNT(7); // (the first diagonal block's rows put in place)
	SNL_DECL;
	SNP_DECL;
	for (int t = 0; t < s; t++)
	{
		const int k0 = 6 * t;
		// ---- B(t): finish column t against the published L_tt (rows below block t; the block's own rows are the pivot wave's).  The
		// 27 numbers of the slot are the same for every lane: lane l loads number l, they arrive through scalar registers ----
		const bool mineB = !pivot_wave && (panel_lane || (ri >= k0 + 6 && ri < n6));
		if (__builtin_amdgcn_ballot_w64(mineB) != 0ull)
		{
			const double sv = sLp[(t & 1) * 28 + ((tid & 63) < 27 ? (tid & 63) : 27)];
			SNP(0);
#pragma unroll
			for (int c = 0; c < 6; c++)
			{
				double v = a[c];
#pragma unroll
				for (int k = 0; k < c; k++) v = fma(-a[k], wave_bcast(sv, c * (c + 1) / 2 + k), v);
				a[c] = v * wave_bcast(sv, 21 + c);
				__builtin_amdgcn_sched_barrier(0); // (a row of L_tt at a time in scalar registers)
			}
			SNP(1);
			if (mineB)
			{
				double* xo = &Ms[ri * xs + k0];
#pragma unroll
				for (int c = 0; c < 6; c++) xo[c] = a[c];
			}
			SNP(2);
		}
		__syncthreads();
		SNP(3);
		SNL(1);
		if (t + 1 < s)
		{
			// ---- the pivot wave: L of the next diagonal block; everybody else A(t + 1): the dot products of the next column ----
			const int k1 = k0 + 6;
			if (pivot_wave) pivot_step(t + 1);
			else
			{
				// rows below block t + 1.  The 36 entries of the pivot rows that a block of dot products needs are the same for every
				// lane: lane l < 36 of every wave loads entry l, they reach the multiply-adds through scalar registers (wave_bcast)
				const int k2 = k1 + 6;
				const bool mine = panel_lane || (ri >= k2 && ri < n6);
				if (__builtin_amdgcn_ballot_w64(mine) != 0ull) // (wave-uniform: every lane of the wave takes part in the loads)
				{
					const int lane = tid & 63, pe = lane < 36 ? lane : lane - 36 < 28 ? lane - 36 : 0;
					const double* pp = &Ls[(k1 + pe / 6) * xs + pe % 6];
					const double* xi = &Ms[(mine ? ri : 0) * xs];
#pragma unroll
					for (int c = 0; c < 6; c++) a[c] = xi[k1 + c];
					double pv = pp[0];
					for (int v = 0; v <= t; v++)
					{
						const double pn = pp[v < t ? 6 * (v + 1) : 0]; // (the next block's entry is under way while this one is used)
						double xv[6];
#pragma unroll
						for (int k = 0; k < 6; k++) xv[k] = xi[6 * v + k];
#pragma unroll
						for (int k = 0; k < 6; k++)
						{
							// (a column of the 6x6 at a time: six independent multiply-adds.  Scheduling barriers that keep the v_readlane of a
							// block from being hoisted all at once -- they need more scalar registers than there are -- were measured slower:
							// 4 400 / 3 840 clocks per column with one per row / per two columns against 3 260 without)
#pragma unroll
							for (int c = 0; c < 6; c++) a[c] = fma(-xv[k], wave_bcast(pv, c * 6 + k), a[c]);
						}
						pv = pn;
					}
				}
				SNP(4);
			}
			__syncthreads();
			SNP(5);
			SNL(0);
		}
	}
	SNL_FLUSH;
	SNT(2);
	if (bad && tid == SN_THREADS) atomicExch(err, 1 + c0);
	if (with_fv)
	{
		const double* yg = &Ms[XR * xs];
		if (blockIdx.y == 0 && tid < n6) fw[(size_t)c0 * 6 + tid] = yg[tid];
		const int slot = ri >= LD && ri != XR ? (ri - LD) / 6 : -1;
		if (panel_lane && slot >= 0 && (!FUSED || slot < HB))
		{
			const double* xr = &Ms[ri * xs];
			double o0 = 0.0, o1 = 0.0;
			for (int k = 0; k + 1 < n6; k += 2) { o0 = fma(xr[k], yg[k], o0); o1 = fma(xr[k + 1], yg[k + 1], o1); } // n6 is even
			const int r = (ri - LD) - 6 * slot;
			atomic_add_f64(fv + (size_t)rowidx[rows0 + sRow[slot]] * 6 + r, -(o0 + o1));
		}
	}
	if (blockIdx.y == 0)
	{
		// inverse of every diagonal 6x6 factor (the triangular solves use it): lane (t, c) solves L_tt x = e_c
		if (tid < n6)
		{
			const int t = tid / 6, c = tid - 6 * t;
			const double* dg = &Ls[(6 * t) * xs + 6 * t];
			double x[6];
#pragma unroll
			for (int r = 0; r < 6; r++)
			{
				double v = r == c ? 1.0 : 0.0;
#pragma unroll
				for (int k = 0; k < r; k++) v = fma(-dg[r * xs + k], x[k], v);
				x[r] = v * sInvD[6 * t + r];
			}
#pragma unroll
			for (int r = 0; r < 6; r++) Dinv[(size_t)(c0 + t) * 36 + r * 6 + c] = r >= c ? x[r] : 0.0;
		}
		// the factored diagonal blocks, to the factor's own array (the other work-groups of the group read the unfactored ones from L)
		for (int q = tid; q < nb * 36; q += nt)
		{
			const int e = q / 36, w = q - e * 36;
			Lg[(size_t)sSrc[e] + w] = Ls[sDst[e] + (w / 6) * xs + w % 6];
		}
	}
	// the solved panel rows X = A L_dd^-T of this work-group's own chunk
	if (diag_pair)
		for (int q = tid; q < (FUSED ? HB : SN_RB) * s * 18; q += nt)
		{
			const int blk = q / 18, w = 2 * (q - blk * 18), il = blk / s, t = blk - il * s, row = sRow[il];
			if (row < 0) continue;
			const double* x = &Xs[(6 * il + w / 6) * xs + 6 * t + w % 6];
			*reinterpret_cast<double2*>(Lg + (size_t)(sCol[t] + (s - t) + row) * 36 + w) = make_double2(x[0], x[1]);
		}
	SNT(3);
#ifdef LSFM_K9_TIMING
	if (threadIdx.x == 0 && blockIdx.y == 0) { atomicAdd(&g_sn_t[(FUSED ? 16 : 0) + 5], 1ull); atomicAdd(&g_sn_t[(FUSED ? 16 : 0) + 6], (unsigned long long)s); }
#endif
	if constexpr (FUSED)
	{
		if (nr == 0) return;
		// ---- rank update of the ancestors: T = X_ca X_cb^T on the matrix cores.  Rows of X past 6 s are padded with zeros up to
		// a multiple of 4 (the k step of the instruction); rows of empty slots hold stale numbers: their products are dropped ----
		const int n6r = (n6 + 3) & ~3;
		if (n6r > n6)
			for (int q = tid; q < 6 * SN_RB * (n6r - n6); q += nt) Xs[(q / (n6r - n6)) * xs + n6 + q % (n6r - n6)] = 0.0;
		__syncthreads(); // (also: the diagonal rows in Ls are no longer read -- the products land there)
		const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
		const double* XB = ca == cb ? Xs : Xs + 6 * HB * xs;
		constexpr int NTL = (6 * HB) / 16; // 16-row tiles per side: 3
		constexpr int TS = 6 * HB + 1;     // row stride of the products in LDS
		double* sT = Ms; // (over the diagonal rows, and into the X rows when the diagonal part is small: hence the barrier below)
		constexpr int TPW = (NTL * NTL + SN_PT / 64 - 1) / (SN_PT / 64);
		sn_v4d acc[TPW];
#pragma unroll
		for (int i = 0; i < TPW; i++)
		{
			acc[i] = (sn_v4d){ 0.0, 0.0, 0.0, 0.0 };
			const int q = wave + (SN_PT / 64) * i;
			if (q < NTL * NTL)
			{
				const int ti = q / NTL, tj = q - ti * NTL;
				const double* pa = &Xs[(16 * ti + (lane & 15)) * xs + (lane >> 4)];
				const double* pb = &XB[(16 * tj + (lane & 15)) * xs + (lane >> 4)];
				for (int ks = 0; ks < n6r; ks += 4) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[ks], pb[ks], acc[i], 0, 0, 0);
			}
		}
		__syncthreads();
#pragma unroll
		for (int i = 0; i < TPW; i++)
		{
			const int q = wave + (SN_PT / 64) * i;
			if (q < NTL * NTL)
			{
				const int ti = q / NTL, tj = q - ti * NTL;
				// C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
				for (int e = 0; e < 4; e++) sT[(16 * ti + (lane >> 4) + 4 * e) * TS + 16 * tj + (lane & 15)] = acc[i][e];
			}
		}
		__syncthreads();
		for (int idx = tid; idx < HB * HB * 36; idx += nt)
		{
			const int p = idx / 36, q = idx - p * 36, ps = spos[p];
			if (ps >= 0) fx_atomic_sub(L + (size_t)ps * 36 + q, sT[(6 * (p / HB) + q / 6) * TS + 6 * (p % HB) + q % 6]);
		}
		SNT(4);
	}
}

// The same rank update on the matrix cores, for the panels too tall for the fused kernel (a synth-16k Mono tree: 100-300 common
// rows per group at its upper levels -- the round-2 update kernel, one scalar 6x6 product chain per PAIR of rows, was 11 % of that tree's
// device time and loaded every block of X once per partner row).  One work-group per pair (ca >= cb) of 8-block-row chunks of a
// group's solved panel X (read from Lg): both chunks go to LDS as dense scalar rows once, T = X_ca X_cb^T is a (48 x 6s) x (6s x
// 48) contraction on v_mfma_f64_16x16x4_f64 (nine 16x16 tiles over the four waves), and the 64 products leave as 36 contiguous
// atomics each -- the tail of k_sn_panel<true> without its redundant solves.  grid (groups, pairs of chunks of the level's
// tallest panel, capped: a work-group walks pairs gridDim.y apart).
__global__ void __launch_bounds__(SN_THREADS) k_sn_syrk(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ grp_nr,
                                                         const int* __restrict__ colptr, const int* __restrict__ rowidx, double* __restrict__ L,
                                                         const double* __restrict__ Lg, int smax, OwnFilter of)
{
	extern __shared__ double Ms[];
	constexpr int HB = SN_RB / 2, NTL = (6 * HB) / 16, TS = 6 * HB + 1, TPW = (NTL * NTL + SN_THREADS / 64 - 1) / (SN_THREADS / 64);
	__shared__ int spos[HB * HB];
	__shared__ int sCol[CHOL_GS];
	const int g = blockIdx.x, c0 = grp_c0[g], s = grp_s[g], nr = grp_nr[g];
	if (nr == 0 || of.skip(c0)) return;
	const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int n6 = 6 * s, n6r = (n6 + 3) & ~3;
	const int xs = ((6 * smax + 3) & ~3) + 1; // odd row stride, room for the zero padding of the MFMA k step
	double* const XA = Ms;
	double* const XBs = Ms + 6 * HB * xs;
	const int nch = (nr + HB - 1) / HB, npairs = nch * (nch + 1) / 2;
	for (int t = tid; t < s; t += nt) sCol[t] = colptr[c0 + t];
	__syncthreads();
	const int rows0 = sCol[s - 1] + 1; // the common rows: what the last column of the run holds below its diagonal
	for (int p = blockIdx.y; p < npairs; p += gridDim.y)
	{
		int ca = (int)((sqrtf(8.0f * p + 1.0f) - 1.0f) * 0.5f);
		while (ca * (ca + 1) / 2 > p) ca--;
		while ((ca + 1) * (ca + 2) / 2 <= p) ca++;
		const int cb = p - ca * (ca + 1) / 2;
		const bool two = ca != cb;
		// targets of the 64 products (fetched first: the loads fly while the panel rows arrive)
		if (tid < HB * HB)
		{
			const int a = tid / HB, b = tid - a * HB;
			const int ia = ca * HB + a, ib = cb * HB + b;
			int pos = -1;
			if (ia < nr && ib < nr && ia >= ib)
			{
				const int ra = rowidx[rows0 + ia], rb = rowidx[rows0 + ib];
				const int cbk = colptr[rb], nbk = colptr[rb + 1] - cbk;
				pos = cbk + (ia - ib);
				if (!(ia - ib < nbk && rowidx[pos] == ra)) pos = find_row(rowidx, cbk, cbk + nbk, ra);
			}
			spos[tid] = pos;
		}
		// the two chunks of X as dense scalar rows: 2 x HB x s blocks, two doubles per load, SN_LD loads in flight per lane;
		// rows past the panel's end and the padding columns are zero
		const int np2 = (two ? 2 : 1) * HB * s * 18;
		for (int base = 0; base < np2; base += nt * SN_LD)
		{
			double2 v[SN_LD];
#pragma unroll
			for (int i = 0; i < SN_LD; i++)
			{
				const int q = base + i * nt + tid;
				v[i] = make_double2(0.0, 0.0);
				if (q < np2)
				{
					const int blk = q / 18, il = blk / s, t = blk - il * s;
					const int row = (il < HB ? ca * HB + il : cb * HB + (il - HB));
					if (row < nr) v[i] = *reinterpret_cast<const double2*>(Lg + (size_t)(sCol[t] + (s - t) + row) * 36 + 2 * (q - blk * 18));
				}
			}
#pragma unroll
			for (int i = 0; i < SN_LD; i++)
			{
				const int q = base + i * nt + tid;
				if (q < np2)
				{
					const int blk = q / 18, w = 2 * (q - blk * 18), il = blk / s, t = blk - il * s;
					double* d = &Ms[(6 * il + w / 6) * xs + 6 * t + w % 6];
					d[0] = v[i].x; d[1] = v[i].y;
				}
			}
		}
		if (n6r > n6)
			for (int q = tid; q < (two ? 2 : 1) * 6 * HB * (n6r - n6); q += nt) Ms[(q / (n6r - n6)) * xs + n6 + q % (n6r - n6)] = 0.0;
		__syncthreads();
		const double* XB = two ? XBs : XA;
		sn_v4d acc[TPW];
#pragma unroll
		for (int i = 0; i < TPW; i++)
		{
			acc[i] = (sn_v4d){ 0.0, 0.0, 0.0, 0.0 };
			const int q = wave + (SN_THREADS / 64) * i;
			if (q < NTL * NTL)
			{
				const int ti = q / NTL, tj = q - ti * NTL;
				const double* pa = &XA[(16 * ti + (lane & 15)) * xs + (lane >> 4)];
				const double* pb = &XB[(16 * tj + (lane & 15)) * xs + (lane >> 4)];
				for (int ks = 0; ks < n6r; ks += 4) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[ks], pb[ks], acc[i], 0, 0, 0);
			}
		}
		__syncthreads(); // the products are staged over the panel rows
		double* sT = Ms;
#pragma unroll
		for (int i = 0; i < TPW; i++)
		{
			const int q = wave + (SN_THREADS / 64) * i;
			if (q < NTL * NTL)
			{
				const int ti = q / NTL, tj = q - ti * NTL;
				// C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
				for (int e = 0; e < 4; e++) sT[(16 * ti + (lane >> 4) + 4 * e) * TS + 16 * tj + (lane & 15)] = acc[i][e];
			}
		}
		__syncthreads();
		for (int idx = tid; idx < HB * HB * 36; idx += nt)
		{
			const int pp = idx / 36, q = idx - pp * 36, ps = spos[pp];
			if (ps >= 0) fx_atomic_sub(L + (size_t)ps * 36 + q, sT[(6 * (pp / HB) + q / 6) * TS + 6 * (pp % HB) + q % 6]);
		}
		__syncthreads(); // spos and the staged products are overwritten by the next pair
	}
}
static size_t sn_syrk_lds(int smax)
{
	const size_t xs = ((6 * (size_t)smax + 3) & ~(size_t)3) + 1;
	return std::max((size_t)(6 * SN_RB) * xs, (size_t)(6 * SN_RB / 2) * (6 * SN_RB / 2 + 1)) * sizeof(double);
}
// dynamic LDS of k_sn_panel for a level whose widest run has smax block columns (the products of the rank update are staged over
// the same memory: at least 48 x 49 doubles)
static size_t sn_panel_lds(int smax)
{
	const size_t LD = 6 * (size_t)smax, xs = ((LD + 3) & ~(size_t)3) + 1;
	return std::max((LD + 6 * SN_RB + 1) * xs, (size_t)(6 * SN_RB / 2) * (6 * SN_RB / 2 + 1)) * sizeof(double);
}
// the factor of the group columns back into L, for readers of the whole factor in one array (chol_merge_groups: the selected
// inversion, lsfm_cov.hip)
__global__ void k_sn_merge(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ colptr, const double* __restrict__ Lg,
                           double* __restrict__ L)
{
	const int g = blockIdx.x, c0 = grp_c0[g], s = grp_s[g];
	const size_t b0 = (size_t)colptr[c0] * 36, b1 = (size_t)colptr[c0 + s] * 36;
	for (size_t q = b0 + threadIdx.x; q < b1; q += blockDim.x) L[q] = Lg[q];
}


// ---------------------------------------------------------------------------------------------------------------
// Triangular solves by supernode group (the columns above the leaf tasks; the leaf sub-trees keep k_chol_fwd/bwd_tasks).
// One work-group per group, one launch per group level.  Forward: y_g = L_dd^-1 v_g by the row-owner recurrence on the
// dense rows of L_dd in LDS (two barriers per block column), then v[r_i] -= X[i,:] y_g for the common rows, four lanes per
// row.  y_g goes to a second vector (another group of the level may still be adding to v_g's neighbours; nobody reads
// v_g after its own level).  Backward: z = y_g - X^T x[rows], x_g = L_dd^-T z, written into v.
// ---------------------------------------------------------------------------------------------------------------
template <class FT> struct SnPair;
template <> struct SnPair<double> { typedef double2 T; };
template <> struct SnPair<float> { typedef float2 T; };
template <class FT>
__device__ __forceinline__ void sn_load_diag(int s, int c0, const int* __restrict__ colptr, const FT* __restrict__ L, double* Ls, int* sSrc,
                                             int* sDst, int* sCol)
{
	const int tid = threadIdx.x, nt = blockDim.x, nb = s * (s + 1) / 2;
	for (int t = tid; t < s; t += nt) sCol[t] = colptr[c0 + t];
	__syncthreads();
	for (int e = tid; e < nb; e += nt)
	{
		int t = 0;
		while (sn_idx(s, s - 1, t) < e) t++;
		const int u = t + (e - sn_idx(s, t, t));
		sSrc[e] = (sCol[t] + (u - t)) * 36;
		sDst[e] = 6 * u * SN_XS + 6 * t;
	}
	__syncthreads();
	const int nd2 = nb * 18;
	for (int base = 0; base < nd2; base += nt * SN_LD)
	{
		typename SnPair<FT>::T v[SN_LD];
#pragma unroll
		for (int i = 0; i < SN_LD; i++)
		{
			const int q = base + i * nt + tid;
			if (q < nd2) { const int e = q / 18; v[i] = *reinterpret_cast<const typename SnPair<FT>::T*>(L + (size_t)sSrc[e] + 2 * (q - e * 18)); }
		}
#pragma unroll
		for (int i = 0; i < SN_LD; i++)
		{
			const int q = base + i * nt + tid;
			if (q < nd2) { const int e = q / 18, w = 2 * (q - e * 18); double* d = &Ls[sDst[e] + (w / 6) * SN_XS + w % 6]; d[0] = (double)v[i].x; d[1] = (double)v[i].y; }
		}
	}
	__syncthreads();
}

template <class FT>
__global__ void __launch_bounds__(SN_THREADS) k_sn_fwd(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ grp_nr,
                                                        const int* __restrict__ colptr, const int* __restrict__ rowidx, const FT* __restrict__ L,
                                                        const FT* __restrict__ Dinv, double* __restrict__ v, double* __restrict__ w, OwnFilter of)
{
	__shared__ double Ls[6 * CHOL_GS * SN_XS];
	__shared__ double sDi[CHOL_GS * 36];
	__shared__ double sA[6], sY[6 * CHOL_GS];
	__shared__ int sSrc[CHOL_GS * (CHOL_GS + 1) / 2], sDst[CHOL_GS * (CHOL_GS + 1) / 2], sCol[CHOL_GS];
	const int g = blockIdx.x, c0 = grp_c0[g], s = grp_s[g], nr = grp_nr[g];
	if (of.skip(c0)) return;
	const int tid = threadIdx.x, n6 = 6 * s;
	for (int q = tid; q < s * 36; q += SN_THREADS) sDi[q] = (double)Dinv[(size_t)c0 * 36 + q];
	double acc = tid < n6 ? v[(size_t)c0 * 6 + tid] : 0.0;
	sn_load_diag(s, c0, colptr, L, Ls, sSrc, sDst, sCol);
	for (int t = 0; t < s; t++)
	{
		const int k0 = 6 * t;
		if (tid >= k0 && tid < k0 + 6) sA[tid - k0] = acc;
		__syncthreads();
		if (tid >= k0 && tid < k0 + 6)
		{
			const int c = tid - k0;
			double y = 0.0;
			for (int k = 0; k <= c; k++) y = fma(sDi[t * 36 + c * 6 + k], sA[k], y);
			sY[tid] = y;
		}
		__syncthreads();
		if (tid >= k0 + 6 && tid < n6)
		{
			const double* lr = &Ls[tid * SN_XS + k0];
#pragma unroll
			for (int k = 0; k < 6; k++) acc = fma(-lr[k], sY[k0 + k], acc);
		}
	}
	if (tid < n6) w[(size_t)c0 * 6 + tid] = sY[tid];
	// the common rows: v[r_i] -= sum_t X[i,t] y_t, four lanes per row (each every 4th column of the run)
	const int rows0 = colptr[c0 + s - 1] + 1;
	const int sub = tid & 3;
	for (int i = tid >> 2; i < nr; i += SN_THREADS / 4)
	{
		double o[6] = { 0, 0, 0, 0, 0, 0 };
		for (int t = sub; t < s; t += 4)
		{
			const FT* blk = L + ((size_t)sCol[t] + (s - t) + i) * 36;
			double b[36];
			ld<36>(b, blk);
#pragma unroll
			for (int r = 0; r < 6; r++)
#pragma unroll
				for (int k = 0; k < 6; k++) o[r] = fma(b[r * 6 + k], sY[6 * t + k], o[r]);
		}
#pragma unroll
		for (int r = 0; r < 6; r++)
		{
			o[r] += __shfl_xor(o[r], 1, LSFM_WAVE);
			o[r] += __shfl_xor(o[r], 2, LSFM_WAVE);
		}
		if (sub == 0)
		{
			double* dst = v + (size_t)rowidx[rows0 + i] * 6;
#pragma unroll
			for (int r = 0; r < 6; r++) atomic_add_f64(dst + r, -o[r]);
		}
	}
}

template <class FT>
__global__ void __launch_bounds__(SN_THREADS) k_sn_bwd(const int* __restrict__ grp_c0, const int* __restrict__ grp_s, const int* __restrict__ grp_nr,
                                                        const int* __restrict__ colptr, const int* __restrict__ rowidx, const FT* __restrict__ L,
                                                        const FT* __restrict__ Dinv, double* __restrict__ v, const double* __restrict__ w, OwnFilter of)
{
	__shared__ double Ls[6 * CHOL_GS * SN_XS];
	__shared__ double sDi[CHOL_GS * 36];
	__shared__ double sA[6], sZ[6 * CHOL_GS], sX[6 * CHOL_GS];
	__shared__ int sSrc[CHOL_GS * (CHOL_GS + 1) / 2], sDst[CHOL_GS * (CHOL_GS + 1) / 2], sCol[CHOL_GS];
	const int g = blockIdx.x, c0 = grp_c0[g], s = grp_s[g], nr = grp_nr[g];
	if (of.skip(c0)) return;
	const int tid = threadIdx.x, n6 = 6 * s;
	for (int q = tid; q < s * 36; q += SN_THREADS) sDi[q] = (double)Dinv[(size_t)c0 * 36 + q];
	if (tid < n6) sZ[tid] = w[(size_t)c0 * 6 + tid];
	sn_load_diag(s, c0, colptr, L, Ls, sSrc, sDst, sCol); // (ends with a barrier: sZ, sDi, sCol visible)
	// z -= X^T x over the common rows (all final: they belong to higher levels), four lanes per row
	const int rows0 = colptr[c0 + s - 1] + 1;
	const int sub = tid & 3;
	for (int i = tid >> 2; i < nr; i += SN_THREADS / 4)
	{
		const double* xr = v + (size_t)rowidx[rows0 + i] * 6;
		double x6[6];
		ld<6>(x6, xr);
		for (int t = sub; t < s; t += 4)
		{
			const FT* blk = L + ((size_t)sCol[t] + (s - t) + i) * 36;
			double b[36];
			ld<36>(b, blk);
#pragma unroll
			for (int c = 0; c < 6; c++)
			{
				double o = 0.0;
#pragma unroll
				for (int r = 0; r < 6; r++) o = fma(b[r * 6 + c], x6[r], o);
				lds_add_f64(&sZ[6 * t + c], -o);
			}
		}
	}
	__syncthreads();
	// x_g = L_dd^-T z: lane (t, c) owns column 6t + c, block columns from the last to the first
	double acc = tid < n6 ? sZ[tid] : 0.0;
	for (int t = s - 1; t >= 0; t--)
	{
		const int k0 = 6 * t;
		if (tid >= k0 && tid < k0 + 6) sA[tid - k0] = acc;
		__syncthreads();
		if (tid >= k0 && tid < k0 + 6)
		{
			const int c = tid - k0;
			double x = 0.0;
			for (int k = c; k < 6; k++) x = fma(sDi[t * 36 + k * 6 + c], sA[k], x);
			sX[tid] = x;
		}
		__syncthreads();
		if (tid < k0)
		{
#pragma unroll
			for (int k = 0; k < 6; k++) acc = fma(-Ls[(k0 + k) * SN_XS + tid], sX[k0 + k], acc);
		}
	}
	if (tid < n6) v[(size_t)c0 * 6 + tid] = sX[tid];
}

__global__ void k_to_float(size_t n, const double* __restrict__ a, float* __restrict__ b)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) b[i] = (float)a[i];
}

// v = D^-1/2 P r  (the factor is the scaled matrix's: k_chol_scatter)
__global__ void k_perm_in(int M, const int* __restrict__ perm, const double* __restrict__ r, const unsigned char* __restrict__ fixed,
                          const double* __restrict__ dscale, double* __restrict__ v, int zero_from)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t)M * 6) return;
	const size_t src = (size_t)perm[i / 6] * 6 + i % 6;
	// (distributed: the shared rows collect the ranks' partial sums; only rank 0 starts them from the right-hand side: zero_from = first shared row elsewhere)
	v[i] = ((fixed && fixed[src]) || (long)(i / 6) >= (long)zero_from) ? 0.0 : r[src] * dscale[i];
}
// z = P^T D^-1/2 v ; rz[nxt] += r . z
__global__ void k_perm_out_dot(int M, const int* __restrict__ pinv, const double* __restrict__ v, const double* __restrict__ r,
                               const unsigned char* __restrict__ fixed, const double* __restrict__ dscale, const int* __restrict__ pose_seg,
                               double* __restrict__ z, double* dot, int dot_stride, const int* __restrict__ col_owner, int rank)
{
	int row = blockIdx.x * blockDim.x + threadIdx.x;
	const bool ok = row < M;
	double acc = 0;
	int sg = 0;
	if (ok)
	{
		sg = pose_seg[row];
		const double* src = v + (size_t)pinv[row] * 6;
		const double* sc = dscale + (size_t)pinv[row] * 6;
		for (int i = 0; i < 6; i++)
		{
			double zz = src[i] * sc[i];
			if (fixed && fixed[(size_t)row * 6 + i]) zz = 0.0;
			// (distributed: a rank holds the solution at its own block's columns, rank 0 at the shared ones too; the sum over the ranks is z)
			if (col_owner) { const int ow = col_owner[pinv[row]]; if (!(ow == rank || (ow < 0 && rank == 0))) zz = 0.0; }
			z[(size_t)row * 6 + i] = zz;
			acc = fma(zz, r[(size_t)row * 6 + i], acc);
		}
	}
	if (dot) wave_scatter_add<1>(dot + (size_t)sg * dot_stride, &acc, ok);
}
// rz[nxt] += r . z  alone (distributed: z is complete only after the ranks' parts have been summed)
__global__ void k_rz_dot(int M, const double* __restrict__ z, const double* __restrict__ r, const int* __restrict__ pose_seg, double* dot, int dot_stride)
{
	int row = blockIdx.x * blockDim.x + threadIdx.x;
	const bool ok = row < M;
	double acc = 0;
	int sg = 0;
	if (ok)
	{
		sg = pose_seg[row];
		for (int i = 0; i < 6; i++) acc = fma(z[(size_t)row * 6 + i], r[(size_t)row * 6 + i], acc);
	}
	wave_scatter_add<1>(dot + (size_t)sg * dot_stride, &acc, ok);
}

// ---------------------------------------------------------------------------------------------------------------
// host: ordering + symbolic factorisation
// ---------------------------------------------------------------------------------------------------------------
// the two small device -> host copies of the analysis (a synchronisation), separate from the host work so that the
// caller can enqueue the numeric Schur assembly in between and let it run under the symbolic factorisation
void chol_fetch(lsfm_context* ctx, const SchurSystem& sy, const int* d_origin, CholHostIn& in)
{
	const int M = sy.M, nnzb = sy.nnzb;
	in.keys.resize(nnzb);
	in.origin.resize(M);
	if (d_origin) LSFM_CHECK_HIP(hipMemcpyAsync(in.origin.data(), d_origin, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	else std::iota(in.origin.begin(), in.origin.end(), 0);
	d2h(ctx, in.keys.data(), sy.upper_keys, (size_t)nnzb * sizeof(unsigned long long));
}

// value arrays of a factorisation and its error flag, zeroed (per run; the index arrays may come from a plan)
void chol_alloc_values(lsfm_context* ctx, CholDev& ch)
{
	Arena& sc = ctx->scratch;
	ch.L = sc.alloc<double>((size_t)ch.nnzL * 36); ch.Dinv = sc.alloc<double>((size_t)ch.M * 36);
	ch.wv = sc.alloc<double>((size_t)ch.M * 6);
	ch.diag0 = sc.alloc<double>((size_t)ch.M * 6);
	ch.dscale = sc.alloc<double>((size_t)ch.M * 6);
	ch.Lg = ch.ngroups ? sc.alloc<double>((size_t)ch.nnzL * 36) : nullptr; // (every block of a group column is written by the factorisation)
	dev_zero(ctx, ch.L, (size_t)ch.nnzL * 36 * sizeof(double));
	static const bool digest = getenv("LSFM_FACTOR_DIGEST") != nullptr; // (the digest reads all of Lg: the leaf columns' slots, never written, must not be noise)
	if (digest && ch.Lg) dev_zero(ctx, ch.Lg, (size_t)ch.nnzL * 36 * sizeof(double));
	ch.d_err = sc.alloc<int>(1);
	dev_zero(ctx, ch.d_err, sizeof(int));
}

// dynamic LDS of the leaf-task triangular solves (k_chol_fwd_tasks / k_chol_bwd_tasks): within CHOL_SOLVE_LDS (chol_upload_index)
static size_t chol_task_lds(const CholDev& ch) { return (size_t)ch.task0_maxsize * CHOL_TASK_LDS_PER_COL + 8; }
// index arrays of a symbolic factorisation to the device in ONE copy (ctx->scratch / ctx->stream as the caller has set them), host
// vectors copied: what a plan keeps
void chol_upload_index(lsfm_context* ctx, const CholSymbolic& sym, CholDev& ch)
{
	Arena& sc = ctx->scratch;
	ch.M = sym.M; ch.nnzL = sym.nnzL; ch.nlevels = sym.nlevels; ch.tail_begin = sym.tail_begin;
	ch.level_ptr = sym.level_ptr;
	if (!sym.tlevel_ptr.empty())
	{
		// the leaf tasks (task level 0) are the only ones walked as tasks, each whole in LDS -- by the factorisation and by the
		// solves (LSFM_TASK_X <= CHOL_TASK_X_MAX makes sure of it)
		ch.ntask0 = sym.tlevel_ptr[1]; ch.ncol0 = sym.tlevel_col0[1];
		ch.task0_maxsize = sym.tlevel_maxsize[0]; ch.task0_lds = sym.tlevel_small_lds[0]; ch.task0_outer = sym.tlevel_outer[0];
		if (sym.tlevel_nsmall[0] != ch.ntask0 || chol_task_lds(ch) > CHOL_SOLVE_LDS)
			LSFM_FAIL(LSFM_ERR_INTERNAL, "a leaf task of the factorisation does not fit LDS (" + std::to_string(sym.tlevel_nsmall[0]) + " of " + std::to_string(ch.ntask0) +
			                                 " fit, " + std::to_string(ch.task0_maxsize) + " columns at most)");
	}
	ch.ngroups = sym.ngroups; ch.glevel_ptr = sym.glevel_ptr; ch.glevel_maxnr = sym.glevel_maxnr; ch.glevel_maxs = sym.glevel_maxs;
	ch.work_total = sym.work_total; ch.work_shared = sym.work_shared;
	ch.first_shared = sym.first_shared; ch.shared_blk0 = sym.colptr[sym.first_shared]; ch.glevel_owned = sym.glevel_owned; ch.glevel_shared = sym.glevel_shared;
	const struct { int** dst; const std::vector<int>* v; } parts[] = {
		{ &ch.grp_c0, &sym.grp_c0 }, { &ch.grp_s, &sym.grp_s }, { &ch.grp_nr, &sym.grp_nr }, { &ch.col_nin, &sym.col_nin }, { &ch.col_task, &sym.col_task },
		{ &ch.col_lpos, &sym.col_lpos }, { &ch.task_cols, &sym.task_cols }, { &ch.task_ptr, &sym.task_ptr }, { &ch.colptr, &sym.colptr },
		{ &ch.rowidx, &sym.rowidx }, { &ch.perm, &sym.perm }, { &ch.pinv, &sym.pinv }, { &ch.order, &sym.order }, { &ch.col_owner, &sym.col_owner } };
	size_t total = 0;
	for (const auto& pt : parts) total += pt.v->size();
	static thread_local std::vector<int> blob;
	blob.resize(total);
	int* d_blob = sc.alloc<int>(total);
	size_t off = 0;
	for (const auto& pt : parts)
	{
		if (!pt.v->empty()) memcpy(blob.data() + off, pt.v->data(), pt.v->size() * sizeof(int));
		*pt.dst = pt.v->empty() ? nullptr : d_blob + off;
		off += pt.v->size();
	}
	h2d(ctx, d_blob, blob.data(), total * sizeof(int));
	ch.blob = d_blob; ch.blob_ints = total;
}
void chol_upload_symbolic(lsfm_context* ctx, const CholSymbolic& sym, CholDev& ch)
{
	chol_upload_index(ctx, sym, ch);
	chol_alloc_values(ctx, ch);
	if (getenv("LSFM_DEBUG") && sym.ngroups > 50)
	{
		int hist[CHOL_GS + 1] = { 0 };
		for (int g = 0; g < sym.ngroups; g++) hist[sym.grp_s[g]]++;
		fprintf(stderr, "[lsfm] groups %d, group levels %d, sizes:", sym.ngroups, (int)sym.glevel_ptr.size() - 1);
		for (int q = 1; q <= CHOL_GS; q++) fprintf(stderr, " %d", hist[q]);
		fprintf(stderr, " | groups per level:");
		for (size_t l = 0; l + 1 < sym.glevel_ptr.size(); l++) fprintf(stderr, " %d", sym.glevel_ptr[l + 1] - sym.glevel_ptr[l]);
		fprintf(stderr, "\n");
	}
}
void chol_analyse(lsfm_context* ctx, const SchurSystem& sy, const CholHostIn& in, CholDev& ch)
{
	static thread_local CholSymbolic sym;
	chol_symbolic(in.keys.data(), sy.nnzb, in.origin.data(), sy.M, sym, ctx->comm ? ctx->comm->block_maps : 0);
	chol_upload_symbolic(ctx, sym, ch);
}

// the factorisation of this system is distributed over the ranks of a feature-sharded run (CholDev::col_owner)
bool chol_distributed(const lsfm_context* ctx, const CholDev& ch)
{
	return ctx->comm && ctx->comm->world > 1 && ch.col_owner && ch.first_shared < ch.M;
}
// sums `count` 8-byte numbers at p over the ranks (through the caller's buffer: p lives in this context's arenas)
static void comm_sum(lsfm_context* ctx, void* p, size_t count, int dtype)
{
	if (!count) return;
	Comm& cm = *ctx->comm;
	const size_t mk = cm.off;
	void* b = cm.alloc_bytes(count * 8);
	LSFM_CHECK_HIP(hipMemcpyAsync(b, p, count * 8, hipMemcpyDeviceToDevice, ctx->stream));
	cm.allreduce(ctx->stream, b, count, dtype);
	LSFM_CHECK_HIP(hipMemcpyAsync(p, b, count * 8, hipMemcpyDeviceToDevice, ctx->stream));
	cm.off = mk; // (consumed in stream order: the next sum may take the same place)
}
// sums the n (one or two) numbers at h, on the host, over the ranks: through the exchange buffer and back, a synchronisation
void comm_sum_host(lsfm_context* ctx, long long* h, int n)
{
	hipStream_t s = ctx->stream;
	Comm& cm = *ctx->comm;
	const size_t mk = cm.off;
	long long* d = cm.alloc<long long>(n);
	LSFM_CHECK_HIP(hipMemcpyAsync(d, h, n * sizeof(long long), hipMemcpyHostToDevice, s));
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	cm.allreduce(s, d, n, LSFM_DTYPE_I64);
	LSFM_CHECK_HIP(hipMemcpyAsync(h, d, n * sizeof(long long), hipMemcpyDeviceToHost, s));
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	cm.off = mk;
}

// the scaled, permuted S into the factor's storage; also leaves the scaling (ch.dscale) that k_perm_in / k_perm_out_dot apply:
// before anything is permuted in
void chol_scatter(lsfm_context* ctx, const SchurSystem& sy, const unsigned char* fixed, CholDev& ch)
{
	// (the columns above the leaf tasks -- what the supernode groups factor -- accumulate in fixed point)
	const bool dist = chol_distributed(ctx, ch);
	if (sy.nnzb)
		hipLaunchKernelGGL(k_chol_scatter, dim3((sy.nnzb + 127) / 128), dim3(128), 0, ctx->stream, sy.nnzb, sy.upper_keys, sy.S, sy.rowptr, ch.pinv, ch.colptr, ch.rowidx,
		                   fixed, ch.col_task, ch.ntask0, ch.L, ch.diag0, ch.dscale, dist ? ch.col_owner : (const int*)nullptr, dist ? ctx->comm->rank : 0);
}
// The leaf tasks in LDS, their deferred updates into the columns above them, then the supernode groups level by level.
// fwd_v != null: a right-hand side in elimination order; on return it holds what the forward substitution leaves (leaf columns in
// place, group columns in ch.wv) -- chol_apply(..., fwd_done) does the rest.
// Distributed (chol_distributed): phase 1 -- every rank factors the columns of its own block (leaf sub-trees, then its supernode
// groups level by level), whose updates into the shared separator columns it collects in its own copy of them; then the shared
// columns' accumulators -- 64-bit integers: the sum is exact and the same bits on every rank -- and the shared rows of the forward
// substitution's vector are summed over the ranks; phase 2 -- every rank factors the shared columns, alike.
void chol_factor(lsfm_context* ctx, const SchurSystem& sy, const unsigned char* fixed, CholDev& ch, double* fwd_v)
{
	hipStream_t s = ctx->stream;
	const bool dist = chol_distributed(ctx, ch);
	const OwnFilter mine{ dist ? ch.col_owner : nullptr, dist ? ctx->comm->rank : 0 }, shared{ dist ? ch.col_owner : nullptr, -1 };
	ch.sn_fused_levels = ch.sn_split_levels = 0;
	if (ch.ntask0)
	{
		hipLaunchKernelGGL(k_chol_factor_level, dim3(ch.ntask0), dim3(128), (size_t)ch.task0_lds, s, ch.task_ptr, ch.task_cols, ch.col_nin, ch.colptr, ch.rowidx,
		                   ch.L, ch.Dinv, ch.d_err, mine);
		if (ch.task0_outer > 0)
		{
			const dim3 grid(ch.ncol0, std::min((ch.task0_outer + CHOL_OUT_THREADS - 1) / CHOL_OUT_THREADS, 64));
			hipLaunchKernelGGL(k_chol_update_outer, grid, dim3(CHOL_OUT_THREADS), 0, s, ch.task_cols, ch.col_nin, ch.colptr, ch.rowidx, ch.L, mine);
		}
		// the leaf sub-trees are factored: their part of the forward substitution, before the groups take theirs
		if (fwd_v)
			hipLaunchKernelGGL(k_chol_fwd_tasks<double>, dim3(ch.ntask0), dim3(128), chol_task_lds(ch), s, ch.task_ptr, ch.task_cols, ch.col_task, ch.col_lpos, 0, ch.colptr,
			                   ch.rowidx, (const double*)ch.L, (const double*)ch.Dinv, fwd_v, mine);
	}
	// one launch per group level while the panels are short enough for the fused kernel (pairs of 8-row chunks: a panel of
	// 64 rows is 36 work-groups per group, each repeating the solve of its two chunks); taller ones take the panel kernel +
	// the rank-update kernel (a synth-16k Mono tree, whose upper levels have panels of 100-300 rows: 684 ms against 826
	// with everything fused)
	static const int fuse_max = getenv("LSFM_SN_FUSE_MAX") ? atoi(getenv("LSFM_SN_FUSE_MAX")) : 96; // (groups of <= 8 columns: 64 -> 96 rows, 9.5 -> 9.2 ms per NC3500 tree; 128 costs synth-16k 143 -> 169 ms)
	static const double piv_floor = getenv("LSFM_PIVOT_FLOOR") ? atof(getenv("LSFM_PIVOT_FLOOR")) : 1e-13; // (0: none)
	static const bool lds_set = []() {
		// (dynamic LDS beyond 64 KB has to be asked for once per kernel)
		(void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sn_panel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sn_panel_lds(CHOL_GS));
		(void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sn_panel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sn_panel_lds(CHOL_GS));
		(void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sn_syrk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sn_syrk_lds(CHOL_GS));
		return true;
	}();
	(void)lds_set;
	for (int phase = 0; phase < (dist ? 2 : 1); phase++)
	{
		const OwnFilter of = phase == 0 ? mine : shared;
		if (phase == 1)
		{
			comm_sum(ctx, ch.L + (size_t)ch.shared_blk0 * 36, ((size_t)ch.nnzL - ch.shared_blk0) * 36, LSFM_DTYPE_I64);
			if (fwd_v) comm_sum(ctx, fwd_v + (size_t)ch.first_shared * 6, ((size_t)ch.M - ch.first_shared) * 6, LSFM_DTYPE_F64);
		}
		for (size_t l = 0; l + 1 < ch.glevel_ptr.size(); l++)
		{
			const int g0 = ch.glevel_ptr[l], ng = ch.glevel_ptr[l + 1] - g0, mnr = ch.glevel_maxnr[l];
			if (!ng) continue;
			if (dist && !(phase == 0 ? ch.glevel_owned[l] : ch.glevel_shared[l])) continue;
			const int smax = l < ch.glevel_maxs.size() ? ch.glevel_maxs[l] : CHOL_GS;
			if (mnr <= fuse_max)
			{
				const int nch = (mnr + SN_RB / 2 - 1) / (SN_RB / 2);
				hipLaunchKernelGGL(k_sn_panel<true>, dim3(ng, std::max(1, nch * (nch + 1) / 2)), dim3(SN_PT), sn_panel_lds(smax), s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0,
				                   ch.colptr, ch.L, ch.Lg, ch.Dinv, ch.d_err, ch.rowidx, fwd_v, ch.wv, smax, ch.diag0, piv_floor, ctx->d_run ? &ctx->d_run->floored : nullptr, of);
				ch.sn_fused_levels++;
				continue;
			}
			hipLaunchKernelGGL(k_sn_panel<false>, dim3(ng, std::max(1, (mnr + SN_RB - 1) / SN_RB)), dim3(SN_PT), sn_panel_lds(smax), s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0,
			                   ch.colptr, ch.L, ch.Lg, ch.Dinv, ch.d_err, ch.rowidx, fwd_v, ch.wv, smax, ch.diag0, piv_floor, ctx->d_run ? &ctx->d_run->floored : nullptr, of);
			const long nch = (mnr + SN_RB / 2 - 1) / (SN_RB / 2), npair = nch * (nch + 1) / 2;
			hipLaunchKernelGGL(k_sn_syrk, dim3(ng, (unsigned)std::max<long>(1, std::min<long>(npair, 8192))), dim3(SN_THREADS), sn_syrk_lds(smax), s,
			                   ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, ch.colptr, ch.rowidx, ch.L, ch.Lg, smax, of);
			ch.sn_split_levels++;
		}
	}
}

void chol_merge_groups(lsfm_context* ctx, const CholDev& ch)
{
	if (ch.ngroups)
		hipLaunchKernelGGL(k_sn_merge, dim3(ch.ngroups), dim3(256), 0, ctx->stream, ch.grp_c0, ch.grp_s, ch.colptr, ch.Lg, ch.L);
}
// mixed precision (BASELINE configs[4]): the factor is rounded to fp32 once and applied from there; S, E, x and the
// residual stay fp64 -- every refinement step corrects against r = E - S x in fp64
void chol_round_to_float(lsfm_context* ctx, CholDev& ch)
{
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	const size_t nl = (size_t)ch.nnzL * 36, nd = (size_t)ch.M * 36;
	ch.Lf = sc.alloc<float>(nl); ch.Dinvf = sc.alloc<float>(nd);
	hipLaunchKernelGGL(k_to_float, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, nl, ch.L, ch.Lf);
	if (ch.Lg)
	{
		ch.Lgf = sc.alloc<float>(nl);
		hipLaunchKernelGGL(k_to_float, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, nl, ch.Lg, ch.Lgf);
	}
	hipLaunchKernelGGL(k_to_float, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, nd, ch.Dinv, ch.Dinvf);
}

// v = D^-1/2 P r: a right-hand side into elimination order, scaled like the factor
void chol_perm_in(lsfm_context* ctx, const CholDev& ch, const double* r, const unsigned char* fixed, double* v)
{
	const size_t ns = (size_t)ch.M * 6;
	// (distributed: the shared rows start from the right-hand side on rank 0 only -- they collect the sum of the ranks' parts)
	const int zero_from = (chol_distributed(ctx, ch) && ctx->comm->rank != 0) ? ch.first_shared : INT_MAX;
	hipLaunchKernelGGL(k_perm_in, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream, ch.M, ch.perm, r, fixed, ch.dscale, v, zero_from);
}

// z = (L L^T)^-1 r in the original numbering, dot[seg] += r . z
// fwd_done: v already went through the forward substitution (chol_factor with fwd_v).
// Distributed: forward -- own columns, then the shared rows of v summed over the ranks, then the shared columns (alike on every
// rank); backward -- the shared columns, then the own ones; z is the sum of the ranks' parts (z: in the caller's exchange buffer).
void chol_apply(lsfm_context* ctx, const CholDev& ch, const double* r, double* v, double* z, const unsigned char* fixed, const int* pose_seg,
                double* dot, int dot_stride, bool fwd_done)
{
	hipStream_t s = ctx->stream;
	if (!fwd_done) chol_perm_in(ctx, ch, r, fixed, v);
	// leaf sub-trees (task level 0) by task, everything above them by supernode group
	const int ngl = (int)ch.glevel_ptr.size() - 1;
	const bool dist = chol_distributed(ctx, ch);
	const OwnFilter mine{ dist ? ch.col_owner : nullptr, dist ? ctx->comm->rank : 0 }, shared{ dist ? ch.col_owner : nullptr, -1 };
	// (Lx: the leaf columns' factor, in place in L; Gx: the group columns' factor, in its own array)
	auto sweep = [&](auto tag, const auto* Lx, const auto* Gx, const auto* Dx) {
		typedef decltype(tag) FT;
		if (!fwd_done)
		{
			if (ch.ntask0) hipLaunchKernelGGL(k_chol_fwd_tasks<FT>, dim3(ch.ntask0), dim3(128), chol_task_lds(ch), s, ch.task_ptr, ch.task_cols, ch.col_task, ch.col_lpos, 0, ch.colptr, ch.rowidx, Lx, Dx, v, mine);
			for (int phase = 0; phase < (dist ? 2 : 1); phase++)
			{
				if (phase == 1) comm_sum(ctx, v + (size_t)ch.first_shared * 6, ((size_t)ch.M - ch.first_shared) * 6, LSFM_DTYPE_F64);
				for (int l = 0; l < ngl; l++)
				{
					const int g0 = ch.glevel_ptr[l], ng = ch.glevel_ptr[l + 1] - g0;
					if (!ng || (dist && !(phase == 0 ? ch.glevel_owned[l] : ch.glevel_shared[l]))) continue;
					hipLaunchKernelGGL(k_sn_fwd<FT>, dim3(ng), dim3(SN_THREADS), 0, s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, ch.colptr, ch.rowidx, Gx, Dx, v, ch.wv, phase == 0 ? mine : shared);
				}
			}
		}
		for (int phase = (dist ? 1 : 0); phase >= 0; phase--) // backward: the shared columns first
			for (int l = ngl - 1; l >= 0; l--)
			{
				const int g0 = ch.glevel_ptr[l], ng = ch.glevel_ptr[l + 1] - g0;
				if (!ng || (dist && !(phase == 0 ? ch.glevel_owned[l] : ch.glevel_shared[l]))) continue;
				hipLaunchKernelGGL(k_sn_bwd<FT>, dim3(ng), dim3(SN_THREADS), 0, s, ch.grp_c0 + g0, ch.grp_s + g0, ch.grp_nr + g0, ch.colptr, ch.rowidx, Gx, Dx, v, ch.wv, (dist && phase == 1) ? shared : mine);
			}
		if (ch.ntask0) hipLaunchKernelGGL(k_chol_bwd_tasks<FT>, dim3(ch.ntask0), dim3(128), chol_task_lds(ch), s, ch.task_ptr, ch.task_cols, ch.col_task, ch.col_lpos, 0, ch.colptr, ch.rowidx, Lx, Dx, v, mine);
	};
	if (ch.Lf) sweep(float(), (const float*)ch.Lf, (const float*)ch.Lgf, (const float*)ch.Dinvf); // mixed precision: the factor applied in fp32
	else sweep(double(), (const double*)ch.L, (const double*)ch.Lg, (const double*)ch.Dinv);
	if (dist)
	{
		hipLaunchKernelGGL(k_perm_out_dot, dim3((ch.M + 127) / 128), dim3(128), 0, s, ch.M, ch.pinv, v, r, fixed, ch.dscale, pose_seg, z, (double*)nullptr, dot_stride,
		                   ch.col_owner, ctx->comm->rank);
		ctx->comm->allreduce(s, z, (size_t)ch.M * 6, LSFM_DTYPE_F64);
		hipLaunchKernelGGL(k_rz_dot, dim3((ch.M + 127) / 128), dim3(128), 0, s, ch.M, z, r, pose_seg, dot, dot_stride);
	}
	else
		hipLaunchKernelGGL(k_perm_out_dot, dim3((ch.M + 127) / 128), dim3(128), 0, s, ch.M, ch.pinv, v, r, fixed, ch.dscale, pose_seg, z, dot, dot_stride, (const int*)nullptr, 0);
}

// The front of the test entries on a caller's matrix (lsfm_chol.hpp): upload, chol_analyse, chol_scatter, chol_factor.
void chol_selftest_front(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                         size_t extra_bytes, int cap_blocks, int* nnzL_out, bool rowsorted, const double* ride_r, SelftestFront& fr)
{
	const int nnzb = rowptr[m];
	const size_t ns = (size_t)m * 6;
	CholHostIn hin;
	hin.keys.resize(nnzb);
	hin.origin.resize(m);
	for (int p = 0; p < m; p++)
	{
		hin.origin[p] = origin ? origin[p] : p;
		for (int k = rowptr[p]; k < rowptr[p + 1]; k++) hin.keys[k] = ((unsigned long long)(unsigned)p << 32) | (unsigned)colidx[k];
	}
	{
		// (the size of the factor first, on the host: the arenas are made for it, and a caller whose arrays are too small learns it here)
		CholSymbolic sym;
		chol_symbolic(hin.keys.data(), nnzb, hin.origin.data(), m, sym);
		if (nnzL_out) *nnzL_out = sym.nnzL;
		if (cap_blocks >= 0 && cap_blocks < sym.nnzL) LSFM_FAIL(LSFM_ERR_ARG, "rowidx / L too small for the factor (" + std::to_string(sym.nnzL) + " blocks)");
		// (L, Lg and their fp32 copies; S, keys and the row-sorted list; a dozen vectors and what the caller adds)
		ctx->ensure_arenas((size_t)sym.nnzL * 36 * 32 + (size_t)nnzb * (rowsorted ? 448 : 320) + ns * 8 * 16 + extra_bytes + ((size_t)64 << 20));
	}
	ctx->scratch.reset();
	Arena& sc = ctx->scratch;
	SchurSystem& sy = fr.sy;
	sy.M = m; sy.nnzb = nnzb;
	unsigned long long* dk = sc.alloc<unsigned long long>(nnzb + 1);
	sy.S = sc.alloc<double>((size_t)nnzb * 36);
	sy.rowptr = sc.alloc<int>(m + 1);
	h2d(ctx, dk, hin.keys.data(), (size_t)nnzb * sizeof(unsigned long long));
	h2d(ctx, sy.S, val, (size_t)nnzb * 36 * sizeof(double));
	h2d(ctx, sy.rowptr, rowptr, (size_t)(m + 1) * sizeof(int));
	sy.upper_keys = dk;
	if (rowsorted)
	{
		struct Keep { lsfm_context* c; int v; ~Keep() { c->pcg.spmv_variant = v; } } keep{ ctx, ctx->pcg.spmv_variant };
		ctx->pcg.spmv_variant = 2;
		build_spmv_index(ctx, sy, dk);
	}
	if (fixed) { fr.d_fixed = sc.alloc<unsigned char>(ns); h2d(ctx, fr.d_fixed, fixed, ns); }
	CholDev& ch = fr.ch;
	chol_analyse(ctx, sy, hin, ch);
	// (the count of floored pivots goes to a record of this call's own, as in lsfm_cov.hip)
	RunStatsDev* d_run = fr.d_run = sc.alloc<RunStatsDev>(1);
	dev_zero(ctx, d_run, sizeof(RunStatsDev));
	struct Swap { lsfm_context* c; RunStatsDev* keep; ~Swap() { c->d_run = keep; } } swap{ ctx, ctx->d_run };
	ctx->d_run = d_run;
	chol_scatter(ctx, sy, fr.d_fixed, ch);
	if (ride_r)
	{
		double* dr = sc.alloc<double>(ns);
		fr.fwd_v = sc.alloc<double>(ns);
		h2d(ctx, dr, ride_r, ns * sizeof(double));
		chol_perm_in(ctx, ch, dr, fr.d_fixed, fr.fwd_v);
	}
	chol_factor(ctx, sy, fr.d_fixed, ch, fr.fwd_v);
}

// Test entry of the C ABI (lsfm_selftest_chol, include/lsfm.h has the arguments): the factor of a caller's matrix and UNREFINED
// applications of it, by the host steps above and nothing else -- chol_analyse, chol_scatter, chol_factor, chol_round_to_float
// (mode bit 1), chol_apply once per right-hand side in order, chol_merge_groups.  Inside a level solve the refinement corrects
// whatever a wrong factor or sweep leaves (it only takes more steps); here nothing does.  The caller has checked the arguments.
int chol_selftest(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                  const int* pose_seg, int nseg, const double* r, int nrhs, int mode, double* z, double* dot, int* perm, int* colptr, int* rowidx,
                  double* L, double* Dinv, double* dscale, int cap_blocks, int* info)
{
	const size_t ns = (size_t)m * 6;
	const bool fused = (mode & 1) != 0;
	SelftestFront fr;
	chol_selftest_front(ctx, m, rowptr, colidx, val, origin, fixed, ns * 8 * 2 * (size_t)nrhs, cap_blocks, &info[0], false, fused ? r : nullptr, fr);
	Arena& sc = ctx->scratch;
	CholDev& ch = fr.ch;
	unsigned char* dfx = fr.d_fixed;
	int* dseg = sc.alloc<int>(m);
	h2d(ctx, dseg, pose_seg, (size_t)m * sizeof(int));
	double* dr = sc.alloc<double>(ns * nrhs);
	double* dz = sc.alloc<double>(ns * nrhs);
	double* ddot = sc.alloc<double>((size_t)nseg * nrhs);
	double* dv = fused ? fr.fwd_v : sc.alloc<double>(ns);
	h2d(ctx, dr, r, ns * nrhs * sizeof(double));
	dev_zero(ctx, ddot, (size_t)nseg * nrhs * sizeof(double));
	if (mode & 2) chol_round_to_float(ctx, ch);
	for (int k = 0; k < nrhs; k++) chol_apply(ctx, ch, dr + ns * k, dv, dz + ns * k, dfx, dseg, ddot + (size_t)nseg * k, 1, fused && k == 0);
	chol_merge_groups(ctx, ch);
	LSFM_CHECK_HIP(hipGetLastError());
	RunStatsDev rs;
	d2h(ctx, &rs, fr.d_run, sizeof rs);
	const int chol_err = d2h_int(ctx, ch.d_err);
	const int ngl = (int)ch.glevel_ptr.size() - 1;
	info[1] = ch.ntask0; info[2] = ch.ncol0; info[3] = ch.task0_outer; info[4] = ch.ngroups; info[5] = std::max(ngl, 0);
	info[6] = ch.sn_fused_levels; info[7] = ch.sn_split_levels;
	info[8] = ch.glevel_maxnr.empty() ? 0 : *std::max_element(ch.glevel_maxnr.begin(), ch.glevel_maxnr.end());
	info[9] = chol_err; info[10] = rs.floored;
	d2h(ctx, z, dz, ns * nrhs * sizeof(double));
	d2h(ctx, dot, ddot, (size_t)nseg * nrhs * sizeof(double));
	if (perm) d2h(ctx, perm, ch.perm, (size_t)m * sizeof(int));
	if (colptr) d2h(ctx, colptr, ch.colptr, (size_t)(m + 1) * sizeof(int));
	if (rowidx) d2h(ctx, rowidx, ch.rowidx, (size_t)ch.nnzL * sizeof(int));
	if (L) d2h(ctx, L, ch.L, (size_t)ch.nnzL * 36 * sizeof(double));
	if (Dinv) d2h(ctx, Dinv, ch.Dinv, (size_t)m * 36 * sizeof(double));
	if (dscale) d2h(ctx, dscale, ch.dscale, ns * sizeof(double));
	if (chol_err) LSFM_FAIL(LSFM_ERR_NOT_SPD, "the matrix is not positive definite (block column " + std::to_string(chol_err - 1) + " of the factor)");
	return LSFM_OK;
}

} // namespace lsfm
