// Marginal covariances of a map's information matrix I = [U W; W^T V] (C ABI: lsfm_map_covariance).  No reference counterpart: the
// reference keeps the matrix and never inverts it.
//
// The camera system S = U - W V^-1 W^T is reduced and factored by the same pieces as a tree level (K9, lsfm_symbolic.cpp, CholDev:
// lsfm_chol.hpp), always in fp64 and always on the sparse path.  The factor is of A = D^-1/2 P S P^T D^-1/2 = L L^T.  Selected
// inversion (Takahashi's recurrences) then gives Z = A^-1 on struct(L), the columns in reverse elimination order.  For column j with
// below-diagonal rows I:
//     Y    = L_Ij L_jj^-1                   (k_selinv_y: every column at once, in place of L_Ij)
//     Z_Ij = -Z_II Y                        (k_selinv_off)
//     Z_jj = L_jj^-T L_jj^-1 - Z_Ij^T Y     (k_selinv_diag)
// Every Z_ik that Z_II needs (i, k in I) lies on struct(L) in a column after j.  The columns of one elimination-tree level only read
// their ancestors' columns, so a level is one launch of each kernel, from the root down (the narrow top, CholDev's tail, a column
// at a time).  Every sum runs in a fixed order in one lane: the result is the same bits on every call.
// Sigma = P^T D^-1/2 Z D^-1/2 P on S's upper pattern (k_cov_pairs), then per feature (k_cov_feat, one wave per feature)
//     Sigma_ff = V_f^-1 + V_f^-1 (sum_{a,b} W_af^T Sigma_{p_a p_b} W_bf) V_f^-1.
// The front end -- argument checks and upload (lsfm_system.hpp), reduction, factorisation -- is cov_front (lsfm_cov.hpp), shared with
// lsfm_map_marginalise_poses and, as cov_front_rowsorted (with the row-sorted block list and the status read), with the columns calls
// (lsfm_covcols.hip, lsfm_featcols.hip) and the merge (lsfm_merge.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lsfm_chol.hpp"
#include "lsfm_cov.hpp"
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_solve.hpp"
#include "lsfm_system.hpp"

namespace lsfm {

namespace {

// block (row, col) of struct(L) -- closed under the recurrence, so it is there; a miss (a broken pattern) reads block `col`'s diagonal
// instead and raises *err rather than reading past the column
__device__ __forceinline__ int find_block(const int* __restrict__ colptr, const int* __restrict__ rowidx, int lo, int col, int row, int* err)
{
	const int hi = colptr[col + 1];
	const int pos = find_row(rowidx, lo, hi, row);
	if (pos < hi && rowidx[pos] == row) return pos;
	atomicExch(err, 2);
	return colptr[col];
}

// Y = L_Ij L_jj^-1 in place of L_Ij, one work-group per column (Dinv: L_jj^-1, lower triangular)
__global__ void __launch_bounds__(64) k_selinv_y(int M, const int* __restrict__ colptr, const double* __restrict__ Dinv, double* __restrict__ L)
{
	__shared__ double sD[36];
	const int j = blockIdx.x;
	if (threadIdx.x < 36) sD[threadIdx.x] = Dinv[(size_t)j * 36 + threadIdx.x];
	__syncthreads();
	const int c0 = colptr[j], n = colptr[j + 1] - c0 - 1;
	for (int w = threadIdx.x; w < n * 6; w += blockDim.x)
	{
		double* row = L + (size_t)(c0 + 1 + w / 6) * 36 + (w % 6) * 6;
		double a[6];
		ld<6>(a, row);
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			double s = 0.0;
#pragma unroll
			for (int t = c; t < 6; t++) s = fma(a[t], sD[t * 6 + c], s);
			row[c] = s;
		}
	}
}

// Z_Ij = -Z_II Y for the columns cols[0 .. gridDim.x): work-group (x, y) takes the output blocks [y SELINV_RB, (y + 1) SELINV_RB) of
// column cols[x], one lane per (block, row); the k-sum runs in ascending k in every lane, Y staged through LDS in chunks
#define SELINV_THREADS 256
#define SELINV_RB (SELINV_THREADS / 6)
#define SELINV_KC 32
__global__ void __launch_bounds__(SELINV_THREADS) k_selinv_off(const int* __restrict__ cols, const int* __restrict__ colptr, const int* __restrict__ rowidx,
                                                               const double* __restrict__ Y, double* __restrict__ Z, int* __restrict__ err)
{
	__shared__ double sY[SELINV_KC * 36];
	__shared__ int sRow[SELINV_KC];
	const int j = cols[blockIdx.x];
	const int c0 = colptr[j], n = colptr[j + 1] - c0 - 1;
	const int b0 = blockIdx.y * SELINV_RB;
	if (b0 >= n) return; // (uniform over the work-group)
	const int tid = threadIdx.x, ii = tid / 6, r = tid - 6 * ii;
	const int bi = b0 + ii;
	const bool act = ii < SELINV_RB && bi < n;
	const int gi = act ? rowidx[c0 + 1 + bi] : 0;
	const int gi0 = act ? colptr[gi] : 0;
	double acc[6] = { 0, 0, 0, 0, 0, 0 };
	int from = gi0; // (column gi's rows ascend: the blocks (k, gi), k > gi, come in ascending k)
	for (int k0 = 0; k0 < n; k0 += SELINV_KC)
	{
		const int nk = min(SELINV_KC, n - k0);
		__syncthreads();
		for (int q = tid; q < nk * 36; q += SELINV_THREADS) sY[q] = Y[(size_t)(c0 + 1 + k0) * 36 + q];
		if (tid < nk) sRow[tid] = rowidx[c0 + 1 + k0 + tid];
		__syncthreads();
		if (!act) continue;
		for (int kk = 0; kk < nk; kk++)
		{
			const int gk = sRow[kk];
			double z[6];
			if (gi >= gk)
			{
				// Z(i, k): column gk holds row gi
				const int pos = find_block(colptr, rowidx, colptr[gk], gk, gi, err);
				ld<6>(z, Z + (size_t)pos * 36 + r * 6);
			}
			else
			{
				// Z(i, k) = Z(k, i)^T: column gi holds row gk
				const int pos = find_block(colptr, rowidx, from, gi, gk, err);
				from = max(from, pos);
				const double* b = Z + (size_t)pos * 36 + r;
#pragma unroll
				for (int t = 0; t < 6; t++) z[t] = b[t * 6];
			}
			const double* y = sY + kk * 36;
#pragma unroll
			for (int c = 0; c < 6; c++)
			{
				double s = acc[c];
#pragma unroll
				for (int t = 0; t < 6; t++) s = fma(z[t], y[t * 6 + c], s);
				acc[c] = s;
			}
		}
	}
	if (act)
	{
		double* o = Z + (size_t)(c0 + 1 + bi) * 36 + r * 6;
#pragma unroll
		for (int c = 0; c < 6; c++) o[c] = -acc[c];
	}
}

// Z_jj = L_jj^-T L_jj^-1 - Z_Ij^T Y, one work-group per column, lane 6 r + c owns element (r, c); stored symmetric
__global__ void __launch_bounds__(64) k_selinv_diag(const int* __restrict__ cols, const int* __restrict__ colptr, const double* __restrict__ Dinv,
                                                    const double* __restrict__ Y, double* __restrict__ Z)
{
	__shared__ double sA[36];
	const int j = cols[blockIdx.x];
	const int c0 = colptr[j], n = colptr[j + 1] - c0 - 1;
	const int tid = threadIdx.x, r = tid / 6, c = tid - 6 * (tid / 6);
	if (tid < 36)
	{
		const double* D = Dinv + (size_t)j * 36;
		double s = 0.0;
		for (int t = 0; t < 6; t++) s = fma(D[t * 6 + r], D[t * 6 + c], s);
		double u = 0.0;
		for (int b = 0; b < n; b++)
		{
			const double* zb = Z + (size_t)(c0 + 1 + b) * 36;
			const double* yb = Y + (size_t)(c0 + 1 + b) * 36;
#pragma unroll
			for (int t = 0; t < 6; t++) u = fma(zb[t * 6 + r], yb[t * 6 + c], u);
		}
		sA[tid] = s - u;
	}
	__syncthreads();
	if (tid < 36) Z[(size_t)c0 * 36 + tid] = r == c ? sA[tid] : 0.5 * (sA[tid] + sA[c * 6 + r]);
}

// Sigma on S's upper pattern (old numbering, unscaled): block e of the pattern is (p, q), p <= q; one lane per (block, row); the
// fixed scalars' rows and columns are 0
__global__ void k_cov_pairs(int nnzb, const unsigned long long* __restrict__ keys, const int* __restrict__ pinv, const int* __restrict__ colptr,
                            const int* __restrict__ rowidx, const double* __restrict__ Z, const double* __restrict__ dscale,
                            const unsigned char* __restrict__ fixed, double* __restrict__ out, int* __restrict__ err)
{
	const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= (long)nnzb * 6) return;
	const int e = (int)(w / 6), r = (int)(w - 6L * e);
	const unsigned long long key = keys[e];
	const int p = (int)(key >> 32), q = (int)(key & 0xffffffffull);
	const int i = pinv[p], j = pinv[q];
	const bool tr = i < j; // Z(i, j) = Z(j, i)^T
	const int col = tr ? i : j, row = tr ? j : i;
	const int pos = find_block(colptr, rowidx, colptr[col], col, row, err);
	const double* b = Z + (size_t)pos * 36;
	const double si = dscale[(size_t)i * 6 + r];
	const bool fr = fixed && fixed[(size_t)p * 6 + r];
	double* o = out + (size_t)e * 36 + r * 6;
#pragma unroll
	for (int c = 0; c < 6; c++)
	{
		const double z = tr ? b[c * 6 + r] : b[r * 6 + c];
		const bool fc = fixed && fixed[(size_t)q * 6 + c];
		o[c] = (fr || fc) ? 0.0 : si * z * dscale[(size_t)j * 6 + c];
	}
}

// Sigma_ff, one wave per feature: the lanes take the pairs (a, b) of the feature's W blocks in turn, the wave sums them in a fixed tree
#define COV_FEAT_THREADS 256
__global__ void __launch_bounds__(COV_FEAT_THREADS) k_cov_feat(int NF, const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W,
                                                               const double* __restrict__ IV, const double* __restrict__ P, const unsigned long long* __restrict__ tab,
                                                               const int* __restrict__ hval, unsigned long long mask, double* __restrict__ out, int* __restrict__ err)
{
	const int f = blockIdx.x * (COV_FEAT_THREADS / LSFM_WAVE) + threadIdx.x / LSFM_WAVE;
	if (f >= NF) return; // (uniform over the wave)
	const int lane = threadIdx.x & (LSFM_WAVE - 1);
	const int w0 = fptr[f], nf = fptr[f + 1] - w0;
	double acc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	for (long t = lane; t < (long)nf * nf; t += LSFM_WAVE)
	{
		const int a = (int)(t / nf), b = (int)(t - (long)a * nf);
		const int pa = photo[w0 + a], pb = photo[w0 + b];
		const int e = hash_find(tab, hval, mask, pair_key(pa, pb));
		if (e < 0) { atomicExch(err, 1); continue; }
		const bool tr = pa > pb; // the stored block is Sigma(min, max)
		const double* sg = P + (size_t)e * 36;
		double wb[18], T[18];
		ld<18>(wb, W + (size_t)(w0 + b) * 18);
		// T = Sigma_{pa pb} W_b (6x3)
#pragma unroll
		for (int r = 0; r < 6; r++)
#pragma unroll
			for (int c = 0; c < 3; c++)
			{
				double s = 0.0;
#pragma unroll
				for (int k = 0; k < 6; k++) s = fma(tr ? sg[k * 6 + r] : sg[r * 6 + k], wb[k * 3 + c], s);
				T[r * 3 + c] = s;
			}
		double wa[18];
		ld<18>(wa, W + (size_t)(w0 + a) * 18);
		mtm<6, 3, 3, true>(wa, T, acc);
	}
#pragma unroll
	for (int q = 0; q < 9; q++)
	{
		double v = acc[q];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, LSFM_WAVE);
		acc[q] = v;
	}
	if (lane == 0)
	{
		double iv[9], tmp[9], s[9];
		ld<9>(iv, IV + (size_t)f * 9);
		// Sigma_ff = IV + IV acc IV (IV symmetric)
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 3; c++)
			{
				double x = 0.0;
#pragma unroll
				for (int k = 0; k < 3; k++) x = fma(acc[r * 3 + k], iv[k * 3 + c], x);
				tmp[r * 3 + c] = x;
			}
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 3; c++)
			{
				double x = 0.0;
#pragma unroll
				for (int k = 0; k < 3; k++) x = fma(iv[r * 3 + k], tmp[k * 3 + c], x);
				s[r * 3 + c] = iv[r * 3 + c] + x;
			}
		double* o = out + (size_t)f * 9;
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 3; c++) o[r * 3 + c] = r == c ? s[r * 3 + c] : 0.5 * (s[r * 3 + c] + s[c * 3 + r]);
	}
}

} // namespace

void cov_front(lsfm_context* ctx, const lsfm_map* map, bool mono, CovFront& fr)
{
	const int m = map->m;
	// ---- arguments (host) ----
	HostSystem h = host_system_of(*map, true);
	h.pose_origin = map->pose_origin;
	const std::vector<int> fptr = system_fptr(h);
	std::vector<unsigned char> fx;
	if (mono)
	{
		// the gauge of lsfm_solve_mono / lsfm_gn_polish: the 6 scalars of pose Ref and scalar Fix of pose ScaP (labels: stno = -id)
		int pr = -1, ps = -1;
		for (int p = 0; p < m; p++)
		{
			if (-map->stno[6 * p] == map->Ref) pr = p;
			if (-map->stno[6 * p] == map->ScaP) ps = p;
		}
		if (pr < 0 || ps < 0 || map->Fix < 0 || map->Fix > 2) LSFM_FAIL(LSFM_ERR_ARG, "Mono map: its Ref / ScaP pose is not in its state or Fix is not 0..2");
		fx = gauge_mask(m, pr, ps * 6 + map->Fix);
	}
	// ---- upload (lsfm_system.hip; the right-hand side is not used) ----
	SolveIO& io = fr.io;
	system_upload(ctx, h, SYS_VALUES | SYS_RHS_0, fptr, mono ? &fx : nullptr, io);
	hipStream_t s = ctx->stream;
	hipEvent_t* ev = fr.ev;
	for (int k = 0; k < 3; k++) ev[k] = ctx->pool_event();
	LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	// ---- reduce + factor: the tree level's own pieces, fp64, sparse path ----
	SchurSystem& sy = fr.sy;
	CholDev& ch = fr.ch;
	CholHostIn hin;
	schur_vinv(ctx, io, sy);
	build_schur_pattern(ctx, io, sy);
	chol_fetch(ctx, sy, io.d_pose_origin, hin);
	build_schur_values(ctx, io, sy);
	chol_analyse(ctx, sy, hin, ch);
	LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	// the count of floored pivots goes to a record of this call's own (a tree's record stays as its run left it)
	RunStatsDev* d_run = fr.d_run = ctx->scratch.alloc<RunStatsDev>(1);
	dev_zero(ctx, d_run, sizeof(RunStatsDev));
	{
		struct Swap { lsfm_context* c; RunStatsDev* keep; ~Swap() { c->d_run = keep; } } swap{ ctx, ctx->d_run };
		ctx->d_run = d_run;
		chol_scatter(ctx, sy, io.d_fixed, ch);
		chol_factor(ctx, sy, io.d_fixed, ch, nullptr);
	}
	chol_merge_groups(ctx, ch);
	LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
}

int cov_front_status(lsfm_context* ctx, const CovFront& fr)
{
	int chol_err = 0;
	RunStatsDev rs;
	d2h(ctx, &chol_err, fr.ch.d_err, sizeof(int));
	d2h(ctx, &rs, fr.d_run, sizeof rs);
	if (chol_err) LSFM_FAIL(LSFM_ERR_NOT_SPD, "the camera system is not positive definite (block column " + std::to_string(chol_err - 1) + " of the factor)");
	return rs.floored;
}

int cov_front_rowsorted(lsfm_context* ctx, const lsfm_map* map, bool mono, CovFront& fr)
{
	{
		// the residual needs the row-sorted list of S's blocks whatever product the context's CG is set to (lsfm_set_spmv_variant)
		struct Keep { lsfm_context* c; int v; ~Keep() { c->pcg.spmv_variant = v; } } keep{ ctx, ctx->pcg.spmv_variant };
		ctx->pcg.spmv_variant = 2;
		cov_front(ctx, map, mono, fr);
	}
	LSFM_CHECK_HIP(hipGetLastError());
	const int floored = cov_front_status(ctx, fr);
	if (floored == 0 && !fr.sy.gent) LSFM_FAIL(LSFM_ERR_INTERNAL, "the camera system has no row-sorted block list");
	return floored;
}

int map_covariance(lsfm_context* ctx, const lsfm_map* map, bool mono, double* pose_cov, double* feat_cov, double* pair_cov, int cap_blocks, int* nnzb_out,
                   double* times)
{
	CovFront fr;
	cov_front(ctx, map, mono, fr);
	const int m = map->m, n = map->n;
	const SolveIO& io = fr.io;
	const SchurSystem& sy = fr.sy;
	CholDev& ch = fr.ch;
	hipStream_t s = ctx->stream;
	const double* dW = io.W; const int *dph = io.photo, *dfp = io.fptr;
	const int nnzb = sy.nnzb;
	*nnzb_out = nnzb;
	if (pair_cov && nnzb > cap_blocks) LSFM_FAIL(LSFM_ERR_ARG, "pair_cov too small for the pattern (" + std::to_string(nnzb) + " blocks)");
	hipEvent_t ev[5] = { fr.ev[0], fr.ev[1], fr.ev[2], ctx->pool_event(), ctx->pool_event() };
	// ---- selected inversion ----
	const int M = ch.M;
	std::vector<int> hcolptr(M + 1), horder(M);
	d2h(ctx, hcolptr.data(), ch.colptr, (size_t)(M + 1) * sizeof(int));
	d2h(ctx, horder.data(), ch.order, (size_t)M * sizeof(int));
	DevBuf zbuf, pbuf, fbuf;
	double* Z = zbuf.get<double>((size_t)ch.nnzL * 36);
	double* dP = pbuf.get<double>((size_t)nnzb * 36);
	double* dF = fbuf.get<double>((size_t)n * 9);
	int* d_ferr = ctx->scratch.alloc<int>(1);
	dev_zero(ctx, d_ferr, sizeof(int));
	hipLaunchKernelGGL(k_selinv_y, dim3(M), dim3(64), 0, s, M, ch.colptr, ch.Dinv, ch.L);
	auto level = [&](int first, int count) {
		int most = 0;
		for (int q = first; q < first + count; q++) most = std::max(most, hcolptr[horder[q] + 1] - hcolptr[horder[q]] - 1);
		if (most > 0) hipLaunchKernelGGL(k_selinv_off, dim3(count, (most + SELINV_RB - 1) / SELINV_RB), dim3(SELINV_THREADS), 0, s, ch.order + first, ch.colptr, ch.rowidx, ch.L, Z, d_ferr);
		hipLaunchKernelGGL(k_selinv_diag, dim3(count), dim3(64), 0, s, ch.order + first, ch.colptr, ch.Dinv, ch.L, Z);
	};
	for (int q = M - 1; q >= ch.tail_begin; q--) level(q, 1); // the tail: ascending column index = a topological order
	for (int l = ch.nlevels - 1; l >= 0; l--)
	{
		const int c = ch.level_ptr[l + 1] - ch.level_ptr[l];
		if (c) level(ch.level_ptr[l], c);
	}
	if (nnzb)
		hipLaunchKernelGGL(k_cov_pairs, dim3((unsigned)(((size_t)nnzb * 6 + 255) / 256)), dim3(256), 0, s, nnzb, sy.upper_keys, ch.pinv, ch.colptr, ch.rowidx, Z, ch.dscale,
		                   io.d_fixed, dP, d_ferr);
	LSFM_CHECK_HIP(hipEventRecord(ev[3], s));
	// ---- features ----
	if (n && feat_cov)
		hipLaunchKernelGGL(k_cov_feat, dim3((n + COV_FEAT_THREADS / LSFM_WAVE - 1) / (COV_FEAT_THREADS / LSFM_WAVE)), dim3(COV_FEAT_THREADS), 0, s, n, dfp, dph, dW, sy.IV, dP,
		                   sy.tab, sy.hval, sy.mask, dF, d_ferr);
	LSFM_CHECK_HIP(hipEventRecord(ev[4], s));
	LSFM_CHECK_HIP(hipGetLastError());
	// ---- status: the factor's pivot word and the floored pivots, read once ----
	int ferr = 0;
	d2h(ctx, &ferr, d_ferr, sizeof(int));
	if (times)
		for (int k = 0; k < 4; k++) times[k] = event_ms(ev[k], ev[k + 1]);
	const int floored = cov_front_status(ctx, fr);
	if (floored > 0) return floored; // the factor is of a perturbed S: nothing is written
	if (ferr) LSFM_FAIL(LSFM_ERR_INTERNAL, ferr == 2 ? "a block of the selected inversion is not on the factor's pattern" : "a feature's pose pair is not in the camera system's pattern");
	std::vector<double> hp((size_t)nnzb * 36);
	d2h(ctx, hp.data(), dP, hp.size() * sizeof(double));
	if (pair_cov) memcpy(pair_cov, hp.data(), hp.size() * sizeof(double));
	if (pose_cov)
	{
		std::vector<int> rowptr(m + 1);
		d2h(ctx, rowptr.data(), sy.rowptr, (size_t)(m + 1) * sizeof(int));
		for (int p = 0; p < m; p++) memcpy(pose_cov + (size_t)p * 36, hp.data() + (size_t)rowptr[p] * 36, 36 * sizeof(double));
	}
	if (feat_cov && n) d2h(ctx, feat_cov, dF, (size_t)n * 9 * sizeof(double));
	return LSFM_OK;
}

} // namespace lsfm
