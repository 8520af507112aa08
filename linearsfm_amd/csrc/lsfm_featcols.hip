// Columns of Sigma = I^-1 for chosen FEATURES and an exact gate for feature pairs (C ABI: lsfm_map_covariance_feature_columns,
// lsfm_map_feature_pair_gate).  No reference counterpart.
//
// One formulation serves both.  A column group a holds up to two signed features (f, +1)[, (g, -1)] and three columns, those of
// I^-1 (e_f - e_g):
//     B_a = - sum_(h,s) s W_h V_h^-1                 6 m x 3, non-zero on the rows of the poses that see f or g (fixed scalars zero)
//     X_a = S^-1 B_a                                 the pose rows: lsfm_covcols.hip's sweeps and refinement (cc_solve_refine)
//     Sigma_{h,a} = s_h V_h^-1 [h in a] - V_h^-1 sum_b W_bh^T X_a[p_b]          the feature rows (k_cc_feat<3>)
//     a pair:  Sigma_d = Var(x_f - x_g) = V_f^-1 + V_g^-1 + B_a^T X_a           a sum of positive semi-definite terms
// The pair's block Sigma_fg is off every pattern the library keeps; through the columns of the poses of f and g it would take
// 6 |P(f) u P(g)| columns and end in a cancelling sum of large marginals.  Here a pair costs 3 columns, nothing cancels, and the
// refinement's relative criterion acts on the scale of the difference.
//
// A chunk is 64 groups = 192 columns: the slabs and launch shapes of a full chunk of lsfm_map_covariance_columns.  The chunk loop
// is that call's too (cc_run, lsfm_cov.hpp, at width 3): the two entries below are its callables -- the right-hand sides k_fc_rhs, the
// kernels behind a chunk's solve and the downloads.  The column groups (FcGroups) and the gate of a chunk (fc_gate) are declared in
// lsfm_cov.hpp: lsfm_jointgate.hip solves the same columns.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lsfm_chol.hpp"
#include "lsfm_cov.hpp"
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_solve.hpp"

namespace lsfm {

namespace {

#define FC_KC (2 * CC_KC) /* column groups per chunk: 3 FC_KC = 6 CC_KC columns */
#define FC_SLOTS 7        /* W blocks a wave of k_fc_gate works on side by side: 9 lanes each */

// B of the chunk into the ZEROED slab B[6 M][R], R = 3 groups: one work-group per column group, lane (q, c) of 18 owns the scalar
// row q of every pose and column c of the group, walks the W blocks of f, then of g, and adds in that order.  A group owns its
// columns, so the only entries met twice -- a pose that sees both features, a pose stored twice in one feature's run -- are met
// by the same lane one after the other: no atomics.
__global__ void __launch_bounds__(LSFM_WAVE) k_fc_rhs(int R, const int* __restrict__ grp, const int* __restrict__ fptr, const int* __restrict__ photo,
                                                      const double* __restrict__ W, const double* __restrict__ IV, const unsigned char* __restrict__ fixed,
                                                      double* __restrict__ B)
{
	const int a = blockIdx.x, lane = threadIdx.x;
	if (lane >= 18) return;
	const int q = lane / 3, c = lane - 3 * q;
	for (int side = 0; side < 2; side++)
	{
		const int h = grp[2 * a + side];
		if (h < 0) continue;
		const double sgn = side ? 1.0 : -1.0; // B = -s W V^-1
		const double* iv = IV + (size_t)h * 9;
		for (int w = fptr[h]; w < fptr[h + 1]; w++)
		{
			const size_t row = (size_t)photo[w] * 6 + q;
			if (fixed && fixed[row]) continue;
			const double* wb = W + (size_t)w * 18 + q * 3;
			const double v = wb[0] * iv[c] + wb[1] * iv[3 + c] + wb[2] * iv[6 + c];
			B[row * R + 3 * a + c] += sgn * v;
		}
	}
}

// The gate of one pair per wave: T_h = sum_w W_w^T X_a[p_w] over the runs of f and g (lane (slot, l, j): every FC_SLOTS-th block,
// the slots summed in a fixed order), Sigma_d = V_f^-1 + V_g^-1 - V_f^-T T_f + V_g^-T T_g, symmetrised, a 3 x 3 Cholesky, d^2 =
// |L^-1 dx|^2.  A non-positive pivot: d^2 = NaN for this pair.
__global__ void __launch_bounds__(LSFM_WAVE) k_fc_gate(int R, const int* __restrict__ grp, const int* __restrict__ fptr, const int* __restrict__ photo,
                                                       const double* __restrict__ W, const double* __restrict__ IV, const double* __restrict__ Xo,
                                                       const double* __restrict__ dx, double* __restrict__ d2, double* __restrict__ cov)
{
	__shared__ double part[2][FC_SLOTS * 9];
	__shared__ double T[2][9];
	const int a = blockIdx.x, lane = threadIdx.x;
	const int slot = lane / 9, lj = lane - 9 * slot, l = lj / 3, j = lj - 3 * l;
	const int f = grp[2 * a], g = grp[2 * a + 1];
	if (slot < FC_SLOTS)
		for (int side = 0; side < 2; side++)
		{
			const int h = side ? g : f;
			double t = 0.0;
			for (int w = fptr[h] + slot; w < fptr[h + 1]; w += FC_SLOTS)
			{
				const double* wb = W + (size_t)w * 18 + l;
				const double* src = Xo + (size_t)photo[w] * 6 * R + 3 * a + j;
#pragma unroll
				for (int q = 0; q < 6; q++) t = fma(wb[q * 3], src[(size_t)q * R], t);
			}
			part[side][lane] = t;
		}
	__syncthreads();
	if (lane < 18)
	{
		const int side = lane / 9, e = lane - 9 * side;
		double t = 0.0;
		for (int sl = 0; sl < FC_SLOTS; sl++) t += part[side][sl * 9 + e];
		T[side][e] = t;
	}
	__syncthreads();
	if (lane != 0) return;
	const double *ivf = IV + (size_t)f * 9, *ivg = IV + (size_t)g * 9;
	double C[9];
	for (int i = 0; i < 3; i++)
		for (int jj = 0; jj < 3; jj++)
		{
			double bx = 0.0; // (B^T X)_ij
			for (int ll = 0; ll < 3; ll++) bx += ivg[ll * 3 + i] * T[1][ll * 3 + jj] - ivf[ll * 3 + i] * T[0][ll * 3 + jj];
			C[i * 3 + jj] = ivf[i * 3 + jj] + ivg[i * 3 + jj] + bx;
		}
	for (int i = 0; i < 3; i++)
		for (int jj = i + 1; jj < 3; jj++) C[i * 3 + jj] = C[jj * 3 + i] = 0.5 * (C[i * 3 + jj] + C[jj * 3 + i]);
	if (cov)
		for (int e = 0; e < 9; e++) cov[(size_t)a * 9 + e] = C[e];
	if (!d2) return;
	// C = L L^T;  y = L^-1 dx
	const double* x = dx + (size_t)a * 3;
	double res = NAN;
	const double p0 = C[0];
	if (p0 > 0.0)
	{
		const double l00 = sqrt(p0), l10 = C[3] / l00, l20 = C[6] / l00;
		const double p1 = C[4] - l10 * l10;
		if (p1 > 0.0)
		{
			const double l11 = sqrt(p1), l21 = (C[7] - l20 * l10) / l11;
			const double p2 = C[8] - l20 * l20 - l21 * l21;
			if (p2 > 0.0)
			{
				const double l22 = sqrt(p2);
				const double y0 = x[0] / l00, y1 = (x[1] - l10 * y0) / l11, y2 = (x[2] - l20 * y0 - l21 * y1) / l22;
				res = y0 * y0 + y1 * y1 + y2 * y2;
			}
		}
	}
	d2[a] = res;
}

} // namespace

// The column groups of a call on the device, and what the group calls hand cc_run (lsfm_cov.hpp) as the right-hand sides of a chunk.
void FcGroups::upload(lsfm_context* ctx, const std::vector<int>& grp)
{
	d = buf.get<int>(grp.size());
	h2d(ctx, d, grp.data(), grp.size() * sizeof(int));
}
CcChunkRhs FcGroups::rhs(lsfm_context* ctx) const
{
	return [this, ctx](int c0, int kcur, int R, const CovFront& fr, double* B) {
		const SolveIO& io = fr.io;
		dev_zero(ctx, B, (size_t)fr.ch.M * 6 * R * sizeof(double));
		hipLaunchKernelGGL(k_fc_rhs, dim3(kcur), dim3(LSFM_WAVE), 0, ctx->stream, R, of(c0), io.fptr, io.photo, io.W, fr.sy.IV, io.d_fixed, B);
	};
}
void fc_gate(lsfm_context* ctx, const CovFront& fr, int R, int kcur, const int* grp, const double* Xo, const double* dx, double* d2, double* cov)
{
	hipLaunchKernelGGL(k_fc_gate, dim3(kcur), dim3(LSFM_WAVE), 0, ctx->stream, R, grp, fr.io.fptr, fr.io.photo, fr.io.W, fr.sy.IV, Xo, dx, d2, cov);
}


int map_covariance_feature_columns(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* feats, int k, double* pose_cols, double* feat_cols,
                                   double* joint, int* steps_out, double* last_corr, double* times)
{
	const int m = map->m, n = map->n;
	std::vector<int> grp(2 * (size_t)k);
	{
		std::vector<char> seen(std::max(n, 1), 0);
		for (int a = 0; a < k; a++)
		{
			if (feats[a] < 0 || feats[a] >= n) LSFM_FAIL(LSFM_ERR_ARG, "requested feature " + std::to_string(feats[a]) + " is not one of the map's " + std::to_string(n));
			if (seen[feats[a]]) LSFM_FAIL(LSFM_ERR_ARG, "feature " + std::to_string(feats[a]) + " is requested twice");
			seen[feats[a]] = 1;
			grp[2 * a] = feats[a];
			grp[2 * a + 1] = -1;
		}
	}
	const int kc = std::min(k, FC_KC);
	const size_t nF = feat_cols ? (size_t)n * 9 * kc : 0, nJ = joint ? (size_t)kc * k * 9 : 0;
	FcGroups dg;
	DevBuf bF, bJ, bQ;
	double *F = nullptr, *Jd = nullptr;
	int* dq = nullptr;
	std::vector<double> hj(nJ);
	int own_steps = 0;
	int& steps = steps_out ? *steps_out : own_steps; // (> 0: the results were written)
	const int rc = cc_run(ctx, map, mono, CcCall{ k, 3, FC_KC, nF + nJ, "features or pairs" }, &steps, last_corr, times,
		[&](const CovFront&) {
			dg.upload(ctx, grp);
			if (feat_cols) F = bF.get<double>(nF);
			if (!joint) return;
			Jd = bJ.get<double>(nJ);
			dq = bQ.get<int>(k);
			h2d(ctx, dq, feats, (size_t)k * sizeof(int));
		},
		dg.rhs(ctx), nullptr,
		[&](int c0, int kcur, int R, const CovFront& fr, CcWork& wk) {
			if (pose_cols) cc_pose_out(ctx, 3, m, R, wk.Xo, wk.Y);
			if (feat_cols) cc_feat(ctx, 3, fr, R, nullptr, n, dg.of(c0), wk.Xo, F);
			if (joint) cc_feat(ctx, 3, fr, R, dq, k, dg.of(c0), wk.Xo, Jd); // the rows of the k requested features alone
		},
		[&](int c0, int kcur, int R, CcWork& wk) {
			if (pose_cols) d2h(ctx, pose_cols + (size_t)c0 * m * 18, wk.Y, (size_t)m * 6 * R * sizeof(double));
			if (feat_cols) d2h(ctx, feat_cols + (size_t)c0 * n * 9, F, (size_t)kcur * n * 9 * sizeof(double));
			if (!joint) return;
			d2h(ctx, hj.data(), Jd, (size_t)kcur * k * 9 * sizeof(double));
			for (int a = 0; a < kcur; a++)
				for (int b = 0; b < k; b++)
					for (int i = 0; i < 3; i++) memcpy(&joint[((size_t)3 * b + i) * 3 * k + 3 * (size_t)(c0 + a)], &hj[((size_t)a * k + b) * 9 + 3 * i], 3 * sizeof(double));
		});
	if (joint && steps > 0) symmetrise_joint(joint, k, 3);
	return rc;
}

int map_feature_pair_gate(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* pairs, int K, double* d2, double* cov_diff, int* steps_out,
                          double* last_corr, double* times)
{
	const int m = map->m, n = map->n;
	std::vector<int> grp(pairs, pairs + 2 * (size_t)K);
	std::vector<double> dx(3 * (size_t)K);
	for (int a = 0; a < K; a++)
	{
		const int f = grp[2 * a], g = grp[2 * a + 1];
		if (f < 0 || f >= n || g < 0 || g >= n) LSFM_FAIL(LSFM_ERR_ARG, "pair " + std::to_string(a) + " (" + std::to_string(f) + ", " + std::to_string(g) + ") names a feature that is not one of the map's " + std::to_string(n));
		if (f == g) LSFM_FAIL(LSFM_ERR_ARG, "pair " + std::to_string(a) + " names feature " + std::to_string(f) + " twice");
		for (int i = 0; i < 3; i++) dx[3 * (size_t)a + i] = map->stVal[(size_t)6 * m + 3 * (size_t)f + i] - map->stVal[(size_t)6 * m + 3 * (size_t)g + i];
	}
	const int kc = std::min(K, FC_KC);
	FcGroups dg;
	DevBuf bX, bD, bC;
	double *ddx = nullptr, *dd2 = nullptr, *dcov = nullptr;
	return cc_run(ctx, map, mono, CcCall{ K, 3, FC_KC, 13 * (size_t)K, "features or pairs" }, steps_out, last_corr, times,
		[&](const CovFront&) {
			dg.upload(ctx, grp);
			ddx = bX.get<double>(3 * (size_t)K);
			h2d(ctx, ddx, dx.data(), 3 * (size_t)K * sizeof(double));
			if (d2) dd2 = bD.get<double>(kc);
			if (cov_diff) dcov = bC.get<double>(9 * (size_t)kc);
		},
		dg.rhs(ctx), nullptr,
		[&](int c0, int kcur, int R, const CovFront& fr, CcWork& wk) {
			fc_gate(ctx, fr, R, kcur, dg.of(c0), wk.Xo, ddx + 3 * (size_t)c0, dd2, dcov);
		},
		[&](int c0, int kcur, int R, CcWork&) {
			if (d2) d2h(ctx, d2 + c0, dd2, (size_t)kcur * sizeof(double));
			if (cov_diff) d2h(ctx, cov_diff + 9 * (size_t)c0, dcov, 9 * (size_t)kcur * sizeof(double));
		});
}

} // namespace lsfm
