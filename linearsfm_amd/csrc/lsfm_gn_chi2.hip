// Gauss-Newton polish (lsfm_gn.hpp): chi^2 of the local maps and of their single features at the frames of k_gn_hubs and the pose
// residuals of k_gn_poses, the M-estimators' weights and objectives, and the correction of U that the feature weights need
// (lsfm_map_chi2, lsfm_gn_polish_robust, lsfm_map_feature_chi2, lsfm_gn_polish_robust_features, lsfm_gn_linearise_features).  No sum here uses an atomic: the same
// state gives the same bits.
#include "lsfm_device.hpp"
#include "lsfm_gn.hpp"

namespace lsfm {

// chi2_k = r_k^T I_k r_k = sum_U (2 - delta_ab) r_a^T U_ab r_b + 2 sum_W r_a^T W_af r_f + sum_f r_f^T V_f r_f over map k's own blocks.
// With g_f = V_f r_f + sum_a W_af^T r_a it splits into a pose part under the map's own Schur complement and one conditional term per
// feature:  chi2_k = r_p^T (U - sum_f W_f V_f^-1 W_f^T) r_p + sum_f c_kf,  c_kf = g_f^T V_f^-1 g_f >= 0.  Scaling the conditional term of f
// by w_f is the information matrix  I_k(w) = [U - sum_f (1 - w_f) W_f V_f^-1 W_f^T, w_f W_f; w_f W_f^T, w_f V_f]  (w = 1: I_k, w_f = 0: f
// marginalised out), so IRLS on c_kf is the plain step on re-weighted maps: k_gn_features<NH, true> scales W and V, the correction of U
// goes into slots of its own behind the map's U blocks (k_gn_feature_ufill) and k_gn_ublocks places them like any other.

// the M-estimator at s: w = rho'(s).  kind 0: rho(s) = s, 1 Huber, 2 Cauchy with threshold c
__device__ __forceinline__ void gn_rho(int kind, double c, double s, double& w, double& rho)
{
	const double c2 = c * c;
	w = 1.0; rho = s;
	if (kind == 1)
	{
		const bool in = s <= c2;
		w = in ? 1.0 : c / sqrt(s);
		rho = in ? s : 2.0 * c * sqrt(s) - c2;
	}
	else if (kind == 2)
	{
		w = 1.0 / (1.0 + s / c2);
		rho = c2 * log1p(s / c2);
	}
}

// V = L L^T of a 3x3 block in registers (lower triangle read): L = l00 l10 l11 l20 l21 l22; false when V is not positive definite
__device__ __forceinline__ bool gn_chol3(const double* V, double* L)
{
	bool ok = V[0] > 0.0;
	L[0] = sqrt(V[0]);
	L[1] = V[3] / L[0]; L[3] = V[6] / L[0];
	const double d1 = V[4] - L[1] * L[1];
	ok = ok && d1 > 0.0;
	L[2] = sqrt(d1);
	L[4] = (V[7] - L[3] * L[1]) / L[2];
	const double d2 = V[8] - L[3] * L[3] - L[4] * L[4];
	ok = ok && d2 > 0.0;
	L[5] = sqrt(d2);
	return ok;
}
// y = L^-1 g
__device__ __forceinline__ void gn_lsolve3(const double* L, const double* g, double* y)
{
	y[0] = g[0] / L[0];
	y[1] = (g[1] - L[1] * y[0]) / L[2];
	y[2] = (g[2] - L[3] * y[0] - L[4] * y[1]) / L[5];
}

// U block i's (2 - delta_ab) r_a^T U_ab r_b
__device__ __forceinline__ double gn_u_term(int i, const double* __restrict__ U, const int* __restrict__ Ui, const int* __restrict__ Uj, const double* __restrict__ rp)
{
	const int a = Ui[i], b = Uj[i];
	double Ub[36], ra[6], rb[6], y[6];
	ld<36>(Ub, U + (size_t)i * 36);
	ld<6>(ra, rp + (size_t)a * 6);
	ld<6>(rb, rp + (size_t)b * 6);
	mm<6, 6, 1, false>(Ub, rb, y);
	double d = 0.0;
#pragma unroll
	for (int q = 0; q < 6; q++) d += ra[q] * y[q];
	return a == b ? d : 2.0 * d;
}
// feature instance f's r_f^T V_f r_f + 2 sum_a r_a^T W_af r_f; the residual is recomputed here (f = R (x_f - t) / Scale, as gn_trans forms
// it): k_gn_features, which forms it too, runs after the weights are set.  FEAT: Vb = V_f and g = g_f as well (without: g = V_f r_f)
template <bool FEAT>
__device__ __forceinline__ double gn_feature_term(const GnMap& t, int f, const double* __restrict__ rp, const int* __restrict__ gf, const double* __restrict__ xf,
                                                  const double* __restrict__ fhat, const int* __restrict__ fptr, const int* __restrict__ photo,
                                                  const double* __restrict__ W, const double* __restrict__ V, double* Vb, double* g)
{
	const double* xn = xf + (size_t)gf[f] * 3;
	double t222[3] = { xn[0] - t.t[0], xn[1] - t.t[1], xn[2] - t.t[2] }, t22[3], rf[3];
	mv3(t.R, t222, t22);
#pragma unroll
	for (int r = 0; r < 3; r++) rf[r] = fhat[(size_t)f * 3 + r] - t22[r] / t.Scale;
	ld<9>(Vb, V + (size_t)f * 9);
	mm<3, 3, 1, false>(Vb, rf, g);
	double d = rf[0] * g[0] + rf[1] * g[1] + rf[2] * g[2];
	for (int j = fptr[f]; j < fptr[f + 1]; j++)
	{
		double Wb[18], ra[6], z[6];
		ld<18>(Wb, W + (size_t)j * 18);
		ld<6>(ra, rp + (size_t)photo[j] * 6);
		mm<6, 3, 1, false>(Wb, rf, z);
		double e = 0.0;
#pragma unroll
		for (int q = 0; q < 6; q++) e += ra[q] * z[q];
		d += 2.0 * e;
		if (FEAT) mtm<6, 3, 1, true>(Wb, ra, g);
	}
	return d;
}

// One work-group per map, reading every U, W and V block of the map once: its lanes stride over the map's OWN U blocks (nu_own: the
// correction slots behind them are not part of I_k) and over its features (each with its run of W), every lane sums in a fixed order,
// then block_sum_fixed.  256 lanes: a map of the NC3500-like set holds 520-763 W blocks (one per feature), one of the RS468-like set
// 1200-1882 over 600-941 features -- two to four features per lane.
// FEAT = false: chi2_k into out[k].  FEAT = true: per feature c_kf and its weight w_kf = rho'(c_kf / 3) (gn_rho), per map chi2_k,
// sum_f c_kf and sum_f rho(c_kf / 3) into out[3 k ..]; bad: the smallest feature instance whose V is not positive definite (an integer
// minimum: the same for every order).  GIVEN (with FEAT; lsfm_gn_linearise_features): no estimator -- fweight is read, not written, and
// the third sum is sum_f w_kf c_kf; kind and c are unused.  The two earlier instantiations are what they were.
#define GN_CHI2_LANES 256
template <bool FEAT, bool GIVEN = false>
__global__ void __launch_bounds__(GN_CHI2_LANES)
k_gn_chi2(int kind, double c, const GnMap* __restrict__ gm, const double* __restrict__ U, const int* __restrict__ Ui, const int* __restrict__ Uj,
          const double* __restrict__ rp, const int* __restrict__ gf, const double* __restrict__ xf, const double* __restrict__ fhat,
          const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W, const double* __restrict__ V, double* __restrict__ out,
          double* __restrict__ fchi2, double* __restrict__ fweight, int* __restrict__ bad)
{
	__shared__ double part[FEAT ? 3 : 1][GN_CHI2_LANES / LSFM_WAVE];
	const int k = blockIdx.x;
	const GnMap& t = gm[k];
	double acc = 0.0, accc = 0.0, accr = 0.0;
	for (int i = t.u0 + (int)threadIdx.x; i < t.u0 + t.nu_own; i += GN_CHI2_LANES) acc += gn_u_term(i, U, Ui, Uj, rp);
	for (int f = t.f0 + (int)threadIdx.x; f < t.f0 + t.n; f += GN_CHI2_LANES)
	{
		double Vb[9], g[3];
		acc += gn_feature_term<FEAT>(t, f, rp, gf, xf, fhat, fptr, photo, W, V, Vb, g);
		if (FEAT)
		{
			double L[6], y[3], w, rho;
			if (!gn_chol3(Vb, L)) atomicMin(bad, f);
			gn_lsolve3(L, g, y);
			const double cf = y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
			if (GIVEN) { w = fweight[f]; rho = w * cf; }
			else gn_rho(kind, c, cf / 3.0, w, rho);
			fchi2[f] = cf;
			if (!GIVEN) fweight[f] = w;
			accc += cf; accr += rho;
		}
	}
	acc = block_sum_fixed<GN_CHI2_LANES>(acc, part[0]);
	if (FEAT)
	{
		accc = block_sum_fixed<GN_CHI2_LANES>(accc, part[FEAT ? 1 : 0]);
		accr = block_sum_fixed<GN_CHI2_LANES>(accr, part[FEAT ? 2 : 0]);
		if (threadIdx.x == 0) { out[(size_t)3 * k] = acc; out[(size_t)3 * k + 1] = accc; out[(size_t)3 * k + 2] = accr; }
	}
	else if (threadIdx.x == 0) out[k] = acc;
}

// one work-group: s_k = chi2_k / dof_k, w_k = rho'(s_k) into the maps' frames (the next assembly's weights) and weight[k], and
// G = sum_k dof_k rho(s_k) summed in a fixed order (lane-strided, block_sum_fixed).  kind 1 Huber, 2 Cauchy.
#define GN_WEIGHT_LANES 256
__global__ void __launch_bounds__(GN_WEIGHT_LANES)
k_gn_robust_weights(int N, int kind, double c, const int* __restrict__ dof, const double* __restrict__ chi2, GnMap* __restrict__ gm,
                    double* __restrict__ weight, double* __restrict__ Gsum)
{
	__shared__ double part[GN_WEIGHT_LANES / LSFM_WAVE];
	double acc = 0.0;
	for (int k = threadIdx.x; k < N; k += GN_WEIGHT_LANES)
	{
		const double n = (double)dof[k];
		double w, rho;
		gn_rho(kind, c, chi2[k] / n, w, rho);
		gm[k].w = w;
		weight[k] = w;
		acc += n * rho;
	}
	acc = block_sum_fixed<GN_WEIGHT_LANES>(acc, part);
	if (threadIdx.x == 0) *Gsum = acc;
}

// one work-group: pose_chi2[k] = chi2_k - sum_f c_kf and G = sum_k (pose_chi2[k] + 3 sum_f rho(c_kf / 3)) in a fixed order
__global__ void __launch_bounds__(GN_WEIGHT_LANES)
k_gn_feature_objective(int N, const double* __restrict__ msum, double* __restrict__ pose_chi2, double* __restrict__ Gsum)
{
	__shared__ double part[GN_WEIGHT_LANES / LSFM_WAVE];
	double acc = 0.0;
	for (int k = threadIdx.x; k < N; k += GN_WEIGHT_LANES)
	{
		const double p = msum[(size_t)3 * k] - msum[(size_t)3 * k + 1];
		pose_chi2[k] = p;
		acc += p + 3.0 * msum[(size_t)3 * k + 2];
	}
	acc = block_sum_fixed<GN_WEIGHT_LANES>(acc, part);
	if (threadIdx.x == 0) *Gsum = acc;
}

// one work-group, the weights given (k_gn_chi2<true, true>): pose_chi2[k] = chi2_k - sum_f c_kf and
// G = sum_k w_k (pose_chi2[k] + sum_f w_kf c_kf) in a fixed order, w_k the maps' weights of gn_upload
__global__ void __launch_bounds__(GN_WEIGHT_LANES)
k_gn_given_objective(int N, const GnMap* __restrict__ gm, const double* __restrict__ msum, double* __restrict__ pose_chi2, double* __restrict__ Gsum)
{
	__shared__ double part[GN_WEIGHT_LANES / LSFM_WAVE];
	double acc = 0.0;
	for (int k = threadIdx.x; k < N; k += GN_WEIGHT_LANES)
	{
		const double p = msum[(size_t)3 * k] - msum[(size_t)3 * k + 1];
		pose_chi2[k] = p;
		acc += gm[k].w * (p + msum[(size_t)3 * k + 2]);
	}
	acc = block_sum_fixed<GN_WEIGHT_LANES>(acc, part);
	if (threadIdx.x == 0) *Gsum = acc;
}

// the maps' own U blocks into the extended list (every map's blocks followed by its correction slots): block i moves by its map's shift
__global__ void __launch_bounds__(256)
k_gn_extend_u(int NU, const int* __restrict__ Ui, const int* __restrict__ pose_map, const int* __restrict__ ushift, const double* __restrict__ U,
              double* __restrict__ Ux)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= NU) return;
	double Ub[36];
	ld<36>(Ub, U + (size_t)i * 36);
	st<36>(Ux + (size_t)(i + ushift[pose_map[Ui[i]]]) * 36, Ub);
}

// Y = L^-1 Wbar^T of entry e: Wbar = the sum of its W blocks eidx[eptr[e] .. eptr[e + 1])
__device__ __forceinline__ void gn_entry_y(int e0, const int* __restrict__ eptr, const int* __restrict__ eidx, const double* __restrict__ W, const double* L, double* Y)
{
	double Wa[18], Wv[18];
	zero<18>(Wa);
	for (int e = eptr[e0]; e < eptr[e0 + 1]; e++)
	{
		ld<18>(Wv, W + (size_t)eidx[e] * 18);
#pragma unroll
		for (int i = 0; i < 18; i++) Wa[i] += Wv[i];
	}
#pragma unroll
	for (int i = 0; i < 6; i++)
	{
		double y[3];
		gn_lsolve3(L, Wa + 3 * i, y);
		Y[i] = y[0]; Y[6 + i] = y[1]; Y[12 + i] = y[2];
	}
}

// The correction of U: slot (a, b), a <= b, of map k holds  - sum_f (1 - w_f) Wbar_af V_f^-1 Wbar_bf^T  over the features f of k that both
// poses see, Wbar_af = the sum of f's W blocks of pose a (a (pose, feature) pair may repeat in a map, and summing per pose first makes
// a diagonal slot full and symmetric).  One wave per slot: its lanes stride the slot's contributors (feature cf, entries ca / cb) in
// their order, every lane sums in registers, one butterfly per entry of the block, lane 0 stores -- no atomics, the same weights give
// the same bits.  With V = L L^T the product is Y_a^T Y_b (gn_entry_y).  A contributor of weight 1 adds exactly 0 and is skipped.  Every
// slot is written by every launch.
#define GN_UFILL_LANES 256
__global__ void __launch_bounds__(GN_UFILL_LANES)
k_gn_feature_ufill(int NS, const int* __restrict__ sptr, const int* __restrict__ cf, const int* __restrict__ ca, const int* __restrict__ cb,
                   const int* __restrict__ eptr, const int* __restrict__ eidx, const int* __restrict__ sdst, const double* __restrict__ W,
                   const double* __restrict__ V, const double* __restrict__ fw, double* __restrict__ Ux)
{
	const int s = blockIdx.x * (GN_UFILL_LANES / LSFM_WAVE) + (int)threadIdx.x / LSFM_WAVE, lane = threadIdx.x & (LSFM_WAVE - 1);
	if (s >= NS) return; // (the whole wave)
	double acc[36];
	zero<36>(acc);
	for (int q = sptr[s] + lane; q < sptr[s + 1]; q += LSFM_WAVE)
	{
		const int f = cf[q];
		const double w = fw[f];
		if (w == 1.0) continue;
		double Vb[9], L[6], Ya[18], Yb[18];
		ld<9>(Vb, V + (size_t)f * 9);
		gn_chol3(Vb, L); // (k_gn_chi2<true> has reported a V that is not positive definite)
		const int ea = ca[q], eb = cb[q];
		gn_entry_y(ea, eptr, eidx, W, L, Ya);
		if (eb == ea)
		{
#pragma unroll
			for (int i = 0; i < 18; i++) Yb[i] = Ya[i];
		}
		else gn_entry_y(eb, eptr, eidx, W, L, Yb);
		const double m = 1.0 - w;
#pragma unroll
		for (int i = 0; i < 6; i++)
#pragma unroll
			for (int j = 0; j < 6; j++)
				acc[6 * i + j] -= m * (Ya[i] * Yb[j] + Ya[6 + i] * Yb[6 + j] + Ya[12 + i] * Yb[12 + j]);
	}
#pragma unroll
	for (int i = 0; i < 36; i++) acc[i] = wave_sum(acc[i]);
	if (lane == 0) st<36>(Ux + (size_t)sdst[s] * 36, acc);
}

template <bool FEAT, bool GIVEN = false>
static void gn_launch_chi2(lsfm_context* ctx, const GnCall& c, int kind, double cth, double* out)
{
	hipLaunchKernelGGL((k_gn_chi2<FEAT, GIVEN>), dim3(c.N), dim3(GN_CHI2_LANES), 0, ctx->stream, kind, cth, c.d_gm, c.u.U, c.u.Ui, c.u.Uj, c.rp, c.d_gf,
	                   c.d_x + (size_t)c.M * 6, c.X.feat, c.X.fptr, c.X.photo, c.X.W, c.X.V, out, c.feat.fchi2, c.feat.fw, c.feat.d_bad);
}
void gn_map_chi2(lsfm_context* ctx, const GnCall& c) { gn_launch_chi2<false>(ctx, c, 0, 1.0, c.d_chi2); }
void gn_map_weights(lsfm_context* ctx, const GnCall& c, int kind, double cth)
{
	hipLaunchKernelGGL(k_gn_robust_weights, dim3(1), dim3(GN_WEIGHT_LANES), 0, ctx->stream, c.N, kind, cth, c.d_dof, c.d_chi2, c.d_gm, c.d_w, c.d_G);
}
void gn_feature_chi2(lsfm_context* ctx, const GnCall& c, int kind, double cth)
{
	gn_launch_chi2<true>(ctx, c, kind, cth, c.feat.msum);
	hipLaunchKernelGGL(k_gn_feature_objective, dim3(1), dim3(GN_WEIGHT_LANES), 0, ctx->stream, c.N, c.feat.msum, c.feat.pose_chi2, c.d_G);
}
void gn_feature_chi2_given(lsfm_context* ctx, const GnCall& c)
{
	gn_launch_chi2<true, true>(ctx, c, 0, 1.0, c.feat.msum);
	hipLaunchKernelGGL(k_gn_given_objective, dim3(1), dim3(GN_WEIGHT_LANES), 0, ctx->stream, c.N, c.d_gm, c.feat.msum, c.feat.pose_chi2, c.d_G);
}
void gn_extend_u(lsfm_context* ctx, const GnCall& c, const int* d_ushift)
{
	const DevBatch& X = c.X;
	if (X.NU) hipLaunchKernelGGL(k_gn_extend_u, gn_grid(X.NU, 256), dim3(256), 0, ctx->stream, X.NU, X.Ui, X.pose_map, d_ushift, X.U, c.feat.Ux);
}
void gn_feature_ufill(lsfm_context* ctx, const GnCall& c)
{
	const GnFeat& fr = c.feat;
	if (fr.NS)
		hipLaunchKernelGGL(k_gn_feature_ufill, gn_grid(fr.NS, GN_UFILL_LANES / LSFM_WAVE), dim3(GN_UFILL_LANES), 0, ctx->stream, fr.NS, fr.d_sptr, fr.d_cf, fr.d_ca,
		                   fr.d_cb, fr.d_eptr, fr.d_eidx, fr.d_sdst, c.X.W, c.X.V, fr.fw, fr.Ux);
}

} // namespace lsfm
