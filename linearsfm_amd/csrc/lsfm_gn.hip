// Gauss-Newton polish of the map-joining objective (named in BASELINE.json's north_star).
//
// NO COUNTERPART IN THE REFERENCE -- parity unpinned: the reference joins once, hierarchically, and has no iterative step.
// What is minimised is the objective its joins linearise, over the GLOBAL state x and all N local maps at once,
//
//     F(x) = sum_k || x^_k - f_k(x) ||^2_{I_k}
//
// with f_k the reference's own change of frame (lmj_Transform_PF3DStereo Imp.cpp:421-455, Mono 3268-3306: origin at the map's
// reference pose, Mono: unit = component Fix_k of its scale pose) and its Jacobian as the reference forms it (J1 / J2 / J3,
// Imp.cpp:485-683 / 3383-3688: J = blkdiag(D) + sum_s C_s e_{h_s}^T, "old state with respect to new state at the new state" -- here
// old = frame k, new = the global frame, h_s = the global poses Ref_k [, ScaP_k]).  One step (the tests hold every step against the CPU checker's statement of it):
//
//     H = sum_k J_k^T I_k J_k,   b = sum_k J_k^T I_k r_k,   r_k = x^_k - f_k(x) (angles wrapped),   H d = b,   x += a d
//
// a = 1, halved while F does not fall.  H is laid out as ONE joint map in the library's own layout (U / W sorted by feature / V) whose
// structure -- which local block lands where -- is worked out once per call on the host from the labels; every step then is
//   k_gn_hubs      one lane per map        : R, dR, t, scale of the map's frame at the current state
//   k_gn_poses     one lane per local pose : r_a, D_a, C_s,a
//   k_gn_ublocks   one lane per local U    : U' = D_a^T U D_b into its place, U [C_s r] into the pose rows of G = I [C_s r]
//   k_gn_features  one lane per local feature (consecutive lanes, consecutive features; Stereo: consecutive W blocks): r_f, D_f, C_s,f,
//                  its run of W: W' = D_a^T W D_f and the hub blocks G_s,f^T D_f into their places in the joint W, V' and the
//                  right-hand side per instance, the pose rows of G and the hub-hub sums by wave-level segmented sums + one atomic per
//                  (wave, key, number)
//   k_gn_pose_post / k_gn_hubhub / k_gn_gather_*   the (a, h_s) and (h_s, h_t) blocks, V and the right-hand sides summed per global
//                  variable over its instances in a fixed order
// and the system goes through the same solve_batch as a tree level (pattern of S, K9 panels, supernodal factorisation, refinement,
// back-substitution).  HBM-bound: a step streams the local maps' W once (144 B in + 144 B out per block, + 144 B per hub block) and
// the joint map through the solver.
#include <algorithm>
#include <chrono>

#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"

namespace lsfm {

struct GnMap {
	// structure (uploaded once)
	int nh;        // hub columns: 0 = the map's frame is the global frame (Stereo, Ref_k == the global Ref), 1 Stereo, 2 Mono
	int hub[2];    // global pose of Ref_k [, ScaP_k]
	int fix;       // Mono: Fix_k
	int p0, m, f0, n, u0, nu; // its poses / features / U blocks in the uploaded batch
	int ubase;     // its first block in the joint U: nh * m blocks (a, h_s), nh (nh + 1) / 2 blocks (h_s, h_t), nu own blocks
	double w;      // weight of the map's information matrix in the step (1 unless the robust polish re-weights it: k_gn_robust_weights)
	// the frame at the current state (k_gn_hubs)
	double R[9], dRA[9], dRB[9], dRG[9], t[3];
	double Scale, Scale2, dSdt[3], dSdtt[3], dSdA, dSdB, dSdG; // (row Fix_k of the reference's dSdt / dSdtt, component Fix_k of dSdA..)
};

__global__ void k_gn_hubs(int N, GnMap* gm, const double* __restrict__ xp)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= N) return;
	GnMap& t = gm[k];
	double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, dRA[9], dRB[9], dRG[9];
	zero<9>(dRA); zero<9>(dRB); zero<9>(dRG);
	t.t[0] = t.t[1] = t.t[2] = 0.0;
	t.Scale = t.Scale2 = 1.0;
	t.dSdA = t.dSdB = t.dSdG = 0.0;
	for (int i = 0; i < 3; i++) { t.dSdt[i] = 0.0; t.dSdtt[i] = 0.0; }
	if (t.nh > 0)
	{
		const double* p = xp + (size_t)t.hub[0] * 6;
		t.t[0] = p[0]; t.t[1] = p[1]; t.t[2] = p[2];
		r_derivation(p[3], p[4], p[5], R, dRA, dRB, dRG);
		if (t.nh == 2)
		{
			// Imp.cpp:3311-3365
			const double* q = xp + (size_t)t.hub[1] * 6;
			double d[3] = { q[0] - p[0], q[1] - p[1], q[2] - p[2] }, ts[3], v[3];
			mv3(R, d, ts);
			const double Sign = ts[t.fix] >= 0 ? 1.0 : -1.0;
			t.Scale = fabs(ts[t.fix]); t.Scale2 = t.Scale * t.Scale;
			for (int c = 0; c < 3; c++) { t.dSdt[c] = -R[3 * t.fix + c] * Sign; t.dSdtt[c] = R[3 * t.fix + c] * Sign; }
			mv3(dRA, d, v); t.dSdA = v[t.fix] * Sign;
			mv3(dRB, d, v); t.dSdB = v[t.fix] * Sign;
			mv3(dRG, d, v); t.dSdG = v[t.fix] * Sign;
		}
	}
	for (int i = 0; i < 9; i++) { t.R[i] = R[i]; t.dRA[i] = dRA[i]; t.dRB[i] = dRB[i]; t.dRG[i] = dRG[i]; }
}

// a position xn of the global state in the map's frame, and the Jacobian of that with respect to xn (a22), the hub's translation and
// angles (adt | tmpc: columns alpha, beta, gamma) and the scale pose's translation (adtt): Imp.cpp:3420-3469 / 3591-3640; Stereo is the
// case Scale = 1, dS = 0 (Imp.cpp:638-680)
__device__ __forceinline__ void gn_trans(const GnMap& t, const double* xn, double* f, double* a22, double* adt, double* tmpc, double* adtt)
{
	double t222[3] = { xn[0] - t.t[0], xn[1] - t.t[1], xn[2] - t.t[2] }, t22[3], v[3];
	mv3(t.R, t222, t22);
#pragma unroll
	for (int r = 0; r < 3; r++) f[r] = t22[r] / t.Scale;
	mv3(t.dRA, t222, v);
#pragma unroll
	for (int r = 0; r < 3; r++) tmpc[3 * r + 0] = (v[r] * t.Scale - t22[r] * t.dSdA) / t.Scale2;
	mv3(t.dRB, t222, v);
#pragma unroll
	for (int r = 0; r < 3; r++) tmpc[3 * r + 1] = (v[r] * t.Scale - t22[r] * t.dSdB) / t.Scale2;
	mv3(t.dRG, t222, v);
#pragma unroll
	for (int r = 0; r < 3; r++) tmpc[3 * r + 2] = (v[r] * t.Scale - t22[r] * t.dSdG) / t.Scale2;
#pragma unroll
	for (int r = 0; r < 3; r++)
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			a22[3 * r + c] = t.R[3 * r + c] / t.Scale;
			adt[3 * r + c] = (-t.R[3 * r + c] * t.Scale - t22[r] * t.dSdt[c]) / t.Scale2;
			adtt[3 * r + c] = (-t22[r] * t.dSdtt[c]) / t.Scale2;
		}
}

__device__ __forceinline__ double gn_wrap(double a)
{
	const double pi = 3.14159265358979323846;
	while (a > pi) a -= 2 * pi;
	while (a < -pi) a += 2 * pi;
	return a;
}

// per local pose: residual, D (6x6), C_1, C_2 (6x6): Imp.cpp:485-635 / 3383-3584; a local pose that IS a hub collects the hub's
// column in its own (Imp.cpp:3495-3581)
__global__ void __launch_bounds__(128)
k_gn_poses(int P, const int* __restrict__ pose_map, const GnMap* __restrict__ gm, const int* __restrict__ gp, const double* __restrict__ xp,
           const double* __restrict__ xhat, double* __restrict__ Dp, double* __restrict__ Cp, double* __restrict__ rp)
{
	const int a = blockIdx.x * blockDim.x + threadIdx.x;
	if (a >= P) return;
	const GnMap& t = gm[pose_map[a]];
	const double* xn = xp + (size_t)gp[a] * 6;
	const double* xh = xhat + (size_t)a * 6;
	double f[3], a22[9], adt[9], tmpc[9], adtt[9], D[36], C1[36], C2[36];
	gn_trans(t, xn, f, a22, adt, tmpc, adtt);
	double R2[9], dRA2[9], dRB2[9], dRG2[9], Ri[9], dRi[9], dd2[3][3], dd[3][3], al, be, ga;
	r_derivation(xn[3], xn[4], xn[5], R2, dRA2, dRB2, dRG2);
	times_rrt(Ri, R2, t.R);
	inv_rmat_ypr(Ri, al, be, ga);
	double* r = rp + (size_t)a * 6;
	r[0] = xh[0] - f[0]; r[1] = xh[1] - f[1]; r[2] = xh[2] - f[2];
	r[3] = gn_wrap(xh[3] - al); r[4] = gn_wrap(xh[4] - be); r[5] = gn_wrap(xh[5] - ga);
	times_rrt(dRi, dRA2, t.R); ypr_rates<false>(dd2[0], dRi, Ri);
	times_rrt(dRi, dRB2, t.R); ypr_rates<false>(dd2[1], dRi, Ri);
	times_rrt(dRi, dRG2, t.R); ypr_rates<false>(dd2[2], dRi, Ri);
	times_rrt(dRi, R2, t.dRA); ypr_rates<false>(dd[0], dRi, Ri);
	times_rrt(dRi, R2, t.dRB); ypr_rates<false>(dd[1], dRi, Ri);
	times_rrt(dRi, R2, t.dRG); ypr_rates<false>(dd[2], dRi, Ri);
	zero<36>(D); zero<36>(C1); zero<36>(C2);
	const bool hubs = t.nh > 0;
#pragma unroll
	for (int rr = 0; rr < 3; rr++)
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			D[6 * rr + c] = a22[3 * rr + c];
			D[6 * (3 + rr) + 3 + c] = dd2[c][rr];
			C1[6 * rr + c] = hubs ? adt[3 * rr + c] : 0.0;
			C1[6 * rr + 3 + c] = hubs ? tmpc[3 * rr + c] : 0.0;
			C1[6 * (3 + rr) + 3 + c] = hubs ? dd[c][rr] : 0.0;
			C2[6 * rr + c] = t.nh == 2 ? adtt[3 * rr + c] : 0.0;
		}
	const bool h0 = hubs && gp[a] == t.hub[0], h1 = t.nh == 2 && gp[a] == t.hub[1];
#pragma unroll
	for (int q = 0; q < 36; q++)
	{
		D[q] += (h0 ? C1[q] : 0.0) + (h1 ? C2[q] : 0.0);
		C1[q] = h0 ? 0.0 : C1[q];
		C2[q] = h1 ? 0.0 : C2[q];
	}
	st<36>(Dp + (size_t)a * 36, D);
	st<36>(Cp + (size_t)a * 36, C1);
	st<36>(Cp + (size_t)P * 36 + (size_t)a * 36, C2);
}

// v[0..N) of the lanes that share `key` summed over the wave, one atomic per (key, number) into base[key * stride + i].  All 64 lanes.
template <int N>
__device__ __forceinline__ void wave_key_add(int key, bool valid, const double* v, double* base, int stride)
{
	unsigned long long todo = __ballot(valid);
	const int lane = threadIdx.x & (LSFM_WAVE - 1);
	while (todo)
	{
		const int leader = __ffsll((long long)todo) - 1;
		const int k = __shfl(key, leader, LSFM_WAVE);
		const bool mine = valid && key == k;
#pragma unroll
		for (int i = 0; i < N; i++)
		{
			const double s = wave_sum(mine ? v[i] : 0.0);
			if (lane == leader) atomic_add_f64(base + (size_t)k * stride + i, s);
		}
		todo &= ~__ballot(mine);
	}
}

#define GN_GW 78 /* pose row of G = I [C_1 C_2 r]: 36 + 36 + 6 */
#define GN_HW 121 /* per map: C_1^T G_1, C_1^T G_2, C_2^T G_2 (36 each), C_1^T g, C_2^T g (6 each), r^T g */

// one lane per local U block (a, b): its part of the pose rows of G, and U' = D_a^T U D_b at its place in the joint U
__global__ void __launch_bounds__(128)
k_gn_ublocks(int NU, int P, const int* __restrict__ Ui, const int* __restrict__ Uj, const double* __restrict__ U, const int* __restrict__ pose_map,
             const GnMap* __restrict__ gm, const int* __restrict__ gp, const double* __restrict__ Dp, const double* __restrict__ Cp,
             const double* __restrict__ rp, double* __restrict__ Gacc, double* __restrict__ UJ)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= NU) return;
	const int a = Ui[i], b = Uj[i];
	const GnMap& t = gm[pose_map[a]];
	double Ub[36], X[36], Y[36];
	ld<36>(Ub, U + (size_t)i * 36);
#pragma unroll
	for (int q = 0; q < 36; q++) Ub[q] *= t.w;
	for (int s = 0; s < 2; s++)
	{
		ld<36>(X, Cp + (size_t)s * P * 36 + (size_t)b * 36);
		mm<6, 6, 6, false>(Ub, X, Y);
		for (int q = 0; q < 36; q++) if (Y[q] != 0.0) atomic_add_f64(Gacc + (size_t)a * GN_GW + 36 * s + q, Y[q]);
		if (a != b)
		{
			ld<36>(X, Cp + (size_t)s * P * 36 + (size_t)a * 36);
			mtm<6, 6, 6, false>(Ub, X, Y);
			for (int q = 0; q < 36; q++) if (Y[q] != 0.0) atomic_add_f64(Gacc + (size_t)b * GN_GW + 36 * s + q, Y[q]);
		}
	}
	{
		double ra[6], rb[6], y[6];
		ld<6>(rb, rp + (size_t)b * 6);
		mm<6, 6, 1, false>(Ub, rb, y);
		for (int q = 0; q < 6; q++) atomic_add_f64(Gacc + (size_t)a * GN_GW + 72 + q, y[q]);
		if (a != b)
		{
			ld<6>(ra, rp + (size_t)a * 6);
			mtm<6, 6, 1, false>(Ub, ra, y);
			for (int q = 0; q < 6; q++) atomic_add_f64(Gacc + (size_t)b * GN_GW + 72 + q, y[q]);
		}
	}
	ld<36>(X, Dp + (size_t)a * 36);
	mtm<6, 6, 6, false>(X, Ub, Y);
	ld<36>(X, Dp + (size_t)b * 36);
	mm<6, 6, 6, false>(Y, X, Ub);
	double* d = UJ + (size_t)(t.ubase + t.nh * t.m + t.nh * (t.nh + 1) / 2 + (i - t.u0)) * 36;
	if (gp[a] <= gp[b]) st<36>(d, Ub);
	else { transpose<6, 6>(Ub, X); st<36>(d, X); }
}

// one lane per local feature (see the header).  NH: 1 Stereo, 2 Mono (a Stereo map in the global frame has t.nh = 0: its C are zero
// and it owns no hub blocks).  FW (lsfm_gn_polish_robust_features only): the instance's W and V blocks are weighted
// by t.w * fw[f], the weight of the feature's conditional term (k_gn_feature_chi2); FW = false is the kernel of the plain and the map-robust polish, fw unused
template <int NH, bool FW>
__global__ void __launch_bounds__(256)
k_gn_features(int NF, int P, const int* __restrict__ feat_map, const GnMap* __restrict__ gm, const int* __restrict__ gf, const double* __restrict__ xf,
              const double* __restrict__ fhat, const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W,
              const double* __restrict__ V, const double* __restrict__ Dp, const double* __restrict__ Cp, const double* __restrict__ rp,
              const int* __restrict__ wdst, double* __restrict__ WJ, double* __restrict__ Vinst, double* __restrict__ eFinst,
              double* __restrict__ Gacc, double* __restrict__ Hacc, const double* __restrict__ fw)
{
	const int f = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = f < NF;
	const int fc = live ? f : 0;
	const int k = feat_map[fc];
	const GnMap& t = gm[k];
	const double fwv = FW ? fw[fc] : 1.0;
	const bool hubs = t.nh > 0;
	double fv[3], Df[9], adt[9], tmpc[9], adtt[9], Cf[NH][18], rf[3], Vb[9];
	gn_trans(t, xf + (size_t)gf[fc] * 3, fv, Df, adt, tmpc, adtt);
#pragma unroll
	for (int r = 0; r < 3; r++)
	{
		rf[r] = fhat[(size_t)fc * 3 + r] - fv[r];
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			Cf[0][6 * r + c] = hubs ? adt[3 * r + c] : 0.0;
			Cf[0][6 * r + 3 + c] = hubs ? tmpc[3 * r + c] : 0.0;
			if (NH == 2) { Cf[NH - 1][6 * r + c] = adtt[3 * r + c]; Cf[NH - 1][6 * r + 3 + c] = 0.0; }
		}
	}
	ld<9>(Vb, V + (size_t)fc * 9);
#pragma unroll
	for (int q = 0; q < 9; q++) Vb[q] *= FW ? t.w * fwv : t.w;
	double gfv[3], Gf[NH][18];
	mm<3, 3, 1, false>(Vb, rf, gfv);
#pragma unroll
	for (int s = 0; s < NH; s++) mm<3, 3, 6, false>(Vb, Cf[s], Gf[s]);
	const int j0 = fptr[fc], len = live ? fptr[fc + 1] - j0 : 0;
	int maxlen = len;
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, off, LSFM_WAVE));
	const int dst0 = wdst[fc] + t.nh;
	for (int jj = 0; jj < maxlen; jj++)
	{
		const bool on = jj < len;
		const int j = on ? j0 + jj : j0;
		const int a = photo[j];
		double Wb[18], pc[GN_GW];
		ld<18>(Wb, W + (size_t)j * 18);
#pragma unroll
		for (int q = 0; q < 18; q++) Wb[q] *= FW ? t.w * fwv : t.w;
		{
			double ra[6], T[18], Da[36];
			ld<6>(ra, rp + (size_t)a * 6);
			if (on) mtm<6, 3, 1, true>(Wb, ra, gfv);
#pragma unroll
			for (int s = 0; s < NH; s++)
			{
				ld<36>(Da, Cp + (size_t)s * P * 36 + (size_t)a * 36);
				if (on) mtm<6, 3, 6, true>(Wb, Da, Gf[s]);
			}
			ld<36>(Da, Dp + (size_t)a * 36);
			mtm<6, 6, 3, false>(Da, Wb, T);
			double Wn[18];
			mm<6, 3, 3, false>(T, Df, Wn);
			if (on) st<18>(WJ + (size_t)(dst0 + jj) * 18, Wn);
		}
		// this block's share of its pose's row of G
		mm<6, 3, 6, false>(Wb, Cf[0], pc);
		if (NH == 2) mm<6, 3, 6, false>(Wb, Cf[NH - 1], pc + 36);
		else zero<36>(pc + 36);
		mm<6, 3, 1, false>(Wb, rf, pc + 72);
		if (NH == 2) wave_key_add<GN_GW>(a, on, pc, Gacc, GN_GW);
		else
		{
			// (Stereo: the second hub column does not exist)
			wave_key_add<36>(a, on, pc, Gacc, GN_GW);
			wave_key_add<6>(a, on, pc + 72, Gacc + 72, GN_GW);
		}
	}
	if (live)
	{
		// the feature's hub blocks G_s,f^T D_f, its V' and right-hand side
#pragma unroll
		for (int s = 0; s < NH; s++)
			if (s < t.nh)
			{
				double Y[18];
				mtm<3, 6, 3, false>(Gf[s], Df, Y);
				st<18>(WJ + (size_t)(wdst[f] + s) * 18, Y);
			}
		double T[9], Vn[9], e[3];
		mtm<3, 3, 3, false>(Df, Vb, T);
		mm<3, 3, 3, false>(T, Df, Vn);
		st<9>(Vinst + (size_t)f * 9, Vn);
		mtm<3, 3, 1, false>(Df, gfv, e);
		st<3>(eFinst + (size_t)f * 3, e);
	}
	// the map's hub-hub sums
	{
		double h[GN_HW];
		mtm<3, 6, 6, false>(Cf[0], Gf[0], h);
		if (NH == 2) { mtm<3, 6, 6, false>(Cf[0], Gf[NH - 1], h + 36); mtm<3, 6, 6, false>(Cf[NH - 1], Gf[NH - 1], h + 72); }
		mtm<3, 6, 1, false>(Cf[0], gfv, h + 108);
		if (NH == 2) mtm<3, 6, 1, false>(Cf[NH - 1], gfv, h + 114);
		h[120] = rf[0] * gfv[0] + rf[1] * gfv[1] + rf[2] * gfv[2];
		if (NH == 2) wave_key_add<GN_HW>(k, live, h, Hacc, GN_HW);
		else
		{
			wave_key_add<36>(k, live, h, Hacc, GN_HW);
			wave_key_add<6>(k, live, h + 108, Hacc + 108, GN_HW);
			wave_key_add<1>(k, live, h + 120, Hacc + 120, GN_HW);
		}
	}
}

// one lane per local pose, after the rows of G are complete: the (a, h_s) blocks D_a^T G_s,a, the pose's right-hand side, its share of
// the hub-hub sums
__global__ void __launch_bounds__(128)
k_gn_pose_post(int P, const int* __restrict__ pose_map, const GnMap* __restrict__ gm, const int* __restrict__ gp, const double* __restrict__ Dp,
               const double* __restrict__ Cp, const double* __restrict__ rp, const double* __restrict__ Gacc, double* __restrict__ UJ,
               double* __restrict__ ePinst, double* __restrict__ Hacc)
{
	const int a = blockIdx.x * blockDim.x + threadIdx.x;
	if (a >= P) return;
	const int k = pose_map[a];
	const GnMap& t = gm[k];
	double D[36], G[2][36], g[6], X[36], e[6];
	ld<36>(D, Dp + (size_t)a * 36);
	ld<36>(G[0], Gacc + (size_t)a * GN_GW); ld<36>(G[1], Gacc + (size_t)a * GN_GW + 36); ld<6>(g, Gacc + (size_t)a * GN_GW + 72);
	for (int s = 0; s < t.nh; s++)
	{
		mtm<6, 6, 6, false>(D, G[s], X);
		double* d = UJ + (size_t)(t.ubase + s * t.m + (a - t.p0)) * 36;
		const int ga = gp[a], h = t.hub[s];
		for (int r = 0; r < 6; r++)
			for (int c = 0; c < 6; c++)
				d[6 * r + c] = ga == h ? X[6 * r + c] + X[6 * c + r] : (ga < h ? X[6 * r + c] : X[6 * c + r]); // a diagonal block in full; row <= column
	}
	mtm<6, 6, 1, false>(D, g, e);
	st<6>(ePinst + (size_t)a * 6, e);
	double* H = Hacc + (size_t)k * GN_HW;
	double C[2][36];
	ld<36>(C[0], Cp + (size_t)a * 36); ld<36>(C[1], Cp + (size_t)P * 36 + (size_t)a * 36);
	if (t.nh > 0)
	{
		mtm<6, 6, 6, false>(C[0], G[0], X);
		for (int q = 0; q < 36; q++) if (X[q] != 0.0) atomic_add_f64(H + q, X[q]);
		mtm<6, 6, 1, false>(C[0], g, e);
		for (int q = 0; q < 6; q++) atomic_add_f64(H + 108 + q, e[q]);
	}
	if (t.nh == 2)
	{
		mtm<6, 6, 6, false>(C[0], G[1], X);
		for (int q = 0; q < 36; q++) if (X[q] != 0.0) atomic_add_f64(H + 36 + q, X[q]);
		mtm<6, 6, 6, false>(C[1], G[1], X);
		for (int q = 0; q < 36; q++) if (X[q] != 0.0) atomic_add_f64(H + 72 + q, X[q]);
		mtm<6, 6, 1, false>(C[1], g, e);
		for (int q = 0; q < 6; q++) atomic_add_f64(H + 114 + q, e[q]);
	}
	double rr[6], dot = 0.0;
	ld<6>(rr, rp + (size_t)a * 6);
	for (int q = 0; q < 6; q++) dot += rr[q] * g[q];
	atomic_add_f64(H + 120, dot);
}

// one lane per map: the hub-hub blocks into the joint U, the map's part of F
__global__ void k_gn_hubhub(int N, const GnMap* __restrict__ gm, const double* __restrict__ Hacc, double* __restrict__ UJ, double* __restrict__ Fsum)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= N) return;
	const GnMap& t = gm[k];
	const double* H = Hacc + (size_t)k * GN_HW;
	atomic_add_f64(Fsum, H[120]);
	if (t.nh == 0) return;
	double* d = UJ + (size_t)(t.ubase + t.nh * t.m) * 36;
	for (int q = 0; q < 36; q++) d[q] = H[q]; // (h_1, h_1)
	if (t.nh == 2)
	{
		const bool up = t.hub[0] < t.hub[1];
		for (int r = 0; r < 6; r++)
			for (int c = 0; c < 6; c++) d[36 + 6 * r + c] = up ? H[36 + 6 * r + c] : H[36 + 6 * c + r]; // (h_1, h_2), row <= column
		for (int q = 0; q < 36; q++) d[72 + q] = H[72 + q]; // (h_2, h_2)
	}
}

// V and the features' right-hand side: every global feature sums its instances in their order
__global__ void k_gn_gather_feat(int NFG, const int* __restrict__ sptr, const int* __restrict__ sidx, const double* __restrict__ Vinst,
                                 const double* __restrict__ eFinst, double* __restrict__ VJ, double* __restrict__ eb)
{
	const int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= NFG) return;
	double v[9], e[3];
	zero<9>(v); zero<3>(e);
	for (int q = sptr[g]; q < sptr[g + 1]; q++)
	{
		const int f = sidx[q];
		for (int i = 0; i < 9; i++) v[i] += Vinst[(size_t)f * 9 + i];
		for (int i = 0; i < 3; i++) e[i] += eFinst[(size_t)f * 3 + i];
	}
	st<9>(VJ + (size_t)g * 9, v);
	st<3>(eb + (size_t)g * 3, e);
}
// the poses' right-hand side: instances (>= 0) and hub roles (-1 - (2 map + s))
__global__ void k_gn_gather_pose(int M, const int* __restrict__ sptr, const int* __restrict__ sidx, const double* __restrict__ ePinst,
                                 const double* __restrict__ Hacc, double* __restrict__ ea)
{
	const int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= M) return;
	double e[6];
	zero<6>(e);
	for (int q = sptr[g]; q < sptr[g + 1]; q++)
	{
		const int sdx = sidx[q];
		const double* src = sdx >= 0 ? ePinst + (size_t)sdx * 6 : Hacc + (size_t)((-1 - sdx) >> 1) * GN_HW + 108 + 6 * ((-1 - sdx) & 1);
		for (int i = 0; i < 6; i++) e[i] += src[i];
	}
	st<6>(ea + (size_t)g * 6, e);
}

// ---- the joint system as a map like any other (lsfm_gn_linearise) ----
// UJ / WJ hold the solver's working form: entries with equal coordinates are repeated and add up.  Output block o is the sum of its
// sources sidx[sptr[o] .. sptr[o + 1]) in that order (map order: the structure pass sorts stably).  One lane per output block,
// consecutive lanes on consecutive output blocks; the sources of neighbouring output blocks lie in the same feature's run of WJ.  The
// sum is held in registers and stored once.  No atomics: given UJ / WJ the result is the same bits every time.  HBM-bound: NWJ * 144 B
// in, nW' * 144 B out (U: 288 B a block), no products.
template <int N>
__device__ __forceinline__ void gn_coalesce_block(int o, const int* __restrict__ sptr, const int* __restrict__ sidx, const double* __restrict__ src, double* __restrict__ dst)
{
	double acc[N], v[N];
	const int q0 = sptr[o], q1 = sptr[o + 1];
	ld<N>(acc, src + (size_t)sidx[q0] * N);
	for (int q = q0 + 1; q < q1; q++)
	{
		ld<N>(v, src + (size_t)sidx[q] * N);
#pragma unroll
		for (int i = 0; i < N; i++) acc[i] += v[i];
	}
	st<N>(dst + (size_t)o * N, acc);
}
__global__ void __launch_bounds__(256)
k_gn_coalesce_w(int nWo, const int* __restrict__ sptr, const int* __restrict__ sidx, const double* __restrict__ WJ, double* __restrict__ Wo)
{
	const int o = blockIdx.x * blockDim.x + threadIdx.x;
	if (o < nWo) gn_coalesce_block<18>(o, sptr, sidx, WJ, Wo);
}
__global__ void __launch_bounds__(256)
k_gn_coalesce_u(int nUo, const int* __restrict__ sptr, const int* __restrict__ sidx, const double* __restrict__ UJ, double* __restrict__ Uo)
{
	const int o = blockIdx.x * blockDim.x + threadIdx.x;
	if (o < nUo) gn_coalesce_block<36>(o, sptr, sidx, UJ, Uo);
}

// ---- per-map chi^2 and the robust weights (lsfm_map_chi2, lsfm_gn_polish_robust) ----
// chi2_k = r_k^T I_k r_k = sum_U (2 - delta_ab) r_a^T U_ab r_b + 2 sum_W r_a^T W_af r_f + sum_f r_f^T V_f r_f over map k's own blocks, at
// the frames of k_gn_hubs and the pose residuals of k_gn_poses.  One work-group per map: its lanes stride over the map's U blocks and its
// features (each with its run of W), every lane sums in a fixed order, then the wave sums and a fixed-order sum over the waves in LDS --
// no atomics, so the same state gives the same bits.  256 lanes: a map of the NC3500-like set holds 520-763 W blocks (one per feature),
// one of the RS468-like set 1200-1882 over 600-941 features -- two to four features per lane.  The feature residual is recomputed here
// (f = R (x_f - t) / Scale, as gn_trans forms it): k_gn_features, which forms it too, runs after the weights that need chi2 are set.
#define GN_CHI2_LANES 256
__global__ void __launch_bounds__(GN_CHI2_LANES)
k_gn_map_chi2(const GnMap* __restrict__ gm, const double* __restrict__ U, const int* __restrict__ Ui, const int* __restrict__ Uj,
              const double* __restrict__ rp, const int* __restrict__ gf, const double* __restrict__ xf, const double* __restrict__ fhat,
              const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W, const double* __restrict__ V,
              double* __restrict__ chi2)
{
	__shared__ double part[GN_CHI2_LANES / LSFM_WAVE];
	const int k = blockIdx.x;
	const GnMap& t = gm[k];
	double acc = 0.0;
	for (int i = t.u0 + (int)threadIdx.x; i < t.u0 + t.nu; i += GN_CHI2_LANES)
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
		acc += a == b ? d : 2.0 * d;
	}
	for (int f = t.f0 + (int)threadIdx.x; f < t.f0 + t.n; f += GN_CHI2_LANES)
	{
		const double* xn = xf + (size_t)gf[f] * 3;
		double t222[3] = { xn[0] - t.t[0], xn[1] - t.t[1], xn[2] - t.t[2] }, t22[3], rf[3], Vb[9], y[3];
		mv3(t.R, t222, t22);
#pragma unroll
		for (int r = 0; r < 3; r++) rf[r] = fhat[(size_t)f * 3 + r] - t22[r] / t.Scale;
		ld<9>(Vb, V + (size_t)f * 9);
		mm<3, 3, 1, false>(Vb, rf, y);
		double d = rf[0] * y[0] + rf[1] * y[1] + rf[2] * y[2];
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
		}
		acc += d;
	}
	acc = wave_sum(acc);
	if ((threadIdx.x & (LSFM_WAVE - 1)) == 0) part[threadIdx.x / LSFM_WAVE] = acc;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		double sum = 0.0;
#pragma unroll
		for (int w = 0; w < GN_CHI2_LANES / LSFM_WAVE; w++) sum += part[w];
		chi2[k] = sum;
	}
}

// one work-group: s_k = chi2_k / dof_k, w_k = rho'(s_k) into the maps' frames (the next assembly's weights) and weight[k], and
// G = sum_k dof_k rho(s_k) summed in a fixed order (lane-strided, wave sums, waves in order).  kind 1 Huber, 2 Cauchy.
#define GN_WEIGHT_LANES 256
__global__ void __launch_bounds__(GN_WEIGHT_LANES)
k_gn_robust_weights(int N, int kind, double c, const int* __restrict__ dof, const double* __restrict__ chi2, GnMap* __restrict__ gm,
                    double* __restrict__ weight, double* __restrict__ Gsum)
{
	__shared__ double part[GN_WEIGHT_LANES / LSFM_WAVE];
	const double c2 = c * c;
	double acc = 0.0;
	for (int k = threadIdx.x; k < N; k += GN_WEIGHT_LANES)
	{
		const double n = (double)dof[k], s = chi2[k] / n;
		double w, rho;
		if (kind == 1)
		{
			const bool in = s <= c2;
			w = in ? 1.0 : c / sqrt(s);
			rho = in ? s : 2.0 * c * sqrt(s) - c2;
		}
		else
		{
			w = 1.0 / (1.0 + s / c2);
			rho = c2 * log1p(s / c2);
		}
		gm[k].w = w;
		weight[k] = w;
		acc += n * rho;
	}
	acc = wave_sum(acc);
	if ((threadIdx.x & (LSFM_WAVE - 1)) == 0) part[threadIdx.x / LSFM_WAVE] = acc;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		double sum = 0.0;
#pragma unroll
		for (int w = 0; w < GN_WEIGHT_LANES / LSFM_WAVE; w++) sum += part[w];
		*Gsum = sum;
	}
}

// ---- per-feature chi^2 and the feature-robust polish (lsfm_map_feature_chi2, lsfm_gn_polish_robust_features) ----
// With g_f = V_f r_f + sum_a W_af^T r_a the map's chi^2 splits into a pose part under the map's own Schur complement and one conditional
// term per feature:  chi2_k = r_p^T (U - sum_f W_f V_f^-1 W_f^T) r_p + sum_f c_kf,  c_kf = g_f^T V_f^-1 g_f >= 0.  Scaling the conditional
// term of f by w_f is the information matrix  I_k(w) = [U - sum_f (1 - w_f) W_f V_f^-1 W_f^T, w_f W_f; w_f W_f^T, w_f V_f]  (w = 1: I_k,
// w_f = 0: f marginalised out), so IRLS on c_kf is the plain step on re-weighted maps: k_gn_features<NH, true> scales W and V, the
// correction of U goes into slots of its own behind the map's U blocks (k_gn_feature_ufill) and k_gn_ublocks places them like any other.

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

// One work-group per map, as k_gn_map_chi2 and reading what it reads (every U, W and V block of the map once): the lanes stride over the
// map's OWN U blocks (nu_own: the correction slots behind them are not part of I_k) and over its features; per feature c_kf, its weight
// w_kf = rho'(c_kf / 3) (kind 0: 1, 1 Huber, 2 Cauchy, as k_gn_robust_weights) and the feature's share of chi2_k; per map chi2_k,
// sum_f c_kf and sum_f rho(c_kf / 3) (msum[3 k ..]) by lane sums, wave sums and a fixed-order sum over the waves -- no atomics on any
// sum.  bad: the smallest feature instance whose V is not positive definite (an integer minimum: the same for every order).
#define GN_FCHI2_LANES 256
__global__ void __launch_bounds__(GN_FCHI2_LANES)
k_gn_feature_chi2(int kind, double c, const GnMap* __restrict__ gm, const int* __restrict__ nu_own, const double* __restrict__ U,
                  const int* __restrict__ Ui, const int* __restrict__ Uj, const double* __restrict__ rp, const int* __restrict__ gf,
                  const double* __restrict__ xf, const double* __restrict__ fhat, const int* __restrict__ fptr, const int* __restrict__ photo,
                  const double* __restrict__ W, const double* __restrict__ V, double* __restrict__ fchi2, double* __restrict__ fweight,
                  double* __restrict__ msum, int* __restrict__ bad)
{
	__shared__ double part[3][GN_FCHI2_LANES / LSFM_WAVE];
	const int k = blockIdx.x;
	const GnMap& t = gm[k];
	const double c2 = c * c;
	double acc = 0.0, accc = 0.0, accr = 0.0;
	for (int i = t.u0 + (int)threadIdx.x; i < t.u0 + nu_own[k]; i += GN_FCHI2_LANES)
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
		acc += a == b ? d : 2.0 * d;
	}
	for (int f = t.f0 + (int)threadIdx.x; f < t.f0 + t.n; f += GN_FCHI2_LANES)
	{
		const double* xn = xf + (size_t)gf[f] * 3;
		double t222[3] = { xn[0] - t.t[0], xn[1] - t.t[1], xn[2] - t.t[2] }, t22[3], rf[3], Vb[9], g[3], L[6], y[3];
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
			mtm<6, 3, 1, true>(Wb, ra, g);
		}
		if (!gn_chol3(Vb, L)) atomicMin(bad, f);
		gn_lsolve3(L, g, y);
		const double cf = y[0] * y[0] + y[1] * y[1] + y[2] * y[2], s = cf / 3.0;
		double w = 1.0, rho = s;
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
		fchi2[f] = cf;
		fweight[f] = w;
		acc += d; accc += cf; accr += rho;
	}
	acc = wave_sum(acc); accc = wave_sum(accc); accr = wave_sum(accr);
	if ((threadIdx.x & (LSFM_WAVE - 1)) == 0)
	{
		part[0][threadIdx.x / LSFM_WAVE] = acc; part[1][threadIdx.x / LSFM_WAVE] = accc; part[2][threadIdx.x / LSFM_WAVE] = accr;
	}
	__syncthreads();
	if (threadIdx.x < 3)
	{
		double sum = 0.0;
#pragma unroll
		for (int w = 0; w < GN_FCHI2_LANES / LSFM_WAVE; w++) sum += part[threadIdx.x][w];
		msum[(size_t)3 * k + threadIdx.x] = sum;
	}
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
	acc = wave_sum(acc);
	if ((threadIdx.x & (LSFM_WAVE - 1)) == 0) part[threadIdx.x / LSFM_WAVE] = acc;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		double sum = 0.0;
#pragma unroll
		for (int w = 0; w < GN_WEIGHT_LANES / LSFM_WAVE; w++) sum += part[w];
		*Gsum = sum;
	}
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

// The correction of U: slot (a, b), a <= b, of map k holds  - sum_f (1 - w_f) Wbar_af V_f^-1 Wbar_bf^T  over the features f of k that both
// poses see, Wbar_af = the sum of f's W blocks of pose a (entry e: blocks eidx[eptr[e] .. eptr[e + 1]); a (pose, feature) pair may repeat
// in a map, and summing per pose first makes a diagonal slot full and symmetric).  One wave per slot: its lanes stride the slot's
// contributors (feature cf, entries ca / cb) in their order, every lane sums in registers, one butterfly per entry of the block, lane 0
// stores -- no atomics, the same weights give the same bits.  With V = L L^T the product is Y_a^T Y_b, Y = L^-1 Wbar^T.  A contributor of
// weight 1 adds exactly 0 and is skipped.  Every slot is written by every launch.
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
		double Vb[9], L[6], Wa[18], Wv[18], Ya[18], Yb[18];
		ld<9>(Vb, V + (size_t)f * 9);
		gn_chol3(Vb, L); // (k_gn_feature_chi2 has reported a V that is not positive definite)
		const int ea = ca[q], eb = cb[q];
		zero<18>(Wa);
		for (int e = eptr[ea]; e < eptr[ea + 1]; e++)
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
			Ya[i] = y[0]; Ya[6 + i] = y[1]; Ya[12 + i] = y[2];
		}
		if (eb == ea)
		{
#pragma unroll
			for (int i = 0; i < 18; i++) Yb[i] = Ya[i];
		}
		else
		{
			zero<18>(Wa);
			for (int e = eptr[eb]; e < eptr[eb + 1]; e++)
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
				Yb[i] = y[0]; Yb[6 + i] = y[1]; Yb[12 + i] = y[2];
			}
		}
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

// largest |v| over the scalars that are not fixed, as the bits of a non-negative double (they order like the numbers)
__global__ void k_gn_maxabs(size_t n, const double* __restrict__ v, const unsigned char* __restrict__ fixed, unsigned long long* out)
{
	double m = 0.0;
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
		if (!(fixed && fixed[i])) { const double a = fabs(v[i]); m = a > m || a != a ? a : m; }
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(m, off, LSFM_WAVE); m = o > m || o != o ? o : m; }
	if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
}

__global__ void k_gn_step(size_t n, const double* __restrict__ x0, const double* __restrict__ d, double alpha, const unsigned char* __restrict__ fixed, double* __restrict__ x)
{
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if (i < n) x[i] = (fixed && fixed[i]) ? x0[i] : x0[i] + alpha * d[i];
}

namespace {
struct Lab { int id, idx; };
int lab_find(const std::vector<Lab>& t, int id)
{
	auto it = std::lower_bound(t.begin(), t.end(), id, [](const Lab& a, int v) { return a.id < v; });
	return (it != t.end() && it->id == id) ? it->idx : -1;
}
inline dim3 grid_for(size_t n, int b) { return dim3((unsigned)std::max<size_t>(1, (n + b - 1) / b)); }

// what gn_setup leaves on the device for the calls' steps: the uploaded local maps, the joint system's structure, the work arrays
struct GnCall {
	int N = 0, M = 0, NFG = 0, P = 0, FI = 0, NUJ = 0, NWJ = 0;
	size_t RS = 0; // scalars of the global state
	bool mono = false;
	DevBatch X;
	std::vector<int> dof; // 6 m_k + 3 n_k
	GnMap* d_gm = nullptr;
	int *d_gp = nullptr, *d_gf = nullptr, *d_wdst = nullptr, *d_fptrJ = nullptr, *d_photoJ = nullptr, *d_fsp = nullptr, *d_fsi = nullptr, *d_psp = nullptr,
	    *d_psi = nullptr, *d_UiJ = nullptr, *d_UjJ = nullptr, *d_org = nullptr, *d_seg = nullptr, *d_dof = nullptr;
	unsigned char* d_fixed = nullptr;
	double *d_x = nullptr, *d_x0 = nullptr, *d_dl = nullptr, *Dp = nullptr, *Cp = nullptr, *rp = nullptr, *Gacc = nullptr, *Hacc = nullptr, *Fsum = nullptr;
	double *ePinst = nullptr, *Vinst = nullptr, *eFinst = nullptr, *UJ = nullptr, *WJ = nullptr, *VJ = nullptr, *ea = nullptr, *eb = nullptr;
	double *d_chi2 = nullptr, *d_w = nullptr, *d_G = nullptr;
	unsigned long long* d_max = nullptr;
};

// lsfm_map_feature_chi2 / lsfm_gn_polish_robust_features only: the per-feature arrays and, for the polish (slots), the correction slots
// of U.  Everything here follows from the labels and index arrays alone, never from values.
struct GnFeat {
	bool slots = true; // false: no system is assembled (lsfm_map_feature_chi2)
	int NS = 0;        // correction slots over all maps
	size_t NC = 0;     // contributors over all slots
	int *d_nu_own = nullptr, *d_sptr = nullptr, *d_cf = nullptr, *d_ca = nullptr, *d_cb = nullptr, *d_eptr = nullptr, *d_eidx = nullptr, *d_sdst = nullptr,
	    *d_bad = nullptr;
	double *fchi2 = nullptr, *fw = nullptr, *msum = nullptr, *pose_chi2 = nullptr;
};
// the correction slots on the host: per map one slot per distinct pair (a <= b, local poses) of poses that see a common feature, sorted by
// (a, b); per slot its contributors in feature order
struct GnSlots {
	std::vector<int> before;           // [N + 1] slots ahead of map k
	std::vector<int> a, b;             // [NS] the slot's local poses
	std::vector<int> sptr, cf, ca, cb; // contributors of slot s: sptr[s] .. sptr[s + 1]; feature instance, entries of a and of b
	std::vector<int> eptr, eidx;       // entry e = one (feature instance, pose): its W blocks eidx[eptr[e] .. eptr[e + 1]) (batch indices)
};
void gn_feature_slots(const lsfm_map* maps, int N, const DevBatch& X, GnSlots& sl)
{
	struct Tup { long long key; int f, ea, eb; };
	std::vector<Tup> tup;
	std::vector<std::pair<int, int>> run; // (local pose, W block)
	std::vector<int> ent, entpose;
	sl.before.assign(N + 1, 0); sl.sptr.clear(); sl.eptr.assign(1, 0);
	for (int k = 0; k < N; k++)
	{
		const lsfm_map& L = maps[k];
		tup.clear();
		int j = 0;
		for (int f = 0; f < L.n; f++)
		{
			run.clear();
			for (; j < L.nW && L.feature[j] == f; j++) run.push_back({ L.photo[j], X.w_off[k] + j });
			const auto by_pose = [](const std::pair<int, int>& p, const std::pair<int, int>& q) { return p.first < q.first; };
			if (!std::is_sorted(run.begin(), run.end(), by_pose)) std::stable_sort(run.begin(), run.end(), by_pose);
			ent.clear(); entpose.clear();
			for (size_t r = 0; r < run.size(); r++)
			{
				if (r == 0 || run[r].first != run[r - 1].first)
				{
					ent.push_back((int)sl.eptr.size() - 1); entpose.push_back(run[r].first);
					sl.eptr.push_back((int)sl.eidx.size());
				}
				sl.eidx.push_back(run[r].second);
				sl.eptr.back() = (int)sl.eidx.size();
			}
			for (size_t i = 0; i < ent.size(); i++)
				for (size_t q = i; q < ent.size(); q++) tup.push_back(Tup{ (long long)entpose[i] * L.m + entpose[q], X.feat_off[k] + f, ent[i], ent[q] });
		}
		const auto by_key = [](const Tup& p, const Tup& q) { return p.key < q.key; };
		if (!std::is_sorted(tup.begin(), tup.end(), by_key)) std::stable_sort(tup.begin(), tup.end(), by_key);
		if (sl.cf.size() + tup.size() > (size_t)INT32_MAX) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: too many co-observations for the feature weights' correction of U");
		for (size_t i = 0; i < tup.size(); i++)
		{
			if (i == 0 || tup[i].key != tup[i - 1].key)
			{
				sl.a.push_back((int)(tup[i].key / L.m)); sl.b.push_back((int)(tup[i].key % L.m));
				sl.sptr.push_back((int)sl.cf.size());
			}
			sl.cf.push_back(tup[i].f); sl.ca.push_back(tup[i].ea); sl.cb.push_back(tup[i].eb);
		}
		sl.before[k + 1] = (int)sl.a.size();
	}
	sl.sptr.push_back((int)sl.cf.size());
}

// lsfm_gn_linearise only: the joint system with every block once.  Output W sorted by feature, within a feature by pose; output U sorted
// by (i, j); per output block its sources in WJ / UJ as a CSR (wsp / wsi, usp / usi), in source (= map) order.  Index arrays on the host
// (they go straight into the map handed out), the CSR and the output blocks on the device.
struct GnCoalesce {
	int nWo = 0, nUo = 0;
	std::vector<int> photo, feature, FBlock, Ui, Uj, origin;
	int *d_wsp = nullptr, *d_wsi = nullptr, *d_usp = nullptr, *d_usi = nullptr;
	double *Wo = nullptr, *Uo = nullptr;
};

// the structure of a call, on the host from the labels, and the upload: which global variable every local one is, where every local
// block lands in the joint system, the gauge (Mono); the state x goes to d_x.  Throws Error (LSFM_ERR_ARG) for what it cannot place.
// weight (may be null: all 1): the maps' weights w_k.  co (may be null): the coalescing structure of lsfm_gn_linearise is built as well.
// fr (may be null): the per-feature arrays of the feature chi^2 pass; with fr->slots every map's U range is extended by its correction
// slots (c.X.U / Ui / Uj / NU then are the extended list, the maps' own blocks first).
void gn_setup(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, GnCall& c, const double* weight = nullptr, GnCoalesce* co = nullptr,
              GnFeat* fr = nullptr)
{
	const int M = c.M = x->m, NFG = c.NFG = x->n;
	c.N = N; c.mono = mono;
	if (M <= 0 || NFG < 0 || !x->stno || !x->stVal) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: the global state is empty");
	// ---- structure, once per call (host): which global variable every local one is, where every local block lands ----
	std::vector<Lab> pt(M), ft(NFG);
	for (int i = 0; i < M; i++) { if (x->stno[6 * i] > 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: state label of a pose must be <= 0"); pt[i] = Lab{ -x->stno[6 * i], i }; }
	for (int i = 0; i < NFG; i++) { if (x->stno[6 * M + 3 * i] <= 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: state label of a feature must be > 0"); ft[i] = Lab{ x->stno[6 * M + 3 * i], i }; }
	auto by_id = [](const Lab& a, const Lab& b) { return a.id < b.id; };
	std::sort(pt.begin(), pt.end(), by_id); std::sort(ft.begin(), ft.end(), by_id);
	size_t need = (size_t)128 << 20;
	{
		size_t P = 0, FI = 0, nW = 0, nU = 0;
		for (int k = 0; k < N; k++) { P += maps[k].m; FI += maps[k].n; nW += maps[k].nW; nU += maps[k].nU; }
		need += ((nW + 2 * FI) * 400 + (nU + 3 * P + 3 * (size_t)N) * 800 + (FI + NFG) * 500 + (P + M) * 6000) * 2 + (size_t)N * 64;
		// (the coalesced blocks and their source lists: at most one output block and one source per joint block)
		if (co) need += (nW + 2 * FI) * (144 + 16) + (nU + 2 * P + 3 * (size_t)N) * (288 + 16) + 1024;
		if (fr)
		{
			// per feature 2 doubles; slots: at most one per contributor, a contributor per pair of blocks of a feature's run
			size_t nc = 0;
			for (int k = 0; k < N; k++)
				for (int j = 0, len = 0; j < maps[k].nW; j++)
				{
					len++;
					if (j + 1 == maps[k].nW || maps[k].feature[j + 1] != maps[k].feature[j]) { nc += (size_t)len * (len + 1) / 2; len = 0; }
				}
			need += FI * 16 + (size_t)N * 64 + 4096;
			if (fr->slots) need += (nU + nc) * (288 + 800 + 8 + 288) + nc * (16 + 36) + nW * 8;
		}
	}
	ctx->ensure_arenas(need);
	ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
	Arena& ar = ctx->arena[0];
	DevBatch& X = c.X;
	batch_upload(ctx, ar, maps, N, mono, X);
	const int P = c.P = X.M, FI = c.FI = X.NF;
	GnSlots sl;
	if (fr && fr->slots) gn_feature_slots(maps, N, X, sl);
	else sl.before.assign(N + 1, 0);
	std::vector<GnMap> gm(N);
	c.dof.resize(N);
	std::vector<int> gp(P), gfi(FI), wdst(FI), origin(M, INT32_MAX);
	std::vector<int> fcnt(NFG + 1, 0), pcnt(M + 1, 0);
	int NUJ = 0;
	for (int k = 0; k < N; k++)
	{
		const lsfm_map& L = maps[k];
		GnMap& t = gm[k];
		memset(&t, 0, sizeof t);
		t.p0 = X.pose_off[k]; t.m = L.m; t.f0 = X.feat_off[k]; t.n = L.n; t.u0 = X.u_off[k] + sl.before[k]; t.nu = L.nU + (sl.before[k + 1] - sl.before[k]);
		t.hub[0] = t.hub[1] = -1;
		t.w = weight ? weight[k] : 1.0;
		if ((c.dof[k] = 6 * L.m + 3 * L.n) <= 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: local map " + std::to_string(k + 1) + " is empty");
		if (!mono && L.Ref == x->Ref) t.nh = 0;
		else
		{
			t.nh = mono ? 2 : 1;
			if ((t.hub[0] = lab_find(pt, L.Ref)) < 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: the reference pose of local map " + std::to_string(k + 1) + " is not in the global state");
			if (mono)
			{
				if ((t.hub[1] = lab_find(pt, L.ScaP)) < 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: the scale pose of local map " + std::to_string(k + 1) + " is not in the global state");
				if (L.Fix < 0 || L.Fix > 2) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: Fix must be 0, 1 or 2");
				t.fix = L.Fix;
			}
		}
		t.ubase = NUJ;
		NUJ += t.nh * L.m + t.nh * (t.nh + 1) / 2 + t.nu;
		for (int i = 0; i < L.m; i++)
		{
			const int g = lab_find(pt, -L.stno[6 * i]);
			if (g < 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: a pose of local map " + std::to_string(k + 1) + " is not in the global state (Stereo: the global reference pose cannot be a variable of a map)");
			gp[t.p0 + i] = g; pcnt[g + 1]++;
			origin[g] = std::min(origin[g], k);
		}
		for (int sdx = 0; sdx < t.nh; sdx++) { pcnt[t.hub[sdx] + 1]++; origin[t.hub[sdx]] = std::min(origin[t.hub[sdx]], k); }
		for (int i = 0; i < L.n; i++)
		{
			const int g = lab_find(ft, L.stno[6 * L.m + 3 * i]);
			if (g < 0) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: a feature of local map " + std::to_string(k + 1) + " is not in the global state");
			gfi[t.f0 + i] = g;
		}
	}
	// joint W: per global feature its instances in map order, an instance's hub block(s) ahead of its own run
	std::vector<int> fptr_loc(FI + 1);
	for (int k = 0; k < N; k++)
	{
		int j = 0; // (W sorted by feature, every feature at least one block: batch_upload has checked)
		for (int f = 0; f < maps[k].n; f++) { fptr_loc[X.feat_off[k] + f] = X.w_off[k] + j; while (j < maps[k].nW && maps[k].feature[j] == f) j++; }
	}
	fptr_loc[FI] = X.NW;
	std::vector<int> fptrJ(NFG + 1, 0);
	for (int k = 0; k < N; k++)
		for (int f = X.feat_off[k]; f < X.feat_off[k + 1]; f++) { fptrJ[gfi[f] + 1] += gm[k].nh + (fptr_loc[f + 1] - fptr_loc[f]); fcnt[gfi[f] + 1]++; }
	for (int g = 0; g < NFG; g++)
	{
		if (!fcnt[g + 1]) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: a feature of the global state is in no local map");
		fptrJ[g + 1] += fptrJ[g]; fcnt[g + 1] += fcnt[g];
	}
	for (int g = 0; g < M; g++)
	{
		if (!pcnt[g + 1]) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: a pose of the global state is in no local map");
		pcnt[g + 1] += pcnt[g];
	}
	const int NWJ = c.NWJ = fptrJ[NFG];
	std::vector<int> photoJ(NWJ), fsrc(FI), psrc(pcnt[M]);
	{
		std::vector<int> wcur(fptrJ.begin(), fptrJ.end() - 1), fcur(fcnt.begin(), fcnt.end() - 1), pcur(pcnt.begin(), pcnt.end() - 1);
		for (int k = 0; k < N; k++)
		{
			const GnMap& t = gm[k];
			for (int f = t.f0; f < t.f0 + t.n; f++)
			{
				const int g = gfi[f], len = fptr_loc[f + 1] - fptr_loc[f];
				wdst[f] = wcur[g];
				for (int sdx = 0; sdx < t.nh; sdx++) photoJ[wcur[g]++] = t.hub[sdx];
				for (int j = 0; j < len; j++) photoJ[wcur[g]++] = gp[t.p0 + maps[k].photo[fptr_loc[f] - X.w_off[k] + j]];
				fsrc[fcur[g]++] = f;
			}
			for (int a = t.p0; a < t.p0 + t.m; a++) psrc[pcur[gp[a]]++] = a;
			for (int sdx = 0; sdx < t.nh; sdx++) psrc[pcur[t.hub[sdx]]++] = -1 - (2 * k + sdx);
		}
	}
	// joint U coordinates (row <= column)
	std::vector<int> UiJ(NUJ), UjJ(NUJ);
	for (int k = 0; k < N; k++)
	{
		const GnMap& t = gm[k];
		int q = t.ubase;
		for (int sdx = 0; sdx < t.nh; sdx++)
			for (int a = 0; a < t.m; a++, q++) { const int ga = gp[t.p0 + a], h = t.hub[sdx]; UiJ[q] = std::min(ga, h); UjJ[q] = std::max(ga, h); }
		if (t.nh >= 1) { UiJ[q] = UjJ[q] = t.hub[0]; q++; }
		if (t.nh == 2) { UiJ[q] = std::min(t.hub[0], t.hub[1]); UjJ[q] = std::max(t.hub[0], t.hub[1]); q++; UiJ[q] = UjJ[q] = t.hub[1]; q++; }
		for (int i = 0; i < t.nu; i++, q++)
		{
			// (the map's own blocks, then its correction slots)
			const int own = maps[k].nU, sq = sl.before[k] + i - own;
			const int ga = gp[t.p0 + (i < own ? maps[k].Ui[i] : sl.a[sq])], gb = gp[t.p0 + (i < own ? maps[k].Uj[i] : sl.b[sq])];
			UiJ[q] = std::min(ga, gb); UjJ[q] = std::max(ga, gb);
		}
	}
	if (x->pose_origin) for (int g = 0; g < M; g++) origin[g] = x->pose_origin[g];
	std::vector<unsigned char> fixed;
	if (mono)
	{
		const int pr = lab_find(pt, x->Ref), ps = lab_find(pt, x->ScaP);
		if (pr < 0 || ps < 0 || x->Fix < 0 || x->Fix > 2) LSFM_FAIL(LSFM_ERR_ARG, "gn polish: the global state's reference / scale pose (Ref, ScaP, Fix) is not in it");
		fixed.assign((size_t)M * 6 + (size_t)NFG * 3, 0);
		for (int i = 0; i < 6; i++) fixed[(size_t)pr * 6 + i] = 1;
		fixed[(size_t)ps * 6 + x->Fix] = 1;
	}
	// ---- device arrays ----
	const size_t RS = c.RS = (size_t)M * 6 + (size_t)NFG * 3;
	c.NUJ = NUJ;
	GnMap* d_gm = c.d_gm = ar.alloc<GnMap>(N);
	int *d_gp = c.d_gp = ar.alloc<int>(P), *d_gf = c.d_gf = ar.alloc<int>(FI), *d_wdst = c.d_wdst = ar.alloc<int>(FI);
	int *d_fptrJ = c.d_fptrJ = ar.alloc<int>(NFG + 1), *d_photoJ = c.d_photoJ = ar.alloc<int>(NWJ);
	int *d_fsp = c.d_fsp = ar.alloc<int>(NFG + 1), *d_fsi = c.d_fsi = ar.alloc<int>(FI), *d_psp = c.d_psp = ar.alloc<int>(M + 1), *d_psi = c.d_psi = ar.alloc<int>(psrc.size());
	int *d_UiJ = c.d_UiJ = ar.alloc<int>(NUJ), *d_UjJ = c.d_UjJ = ar.alloc<int>(NUJ), *d_org = c.d_org = ar.alloc<int>(M), *d_seg = c.d_seg = ar.alloc<int>(M + NFG + 1);
	unsigned char* d_fixed = c.d_fixed = mono ? ar.alloc<unsigned char>(RS) : nullptr;
	c.d_x = ar.alloc<double>(RS); c.d_x0 = ar.alloc<double>(RS); c.d_dl = ar.alloc<double>(RS);
	c.Dp = ar.alloc<double>((size_t)P * 36); c.Cp = ar.alloc<double>((size_t)P * 72); c.rp = ar.alloc<double>((size_t)P * 6);
	c.Gacc = ar.alloc<double>((size_t)P * GN_GW + (size_t)N * GN_HW + 2); c.Hacc = c.Gacc + (size_t)P * GN_GW; c.Fsum = c.Hacc + (size_t)N * GN_HW;
	c.ePinst = ar.alloc<double>((size_t)P * 6); c.Vinst = ar.alloc<double>((size_t)FI * 9); c.eFinst = ar.alloc<double>((size_t)FI * 3);
	c.UJ = ar.alloc<double>((size_t)NUJ * 36); c.WJ = ar.alloc<double>((size_t)NWJ * 18); c.VJ = ar.alloc<double>((size_t)NFG * 9);
	c.ea = ar.alloc<double>((size_t)M * 6); c.eb = ar.alloc<double>((size_t)NFG * 3);
	c.d_max = ar.alloc<unsigned long long>(2);
	c.d_dof = ar.alloc<int>(N); c.d_chi2 = ar.alloc<double>(N); c.d_w = ar.alloc<double>(N); c.d_G = ar.alloc<double>(1);
	h2d(ctx, d_gm, gm.data(), gm.size() * sizeof(GnMap));
	h2d(ctx, d_gp, gp.data(), gp.size() * sizeof(int)); h2d(ctx, d_gf, gfi.data(), gfi.size() * sizeof(int)); h2d(ctx, d_wdst, wdst.data(), wdst.size() * sizeof(int));
	h2d(ctx, d_fptrJ, fptrJ.data(), fptrJ.size() * sizeof(int)); h2d(ctx, d_photoJ, photoJ.data(), photoJ.size() * sizeof(int));
	h2d(ctx, d_fsp, fcnt.data(), fcnt.size() * sizeof(int)); h2d(ctx, d_fsi, fsrc.data(), fsrc.size() * sizeof(int));
	h2d(ctx, d_psp, pcnt.data(), pcnt.size() * sizeof(int)); h2d(ctx, d_psi, psrc.data(), psrc.size() * sizeof(int));
	h2d(ctx, d_UiJ, UiJ.data(), UiJ.size() * sizeof(int)); h2d(ctx, d_UjJ, UjJ.data(), UjJ.size() * sizeof(int));
	h2d(ctx, d_org, origin.data(), origin.size() * sizeof(int));
	if (mono) h2d(ctx, d_fixed, fixed.data(), fixed.size());
	h2d(ctx, c.d_dof, c.dof.data(), c.dof.size() * sizeof(int));
	h2d(ctx, c.d_x, x->stVal, RS * sizeof(double));
	dev_zero(ctx, d_seg, (size_t)(M + NFG + 1) * sizeof(int));
	if (fr)
	{
		std::vector<int> nu_own(N);
		for (int k = 0; k < N; k++) nu_own[k] = maps[k].nU;
		fr->d_nu_own = ar.alloc<int>(N); fr->d_bad = ar.alloc<int>(1);
		fr->fchi2 = ar.alloc<double>(FI); fr->fw = ar.alloc<double>(FI); fr->msum = ar.alloc<double>((size_t)3 * N); fr->pose_chi2 = ar.alloc<double>(N);
		h2d(ctx, fr->d_nu_own, nu_own.data(), nu_own.size() * sizeof(int));
		const int none = INT32_MAX;
		h2d(ctx, fr->d_bad, &none, sizeof(int));
	}
	if (fr && fr->slots)
	{
		// the extended U list: every map's own blocks (copied once: k_gn_extend_u), then its slots (k_gn_feature_ufill, every assembly)
		const int NS = fr->NS = (int)sl.a.size(), NUX = X.NU + NS;
		fr->NC = sl.cf.size();
		std::vector<int> Uix(NUX), Ujx(NUX), sdst(NS), ushift(N);
		for (int k = 0; k < N; k++)
		{
			const GnMap& t = gm[k];
			ushift[k] = sl.before[k];
			for (int i = 0; i < maps[k].nU; i++) { Uix[t.u0 + i] = t.p0 + maps[k].Ui[i]; Ujx[t.u0 + i] = t.p0 + maps[k].Uj[i]; }
			for (int q = sl.before[k]; q < sl.before[k + 1]; q++)
			{
				const int d = t.u0 + maps[k].nU + (q - sl.before[k]);
				sdst[q] = d; Uix[d] = t.p0 + sl.a[q]; Ujx[d] = t.p0 + sl.b[q];
			}
		}
		double* Ux = ar.alloc<double>((size_t)NUX * 36);
		int *d_Uix = ar.alloc<int>(NUX), *d_Ujx = ar.alloc<int>(NUX), *d_ushift = ar.alloc<int>(N);
		fr->d_sptr = ar.alloc<int>(NS + 1); fr->d_cf = ar.alloc<int>(fr->NC); fr->d_ca = ar.alloc<int>(fr->NC); fr->d_cb = ar.alloc<int>(fr->NC);
		fr->d_eptr = ar.alloc<int>(sl.eptr.size()); fr->d_eidx = ar.alloc<int>(sl.eidx.size()); fr->d_sdst = ar.alloc<int>(NS);
		h2d(ctx, d_Uix, Uix.data(), Uix.size() * sizeof(int)); h2d(ctx, d_Ujx, Ujx.data(), Ujx.size() * sizeof(int));
		h2d(ctx, d_ushift, ushift.data(), ushift.size() * sizeof(int));
		h2d(ctx, fr->d_sptr, sl.sptr.data(), sl.sptr.size() * sizeof(int));
		h2d(ctx, fr->d_cf, sl.cf.data(), sl.cf.size() * sizeof(int)); h2d(ctx, fr->d_ca, sl.ca.data(), sl.ca.size() * sizeof(int));
		h2d(ctx, fr->d_cb, sl.cb.data(), sl.cb.size() * sizeof(int));
		h2d(ctx, fr->d_eptr, sl.eptr.data(), sl.eptr.size() * sizeof(int)); h2d(ctx, fr->d_eidx, sl.eidx.data(), sl.eidx.size() * sizeof(int));
		h2d(ctx, fr->d_sdst, sdst.data(), sdst.size() * sizeof(int));
		dev_zero(ctx, Ux, (size_t)NUX * 36 * sizeof(double));
		if (X.NU) hipLaunchKernelGGL(k_gn_extend_u, grid_for(X.NU, 256), dim3(256), 0, ctx->stream, X.NU, X.Ui, X.pose_map, d_ushift, X.U, Ux);
		X.U = Ux; X.Ui = d_Uix; X.Uj = d_Ujx; X.NU = NUX;
	}
	if (co)
	{
		// W: every feature's joint run sorted stably by pose, equal poses merged
		std::vector<int> wsp(1, 0), wsi(NWJ), usp(1, 0), usi(NUJ);
		co->photo.clear(); co->feature.clear(); co->FBlock.assign(NFG, 0);
		for (int q = 0; q < NWJ; q++) wsi[q] = q;
		for (int g = 0; g < NFG; g++)
		{
			std::stable_sort(wsi.begin() + fptrJ[g], wsi.begin() + fptrJ[g + 1], [&](int a, int b) { return photoJ[a] < photoJ[b]; });
			co->FBlock[g] = (int)co->photo.size();
			for (int q = fptrJ[g]; q < fptrJ[g + 1]; q++)
			{
				if (q > fptrJ[g] && photoJ[wsi[q]] == photoJ[wsi[q - 1]]) continue;
				if (q > 0) wsp.push_back(q);
				co->photo.push_back(photoJ[wsi[q]]); co->feature.push_back(g);
			}
		}
		wsp.push_back(NWJ);
		if (NWJ == 0) wsp.assign(1, 0);
		// U: the joint keys sorted stably by (i, j), equal keys merged
		for (int q = 0; q < NUJ; q++) usi[q] = q;
		std::stable_sort(usi.begin(), usi.end(), [&](int a, int b) { return UiJ[a] != UiJ[b] ? UiJ[a] < UiJ[b] : UjJ[a] < UjJ[b]; });
		co->Ui.clear(); co->Uj.clear();
		for (int q = 0; q < NUJ; q++)
		{
			if (q > 0 && UiJ[usi[q]] == UiJ[usi[q - 1]] && UjJ[usi[q]] == UjJ[usi[q - 1]]) continue;
			if (q > 0) usp.push_back(q);
			co->Ui.push_back(UiJ[usi[q]]); co->Uj.push_back(UjJ[usi[q]]);
		}
		usp.push_back(NUJ);
		if (NUJ == 0) usp.assign(1, 0);
		co->nWo = (int)co->photo.size(); co->nUo = (int)co->Ui.size();
		co->origin = origin;
		co->d_wsp = ar.alloc<int>(wsp.size()); co->d_wsi = ar.alloc<int>(NWJ); co->d_usp = ar.alloc<int>(usp.size()); co->d_usi = ar.alloc<int>(NUJ);
		co->Wo = ar.alloc<double>((size_t)co->nWo * 18); co->Uo = ar.alloc<double>((size_t)co->nUo * 36);
		h2d(ctx, co->d_wsp, wsp.data(), wsp.size() * sizeof(int)); h2d(ctx, co->d_wsi, wsi.data(), wsi.size() * sizeof(int));
		h2d(ctx, co->d_usp, usp.data(), usp.size() * sizeof(int)); h2d(ctx, co->d_usi, usi.data(), usi.size() * sizeof(int));
	}
}

// the frames of the maps at the state in d_x, the pose residuals r_a with their D_a and C_s,a
void gn_frames(lsfm_context* ctx, const GnCall& c)
{
	hipStream_t s = ctx->stream;
	hipLaunchKernelGGL(k_gn_hubs, grid_for(c.N, 128), dim3(128), 0, s, c.N, c.d_gm, c.d_x);
	hipLaunchKernelGGL(k_gn_poses, grid_for(c.P, 128), dim3(128), 0, s, c.P, c.X.pose_map, c.d_gm, c.d_gp, c.d_x, c.X.pose, c.Dp, c.Cp, c.rp);
}

// chi2_k of every map into d_chi2 (after gn_frames)
void gn_chi2(lsfm_context* ctx, const GnCall& c)
{
	hipLaunchKernelGGL(k_gn_map_chi2, dim3(c.N), dim3(GN_CHI2_LANES), 0, ctx->stream, c.d_gm, c.X.U, c.X.Ui, c.X.Uj, c.rp, c.d_gf,
	                   c.d_x + (size_t)c.M * 6, c.X.feat, c.X.fptr, c.X.photo, c.X.W, c.X.V, c.d_chi2);
}
// c_kf, w_kf and the per-map sums at the state in d_x (after gn_frames), then pose_chi2 and G into d_G
void gn_feature_chi2(lsfm_context* ctx, const GnCall& c, const GnFeat& fr, int kind, double cth)
{
	hipLaunchKernelGGL(k_gn_feature_chi2, dim3(c.N), dim3(GN_FCHI2_LANES), 0, ctx->stream, kind, cth, c.d_gm, fr.d_nu_own, c.X.U, c.X.Ui, c.X.Uj, c.rp,
	                   c.d_gf, c.d_x + (size_t)c.M * 6, c.X.feat, c.X.fptr, c.X.photo, c.X.W, c.X.V, fr.fchi2, fr.fw, fr.msum, fr.d_bad);
	hipLaunchKernelGGL(k_gn_feature_objective, dim3(1), dim3(GN_WEIGHT_LANES), 0, ctx->stream, c.N, fr.msum, fr.pose_chi2, c.d_G);
}
// what k_gn_feature_chi2 found: throws LSFM_ERR_NOT_SPD naming the first feature whose V is not positive definite
void gn_feature_check(lsfm_context* ctx, const lsfm_map* maps, const GnCall& c, const GnFeat& fr)
{
	int bad = INT32_MAX;
	d2h(ctx, &bad, fr.d_bad, sizeof(int));
	if (bad == INT32_MAX) return;
	const int k = (int)(std::upper_bound(c.X.feat_off.begin(), c.X.feat_off.end(), bad) - c.X.feat_off.begin()) - 1, f = bad - c.X.feat_off[k];
	LSFM_FAIL(LSFM_ERR_NOT_SPD, "feature chi2: V of feature " + std::to_string(f + 1) + " (label " + std::to_string(maps[k].stno[6 * maps[k].m + 3 * f]) +
	                                ") of local map " + std::to_string(k + 1) + " is not positive definite");
}
// the launches of one assembly at the state in d_x: F into Fsum (kind != 0: the robust weights first, G into d_G), the joint system
// UJ / WJ / VJ and the right-hand sides ea / eb.  bracket_chi2 (may be null): [2] events recorded around the chi2 + weights kernels.
// fr (may be null; then kind != 0): the estimator is on the features -- the feature chi2 pass (G into d_G), the correction slots of U,
// W and V weighted per feature; the maps' own weights stay as gn_setup left them.  bracket_chi2 then is [4]: [2], [3] around the slots' fill.
void gn_assemble(lsfm_context* ctx, const GnCall& c, int kind, double cth, const hipEvent_t* bracket_chi2, const GnFeat* fr = nullptr)
{
	hipStream_t s = ctx->stream;
	const DevBatch& X = c.X;
	const int N = c.N, M = c.M, NFG = c.NFG, P = c.P, FI = c.FI;
	const bool mono = c.mono;
	dev_zero(ctx, c.Gacc, ((size_t)P * GN_GW + (size_t)N * GN_HW + 2) * sizeof(double));
	gn_frames(ctx, c);
	if (fr)
	{
		if (bracket_chi2) LSFM_CHECK_HIP(hipEventRecord(bracket_chi2[0], s));
		gn_feature_chi2(ctx, c, *fr, kind, cth);
		if (bracket_chi2) { LSFM_CHECK_HIP(hipEventRecord(bracket_chi2[1], s)); LSFM_CHECK_HIP(hipEventRecord(bracket_chi2[2], s)); }
		if (fr->NS)
			hipLaunchKernelGGL(k_gn_feature_ufill, grid_for(fr->NS, GN_UFILL_LANES / LSFM_WAVE), dim3(GN_UFILL_LANES), 0, s, fr->NS, fr->d_sptr, fr->d_cf, fr->d_ca,
			                   fr->d_cb, fr->d_eptr, fr->d_eidx, fr->d_sdst, X.W, X.V, fr->fw, X.U);
		if (bracket_chi2) LSFM_CHECK_HIP(hipEventRecord(bracket_chi2[3], s));
	}
	else if (kind != 0)
	{
		if (bracket_chi2) LSFM_CHECK_HIP(hipEventRecord(bracket_chi2[0], s));
		gn_chi2(ctx, c);
		hipLaunchKernelGGL(k_gn_robust_weights, dim3(1), dim3(GN_WEIGHT_LANES), 0, s, N, kind, cth, c.d_dof, c.d_chi2, c.d_gm, c.d_w, c.d_G);
		if (bracket_chi2) LSFM_CHECK_HIP(hipEventRecord(bracket_chi2[1], s));
	}
	if (X.NU) hipLaunchKernelGGL(k_gn_ublocks, grid_for(X.NU, 128), dim3(128), 0, s, X.NU, P, X.Ui, X.Uj, X.U, X.pose_map, c.d_gm, c.d_gp, c.Dp, c.Cp, c.rp, c.Gacc, c.UJ);
	if (FI)
	{
#define GN_FEATURES_CALL X.feat_map, c.d_gm, c.d_gf, c.d_x + (size_t)M * 6, X.feat, X.fptr, X.photo, X.W, X.V, c.Dp, c.Cp, c.rp, c.d_wdst, c.WJ, c.Vinst, c.eFinst, c.Gacc, c.Hacc
		const double* none = nullptr;
		if (fr)
		{
			if (mono) hipLaunchKernelGGL((k_gn_features<2, true>), grid_for(FI, 256), dim3(256), 0, s, FI, P, GN_FEATURES_CALL, fr->fw);
			else hipLaunchKernelGGL((k_gn_features<1, true>), grid_for(FI, 256), dim3(256), 0, s, FI, P, GN_FEATURES_CALL, fr->fw);
		}
		else if (mono) hipLaunchKernelGGL((k_gn_features<2, false>), grid_for(FI, 256), dim3(256), 0, s, FI, P, GN_FEATURES_CALL, none);
		else hipLaunchKernelGGL((k_gn_features<1, false>), grid_for(FI, 256), dim3(256), 0, s, FI, P, GN_FEATURES_CALL, none);
#undef GN_FEATURES_CALL
	}
	hipLaunchKernelGGL(k_gn_pose_post, grid_for(P, 128), dim3(128), 0, s, P, X.pose_map, c.d_gm, c.d_gp, c.Dp, c.Cp, c.rp, c.Gacc, c.UJ, c.ePinst, c.Hacc);
	hipLaunchKernelGGL(k_gn_hubhub, grid_for(N, 128), dim3(128), 0, s, N, c.d_gm, c.Hacc, c.UJ, c.Fsum);
	if (NFG) hipLaunchKernelGGL(k_gn_gather_feat, grid_for(NFG, 256), dim3(256), 0, s, NFG, c.d_fsp, c.d_fsi, c.Vinst, c.eFinst, c.VJ, c.eb);
	hipLaunchKernelGGL(k_gn_gather_pose, grid_for(M, 128), dim3(128), 0, s, M, c.d_psp, c.d_psi, c.ePinst, c.Hacc, c.ea);
}
} // namespace

// x: the global state (stno / stVal / m / n, Ref; Mono: ScaP, Fix; optional pose_origin); stVal is updated in place.
// kind: 0 the plain polish (F, every weight 1: no chi^2 is formed during the steps), 1 Huber, 2 Cauchy on s_k = chi2_k / dof_k with
// threshold c (IRLS: every assembly forms chi2, the weights w_k = rho'(s_k) and G first, then the system with w_k I_k).
// obj / gnorm: [iters + 1]; halvings: [iters] or null; chi2 / weight: [N] or null, at the returned state.  Returns LSFM_OK or
// LSFM_NOT_CONVERGED (a step's camera system was left above its residual bound); throws Error for invalid input.
// feat: the estimator is on the features (kind 1 or 2): G of lsfm_gn_polish_robust_features; chi2 / weight then are per local feature
// instance [sum n_k] and the maps keep weight 1.
int gn_polish(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, int kind, double cth, double* obj, double* gnorm,
              int* halvings, double* chi2, double* weight, bool feat)
{
	hipStream_t s = ctx->stream;
	// LSFM_GN_TIMING=1: wall clock of the call's parts on stderr (every part ends with a synchronisation of its own)
	static const bool timing = getenv("LSFM_GN_TIMING") != nullptr;
	auto wall = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double tw0 = wall();
	double t_asm = 0.0, t_solve = 0.0, t_chi2 = 0.0, t_fill = 0.0;
	int n_asm = 0, n_solve = 0;
	GnCall c;
	GnFeat fr;
	gn_setup(ctx, maps, N, mono, x, c, nullptr, nullptr, feat ? &fr : nullptr);
	const int M = c.M, NFG = c.NFG;
	const size_t RS = c.RS;
	const bool robust = kind != 0;

	// F (robust: G) and the step's system at the state in d_x
	hipEvent_t e_chi2[4] = { nullptr, nullptr, nullptr, nullptr };
	if (robust && timing) for (int i = 0; i < (feat ? 4 : 2); i++) e_chi2[i] = ctx->pool_event();
	auto assemble = [&]() -> double {
		const double ta = wall();
		gn_assemble(ctx, c, kind, cth, robust && timing ? e_chi2 : nullptr, feat ? &fr : nullptr);
		double F = 0.0;
		d2h(ctx, &F, robust ? c.d_G : c.Fsum, sizeof(double));
		if (feat && n_asm == 0) gn_feature_check(ctx, maps, c, fr); // (V does not change during the call)
		if (robust && timing)
		{
			float ms = 0.0f;
			LSFM_CHECK_HIP(hipEventElapsedTime(&ms, e_chi2[0], e_chi2[1]));
			t_chi2 += ms;
			if (feat) { LSFM_CHECK_HIP(hipEventElapsedTime(&ms, e_chi2[2], e_chi2[3])); t_fill += ms; }
		}
		t_asm += wall() - ta; n_asm++;
		return F;
	};
	auto grad_norm = [&]() -> double {
		dev_zero(ctx, c.d_max, 2 * sizeof(unsigned long long));
		hipLaunchKernelGGL(k_gn_maxabs, dim3(256), dim3(256), 0, s, (size_t)M * 6, c.ea, c.d_fixed, c.d_max);
		if (NFG) hipLaunchKernelGGL(k_gn_maxabs, dim3(256), dim3(256), 0, s, (size_t)NFG * 3, c.eb, (const unsigned char*)nullptr, c.d_max);
		double v = 0.0;
		d2h(ctx, &v, c.d_max, sizeof(double));
		return v;
	};
	SolveIO io;
	io.M = M; io.NF = NFG; io.NU = c.NUJ; io.NW = c.NWJ; io.nseg = 1;
	io.d_pose_seg = c.d_seg; io.d_feat_seg = c.d_seg + M;
	io.U = c.UJ; io.Ui = c.d_UiJ; io.Uj = c.d_UjJ; io.W = c.WJ; io.photo = c.d_photoJ; io.fptr = c.d_fptrJ; io.V = c.VJ;
	io.ea = c.ea; io.eb = c.eb; io.x_pose = c.d_dl; io.x_feat = c.d_dl + (size_t)M * 6;
	io.d_fixed = c.d_fixed; io.d_pose_origin = c.d_org;
	io.seg_rows.assign(1, M);

	int ret = LSFM_OK;
	bool stopped = false;
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	const double tw1 = wall();
	double F = assemble();
	for (int it = 0; it <= iters; it++)
	{
		obj[it] = F; gnorm[it] = grad_norm();
		if (it == iters) break;
		if (halvings) halvings[it] = 0;
		if (stopped) continue;
		if (!(F == F)) LSFM_FAIL(LSFM_ERR_INTERNAL, "gn polish: the objective is not a number");
		const size_t smark = ctx->scratch.mark();
		const double ts = wall();
		const int rc = solve_batch(ctx, io).not_converged;
		LSFM_CHECK_HIP(hipStreamSynchronize(s));
		t_solve += wall() - ts; n_solve++;
		ctx->scratch.release(smark);
		if (rc) ret = LSFM_NOT_CONVERGED;
		LSFM_CHECK_HIP(hipMemcpyAsync(c.d_x0, c.d_x, RS * sizeof(double), hipMemcpyDeviceToDevice, s));
		double alpha = 1.0, F1 = 0.0;
		int h = 0;
		for (; h <= 8; h++, alpha *= 0.5)
		{
			hipLaunchKernelGGL(k_gn_step, grid_for(RS, 256), dim3(256), 0, s, RS, c.d_x0, c.d_dl, alpha, c.d_fixed, c.d_x);
			F1 = assemble(); // (the system at the new state: the next step's, when this one is taken)
			if (F1 <= F + 1e-12 * fabs(F)) break; // (at the minimiser two evaluations differ by their rounding)
		}
		if (h > 8)
		{
			// no decrease along the step: the state stays where it was, the run ends
			LSFM_CHECK_HIP(hipMemcpyAsync(c.d_x, c.d_x0, RS * sizeof(double), hipMemcpyDeviceToDevice, s));
			F = assemble();
			stopped = true;
		}
		else F = F1;
		if (halvings) halvings[it] = h > 8 ? 9 : h;
	}
	d2h(ctx, x->stVal, c.d_x, RS * sizeof(double));
	// chi2 / weights at the returned state: the last assembly's (robust), or formed once now from its frames and residuals (plain)
	if (feat)
	{
		if (chi2 && c.FI) d2h(ctx, chi2, fr.fchi2, (size_t)c.FI * sizeof(double));
		if (weight && c.FI) d2h(ctx, weight, fr.fw, (size_t)c.FI * sizeof(double));
	}
	else
	{
		if (chi2)
		{
			if (!robust) gn_chi2(ctx, c);
			d2h(ctx, chi2, c.d_chi2, (size_t)N * sizeof(double));
		}
		if (weight)
		{
			if (robust) d2h(ctx, weight, c.d_w, (size_t)N * sizeof(double));
			else std::fill(weight, weight + N, 1.0);
		}
	}
	if (timing && feat)
		fprintf(stderr, "lsfm_gn: %d maps, %d poses, %d features, joint system %d U / %d W blocks; structure + upload %.2f ms, %d assemblies %.2f ms each "
		                "(chi2 + weights %.3f ms each, U correction %.3f ms each: %d slots, %zu contributors), %d solves %.2f ms each, call %.2f ms\n", N, M, NFG,
		        c.NUJ, c.NWJ, tw1 - tw0, n_asm, n_asm ? t_asm / n_asm : 0.0, n_asm ? t_chi2 / n_asm : 0.0, n_asm ? t_fill / n_asm : 0.0, fr.NS, fr.NC, n_solve,
		        n_solve ? t_solve / n_solve : 0.0, wall() - tw0);
	else if (timing)
		fprintf(stderr, "lsfm_gn: %d maps, %d poses, %d features, joint system %d U / %d W blocks; structure + upload %.2f ms, %d assemblies %.2f ms each "
		                "(chi2 + weights %.3f ms each), %d solves %.2f ms each, call %.2f ms\n", N, M, NFG, c.NUJ, c.NWJ, tw1 - tw0, n_asm,
		        n_asm ? t_asm / n_asm : 0.0, n_asm ? t_chi2 / n_asm : 0.0, n_solve, n_solve ? t_solve / n_solve : 0.0, wall() - tw0);
	return ret;
}

// chi2_k of every local map at the global state x (x is read only); dof (may be null) = 6 m_k + 3 n_k
int map_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, double* chi2, int* dof)
{
	GnCall c;
	gn_setup(ctx, maps, N, mono, x, c);
	gn_frames(ctx, c);
	gn_chi2(ctx, c);
	d2h(ctx, chi2, c.d_chi2, (size_t)N * sizeof(double));
	if (dof) std::copy(c.dof.begin(), c.dof.end(), dof);
	return LSFM_OK;
}

// c_kf of every local feature instance at the global state x (x is read only), in map order and within a map in its feature order;
// pose_chi2 (may be null) [N] = chi2_k - sum_f c_kf
int map_feature_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, double* fchi2, double* pose_chi2)
{
	GnCall c;
	GnFeat fr;
	fr.slots = false;
	gn_setup(ctx, maps, N, mono, x, c, nullptr, nullptr, &fr);
	gn_frames(ctx, c);
	gn_feature_chi2(ctx, c, fr, 0, 1.0);
	gn_feature_check(ctx, maps, c, fr);
	if (c.FI) d2h(ctx, fchi2, fr.fchi2, (size_t)c.FI * sizeof(double));
	if (pose_chi2) d2h(ctx, pose_chi2, fr.pose_chi2, (size_t)N * sizeof(double));
	return LSFM_OK;
}

// lsfm_gn_polish_robust_features: kind 0 is the plain polish with the feature chi2 of its result; fchi2 / fweight [sum n_k], may be null
int gn_polish_features(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, int kind, double cth, double* obj, double* gnorm,
                       int* halvings, double* fchi2, double* fweight)
{
	if (kind != 0) return gn_polish(ctx, maps, N, mono, x, iters, kind, cth, obj, gnorm, halvings, fchi2, fweight, true);
	const int rc = gn_polish(ctx, maps, N, mono, x, iters, 0, 1.0, obj, gnorm, halvings, nullptr, nullptr, false);
	size_t FI = 0;
	for (int k = 0; k < N; k++) FI += maps[k].n;
	if (fchi2)
	{
		map_feature_chi2(ctx, maps, N, mono, x, fchi2, nullptr);
	}
	if (fweight) std::fill(fweight, fweight + FI, 1.0);
	return rc;
}

// The joint system of the N local maps linearised at x, as a map like any other (C ABI: lsfm_gn_linearise).  One assembly at x with the
// maps' weights, then every block of UJ / WJ summed once into its place (k_gn_coalesce_u / _w), then the download into arrays of the
// library's own allocator (lsfm_map_release frees them).  x is read only.  The assembly sums with atomics: two calls agree to rounding,
// not bit for bit; the structure of `out` depends on the labels alone.
// times (may be null): [3] HIP-event ms of the assembly, k_gn_coalesce_w, k_gn_coalesce_u; counts (may be null): [4] NWJ, nW', NUJ, nU'.
int gn_linearise(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, const double* weight, lsfm_map* out, double* obj,
                 double* b, double* times, int* counts)
{
	hipStream_t s = ctx->stream;
	// LSFM_GN_TIMING=1: wall clock of the call's parts on stderr, as lsfm_gn_polish
	static const bool timing = getenv("LSFM_GN_TIMING") != nullptr;
	auto wall = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double tw0 = wall();
	GnCall c;
	GnCoalesce co;
	gn_setup(ctx, maps, N, mono, x, c, weight, &co);
	const int M = c.M, NFG = c.NFG;
	if (timing) LSFM_CHECK_HIP(hipStreamSynchronize(s));
	const double tw1 = wall();
	hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }; // around the assembly and the two coalescing launches
	if (times) for (hipEvent_t& e : ev) e = ctx->pool_event();
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	gn_assemble(ctx, c, 0, 1.0, nullptr);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	if (co.nWo) hipLaunchKernelGGL(k_gn_coalesce_w, grid_for(co.nWo, 256), dim3(256), 0, s, co.nWo, co.d_wsp, co.d_wsi, c.WJ, co.Wo);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
	if (co.nUo) hipLaunchKernelGGL(k_gn_coalesce_u, grid_for(co.nUo, 256), dim3(256), 0, s, co.nUo, co.d_usp, co.d_usi, c.UJ, co.Uo);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[3], s));
	if (timing) LSFM_CHECK_HIP(hipStreamSynchronize(s));
	const double tw2 = wall();
	lsfm_map g;
	memset(&g, 0, sizeof g);
	g.m = M; g.n = NFG; g.nU = co.nUo; g.nW = co.nWo;
	g.Ref = x->Ref; g.FRef = x->FRef; g.ScaP = x->ScaP; g.Fix = x->Fix; g.Sign = x->Sign; g.FScaP = x->FScaP; g.FFix = x->FFix;
	g.stno = host_alloc<int>(c.RS); g.stVal = host_alloc<double>(c.RS);
	g.U = host_alloc<double>((size_t)g.nU * 36); g.Ui = host_alloc<int>(g.nU); g.Uj = host_alloc<int>(g.nU);
	g.W = host_alloc<double>((size_t)g.nW * 18); g.photo = host_alloc<int>(g.nW); g.feature = host_alloc<int>(g.nW);
	g.V = host_alloc<double>((size_t)NFG * 9); g.FBlock = host_alloc<int>(NFG);
	g.pose_origin = host_alloc<int>(M);
	if (!g.stno || !g.stVal || !g.U || !g.Ui || !g.Uj || !g.W || !g.photo || !g.feature || !g.V || !g.FBlock || !g.pose_origin)
	{
		lsfm_map_release(&g);
		LSFM_FAIL(LSFM_ERR_OOM, "gn linearise: out of host memory for the map");
	}
	try
	{
		std::copy(x->stno, x->stno + c.RS, g.stno); std::copy(x->stVal, x->stVal + c.RS, g.stVal);
		std::copy(co.Ui.begin(), co.Ui.end(), g.Ui); std::copy(co.Uj.begin(), co.Uj.end(), g.Uj);
		std::copy(co.photo.begin(), co.photo.end(), g.photo); std::copy(co.feature.begin(), co.feature.end(), g.feature);
		std::copy(co.FBlock.begin(), co.FBlock.end(), g.FBlock); std::copy(co.origin.begin(), co.origin.end(), g.pose_origin);
		if (g.nU) d2h(ctx, g.U, co.Uo, (size_t)g.nU * 36 * sizeof(double));
		if (g.nW) d2h(ctx, g.W, co.Wo, (size_t)g.nW * 18 * sizeof(double));
		if (NFG) d2h(ctx, g.V, c.VJ, (size_t)NFG * 9 * sizeof(double));
		if (obj) d2h(ctx, obj, c.Fsum, sizeof(double));
		if (b)
		{
			d2h(ctx, b, c.ea, (size_t)M * 6 * sizeof(double));
			if (NFG) d2h(ctx, b + (size_t)M * 6, c.eb, (size_t)NFG * 3 * sizeof(double));
		}
		LSFM_CHECK_HIP(hipStreamSynchronize(s));
		if (times)
		{
			float ms[3] = { 0.0f, 0.0f, 0.0f };
			for (int i = 0; i < 3; i++) LSFM_CHECK_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
			for (int i = 0; i < 3; i++) times[i] = ms[i];
		}
	}
	catch (...)
	{
		lsfm_map_release(&g);
		throw;
	}
	if (counts) { counts[0] = c.NWJ; counts[1] = co.nWo; counts[2] = c.NUJ; counts[3] = co.nUo; }
	if (timing)
		fprintf(stderr, "lsfm_gn_linearise: %d maps, %d poses, %d features, W %d -> %d blocks, U %d -> %d blocks; structure + upload %.2f ms, assembly + coalescing "
		                "%.2f ms, download %.2f ms, call %.2f ms\n", N, M, NFG, c.NWJ, co.nWo, c.NUJ, co.nUo, tw1 - tw0, tw2 - tw1, wall() - tw2, wall() - tw0);
	*out = g;
	return LSFM_OK;
}

} // namespace lsfm
