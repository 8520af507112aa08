// Merging feature pairs of a joined map (C ABI: lsfm_map_merge_features).  No reference counterpart.
//
// Declaring x_f = x_g for the K pairs is a linear constraint x = T y on the Gaussian (x^, I = [U W; W^T V]).  The constrained map is
//     I' = T^T I T:   U' = U,   V'_c = sum_{h in c} V_h,   W'_{p,c} = sum_{h in c} W_{p,h}           (V is block diagonal: again a map)
//     y^ = y0 + I'^-1 eta,   eta = T^T I r,   r = x^ - T y0          y0 = x^ with every class at its representative's estimate
// r is non-zero only at the merged-away features g (r_g = x^_g - x^_rep), so eta_p = sum_g W_{p,g} r_g and eta_c = sum_g V_g r_g.
// delta = I'^-1 eta by the Schur route on the merged map:
//     B = eta_p - sum_c W'_c V'_c^-1 eta_c;   delta_p = S'^-1 B  (ONE right-hand side: cc_solve_refine, R = 1);
//     delta_c = V'_c^-1 (eta_c - sum_b W'_{b,c}^T delta_{p_b})
// and the joint compatibility of all pairs is D^2 = sum_g r_g^T V_g r_g - eta^T delta, 3 (n - n') degrees of freedom.
//
// Pipeline (structure: lsfm_merge_structure.cpp, host, index arrays and pairs alone):
//   k_gn_coalesce<18>      W': one lane per output block, its sources summed in registers in the structure's order, stored once
//   k_merge_features       one lane per output feature: V' (members ascending; a class of one: a copy), the representative's label and
//                          estimate, eta_c and sum_g r_g^T V_g r_g of a larger class
//   -- the merged map goes through the host here (map_alloc / MapOut, lsfm_map.hpp): cov_front_rowsorted uploads it, reduces it and factors S' --
//   k_merge_rhs            one work-group per class of more than one member and one COLUMN of two slabs per class (k_fc_rhs's shape): the
//                          class's part of eta_p from the W runs of its merged-away members, and W'_c V'_c^-1 eta_c from its merged run
//   k_merge_rowsum         a lane per pose scalar sums the columns in ascending order: eta_p and B.  No atomics: the same bits every time
//   cc_solve_refine        R = 1: the sweeps' launch shapes round one column up to a wave; the other lanes are off (r < R), so no zero
//                          column is padded in and the stopping rule sees the one column alone
//   k_merge_backsub        one lane per output feature: delta_c, y^_c and eta_c . delta_c
//   k_merge_pose           y^_p = x^_p + delta_p (a gauge scalar: x^_p itself) and eta_p delta_p per scalar
//   k_merge_d2             one work-group: strided partial sums and a tree in LDS, a fixed order
// Bit-reproducible: the structure, U' V' W', eta, B, and D^2 given delta_p.  Not: delta_p (the sweeps add with atomics), and so y^.
#include <algorithm>
#include <cstring>
#include <vector>

#include "lsfm_coalesce.hpp"
#include "lsfm_cov.hpp"
#include "lsfm_device.hpp"
#include "lsfm_internal.hpp"
#include "lsfm_merge_structure.hpp"
#include "lsfm_system.hpp"

namespace lsfm {

namespace {

#define MG_COLS 192 /* classes per launch of k_merge_rhs: the columns of the two slabs [6 M][MG_COLS] */
#define MG_RED 256  /* lanes of k_merge_d2 */

__global__ void __launch_bounds__(256)
k_merge_features(int no, const int* __restrict__ cptr, const int* __restrict__ cmem, const double* __restrict__ V, const double* __restrict__ feat,
                 const int* __restrict__ label, double* __restrict__ oV, double* __restrict__ ofeat, int* __restrict__ olabel, double* __restrict__ eta,
                 double* __restrict__ quad)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= no) return;
	const int m0 = cptr[c], m1 = cptr[c + 1];
	const int rep = cmem[m0];
	double v[9], x[3], e[3] = { 0.0, 0.0, 0.0 }, t = 0.0;
	ld<9>(v, V + (size_t)rep * 9);
	ld<3>(x, feat + (size_t)rep * 3);
	for (int k = m0 + 1; k < m1; k++)
	{
		const int g = cmem[k];
		double vg[9], r[3];
		ld<9>(vg, V + (size_t)g * 9);
#pragma unroll
		for (int i = 0; i < 3; i++) r[i] = feat[(size_t)g * 3 + i] - x[i];
#pragma unroll
		for (int i = 0; i < 3; i++)
		{
			const double vr = vg[3 * i] * r[0] + vg[3 * i + 1] * r[1] + vg[3 * i + 2] * r[2];
			e[i] += vr;
			t += r[i] * vr;
		}
#pragma unroll
		for (int i = 0; i < 9; i++) v[i] += vg[i];
	}
	st<9>(oV + (size_t)c * 9, v);
	st<3>(ofeat + (size_t)c * 3, x);
	st<3>(eta + (size_t)c * 3, e);
	quad[c] = t;
#pragma unroll
	for (int i = 0; i < 3; i++) olabel[(size_t)c * 3 + i] = label[(size_t)rep * 3 + i];
}

// Class bigs[k0 + blockIdx.x] into column blockIdx.x of the ZEROED slabs E and T [6 M][cols]: lane q < 6 owns scalar row q of every pose.
// E: the merged-away members' runs (aW / aphoto, member a's blocks awptr[a] .. awptr[a + 1], its r at ar + 3 a), walked in order;
// T: the class's merged run.  A class owns its column, and a row met twice is met by the same lane one after the other.
// The six lanes walk ALL blocks of a class one after the other (a read-modify-write of global memory per block), so the time of a
// launch is linear in the block count of its largest class: right for what a gate accepts -- classes of a few features, each seen by
// a few poses --, and the wrong shape for one huge class ("every feature one point" on a large map runs the whole of W through one
// wave: correct, and as slow as that sounds).
__global__ void __launch_bounds__(LSFM_WAVE)
k_merge_rhs(int k0, int cols, const int* __restrict__ bigs, const int* __restrict__ aptr, const int* __restrict__ awptr, const int* __restrict__ aphoto,
            const double* __restrict__ aW, const double* __restrict__ ar, const int* __restrict__ fptr, const int* __restrict__ photo,
            const double* __restrict__ W, const double* __restrict__ IV, const double* __restrict__ eta, const unsigned char* __restrict__ fixed,
            double* __restrict__ E, double* __restrict__ T)
{
	const int q = threadIdx.x;
	if (q >= 6) return;
	const int col = blockIdx.x, k = k0 + col, c = bigs[k];
	for (int a = aptr[k]; a < aptr[k + 1]; a++)
	{
		const double r0 = ar[(size_t)a * 3], r1 = ar[(size_t)a * 3 + 1], r2 = ar[(size_t)a * 3 + 2];
		for (int w = awptr[a]; w < awptr[a + 1]; w++)
		{
			const size_t row = (size_t)aphoto[w] * 6 + q;
			if (fixed && fixed[row]) continue;
			const double* wb = aW + (size_t)w * 18 + q * 3;
			E[row * cols + col] += wb[0] * r0 + wb[1] * r1 + wb[2] * r2;
		}
	}
	const double* iv = IV + (size_t)c * 9;
	const double e0 = eta[(size_t)c * 3], e1 = eta[(size_t)c * 3 + 1], e2 = eta[(size_t)c * 3 + 2];
	const double z0 = iv[0] * e0 + iv[1] * e1 + iv[2] * e2, z1 = iv[3] * e0 + iv[4] * e1 + iv[5] * e2, z2 = iv[6] * e0 + iv[7] * e1 + iv[8] * e2;
	for (int w = fptr[c]; w < fptr[c + 1]; w++)
	{
		const size_t row = (size_t)photo[w] * 6 + q;
		if (fixed && fixed[row]) continue;
		const double* wb = W + (size_t)w * 18 + q * 3;
		T[row * cols + col] += wb[0] * z0 + wb[1] * z1 + wb[2] * z2;
	}
}

// etaP[row] += sum_col E,  B[row] += sum_col E - sum_col T, the columns in ascending order (etaP and B zeroed before the first launch)
__global__ void __launch_bounds__(256)
k_merge_rowsum(int rows, int cols, const double* __restrict__ E, const double* __restrict__ T, double* __restrict__ etaP, double* __restrict__ B)
{
	const int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= rows) return;
	double se = 0.0, st_ = 0.0;
	for (int c = 0; c < cols; c++) { se += E[(size_t)row * cols + c]; st_ += T[(size_t)row * cols + c]; }
	etaP[row] += se;
	B[row] += se - st_;
}

// delta_c = V'_c^-1 (eta_c - sum_b W'_bc^T delta_p[p_b]),  y^_c = y0_c + delta_c,  dot[c] = eta_c . delta_c   (X = delta_p, [6 M][1])
__global__ void __launch_bounds__(256)
k_merge_backsub(int no, const int* __restrict__ fptr, const int* __restrict__ photo, const double* __restrict__ W, const double* __restrict__ IV,
                const double* __restrict__ eta, const double* __restrict__ X, const double* __restrict__ y0, double* __restrict__ y, double* __restrict__ dot)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= no) return;
	double t[3] = { 0.0, 0.0, 0.0 };
	for (int w = fptr[c]; w < fptr[c + 1]; w++)
	{
		const double* wb = W + (size_t)w * 18;
		const double* x = X + (size_t)photo[w] * 6;
#pragma unroll
		for (int q = 0; q < 6; q++)
#pragma unroll
			for (int j = 0; j < 3; j++) t[j] = fma(wb[q * 3 + j], x[q], t[j]);
	}
	const double* iv = IV + (size_t)c * 9;
	double e[3], s = 0.0;
#pragma unroll
	for (int i = 0; i < 3; i++) e[i] = eta[(size_t)c * 3 + i] - t[i];
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
		const double d = iv[3 * i] * e[0] + iv[3 * i + 1] * e[1] + iv[3 * i + 2] * e[2];
		y[(size_t)c * 3 + i] = y0[(size_t)c * 3 + i] + d;
		s += eta[(size_t)c * 3 + i] * d;
	}
	dot[c] = s;
}

__global__ void __launch_bounds__(256)
k_merge_pose(int rows, const double* __restrict__ x, const double* __restrict__ X, const double* __restrict__ etaP, const unsigned char* __restrict__ fixed,
             double* __restrict__ y, double* __restrict__ dot)
{
	const int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= rows) return;
	const bool fx = fixed && fixed[row];
	y[row] = fx ? x[row] : x[row] + X[row];
	dot[row] = fx ? 0.0 : etaP[row] * X[row];
}

// out = { D^2, sum quad, eta^T delta }: lane l sums the entries l, l + MG_RED, ... of each array, the lanes' sums meet in a tree
__global__ void __launch_bounds__(MG_RED)
k_merge_d2(int no, const double* __restrict__ quad, const double* __restrict__ fdot, int rows, const double* __restrict__ pdot, double* __restrict__ out)
{
	__shared__ double sq[MG_RED], sd[MG_RED];
	const int l = threadIdx.x;
	double q = 0.0, d = 0.0;
	for (int i = l; i < no; i += MG_RED) { q += quad[i]; d += fdot[i]; }
	for (int i = l; i < rows; i += MG_RED) d += pdot[i];
	sq[l] = q; sd[l] = d;
	__syncthreads();
	for (int h = MG_RED / 2; h > 0; h >>= 1)
	{
		if (l < h) { sq[l] += sq[l + h]; sd[l] += sd[l + h]; }
		__syncthreads();
	}
	if (l == 0) { out[0] = sq[0] - sd[0]; out[1] = sq[0]; out[2] = sd[0]; }
}

inline dim3 grid(size_t n) { return dim3((unsigned)((std::max<size_t>(n, 1) + 255) / 256)); }

template <class T> T* put(lsfm_context* ctx, DevBuf& b, const T* src, size_t count)
{
	T* d = b.get<T>(count);
	h2d(ctx, d, src, count * sizeof(T));
	return d;
}

} // namespace

int map_merge_features(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* pairs, int K, lsfm_map* out, double* d2, int* dof, int* rep,
                       int* steps_out, double* last_corr, double* times)
{
	if (steps_out) *steps_out = 0;
	const int m = map->m, n = map->n, nW = map->nW;
	if (!map->stno || !map->stVal) LSFM_FAIL(LSFM_ERR_ARG, "the map has no labels or no estimates");
	// ---- arguments and structure (host) ----
	const std::vector<int> fptr = system_fptr(host_system_of(*map, true));
	if ((map->nU && !map->U) || (nW && !map->W) || (n && !map->V)) LSFM_FAIL(LSFM_ERR_ARG, "null value array");
	MergeStructure st;
	{
		std::string why;
		if (merge_structure(n, fptr, map->photo, pairs, K, st, why) != LSFM_OK) LSFM_FAIL(LSFM_ERR_ARG, why);
	}
	const int no = st.no, nWo = st.nWo, big = st.big;
	const double* xf = map->stVal + (size_t)6 * m;
	// the merged-away members of the larger classes, class by class: their r and their W runs back to back
	std::vector<int> aptr((size_t)big + 1, 0), awptr(1, 0), aphoto;
	std::vector<double> ar, aW;
	for (int k = 0; k < big; k++)
	{
		const int c = st.bigs[k], r0 = st.cmem[st.cptr[c]];
		for (int i = st.cptr[c] + 1; i < st.cptr[c + 1]; i++)
		{
			const int g = st.cmem[i];
			for (int j = 0; j < 3; j++) ar.push_back(xf[(size_t)3 * g + j] - xf[(size_t)3 * r0 + j]);
			aphoto.insert(aphoto.end(), map->photo + fptr[g], map->photo + fptr[g + 1]);
			aW.insert(aW.end(), map->W + (size_t)18 * fptr[g], map->W + (size_t)18 * fptr[g + 1]);
			awptr.push_back((int)aphoto.size());
		}
		aptr[k + 1] = (int)awptr.size() - 1;
	}
	hipStream_t s = ctx->stream;
	hipEvent_t ev[5]; // start | merged map on the host | solved | D^2 | downloaded
	for (int k = 0; k < 5; k++) ev[k] = ctx->pool_event();
	LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	// ---- upload; W' and V' ----
	DevBuf bW, bV, bX, bL, bSp, bSi, bCp, bCm, bOW, bOV, bOX, bOL, bEta, bQ;
	const double* dW = put(ctx, bW, map->W, (size_t)nW * 18);
	const double* dV = put(ctx, bV, map->V, (size_t)n * 9);
	const double* dX = put(ctx, bX, xf, (size_t)n * 3);
	const int* dL = put(ctx, bL, map->stno + (size_t)6 * m, (size_t)n * 3);
	const int* dsp = put(ctx, bSp, st.sptr.data(), st.sptr.size());
	const int* dsi = put(ctx, bSi, st.sidx.data(), st.sidx.size());
	const int* dcp = put(ctx, bCp, st.cptr.data(), st.cptr.size());
	const int* dcm = put(ctx, bCm, st.cmem.data(), st.cmem.size());
	double* oW = bOW.get<double>((size_t)nWo * 18);
	double* oV = bOV.get<double>((size_t)no * 9);
	double* oX = bOX.get<double>((size_t)no * 3);
	int* oL = bOL.get<int>((size_t)no * 3);
	double* eta = bEta.get<double>((size_t)no * 3);
	double* quad = bQ.get<double>(no);
	if (nWo) hipLaunchKernelGGL(k_gn_coalesce<18>, grid(nWo), dim3(256), 0, s, nWo, dsp, dsi, dW, oW);
	if (no) hipLaunchKernelGGL(k_merge_features, grid(no), dim3(256), 0, s, no, dcp, dcm, dV, dX, dL, oV, oX, oL, eta, quad);
	LSFM_CHECK_HIP(hipGetLastError());
	// ---- the merged map (library-allocated), at y0 for now: this version hands it to cov_front through the host ----
	MapOut G;
	map_new(G.g, map, m, no, map->nU, nWo, map->pose_origin != nullptr);
	lsfm_map& g = G.g;
	if (map->pose_origin) memcpy(g.pose_origin, map->pose_origin, (size_t)m * sizeof(int));
	memcpy(g.stno, map->stno, (size_t)6 * m * sizeof(int));
	memcpy(g.stVal, map->stVal, (size_t)6 * m * sizeof(double));
	memcpy(g.U, map->U, (size_t)map->nU * 36 * sizeof(double));
	memcpy(g.Ui, map->Ui, (size_t)map->nU * sizeof(int));
	memcpy(g.Uj, map->Uj, (size_t)map->nU * sizeof(int));
	memcpy(g.photo, st.photo.data(), (size_t)nWo * sizeof(int));
	memcpy(g.feature, st.feature.data(), (size_t)nWo * sizeof(int));
	memcpy(g.FBlock, st.FBlock.data(), (size_t)no * sizeof(int));
	d2h(ctx, g.W, oW, (size_t)nWo * 18 * sizeof(double));
	d2h(ctx, g.V, oV, (size_t)no * 9 * sizeof(double));
	d2h(ctx, g.stVal + (size_t)6 * m, oX, (size_t)no * 3 * sizeof(double));
	d2h(ctx, g.stno + (size_t)6 * m, oL, (size_t)no * 3 * sizeof(int));
	LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	LSFM_CHECK_HIP(hipStreamSynchronize(s)); // (the staged copies have left the host vectors before cov_front reuses the ring)
	// ---- factor S' ----
	CovFront fr;
	const int floored = cov_front_rowsorted(ctx, &g, mono, fr);
	if (floored > 0) return floored; // the factor is of a perturbed S': nothing is written, the staged map is released
	const SolveIO& io = fr.io;
	const int rows = 6 * m;
	// ---- the right-hand side ----
	DevBuf bBg, bAp, bAwp, bAph, bAW, bAr, bE, bT, bEp, bB, bXp, bYp, bYf, bPd, bFd, bD;
	const int* dbigs = put(ctx, bBg, st.bigs.data(), (size_t)big);
	const int* daptr = put(ctx, bAp, aptr.data(), aptr.size());
	const int* dawptr = put(ctx, bAwp, awptr.data(), awptr.size());
	const int* daphoto = put(ctx, bAph, aphoto.data(), aphoto.size());
	const double* daW = put(ctx, bAW, aW.data(), aW.size());
	const double* dar = put(ctx, bAr, ar.data(), ar.size());
	const int cols = std::min(big, MG_COLS);
	double* E = bE.get<double>((size_t)rows * cols);
	double* T = bT.get<double>((size_t)rows * cols);
	double* etaP = bEp.get<double>(rows);
	double* B = bB.get<double>(rows);
	const double* dxp = put(ctx, bXp, map->stVal, (size_t)rows);
	double* yp = bYp.get<double>(rows);
	double* yf = bYf.get<double>((size_t)no * 3);
	double* pdot = bPd.get<double>(rows);
	double* fdot = bFd.get<double>(no);
	double* dd = bD.get<double>(3);
	dev_zero(ctx, etaP, (size_t)rows * sizeof(double));
	dev_zero(ctx, B, (size_t)rows * sizeof(double));
	for (int k0 = 0; k0 < big; k0 += cols)
	{
		const int kc = std::min(cols, big - k0);
		dev_zero(ctx, E, (size_t)rows * kc * sizeof(double));
		dev_zero(ctx, T, (size_t)rows * kc * sizeof(double));
		hipLaunchKernelGGL(k_merge_rhs, dim3(kc), dim3(LSFM_WAVE), 0, s, k0, kc, dbigs, daptr, dawptr, daphoto, daW, dar, io.fptr, io.photo, io.W, fr.sy.IV, eta,
		                   io.d_fixed, E, T);
		hipLaunchKernelGGL(k_merge_rowsum, grid(rows), dim3(256), 0, s, rows, kc, E, T, etaP, B);
	}
	// ---- delta_p = S'^-1 B ----
	CcWork wk;
	wk.alloc(fr.ch.M, 1);
	const CcOutcome oc = cc_solve_refine(ctx, fr, 1, wk, [&](double* dst) {
		LSFM_CHECK_HIP(hipMemcpyAsync(dst, B, (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, s));
	});
	LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
	// ---- back-substitution and D^2 ----
	if (no) hipLaunchKernelGGL(k_merge_backsub, grid(no), dim3(256), 0, s, no, io.fptr, io.photo, io.W, fr.sy.IV, eta, wk.Xo, oX, yf, fdot);
	hipLaunchKernelGGL(k_merge_pose, grid(rows), dim3(256), 0, s, rows, dxp, wk.Xo, etaP, io.d_fixed, yp, pdot);
	hipLaunchKernelGGL(k_merge_d2, dim3(1), dim3(MG_RED), 0, s, no, quad, fdot, rows, pdot, dd);
	LSFM_CHECK_HIP(hipEventRecord(ev[3], s));
	LSFM_CHECK_HIP(hipGetLastError());
	double hd[3] = { 0.0, 0.0, 0.0 };
	d2h(ctx, g.stVal, yp, (size_t)rows * sizeof(double));
	d2h(ctx, g.stVal + (size_t)rows, yf, (size_t)no * 3 * sizeof(double));
	d2h(ctx, hd, dd, sizeof hd);
	LSFM_CHECK_HIP(hipEventRecord(ev[4], s));
	LSFM_CHECK_HIP(hipEventSynchronize(ev[4]));
	if (times)
	{
		times[0] = event_ms(ev[0], ev[1]);
		times[1] = event_ms(ev[1], fr.ev[2]);
		times[2] = event_ms(fr.ev[2], ev[2]);
		times[3] = event_ms(ev[2], ev[3]);
		times[4] = event_ms(ev[3], ev[4]);
	}
	if (d2) *d2 = hd[0];
	if (dof) *dof = 3 * st.removed;
	if (rep) memcpy(rep, st.rep.data(), (size_t)n * sizeof(int));
	if (steps_out) *steps_out = oc.steps;
	if (last_corr) last_corr[0] = wk.ratio[0];
	G.give(out);
	return oc.undone ? LSFM_NOT_CONVERGED : LSFM_OK;
}

} // namespace lsfm
