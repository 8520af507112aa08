// Gauss-Newton polish of the map-joining objective (lsfm_gn.hpp; the objective and a step's kernels: lsfm_gn_assemble.hip): a call's way onto
// the device (gn_begin), the polish loop, and the calls that read one state -- lsfm_map_chi2, lsfm_map_feature_chi2, lsfm_gn_linearise.
// A call begins with the batch's upload, gn_structure (host, labels alone: lsfm_gn_structure.cpp) and gn_upload (the structure's arrays);
// then gn_assemble / solve_batch per step.
#include <algorithm>
#include <chrono>

#include "lsfm_coalesce.hpp"
#include "lsfm_device.hpp"
#include "lsfm_gn.hpp"

namespace lsfm {


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
template <class T>
T* gn_put(lsfm_context* ctx, Arena& ar, const std::vector<T>& v)
{
	T* d = ar.alloc<T>(v.size());
	h2d(ctx, d, v.data(), v.size() * sizeof(T));
	return d;
}

// what ensure_arenas is asked for on behalf of a call
size_t gn_arena_need(const lsfm_map* maps, int N, const lsfm_map* x, const GnWants& w)
{
	size_t need = (size_t)128 << 20, P = 0, FI = 0, nW = 0, nU = 0;
	for (int k = 0; k < N; k++) { P += maps[k].m; FI += maps[k].n; nW += maps[k].nW; nU += maps[k].nU; }
	need += ((nW + 2 * FI) * 400 + (nU + 3 * P + 3 * (size_t)N) * 800 + (FI + std::max(x->n, 0)) * 500 + (P + std::max(x->m, 0)) * 6000) * 2 + (size_t)N * 64;
	// (the coalesced blocks and their source lists: at most one output block and one source per joint block)
	if (w.coalesce) need += (nW + 2 * FI) * (144 + 16) + (nU + 2 * P + 3 * (size_t)N) * (288 + 16) + 1024;
	if (w.feat)
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
		if (w.slots) need += (nU + nc) * (288 + 800 + 8 + 288) + nc * (16 + 36) + nW * 8;
		// (every slot is one more joint U block: one more source of the coalesced form and at most one more output block)
		if (w.slots && w.coalesce) need += nc * (288 + 16);
	}
	return need;
}

// the per-feature arrays of the feature chi^2 pass
void gn_upload_features(lsfm_context* ctx, Arena& ar, const GnStructure& st, GnFeat& fr)
{
	fr.d_bad = gn_put(ctx, ar, std::vector<int>(1, INT32_MAX));
	fr.fchi2 = ar.alloc<double>(st.FI); fr.fw = ar.alloc<double>(st.FI); fr.msum = ar.alloc<double>((size_t)3 * st.N); fr.pose_chi2 = ar.alloc<double>(st.N);
}
// the extended U list: every map's own blocks (copied once: k_gn_extend_u), then its slots (k_gn_feature_ufill, every assembly)
void gn_upload_slots(lsfm_context* ctx, Arena& ar, const GnStructure& st, GnCall& c)
{
	const GnSlots& sl = st.sl;
	GnFeat& fr = c.feat;
	const int NUX = (int)sl.Uix.size();
	fr.NS = (int)sl.a.size(); fr.NC = sl.cf.size();
	fr.Ux = ar.alloc<double>((size_t)NUX * 36);
	const int *d_Uix = gn_put(ctx, ar, sl.Uix), *d_Ujx = gn_put(ctx, ar, sl.Ujx), *d_ushift = gn_put(ctx, ar, sl.ushift);
	fr.d_sptr = gn_put(ctx, ar, sl.sptr); fr.d_cf = gn_put(ctx, ar, sl.cf); fr.d_ca = gn_put(ctx, ar, sl.ca); fr.d_cb = gn_put(ctx, ar, sl.cb);
	fr.d_eptr = gn_put(ctx, ar, sl.eptr); fr.d_eidx = gn_put(ctx, ar, sl.eidx); fr.d_sdst = gn_put(ctx, ar, sl.sdst);
	dev_zero(ctx, fr.Ux, (size_t)NUX * 36 * sizeof(double));
	gn_extend_u(ctx, c, d_ushift);
	c.u = GnUView{ fr.Ux, d_Uix, d_Ujx, NUX };
}
// lsfm_gn_linearise: the sources of the output blocks, and the blocks
void gn_upload_coalesce(lsfm_context* ctx, Arena& ar, const GnCoalesced& co, GnCoalesceDev& d)
{
	d.d_wsp = gn_put(ctx, ar, co.wsp); d.d_wsi = gn_put(ctx, ar, co.wsi); d.d_usp = gn_put(ctx, ar, co.usp); d.d_usi = gn_put(ctx, ar, co.usi);
	d.Wo = ar.alloc<double>((size_t)co.nWo * 18); d.Uo = ar.alloc<double>((size_t)co.nUo * 36);
}

// The structure's arrays and the state x (to d_x) onto the device, behind the uploaded batch; the work arrays.  weight (may be null: all
// 1): the maps' weights w_k.  The per-feature arrays where w.feat; the extended U list and the coalescing arrays where st holds them.
void gn_upload(lsfm_context* ctx, const lsfm_map* x, const double* weight, const GnStructure& st, const GnWants& w, GnCall& c)
{
	const int N = c.N = st.N, M = c.M = st.M, NFG = c.NFG = st.NFG, P = c.P = st.P, FI = c.FI = st.FI, NUJ = c.NUJ = st.NUJ, NWJ = c.NWJ = st.NWJ;
	const bool mono = c.mono = st.mono;
	Arena& ar = ctx->arena[0];
	const DevBatch& X = c.X;
	if (X.pose_off != st.pose_off || X.feat_off != st.feat_off || X.u_off != st.u_off || X.w_off != st.w_off)
		LSFM_FAIL(LSFM_ERR_INTERNAL, "gn polish: the structure's offsets are not the uploaded batch's");
	c.u = GnUView{ X.U, X.Ui, X.Uj, X.NU };
	std::vector<GnMap> gm(N);
	for (int k = 0; k < N; k++)
	{
		memset(&gm[k], 0, sizeof(GnMap));
		static_cast<GnMapShape&>(gm[k]) = st.map[k];
		gm[k].w = weight ? weight[k] : 1.0;
	}
	const size_t RS = c.RS = (size_t)M * 6 + (size_t)NFG * 3;
	c.d_gm = gn_put(ctx, ar, gm);
	c.d_gp = gn_put(ctx, ar, st.gp); c.d_gf = gn_put(ctx, ar, st.gf); c.d_wdst = gn_put(ctx, ar, st.wdst);
	c.d_fptrJ = gn_put(ctx, ar, st.fptrJ); c.d_photoJ = gn_put(ctx, ar, st.photoJ);
	c.d_fsp = gn_put(ctx, ar, st.fsp); c.d_fsi = gn_put(ctx, ar, st.fsi); c.d_psp = gn_put(ctx, ar, st.psp); c.d_psi = gn_put(ctx, ar, st.psi);
	c.d_UiJ = gn_put(ctx, ar, st.UiJ); c.d_UjJ = gn_put(ctx, ar, st.UjJ); c.d_org = gn_put(ctx, ar, st.origin);
	c.d_seg = ar.alloc<int>(M + NFG + 1);
	c.d_fixed = mono ? gn_put(ctx, ar, st.fixed) : nullptr;
	c.d_x = ar.alloc<double>(RS); c.d_x0 = ar.alloc<double>(RS); c.d_dl = ar.alloc<double>(RS);
	c.Dp = ar.alloc<double>((size_t)P * 36); c.Cp = ar.alloc<double>((size_t)P * 72); c.rp = ar.alloc<double>((size_t)P * 6);
	c.Gacc = ar.alloc<double>((size_t)P * GN_GW + (size_t)N * GN_HW + 2); c.Hacc = c.Gacc + (size_t)P * GN_GW; c.Fsum = c.Hacc + (size_t)N * GN_HW;
	c.ePinst = ar.alloc<double>((size_t)P * 6); c.Vinst = ar.alloc<double>((size_t)FI * 9); c.eFinst = ar.alloc<double>((size_t)FI * 3);
	c.UJ = ar.alloc<double>((size_t)NUJ * 36); c.WJ = ar.alloc<double>((size_t)NWJ * 18); c.VJ = ar.alloc<double>((size_t)NFG * 9);
	c.ea = ar.alloc<double>((size_t)M * 6); c.eb = ar.alloc<double>((size_t)NFG * 3);
	c.d_max = ar.alloc<unsigned long long>(2);
	c.d_dof = gn_put(ctx, ar, st.dof); c.d_chi2 = ar.alloc<double>(N); c.d_w = ar.alloc<double>(N); c.d_G = ar.alloc<double>(1);
	h2d(ctx, c.d_x, x->stVal, RS * sizeof(double));
	dev_zero(ctx, c.d_seg, (size_t)(M + NFG + 1) * sizeof(int));
	if (w.feat) gn_upload_features(ctx, ar, st, c.feat);
	if (st.has_slots) gn_upload_slots(ctx, ar, st, c);
	if (st.has_coalesced) gn_upload_coalesce(ctx, ar, st.co, c.co);
}

// A call's way onto the device: the arenas sized and reset, the local maps uploaded (batch_upload: it checks their index arrays), the
// structure derived from the labels (its refusals as an Error, LSFM_ERR_ARG, with its message), then gn_upload
void gn_begin(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, const double* weight, const GnWants& w, GnStructure& st, GnCall& c)
{
	ctx->ensure_arenas(gn_arena_need(maps, N, x, w));
	ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->scratch.reset();
	batch_upload(ctx, ctx->arena[0], maps, N, mono, c.X);
	std::string why;
	if (gn_structure(maps, N, mono, x, w.slots, w.coalesce, st, why) != LSFM_OK) LSFM_FAIL(LSFM_ERR_ARG, why);
	gn_upload(ctx, x, weight, st, w, c);
}

// what k_gn_chi2<true> found: throws LSFM_ERR_NOT_SPD naming the first feature whose V is not positive definite
void gn_feature_check(lsfm_context* ctx, const lsfm_map* maps, const GnCall& c)
{
	int bad = INT32_MAX;
	d2h(ctx, &bad, c.feat.d_bad, sizeof(int));
	if (bad == INT32_MAX) return;
	const int k = (int)(std::upper_bound(c.X.feat_off.begin(), c.X.feat_off.end(), bad) - c.X.feat_off.begin()) - 1, f = bad - c.X.feat_off[k];
	LSFM_FAIL(LSFM_ERR_NOT_SPD, "feature chi2: V of feature " + std::to_string(f + 1) + " (label " + std::to_string(maps[k].stno[6 * maps[k].m + 3 * f]) +
	                                ") of local map " + std::to_string(k + 1) + " is not positive definite");
}

inline double gn_wall() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// LSFM_GN_TIMING=1: wall clock of a call's parts on stderr (every part ends with a synchronisation of its own)
inline bool gn_timing() { static const bool on = getenv("LSFM_GN_TIMING") != nullptr; return on; }

// The polish under an estimator.  est.on == none: F, every weight 1, no chi^2 is formed during the steps.  maps: IRLS on
// s_k = chi2_k / dof_k -- every assembly forms chi2, the weights w_k = rho'(s_k) and G first, then the system with w_k I_k; chi2 / weight
// are [N].  features: G of lsfm_gn_polish_robust_features; chi2 / weight then are per local feature instance [sum n_k] and the maps keep
// weight 1.  obj / gnorm: [iters + 1]; halvings: [iters] or null; chi2 / weight may be null, at the returned state.  Returns LSFM_OK or
// LSFM_NOT_CONVERGED (a step's camera system was left above its residual bound); throws Error for invalid input.
int gn_run(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, const GnEstimator& est, double* obj, double* gnorm,
           int* halvings, double* chi2, double* weight)
{
	hipStream_t s = ctx->stream;
	const bool timing = gn_timing(), robust = est.on != GnEstimator::none, feat = est.on == GnEstimator::features;
	const double tw0 = gn_wall();
	double t_asm = 0.0, t_solve = 0.0, t_chi2 = 0.0, t_fill = 0.0;
	int n_asm = 0, n_solve = 0;
	GnStructure st;
	GnCall c;
	gn_begin(ctx, maps, N, mono, x, nullptr, feat ? GnWants::polish_features() : GnWants(), st, c);
	const int M = c.M, NFG = c.NFG;
	const size_t RS = c.RS;

	// F (robust: G) and the step's system at the state in d_x
	GnEvents ev;
	if (robust && timing) { ev.chi2[0] = ctx->pool_event(); ev.chi2[1] = ctx->pool_event(); }
	if (feat && timing) { ev.fill[0] = ctx->pool_event(); ev.fill[1] = ctx->pool_event(); }
	auto assemble = [&]() -> double {
		const double ta = gn_wall();
		gn_assemble(ctx, c, est, robust && timing ? &ev : nullptr);
		double F = 0.0;
		d2h(ctx, &F, robust ? c.d_G : c.Fsum, sizeof(double));
		if (feat && n_asm == 0) gn_feature_check(ctx, maps, c); // (V does not change during the call)
		if (robust && timing)
		{
			t_chi2 += event_ms(ev.chi2[0], ev.chi2[1]);
			if (feat) t_fill += event_ms(ev.fill[0], ev.fill[1]);
		}
		t_asm += gn_wall() - ta; n_asm++;
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
	const double tw1 = gn_wall();
	double F = assemble();
	for (int it = 0; it <= iters; it++)
	{
		obj[it] = F; gnorm[it] = grad_norm();
		if (it == iters) break;
		if (halvings) halvings[it] = 0;
		if (stopped) continue;
		if (!(F == F)) LSFM_FAIL(LSFM_ERR_INTERNAL, "gn polish: the objective is not a number");
		const size_t smark = ctx->scratch.mark();
		const double ts = gn_wall();
		const int rc = solve_batch(ctx, io).not_converged;
		LSFM_CHECK_HIP(hipStreamSynchronize(s));
		t_solve += gn_wall() - ts; n_solve++;
		ctx->scratch.release(smark);
		if (rc) ret = LSFM_NOT_CONVERGED;
		LSFM_CHECK_HIP(hipMemcpyAsync(c.d_x0, c.d_x, RS * sizeof(double), hipMemcpyDeviceToDevice, s));
		double alpha = 1.0, F1 = 0.0;
		int h = 0;
		for (; h <= 8; h++, alpha *= 0.5)
		{
			hipLaunchKernelGGL(k_gn_step, gn_grid(RS, 256), dim3(256), 0, s, RS, c.d_x0, c.d_dl, alpha, c.d_fixed, c.d_x);
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
		if (chi2 && c.FI) d2h(ctx, chi2, c.feat.fchi2, (size_t)c.FI * sizeof(double));
		if (weight && c.FI) d2h(ctx, weight, c.feat.fw, (size_t)c.FI * sizeof(double));
	}
	else
	{
		if (chi2)
		{
			if (!robust) gn_map_chi2(ctx, c);
			d2h(ctx, chi2, c.d_chi2, (size_t)N * sizeof(double));
		}
		if (weight)
		{
			if (robust) d2h(ctx, weight, c.d_w, (size_t)N * sizeof(double));
			else std::fill(weight, weight + N, 1.0);
		}
	}
	if (timing)
	{
		char fill[128] = "";
		if (feat) snprintf(fill, sizeof fill, ", U correction %.3f ms each: %d slots, %zu contributors", n_asm ? t_fill / n_asm : 0.0, c.feat.NS, c.feat.NC);
		fprintf(stderr, "lsfm_gn: %d maps, %d poses, %d features, joint system %d U / %d W blocks; structure + upload %.2f ms, %d assemblies %.2f ms each "
		                "(chi2 + weights %.3f ms each%s), %d solves %.2f ms each, call %.2f ms\n", N, M, NFG, c.NUJ, c.NWJ, tw1 - tw0, n_asm,
		        n_asm ? t_asm / n_asm : 0.0, n_asm ? t_chi2 / n_asm : 0.0, fill, n_solve, n_solve ? t_solve / n_solve : 0.0, gn_wall() - tw0);
	}
	return ret;
}
} // namespace

// x: the global state (stno / stVal / m / n, Ref; Mono: ScaP, Fix; optional pose_origin); stVal is updated in place.
// kind: 0 the plain polish, 1 Huber, 2 Cauchy on the maps with threshold c (gn_run)
int gn_polish(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, int kind, double cth, double* obj, double* gnorm,
              int* halvings, double* chi2, double* weight)
{
	const GnEstimator est{ kind != 0 ? GnEstimator::maps : GnEstimator::none, kind, cth };
	return gn_run(ctx, maps, N, mono, x, iters, est, obj, gnorm, halvings, chi2, weight);
}

// chi2_k of every local map at the global state x (x is read only); dof (may be null) = 6 m_k + 3 n_k
int map_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, double* chi2, int* dof)
{
	GnStructure st;
	GnCall c;
	gn_begin(ctx, maps, N, mono, x, nullptr, GnWants(), st, c);
	gn_frames(ctx, c);
	gn_map_chi2(ctx, c);
	d2h(ctx, chi2, c.d_chi2, (size_t)N * sizeof(double));
	if (dof) std::copy(st.dof.begin(), st.dof.end(), dof);
	return LSFM_OK;
}

// c_kf of every local feature instance at the global state x (x is read only), in map order and within a map in its feature order;
// pose_chi2 (may be null) [N] = chi2_k - sum_f c_kf.  No system is assembled: the per-feature arrays without the correction slots.
int map_feature_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, double* fchi2, double* pose_chi2)
{
	GnStructure st;
	GnCall c;
	gn_begin(ctx, maps, N, mono, x, nullptr, GnWants::feature_chi2(), st, c);
	gn_frames(ctx, c);
	gn_feature_chi2(ctx, c, 0, 1.0);
	gn_feature_check(ctx, maps, c);
	if (c.FI) d2h(ctx, fchi2, c.feat.fchi2, (size_t)c.FI * sizeof(double));
	if (pose_chi2) d2h(ctx, pose_chi2, c.feat.pose_chi2, (size_t)N * sizeof(double));
	return LSFM_OK;
}

// lsfm_gn_polish_robust_features: kind 0 is the plain polish with the feature chi2 of its result; fchi2 / fweight [sum n_k], may be null
int gn_polish_features(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, int kind, double cth, double* obj, double* gnorm,
                       int* halvings, double* fchi2, double* fweight)
{
	if (kind != 0) return gn_run(ctx, maps, N, mono, x, iters, GnEstimator{ GnEstimator::features, kind, cth }, obj, gnorm, halvings, fchi2, fweight);
	const int rc = gn_run(ctx, maps, N, mono, x, iters, GnEstimator(), obj, gnorm, halvings, nullptr, nullptr);
	size_t FI = 0;
	for (int k = 0; k < N; k++) FI += maps[k].n;
	if (fchi2) map_feature_chi2(ctx, maps, N, mono, x, fchi2, nullptr);
	if (fweight) std::fill(fweight, fweight + FI, 1.0);
	return rc;
}

// The joint system of the N local maps linearised at x, as a map like any other (C ABI: lsfm_gn_linearise).  One assembly at x with the
// maps' weights, then every block of UJ / WJ summed once into its place (UJ / WJ hold the solver's working form: entries with equal
// coordinates are repeated and add up; k_gn_coalesce<36> / <18>, lsfm_coalesce.hpp, sums the sources of an output block in map order -- the
// structure pass sorts stably; HBM-bound: NWJ * 144 B in, nW' * 144 B out, U: 288 B a block), then the download into arrays of the
// library's own allocator (lsfm_map_release frees them).  x is read only.  The assembly sums with atomics: two calls agree to rounding,
// not bit for bit; the structure of `out` depends on the labels alone.
// fweight (null: lsfm_gn_linearise, the launches above and no others; else lsfm_gn_linearise_features): [sum n_k] weights w_kf in [0, 1]
// of the features' conditional terms (the caller has checked them).  The maps are then I_k(w_k.) of lsfm_gn_chi2.hip: the structure
// carries the correction slots as well as the coalesced form, the assembly is the feature-robust step's with the weights given
// (GnEstimator::given: chi^2 pass, slot fill, k_gn_ublocks over the extended list, k_gn_features<NH, true>), a map's weight w_k reaches
// its slots as it reaches its own blocks (k_gn_ublocks scales every block of the list it reads), and the coalescing sums the slots'
// joint blocks with the others.  obj is then sum_k w_k (pose_chi2_k + sum_f w_kf c_kf), summed without atomics.
// times (may be null): [3] HIP-event ms of the assembly, k_gn_coalesce<18> (W), k_gn_coalesce<36> (U) -- with fweight [4]: the chi^2 pass
// + slot fill first, then the rest of the assembly and the two; counts (may be null): [4] NWJ, nW', NUJ, nU'.
int gn_linearise(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, const double* weight, const double* fweight,
                 lsfm_map* out, double* obj, double* b, double* times, int* counts)
{
	hipStream_t s = ctx->stream;
	const bool timing = gn_timing(), given = fweight != nullptr;
	const double tw0 = gn_wall();
	GnStructure st;
	GnCall c;
	gn_begin(ctx, maps, N, mono, x, weight, given ? GnWants::linearise_features() : GnWants::linearise(), st, c);
	const GnCoalesced& co = st.co;
	const int M = c.M, NFG = c.NFG;
	if (given && c.FI) h2d(ctx, c.feat.fw, fweight, (size_t)c.FI * sizeof(double));
	if (timing) LSFM_CHECK_HIP(hipStreamSynchronize(s));
	const double tw1 = gn_wall();
	hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }; // around the assembly and the two coalescing launches
	GnEvents gev;                                              // given: around the chi^2 pass and the slot fill inside the assembly
	if (times) for (hipEvent_t& e : ev) e = ctx->pool_event();
	if (times && given) { gev.chi2[0] = ctx->pool_event(); gev.chi2[1] = ctx->pool_event(); gev.fill[0] = ctx->pool_event(); gev.fill[1] = ctx->pool_event(); }
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[0], s));
	if (given) gn_assemble(ctx, c, GnEstimator{ GnEstimator::given, 0, 1.0 }, times ? &gev : nullptr);
	else gn_assemble(ctx, c, GnEstimator(), nullptr);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[1], s));
	if (co.nWo) hipLaunchKernelGGL(k_gn_coalesce<18>, gn_grid(co.nWo, 256), dim3(256), 0, s, co.nWo, c.co.d_wsp, c.co.d_wsi, c.WJ, c.co.Wo);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[2], s));
	if (co.nUo) hipLaunchKernelGGL(k_gn_coalesce<36>, gn_grid(co.nUo, 256), dim3(256), 0, s, co.nUo, c.co.d_usp, c.co.d_usi, c.UJ, c.co.Uo);
	if (times) LSFM_CHECK_HIP(hipEventRecord(ev[3], s));
	if (timing) LSFM_CHECK_HIP(hipStreamSynchronize(s));
	const double tw2 = gn_wall();
	if (given) gn_feature_check(ctx, maps, c); // (before anything is allocated for the caller)
	MapOut G;
	map_new(G.g, x, M, NFG, co.nUo, co.nWo, true);
	lsfm_map& g = G.g;
	std::copy(x->stno, x->stno + c.RS, g.stno); std::copy(x->stVal, x->stVal + c.RS, g.stVal);
	std::copy(co.Ui.begin(), co.Ui.end(), g.Ui); std::copy(co.Uj.begin(), co.Uj.end(), g.Uj);
	std::copy(co.photo.begin(), co.photo.end(), g.photo); std::copy(co.feature.begin(), co.feature.end(), g.feature);
	std::copy(co.FBlock.begin(), co.FBlock.end(), g.FBlock); std::copy(st.origin.begin(), st.origin.end(), g.pose_origin);
	if (g.nU) d2h(ctx, g.U, c.co.Uo, (size_t)g.nU * 36 * sizeof(double));
	if (g.nW) d2h(ctx, g.W, c.co.Wo, (size_t)g.nW * 18 * sizeof(double));
	if (NFG) d2h(ctx, g.V, c.VJ, (size_t)NFG * 9 * sizeof(double));
	if (obj) d2h(ctx, obj, given ? c.d_G : c.Fsum, sizeof(double));
	if (b)
	{
		d2h(ctx, b, c.ea, (size_t)M * 6 * sizeof(double));
		if (NFG) d2h(ctx, b + (size_t)M * 6, c.eb, (size_t)NFG * 3 * sizeof(double));
	}
	LSFM_CHECK_HIP(hipStreamSynchronize(s));
	if (times)
	{
		double* t = times + (given ? 1 : 0);
		for (int i = 0; i < 3; i++) t[i] = event_ms(ev[i], ev[i + 1]);
		if (given) { times[0] = event_ms(gev.chi2[0], gev.fill[1]); t[0] -= times[0]; }
	}
	if (counts) { counts[0] = c.NWJ; counts[1] = co.nWo; counts[2] = c.NUJ; counts[3] = co.nUo; }
	if (timing)
		fprintf(stderr, "lsfm_gn_linearise%s: %d maps, %d poses, %d features, W %d -> %d blocks, U %d -> %d blocks; structure + upload %.2f ms, assembly + coalescing "
		                "%.2f ms, download %.2f ms, call %.2f ms\n", given ? "_features" : "", N, M, NFG, c.NWJ, co.nWo, c.NUJ, co.nUo, tw1 - tw0, tw2 - tw1, gn_wall() - tw2, gn_wall() - tw0);
	G.give(out);
	return LSFM_OK;
}

} // namespace lsfm
