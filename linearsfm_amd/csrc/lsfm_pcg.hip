// K10: the refinement of the camera systems S x = E of one tree level around their Cholesky factor, all independent systems of the
// level stepping together with per-system scalars (PcgSeg).  The factor (lsfm_chol.hip) is that of S itself, so the conjugate
// gradients it preconditions act as iterative refinement: the residual is recomputed as E - S x in every step, and a well-conditioned
// level is done after one step, an ill-conditioned one (a deep monocular tree, condition ~1e10) after a handful.
// The level solve (lsfm_level.hip solve_batch) calls this in two halves, because the first forward substitution rides on the
// factorisation:  pcg_begin (x = x0, r = E - S x)  ->  chol_scatter, chol_perm_in, chol_factor(fwd_v)  ->  pcg_run (first
// preconditioner application, then the steps).  How many steps are enqueued, and when the host asks the device whether every
// system is done, is decided in pcg_run: a first run asks after every step; a run with a plan, or with the count an earlier run
// left as a hint, enqueues that count without asking (ask_after: asks once behind them and goes on step by step if one is missing);
// in a feature-sharded run the ranks agree on every such answer.  Systems that are done are frozen by the device-side test.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "lsfm_device.hpp"
#include "lsfm_pcg.hpp"

namespace lsfm {

struct PcgSeg {
	double rz[2];
	double pAp;
	double rr, ee, thresh, rr_prev;
	int done, its, row0, active;
	int slow, pad; // steps in a row that shrank the true residual by less than half
};
static_assert(sizeof(PcgSeg) % sizeof(double) == 0, "PcgSeg is strided in doubles by the fused dot products");
#define SEG_STRIDE ((int)(sizeof(PcgSeg) / sizeof(double)))

// ---------------------------------------------------------------------------------------------------------------
// CG pieces
// ---------------------------------------------------------------------------------------------------------------
// (also: the product's accumulator y and the level's counters start from zero -- two fills of their own until round 5)
__global__ void k_x_init(int M, const double* __restrict__ x0, const unsigned char* __restrict__ fixed, double* __restrict__ x, double* __restrict__ y, int* __restrict__ misc)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < 4) misc[i] = 0;
	if (i >= (size_t)M * 6) return;
	y[i] = 0.0;
	double v = x0 ? x0[i] : 0.0;
	if (fixed && fixed[i]) v = 0.0;
	x[i] = v;
}

// r = E - y ; rr += r.r ; ee += E.E   (fixed scalars are not part of the system)
// (y is spent afterwards: it is left zeroed for the next product, which adds into it)
__global__ void k_pcg_resid(int M, const double* __restrict__ E, double* __restrict__ y, const int* __restrict__ pose_seg,
                            const unsigned char* __restrict__ fixed, double* __restrict__ r, PcgSeg* seg, int with_ee)
{
	int row = blockIdx.x * blockDim.x + threadIdx.x;
	bool v = row < M;
	double a[2] = { 0, 0 };
	int sg = 0;
	if (v)
	{
		sg = pose_seg[row];
		for (int i = 0; i < 6; i++)
		{
			const size_t o = (size_t)row * 6 + i;
			double e = E[o], d = e - y[o];
			y[o] = 0.0;
			if (fixed && fixed[o]) { e = 0; d = 0; }
			if (r) r[o] = d;
			a[0] += d * d; a[1] += e * e;
		}
		if (seg[sg].done) v = false; // converged systems are frozen
	}
	if (!with_ee) a[1] = 0.0;
	wave_scatter_add<2>(&seg[sg].rr, a, v); // rr, ee are adjacent
}

// p = z, per system: thresholds, convergence state
// (err / run: a non-positive pivot of the factorisation goes to the run's record here, when the level does not stop to read it)
__global__ void k_pcg_start(int nseg, PcgSeg* seg, const unsigned char* __restrict__ active, double rel_tol, int* ndone, const int* __restrict__ err, RunStatsDev* run)
{
	int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s == 0 && run && *err && !run->chol_err) run->chol_err = *err;
	if (s >= nseg) return;
	PcgSeg& g = seg[s];
	g.thresh = rel_tol * rel_tol * g.ee;
	g.pAp = 0; g.rz[1] = 0; g.its = 0;
	g.active = active ? active[s] : 1;
	g.done = (!g.active || !(g.rr > g.thresh)) ? 1 : 0;
	g.rr_prev = g.rr;
	// the record of the system's LAST true residual (seg[nseg + s]: what k_pcg_run_stats and the host's verdict read): the starting
	// point's, until a step's test replaces it (k_pcg_check) -- a system that starts below its bound is never touched again
	seg[nseg + s].rr = g.rr; seg[nseg + s].ee = g.ee;
	g.rr = 0;
	if (g.done) atomicAdd(ndone, 1);
}
__global__ void k_copy(size_t n, const double* __restrict__ a, double* __restrict__ b)
{
	size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) b[i] = a[i];
}

// alpha = rz/pAp ; x += alpha p ; y = 0.  The residual is then RECOMPUTED as E - S x (residual replacement in every
// iteration): with the exact factor as preconditioner CG acts as iterative refinement, and the recursively updated
// residual would hide the attainable accuracy (the camera systems reach condition numbers ~1e9).
__global__ void k_pcg_update1(int M, int cur, const int* __restrict__ pose_seg, double* __restrict__ x, const double* __restrict__ p,
                              double* __restrict__ y, const PcgSeg* __restrict__ seg)
{
	int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= M) return;
	const PcgSeg& g = seg[pose_seg[row]];
	for (int i = 0; i < 6; i++) y[(size_t)row * 6 + i] = 0.0;
	if (g.done) return;
	const double alpha = g.rz[cur] / g.pAp;
	for (int i = 0; i < 6; i++) { const size_t o = (size_t)row * 6 + i; x[o] += alpha * p[o]; }
}

// beta = rz[nxt]/rz[cur] ; p = z + beta p ; Ap = 0 ; per system: convergence test, reset accumulators
__global__ void k_pcg_update2(int M, int cur, const double* __restrict__ z, const int* __restrict__ pose_seg, double* __restrict__ p,
                              double* __restrict__ Ap, PcgSeg* seg, int* ndone)
{
	int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= M) return;
	const int sg = pose_seg[row];
	PcgSeg& g = seg[sg];
	const bool done = g.done;
	const double rzn = g.rz[cur ^ 1], rzc = g.rz[cur];
	for (int i = 0; i < 6; i++) Ap[(size_t)row * 6 + i] = 0.0;
	if (!done)
	{
		const double beta = rzn / rzc;
		for (int i = 0; i < 6; i++) { const size_t o = (size_t)row * 6 + i; p[o] = z[o] + beta * p[o]; }
	}
}
// after the residual is known and before the preconditioner is applied to it: convergence test per system
__global__ void k_pcg_check(int nseg, PcgSeg* seg, int* ndone)
{
	int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg) return;
	PcgSeg& g = seg[s];
	if (g.done) return;
	const double rr = g.rr;
	g.its++;
	seg[nseg + s].rr = rr; // (the true residual r = E - S x of the iterate just formed: frozen systems keep the one they froze with)
	// converged; or the true residual stopped shrinking where a direct solve would leave it too (relative 1e-8: attainable
	// accuracy reached); or -- far above that -- three steps in a row that hardly moved it (a system this badly conditioned is
	// reported: the final check counts it as not converged).  One slow step alone does not end the refinement: the camera
	// systems of a deep monocular tree now and then take a step that gains little and go on to 1e-12 with the next.
	// (ten such steps, not three: the residuals of a CG are not monotone, and the top systems of a 16 384-map monocular tree --
	// conditioned ~1e10, factored with sums whose order changes from run to run -- were given up at 3e-8 in one run out of a
	// dozen where a few more steps take them to 1e-11; a system that ends above 1e-8 is a failure anyway, patience costs the
	// others nothing)
	const bool slow = !(rr < 0.25 * g.rr_prev);
	g.slow = slow ? g.slow + 1 : 0;
	if (!(rr > g.thresh) || !(rr == rr) || (slow && (!(rr > 1e-16 * g.ee) || g.slow >= 10))) { g.done = (rr == rr) ? 1 : 2; atomicAdd(ndone, 1); }
	g.rr_prev = rr;
}
// after update2 (separate launch: update2 reads the scalars of its system from every row): reset the accumulators
__global__ void k_pcg_reset(int nseg, int cur, PcgSeg* seg)
{
	int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg) return;
	PcgSeg& g = seg[s];
	if (g.done) return;
	g.pAp = 0; g.rr = 0; g.rz[cur] = 0; // rz[cur] is the accumulator of the next iteration
}

// (a feature-sharded run forms the final residual once more, for the x every rank ends with: its record starts from zero)
__global__ void k_pcg_final_zero(int nseg, PcgSeg* fin)
{
	int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s < nseg) { fin[s].rr = 0.0; fin[s].ee = 0.0; }
}
// per-system outcome of a level into the run's device accumulators (a warm level does not stop to read them)
__global__ void k_pcg_run_stats(int nseg, const PcgSeg* __restrict__ seg, RunStatsDev* run)
{
	int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= nseg || !seg[g].active) return;
	const PcgSeg& fin = seg[nseg + g];
	const double rel = fin.ee > 0 ? sqrt(fin.rr / fin.ee) : 0.0;
	if (!(rel < 1e-8) || (seg[g].done != 1 && !(rel < 1e-9))) atomicAdd(&run->not_converged, 1);
	// (steps enqueued by a count from an earlier run: a system that had not met its stopping rule when they ran out and is not
	// within two orders of the target either -- the run is repeated asking after every step)
	if (seg[g].done == 0 && !(rel < 1e-10)) atomicAdd(&run->undone, 1);
	// max of non-negative doubles = max of their bit patterns
	atomicMax(reinterpret_cast<unsigned long long*>(&run->max_rel_residual), (unsigned long long)__double_as_longlong(rel == rel ? rel : 1e300));
}
// LSFM_DEBUG_CONV=1: the systems a level leaves above 1e-9, with the state of their refinement
__global__ void k_pcg_debug(int nseg, int M, const PcgSeg* __restrict__ seg)
{
	int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= nseg || !seg[g].active) return;
	const PcgSeg& fin = seg[nseg + g];
	const double rel = fin.ee > 0 ? sqrt(fin.rr / fin.ee) : 0.0;
	if (!(rel < 1e-9))
		printf("[lsfm conv] M=%d nseg=%d system %d: rel %.3e its %d done %d slow %d rr_prev/ee %.3e thresh/ee %.3e ee %.3e pAp %.3e rz %.3e %.3e\n", M, nseg, g, rel, seg[g].its,
		       seg[g].done, seg[g].slow, seg[g].rr_prev / fin.ee, seg[g].thresh / fin.ee, fin.ee, seg[g].pAp, seg[g].rz[0], seg[g].rz[1]);
}

// ---------------------------------------------------------------------------------------------------------------
// host: the refinement, in the two halves the level solve puts around the factorisation
// ---------------------------------------------------------------------------------------------------------------
// CG set-up first: the residual of the starting point is the right-hand side of the first preconditioner application, whose
// forward substitution rides on the factorisation (chol_factor)
PcgWork pcg_begin(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const CholDev& ch)
{
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	const int M = io.M, nseg = io.nseg;
	PcgWork w;
	w.d_misc = sc.alloc<int>(4); // [1] ndone (zeroed by k_x_init)
	std::vector<PcgSeg> hseg(2 * (size_t)nseg); // [nseg, 2 nseg): accumulators of the final residual check
	memset(hseg.data(), 0, sizeof(PcgSeg) * hseg.size());
	for (int g = 0, row = 0; g < nseg; g++) { hseg[g].row0 = hseg[nseg + g].row0 = row; row += io.seg_rows[g]; }
	w.seg = sc.alloc<PcgSeg>(hseg.size());
	h2d(ctx, w.seg, hseg.data(), sizeof(PcgSeg) * hseg.size());
	const size_t nscal = (size_t)M * 6;
	// (feature-sharded run: z is a sum over the ranks when the factorisation is distributed -- it lives in the exchange buffer)
	w.r = sc.alloc<double>(nscal); w.z = ctx->comm ? ctx->comm->alloc<double>(nscal) : sc.alloc<double>(nscal); w.p = sc.alloc<double>(nscal);
	w.Ap = sc.alloc<double>(nscal); w.v = sc.alloc<double>(nscal);
	const unsigned nbe = (unsigned)((nscal + 255) / 256);
	hipLaunchKernelGGL(k_x_init, dim3(std::max(1u, nbe)), dim3(256), 0, s, M, io.x0, io.d_fixed, io.x_pose, w.Ap, w.d_misc);
	launch_spmv(ctx, sy, io.x_pose, w.Ap, io.d_fixed, nullptr, nullptr, nullptr, 1);
	hipLaunchKernelGGL(k_pcg_resid, dim3((M + 127) / 128), dim3(128), 0, s, M, sy.E, w.Ap, io.d_pose_seg, io.d_fixed, w.r, w.seg, 1);
	// (mixed: the factor is applied from its fp32 copy, made after the factorisation; LSFM_NO_FUSED_FWD: the first application too
	// runs the forward substitution of its own, as every later one does)
	static const bool no_fused_fwd = getenv("LSFM_NO_FUSED_FWD") != nullptr;
	w.fused_fwd = !ctx->pcg.mixed && !no_fused_fwd && ch.M > 0;
	return w;
}

// The first preconditioner application, then the steps.  One refinement step: x += alpha p, true residual, convergence test per
// system (converged systems freeze), then the preconditioner for the next step.  A first run reads the number of finished systems
// back after every step; a warm run enqueues the steps the first run needed -- the device-side tests still freeze what is done, and
// whether every system ended below its bound is read once at the end of the whole run.
PcgResult pcg_run(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const CholDev& ch, PcgWork& w, const PcgSteps& steps)
{
	hipStream_t s = ctx->stream;
	const int M = io.M, nseg = io.nseg;
	const size_t nscal = (size_t)M * 6;
	const int nbr = (M + 127) / 128, nbs = (nseg + 127) / 128;
	const unsigned nbe = (unsigned)((nscal + 255) / 256);
	double *x = io.x_pose, *r = w.r, *z = w.z, *p = w.p, *Ap = w.Ap, *v = w.v;
	PcgSeg* seg = w.seg;
	int* d_misc = w.d_misc;
	const bool mixed = ctx->pcg.mixed;
	chol_apply(ctx, ch, r, v, z, io.d_fixed, io.d_pose_seg, &seg[0].rz[0], SEG_STRIDE, w.fused_fwd);
	hipLaunchKernelGGL(k_copy, dim3(nbe), dim3(256), 0, s, nscal, z, p);
	// (Ap is zero again: k_pcg_resid leaves it so)
	// (a non-positive pivot of the factorisation: a feature-sharded run never throws for it in the middle of a pass: the ranks' factorisations are their own, and a rank that left
	// the pass alone would leave its peers in a sum it never joins -- the flags are exchanged at the end of the run)
	const bool err_to_run = steps.deferred || (ctx->comm && ctx->d_run);
	hipLaunchKernelGGL(k_pcg_start, dim3(nbs), dim3(128), 0, s, nseg, seg, io.d_seg_active, ctx->pcg.rel_tol, d_misc + 1, ch.d_err, err_to_run ? ctx->d_run : (RunStatsDev*)nullptr); // (a bad pivot: reported at the end of the run)

	const int maxit = std::max(1, std::min(50, ctx->pcg.max_steps));
	// the step count was recorded with the preconditioner in this precision, for this tolerance, under this cap
	// ... or, in a run that analyses, what an earlier run of the same tree needed at this level (a guess about values, checked at
	// the end of the run like a plan's count)
	const bool hinted = !steps.warm && steps.deferred && io.step_hint > 0 && io.step_hint <= maxit;
	const bool planned_run = hinted || (steps.warm && steps.mixed == mixed && steps.rel_tol == ctx->pcg.rel_tol && steps.its <= maxit);
	// (a run that counts its steps does not stop to ask before the first one either: systems that start below their bound
	// are frozen on the device, the step costs them nothing)
	int its = 0, ndone = 0;
	w.es0 = ctx->pool_event(); w.es1 = ctx->pool_event();
	// (a level that needed two steps or more -- three with the fp32 preconditioner, where two is the rule -- is ill-conditioned enough
	// for its count to vary from run to run -- one synth-16k run in
	// eight asked for one more than the run before and had to be repeated as a whole: such levels get one step of margin; systems
	// that are done are frozen on the device, the extra step costs them the launches only)
	// A hinted level whose caller waits for the device at its end anyway (io.caller_syncs: a Mono level that analyses) needs neither the
	// margin nor the repeat: it enqueues the steps the run before needed, asks ONCE whether every system is done, and goes on asking
	// step by step if not -- one synth-16k analysing run in eight to twenty was repeated as a whole (twice its time) until round 6.
	const bool ask_after = hinted && io.caller_syncs && !ctx->comm;
	const int base_steps = hinted ? io.step_hint : (planned_run ? steps.its : maxit);
	const int planned = (planned_run && !ask_after && base_steps >= (mixed ? 3 : 2)) ? std::min(base_steps + 1, maxit) : base_steps;
	bool counting = planned_run; // (the steps are enqueued without asking)
	// (an extension is for the run that needs ONE step more than the run before -- the counts scatter by one or two; a system that is
	// still not done three steps on has stalled where its true residual stops shrinking, and steps do not cure that: the run is
	// joined again, as before, which does -- the rounding falls differently.  Nor does an extension raise the hint: it would stay
	// raised, and every later run would pay for the one that stalled)
	int cap = maxit;
	while ((counting ? its < planned : (ndone < nseg && its < cap)))
	{
		const int cur = its & 1;
		launch_spmv(ctx, sy, p, Ap, io.d_fixed, p, io.d_pose_seg, &seg[0].pAp, SEG_STRIDE);
		hipLaunchKernelGGL(k_pcg_update1, dim3(nbr), dim3(128), 0, s, M, cur, io.d_pose_seg, x, p, Ap, seg);
		if (!w.es_done) LSFM_REC_T(w.es0, s);
		launch_spmv(ctx, sy, x, Ap, io.d_fixed, nullptr, nullptr, nullptr, 1);
		if (!w.es_done) { LSFM_REC_T(w.es1, s); w.es_done = true; }
		hipLaunchKernelGGL(k_pcg_resid, dim3(nbr), dim3(128), 0, s, M, sy.E, Ap, io.d_pose_seg, io.d_fixed, r, seg, 0);
		// the test comes before the preconditioner: the apply for a residual that already passed would be wasted
		hipLaunchKernelGGL(k_pcg_check, dim3(nbs), dim3(128), 0, s, nseg, seg, d_misc + 1);
		its++;
		if (counting)
		{
			if (its >= planned)
			{
				if (!ask_after) break;
				ndone = d2h_int(ctx, d_misc + 1);
				if (ndone >= nseg || its >= maxit) break;
				counting = false; // (a system needs more than the run before did: from here on like a run without a hint)
				cap = std::min(maxit, planned + 3);
			}
		}
		else
		{
			ctx->mark("cg_enq");
			ndone = d2h_int(ctx, d_misc + 1);
			ctx->mark("cg_sync");
			const int cerr = (its == 1 && !err_to_run) ? d2h_int(ctx, ch.d_err) : 0; // (the stream is drained: this costs no second wait)
			if (cerr) LSFM_FAIL(LSFM_ERR_NOT_SPD, "Schur system is not positive definite (block column " + std::to_string(cerr - 1) + " of the factor)");
			if (ctx->comm && ctx->comm->world > 1)
			{
				// feature-sharded run: whether another step follows must be the same answer on every rank -- the next step holds sums
				// over the ranks when the factorisation is distributed (chol_apply), and the ranks' residuals, taken from floating-point
				// atomic sums, may differ in the last bits: at a threshold one rank would leave the loop for the sum of x while another
				// enters the sums of the preconditioner (advisor, round 4).  Any rank's doubt is everybody's: one 8-byte sum per step,
				// in runs that ask after every step only.
				long long more = ndone >= nseg ? 0 : 1;
				comm_sum_host(ctx, &more, 1);
				if (!more) break;
				ndone = std::min(ndone, nseg - 1); // (a peer goes on: so does this rank -- its finished systems are frozen on the device)
			}
			else if (ndone >= nseg) break;
		}
		chol_apply(ctx, ch, r, v, z, io.d_fixed, io.d_pose_seg, &seg[0].rz[cur ^ 1], SEG_STRIDE);
		hipLaunchKernelGGL(k_pcg_update2, dim3(nbr), dim3(128), 0, s, M, cur, z, io.d_pose_seg, p, Ap, seg, d_misc + 1);
		hipLaunchKernelGGL(k_pcg_reset, dim3(nbs), dim3(128), 0, s, nseg, cur, seg);
	}
	return PcgResult{ its, planned_run };
}

// Every step's test has left the system's last true residual r = E - S x in seg[nseg + g] (k_pcg_start / k_pcg_check): the product
// and the residual kernel that formed it once more behind the loop (until round 6) are gone -- except in a feature-sharded run, whose
// x has just been replaced by rank 0's.  One of the loop's products is timed with HIP events (es0, es1): here, if the loop ran none.
void pcg_final_residual(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, PcgWork& w)
{
	if (!ctx->comm && w.es_done) return;
	hipStream_t s = ctx->stream;
	const int M = io.M, nseg = io.nseg, nbr = (M + 127) / 128, nbs = (nseg + 127) / 128;
	PcgSeg* seg2 = w.seg + nseg;
	if (!w.es_done) LSFM_REC_T(w.es0, s);
	launch_spmv(ctx, sy, io.x_pose, w.Ap, io.d_fixed, nullptr, nullptr, nullptr, 1);
	if (!w.es_done) { LSFM_REC_T(w.es1, s); w.es_done = true; }
	hipLaunchKernelGGL(k_pcg_final_zero, dim3(nbs), dim3(128), 0, s, nseg, seg2);
	hipLaunchKernelGGL(k_pcg_resid, dim3(nbr), dim3(128), 0, s, M, sy.E, w.Ap, io.d_pose_seg, io.d_fixed, (double*)nullptr, seg2, 1);
}

int pcg_read_verdict(lsfm_context* ctx, const SolveIO& io, const PcgWork& w, double* maxrel)
{
	const int nseg = io.nseg;
	std::vector<PcgSeg> hs2(2 * (size_t)nseg);
	d2h(ctx, hs2.data(), w.seg, sizeof(PcgSeg) * 2 * nseg); // synchronises
	int notconv = 0;
	*maxrel = 0;
	for (int g = 0; g < nseg; g++)
	{
		if (!hs2[g].active) continue;
		const PcgSeg& fin = hs2[nseg + g];
		const double rel = fin.ee > 0 ? sqrt(fin.rr / fin.ee) : 0.0;
		*maxrel = std::max(*maxrel, rel);
		// converged = stopped by the tolerance, or stopped by stagnation with a residual a direct solve would also leave
		if (!(rel < 1e-8) || (hs2[g].done != 1 && !(rel < 1e-9))) notconv++;
	}
	return notconv;
}

} // namespace lsfm
