// The refinement of a level's camera systems around their Cholesky factor (lsfm_pcg.hip), in the two halves the level solve
// (lsfm_level.hip solve_batch) puts around the factorisation, and what it reads of the outcome.
#pragma once
#include "lsfm_chol.hpp"

namespace lsfm {

struct PcgSeg; // per-system scalars on the device (lsfm_pcg.hip)

// what pcg_begin leaves for pcg_run and for the level's statistics: device arrays in ctx->scratch
struct PcgWork {
	double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr, *v = nullptr;
	PcgSeg* seg = nullptr; // [2 nseg]: the systems' state; [nseg, 2 nseg): the record of their last true residual
	int* d_misc = nullptr; // [1]: systems that are done
	bool fused_fwd = false; // v is to go through the forward substitution with the factorisation (chol_perm_in, chol_factor's fwd_v)
	hipEvent_t es0 = nullptr, es1 = nullptr; // around one product S x of the refinement (lsfm_stats.spmv_ms)
	bool es_done = false;
};
// how the steps are run: warm -- the level has a plan, whose step count `its` was recorded with the preconditioner in precision
// `mixed` for tolerance `rel_tol`; deferred -- the outcome goes to the run's device record instead of being read here
struct PcgSteps { bool warm, deferred; int its; bool mixed; double rel_tol; };
// steps taken; planned: they were enqueued by a count (the plan's, or the hint of an earlier run) without asking the device
struct PcgResult { int its; bool planned; };

// x = x0, r = E - S x with its norms per system: before the factorisation, whose fused forward substitution takes r
PcgWork pcg_begin(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const CholDev& ch);
// the first preconditioner application and the refinement steps, behind the factorisation
PcgResult pcg_run(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const CholDev& ch, PcgWork& w, const PcgSteps& steps);
// the true residual of the final x once more where the loop's record does not hold it (a feature-sharded run, whose x was just
// replaced by rank 0's) or no product of the loop was timed
void pcg_final_residual(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, PcgWork& w);
// the outcome per system into the run's device record (a level that does not stop to read it); LSFM_DEBUG_CONV: the systems left above 1e-9
__global__ void k_pcg_run_stats(int nseg, const PcgSeg* __restrict__ seg, RunStatsDev* run);
__global__ void k_pcg_debug(int nseg, int M, const PcgSeg* __restrict__ seg);
// ... or read here (synchronises): the number of systems that did not converge, the largest relative residual to *maxrel
int pcg_read_verdict(lsfm_context* ctx, const SolveIO& io, const PcgWork& w, double* maxrel);

} // namespace lsfm
